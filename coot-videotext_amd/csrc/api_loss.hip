// C-ABI, part 2: losses, packing, kernel-level entry points and hardware probes.
#include <string.h>

#include "../../include/coot_hip.h"
#include "attention.h"
#include "common.h"
#include "gemm.h"
#include "loss.h"
#include "pool.h"
#include "rowops.h"

using namespace coot;

#define RUN(x) do { int _rc = (x); if (_rc) return _rc; } while (0)

namespace {
struct Bump {
  char* base; size_t cap; size_t off = 0; bool overflow = false;
  Bump(void* b, size_t c) : base((char*)b), cap(c) {}
  template <typename T> T* get(size_t n) {
    off = (off + 255) & ~(size_t)255;
    char* p = base ? base + off : nullptr;
    off += n * sizeof(T);
    if (base && off > cap) overflow = true;
    return (T*)p;
  }
};
}  // namespace

extern "C" {

int coot_pack_fwd(const float* emb, const int64_t* counts, int B, int Cmax, int D, float* out, uint8_t* mask, int64_t* lens,
                  coot_stream_t stream) {
  return launch_pack_fwd(emb, (const long long*)counts, B, Cmax, D, out, mask, (long long*)lens, (hipStream_t)stream);
}
int coot_pack_bwd(const float* dout, const int64_t* counts, int B, int Cmax, int D, float* demb, coot_stream_t stream) {
  return launch_pack_bwd(dout, (const long long*)counts, B, Cmax, D, demb, (hipStream_t)stream);
}

size_t coot_contrastive_scratch_bytes(int n_high, int n_low, int d_high, int d_low) {
  return contrastive_fused_scratch_bytes(n_high, n_low, d_high, d_low);
}

int coot_contrastive_fwd_bwd(const coot_contrastive_config* cfg, int n_high, int n_low, int d_high, int d_low, const float* vid_emb,
                             const float* par_emb, const float* clip_emb, const float* sent_emb, const float* vid_ctx,
                             const float* par_ctx, float* loss, float* d_vid_emb, float* d_par_emb, float* d_clip_emb,
                             float* d_sent_emb, float* d_vid_ctx, float* d_par_ctx, void* scratch, size_t scratch_bytes,
                             coot_stream_t stream) {
  return coot_contrastive_fwd_bwd_part(cfg, n_high, n_low, d_high, d_low, vid_emb, par_emb, clip_emb, sent_emb, vid_ctx, par_ctx, loss, d_vid_emb,
                                       d_par_emb, d_clip_emb, d_sent_emb, d_vid_ctx, d_par_ctx, scratch, scratch_bytes,
                                       COOT_CONTRASTIVE_GLOBAL | COOT_CONTRASTIVE_LOCAL, stream);
}

int coot_contrastive_fwd_bwd_part(const coot_contrastive_config* cfg, int n_high, int n_low, int d_high, int d_low, const float* vid_emb,
                                  const float* par_emb, const float* clip_emb, const float* sent_emb, const float* vid_ctx,
                                  const float* par_ctx, float* loss, float* d_vid_emb, float* d_par_emb, float* d_clip_emb,
                                  float* d_sent_emb, float* d_vid_ctx, float* d_par_ctx, void* scratch, size_t scratch_bytes, int part,
                                  coot_stream_t stream) {
  hipStream_t st = (hipStream_t)stream;
  COOT_REQUIRE((part & ~3) == 0 && part != 0, "contrastive: part = COOT_CONTRASTIVE_GLOBAL | COOT_CONTRASTIVE_LOCAL");
  COOT_REQUIRE(cfg && vid_emb && par_emb && clip_emb && sent_emb && vid_ctx && par_ctx && loss && scratch, "contrastive: null pointer");
  const bool bwd = d_vid_emb != nullptr;
  COOT_REQUIRE(!bwd || (d_par_emb && d_clip_emb && d_sent_emb && d_vid_ctx && d_par_ctx), "contrastive: gradient pointers must be all set or all null");
  const float* vs[6] = {vid_emb, par_emb, clip_emb, sent_emb, vid_ctx, par_ctx};
  float* dvs[6] = {d_vid_emb, d_par_emb, d_clip_emb, d_sent_emb, d_vid_ctx, d_par_ctx};
  // coot/trainer_retrieval.py:168-182 (note :181 weights the context cluster term with weight_low_internal)
  const float w_pair[3] = {cfg->weight_high, cfg->weight_low, cfg->weight_context};
  const float w_self[3] = {0.5f * cfg->weight_high_internal, 0.5f * cfg->weight_low_internal,
                           cfg->weight_context_internal != 0.f ? 0.5f * cfg->weight_low_internal : 0.f};
  const int pair_mask = ((part & COOT_CONTRASTIVE_GLOBAL) ? 1 : 0) | ((part & COOT_CONTRASTIVE_LOCAL) ? 6 : 0);
  return launch_contrastive_fused(vs, dvs, n_high, n_low, d_high, d_low, w_pair, w_self, cfg->margin, loss, scratch, scratch_bytes, st, nullptr,
                                  nullptr, pair_mask);
}

size_t coot_contrastive_f32_scratch_bytes(int n_high, int n_low, int d_high, int d_low) {
  return contrastive_f32_scratch_bytes(n_high, n_low, d_high, d_low);
}

int coot_contrastive_fwd_bwd_f32(const coot_contrastive_config* cfg, int n_high, int n_low, int d_high, int d_low, const float* vid_emb,
                                 const float* par_emb, const float* clip_emb, const float* sent_emb, const float* vid_ctx,
                                 const float* par_ctx, float* loss, float* d_vid_emb, float* d_par_emb, float* d_clip_emb,
                                 float* d_sent_emb, float* d_vid_ctx, float* d_par_ctx, void* scratch, size_t scratch_bytes,
                                 coot_stream_t stream) {
  COOT_REQUIRE(cfg && vid_emb && par_emb && clip_emb && sent_emb && vid_ctx && par_ctx && loss && scratch, "contrastive_f32: null pointer");
  const bool bwd = d_vid_emb != nullptr;
  COOT_REQUIRE(!bwd || (d_par_emb && d_clip_emb && d_sent_emb && d_vid_ctx && d_par_ctx), "contrastive_f32: gradient pointers must be all set or all null");
  const float* vs[6] = {vid_emb, par_emb, clip_emb, sent_emb, vid_ctx, par_ctx};
  float* dvs[6] = {d_vid_emb, d_par_emb, d_clip_emb, d_sent_emb, d_vid_ctx, d_par_ctx};
  const float w_pair[3] = {cfg->weight_high, cfg->weight_low, cfg->weight_context};
  const float w_self[3] = {0.5f * cfg->weight_high_internal, 0.5f * cfg->weight_low_internal,
                           cfg->weight_context_internal != 0.f ? 0.5f * cfg->weight_low_internal : 0.f};  // (:181, as the fast path)
  return launch_contrastive_f32(vs, dvs, n_high, n_low, d_high, d_low, w_pair, w_self, cfg->margin, loss, scratch, scratch_bytes, (hipStream_t)stream);
}

int coot_contrastive_fwd_bwd_dp(const coot_contrastive_config* cfg, int n_high, int n_low, int d_high, int d_low, const float* const sets[6],
                                const int64_t ld[6], float* loss, float* const d_own[6], int own_high0, int own_high, int own_low0, int own_low,
                                void* scratch, size_t scratch_bytes, coot_stream_t stream) {
  COOT_REQUIRE(cfg && sets && ld && loss && d_own && scratch, "contrastive_dp: null pointer");
  COOT_REQUIRE(own_high0 >= 0 && own_high0 + own_high <= n_high && own_low0 >= 0 && own_low0 + own_low <= n_low, "contrastive_dp: window outside the batch");
  const float w_pair[3] = {cfg->weight_high, cfg->weight_low, cfg->weight_context};
  const float w_self[3] = {0.5f * cfg->weight_high_internal, 0.5f * cfg->weight_low_internal,
                           cfg->weight_context_internal != 0.f ? 0.5f * cfg->weight_low_internal : 0.f};
  long ldv[6];
  for (int i = 0; i < 6; ++i) { COOT_REQUIRE(sets[i] && d_own[i] && ld[i] % 4 == 0, "contrastive_dp: set %d", i); ldv[i] = (long)ld[i]; }
  const int window[4] = {own_high0, own_high, own_low0, own_low};
  return launch_contrastive_fused(sets, d_own, n_high, n_low, d_high, d_low, w_pair, w_self, cfg->margin, loss, scratch, scratch_bytes,
                                  (hipStream_t)stream, ldv, window);
}

int coot_contrastive_fwd_bwd_dp_blocks(const coot_contrastive_config* cfg, int world, int rank, const int64_t* counts_high,
                                       const int64_t* counts_low, int d_high, int d_low, const float* blocks, const int64_t* set_base,
                                       const int64_t ld[6], float* loss, float* const d_own[6], void* scratch, size_t scratch_bytes,
                                       coot_stream_t stream) {
  COOT_REQUIRE(cfg && counts_high && counts_low && blocks && set_base && ld && loss && d_own && scratch, "contrastive_dp_blocks: null pointer");
  COOT_REQUIRE(world >= 1 && world <= CL_MAX_RANKS && rank >= 0 && rank < world, "contrastive_dp_blocks: %d ranks (1 .. %d), rank %d", world,
               CL_MAX_RANKS, rank);
  const float w_pair[3] = {cfg->weight_high, cfg->weight_low, cfg->weight_context};
  const float w_self[3] = {0.5f * cfg->weight_high_internal, 0.5f * cfg->weight_low_internal,
                           cfg->weight_context_internal != 0.f ? 0.5f * cfg->weight_low_internal : 0.f};
  ClBlocks B; B.blocks = blocks; B.world = world;
  long n[2] = {0, 0};
  for (int r = 0; r < world; ++r) {
    COOT_REQUIRE(counts_high[r] >= 0 && counts_low[r] >= 0, "contrastive_dp_blocks: negative row count of rank %d", r);
    B.row0[0][r] = (int)n[0]; B.row0[1][r] = (int)n[1];
    n[0] += counts_high[r]; n[1] += counts_low[r];
    for (int s = 0; s < 6; ++s) { COOT_REQUIRE(set_base[s * world + r] % 4 == 0, "contrastive_dp_blocks: set %d of rank %d is not 16-byte aligned", s, r); B.base[s][r] = (long)set_base[s * world + r]; }
  }
  COOT_REQUIRE(n[0] < (1l << 30) && n[1] < (1l << 30), "contrastive_dp_blocks: batch too large");
  B.row0[0][world] = (int)n[0]; B.row0[1][world] = (int)n[1];
  long ldv[6];
  const float* vs[6];
  const int window[4] = {B.row0[0][rank], (int)counts_high[rank], B.row0[1][rank], (int)counts_low[rank]};
  for (int s = 0; s < 6; ++s) {
    COOT_REQUIRE(d_own[s] && ld[s] % 4 == 0, "contrastive_dp_blocks: set %d", s);
    ldv[s] = (long)ld[s];
    // the window's rows (the only ones read through v[s]: F.normalize backward of this rank's rows) live in this rank's block
    vs[s] = blocks + B.base[s][rank] - (long)window[(s == 2 || s == 3) ? 2 : 0] * ldv[s];
  }
  return launch_contrastive_fused(vs, d_own, (int)n[0], (int)n[1], d_high, d_low, w_pair, w_self, cfg->margin, loss, scratch, scratch_bytes,
                                  (hipStream_t)stream, ldv, window, 7, &B);
}

int coot_cyclecons_fwd_bwd(const float* clip, const float* sent, const int64_t* clip_lens, const int64_t* sent_lens,
                           const int64_t* idx_clip, const int64_t* idx_sent, int B, int Cc, int Cs, int D, float weight,
                           float inv_batch, float* loss, float* rows_clip, float* rows_sent, float* dclip, float* dsent,
                           coot_stream_t stream) {
  CycleArgs a; a.clip = clip; a.sent = sent; a.clip_lens = (const long long*)clip_lens; a.sent_lens = (const long long*)sent_lens;
  a.idx_clip = (const long long*)idx_clip; a.idx_sent = (const long long*)idx_sent; a.B = B; a.Cc = Cc; a.Cs = Cs; a.D = D;
  a.weight = weight; a.inv_batch = inv_batch; a.loss = loss; a.rows_clip = rows_clip; a.rows_sent = rows_sent; a.dclip = dclip; a.dsent = dsent;
  return launch_cyclecons(a, (hipStream_t)stream);
}

// ---- kernel-level entry points -----------------------------------------------------------------------
int coot_gemm_nt(const void* X, int64_t ldx, const void* W, int64_t ldw, int M, int N, int K, const float* bias, int act,
                 const void* residual_bf16, int64_t ldres, void* out, int64_t ldc, int out_f32, coot_stream_t stream) {
  GemmNT g; g.X = (const bf16_t*)X; g.ldx = ldx; g.W = (const bf16_t*)W; g.ldw = ldw; g.M = M; g.N = N; g.K = K;
  g.epi.bias = bias; g.epi.act = act; g.epi.res = (const bf16_t*)residual_bf16; g.epi.ldres = ldres; g.epi.out = out; g.epi.ldc = ldc;
  g.epi.out_f32 = out_f32;
  return launch_gemm_nt(g, (hipStream_t)stream);
}
// tests: the descriptor as the networks fill it (api.hip), dropout threshold and scale by mkdrop's arithmetic
int coot_debug_gemm_nt(const coot_gemm_nt_args* a, coot_stream_t stream) {
  COOT_REQUIRE(a, "debug_gemm_nt: null arguments");
  COOT_REQUIRE(!a->pe || (a->pe_L > 0 && a->pe_L2 > 0), "debug_gemm_nt: pe_L / pe_L2 must be positive");
  COOT_REQUIRE(a->act != 2 || a->aux, "debug_gemm_nt: act 2 needs aux");
  COOT_REQUIRE(!(a->p > 0.f) || a->drop_ld % 2 == 0, "debug_gemm_nt: drop_ld must be even");
  GemmNT g; g.X = (const bf16_t*)a->X; g.ldx = a->ldx; g.W = (const bf16_t*)a->W; g.ldw = a->ldw; g.M = a->M; g.N = a->N; g.K = a->K;
  g.groups = a->groups > 0 ? a->groups : 1; g.zX = a->zX; g.zW = a->zW; g.zOut = a->zOut;
  GemmEpi& e = g.epi;
  e.bias = a->bias; e.act = a->act; e.aux = (const bf16_t*)a->aux; e.ldaux = a->ldaux; e.save_pre = (bf16_t*)a->save_pre; e.ldpre = a->ldpre;
  e.res = (const bf16_t*)a->res; e.ldres = a->ldres; e.colsum = a->colsum;
  if (a->pe) { e.pe = a->pe; e.pe_L = a->pe_L; e.pe_T0 = a->pe_T0; e.pe_L2 = a->pe_L2; }
  if (a->p > 0.f) {
    const double t = (double)a->p * 4294967296.0;
    e.drop_thr = t >= 4294967295.0 ? 4294967295u : (unsigned)t;
    if (e.drop_thr < 65536u) e.drop_thr = 65536u;
    e.drop_inv_keep = (float)(1.0 / (1.0 - (double)(e.drop_thr >> 16) / 65536.0));
    e.drop_seed = a->seed; e.drop_site = a->site; e.drop_ld = a->drop_ld;
  }
  e.out = a->out; e.ldc = a->ldc; e.out_f32 = a->out_f32;
  if (a->part_ws) set_partials_workspace(a->part_ws, a->part_ws_floats);
  const int rc = launch_gemm_nt(g, (hipStream_t)stream);
  if (a->part_ws) set_partials_workspace(nullptr, 0);
  return rc;
}
// tests: the attention descriptor as attention_all (api.hip) fills it, dropout by the networks' own make_drop (rowops.h)
int coot_debug_attn(const coot_attn_args* a, int backward, coot_stream_t stream) {
  COOT_REQUIRE(a, "debug_attn: null arguments");
  COOT_REQUIRE(a->q && a->k && a->v && a->o && a->lse && a->lens, "debug_attn: null pointer");
  COOT_REQUIRE(a->Nseq >= 1 && a->Lq >= 1 && a->Lk >= 1 && a->H >= 1, "debug_attn: Nseq, Lq, Lk, H must be positive");
  COOT_REQUIRE(a->dh == 16 || a->dh == 32 || a->dh == 48 || a->dh == 64, "debug_attn: d_head=%d unsupported (16,32,48,64)", a->dh);
  const int64_t D = (int64_t)a->H * a->dh;
  COOT_REQUIRE(a->ldq % 8 == 0 && a->ldk % 8 == 0 && a->ldv % 8 == 0 && a->ldo % 8 == 0 && a->ldq >= D && a->ldk >= D && a->ldv >= D && a->ldo >= D,
               "debug_attn: strides must be multiples of 8 and at least H * dh");
  COOT_REQUIRE(a->Nseq2 >= 0 && a->p >= 0.f && a->p < 1.f, "debug_attn: Nseq2 >= 0, 0 <= p < 1");
  if (a->Nseq2 > 0 || a->cu) {  // a second segment and packed rows exist in the short kernels only (attention_all splits or refuses the rest)
    COOT_REQUIRE(a->Lq == a->Lk && attn_short_path(a->Lk), "debug_attn: a second segment / packed rows need self-attention on the short kernels");
    COOT_REQUIRE(a->Nseq2 == 0 || (a->lens2 && attn_short_path(a->L2)), "debug_attn: the second segment needs lens2 and a short L2");
  }
  if (backward) {
    COOT_REQUIRE(a->dout && a->delta && a->dq && a->dk && a->dv, "debug_attn: backward: null pointer");
    COOT_REQUIRE(a->lddo % 8 == 0 && a->lddq % 8 == 0 && a->lddk % 8 == 0 && a->lddv % 8 == 0 && a->lddo >= D && a->lddq >= D && a->lddk >= D && a->lddv >= D,
                 "debug_attn: backward: strides must be multiples of 8 and at least H * dh");
  }
  AttnArgs g;
  g.q = (const bf16_t*)a->q; g.ldq = a->ldq; g.k = (const bf16_t*)a->k; g.ldk = a->ldk; g.v = (const bf16_t*)a->v; g.ldv = a->ldv;
  g.o = (bf16_t*)a->o; g.ldo = a->ldo; g.lse = a->lse; g.lens = (const long long*)a->lens;
  g.Nseq = a->Nseq; g.Lq = a->Lq; g.Lk = a->Lk; g.H = a->H; g.dh = a->dh; g.scale = 1.0f / sqrtf((float)a->dh);
  if (a->Nseq2 > 0) { g.Nseq2 = a->Nseq2; g.L2 = a->L2; g.lens2 = (const long long*)a->lens2; g.seed2_delta = kAttnSeed2Delta; }
  g.cu = a->cu;
  g.drop = make_drop(1, a->p, a->seed, a->site, nullptr);
  if (backward) {
    g.dout = (const bf16_t*)a->dout; g.lddo = a->lddo; g.delta = a->delta;
    g.dq = (bf16_t*)a->dq; g.lddq = a->lddq; g.dk = (bf16_t*)a->dk; g.lddk = a->lddk; g.dv = (bf16_t*)a->dv; g.lddv = a->lddv;
  }
  return backward ? launch_attn_bwd(g, (hipStream_t)stream) : launch_attn_fwd(g, (hipStream_t)stream);
}
// tests: the LayerNorm descriptors as the networks fill them (api.hip); part_ws is the launcher's business (set_partials_workspace)
int coot_debug_ln(const coot_ln_args* a, int backward, coot_stream_t stream) {
  COOT_REQUIRE(a, "debug_ln: null arguments");
  COOT_REQUIRE(a->x && a->R >= 0, "debug_ln: null source or negative R");
  COOT_REQUIRE(a->D >= 8 && a->D % 4 == 0 && a->D <= (backward ? 1024 : 4096), "debug_ln: D=%d unsupported (multiple of 4, 8 .. %d)", a->D,
               backward ? 1024 : 4096);
  const int64_t D = a->D;
  COOT_REQUIRE(a->ldx >= D && a->ldx % 4 == 0, "debug_ln: ldx must be a multiple of 4 and at least D");
  COOT_REQUIRE(a->p >= 0.f && a->p < 1.f && a->pm >= 0.f && a->pm < 1.f, "debug_ln: 0 <= p < 1");
  if (!backward) {
    COOT_REQUIRE(a->y || a->y32, "debug_ln: no output");
    COOT_REQUIRE((!a->y || (a->ldy >= D && a->ldy % 4 == 0)) && (!a->y32 || (a->ldy32 >= D && a->ldy32 % 4 == 0)),
                 "debug_ln: output strides must be multiples of 4 and at least D");
    COOT_REQUIRE(!a->gain || a->bias, "debug_ln: gain needs bias");
    COOT_REQUIRE(!a->pe || a->pe_L >= 1, "debug_ln: pe needs pe_L >= 1");
    COOT_REQUIRE(!a->x2 || (a->R0 >= 0 && a->R0 <= a->R), "debug_ln: R0 outside 0 .. R");
    COOT_REQUIRE(!a->cu || (a->nseq >= 1 && (a->src_packed || (a->N0 >= 0 && a->L0 >= 1 && (a->N0 >= a->nseq || (a->x2 && a->L1 >= 1))))),
                 "debug_ln: packed rows need nseq >= 1 and, with a padded source, N0, L0 (and x2, L1 for sequences >= N0)");
    COOT_REQUIRE(a->cu || (!a->pos_out && !a->src_packed), "debug_ln: pos_out / src_packed need cu");
    COOT_REQUIRE(a->max_wgs >= 0, "debug_ln: max_wgs < 0");
    LnFwd l; l.x = a->x; l.x_f32 = a->x_f32 ? 1 : 0; l.ldx = a->ldx; l.x2 = a->x2; l.R0 = a->R0; l.R = a->R; l.D = a->D;
    l.gain = a->gain; l.bias = a->bias; l.pe = a->pe; l.pe_L = a->pe ? a->pe_L : 1;
    l.y = (bf16_t*)a->y; l.ldy = a->ldy; l.y32 = a->y32; l.ldy32 = a->ldy32;
    l.drop = make_drop(1, a->p, a->seed, a->site, nullptr);
    l.cu = a->cu; l.nseq = a->nseq; l.N0 = a->N0; l.L0 = a->L0; l.L1 = a->L1; l.pos_out = a->pos_out; l.src_packed = a->src_packed ? 1 : 0;
    l.max_wgs = a->max_wgs; l.nt = a->nt ? 1 : 0;
    return launch_ln_fwd(l, (hipStream_t)stream);
  }
  COOT_REQUIRE((a->dy || a->dy32) && a->gain, "debug_ln: backward: null pointer");
  COOT_REQUIRE((!a->dy || a->dy32 || (a->lddy >= D && a->lddy % 4 == 0)) && (!a->dy32 || (a->lddy32 >= D && a->lddy32 % 4 == 0)) &&
               (!a->dy_add || (a->lddy_add >= D && a->lddy_add % 4 == 0)), "debug_ln: backward: gradient strides must be multiples of 4 and at least D");
  COOT_REQUIRE((!a->dx || (a->lddx >= D && a->lddx % 4 == 0)) && (!a->dx32 || (a->lddx32 >= D && a->lddx32 % 4 == 0)) &&
               (!a->dxm || (a->lddxm >= D && a->lddxm % 4 == 0)), "debug_ln: backward: output strides must be multiples of 4 and at least D");
  COOT_REQUIRE(!(a->dxm && a->pm > 0.f) || (a->dxm_drop_ld >= D && a->dxm_drop_ld % 2 == 0), "debug_ln: backward: dxm_drop_ld must be even and at least D");
  COOT_REQUIRE(!a->part_ws || a->part_ws_floats > 0, "debug_ln: part_ws without part_ws_floats");
  LnBwd b; b.dy = (const bf16_t*)a->dy; b.lddy = a->lddy; b.dy32 = a->dy32; b.lddy32 = a->lddy32; b.dy_add = (const bf16_t*)a->dy_add; b.lddy_add = a->lddy_add;
  b.x = a->x; b.x_f32 = a->x_f32 ? 1 : 0; b.ldx = a->ldx; b.gain = a->gain; b.R = a->R; b.D = a->D;
  b.dx = (bf16_t*)a->dx; b.lddx = a->lddx; b.dx32 = a->dx32; b.lddx32 = a->lddx32; b.dxm = (bf16_t*)a->dxm; b.lddxm = a->lddxm;
  b.dxm_drop = make_drop(1, a->pm, a->seed_m, a->site_m, nullptr); b.dxm_drop_ld = a->dxm_drop_ld;
  b.dgain = a->dgain; b.dbias = a->dbias; b.dxcolsum = a->dxcolsum;
  b.drop = make_drop(1, a->p, a->seed, a->site, nullptr);
  if (a->part_ws) set_partials_workspace(a->part_ws, a->part_ws_floats);
  const int rc = launch_ln_bwd(b, (hipStream_t)stream);
  if (a->part_ws) set_partials_workspace(nullptr, 0);
  return rc;
}
// tests: one or two GenPool segments as pool_all (api.hip) fills them; defer: the backward's column sum inside a deferred-reduction scope
int coot_debug_pool(const coot_pool_args* segs, int nseg, int backward, float* part_ws, size_t part_ws_floats, int defer, coot_stream_t stream) {
  COOT_REQUIRE(segs, "debug_pool: null arguments");
  COOT_REQUIRE(nseg >= 1 && nseg <= 2, "debug_pool: one or two segments");
  COOT_REQUIRE(!part_ws || part_ws_floats > 0, "debug_pool: part_ws without part_ws_floats");
  COOT_REQUIRE(!defer || (backward && part_ws), "debug_pool: defer needs the backward and a workspace");
  PoolArgs g[2];
  for (int i = 0; i < nseg; ++i) {
    const coot_pool_args& a = segs[i];
    const int64_t D = a.D;
    COOT_REQUIRE(a.s && a.z && a.lens && a.pooled, "debug_pool: null pointer");
    COOT_REQUIRE(a.D >= 64 && a.D <= 512 && a.D % 8 == 0 && a.D == segs[0].D, "debug_pool: D=%d unsupported (multiple of 8, 64 .. 512, the same in both segments)", a.D);
    COOT_REQUIRE(a.N >= 1 && (a.cu || a.L >= 1), "debug_pool: N and L must be positive");
    COOT_REQUIRE(a.lds >= D && a.lds % 8 == 0 && a.ldz >= D && a.ldz % 8 == 0 && a.ldp >= D, "debug_pool: strides must be multiples of 8 (ldp: any) and at least D");
    COOT_REQUIRE(a.p_w >= 0.f && a.p_w < 1.f && a.p_s >= 0.f && a.p_s < 1.f, "debug_pool: 0 <= p < 1");
    COOT_REQUIRE(!a.smax == !a.ssum, "debug_pool: smax and ssum go together");
    if (a.pk_out) COOT_REQUIRE(!backward && a.pk_counts && a.pk_B >= 1 && a.pk_Cmax >= 1, "debug_pool: the hand-over needs pk_counts, pk_B, pk_Cmax (forward only)");
    if (backward) {
      COOT_REQUIRE(a.dpooled && a.ds && a.dz && a.smax && a.ssum, "debug_pool: backward: null pointer");
      COOT_REQUIRE(a.lddp >= D && a.ldds >= D && a.ldds % 8 == 0 && a.lddz >= D && a.lddz % 8 == 0, "debug_pool: backward: strides must be multiples of 8 (lddp: any) and at least D");
      COOT_REQUIRE(!(a.p_s > 0.f) || (a.drop_s_ld >= D && a.drop_s_ld % 2 == 0 && a.drop_s_row0 >= 0), "debug_pool: backward: drop_s_ld must be even and at least D, drop_s_row0 >= 0");
      COOT_REQUIRE(a.ds_colsum == segs[0].ds_colsum, "debug_pool: backward: the segments share ds_colsum");
    }
    PoolArgs& p = g[i];
    p.s = (const bf16_t*)a.s; p.lds = a.lds; p.z = (const bf16_t*)a.z; p.ldz = a.ldz; p.lens = (const long long*)a.lens; p.cu = a.cu;
    p.N = a.N; p.L = a.L; p.D = a.D; p.pooled = a.pooled; p.ldp = a.ldp; p.pooled_copy = a.pooled_copy; p.smax = a.smax; p.ssum = a.ssum;
    p.drop_w = make_drop(1, a.p_w, a.seed_w, a.site_w, nullptr);
    if (backward) {
      p.dpooled = a.dpooled; p.lddp = a.lddp; p.ds = (bf16_t*)a.ds; p.ldds = a.ldds; p.dz = (bf16_t*)a.dz; p.lddz = a.lddz; p.ds_colsum = a.ds_colsum;
      p.drop_s = make_drop(1, a.p_s, a.seed_s, a.site_s, nullptr); p.drop_s_ld = a.drop_s_ld; p.drop_s_row0 = a.drop_s_row0;
    } else if (a.pk_out) {
      p.pk_counts = (const long long*)a.pk_counts; p.pk_B = a.pk_B; p.pk_Cmax = a.pk_Cmax; p.pk_out = a.pk_out; p.pk_mask = a.pk_mask; p.pk_lens = (long long*)a.pk_lens;
    }
  }
  if (part_ws) set_partials_workspace(part_ws, part_ws_floats);
  int rc;
  if (!backward) rc = launch_pool_fwd2(g, nseg, (hipStream_t)stream);
  else if (!defer) rc = launch_pool_bwd2(g, nseg, (hipStream_t)stream);
  else {
    colsum_defer_begin();
    rc = launch_pool_bwd2(g, nseg, (hipStream_t)stream);
    if (!rc) rc = colsum_defer_flush((hipStream_t)stream);
    colsum_defer_end();
  }
  if (part_ws) set_partials_workspace(nullptr, 0);
  return rc;
}
int coot_debug_avgpool(const void* z, int64_t ldz, const int64_t* lens, int N, int L, int D, float* out, int64_t ldo, coot_stream_t stream) {
  COOT_REQUIRE(z && lens && out, "debug_avgpool: null pointer");
  COOT_REQUIRE(N >= 0 && L >= 1 && D >= 2 && D % 2 == 0 && ldz >= D && ldz % 2 == 0 && ldo >= D, "debug_avgpool: D even, ldz even, strides at least D");
  return launch_avgpool_fwd((const bf16_t*)z, ldz, (const long long*)lens, N, L, D, out, ldo, (hipStream_t)stream);
}
int coot_debug_avgpool_bwd(const float* dpooled, int64_t lddp, const int64_t* lens, int N, int L, int D, void* dz, int64_t lddz, coot_stream_t stream) {
  COOT_REQUIRE(dpooled && lens && dz, "debug_avgpool_bwd: null pointer");
  COOT_REQUIRE(N >= 0 && L >= 1 && D >= 2 && D % 2 == 0 && lddz >= D && lddz % 2 == 0 && lddp >= D, "debug_avgpool_bwd: D even, lddz even, strides at least D");
  return launch_avgpool_bwd(dpooled, lddp, (const long long*)lens, N, L, D, (bf16_t*)dz, lddz, (hipStream_t)stream);
}
int coot_debug_pack_bwd_join(const float* dout1, const float* dout2, const float* dctx, const int64_t* counts, int B, int Cmax, int D,
                             float* demb_items, float* demb_ctx, coot_stream_t stream) {
  COOT_REQUIRE(dout1 && counts && demb_items && (!dctx || demb_ctx), "debug_pack_bwd_join: null pointer");
  COOT_REQUIRE(B >= 0 && Cmax >= 1 && D >= 1, "debug_pack_bwd_join: B >= 0, Cmax >= 1, D >= 1");
  return launch_pack_bwd_join(dout1, dout2, dctx, (const long long*)counts, B, Cmax, D, demb_items, demb_ctx, (hipStream_t)stream);
}
int coot_debug_colsum_bf16(const void* x, int64_t ldx, int R, int C, float* out, float* part_ws, size_t part_ws_floats, coot_stream_t stream) {
  COOT_REQUIRE(x && out, "debug_colsum_bf16: null pointer");
  COOT_REQUIRE(R >= 0 && C >= 2 && C % 2 == 0 && ldx >= C && ldx % 2 == 0, "debug_colsum_bf16: C even, ldx even and at least C");
  COOT_REQUIRE(!part_ws || part_ws_floats > 0, "debug_colsum_bf16: part_ws without part_ws_floats");
  if (part_ws) set_partials_workspace(part_ws, part_ws_floats);
  const int rc = launch_colsum_bf16((const bf16_t*)x, ldx, R, C, out, (hipStream_t)stream);
  if (part_ws) set_partials_workspace(nullptr, 0);
  return rc;
}
size_t coot_gemm_tn_workspace_bytes(int T, int Mo, int No) { return gemm_tn_workspace_floats(T, Mo, No, 1) * sizeof(float); }
int coot_gemm_tn(const void* A, int64_t lda, const void* B, int64_t ldb, int T, int Mo, int No, float* C, int64_t ldc,
                 void* workspace, size_t workspace_bytes, coot_stream_t stream) {
  GemmTN t; t.A = (const bf16_t*)A; t.lda = lda; t.B = (const bf16_t*)B; t.ldb = ldb; t.T = T; t.Mo = Mo; t.No = No; t.C = C; t.ldc = ldc;
  t.ws = (float*)workspace; t.ws_floats = workspace_bytes / sizeof(float);
  return launch_gemm_tn(t, (hipStream_t)stream);
}
int coot_gemm_tn_batch(const coot_tn_problem* p, int n, void* workspace, size_t workspace_bytes, uint64_t* stamps, coot_stream_t stream) {
  if (n < 0 || (n > 0 && !p)) { set_error("gemm_tn_batch: bad arguments"); return -1; }
  float* old_ws; size_t old_n;
  get_tn_default_workspace(&old_ws, &old_n);
  set_tn_default_workspace((float*)workspace, workspace_bytes / sizeof(float));
  tn_batch_begin();
  int rc = 0;
  for (int i = 0; i < n && !rc; ++i) {
    GemmTN t; t.A = (const bf16_t*)p[i].A; t.lda = p[i].lda; t.B = (const bf16_t*)p[i].B; t.ldb = p[i].ldb; t.T = p[i].T; t.Mo = p[i].Mo; t.No = p[i].No;
    t.C = p[i].C; t.ldc = p[i].ldc; t.a_colsum = p[i].a_colsum; t.overwrite = p[i].overwrite;
    t.groups = p[i].groups > 0 ? p[i].groups : 1; t.zA = p[i].zA; t.zB = p[i].zB; t.zC = p[i].zC;
    t.stamps = (unsigned long long*)stamps;  // phase stamps: tile (0, 0, 0) of EVERY problem writes them (same slots: use one problem, or read them as "some problem")
    rc = launch_gemm_tn(t, (hipStream_t)stream);
  }
  if (!rc) rc = tn_batch_flush((hipStream_t)stream);
  tn_batch_end();
  set_tn_default_workspace(old_ws, old_n);
  return rc;
}
int coot_debug_tn_xcd_map(int n, const int* gx, const int* gy, const int* groups, const int* splits, int* out_item, int* out_local, int max_blocks) {
  return tn_debug_xcd_map(n, gx, gy, groups, splits, out_item, out_local, max_blocks);
}
int coot_ln_fwd(const float* x, int R, int D, const float* gain, const float* bias, void* y_bf16, float* y_f32, coot_stream_t stream) {
  LnFwd l; l.x = x; l.x_f32 = 1; l.ldx = D; l.R = R; l.D = D; l.gain = gain; l.bias = bias; l.y = (bf16_t*)y_bf16; l.ldy = D; l.y32 = y_f32; l.ldy32 = D;
  return launch_ln_fwd(l, (hipStream_t)stream);
}
int coot_attn_fwd(const void* qkv, int Nseq, int L, int H, int dh, const int64_t* lens, void* out, float* lse, coot_stream_t stream) {
  const int D = H * dh;
  AttnArgs a; a.q = (const bf16_t*)qkv; a.k = a.q + D; a.v = a.q + 2 * D; a.ldq = a.ldk = a.ldv = 3 * D; a.o = (bf16_t*)out; a.ldo = D;
  a.lse = lse; a.lens = (const long long*)lens; a.Nseq = Nseq; a.Lq = L; a.Lk = L; a.H = H; a.dh = dh; a.scale = 1.0f / sqrtf((float)dh);
  return launch_attn_fwd(a, (hipStream_t)stream);
}

}  // extern "C"

// Clock monitor: ONE wave samples (100 MHz real-time counter, shader clock counter) every `interval_ticks` ticks of the former,
// n samples: the shader clock actually delivered while other streams run (power management lowers it under matrix load).
__global__ void clock_monitor_kernel(unsigned long long* out, int n, int interval_ticks) {
  if (threadIdx.x != 0) return;
  unsigned long long next = __builtin_amdgcn_s_memrealtime();
  for (int i = 0; i < n; ++i) {
    unsigned long long rt;
    do { __builtin_amdgcn_s_sleep(8); rt = __builtin_amdgcn_s_memrealtime(); } while (rt < next);
    out[2 * i] = rt;
    out[2 * i + 1] = __builtin_amdgcn_s_memtime();
    next = rt + interval_ticks;
  }
}
extern "C" int coot_debug_clock_monitor(uint64_t* out, int n, int interval_ticks, coot_stream_t stream) {
  hipLaunchKernelGGL(clock_monitor_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, (unsigned long long*)out, n, interval_ticks);
  COOT_CHECK_LAUNCH("clock_monitor");
  return 0;
}

extern "C" int coot_timing_enable(int on) { gemm_timing_enable(on); return 0; }
extern "C" int coot_timing_collect(int only_big_k, double* ms, double* flops, int* launches) {
  int rc = gemm_timing_collect(only_big_k, ms, flops, launches);
  if (rc) set_error("timing_collect: event query failed");
  return rc;
}

// probe: LDS holds tile[r][c] = r*64 + c (16 rows x 64 cols bf16 bit patterns as raw u16);
// lane p of each 16-lane group g supplies the address of row (4*g + (p>>2)), cols (p&3)*4..+3.
__global__ void probe_tr16_kernel(uint16_t* out) {
  __shared__ __attribute__((aligned(16))) uint16_t tile[16 * 64];
  for (int i = threadIdx.x; i < 16 * 64; i += 64) tile[i] = (uint16_t)i;
  __syncthreads();
  const int lane = threadIdx.x, g = lane >> 4, p = lane & 15;
  const uint16_t* addr = &tile[(4 * g + (p >> 2)) * 64 + (p & 3) * 4];
  s16x4_t v = __builtin_amdgcn_ds_read_tr16_b64_v4i16((s16x4_t __attribute__((address_space(3)))*)(addr));
  for (int j = 0; j < 4; ++j) out[lane * 4 + j] = (uint16_t)v[j];
}
extern "C" int coot_probe_tr16(uint16_t* out, coot_stream_t stream) {
  hipLaunchKernelGGL(probe_tr16_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, out);
  COOT_CHECK_LAUNCH("probe_tr16");
  return 0;
}
