// ---- top-K for a few queries on a prepared gallery (coot_retrieval_topk_few) ---------------------------------------------------
// The search as it is used after training: M <= 16 queries against a gallery that stays in HBM, its row norms computed once
// (coot_retrieval_row_norms).  One sweep of the gallery bounds the call, so the 64 x 64 tile (at most 64 workgroups for one row
// tile, 63 of 64 accumulator rows padding at M = 1) is replaced by one gallery row per thread and one accumulator per query;
// element (i, j) is still tile_dot's chain — acc = fmaf(q_ik, g_jk, acc) from +0 over k in order, the zero padding of the last
// chunk of 32 included, operands divided by their row norms at staging — so sim, idx and scores are coot_retrieval_topk's bits.
//   rt_few_prep_kernel: the operand table qn [dpad][16] = q_ik / |q_i| (zeros beyond M and d), the same for every gallery row.
//   rt_few_kernel: workgroup s (128 threads) sweeps a contiguous range of 128-row blocks.  Per chunk of 32 k: the block's
//     128 x 32 floats (coalesced 16-byte loads, divided by the row norm) and the table's 32 x 16 go to LDS, then a thread walks
//     its own row (stride RP: no bank conflict) against broadcast reads of the queries.  The next chunk's global loads are issued
//     before the FMAs and several workgroups share a CU: the loads in flight hide the HBM latency.  Selection as in
//     rt_topk_kernel: a sorted list of <= K entries per query, candidates that beat the K-th entry, folded in by rank (TkFold);
//     the candidate buffer lies over the tile, which is idle then.
//   rt_few_merge_kernel: rt_topk_merge_kernel's merge by rank over <= 32 lists held in LDS, one workgroup of 1 024 threads per (group, query); a
//     round writes entry lists again (782 lists -> 25 -> the result), the last one idx / score.  Unfilled slots (0) rank behind
//     every entry and land on the unfilled slots of the merged list, so short lists (K > rows of a workgroup) pass through.
// A gallery stored in bfloat16 or IEEE half (coot_retrieval_topk_few_h): rt_few_kernel on that element type.  Only the global load
// and the widening at staging differ — 16 bytes are 8 elements, a chunk of a block is 4 loads per thread — and a widened element is
// the fp32 value of the widened copy, so the tile, the chain and everything after it are the fp32 sweep's and so are the bytes.
// One chunk is in flight under the FMAs, as in the fp32 sweep, and it is half the bytes: whether two chunks in flight pay for their
// registers has not been timed.
#include "retrieval.h"

namespace coot {
namespace {

constexpr int FEW_SMAX = 1024;                   // row splits: about four workgroups per CU
constexpr int FEW_MT = 1024;                     // threads of a merge workgroup: the searches are LDS latency, so as many waves as fit
int g_rt_few_splits = 0;                         // coot_set_option("rt_few_splits", n) (tests); 0 = automatic
static_assert(FEW_MAX * FR * 8 <= (FR * RP + RK * FEW_MAX) * 4, "the candidate buffer lies over the staged tile");

// one wave per query slot: the norm of rt_norms_kernel, column i of the table (slots beyond M: zeros)
__global__ __launch_bounds__(64) void rt_few_prep_kernel(const float* q, int M, int d, int dpad, int norm, float* qnorm, float* qn) {
  const int i = blockIdx.x, lane = threadIdx.x;
  if (i >= M) {
    for (int k = lane; k < dpad; k += 64) qn[k * FEW_MAX + i] = 0.f;
    return;
  }
  const float* src = q + (long)i * d;
  const float nrm = norm ? sqrtf(row_sumsq(src, d, lane)) : 1.f;
  if (lane == 0) qnorm[i] = nrm;
  for (int k = lane; k < dpad; k += 64) qn[k * FEW_MAX + i] = k < d ? (norm ? src[k] / nrm : src[k]) : 0.f;
}

size_t few_lds_bytes(int MQ, int K) { return (size_t)(FR * RP + RK * FEW_MAX) * 4 + (size_t)MQ * K * 8 + 2 * FEW_MAX * 4; }

// grid (S); MQ = M rounded up to 1, 2, 4, 8, 16 accumulators; LDS: tile [FR][RP] | qs [RK][16] | list [MQ][K] | cnt | ncand
// GT: the gallery's element type, float, unsigned short (bfloat16) or _Float16
// MASKED (coot_retrieval_topk_few_masked): keep [N] as in rt_topk_kernel, one byte per thread.  Without sim a 128-row block that
// keeps no row is skipped before its first load (no gallery bytes, no FMAs, no fold); the vote is a workgroup reduction.
template <typename GT, int MQ, bool NORM, bool MASKED>
__global__ __launch_bounds__(FR) void rt_few_kernel(const GT* __restrict__ G, const float* __restrict__ gnorm, const float* __restrict__ qn, int M,
                                                    int N, int d, int K, int blocks_per_split, int S, int vec, float* __restrict__ sim,
                                                    tk_entry_t* __restrict__ part, int* __restrict__ idx_out, float* __restrict__ score_out,
                                                    const unsigned char* __restrict__ keep) {
  extern __shared__ __attribute__((aligned(16))) char few_lds[];
  float* tile = (float*)few_lds;
  float* qs = tile + FR * RP;
  tk_entry_t* cand = (tk_entry_t*)few_lds;  // [MQ][FR], between the last FMA of a block and the next block's staging
  tk_entry_t* list = (tk_entry_t*)(qs + RK * FEW_MAX);
  int* cnt = (int*)(list + MQ * K);
  int* ncand = cnt + FEW_MAX;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int nb = (N + FR - 1) / FR, nchunks = (d + RK - 1) / RK;
  const int b0 = blockIdx.x * blocks_per_split, b1 = min(nb, b0 + blocks_per_split);
  if (tid < FEW_MAX) { cnt[tid] = 0; ncand[tid] = 0; }
  for (int e = tid; e < MQ * K; e += FR) list[e] = 0ull;  // 0 = behind every entry: an unfilled slot
  for (int b = b0; b < b1; ++b) {
    const int j0 = b * FR;
    bool kept = true;  // MASKED: the keep flag of this thread's row j0 + tid
    if constexpr (MASKED) {
      kept = j0 + tid < N && keep[j0 + tid];
      if (!sim && !__syncthreads_or(kept)) continue;  // (uniform: nothing of this block is touched)
    }
    float acc[MQ];
    if constexpr (sizeof(GT) == 4) {
      const int sr = tid >> 3, sk = (tid & 7) * 4;  // staging: floats sk .. sk + 3 of the rows sr + 16 q of a chunk
      float rb[8];
      if (NORM) {
#pragma unroll
        for (int q = 0; q < 8; ++q) rb[q] = j0 + sr + 16 * q < N ? gnorm[j0 + sr + 16 * q] : 1.f;
      }
      float4 pf[8], pq;
      // one chunk into registers: 8 x 16 bytes of the gallery and 16 of the table per thread.  No branch: an address beyond N or d
      // is clamped into the gallery and its value is dropped at staging
      auto load = [&](int k0) {
        const int k = k0 + sk;
#pragma unroll
        for (int q = 0; q < 8; ++q) {
          const float* p = G + (long)min(j0 + sr + 16 * q, N - 1) * d;
          if (vec) {
            pf[q] = *(const float4*)(p + (k < d ? k : 0));
          } else {
            pf[q].x = p[min(k, d - 1)]; pf[q].y = p[min(k + 1, d - 1)]; pf[q].z = p[min(k + 2, d - 1)]; pf[q].w = p[min(k + 3, d - 1)];
          }
        }
        pq = *(const float4*)(qn + (long)k0 * FEW_MAX + tid * 4);
      };
#pragma unroll
      for (int i = 0; i < MQ; ++i) acc[i] = 0.f;
      load(0);
      for (int c = 0; c < nchunks; ++c) {
        const int k0 = c * RK;
#pragma unroll
        for (int q = 0; q < 8; ++q) {
          const int r = sr + 16 * q;
          const bool rin = j0 + r < N;
          const float v[4] = {pf[q].x, pf[q].y, pf[q].z, pf[q].w};
#pragma unroll
          for (int e = 0; e < 4; ++e)  // rows beyond N and columns beyond d are zero, as tile_dot stages them
            tile[r * RP + sk + e] = (rin && k0 + sk + e < d) ? (NORM ? v[e] / rb[q] : v[e]) : 0.f;
        }
        *(float4*)(qs + tid * 4) = pq;
        __syncthreads();
        if (c + 1 < nchunks) load(k0 + RK);  // in flight under the FMAs
#pragma unroll 4
        for (int k = 0; k < RK; ++k) {
          const float bv = tile[tid * RP + k];
          float qv[MQ];
          if constexpr (MQ >= 4) {
#pragma unroll
            for (int u = 0; u < MQ / 4; ++u) {
              const float4 t = *(const float4*)(qs + k * FEW_MAX + 4 * u);
              qv[4 * u] = t.x; qv[4 * u + 1] = t.y; qv[4 * u + 2] = t.z; qv[4 * u + 3] = t.w;
            }
          } else if constexpr (MQ == 2) {
            const float2 t = *(const float2*)(qs + k * FEW_MAX);
            qv[0] = t.x; qv[1] = t.y;
          } else {
            qv[0] = qs[k * FEW_MAX];
          }
#pragma unroll
          for (int i = 0; i < MQ; ++i) acc[i] = fmaf(qv[i], bv, acc[i]);
        }
        __syncthreads();
      }
    } else {
      // 16-bit storage: 16 bytes are 8 elements, so a chunk is 4 loads per thread, elements sk .. sk + 7 of the rows sr + 32 q.  The
      // same clamping and the same zeros; an element is widened when it is staged and the fp32 tile is the one above
      const int sr = tid >> 2, sk = (tid & 3) * 8;
      float rb[4];
      if (NORM) {
#pragma unroll
        for (int q = 0; q < 4; ++q) rb[q] = j0 + sr + 32 * q < N ? gnorm[j0 + sr + 32 * q] : 1.f;
      }
      auto load = [&](int k0, uint4 (&pf)[4], float4& pq) {
        const int k = k0 + sk;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const unsigned short* p = (const unsigned short*)(G + (long)min(j0 + sr + 32 * q, N - 1) * d);
          if (vec) {  // d % 8 == 0: k < d leaves 8 elements in the row
            pf[q] = *(const uint4*)(p + (k < d ? k : 0));
          } else {
            unsigned w[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) w[e] = (unsigned)p[min(k + 2 * e, d - 1)] | (unsigned)p[min(k + 2 * e + 1, d - 1)] << 16;
            pf[q] = make_uint4(w[0], w[1], w[2], w[3]);
          }
        }
        pq = *(const float4*)(qn + (long)k0 * FEW_MAX + tid * 4);
      };
      auto stage = [&](int k0, const uint4 (&pf)[4], const float4& pq) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int r = sr + 32 * q;
          const bool rin = j0 + r < N;
          const unsigned w[4] = {pf[q].x, pf[q].y, pf[q].z, pf[q].w};
#pragma unroll
          for (int e = 0; e < 8; ++e) {
            const float v = widen_half<GT>(w[e >> 1], e & 1);
            tile[r * RP + sk + e] = (rin && k0 + sk + e < d) ? (NORM ? v / rb[q] : v) : 0.f;
          }
        }
        *(float4*)(qs + tid * 4) = pq;
      };
#pragma unroll
      for (int i = 0; i < MQ; ++i) acc[i] = 0.f;
      uint4 pf[4];
      float4 pq;
      load(0, pf, pq);
      for (int c = 0; c < nchunks; ++c) {
        stage(c * RK, pf, pq);
        __syncthreads();
        if (c + 1 < nchunks) load((c + 1) * RK, pf, pq);  // in flight under the FMAs
        few_fma_chunk<MQ>(tile, qs, tid, acc);
        __syncthreads();
      }
    }
    const int j = j0 + tid;
    if (j < N) {
#pragma unroll
      for (int i = 0; i < MQ; ++i) {
        if (i < M) {
          const float s = acc[i];
          if (sim) sim[(long)i * N + j] = s;
          if constexpr (MASKED) { if (!kept) continue; }
          const tk_entry_t e = tk_pack(s, j);
          if (cnt[i] < K || e > list[i * K + K - 1]) cand[i * FR + atomicAdd(&ncand[i], 1)] = e;  // <= FR rows of this block per query
        }
      }
    }
    __syncthreads();
    // fold the candidates in, 64 at a time: wave w takes the queries w, w + 2, ... (the same trip count for both waves)
    int maxnc = 0;
#pragma unroll
    for (int i = 0; i < MQ; ++i) maxnc = max(maxnc, ncand[i]);
    for (int c0 = 0; c0 < maxnc; c0 += 64) {
      for (int i0 = 0; i0 < MQ; i0 += FR / 64) {
        const bool on = i0 + wave < MQ;
        const int i = on ? i0 + wave : 0;
        const int nc = on ? min(64, max(0, ncand[i] - c0)) : 0, n = cnt[i];
        tk_entry_t* L = list + i * K;
        TkFold f;
        f.read(L, n, cand + i * FR + c0, nc, lane);
        __syncthreads();
        if (nc) {
          f.place(L, K);
          if (lane == 0) cnt[i] = min(K, n + nc);
        }
      }
      __syncthreads();
    }
    if (maxnc && tid < MQ) ncand[tid] = 0;  // (the next block's chunk loop has barriers before the next candidate)
  }
  __syncthreads();
  for (int e = tid; e < M * K; e += FR) {
    const int i = e / K, r = e - i * K;
    const tk_entry_t v = list[e];
    if (S == 1) {
      idx_out[e] = MASKED ? tk_idx_masked(v) : (int)(unsigned)v;
      score_out[e] = MASKED ? tk_score_masked(v) : tk_score(v);
    } else {
      part[((long)i * S + blockIdx.x) * K + r] = v;
    }
  }
}

// grid (groups, M): the lists [g FEW_G, g FEW_G + ns) of in [M][S][K] -> list g of out [M][S_out][K], or (FINAL, one group) idx / score
// Short and empty lists (MASKED: fewer than K kept rows in a split, or none): rt_topk_merge_kernel's argument holds for every
// group and every round, so all K slots of a merged list are written, the unfilled ones with 0, or (FINAL, MASKED) (-1, -inf).
template <bool FINAL, bool MASKED>
__global__ __launch_bounds__(FEW_MT) void rt_few_merge_kernel(const tk_entry_t* in, int S, int K, tk_entry_t* out, int S_out, int* idx_out,
                                                           float* score_out) {
  extern __shared__ __attribute__((aligned(16))) char few_lds[];
  tk_entry_t* P = (tk_entry_t*)few_lds;  // [ns][K]
  const int tid = threadIdx.x, g = blockIdx.x, q = blockIdx.y;
  const int s0 = g * FEW_G, ns = min(FEW_G, S - s0);
  const tk_entry_t* src = in + ((long)q * S + s0) * K;
  for (int e = tid; e < ns * K; e += FEW_MT) P[e] = src[e];
  __syncthreads();
  for (int e = tid; e < ns * K; e += FEW_MT) {
    const int s = e / K;
    const tk_entry_t v = P[e];
    int rank = e - s * K;
    for (int t = 0; t < ns && rank < K; ++t)
      if (t != s) rank += tk_ahead(P + t * K, K, v);
    if (rank < K) {
      if (FINAL) {  // (unmasked: an unfilled slot is behind all N >= K real entries)
        idx_out[(long)q * K + rank] = MASKED ? tk_idx_masked(v) : (int)(unsigned)v;
        score_out[(long)q * K + rank] = MASKED ? tk_score_masked(v) : tk_score(v);
      } else {
        out[((long)q * S_out + g) * K + rank] = v;
      }
    }
  }
}

}  // namespace
// row splits and the 128-row blocks each one sweeps: every split has at least one block.  cap bounds S whatever the option says:
// the workspace is sized by it, so it does not depend on the option and stops growing with N.
FewPlan few_plan(int M, int N) {
  FewPlan p;
  p.MQ = M <= 1 ? 1 : M <= 2 ? 2 : M <= 4 ? 4 : M <= 8 ? 8 : 16;
  const int nb = (N + FR - 1) / FR;
  p.cap = nb < FEW_SMAX ? nb : FEW_SMAX;
  int S = g_rt_few_splits > 0 ? g_rt_few_splits : p.cap;
  S = S > p.cap ? p.cap : S;
  p.blocks = (nb + S - 1) / S; p.S = (nb + p.blocks - 1) / p.blocks;
  return p;
}
int rt_few_launch_prep(const float* queries, int M, int d, bool norm, float* qnorm, float* qn, hipStream_t st) {
  hipLaunchKernelGGL(rt_few_prep_kernel, dim3(FEW_MAX), dim3(64), 0, st, queries, M, d, (d + RK - 1) / RK * RK, (int)norm, qnorm, qn);
  COOT_CHECK_LAUNCH("rt_few_prep");
  return 0;
}
// merge by rank in rounds of <= FEW_G lists, the two list buffers taking turns
int rt_few_merge_lists(const tk_entry_t* lists, tk_entry_t* spare, int S, int M, int K, bool masked, int32_t* idx_out, float* score_out, hipStream_t st) {
  const tk_entry_t* cur = lists;
  tk_entry_t* nxt = spare;
  while (S > FEW_G) {
    const int So = (S + FEW_G - 1) / FEW_G;
    hipLaunchKernelGGL((rt_few_merge_kernel<false, false>), dim3(So, M), dim3(FEW_MT), (size_t)FEW_G * K * 8, st, cur, S, K, nxt, So, (int*)nullptr, (float*)nullptr);
    COOT_CHECK_LAUNCH("rt_few_merge");
    tk_entry_t* done = nxt; nxt = (tk_entry_t*)cur; cur = done; S = So;
  }
  with_bool(masked, [&](auto mk) {
    hipLaunchKernelGGL((rt_few_merge_kernel<true, decltype(mk)::value>), dim3(1, M), dim3(FEW_MT), (size_t)S * K * 8, st, cur, S, K,
                       (tk_entry_t*)nullptr, 1, (int*)idx_out, score_out);
  });
  COOT_CHECK_LAUNCH("rt_few_merge");
  return 0;
}
namespace {
struct FewWs { float *qnorm, *qn; tk_entry_t *part_a, *part_b; size_t bytes; };
FewWs few_layout(void* base, int M, int d, int K, int cap) {
  Arena a{(char*)base}; FewWs w;
  const int dpad = (d + RK - 1) / RK * RK;
  w.qnorm = a.take<float>(FEW_MAX); w.qn = a.take<float>((size_t)dpad * FEW_MAX);
  w.part_a = a.take<tk_entry_t>(cap > 1 ? (size_t)M * cap * K : 0);
  w.part_b = a.take<tk_entry_t>(cap > FEW_G ? (size_t)M * ((cap + FEW_G - 1) / FEW_G) * K : 0);
  w.bytes = a.off;
  return w;
}

// coot_retrieval_topk_few (GT = float), coot_retrieval_topk_few_h (a 16-bit GT) and coot_retrieval_topk_few_masked (any GT; keep
// == nullptr: the unmasked kernels, launched as the other two launch them): fn names the entry in a refusal
template <typename GT>
int few_search(const char* fn, const float* queries, const GT* gallery, const float* gallery_norms, const unsigned char* keep, int M, int N, int d, int K,
               int32_t* idx_out, float* score_out, float* sim_out, void* workspace, size_t workspace_bytes, hipStream_t st) {
  COOT_REQUIRE(queries && gallery && idx_out && score_out && workspace, "%s: null pointer", fn);
  COOT_REQUIRE(M >= 1 && M <= FEW_MAX && N >= 1 && d >= 1, "%s: M = %d (1 .. %d), N = %d, d = %d", fn, M, FEW_MAX, N, d);
  COOT_REQUIRE(K >= 1 && K <= N && K <= TK_MAX, "%s: K = %d is outside 1 .. min(N = %d, %d)", fn, K, N, TK_MAX);
  COOT_REQUIRE(((uintptr_t)workspace & 15) == 0, "%s: workspace is not 16-byte aligned", fn);
  const FewPlan p = few_plan(M, N);
  const FewWs w = few_layout(workspace, M, d, K, p.cap);
  COOT_REQUIRE(w.bytes <= workspace_bytes, "%s: workspace too small (%zu < %zu)", fn, workspace_bytes, w.bytes);
  if (int rc = rt_few_launch_prep(queries, M, d, gallery_norms != nullptr, w.qnorm, w.qn, st)) return rc;
  const int vec = d % (16 / (int)sizeof(GT)) == 0 && ((uintptr_t)gallery & 15) == 0;  // every row starts 16-byte aligned
  with_mq(p.MQ, [&](auto mq) {
    with_bool(gallery_norms != nullptr, keep != nullptr, [&](auto norm, auto masked) {
      hipLaunchKernelGGL((rt_few_kernel<GT, decltype(mq)::value, decltype(norm)::value, decltype(masked)::value>), dim3(p.S), dim3(FR),
                         few_lds_bytes(decltype(mq)::value, K), st, gallery, gallery_norms, (const float*)w.qn, M, N, d, K, p.blocks, p.S, vec, sim_out,
                         w.part_a, (int*)idx_out, score_out, keep);
    });
  });
  COOT_CHECK_LAUNCH("rt_few");
  if (p.S == 1) return 0;
  return rt_few_merge_lists(w.part_a, w.part_b, p.S, M, K, keep != nullptr, idx_out, score_out, st);
}

}  // namespace
void set_rt_few_splits(int n) { g_rt_few_splits = n; }
int get_rt_few_splits() { return g_rt_few_splits; }
}  // namespace coot

using namespace coot;

extern "C" {

size_t coot_retrieval_topk_few_workspace_bytes(int M, int N, int d, int K) {
  if (M < 1 || N < 1 || d < 1 || K < 1) return 256;
  return few_layout(nullptr, M, d, K, few_plan(M, N).cap).bytes + 256;
}

int coot_retrieval_topk_few(const float* queries, const float* gallery, const float* gallery_norms, int M, int N, int d, int K, int32_t* idx_out,
                            float* score_out, float* sim_out, void* workspace, size_t workspace_bytes, coot_stream_t stream) {
  return few_search("retrieval_topk_few", queries, gallery, gallery_norms, nullptr, M, N, d, K, idx_out, score_out, sim_out, workspace, workspace_bytes,
                    (hipStream_t)stream);
}

int coot_retrieval_topk_few_h(const float* queries, const void* gallery, int gallery_dtype, const float* gallery_norms, int M, int N, int d, int K,
                              int32_t* idx_out, float* score_out, float* sim_out, void* workspace, size_t workspace_bytes, coot_stream_t stream) {
  COOT_REQUIRE(gallery_dtype == COOT_GALLERY_BF16 || gallery_dtype == COOT_GALLERY_F16,
               "retrieval_topk_few_h: gallery_dtype = %d (COOT_GALLERY_BF16 or COOT_GALLERY_F16)", gallery_dtype);
  return with_elem(gallery_dtype, [&](auto t) {
    return few_search("retrieval_topk_few_h", queries, (const typename decltype(t)::type*)gallery, gallery_norms, nullptr, M, N, d, K, idx_out, score_out,
                      sim_out, workspace, workspace_bytes, (hipStream_t)stream);
  });
}

int coot_retrieval_topk_few_masked(const float* queries, const void* gallery, int gallery_dtype, const float* gallery_norms, const uint8_t* keep, int M,
                                   int N, int d, int K, int32_t* idx_out, float* score_out, float* sim_out, void* workspace, size_t workspace_bytes,
                                   coot_stream_t stream) {
  const char* fn = "retrieval_topk_few_masked";
  COOT_REQUIRE(gallery_dtype == COOT_GALLERY_F32 || gallery_dtype == COOT_GALLERY_BF16 || gallery_dtype == COOT_GALLERY_F16,
               "%s: gallery_dtype = %d (COOT_GALLERY_F32, COOT_GALLERY_BF16 or COOT_GALLERY_F16)", fn, gallery_dtype);
  return with_elem(gallery_dtype, [&](auto t) {
    return few_search(fn, queries, (const typename decltype(t)::type*)gallery, gallery_norms, keep, M, N, d, K, idx_out, score_out, sim_out, workspace,
                      workspace_bytes, (hipStream_t)stream);
  });
}

}  // extern "C"
