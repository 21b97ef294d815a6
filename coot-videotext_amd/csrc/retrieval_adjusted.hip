// ---- adjusted top-K for a few queries on a prepared gallery (coot_retrieval_topk_adjusted), and the hubness offsets ---------------
// Every gallery row brings a number that is taken off its similarity before the selection: a(i, j) = s(i, j) - offset[j], one fp32
// subtraction after the chain.  s(i, j) is rt_few_kernel's chain, bit for bit, and the selection is its selection on a: the result of
// query i is compute_retrieval_topk_masked of a's row i and depends on neither the batch-mates of a query nor the sweep's splits.  A
// row with offset +inf scores -inf and is still a row (unlike a masked one); -inf puts it first.
//   rt_few_prep_kernel (retrieval_few.hip): the operand table, as in the few-query search.
//   rt_adjusted_kernel: rt_scoped_kernel's sweep (retrieval_scoped.hip) without the eligibility word and the ids.  Per 128-row block
//     the thread of row j reads keep[j] and offset[j], one coalesced load each; keep gates the row's candidates for every query.
//     Without sim a block in which keep leaves no row is left before its first gallery load (a workgroup vote, uniform).  The offset
//     waits in LDS while the chain runs, so no register carries it under the FMAs and no load stands between the chain and the pack.
//   Lists [M][S][K] and rt_few_merge_kernel (masked) for S > 1, (-1, -inf) for an unfilled slot, as in the masked search.
//   rt_hub_offsets_kernel (coot_retrieval_hub_offsets): the lists of a k-NN join into one offset per row, half the mean score of the
//     row's filled slots, summed in rank order: with the search above, CSLS.
// The workspace of the search is the few-query search's.
#include "retrieval.h"

namespace coot {
namespace {

static_assert(FEW_MAX * FR * 8 <= (FR * RP + RK * FEW_MAX) * 4, "the candidate buffer lies over the staged tile");

size_t adjusted_lds_bytes(int MQ, int K) { return (size_t)(FR * RP + RK * FEW_MAX) * 4 + (size_t)MQ * K * 8 + 2 * FEW_MAX * 4 + FR * 4; }

// grid (S), 128 threads; MQ, GT, NORM as in rt_few_kernel; LDS: tile [FR][RP] | qs [RK][16] | list [MQ][K] | cnt | ncand | offs [FR]
// keep: may be null (no mask); keep and offset are read for j < N only.
template <typename GT, int MQ, bool NORM>
__global__ __launch_bounds__(FR) void rt_adjusted_kernel(const GT* __restrict__ G, const float* __restrict__ gnorm, const float* __restrict__ qn, int M,
                                                         int N, int d, int K, int blocks_per_split, int S, int vec, float* __restrict__ sim,
                                                         tk_entry_t* __restrict__ part, int* __restrict__ idx_out, float* __restrict__ score_out,
                                                         const unsigned char* __restrict__ keep, const float* __restrict__ offset) {
  constexpr int EPL = 16 / (int)sizeof(GT), TPR = RK / EPL, RPP = FR / TPR, NQ = FR / RPP;
  extern __shared__ __attribute__((aligned(16))) char adjusted_lds[];
  float* tile = (float*)adjusted_lds;
  float* qs = tile + FR * RP;
  tk_entry_t* cand = (tk_entry_t*)adjusted_lds;  // [MQ][FR], between the last FMA of a block and the next block's staging
  tk_entry_t* list = (tk_entry_t*)(qs + RK * FEW_MAX);
  int* cnt = (int*)(list + MQ * K);
  int* ncand = cnt + FEW_MAX;
  float* offs = (float*)(ncand + FEW_MAX);
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int nb = (N + FR - 1) / FR, nchunks = (d + RK - 1) / RK;
  const int b0 = blockIdx.x * blocks_per_split, b1 = min(nb, b0 + blocks_per_split);
  const int sr = tid / TPR, sk = (tid % TPR) * EPL;
  if (tid < FEW_MAX) { cnt[tid] = 0; ncand[tid] = 0; }
  for (int e = tid; e < MQ * K; e += FR) list[e] = 0ull;  // 0 = behind every entry: an unfilled slot
  __syncthreads();
  for (int b = b0; b < b1; ++b) {
    const int j0 = b * FR, j = j0 + tid;
    const bool kept = j < N && (!keep || keep[j]);
    if (keep && !sim && !__syncthreads_or(kept)) continue;  // (uniform: nothing of this block is touched)
    const float off = j < N ? offset[j] : 0.f;
    float rb[NQ];
    if (NORM) {
#pragma unroll
      for (int q = 0; q < NQ; ++q) rb[q] = j0 + sr + RPP * q < N ? gnorm[j0 + sr + RPP * q] : 1.f;
    }
    uint4 pf[NQ];
    float4 pq;
    // one chunk into registers.  No branch: an address beyond N or d is clamped into the gallery and its value is dropped at staging
    auto load = [&](int k0) {
      const int k = k0 + sk;
#pragma unroll
      for (int q = 0; q < NQ; ++q) {
        const GT* p = G + (long)min(j0 + sr + RPP * q, N - 1) * d;
        if (vec) {  // d % EPL == 0: k < d leaves EPL elements in the row
          pf[q] = *(const uint4*)(p + (k < d ? k : 0));
        } else if constexpr (sizeof(GT) == 4) {
          const unsigned* u = (const unsigned*)p;
          pf[q] = make_uint4(u[min(k, d - 1)], u[min(k + 1, d - 1)], u[min(k + 2, d - 1)], u[min(k + 3, d - 1)]);
        } else {
          const unsigned short* u = (const unsigned short*)p;
          unsigned w[4];
#pragma unroll
          for (int e = 0; e < 4; ++e) w[e] = (unsigned)u[min(k + 2 * e, d - 1)] | (unsigned)u[min(k + 2 * e + 1, d - 1)] << 16;
          pf[q] = make_uint4(w[0], w[1], w[2], w[3]);
        }
      }
      pq = *(const float4*)(qn + (long)k0 * FEW_MAX + tid * 4);
    };
    float acc[MQ];
#pragma unroll
    for (int i = 0; i < MQ; ++i) acc[i] = 0.f;
    load(0);
    offs[tid] = off;  // (read back by this thread only, behind the chunk loop's barriers)
    for (int c = 0; c < nchunks; ++c) {
      const int k0 = c * RK;
#pragma unroll
      for (int q = 0; q < NQ; ++q) {
        const int r = sr + RPP * q;
        const bool rin = j0 + r < N;
        const unsigned w[4] = {pf[q].x, pf[q].y, pf[q].z, pf[q].w};
#pragma unroll
        for (int e = 0; e < EPL; ++e) {  // rows beyond N and columns beyond d are zero, as tile_dot stages them
          float v;
          if constexpr (sizeof(GT) == 4) v = __uint_as_float(w[e]); else v = widen_half<GT>(w[e >> 1], e & 1);
          tile[r * RP + sk + e] = (rin && k0 + sk + e < d) ? (NORM ? v / rb[q] : v) : 0.f;
        }
      }
      *(float4*)(qs + tid * 4) = pq;
      __syncthreads();
      if (c + 1 < nchunks) load(k0 + RK);  // in flight under the FMAs
      few_fma_chunk<MQ>(tile, qs, tid, acc);
      __syncthreads();
    }
    if (j < N) {
      const float o = offs[tid];
#pragma unroll
      for (int i = 0; i < MQ; ++i) {
        if (i < M) {
          const float s = acc[i];
          if (sim) sim[(long)i * N + j] = s;
          if (!kept) continue;
          const tk_entry_t e = tk_pack(s - o, j);
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
      idx_out[e] = tk_idx_masked(v);
      score_out[e] = tk_score_masked(v);
    } else {
      part[((long)i * S + blockIdx.x) * K + r] = v;
    }
  }
}

// one thread per row of the lists idx / scores [N][K]: c = the slots with idx >= 0 (a prefix, as every search here fills them), the
// sum of their scores in rank order, out = 0.5 * (sum / c), or 0 for a row without a filled slot.  Plain fp32, no reassociation.
__global__ __launch_bounds__(256) void rt_hub_offsets_kernel(const float* __restrict__ scores, const int* __restrict__ idx, int N, int K,
                                                             float* __restrict__ out) {
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j >= N) return;
  const int* ix = idx + (long)j * K;
  const float* sc = scores + (long)j * K;
  int c = 0;
  for (int t = 0; t < K; ++t) c += ix[t] >= 0;
  float acc = 0.f;
  for (int t = 0; t < c; ++t) acc += sc[t];
  out[j] = c ? 0.5f * (acc / (float)c) : 0.f;
}

// the few-query search's workspace (few_layout, retrieval_few.hip), restated: sized by the plan's cap, so not by the split option
struct AdjustedWs { float *qnorm, *qn; tk_entry_t *part_a, *part_b; size_t bytes; };
AdjustedWs adjusted_layout(void* base, int M, int d, int K, int cap) {
  Arena a{(char*)base}; AdjustedWs w;
  const int dpad = (d + RK - 1) / RK * RK;
  w.qnorm = a.take<float>(FEW_MAX); w.qn = a.take<float>((size_t)dpad * FEW_MAX);
  w.part_a = a.take<tk_entry_t>(cap > 1 ? (size_t)M * cap * K : 0);
  w.part_b = a.take<tk_entry_t>(cap > FEW_G ? (size_t)M * ((cap + FEW_G - 1) / FEW_G) * K : 0);
  w.bytes = a.off;
  return w;
}

int adjusted_search(const char* fn, const float* queries, const void* gallery, int gallery_dtype, const float* gallery_norms, const unsigned char* keep,
                    const float* offset, int M, int N, int d, int K, int32_t* idx_out, float* score_out, float* sim_out, void* workspace,
                    size_t workspace_bytes, hipStream_t st) {
  COOT_REQUIRE(queries && gallery && offset && idx_out && score_out && workspace, "%s: null pointer", fn);
  COOT_REQUIRE(M >= 1 && M <= FEW_MAX && N >= 1 && d >= 1, "%s: M = %d (1 .. %d), N = %d, d = %d", fn, M, FEW_MAX, N, d);
  COOT_REQUIRE(K >= 1 && K <= N && K <= TK_MAX, "%s: K = %d is outside 1 .. min(N = %d, %d)", fn, K, N, TK_MAX);
  COOT_REQUIRE(((uintptr_t)workspace & 15) == 0, "%s: workspace is not 16-byte aligned", fn);
  const FewPlan p = few_plan(M, N);
  const AdjustedWs w = adjusted_layout(workspace, M, d, K, p.cap);
  COOT_REQUIRE(w.bytes <= workspace_bytes, "%s: workspace too small (%zu < %zu)", fn, workspace_bytes, w.bytes);
  if (int rc = rt_few_launch_prep(queries, M, d, gallery_norms != nullptr, w.qnorm, w.qn, st)) return rc;
  with_elem(gallery_dtype, [&](auto t) {
    using GT = typename decltype(t)::type;
    const int vec = d % (16 / (int)sizeof(GT)) == 0 && ((uintptr_t)gallery & 15) == 0;  // every row starts 16-byte aligned
    with_mq(p.MQ, [&](auto mq) {
      with_bool(gallery_norms != nullptr, [&](auto norm) {
        hipLaunchKernelGGL((rt_adjusted_kernel<GT, decltype(mq)::value, decltype(norm)::value>), dim3(p.S), dim3(FR),
                           adjusted_lds_bytes(decltype(mq)::value, K), st, (const GT*)gallery, gallery_norms, (const float*)w.qn, M, N, d, K, p.blocks,
                           p.S, vec, sim_out, w.part_a, (int*)idx_out, score_out, keep, offset);
      });
    });
  });
  COOT_CHECK_LAUNCH("rt_adjusted");
  if (p.S == 1) return 0;
  return rt_few_merge_lists(w.part_a, w.part_b, p.S, M, K, true, idx_out, score_out, st);
}

}  // namespace
}  // namespace coot

using namespace coot;

extern "C" {

size_t coot_retrieval_topk_adjusted_workspace_bytes(int M, int N, int d, int K) {
  if (M < 1 || M > FEW_MAX || N < 1 || d < 1 || K < 1 || K > N || K > TK_MAX) return 256;
  return adjusted_layout(nullptr, M, d, K, few_plan(M, N).cap).bytes + 256;
}

int coot_retrieval_topk_adjusted(const float* queries, const void* gallery, int gallery_dtype, const float* gallery_norms, const uint8_t* keep,
                                 const float* offset, int M, int N, int d, int K, int32_t* idx_out, float* score_out, float* sim_out,
                                 void* workspace, size_t workspace_bytes, coot_stream_t stream) {
  const char* fn = "retrieval_topk_adjusted";
  COOT_REQUIRE(gallery_dtype == COOT_GALLERY_F32 || gallery_dtype == COOT_GALLERY_BF16 || gallery_dtype == COOT_GALLERY_F16,
               "%s: gallery_dtype = %d (COOT_GALLERY_F32, COOT_GALLERY_BF16 or COOT_GALLERY_F16)", fn, gallery_dtype);
  return adjusted_search(fn, queries, gallery, gallery_dtype, gallery_norms, keep, offset, M, N, d, K, idx_out, score_out, sim_out, workspace,
                         workspace_bytes, (hipStream_t)stream);
}

int coot_retrieval_hub_offsets(const float* scores, const int32_t* idx, int N, int K, float* out, coot_stream_t stream) {
  const char* fn = "retrieval_hub_offsets";
  COOT_REQUIRE(scores && idx && out, "%s: null pointer", fn);
  COOT_REQUIRE(N >= 1 && K >= 1 && K <= TK_MAX, "%s: N = %d, K = %d (1 .. %d)", fn, N, K, TK_MAX);
  hipLaunchKernelGGL(rt_hub_offsets_kernel, dim3((N + 255) / 256), dim3(256), 0, (hipStream_t)stream, scores, (const int*)idx, N, K, out);
  COOT_CHECK_LAUNCH("rt_hub_offsets");
  return 0;
}

}  // extern "C"
