// ---- grouped top-K for a few queries on a prepared gallery (coot_retrieval_topk_grouped) ----------------------------------------
// groups[j] is the group of gallery row j (a video of a clip gallery); the result is the K best GROUPS of a query, each through its
// best row.  The top-K entry (retrieval.h) is one 64-bit word with a strict total order, so the best row of a group is a plain
// maximum of entries, which does not depend on the order in which rows arrive: it is taken across workgroups with a 64-bit unsigned
// atomic maximum and no tie-breaking protocol.  Element (i, j) is rt_few_kernel's chain, so the scores are the other searches' bits.
//   rt_few_prep_kernel (retrieval_few.hip): the operand table, as in the few-query search.
//   hipMemsetAsync: the table best [M][G] of entries to 0 = unfilled, every call: no state survives in a workspace.
//   rt_grouped_kernel: rt_few_kernel's sweep (one gallery row per thread, the same staging and chain; one generic staging for the
//     three element types) with another tail: the thread of row j packs tk_pack(acc[i], j) per query.  A wave first folds runs of
//     consecutive lanes with one group id into the run's first lane (a segmented maximum by shuffles: a video's clips are usually
//     adjacent rows, and adders on one address are the slow shape of a memory atomic), then the first lanes raise best[i][g] with
//     atomicMax.  The table only grows, so a plain load first skips the atomic when the entry is not ahead of what it reads; a stale
//     read costs one redundant atomic and cannot lose a maximum.  The group id is bounds-checked before the address is formed, masked
//     rows contribute nothing, and a 128-row block that keeps no row is skipped before its first load, as in rt_few_kernel.
//   rt_grouped_select_kernel: workgroup (t, i) folds range t of best[i] into a sorted list of <= K entries (TkFold); one range writes
//     the result, several write lists [M][T][K] that rt_few_merge_kernel merges by rank ((-1, -inf) for the entry 0).
//   rt_grouped_label_kernel: group_out = idx < 0 ? -1 : groups[idx] (after a merge; a single range labels its own result).
// The result depends on neither the sweep's splits (rt_few_splits) nor the table's ranges (rt_grouped_splits).
// rt_grouped_launch_slice (prep + sweep into a table the caller has reset) and grp_plan are shared with the multi-vector search
// (retrieval_multi.hip), which runs a slice per 16 sentences into one table and selects on sums of its columns.
#include "retrieval.h"

namespace coot {
namespace {

constexpr int GRP_RANGE_MIN = 16;  // table entries per range at least: the cap of the ranges is min(ceil(G / 16), GRP_TMAX)
constexpr int GRP_TMAX = 256;      // ranges (lists per query before the merge)
int g_rt_grouped_splits = 0;       // coot_set_option("rt_grouped_splits", n) (tests); 0 = automatic

// grid (S), 128 threads; MQ, GT, NORM, MASKED as in rt_few_kernel; LDS: tile [FR][RP] | qs [RK][16]
// A 16-byte load holds EPL elements, so a chunk of a block is NQ loads per thread: elements sk .. sk + EPL - 1 of the rows sr + RPP q.
template <typename GT, int MQ, bool NORM, bool MASKED>
__global__ __launch_bounds__(FR) void rt_grouped_kernel(const GT* __restrict__ G, const float* __restrict__ gnorm, const float* __restrict__ qn, int M,
                                                        int N, int d, int blocks_per_split, int vec, float* __restrict__ sim,
                                                        const unsigned char* __restrict__ keep, const int* __restrict__ groups, int NG,
                                                        tk_entry_t* best) {
  constexpr int EPL = 16 / (int)sizeof(GT), TPR = RK / EPL, RPP = FR / TPR, NQ = FR / RPP;
  extern __shared__ __attribute__((aligned(16))) char grp_lds[];
  float* tile = (float*)grp_lds;
  float* qs = tile + FR * RP;
  const int tid = threadIdx.x, lane = tid & 63;
  const int nb = (N + FR - 1) / FR, nchunks = (d + RK - 1) / RK;
  const int b0 = blockIdx.x * blocks_per_split, b1 = min(nb, b0 + blocks_per_split);
  const int sr = tid / TPR, sk = (tid % TPR) * EPL;
  for (int b = b0; b < b1; ++b) {
    const int j0 = b * FR, j = j0 + tid;
    bool kept = j < N;
    if constexpr (MASKED) {
      kept = kept && keep[j];
      if (!sim && !__syncthreads_or(kept)) continue;  // (uniform: nothing of this block is touched)
    }
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
    // the tail.  g: this row's group, -1 for a row that contributes nothing (beyond N, masked out, or an id outside [0, NG))
    int g = -1;
    if (kept) {
      g = groups[j];
      if ((unsigned)g >= (unsigned)NG) g = -1;
    }
    const int gp = __shfl_up(g, 1, 64);          // (by every lane, before any branch: a shuffle reads nothing from a lane that is switched off)
    const bool head = lane == 0 || gp != g;      // first lane of a run of one group id
#pragma unroll
    for (int i = 0; i < MQ; ++i) {
      if (i < M) {  // (uniform)
        const float s = acc[i];
        if (sim && j < N) sim[(long)i * N + j] = s;
        tk_entry_t e = g >= 0 ? tk_pack(s, j) : 0ull;
        // segmented maximum: after the step of distance o lane l holds the maximum over the lanes l .. l + 2 o - 1 of its run.  A value is
        // taken only from a lane of the same group, so whatever the layout every lane holds an entry of its own group
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
          const tk_entry_t eo = __shfl_down(e, o, 64);
          const int go = __shfl_down(g, o, 64);
          if (lane + o < 64 && go == g && eo > e) e = eo;
        }
        if (head && g >= 0) {
          tk_entry_t* p = best + (long)i * NG + g;
          if (e > *p) atomicMax(p, e);
        }
      }
    }
  }
}

// grid (T, M), 64 threads: range t of best[i] = the groups [t span, min(NG, (t + 1) span)), folded 64 entries at a time into a sorted
// list of <= K (0 = an empty group: no candidate).  T == 1: group / idx / score of query i; else list t of part [M][T][K].
__global__ __launch_bounds__(64) void rt_grouped_select_kernel(const tk_entry_t* __restrict__ best, const int* __restrict__ groups, int NG, int K, int span,
                                                               int T, tk_entry_t* __restrict__ part, int* __restrict__ group_out,
                                                               int* __restrict__ idx_out, float* __restrict__ score_out) {
  __shared__ tk_entry_t list[TK_MAX];
  __shared__ tk_entry_t cand[64];
  __shared__ int ncand;
  const int lane = threadIdx.x, t = blockIdx.x, i = blockIdx.y;
  const int g0 = t * span, g1 = min(NG, g0 + span);
  const tk_entry_t* row = best + (long)i * NG;
  for (int e = lane; e < K; e += 64) list[e] = 0ull;
  if (lane == 0) ncand = 0;
  int cnt = 0;  // (uniform)
  __syncthreads();
  for (int c0 = g0; c0 < g1; c0 += 64 * GRP_U) {
    tk_entry_t v[GRP_U];
#pragma unroll
    for (int u = 0; u < GRP_U; ++u) {
      const int g = c0 + u * 64 + lane;
      v[u] = g < g1 ? row[g] : 0ull;
    }
#pragma unroll
    for (int u = 0; u < GRP_U; ++u) {
      if (v[u] != 0ull && (cnt < K || v[u] > list[K - 1])) cand[atomicAdd(&ncand, 1)] = v[u];
      __syncthreads();
      const int nc = ncand;
      TkFold f;
      f.read(list, cnt, cand, nc, lane);
      __syncthreads();
      if (nc) {
        f.place(list, K);
        cnt = min(K, cnt + nc);
        if (lane == 0) ncand = 0;
      }
      __syncthreads();
    }
  }
  for (int r = lane; r < K; r += 64) {
    const tk_entry_t e = list[r];
    if (T == 1) {
      const int idx = tk_idx_masked(e);
      idx_out[(long)i * K + r] = idx;
      score_out[(long)i * K + r] = tk_score_masked(e);
      group_out[(long)i * K + r] = idx < 0 ? -1 : groups[idx];
    } else {
      part[((long)i * T + t) * K + r] = e;
    }
  }
}

__global__ __launch_bounds__(256) void rt_grouped_label_kernel(const int* __restrict__ idx, const int* __restrict__ groups, int n, int* __restrict__ group_out) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e < n) group_out[e] = idx[e] < 0 ? -1 : groups[idx[e]];
}

}  // namespace
// the ranges of the table: cap bounds T whatever the option says, and the workspace is sized by it
GrpPlan grp_plan(int NG) {
  GrpPlan p;
  const int most = (NG + GRP_RANGE_MIN - 1) / GRP_RANGE_MIN;
  p.cap = most < GRP_TMAX ? most : GRP_TMAX;
  int T = g_rt_grouped_splits > 0 ? g_rt_grouped_splits : (NG + 255) / 256 < FEW_G ? (NG + 255) / 256 : FEW_G;  // automatic: one merge round
  T = T > p.cap ? p.cap : T;
  p.span = (NG + T - 1) / T; p.T = (NG + p.span - 1) / p.span;
  return p;
}
// prep + sweep of one slice of M <= FEW_MAX queries into a table the caller has reset (the grouped search: its only slice; the
// multi-vector search, retrieval_multi.hip: every 16 sentences)
int rt_grouped_launch_slice(const float* queries, const void* gallery, int gallery_dtype, const float* gallery_norms, const unsigned char* keep,
                            const int32_t* groups, int NG, int M, int N, int d, float* sim, float* qnorm, float* qn, tk_entry_t* best, hipStream_t st) {
  if (int rc = rt_few_launch_prep(queries, M, d, gallery_norms != nullptr, qnorm, qn, st)) return rc;
  const FewPlan p = few_plan(M, N);
  with_elem(gallery_dtype, [&](auto t) {
    using GT = typename decltype(t)::type;
    const int vec = d % (16 / (int)sizeof(GT)) == 0 && ((uintptr_t)gallery & 15) == 0;  // every row starts 16-byte aligned
    with_mq(p.MQ, [&](auto mq) {
      with_bool(gallery_norms != nullptr, keep != nullptr, [&](auto norm, auto masked) {
        hipLaunchKernelGGL((rt_grouped_kernel<GT, decltype(mq)::value, decltype(norm)::value, decltype(masked)::value>), dim3(p.S), dim3(FR),
                           (size_t)(FR * RP + RK * FEW_MAX) * 4, st, (const GT*)gallery, gallery_norms, (const float*)qn, M, N, d, p.blocks, vec, sim, keep,
                           (const int*)groups, NG, best);
      });
    });
  });
  COOT_CHECK_LAUNCH("rt_grouped");
  return 0;
}
namespace {
struct GrpWs { float *qnorm, *qn; tk_entry_t *best, *part_a, *part_b; size_t bytes; };
GrpWs grp_layout(void* base, int M, int d, int K, int NG, int cap) {
  Arena a{(char*)base}; GrpWs w;
  const int dpad = (d + RK - 1) / RK * RK;
  w.qnorm = a.take<float>(FEW_MAX); w.qn = a.take<float>((size_t)dpad * FEW_MAX);
  w.best = a.take<tk_entry_t>((size_t)M * NG);
  w.part_a = a.take<tk_entry_t>(cap > 1 ? (size_t)M * cap * K : 0);
  w.part_b = a.take<tk_entry_t>(cap > FEW_G ? (size_t)M * ((cap + FEW_G - 1) / FEW_G) * K : 0);
  w.bytes = a.off;
  return w;
}

int grouped_search(const char* fn, const float* queries, const void* gallery, int gallery_dtype, const float* gallery_norms, const unsigned char* keep,
                   const int32_t* groups, int NG, int M, int N, int d, int K, int32_t* group_out, int32_t* idx_out, float* score_out, float* sim_out,
                   void* workspace, size_t workspace_bytes, hipStream_t st) {
  COOT_REQUIRE(queries && gallery && groups && group_out && idx_out && score_out && workspace, "%s: null pointer", fn);
  COOT_REQUIRE(M >= 1 && M <= FEW_MAX && N >= 1 && d >= 1, "%s: M = %d (1 .. %d), N = %d, d = %d", fn, M, FEW_MAX, N, d);
  COOT_REQUIRE(K >= 1 && K <= N && K <= TK_MAX, "%s: K = %d is outside 1 .. min(N = %d, %d)", fn, K, N, TK_MAX);
  COOT_REQUIRE(NG >= 1 && NG <= GRP_GMAX, "%s: num_groups = %d is outside 1 .. %d", fn, NG, GRP_GMAX);
  COOT_REQUIRE(((uintptr_t)workspace & 15) == 0, "%s: workspace is not 16-byte aligned", fn);
  const GrpPlan gp = grp_plan(NG);
  const GrpWs w = grp_layout(workspace, M, d, K, NG, gp.cap);
  COOT_REQUIRE(w.bytes <= workspace_bytes, "%s: workspace too small (%zu < %zu)", fn, workspace_bytes, w.bytes);
  if (int rc = check_hip(hipMemsetAsync(w.best, 0, (size_t)M * NG * sizeof(tk_entry_t), st), "rt_grouped table reset")) return rc;
  if (int rc = rt_grouped_launch_slice(queries, gallery, gallery_dtype, gallery_norms, keep, groups, NG, M, N, d, sim_out, w.qnorm, w.qn, w.best, st)) return rc;
  hipLaunchKernelGGL(rt_grouped_select_kernel, dim3(gp.T, M), dim3(64), 0, st, (const tk_entry_t*)w.best, (const int*)groups, NG, K, gp.span, gp.T, w.part_a,
                     (int*)group_out, (int*)idx_out, score_out);
  COOT_CHECK_LAUNCH("rt_grouped_select");
  if (gp.T == 1) return 0;
  if (int rc = rt_few_merge_lists(w.part_a, w.part_b, gp.T, M, K, true, idx_out, score_out, st)) return rc;
  hipLaunchKernelGGL(rt_grouped_label_kernel, dim3((M * K + 255) / 256), dim3(256), 0, st, (const int*)idx_out, (const int*)groups, M * K, (int*)group_out);
  COOT_CHECK_LAUNCH("rt_grouped_label");
  return 0;
}

}  // namespace
void set_rt_grouped_splits(int n) { g_rt_grouped_splits = n; }
int get_rt_grouped_splits() { return g_rt_grouped_splits; }
}  // namespace coot

using namespace coot;

extern "C" {

size_t coot_retrieval_topk_grouped_workspace_bytes(int M, int N, int d, int K, int num_groups) {
  if (M < 1 || N < 1 || d < 1 || K < 1 || num_groups < 1 || num_groups > GRP_GMAX) return 256;
  return grp_layout(nullptr, M, d, K, num_groups, grp_plan(num_groups).cap).bytes + 256;
}

int coot_retrieval_topk_grouped(const float* queries, const void* gallery, int gallery_dtype, const float* gallery_norms, const uint8_t* keep,
                                const int32_t* groups, int num_groups, int M, int N, int d, int K, int32_t* group_out, int32_t* idx_out,
                                float* score_out, float* sim_out, void* workspace, size_t workspace_bytes, coot_stream_t stream) {
  const char* fn = "retrieval_topk_grouped";
  COOT_REQUIRE(gallery_dtype == COOT_GALLERY_F32 || gallery_dtype == COOT_GALLERY_BF16 || gallery_dtype == COOT_GALLERY_F16,
               "%s: gallery_dtype = %d (COOT_GALLERY_F32, COOT_GALLERY_BF16 or COOT_GALLERY_F16)", fn, gallery_dtype);
  return grouped_search(fn, queries, gallery, gallery_dtype, gallery_norms, keep, groups, num_groups, M, N, d, K, group_out, idx_out, score_out, sim_out,
                        workspace, workspace_bytes, (hipStream_t)stream);
}

}  // extern "C"
