// ---- multi-vector top-K on a prepared gallery: a paragraph's sentences against grouped rows (coot_retrieval_topk_multi) ----------
// queries [M][d] are the sentences of P paragraphs, paragraph p the rows [offsets[p], offsets[p + 1]); groups[j] is the group of gallery
// row j (the video of a clip).  The score of a group for a paragraph is the sum, over the paragraph's sentences in order, of the
// sentence's best row in the group (MaxSim, late interaction); the result is the K best groups of every paragraph and, per sentence,
// the row that answered it in each of them.  The intermediate is the grouped search's table best [M][G] of 64-bit entries
// (retrieval_grouped.hip): a maximum under a strict total order, so it depends on no schedule, and neither does anything below.
//   hipMemsetAsync: the whole table to 0 = unfilled, every call: no state survives in a workspace.
//   rt_grouped_launch_slice (retrieval_grouped.hip), per 16 sentences: rt_few_prep_kernel and rt_grouped_kernel, the grouped search's
//     launches, into rows [16 s, 16 s + 16) of the table and of sim.  The scores are the other searches' bits.
//   rt_multi_select_kernel: workgroup (t, p) walks range t of the groups, lanes on consecutive g, GRP_U groups per lane.  Per group it
//     reads best[i][g] for i = offsets[p] .. offsets[p + 1] - 1 in order (every i one coalesced load of 512 bytes per wave and u), and
//     s = s + score from +0: plain fp32 adds in that order (no product: nothing to contract).  A group is a candidate when every entry
//     was filled; candidates are packed tk_pack(s, g) — score descending, then GROUP id descending — and folded into a sorted list
//     of <= K (TkFold), as in rt_grouped_select_kernel.  One range writes group / score; several write lists [P][T][K] that
//     rt_few_merge_lists merges by rank, its idx the group and its score the sum ((-1, -inf) for the entry 0).
//   rt_multi_align_kernel: thread (i, r) finds the paragraph of sentence i by a binary search in offsets and writes the row and score
//     of best[i][group_out[p][r]], (-1, -inf) where the slot is unfilled or no paragraph covers i.
// offsets is device memory that nobody has checked: both kernels clamp a paragraph to i0 = clamp(off[p], 0, M), i1 = clamp(off[p + 1],
// i0, M) before an address is formed, and a group read back from group_out is bounds-checked before it indexes the table.
// The table read, 8 M G bytes, is the only traffic the grouped search does not have.  The ranges are grp_plan's (rt_grouped_splits).
#include "retrieval.h"

namespace coot {
namespace {

constexpr int MULTI_PMAX = 65535;       // paragraphs of a call: the second grid dimension of the selection and the merge
constexpr long MULTI_TABLE_MAX = 1l << 28;  // M x G entries of a call (2 GiB)

// paragraph p as rows of the table, whatever offsets holds
__device__ __forceinline__ void multi_segment(const int* __restrict__ off, int p, int M, int& i0, int& i1) {
  i0 = min(max(off[p], 0), M);
  i1 = min(max(off[p + 1], i0), M);
}

// grid (T, P), 64 threads: the groups [t span, min(NG, (t + 1) span)) for paragraph p, 64 GRP_U groups at a time.
// T == 1: group / score of paragraph p; else list t of part [P][T][K].  An empty paragraph has no candidate: every slot unfilled.
__global__ __launch_bounds__(64) void rt_multi_select_kernel(const tk_entry_t* __restrict__ best, const int* __restrict__ off, int M, int NG, int K, int span,
                                                             int T, tk_entry_t* __restrict__ part, int* __restrict__ group_out,
                                                             float* __restrict__ score_out) {
  __shared__ tk_entry_t list[TK_MAX];
  __shared__ tk_entry_t cand[64];
  __shared__ int ncand;
  const int lane = threadIdx.x, t = blockIdx.x, p = blockIdx.y;
  int i0, i1;
  multi_segment(off, p, M, i0, i1);
  const int g0 = t * span, g1 = min(NG, g0 + span);
  for (int e = lane; e < K; e += 64) list[e] = 0ull;
  if (lane == 0) ncand = 0;
  int cnt = 0;  // (uniform)
  __syncthreads();
  if (i1 > i0) {  // (uniform)
    for (int c0 = g0; c0 < g1; c0 += 64 * GRP_U) {
      float s[GRP_U];
      bool in[GRP_U], ok[GRP_U];
#pragma unroll
      for (int u = 0; u < GRP_U; ++u) {
        s[u] = 0.f;
        in[u] = ok[u] = c0 + u * 64 + lane < g1;
      }
      const tk_entry_t* col = best + (long)i0 * NG + c0 + lane;  // (dereferenced only where in[u])
      for (int i = i0; i < i1; ++i, col += NG) {
        tk_entry_t v[GRP_U];
#pragma unroll
        for (int u = 0; u < GRP_U; ++u) v[u] = in[u] ? col[u * 64] : 0ull;
#pragma unroll
        for (int u = 0; u < GRP_U; ++u) {
          ok[u] = ok[u] && v[u] != 0ull;
          s[u] = s[u] + tk_score(v[u]);  // (of an unfilled entry: a NaN that ok[u] discards)
        }
      }
#pragma unroll
      for (int u = 0; u < GRP_U; ++u) {
        const tk_entry_t v = ok[u] ? tk_pack(s[u], c0 + u * 64 + lane) : 0ull;
        if (v != 0ull && (cnt < K || v > list[K - 1])) cand[atomicAdd(&ncand, 1)] = v;
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
  }
  for (int r = lane; r < K; r += 64) {
    const tk_entry_t e = list[r];
    if (T == 1) {
      group_out[(long)p * K + r] = tk_idx_masked(e);
      score_out[(long)p * K + r] = tk_score_masked(e);
    } else {
      part[((long)p * T + t) * K + r] = e;
    }
  }
}

// one thread per (sentence i, slot r): the paragraph of i is the last p with off[p] <= i (a binary search: offsets that do not
// decrease find the one paragraph that holds i; any others find some p, which is used only if its clamped segment holds i)
__global__ __launch_bounds__(256) void rt_multi_align_kernel(const tk_entry_t* __restrict__ best, const int* __restrict__ off,
                                                             const int* __restrict__ group_out, int P, int M, int NG, int K, int* __restrict__ row_out,
                                                             float* __restrict__ row_score_out) {
  const long e = (long)blockIdx.x * 256 + threadIdx.x;
  if (e >= (long)M * K) return;
  const int i = (int)(e / K), r = (int)(e - (long)i * K);
  int lo = 0, hi = P + 1;  // the first q of [0, P] with off[q] > i, P + 1 if there is none
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (off[mid] > i) hi = mid; else lo = mid + 1;
  }
  const int p = lo - 1;
  tk_entry_t v = 0ull;
  if (p >= 0 && p < P) {
    int i0, i1;
    multi_segment(off, p, M, i0, i1);
    if (i >= i0 && i < i1) {
      const int g = group_out[(long)p * K + r];
      if ((unsigned)g < (unsigned)NG) v = best[(long)i * NG + g];
    }
  }
  row_out[e] = tk_idx_masked(v);
  row_score_out[e] = tk_score_masked(v);
}

struct MultiWs { float *qnorm, *qn; tk_entry_t *best, *part_a, *part_b; size_t bytes; };
MultiWs multi_layout(void* base, int P, int M, int d, int K, int NG, int cap) {
  Arena a{(char*)base}; MultiWs w;
  const int dpad = (d + RK - 1) / RK * RK;
  w.qnorm = a.take<float>(FEW_MAX); w.qn = a.take<float>((size_t)dpad * FEW_MAX);
  w.best = a.take<tk_entry_t>((size_t)M * NG);
  w.part_a = a.take<tk_entry_t>(cap > 1 ? (size_t)P * cap * K : 0);
  w.part_b = a.take<tk_entry_t>(cap > FEW_G ? (size_t)P * ((cap + FEW_G - 1) / FEW_G) * K : 0);
  w.bytes = a.off;
  return w;
}
bool multi_in_range(int P, int M, int N, int d, int K, int NG) {
  return P >= 1 && P <= MULTI_PMAX && M >= 1 && N >= 1 && d >= 1 && K >= 1 && NG >= 1 && NG <= GRP_GMAX && (long)M * NG <= MULTI_TABLE_MAX;
}

}  // namespace
}  // namespace coot

using namespace coot;

extern "C" {

size_t coot_retrieval_topk_multi_workspace_bytes(int P, int M, int N, int d, int K, int num_groups) {
  if (!multi_in_range(P, M, N, d, K, num_groups)) return 256;
  return multi_layout(nullptr, P, M, d, K, num_groups, grp_plan(num_groups).cap).bytes + 256;
}

int coot_retrieval_topk_multi(const float* queries, const void* gallery, int gallery_dtype, const float* gallery_norms, const uint8_t* keep,
                              const int32_t* groups, int num_groups, const int32_t* offsets, int P, int M, int N, int d, int K, int32_t* group_out,
                              float* score_out, int32_t* row_out, float* row_score_out, float* sim_out, void* workspace, size_t workspace_bytes,
                              coot_stream_t stream) {
  const char* fn = "retrieval_topk_multi";
  const int NG = num_groups;
  hipStream_t st = (hipStream_t)stream;
  COOT_REQUIRE(gallery_dtype == COOT_GALLERY_F32 || gallery_dtype == COOT_GALLERY_BF16 || gallery_dtype == COOT_GALLERY_F16,
               "%s: gallery_dtype = %d (COOT_GALLERY_F32, COOT_GALLERY_BF16 or COOT_GALLERY_F16)", fn, gallery_dtype);
  COOT_REQUIRE(queries && gallery && groups && offsets && group_out && score_out && row_out && row_score_out && workspace, "%s: null pointer", fn);
  COOT_REQUIRE(P >= 1 && P <= MULTI_PMAX && M >= 1 && N >= 1 && d >= 1, "%s: P = %d (1 .. %d), M = %d, N = %d, d = %d", fn, P, MULTI_PMAX, M, N, d);
  COOT_REQUIRE(K >= 1 && K <= N && K <= TK_MAX, "%s: K = %d is outside 1 .. min(N = %d, %d)", fn, K, N, TK_MAX);
  COOT_REQUIRE(NG >= 1 && NG <= GRP_GMAX, "%s: num_groups = %d is outside 1 .. %d", fn, NG, GRP_GMAX);
  COOT_REQUIRE((long)M * NG <= MULTI_TABLE_MAX, "%s: a table of M = %d x num_groups = %d entries; at most 2^28 in one call", fn, M, NG);
  COOT_REQUIRE(((uintptr_t)workspace & 15) == 0, "%s: workspace is not 16-byte aligned", fn);
  const GrpPlan gp = grp_plan(NG);
  const MultiWs w = multi_layout(workspace, P, M, d, K, NG, gp.cap);
  COOT_REQUIRE(w.bytes <= workspace_bytes, "%s: workspace too small (%zu < %zu)", fn, workspace_bytes, w.bytes);
  if (int rc = check_hip(hipMemsetAsync(w.best, 0, (size_t)M * NG * sizeof(tk_entry_t), st), "rt_multi table reset")) return rc;
  for (int i = 0; i < M; i += FEW_MAX) {  // the launches of a stream run in order: one operand table for every slice
    if (int rc = rt_grouped_launch_slice(queries + (size_t)i * d, gallery, gallery_dtype, gallery_norms, keep, groups, NG, M - i < FEW_MAX ? M - i : FEW_MAX, N,
                                         d, sim_out ? sim_out + (size_t)i * N : nullptr, w.qnorm, w.qn, w.best + (size_t)i * NG, st))
      return rc;
  }
  hipLaunchKernelGGL(rt_multi_select_kernel, dim3(gp.T, P), dim3(64), 0, st, (const tk_entry_t*)w.best, (const int*)offsets, M, NG, K, gp.span, gp.T, w.part_a,
                     (int*)group_out, score_out);
  COOT_CHECK_LAUNCH("rt_multi_select");
  if (gp.T > 1)
    if (int rc = rt_few_merge_lists(w.part_a, w.part_b, gp.T, P, K, true, group_out, score_out, st)) return rc;
  const long slots = (long)M * K;
  hipLaunchKernelGGL(rt_multi_align_kernel, dim3((unsigned)((slots + 255) / 256)), dim3(256), 0, st, (const tk_entry_t*)w.best, (const int*)offsets,
                     (const int*)group_out, P, M, NG, K, (int*)row_out, row_score_out);
  COOT_CHECK_LAUNCH("rt_multi_align");
  return 0;
}

}  // extern "C"
