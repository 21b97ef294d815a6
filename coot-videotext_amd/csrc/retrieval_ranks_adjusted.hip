// ---- labelled ranking under offsets: M queries, N gallery rows, a number per column and per row (coot_retrieval_ranks_adjusted) ------
// coot_retrieval_ranks_labeled (retrieval_tile.hip) on the adjusted matrix
//   a(i, j) = (s(i, j) - col[j]) - row[i]
// s is the tile_dot chain, bit for bit what coot_retrieval_ranks_labeled writes to sim_out; each subtraction is one fp32 subtraction
// after the chain, the column's first.  An offset that is not given is +0: x - (+0) is x in every bit, so without offsets, and with
// zeros, the results are coot_retrieval_ranks_labeled's.  col is the offset of coot_retrieval_topk_adjusted: with col alone query i
// sits at position ranks_q[i] of its adjusted search.  A column at +inf scores -inf, is still a column and still a valid label.
//   rt_adj_own_kernel: rt_lab_own_kernel with own[i] = (s[i, g] - col[g]) - row[i], g = labels[i], and the integer atomic max of the
//     (own, i) word into best[g].
//   rt_lab_prepare_kernel (retrieval_tile.hip, through rt_launch_lab_prepare): ranks = 0 or -1, n_valid.
//   rt_adj_rank_kernel: rt_lab_rank_kernel's counting on a.  Offsets, like labels and thresholds, are loaded after the accumulation:
//     no register carries them under the FMAs.
//   rt_metrics_kernel<true> (retrieval_tile.hip, through rt_launch_lab_metrics).
// The staging is this file's own (adj_tile_dot: acc = 0, one fmaf per k in k order, chunks of 32 with zero padding, x / norm(row)
// staged): shared with retrieval_tile.hip, tile_dot's other callers would be optimised with these kernels in view and compile to other
// instructions (tools/kernel_isa.py).  Integer atomics only, no split k: nothing depends on the workgroup schedule.
#include "retrieval.h"

namespace coot {
namespace {

// tile_dot of retrieval_tile.hip for fp32 operands, statement for statement: one 64 x 64 tile, thread (ty, tx) of a 16 x 16 grid owns
// rows 4 ty .., columns 4 tx ..
struct AdjTile { float acc[4][4]; };
template <bool NORM>
__device__ __forceinline__ void adj_tile_dot(const float* A, const float* B, int NA, int NB, int d, int i0, int j0, float (*As)[RP], float (*Bs)[RP],
                                             AdjTile& t, const float* nA, const float* nB) {
  const int tid = threadIdx.x, ty = tid >> 4, tx = tid & 15;
  float ra[8], rb[8];  // NORM: the norms of the 8 rows of each operand this thread stages (the same rows in every chunk)
  if (NORM) {
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      const int r = (tid >> 5) + 8 * q;
      ra[q] = i0 + r < NA ? nA[i0 + r] : 1.f;
      rb[q] = j0 + r < NB ? nB[j0 + r] : 1.f;
    }
  }
#pragma unroll
  for (int r = 0; r < 4; ++r)
#pragma unroll
    for (int c = 0; c < 4; ++c) t.acc[r][c] = 0.f;
  for (int k0 = 0; k0 < d; k0 += RK) {
    // stage 64 x 32 of each operand: 2048 floats each, 8 per thread; rows beyond N and columns beyond d are zero
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      const int e = tid + 256 * q, r = e >> 5, k = e & 31;
      const bool kin = k0 + k < d;
      if (NORM) {
        As[r][k] = (kin && i0 + r < NA) ? A[(long)(i0 + r) * d + k0 + k] / ra[q] : 0.f;
        Bs[r][k] = (kin && j0 + r < NB) ? B[(long)(j0 + r) * d + k0 + k] / rb[q] : 0.f;
      } else {
        As[r][k] = (kin && i0 + r < NA) ? A[(long)(i0 + r) * d + k0 + k] : 0.f;
        Bs[r][k] = (kin && j0 + r < NB) ? B[(long)(j0 + r) * d + k0 + k] : 0.f;
      }
    }
    __syncthreads();
#pragma unroll 8
    for (int k = 0; k < RK; ++k) {
      float av[4], bv[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) av[r] = As[4 * ty + r][k];
#pragma unroll
      for (int c = 0; c < 4; ++c) bv[c] = Bs[4 * tx + c][k];
#pragma unroll
      for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int c = 0; c < 4; ++c) t.acc[r][c] = fmaf(av[r], bv[c], t.acc[r][c]);
    }
    __syncthreads();
  }
}

// own[i] = a[i, labels[i]] by the chain of adj_tile_dot (64 queries per workgroup, the operands staged as there, gallery rows gathered;
// one thread per query walks k, zero padding of the last chunk included: the accumulators' bits), and an integer atomic max of the
// (own, i) word into best[g].  best = 0: no valid query.  col, row: may be null.
template <bool NORM>
__global__ __launch_bounds__(256) void rt_adj_own_kernel(const float* A, const float* B, const int* labels, const float* nA, const float* nB,
                                                         const float* col, const float* row, int M, int N, int d, float* own, tk_entry_t* best) {
  __shared__ float As[RT][RP], Bs[RT][RP];
  __shared__ int lab[RT];
  const int tid = threadIdx.x, i0 = blockIdx.x * RT;
  if (tid < RT) {
    const int g = i0 + tid < M ? labels[i0 + tid] : -1;
    lab[tid] = (unsigned)g < (unsigned)N ? g : -1;  // -1: no ground truth (or no such query): staged as zeros, nothing written
  }
  __syncthreads();
  int gq[8];  // the gallery rows of the 8 queries this thread stages (the same rows in every chunk)
  float ra[8], rb[8];
#pragma unroll
  for (int q = 0; q < 8; ++q) {
    const int r = (tid >> 5) + 8 * q;
    gq[q] = lab[r];
    ra[q] = NORM && gq[q] >= 0 ? nA[i0 + r] : 1.f;
    rb[q] = NORM && gq[q] >= 0 ? nB[gq[q]] : 1.f;
  }
  float acc = 0.f;
  for (int k0 = 0; k0 < d; k0 += RK) {
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      const int e = tid + 256 * q, r = e >> 5, k = e & 31;
      const bool in = k0 + k < d && gq[q] >= 0;
      if (NORM) {
        As[r][k] = in ? A[(long)(i0 + r) * d + k0 + k] / ra[q] : 0.f;
        Bs[r][k] = in ? B[(long)gq[q] * d + k0 + k] / rb[q] : 0.f;
      } else {
        As[r][k] = in ? A[(long)(i0 + r) * d + k0 + k] : 0.f;
        Bs[r][k] = in ? B[(long)gq[q] * d + k0 + k] : 0.f;
      }
    }
    __syncthreads();
    if (tid < RT) {
#pragma unroll 8
      for (int k = 0; k < RK; ++k) acc = fmaf(As[tid][k], Bs[tid][k], acc);
    }
    __syncthreads();
  }
  if (tid < RT && lab[tid] >= 0) {
    const float co = col ? col[lab[tid]] : 0.f, ro = row ? row[i0 + tid] : 0.f;
    const float a = (acc - co) - ro;
    own[i0 + tid] = a;
    atomicMax(best + lab[tid], tk_pack(a, i0 + tid));
  }
}

// every tile of a: grid (column tiles, row tiles); row counts -> ranks_q, column counts -> ranks_g; sim holds the raw s
// (waves_per_eu: rt_lab_rank_kernel's occupancy, four waves per SIMD)
template <bool NORM>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(4, 4))) void rt_adj_rank_kernel(const float* A, const float* B, const int* labels, const float* nA, const float* nB,
                                                          const float* col, const float* row, int M, int N, int d, const float* own,
                                                          const tk_entry_t* best, float* sim, int* ranks_q, int* ranks_g) {
  __shared__ float As[RT][RP], Bs[RT][RP];
  __shared__ int rowc[RT], colc[RT];
  const int i0 = blockIdx.y * RT, j0 = blockIdx.x * RT;
  const int tid = threadIdx.x, ty = tid >> 4, tx = tid & 15;
  if (tid < RT) { rowc[tid] = 0; colc[tid] = 0; }
  AdjTile t;
  adj_tile_dot<NORM>(A, B, M, N, d, i0, j0, As, Bs, t, nA, nB);  // ends with a barrier: the counters are zeroed
  float di[4], tj[4], ro[4], co[4];
  int gi[4], aj[4];  // gi: the row's label, -1 = none;  aj: the column's best positive query, -1 = none
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int i = i0 + 4 * ty + r, g = i < M ? labels[i] : -1;
    gi[r] = (unsigned)g < (unsigned)N ? g : -1;
    di[r] = gi[r] >= 0 ? own[i] : 0.f;
    ro[r] = row && i < M ? row[i] : 0.f;
  }
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    const int j = j0 + 4 * tx + c;
    const tk_entry_t e = j < N ? best[j] : 0ull;
    aj[c] = e ? (int)(unsigned)e : -1;
    tj[c] = tk_score(e);
    co[c] = col && j < N ? col[j] : 0.f;
  }
  int rc[4] = {0, 0, 0, 0}, cc[4] = {0, 0, 0, 0};
#pragma unroll
  for (int r = 0; r < 4; ++r)
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const int i = i0 + 4 * ty + r, j = j0 + 4 * tx + c;
      if (i < M && j < N) {
        const float s = t.acc[r][c];
        if (sim) sim[(long)i * N + j] = s;
        const float a = (s - co[c]) - ro[r];
        // row i: is j ahead of the label's column?   column j: is i ahead of the column's best positive?
        if (gi[r] >= 0 && j != gi[r] && (a > di[r] || (a == di[r] && j > gi[r]))) ++rc[r];
        if (aj[c] >= 0 && (a > tj[c] || (a == tj[c] && i > aj[c]))) ++cc[c];
      }
    }
#pragma unroll
  for (int r = 0; r < 4; ++r) if (rc[r]) atomicAdd(&rowc[4 * ty + r], rc[r]);
#pragma unroll
  for (int c = 0; c < 4; ++c) if (cc[c]) atomicAdd(&colc[4 * tx + c], cc[c]);
  __syncthreads();
  if (tid < RT) {
    if (i0 + tid < M && rowc[tid]) atomicAdd(ranks_q + i0 + tid, rowc[tid]);
    if (j0 + tid < N && colc[tid]) atomicAdd(ranks_g + j0 + tid, colc[tid]);
  }
}

// coot_retrieval_ranks_labeled's layout (lab_layout, retrieval_tile.hip), restated; best and hist are adjacent: one zero fill
struct AdjRanksWs { float *na, *nb, *own; tk_entry_t* best; int* hist; size_t zero_bytes, bytes; };
AdjRanksWs adj_ranks_layout(void* base, int M, int N) {
  Arena a{(char*)base}; AdjRanksWs w;
  w.na = a.take<float>(M); w.nb = a.take<float>(N); w.own = a.take<float>(M);
  const size_t z0 = a.off;
  w.best = a.take<tk_entry_t>(N);
  w.hist = a.take<int>((size_t)N + M);
  w.zero_bytes = a.off - z0;
  w.bytes = a.off;
  return w;
}

}  // namespace
}  // namespace coot

using namespace coot;

extern "C" {

size_t coot_retrieval_ranks_adjusted_workspace_bytes(int M, int N, int d) {
  (void)d;  // no normalised copy is kept: the norms only
  if (M < 1 || N < 1) return 0;
  return adj_ranks_layout(nullptr, M, N).bytes;  // exact: the call refuses one byte less
}

int coot_retrieval_ranks_adjusted(const float* queries, const float* gallery, const int32_t* labels, const float* row_offset, const float* col_offset,
                                  int M, int N, int d, int normalize, int32_t* ranks_q, int32_t* ranks_g, int32_t* n_valid, float* metrics,
                                  float* sim_out, void* workspace, size_t workspace_bytes, coot_stream_t stream) {
  COOT_REQUIRE(queries && gallery && labels && ranks_q && ranks_g && n_valid && workspace, "retrieval_ranks_adjusted: null pointer");
  COOT_REQUIRE(M >= 1 && N >= 1 && d >= 1 && (M + RT - 1) / RT <= 65535, "retrieval_ranks_adjusted: M = %d, N = %d, d = %d", M, N, d);
  COOT_REQUIRE(((uintptr_t)workspace & 7) == 0, "retrieval_ranks_adjusted: workspace is not 8-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  AdjRanksWs w = adj_ranks_layout(workspace, M, N);
  COOT_REQUIRE(w.bytes <= workspace_bytes, "retrieval_ranks_adjusted: workspace too small (%zu < %zu)", workspace_bytes, w.bytes);
  const int mt = (M + RT - 1) / RT, nt = (N + RT - 1) / RT;
  const int* lab = (const int*)labels;
  if (int rc = check_hip(hipMemsetAsync(w.best, 0, w.zero_bytes, st), "memset best, hist")) return rc;
  const float *na = normalize ? w.na : nullptr, *nb = normalize ? w.nb : nullptr;  // the instantiations without NORM get no norms
  if (normalize) {
    rt_launch_norms(queries, M, gallery, N, d, w.na, w.nb, st);
    COOT_CHECK_LAUNCH("rt_norms");
  }
  with_bool(normalize, [&](auto norm) {
    hipLaunchKernelGGL(rt_adj_own_kernel<decltype(norm)::value>, dim3(mt), dim3(256), 0, st, queries, gallery, lab, na, nb, col_offset, row_offset, M, N, d,
                       w.own, w.best);
  });
  COOT_CHECK_LAUNCH("rt_adj_own");
  rt_launch_lab_prepare(labels, w.best, M, N, ranks_q, ranks_g, n_valid, st);
  COOT_CHECK_LAUNCH("rt_lab_prepare");
  with_bool(normalize, [&](auto norm) {
    hipLaunchKernelGGL(rt_adj_rank_kernel<decltype(norm)::value>, dim3(nt, mt), dim3(256), 0, st, queries, gallery, lab, na, nb, col_offset, row_offset, M, N,
                       d, (const float*)w.own, (const tk_entry_t*)w.best, sim_out, (int*)ranks_q, (int*)ranks_g);
  });
  COOT_CHECK_LAUNCH("rt_adj_rank");
  if (metrics) {
    rt_launch_lab_metrics(ranks_q, ranks_g, M, N, w.hist, metrics, st);
    COOT_CHECK_LAUNCH("rt_lab_metrics");
  }
  return 0;
}

}  // extern "C"
