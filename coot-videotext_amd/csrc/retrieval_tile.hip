// Retrieval ranking on the device: validate_epoch's normalisation (coot/trainer_retrieval.py:397-402),
// the similarity matrix d = emb1 . emb2^T and compute_retrieval_cosine (nntrainer/retrieval.py:57-98) for BOTH directions,
// without materialising d and without leaving the GPU.  The reference does this on the host: a D2H copy per batch, an
// fp32 sgemm and one numpy argsort per row (O(N^2 log N), ~30 s per epoch for the 4 917 ActivityNet validation videos).
//
//   rank of item i in row i of d = position of i in argsort(d[i])[::-1] = #{j : d_ij > d_ii}            (no exact ties)
//   ties: counted as ahead of i when j > i (= the reversal of a stable ascending sort; numpy's introsort leaves the order
//         of exact ties unspecified, so no rule can be "the" reference one — exact fp32 ties between different
//         embeddings do not occur on real data)
//
// Everything is integer counting on top of fp32 similarities, so the similarity arithmetic is fixed: one fp32 FMA chain
// per element in k order (chunks of 32), identical in the diagonal pass and in the full pass, and identical to what
// the optional sim output holds — the ranks are bit-exact functions of that matrix (tests/test_retrieval_device.py
// checks them against numpy's argsort on the matrix the kernel wrote).
//
// HBM / VALU bound integer + fp32 work: not reshaped into bf16 MFMA GEMMs (bf16 similarities would reorder near-ties).
//
// This file holds every kernel that is built on tile_dot, the 64 x 64 tile: the ranks, the tile top-K search and the labelled ranking,
// each with its entry points.  They share one translation unit on purpose.  tile_dot has internal linkage and is optimised with all
// of its callers in view; with the callers in separate files the four rt_topk_kernel instantiations and rt_lab_rank_kernel<true>
// compile to different instructions (tools/kernel_isa.py shows it).  The few-query search is retrieval_few.hip, the rows of a
// prepared gallery retrieval_index.hip, what they share retrieval.h.
#include "retrieval.h"

namespace coot {
namespace {

// x / sqrt(sum x^2) per row (coot/trainer_retrieval.py:400-402: no eps), one wave per row; rows [0, N) of a, then of b
__global__ __launch_bounds__(256) void rt_normalize_kernel(const float* a, const float* b, int N, int d, float* na, float* nb) {
  const int lane = threadIdx.x & 63, row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= 2 * N) return;
  const float* src = row < N ? a + (long)row * d : b + (long)(row - N) * d;
  float* dst = row < N ? na + (long)row * d : nb + (long)(row - N) * d;
  const float nrm = sqrtf(row_sumsq(src, d, lane));
  for (int c = lane; c < d; c += 64) dst[c] = src[c] / nrm;
}

// One 64 x 64 tile of d: thread (ty, tx) of a 16 x 16 grid owns the 4 x 4 block rows 4 ty .., columns 4 tx ..
// acc[r][c] accumulates in k order, chunk by chunk: the same chain for every element in every pass.
// A has NA rows, B has NB rows.  NORM (the top-K search, which keeps no normalised copy of a 200 000-row gallery): the staged value
// is x / norm of its row, the division rt_normalize_kernel makes, so the chain sees the same operands as on a normalised copy.
// TB (the search on a prepared gallery, which may hold 16-bit rows): the element type of B, widened as it is staged; from LDS on
// nothing knows of it.
struct Tile { float acc[4][4]; };
template <bool NORM = false, typename TB = float>
__device__ __forceinline__ void tile_dot(const float* A, const TB* B, int NA, int NB, int d, int i0, int j0, float (*As)[RP], float (*Bs)[RP], Tile& t,
                                         const float* nA = nullptr, const float* nB = nullptr) {
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
        Bs[r][k] = (kin && j0 + r < NB) ? widen(B[(long)(j0 + r) * d + k0 + k]) / rb[q] : 0.f;
      } else {
        As[r][k] = (kin && i0 + r < NA) ? A[(long)(i0 + r) * d + k0 + k] : 0.f;
        Bs[r][k] = (kin && j0 + r < NB) ? widen(B[(long)(j0 + r) * d + k0 + k]) : 0.f;
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

// pass 1: the diagonal entries d_ii (tile (I, I) only)
__global__ __launch_bounds__(256) void rt_diag_kernel(const float* A, const float* B, int N, int d, float* diag) {
  __shared__ float As[RT][RP], Bs[RT][RP];
  const int i0 = blockIdx.x * RT;
  Tile t;
  tile_dot(A, B, N, N, d, i0, i0, As, Bs, t);
  const int ty = threadIdx.x >> 4, tx = threadIdx.x & 15;
  if (ty == tx) {
#pragma unroll
    for (int r = 0; r < 4; ++r)
      if (i0 + 4 * ty + r < N) diag[i0 + 4 * ty + r] = t.acc[r][r];
  }
}

// pass 2: every tile; row counts -> ranks_ab (emb1 -> emb2), column counts -> ranks_ba
// PART (coot_retrieval_ranks_part): the rows [row0, row0 + rows) of d only, grid.y = the strip's row tiles, which start at row0
// (not tile aligned: an element's chain does not depend on the tile it sits in).  Row counts of the strip are final, column
// counts are the strip's share; sim is the strip [rows, N].  Integer sums, so the strips of a partition add up to the whole.
template <bool PART>
__global__ __launch_bounds__(256) void rt_rank_kernel(const float* A, const float* B, int N, int d, const float* diag, float* sim,
                                                      int* ranks_ab, int* ranks_ba, int row0, int rows) {
  __shared__ float As[RT][RP], Bs[RT][RP];
  __shared__ int rowc[RT], colc[RT];
  const int r0 = PART ? row0 : 0, r1 = PART ? row0 + rows : N;  // the rows this launch covers
  const int i0 = r0 + blockIdx.y * RT, j0 = blockIdx.x * RT;
  const int tid = threadIdx.x, ty = tid >> 4, tx = tid & 15;
  if (tid < RT) { rowc[tid] = 0; colc[tid] = 0; }
  Tile t;
  tile_dot(A, B, r1, N, d, i0, j0, As, Bs, t);  // ends with a barrier: the counters are zeroed
  float di[4], dj[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) di[r] = i0 + 4 * ty + r < r1 ? diag[i0 + 4 * ty + r] : 0.f;
#pragma unroll
  for (int c = 0; c < 4; ++c) dj[c] = j0 + 4 * tx + c < N ? diag[j0 + 4 * tx + c] : 0.f;
  int rc[4] = {0, 0, 0, 0}, cc[4] = {0, 0, 0, 0};
#pragma unroll
  for (int r = 0; r < 4; ++r)
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const int i = i0 + 4 * ty + r, j = j0 + 4 * tx + c;
      if (i < r1 && j < N) {
        const float s = t.acc[r][c];
        if (sim) sim[(long)(i - r0) * N + j] = s;
        if (i != j) {
          // row i of d: is j ahead of i?   column j of d (= row j of d^T): is i ahead of j?
          if (s > di[r] || (s == di[r] && j > i)) ++rc[r];
          if (s > dj[c] || (s == dj[c] && i > j)) ++cc[c];
        }
      }
    }
#pragma unroll
  for (int r = 0; r < 4; ++r) if (rc[r]) atomicAdd(&rowc[4 * ty + r], rc[r]);
#pragma unroll
  for (int c = 0; c < 4; ++c) if (cc[c]) atomicAdd(&colc[4 * tx + c], cc[c]);
  __syncthreads();
  if (tid < RT) {
    if (i0 + tid < r1 && rowc[tid]) atomicAdd(ranks_ab + i0 + tid, rowc[tid]);
    if (j0 + tid < N && colc[tid]) atomicAdd(ranks_ba + j0 + tid, colc[tid]);
  }
}

// R@1/5/10/50 (fractions), medr = floor(median) + 1, meanr = mean + 1, sum = r1 + r5 + r50 (nntrainer/retrieval.py:88-97)
// for one direction per workgroup.  The median of n integers from their histogram.  Workgroup 0 = ranks_a [M], ranks in [0, N),
// hist [N]; workgroup 1 = ranks_b [N], ranks in [0, M), hist + N [M].  hist zeroed.
// LAB = false (coot_retrieval_ranks, coot_retrieval_metrics; M == N): every entry counts, n = N; an entry outside [0, N) is in the
// sum and the recall counters and not in the histogram.  LAB = true (coot_retrieval_ranks_labeled): over the n entries >= 0 of each
// vector; n = 0: seven zeros.
template <bool LAB>
__global__ __launch_bounds__(1024) void rt_metrics_kernel(const int* ranks_a, const int* ranks_b, int M, int N, int* hist, float* out) {
  __shared__ unsigned long long s_sum;
  __shared__ int s_cnt[5];  // < 1, < 5, < 10, < 50, n
  __shared__ int s_scan[1024];
  __shared__ int s_med[2];
  const int* ranks = blockIdx.x == 0 ? ranks_a : ranks_b;
  const int len = blockIdx.x == 0 ? M : N, H = blockIdx.x == 0 ? N : M;
  int* h = hist + (long)blockIdx.x * N;
  const int tid = threadIdx.x;
  if (tid == 0) { s_sum = 0ull; s_med[0] = -1; s_med[1] = -1; }
  if (tid < 5) s_cnt[tid] = 0;
  __syncthreads();
  unsigned long long ls = 0ull;
  int lc[5] = {0, 0, 0, 0, 0};
  for (int i = tid; i < len; i += 1024) {
    const int r = ranks[i];
    if (LAB && r < 0) continue;
    ls += (unsigned long long)r;
    lc[0] += r < 1; lc[1] += r < 5; lc[2] += r < 10; lc[3] += r < 50; ++lc[4];
    if ((unsigned)r < (unsigned)H) atomicAdd(h + r, 1);  // (a rank is < H; coot_retrieval_metrics takes the caller's: never outside hist)
  }
  atomicAdd(&s_sum, ls);
#pragma unroll
  for (int q = 0; q < 5; ++q) if (lc[q]) atomicAdd(&s_cnt[q], lc[q]);
  __threadfence();
  __syncthreads();
  const int n = LAB ? s_cnt[4] : len;
  // order statistics (n - 1) / 2 and n / 2 (0-based) of the sorted ranks: np.median averages them
  const int per = (H + 1023) / 1024, lo = min(H, tid * per), hi = min(H, lo + per);
  int part = 0;
  for (int v = lo; v < hi; ++v) part += __hip_atomic_load(h + v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // the counts were made with device atomics
  s_scan[tid] = part;
  __syncthreads();
  if (tid == 0) {
    int run = 0;
    for (int q = 0; q < 1024; ++q) { const int c = s_scan[q]; s_scan[q] = run; run += c; }
  }
  __syncthreads();
  const int k0 = (n - 1) / 2, k1 = n / 2;
  int run = s_scan[tid];
  for (int v = lo; v < hi; ++v) {
    const int c = __hip_atomic_load(h + v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (c) {
      if (k0 >= run && k0 < run + c) s_med[0] = v;
      if (k1 >= run && k1 < run + c) s_med[1] = v;
      run += c;
    }
  }
  __syncthreads();
  if (tid == 0) {
    float* o = out + 7 * blockIdx.x;
    if (LAB && n == 0) {
      for (int q = 0; q < 7; ++q) o[q] = 0.f;
    } else {
      const float nf = (float)n;
      const float r1 = s_cnt[0] / nf, r5 = s_cnt[1] / nf, r10 = s_cnt[2] / nf, r50 = s_cnt[3] / nf;
      const double med = 0.5 * ((double)s_med[0] + (double)s_med[1]);
      o[0] = r1; o[1] = r5; o[2] = r10; o[3] = r50;
      o[4] = (float)(floor(med) + 1.0);
      o[5] = (float)((double)s_sum / (double)n + 1.0);
      o[6] = r1 + r5 + r50;
    }
  }
}

struct Ws { float *na, *nb, *diag; int* hist; size_t bytes; };
Ws layout(void* base, int N, int d) {
  Arena a{(char*)base}; Ws w;
  w.na = a.take<float>((size_t)N * d); w.nb = a.take<float>((size_t)N * d); w.diag = a.take<float>(N);
  w.hist = a.take<int>((size_t)2 * N);
  w.bytes = a.off;
  return w;
}

// the histogram zero fill + rt_metrics_kernel<false>: the tail of coot_retrieval_ranks and all of coot_retrieval_metrics
int launch_metrics(const int32_t* ranks_12, const int32_t* ranks_21, int N, int* hist, float* metrics, hipStream_t st) {
  if (int rc = check_hip(hipMemsetAsync(hist, 0, (size_t)2 * N * 4, st), "memset hist")) return rc;
  hipLaunchKernelGGL(rt_metrics_kernel<false>, dim3(2), dim3(1024), 0, st, (const int*)ranks_12, (const int*)ranks_21, N, N, hist, metrics);
  COOT_CHECK_LAUNCH("rt_metrics");
  return 0;
}

// ---- top-K search: M queries against an N-row gallery (coot_retrieval_topk) --------------------------------------------------
// Row i of the result = the K best columns of row i of d = queries . gallery^T by the total order (score descending, then
// column descending) = np.argsort(d[i], kind="stable")[::-1][:K]: the tie rule of the ranks above (j > i counts as ahead), so
// on square input item i sits at position ranks_12[i] of its row.  d is the tile_dot chain and is never stored (unless the
// caller asks for it): the selection runs on the tile accumulators.
//
//   rt_topk_kernel: workgroup (split s, row tile I) walks its share of the column tiles.  Per row a sorted list of <= K
//     entries in LDS; an accumulator is compared with the row's K-th entry (after a few tiles almost none passes) and the
//     ones that pass are appended to the row's candidate buffer (an LDS counter hands out the slot: the buffer's ORDER depends
//     on the schedule, its content does not).  Then one wave per row folds the candidates into the list by rank: the new
//     position of an entry is the number of entries ahead of it.
//   rt_topk_merge_kernel: the S partial lists of a row hold distinct columns, so the final position of an entry is its own
//     position plus the number of entries ahead of it in the other lists (binary searches).  S = 1 writes the result directly.
constexpr int TK_SMAX = 64;          // column splits
constexpr int TK_TARGET_WGS = 1024;  // automatic split count: about four workgroups per CU
int g_rt_topk_splits = 0;            // coot_set_option("rt_topk_splits", n) (tests); 0 = automatic

size_t tk_lds_bytes(int K) { return (size_t)2 * RT * RP * 4 + (size_t)RT * RT * 8 + (size_t)RT * K * 8 + 2 * RT * 4; }

// grid (S, row tiles); LDS: As | Bs | cand [RT][RT] | list [RT][K] | cnt [RT] | ncand [RT]   (tk_lds_bytes)
// MASKED (coot_retrieval_topk_masked): keep [N] bytes, nonzero = the gallery row may be returned.  A row whose byte is zero is
// never a candidate (its accumulator is neither compared nor appended); sim still holds every similarity.  Without sim a column
// tile that keeps no row is skipped before its first load: the vote is a workgroup reduction, so every thread takes the same
// way round the barriers.  keep is the last parameter: the unmasked instantiations read the arguments they always read.
template <bool NORM, bool MASKED>
__global__ __launch_bounds__(256) void rt_topk_kernel(const float* A, const float* B, const float* nA, const float* nB, int M, int N, int d,
                                                      int K, int tiles_per_split, int S, float* sim, tk_entry_t* part, int* idx_out,
                                                      float* score_out, const unsigned char* keep) {
  extern __shared__ __attribute__((aligned(16))) char tk_lds[];
  float (*As)[RP] = (float (*)[RP])tk_lds;
  float (*Bs)[RP] = (float (*)[RP])(tk_lds + RT * RP * 4);
  tk_entry_t* cand = (tk_entry_t*)(tk_lds + 2 * RT * RP * 4);
  tk_entry_t* list = cand + RT * RT;
  int* cnt = (int*)(list + RT * K);
  int* ncand = cnt + RT;
  const int tid = threadIdx.x, ty = tid >> 4, tx = tid & 15, wave = tid >> 6, lane = tid & 63;
  const int i0 = blockIdx.y * RT, nt = (N + RT - 1) / RT;
  const int t0 = blockIdx.x * tiles_per_split, t1 = min(nt, t0 + tiles_per_split);
  if (tid < RT) { cnt[tid] = 0; ncand[tid] = 0; }
  for (int e = tid; e < RT * K; e += 256) list[e] = 0ull;  // 0 = behind every entry: an unfilled slot
  for (int tj = t0; tj < t1; ++tj) {
    const int j0 = tj * RT;
    unsigned kp = 0u;  // MASKED: bit c = the keep flag of column j0 + 4 tx + c
    if constexpr (MASKED) {
      if (!sim && !__syncthreads_or(tid < RT && j0 + tid < N && keep[j0 + tid])) continue;  // (uniform: nothing of this tile is touched)
#pragma unroll
      for (int c = 0; c < 4; ++c) kp |= (j0 + 4 * tx + c < N && keep[j0 + 4 * tx + c]) ? 1u << c : 0u;
    }
    Tile t;
    tile_dot<NORM>(A, B, M, N, d, i0, j0, As, Bs, t, nA, nB);  // ends with a barrier: lists and counters of the previous tile are settled
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = 4 * ty + r, i = i0 + row;
      if (i >= M) continue;
      const bool full = cnt[row] >= K;
      const tk_entry_t kth = list[row * K + K - 1];
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const int j = j0 + 4 * tx + c;
        if (j >= N) continue;
        const float s = t.acc[r][c];
        if (sim) sim[(long)i * N + j] = s;
        if constexpr (MASKED) { if (!(kp >> c & 1u)) continue; }
        const tk_entry_t e = tk_pack(s, j);
        if (!full || e > kth) cand[row * RT + atomicAdd(&ncand[row], 1)] = e;  // <= RT columns of this tile per row
      }
    }
    __syncthreads();
    // fold the candidates in: wave w takes rows w, w + 4, ...; every entry is read before the barrier and placed after it
    for (int row = wave; row < RT; row += 4) {
      const int nc = ncand[row], n = cnt[row];
      tk_entry_t* L = list + row * K;
      const tk_entry_t* C = cand + row * RT;
      TkFold f;
      f.read(L, n, C, nc, lane);
      __syncthreads();
      if (nc) {
        f.place(L, K);
        if (lane == 0) { cnt[row] = min(K, n + nc); ncand[row] = 0; }
      }
    }
  }
  __syncthreads();
  for (int e = tid; e < RT * K; e += 256) {
    const int row = e / K, r = e - row * K, i = i0 + row;
    if (i >= M) continue;
    const tk_entry_t v = list[e];
    if (S == 1) {
      idx_out[(long)i * K + r] = MASKED ? tk_idx_masked(v) : (int)(unsigned)v;
      score_out[(long)i * K + r] = MASKED ? tk_score_masked(v) : tk_score(v);
    } else {
      part[((long)i * S + blockIdx.x) * K + r] = v;
    }
  }
}

// rt_topk_kernel on the 16-bit rows of a prepared gallery (coot_retrieval_topk_index; TB = unsigned short: bfloat16, or _Float16): the
// same statements, B of element type TB, which tile_dot widens as it stages it; nB are the norms the caller holds.  A kernel of its
// own and not a body shared with rt_topk_kernel: moved into a function that both kernels inline, the four fp32 instantiations come out
// with another instruction schedule (tools/kernel_isa.py), and they are promised to stay the parent's instruction for instruction.
template <typename TB, bool NORM, bool MASKED>
__global__ __launch_bounds__(256) void rt_topk_index_kernel(const float* A, const TB* B, const float* nA, const float* nB, int M, int N, int d,
                                                            int K, int tiles_per_split, int S, float* sim, tk_entry_t* part, int* idx_out,
                                                            float* score_out, const unsigned char* keep) {
  extern __shared__ __attribute__((aligned(16))) char tk_lds[];
  float (*As)[RP] = (float (*)[RP])tk_lds;
  float (*Bs)[RP] = (float (*)[RP])(tk_lds + RT * RP * 4);
  tk_entry_t* cand = (tk_entry_t*)(tk_lds + 2 * RT * RP * 4);
  tk_entry_t* list = cand + RT * RT;
  int* cnt = (int*)(list + RT * K);
  int* ncand = cnt + RT;
  const int tid = threadIdx.x, ty = tid >> 4, tx = tid & 15, wave = tid >> 6, lane = tid & 63;
  const int i0 = blockIdx.y * RT, nt = (N + RT - 1) / RT;
  const int t0 = blockIdx.x * tiles_per_split, t1 = min(nt, t0 + tiles_per_split);
  if (tid < RT) { cnt[tid] = 0; ncand[tid] = 0; }
  for (int e = tid; e < RT * K; e += 256) list[e] = 0ull;  // 0 = behind every entry: an unfilled slot
  for (int tj = t0; tj < t1; ++tj) {
    const int j0 = tj * RT;
    unsigned kp = 0u;  // MASKED: bit c = the keep flag of column j0 + 4 tx + c
    if constexpr (MASKED) {
      if (!sim && !__syncthreads_or(tid < RT && j0 + tid < N && keep[j0 + tid])) continue;  // (uniform: nothing of this tile is touched)
#pragma unroll
      for (int c = 0; c < 4; ++c) kp |= (j0 + 4 * tx + c < N && keep[j0 + 4 * tx + c]) ? 1u << c : 0u;
    }
    Tile t;
    tile_dot<NORM, TB>(A, B, M, N, d, i0, j0, As, Bs, t, nA, nB);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = 4 * ty + r, i = i0 + row;
      if (i >= M) continue;
      const bool full = cnt[row] >= K;
      const tk_entry_t kth = list[row * K + K - 1];
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const int j = j0 + 4 * tx + c;
        if (j >= N) continue;
        const float s = t.acc[r][c];
        if (sim) sim[(long)i * N + j] = s;
        if constexpr (MASKED) { if (!(kp >> c & 1u)) continue; }
        const tk_entry_t e = tk_pack(s, j);
        if (!full || e > kth) cand[row * RT + atomicAdd(&ncand[row], 1)] = e;  // <= RT columns of this tile per row
      }
    }
    __syncthreads();
    for (int row = wave; row < RT; row += 4) {
      const int nc = ncand[row], n = cnt[row];
      tk_entry_t* L = list + row * K;
      const tk_entry_t* C = cand + row * RT;
      TkFold f;
      f.read(L, n, C, nc, lane);
      __syncthreads();
      if (nc) {
        f.place(L, K);
        if (lane == 0) { cnt[row] = min(K, n + nc); ncand[row] = 0; }
      }
    }
  }
  __syncthreads();
  for (int e = tid; e < RT * K; e += 256) {
    const int row = e / K, r = e - row * K, i = i0 + row;
    if (i >= M) continue;
    const tk_entry_t v = list[e];
    if (S == 1) {
      idx_out[(long)i * K + r] = MASKED ? tk_idx_masked(v) : (int)(unsigned)v;
      score_out[(long)i * K + r] = MASKED ? tk_score_masked(v) : tk_score(v);
    } else {
      part[((long)i * S + blockIdx.x) * K + r] = v;
    }
  }
}

// one wave per row: part [M][S][K], every list sorted best first, unfilled slots 0 at its end
// MASKED: the real entries of a row may total R < K (a split whose columns are all masked hands in an all-unfilled list).  A real
// entry's rank is its position among the real ones, below R.  An unfilled slot at position p of list s, which holds n_s real
// entries, has every real entry of the other lists ahead of it: rank p + (R - n_s) >= R, and as p runs over [n_s, K) that covers
// [R, K + R - n_s), which contains [R, K) whichever list it is.  So every output slot is written; unfilled slots of different lists
// may share a rank, and all of them write (-1, -inf).
template <bool MASKED>
__global__ __launch_bounds__(256) void rt_topk_merge_kernel(const tk_entry_t* part, int M, int S, int K, int* idx_out, float* score_out) {
  const int lane = threadIdx.x & 63, row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= M) return;
  const tk_entry_t* P = part + (long)row * S * K;
  for (int e = lane; e < S * K; e += 64) {
    const int s = e / K;
    const tk_entry_t v = P[e];
    int rank = e - s * K;
    for (int t = 0; t < S && rank < K; ++t)
      if (t != s) rank += tk_ahead(P + t * K, K, v);
    if (rank < K) {  // (unmasked: an unfilled slot is behind all N >= K real entries)
      idx_out[(long)row * K + rank] = MASKED ? tk_idx_masked(v) : (int)(unsigned)v;
      score_out[(long)row * K + rank] = MASKED ? tk_score_masked(v) : tk_score(v);
    }
  }
}

// column splits and the tiles each one walks: every split has at least one tile
struct TkSplit { int S, tiles; };
TkSplit tk_split(int M, int N) {
  const int mt = (M + RT - 1) / RT, nt = (N + RT - 1) / RT;
  int S = g_rt_topk_splits > 0 ? g_rt_topk_splits : (TK_TARGET_WGS + mt - 1) / mt;
  S = S < 1 ? 1 : S; S = S > TK_SMAX ? TK_SMAX : S; S = S > nt ? nt : S;
  TkSplit r; r.tiles = (nt + S - 1) / S; r.S = (nt + r.tiles - 1) / r.tiles;
  return r;
}
struct TkWs { float *na, *nb; tk_entry_t* part; size_t bytes; };
TkWs tk_layout(void* base, int M, int N, int K, int S) {
  Arena a{(char*)base}; TkWs w;
  w.na = a.take<float>(M); w.nb = a.take<float>(N);
  w.part = a.take<tk_entry_t>(S > 1 ? (size_t)M * S * K : 0);
  w.bytes = a.off;
  return w;
}

// The tile kernel on a gallery of element type T and, with more than one split, the merge: what every tile search launches after its
// norms.  fp32 rows take rt_topk_kernel, 16-bit rows rt_topk_index_kernel; na / nb == nullptr: the instantiations without NORM.
template <typename T>
int tk_launch(const float* queries, const T* gallery, const float* na, const float* nb, const unsigned char* keep, int M, int N, int d, int K, TkSplit sp,
              tk_entry_t* part, int32_t* idx_out, float* score_out, float* sim_out, hipStream_t st) {
  with_bool(na != nullptr, keep != nullptr, [&](auto norm, auto masked) {
    constexpr bool NORM = decltype(norm)::value, MASKED = decltype(masked)::value;
    const dim3 grid(sp.S, (M + RT - 1) / RT);
    if constexpr (std::is_same_v<T, float>)
      hipLaunchKernelGGL((rt_topk_kernel<NORM, MASKED>), grid, dim3(256), tk_lds_bytes(K), st, queries, gallery, na, nb, M, N, d, K, sp.tiles, sp.S, sim_out,
                         part, (int*)idx_out, score_out, keep);
    else
      hipLaunchKernelGGL((rt_topk_index_kernel<T, NORM, MASKED>), grid, dim3(256), tk_lds_bytes(K), st, queries, gallery, na, nb, M, N, d, K, sp.tiles, sp.S,
                         sim_out, part, (int*)idx_out, score_out, keep);
  });
  COOT_CHECK_LAUNCH("rt_topk");
  if (sp.S > 1) {
    with_bool(keep != nullptr, [&](auto masked) {
      hipLaunchKernelGGL(rt_topk_merge_kernel<decltype(masked)::value>, dim3((M + 3) / 4), dim3(256), 0, st, (const tk_entry_t*)part, M, sp.S, K,
                         (int*)idx_out, score_out);
    });
    COOT_CHECK_LAUNCH("rt_topk_merge");
  }
  return 0;
}

// coot_retrieval_topk and coot_retrieval_topk_masked (keep == nullptr: the unmasked kernels, launched as coot_retrieval_topk
// launches them): fn names the entry in a refusal
int topk_search(const char* fn, const float* queries, const float* gallery, const unsigned char* keep, int M, int N, int d, int K, int normalize,
                int32_t* idx_out, float* score_out, float* sim_out, void* workspace, size_t workspace_bytes, hipStream_t st) {
  COOT_REQUIRE(queries && gallery && idx_out && score_out && workspace, "%s: null pointer", fn);
  COOT_REQUIRE(M >= 1 && N >= 1 && d >= 1 && (M + RT - 1) / RT <= 65535, "%s: M = %d, N = %d, d = %d", fn, M, N, d);
  COOT_REQUIRE(K >= 1 && K <= N && K <= TK_MAX, "%s: K = %d is outside 1 .. min(N = %d, %d)", fn, K, N, TK_MAX);
  const TkSplit sp = tk_split(M, N);
  TkWs w = tk_layout(workspace, M, N, K, sp.S);
  COOT_REQUIRE(w.bytes <= workspace_bytes, "%s: workspace too small (%zu < %zu)", fn, workspace_bytes, w.bytes);
  if (normalize) {
    rt_launch_norms(queries, M, gallery, N, d, w.na, w.nb, st);
    COOT_CHECK_LAUNCH("rt_norms");
  }
  // the instantiations without NORM get no norms
  return tk_launch(queries, gallery, normalize ? w.na : nullptr, normalize ? w.nb : nullptr, keep, M, N, d, K, sp, w.part, idx_out, score_out, sim_out, st);
}

// coot_retrieval_topk_index: the query norms and the partial lists; the gallery's norms are the caller's
struct TkIndexWs { float* na; tk_entry_t* part; size_t bytes; };
TkIndexWs tk_index_layout(void* base, int M, int K, int S) {
  Arena a{(char*)base}; TkIndexWs w;
  w.na = a.take<float>(M);
  w.part = a.take<tk_entry_t>(S > 1 ? (size_t)M * S * K : 0);
  w.bytes = a.off;
  return w;
}

// ---- labelled ranking: M queries, N gallery rows, labels[i] = the gallery row of query i (coot_retrieval_ranks_labeled) ------
// The ranks of coot_retrieval_ranks without the diagonal assumption: several queries per gallery row, gallery rows without a
// query, queries without a row (a label outside [0, N): rank -1, in neither direction's metrics, never used as an index).
//   query -> gallery: ranks_q[i] = #{j != g : (s_ij, j) ahead of (s_ig, g)}, g = labels[i]
//   gallery -> query: the best positive of column j is the valid query i with labels[i] = j that is ahead of the others,
//                     (t_j, a_j) = (s_ij, i);  ranks_g[j] = #{i' : (s_i'j, i') ahead of (t_j, a_j)}: the best-ranked ground truth
// "ahead" = the tie rule above (larger, or equal with a later index).  s is the tile_dot chain, never stored:
//   rt_lab_own_kernel: own[i] = s[i, labels[i]] by the chain of tile_dot (64 queries per workgroup, the operands staged as there,
//     gallery rows gathered; one thread per query walks k, zero padding of the last chunk included: the accumulators' bits), and
//     an integer atomic max of the (score, i) word into best[j]: independent of the schedule.  best = 0: no valid query.
//   rt_lab_prepare_kernel: ranks_q / ranks_g = 0 or -1, n_valid.
//   rt_lab_rank_kernel: rt_rank_kernel's counting with thresholds (own[i], labels[i]) per row and (t_j, a_j) per column.
//   rt_metrics_kernel<true>: the metrics over the entries >= 0 of each vector.
template <bool NORM>
__global__ __launch_bounds__(256) void rt_lab_own_kernel(const float* A, const float* B, const int* labels, const float* nA, const float* nB, int M,
                                                         int N, int d, float* own, tk_entry_t* best) {
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
    own[i0 + tid] = acc;
    atomicMax(best + lab[tid], tk_pack(acc, i0 + tid));
  }
}

// one workgroup: the rank vectors start at 0 where there is a ground truth and stay -1 elsewhere; n_valid = the numbers of both
__global__ __launch_bounds__(1024) void rt_lab_prepare_kernel(const int* labels, const tk_entry_t* best, int M, int N, int* ranks_q, int* ranks_g,
                                                              int* n_valid) {
  __shared__ int s_n[2];
  const int tid = threadIdx.x;
  if (tid < 2) s_n[tid] = 0;
  __syncthreads();
  int nq = 0, ng = 0;
  for (int i = tid; i < M; i += 1024) {
    const bool v = (unsigned)labels[i] < (unsigned)N;
    ranks_q[i] = v ? 0 : -1; nq += v;
  }
  for (int j = tid; j < N; j += 1024) {
    const bool v = best[j] != 0ull;
    ranks_g[j] = v ? 0 : -1; ng += v;
  }
  if (nq) atomicAdd(&s_n[0], nq);
  if (ng) atomicAdd(&s_n[1], ng);
  __syncthreads();
  if (tid < 2) n_valid[tid] = s_n[tid];
}

// every tile of s: grid (column tiles, row tiles); row counts -> ranks_q, column counts -> ranks_g
// (waves_per_eu: NORM would take 130 VGPRs, two more than 4 waves per SIMD allow — rt_rank_kernel's occupancy; no spill at 128)
template <bool NORM>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(4, 4))) void rt_lab_rank_kernel(const float* A, const float* B, const int* labels, const float* nA, const float* nB, int M,
                                                          int N, int d, const float* own, const tk_entry_t* best, float* sim, int* ranks_q,
                                                          int* ranks_g) {
  __shared__ float As[RT][RP], Bs[RT][RP];
  __shared__ int rowc[RT], colc[RT];
  const int i0 = blockIdx.y * RT, j0 = blockIdx.x * RT;
  const int tid = threadIdx.x, ty = tid >> 4, tx = tid & 15;
  if (tid < RT) { rowc[tid] = 0; colc[tid] = 0; }
  Tile t;
  tile_dot<NORM>(A, B, M, N, d, i0, j0, As, Bs, t, nA, nB);  // ends with a barrier: the counters are zeroed
  float di[4], tj[4];
  int gi[4], aj[4];  // gi: the row's label, -1 = none;  aj: the column's best positive query, -1 = none
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int i = i0 + 4 * ty + r, g = i < M ? labels[i] : -1;
    gi[r] = (unsigned)g < (unsigned)N ? g : -1;
    di[r] = gi[r] >= 0 ? own[i] : 0.f;
  }
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    const int j = j0 + 4 * tx + c;
    const tk_entry_t e = j < N ? best[j] : 0ull;
    aj[c] = e ? (int)(unsigned)e : -1;
    tj[c] = tk_score(e);
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
        // row i: is j ahead of the label's column?   column j: is i ahead of the column's best positive?
        if (gi[r] >= 0 && j != gi[r] && (s > di[r] || (s == di[r] && j > gi[r]))) ++rc[r];
        if (aj[c] >= 0 && (s > tj[c] || (s == tj[c] && i > aj[c]))) ++cc[c];
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

// best and hist are adjacent: one zero fill
struct LabWs { float *na, *nb, *own; tk_entry_t* best; int* hist; size_t zero_bytes, bytes; };
LabWs lab_layout(void* base, int M, int N) {
  Arena a{(char*)base}; LabWs w;
  w.na = a.take<float>(M); w.nb = a.take<float>(N); w.own = a.take<float>(M);
  const size_t z0 = a.off;
  w.best = a.take<tk_entry_t>(N);
  w.hist = a.take<int>((size_t)N + M);
  w.zero_bytes = a.off - z0;
  w.bytes = a.off;
  return w;
}

}  // namespace
// rt_lab_prepare_kernel and rt_metrics_kernel<true> for the labelled ranking under offsets (retrieval_ranks_adjusted.hip)
void rt_launch_lab_prepare(const int32_t* labels, const unsigned long long* best, int M, int N, int32_t* ranks_q, int32_t* ranks_g, int32_t* n_valid,
                           hipStream_t st) {
  hipLaunchKernelGGL(rt_lab_prepare_kernel, dim3(1), dim3(1024), 0, st, (const int*)labels, (const tk_entry_t*)best, M, N, (int*)ranks_q, (int*)ranks_g,
                     (int*)n_valid);
}
void rt_launch_lab_metrics(const int32_t* ranks_q, const int32_t* ranks_g, int M, int N, int* hist, float* metrics, hipStream_t st) {
  hipLaunchKernelGGL(rt_metrics_kernel<true>, dim3(2), dim3(1024), 0, st, (const int*)ranks_q, (const int*)ranks_g, M, N, hist, metrics);
}
void set_rt_topk_splits(int n) { g_rt_topk_splits = n; }
int get_rt_topk_splits() { return g_rt_topk_splits; }
}  // namespace coot

using namespace coot;

extern "C" {

size_t coot_retrieval_workspace_bytes(int N, int d) { return layout(nullptr, N, d).bytes + 256; }

int coot_retrieval_ranks(const float* emb1, const float* emb2, int N, int d, int normalize, int32_t* ranks_12, int32_t* ranks_21,
                         float* metrics, float* sim_out, void* workspace, size_t workspace_bytes, coot_stream_t stream) {
  COOT_REQUIRE(emb1 && emb2 && ranks_12 && ranks_21 && workspace, "retrieval: null pointer");
  COOT_REQUIRE(N >= 1 && d >= 1, "retrieval: N = %d, d = %d", N, d);
  hipStream_t st = (hipStream_t)stream;
  Ws w = layout(workspace, N, d);
  COOT_REQUIRE(w.bytes <= workspace_bytes, "retrieval: workspace too small (%zu < %zu)", workspace_bytes, w.bytes);
  const float *A = emb1, *B = emb2;
  if (normalize) {
    hipLaunchKernelGGL(rt_normalize_kernel, dim3((2 * N + 3) / 4), dim3(256), 0, st, emb1, emb2, N, d, w.na, w.nb);
    COOT_CHECK_LAUNCH("rt_normalize");
    A = w.na; B = w.nb;
  }
  if (int rc = check_hip(hipMemsetAsync(ranks_12, 0, (size_t)N * 4, st), "memset ranks")) return rc;
  if (int rc = check_hip(hipMemsetAsync(ranks_21, 0, (size_t)N * 4, st), "memset ranks")) return rc;
  const int nt = (N + RT - 1) / RT;
  hipLaunchKernelGGL(rt_diag_kernel, dim3(nt), dim3(256), 0, st, A, B, N, d, w.diag);
  COOT_CHECK_LAUNCH("rt_diag");
  hipLaunchKernelGGL(rt_rank_kernel<false>, dim3(nt, nt), dim3(256), 0, st, A, B, N, d, (const float*)w.diag, sim_out, (int*)ranks_12, (int*)ranks_21, 0, N);
  COOT_CHECK_LAUNCH("rt_rank");
  if (metrics) return launch_metrics(ranks_12, ranks_21, N, w.hist, metrics, st);
  return 0;
}

size_t coot_retrieval_ranks_part_workspace_bytes(int N, int d) { return layout(nullptr, N, d).bytes + 256; }

int coot_retrieval_ranks_part(const float* emb1, const float* emb2, int N, int d, int normalize, int row0, int rows, int32_t* counts_12,
                              int32_t* counts_21, float* sim_out, void* workspace, size_t workspace_bytes, coot_stream_t stream) {
  COOT_REQUIRE(emb1 && emb2 && counts_12 && counts_21 && workspace, "retrieval_part: null pointer");
  COOT_REQUIRE(N >= 1 && d >= 1, "retrieval_part: N = %d, d = %d", N, d);
  COOT_REQUIRE(row0 >= 0 && rows >= 0 && row0 <= N && rows <= N - row0, "retrieval_part: rows [%d, %d + %d) are not inside [0, %d)", row0, row0, rows, N);
  hipStream_t st = (hipStream_t)stream;
  Ws w = layout(workspace, N, d);
  COOT_REQUIRE(w.bytes <= workspace_bytes, "retrieval_part: workspace too small (%zu < %zu)", workspace_bytes, w.bytes);
  if (int rc = check_hip(hipMemsetAsync(counts_12, 0, (size_t)N * 4, st), "memset counts")) return rc;
  if (int rc = check_hip(hipMemsetAsync(counts_21, 0, (size_t)N * 4, st), "memset counts")) return rc;
  if (rows == 0) return 0;
  const float *A = emb1, *B = emb2;
  if (normalize) {  // every row: all of emb2 is read, and the diagonal below needs all of emb1
    hipLaunchKernelGGL(rt_normalize_kernel, dim3((2 * N + 3) / 4), dim3(256), 0, st, emb1, emb2, N, d, w.na, w.nb);
    COOT_CHECK_LAUNCH("rt_normalize");
    A = w.na; B = w.nb;
  }
  const int nt = (N + RT - 1) / RT;
  hipLaunchKernelGGL(rt_diag_kernel, dim3(nt), dim3(256), 0, st, A, B, N, d, w.diag);  // d_jj of every column
  COOT_CHECK_LAUNCH("rt_diag");
  hipLaunchKernelGGL(rt_rank_kernel<true>, dim3(nt, (rows + RT - 1) / RT), dim3(256), 0, st, A, B, N, d, (const float*)w.diag, sim_out,
                     (int*)counts_12, (int*)counts_21, row0, rows);
  COOT_CHECK_LAUNCH("rt_rank_part");
  return 0;
}

int coot_retrieval_metrics(const int32_t* ranks_12, const int32_t* ranks_21, int N, float* metrics, void* workspace, size_t workspace_bytes,
                           coot_stream_t stream) {
  COOT_REQUIRE(ranks_12 && ranks_21 && metrics && workspace, "retrieval_metrics: null pointer");
  COOT_REQUIRE(N >= 1, "retrieval_metrics: N = %d", N);
  COOT_REQUIRE((size_t)2 * N * 4 <= workspace_bytes, "retrieval_metrics: workspace too small (%zu < %zu)", workspace_bytes, (size_t)2 * N * 4);
  COOT_REQUIRE(((uintptr_t)workspace & 3) == 0, "retrieval_metrics: workspace is not 4-byte aligned");
  return launch_metrics(ranks_12, ranks_21, N, (int*)workspace, metrics, (hipStream_t)stream);
}

size_t coot_retrieval_topk_workspace_bytes(int M, int N, int d, int K) {
  (void)d;  // no normalised copy is kept: the norms only
  if (M < 1 || N < 1 || K < 1) return 256;
  return tk_layout(nullptr, M, N, K, tk_split(M, N).S).bytes + 256;
}

int coot_retrieval_topk(const float* queries, const float* gallery, int M, int N, int d, int K, int normalize, int32_t* idx_out,
                        float* score_out, float* sim_out, void* workspace, size_t workspace_bytes, coot_stream_t stream) {
  return topk_search("retrieval_topk", queries, gallery, nullptr, M, N, d, K, normalize, idx_out, score_out, sim_out, workspace, workspace_bytes,
                     (hipStream_t)stream);
}

int coot_retrieval_topk_masked(const float* queries, const float* gallery, const uint8_t* keep, int M, int N, int d, int K, int normalize,
                               int32_t* idx_out, float* score_out, float* sim_out, void* workspace, size_t workspace_bytes, coot_stream_t stream) {
  return topk_search("retrieval_topk_masked", queries, gallery, keep, M, N, d, K, normalize, idx_out, score_out, sim_out, workspace, workspace_bytes,
                     (hipStream_t)stream);
}

size_t coot_retrieval_topk_index_workspace_bytes(int M, int N, int d, int K) {
  (void)d;
  if (M < 1 || N < 1 || K < 1) return 0;
  return tk_index_layout(nullptr, M, K, tk_split(M, N).S).bytes;  // exact: the call refuses one byte less
}

int coot_retrieval_topk_index(const float* queries, const void* gallery, int gallery_dtype, const float* gallery_norms, const uint8_t* keep, int M, int N,
                              int d, int K, int32_t* idx_out, float* score_out, float* sim_out, void* workspace, size_t workspace_bytes,
                              coot_stream_t stream) {
  const char* fn = "retrieval_topk_index";
  COOT_REQUIRE(gallery_dtype == COOT_GALLERY_F32 || gallery_dtype == COOT_GALLERY_BF16 || gallery_dtype == COOT_GALLERY_F16,
               "%s: gallery_dtype = %d (COOT_GALLERY_F32, COOT_GALLERY_BF16 or COOT_GALLERY_F16)", fn, gallery_dtype);
  COOT_REQUIRE(queries && gallery && idx_out && score_out && workspace, "%s: null pointer", fn);
  COOT_REQUIRE(M >= 1 && N >= 1 && d >= 1 && (M + RT - 1) / RT <= 65535, "%s: M = %d, N = %d, d = %d", fn, M, N, d);
  COOT_REQUIRE(K >= 1 && K <= N && K <= TK_MAX, "%s: K = %d is outside 1 .. min(N = %d, %d)", fn, K, N, TK_MAX);
  COOT_REQUIRE(((uintptr_t)workspace & 7) == 0, "%s: workspace is not 8-byte aligned", fn);
  hipStream_t st = (hipStream_t)stream;
  const TkSplit sp = tk_split(M, N);
  TkIndexWs w = tk_index_layout(workspace, M, K, sp.S);
  COOT_REQUIRE(w.bytes <= workspace_bytes, "%s: workspace too small (%zu < %zu)", fn, workspace_bytes, w.bytes);
  if (gallery_norms) {  // the queries' norms only: one launch over M rows
    rt_launch_norms(queries, M, nullptr, 0, d, w.na, nullptr, st);
    COOT_CHECK_LAUNCH("rt_norms");
  }
  return with_elem(gallery_dtype, [&](auto t) {
    using T = typename decltype(t)::type;
    return tk_launch(queries, (const T*)gallery, gallery_norms ? w.na : nullptr, gallery_norms, keep, M, N, d, K, sp, w.part, idx_out, score_out, sim_out, st);
  });
}

size_t coot_retrieval_ranks_labeled_workspace_bytes(int M, int N, int d) {
  (void)d;  // no normalised copy is kept: the norms only
  if (M < 1 || N < 1) return 0;
  return lab_layout(nullptr, M, N).bytes;  // exact: the call refuses one byte less
}

int coot_retrieval_ranks_labeled(const float* queries, const float* gallery, const int32_t* labels, int M, int N, int d, int normalize,
                                 int32_t* ranks_q, int32_t* ranks_g, int32_t* n_valid, float* metrics, float* sim_out, void* workspace,
                                 size_t workspace_bytes, coot_stream_t stream) {
  COOT_REQUIRE(queries && gallery && labels && ranks_q && ranks_g && n_valid && workspace, "retrieval_labeled: null pointer");
  COOT_REQUIRE(M >= 1 && N >= 1 && d >= 1 && (M + RT - 1) / RT <= 65535, "retrieval_labeled: M = %d, N = %d, d = %d", M, N, d);
  COOT_REQUIRE(((uintptr_t)workspace & 7) == 0, "retrieval_labeled: workspace is not 8-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  LabWs w = lab_layout(workspace, M, N);
  COOT_REQUIRE(w.bytes <= workspace_bytes, "retrieval_labeled: workspace too small (%zu < %zu)", workspace_bytes, w.bytes);
  const int mt = (M + RT - 1) / RT, nt = (N + RT - 1) / RT;
  const int* lab = (const int*)labels;
  if (int rc = check_hip(hipMemsetAsync(w.best, 0, w.zero_bytes, st), "memset best, hist")) return rc;
  const float *na = normalize ? w.na : nullptr, *nb = normalize ? w.nb : nullptr;  // the instantiations without NORM get no norms
  if (normalize) {
    rt_launch_norms(queries, M, gallery, N, d, w.na, w.nb, st);
    COOT_CHECK_LAUNCH("rt_norms");
  }
  with_bool(normalize, [&](auto norm) {
    hipLaunchKernelGGL(rt_lab_own_kernel<decltype(norm)::value>, dim3(mt), dim3(256), 0, st, queries, gallery, lab, na, nb, M, N, d, w.own, w.best);
  });
  COOT_CHECK_LAUNCH("rt_lab_own");
  hipLaunchKernelGGL(rt_lab_prepare_kernel, dim3(1), dim3(1024), 0, st, lab, (const tk_entry_t*)w.best, M, N, (int*)ranks_q, (int*)ranks_g,
                     (int*)n_valid);
  COOT_CHECK_LAUNCH("rt_lab_prepare");
  with_bool(normalize, [&](auto norm) {
    hipLaunchKernelGGL(rt_lab_rank_kernel<decltype(norm)::value>, dim3(nt, mt), dim3(256), 0, st, queries, gallery, lab, na, nb, M, N, d, (const float*)w.own,
                       (const tk_entry_t*)w.best, sim_out, (int*)ranks_q, (int*)ranks_g);
  });
  COOT_CHECK_LAUNCH("rt_lab_rank");
  if (metrics) {
    hipLaunchKernelGGL(rt_metrics_kernel<true>, dim3(2), dim3(1024), 0, st, (const int*)ranks_q, (const int*)ranks_g, M, N, w.hist, metrics);
    COOT_CHECK_LAUNCH("rt_lab_metrics");
  }
  return 0;
}

}  // extern "C"
