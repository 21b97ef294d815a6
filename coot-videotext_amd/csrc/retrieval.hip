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
#include "../../include/coot_hip.h"
#include "common.h"

namespace coot {
namespace {

constexpr int RT = 64;   // tile: 64 rows of emb1 x 64 rows of emb2
constexpr int RK = 32;   // k chunk
constexpr int RP = RK + 1;

// A gallery element as fp32: itself, a bfloat16 (unsigned short: the upper half of the fp32 word) or an IEEE half (v_cvt_f32_f16).
// Both 16-bit formats widen exactly, so whatever follows sees the operands of the widened fp32 copy.
__device__ __forceinline__ float widen(float x) { return x; }
__device__ __forceinline__ float widen(unsigned short x) { return __uint_as_float((unsigned)x << 16); }
__device__ __forceinline__ float widen(_Float16 x) { return (float)x; }
// half e (0 = low) of a 32-bit word that holds two 16-bit elements
template <typename T>
__device__ __forceinline__ float widen_half(unsigned w, int e) {
  const unsigned short b = (unsigned short)(e ? w >> 16 : w & 0xFFFFu);
  return widen(__builtin_bit_cast(T, b));
}

// sum x^2 of one row by one wave: the norm of rt_normalize_kernel and of rt_norms_kernel is this sum's sqrtf
template <typename T>
__device__ __forceinline__ float row_sumsq(const T* src, int d, int lane) {
  float s = 0.f;
  for (int c = lane; c < d; c += 64) { const float x = widen(src[c]); s += x * x; }
  return wave_sum(s);
}

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
struct Tile { float acc[4][4]; };
template <bool NORM = false>
__device__ __forceinline__ void tile_dot(const float* A, const float* B, int NA, int NB, int d, int i0, int j0, float (*As)[RP], float (*Bs)[RP], Tile& t,
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
// for one direction per workgroup.  hist: [2][N] ints, zeroed.  The median of N integers from their histogram.
__global__ __launch_bounds__(1024) void rt_metrics_kernel(const int* ranks_ab, const int* ranks_ba, int N, int* hist, float* out) {
  __shared__ unsigned long long s_sum;
  __shared__ int s_cnt[4];
  __shared__ int s_scan[1024];
  __shared__ int s_med[2];
  const int* ranks = blockIdx.x == 0 ? ranks_ab : ranks_ba;
  int* h = hist + (long)blockIdx.x * N;
  const int tid = threadIdx.x;
  if (tid == 0) { s_sum = 0ull; s_med[0] = -1; s_med[1] = -1; }
  if (tid < 4) s_cnt[tid] = 0;
  __syncthreads();
  unsigned long long ls = 0ull;
  int lc[4] = {0, 0, 0, 0};
  for (int i = tid; i < N; i += 1024) {
    const int r = ranks[i];
    ls += (unsigned long long)r;
    lc[0] += r < 1; lc[1] += r < 5; lc[2] += r < 10; lc[3] += r < 50;
    if ((unsigned)r < (unsigned)N) atomicAdd(h + r, 1);  // (a rank is < N; coot_retrieval_metrics takes the caller's: never outside hist)
  }
  atomicAdd(&s_sum, ls);
#pragma unroll
  for (int q = 0; q < 4; ++q) if (lc[q]) atomicAdd(&s_cnt[q], lc[q]);
  __threadfence();
  __syncthreads();
  // order statistics (N - 1) / 2 and N / 2 (0-based) of the sorted ranks: np.median averages them
  const int per = (N + 1023) / 1024, lo = tid * per, hi = min(N, lo + per);
  int part = 0;
  for (int v = lo; v < hi; ++v) part += __hip_atomic_load(h + v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // the counts were made with device atomics
  s_scan[tid] = part;
  __syncthreads();
  if (tid == 0) {
    int run = 0;
    for (int q = 0; q < 1024; ++q) { const int c = s_scan[q]; s_scan[q] = run; run += c; }
  }
  __syncthreads();
  const int k0 = (N - 1) / 2, k1 = N / 2;
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
    const float n = (float)N;
    const float r1 = s_cnt[0] / n, r5 = s_cnt[1] / n, r10 = s_cnt[2] / n, r50 = s_cnt[3] / n;
    const double med = 0.5 * ((double)s_med[0] + (double)s_med[1]);
    o[0] = r1; o[1] = r5; o[2] = r10; o[3] = r50;
    o[4] = (float)(floor(med) + 1.0);
    o[5] = (float)((double)s_sum / (double)N + 1.0);
    o[6] = r1 + r5 + r50;
  }
}

struct Ws { float *na, *nb, *diag; int* hist; size_t bytes; };
Ws layout(void* base, int N, int d) {
  Ws w; size_t off = 0;
  auto take = [&](size_t n) { char* p = base ? (char*)base + off : nullptr; off += (n + 255) & ~(size_t)255; return (void*)p; };
  w.na = (float*)take((size_t)N * d * 4); w.nb = (float*)take((size_t)N * d * 4); w.diag = (float*)take((size_t)N * 4);
  w.hist = (int*)take((size_t)2 * N * 4);
  w.bytes = off;
  return w;
}

// the histogram zero fill + rt_metrics_kernel: the tail of coot_retrieval_ranks and all of coot_retrieval_metrics
int launch_metrics(const int32_t* ranks_12, const int32_t* ranks_21, int N, int* hist, float* metrics, hipStream_t st) {
  if (int rc = check_hip(hipMemsetAsync(hist, 0, (size_t)2 * N * 4, st), "memset hist")) return rc;
  hipLaunchKernelGGL(rt_metrics_kernel, dim3(2), dim3(1024), 0, st, (const int*)ranks_12, (const int*)ranks_21, N, hist, metrics);
  COOT_CHECK_LAUNCH("rt_metrics");
  return 0;
}

// ---- top-K search: M queries against an N-row gallery (coot_retrieval_topk) --------------------------------------------------
// Row i of the result = the K best columns of row i of d = queries . gallery^T by the total order (score descending, then
// column descending) = np.argsort(d[i], kind="stable")[::-1][:K]: the tie rule of the ranks above (j > i counts as ahead), so
// on square input item i sits at position ranks_12[i] of its row.  d is the tile_dot chain and is never stored (unless the
// caller asks for it): the selection runs on the tile accumulators.
//
// An entry is one 64-bit word, (order-preserving image of the score) << 32 | column: "ahead" is one unsigned compare, a strict
// total order over every bit pattern (NaNs included), so selection and merge cannot depend on who came first.
//   rt_topk_kernel: workgroup (split s, row tile I) walks its share of the column tiles.  Per row a sorted list of <= K
//     entries in LDS; an accumulator is compared with the row's K-th entry (after a few tiles almost none passes) and the
//     ones that pass are appended to the row's candidate buffer (an LDS counter hands out the slot: the buffer's ORDER depends
//     on the schedule, its content does not).  Then one wave per row folds the candidates into the list by rank: the new
//     position of an entry is the number of entries ahead of it.
//   rt_topk_merge_kernel: the S partial lists of a row hold distinct columns, so the final position of an entry is its own
//     position plus the number of entries ahead of it in the other lists (binary searches).  S = 1 writes the result directly.
constexpr int TK_MAX = 128;          // K
constexpr int TK_SMAX = 64;          // column splits
constexpr int TK_TARGET_WGS = 1024;  // automatic split count: about four workgroups per CU
int g_rt_topk_splits = 0;            // coot_set_option("rt_topk_splits", n) (tests); 0 = automatic

typedef unsigned long long tk_entry_t;
__device__ __forceinline__ tk_entry_t tk_pack(float s, int j) {
  unsigned u = __float_as_uint(s + 0.0f);  // -0 -> +0: equal scores, as numpy compares them
  u ^= (unsigned)((int)u >> 31) | 0x80000000u;
  return ((tk_entry_t)u << 32) | (unsigned)j;
}
__device__ __forceinline__ float tk_score(tk_entry_t e) {
  const unsigned u = (unsigned)(e >> 32);
  return __uint_as_float(u ^ ((u & 0x80000000u) ? 0x80000000u : 0xFFFFFFFFu));
}
// number of entries ahead of v in a list sorted best first
__device__ __forceinline__ int tk_ahead(const tk_entry_t* L, int n, tk_entry_t v) {
  int lo = 0, hi = n;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (L[mid] > v) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// One wave folds nc <= 64 candidates C into the sorted list L of n entries, of which the K best stay: the new position of an entry
// is the number of entries ahead of it.  read() takes every entry and counts; place() writes them after a barrier of the waves
// that share the list (every entry is read before one is placed).
struct TkFold {
  tk_entry_t ec, e0, e1;
  int pc, p0, p1;
  bool hc, h0, h1;
  __device__ __forceinline__ void read(const tk_entry_t* L, int n, const tk_entry_t* C, int nc, int lane) {
    hc = lane < nc; h0 = lane < n; h1 = lane + 64 < n;
    ec = 0ull; e0 = 0ull; e1 = 0ull;
    pc = 0; p0 = lane; p1 = lane + 64;
    if (nc) {
      if (hc) { ec = C[lane]; pc = tk_ahead(L, n, ec); }
      if (h0) e0 = L[lane];
      if (h1) e1 = L[lane + 64];
      for (int q = 0; q < nc; ++q) {
        const tk_entry_t v = C[q];
        pc += v > ec; p0 += v > e0; p1 += v > e1;
      }
    }
  }
  __device__ __forceinline__ void place(tk_entry_t* L, int K) const {
    if (hc && pc < K) L[pc] = ec;
    if (h0 && p0 < K) L[p0] = e0;
    if (h1 && p1 < K) L[p1] = e1;
  }
};

size_t tk_lds_bytes(int K) { return (size_t)2 * RT * RP * 4 + (size_t)RT * RT * 8 + (size_t)RT * K * 8 + 2 * RT * 4; }

// The result of an unfilled slot in the masked searches (fewer than K kept rows): index -1, score -inf.  Word 0 is a real entry
// only for the all-ones NaN at column 0 (tk_pack), which a masked search therefore reports as unfilled.
__device__ __forceinline__ int tk_idx_masked(tk_entry_t e) { return e ? (int)(unsigned)e : -1; }
__device__ __forceinline__ float tk_score_masked(tk_entry_t e) { return e ? tk_score(e) : __uint_as_float(0xFF800000u); }

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

// sqrt(sum x^2) of every row of a [Ma, d], then of b [Nb, d]: rt_normalize_kernel's divisor (T: fp32 rows, or 16-bit rows widened)
template <typename T>
__global__ __launch_bounds__(256) void rt_norms_kernel(const T* a, int Ma, const T* b, int Nb, int d, float* na, float* nb) {
  const int lane = threadIdx.x & 63, row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= Ma + Nb) return;
  const float s = row_sumsq(row < Ma ? a + (long)row * d : b + (long)(row - Ma) * d, d, lane);
  if (lane == 0) { if (row < Ma) na[row] = sqrtf(s); else nb[row - Ma] = sqrtf(s); }
}

// An fp32 or 16-bit source element as a gallery element of type G (rt_put_kernel).  fp32 -> bfloat16 rounds to nearest even and writes
// every NaN as 0x7FC0 (what tensor.to(torch.bfloat16) writes); fp32 -> IEEE half is v_cvt_f16_f32 (nearest even, infinities above
// 65 504); a 16-bit element widens exactly; the same type is moved, never computed on: its bits stay.
template <typename G> struct Put;
template <> struct Put<float> {
  static __device__ __forceinline__ float from(float x) { return x; }
  static __device__ __forceinline__ float from(unsigned short x) { return widen(x); }
  static __device__ __forceinline__ float from(_Float16 x) { return widen(x); }
};
template <> struct Put<unsigned short> {
  static __device__ __forceinline__ unsigned short from(unsigned short x) { return x; }
  static __device__ __forceinline__ unsigned short from(float x) {
    const unsigned u = __float_as_uint(x);
    return x != x ? (unsigned short)0x7FC0u : (unsigned short)((u + 0x7FFFu + ((u >> 16) & 1u)) >> 16);
  }
};
template <> struct Put<_Float16> {
  static __device__ __forceinline__ _Float16 from(_Float16 x) { return x; }
  static __device__ __forceinline__ _Float16 from(float x) { return (_Float16)x; }
};

// Source row p of src [R, d] becomes row dest[p] (dest == nullptr: row0 + p) of gallery [N, d], and norms[row] (when given) the norm
// rt_norms_kernel computes on the stored row: one wave per row, four rows per workgroup, row_sumsq on what was stored.  A lane reads
// back exactly the elements it stored itself (the same striding), so program order is all the ordering the read needs.  A destination
// outside [0, N) skips the row (the whole wave: the row number is uniform in it).
template <typename S, typename G>
__global__ __launch_bounds__(256) void rt_put_kernel(const S* __restrict__ src, int R, int d, const int* __restrict__ dest, int row0, G* gallery,
                                                     int N, float* norms) {
  const int lane = threadIdx.x & 63, p = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (p >= R) return;
  const int row = dest ? dest[p] : row0 + p;
  if (row < 0 || row >= N) return;
  const S* s = src + (long)p * d;
  G* g = gallery + (long)row * d;
  for (int c = lane; c < d; c += 64) g[c] = Put<G>::from(s[c]);
  if (norms) {
    const float sq = row_sumsq((const G*)g, d, lane);
    if (lane == 0) norms[row] = sqrtf(sq);
  }
}

template <typename S, typename G>
int put_launch(const void* src, int R, int d, const int32_t* dest, int row0, void* gallery, int N, float* norms, hipStream_t st) {
  hipLaunchKernelGGL((rt_put_kernel<S, G>), dim3((R + 3) / 4), dim3(256), 0, st, (const S*)src, R, d, (const int*)dest, row0, (G*)gallery, N, norms);
  COOT_CHECK_LAUNCH("rt_put");
  return 0;
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
  TkWs w; size_t off = 0;
  auto take = [&](size_t n) { char* p = base ? (char*)base + off : nullptr; off += (n + 255) & ~(size_t)255; return (void*)p; };
  w.na = (float*)take((size_t)M * 4); w.nb = (float*)take((size_t)N * 4);
  w.part = (tk_entry_t*)take(S > 1 ? (size_t)M * S * K * 8 : 0);
  w.bytes = off;
  return w;
}

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
constexpr int FEW_MAX = COOT_RETRIEVAL_FEW_MAX;  // queries
constexpr int FR = 128;                          // gallery rows per step = threads per workgroup
constexpr int FEW_SMAX = 1024;                   // row splits: about four workgroups per CU
constexpr int FEW_G = 32;                        // lists per merge workgroup
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

// one chunk of the chain for the thread's gallery row: acc[i] = fmaf(q_ik, g_jk, acc[i]) over the chunk's 32 k in order.  The 16-bit
// sweep calls it; the fp32 sweep keeps the same loop in its body, so that its instantiations compile to the instructions they had
template <int MQ>
__device__ __forceinline__ void few_fma_chunk(const float* tile, const float* qs, int tid, float (&acc)[MQ]) {
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
}

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

// row splits and the 128-row blocks each one sweeps: every split has at least one block.  cap bounds S whatever the option says:
// the workspace is sized by it, so it does not depend on the option and stops growing with N.
struct FewPlan { int MQ, S, blocks, cap; };
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
struct FewWs { float *qnorm, *qn; tk_entry_t *part_a, *part_b; size_t bytes; };
FewWs few_layout(void* base, int M, int d, int K, int cap) {
  FewWs w; size_t off = 0;
  auto take = [&](size_t n) { char* p = base ? (char*)base + off : nullptr; off += (n + 255) & ~(size_t)255; return (void*)p; };
  const int dpad = (d + RK - 1) / RK * RK;
  w.qnorm = (float*)take((size_t)FEW_MAX * 4); w.qn = (float*)take((size_t)dpad * FEW_MAX * 4);
  w.part_a = (tk_entry_t*)take(cap > 1 ? (size_t)M * cap * K * 8 : 0);
  w.part_b = (tk_entry_t*)take(cap > FEW_G ? (size_t)M * ((cap + FEW_G - 1) / FEW_G) * K * 8 : 0);
  w.bytes = off;
  return w;
}

template <typename GT, int MQ, bool MASKED>
void few_launch(const FewPlan& p, const FewWs& w, const GT* gallery, const float* gallery_norms, const unsigned char* keep, int M, int N, int d, int K,
                int32_t* idx_out, float* score_out, float* sim_out, hipStream_t st) {
  const int vec = d % (16 / (int)sizeof(GT)) == 0 && ((uintptr_t)gallery & 15) == 0;  // every row starts 16-byte aligned
  const size_t lds = few_lds_bytes(MQ, K);
  if (gallery_norms)
    hipLaunchKernelGGL((rt_few_kernel<GT, MQ, true, MASKED>), dim3(p.S), dim3(FR), lds, st, gallery, gallery_norms, (const float*)w.qn, M, N, d, K,
                       p.blocks, p.S, vec, sim_out, w.part_a, (int*)idx_out, score_out, keep);
  else
    hipLaunchKernelGGL((rt_few_kernel<GT, MQ, false, MASKED>), dim3(p.S), dim3(FR), lds, st, gallery, (const float*)nullptr, (const float*)w.qn, M, N, d,
                       K, p.blocks, p.S, vec, sim_out, w.part_a, (int*)idx_out, score_out, keep);
}
template <typename GT, bool MASKED>
void few_launch_mq(const FewPlan& p, const FewWs& w, const GT* gallery, const float* gallery_norms, const unsigned char* keep, int M, int N, int d, int K,
                   int32_t* idx_out, float* score_out, float* sim_out, hipStream_t st) {
  switch (p.MQ) {
    case 1: few_launch<GT, 1, MASKED>(p, w, gallery, gallery_norms, keep, M, N, d, K, idx_out, score_out, sim_out, st); break;
    case 2: few_launch<GT, 2, MASKED>(p, w, gallery, gallery_norms, keep, M, N, d, K, idx_out, score_out, sim_out, st); break;
    case 4: few_launch<GT, 4, MASKED>(p, w, gallery, gallery_norms, keep, M, N, d, K, idx_out, score_out, sim_out, st); break;
    case 8: few_launch<GT, 8, MASKED>(p, w, gallery, gallery_norms, keep, M, N, d, K, idx_out, score_out, sim_out, st); break;
    default: few_launch<GT, 16, MASKED>(p, w, gallery, gallery_norms, keep, M, N, d, K, idx_out, score_out, sim_out, st); break;
  }
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
  hipLaunchKernelGGL(rt_few_prep_kernel, dim3(FEW_MAX), dim3(64), 0, st, queries, M, d, (d + RK - 1) / RK * RK, gallery_norms != nullptr, w.qnorm, w.qn);
  COOT_CHECK_LAUNCH("rt_few_prep");
  if (keep) few_launch_mq<GT, true>(p, w, gallery, gallery_norms, keep, M, N, d, K, idx_out, score_out, sim_out, st);
  else few_launch_mq<GT, false>(p, w, gallery, gallery_norms, keep, M, N, d, K, idx_out, score_out, sim_out, st);
  COOT_CHECK_LAUNCH("rt_few");
  if (p.S == 1) return 0;
  // merge by rank in rounds of <= FEW_G lists, the two list buffers taking turns
  const tk_entry_t* cur = w.part_a;
  tk_entry_t* nxt = w.part_b;
  int S = p.S;
  while (S > FEW_G) {
    const int So = (S + FEW_G - 1) / FEW_G;
    hipLaunchKernelGGL((rt_few_merge_kernel<false, false>), dim3(So, M), dim3(FEW_MT), (size_t)FEW_G * K * 8, st, cur, S, K, nxt, So, (int*)nullptr, (float*)nullptr);
    COOT_CHECK_LAUNCH("rt_few_merge");
    tk_entry_t* done = nxt; nxt = (tk_entry_t*)cur; cur = done; S = So;
  }
  if (keep)
    hipLaunchKernelGGL((rt_few_merge_kernel<true, true>), dim3(1, M), dim3(FEW_MT), (size_t)S * K * 8, st, cur, S, K, (tk_entry_t*)nullptr, 1, (int*)idx_out,
                       score_out);
  else
    hipLaunchKernelGGL((rt_few_merge_kernel<true, false>), dim3(1, M), dim3(FEW_MT), (size_t)S * K * 8, st, cur, S, K, (tk_entry_t*)nullptr, 1, (int*)idx_out,
                       score_out);
  COOT_CHECK_LAUNCH("rt_few_merge");
  return 0;
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
//   rt_lab_metrics_kernel: rt_metrics_kernel over the entries >= 0 of each vector.
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

// rt_metrics_kernel over the n entries >= 0 of each vector: workgroup 0 = ranks_q [M], ranks in [0, N), hist [N];
// workgroup 1 = ranks_g [N], ranks in [0, M), hist + N [M].  hist zeroed.  n = 0: seven zeros.
__global__ __launch_bounds__(1024) void rt_lab_metrics_kernel(const int* ranks_q, const int* ranks_g, int M, int N, int* hist, float* out) {
  __shared__ unsigned long long s_sum;
  __shared__ int s_cnt[5];  // < 1, < 5, < 10, < 50, n
  __shared__ int s_scan[1024];
  __shared__ int s_med[2];
  const int* ranks = blockIdx.x == 0 ? ranks_q : ranks_g;
  const int len = blockIdx.x == 0 ? M : N, H = blockIdx.x == 0 ? N : M;
  int* h = blockIdx.x == 0 ? hist : hist + N;
  const int tid = threadIdx.x;
  if (tid == 0) { s_sum = 0ull; s_med[0] = -1; s_med[1] = -1; }
  if (tid < 5) s_cnt[tid] = 0;
  __syncthreads();
  unsigned long long ls = 0ull;
  int lc[5] = {0, 0, 0, 0, 0};
  for (int i = tid; i < len; i += 1024) {
    const int r = ranks[i];
    if (r < 0) continue;
    ls += (unsigned long long)r;
    lc[0] += r < 1; lc[1] += r < 5; lc[2] += r < 10; lc[3] += r < 50; ++lc[4];
    if (r < H) atomicAdd(h + r, 1);  // (a rank is < H: never outside hist)
  }
  atomicAdd(&s_sum, ls);
#pragma unroll
  for (int q = 0; q < 5; ++q) if (lc[q]) atomicAdd(&s_cnt[q], lc[q]);
  __threadfence();
  __syncthreads();
  const int n = s_cnt[4];
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
    if (n == 0) {
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

// best and hist are adjacent: one zero fill
struct LabWs { float *na, *nb, *own; tk_entry_t* best; int* hist; size_t zero_bytes, bytes; };
LabWs lab_layout(void* base, int M, int N) {
  LabWs w; size_t off = 0;
  auto take = [&](size_t n) { char* p = base ? (char*)base + off : nullptr; off += (n + 255) & ~(size_t)255; return (void*)p; };
  w.na = (float*)take((size_t)M * 4); w.nb = (float*)take((size_t)N * 4); w.own = (float*)take((size_t)M * 4);
  const size_t z0 = off;
  w.best = (tk_entry_t*)take((size_t)N * 8);
  w.hist = (int*)take(((size_t)N + M) * 4);
  w.zero_bytes = off - z0;
  w.bytes = off;
  return w;
}

// coot_retrieval_topk and coot_retrieval_topk_masked (keep == nullptr: the unmasked kernels, launched as coot_retrieval_topk
// launches them): fn names the entry in a refusal
template <bool MASKED>
void topk_launch(const TkSplit& sp, const TkWs& w, const float* queries, const float* gallery, const unsigned char* keep, int M, int N, int d, int K,
                 int normalize, int32_t* idx_out, float* score_out, float* sim_out, hipStream_t st) {
  const dim3 grid(sp.S, (M + RT - 1) / RT);
  const size_t lds = tk_lds_bytes(K);
  if (normalize)
    hipLaunchKernelGGL((rt_topk_kernel<true, MASKED>), grid, dim3(256), lds, st, queries, gallery, (const float*)w.na, (const float*)w.nb, M, N, d, K,
                       sp.tiles, sp.S, sim_out, w.part, (int*)idx_out, score_out, keep);
  else
    hipLaunchKernelGGL((rt_topk_kernel<false, MASKED>), grid, dim3(256), lds, st, queries, gallery, (const float*)nullptr, (const float*)nullptr, M, N, d,
                       K, sp.tiles, sp.S, sim_out, w.part, (int*)idx_out, score_out, keep);
}
int topk_search(const char* fn, const float* queries, const float* gallery, const unsigned char* keep, int M, int N, int d, int K, int normalize,
                int32_t* idx_out, float* score_out, float* sim_out, void* workspace, size_t workspace_bytes, hipStream_t st) {
  COOT_REQUIRE(queries && gallery && idx_out && score_out && workspace, "%s: null pointer", fn);
  COOT_REQUIRE(M >= 1 && N >= 1 && d >= 1 && (M + RT - 1) / RT <= 65535, "%s: M = %d, N = %d, d = %d", fn, M, N, d);
  COOT_REQUIRE(K >= 1 && K <= N && K <= TK_MAX, "%s: K = %d is outside 1 .. min(N = %d, %d)", fn, K, N, TK_MAX);
  const TkSplit sp = tk_split(M, N);
  TkWs w = tk_layout(workspace, M, N, K, sp.S);
  COOT_REQUIRE(w.bytes <= workspace_bytes, "%s: workspace too small (%zu < %zu)", fn, workspace_bytes, w.bytes);
  if (normalize) {
    hipLaunchKernelGGL(rt_norms_kernel<float>, dim3((M + N + 3) / 4), dim3(256), 0, st, queries, M, gallery, N, d, w.na, w.nb);
    COOT_CHECK_LAUNCH("rt_norms");
  }
  if (keep) topk_launch<true>(sp, w, queries, gallery, keep, M, N, d, K, normalize, idx_out, score_out, sim_out, st);
  else topk_launch<false>(sp, w, queries, gallery, keep, M, N, d, K, normalize, idx_out, score_out, sim_out, st);
  COOT_CHECK_LAUNCH("rt_topk");
  if (sp.S > 1) {
    if (keep)
      hipLaunchKernelGGL(rt_topk_merge_kernel<true>, dim3((M + 3) / 4), dim3(256), 0, st, (const tk_entry_t*)w.part, M, sp.S, K, (int*)idx_out, score_out);
    else
      hipLaunchKernelGGL(rt_topk_merge_kernel<false>, dim3((M + 3) / 4), dim3(256), 0, st, (const tk_entry_t*)w.part, M, sp.S, K, (int*)idx_out, score_out);
    COOT_CHECK_LAUNCH("rt_topk_merge");
  }
  return 0;
}

}  // namespace
void set_rt_topk_splits(int n) { g_rt_topk_splits = n; }
int get_rt_topk_splits() { return g_rt_topk_splits; }
void set_rt_few_splits(int n) { g_rt_few_splits = n; }
int get_rt_few_splits() { return g_rt_few_splits; }
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

int coot_retrieval_row_norms(const float* rows, int N, int d, float* norms, coot_stream_t stream) {
  COOT_REQUIRE(rows && norms, "retrieval_row_norms: null pointer");
  COOT_REQUIRE(N >= 1 && d >= 1, "retrieval_row_norms: N = %d, d = %d", N, d);
  hipLaunchKernelGGL(rt_norms_kernel<float>, dim3((N + 3) / 4), dim3(256), 0, (hipStream_t)stream, rows, N, (const float*)nullptr, 0, d, norms, (float*)nullptr);
  COOT_CHECK_LAUNCH("rt_norms");
  return 0;
}

size_t coot_retrieval_topk_few_workspace_bytes(int M, int N, int d, int K) {
  if (M < 1 || N < 1 || d < 1 || K < 1) return 256;
  return few_layout(nullptr, M, d, K, few_plan(M, N).cap).bytes + 256;
}

int coot_retrieval_topk_few(const float* queries, const float* gallery, const float* gallery_norms, int M, int N, int d, int K, int32_t* idx_out,
                            float* score_out, float* sim_out, void* workspace, size_t workspace_bytes, coot_stream_t stream) {
  return few_search("retrieval_topk_few", queries, gallery, gallery_norms, nullptr, M, N, d, K, idx_out, score_out, sim_out, workspace, workspace_bytes,
                    (hipStream_t)stream);
}

int coot_retrieval_row_norms_h(const void* rows, int dtype, int N, int d, float* norms, coot_stream_t stream) {
  COOT_REQUIRE(dtype == COOT_GALLERY_BF16 || dtype == COOT_GALLERY_F16, "retrieval_row_norms_h: dtype = %d (COOT_GALLERY_BF16 or COOT_GALLERY_F16)", dtype);
  COOT_REQUIRE(rows && norms, "retrieval_row_norms_h: null pointer");
  COOT_REQUIRE(N >= 1 && d >= 1, "retrieval_row_norms_h: N = %d, d = %d", N, d);
  const dim3 grid((N + 3) / 4);
  if (dtype == COOT_GALLERY_BF16)
    hipLaunchKernelGGL(rt_norms_kernel<unsigned short>, grid, dim3(256), 0, (hipStream_t)stream, (const unsigned short*)rows, N,
                       (const unsigned short*)nullptr, 0, d, norms, (float*)nullptr);
  else
    hipLaunchKernelGGL(rt_norms_kernel<_Float16>, grid, dim3(256), 0, (hipStream_t)stream, (const _Float16*)rows, N, (const _Float16*)nullptr, 0, d,
                       norms, (float*)nullptr);
  COOT_CHECK_LAUNCH("rt_norms_h");
  return 0;
}

int coot_retrieval_topk_few_h(const float* queries, const void* gallery, int gallery_dtype, const float* gallery_norms, int M, int N, int d, int K,
                              int32_t* idx_out, float* score_out, float* sim_out, void* workspace, size_t workspace_bytes, coot_stream_t stream) {
  COOT_REQUIRE(gallery_dtype == COOT_GALLERY_BF16 || gallery_dtype == COOT_GALLERY_F16,
               "retrieval_topk_few_h: gallery_dtype = %d (COOT_GALLERY_BF16 or COOT_GALLERY_F16)", gallery_dtype);
  if (gallery_dtype == COOT_GALLERY_BF16)
    return few_search("retrieval_topk_few_h", queries, (const unsigned short*)gallery, gallery_norms, nullptr, M, N, d, K, idx_out, score_out, sim_out, workspace,
                      workspace_bytes, (hipStream_t)stream);
  return few_search("retrieval_topk_few_h", queries, (const _Float16*)gallery, gallery_norms, nullptr, M, N, d, K, idx_out, score_out, sim_out, workspace,
                    workspace_bytes, (hipStream_t)stream);
}

int coot_retrieval_topk_few_masked(const float* queries, const void* gallery, int gallery_dtype, const float* gallery_norms, const uint8_t* keep, int M,
                                   int N, int d, int K, int32_t* idx_out, float* score_out, float* sim_out, void* workspace, size_t workspace_bytes,
                                   coot_stream_t stream) {
  const char* fn = "retrieval_topk_few_masked";
  COOT_REQUIRE(gallery_dtype == COOT_GALLERY_F32 || gallery_dtype == COOT_GALLERY_BF16 || gallery_dtype == COOT_GALLERY_F16,
               "%s: gallery_dtype = %d (COOT_GALLERY_F32, COOT_GALLERY_BF16 or COOT_GALLERY_F16)", fn, gallery_dtype);
  hipStream_t st = (hipStream_t)stream;
  if (gallery_dtype == COOT_GALLERY_F32)
    return few_search(fn, queries, (const float*)gallery, gallery_norms, keep, M, N, d, K, idx_out, score_out, sim_out, workspace, workspace_bytes, st);
  if (gallery_dtype == COOT_GALLERY_BF16)
    return few_search(fn, queries, (const unsigned short*)gallery, gallery_norms, keep, M, N, d, K, idx_out, score_out, sim_out, workspace,
                      workspace_bytes, st);
  return few_search(fn, queries, (const _Float16*)gallery, gallery_norms, keep, M, N, d, K, idx_out, score_out, sim_out, workspace, workspace_bytes, st);
}

int coot_retrieval_rows_put(const void* src, int src_dtype, int R, int d, const int32_t* dest, int row0, void* gallery, int gallery_dtype, int N,
                            float* norms, coot_stream_t stream) {
  const char* fn = "retrieval_rows_put";
  const int F = COOT_GALLERY_F32, B = COOT_GALLERY_BF16, H = COOT_GALLERY_F16;
  COOT_REQUIRE(src && gallery, "%s: null pointer", fn);
  COOT_REQUIRE(R >= 1 && d >= 1 && N >= 1, "%s: R = %d, d = %d, N = %d", fn, R, d, N);
  COOT_REQUIRE((src_dtype == F && (gallery_dtype == F || gallery_dtype == B || gallery_dtype == H)) ||
                   (src_dtype == B && (gallery_dtype == B || gallery_dtype == F)) || (src_dtype == H && (gallery_dtype == H || gallery_dtype == F)),
               "%s: src_dtype = %d, gallery_dtype = %d (fp32 into any of COOT_GALLERY_F32, _BF16, _F16; a 16-bit type into itself or fp32)", fn,
               src_dtype, gallery_dtype);
  if (dest) COOT_REQUIRE(row0 == 0, "%s: row0 = %d with dest (the destinations are dest[p]: row0 has to be 0)", fn, row0);
  else COOT_REQUIRE(row0 >= 0 && row0 <= N && R <= N - row0, "%s: rows [%d, %d + %d) are not inside [0, %d)", fn, row0, row0, R, N);
  hipStream_t st = (hipStream_t)stream;
  if (src_dtype == F && gallery_dtype == F) return put_launch<float, float>(src, R, d, dest, row0, gallery, N, norms, st);
  if (src_dtype == F && gallery_dtype == B) return put_launch<float, unsigned short>(src, R, d, dest, row0, gallery, N, norms, st);
  if (src_dtype == F) return put_launch<float, _Float16>(src, R, d, dest, row0, gallery, N, norms, st);
  if (src_dtype == B && gallery_dtype == B) return put_launch<unsigned short, unsigned short>(src, R, d, dest, row0, gallery, N, norms, st);
  if (src_dtype == B) return put_launch<unsigned short, float>(src, R, d, dest, row0, gallery, N, norms, st);
  if (gallery_dtype == H) return put_launch<_Float16, _Float16>(src, R, d, dest, row0, gallery, N, norms, st);
  return put_launch<_Float16, float>(src, R, d, dest, row0, gallery, N, norms, st);
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
  if (normalize) {
    hipLaunchKernelGGL(rt_norms_kernel<float>, dim3((M + N + 3) / 4), dim3(256), 0, st, queries, M, gallery, N, d, w.na, w.nb);
    COOT_CHECK_LAUNCH("rt_norms");
    hipLaunchKernelGGL(rt_lab_own_kernel<true>, dim3(mt), dim3(256), 0, st, queries, gallery, lab, (const float*)w.na, (const float*)w.nb, M, N, d,
                       w.own, w.best);
  } else {
    hipLaunchKernelGGL(rt_lab_own_kernel<false>, dim3(mt), dim3(256), 0, st, queries, gallery, lab, (const float*)nullptr, (const float*)nullptr, M, N,
                       d, w.own, w.best);
  }
  COOT_CHECK_LAUNCH("rt_lab_own");
  hipLaunchKernelGGL(rt_lab_prepare_kernel, dim3(1), dim3(1024), 0, st, lab, (const tk_entry_t*)w.best, M, N, (int*)ranks_q, (int*)ranks_g,
                     (int*)n_valid);
  COOT_CHECK_LAUNCH("rt_lab_prepare");
  if (normalize) {
    hipLaunchKernelGGL(rt_lab_rank_kernel<true>, dim3(nt, mt), dim3(256), 0, st, queries, gallery, lab, (const float*)w.na, (const float*)w.nb, M, N, d,
                       (const float*)w.own, (const tk_entry_t*)w.best, sim_out, (int*)ranks_q, (int*)ranks_g);
  } else {
    hipLaunchKernelGGL(rt_lab_rank_kernel<false>, dim3(nt, mt), dim3(256), 0, st, queries, gallery, lab, (const float*)nullptr, (const float*)nullptr, M,
                       N, d, (const float*)w.own, (const tk_entry_t*)w.best, sim_out, (int*)ranks_q, (int*)ranks_g);
  }
  COOT_CHECK_LAUNCH("rt_lab_rank");
  if (metrics) {
    hipLaunchKernelGGL(rt_lab_metrics_kernel, dim3(2), dim3(1024), 0, st, (const int*)ranks_q, (const int*)ranks_g, M, N, w.hist, metrics);
    COOT_CHECK_LAUNCH("rt_lab_metrics");
  }
  return 0;
}

}  // extern "C"
