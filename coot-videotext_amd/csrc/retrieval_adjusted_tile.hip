// ---- adjusted top-K for many queries on a prepared gallery: one tile call (coot_retrieval_topk_adjusted_tile) ------------------------
// coot_retrieval_topk_adjusted (retrieval_adjusted.hip: slices of 16 queries, one sweep of the gallery each) for a whole query set:
// a(i, j) = s(i, j) - offset[j], one fp32 subtraction after the chain, and row i of the result is the K best rows j that keep lets pass
// by a, in the order of every search here (a descending, then the larger row); fewer than K kept rows leave a tail of -1 / -inf.  keep
// gates eligibility, the offset gates nothing: a row at +inf scores -inf and is still a row.  s(i, j) is the chain of every search: acc
// = 0, one fmaf per k in k order, chunks of 32, zero padding beyond d, the chunk and N, operands x / norm(row) with NORM.  The left side
// is the fp32 queries, their norms from rt_launch_norms: the bits the few-query preparation divides by.
//   rt_adjusted_tile_kernel is rt_knn_tile_kernel (retrieval_knn.hip) with a fixed left side (fp32 rows, no left keep, no groups, no
//   j != i) and an offset.  grid (S, row tiles), 256 threads: a workgroup serves queries i0 .. i0 + 63 and the 128-row blocks b0 .. b1 - 1
//   of the gallery.  Staging, prefetch and thread layout (rows 4 ty .. 4 ty + 3, columns tx + 16 c, 4 x 8 accumulators, the next chunk's
//   global loads in flight under the FMAs) are that kernel's.  offset[j] of the block's 128 rows is loaded into LDS at the head of the
//   block and read back after the chain, as the keep flags are: nothing of either occupies a register under the FMAs.
//   Per row a sorted list of <= K entries; a kept column whose tk_pack(acc - off, j) beats the row's K-th entry is appended to the row's
//   candidate buffer (an LDS counter hands out the slot: the buffer's order depends on the schedule, its content does not), and one wave
//   per row folds the candidates in by rank (TkFold), a block in two halves of 64 columns; a half in which no thread appended is not
//   folded (uniform vote).  With sim the raw acc of every in-range pair is written, kept or not, and no block is skipped; without it a
//   block in which keep leaves no row is left before its first load.  S == 1 writes idx / scores, S > 1 the lists part [M][S][K], which
//   rt_few_merge_lists merges.
// Dynamic LDS: As [64][33] | Bs [128][33] | nAs [64] | nBs [128] | offs [128] | cnt [64] | ncand [64] (27 136 bytes) | cand [64][64]
//   (32 768) | list [64][K] (512 K): 60 416 bytes at K = 1, 65 024 at K = 10, 125 440 at K = 128.
// No MFMA, no split k, no global atomic, no floating-point atomic: the bytes depend on neither S, the schedule nor a query's batch-mates.
#include "retrieval.h"

namespace coot {
namespace {

constexpr int AB = COOT_RETRIEVAL_RANGE_BLOCK;  // gallery rows of one step = columns of the tile
static_assert(AB == 2 * RT && RT == 64, "a block is folded in two halves of 64 columns, the most a fold takes");
// the split plan of the k-NN join (retrieval_knn.hip): about eight workgroups per CU, no share under 8 blocks, one merge round
constexpr int ADJT_SMAX = 32;
constexpr int ADJT_TARGET_WGS = 2048;
constexpr int ADJT_MIN_BLOCKS = 8;
int g_rt_adjusted_tile_splits = 0;     // coot_set_option("rt_adjusted_tile_splits", n) (tests); 0 = automatic
constexpr int ADJT_MERGE_ROWS = 65535; // rows of one merge call: its grid's y

constexpr size_t ADJT_LDS_FIXED = (size_t)(RT + AB) * RP * 4 + (size_t)(RT + AB) * 4 + AB * 4 + 2 * RT * 4;
size_t adjt_lds_bytes(int K) { return ADJT_LDS_FIXED + (size_t)RT * RT * 8 + (size_t)RT * K * 8; }
static_assert(ADJT_LDS_FIXED % 8 == 0, "the entries behind the fixed part are 64-bit words");

// keep: may be null (no mask); keep and offset are read for j < N only
template <typename TB, bool NORM>
__global__ __launch_bounds__(256) void rt_adjusted_tile_kernel(const float* __restrict__ A, const float* __restrict__ anorm, const TB* __restrict__ B,
                                                               const float* __restrict__ bnorm, const unsigned char* __restrict__ keep,
                                                               const float* __restrict__ offset, int M, int N, int d, int K, int blocks_per_split,
                                                               int S, float* __restrict__ sim, tk_entry_t* __restrict__ part,
                                                               int* __restrict__ idx_out, float* __restrict__ score_out) {
  extern __shared__ __attribute__((aligned(16))) char adjt_lds[];
  float (*As)[RP] = (float (*)[RP])adjt_lds;
  float (*Bs)[RP] = (float (*)[RP])(adjt_lds + RT * RP * 4);
  float* nAs = (float*)(adjt_lds + (RT + AB) * RP * 4);  // NORM: the norms of the staged rows (1 beyond M / N: those rows are staged as zeros)
  float* nBs = nAs + RT;
  float* offs = nBs + AB;  // the offsets of the block's rows (0 beyond N)
  int* cnt = (int*)(offs + AB);  // entries of a row's list
  int* ncand = cnt + RT;         // candidates of a row that wait for the fold
  tk_entry_t* cand = (tk_entry_t*)(adjt_lds + ADJT_LDS_FIXED);  // [RT][RT]
  tk_entry_t* list = cand + RT * RT;                            // [RT][K], best first; 0 = behind every entry: an unfilled slot
  const int tid = threadIdx.x, ty = tid >> 4, tx = tid & 15, wave = tid >> 6, lane = tid & 63;
  const int sr = tid >> 5, sk = tid & 31;  // staging: column sk of the chunk, rows sr + 8 q
  const int i0 = blockIdx.y * RT;
  const int nb = (N + AB - 1) / AB;
  const int b0 = blockIdx.x * blocks_per_split, b1 = min(nb, b0 + blocks_per_split);
  if (tid < RT) { cnt[tid] = 0; ncand[tid] = 0; }
  for (int e = tid; e < RT * K; e += 256) list[e] = 0ull;
  for (int b = b0; b < b1; ++b) {
    const int j0 = b * AB;
    if (keep && !sim) {  // (uniform: nothing of this block is touched)
      if (!__syncthreads_or(tid < AB && j0 + tid < N && keep[j0 + tid])) continue;
    }
    if (tid < AB) {
      if (NORM) nBs[tid] = j0 + tid < N ? bnorm[j0 + tid] : 1.f;
      offs[tid] = j0 + tid < N ? offset[j0 + tid] : 0.f;
    } else if (tid < AB + RT) {
      if (NORM) nAs[tid - AB] = i0 + tid - AB < M ? anorm[i0 + tid - AB] : 1.f;
    }
    float pa[8];
    TB pb[16];
    // one chunk into registers.  No branch: an address beyond M, N or d is clamped into its matrix and its value is dropped at staging
    auto load = [&](int k0) {
      const int k = min(k0 + sk, d - 1);
#pragma unroll
      for (int q = 0; q < 8; ++q) pa[q] = A[(long)min(i0 + sr + 8 * q, M - 1) * d + k];
#pragma unroll
      for (int q = 0; q < 16; ++q) pb[q] = B[(long)min(j0 + sr + 8 * q, N - 1) * d + k];
    };
    float acc[4][8];
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
      for (int c = 0; c < 8; ++c) acc[r][c] = 0.f;
    load(0);
    __syncthreads();  // the norms and offsets are in LDS; the lists and counters of the previous block are settled
    for (int k0 = 0; k0 < d; k0 += RK) {
      // stage 64 x 32 of the query tile and 128 x 32 of the block; rows beyond M / N and columns beyond d are zero
      const bool kin = k0 + sk < d;
#pragma unroll
      for (int q = 0; q < 8; ++q) {
        const int r = sr + 8 * q;
        As[r][sk] = (kin && i0 + r < M) ? (NORM ? pa[q] / nAs[r] : pa[q]) : 0.f;
      }
#pragma unroll
      for (int q = 0; q < 16; ++q) {
        const int r = sr + 8 * q;
        Bs[r][sk] = (kin && j0 + r < N) ? (NORM ? widen(pb[q]) / nBs[r] : widen(pb[q])) : 0.f;
      }
      __syncthreads();
      if (k0 + RK < d) load(k0 + RK);  // in flight under the FMAs
#pragma unroll 8
      for (int k = 0; k < RK; ++k) {
        float av[4], bv[8];
#pragma unroll
        for (int r = 0; r < 4; ++r) av[r] = As[4 * ty + r][k];
#pragma unroll
        for (int c = 0; c < 8; ++c) bv[c] = Bs[tx + 16 * c][k];
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
          for (int c = 0; c < 8; ++c) acc[r][c] = fmaf(av[r], bv[c], acc[r][c]);
      }
      __syncthreads();
    }
    if (sim) {  // the raw similarity of every pair in range, kept or not
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int i = i0 + 4 * ty + r;
        if (i >= M) continue;
#pragma unroll
        for (int c = 0; c < 8; ++c)
          if (j0 + tx + 16 * c < N) sim[(long)i * N + j0 + tx + 16 * c] = acc[r][c];
      }
    }
    // which columns are eligible is read after the chain, so that nothing of it occupies a register under the FMAs
    unsigned kp = 0u;  // bit c: column j0 + tx + 16 c exists and passes keep
#pragma unroll
    for (int c = 0; c < 8; ++c) kp |= (j0 + tx + 16 * c < N && (!keep || keep[j0 + tx + 16 * c])) ? 1u << c : 0u;
#pragma unroll
    for (int h = 0; h < 2; ++h) {  // columns c < 4, then c >= 4: <= 64 candidates per row and fold
      int any = 0;
      const unsigned bits = kp >> (4 * h) & 15u;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = 4 * ty + r;
        if (!bits || i0 + row >= M) continue;
        const bool full = cnt[row] >= K;
        const tk_entry_t kth = list[row * K + K - 1];
#pragma unroll
        for (int cc = 0; cc < 4; ++cc) {
          if (!(bits >> cc & 1u)) continue;
          const int col = tx + 16 * (4 * h + cc);
          const tk_entry_t e = tk_pack(acc[r][4 * h + cc] - offs[col], j0 + col);
          if (!full || e > kth) { cand[row * RT + atomicAdd(&ncand[row], 1)] = e; any = 1; }
        }
      }
      if (!__syncthreads_or(any)) continue;  // (uniform) nothing to fold: lists and counters stay
      // wave w takes rows w, w + 4, ...; every entry is read before the barrier and placed after it
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
      __syncthreads();  // the lists are settled: the next half compares with them
    }
  }
  __syncthreads();
  for (int e = tid; e < RT * K; e += 256) {
    const int row = e / K, r = e - row * K, i = i0 + row;
    if (i >= M) continue;
    const tk_entry_t v = list[e];
    if (S == 1) {
      idx_out[(long)i * K + r] = tk_idx_masked(v);
      score_out[(long)i * K + r] = tk_score_masked(v);
    } else {
      part[((long)i * S + blockIdx.x) * K + r] = v;
    }
  }
}

// shares of the gallery and the blocks each one walks: every share has at least one block
struct AdjtPlan { int S, blocks; };
AdjtPlan adjt_plan(int M, int N) {
  const int mt = (M + RT - 1) / RT, nb = (N + AB - 1) / AB;
  int S = g_rt_adjusted_tile_splits;
  if (S <= 0) {
    S = (ADJT_TARGET_WGS + mt - 1) / mt;
    S = S > nb / ADJT_MIN_BLOCKS ? nb / ADJT_MIN_BLOCKS : S;
  }
  S = S < 1 ? 1 : S; S = S > ADJT_SMAX ? ADJT_SMAX : S; S = S > nb ? nb : S;
  AdjtPlan p; p.blocks = (nb + S - 1) / S; p.S = (nb + p.blocks - 1) / p.blocks;
  return p;
}
// the query norms and the partial lists
struct AdjtWs { float* na; tk_entry_t* part; size_t bytes; };
AdjtWs adjt_layout(void* base, int M, int K, int S) {
  Arena a{(char*)base}; AdjtWs w;
  w.na = a.take<float>(M);
  w.part = a.take<tk_entry_t>(S > 1 ? (size_t)M * S * K : 0);
  w.bytes = a.off;
  return w;
}

}  // namespace
void set_rt_adjusted_tile_splits(int n) { g_rt_adjusted_tile_splits = n; }
int get_rt_adjusted_tile_splits() { return g_rt_adjusted_tile_splits; }
}  // namespace coot

using namespace coot;

extern "C" {

size_t coot_retrieval_topk_adjusted_tile_workspace_bytes(int M, int N, int d, int K) {
  (void)d;
  if (M < 1 || N < 1 || K < 1 || K > N || K > TK_MAX) return 0;
  return adjt_layout(nullptr, M, K, adjt_plan(M, N).S).bytes;  // exact: the call refuses one byte less
}

int coot_retrieval_topk_adjusted_tile(const float* queries, const void* gallery, int gallery_dtype, const float* gallery_norms, const uint8_t* keep,
                                      const float* offset, int M, int N, int d, int K, int32_t* idx_out, float* score_out, float* sim_out,
                                      void* workspace, size_t workspace_bytes, coot_stream_t stream) {
  const char* fn = "retrieval_topk_adjusted_tile";
  COOT_REQUIRE(gallery_dtype == COOT_GALLERY_F32 || gallery_dtype == COOT_GALLERY_BF16 || gallery_dtype == COOT_GALLERY_F16,
               "%s: gallery_dtype = %d (COOT_GALLERY_F32, COOT_GALLERY_BF16 or COOT_GALLERY_F16)", fn, gallery_dtype);
  COOT_REQUIRE(queries && gallery && offset && idx_out && score_out && workspace, "%s: null pointer", fn);
  COOT_REQUIRE(M >= 1 && N >= 1 && d >= 1 && (M + RT - 1) / RT <= 65535, "%s: M = %d (1 .. %d), N = %d, d = %d", fn, M, 65535 * RT, N, d);
  COOT_REQUIRE(K >= 1 && K <= N && K <= TK_MAX, "%s: K = %d is outside 1 .. min(N = %d, %d)", fn, K, N, TK_MAX);
  COOT_REQUIRE(((uintptr_t)workspace & 15) == 0, "%s: workspace is not 16-byte aligned", fn);
  hipStream_t st = (hipStream_t)stream;
  const AdjtPlan p = adjt_plan(M, N);
  const AdjtWs w = adjt_layout(workspace, M, K, p.S);
  COOT_REQUIRE(w.bytes <= workspace_bytes, "%s: workspace too small (%zu < %zu)", fn, workspace_bytes, w.bytes);
  if (gallery_norms) {  // the queries' norms only: one launch over M rows
    rt_launch_norms(queries, M, nullptr, 0, d, w.na, nullptr, st);
    COOT_CHECK_LAUNCH("rt_norms");
  }
  const dim3 grid(p.S, (M + RT - 1) / RT);
  with_elem(gallery_dtype, [&](auto t) {
    using TB = typename decltype(t)::type;
    with_bool(gallery_norms != nullptr, [&](auto norm) {
      hipLaunchKernelGGL((rt_adjusted_tile_kernel<TB, decltype(norm)::value>), grid, dim3(256), adjt_lds_bytes(K), st, queries, (const float*)w.na,
                         (const TB*)gallery, gallery_norms, keep, offset, M, N, d, K, p.blocks, p.S, sim_out, w.part, (int*)idx_out, score_out);
    });
  });
  COOT_CHECK_LAUNCH("rt_adjusted_tile");
  // the merge's grid has a row in y: calls of <= 65 535 rows, each on its rows of the lists and of the result
  for (int r0 = 0; p.S > 1 && r0 < M; r0 += ADJT_MERGE_ROWS) {
    const int rows = M - r0 < ADJT_MERGE_ROWS ? M - r0 : ADJT_MERGE_ROWS;
    if (int rc = rt_few_merge_lists(w.part + (size_t)r0 * p.S * K, nullptr, p.S, rows, K, true, idx_out + (size_t)r0 * K, score_out + (size_t)r0 * K, st))
      return rc;
  }
  return 0;
}

}  // extern "C"
