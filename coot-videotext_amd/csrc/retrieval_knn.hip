// ---- K best partners of every row of a prepared gallery, in a second gallery or in itself (coot_retrieval_knn_join) -------------------
// The staging of rt_cross_join_kernel (retrieval_cross_join.hip) with the selection of rt_topk_kernel (retrieval_tile.hip) behind it.
// Pair (i, j), row i of the left gallery and row j of the right one, is eligible when the left keep lets row i pass, the right keep row
// j, the groups (if given) differ and (exclude_same_row) j != i.  Row i of the result is the K best eligible j by the order of every
// search here: score descending, then the larger row; fewer than K eligible rows leave a tail of -1 / -inf, and a left row that its keep
// masks is -1 / -inf throughout.  s(i, j) is the chain of every search: acc = 0, one fmaf per k in k order, chunks of 32, zero padding
// beyond d, the chunk and N_right, operands x / norm(row) with NORM.  Both operands are the rows as their index stores them, widened as
// they are staged, and both norms are the stored ones, so the bits are those of the right index's search with the widened left rows as
// queries, without the copy and without a norm pass.
//   grid (S, row tiles), 256 threads: a workgroup serves left rows i0 .. i0 + 63 and the 128-row blocks b0 .. b1 - 1 of the right gallery.
//   Staging, prefetch and thread layout (rows 4 ty .. 4 ty + 3, columns tx + 16 c, 4 x 8 accumulators, the next chunk's global loads in
//   flight under the FMAs) are rt_cross_join_kernel's; tile_dot is not called.  Keep flags, ids and j != i are read after the chain.
//   Per row a sorted list of <= K entries; an accumulator that is eligible and beats the row's K-th entry is appended to the row's
//   candidate buffer (an LDS counter hands out the slot: the buffer's order depends on the schedule, its content does not), and one wave
//   per row folds the candidates in by rank (TkFold).  A fold takes <= 64 candidates and a block has 128 columns, so a block is folded
//   in two halves, columns c < 4 and c >= 4; a half in which no thread appended is not folded (uniform vote).
//   A block in which the right keep leaves no row is skipped before its first load; a tile whose 64 left rows are all masked writes its
//   unfilled lists and ends.  S == 1 writes idx / scores, S > 1 the lists part [N_left][S][K], which rt_few_merge_lists merges.
// Dynamic LDS: As [64][33] | Bs [128][33] | nAs [64] | nBs [128] | gA [64] | gB [128] | cnt [64] | ncand [64] (27 392 bytes) |
//   cand [64][64] (32 768) | list [64][K] (512 K): 60 672 bytes at K = 1, 65 280 at K = 10, 125 696 at K = 128; two workgroups per CU fit
//   up to K = 41.
// Registers (tools/kernel_resources.py, gfx950; the nine element pairs alike): 227 VGPRs without norms, 230 with, no scratch: two waves
//   per SIMD = two workgroups per CU by registers, as rt_cross_join_kernel, and the LDS allows the second one up to K = 41.
// No MFMA, no split k, no global atomic, no floating-point atomic: the bytes depend on neither S, the schedule nor a row's batch-mates.
#include "retrieval.h"

namespace coot {
namespace {

constexpr int KB = COOT_RETRIEVAL_RANGE_BLOCK;  // right rows of one step = columns of the tile
static_assert(KB == 2 * RT && RT == 64, "a block is folded in two halves of 64 columns, the most a fold takes");
constexpr int KNN_SMAX = 32;          // splits of the right gallery: one merge round (FEW_G lists)
// The automatic split count: about eight workgroups per CU, and no share shorter than 8 blocks.  From the sweep of
// tools/knn_join_bench.py --sweep 1 (profiles/r30_knn_join_sweep.json, K = 10): 282 row tiles x 141 blocks are fastest at S = 8 (8.4 ms;
// S = 4: 9.2, S = 16: 8.5, S = 32: 9.0); 32 row tiles x 141 blocks at S = 16 (1.09 ms; S = 8: 1.66, S = 32: 1.27: shares of 4 - 5 blocks
// pay more for their lists and the merge than they gain); 32 row tiles x 1 563 blocks at S = 32 (15.9 ms; S = 16: 16.1, S = 8: 26.1).
constexpr int KNN_TARGET_WGS = 2048;
constexpr int KNN_MIN_BLOCKS = 8;
int g_rt_knn_splits = 0;              // coot_set_option("rt_knn_splits", n) (tests); 0 = automatic
constexpr int KNN_MERGE_ROWS = 65535; // rows of one merge call: its grid's y

constexpr size_t KNN_LDS_FIXED = (size_t)(RT + KB) * RP * 4 + (size_t)(RT + KB) * 8 + 2 * RT * 4;
size_t knn_lds_bytes(int K) { return KNN_LDS_FIXED + (size_t)RT * RT * 8 + (size_t)RT * K * 8; }
static_assert(KNN_LDS_FIXED % 8 == 0, "the entries behind the fixed part are 64-bit words");

template <typename TA, typename TB, bool NORM>
__global__ __launch_bounds__(256) void rt_knn_tile_kernel(const TA* __restrict__ A, const float* __restrict__ anorm, const TB* __restrict__ B,
                                                          const float* __restrict__ bnorm, const unsigned char* __restrict__ keepA,
                                                          const unsigned char* __restrict__ keepB, const int* __restrict__ groupsA,
                                                          const int* __restrict__ groupsB, int not_self, int NL, int N, int d, int K,
                                                          int blocks_per_split, int S, tk_entry_t* __restrict__ part, int* __restrict__ idx_out,
                                                          float* __restrict__ score_out) {
  extern __shared__ __attribute__((aligned(16))) char knn_lds[];
  float (*As)[RP] = (float (*)[RP])knn_lds;
  float (*Bs)[RP] = (float (*)[RP])(knn_lds + RT * RP * 4);
  float* nAs = (float*)(knn_lds + (RT + KB) * RP * 4);  // NORM: the norms of the staged rows (1 beyond N_left / N: those rows are staged as zeros)
  float* nBs = nAs + RT;
  int* gA = (int*)(nBs + KB);  // groups: the ids of the staged rows
  int* gB = gA + RT;
  int* cnt = gB + KB;      // entries of a row's list
  int* ncand = cnt + RT;   // candidates of a row that wait for the fold
  tk_entry_t* cand = (tk_entry_t*)(knn_lds + KNN_LDS_FIXED);  // [RT][RT]
  tk_entry_t* list = cand + RT * RT;                          // [RT][K], best first; 0 = behind every entry: an unfilled slot
  const int tid = threadIdx.x, ty = tid >> 4, tx = tid & 15, wave = tid >> 6, lane = tid & 63;
  const int sr = tid >> 5, sk = tid & 31;  // staging: column sk of the chunk, rows sr + 8 q
  const int i0 = blockIdx.y * RT;
  const int nb = (N + KB - 1) / KB;
  int b0 = blockIdx.x * blocks_per_split;
  const int b1 = min(nb, b0 + blocks_per_split);
  if (tid < RT) { cnt[tid] = 0; ncand[tid] = 0; }
  for (int e = tid; e < RT * K; e += 256) list[e] = 0ull;
  if (keepA) {  // (uniform) no row of the tile asks: the unfilled lists are its result
    if (!__syncthreads_or(tid < RT && i0 + tid < NL && keepA[i0 + tid])) b0 = b1;
  }
  for (int b = b0; b < b1; ++b) {
    const int j0 = b * KB;
    if (keepB) {  // (uniform: nothing of this block is touched)
      if (!__syncthreads_or(tid < KB && j0 + tid < N && keepB[j0 + tid])) continue;
    }
    if (tid < KB) {
      if (NORM) nBs[tid] = j0 + tid < N ? bnorm[j0 + tid] : 1.f;
      if (groupsB) gB[tid] = j0 + tid < N ? groupsB[j0 + tid] : 0;
    } else if (tid < KB + RT) {
      if (NORM) nAs[tid - KB] = i0 + tid - KB < NL ? anorm[i0 + tid - KB] : 1.f;
      if (groupsA) gA[tid - KB] = i0 + tid - KB < NL ? groupsA[i0 + tid - KB] : 0;
    }
    TA pa[8];
    TB pb[16];
    // one chunk into registers.  No branch: an address beyond N_left, N or d is clamped into its gallery and its value is dropped at staging
    auto load = [&](int k0) {
      const int k = min(k0 + sk, d - 1);
#pragma unroll
      for (int q = 0; q < 8; ++q) pa[q] = A[(long)min(i0 + sr + 8 * q, NL - 1) * d + k];
#pragma unroll
      for (int q = 0; q < 16; ++q) pb[q] = B[(long)min(j0 + sr + 8 * q, N - 1) * d + k];
    };
    float acc[4][8];
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
      for (int c = 0; c < 8; ++c) acc[r][c] = 0.f;
    load(0);
    __syncthreads();  // the norms and ids are in LDS; the lists and counters of the previous block are settled
    for (int k0 = 0; k0 < d; k0 += RK) {
      // stage 64 x 32 of the row tile and 128 x 32 of the block; rows beyond N_left / N and columns beyond d are zero
      const bool kin = k0 + sk < d;
#pragma unroll
      for (int q = 0; q < 8; ++q) {
        const int r = sr + 8 * q;
        As[r][sk] = (kin && i0 + r < NL) ? (NORM ? widen(pa[q]) / nAs[r] : widen(pa[q])) : 0.f;
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
    // which pairs are eligible is read after the chain, so that nothing of it occupies a register under the FMAs
    unsigned kp = 0u;  // bit c: column j0 + tx + 16 c exists and passes the right keep
#pragma unroll
    for (int c = 0; c < 8; ++c) kp |= (j0 + tx + 16 * c < N && (!keepB || keepB[j0 + tx + 16 * c])) ? 1u << c : 0u;
    unsigned okm = 0u;  // byte r: the eligible pairs of row 4 ty + r, bit c = column tx + 16 c
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int i = i0 + 4 * ty + r;
      const bool rin = i < NL && (!keepA || keepA[i]);  // row i exists and passes the left keep
      unsigned ok = rin ? kp : 0u;
      if (groupsA) {
        const int ga = gA[4 * ty + r];
#pragma unroll
        for (int c = 0; c < 8; ++c) ok &= gB[tx + 16 * c] != ga ? ~0u : ~(1u << c);
      }
      if (not_self) {
#pragma unroll
        for (int c = 0; c < 8; ++c) ok &= j0 + tx + 16 * c != i ? ~0u : ~(1u << c);
      }
      okm |= ok << (8 * r);
    }
#pragma unroll
    for (int h = 0; h < 2; ++h) {  // columns c < 4, then c >= 4: <= 64 candidates per row and fold
      int any = 0;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const unsigned bits = okm >> (8 * r + 4 * h) & 15u;
        if (!bits) continue;
        const int row = 4 * ty + r;
        const bool full = cnt[row] >= K;
        const tk_entry_t kth = list[row * K + K - 1];
#pragma unroll
        for (int cc = 0; cc < 4; ++cc) {
          if (!(bits >> cc & 1u)) continue;
          const tk_entry_t e = tk_pack(acc[r][4 * h + cc], j0 + tx + 16 * (4 * h + cc));
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
    if (i >= NL) continue;
    const tk_entry_t v = list[e];
    if (S == 1) {
      idx_out[(long)i * K + r] = tk_idx_masked(v);
      score_out[(long)i * K + r] = tk_score_masked(v);
    } else {
      part[((long)i * S + blockIdx.x) * K + r] = v;
    }
  }
}

// splits of the right gallery and the blocks each one walks: every split has at least one block
struct KnnPlan { int S, blocks; };
KnnPlan knn_plan(int NL, int NR) {
  const int mt = (NL + RT - 1) / RT, nb = (NR + KB - 1) / KB;
  int S = g_rt_knn_splits;
  if (S <= 0) {
    S = (KNN_TARGET_WGS + mt - 1) / mt;
    S = S > nb / KNN_MIN_BLOCKS ? nb / KNN_MIN_BLOCKS : S;
  }
  S = S < 1 ? 1 : S; S = S > KNN_SMAX ? KNN_SMAX : S; S = S > nb ? nb : S;
  KnnPlan p; p.blocks = (nb + S - 1) / S; p.S = (nb + p.blocks - 1) / p.blocks;
  return p;
}
size_t knn_part_bytes(int NL, int K, int S) { return S > 1 ? (size_t)NL * S * K * sizeof(tk_entry_t) : 0; }

bool dtype_ok(int code) { return code == COOT_GALLERY_F32 || code == COOT_GALLERY_BF16 || code == COOT_GALLERY_F16; }

}  // namespace
void set_rt_knn_splits(int n) { g_rt_knn_splits = n; }
int get_rt_knn_splits() { return g_rt_knn_splits; }
}  // namespace coot

using namespace coot;

extern "C" {

size_t coot_retrieval_knn_join_workspace_bytes(int N_left, int N_right, int K) {
  if (N_left < 1 || N_right < 1 || K < 1 || K > N_right || K > TK_MAX) return 256;
  return knn_part_bytes(N_left, K, knn_plan(N_left, N_right).S) + 256;
}

int coot_retrieval_knn_join(const void* left, int left_dtype, const float* left_norms, const void* right, int right_dtype,
                            const float* right_norms, const uint8_t* left_keep, const uint8_t* right_keep, const int32_t* left_groups,
                            const int32_t* right_groups, int exclude_same_row, int N_left, int N_right, int d, int K, int32_t* idx_out,
                            float* score_out, void* workspace, size_t workspace_bytes, coot_stream_t stream) {
  const char* fn = "retrieval_knn_join";
  hipStream_t st = (hipStream_t)stream;
  COOT_REQUIRE(dtype_ok(left_dtype) && dtype_ok(right_dtype),
               "%s: left_dtype = %d, right_dtype = %d (COOT_GALLERY_F32, COOT_GALLERY_BF16 or COOT_GALLERY_F16)", fn, left_dtype, right_dtype);
  COOT_REQUIRE(left && right && idx_out && score_out && workspace, "%s: null pointer", fn);
  COOT_REQUIRE((left_norms != nullptr) == (right_norms != nullptr), "%s: left_norms and right_norms: both or neither", fn);
  COOT_REQUIRE((left_groups != nullptr) == (right_groups != nullptr), "%s: left_groups and right_groups: both or neither", fn);
  COOT_REQUIRE(exclude_same_row == 0 || exclude_same_row == 1, "%s: exclude_same_row = %d (0 or 1)", fn, exclude_same_row);
  COOT_REQUIRE(N_left >= 1 && N_right >= 1 && d >= 1 && (N_left + RT - 1) / RT <= 65535, "%s: N_left = %d (1 .. %d), N_right = %d, d = %d", fn,
               N_left, 65535 * RT, N_right, d);
  COOT_REQUIRE(K >= 1 && K <= N_right && K <= TK_MAX, "%s: K = %d is outside 1 .. min(N_right = %d, %d)", fn, K, N_right, TK_MAX);
  COOT_REQUIRE(((uintptr_t)workspace & 15) == 0, "%s: workspace is not 16-byte aligned", fn);
  const KnnPlan p = knn_plan(N_left, N_right);
  const size_t need = knn_part_bytes(N_left, K, p.S);
  COOT_REQUIRE(need <= workspace_bytes, "%s: workspace too small (%zu < %zu)", fn, workspace_bytes, need);
  tk_entry_t* part = p.S > 1 ? (tk_entry_t*)workspace : nullptr;
  const dim3 grid(p.S, (N_left + RT - 1) / RT);
  with_elem(left_dtype, [&](auto ta) {
    using TA = typename decltype(ta)::type;
    with_elem(right_dtype, [&](auto tb) {
      using TB = typename decltype(tb)::type;
      with_bool(left_norms != nullptr, [&](auto norm) {
        hipLaunchKernelGGL((rt_knn_tile_kernel<TA, TB, decltype(norm)::value>), grid, dim3(256), knn_lds_bytes(K), st, (const TA*)left, left_norms,
                           (const TB*)right, right_norms, left_keep, right_keep, (const int*)left_groups, (const int*)right_groups,
                           exclude_same_row, N_left, N_right, d, K, p.blocks, p.S, part, (int*)idx_out, score_out);
      });
    });
  });
  COOT_CHECK_LAUNCH("rt_knn_tile");
  // the merge's grid has a row in y: calls of <= 65 535 rows, each on its rows of the lists and of the result
  for (int r0 = 0; p.S > 1 && r0 < N_left; r0 += KNN_MERGE_ROWS) {
    const int rows = N_left - r0 < KNN_MERGE_ROWS ? N_left - r0 : KNN_MERGE_ROWS;
    if (int rc = rt_few_merge_lists(part + (size_t)r0 * p.S * K, nullptr, p.S, rows, K, true, idx_out + (size_t)r0 * K, score_out + (size_t)r0 * K, st))
      return rc;
  }
  return 0;
}

}  // extern "C"
