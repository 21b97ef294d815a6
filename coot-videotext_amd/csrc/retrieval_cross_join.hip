// ---- join of two prepared galleries: all row pairs at or above a threshold (coot_retrieval_cross_join_count / _fill) -----------------
// The tile kernel of retrieval_join.hip with two galleries: pair (i, j), row i of the left gallery and row j of the right one, is a hit
// when the left keep lets row i pass, the right keep row j, the groups (if given) differ and s(i, j) >= thr[i].  s(i, j) is the chain of
// rt_range_tile_kernel, so of every search: acc = 0, one fmaf per k in k order, chunks of 32, zero padding beyond d, the chunk and
// N_right, operands x / norm(row) with NORM.  Both operands are the rows as their index stores them, widened as they are staged (a
// 16-bit value widens exactly), and both norms are the stored ones: the left norm is the norm of the widened row, which is what the
// range search computes for the float32 copy of that row.  So the bits are those of right.search_range(left.gallery.float()), without
// the copy and without a norm pass.  There is no diagonal: every block of the right gallery is a candidate for every row tile.
// One call serves a chunk of left rows [row0, row0 + rows), row0 a multiple of 64: its table [rows][nb + 1], nb = ceil(N_right / 128),
// is the table of `rows` queries against N_right rows, which coot_retrieval_range_scan scans unchanged.
//   grid (ceil(nb / blocks_per_wg), row tiles), 256 threads: a workgroup serves left rows i0 .. i0 + 63 and the blocks b0 .. b1 - 1.
//   Staging, prefetch, thread layout (rows 4 ty .. 4 ty + 3, columns tx + 16 c), hit words in LDS by integer OR and computed positions
//   as in rt_join_tile_kernel.  With groups the ids of the 64 + 128 staged rows sit in LDS next to the norms and gate the bit by
//   inequality.
//   FILL = false: table[i][b] = the popcount of both words.  A tile whose 64 rows the left keep masks writes zeros for all its blocks
//     and ends; a block in which the right keep leaves no row is left with zeros, before its first load.
//   FILL = true: a block in which none of the tile's rows has a hit is left before its first load; a hit goes to offs[i] +
//     table[i][b] + the popcount of the row's bits below column j, written only below the capacity.
// No global atomic, no floating-point atomic.  Both keeps and both groups may be null (run-time checks); all are read for rows inside
// the chunk / N_right only.
#include "retrieval.h"

namespace coot {
namespace {

constexpr int JB = COOT_RETRIEVAL_RANGE_BLOCK;  // right rows of a table slot = columns of the tile
static_assert(JB == 2 * RT && RT == 64, "a row's hit bits of a block are two 64-bit words");
constexpr int CROSS_WGS = 1 << 20;  // above this many workgroups a workgroup walks several blocks

// static LDS: As [64][33] | Bs [128][33] | hw [2][64] | gA [64] | gB [128], 27 392 bytes, and with NORM nAs [64] | nBs [128]: 28 160.
// Registers (tools/kernel_resources.py; the nine element pairs alike), count / fill: 217 / 235 VGPRs, with norms 224 / 242, no scratch:
// two waves per SIMD = two workgroups per CU everywhere, as rt_join_tile_kernel (which has the j > i gate on top: 222 / 241, 228 / 247).
// Thresholds, keep flags and ids are read after the chain, as there.
template <typename TA, typename TB, bool NORM, bool FILL>
__global__ __launch_bounds__(256) void rt_cross_join_kernel(const TA* __restrict__ A, const float* __restrict__ anorm, const TB* __restrict__ B,
                                                            const float* __restrict__ bnorm, const unsigned char* __restrict__ keepA,
                                                            const unsigned char* __restrict__ keepB, const int* __restrict__ groupsA,
                                                            const int* __restrict__ groupsB, const float* __restrict__ thr, int row0, int rows,
                                                            int N, int d, int blocks_per_wg, int* __restrict__ table,
                                                            const long long* __restrict__ offs, long long capacity, int* __restrict__ rows_out,
                                                            float* __restrict__ scores_out) {
  __shared__ float As[RT][RP], Bs[JB][RP];
  __shared__ float nAs[RT], nBs[JB];        // NORM: the norms of the staged rows (1 beyond the chunk / N: those rows are staged as zeros)
  __shared__ int gA[RT], gB[JB];            // groups: the ids of the staged rows
  __shared__ unsigned long long hw[2][RT];  // hw[h][r]: the hit bits of row r of the row tile in columns 64 h .. 64 h + 63 of the block
  const int tid = threadIdx.x, ty = tid >> 4, tx = tid & 15;
  const int sr = tid >> 5, sk = tid & 31;  // staging: column sk of the chunk, rows sr + 8 q
  const int i0 = row0 + blockIdx.y * RT, iend = row0 + rows;  // (iend <= N_left)
  const int nb = (N + JB - 1) / JB, stride = nb + 1;
  const int b0 = blockIdx.x * blocks_per_wg, b1 = min(nb, b0 + blocks_per_wg);
  auto slot = [&](int b) -> int& { return table[(long)(i0 - row0 + tid) * stride + b]; };  // of tile row tid (tid < 64) and block b
  if constexpr (!FILL) {
    if (keepA) {  // (uniform) no row of the tile asks: zeros for all its blocks
      if (!__syncthreads_or(tid < RT && i0 + tid < iend && keepA[i0 + tid])) {
        if (tid < RT && i0 + tid < iend)
          for (int b = b0; b < b1; ++b) slot(b) = 0;
        return;
      }
    }
  }
  for (int b = b0; b < b1; ++b) {
    const int j0 = b * JB;
    if constexpr (FILL) {  // (uniform: nothing of a block without a hit is touched)
      int any = 0;
      if (tid < RT && i0 + tid < iend) any = slot(b + 1) - slot(b);
      if (!__syncthreads_or(any)) continue;
    } else if (keepB) {
      if (!__syncthreads_or(tid < JB && j0 + tid < N && keepB[j0 + tid])) {
        if (tid < RT && i0 + tid < iend) slot(b) = 0;
        continue;
      }
    }
    if (tid < JB) {
      (&hw[0][0])[tid] = 0ull;
      if (NORM) nBs[tid] = j0 + tid < N ? bnorm[j0 + tid] : 1.f;
      if (groupsB) gB[tid] = j0 + tid < N ? groupsB[j0 + tid] : 0;
    } else if (tid < JB + RT) {
      if (NORM) nAs[tid - JB] = i0 + tid - JB < iend ? anorm[i0 + tid - JB] : 1.f;
      if (groupsA) gA[tid - JB] = i0 + tid - JB < iend ? groupsA[i0 + tid - JB] : 0;
    }
    TA pa[8];
    TB pb[16];
    // one chunk into registers.  No branch: an address beyond the chunk, N or d is clamped into its gallery and its value is dropped at staging
    auto load = [&](int k0) {
      const int k = min(k0 + sk, d - 1);
#pragma unroll
      for (int q = 0; q < 8; ++q) pa[q] = A[(long)min(i0 + sr + 8 * q, iend - 1) * d + k];
#pragma unroll
      for (int q = 0; q < 16; ++q) pb[q] = B[(long)min(j0 + sr + 8 * q, N - 1) * d + k];
    };
    float acc[4][8];
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
      for (int c = 0; c < 8; ++c) acc[r][c] = 0.f;
    load(0);
    __syncthreads();  // the norms and ids are in LDS, the words are cleared
    for (int k0 = 0; k0 < d; k0 += RK) {
      // stage 64 x 32 of the row tile and 128 x 32 of the block; rows beyond the chunk / N and columns beyond d are zero
      const bool kin = k0 + sk < d;
#pragma unroll
      for (int q = 0; q < 8; ++q) {
        const int r = sr + 8 * q;
        As[r][sk] = (kin && i0 + r < iend) ? (NORM ? widen(pa[q]) / nAs[r] : widen(pa[q])) : 0.f;
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
    // which pairs may be hits is read after the chain, so that nothing of it occupies a register under the FMAs
    unsigned kp = 0u;  // bit c: column j0 + tx + 16 c exists and passes the right keep
#pragma unroll
    for (int c = 0; c < 8; ++c) kp |= (j0 + tx + 16 * c < N && (!keepB || keepB[j0 + tx + 16 * c])) ? 1u << c : 0u;
    unsigned mine = 0u;  // byte r: this thread's hit bits of row 4 ty + r, bit c = column tx + 16 c
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int i = i0 + 4 * ty + r;
      const bool rin = i < iend && (!keepA || keepA[i]);  // row i is in the chunk and passes the left keep
      const float th = rin ? thr[i] : 0.f;
      unsigned ok = rin ? kp : 0u;  // bit c: the pair may be a hit
      if (groupsA) {
        const int ga = gA[4 * ty + r];
#pragma unroll
        for (int c = 0; c < 8; ++c) ok &= gB[tx + 16 * c] != ga ? ~0u : ~(1u << c);
      }
      unsigned hit = 0u;
#pragma unroll
      for (int c = 0; c < 8; ++c) hit |= ((ok >> c & 1u) && acc[r][c] >= th) ? 1u << c : 0u;
      unsigned long long w[2] = {0ull, 0ull};
#pragma unroll
      for (int c = 0; c < 8; ++c) w[c >> 2] |= (unsigned long long)(hit >> c & 1u) << (tx + 16 * (c & 3));
      if (w[0]) atomicOr(&hw[0][4 * ty + r], w[0]);
      if (w[1]) atomicOr(&hw[1][4 * ty + r], w[1]);
      mine |= hit << (8 * r);
    }
    __syncthreads();
    if constexpr (!FILL) {
      if (tid < RT && i0 + tid < iend) slot(b) = __popcll(hw[0][tid]) + __popcll(hw[1][tid]);
    } else {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        if (!(mine >> (8 * r) & 255u)) continue;  // (a hit implies i < iend and j < N)
        const int i = i0 + 4 * ty + r;
        const unsigned long long w0 = hw[0][4 * ty + r], w1 = hw[1][4 * ty + r];
        const long long base = offs[i - row0] + table[(long)(i - row0) * stride + b];
#pragma unroll
        for (int c = 0; c < 8; ++c) {
          if (!(mine >> (8 * r + c) & 1u)) continue;
          const unsigned long long below = (1ull << (tx + 16 * (c & 3))) - 1ull;
          const long long pos = base + (c < 4 ? __popcll(w0 & below) : __popcll(w0) + __popcll(w1 & below));
          if ((unsigned long long)pos < (unsigned long long)capacity) { rows_out[pos] = j0 + tx + 16 * c; scores_out[pos] = acc[r][c]; }  // (nor below 0)
        }
      }
    }
    __syncthreads();  // the words are read: the next block may clear them
  }
}

bool dtype_ok(int code) { return code == COOT_GALLERY_F32 || code == COOT_GALLERY_BF16 || code == COOT_GALLERY_F16; }

template <bool FILL>
int cross_join(const char* fn, const void* left, int left_dtype, const float* left_norms, const void* right, int right_dtype,
               const float* right_norms, const unsigned char* left_keep, const unsigned char* right_keep, const int32_t* left_groups,
               const int32_t* right_groups, const float* thresholds, int row0, int rows, int NL, int NR, int d, int32_t* table,
               const int64_t* offsets, int64_t capacity, int32_t* rows_out, float* scores_out, hipStream_t st) {
  COOT_REQUIRE(dtype_ok(left_dtype) && dtype_ok(right_dtype),
               "%s: left_dtype = %d, right_dtype = %d (COOT_GALLERY_F32, COOT_GALLERY_BF16 or COOT_GALLERY_F16)", fn, left_dtype, right_dtype);
  COOT_REQUIRE(left && right && thresholds && table && (!FILL || (offsets && rows_out && scores_out)), "%s: null pointer", fn);
  COOT_REQUIRE((left_norms != nullptr) == (right_norms != nullptr), "%s: left_norms and right_norms: both or neither", fn);
  COOT_REQUIRE((left_groups != nullptr) == (right_groups != nullptr), "%s: left_groups and right_groups: both or neither", fn);
  COOT_REQUIRE(NL >= 1 && NR >= 1 && d >= 1, "%s: N_left = %d, N_right = %d, d = %d", fn, NL, NR, d);
  COOT_REQUIRE(row0 >= 0 && row0 % RT == 0 && rows >= 1 && row0 < NL && rows <= NL - row0 && (rows + RT - 1) / RT <= 65535,
               "%s: row0 = %d (a multiple of %d), rows = %d (1 .. min(N_left - row0, %d)), N_left = %d", fn, row0, RT, rows, 65535 * RT, NL);
  COOT_REQUIRE(capacity >= 0, "%s: capacity = %lld is negative", fn, (long long)capacity);
  const int mt = (rows + RT - 1) / RT, nb = (NR + JB - 1) / JB;
  const int per = (int)(((long long)nb * mt + CROSS_WGS - 1) / CROSS_WGS);  // 1 up to 2^20 workgroups
  const dim3 grid((nb + per - 1) / per, mt);
  with_elem(left_dtype, [&](auto ta) {
    using TA = typename decltype(ta)::type;
    with_elem(right_dtype, [&](auto tb) {
      using TB = typename decltype(tb)::type;
      with_bool(left_norms != nullptr, [&](auto norm) {
        hipLaunchKernelGGL((rt_cross_join_kernel<TA, TB, decltype(norm)::value, FILL>), grid, dim3(256), 0, st, (const TA*)left, left_norms,
                           (const TB*)right, right_norms, left_keep, right_keep, (const int*)left_groups, (const int*)right_groups, thresholds,
                           row0, rows, NR, d, per, (int*)table, (const long long*)offsets, (long long)capacity, (int*)rows_out, scores_out);
      });
    });
  });
  COOT_CHECK_LAUNCH(FILL ? "rt_cross_join (fill)" : "rt_cross_join (count)");
  return 0;
}

}  // namespace
}  // namespace coot

using namespace coot;

extern "C" {

int coot_retrieval_cross_join_count(const void* left, int left_dtype, const float* left_norms, const void* right, int right_dtype,
                                    const float* right_norms, const uint8_t* left_keep, const uint8_t* right_keep, const int32_t* left_groups,
                                    const int32_t* right_groups, const float* thresholds, int row0, int rows, int N_left, int N_right, int d,
                                    int32_t* block_counts, coot_stream_t stream) {
  return cross_join<false>("retrieval_cross_join_count", left, left_dtype, left_norms, right, right_dtype, right_norms, left_keep, right_keep,
                           left_groups, right_groups, thresholds, row0, rows, N_left, N_right, d, block_counts, nullptr, 0, nullptr, nullptr,
                           (hipStream_t)stream);
}

int coot_retrieval_cross_join_fill(const void* left, int left_dtype, const float* left_norms, const void* right, int right_dtype,
                                   const float* right_norms, const uint8_t* left_keep, const uint8_t* right_keep, const int32_t* left_groups,
                                   const int32_t* right_groups, const float* thresholds, int row0, int rows, int N_left, int N_right, int d,
                                   const int32_t* block_base, const int64_t* offsets, int64_t capacity, int32_t* rows_out, float* scores_out,
                                   coot_stream_t stream) {
  return cross_join<true>("retrieval_cross_join_fill", left, left_dtype, left_norms, right, right_dtype, right_norms, left_keep, right_keep,
                          left_groups, right_groups, thresholds, row0, rows, N_left, N_right, d, (int32_t*)block_base, offsets, capacity,
                          rows_out, scores_out, (hipStream_t)stream);
}

}  // extern "C"
