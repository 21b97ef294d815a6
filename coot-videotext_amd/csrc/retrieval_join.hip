// ---- self-join of a prepared gallery: all row pairs at or above a threshold (coot_retrieval_join_count / _fill) ---------------------
// The tile range search of retrieval_range_tile.hip with the gallery on both sides: pair (i, j), i < j, is a hit when keep lets both
// rows pass, groups (if given) differ and s(i, j) >= thr[i].  s(i, j) is the chain of rt_range_tile_kernel, so of every search: acc = 0,
// one fmaf per k in k order, chunks of 32, zero padding beyond d and N, operands x / norm(row) with NORM.  The A operand is the gallery
// row as the index stores it, widened as it is staged (a 16-bit value widens exactly), and its norm is the stored one: the norm of the
// widened row, which is what the range search computes for the float32 copy of that row.  So the bits are those of
// search_range(gallery.float()), without the copy, without a norm pass and without the half of the pairs left of the diagonal.
// One call serves a chunk of rows [row0, row0 + rows), row0 a multiple of 128: its table [rows][nbc + 1], nbc = nb - row0 / 128, has one
// slot per (row, block at or right of the chunk's first block) and is the table of a gallery of N - row0 rows, which
// coot_retrieval_range_scan scans unchanged.
//   grid (ceil(nbc / blocks_per_wg), row tiles), 256 threads: a workgroup serves rows i0 .. i0 + 63 and the blocks b0 .. b1 - 1.
//   Staging, prefetch, thread layout (rows 4 ty .. 4 ty + 3, columns tx + 16 c), hit words in LDS by integer OR and computed positions
//   as in rt_range_tile_kernel.  A block with 128 (b + 1) <= i0 + 1 holds no j > i for the tile: it is left before its first load, with
//   zeros written by the count pass.  Everywhere else the hit bit is gated by j > i (one compare per accumulator, after the chain).
//   With groups the ids of the 64 + 128 staged rows sit in LDS next to the norms and gate the bit by inequality.
//   FILL = false: table[i][b] = the popcount of both words; a block in which keep leaves no row is left with zeros.
//   FILL = true: a block in which none of the tile's rows has a hit is left; a hit goes to offs[i] + table[i][b] + the popcount of the
//     row's bits below column j, written only below the capacity.
// No global atomic, no floating-point atomic.  keep and groups may be null (run-time checks); both are read for rows < N only.
#include "retrieval.h"

namespace coot {
namespace {

constexpr int JB = COOT_RETRIEVAL_RANGE_BLOCK;  // gallery rows of a table slot = columns of the tile
static_assert(JB == 2 * RT && RT == 64, "a row's hit bits of a block are two 64-bit words");
constexpr int JOIN_WGS = 1 << 20;  // above this many workgroups a workgroup walks several blocks

// static LDS: As [64][33] | Bs [128][33] | hw [2][64] | gA [64] | gB [128], 27 392 bytes, and with NORM nAs [64] | nBs [128]: 28 160.
// Registers (tools/kernel_resources.py; the three element types and both builds alike), count / fill: 222 / 241 VGPRs, with norms
// 228 / 247, no scratch: two waves per SIMD = two workgroups per CU everywhere, as rt_range_tile_kernel.  Thresholds, keep flags and ids
// are read after the chain: held in registers under the FMAs they cost the fill with norms its second wave (255 VGPRs).
template <typename TB, bool NORM, bool FILL>
__global__ __launch_bounds__(256) void rt_join_tile_kernel(const TB* __restrict__ G, const float* __restrict__ gnorm, const float* __restrict__ thr,
                                                           const unsigned char* __restrict__ keep, const int* __restrict__ groups, int row0, int rows,
                                                           int N, int d, int blocks_per_wg, int* __restrict__ table,
                                                           const long long* __restrict__ offs, long long capacity, int* __restrict__ rows_out,
                                                           float* __restrict__ scores_out) {
  __shared__ float As[RT][RP], Bs[JB][RP];
  __shared__ float nAs[RT], nBs[JB];        // NORM: the norms of the staged rows (1 beyond the chunk / N: those rows are staged as zeros)
  __shared__ int gA[RT], gB[JB];            // groups: the ids of the staged rows
  __shared__ unsigned long long hw[2][RT];  // hw[h][r]: the hit bits of row r of the row tile in columns 64 h .. 64 h + 63 of the block
  const int tid = threadIdx.x, ty = tid >> 4, tx = tid & 15;
  const int sr = tid >> 5, sk = tid & 31;  // staging: column sk of the chunk, rows sr + 8 q
  const int i0 = row0 + blockIdx.y * RT, iend = row0 + rows;  // (iend <= N)
  const int bf = row0 / JB, nb = (N + JB - 1) / JB, stride = nb - bf + 1;
  const int b0 = bf + blockIdx.x * blocks_per_wg, b1 = min(nb, b0 + blocks_per_wg);
  auto slot = [&](int b) -> int& { return table[(long)(i0 - row0 + tid) * stride + b - bf]; };  // of tile row tid (tid < 64) and block b
  for (int b = b0; b < b1; ++b) {
    const int j0 = b * JB;
    if (j0 + JB <= i0 + 1) {  // (uniform) left of the diagonal: no j > i for any row of the tile
      if (!FILL && tid < RT && i0 + tid < iend) slot(b) = 0;
      continue;
    }
    if constexpr (FILL) {  // (uniform: nothing of a block without a hit is touched)
      int any = 0;
      if (tid < RT && i0 + tid < iend) any = slot(b + 1) - slot(b);
      if (!__syncthreads_or(any)) continue;
    } else if (keep) {
      if (!__syncthreads_or(tid < JB && j0 + tid < N && keep[j0 + tid])) {
        if (tid < RT && i0 + tid < iend) slot(b) = 0;
        continue;
      }
    }
    if (tid < JB) {
      (&hw[0][0])[tid] = 0ull;
      if (NORM) nBs[tid] = j0 + tid < N ? gnorm[j0 + tid] : 1.f;
      if (groups) gB[tid] = j0 + tid < N ? groups[j0 + tid] : 0;
    } else if (tid < JB + RT) {
      if (NORM) nAs[tid - JB] = i0 + tid - JB < iend ? gnorm[i0 + tid - JB] : 1.f;
      if (groups) gA[tid - JB] = i0 + tid - JB < iend ? groups[i0 + tid - JB] : 0;
    }
    TB pa[8], pb[16];
    // one chunk into registers.  No branch: an address beyond the chunk, N or d is clamped into the gallery and its value is dropped at staging
    auto load = [&](int k0) {
      const int k = min(k0 + sk, d - 1);
#pragma unroll
      for (int q = 0; q < 8; ++q) pa[q] = G[(long)min(i0 + sr + 8 * q, iend - 1) * d + k];
#pragma unroll
      for (int q = 0; q < 16; ++q) pb[q] = G[(long)min(j0 + sr + 8 * q, N - 1) * d + k];
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
    unsigned kp = 0u;  // bit c: column j0 + tx + 16 c exists and passes keep
#pragma unroll
    for (int c = 0; c < 8; ++c) kp |= (j0 + tx + 16 * c < N && (!keep || keep[j0 + tx + 16 * c])) ? 1u << c : 0u;
    unsigned mine = 0u;  // byte r: this thread's hit bits of row 4 ty + r, bit c = column tx + 16 c
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int i = i0 + 4 * ty + r;
      const bool rin = i < iend && (!keep || keep[i]);  // row i is in the chunk and passes keep
      const float th = rin ? thr[i] : 0.f;
      unsigned ok = rin ? kp : 0u;  // bit c: the pair may be a hit
#pragma unroll
      for (int c = 0; c < 8; ++c) ok &= j0 + tx + 16 * c > i ? ~0u : ~(1u << c);
      if (groups) {
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
        const long long base = offs[i - row0] + table[(long)(i - row0) * stride + b - bf];
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

template <bool FILL>
int join(const char* fn, const void* gallery, int gallery_dtype, const float* gallery_norms, const unsigned char* keep, const int32_t* groups,
         const float* thresholds, int row0, int rows, int N, int d, int32_t* table, const int64_t* offsets, int64_t capacity, int32_t* rows_out,
         float* scores_out, hipStream_t st) {
  COOT_REQUIRE(gallery_dtype == COOT_GALLERY_F32 || gallery_dtype == COOT_GALLERY_BF16 || gallery_dtype == COOT_GALLERY_F16,
               "%s: gallery_dtype = %d (COOT_GALLERY_F32, COOT_GALLERY_BF16 or COOT_GALLERY_F16)", fn, gallery_dtype);
  COOT_REQUIRE(gallery && thresholds && table && (!FILL || (offsets && rows_out && scores_out)), "%s: null pointer", fn);
  COOT_REQUIRE(N >= 1 && d >= 1, "%s: N = %d, d = %d", fn, N, d);
  COOT_REQUIRE(row0 >= 0 && row0 % JB == 0 && rows >= 1 && row0 < N && rows <= N - row0 && (rows + RT - 1) / RT <= 65535,
               "%s: row0 = %d (a multiple of %d), rows = %d (1 .. min(N - row0, %d)), N = %d", fn, row0, JB, rows, 65535 * RT, N);
  COOT_REQUIRE(capacity >= 0, "%s: capacity = %lld is negative", fn, (long long)capacity);
  const int mt = (rows + RT - 1) / RT, nbc = (N + JB - 1) / JB - row0 / JB;
  const int per = (int)(((long long)nbc * mt + JOIN_WGS - 1) / JOIN_WGS);  // 1 up to 2^20 workgroups
  const dim3 grid((nbc + per - 1) / per, mt);
  with_elem(gallery_dtype, [&](auto t) {
    using TB = typename decltype(t)::type;
    with_bool(gallery_norms != nullptr, [&](auto norm) {
      hipLaunchKernelGGL((rt_join_tile_kernel<TB, decltype(norm)::value, FILL>), grid, dim3(256), 0, st, (const TB*)gallery, gallery_norms, thresholds,
                         keep, (const int*)groups, row0, rows, N, d, per, (int*)table, (const long long*)offsets, (long long)capacity, (int*)rows_out,
                         scores_out);
    });
  });
  COOT_CHECK_LAUNCH(FILL ? "rt_join_tile (fill)" : "rt_join_tile (count)");
  return 0;
}

}  // namespace
}  // namespace coot

using namespace coot;

extern "C" {

int coot_retrieval_join_count(const void* gallery, int gallery_dtype, const float* gallery_norms, const uint8_t* keep, const int32_t* groups,
                              const float* thresholds, int row0, int rows, int N, int d, int32_t* block_counts, coot_stream_t stream) {
  return join<false>("retrieval_join_count", gallery, gallery_dtype, gallery_norms, keep, groups, thresholds, row0, rows, N, d, block_counts, nullptr, 0,
                     nullptr, nullptr, (hipStream_t)stream);
}

int coot_retrieval_join_fill(const void* gallery, int gallery_dtype, const float* gallery_norms, const uint8_t* keep, const int32_t* groups,
                             const float* thresholds, int row0, int rows, int N, int d, const int32_t* block_base, const int64_t* offsets,
                             int64_t capacity, int32_t* rows_out, float* scores_out, coot_stream_t stream) {
  return join<true>("retrieval_join_fill", gallery, gallery_dtype, gallery_norms, keep, groups, thresholds, row0, rows, N, d, (int32_t*)block_base,
                    offsets, capacity, rows_out, scores_out, (hipStream_t)stream);
}

}  // extern "C"
