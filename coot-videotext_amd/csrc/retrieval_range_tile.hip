// ---- range search for many queries on a prepared gallery (coot_retrieval_range_tile_count / _fill) ---------------------------------
// The range search of retrieval_range.hip on a 64 x 128 tile: the same hit rule, the same table [M][nb + 1] of int32 with one slot per
// (query, 128-row block), the same scan between the two passes (coot_retrieval_range_scan, untouched) and the same CSR result.  s(i, j)
// is the chain of tile_dot (retrieval_tile.hip), which is the chain of rt_few_kernel and rt_range_kernel: acc = 0, one fmaf per k in k
// order, chunks of 32, zero padding beyond d, M and N, operands x / norm(row) with NORM.  So table and result do not depend on which of
// the two routes served a query.  Where the sweep serves 16 queries per pass over the gallery, a workgroup here serves 64 and there is
// no list to merge, so the grid is (blocks x row tiles): every block of the gallery is read once per 64 queries and pass.
//   grid (ceil(nb / blocks_per_wg), row tiles), 256 threads: a workgroup serves the queries i0 .. i0 + 63 and the blocks b0 .. b1 - 1.
//   Staging as in tile_dot (64 x 32 of the queries, 128 x 32 of the block per chunk, the division made as the value is staged), with
//   the next chunk's global loads in flight under the FMAs (an address beyond M, N or d is clamped into the operand and its value is
//   dropped at staging) and the norms of the staged rows in LDS.  Thread (ty, tx) of a 16 x 16 grid owns rows 4 ty .. 4 ty + 3 and the
//   8 columns tx + 16 c of the block: 12 LDS reads for 32 FMAs per k (tile_dot: 8 for 16), and the column reads of a half wave fall
//   into 16 different banks (at columns 4 tx + c two lanes share each bank).  Every element is still one chain of its own.
//   The hit bits of a thread's row go by integer OR into the row's two 64-bit words in LDS (no order); after the barrier word h of a row
//   holds its hit bits of columns 64 h .. 64 h + 63 of the block.
//   FILL = false: table[i][b] = the popcount of both words.  A block in which keep leaves no row is left before its first load with zeros
//     written for the tile's queries.
//   FILL = true: hit (i, j) goes to offs[i] + table[i][b] + the popcount of the row's bits below column j, written only below the
//     capacity (one unsigned compare).  A block in which none of the tile's 64 queries has a hit (table[i][b + 1] == table[i][b]) is
//     left before its first load.
// A position is computed, never claimed: no global atomic, no floating-point atomic.  table is the whole table, offs the offsets of
// all M queries.  keep may be null; it is read for j < N only.
#include "retrieval.h"

namespace coot {
namespace {

constexpr int RB = COOT_RETRIEVAL_RANGE_BLOCK;  // gallery rows of a table slot = columns of the tile
static_assert(RB == 2 * RT && RT == 64, "a row's hit bits of a block are two 64-bit words");
constexpr int RANGE_TILE_WGS = 1 << 20;  // above this many workgroups a workgroup walks several blocks

// static LDS: As [64][33] | Bs [128][33] | hw [2][64], 26 624 bytes, and with NORM nAs [64] | nBs [128]: 27 392.
// Registers (tools/kernel_resources.py; the three element types and both builds alike), count / fill: 214 / 236 VGPRs, with norms
// 221 / 242, no scratch: two waves per SIMD = two workgroups per CU everywhere (32 accumulators, the 24 values of the chunk in flight
// and eight k of LDS reads ahead of their FMAs).
template <typename TB, bool NORM, bool FILL>
__global__ __launch_bounds__(256) void rt_range_tile_kernel(const float* __restrict__ A, const TB* __restrict__ B, const float* __restrict__ nA,
                                                            const float* __restrict__ nB, const float* __restrict__ thr, int M, int N, int d,
                                                            int blocks_per_wg, const unsigned char* __restrict__ keep, int* __restrict__ table,
                                                            const long long* __restrict__ offs, long long capacity, int* __restrict__ rows_out,
                                                            float* __restrict__ scores_out) {
  __shared__ float As[RT][RP], Bs[RB][RP];
  __shared__ float nAs[RT], nBs[RB];        // NORM: the norms of the staged rows (1 beyond M / N: those rows are staged as zeros)
  __shared__ unsigned long long hw[2][RT];  // hw[h][r]: the hit bits of row r of the row tile in columns 64 h .. 64 h + 63 of the block
  const int tid = threadIdx.x, ty = tid >> 4, tx = tid & 15;
  const int sr = tid >> 5, sk = tid & 31;  // staging: column sk of the chunk, rows sr + 8 q
  const int i0 = blockIdx.y * RT, nb = (N + RB - 1) / RB, stride = nb + 1;
  const int b0 = blockIdx.x * blocks_per_wg, b1 = min(nb, b0 + blocks_per_wg);
  float th[4];
  unsigned rin = 0u;  // bit r: row i0 + 4 ty + r is a query
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int i = i0 + 4 * ty + r;
    th[r] = i < M ? thr[i] : 0.f;
    rin |= i < M ? 1u << r : 0u;
  }
  for (int b = b0; b < b1; ++b) {
    const int j0 = b * RB;
    if constexpr (FILL) {  // (uniform: nothing of a block without a hit is touched)
      int any = 0;
      if (tid < RT && i0 + tid < M) any = table[(long)(i0 + tid) * stride + b + 1] - table[(long)(i0 + tid) * stride + b];
      if (!__syncthreads_or(any)) continue;
    } else if (keep) {
      if (!__syncthreads_or(tid < RB && j0 + tid < N && keep[j0 + tid])) {
        if (tid < RT && i0 + tid < M) table[(long)(i0 + tid) * stride + b] = 0;
        continue;
      }
    }
    if (tid < RB) {
      (&hw[0][0])[tid] = 0ull;
      if (NORM) nBs[tid] = j0 + tid < N ? nB[j0 + tid] : 1.f;
    } else if (NORM && tid < RB + RT) {
      nAs[tid - RB] = i0 + tid - RB < M ? nA[i0 + tid - RB] : 1.f;
    }
    unsigned kp = 0u;  // bit c: column j0 + tx + 16 c exists and passes keep
#pragma unroll
    for (int c = 0; c < 8; ++c) kp |= (j0 + tx + 16 * c < N && (!keep || keep[j0 + tx + 16 * c])) ? 1u << c : 0u;
    float pa[8];
    TB pb[16];
    // one chunk into registers.  No branch: an address beyond M, N or d is clamped into the operand and its value is dropped at staging
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
    __syncthreads();  // the norms are in LDS, the words are cleared
    for (int k0 = 0; k0 < d; k0 += RK) {
      // stage 64 x 32 of the queries and 128 x 32 of the block; rows beyond M / N and columns beyond d are zero, as tile_dot stages them
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
    unsigned mine = 0u;  // byte r: this thread's hit bits of row 4 ty + r, bit c = column tx + 16 c
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      unsigned hit = 0u;
#pragma unroll
      for (int c = 0; c < 8; ++c) hit |= ((rin >> r & 1u) && (kp >> c & 1u) && acc[r][c] >= th[r]) ? 1u << c : 0u;
      unsigned long long w[2] = {0ull, 0ull};
#pragma unroll
      for (int c = 0; c < 8; ++c) w[c >> 2] |= (unsigned long long)(hit >> c & 1u) << (tx + 16 * (c & 3));
      if (w[0]) atomicOr(&hw[0][4 * ty + r], w[0]);
      if (w[1]) atomicOr(&hw[1][4 * ty + r], w[1]);
      mine |= hit << (8 * r);
    }
    __syncthreads();
    if constexpr (!FILL) {
      if (tid < RT && i0 + tid < M) table[(long)(i0 + tid) * stride + b] = __popcll(hw[0][tid]) + __popcll(hw[1][tid]);
    } else {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        if (!(mine >> (8 * r) & 255u)) continue;  // (a hit implies i < M and j < N)
        const int i = i0 + 4 * ty + r;
        const unsigned long long w0 = hw[0][4 * ty + r], w1 = hw[1][4 * ty + r];
        const long long base = offs[i] + table[(long)i * stride + b];
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

// the query norms: what a count or fill call needs besides the caller's table
struct RangeTileWs { float* na; size_t bytes; };
RangeTileWs range_tile_layout(void* base, int M) {
  Arena a{(char*)base}; RangeTileWs w;
  w.na = a.take<float>(M);
  w.bytes = a.off;
  return w;
}
bool range_tile_args_ok(int M, int N, int d) { return M >= 1 && (M + RT - 1) / RT <= 65535 && N >= 1 && d >= 1; }

template <bool FILL>
int range_tile(const char* fn, const float* queries, const void* gallery, int gallery_dtype, const float* gallery_norms, const unsigned char* keep,
               const float* thresholds, int M, int N, int d, int32_t* table, const int64_t* offsets, int64_t capacity, int32_t* rows_out,
               float* scores_out, void* workspace, size_t workspace_bytes, hipStream_t st) {
  COOT_REQUIRE(gallery_dtype == COOT_GALLERY_F32 || gallery_dtype == COOT_GALLERY_BF16 || gallery_dtype == COOT_GALLERY_F16,
               "%s: gallery_dtype = %d (COOT_GALLERY_F32, COOT_GALLERY_BF16 or COOT_GALLERY_F16)", fn, gallery_dtype);
  COOT_REQUIRE(queries && gallery && thresholds && table && workspace && (!FILL || (offsets && rows_out && scores_out)), "%s: null pointer", fn);
  COOT_REQUIRE(range_tile_args_ok(M, N, d), "%s: M = %d (1 .. %d), N = %d, d = %d", fn, M, 65535 * RT, N, d);
  COOT_REQUIRE(capacity >= 0, "%s: capacity = %lld is negative", fn, (long long)capacity);
  COOT_REQUIRE(((uintptr_t)workspace & 15) == 0, "%s: workspace is not 16-byte aligned", fn);
  const RangeTileWs w = range_tile_layout(workspace, M);
  COOT_REQUIRE(w.bytes <= workspace_bytes, "%s: workspace too small (%zu < %zu)", fn, workspace_bytes, w.bytes);
  if (gallery_norms) {  // the queries' norms only: one launch over M rows
    rt_launch_norms(queries, M, nullptr, 0, d, w.na, nullptr, st);
    COOT_CHECK_LAUNCH("rt_norms");
  }
  const int mt = (M + RT - 1) / RT, nb = (N + RB - 1) / RB;
  const int per = (int)(((long long)nb * mt + RANGE_TILE_WGS - 1) / RANGE_TILE_WGS);  // 1 up to 2^20 workgroups
  const dim3 grid((nb + per - 1) / per, mt);
  with_elem(gallery_dtype, [&](auto t) {
    using TB = typename decltype(t)::type;
    with_bool(gallery_norms != nullptr, [&](auto norm) {
      hipLaunchKernelGGL((rt_range_tile_kernel<TB, decltype(norm)::value, FILL>), grid, dim3(256), 0, st, queries, (const TB*)gallery,
                         gallery_norms ? (const float*)w.na : nullptr, gallery_norms, thresholds, M, N, d, per, keep, (int*)table,
                         (const long long*)offsets, (long long)capacity, (int*)rows_out, scores_out);
    });
  });
  COOT_CHECK_LAUNCH(FILL ? "rt_range_tile (fill)" : "rt_range_tile (count)");
  return 0;
}

}  // namespace
}  // namespace coot

using namespace coot;

extern "C" {

size_t coot_retrieval_range_tile_workspace_bytes(int M, int N, int d) {
  if (!range_tile_args_ok(M, N, d)) return 256;
  return range_tile_layout(nullptr, M).bytes + 256;  // the query norms only
}

int coot_retrieval_range_tile_count(const float* queries, const void* gallery, int gallery_dtype, const float* gallery_norms, const uint8_t* keep,
                                    const float* thresholds, int M, int N, int d, int32_t* block_counts, void* workspace, size_t workspace_bytes,
                                    coot_stream_t stream) {
  return range_tile<false>("retrieval_range_tile_count", queries, gallery, gallery_dtype, gallery_norms, keep, thresholds, M, N, d, block_counts, nullptr, 0,
                           nullptr, nullptr, workspace, workspace_bytes, (hipStream_t)stream);
}

int coot_retrieval_range_tile_fill(const float* queries, const void* gallery, int gallery_dtype, const float* gallery_norms, const uint8_t* keep,
                                   const float* thresholds, int M, int N, int d, const int32_t* block_base, const int64_t* offsets, int64_t capacity,
                                   int32_t* rows_out, float* scores_out, void* workspace, size_t workspace_bytes, coot_stream_t stream) {
  return range_tile<true>("retrieval_range_tile_fill", queries, gallery, gallery_dtype, gallery_norms, keep, thresholds, M, N, d, (int32_t*)block_base,
                          offsets, capacity, rows_out, scores_out, workspace, workspace_bytes, (hipStream_t)stream);
}

}  // extern "C"
