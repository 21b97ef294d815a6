// ---- range search for a few queries on a prepared gallery (coot_retrieval_range_count / _scan / _fill) ----------------------------
// Which rows score at least t, however many there are: row j is a hit of query i when it passes keep and s(i, j) >= t[i] (an IEEE fp32
// compare: a NaN on either side is no hit, -0 >= +0 holds), s(i, j) being rt_few_kernel's chain, so the bits every top-K search ranks
// on.  The result is CSR: offsets int64 [M + 1], and per query its hit rows in ascending order with their scores.  Nothing goes
// through a global atomic: a hit's position is computed, not claimed, so the bytes do not depend on the schedule, on the batch-mates
// of a query or on the sweep's splits.
//   rt_few_prep_kernel (retrieval_few.hip): the operand table, as in the few-query search.
//   rt_range_kernel<.., FILL = false>, the count pass: rt_scoped_kernel's staging and chain (one body for the three element types), one
//     thread per row of a 128-row block.  The hit bit of the thread's row for query i is gathered by a 64-lane ballot; the popcounts of
//     the two waves meet in LDS and one int32 per (query, block) goes into the table [M][nb + 1].  A block in which keep leaves no row
//     is left before its first gallery load with zeros in the table.
//   rt_range_scan_kernel: per query the exclusive prefix of its block counts, in place, the total in slot nb (int32: a query has at
//     most N < 2^31 hits); rt_range_offsets_kernel: the int64 prefix over the totals, offsets [M + 1] (M x N can exceed 2^31).
//   rt_range_kernel<.., FILL = true>, the fill pass: the same chain again, so the same bits and the same ballots.  A hit goes to
//     offsets[i] + base[i][b] + (hits of lower rows in the block): the popcount of the ballot below the lane, plus wave 0's count for
//     wave 1.  Written only below the capacity.  A block in which no query of the call has a hit (base[i][b + 1] == base[i][b] for all
//     i, read from the table) is left before its first gallery load: with a selective threshold the pass reads a few blocks.
// The table of a search of more than 16 queries is one buffer; count and fill serve 16 rows of it per call and the scan all of them.
#include "retrieval.h"

namespace coot {
namespace {

static_assert(FR == COOT_RETRIEVAL_RANGE_BLOCK, "the table a C caller sizes has one slot per block of the sweep");
static_assert(FR == 128, "two waves per workgroup: wave 1 ranks behind wave 0's count");
constexpr int RANGE_SCAN_T = 256;  // threads of the two scan kernels

// grid (S), 128 threads; MQ, GT, NORM as in rt_scoped_kernel; static LDS: tile [FR][RP] | qs [RK][16] | th [16] | w0 [16], 19 072 bytes
// (rt_scoped_kernel at K = 10, 16 accumulators: 20 416).  table: the M rows [nb + 1] of this call's queries, row stride nb + 1;
// offs [M], rows_out, scores_out: FILL only.  keep may be null; it is read for j < N only.
// Registers at 16 accumulators (tools/kernel_resources.py, both builds alike), count / fill: fp32 120 / 124 VGPRs (128 / 132 with norms),
// 16-bit 113 / 118 (117 / 121), no scratch; LDS 19 328 bytes.  Four waves per SIMD = eight workgroups per CU everywhere but the fp32
// fill with norms (132 VGPRs: three).  rt_scoped_kernel holds 222 - 230 (fp32) and 155 - 158 (16-bit) VGPRs at the same width, two and
// three waves: without candidate lists behind the chain the sweep needs less LDS and about 100 fewer registers.
template <typename GT, int MQ, bool NORM, bool FILL>
__global__ __launch_bounds__(FR) void rt_range_kernel(const GT* __restrict__ G, const float* __restrict__ gnorm, const float* __restrict__ qn,
                                                      const float* __restrict__ thr, int M, int N, int d, int blocks_per_split, int vec,
                                                      const unsigned char* __restrict__ keep, int* __restrict__ table,
                                                      const long long* __restrict__ offs, long long capacity, int* __restrict__ rows_out,
                                                      float* __restrict__ scores_out) {
  constexpr int EPL = 16 / (int)sizeof(GT), TPR = RK / EPL, RPP = FR / TPR, NQ = FR / RPP;
  __shared__ __attribute__((aligned(16))) float tile[FR * RP];
  __shared__ __attribute__((aligned(16))) float qs[RK * FEW_MAX];
  __shared__ float th[FEW_MAX];
  __shared__ int w0[FEW_MAX];  // wave 0's hits of the block, per query
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int nb = (N + FR - 1) / FR, nchunks = (d + RK - 1) / RK, stride = nb + 1;
  const int b0 = blockIdx.x * blocks_per_split, b1 = min(nb, b0 + blocks_per_split);
  const int sr = tid / TPR, sk = (tid % TPR) * EPL;
  if (tid < FEW_MAX) th[tid] = tid < M ? thr[tid] : 0.f;
  __syncthreads();
  for (int b = b0; b < b1; ++b) {
    const int j0 = b * FR, j = j0 + tid;
    const bool kept = j < N && (!keep || keep[j]);
    if (FILL) {  // (uniform: nothing of a block without a hit is touched)
      int any = 0;
      if (tid < M) any = table[(long)tid * stride + b + 1] - table[(long)tid * stride + b];
      if (!__syncthreads_or(any)) continue;
    } else if (keep) {
      if (!__syncthreads_or(kept)) {
        if (tid < M) table[(long)tid * stride + b] = 0;
        continue;
      }
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
    // the hit bits of the wave's 64 rows, per query (uniform words); w0 is free: its readers of the block before passed a barrier since
    unsigned long long bal[MQ];
#pragma unroll
    for (int i = 0; i < MQ; ++i) {
      bal[i] = __ballot(i < M && kept && acc[i] >= th[i]);
      if (wave == 0 && lane == 0) w0[i] = __popcll(bal[i]);
    }
    __syncthreads();
    if (!FILL) {
      if (wave == 1 && lane == 0) {
#pragma unroll
        for (int i = 0; i < MQ; ++i)
          if (i < M) table[(long)i * stride + b] = w0[i] + __popcll(bal[i]);
      }
    } else {
      const unsigned long long below = (1ull << lane) - 1ull;
#pragma unroll
      for (int i = 0; i < MQ; ++i) {
        if (bal[i] >> lane & 1ull) {  // (implies i < M and j < N)
          const long long pos = offs[i] + table[(long)i * stride + b] + (wave ? w0[i] : 0) + __popcll(bal[i] & below);
          if ((unsigned long long)pos < (unsigned long long)capacity) { rows_out[pos] = j; scores_out[pos] = acc[i]; }  // (nor below 0)
        }
      }
    }
  }
}

// grid (M), 256 threads: row i of the table [M][nb + 1] becomes the exclusive prefix of its nb counts, slot nb their sum (= counts_out[i])
__global__ __launch_bounds__(RANGE_SCAN_T) void rt_range_scan_kernel(int* __restrict__ table, int nb, int* __restrict__ counts_out) {
  __shared__ int part[RANGE_SCAN_T];
  const int tid = threadIdx.x;
  int* row = table + (long)blockIdx.x * (nb + 1);
  const int per = (nb + RANGE_SCAN_T - 1) / RANGE_SCAN_T, b0 = min(nb, tid * per), b1 = min(nb, b0 + per);
  int s = 0;
  for (int b = b0; b < b1; ++b) s += row[b];
  part[tid] = s;
  __syncthreads();
  for (int o = 1; o < RANGE_SCAN_T; o <<= 1) {
    const int v = tid >= o ? part[tid - o] : 0;
    __syncthreads();
    part[tid] += v;
    __syncthreads();
  }
  int run = part[tid] - s;
  for (int b = b0; b < b1; ++b) { const int c = row[b]; row[b] = run; run += c; }
  if (tid == RANGE_SCAN_T - 1) {
    row[nb] = part[tid];
    if (counts_out) counts_out[blockIdx.x] = part[tid];
  }
}

// one workgroup of 256 threads: offsets[0] = 0, offsets[i + 1] = the sum of the totals (slot nb) of the rows 0 .. i, in int64
__global__ __launch_bounds__(RANGE_SCAN_T) void rt_range_offsets_kernel(const int* __restrict__ table, int M, int nb, long long* __restrict__ offsets) {
  __shared__ long long part[RANGE_SCAN_T];
  const int tid = threadIdx.x;
  const int per = (M + RANGE_SCAN_T - 1) / RANGE_SCAN_T, i0 = min(M, tid * per), i1 = min(M, i0 + per);
  long long s = 0;
  for (int i = i0; i < i1; ++i) s += table[(long)i * (nb + 1) + nb];
  part[tid] = s;
  __syncthreads();
  for (int o = 1; o < RANGE_SCAN_T; o <<= 1) {
    const long long v = tid >= o ? part[tid - o] : 0;
    __syncthreads();
    part[tid] += v;
    __syncthreads();
  }
  long long run = part[tid] - s;
  if (tid == 0) offsets[0] = 0;
  for (int i = i0; i < i1; ++i) { run += table[(long)i * (nb + 1) + nb]; offsets[i + 1] = run; }
}

// the operand table of rt_few_launch_prep: what a count or fill call needs besides the caller's table
struct RangeWs { float *qnorm, *qn; size_t bytes; };
RangeWs range_layout(void* base, int d) {
  Arena a{(char*)base}; RangeWs w;
  const int dpad = (d + RK - 1) / RK * RK;
  w.qnorm = a.take<float>(FEW_MAX); w.qn = a.take<float>((size_t)dpad * FEW_MAX);
  w.bytes = a.off;
  return w;
}

template <bool FILL>
int range_sweep(const char* fn, const float* queries, const void* gallery, int gallery_dtype, const float* gallery_norms, const unsigned char* keep,
                const float* thresholds, int M, int N, int d, int32_t* table, const int64_t* offsets, int64_t capacity, int32_t* rows_out,
                float* scores_out, void* workspace, size_t workspace_bytes, hipStream_t st) {
  COOT_REQUIRE(gallery_dtype == COOT_GALLERY_F32 || gallery_dtype == COOT_GALLERY_BF16 || gallery_dtype == COOT_GALLERY_F16,
               "%s: gallery_dtype = %d (COOT_GALLERY_F32, COOT_GALLERY_BF16 or COOT_GALLERY_F16)", fn, gallery_dtype);
  COOT_REQUIRE(queries && gallery && thresholds && table && workspace && (!FILL || (offsets && rows_out && scores_out)), "%s: null pointer", fn);
  COOT_REQUIRE(M >= 1 && M <= FEW_MAX && N >= 1 && d >= 1, "%s: M = %d (1 .. %d), N = %d, d = %d", fn, M, FEW_MAX, N, d);
  COOT_REQUIRE(capacity >= 0, "%s: capacity = %lld is negative", fn, (long long)capacity);
  COOT_REQUIRE(((uintptr_t)workspace & 15) == 0, "%s: workspace is not 16-byte aligned", fn);
  const RangeWs w = range_layout(workspace, d);
  COOT_REQUIRE(w.bytes <= workspace_bytes, "%s: workspace too small (%zu < %zu)", fn, workspace_bytes, w.bytes);
  const FewPlan p = few_plan(M, N);
  if (int rc = rt_few_launch_prep(queries, M, d, gallery_norms != nullptr, w.qnorm, w.qn, st)) return rc;
  with_elem(gallery_dtype, [&](auto t) {
    using GT = typename decltype(t)::type;
    const int vec = d % (16 / (int)sizeof(GT)) == 0 && ((uintptr_t)gallery & 15) == 0;  // every row starts 16-byte aligned
    with_mq(p.MQ, [&](auto mq) {
      with_bool(gallery_norms != nullptr, [&](auto norm) {
        hipLaunchKernelGGL((rt_range_kernel<GT, decltype(mq)::value, decltype(norm)::value, FILL>), dim3(p.S), dim3(FR), 0, st, (const GT*)gallery,
                           gallery_norms, (const float*)w.qn, thresholds, M, N, d, p.blocks, vec, keep, (int*)table, (const long long*)offsets,
                           (long long)capacity, (int*)rows_out, scores_out);
      });
    });
  });
  COOT_CHECK_LAUNCH(FILL ? "rt_range (fill)" : "rt_range (count)");
  return 0;
}

}  // namespace
}  // namespace coot

using namespace coot;

extern "C" {

size_t coot_retrieval_range_workspace_bytes(int M, int N, int d) {
  if (M < 1 || M > FEW_MAX || N < 1 || d < 1) return 256;
  return range_layout(nullptr, d).bytes + 256;
}

int coot_retrieval_range_count(const float* queries, const void* gallery, int gallery_dtype, const float* gallery_norms, const uint8_t* keep,
                               const float* thresholds, int M, int N, int d, int32_t* block_counts, void* workspace, size_t workspace_bytes,
                               coot_stream_t stream) {
  return range_sweep<false>("retrieval_range_count", queries, gallery, gallery_dtype, gallery_norms, keep, thresholds, M, N, d, block_counts, nullptr, 0,
                            nullptr, nullptr, workspace, workspace_bytes, (hipStream_t)stream);
}

int coot_retrieval_range_scan(int32_t* block_counts, int M, int N, int64_t* offsets, int32_t* counts_out, coot_stream_t stream) {
  const char* fn = "retrieval_range_scan";
  COOT_REQUIRE(block_counts, "%s: null pointer", fn);
  COOT_REQUIRE(M >= 1 && N >= 1, "%s: M = %d, N = %d", fn, M, N);
  const int nb = (N + FR - 1) / FR;
  hipLaunchKernelGGL(rt_range_scan_kernel, dim3(M), dim3(RANGE_SCAN_T), 0, (hipStream_t)stream, (int*)block_counts, nb, (int*)counts_out);
  COOT_CHECK_LAUNCH("rt_range_scan");
  if (!offsets) return 0;
  hipLaunchKernelGGL(rt_range_offsets_kernel, dim3(1), dim3(RANGE_SCAN_T), 0, (hipStream_t)stream, (const int*)block_counts, M, nb, (long long*)offsets);
  COOT_CHECK_LAUNCH("rt_range_offsets");
  return 0;
}

int coot_retrieval_range_fill(const float* queries, const void* gallery, int gallery_dtype, const float* gallery_norms, const uint8_t* keep,
                              const float* thresholds, int M, int N, int d, const int32_t* block_base, const int64_t* offsets, int64_t capacity,
                              int32_t* rows_out, float* scores_out, void* workspace, size_t workspace_bytes, coot_stream_t stream) {
  return range_sweep<true>("retrieval_range_fill", queries, gallery, gallery_dtype, gallery_norms, keep, thresholds, M, N, d, (int32_t*)block_base, offsets,
                           capacity, rows_out, scores_out, workspace, workspace_bytes, (hipStream_t)stream);
}

}  // extern "C"
