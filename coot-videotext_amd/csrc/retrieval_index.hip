// The rows of a prepared gallery (GalleryIndex): their norms, computed once, and rows written into the gallery in its storage type
// together with their norms (coot_retrieval_row_norms, coot_retrieval_row_norms_h, coot_retrieval_rows_put).
#include "retrieval.h"

namespace coot {
namespace {

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

}  // namespace

void rt_launch_norms(const float* a, int Ma, const float* b, int Nb, int d, float* na, float* nb, hipStream_t st) {
  hipLaunchKernelGGL(rt_norms_kernel<float>, dim3((Ma + Nb + 3) / 4), dim3(256), 0, st, a, Ma, b, Nb, d, na, nb);
}
}  // namespace coot

using namespace coot;

extern "C" {

int coot_retrieval_row_norms(const float* rows, int N, int d, float* norms, coot_stream_t stream) {
  COOT_REQUIRE(rows && norms, "retrieval_row_norms: null pointer");
  COOT_REQUIRE(N >= 1 && d >= 1, "retrieval_row_norms: N = %d, d = %d", N, d);
  rt_launch_norms(rows, N, nullptr, 0, d, norms, nullptr, (hipStream_t)stream);
  COOT_CHECK_LAUNCH("rt_norms");
  return 0;
}

int coot_retrieval_row_norms_h(const void* rows, int dtype, int N, int d, float* norms, coot_stream_t stream) {
  COOT_REQUIRE(dtype == COOT_GALLERY_BF16 || dtype == COOT_GALLERY_F16, "retrieval_row_norms_h: dtype = %d (COOT_GALLERY_BF16 or COOT_GALLERY_F16)", dtype);
  COOT_REQUIRE(rows && norms, "retrieval_row_norms_h: null pointer");
  COOT_REQUIRE(N >= 1 && d >= 1, "retrieval_row_norms_h: N = %d, d = %d", N, d);
  with_elem(dtype, [&](auto t) {
    using T = typename decltype(t)::type;
    hipLaunchKernelGGL(rt_norms_kernel<T>, dim3((N + 3) / 4), dim3(256), 0, (hipStream_t)stream, (const T*)rows, N, (const T*)nullptr, 0, d, norms,
                       (float*)nullptr);
  });
  COOT_CHECK_LAUNCH("rt_norms_h");
  return 0;
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
  with_elem(src_dtype, [&](auto s) {
    with_elem(gallery_dtype, [&](auto g) {
      using S = typename decltype(s)::type;
      using G = typename decltype(g)::type;
      if constexpr (std::is_same_v<S, float> || std::is_same_v<G, float> || std::is_same_v<S, G>)  // the pairs that pass the check above
        hipLaunchKernelGGL((rt_put_kernel<S, G>), dim3((R + 3) / 4), dim3(256), 0, st, (const S*)src, R, d, (const int*)dest, row0, (G*)gallery, N, norms);
    });
  });
  COOT_CHECK_LAUNCH("rt_put");
  return 0;
}

}  // extern "C"
