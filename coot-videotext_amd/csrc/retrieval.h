// What the retrieval sources share (retrieval_tile.hip, retrieval_few.hip, retrieval_grouped.hip, retrieval_multi.hip, retrieval_scoped.hip, retrieval_adjusted.hip, retrieval_index.hip): the chunk constants and the widening of a
// gallery element, the 64-bit top-K entry and the fold of candidates into a sorted list, and the host helpers that carve a workspace
// and turn a run-time value into a template argument.  Every kernel is instantiated in one file only.
#pragma once
#include <type_traits>
#include "../../include/coot_hip.h"
#include "common.h"

namespace coot {

// rt_norms_kernel<float> (retrieval_index.hip) on rows [0, Ma) of a, then [0, Nb) of b; the caller checks the launch
void rt_launch_norms(const float* a, int Ma, const float* b, int Nb, int d, float* na, float* nb, hipStream_t st);

// The head and the tail of the labelled ranking (retrieval_tile.hip) for the ranking under offsets (retrieval_ranks_adjusted.hip):
// rt_lab_prepare_kernel (ranks = 0 or -1 and n_valid, from labels and best [N]) and rt_metrics_kernel<true> (hist [N + M], zeroed);
// the caller checks the launch
void rt_launch_lab_prepare(const int32_t* labels, const unsigned long long* best, int M, int N, int32_t* ranks_q, int32_t* ranks_g, int32_t* n_valid,
                           hipStream_t st);
void rt_launch_lab_metrics(const int32_t* ranks_q, const int32_t* ranks_g, int M, int N, int* hist, float* metrics, hipStream_t st);

// The few-query sweep's plan and the launches of its kernels that the grouped search shares (retrieval_few.hip):
// few_plan: row splits and the 128-row blocks each one sweeps (every split has at least one block; cap bounds S whatever the option says);
// rt_few_launch_prep: rt_few_prep_kernel, the query norms [16] and the operand table qn [d rounded up to 32][16];
// rt_few_merge_lists: the merge by rank of S >= 2 sorted lists per query, lists [M][S][K], into idx_out / score_out, in rounds of <= 32
//   lists; spare takes every other round's lists (M x ceil(S / 32) x K entries, unused for S <= 32).  Both return a launch's error.
struct FewPlan { int MQ, S, blocks, cap; };
FewPlan few_plan(int M, int N);
int rt_few_launch_prep(const float* queries, int M, int d, bool norm, float* qnorm, float* qn, hipStream_t st);
int rt_few_merge_lists(const unsigned long long* lists, unsigned long long* spare, int S, int M, int K, bool masked, int32_t* idx_out, float* score_out,
                       hipStream_t st);

// What the multi-vector search shares with the grouped one (retrieval_grouped.hip):
// grp_plan: the ranges of a table of NG groups that a selection walks (coot_set_option("rt_grouped_splits", n); cap bounds T whatever
//   the option says, and a workspace is sized by it);
// rt_grouped_launch_slice: rt_few_prep_kernel, then rt_grouped_kernel, for one slice of M <= 16 queries: the sweep raises best [M][NG],
//   which the caller has reset, and writes sim [M][N] where it is given.  gallery_dtype: a COOT_GALLERY_* code the caller has checked;
//   qnorm [16] and qn [d rounded up to 32][16]: the workspace of rt_few_launch_prep.  Returns a launch's error.
struct GrpPlan { int T, span, cap; };
GrpPlan grp_plan(int NG);
int rt_grouped_launch_slice(const float* queries, const void* gallery, int gallery_dtype, const float* gallery_norms, const unsigned char* keep,
                            const int32_t* groups, int NG, int M, int N, int d, float* sim, float* qnorm, float* qn, unsigned long long* best,
                            hipStream_t st);

namespace {

constexpr int RT = 64;   // tile: 64 rows of emb1 x 64 rows of emb2
constexpr int RK = 32;   // k chunk
constexpr int RP = RK + 1;
constexpr int FEW_MAX = COOT_RETRIEVAL_FEW_MAX;  // queries of a few-query sweep
constexpr int FR = 128;                          // gallery rows per step of the sweep = threads per workgroup
constexpr int FEW_G = 32;                        // lists per merge workgroup
constexpr int GRP_GMAX = 1 << 26;                // groups of a grouped search: M x G entries of 8 bytes are the table
constexpr int GRP_U = 4;                         // table loads in flight per lane of a table selection

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

// one chunk of the chain for the thread's gallery row: acc[i] = fmaf(q_ik, g_jk, acc[i]) over the chunk's 32 k in order.  The 16-bit
// sweep and the grouped sweep call it; the fp32 sweep of rt_few_kernel keeps the same loop in its body, so that its instantiations
// compile to the instructions they had
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

// ---- the top-K entry ------------------------------------------------------------------------------------------------------------
// An entry is one 64-bit word, (order-preserving image of the score) << 32 | column: "ahead" is one unsigned compare, a strict
// total order over every bit pattern (NaNs included), so selection and merge cannot depend on who came first.
constexpr int TK_MAX = 128;  // K
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

// The result of an unfilled slot in the masked searches (fewer than K kept rows): index -1, score -inf.  Word 0 is a real entry
// only for the all-ones NaN at column 0 (tk_pack), which a masked search therefore reports as unfilled.
__device__ __forceinline__ int tk_idx_masked(tk_entry_t e) { return e ? (int)(unsigned)e : -1; }
__device__ __forceinline__ float tk_score_masked(tk_entry_t e) { return e ? tk_score(e) : __uint_as_float(0xFF800000u); }

// ---- host helpers ---------------------------------------------------------------------------------------------------------------
// A workspace carved into consecutive pieces, each rounded up to 256 bytes.  A null base sizes a layout: every piece is nullptr
// and off is the bytes a real base has to hold.
struct Arena {
  char* base;
  size_t off = 0;
  template <typename T>
  T* take(size_t count) { T* p = base ? (T*)(base + off) : nullptr; off += (count * sizeof(T) + 255) & ~(size_t)255; return p; }
};

// A run-time value as a template argument: f is a generic lambda that receives it as a std::bool_constant, a std::integral_constant
// or (an element type) an ElemType, and what f returns is returned.
template <typename F>
auto with_bool(bool b, F&& f) { return b ? f(std::true_type{}) : f(std::false_type{}); }
template <typename F>
auto with_bool(bool a, bool b, F&& f) {
  return with_bool(a, [&](auto ta) { return with_bool(b, [&](auto tb) { return f(ta, tb); }); });
}
// mq: the 1, 2, 4, 8 or 16 accumulators of rt_few_kernel
template <typename F>
auto with_mq(int mq, F&& f) {
  switch (mq) {
    case 1: return f(std::integral_constant<int, 1>{});
    case 2: return f(std::integral_constant<int, 2>{});
    case 4: return f(std::integral_constant<int, 4>{});
    case 8: return f(std::integral_constant<int, 8>{});
    default: return f(std::integral_constant<int, 16>{});
  }
}
// code: COOT_GALLERY_F32, _BF16 (unsigned short) or _F16, which the caller has checked
template <typename T> struct ElemType { using type = T; };
template <typename F>
auto with_elem(int code, F&& f) {
  return code == COOT_GALLERY_F32 ? f(ElemType<float>{}) : code == COOT_GALLERY_BF16 ? f(ElemType<unsigned short>{}) : f(ElemType<_Float16>{});
}

}  // namespace
}  // namespace coot
