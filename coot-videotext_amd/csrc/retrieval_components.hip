// ---- connected components of a prepared gallery's self-join: a cluster label per row in one sweep (coot_retrieval_components) ------
// The edge set is the hit set of retrieval_join.hip: pair (i, j), i < j, is an edge when keep lets both rows pass, groups (if given)
// differ and s(i, j) >= thr[i], s(i, j) being the chain of rt_join_tile_kernel, so of every search: acc = 0, one fmaf per k in k order,
// chunks of 32, zero padding beyond d and N, operands x / norm(row) with NORM, both operands the stored rows widened as they are staged.
// Where the count pass of the join writes a popcount, each hit becomes a union in parent [N]; labels[i] is then the smallest row of
// row i's component, -1 for a row that keep masks.  No table, no scan, no fill pass, no pair list, no chunks.  Three launches:
//   rt_comp_init_kernel: parent[i] = i.
//   rt_comp_link_kernel<TB, NORM>: grid (ceil(nb / blocks_per_wg), row tiles), 256 threads: a workgroup serves rows i0 .. i0 + 63 and the
//     128-row blocks b0 .. b1 - 1 of the whole gallery.  Staging, prefetch, thread layout (rows 4 ty .. 4 ty + 3, columns tx + 16 c) and
//     hit words in LDS by integer OR as in rt_join_tile_kernel<TB, NORM, false>; a block left of the diagonal and a block in which keep
//     leaves no row are left before their first load; thresholds, keep flags and ids are read after the chain.  Then thread r < 64
//     walks the set bits of its row's two hit words and unites i0 + r with each column, keeping its row's current root across the bits.
//   rt_comp_label_kernel: labels[i] = keep allows i ? the root of i : -1, from parent alone, after the kernel boundary.
// The union-find.  parent[x] <= x always, and every store lowers a value: a root is linked below a SMALLER root by compare-and-swap, and
// path halving is atomicMin(&parent[x], grandparent).  find follows p = parent[x] while p != x: strictly descending, so it ends whatever
// other workgroups do.  unite(a, b) takes both roots and, while they differ, tries CAS(&parent[larger], larger, smaller); a failed CAS
// returns a value below the larger root, from which both finds go on: the pair strictly decreases at every failed attempt, so the loop is
// bounded by the values, not by the schedule — no spin on another workgroup's progress, no flag, no ticket.  By induction the root of a
// set is its smallest member, so the labels are a function of the edge set alone.
// Memory.  gfx950 has eight private L2s.  Inside the link kernel every read of parent is a relaxed agent-scope atomic load and every
// write an agent-scope atomicCAS or atomicMin.  A read may still be stale: a stale parent is an earlier value, so a member of the same
// set with a number <= the row's own, and the CAS catches a stale "root" — correctness does not depend on freshness.  No floating-point
// atomic, no assembly.  keep and groups may be null (run-time checks); both are read for rows < N only.
#include "retrieval.h"

namespace coot {

int g_rt_comp_blocks_per_wg = 0;  // coot_set_option("rt_comp_blocks_per_wg", n) (tests); 0 = automatic

namespace {

constexpr int JB = COOT_RETRIEVAL_RANGE_BLOCK;  // gallery rows of a block = columns of the tile
static_assert(JB == 2 * RT && RT == 64, "a row's hit bits of a block are two 64-bit words");
constexpr int COMP_WGS = 1 << 20;  // above this many workgroups a workgroup walks several blocks (the join's rule)

__device__ __forceinline__ int uf_load(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// the root of x as far as this thread can see: a member of x's set, <= x, that read as its own parent
__device__ __forceinline__ int uf_find(int* parent, int x) {
  int p = uf_load(parent + x);
  while (p != x) {  // (p < x)
    const int gp = uf_load(parent + p);
    if (gp != p) atomicMin(parent + x, gp);  // path halving: x is no root (a value never rises), gp is an ancestor below p
    x = p;
    p = gp;
  }
  return x;
}

// Unites the sets of ra, the root of a row's set as its thread last knew it, and row b; returns the root of the union as known now.
__device__ __forceinline__ int uf_unite(int* parent, int ra, int b) {
  int rb = uf_find(parent, b);
  ra = uf_find(parent, ra);  // (one load while ra is still the root)
  while (ra != rb) {
    if (ra < rb) { const int t = ra; ra = rb; rb = t; }
    const int old = atomicCAS(parent + ra, ra, rb);
    if (old == ra) return rb;  // linked: ra was a root, and rb < ra
    ra = uf_find(parent, old);  // old < ra: the pair decreases
    rb = uf_find(parent, rb);
  }
  return ra;
}

__global__ __launch_bounds__(256) void rt_comp_init_kernel(int* __restrict__ parent, int N) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < N) parent[i] = i;
}

__global__ __launch_bounds__(256) void rt_comp_label_kernel(const int* __restrict__ parent, const unsigned char* __restrict__ keep, int N,
                                                            int* __restrict__ labels) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= N) return;
  int x = i;
  if (keep && !keep[i]) {
    x = -1;
  } else {
    for (int p = parent[x]; p != x; p = parent[x]) x = p;  // (p < x)
  }
  labels[i] = x;
}

// static LDS: As [64][33] | Bs [128][33] | hw [2][64] | gA [64] | gB [128], 27 392 bytes, and with NORM nAs [64] | nBs [128]: 28 160.
// Registers (tools/kernel_resources.py; the three element types and both builds alike): 221 VGPRs, with norms 228, 106 SGPRs, no scratch:
// two waves per SIMD = two workgroups per CU, as the count form of rt_join_tile_kernel (222 / 228).  The union-find runs after the
// chain, when the accumulators are dead.  rt_comp_init_kernel: 4 VGPRs, rt_comp_label_kernel: 6, neither with LDS or scratch.
template <typename TB, bool NORM>
__global__ __launch_bounds__(256) void rt_comp_link_kernel(const TB* __restrict__ G, const float* __restrict__ gnorm, const float* __restrict__ thr,
                                                           const unsigned char* __restrict__ keep, const int* __restrict__ groups, int N, int d,
                                                           int blocks_per_wg, int* parent) {
  __shared__ float As[RT][RP], Bs[JB][RP];
  __shared__ float nAs[RT], nBs[JB];        // NORM: the norms of the staged rows (1 beyond N: those rows are staged as zeros)
  __shared__ int gA[RT], gB[JB];            // groups: the ids of the staged rows
  __shared__ unsigned long long hw[2][RT];  // hw[h][r]: the hit bits of row r of the row tile in columns 64 h .. 64 h + 63 of the block
  const int tid = threadIdx.x, ty = tid >> 4, tx = tid & 15;
  const int sr = tid >> 5, sk = tid & 31;  // staging: column sk of the chunk, rows sr + 8 q
  const int i0 = blockIdx.y * RT;
  const int nb = (N + JB - 1) / JB;
  const int b0 = blockIdx.x * blocks_per_wg, b1 = min(nb, b0 + blocks_per_wg);
  int root = i0 + tid;  // tid < 64: the root of row i0 + tid's set as this thread last knew it (the row itself before its first union)
  for (int b = b0; b < b1; ++b) {
    const int j0 = b * JB;
    if (j0 + JB <= i0 + 1) continue;  // (uniform) left of the diagonal: no j > i for any row of the tile
    if (keep) {
      if (!__syncthreads_or(tid < JB && j0 + tid < N && keep[j0 + tid])) continue;  // (uniform) keep leaves no row of the block
    }
    if (tid < JB) {
      (&hw[0][0])[tid] = 0ull;
      if (NORM) nBs[tid] = j0 + tid < N ? gnorm[j0 + tid] : 1.f;
      if (groups) gB[tid] = j0 + tid < N ? groups[j0 + tid] : 0;
    } else if (tid < JB + RT) {
      if (NORM) nAs[tid - JB] = i0 + tid - JB < N ? gnorm[i0 + tid - JB] : 1.f;
      if (groups) gA[tid - JB] = i0 + tid - JB < N ? groups[i0 + tid - JB] : 0;
    }
    TB pa[8], pb[16];
    // one chunk into registers.  No branch: an address beyond N or d is clamped into the gallery and its value is dropped at staging
    auto load = [&](int k0) {
      const int k = min(k0 + sk, d - 1);
#pragma unroll
      for (int q = 0; q < 8; ++q) pa[q] = G[(long)min(i0 + sr + 8 * q, N - 1) * d + k];
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
      // stage 64 x 32 of the row tile and 128 x 32 of the block; rows beyond N and columns beyond d are zero
      const bool kin = k0 + sk < d;
#pragma unroll
      for (int q = 0; q < 8; ++q) {
        const int r = sr + 8 * q;
        As[r][sk] = (kin && i0 + r < N) ? (NORM ? widen(pa[q]) / nAs[r] : widen(pa[q])) : 0.f;
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
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int i = i0 + 4 * ty + r;
      const bool rin = i < N && (!keep || keep[i]);  // row i exists and passes keep
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
    }
    __syncthreads();
    if (tid < RT) {  // (a set bit implies i0 + tid < N and its column < N)
#pragma unroll
      for (int h = 0; h < 2; ++h)
        for (unsigned long long w = hw[h][tid]; w; w &= w - 1ull) root = uf_unite(parent, root, j0 + 64 * h + __ffsll((long long)w) - 1);
    }
    __syncthreads();  // the words are read: the next block may clear them
  }
}

}  // namespace

void set_rt_comp_blocks_per_wg(int n) { g_rt_comp_blocks_per_wg = n; }
int get_rt_comp_blocks_per_wg() { return g_rt_comp_blocks_per_wg; }

}  // namespace coot

using namespace coot;

extern "C" {

int coot_retrieval_components(const void* gallery, int gallery_dtype, const float* gallery_norms, const uint8_t* keep, const int32_t* groups,
                              const float* thresholds, int N, int d, int32_t* parent, int32_t* labels, coot_stream_t stream) {
  const char* fn = "retrieval_components";
  hipStream_t st = (hipStream_t)stream;
  COOT_REQUIRE(gallery_dtype == COOT_GALLERY_F32 || gallery_dtype == COOT_GALLERY_BF16 || gallery_dtype == COOT_GALLERY_F16,
               "%s: gallery_dtype = %d (COOT_GALLERY_F32, COOT_GALLERY_BF16 or COOT_GALLERY_F16)", fn, gallery_dtype);
  COOT_REQUIRE(gallery && thresholds && parent && labels, "%s: null pointer", fn);
  COOT_REQUIRE(N >= 1 && d >= 1, "%s: N = %d, d = %d", fn, N, d);
  COOT_REQUIRE(((long long)N + RT - 1) / RT <= 65535, "%s: N = %d (one launch covers all rows: 1 .. %d)", fn, N, 65535 * RT);
  const int mt = (N + RT - 1) / RT, nb = (N + JB - 1) / JB;
  int per = (int)(((long long)nb * mt + COMP_WGS - 1) / COMP_WGS);  // 1 up to 2^20 workgroups
  if (g_rt_comp_blocks_per_wg > 0) per = min(g_rt_comp_blocks_per_wg, nb);
  hipLaunchKernelGGL(rt_comp_init_kernel, dim3((N + 255) / 256), dim3(256), 0, st, (int*)parent, N);
  COOT_CHECK_LAUNCH("rt_comp_init");
  const dim3 grid((nb + per - 1) / per, mt);
  with_elem(gallery_dtype, [&](auto t) {
    using TB = typename decltype(t)::type;
    with_bool(gallery_norms != nullptr, [&](auto norm) {
      hipLaunchKernelGGL((rt_comp_link_kernel<TB, decltype(norm)::value>), grid, dim3(256), 0, st, (const TB*)gallery, gallery_norms, thresholds, keep,
                         (const int*)groups, N, d, per, (int*)parent);
    });
  });
  COOT_CHECK_LAUNCH("rt_comp_link");
  hipLaunchKernelGGL(rt_comp_label_kernel, dim3((N + 255) / 256), dim3(256), 0, st, (const int*)parent, keep, N, (int*)labels);
  COOT_CHECK_LAUNCH("rt_comp_label");
  return 0;
}

}  // extern "C"
