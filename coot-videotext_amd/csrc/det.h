// Deterministic accumulation (coot_det_configure; the reference tests run-to-run determinism: tests_nntrainer/integration_deter.py:18-66).
//
// Everything in this library is computed in a fixed order EXCEPT the few places where several workgroups add into one fp32 word with
// atomicAdd (bias / LayerNorm-parameter gradients of the global networks' single-launch backward, the bias gradients the weight-
// gradient GEMM's loader waves collect per split, the pooling bias gradient, the folded input-LayerNorm gradients, the per-op path's
// column sums, the cycle-consistency loss word): float addition does not associate, so the arrival order of the atomics moves the last
// bits, and Adam (eps = 1e-8: an update is +-lr whatever the gradient's size) turns last bits into different trajectories.
// Deterministic mode gives every REGISTERED fp32 range (the gradient arenas, the loss words) a shadow of 64-bit fixed-point
// accumulators (2^-40 units): acc_add() adds round(v 2^40) there with an INTEGER atomic — integer addition associates, the sum does not
// depend on the order — and coot_det_flush adds the sums into the fp32 words (one float addition per word, in stream order behind every
// adder) and clears the shadow.  Addresses outside the registered ranges, and everything while the mode is off, take the plain float
// atomic.  Resolution 9.1e-13 absolute, range +-8.4e6 per word: below fp32 round-off for any gradient entry above 1e-5 in magnitude.
// An addend that is NaN, Inf or >= 2^22 in magnitude bypasses the shadow (plain float atomic on the fp32 word): a diverged step shows
// up as NaN / Inf in the gradients and the loss exactly as without the mode (the run is no longer bit-reproducible then — it is lost anyway).
// Every such addend is COUNTED (a word in the shadow's padding; coot_get_option("det_bypasses") reads it, synchronising): a caller
// that relies on bit-reproducibility checks that the count stayed 0 (RetrievalTrainer.det_bypass_count).
// The 64-bit word itself wraps past +-2^23 (in value units).  With the overflow guard on (coot_set_option("det_overflow_check", 1):
// what a loss-scaled deterministic run turns on, where a scaled word can get there) every shadow add reads the old word back, and an
// add whose sum wraps sets the fp32 word to NaN (and is counted: coot_get_option("det_overflows")) — the wrapped, finite garbage the
// flush would otherwise fold in becomes a non-finite gradient that the loss scaler's check sees and skips.  Off, the add returns nothing
// (the unscaled path: no word reaches 2^23 there) and costs what it always did.
#pragma once
#include "common.h"

namespace coot {

struct DetRange { const char* base; size_t bytes; long long* shadow; };
struct DetTable {
  int n; DetRange r[8];
  unsigned* bypass;    // counts the addends that left the fixed-point path (below), in the shadow's padding
  int guard;           // overflow guard on (above)
  unsigned* overflow;  // counts the wrapped adds (next to bypass)
};
constexpr double kDetScale = 1099511627776.0;  // 2^40
constexpr float kDetMaxAddend = 4194304.0f;    // 2^22: one addend; the 64-bit word itself holds sums up to +-8.4e6

// one table per translation unit (the library is built without relocatable device code): COOT_DET_DEFINE_SETTER(name) defines
// det_set_table_<name>(), det.hip installs the same table in all of them
static __device__ DetTable g_det_dev = {0, {}, nullptr, 0, nullptr};

__device__ __forceinline__ void acc_add(float* p, float v) {
  const int n = g_det_dev.n;
  for (int i = 0; i < n; ++i) {
    const size_t off = (size_t)(reinterpret_cast<const char*>(p) - g_det_dev.r[i].base);  // (wraps to a huge value below the base)
    if (off < g_det_dev.r[i].bytes) {
      // outside the fixed-point range (|v| >= 2^22: a single addend that large is an exploding gradient; words that accumulate up to
      // +-8.4e6 stay exact) or not finite: llrint would be undefined (LLONG_MIN in practice — a finite garbage word that hides the
      // NaN from the trainer's loss checks).  Such an addend takes the plain float atomic: NaN / Inf reach the fp32 word.
      if (!(fabsf(v) < kDetMaxAddend)) {  // counted: a run that took this exit is no longer bit-reproducible (coot_get_option("det_bypasses"))
        atomicAdd(g_det_dev.bypass, 1u);
        break;
      }
      unsigned long long* w = reinterpret_cast<unsigned long long*>(g_det_dev.r[i].shadow + (off >> 2));
      const unsigned long long a = (unsigned long long)llrint((double)v * kDetScale);
      if (g_det_dev.guard) {
        const unsigned long long old = atomicAdd(w, a), sum = old + a;
        if ((long long)((old ^ sum) & (a ^ sum)) < 0) {  // signed overflow of old + a: the word no longer holds the sum
          atomicAdd(g_det_dev.overflow, 1u);
          atomicAdd(p, __builtin_nanf(""));
        }
      } else {
        atomicAdd(w, a);
      }
      return;
    }
  }
  atomicAdd(p, v);
}

#define COOT_DET_DEFINE_SETTER(name)                                                                              \
  int det_set_table_##name(const DetTable& t) {                                                                   \
    return check_hip(hipMemcpyToSymbol(HIP_SYMBOL(g_det_dev), &t, sizeof(DetTable)), "det table (" #name ")");   \
  }

int det_set_table_fused(const DetTable& t);
int det_set_table_gemm(const DetTable& t);
int det_set_table_loss(const DetTable& t);
int det_set_table_pool(const DetTable& t);
int det_set_table_rowops(const DetTable& t);
// adds the shadow sums of the registered words inside [base, base + bytes) into them and clears the shadow (no-op while the mode is off)
int det_flush_range(const void* base, size_t bytes, hipStream_t st);

// The flush of ONE word: the fixed-point sum v joins the fp32 word in a single rounded addition (explicit: no contraction can change it).
// det_flush_kernel and every launch that flushes words on its way (coot_train_step's update: api_step.hip) compute exactly this.
__device__ __forceinline__ float det_fold(float w, long long v) { return __fadd_rn(w, (float)((double)v * (1.0 / kDetScale))); }

// Segment flushes.  Only some words of a registered range can hold a sum — in a gradient arena whose weight matrices the backward
// WROTE (coot_net_grads_overwrite), the biases / LayerNorm vectors between them — so a step flushes those segments, not the whole range.
// det_locate: the shadow word of `base` when [base, base + bytes) lies inside ONE registered range (returns 1), 0 when it touches none
// (nothing to flush), -1 when it straddles a range's end (only det_flush_range handles that)
int det_locate(const void* base, size_t bytes, long long** shadow);
constexpr int kDetMaxSegs = 64;
struct DetSeg { float* p; long long* shadow; int n; int blk0; };
struct DetSegs { int n = 0; DetSeg s[kDetMaxSegs]; };
// adds [p, p + n) to the list (located as above; a straddling segment is flushed by det_flush_range right away on `st`)
int det_segs_add(DetSegs& s, float* p, long n, hipStream_t st);
// all segments of the list in ONE launch (no launch for an empty list)
int det_flush_segs(DetSegs& s, hipStream_t st);
// The one route that acc_add()s into a weight MATRIX in overwrite mode: launch_gemm_tn's one-pass path (fp32 atomics into C, which it
// zero-filled first).  It notes itself here (host, this thread); the step takes the note after each backward pass and flushes that arena
// whole.
void det_note_matrix_atomics();
bool det_take_matrix_atomics();
bool det_on();
int det_bypass_count();
int det_overflow_count();                    // wrapped adds since coot_det_configure (synchronises; -1: mode off)
int det_set_overflow_guard(int on);          // uploads the table (synchronises the device): a setup call
int det_overflow_guard();

}  // namespace coot
