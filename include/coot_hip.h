/*
 * coot_hip.h — C ABI of libcoot_hip.so: the MI355X (gfx950) implementation of the COOT retrieval
 * training hot path.  Plain pointers and sizes only; every pointer is DEVICE memory unless stated
 * otherwise; every call enqueues asynchronously on the given hipStream_t (pass
 * torch.cuda.current_stream().cuda_stream) and never allocates, frees or synchronises.  Return value: 0 = ok,
 * negative = error (message via coot_last_error()).
 *
 * Retained pointers (ownership contract).  A compute call keeps NO pointer of its arguments after it returns (the
 * launches it enqueued read them, in stream order: the caller keeps the memory alive until those launches ran, as with any
 * asynchronous call).  The ONLY entry points that store a caller pointer beyond their own return are these setters; the memory
 * stays the caller's and must outlive the registration:
 *   coot_step_set_device_state(state)         thread-local; read by every later coot_train_step of the thread (and by every
 *                                             replay of a step captured while it was set) until reset with NULL
 *   coot_step_set_loss_scaler(block)          thread-local; read and written by every later coot_train_step / coot_step_backward /
 *                                             coot_step_update / coot_step_unscale_grads and loss-gradient call of the thread (and
 *                                             by every replay of a step captured while it was set) until reset with NULL
 *   coot_step_set_grad_clip(block, before)    thread-local; read and written by every later coot_train_step / coot_step_update /
 *                                             coot_step_unscale_grads / coot_step_grad_norm of the thread (and by every replay of a
 *                                             step captured while it was set) until reset with (NULL, 0)
 *   coot_step_set_input_stages(s0, s1, n)     thread-local; written / read by steps that carry COOT_STEP_INPUT_STAGES or
 *                                             COOT_FWD_INPUT_STAGES until reset with (NULL, NULL, 0); a reset also forgets which
 *                                             stage holds which batch
 *   coot_step_set_next_batch(next, dims)      thread-local, ONE-SHOT: the two structs are COPIED at the call, the feature
 *                                             pointers inside them are read by the next coot_train_step / coot_step_forward of the
 *                                             thread (which consumes the announcement) and by nothing after it; (NULL, NULL) drops
 *                                             a pending announcement
 *   coot_step_set_global_done_events(ev, ev)  thread-local hipEvent_t handles, recorded by every later coot_step_backward of the
 *                                             thread until reset with (NULL, NULL)
 *   coot_step_set_cycle_indices(idx)          thread-local; read at every later coot_train_step / cycle-consistency phase of the
 *                                             thread until reset with NULL
 *   coot_det_configure(n, bases, bytes, shadow, ...)  PROCESS-GLOBAL; the base / size arrays are copied, the ranges and the shadow
 *                                             are consulted by every accumulating kernel of every thread until coot_det_configure(0,
 *                                             ...), which synchronises the device before it returns
 * A caller that frees such memory resets the registration first (RetrievalTrainer.close() does; tests/conftest.py does between
 * modules).  A captured step (hipStreamBeginCapture around coot_train_step) additionally bakes every argument pointer and the
 * registrations above into its nodes: all of them must stay valid for as long as the graph may be replayed.
 *
 * The reference (simon-ging/coot-videotext) is pure Python/PyTorch and has no FFI for this path;
 * each entry point names the reference code it replaces (file:line relative to the reference
 * root) — INTEGRATION.md shows the ctypes binding a maintainer adds.
 */
#ifndef COOT_HIP_H
#define COOT_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif
/* The library is built with -fvisibility=hidden: exactly the functions declared between this push and the pop at the end of
 * the header leave libcoot_hip.so (tests/test_cpu_host.py checks the dynamic symbol table against this file). */
#if defined(__GNUC__) || defined(__clang__)
#pragma GCC visibility push(default)
#endif

typedef void* coot_stream_t; /* hipStream_t */

/* One COOT network = nntrainer/models/transformer_legacy.py:26-97 (TransformerConfig) restricted to
 * the options the shipped YAMLs use. */
typedef struct coot_net_config {
  int input_dim;      /* feature dim fed to norm_input                                    */
  int hidden_dim;     /* selfatn_config.hidden_dim (d_model)                              */
  int num_heads;      /* selfatn_config.num_heads                                         */
  int ff_dim;         /* selfatn_config.pointwise_ff_dim (0 => hidden_dim)                */
  int num_layers;     /* selfatn_config.num_layers                                        */
  int use_input_fc;   /* input_fc: Linear(input_dim, hidden_dim) + GELU                   */
  int use_context;    /* cross-attention context block (global nets)                      */
  int ctx_num_layers; /* crossatn_config.num_layers                                       */
  int pooler;         /* 0 = "atn" (GenPool), 1 = "avg_special" (TemporalAvgPool)         */
  int pool_hidden;    /* pooler_config.hidden_dim (0 => hidden_dim)                       */
  int pool_heads;     /* pooler_config.num_heads                                          */
  float dropout;      /* selfatn_config.dropout   (used only when train != 0)             */
  float ctx_dropout;  /* crossatn_config.dropout                                          */
  float pool_dropout; /* pooler_config.dropout                                            */
  int dtype;          /* COOT_DTYPE_BF16 (0, default): bf16 MFMA operands, fp32 accumulation / statistics — the fast path.
                         COOT_DTYPE_F32: the fp32 REFERENCE MODE of coot_net_fwd / coot_net_bwd — the reference's op sequence
                         (nntrainer/models/transformer_legacy.py:200-288, eval mode) with every activation, weight and
                         accumulation in fp32, exact erf GELU, nothing fused or folded: agrees with the reference to ~1e-6 of the
                         output scale, so a difference between the two modes is bf16 rounding and a difference to the reference in
                         F32 mode is a logic error.  coot_net_bwd in this mode is the derivative of exactly that sequence in fp32
                         (parameter gradients to ~1e-5 of the reference's).  A checker: eval only (train must be 0), never what
                         bench.py times.  `saved` keeps every intermediate of the forward (coot_net_saved_bytes accounts for it),
                         `scratch` the backward's temporaries (coot_net_scratch_bytes); wpack is not read.                       */
} coot_net_config;
#define COOT_DTYPE_BF16 0
#define COOT_DTYPE_F32 1
#define COOT_DTYPE_F16 2 /* IEEE half operands: the SECOND BUILD of these sources, libcoot_hip_f16.so (csrc/build.sh, -DCOOT_OPERAND_F16) — the
                            arithmetic of the reference's GPU path (fp16 autocast, coot/trainer_retrieval.py:264; BASELINE.json configs[3]).  The
                            16-bit operand format is a property of the build: libcoot_hip.so accepts COOT_DTYPE_BF16 (and _F32),
                            libcoot_hip_f16.so COOT_DTYPE_F16 (and _F32); coot_get_option("operand_f16") tells which one is loaded.  The f16
                            build is FORWARD-ONLY (coot_net_fwd, coot_step_forward, the loss forward): the reference trains its fp16 path under a
                            GradScaler (coot/trainer_retrieval.py:277-285), which is not built; its backward entry points refuse.            */

const char* coot_last_error(void);
/* ABI version of this header: struct layouts (coot_net_config gained `dtype`, coot_step_buffers `decay_block_all` in round 4) and the
 * meaning of flag words (coot_step_update's `repack` is a bit mask since round 4).  coot_version() returns the value the library was
 * built with; a binding compares the two when it loads the library (coot-videotext_amd/lib.py does) and refuses a mismatch. */
#define COOT_ABI_VERSION 7
int coot_version(void);
/* Option switches for A/B measurements and tests ("fused", "packed", "tn_dma", "grad_poison", ...: the names coot_set_option
 * accepts are listed in csrc/api.hip).  They are PROCESS-GLOBAL ints read at launch time without synchronisation: set them
 * while no other host thread is inside the library (one host thread per process and device is the supported model, SURVEY
 * 8b); the error string, coot_net_grads_overwrite, the step's device-state pointer and the injected cycle indices are
 * thread-local. */
int coot_set_option(const char* name, int value);
/* current value of "tn_dma" / "xcd_order" / "tn_mode" (tests restore what they switch) */
int coot_get_option(const char* name, int* value);
/* profiling aid: device buffer (>= 64 x uint64) receiving s_memtime stamps of block 0 of the fused chain kernels (NULL = off) */
int coot_debug_timestamps(void* dev_u64);
/* coot_set_option("step_stamps", 1): coot_train_step records HIP events at its phase boundaries; this call synchronises
 * the device and writes one line per boundary (microseconds since the start of the last step) into buf.  Profiling aid. */
int coot_debug_step_stamps(char* buf, int buf_bytes);
/* host-only (tests): the keep-scales (0 or 1 / keep-probability) the kernels draw for the n consecutive elements idx0, idx0 + 1, ...
 * of an element-wise dropout site (idx = token row * row width + column), resp. for the Lk attention probabilities of mask row
 * row32 = (sequence * heads + head) * Lq + query — evaluated on the host by the SAME functions (csrc/common.h) and the same
 * quantisation of p the device code uses.  out_host: HOST memory.  Pins oracle/dropout_masks.py (the masks injected into the
 * reference for train-mode parity; nn.Dropout sites of nntrainer/models/transformer_legacy.py:418,435,487,553,592-598 and
 * nntrainer/models/poolers.py:139-143) to this library. */
int coot_debug_dropout_scales(uint64_t seed, unsigned site, uint64_t idx0, int64_t n, float p, float* out_host);
int coot_debug_attn_dropout_scales(uint64_t seed, unsigned site, unsigned row32, int Lk, float p, float* out_host);

/* ---- parameter layout (flat fp32 arena per network; gradients use the same layout) -----------
 * Names and shapes are the reference state-dict names, e.g.
 * "tf.encoder_layers.0.self_attention_layer.sublayer.query_projection.weight". */
int64_t coot_net_param_numel(const coot_net_config* cfg);
int coot_net_param_count(const coot_net_config* cfg);
int coot_net_param_info(const coot_net_config* cfg, int index, char* name, int name_len, int64_t* offset,
                        int64_t shape[4], int* ndim);
int coot_net_out_dim(const coot_net_config* cfg);

/* ---- bf16 weight pack (once per optimizer step) ---------------------------------------------- */
size_t coot_net_wpack_bytes(const coot_net_config* cfg);
int coot_net_pack_weights(const coot_net_config* cfg, const float* params, void* wpack, coot_stream_t stream);
/* The same for n networks in ONE launch (the train step rebuilds the packs of a side's local + global network right after
 * their update: one launch instead of two dependent ones at the end of the step). */
int coot_nets_pack_weights(int n, const coot_net_config* const* cfgs, const float* const* params, void* const* wpacks,
                           coot_stream_t stream);

/* ---- one network forward / backward -----------------------------------------------------------
 * Replaces TransformerLegacy.forward (nntrainer/models/transformer_legacy.py:200-288) and its
 * autograd backward.  feats [N, L, input_dim] fp32 zero padded, lengths [N] int64 (valid rows),
 * hidden [N, hidden_dim] fp32 or NULL, pe = embedding.pe [>=L, hidden_dim] fp32.
 * pooled [N, out_dim] fp32; per_token [N, L, hidden_dim] fp32 or NULL.
 * `saved` carries activations from fwd to bwd (coot_net_saved_bytes), `scratch` is temporary
 * (coot_net_scratch_bytes).  train != 0 enables dropout with the given seed. */
/* Packed (variable-length) token rows, SURVEY 8f-2.  The reference pads every sequence of a batch to the batch maximum
 * (coot/dataset_retrieval.py:335-463) and runs all padded frames / words through the local networks.  With `packed` set, a local
 * network (input_fc + atn pooler) processes only the valid tokens: cu_seqlens[i] (DEVICE, int32, N + N2 + 1 entries, segment 1's
 * sequences first, cu_seqlens[0] = 0) is the first packed row of sequence i, total_tokens = cu_seqlens[N + N2] (HOST copy: it sizes
 * the launches).  The input stays the reference's padded feats (+ lengths): the input LayerNorm gathers the valid rows, the
 * token-tile chains are row independent, attention / pooling / positional encoding take the sequence boundaries from cu_seqlens.
 * Pooled outputs and all gradients equal the padded computation (padded rows carry exactly zero pooling weight, poolers.py:190).
 * NULL (or a network / size the packed path does not cover): the padded layout.  Forward and backward take the same decision.
 * source: where the token rows come from.  COOT_SOURCE_PADDED (0): feats / feats2 are the reference's zero-padded fp32 tensors
 * (coot/dataset_retrieval.py:335-463), the input LayerNorm gathers the valid rows.  COOT_SOURCE_PACKED_F32 / _BF16: `feats` IS the
 * packed matrix [total_tokens, input_dim] (rows in cu_seqlens order, fp32 resp. bf16 bits; feats2 is ignored) as
 * coot_collate_packed writes it — no padding ever crosses PCIe or is read from HBM.  A packed source needs the packed path (it
 * cannot fall back to the padded layout): the call fails where packed rows are not supported. */
#define COOT_SOURCE_PADDED 0
#define COOT_SOURCE_PACKED_F32 1
#define COOT_SOURCE_PACKED_BF16 2
typedef struct coot_packed_seqs { const int32_t* cu_seqlens; int total_tokens; int source; } coot_packed_seqs;
size_t coot_net_saved_bytes(const coot_net_config* cfg, int N, int L, int N2, int L2);
size_t coot_net_scratch_bytes(const coot_net_config* cfg, int N, int L, int N2, int L2);
/* Optional SECOND SEGMENT (feats2 [N2, L2, input_dim], lengths2 [N2]; N2 = 0 / NULL when unused): a second set
 * of sequences pushed through the same network in the same call (the reference calls net_video_local twice
 * per step, coot/model_retrieval.py:104 and :120).  pooled then holds N + N2 rows (segment 1 first). */
int coot_net_fwd(const coot_net_config* cfg, const float* params, const void* wpack, const float* pe,
                 const float* feats, const int64_t* lengths, int N, int L, const float* feats2,
                 const int64_t* lengths2, int N2, int L2, const float* hidden,
                 float* pooled, float* per_token, void* saved, size_t saved_bytes, void* scratch,
                 size_t scratch_bytes, int train, uint64_t seed, const uint64_t* seed_dev, coot_stream_t stream,
                 const coot_packed_seqs* packed /* NULL: padded rows */);
/* Dropout (train != 0) draws from a counter-based generator keyed by (seed + *seed_dev, site, element); seed_dev
 * is an optional DEVICE word the caller advances once per step — with it a captured HIP graph of the step draws new
 * masks on every replay; forward and backward of one step must see the same value.
 * grads: flat fp32 arena, ACCUMULATED (+=).  dhidden [N, hidden_dim] (written) or NULL.
 * dfeats [N, L, input_dim] fp32 (written; only supported when use_input_fc == 0) or NULL. */
int coot_net_bwd(const coot_net_config* cfg, const float* params, const void* wpack, const float* pe,
                 const float* feats, const int64_t* lengths, int N, int L, const float* feats2,
                 const int64_t* lengths2, int N2, int L2, const float* hidden,
                 const float* dpooled, float* grads, float* dhidden, float* dfeats, void* saved,
                 size_t saved_bytes, void* scratch, size_t scratch_bytes, int train, uint64_t seed,
                 const uint64_t* seed_dev, coot_stream_t stream,
                 const coot_packed_seqs* packed /* the forward's */);

/* coot_net_bwd accumulates into `grads`.  coot_net_grads_overwrite(1) (thread-local, until switched off): the weight MATRIX
 * gradients (input FC, QKV / output / feed-forward projections, pooling FCs — each the result of exactly one weight-gradient
 * problem of the pass) are WRITTEN instead; biases and LayerNorm parameters are still accumulated.  coot_nets_zero_grads zeroes
 * the gradient arenas of n networks: all of them (skip_matrices = 0), or only what is still accumulated in that mode
 * (skip_matrices = 1: < 1 % of the arena, one launch).  coot_train_step uses the pair: no 30 MB fill, no read-back of the
 * destination by the weight-gradient launches. */
int coot_net_grads_overwrite(int on);
int coot_nets_zero_grads(int n, const coot_net_config* const* cfgs, float* const* grads, int skip_matrices,
                         coot_stream_t stream);
/* host-only (tests): the (offset, elements) ranges of the arena that mode leaves to the backward; returns their number */
int coot_debug_written_matrices(const coot_net_config* cfg, int64_t* offsets, int64_t* sizes, int max_ranges);
/* the same launch also zeroes n_extra fp32 ranges (extra[i], extra_n[i] floats) */
int coot_nets_zero_grads_ex(int n, const coot_net_config* const* cfgs, float* const* grads, int skip_matrices,
                            float* const* extra, const int64_t* extra_n, int n_extra, coot_stream_t stream);

/* ---- clip -> video packing: the python loop of coot/model_retrieval.py:121-136 ---------------- */
int coot_pack_fwd(const float* emb, const int64_t* counts, int B, int Cmax, int D, float* out /*[B,Cmax,D]*/,
                  uint8_t* mask /*[B,Cmax] 1 = pad*/, int64_t* lens /*[B]*/, coot_stream_t stream);
int coot_pack_bwd(const float* dout, const int64_t* counts, int B, int Cmax, int D, float* demb /* += */,
                  coot_stream_t stream);

/* ---- losses ------------------------------------------------------------------------------------
 * compute_total_constrastive_loss (coot/trainer_retrieval.py:148-182) with ContrastiveLoss
 * (coot/loss_fn.py:63-100): six un-normalised embedding sets, loss accumulated into *loss,
 * gradients accumulated into d* (all NULL => forward only). */
typedef struct coot_contrastive_config {
  float margin;
  float weight_high, weight_high_internal, weight_low, weight_low_internal, weight_context,
      weight_context_internal;
} coot_contrastive_config;
size_t coot_contrastive_scratch_bytes(int n_high, int n_low, int d_high, int d_low);
int coot_contrastive_fwd_bwd(const coot_contrastive_config* cfg, int n_high, int n_low, int d_high, int d_low,
                             const float* vid_emb, const float* par_emb, const float* clip_emb,
                             const float* sent_emb, const float* vid_ctx, const float* par_ctx, float* loss,
                             float* d_vid_emb, float* d_par_emb, float* d_clip_emb, float* d_sent_emb,
                             float* d_vid_ctx, float* d_par_ctx, void* scratch, size_t scratch_bytes,
                             coot_stream_t stream);
/* The same, restricted to a part of the seven terms: COOT_CONTRASTIVE_GLOBAL = the terms on (vid_emb, par_emb) — the outputs of
 * the global networks (trainer_retrieval.py:168-171); COOT_CONTRASTIVE_LOCAL = the terms on (clip_emb, sent_emb) and
 * (vid_ctx, par_ctx) (:172-182), which need the local networks only.  Two calls with the two parts on the same scratch buffer
 * add up to the full call (disjoint scratch regions and gradient outputs, *loss added atomically) and may run on different
 * streams: coot_train_step computes the local part on the text stream next to the video side's global backward (which does not
 * read its gradients).  A part whose sets all fit the LDS (<= 128 rows, (rows + 16) (d + 8) bf16 <= 150 KB: the global part at the
 * paper shapes) takes two launches instead of three, with bit-identical results (coot_set_option("cl_small", 0): three). */
#define COOT_CONTRASTIVE_GLOBAL 1
#define COOT_CONTRASTIVE_LOCAL 2
int coot_contrastive_fwd_bwd_part(const coot_contrastive_config* cfg, int n_high, int n_low, int d_high, int d_low,
                                  const float* vid_emb, const float* par_emb, const float* clip_emb,
                                  const float* sent_emb, const float* vid_ctx, const float* par_ctx, float* loss,
                                  float* d_vid_emb, float* d_par_emb, float* d_clip_emb, float* d_sent_emb,
                                  float* d_vid_ctx, float* d_par_ctx, void* scratch, size_t scratch_bytes, int part,
                                  coot_stream_t stream);

/* fp32 REFERENCE MODE of coot_contrastive_fwd_bwd (the COOT_DTYPE_F32 of the losses; csrc/loss_f32.hip): the same arguments and
 * semantics — F.normalize, the seven ContrastiveLoss terms of coot/trainer_retrieval.py:148-182 / coot/loss_fn.py:63-100, *loss and
 * the six gradients ACCUMULATED — computed by plain fp32 FMA kernels in a fixed summation order: no MFMA, no bf16 operand, no
 * atomics.  With coot_net_config.dtype = COOT_DTYPE_F32 networks around it (and coot_cyclecons_fwd_bwd, which is fp32 VALU code in
 * both modes) the whole forward + loss + backward runs in the library in fp32: every parameter gradient of the reference's eval
 * fixtures to <= 1e-4 relative (tests/test_gpu_f32_mode.py).  A checker: one GPU, the full batch, never what bench.py times.
 * scratch: coot_contrastive_f32_scratch_bytes (NOT coot_contrastive_scratch_bytes). */
size_t coot_contrastive_f32_scratch_bytes(int n_high, int n_low, int d_high, int d_low);
int coot_contrastive_fwd_bwd_f32(const coot_contrastive_config* cfg, int n_high, int n_low, int d_high, int d_low,
                                 const float* vid_emb, const float* par_emb, const float* clip_emb,
                                 const float* sent_emb, const float* vid_ctx, const float* par_ctx, float* loss,
                                 float* d_vid_emb, float* d_par_emb, float* d_clip_emb, float* d_sent_emb,
                                 float* d_vid_ctx, float* d_par_ctx, void* scratch, size_t scratch_bytes,
                                 coot_stream_t stream);

/* The same loss for data-parallel training: sets[i] are the six GATHERED sets (row stride ld[i] floats: they may be column
 * slices of the all-gather buffers), the loss is the mean over the global batch — *loss receives THIS RANK'S SHARE of it (the
 * hinge terms of its rows against every column: the caller adds the shares of all ranks, e.g. in the gradient all-reduce;
 * scoring only its own strips keeps the per-rank cost linear in the global batch); gradients are produced only for this
 * rank's rows — [own_high0, own_high0 + own_high) of the per-video sets (0 vid_emb, 1 par_emb, 4 vid_ctx, 5 par_ctx),
 * [own_low0, own_low0 + own_low) of the per-clip sets (2 clip_emb, 3 sent_emb) — accumulated into the compact arrays
 * d_own[i] [own rows, d]. */
int coot_contrastive_fwd_bwd_dp(const coot_contrastive_config* cfg, int n_high, int n_low, int d_high, int d_low,
                                const float* const sets[6], const int64_t ld[6], float* loss, float* const d_own[6],
                                int own_high0, int own_high, int own_low0, int own_low, void* scratch,
                                size_t scratch_bytes, coot_stream_t stream);

/* The same, reading the rows straight from the BLOCKS of ONE all-gather (no repacking between the collective and the loss): every
 * rank contributes one block holding its six sets; set s of rank r has counts_high[r] (sets 0, 1, 4, 5) or counts_low[r]
 * (sets 2, 3) rows of stride ld[s] floats and starts at blocks + set_base[s * world + r] (floats, multiples of 4).  The global
 * batch is the concatenation of the ranks' rows in rank order; gradients for rank `rank`'s rows into d_own[s] [own rows, d];
 * *loss receives this rank's share.  world <= COOT_DP_MAX_RANKS (the block table travels in the kernel arguments).
 * counts_* / set_base / ld are host arrays.  Replaces the gather + concatenation of nn.DataParallel (nntrainer/trainer_base.py:126-129). */
#define COOT_DP_MAX_RANKS 16
int coot_contrastive_fwd_bwd_dp_blocks(const coot_contrastive_config* cfg, int world, int rank, const int64_t* counts_high,
                                       const int64_t* counts_low, int d_high, int d_low, const float* blocks,
                                       const int64_t* set_base, const int64_t ld[6], float* loss, float* const d_own[6],
                                       void* scratch, size_t scratch_bytes, coot_stream_t stream);

/* CycleConsistencyLoss.forward + get_total_loss(num_samples=1) (coot/loss_fn.py:143-319).
 * idx_* are the th.multinomial draws (one valid position per video).  loss += weight *
 * inv_batch * sum_b (l_clip[b, idx_clip[b]] + l_sent[b, idx_sent[b]]); rows_* optional [B, C]. */
int coot_cyclecons_fwd_bwd(const float* clip, const float* sent, const int64_t* clip_lens,
                           const int64_t* sent_lens, const int64_t* idx_clip, const int64_t* idx_sent, int B,
                           int Cc, int Cs, int D, float weight, float inv_batch, float* loss, float* rows_clip,
                           float* rows_sent, float* dclip, float* dsent, coot_stream_t stream);

/* ---- input side: batch collation into a staging arena ---------------------------------------------
 * One feature level of RetrievalDataset.collate_fn (coot/dataset_retrieval.py:335-463: the zero-padded tensor + the bool
 * mask the loops at :362-364, :378-380, :404-414, :438-452 fill): n sequences, seq[i] -> fp32 [rows[i], dim], are written to
 * dst [n, max_rows, dim] (fp32 copy, or bf16 round-to-nearest-even when dst_bf16 != 0), rows beyond rows[i] zeroed;
 * mask [n, max_rows] bytes (optional): 0 = data, 1 = padding.  Host-only: dst is normally a slice of ONE pinned arena that
 * carries all four levels, lengths and masks and goes to the device with one hipMemcpyAsync on a copy stream.  threads > 1
 * splits the sequences over that many host threads. */
int coot_collate_level(const float* const* seq, const int64_t* rows, int64_t n, int64_t dim, int64_t max_rows, int dst_bf16,
                       void* dst, uint8_t* mask, int threads);
/* Packed at the source ("produce packed varlen features directly in pinned memory, drop the zero padding"): the same n
 * sequences written BACK TO BACK, dst [sum rows, dim] (fp32 copy or bf16 round-to-nearest-even), and their row starts
 * cu_seqlens [n + 1] (int32, cu_seqlens[0] = 0) — exactly what coot_packed_seqs / coot_step_batch.cu_vis take, so one call per side
 * (the B videos followed by the Nc clips; the B paragraphs followed by the Nc sentences) produces the side's input.  Replaces the
 * padded blocks of RetrievalDataset.collate_fn (coot/dataset_retrieval.py:362-364, :378-380, :404-414, :438-452); the padded
 * batch is recoverable bit-exactly (dataset_retrieval.unpack_batch, tests/test_input_pipeline.py).  Host-only. */
int coot_collate_packed(const float* const* seq, const int64_t* rows, int64_t n, int64_t dim, int dst_bf16, void* dst,
                        int32_t* cu_seqlens, int threads);

/* ---- retrieval ranking on the device -----------------------------------------------------------
 * validate_epoch's metric tail (coot/trainer_retrieval.py:397-402, :425-436) + nntrainer/retrieval.py:31-98 for one pair
 * of embedding sets emb1, emb2 [N, d] fp32 (e.g. vid_emb / par_emb of the whole validation set), both directions:
 *   normalize != 0: rows are first divided by sqrt(sum x^2) (the reference's manual normalisation, no eps);
 *   ranks_12[i] = position of i in argsort(d[i])[::-1], d = emb1 . emb2^T (fp32 FMA chains in k order);  ranks_21: the same
 *   for d^T.  Exact ties are ordered as the reversal of a stable ascending sort (j > i ahead of i);
 *   metrics (optional, 14 floats): {r1, r5, r10, r50, medr, meanr, sum} for 1 -> 2, then for 2 -> 1 (VALKEYS order,
 *   R@K as fractions, medr = floor(median) + 1, meanr = mean + 1);
 *   sim_out (optional, [N, N]): the similarity matrix the ranks were counted on (testing aid).
 * The similarity matrix is never materialised otherwise.  workspace: coot_retrieval_workspace_bytes(N, d). */
size_t coot_retrieval_workspace_bytes(int N, int d);
int coot_retrieval_ranks(const float* emb1, const float* emb2, int N, int d, int normalize, int32_t* ranks_12, int32_t* ranks_21,
                         float* metrics, float* sim_out, void* workspace, size_t workspace_bytes, coot_stream_t stream);

/* ---- the same ranking, one strip of rows at a time (sharded validation: every rank of a data-parallel run takes a strip) ----
 * coot_retrieval_ranks_part counts on the rows [row0, row0 + rows) of d = emb1 . emb2^T against all N columns.  It zeroes
 * counts_12 and counts_21 (int32 [N] each) itself, then
 *   counts_12[i] = ranks_12[i] of coot_retrieval_ranks for row0 <= i < row0 + rows, 0 elsewhere;
 *   counts_21[j] = the number of rows i of the strip that are ahead of j in column j, for every j;
 *   sim_out (optional, [rows, N]): the strip of the similarity matrix (testing aid).
 * Normalisation, the similarity chain, the comparison and the tie rule are those of coot_retrieval_ranks.  row0 and rows are
 * arbitrary (0 <= row0, 0 <= rows, row0 + rows <= N; not tile aligned); rows == 0 only zeroes the outputs.
 * STRIP CONTRACT: for any partition of [0, N) into strips, the element-wise integer sums of counts_12 and of counts_21 over the
 * strips equal ranks_12 and ranks_21 of coot_retrieval_ranks exactly, in any order of summation (an all-reduce of the counts),
 * and the stacked sim_out strips equal its sim_out bit for bit.
 * coot_retrieval_metrics computes the 14 metric floats of coot_retrieval_ranks from two rank vectors (e.g. the reduced counts):
 * the same bits that call writes for the same ranks.  Ranks must lie in [0, N).  Its workspace holds 2 N int32 (4-byte aligned;
 * a workspace of coot_retrieval_ranks_part_workspace_bytes(N, d) is large enough).
 * Neither call retains a pointer: every buffer may be freed or reused once the work enqueued on `stream` has completed. */
size_t coot_retrieval_ranks_part_workspace_bytes(int N, int d);
int coot_retrieval_ranks_part(const float* emb1, const float* emb2, int N, int d, int normalize, int row0, int rows, int32_t* counts_12,
                              int32_t* counts_21, float* sim_out, void* workspace, size_t workspace_bytes, coot_stream_t stream);
int coot_retrieval_metrics(const int32_t* ranks_12, const int32_t* ranks_21, int N, float* metrics, void* workspace, size_t workspace_bytes,
                           coot_stream_t stream);

/* ---- top-K retrieval search on the device: M queries against an N-row gallery ------------------------------------------
 * What the model is trained for, for sets that need not be square or aligned (exported embeddings, a few text queries against
 * every clip): row i of idx_out / score_out [M, K] holds the K best gallery rows for query i and their similarities, best first,
 * by the total order (similarity descending, then gallery index descending) = np.argsort(s[i], kind="stable")[::-1][:K].
 *   normalize != 0: every row of both sets is first divided by sqrt(sum x^2), no eps (as in coot_retrieval_ranks);
 *   s = queries . gallery^T is the fp32 FMA chain of coot_retrieval_ranks (k order, chunks of 32): for M = N the optional
 *   sim_out [M, N] (testing aid) equals that call's sim_out bit for bit, idx_out[i, r] == i exactly when ranks_12[i] == r
 *   (r < K: the same tie rule, a later index is ahead), and idx_out[:, 0] is the reference's top1 (nntrainer/retrieval.py:79-98)
 *   wherever the row maximum is unique;
 *   1 <= K <= min(N, 128); M, N >= 1, independent, any size.
 * No M x N array exists unless sim_out is given: the selection runs on the tile accumulators, the column range is split over
 * workgroups and the per-row partial lists are merged in a second launch.  Every comparison is on the total order above, so the
 * result does not depend on the split count or on the workgroup schedule (coot_set_option("rt_topk_splits", n) fixes the number
 * of column splits for tests, 0 = automatic; set it before asking for the workspace size).  A row with non-finite similarities
 * has unspecified order.  workspace: coot_retrieval_topk_workspace_bytes(M, N, d, K) = the row norms and the partial lists,
 * (M + N) floats + M x splits x K 64-bit words, splits <= 64. */
size_t coot_retrieval_topk_workspace_bytes(int M, int N, int d, int K);
int coot_retrieval_topk(const float* queries, const float* gallery, int M, int N, int d, int K, int normalize, int32_t* idx_out,
                        float* score_out, float* sim_out, void* workspace, size_t workspace_bytes, coot_stream_t stream);

/* ---- the same search for a few queries on a prepared gallery (low latency) ---------------------------------------------
 * How a trained model is used: one paragraph, or a handful, against a corpus that stays in device memory between calls.
 * coot_retrieval_row_norms writes norms[j] = sqrt(sum x^2) of every row of rows [N, d]: exactly the divisor normalize != 0 uses
 * in the calls above.  It is the "prepared" part: the caller computes it once per gallery and owns the buffer (the library
 * retains no pointer); a gallery that changes needs its norms again.
 * coot_retrieval_topk_few: 1 <= M <= COOT_RETRIEVAL_FEW_MAX queries, 1 <= K <= min(N, 128).  idx_out, score_out [M, K] and the
 * optional sim_out [M, N] (testing aid) are byte for byte what coot_retrieval_topk writes for the same inputs, with
 *   gallery_norms != NULL: normalize = 1; the query norms are computed inside the call, the gallery's are taken as given;
 *   gallery_norms == NULL: normalize = 0, rows used as they are.
 * One gallery row per thread and one accumulator per query instead of 64 x 64 tiles: the same fp32 FMA chain per element (k order,
 * chunks of 32), the same total order in selection and merge, so the result does not depend on the row split or the schedule
 * (coot_set_option("rt_few_splits", n) fixes the number of row splits for tests, 0 = automatic; the workspace size does not
 * depend on it).  The gallery is read once per call.  workspace (16-byte aligned): coot_retrieval_topk_few_workspace_bytes =
 * the query norms, the normalised queries [d rounded up to 32, 16] and the partial lists, M x splits x K 64-bit words (+ 1/32 of
 * that for the merge rounds), splits <= min(ceil(N / 128), 1024): it does not grow with N beyond 131 072 rows.
 * A refused call (null pointer, M or K outside its range, workspace too small) writes nothing.  No allocation, no synchronisation. */
#define COOT_RETRIEVAL_FEW_MAX 16
int coot_retrieval_row_norms(const float* rows, int N, int d, float* norms, coot_stream_t stream);
size_t coot_retrieval_topk_few_workspace_bytes(int M, int N, int d, int K);
int coot_retrieval_topk_few(const float* queries, const float* gallery, const float* gallery_norms, int M, int N, int d, int K,
                            int32_t* idx_out, float* score_out, float* sim_out, void* workspace, size_t workspace_bytes,
                            coot_stream_t stream);

/* ---- the prepared gallery stored in 16-bit floats ---------------------------------------------------------------------
 * Only the storage changes: a bfloat16 or IEEE-half value widens to fp32 exactly, and the arithmetic and the total order are those
 * above.  dtype / gallery_dtype: COOT_GALLERY_BF16 or COOT_GALLERY_F16, the element type of the [N, d] rows (2-byte aligned, row
 * stride d), independent of the library's MFMA operand format: both builds serve both.
 * coot_retrieval_row_norms_h: norms[j] = the bytes coot_retrieval_row_norms writes for the rows widened to fp32.
 * coot_retrieval_topk_few_h: idx_out, score_out and the optional sim_out are byte for byte the results of coot_retrieval_topk_few on
 * the gallery widened to fp32, with the same queries (fp32), gallery_norms (NULL: rows used as they are), M, K, workspace
 * (coot_retrieval_topk_few_workspace_bytes: it does not depend on the gallery's type) and split option; no widened copy is made:
 * the sweep reads the 16-bit rows (half the bytes) and widens at staging.  Neither call retains a pointer.  A refused call
 * (unknown dtype, null pointer, M or K outside its range, workspace too small) writes nothing.  No allocation, no synchronisation. */
#define COOT_GALLERY_BF16 1
#define COOT_GALLERY_F16 2
int coot_retrieval_row_norms_h(const void* rows, int dtype, int N, int d, float* norms, coot_stream_t stream);
int coot_retrieval_topk_few_h(const float* queries, const void* gallery, int gallery_dtype, const float* gallery_norms, int M, int N,
                              int d, int K, int32_t* idx_out, float* score_out, float* sim_out, void* workspace, size_t workspace_bytes,
                              coot_stream_t stream);

/* ---- filtered search: a keep mask over the gallery rows ------------------------------------------------------------------
 * keep: device bytes [N], nonzero = the gallery row may be returned.  A row whose byte is zero is never a candidate: a search
 * restricted to a subset, or one that skips deleted rows, without copying or renumbering the gallery.  A similarity is the same
 * FMA chain wherever its row lies and the total order survives a monotone renumbering, so idx_out / score_out are, byte for byte,
 * the unmasked call on the compacted gallery (the kept rows in order) with its indices mapped back to rows of the full gallery.
 *   K is validated against N only, 1 <= K <= min(N, 128): counting the mask would need a host synchronisation.  With c < K kept
 *   rows, slots r >= c of a query hold idx = -1, score = -inf.  (Inside the kernels an unfilled slot is the entry word 0, which is
 *   a real entry only for a similarity that is the all-ones NaN at gallery row 0: a masked search reports that one as unfilled.)
 *   sim_out, when given, is not affected by the mask: every similarity, the bytes of the unmasked call.
 *   sim_out == NULL: a block of rows without a kept one (64 rows in coot_retrieval_topk_masked, 128 in
 *   coot_retrieval_topk_few_masked) is skipped before its first load: no gallery bytes, no FMAs.  Contiguous masks make a search
 *   cheaper, scattered ones do not.  Norms, when used, are still those of all N rows.
 *   keep == NULL: the unmasked kernels, exactly the launches of the unmasked call.
 * coot_retrieval_topk_masked: coot_retrieval_topk with keep.  coot_retrieval_topk_few_masked: coot_retrieval_topk_few
 * (gallery_dtype == COOT_GALLERY_F32) or coot_retrieval_topk_few_h (COOT_GALLERY_BF16, COOT_GALLERY_F16) with keep.  The mask
 * needs no workspace: coot_retrieval_topk_workspace_bytes and coot_retrieval_topk_few_workspace_bytes serve them, and the split
 * options act as on the unmasked calls.  A refused call (unknown dtype, null pointer other than keep, M or K outside its range,
 * workspace too small) returns before any launch and writes nothing.  No allocation, no synchronisation; no pointer is retained. */
#define COOT_GALLERY_F32 0
int coot_retrieval_topk_masked(const float* queries, const float* gallery, const uint8_t* keep, int M, int N, int d, int K, int normalize,
                               int32_t* idx_out, float* score_out, float* sim_out, void* workspace, size_t workspace_bytes,
                               coot_stream_t stream);
int coot_retrieval_topk_few_masked(const float* queries, const void* gallery, int gallery_dtype, const float* gallery_norms,
                                   const uint8_t* keep, int M, int N, int d, int K, int32_t* idx_out, float* score_out, float* sim_out,
                                   void* workspace, size_t workspace_bytes, coot_stream_t stream);

/* ---- the tile search on a prepared gallery: many queries, any storage, stored norms -------------------------------------------
 * coot_retrieval_topk_index: M >= 1 queries (fp32) against the gallery as a prepared index holds it, gallery_dtype COOT_GALLERY_F32,
 * _BF16 or _F16, with the norms it already has.  idx_out, score_out [M, K] and the optional sim_out [M, N] are byte for byte what
 *   coot_retrieval_topk_masked(queries, W, keep, M, N, d, K, gallery_norms != NULL, ...)
 * writes, W = the gallery widened to fp32, whenever gallery_norms holds what coot_retrieval_row_norms / coot_retrieval_row_norms_h
 * compute for it (NULL: rows used as they are): unfilled slots under a mask (-1, -inf) included, for every split count
 * (coot_set_option("rt_topk_splits", n), as above), and so for M <= COOT_RETRIEVAL_FEW_MAX also the bytes of
 * coot_retrieval_topk_few_masked.  The walk over 64 x 64 tiles, the FMA chain, the selection and the merge are those of
 * coot_retrieval_topk; a gallery element is widened as it is staged, no widened copy is made, and the gallery's norms are read, not
 * recomputed: one launch computes the M query norms, and no pass over the gallery precedes the search.  keep: as in the filtered
 * searches above (NULL: none; without sim_out a tile of 64 rows that keeps nothing is skipped).
 * workspace (8-byte aligned): coot_retrieval_topk_index_workspace_bytes(M, N, d, K), exact = M floats and M x splits x K 64-bit
 * words, each rounded up to 256 bytes; it depends on the split option: set that first.  A refused call (unknown dtype, null
 * pointer other than gallery_norms, keep and sim_out, M, N or d < 1, K outside 1 .. min(N, 128), a workspace one byte short) returns
 * before any launch and writes nothing.  No allocation, no synchronisation; no pointer is retained. */
size_t coot_retrieval_topk_index_workspace_bytes(int M, int N, int d, int K);
int coot_retrieval_topk_index(const float* queries, const void* gallery, int gallery_dtype, const float* gallery_norms, const uint8_t* keep,
                              int M, int N, int d, int K, int32_t* idx_out, float* score_out, float* sim_out, void* workspace,
                              size_t workspace_bytes, coot_stream_t stream);

/* ---- grouped search: the K best groups of gallery rows, one row for each ------------------------------------------------------
 * groups: device int32 [N], groups[j] = the group of gallery row j (the video of a clip, a speaker, a cluster of near-duplicates);
 * num_groups = G.  For every query: take the ranking of all rows that coot_retrieval_topk defines (score descending, then row
 * descending), drop the rows that keep masks out and the rows whose group id lies outside [0, G), keep the first row of every group,
 * and return the first K of those: group_out, idx_out, score_out [M, K] = the group, its best row and that row's score, the fp32
 * similarity of the searches above (the same FMA chain; sim_out [M, N], optional, holds every similarity).  With fewer than K groups
 * left, the tail is group -1, idx -1, score -inf, the filtered searches' unfilled slot.  Exact: with groups[j] = j idx_out and
 * score_out are byte for byte coot_retrieval_topk_few_masked's and group_out equals idx_out; with one group slot 0 is that search at
 * K = 1.  An out-of-range id is never used as an index.
 *   1 <= M <= COOT_RETRIEVAL_FEW_MAX, 1 <= K <= min(N, 128) (K is not checked against G or the mask), 1 <= num_groups <= 2^26;
 *   gallery_dtype COOT_GALLERY_F32, _BF16 or _F16; gallery_norms NULL: rows used as they are; keep NULL: no filter.
 * The few-query sweep (one gallery row per thread) raises a table best [M][G] of 64-bit top-K entries with an unsigned 64-bit atomic
 * maximum: an entry is (score image, row) under a strict total order, so a group's best row does not depend on arrival order, nor
 * the result on the sweep's row splits (coot_set_option("rt_few_splits", n)), the table ranges of the selection
 * (coot_set_option("rt_grouped_splits", n), 0 = automatic) or the schedule.  The table is reset inside every call: nothing survives in
 * a workspace.  workspace (16-byte aligned): coot_retrieval_topk_grouped_workspace_bytes(M, N, d, K, num_groups) = the query norms, the
 * normalised queries, M x G entries and M x ranges x K entries of lists, ranges <= 256; it depends on neither option.  A refused call
 * (unknown dtype, null pointer other than gallery_norms, keep and sim_out, M, K or num_groups outside its range, workspace misaligned
 * or too small) returns before any launch and writes nothing.  No allocation, no synchronisation; no pointer is retained. */
size_t coot_retrieval_topk_grouped_workspace_bytes(int M, int N, int d, int K, int num_groups);
int coot_retrieval_topk_grouped(const float* queries, const void* gallery, int gallery_dtype, const float* gallery_norms, const uint8_t* keep,
                                const int32_t* groups, int num_groups, int M, int N, int d, int K, int32_t* group_out, int32_t* idx_out,
                                float* score_out, float* sim_out, void* workspace, size_t workspace_bytes, coot_stream_t stream);

/* ---- multi-vector search: a paragraph's sentences against grouped rows (MaxSim, late interaction) -----------------------------
 * queries [M, d] are the sentences of P paragraphs, concatenated; offsets: DEVICE int32 [P + 1], paragraph p = the query rows
 * [offsets[p], offsets[p + 1]), which may be empty; a caller passes 0 = offsets[0] <= ... <= offsets[P] = M.  groups, num_groups = G and
 * keep as in the grouped search.  The definition, byte for byte:
 *   entry: best[i][g] = the first row of group g in sentence i's ranking of the kept rows with an id inside [0, G) (score descending,
 *     then row descending): what the grouped search returns for g.  Its score is the fp32 similarity of the other searches, -0 as +0.
 *   candidates: group g for paragraph p, if p is not empty and every sentence of p has an entry for g.
 *   score: s = +0; for i = offsets[p] .. offsets[p + 1] - 1 ascending: s = s + score(best[i][g]) — plain fp32 adds in that order.
 *   order: s descending, then GROUP id descending (the grouped search breaks ties by row; a paragraph has no single row).
 * group_out, score_out [P, K]: the K first candidates of every paragraph, the tail (-1, -inf) where fewer exist, every slot of an
 * empty paragraph.  row_out, row_score_out [M, K], the alignment: for sentence i of paragraph p, slot r = the row and score of
 * best[i][group_out[p][r]], (-1, -inf) where group_out[p][r] is -1.  sim_out [M, N], optional: every similarity, mask or not.
 * Sums that are NaN or infinite: no fault and no index out of range, otherwise unspecified.
 *   1 <= P <= 65535, M >= 1, M x num_groups <= 2^28, 1 <= K <= min(N, 128) (not checked against G or the mask), 1 <= num_groups <= 2^26.
 * The table best [M][G] of the grouped search is reset once, raised by the grouped search's sweep per 16 sentences, read once by a
 * selection that sums column segments, and once per result slot by the alignment.  The result depends on neither split option
 * ("rt_few_splits", "rt_grouped_splits": the ranges of the selection) nor the schedule; nothing survives in a workspace.
 * offsets is read on the device and never trusted: a paragraph is clamped to i0 = clamp(offsets[p], 0, M), i1 = clamp(offsets[p + 1],
 * i0, M); with entries out of order the alignment of a sentence follows the paragraph a binary search finds, if that one holds it,
 * and is (-1, -inf) otherwise.  workspace (16-byte aligned): coot_retrieval_topk_multi_workspace_bytes(P, M, N, d, K, num_groups) = the
 * operand table of one slice, M x G entries and P x ranges x K entries of lists, ranges <= 256; it needs no device, depends on neither
 * option and is 256 for arguments out of range.  A refused call (unknown dtype, null pointer other than gallery_norms, keep and
 * sim_out, P, M, K, num_groups or the table outside its range, workspace misaligned or too small) returns before any launch and
 * writes nothing.  No allocation, no synchronisation; no pointer is retained. */
size_t coot_retrieval_topk_multi_workspace_bytes(int P, int M, int N, int d, int K, int num_groups);
int coot_retrieval_topk_multi(const float* queries, const void* gallery, int gallery_dtype, const float* gallery_norms, const uint8_t* keep,
                              const int32_t* groups, int num_groups, const int32_t* offsets, int P, int M, int N, int d, int K,
                              int32_t* group_out, float* score_out, int32_t* row_out, float* row_score_out, float* sim_out, void* workspace,
                              size_t workspace_bytes, coot_stream_t stream);

/* ---- scoped search: every query has its own slice of the gallery ----------------------------------------------------------------
 * groups: device int32 [N], groups[j] = the id of gallery row j (the video of a clip, a tenant, a split), any int32 value; NULL: every
 * row is its own id, groups[j] = j.  scope: device int32 [M], one id per query.  Row j is eligible for query i when it passes keep
 * (NULL: no filter) and
 *   exclude == 0 ("only"):    groups[j] == scope[i]  — within one video: which clip of it answers the sentence;
 *   exclude == 1 ("exclude"): groups[j] != scope[i]  — everything but one video: neighbours outside a clip's own video.
 * The compare is integer equality: no range and no num_groups.  An id that no row carries selects nothing under only (every slot of
 * that query is unfilled) and excludes nothing under exclude.  idx_out, score_out [M, K]: row i is, byte for byte, what
 * coot_retrieval_topk_few_masked returns for query i alone with keep = the flags of its eligible rows: the same fp32 FMA chain, the
 * same total order (score descending, then the larger row), idx -1 / score -inf in the slots that fewer than K eligible rows leave
 * unfilled.  sim_out [M, N], optional: every similarity, eligible or not.
 *   1 <= M <= COOT_RETRIEVAL_FEW_MAX, 1 <= K <= min(N, 128) (K is not checked against the scopes or the mask);
 *   gallery_dtype COOT_GALLERY_F32, _BF16 or _F16; gallery_norms NULL: rows used as they are.
 * One sweep of the gallery serves all M queries: the thread of a row forms a 16-bit word, bit i = eligible for query i, which gates
 * the candidates.  Without sim_out a block of 128 rows in which no row is eligible for any query is not read at all, so under only,
 * with a scope's rows adjacent, a call reads the blocks those rows lie in; under exclude, or with scattered ids, it reads the gallery
 * once.  The result does not depend on the sweep's row splits (coot_set_option("rt_few_splits", n)).  workspace (16-byte aligned):
 * coot_retrieval_topk_scoped_workspace_bytes(M, N, d, K), the few-query search's layout; it needs no device, does not depend on the
 * option and is 256 for arguments out of range.  A refused call (unknown dtype, null pointer other than gallery_norms, keep, groups and
 * sim_out, M or K outside its range, exclude not 0 or 1, workspace misaligned or too small) returns before any launch and writes
 * nothing.  No allocation, no synchronisation; no pointer is retained. */
size_t coot_retrieval_topk_scoped_workspace_bytes(int M, int N, int d, int K);
int coot_retrieval_topk_scoped(const float* queries, const void* gallery, int gallery_dtype, const float* gallery_norms, const uint8_t* keep,
                               const int32_t* groups, const int32_t* scope, int exclude, int M, int N, int d, int K, int32_t* idx_out,
                               float* score_out, float* sim_out, void* workspace, size_t workspace_bytes, coot_stream_t stream);

/* ---- adjusted search: a number per gallery row is taken off its similarity before the selection -----------------------------------
 * offset: device fp32 [N].  The adjusted score is a(i, j) = s(i, j) - offset[j], one IEEE fp32 subtraction after the chain, where
 * s(i, j) is the fp32 similarity every search here ranks on, bit for bit the sim_out of coot_retrieval_topk_few_masked.  idx_out,
 * score_out [M, K]: the K best rows of every query that pass keep (NULL: no filter) by a, in the order of every search (a descending,
 * then the larger row), and the bytes of a; idx -1 / score -inf in the slots that fewer than K kept rows leave unfilled.  offset[j] =
 * +inf gives a = -inf: the row is still a row and is returned with its index once nothing better is left, ties at -inf going to the
 * larger row; offset[j] = -inf puts the row first; a NaN is ordered as a NaN similarity is.  sim_out [M, N], optional: the raw s of
 * every row, kept or not.  A hubness correction (coot_retrieval_hub_offsets: CSLS), a recency boost, a popularity prior or a
 * calibration constant per source are all such an offset.
 *   1 <= M <= COOT_RETRIEVAL_FEW_MAX, 1 <= K <= min(N, 128) (K is not checked against the mask);
 *   gallery_dtype COOT_GALLERY_F32, _BF16 or _F16; gallery_norms NULL: rows used as they are.
 * One sweep of the gallery serves all M queries, the few-query search's with one more 4-byte load per row.  Without sim_out a block of
 * 128 rows in which keep leaves no row is not read at all.  The result depends on neither a query's batch-mates, the storage type
 * (beyond the exact widening) nor the sweep's row splits (coot_set_option("rt_few_splits", n)).  workspace (16-byte aligned):
 * coot_retrieval_topk_adjusted_workspace_bytes(M, N, d, K), the few-query search's layout; it needs no device, does not depend on the
 * option and is 256 for arguments out of range.  A refused call (unknown dtype, null pointer other than gallery_norms, keep and
 * sim_out, M or K outside its range, workspace misaligned or too small) returns before any launch and writes nothing.  No allocation,
 * no synchronisation; no pointer is retained. */
size_t coot_retrieval_topk_adjusted_workspace_bytes(int M, int N, int d, int K);
int coot_retrieval_topk_adjusted(const float* queries, const void* gallery, int gallery_dtype, const float* gallery_norms, const uint8_t* keep,
                                 const float* offset, int M, int N, int d, int K, int32_t* idx_out, float* score_out, float* sim_out,
                                 void* workspace, size_t workspace_bytes, coot_stream_t stream);

/* ---- adjusted search for a whole query set: one tile call -----------------------------------------------------------------------------
 * coot_retrieval_topk_adjusted for any M in one call: the same arguments, the same definition and, for every query, the same bytes of
 * idx_out, score_out [M, K] and sim_out [M, N] (optional: the raw s of every row, kept or not) as that call returns for the query in
 * any slice of COOT_RETRIEVAL_FEW_MAX.  64 queries x one 128-row block of the gallery per step of a workgroup, the selection of
 * coot_retrieval_knn_join behind the chain; offset[j] of a block waits in on-chip memory while the chain runs.  keep gates which rows
 * are candidates, the offset gates nothing (+inf: score -inf, still a row).  Without sim_out a block of 128 rows in which keep leaves
 * no row is not read at all; with it no block is skipped.
 *   1 <= M, ceil(M / 64) <= 65 535, 1 <= K <= min(N, 128) (K is not checked against the mask);
 *   gallery_dtype COOT_GALLERY_F32, _BF16 or _F16; gallery_norms NULL: rows used as they are, else the queries' norms are computed
 *   here (one launch) and both sides are divided at staging.
 * The gallery is cut into S shares (automatic: about 2 048 workgroups, no share under 8 blocks, at most 32;
 * coot_set_option("rt_adjusted_tile_splits", n) fixes S for tests, 0 = automatic), S > 1 merged by rank; the result depends on neither S,
 * the workgroup schedule nor a query's batch-mates.  workspace (16-byte aligned): coot_retrieval_topk_adjusted_tile_workspace_bytes(M,
 * N, d, K), exact = M floats and, for S > 1, M x S x K 64-bit words, each rounded up to 256 bytes (0 for arguments out of range).  A
 * refused call (unknown dtype, null pointer other than gallery_norms, keep and sim_out, M or K outside its range, workspace misaligned
 * or too small) returns before any launch and writes nothing.  No allocation, no synchronisation; no pointer is retained. */
size_t coot_retrieval_topk_adjusted_tile_workspace_bytes(int M, int N, int d, int K);
int coot_retrieval_topk_adjusted_tile(const float* queries, const void* gallery, int gallery_dtype, const float* gallery_norms, const uint8_t* keep,
                                      const float* offset, int M, int N, int d, int K, int32_t* idx_out, float* score_out, float* sim_out,
                                      void* workspace, size_t workspace_bytes, coot_stream_t stream);

/* ---- hubness offsets: the lists of a k-NN join into one number per row ---------------------------------------------------------------
 * scores (fp32), idx (int32): device [N][K], the lists coot_retrieval_knn_join wrote for the N gallery rows against a bank of
 * representative queries.  Per row j: c = the number of slots with idx >= 0 (the filled ones, a prefix); c > 0: acc = 0, then
 * acc += scores[j][t] for t = 0 .. c - 1 in that order, in fp32, and out[j] = 0.5f * (acc / (float)c); c == 0 (a masked row, or no
 * bank row eligible): out[j] = 0.  out: device fp32 [N], half the mean similarity of row j to its k nearest bank rows: with it as
 * the offset, coot_retrieval_topk_adjusted ranks by CSLS, 2 s(i, j) - r_q(i) - r_g(j), whose r_q is constant per query.  The bytes are
 * defined: one thread per row, no reassociation, no transcendental.  1 <= N, 1 <= K <= 128.  One launch; a refused call (null pointer,
 * N or K outside its range) returns before it and writes nothing.  No workspace, no allocation, no synchronisation; no pointer is
 * retained. */
int coot_retrieval_hub_offsets(const float* scores, const int32_t* idx, int N, int K, float* out, coot_stream_t stream);

/* ---- range search: every gallery row at or above a query's threshold ------------------------------------------------------------
 * Row j is a hit of query i when it passes keep (NULL: no filter) and s(i, j) >= thresholds[i], an IEEE fp32 compare: a NaN score or a
 * NaN threshold is no hit, -0 >= +0 holds, -inf returns every kept row whose score is not a NaN, +inf only rows that score +inf.
 * s(i, j) is the fp32 similarity every search here ranks on, bit for bit the sim_out of coot_retrieval_topk_few_masked.  The result is
 * CSR: offsets int64 [M + 1], offsets[0] = 0, and the hits of query i at offsets[i] .. offsets[i + 1] - 1 of rows_out (int32) and
 * scores_out (fp32, the bytes of s), in ascending row order.  A hit's position is computed, never claimed through an atomic: the bytes
 * do not depend on the schedule, on the other queries of a call or on the sweep's row splits (coot_set_option("rt_few_splits", n)).
 * Three calls on one stream, because only the middle one sees all queries and only the caller knows how much room the result may take:
 *   coot_retrieval_range_count: 1 <= M <= COOT_RETRIEVAL_FEW_MAX queries, one sweep of the gallery.  block_counts: the M rows of these
 *     queries in a table of int32, COOT_RETRIEVAL_RANGE_TABLE_ROW(N) entries per query (one per block of COOT_RETRIEVAL_RANGE_BLOCK
 *     gallery rows, and one more); it writes the first ceil(N / 128) entries of each row, the query's hits per block.  A block in
 *     which keep leaves no row is not read.  A search of more queries calls it once per 16, each on its rows of one table.
 *   coot_retrieval_range_scan: any M >= 1, all rows of the table at once: every row becomes the exclusive prefix of its counts with
 *     the query's total in its last entry; counts_out (int32 [M], optional) takes the totals, offsets (int64 [M + 1], optional) their
 *     prefix.  With offsets == NULL it is a count of hits and nothing more.  Nothing is read back: the host learns sizes only if the
 *     caller copies offsets[M].
 *   coot_retrieval_range_fill: the count call's arguments again (the same M queries, thresholds and keep), block_base = those queries'
 *     rows of the scanned table, offsets = their M entries of the offsets (offsets + i0 for queries i0 ..), and rows_out / scores_out
 *     with room for `capacity` entries: a hit whose position is below capacity is written, the others are not, and entries that no
 *     hit claims are not touched (a caller that cuts the result presets them).  It sweeps again, the same chain and so the same bits,
 *     but a block in which none of the call's queries has a hit is not read: under a selective threshold it reads few blocks.
 *   gallery_dtype COOT_GALLERY_F32, _BF16 or _F16; gallery_norms NULL: rows used as they are; thresholds: device fp32 [M].
 * workspace (16-byte aligned) of count and fill: coot_retrieval_range_workspace_bytes(M, N, d); it needs no device and is 256 for
 * arguments out of range.  count reads queries, gallery, gallery_norms, keep, thresholds and writes block_counts and the workspace;
 * scan reads and writes block_counts and writes offsets and counts_out; fill reads what count reads, block_base and offsets, and writes
 * rows_out, scores_out and the workspace.  A refused call (unknown dtype, a null pointer other than gallery_norms, keep, offsets and
 * counts_out of the scan, M outside its range, N or d < 1, capacity < 0, workspace misaligned or too small) returns before any launch and
 * writes nothing.  No allocation, no synchronisation; no pointer is retained. */
#define COOT_RETRIEVAL_RANGE_BLOCK 128
#define COOT_RETRIEVAL_RANGE_TABLE_ROW(N) (((N) + COOT_RETRIEVAL_RANGE_BLOCK - 1) / COOT_RETRIEVAL_RANGE_BLOCK + 1)
size_t coot_retrieval_range_workspace_bytes(int M, int N, int d);
int coot_retrieval_range_count(const float* queries, const void* gallery, int gallery_dtype, const float* gallery_norms, const uint8_t* keep,
                               const float* thresholds, int M, int N, int d, int32_t* block_counts, void* workspace, size_t workspace_bytes,
                               coot_stream_t stream);
int coot_retrieval_range_scan(int32_t* block_counts, int M, int N, int64_t* offsets, int32_t* counts_out, coot_stream_t stream);
int coot_retrieval_range_fill(const float* queries, const void* gallery, int gallery_dtype, const float* gallery_norms, const uint8_t* keep,
                              const float* thresholds, int M, int N, int d, const int32_t* block_base, const int64_t* offsets, int64_t capacity,
                              int32_t* rows_out, float* scores_out, void* workspace, size_t workspace_bytes, coot_stream_t stream);

/* ---- range search for many queries: the count and the fill pass on the 64 x 64 tile -----------------------------------------------
 * The range search above, same hit rule, same table, same scan, same CSR result, for any number of queries in one call per pass:
 *   coot_retrieval_range_tile_count: any M >= 1 with ceil(M / 64) <= 65535.  block_counts: the whole table, int32
 *     [M][COOT_RETRIEVAL_RANGE_TABLE_ROW(N)]; it writes the first ceil(N / 128) entries of every row, slot for slot what
 *     coot_retrieval_range_count writes for the same queries in calls of 16.  A workgroup serves 64 queries and a block of 128 rows; a
 *     block in which keep leaves no row is not read.
 *   coot_retrieval_range_scan, unchanged, on the table.
 *   coot_retrieval_range_tile_fill: the count call's arguments again, block_base = the scanned table, offsets = the scan's offsets (all
 *     M + 1; M are read), and rows_out / scores_out with room for `capacity` entries: a hit whose position is below capacity is written,
 *     the others are not, and entries that no hit claims are not touched.  A block in which none of a workgroup's 64 queries has a hit
 *     is not read by that workgroup.
 * s(i, j) is the same fp32 chain as in every other search, so table, offsets, rows and scores are byte for byte those of the three
 * calls above, whichever pass ran on which route; they do not depend on the schedule or on the other queries of the call.  No atomic
 * touches global memory.  gallery_dtype, gallery_norms (NULL: rows used as they are; otherwise the queries' norms are computed into the
 * workspace), keep (NULL: no filter) and thresholds (device fp32 [M]) as above.
 * workspace (16-byte aligned): coot_retrieval_range_tile_workspace_bytes(M, N, d), the query norms; it needs no device and is 256 for
 * arguments out of range.  count reads queries, gallery, gallery_norms, keep, thresholds and writes block_counts and the workspace; fill
 * reads what count reads, block_base and offsets, and writes rows_out, scores_out and the workspace.  A refused call (unknown dtype, a
 * null pointer other than gallery_norms and keep, M outside its range, N or d < 1, capacity < 0, workspace misaligned or too small)
 * returns before any launch and writes nothing.  No allocation, no synchronisation; no pointer is retained. */
size_t coot_retrieval_range_tile_workspace_bytes(int M, int N, int d);
int coot_retrieval_range_tile_count(const float* queries, const void* gallery, int gallery_dtype, const float* gallery_norms, const uint8_t* keep,
                                    const float* thresholds, int M, int N, int d, int32_t* block_counts, void* workspace, size_t workspace_bytes,
                                    coot_stream_t stream);
int coot_retrieval_range_tile_fill(const float* queries, const void* gallery, int gallery_dtype, const float* gallery_norms, const uint8_t* keep,
                                   const float* thresholds, int M, int N, int d, const int32_t* block_base, const int64_t* offsets, int64_t capacity,
                                   int32_t* rows_out, float* scores_out, void* workspace, size_t workspace_bytes, coot_stream_t stream);

/* ---- self-join: all pairs of gallery rows at or above a threshold ------------------------------------------------------------------
 * The tile range search with the gallery on both sides.  Pair (i, j), i < j, is a hit when keep (NULL: no filter) lets BOTH rows pass,
 * groups is NULL or groups[i] != groups[j] (device int32 [N] as in coot_retrieval_topk_scoped, integer compare), and
 * s(i, j) >= thresholds[i], the IEEE fp32 compare of the range search.  s(i, j) is the fp32 chain of every search here with row i as the
 * query: the stored row widened (exact) and gallery_norms[i] as its norm, which is the norm of the widened row — so the bits are those
 * of coot_retrieval_range_tile_count / _fill on a float32 copy of the gallery, and s(i, j) == s(j, i).  Every unordered pair appears
 * once, under its smaller row, rows ascending: the CSR of the range search read as pairs.
 * A call serves the rows [row0, row0 + rows), row0 a multiple of COOT_RETRIEVAL_RANGE_BLOCK, rows >= 1, row0 + rows <= N,
 * ceil(rows / 64) <= 65535.  thresholds: device fp32 [N], indexed by the absolute row.  block_counts: int32
 * [rows][COOT_RETRIEVAL_RANGE_TABLE_ROW(N - row0)], one slot per block at or right of the chunk's first block — the table of a
 * gallery of N - row0 rows:
 *   coot_retrieval_join_count writes the first ceil(N / 128) - row0 / 128 entries of every row; the slots left of the diagonal are
 *     zeros and their blocks are not read, nor is a block in which keep leaves no row.
 *   coot_retrieval_range_scan(block_counts, rows, N - row0, offsets, counts_out, stream), unchanged.
 *   coot_retrieval_join_fill: the count call's arguments again, block_base = the scanned table, offsets = int64 [rows], the position of
 *     the first hit of row row0 + r at offsets[r] (the scan's, or the scan's shifted by what earlier chunks hold), and rows_out /
 *     scores_out with room for `capacity` entries: a hit whose position is below capacity is written, the others are not, and entries
 *     that no hit claims are not touched.  A block in which none of a workgroup's 64 rows has a hit is not read.
 * No workspace: the index's norms serve both sides.  No atomic touches global memory: the bytes do not depend on the schedule or on
 * how the rows are cut into chunks.  A refused call (unknown dtype, a null pointer other than gallery_norms, keep and groups, row0 or
 * rows outside their range, N or d < 1, capacity < 0) returns before any launch and writes nothing.  No allocation, no synchronisation;
 * no pointer is retained. */
int coot_retrieval_join_count(const void* gallery, int gallery_dtype, const float* gallery_norms, const uint8_t* keep, const int32_t* groups,
                              const float* thresholds, int row0, int rows, int N, int d, int32_t* block_counts, coot_stream_t stream);
int coot_retrieval_join_fill(const void* gallery, int gallery_dtype, const float* gallery_norms, const uint8_t* keep, const int32_t* groups,
                             const float* thresholds, int row0, int rows, int N, int d, const int32_t* block_base, const int64_t* offsets,
                             int64_t capacity, int32_t* rows_out, float* scores_out, coot_stream_t stream);

/* ---- join of two galleries: all pairs (left row, right row) at or above a threshold -------------------------------------------------
 * The tile range search with a prepared gallery on either side.  Pair (i, j), row i of left [N_left, d] and row j of right [N_right, d],
 * is a hit when left_keep (NULL: no filter) lets row i pass, right_keep row j, left_groups and right_groups are both NULL or
 * left_groups[i] != right_groups[j] (device int32 [N_left] and [N_right] in one id space, integer compare), and
 * s(i, j) >= thresholds[i], the IEEE fp32 compare of the range search.  s(i, j) is the fp32 chain of every search here with left row i
 * as the query: the stored row widened (exact) and left_norms[i] as its norm, which is the norm of the widened row — so the bits are
 * those of coot_retrieval_range_tile_count / _fill with a float32 copy of left as the queries.  left_dtype and right_dtype are
 * COOT_GALLERY_* codes and need not agree; left_norms and right_norms are both given (both sides divided by their norms) or both NULL.
 * The result is the CSR of the range search: the hits of left row i are rows of right, ascending.
 * A call serves the left rows [row0, row0 + rows), row0 a multiple of 64, rows >= 1, row0 + rows <= N_left, ceil(rows / 64) <= 65535.
 * thresholds: device fp32 [N_left], indexed by the absolute row.  block_counts: int32 [rows][COOT_RETRIEVAL_RANGE_TABLE_ROW(N_right)],
 * the table of `rows` queries against a gallery of N_right rows:
 *   coot_retrieval_cross_join_count writes the first ceil(N_right / 128) entries of every row; a block in which right_keep leaves no
 *     row is not read, nor is anything for 64 left rows that left_keep masks altogether: their slots are zeros.
 *   coot_retrieval_range_scan(block_counts, rows, N_right, offsets, counts_out, stream), unchanged.
 *   coot_retrieval_cross_join_fill: the count call's arguments again, block_base = the scanned table, offsets = int64 [rows], the
 *     position of the first hit of left row row0 + r at offsets[r] (the scan's, or the scan's shifted by what earlier chunks hold), and
 *     rows_out / scores_out with room for `capacity` entries: a hit whose position is below capacity is written, the others are not,
 *     and entries that no hit claims are not touched.  A block in which none of a workgroup's 64 rows has a hit is not read.
 * No workspace.  No atomic touches global memory: the bytes do not depend on the schedule or on how the left rows are cut into chunks.
 * A refused call (unknown dtype, a null pointer other than the norms, keeps and groups, one norm or one groups table without the other,
 * row0 or rows outside their range, N_left, N_right or d < 1, capacity < 0) returns before any launch and writes nothing.  No
 * allocation, no synchronisation; no pointer is retained. */
int coot_retrieval_cross_join_count(const void* left, int left_dtype, const float* left_norms, const void* right, int right_dtype,
                                    const float* right_norms, const uint8_t* left_keep, const uint8_t* right_keep, const int32_t* left_groups,
                                    const int32_t* right_groups, const float* thresholds, int row0, int rows, int N_left, int N_right, int d,
                                    int32_t* block_counts, coot_stream_t stream);
int coot_retrieval_cross_join_fill(const void* left, int left_dtype, const float* left_norms, const void* right, int right_dtype,
                                   const float* right_norms, const uint8_t* left_keep, const uint8_t* right_keep, const int32_t* left_groups,
                                   const int32_t* right_groups, const float* thresholds, int row0, int rows, int N_left, int N_right, int d,
                                   const int32_t* block_base, const int64_t* offsets, int64_t capacity, int32_t* rows_out, float* scores_out,
                                   coot_stream_t stream);

/* ---- K best partners of every row: a prepared gallery against a second one, or against itself ------------------------------------
 * For every row i of left [N_left, d] the K best rows j of right [N_right, d], without a float32 copy of the left side, without a norm
 * pass and in one call for any N_left.  Pair (i, j) is eligible when left_keep (NULL: no filter) lets row i pass, right_keep row j,
 * left_groups and right_groups are both NULL or left_groups[i] != right_groups[j] (device int32 [N_left] and [N_right] in one id space,
 * integer compare), and, with exclude_same_row = 1, j != i (the self case: left and right the same gallery).  Row i of idx_out /
 * score_out (int32 / fp32 [N_left][K]) holds the K best eligible j by the order of every search here, score descending, then the
 * larger row; fewer than K eligible rows leave a tail of idx -1, score -inf, and a left row that left_keep masks is -1 / -inf in all K
 * slots: it does not ask.  s(i, j) is the fp32 chain of every search with left row i as the query: the stored row widened (exact) and
 * left_norms[i] as its norm — bit for bit the sim_out of coot_retrieval_topk_index with a float32 copy of left as the queries.  So an
 * unmasked row is, byte for byte, the row coot_retrieval_topk_scoped returns for that query with exclude = 1 and scope = left_groups[i],
 * and without groups and exclude_same_row the row of coot_retrieval_topk_index under keep = right_keep.
 * left_dtype and right_dtype are COOT_GALLERY_* codes and need not agree; left_norms and right_norms are both given (both sides divided
 * by their norms) or both NULL.  1 <= K <= min(N_right, 128), checked against N_right whatever the filters hold; ceil(N_left / 64) <=
 * 65535.  A workgroup serves 64 left rows and a share of the 128-row blocks of right; a block in which right_keep leaves no row is not
 * read, nor is anything for 64 left rows that left_keep masks altogether.  The right gallery is cut into S shares whose lists are merged
 * by rank (automatic: enough workgroups to fill the device; coot_set_option("rt_knn_splits", n) fixes S for tests, 0 = automatic); the
 * result depends on neither S, the schedule nor the other rows of the call.  No atomic touches global memory.
 * workspace (16-byte aligned): coot_retrieval_knn_join_workspace_bytes(N_left, N_right, K), the lists of the shares under the split
 * option in force when it is asked; it needs no device and is 256 for arguments out of range.  Reads left, right, the norms, keeps and
 * groups; writes idx_out, score_out and the workspace.  A refused call (unknown dtype, a null pointer other than the norms, keeps and
 * groups, one norm or one groups table without the other, exclude_same_row not 0 or 1, N_left, N_right, d or K outside their range,
 * workspace misaligned or too small) returns before any launch and writes nothing.  No allocation, no synchronisation; no pointer is
 * retained. */
size_t coot_retrieval_knn_join_workspace_bytes(int N_left, int N_right, int K);
int coot_retrieval_knn_join(const void* left, int left_dtype, const float* left_norms, const void* right, int right_dtype,
                            const float* right_norms, const uint8_t* left_keep, const uint8_t* right_keep, const int32_t* left_groups,
                            const int32_t* right_groups, int exclude_same_row, int N_left, int N_right, int d, int K, int32_t* idx_out,
                            float* score_out, void* workspace, size_t workspace_bytes, coot_stream_t stream);

/* ---- connected components of the self-join: a cluster label per gallery row, in one sweep -------------------------------------------
 * The edge set is the hit set of coot_retrieval_join_count / _fill over the whole gallery: pair (i, j), i < j, is an edge when keep
 * (NULL: no filter) lets BOTH rows pass, groups is NULL or groups[i] != groups[j] (device int32 [N], integer compare), and
 * s(i, j) >= thresholds[i] (device fp32 [N]), the IEEE fp32 compare and the bits of s of the self-join.  labels[i] (int32 [N]) is the
 * smallest row number in the connected component of row i under those edges: a row without an edge labels itself, a row that keep
 * masks is -1 and is no vertex, so it does not connect its neighbours.  With groups two rows of one group are never joined directly but
 * may share a component through a row of another group.
 * Three launches on the stream: parent[i] = i; the count pass of the self-join over the whole upper triangle (one grid: ceil(N / 64) <=
 * 65535 row tiles; blocks left of the diagonal and blocks in which keep leaves no row are not read), in which every hit is a union in
 * parent instead of a count; labels from parent.  No table, no scan, no fill pass, no pair list: parent (int32 [N], a workspace whose
 * contents before and after the call mean nothing) and labels are all the memory there is.
 * The union-find keeps parent[x] <= x and only ever lowers a value (a root is linked below a smaller root by compare-and-swap, paths
 * are halved by atomic minimum), every loop strictly descends and none waits for another workgroup; the root of a set is its smallest
 * member, so labels is a function of the edge set alone: it depends on neither the schedule, the grid, the storage type nor a rerun.
 * coot_set_option("rt_comp_blocks_per_wg", n) fixes how many 128-row blocks a workgroup walks (tests; 0 = automatic: one, up to 2^20
 * workgroups).  Integer atomics on parent only; no floating-point atomic.
 * Reads gallery, gallery_norms (NULL: rows used as they are), keep, groups and thresholds; writes parent and labels.  A refused call
 * (unknown dtype, a null pointer other than gallery_norms, keep and groups, N or d < 1, ceil(N / 64) > 65535) returns before any launch
 * and writes nothing.  No allocation, no synchronisation; no pointer is retained. */
int coot_retrieval_components(const void* gallery, int gallery_dtype, const float* gallery_norms, const uint8_t* keep, const int32_t* groups,
                              const float* thresholds, int N, int d, int32_t* parent, int32_t* labels, coot_stream_t stream);

/* ---- a prepared gallery that changes: rows written in place, their norms with them ---------------------------------------
 * coot_retrieval_rows_put writes the R rows of src [R, d] into the buffer gallery [N, d] and, where norms != NULL, norms[row] of
 * every row it wrote: what a corpus that grows (rows appended into spare capacity) or is re-encoded (rows overwritten) needs,
 * O(R d) bytes instead of a new gallery.  One launch, no workspace, no allocation, no synchronisation; no pointer is retained.
 *   dest == NULL: source row p goes to gallery row row0 + p; 0 <= row0 and row0 + R <= N.
 *   dest != NULL (device int32 [R]): source row p goes to row dest[p]; a dest[p] outside [0, N) skips that row; row0 has to be 0.
 *   Two positions with the same destination race: which one stays, and whether the row is one of them at all, is unspecified.
 *   src_dtype / gallery_dtype: COOT_GALLERY_F32, _BF16, _F16.  Allowed: fp32 into any of the three, bfloat16 into bfloat16 or fp32,
 *   IEEE half into IEEE half or fp32.  The stored bytes are those of torch's src.to(gallery dtype) for every element that is not a
 *   NaN: fp32 -> 16 bits rounds to nearest even (bfloat16: every NaN becomes 0x7FC0; IEEE half: the hardware conversion, values
 *   above 65 504 become infinities), a 16-bit element widens exactly, the same type is copied bit for bit.  A NaN stays a NaN.
 *   norms[row] has the bits coot_retrieval_row_norms (fp32 gallery) / coot_retrieval_row_norms_h (16-bit) compute on the stored row:
 *   the sum runs over the stored (rounded) values in the same order, not over the fp32 source.  Slots of rows not written stay.
 * src and gallery must not overlap (undefined otherwise).  A refused call (null src or gallery, R, d or N < 1, a type pair that
 * is not allowed, rows outside the buffer, row0 != 0 with dest) returns before any launch and writes nothing. */
int coot_retrieval_rows_put(const void* src, int src_dtype, int R, int d, const int32_t* dest, int row0, void* gallery, int gallery_dtype,
                            int N, float* norms, coot_stream_t stream);

/* ---- labelled retrieval ranking on the device: M queries, N gallery rows, several queries per row -----------------------
 * coot_retrieval_ranks without the assumption "N x N, ground truth on the diagonal": labels[i] (device int32 [M]) is the gallery
 * row of query i.  Several queries may share a row (a second annotation set, several captions per clip), rows may have no query
 * (distractors), and a label outside [0, N), e.g. -1, means "no ground truth": it is never used as an index, the query's rank is -1
 * and it enters neither direction's ranks nor metrics (as a competitor in its columns it still counts).
 *   normalize != 0: every row of both sets is divided by sqrt(sum x^2), no eps, at staging (no normalised copy, as in
 *   coot_retrieval_topk);  s = queries . gallery^T is the fp32 FMA chain of coot_retrieval_ranks and coot_retrieval_topk (k order,
 *   chunks of 32): the optional sim_out [M, N] (testing aid) equals coot_retrieval_topk's bit for bit;
 *   "ahead": (score, index) is ahead of (t, a) when score > t, or score == t and index > a (float comparison: -0 == +0);
 *   ranks_q[i] = #{j != g : (s[i,j], j) ahead of (s[i,g], g)}, g = labels[i] = the position of g in
 *   np.argsort(s[i], kind="stable")[::-1];
 *   ranks_g[j], for a gallery row j that is the label of at least one valid query: let (t, a) = (s[i,j], i) of the query i with
 *   labels[i] == j that is ahead of all others (the best positive); ranks_g[j] = #{i' in [0, M) : (s[i',j], i') ahead of (t, a)} =
 *   the minimum over those queries of their position in np.argsort(s[:, j], kind="stable")[::-1] (the multi-caption protocol:
 *   the best-ranked ground truth counts).  Rows without a valid query: ranks_g[j] = -1;
 *   n_valid [2] = (n_q, n_g): the valid queries and the gallery rows that have one;
 *   metrics (optional, [2, 7]): {r1, r5, r10, r50, medr, meanr, sum} query -> gallery, then gallery -> query, each over its n
 *   entries >= 0 with the arithmetic of coot_retrieval_ranks (r@k = float(count) / float(n), medr = floor(median) + 1 in double,
 *   meanr = float(double(sum) / n + 1), sum = r1 + r5 + r50 in fp32); n == 0: seven zeros.
 * For M == N and labels[i] == i: ranks_q, ranks_g and metrics are coot_retrieval_ranks' ranks_12, ranks_21 and metrics bit for bit.
 * A row or column with a non-finite similarity has unspecified ranks.  M, N, d >= 1.  No M x N array exists unless sim_out is
 * given; every result is an integer function of s (integer atomics only), so it does not depend on the workgroup schedule.
 * workspace (8-byte aligned): coot_retrieval_ranks_labeled_workspace_bytes(M, N, d), exact = (2 M + N) floats, N 64-bit words and
 * (M + N) int32, each rounded up to 256 bytes.  The call retains no pointer and does not synchronise. */
size_t coot_retrieval_ranks_labeled_workspace_bytes(int M, int N, int d);
int coot_retrieval_ranks_labeled(const float* queries, const float* gallery, const int32_t* labels, int M, int N, int d, int normalize,
                                 int32_t* ranks_q, int32_t* ranks_g, int32_t* n_valid, float* metrics, float* sim_out, void* workspace,
                                 size_t workspace_bytes, coot_stream_t stream);

/* ---- labelled ranking under offsets: a number per gallery row and per query is taken off every similarity ----------------------------
 * coot_retrieval_ranks_labeled on the adjusted matrix
 *   a(i, j) = s(i, j)                       neither offset given
 *   a(i, j) = s(i, j) - col[j]              col_offset given (device fp32 [N])
 *   a(i, j) = (s(i, j) - col[j]) - row[i]   both given (row_offset: device fp32 [M]; alone: s(i, j) - row[i])
 * s is bit for bit the sim_out of coot_retrieval_ranks_labeled, and sim_out here holds the same raw s; each subtraction is one IEEE
 * fp32 subtraction after the chain, the column's first.  ranks_q, ranks_g, n_valid and metrics are those of
 * coot_retrieval_ranks_labeled with a in the place of s: the same tie rule, labels outside [0, N) without ground truth, several queries
 * per row, rows without a query, the best-ranked ground truth per gallery row.  col_offset is the offset of
 * coot_retrieval_topk_adjusted: with it alone, ranks_q[i] < K holds exactly when labels[i] is among the K rows that search returns for
 * query i, at that position.  An offset of +inf leaves a = -inf: a column at +inf is still a column and still a valid label; a NaN in
 * a (inf - inf) has unspecified ranks.  Without offsets, and with zeros, every output is coot_retrieval_ranks_labeled's, byte for byte.
 * A hubness correction in both directions (CSLS) is col = coot_retrieval_hub_offsets of the gallery against the queries and row = the
 * same of the queries against the gallery.  Gallery and queries are fp32; normalize, M, N, d and the refusals as in
 * coot_retrieval_ranks_labeled (null pointer other than the offsets, metrics and sim_out; ceil(M / 64) > 65 535; workspace misaligned
 * or too small), before any launch: a refused call writes nothing.  Integer atomics only: nothing depends on the workgroup schedule.
 * workspace (8-byte aligned): coot_retrieval_ranks_adjusted_workspace_bytes(M, N, d), exact, the layout of
 * coot_retrieval_ranks_labeled.  The call retains no pointer and does not synchronise. */
size_t coot_retrieval_ranks_adjusted_workspace_bytes(int M, int N, int d);
int coot_retrieval_ranks_adjusted(const float* queries, const float* gallery, const int32_t* labels, const float* row_offset, const float* col_offset,
                                  int M, int N, int d, int normalize, int32_t* ranks_q, int32_t* ranks_g, int32_t* n_valid, float* metrics,
                                  float* sim_out, void* workspace, size_t workspace_bytes, coot_stream_t stream);

/* ---- the whole training step as native code (coot/trainer_retrieval.py:253-291) -------------------------------
 * Networks are indexed 0 = net_video_local, 1 = net_video_global, 2 = net_text_local, 3 = net_text_global
 * (coot/configs_retrieval.py:182-189).  All buffers are caller-owned device memory. */
typedef struct coot_step_config {
  coot_net_config net[4];
  coot_contrastive_config contr;
  float cc_weight;                               /* train.loss_cycle_cons                                    */
  float lr, beta1, beta2, eps, weight_decay;     /* optimizer as built by nntrainer/optimization.py:45-74     */
  int optimizer;                                 /* 0 = torch.optim.Adam, 1 = the in-file RAdam (:79-181)     */
  int radam_degentosgd;                          /* RAdam degenerated_to_sgd (optimizer.radam_degentosgd)     */
} coot_step_config;
typedef struct coot_step_dims {
  int B, Nc, Lv, Lc, Lp, Ls, Cmax_clip, Cmax_sent;
  int tok_vis, tok_txt;   /* packed rows (coot_packed_seqs): valid frames of the B videos + Nc clips, valid words of the B paragraphs +
                             Nc sentences (host values; 0 = padded layout); used with coot_step_batch.cu_vis / cu_txt */
  int source;             /* COOT_SOURCE_*: PADDED = the four padded fp32 tensors of the reference's batch; PACKED_F32 / PACKED_BF16 =
                             coot_step_batch.vid_feat / par_feat point at the packed matrices [tok_vis, Dv] / [tok_txt, Dt] of
                             coot_collate_packed (videos then clips, paragraphs then sentences), clip_feat / sent_feat are unused */
} coot_step_dims;
typedef struct coot_step_buffers {
  float* params[4]; float* grads[4]; void* wpack[4];       /* flat arenas (coot_net_param_info layout), bf16 pack */
  float* adam_m[4]; float* adam_v[4];                      /* Adam moments, same layout                            */
  const float* decay_mask[4];                              /* 1.0 / 0.0 per element (decay_mult), or NULL = all 1  */
  const float* pe[4];                                      /* embedding.pe tables                                  */
  const uint8_t* decay_block_all[4];                       /* optional, one byte per 1 024 consecutive elements of the arena
                                                              (the last block may be partial): non-zero = decay_mask is 1.0 on
                                                              the whole block — the update then does not read the mask there
                                                              (the mask is 0 on the bias vectors only: > 99 % of the blocks;
                                                              30 MB of the step's HBM reads).  NULL = read the mask everywhere */
} coot_step_buffers;
typedef struct coot_step_batch {                           /* RetrievalDataBatchTuple (coot/dataset_retrieval.py:64-102) */
  const float *vid_feat, *clip_feat, *par_feat, *sent_feat;
  const int64_t *vid_len, *clip_len, *par_len, *sent_len, *clip_num, *sent_num;
  const int32_t *cu_vis, *cu_txt;  /* optional packed row starts [B + Nc + 1]: the B videos (paragraphs) first, then the Nc clips
                                      (sentences); NULL = padded layout */
} coot_step_batch;
size_t coot_step_workspace_bytes(const coot_step_config* cfg, const coot_step_dims* dims);
/* One optimisation step in one call: grads zeroed, both sides encoded on side_v / side_t, contrastive +
 * cycle-consistency losses (cycle indices drawn on the device), backward, Adam (`step` is the 1-based step count for the
 * bias correction).  losses[3] = {total, contrastive, cycle-consistency} (device, overwritten).
 * do_optimizer: bit mask of COOT_STEP_*.  side_v may be the same stream as main_s (recommended: the heavier video side then
 * runs without any cross-stream hop); side_t must differ from side_v.  On return main_s is ordered after both sides.
 * The call also uses one internal stream of the calling thread (created on first use): for the next batch's input LayerNorm
 * (COOT_STEP_INPUT_STAGES) and for the update of the GLOBAL networks, which starts behind their backward and runs next to the local
 * backward (sides whose local network has >= 8192 rows; not in deterministic mode, not in a captured step); side_v / side_t are
 * ordered after it before the call's last launches, so the ordering guarantees above hold unchanged. */
#define COOT_STEP_OPTIMIZER 1   /* Adam update of all four networks                                                          */
#define COOT_STEP_REPACK 2      /* rebuild the bf16 weight packs right after the update (off the next step's critical path)  */
#define COOT_STEP_PACKS_FRESH 4 /* wpack[] is current (previous step ran with REPACK and nothing else touched the parameters):
                                   skip the packing at the start of the step                                                */
#define COOT_STEP_INPUT_STAGES 16 /* x^ of the input LayerNorm lives in the caller's input stages (coot_step_set_input_stages below)      */
#define COOT_STEP_STAGE_ANNOUNCED 32 /* the caller asserts that `batch` IS the batch it announced with coot_step_set_next_batch and that its
                                   contents have not changed since: only then may the step use the x^ a previous step prepared.  Without the
                                   bit a prepared stage is never used, whatever the pointers say (a loader that refills a fixed-shape arena
                                   in place presents the SAME pointers and dims with other data)                              */
#define COOT_STEP_DEFER_TEXT_JOIN 8 /* on return main_s is ordered after the VIDEO side only: the text side's tail (its Adam update,
                                   weight packs) is still running on side_t; the three loss words are final on main_s.  The next coot_train_step with the
                                   same streams needs no join (its text side continues on side_t in order, its video side touches
                                   nothing the text tail writes): back-to-back steps overlap that tail (~30 us) with the next
                                   forward.  Before anything else reads the text networks' parameters / packs from another
                                   stream, the CALLER orders that stream after side_t.  COOT_STEP_TEXT_AHEAD (below) lets that
                                   next step start its text side without waiting for main_s at all.                        */
#define COOT_STEP_TEXT_AHEAD 64 /* back-to-back steps: the caller vouches that nothing it enqueued on main_s since the previous
                                   coot_train_step on these streams is needed by the text side, and that this previous step ended with
                                   COOT_STEP_DEFER_TEXT_JOIN and has not been joined since.  The text side of this step is then ordered
                                   after side_t's own tail and the input stage's event, NOT after main_s at entry: with side_v == main_s
                                   its forward no longer waits for the video side's update tail of the previous step.  Taken only when
                                   the step runs on a prepared input stage (COOT_STEP_INPUT_STAGES + COOT_STEP_STAGE_ANNOUNCED, a hit)
                                   with COOT_STEP_PACKS_FRESH, side_t is the stream this thread's previous coot_train_step deferred
                                   its join on, main_s is not being captured, and no loss scaler, gradient-clip block or injected cycle
                                   indices are registered (the caller prepares those on main_s); in every other case the bit changes
                                   nothing.  coot_set_option("text_ahead", 0) ignores it; coot_get_option("text_ahead_steps") counts
                                   the steps of this thread that took it.  Same results either way.                        */
int coot_train_step(const coot_step_config* cfg, const coot_step_buffers* bufs, const coot_step_batch* batch,
                    const coot_step_dims* dims, float* losses, void* workspace, size_t workspace_bytes, int train,
                    uint64_t seed, int64_t step, int do_optimizer, coot_stream_t main_stream, coot_stream_t side_v,
                    coot_stream_t side_t);
/* The same step split in phases, for data parallel training where torch.distributed collectives (all-gather of the
 * embeddings, all-reduce of the gradients) sit between them.  local_* = [B + Nc, D] (context rows first, then
 * clip / sentence embeddings), glob_* = [B, 2D], resh_* = [B, Cmax, D] (packed + zero padded). */
#define COOT_FWD_PACKS_FRESH 1
#define COOT_FWD_INPUT_STAGES 2
#define COOT_FWD_STAGE_ANNOUNCED 4   /* as COOT_STEP_STAGE_ANNOUNCED */
int coot_step_forward(const coot_step_config* cfg, const coot_step_buffers* bufs, const coot_step_batch* batch,
                      const coot_step_dims* dims, float* local_v, float* local_t, float* glob_v, float* glob_t,
                      float* resh_v, float* resh_t, void* workspace, size_t workspace_bytes, int train, uint64_t seed,
                      int packs_fresh /* bit mask: COOT_FWD_PACKS_FRESH = the bf16 weight packs are current (coot_step_update repacked
                                         them): skip the packing; COOT_FWD_INPUT_STAGES = as COOT_STEP_INPUT_STAGES of coot_train_step (the
                                         following coot_step_backward of this thread reads x^ in the same stage) */,
                      coot_stream_t main_stream, coot_stream_t side_v, coot_stream_t side_t);
int coot_step_backward(const coot_step_config* cfg, const coot_step_buffers* bufs, const coot_step_batch* batch,
                       const coot_step_dims* dims, const float* local_v, const float* local_t, const float* resh_v,
                       const float* resh_t, float* d_local_v, float* d_local_t, const float* d_glob_v,
                       const float* d_glob_t, const float* d_resh_v, const float* d_resh_t, void* workspace,
                       size_t workspace_bytes, int train, uint64_t seed, coot_stream_t main_stream, coot_stream_t side_v,
                       coot_stream_t side_t);
/* Replayable step (hipGraph): with a device state block set (coot_step_device_state_bytes() bytes: { uint64 seed; uint64
 * step; float lr; int pad; 32 bytes of optimizer scalars }), coot_train_step reads its per-step scalars from DEVICE memory — its
 * first node advances them (step += 1, seed += 7919, optimizer scalars from step and lr) exactly as the host does between two
 * eager steps; the seed argument becomes a salt (pass 0), the step argument is ignored.  The call can then be captured once
 * (hipStreamBeginCapture on `main`, side_v == main) and replayed: dependent launches cost 1.7 us in a replay against 3.1 us
 * launched one by one (tools/micro/launchgap.hip).  The host initialises seed / step / lr before the first step and rewrites
 * lr when the schedule changes it.  NULL returns to argument-driven steps.  Thread-local. */
size_t coot_step_device_state_bytes(void);
int coot_step_set_device_state(void* state);
/* Dynamic loss scaling (torch.cuda.amp.GradScaler semantics, decided on the device: no host synchronisation per step).  Opt-in: with
 * no block set (the default) nothing below happens and every call computes what it always did.  The block is caller-owned DEVICE
 * memory of coot_step_loss_scaler_bytes() bytes (80), laid out as
 *   { float scale; int32 growth_tracker; int32 found_inf; int32 skipped; float growth_factor; float backoff_factor;
 *     int32 growth_interval; int32 work (0); int64 step; int32 pad[2]; 32 bytes of optimizer scalars (written by the library) }
 * The caller initialises it (scale = 65536, growth_factor = 2, backoff_factor = 0.5, growth_interval = 2000 are GradScaler's defaults;
 * growth_factor = backoff_factor = 1 hold a fixed scale; step = optimizer steps already taken, the rest 0).  While it is set:
 *   - the loss-gradient launches (coot_contrastive_fwd_bwd*, coot_cyclecons_fwd_bwd, and those inside coot_train_step) multiply the
 *     gradients they seed by `scale` (read on the device at run time); the loss words stay unscaled.  The backward is linear in the seed,
 *     so every 16-bit activation gradient is scaled — what lets the IEEE-half build train: its coot_train_step / coot_step_backward run
 *     only with a block set (coot_net_bwd, the per-op route, still refuses there);
 *   - behind the backward, one check launch unscales the four gradient arenas in place (gradient * 1 / scale, as GradScaler.unscale_;
 *     deterministic mode: after folding their fixed-point sums) and sets found_inf = 1 if any word is NaN or Inf.  On an optimizer step
 *     a one-thread launch then applies torch._amp_update_scale_: found_inf -> scale *= backoff_factor, growth_tracker = 0, skipped += 1;
 *     else growth_tracker += 1 and at growth_interval scale *= growth_factor (if finite), growth_tracker = 0; a finite step also does
 *     step += 1 and derives the optimizer scalars from it (the `step` arguments and the device state block's step are then NOT used
 *     for the update; lr still comes from cfg or the device state block).  With found_inf set the update launches change no parameter
 *     or moment word — the step is skipped, its loss words are still written;
 *   - coot_train_step updates the four networks together behind the check (no early update of the global networks); coot_step_update
 *     runs the check itself on main_stream first (main_stream must be ordered behind every gradient word, e.g. behind the all-reduce)
 *     and refuses COOT_UPDATE_GLOBAL_ONLY / COOT_UPDATE_SKIP_GLOBAL; coot_train_step without COOT_STEP_OPTIMIZER and
 *     coot_step_unscale_grads (a data-parallel step without an update) unscale and set found_inf but leave scale, growth_tracker,
 *     skipped and step alone.
 * What the caller may read: behind the step in stream order (main_stream after coot_train_step / coot_step_update / coot_step_unscale_grads)
 * the gradient arenas hold UNSCALED gradients and found_inf, scale, growth_tracker, skipped and step are final for that step. */
size_t coot_step_loss_scaler_bytes(void);
int coot_step_set_loss_scaler(void* block);
int coot_step_unscale_grads(const coot_step_config* cfg, const coot_step_buffers* bufs, coot_stream_t stream);
/* Gradient norm and clipping (torch.nn.utils.clip_grad_norm_ over all parameters of the four networks, computed on the device: no
 * host synchronisation per step).  Opt-in: with no block set (the default) nothing below is launched and every call computes what
 * it always did.  The block is caller-owned DEVICE memory of coot_step_grad_clip_bytes(cfg) bytes: a 32-byte header, one fp64
 * partial per workgroup of the update's grid over the four arenas (one per 1 024 parameter words) and one ticket per 64 partials,
 * each on a 128-byte line of its own:
 *   { float max_norm; int32 mode; float norm; float coef; int32 clipped; uint32 ticket (0); int32 capacity; int32 pad;
 *     double partials[capacity]; uint32 group_tickets[(capacity + 63) / 64][32] (0) }
 * The caller initialises max_norm (>= 0; a device word: it may be rewritten between steps, also under graph replay), capacity = the
 * largest n with 32 + 8 n + 128 ceil(n / 64) <= coot_step_grad_clip_bytes(cfg), and the rest to 0 (the tickets are 0 again after
 * every launch).  Each norm launch writes norm = ||every gradient word||_2 (summed in
 * fp64 in a fixed order: the same bits for the same gradients, whatever the workgroup schedule), coef = min(max_norm / (norm +
 * 1e-6), 1) (a NaN norm gives a NaN coef, as torch's clamp does), mode = the registration's `before_update`, and clipped += 1 when
 * coef < 1.  A block with a capacity below the grid gets norm = NaN.
 * coot_step_set_grad_clip(block, before_update):
 *   before_update = 0, report only (what the reference does: it clips after optimizer.step(), so its clipping moves no parameter):
 *     the norm of the step's final gradients is taken behind the update, one launch per side on that side's stream (no early update
 *     is given up, the deferred text join stays); parameters, moments, loss words and gradient arenas are bit-identical to a step
 *     without a block;
 *   before_update = 1, clip before the update: the norm is taken in front of the update and the update reads every gradient word
 *     times coef (the arenas keep the unclipped words).  coot_train_step updates the four networks together behind the norm (no early
 *     update of the global networks); coot_step_update takes the norm on main_stream first (main_stream must be ordered behind every
 *     gradient word) and refuses COOT_UPDATE_GLOBAL_ONLY / COOT_UPDATE_SKIP_GLOBAL.
 *   With a loss scaler set the sum of squares of the UNSCALED words rides on its check launch (no launch of its own; the order is
 *   torch's AMP recipe: unscale -> clip -> step -> update); a non-finite gradient skips the step, norm is then not finite.
 * coot_step_grad_norm: the norm and coef of the arenas as they are (deterministic mode: after folding their fixed-point sums), no
 * update — e.g. a data-parallel step without one.  norm / coef / clipped are final behind the step in stream order: main_stream
 * after coot_train_step / coot_step_update, after the text stream's join too where that is deferred. */
size_t coot_step_grad_clip_bytes(const coot_step_config* cfg);
int coot_step_set_grad_clip(void* block, int before_update);
int coot_step_grad_norm(const coot_step_config* cfg, const coot_step_buffers* bufs, coot_stream_t stream);
/* Data parallel: hipEvent_t handles (or NULL) that coot_step_backward records on the video / text stream as soon as that side's
 * GLOBAL network backward is enqueued — its parameter gradients (networks 1 and 3) are final from there on, so a communication
 * stream can wait on the events and reduce them while the local backward (two thirds of the pass) still runs.  Thread-local,
 * stays set until changed. */
int coot_step_set_global_done_events(void* ev_video, void* ev_text);
/* Stream ordering without system-scope fences.  A default HIP event (what hipEventCreate, torch.cuda.Event and torch's wait_stream
 * use) performs a system-scope release at every record: an L2 writeback / invalidation that makes device memory visible to the host and
 * other devices — and evicts what the step's latency-bound kernels keep in L2.  Ordering two streams of ONE device needs none of it.
 * The library owns COOT_SYNC_EVENTS events created with hipEventDisableTiming | hipEventDisableSystemFence: coot_event_record /
 * coot_event_wait (slot 0 .. COOT_SYNC_EVENTS - 1; coot_event_handle returns the hipEvent_t, e.g. for
 * coot_step_set_global_done_events), coot_stream_hop = everything enqueued on `to` afterwards runs behind everything enqueued on `from`
 * before (internal event ring).  Thread-local, like the streams' owner. */
/* Streams that really run CONCURRENTLY.  HIP multiplexes a process's streams onto a few hardware queues (GPU_MAX_HW_QUEUES, 4 by
 * default) in the order they are created; two streams that land on one queue run their kernels one after the other whatever the
 * events between them say — with the step's video and text side on one queue the ActivityNet step costs 1.72 instead of 1.22 ms, and
 * one more stream created anywhere in the process before the trainer's is enough to get there (profiles/r06_stream_queues.txt).
 * coot_stream_create_concurrent creates (non-blocking) candidate streams until one's kernels overlap those of every stream in
 * others[0 .. n_others) (n_others <= 8; NULL entries = the null stream): a 100-us spin kernel on both must finish in the time of one.
 * It also keeps clear of the library's own stream (next batch's input LayerNorm, early update) when the queues allow it.
 * priority: 0 normal, > 0 the device's lowest, < 0 its highest.  *concurrent (may be NULL) = 1 if such a stream was found within 32
 * candidates, else 0 with the last candidate returned and a line on stderr (GPU_MAX_HW_QUEUES=1, a tool that serialises the
 * queues).  Release with coot_stream_destroy (synchronises the stream).  coot_streams_overlap(a, b): the test itself — 1 kernels overlap,
 * 0 they run one after the other, < 0 error.  All three SYNCHRONISE THE DEVICE: setup calls, not step calls.   Thread-local bookkeeping.  The library verifies its own stream the same way against (side_v, side_t) at the head of the
 * first coot_train_step / coot_step_forward that brings a new pair (one device synchronisation; never under capture).
 * coot_get_option: stream_overlap_tests / stream_candidates_rejected / stream_unresolved. */
int coot_stream_create_concurrent(const coot_stream_t* others, int n_others, int priority, coot_stream_t* out, int* concurrent);
int coot_stream_destroy(coot_stream_t stream);
int coot_streams_overlap(coot_stream_t a, coot_stream_t b);
#define COOT_SYNC_EVENTS 8
int coot_event_record(int slot, coot_stream_t stream);
int coot_event_wait(int slot, coot_stream_t stream);
void* coot_event_handle(int slot);
int coot_stream_hop(coot_stream_t from, coot_stream_t to);
/* Optimizer update of the four networks after the gradient all-reduce (cfg->optimizer; `step` 1-based): one launch per side on
 * side_v / side_t.  repack: bit mask — COOT_UPDATE_REPACK: the bf16 weight packs are rebuilt so that the next coot_step_forward may skip
 * the packing; COOT_UPDATE_DEFER_TEXT_JOIN: on return main_s is ordered after the VIDEO side only (as COOT_STEP_DEFER_TEXT_JOIN: the
 * text side's update tail overlaps the next step's forward; the caller orders whatever else touches the text networks or the gradient
 * arenas after side_t).
 * losses (may be NULL): the three loss words { total, contrastive, cycle-consistency } of the step; the video side's update launch
 * writes total = contrastive + cycle-consistency (a data-parallel caller keeps the two all-reduced words there: no extra launch). */
#define COOT_UPDATE_REPACK 1
#define COOT_UPDATE_DEFER_TEXT_JOIN 2
#define COOT_UPDATE_SKIP_GLOBAL 4  /* the two global networks are left alone: a COOT_UPDATE_GLOBAL_ONLY call of the same step updated them */
#define COOT_UPDATE_GLOBAL_ONLY 8  /* update (and repack) the two GLOBAL networks only, on main_s alone (side_v / side_t unused, losses untouched):
                                      their gradients are final behind the global backward (data parallel: behind their all-reduce bucket), a whole
                                      local backward before the step's end — as coot_train_step's early update of the global networks         */
int coot_step_update(const coot_step_config* cfg, const coot_step_buffers* bufs, int64_t step, int repack, float* losses,
                     coot_stream_t main_stream, coot_stream_t side_v, coot_stream_t side_t);
/* One valid clip / sentence position per video for the cycle-consistency loss (th.multinomial(mask, 1), coot/loss_fn.py:306-314),
 * drawn on the device: idx[0 .. B) from clip_num, idx[B .. 2B) from sent_num. */
int coot_sample_cycle_indices(const int64_t* clip_num, const int64_t* sent_num, int B, uint64_t seed, int64_t* idx,
                              coot_stream_t stream);
/* Injects the draw instead: idx[0 .. B) clip positions, idx[B .. 2B) sentence positions (device memory, read at every
 * coot_train_step / phase 4 until reset with NULL).  For reproducing a given th.multinomial sequence of the reference
 * (coot/loss_fn.py:306-314 consumes the global torch RNG, which no device kernel can replay).  Thread-local. */
int coot_step_set_cycle_indices(const int64_t* idx);
/* Software-pipelined input LayerNorm (COOT_STEP_INPUT_STAGES).  The input LayerNorm of the local networks
 * (nntrainer/models/transformer_legacy.py:224-239, norm_input) has no parameters of its own here — its gain / bias are folded into the
 * packed input-FC weights — so the normalised features x^ of batch t + 1 depend on nothing step t computes.  With two caller-owned
 * device buffers ("stages", each >= coot_step_input_stage_bytes() of the largest batch) a coot_train_step that carries the flag
 *   - keeps this batch's x^ in one stage (normalising it first unless the previous step already did), and
 *   - if a next batch was announced (coot_step_set_next_batch, one-shot: consumed by that step), normalises THAT batch into the
 *     other stage on an internal stream behind both sides' local forward passes — where the step runs its global networks and losses
 *     on a handful of CUs and the memory system is idle; the next coot_train_step on that batch (same pointers and dims) finds x^
 *     ready and starts with the input FC — provided the caller says so (COOT_STEP_STAGE_ANNOUNCED): equal pointers and dims alone do
 *     not identify a batch (arena slots are refilled in place), so without the bit the step normalises itself, after waiting for the
 *     internal stream's last launch (whose reads of the announced batch are then ordered before anything the caller enqueues next).
 * Every step still executes exactly one input LayerNorm per side (for the following batch); what a data loader's lookahead buys is
 * that it runs off the critical path.  Results are bit-identical to a step without stages.  The state (which stage holds what) is
 * thread-local and reset when the stage pointers change; steps without the flag never touch it.  Not available under graph capture. */
size_t coot_step_input_stage_bytes(const coot_step_config* cfg, const coot_step_dims* dims);
int coot_step_set_input_stages(void* stage0, void* stage1, size_t bytes_each);
int coot_step_set_next_batch(const coot_step_batch* next, const coot_step_dims* next_dims);
/* Deterministic mode (the reference tests run-to-run determinism: tests_nntrainer/integration_deter.py:18-66).  Everything in the
 * library is computed in a fixed order except the fp32 atomicAdds by which several workgroups add into one word (bias / LayerNorm
 * parameter gradients of a few kernels, the cycle-consistency loss word): their arrival order moves the last bits of a gradient, and
 * Adam amplifies last bits into different trajectories.  coot_det_configure registers up to 8 fp32 ranges (the gradient arenas, the
 * loss words) and a caller-owned shadow (coot_det_shadow_bytes) of 64-bit fixed-point accumulators: while it is set, every such add
 * into a registered range goes to the shadow as an INTEGER atomic (order independent) and coot_det_flush — called by coot_train_step /
 * coot_step_backward for the arenas and loss words they were given, by the caller for anything else — adds the sums into the fp32
 * words and clears the shadow.  With it two runs of the same steps are bit-identical.  n = 0 switches the mode off.  PROCESS-GLOBAL
 * (like the option switches); configure synchronises the device. */
size_t coot_det_shadow_bytes(int n, const size_t* bytes);
int coot_det_configure(int n, void* const* bases, const size_t* bytes, void* shadow, size_t shadow_bytes, coot_stream_t stream);
int coot_det_flush(const void* base, size_t bytes, coot_stream_t stream);
int coot_adam_step(float* params, const float* grads, float* m, float* v, const float* decay_mask, int64_t n, float lr,
                   float beta1, float beta2, float eps, float weight_decay, int64_t step, coot_stream_t stream);
/* RAdam of nntrainer/optimization.py:79-181 on one flat arena: decoupled decay weight_decay * decay_mask,
 * rectified update when N_sma >= 5, otherwise SGD-with-momentum (degenerated_to_sgd) or no parameter update. */
int coot_radam_step(float* params, const float* grads, float* m, float* v, const float* decay_mask, int64_t n, float lr,
                    float beta1, float beta2, float eps, float weight_decay, int64_t step, int degenerated_to_sgd,
                    coot_stream_t stream);

/* ---- kernel-level entry points (unit tests / microbenchmarks) ---------------------------------- */
/* C[M,N] (bf16 or fp32) = act(X[M,K] . W[N,K]^T + bias) (+ residual)   (bf16 operands as uint16) */
int coot_gemm_nt(const void* X, int64_t ldx, const void* W, int64_t ldw, int M, int N, int K, const float* bias,
                 int act, const void* residual_bf16, int64_t ldres, void* out, int64_t ldc, int out_f32,
                 coot_stream_t stream);
/* The whole gemm_nt descriptor the networks use (tests): every launch variant, grouped launches and the full fused epilogue.
 * Per element, in this order: v = acc + bias; v *= dropout scale (act 0/1); save_pre = bf16(v); act 1: v = gelu(v);
 * v += pe[pos][col] (pos = row % pe_L for rows < pe_T0, else (row - pe_T0) % pe_L2; pe has N columns); v += res;
 * act 2: v *= gelu'(aux) * dropout scale; out = v; colsum[col] += v.  Group z (blockIdx.z) reads X + z*zX, W + z*zW and
 * addresses bias / aux / save_pre / res / colsum / out at column z*zOut + col.  Dropout (p > 0): the mask of (seed, site) at
 * element index row*drop_ld + z*zOut + col, p quantised as coot_debug_dropout_scales does.  part_ws (optional, device fp32,
 * ceil(M/64) * max(N, groups*zOut) floats): the column sums of the M > 512 kernels go through per-row-block partials and one
 * reduction, as inside a network call; without it they are added with atomics.  M, ld*, z* in elements; N, K, ld*, z* % 8 == 0. */
typedef struct coot_gemm_nt_args {
  const void* X; int64_t ldx;   /* bf16 [M, K] */
  const void* W; int64_t ldw;   /* bf16 [N, K] */
  int M, N, K;
  int groups; int64_t zX, zW, zOut;
  const float* bias;            /* fp32 [groups*zOut] or NULL */
  int act;                      /* 0 none | 1 gelu | 2 multiply by gelu'(aux) */
  const void* aux; int64_t ldaux;
  void* save_pre; int64_t ldpre;
  const void* res; int64_t ldres;
  const float* pe; int pe_L, pe_T0, pe_L2;
  float* colsum;
  float p; uint64_t seed; unsigned site; int64_t drop_ld;
  void* out; int64_t ldc; int out_f32;
  float* part_ws; size_t part_ws_floats;
} coot_gemm_nt_args;
int coot_debug_gemm_nt(const coot_gemm_nt_args* a, coot_stream_t stream);
/* C[Mo,No] fp32 += sum_t A[t,Mo] * B[t,No].  workspace (coot_gemm_tn_workspace_bytes) selects the two-pass
 * split reduction; NULL falls back to fp32 atomics. */
size_t coot_gemm_tn_workspace_bytes(int T, int Mo, int No);
int coot_gemm_tn(const void* A, int64_t lda, const void* B, int64_t ldb, int T, int Mo, int No, float* C,
                 int64_t ldc, void* workspace, size_t workspace_bytes, coot_stream_t stream);
/* n weight-gradient problems C_i[Mo_i,No_i] (+)= A_i^T . B_i in ONE launch (+ one split reduction) — the way a network's
 * backward pass issues them (coot_net_bwd); a_colsum (optional) += column sums of A_i (the bias gradient).  workspace: fp32
 * partial tiles, sum_i splits_i * Mo_i * No_i * 4 bytes with splits_i <= 8 (too small: the problems run one by one).
 * stamps (optional, (64 + 2 x workgroups) x uint64 on the device): phase times of tile (0,0) of problem 0 in shader clocks. */
typedef struct coot_tn_problem {
  const void* A; int64_t lda;   /* bf16 [T, Mo] */
  const void* B; int64_t ldb;   /* bf16 [T, No] */
  int T, Mo, No;
  float* C; int64_t ldc;        /* fp32 [Mo, No] */
  float* a_colsum;              /* fp32 [Mo] or NULL (groups == 1) */
  int overwrite;                /* 1: C = ..., 0: C += ... */
  int groups;                   /* >= 1: batch of problems, group z at A + z*zA, B + z*zB, C + z*zC (elements) */
  int64_t zA, zB, zC;
} coot_tn_problem;
int coot_gemm_tn_batch(const coot_tn_problem* problems, int n, void* workspace, size_t workspace_bytes,
                       uint64_t* stamps, coot_stream_t stream);
/* host-only: the workgroup -> (problem, tile) table of such a launch (tiles of one problem, split and group on one XCD: block b
 * runs on XCD b % 8) for n problems with gx x gy tiles, `groups` groups and `splits` splits each; out_item / out_local
 * [max_blocks] (-1 = empty slot); returns the grid size (0: the launch does not fit the table, linear order is used) */
int coot_debug_tn_xcd_map(int n, const int* gx, const int* gy, const int* groups, const int* splits, int* out_item,
                          int* out_local, int max_blocks);
/* one wave writes n pairs (100 MHz real-time counter, shader clock counter), one every interval_ticks real-time ticks:
 * run it on a side stream to see the shader clock the device delivers under the step's load (tools/clock_probe.py) */
int coot_debug_clock_monitor(uint64_t* out, int n, int interval_ticks, coot_stream_t stream);
int coot_ln_fwd(const float* x, int R, int D, const float* gain, const float* bias, void* y_bf16, float* y_f32,
                coot_stream_t stream);
int coot_attn_fwd(const void* qkv, int Nseq, int L, int H, int dh, const int64_t* lens, void* out, float* lse,
                  coot_stream_t stream);
/* The whole attention descriptor the networks use (tests): launch_attn_fwd (backward == 0) or launch_attn_bwd on it, so every
 * dispatch path can be called alone: the one-query kernels (Lq == 1, Lk <= 64, one segment), the short kernels (Lq == Lk <= 128:
 * optionally a second segment of Nseq2 sequences of length L2 whose rows start at row Nseq * Lk of every matrix, or packed rows:
 * sequence n of both segments starts at row cu[n] and has lens[n] resp. lens2[n - Nseq] rows) and the chunked kernels (anything
 * else, one segment).  Head h is columns [h dh, (h + 1) dh) of q, k, v, o, dout, dq, dk, dv; lse and delta are [rows, H] fp32.
 * scale = 1 / sqrt(dh).  Keys >= lens[n] are filled with -32752 before the softmax over all Lk keys and pass no gradient; all Lq
 * query rows are computed.  Dropout (p > 0) multiplies the probabilities by the mask of (seed, site) at mask row
 * (n H + h) Lq + query, p quantised as coot_debug_attn_dropout_scales does; n counts within the segment, the second segment
 * draws from seed + 0x9E3779B97F4A7C15, and a packed sequence uses its own length as Lq and Lk.  The backward reads o and lse
 * (the forward's outputs), writes dq, dk, dv and uses delta as scratch.  Strides in elements, multiples of 8, base pointers
 * 16-byte aligned.  lens[n] >= 1 is the caller's business (lens lives on the device): with every key filled the forward is
 * uniform over Lk as in the reference, but the backward's dV is zero where the reference's is not.  coot_collate_level and
 * coot_collate_packed do accept a sequence of 0 rows; the reference's dataset expands every segment to a minimum of frames. */
typedef struct coot_attn_args {
  const void* q; int64_t ldq;   /* bf16 [Nseq * Lq (+ Nseq2 * L2), >= H dh] */
  const void* k; int64_t ldk;   /* bf16 [Nseq * Lk (+ Nseq2 * L2), >= H dh] */
  const void* v; int64_t ldv;
  void* o; int64_t ldo;         /* forward: output; backward: the saved output */
  float* lse;                   /* fp32 [rows of q, H] */
  const int64_t* lens;          /* [Nseq] valid keys */
  int Nseq, Lq, Lk, H, dh;
  int Nseq2, L2; const int64_t* lens2;
  const int* cu;                /* packed rows: int32 [Nseq + Nseq2] first rows, or NULL */
  const void* dout; int64_t lddo;
  float* delta;                 /* fp32 [rows of q, H] scratch */
  void* dq; int64_t lddq;
  void* dk; int64_t lddk;
  void* dv; int64_t lddv;
  float p; uint64_t seed; unsigned site;
} coot_attn_args;
int coot_debug_attn(const coot_attn_args* a, int backward, coot_stream_t stream);
/* The whole LayerNorm descriptors the networks use (tests): launch_ln_fwd (backward == 0) or launch_ln_bwd on them.
 * y = gain (x - mean) / (std_unbiased + 1e-6) + bias (gain NULL: no affine), + pe[(row % pe_L) D + col], times the dropout mask of
 * (seed, site) at element row D + col (p quantised as coot_debug_dropout_scales does), to y (16-bit) and / or y32.  x is fp32
 * (x_f32 != 0) or 16-bit.  x2: rows R0 .. R - 1 are rows 0 .. of x2.  cu (int32 [nseq + 1] row starts): output row r is token
 * r - cu[n] of sequence n, read from row n L0 + l of x (n < N0) or (n - N0) L1 + l of x2, or from row r of x with src_packed;
 * pos_out[r] = l.  max_wgs > 0 or nt != 0: the row-walking kernel of the input stages.  Backward (D <= 1024): dy (16-bit) or dy32,
 * plus dy_add, times the forward's mask (p, seed, site), gives dx (16-bit), dx32, dxm = dx times the mask of (seed_m, site_m) at
 * element row dxm_drop_ld + col; dgain, dbias, dxcolsum (column sums of dxm if set, else of dx) are ADDED to; any of them may be
 * NULL.  part_ws (optional): the partial-sum workspace a network call would provide.  Strides in elements, multiples of 4. */
typedef struct coot_ln_args {
  const void* x; int x_f32; int64_t ldx;
  const void* x2; int R0;
  int R, D;
  const float* gain; const float* bias;
  const float* pe; int pe_L;
  void* y; int64_t ldy;
  float* y32; int64_t ldy32;
  float p; uint64_t seed; unsigned site;
  const int* cu; int nseq, N0, L0, L1; int* pos_out; int src_packed;
  int max_wgs, nt;
  const void* dy; int64_t lddy;
  const float* dy32; int64_t lddy32;
  const void* dy_add; int64_t lddy_add;
  void* dx; int64_t lddx;
  float* dx32; int64_t lddx32;
  void* dxm; int64_t lddxm;
  float pm; uint64_t seed_m; unsigned site_m; int64_t dxm_drop_ld;
  float* dgain; float* dbias; float* dxcolsum;
  float* part_ws; size_t part_ws_floats;
} coot_ln_args;
int coot_debug_ln(const coot_ln_args* a, int backward, coot_stream_t stream);
/* One or two GenPool segments (tests): launch_pool_fwd2 / launch_pool_bwd2.  Per sequence n and channel: rows >= lens[n] of the L
 * padded rows count as scores of -32752; w = softmax of s over the rows; pooled = sum_l w m_w z with m_w the dropout mask of
 * (seed_w, site_w) at element (first row + l) D + channel; smax / ssum: the maximum and sum exp(s - max).  cu: sequence n is rows
 * cu[n] .. cu[n] + lens[n] - 1, without padding rows.  pk_*: pooled rows also go to pk_out [pk_B, pk_Cmax, D] by pk_counts (zero
 * padded), pk_mask (1 = padding), pk_lens.  Backward: reads smax, ssum, pooled; ds = w (dpooled z m_w - dpooled pooled) m_s with m_s
 * the mask of (seed_s, site_s) at element (drop_s_row0 + row) drop_s_ld + channel; dz = dpooled w m_w; padded rows zero;
 * ds_colsum += column sums of ds (through part_ws if given; inside a deferred-reduction scope with defer != 0). */
typedef struct coot_pool_args {
  const void* s; int64_t lds;
  const void* z; int64_t ldz;
  const int64_t* lens; const int* cu;
  int N, L, D;
  float* pooled; int64_t ldp;
  float* pooled_copy; float* smax; float* ssum;
  float p_w; uint64_t seed_w; unsigned site_w;
  const float* dpooled; int64_t lddp;
  void* ds; int64_t ldds;
  void* dz; int64_t lddz;
  float* ds_colsum;
  float p_s; uint64_t seed_s; unsigned site_s; int64_t drop_s_ld, drop_s_row0;
  const int64_t* pk_counts; int pk_B, pk_Cmax;
  float* pk_out; uint8_t* pk_mask; int64_t* pk_lens;
} coot_pool_args;
int coot_debug_pool(const coot_pool_args* segs, int nseg, int backward, float* part_ws, size_t part_ws_floats, int defer,
                    coot_stream_t stream);
/* avg_special: out[n] = sum over ALL L rows of z / lens[n]; backward: every one of the L rows of dz = dpooled[n] / lens[n] */
int coot_debug_avgpool(const void* z, int64_t ldz, const int64_t* lens, int N, int L, int D, float* out, int64_t ldo,
                       coot_stream_t stream);
int coot_debug_avgpool_bwd(const float* dpooled, int64_t lddp, const int64_t* lens, int N, int L, int D, void* dz, int64_t lddz,
                           coot_stream_t stream);
/* demb_items[ptr_b + c] += dout1[b, c] (+ dout2[b, c]) for c < counts[b]; demb_ctx[b] += dctx[b] (dout2, dctx optional) */
int coot_debug_pack_bwd_join(const float* dout1, const float* dout2, const float* dctx, const int64_t* counts, int B, int Cmax,
                             int D, float* demb_items, float* demb_ctx, coot_stream_t stream);
/* out[c] += sum_r x[r, c] (x 16-bit); part_ws as in coot_debug_ln */
int coot_debug_colsum_bf16(const void* x, int64_t ldx, int R, int C, float* out, float* part_ws, size_t part_ws_floats,
                           coot_stream_t stream);
/* HIP-event timing of every gemm_nt launch (the dominant kernel) while enabled; collect() synchronises the
 * recorded events and returns summed duration [ms], algorithmic flops (2*M*N*K) and launch count.
 * only_big_k != 0 restricts to the input-FC instances (K >= 1024). */
int coot_timing_enable(int on);
int coot_timing_collect(int only_big_k, double* ms, double* flops, int* launches);
/* probe of ds_read_b64_tr_b16: out[64*4] = what each lane reads from a 16x64 bf16 LDS tile holding its own index */
int coot_probe_tr16(uint16_t* out, coot_stream_t stream);

#if defined(__GNUC__) || defined(__clang__)
#pragma GCC visibility pop
#endif
#ifdef __cplusplus
}
#endif
#endif /* COOT_HIP_H */
