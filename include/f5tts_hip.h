/*
 * f5tts_hip.h -- C ABI of the MI355X-native (gfx950) F5-TTS flow-matching sampling engine.
 *
 * The reference (lucasnewman/f5-tts-mlx) has no FFI layer: its boundary for this path is the Python
 * API `F5TTS.sample` (f5_tts_mlx/cfm.py:264-402) -> `DiT.__call__` (f5_tts_mlx/dit.py:374-401) with
 * MLX arrays.  This header is what a Python/ctypes (or cgo/JNI/...) host binds instead; every entry
 * point cites the reference code it replaces.  Conventions:
 *   - plain pointers and sizes only; "dev" pointers are HIP device pointers, "host" pointers are
 *     ordinary host memory; the caller owns every buffer (weights arena, workspace, inputs, outputs)
 *   - every function returns 0 on success, non-zero on error; `f5_last_error()` (thread local)
 *     describes the last failure.  Nothing throws across the ABI.
 *   - `stream` is a hipStream_t passed as void*; all work is enqueued on it, nothing synchronises
 *     unless stated.  An engine handle is not re-entrant (one handle per device / stream at a time).
 */
#ifndef F5TTS_HIP_H
#define F5TTS_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct f5_engine f5_engine;

/* Constructor arguments of the reference DiT (dit.py:332-346) + derived sizes.  The accepted family (docs/geometries.md): dim a
 * multiple of 256 up to 1024; dim_head 64; the attention inner width heads * dim_head a multiple of 256 up to 1024, equal to dim or
 * not (dit.py:117-125 projects dim -> inner -> dim); dim / conv_pos_groups 32, 48 or 64 channels per group; text_dim a multiple of 128
 * up to 1024.  F5_PREC_MXFP8 accepts only inner == dim, 64-channel groups and text_dim % 256 == 0. */
typedef struct f5_config {
    int32_t dim;             /* 1024 */
    int32_t depth;           /* 22 */
    int32_t heads;           /* 16 (heads * dim_head: a multiple of 256, <= 1024; need not equal dim) */
    int32_t dim_head;        /* 64 (only 64 is supported by the attention kernel) */
    int32_t ff_dim;          /* dim * ff_mult = 2048 */
    int32_t mel_dim;         /* 100 */
    int32_t text_num_embeds; /* 2545 (embedding table has +1 rows, dit.py:184) */
    int32_t text_dim;        /* 512 (a multiple of 128, <= 1024) */
    int32_t text_ff_dim;     /* text_dim * conv_mult = 1024 */
    int32_t conv_layers;     /* 4; 0 = plain embedding: no positional table, no ConvNeXt blocks, no masking (dit.py:188-194) */
    int32_t conv_pos_kernel; /* 31 */
    int32_t conv_pos_groups; /* 16 (dim / groups must be 32, 48 or 64; 32 needs an even group count) */
    int32_t freq_embed_dim;  /* 256 */
    int32_t text_max_pos;    /* 4096 */
    int32_t text_mask_padding; /* 1 (dit.py:186): zero the text embedding at filler / padded positions around every text block */
} f5_config;

/* MFMA operand encoding.  The reference computes in fp32 throughout (dit.py, cfm.py); measured mel-L1 drift of a full 32-point
 * sample against the fp32 oracle: BF16 2-4e-3 (outside the 1e-3 gate), F16 (IEEE half operands, same MFMA rate, 11 significand
 * bits, producers saturate at +-65504) inside the gate, BF16X3 (hi/lo split, 3 MFMA passes) ~5e-6; MXFP8: the four block GEMMs on
 * MX-fp8 (e4m3 + E8M0 per 32), rest bf16 -- a reduced-precision mode. */
enum { F5_PREC_BF16 = 0, F5_PREC_BF16X3 = 1, F5_PREC_MXFP8 = 2, F5_PREC_F16 = 3 };
enum { F5_GRAPH_OFF = 0, F5_GRAPH_ON = 1, F5_GRAPH_AUTO = 2 };  /* f5_sample_args.use_graph */
enum { F5_EULER = 0, F5_MIDPOINT = 1, F5_RK4 = 2,         /* cfm.py:38-122 */
       /* Adams-Bashforth of order 2 / 3 on the call's (possibly non-uniform, possibly per-row) grid: ONE evaluation per step, at the grid
        * point t_i, like Euler; step i adds h (w0 k_i + w1 k_{i-1} + w2 k_{i-2}), k = the guided velocities of this and the two steps
        * before, kept in the workspace.  The weights integrate the Lagrange interpolant through the nodes in use over [t_i, t_{i+1}],
        * computed on the host in fp64 from the fp32 grid and rounded once; step 0 is the Euler step, step 1 is second order; a step
        * whose back-spacing is not positive drops to the highest order whose spacings are (docs/multistep.md).  Every entry point and
        * every size query takes them; the workspace grows by the weight words only. */
       F5_AB2 = 3, F5_AB3 = 4 };

const char* f5_last_error(void);
int f5_version(void);

/* ---- engine lifetime ------------------------------------------------------------------------ */
int f5_engine_create(const f5_config* cfg, int precision, f5_engine** out);
void f5_engine_destroy(f5_engine* e);   /* also destroys every cached hipGraphExec */
/* at most `max_graphs` (default 8) captured sample graphs are kept per engine; the least recently used one is destroyed */
int f5_engine_set_graph_cache(f5_engine* e, int max_graphs);
int f5_engine_graph_count(f5_engine* e);
/* Per-engine launch options (two engines of one process keep their own): "q_premul" (1: q leaves the QKV epilogue multiplied by
 * softmax_scale * log2 e), "qkv_transposed" (1: transposed q / k tiles in the 256x256 QKV kernel), "ln_fusion" (0; 1 = LN-modulate
 * fused behind small-tile residual GEMMs, measured slower), "gemm_flags" (0; F5GemmArgs debug bits of this engine's launches),
 * "attn_pipe" (-1 = the process default of f5_debug_set_attn_pipe, 0 = large-grid attention kernel v2f, 1 = in-wave software-pipelined v2p),
 * "null_keeps_cond" (0; 1 = the second branch of f5_dit_forward / f5_sample keeps the audio conditioning and drops only the text:
 * DiT.__call__(drop_audio_cond=False, drop_text=True), dit.py:374-401), "ln_fold" (LN-modulate folded into the epilogues of the block
 * GEMMs around it, see f5_debug_set_op_fold_producer: -1 (default) = where it is measured faster: >= 22 000 rows (batch >= 12 at the
 * 335M shape and 937 frames) with the four block GEMMs on the 256x256 / role-split 128x256 kernels, f16 / bf16 modes; 0 = never;
 * 1 = wherever it can run (batch >= 4 at that shape), f5_sample fails where it cannot), "isolate_rows" (0; 1 = in a call with
 * args->use_mask, row b reads nothing from its own positions n >= durations[b]: both conv-pos launches and the depthwise conv of the
 * text blocks read zeros there and the text GRN norms over the row's own durations[b] frames, so a row of a padded batch runs the
 * arithmetic of the reference's sample() on that row alone, docs/isolate_rows.md.  It serves f5_sample, _edit, _rows, _dual, _window
 * and f5_dit_forward*; a call without use_mask launches what it launches with 0; the workspace sizes do not change; precision mxfp8
 * refuses it in every one of those calls, before any launch).
 * Part of the hipGraph cache key.  New engines start from the process defaults (f5_debug_set_ln_fusion / _qkv_transposed /
 * _q_premul). */
int f5_engine_set_option(f5_engine* e, const char* name, int value);
int f5_engine_get_option(f5_engine* e, const char* name, int* value);

/* ---- weights: replaces F5TTS.load_weights / from_pretrained upload (cfm.py:475-518) ------------
 * The caller allocates `f5_weights_bytes` of device memory (one contiguous arena, so that a single
 * RCCL broadcast replicates the model), hands it over, then loads every tensor by its reference
 * (MLX-layout) name, e.g. "transformer.transformer_blocks.3.attn.to_q.weight".  host_data is fp32,
 * C-contiguous, shape as in the reference.  f5_finalize_weights checks completeness and builds the
 * derived tables (text positional table, rope.py:63-73). */
int f5_weights_bytes(f5_engine* e, size_t* bytes);
int f5_set_weights_arena(f5_engine* e, void* dev_arena, size_t bytes, void* stream);
int f5_load_tensor(f5_engine* e, const char* name, const float* host_data, int ndim, const int64_t* shape);
int f5_finalize_weights(f5_engine* e, void* stream);
/* A second handle on `owner`'s finalised arena (same f5_config and precision; nothing is copied or written, the caller keeps the arena
 * alive for both).  Handles are not re-entrant, but two handles may run at once: a host that drives two of them from two threads on two
 * streams, each with half of a large batch, fills the partly empty last rounds of each other's launches (-5 % at 32 utterances;
 * f5_tts_mlx_amd/engine.py Engine._sample_split does this, INTEGRATION.md describes it).  Own workspace, hipGraphs and status word per
 * handle. */
int f5_share_weights(f5_engine* e, const f5_engine* owner);
/* Multi-GPU start-up (one process per GPU, utterances sharded, no per-step communication): replicate rank `root`'s arena over an
 * RCCL communicator (`nccl_comm` = ncclComm_t) with ONE ncclBroadcast enqueued on `stream`; ranks other than root are marked
 * loaded and then call f5_finalize_weights.  librccl.so is resolved with dlopen at the first call.  (A torch.distributed host
 * does the same with dist.broadcast on the arena tensor, f5_tts_mlx_amd/dist.py.) */
int f5_broadcast_weights(f5_engine* e, void* nccl_comm, int root, int rank, void* stream);
/* for ranks that received the arena by broadcast instead of f5_load_tensor */
int f5_mark_weights_loaded(f5_engine* e);

/* ---- F5TTS.sample hot path (cfm.py:312-397) ---------------------------------------------------
 * The Python wrapper keeps the reference's host logic (text -> ids, lens / duration clamp, time
 * grid); the engine runs everything from the masks to the final splice on the GPU.             */
typedef struct f5_sample_args {
    int32_t B;                 /* utterances                                                     */
    int32_t N;                 /* max_duration in frames (cfm.py:319); the engine needs N >= 4   */
    int32_t nt;                /* text columns                                                   */
    const int32_t* text;       /* dev  [B][nt] token ids, -1 padded (utils.py:124-133)           */
    const float* cond;         /* dev  [B][N][mel] reference mel, zero padded to N (cfm.py:321)  */
    const int32_t* lens;       /* host [B] conditioning length per utterance (cfm.py:301-303)    */
    const int32_t* durations;  /* host [B] total frames per utterance (cfm.py:317-318)           */
    const float* y0;           /* dev  [B][N][mel] initial noise, zero beyond durations[b]       */
    const float* t;            /* host [steps] time grid (cfm.py:379-381)                        */
    int32_t steps;             /* number of grid POINTS                                          */
    int32_t method;            /* F5_EULER / F5_MIDPOINT / F5_RK4 / F5_AB2 / F5_AB3               */
    float cfg_strength;        /* < 1e-5 disables the null branch (cfm.py:352)                   */
    int32_t use_mask;          /* key-padding mask + output row mask; reference: batch > 1       */
    int32_t use_graph;         /* F5_GRAPH_ON: capture/replay the whole call as one hipGraph (cached per shape signature,
                                * LRU bounded); F5_GRAPH_AUTO: eager on the first sighting of a signature, graph from the
                                * second on (mx.compile re-traces per call shape in the reference, cfm.py:392)       */
    float* out;                /* dev  [B][N][mel] where(cond_mask, cond, y_final)               */
    float* trajectory;         /* dev  [steps][B][N][mel] or NULL                                */
    void* workspace;           /* dev, f5_workspace_bytes                                        */
    size_t workspace_bytes;
} f5_sample_args;

int f5_workspace_bytes(f5_engine* e, int B, int N, int nt, int steps, int method, size_t* bytes);
int f5_sample(f5_engine* e, const f5_sample_args* args, void* stream);
/* Speech editing: f5_sample with the conditioning chosen FRAME BY FRAME.  The reference trains the DiT as an infilling model -- its
 * training forward zeroes an interior span of the conditioning mel and predicts that span (F5TTS.__call__, cfm.py:198-224) -- but its
 * sampler only ever conditions on a prefix (cond_mask = lens_to_mask(lens), cfm.py:323-331, :395-397).  Here cond_keep_dev, dev uint8
 * [B][N] (non-zero = "this frame is conditioning"), replaces the test n < lens[b] in the two places that decide between conditioning
 * and generated frames: step_cond = where(keep, cond, 0) in the hoisted input packing (cfm.py:331) and out = where(keep, cond, y) in
 * the final splice (cfm.py:395-397).  Values are selected, never multiplied by the mask: whatever `cond` holds at a frame that is not
 * kept (NaN included) reaches nothing.  Everything else -- launches, noise, time grid, key-padding mask, status word -- is f5_sample's;
 * with keep[b][n] = (n < lens[b]) the results are f5_sample's bit for bit.  `lens` in the arguments is validated as in f5_sample and
 * otherwise unused.  The mask is copied into the workspace (behind everything f5_sample uses; f5_workspace_bytes covers both calls)
 * outside the captured part: one hipGraph per shape signature serves every mask, and the graphs of f5_sample and f5_sample_edit share
 * the engine's cache without replaying each other (the edit flag is part of the key).  Refused before any launch: a null mask and
 * everything f5_sample refuses. */
int f5_sample_edit(f5_engine* e, const f5_sample_args* args, const uint8_t* cond_keep_dev /* [B][N] */, void* stream);

/* Per-request sampling controls: f5_sample with the time grid and the guidance strength chosen PER BATCH ROW, so that requests with
 * different sway coefficients / cfg strengths share one call.  args->t and args->cfg_strength are not read.  The adaLN table is built for
 * every (evaluation, row) pair, [nfe][B][(6 depth + 2) dim] floats (about 545 MB for 32 rows x 31 evaluations at the 335M shape): only
 * f5_workspace_bytes_rows asks for that space, f5_workspace_bytes is unchanged.  The two gated projections of a block write their fp32
 * result into a dead buffer and one row kernel applies the row's gate and produces the LayerNorm-modulate that follows; the LN fold and
 * the fused LN tail do not run (ln_fold = 1 fails with a message), precision mxfp8 is refused.  A row with cfg_rows[b] < 1e-5 takes the
 * conditional prediction alone (cfm.py:352); the null branch runs when any row is guided.  Controls (and the optional keep mask, as in
 * f5_sample_edit) are staged into the workspace outside the captured part: one hipGraph per shape signature serves every set of
 * values, and the rows flag is part of the cache key.  Status word, f5_sample_status*, trajectory and the final splice are f5_sample's.
 * Refused before any launch: null controls / t_rows / cfg_rows, a non-finite control value, a workspace smaller than
 * f5_workspace_bytes_rows, and everything f5_sample refuses. */
typedef struct f5_row_controls {
    const float* t_rows;          /* host [B][steps]: each row's own time grid (cfm.py:379-381 evaluated per row) */
    const float* cfg_rows;        /* host [B] */
    const uint8_t* cond_keep_dev; /* dev [B][N] or NULL: as f5_sample_edit */
} f5_row_controls;
int f5_workspace_bytes_rows(f5_engine* e, int B, int N, int nt, int steps, int method, size_t* bytes);
int f5_sample_rows(f5_engine* e, const f5_sample_args* args, const f5_row_controls* controls, void* stream);

/* Dual guidance: f5_sample_rows with TWO guidance strengths per batch row.  The reference trains three conditioning states (its loss
 * forward drops the audio alone, and the text only together with the audio, cfm.py:230-232): F = audio and text kept, T = audio dropped,
 * N = both dropped.  Per element, in fp32, with a = audio_cfg_rows[b] and c = text_cfg_rows[b]:
 *     k = (F + (F - T) a) + (T - N) c
 * (a == c is algebraically F + (F - N) c, the rule of f5_sample -- within rounding, not bit for bit).  A row with both strengths below
 * 1e-5 takes k = F; T is loaded when either is >= 1e-5, N only when c >= 1e-5; selections, so a NaN on a side that is not taken
 * reaches nothing.  All three branches run as one batch of 3 B N rows (in the order F, N, T) as soon as any row has either strength,
 * else F alone.  The route is the per-row one (adaLN table per (evaluation, row), no LN fold); the text path still runs for two
 * branches, T reuses F's text embedding.  f5_workspace_bytes_dual is the plan of f5_workspace_bytes_rows with every buffer of the DiT
 * itself at 3 B N rows; f5_workspace_bytes and f5_workspace_bytes_rows are unchanged.  Graphs: controls are staged outside the captured
 * part and a dual flag is part of the cache key.  args->t and args->cfg_strength are not read.
 * Refused before any launch: everything f5_sample_rows refuses (mxfp8 included), a non-finite strength, a workspace below
 * f5_workspace_bytes_dual, and engine option null_keeps_cond = 1 (the meanings of the branches would collide). */
typedef struct f5_dual_controls {
    const float* t_rows;          /* host [B][steps] */
    const float* text_cfg_rows;   /* host [B]: T against N */
    const float* audio_cfg_rows;  /* host [B]: F against T */
    const uint8_t* cond_keep_dev; /* dev [B][N] or NULL: as f5_sample_edit */
} f5_dual_controls;
int f5_workspace_bytes_dual(f5_engine* e, int B, int N, int nt, int steps, int method, size_t* bytes);
int f5_sample_dual(f5_engine* e, const f5_sample_args* args, const f5_dual_controls* controls, void* stream);

/* Guidance window: f5_sample_rows / f5_sample_dual with the guidance of row b applied only while lo_rows[b] <= t <= hi_rows[b].  `t` is
 * the fp32 time of the FUNCTION EVALUATION for that row -- the value the adaLN table is built from; for midpoint and rk4 the stage's
 * time, not the step's -- and both ends are inclusive, compared in fp32.  Outside its window a row's effective strengths are 0 (with
 * dual guidance both strengths are gated by the one window).  An evaluation in which some row has an effective strength >= 1e-5 is WIDE:
 * it runs the call's full branch count (2, or 3 with audio_cfg_rows), and a row outside its window takes k = F by the selection of the
 * stage kernels.  Every other evaluation is NARROW: the DiT runs on the conditional branch alone (the first B N rows of every buffer)
 * and every row takes k = F.  With no wide evaluation the whole call runs one branch.  audio_cfg_rows = NULL selects single guidance
 * (f5_sample_rows' rule and two branches), else dual guidance (f5_sample_dual's rule and three).  f5_workspace_bytes_window is the plan
 * of f5_workspace_bytes_rows (dual = 0) or f5_workspace_bytes_dual (dual = 1) plus the effective-strength tables, [nfe][B] floats, one
 * or two of them, behind everything those plans lay out; the other three size calls are unchanged.  Graphs: the tables are staged
 * outside the captured part with the other row scalars; the wide / narrow pattern is structural and part of the cache key, the
 * strengths and bounds are not, so one graph serves every set of values with the same pattern.  args->t and args->cfg_strength are not
 * read.  Refused before any launch, each with its own message: null controls or a null t_rows / text_cfg_rows / lo_rows / hi_rows, a
 * non-finite strength or bound, lo > hi, a workspace below f5_workspace_bytes_window, and everything f5_sample_rows / f5_sample_dual
 * refuse (mxfp8 and ln_fold = 1 included). */
typedef struct f5_window_controls {
    const float* t_rows;          /* host [B][steps] */
    const float* text_cfg_rows;   /* host [B]: the strength of single guidance, T against N with dual guidance */
    const float* audio_cfg_rows;  /* host [B]: F against T, or NULL = single guidance with two branches */
    const float* lo_rows;         /* host [B] */
    const float* hi_rows;         /* host [B] */
    const uint8_t* cond_keep_dev; /* dev [B][N] or NULL: as f5_sample_edit */
} f5_window_controls;
int f5_workspace_bytes_window(f5_engine* e, int B, int N, int nt, int steps, int method, int dual, size_t* bytes);
int f5_sample_window(f5_engine* e, const f5_sample_args* args, const f5_window_controls* controls, void* stream);
/* Test hook: the wide (1) / narrow (0) flag of every evaluation of the engine's most recent f5_sample_window call that got past its
 * argument checks.  *nfe gets the number of evaluations, `wide` the first min(*nfe, cap) flags.  Host bookkeeping only. */
int f5_debug_last_sample_pattern(f5_engine* e, int* nfe, uint8_t* wide, int cap);

/* Status word of the last f5_sample / f5_dit_forward on the workspace of `args`.  It is the FIRST 32-bit word of the workspace for every
 * shape and solver (a caller may copy it itself).  bit 1 (F5_STATUS_FOLD_RAN) = the LN fold (engine option "ln_fold") ran in that call;
 * bit 0 (F5_STATUS_FOLD_OVERFLOW) = a value of the folded LayerNorm operand (x - m)(1 + scale) did not fit fp16 (precision f16): the
 * output is saturated there -- rerun with ln_fold = 0 or in bf16 (f5_tts_mlx_amd.engine.Engine does that by itself);
 * bit 2 (F5_STATUS_SATURATED, precision f16, engine option "sat_check" = 1, the default) = some OTHER producer of a 16-bit MFMA operand
 * -- LN-modulate, q / k / v behind the rotation, the GELU output of FF1, conv-pos, the packed ODE state, the text path -- clamped a
 * value beyond +-65 504 somewhere in the call (every block of every evaluation is covered, at every batch size): the result is finite
 * and wrong there; this checkpoint / input needs precision bf16x3 (fp32-class) or bf16 (Engine re-runs the call in bf16x3 by itself).
 * f5_sample_status synchronises `stream`; f5_sample_status_async only
 * enqueues the 4-byte device-to-host copy behind the call (`flags` should be pinned host memory, valid once the caller has
 * synchronised `stream` or an event recorded after it): no host block per call.  No reference counterpart (the reference has no
 * reduced-precision operands). */
#define F5_STATUS_FOLD_OVERFLOW 1
#define F5_STATUS_FOLD_RAN 2
#define F5_STATUS_SATURATED 4
int f5_sample_status(f5_engine* e, const f5_sample_args* args, int* flags, void* stream);
int f5_sample_status_async(f5_engine* e, const f5_sample_args* args, int* flags, void* stream);
/* *active = 1 when f5_sample with these arguments runs the LN fold (the only configuration that can set bit 0 of the status word): a
 * host-side question, no GPU work, so a caller only reads the word where it can say something.  For f5_dit_forward pass steps = 2,
 * method = F5_EULER. */
int f5_engine_ln_fold_active(f5_engine* e, const f5_sample_args* args, int* active);

/* One DiT forward (dit.py:374-401) for tests/diagnostics: same inputs as f5_sample, evaluates the
 * velocity field at time `t` for state `x` (dev [B][N][mel]); writes pred (and null when
 * cfg_strength >= 1e-5) as dev [B][N][mel] each. */
int f5_dit_forward(f5_engine* e, const f5_sample_args* args, const float* x, float t, float* pred, float* null_pred,
                   void* stream);
/* The same with one time per batch row (host [B]), as the reference's DiT takes it: one batched forward for rows at different times.
 * Workspace: f5_workspace_bytes_rows(B, N, nt, 2, F5_EULER). */
int f5_dit_forward_rows(f5_engine* e, const f5_sample_args* args, const float* x, const float* t_rows_host /* [B] */, float* pred,
                        float* null_pred, void* stream);
/* One evaluation of the three branches of dual guidance (f5_sample_dual): pred = F, null_pred = N, text_pred = T, dev [B][N][mel] each
 * (null_pred and text_pred may be NULL); all three always run, args->cfg_strength is not read.
 * Workspace: f5_workspace_bytes_dual(B, N, nt, 2, F5_EULER). */
int f5_dit_forward_dual(f5_engine* e, const f5_sample_args* args, const float* x, const float* t_rows_host /* [B] */, float* pred,
                        float* null_pred, float* text_pred, void* stream);

/* ---- per-op entry points (exported for the parity tests; all pointers are dev) ------------------
 * 16-bit operand buffers (a_hi, w_hi, qk_hi, out_hi ...) hold bf16 by default; f5_op_set_operand_type(1) switches every
 * f5_op_* call of the process to IEEE fp16 operands (the kernels are built for both), 0 switches back. */
int f5_op_set_operand_type(int fp16);
int f5_op_get_operand_type(void);   /* current setting: 0 bf16, 1 fp16 (callers that switch temporarily restore this) */
/* C = A * W^T (+epilogue), bf16 MFMA; epi codes in csrc/gemm.hpp (0 = fp32 out + bias, 1 = bf16 out) */
int f5_op_gemm(const void* a_hi, const void* a_lo, const void* w_hi, const void* w_lo, const float* bias, float* out_f32,
               void* out_bf_hi, void* out_bf_lo, int M, int N, int K, int lda, int ldw, int ldo, int nseg, int epi,
               void* stream);
/* dit.py:136-166: qk [B*n][2*dmodel] (RoPE'd q | k), vt [B*H][64][npad] -> out [B*n][dmodel] */
int f5_op_attention(const void* qk_hi, const void* qk_lo, const void* vt_hi, const void* vt_lo, void* out_hi, void* out_lo,
                    const int32_t* kv_len, int B, int H, int seq_len, int npad, int dmodel, float scale, int hp, void* stream);
/* the same with every field of the launch from the caller: leading dimensions of qk (ldqk % 8 == 0) and out (ldo % 4 == 0),
 * q_prescaled (1 = q already carries scale * log2(e): scores are in exp2 units), pipe (-1 = process default, 0 = v2f, 1 = v2p where the
 * large-grid kernels run) and the MX-fp8 output of the one-pass kernels: out8 e4m3 [B*n][ldo8] (ldo8 % 4 == 0) + out8s E8M0
 * [B*n][dmodel/32]; with out8 set the 16-bit output is not written.  f5_op_attention is this with ldqk = 2 dmodel, ldo = dmodel,
 * q_prescaled from f5_debug_set_op_q_premul, pipe = -1 and no fp8 output. */
int f5_op_attention_ex(const void* qk_hi, const void* qk_lo, const void* vt_hi, const void* vt_lo, void* out_hi, void* out_lo,
                       const int32_t* kv_len, int B, int H, int seq_len, int npad, int dmodel, float scale, int hp, int ldqk, int ldo,
                       int q_prescaled, int pipe, void* out8, void* out8s, int ldo8, void* stream);
/* QKV projection + bias + RoPE + head split (dit.py:136-158); B > 1 needs seq_len >= 4 */
int f5_op_qkv_rope(const void* a_hi, const void* a_lo, const void* w_hi, const void* w_lo, const float* bias,
                   const float* rope_cos, const float* rope_sin, void* qk_hi, void* qk_lo, void* vt_hi, void* vt_lo, int B,
                   int seq_len, int npad, int heads, int dmodel, int nseg, void* stream);
/* the same for an attention inner width (inner = heads * 64) that is not the input width K (dit.py:117-125): a [B seq_len][K],
 * w [3 inner][K], q | k [B seq_len][2 inner], V^T [B heads 64][npad].  The LN-fold hooks do not apply. */
int f5_op_qkv_rope_k(const void* a_hi, const void* a_lo, const void* w_hi, const void* w_lo, const float* bias,
                     const float* rope_cos, const float* rope_sin, void* qk_hi, void* qk_lo, void* vt_hi, void* vt_lo, int B,
                     int seq_len, int npad, int heads, int inner, int K, int nseg, void* stream);
int f5_op_rope_table(float* cos_t, float* sin_t, int seq_len, int dim_head, void* stream);
/* GROUP-major twins of the rotation tables: tq / tk are [dim_head/4][seq_len][4] floats (16 seq_len dim_head/4 bytes each, 16-byte
 * aligned), element (g, n) = (cos, cos, sin, sin) of rotation pairs 2g, 2g + 1 at position n, the q table multiplied by qscale (1 = plain
 * q): with them the staged QKV kernels accumulate the q / k column tiles transposed (rotation pairs in-lane, one 16-byte load per lane
 * and 4 features); sample() builds its own */
int f5_op_rope_table_g4(float* tq, float* tk, int seq_len, int dim_head, float qscale, void* stream);
/* dit.py:29-50 one grouped conv + Mish; mode 0 -> bf16 out, mode 1 -> out_f32 +=.  C / groups = 64, 48 or 32 channels per group; w is
 * the matrix f5_op_pack_conv_groups leaves ([f5_op_conv_packed_rows(C, C / groups)][taps * 64], rounded to the operand type): at 64
 * channels per group the reference tensor (C, taps, 64) as it is. */
int f5_op_convpos(const void* in_hi, const void* in_lo, const void* w_hi, const void* w_lo, const float* bias, void* out_hi,
                  void* out_lo, float* out_f32, int B, int seq_len, int C, int groups, int taps, int nseg, int mode,
                  void* stream);
/* f5_op_convpos on a padded batch: lens_dev, device [B], element b is lens[b] <= seq_len tokens long (elements stay seq_len rows apart).
 * Rows n >= lens[b] are read as zero without being loaded (NaN there stays out), are not written in either mode and report no
 * saturation; a workgroup whose whole 128-token tile lies at or beyond lens[b] returns at once.  Same kernels and routes as
 * f5_op_convpos; rows n < lens[b] get the bits f5_op_convpos gives at the same shape on an input with zeros past the lengths.
 * lens_dev == NULL: f5_op_convpos. */
int f5_op_convpos_ragged(const void* in_hi, const void* in_lo, const void* w_hi, const void* w_lo, const float* bias, void* out_hi,
                         void* out_lo, float* out_f32, int B, int seq_len, int C, int groups, int taps, int nseg, int mode,
                         const int32_t* lens_dev, void* stream);
/* The weight store's packing of a conv-pos weight w = (C, taps, cpg) fp32, cpg = C / groups = 32, 48 or 64, done on the host (no
 * device): out = [f5_op_conv_packed_rows(C, cpg)][taps * 64] floats.  cpg 64: w itself.  cpg 32: C rows, two groups share a block-
 * diagonal 64-wide super group (output channel o keeps its 32 input channels in columns ((o / 32) % 2) * 32 ... + 31 of every tap, the
 * rest is zero).  cpg 48: C / 48 * 64 rows, group g in rows g * 64 ... g * 64 + 47 with its 48 input channels in columns 0 ... 47 of
 * every tap, zeros elsewhere.  f5_op_conv_packed_rows: -1 for a width other than 32 / 48 / 64 or one that does not divide C. */
int f5_op_conv_packed_rows(int C, int cpg);
int f5_op_pack_conv_groups(const float* w, int C, int taps, int cpg, float* out);
/* dit.py:270 */
int f5_op_ln_modulate(const float* x, const float* scale, const float* shift, void* out_hi, void* out_lo, int rows, int dim,
                      void* stream);
/* MFMA rate yardstick (no reference counterpart; BASELINE.md section 4: "print the measured MFMA micro-benchmark peak you divide by"):
 * blocks x 8 waves x iters x 16 v_mfma_f32_32x32x16 of the current operand type on register operands -- operands NULL = lane-constant
 * registers, else >= 16 x 64 x 8 16-bit values of workload-like data that are rotated through the MFMAs; *flops = flops of the launch */
int f5_op_mfma_peak(const void* operands, int blocks, int iters, float* sink, double* flops, void* stream);
/* convnext_v2.py:46-48 */
int f5_op_dwconv_ln(const float* x, const float* dw_w, const float* dw_b, const float* ln_w, const float* ln_b, void* out_hi,
                    void* out_lo, int nbatch, int seq_len, int dim, void* stream);
/* convnext_v2.py:15-18; scratch: f5_op_grn_scratch_floats floats */
size_t f5_op_grn_scratch_floats(int nbatch, int seq_len, int dim);
int f5_op_grn(const float* g, const float* gamma, const float* beta, float* scratch, void* out_hi, void* out_lo, int nbatch,
              int seq_len, int dim, void* stream);
/* f5_op_grn on a padded batch: lens_dev, device [nbatch], element b's norm runs over its own lens[b] <= seq_len tokens.  Tokens
 * n < lens[b] get the bits of f5_op_grn on that element alone at seq_len = lens[b]; tokens past the length are exact zeros, their g is
 * not loaded and they report no saturation.  scratch: f5_op_grn_scratch_floats(nbatch, seq_len, dim) floats. */
int f5_op_grn_ragged(const float* g, const float* gamma, const float* beta, float* scratch, void* out_hi, void* out_lo, int nbatch,
                     int seq_len, int dim, const int32_t* lens_dev, void* stream);
/* dit.py:196-222 (index path is bit exact) */
int f5_op_text_embed(const int32_t* text, int nt, const float* table, const float* pos_table, int max_pos, float* out,
                     int32_t* ids_out, uint8_t* keep_out, int B, int seq_len, int dim, void* stream);
/* same with mask_padding=False (duration.py:116-118): filler positions keep their embedding */
int f5_op_text_embed_nomask(const int32_t* text, int nt, const float* table, const float* pos_table, int max_pos, float* out,
                            int32_t* ids_out, uint8_t* keep_out, int B, int seq_len, int dim, void* stream);
int f5_op_text_pos_table(float* table, int max_pos, int dim, void* stream);
/* out = (resid + A W^T + bias) * keep[row]  (convnext_v2.py:53-54, dit.py:225); keep may be NULL */
int f5_op_gemm_resid_keep(const void* a_hi, const void* a_lo, const void* w_hi, const void* w_lo, const float* bias,
                          const float* resid, const uint8_t* rowkeep, float* out, int M, int N, int K, int lda, int ldw, int ldo,
                          int nseg, void* stream);
/* fp32 [rows][cols] (rows with keep==0 zeroed) -> bf16 (hi, lo) columns [col0, col0+cols) of a [rows][ld] operand matrix */
int f5_op_pack_bf16(const float* src, const uint8_t* rowkeep, void* out_hi, void* out_lo, int rows, int cols, int ld, int col0,
                    void* stream);
/* duration.py:137,188-190 + utils.py:82-90: RMSNorm -> masked mean over n -> Linear(dim->1) -> Softplus; out [B] seconds */
int f5_op_duration_head(const float* x, const float* g, const float* w, const uint8_t* mask, float* out, int B, int seq_len,
                        int dim, float eps, void* stream);
/* dit.py:61-82, 267 small fp32 GEMM */
int f5_op_time_sinus(const float* t, float* out, int n, int dim, void* stream);
int f5_op_skinny_gemm(const float* a, const float* w, const float* b, float* out, int M, int N, int K, int silu_in,
                      int silu_out, void* stream);
/* cfm.py:56,364: out = base + (coef*dt/divisor) * cfg(pred, null) */
int f5_op_cfg_axpy(const float* pred, const float* null_pred, float cfg, const float* base, const float* dt_dev, float coef,
                   float divisor, float* out, void* xin_hi, void* xin_lo, int rows, int mel_dim, void* stream);
/* cfm.py:38-122, :364, the whole ODE stage: k = pred + (pred - null_pred) * cfg (pred alone when null_pred is NULL; cfg_ptr, a
 * device scalar, replaces cfg when not NULL), kstore = k when not NULL, a = coef * dt / divisor;
 * mode 0: out = base + a * k; mode 1 (RK4 final, cfm.py:117): out = base + a * (k1 + 2 k2 + 2 k3 + k).
 * (xin_hi, xin_lo): `out` as 16-bit operands [rows][128], zero padded (either may be NULL) */
int f5_op_ode_stage(const float* pred, const float* null_pred, float cfg, const float* cfg_ptr, const float* base, const float* dt_dev,
                    float coef, float divisor, int mode, float* kstore, const float* k1, const float* k2, const float* k3, float* out,
                    void* xin_hi, void* xin_lo, int rows, int mel_dim, void* stream);
/* f5_op_ode_stage with the guidance strength and the step size per row: row r uses cfg_rows[v] and dt_rows[v] (dev fp32 [nvec] each),
 * v = (r / rows_per_vec) % nvec.  Same arithmetic per element; a row with cfg_rows[v] < 1e-5 takes k = pred by selection (cfm.py:352),
 * even when null_pred is given (a NaN there reaches nothing). */
int f5_op_ode_stage_rows(const float* pred, const float* null_pred, const float* cfg_rows, const float* base, const float* dt_rows,
                         int rows_per_vec, int nvec, float coef, float divisor, int mode, float* kstore, const float* k1, const float* k2,
                         const float* k3, float* out, void* xin_hi, void* xin_lo, int rows, int mel_dim, void* stream);
/* f5_op_ode_stage_rows for dual guidance: F = pred, T = text_pred, N = null_pred and two strengths per row,
 * k = (F + (F - T) audio_cfg_rows[v]) + (T - N) text_cfg_rows[v] in fp32.  T is loaded when either strength is >= 1e-5, N only when
 * text_cfg_rows[v] >= 1e-5, a row with both below takes k = F: selections, a NaN on a side that is not taken reaches nothing.  A NULL
 * text_pred is k = F; a NULL null_pred leaves the (T - N) term out.  Everything behind k (step, kstore, rk4 combine, xin packing) has the
 * bits of f5_op_ode_stage.  Refused before a launch, each with its own message: null pred, base, out, strengths or dt_rows;
 * rows_per_vec < 1; nvec < 1; mel_dim > 128. */
int f5_op_ode_stage_dual(const float* pred, const float* text_pred, const float* null_pred, const float* audio_cfg_rows,
                         const float* text_cfg_rows, const float* base, const float* dt_rows, int rows_per_vec, int nvec, float coef,
                         float divisor, int mode, float* kstore, const float* k1, const float* k2, const float* k3, float* out,
                         void* xin_hi, void* xin_lo, int rows, int mel_dim, void* stream);
/* Mode 2 of the three stage kernels, the Adams-Bashforth step of F5_AB2 / F5_AB3 (kernels of their own: modes 0 and 1 are untouched).
 * route 0 = f5_op_ode_stage's rule for k (cfg: device scalar or NULL, dt and abw [3] for the call; text_pred, audio_cfg_rows,
 * rows_per_vec and nvec are not read), 1 = f5_op_ode_stage_rows' (cfg and dt [nvec], abw [nvec][3]), 2 = f5_op_ode_stage_dual's.  Then
 *     out = fma(dt, fma(w2, k2, fma(w1, k1, w0 k)), base),   k -> kstore,   (w0, w1, w2) = abw[3 v ...]
 * k1 / k2: the velocities of the step before and of the one before that.  A term whose pointer is NULL or whose weight is exactly 0 is
 * left out by selection: its buffer is not loaded.  The padded 16-bit copy of out goes to xin_hi / xin_lo as in mode 0.  Refused before
 * a launch: a route outside 0..2; null pred, base, dt, out, abw or kstore; kstore equal to k1 or k2; what the route's launcher refuses. */
int f5_op_ode_stage_ab(int route, const float* pred, const float* text_pred, const float* null_pred, const float* audio_cfg_rows,
                       const float* cfg, const float* base, const float* dt, const float* abw, int rows_per_vec, int nvec,
                       float* kstore, const float* k1, const float* k2, float* out, void* xin_hi, void* xin_lo, int rows, int mel_dim,
                       void* stream);
/* Residual update and the LayerNorm-modulate behind it with per-row vectors: row r of the [rows][dim] buffers reads vector
 * v = (r / rows_per_vec) % nvec of gate / ln_scale / ln_shift (vec_stride >= dim floats apart, a multiple of 4).
 * With y (fp32 [rows][dim], the GEMM result including bias; may be NULL): x = fmaf(gate[v][c], rowkeep[r] ? y : 0, x) in place (rowkeep
 * uint8 [rows] or NULL; a selection: NaN in a dropped row's y reaches nothing).  With ln_scale (NULL together with ln_shift = no LN
 * output): (out_hi, out_lo) = LN(x)(1 + ln_scale[v]) + ln_shift[v], eps 1e-6, the bits of f5_op_ln_modulate on that row (out_lo may
 * be NULL).  y == NULL is f5_op_ln_modulate with per-row vectors.  dim 256 / 512 / 768 / 1024. */
int f5_op_resid_gate_ln_rows(const float* y, float* x, const float* gate, const uint8_t* rowkeep, const float* ln_scale,
                             const float* ln_shift, void* out_hi, void* out_lo, int rows, int dim, int rows_per_vec, int nvec,
                             size_t vec_stride, void* stream);
/* dit.py:250 (A operand of the hoisted input projection): [2][B][seq_len][128 + dt] 16-bit operands = [cond, zero padded to 128 | text_emb];
 * branch 0: cond where n < lens[b] (step_cond, cfm.py:331), branch 1: cond dropped (dit.py:249) unless null_keeps_cond;
 * cond [B][seq_len][mel_dim <= 128], text_emb [2][B][seq_len][dt] */
int f5_op_pack_cond_text(const float* cond, const int32_t* lens, const float* text_emb, void* out_hi, void* out_lo, int B, int seq_len,
                         int mel_dim, int dt, int null_keeps_cond, void* stream);
/* dit.py:250, the x part: y [rows][mel_dim <= 128] fp32 -> 16-bit operands [rows][128], zero padded */
int f5_op_pack_x(const float* y, void* out_hi, void* out_lo, int rows, int mel_dim, void* stream);
/* cfm.py:395-397: out = where(n < lens[b], cond, y), all [B][seq_len][mel_dim] */
int f5_op_splice(const float* cond, const float* y, const int32_t* lens, float* out, int B, int seq_len, int mel_dim, void* stream);
/* The keep-mask twins of the two ops above (f5_sample_edit): keep dev uint8 [B][seq_len], non-zero = conditioning frame, in place of
 * n < lens[b].  pack_cond_text_keep generalises step_cond = where(cond_mask, cond, 0) (cfm.py:331) to the interior spans the training
 * forward masks (cfm.py:198-224): branch 0 takes cond[b][n] where keep[b][n] != 0 and zeros elsewhere, branch 1 the same when
 * null_keeps_cond is set; 16-bit split, saturation report, text columns and both operand types as f5_op_pack_cond_text.  splice_keep
 * generalises cfm.py:395-397: out = keep ? cond : y.  Both SELECT by the test: the side that is not taken is not loaded, so a NaN in a
 * dropped conditioning frame does not reach the output.  Refused before a launch: null pointers (out_lo may be NULL), sizes < 1. */
int f5_op_pack_cond_text_keep(const float* cond, const uint8_t* keep, const float* text_emb, void* out_hi, void* out_lo, int B,
                              int seq_len, int mel_dim, int dt, int null_keeps_cond, void* stream);
int f5_op_splice_keep(const float* cond, const float* y, const uint8_t* keep, float* out, int B, int seq_len, int mel_dim, void* stream);
/* The three-branch operand of dual guidance: [3][B][seq_len][128 + dt] in the order F, N, T.  Branches 0 and 1 are what
 * f5_op_pack_cond_text (or its keep twin) writes with null_keeps_cond = 0; branch 2 has zero cond columns and BRANCH 0's text columns
 * (text_emb stays [2][B][seq_len][dt]).  Split, saturation report, operand types and selection as there. */
int f5_op_pack_cond_text_dual(const float* cond, const int32_t* lens, const float* text_emb, void* out_hi, void* out_lo, int B, int seq_len,
                              int mel_dim, int dt, void* stream);
int f5_op_pack_cond_text_dual_keep(const float* cond, const uint8_t* keep, const float* text_emb, void* out_hi, void* out_lo, int B,
                                   int seq_len, int mel_dim, int dt, void* stream);
/* Frame gather (no reference counterpart; the layout step of speech editing): src dev [B][n_src][mel_dim] fp32, src_idx dev int32
 * [B][seq_len] -> cond_out dev [B][seq_len][mel_dim], keep_out dev uint8 [B][seq_len].  An index in [0, n_src) copies that frame of the
 * same row and sets keep to 1; any other index (-1 is the documented "regenerate here") writes zeros and keep 0 and reads nothing.
 * One launch lays out an edited utterance: kept stretches shifted, replaced spans resized (f5_tts_mlx_amd/edit.py edit_layout builds
 * the map). */
int f5_op_gather_frames(const float* src, const int32_t* src_idx, float* cond_out, uint8_t* keep_out, int B, int n_src, int seq_len,
                        int mel_dim, void* stream);
/* lens_to_mask of the durations (utils.py:39, cfm.py:334): keep[b][n] = n < dur[b] */
int f5_op_rowkeep(const int32_t* dur, uint8_t* keep, int nbatch, int seq_len, void* stream);
/* the staging kernels sample() uses in place of mx.array(...) / copies: device -> device copy of nwords 32-bit words (4-byte aligned
 * pointers; 16-byte accesses when both allow it), host words -> device through kernel arguments */
int f5_op_copy_words(const void* src, void* dst, size_t nwords, void* stream);
int f5_op_stage_words(const uint32_t* host_words, size_t nwords, uint32_t* dst, void* stream);
/* V^T [rows][npad] 16-bit operands: zeroes the pad columns [seq_len, npad) (no reference line: the reference has no padded V^T) */
int f5_op_zero_vt_pad(void* vt, size_t rows, int seq_len, int npad, void* stream);

/* Initial noise of F5TTS.sample (cfm.py:369-375) on the device: for each batch element the channel-major draw
 * `mx.random.seed(seed); mx.random.normal((mel, dur))`, zero padded to N frames, laid out [B][N][mel].  The generator follows
 * the published MLX algorithm as restated in f5_tts_mlx_amd/rng.py (threefry2x32 key split and counters: bit-exact integer path;
 * float32 uniform mapping step by step; sqrt(2) * erfinv in float64, one final rounding) -- unverifiable against MLX itself here.
 * seeds: one per element (the reference uses the same seed for all); durations: host; scratch_words: >= 3 * B device words. */
int f5_noise_normal(const uint64_t* seeds, int B, const int32_t* durations, int N, int mel, float* y0, void* scratch_words,
                    void* stream);
/* the float path of f5_noise_normal alone, for the tests: out[i] = the normal value the generator maps the 32 random bits
 * bits_dev[i] to (f5_tts_mlx_amd/rng.py bits_to_normal), n values, both pointers on the device */
int f5_op_noise_from_bits(const uint32_t* bits_dev, size_t n, float* out, void* stream);

/* x += gate[col] * ((A W^T + bias) * keep[row])  (dit.py:319,323; also Vocos' layer-scale + residual) */
int f5_op_gemm_resid_gate(const void* a_hi, const void* a_lo, const void* w_hi, const void* w_lo, const float* bias,
                          const float* gate, const uint8_t* rowkeep, float* x, int M, int N, int K, int lda, int ldw, int ldx,
                          int nseg, void* stream);
/* the same with the LN-modulate that follows it in a DiT block (dit.py:321 after :319; the next block's dit.py:270 after :323)
 * fused into the launch: h = LN(x_new) * (1 + ln_scale) + ln_shift, bit-identical to f5_op_gemm_resid_gate followed by
 * f5_op_ln_modulate.  Small-tile shapes only (batch-1-sized M; an error otherwise); N = 256 / 512 / 768 / 1024, x is [M][N];
 * counters: >= ceil(M / 64) ints, zero on entry, zero again on exit. */
int f5_op_gemm_resid_gate_ln(const void* a_hi, const void* a_lo, const void* w_hi, const void* w_lo, const float* bias,
                             const float* gate, const uint8_t* rowkeep, float* x, const float* ln_scale, const float* ln_shift,
                             void* h_hi, void* h_lo, int* counters, int M, int N, int K, int lda, int ldw, int nseg, void* stream);
/* out_f32 = A[row % a_row_mod] W^T + addrows[row]; (out_hi, out_lo) = the same as 16-bit operands: the split input projection of
 * InputEmbedding (dit.py:250), x part per step + hoisted cond / text part, x rows shared by the two CFG branches */
int f5_op_gemm_addrows(const void* a_hi, const void* a_lo, const void* w_hi, const void* w_lo, const float* addrows,
                       int a_row_mod, float* out_f32, void* out_hi, void* out_lo, int M, int N, int K, int lda, int ldw, int ldo,
                       int nseg, void* stream);
/* nn.LayerNorm with affine parameters, eps 1e-6; fp32 and/or bf16 (hi, lo) outputs (any may be NULL) */
int f5_op_layernorm(const float* x, const float* w, const float* b, float* out_f32, void* out_hi, void* out_lo, int rows,
                    int dim, void* stream);
/* im2col for Conv1d(k=7, pad=3), channels-last input with <= 128 channels -> bf16 [rows][7*128] */
int f5_op_im2col7(const float* x, void* out_hi, void* out_lo, int nbatch, int seq_len, int channels, void* stream);
/* Vocos ISTFT head (vocos_mlx Vocos.decode tail, cfm.py:399-400): x [nframes][ldx>=1026] (log-mag | phase) ->
 * wave [hop*(nframes-1)]; frames_scratch [nframes][1024] */
int f5_op_istft(const float* x, int ldx, const float* window, float* frames_scratch, float* wave, int nframes, int n_fft,
                int hop, void* stream);

/* host-side float <-> 16-bit operand conversions used by f5_load_tensor (exported for the CPU tests): fp16 / bf16 round to
 * nearest even; fp16 saturates at +-65504 instead of overflowing to inf */
uint16_t f5_debug_f2h_bits(float f);
float f5_debug_h_bits2f(uint16_t h);
uint16_t f5_debug_f2bf_bits(float f);
/* ---- test hooks.  Process-wide (set them once, before the calls they should affect); they choose among kernels that sample()
 * itself reaches by shape, so that small test shapes can exercise every shipped tile path. */
/* force the GEMM block tile: 0 auto, 1 = 128x128, 2 = 64x128, 3 = 64x64 (register-staged), 4 = 256x256 (gemm256.hip), 5 / 6 = ring
 * 64x128 / 64x64, 8 / 9 = 8-wave ring 128x192 / 128x128, 10 / 11 = in-workgroup split-K 64x128 / 128x128, 12 / 13 = 8-wave ring
 * 128x256 with 64x64 / 32x128 wave tiles, 14 = role-split 128x256 (gemm_rs128.hip).  What a selector means for a given launch --
 * which shapes and epilogues fall back to the automatic choice -- is written once, in csrc/gemm_route.hpp f5_gemm_route. */
int f5_debug_set_gemm_tile(int sel);
/* which kernel did it run?  Copies (at most n - 1 characters + NUL) a short stable name of the kernel the most recent GEMM launch of
 * the process resolved to and returns the name's length: family plus the template parameters that tell instantiations apart --
 * cfg<2,2> / cfg<1,2> / cfg<1,1> (register-staged), ring<1,2> / ring<1,1>, ring8<3> / ring8<2> (+fold_consumer), ring_ks2<1> (+fold_producer)
 * / ring_ks2<2>, ring_wide<2,2,2,4> / ring_wide<1,4,4,2>, gemm256 and rs128 (+qk_tr, +fold_rowf / +fold_stats).  "" after a launch that
 * was refused.  Host side only: nothing reaches a kernel.  The operand type is f5_op_get_operand_type's. */
int f5_debug_last_gemm_kernel(char* buf, int n);
/* the same for attention: the instantiation the most recent attention launch of the process resolved to -- f5_attn2_kernel<true,0> /
 * <false,0>, f5_attn2f_kernel<true> / <false>, f5_attn2p_kernel, f5_attn2s_kernel<true,2,2> / <false,2,3,true> / <false,4,2,true> --
 * with "+f8" appended when the launch carried the MX-fp8 output; "" after a launch that was refused.  Host side only. */
int f5_debug_last_attn_kernel(char* buf, int n);
/* the same for the conv-pos kernel: the instantiation the most recent conv-pos launch of the process resolved to --
 * f5_convpos_kernel<false,1> / <false,2> / <false,4> / <true,1> / <true,2> (",48" inside the brackets for the 48-channels-per-group
 * instantiation: f5_convpos_kernel<false,1,48>) -- with "+xcd" appended when the 1-D "groups dealt to XCDs"
 * block numbering ran; "" after a launch that was refused.  Host side only: nothing reaches a kernel.  The operand type is
 * f5_op_get_operand_type's. */
int f5_debug_last_convpos_kernel(char* buf, int n);
/* which conv-pos kernel WOULD a launch of this shape run under the current selectors?  The launcher's own decision, in the names of
 * f5_debug_last_convpos_kernel (f5_convpos_ring_kernel among them); nothing is launched and no device is touched. */
int f5_debug_convpos_route(int B, int seq_len, int groups, int nseg, char* buf, int n);
/* the same for `groups` groups of cpg = 32, 48 or 64 channels each: narrow groups never run f5_convpos_ring_kernel */
int f5_debug_convpos_route_groups(int B, int seq_len, int groups, int cpg, int nseg, char* buf, int n);
/* which kernel WOULD it run?  The same routing function the launcher switches over (csrc/gemm_route.hpp), asked for a launch of this
 * epilogue and shape under the current selectors (f5_debug_set_gemm_tile / _ring / _qkv_tile) and process-wide flags; nothing is
 * launched and no device is touched.  variant_bits: 1 = group-major rotation tables set (transposed q / k tiles), 2 = fused LN tail,
 * 4 = LN-fold producer, 8 = LN-fold consumer in the statistics form, 16 = LN-fold consumer with row factors.  Copies the name
 * f5_debug_last_gemm_kernel would report after the launch and returns its length, or a negative value when the launch would be refused
 * (f5_last_error says why).  facts (may be NULL): bit 0 = staged multi-round kernel, bit 1 = single-round LN-fold launch, bit 2 = an
 * EPI_RESID_GATE launch of this shape with ldo == N can carry the fused LN tail -- what the engine plans the LN fold with. */
int f5_debug_gemm_route(int epi, int M, int N, int nseg, int seq_len, int variant_bits, int debug_flags, char* name, int n, int* facts);
/* GEMM flag bits, OR-ed into every GEMM launch of the process (an engine's own: f5_engine_set_option "gemm_flags"):
 * bit 0: skip the epilogue of the 256x256 kernel (timing only; results are garbage);
 * bit 1: small-tile kernels use the direct (2-byte store) epilogue instead of the LDS-staged one;
 * bit 3 (8): routes the residual update exactly like bit 8 (the two are tested together);
 * bit 8 (256): the small-tile ring kernels load x / bias / gate / keep of the residual update in the epilogue instead of
 *            requesting them before the K loop (A/B of the default; identical bits);
 * bit 12 (4096): the role-split 128x256 kernel numbers its tiles as an XCD-chunked list (M fastest) instead of dealing a 2 x 4
 *            grid of tile blocks to the XCDs (A/B of the default; identical bits);
 * bit 14 (16384): the 256x256 kernel accumulates 16-bit-output tiles (FF1, plain 16-bit, q / k of QKV) in the straight order with
 *            2-byte staging writes instead of transposed with 8-byte ones (A/B; identical bits for FF1 / plain);
 * bits 4-7 and 9-11 are read nowhere. */
int f5_debug_set_gemm_flags(int v);
/* ring GEMM tile numbering: 0 auto (band-major one-round launches whose A fits an L2, else m / n fastest), 1 n fastest, 2 m fastest,
 * 3 band-major (bands of 4 column tiles) wherever the tile grid allows */
int f5_debug_set_gemm_order(int v);
/* small-tile GEMM staging: 1 = global_load_lds ring (default), 0 = register-staged double buffer */
int f5_debug_set_gemm_ring(int v);
int f5_debug_set_gemm_qkv_tile(int sel);    /* small-M QKV projection with pair-major tables: 0 = auto (role-split 128x256 tiles when one round of >= 176), 1 = small tiles, 12 / 13 = lock-step 8-wave 128x256 ring, 14 = role-split whenever one round */
int f5_debug_set_gemm_nband(int n);         /* 256x256 GEMM: tiles numbered in bands of n column tiles (0 = n fastest) */
/* conv-pos kernel: weight slabs per pipeline step, 0 = auto, 1 / 2 / 4, or 8 = the ring kernel f5_convpos_ring_kernel, weight slabs by LDS-DMA
 * into a deep ring, for every one-pass launch.  Auto is 1 slab per step, except that one-pass launches of one round (at most 256 workgroups)
 * with seq_len >= 512 and the groups dealt to XCDs run the ring kernel.  The one-pass kernel (nseg 1) is built for 1 / 2 / 4; the
 * three-pass kernel (nseg 3) for 1 and 2 only: with nseg == 3 a selector of 2, 4 or 8 runs f5_convpos_kernel<true,2>
 * (f5_debug_last_convpos_kernel says which instantiation a launch ran) */
int f5_debug_set_convpos_tps(int taps);
int f5_debug_set_convpos_xcd_map(int on);   /* conv-pos kernel: 1 (default) = groups dealt to XCDs, 0 = plain 3-D block numbering */
/* 256-query attention workgroups with two query blocks per wave (one-pass modes, large grids): -1 auto, 0 off, 1 force */
int f5_debug_set_attn_wide(int v);
/* in-workgroup KV split of the attention kernel: -1 auto (by grid size), 1 none, 2 / 4 wave groups */
int f5_debug_set_attn_kvsplit(int v);
/* large-grid attention kernel (q pre-multiplied): 1 = in-wave software-pipelined kernel, one wave per SIMD (v2p), 0 = v2f */
int f5_debug_set_attn_pipe(int v);
/* process DEFAULTS of the per-engine options (f5_engine_set_option); engines that already exist keep their own values */
int f5_debug_set_ln_fusion(int on);         /* 1: LN-modulate fused behind the residual GEMMs of small-M launches (default 0: measured slower) */
int f5_debug_set_qkv_transposed(int on);    /* 1 (default): sample() hands the pair-major rotation tables to the QKV projection (256x256 kernel: transposed q / k tiles) */
int f5_debug_set_q_premul(int on);          /* 1 (default): sample() multiplies q by softmax_scale * log2(e) in the QKV epilogue (single-segment operand modes) */
/* LN-modulate folded into the GEMMs around it (dit.py:270 / :321 between the residual updates :319 / :323 and the projections;
 * csrc/gemm.hpp fold_*; engine option "ln_fold"), for any per-row shift m:
 *   (LN(x)(1 + s) + b) W^T + bias = rstd (((x - m)(1 + s)) W^T) - rstd (mean - m) c1 + c2.
 * Op-level twins: with a producer set, f5_op_gemm_resid_gate also writes (x - row_shift)(1 + next_scale) as [M][N] 16-bit operands and
 * the slice statistics [N / 64][M][2] (slice-major: sum of d = x - row_shift over the slice's 64 columns, sum of squares about the
 * slice mean); row_shift [M] or NULL = 0.  f5_op_fold_rows merges those into the row factors [M][2] = (rstd, rstd * (mean - m)),
 * eps 1e-6; its row_shift (NULL = 0) is m on entry and the row's mean on exit (the next producer's shift).  f5_debug_set_op_ln_mean_out:
 * f5_op_ln_modulate also writes the row means [rows] (the first shift of a forward).  With a consumer set, f5_op_gemm (epi 2) and
 * f5_op_qkv_rope take the operands as A and finish the LN in their epilogues (bias ignored: it is inside c2).  Shapes must run on the
 * 256x256 / role-split 128x256 kernels.  NULLs = off. */
int f5_debug_set_op_fold_producer(const float* next_scale, void* x16_out, float* stats_out, const float* row_shift);
int f5_op_fold_rows(const float* stats, int nslice, int M, float* rowf, float* row_shift, void* stream);
int f5_debug_set_op_ln_mean_out(float* mean_out);
int f5_debug_set_op_fold_consumer(const float* rowf, const float* c1, const float* c2);
/* the statistics form of the consumer (round 6): with rowf = NULL above, f5_op_gemm (epi 2) / f5_op_qkv_rope merge the producer's slice
 * statistics (its stats_out, [16][ld][2]; K = 1024) into their rows' factors themselves -- no f5_op_fold_rows launch in between; shift = the
 * producer's row_shift on ENTRY (or NULL = 0); mean_out (or NULL) receives the rows' means from the workgroups of column tile 0 and must
 * not alias shift.  NULL stats = off. */
int f5_debug_set_op_fold_stats(const float* stats, int ld, const float* shift, float* mean_out);
int f5_debug_set_op_sat_flag(int* flag);   /* device word the 16-bit packers of the f5_op_* launches that follow OR F5_STATUS_SATURATED into (fp16 operand type); NULL = off */
int f5_debug_set_op_fold_overflow_flag(int* flag);   /* device word the producer ORs bit 0 into when (x - m)(1 + s) leaves the fp16 range; NULL = off */
/* c1[v][n] = sum_k W[n][k] (1 + scale_v[k]), c2[v][n] = sum_k W[n][k] shift_v[k] + bias[n] for nvec modulation vectors (vec_stride
 * floats apart; result rows out_stride floats apart); K % 256 == 0, K <= 2048 */
int f5_op_fold_consts(const void* w_hi, int ldw, const float* bias, const float* scale, const float* shift, size_t vec_stride, int nvec,
                      float* c1, float* c2, size_t out_stride, int N, int K, void* stream);
/* op-level twins for f5_op_qkv_rope / f5_op_attention */
int f5_debug_set_op_rope_tables_g4(const float* tq, const float* tk); /* NULLs = off */
int f5_debug_set_op_q_premul(float factor); /* f5_op_qkv_rope scales q by factor, f5_op_attention expects q pre-scaled; 0 = off (default) */

/* ---- MX-fp8 path (BASELINE configs[4]; gfx950 v_mfma_scale_f32_32x32x64_f8f6f4): OCP e4m3 elements, one E8M0 scale per 32
 * consecutive K elements (scale = 2^ceil(log2(amax/448))).  No reference counterpart (the reference's reduced-precision mode
 * is MLX int4/int8 weight quantisation, cfm.py:510-515). ---------------------------------------------------------------- */
/* rows of fp32 [rows][ldx] -> e4m3 [rows][ldq] + E8M0 [rows][cols/32] (dense); cols % 32 == 0, ldx % 4 == 0, ldq % 4 == 0, both
 * >= cols; x 16-byte aligned, q 4-byte aligned.  Finite inputs. */
int f5_op_quantize_mx(const float* x, int ldx, void* q, int ldq, void* scales, int rows, int cols, void* stream);
/* the same from 16-bit rows of the operand type of f5_op_set_operand_type (bf16 or fp16; what quantises the weights of the mode from
 * their 16-bit copies); x16 8-byte aligned */
int f5_op_quantize_mx_bf16(const void* x16, int ldx, void* q, int ldq, void* scales, int rows, int cols, void* stream);
/* (q, q_scales) = MX-fp8(LN(x) (1 + scale) + shift): x fp32 [rows][dim] dense, q e4m3 [rows][dim], q_scales E8M0 [rows][dim/32];
 * dim 256 / 512 / 768 / 1024; x / scale / shift 16-byte aligned, q 4-byte aligned.  The A operand of the QKV and FF1 GEMMs of an
 * mxfp8 block (dit.py:270 with the MX rounding of oracle/mx_oracle.py behind it). */
int f5_op_ln_modulate_f8(const float* x, const float* scale, const float* shift, void* q, void* q_scales, int rows, int dim, float eps,
                         void* stream);
/* C = A W^T on MX-fp8 operands.  epi 0: out_f32 = acc + bias; 1: out_bf = bf16(acc + bias);
 * 2: (out8, out8_scales) = MX-fp8(gelu_tanh(acc + bias)); 4: out_f32 += gate * ((acc + bias) * keep[row]) (rowkeep NULL = all 1).
 * Shapes: N % 256 == 0, K % 128 == 0, any M >= 1.  a8 [M][lda8] and w8 [N][ldw8] (exactly N rows are read, in whole 256-row tiles):
 * lda8 / ldw8 multiples of 16 and >= K, both pointers 16-byte aligned (the rows are staged with 16-byte LDS-direct loads); a_scales
 * [M][K/32] and w_scales [N][K/32] dense, 4-byte aligned.
 * `ldo` is the leading dimension of whichever output the epilogue writes, >= N, and the launcher refuses what the row stores of the
 * epilogue cannot take:
 *   epi 0  out_f32, element stores: no further rule;
 *   epi 1  out_bf, 16-byte stores: ldo % 8 == 0, out_bf 16-byte aligned;
 *   epi 2  out8, 8-byte stores: ldo % 8 == 0, out8 8-byte aligned; out8_scales is dense [M][N/32] -- it has NO leading dimension;
 *   epi 4  out_f32 and gate, 16-byte accesses: ldo % 4 == 0, out_f32 and gate 16-byte aligned.
 * Operand type: the MX-fp8 mode exists in the bf16 build of the kernels only.  epi 1 writes bf16 (one round-to-nearest-even of the fp32
 * value) whatever f5_op_set_operand_type says, and so does f5_op_qkv_rope_f8. */
int f5_op_gemm_f8(const void* a8, const void* a_scales, const void* w8, const void* w_scales, const float* bias,
                  const float* gate, const uint8_t* rowkeep, float* out_f32, void* out_bf, void* out8, void* out8_scales,
                  int M, int N, int K, int lda8, int ldw8, int ldo, int epi, void* stream);
/* the QKV projection of an mxfp8 block (what f5_op_qkv_rope is to the 16-bit modes): M = B seq_len rows, N = 3 dmodel, K = dmodel,
 * heads * 64 == dmodel, dmodel % 128 == 0 (and % 256 through N); qk bf16 [M][2 dmodel] dense, 16-byte aligned (rotated q | k, q times
 * q_premul when that is non-zero); vt bf16 [B heads 64][npad], V transposed, columns seq_len ... npad - 1 are not written;
 * rope_cos / rope_sin [seq_len][32] (f5_op_rope_table, dim_head 64); B > 1 needs seq_len >= 4.  Operands as for f5_op_gemm_f8. */
int f5_op_qkv_rope_f8(const void* a8, const void* a_scales, const void* w8, const void* w_scales, const float* bias, const float* rope_cos,
                      const float* rope_sin, void* qk, void* vt, int B, int seq_len, int npad, int heads, int dmodel, int lda8, int ldw8,
                      float q_premul, void* stream);

/* ---- audio front-end (audio.py:115-230) ---------------------------------------------------------- */
/* log-mel spectrogram (audio.py:162-210: zero centre padding, periodic Hann, |rfft|, HTK filterbank, log(max(., 1e-5))) of a
 * batch of equally long waveforms in ONE launch: wave dev [B][L] fp32 -> out dev [B][L / hop][n_mels].  The reference loops
 * over the batch in Python (audio.py:195). */
int f5_mel_spectrogram_batch(const float* wave, int B, int64_t L, const float* window, const float* filterbank, int n_fft, int hop,
                             int n_mels, float* out, void* stream);
/* the same for one waveform: wave dev [L] -> out dev [L / hop][n_mels] */
int f5_mel_spectrogram(const float* wave, int64_t L, const float* window, const float* filterbank, int n_fft, int hop,
                       int n_mels, float* out, void* stream);
/* The same for a padded batch of recordings of DIFFERENT lengths, in one launch (no reference counterpart: the reference's sample()
 * takes a raw wave for batch 1 only, cfm.py:283-286).  wave dev [B][L]; begin_dev, lens_dev dev int32 [B]; gain_dev dev fp32 [B] or
 * NULL; out dev [B][N][n_mels].  Row b is the recording wave[b][begin[b] .. begin[b] + lens[b]) and has F_b = lens[b] / hop frames.
 *   - frame n < F_b: the bits f5_mel_spectrogram gives for a contiguous copy of that slice with every sample multiplied by gain[b]
 *     first (the product is rounded once to fp32, then multiplied by the window; gain_dev == NULL: no multiplication at all).  The
 *     two kernels share the frame body as one device function.  Samples outside the slice count as zero by the index test and are
 *     not loaded (NaN there stays out);
 *   - frame F_b <= n < N: exactly 0.0f in every band -- the zero padding sample() gives the conditioning (cfm.py:321), not log(1e-5).
 * Refused before a launch: what f5_mel_spectrogram_batch refuses (a null pointer other than gain_dev, n_fft != 1024, hop / n_mels < 1,
 * B outside 1 .. 65 535), N < 1, L outside 0 .. 2^31 - 1.  begin[b] / lens[b] outside the row are clamped in the kernel (begin to
 * 0 .. L, lens to 0 .. L - begin): wrong results, no access outside the buffers -- the convention of the ragged vocoder ops.  Rows with
 * F_b > N lose their frames past N: the lengths live on the device, the caller checks them (audio.py log_mel_spectrogram_ragged). */
int f5_mel_spectrogram_ragged(const float* wave, int B, int64_t L, const int32_t* begin_dev, const int32_t* lens_dev,
                              const float* gain_dev /* may be NULL */, const float* window, const float* filterbank, int n_fft, int hop,
                              int n_mels, float* out, int N, void* stream);
/* Block energies of a padded batch of recordings (no reference counterpart; the silence window and the RMS gain of
 * audio.py prepare_references are host arithmetic on this table): wave dev [B][L], lens_dev dev int32 [B], energy dev [B][nblk],
 * nblk = ceil(L / block).  energy[b][k] = sum of wave[b][s]^2 over s in [k block, min((k + 1) block, lens[b])); an empty range gives
 * exactly 0.0f.  A sample at s >= lens[b] is never loaded: the value is selected by the index test, never multiplied by a mask, so NaN
 * in the padding stays out.
 * Summation order (fixed: it depends on `block` and on the position inside the block only, so row b of a batch has the bits of the
 * same call on that row alone): one 64-lane wave per block; lane l accumulates the block's samples l, l + 64, l + 128, ... in
 * increasing order with acc = fmaf(x, x, acc) from acc = 0; the 64 lane sums are combined by an xor butterfly,
 * v = v + shfl_xor(v, d) for d = 32, 16, 8, 4, 2, 1.
 * Refused on the host before any launch, each with its own message: a null pointer; B outside 1 .. 65 535; block outside 1 .. 4096;
 * L outside 0 .. 2^31 - 1; nblk != ceil(L / block).  L = 0 is a successful call without a launch.  lens[b] outside 0 .. L is clamped in
 * the kernel (wrong results, no access outside the buffers). */
int f5_wave_block_energy(const float* wave, int B, int64_t L, const int32_t* lens_dev, int block, float* energy, int nblk,
                         void* stream);
/* Sample-rate conversion of a batch of equally long waveforms in ONE launch (no reference counterpart: generate.py:147-148 refuses
 * anything but 24 kHz): wave dev [B][L] fp32 -> out dev [B][L_out], L_out = ceil(n L / o).  A Hann-windowed sinc polyphase filter, the
 * design of torchaudio's default `resample`.  With g = gcd(orig, new), o = orig / g, n = new / g, base = 0.99 min(o, n),
 * width = ceil(6 o / base):  out[j n + i] = sum_k h[i][k] x[j o + k - width]  (x = 0 outside [0, L)),  k = 0 .. 2 width + o - 1,
 *   h[i][k] = sinc(pi t) cos^2(pi t / 12) base / o,  t = (-i / n + (k - width) / o) base,  0 where |t| >= 6,
 * computed in fp64 and rounded once to fp32.  The caller hands over the compact table (audio.py resample_table builds it):
 *   first dev [n] int32:  index k of the first non-zero tap of phase i
 *   taps  dev [T][n] fp32: taps[t][i] = h[i][first[i] + t], T = longest non-zero run of a phase, shorter runs zero padded
 * (at most 2 width + 1 taps of a phase are non-zero: T = 25 for 48 kHz -> 24 kHz, 13 of 161 for 11 025 Hz -> 24 kHz).  fp32 FMAs in
 * tap order; B = 1 .. 65 535; L = 0 is a successful call without a launch.
 * Ratio limit: a workgroup stages the input span of 1024 consecutive outputs in 8192 floats of LDS, so the call refuses (no launch)
 * unless  (1023 / n + 1) o + 2 width + o + T - 1 <= 8192  (integer division) -- with the table above, down-sampling by up to 7:1 (8:1 is
 * refused), a little less when o is large: 48 kHz -> 8 kHz (6:1), 44.1 kHz -> 8 kHz (441:80) and every pair between
 * 8 / 11.025 / 16 / 22.05 / 24 / 32 / 44.1 / 48 kHz and 24 kHz pass.  Rates whose gcd is small are refused whatever the ratio (o near
 * 3 500 and beyond: the span holds two groups of o samples).  Also refused: null pointers, o / n / T / width < 1, gcd(o, n) != 1, T > 2 width + o, L < 0, L_out != ceil(n L / o). */
int f5_resample_batch(const float* wave, int B, int64_t L, const float* taps, const int32_t* first, int o, int n, int T, int width,
                      float* out, int64_t L_out, void* stream);

/* Waveform patch (no reference counterpart; the last step of speech editing): puts the original samples back outside the edited spans
 * of a vocoded edit result.  gen dev [B][L] (the vocoded result), src dev [B][Ls] (the source recording at the model's rate and scale),
 * out dev [B][L]; segs_host host int32 [B][S][3] = (dst_begin, dst_end, src_begin) in samples, src_begin = -1 for a regenerated
 * segment -- staged to the device through kernel arguments like f5_op_stage_words' words (no host buffer outlives the call, no
 * synchronisation); fade dev fp32 [F] (may be NULL when F = 0).  Per row the segments are sorted, contiguous from 0 and may be empty;
 * rows with fewer than S segments pad with empty ones.
 *   - inside a regenerated segment out = gen; past the last segment's end out = exactly 0.0f;
 *   - inside a kept segment out = src[src_begin + (s - dst_begin)] by selection: the source's own bits, not g + 1 (o - g);
 *   - the first F samples of a kept segment whose predecessor in the table is regenerated: out = g + fade[i] (o - g), ONE fused
 *     multiply-add on the fp32 difference o - g, i = s - dst_begin; the last F samples of one whose successor is regenerated: the same
 *     with i = dst_end - 1 - s.  (Predecessor / successor = the table entry before / after, whatever its length.)
 * The caller builds fade[i] = 0.5 (1 - cos(pi (i + 0.5) / F)) in fp64 and rounds once (f5_tts_mlx_amd/edit.py fade_table; the
 * convention of audio.py resample_table).  F = 0 is a plain piecewise copy.  Refused on the host before any launch, each with its own
 * message: null pointers; B < 1; S outside 1 .. 64; F < 0; L or Ls outside 0 .. 2^31 - 1; an unsorted or non-contiguous table; a
 * segment that ends beyond L; a kept segment whose source range leaves [0, Ls]; a kept segment shorter than the fades it must hold (F
 * with one regenerated neighbour, 2 F with two).  L = 0 is a successful call without a launch. */
int f5_op_wave_patch(const float* gen, const float* src, const int32_t* segs_host, const float* fade, float* out, int B, int64_t L,
                     int64_t Ls, int S, int F, void* stream);

/* Sentence join (no reference counterpart; the last step of generate() / generate_many() when edge trim, pauses or cross-fades between
 * sentences are asked for): ONE call lays Q output waves out from R decoded rows.  src dev [R][Ls] (the decoded rows), out dev [Q][Lout];
 * segs_host host int32 [Q][S][6] = (dst_begin, src_row, src_begin, len, fade_in, fade_out) in samples -- staged to the device through
 * kernel arguments like f5_op_wave_patch's table, in chunks of output rows when it does not fit one launch (160 segments per launch;
 * no host buffer outlives the call, no synchronisation).  A row with fewer than S segments pads with len = 0 entries; an empty entry
 * covers nothing and takes no part in the order.  Segment k of row q covers out[q][dst_begin .. dst_begin + len) =: [d0, d1).
 * Fade weight: w(i, F) = (float)(2 i + 1) / (float)(2 F), ONE correctly rounded fp32 division of two exactly representable integers
 * (a linear fade, as in the PyTorch F5-TTS infer_process; no table is handed over, so every join has its own length).  out[q][s]:
 *   - covered by no segment (between segments, or past the last one): exactly +0.0f;
 *   - covered by one segment, outside its fades: src[src_row][src_begin + s - d0] by selection: the source's own bits, not 1.0f * x;
 *   - in the first fade_in samples of a segment, not overlapped: w(i, fade_in) * x, i = s - d0, one fp32 multiplication;
 *   - in the last fade_out samples of a segment, not overlapped: w(j, fade_out) * x, j = d1 - 1 - s, one fp32 multiplication;
 *   - covered by segment k (value a) and the next non-empty segment k' (value b): fmaf(w(i, F), b - a, a), i = s - d0[k'] -- ONE fused
 *     multiply-add on the fp32 difference, the form of f5_op_wave_patch.  Allowed only as a pure cross-fade: fade_out[k] ==
 *     fade_in[k'] == F and the overlap is exactly those F samples.  w(F - 1 - i, F) = 1 - w(i, F) in the reals: a constant-gain
 *     cross-fade, each output a convex combination of two samples.
 * A source sample outside the ranges the table names is never loaded (selected by the index tests, never multiplied by a mask): NaN in
 * the padding of src stays out of out.
 * Refused on the host before any launch, each with its own message: null pointers; R or Q outside 1 .. 65 535; S outside 1 .. 64; Ls or
 * Lout outside 0 .. 2^31 - 1; a negative field; src_row >= R; a source range that leaves [0, Ls]; a fade longer than 2^22 (beyond it
 * 2 i + 1 and 2 F are no longer exact in fp32); fade_in + fade_out > len; non-empty segments of a row not sorted by dst_begin; a
 * segment that ends beyond Lout; an overlap that is not the pure cross-fade above (with fade_in + fade_out <= len this also rules out
 * three segments covering one sample).  Lout = 0 is a successful call without a launch. */
int f5_wave_join(const float* src, int R, int64_t Ls, const int32_t* segs_host, int Q, int S, float* out, int64_t Lout, void* stream);

/* ---- vocoder: Vocos mel-24khz behind one call (replaces `self._vocoder(out)`, cfm.py:399-400; wiring cfm.py:446,471) ---------
 * The reference delegates to the third-party `vocos_mlx` package (not in its repository); this is the published Vocos
 * architecture (ConvNeXt backbone + ISTFT head) on the same kernels as the DiT.  Same ownership rules as the engine: the caller
 * allocates the weights arena and the workspace; tensors are loaded by their upstream state-dict names
 * ("backbone.embed.weight", "backbone.convnext.0.pwconv1.weight", ..., "head.out.bias"), conv weights in the PyTorch (out, in, k)
 * or the MLX (out, k, in) layout.  PARITY UNPINNED against vocos_mlx (no vector, no checkpoint reachable offline). */
typedef struct f5_vocoder f5_vocoder;
typedef struct f5_vocos_config {
    int32_t n_mels;            /* 100 */
    int32_t dim;               /* 512 */
    int32_t intermediate_dim;  /* 1536 */
    int32_t num_layers;        /* 8 */
    int32_t n_fft;             /* 1024 (only value supported) */
    int32_t hop_length;        /* 256 */
} f5_vocos_config;
int f5_vocoder_create(const f5_vocos_config* cfg, int precision, f5_vocoder** out);   /* F5_PREC_BF16 / _BF16X3 / _F16 */
void f5_vocoder_destroy(f5_vocoder* v);
int f5_vocoder_weights_bytes(f5_vocoder* v, size_t* bytes);
int f5_vocoder_set_weights_arena(f5_vocoder* v, void* dev_arena, size_t bytes, void* stream);
int f5_vocoder_load_tensor(f5_vocoder* v, const char* name, const float* host_data, int ndim, const int64_t* shape);
int f5_vocoder_mark_weights_loaded(f5_vocoder* v);     /* arena content arrived by a broadcast */
int f5_vocoder_finalize(f5_vocoder* v, void* stream);
int f5_vocoder_workspace_bytes(f5_vocoder* v, int B, int N, size_t* bytes);
/* mel dev [B][N][n_mels] fp32 -> wave dev [B][hop * (N - 1)] fp32; use_graph != 0: captured per (B, N, workspace), <= 8 graphs kept */
int f5_vocode(f5_vocoder* v, const float* mel, int B, int N, float* wave, void* workspace, size_t workspace_bytes, int use_graph,
              void* stream);
/* Ragged batch (no reference counterpart: the reference vocodes the padded batch, cfm.py:399-400): row b of mel dev [B][N][n_mels]
 * is lens[b] frames long (host [B], 2 <= lens[b] <= N) and is decoded on those frames alone -- wave dev [B][hop * (N - 1)], row b =
 * what f5_vocode gives for mel[b][:lens[b]] by itself for hop * (lens[b] - 1) samples, exactly 0.0f beyond.  The launch sequence is
 * f5_vocode's with the three launches that mix time steps replaced by their ragged twins (below); the rest is row-wise.  `lens` is
 * staged into the workspace outside the captured part: one graph per (B, N, workspace, ragged) serves every set of lengths, and the
 * graphs of f5_vocode and of this call share the handle's 8 slots without replacing each other.  Refused before any launch, each
 * with its own message: a null pointer, B < 1, N < 2, a lens[b] outside 2 .. N, an unfinalised handle, a workspace that is too small
 * (f5_vocoder_workspace_bytes covers both calls) or not 256-byte aligned. */
int f5_vocode_ragged(f5_vocoder* v, const float* mel, const int32_t* lens, int B, int N, float* wave, void* workspace,
                     size_t workspace_bytes, int use_graph, void* stream);
int f5_vocoder_graph_count(f5_vocoder* v);   /* captured graphs the handle holds now (both calls) */
/* ISTFT head alone (per-op entry for tests): x dev [B * nframes][ldx >= n_fft + 2] (log-magnitude | phase) ->
 * wave dev [B][hop * (nframes - 1)]; frames_scratch dev [B * nframes][n_fft]; two launches for the whole batch */
int f5_op_istft_batch(const float* x, int ldx, const float* window, float* frames_scratch, float* wave, int B, int nframes,
                      int n_fft, int hop, void* stream);
/* The ragged twins of f5_op_im2col7, f5_op_dwconv_ln and f5_op_istft_batch: the same arguments plus lens_dev, dev int32 [nbatch] with
 * 2 <= lens_dev[b] <= seq_len (nframes); the buffers keep their padded shapes, rows seq_len apart.  Row b ends at lens_dev[b]:
 *   im2col7:   a tap at a frame >= lens[b] is zero, as a tap at a frame >= seq_len is in f5_op_im2col7, and an output row
 *              n >= lens[b] is all zeros; the value is selected by the index test, never multiplied by a mask, so nothing the
 *              padding holds (NaN included) is loaded;
 *   dwconv_ln: a tap at nn >= lens[b] is left out of the sum (FMA order t = 0 .. 6 as in f5_op_dwconv_ln); a token n >= lens[b]
 *              writes zeros to out_hi / out_lo and takes no part in the saturation report;
 *   istft:     the overlap-add of row b uses lens[b] frames in its last-frame clamp and its envelope, writes wave[b][s] for
 *              s < hop * (lens[b] - 1) and exactly 0.0f from there to hop * (nframes - 1); frames past lens[b] are not read.
 * A valid output is produced by the floating-point operations of the plain op run on that row's slice alone (nbatch = 1,
 * seq_len = lens[b]), in the same order: the same bits.  Refused before a launch: null pointers, nbatch < 1, seq_len < 2 and what
 * the plain ops refuse.  The kernels clamp a length outside the stated range to it: wrong results, no access outside the buffers. */
int f5_op_im2col7_ragged(const float* x, void* out_hi, void* out_lo, int nbatch, int seq_len, int channels, const int32_t* lens_dev,
                         void* stream);
int f5_op_dwconv_ln_ragged(const float* x, const float* dw_w, const float* dw_b, const float* ln_w, const float* ln_b, void* out_hi,
                           void* out_lo, int nbatch, int seq_len, int dim, const int32_t* lens_dev, void* stream);
int f5_op_istft_ragged(const float* x, int ldx, const float* window, float* frames_scratch, float* wave, int B, int nframes,
                       int n_fft, int hop, const int32_t* lens_dev, void* stream);

/* ---- duration predictor behind one call (replaces `self._duration_predictor(cond, text)` and the frame arithmetic of
 * F5TTS.predict_duration, cfm.py:253-262, :307-308; model: duration.py:97-260; wiring cfm.py:429-438) ---------------------------
 * DurationPredictor(DurationTransformer): TextEmbedding without padding mask (duration.py:116-118), Linear(mel + text -> dim) +
 * ConvPositionEmbedding (duration.py:44-58), `depth` pre-LN blocks with plain LayerNorm (duration.py:64-94), RMSNorm, masked mean,
 * Linear(dim -> 1) + Softplus = seconds (duration.py:137,188-190,249-251).  Same ownership rules as the engine and the vocoder: the
 * caller allocates the weights arena and the workspace.  Tensors are loaded by their reference (MLX-layout) names and shapes --
 * "transformer.text_embed.text_embed.weight", "transformer.transformer_blocks.3.attn.to_q.weight", "to_pred.layers.0.weight" ... --
 * with or without the "duration_predictor." prefix of an F5TTS checkpoint; the loader pads the matrices to 128 rows, lays
 * input_embed.proj out as [x padded to 128 | text] columns, stacks to_q / to_k / to_v and expands 32-channel conv-pos groups to the
 * block-diagonal 64-channel groups the kernel works on.  f5_duration_load_tensor checks name and shape before it needs the arena. */
typedef struct f5_duration f5_duration;
typedef struct f5_duration_config {       /* duration.py:97-158 */
    int32_t dim;               /* 512 */
    int32_t depth;             /* 8 */
    int32_t heads;             /* 8 */
    int32_t dim_head;          /* 64 (only 64 is supported by the attention kernel) */
    int32_t ff_dim;            /* dim * ff_mult = 1024 */
    int32_t mel_dim;           /* 100 (<= 128) */
    int32_t text_num_embeds;   /* 2545 (embedding table has +1 rows, duration.py:116) */
    int32_t text_dim;          /* 512 (a multiple of 256) */
    int32_t conv_layers;       /* 2 (>= 1) */
    int32_t conv_pos_kernel;   /* 31 */
    int32_t conv_pos_groups;   /* 16 (dim / groups must be 32 or 64) */
    int32_t text_max_pos;      /* 4096 */
} f5_duration_config;
int f5_duration_create(const f5_duration_config* cfg, int precision, f5_duration** out);   /* F5_PREC_BF16 / _BF16X3 / _F16; plans only, no device */
void f5_duration_destroy(f5_duration* d);   /* also destroys every cached hipGraphExec */
int f5_duration_weights_bytes(f5_duration* d, size_t* bytes);
int f5_duration_set_weights_arena(f5_duration* d, void* dev_arena, size_t bytes, void* stream);
int f5_duration_load_tensor(f5_duration* d, const char* name, const float* host_data, int ndim, const int64_t* shape);
int f5_duration_mark_weights_loaded(f5_duration* d);   /* arena content arrived by a broadcast */
int f5_duration_finalize(f5_duration* d, void* stream);   /* refuses a missing tensor by name, builds the text positional table (rope.py:63-73) */
/* N = max(n_in, nt) (duration.py:218-220); needs B >= 1, n_in >= 1, nt >= 1, 4 <= N <= text_max_pos */
int f5_duration_workspace_bytes(f5_duration* d, int B, int n_in, int nt, size_t* bytes);
typedef struct f5_duration_args {
    int32_t B;                 /* utterances                                                                 */
    int32_t n_in;              /* mel frames of the input                                                    */
    int32_t nt;                /* text columns                                                               */
    const float* mel;          /* dev  [B][n_in][mel_dim] (duration.py:203-206 turns a raw wave into this)   */
    const int32_t* text;       /* dev  [B][nt] token ids, -1 padded (utils.py:124-133)                       */
    const int32_t* lens;       /* host [B] (duration.py:222-226) or NULL = every row is N = max(n_in, nt) long */
    float frame_rate;          /* sample_rate // hop_length = 93 (cfm.py:260)                                */
    float speed;               /* cfm.py:261                                                                 */
    float* seconds;            /* dev  [B]                                                                   */
    int32_t* frames;           /* dev  [B] or NULL: (int32)(seconds * frame_rate / speed), an fp32 product, an fp32 division, truncation */
    void* workspace;           /* dev, f5_duration_workspace_bytes, 256-byte aligned                         */
    size_t workspace_bytes;
    int32_t use_graph;         /* != 0: the launch sequence is captured per (B, n_in, nt, workspace) -- and per entry point, f5_predict_duration / _rows -- and replayed, <= 8 graphs kept (LRU) */
} f5_duration_args;
/* mel / text / lens are staged into the workspace and seconds / frames copied out by kernels OUTSIDE the captured part: a replay
 * serves new inputs of the same shape.  The handle carries its own operand type: the process-wide one (f5_op_set_operand_type) is
 * neither read nor written.  Handles are not re-entrant. */
int f5_predict_duration(f5_duration* d, const f5_duration_args* args, void* stream);
/* Status word of the last f5_predict_duration on the workspace of `args` (the FIRST 32-bit word of the workspace, zeroed by every call):
 * F5_STATUS_SATURATED (precision f16) = a producer of a 16-bit MFMA operand -- the packed input, the text path, conv-pos, LayerNorm,
 * q / k / v, the GELU output -- clamped a value beyond +-65 504: the seconds are finite and wrong; use bf16x3 or bf16 for this input.
 * Synchronises `stream`.  No reference counterpart. */
int f5_duration_status(f5_duration* d, const f5_duration_args* args, int* flags, void* stream);
int f5_duration_graph_count(f5_duration* d);
/* Row-isolated prediction of a padded batch (docs/duration_rows.md; no reference counterpart).  f5_predict_duration runs every row at
 * N = max(n_in, nt): the text blocks' depthwise conv and GRN, both conv-pos layers and the attention (which has no key mask) read a
 * row's padding, so a row's seconds depend on its batch-mates.  Here row b has the length L[b] = max(lens[b], text_lens[b]) -- the N a
 * call of that row alone would run at (duration.py:218-220) -- and reads nothing from its own positions n >= L[b]: the depthwise conv
 * leaves those taps out, the GRN norms over L[b] positions, both conv-pos launches read them as zero, every attention launch gets
 * kv_len = L, and the head's mean stays over n < lens[b].  Values are selected by the index test, never multiplied by a mask: mel
 * frames n >= lens[b] may be NaN.  Filler text positions text_lens[b] <= n < L[b] belong to the row, as in a call of the row alone.
 * text_lens: host [B], one past the row's last text id >= 0.  args->lens == NULL: every lens[b] = n_in.  The lengths are staged next
 * to lens outside the captured part (a replay serves new lengths of the same shape); the graph is keyed apart from
 * f5_predict_duration's, which keeps its key, its launches and its bits; the status word is the same word.  Workspace:
 * f5_duration_workspace_bytes_rows (the plan of f5_duration_workspace_bytes plus [B] int32 behind it).  Refused before any launch,
 * naming the row: text_lens[b] outside [0, nt], lens[b] outside [1, n_in], L[b] < 4 (a call of that row alone is refused for N < 4),
 * a workspace below f5_duration_workspace_bytes_rows, and everything f5_predict_duration refuses. */
int f5_duration_workspace_bytes_rows(f5_duration* d, int B, int n_in, int nt, size_t* bytes);
int f5_predict_duration_rows(f5_duration* d, const f5_duration_args* args, const int32_t* text_lens /* host [B] */, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* F5TTS_HIP_H */
