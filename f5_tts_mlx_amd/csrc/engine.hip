// Engine: weights arena, workspace plan, F5TTS.sample orchestration (eager or hipGraph) and the C ABI.
// Reference path: F5TTS.sample (cfm.py:312-397) -> fn/CFG (cfm.py:340-365) -> DiT.__call__ (dit.py:374-401).
//
// What is hoisted out of the ODE loop (numerically identical up to summation order):
//   * time MLP + all 22 adaLN linears + final adaLN for every function evaluation time (t only),
//   * the text path (TextEmbedding + ConvNeXtV2 blocks) for the cond and null branches (text only),
//   * the cond/text part of the input projection  W_c*cond + W_t*text + b  (dit.py:250).
// Per function evaluation the cond and null branches run as one batch of 2*B*N rows; dual guidance (f5_sample_dual) adds a third
// branch (audio dropped, text kept) behind them: 3*B*N rows in the order F, N, T (docs/dual_guidance.md).
#include <stdarg.h>

#include <cmath>

#include <string>
#include <vector>

#include "../../include/f5tts_hip.h"
#include "host_common.hpp"

// operand type of the per-op entry points (f5_op_*), set by f5_op_set_operand_type; engines carry their own
static Ops g_ops;

// ------------------------------------------------------------------------------------------------
// error string
// ------------------------------------------------------------------------------------------------
static thread_local char g_err[1024] = "";
void f5_set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}
extern "C" const char* f5_last_error(void) { return g_err; }
extern "C" int f5_version(void) { return 1; }

struct MatF8 {          // MX-fp8 matrix in the arena: e4m3 [rows_pad][ld] + E8M0 [rows_pad][ld/32]
    size_t q = 0, s = 0;
    int rows = 0, ld = 0;
};
struct BlockW {
    MatBF qkv, o, ff1, ff2;
    MatF8 qkv8, o8, ff1_8, ff2_8;  // precision mxfp8 only (quantised from the bf16 copies at finalize)
    size_t bqkv, bo, bff1, bff2;  // fp32
};
struct TextBlockW {
    size_t dw_w, dw_b, ln_w, ln_b, b1, gamma, beta, b2;
    MatBF pw1, pw2;
};

struct Workspace {
    size_t total = 0;          // bytes of the whole plan of the call's route (plan_workspace)
    size_t scal, scal_words;   // per-call host scalars, contiguous: [status 1 | lens B | dur2 nbr B | tgrid nfe | dt steps | cfg 1 | lncnt] (32-bit
                               // words; lens and dur2 together are (1 + nbr) B)
    size_t status;             // THE FIRST WORD OF THE WORKSPACE for every shape / solver (a C caller may read it without re-planning), staged
                               // with the scalars: bit 1 = the LN fold ran in this call (set by the host), bit 0 = a folded operand left the
                               // fp16 range (set by the producing epilogue); f5_sample_status / f5_sample_status_async
    size_t lncnt, lncnt_words; // row-block arrival counters of the fused LN tail (zeroed with the scalars; 0 words = no fusion)
    size_t lens, dur2, text, ids, keep, rowkeep;
    size_t tgrid, dt, cfgv, sinus, th, temb, mod;
    size_t rope_cos, rope_sin;
    size_t rope_t;                 // group-major q / k rotation tables (gemm.hpp rope_g4*): 2 x [16][N][4] floats
    size_t cond, traj, ytmp, kst, vel;
    size_t xin[2];
    size_t te[2], tg, grn_partial, grn_nx;
    size_t tln[2], tg2[2], ct[2];
    size_t hc, x;
    size_t xb[2], c1[2], h[2], qk[2], vt[2], ao[2], ffh[2];
    size_t h8, h8s, ao8, ao8s, ffh8, ffh8s;   // precision mxfp8: block-GEMM A operands as e4m3 + E8M0
    // LN fold (0 bytes each where the fold cannot run: plan_workspace)
    size_t lnstats;                // per 64-column slice and row (sum d, centred sum of squares) of d = x - lnmean, [D / 64][M2][2] floats
    size_t lnrowf;                 // row factors (rstd, rstd * (mean - lnmean)), [M2][2] floats
    size_t lnmean;                 // the row's mean at its previous LayerNorm = the shift of the next folded operand, 2 x [M2] floats: the
                                   // consumers that merge the statistics themselves (option fold_stats) read one and write the other
    size_t foldc[2];               // c1, c2 tables, [nfe][L][3 D + FF] floats each
    bool fold_planned;
    size_t vt_bytes;
    size_t cond_keep;              // f5_sample_edit: the per-frame conditioning mask, [B][N] bytes, BEHIND everything above (no other offset moves)
    // per-row routes only (Route::rows; behind everything above: no offset of the base part moves)
    size_t rscal = 0, rscal_words = 0;          // per-row controls, staged per call: [tgrid nfe x B | dt steps x B | cfg B] floats
    size_t rtgrid = 0, rdt = 0, rcfg = 0;
    size_t racfg = 0;                           // dual guidance: the rows' audio strengths, B floats behind rcfg (0 words in the rows plan)
    size_t rsinus = 0, rth = 0, rtemb = 0;      // time MLP of every (evaluation, row): [nfe x B] rows each
    size_t rmod = 0;                            // adaLN table [nfe][B][(6L+2) D]
    int nbr = 2;                                // branches the plan lays out: 2 (cond + null), 3 = dual guidance (F, N, T)
    // f5_sample_window only (Route::window; behind the rows part): the rows' EFFECTIVE strengths of every evaluation, [nfe][B] floats
    // each, staged per call; stage j reads row j where the rows / dual calls read the one [B] vector at rcfg / racfg
    size_t wcfg = 0, wacfg = 0, wtab_words = 0;
    // F5_AB2 / F5_AB3 only (behind everything else): the weight triples, [steps - 1][3] floats, on a per-row route [steps - 1][B][3]
    size_t abw = 0, abw_words = 0;
};

// Per-engine launch options: everything that reaches a kernel as a by-value argument or changes the launch sequence of sample()
// lives in the engine handle, so two engines of one process keep their own configuration (f5_engine_set_option).  The process-wide
// f5_debug_set_* hooks only set the DEFAULTS a new engine starts from (and what the per-op entry points f5_op_* use).
struct F5Options {
    int q_premul = 1;     // q leaves the QKV epilogue multiplied by softmax_scale * log2(e) (single-segment operand modes)
    int qkv_tr = 1;       // 256x256 QKV kernel: q / k tiles accumulated transposed (pair-major rotation tables)
    int fuse_ln = 0;      // LN-modulate fused behind the small-tile residual GEMMs (measured slower, profiles/r02/ln_fusion_ab.txt)
    int gemm_flags = 0;   // F5GemmArgs::debug_flags of this engine's GEMM launches
    int attn_pipe = -1;   // large-grid attention: -1 = process default (f5_debug_set_attn_pipe), 0 = v2f, 1 = v2p (in-wave software pipeline)
    int ln_fold = -1;     // LN-modulate folded into the GEMMs around it (gemm.hpp fold_*): -1 = where it is measured faster (>= LN_FOLD_AUTO_ROWS
                          // rows and the four block GEMMs on the staged kernels, one-pass operand modes), 0 = never, 1 = wherever it can run
                          // (batch >= 4 at the 335M shape; fails loudly elsewhere)
    int fold_stats = -1;  // LN fold: 1 = the consumer GEMMs merge the producer's slice statistics into their row factors themselves (gemm.hpp fold_stats;
                          // width 1024 only), 0 = a f5_fold_rows launch between producer and consumer (round 4-5; rules the batch-1-sized route
                          // out), -1 = the statistics form on the batch-1-sized route only
    int graph_split = 0;  // 0: a call is ONE hipGraphExec (~5 000 kernel nodes at 32 points); 1: one exec per ODE step (prep rides in the first), launched
                          // back to back -- the same kernels with the same arguments, 31 replays of ~165 nodes (round-6 probe: does a long exec cost more per node?)
    int sat_check = 1;    // precision f16: every 16-bit operand producer reports values beyond +-65 504 in the status word (bit 2); 0 = A/B
    int null_keeps_cond = 0;   // the second (null) branch keeps the audio conditioning: DiT.__call__(drop_audio_cond=False, drop_text=True), dit.py:374-401
    int isolate_rows = 0;      // calls with use_mask: row b reads nothing from its own positions n >= durations[b] -- conv-pos and the text blocks'
                               // depthwise conv see zeros there, the text GRN norms over the row's own frames (docs/isolate_rows.md)
};
static F5Options g_default_options;
static int g_live_engines = 0;   // f5_debug_set_{ln_fusion,qkv_transposed,q_premul} only change the DEFAULTS: with engines alive they say so
// bumped by every process-wide launch knob change (f5_debug_set_*): part of the graph key, so a cached hipGraph captured under other
// knob values is never replayed
static int g_knob_epoch = 0;

struct f5_engine : WeightStore {
    f5_config cfg;
    int prec;
    // arena offsets
    size_t time_w0, time_b0, time_w2, time_b2;
    size_t ada_w, ada_b;  // [(6*depth+2)*D][D], [(6*depth+2)*D]
    size_t text_table, text_pos;
    std::vector<TextBlockW> tblocks;
    MatBF wx, wct;
    size_t bproj;
    MatBF conv_w[2];
    size_t conv_b[2];
    std::vector<BlockW> blocks;
    // LN fold constants (run_prep): the blocks' QKV / FF1 weights (bytes) and biases (bytes) sit `fold_stride` apart in the arena; uniform =
    // at one stride for every block, so the blocks of a projection go in ONE fold_consts launch (build_arena_plan)
    long fold_stride[4] = {0, 0, 0, 0};       // qkv weight, ff1 weight, qkv bias, ff1 bias
    bool fold_uniform = false;
    MatBF wout;
    size_t bout;
    Ops ops;                          // kernels of this engine's operand type
    F5Options opt = g_default_options;
    GraphCache graphs;                // cached hipGraphExecs, at most f5_engine_set_graph_cache (default 8)
    std::vector<std::string> seen;    // signatures sampled once in "auto" graph mode (captured on the second sighting)
    std::vector<uint8_t> last_pattern; // f5_sample_window: wide (1) / narrow (0) per evaluation of the most recent call (f5_debug_last_sample_pattern)
};

static bool method_known(int method) { return method >= F5_EULER && method <= F5_AB3; }
// Adams-Bashforth: the highest order the method reaches (0 = a one-step method)
static int ab_order(int method) { return method == F5_AB2 ? 2 : (method == F5_AB3 ? 3 : 0); }
static int nfe_per_step(int method) { return (method == F5_EULER || ab_order(method)) ? 1 : (method == F5_MIDPOINT ? 2 : 4); }
// The weights of Adams-Bashforth step i on the grid t (fp32 values, arithmetic in fp64, rounded once): the integral over [t_i, t_i+1] of
// the Lagrange interpolant through (t_i, k_i), (t_i-1, k_i-1) (, (t_i-2, k_i-2)), divided by h.  a = t_i - t_i-1, b = t_i - t_i-2.  Order
// min(i + 1, order); a spacing that is not positive (a <= 0; third order: b - a <= 0) drops to the highest order whose spacings are.  An
// absent weight is exactly 0.  (cfm.ab_weights is the same rule in Python.)
static void ab_weights(const float* t, int i, int order, float w[3]) {
    const double h = (double)t[i + 1] - (double)t[i];
    const double a = i >= 1 ? (double)t[i] - (double)t[i - 1] : 0.0, b = i >= 2 ? (double)t[i] - (double)t[i - 2] : 0.0;
    int ord = order < i + 1 ? order : i + 1;
    if (ord >= 3 && !(b - a > 0.0)) ord = 2;
    if (ord >= 2 && !(a > 0.0)) ord = 1;
    w[0] = 1.0f;
    w[1] = w[2] = 0.0f;
    if (ord == 2) {
        w[0] = (float)(1.0 + h / (2.0 * a));
        w[1] = (float)(0.0 - h / (2.0 * a));          // (0 - x: a step of length 0 gives +0, not -0)
    } else if (ord == 3) {
        w[0] = (float)((h * h / 3.0 + (a + b) * h / 2.0 + a * b) / (a * b));
        w[1] = (float)(0.0 - (h * h / 3.0 + b * h / 2.0) / (a * (b - a)));
        w[2] = (float)((h * h / 3.0 + a * h / 2.0) / (b * (b - a)));
    }
}

static MatF8 alloc_f8(Bump& b, int rows, int ld) {
    MatF8 m;
    m.rows = rows;
    m.ld = ld;
    const int rows_pad = (rows + 255) / 256 * 256;  // the MX GEMM reads whole 256-row weight tiles
    m.q = b.take((size_t)rows_pad * ld);
    m.s = b.take((size_t)rows_pad * (ld / 32));
    return m;
}

static int build_arena_plan(f5_engine* e) {
    const f5_config& c = e->cfg;
    const int D = c.dim, Dt = c.text_dim, FF = c.ff_dim, TF = c.text_ff_dim, L = c.depth, np = e->np;
    Bump b;
    const std::string p = "transformer.";
    // time MLP (fp32)
    e->time_w0 = b.take((size_t)D * c.freq_embed_dim * 4);
    e->time_b0 = b.take((size_t)D * 4);
    e->time_w2 = b.take((size_t)D * D * 4);
    e->time_b2 = b.take((size_t)D * 4);
    e->add_f32(p + "time_embed.time_mlp.layers.0.weight", e->time_w0, {D, c.freq_embed_dim});
    e->add_f32(p + "time_embed.time_mlp.layers.0.bias", e->time_b0, {D});
    e->add_f32(p + "time_embed.time_mlp.layers.2.weight", e->time_w2, {D, D});
    e->add_f32(p + "time_embed.time_mlp.layers.2.bias", e->time_b2, {D});
    // adaLN (fp32): all blocks + final stacked so one skinny GEMM builds the whole modulation table
    const size_t ada_rows = (size_t)(6 * L + 2) * D;
    e->ada_w = b.take(ada_rows * D * 4);
    e->ada_b = b.take(ada_rows * 4);
    // text embedding
    e->text_table = b.take((size_t)(c.text_num_embeds + 1) * Dt * 4);
    e->text_pos = b.take((size_t)c.text_max_pos * Dt * 4);
    e->add_f32(p + "text_embed.text_embed.weight", e->text_table, {c.text_num_embeds + 1, Dt});
    e->tblocks.resize(c.conv_layers);
    for (int i = 0; i < c.conv_layers; ++i) {
        TextBlockW& t = e->tblocks[i];
        const std::string q = p + "text_embed.text_blocks.layers." + std::to_string(i) + ".";
        t.dw_w = b.take((size_t)Dt * 7 * 4);
        t.dw_b = b.take((size_t)Dt * 4);
        t.ln_w = b.take((size_t)Dt * 4);
        t.ln_b = b.take((size_t)Dt * 4);
        t.b1 = b.take((size_t)TF * 4);
        t.gamma = b.take((size_t)TF * 4);
        t.beta = b.take((size_t)TF * 4);
        t.b2 = b.take((size_t)Dt * 4);
        t.pw1 = alloc_mat(b, TF, Dt, np);
        t.pw2 = alloc_mat(b, Dt, TF, np);
        e->add_f32(q + "dwconv.weight", t.dw_w, {Dt, 7, 1});
        e->add_f32(q + "dwconv.bias", t.dw_b, {Dt});
        e->add_f32(q + "norm.weight", t.ln_w, {Dt});
        e->add_f32(q + "norm.bias", t.ln_b, {Dt});
        e->add_mat(q + "pwconv1.weight", t.pw1, 0, TF, Dt, 0, Dt, 0, {TF, Dt});
        e->add_f32(q + "pwconv1.bias", t.b1, {TF});
        e->add_f32(q + "grn.gamma", t.gamma, {1, 1, TF});
        e->add_f32(q + "grn.beta", t.beta, {1, 1, TF});
        e->add_mat(q + "pwconv2.weight", t.pw2, 0, Dt, TF, 0, TF, 0, {Dt, TF});
        e->add_f32(q + "pwconv2.bias", t.b2, {Dt});
    }
    // input projection, split by input segment (x | cond | text), dit.py:250
    const int M = c.mel_dim, IN = 2 * M + Dt;
    e->wx = alloc_mat(b, D, 128, np);
    e->wct = alloc_mat(b, D, 128 + Dt, np);
    e->bproj = b.take((size_t)D * 4);
    e->add_mat(p + "input_embed.proj.weight", e->wx, 0, D, IN, 0, M, 0, {D, IN});
    e->add_mat(p + "input_embed.proj.weight", e->wct, 0, D, IN, M, 2 * M, 0, {D, IN});
    e->add_mat(p + "input_embed.proj.weight", e->wct, 0, D, IN, 2 * M, IN, 128, {D, IN});
    e->add_f32(p + "input_embed.proj.bias", e->bproj, {D});
    const int kc = c.conv_pos_kernel, gin = D / c.conv_pos_groups;
    for (int j = 0; j < 2; ++j) {      // 64 channels per group: the tensor as it is; 32 and 48 in the packed form of f5_pack_conv_groups
        const std::string q = p + "input_embed.conv_pos_embed.conv1d.layers." + std::to_string(j * 2) + ".";
        e->conv_w[j] = e->add_conv_groups(b, q + "weight", D, kc, gin);
        e->conv_b[j] = b.take((size_t)D * 4);
        e->add_f32(q + "bias", e->conv_b[j], {D});
    }
    // attention inner width I = heads * dim_head (dit.py:117-125: dim -> I -> dim); q | k | v rows of the fused projection are I apart
    const int I = c.heads * c.dim_head;
    e->blocks.resize(L);
    for (int i = 0; i < L; ++i) {
        BlockW& w = e->blocks[i];
        const std::string q = p + "transformer_blocks." + std::to_string(i) + ".";
        w.qkv = alloc_mat(b, 3 * I, D, np);
        w.o = alloc_mat(b, D, I, np);
        w.ff1 = alloc_mat(b, FF, D, np);
        w.ff2 = alloc_mat(b, D, FF, np);
        if (e->prec == F5_PREC_MXFP8) {
            w.qkv8 = alloc_f8(b, 3 * I, D);
            w.o8 = alloc_f8(b, D, I);
            w.ff1_8 = alloc_f8(b, FF, D);
            w.ff2_8 = alloc_f8(b, D, FF);
        }
        w.bqkv = b.take((size_t)3 * I * 4);
        w.bo = b.take((size_t)D * 4);
        w.bff1 = b.take((size_t)FF * 4);
        w.bff2 = b.take((size_t)D * 4);
        e->add_f32(q + "attn_norm.linear.weight", e->ada_w + (size_t)i * 6 * D * D * 4, {6 * D, D});
        e->add_f32(q + "attn_norm.linear.bias", e->ada_b + (size_t)i * 6 * D * 4, {6 * D});
        const char* nm[3] = {"to_q", "to_k", "to_v"};
        for (int k = 0; k < 3; ++k) {
            e->add_mat(q + "attn." + nm[k] + ".weight", w.qkv, k * I, I, D, 0, D, 0, {I, D});
            e->add_f32(q + "attn." + nm[k] + ".bias", w.bqkv + (size_t)k * I * 4, {I});
        }
        e->add_mat(q + "attn.to_out.layers.0.weight", w.o, 0, D, I, 0, I, 0, {D, I});
        e->add_f32(q + "attn.to_out.layers.0.bias", w.bo, {D});
        e->add_mat(q + "ff.ff.layers.0.layers.0.weight", w.ff1, 0, FF, D, 0, D, 0, {FF, D});
        e->add_f32(q + "ff.ff.layers.0.layers.0.bias", w.bff1, {FF});
        e->add_mat(q + "ff.ff.layers.2.weight", w.ff2, 0, D, FF, 0, FF, 0, {D, FF});
        e->add_f32(q + "ff.ff.layers.2.bias", w.bff2, {D});
    }
    // every block allocates the same tensors in the same order, so the strides are uniform; checked, because run_prep batches on it
    const BlockW& b0 = e->blocks[0];
    const auto offs = [&](const BlockW& w, int k) { return (long)(k == 0 ? w.qkv.hi : k == 1 ? w.ff1.hi : k == 2 ? w.bqkv : w.bff1); };
    e->fold_uniform = L >= 2;
    for (int k = 0; k < 4; ++k) {
        long& st = e->fold_stride[k];
        st = L >= 2 ? offs(e->blocks[1], k) - offs(b0, k) : 0;
        for (int i = 1; i < L; ++i) e->fold_uniform = e->fold_uniform && offs(e->blocks[i], k) - offs(b0, k) == i * st;
        e->fold_uniform = e->fold_uniform && st > 0 && st % (k < 2 ? 8 : 4) == 0;
    }
    for (int i = 1; i < L; ++i) e->fold_uniform = e->fold_uniform && e->blocks[i].qkv.ld == b0.qkv.ld && e->blocks[i].ff1.ld == b0.ff1.ld;
    e->add_f32(p + "norm_out.linear.weight", e->ada_w + (size_t)L * 6 * D * D * 4, {2 * D, D});
    e->add_f32(p + "norm_out.linear.bias", e->ada_b + (size_t)L * 6 * D * 4, {2 * D});
    e->wout = alloc_mat(b, M, D, np);
    e->bout = b.take((size_t)M * 4);
    e->add_mat(p + "proj_out.weight", e->wout, 0, M, D, 0, D, 0, {M, D});
    e->add_f32(p + "proj_out.bias", e->bout, {M});
    e->arena_need = b.off;
    return 0;
}

extern "C" int f5_engine_create(const f5_config* cfg, int precision, f5_engine** out) {
    F5_REQUIRE(cfg && out, "f5_engine_create: null argument");
    const f5_config& c = *cfg;
    F5_REQUIRE(precision == F5_PREC_BF16 || precision == F5_PREC_BF16X3 || precision == F5_PREC_MXFP8 || precision == F5_PREC_F16,
               "unknown precision %d", precision);
    F5_REQUIRE(precision != F5_PREC_MXFP8 || (cfg->ff_dim % 256 == 0 && cfg->dim % 256 == 0), "mxfp8 needs dim and ff_dim to be multiples of 256");
    F5_REQUIRE(c.dim_head == 64, "dim_head must be 64 (got %d)", c.dim_head);
    // the accepted family (docs/geometries.md): the attention inner width need not be the model width, conv-pos groups may be 32, 48 or
    // 64 channels wide, the text width is a multiple of 128
    const int inner = c.heads * c.dim_head;
    F5_REQUIRE(c.heads >= 1 && inner % 256 == 0, "heads * dim_head must be a multiple of 256 (got %d * %d = %d)", c.heads, c.dim_head, inner);
    F5_REQUIRE(inner <= 1024, "heads * dim_head must be <= 1024 (got %d * %d = %d)", c.heads, c.dim_head, inner);
    const int cpg = c.conv_pos_groups >= 1 && c.dim % c.conv_pos_groups == 0 ? c.dim / c.conv_pos_groups : 0;
    F5_REQUIRE(cpg == 64 || cpg == 48 || (cpg == 32 && c.conv_pos_groups % 2 == 0),
               "dim / conv_pos_groups must be 32, 48 or 64 channels per group (got %d / %d)", c.dim, c.conv_pos_groups);
    F5_REQUIRE(c.dim % 256 == 0 && c.dim <= 1024, "dim must be a multiple of 256 and <= 1024 (got %d)", c.dim);
    F5_REQUIRE(c.conv_pos_kernel % 2 == 1 && c.conv_pos_kernel <= 31, "conv_pos_kernel must be odd and <= 31");
    F5_REQUIRE(c.text_dim >= 128 && c.text_dim % 128 == 0 && c.text_dim <= 1024, "text_dim must be a multiple of 128 and <= 1024 (got %d)", c.text_dim);
    // the MX-fp8 blocks are built and measured for the original family only
    F5_REQUIRE(precision != F5_PREC_MXFP8 || (inner == c.dim && cpg == 64 && c.text_dim % 256 == 0),
               "mxfp8 needs heads * dim_head == dim, 64-channel conv-pos groups and text_dim %% 256 == 0 (got inner %d, dim %d, %d channels per "
               "group, text_dim %d): run this geometry in f16, bf16 or bf16x3",
               inner, c.dim, cpg, c.text_dim);
    F5_REQUIRE(c.ff_dim % 128 == 0 && c.text_ff_dim % 128 == 0, "ff dims must be multiples of 128");
    F5_REQUIRE(c.mel_dim >= 1 && c.mel_dim <= 128, "mel_dim must be in [1,128]");
    F5_REQUIRE(c.freq_embed_dim % 256 == 0 && c.freq_embed_dim <= 1024, "freq_embed_dim must be a multiple of 256");
    F5_REQUIRE(c.depth >= 1 && c.conv_layers >= 0, "depth must be >= 1 and conv_layers >= 0");
    f5_engine* e = new f5_engine();
    e->cfg = c;
    e->prec = precision;
    e->np = precision == F5_PREC_BF16X3 ? 2 : 1;
    e->f16 = e->ops.h = precision == F5_PREC_F16;
    build_arena_plan(e);
    ++g_live_engines;
    *out = e;
    return 0;
}

extern "C" void f5_engine_destroy(f5_engine* e) {
    if (!e) return;
    --g_live_engines;
    delete e;      // (~GraphCache waits for the last replay of every exec)
}

extern "C" int f5_engine_set_graph_cache(f5_engine* e, int max_graphs) {
    F5_REQUIRE(e && max_graphs >= 1 && max_graphs <= 1024, "graph cache size must be in [1, 1024]");
    e->graphs.set_cap((size_t)max_graphs);
    return 0;
}

// The engine options by name.  Switches are 0 / 1, tri-states -1 (automatic) / 0 / 1, gemm_flags is a raw word.  One table serves
// set, get, the message that lists the names and the option part of the graph key.  `group`: null = a launch option, named inside the
// parentheses of that message (the list callers parse); an option of another kind is named behind the list under its group.
enum OptKind { OPT_SWITCH, OPT_TRI, OPT_INT };
static const struct OptDesc {
    const char* name;
    int F5Options::*member;
    OptKind kind;
    const char* group = nullptr;
} k_options[] = {
    {"q_premul", &F5Options::q_premul, OPT_SWITCH},     {"qkv_transposed", &F5Options::qkv_tr, OPT_SWITCH},
    {"ln_fusion", &F5Options::fuse_ln, OPT_SWITCH},     {"gemm_flags", &F5Options::gemm_flags, OPT_INT},
    {"attn_pipe", &F5Options::attn_pipe, OPT_TRI},      {"null_keeps_cond", &F5Options::null_keeps_cond, OPT_SWITCH},
    {"ln_fold", &F5Options::ln_fold, OPT_TRI},          {"sat_check", &F5Options::sat_check, OPT_SWITCH},
    {"graph_split", &F5Options::graph_split, OPT_SWITCH}, {"fold_stats", &F5Options::fold_stats, OPT_TRI},
    {"isolate_rows", &F5Options::isolate_rows, OPT_SWITCH, "row isolation"},
};
static const OptDesc* find_option(const char* name) {
    std::string names, grouped;
    for (const OptDesc& o : k_options) {
        if (strcmp(o.name, name) == 0) return &o;
        if (o.group) {
            grouped += std::string("; ") + o.group + ": " + o.name;
            continue;
        }
        names += names.empty() ? "" : ", ";
        names += o.name;
    }
    f5_set_error("unknown engine option %s (%s)%s", name, names.c_str(), grouped.c_str());
    return nullptr;
}
extern "C" int f5_engine_set_option(f5_engine* e, const char* name, int value) {
    F5_REQUIRE(e && name, "null argument");
    const OptDesc* o = find_option(name);
    if (!o) return 2;
    e->opt.*o->member = o->kind == OPT_INT ? value : (o->kind == OPT_TRI && value < 0 ? -1 : (value ? 1 : 0));
    return 0;
}
extern "C" int f5_engine_get_option(f5_engine* e, const char* name, int* value) {
    F5_REQUIRE(e && name && value, "null argument");
    const OptDesc* o = find_option(name);
    if (!o) return 2;
    *value = e->opt.*o->member;
    return 0;
}
extern "C" int f5_engine_graph_count(f5_engine* e) { return e ? e->graphs.size() : -1; }

extern "C" int f5_weights_bytes(f5_engine* e, size_t* bytes) {
    F5_REQUIRE(e && bytes, "null argument");
    *bytes = e->arena_need;
    return 0;
}

extern "C" int f5_set_weights_arena(f5_engine* e, void* dev_arena, size_t bytes, void* stream) {
    F5_REQUIRE(e && dev_arena, "null argument");
    return e->set_arena(dev_arena, bytes, (hipStream_t)stream);
}

extern "C" int f5_load_tensor(f5_engine* e, const char* name, const float* host, int ndim, const int64_t* shape) {
    F5_REQUIRE(e && name && host && shape, "null argument");
    // the name and the shape are checked before the arena, so that a host can validate a checkpoint without a device
    std::vector<TensorDst>* dsts = nullptr;
    size_t count = 0;
    RC(e->lookup(name, name, &dsts));
    RC(e->match(name, *dsts, ndim, shape, &count));
    F5_REQUIRE(e->arena, "f5_set_weights_arena must be called first");
    for (TensorDst& d : *dsts) RC(e->upload(d, host, count));
    return 0;
}

extern "C" int f5_mark_weights_loaded(f5_engine* e) {
    F5_REQUIRE(e, "null argument");
    e->mark_all_loaded();
    return 0;
}

// A second handle on the arena of `owner` (same configuration and precision, weights finalised): nothing is written, the caller keeps the
// arena alive for both.  What it is for: two handles driven by two host threads on two streams (two half batches of one sample() call fill
// the partly empty last rounds of each other's launches: engine.py Engine._sample_split); every handle has its own
// workspace, hipGraphs and status word, the weights are read-only on the hot path.
extern "C" int f5_share_weights(f5_engine* e, const f5_engine* owner) {
    F5_REQUIRE(e && owner && e != owner, "f5_share_weights: null argument / the same handle twice");
    F5_REQUIRE(owner->arena && owner->finalized, "f5_share_weights: the owner's weights are not finalised");
    F5_REQUIRE(e->prec == owner->prec && e->arena_need == owner->arena_need && memcmp(&e->cfg, &owner->cfg, sizeof(f5_config)) == 0,
               "f5_share_weights: the two handles differ in configuration or precision");
    e->arena = owner->arena;
    e->arena_bytes = owner->arena_bytes;
    e->mark_all_loaded();
    e->finalized = true;
    return 0;
}

// One collective replicates the model: the arena is contiguous, so a host that owns an RCCL communicator (one process per GPU,
// xGMI) broadcasts it from `root` with a single ncclBroadcast.  RCCL is resolved at run time (dlopen) so that the library has
// no link-time dependency on it; the torch.distributed path of the Python wrapper (dist.py) does the same with dist.broadcast.
#include <dlfcn.h>
extern "C" int f5_broadcast_weights(f5_engine* e, void* nccl_comm, int root, int rank, void* stream) {
    F5_REQUIRE(e && e->arena && nccl_comm, "f5_broadcast_weights: null engine / arena / communicator");
    typedef int (*bcast_fn)(const void*, void*, size_t, int, int, void*, hipStream_t);
    static bcast_fn fn = nullptr;
    if (!fn) {
        void* h = nullptr;
        for (const char* name : {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1", "/opt/rocm/lib/librccl.so"}) {
            h = dlopen(name, RTLD_NOW | RTLD_GLOBAL);
            if (h) break;
        }
        F5_REQUIRE(h != nullptr, "f5_broadcast_weights: librccl.so not found (%s)", dlerror());
        fn = (bcast_fn)dlsym(h, "ncclBroadcast");
        F5_REQUIRE(fn != nullptr, "f5_broadcast_weights: ncclBroadcast not found in librccl.so");
    }
    const int ncclUint8 = 1;
    const int rc = fn(e->arena, e->arena, e->arena_need, ncclUint8, root, nccl_comm, (hipStream_t)stream);
    F5_REQUIRE(rc == 0, "ncclBroadcast failed with ncclResult_t %d", rc);
    if (rank != root) e->mark_all_loaded();
    return 0;
}

extern "C" int f5_finalize_weights(f5_engine* e, void* stream) {
    F5_REQUIRE(e && e->arena, "arena not set");
    RC(e->require_loaded());
    int rc = f5_launch_text_pos_table((float*)(e->arena + e->text_pos), e->cfg.text_max_pos, e->cfg.text_dim, (hipStream_t)stream);
    if (rc) return rc;
    if (e->prec == F5_PREC_MXFP8) {
        // MX-fp8 copies of the four block matrices, from the bf16 copies (pad rows of the arena are zero -> scale 0, bytes 0)
        for (const BlockW& w : e->blocks) {
            const MatBF* src[4] = {&w.qkv, &w.o, &w.ff1, &w.ff2};
            const MatF8* dst[4] = {&w.qkv8, &w.o8, &w.ff1_8, &w.ff2_8};
            for (int k = 0; k < 4; ++k) {
                rc = f5_launch_quantize_mx_bf16((const op16_t*)(e->arena + src[k]->hi), src[k]->ld, (uint8_t*)(e->arena + dst[k]->q),
                                                dst[k]->ld, (uint8_t*)(e->arena + dst[k]->s), src[k]->rows, src[k]->ld,
                                                (hipStream_t)stream);
                if (rc) return rc;
            }
        }
    }
    F5_HIP_CHECK(hipStreamSynchronize((hipStream_t)stream));
    e->finalized = true;
    return 0;
}

// ------------------------------------------------------------------------------------------------
// workspace plan
// ------------------------------------------------------------------------------------------------
// LN fold, automatic mode: measured on sample(), 335M shape, f16 (profiles/r04/ln_fold_ab.jsonl): batch 4 -1.2 %, 8 -1.1 %, 12 +0.3 %,
// 16 +0.8 %, 32 +2.5 %: the LN launches it removes cost ~2 us per thousand rows, what it adds (x16 write in the residual epilogues, the
// row-factor kernel) has a floor
constexpr long LN_FOLD_AUTO_ROWS = 22000;
// The batch-1-sized route (round 6): all four block GEMMs are ONE round of workgroups, the consumers merge the slice statistics themselves
// (no row-factor launch), so the fold removes 44 of the 46 LN-modulate launches of a forward for a few hundred VALU instructions in the
// residual epilogues.  LN_FOLD_SMALL_AUTO: chosen by the automatic mode (-1) where the route applies.
constexpr long LN_FOLD_SMALL_ROWS = 2048;
constexpr bool LN_FOLD_SMALL_AUTO = false;     // measured -1.5 ... +0.7 % at batch 1 (profiles/r06): below the 4 % bar, so opt-in (ln_fold = 1)

// Which of the entry points a call came through, as far as the plan and the launch sequence care: rows = time and guidance strength per
// batch row (f5_sample_rows, f5_dit_forward_rows and everything below), dual = the rows route with three branches F, N, T
// (f5_sample_dual, f5_dit_forward_dual), window = the strengths gated per evaluation (f5_sample_window, single or dual).
struct Route {
    bool rows = false, dual = false, window = false;
    int nbr() const { return dual ? 3 : 2; }     // branches of a function evaluation the plan has room for
};

// The base part, then the per-row part (route.rows), then the window tables (route.window); each part lies behind the one before, so no
// offset of an earlier part depends on a later one.  The text path always runs for two branches (the third branch of dual guidance reuses
// branch 0's text embedding), so only the buffers of the DiT itself -- MB rows -- and the per-branch durations grow with nbr.
static Workspace plan_workspace(const f5_engine* e, int B, int N, int nt, int steps, int method, Route route) {
    const f5_config& c = e->cfg;
    const int D = c.dim, Dt = c.text_dim, FF = c.ff_dim, TF = c.text_ff_dim, L = c.depth, np = e->np, mel = c.mel_dim, nbr = route.nbr();
    const int I = c.heads * c.dim_head;      // attention inner width: q, k, V^T and the attention output are I wide
    const size_t M1 = (size_t)B * N, M2 = 2 * M1, MB = (size_t)nbr * M1;
    const int nfe = (steps - 1) * nfe_per_step(method);
    const int npad = (N + 63) / 64 * 64;
    Bump b;
    Workspace w;
    w.nbr = nbr;
    const size_t nfe1 = (size_t)(nfe > 0 ? nfe : 1);
    // one counter per 64 rows of the residual stream; only small-M launches fuse (gemm.hpp ln_counter), large ones get none
    w.lncnt_words = (M2 + 63) / 64 <= 512 ? (M2 + 63) / 64 : 0;
    w.scal_words = (size_t)1 + (size_t)(1 + nbr) * B + nfe1 + steps + 1 + w.lncnt_words;
    w.scal = b.take(w.scal_words * 4);
    w.status = w.scal;                      // offset 0, whatever the sizes
    w.lens = w.scal + 4;
    w.dur2 = w.lens + (size_t)B * 4;
    w.tgrid = w.dur2 + (size_t)nbr * B * 4;
    w.dt = w.tgrid + nfe1 * 4;
    w.cfgv = w.dt + (size_t)steps * 4;
    w.lncnt = w.cfgv + 4;
    w.text = b.take((size_t)B * (nt > 0 ? nt : 1) * 4);
    w.ids = b.take(M2 * 4);
    w.keep = b.take(M2);
    w.rowkeep = b.take(MB);
    w.sinus = b.take((size_t)(nfe + 1) * c.freq_embed_dim * 4);
    w.th = b.take((size_t)(nfe + 1) * D * 4);
    w.temb = b.take((size_t)(nfe + 1) * D * 4);
    w.mod = b.take((size_t)(nfe + 1) * (6 * L + 2) * D * 4);
    w.rope_cos = b.take((size_t)N * 32 * 4);
    w.rope_sin = b.take((size_t)N * 32 * 4);
    w.rope_t = b.take((size_t)4 * 32 * N * 4);
    w.cond = b.take(M1 * mel * 4);
    w.traj = b.take((size_t)steps * M1 * mel * 4);
    w.ytmp = b.take(M1 * mel * 4);
    w.kst = b.take(3 * M1 * mel * 4);
    w.vel = b.take(MB * mel * 4);
    for (int p = 0; p < 2; ++p) w.xin[p] = p < np ? b.take(M1 * 128 * 2) : 0;
    w.te[0] = b.take(M2 * Dt * 4);
    w.te[1] = b.take(M2 * Dt * 4);
    w.tg = b.take(M2 * TF * 4);
    w.grn_partial = b.take(f5_grn_partial_floats(2 * B, N, TF) * 4);
    w.grn_nx = b.take((size_t)2 * B * TF * 4);
    for (int p = 0; p < 2; ++p) {
        w.tln[p] = p < np ? b.take(M2 * Dt * 2) : 0;
        w.tg2[p] = p < np ? b.take(M2 * TF * 2) : 0;
        w.ct[p] = p < np ? b.take(MB * (128 + Dt) * 2) : 0;
    }
    w.hc = b.take(MB * D * 4);
    w.x = b.take(MB * D * 4);
    w.vt_bytes = (size_t)nbr * B * c.heads * 64 * npad * 2;
    for (int p = 0; p < 2; ++p) {
        w.xb[p] = p < np ? b.take(MB * D * 2) : 0;
        w.c1[p] = p < np ? b.take(MB * D * 2) : 0;
        w.h[p] = p < np ? b.take(MB * D * 2) : 0;
        // q | k also parks the fp32 result of the two gated projections on the per-row route (resid_ln, LN_ROWS): M D floats, more than
        // the 2 I 16-bit values per row when I < D
        w.qk[p] = p < np ? b.take(MB * (size_t)2 * (p == 0 && I < D ? D : I) * 2) : 0;
        w.vt[p] = p < np ? b.take(w.vt_bytes) : 0;
        w.ao[p] = p < np ? b.take(MB * I * 2) : 0;
        w.ffh[p] = p < np ? b.take(MB * FF * 2) : 0;
    }
    // LN fold buffers only where the fold can run (a superset of the LN plan's fold: that one also knows the branch count of the call):
    // one-pass 16-bit operand modes, the option not 0, and -- in the automatic mode -- enough rows for it to be chosen with both branches
    // (... or few enough for the single-round kernels of the batch-1-sized route, gemm_route.hpp f5_gemm_fold_small: <= 2 048 rows at width 1024)
    w.fold_planned = np == 1 && e->prec != F5_PREC_MXFP8 && e->opt.ln_fold != 0 &&
                     (e->opt.ln_fold == 1 || (long)M2 >= LN_FOLD_AUTO_ROWS || ((long)M2 <= LN_FOLD_SMALL_ROWS && LN_FOLD_SMALL_AUTO));
    const size_t fp = w.fold_planned ? 1 : 0;
    w.lnstats = b.take(fp * M2 * (size_t)((D + 63) / 64) * 2 * 4);
    w.lnrowf = b.take(fp * M2 * 2 * 4);
    w.lnmean = b.take(fp * 2 * M2 * 4);
    for (int p = 0; p < 2; ++p) w.foldc[p] = b.take(fp * nfe1 * L * (size_t)(3 * D + FF) * 4);
    w.h8 = w.h8s = w.ao8 = w.ao8s = w.ffh8 = w.ffh8s = 0;
    if (e->prec == F5_PREC_MXFP8) {
        w.h8 = b.take(M2 * D);
        w.h8s = b.take(M2 * (D / 32));
        w.ao8 = b.take(M2 * D);
        w.ao8s = b.take(M2 * (D / 32));
        w.ffh8 = b.take(M2 * FF);
        w.ffh8s = b.take(M2 * (FF / 32));
    }
    w.cond_keep = b.take(M1);
    if (route.rows) {
        // the staged controls and the time / adaLN tables of every (evaluation, row) pair.  The fp32 scratch of the two gated projections
        // needs no space of its own: w.qk[0] (2 M D 16-bit values = M D floats) is dead from the end of a block's attention to the next
        // block's QKV projection, which is where both projections run.
        const size_t rows = nfe1 * B;
        w.rscal_words = rows + (size_t)steps * B + B + (route.dual ? (size_t)B : 0);
        w.rscal = b.take(w.rscal_words * 4);
        w.rtgrid = w.rscal;
        w.rdt = w.rtgrid + rows * 4;
        w.rcfg = w.rdt + (size_t)steps * B * 4;
        w.racfg = w.rcfg + (size_t)B * 4;
        w.rsinus = b.take(rows * c.freq_embed_dim * 4);
        w.rth = b.take(rows * D * 4);
        w.rtemb = b.take(rows * D * 4);
        w.rmod = b.take(rows * (size_t)(6 * L + 2) * D * 4);
        if (route.window) {
            w.wtab_words = (route.dual ? 2 : 1) * rows;
            w.wcfg = b.take(w.wtab_words * 4);
            w.wacfg = route.dual ? w.wcfg + rows * 4 : 0;
        }
    }
    if (ab_order(method)) {
        w.abw_words = (size_t)3 * (steps > 1 ? steps - 1 : 1) * (route.rows ? B : 1);
        w.abw = b.take(w.abw_words * 4);
    }
    w.total = b.off;
    return w;
}

// the four size queries: f5_workspace_bytes (plain), _rows, _dual (the rows plan with room for the third branch) and _window (either
// with the effective-strength tables behind it)
static int workspace_bytes(f5_engine* e, int B, int N, int nt, int steps, int method, Route route, size_t* bytes) {
    F5_REQUIRE(e && bytes, "null argument");
    F5_REQUIRE(B >= 1 && N >= 1 && steps >= 1, "bad sizes B=%d N=%d steps=%d", B, N, steps);
    F5_REQUIRE(method_known(method), "Unknown method: %d", method);
    *bytes = plan_workspace(e, B, N, nt, steps, method, route).total;
    return 0;
}
extern "C" int f5_workspace_bytes(f5_engine* e, int B, int N, int nt, int steps, int method, size_t* bytes) {
    return workspace_bytes(e, B, N, nt, steps, method, Route{}, bytes);
}
extern "C" int f5_workspace_bytes_rows(f5_engine* e, int B, int N, int nt, int steps, int method, size_t* bytes) {
    return workspace_bytes(e, B, N, nt, steps, method, Route{true, false, false}, bytes);
}
extern "C" int f5_workspace_bytes_dual(f5_engine* e, int B, int N, int nt, int steps, int method, size_t* bytes) {
    return workspace_bytes(e, B, N, nt, steps, method, Route{true, true, false}, bytes);
}
extern "C" int f5_workspace_bytes_window(f5_engine* e, int B, int N, int nt, int steps, int method, int dual, size_t* bytes) {
    return workspace_bytes(e, B, N, nt, steps, method, Route{true, dual != 0, true}, bytes);
}

// ------------------------------------------------------------------------------------------------
// launch context
// ------------------------------------------------------------------------------------------------
// Who writes the 16-bit operand `h` that a block's QKV / FF1 GEMM reads -- one answer per context, not per block:
enum LnMode {
    LN_KERNEL,       // the LN-modulate kernel, a launch of its own (the MX-fp8 blocks: its fp8 twin)
    LN_TAIL,         // the tail fused behind a small-tile residual GEMM (option ln_fusion, gemm.hpp ln_counter)
    LN_FOLD_ROWF,    // LN fold: the residual GEMM leaves x (1 + scale) and slice statistics, a fold_rows launch the row factors
    LN_FOLD_STATS,   // LN fold, statistics form: the consumer GEMM merges the slice statistics itself
    LN_ROWS,         // per-row controls: resid_gate_ln_rows gates the residual and modulates in one row kernel
};
struct LnPlan {
    LnMode mode = LN_KERNEL;
    int fold_state = 0;               // 0 = no fold, 1 = on the staged kernels, 2 = on the batch-1-sized route: f5_engine_ln_fold_active, status bit 1
    const char* refused = nullptr;    // ln_fold = 1 cannot run here: the message (a format that takes the entry point's name), raised by ln_refusal
    bool fold() const { return fold_state != 0; }
};

struct Ctx : LaunchView {
    f5_engine* e;
    Workspace w;
    LnPlan ln;          // decided by make_ctx, once per context
    hipStream_t s;
    int B, N, nt, nb;   // nb = branches evaluated per function evaluation (1 or 2; 1 or 3 with dual guidance)
    int npad;
    bool edit = false;  // f5_sample_edit: conditioning frames are chosen by the mask at w.cond_keep instead of n < lens[b]
    Route route;        // rows: time and guidance strength per batch row (w.r*); dual: three branches F, N, T (w.nbr == 3)
    bool use_mask;
    bool isolate = false;   // engine option isolate_rows in a call with use_mask: conv-pos, the text blocks' conv and GRN stop at each row's duration
    // f5_sample_window: wide (1) / narrow (0) per evaluation, null = every evaluation runs `nb` branches.  A narrow one runs the
    // conditional branch alone and its stage takes k = F for every row (the effective strengths at w.wcfg / w.wacfg are 0 there).
    const uint8_t* pattern = nullptr;
};

// factor folded into q by the QKV epilogue (0 = none): single-segment operand modes only, see run_dit
static float q_premul_factor(const f5_engine* e) {
    return (e->opt.q_premul && e->np == 1) ? (1.0f / sqrtf((float)e->cfg.dim_head)) * 1.4426950408889634f : 0.0f;
}

static F5GemmArgs gemm_base(const Ctx& c, const op16_t* a_hi, const op16_t* a_lo, int lda, const MatBF& w, int M, int N, int K,
                            const float* bias) {
    F5GemmArgs g = c.gemm(a_hi, a_lo, lda, w, M, N, K, bias);
    g.debug_flags = c.e->opt.gemm_flags;      // this engine's own flags (f5_engine_set_option)
    return g;
}

// The LN plan of a context: a function of the engine options, precision, route and nb B N, the rows of one evaluation.
// LN fold (gemm.hpp fold_*): 44 of the 46 LN-modulate launches of a forward disappear into the epilogues of the GEMMs around them
// (the first LN of block 0 follows conv-pos and the final one feeds a small-tile GEMM: both keep the LN kernel).  Only where all
// four block GEMMs of this shape run on the staged kernels, in the one-pass operand modes, with the transposed q / k tiles.
static LnPlan ln_fold_state(const Ctx& c) {
    const f5_engine* e = c.e;
    const f5_config& cf = e->cfg;
    const int D = cf.dim, FF = cf.ff_dim, M = c.nb * c.B * c.N;
    LnPlan p;
    if (c.route.rows) {        // the fold's constants c1, c2 are built per evaluation, not per row; the tail has no per-row form either
        p.mode = LN_ROWS;
        if (e->opt.ln_fold == 1)
            p.refused = c.route.window ? "%s: ln_fold = 1: the folded LN cannot run with per-row sampling controls (its constants are per "
                                         "evaluation); use ln_fold = -1 or 0"
                                       : "ln_fold = 1: the folded LN cannot run with per-row sampling controls (its constants are per evaluation); "
                                         "use ln_fold = -1 or 0 for f5_sample_rows / f5_dit_forward_rows";
        return p;
    }
    F5GemmQuery q = {};
    q.M = M;
    q.seq_len = c.N;
    q.nseg = c.nseg();
    // the fused tail: the out-projection and FF2 are the same launch to the routing (EPI_RESID_GATE, N = ldo = D), so one question serves both
    q.N = D;
    q.epi = EPI_RESID_GATE;
    if (e->prec != F5_PREC_MXFP8 && e->opt.fuse_ln && c.w.lncnt_words != 0 && f5_gemm_resid_ln_fusable(q, D)) p.mode = LN_TAIL;
    if (e->opt.ln_fold == 0) return p;
    // (the fold's constants and statistics are laid out for heads * dim_head == dim, and it was measured on the original family only:
    // 64-channel conv-pos groups, text_dim % 256 == 0 -- docs/geometries.md)
    const bool base_family = cf.heads * cf.dim_head == D && D / cf.conv_pos_groups == 64 && cf.text_dim % 256 == 0;
    bool ok = e->np == 1 && e->prec != F5_PREC_MXFP8 && e->opt.qkv_tr && !e->opt.fuse_ln && D % 256 == 0 && D <= 2048 && FF % 256 == 0 &&
              (e->opt.gemm_flags & 16384) == 0 && cf.depth >= 1 && base_family;
    bool small = ok && D == 1024 && e->opt.fold_stats != 0 && (e->opt.gemm_flags & (8 | 256)) == 0;   // the single-round kernels: statistics form only
    if (ok) {
        q.g4 = true;             // (e->opt.qkv_tr and nseg == 1 are part of `ok`)
        const int shapes[4][2] = {{3 * D, EPI_QKV_ROPE}, {D, EPI_RESID_GATE}, {FF, EPI_GELU_TANH}, {D, EPI_RESID_GATE}};
        for (const auto& sh : shapes) {
            q.N = sh[0];
            q.epi = sh[1];
            ok = ok && f5_gemm_runs_staged(q);
            small = small && f5_gemm_fold_small(q);
        }
    }
    if (e->opt.ln_fold < 0 && !(M >= LN_FOLD_AUTO_ROWS && ok) && !(small && LN_FOLD_SMALL_AUTO)) return p;
    if (!ok && !small)
        p.refused = "ln_fold = 1: this shape / precision cannot run the folded LN (needs f16 or bf16, qkv_transposed, no ln_fusion, dim %% 256 "
                    "== 0, heads * dim_head == dim, 64-channel conv-pos groups, text_dim %% 256 == 0, and all four block GEMMs on the 256x256 / role-split 128x256 kernels -- batch >= 4 at the 335M shape -- or on the "
                    "single-round kernels of the batch-1-sized route: width 1024, fold_stats != 0)";
    p.fold_state = ok ? 1 : (small ? 2 : 0);
    // statistics form: always on the batch-1-sized route (state 2: its kernels have no other), by option on the staged kernels (measured
    // slower there: every tile of a multi-round launch repeats the merge -- +1.9 % at batch 32, +1.6 % at 8, profiles/r06)
    if (p.fold()) p.mode = (p.fold_state == 2 || (e->opt.fold_stats == 1 && D == 1024)) ? LN_FOLD_STATS : LN_FOLD_ROWF;
    return p;
}
// The refusal of a forced fold (return code 2), raised where the entry point's order of refusals puts it; `what` names the entry point.
static int ln_refusal(const Ctx& c, const char* what) {
    // (plan_workspace's predicate contains the LN plan's only while LN_FOLD_SMALL_AUTO is off and nb <= 2: checked, not assumed)
    F5_REQUIRE(!c.ln.fold() || c.w.fold_planned, "internal: the LN fold is on but the workspace plan has no room for it");
    if (!c.ln.refused) return 0;
    f5_set_error(c.ln.refused, what);
    return 2;
}

// loop-invariant preparation: time/adaLN tables, text path, hoisted input projection, masks, rope
static int run_prep(const Ctx& c, int nfe) {
    const f5_engine* e = c.e;
    const f5_config& cf = e->cfg;
    const Workspace& w = c.w;
    const int D = cf.dim, Dt = cf.text_dim, TF = cf.text_ff_dim, L = cf.depth;
    const int M1 = c.B * c.N, M2 = 2 * M1;
    hipStream_t s = c.s;
    const Ops& K = c.ops;

    // --- t-only tables (dit.py:61-82, 267, 286)
    if (nfe > 0) {
        // per-row controls: one table row per (evaluation, batch row), [nfe][B] (f5_launch_skinny_gemm slices any row count by itself)
        const int nt_rows = c.route.rows ? nfe * c.B : nfe;
        const float* tg = c.p<float>(c.route.rows ? w.rtgrid : w.tgrid);
        float *sinus = c.p<float>(c.route.rows ? w.rsinus : w.sinus), *th = c.p<float>(c.route.rows ? w.rth : w.th);
        float *temb = c.p<float>(c.route.rows ? w.rtemb : w.temb), *modt = c.p<float>(c.route.rows ? w.rmod : w.mod);
        RC(f5_launch_time_sinus(tg, sinus, nt_rows, cf.freq_embed_dim, s));
        RC(f5_launch_skinny_gemm(sinus, c.a<float>(e->time_w0), c.a<float>(e->time_b0), th, nt_rows, D, cf.freq_embed_dim, 0, 1, s));
        RC(f5_launch_skinny_gemm(th, c.a<float>(e->time_w2), c.a<float>(e->time_b2), temb, nt_rows, D, D, 0, 0, s));
        RC(f5_launch_skinny_gemm(temb, c.a<float>(e->ada_w), c.a<float>(e->ada_b), modt, nt_rows, (6 * L + 2) * D, D, 1, 0, s));
    }
    if (c.ln.fold_state && nfe > 0) {
        // c1 = W (1 + scale), c2 = W shift + bias for every evaluation and block: QKV against (scale_msa, shift_msa), FF1 against
        // (scale_mlp, shift_mlp); mod rows are [shift_msa, scale_msa, gate_msa, shift_mlp, scale_mlp, gate_mlp] (dit.py:53-58)
        const int FF = cf.ff_dim;
        const size_t vstride = (size_t)(6 * L + 2) * D, ostride = (size_t)L * (3 * D + FF);
        // the 22 blocks of a projection in ONE launch when their weights sit at a uniform stride in the arena (f5_engine::fold_uniform),
        // else block by block
        const long sq = e->fold_stride[0], sf = e->fold_stride[1], sbq = e->fold_stride[2], sbf = e->fold_stride[3];
        const int nlaunch = e->fold_uniform ? 1 : L, count = e->fold_uniform ? L : 1;
        for (int i = 0; i < nlaunch; ++i) {
            const BlockW& bw = e->blocks[i];
            const float* m6 = c.p<float>(w.mod) + (size_t)i * 6 * D;
            float* c1 = c.p<float>(w.foldc[0]) + (size_t)i * (3 * D + FF);
            float* c2 = c.p<float>(w.foldc[1]) + (size_t)i * (3 * D + FF);
            RC(K.fold_consts(c.wm(bw.qkv, 0), bw.qkv.ld, c.a<float>(bw.bqkv), m6 + D, m6, vstride, nfe, c1, c2, ostride, 3 * D, D, s, count,
                             (size_t)sq / 2, (size_t)sbq / 4, (size_t)6 * D, (size_t)(3 * D + FF)));
            RC(K.fold_consts(c.wm(bw.ff1, 0), bw.ff1.ld, c.a<float>(bw.bff1), m6 + 4 * D, m6 + 3 * D, vstride, nfe, c1 + 3 * D, c2 + 3 * D,
                             ostride, FF, D, s, count, (size_t)sf / 2, (size_t)sbf / 4, (size_t)6 * D, (size_t)(3 * D + FF)));
        }
    }
    RC(f5_launch_rope_table(c.p<float>(w.rope_cos), c.p<float>(w.rope_sin), c.N, cf.dim_head, s));
    {
        float* t = c.p<float>(w.rope_t);
        const size_t tn = (size_t)32 * c.N;
        const float qf = q_premul_factor(e);
        RC(f5_launch_rope_table_g4(t, t + 2 * tn, c.N, cf.dim_head, qf != 0.0f ? qf : 1.0f, s));      // q table | k table, 64 N floats each
    }
    RC(f5_launch_rowkeep(c.p<int>(w.dur2), c.p<uint8_t>(w.rowkeep), w.nbr * c.B, c.N, s));
    for (int p = 0; p < e->np; ++p) RC(K.zero_vt_pad(c.pb(w.vt, p), (size_t)w.nbr * c.B * cf.heads * 64, c.N, c.npad, s));

    // --- text path for both branches (dit.py:196-229, convnext_v2.py:46-54)
    // conv_layers == 0 (dit.py:193-194): the plain embedding, no positional table and no masking; text_mask_padding == 0: no masking
    RC(f5_launch_text_embed(c.p<int>(w.text), c.nt, c.a<float>(e->text_table), cf.conv_layers > 0 ? c.a<float>(e->text_pos) : nullptr,
                            cf.text_max_pos, c.p<float>(w.te[0]), c.p<int>(w.ids), c.p<uint8_t>(w.keep), c.B, c.N, Dt,
                            (cf.conv_layers > 0 && cf.text_mask_padding) ? 1 : 0, s));
    int cur = 0;
    for (int i = 0; i < cf.conv_layers; ++i) {
        const TextBlockW& t = e->tblocks[i];
        // isolate_rows: both branches' rows end at their durations (the first 2 B entries of dur2), conv and GRN stop there
        if (c.isolate)
            RC(K.dwconv_ln_ragged(c.p<float>(w.te[cur]), c.a<float>(t.dw_w), c.a<float>(t.dw_b), c.a<float>(t.ln_w), c.a<float>(t.ln_b),
                                  c.pb(w.tln, 0), c.pb(w.tln, 1), 2 * c.B, c.N, Dt, 1e-6f, c.p<int>(w.dur2), s));
        else
            RC(K.dwconv_ln(c.p<float>(w.te[cur]), c.a<float>(t.dw_w), c.a<float>(t.dw_b), c.a<float>(t.ln_w),
                               c.a<float>(t.ln_b), c.pb(w.tln, 0), c.pb(w.tln, 1), 2 * c.B, c.N, Dt, 1e-6f, s));
        F5GemmArgs g1 = gemm_base(c, c.pb(w.tln, 0), c.pb(w.tln, 1), Dt, t.pw1, M2, TF, Dt, c.a<float>(t.b1));
        g1.out_f32 = c.p<float>(w.tg);
        g1.ldo = TF;
        RC(K.gemm(g1, EPI_GELU_ERF, s));
        if (c.isolate)
            RC(K.grn_ragged(c.p<float>(w.tg), c.a<float>(t.gamma), c.a<float>(t.beta), c.p<float>(w.grn_partial), c.p<float>(w.grn_nx),
                            c.pb(w.tg2, 0), c.pb(w.tg2, 1), 2 * c.B, c.N, TF, c.p<int>(w.dur2), s));
        else
            RC(K.grn(c.p<float>(w.tg), c.a<float>(t.gamma), c.a<float>(t.beta), c.p<float>(w.grn_partial),
                         c.p<float>(w.grn_nx), c.pb(w.tg2, 0), c.pb(w.tg2, 1), 2 * c.B, c.N, TF, s));
        F5GemmArgs g2 = gemm_base(c, c.pb(w.tg2, 0), c.pb(w.tg2, 1), TF, t.pw2, M2, Dt, TF, c.a<float>(t.b2));
        g2.out_f32 = c.p<float>(w.te[cur ^ 1]);
        g2.ldo = Dt;
        g2.resid = c.p<float>(w.te[cur]);
        g2.ldres = Dt;
        g2.rowkeep = c.p<uint8_t>(w.keep);
        RC(K.gemm(g2, EPI_RESID_KEEP, s));
        cur ^= 1;
    }
    // --- hoisted part of the input projection: Hc = [cond | text] * Wct^T + b   (dit.py:249-250)
    if (c.route.dual)         // three branches F, N, T; the text path above stays at two
        RC(K.pack_cond_text_dual(c.p<float>(w.cond), c.p<int>(w.lens), c.edit ? c.p<uint8_t>(w.cond_keep) : nullptr, c.p<float>(w.te[cur]),
                                 c.pb(w.ct, 0), c.pb(w.ct, 1), c.B, c.N, cf.mel_dim, Dt, s));
    else if (c.edit)
        RC(K.pack_cond_text_keep(c.p<float>(w.cond), c.p<uint8_t>(w.cond_keep), c.p<float>(w.te[cur]), c.pb(w.ct, 0), c.pb(w.ct, 1),
                                 c.B, c.N, cf.mel_dim, Dt, e->opt.null_keeps_cond, s));
    else
        RC(K.pack_cond_text(c.p<float>(w.cond), c.p<int>(w.lens), c.p<float>(w.te[cur]), c.pb(w.ct, 0), c.pb(w.ct, 1), c.B,
                                c.N, cf.mel_dim, Dt, e->opt.null_keeps_cond, s));
    F5GemmArgs gh = gemm_base(c, c.pb(w.ct, 0), c.pb(w.ct, 1), 128 + Dt, e->wct, w.nbr * M1, D, 128 + Dt, c.a<float>(e->bproj));
    gh.out_f32 = c.p<float>(w.hc);
    gh.ldo = D;
    RC(K.gemm(gh, EPI_F32, s));
    return 0;
}

// ---- one batched DiT forward (the context's nb branches); input = xin (16-bit padded state), modulation row `j`: run_dit below runs the
// input stage, the blocks and the output projection.  What the parts of one evaluation share:
struct DitEval {
    int j;                // the evaluation: row of the fold-constant tables
    const float* mod;     // its modulation vector; per-row controls: vector 0 of the [nfe][B][(6L+2) D] table, the row kernels step through the B vectors
    // LN fold, the one piece of state that travels from GEMM to GEMM: the rows' shift m lives in lnmean[cur_mean]; in the statistics form a
    // consumer reads it, writes the rows' new means into the other half and the halves swap; a fold_rows launch updates lnmean[0] in place
    int cur_mean = 0;
};
static float* ln_mean(const Ctx& c, int which) { return c.p<float>(c.w.lnmean) + (size_t)which * c.nb * c.B * c.N; }

// x = Wx * x_t + Hc  (dit.py:250), all branches share x_t; then x += conv_pos_embed(x)  (dit.py:251)
static int dit_input(const Ctx& c) {
    const f5_engine* e = c.e;
    const f5_config& cf = e->cfg;
    const Workspace& w = c.w;
    const int D = cf.dim, M1 = c.B * c.N;
    F5GemmArgs g0 = gemm_base(c, c.pb(w.xin, 0), c.pb(w.xin, 1), 128, e->wx, c.nb * M1, D, 128, nullptr);
    g0.a_row_mod = M1;
    g0.addrows = c.p<float>(w.hc);
    g0.ldadd = D;
    g0.out_f32 = c.p<float>(w.x);
    g0.ldo = D;
    g0.out_bf[0] = c.pb(w.xb, 0);
    g0.out_bf[1] = c.pb(w.xb, 1);
    g0.ldob = D;
    RC(c.ops.gemm(g0, EPI_ADDROWS, c.s));

    F5ConvPosArgs cp;
    memset(&cp, 0, sizeof(cp));
    cp.B = c.nb * c.B;
    cp.seq_len = c.N;
    cp.C = D;
    cp.groups = cf.conv_pos_groups;
    cp.taps = cf.conv_pos_kernel;
    cp.ld = D;
    cp.ldo = D;
    cp.nseg = c.nseg();
    cp.lens = c.isolate ? c.p<int>(w.dur2) : nullptr;       // isolate_rows: one duration per element of the launch, nb B of dur2's nbr B
    cp.in[0] = c.pb(w.xb, 0);
    cp.in[1] = c.pb(w.xb, 1);
    cp.W[0] = c.wm(e->conv_w[0], 0);
    cp.W[1] = c.wm(e->conv_w[0], 1);
    cp.bias = c.a<float>(e->conv_b[0]);
    cp.mode = 0;
    cp.out_bf[0] = c.pb(w.c1, 0);
    cp.out_bf[1] = c.pb(w.c1, 1);
    RC(c.ops.convpos(cp, c.s));
    cp.in[0] = c.pb(w.c1, 0);
    cp.in[1] = c.pb(w.c1, 1);
    cp.W[0] = c.wm(e->conv_w[1], 0);
    cp.W[1] = c.wm(e->conv_w[1], 1);
    cp.bias = c.a<float>(e->conv_b[1]);
    cp.mode = 1;
    cp.out_bf[0] = cp.out_bf[1] = nullptr;
    cp.out_f32 = c.p<float>(w.x);
    return c.ops.convpos(cp, c.s);
}

// What the QKV projection and the attention of a block are given in either precision.
// q leaves the QKV epilogue multiplied by softmax_scale * log2(e) (one rounding, like the unscaled q): the attention kernels
// then get their scores in exp2 units straight from the matrix cores (attention.hip v2f).  Single-segment operand modes only;
// bf16x3 keeps the unscaled q (hi / lo split of the reference-exact value).  f5_debug_set_q_premul(0) = A/B.
static void dit_qkv_fields(const Ctx& c, F5GemmArgs& g) {
    const Workspace& w = c.w;
    f5_qkv_rope_fields(g, c.pb(w.qk, 0), c.pb(w.qk, 1), c.pb(w.vt, 0), c.pb(w.vt, 1), c.p<float>(w.rope_cos), c.p<float>(w.rope_sin), c.N, c.npad,
                       c.e->cfg.heads, c.e->cfg.heads * c.e->cfg.dim_head, q_premul_factor(c.e));      // "dmodel" = width of the q and k sections
}
static F5AttnArgs dit_attn_args(const Ctx& c, op16_t* out_hi, op16_t* out_lo) {
    const f5_config& cf = c.e->cfg;
    const Workspace& w = c.w;
    return f5_attn_args(c.pb(w.qk, 0), c.pb(w.qk, 1), c.pb(w.vt, 0), c.pb(w.vt, 1), out_hi, out_lo, c.use_mask ? c.p<int>(w.dur2) : nullptr,
                        c.nb * c.B, cf.heads, c.N, c.npad, cf.heads * cf.dim_head, 1.0f / sqrtf((float)cf.dim_head), c.e->np == 2,
                        2 * cf.heads * cf.dim_head, cf.heads * cf.dim_head, q_premul_factor(c.e) != 0.0f, c.e->opt.attn_pipe);
}

// MX-fp8 block: the four GEMMs run on e4m3 operands with E8M0 block scales (v_mfma_scale_f32_32x32x64_f8f6f4); their A
// operands are produced directly in that format by the LN kernel, the attention epilogue and the GELU epilogue.
// q / k / V^T and the attention itself stay bf16, the residual stream fp32.
static int dit_block_f8(const Ctx& c, const DitEval& ev, int i) {
    const f5_engine* e = c.e;
    const Workspace& w = c.w;
    const int D = e->cfg.dim, FF = e->cfg.ff_dim, M = c.nb * c.B * c.N;
    hipStream_t s = c.s;
    const BlockW& bw = e->blocks[i];
    const float* m6 = ev.mod + (size_t)i * 6 * D;
    uint8_t *h8 = c.p<uint8_t>(w.h8), *h8s = c.p<uint8_t>(w.h8s), *ao8 = c.p<uint8_t>(w.ao8), *ao8s = c.p<uint8_t>(w.ao8s);
    auto f8args = [&](const uint8_t* a8, const uint8_t* as, int lda, const MatF8& wm, int N_, int K_, size_t bias) {
        F5GemmArgs g = f5_gemm_f8_args(a8, as, e->arena + wm.q, e->arena + wm.s, lda, wm.ld, M, N_, K_, c.a<float>(bias));
        g.debug_flags = e->opt.gemm_flags;
        return g;
    };
    RC(f5_launch_ln_modulate_f8(c.p<float>(w.x), m6 + D, m6, h8, h8s, M, D, 1e-6f, s));
    F5GemmArgs gq = f8args(h8, h8s, D, bw.qkv8, 3 * D, D, bw.bqkv);
    dit_qkv_fields(c, gq);
    RC(f5_launch_gemm_f8(gq, EPI_QKV_ROPE, s));

    F5AttnArgs at = dit_attn_args(c, nullptr, nullptr);
    at.out8 = ao8;
    at.out8s = ao8s;
    at.ldo8 = D;
    RC(c.ops.attention(at, s));

    F5GemmArgs go = f8args(ao8, ao8s, D, bw.o8, D, D, bw.bo);
    go.out_f32 = c.p<float>(w.x);
    go.ldo = D;
    go.gate = m6 + 2 * D;
    go.rowkeep = c.use_mask ? c.p<uint8_t>(w.rowkeep) : nullptr;
    RC(f5_launch_gemm_f8(go, EPI_RESID_GATE, s));

    RC(f5_launch_ln_modulate_f8(c.p<float>(w.x), m6 + 4 * D, m6 + 3 * D, h8, h8s, M, D, 1e-6f, s));
    F5GemmArgs g1 = f8args(h8, h8s, D, bw.ff1_8, FF, D, bw.bff1);
    g1.out8 = c.p<uint8_t>(w.ffh8);
    g1.out8s = c.p<uint8_t>(w.ffh8s);
    g1.ldo8 = FF;
    RC(f5_launch_gemm_f8(g1, EPI_GELU_TANH, s));
    F5GemmArgs g2 = f8args(g1.out8, g1.out8s, FF, bw.ff2_8, D, FF, bw.bff2);
    g2.out_f32 = c.p<float>(w.x);
    g2.ldo = D;
    g2.gate = m6 + 5 * D;
    return f5_launch_gemm_f8(g2, EPI_RESID_GATE, s);
}

// LN fold, consumer side (QKV: col0 = 0, FF1: col0 = 3 D): the GEMM finishes the LN in its epilogue with the constants of this evaluation
// and block (run_prep), from the row factors or -- statistics form -- from the producer's slice statistics
static void fold_consumer(const Ctx& c, DitEval& ev, F5GemmArgs& g, int i, int col0) {
    const f5_config& cf = c.e->cfg;
    const size_t off = ((size_t)ev.j * cf.depth + i) * (3 * cf.dim + cf.ff_dim) + col0;
    if (c.ln.mode == LN_FOLD_STATS) {
        g.fold_stats = c.p<float>(c.w.lnstats);
        g.fold_stats_ld = c.nb * c.B * c.N;
        g.fold_shift = ln_mean(c, ev.cur_mean);
        g.fold_mean_out = ln_mean(c, ev.cur_mean ^ 1);
        g.fold_eps = 1e-6f;
        ev.cur_mean ^= 1;
    } else {
        g.fold_rowf = c.p<float>(c.w.lnrowf);
    }
    g.fold_c1 = c.p<float>(c.w.foldc[0]) + off;
    g.fold_c2 = c.p<float>(c.w.foldc[1]) + off;
}

// A residual GEMM of a 16-bit block (out-projection, FF2): x += gate * (y * keep), and the LN-modulate (scale, shift) behind it that leaves
// `h`, the operand of the next GEMM -- the one place that acts on the LN plan.  `final`: the LN is the one in front of the output
// projection, which feeds a small mel GEMM: kernel and fold leave it to dit_output, tail and rows produce it here.
static int resid_ln(const Ctx& c, DitEval& ev, F5GemmArgs& g, const float* gate, const uint8_t* keep, const float* scale, const float* shift,
                    bool final) {
    const Workspace& w = c.w;
    const int D = c.e->cfg.dim, M = c.nb * c.B * c.N;
    const LnMode mode = c.ln.mode;
    g.ldo = D;
    if (mode == LN_ROWS) {
        // the GEMM leaves its fp32 result (bias included) in q | k, dead once the attention has run; then x += gate[row] * (keep ? y : 0)
        // and the LN-modulate in one row kernel
        g.out_f32 = reinterpret_cast<float*>(c.pb(w.qk, 0));
        RC(c.ops.gemm(g, EPI_F32, c.s));
        return c.ops.resid_gate_ln_rows(g.out_f32, c.p<float>(w.x), gate, keep, scale, shift, c.pb(w.h, 0), c.pb(w.h, 1), M, D, c.N, c.B,
                                        (size_t)(6 * c.e->cfg.depth + 2) * D, 1e-6f, c.s);
    }
    g.out_f32 = c.p<float>(w.x);
    g.gate = gate;
    g.rowkeep = keep;
    if (mode == LN_TAIL) {        // h = LN(x) (1 + scale) + shift in the same launch
        g.ln_counter = c.p<int>(w.lncnt);
        g.ln_scale = scale;
        g.ln_shift = shift;
        g.ln_out[0] = c.pb(w.h, 0);
        g.ln_out[1] = c.pb(w.h, 1);
        g.ln_eps = 1e-6f;
    }
    const bool fold = c.ln.fold() && !final;
    if (fold) {                   // producer: x (1 + scale) in the operand type in `h`, the row sums in `lnstats`
        g.x16_out = c.pb(w.h, 0);
        g.ldx16 = D;
        g.x16_scale = scale;
        g.x16_shift = ln_mean(c, ev.cur_mean);     // the row's mean at the previous LayerNorm (LN kernel of block 0 / the last consumer / fold_rows)
        g.stats_out = c.p<float>(w.lnstats);
        g.stats_ld = M;
        g.x16_overflow = c.p<int>(w.status);
    }
    RC(c.ops.gemm(g, EPI_RESID_GATE, c.s));
    if (fold && mode == LN_FOLD_ROWF) return c.ops.fold_rows(c.p<float>(w.lnstats), M, D / 64, M, 1e-6f, c.p<float>(w.lnrowf), c.p<float>(w.lnmean), c.s);
    if (mode == LN_KERNEL && !final) return c.ops.ln_modulate(c.p<float>(w.x), scale, shift, c.pb(w.h, 0), c.pb(w.h, 1), M, D, 1e-6f, c.s);
    return 0;
}

// 16-bit block (bf16, f16, bf16x3)
static int dit_block(const Ctx& c, DitEval& ev, int i) {
    const f5_engine* e = c.e;
    const Workspace& w = c.w;
    const int D = e->cfg.dim, FF = e->cfg.ff_dim, L = e->cfg.depth, M = c.nb * c.B * c.N;
    const int I = e->cfg.heads * e->cfg.dim_head;      // attention inner width (dit.py:117-125)
    hipStream_t s = c.s;
    const Ops& K = c.ops;
    const BlockW& bw = e->blocks[i];
    const float* m6 = ev.mod + (size_t)i * 6 * D;  // shift_msa, scale_msa, gate_msa, shift_mlp, scale_mlp, gate_mlp
    if (i == 0) {     // no residual GEMM in front of block 0: its attention LN is a launch of its own, which also seeds the fold's row means
        if (c.ln.mode == LN_ROWS)
            RC(K.resid_gate_ln_rows(nullptr, c.p<float>(w.x), nullptr, nullptr, m6 + D, m6, c.pb(w.h, 0), c.pb(w.h, 1), M, D, c.N, c.B,
                                    (size_t)(6 * L + 2) * D, 1e-6f, s));
        else
            RC(K.ln_modulate(c.p<float>(w.x), m6 + D, m6, c.pb(w.h, 0), c.pb(w.h, 1), M, D, 1e-6f, s, c.ln.fold() ? c.p<float>(w.lnmean) : nullptr));
    }
    F5GemmArgs gq = gemm_base(c, c.pb(w.h, 0), c.pb(w.h, 1), D, bw.qkv, M, 3 * I, D, c.a<float>(bw.bqkv));
    if (c.ln.fold() && i > 0) fold_consumer(c, ev, gq, i, 0);
    dit_qkv_fields(c, gq);
    if (e->opt.qkv_tr) {                             // pair-major tables (the q pair carries qpre, or 1): used by the 256x256 kernel
        gq.rope_g4q = c.p<float>(w.rope_t);
        gq.rope_g4k = gq.rope_g4q + (size_t)64 * c.N;
    }
    RC(K.gemm(gq, EPI_QKV_ROPE, s));
    RC(K.attention(dit_attn_args(c, c.pb(w.ao, 0), c.pb(w.ao, 1)), s));

    F5GemmArgs go = gemm_base(c, c.pb(w.ao, 0), c.pb(w.ao, 1), I, bw.o, M, D, I, c.a<float>(bw.bo));
    RC(resid_ln(c, ev, go, m6 + 2 * D, c.use_mask ? c.p<uint8_t>(w.rowkeep) : nullptr, m6 + 4 * D, m6 + 3 * D, false));
    F5GemmArgs g1 = gemm_base(c, c.pb(w.h, 0), c.pb(w.h, 1), D, bw.ff1, M, FF, D, c.a<float>(bw.bff1));
    if (c.ln.fold()) fold_consumer(c, ev, g1, i, 3 * D);
    g1.out_bf[0] = c.pb(w.ffh, 0);
    g1.out_bf[1] = c.pb(w.ffh, 1);
    g1.ldob = FF;
    RC(K.gemm(g1, EPI_GELU_TANH, s));
    F5GemmArgs g2 = gemm_base(c, c.pb(w.ffh, 0), c.pb(w.ffh, 1), FF, bw.ff2, M, D, FF, c.a<float>(bw.bff2));
    // the LN that follows FF2: the next block's attention LN (shift_msa, scale_msa), or the final one (dit.py:287: scale, shift); no row
    // mask on FF2
    const float* m6n = m6 + 6 * D;
    const bool final = i + 1 == L;
    return resid_ln(c, ev, g2, m6 + 5 * D, nullptr, final ? m6n : m6n + D, final ? m6n + D : m6n, final);
}

// the final LN (unless the last block's FF2 left it: tail, rows) and the mel projection
static int dit_output(const Ctx& c, const DitEval& ev) {
    const f5_config& cf = c.e->cfg;
    const Workspace& w = c.w;
    const int D = cf.dim, M = c.nb * c.B * c.N;
    const float* mf = ev.mod + (size_t)cf.depth * 6 * D;  // final adaLN: (scale, shift) order, dit.py:287
    if (c.ln.mode != LN_TAIL && c.ln.mode != LN_ROWS)
        RC(c.ops.ln_modulate(c.p<float>(w.x), mf, mf + D, c.pb(w.h, 0), c.pb(w.h, 1), M, D, 1e-6f, c.s));
    F5GemmArgs gf = gemm_base(c, c.pb(w.h, 0), c.pb(w.h, 1), D, c.e->wout, M, cf.mel_dim, D, c.a<float>(c.e->bout));
    gf.out_f32 = c.p<float>(w.vel);
    gf.ldo = cf.mel_dim;
    return c.ops.gemm(gf, EPI_F32, c.s);
}

// f5_debug_set_ln_fusion: LN-modulate fused behind the residual GEMMs of small-tile launches (gemm.hpp ln_counter): at batch 1 that
// removes 2 of the 7 launches of a block.  OFF by default: bit-identical, but measured SLOWER at batch 1 (88.5 / 90.3 ms per sample
// against 75.1 / 78.6 on the same boxes, profiles/r02/ln_fusion_ab.txt): a cross-XCD hand-over inside a kernel is three dependent trips
// to the memory side (write-through ack, counter atomic, agent-scope re-read: ~10 us per GEMM) where the separate LN launch costs 5.2 us.
static int run_dit(const Ctx& c, int j) {
    const f5_config& cf = c.e->cfg;
    const size_t vstride = (size_t)(6 * cf.depth + 2) * cf.dim;
    DitEval ev = {j, c.route.rows ? c.p<float>(c.w.rmod) + (size_t)j * c.B * vstride : c.p<float>(c.w.mod) + (size_t)j * vstride};
    RC(dit_input(c));
    for (int i = 0; i < cf.depth; ++i) RC(c.e->prec == F5_PREC_MXFP8 ? dit_block_f8(c, ev, i) : dit_block(c, ev, i));
    return dit_output(c, ev);
}

// steps [i0, i1) of the solve; i0 == 0 also runs the per-call preparation (hoisted tables, text path, first operand pack)
static int run_sample_body(const Ctx& c, const f5_sample_args* a, int i0 = 0, int i1 = 1 << 30) {
    const f5_config& cf = c.e->cfg;
    const Workspace& w = c.w;
    const int mel = cf.mel_dim;
    const size_t M1 = (size_t)c.B * c.N;
    const int per = nfe_per_step(a->method);
    const int nfe = (a->steps - 1) * per;
    hipStream_t s = c.s;
    const Ops& K = c.ops;
    float* traj = c.p<float>(w.traj);
    if (i0 == 0) {
        RC(run_prep(c, nfe));
        RC(K.pack_x(traj, c.pb(w.xin, 0), c.pb(w.xin, 1), (int)M1, mel, s));
    }
    const float* pred = c.p<float>(w.vel);
    const float* nullp = c.nb >= 2 ? pred + M1 * mel : nullptr;
    const float* textp = c.nb == 3 ? pred + 2 * M1 * mel : nullptr;       // dual guidance: the branches are F, N, T
    float* kst = c.p<float>(w.kst);
    float* ytmp = c.p<float>(w.ytmp);
    // per-row controls: every stage reads its row's guidance strength and the step's [B] step sizes
    const float* dt_rows = nullptr;
    // guidance window: evaluation j reads row j of the effective-strength tables, and a narrow one runs the DiT on a one-branch context
    const bool win = c.pattern != nullptr;
    Ctx narrow = c;
    narrow.nb = 1;
    // another row count, so its own LN plan; a window call is a per-row route, which shuts out tail and fold: always the rows mode
    if (win) narrow.ln = ln_fold_state(narrow);
    int jcur = 0;
    auto dit = [&](int j) {
        jcur = j;
        return run_dit(win && !c.pattern[j] ? narrow : c, j);
    };
    auto stage = [&](const F5OdeArgs& o) {
        const float* cfg_rows = win ? c.p<float>(w.wcfg) + (size_t)jcur * c.B : c.p<float>(w.rcfg);
        const float* acfg_rows = win ? c.p<float>(w.wacfg) + (size_t)jcur * c.B : c.p<float>(w.racfg);
        if (c.route.dual) return K.ode_stage_dual(o, textp, acfg_rows, cfg_rows, dt_rows, c.N, c.B, s);
        return c.route.rows ? K.ode_stage_rows(o, cfg_rows, dt_rows, c.N, c.B, s) : K.ode_stage(o, s);
    };
    for (int i = i0; i + 1 < a->steps && i < i1; ++i) {
        if (c.route.rows) dt_rows = c.p<float>(w.rdt) + (size_t)i * c.B;
        float* y = traj + (size_t)i * M1 * mel;
        float* ynext = traj + (size_t)(i + 1) * M1 * mel;
        F5OdeArgs o;
        memset(&o, 0, sizeof(o));
        o.pred = pred;
        o.null_pred = nullp;
        o.cfg_ptr = c.p<float>(w.cfgv);   // staged per call: a by-value scalar would be frozen into the cached hipGraph
        o.base = y;
        o.dt_ptr = c.p<float>(w.dt) + i;
        o.divisor = 1.0f;
        o.rows = (int)M1;
        o.mel_dim = mel;
        o.xin_hi = c.pb(w.xin, 0);
        o.xin_lo = c.pb(w.xin, 1);
        if (a->method == F5_EULER) {
            RC(dit(i));
            o.coef = 1.0f;
            o.out = ynext;
            RC(stage(o));
        } else if (ab_order(a->method)) {
            // the velocities of the last three steps as a ring in w.kst: step i writes slot i % 3 and reads the other two, so no launch
            // reads the buffer it writes; they live in the workspace, so they outlast a graph segment (graph_split)
            RC(dit(i));
            o.coef = 1.0f;
            o.out = ynext;
            o.kstore = kst + (size_t)(i % 3) * M1 * mel;
            if (i > 0) {
                o.mode = 2;
                o.k1 = kst + (size_t)((i + 2) % 3) * M1 * mel;
                o.k2 = (i > 1 && ab_order(a->method) == 3) ? kst + (size_t)((i + 1) % 3) * M1 * mel : nullptr;
                o.abw = c.p<float>(w.abw) + (size_t)3 * i * (c.route.rows ? c.B : 1);
            }
            RC(stage(o));
        } else if (a->method == F5_MIDPOINT) {
            RC(dit(2 * i));
            o.coef = 0.5f;
            o.out = ytmp;
            RC(stage(o));
            RC(dit(2 * i + 1));
            o.coef = 1.0f;
            o.out = ynext;
            RC(stage(o));
        } else {
            RC(dit(4 * i));
            o.coef = 0.5f;
            o.out = ytmp;
            o.kstore = kst;
            RC(stage(o));
            RC(dit(4 * i + 1));
            o.kstore = kst + M1 * mel;
            RC(stage(o));
            RC(dit(4 * i + 2));
            o.coef = 1.0f;
            o.kstore = kst + 2 * M1 * mel;
            RC(stage(o));
            RC(dit(4 * i + 3));
            o.kstore = nullptr;
            o.mode = 1;
            o.divisor = 6.0f;
            o.k1 = kst;
            o.k2 = kst + M1 * mel;
            o.k3 = kst + 2 * M1 * mel;
            o.out = ynext;
            RC(stage(o));
        }
    }
    return 0;
}

static int check_args(const f5_engine* e, const f5_sample_args* a) {
    F5_REQUIRE(e && a, "null argument");
    F5_REQUIRE(e->finalized, "weights are not finalized");
    F5_REQUIRE(a->B >= 1 && a->N >= 1 && a->nt >= 1 && a->steps >= 1, "bad sizes B=%d N=%d nt=%d steps=%d", a->B, a->N, a->nt,
               a->steps);
    // the RoPE / head-split epilogues step through a 4-row group with a single wrap at the sequence boundary
    F5_REQUIRE(a->N >= 4, "sequences shorter than 4 mel frames are not supported (N=%d)", a->N);
    F5_REQUIRE(method_known(a->method), "Unknown method: %d", a->method);
    F5_REQUIRE(a->text && a->cond && a->lens && a->durations && a->workspace, "null pointer in f5_sample_args");
    F5_REQUIRE(((uintptr_t)a->workspace & 255) == 0, "workspace must be 256-byte aligned");
    for (int b = 0; b < a->B; ++b) {
        F5_REQUIRE(a->durations[b] >= 1 && a->durations[b] <= a->N, "durations[%d]=%d out of range [1,%d]", b, a->durations[b],
                   a->N);
        F5_REQUIRE(a->lens[b] >= 0 && a->lens[b] <= a->N, "lens[%d]=%d out of range", b, a->lens[b]);
    }
    return 0;
}

// stage the call's inputs into the workspace (outside any graph: source pointers are caller owned)
static int stage_inputs(Ctx& c, const f5_sample_args* a, const float* x_override, const std::vector<float>& tnfe,
                        const std::vector<float>& dts) {
    const Workspace& w = c.w;
    const size_t M1 = (size_t)c.B * c.N;
    const int mel = c.e->cfg.mel_dim;
    hipStream_t s = c.s;
    // host scalars -> workspace as kernel arguments (no host buffer outlives this call, no host synchronisation)
    const size_t nfe1 = tnfe.empty() ? 1 : tnfe.size();
    std::vector<uint32_t> words(w.scal_words, 0u);
    const size_t nd = (size_t)(1 + w.nbr) * c.B;     // lens and the durations of every branch
    F5_REQUIRE(w.scal_words == (size_t)1 + nd + nfe1 + a->steps + 1 + w.lncnt_words && dts.size() <= (size_t)a->steps,
               "internal: scalar staging layout");
    words[0] = c.ln.fold() ? 2u : 0u;                // status word: bit 1 = the LN fold runs in this call, bit 0 is the kernels'
    uint32_t* wd = words.data() + 1;
    memcpy(wd, a->lens, (size_t)c.B * 4);
    for (int br = 1; br <= w.nbr; ++br)
        for (int b = 0; b < c.B; ++b) wd[br * c.B + b] = (uint32_t)a->durations[b];
    if (!tnfe.empty()) memcpy(wd + nd, tnfe.data(), tnfe.size() * 4);
    if (!dts.empty()) memcpy(wd + nd + nfe1, dts.data(), dts.size() * 4);
    memcpy(wd + nd + nfe1 + a->steps, &a->cfg_strength, 4);
    RC(f5_launch_stage_words(words.data(), words.size(), c.p<uint32_t>(w.scal), s));
    // caller-owned device inputs -> workspace (the captured graph only references the workspace and the arena)
    RC(f5_launch_copy_words(a->text, c.ws + w.text, (size_t)c.B * c.nt, s));
    RC(f5_launch_copy_words(a->cond, c.ws + w.cond, M1 * mel, s));
    const float* x0 = x_override ? x_override : a->y0;
    F5_REQUIRE(x0 != nullptr, "initial state (y0) is null");
    RC(f5_launch_copy_words(x0, c.ws + w.traj, M1 * mel, s));
    return 0;
}

// A strength below 1e-5 is "not guided" (written so that a NaN counts as guided: it reaches the finite checks, not a silent one-branch run).
// -> the branches a call evaluates: 1 when none of the n rows is guided by either strength, else all the route lays out.
static int branch_count(Route route, const float* cfg, const float* audio, int n) {
    for (int b = 0; b < n; ++b)
        if (!(cfg[b] < 1e-5f) || (route.dual && !(audio[b] < 1e-5f))) return route.nbr();
    return 1;
}

static Ctx make_ctx(f5_engine* e, const f5_sample_args* a, hipStream_t s, Route route, int nb) {
    Ctx c;
    c.arena = e->arena;
    c.ws = (char*)a->workspace;
    c.np = e->np;
    c.ops = e->ops;
    c.e = e;
    c.route = route;
    c.w = plan_workspace(e, a->B, a->N, a->nt, a->steps, a->method, route);
    c.s = s;
    c.B = a->B;
    c.N = a->N;
    c.nt = a->nt;
    c.nb = nb;
    c.npad = (a->N + 63) / 64 * 64;
    c.use_mask = a->use_mask != 0;
    c.isolate = c.use_mask && e->opt.isolate_rows != 0;     // without a mask the call has no padding: today's launches
    // nb is final here, except for a window call (stage_controls): a per-row route, whose plan does not read it
    c.ln = ln_fold_state(c);
    return c;
}

// function-evaluation times and step sizes of one time grid in fp32, as the solvers compute them (cfm.py:50-56,76-86,106-114)
static void eval_times(const float* t, int steps, int method, std::vector<float>& tnfe, std::vector<float>& dts) {
    for (int i = 0; i + 1 < steps; ++i) {
        const float t0 = t[i];
        const float dt = t[i + 1] - t0;
        dts.push_back(dt);
        if (method == F5_EULER || ab_order(method)) {
            tnfe.push_back(t0);
        } else if (method == F5_MIDPOINT) {
            tnfe.push_back(t0);
            tnfe.push_back(t0 + 0.5f * dt);
        } else {
            tnfe.push_back(t0);
            tnfe.push_back(t0 + 0.5f * dt);
            tnfe.push_back(t0 + 0.5f * dt);
            tnfe.push_back(t0 + dt);
        }
    }
}

// what a per-row route refuses on top of check_args, before any launch; `what` names the call
static int check_route(const f5_engine* e, Route route, const char* what) {
    if (route.rows) F5_REQUIRE(e->prec != F5_PREC_MXFP8, "%s: precision mxfp8 has no per-row modulation kernels (use f16, bf16 or bf16x3)", what);
    if (route.dual)
        F5_REQUIRE(!e->opt.null_keeps_cond, "%s: engine option null_keeps_cond = 1 gives the second branch the meaning (audio kept, text dropped); "
                   "dual guidance needs it to be (both dropped)", what);
    return 0;
}

// the size query that matches a route, for the "workspace too small" message
static const char* workspace_fn(Route route) {
    if (route.window) return "f5_workspace_bytes_window";
    return route.dual ? "f5_workspace_bytes_dual" : (route.rows ? "f5_workspace_bytes_rows" : "f5_workspace_bytes");
}
static int check_workspace(const Ctx& c, const f5_sample_args* a, const char* what) {
    if (c.route.rows)
        F5_REQUIRE(a->workspace_bytes >= c.w.total, "%s: workspace too small: %zu < %zu (%s)", what, a->workspace_bytes, c.w.total,
                   workspace_fn(c.route));
    else
        F5_REQUIRE(a->workspace_bytes >= c.w.total, "workspace too small: %zu < %zu", a->workspace_bytes, c.w.total);
    return 0;
}

// The controls of one sampling call, whichever entry point it came through: f5_sample (nothing set), f5_sample_edit (cond_keep),
// f5_sample_rows (route.rows: time grid and guidance strength per batch row), f5_sample_dual (route.dual: audio_rows as well) and
// f5_sample_window (route.window: either of the two with the strengths gated per evaluation by each row's time window).  With a mask
// it replaces n < lens[b] in the hoisted input packing and the final splice.
struct RowCtl {
    Route route;
    const char* what;                     // the entry point, for messages
    const uint8_t* cond_keep = nullptr;   // device, [B][N]
    const float* t_rows = nullptr;        // route.rows: [B][steps]
    const float* cfg_rows = nullptr;      // ... [B]; the text strength of dual guidance
    const float* audio_rows = nullptr;    // route.dual: [B]
    const float* lo_rows = nullptr;       // route.window: each row's guidance window [lo, hi] on its own evaluation times
    const float* hi_rows = nullptr;
};

// everything a per-row call refuses before any launch, then the workspace size of every call
static int validate_controls(const Ctx& c, const f5_sample_args* a, const RowCtl& rc) {
    const Route r = rc.route;
    if (r.rows) {
        RC(check_route(c.e, r, rc.what));
        for (size_t i = 0; i < (size_t)a->B * a->steps; ++i)
            F5_REQUIRE(std::isfinite(rc.t_rows[i]), "%s: t_rows[%zu][%zu] is not finite", rc.what, i / a->steps, i % a->steps);
        for (int b = 0; b < a->B; ++b)
            F5_REQUIRE(std::isfinite(rc.cfg_rows[b]), "%s: %s[%d] is not finite", rc.what, (r.dual || r.window) ? "text_cfg_rows" : "cfg_rows", b);
        for (int b = 0; b < a->B && r.dual; ++b)
            F5_REQUIRE(std::isfinite(rc.audio_rows[b]), "%s: audio_cfg_rows[%d] is not finite", rc.what, b);
        for (int b = 0; b < a->B && r.window; ++b) {
            F5_REQUIRE(std::isfinite(rc.lo_rows[b]), "%s: lo_rows[%d] is not finite", rc.what, b);
            F5_REQUIRE(std::isfinite(rc.hi_rows[b]), "%s: hi_rows[%d] is not finite", rc.what, b);
            F5_REQUIRE(rc.lo_rows[b] <= rc.hi_rows[b], "%s: lo_rows[%d] = %g is above hi_rows[%d] = %g", rc.what, b, rc.lo_rows[b], b,
                       rc.hi_rows[b]);
        }
        // (the window call tries the forced-fold refusal before the size, every other call after it)
        if (r.window) RC(ln_refusal(c, rc.what));
    }
    RC(check_workspace(c, a, rc.what));
    return ln_refusal(c, rc.what);
}

// Stages the call's inputs and controls into the workspace.  Per-row routes: the rows words ([tgrid nfe x B | dt steps x B | cfg B
// (| audio B)]); with a window also the effective strengths [nfe][B] text (| [nfe][B] audio) and `pattern`, wide (1) / narrow (0) per
// evaluation, which settles c.nb and becomes c.pattern and the engine's last_pattern.
static int stage_controls(Ctx& c, const f5_sample_args* a, const RowCtl& rc, std::vector<uint8_t>& pattern) {
    const Route r = rc.route;
    hipStream_t s = c.s;
    std::vector<float> tnfe, dts;
    if (!r.rows) {
        eval_times(a->t, a->steps, a->method, tnfe, dts);
        RC(stage_inputs(c, a, nullptr, tnfe, dts));
    } else {
        // every row's own grid through the same fp32 arithmetic, laid out [nfe][B] / [steps - 1][B]; the scalar slots get row 0's
        const int nfe = (a->steps - 1) * nfe_per_step(a->method);
        const size_t rows = (size_t)(nfe > 0 ? nfe : 1) * c.B;
        std::vector<uint32_t> words(c.w.rscal_words, 0u), wtab;
        float* rt = reinterpret_cast<float*>(words.data());
        float* rd = rt + rows;
        for (int b = 0; b < c.B; ++b) {
            std::vector<float> tb, db;
            eval_times(rc.t_rows + (size_t)b * a->steps, a->steps, a->method, tb, db);
            for (size_t j = 0; j < tb.size(); ++j) rt[j * c.B + b] = tb[j];
            for (size_t i = 0; i < db.size(); ++i) rd[i * c.B + b] = db[i];
            if (b == 0) {
                tnfe = tb;
                dts = db;
            }
        }
        memcpy(rd + (size_t)a->steps * c.B, rc.cfg_rows, (size_t)c.B * 4);
        if (r.dual) memcpy(rd + (size_t)a->steps * c.B + c.B, rc.audio_rows, (size_t)c.B * 4);
        if (r.window) {
            // a row's strengths count at evaluation j when lo <= t_eval[j][b] <= hi on the fp32 time staged above (both ends inclusive), else
            // they are 0; an evaluation is wide when any row is left guided (branch_count)
            wtab.assign(c.w.wtab_words, 0u);
            float* wt = reinterpret_cast<float*>(wtab.data());
            float* wa = r.dual ? wt + rows : nullptr;
            pattern.assign((size_t)nfe, 0);
            bool any_wide = false;
            for (int j = 0; j < nfe; ++j)
                for (int b = 0; b < c.B; ++b) {
                    const float tj = rt[(size_t)j * c.B + b];
                    const bool in = rc.lo_rows[b] <= tj && tj <= rc.hi_rows[b];
                    const float ct = in ? rc.cfg_rows[b] : 0.0f, ca = (in && r.dual) ? rc.audio_rows[b] : 0.0f;
                    wt[(size_t)j * c.B + b] = ct;
                    if (wa) wa[(size_t)j * c.B + b] = ca;
                    if (branch_count(r, &ct, &ca, 1) > 1) pattern[j] = 1;
                    any_wide = any_wide || pattern[j];
                }
            c.nb = any_wide ? r.nbr() : 1;
            c.pattern = pattern.data();
            c.e->last_pattern = pattern;
        }
        RC(stage_inputs(c, a, nullptr, tnfe, dts));
        RC(f5_launch_stage_words(words.data(), words.size(), c.p<uint32_t>(c.w.rscal), s));
        if (r.window) RC(f5_launch_stage_words(wtab.data(), wtab.size(), c.p<uint32_t>(c.w.wcfg), s));
    }
    if (ab_order(a->method) && a->steps > 1) {
        // Adams-Bashforth weights of every step, per row on a per-row route ([steps - 1][B][3]); step 0's triple is (1, 0, 0) and is not read
        const int nrow = r.rows ? c.B : 1;
        std::vector<uint32_t> abw(c.w.abw_words, 0u);
        float* wv = reinterpret_cast<float*>(abw.data());
        for (int i = 0; i + 1 < a->steps; ++i)
            for (int b = 0; b < nrow; ++b)
                ab_weights(r.rows ? rc.t_rows + (size_t)b * a->steps : a->t, i, ab_order(a->method), wv + ((size_t)i * nrow + b) * 3);
        RC(f5_launch_stage_words(abw.data(), abw.size(), c.p<uint32_t>(c.w.abw), s));
    }
    // the mask travels like text / cond / y0: copied into the workspace outside the captured part, so one graph serves every mask of a shape
    if (c.edit) RC(f5_launch_copy_bytes(rc.cond_keep, c.ws + c.w.cond_keep, (size_t)c.B * c.N, s));
    return 0;
}

// hipGraph cache key: everything a captured node depends on BY VALUE: shapes, solver, branch count, masking, the route, the launch knobs and
// options, and the workspace address.  Per-call scalars (cfg strength, time grid, dt) are read from workspace memory staged before.
static std::string graph_key(const Ctx& c, const f5_sample_args* a, const std::vector<uint8_t>& pattern) {
    char shape_key[192];
    snprintf(shape_key, sizeof(shape_key), "B%d N%d nt%d st%d m%d nb%d mask%d edit%d rows%d dual%d ke%d ws%p opt", c.B, c.N, c.nt, a->steps,
             a->method, c.nb, (int)c.use_mask, (int)c.edit, (int)c.route.rows, (int)c.route.dual, g_knob_epoch, a->workspace);
    std::string key(shape_key);
    for (const OptDesc& o : k_options) key += " " + std::to_string(c.e->opt.*o.member);
    if (c.pattern) {
        // the wide / narrow pattern decides which evaluations run one branch: structural, so part of the key (nfe bits as hex); the
        // strengths and bounds behind it are staged values and are not
        key += " win";
        static const char hex[] = "0123456789abcdef";
        for (size_t j = 0; j < pattern.size(); j += 4) {
            int v = 0;
            for (size_t k = j; k < j + 4 && k < pattern.size(); ++k) v |= pattern[k] << (k - j);
            key += hex[v];
        }
    }
    return key;
}

// the solve -- eager, or a cached / freshly captured hipGraph under `key` -- and the final splice into the caller's buffers
static int launch_sample(const Ctx& c, const f5_sample_args* a, const std::string& key) {
    f5_engine* e = c.e;
    hipStream_t s = c.s;
    const bool graph_on = a->use_graph == F5_GRAPH_ON, graph_auto = a->use_graph == F5_GRAPH_AUTO;
    GraphCache::Entry* entry = (graph_on || graph_auto) ? e->graphs.find(key, a->workspace) : nullptr;
    bool graph = graph_on || entry != nullptr;
    if (graph_auto && !entry) {
        // a text-to-speech service sees a new (N, nt) on almost every call and capture + instantiate of ~5000 nodes costs more
        // than one eager pass: run a signature eagerly the first time, capture it when it comes back
        for (auto& k : e->seen) graph |= k == key;
        if (!graph) {
            if (e->seen.size() >= 64) e->seen.erase(e->seen.begin());
            e->seen.push_back(key);
        }
    }
    if (graph) {
        if (!entry) {
            // segments: the whole call, or (graph_split) one per ODE step
            const int nseg = (e->opt.graph_split && a->steps > 2) ? a->steps - 1 : 1;
            RC(e->graphs.capture(key, a->workspace, s, nseg,
                                 [&](int sg) { return nseg == 1 ? run_sample_body(c, a) : run_sample_body(c, a, sg, sg + 1); }, &entry));
        }
        RC(GraphCache::launch(entry, s));
    } else {
        RC(run_sample_body(c, a));
    }
    const int mel = e->cfg.mel_dim;
    const size_t M1 = (size_t)c.B * c.N;
    const float* ylast = c.p<float>(c.w.traj) + (size_t)(a->steps - 1) * M1 * mel;
    if (c.edit)
        RC(f5_launch_splice_keep(c.p<float>(c.w.cond), ylast, c.p<uint8_t>(c.w.cond_keep), a->out, c.B, c.N, mel, s));
    else
        RC(f5_launch_splice(c.p<float>(c.w.cond), ylast, c.p<int>(c.w.lens), a->out, c.B, c.N, mel, s));
    if (a->trajectory) RC(f5_launch_copy_words(c.ws + c.w.traj, a->trajectory, (size_t)a->steps * M1 * mel, s));
    return 0;
}

// engine option isolate_rows on a precision the row-isolated mode is not claimed for; `what` names the call
static int check_isolate(const f5_engine* e, const char* what) {
    F5_REQUIRE(!(e && e->opt.isolate_rows && e->prec == F5_PREC_MXFP8),
               "%s: engine option isolate_rows = 1 is not supported in precision mxfp8 (row isolation is claimed for f16, bf16 and bf16x3); set "
               "isolate_rows = 0", what);
    return 0;
}

static int sample_impl(f5_engine* e, const f5_sample_args* a, void* stream, const RowCtl& rc) {
    RC(check_isolate(e, rc.what));
    RC(check_args(e, a));
    F5_REQUIRE(a->y0 && (a->t || rc.route.rows) && a->out, "null pointer in f5_sample_args (y0/t/out)");
    // (a window call's branch count is settled by stage_controls, once the evaluation times say which evaluations are wide)
    const int nb = rc.route.rows ? branch_count(rc.route, rc.cfg_rows, rc.audio_rows, a->B) : branch_count(rc.route, &a->cfg_strength, nullptr, 1);
    Ctx c = make_ctx(e, a, (hipStream_t)stream, rc.route, nb);
    c.edit = rc.cond_keep != nullptr;
    RC(validate_controls(c, a, rc));
    SatScope sat(e->prec == F5_PREC_F16 && e->opt.sat_check, c.p<int>(c.w.status));
    std::vector<uint8_t> pattern;       // f5_sample_window: wide / narrow per evaluation (c.pattern points into it)
    RC(stage_controls(c, a, rc, pattern));
    return launch_sample(c, a, graph_key(c, a, pattern));
}
extern "C" int f5_sample(f5_engine* e, const f5_sample_args* a, void* stream) { return sample_impl(e, a, stream, RowCtl{Route{}, "f5_sample"}); }
extern "C" int f5_sample_edit(f5_engine* e, const f5_sample_args* a, const uint8_t* cond_keep_dev, void* stream) {
    F5_REQUIRE(cond_keep_dev, "f5_sample_edit: cond_keep is null");
    return sample_impl(e, a, stream, RowCtl{Route{}, "f5_sample_edit", cond_keep_dev});
}
extern "C" int f5_sample_rows(f5_engine* e, const f5_sample_args* a, const f5_row_controls* rc, void* stream) {
    F5_REQUIRE(rc != nullptr, "f5_sample_rows: controls is null");
    F5_REQUIRE(rc->t_rows != nullptr, "f5_sample_rows: controls.t_rows is null");
    F5_REQUIRE(rc->cfg_rows != nullptr, "f5_sample_rows: controls.cfg_rows is null");
    return sample_impl(e, a, stream, RowCtl{Route{true, false, false}, "f5_sample_rows", rc->cond_keep_dev, rc->t_rows, rc->cfg_rows});
}
extern "C" int f5_sample_dual(f5_engine* e, const f5_sample_args* a, const f5_dual_controls* dc, void* stream) {
    F5_REQUIRE(dc != nullptr, "f5_sample_dual: controls is null");
    F5_REQUIRE(dc->t_rows != nullptr, "f5_sample_dual: controls.t_rows is null");
    F5_REQUIRE(dc->text_cfg_rows != nullptr, "f5_sample_dual: controls.text_cfg_rows is null");
    F5_REQUIRE(dc->audio_cfg_rows != nullptr, "f5_sample_dual: controls.audio_cfg_rows is null");
    return sample_impl(e, a, stream,
                       RowCtl{Route{true, true, false}, "f5_sample_dual", dc->cond_keep_dev, dc->t_rows, dc->text_cfg_rows, dc->audio_cfg_rows});
}
extern "C" int f5_sample_window(f5_engine* e, const f5_sample_args* a, const f5_window_controls* wc, void* stream) {
    F5_REQUIRE(wc != nullptr, "f5_sample_window: controls is null");
    F5_REQUIRE(wc->t_rows != nullptr, "f5_sample_window: controls.t_rows is null");
    F5_REQUIRE(wc->text_cfg_rows != nullptr, "f5_sample_window: controls.text_cfg_rows is null");
    F5_REQUIRE(wc->lo_rows != nullptr, "f5_sample_window: controls.lo_rows is null");
    F5_REQUIRE(wc->hi_rows != nullptr, "f5_sample_window: controls.hi_rows is null");
    return sample_impl(e, a, stream, RowCtl{Route{true, wc->audio_cfg_rows != nullptr, true}, "f5_sample_window", wc->cond_keep_dev, wc->t_rows,
                                            wc->text_cfg_rows, wc->audio_cfg_rows, wc->lo_rows, wc->hi_rows});
}
extern "C" int f5_debug_last_sample_pattern(f5_engine* e, int* nfe, uint8_t* wide, int cap) {
    F5_REQUIRE(e && nfe, "null argument");
    F5_REQUIRE(cap == 0 || wide, "f5_debug_last_sample_pattern: wide is null with cap = %d", cap);
    *nfe = (int)e->last_pattern.size();
    for (int j = 0; j < cap && j < *nfe; ++j) wide[j] = e->last_pattern[j];
    return 0;
}

// Status word of the last f5_sample / f5_dit_forward that used this workspace (its FIRST 32-bit word, for every shape and solver):
// bit 1 = the LN fold ran in that call; bit 0 = a value of the folded operand (x - m)(1 + scale) did not fit fp16 (precision f16): the
// result is saturated there -- rerun with the engine option ln_fold = 0 (or in bf16).  f5_sample_status synchronises the stream;
// f5_sample_status_async only enqueues the 4-byte copy (flags should be pinned host memory; read it after the caller's own
// synchronisation / event): no host block per call.
extern "C" int f5_sample_status_async(f5_engine* e, const f5_sample_args* a, int* flags, void* stream) {
    F5_REQUIRE(e && a && flags && a->workspace && a->workspace_bytes >= 4, "null argument");
    F5_HIP_CHECK(hipMemcpyAsync(flags, (const char*)a->workspace, 4, hipMemcpyDeviceToHost, (hipStream_t)stream));
    return 0;
}
// 1 when f5_sample with these arguments runs the LN fold (engine option "ln_fold", sizes, precision, branch count of cfg_strength) --
// the only configuration that can set bit 0 of the status word; host-side, no GPU work.  f5_dit_forward: pass steps = 2, method = F5_EULER.
extern "C" int f5_engine_ln_fold_active(f5_engine* e, const f5_sample_args* a, int* active) {
    F5_REQUIRE(e && a && active, "null argument");
    F5_REQUIRE(a->B >= 1 && a->N >= 1 && a->nt >= 1 && a->steps >= 1 && method_known(a->method), "bad sizes");
    const Ctx c = make_ctx(e, a, nullptr, Route{}, branch_count(Route{}, &a->cfg_strength, nullptr, 1));
    RC(ln_refusal(c, ""));
    *active = c.ln.fold_state;
    return 0;
}
extern "C" int f5_sample_status(f5_engine* e, const f5_sample_args* a, int* flags, void* stream) {
    RC(f5_sample_status_async(e, a, flags, stream));
    F5_HIP_CHECK(hipStreamSynchronize((hipStream_t)stream));
    return 0;
}

// One function evaluation.  t: the time (one float), or with a per-row route one time per batch row, [B] host floats.  outs: where the
// branches go, in the engine's order F, N, T; a null entry, or one beyond the branches that ran, is not written.  Two branches when
// args->cfg_strength is a guiding one, else one -- dual guidance always runs all three and does not read it.
static int forward_impl(f5_engine* e, const f5_sample_args* a, const float* x, const float* t, Route route, float* const outs[3],
                        const char* what, void* stream) {
    RC(check_isolate(e, what));
    RC(check_args(e, a));
    F5_REQUIRE(x && outs[0], "null pointer");
    if (route.rows) {
        F5_REQUIRE(t != nullptr, "%s: t_rows is null", what);
        RC(check_route(e, route, what));
        for (int b = 0; b < a->B; ++b) F5_REQUIRE(std::isfinite(t[b]), "%s: t_rows[%d] is not finite", what, b);
    }
    hipStream_t s = (hipStream_t)stream;
    f5_sample_args a2 = *a;
    a2.steps = 2;
    a2.method = F5_EULER;
    Ctx c = make_ctx(e, &a2, s, route, route.dual ? 3 : branch_count(route, &a2.cfg_strength, nullptr, 1));
    RC(check_workspace(c, a, what));
    RC(ln_refusal(c, what));
    const int mel = e->cfg.mel_dim;
    const size_t M1 = (size_t)c.B * c.N;
    SatScope sat(e->prec == F5_PREC_F16 && e->opt.sat_check, c.p<int>(c.w.status));
    std::vector<float> tnfe(1, t[0]), dts(1, 0.0f);
    RC(stage_inputs(c, &a2, x, tnfe, dts));
    if (route.rows) {
        std::vector<uint32_t> words(c.w.rscal_words, 0u);       // [tgrid B | dt 2 B | cfg B (| audio B)]: only the times are read by a forward
        memcpy(words.data(), t, (size_t)c.B * 4);
        RC(f5_launch_stage_words(words.data(), words.size(), c.p<uint32_t>(c.w.rscal), s));
    }
    RC(run_prep(c, 1));
    RC(c.ops.pack_x(c.p<float>(c.w.traj), c.pb(c.w.xin, 0), c.pb(c.w.xin, 1), (int)M1, mel, s));
    RC(run_dit(c, 0));
    for (int br = 0; br < c.nb; ++br)
        if (outs[br]) RC(f5_launch_copy_words(c.ws + c.w.vel + (size_t)br * M1 * mel * 4, outs[br], M1 * mel, s));
    return 0;
}

extern "C" int f5_dit_forward(f5_engine* e, const f5_sample_args* a, const float* x, float t, float* pred, float* null_pred,
                              void* stream) {
    float* const outs[3] = {pred, null_pred, nullptr};
    return forward_impl(e, a, x, &t, Route{}, outs, "f5_dit_forward", stream);
}
// f5_dit_forward with one time per batch row (the reference's DiT takes `time` as (b,), dit.py:374-401): one batched forward where the
// scalar entry point needs one call per distinct time.  Workspace: f5_workspace_bytes_rows with steps = 2, method = F5_EULER.
extern "C" int f5_dit_forward_rows(f5_engine* e, const f5_sample_args* a, const float* x, const float* t_rows_host, float* pred,
                                   float* null_pred, void* stream) {
    float* const outs[3] = {pred, null_pred, nullptr};
    return forward_impl(e, a, x, t_rows_host, Route{true, false, false}, outs, "f5_dit_forward_rows", stream);
}
// One evaluation of the three branches of dual guidance, one time per batch row: pred = F (audio and text kept), null_pred = N (both
// dropped), text_pred = T (audio dropped, text kept).  Workspace: f5_workspace_bytes_dual with steps = 2, method = F5_EULER.
extern "C" int f5_dit_forward_dual(f5_engine* e, const f5_sample_args* a, const float* x, const float* t_rows_host, float* pred,
                                   float* null_pred, float* text_pred, void* stream) {
    float* const outs[3] = {pred, null_pred, text_pred};
    return forward_impl(e, a, x, t_rows_host, Route{true, true, false}, outs, "f5_dit_forward_dual", stream);
}

// ------------------------------------------------------------------------------------------------
// per-op entry points
// ------------------------------------------------------------------------------------------------
// Test hooks.  They live in both kernel builds (bf16 / fp16 operands) and are process-wide: meant for the op-level tests and the
// A/B tools, which set them once; a change bumps g_knob_epoch, so no cached hipGraph captured under other values is replayed.
// They choose only among the kernels sample() itself can reach (tile shapes, attention workgroup shapes, conv-pos pipeline step,
// tile numbering).
#define F5_DECL_KNOB(v) namespace f5bf { extern int v; } namespace f5hf { extern int v; }
#define F5_SET_BOTH(v, x) do { f5bf::v = (x); f5hf::v = (x); ++g_knob_epoch; } while (0)
#define F5_SET_ROUTE_KNOB(v, x) do { f5dbg::gemm_knobs.v = (x); ++g_knob_epoch; } while (0)    // gemm_route.hpp: one object for both builds
F5_DECL_KNOB(f5_convpos_tps)
F5_DECL_KNOB(f5_convpos_xcd_map)
F5_DECL_KNOB(f5_attn_wide)
F5_DECL_KNOB(f5_attn_kvsplit)
F5_DECL_KNOB(f5_attn_pipe)
F5_DECL_KNOB(f5_gemm_order)
F5_DECL_KNOB(f5_gemm_nband)
F5_DECL_KNOB(f5_gemm_debug_flags)
extern "C" int f5_op_set_operand_type(int fp16) {
    F5_REQUIRE(fp16 == 0 || fp16 == 1, "operand type must be 0 (bf16) or 1 (fp16)");
    g_ops.h = fp16 != 0;
    return 0;
}
extern "C" int f5_op_get_operand_type(void) { return g_ops.h ? 1 : 0; }
// host-side conversions used by f5_load_tensor, exported for the CPU tests (no GPU needed)
extern "C" uint16_t f5_debug_f2h_bits(float f) { return f5_f2h_bits(f); }
extern "C" float f5_debug_h_bits2f(uint16_t h) { return f5_h_bits2f(h); }
extern "C" uint16_t f5_debug_f2bf_bits(float f) { return f5_f2bf_bits(f); }
extern "C" int f5_debug_set_convpos_tps(int v) {
    F5_REQUIRE(v == 0 || v == 1 || v == 2 || v == 4 || v == 8, "conv-pos taps per pipeline step must be 0 (auto), 1, 2, 4 or 8 (the ring kernel)");
    F5_SET_BOTH(f5_convpos_tps, v);
    return 0;
}
extern "C" int f5_debug_set_convpos_xcd_map(int on) {
    F5_SET_BOTH(f5_convpos_xcd_map, on ? 1 : 0);
    return 0;
}
// process DEFAULTS of the per-engine options (f5_engine_set_option changes one engine; engines that already exist keep theirs)
static void warn_defaults_only(const char* hook, const char* option) {
    if (g_live_engines > 0)
        fprintf(stderr, "[f5tts_hip] %s changes the default of NEW engines only: %d engine(s) already exist and keep their value "
                        "(use f5_engine_set_option(e, \"%s\", v) for those)\n", hook, g_live_engines, option);
}
extern "C" int f5_debug_set_ln_fusion(int on) {
    warn_defaults_only("f5_debug_set_ln_fusion", "ln_fusion");
    g_default_options.fuse_ln = on ? 1 : 0;
    return 0;
}
extern "C" int f5_debug_set_qkv_transposed(int on) {
    warn_defaults_only("f5_debug_set_qkv_transposed", "qkv_transposed");
    g_default_options.qkv_tr = on ? 1 : 0;
    return 0;
}
extern "C" int f5_debug_set_q_premul(int on) {
    warn_defaults_only("f5_debug_set_q_premul", "q_premul");
    g_default_options.q_premul = on ? 1 : 0;
    return 0;
}
extern "C" int f5_debug_set_attn_wide(int v) {
    F5_REQUIRE(v >= -1 && v <= 1, "attention wide-workgroup switch must be -1 (auto), 0 or 1 (256-query workgroups)");
    F5_SET_BOTH(f5_attn_wide, v);
    return 0;
}
extern "C" int f5_debug_set_attn_pipe(int v) {
    F5_REQUIRE(v == 0 || v == 1, "attention pipelining switch must be 0 (v2f) or 1 (v2p: in-wave software pipeline, one wave per SIMD)");
    F5_SET_BOTH(f5_attn_pipe, v);
    return 0;
}
extern "C" int f5_debug_set_attn_kvsplit(int v) {
    F5_REQUIRE(v == -1 || v == 1 || v == 2 || v == 4, "attention KV split must be -1 (auto), 1, 2 or 4");
    F5_SET_BOTH(f5_attn_kvsplit, v);
    return 0;
}
extern "C" int f5_debug_set_gemm_qkv_tile(int v) {
    F5_REQUIRE(v == 0 || v == 1 || v == 12 || v == 13 || v == 14, "small-M QKV tile must be 0 (auto), 1 (small tiles), 12 / 13 (8-wave 128x256 ring) or 14 (role-split 128x256)");
    F5_SET_ROUTE_KNOB(qkv_tile, v);
    return 0;
}
extern "C" int f5_debug_set_gemm_nband(int v) {
    F5_REQUIRE(v >= 0 && v <= 16, "column-tile band width of the 256x256 tile numbering must be 0 (n fastest) .. 16");
    F5_SET_BOTH(f5_gemm_nband, v);
    return 0;
}
extern "C" int f5_debug_set_gemm_ring(int v) {
    F5_SET_ROUTE_KNOB(ring, v ? 1 : 0);
    return 0;
}
extern "C" int f5_debug_set_gemm_order(int v) {
    F5_REQUIRE(v >= 0 && v <= 3, "gemm order must be 0 (auto), 1 (n fastest), 2 (m fastest) or 3 (band-major where it applies)");
    F5_SET_BOTH(f5_gemm_order, v);
    return 0;
}
// process-wide GEMM flags, OR-ed into every GEMM launch of the process (op-level tests, A/B tools); an engine's own flags are
// f5_engine_set_option(e, "gemm_flags", v)
extern "C" int f5_debug_set_gemm_flags(int v) {
    F5_SET_BOTH(f5_gemm_debug_flags, v);
    return 0;
}
namespace f5dbg {
int last_gemm_kernel = 0;
int last_attn_kernel = 0;
int last_convpos_kernel = 0;
}
static int copy_name(const std::string& s, char* buf, int n) {
    if (buf != nullptr && n > 0) {
        strncpy(buf, s.c_str(), (size_t)n - 1);
        buf[n - 1] = 0;
    }
    return (int)s.size();
}
// name of the kernel the most recent f5_launch_gemm of the process resolved to ("" = it refused the launch); returns its length
extern "C" int f5_debug_last_gemm_kernel(char* buf, int n) {
    return copy_name(f5_gemm_kernel_name(f5dbg::last_gemm_kernel), buf, n);
}
// name of the kernel the most recent f5_launch_attention of the process launched (one per instantiation, "+f8" when the launch carried
// the MX-fp8 output; "" = it refused the launch); returns its length
extern "C" int f5_debug_last_attn_kernel(char* buf, int n) {
    static const char* const names[] = {"", "f5_attn2_kernel<true,0>", "f5_attn2_kernel<false,0>", "f5_attn2f_kernel<true>", "f5_attn2f_kernel<false>",
                                        "f5_attn2p_kernel", "f5_attn2s_kernel<true,2,2>", "f5_attn2s_kernel<false,2,3,true>",
                                        "f5_attn2s_kernel<false,4,2,true>"};
    const int k = f5dbg::last_attn_kernel & (F5A_OUT8 - 1);
    std::string s = k <= F5A_V2S_KS4 ? names[k] : "";
    if (k != F5A_NONE && (f5dbg::last_attn_kernel & F5A_OUT8)) s += "+f8";
    return copy_name(s, buf, n);
}
// name of an F5ConvPosKernel word, "+xcd" appended when it carries F5CP_XCD
static std::string convpos_kernel_name(int word) {
    static const char* const names[] = {"", "f5_convpos_kernel<false,1>", "f5_convpos_kernel<false,2>", "f5_convpos_kernel<false,4>",
                                        "f5_convpos_kernel<true,1>", "f5_convpos_kernel<true,2>", "f5_convpos_ring_kernel"};
    const int k = word & (F5CP_XCD - 1);
    std::string s = k <= F5CP_RING ? names[k] : "";
    if (k != F5CP_NONE && k != F5CP_RING && (word & F5CP_N48)) s.insert(s.size() - 1, ",48");     // f5_convpos_kernel<false,1,48>
    if (k != F5CP_NONE && (word & F5CP_XCD)) s += "+xcd";
    return s;
}
// name of the instantiation the most recent f5_launch_convpos of the process launched, "+xcd" appended when the 1-D block numbering
// ran ("" = it refused the launch); returns its length
extern "C" int f5_debug_last_convpos_kernel(char* buf, int n) { return copy_name(convpos_kernel_name(f5dbg::last_convpos_kernel), buf, n); }
// The name a conv-pos launch of this shape would report under the current selectors, without launching anything or touching a device
// (f5_convpos_route is the launcher's own decision; the selectors are the same in both operand builds)
extern "C" int f5_debug_convpos_route(int B, int seq_len, int groups, int nseg, char* buf, int n) {
    return f5_debug_convpos_route_groups(B, seq_len, groups, 64, nseg, buf, n);
}
// the same for `groups` groups of cpg = 32, 48 or 64 channels (narrow groups never reach the ring kernel)
extern "C" int f5_debug_convpos_route_groups(int B, int seq_len, int groups, int cpg, int nseg, char* buf, int n) {
    F5_REQUIRE(B > 0 && seq_len > 0 && groups > 0 && (nseg == 1 || nseg == 3), "convpos route: bad shape");
    F5_REQUIRE(cpg == 64 || cpg == 48 || (cpg == 32 && groups % 2 == 0), "convpos route: channels per group must be 32, 48 or 64");
    copy_name(convpos_kernel_name(f5bf::f5_convpos_route(B, seq_len, groups, nseg, cpg)), buf, n);
    return 0;
}
// The route (gemm_route.hpp) a GEMM launch of this shape would take under the current knobs and process-wide flags, without launching
// anything or touching a device.  variant_bits: 1 = group-major rotation tables, 2 = fused LN tail, 4 = LN-fold producer, 8 = consumer in
// the statistics form, 16 = consumer with row factors.  -> length of the kernel name (as f5_debug_last_gemm_kernel would report it), or
// -1 when the launch would be refused (f5_last_error says why); facts (optional): bit 0 staged, 1 fold-small, 2 resid-LN-fusable
extern "C" int f5_debug_gemm_route(int epi, int M, int N, int nseg, int seq_len, int variant_bits, int debug_flags, char* name, int n, int* facts) {
    F5_REQUIRE(epi >= EPI_F32 && epi <= EPI_GELU_ERF_BF16 && M >= 1 && N >= 1, "gemm route: bad epilogue %d or shape M=%d N=%d", epi, M, N);
    const F5GemmQuery q = {epi, M, N, nseg, seq_len, (variant_bits & 1) != 0, (variant_bits & 2) != 0, (unsigned)(variant_bits >> 2) & 7u,
                           debug_flags | f5bf::f5_gemm_debug_flags};     // (F5_SET_BOTH keeps the fp16 build's copy equal)
    const F5GemmRoute r = f5_gemm_route(q);
    if (facts != nullptr) *facts = (r.staged ? 1 : 0) | (r.fold_small ? 2 : 0) | (r.ln_fusable ? 4 : 0);
    if (r.kernel == F5K_NONE) {
        f5_set_error("%s", r.refused);
        return -1;
    }
    return copy_name(f5_gemm_kernel_name(f5_gemm_reached(r.kernel, q)), name, n);
}
extern "C" int f5_debug_set_gemm_tile(int sel) {
    F5_REQUIRE(sel >= 0 && sel <= 14, "gemm tile override must be 0 (auto) .. 14");
    F5_REQUIRE(sel != 7, "gemm tile 7 does not exist (tiles are 0 .. 6 and 8 .. 14)");
    F5_SET_ROUTE_KNOB(tile, sel);
    return 0;
}

// op-level twins of the LN fold (gemm.hpp fold_*): what run_dit sets on its block GEMMs, for the per-op entry points
static struct {
    const float* next_scale = nullptr;       // producer: f5_op_gemm_resid_gate
    op16_t* x16 = nullptr;
    float* stats_out = nullptr;
    const float* row_shift = nullptr;
    float* ln_mean_out = nullptr;            // f5_op_ln_modulate: the row means (the first folded operand's shift)
    const float* rowf = nullptr;             // consumer: f5_op_gemm (epi 2), f5_op_qkv_rope
    const float* c1 = nullptr;
    const float* c2 = nullptr;
} g_op_fold;
extern "C" int f5_debug_set_op_fold_producer(const float* next_scale, void* x16_out, float* stats_out, const float* row_shift) {
    g_op_fold.next_scale = next_scale;
    g_op_fold.x16 = (op16_t*)x16_out;
    g_op_fold.stats_out = stats_out;
    g_op_fold.row_shift = row_shift;
    return 0;
}
extern "C" int f5_debug_set_op_ln_mean_out(float* mean_out) {
    g_op_fold.ln_mean_out = mean_out;
    return 0;
}
// op-level tests: where the 16-bit packers of the f5_op_* launches that follow report saturation (fp16 operand build; null = nowhere)
extern "C" int f5_debug_set_op_sat_flag(int* flag) {
    f5hf::f5_sat_flag_host = flag;
    return 0;
}
static int* g_op_fold_overflow = nullptr;
extern "C" int f5_debug_set_op_fold_overflow_flag(int* flag) {
    g_op_fold_overflow = flag;
    return 0;
}
extern "C" int f5_debug_set_op_fold_consumer(const float* rowf, const float* c1, const float* c2) {
    g_op_fold.rowf = rowf;
    g_op_fold.c1 = c1;
    g_op_fold.c2 = c2;
    return 0;
}
// the statistics form (gemm.hpp fold_stats): the consumers of the f5_op_* launches that follow merge the producer's slice statistics
// themselves; stats = the producer's stats_out ([16][ld][2]), shift = what it subtracted (or NULL), mean_out = where column tile 0
// writes the rows' means (or NULL).  Takes the place of `rowf` of f5_debug_set_op_fold_consumer (set that one with rowf = NULL).
static struct { const float* stats; int ld; const float* shift; float* mean_out; } g_op_fold_stats = {nullptr, 0, nullptr, nullptr};
extern "C" int f5_debug_set_op_fold_stats(const float* stats, int ld, const float* shift, float* mean_out) {
    g_op_fold_stats = {stats, ld, shift, mean_out};
    return 0;
}
static void op_fold_consumer(F5GemmArgs& g) {
    g.fold_rowf = g_op_fold.rowf;
    g.fold_c1 = g_op_fold.c1;
    g.fold_c2 = g_op_fold.c2;
    if (g_op_fold.rowf == nullptr) {
        g.fold_stats = g_op_fold_stats.stats;
        g.fold_stats_ld = g_op_fold_stats.ld;
        g.fold_shift = g_op_fold_stats.shift;
        g.fold_mean_out = g_op_fold_stats.mean_out;
        g.fold_eps = 1e-6f;
    }
}
extern "C" int f5_op_fold_rows(const float* stats, int nslice, int M, float* rowf, float* row_shift, void* stream) {
    return g_ops.fold_rows(stats, M, nslice, M, 1e-6f, rowf, row_shift, (hipStream_t)stream);
}
extern "C" int f5_op_fold_consts(const void* w_hi, int ldw, const float* bias, const float* scale, const float* shift, size_t vec_stride,
                                 int nvec, float* c1, float* c2, size_t out_stride, int N, int K, void* stream) {
    return g_ops.fold_consts((const op16_t*)w_hi, ldw, bias, scale, shift, vec_stride, nvec, c1, c2, out_stride, N, K, (hipStream_t)stream);
}

extern "C" int f5_op_gemm(const void* a_hi, const void* a_lo, const void* w_hi, const void* w_lo, const float* bias,
                          float* out_f32, void* out_bf_hi, void* out_bf_lo, int M, int N, int K, int lda, int ldw, int ldo,
                          int nseg, int epi, void* stream) {
    F5_REQUIRE(epi == EPI_F32 || epi == EPI_BF16 || epi == EPI_GELU_TANH || epi == EPI_GELU_ERF || epi == EPI_GELU_ERF_BF16,
               "f5_op_gemm supports epilogues 0-3 and 8 only");
    F5GemmArgs g = f5_gemm_args(a_hi, a_lo, w_hi, w_lo, lda, ldw, M, N, K, nseg, bias);
    g.out_f32 = out_f32;
    g.ldo = ldo;
    g.out_bf[0] = (op16_t*)out_bf_hi;
    g.out_bf[1] = (op16_t*)out_bf_lo;
    g.ldob = ldo;
    if (epi == EPI_GELU_TANH && (g_op_fold.rowf != nullptr || g_op_fold_stats.stats != nullptr)) op_fold_consumer(g);
    return g_ops.gemm(g, epi, (hipStream_t)stream);
}

// MX-fp8 GEMM: A8/W8 e4m3 [rows][ld] + E8M0 scales [rows][K/32].  epi 0: out_f32 = acc + bias; 1: out_bf = bf16(acc + bias);
// 2: (out8, out8s) = MX-fp8(gelu_tanh(acc + bias)); 4: out_f32 += gate * ((acc + bias) * keep[row]).  Always the bf16 build of the
// kernel (the mode has no fp16 form): epi 1 writes bf16 whatever f5_op_set_operand_type says.  ldo serves the output of the epilogue.
extern "C" int f5_op_gemm_f8(const void* a8, const void* a_scales, const void* w8, const void* w_scales, const float* bias,
                             const float* gate, const uint8_t* rowkeep, float* out_f32, void* out_bf, void* out8, void* out8_scales,
                             int M, int N, int K, int lda8, int ldw8, int ldo, int epi, void* stream) {
    F5_REQUIRE(epi == EPI_F32 || epi == EPI_BF16 || epi == EPI_GELU_TANH || epi == EPI_RESID_GATE,
               "f5_op_gemm_f8 supports epilogues 0, 1, 2 and 4");
    F5GemmArgs g = f5_gemm_f8_args(a8, a_scales, w8, w_scales, lda8, ldw8, M, N, K, bias);
    g.gate = gate;
    g.rowkeep = rowkeep;
    g.out_f32 = out_f32;
    g.ldo = ldo;
    g.out_bf[0] = (op16_t*)out_bf;
    g.ldob = ldo;
    g.out8 = (uint8_t*)out8;
    g.out8s = (uint8_t*)out8_scales;
    g.ldo8 = ldo;
    return f5_launch_gemm_f8(g, epi, (hipStream_t)stream);
}
extern "C" int f5_op_quantize_mx(const float* x, int ldx, void* q, int ldq, void* scales, int rows, int cols, void* stream) {
    return f5_launch_quantize_mx(x, ldx, (uint8_t*)q, ldq, (uint8_t*)scales, rows, cols, (hipStream_t)stream);
}
// the weights' quantiser (f5_engine_finalize, precision mxfp8): 16-bit rows of the current operand type -> e4m3 + E8M0
extern "C" int f5_op_quantize_mx_bf16(const void* x16, int ldx, void* q, int ldq, void* scales, int rows, int cols, void* stream) {
    return g_ops.h ? f5hf::f5_launch_quantize_mx_bf16((const f5hf::op16_t*)x16, ldx, (uint8_t*)q, ldq, (uint8_t*)scales, rows, cols,
                                                      (hipStream_t)stream)
                   : f5bf::f5_launch_quantize_mx_bf16((const op16_t*)x16, ldx, (uint8_t*)q, ldq, (uint8_t*)scales, rows, cols,
                                                      (hipStream_t)stream);
}
// LN-modulate straight into an MX-fp8 A operand (the first launch of both halves of an mxfp8 block)
extern "C" int f5_op_ln_modulate_f8(const float* x, const float* scale, const float* shift, void* q, void* q_scales, int rows, int dim,
                                    float eps, void* stream) {
    return f5_launch_ln_modulate_f8(x, scale, shift, (uint8_t*)q, (uint8_t*)q_scales, rows, dim, eps, (hipStream_t)stream);
}
// the QKV projection of an mxfp8 block: the argument builders of run_dit's own launch
extern "C" int f5_op_qkv_rope_f8(const void* a8, const void* a_scales, const void* w8, const void* w_scales, const float* bias,
                                 const float* rope_cos, const float* rope_sin, void* qk, void* vt, int B, int seq_len, int npad, int heads,
                                 int dmodel, int lda8, int ldw8, float q_premul, void* stream) {
    F5GemmArgs g = f5_gemm_f8_args(a8, a_scales, w8, w_scales, lda8, ldw8, B * seq_len, 3 * dmodel, dmodel, bias);
    f5_qkv_rope_fields(g, qk, nullptr, vt, nullptr, rope_cos, rope_sin, seq_len, npad, heads, dmodel, q_premul);
    return f5_launch_gemm_f8(g, EPI_QKV_ROPE, (hipStream_t)stream);
}

// group-major twins of the rotation tables ([dim_head/4][seq_len][4] = (cos, cos, sin, sin) of two neighbouring pairs; the q table
// multiplied by qscale; 16 seq_len dim_head/4 bytes each, 16-byte aligned) and an op-level hook that hands them to f5_op_qkv_rope: with
// both set (and the q factor of f5_debug_set_op_q_premul folded into the q table by the caller) the staged kernels accumulate the
// q / k tiles transposed, as sample() does.  Null = off.
static const float* g_op_rope_t[2] = {nullptr, nullptr};
extern "C" int f5_debug_set_op_rope_tables_g4(const float* tq, const float* tk) {
    g_op_rope_t[0] = tq;
    g_op_rope_t[1] = tk;
    return 0;
}
// op-level twin of the engine's q pre-multiplication (run_dit): when set (single-segment operands only), f5_op_qkv_rope scales
// the q columns by this factor and f5_op_attention treats q as already carrying scale * log2(e).  0 (default) = plain q.
static float g_op_q_premul = 0.0f;
extern "C" int f5_debug_set_op_q_premul(float v) {
    g_op_q_premul = v;
    return 0;
}
// every F5AttnArgs field from the caller (the op-level tests: leading dimensions, q pre-scaling, the v2f / v2p choice, the MX-fp8 output)
extern "C" int f5_op_attention_ex(const void* qk_hi, const void* qk_lo, const void* vt_hi, const void* vt_lo, void* out_hi, void* out_lo,
                                  const int32_t* kv_len, int B, int H, int seq_len, int npad, int dmodel, float scale, int hp, int ldqk,
                                  int ldo, int q_prescaled, int pipe, void* out8, void* out8s, int ldo8, void* stream) {
    F5AttnArgs at = f5_attn_args(qk_hi, qk_lo, vt_hi, vt_lo, out_hi, out_lo, kv_len, B, H, seq_len, npad, dmodel, scale, hp, ldqk, ldo, q_prescaled,
                                 pipe);
    at.out8 = (uint8_t*)out8;
    at.out8s = (uint8_t*)out8s;
    at.ldo8 = ldo8;
    return g_ops.attention(at, (hipStream_t)stream);
}
extern "C" int f5_op_attention(const void* qk_hi, const void* qk_lo, const void* vt_hi, const void* vt_lo, void* out_hi,
                               void* out_lo, const int32_t* kv_len, int B, int H, int seq_len, int npad, int dmodel, float scale,
                               int hp, void* stream) {
    // tight leading dimensions, q pre-scaled when the op-level twin of the engine's q_premul is set, the process default of pipe
    return f5_op_attention_ex(qk_hi, qk_lo, vt_hi, vt_lo, out_hi, out_lo, kv_len, B, H, seq_len, npad, dmodel, scale, hp, 2 * dmodel, dmodel,
                              g_op_q_premul != 0.0f && hp == 0, -1, nullptr, nullptr, 0, stream);
}

extern "C" int f5_op_qkv_rope(const void* a_hi, const void* a_lo, const void* w_hi, const void* w_lo, const float* bias,
                              const float* rope_cos, const float* rope_sin, void* qk_hi, void* qk_lo, void* vt_hi, void* vt_lo,
                              int B, int seq_len, int npad, int heads, int dmodel, int nseg, void* stream) {
    F5GemmArgs g = f5_gemm_args(a_hi, a_lo, w_hi, w_lo, dmodel, dmodel, B * seq_len, 3 * dmodel, dmodel, nseg, bias);
    f5_qkv_rope_fields(g, qk_hi, qk_lo, vt_hi, vt_lo, rope_cos, rope_sin, seq_len, npad, heads, dmodel, nseg == 1 ? g_op_q_premul : 0.0f,
                       g_op_rope_t[0], g_op_rope_t[1]);
    if (g_op_fold.rowf != nullptr || g_op_fold_stats.stats != nullptr) op_fold_consumer(g);
    return g_ops.gemm(g, EPI_QKV_ROPE, (hipStream_t)stream);
}

// f5_op_qkv_rope for an attention inner width that is not the model width: a [B seq_len][K], w [3 inner][K], q | k [.][2 inner]
// (inner = heads * 64; docs/geometries.md).  The hooks f5_op_qkv_rope reads apply but for the LN fold, which is laid out for K == inner.
extern "C" int f5_op_qkv_rope_k(const void* a_hi, const void* a_lo, const void* w_hi, const void* w_lo, const float* bias,
                                const float* rope_cos, const float* rope_sin, void* qk_hi, void* qk_lo, void* vt_hi, void* vt_lo,
                                int B, int seq_len, int npad, int heads, int inner, int K, int nseg, void* stream) {
    F5GemmArgs g = f5_gemm_args(a_hi, a_lo, w_hi, w_lo, K, K, B * seq_len, 3 * inner, K, nseg, bias);
    f5_qkv_rope_fields(g, qk_hi, qk_lo, vt_hi, vt_lo, rope_cos, rope_sin, seq_len, npad, heads, inner, nseg == 1 ? g_op_q_premul : 0.0f,
                       g_op_rope_t[0], g_op_rope_t[1]);
    return g_ops.gemm(g, EPI_QKV_ROPE, (hipStream_t)stream);
}

extern "C" int f5_op_rope_table_g4(float* tq, float* tk, int seq_len, int dim_head, float qscale, void* stream) {
    return f5_launch_rope_table_g4(tq, tk, seq_len, dim_head, qscale, (hipStream_t)stream);
}
extern "C" int f5_op_rope_table(float* cos_t, float* sin_t, int seq_len, int dim_head, void* stream) {
    return f5_launch_rope_table(cos_t, sin_t, seq_len, dim_head, (hipStream_t)stream);
}

extern "C" int f5_op_convpos(const void* in_hi, const void* in_lo, const void* w_hi, const void* w_lo, const float* bias,
                             void* out_hi, void* out_lo, float* out_f32, int B, int seq_len, int C, int groups, int taps,
                             int nseg, int mode, void* stream) {
    return f5_op_convpos_ragged(in_hi, in_lo, w_hi, w_lo, bias, out_hi, out_lo, out_f32, B, seq_len, C, groups, taps, nseg, mode, nullptr, stream);
}

// MFMA rate yardstick of the current operand type (f5_op_set_operand_type): see rowops.hip mfma_peak_kernel
extern "C" int f5_op_mfma_peak(const void* operands, int blocks, int iters, float* sink, double* flops, void* stream) {
    return g_ops.h ? f5hf::f5_launch_mfma_peak((const f5hf::op16_t*)operands, blocks, iters, sink, flops, (hipStream_t)stream)
                   : f5bf::f5_launch_mfma_peak((const f5bf::op16_t*)operands, blocks, iters, sink, flops, (hipStream_t)stream);
}

extern "C" int f5_op_ln_modulate(const float* x, const float* scale, const float* shift, void* out_hi, void* out_lo, int rows,
                                 int dim, void* stream) {
    return g_ops.ln_modulate(x, scale, shift, (op16_t*)out_hi, (op16_t*)out_lo, rows, dim, 1e-6f, (hipStream_t)stream, g_op_fold.ln_mean_out);
}

extern "C" int f5_op_dwconv_ln(const float* x, const float* dw_w, const float* dw_b, const float* ln_w, const float* ln_b,
                               void* out_hi, void* out_lo, int nbatch, int seq_len, int dim, void* stream) {
    return g_ops.dwconv_ln(x, dw_w, dw_b, ln_w, ln_b, (op16_t*)out_hi, (op16_t*)out_lo, nbatch, seq_len, dim, 1e-6f,
                               (hipStream_t)stream);
}
extern "C" int f5_op_dwconv_ln_ragged(const float* x, const float* dw_w, const float* dw_b, const float* ln_w, const float* ln_b,
                                      void* out_hi, void* out_lo, int nbatch, int seq_len, int dim, const int32_t* lens_dev,
                                      void* stream) {
    return g_ops.dwconv_ln_ragged(x, dw_w, dw_b, ln_w, ln_b, (op16_t*)out_hi, (op16_t*)out_lo, nbatch, seq_len, dim, 1e-6f, lens_dev,
                                  (hipStream_t)stream);
}

// f5_op_convpos with row lengths (F5ConvPosArgs::lens, dev [B]; NULL = f5_op_convpos)
extern "C" int f5_op_convpos_ragged(const void* in_hi, const void* in_lo, const void* w_hi, const void* w_lo, const float* bias,
                                    void* out_hi, void* out_lo, float* out_f32, int B, int seq_len, int C, int groups, int taps,
                                    int nseg, int mode, const int32_t* lens_dev, void* stream) {
    F5ConvPosArgs cp;
    memset(&cp, 0, sizeof(cp));
    cp.in[0] = (const op16_t*)in_hi;
    cp.in[1] = (const op16_t*)in_lo;
    cp.W[0] = (const op16_t*)w_hi;
    cp.W[1] = (const op16_t*)w_lo;
    cp.bias = bias;
    cp.B = B;
    cp.seq_len = seq_len;
    cp.C = C;
    cp.groups = groups;
    cp.taps = taps;
    cp.ld = C;
    cp.ldo = C;
    cp.nseg = nseg;
    cp.mode = mode;
    cp.out_bf[0] = (op16_t*)out_hi;
    cp.out_bf[1] = (op16_t*)out_lo;
    cp.out_f32 = out_f32;
    cp.lens = lens_dev;
    return g_ops.convpos(cp, (hipStream_t)stream);
}

// The weight store's packing of a conv-pos weight (C, taps, cpg), cpg = 32, 48 or 64, on the host (host_common.hpp f5_pack_conv_groups):
// out = [f5_op_conv_packed_rows(C, cpg)][taps * 64] floats, the matrix f5_op_convpos reads once rounded to the operand type.  No device.
extern "C" int f5_op_conv_packed_rows(int C, int cpg) {
    return (C > 0 && (cpg == 64 || cpg == 48 || cpg == 32) && C % cpg == 0) ? f5_conv_packed_rows(C, cpg) : -1;
}
extern "C" int f5_op_pack_conv_groups(const float* w, int C, int taps, int cpg, float* out) {
    F5_REQUIRE(w && out && taps >= 1, "pack_conv_groups: null argument / no taps");
    F5_REQUIRE(f5_op_conv_packed_rows(C, cpg) > 0, "pack_conv_groups: channels per group must be 32, 48 or 64 and divide C (C=%d cpg=%d)", C, cpg);
    std::vector<float> m;
    f5_pack_conv_groups(w, C, taps, cpg, m);
    memcpy(out, m.data(), m.size() * sizeof(float));
    return 0;
}

extern "C" size_t f5_op_grn_scratch_floats(int nbatch, int seq_len, int dim) {
    return f5_grn_partial_floats(nbatch, seq_len, dim) + (size_t)nbatch * dim;
}
extern "C" int f5_op_grn(const float* g, const float* gamma, const float* beta, float* scratch, void* out_hi, void* out_lo,
                         int nbatch, int seq_len, int dim, void* stream) {
    float* nx = scratch + f5_grn_partial_floats(nbatch, seq_len, dim);
    return g_ops.grn(g, gamma, beta, scratch, nx, (op16_t*)out_hi, (op16_t*)out_lo, nbatch, seq_len, dim, (hipStream_t)stream);
}
extern "C" int f5_op_grn_ragged(const float* g, const float* gamma, const float* beta, float* scratch, void* out_hi, void* out_lo,
                                int nbatch, int seq_len, int dim, const int32_t* lens_dev, void* stream) {
    F5_REQUIRE(scratch, "f5_op_grn_ragged: scratch is null");
    F5_REQUIRE(nbatch >= 1 && seq_len >= 1 && dim >= 1, "f5_op_grn_ragged: bad sizes nbatch=%d seq_len=%d dim=%d", nbatch, seq_len, dim);
    float* nx = scratch + f5_grn_partial_floats(nbatch, seq_len, dim);
    return g_ops.grn_ragged(g, gamma, beta, scratch, nx, (op16_t*)out_hi, (op16_t*)out_lo, nbatch, seq_len, dim, lens_dev,
                            (hipStream_t)stream);
}

extern "C" int f5_op_text_embed(const int32_t* text, int nt, const float* table, const float* pos_table, int max_pos, float* out,
                                int32_t* ids_out, uint8_t* keep_out, int B, int seq_len, int dim, void* stream) {
    return f5_launch_text_embed(text, nt, table, pos_table, max_pos, out, ids_out, keep_out, B, seq_len, dim, 1, (hipStream_t)stream);
}
extern "C" int f5_op_text_embed_nomask(const int32_t* text, int nt, const float* table, const float* pos_table, int max_pos,
                                       float* out, int32_t* ids_out, uint8_t* keep_out, int B, int seq_len, int dim, void* stream) {
    return f5_launch_text_embed(text, nt, table, pos_table, max_pos, out, ids_out, keep_out, B, seq_len, dim, 0, (hipStream_t)stream);
}
// out = (resid + A W^T + bias) * keep[row]   (convnext_v2.py:53-54 + dit.py:225; keep may be NULL)
extern "C" int f5_op_gemm_resid_keep(const void* a_hi, const void* a_lo, const void* w_hi, const void* w_lo, const float* bias,
                                     const float* resid, const uint8_t* rowkeep, float* out, int M, int N, int K, int lda, int ldw,
                                     int ldo, int nseg, void* stream) {
    F5GemmArgs g = f5_gemm_args(a_hi, a_lo, w_hi, w_lo, lda, ldw, M, N, K, nseg, bias);
    g.resid = resid;
    g.ldres = ldo;
    g.rowkeep = rowkeep;
    g.out_f32 = out;
    g.ldo = ldo;
    F5_REQUIRE(resid != nullptr && out != nullptr, "gemm_resid_keep: null resid / out");
    return g_ops.gemm(g, EPI_RESID_KEEP, (hipStream_t)stream);
}
extern "C" int f5_op_pack_bf16(const float* src, const uint8_t* rowkeep, void* out_hi, void* out_lo, int rows, int cols, int ld,
                               int col0, void* stream) {
    return g_ops.pack_bf16(src, rowkeep, (op16_t*)out_hi, (op16_t*)out_lo, rows, cols, ld, col0, (hipStream_t)stream);
}
extern "C" int f5_op_duration_head(const float* x, const float* g, const float* w, const uint8_t* mask, float* out, int B,
                                   int seq_len, int dim, float eps, void* stream) {
    return f5_launch_duration_head(x, g, w, mask, out, B, seq_len, dim, eps, (hipStream_t)stream);
}
extern "C" int f5_op_text_pos_table(float* table, int max_pos, int dim, void* stream) {
    return f5_launch_text_pos_table(table, max_pos, dim, (hipStream_t)stream);
}
extern "C" int f5_op_time_sinus(const float* t, float* out, int n, int dim, void* stream) {
    return f5_launch_time_sinus(t, out, n, dim, (hipStream_t)stream);
}
extern "C" int f5_op_skinny_gemm(const float* a, const float* w, const float* b, float* out, int M, int N, int K, int silu_in,
                                 int silu_out, void* stream) {
    return f5_launch_skinny_gemm(a, w, b, out, M, N, K, silu_in, silu_out, (hipStream_t)stream);
}
extern "C" int f5_op_cfg_axpy(const float* pred, const float* null_pred, float cfg, const float* base, const float* dt_dev,
                              float coef, float divisor, float* out, void* xin_hi, void* xin_lo, int rows, int mel_dim,
                              void* stream) {
    F5OdeArgs o;
    memset(&o, 0, sizeof(o));
    o.pred = pred;
    o.null_pred = null_pred;
    o.cfg = cfg;
    o.base = base;
    o.dt_ptr = dt_dev;
    o.coef = coef;
    o.divisor = divisor;
    o.out = out;
    o.xin_hi = (op16_t*)xin_hi;
    o.xin_lo = (op16_t*)xin_lo;
    o.rows = rows;
    o.mel_dim = mel_dim;
    return g_ops.ode_stage(o, (hipStream_t)stream);
}
// the whole stage kernel (rowops.hpp F5OdeArgs, field by field; saturation goes to the word of f5_debug_set_op_sat_flag)
extern "C" int f5_op_ode_stage(const float* pred, const float* null_pred, float cfg, const float* cfg_ptr, const float* base,
                               const float* dt_dev, float coef, float divisor, int mode, float* kstore, const float* k1,
                               const float* k2, const float* k3, float* out, void* xin_hi, void* xin_lo, int rows, int mel_dim,
                               void* stream) {
    F5OdeArgs o;
    memset(&o, 0, sizeof(o));
    o.pred = pred;
    o.null_pred = null_pred;
    o.cfg = cfg;
    o.cfg_ptr = cfg_ptr;
    o.base = base;
    o.dt_ptr = dt_dev;
    o.coef = coef;
    o.divisor = divisor;
    o.mode = mode;
    o.kstore = kstore;
    o.k1 = k1;
    o.k2 = k2;
    o.k3 = k3;
    o.out = out;
    o.xin_hi = (op16_t*)xin_hi;
    o.xin_lo = (op16_t*)xin_lo;
    o.rows = rows;
    o.mel_dim = mel_dim;
    F5_REQUIRE(pred != nullptr && base != nullptr && dt_dev != nullptr && out != nullptr, "ode_stage: null pred / base / dt / out");
    F5_REQUIRE(mode == 0 || (mode == 1 && k1 != nullptr && k2 != nullptr && k3 != nullptr), "ode_stage: mode 1 needs k1, k2 and k3");
    return g_ops.ode_stage(o, (hipStream_t)stream);
}
// the stage kernel with guidance strength and step size per row (rowops.hpp f5_launch_ode_stage_rows)
extern "C" int f5_op_ode_stage_rows(const float* pred, const float* null_pred, const float* cfg_rows, const float* base, const float* dt_rows,
                                    int rows_per_vec, int nvec, float coef, float divisor, int mode, float* kstore, const float* k1,
                                    const float* k2, const float* k3, float* out, void* xin_hi, void* xin_lo, int rows, int mel_dim,
                                    void* stream) {
    F5OdeArgs o;
    memset(&o, 0, sizeof(o));
    o.pred = pred;
    o.null_pred = null_pred;
    o.base = base;
    o.coef = coef;
    o.divisor = divisor;
    o.mode = mode;
    o.kstore = kstore;
    o.k1 = k1;
    o.k2 = k2;
    o.k3 = k3;
    o.out = out;
    o.xin_hi = (op16_t*)xin_hi;
    o.xin_lo = (op16_t*)xin_lo;
    o.rows = rows;
    o.mel_dim = mel_dim;
    F5_REQUIRE(pred != nullptr && base != nullptr && out != nullptr, "ode_stage_rows: null pred / base / out");
    F5_REQUIRE(mode == 0 || (mode == 1 && k1 != nullptr && k2 != nullptr && k3 != nullptr), "ode_stage_rows: mode 1 needs k1, k2 and k3");
    return g_ops.ode_stage_rows(o, cfg_rows, dt_rows, rows_per_vec, nvec, (hipStream_t)stream);
}
// the stage kernel of dual guidance (rowops.hpp f5_launch_ode_stage_dual, which refuses what it refuses)
extern "C" int f5_op_ode_stage_dual(const float* pred, const float* text_pred, const float* null_pred, const float* audio_cfg_rows,
                                    const float* text_cfg_rows, const float* base, const float* dt_rows, int rows_per_vec, int nvec, float coef,
                                    float divisor, int mode, float* kstore, const float* k1, const float* k2, const float* k3, float* out,
                                    void* xin_hi, void* xin_lo, int rows, int mel_dim, void* stream) {
    F5OdeArgs o;
    memset(&o, 0, sizeof(o));
    o.pred = pred;
    o.null_pred = null_pred;
    o.base = base;
    o.coef = coef;
    o.divisor = divisor;
    o.mode = mode;
    o.kstore = kstore;
    o.k1 = k1;
    o.k2 = k2;
    o.k3 = k3;
    o.out = out;
    o.xin_hi = (op16_t*)xin_hi;
    o.xin_lo = (op16_t*)xin_lo;
    o.rows = rows;
    o.mel_dim = mel_dim;
    return g_ops.ode_stage_dual(o, text_pred, audio_cfg_rows, text_cfg_rows, dt_rows, rows_per_vec, nvec, (hipStream_t)stream);
}
// Mode 2 of the three stage kernels, the Adams-Bashforth step (rowops.hpp F5OdeArgs): route 0 = the scalar kernel (cfg_ptr, dt and
// abw [3] for the call; text_pred, audio_cfg_rows, rows_per_vec and nvec not read), 1 = per row (cfg_rows, dt_rows, abw [nvec][3]),
// 2 = dual guidance (text_pred and audio_cfg_rows as well).  k1 / k2: the velocities of the step before and the one before that, or null.
extern "C" int f5_op_ode_stage_ab(int route, const float* pred, const float* text_pred, const float* null_pred, const float* audio_cfg_rows,
                                  const float* cfg, const float* base, const float* dt, const float* abw, int rows_per_vec, int nvec,
                                  float* kstore, const float* k1, const float* k2, float* out, void* xin_hi, void* xin_lo, int rows,
                                  int mel_dim, void* stream) {
    F5_REQUIRE(route >= 0 && route <= 2, "ode_stage_ab: route must be 0, 1 or 2 (got %d)", route);
    F5_REQUIRE(pred != nullptr && base != nullptr && dt != nullptr && out != nullptr, "ode_stage_ab: null pred / base / dt / out");
    F5_REQUIRE(rows >= 1 && mel_dim >= 1, "ode_stage_ab: no rows / columns (got %d, %d)", rows, mel_dim);
    F5_REQUIRE(route == 0 || cfg != nullptr, "ode_stage_ab: null cfg_rows");
    F5OdeArgs o;
    memset(&o, 0, sizeof(o));
    o.pred = pred;
    o.null_pred = null_pred;
    o.cfg_ptr = cfg;
    o.base = base;
    o.dt_ptr = dt;
    o.coef = 1.0f;
    o.divisor = 1.0f;
    o.mode = 2;
    o.kstore = kstore;
    o.k1 = k1;
    o.k2 = k2;
    o.abw = abw;
    o.out = out;
    o.xin_hi = (op16_t*)xin_hi;
    o.xin_lo = (op16_t*)xin_lo;
    o.rows = rows;
    o.mel_dim = mel_dim;
    if (route == 2) return g_ops.ode_stage_dual(o, text_pred, audio_cfg_rows, cfg, dt, rows_per_vec, nvec, (hipStream_t)stream);
    return route == 1 ? g_ops.ode_stage_rows(o, cfg, dt, rows_per_vec, nvec, (hipStream_t)stream) : g_ops.ode_stage(o, (hipStream_t)stream);
}
extern "C" int f5_op_pack_cond_text_dual(const float* cond, const int32_t* lens, const float* text_emb, void* out_hi, void* out_lo, int B,
                                         int seq_len, int mel_dim, int dt, void* stream) {
    F5_REQUIRE(lens != nullptr, "pack_cond_text_dual: lens is null");
    return g_ops.pack_cond_text_dual(cond, lens, nullptr, text_emb, (op16_t*)out_hi, (op16_t*)out_lo, B, seq_len, mel_dim, dt,
                                     (hipStream_t)stream);
}
extern "C" int f5_op_pack_cond_text_dual_keep(const float* cond, const uint8_t* keep, const float* text_emb, void* out_hi, void* out_lo, int B,
                                              int seq_len, int mel_dim, int dt, void* stream) {
    F5_REQUIRE(keep != nullptr, "pack_cond_text_dual_keep: keep is null");
    return g_ops.pack_cond_text_dual(cond, nullptr, keep, text_emb, (op16_t*)out_hi, (op16_t*)out_lo, B, seq_len, mel_dim, dt,
                                     (hipStream_t)stream);
}
// residual update + LN-modulate with per-row vectors (rowops.hpp f5_launch_resid_gate_ln_rows), eps 1e-6
extern "C" int f5_op_resid_gate_ln_rows(const float* y, float* x, const float* gate, const uint8_t* rowkeep, const float* ln_scale,
                                        const float* ln_shift, void* out_hi, void* out_lo, int rows, int dim, int rows_per_vec, int nvec,
                                        size_t vec_stride, void* stream) {
    return g_ops.resid_gate_ln_rows(y, x, gate, rowkeep, ln_scale, ln_shift, (op16_t*)out_hi, (op16_t*)out_lo, rows, dim, rows_per_vec, nvec,
                                    vec_stride, 1e-6f, (hipStream_t)stream);
}
extern "C" int f5_op_pack_cond_text(const float* cond, const int32_t* lens, const float* text_emb, void* out_hi, void* out_lo, int B,
                                    int seq_len, int mel_dim, int dt, int null_keeps_cond, void* stream) {
    return g_ops.pack_cond_text(cond, lens, text_emb, (op16_t*)out_hi, (op16_t*)out_lo, B, seq_len, mel_dim, dt, null_keeps_cond,
                                (hipStream_t)stream);
}
extern "C" int f5_op_pack_x(const float* y, void* out_hi, void* out_lo, int rows, int mel_dim, void* stream) {
    F5_REQUIRE(mel_dim <= 128, "pack_x: mel_dim must be <= 128");
    return g_ops.pack_x(y, (op16_t*)out_hi, (op16_t*)out_lo, rows, mel_dim, (hipStream_t)stream);
}
extern "C" int f5_op_pack_cond_text_keep(const float* cond, const uint8_t* keep, const float* text_emb, void* out_hi, void* out_lo, int B,
                                         int seq_len, int mel_dim, int dt, int null_keeps_cond, void* stream) {
    F5_REQUIRE(cond && keep && text_emb && out_hi, "pack_cond_text_keep: null pointer");
    F5_REQUIRE(B >= 1 && seq_len >= 1 && mel_dim >= 1 && dt >= 0, "pack_cond_text_keep: bad sizes B=%d seq_len=%d mel_dim=%d dt=%d", B, seq_len,
               mel_dim, dt);
    return g_ops.pack_cond_text_keep(cond, keep, text_emb, (op16_t*)out_hi, (op16_t*)out_lo, B, seq_len, mel_dim, dt, null_keeps_cond,
                                     (hipStream_t)stream);
}
extern "C" int f5_op_splice_keep(const float* cond, const float* y, const uint8_t* keep, float* out, int B, int seq_len, int mel_dim,
                                 void* stream) {
    F5_REQUIRE(cond && y && keep && out, "splice_keep: null pointer");
    F5_REQUIRE(B >= 1 && seq_len >= 1 && mel_dim >= 1, "splice_keep: bad sizes B=%d seq_len=%d mel_dim=%d", B, seq_len, mel_dim);
    return f5_launch_splice_keep(cond, y, keep, out, B, seq_len, mel_dim, (hipStream_t)stream);
}
extern "C" int f5_op_gather_frames(const float* src, const int32_t* src_idx, float* cond_out, uint8_t* keep_out, int B, int n_src,
                                   int seq_len, int mel_dim, void* stream) {
    F5_REQUIRE(src && src_idx && cond_out && keep_out, "gather_frames: null pointer");
    F5_REQUIRE(B >= 1 && n_src >= 1 && seq_len >= 1 && mel_dim >= 1, "gather_frames: bad sizes B=%d n_src=%d seq_len=%d mel_dim=%d", B, n_src,
               seq_len, mel_dim);
    return f5_launch_gather_frames(src, src_idx, cond_out, keep_out, B, n_src, seq_len, mel_dim, (hipStream_t)stream);
}
extern "C" int f5_op_splice(const float* cond, const float* y, const int32_t* lens, float* out, int B, int seq_len, int mel_dim,
                            void* stream) {
    return f5_launch_splice(cond, y, lens, out, B, seq_len, mel_dim, (hipStream_t)stream);
}
extern "C" int f5_op_rowkeep(const int32_t* dur, uint8_t* keep, int nbatch, int seq_len, void* stream) {
    return f5_launch_rowkeep(dur, keep, nbatch, seq_len, (hipStream_t)stream);
}
extern "C" int f5_op_copy_words(const void* src, void* dst, size_t nwords, void* stream) {
    F5_REQUIRE((((uintptr_t)src | (uintptr_t)dst) & 3) == 0, "copy_words: pointers must be 4-byte aligned");
    return f5_launch_copy_words(src, dst, nwords, (hipStream_t)stream);
}
extern "C" int f5_op_stage_words(const uint32_t* host_words, size_t nwords, uint32_t* dst, void* stream) {
    return f5_launch_stage_words(host_words, nwords, dst, (hipStream_t)stream);
}
extern "C" int f5_op_zero_vt_pad(void* vt, size_t rows, int seq_len, int npad, void* stream) {
    return g_ops.zero_vt_pad((op16_t*)vt, rows, seq_len, npad, (hipStream_t)stream);
}

// x[row][col] += gate[col] * ((A W^T + bias)[row][col] * keep[row])   (dit.py:319,323; Vocos layer scale + residual)
extern "C" int f5_op_gemm_resid_gate(const void* a_hi, const void* a_lo, const void* w_hi, const void* w_lo, const float* bias,
                                     const float* gate, const uint8_t* rowkeep, float* x, int M, int N, int K, int lda, int ldw,
                                     int ldx, int nseg, void* stream) {
    F5GemmArgs g = f5_gemm_args(a_hi, a_lo, w_hi, w_lo, lda, ldw, M, N, K, nseg, bias);
    g.gate = gate;
    g.rowkeep = rowkeep;
    g.out_f32 = x;
    g.ldo = ldx;
    F5_REQUIRE(gate != nullptr && x != nullptr, "gemm_resid_gate: null gate / x");
    if (g_op_fold.x16 != nullptr) {
        g.x16_out = g_op_fold.x16;
        g.ldx16 = N;
        g.x16_scale = g_op_fold.next_scale;
        g.x16_shift = g_op_fold.row_shift;
        g.stats_out = g_op_fold.stats_out;
        g.stats_ld = M;
        g.x16_overflow = g_op_fold_overflow;
    }
    return g_ops.gemm(g, EPI_RESID_GATE, (hipStream_t)stream);
}
// the same with the LN-modulate of the next sub-layer fused behind it (small-tile shapes only, see gemm.hpp ln_counter):
// h = LN(x_new) * (1 + ln_scale) + ln_shift, bit-identical to f5_op_gemm_resid_gate followed by f5_op_ln_modulate.
// counters: >= ceil(M / 64) ints, zero on entry (left zero on exit).  Returns an error for shapes that run the large-tile kernels.
extern "C" int f5_op_gemm_resid_gate_ln(const void* a_hi, const void* a_lo, const void* w_hi, const void* w_lo, const float* bias,
                                        const float* gate, const uint8_t* rowkeep, float* x, const float* ln_scale,
                                        const float* ln_shift, void* h_hi, void* h_lo, int* counters, int M, int N, int K, int lda,
                                        int ldw, int nseg, void* stream) {
    F5GemmArgs g = f5_gemm_args(a_hi, a_lo, w_hi, w_lo, lda, ldw, M, N, K, nseg, bias);
    g.gate = gate;
    g.rowkeep = rowkeep;
    g.out_f32 = x;
    g.ldo = N;
    g.ln_counter = counters;
    g.ln_scale = ln_scale;
    g.ln_shift = ln_shift;
    g.ln_out[0] = (op16_t*)h_hi;
    g.ln_out[1] = (op16_t*)h_lo;
    g.ln_eps = 1e-6f;
    F5_REQUIRE(gate && x && ln_scale && ln_shift && h_hi && counters, "gemm_resid_gate_ln: null pointer");
    return g_ops.gemm(g, EPI_RESID_GATE, (hipStream_t)stream);
}
// out_f32 = A[row % a_row_mod] W^T + addrows[row], out_bf = the same rounded to the operand type (dit.py:250: the per-step
// x projection added to the hoisted cond / text part; both CFG branches share the x rows through a_row_mod)
extern "C" int f5_op_gemm_addrows(const void* a_hi, const void* a_lo, const void* w_hi, const void* w_lo, const float* addrows,
                                  int a_row_mod, float* out_f32, void* out_hi, void* out_lo, int M, int N, int K, int lda, int ldw,
                                  int ldo, int nseg, void* stream) {
    F5GemmArgs g = f5_gemm_args(a_hi, a_lo, w_hi, w_lo, lda, ldw, M, N, K, nseg, nullptr);
    g.a_row_mod = a_row_mod;
    g.addrows = addrows;
    g.ldadd = ldo;
    g.out_f32 = out_f32;
    g.ldo = ldo;
    g.out_bf[0] = (op16_t*)out_hi;
    g.out_bf[1] = (op16_t*)out_lo;
    g.ldob = ldo;
    F5_REQUIRE(addrows != nullptr && out_f32 != nullptr && out_hi != nullptr, "gemm_addrows: null addrows / out");
    return g_ops.gemm(g, EPI_ADDROWS, (hipStream_t)stream);
}
extern "C" int f5_op_layernorm(const float* x, const float* w, const float* b, float* out_f32, void* out_hi, void* out_lo,
                               int rows, int dim, void* stream) {
    return g_ops.layernorm(x, w, b, out_f32, (op16_t*)out_hi, (op16_t*)out_lo, rows, dim, 1e-6f, (hipStream_t)stream);
}
extern "C" int f5_op_im2col7(const float* x, void* out_hi, void* out_lo, int nbatch, int seq_len, int channels, void* stream) {
    return g_ops.im2col7(x, (op16_t*)out_hi, (op16_t*)out_lo, nbatch, seq_len, channels, (hipStream_t)stream);
}
extern "C" int f5_op_im2col7_ragged(const float* x, void* out_hi, void* out_lo, int nbatch, int seq_len, int channels,
                                    const int32_t* lens_dev, void* stream) {
    return g_ops.im2col7_ragged(x, (op16_t*)out_hi, (op16_t*)out_lo, nbatch, seq_len, channels, lens_dev, (hipStream_t)stream);
}
