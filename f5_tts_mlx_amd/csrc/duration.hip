// Duration predictor behind the C ABI: (mel, text, lens) -> seconds (and frames), one call (`f5_predict_duration`), hipGraph captured.
//
// Reference: DurationPredictor / DurationTransformer (duration.py:97-260), reached from F5TTS.predict_duration (cfm.py:253-262, :307-308):
//   TextEmbedding WITHOUT padding mask (duration.py:116-118)  -> text_embed kernel + ConvNeXtV2 blocks (dwconv_ln, GEMM + GELU, GRN, GEMM)
//   Linear(mel + text -> dim) + ConvPositionEmbedding (duration.py:44-58) -> packed [mel padded to 128 | text] operand, GEMM, two conv-pos launches
//   depth x pre-LN block, plain LayerNorm, no gates, no masks (duration.py:64-94) -> ln_modulate on a zero vector, QKV + RoPE, attention,
//                                                                  residual epilogue on a ones vector, FF1 + GELU, FF2
//   RMSNorm -> masked mean -> Linear(dim -> 1) -> Softplus (duration.py:137,188-190,249-251) -> duration_head kernel
// The launch sequence is the one f5_tts_mlx_amd/duration.py `_run_ops` issues through the f5_op_* entry points -- the same kernels in the
// same order with the same arguments -- on this handle's own Ops: nothing here reads or writes the process-wide operand type.
#include <stdarg.h>

#include <string>
#include <vector>

#include "../../include/f5tts_hip.h"
#include "host_common.hpp"

struct DTextBlock {
    size_t dw_w, dw_b, ln_w, ln_b, b1, gamma, beta, b2;
    MatBF pw1, pw2;
};
struct DBlock {
    MatBF qkv, o, ff1, ff2;
    size_t bqkv, bo, bff1, bff2;
};
struct DWorkspace {
    size_t total = 0;
    size_t status;           // THE FIRST WORD OF THE WORKSPACE: F5_STATUS_* of the last call, zeroed by every call
    size_t lens, text, mel;  // staged caller inputs (outside the captured part)
    size_t mask, te, ids, keep, t_nxt, tg, scratch, x, cos_t, sin_t, pred;
    size_t tln[2], tg2[2], a0[2], xb[2], c1[2], h[2], qk[2], vt[2], ao[2], ffh[2];
    size_t rowlen = 0;       // row lengths L[b] = max(lens[b], text_lens[b]) of f5_predict_duration_rows, staged like lens; behind the plain plan
};

struct f5_duration : WeightStore {
    f5_duration_config cfg;
    Ops ops;
    size_t table, pos, bproj, norm_out, to_pred, zeros, ones;
    std::vector<DTextBlock> tblocks;
    MatBF proj, conv_w[2];
    size_t conv_b[2];
    std::vector<DBlock> blocks;
    GraphCache graphs;       // at most 8; keyed by (B, n_in, nt, row-isolated).  The caller keeps one workspace per shape: nothing is purged
};

extern "C" int f5_duration_create(const f5_duration_config* cfg, int precision, f5_duration** out) {
    F5_REQUIRE(cfg && out, "f5_duration_create: null argument");
    const f5_duration_config& c = *cfg;
    F5_REQUIRE(precision == F5_PREC_BF16 || precision == F5_PREC_BF16X3 || precision == F5_PREC_F16,
               "duration predictor precision must be bf16, bf16x3 or f16 (got %d)", precision);
    F5_REQUIRE(c.dim_head == 64, "duration predictor: dim_head must be 64 (got %d)", c.dim_head);
    F5_REQUIRE(c.heads >= 1 && c.heads * c.dim_head == c.dim, "duration predictor: heads * dim_head must equal dim (%d * %d != %d)", c.heads,
               c.dim_head, c.dim);
    F5_REQUIRE(c.dim % 256 == 0 && c.dim <= 1024, "duration predictor: dim must be a multiple of 256 and <= 1024 (got %d)", c.dim);
    F5_REQUIRE(c.conv_pos_groups >= 1 && c.dim % c.conv_pos_groups == 0 && (c.dim / c.conv_pos_groups == 32 || c.dim / c.conv_pos_groups == 64),
               "duration predictor: dim / conv_pos_groups must be 32 or 64 (got %d / %d)", c.dim, c.conv_pos_groups);
    F5_REQUIRE(c.conv_pos_kernel >= 1 && c.conv_pos_kernel % 2 == 1 && c.conv_pos_kernel <= 31,
               "duration predictor: conv_pos_kernel must be odd and <= 31 (got %d)", c.conv_pos_kernel);
    F5_REQUIRE(c.text_dim >= 256 && c.text_dim % 256 == 0 && c.text_dim <= 1024,
               "duration predictor: text_dim must be a multiple of 256 and <= 1024 (got %d)", c.text_dim);
    F5_REQUIRE(c.ff_dim >= 128 && c.ff_dim % 128 == 0, "duration predictor: ff_dim must be a multiple of 128 (got %d)", c.ff_dim);
    F5_REQUIRE(c.mel_dim >= 1 && c.mel_dim <= 128, "duration predictor: mel_dim must be in [1, 128] (got %d)", c.mel_dim);
    F5_REQUIRE(c.text_num_embeds >= 1, "duration predictor: text_num_embeds must be >= 1 (got %d)", c.text_num_embeds);
    F5_REQUIRE(c.depth >= 1 && c.depth <= 64, "duration predictor: depth out of range (got %d)", c.depth);
    F5_REQUIRE(c.conv_layers >= 1 && c.conv_layers <= 64, "duration predictor: conv_layers must be >= 1 (got %d)", c.conv_layers);
    F5_REQUIRE(c.text_max_pos >= 4, "duration predictor: text_max_pos must be >= 4 (got %d)", c.text_max_pos);
    f5_duration* d = new f5_duration();
    d->cfg = c;
    d->label = "duration predictor ";
    d->np = precision == F5_PREC_BF16X3 ? 2 : 1;
    d->f16 = d->ops.h = precision == F5_PREC_F16;
    d->graphs.purge = false;
    const int D = c.dim, Dt = c.text_dim, TF = 2 * c.text_dim, FF = c.ff_dim, M = c.mel_dim, np = d->np;
    const std::string p = "transformer.";
    Bump b;
    d->table = b.take((size_t)(c.text_num_embeds + 1) * Dt * 4);
    d->pos = b.take((size_t)c.text_max_pos * Dt * 4);
    d->add_f32(p + "text_embed.text_embed.weight", d->table, {c.text_num_embeds + 1, Dt});
    d->tblocks.resize(c.conv_layers);
    for (int i = 0; i < c.conv_layers; ++i) {
        DTextBlock& t = d->tblocks[i];
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
        d->add_f32(q + "dwconv.weight", t.dw_w, {Dt, 7, 1});       // (dim, 7, 1) = the bytes of [dim][7]
        d->add_f32(q + "dwconv.bias", t.dw_b, {Dt});
        d->add_f32(q + "norm.weight", t.ln_w, {Dt});
        d->add_f32(q + "norm.bias", t.ln_b, {Dt});
        d->add_mat(q + "pwconv1.weight", t.pw1, 0, TF, Dt, 0, Dt, 0, {TF, Dt});
        d->add_f32(q + "pwconv1.bias", t.b1, {TF});
        d->add_f32(q + "grn.gamma", t.gamma, {1, 1, TF});
        d->add_f32(q + "grn.beta", t.beta, {1, 1, TF});
        d->add_mat(q + "pwconv2.weight", t.pw2, 0, Dt, TF, 0, TF, 0, {Dt, TF});
        d->add_f32(q + "pwconv2.bias", t.b2, {Dt});
    }
    // input projection: reference input order (x | text) (duration.py:44-58) -> operand columns [x padded to 128 | text]
    d->proj = alloc_mat(b, D, 128 + Dt, np);
    d->bproj = b.take((size_t)D * 4);
    d->add_mat(p + "input_embed.proj.weight", d->proj, 0, D, M + Dt, 0, M, 0, {D, M + Dt});
    d->add_mat(p + "input_embed.proj.weight", d->proj, 0, D, M + Dt, M, M + Dt, 128, {D, M + Dt});
    d->add_f32(p + "input_embed.proj.bias", d->bproj, {D});
    // conv position embedding: the kernel works on 64-channel groups; 32-channel groups are loaded as block-diagonal 64-wide super
    // groups (host_common.hpp f5_pack_conv_groups, on the way into the weight store)
    const int kc = c.conv_pos_kernel, gin = D / c.conv_pos_groups;
    for (int j = 0; j < 2; ++j) {
        const std::string q = p + "input_embed.conv_pos_embed.conv1d.layers." + std::to_string(j * 2) + ".";
        d->conv_w[j] = d->add_conv_groups(b, q + "weight", D, kc, gin);
        d->conv_b[j] = b.take((size_t)D * 4);
        d->add_f32(q + "bias", d->conv_b[j], {D});
    }
    d->blocks.resize(c.depth);
    for (int i = 0; i < c.depth; ++i) {
        DBlock& w = d->blocks[i];
        const std::string q = p + "transformer_blocks." + std::to_string(i) + ".";
        w.qkv = alloc_mat(b, 3 * D, D, np);
        w.o = alloc_mat(b, D, D, np);
        w.ff1 = alloc_mat(b, FF, D, np);
        w.ff2 = alloc_mat(b, D, FF, np);
        w.bqkv = b.take((size_t)3 * D * 4);
        w.bo = b.take((size_t)D * 4);
        w.bff1 = b.take((size_t)FF * 4);
        w.bff2 = b.take((size_t)D * 4);
        const char* nm[3] = {"to_q", "to_k", "to_v"};
        for (int k = 0; k < 3; ++k) {
            d->add_mat(q + "attn." + nm[k] + ".weight", w.qkv, k * D, D, D, 0, D, 0, {D, D});
            d->add_f32(q + "attn." + nm[k] + ".bias", w.bqkv + (size_t)k * D * 4, {D});
        }
        d->add_mat(q + "attn.to_out.layers.0.weight", w.o, 0, D, D, 0, D, 0, {D, D});
        d->add_f32(q + "attn.to_out.layers.0.bias", w.bo, {D});
        d->add_mat(q + "ff.ff.layers.0.layers.0.weight", w.ff1, 0, FF, D, 0, D, 0, {FF, D});
        d->add_f32(q + "ff.ff.layers.0.layers.0.bias", w.bff1, {FF});
        d->add_mat(q + "ff.ff.layers.2.weight", w.ff2, 0, D, FF, 0, FF, 0, {D, FF});
        d->add_f32(q + "ff.ff.layers.2.bias", w.bff2, {D});
    }
    d->norm_out = b.take((size_t)D * 4);
    d->to_pred = b.take((size_t)D * 4);
    d->add_f32(p + "norm_out.weight", d->norm_out, {D});
    d->add_f32("to_pred.layers.0.weight", d->to_pred, {1, D});
    d->zeros = b.take((size_t)D * 4);      // scale = shift = 0: ln_modulate is the plain LayerNorm of duration.py:86,91
    d->ones = b.take((size_t)D * 4);       // gate = 1: the gated-residual epilogue is `x = x + y`
    d->arena_need = b.off;
    *out = d;
    return 0;
}

extern "C" void f5_duration_destroy(f5_duration* d) {
    delete d;      // (~GraphCache waits for the last replay of every exec)
}

extern "C" int f5_duration_weights_bytes(f5_duration* d, size_t* bytes) {
    F5_REQUIRE(d && bytes, "null argument");
    *bytes = d->arena_need;
    return 0;
}

extern "C" int f5_duration_set_weights_arena(f5_duration* d, void* dev_arena, size_t bytes, void* stream) {
    F5_REQUIRE(d && dev_arena, "null argument");
    return d->set_arena(dev_arena, bytes, (hipStream_t)stream);   // zero pads, the zero vector
}

// Tensor names are the reference's (the keys of duration_param_specs in f5_tts_mlx_amd/duration.py: "transformer.text_embed...",
// "to_pred.layers.0.weight"), with or without the "duration_predictor." prefix they carry inside an F5TTS checkpoint; shapes are the
// reference's (MLX layout).  The name and the shape are checked before the arena, so that a host can validate a checkpoint without a device.
extern "C" int f5_duration_load_tensor(f5_duration* d, const char* name, const float* host, int ndim, const int64_t* shape) {
    F5_REQUIRE(d && name && host && shape, "null argument");
    std::string key(name);
    const std::string prefix = "duration_predictor.";
    if (key.compare(0, prefix.size(), prefix) == 0) key = key.substr(prefix.size());
    std::vector<TensorDst>* dsts = nullptr;
    size_t count = 0;
    RC(d->lookup(key, name, &dsts));
    RC(d->match(name, *dsts, ndim, shape, &count));
    F5_REQUIRE(d->arena, "f5_duration_set_weights_arena must be called first");
    for (TensorDst& t : *dsts) RC(d->upload(t, host, count));      // (conv-pos weights of 32-channel groups are packed on the way in)
    return 0;
}

extern "C" int f5_duration_mark_weights_loaded(f5_duration* d) {
    F5_REQUIRE(d, "null argument");
    d->mark_all_loaded();
    return 0;
}

extern "C" int f5_duration_finalize(f5_duration* d, void* stream) {
    F5_REQUIRE(d && d->arena, "duration predictor arena not set");
    RC(d->require_loaded());
    RC(f5_launch_text_pos_table((float*)(d->arena + d->pos), d->cfg.text_max_pos, d->cfg.text_dim, (hipStream_t)stream));
    const std::vector<float> one((size_t)d->cfg.dim, 1.0f), zero((size_t)d->cfg.dim, 0.0f);
    F5_HIP_CHECK(hipStreamSynchronize((hipStream_t)stream));
    F5_HIP_CHECK(hipMemcpy(d->arena + d->ones, one.data(), one.size() * 4, hipMemcpyHostToDevice));
    F5_HIP_CHECK(hipMemcpy(d->arena + d->zeros, zero.data(), zero.size() * 4, hipMemcpyHostToDevice));
    d->finalized = true;
    return 0;
}

static int dshape_ok(const f5_duration* d, int B, int n_in, int nt) {
    const int N = n_in > nt ? n_in : nt;
    F5_REQUIRE(B >= 1 && n_in >= 1 && nt >= 1, "duration predictor: need B >= 1, n_in >= 1 and nt >= 1 (got B=%d n_in=%d nt=%d)", B, n_in, nt);
    F5_REQUIRE(N >= 4, "duration predictor: need N = max(n_in, nt) >= 4 (got %d)", N);
    F5_REQUIRE(N <= d->cfg.text_max_pos, "duration predictor: N = max(n_in, nt) = %d exceeds text_max_pos = %d", N, d->cfg.text_max_pos);
    const int widest = d->cfg.ff_dim > 3 * d->cfg.dim ? d->cfg.ff_dim : 3 * d->cfg.dim;
    F5_REQUIRE((size_t)B * N * widest < ((size_t)1 << 31), "duration predictor: B * N = %zu rows is too many for one call", (size_t)B * N);
    return 0;
}

static DWorkspace dplan(const f5_duration* d, int B, int n_in, int nt, bool isolated = false) {
    const f5_duration_config& c = d->cfg;
    const int N = n_in > nt ? n_in : nt, npad = (N + 63) / 64 * 64;
    const size_t rows = (size_t)B * N, D = c.dim, Dt = c.text_dim, TF = 2 * Dt, K0 = 128 + Dt;
    Bump b;
    DWorkspace w;
    w.status = b.take(4);
    w.lens = b.take((size_t)B * 4);
    w.text = b.take(rows * 4);                       // [B][nt], nt <= N: sized by N so that the plan depends on (B, N) alone below
    w.mel = b.take(rows * c.mel_dim * 4);            // [B][N][mel_dim], rows >= n_in zero
    w.mask = b.take(rows);
    w.te = b.take(2 * rows * Dt * 4);                // the text_embed kernel writes both branches (cond | dropped text)
    w.ids = b.take(2 * rows * 4);
    w.keep = b.take(2 * rows);
    w.t_nxt = b.take(rows * Dt * 4);
    w.tg = b.take(rows * TF * 4);
    w.scratch = b.take((f5_grn_partial_floats(B, N, (int)TF) + (size_t)B * TF) * 4);
    w.x = b.take(rows * D * 4);
    w.cos_t = b.take((size_t)N * 32 * 4);
    w.sin_t = b.take((size_t)N * 32 * 4);
    w.pred = b.take((size_t)B * 4);
    for (int p = 0; p < 2; ++p) {
        const bool on = p < d->np;
        w.tln[p] = on ? b.take(rows * Dt * 2) : 0;
        w.tg2[p] = on ? b.take(rows * TF * 2) : 0;
        w.a0[p] = on ? b.take(rows * K0 * 2) : 0;
        w.xb[p] = on ? b.take(rows * D * 2) : 0;
        w.c1[p] = on ? b.take(rows * D * 2) : 0;
        w.h[p] = on ? b.take(rows * D * 2) : 0;
        w.qk[p] = on ? b.take(rows * 2 * D * 2) : 0;
        w.vt[p] = on ? b.take((size_t)B * c.heads * 64 * npad * 2) : 0;
        w.ao[p] = on ? b.take(rows * D * 2) : 0;
        w.ffh[p] = on ? b.take(rows * c.ff_dim * 2) : 0;
    }
    if (isolated) w.rowlen = b.take((size_t)B * 4);      // the one buffer the row-isolated call adds: everything above is the plain plan
    w.total = b.off;
    return w;
}

extern "C" int f5_duration_workspace_bytes(f5_duration* d, int B, int n_in, int nt, size_t* bytes) {
    F5_REQUIRE(d && bytes, "null argument");
    RC(dshape_ok(d, B, n_in, nt));
    *bytes = dplan(d, B, n_in, nt).total;
    return 0;
}

// the plan of f5_duration_workspace_bytes plus the staged row lengths of f5_predict_duration_rows ([B] int32 behind it)
extern "C" int f5_duration_workspace_bytes_rows(f5_duration* d, int B, int n_in, int nt, size_t* bytes) {
    F5_REQUIRE(d && bytes, "null argument");
    RC(dshape_ok(d, B, n_in, nt));
    *bytes = dplan(d, B, n_in, nt, true).total;
    return 0;
}

// the launch sequence of DurationPredictor._run_ops (f5_tts_mlx_amd/duration.py), everything on the workspace and the arena.
// rowlen (dev [B], or null = the plain call): the row-isolated mode (docs/duration_rows.md).  Row b reads nothing from its own positions
// n >= rowlen[b]: the text blocks' depthwise conv and GRN, both conv-pos launches and every attention launch take the lengths; the
// launches in between work row by row, and the head's mean stays over n < lens[b].  What positions n >= rowlen[b] hold is never read.
static int duration_body(const f5_duration* d, const DWorkspace& w, char* ws, int B, int N, int nt, const int* rowlen, hipStream_t s) {
    const f5_duration_config& c = d->cfg;
    const Ops& K = d->ops;
    const int D = c.dim, Dt = c.text_dim, TF = 2 * c.text_dim, FF = c.ff_dim, H = c.heads, K0 = 128 + c.text_dim;
    const int rows = B * N, npad = (N + 63) / 64 * 64;
    const LaunchView L{d->arena, ws, d->np, d->ops};
    const int nseg = L.nseg();
    // fp16 handles: the 16-bit packers of the launches issued inside this scope report a clamp into the call's status word
    SatScope sat(d->ops.h, L.p<int>(w.status));
    uint8_t* mask = reinterpret_cast<uint8_t*>(ws + w.mask);
    const uint32_t zero_word = 0;
    RC(f5_launch_stage_words(&zero_word, 1, reinterpret_cast<uint32_t*>(ws + w.status), s));      // status = 0, a kernel like the rest
    RC(K.rowkeep(reinterpret_cast<const int*>(ws + w.lens), mask, B, N, s));                     // mask = n < lens[b]

    // ---- text path, no padding mask (duration.py:116-118)
    RC(K.text_embed(reinterpret_cast<const int*>(ws + w.text), nt, L.a<float>(d->table), L.a<float>(d->pos), c.text_max_pos, L.p<float>(w.te),
                    reinterpret_cast<int*>(ws + w.ids), reinterpret_cast<uint8_t*>(ws + w.keep), B, N, Dt, 0, s));
    float* t_cur = L.p<float>(w.te);            // branch 0
    float* t_nxt = L.p<float>(w.t_nxt);
    float* scratch = L.p<float>(w.scratch);
    for (const DTextBlock& k : d->tblocks) {
        if (rowlen)
            RC(K.dwconv_ln_ragged(t_cur, L.a<float>(k.dw_w), L.a<float>(k.dw_b), L.a<float>(k.ln_w), L.a<float>(k.ln_b), L.pb(w.tln, 0), L.pb(w.tln, 1), B, N, Dt, 1e-6f, rowlen, s));
        else
            RC(K.dwconv_ln(t_cur, L.a<float>(k.dw_w), L.a<float>(k.dw_b), L.a<float>(k.ln_w), L.a<float>(k.ln_b), L.pb(w.tln, 0), L.pb(w.tln, 1), B, N, Dt, 1e-6f, s));
        F5GemmArgs g1 = L.gemm(L.pb(w.tln, 0), L.pb(w.tln, 1), Dt, k.pw1, rows, TF, Dt, L.a<float>(k.b1));
        g1.out_f32 = L.p<float>(w.tg);
        g1.ldo = TF;
        g1.ldob = TF;
        RC(K.gemm(g1, EPI_GELU_ERF, s));
        float* nx = scratch + f5_grn_partial_floats(B, N, TF);
        if (rowlen)
            RC(K.grn_ragged(L.p<float>(w.tg), L.a<float>(k.gamma), L.a<float>(k.beta), scratch, nx, L.pb(w.tg2, 0), L.pb(w.tg2, 1), B, N, TF, rowlen, s));
        else
            RC(K.grn(L.p<float>(w.tg), L.a<float>(k.gamma), L.a<float>(k.beta), scratch, nx, L.pb(w.tg2, 0), L.pb(w.tg2, 1), B, N, TF, s));
        F5GemmArgs g2 = L.gemm(L.pb(w.tg2, 0), L.pb(w.tg2, 1), TF, k.pw2, rows, Dt, TF, L.a<float>(k.b2));
        g2.resid = t_cur;
        g2.ldres = Dt;
        g2.out_f32 = t_nxt;
        g2.ldo = Dt;
        RC(K.gemm(g2, EPI_RESID_KEEP, s));
        float* t = t_cur;
        t_cur = t_nxt;
        t_nxt = t;
    }

    // ---- input embedding: proj(concat(masked mel, text)) + conv_pos_embed (duration.py:44-58, :243-247)
    for (int p = 0; p < d->np; ++p) RC(K.zero_vt_pad(L.pb(w.a0, p), (size_t)rows, 0, K0, s));     // every column: the pad [mel_dim, 128) must be 0
    RC(K.pack_bf16(L.p<float>(w.mel), mask, L.pb(w.a0, 0), L.pb(w.a0, 1), rows, c.mel_dim, K0, 0, s));
    RC(K.pack_bf16(t_cur, nullptr, L.pb(w.a0, 0), L.pb(w.a0, 1), rows, Dt, K0, 128, s));
    F5GemmArgs gp = L.gemm(L.pb(w.a0, 0), L.pb(w.a0, 1), K0, d->proj, rows, D, K0, L.a<float>(d->bproj));
    gp.out_f32 = L.p<float>(w.x);
    gp.ldo = D;
    gp.ldob = D;
    RC(K.gemm(gp, EPI_F32, s));
    RC(K.pack_bf16(L.p<float>(w.x), nullptr, L.pb(w.xb, 0), L.pb(w.xb, 1), rows, D, D, 0, s));
    for (int j = 0; j < 2; ++j) {
        F5ConvPosArgs cp;
        memset(&cp, 0, sizeof(cp));
        cp.in[0] = j == 0 ? L.pb(w.xb, 0) : L.pb(w.c1, 0);
        cp.in[1] = j == 0 ? L.pb(w.xb, 1) : L.pb(w.c1, 1);
        cp.W[0] = L.wm(d->conv_w[j], 0);
        cp.W[1] = L.wm(d->conv_w[j], 1);
        cp.bias = L.a<float>(d->conv_b[j]);
        cp.B = B;
        cp.seq_len = N;
        cp.C = D;
        cp.groups = D / 64;
        cp.taps = c.conv_pos_kernel;
        cp.ld = D;
        cp.ldo = D;
        cp.nseg = nseg;
        cp.mode = j;                                  // 0: c1 = 16-bit(mish(.)); 1: x += mish(.)
        cp.out_bf[0] = j == 0 ? L.pb(w.c1, 0) : nullptr;
        cp.out_bf[1] = j == 0 ? L.pb(w.c1, 1) : nullptr;
        cp.out_f32 = j == 0 ? nullptr : L.p<float>(w.x);
        cp.lens = rowlen;                             // null = the instantiations without row lengths
        RC(K.convpos(cp, s));
    }

    // ---- pre-LN transformer blocks without modulation / gates / masks (duration.py:64-94)
    RC(K.rope_table(L.p<float>(w.cos_t), L.p<float>(w.sin_t), N, 64, s));
    for (int p = 0; p < d->np; ++p) RC(K.zero_vt_pad(L.pb(w.vt, p), (size_t)B * H * 64, N, npad, s));   // columns < N: every QKV epilogue
    for (const DBlock& k : d->blocks) {
        RC(K.ln_modulate(L.p<float>(w.x), L.a<float>(d->zeros), L.a<float>(d->zeros), L.pb(w.h, 0), L.pb(w.h, 1), rows, D, 1e-6f, s));
        RC(K.qkv_rope(L.pb(w.h, 0), L.pb(w.h, 1), L.wm(k.qkv, 0), L.wm(k.qkv, 1), L.a<float>(k.bqkv), L.p<float>(w.cos_t), L.p<float>(w.sin_t), L.pb(w.qk, 0), L.pb(w.qk, 1),
                      L.pb(w.vt, 0), L.pb(w.vt, 1), B, N, npad, H, D, nseg, s));
        F5AttnArgs at;
        memset(&at, 0, sizeof(at));
        at.qk[0] = L.pb(w.qk, 0);
        at.qk[1] = L.pb(w.qk, 1);
        at.vt[0] = L.pb(w.vt, 0);
        at.vt[1] = L.pb(w.vt, 1);
        at.out[0] = L.pb(w.ao, 0);
        at.out[1] = L.pb(w.ao, 1);
        at.B = B;
        at.H = H;
        at.seq_len = N;
        at.npad = npad;
        at.ldqk = 2 * D;
        at.ldo = D;
        at.dmodel = D;
        at.hp = d->np == 2;
        at.scale = 0.125f;
        at.pipe = -1;
        at.kv_len = rowlen;                           // null = every key
        RC(K.attention(at, s));
        F5GemmArgs go = L.gemm(L.pb(w.ao, 0), L.pb(w.ao, 1), D, k.o, rows, D, D, L.a<float>(k.bo));
        go.gate = L.a<float>(d->ones);
        go.out_f32 = L.p<float>(w.x);
        go.ldo = D;
        RC(K.gemm(go, EPI_RESID_GATE, s));
        RC(K.ln_modulate(L.p<float>(w.x), L.a<float>(d->zeros), L.a<float>(d->zeros), L.pb(w.h, 0), L.pb(w.h, 1), rows, D, 1e-6f, s));
        F5GemmArgs g1 = L.gemm(L.pb(w.h, 0), L.pb(w.h, 1), D, k.ff1, rows, FF, D, L.a<float>(k.bff1));
        g1.out_bf[0] = L.pb(w.ffh, 0);
        g1.out_bf[1] = L.pb(w.ffh, 1);
        g1.ldo = FF;
        g1.ldob = FF;
        RC(K.gemm(g1, EPI_GELU_TANH, s));
        F5GemmArgs g2 = L.gemm(L.pb(w.ffh, 0), L.pb(w.ffh, 1), FF, k.ff2, rows, D, FF, L.a<float>(k.bff2));
        g2.gate = L.a<float>(d->ones);
        g2.out_f32 = L.p<float>(w.x);
        g2.ldo = D;
        RC(K.gemm(g2, EPI_RESID_GATE, s));
    }

    // ---- RMSNorm -> masked mean -> Linear(dim -> 1) -> Softplus (duration.py:137,188-190,249-251)
    RC(K.duration_head(L.p<float>(w.x), L.a<float>(d->norm_out), L.a<float>(d->to_pred), mask, L.p<float>(w.pred), B, N, D, 1e-5f, s));
    return 0;
}

// One prediction.  rowlen == null: f5_predict_duration; else host [B] row lengths of f5_predict_duration_rows (already checked).
static int predict(f5_duration* d, const f5_duration_args* a, const uint32_t* rowlen, const char* fn, void* stream) {
    F5_REQUIRE(a->mel && a->text && a->seconds && a->workspace, "%s: null mel / text / seconds / workspace", fn);
    F5_REQUIRE(d->finalized, "duration predictor weights are not finalized");
    const int B = a->B, n_in = a->n_in, nt = a->nt;
    RC(dshape_ok(d, B, n_in, nt));
    F5_REQUIRE(a->frames == nullptr || (a->speed > 0.0f && a->frame_rate > 0.0f), "duration predictor: frames need frame_rate > 0 and speed > 0");
    F5_REQUIRE(((uintptr_t)a->workspace & 255) == 0, "duration predictor workspace must be 256-byte aligned");
    F5_REQUIRE((((uintptr_t)a->mel | (uintptr_t)a->text | (uintptr_t)a->seconds | (uintptr_t)a->frames) & 3) == 0,
               "duration predictor: mel / text / seconds / frames must be 4-byte aligned");
    const DWorkspace w = dplan(d, B, n_in, nt, rowlen != nullptr);
    F5_REQUIRE(a->workspace_bytes >= w.total, "duration predictor workspace too small: %zu < %zu", a->workspace_bytes, w.total);
    const int N = n_in > nt ? n_in : nt, mel = d->cfg.mel_dim;
    hipStream_t s = (hipStream_t)stream;
    char* ws = (char*)a->workspace;
    void* workspace = a->workspace;
    // caller buffers are staged outside the graph: the captured nodes only reference the workspace and the arena, so a replay serves
    // new mel / text / lens (and row lengths) of the same shape
    std::vector<uint32_t> lens((size_t)B);
    for (int b = 0; b < B; ++b) lens[b] = (uint32_t)(a->lens ? a->lens[b] : (rowlen ? n_in : N));
    RC(f5_launch_stage_words(lens.data(), lens.size(), reinterpret_cast<uint32_t*>(ws + w.lens), s));
    if (rowlen) RC(f5_launch_stage_words(rowlen, (size_t)B, reinterpret_cast<uint32_t*>(ws + w.rowlen), s));
    RC(f5_launch_copy_words(a->text, ws + w.text, (size_t)B * nt, s));
    if (n_in == N) {
        RC(f5_launch_copy_words(a->mel, ws + w.mel, (size_t)B * N * mel, s));
    } else {
        // duration.py:218-220: the mel is zero padded to the text length.  The staging buffer seen as B rows of 16-bit words: the
        // columns behind an utterance's n_in frames are zeroed, the frames themselves copied
        RC(d->ops.zero_vt_pad(reinterpret_cast<op16_t*>(ws + w.mel), (size_t)B, n_in * mel * 2, N * mel * 2, s));
        for (int b = 0; b < B; ++b)
            RC(f5_launch_copy_words(a->mel + (size_t)b * n_in * mel, ws + w.mel + (size_t)b * N * mel * 4, (size_t)n_in * mel, s));
    }
    const int* rowlen_dev = rowlen ? reinterpret_cast<const int*>(ws + w.rowlen) : nullptr;
    if (a->use_graph) {
        char key[64];
        snprintf(key, sizeof(key), "B%d n%d nt%d%s", B, n_in, nt, rowlen ? " rows" : "");
        GraphCache::Entry* g = d->graphs.find(key, workspace);
        if (!g) RC(d->graphs.capture(key, workspace, s, 1, [&](int) { return duration_body(d, w, ws, B, N, nt, rowlen_dev, s); }, &g));
        RC(GraphCache::launch(g, s));
    } else {
        RC(duration_body(d, w, ws, B, N, nt, rowlen_dev, s));
    }
    // frame_rate / speed are by-value scalars: they stay outside the graph, like the copies to the caller
    if (a->frames) RC(d->ops.seconds_to_frames(reinterpret_cast<const float*>(ws + w.pred), a->frames, B, a->frame_rate, a->speed, s));
    RC(f5_launch_copy_words(ws + w.pred, a->seconds, (size_t)B, s));
    return 0;
}

// Replaces `self._duration_predictor(cond, text)` and the frame arithmetic of F5TTS.predict_duration (cfm.py:253-262).
extern "C" int f5_predict_duration(f5_duration* d, const f5_duration_args* a, void* stream) {
    F5_REQUIRE(d && a, "f5_predict_duration: null argument");
    return predict(d, a, nullptr, "f5_predict_duration", stream);
}

// The row-isolated prediction of a padded batch (docs/duration_rows.md): row b runs at its own length L[b] = max(lens[b], text_lens[b]),
// the N a call of that row alone would run at (duration.py:218-220), and reads nothing from its positions n >= L[b].  text_lens: host
// [B], one past the row's last text id >= 0.  lens == NULL: every lens[b] = n_in.  Everything is checked before the first launch.
extern "C" int f5_predict_duration_rows(f5_duration* d, const f5_duration_args* a, const int32_t* text_lens, void* stream) {
    F5_REQUIRE(d && a && text_lens, "f5_predict_duration_rows: null argument");
    const int B = a->B, n_in = a->n_in, nt = a->nt;
    RC(dshape_ok(d, B, n_in, nt));
    std::vector<uint32_t> rowlen((size_t)B);
    for (int b = 0; b < B; ++b) {
        const int tl = text_lens[b], ln = a->lens ? a->lens[b] : n_in;
        F5_REQUIRE(tl >= 0 && tl <= nt, "duration predictor: row %d: text_lens = %d is outside [0, nt = %d]", b, tl, nt);
        F5_REQUIRE(ln >= 1 && ln <= n_in, "duration predictor: row %d: lens = %d is outside [1, n_in = %d]", b, ln, n_in);
        const int len = ln > tl ? ln : tl;
        F5_REQUIRE(len >= 4, "duration predictor: row %d: its length max(lens, text_lens) = %d is below 4 (a call of the row alone needs N >= 4)", b, len);
        rowlen[b] = (uint32_t)len;
    }
    return predict(d, a, rowlen.data(), "f5_predict_duration_rows", stream);
}

// Status word of the last f5_predict_duration on the workspace of `a` (its first 32-bit word): F5_STATUS_SATURATED = a producer of a
// 16-bit operand clamped a value beyond +-65 504 (precision f16; always 0 in the bf16 modes).  Synchronises `stream`.
extern "C" int f5_duration_status(f5_duration* d, const f5_duration_args* a, int* flags, void* stream) {
    F5_REQUIRE(d && a && flags && a->workspace && a->workspace_bytes >= 4, "null argument");
    F5_HIP_CHECK(hipMemcpyAsync(flags, (const char*)a->workspace, 4, hipMemcpyDeviceToHost, (hipStream_t)stream));
    F5_HIP_CHECK(hipStreamSynchronize((hipStream_t)stream));
    return 0;
}

extern "C" int f5_duration_graph_count(f5_duration* d) { return d ? d->graphs.size() : -1; }
