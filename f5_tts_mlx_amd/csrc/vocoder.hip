// Vocos vocoder behind the C ABI: mel (b, n, 100) -> waveform, one call (`f5_vocode`), hipGraph captured.
//
// Reference call sites: cfm.py:19 (import), :399-400 (`self._vocoder(out)` at the end of F5TTS.sample), :446 / :471
// (`Vocos.from_pretrained("lucasnewman/vocos-mel-24khz")` wired into F5TTS).  The implementation of `vocos_mlx` is a third-party
// dependency that is NOT in /root/reference (pyproject.toml:42, unpinned): what runs here is restated from the published Vocos
// architecture (gemelo-ai/vocos `VocosBackbone` + `ISTFTHead`, mel-24khz configuration):
//   embed   = Conv1d(n_mels -> dim, k = 7, pad 3)            -> im2col (tap major, channels padded to 128) + MFMA GEMM
//   norm    = LayerNorm(dim, eps 1e-6)
//   8 x ConvNeXtBlock: depthwise Conv1d(k = 7) -> LayerNorm -> Linear(dim -> 3 dim) -> GELU(erf) -> Linear(3 dim -> dim)
//                      -> x + gamma * (.)                     -> dwconv_ln kernel, two MFMA GEMMs with fused epilogues
//   final_layer_norm, head.out = Linear(dim -> n_fft + 2)     -> (log-magnitude | phase), exp clipped at 1e2
//   ISTFT(n_fft 1024, hop 256, hann, center)                  -> per-frame inverse FFT in LDS + overlap-add, whole batch in 2 launches
// PARITY UNPINNED: no reference-side vector exists for this stage (no vocos_mlx, no checkpoint, no network); tests compare with
// oracle/vocos_oracle.py (a CPU restatement of the same published architecture) and torch.istft.
#include <stdarg.h>

#include <string>
#include <vector>

#include "../../include/f5tts_hip.h"
#include "host_common.hpp"

int f5_launch_istft(const float* x, int ldx, const float* window, float* frames_scratch, float* wave, int B, int nframes, int hop,
                    hipStream_t s);   // audio.hip
int f5_launch_istft_ragged(const float* x, int ldx, const float* window, float* frames_scratch, float* wave, int B, int nframes, int hop,
                           const int* lens, hipStream_t s);   // audio.hip

struct VBlock {
    size_t dw_w, dw_b, ln_w, ln_b, b1, b2, gamma;
    MatBF pw1, pw2;
};
struct VWorkspace {
    size_t total = 0;
    size_t mel, x0, x, y, frames, wave;
    size_t a0[2], h[2], g[2];
    size_t lens;             // int32 [B], staged by f5_vocode_ragged outside the captured part; last, so the plain plan keeps its offsets
};

struct f5_vocoder : WeightStore {
    f5_vocos_config cfg;
    Ops ops;
    MatBF w_embed, w_head;
    size_t b_embed, norm_w, norm_b, fnorm_w, fnorm_b, b_head, window;
    bool embed_loaded = false;
    std::vector<VBlock> blocks;
    GraphCache graphs;       // at most 8; keyed by (B, N, ragged): a ragged graph reads the lengths staged in its workspace
};

extern "C" int f5_vocoder_create(const f5_vocos_config* cfg, int precision, f5_vocoder** out) {
    F5_REQUIRE(cfg && out, "f5_vocoder_create: null argument");
    const f5_vocos_config& c = *cfg;
    F5_REQUIRE(precision == F5_PREC_BF16 || precision == F5_PREC_BF16X3 || precision == F5_PREC_F16,
               "vocoder precision must be bf16, bf16x3 or f16 (got %d)", precision);
    F5_REQUIRE(c.n_fft == 1024, "vocoder: only n_fft = 1024 is supported (got %d)", c.n_fft);
    F5_REQUIRE(c.hop_length > 0 && c.n_fft % c.hop_length == 0, "vocoder: hop_length must divide n_fft");
    F5_REQUIRE(c.n_mels >= 1 && c.n_mels <= 128, "vocoder: n_mels must be in [1, 128]");
    F5_REQUIRE(c.dim % 256 == 0 && c.dim >= 256 && c.dim <= 1024, "vocoder: dim must be 256 / 512 / 768 / 1024");
    F5_REQUIRE(c.intermediate_dim % 128 == 0 && c.intermediate_dim >= 128, "vocoder: intermediate_dim must be a multiple of 128");
    F5_REQUIRE(c.num_layers >= 1 && c.num_layers <= 64, "vocoder: num_layers out of range");
    f5_vocoder* v = new f5_vocoder();
    v->cfg = c;
    v->label = "vocoder ";
    v->np = precision == F5_PREC_BF16X3 ? 2 : 1;
    v->f16 = v->ops.h = precision == F5_PREC_F16;
    const int D = c.dim, I = c.intermediate_dim, NF = c.n_fft + 2;
    Bump b;
    v->w_embed = alloc_mat(b, D, 7 * 128, v->np);      // [co][tap][c padded to 128]; loaded through the layout-aware path
    v->b_embed = b.take((size_t)D * 4);
    v->norm_w = b.take((size_t)D * 4);
    v->norm_b = b.take((size_t)D * 4);
    v->add_f32("backbone.embed.bias", v->b_embed, {D});
    v->add_f32("backbone.norm.weight", v->norm_w, {D});
    v->add_f32("backbone.norm.bias", v->norm_b, {D});
    v->blocks.resize(c.num_layers);
    for (int i = 0; i < c.num_layers; ++i) {
        VBlock& k = v->blocks[i];
        const std::string p = "backbone.convnext." + std::to_string(i) + ".";
        k.dw_w = b.take((size_t)D * 7 * 4);
        k.dw_b = b.take((size_t)D * 4);
        k.ln_w = b.take((size_t)D * 4);
        k.ln_b = b.take((size_t)D * 4);
        k.b1 = b.take((size_t)I * 4);
        k.b2 = b.take((size_t)D * 4);
        k.gamma = b.take((size_t)D * 4);
        k.pw1 = alloc_mat(b, I, D, v->np);
        k.pw2 = alloc_mat(b, D, I, v->np);
        // depthwise weight: upstream (dim, 1, 7) and MLX (dim, 7, 1) are the same bytes, [dim][7]; both shapes are accepted
        v->add_f32(p + "dwconv.weight", k.dw_w, {D, 1, 7});
        v->add_f32(p + "dwconv.bias", k.dw_b, {D});
        v->add_f32(p + "norm.weight", k.ln_w, {D});
        v->add_f32(p + "norm.bias", k.ln_b, {D});
        v->add_mat(p + "pwconv1.weight", k.pw1, I, D);
        v->add_f32(p + "pwconv1.bias", k.b1, {I});
        v->add_mat(p + "pwconv2.weight", k.pw2, D, I);
        v->add_f32(p + "pwconv2.bias", k.b2, {D});
        v->add_f32(p + "gamma", k.gamma, {D});
    }
    v->fnorm_w = b.take((size_t)D * 4);
    v->fnorm_b = b.take((size_t)D * 4);
    v->add_f32("backbone.final_layer_norm.weight", v->fnorm_w, {D});
    v->add_f32("backbone.final_layer_norm.bias", v->fnorm_b, {D});
    v->w_head = alloc_mat(b, NF, D, v->np);
    v->b_head = b.take((size_t)NF * 4);
    v->add_mat("head.out.weight", v->w_head, NF, D);
    v->add_f32("head.out.bias", v->b_head, {NF});
    v->window = b.take((size_t)c.n_fft * 4);
    v->arena_need = b.off;
    *out = v;
    return 0;
}

extern "C" void f5_vocoder_destroy(f5_vocoder* v) {
    delete v;      // (~GraphCache waits for the last replay of every exec)
}

extern "C" int f5_vocoder_weights_bytes(f5_vocoder* v, size_t* bytes) {
    F5_REQUIRE(v && bytes, "null argument");
    *bytes = v->arena_need;
    return 0;
}

extern "C" int f5_vocoder_set_weights_arena(f5_vocoder* v, void* dev_arena, size_t bytes, void* stream) {
    F5_REQUIRE(v && dev_arena, "null argument");
    return v->set_arena(dev_arena, bytes, (hipStream_t)stream);
}

// Tensor names are the upstream Vocos state-dict names (`backbone.embed.weight`, `backbone.convnext.3.pwconv1.weight`,
// `head.out.bias` ...), which are also what an MLX module tree of the same structure produces; conv weights are accepted in the
// PyTorch layout (out, in, k) and in the MLX layout (out, k, in) -- told apart by their shape.  The name and the shape are checked
// before the arena, so that a host can validate a checkpoint without a device.
extern "C" int f5_vocoder_load_tensor(f5_vocoder* v, const char* name, const float* host, int ndim, const int64_t* shape) {
    F5_REQUIRE(v && name && host && shape, "null argument");
    const f5_vocos_config& c = v->cfg;
    if (std::string(name) == "backbone.embed.weight") {
        F5_REQUIRE(ndim == 3 && shape[0] == c.dim, "tensor '%s': expected (dim, n_mels, 7) or (dim, 7, n_mels)", name);
        const bool torch_layout = shape[1] == c.n_mels && shape[2] == 7;
        const bool mlx_layout = shape[1] == 7 && shape[2] == c.n_mels;
        F5_REQUIRE(torch_layout || mlx_layout, "tensor '%s': expected (dim, n_mels, 7) or (dim, 7, n_mels)", name);
        F5_REQUIRE(v->arena, "f5_vocoder_set_weights_arena must be called first");
        std::vector<float> m((size_t)c.dim * 7 * 128, 0.0f);
        for (int co = 0; co < c.dim; ++co)
            for (int tap = 0; tap < 7; ++tap)
                for (int ci = 0; ci < c.n_mels; ++ci)
                    m[((size_t)co * 7 + tap) * 128 + ci] = torch_layout ? host[((size_t)co * c.n_mels + ci) * 7 + tap]
                                                                         : host[((size_t)co * 7 + tap) * c.n_mels + ci];
        TensorDst d;
        d.kind = 1;
        d.mat = v->w_embed;
        d.src_rows = c.dim;
        d.src_cols = 7 * 128;
        d.c0 = 0;
        d.c1 = 7 * 128;
        RC(v->upload(d, m.data(), m.size()));
        v->embed_loaded = true;
        return 0;
    }
    std::vector<TensorDst>* dsts = nullptr;
    RC(v->lookup(name, name, &dsts));
    size_t count = 1;
    for (int i = 0; i < ndim; ++i) count *= (size_t)shape[i];
    for (const TensorDst& d : *dsts) {
        size_t want = 1;
        for (int64_t s : d.shape) want *= (size_t)s;
        bool ok = (int)d.shape.size() == ndim;
        for (int i = 0; ok && i < ndim; ++i) ok = d.shape[i] == shape[i];
        // depthwise conv weight in the MLX layout (dim, 7, 1): same bytes as (dim, 1, 7)
        if (!ok && d.kind == 0 && ndim == 3 && d.shape.size() == 3 && shape[0] == d.shape[0] && shape[1] == 7 && shape[2] == 1) ok = true;
        // LayerScale gamma is sometimes stored (1, 1, dim)
        if (!ok && d.kind == 0 && count == want && d.shape.size() == 1) ok = true;
        F5_REQUIRE(ok && count == want, "tensor '%s': unexpected shape", name);
    }
    F5_REQUIRE(v->arena, "f5_vocoder_set_weights_arena must be called first");
    for (TensorDst& d : *dsts) RC(v->upload(d, host, count));
    return 0;
}

extern "C" int f5_vocoder_mark_weights_loaded(f5_vocoder* v) {
    F5_REQUIRE(v, "null argument");
    v->mark_all_loaded();
    v->embed_loaded = true;
    return 0;
}

extern "C" int f5_vocoder_finalize(f5_vocoder* v, void* stream) {
    F5_REQUIRE(v && v->arena, "vocoder arena not set");
    F5_REQUIRE(v->embed_loaded, "vocoder tensor 'backbone.embed.weight' was never loaded");
    RC(v->require_loaded());
    // periodic Hann window of the ISTFT head (torch.hann_window(n_fft)), computed in double like numpy's np.hanning(n+1)[:-1]
    std::vector<float> win(v->cfg.n_fft);
    for (int i = 0; i < v->cfg.n_fft; ++i) win[i] = (float)(0.5 - 0.5 * cos(2.0 * 3.14159265358979323846 * i / v->cfg.n_fft));
    F5_HIP_CHECK(hipMemcpy(v->arena + v->window, win.data(), win.size() * 4, hipMemcpyHostToDevice));
    (void)stream;
    v->finalized = true;
    return 0;
}

static VWorkspace vplan(const f5_vocoder* v, int B, int N) {
    const f5_vocos_config& c = v->cfg;
    const size_t rows = (size_t)B * N;
    Bump b;
    VWorkspace w;
    w.mel = b.take(rows * c.n_mels * 4);
    w.x0 = b.take(rows * c.dim * 4);
    w.x = b.take(rows * c.dim * 4);
    w.y = b.take(rows * (c.n_fft + 2) * 4);
    w.frames = b.take(rows * c.n_fft * 4);
    w.wave = b.take((size_t)B * c.hop_length * (N > 1 ? N - 1 : 1) * 4);
    for (int p = 0; p < 2; ++p) {
        w.a0[p] = p < v->np ? b.take(rows * 7 * 128 * 2) : 0;
        w.h[p] = p < v->np ? b.take(rows * c.dim * 2) : 0;
        w.g[p] = p < v->np ? b.take(rows * c.intermediate_dim * 2) : 0;
    }
    w.lens = b.take((size_t)B * 4);
    w.total = b.off;
    return w;
}

extern "C" int f5_vocoder_workspace_bytes(f5_vocoder* v, int B, int N, size_t* bytes) {
    F5_REQUIRE(v && bytes, "null argument");
    F5_REQUIRE(B >= 1 && N >= 2, "vocoder: need B >= 1 and N >= 2 frames (got B=%d N=%d)", B, N);
    *bytes = vplan(v, B, N).total;
    return 0;
}

// lens: dev int32 [B] (the staged copy in the workspace) = every row decoded on its own lens[b] frames: the three launches that mix
// time steps stop there; nullptr = every row is N frames long
static int vocode_body(const f5_vocoder* v, const VWorkspace& w, char* ws, int B, int N, const int* lens, hipStream_t s) {
    const f5_vocos_config& c = v->cfg;
    const LaunchView L{v->arena, ws, v->np, v->ops};
    const Ops& K = v->ops;
    const int D = c.dim, I = c.intermediate_dim, NF = c.n_fft + 2, rows = B * N;
    // embed conv as a GEMM over im2col rows
    if (lens)
        RC(K.im2col7_ragged(L.p<float>(w.mel), L.pb(w.a0, 0), L.pb(w.a0, 1), B, N, c.n_mels, lens, s));
    else
        RC(K.im2col7(L.p<float>(w.mel), L.pb(w.a0, 0), L.pb(w.a0, 1), B, N, c.n_mels, s));
    F5GemmArgs ge = L.gemm(L.pb(w.a0, 0), L.pb(w.a0, 1), 7 * 128, v->w_embed, rows, D, 7 * 128, L.a<float>(v->b_embed));
    ge.out_f32 = L.p<float>(w.x0);
    ge.ldo = D;
    RC(K.gemm(ge, EPI_F32, s));
    RC(K.layernorm(L.p<float>(w.x0), L.a<float>(v->norm_w), L.a<float>(v->norm_b), L.p<float>(w.x), nullptr, nullptr, rows, D, 1e-6f, s));
    for (const VBlock& k : v->blocks) {
        if (lens)
            RC(K.dwconv_ln_ragged(L.p<float>(w.x), L.a<float>(k.dw_w), L.a<float>(k.dw_b), L.a<float>(k.ln_w), L.a<float>(k.ln_b), L.pb(w.h, 0), L.pb(w.h, 1), B, N, D, 1e-6f, lens, s));
        else
            RC(K.dwconv_ln(L.p<float>(w.x), L.a<float>(k.dw_w), L.a<float>(k.dw_b), L.a<float>(k.ln_w), L.a<float>(k.ln_b), L.pb(w.h, 0), L.pb(w.h, 1), B, N, D, 1e-6f, s));
        F5GemmArgs g1 = L.gemm(L.pb(w.h, 0), L.pb(w.h, 1), D, k.pw1, rows, I, D, L.a<float>(k.b1));
        g1.out_bf[0] = L.pb(w.g, 0);
        g1.out_bf[1] = L.pb(w.g, 1);
        g1.ldob = I;
        RC(K.gemm(g1, EPI_GELU_ERF_BF16, s));
        F5GemmArgs g2 = L.gemm(L.pb(w.g, 0), L.pb(w.g, 1), I, k.pw2, rows, D, I, L.a<float>(k.b2));
        g2.out_f32 = L.p<float>(w.x);
        g2.ldo = D;
        g2.gate = L.a<float>(k.gamma);                     // LayerScale gamma = the per-column gate of the residual epilogue
        RC(K.gemm(g2, EPI_RESID_GATE, s));
    }
    RC(K.layernorm(L.p<float>(w.x), L.a<float>(v->fnorm_w), L.a<float>(v->fnorm_b), nullptr, L.pb(w.h, 0), L.pb(w.h, 1), rows, D, 1e-6f, s));
    F5GemmArgs gh = L.gemm(L.pb(w.h, 0), L.pb(w.h, 1), D, v->w_head, rows, NF, D, L.a<float>(v->b_head));
    gh.out_f32 = L.p<float>(w.y);
    gh.ldo = NF;
    RC(K.gemm(gh, EPI_F32, s));
    if (lens)
        RC(f5_launch_istft_ragged(L.p<float>(w.y), NF, L.a<float>(v->window), L.p<float>(w.frames), L.p<float>(w.wave), B, N, c.hop_length, lens, s));
    else
        RC(f5_launch_istft(L.p<float>(w.y), NF, L.a<float>(v->window), L.p<float>(w.frames), L.p<float>(w.wave), B, N, c.hop_length, s));
    return 0;
}

// The call behind f5_vocode (lens_host == nullptr) and f5_vocode_ragged, after their argument checks.
static int vocode_run(f5_vocoder* v, const VWorkspace& w, const float* mel, const int32_t* lens_host, int B, int N, float* wave,
                      void* workspace, int use_graph, hipStream_t s) {
    char* ws = (char*)workspace;
    const size_t rows = (size_t)B * N;
    const bool ragged = lens_host != nullptr;
    const int* lens = ragged ? reinterpret_cast<const int*>(ws + w.lens) : nullptr;
    // caller buffers are staged outside the graph: the captured nodes only reference the workspace and the arena
    RC(f5_launch_copy_words(mel, ws + w.mel, rows * v->cfg.n_mels, s));      // copy KERNELS, not memcpy nodes (rowops.hip)
    if (ragged)                                                               // host words through kernel arguments: a replay serves new lengths
        RC(f5_launch_stage_words(reinterpret_cast<const uint32_t*>(lens_host), (size_t)B, reinterpret_cast<uint32_t*>(ws + w.lens), s));
    if (use_graph) {
        char key[64];
        snprintf(key, sizeof(key), "B%d N%d r%d", B, N, (int)ragged);
        GraphCache::Entry* g = v->graphs.find(key, workspace);
        if (!g) RC(v->graphs.capture(key, workspace, s, 1, [&](int) { return vocode_body(v, w, ws, B, N, lens, s); }, &g));
        RC(GraphCache::launch(g, s));
    } else {
        RC(vocode_body(v, w, ws, B, N, lens, s));
    }
    RC(f5_launch_copy_words(ws + w.wave, wave, (size_t)B * v->cfg.hop_length * (N - 1), s));
    return 0;
}

// mel dev [B][N][n_mels] fp32 -> wave dev [B][hop * (N - 1)] fp32.  Replaces `self._vocoder(out)` (cfm.py:399-400).
extern "C" int f5_vocode(f5_vocoder* v, const float* mel, int B, int N, float* wave, void* workspace, size_t workspace_bytes,
                         int use_graph, void* stream) {
    F5_REQUIRE(v && mel && wave && workspace, "f5_vocode: null argument");
    F5_REQUIRE(v->finalized, "vocoder weights are not finalized");
    F5_REQUIRE(B >= 1 && N >= 2, "vocoder: need B >= 1 and N >= 2 frames (got B=%d N=%d)", B, N);
    F5_REQUIRE(((uintptr_t)workspace & 255) == 0, "vocoder workspace must be 256-byte aligned");
    const VWorkspace w = vplan(v, B, N);
    F5_REQUIRE(workspace_bytes >= w.total, "vocoder workspace too small: %zu < %zu", workspace_bytes, w.total);
    return vocode_run(v, w, mel, nullptr, B, N, wave, workspace, use_graph, (hipStream_t)stream);
}

// The same for a padded batch whose row b is lens[b] frames long (no reference counterpart: the reference vocodes the padded batch,
// cfm.py:399-400, and its app loop never has one): row b of `wave` is what f5_vocode gives for mel[b][:lens[b]] alone, then zeros.
extern "C" int f5_vocode_ragged(f5_vocoder* v, const float* mel, const int32_t* lens, int B, int N, float* wave, void* workspace,
                                size_t workspace_bytes, int use_graph, void* stream) {
    F5_REQUIRE(v, "f5_vocode_ragged: the handle is null");
    F5_REQUIRE(mel, "f5_vocode_ragged: mel is null");
    F5_REQUIRE(lens, "f5_vocode_ragged: lens is null");
    F5_REQUIRE(wave, "f5_vocode_ragged: wave is null");
    F5_REQUIRE(workspace, "f5_vocode_ragged: workspace is null");
    F5_REQUIRE(B >= 1, "f5_vocode_ragged: B must be >= 1 (got %d)", B);
    F5_REQUIRE(N >= 2, "f5_vocode_ragged: N must be >= 2 frames (got %d)", N);
    for (int b = 0; b < B; ++b)
        F5_REQUIRE(lens[b] >= 2 && lens[b] <= N, "f5_vocode_ragged: lens[%d] = %d outside 2..N = %d", b, lens[b], N);
    F5_REQUIRE(v->finalized, "f5_vocode_ragged: vocoder weights are not finalized");
    F5_REQUIRE(((uintptr_t)workspace & 255) == 0, "f5_vocode_ragged: workspace must be 256-byte aligned");
    const VWorkspace w = vplan(v, B, N);
    F5_REQUIRE(workspace_bytes >= w.total, "f5_vocode_ragged: workspace too small: %zu < %zu", workspace_bytes, w.total);
    return vocode_run(v, w, mel, lens, B, N, wave, workspace, use_graph, (hipStream_t)stream);
}

extern "C" int f5_vocoder_graph_count(f5_vocoder* v) { return v ? v->graphs.size() : 0; }
