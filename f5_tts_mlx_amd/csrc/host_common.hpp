// Host-side plumbing shared by the engine (engine.hip), the vocoder (vocoder.hip) and the duration predictor (duration.hip): declarations of both kernel builds, the
// operand-type dispatch, the weights store (arena plan, tensor map, fp32 -> 16-bit upload), the launch view of a call, the fp16
// saturation scope and the hipGraph cache.
#pragma once
#include <string>
#include <unordered_map>
#include <vector>

// the kernel sources are built twice (bf16 operands: namespace f5bf, fp16 operands: namespace f5hf, op16.hpp); this file is
// built once and sees both sets of declarations
#define F5_F16 0
#include "attention.hpp"
#include "convpos.hpp"
#include "gemm.hpp"
#include "rowops.hpp"
#undef F5_F16
#define F5_F16 1
#include "attention.hpp"
#include "convpos.hpp"
#include "gemm.hpp"
#include "rowops.hpp"
#undef F5_F16

// Host-side view: 16-bit operand buffers are opaque storage (typed as the bf16 build's op16_t), argument structs are the
// bf16 build's; the fp16 build's structs have the same layout (only the pointee type of the operand pointers differs).
typedef f5bf::op16_t op16_t;
using f5bf::F5AttnArgs;
using f5bf::F5ConvPosArgs;
using f5bf::F5GemmArgs;
using f5bf::F5OdeArgs;
// launches that do not touch 16-bit operands (or are bf16-only by definition: the MX-fp8 mode) come from the bf16 build
using f5bf::f5_grn_partial_floats;
using f5bf::f5_launch_duration_head;
using f5bf::f5_launch_gemm_f8;
using f5bf::f5_launch_ln_modulate_f8;
using f5bf::f5_launch_quantize_mx;
using f5bf::f5_launch_quantize_mx_bf16;
using f5bf::f5_launch_rope_table;
using f5bf::f5_launch_rope_table_g4;
using f5bf::f5_launch_rowkeep;
using f5bf::f5_launch_seconds_to_frames;
using f5bf::f5_launch_stage_words;
using f5bf::f5_launch_copy_words;
using f5bf::f5_launch_skinny_gemm;
using f5bf::f5_launch_splice;
using f5bf::f5_launch_splice_keep;
using f5bf::f5_launch_gather_frames;
using f5bf::f5_launch_copy_bytes;
using f5bf::f5_launch_text_embed;
using f5bf::f5_launch_text_pos_table;
using f5bf::f5_launch_time_sinus;

// operands, shape and bias of a GEMM launch on raw operand pointers; everything else zero
static inline F5GemmArgs f5_gemm_args(const void* a_hi, const void* a_lo, const void* w_hi, const void* w_lo, int lda, int ldw, int M, int N,
                                      int K, int nseg, const float* bias) {
    F5GemmArgs g;
    memset(&g, 0, sizeof(g));
    g.A[0] = (const op16_t*)a_hi;
    g.A[1] = (const op16_t*)a_lo;
    g.W[0] = (const op16_t*)w_hi;
    g.W[1] = (const op16_t*)w_lo;
    g.lda = lda;
    g.ldw = ldw;
    g.M = M;
    g.N = N;
    g.K = K;
    g.nseg = nseg;
    g.bias = bias;
    return g;
}
// the same for an MX-fp8 launch: e4m3 operands with their E8M0 block scales, one operand segment
static inline F5GemmArgs f5_gemm_f8_args(const void* a8, const void* a_scales, const void* w8, const void* w_scales, int lda8, int ldw8, int M,
                                         int N, int K, const float* bias) {
    F5GemmArgs g = f5_gemm_args(nullptr, nullptr, nullptr, nullptr, 0, 0, M, N, K, 1, bias);
    g.A8 = (const uint8_t*)a8;
    g.As = (const uint8_t*)a_scales;
    g.W8 = (const uint8_t*)w8;
    g.Ws = (const uint8_t*)w_scales;
    g.lda8 = lda8;
    g.ldw8 = ldw8;
    return g;
}
// what EPI_QKV_ROPE reads beyond operands and shape: q | k out, token-major rotation tables, head geometry, V^T out, the factor folded
// into q (0 = none) and, optionally, the group-major tables of the transposed q / k tiles
static inline void f5_qkv_rope_fields(F5GemmArgs& g, void* qk_hi, void* qk_lo, void* vt_hi, void* vt_lo, const float* rope_cos,
                                      const float* rope_sin, int seq_len, int npad, int heads, int dmodel, float q_premul,
                                      const float* rope_g4q = nullptr, const float* rope_g4k = nullptr) {
    g.out_bf[0] = (op16_t*)qk_hi;
    g.out_bf[1] = (op16_t*)qk_lo;
    g.ldob = 2 * dmodel;
    g.rope_cos = rope_cos;
    g.rope_sin = rope_sin;
    g.seq_len = seq_len;
    g.npad = npad;
    g.heads = heads;
    g.dmodel = dmodel;
    g.vt[0] = (op16_t*)vt_hi;
    g.vt[1] = (op16_t*)vt_lo;
    g.q_premul = q_premul;
    g.rope_g4q = rope_g4q;
    g.rope_g4k = rope_g4k;
}
// attention over q | k rows and V^T as the QKV epilogue leaves them; the MX-fp8 output (out8, out8s, ldo8) stays with the caller
static inline F5AttnArgs f5_attn_args(const void* qk_hi, const void* qk_lo, const void* vt_hi, const void* vt_lo, void* out_hi, void* out_lo,
                                      const int* kv_len, int B, int H, int seq_len, int npad, int dmodel, float scale, int hp, int ldqk,
                                      int ldo, int q_prescaled, int pipe) {
    F5AttnArgs at;
    memset(&at, 0, sizeof(at));
    at.qk[0] = (const op16_t*)qk_hi;
    at.qk[1] = (const op16_t*)qk_lo;
    at.vt[0] = (const op16_t*)vt_hi;
    at.vt[1] = (const op16_t*)vt_lo;
    at.out[0] = (op16_t*)out_hi;
    at.out[1] = (op16_t*)out_lo;
    at.kv_len = kv_len;
    at.B = B;
    at.H = H;
    at.seq_len = seq_len;
    at.npad = npad;
    at.ldqk = ldqk;
    at.ldo = ldo;
    at.dmodel = dmodel;
    at.hp = hp;
    at.scale = scale;
    at.q_prescaled = q_prescaled;
    at.pipe = pipe;
    return at;
}

// Kernels of one operand type.  `h` selects the fp16 build.
struct Ops {
    bool h = false;
    static f5hf::op16_t* H(op16_t* p) { return reinterpret_cast<f5hf::op16_t*>(p); }
    int gemm(const F5GemmArgs& a, int epi, hipStream_t s) const {
        return h ? f5hf::f5_launch_gemm(reinterpret_cast<const f5hf::F5GemmArgs&>(a), epi, s) : f5bf::f5_launch_gemm(a, epi, s);
    }
    int fold_rows(const float* stats, int ld, int nslice, int M, float eps, float* rowf, float* row_shift, hipStream_t s) const {
        return h ? f5hf::f5_launch_fold_rows(stats, ld, nslice, M, eps, rowf, row_shift, s)
                 : f5bf::f5_launch_fold_rows(stats, ld, nslice, M, eps, rowf, row_shift, s);
    }
    // batch: {count, w_stride, bias_stride, mod_stride, out_blk_stride} (gemm.hpp F5FoldBatch), count == 1 = a single problem
    int fold_consts(const op16_t* w, int ldw, const float* bias, const float* scale, const float* shift, size_t vec_stride, int nvec, float* c1,
                    float* c2, size_t out_stride, int N, int K, hipStream_t s, int count = 1, size_t w_stride = 0, size_t bias_stride = 0,
                    size_t mod_stride = 0, size_t out_blk_stride = 0) const {
        if (h) {
            const f5hf::F5FoldBatch bt = {count, w_stride, bias_stride, mod_stride, out_blk_stride};
            return f5hf::f5_launch_fold_consts(reinterpret_cast<const f5hf::op16_t*>(w), ldw, bias, scale, shift, vec_stride, nvec, c1, c2,
                                               out_stride, N, K, s, &bt);
        }
        const f5bf::F5FoldBatch bt = {count, w_stride, bias_stride, mod_stride, out_blk_stride};
        return f5bf::f5_launch_fold_consts(w, ldw, bias, scale, shift, vec_stride, nvec, c1, c2, out_stride, N, K, s, &bt);
    }
    int attention(const F5AttnArgs& a, hipStream_t s) const {
        return h ? f5hf::f5_launch_attention(reinterpret_cast<const f5hf::F5AttnArgs&>(a), s) : f5bf::f5_launch_attention(a, s);
    }
    int convpos(const F5ConvPosArgs& a, hipStream_t s) const {
        return h ? f5hf::f5_launch_convpos(reinterpret_cast<const f5hf::F5ConvPosArgs&>(a), s) : f5bf::f5_launch_convpos(a, s);
    }
    int ode_stage(const F5OdeArgs& a, hipStream_t s) const {
        return h ? f5hf::f5_launch_ode_stage(reinterpret_cast<const f5hf::F5OdeArgs&>(a), s) : f5bf::f5_launch_ode_stage(a, s);
    }
    int ode_stage_rows(const F5OdeArgs& a, const float* cfg_rows, const float* dt_rows, int rows_per_vec, int nvec, hipStream_t s) const {
        return h ? f5hf::f5_launch_ode_stage_rows(reinterpret_cast<const f5hf::F5OdeArgs&>(a), cfg_rows, dt_rows, rows_per_vec, nvec, s)
                 : f5bf::f5_launch_ode_stage_rows(a, cfg_rows, dt_rows, rows_per_vec, nvec, s);
    }
    int ode_stage_dual(const F5OdeArgs& a, const float* text_pred, const float* audio_rows, const float* text_rows, const float* dt_rows,
                       int rows_per_vec, int nvec, hipStream_t s) const {
        return h ? f5hf::f5_launch_ode_stage_dual(reinterpret_cast<const f5hf::F5OdeArgs&>(a), text_pred, audio_rows, text_rows, dt_rows,
                                                  rows_per_vec, nvec, s)
                 : f5bf::f5_launch_ode_stage_dual(a, text_pred, audio_rows, text_rows, dt_rows, rows_per_vec, nvec, s);
    }
    int resid_gate_ln_rows(const float* y, float* x, const float* gate, const uint8_t* rowkeep, const float* ln_scale, const float* ln_shift,
                           op16_t* hi, op16_t* lo, int rows, int dim, int rows_per_vec, int nvec, size_t vec_stride, float eps,
                           hipStream_t s) const {
        return h ? f5hf::f5_launch_resid_gate_ln_rows(y, x, gate, rowkeep, ln_scale, ln_shift, H(hi), H(lo), rows, dim, rows_per_vec, nvec,
                                                      vec_stride, eps, s)
                 : f5bf::f5_launch_resid_gate_ln_rows(y, x, gate, rowkeep, ln_scale, ln_shift, hi, lo, rows, dim, rows_per_vec, nvec,
                                                      vec_stride, eps, s);
    }
    int ln_modulate(const float* x, const float* scale, const float* shift, op16_t* hi, op16_t* lo, int rows, int dim, float eps,
                    hipStream_t s, float* mean_out = nullptr) const {
        return h ? f5hf::f5_launch_ln_modulate(x, scale, shift, H(hi), H(lo), rows, dim, eps, s, mean_out)
                 : f5bf::f5_launch_ln_modulate(x, scale, shift, hi, lo, rows, dim, eps, s, mean_out);
    }
    int dwconv_ln(const float* x, const float* dw_w, const float* dw_b, const float* ln_w, const float* ln_b, op16_t* hi, op16_t* lo,
                  int nbatch, int seq_len, int dim, float eps, hipStream_t s) const {
        return h ? f5hf::f5_launch_dwconv_ln(x, dw_w, dw_b, ln_w, ln_b, H(hi), H(lo), nbatch, seq_len, dim, eps, s)
                 : f5bf::f5_launch_dwconv_ln(x, dw_w, dw_b, ln_w, ln_b, hi, lo, nbatch, seq_len, dim, eps, s);
    }
    int dwconv_ln_ragged(const float* x, const float* dw_w, const float* dw_b, const float* ln_w, const float* ln_b, op16_t* hi,
                         op16_t* lo, int nbatch, int seq_len, int dim, float eps, const int* lens, hipStream_t s) const {
        return h ? f5hf::f5_launch_dwconv_ln_ragged(x, dw_w, dw_b, ln_w, ln_b, H(hi), H(lo), nbatch, seq_len, dim, eps, lens, s)
                 : f5bf::f5_launch_dwconv_ln_ragged(x, dw_w, dw_b, ln_w, ln_b, hi, lo, nbatch, seq_len, dim, eps, lens, s);
    }
    int grn(const float* g, const float* gamma, const float* beta, float* partial, float* nx, op16_t* hi, op16_t* lo, int nbatch,
            int seq_len, int dim, hipStream_t s) const {
        return h ? f5hf::f5_launch_grn(g, gamma, beta, partial, nx, H(hi), H(lo), nbatch, seq_len, dim, s)
                 : f5bf::f5_launch_grn(g, gamma, beta, partial, nx, hi, lo, nbatch, seq_len, dim, s);
    }
    int grn_ragged(const float* g, const float* gamma, const float* beta, float* partial, float* nx, op16_t* hi, op16_t* lo, int nbatch,
                   int seq_len, int dim, const int* lens, hipStream_t s) const {
        return h ? f5hf::f5_launch_grn_ragged(g, gamma, beta, partial, nx, H(hi), H(lo), nbatch, seq_len, dim, lens, s)
                 : f5bf::f5_launch_grn_ragged(g, gamma, beta, partial, nx, hi, lo, nbatch, seq_len, dim, lens, s);
    }
    int pack_cond_text(const float* cond, const int* lens, const float* text_emb, op16_t* hi, op16_t* lo, int B, int seq_len,
                       int mel_dim, int dt, int null_keeps_cond, hipStream_t s) const {
        return h ? f5hf::f5_launch_pack_cond_text(cond, lens, text_emb, H(hi), H(lo), B, seq_len, mel_dim, dt, null_keeps_cond, s)
                 : f5bf::f5_launch_pack_cond_text(cond, lens, text_emb, hi, lo, B, seq_len, mel_dim, dt, null_keeps_cond, s);
    }
    int pack_cond_text_keep(const float* cond, const uint8_t* keep, const float* text_emb, op16_t* hi, op16_t* lo, int B, int seq_len,
                            int mel_dim, int dt, int null_keeps_cond, hipStream_t s) const {
        return h ? f5hf::f5_launch_pack_cond_text_keep(cond, keep, text_emb, H(hi), H(lo), B, seq_len, mel_dim, dt, null_keeps_cond, s)
                 : f5bf::f5_launch_pack_cond_text_keep(cond, keep, text_emb, hi, lo, B, seq_len, mel_dim, dt, null_keeps_cond, s);
    }
    int pack_cond_text_dual(const float* cond, const int* lens, const uint8_t* keep, const float* text_emb, op16_t* hi, op16_t* lo, int B,
                            int seq_len, int mel_dim, int dt, hipStream_t s) const {
        return h ? f5hf::f5_launch_pack_cond_text_dual(cond, lens, keep, text_emb, H(hi), H(lo), B, seq_len, mel_dim, dt, s)
                 : f5bf::f5_launch_pack_cond_text_dual(cond, lens, keep, text_emb, hi, lo, B, seq_len, mel_dim, dt, s);
    }
    int pack_x(const float* y, op16_t* hi, op16_t* lo, int rows, int mel_dim, hipStream_t s) const {
        return h ? f5hf::f5_launch_pack_x(y, H(hi), H(lo), rows, mel_dim, s) : f5bf::f5_launch_pack_x(y, hi, lo, rows, mel_dim, s);
    }
    int layernorm(const float* x, const float* w, const float* b, float* out_f32, op16_t* hi, op16_t* lo, int rows, int dim,
                  float eps, hipStream_t s) const {
        return h ? f5hf::f5_launch_layernorm(x, w, b, out_f32, H(hi), H(lo), rows, dim, eps, s)
                 : f5bf::f5_launch_layernorm(x, w, b, out_f32, hi, lo, rows, dim, eps, s);
    }
    int im2col7(const float* x, op16_t* hi, op16_t* lo, int nbatch, int seq_len, int channels, hipStream_t s) const {
        return h ? f5hf::f5_launch_im2col7(x, H(hi), H(lo), nbatch, seq_len, channels, s)
                 : f5bf::f5_launch_im2col7(x, hi, lo, nbatch, seq_len, channels, s);
    }
    int im2col7_ragged(const float* x, op16_t* hi, op16_t* lo, int nbatch, int seq_len, int channels, const int* lens,
                       hipStream_t s) const {
        return h ? f5hf::f5_launch_im2col7_ragged(x, H(hi), H(lo), nbatch, seq_len, channels, lens, s)
                 : f5bf::f5_launch_im2col7_ragged(x, hi, lo, nbatch, seq_len, channels, lens, s);
    }
    int zero_vt_pad(op16_t* vt, size_t rows, int seq_len, int npad, hipStream_t s) const {
        return h ? f5hf::f5_launch_zero_vt_pad(H(vt), rows, seq_len, npad, s) : f5bf::f5_launch_zero_vt_pad(vt, rows, seq_len, npad, s);
    }
    int pack_bf16(const float* src, const uint8_t* rowkeep, op16_t* hi, op16_t* lo, int rows, int cols, int ld, int col0,
                  hipStream_t s) const {
        return h ? f5hf::f5_launch_pack_bf16(src, rowkeep, H(hi), H(lo), rows, cols, ld, col0, s)
                 : f5bf::f5_launch_pack_bf16(src, rowkeep, hi, lo, rows, cols, ld, col0, s);
    }
    // fused QKV projection + RoPE + V transpose on token-major rotation tables (what f5_op_qkv_rope launches with its hooks unset)
    int qkv_rope(const op16_t* a_hi, const op16_t* a_lo, const op16_t* w_hi, const op16_t* w_lo, const float* bias, const float* rope_cos,
                 const float* rope_sin, op16_t* qk_hi, op16_t* qk_lo, op16_t* vt_hi, op16_t* vt_lo, int B, int seq_len, int npad, int heads,
                 int dmodel, int nseg, hipStream_t s) const {
        F5GemmArgs g = f5_gemm_args(a_hi, a_lo, w_hi, w_lo, dmodel, dmodel, B * seq_len, 3 * dmodel, dmodel, nseg, bias);
        f5_qkv_rope_fields(g, qk_hi, qk_lo, vt_hi, vt_lo, rope_cos, rope_sin, seq_len, npad, heads, dmodel, 0.0f);
        return gemm(g, EPI_QKV_ROPE, s);
    }
    // launches without 16-bit operands: one build serves both operand types
    int text_embed(const int* text, int nt, const float* table, const float* pos_table, int max_pos, float* out, int* ids_out,
                   uint8_t* keep_out, int B, int seq_len, int dim, int mask_padding, hipStream_t s) const {
        return f5_launch_text_embed(text, nt, table, pos_table, max_pos, out, ids_out, keep_out, B, seq_len, dim, mask_padding, s);
    }
    int rope_table(float* cos_t, float* sin_t, int seq_len, int dim_head, hipStream_t s) const {
        return f5_launch_rope_table(cos_t, sin_t, seq_len, dim_head, s);
    }
    int rowkeep(const int* dur, uint8_t* keep, int nbatch, int seq_len, hipStream_t s) const {
        return f5_launch_rowkeep(dur, keep, nbatch, seq_len, s);
    }
    int duration_head(const float* x, const float* g, const float* w, const uint8_t* mask, float* out, int B, int seq_len, int dim,
                      float eps, hipStream_t s) const {
        return f5_launch_duration_head(x, g, w, mask, out, B, seq_len, dim, eps, s);
    }
    int seconds_to_frames(const float* seconds, int* frames, int B, float frame_rate, float speed, hipStream_t s) const {
        return f5_launch_seconds_to_frames(seconds, frames, B, frame_rate, speed, s);
    }
};


#define RC(expr)            \
    do {                    \
        int _rc = (expr);   \
        if (_rc) return _rc; \
    } while (0)

// ------------------------------------------------------------------------------------------------
// arena / workspace bump allocator
// ------------------------------------------------------------------------------------------------
struct Bump {
    size_t off = 0;
    size_t take(size_t bytes) {
        const size_t o = off;
        off += (bytes + 255) & ~(size_t)255;
        return o;
    }
};

struct MatBF {          // bf16 matrix in the arena (hi + optional lo)
    size_t hi = 0, lo = 0;
    int rows = 0, ld = 0;
};

struct TensorDst {      // where (part of) a reference tensor goes
    int kind;           // 0: fp32 copy at off (count elements); 1: bf16 matrix placement
    size_t off = 0;     // kind 0
    MatBF mat;          // kind 1
    int row0 = 0;       // first destination row
    int src_rows = 0, src_cols = 0;
    int c0 = 0, c1 = 0, dst_c0 = 0;  // source column range -> destination column offset
    std::vector<int64_t> shape;
    bool loaded = false;
    int conv_cpg = 0;   // != 0: a conv-pos weight (C, taps, conv_cpg), placed as f5_pack_conv_groups leaves it
};

// Conv-pos weights (C, taps, cpg) in the reference's layout -> the matrix f5_launch_convpos reads, 64 input columns per tap:
//   cpg 64: [C][taps * 64], the tensor as it is;
//   cpg 32: [C][taps * 64], two groups share one block-diagonal 64-wide super group: output channel o keeps its 32 input channels in the
//           half of the 64 columns that holds its group, the other half is zero;
//   cpg 48: [C / 48 * 64][taps * 64], a group in a 64-row tile of its own: rows g * 64 + 0..47 hold the group's output channels with
//           their 48 input channels in columns 0..47, everything else is zero.
static inline int f5_conv_packed_rows(int C, int cpg) { return cpg == 48 ? C / 48 * 64 : C; }
static inline void f5_pack_conv_groups(const float* w, int C, int taps, int cpg, std::vector<float>& m) {
    m.assign((size_t)f5_conv_packed_rows(C, cpg) * taps * 64, 0.0f);
    for (int o = 0; o < C; ++o) {
        const int row = cpg == 48 ? o / 48 * 64 + o % 48 : o;
        const int off = cpg == 32 ? ((o / 32) % 2) * 32 : 0;
        for (int k = 0; k < taps; ++k)
            memcpy(&m[((size_t)row * taps + k) * 64 + off], w + ((size_t)o * taps + k) * cpg, (size_t)cpg * sizeof(float));
    }
}

static inline MatBF alloc_mat(Bump& b, int rows, int ld, int np) {
    MatBF m;
    m.rows = rows;
    m.ld = ld;
    const int rows_pad = (rows + 127) / 128 * 128;  // GEMM reads whole 128-row weight tiles
    m.hi = b.take((size_t)rows_pad * ld * 2);
    m.lo = np == 2 ? b.take((size_t)rows_pad * ld * 2) : 0;
    return m;
}


// upload (part of) one reference tensor: fp32 copy, or rows x column range of a matrix rounded to the 16-bit operand type
// (bf16, or fp16 when f16; np == 2 adds the bf16 residual copy of the 3-pass mode)
static inline int f5_upload_tensor(char* arena, const TensorDst& d, const float* host, size_t count, int np, bool f16) {
    if (d.kind == 0) {
        F5_HIP_CHECK(hipMemcpy(arena + d.off, host, count * 4, hipMemcpyHostToDevice));
        return 0;
    }
    const int ncol = d.c1 - d.c0;
    std::vector<u16> hi((size_t)d.src_rows * ncol), lo;
    if (np == 2) lo.resize(hi.size());
    for (int r = 0; r < d.src_rows; ++r)
        for (int cc = 0; cc < ncol; ++cc) {
            const float v = host[(size_t)r * d.src_cols + d.c0 + cc];
            const u16 h = f16 ? f5_f2h_bits(v) : f5_f2bf_bits(v);
            hi[(size_t)r * ncol + cc] = h;
            if (np == 2) lo[(size_t)r * ncol + cc] = f5_f2bf_bits(v - f5_bf_bits2f(h));
        }
    const size_t dst_off = ((size_t)d.row0 * d.mat.ld + d.dst_c0) * 2;
    F5_HIP_CHECK(hipMemcpy2D(arena + d.mat.hi + dst_off, (size_t)d.mat.ld * 2, hi.data(), (size_t)ncol * 2, (size_t)ncol * 2,
                             d.src_rows, hipMemcpyHostToDevice));
    if (np == 2)
        F5_HIP_CHECK(hipMemcpy2D(arena + d.mat.lo + dst_off, (size_t)d.mat.ld * 2, lo.data(), (size_t)ncol * 2, (size_t)ncol * 2,
                                 d.src_rows, hipMemcpyHostToDevice));
    return 0;
}

// ------------------------------------------------------------------------------------------------
// weight store: the arena plan of one model handle, its tensor map and the loading protocol
// (weights_bytes -> set_arena -> load_tensor ... / mark_all_loaded -> finalize)
// ------------------------------------------------------------------------------------------------
struct WeightStore {
    const char* label = "";   // prefix of the messages: "" (engine), "vocoder ", "duration predictor "
    char* arena = nullptr;
    size_t arena_need = 0, arena_bytes = 0;
    bool finalized = false;
    int np = 1;               // precision parts (1, or 2: hi + lo)
    bool f16 = false;         // 16-bit operand type of the matrices
    std::unordered_map<std::string, std::vector<TensorDst>> tmap;

    void add_f32(const std::string& name, size_t off, std::vector<int64_t> shape) {
        TensorDst d;
        d.kind = 0;
        d.off = off;
        d.shape = shape;
        tmap[name].push_back(d);
    }
    void add_mat(const std::string& name, const MatBF& m, int row0, int src_rows, int src_cols, int c0, int c1, int dst_c0,
                 std::vector<int64_t> shape) {
        TensorDst d;
        d.kind = 1;
        d.mat = m;
        d.row0 = row0;
        d.src_rows = src_rows;
        d.src_cols = src_cols;
        d.c0 = c0;
        d.c1 = c1;
        d.dst_c0 = dst_c0;
        d.shape = shape;
        tmap[name].push_back(d);
    }
    void add_mat(const std::string& name, const MatBF& m, int rows, int cols) { add_mat(name, m, 0, rows, cols, 0, cols, 0, {rows, cols}); }
    // a conv-pos weight (C, taps, cpg), cpg = 32, 48 or 64: the matrix is allocated here, in the packed form of f5_pack_conv_groups
    MatBF add_conv_groups(Bump& b, const std::string& name, int C, int taps, int cpg) {
        const int rows = f5_conv_packed_rows(C, cpg);
        const MatBF m = alloc_mat(b, rows, taps * 64, np);
        add_mat(name, m, 0, rows, taps * 64, 0, taps * 64, 0, {C, taps, cpg});
        tmap[name].back().conv_cpg = cpg;
        return m;
    }

    int set_arena(void* dev_arena, size_t bytes, hipStream_t s) {
        F5_REQUIRE(bytes >= arena_need, "%sweights arena too small: %zu < %zu", label, bytes, arena_need);
        F5_REQUIRE(((uintptr_t)dev_arena & 255) == 0, "%sweights arena must be 256-byte aligned", label);
        arena = (char*)dev_arena;
        arena_bytes = bytes;
        F5_HIP_CHECK(hipMemsetAsync(dev_arena, 0, arena_need, s));   // zero pads
        F5_HIP_CHECK(hipStreamSynchronize(s));
        return 0;
    }
    // destinations of tensor `key`; `name` is what the caller passed (the message names it)
    int lookup(const std::string& key, const char* name, std::vector<TensorDst>** dsts) {
        auto it = tmap.find(key);
        F5_REQUIRE(it != tmap.end(), "unknown %stensor name '%s'", label, name);
        *dsts = &it->second;
        return 0;
    }
    // the exact-shape check of every destination; count = number of elements
    int match(const char* name, const std::vector<TensorDst>& dsts, int ndim, const int64_t* shape, size_t* count) const {
        for (const TensorDst& d : dsts) {
            F5_REQUIRE((int)d.shape.size() == ndim, "tensor '%s': expected %zu dims, got %d", name, d.shape.size(), ndim);
            for (int i = 0; i < ndim; ++i)
                F5_REQUIRE(d.shape[i] == shape[i], "tensor '%s': dim %d is %lld, expected %lld", name, i, (long long)shape[i],
                           (long long)d.shape[i]);
        }
        *count = 1;
        for (int i = 0; i < ndim; ++i) *count *= (size_t)shape[i];
        return 0;
    }
    int upload(TensorDst& d, const float* host, size_t count) {
        if (d.conv_cpg != 0 && d.conv_cpg != 64) {        // narrow conv-pos groups: packed on the way in
            std::vector<float> m;
            f5_pack_conv_groups(host, (int)d.shape[0], (int)d.shape[1], d.conv_cpg, m);
            RC(f5_upload_tensor(arena, d, m.data(), m.size(), np, f16));
            d.loaded = true;
            return 0;
        }
        RC(f5_upload_tensor(arena, d, host, count, np, f16));
        d.loaded = true;
        return 0;
    }
    void mark_all_loaded() {
        for (auto& kv : tmap)
            for (auto& d : kv.second) d.loaded = true;
    }
    int require_loaded() const {
        for (auto& kv : tmap)
            for (auto& d : kv.second) F5_REQUIRE(d.loaded, "%stensor '%s' was never loaded", label, kv.first.c_str());
        return 0;
    }
};

// ------------------------------------------------------------------------------------------------
// launch view: typed pointers into the workspace and the arena of one call, and the GEMM argument base
// ------------------------------------------------------------------------------------------------
struct LaunchView {
    const char* arena;
    char* ws;
    int np;
    Ops ops;
    template <typename T>
    T* p(size_t off) const { return reinterpret_cast<T*>(ws + off); }
    template <typename T>
    const T* a(size_t off) const { return reinterpret_cast<const T*>(arena + off); }
    op16_t* pb(const size_t (&offs)[2], int part) const { return part < np ? reinterpret_cast<op16_t*>(ws + offs[part]) : nullptr; }
    const op16_t* wm(const MatBF& m, int part) const {
        if (part == 0) return reinterpret_cast<const op16_t*>(arena + m.hi);
        return np == 2 ? reinterpret_cast<const op16_t*>(arena + m.lo) : nullptr;
    }
    int nseg() const { return np == 2 ? 3 : 1; }
    F5GemmArgs gemm(const op16_t* a_hi, const op16_t* a_lo, int lda, const MatBF& w, int M, int N, int K, const float* bias) const {
        return f5_gemm_args(a_hi, a_lo, wm(w, 0), wm(w, 1), lda, w.ld, M, N, K, nseg(), bias);
    }
};

// fp16 range detector (op16.hpp): while an active one is alive the 16-bit packers of every launch of the fp16 build report saturation
// into the call's status word (bit F5_STATUS_SATURATED).  Host-side: the pointer travels as a kernel argument, a captured graph keeps
// the status word of the workspace it was captured against (part of the graph key).
struct SatScope {
    int* saved;
    SatScope(bool active, int* status_word) : saved(f5hf::f5_sat_flag_host) {
        if (active) f5hf::f5_sat_flag_host = status_word;
    }
    ~SatScope() { f5hf::f5_sat_flag_host = saved; }
};

// ------------------------------------------------------------------------------------------------
// hipGraph cache of one model handle: captured calls by (key, workspace), least recently used evicted
// ------------------------------------------------------------------------------------------------
struct GraphCache {
    struct Entry {
        std::string key;                    // everything a captured node depends on BY VALUE
        const void* workspace;              // the captured nodes reference this buffer
        std::vector<hipGraphExec_t> execs;  // the segments of the call, launched in order
        uint64_t stamp;                     // last use (LRU)
        hipEvent_t done;                    // recorded after every launch: an exec is only destroyed once its last replay has finished
    };
    std::vector<Entry> entries;
    size_t cap = 8;
    bool purge = true;    // an entry captured against another workspace is dead (the caller re-allocated it): dropped before an insert
    uint64_t clock = 0;

    GraphCache() = default;
    GraphCache(const GraphCache&) = delete;
    GraphCache& operator=(const GraphCache&) = delete;
    ~GraphCache() { clear(); }

    int size() const { return (int)entries.size(); }
    void clear() {
        while (!entries.empty()) erase(entries.size() - 1);
    }
    void set_cap(size_t n) {
        cap = n;
        while (entries.size() > cap) evict_lru();
    }
    Entry* find(const std::string& key, const void* workspace) {
        for (Entry& g : entries)
            if (g.workspace == workspace && g.key == key) {
                g.stamp = ++clock;
                return &g;
            }
        return nullptr;
    }
    // Captures body(0) ... body(nseg - 1) on `s`, one exec each, and inserts the entry.  A failure leaves nothing behind: the graph
    // and the execs built so far are destroyed; the body's return code goes ahead of the HIP error.
    template <typename Body>
    int capture(const std::string& key, const void* workspace, hipStream_t s, int nseg, Body&& body, Entry** out) {
        for (size_t i = purge ? entries.size() : 0; i-- > 0;)
            if (entries[i].workspace != workspace) erase(i);
        while (entries.size() >= cap && !entries.empty()) evict_lru();
        Entry e{key, workspace, {}, 0, nullptr};
        for (int seg = 0; seg < nseg; ++seg) {
            hipGraph_t graph = nullptr;
            hipGraphExec_t exec = nullptr;
            hipError_t err = hipStreamBeginCapture(s, hipStreamCaptureModeThreadLocal);
            int rc = 0;
            if (err == hipSuccess) {
                rc = body(seg);
                err = hipStreamEndCapture(s, &graph);
            }
            if (!rc && err == hipSuccess) err = hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0);
            if (graph) (void)hipGraphDestroy(graph);
            if (rc || err != hipSuccess) {
                destroy_execs(e);
                if (rc) return rc;
                f5_set_error("graph capture failed: %s (segment %d of %d)", hipGetErrorString(err), seg, nseg);
                return 1;
            }
            e.execs.push_back(exec);
        }
        if (hipEventCreateWithFlags(&e.done, hipEventDisableTiming) != hipSuccess) {
            destroy_execs(e);
            f5_set_error("graph capture: hipEventCreateWithFlags failed");
            return 3;
        }
        e.stamp = ++clock;
        entries.push_back(std::move(e));
        *out = &entries.back();
        return 0;
    }
    static int launch(Entry* g, hipStream_t s) {
        for (hipGraphExec_t x : g->execs) F5_HIP_CHECK(hipGraphLaunch(x, s));
        F5_HIP_CHECK(hipEventRecord(g->done, s));
        return 0;
    }

  private:
    static void destroy_execs(Entry& g) {
        for (hipGraphExec_t x : g.execs) (void)hipGraphExecDestroy(x);
        g.execs.clear();
    }
    void erase(size_t i) {
        Entry& g = entries[i];
        if (g.done) {
            (void)hipEventSynchronize(g.done);        // the exec may still be running on the stream of its last launch
            (void)hipEventDestroy(g.done);
        }
        destroy_execs(g);
        entries.erase(entries.begin() + i);
    }
    void evict_lru() {
        size_t lru = 0;
        for (size_t i = 1; i < entries.size(); ++i)
            if (entries[i].stamp < entries[lru].stamp) lru = i;
        erase(lru);
    }
};
