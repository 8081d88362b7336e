// GEMM routing: which kernel f5_launch_gemm (gemm.hip) runs a launch on, decided in ONE place.  Host only, plain C++17, no HIP types,
// the same for both operand builds.  The launcher switches over f5_gemm_route(); the engine asks the same function which kernel a
// launch would reach before it sets argument fields that only that kernel implements (LN fold, fused LN tail); the tests ask it through
// f5_debug_gemm_route.  The tile counts and thresholds below appear nowhere else in the C++ sources.
#pragma once
#include <string>

// GEMM epilogues (csrc/gemm.hip); "BF16" in a name means "the 16-bit operand type of the build" (bf16 or fp16, op16.hpp)
enum F5Epi : int {
    EPI_F32 = 0,         // out_f32 = acc + bias
    EPI_BF16 = 1,        // out_bf  = bf16(acc + bias)
    EPI_GELU_TANH = 2,   // out_bf  = bf16(gelu_tanh(acc + bias))                 (dit.py:94-99)
    EPI_GELU_ERF = 3,    // out_f32 = gelu_erf(acc + bias)                        (convnext_v2.py:50-51)
    EPI_RESID_GATE = 4,  // out_f32 += gate[col] * ((acc + bias) * keep[row])     (dit.py:172-173,319,323)
    EPI_QKV_ROPE = 5,    // q,k: rope(acc + bias) -> qk[row][col]; v -> vt[b,h][d][n] (dit.py:136-158)
    EPI_ADDROWS = 6,     // out_f32 = acc + addrows[row][col]; out_bf = bf16(same)  (dit.py:250 split GEMM)
    EPI_RESID_KEEP = 7,  // out_f32 = (resid[row][col] + acc + bias) * keep[row]  (convnext_v2.py:53-54, dit.py:225)
    EPI_GELU_ERF_BF16 = 8,  // out_bf = bf16(gelu_erf(acc + bias))              (Vocos ConvNeXt block)
};

// one value per launcher the dispatcher can reach, in the order of F5_GEMM_KERNEL_NAME; F5K_NONE = the launch is refused
enum F5GemmKernel : int {
    F5K_NONE = 0, F5K_GEMM256, F5K_RS128, F5K_RING_WIDE_2224, F5K_RING_WIDE_1442, F5K_RING_KS2_1, F5K_RING_KS2_2, F5K_RING8_3, F5K_RING8_2,
    F5K_RING_1_2, F5K_RING_1_1, F5K_CFG_2_2, F5K_CFG_1_2, F5K_CFG_1_1
};
inline constexpr const char* F5_GEMM_KERNEL_NAME[] = {"", "gemm256", "rs128", "ring_wide<2,2,2,4>", "ring_wide<1,4,4,2>", "ring_ks2<1>", "ring_ks2<2>",
                                                      "ring8<3>", "ring8<2>", "ring<1,2>", "ring<1,1>", "cfg<2,2>", "cfg<1,2>", "cfg<1,1>"};

// LN-fold roles a launch can request (gemm.hpp x16_out / fold_stats / fold_rowf); bits, because the argument struct can carry several
enum : unsigned { F5_FOLD_PRODUCER = 1, F5_FOLD_STATS = 2, F5_FOLD_ROWF = 4 };

// what routing reads of a launch, and nothing else
struct F5GemmQuery {
    int epi, M, N, nseg, seq_len;
    bool g4;           // group-major rotation tables set (after f5_launch_gemm cleared them for dmodel % 256, an unaligned bias or flag 16384)
    bool ln_tail;      // the fused LN tail is requested (ln_counter)
    unsigned fold;     // F5_FOLD_* requested
    int debug_flags;   // the launch's flags with the process-wide ones OR-ed in (bits 8 and 256 matter)
};

// the dispatch knobs (f5_debug_set_gemm_tile / _ring / _qkv_tile): one object for both operand builds
struct F5GemmKnobs {
    int tile = 0;      // 0 auto, 1 = 128x128, 2 = 64x128, 3 = 64x64, 4 = 256x256 v2, 5 = 64x128 ring, 6 = 64x64 ring, 8 = 128x192 8-wave ring,
                       // 9 = 128x128 8-wave ring, 10 / 11 = 64x128 / 128x128 split-K ring, 12 / 13 = 8-wave 128x256 ring, 14 = role-split 128x256
    int ring = 1;      // auto mode: small tiles use the global_load_lds ring kernel
    int qkv_tile = 0;  // small-M QKV projection with group-major tables: 0 = auto, 14 = role-split whenever one round, 12 / 13 = 8-wave 128x256 ring
};
namespace f5dbg { inline F5GemmKnobs gemm_knobs; }

struct F5GemmRoute {
    F5GemmKernel kernel;
    const char* refused;   // why, when kernel == F5K_NONE
    // staged: a kernel with the LDS-staged epilogues (256x256 / role-split 128x256) runs one of the three epilogues of the LN fold in
    // several rounds -- the only launches that implement x16_out / stats_out / fold_* in every form.  The single-round QKV launch
    // (qkv14 below) reaches the role-split kernel too, but reports through fold_small, which is how the engine's plan counts it.
    bool staged;
    // fold_small: one of the batch-1-sized (single-round) launches that implement the fold for their role -- EPI_RESID_GATE on
    // ring_ks2<1> (producer), EPI_GELU_TANH on ring8<2> and EPI_QKV_ROPE on rs128 (consumers, statistics form only)
    bool fold_small;
    // ln_fusable: an EPI_RESID_GATE launch of this shape with ldo == N runs a small-tile kernel that implements the fused LN tail (the
    // large-shape kernels have none: at those sizes LN-modulate is HBM-bound, not launch-bound)
    bool ln_fusable;
};

inline constexpr const char* F5_GEMM_MSG_LN_TAIL =
    "gemm: the fused LN tail needs EPI_RESID_GATE on a small-tile shape (f5_gemm_resid_ln_fusable) and ln_* set";

// tile shape: the largest of 128x128 / 64x128 / 64x64 that still gives the 256 CUs >= 1.5 workgroups each (small-batch shapes such as
// M = 1874 are otherwise a fraction of one wave of tiles)
inline F5GemmRoute f5_gemm_route(const F5GemmQuery& q, const F5GemmKnobs& k = f5dbg::gemm_knobs) {
    const auto cdiv = [](long a, long b) { return (a + b - 1) / b; };
    const int epi = q.epi, M = q.M, N = q.N;
    const bool qkv = epi == EPI_QKV_ROPE, n256 = N % 256 == 0, v2ok = n256 && M >= 256;
    const bool fold_epi = epi == EPI_RESID_GATE || epi == EPI_QKV_ROPE || epi == EPI_GELU_TANH;
    const long t256 = cdiv(M, 256) * (N / 256), t128 = cdiv(M, 128) * cdiv(N, 128), t64x128 = cdiv(M, 64) * cdiv(N, 128);
    const bool big = k.tile == 4 || (k.tile == 0 && v2ok && t256 >= 512);
    F5GemmRoute r = {F5K_NONE, nullptr, false, false, false};
    r.ln_fusable = !big && n256 && N >= 256 && N <= 1024 && M <= 64 * 65536;
    const auto refuse = [&](const char* why) {
        r.refused = why;
        return r;
    };
    // staged / small: what the branch knows of the two facts (`small` at the three single-round branches)
    const auto done = [&](F5GemmKernel kern, bool staged = false, bool small = false) {
        r.staged = staged;
        r.fold_small = small && k.tile == 0 && k.ring && !q.ln_tail && q.nseg == 1 && n256 && M >= 1;
        // the small single-round kernels implement the fold for exactly the fold_small launches, in the statistics form
        const bool role_ok = r.fold_small && ((q.fold == F5_FOLD_PRODUCER && epi == EPI_RESID_GATE) || (q.fold == F5_FOLD_STATS && epi == EPI_GELU_TANH));
        if (kern != F5K_GEMM256 && kern != F5K_RS128 && q.fold != 0 && !role_ok)
            return refuse("gemm: the LN fold (x16_out / fold_rowf / fold_stats) needs a launch on the 256x256 or the role-split 128x256 kernel "
                          "(f5_gemm_runs_staged), or one of the batch-1-sized launches of f5_gemm_fold_small in the statistics form");
        r.kernel = kern;
        return r;
    };
    if (q.ln_tail && !(epi == EPI_RESID_GATE && r.ln_fusable)) return refuse(F5_GEMM_MSG_LN_TAIL);
    int sel = k.tile;
    if (big) {
        if (!v2ok) return refuse("gemm: the 256x256 kernel needs N % 256 == 0 and M >= 256");
        return done(F5K_GEMM256, fold_epi);
    }
    if (epi == EPI_F32 || epi == EPI_BF16 || epi == EPI_GELU_TANH || epi == EPI_RESID_GATE || qkv) {
        // role-split 128 x 256 tiles (gemm_rs128.hip): forced by tile 14, or by the QKV-only knob at batch-1-sized shapes
        long t128x256 = cdiv(M, 128) * (N / 256);
        if (qkv && q.seq_len > 0) t128x256 = (long)(M / q.seq_len) * cdiv(q.seq_len, 128) * (N / 256);   // per-element row tiles
        // QKV at batch-1-sized shapes: one round of role-split 128 x 256 tiles when they fill >= 70 % of the CUs (M = 2 x 937: 192 tiles,
        // 22.0 vs 27.3 us for the 64 x 128 register-staged tiles, sample() 78.3 -> 73.7-76.4 ms; smaller grids stay with the small
        // tiles: M = 3 x 431 22.4 vs 18.4 us).  qkv_tile: 0 = this rule, 14 = whenever one round, 12 / 13 = lock-step ring.
        // (the role-split QKV epilogue deals row tiles per batch element: it needs whole sequences, other shapes keep the small tiles)
        const bool qkv_rows_ok = !qkv || (q.seq_len > 0 && M % q.seq_len == 0);
        const bool qkv14 = qkv && sel == 0 && qkv_rows_ok && q.g4 && t128x256 <= 256 && (k.qkv_tile == 14 || (k.qkv_tile == 0 && t128x256 >= 176));
        // MID sizes (batch 2 ... 16: more than one round of small tiles, too few 256 x 256 tiles to fill the chip twice): the role-split
        // 128 x 256 kernel in several rounds instead of the register-staged 128 x 128 kernel of round 1, which is where the `t128 >= 384`
        // fallback below used to send them.  sample() with it forced on every block GEMM (tile 14): batch 2 121.6 -> 110.1 ms, batch 3
        // 167.7 -> 154.5, batch 4 203.7 -> 166.5; equal to the 256 x 256 kernel at batch 8 (328.5 vs 327.4) and 16 (642.5 vs 650.6), whose
        // N = 1024 GEMMs (t256 < 512) fell to the small kernels as well (profiles/r03/mid_batch_dispatch.txt)
        const bool mid = sel == 0 && t128 >= 384 && qkv_rows_ok;
        if ((sel == 14 || qkv14 || mid) && n256 && !q.ln_tail) {
            // tile 14 forces the QKV projection here even with a ragged M % seq_len, which the kernel cannot run: the launch is refused
            // (with the kernel's own message) and not reported as staged: the engine must not plan a fold on it
            if (!qkv_rows_ok) return refuse("gemm_rs128(qkv): M must be a multiple of seq_len");
            return done(F5K_RS128, fold_epi && (sel == 14 || mid), qkv14 && !mid && k.qkv_tile == 0);
        }
        if (sel == 14) sel = 0;     // (an epilogue the role-split kernel lacks keeps 14 and ends on the 64x64 tiles below)
    }
    // batch-1-sized QKV projection with group-major tables: one round of 8-wave 128 x 256 tiles with transposed q / k wave tiles
    // (qkv_tile = 13 / 12) instead of 64 x 128 register-staged tiles (0)
    if (qkv && sel == 0 && (k.qkv_tile == 12 || k.qkv_tile == 13) && q.g4 && n256 && cdiv(M, 128) * (N / 256) <= 256) sel = k.qkv_tile;
    if (sel == 12 || sel == 13) {
        if ((qkv || epi == EPI_BF16 || epi == EPI_GELU_TANH) && n256) return done(sel == 12 ? F5K_RING_WIDE_2224 : F5K_RING_WIDE_1442);
        sel = 0;
    }
    if (sel == 10) return done(F5K_RING_KS2_1);
    if (sel == 11) return done(F5K_RING_KS2_2);
    if (sel == 8 || sel == 9) {
        if (N % (sel == 8 ? 192 : 128) == 0) return done(sel == 8 ? F5K_RING8_3 : F5K_RING8_2);
        sel = 0;
    }
    if (sel == 0 && k.ring) {
        // one round of 8-wave workgroups (measured at M = 937 / 1874, tools/ring8_bench.py): 128x128 tiles when they fill
        // 70-100 % of the CUs (FF1 at batch 1: 15.0 vs 17.5 us), else 64x128 tiles with the K tiles split over two wave
        // groups (out-proj 12.4 vs 13.4 us, FF2 18.2 vs 20-21 us)
        if (N % 128 == 0 && t128 >= 176 && t128 <= 256) return done(F5K_RING8_2, false, epi == EPI_GELU_TANH);
        if (t64x128 >= 176 && t64x128 <= 256) return done(F5K_RING_KS2_1, false, epi == EPI_RESID_GATE && (q.debug_flags & (8 | 256)) == 0);
    }
    if (sel == 0) sel = t128 >= 384 ? 1 : (t64x128 >= 384 ? 2 : 3);
    if (qkv && sel == 3) sel = 2;
    if (qkv && sel == 6) sel = 5;  // the V^T / head mapping wants >= one whole head per tile column
    if (sel == 5) return done(F5K_RING_1_2);
    if (sel == 6) return done(F5K_RING_1_1);
    if (sel == 1) return done(F5K_CFG_2_2);
    if (k.ring) {
        // the ring kernels hold 2 workgroups per CU (512 slots); the register-staged 64x128 kernel needs only 48 KB of
        // LDS (3 per CU, 768 slots): prefer it when that turns two rounds of tiles into one (QKV at M = 2*937: 720 tiles)
        if (sel == 2 && t64x128 > 512 && t64x128 <= 768) return done(F5K_CFG_1_2);
        return done(sel == 2 ? F5K_RING_1_2 : F5K_RING_1_1);
    }
    return done(sel == 2 ? F5K_CFG_1_2 : F5K_CFG_1_1);
}

// the engine's questions (ln_fold_state, the workspace plan, the fused LN tail), under the names the messages above use
inline bool f5_gemm_runs_staged(const F5GemmQuery& q) { return f5_gemm_route(q).staged; }
inline bool f5_gemm_fold_small(const F5GemmQuery& q) { return f5_gemm_route(q).fold_small; }
inline bool f5_gemm_resid_ln_fusable(const F5GemmQuery& q, int ldo) { return f5_gemm_route(q).ln_fusable && ldo == q.N; }

// What a launch reached, in one word: the kernel and what selects its variant (epilogue, group-major tables, fold request); 0 = no
// kernel.  f5_launch_gemm stores the word (one plain store: no allocation on the launch path, harmless when two host threads launch
// at once); the name is composed from it where it is asked for.
inline int f5_gemm_reached(F5GemmKernel kern, const F5GemmQuery& q) { return kern | q.epi << 4 | (q.g4 ? 1 : 0) << 8 | (int)q.fold << 9; }
// the name f5_debug_last_gemm_kernel reports: the route's base name plus the variant the arguments select on that kernel
inline std::string f5_gemm_kernel_name(int reached) {
    const int kern = reached & 15, epi = reached >> 4 & 15;
    const unsigned fold = (unsigned)reached >> 9 & 7u;
    std::string s = F5_GEMM_KERNEL_NAME[kern];
    if (kern == F5K_GEMM256 || kern == F5K_RS128) {
        if (epi == EPI_QKV_ROPE && (reached >> 8 & 1)) s += "+qk_tr";
        if (epi == EPI_QKV_ROPE || epi == EPI_GELU_TANH) s += (fold & F5_FOLD_STATS) ? "+fold_stats" : (fold & F5_FOLD_ROWF) ? "+fold_rowf" : "";
    } else if (fold != 0) {      // (the route has refused every fold request but the two single-round ones)
        s += (fold & F5_FOLD_PRODUCER) ? "+fold_producer" : "+fold_consumer";
    }
    return s;
}
