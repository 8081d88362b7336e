// Flash attention (non-causal, key-padding by per-batch prefix length) for gfx950, head_dim = 64.
// Reference semantics: mx.fast.scaled_dot_product_attention(q, k, v, scale, mask) at dit.py:166.
//
// Layout trick (all softmax state stays lane-local, no LDS round trip for P):
//   S^T = K * Q^T  via v_mfma_f32_32x32x16_bf16 with A = K tile rows (keys), B = Q rows (queries);
//         C layout => lane (l&31) owns ONE query column, its 16 accumulators are 16 of the 32 keys
//         of the block (the other 16 live in lane l^32).  Row max / row sum = in-lane reduction +
//         one exchange with lane^32.
//   O^T = V^T * P^T with A = V^T rows (dims) and B = P^T: the MFMA "k" index only has to be the SAME
//         key for A and B, so P is fed straight from the S accumulators (keys {0-3,8-11}+4*hi per
//         16-key step) and V^T is read from LDS with the matching key permutation.  V is kept
//         transposed in HBM ([b*h][64][npad], written by the QKV GEMM epilogue).
//   O^T's C layout again has query = lane&31, so the online-softmax rescale is a per-lane multiply.
//
// A wave owns 32 queries (or two blocks of 32); the KV tile is 64 keys.  K and V^T tiles go HBM -> LDS with
// global_load_lds into a ring of tiles, counted vmcnt, ONE barrier per tile, no staging VGPRs.  LDS images are
// lane-linear 128-byte rows, so the 16-byte XOR swizzle chunk ^= (row>>1)&7 is applied to the SOURCE address
// and again on every read.  bf16x3 mode (HP) carries hi/lo for Q, K, V and splits P in registers: 3 MFMAs per
// product.
//
// Four kernels share the pieces defined in front of them:
//   f5_attn2_kernel   32 queries per wave, per-tile maximum; bf16 and bf16x3
//   f5_attn2s_kernel  the same with KS wave groups that split the KV range inside the workgroup (small grids)
//   f5_attn2f_kernel  large grids: 64 queries per wave, no per-tile maximum
//   f5_attn2p_kernel  f5_attn2f_kernel's arithmetic, software-pipelined inside the wave
#include "attention.hpp"

namespace F5_NS {

// workgroup -> (query block, batch*head).  Workgroups are dealt to the 8 XCDs round-robin by their linear id, and every query
// block of a head streams that head's whole K / V^T: with a plain (x = query block, y = head) numbering the query blocks of
// a head land on different XCDs and K / V^T is fetched into several private L2s (FETCH_SIZE 1.12 GB per launch at 64 x 16 x
// 937 with 256-query blocks, against 0.37 GB of q + k + v; tools/gpu_pmc_ops.sh).  The launcher therefore uses a 1-D grid of
// 8 * ceil(B*H / 8) * nqb workgroups: XCD = id & 7, and on one XCD consecutive workgroups walk the query blocks of one head
// before moving to the next head (measured +3.5-6 % on the large-grid kernel, tools/attn_prio_bench.py).  A 2-D grid keeps the
// plain numbering.
__device__ __forceinline__ bool attn_block_map(const F5AttnArgs& p, int qrows, int& bh, int& qblk) {
    if (gridDim.y != 1) {
        bh = blockIdx.y;
        qblk = blockIdx.x;
        return true;
    }
    const int nqb = (p.seq_len + qrows - 1) / qrows;
    const int s = blockIdx.x >> 3;
    qblk = s % nqb;
    bh = (s / nqb) * 8 + (blockIdx.x & 7);
    return bh < p.B * p.H;
}

// the whole argument block in ONE scalar-load clause (left alone the compiler loads each field where it is first used: three or
// four dependent s_load / s_waitcnt rounds in the prologue of a kernel that is one latency chain at batch 1).  SCALE: the kernel
// reads p.scale (q not pre-multiplied)
template <bool SCALE>
__device__ __forceinline__ void attn_pin_args(const F5AttnArgs& p) {
    if (SCALE)
        asm volatile("" ::"s"(p.qk[0]), "s"(p.vt[0]), "s"(p.out[0]), "s"(p.kv_len), "s"(p.B), "s"(p.H), "s"(p.seq_len), "s"(p.npad), "s"(p.ldqk),
                     "s"(p.ldo), "s"(p.dmodel), "s"(p.scale), "s"(p.out8));
    else
        asm volatile("" ::"s"(p.qk[0]), "s"(p.vt[0]), "s"(p.out[0]), "s"(p.kv_len), "s"(p.B), "s"(p.H), "s"(p.seq_len), "s"(p.npad), "s"(p.ldqk),
                     "s"(p.ldo), "s"(p.dmodel), "s"(p.out8));
}

// Q^T fragments (the B operand of S^T = K Q^T) of NQB 32-query blocks starting at query q0, NP parts (hi, lo) each, into
// qf[qb * NP + part]: query row q0 + 32 qb + lq of this lane, clamped to the last row of the sequence (a block past the end computes
// on a copy of it and stores nothing)
template <int NQB, int NP>
__device__ __forceinline__ void attn_load_q(op16x8 (&qf)[NQB * NP][4], const F5AttnArgs& p, size_t rowbase, int q0, int lq, int h, int hi) {
#pragma unroll
    for (int qb = 0; qb < NQB; ++qb) {
        int qr = q0 + qb * 32 + lq;
        if (qr > p.seq_len - 1) qr = p.seq_len - 1;
#pragma unroll
        for (int pp = 0; pp < NP; ++pp)
#pragma unroll
            for (int ks = 0; ks < 4; ++ks)
                qf[qb * NP + pp][ks] = *reinterpret_cast<const op16x8*>(p.qk[pp] + (rowbase + qr) * p.ldqk + h * 64 + ks * 16 + hi * 8);
    }
}

// The compiler does not see hand-counted `s_waitcnt vmcnt(N)` (inline asm).  Q fragments loaded from global memory before a tile
// loop are first USED inside the loop, so the compiler's own wait for them lands in the loop body -- as vmcnt(0) on every
// iteration, draining the K / V^T prefetch each time.  A use it can see, placed before the loop, keeps that wait in the prologue.
#define ATTN_PIN_Q(qf_, n0_, n1_)                                                                            \
    _Pragma("unroll") for (int a_ = 0; a_ < (n0_); ++a_)                                                     \
        _Pragma("unroll") for (int b_ = 0; b_ < (n1_); ++b_) asm volatile("" ::"v"((qf_)[a_][b_]));

__device__ __forceinline__ void attn_glds16(const op16_t* gptr, op16_t* lds_wave_base) {
    __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(gptr),
                                     (__attribute__((address_space(3))) void*)(lds_wave_base), 16, 0, 0);
}
__device__ __forceinline__ int attn_swz(int row, int chunk) { return row * 64 + ((chunk ^ ((row >> 1) & 7)) << 3); }
// K tile rows are stored PERMUTED: LDS row i of a 32-key block holds key (i&3) + 4*(i>>3) + 16*((i>>2)&1).  In the
// S^T = K Q^T accumulator layout lane-half hi then owns the 16 CONSECUTIVE keys 16*hi + r (r = register index), so
// the P operand of a 16-key MFMA step is 8 consecutive keys and the matching V^T fragment is ONE ds_read_b128
// (no bank conflicts, no register shuffles) instead of two ds_read_b64 halves.
__device__ __forceinline__ int attn_kperm(int i) { return (i & 32) | ((i & 3) + 4 * ((i >> 3) & 3) + 16 * ((i >> 2) & 1)); }

// workgroup barrier the compiler moves no memory access across (the global_load_lds writes and the LDS reads are invisible to it)
__device__ __forceinline__ void attn_barrier() {
    asm volatile("" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
}
// top of a tile: wait for this thread's own loads of the tile, then make every wave's part visible.  ahead: the next tile's four
// loads were issued behind them and may stay in flight (three-stage ring)
__device__ __forceinline__ void attn_wait_barrier(bool ahead) {
    if (ahead) {
        asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
    } else {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    attn_barrier();
}

// Row sums up to this take the fast path of the kernels without a per-tile maximum (f5_attn2f_kernel has the reasoning): if a
// lane's partial sum of a tile is <= 2^14, every p of it is, inside half's range with the usual relative rounding
constexpr float ATTN_SUM_LIMIT = 16384.0f;

// O^T accumulators of one 32-query block -> MX-fp8: the 64 head dims are two MX blocks (db = 0, 1); a lane holds 16 values of
// each (the other 16 sit in lane ^ 32), 4 consecutive d per accumulator row group -> one 4-byte store each.
__device__ __forceinline__ void attn_store_f8(const F5AttnArgs& p, const f32x16 (&o)[2], float inv, size_t row, int h, int hi) {
#pragma unroll
    for (int db = 0; db < 2; ++db) {
        float am = 0.0f;
#pragma unroll
        for (int e = 0; e < 16; ++e) am = fmaxf(am, fabsf(o[db][e] * inv));
        am = fmaxf(am, __shfl_xor(am, 32, 64));
        const int e8 = f5_mx_scale_byte(am);
        const float sc = inv * f5_mx_inv_scale(e8);
#pragma unroll
        for (int rg = 0; rg < 4; ++rg) {
            const int d = db * 32 + 8 * rg + 4 * hi;
            *reinterpret_cast<uint32_t*>(p.out8 + row * p.ldo8 + h * 64 + d) =
                f5_pack4_fp8(o[db][rg * 4 + 0] * sc, o[db][rg * 4 + 1] * sc, o[db][rg * 4 + 2] * sc, o[db][rg * 4 + 3] * sc);
        }
        if (hi == 0) p.out8s[row * (size_t)(p.dmodel >> 5) + h * 2 + db] = (uint8_t)e8;
    }
}
// end of a 32-query block: O^T / l of query row qr (lane halves hold partial row sums) -> out[0], with the residual in out[1] when
// HP and the buffer is given, or MX-fp8 (one-pass kernels only)
template <bool HP>
__device__ __forceinline__ void attn_store_block(const F5AttnArgs& p, const f32x16 (&o)[2], float l_run, size_t rowbase, int qr, int h,
                                                 int hi) {
    const float l_tot = l_run + __shfl_xor(l_run, 32, 64);
    const float inv = 1.0f / l_tot;
    if (!HP && p.out8) {
        if (qr < p.seq_len) attn_store_f8(p, o, inv, rowbase + qr, h, hi);
    } else if (qr < p.seq_len) {
#pragma unroll
        for (int db = 0; db < 2; ++db)
#pragma unroll
            for (int rg = 0; rg < 4; ++rg) {
                const int d = db * 32 + 8 * rg + 4 * hi;
                const float v0 = o[db][rg * 4 + 0] * inv, v1 = o[db][rg * 4 + 1] * inv;
                const float v2 = o[db][rg * 4 + 2] * inv, v3 = o[db][rg * 4 + 3] * inv;
                const size_t off = (rowbase + qr) * p.ldo + h * 64 + d;
                *reinterpret_cast<u32x2*>(p.out[0] + off) = u32x2{f5_pack2_bounded(v0, v1), f5_pack2_bounded(v2, v3)};
                if (HP && p.out[1])
                    *reinterpret_cast<u32x2*>(p.out[1] + off) = u32x2{f5_pack2_lo(v0, v1), f5_pack2_lo(v2, v3)};
            }
    }
}

// p = exp2(s * c2 - mc) for a 16-register accumulator block, in place, returning the partial row sum: the scale / subtract and the
// sum run as packed v_pk_fma_f32 / v_pk_add_f32 (two values per VALU issue; MFMA and VALU time add on a SIMD, so every VALU
// instruction saved is kernel time, tools/probes/coissue.hip)
typedef float attn_f32x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ attn_f32x2 attn_exp_block(f32x16& s, float c2, float mc, attn_f32x2 sum2) {
    const attn_f32x2 c2v = {c2, c2}, mcv = {mc, mc};
#pragma unroll
    for (int r = 0; r < 16; r += 2) {
        attn_f32x2 t = {s[r], s[r + 1]};
        t = t * c2v - mcv;
        t[0] = __builtin_amdgcn_exp2f(t[0]);
        t[1] = __builtin_amdgcn_exp2f(t[1]);
        s[r] = t[0];
        s[r + 1] = t[1];
        sum2 += t;
    }
    return sum2;
}

// =================================================================================================
// v2: 128 queries per workgroup, per-tile maximum.  K and V^T tiles go HBM -> LDS with global_load_lds into a ring of NST
// tiles (3 for bf16: two tiles in flight while one is consumed; 2 for bf16x3), counted vmcnt, ONE barrier per
// tile, no staging VGPRs (=> 3 workgroups per CU for bf16).  The O rescale is skipped when no lane's running max
// moved (exact: alpha == 1 for every lane).  f5_attn2s_kernel with ONE wave group computes the same bits with the same
// registers, LDS and occupancy, but timed against this kernel (N = 937, 16 heads, medians of ten alternations, this kernel's spread in
// brackets) it was 36.85 -> 36.97 us (0.10) at B = 6 bf16 and 53.80 -> 54.01 us (0.08) at B = 4 bf16x3, and in other builds
// of the same source up to 1 % either way: the two stay separate kernels.
// =================================================================================================
template <bool HP>
__global__ __launch_bounds__(256, HP ? 2 : 3) void f5_attn2_kernel(F5AttnArgs p) {
    constexpr int NP = HP ? 2 : 1;
    constexpr int NST = HP ? 2 : 3;
    constexpr int TILE = 64 * 64;                       // elements per K or V^T tile image
    __shared__ __attribute__((aligned(16))) op16_t smem[NST * NP * 2 * TILE];   // [stage][part][K | V^T][64*64]

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int hi = lane >> 5, lq = lane & 31;
    int bh, qblk;
    if (!attn_block_map(p, 128, bh, qblk)) return;
    const int b = bh / p.H, h = bh - b * p.H;
    const int q0 = qblk * 128 + wave * 32;
    const int kvlen = p.kv_len ? p.kv_len[b] : p.seq_len;
    const int ntile = (kvlen + 63) >> 6;
    const size_t rowbase = (size_t)b * p.seq_len;

    op16x8 qf[NP][4];
    {
        int qr = q0 + lq;
        if (qr > p.seq_len - 1) qr = p.seq_len - 1;
#pragma unroll
        for (int pp = 0; pp < NP; ++pp)
#pragma unroll
            for (int ks = 0; ks < 4; ++ks)
                qf[pp][ks] = *reinterpret_cast<const op16x8*>(p.qk[pp] + (rowbase + qr) * p.ldqk + h * 64 + ks * 16 + hi * 8);
    }

    // staging pointers (advanced by one KV tile per issue: tiles are issued in increasing order) + wave-uniform LDS offsets
    const op16_t* kptr[NP][2];
    const op16_t* vptr[NP][2];
    int krow[2], kcol[2], ldsoff[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int q_ = i * 256 + tid;
        const int srow = q_ >> 3;
        const int schunk = (q_ & 7) ^ ((srow >> 1) & 7);
        krow[i] = attn_kperm(srow);
        kcol[i] = p.dmodel + h * 64 + schunk * 8;
        ldsoff[i] = (i * 256 + wave * 64) * 8;
#pragma unroll
        for (int pp = 0; pp < NP; ++pp) {
            kptr[pp][i] = p.qk[pp] + (rowbase + krow[i]) * p.ldqk + kcol[i];
            vptr[pp][i] = p.vt[pp] + ((size_t)bh * 64 + srow) * p.npad + schunk * 8;
        }
    }
    const size_t kstep = (size_t)64 * p.ldqk;
#define A2_ISSUE(j_)                                                                                         \
    {                                                                                                        \
        op16_t* st_ = smem + ((j_) % NST) * (NP * 2 * TILE);                                                 \
        const bool tail_ = ((j_) * 64 + 63) > p.seq_len - 1;                                                 \
        _Pragma("unroll") for (int i = 0; i < 2; ++i) {                                                      \
            _Pragma("unroll") for (int pp = 0; pp < NP; ++pp) {                                              \
                const op16_t* ks_ = kptr[pp][i];                                                             \
                if (tail_) {                                                                                 \
                    int key_ = (j_) * 64 + krow[i];                                                          \
                    if (key_ > p.seq_len - 1) key_ = p.seq_len - 1;                                          \
                    ks_ = p.qk[pp] + (rowbase + key_) * p.ldqk + kcol[i];                                    \
                }                                                                                            \
                attn_glds16(ks_, st_ + (pp * 2) * TILE + ldsoff[i]);                                         \
                attn_glds16(vptr[pp][i], st_ + (pp * 2 + 1) * TILE + ldsoff[i]);                             \
                kptr[pp][i] += kstep;                                                                        \
                vptr[pp][i] += 64;                                                                           \
            }                                                                                                \
        }                                                                                                    \
    }

    f32x16 o[2];
#pragma unroll
    for (int e = 0; e < 16; ++e) {
        o[0][e] = 0.0f;
        o[1][e] = 0.0f;
    }
    float m_run = -INFINITY, l_run = 0.0f;
    const float c2 = p.q_prescaled ? 1.0f : p.scale * 1.4426950408889634f;

    A2_ISSUE(0);
    if (NST == 3 && ntile > 1) A2_ISSUE(1);
    ATTN_PIN_Q(qf, NP, 4);

    for (int j = 0; j < ntile; ++j) {
        // wait for tile j (own loads), then make every wave's part visible; tile j+1 may stay in flight (NST == 3)
        attn_wait_barrier(NST == 3 && j + 1 < ntile);
        if (j + NST - 1 < ntile) A2_ISSUE(j + NST - 1);   // slot consumed in iteration j-1: every wave is past it

        const op16_t* st = smem + (j % NST) * (NP * 2 * TILE);
        const op16_t* sK = st;
        const op16_t* sV = st + TILE;
        const op16_t* sKl = st + (NP - 1) * 2 * TILE;
        const op16_t* sVl = st + (NP - 1) * 2 * TILE + TILE;

        f32x16 s[2];
        __builtin_amdgcn_s_setprio(1);
#pragma unroll
        for (int kb = 0; kb < 2; ++kb) {
#pragma unroll
            for (int e = 0; e < 16; ++e) s[kb][e] = 0.0f;
#pragma unroll
            for (int ks = 0; ks < 4; ++ks) {
                const int off = attn_swz(kb * 32 + lq, ks * 2 + hi);
                const op16x8 a = *reinterpret_cast<const op16x8*>(&sK[off]);
                s[kb] = F5_MFMA32(a, qf[0][ks], s[kb], 0, 0, 0);
                if (HP) {
                    const op16x8 al = *reinterpret_cast<const op16x8*>(&sKl[off]);
                    s[kb] = F5_MFMA32(al, qf[0][ks], s[kb], 0, 0, 0);
                    s[kb] = F5_MFMA32(a, qf[NP - 1][ks], s[kb], 0, 0, 0);
                }
            }
        }
        __builtin_amdgcn_s_setprio(0);

        const int key0 = j * 64;
        if (key0 + 64 > kvlen) {
#pragma unroll
            for (int kb = 0; kb < 2; ++kb)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int key = key0 + kb * 32 + 16 * hi + r;
                    if (key >= kvlen) s[kb][r] = -INFINITY;
                }
        }
        float tmax = -INFINITY;
#pragma unroll
        for (int kb = 0; kb < 2; ++kb)
#pragma unroll
            for (int r = 0; r < 16; ++r) tmax = fmaxf(tmax, s[kb][r]);
        tmax = fmaxf(tmax, __shfl_xor(tmax, 32, 64));
        if (__any(tmax > m_run)) {          // wave-uniform: rescale only when some lane's running max moved
            const float m_new = fmaxf(m_run, tmax);
            const float alpha = __builtin_amdgcn_exp2f((m_run - m_new) * c2);
            m_run = m_new;
            l_run *= alpha;
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                o[0][e] *= alpha;
                o[1][e] *= alpha;
            }
        }
        const float mc = m_run * c2;
        attn_f32x2 ps2 = {0.0f, 0.0f};
        ps2 = attn_exp_block(s[0], c2, mc, ps2);
        ps2 = attn_exp_block(s[1], c2, mc, ps2);
        l_run += ps2[0] + ps2[1];

#pragma unroll
        for (int ks4 = 0; ks4 < 4; ++ks4) {
            const int kb = ks4 >> 1, sp = ks4 & 1;
            uint32_t pw[4], pwl[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float p0 = s[kb][8 * sp + 2 * e], p1 = s[kb][8 * sp + 2 * e + 1];
                pw[e] = f5_pack2_bounded(p0, p1);
                if (HP) pwl[e] = f5_pack2_lo(p0, p1);
            }
            const op16x8 pb = __builtin_bit_cast(op16x8, u32x4{pw[0], pw[1], pw[2], pw[3]});
            op16x8 pbl = pb;
            if (HP) pbl = __builtin_bit_cast(op16x8, u32x4{pwl[0], pwl[1], pwl[2], pwl[3]});
            __builtin_amdgcn_s_setprio(1);
#pragma unroll
            for (int db = 0; db < 2; ++db) {
                const int voff = attn_swz(db * 32 + lq, 4 * kb + 2 * hi + sp);
                const op16x8 a = *reinterpret_cast<const op16x8*>(&sV[voff]);
                o[db] = F5_MFMA32(a, pb, o[db], 0, 0, 0);
                if (HP) {
                    const op16x8 al = *reinterpret_cast<const op16x8*>(&sVl[voff]);
                    o[db] = F5_MFMA32(al, pb, o[db], 0, 0, 0);
                    o[db] = F5_MFMA32(a, pbl, o[db], 0, 0, 0);
                }
            }
            __builtin_amdgcn_s_setprio(0);
        }
    }

    const float l_tot = l_run + __shfl_xor(l_run, 32, 64);
    const float inv = 1.0f / l_tot;
    const int qr = q0 + lq;
    if (!HP && p.out8) {
        if (qr < p.seq_len) attn_store_f8(p, o, inv, rowbase + qr, h, hi);
    } else if (qr < p.seq_len) {
#pragma unroll
        for (int db = 0; db < 2; ++db)
#pragma unroll
            for (int rg = 0; rg < 4; ++rg) {
                const int d = db * 32 + 8 * rg + 4 * hi;
                const float v0 = o[db][rg * 4 + 0] * inv, v1 = o[db][rg * 4 + 1] * inv;
                const float v2 = o[db][rg * 4 + 2] * inv, v3 = o[db][rg * 4 + 3] * inv;
                const size_t off = (rowbase + qr) * p.ldo + h * 64 + d;
                *reinterpret_cast<u32x2*>(p.out[0] + off) = u32x2{f5_pack2_bounded(v0, v1), f5_pack2_bounded(v2, v3)};
                if (HP && p.out[1])
                    *reinterpret_cast<u32x2*>(p.out[1] + off) = u32x2{f5_pack2_lo(v0, v1), f5_pack2_lo(v2, v3)};
            }
    }
}

// =================================================================================================
// v2f (large grids, default): v2w with the softmax BOOKKEEPING taken off the per-tile path.  MFMA time and VALU time add on a
// SIMD (tools/probes/coissue.hip), and at head dim 64 a key costs more VALU than MFMA issue time, so every instruction removed
// from the softmax is kernel time.  Two things go:
//  (1) the running maximum.  v2w needs max(S) of every tile (32 v_max3 + a cross-lane exchange through the LDS pipe per
//      query block) only to find out that the reference point m_ref of the exponentials does not have to move.  Here the fast
//      path never looks at the scores: p = exp2(s - m_ref) is computed unconditionally and the ROW SUMS, which are needed
//      anyway, tell whether that was safe: if a lane's partial sum of a tile is <= 2^14, every p of it is <= 2^14, inside
//      half's range with the usual relative rounding; the O / l accumulators are fp32.  Only when some sum is larger (or inf:
//      a score more than 2^14 above the reference point), and on the first tile, the wave takes the slow path -- recompute
//      the scores of the tile (K is still in LDS), take the true maximum, move m_ref there, rescale O and l -- which is v2w's
//      arithmetic.  Softmax is shift invariant, so any reference point gives the same normalised result.
//  (2) the scale / subtract.  With q pre-multiplied by scale * log2(e) in the QKV epilogue (p.q_prescaled; PRE) the MFMA
//      result is already in exp2 units, and -m_ref enters as the C operand of the first QK^T MFMA of a block (16 registers per
//      query block holding the same per-lane value, rewritten only on the slow path): the accumulator leaves the matrix core
//      as s - m_ref and goes straight into v_exp_f32.  Without PRE the packed fma of v2w stays.
// Per 64-key tile and wave: 32 MFMAs next to 64 v_exp + 32 v_pk_add + 32 v_cvt_pk (+ 32 v_pk_fma without PRE), against
// v2w's additional 32 v_max3 + 10 v_max + 2 ds_bpermute round trips + the rescale test.
// =================================================================================================
__device__ __forceinline__ attn_f32x2 attn_exp_block_pre(f32x16& s, attn_f32x2 sum2) {
#pragma unroll
    for (int r = 0; r < 16; r += 2) {
        attn_f32x2 t;
        t[0] = __builtin_amdgcn_exp2f(s[r]);
        t[1] = __builtin_amdgcn_exp2f(s[r + 1]);
        s[r] = t[0];
        s[r + 1] = t[1];
        sum2 += t;
    }
    return sum2;
}

template <bool PRE>
__global__ __launch_bounds__(256, 2) void f5_attn2f_kernel(F5AttnArgs p) {
    constexpr int NST = 3;
    constexpr int TILE = 64 * 64;
    __shared__ __attribute__((aligned(16))) op16_t smem[NST * 2 * TILE];   // [stage][K | V^T][64*64]

    attn_pin_args<true>(p);
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int hi = lane >> 5, lq = lane & 31;
    int bh, qblk;
    if (!attn_block_map(p, 256, bh, qblk)) return;
    const int b = bh / p.H, h = bh - b * p.H;
    const int q0 = qblk * 256 + wave * 64;
    const int kvlen = p.kv_len ? p.kv_len[b] : p.seq_len;
    const int ntile = (kvlen + 63) >> 6;
    const size_t rowbase = (size_t)b * p.seq_len;
    // wave-uniform: at N = 937 one wave in 16 lies entirely past the sequence; it used to compute on clamped rows (6 % of the
    // launch's MFMA and softmax work, thrown away at the store -- on a power-limited part that is 6 % of the time)
    const bool live = q0 < p.seq_len;

    op16x8 qf[2][4];
    attn_load_q<2, 1>(qf, p, rowbase, q0, lq, h, hi);

    const op16_t* kptr[2];
    const op16_t* vptr[2];
    int krow[2], kcol[2], ldsoff[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int q_ = i * 256 + tid;
        const int srow = q_ >> 3;
        const int schunk = (q_ & 7) ^ ((srow >> 1) & 7);
        krow[i] = attn_kperm(srow);
        kcol[i] = p.dmodel + h * 64 + schunk * 8;
        ldsoff[i] = (i * 256 + wave * 64) * 8;
        kptr[i] = p.qk[0] + (rowbase + krow[i]) * p.ldqk + kcol[i];
        vptr[i] = p.vt[0] + ((size_t)bh * 64 + srow) * p.npad + schunk * 8;
    }
    const size_t kstep = (size_t)64 * p.ldqk;
#define A2F_ISSUE(j_)                                                                                        \
    {                                                                                                        \
        op16_t* st_ = smem + ((j_) % NST) * (2 * TILE);                                                      \
        const bool tail_ = ((j_) * 64 + 63) > p.seq_len - 1;                                                 \
        _Pragma("unroll") for (int i = 0; i < 2; ++i) {                                                      \
            const op16_t* ks_ = kptr[i];                                                                     \
            if (tail_) {                                                                                     \
                int key_ = (j_) * 64 + krow[i];                                                              \
                if (key_ > p.seq_len - 1) key_ = p.seq_len - 1;                                              \
                ks_ = p.qk[0] + (rowbase + key_) * p.ldqk + kcol[i];                                         \
            }                                                                                                \
            attn_glds16(ks_, st_ + ldsoff[i]);                                                               \
            attn_glds16(vptr[i], st_ + TILE + ldsoff[i]);                                                    \
            kptr[i] += kstep;                                                                                \
            vptr[i] += 64;                                                                                   \
        }                                                                                                    \
    }
    // S^T blocks of the current tile for both query blocks; USE_M: accumulate on top of -m_ref (PRE fast path)
#define A2F_QK(USE_M)                                                                                        \
    {                                                                                                        \
        __builtin_amdgcn_s_setprio(1);                                                                       \
        _Pragma("unroll") for (int kb = 0; kb < 2; ++kb) {                                                   \
            _Pragma("unroll") for (int ks = 0; ks < 4; ++ks) {                                               \
                const op16x8 a = *reinterpret_cast<const op16x8*>(&sK[attn_swz(kb * 32 + lq, ks * 2 + hi)]); \
                s[0][kb] = F5_MFMA32(a, qf[0][ks], ks == 0 ? ((USE_M) ? mneg[0] : zero16) : s[0][kb], 0, 0, 0); \
                s[1][kb] = F5_MFMA32(a, qf[1][ks], ks == 0 ? ((USE_M) ? mneg[1] : zero16) : s[1][kb], 0, 0, 0); \
            }                                                                                                \
        }                                                                                                    \
        __builtin_amdgcn_s_setprio(0);                                                                       \
        if (j * 64 + 64 > kvlen) {                                                                           \
            _Pragma("unroll") for (int qb = 0; qb < 2; ++qb)                                                 \
                _Pragma("unroll") for (int kb = 0; kb < 2; ++kb)                                             \
                    _Pragma("unroll") for (int r = 0; r < 16; ++r) {                                         \
                        const int key = j * 64 + kb * 32 + 16 * hi + r;                                      \
                        if (key >= kvlen) s[qb][kb][r] = -INFINITY;                                          \
                    }                                                                                        \
        }                                                                                                    \
    }

    f32x16 o[2][2], mneg[2], zero16;
#pragma unroll
    for (int e = 0; e < 16; ++e) {
        zero16[e] = 0.0f;
#pragma unroll
        for (int qb = 0; qb < 2; ++qb) {
            o[qb][0][e] = 0.0f;
            o[qb][1][e] = 0.0f;
            mneg[qb][e] = 0.0f;
        }
    }
    float m_ref[2] = {-INFINITY, -INFINITY}, l_run[2] = {0.0f, 0.0f};   // m_ref in exp2 units (scores * c2)
    const float c2 = PRE ? 1.0f : p.scale * 1.4426950408889634f;

    A2F_ISSUE(0);
    if (ntile > 1) A2F_ISSUE(1);
    ATTN_PIN_Q(qf, 2, 4);

    for (int j = 0; j < ntile; ++j) {
        attn_wait_barrier(j + 1 < ntile);
        if (j + NST - 1 < ntile) A2F_ISSUE(j + NST - 1);

        const op16_t* sK = smem + (j % NST) * (2 * TILE);
        const op16_t* sV = sK + TILE;

        if (!live) continue;                              // a wave entirely past the sequence only stages tiles and keeps the barriers
        f32x16 s[2][2];                                   // [query block][key block]
        float psum[2];
        bool slow = j == 0;
        if (!slow) {
            A2F_QK(PRE);
            bool bad = false;
#pragma unroll
            for (int qb = 0; qb < 2; ++qb) {
                attn_f32x2 ps2 = {0.0f, 0.0f};
                if (PRE) {
                    ps2 = attn_exp_block_pre(s[qb][0], ps2);
                    ps2 = attn_exp_block_pre(s[qb][1], ps2);
                } else {
                    ps2 = attn_exp_block(s[qb][0], c2, m_ref[qb], ps2);
                    ps2 = attn_exp_block(s[qb][1], c2, m_ref[qb], ps2);
                }
                psum[qb] = ps2[0] + ps2[1];
                bad = bad || !(psum[qb] <= ATTN_SUM_LIMIT);
            }
            slow = __any(bad);
        }
        if (slow) {                                       // wave-uniform: first tile, or a score far above the reference point
            A2F_QK(false);
#pragma unroll
            for (int qb = 0; qb < 2; ++qb) {
                float tmax = -INFINITY;
#pragma unroll
                for (int kb = 0; kb < 2; ++kb)
#pragma unroll
                    for (int r = 0; r < 16; ++r) tmax = fmaxf(tmax, s[qb][kb][r]);
                tmax = fmaxf(tmax, __shfl_xor(tmax, 32, 64));
                const float m_new = fmaxf(m_ref[qb], tmax * c2);
                const float alpha = __builtin_amdgcn_exp2f(m_ref[qb] - m_new);
                m_ref[qb] = m_new;
                l_run[qb] *= alpha;
#pragma unroll
                for (int e = 0; e < 16; ++e) {
                    o[qb][0][e] *= alpha;
                    o[qb][1][e] *= alpha;
                    mneg[qb][e] = -m_new;
                }
                attn_f32x2 ps2 = {0.0f, 0.0f};
                ps2 = attn_exp_block(s[qb][0], c2, m_new, ps2);
                ps2 = attn_exp_block(s[qb][1], c2, m_new, ps2);
                psum[qb] = ps2[0] + ps2[1];
            }
        }
        l_run[0] += psum[0];
        l_run[1] += psum[1];

#pragma unroll
        for (int ks4 = 0; ks4 < 4; ++ks4) {
            const int kb = ks4 >> 1, sp = ks4 & 1;
            op16x8 pb[2];
#pragma unroll
            for (int qb = 0; qb < 2; ++qb) {
                uint32_t pw[4];
#pragma unroll
                for (int e = 0; e < 4; ++e) pw[e] = f5_pack2_bounded(s[qb][kb][8 * sp + 2 * e], s[qb][kb][8 * sp + 2 * e + 1]);
                pb[qb] = __builtin_bit_cast(op16x8, u32x4{pw[0], pw[1], pw[2], pw[3]});
            }
            __builtin_amdgcn_s_setprio(1);
#pragma unroll
            for (int db = 0; db < 2; ++db) {
                const op16x8 a = *reinterpret_cast<const op16x8*>(&sV[attn_swz(db * 32 + lq, 4 * kb + 2 * hi + sp)]);
                o[0][db] = F5_MFMA32(a, pb[0], o[0][db], 0, 0, 0);
                o[1][db] = F5_MFMA32(a, pb[1], o[1][db], 0, 0, 0);
            }
            __builtin_amdgcn_s_setprio(0);
        }
    }
#undef A2F_ISSUE
#undef A2F_QK

#pragma unroll
    for (int qb = 0; qb < 2; ++qb) attn_store_block<false>(p, o[qb], l_run[qb], rowbase, q0 + qb * 32 + lq, h, hi);
}

// =================================================================================================
// v2p (large grids, q pre-multiplied): v2f's arithmetic, software-pipelined INSIDE the wave, ONE wave per SIMD.
//
// A wave's VALU / LDS instructions overlap matrix work only when they sit between the MFMAs of the SAME instruction stream: a
// 32-cycle v_mfma_f32_32x32x16 leaves ~8 issue slots, of which ~5 can be filled for free (MI355X_MICROARCH.md, "one wave per SIMD");
// two co-resident waves do not do that for each other (tools/probes/coissue.hip).  v2f runs S = K Q^T -> exp -> O += V^T P one after
// the other, so per 64-key tile its 32 MFMAs (1 024 cycles) and ~160 VALU + 16 LDS reads ADD: 2 720 cycles per wave tile.  The
// round-2 attempt at in-wave pipelining (v5) kept 32 queries per wave -- one LDS fragment per MFMA -- and the per-tile maximum:
// 9+ fillers per MFMA, slower.  With v2f's softmax (no tile maximum, -m_ref as the C operand of the first QK^T MFMA, scores already
// in exp2 units) and 64 queries per wave (every K / V^T fragment feeds TWO MFMAs) a 64-key tile is 32 MFMAs next to
//     64 v_exp_f32 + 64 v_add_f32 + 32 v_cvt_pk + 16 ds_read_b128  =  5.5 fillers per MFMA.
// The pipeline step is HALF a tile (32 keys x 64 queries).  Half-step (j, kb) issues, as ONE stream of independent work,
//     MFMA:  S(next half) = K Q^T - m_ref      (8: the other key block of tile j, or key block 0 of tile j+1)
//            O^T += V^T(prev half) P(prev half) (8: P packed in the previous half-step)
//     VALU:  P(j, kb) = exp2(S(j, kb)), row sums (S computed in the previous half-step)
// as 16 half-slots of {2 exp, 2 add + 1 cvt_pk of the previous pair, 1 MFMA, every other one a fragment read three fragments ahead},
// pinned with sched_barrier.  S and P are double-buffered per key block (static roles: block 0 <-> buffer A, block 1 <-> buffer B).
//
// Registers.  VALU instructions cannot read the accumulator half of the register file, an MFMA's C and D must sit in the same
// half, and left to itself the compiler parks MFMA results in AGPRs as soon as a kernel needs more than 256 registers and copies
// them back one v_accvgpr_read at a time (the first build of this kernel: 130 reads + 226 writes per tile, 362 spilled registers).
// So the MFMAs are inline asm with the register class in the constraint: O^T (64), Q^T (32) and the K / V^T fragments (16) live in
// AGPRs ("a"); the two S buffers (64), -m_ref (32) and the two P buffers (32) in VGPRs ("v").  An asm MFMA is opaque to the
// compiler's hazard padding; the places where an MFMA result or operand is touched by another instruction class within the hazard
// window are padded by hand (A2P_PAD, s_nop 1).
//
// LDS: a K ring and a V^T ring of 4 stages each (2 x 32 KB), tile t in stage t & 3.  Iteration j reads K(j) (key block 1), K(j+1)
// (key block 0), V^T(j-1) (second half) and V^T(j) (first half); after its barrier it issues K(j+3) and V^T(j+2) (global_load_lds,
// uniform base + 32-bit lane offset), and the counted wait at its top lets the previous iteration's group stay in flight: every
// tile has two iterations to arrive (the first build issued one tile ahead behind vmcnt(0): each iteration then waited out a full
// HBM / L2 round trip, 4 800 cycles per tile).  One barrier per tile.  The tile loop is unrolled four times so that every fragment
// address is one loop-invariant VGPR plus an immediate.
// The slow path (a row sum above 2^14: some score far above the reference point) runs at the END of the half-step: S(j, kb) is
// still in registers (the exponentials are not taken in place), so the reference point moves by delta = max(S) and O, l, -m_ref,
// the already computed next S and this P follow.  The first half tile takes its true maximum in the prologue.  Same layouts
// (permuted K rows, XOR-swizzled 128-byte rows, P fed from the S accumulators) and the same results as v2f up to the order of the
// row-sum additions and the reference point of the rows.
// =================================================================================================
#if F5_F16
#define A2P_MFMA_OP "v_mfma_f32_32x32x16_f16"
#else
#define A2P_MFMA_OP "v_mfma_f32_32x32x16_bf16"
#endif
// 20 wait states: more than the 12 an 8-pass MFMA needs before another instruction class may touch its result
#define A2P_PAD "s_nop 15\n\ts_nop 3"
#define ATTN2P_TILE (64 * 64)
// The compiler may place a register copy (v_mov / v_accvgpr_mov / v_accvgpr_write, or the v_cvt_pk that produced a P word) directly in
// front of an asm statement; a VALU result needs 2 wait states before an MFMA may read it and the hazard recogniser does not look
// into asm (first build: stale O accumulators and P words wherever such a copy sat in front of an MFMA).  Every asm MFMA therefore
// opens with its own two states.
#define A2P_GUARD "s_nop 1\n\t"
// d (VGPRs) = a * b + c: first MFMA of a score block, c = -m_ref (VGPRs: C and D share one half of the register file)
__device__ __forceinline__ void a2p_mfma_first(f32x16& d, const op16x8& a, const op16x8& b, const f32x16& c) {
    asm volatile(A2P_GUARD A2P_MFMA_OP " %0, %1, %2, %3" : "=&v"(d) : "a"(a), "a"(b), "v"(c));
}
// d (VGPRs) = a * b (C = inline constant 0)
__device__ __forceinline__ void a2p_mfma_first0(f32x16& d, const op16x8& a, const op16x8& b) {
    asm volatile(A2P_GUARD A2P_MFMA_OP " %0, %1, %2, 0" : "=&v"(d) : "a"(a), "a"(b));
}
// d (VGPRs) += a * b
__device__ __forceinline__ void a2p_mfma_s(f32x16& d, const op16x8& a, const op16x8& b) {
    asm volatile(A2P_GUARD A2P_MFMA_OP " %0, %1, %2, %0" : "+v"(d) : "a"(a), "a"(b));
}
// d (AGPRs) += a * b, b = P (VGPRs)
__device__ __forceinline__ void a2p_mfma_o(f32x16& d, const op16x8& a, const op16x8& b) {
    asm volatile(A2P_GUARD A2P_MFMA_OP " %0, %1, %2, %0" : "+a"(d) : "a"(a), "v"(b));
}
// a wave-uniform pointer the compiler can see is uniform (SGPR pair): global_load_lds then uses the "SGPR base + 32-bit VGPR offset" form
__device__ __forceinline__ const char* attn_uniform_ptr(const void* ptr) {
    const uint64_t u = reinterpret_cast<uint64_t>(ptr);
    const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)u), hi = __builtin_amdgcn_readfirstlane((uint32_t)(u >> 32));
    return reinterpret_cast<const char*>(((uint64_t)hi << 32) | lo);
}

// One half-step.  s_cur: the scores of this 32-key block (both query blocks); s_nxt: the scores of the next block, taken from key
// block KBN of the K tile in ring stage ST_K; p_prev: P of the previous block = key block KBP of the tile whose V^T sits in stage
// ST_V; nvalid (MASK instantiations = last tile only): keys of THIS block that exist (>= 32: all).  pk / pv: LDS addresses of this
// lane's K / V^T fragments inside stage 0 (loop invariant; stage, key / d block are immediates).
// LDS fragment load in asm, straight into the accumulator file, with the wait counted by hand (the compiler's own lgkmcnt waits for
// its ds_reads were lgkmcnt(0) in front of the first MFMA that used one: a full LDS round trip, ~100 cycles, exposed twice per
// half-step; tools/probes/inwave_overlap.hip modes 11 / 13).  The destination is only valid after a2p_lds_wait.
__device__ __forceinline__ uint32_t a2p_lds_addr(const void* p) {
    return (uint32_t)reinterpret_cast<uintptr_t>((const __attribute__((address_space(3))) void*)p);
}
template <int BYTES>
__device__ __forceinline__ void a2p_lds_read(op16x8& dst, uint32_t addr) {
    static_assert(BYTES >= 0 && BYTES < 65536, "ds_read offset field");
    asm volatile("ds_read_b128 %0, %1 offset:%2" : "=a"(dst) : "v"(addr), "n"(BYTES));
}
__device__ __forceinline__ void a2p_lds_wait(op16x8 (&f)[8]) {
    asm volatile("s_waitcnt lgkmcnt(0)" : "+a"(f[0]), "+a"(f[1]), "+a"(f[2]), "+a"(f[3]), "+a"(f[4]), "+a"(f[5]), "+a"(f[6]), "+a"(f[7]));
}
// the eight fragments of a half-step: K steps 0..3 of key block KBN of the K tile in ring stage ST_K, then V^T pieces (16-key step
// 2 KBP + (g >> 1), d block g & 1), g = 0..3, of the V^T tile in stage ST_V.  ak / av: this lane's LDS byte addresses inside stage 0.
template <int F, int ST_K, int KBN, int ST_V, int KBP>
__device__ __forceinline__ void a2p_load_frag(op16x8& dst, const uint32_t (&ak)[4], const uint32_t (&av)[4]) {
    if (F < 4) a2p_lds_read<(ST_K * ATTN2P_TILE + KBN * 2048) * 2>(dst, ak[F]);
    else a2p_lds_read<((4 + ST_V) * ATTN2P_TILE + ((F - 4) & 1) * 2048) * 2>(dst, av[2 * KBP + ((F - 4) >> 1)]);
}

// One half-step.  s_cur: the scores of this 32-key block (both query blocks); s_nxt: the scores of the next block; fr: the eight
// LDS fragments of THIS half-step (requested during the previous one, complete on entry); fn: those of the NEXT half-step, whose
// parameters are N_* -- requested in the first eight half-slots, waited for at the end; p_prev: P of the previous block;
// nvalid: keys of THIS block that exist (>= 32: all).
template <int N_ST_K, int N_KBN, int N_ST_V, int N_KBP>
__device__ __forceinline__ void attn2p_half(const uint32_t (&ak)[4], const uint32_t (&av)[4], const op16x8 (&qf)[2][4], op16x8 (&fr)[8],
                                            op16x8 (&fn)[8], f32x16 (&s_cur)[2], f32x16 (&s_nxt)[2], f32x16 (&o)[2][2], f32x16 (&mneg)[2],
                                            const uint32_t (&p_prev)[2][8], uint32_t (&p_cur)[2][8], float (&l_run)[2], int hi,
                                            int nvalid) {
    if (__builtin_expect(nvalid < 32, 0)) {                  // wave-uniform; only the last tile of a sequence can be partial
#pragma unroll
        for (int qb = 0; qb < 2; ++qb)
#pragma unroll
            for (int r = 0; r < 16; ++r)
                if (16 * hi + r >= nvalid) s_cur[qb][r] = -INFINITY;
    }
    float sa[2] = {0.0f, 0.0f}, sb[2] = {0.0f, 0.0f};        // two partial row sums per query block (even / odd key of a pair)
    float y0 = 0.0f, y1 = 0.0f;                              // exponentials of the previous pair (summed / packed one half-slot later)
#define A2P_HALF_SLOT(H)                                                                                                \
    {                                                                                                                   \
        constexpr int h = (H), f = h >> 1, qb = h & 1;                                                                  \
        if (h < 8) a2p_load_frag<(h < 8 ? h : 0), N_ST_K, N_KBN, N_ST_V, N_KBP>(fn[h < 8 ? h : 0], ak, av);               \
        {                                                                                                               \
            constexpr int pq = h >> 3, pi = h & 7;           /* pair (query block, i): scores 2i, 2i + 1 of s_cur[.] */ \
            float x0 = __builtin_amdgcn_exp2f(s_cur[pq][2 * pi]);                                                       \
            float x1 = __builtin_amdgcn_exp2f(s_cur[pq][2 * pi + 1]);                                                   \
            asm volatile("" : "+v"(x0), "+v"(x1));                                                                      \
            if (h > 0) {                                                                                                \
                constexpr int qq = (h > 0 ? h - 1 : 0) >> 3, w = (h > 0 ? h - 1 : 0) & 7;                               \
                sa[qq] += y0;                                                                                           \
                sb[qq] += y1;                                                                                           \
                p_cur[qq][w] = f5_pack2_bounded(y0, y1);                                                                \
                asm volatile("" : "+v"(sa[qq]), "+v"(sb[qq]), "+v"(p_cur[qq][w]));                                      \
            }                                                                                                           \
            y0 = x0;                                                                                                    \
            y1 = x1;                                                                                                    \
        }                                                                                                               \
        if (f < 4) {                                                                                                    \
            if (f == 0) a2p_mfma_first(s_nxt[qb], fr[f], qf[qb][f < 4 ? f : 0], mneg[qb]);                              \
            else a2p_mfma_s(s_nxt[qb], fr[f], qf[qb][f < 4 ? f : 0]);                                                   \
        } else {                                                                                                        \
            constexpr int sp = (f - 4) >> 1 & 1, db = (f - 4) & 1;                                                      \
            const op16x8 pb = __builtin_bit_cast(op16x8, u32x4{p_prev[qb][4 * sp], p_prev[qb][4 * sp + 1], p_prev[qb][4 * sp + 2], \
                                                               p_prev[qb][4 * sp + 3]});                                \
            a2p_mfma_o(o[qb][db], fr[f], pb);                                                                           \
        }                                                                                                               \
        __builtin_amdgcn_sched_barrier(0);                                                                              \
    }
    A2P_HALF_SLOT(0) A2P_HALF_SLOT(1) A2P_HALF_SLOT(2) A2P_HALF_SLOT(3) A2P_HALF_SLOT(4) A2P_HALF_SLOT(5) A2P_HALF_SLOT(6) A2P_HALF_SLOT(7)
    A2P_HALF_SLOT(8) A2P_HALF_SLOT(9) A2P_HALF_SLOT(10) A2P_HALF_SLOT(11) A2P_HALF_SLOT(12) A2P_HALF_SLOT(13) A2P_HALF_SLOT(14) A2P_HALF_SLOT(15)
#undef A2P_HALF_SLOT
    sa[1] += y0;
    sb[1] += y1;
    p_cur[1][7] = f5_pack2_bounded(y0, y1);
    a2p_lds_wait(fn);                                        // requested eight or more half-slots ago
    float psum[2] = {sa[0] + sb[0], sa[1] + sb[1]};
    if (__builtin_expect(__any(!(psum[0] <= ATTN_SUM_LIMIT) || !(psum[1] <= ATTN_SUM_LIMIT)) != 0, 0)) {
        // wave-uniform and rare: some score of this block lies more than 14 (exp2 units) above the reference point.  Move the
        // reference point of every row to max(old, this block's maximum): O and l shrink by alpha, -m_ref and the scores of the next
        // block (already computed against the old point) shift by delta, the block's P is taken again.
        asm volatile(A2P_PAD : "+a"(o[0][0]), "+a"(o[0][1]), "+a"(o[1][0]), "+a"(o[1][1]));     // the last MFMAs of the half-step wrote O
        asm volatile("" : "+v"(s_nxt[0]), "+v"(s_nxt[1]));                                       // ... issued after the S MFMAs: covered
#pragma unroll
        for (int qb = 0; qb < 2; ++qb) {
            float tmax = 0.0f;
#pragma unroll
            for (int r = 0; r < 16; ++r) tmax = fmaxf(tmax, s_cur[qb][r]);
            const float delta = fmaxf(tmax, __shfl_xor(tmax, 32, 64));       // >= 0, in exp2 units
            const float alpha = __builtin_amdgcn_exp2f(-delta);
            l_run[qb] *= alpha;
            float s0 = 0.0f, s1 = 0.0f;
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                o[qb][0][e] *= alpha;
                o[qb][1][e] *= alpha;
                mneg[qb][e] -= delta;
                s_nxt[qb][e] -= delta;
            }
#pragma unroll
            for (int w = 0; w < 8; ++w) {
                const float e0 = __builtin_amdgcn_exp2f(s_cur[qb][2 * w] - delta);
                const float e1 = __builtin_amdgcn_exp2f(s_cur[qb][2 * w + 1] - delta);
                s0 += e0;
                s1 += e1;
                p_cur[qb][w] = f5_pack2_bounded(e0, e1);
            }
            psum[qb] = s0 + s1;
        }
        // the rewritten accumulators / -m_ref are MFMA operands of the next half-step: a VALU result needs 2 states
        asm volatile("s_nop 1" : "+a"(o[0][0]), "+a"(o[0][1]), "+a"(o[1][0]), "+a"(o[1][1]), "+v"(mneg[0]), "+v"(mneg[1]));
    }
    l_run[0] += psum[0];
    l_run[1] += psum[1];
}

__global__ __launch_bounds__(256, 1) void f5_attn2p_kernel(F5AttnArgs p) {
    constexpr int TILE = 64 * 64;
    __shared__ __attribute__((aligned(16))) op16_t smem[8 * TILE];       // K ring [4][64*64] then V^T ring [4][64*64]: 64 KB

    attn_pin_args<false>(p);
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int hi = lane >> 5, lq = lane & 31;
    int bh, qblk;
    if (!attn_block_map(p, 256, bh, qblk)) return;
    const int b = bh / p.H, h = bh - b * p.H;
    const int q0 = qblk * 256 + wave * 64;
    const int kvlen = p.kv_len ? p.kv_len[b] : p.seq_len;
    const int T = (kvlen + 63) >> 6;
    const size_t rowbase = (size_t)b * p.seq_len;
    const bool live = q0 < p.seq_len;                       // a wave entirely past the sequence only stages tiles and keeps the barriers

    op16x8 qf[2][4];
    attn_load_q<2, 1>(qf, p, rowbase, q0, lq, h, hi);
    // staging: 2 16-byte chunks of K and of V^T per thread per tile (thread q_ = i * 256 + tid fills LDS chunk q_ of the tile image);
    // source = wave-uniform tile base (SGPR pair) + a loop-invariant 32-bit lane offset
    const char* kbase = attn_uniform_ptr(p.qk[0] + rowbase * p.ldqk + p.dmodel + h * 64);     // key 0 of this head
    const char* vbase = attn_uniform_ptr(p.vt[0] + (size_t)bh * 64 * p.npad);                  // key 0, d 0
    const uint32_t kstep = (uint32_t)(64 * p.ldqk) * 2u;                                      // bytes per tile
    uint32_t koff[2], voff[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int q_ = i * 256 + tid;
        const int srow = q_ >> 3;
        const int schunk = (q_ & 7) ^ ((srow >> 1) & 7);
        koff[i] = ((uint32_t)attn_kperm(srow) * (uint32_t)p.ldqk + schunk * 8) * 2u;
        voff[i] = ((uint32_t)srow * (uint32_t)p.npad + schunk * 8) * 2u;
    }
    const int ldsw = wave * 64 * 8;                          // this wave's 1 KB piece of a 4 KB staging instruction (elements)
#define A2P_ISSUE_K(t_)                          /* K tile t_ -> K ring stage t_ & 3 */                   \
    {                                                                                                        \
        op16_t* dst_ = smem + ((t_) & 3) * TILE + ldsw;                                                      \
        const char* ks_ = kbase + (size_t)(t_) * kstep;                                                      \
        const bool tail_ = ((t_) * 64 + 63) > p.seq_len - 1;                                                 \
        _Pragma("unroll") for (int i = 0; i < 2; ++i) {                                                      \
            uint32_t ko_ = koff[i];                                                                          \
            if (tail_) {                                     /* rows past the sequence: re-read its last key */ \
                const int q_ = i * 256 + tid, srow_ = q_ >> 3;                                               \
                int key_ = (t_) * 64 + attn_kperm(srow_);                                                    \
                if (key_ > p.seq_len - 1) key_ = p.seq_len - 1;                                              \
                ko_ = ((uint32_t)(key_ - (t_) * 64) * (uint32_t)p.ldqk + ((q_ & 7) ^ ((srow_ >> 1) & 7)) * 8) * 2u; \
            }                                                                                                \
            attn_glds16(reinterpret_cast<const op16_t*>(ks_ + ko_), dst_ + i * 2048);                        \
        }                                                                                                    \
    }
#define A2P_ISSUE_V(t_)                          /* V^T tile t_ -> V ring stage t_ & 3 */                 \
    {                                                                                                        \
        op16_t* dst_ = smem + (4 + ((t_) & 3)) * TILE + ldsw;                                                \
        const char* vs_ = vbase + (size_t)(t_) * 128;                                                        \
        _Pragma("unroll") for (int i = 0; i < 2; ++i)                                                        \
            attn_glds16(reinterpret_cast<const op16_t*>(vs_ + voff[i]), dst_ + i * 2048);                    \
    }
    // issue group of iteration j (after its barrier): K(j+3) and V^T(j+2); the wait at the top of iteration j lets the group of
    // iteration j-1 -- K(j+2), V^T(j+1), 2 instructions each where the tile exists -- stay in flight
#define A2P_ISSUE_GROUP(j_)                                  \
    {                                                        \
        if ((j_) + 3 < T) A2P_ISSUE_K((j_) + 3);             \
        if ((j_) + 2 < T) A2P_ISSUE_V((j_) + 2);             \
    }
#define A2P_WAIT_TOP(j_)                                     \
    if ((j_) + 2 < T) {                                      \
        asm volatile("s_waitcnt vmcnt(4)" ::: "memory");     \
    } else if ((j_) + 1 < T) {                               \
        asm volatile("s_waitcnt vmcnt(2)" ::: "memory");     \
    } else {                                                 \
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");     \
    }
    // this lane's fragment addresses (LDS bytes) inside a 64 x 64 tile image of stage 0: lane part of attn_swz; the key / d block adds 32 rows
    uint32_t ak[4], av[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        ak[i] = a2p_lds_addr(smem + lq * 64 + (((i * 2 + hi) ^ ((lq >> 1) & 7)) << 3));                       // QK^T k-step i: chunk 2 i + hi
        av[i] = a2p_lds_addr(smem + lq * 64 + (((4 * (i >> 1) + 2 * hi + (i & 1)) ^ ((lq >> 1) & 7)) << 3));  // 16-key step i of the tile
    }

    // ---- prologue: K(0), V^T(0), K(1), then the group "of iteration -1": K(2), V^T(1).  P(-1, 1) = 0 multiplies the V^T stage of
    // "tile -1" (stage 3) in the first half-step: that stage is zeroed here (uninitialised LDS may hold NaN patterns).
    A2P_ISSUE_K(0);
    A2P_ISSUE_V(0);
    if (T > 1) A2P_ISSUE_K(1);
    if (T > 2) A2P_ISSUE_K(2);
    if (T > 1) A2P_ISSUE_V(1);
    {
        const u32x4 z4 = {0u, 0u, 0u, 0u};
        *reinterpret_cast<u32x4*>(smem + 7 * TILE + tid * 8) = z4;
        *reinterpret_cast<u32x4*>(smem + 7 * TILE + 2048 + tid * 8) = z4;
    }
    // Q^T fragments: waited for here (a use the compiler sees, as ATTN_PIN_Q) and from here on accumulator-file values -- every
    // MFMA takes them as "a" operands; defined as VGPR values they would be copied (4 v_accvgpr_write) in front of every use
#pragma unroll
    for (int qb = 0; qb < 2; ++qb)
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) asm volatile("" : "+a"(qf[qb][ks]));
    // K(0) has landed (the oldest 2 of the 4 + 2 [T > 1] + 4 [T > 2: 2, else V^T(1) only] requests)
    if (T > 2) {
        asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
    } else if (T > 1) {
        asm volatile("s_waitcnt vmcnt(6)" ::: "memory");
    } else {
        asm volatile("s_waitcnt vmcnt(2)" ::: "memory");
    }
    attn_barrier();
    if (!live) {                                             // same barriers, same staging, no arithmetic
        for (int j = 0; j < T; ++j) {
            A2P_WAIT_TOP(j);
            attn_barrier();
            A2P_ISSUE_GROUP(j);
        }
        return;
    }

    f32x16 o[2][2], mneg[2], s_a[2], s_b[2];                 // s_a / p_a: key block 0 of a tile, s_b / p_b: key block 1
    uint32_t p_a[2][8], p_b[2][8];
    op16x8 fr_a[8], fr_b[8];                                 // LDS fragments of the (j, 0) / (j, 1) half-steps: each set is requested during the other's half-step
#pragma unroll
    for (int qb = 0; qb < 2; ++qb) {
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            o[qb][0][e] = 0.0f;
            o[qb][1][e] = 0.0f;
        }
#pragma unroll
        for (int w = 0; w < 8; ++w) p_b[qb][w] = 0u;         // P(-1, 1)
    }
    float l_run[2] = {0.0f, 0.0f};

    // ---- the reference point: the true maximum of S(0, block 0) per row; s_a = S(0, 0) - m_ref enters the loop like every other block
    {
        a2p_load_frag<0, 0, 0, 0, 0>(fr_b[0], ak, av);       // K(0) block 0, steps 0..3 (fr_b is free until half-step (0, 0) requests into it)
        a2p_load_frag<1, 0, 0, 0, 0>(fr_b[1], ak, av);
        a2p_load_frag<2, 0, 0, 0, 0>(fr_b[2], ak, av);
        a2p_load_frag<3, 0, 0, 0, 0>(fr_b[3], ak, av);
        // the fragments of half-step (0, 0): K(0) block 1; V^T(-1) second half = the zeroed stage 3
        a2p_load_frag<0, 0, 1, 3, 1>(fr_a[0], ak, av);
        a2p_load_frag<1, 0, 1, 3, 1>(fr_a[1], ak, av);
        a2p_load_frag<2, 0, 1, 3, 1>(fr_a[2], ak, av);
        a2p_load_frag<3, 0, 1, 3, 1>(fr_a[3], ak, av);
        a2p_load_frag<4, 0, 1, 3, 1>(fr_a[4], ak, av);
        a2p_load_frag<5, 0, 1, 3, 1>(fr_a[5], ak, av);
        a2p_load_frag<6, 0, 1, 3, 1>(fr_a[6], ak, av);
        a2p_load_frag<7, 0, 1, 3, 1>(fr_a[7], ak, av);
        asm volatile("s_waitcnt lgkmcnt(0)" : "+a"(fr_b[0]), "+a"(fr_b[1]), "+a"(fr_b[2]), "+a"(fr_b[3]));
        a2p_lds_wait(fr_a);
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
            if (ks == 0) {
                a2p_mfma_first0(s_a[0], fr_b[ks], qf[0][ks]);
                a2p_mfma_first0(s_a[1], fr_b[ks], qf[1][ks]);
            } else {
                a2p_mfma_s(s_a[0], fr_b[ks], qf[0][ks]);
                a2p_mfma_s(s_a[1], fr_b[ks], qf[1][ks]);
            }
        }
        asm volatile(A2P_PAD : "+v"(s_a[0]), "+v"(s_a[1]));
#pragma unroll
        for (int qb = 0; qb < 2; ++qb) {
            float tmax = -INFINITY;
#pragma unroll
            for (int r = 0; r < 16; ++r) tmax = fmaxf(tmax, (16 * hi + r < kvlen) ? s_a[qb][r] : -INFINITY);
            const float m0 = fmaxf(tmax, __shfl_xor(tmax, 32, 64));
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                mneg[qb][e] = -m0;
                s_a[qb][e] -= m0;
            }
        }
        asm volatile("s_nop 1" : "+v"(mneg[0]), "+v"(mneg[1]));
    }

    // ---- tiles.  Tile j = 4 g + PH (PH compile-time: four tiles per loop trip, a tile past the end is skipped by a scalar branch):
    //   TOP:    K(j+1) and V^T(j) have landed (counted wait), barrier, issue K(j+3) and V^T(j+2)
    //   (j, 0): exp of S(j, 0) in s_a -> p_a;  S(j, 1) -> s_b from K stage PH;            O += V^T(j-1, 1) p_b, V stage PH - 1
    //   (j, 1): exp of S(j, 1) in s_b -> p_b;  S(j+1, 0) -> s_a from K stage PH + 1;      O += V^T(j, 0) p_a,   V stage PH
    // Every tile runs the same code: keys past kvlen (last tile only) are masked under a wave-uniform branch, and the last tile's
    // second half-step computes an S(T, 0) nobody reads (K stage PH + 1 then holds an older tile or nothing: finite or not, unused).
    // After the loop: O += V^T(T-1, 1) p_b.
#define A2P_STEP(PH)                                                                                                    \
    if (j < T) {                                                                                                        \
        A2P_WAIT_TOP(j)                                                                                                 \
        attn_barrier();                                                                                                 \
        A2P_ISSUE_GROUP(j)                                                                                              \
        const int nv_ = kvlen - j * 64;                                                                                 \
        /* (j, 0) requests the fragments of (j, 1): K(j+1) block 0, V^T(j) first half; (j, 1) those of (j+1, 0): K(j+1) block 1, V^T(j) second half */ \
        attn2p_half<((PH) + 1) & 3, 0, (PH), 0>(ak, av, qf, fr_a, fr_b, s_a, s_b, o, mneg, p_b, p_a, l_run, hi, nv_);       \
        attn2p_half<((PH) + 1) & 3, 1, (PH), 1>(ak, av, qf, fr_b, fr_a, s_b, s_a, o, mneg, p_a, p_b, l_run, hi, nv_ - 32);  \
        ++j;                                                                                                            \
    }
    {
        int j = 0;
        for (int g = (T + 3) >> 2; g > 0; --g) {
            A2P_STEP(0)
            A2P_STEP(1)
            A2P_STEP(2)
            A2P_STEP(3)
        }
    }
#undef A2P_STEP
    // O^T += V^T(T-1, 1) P(T-1, 1): the V ring stage of the last tile is a run-time value here (added to the lane address)
    {
        const uint32_t stv = (uint32_t)((T - 1) & 3) * (ATTN2P_TILE * 2);
        uint32_t avf[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) avf[i] = av[i] + stv;
        a2p_load_frag<4, 0, 0, 0, 1>(fr_a[0], ak, avf);      // stage "0" + the run-time offset, second half of the tile (KBP = 1), pieces 0..3
        a2p_load_frag<5, 0, 0, 0, 1>(fr_a[1], ak, avf);
        a2p_load_frag<6, 0, 0, 0, 1>(fr_a[2], ak, avf);
        a2p_load_frag<7, 0, 0, 0, 1>(fr_a[3], ak, avf);
        asm volatile("s_waitcnt lgkmcnt(0)" : "+a"(fr_a[0]), "+a"(fr_a[1]), "+a"(fr_a[2]), "+a"(fr_a[3]));
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const int sp = g >> 1, db = g & 1;
#pragma unroll
            for (int qb = 0; qb < 2; ++qb) {
                const op16x8 pb = __builtin_bit_cast(op16x8, u32x4{p_b[qb][4 * sp], p_b[qb][4 * sp + 1], p_b[qb][4 * sp + 2], p_b[qb][4 * sp + 3]});
                a2p_mfma_o(o[qb][db], fr_a[g], pb);
            }
        }
    }
#undef A2P_WAIT_TOP
#undef A2P_ISSUE_GROUP
#undef A2P_ISSUE_V
#undef A2P_ISSUE_K
    asm volatile(A2P_PAD : "+a"(o[0][0]), "+a"(o[0][1]), "+a"(o[1][0]), "+a"(o[1][1]));

#pragma unroll
    for (int qb = 0; qb < 2; ++qb) attn_store_block<false>(p, o[qb], l_run[qb], rowbase, q0 + qb * 32 + lq, h, hi);
}

// =================================================================================================
// v2s: v2 with the KV range split across KS wave groups INSIDE the workgroup (small batches: B*H*ceil(N/128)
// workgroups of 4 waves leave the 256 CUs with one wave per SIMD and the whole kernel is one workgroup's latency
// chain over all KV tiles).  Group g (4 waves, the same 128 queries as the other groups) walks tiles g, g+KS, ...
// with its own LDS ring; barriers are shared, so every group runs ceil(ntile/KS) iterations.  At the end the groups
// park (m, l, O^T) in LDS (the rings are dead by then) and merge them flash-decoding style:
// m = max m_g, l = sum l_g 2^((m_g-m)c), O = sum O_g 2^((m_g-m)c) — the same numbers as one pass up to fp32 rounding.
// Every group merges and stores its 1 / KS of the head dimension (the fp8 output: group 0 merges all of it).
// =================================================================================================
template <bool HP, int KS, int NST, bool FAST = false>
__global__ __launch_bounds__(256 * KS, 1) void f5_attn2s_kernel(F5AttnArgs p) {
    constexpr int NP = HP ? 2 : 1;
    constexpr int TILE = 64 * 64;
    constexpr int RING = NST * NP * 2 * TILE;           // elements per group ring
    static_assert(KS * RING * 2 <= 160 * 1024, "LDS budget");
    static_assert((KS - 1) * 4 * 34 * 64 * 4 <= KS * RING * 2, "merge area must fit in the rings");
    __shared__ __attribute__((aligned(16))) op16_t smem_all[KS * RING];

    attn_pin_args<true>(p);
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave_all = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int grp = wave_all >> 2, wave = wave_all & 3;
    const int tg = tid & 255;
    op16_t* smem = smem_all + grp * RING;
    const int hi = lane >> 5, lq = lane & 31;
    int bh, qblk;
    if (!attn_block_map(p, 128, bh, qblk)) return;
    const int b = bh / p.H, h = bh - b * p.H;
    const int q0 = qblk * 128 + wave * 32;
    const int kvlen = p.kv_len ? p.kv_len[b] : p.seq_len;
    const int ntile = (kvlen + 63) >> 6;
    const int nit = (ntile + KS - 1) / KS;              // iterations of group 0 (the most)
    const int ntg = ntile > grp ? (ntile - grp + KS - 1) / KS : 0;   // tiles of this group
    const size_t rowbase = (size_t)b * p.seq_len;

    op16x8 qf[NP][4];
    {
        int qr = q0 + lq;
        if (qr > p.seq_len - 1) qr = p.seq_len - 1;
#pragma unroll
        for (int pp = 0; pp < NP; ++pp)
#pragma unroll
            for (int ks = 0; ks < 4; ++ks)
                qf[pp][ks] = *reinterpret_cast<const op16x8*>(p.qk[pp] + (rowbase + qr) * p.ldqk + h * 64 + ks * 16 + hi * 8);
    }

    const op16_t* kptr[NP][2];
    const op16_t* vptr[NP][2];
    int krow[2], kcol[2], ldsoff[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int q_ = i * 256 + tg;
        const int srow = q_ >> 3;
        const int schunk = (q_ & 7) ^ ((srow >> 1) & 7);
        krow[i] = attn_kperm(srow);
        kcol[i] = p.dmodel + h * 64 + schunk * 8;
        ldsoff[i] = (i * 256 + wave * 64) * 8;
#pragma unroll
        for (int pp = 0; pp < NP; ++pp) {
            kptr[pp][i] = p.qk[pp] + (rowbase + grp * 64 + krow[i]) * p.ldqk + kcol[i];
            vptr[pp][i] = p.vt[pp] + ((size_t)bh * 64 + srow) * p.npad + grp * 64 + schunk * 8;
        }
    }
    const size_t kstep = (size_t)64 * KS * p.ldqk;
    // jj_ = group-local tile number; the global tile is jj_*KS + grp
#define A2S_ISSUE(jj_)                                                                                       \
    {                                                                                                        \
        op16_t* st_ = smem + ((jj_) % NST) * (NP * 2 * TILE);                                                \
        const int gt_ = (jj_) * KS + grp;                                                                    \
        const bool tail_ = (gt_ * 64 + 63) > p.seq_len - 1;                                                  \
        _Pragma("unroll") for (int i = 0; i < 2; ++i) {                                                      \
            _Pragma("unroll") for (int pp = 0; pp < NP; ++pp) {                                              \
                const op16_t* ks_ = kptr[pp][i];                                                             \
                if (tail_) {                                                                                 \
                    int key_ = gt_ * 64 + krow[i];                                                           \
                    if (key_ > p.seq_len - 1) key_ = p.seq_len - 1;                                          \
                    ks_ = p.qk[pp] + (rowbase + key_) * p.ldqk + kcol[i];                                    \
                }                                                                                            \
                attn_glds16(ks_, st_ + (pp * 2) * TILE + ldsoff[i]);                                         \
                attn_glds16(vptr[pp][i], st_ + (pp * 2 + 1) * TILE + ldsoff[i]);                             \
                kptr[pp][i] += kstep;                                                                        \
                vptr[pp][i] += 64 * KS;                                                                      \
            }                                                                                                \
        }                                                                                                    \
    }

    f32x16 o[2];
#pragma unroll
    for (int e = 0; e < 16; ++e) {
        o[0][e] = 0.0f;
        o[1][e] = 0.0f;
    }
    float m_run = -INFINITY, l_run = 0.0f;
    const float c2 = p.q_prescaled ? 1.0f : p.scale * 1.4426950408889634f;

    if (ntg > 0) A2S_ISSUE(0);
    if (NST == 3 && ntg > 1) A2S_ISSUE(1);
    ATTN_PIN_Q(qf, NP, 4);

    for (int jj = 0; jj < nit; ++jj) {
        // wait for tile jj (own loads), then make every wave's part visible; tile jj+1 may stay in flight (NST == 3)
        attn_wait_barrier(NST == 3 && jj + 1 < ntg);
        if (jj + NST - 1 < ntg) A2S_ISSUE(jj + NST - 1);   // slot consumed in iteration jj-1: every wave is past it
        if (jj >= ntg) continue;                          // wave-uniform: this group has no tile left (still meets the barrier)

        const op16_t* st = smem + (jj % NST) * (NP * 2 * TILE);
        const op16_t* sK = st;
        const op16_t* sV = st + TILE;
        const op16_t* sKl = st + (NP - 1) * 2 * TILE;
        const op16_t* sVl = st + (NP - 1) * 2 * TILE + TILE;

        f32x16 s[2];
        const int key0 = (jj * KS + grp) * 64;
        // scores of the tile (raw units) with the key-padding tail masked
#define A2S_QK()                                                                                             \
        {                                                                                                    \
            __builtin_amdgcn_s_setprio(1);                                                                   \
            _Pragma("unroll") for (int kb = 0; kb < 2; ++kb) {                                               \
                _Pragma("unroll") for (int e = 0; e < 16; ++e) s[kb][e] = 0.0f;                              \
                _Pragma("unroll") for (int ks = 0; ks < 4; ++ks) {                                           \
                    const int off = attn_swz(kb * 32 + lq, ks * 2 + hi);                                     \
                    const op16x8 a = *reinterpret_cast<const op16x8*>(&sK[off]);                             \
                    s[kb] = F5_MFMA32(a, qf[0][ks], s[kb], 0, 0, 0);                                         \
                    if (HP) {                                                                                \
                        const op16x8 al = *reinterpret_cast<const op16x8*>(&sKl[off]);                       \
                        s[kb] = F5_MFMA32(al, qf[0][ks], s[kb], 0, 0, 0);                                    \
                        s[kb] = F5_MFMA32(a, qf[NP - 1][ks], s[kb], 0, 0, 0);                                \
                    }                                                                                        \
                }                                                                                            \
            }                                                                                                \
            __builtin_amdgcn_s_setprio(0);                                                                   \
            if (key0 + 64 > kvlen) {                                                                         \
                _Pragma("unroll") for (int kb = 0; kb < 2; ++kb)                                             \
                    _Pragma("unroll") for (int r = 0; r < 16; ++r) {                                         \
                        const int key = key0 + kb * 32 + 16 * hi + r;                                        \
                        if (key >= kvlen) s[kb][r] = -INFINITY;                                              \
                    }                                                                                        \
            }                                                                                                \
        }
        A2S_QK();
        // FAST (see f5_attn2f_kernel): after a group's first tile the exponentials are taken against the standing reference point
        // m_run without looking for the tile maximum -- at this grid size the kernel is one workgroup's latency chain, and
        // max -> cross-lane exchange (an LDS round trip) -> rescale test sits in front of every tile's exponentials.  The row
        // sums tell whether that was safe (every p <= 2^14); if not, the tile is redone the slow way.
        float psum = 0.0f;
        bool slow = !FAST || HP || jj == 0;
        if (!slow) {
            const float mc = m_run * c2;
            attn_f32x2 ps2 = {0.0f, 0.0f};
            ps2 = attn_exp_block(s[0], c2, mc, ps2);
            ps2 = attn_exp_block(s[1], c2, mc, ps2);
            psum = ps2[0] + ps2[1];
            slow = __any(!(psum <= ATTN_SUM_LIMIT));
            if (slow) A2S_QK();
        }
        if (slow) {
            float tmax = -INFINITY;
#pragma unroll
            for (int kb = 0; kb < 2; ++kb)
#pragma unroll
                for (int r = 0; r < 16; ++r) tmax = fmaxf(tmax, s[kb][r]);
            tmax = fmaxf(tmax, __shfl_xor(tmax, 32, 64));
            if (__any(tmax > m_run)) {                    // wave-uniform: rescale only when some lane's running max moved
                const float m_new = fmaxf(m_run, tmax);
                const float alpha = __builtin_amdgcn_exp2f((m_run - m_new) * c2);
                m_run = m_new;
                l_run *= alpha;
#pragma unroll
                for (int e = 0; e < 16; ++e) {
                    o[0][e] *= alpha;
                    o[1][e] *= alpha;
                }
            }
            const float mc = m_run * c2;
            attn_f32x2 ps2 = {0.0f, 0.0f};
            ps2 = attn_exp_block(s[0], c2, mc, ps2);
            ps2 = attn_exp_block(s[1], c2, mc, ps2);
            psum = ps2[0] + ps2[1];
        }
        l_run += psum;
#undef A2S_QK

#pragma unroll
        for (int ks4 = 0; ks4 < 4; ++ks4) {
            const int kb = ks4 >> 1, sp = ks4 & 1;
            uint32_t pw[4], pwl[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float p0 = s[kb][8 * sp + 2 * e], p1 = s[kb][8 * sp + 2 * e + 1];
                pw[e] = f5_pack2_bounded(p0, p1);
                if (HP) pwl[e] = f5_pack2_lo(p0, p1);
            }
            const op16x8 pb = __builtin_bit_cast(op16x8, u32x4{pw[0], pw[1], pw[2], pw[3]});
            op16x8 pbl = pb;
            if (HP) pbl = __builtin_bit_cast(op16x8, u32x4{pwl[0], pwl[1], pwl[2], pwl[3]});
            __builtin_amdgcn_s_setprio(1);
#pragma unroll
            for (int db = 0; db < 2; ++db) {
                const int voff = attn_swz(db * 32 + lq, 4 * kb + 2 * hi + sp);
                const op16x8 a = *reinterpret_cast<const op16x8*>(&sV[voff]);
                o[db] = F5_MFMA32(a, pb, o[db], 0, 0, 0);
                if (HP) {
                    const op16x8 al = *reinterpret_cast<const op16x8*>(&sVl[voff]);
                    o[db] = F5_MFMA32(al, pb, o[db], 0, 0, 0);
                    o[db] = F5_MFMA32(a, pbl, o[db], 0, 0, 0);
                }
            }
            __builtin_amdgcn_s_setprio(0);
        }
    }
#undef A2S_ISSUE

    // ---- merge the KS partial states (same lane of the same wave index in every group holds the same elements)
    __syncthreads();                                     // every ring is dead
    float* mrg = reinterpret_cast<float*>(smem_all);     // [KS-1][4 waves][34][64 lanes]
    if (HP || !p.out8) {
        // Every group finishes its share of O^T: group g owns the Q = 32 / KS accumulator elements [g Q, (g + 1) Q) of (db, e) -- head-dim
        // block db == g for two groups, a quarter each for four.  It parks (m, l) and the elements it does not own, reads its partners'
        // parts of the ones it does, and merges them with the expressions and in the group order of the one-group merge below: per wave
        // 1 / KS of the exponent-weighted sums and of the output.  The one-pass kernels then hand the packed 16-bit rows over through
        // LDS, so that a head's row (128 bytes, one line) leaves as eight 16-byte stores instead of one 8-byte store per lane and line.
        constexpr int Q = 32 / KS, NPK = 2 + 32 - Q;     // floats a lane parks: m, l, the elements of the other groups
        constexpr int SLD = 64 + 8;                      // staging row (16-bit elements): 128 queries x 64, padded
        static_assert(KS * 4 * NPK * 64 * 4 + (HP ? 0 : 128 * SLD * 2) <= KS * RING * 2, "merge area + output staging fit in the rings");
        float* mine = mrg + (size_t)((grp * 4 + wave) * NPK) * 64 + lane;
        mine[0] = m_run;
        mine[64] = l_run;
#pragma unroll
        for (int g = 0; g < KS; ++g)                     // (unrolled, grp is wave-uniform: one scalar branch, constant register indices)
            if (grp == g) {
#pragma unroll
                for (int i = 0; i < 32; ++i)
                    if (i / Q != g) mine[(2 + (i < g * Q ? i : i - Q)) * 64] = o[i >> 4][i & 15];
            }
        __syncthreads();
        const float* src[KS];
        float mg[KS];
#pragma unroll
        for (int g = 0; g < KS; ++g) {
            src[g] = mrg + (size_t)((g * 4 + wave) * NPK) * 64 + lane;
            mg[g] = src[g][0];
        }
        float m_all = mg[0];
#pragma unroll
        for (int g = 1; g < KS; ++g) m_all = fmaxf(m_all, mg[g]);
        float ag[KS];
#pragma unroll
        for (int g = 0; g < KS; ++g) ag[g] = __builtin_amdgcn_exp2f((mg[g] - m_all) * c2);    // empty group: m = -inf -> 0
        // The roundings are spelled out (explicit fma, nothing left to contract): of "l_0 a_0 + l_1 a_1" the compiler may fuse either product
        // into the addition, and for l it rounds l_1 a_1 and fuses l_0 a_0 in the one-group merge below (all six instantiations).  The
        // bits are pinned by tests/test_split_tail_gpu.py.
        float l_all = __builtin_fmaf(src[0][64], ag[0], src[1][64] * ag[1]);
#pragma unroll
        for (int g = 2; g < KS; ++g) l_all = __builtin_fmaf(src[g][64], ag[g], l_all);
        float own[Q];
#pragma unroll
        for (int g = 0; g < KS; ++g)
            if (grp == g) {
#pragma unroll
                for (int j = 0; j < Q; ++j) {
                    const int i = g * Q + j;
                    // every element gets its own copy of the weights: the SLP vectoriser pairs the elements up, and a weight it knows to be
                    // common to a pair may be broadcast out of the HI half of a register pair -- the packed-f32 form that must not run
                    // next to MFMAs (build.sh, tests/test_isa.py)
                    float w[KS];
#pragma unroll
                    for (int k = 0; k < KS; ++k) {
                        w[k] = ag[k];
                        asm volatile("" : "+v"(w[k]));
                    }
                    float x[KS];                         // the element's partial sums in group order (group 0 parks i >= Q at slot i - Q)
#pragma unroll
                    for (int k = 0; k < KS; ++k) x[k] = k == g ? o[i >> 4][i & 15] : src[k][(2 + (i < k * Q ? i : i - Q)) * 64];
                    // (which product is rounded and which is fused, as the one-group merge is compiled -- see l_all: with two groups the
                    // compiler rounds o_1 a_1 and fuses o_0 a_0, with four it rounds o_0 a_0 and fuses the others one after the other)
                    float acc;
                    if (KS == 2) {
                        acc = __builtin_fmaf(x[0], w[0], x[1] * w[1]);
                    } else {
                        acc = x[0] * w[0];
#pragma unroll
                        for (int k = 1; k < KS; ++k) acc = __builtin_fmaf(x[k], w[k], acc);
                    }
                    own[j] = acc;
                }
            }
        const float l_tot = l_all + __shfl_xor(l_all, 32, 64);
        const float inv = 1.0f / l_tot;
        const int qr = q0 + lq;
        op16_t* stg = reinterpret_cast<op16_t*>(mrg + KS * 4 * NPK * 64);
#pragma unroll
        for (int j = 0; j < Q; j += 4) {
            const int i = grp * Q + j;                   // (db, rg) of these four elements
            const int d = (i >> 4) * 32 + 8 * ((i & 15) >> 2) + 4 * hi;
            const float v0 = own[j] * inv, v1 = own[j + 1] * inv, v2 = own[j + 2] * inv, v3 = own[j + 3] * inv;
            const u32x2 pk = {f5_pack2_bounded(v0, v1), f5_pack2_bounded(v2, v3)};
            if (HP) {
                if (qr < p.seq_len) {
                    const size_t off = (rowbase + qr) * p.ldo + h * 64 + d;
                    *reinterpret_cast<u32x2*>(p.out[0] + off) = pk;
                    if (p.out[1]) *reinterpret_cast<u32x2*>(p.out[1] + off) = u32x2{f5_pack2_lo(v0, v1), f5_pack2_lo(v2, v3)};
                }
            } else {
                *reinterpret_cast<u32x2*>(&stg[(wave * 32 + lq) * SLD + d]) = pk;
            }
        }
        if (HP) return;
        __syncthreads();                                 // the last barrier; a row's blocks come from different groups
#pragma unroll
        for (int c = tid; c < 128 * 8; c += 256 * KS) {
            const int row = c >> 3, ch = c & 7;
            const int qrow = qblk * 128 + row;
            if (qrow < p.seq_len)
                *reinterpret_cast<u32x4*>(p.out[0] + (rowbase + qrow) * p.ldo + h * 64 + ch * 8) = *reinterpret_cast<const u32x4*>(&stg[row * SLD + ch * 8]);
        }
        return;
    }
    // fp8 output (attn_store_f8 wants whole rows in one wave): groups 1.. park everything, group 0 merges and stores
    if (grp > 0) {
        float* dst = mrg + (size_t)((grp - 1) * 4 + wave) * 34 * 64 + lane;
        dst[0] = m_run;
        dst[64] = l_run;
#pragma unroll
        for (int db = 0; db < 2; ++db)
#pragma unroll
            for (int e = 0; e < 16; ++e) dst[(2 + db * 16 + e) * 64] = o[db][e];
    }
    __syncthreads();
    if (grp > 0) return;
    float m_all = m_run;
#pragma unroll
    for (int g = 1; g < KS; ++g) m_all = fmaxf(m_all, mrg[(size_t)((g - 1) * 4 + wave) * 34 * 64 + lane]);
    {
        const float a0 = __builtin_amdgcn_exp2f((m_run - m_all) * c2);
        l_run *= a0;
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            o[0][e] *= a0;
            o[1][e] *= a0;
        }
    }
#pragma unroll
    for (int g = 1; g < KS; ++g) {
        const float* src = mrg + (size_t)((g - 1) * 4 + wave) * 34 * 64 + lane;
        const float ag = __builtin_amdgcn_exp2f((src[0] - m_all) * c2);    // empty group: m = -inf -> 0
        l_run += src[64] * ag;
#pragma unroll
        for (int db = 0; db < 2; ++db)
#pragma unroll
            for (int e = 0; e < 16; ++e) o[db][e] += src[(2 + db * 16 + e) * 64] * ag;
    }

    const float l_tot = l_run + __shfl_xor(l_run, 32, 64);
    const float inv = 1.0f / l_tot;
    const int qr = q0 + lq;
    if (!HP && p.out8) {
        if (qr < p.seq_len) attn_store_f8(p, o, inv, rowbase + qr, h, hi);
    } else if (qr < p.seq_len) {
#pragma unroll
        for (int db = 0; db < 2; ++db)
#pragma unroll
            for (int rg = 0; rg < 4; ++rg) {
                const int d = db * 32 + 8 * rg + 4 * hi;
                const float v0 = o[db][rg * 4 + 0] * inv, v1 = o[db][rg * 4 + 1] * inv;
                const float v2 = o[db][rg * 4 + 2] * inv, v3 = o[db][rg * 4 + 3] * inv;
                const size_t off = (rowbase + qr) * p.ldo + h * 64 + d;
                *reinterpret_cast<u32x2*>(p.out[0] + off) = u32x2{f5_pack2_bounded(v0, v1), f5_pack2_bounded(v2, v3)};
                if (HP && p.out[1])
                    *reinterpret_cast<u32x2*>(p.out[1] + off) = u32x2{f5_pack2_lo(v0, v1), f5_pack2_lo(v2, v3)};
            }
    }
}

// test hooks that choose among the SHIPPED kernels (the shape heuristics below decide otherwise)
int f5_attn_wide = -1;     // -1 auto (>= 512 workgroups of 256 queries), 0 off, 1 force: 256-query workgroups, two query blocks per wave
int f5_attn_kvsplit = -1;  // -1 auto, 1 / 2 / 4 = force the in-workgroup KV split
int f5_attn_pipe = 0;      // process default of F5AttnArgs::pipe (-1): 1 = in-wave software-pipelined v2p (one wave per SIMD), 0 = v2f

// 1-D XCD-aware grid (attn_block_map)
static dim3 attn_grid(const F5AttnArgs& a, int qrows) {
    const int nqb = f5_cdiv(a.seq_len, qrows);
    return dim3(nqb * 8 * f5_cdiv(a.B * a.H, 8), 1);
}

// the kernel a legal launch goes to under the knobs above (bf16x3 only has the 128-query kernels)
static F5AttnKernel attn_route(const F5AttnArgs& a) {
    // small batches: fewer workgroups than ~2 per CU -> split the KV range over 2 or 4 wave groups inside the workgroup
    int ks = f5_attn_kvsplit;
    if (ks < 0) {
        const long wgs = (long)f5_cdiv(a.seq_len, 128) * a.B * a.H;
        const int ntile = f5_cdiv(a.seq_len, 64);
        // measured (tools/attn_split_bench.py, N = 937, 16 heads): 128 WGs 20.5 / 17.4 / 16.2 us for 1 / 2 / 4 groups,
        // 256 WGs 21.4 / 19.1 / 20.1, 512 WGs 31.8 / 37.3 / 38.9
        ks = (wgs <= 160 && ntile >= 8) ? 4 : ((wgs <= 320 && ntile >= 4) ? 2 : 1);
    }
    // large grids (one-pass modes): two query blocks per wave (256 queries per workgroup), no per-tile maximum
    if (!a.hp && ks <= 1 &&
        (f5_attn_wide >= 1 || (f5_attn_wide < 0 && (long)f5_cdiv(a.seq_len, 256) * a.B * a.H >= 512))) {
        // f5_attn_pipe: 1 = the in-wave software-pipelined kernel (v2p, one wave per SIMD), 0 = v2f; q must be pre-multiplied
        const bool pipe = (a.pipe < 0 ? f5_attn_pipe : a.pipe) && a.q_prescaled;
        return pipe ? F5A_V2P : (a.q_prescaled ? F5A_V2F_PRE : F5A_V2F);
    }
    if (ks > 1) return a.hp ? F5A_V2S_HP : (ks >= 4 ? F5A_V2S_KS4 : F5A_V2S_KS2);
    return a.hp ? F5A_V2_HP : F5A_V2;
}

// checks, routes and launches; reached = what f5_debug_last_attn_kernel is to report when this returns 0
static int attn_launch(const F5AttnArgs& a, hipStream_t stream, int& reached) {
    F5_REQUIRE(a.B > 0 && a.H > 0 && a.seq_len > 0, "attention: bad shape");
    F5_REQUIRE(a.npad % 64 == 0 && a.npad >= a.seq_len, "attention: npad must be a multiple of 64 and >= seq_len");
    F5_REQUIRE(a.ldqk % 8 == 0 && a.ldo % 4 == 0, "attention: bad leading dims");
    F5_REQUIRE(a.qk[0] && a.vt[0] && (a.out[0] || a.out8), "attention: null pointer");
    F5_REQUIRE(!a.out8 || (!a.hp && a.out8s && a.ldo8 % 4 == 0),
               "attention: fp8 output needs the bf16 ring kernels");
    F5_REQUIRE(!a.hp || (a.qk[1] && a.vt[1] && a.out[1]), "attention: bf16x3 needs lo buffers");
    const F5AttnKernel k = attn_route(a);
    const dim3 grid = attn_grid(a, 128), gw = attn_grid(a, 256);
    switch (k) {
        case F5A_V2_HP: hipLaunchKernelGGL(f5_attn2_kernel<true>, grid, dim3(256), 0, stream, a); break;
        case F5A_V2: hipLaunchKernelGGL(f5_attn2_kernel<false>, grid, dim3(256), 0, stream, a); break;
        case F5A_V2F_PRE: hipLaunchKernelGGL(f5_attn2f_kernel<true>, gw, dim3(256), 0, stream, a); break;
        case F5A_V2F: hipLaunchKernelGGL(f5_attn2f_kernel<false>, gw, dim3(256), 0, stream, a); break;
        case F5A_V2P: hipLaunchKernelGGL(f5_attn2p_kernel, gw, dim3(256), 0, stream, a); break;
        case F5A_V2S_HP: hipLaunchKernelGGL((f5_attn2s_kernel<true, 2, 2>), grid, dim3(512), 0, stream, a); break;
        case F5A_V2S_KS2: hipLaunchKernelGGL((f5_attn2s_kernel<false, 2, 3, true>), grid, dim3(512), 0, stream, a); break;
        case F5A_V2S_KS4: hipLaunchKernelGGL((f5_attn2s_kernel<false, 4, 2, true>), grid, dim3(1024), 0, stream, a); break;
        default: break;                                   // attn_route returns one of the eight above
    }
    F5_LAUNCH_CHECK();
    reached = k;
    return 0;
}

int f5_launch_attention(const F5AttnArgs& a, hipStream_t stream) {
    int reached = F5A_NONE;
    const int rc = attn_launch(a, stream, reached);
    f5dbg::last_attn_kernel = rc == 0 ? (reached | (a.out8 ? F5A_OUT8 : 0)) : F5A_NONE;    // the one place the hook is written
    return rc;
}
}  // namespace F5_NS
