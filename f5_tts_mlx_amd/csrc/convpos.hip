// ConvPositionEmbedding conv (dit.py:29-50): grouped Conv1d(C, C, k=31, groups=C/64, pad=15) + Mish on
// channels-last (b, n, c) input, as an implicit GEMM per group on v_mfma_f32_32x32x16_bf16:
//   out[n][co] = sum_{tap, ci} x[n + tap - 15][ci] * w[co][tap][ci]      (M = tokens, N = 64, K = taps*64)
// The A operand is a sliding window over ONE LDS-resident halo tile of x ((128 + taps - 1) rows x 64 ci),
// so x is read from HBM once per block; the per-tap weight slab [64 co][64 ci] is double-buffered.
// Sequence edges are zero padded per batch element (Conv1d padding); no mask (dit.py:251 passes none).  With F5ConvPosArgs::lens the
// edge of element b is lens[b] instead of seq_len: the conv of that element alone, whatever the rows behind it hold.
// Two kernels: f5_convpos_kernel (register-staged slabs, small LDS footprint: several workgroups per CU hide each other's round
// trips) and, for single-segment grids of one round, f5_convpos_ring_kernel further down (same arithmetic, slabs by LDS-DMA into a ring).
#include "convpos.hpp"
#include "rowops.hpp"     // f5_sat_flag_host

namespace F5_NS {

#define XLD 72  // LDS row stride (elements) for both tiles: 144 B rows => conflict-free ds_read_b128
#define CP_ROWS 128
#define CP_MAXTAPS 31
// Ablation switches for tools/convpos_bench.py's probe builds (-DCP_ABL=bits); 0 in the library, where every test below is a constant
// that compiles away.  1: no tap loop; 2: tap loop without fragment reads and MFMAs; 4: tap loop without the slab loads and stores;
// 8: epilogue without its stores.  Applies to f5_convpos_kernel and to f5_convpos_ring_kernel alike.
#ifndef CP_ABL
#define CP_ABL 0
#endif

// TPS = taps per pipeline step: the weight slabs of TPS taps are fetched, stored and synchronised together (fewer, fatter
// steps).  Measured no better than TPS = 1 at batch 1 and worse at batch 32, where the 18 KB weight ring of TPS = 1 lets 3-4
// workgroups share a CU (tools/convpos_bench.py); what did help at batch 1 is the block numbering below (25.5 -> 19.8 us).
// LENS: the launch carries row lengths (F5ConvPosArgs::lens).  Without them the instantiation is the kernel as it was, instruction for
// instruction: the batch-1 launches are one round of workgroups and pay for every scalar load in front of their first request.
// CPG: channels per group, 64 or 48.  A 48-channel group sits in a 64-wide tile of its own: the halo tile holds columns g*48 .. g*48+47
// and zeros in the other 16 (never loaded), the weight slabs come zero padded to [64 co][tap][64 ci] from the weight store
// (host_common.hpp f5_pack_conv_groups), the K steps stop at 48 input channels and the epilogue writes 48 columns.  Of the 6 MFMAs per
// tap and wave a quarter multiply the zero rows co = 48..63: the price of a 32-wide MFMA on a 48-wide group.  Every CPG test below is a
// constant: 64 instantiates the kernel as it was.
template <bool HP, int TPS, bool LENS, int CPG>
__global__ __launch_bounds__(256) void f5_convpos_kernel(F5ConvPosArgs p) {
    static_assert(CPG == 64 || CPG == 48, "channels per group: 64, or 48 in a zero-padded 64-wide tile");
    constexpr int NP = HP ? 2 : 1;
    constexpr int HALO = CP_ROWS + CP_MAXTAPS - 1;
    __shared__ __attribute__((aligned(16))) op16_t sX[NP][HALO * XLD];
    __shared__ __attribute__((aligned(16))) op16_t sW[2][TPS][NP][64 * XLD];

    asm volatile("" ::"s"(p.in[0]), "s"(p.W[0]), "s"(p.bias), "s"(p.B), "s"(p.seq_len), "s"(p.groups), "s"(p.taps), "s"(p.ld), "s"(p.mode),
                 "s"(p.out_bf[0]), "s"(p.out_f32), "s"(p.ldo));              // the argument block in one scalar-load clause
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int hi = lane >> 5, lr = lane & 31;
    // workgroup -> (token tile, group, batch element).  Every workgroup of a group streams that group's 31 weight slabs
    // (254 KB); with the plain (x = token tile, y = group, z = batch) numbering the token tiles of a group sit on different
    // XCDs (XCD = linear id & 7) and every XCD's L2 ends up streaming ALL groups' weights.  The 1-D grid used when the group
    // count is a multiple of 8 deals groups to XCDs instead: XCD x hosts groups x, x + 8, ... with all their token tiles and
    // batch elements, so a group's weights are fetched into one L2 and shared by its workgroups.
    // A 3-D grid has one y per group, so with a group count that is a multiple of 8 a single y means the 1-D grid.  The group
    // count is part of the test: one group and one batch element make a 3-D grid (token tiles, 1, 1) that must not be decoded as 1-D.
    int n0, g, b;
    if (gridDim.y == 1 && (p.groups & 7) == 0) {
        const int nx = (p.seq_len + CP_ROWS - 1) / CP_ROWS;
        const int per_group = nx * p.B;
        const int s_ = blockIdx.x >> 3;
        const int gl = s_ / per_group, rem = s_ - gl * per_group;
        g = gl * 8 + (blockIdx.x & 7);
        b = rem / nx;
        n0 = (rem - b * nx) * CP_ROWS;
    } else {
        n0 = blockIdx.x * CP_ROWS;
        g = blockIdx.y;
        b = blockIdx.z;
    }
    const int taps = p.taps;
    const int pad = taps >> 1;
    const int halo = CP_ROWS + taps - 1;
    const size_t rowbase = (size_t)b * p.seq_len;
    const int kdim = taps * 64;
    // row lengths: this element's rows n >= len_b are zeros in the halo tile, never loaded, and are not written.  A workgroup whose whole
    // token tile lies there has nothing to write: it leaves (n0 and b are workgroup-uniform).
    const int len_b = LENS ? min(max(p.lens[b], 0), p.seq_len) : p.seq_len;
    if (LENS && n0 >= len_b) return;

    // ---- stage the x halo tile (zero outside [0, len_b)) ----------------------------------------
    for (int qd = tid; qd < halo * 8; qd += 256) {
        const int r = qd >> 3, c = qd & 7;
        const int n = n0 - pad + r;
        const bool ok = (n >= 0) && (n < len_b) && (CPG == 64 || c < CPG / 8);
#pragma unroll
        for (int pp = 0; pp < NP; ++pp) {
            u32x4 v = {0u, 0u, 0u, 0u};
            if (ok) v = *reinterpret_cast<const u32x4*>(p.in[pp] + (rowbase + n) * p.ld + g * CPG + c * 8);
            *reinterpret_cast<u32x4*>(&sX[pp][r * XLD + c * 8]) = v;
        }
    }

    // ---- weight slab staging: 2 chunks per thread per part per tap ------------------------------
    u32x4 rw[TPS][NP][2];
#define CP_LOADW(t0_)                                                                                   \
    {                                                                                                   \
        _Pragma("unroll") for (int tt_ = 0; tt_ < TPS; ++tt_) {                                         \
            const int tap_ = (t0_) + tt_ < taps ? (t0_) + tt_ : taps - 1;   /* clamped slabs are loaded, never used */ \
            _Pragma("unroll") for (int i = 0; i < 2; ++i) {                                             \
                const int qd_ = tid + 256 * i;                                                          \
                const int r_ = qd_ >> 3, c_ = qd_ & 7;                                                  \
                _Pragma("unroll") for (int pp = 0; pp < NP; ++pp) rw[tt_][pp][i] =                      \
                    *reinterpret_cast<const u32x4*>(p.W[pp] + (size_t)(g * 64 + r_) * kdim + tap_ * 64 + c_ * 8); \
            }                                                                                           \
        }                                                                                               \
    }
#define CP_STOREW(buf_)                                                                                 \
    {                                                                                                   \
        _Pragma("unroll") for (int tt_ = 0; tt_ < TPS; ++tt_)                                           \
            _Pragma("unroll") for (int i = 0; i < 2; ++i) {                                             \
                const int qd_ = tid + 256 * i;                                                          \
                const int r_ = qd_ >> 3, c_ = qd_ & 7;                                                  \
                _Pragma("unroll") for (int pp = 0; pp < NP; ++pp)                                       \
                    *reinterpret_cast<u32x4*>(&sW[buf_][tt_][pp][r_ * XLD + c_ * 8]) = rw[tt_][pp][i];  \
            }                                                                                           \
    }

    f32x16 acc[2];
#pragma unroll
    for (int e = 0; e < 16; ++e) {
        acc[0][e] = 0.0f;
        acc[1][e] = 0.0f;
    }

    if (!(CP_ABL & 4)) {
        CP_LOADW(0);
        CP_STOREW(0);
    }
    __syncthreads();

    // mode 1 accumulates into x.  `out[off] += v` element by element in the epilogue made the compiler keep every
    // read-modify-write in program order (it cannot rule out that one store aliases the next load): 32 dependent memory round
    // trips per lane at the end of the kernel.  The old values are requested HERE, before the tap loop (clamped rows, so the loads
    // are straight-line), and are long there when the epilogue adds and stores.
    float old[2][16];
    if (p.mode != 0) {
#pragma unroll
        for (int nb = 0; nb < 2; ++nb)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                int n = n0 + wave * 32 + (r & 3) + 8 * (r >> 2) + 4 * hi;
                if (n > p.seq_len - 1) n = p.seq_len - 1;
                // (a 48-channel group: the lanes of columns 48..63 load column 47, and never use it)
                if (CPG == 64) old[nb][r] = p.out_f32[(rowbase + n) * p.ldo + g * 64 + nb * 32 + lr];
                else old[nb][r] = p.out_f32[(rowbase + n) * p.ldo + g * CPG + min(nb * 32 + lr, CPG - 1)];
            }
    }

    for (int t0 = 0, step = 0; t0 < ((CP_ABL & 1) ? 0 : taps); t0 += TPS, ++step) {
        const int cur = step & 1;
        if (!(CP_ABL & 4) && t0 + TPS < taps) CP_LOADW(t0 + TPS);
#pragma unroll
        for (int tt = 0; tt < TPS; ++tt) {
            const int t = t0 + tt;
            if (!(CP_ABL & 2) && t < taps) {
#pragma unroll
                for (int ks = 0; ks < CPG / 16; ++ks) {
                    const int aoff = (wave * 32 + lr + t) * XLD + ks * 16 + hi * 8;
                    const op16x8 a = *reinterpret_cast<const op16x8*>(&sX[0][aoff]);
                    op16x8 al = a;
                    if (HP) al = *reinterpret_cast<const op16x8*>(&sX[NP - 1][aoff]);
#pragma unroll
                    for (int nb = 0; nb < 2; ++nb) {
                        const int boff = (nb * 32 + lr) * XLD + ks * 16 + hi * 8;
                        const op16x8 w = *reinterpret_cast<const op16x8*>(&sW[cur][tt][0][boff]);
                        acc[nb] = F5_MFMA32(a, w, acc[nb], 0, 0, 0);
                        if (HP) {
                            const op16x8 wl = *reinterpret_cast<const op16x8*>(&sW[cur][tt][NP - 1][boff]);
                            acc[nb] = F5_MFMA32(al, w, acc[nb], 0, 0, 0);
                            acc[nb] = F5_MFMA32(a, wl, acc[nb], 0, 0, 0);
                        }
                    }
                }
            }
        }
        if (!(CP_ABL & 4) && t0 + TPS < taps) CP_STOREW(cur ^ 1);
        __syncthreads();
    }

    // ---- epilogue: + bias, Mish, store ----------------------------------------------------------
    // the two bias values are requested together and waited for ONCE, outside the per-row conditionals: with the load inside the
    // nb loop the compiler put its `s_waitcnt vmcnt(0)` for it into every conditional row block, where it also waits for all the
    // stores issued so far -- the stores of a lane went out one memory round trip apart
    float bias2[2] = {p.bias[g * CPG + lr], p.bias[CPG == 64 ? g * 64 + 32 + lr : g * CPG + min(32 + lr, CPG - 1)]};
    asm volatile("" : "+v"(bias2[0]), "+v"(bias2[1]));
    f5_sat_t trk;
#pragma unroll
    for (int nb = 0; nb < 2; ++nb) {
        const int co = g * CPG + nb * 32 + lr;
        const float bias = bias2[nb];
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int n = n0 + wave * 32 + (r & 3) + 8 * (r >> 2) + 4 * hi;
            if (n < len_b && (CPG == 64 || nb * 32 + lr < CPG)) {     // a 48-channel group: columns 48..63 of the tile belong to no channel
                const float v = f5_mish(acc[nb][r] + bias);
                const size_t off = (rowbase + n) * p.ldo + co;
                if ((CP_ABL & 8) && p.taps > 0) {
                    asm volatile("" ::"v"(v), "v"(old[nb][r]));           // the arithmetic stays, the stores go
                } else if (p.mode == 0) {
                    op16_t h, l;
                    f5_split(v, h, l, trk);
                    p.out_bf[0][off] = h;
                    if (p.out_bf[1]) p.out_bf[1][off] = l;
                } else {
                    p.out_f32[off] = old[nb][r] + v;
                }
            }
        }
    }
    f5_sat_commit(trk, p.sat_flag);
}

// ================================================================================================================================
// f5_convpos_ring_kernel: the single-segment conv for grids of one round (one workgroup per CU, one wave per SIMD), where nothing
// but the kernel's own pipeline hides a round trip.  Same workgroup -> (token tile, group, element) mapping, same 128-token tile and
// 4 waves, same arithmetic in the same order as f5_convpos_kernel<false, .> (per accumulator: taps ascending, ks = 0..3), so the same
// bits.  What differs is how the operands travel:
//   - the weight slabs go HBM -> LDS by global_load_lds (16 B per lane, no staging VGPRs) into a ring of NST slots of 8 KB; the first
//     NST - 1 slabs are requested in the prologue, and behind every tap's barrier the next one goes into the slot of the tap before.
//     One barrier per tap; the counted `s_waitcnt vmcnt` in front of it leaves NST - 3 slabs in flight;
//   - the halo tile goes the same way, in front of slab 0 (rows outside [0, len_b) are zeros written by ds_write), so the prologue
//     is one burst of requests and not a chain of load -> store -> load;
//   - the fragments of tap t + 1 are read from LDS into a second register set BEFORE the MFMAs of tap t (tools/convpos_bench.py's probe
//     builds: with a read -> wait -> MFMA sequence per K step the tap loop without any slab traffic took 7.7 us against 3.4 us of
//     MFMA time).  The barrier of tap t therefore waits for slab t + 1.
// LDS images.  An LDS-DMA instruction writes lane-linear (wave base + 16 lane), so rows are 128 B without padding and the 16-byte
// chunk c of row r sits at chunk c ^ ((r >> 1) & 7): applied to the SOURCE address when staging and again on every read.
// ds_read_b128 is served in groups of 16 lanes, 256 B over the 64 banks; the lanes of a group read one logical chunk c of 16
// consecutive rows r0 .. r0 + 15 (r0 = wave * 32 + t (+ 16) for the sliding A window, any tap offset t).  Byte address mod 256 =
// 128 (r & 1) + 16 (c ^ ((r >> 1) & 7)): among the 8 rows of either parity r >> 1 runs over 8 consecutive numbers, all residues
// mod 8, so the 16 lanes hit 16 different 16-byte bank groups whatever r0 is: no conflict for any t.
// vmcnt is counted per wave in issue order.  Order of issue: halo, slab 0, the 2 bias loads and mode 1's 32 `old` loads, slabs
// 1 .. NST-2, then one slab per tap.  A wait for "slabs below u" may leave 2 (issued - u) instructions out when the slabs issued so
// far are all the ring can hold ("steady": the counts are then compile-time constants), plus bias and `old` while u == 1; otherwise
// the wave drains (short tap counts, the tail).
// Ordering.  A slab is read one barrier after the wait that retired it; a slot is refilled behind the barrier of tap t with the slab of
// tap t + NST - 1, and was last read (tap t - 1's fragments) before the barrier of tap t - 1, where lgkmcnt(0) retired the reads.
// Measured at (C 1024, N 937, 2 elements), op level: ring depth 4 / 8 / 12 and 1 / 2 / 4 taps per barrier within each other's scatter,
// mode 0's rows staged through LDS into 16-byte stores no faster than the 2-byte stores (profiles/r08): 8 slots, 1 tap, direct stores.
// ================================================================================================================================
#ifndef CP_RING_NST
#define CP_RING_NST 8
#endif
#define CPR_XROWS 160                     // halo rows staged (158 used at 31 taps): 5 LDS-DMA pieces of 8 rows per wave
#define CPR_SLAB (64 * 64)                // elements per weight slab image

__device__ __forceinline__ void cp_glds16(const op16_t* gptr, op16_t* lds_wave_base) {
    __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(gptr),
                                     (__attribute__((address_space(3))) void*)(lds_wave_base), 16, 0, 0);
}
__device__ __forceinline__ int cp_swz(int row, int chunk) { return row * 64 + ((chunk ^ ((row >> 1) & 7)) << 3); }
// workgroup barrier the compiler moves no memory access across; this wave's LDS accesses are complete when it arrives
__device__ __forceinline__ void cp_barrier() {
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
}
template <int N>
__device__ __forceinline__ void cp_vmcnt() {
    static_assert(N >= 0 && N < 64, "vmcnt is a 6-bit field");
    asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
}

constexpr size_t cp_ring_lds_bytes(int nst) { return (size_t)(CPR_XROWS * 64 + nst * CPR_SLAB) * sizeof(op16_t); }

template <int NST, bool LENS>
__global__ __launch_bounds__(256) void f5_convpos_ring_kernel(F5ConvPosArgs p) {
    static_assert(NST >= 3 && 2 * (NST - 2) + 34 < 64, "ring depth: two slabs in use, vmcnt range");
    extern __shared__ __attribute__((aligned(16))) op16_t cp_smem[];
    op16_t* const sX = cp_smem;
    op16_t* const sW = cp_smem + CPR_XROWS * 64;

    asm volatile("" ::"s"(p.in[0]), "s"(p.W[0]), "s"(p.bias), "s"(p.B), "s"(p.seq_len), "s"(p.groups), "s"(p.taps), "s"(p.ld), "s"(p.mode),
                 "s"(p.out_bf[0]), "s"(p.out_f32), "s"(p.ldo));              // the argument block in one scalar-load clause
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int hi = lane >> 5, lr = lane & 31;
    int n0, g, b;                          // f5_convpos_kernel's mapping, 1-D group-per-XCD numbering included
    if (gridDim.y == 1 && (p.groups & 7) == 0) {
        const int nx = (p.seq_len + CP_ROWS - 1) / CP_ROWS;
        const int per_group = nx * p.B;
        const int s_ = blockIdx.x >> 3;
        const int gl = s_ / per_group, rem = s_ - gl * per_group;
        g = gl * 8 + (blockIdx.x & 7);
        b = rem / nx;
        n0 = (rem - b * nx) * CP_ROWS;
    } else {
        n0 = blockIdx.x * CP_ROWS;
        g = blockIdx.y;
        b = blockIdx.z;
    }
    const int taps = p.taps;
    const int pad = taps >> 1;
    const int halo = CP_ROWS + taps - 1;
    const size_t rowbase = (size_t)b * p.seq_len;
    const int kdim = taps * 64;
    // row lengths as in f5_convpos_kernel; the workgroup-uniform exit lies in front of the first LDS-DMA issue and of every barrier
    const int len_b = LENS ? min(max(p.lens[b], 0), p.seq_len) : p.seq_len;
    if (LENS && n0 >= len_b) return;

    // ---- halo tile: in-range rows by LDS-DMA (the lanes of the other rows are masked off and write zeros themselves) ----------
#pragma unroll
    for (int j = 0; j < CPR_XROWS * 8 / 256; ++j) {
        const int qd = j * 256 + tid;
        const int r = qd >> 3, c = qd & 7;
        const int n = n0 - pad + r;
        if (r < halo && n >= 0 && n < len_b)
            cp_glds16(p.in[0] + (rowbase + n) * p.ld + g * 64 + ((c ^ ((r >> 1) & 7)) << 3), sX + (j * 256 + wave * 64) * 8);
        else
            *reinterpret_cast<u32x4*>(&sX[qd * 8]) = u32x4{0u, 0u, 0u, 0u};
    }

    // ---- weight slabs: 2 pieces per wave per tap, source chunk swizzled, advanced by one tap per issue ------------------------
    const op16_t* wptr[2];
    int wlds[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int qd = i * 256 + tid;
        const int r = qd >> 3, c = qd & 7;
        wptr[i] = p.W[0] + (size_t)(g * 64 + r) * kdim + ((c ^ ((r >> 1) & 7)) << 3);
        wlds[i] = (i * 256 + wave * 64) * 8;
    }
    int issued = 0, islot = 0;
#define CPR_ISSUE()                                                   \
    if (!(CP_ABL & 4) && issued < taps) {                             \
        op16_t* st_ = sW + islot * CPR_SLAB;                          \
        cp_glds16(wptr[0], st_ + wlds[0]);                            \
        cp_glds16(wptr[1], st_ + wlds[1]);                            \
        wptr[0] += 64;                                                \
        wptr[1] += 64;                                                \
        islot = islot + 1 == NST ? 0 : islot + 1;                     \
        ++issued;                                                     \
    }
    CPR_ISSUE();
    asm volatile("" ::: "memory");

    // bias, and for mode 1 the old values, requested before the tap loop as in f5_convpos_kernel (clamped rows, straight-line loads)
    float bias2[2] = {p.bias[g * 64 + lr], p.bias[g * 64 + 32 + lr]};
    float old[2][16];
    if (p.mode != 0) {
#pragma unroll
        for (int nb = 0; nb < 2; ++nb)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                int n = n0 + wave * 32 + (r & 3) + 8 * (r >> 2) + 4 * hi;
                if (n > p.seq_len - 1) n = p.seq_len - 1;
                old[nb][r] = p.out_f32[(rowbase + n) * p.ldo + g * 64 + nb * 32 + lr];
            }
    }
    asm volatile("" ::: "memory");
#pragma unroll
    for (int i = 1; i < NST - 1; ++i) CPR_ISSUE();

    f32x16 acc[2];
#pragma unroll
    for (int e = 0; e < 16; ++e) {
        acc[0][e] = 0.0f;
        acc[1][e] = 0.0f;
    }

    // halo and slab 0 have landed (this wave's pieces); the barrier makes every wave's visible
    if (issued == NST - 1) {
        if (p.mode != 0) cp_vmcnt<2 * (NST - 2) + 34>();
        else cp_vmcnt<2 * (NST - 2) + 2>();
    } else {
        cp_vmcnt<0>();
    }
    cp_barrier();

    op16x8 fa[2][4], fw[2][8];             // fragments of two taps: [set][ks] and [set][ks * 2 + nb]
#define CPR_READ(set_, t_)                                                                                             \
    {                                                                                                                  \
        const op16_t* sw_ = sW + ((t_) % NST) * CPR_SLAB;                                                              \
        _Pragma("unroll") for (int ks = 0; ks < 4; ++ks) {                                                             \
            fa[set_][ks] = *reinterpret_cast<const op16x8*>(&sX[cp_swz(wave * 32 + lr + (t_), ks * 2 + hi)]);          \
            _Pragma("unroll") for (int nb = 0; nb < 2; ++nb)                                                           \
                fw[set_][ks * 2 + nb] = *reinterpret_cast<const op16x8*>(&sw_[cp_swz(nb * 32 + lr, ks * 2 + hi)]);     \
        }                                                                                                              \
    }
    // tap t_: slab t_ + 1 has landed and is made visible, the slot of tap t_ - 1 takes the next slab, tap t_ + 1's fragments are
    // requested (NEXT_), then the MFMAs of tap t_ run on the set read one tap earlier.  No condition around the reads or the MFMAs:
    // with `if (t + 1 < taps)` around either the compiler waited lgkmcnt(0) in front of the MFMAs and carried the accumulators
    // through VGPRs from one iteration to the next
#define CPR_TAP(cur_, t_, NEXT_)                                                                                       \
    {                                                                                                                  \
        if (issued - ((t_) + 2) == NST - 3) cp_vmcnt<2 * (NST - 3)>();                                                 \
        else cp_vmcnt<0>();                                                                                            \
        cp_barrier();                                                                                                  \
        CPR_ISSUE();                                                                                                   \
        if (!(CP_ABL & 2)) {                                                                                           \
            if (NEXT_) CPR_READ((cur_) ^ 1, (t_) + 1);                                                                 \
            _Pragma("unroll") for (int ks = 0; ks < 4; ++ks)                                                           \
                _Pragma("unroll") for (int nb = 0; nb < 2; ++nb)                                                       \
                    acc[nb] = F5_MFMA32(fa[cur_][ks], fw[cur_][ks * 2 + nb], acc[nb], 0, 0, 0);                        \
        }                                                                                                              \
    }
    // the tap count is odd: pairs of taps, then the last one on set 0
    if (!(CP_ABL & 1)) {
        if (!(CP_ABL & 2)) CPR_READ(0, 0);
        int t = 0;
        for (; t + 1 < taps; t += 2) {
            CPR_TAP(0, t, true);
            CPR_TAP(1, t + 1, true);
        }
        CPR_TAP(0, t, false);
    }

    // ---- epilogue: + bias, Mish, store (f5_convpos_kernel's, value for value) ------------------------------------------------
    asm volatile("" : "+v"(bias2[0]), "+v"(bias2[1]));
    f5_sat_t trk;
#pragma unroll
    for (int nb = 0; nb < 2; ++nb) {
        const int co = g * 64 + nb * 32 + lr;
        const float bias = bias2[nb];
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int n = n0 + wave * 32 + (r & 3) + 8 * (r >> 2) + 4 * hi;
            if (n < len_b) {
                const float v = f5_mish(acc[nb][r] + bias);
                const size_t off = (rowbase + n) * p.ldo + co;
                if ((CP_ABL & 8) && p.taps > 0) {
                    asm volatile("" ::"v"(v), "v"(old[nb][r]));
                } else if (p.mode == 0) {
                    op16_t h, l;
                    f5_split(v, h, l, trk);
                    p.out_bf[0][off] = h;
                    if (p.out_bf[1]) p.out_bf[1][off] = l;
                } else {
                    p.out_f32[off] = old[nb][r] + v;
                }
            }
        }
    }
    f5_sat_commit(trk, p.sat_flag);
}

// the ring kernel's LDS (84 KB at 8 slots) is beyond the 64 KB a kernel gets without asking: asked once per device and instantiation
template <bool LENS>
static int cp_launch_ring(const F5ConvPosArgs& ab, dim3 grid, hipStream_t stream) {
    constexpr size_t lds = cp_ring_lds_bytes(CP_RING_NST);
    static bool asked[64] = {};
    int dev = 0;
    F5_REQUIRE(hipGetDevice(&dev) == hipSuccess && dev >= 0 && dev < 64, "convpos: no current device");
    if (!asked[dev]) {
        F5_REQUIRE(hipFuncSetAttribute(reinterpret_cast<const void*>(&f5_convpos_ring_kernel<CP_RING_NST, LENS>),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) == hipSuccess,
                   "convpos: %zu bytes of LDS refused", lds);
        asked[dev] = true;
    }
    hipLaunchKernelGGL((f5_convpos_ring_kernel<CP_RING_NST, LENS>), grid, dim3(256), lds, stream, ab);
    return 0;
}

int f5_convpos_tps = 0;   // taps per pipeline step: 0 auto, 1 / 2 / 4 forced, 8: the ring kernel (f5_debug_set_convpos_tps)
int f5_convpos_xcd_map = 1;   // 0: plain 3-D block numbering (A/B)
// grids up to this many workgroups count as "one round" for the automatic route to the ring kernel (256 CUs, one workgroup each)
#ifndef CP_RING_MAX_WG
#define CP_RING_MAX_WG 256
#endif

// The kernel a launch of this shape runs under the current selectors (F5ConvPosKernel, F5CP_XCD included): the one place that
// decides, used by the launcher and by the f5_debug_convpos_route hook.
//   ring kernel, automatic: single segment, groups dealt to XCDs (a multiple of 8 of them, numbering on), seq_len >= 512 and a grid
//   of one round.  Below 512 tokens or beyond one round several workgroups share a CU, and f5_convpos_kernel<false,1>'s 36 KB of LDS
//   lets 3-4 of them hide each other's round trips (batch 32: 304 us), which the ring kernel's 84 KB does not.
//   selector 8 forces it for every single-segment launch; with three segments 8 acts like 2 and 4: f5_convpos_kernel<true,2>.
// Narrow groups (cpg = 32 or 48 channels per group) never take the ring kernel, which is built for 64-channel groups only: selector 8
// acts like 1 there.  `groups` is the launch's own count: at 32 channels the grid runs groups / 2 super groups (f5_launch_convpos).
int f5_convpos_route(int B, int seq_len, int groups, int nseg, int cpg) {
    if (cpg == 32) groups /= 2;
    const bool narrow = cpg != 64;
    const long nwg = (long)f5_cdiv(seq_len, CP_ROWS) * groups * B;
    const bool xcd = groups % 8 == 0 && f5_convpos_xcd_map;
    const int tps = f5_convpos_tps;
    int k;
    if (nseg == 3) k = tps > 1 ? F5CP_HP2 : F5CP_HP1;
    else if (!narrow && (tps == 8 || (tps == 0 && xcd && seq_len >= 512 && nwg <= CP_RING_MAX_WG))) k = F5CP_RING;
    else if (tps >= 4 && tps != 8) k = F5CP_4;
    else if (tps == 8) k = F5CP_1;
    else if (tps >= 2) k = F5CP_2;
    else k = F5CP_1;       // measured (tools/convpos_bench.py): 1 tap per step beats 2 and 4 at every size (batch 32: 304 / 355 / 629 us)
    return k | (xcd ? F5CP_XCD : 0) | (cpg == 48 ? F5CP_N48 : 0);
}

int f5_launch_convpos(const F5ConvPosArgs& a, hipStream_t stream) {
    f5dbg::last_convpos_kernel = F5CP_NONE;                // a launch that is refused, or fails, reports no kernel
    F5_REQUIRE(a.B > 0 && a.seq_len > 0 && a.groups > 0, "convpos: bad shape");
    // channels per group: 64; 48 (own instantiation); 32 as block-diagonal 64-wide super groups of two (the weights come packed that way
    // from the weight store, so the launch is the 64-channel one on half the groups)
    const int cpg = a.C % a.groups == 0 ? a.C / a.groups : 0;
    F5_REQUIRE(cpg == 64 || cpg == 48 || (cpg == 32 && a.groups % 2 == 0),
               "convpos: channels per group must be 32 (an even number of groups), 48 or 64 (C=%d groups=%d)", a.C, a.groups);
    const int groups = cpg == 32 ? a.groups / 2 : a.groups;
    F5_REQUIRE(a.taps >= 1 && a.taps <= CP_MAXTAPS && (a.taps & 1), "convpos: taps must be odd and <= %d", CP_MAXTAPS);
    F5_REQUIRE(a.ld % 8 == 0, "convpos: ld must be a multiple of 8");
    dim3 grid(f5_cdiv(a.seq_len, CP_ROWS), groups, a.B);
    const long nwg = (long)grid.x * grid.y * grid.z;
    const int reached = f5_convpos_route(a.B, a.seq_len, a.groups, a.nseg, cpg);
    if (reached & F5CP_XCD) grid = dim3((unsigned)nwg, 1, 1);   // group-per-XCD numbering (see the kernel)
    F5ConvPosArgs ab = a;
    ab.groups = groups;
    if (ab.sat_flag == nullptr) ab.sat_flag = f5_sat_flag_host;
    // every kernel in two instantiations: with row lengths (a.lens) and as it was
#define CP_LAUNCH_W(HP_, TPS_, CPG_)                                                                                      \
    {                                                                                                                     \
        if (ab.lens) hipLaunchKernelGGL((f5_convpos_kernel<HP_, TPS_, true, CPG_>), grid, dim3(256), 0, stream, ab);      \
        else hipLaunchKernelGGL((f5_convpos_kernel<HP_, TPS_, false, CPG_>), grid, dim3(256), 0, stream, ab);             \
    }
#define CP_LAUNCH(HP_, TPS_)                                                                                              \
    {                                                                                                                     \
        if (cpg == 48) CP_LAUNCH_W(HP_, TPS_, 48)                                                                         \
        else CP_LAUNCH_W(HP_, TPS_, 64)                                                                                   \
    }
    switch (reached & (F5CP_XCD - 1)) {
    case F5CP_HP1:
    case F5CP_HP2:
        F5_REQUIRE(a.in[1] && a.W[1], "convpos: bf16x3 needs lo operands");
        // the three-pass kernel is built for 1 and 2 taps per step only: a selector of 4 or 8 runs <true, 2>
        if ((reached & (F5CP_XCD - 1)) == F5CP_HP2) CP_LAUNCH(true, 2)
        else CP_LAUNCH(true, 1)
        break;
    case F5CP_RING:
        if (const int rc = ab.lens ? cp_launch_ring<true>(ab, grid, stream) : cp_launch_ring<false>(ab, grid, stream)) return rc;
        break;
    case F5CP_4: CP_LAUNCH(false, 4) break;
    case F5CP_2: CP_LAUNCH(false, 2) break;
    default: CP_LAUNCH(false, 1) break;
    }
#undef CP_LAUNCH
#undef CP_LAUNCH_W
    F5_LAUNCH_CHECK();
    f5dbg::last_convpos_kernel = reached;
    return 0;
}
}  // namespace F5_NS
