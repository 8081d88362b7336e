// probe: how wide is the alignment of v_mfma_scale_f32_32x32x64_f8f6f4?  The 64 products of one output element are exact (4-bit x 4-bit
// significands, power-of-two scales); the instruction aligns them to a common exponent before it adds them.  This program measures, on one
// output element, how far below the largest term a smaller one still counts, whether what falls below is truncated or rounded, whether the
// terms are cut one by one or after their sum, and whether the accumulator input C takes part in the alignment.  It measures the
// instruction, not the GEMM kernel (tests/mxfp8_matrix.py derives its bound from the figures; its docstring quotes them).
//   hipcc --offload-arch=gfx950 -O2 tools/probes/mxalign.hip -o tools/probes/bin/mxalign && tools/probes/bin/mxalign
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
typedef int i32x8 __attribute__((ext_vector_type(8)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

// a / b: the 64 e4m3 bytes of row 0 / column 0 in K order (every row and column gets the same); s*: E8M0 of MX block 0 / 1
__global__ void k(const uint8_t* a, const uint8_t* b, int sa0, int sa1, int sb0, int sb1, float c0, float* out) {
    const int l = threadIdx.x, h = l >> 5;
    i32x8 av, bv;
    for (int w = 0; w < 8; ++w) {
        uint32_t x = 0, y = 0;
        for (int q = 0; q < 4; ++q) {
            const int j = 4 * w + q;
            const int kk = 32 * (j / 16) + 16 * h + j % 16;      // tools/probes/mxscale.hip: the K index of a lane's byte j
            x |= (uint32_t)a[kk] << (8 * q);
            y |= (uint32_t)b[kk] << (8 * q);
        }
        av[w] = (int)x;
        bv[w] = (int)y;
    }
    const int sa = l < 32 ? sa0 : sa1, sb = l < 32 ? sb0 : sb1;
    f32x16 c;
    for (int i = 0; i < 16; ++i) c[i] = c0;
    c = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(av, bv, c, 0, 0, 0, sa, 0, sb);
    out[l] = c[0];                                               // every lane stores: the whole wave must reach the MFMA with its operands set
}

static uint8_t enc(double v) {             // exactly representable e4m3 values only
    uint8_t s = 0;
    if (v < 0) { s = 0x80; v = -v; }
    if (v == 0) return s;
    int e;
    const double m = frexp(v, &e);         // v = m 2^e, m in [0.5, 1)
    e -= 1;                                // v = (2m) 2^e
    if (e < -6) return s | (uint8_t)lrint(v * 512.0);
    return s | (uint8_t)(((e + 7) << 3) | (int)lrint((2 * m - 1) * 8));
}

static uint8_t *da, *db;
static float* dout;
static float run(const double* a, const double* b, int sa0, int sa1, int sb0, int sb1, float c0) {
    uint8_t ha[64], hb[64];
    for (int i = 0; i < 64; ++i) { ha[i] = enc(a[i]); hb[i] = enc(b[i]); }
    hipMemcpy(da, ha, 64, hipMemcpyHostToDevice);
    hipMemcpy(db, hb, 64, hipMemcpyHostToDevice);
    hipLaunchKernelGGL(k, dim3(1), dim3(64), 0, 0, da, db, sa0, sa1, sb0, sb1, c0, dout);
    float r;
    hipMemcpy(&r, dout, 4, hipMemcpyDeviceToHost);
    return r;
}
// 2^x as a product of two e4m3 powers of two, x in [-18, 16]
static void split(int x, double* pa, double* pb) {
    int i = x / 2, j = x - i;
    if (i < -9) { j += i + 9; i = -9; }
    if (j < -9) { i += j + 9; j = -9; }
    if (i > 8) { j += i - 8; i = 8; }
    if (j > 8) { i += j - 8; j = 8; }
    *pa = ldexp(1.0, i);
    *pb = ldexp(1.0, j);
}

int main() {
    hipMalloc(&da, 64);
    hipMalloc(&db, 64);
    hipMalloc(&dout, 64 * 4);
    double a[64], b[64];
    printf("excess = (result - largest term) / smaller term; 1 = kept, 0 = lost (s = log2 of largest / smaller)\n");
    printf("%3s %12s %12s %12s %12s %12s %12s %12s %12s\n", "s", "same block", "other block", "63 small", "1.5 x small", "-1.5 x small",
           "-1 x small", "C + small", "small C");
    for (int s = 1; s <= 25; ++s) {
        double r[8];
        // (1) largest term 2^8 and one smaller term 2^(8 - s) in the same MX block
        memset(a, 0, sizeof(a));
        memset(b, 0, sizeof(b));
        a[0] = 16; b[0] = 16;
        split(8 - s, &a[1], &b[1]);
        r[0] = ((double)run(a, b, 127, 127, 127, 127, 0.f) - 256.0) / ldexp(1.0, 8 - s);
        // (2) the smaller term in the other MX block, made small by that block's scale
        memset(a, 0, sizeof(a));
        memset(b, 0, sizeof(b));
        a[0] = 1; b[0] = 1; a[32] = 1; b[32] = 1;
        r[1] = ((double)run(a, b, 127, 127 - s, 127, 127, 0.f) - 1.0) / ldexp(1.0, -s);
        // (3) 63 smaller terms next to the largest: cut one by one (excess 0 beyond the width) or after their sum (63 until 6 bits later)?
        for (int i = 0; i < 64; ++i) { a[i] = 1; b[i] = 1; }
        for (int i = 1; i < 64; ++i) split(-s, &a[i], &b[i]);
        a[0] = 1; b[0] = 1;
        r[2] = s <= 18 ? ((double)run(a, b, 127, 127, 127, 127, 0.f) - 1.0) / ldexp(1.0, -s) : NAN;
        // (4, 5, 6) 1.5 x, -1.5 x and -1 x the smaller term: truncation or rounding, toward zero or toward minus infinity
        for (int q = 0; q < 3; ++q) {
            memset(a, 0, sizeof(a));
            memset(b, 0, sizeof(b));
            a[0] = 16; b[0] = 16;
            split(8 - s, &a[1], &b[1]);
            a[1] *= q == 0 ? 1.5 : (q == 1 ? -1.5 : -1.0);
            r[3 + q] = ((double)run(a, b, 127, 127, 127, 127, 0.f) - 256.0) / ldexp(1.0, 8 - s);
        }
        // (7) the accumulator input is the largest term: C = 256, one product 2^(8 - s)
        memset(a, 0, sizeof(a));
        memset(b, 0, sizeof(b));
        split(8 - s, &a[1], &b[1]);
        r[6] = ((double)run(a, b, 127, 127, 127, 127, 256.f) - 256.0) / ldexp(1.0, 8 - s);
        // (8) the accumulator input is the smaller term: C = 2^(8 - s), one product 256
        memset(a, 0, sizeof(a));
        memset(b, 0, sizeof(b));
        a[0] = 16; b[0] = 16;
        r[7] = ((double)run(a, b, 127, 127, 127, 127, (float)ldexp(1.0, 8 - s)) - 256.0) / ldexp(1.0, 8 - s);
        printf("%3d %12.4f %12.4f %12.4f %12.4f %12.4f %12.4f %12.4f %12.4f\n", s, r[0], r[1], r[2], r[3], r[4], r[5], r[6], r[7]);
    }
    // (9) which K positions share the alignment of position 0?  largest term at k = 0, one term 2^-16 of it at k: lost = same group
    printf("positions whose 2^-16 term is lost next to the largest term at k = 0:");
    for (int kk = 1; kk < 64; ++kk) {
        memset(a, 0, sizeof(a));
        memset(b, 0, sizeof(b));
        a[0] = 16; b[0] = 16;
        split(-8, &a[kk], &b[kk]);
        if (run(a, b, 127, 127, 127, 127, 0.f) == 256.0f) printf(" %d", kk);
    }
    printf("\n... and next to the largest term at k = 21:");
    for (int kk = 0; kk < 64; ++kk) {
        if (kk == 21) continue;
        memset(a, 0, sizeof(a));
        memset(b, 0, sizeof(b));
        a[21] = 16; b[21] = 16;
        split(-8, &a[kk], &b[kk]);
        if (run(a, b, 127, 127, 127, 127, 0.f) == 256.0f) printf(" %d", kk);
    }
    // (10) the sum across the groups and C: 1 (block 0) + x 2^-23 (block 1, by its scale), in units of 2^-23 -- 2 = to nearest, 1 = cut
    printf("\nacross groups, result - 1 in ulps:");
    for (double x : {1.75, -1.75, 1.25, -1.25}) {
        memset(a, 0, sizeof(a));
        memset(b, 0, sizeof(b));
        a[0] = 1; b[0] = 1; a[32] = x; b[32] = 1;
        printf("  x = %5.2f -> %g", x, ((double)run(a, b, 127, 127 - 23, 127, 127, 0.f) - 1.0) * 8388608.0);
    }
    // the same with the small term as C
    for (float c : {1.75f, -1.75f}) {
        memset(a, 0, sizeof(a));
        memset(b, 0, sizeof(b));
        a[0] = 1; b[0] = 1;
        printf("  C = %5.2f ulp -> %g", c, ((double)run(a, b, 127, 127, 127, 127, c / 8388608.0f) - 1.0) * 8388608.0);
    }
    printf("\n");
    return 0;
}
