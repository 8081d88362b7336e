// Largest ULP error of the device math functions the row kernels call (csrc/rowops.hip: rsqrtf, expf, log1pf, sinf, cosf, powf, plus
// sqrtf and SiLU), of the exp2 instruction behind csrc/attention.hip's softmax and f5_mish (__builtin_amdgcn_exp2f), and of what the
// audio and conv-pos kernels add to those (csrc/audio.hip: sincosf on the FFT twiddle grid and on ISTFT phases, logf; common.hpp
// f5_mish: __builtin_amdgcn_rcpf), against fp64 on the host, over 2^21 arguments per function in the ranges those kernels produce plus
// the exact grids of the time / rotation / position / twiddle tables.  abs_u is the largest absolute error in units of 2^-24 (what a
// sine or cosine near one of its zeros is judged by).
// tests/rowops_matrix.py, tests/attention_matrix.py and tests/convaudio_matrix.py grant four times the figures this prints (their
// docstrings have the tables): re-run after a ROCm update and refresh all three.  hipcc --offload-arch=gfx950 -O3 math_ulp.hip -o bin/math_ulp
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdio>
#include <vector>
#include <random>
__global__ void k(const float* x, float* y, int n, int fn) {
    int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    float v = x[i], r;
    switch (fn) {
        case 0: r = rsqrtf(v); break;
        case 1: r = expf(v); break;
        case 2: r = log1pf(v); break;
        case 3: r = sinf(v); break;
        case 4: r = cosf(v); break;
        case 5: r = powf(10000.0f, v); break;
        case 6: r = 1.0f / powf(10000.0f, v); break;
        case 7: r = sqrtf(v); break;
        case 9: r = __builtin_amdgcn_exp2f(v); break;
        case 10: case 12: { float c; sincosf(v, &r, &c); break; }
        case 11: case 13: { float sn; sincosf(v, &sn, &r); break; }
        case 14: r = logf(v); break;
        case 15: r = __builtin_amdgcn_rcpf(v); break;
        default: r = v / (1.0f + expf(-v)); break;
    }
    y[i] = r;
}
static double ref(int fn, double v) {
    switch (fn) {
        case 0: return 1.0 / std::sqrt(v);
        case 1: return std::exp(v);
        case 2: return std::log1p(v);
        case 3: return std::sin(v);
        case 4: return std::cos(v);
        case 5: return std::pow(10000.0, v);
        case 6: return 1.0 / std::pow(10000.0, v);
        case 7: return std::sqrt(v);
        case 9: return std::exp2(v);
        case 10: case 12: return std::sin(v);
        case 11: case 13: return std::cos(v);
        case 14: return std::log(v);
        case 15: return 1.0 / v;
        default: return v / (1.0 + std::exp(-v));
    }
}
int main() {
    const char* names[] = {"rsqrtf", "expf", "log1pf", "sinf", "cosf", "powf(1e4,x)", "1/powf(1e4,x)", "sqrtf", "silu", "amdgcn_exp2f",
                           "sincosf.sin twid", "sincosf.cos twid", "sincosf.sin ph", "sincosf.cos ph", "logf", "amdgcn_rcpf"};
    std::mt19937_64 g(1);
    const int n = 1 << 21;
    float *dx, *dy;
    if (hipMalloc(&dx, n * 4) != hipSuccess || hipMalloc(&dy, n * 4) != hipSuccess) return 2;
    for (int fn = 0; fn < 16; ++fn) {
        std::vector<float> x(n), y(n);
        std::uniform_real_distribution<double> u(0.0, 1.0);
        for (int i = 0; i < n; ++i) {
            double t = u(g);
            switch (fn) {
                case 0: case 7: x[i] = (float)std::pow(10.0, -6.0 + 15.0 * t); break;   // var + eps, sums of squares
                case 1: x[i] = (float)(-30.0 + 50.0 * t); break;                     // softplus argument, time frequencies
                case 2: x[i] = (float)std::exp(-30.0 + 50.0 * t); break;            // exp(mean), mean <= 20
                case 3: case 4: x[i] = (float)(4096.0 * t); break;                   // angles of the tables
                case 5: case 6: x[i] = (float)t; break;                              // 2 j / dim
                case 9: x[i] = (float)(-60.0 + 75.0 * t); break;                    // scores against the reference point, exp2 units: <= 14 on the fast paths
                case 10: case 11: { int j = i & 511; float a = 6.2831853f * (float)j / 1024.0f; x[i] = (i & 512) ? -a : a; break; }   // the twiddle grid of the 1024-point FFTs, both directions, and nothing else
                case 12: case 13: x[i] = (float)(-100.0 + 200.0 * t); break;        // ISTFT phases
                case 14: x[i] = (float)std::pow(10.0, -5.0 + 19.0 * t); break;      // filterbank sums behind the 1e-5 floor, up to 1e14 (the matrix feeds 1e10 samples)
                case 15: x[i] = (float)(2.0 * std::pow(10.0, 30.0 * t)); break;      // w (w + 2) + 2 of f5_mish, w = exp(min(x, 30))
                default: x[i] = (float)(-20.0 + 40.0 * t); break;
            }
        }
        // the grids the kernels really use
        int q = 0;
        if (fn == 5 || fn == 6) for (int d : {4, 64, 100, 128, 256, 512, 516, 1024}) for (int j = 0; j < d / 2; ++j) x[q++] = (float)(2 * j) / (float)d;
        if (fn == 1) for (int half : {2, 127, 128, 512}) { float step = logf(10000.0f) / (float)(half - 1); for (int j = 0; j < half; ++j) x[q++] = (float)j * -step; }
        if (fn == 3 || fn == 4) for (int d : {64, 128, 512}) for (int j = 0; j < d / 2; ++j) { float inv = 1.0f / powf(10000.0f, (float)(2 * j) / (float)d); for (int p = 0; p < 4096 && q < n / 2; p += 7) x[q++] = (float)p * inv; }
        if (hipMemcpy(dx, x.data(), n * 4, hipMemcpyHostToDevice) != hipSuccess) return 3;
        hipLaunchKernelGGL(k, dim3(n / 256), dim3(256), 0, 0, dx, dy, n, fn);
        if (hipMemcpy(y.data(), dy, n * 4, hipMemcpyDeviceToHost) != hipSuccess) return 3;
        double worst = 0, worst_abs = 0; float wx = 0;
        for (int i = 0; i < n; ++i) {
            double r = ref(fn, (double)x[i]);
            if (r == 0.0 || !std::isfinite(r)) continue;
            int e; std::frexp(r, &e);                       // |r| in [2^(e-1), 2^e)
            double ulp = std::ldexp(1.0, e - 24);
            if (std::fabs(r) < 1.17549435e-38) ulp = std::ldexp(1.0, -149);
            double err = std::fabs((double)y[i] - r) / ulp;
            if (err > worst) { worst = err; wx = x[i]; }
            worst_abs = std::fmax(worst_abs, std::fabs((double)y[i] - r));
        }
        printf("%-16s max_ulp %.3f at x=%.9g  max_abs %.3e  abs_u %.3f\n", names[fn], worst, wx, worst_abs, worst_abs * 16777216.0);
    }
    return 0;
}
