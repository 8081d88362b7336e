// Mel front-end (audio.py:115-210): zero ("constant") centre padding, frames of n_fft with hop,
// periodic Hann window, rfft magnitude, HTK mel filterbank matmul, log(max(., 1e-5)).
// One workgroup per frame: the 1024-point FFT runs in LDS (radix-2 DIT, fp32), the filterbank
// product and the log are fused behind it.  Output layout (frames, n_mels), last STFT frame dropped
// (audio.py:202) => frames = L / hop.
#include "../../include/f5tts_hip.h"
#include "common.hpp"

#define MEL_NFFT 1024
#define MEL_LOG2 10

// One frame of one recording, by one workgroup of 256 threads: the body of mel_kernel and mel_ragged_kernel, so that the two cannot
// drift.  The recording is row[lo .. hi); the frame's first sample is row[start] (start + MEL_NFFT / 2 = the frame's centre); a sample
// outside [lo, hi) counts as zero by the index test and is not loaded.  has_gain (the same for the whole workgroup): every sample is
// multiplied by `gain` first -- that product is rounded once to fp32, then multiplied by the window; without it there is no such
// multiplication at all.
__device__ __forceinline__ void mel_frame(const float* __restrict__ row, long lo, long hi, long start, bool has_gain, float gain,
                                          const float* __restrict__ window, const float* __restrict__ fb, int n_mels,
                                          float* __restrict__ out_frame) {
    __shared__ float re[MEL_NFFT], im[MEL_NFFT];
    __shared__ float twc[MEL_NFFT / 2], tws[MEL_NFFT / 2];
    const int tid = threadIdx.x;
    for (int i = tid; i < MEL_NFFT; i += 256) {
        const long si = start + i;
        float v = 0.0f;
        if (si >= lo && si < hi) {
            float x = row[si];
            if (has_gain) x = x * gain;
            v = x * window[i];
        }
        const int r = (int)(__brev((unsigned)i) >> (32 - MEL_LOG2));
        re[r] = v;
        im[r] = 0.0f;
    }
    for (int i = tid; i < MEL_NFFT / 2; i += 256) {
        float sn, cs;
        sincosf(-6.283185307179586f * (float)i / (float)MEL_NFFT, &sn, &cs);
        twc[i] = cs;
        tws[i] = sn;
    }
    __syncthreads();
    for (int s = 1; s <= MEL_LOG2; ++s) {
        const int half = 1 << (s - 1);
        const int tstep = MEL_NFFT >> s;
        for (int j = tid; j < MEL_NFFT / 2; j += 256) {
            const int grp = j >> (s - 1), pos = j & (half - 1);
            const int i0 = (grp << s) + pos, i1 = i0 + half;
            const float wr = twc[pos * tstep], wi = tws[pos * tstep];
            const float xr = re[i1], xi = im[i1];
            const float tr = wr * xr - wi * xi, ti = wr * xi + wi * xr;
            const float ur = re[i0], ui = im[i0];
            re[i0] = ur + tr;
            im[i0] = ui + ti;
            re[i1] = ur - tr;
            im[i1] = ui - ti;
        }
        __syncthreads();
    }
    // magnitude into re[0..512]
    for (int k = tid; k <= MEL_NFFT / 2; k += 256) {
        const float a = re[k], b = im[k];
        re[k] = sqrtf(a * a + b * b);
    }
    __syncthreads();
    const int nbin = MEL_NFFT / 2 + 1;
    for (int m = tid; m < n_mels; m += 256) {
        const float* f = fb + (size_t)m * nbin;
        float acc = 0.0f;
        for (int k = 0; k < nbin; ++k) acc += re[k] * f[k];
        out_frame[m] = logf(fmaxf(acc, 1e-5f));
    }
}

__global__ __launch_bounds__(256) void mel_kernel(const float* __restrict__ wave, long L, const float* __restrict__ window,
                                                  const float* __restrict__ fb, int hop, int n_mels, float* __restrict__ out) {
    const long frame = blockIdx.x;
    wave += (long)blockIdx.y * L;                                   // batch element: waves are [B][L], outputs [B][frames][n_mels]
    out += (long)blockIdx.y * (long)gridDim.x * n_mels;
    mel_frame(wave, 0, L, frame * hop - MEL_NFFT / 2, false, 1.0f, window, fb, n_mels, out + frame * n_mels);
}

// Padded batch of recordings of different lengths: row b is wave[b][begin[b] .. begin[b] + lens[b]), F_b = lens[b] / hop frames of it
// are mel_frame's (the bits mel_kernel gives for a contiguous copy of the slice, scaled by gain[b]); frames F_b <= n < N are exactly
// 0.0f in every band (the zero padding sample() gives the conditioning, not log(1e-5)).  One workgroup per (frame, row): the test on
// n is the same for all its threads.
__global__ __launch_bounds__(256) void mel_ragged_kernel(const float* __restrict__ wave, int L, const int* __restrict__ begin,
                                                         const int* __restrict__ lens, const float* __restrict__ gain,
                                                         const float* __restrict__ window, const float* __restrict__ fb, int hop,
                                                         int n_mels, float* __restrict__ out) {
    const int b = blockIdx.y;
    const long n = blockIdx.x;
    int b0 = begin[b], len = lens[b];
    b0 = b0 < 0 ? 0 : (b0 > L ? L : b0);                            // a slice that lies cannot take the reads out of the row
    len = len < 0 ? 0 : (len > L - b0 ? L - b0 : len);
    float* o = out + ((long)b * gridDim.x + n) * n_mels;
    if (n >= len / hop) {
        for (int m = threadIdx.x; m < n_mels; m += 256) o[m] = 0.0f;
        return;
    }
    mel_frame(wave + (long)b * L, b0, (long)b0 + len, b0 + n * hop - MEL_NFFT / 2, gain != nullptr, gain ? gain[b] : 1.0f, window, fb,
              n_mels, o);
}

extern "C" int f5_mel_spectrogram_ragged(const float* wave, int B, int64_t L, const int32_t* begin_dev, const int32_t* lens_dev,
                                         const float* gain_dev, const float* window, const float* filterbank, int n_fft, int hop,
                                         int n_mels, float* out, int N, void* stream) {
    F5_REQUIRE(wave && begin_dev && lens_dev && window && filterbank && out, "mel_ragged: null pointer");
    F5_REQUIRE(n_fft == MEL_NFFT, "mel_ragged: only n_fft = 1024 is supported (got %d)", n_fft);
    F5_REQUIRE(hop > 0 && n_mels > 0 && B >= 1 && B <= 65535, "mel_ragged: bad hop / n_mels / batch");
    F5_REQUIRE(N >= 1, "mel_ragged: N = %d frames per row must be >= 1", N);
    F5_REQUIRE(L >= 0 && L <= 0x7fffffffLL, "mel_ragged: L = %lld outside 0..2^31 - 1", (long long)L);
    hipLaunchKernelGGL(mel_ragged_kernel, dim3((unsigned)N, (unsigned)B), dim3(256), 0, (hipStream_t)stream, wave, (int)L, begin_dev,
                       lens_dev, gain_dev, window, filterbank, hop, n_mels, out);
    F5_LAUNCH_CHECK();
    return 0;
}

// =================================================================================================
// Block energies of a padded batch (no reference counterpart; feeds the silence window and the RMS gain of audio.prepare_references):
// energy[b][k] = sum of wave[b][s]^2 over s in [k block, min((k + 1) block, lens[b])).  One wave (64 lanes) per block of samples, four
// per workgroup.  Summation order, fixed by `block` and the position in the block alone: lane l runs acc = fmaf(x, x, acc) over the
// samples l, l + 64, l + 128, ... of the block in increasing order, from acc = 0; the 64 lane sums are then combined by an xor
// butterfly, v += shfl_xor(v, d) for d = 32, 16, 8, 4, 2, 1.  A sample at s >= lens[b] is selected away by the index test: never
// loaded, never multiplied.
// =================================================================================================
__global__ __launch_bounds__(256) void block_energy_kernel(const float* __restrict__ wave, int L, const int* __restrict__ lens,
                                                           int block, float* __restrict__ energy, int nblk) {
    const int lane = threadIdx.x & 63;
    const long k = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (k >= nblk) return;                                          // whole waves leave: the butterfly below stays among 64 live lanes
    const int b = blockIdx.y;
    int len = lens[b];
    len = len < 0 ? 0 : (len > L ? L : len);                        // a length that lies cannot take the reads out of the row
    const float* x = wave + (long)b * L;
    const long s0 = k * block;
    long s1 = s0 + block;
    if (s1 > len) s1 = len;
    float acc = 0.0f;
    for (long s = s0 + lane; s < s1; s += 64) {
        const float v = x[s];
        acc = fmaf(v, v, acc);
    }
    for (int d = 32; d >= 1; d >>= 1) acc += __shfl_xor(acc, d, 64);
    if (lane == 0) energy[(long)b * nblk + k] = acc;
}

extern "C" int f5_wave_block_energy(const float* wave, int B, int64_t L, const int32_t* lens_dev, int block, float* energy, int nblk,
                                    void* stream) {
    F5_REQUIRE(wave && lens_dev && energy, "block_energy: null pointer");
    F5_REQUIRE(B >= 1 && B <= 65535, "block_energy: B = %d outside 1..65535", B);
    F5_REQUIRE(block >= 1 && block <= 4096, "block_energy: block = %d outside 1..4096", block);
    F5_REQUIRE(L >= 0 && L <= 0x7fffffffLL, "block_energy: L = %lld outside 0..2^31 - 1", (long long)L);
    const int64_t want = (L + block - 1) / block;
    F5_REQUIRE(nblk == want, "block_energy: nblk = %d, but ceil(L / block) = %lld", nblk, (long long)want);
    if (L == 0) return 0;
    hipLaunchKernelGGL(block_energy_kernel, dim3((unsigned)((nblk + 3) / 4), (unsigned)B), dim3(256), 0, (hipStream_t)stream, wave,
                       (int)L, lens_dev, block, energy, nblk);
    F5_LAUNCH_CHECK();
    return 0;
}

extern "C" int f5_mel_spectrogram_batch(const float* wave, int B, int64_t L, const float* window, const float* filterbank, int n_fft,
                                        int hop, int n_mels, float* out, void* stream) {
    F5_REQUIRE(wave && window && filterbank && out, "mel: null pointer");
    F5_REQUIRE(n_fft == MEL_NFFT, "mel: only n_fft = 1024 is supported (got %d)", n_fft);
    F5_REQUIRE(hop > 0 && n_mels > 0 && B >= 1 && B <= 65535, "mel: bad hop / n_mels / batch");
    const long frames = L / hop;
    if (frames <= 0) return 0;
    hipLaunchKernelGGL(mel_kernel, dim3((unsigned)frames, (unsigned)B), dim3(256), 0, (hipStream_t)stream, wave, (long)L, window,
                       filterbank, hop, n_mels, out);
    F5_LAUNCH_CHECK();
    return 0;
}
extern "C" int f5_mel_spectrogram(const float* wave, int64_t L, const float* window, const float* filterbank, int n_fft, int hop,
                                  int n_mels, float* out, void* stream) {
    return f5_mel_spectrogram_batch(wave, 1, L, window, filterbank, n_fft, hop, n_mels, out, stream);
}

// =================================================================================================
// Vocos ISTFT head (third-party vocos_mlx `Vocos.decode`, call site cfm.py:399-400; restated from the
// upstream gemelo-ai/vocos ISTFTHead): x[frame][0:513] = log-magnitude, x[frame][513:1026] = phase;
// S = min(exp(mag), 1e2) * (cos p + i sin p); wave = istft(S, n_fft=1024, hop=256, hann, center=True).
// Kernel 1: per frame, Hermitian-extend + inverse FFT in LDS, multiply by the window.
// Kernel 2: overlap-add of <= n_fft/hop frames per sample, divide by the window-square envelope, trim n_fft/2.
// =================================================================================================
__global__ __launch_bounds__(256) void istft_frames_kernel(const float* __restrict__ x, int ldx, const float* __restrict__ window,
                                                           float* __restrict__ frames) {
    __shared__ float re[MEL_NFFT], im[MEL_NFFT];
    __shared__ float twc[MEL_NFFT / 2], tws[MEL_NFFT / 2];
    const int tid = threadIdx.x;
    const long f = blockIdx.x;
    const float* xf = x + f * (long)ldx;
    const int nbin = MEL_NFFT / 2 + 1;
    for (int k = tid; k < MEL_NFFT; k += 256) {
        const int kk = k < nbin ? k : MEL_NFFT - k;             // Hermitian extension X[N-k] = conj(X[k])
        const float mag = fminf(expf(xf[kk]), 100.0f);
        float sn, cs;
        sincosf(xf[nbin + kk], &sn, &cs);
        float vr = mag * cs, vi = mag * sn;
        if (k >= nbin) vi = -vi;
        if (k == 0 || k == MEL_NFFT / 2) vi = 0.0f;            // irfft ignores the imaginary part of DC / Nyquist
        const int r = (int)(__brev((unsigned)k) >> (32 - MEL_LOG2));
        re[r] = vr;
        im[r] = vi;
    }
    for (int i = tid; i < MEL_NFFT / 2; i += 256) {
        float sn, cs;
        sincosf(6.283185307179586f * (float)i / (float)MEL_NFFT, &sn, &cs);   // inverse transform: +i
        twc[i] = cs;
        tws[i] = sn;
    }
    __syncthreads();
    for (int s = 1; s <= MEL_LOG2; ++s) {
        const int half = 1 << (s - 1);
        const int tstep = MEL_NFFT >> s;
        for (int j = tid; j < MEL_NFFT / 2; j += 256) {
            const int grp = j >> (s - 1), pos = j & (half - 1);
            const int i0 = (grp << s) + pos, i1 = i0 + half;
            const float wr = twc[pos * tstep], wi = tws[pos * tstep];
            const float xr = re[i1], xi = im[i1];
            const float tr = wr * xr - wi * xi, ti = wr * xi + wi * xr;
            const float ur = re[i0], ui = im[i0];
            re[i0] = ur + tr;
            im[i0] = ui + ti;
            re[i1] = ur - tr;
            im[i1] = ui - ti;
        }
        __syncthreads();
    }
    for (int i = tid; i < MEL_NFFT; i += 256) frames[f * MEL_NFFT + i] = re[i] * (1.0f / MEL_NFFT) * window[i];
}

__global__ __launch_bounds__(256) void istft_ola_kernel(const float* __restrict__ frames, const float* __restrict__ window,
                                                        float* __restrict__ wave, int nframes, int hop, long out_len) {
    const long s = (long)blockIdx.x * 256 + threadIdx.x;
    if (s >= out_len) return;
    frames += (long)blockIdx.y * nframes * MEL_NFFT;            // batch element
    wave += (long)blockIdx.y * out_len;
    const long pos = s + MEL_NFFT / 2;                          // position in the untrimmed signal
    int f1 = (int)(pos / hop);
    if (f1 > nframes - 1) f1 = nframes - 1;
    long f0l = (pos - MEL_NFFT) / hop + 1;
    if (pos - MEL_NFFT < 0) f0l = 0;
    const int f0 = (int)(f0l < 0 ? 0 : f0l);
    float acc = 0.0f, env = 0.0f;
    for (int f = f0; f <= f1; ++f) {
        const int off = (int)(pos - (long)f * hop);
        if (off >= 0 && off < MEL_NFFT) {
            acc += frames[(long)f * MEL_NFFT + off];
            const float w = window[off];
            env += w * w;
        }
    }
    wave[s] = acc / env;
}

// x [B * nframes][ldx] (rows of utterance b are b*nframes ...), frames_scratch [B * nframes][n_fft], wave [B][hop * (nframes - 1)]:
// two launches for the whole batch
int f5_launch_istft(const float* x, int ldx, const float* window, float* frames_scratch, float* wave, int B, int nframes, int hop,
                    hipStream_t s) {
    F5_REQUIRE(x && window && frames_scratch && wave, "istft: null pointer");
    F5_REQUIRE(B >= 1 && B <= 65535 && nframes >= 1 && hop > 0 && ldx >= MEL_NFFT + 2, "istft: bad sizes");
    hipLaunchKernelGGL(istft_frames_kernel, dim3((unsigned)(B * nframes)), dim3(256), 0, s, x, ldx, window, frames_scratch);
    const long out_len = (long)hop * (nframes - 1);
    if (out_len > 0)
        hipLaunchKernelGGL(istft_ola_kernel, dim3(f5_cdiv(out_len, 256), (unsigned)B), dim3(256), 0, s, frames_scratch, window, wave,
                           nframes, hop, out_len);
    F5_LAUNCH_CHECK();
    return 0;
}
extern "C" int f5_op_istft_batch(const float* x, int ldx, const float* window, float* frames_scratch, float* wave, int B, int nframes,
                                 int n_fft, int hop, void* stream) {
    F5_REQUIRE(n_fft == MEL_NFFT, "istft: only n_fft = 1024 is supported (got %d)", n_fft);
    return f5_launch_istft(x, ldx, window, frames_scratch, wave, B, nframes, hop, (hipStream_t)stream);
}
extern "C" int f5_op_istft(const float* x, int ldx, const float* window, float* frames_scratch, float* wave, int nframes,
                           int n_fft, int hop, void* stream) {
    return f5_op_istft_batch(x, ldx, window, frames_scratch, wave, 1, nframes, n_fft, hop, stream);
}

// Overlap-add of a padded batch: row b holds lens[b] <= nframes frames (rows stay nframes frames apart).  Its f1 clamp and its
// envelope stop at lens[b], so sample s < hop * (lens[b] - 1) is the sum istft_ola_kernel forms for that row alone, term by term; the
// rest of the row, up to hop * (nframes - 1), is written as 0.0f.  Frames past lens[b] are never read.
__global__ __launch_bounds__(256) void istft_ola_ragged_kernel(const float* __restrict__ frames, const float* __restrict__ window,
                                                               float* __restrict__ wave, int nframes, int hop, long out_len,
                                                               const int* __restrict__ lens) {
    const long s = (long)blockIdx.x * 256 + threadIdx.x;
    if (s >= out_len) return;
    frames += (long)blockIdx.y * nframes * MEL_NFFT;            // batch element
    wave += (long)blockIdx.y * out_len;
    int nf = lens[blockIdx.y];
    nf = nf < 1 ? 1 : (nf > nframes ? nframes : nf);            // a length that lies cannot take the reads out of the row
    if (s >= (long)hop * (nf - 1)) {
        wave[s] = 0.0f;
        return;
    }
    const long pos = s + MEL_NFFT / 2;                          // position in the untrimmed signal
    int f1 = (int)(pos / hop);
    if (f1 > nf - 1) f1 = nf - 1;
    long f0l = (pos - MEL_NFFT) / hop + 1;
    if (pos - MEL_NFFT < 0) f0l = 0;
    const int f0 = (int)(f0l < 0 ? 0 : f0l);
    float acc = 0.0f, env = 0.0f;
    for (int f = f0; f <= f1; ++f) {
        const int off = (int)(pos - (long)f * hop);
        if (off >= 0 && off < MEL_NFFT) {
            acc += frames[(long)f * MEL_NFFT + off];
            const float w = window[off];
            env += w * w;
        }
    }
    wave[s] = acc / env;
}

// lens dev [B], 2 <= lens[b] <= nframes.  istft_frames_kernel is per frame and runs as it is, over every frame of the padded batch
// (the padding rows of the vocoder hold finite values; whatever they transform to is not read).
int f5_launch_istft_ragged(const float* x, int ldx, const float* window, float* frames_scratch, float* wave, int B, int nframes, int hop,
                           const int* lens, hipStream_t s) {
    F5_REQUIRE(x, "istft_ragged: x is null");
    F5_REQUIRE(window, "istft_ragged: window is null");
    F5_REQUIRE(frames_scratch, "istft_ragged: frames_scratch is null");
    F5_REQUIRE(wave, "istft_ragged: wave is null");
    F5_REQUIRE(lens, "istft_ragged: lens is null");
    F5_REQUIRE(B >= 1 && B <= 65535, "istft_ragged: B = %d outside 1..65535", B);
    F5_REQUIRE(nframes >= 2, "istft_ragged: nframes must be >= 2 (got %d)", nframes);
    F5_REQUIRE((long)B * nframes <= 0x7fffffffL, "istft_ragged: B * nframes = %ld frames exceed the grid", (long)B * nframes);
    F5_REQUIRE(hop > 0 && MEL_NFFT % hop == 0, "istft_ragged: hop = %d must divide n_fft", hop);
    F5_REQUIRE(ldx >= MEL_NFFT + 2, "istft_ragged: ldx = %d below n_fft + 2", ldx);
    hipLaunchKernelGGL(istft_frames_kernel, dim3((unsigned)(B * nframes)), dim3(256), 0, s, x, ldx, window, frames_scratch);
    const long out_len = (long)hop * (nframes - 1);
    hipLaunchKernelGGL(istft_ola_ragged_kernel, dim3(f5_cdiv(out_len, 256), (unsigned)B), dim3(256), 0, s, frames_scratch, window, wave,
                       nframes, hop, out_len, lens);
    F5_LAUNCH_CHECK();
    return 0;
}
extern "C" int f5_op_istft_ragged(const float* x, int ldx, const float* window, float* frames_scratch, float* wave, int B, int nframes,
                                  int n_fft, int hop, const int32_t* lens_dev, void* stream) {
    F5_REQUIRE(n_fft == MEL_NFFT, "istft_ragged: only n_fft = 1024 is supported (got %d)", n_fft);
    return f5_launch_istft_ragged(x, ldx, window, frames_scratch, wave, B, nframes, hop, lens_dev, (hipStream_t)stream);
}

// =================================================================================================
// Polyphase resampler (no reference counterpart: generate.py:147-148 refuses anything but 24 kHz).  Hann-windowed sinc, the
// design of torchaudio's default `resample`; the table is built on the host (audio.py resample_table).  With o = orig / gcd,
// n = new / gcd:  out[j n + i] = sum_k h[i][k] x[j o + k - width],  x = 0 outside [0, L).  The kernel gets the compact table:
// first[i] = first non-zero tap of phase i, taps [T][n] = the T taps from there on (consecutive lanes hold consecutive phases
// and read consecutive words).  One workgroup per RS_TILE consecutive outputs of one batch row: it stages the input span of its
// tile into LDS once (coalesced, zero-filled by an index test), then every thread runs T FMAs per output from LDS.
// =================================================================================================
#define RS_TILE 1024                 // outputs per workgroup
#define RS_LDS 8192                  // floats of LDS for the staged span

// floats a tile can need: its outputs come from at most (RS_TILE - 1) / n + 2 input groups of o samples, the last of which reaches
// first[i] + T - 1 <= 2 width + o - 1 + T - 1 past its start
static inline int64_t resample_span_max(int o, int n, int T, int width) {
    return ((int64_t)(RS_TILE - 1) / n + 1) * o + 2 * (int64_t)width + o + T - 1;
}

__global__ __launch_bounds__(256) void resample_kernel(const float* __restrict__ wave, long L, const float* __restrict__ taps,
                                                       const int* __restrict__ first, int o, int n, int T, int width,
                                                       float* __restrict__ out, long L_out) {
    __shared__ float xs[RS_LDS];
    const int tid = threadIdx.x;
    wave += (long)blockIdx.y * L;                                   // batch element: waves are [B][L], outputs [B][L_out]
    out += (long)blockIdx.y * L_out;
    const long p0 = (long)blockIdx.x * RS_TILE;
    const long p1 = p0 + RS_TILE < L_out ? p0 + RS_TILE : L_out;
    const long j0 = p0 / n, j1 = (p1 - 1) / n;
    const long g0 = j0 * o - width;                                 // sample index of xs[0]
    const int span = (int)(j1 - j0) * o + 2 * width + o + T - 1;    // <= resample_span_max <= RS_LDS (checked on the host)
    for (int s = tid; s < span; s += 256) {
        const long g = g0 + s;
        xs[s] = (g >= 0 && g < L) ? wave[g] : 0.0f;
    }
    __syncthreads();
    const int fmax = 2 * width + o - 1;
    for (long p = p0 + tid; p < p1; p += 256) {
        const long j = p / n;
        const int i = (int)(p - j * n);
        int f = first[i];
        f = f < 0 ? 0 : (f > fmax ? fmax : f);                      // a table that lies cannot take the reads out of xs
        const float* x = xs + (int)(j - j0) * o + f;
        const float* h = taps + i;
        float acc = 0.0f;
        for (int t = 0; t < T; ++t) acc = fmaf(h[(size_t)t * n], x[t], acc);
        out[p] = acc;
    }
}

extern "C" int f5_resample_batch(const float* wave, int B, int64_t L, const float* taps, const int32_t* first, int o, int n, int T,
                                 int width, float* out, int64_t L_out, void* stream) {
    F5_REQUIRE(wave && taps && first && out, "resample: null pointer");
    F5_REQUIRE(o >= 1 && n >= 1 && T >= 1 && width >= 1, "resample: o, n, T and width must be >= 1 (got %d, %d, %d, %d)", o, n, T, width);
    int a = o, b = n;
    while (b) {
        const int r = a % b;
        a = b;
        b = r;
    }
    F5_REQUIRE(a == 1, "resample: o = %d and n = %d are not coprime (gcd %d): divide the rates by their gcd", o, n, a);
    F5_REQUIRE(T <= 2 * (int64_t)width + o, "resample: T = %d exceeds the 2 * width + o = %lld taps of a phase", T,
               (long long)(2 * (int64_t)width + o));
    F5_REQUIRE(B >= 1 && B <= 65535, "resample: batch %d outside 1..65535", B);
    F5_REQUIRE(L >= 0, "resample: negative length %lld", (long long)L);
    F5_REQUIRE(L <= (INT64_MAX - o) / n, "resample: length %lld too long for n = %d", (long long)L, n);
    const int64_t want = ((int64_t)n * L + o - 1) / o;
    F5_REQUIRE(L_out == want, "resample: L_out = %lld, but ceil(n * L / o) = %lld", (long long)L_out, (long long)want);
    const int64_t need = resample_span_max(o, n, T, width);
    F5_REQUIRE(need <= RS_LDS,
               "resample: ratio %d:%d too large: a tile of %d outputs spans up to %lld input samples (T = %d, width = %d), the kernel "
               "stages at most %d",
               o, n, RS_TILE, (long long)need, T, width, RS_LDS);
    if (L == 0) return 0;
    const int64_t tiles = (L_out + RS_TILE - 1) / RS_TILE;
    F5_REQUIRE(tiles <= 0x7fffffff, "resample: %lld output tiles exceed the grid", (long long)tiles);
    hipLaunchKernelGGL(resample_kernel, dim3((unsigned)tiles, (unsigned)B), dim3(256), 0, (hipStream_t)stream, wave, (long)L, taps,
                       first, o, n, T, width, out, (long)L_out);
    F5_LAUNCH_CHECK();
    return 0;
}

// =================================================================================================
// Waveform patch (speech editing: no reference counterpart).  The vocoded result of an edit call keeps the original samples outside
// the edited spans: row b of `out` is laid out by a table of segments (dst_begin, dst_end, src_begin), sorted and contiguous from 0;
// src_begin >= 0 = a KEPT segment (out = src[src_begin + s - dst_begin], selected: the source's own bits), src_begin < 0 = a
// REGENERATED one (out = gen).  Where a kept segment meets a regenerated neighbour (the table entry before / after it, whatever its
// length) its first / last F samples cross-fade: out = g + fade[i] (o - g), one FMA on the fp32 difference, i counted from the seam.
// Samples past the last segment are exactly 0.0f.  The table travels as a kernel argument (copied at launch time, like
// stage_words_kernel's words): WP_ROWS_MAX rows of at most 64 segments per launch.
// =================================================================================================
#define WP_SEG_MAX 64
#define WP_WORDS 960                 // int32 words of table per launch (a kernel argument of 3 840 bytes)
struct F5WavePatchTable {
    int w[WP_WORDS];                 // [rows][S][3]
};
__global__ __launch_bounds__(256) void wave_patch_kernel(const float* __restrict__ gen, const float* __restrict__ src,
                                                         F5WavePatchTable t, const float* __restrict__ fade, float* __restrict__ out,
                                                         long L, long Ls, int S, int F) {
    const long s = (long)blockIdx.x * 256 + threadIdx.x;
    if (s >= L) return;
    const int* seg = t.w + (size_t)blockIdx.y * S * 3;
    gen += (long)blockIdx.y * L;                                    // the launcher offsets gen / src / out to the first row of the launch
    src += (long)blockIdx.y * Ls;
    out += (long)blockIdx.y * L;
    float v = 0.0f;                                                 // past the last segment
    for (int k = 0; k < S; ++k) {
        const int d0 = seg[3 * k], d1 = seg[3 * k + 1], s0 = seg[3 * k + 2];
        if (s < d0 || s >= d1) continue;
        const float g = gen[s];
        v = g;
        if (s0 >= 0) {
            const long si = (long)s0 + (s - d0);
            if (si < Ls) {                                          // (checked on the host: a table that lies cannot take the load out of the row)
                const float o = src[si];
                v = o;
                const long i0 = s - d0, i1 = (long)d1 - 1 - s;
                if (i0 < F && k > 0 && seg[3 * (k - 1) + 2] < 0) v = fmaf(fade[i0], o - g, g);
                else if (i1 < F && k + 1 < S && seg[3 * (k + 1) + 2] < 0) v = fmaf(fade[i1], o - g, g);
            }
        }
        break;
    }
    out[s] = v;
}

extern "C" int f5_op_wave_patch(const float* gen, const float* src, const int32_t* segs_host, const float* fade, float* out, int B,
                                int64_t L, int64_t Ls, int S, int F, void* stream) {
    F5_REQUIRE(gen && src && segs_host && out && (fade || F <= 0), "wave_patch: null pointer");
    F5_REQUIRE(B >= 1 && B <= 65535, "wave_patch: batch %d outside 1..65535", B);
    F5_REQUIRE(S >= 1 && S <= WP_SEG_MAX, "wave_patch: S = %d segments per row outside 1..%d", S, WP_SEG_MAX);
    F5_REQUIRE(F >= 0, "wave_patch: negative fade length F = %d", F);
    F5_REQUIRE(L >= 0 && L <= 0x7fffffff && Ls >= 0 && Ls <= 0x7fffffff, "wave_patch: lengths L = %lld, Ls = %lld outside 0..2^31 - 1",
               (long long)L, (long long)Ls);
    for (int b = 0; b < B; ++b) {
        const int32_t* t = segs_host + (size_t)b * S * 3;
        int64_t at = 0;
        for (int k = 0; k < S; ++k) {
            const int64_t d0 = t[3 * k], d1 = t[3 * k + 1], s0 = t[3 * k + 2];
            F5_REQUIRE(d0 == at && d1 >= d0,
                       "wave_patch: row %d segment %d is [%lld, %lld) where %lld was expected: the table must be sorted and contiguous from 0",
                       b, k, (long long)d0, (long long)d1, (long long)at);
            F5_REQUIRE(d1 <= L, "wave_patch: row %d segment %d ends at %lld, beyond the row length L = %lld", b, k, (long long)d1, (long long)L);
            at = d1;
            if (s0 < 0) continue;
            F5_REQUIRE(s0 + (d1 - d0) <= Ls, "wave_patch: row %d kept segment %d reads source samples [%lld, %lld), outside [0, %lld]", b, k,
                       (long long)s0, (long long)(s0 + d1 - d0), (long long)Ls);
            const int nfade = (k > 0 && t[3 * (k - 1) + 2] < 0 ? 1 : 0) + (k + 1 < S && t[3 * (k + 1) + 2] < 0 ? 1 : 0);
            F5_REQUIRE(d1 - d0 >= (int64_t)nfade * F,
                       "wave_patch: row %d kept segment %d is %lld samples long, shorter than its %d fade(s) of F = %d samples", b, k,
                       (long long)(d1 - d0), nfade, F);
        }
    }
    if (L == 0) return 0;
    const int rows_max = WP_WORDS / (3 * S);
    for (int b0 = 0; b0 < B; b0 += rows_max) {
        const int rows = B - b0 < rows_max ? B - b0 : rows_max;
        F5WavePatchTable t;
        memcpy(t.w, segs_host + (size_t)b0 * S * 3, (size_t)rows * S * 3 * sizeof(int));
        hipLaunchKernelGGL(wave_patch_kernel, dim3((unsigned)((L + 255) / 256), (unsigned)rows), dim3(256), 0, (hipStream_t)stream,
                           gen + (size_t)b0 * L, src + (size_t)b0 * Ls, t, fade, out + (size_t)b0 * L, (long)L, (long)Ls, S, F);
    }
    F5_LAUNCH_CHECK();
    return 0;
}

// =================================================================================================
// Sentence join (no reference counterpart; the back half of generate() / generate_many(): docs/sentence_joins.md).  Q output waves are
// laid out from R decoded rows by a table of segments (dst_begin, src_row, src_begin, len, fade_in, fade_out), in samples; the rules
// per output sample are in include/f5tts_hip.h.  One thread per output sample, one workgroup per 256 consecutive samples of one output
// row: the segment table is a kernel argument (uniform reads), the stores are one coalesced dword per lane (rows are Lout floats apart,
// so they share no alignment wider than that), and each source sample is loaded by the one or two lanes whose output it reaches --
// selected by the index tests, so nothing outside the ranges the table names is loaded.  Of the S entries of a row at most two cover
// a sample (checked on the host): the first hit is the earlier segment, the second the one that fades in over it.
// The fade weight w(i, F) = (2 i + 1) / (2 F) is one correctly rounded fp32 division of two integers below 2^24 (hence F <= 2^22).
// =================================================================================================
#define WJ_SEG_MAX 64
#define WJ_FADE_MAX (1 << 22)
#define WJ_WORDS 960                 // int32 words of table per launch (a kernel argument of 3 840 bytes): 160 segments
struct F5WaveJoinTable {
    int w[WJ_WORDS];                 // [rows][S][6]
};
__device__ __forceinline__ float wave_join_weight(int i, int F) { return __fdiv_rn((float)(2 * i + 1), (float)(2 * F)); }

__global__ __launch_bounds__(256) void wave_join_kernel(const float* __restrict__ src, int R, long Ls, F5WaveJoinTable t, int S,
                                                        float* __restrict__ out, long Lout) {
    const long s = (long)blockIdx.x * 256 + threadIdx.x;
    if (s >= Lout) return;
    const int* seg = t.w + (size_t)blockIdx.y * S * 6;
    out += (long)blockIdx.y * Lout;                                 // the launcher offsets out to the first row of the launch
    int ka = -1, kb = -1;
    for (int k = 0; k < S; ++k) {
        const long i = s - seg[6 * k];
        if (i >= 0 && i < seg[6 * k + 3]) {
            if (ka < 0) ka = k;
            else kb = k;
        }
    }
    float v = 0.0f;                                                 // covered by no segment
    if (ka >= 0) {
        const int* a = seg + 6 * ka;
        const long ia = s - a[0], sa = (long)a[2] + ia;
        // (checked on the host: a table that lies cannot take the loads out of src)
        const float xa = (a[1] < R && sa < Ls) ? src[(long)a[1] * Ls + sa] : 0.0f;
        if (kb < 0) {
            const long ja = (long)a[3] - 1 - ia;
            v = xa;                                                 // selected: the source's own bits
            if (ia < a[4]) v = __fmul_rn(wave_join_weight((int)ia, a[4]), xa);
            else if (ja < a[5]) v = __fmul_rn(wave_join_weight((int)ja, a[5]), xa);
        } else {
            const int* b = seg + 6 * kb;
            const long ib = s - b[0], sb = (long)b[2] + ib;
            const float xb = (b[1] < R && sb < Ls) ? src[(long)b[1] * Ls + sb] : 0.0f;
            v = fmaf(wave_join_weight((int)ib, b[4]), xb - xa, xa);
        }
    }
    out[s] = v;
}

extern "C" int f5_wave_join(const float* src, int R, int64_t Ls, const int32_t* segs_host, int Q, int S, float* out, int64_t Lout,
                            void* stream) {
    F5_REQUIRE(src && segs_host && out, "wave_join: null pointer");
    F5_REQUIRE(R >= 1 && R <= 65535, "wave_join: R = %d source rows outside 1..65535", R);
    F5_REQUIRE(Q >= 1 && Q <= 65535, "wave_join: Q = %d output rows outside 1..65535", Q);
    F5_REQUIRE(S >= 1 && S <= WJ_SEG_MAX, "wave_join: S = %d segments per row outside 1..%d", S, WJ_SEG_MAX);
    F5_REQUIRE(Ls >= 0 && Ls <= 0x7fffffffLL, "wave_join: Ls = %lld outside 0..2^31 - 1", (long long)Ls);
    F5_REQUIRE(Lout >= 0 && Lout <= 0x7fffffffLL, "wave_join: Lout = %lld outside 0..2^31 - 1", (long long)Lout);
    for (int q = 0; q < Q; ++q) {
        const int32_t* t = segs_host + (size_t)q * S * 6;
        int prev = -1;                                              // the last segment that was not empty
        for (int k = 0; k < S; ++k) {
            const int64_t d0 = t[6 * k], row = t[6 * k + 1], s0 = t[6 * k + 2], len = t[6 * k + 3], fi = t[6 * k + 4], fo = t[6 * k + 5];
            F5_REQUIRE(d0 >= 0 && row >= 0 && s0 >= 0 && len >= 0 && fi >= 0 && fo >= 0,
                       "wave_join: row %d segment %d has a negative field (%lld, %lld, %lld, %lld, %lld, %lld)", q, k, (long long)d0,
                       (long long)row, (long long)s0, (long long)len, (long long)fi, (long long)fo);
            F5_REQUIRE(row < R, "wave_join: row %d segment %d names source row %lld, but R = %d", q, k, (long long)row, R);
            F5_REQUIRE(s0 + len <= Ls, "wave_join: row %d segment %d reads source samples [%lld, %lld), outside [0, %lld]", q, k,
                       (long long)s0, (long long)(s0 + len), (long long)Ls);
            F5_REQUIRE(fi <= WJ_FADE_MAX && fo <= WJ_FADE_MAX, "wave_join: row %d segment %d has a fade longer than 2^22 samples (%lld, %lld)",
                       q, k, (long long)fi, (long long)fo);
            F5_REQUIRE(fi + fo <= len, "wave_join: row %d segment %d is %lld samples long, shorter than its fades of %lld + %lld", q, k,
                       (long long)len, (long long)fi, (long long)fo);
            if (len == 0) continue;                                 // an empty entry covers nothing and takes no part in the order
            F5_REQUIRE(d0 + len <= Lout, "wave_join: row %d segment %d ends at %lld, beyond the row length Lout = %lld", q, k,
                       (long long)(d0 + len), (long long)Lout);
            if (prev >= 0) {
                const int64_t p0 = t[6 * prev], p1 = p0 + t[6 * prev + 3], pfo = t[6 * prev + 5];
                F5_REQUIRE(d0 >= p0, "wave_join: row %d segment %d begins at %lld, before segment %d at %lld: the table must be sorted by dst_begin",
                           q, k, (long long)d0, prev, (long long)p0);
                // a pure cross-fade: the last F samples of one segment are the first F of the next, F = its fade-out = the other's
                // fade-in.  With fade_in + fade_out <= len on both sides no third segment can reach such a sample.
                F5_REQUIRE(d0 >= p1 || (p1 - d0 == pfo && p1 - d0 == fi),
                           "wave_join: row %d segments %d and %d overlap by %lld samples, which is not a pure cross-fade (fade_out %lld, fade_in %lld)",
                           q, prev, k, (long long)(p1 - d0), (long long)pfo, (long long)fi);
            }
            prev = k;
        }
    }
    if (Lout == 0) return 0;
    const int rows_max = WJ_WORDS / (6 * S);
    for (int q0 = 0; q0 < Q; q0 += rows_max) {
        const int rows = Q - q0 < rows_max ? Q - q0 : rows_max;
        F5WaveJoinTable t;
        memcpy(t.w, segs_host + (size_t)q0 * S * 6, (size_t)rows * S * 6 * sizeof(int));
        hipLaunchKernelGGL(wave_join_kernel, dim3((unsigned)((Lout + 255) / 256), (unsigned)rows), dim3(256), 0, (hipStream_t)stream, src,
                           R, (long)Ls, t, S, out + (size_t)q0 * Lout, (long)Lout);
    }
    F5_LAUNCH_CHECK();
    return 0;
}
