// The mel front end: melspectrogram(y) = normalize(amp_to_db(mel_basis @ |stft(y)|)) of wavernn/utils/dsp.py:72-81 with the
// librosa semantics of the reference's era (center=True reflect padding, periodic Hann of win_length centred in n_fft, Slaney
// filterbank).  One workgroup of 256 threads per frame, grid (T_max, B): the frame's non-zero taps are gathered straight from the
// clip with the reflect index, the 2048 real points run as a 1024-point complex radix-4 transform in LDS plus the split pass,
// the magnitudes stay in LDS and the sparse filterbank, dB and normalisation finish the column.  Nothing crosses workgroups.
//
// The kernel is a template on PROFILE.  <false> is the kernel above and nothing else.  <true> carries the feature profile of
// wrnn_mel_features (the Tacotron-side mel of tacotron/datasets/audio.py:95-102, 203-207, 250-295) as run-time, workgroup-uniform
// arms of the same stages: pre-emphasis and the rescale to the pre-emphasised peak fused into the tap gather, zero padding, the power
// spectrum, ref_level_db and the symmetric normalisation.  The peak comes from melspec_peak_kernel, one launch in front.
#include <cmath>

#include "dsp_device.h"
#include "dsp_tables.h"
#include "mel_internal.h"

namespace {

constexpr int NC = WRNN_MEL_NFFT / 2;   // complex points

// sample j of the pre-emphasised clip, 0 <= j < n: x[j] - k x[j-1] with x[-1] = 0.  The peak launch and the tap gather share it.
__device__ inline float preemph_at(const float *x, long j, float k) { return x[j] - k * (j > 0 ? x[j - 1] : 0.0f); }

constexpr int PEAK_THREADS = 256, PEAK_PER_THREAD = 16, PEAK_CHUNK = PEAK_THREADS * PEAK_PER_THREAD;

// grid (ceil(n_max / PEAK_CHUNK), B): the maximum of one chunk of one clip, then one atomic per workgroup.  The values are
// non-negative floats, whose order is the order of their bit patterns, so the atomic is an unsigned integer maximum and the result does
// not depend on the order the workgroups arrive in.  peak[] is zeroed in front of the launch.
__global__ void __launch_bounds__(PEAK_THREADS) melspec_peak_kernel(const float *wav, long n_max, const int32_t *n_samples, float k, float *peak) {
    __shared__ float part[PEAK_THREADS / 64];
    const int b = blockIdx.y, tid = threadIdx.x;
    long n = n_samples[b];
    if (n > n_max) n = n_max;
    const long lo = (long)blockIdx.x * PEAK_CHUNK;
    if (lo >= n) return;              // workgroup-uniform: the chunk lies past this clip's own end
    const float *x = wav + (long)b * n_max;
    float m = 0.0f;
#pragma unroll 4
    for (int i = 0; i < PEAK_PER_THREAD; ++i) {
        const long j = lo + tid + (long)i * PEAK_THREADS;
        if (j < n) m = fmaxf(m, fabsf(preemph_at(x, j, k)));
    }
    for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
    if ((tid & 63) == 0) part[tid >> 6] = m;
    __syncthreads();
    if (tid == 0) {
        for (int w = 1; w < PEAK_THREADS / 64; ++w) m = fmaxf(m, part[w]);
        atomicMax((unsigned int *)(peak + b), __float_as_uint(m));
    }
}

template <bool PROFILE>
__global__ void __launch_bounds__(WRNN_MEL_THREADS) melspec_kernel(WrnnMelArgs a) {
    __shared__ float2 z[NC];          // 8 KiB: the transform, in place
    __shared__ float mag[NC + 1];     // 4 KiB + 4 B: |X[k]| (or |X[k]|^2), k = 0 .. n_fft/2
    const int t = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
    long n = a.n_samples[b];
    if (n > a.n_max) n = a.n_max;
    // a clip that cannot be reflect-padded has no frames (the host side refuses it before the launch); zero padding needs one sample
    const long T_b = n >= (PROFILE && a.pad_zero ? 1 : NC + 1) ? 1 + n / a.hop : 0;
    float *out = a.out + (long)b * a.n_mels * a.T_max + t;
    if (t >= T_b) {                   // workgroup-uniform: past the clip's own end, the zero conditioning of a ragged batch
        for (int m = tid; m < a.n_mels; m += WRNN_MEL_THREADS) out[(long)m * a.T_max] = 0.0f;
        return;
    }
    const float *x = a.wav + (long)b * a.n_max;
    const int off = (WRNN_MEL_NFFT - a.win_length) / 2;
    const long j0 = (long)t * a.hop - NC;          // clip index of frame sample 0
    // z[k] = x[2k] + i x[2k + 1] of the windowed frame, stored digit-reversed for the in-place decimation-in-time passes
    // profile: the clip is pre-emphasised and scaled to the peak `rescale` on the fly; an all-zero clip (peak 0) stays as it is
    float scale = 1.0f;
    if (PROFILE && a.rescale > 0.0f) {
        const float peak = a.peak[b];
        if (peak > 0.0f) scale = a.rescale / peak;
    }
    for (int k = tid; k < NC; k += WRNN_MEL_THREADS) {
        float v[2];
#pragma unroll
        for (int e = 0; e < 2; ++e) {
            const int i = 2 * k + e - off;         // window tap
            v[e] = 0.0f;
            if (i >= 0 && i < a.win_length) {
                long j = j0 + 2 * k + e;
                if constexpr (PROFILE) {
                    const bool outside = j < 0 || j >= n;
                    if (outside && !a.pad_zero) j = j < 0 ? -j : 2 * (n - 1) - j;
                    if (!outside || !a.pad_zero) v[e] = preemph_at(x, j, a.preemph) * scale * a.window[i];
                } else {
                    if (j < 0) j = -j;
                    else if (j >= n) j = 2 * (n - 1) - j;
                    v[e] = x[j] * a.window[i];
                }
            }
        }
        z[rev4(k)] = make_float2(v[0], v[1]);
    }
    // five radix-4 passes, one butterfly per thread and pass; W_4 = -i.  (radix4_1024 of dsp_device.h is this loop as a function; called
    // from here the compiler schedules this kernel differently, so the passes stay inline and the machine code stays what it was.)
#pragma unroll
    for (int s = 0; s < 5; ++s) {
        __syncthreads();
        const int q = 1 << (2 * s);
        const int pos = tid & (q - 1), base = ((tid >> (2 * s)) << (2 * s + 2)) + pos;
        float2 a0 = z[base], a1 = z[base + q], a2 = z[base + 2 * q], a3 = z[base + 3 * q];
        if (s > 0) {
            const int ts = pos * (512 >> (2 * s));   // W_L^pos as an index into the n_fft-point table, L = 4 q
            a1 = cmul(a1, a.twiddle[ts]);
            a2 = cmul(a2, a.twiddle[2 * ts]);
            a3 = cmul(a3, a.twiddle[3 * ts]);
        }
        const float2 s02 = make_float2(a0.x + a2.x, a0.y + a2.y), d02 = make_float2(a0.x - a2.x, a0.y - a2.y);
        const float2 s13 = make_float2(a1.x + a3.x, a1.y + a3.y), d13 = make_float2(a1.x - a3.x, a1.y - a3.y);
        z[base] = make_float2(s02.x + s13.x, s02.y + s13.y);
        z[base + q] = make_float2(d02.x + d13.y, d02.y - d13.x);       // d02 - i d13
        z[base + 2 * q] = make_float2(s02.x - s13.x, s02.y - s13.y);
        z[base + 3 * q] = make_float2(d02.x - d13.y, d02.y + d13.x);   // d02 + i d13
    }
    __syncthreads();
    // split pass: X[k] = E[k] + W^k O[k], X[NC - k] = conj(E[k] - W^k O[k]); only the magnitudes are kept
    for (int k = tid; k <= NC / 2; k += WRNN_MEL_THREADS) {
        if (k == 0) {
            const float2 z0 = z[0];
            const float dc = z0.x + z0.y, ny = z0.x - z0.y;
            const bool p2 = PROFILE && a.power2;
            mag[0] = p2 ? dc * dc : fabsf(dc);
            mag[NC] = p2 ? ny * ny : fabsf(ny);
        } else {
            const float2 zk = z[k], zn = z[NC - k];
            const float2 E = make_float2(0.5f * (zk.x + zn.x), 0.5f * (zk.y - zn.y));
            const float2 O = make_float2(0.5f * (zk.y + zn.y), -0.5f * (zk.x - zn.x));
            const float2 WO = cmul(a.twiddle[k], O);
            const float pr = E.x + WO.x, pi = E.y + WO.y, mr = E.x - WO.x, mi = E.y - WO.y;
            const float pp = pr * pr + pi * pi, mm = mr * mr + mi * mi;
            if (PROFILE && a.power2) {
                mag[k] = pp;
                mag[NC - k] = mm;
            } else {
                mag[k] = sqrtf(pp);
                mag[NC - k] = sqrtf(mm);
            }
        }
    }
    __syncthreads();
    // sparse filterbank: four lanes per mel row, then amp_to_db and normalize
    for (int m0 = 0; m0 < a.n_mels; m0 += WRNN_MEL_THREADS / 4) {
        const int m = m0 + (tid >> 2), sub = tid & 3;
        float acc = 0.0f;
        if (m < a.n_mels) {
            const int first = a.rows[3 * m], nb = a.rows[3 * m + 1];
            const float *w = a.weights + a.rows[3 * m + 2];
            for (int i = sub; i < nb; i += 4) acc += w[i] * mag[first + i];
        }
        acc += __shfl_xor(acc, 1);
        acc += __shfl_xor(acc, 2);
        if (m < a.n_mels && sub == 0) {
            if constexpr (PROFILE) {
                // the floor 10^(min_level_db / 20) is min_level_db exactly, as below; whatever lies under it is clipped to 0 anyway
                const float S = (acc > a.floor_amp ? 20.0f * log10f(acc) : a.min_level_db) - a.ref_level_db;
                float v = (S - a.min_level_db) / -a.min_level_db;
                if (a.max_abs > 0.0f) {
                    // the [-A, A] value Tacotron's preprocessing stores, then wavernn_preprocess.py's map to [0, 1]
                    const float A = a.max_abs, sym = fminf(fmaxf(2.0f * A * v - A, -A), A);
                    v = (sym + A) / (2.0f * A);
                }
                out[(long)m * a.T_max] = fminf(fmaxf(v, 0.0f), 1.0f);
            } else {
                // 20 log10(1e-5) is -100 exactly; log10f of the float nearest to 1e-5 need not round to -5
                const float S = acc > 1e-5f ? 20.0f * log10f(acc) : -100.0f;
                const float v = (S - a.min_level_db) / -a.min_level_db;
                out[(long)m * a.T_max] = fminf(fmaxf(v, 0.0f), 1.0f);
            }
        }
    }
}

}  // namespace

bool wrnn_mel_build_tables(int sample_rate, int win_length, int n_mels, double fmin, double fmax_arg, WrnnMelTables *out) {
    const int N = WRNN_MEL_NFFT;
    const double nyquist = 0.5 * (double)sample_rate, fmax = fmax_arg == 0.0 ? nyquist : fmax_arg;
    if (sample_rate < 1 || win_length < 1 || win_length > N || n_mels < 1 || n_mels > WRNN_MEL_MAX_MELS || !(fmin >= 0.0) || !(fmin < fmax) ||
        !(fmax <= nyquist))
        return false;
    // the shared float64 tables, rounded to float32 once
    const std::vector<double> window = wrnn_dsp::hann_periodic(win_length), twiddle = wrnn_dsp::twiddles(N);
    out->window.assign(window.begin(), window.end());
    out->twiddle.assign(twiddle.begin(), twiddle.end());
    const std::vector<double> basis = wrnn_dsp::slaney_basis(sample_rate, N, n_mels, fmin, fmax_arg);
    out->rows.assign(3 * (size_t)n_mels, 0);
    out->weights.clear();
    for (int i = 0; i < n_mels; ++i) {
        int first = -1, last = -1;
        std::vector<float> row(1 + N / 2, 0.0f);
        for (int k = 0; k <= N / 2; ++k) {
            row[k] = (float)basis[(size_t)i * (1 + N / 2) + k];
            if (row[k] != 0.0f) {
                if (first < 0) first = k;
                last = k;
            }
        }
        out->rows[3 * i] = first < 0 ? 0 : first;
        out->rows[3 * i + 1] = first < 0 ? 0 : last - first + 1;
        out->rows[3 * i + 2] = (int32_t)out->weights.size();
        if (first >= 0) out->weights.insert(out->weights.end(), row.begin() + first, row.begin() + last + 1);
    }
    return true;
}

hipError_t wrnn_launch_melspec(const WrnnMelArgs &a, int B, bool profile, hipStream_t s) {
    const dim3 grid((unsigned)a.T_max, (unsigned)B), block(WRNN_MEL_THREADS);
    if (profile) hipLaunchKernelGGL(melspec_kernel<true>, grid, block, 0, s, a);
    else hipLaunchKernelGGL(melspec_kernel<false>, grid, block, 0, s, a);
    return hipGetLastError();
}

hipError_t wrnn_launch_mel_peak(const float *wav, int64_t n_max, const int32_t *n_samples, int B, float preemph, float *peak, hipStream_t s) {
    hipError_t e = hipMemsetAsync(peak, 0, (size_t)B * sizeof(float), s);
    if (e != hipSuccess) return e;
    const dim3 grid((unsigned)((n_max + PEAK_CHUNK - 1) / PEAK_CHUNK), (unsigned)B);
    hipLaunchKernelGGL(melspec_peak_kernel, grid, dim3(PEAK_THREADS), 0, s, wav, (long)n_max, n_samples, preemph, peak);
    return hipGetLastError();
}
