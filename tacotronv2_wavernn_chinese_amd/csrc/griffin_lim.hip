// Griffin-Lim on the device: [0, 1] mel -> wav with no trained model, the inverse of the mel front end (melspec.hip) in both feature
// profiles.  The chain is inv_mel_spectrogram of tacotron/datasets/audio.py:122-137, 176-186, 203-210, 256-260: undo the normalisation
// and the dB, pseudo-inverse of the filterbank, ** power, n_iter rounds of stft / istft that keep the magnitudes and take the phases of
// the current wave, de-emphasis.  Four plain grid kernels; nothing crosses workgroups, nothing spins, and every sum is a gather in a
// fixed order (no atomics), so two runs give the same bits:
//   griffin_magnitude_kernel  grid (T_max, B)               mel column -> S = max(1e-10, P a) ^ power, n_fft/2 + 1 bins
//   griffin_frame_kernel      grid (T_max, B)               one frame of one round: taps of the wave under the window -> real FFT ->
//                                                           u = X / |X| -> Z = S u -> inverse real FFT -> taps under the window
//   griffin_ola_kernel        grid (ceil(n / 256), B)       overlap-add of the stored taps over the window-sum-square (librosa.istft)
//   deemphasis_kernel         grid (B)                      y[i] = x[i] + k y[i-1], a blocked float64 scan
// The 2048-point real transforms are the 1024-point complex radix-4 transform of melspec.hip (radix4_1024 of dsp_device.h, in float64) with
// its split pass.
// Precision: the mel, the injected phases and the wav are float32; everything between them is float64 -- the pseudo-inverse, the window
// and the twiddles (dsp_tables.h, unrounded; the float32 tables of mel_internal.h are the mel front end's), S, the transforms, the
// stored taps and the wave between rounds.  The rounds are not a contraction: where a bin of the current wave's spectrum comes close to
// zero, u = X / |X| turns a rounding error into a phase error, and a float32 chain was measured to drift from the float64 one by up to
// 150 times its one-round error over 60 rounds.  In float64 the drift stays far under the float32 rounding of the output.
// The C entries of the header's Griffin-Lim section are at the end of this file: a handle of its own like the mel front end's, no weights.
#include <cfloat>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "device_util.h"
#include "dsp_device.h"
#include "dsp_tables.h"
#include "handle_common.h"
#include "mel_internal.h"

namespace {

constexpr int NC = WRNN_MEL_NFFT / 2;   // complex points
constexpr int NB = NC + 1;              // bins
constexpr int THREADS = WRNN_MEL_THREADS;

struct GriffinArgs {
    const float *mel;             // (B, n_mels, T_max) in [0, 1]
    const int32_t *frames;        // [B] frames of every clip (ragged; read as clamped to 0 .. T_max)
    const double *window;         // [win_length]
    const double2 *twiddle;       // [n_fft]  cos, -sin of 2 pi k / n_fft
    const double *pinv_t;         // (n_mels, NB): the pseudo-inverse, transposed so that neighbouring lanes read neighbouring bins
    double *S;                    // (B, T_max, NB) target magnitudes
    float *S_out;                 // the caller's copy of S, or NULL
    double *taps;                 // (B, T_max, win_length) windowed frames of the round
    const double *wave;           // (B, n_wave) the current estimate
    const float *phases;          // (B, T_max, NB) r of the first round's exp(2 pi i r), or NULL
    uint64_t seed;
    int64_t n_wave;
    int32_t T_max, n_mels, hop, win_length, pad_zero, phase_mode, magnitude_power;
    float min_level_db, ref_level_db, max_abs, power;
};

__device__ inline int clip_frames(const GriffinArgs &a, int b) { return min(max(a.frames[b], 0), a.T_max); }

// ---- a. mel -> magnitude ------------------------------------------------------------------------------------------------------------
// Steps 7, 6 and 4 of wrnn_mel_features backwards, then the pseudo-inverse of the filterbank (a dense product, P has both signs), the
// floor and ** power.
__global__ void __launch_bounds__(THREADS) griffin_magnitude_kernel(GriffinArgs a) {
    __shared__ double amp[WRNN_MEL_MAX_MELS];
    const int t = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
    const bool live = t < clip_frames(a, b);        // workgroup-uniform
    const long row = ((long)b * a.T_max + t) * NB;
    if (!live) {
        if (a.S_out)
            for (int k = tid; k < NB; k += THREADS) a.S_out[row + k] = 0.0f;
        return;
    }
    if (tid < a.n_mels) {
        const double m = (double)a.mel[((long)b * a.n_mels + tid) * a.T_max + t], lo = (double)a.min_level_db;
        double S_db;
        if (a.max_abs > 0.0f) {
            const double A = (double)a.max_abs, sym = fmin(fmax(2.0 * A * m - A, -A), A);
            S_db = (sym + A) * -lo / (2.0 * A) + lo;
        } else {
            S_db = fmin(fmax(m, 0.0), 1.0) * -lo + lo;
        }
        const double v = pow(10.0, (S_db + (double)a.ref_level_db) / 20.0);
        amp[tid] = a.magnitude_power == 2 ? sqrt(v) : v;
    }
    __syncthreads();
    for (int k = tid; k < NB; k += THREADS) {
        double acc = 0.0;
        for (int m = 0; m < a.n_mels; ++m) acc = fma(a.pinv_t[(long)m * NB + k], amp[m], acc);
        const double S = pow(fmax(acc, 1e-10), (double)a.power);
        a.S[row + k] = S;
        if (a.S_out) a.S_out[row + k] = (float)S;
    }
}

// ---- b. one frame of one round --------------------------------------------------------------------------------------------------------
// index of the wave that position j of the padded clip reads under reflection: numpy's mode='reflect' for any pad width, the triangle
// wave of period 2 (n - 1)
__device__ inline long reflect_index(long j, long n) {
    if (n == 1) return 0;
    const long period = 2 * (n - 1);
    long m = j % period;
    if (m < 0) m += period;
    return m < n ? m : period - m;
}

__device__ inline double2 unit_phase(double re, double im) {
    const double r = hypot(re, im);                  // no underflow of re^2 + im^2 for a small X
    return r > 0.0 ? make_double2(re / r, im / r) : make_double2(1.0, 0.0);   // np.exp(1j * np.angle(0)) = 1
}

// exp(2 pi i r) of the first round: r drawn by Philox keyed (seed, clip, frame, bin), injected, or 0
__device__ inline double2 first_phase(const GriffinArgs &a, int b, int t, int k) {
    float r = 0.0f;
    if (a.phase_mode == WRNN_GRIFFIN_PHASE_PHILOX) r = wrnn_uniform(a.seed, (uint64_t)t, (uint32_t)b, (uint32_t)k);
    else if (a.phase_mode == WRNN_GRIFFIN_PHASE_INJECTED) r = a.phases[((long)b * a.T_max + t) * NB + k];
    double s, c;
    sincospi(2.0 * (double)r, &s, &c);
    return make_double2(c, s);
}

// FIRST: the phases are first_phase and no wave is read.  Otherwise the frame's taps are gathered from the wave, transformed, and the
// phases are those of the transform.  Either way Z = S u goes through the inverse transform and the win_length taps under the window
// are stored for the overlap-add.  A clip of fewer than two frames has no samples and nothing to do.
template <bool FIRST>
__global__ void __launch_bounds__(THREADS) griffin_frame_kernel(GriffinArgs a) {
    __shared__ double2 z[NC];         // 16 KiB: the forward transform, in place
    __shared__ double2 y[NC];         // 16 KiB: the inverse transform, in place
    const int t = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
    const int T_b = clip_frames(a, b);
    if (t >= T_b || T_b < 2) return;  // workgroup-uniform
    const int off = (WRNN_MEL_NFFT - a.win_length) / 2;
    const double *S = a.S + ((long)b * a.T_max + t) * NB;
    if constexpr (!FIRST) {
        const long n = (long)a.hop * (T_b - 1);
        const double *x = a.wave + (long)b * a.n_wave;
        const long j0 = (long)t * a.hop - NC;          // wave index of frame sample 0
        for (int k = tid; k < NC; k += THREADS) {
            double v[2];
#pragma unroll
            for (int e = 0; e < 2; ++e) {
                const int i = 2 * k + e - off;         // window tap
                v[e] = 0.0;
                if (i >= 0 && i < a.win_length) {
                    const long j = j0 + 2 * k + e;
                    const bool outside = j < 0 || j >= n;
                    if (!outside) v[e] = x[j] * a.window[i];
                    else if (!a.pad_zero) v[e] = x[reflect_index(j, n)] * a.window[i];
                }
            }
            z[rev4(k)] = make_double2(v[0], v[1]);
        }
        radix4_1024(z, a.twiddle, tid);
    }
    // Split pass, projection and the inverse split pass, one pair of bins (k, NC - k) per step.  Forward: X[k] = E + W^k O,
    // X[NC - k] = conj(E - W^k O).  Backward, for the spectrum Z: E' = (Z[k] + conj(Z[NC - k])) / 2, O' = conj(W^k) (Z[k] - conj(Z[NC - k])) / 2,
    // and the complex input of the half-length transform is C[k] = E' + i O', C[NC - k] = conj(E') + i conj(O').  The inverse transform
    // is the conjugate of the forward one on the conjugated input, so conj(C) is what is stored, digit-reversed.
    for (int k = tid; k <= NC / 2; k += THREADS) {
        if (k == 0) {
            double z0, zn;
            if constexpr (FIRST) {
                // irfft reads the real parts of the two real bins only
                z0 = S[0] * first_phase(a, b, t, 0).x;
                zn = S[NC] * first_phase(a, b, t, NC).x;
            } else {
                const double2 c = z[0];
                z0 = c.x + c.y < 0.0 ? -S[0] : S[0];
                zn = c.x - c.y < 0.0 ? -S[NC] : S[NC];
            }
            y[0] = make_double2(0.5 * (z0 + zn), -0.5 * (z0 - zn));
        } else {
            const double2 W = a.twiddle[k];
            double2 uk, un;
            if constexpr (FIRST) {
                uk = first_phase(a, b, t, k);
                un = first_phase(a, b, t, NC - k);
            } else {
                const double2 zk = z[k], zm = z[NC - k];
                const double2 E = make_double2(0.5 * (zk.x + zm.x), 0.5 * (zk.y - zm.y));
                const double2 O = make_double2(0.5 * (zk.y + zm.y), -0.5 * (zk.x - zm.x));
                const double2 WO = cmul(W, O);
                uk = unit_phase(E.x + WO.x, E.y + WO.y);
                un = unit_phase(E.x - WO.x, -(E.y - WO.y));
            }
            const double sk = S[k], sn = S[NC - k];
            const double2 Zk = make_double2(sk * uk.x, sk * uk.y), Zn = make_double2(sn * un.x, sn * un.y);
            const double2 Ei = make_double2(0.5 * (Zk.x + Zn.x), 0.5 * (Zk.y - Zn.y));
            const double2 D = make_double2(0.5 * (Zk.x - Zn.x), 0.5 * (Zk.y + Zn.y));
            const double2 Oi = cmul(make_double2(W.x, -W.y), D);
            // C[k] = Ei + i Oi = (Ei.x - Oi.y, Ei.y + Oi.x); C[NC - k] = conj(Ei) + i conj(Oi) = (Ei.x + Oi.y, Oi.x - Ei.y)
            y[rev4(k)] = make_double2(Ei.x - Oi.y, -(Ei.y + Oi.x));
            y[rev4(NC - k)] = make_double2(Ei.x + Oi.y, -(Oi.x - Ei.y));
        }
    }
    radix4_1024(y, a.twiddle, tid);
    // frame sample 2 n = Re conj(y[n]) / NC, sample 2 n + 1 = Im conj(y[n]) / NC
    double *out = a.taps + ((long)b * a.T_max + t) * a.win_length;
    const double scale = 1.0 / (double)NC;
    for (int i = tid; i < a.win_length; i += THREADS) {
        const int s = i + off;
        const double2 c = y[s >> 1];
        out[i] = ((s & 1) ? -c.y : c.x) * scale * a.window[i];
    }
}

// ---- c. overlap-add -------------------------------------------------------------------------------------------------------------------
// Output sample n of a clip of T frames sits at position p = n + n_fft/2 of the padded signal; frame t covers it with its tap
// p - t hop - off.  The taps and the squares of the window are summed in ascending frame order.
// OUT: double for the wave the next round (or the de-emphasis) reads, float for the caller's buffer.
template <typename OUT>
__global__ void __launch_bounds__(THREADS) griffin_ola_kernel(GriffinArgs a, OUT *out, long n_out_max) {
    const int b = blockIdx.y;
    const long n = (long)blockIdx.x * THREADS + threadIdx.x;
    if (n >= n_out_max) return;
    const int T_b = clip_frames(a, b);
    double v = 0.0;
    if (n < (long)a.hop * (T_b - 1)) {
        const int off = (WRNN_MEL_NFFT - a.win_length) / 2;
        const long q = n + NC - off;                               // tap index in frame 0
        long t_lo = q - a.win_length + 1 <= 0 ? 0 : (q - a.win_length + a.hop) / a.hop;   // ceil((q - win + 1) / hop)
        long t_hi = q / a.hop;
        if (t_hi > T_b - 1) t_hi = T_b - 1;
        const double *taps = a.taps + (long)b * a.T_max * a.win_length;
        double acc = 0.0, wss = 0.0;
        for (long t = t_lo; t <= t_hi; ++t) {
            const int i = (int)(q - t * a.hop);
            const double w = a.window[i];
            acc += taps[t * a.win_length + i];
            wss = fma(w, w, wss);
        }
        v = wss > (double)FLT_MIN ? acc / wss : acc;
    }
    out[(long)b * n_out_max + n] = (OUT)v;
}

// ---- d. de-emphasis -------------------------------------------------------------------------------------------------------------------
// y[i] = x[i] + k y[i-1] in float64, one workgroup per clip walking tiles of THREADS * DE_PER samples: every thread runs its DE_PER
// samples from a zero start (thread 0 from the carry of the tile in front), a Hillis-Steele pass over the threads' last values gives
// each thread the y in front of its run, which enters its samples with the powers of k.  Fixed order: the same bits on every run.
constexpr int DE_PER = 8, DE_TILE = THREADS * DE_PER;

// IN: float for the public entry's clips, double for the wave of the last round.
template <typename IN>
__global__ void __launch_bounds__(THREADS) deemphasis_kernel(const IN *in, long in_stride, const int32_t *n_dev, int frames_hop, double k,
                                                             float *out, long out_stride) {
    __shared__ double last[2][THREADS];
    const int b = blockIdx.x, tid = threadIdx.x;
    long n = n_dev[b];
    if (frames_hop > 0) n = (long)frames_hop * (n - 1);    // n_dev holds frame counts: the clip has hop (T - 1) samples
    n = n < 0 ? 0 : n > in_stride ? in_stride : n;
    if (n > out_stride) n = out_stride;
    const IN *x = in + (long)b * in_stride;
    float *y = out + (long)b * out_stride;
    double kp[DE_PER + 1];                                 // k^e
    kp[0] = 1.0;
#pragma unroll
    for (int e = 1; e <= DE_PER; ++e) kp[e] = kp[e - 1] * k;
    double carry = 0.0;
    for (long base = 0; base < n; base += DE_TILE) {
        const long i0 = base + (long)tid * DE_PER;
        double v[DE_PER], prev = tid == 0 ? carry : 0.0;
#pragma unroll
        for (int e = 0; e < DE_PER; ++e) {
            const double xe = i0 + e < n ? (double)x[i0 + e] : 0.0;
            prev = v[e] = fma(k, prev, xe);
        }
        int cur = 0;
        last[0][tid] = prev;
        double f = kp[DE_PER];                              // k^(DE_PER d) of the pass with distance d
        for (int d = 1; d < THREADS; d <<= 1) {
            __syncthreads();
            const double mine = last[cur][tid];
            last[cur ^ 1][tid] = tid >= d ? fma(f, last[cur][tid - d], mine) : mine;
            cur ^= 1;
            f *= f;
        }
        __syncthreads();
        const double before = tid > 0 ? last[cur][tid - 1] : 0.0;   // y[i0 - 1]; thread 0 started from the carry itself
        carry = last[cur][THREADS - 1];
#pragma unroll
        for (int e = 0; e < DE_PER; ++e)
            if (i0 + e < n) y[i0 + e] = (float)fma(kp[e + 1], before, v[e]);
        __syncthreads();                                    // `last` is written again by the next tile
    }
    for (long i = n + tid; i < out_stride; i += THREADS) y[i] = 0.0f;
}

template <typename IN>
hipError_t launch_deemphasis(const IN *in, long in_stride, const int32_t *n_dev, int frames_hop, int B, double k, float *out, long out_stride,
                             hipStream_t s) {
    hipLaunchKernelGGL(deemphasis_kernel<IN>, dim3((unsigned)B), dim3(THREADS), 0, s, in, in_stride, n_dev, frames_hop, k, out, out_stride);
    return hipGetLastError();
}

// ---- host tables (the basis, the window and the twiddles are dsp_tables.h's, unrounded) -----------------------------------------------
// P = B^T (B B^T)^-1 of a basis of full row rank, (NB, n) row-major, by a Cholesky factorisation of the n x n Gram matrix.
// 0: done; 1: an empty filterbank row; 2: the Gram matrix is not positive definite.
int pseudo_inverse(const std::vector<double> &basis, int n, std::vector<double> *P) {
    for (int i = 0; i < n; ++i) {
        bool any = false;
        for (int k = 0; k < NB && !any; ++k) any = basis[(size_t)i * NB + k] != 0.0;
        if (!any) return 1;
    }
    std::vector<double> L((size_t)n * n, 0.0);
    for (int i = 0; i < n; ++i)
        for (int j = 0; j <= i; ++j) {
            double g = 0.0;
            for (int k = 0; k < NB; ++k) g += basis[(size_t)i * NB + k] * basis[(size_t)j * NB + k];
            L[(size_t)i * n + j] = g;
        }
    for (int j = 0; j < n; ++j) {
        double d = L[(size_t)j * n + j];
        for (int m = 0; m < j; ++m) d -= L[(size_t)j * n + m] * L[(size_t)j * n + m];
        if (!(d > 0.0) || !std::isfinite(d)) return 2;
        d = std::sqrt(d);
        L[(size_t)j * n + j] = d;
        for (int i = j + 1; i < n; ++i) {
            double v = L[(size_t)i * n + j];
            for (int m = 0; m < j; ++m) v -= L[(size_t)i * n + m] * L[(size_t)j * n + m];
            L[(size_t)i * n + j] = v / d;
        }
    }
    // column k of the basis is one right-hand side of (L L^T) x = B[:, k]; x is row k of P
    P->assign((size_t)NB * n, 0.0);
    std::vector<double> x(n);
    for (int k = 0; k < NB; ++k) {
        for (int i = 0; i < n; ++i) {
            double v = basis[(size_t)i * NB + k];
            for (int m = 0; m < i; ++m) v -= L[(size_t)i * n + m] * x[m];
            x[i] = v / L[(size_t)i * n + i];
        }
        for (int i = n - 1; i >= 0; --i) {
            double v = x[i];
            for (int m = i + 1; m < n; ++m) v -= L[(size_t)m * n + i] * x[m];
            x[i] = v / L[(size_t)i * n + i];
        }
        for (int i = 0; i < n; ++i) (*P)[(size_t)k * n + i] = x[i];
    }
    return 0;
}

}  // namespace

// ---- the C entries ----------------------------------------------------------------------------------------------------------------------

struct wrnn_griffin_handle {
    wrnn_mel_config cfg{};
    wrnn_mel_features feat{};
    wrnn_griffin_config gcfg{};
    WrnnMelTables tab;                // the float32 window of the tables entry; empty while the configuration is refused
    std::vector<double> window;       // [win_length] the periodic Hann window the kernels read, unrounded
    std::vector<double> pinv;         // (NB, n_mels) the pseudo-inverse, unrounded
    void *dev = nullptr;              // window | twiddle | pinv transposed, all float64, uploaded by the first call
    size_t o_tw = 0, o_p = 0;
    WrnnScratch ws;                   // S | taps | wave, grown on demand
    std::string err;
};

extern "C" {

int wrnn_griffin_create(const wrnn_mel_config *cfg, const wrnn_mel_features *f, const wrnn_griffin_config *g, wrnn_griffin_handle **out) {
    if (!cfg || !f || !g || !out) return WRNN_ERR_INVALID;
    wrnn_griffin_handle *h = new wrnn_griffin_handle();
    *out = h;
    h->cfg = *cfg;
    if (f->struct_size != sizeof(wrnn_mel_features))
        return wrnn_failf(h, WRNN_ERR_INVALID, "features.struct_size = %u, this library's wrnn_mel_features has %zu bytes", f->struct_size, sizeof(wrnn_mel_features));
    if (g->struct_size != sizeof(wrnn_griffin_config))
        return wrnn_failf(h, WRNN_ERR_INVALID, "griffin.struct_size = %u, this library's wrnn_griffin_config has %zu bytes", g->struct_size, sizeof(wrnn_griffin_config));
    h->feat = *f;
    h->gcfg = *g;
    if (const int rc = wrnn_mel_check(h, cfg, f, "Griffin-Lim")) return rc;
    if (!(g->power > 0.0f) || !std::isfinite(g->power) || g->n_iter_default < 0)
        return wrnn_failf(h, WRNN_ERR_INVALID, "bad griffin configuration: power is finite and > 0, n_iter_default >= 0");
    WrnnMelTables tab;
    if (!wrnn_mel_build_tables(cfg->sample_rate, cfg->win_length, cfg->n_mels, (double)cfg->fmin, (double)f->fmax, &tab))
        return wrnn_failf(h, WRNN_ERR_INVALID, "bad configuration: 1 <= win_length <= n_fft, 1 <= n_mels <= %d, 0 <= fmin < sample_rate / 2", WRNN_MEL_MAX_MELS);
    std::vector<double> P;
    const int rc = pseudo_inverse(wrnn_dsp::slaney_basis(cfg->sample_rate, WRNN_MEL_NFFT, cfg->n_mels, (double)cfg->fmin, (double)f->fmax), cfg->n_mels, &P);
    if (rc == 1) return wrnn_failf(h, WRNN_ERR_UNSUPPORTED, "a filterbank row is empty (n_mels = %d over this band is finer than the bins): the mel cannot be inverted", cfg->n_mels);
    if (rc == 2) return wrnn_failf(h, WRNN_ERR_UNSUPPORTED, "the filterbank has no full row rank (the Cholesky factorisation of its Gram matrix failed)");
    h->pinv = std::move(P);
    h->window = wrnn_dsp::hann_periodic(cfg->win_length);   // unrounded, where wrnn_mel_build_tables rounds it to float32
    h->tab = std::move(tab);
    return WRNN_OK;
}

int64_t wrnn_griffin_samples(const wrnn_griffin_handle *h, int64_t frames) {
    if (!h || h->tab.window.empty() || frames < 1 || frames > INT32_MAX) return WRNN_ERR_INVALID;
    return (int64_t)h->cfg.hop_length * (frames - 1);
}

int wrnn_griffin_tables(const wrnn_griffin_handle *h, float *pinv, float *window, int32_t frames, float *window_sumsquare) {
    if (!h || h->tab.window.empty() || (window_sumsquare && frames < 1)) return WRNN_ERR_INVALID;
    if (pinv)
        for (size_t i = 0; i < h->pinv.size(); ++i) pinv[i] = (float)h->pinv[i];
    if (window)
        for (size_t i = 0; i < h->window.size(); ++i) window[i] = (float)h->window[i];
    if (window_sumsquare) {
        // position p of the padded signal, as the overlap-add kernel sums it in float64: ascending frames, one fused multiply-add each
        const int win = h->cfg.win_length, hop = h->cfg.hop_length, off = (WRNN_MEL_NFFT - win) / 2;
        const int64_t len = WRNN_MEL_NFFT + (int64_t)hop * (frames - 1);
        for (int64_t p = 0; p < len; ++p) {
            double wss = 0.0;
            for (int64_t t = 0; t < frames; ++t) {
                const int64_t i = p - t * hop - off;
                if (i >= 0 && i < win) wss = std::fma(h->window[i], h->window[i], wss);
            }
            window_sumsquare[p] = (float)wss;
        }
    }
    return WRNN_OK;
}

int wrnn_deemphasis(const float *wav_dev, int64_t n_max, const int32_t *n_dev, int32_t B, double k, float *out_dev, void *stream) {
    if (!wav_dev || !n_dev || !out_dev || n_max < 1 || B < 1 || B > WRNN_MAX_GRID_Y || !std::isfinite(k) || !(std::fabs(k) < 1.0)) return WRNN_ERR_INVALID;
    return launch_deemphasis(wav_dev, (long)n_max, n_dev, 0, B, k, out_dev, (long)n_max, (hipStream_t)stream) == hipSuccess ? WRNN_OK : WRNN_ERR_HIP;
}

int wrnn_griffin_lim(wrnn_griffin_handle *h, const float *mel_dev, const int32_t *frames_dev, int32_t B, int32_t T_max, int32_t n_iter,
                     int32_t phase_mode, uint64_t seed, const float *phases_dev, float *wav_out_dev, int64_t n_out_max,
                     float *magnitude_out_dev, void *stream) {
    if (!h) return WRNN_ERR_INVALID;
    if (h->tab.window.empty()) return wrnn_failf(h, WRNN_ERR_STATE, "the handle's configuration was refused by wrnn_griffin_create");
    if (n_iter < 0) n_iter = h->gcfg.n_iter_default;
    const int64_t n_wave = (int64_t)h->cfg.hop_length * (T_max - 1);
    if (!mel_dev || !frames_dev || !wav_out_dev || B < 1 || B > WRNN_MAX_GRID_Y || T_max < 1 || T_max > 65535 * 32 || n_out_max < 1 || n_out_max < n_wave ||
        n_out_max >= ((int64_t)1 << 31) * THREADS)
        return wrnn_failf(h, WRNN_ERR_INVALID, "bad arguments: device pointers, 1 <= B <= 65535, T_max >= 1, n_out_max >= max(1, hop (T_max - 1))");
    if (phase_mode != WRNN_GRIFFIN_PHASE_ZERO && phase_mode != WRNN_GRIFFIN_PHASE_PHILOX && phase_mode != WRNN_GRIFFIN_PHASE_INJECTED)
        return wrnn_failf(h, WRNN_ERR_INVALID, "phase_mode %d is none of WRNN_GRIFFIN_PHASE_ZERO, _PHILOX, _INJECTED", phase_mode);
    if ((phase_mode == WRNN_GRIFFIN_PHASE_INJECTED) != (phases_dev != nullptr))
        return wrnn_failf(h, WRNN_ERR_INVALID, "phases_dev goes with WRNN_GRIFFIN_PHASE_INJECTED, and with that mode only");
    hipStream_t s = (hipStream_t)stream;
    WRNN_TRY(h, hipSetDevice(h->cfg.device));
    const int n_mels = h->cfg.n_mels, win = h->cfg.win_length;
    if (!h->dev) {
        WrnnImage img;
        img.put(h->window.data(), h->window.size() * 8);
        const std::vector<double> tw = wrnn_dsp::twiddles(WRNN_MEL_NFFT);
        h->o_tw = img.put(tw.data(), tw.size() * 8);
        h->o_p = img.take(h->pinv.size() * 8);
        double *pt = img.at<double>(h->o_p);
        for (int k = 0; k < NB; ++k)
            for (int m = 0; m < n_mels; ++m) pt[(size_t)m * NB + k] = h->pinv[(size_t)k * n_mels + m];
        const hipError_t e = img.upload(&h->dev);
        if (e != hipSuccess) return wrnn_failf(h, WRNN_ERR_HIP, "uploading the Griffin-Lim tables: %s", hipGetErrorString(e));
    }
    // S | taps | wave: the calls on one handle share them, so the caller orders those calls (one stream at a time)
    const size_t n_S = wrnn_up256((size_t)B * T_max * NB * 8) / 8, n_taps = wrnn_up256((size_t)B * T_max * win * 8) / 8;
    const size_t n_ws = n_S + n_taps + wrnn_up256((size_t)B * (size_t)(n_wave > 0 ? n_wave : 1) * 8) / 8;
    WRNN_TRY(h, h->ws.reserve(n_ws * 8, s));
    double *ws = (double *)h->ws.p;
    GriffinArgs a{};
    const char *d = (const char *)h->dev;
    a.mel = mel_dev; a.frames = frames_dev;
    a.window = (const double *)d; a.twiddle = (const double2 *)(d + h->o_tw); a.pinv_t = (const double *)(d + h->o_p);
    a.S = ws; a.S_out = magnitude_out_dev; a.taps = ws + n_S;
    double *wave = ws + n_S + n_taps;
    a.wave = wave; a.n_wave = n_wave > 0 ? n_wave : 1;
    a.phases = phases_dev; a.seed = seed; a.phase_mode = phase_mode;
    a.T_max = T_max; a.n_mels = n_mels; a.hop = h->cfg.hop_length; a.win_length = win;
    a.pad_zero = h->feat.pad_mode == WRNN_MEL_PAD_ZERO; a.magnitude_power = h->feat.magnitude_power;
    a.min_level_db = h->cfg.min_level_db; a.ref_level_db = h->feat.ref_level_db; a.max_abs = h->feat.max_abs_value; a.power = h->gcfg.power;
    const dim3 fgrid((unsigned)T_max, (unsigned)B), block(THREADS);
    hipLaunchKernelGGL(griffin_magnitude_kernel, fgrid, block, 0, s, a);
    WRNN_TRY(h, hipGetLastError());
    const double k = (double)h->feat.preemphasis;
    for (int it = 0; it <= n_iter; ++it) {
        if (it == 0) hipLaunchKernelGGL(griffin_frame_kernel<true>, fgrid, block, 0, s, a);
        else hipLaunchKernelGGL(griffin_frame_kernel<false>, fgrid, block, 0, s, a);
        WRNN_TRY(h, hipGetLastError());
        // the last overlap-add writes the caller's buffer itself (zeros past every clip's end) unless the de-emphasis follows
        const bool to_caller = it == n_iter && k == 0.0;
        const long dst_n = to_caller ? (long)n_out_max : (long)a.n_wave;
        const dim3 ogrid((unsigned)((dst_n + THREADS - 1) / THREADS), (unsigned)B);
        if (to_caller) hipLaunchKernelGGL(griffin_ola_kernel<float>, ogrid, block, 0, s, a, wav_out_dev, dst_n);
        else hipLaunchKernelGGL(griffin_ola_kernel<double>, ogrid, block, 0, s, a, wave, dst_n);
        WRNN_TRY(h, hipGetLastError());
    }
    if (k != 0.0) WRNN_TRY(h, launch_deemphasis(wave, (long)a.n_wave, frames_dev, h->cfg.hop_length, B, k, wav_out_dev, (long)n_out_max, s));
    return WRNN_OK;
}

const char *wrnn_griffin_last_error(const wrnn_griffin_handle *h) { return wrnn_last_error_of(h); }

void wrnn_griffin_destroy(wrnn_griffin_handle *h) {
    if (!h) return;
    if (h->dev || h->ws.p) {
        (void)hipSetDevice(h->cfg.device);
        if (h->dev) (void)hipFree(h->dev);
        h->ws.release();
    }
    delete h;
}

}  // extern "C"
