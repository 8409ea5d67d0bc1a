// Pitch on the device: a YIN F0 track of float32 clips and the F0 / voicing error scores of a test clip against a target clip.  The
// definitions are in the header's section.  Plain grid kernels; nothing crosses workgroups, nothing spins, no floating-point atomics,
// every sum in a fixed order:
//   pitch_track_kernel    grid (T_max, B, clips of a pair)   one workgroup per (clip, frame): the frame to LDS once, the lags dealt
//                                                            over the threads, then one wave for the normalisation, the search and the parabola
//   pitch_pair_kernel     grid (ceil(T_max / 256), B)        the per-frame cents of a pair
//   pitch_summary_kernel  grid (B)                           the two tracks of a pair -> its WRNN_PITCH_FIELDS summaries
// Precision: the samples are float32; every operation on them is float64 (a threshold decision on a float32 difference function flips
// too easily), and f0 and the aperiodicity are rounded to float32 once.  The summaries are float64 from those float32 tracks.
// Order: d(tau) is four chains over j = c mod 4, added as (c0 + c1) + (c2 + c3); the running sum under d' is a 64-wide scan per block of
// 64 lags plus the carry of the blocks before it.  Both depend on (tau, j) alone, never on B, the clip's place in the batch or the grid,
// so a clip of a ragged batch gives the bits of the call on it alone.  The target and the test of a pair are two workgroups of the same
// kernel (blockIdx.z), so identical clips give identical tracks and score exactly 0.
// LDS per workgroup: the frame and (tau_max + 3) doubles: 11 KiB at the defaults (lags 37 .. 367, frame 2048), 48 KiB at the limit.
// Reading x[j .. j + 3] is one 16-byte broadcast, x[j + tau] is consecutive across the lanes: no bank conflicts.
#include <climits>
#include <cmath>
#include <cstring>
#include <string>

#include "dsp_device.h"
#include "handle_common.h"

namespace {

constexpr int THREADS = 256;

struct PitchTrackArgs {
    const float *src[2];          // the clips of blockIdx.z = 0, 1; row stride n_max
    float *f0[2], *ap[2];         // row stride `stride`; ap may be NULL
    const int32_t *n_samples;     // [B]
    int64_t n_max, stride;
    int32_t T_max, hop, frame_length, window, tau_min, tau_max;
    double sample_rate, threshold, silence_rms;
};

// The clip's own length as every kernel here reads it: clamped to the buffer, 0 for anything below 1.
__device__ inline long clip_len(const int32_t *n_samples, int b, long n_max) {
    long n = n_samples[b];
    if (n > n_max) n = n_max;
    return n > 0 ? n : 0;
}

// sum_{j < W} (x[j] - x[j + tau])^2, or sum_j x[j]^2 with ENERGY: four chains, j = c mod 4, in ascending j each.  x is 16-byte aligned:
// the four x[j] of a step are one broadcast read; the loop has no branch, so the reads of a step are in flight together.
template <bool ENERGY>
__device__ inline double lag_sum(const float *x, int tau, int W) {
    double c0 = 0.0, c1 = 0.0, c2 = 0.0, c3 = 0.0;
    const float *y = x + tau;
    int j = 0;
    for (; j + 3 < W; j += 4) {
        const float4 a = *(const float4 *)(x + j);
        const double e0 = ENERGY ? (double)a.x : (double)a.x - (double)y[j];
        const double e1 = ENERGY ? (double)a.y : (double)a.y - (double)y[j + 1];
        const double e2 = ENERGY ? (double)a.z : (double)a.z - (double)y[j + 2];
        const double e3 = ENERGY ? (double)a.w : (double)a.w - (double)y[j + 3];
        c0 = fma(e0, e0, c0);
        c1 = fma(e1, e1, c1);
        c2 = fma(e2, e2, c2);
        c3 = fma(e3, e3, c3);
    }
    if (j < W) {
        const double e = ENERGY ? (double)x[j] : (double)x[j] - (double)y[j];
        c0 = fma(e, e, c0);
    }
    if (j + 1 < W) {
        const double e = ENERGY ? (double)x[j + 1] : (double)x[j + 1] - (double)y[j + 1];
        c1 = fma(e, e, c1);
    }
    if (j + 2 < W) {
        const double e = ENERGY ? (double)x[j + 2] : (double)x[j + 2] - (double)y[j + 2];
        c2 = fma(e, e, c2);
    }
    return (c0 + c1) + (c2 + c3);
}

__global__ void __launch_bounds__(THREADS) pitch_track_kernel(PitchTrackArgs g) {
    extern __shared__ float4 smem[];        // the frame (a multiple of 16 bytes), then the doubles
    const int n_d = g.tau_max + 3;          // d(0 .. tau_max + 1), then the window's energy
    float *x = (float *)smem;
    double *dd = (double *)(x + g.frame_length);
    const int tid = threadIdx.x, t = blockIdx.x, b = blockIdx.y, sig = blockIdx.z;
    const long n = clip_len(g.n_samples, b, g.n_max);
    const int T_b = n > 0 ? (int)(1 + n / g.hop) : 0;
    float *f0_out = g.f0[sig] + (long)b * g.stride, *ap_out = g.ap[sig] ? g.ap[sig] + (long)b * g.stride : nullptr;
    if (t >= T_b) {                         // workgroup-uniform
        if (tid == 0) {
            f0_out[t] = 0.0f;
            if (ap_out) ap_out[t] = 0.0f;
        }
        return;
    }
    const float *src = g.src[sig] + (long)b * g.n_max;
    const long j0 = (long)t * g.hop - g.frame_length / 2;
    for (int i = tid; i < g.frame_length; i += THREADS) {
        const long j = j0 + i;
        x[i] = j >= 0 && j < n ? src[j] : 0.0f;
    }
    __syncthreads();
    // the lags, dealt over the threads; j + tau <= window + tau_max < frame_length
    for (int i = tid; i < n_d - 1; i += THREADS) dd[i] = lag_sum<false>(x, i, g.window);
    if (tid == (n_d - 1) % THREADS) dd[n_d - 1] = lag_sum<true>(x, 0, g.window);    // the thread the next lag would go to
    __syncthreads();
    const int lane = tid & 63;
    // d -> d' in place: blocks of 64 lags, an inclusive scan in the wave, the carry of the blocks before
    if (tid < 64) {
        double carry = 0.0;
        for (int base = 1; base <= g.tau_max + 1; base += 64) {
            const int tau = base + lane;
            const bool in = tau <= g.tau_max + 1;
            const double d = in ? dd[tau] : 0.0;
            double s = d;
            for (int o = 1; o < 64; o <<= 1) {
                const double u = __shfl_up(s, o);
                if (lane >= o) s += u;
            }
            s += carry;
            carry = __shfl(s, 63);
            if (in) dd[tau] = s > 0.0 ? d * (double)tau / s : 1.0;
        }
        if (lane == 0) dd[0] = 1.0;
    }
    __syncthreads();
    if (tid < 64) {
        double mn = INFINITY;
        int first = INT_MAX;
        for (int tau = g.tau_min + lane; tau <= g.tau_max; tau += 64) {
            const double v = dd[tau];
            mn = fmin(mn, v);
            if (v < g.threshold && tau < first) first = tau;
        }
        for (int o = 32; o > 0; o >>= 1) {
            mn = fmin(mn, __shfl_xor(mn, o));
            const int f = __shfl_xor(first, o);
            first = f < first ? f : first;
        }
        if (lane == 0) {
            float f0 = 0.0f;
            if (first != INT_MAX) {
                int tau = first;
                while (tau + 1 <= g.tau_max && dd[tau + 1] < dd[tau]) ++tau;
                const double rms = sqrt(dd[n_d - 1] / (double)g.window);
                if (rms >= g.silence_rms) {
                    const double a = dd[tau - 1], bb = dd[tau], c = dd[tau + 1];
                    const double den = a - 2.0 * bb + c;
                    double off = den > 0.0 ? 0.5 * (a - c) / den : 0.0;
                    off = off < -0.5 ? -0.5 : off > 0.5 ? 0.5 : off;
                    f0 = (float)(g.sample_rate / ((double)tau + off));
                }
            }
            f0_out[t] = f0;
            if (ap_out) ap_out[t] = (float)mn;
        }
    }
}

struct PitchPairArgs {
    const float *frames;          // f0_t | ap_t | f0_s | ap_s | cents, every segment T_max long
    float *cents;                 // the fifth segment of row 0
    const int32_t *n_samples;
    double *summary;              // (B, WRNN_PITCH_FIELDS)
    int64_t n_max, stride;
    int32_t T_max, hop;
    double gpe_ratio;
};

__global__ void __launch_bounds__(THREADS) pitch_pair_kernel(PitchPairArgs g) {
    const int t = blockIdx.x * THREADS + threadIdx.x, b = blockIdx.y;
    if (t >= g.T_max) return;
    const long n = clip_len(g.n_samples, b, g.n_max);
    const int T_b = n > 0 ? (int)(1 + n / g.hop) : 0;
    const float *row = g.frames + (long)b * g.stride;
    const float ft = row[t], fs = row[2L * g.T_max + t];
    float c = 0.0f;
    if (t < T_b && ft > 0.0f && fs > 0.0f) c = (float)(1200.0 * log2((double)fs / (double)ft));
    g.cents[(long)b * g.stride + t] = c;
}

// One workgroup per pair.  Thread i takes frames i, i + 256, ... in ascending order, then the threads are added in a fixed tree: the
// order depends on a frame's index alone.  Two passes: the counts, the squared cents and the means of log2 f0, then the central moments.
__global__ void __launch_bounds__(THREADS) pitch_summary_kernel(PitchPairArgs g) {
    __shared__ double acc[8 * THREADS];
    const int tid = threadIdx.x, b = blockIdx.x;
    const long n = clip_len(g.n_samples, b, g.n_max);
    const int T_b = n > 0 ? (int)(1 + n / g.hop) : 0;
    const float *ft_row = g.frames + (long)b * g.stride, *fs_row = ft_row + 2L * g.T_max;
    double n_t = 0.0, n_s = 0.0, n_v = 0.0, n_vde = 0.0, n_gpe = 0.0, c2 = 0.0, lt = 0.0, ls = 0.0;
    for (int t = tid; t < T_b; t += THREADS) {
        const double ft = (double)ft_row[t], fs = (double)fs_row[t];
        const bool vt = ft > 0.0, vs = fs > 0.0;
        n_t += vt ? 1.0 : 0.0;
        n_s += vs ? 1.0 : 0.0;
        n_vde += vt != vs ? 1.0 : 0.0;
        if (vt && vs) {
            const double ratio = fs / ft, c = 1200.0 * log2(ratio);
            n_v += 1.0;
            n_gpe += fabs(ratio - 1.0) > g.gpe_ratio ? 1.0 : 0.0;
            c2 += c * c;
            lt += log2(ft);
            ls += log2(fs);
        }
    }
    double first[8] = {n_t, n_s, n_v, n_vde, n_gpe, c2, lt, ls};
    block_sums<THREADS>(first, acc);
    n_t = first[0]; n_s = first[1]; n_v = first[2]; n_vde = first[3]; n_gpe = first[4]; c2 = first[5]; lt = first[6]; ls = first[7];
    const double mt = n_v > 0.0 ? lt / n_v : 0.0, ms = n_v > 0.0 ? ls / n_v : 0.0;
    double cov = 0.0, var_t = 0.0, var_s = 0.0;
    for (int t = tid; t < T_b; t += THREADS) {
        const double ft = (double)ft_row[t], fs = (double)fs_row[t];
        if (ft > 0.0 && fs > 0.0) {
            const double a = log2(ft) - mt, c = log2(fs) - ms;
            cov += a * c;
            var_t += a * a;
            var_s += c * c;
        }
    }
    double second[3] = {cov, var_t, var_s};
    block_sums<THREADS>(second, acc);
    cov = second[0]; var_t = second[1]; var_s = second[2];
    if (tid != 0) return;
    double *o = g.summary + (long)b * WRNN_PITCH_FIELDS;
    for (int i = 0; i < WRNN_PITCH_FIELDS; ++i) o[i] = 0.0;
    if (T_b == 0) return;
    const double T = (double)T_b;
    if (n_v > 0.0) {
        o[WRNN_PITCH_F0_RMSE_CENTS] = sqrt(c2 / n_v);
        o[WRNN_PITCH_GPE] = n_gpe / n_v;
    }
    o[WRNN_PITCH_VDE] = n_vde / T;
    o[WRNN_PITCH_FFE] = (n_gpe + n_vde) / T;
    if (n_v >= 2.0 && var_t > 0.0 && var_s > 0.0) o[WRNN_PITCH_F0_CORR] = cov / sqrt(var_t * var_s);
    o[WRNN_PITCH_VOICED_TARGET] = n_t;
    o[WRNN_PITCH_VOICED_TEST] = n_s;
    o[WRNN_PITCH_VOICED_BOTH] = n_v;
}

}  // namespace

// ---- the C entries ----------------------------------------------------------------------------------------------------------------------

struct wrnn_pitch_handle {
    wrnn_pitch_config cfg{};
    bool ok = false;                  // false while the configuration is refused
    int tau_min = 0, tau_max = 0;
    WrnnScratch ws;                   // the per-frame rows of a score call without frames_dev, grown on demand
    std::string err;
};

namespace {
int64_t pt_frames(const wrnn_pitch_handle *h, int64_t n) { return n > 0 ? 1 + n / h->cfg.hop : 0; }

int pt_launch_track(wrnn_pitch_handle *h, const float *a, const float *b, float *f0_a, float *ap_a, float *f0_b, float *ap_b, int64_t n_max,
                    const int32_t *n_dev, int B, int64_t stride, hipStream_t s) {
    const wrnn_pitch_config &c = h->cfg;
    PitchTrackArgs g{};
    g.src[0] = a; g.src[1] = b; g.f0[0] = f0_a; g.f0[1] = f0_b; g.ap[0] = ap_a; g.ap[1] = ap_b;
    g.n_samples = n_dev; g.n_max = n_max; g.stride = stride;
    g.T_max = (int32_t)pt_frames(h, n_max); g.hop = c.hop; g.frame_length = c.frame_length; g.window = c.window;
    g.tau_min = h->tau_min; g.tau_max = h->tau_max;
    g.sample_rate = (double)c.sample_rate; g.threshold = c.threshold; g.silence_rms = c.silence_rms;
    const size_t lds = (size_t)(h->tau_max + 3) * 8 + (size_t)c.frame_length * 4;
    hipLaunchKernelGGL(pitch_track_kernel, dim3((unsigned)g.T_max, (unsigned)B, b ? 2u : 1u), dim3(THREADS), lds, s, g);
    WRNN_TRY(h, hipGetLastError());
    return WRNN_OK;
}
}  // namespace

extern "C" {

int wrnn_pitch_create(const wrnn_pitch_config *cfg, wrnn_pitch_handle **out) {
    if (!cfg || !out) return WRNN_ERR_INVALID;
    wrnn_pitch_handle *h = new wrnn_pitch_handle();
    *out = h;
    if (cfg->struct_size != sizeof(wrnn_pitch_config))
        return wrnn_failf(h, WRNN_ERR_INVALID, "struct_size = %u, this library's wrnn_pitch_config has %zu bytes", cfg->struct_size, sizeof(wrnn_pitch_config));
    h->cfg = *cfg;
    if (cfg->sample_rate < 1 || cfg->hop < 1)
        return wrnn_failf(h, WRNN_ERR_INVALID, "sample_rate = %d, hop = %d: both are at least 1", cfg->sample_rate, cfg->hop);
    if (!std::isfinite(cfg->fmin) || !std::isfinite(cfg->fmax) || !(cfg->fmin < cfg->fmax))
        return wrnn_failf(h, WRNN_ERR_INVALID, "fmin = %g, fmax = %g: finite, and fmin < fmax", cfg->fmin, cfg->fmax);
    const double lo = std::ceil((double)cfg->sample_rate / cfg->fmax), hi = std::floor((double)cfg->sample_rate / cfg->fmin);
    if (lo < 1.0) return wrnn_failf(h, WRNN_ERR_INVALID, "tau_min = ceil(sample_rate / fmax) = %g: a lag is at least 1", lo);
    if (!(cfg->fmin > 0.0)) return wrnn_failf(h, WRNN_ERR_INVALID, "fmin = %g: tau_max = floor(sample_rate / fmin) needs fmin > 0", cfg->fmin);
    if (lo > hi) return wrnn_failf(h, WRNN_ERR_INVALID, "tau_min = %g > tau_max = %g: no lag lies between sample_rate / fmax and sample_rate / fmin", lo, hi);
    if (!(cfg->threshold > 0.0 && cfg->threshold < 1.0)) return wrnn_failf(h, WRNN_ERR_INVALID, "threshold = %g is outside (0, 1)", cfg->threshold);
    if (!(cfg->silence_rms >= 0.0) || !std::isfinite(cfg->silence_rms))
        return wrnn_failf(h, WRNN_ERR_INVALID, "silence_rms = %g: finite and at least 0", cfg->silence_rms);
    if (!(cfg->gpe_ratio > 0.0) || !std::isfinite(cfg->gpe_ratio)) return wrnn_failf(h, WRNN_ERR_INVALID, "gpe_ratio = %g: finite and above 0", cfg->gpe_ratio);
    if (cfg->window < 1) return wrnn_failf(h, WRNN_ERR_INVALID, "window = %d: at least 1", cfg->window);
    const int fl = cfg->frame_length;
    if (fl != 512 && fl != 1024 && fl != 2048 && fl != 4096)
        return wrnn_failf(h, WRNN_ERR_UNSUPPORTED, "frame_length = %d is none of 512, 1024, 2048, 4096", fl);
    if ((double)cfg->window + hi + 1.0 > (double)fl)
        return wrnn_failf(h, WRNN_ERR_UNSUPPORTED, "window + tau_max + 1 = %d + %g + 1 exceeds frame_length = %d", cfg->window, hi, fl);
    h->tau_min = (int)lo;
    h->tau_max = (int)hi;
    h->ok = true;
    return WRNN_OK;
}

int64_t wrnn_pitch_frames(const wrnn_pitch_handle *h, int64_t n) {
    if (!h || !h->ok || n < 0 || n > INT32_MAX) return WRNN_ERR_INVALID;
    return pt_frames(h, n);
}

int wrnn_pitch_lags(const wrnn_pitch_handle *h, int32_t *tau_min, int32_t *tau_max) {
    if (!h || !h->ok) return WRNN_ERR_INVALID;
    if (tau_min) *tau_min = h->tau_min;
    if (tau_max) *tau_max = h->tau_max;
    return WRNN_OK;
}

int wrnn_pitch_track(wrnn_pitch_handle *h, const float *wav_dev, int64_t n_max, const int32_t *n_dev, int32_t B, float *f0_dev,
                     float *aperiodicity_dev, int64_t frames_stride, void *stream) {
    if (!h) return WRNN_ERR_INVALID;
    if (!h->ok) return wrnn_failf(h, WRNN_ERR_STATE, "the handle's configuration was refused by wrnn_pitch_create");
    if (!wav_dev || !n_dev || !f0_dev || B < 1 || B > WRNN_MAX_GRID_Y || n_max < 1 || n_max > INT32_MAX)
        return wrnn_failf(h, WRNN_ERR_INVALID, "bad arguments: device pointers, 1 <= B <= 65535, 1 <= n_max < 2^31");
    if (frames_stride < pt_frames(h, n_max))
        return wrnn_failf(h, WRNN_ERR_INVALID, "frames_stride = %lld: a row holds %lld frames for n_max = %lld", (long long)frames_stride,
                       (long long)pt_frames(h, n_max), (long long)n_max);
    WRNN_TRY(h, hipSetDevice(h->cfg.device));
    return pt_launch_track(h, wav_dev, nullptr, f0_dev, aperiodicity_dev, nullptr, nullptr, n_max, n_dev, B, frames_stride, (hipStream_t)stream);
}

int wrnn_pitch_score(wrnn_pitch_handle *h, const float *target_dev, const float *test_dev, int64_t n_max, const int32_t *n_dev, int32_t B,
                     double *summary_dev, float *frames_dev, int64_t frames_stride, void *stream) {
    if (!h) return WRNN_ERR_INVALID;
    if (!h->ok) return wrnn_failf(h, WRNN_ERR_STATE, "the handle's configuration was refused by wrnn_pitch_create");
    if (!target_dev || !test_dev || !n_dev || !summary_dev || B < 1 || B > WRNN_MAX_GRID_Y || n_max < 1 || n_max > INT32_MAX)
        return wrnn_failf(h, WRNN_ERR_INVALID, "bad arguments: device pointers, 1 <= B <= 65535, 1 <= n_max < 2^31");
    const int64_t T = pt_frames(h, n_max), total = 5 * T;
    if (frames_dev && frames_stride < total)
        return wrnn_failf(h, WRNN_ERR_INVALID, "frames_stride = %lld: a row of the per-frame buffer holds %lld values for n_max = %lld", (long long)frames_stride,
                       (long long)total, (long long)n_max);
    hipStream_t s = (hipStream_t)stream;
    WRNN_TRY(h, hipSetDevice(h->cfg.device));
    const int64_t stride = frames_dev ? frames_stride : total;
    if (!frames_dev) WRNN_TRY(h, h->ws.reserve((size_t)B * (size_t)total * 4, s));
    float *frames = frames_dev ? frames_dev : (float *)h->ws.p;
    const int rc = pt_launch_track(h, target_dev, test_dev, frames, frames + T, frames + 2 * T, frames + 3 * T, n_max, n_dev, B, stride, s);
    if (rc != WRNN_OK) return rc;
    PitchPairArgs p{};
    p.frames = frames; p.cents = frames + 4 * T; p.n_samples = n_dev; p.summary = summary_dev; p.n_max = n_max; p.stride = stride;
    p.T_max = (int32_t)T; p.hop = h->cfg.hop; p.gpe_ratio = h->cfg.gpe_ratio;
    hipLaunchKernelGGL(pitch_pair_kernel, dim3((unsigned)((T + THREADS - 1) / THREADS), (unsigned)B), dim3(THREADS), 0, s, p);
    WRNN_TRY(h, hipGetLastError());
    hipLaunchKernelGGL(pitch_summary_kernel, dim3((unsigned)B), dim3(THREADS), 0, s, p);
    WRNN_TRY(h, hipGetLastError());
    return WRNN_OK;
}

const char *wrnn_pitch_last_error(const wrnn_pitch_handle *h) { return wrnn_last_error_of(h); }

void wrnn_pitch_destroy(wrnn_pitch_handle *h) {
    if (!h) return;
    if (h->ws.p) {
        (void)hipSetDevice(h->cfg.device);
        h->ws.release();
    }
    delete h;
}

}  // extern "C"
