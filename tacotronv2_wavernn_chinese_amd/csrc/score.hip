// Spectral scores on the device: how far a test clip is from a target clip, as the two mel distances (per-frame log-mel distance and
// mel-cepstral distortion over the front end's own mel, melspec.hip as it is) and the multi-resolution STFT distance (spectral
// convergence and log-magnitude distance at up to four (n_fft, hop, win) resolutions).  The definitions are in the header's section.
// Plain grid kernels; nothing crosses workgroups, nothing spins, no floating-point atomics, every sum in a fixed order:
//   score_stft_kernel<LOG>  grid (ceil(T_max / FPW), B), once per resolution   gather with reflection under the window, both clips'
//                           frames as two real transforms side by side in LDS, split pass, floored magnitudes, the three bin sums
//   score_mel_kernel        grid (ceil(T_max / 4), B)      one wave per frame over the two mels: lsd_t and the K DCT rows of mcd_t
//   score_reduce_kernel     grid (quantities, B)           float32 per-frame values -> one float64 sum
//   score_finalize_kernel   grid (ceil(B / 64))            the sums -> the WRNN_SCORE_FIELDS summaries of a clip
// Both clips of a frame run through the SAME instruction sequence (the transform index is a loop variable, not a code path), so
// identical clips give identical magnitudes and every distance is exactly 0.  The one-complex-transform-for-two-real-signals form is not
// used: its split cancels, and identical clips would no longer give equal bits.
// Precision: the clips and every per-frame value are float32.  The window, the twiddles and the transform up to re^2 + im^2 are float64,
// rounded to float32 once per bin; the floor, the square root and the logarithm are float32; the bin sums are carried in float64 and
// rounded once per frame.  A float32 transform was measured to miss the parity bound: |ln A - ln B| divides the transform's absolute
// error by the bin's magnitude, the smallest bins of a noisy frame lie a thousand times under its RMS, and two float32 factorisations
// then differ by an order of magnitude more than either's typical error (13 x the restatement's own float32 error on white noise at
// n_fft 2048).  With the float64 transform every quantity stays under 1 x that error.
// LDS per workgroup: 2 clips x FPW frames x (n_fft / 2) double2 = 32 KiB at n_fft 2048, 16 KiB at 1024, 512 and 256, plus 12 doubles for
// the waves' sums.
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "dsp_device.h"
#include "dsp_tables.h"
#include "handle_common.h"

namespace {

constexpr int THREADS = 256;
constexpr int MAX_WAVES = THREADS / 64;
constexpr int MAX_MELS = 128;                          // the front end's own limit
constexpr int MAX_QUANT = 2 + 3 * WRNN_SCORE_MAX_RES;   // per-frame quantities: lsd, mcd, then num, den, lm per resolution

struct ScoreStftArgs {
    const float *a, *b;           // target and test clips, row stride n_max
    const int32_t *n_samples;     // [B]
    const double *window;         // [win]
    const double2 *twiddle;       // [n_fft]  cos, -sin of 2 pi k / n_fft
    float *frames;                // per-frame buffer, row stride `stride`; this resolution's num | den | lm from `offset`
    int64_t n_max, stride, offset;
    int32_t T_max, hop, win, min_samples;
    float floor;
};

// The clip's own length as every kernel here reads it: clamped to the buffer, and 0 (no frames anywhere) for a clip too short to pad.
__device__ inline long clip_len(const int32_t *n_samples, int b, long n_max, int min_samples) {
    long n = n_samples[b];
    if (n > n_max) n = n_max;
    return n >= min_samples ? n : 0;
}

// LOG = log2(n_fft / 2), the complex points NC of one real transform.  FPW frames per workgroup, TPF threads per frame (a multiple of
// the wave); the frame's two transforms (target, test) share its threads.
template <int LOG>
__global__ void __launch_bounds__(THREADS) score_stft_kernel(ScoreStftArgs g) {
    constexpr int NC = 1 << LOG, N = 2 * NC;
    constexpr int FPW = NC >= 512 ? 1 : 512 / NC, TPF = THREADS / FPW, WPF = TPF / 64;
    __shared__ double2 z[FPW * 2 * NC];
    __shared__ double part[3][MAX_WAVES];
    const int tid = threadIdx.x, b = blockIdx.y, f = tid / TPF, lt = tid % TPF;
    const int t = blockIdx.x * FPW + f;
    const long n = clip_len(g.n_samples, b, g.n_max, g.min_samples);
    const int T_b = n > 0 ? (int)(1 + n / g.hop) : 0;
    float *out = g.frames + (long)b * g.stride + g.offset;
    if ((int)blockIdx.x * FPW >= T_b) {     // workgroup-uniform: every frame of this workgroup lies past the clip's own end
        if (lt == 0 && t < g.T_max) out[t] = out[g.T_max + t] = out[2L * g.T_max + t] = 0.0f;
        return;
    }
    const bool live = t < T_b;              // uniform over the frame's threads; a dead frame of a live workgroup transforms zeros
    double2 *zf = z + f * 2 * NC;
    const int off = (N - g.win) / 2;
    const long j0 = (long)t * g.hop - NC;   // clip index of frame sample 0
    // z[k] = x[2k] + i x[2k + 1] of the windowed frame, stored bit-reversed for the in-place decimation-in-time passes
    for (int i = lt; i < 2 * NC; i += TPF) {
        const int sig = i >> LOG, k = i & (NC - 1);
        const float *x = (sig ? g.b : g.a) + (long)b * g.n_max;
        double v[2];
#pragma unroll
        for (int e = 0; e < 2; ++e) {
            const int w = 2 * k + e - off;  // window tap
            v[e] = 0.0;
            if (live && w >= 0 && w < g.win) {
                long j = j0 + 2 * k + e;
                if (j < 0) j = -j;
                else if (j >= n) j = 2 * (n - 1) - j;
                v[e] = (double)x[j] * g.window[w];
            }
        }
        zf[sig * NC + (int)(__brev((unsigned)k) >> (32 - LOG))] = make_double2(v[0], v[1]);
    }
    // radix-2 passes, fused in pairs (one four-point butterfly per step); an odd LOG starts with one pass of span 1 (twiddle 1)
    int s = 0;
    if (LOG & 1) {
        __syncthreads();
        for (int i = lt; i < NC; i += TPF) {            // 2 transforms x NC / 2 butterflies
            double2 *p = zf + (i >> (LOG - 1)) * NC + 2 * (i & (NC / 2 - 1));
            const double2 x0 = p[0], x1 = p[1];
            p[0] = make_double2(x0.x + x1.x, x0.y + x1.y);
            p[1] = make_double2(x0.x - x1.x, x0.y - x1.y);
        }
        s = 1;
    }
#pragma unroll
    for (; s < LOG; s += 2) {
        __syncthreads();
        const int q = 1 << s;
        for (int i = lt; i < NC / 2; i += TPF) {        // 2 transforms x NC / 4 butterflies
            const int sig = i >> (LOG - 2), j = i & (NC / 4 - 1);
            const int pos = j & (q - 1);
            double2 *p = zf + sig * NC + ((j >> s) << (s + 2)) + pos;
            const double2 x0 = p[0], x1 = p[q], x2 = p[2 * q], x3 = p[3 * q];
            // pass s: pairs (0, 1) and (2, 3) at distance q with W_{2q}^pos; pass s + 1: pairs (0, 2) with W_{4q}^pos and (1, 3) with
            // W_{4q}^{pos + q} = -i W_{4q}^pos.  Both as indices into the n_fft-point table.
            const double2 w1 = g.twiddle[pos * (N >> (s + 1))], w2 = g.twiddle[pos * (N >> (s + 2))];
            const double2 t1 = cmul(w1, x1), t3 = cmul(w1, x3);
            const double2 u0 = make_double2(x0.x + t1.x, x0.y + t1.y), u1 = make_double2(x0.x - t1.x, x0.y - t1.y);
            const double2 u2 = make_double2(x2.x + t3.x, x2.y + t3.y), u3 = make_double2(x2.x - t3.x, x2.y - t3.y);
            const double2 v2 = cmul(w2, u2), v3 = cmul(w2, u3);
            p[0] = make_double2(u0.x + v2.x, u0.y + v2.y);
            p[2 * q] = make_double2(u0.x - v2.x, u0.y - v2.y);
            p[q] = make_double2(u1.x + v3.y, u1.y - v3.x);        // u1 - i v3
            p[3 * q] = make_double2(u1.x - v3.y, u1.y + v3.x);    // u1 + i v3
        }
    }
    __syncthreads();
    // split pass: X[k] = E[k] + W^k O[k], X[NC - k] = conj(E[k] - W^k O[k]); the squared magnitudes of bins k and NC - k of both clips
    // The terms are float32; their sums are carried in float64 and rounded once, so a frame's value is the float32 next to the sum of
    // its terms (a float32 sum over 1025 bins would add an error of its own, of the size of the last place of the result).
    double num = 0.0, den = 0.0, lm = 0.0;
    for (int k = lt; k <= NC / 2; k += TPF) {
        float pw[2][2];                     // [clip][bin k, bin NC - k] re^2 + im^2, rounded to float32 here
#pragma unroll
        for (int sig = 0; sig < 2; ++sig) {
            const double2 *zs = zf + sig * NC;
            if (k == 0) {
                const double2 z0 = zs[0];
                const double dc = z0.x + z0.y, ny = z0.x - z0.y;
                pw[sig][0] = (float)(dc * dc);
                pw[sig][1] = (float)(ny * ny);
            } else {
                const double2 zk = zs[k], zn = zs[NC - k];
                const double2 E = make_double2(0.5 * (zk.x + zn.x), 0.5 * (zk.y - zn.y));
                const double2 O = make_double2(0.5 * (zk.y + zn.y), -0.5 * (zk.x - zn.x));
                const double2 WO = cmul(g.twiddle[k], O);
                const double pr = E.x + WO.x, pi = E.y + WO.y, mr = E.x - WO.x, mi = E.y - WO.y;
                pw[sig][0] = (float)(pr * pr + pi * pi);
                pw[sig][1] = (float)(mr * mr + mi * mi);
            }
        }
        const int bins = 2 * k == NC ? 1 : 2;   // the middle item is one bin, not a pair
        for (int e = 0; e < bins; ++e) {
            const float A = sqrtf(fmaxf(pw[0][e], g.floor)), Bm = sqrtf(fmaxf(pw[1][e], g.floor));
            const float d = Bm - A;
            num += (double)(d * d);
            den += (double)(A * A);
            lm += (double)fabsf(logf(A) - logf(Bm));
        }
    }
    // bin sums: the wave, then the frame's waves in ascending order
    for (int o = 32; o > 0; o >>= 1) {
        num += __shfl_xor(num, o);
        den += __shfl_xor(den, o);
        lm += __shfl_xor(lm, o);
    }
    if ((tid & 63) == 0) {
        part[0][tid >> 6] = num;
        part[1][tid >> 6] = den;
        part[2][tid >> 6] = lm;
    }
    __syncthreads();
    if (lt == 0 && t < g.T_max) {
        double r[3];
        for (int c = 0; c < 3; ++c) {
            r[c] = part[c][f * WPF];
            for (int w = 1; w < WPF; ++w) r[c] += part[c][f * WPF + w];
        }
        out[t] = live ? (float)r[0] : 0.0f;
        out[g.T_max + t] = live ? (float)r[1] : 0.0f;
        out[2L * g.T_max + t] = live ? (float)r[2] : 0.0f;
    }
}

struct ScoreMelArgs {
    const float *mel_a, *mel_b;   // (B, n_mels, T_max) in [0, 1]
    const int32_t *n_samples;
    const float *dct_t;           // (n_mels, K): C[k, m] at [m * K + k - 1]
    float *frames;                // lsd | mcd from column 0 of every row
    int64_t n_max, stride;
    int32_t T_max, n_mels, hop, K, min_samples;
    float range_db;               // -min_level_db
};

// One wave per frame; lane l holds mel rows l and l + 64, then DCT rows l + 1 and l + 65.
__global__ void __launch_bounds__(THREADS) score_mel_kernel(ScoreMelArgs g) {
    __shared__ float e[MAX_WAVES][MAX_MELS];    // D ln10 / 20 of the wave's frame
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, b = blockIdx.y;
    const int t = blockIdx.x * MAX_WAVES + wave;
    if (t >= g.T_max) return;               // wave-uniform; no barrier below, every wave keeps to its own row of `e`
    float *out = g.frames + (long)b * g.stride;
    const long n = clip_len(g.n_samples, b, g.n_max, g.min_samples);
    const int T_b = n > 0 ? (int)(1 + n / g.hop) : 0;
    if (t >= T_b) {
        if (lane == 0) out[t] = out[g.T_max + t] = 0.0f;
        return;
    }
    const float ln10_20 = 0.11512925464970229f;
    double sq = 0.0;              // float32 terms, float64 sums, rounded once (as in the transform kernel)
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const int m = lane + 64 * h;
        if (m < g.n_mels) {
            const long i = ((long)b * g.n_mels + m) * g.T_max + t;
            const float d = (g.mel_a[i] - g.mel_b[i]) * g.range_db;
            sq += (double)(d * d);
            e[wave][m] = d * ln10_20;
        }
    }
    for (int o = 32; o > 0; o >>= 1) sq += __shfl_xor(sq, o);
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    double cc = 0.0;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const int k = lane + 64 * h;        // DCT row k + 1
        if (k < g.K) {
            double c = 0.0;
            for (int m = 0; m < g.n_mels; ++m) c = fma((double)g.dct_t[m * g.K + k], (double)e[wave][m], c);
            cc += c * c;
        }
    }
    for (int o = 32; o > 0; o >>= 1) cc += __shfl_xor(cc, o);
    if (lane == 0) {
        out[t] = (float)sqrt(sq / (double)g.n_mels);
        out[g.T_max + t] = (float)(4.342944819032518 * sqrt(2.0 * cc));   // 10 / ln 10
    }
}

// grid (Q, B): the float32 per-frame values of one quantity of one clip -> their float64 sum.  Thread i adds entries i, i + 256, ...
// in ascending order, then the threads are added pairwise in a fixed tree: the order depends on an entry's position only, and the
// zeros past a clip's own frames change nothing, so a clip of a ragged batch gives the bits of the call on it alone.
struct ScoreReduceArgs {
    const float *frames;
    double *sums;                 // (B, Q)
    int64_t stride;
    int64_t seg_off[MAX_QUANT];
    int32_t seg_len[MAX_QUANT];
    int32_t Q;
};

__global__ void __launch_bounds__(THREADS) score_reduce_kernel(ScoreReduceArgs g) {
    __shared__ double acc[THREADS];
    const int q = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
    const float *v = g.frames + (long)b * g.stride + g.seg_off[q];
    const int len = g.seg_len[q];
    double s = 0.0;
    for (int i = tid; i < len; i += THREADS) s += (double)v[i];
    acc[tid] = s;
    for (int d = THREADS / 2; d > 0; d >>= 1) {
        __syncthreads();
        if (tid < d) acc[tid] += acc[tid + d];
    }
    if (tid == 0) g.sums[(long)b * g.Q + q] = acc[0];
}

struct ScoreFinalArgs {
    const double *sums;           // (B, Q): lsd, mcd, then num, den, lm per resolution
    const int32_t *n_samples;
    double *summary;              // (B, WRNN_SCORE_FIELDS)
    int64_t n_max;
    int32_t B, n_res, mel_hop, min_samples;
    int32_t hop[WRNN_SCORE_MAX_RES], bins[WRNN_SCORE_MAX_RES];
};

__global__ void __launch_bounds__(64) score_finalize_kernel(ScoreFinalArgs g) {
    const int b = blockIdx.x * 64 + threadIdx.x;
    if (b >= g.B) return;
    const long n = clip_len(g.n_samples, b, g.n_max, g.min_samples);
    const double *s = g.sums + (long)b * (2 + 3 * g.n_res);
    double *o = g.summary + (long)b * WRNN_SCORE_FIELDS;
    for (int i = 0; i < WRNN_SCORE_FIELDS; ++i) o[i] = 0.0;
    if (n == 0) return;
    const double T_mel = (double)(1 + n / g.mel_hop);
    o[WRNN_SCORE_MEL_LSD_DB] = s[0] / T_mel;
    o[WRNN_SCORE_MCD_DB] = s[1] / T_mel;
    double sc_sum = 0.0, lm_sum = 0.0;
    for (int r = 0; r < g.n_res; ++r) {
        const double T = (double)(1 + n / g.hop[r]);
        const double sc = sqrt(s[2 + 3 * r]) / sqrt(s[3 + 3 * r]), lm = s[4 + 3 * r] / (T * (double)g.bins[r]);
        o[WRNN_SCORE_SC0 + r] = sc;
        o[WRNN_SCORE_LOGMAG0 + r] = lm;
        sc_sum += sc;
        lm_sum += lm;
    }
    o[WRNN_SCORE_MR_SC] = sc_sum / (double)g.n_res;
    o[WRNN_SCORE_MR_LOGMAG] = lm_sum / (double)g.n_res;
}

template <int LOG>
void launch_stft(const ScoreStftArgs &a, int B, hipStream_t s) {
    constexpr int NC = 1 << LOG, FPW = NC >= 512 ? 1 : 512 / NC;
    hipLaunchKernelGGL(score_stft_kernel<LOG>, dim3((unsigned)((a.T_max + FPW - 1) / FPW), (unsigned)B), dim3(THREADS), 0, s, a);
}

}  // namespace

// ---- the C entries ----------------------------------------------------------------------------------------------------------------------

struct wrnn_score_handle {
    wrnn_mel_config cfg{};
    wrnn_mel_features feat{};
    wrnn_score_config scfg{};
    bool ok = false;                  // false while the configuration is refused
    int min_samples = 0;              // the shortest clip every transform (and the mel) can pad
    wrnn_mel_handle *mel = nullptr;   // the front end the mels come from: its own handle, its own launch path
    std::vector<double> window[WRNN_SCORE_MAX_RES], twiddle[WRNN_SCORE_MAX_RES];   // float64, as the transform kernel reads them
    std::vector<float> dct;           // (K, n_mels): dsp_tables.h's rows, rounded to float32 once
    void *dev = nullptr;              // per resolution window | twiddle (float64), then the DCT transposed (float32); uploaded by the first call
    size_t o_win[WRNN_SCORE_MAX_RES] = {}, o_tw[WRNN_SCORE_MAX_RES] = {}, o_dct = 0;
    WrnnScratch ws;                   // the two mels | the sums | the per-frame scratch, grown on demand
    std::string err;
};

namespace {
int64_t frames_of(const wrnn_score_handle *h, int r, int64_t n) { return 1 + n / (r < 0 ? h->cfg.hop_length : h->scfg.hop[r]); }
}  // namespace

extern "C" {

int wrnn_score_create(const wrnn_mel_config *cfg, const wrnn_mel_features *f, const wrnn_score_config *sc, wrnn_score_handle **out) {
    if (!cfg || !sc || !out) return WRNN_ERR_INVALID;
    wrnn_score_handle *h = new wrnn_score_handle();
    *out = h;
    h->cfg = *cfg;
    if (!f) f = &WRNN_DEFAULT_MEL_FEATURES;
    if (sc->struct_size != sizeof(wrnn_score_config))
        return wrnn_failf(h, WRNN_ERR_INVALID, "score.struct_size = %u, this library's wrnn_score_config has %zu bytes", sc->struct_size, sizeof(wrnn_score_config));
    h->scfg = *sc;
    // the front end checks its own configuration (struct_size of the features included) and builds its own tables; no device is touched
    const int rc = wrnn_mel_create_features(cfg, f, &h->mel);
    if (rc != WRNN_OK) return wrnn_failf(h, rc, "%s", h->mel ? wrnn_mel_last_error(h->mel) : "wrnn_mel_create_features failed");
    h->feat = *f;
    if (sc->n_res < 1 || sc->n_res > WRNN_SCORE_MAX_RES)
        return wrnn_failf(h, WRNN_ERR_INVALID, "n_res = %d: a handle holds 1 .. %d resolutions", sc->n_res, WRNN_SCORE_MAX_RES);
    int min_samples = f->pad_mode == WRNN_MEL_PAD_REFLECT ? cfg->n_fft / 2 + 1 : 1;
    for (int r = 0; r < sc->n_res; ++r) {
        const int n_fft = sc->n_fft[r];
        if (n_fft != 256 && n_fft != 512 && n_fft != 1024 && n_fft != 2048)
            return wrnn_failf(h, WRNN_ERR_INVALID, "resolution %d: n_fft = %d is none of 256, 512, 1024, 2048", r, n_fft);
        if (sc->win[r] < 1 || sc->win[r] > n_fft || sc->hop[r] < 1)
            return wrnn_failf(h, WRNN_ERR_INVALID, "resolution %d: 1 <= win <= n_fft and hop >= 1, got win = %d, hop = %d", r, sc->win[r], sc->hop[r]);
        if (n_fft / 2 + 1 > min_samples) min_samples = n_fft / 2 + 1;
    }
    if (!(sc->mag_floor > 0.0f) || !std::isfinite(sc->mag_floor))
        return wrnn_failf(h, WRNN_ERR_INVALID, "mag_floor = %g: the floor under re^2 + im^2 is finite and > 0 (its logarithm is taken)", (double)sc->mag_floor);
    if (sc->mcd_order < 1 || sc->mcd_order > cfg->n_mels - 1)
        return wrnn_failf(h, WRNN_ERR_INVALID, "mcd_order = %d: 1 <= mcd_order <= n_mels - 1 = %d", sc->mcd_order, cfg->n_mels - 1);
    // float64: the transform kernel reads the window and the twiddles unrounded
    for (int r = 0; r < sc->n_res; ++r) {
        h->window[r] = wrnn_dsp::hann_periodic(sc->win[r]);
        h->twiddle[r] = wrnn_dsp::twiddles(sc->n_fft[r]);
    }
    const std::vector<double> dct = wrnn_dsp::dct_rows(cfg->n_mels, sc->mcd_order);
    h->dct.assign(dct.begin(), dct.end());
    h->min_samples = min_samples;
    h->ok = true;
    return WRNN_OK;
}

int64_t wrnn_score_frames(const wrnn_score_handle *h, int32_t r, int64_t n) {
    if (!h || !h->ok || r < -1 || r >= h->scfg.n_res || n < h->min_samples || n > INT32_MAX) return WRNN_ERR_INVALID;
    return frames_of(h, r, n);
}

int wrnn_score_tables(const wrnn_score_handle *h, int32_t r, float *window, float *twiddle, float *dct) {
    if (!h || !h->ok || r < 0 || r >= h->scfg.n_res) return WRNN_ERR_INVALID;
    if (window)
        for (size_t i = 0; i < h->window[r].size(); ++i) window[i] = (float)h->window[r][i];
    if (twiddle)
        for (size_t i = 0; i < h->twiddle[r].size(); ++i) twiddle[i] = (float)h->twiddle[r][i];
    if (dct) std::memcpy(dct, h->dct.data(), h->dct.size() * 4);
    return WRNN_OK;
}

int wrnn_score(wrnn_score_handle *h, const float *target_dev, const float *test_dev, int64_t n_max, const int32_t *n_dev, int32_t B,
               double *summary_dev, float *frames_dev, int64_t frames_stride, void *stream) {
    if (!h) return WRNN_ERR_INVALID;
    if (!h->ok) return wrnn_failf(h, WRNN_ERR_STATE, "the handle's configuration was refused by wrnn_score_create");
    if (!target_dev || !test_dev || !n_dev || !summary_dev || B < 1 || B > WRNN_MAX_GRID_Y || n_max < h->min_samples || n_max > INT32_MAX)
        return wrnn_failf(h, WRNN_ERR_INVALID, "bad arguments: device pointers, 1 <= B <= 65535, %d <= n_max < 2^31", h->min_samples);
    const wrnn_score_config &sc = h->scfg;
    const int n_res = sc.n_res, Q = 2 + 3 * n_res, n_mels = h->cfg.n_mels, K = sc.mcd_order;
    // the per-frame row: lsd | mcd | (num | den | lm) of every resolution, every segment as long as the frames of n_max samples
    int64_t seg_off[MAX_QUANT], total = 0;
    int32_t seg_len[MAX_QUANT];
    for (int q = 0; q < Q; ++q) {
        const int64_t T = frames_of(h, q < 2 ? -1 : (q - 2) / 3, n_max);
        seg_off[q] = total;
        seg_len[q] = (int32_t)T;
        total += T;
    }
    if (frames_dev && frames_stride < total)
        return wrnn_failf(h, WRNN_ERR_INVALID, "frames_stride = %lld: a row of the per-frame buffer holds %lld values for n_max = %lld", (long long)frames_stride,
                       (long long)total, (long long)n_max);
    hipStream_t s = (hipStream_t)stream;
    WRNN_TRY(h, hipSetDevice(h->cfg.device));
    if (!h->dev) {
        WrnnImage img;
        for (int r = 0; r < n_res; ++r) {
            h->o_win[r] = img.put(h->window[r].data(), h->window[r].size() * 8);
            h->o_tw[r] = img.put(h->twiddle[r].data(), h->twiddle[r].size() * 8);
        }
        h->o_dct = img.take(h->dct.size() * 4);
        float *dt = img.at<float>(h->o_dct);
        for (int k = 0; k < K; ++k)
            for (int m = 0; m < n_mels; ++m) dt[(size_t)m * K + k] = h->dct[(size_t)k * n_mels + m];
        const hipError_t e = img.upload(&h->dev);
        if (e != hipSuccess) return wrnn_failf(h, WRNN_ERR_HIP, "uploading the score tables: %s", hipGetErrorString(e));
    }
    // the two mels | the sums | the per-frame scratch: the calls on one handle share them, so the caller orders those calls
    const int T_mel = seg_len[0];
    const size_t b_mel = wrnn_up256((size_t)B * n_mels * T_mel * 4), b_sums = wrnn_up256((size_t)B * Q * 8);
    const int64_t stride = frames_dev ? frames_stride : total;
    WRNN_TRY(h, h->ws.reserve(2 * b_mel + b_sums + (frames_dev ? 0 : wrnn_up256((size_t)B * total * 4)), s));
    char *ws = h->ws.p;
    float *mel_a = (float *)ws, *mel_b = (float *)(ws + b_mel);
    double *sums = (double *)(ws + 2 * b_mel);
    float *frames = frames_dev ? frames_dev : (float *)(ws + 2 * b_mel + b_sums);
    const char *d = (const char *)h->dev;
    // the mels: the front end's own entry, twice into scratch
    if (wrnn_melspectrogram(h->mel, target_dev, n_max, n_dev, B, T_mel, mel_a, stream) != WRNN_OK ||
        wrnn_melspectrogram(h->mel, test_dev, n_max, n_dev, B, T_mel, mel_b, stream) != WRNN_OK)
        return wrnn_failf(h, WRNN_ERR_HIP, "the mel front end: %s", wrnn_mel_last_error(h->mel));
    ScoreMelArgs m{};
    m.mel_a = mel_a; m.mel_b = mel_b; m.n_samples = n_dev; m.dct_t = (const float *)(d + h->o_dct); m.frames = frames;
    m.n_max = n_max; m.stride = stride; m.T_max = T_mel; m.n_mels = n_mels; m.hop = h->cfg.hop_length; m.K = K; m.min_samples = h->min_samples;
    m.range_db = -h->cfg.min_level_db;
    hipLaunchKernelGGL(score_mel_kernel, dim3((unsigned)((T_mel + MAX_WAVES - 1) / MAX_WAVES), (unsigned)B), dim3(THREADS), 0, s, m);
    WRNN_TRY(h, hipGetLastError());
    for (int r = 0; r < n_res; ++r) {
        ScoreStftArgs a{};
        a.a = target_dev; a.b = test_dev; a.n_samples = n_dev;
        a.window = (const double *)(d + h->o_win[r]); a.twiddle = (const double2 *)(d + h->o_tw[r]);
        a.frames = frames; a.n_max = n_max; a.stride = stride; a.offset = seg_off[2 + 3 * r];
        a.T_max = seg_len[2 + 3 * r]; a.hop = sc.hop[r]; a.win = sc.win[r]; a.min_samples = h->min_samples; a.floor = sc.mag_floor;
        switch (sc.n_fft[r]) {
            case 256: launch_stft<7>(a, B, s); break;
            case 512: launch_stft<8>(a, B, s); break;
            case 1024: launch_stft<9>(a, B, s); break;
            default: launch_stft<10>(a, B, s); break;
        }
        WRNN_TRY(h, hipGetLastError());
    }
    ScoreReduceArgs ra{};
    ra.frames = frames; ra.sums = sums; ra.stride = stride; ra.Q = Q;
    for (int q = 0; q < Q; ++q) {
        ra.seg_off[q] = seg_off[q];
        ra.seg_len[q] = seg_len[q];
    }
    hipLaunchKernelGGL(score_reduce_kernel, dim3((unsigned)Q, (unsigned)B), dim3(THREADS), 0, s, ra);
    WRNN_TRY(h, hipGetLastError());
    ScoreFinalArgs fa{};
    fa.sums = sums; fa.n_samples = n_dev; fa.summary = summary_dev; fa.n_max = n_max; fa.B = B; fa.n_res = n_res;
    fa.mel_hop = h->cfg.hop_length; fa.min_samples = h->min_samples;
    for (int r = 0; r < n_res; ++r) {
        fa.hop[r] = sc.hop[r];
        fa.bins[r] = sc.n_fft[r] / 2 + 1;
    }
    hipLaunchKernelGGL(score_finalize_kernel, dim3((unsigned)((B + 63) / 64)), dim3(64), 0, s, fa);
    WRNN_TRY(h, hipGetLastError());
    return WRNN_OK;
}

const char *wrnn_score_last_error(const wrnn_score_handle *h) { return wrnn_last_error_of(h); }

void wrnn_score_destroy(wrnn_score_handle *h) {
    if (!h) return;
    if (h->dev || h->ws.p) {
        (void)hipSetDevice(h->cfg.device);
        if (h->dev) (void)hipFree(h->dev);
        h->ws.release();
    }
    if (h->mel) wrnn_mel_destroy(h->mel);
    delete h;
}

}  // extern "C"
