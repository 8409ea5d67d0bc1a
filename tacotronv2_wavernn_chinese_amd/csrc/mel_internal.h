// The mel front end (melspec.hip): wav -> normalised mel spectrogram, wavernn/utils/dsp.py:41-43, 50-51, 58-59, 72-81.
#pragma once
#include <stdint.h>

#include <cmath>
#include <vector>

#include <hip/hip_runtime.h>

#include "handle_common.h"

#define WRNN_MEL_NFFT 2048       // the one transform length the kernel is built for
#define WRNN_MEL_MAX_MELS 128
#define WRNN_MEL_THREADS 256

// Everything the kernel reads besides the clips, built on the host in float64 and rounded to float32 once (wrnn_mel_build_tables).
struct WrnnMelTables {
    std::vector<float> window;    // [win_length]  periodic Hann
    std::vector<float> twiddle;   // [NFFT][2]     cos, sin of -2 pi k / NFFT
    std::vector<int32_t> rows;    // [n_mels][3]   first_bin, n_bins, offset of the row in `weights`
    std::vector<float> weights;   // packed non-zero filterbank weights, row after row
};

struct WrnnMelArgs {
    const float *wav;             // B clips, row stride n_max
    const int32_t *n_samples;     // [B]
    float *out;                   // (B, n_mels, T_max)
    const float *window;
    const float2 *twiddle;
    const int32_t *rows;
    const float *weights;
    int64_t n_max;
    int32_t T_max, n_mels, hop, win_length;
    float min_level_db;
    // the feature profile (wrnn_mel_features); read by the profile instantiation of the kernel only
    const float *peak;            // [B] max |pre-emphasised clip|, written by the peak launch; NULL when preemph_rescale == 0
    int32_t pad_zero, power2;     // zero padding instead of reflection; |X|^2 instead of |X|
    float preemph, rescale;       // k of x[i] - k x[i-1]; the peak the pre-emphasised clip is scaled to (0: unscaled)
    float floor_amp;              // 10^(min_level_db / 20), rounded to float32
    float ref_level_db, max_abs;
};

// Host only.  Returns false for a configuration outside the supported set (n_mels, win_length, fmin); n_fft is the caller's check.
// fmax == 0: sample_rate / 2.
bool wrnn_mel_build_tables(int sample_rate, int win_length, int n_mels, double fmin, double fmax, WrnnMelTables *out);
// profile == false: the kernel of the default features (reflect padding, |X|, no pre-emphasis, direct normalisation), which reads none
// of the profile fields.  profile == true: every profile field is a run-time, workgroup-uniform switch.
hipError_t wrnn_launch_melspec(const WrnnMelArgs &a, int B, bool profile, hipStream_t s);
// peak[b] = max over i < min(n_samples[b], n_max) of |x[i] - preemph * x[i-1]| (x[-1] = 0): a memset and one launch, asynchronous.
hipError_t wrnn_launch_mel_peak(const float *wav, int64_t n_max, const int32_t *n_samples, int B, float preemph, float *peak, hipStream_t s);

// Host only.  The checks of a wrnn_mel_config and its wrnn_mel_features that do not need the tables, shared by the front end and by
// Griffin-Lim (`who` names the caller in the n_fft text).  WRNN_OK, or the status of the first refusal with its text in h->err.
template <class H>
int wrnn_mel_check(H *h, const wrnn_mel_config *cfg, const wrnn_mel_features *f, const char *who) {
    if (cfg->n_fft != WRNN_MEL_NFFT) return wrnn_failf(h, WRNN_ERR_UNSUPPORTED, "n_fft = %d: %s is built for n_fft = %d only", cfg->n_fft, who, WRNN_MEL_NFFT);
    if (cfg->hop_length < 1 || !(cfg->min_level_db < 0.0f) || cfg->device < 0)
        return wrnn_failf(h, WRNN_ERR_INVALID, "bad configuration: hop_length >= 1, min_level_db < 0, device >= 0");
    if ((f->pad_mode != WRNN_MEL_PAD_REFLECT && f->pad_mode != WRNN_MEL_PAD_ZERO) || (f->magnitude_power != 1 && f->magnitude_power != 2))
        return wrnn_failf(h, WRNN_ERR_INVALID, "bad features: pad_mode is WRNN_MEL_PAD_REFLECT or WRNN_MEL_PAD_ZERO, magnitude_power 1 or 2");
    if (!(f->preemphasis >= 0.0f) || !(f->preemph_rescale >= 0.0f) || !(f->max_abs_value >= 0.0f) || !std::isfinite(f->preemphasis) ||
        !std::isfinite(f->preemph_rescale) || !std::isfinite(f->max_abs_value) || !std::isfinite(f->ref_level_db))
        return wrnn_failf(h, WRNN_ERR_INVALID, "bad features: preemphasis, preemph_rescale and max_abs_value are finite and >= 0, ref_level_db is finite");
    if (f->fmax != 0.0f && !((double)f->fmax > (double)cfg->fmin && (double)f->fmax <= 0.5 * (double)cfg->sample_rate))
        return wrnn_failf(h, WRNN_ERR_INVALID, "bad features: fmax = %g is not in (fmin, sample_rate / 2] (0 stands for sample_rate / 2)", (double)f->fmax);
    return WRNN_OK;
}
