// The mel front end (melspec.hip): wav -> normalised mel spectrogram, wavernn/utils/dsp.py:41-43, 50-51, 58-59, 72-81.
#pragma once
#include <stdint.h>

#include <vector>

#include <hip/hip_runtime.h>

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
};

// Host only.  Returns false for a configuration outside the supported set (n_mels, win_length, fmin); n_fft is the caller's check.
bool wrnn_mel_build_tables(int sample_rate, int win_length, int n_mels, double fmin, WrnnMelTables *out);
hipError_t wrnn_launch_melspec(const WrnnMelArgs &a, int B, hipStream_t s);
