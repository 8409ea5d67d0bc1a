// The resampler (resample.hip): a Kaiser-windowed sinc evaluated as a polyphase bank, what librosa.load(path, sr=...) does in
// wavernn/utils/dsp.py:18-19 for a file at another rate.
#pragma once
#include <stdint.h>

#include <vector>

#include <hip/hip_runtime.h>

#define WRNN_RS_THREADS 256
#define WRNN_RS_TILE 256               // outputs per workgroup, one per thread
#define WRNN_RS_ZEROS 64               // zero crossings on each side of the filter's centre
#define WRNN_RS_MIN_SCALE_INV 32       // scale = min(1, dst / src) >= 1 / 32: bounds the LDS span
#define WRNN_RS_MAX_BANK (1 << 24)     // p * taps entries (64 MB)

// src -> dst in lowest terms: output t sits at input time t q / p.
struct WrnnResamplePlan {
    int32_t p = 0, q = 0, half = 0, taps = 0;   // taps = 2 half: j = -half + 1 .. half
    int32_t span_max = 0;                       // input samples one tile of outputs can need: ceil((TILE - 1) q / p) + taps
    std::vector<float> bank;                    // [p][taps]: bank[r][k] = h(k - half + 1 - r / p)
};

struct WrnnResampleArgs {
    const float *in;                // B clips, row stride n_in_max
    const int32_t *n_in;            // [B]
    float *out;                     // (B, n_out_max)
    const float *bank;            // wrnn_resample_device_bank: [p][taps], phase-major (resample.hip names the knob for the other layout)
    int64_t n_in_max, n_out_max;
    int32_t p, q, half, taps;
};

// Host only.  WRNN_OK, WRNN_ERR_INVALID (a rate <= 0) or WRNN_ERR_UNSUPPORTED (scale < 1/32, or a bank above WRNN_RS_MAX_BANK entries);
// the bank is built only for WRNN_OK.
int wrnn_resample_build_plan(int64_t src_rate, int64_t dst_rate, WrnnResamplePlan *out);
// The bank in the layout the kernel reads.
std::vector<float> wrnn_resample_device_bank(const WrnnResamplePlan &plan);
hipError_t wrnn_launch_resample(const WrnnResampleArgs &a, int B, int span_max, hipStream_t s);
