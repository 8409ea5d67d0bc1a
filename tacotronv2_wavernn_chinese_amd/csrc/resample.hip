// The resampler: y[t] = sum_{j = -half + 1 .. half} h(j - r / p) x[n + j] with n = (t q) / p, r = (t q) % p in 64-bit integers, for
// src -> dst = q : p in lowest terms; h is the Kaiser-windowed sinc of the `kaiser_best` family (64 zero crossings), evaluated exactly at
// the p x 2 half tap positions on the host in float64 and rounded to float32 once.  One workgroup of 256 threads per tile of 256
// outputs, grid (tiles, B): the input span the tile needs is staged in LDS (zeros outside the clip), every thread accumulates its own
// output in float32, and outputs at or past the clip's own length are written as zeros up to n_out_max.  Nothing crosses workgroups.
//
// Knob (tools/build_variant.sh): the bank lies on the device phase-major, [p][taps], every lane walking its own contiguous row (four taps
// are one 16-byte load); -DRS_PHASE_MAJOR=0 builds the tap-major [taps][p], in which one step of a wave reads one run of at most p floats.
// Phase-major measured 1.35x (one 5 s clip at 48 kHz) to 1.7x (ragged queue of 8) faster.
#include <cmath>

#include "../../include/wavernn_amd.h"
#include "resample_internal.h"

#ifndef RS_PHASE_MAJOR
#define RS_PHASE_MAJOR 1
#endif

namespace {

__global__ void __launch_bounds__(WRNN_RS_THREADS) resample_kernel(WrnnResampleArgs a) {
    extern __shared__ __attribute__((aligned(16))) float span[];
    const int b = blockIdx.y, tid = threadIdx.x;
    long n = a.n_in[b];
    if (n > a.n_in_max) n = a.n_in_max;
    if (n < 0) n = 0;
    long n_out = (n * a.p + a.q - 1) / a.q;
    if (n_out > a.n_out_max) n_out = a.n_out_max;
    const long t0 = (long)blockIdx.x * WRNN_RS_TILE, t = t0 + tid;
    float *out = a.out + (long)b * a.n_out_max;
    if (t0 >= n_out) {               // workgroup-uniform: the whole tile lies past the clip's own end
        if (t < a.n_out_max) out[t] = 0.0f;
        return;
    }
    const long t_last = (t0 + WRNN_RS_TILE - 1 < n_out ? t0 + WRNN_RS_TILE : n_out) - 1;
    const long n0 = (t0 * a.q) / a.p;
    const long lo = n0 - a.half + 1;                                 // clip index of span[0]
    const int len = (int)((t_last * a.q) / a.p + a.half - lo + 1);   // <= ceil((TILE - 1) q / p) + taps, the launch's LDS size
    const float *x = a.in + (long)b * a.n_in_max;
    for (int i = tid; i < len; i += WRNN_RS_THREADS) {
        const long j = lo + i;
        span[i] = (j >= 0 && j < n) ? x[j] : 0.0f;                   // whatever the buffer holds past the clip is never read
    }
    __syncthreads();
    if (t >= a.n_out_max) return;
    if (t >= n_out) {
        out[t] = 0.0f;
        return;
    }
    const long tq = t * a.q;
    const int r = (int)(tq % a.p);
    const float *s = span + (int)(tq / a.p - n0);                    // s[k] = x[n + k - half + 1]
#if RS_PHASE_MAJOR
    const float *h = a.bank + (long)r * a.taps;
    const int p = 1;
#else
    const float *h = a.bank + r;
    const int p = a.p;
#endif
    float acc0 = 0.0f, acc1 = 0.0f, acc2 = 0.0f, acc3 = 0.0f;       // taps is even; four chains hide the LDS and cache latency
    int k = 0;
    for (; k + 4 <= a.taps; k += 4) {
        acc0 = fmaf(h[(long)k * p], s[k], acc0);
        acc1 = fmaf(h[(long)(k + 1) * p], s[k + 1], acc1);
        acc2 = fmaf(h[(long)(k + 2) * p], s[k + 2], acc2);
        acc3 = fmaf(h[(long)(k + 3) * p], s[k + 3], acc3);
    }
    for (; k < a.taps; ++k) acc0 = fmaf(h[(long)k * p], s[k], acc0);
    out[t] = (acc0 + acc1) + (acc2 + acc3);
}

// I0(x) by its power series sum ((x / 2)^k / k!)^2: every term is positive, so nothing cancels (x <= beta here, about 40 terms)
double bessel_i0(double x) {
    const double y = 0.25 * x * x;
    double term = 1.0, sum = 1.0;
    for (int k = 1; k < 500; ++k) {
        term *= y / ((double)k * (double)k);
        sum += term;
        if (term < 1e-18 * sum) break;
    }
    return sum;
}

int64_t gcd64(int64_t a, int64_t b) {
    while (b) {
        const int64_t c = a % b;
        a = b;
        b = c;
    }
    return a;
}

}  // namespace

int wrnn_resample_build_plan(int64_t src_rate, int64_t dst_rate, WrnnResamplePlan *out) {
    if (src_rate < 1 || dst_rate < 1 || src_rate > INT32_MAX || dst_rate > INT32_MAX) return WRNN_ERR_INVALID;
    const int64_t g = gcd64(src_rate, dst_rate), p = dst_rate / g, q = src_rate / g;
    if (p * WRNN_RS_MIN_SCALE_INV < q) return WRNN_ERR_UNSUPPORTED;
    const int64_t half = q > p ? (WRNN_RS_ZEROS * q + p - 1) / p : WRNN_RS_ZEROS;   // ceil(64 / scale)
    if (p * 2 * half > WRNN_RS_MAX_BANK) return WRNN_ERR_UNSUPPORTED;
    out->p = (int32_t)p; out->q = (int32_t)q; out->half = (int32_t)half; out->taps = (int32_t)(2 * half);
    out->span_max = (int32_t)(((WRNN_RS_TILE - 1) * q + p - 1) / p + 2 * half);
    // the filter parameters of the `kaiser_best` family
    const double rolloff = 0.9475937167399596, beta = 14.769656459379492, pi = 3.141592653589793;
    const double scale = q > p ? (double)p / (double)q : 1.0, i0_beta = bessel_i0(beta);
    out->bank.resize((size_t)p * (size_t)out->taps);
    for (int64_t r = 0; r < p; ++r)
        for (int64_t k = 0; k < 2 * half; ++k) {
            const double u = (double)(k - half + 1) - (double)r / (double)p, v = scale * std::fabs(u);
            double hv = 0.0;
            if (v < (double)WRNN_RS_ZEROS) {
                const double xs = pi * (rolloff * v), sinc = xs == 0.0 ? 1.0 : std::sin(xs) / xs, w = v / (double)WRNN_RS_ZEROS;
                hv = scale * rolloff * sinc * bessel_i0(beta * std::sqrt(1.0 - w * w)) / i0_beta;
            }
            out->bank[(size_t)r * out->taps + k] = (float)hv;
        }
    return WRNN_OK;
}

std::vector<float> wrnn_resample_device_bank(const WrnnResamplePlan &pl) {
#if RS_PHASE_MAJOR
    return pl.bank;
#else
    std::vector<float> bt(pl.bank.size());
    for (int r = 0; r < pl.p; ++r)
        for (int k = 0; k < pl.taps; ++k) bt[(size_t)k * pl.p + r] = pl.bank[(size_t)r * pl.taps + k];
    return bt;
#endif
}

hipError_t wrnn_launch_resample(const WrnnResampleArgs &a, int B, int span_max, hipStream_t s) {
    const unsigned tiles = (unsigned)((a.n_out_max + WRNN_RS_TILE - 1) / WRNN_RS_TILE);
    hipLaunchKernelGGL(resample_kernel, dim3(tiles, (unsigned)B), dim3(WRNN_RS_THREADS), (size_t)span_max * sizeof(float), s, a);
    return hipGetLastError();
}
