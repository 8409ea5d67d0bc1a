// Wav conditioning on the device, between the resampler and the mel front end / quantiser: trim leading and trailing silence
// (librosa.effects.trim as tacotron/datasets/audio.py:71-77 calls it: frame energies of the reflect-padded clip against the loudest
// frame) and rescale to the peak (preprocessor.py:72, wav / abs(wav).max() * rescaling_max).  Three launches over ragged (B, n_max)
// buffers with device-resident lengths, nothing waits on the host:
//   energy_kernel  one wave per frame: lane l adds the squares of samples l, l + 64, ... of the frame in float64, in that order, then the
//                  64 partial sums fold by halves (32, 16, ... 1).  The order depends on the frame alone, not on B or the row, so a row
//                  of a ragged call equals the call on that clip alone bit for bit.
//   decide_kernel  one workgroup per clip: loudest frame, first and last frame above the threshold, the bounds, then max |x| over
//                  [start, end).  min and max do not round, so the order of these reductions does not matter.
//   gather_kernel  grid (tiles, B): out[b, i] = x[b, start + i] / peak * target for i < end - start, zero from there to n_out_max.
// The Makefile builds this file with -ffp-contract=off, and no fast-math flag belongs on it: the scale is NumPy's float32 divide, then
// its float32 multiply.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cmath>

#include "../../include/wavernn_amd.h"

namespace {

constexpr int CD_THREADS = 256;
constexpr int CD_WAVES = CD_THREADS / 64;
constexpr int CD_GATHER_PER_THREAD = 4;
constexpr int CD_GATHER_TILE = CD_THREADS * CD_GATHER_PER_THREAD;
constexpr double CD_AMIN = 1e-10;

struct ClipRecord {   // what decide_kernel leaves for gather_kernel, one per clip behind the (B, F_max) energies
    int32_t start;
    float peak;
};
static_assert(sizeof(ClipRecord) == sizeof(double), "one float64 slot of the workspace per clip");

struct ConditionArgs {
    const float *wav;
    const int32_t *n;
    int64_t n_max, n_out_max;
    int32_t trim, frame_length, hop, F_max;
    double ratio;     // 10 ** (-top_db / 10)
    float target;     // 0: no scaling
    double *energy;
    ClipRecord *record;
    float *out;
    int32_t *n_out, *bounds;
    float *peak;
};

__device__ __forceinline__ int64_t clip_len(const ConditionArgs &a, int b) {
    int64_t n = a.n[b];
    if (n > a.n_max) n = a.n_max;
    return n < 0 ? 0 : n;
}

// grid (ceil(F_max / 4), B), one wave per frame.  Frames at and past the clip's own 1 + n / hop are written as zeros.
__global__ __launch_bounds__(CD_THREADS) void energy_kernel(ConditionArgs a) {
    const int b = blockIdx.y, lane = threadIdx.x & 63;
    const int64_t f = (int64_t)blockIdx.x * CD_WAVES + (threadIdx.x >> 6);
    if (f >= a.F_max) return;   // wave-uniform
    const int64_t n = clip_len(a, b), pad = a.frame_length / 2;
    double *e = a.energy + (int64_t)b * a.F_max + f;
    if (f > n / a.hop || n < 1) {
        if (lane == 0) *e = 0.0;
        return;
    }
    const float *x = a.wav + (int64_t)b * a.n_max;
    // an odd frame_length pads one sample less than the last frame wants when hop divides n: that frame is the shorter slice NumPy takes
    const int64_t j0 = f * a.hop, avail = n + 2 * pad - j0;
    const int count = (int)(avail < a.frame_length ? avail : a.frame_length);
    double acc = 0.0;
    for (int k = lane; k < count; k += 64) {
        int64_t i = j0 + k - pad;                    // numpy.pad(mode='reflect'): ... x[2] x[1] | x[0] ... x[n - 1] | x[n - 2] x[n - 3] ...
        if (i < 0) i = -i;
        if (i >= n) i = 2 * (n - 1) - i;
        i = i < 0 ? 0 : i > n - 1 ? n - 1 : i;       // a clip shorter than pad + 1 (refused on the host where its length is known) stays inside itself
        const double v = (double)x[i];
        acc += v * v;
    }
    for (int off = 32; off > 0; off >>= 1) acc += __shfl_down(acc, off, 64);
    if (lane == 0) *e = acc / (double)count;
}

// grid (B), one workgroup per clip
__global__ __launch_bounds__(CD_THREADS) void decide_kernel(ConditionArgs a) {
    __shared__ double s_max[CD_WAVES];
    __shared__ int s_first[CD_WAVES], s_last[CD_WAVES];
    __shared__ float s_peak[CD_WAVES];
    __shared__ int64_t s_bounds[2];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t n = clip_len(a, b);
    int64_t start = 0, end = n;
    if (a.trim) {
        int64_t frames = 1 + n / a.hop;
        const int F = (int)(frames < a.F_max ? frames : a.F_max);
        const double *e = a.energy + (int64_t)b * a.F_max;
        double m = 0.0;
        for (int f = tid; f < F; f += CD_THREADS) m = fmax(m, e[f]);          // fmax drops a NaN
        for (int off = 32; off > 0; off >>= 1) m = fmax(m, __shfl_down(m, off, 64));
        if (lane == 0) s_max[wave] = m;
        __syncthreads();
        m = s_max[0];
        for (int w = 1; w < CD_WAVES; ++w) m = fmax(m, s_max[w]);
        const double thr = a.ratio * fmax(CD_AMIN, m);
        int first = INT32_MAX, last = -1;
        for (int f = tid; f < F; f += CD_THREADS)
            if (fmax(CD_AMIN, e[f]) > thr) {
                first = first < f ? first : f;
                last = f;
            }
        for (int off = 32; off > 0; off >>= 1) {
            const int of = __shfl_down(first, off, 64), ol = __shfl_down(last, off, 64);
            first = first < of ? first : of;
            last = last > ol ? last : ol;
        }
        if (lane == 0) {
            s_first[wave] = first;
            s_last[wave] = last;
        }
        __syncthreads();
        if (tid == 0) {
            for (int w = 1; w < CD_WAVES; ++w) {
                first = first < s_first[w] ? first : s_first[w];
                last = last > s_last[w] ? last : s_last[w];
            }
            int64_t s = 0, t = 0;                     // no frame above the threshold (non-finite input only): an empty clip, as librosa returns
            if (last >= 0) {
                s = (int64_t)first * a.hop;
                t = ((int64_t)last + 1) * a.hop;
                if (t > n) t = n;
                if (s > t) s = t;
            }
            s_bounds[0] = s;
            s_bounds[1] = t;
        }
        __syncthreads();
        start = s_bounds[0];
        end = s_bounds[1];
    }
    const float *x = a.wav + (int64_t)b * a.n_max;
    float pk = 0.0f;
    for (int64_t i = start + tid; i < end; i += CD_THREADS) pk = fmaxf(pk, fabsf(x[i]));
    for (int off = 32; off > 0; off >>= 1) pk = fmaxf(pk, __shfl_down(pk, off, 64));
    if (lane == 0) s_peak[wave] = pk;
    __syncthreads();
    if (tid == 0) {
        for (int w = 1; w < CD_WAVES; ++w) pk = fmaxf(pk, s_peak[w]);
        ClipRecord r;
        r.start = (int32_t)start;
        r.peak = pk;
        a.record[b] = r;
        a.n_out[b] = (int32_t)(end - start);
        if (a.bounds) {
            a.bounds[2 * b] = (int32_t)start;
            a.bounds[2 * b + 1] = (int32_t)end;
        }
        if (a.peak) a.peak[b] = pk;
    }
}

// grid (ceil(n_out_max / 1024), B): four coalesced runs of 256 samples per workgroup
__global__ __launch_bounds__(CD_THREADS) void gather_kernel(ConditionArgs a) {
    const int b = blockIdx.y;
    const ClipRecord r = a.record[b];
    const int64_t n_out = a.n_out[b];
    const float *x = a.wav + (int64_t)b * a.n_max + r.start;
    float *out = a.out + (int64_t)b * a.n_out_max;
    const bool scale = a.target != 0.0f && r.peak > 0.0f;   // peak == 0: digital silence stays as it is (the reference divides by zero)
    const int64_t i0 = (int64_t)blockIdx.x * CD_GATHER_TILE + threadIdx.x;
#pragma unroll
    for (int k = 0; k < CD_GATHER_PER_THREAD; ++k) {
        const int64_t i = i0 + (int64_t)k * CD_THREADS;
        if (i >= a.n_out_max) break;
        float v = 0.0f;
        if (i < n_out) {
            v = x[i];
            if (scale) v = __fmul_rn(__fdiv_rn(v, r.peak), a.target);
        }
        out[i] = v;
    }
}

bool window_ok(int32_t frame_length, int32_t hop) { return frame_length >= 2 && frame_length <= 8192 && hop >= 1 && hop <= frame_length; }

}  // namespace

extern "C" {

int64_t wrnn_condition_frames(int64_t n, int32_t frame_length, int32_t hop) {
    if (!window_ok(frame_length, hop) || n < frame_length / 2 + 1) return WRNN_ERR_INVALID;
    return 1 + n / hop;
}

int wrnn_condition(const float *wav_dev, int64_t n_max, const int32_t *n_dev, int32_t B, int32_t trim, double top_db, int32_t frame_length,
                   int32_t hop, float peak_target, double *energy_ws_dev, int32_t F_max, float *out_dev, int64_t n_out_max, int32_t *n_out_dev,
                   int32_t *bounds_dev, float *peak_dev, void *stream) {
    if (!trim && peak_target == 0.0f) return WRNN_ERR_INVALID;                      // nothing to do
    if (!(top_db > 0.0) || !std::isfinite(top_db) || !window_ok(frame_length, hop)) return WRNN_ERR_INVALID;
    if (!(peak_target >= 0.0f) || !std::isfinite(peak_target)) return WRNN_ERR_INVALID;
    if (B < 1 || B > 65535 || n_max < 1 || n_max > INT32_MAX || n_out_max < n_max || n_out_max > INT32_MAX || F_max < 1) return WRNN_ERR_INVALID;
    if (!wav_dev || !n_dev || !energy_ws_dev || !out_dev || !n_out_dev) return WRNN_ERR_INVALID;
    ConditionArgs a{};
    a.wav = wav_dev; a.n = n_dev; a.n_max = n_max; a.n_out_max = n_out_max;
    a.trim = trim != 0; a.frame_length = frame_length; a.hop = hop; a.F_max = F_max;
    a.ratio = std::pow(10.0, -top_db / 10.0);
    a.target = peak_target;
    a.energy = energy_ws_dev;
    a.record = reinterpret_cast<ClipRecord *>(energy_ws_dev + (int64_t)B * F_max);
    a.out = out_dev; a.n_out = n_out_dev; a.bounds = bounds_dev; a.peak = peak_dev;
    hipStream_t s = (hipStream_t)stream;
    if (a.trim)
        hipLaunchKernelGGL(energy_kernel, dim3((unsigned)((F_max + CD_WAVES - 1) / CD_WAVES), (unsigned)B), dim3(CD_THREADS), 0, s, a);
    hipLaunchKernelGGL(decide_kernel, dim3((unsigned)B), dim3(CD_THREADS), 0, s, a);
    hipLaunchKernelGGL(gather_kernel, dim3((unsigned)((n_out_max + CD_GATHER_TILE - 1) / CD_GATHER_TILE), (unsigned)B), dim3(CD_THREADS), 0, s, a);
    return hipGetLastError() == hipSuccess ? WRNN_OK : WRNN_ERR_HIP;
}

}  // extern "C"
