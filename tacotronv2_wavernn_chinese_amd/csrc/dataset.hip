// The training-data side on the device: wav -> class labels (wrnn_quantise) and resident corpus -> one training batch
// (wrnn_collate_windows).  Both are memory-bound element-wise kernels, plain HIP, 256-thread workgroups, 64-bit sample offsets.
// No fast-math flag may be put on this file: label_2_float below has to round like torch's float32 arithmetic on the host.  The
// Makefile builds it with -ffp-contract=off: the quantiser rounds after every operation, as NumPy does.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/wavernn_amd.h"

namespace {

constexpr int DS_THREADS = 256;
constexpr int64_t DS_MAX_BLOCKS = 4096;   // grid-stride above this: 16 workgroups per CU keep HBM busy, more only adds launch work

// encode_mu_law(x, 2**bits) (wavernn/utils/dsp.py:92-95) or float_2_label(x, bits) (:12-15) + the collate's .astype(int64)
// (dataset.py:118), in float64 and in the reference's operation order.  A NaN counts as clipped and becomes label 0.
__global__ __launch_bounds__(DS_THREADS) void quantise_kernel(const float *__restrict__ wav, int64_t n, double mu, int mu_law,
                                                               int32_t *__restrict__ labels, unsigned long long *n_clipped) {
    const int64_t stride = (int64_t)gridDim.x * DS_THREADS;
    const double log1p_mu = log(1.0 + mu);
    unsigned long long clipped = 0;
    for (int64_t i = (int64_t)blockIdx.x * DS_THREADS + threadIdx.x; i < n; i += stride) {
        const double x = (double)wav[i];
        const double ax = fabs(x);
        if (!(ax <= 1.0)) ++clipped;
        double v;
        if (mu_law) {
            const double sign = x > 0.0 ? 1.0 : x < 0.0 ? -1.0 : 0.0;
            const double fx = sign * log(1.0 + mu * ax) / log1p_mu;
            v = floor((fx + 1.0) / 2.0 * mu + 0.5);
        } else {
            v = (x + 1.0) * mu / 2.0;
        }
        v = fmin(fmax(v, 0.0), mu);   // fmax drops a NaN
        labels[i] = (int32_t)v;       // truncation: what .astype(np.int64) does to the linear labels
    }
    if (n_clipped && clipped) atomicAdd(n_clipped, clipped);
}

// label_2_float (dsp.py:8-9) as torch evaluates `2.0 * x.float() / (2 ** bits - 1.0) - 1.0` on a float32 tensor: every operation
// rounded to float32, the divide a correctly rounded one.
__device__ __forceinline__ float label_2_float(int32_t label, float denom) {
    return __fsub_rn(__fdiv_rn(__fmul_rn((float)label, 2.0f), denom), 1.0f);
}

struct CollateArgs {
    const int32_t *labels;
    const float *mels;
    const int64_t *label_off, *mel_off;
    const int32_t *frames, *utt, *win_off;
    int32_t n_mels, hop, pad, seq_len, win, y_float;
    float denom;
    float *x_out;
    void *y_out;
    float *mels_out;
};

// grid (ceil(max(seq_len, n_mels * win) / 256), B): thread i of row b writes x[b, i], y[b, i] and element i of the row's mel window.
// A row whose offset is outside the range the collate draws from (the host refuses those before the launch) is written as zeros, never read.
__global__ __launch_bounds__(DS_THREADS) void collate_kernel(CollateArgs a) {
    const int b = blockIdx.y;
    const int i = blockIdx.x * DS_THREADS + threadIdx.x;
    const int u = a.utt[b];
    const int64_t off = a.win_off[b];
    const int64_t s0 = (off + a.pad) * (int64_t)a.hop;
    // collate_vocoder's own range of offsets (dataset.py:109-110).  Inside it the mel window ends before frame frames - 2 - 2 * pad and the
    // label window before sample (frames - 1) * hop, and an utterance holds at least that many labels (the host checks it when it packs).
    const bool inside = off >= 0 && off < (int64_t)a.frames[u] - 2 - (a.win + 2 * a.pad);
    if (i < a.seq_len) {
        const int32_t *lab = a.labels + a.label_off[u] + s0 + i;
        const int32_t l0 = inside ? lab[0] : 0, l1 = inside ? lab[1] : 0;
        const int64_t o = (int64_t)b * a.seq_len + i;
        a.x_out[o] = inside ? label_2_float(l0, a.denom) : 0.0f;
        if (a.y_float)
            ((float *)a.y_out)[o] = inside ? label_2_float(l1, a.denom) : 0.0f;
        else
            ((int64_t *)a.y_out)[o] = (int64_t)l1;
    }
    const int n_win = a.n_mels * a.win;
    if (i < n_win) {
        // the corpus keeps an utterance frames-major, (frames, n_mels): the window is one contiguous run of win * n_mels floats, read
        // in order here and scattered into the (n_mels, win) layout the model takes
        const int f = i / a.n_mels, m = i - f * a.n_mels;
        const float v = inside ? a.mels[a.mel_off[u] + (off * a.n_mels + i)] : 0.0f;
        a.mels_out[((int64_t)b * a.n_mels + m) * a.win + f] = v;
    }
}

}  // namespace

extern "C" {

int wrnn_quantise(const float *wav_dev, int64_t n, int32_t bits, int32_t mu_law, int32_t *labels_dev, int64_t *n_clipped_dev, void *stream) {
    if (bits < 1 || bits > 16 || n < 0) return WRNN_ERR_INVALID;
    if (n == 0) return WRNN_OK;
    if (!wav_dev || !labels_dev) return WRNN_ERR_INVALID;
    const int64_t blocks = (n + DS_THREADS - 1) / DS_THREADS;
    const double mu = (double)((1 << bits) - 1);
    hipLaunchKernelGGL(quantise_kernel, dim3((unsigned)(blocks < DS_MAX_BLOCKS ? blocks : DS_MAX_BLOCKS)), dim3(DS_THREADS), 0, (hipStream_t)stream,
                       wav_dev, n, mu, (int)(mu_law != 0), labels_dev, (unsigned long long *)n_clipped_dev);
    return hipGetLastError() == hipSuccess ? WRNN_OK : WRNN_ERR_HIP;
}

int wrnn_collate_windows(const int32_t *labels_dev, const float *mels_dev, const int64_t *label_off_dev, const int64_t *mel_off_dev,
                         const int32_t *frames_dev, const int32_t *utt_dev, const int32_t *win_off_dev, int32_t B, int32_t n_mels, int32_t hop,
                         int32_t pad, int32_t seq_len, int32_t sig_bits, int32_t y_float, float *x_out, void *y_out, float *mels_out,
                         void *stream) {
    if (B < 1 || B > 65535 || n_mels < 1 || hop < 1 || pad < 0 || seq_len < 1 || seq_len % hop != 0 || sig_bits < 1 || sig_bits > 16)
        return WRNN_ERR_INVALID;
    if (!labels_dev || !mels_dev || !label_off_dev || !mel_off_dev || !frames_dev || !utt_dev || !win_off_dev || !x_out || !y_out || !mels_out)
        return WRNN_ERR_INVALID;
    const int64_t win = (int64_t)seq_len / hop + 2 * (int64_t)pad;
    if (win * n_mels > INT32_MAX / 2 || seq_len > INT32_MAX / 2) return WRNN_ERR_INVALID;   // the kernel's per-row index is an int
    CollateArgs a{};
    a.labels = labels_dev; a.mels = mels_dev; a.label_off = label_off_dev; a.mel_off = mel_off_dev;
    a.frames = frames_dev; a.utt = utt_dev; a.win_off = win_off_dev;
    a.n_mels = n_mels; a.hop = hop; a.pad = pad; a.seq_len = seq_len; a.win = (int32_t)win; a.y_float = y_float != 0;
    a.denom = (float)((1 << sig_bits) - 1);
    a.x_out = x_out; a.y_out = y_out; a.mels_out = mels_out;
    const int64_t per_row = seq_len > win * n_mels ? seq_len : win * n_mels;
    hipLaunchKernelGGL(collate_kernel, dim3((unsigned)((per_row + DS_THREADS - 1) / DS_THREADS), (unsigned)B), dim3(DS_THREADS), 0,
                       (hipStream_t)stream, a);
    return hipGetLastError() == hipSuccess ? WRNN_OK : WRNN_ERR_HIP;
}

}  // extern "C"
