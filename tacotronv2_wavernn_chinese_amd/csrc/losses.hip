// The two losses the reference's training script applies to WaveRNN.forward's output (wavernn_train.py:82,112-121):
//   RAW: F.cross_entropy(y_hat.transpose(1, 2).unsqueeze(-1), y.unsqueeze(-1))  -- mean over B*L of logsumexp(row) - row[y]
//   MOL: discretized_mix_logistic_loss(y_hat, y)  (wavernn/utils/distribution.py:16-84, num_classes = 65536,
//        log_scale_min = log(1e-14), reduce = True)  -- mean over B*L of -logsumexp_k(log_prob_k + log_softmax(logit)_k)
// Forward values only (the path here is inference; the numbers are what a training log would print).
// Both are HBM-read-bound row reductions: one wave per row (RAW, 4 KB per row) / one thread per row (MOL, 120 B per row, the arm
// values in double), per-block partial sums in double, summed in a fixed order by a second kernel (deterministic, no atomics).
#include "wrnn_internal.h"

namespace {

__device__ __forceinline__ float wave_sum_f(float v) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}
__device__ __forceinline__ float wave_max_f(float v) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v = fmaxf(v, __shfl_xor(v, off, 64));
    return v;
}

// grid ceil(rows / 4), block 256: wave w of block b reduces row 4 b + w
__global__ void __launch_bounds__(256) ce_rows_kernel(const float *__restrict__ logits, const int32_t *__restrict__ y, int NC,
                                                      long n_rows, double *__restrict__ partial, int *__restrict__ bad) {
    __shared__ double part[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long row = (long)blockIdx.x * 4 + wave;
    double nll = 0.0;
    if (row < n_rows) {
        const float *p = logits + (size_t)row * NC;
        float m = -INFINITY;
        for (int c = lane; c < NC; c += 64) m = fmaxf(m, p[c]);
        m = wave_max_f(m);
        float s = 0.0f;
        for (int c = lane; c < NC; c += 64) s += expf(p[c] - m);
        s = wave_sum_f(s);
        const int t = y[row];
        if (t < 0 || t >= NC) { if (lane == 0) atomicExch(bad, 1); }
        // -log_softmax(row)[y] as torch writes it: both terms are of the size of the loss.  (m + logf(s)) - p[t] rounds the log-sum-exp at
        // the spacing of m before p[t] comes off: 5e-5 off at logits near 1024, 1e-3 near 30 000, whatever the loss is
        else nll = (double)(logf(s) - (p[t] - m));
    }
    if (lane == 0) part[wave] = nll;
    __syncthreads();
    if (threadIdx.x == 0) partial[blockIdx.x] = (part[0] + part[1]) + (part[2] + part[3]);
}

__device__ __forceinline__ float sigmoid_ref(float x) { return 1.0f / (1.0f + expf(-x)); }
__device__ __forceinline__ double softplus_d(double x) { return x > 30.0 ? x : log1p(exp(x)); }   // F.softplus; past 30 log1p(exp(x)) == x in double
__device__ __forceinline__ double sigmoid_d(double x) { return 1.0 / (1.0 + exp(-x)); }

// grid ceil(rows / 256), block 256: one thread per (b, t) row of y_hat (rows, 3 * nr_mix).
// WHICH arm a (row, component) takes is decided as the reference's float32 arithmetic decides it: y against +-0.999f, and the float32
// difference of float32 sigmoids against 1e-5f (the same expression `mol_grad_kernel` uses, so loss and gradient are on one arm).  The
// VALUE of the arm and everything after it is evaluated in double and rounded to float32 once, at the end (`mean_kernel`): in float32 the
// row value itself is a few ulp off, and against a float64 restatement that is up to 18x what the reference's own float32 result loses
// on rows where that result happens to round well (edge rows, 1000 of them: 1.26e-7 against 6.8e-9).  The reference's blends
// `c * arm_a + (1 - c) * arm_b` multiply the arm not taken by 0: written as a selection here.  30 doubles per row, B*L rows: next to the
// GEMMs of a training step this costs nothing.
__global__ void __launch_bounds__(256) mol_rows_kernel(const float *__restrict__ y_hat, const float *__restrict__ yv, int nr_mix,
                                                       long n_rows, float num_classes, double log_scale_min,
                                                       double *__restrict__ partial) {
    __shared__ double part[4];
    const long row = (long)blockIdx.x * 256 + threadIdx.x;
    double loss = 0.0;
    if (row < n_rows) {
        const float *p = y_hat + (size_t)row * 3 * nr_mix;
        const float yf = yv[row];
        const double y = (double)yf;
        // log_softmax(logit_probs)                                   (:77)
        double lm = -INFINITY;
        for (int k = 0; k < nr_mix; ++k) lm = fmax(lm, (double)p[k]);
        double ls = 0.0;
        for (int k = 0; k < nr_mix; ++k) ls += exp((double)p[k] - lm);
        const double lse_logit = lm + log(ls);
        const double half_bin = 1.0 / ((double)num_classes - 1.0);
        const double log_half = log(((double)num_classes - 1.0) / 2.0);
        const float half_bin_f = 1.0f / (num_classes - 1.0f), ls_min_f = (float)log_scale_min;
        double lp[16];
        double mx = -INFINITY;
        for (int k = 0; k < nr_mix; ++k) {
            const double mean = (double)p[nr_mix + k];
            const double lsc = fmax((double)p[2 * nr_mix + k], log_scale_min);  // :31
            const double cy = y - mean;                                         // :36
            const double inv = exp(-lsc);                                       // :37
            // the float32 cdf_delta the reference compares with 1e-5          (:39-54, :69)
            const float inv_f = expf(-fmaxf(p[2 * nr_mix + k], ls_min_f)), cy_f = yf - p[nr_mix + k];
            const float cdf_f = sigmoid_ref(inv_f * (cy_f + half_bin_f)) - sigmoid_ref(inv_f * (cy_f - half_bin_f));
            double v;
            if (yf < -0.999f) {                                                 // :76  log_cdf_plus :45
                const double plus_in = inv * (cy + half_bin);
                v = plus_in - softplus_d(plus_in);
            } else if (yf > 0.999f) {                                           // :74  log_one_minus_cdf_min :49
                v = -softplus_d(inv * (cy - half_bin));
            } else if (cdf_f > 1e-5f) {                                         // :69-72
                const double cdf_delta = sigmoid_d(inv * (cy + half_bin)) - sigmoid_d(inv * (cy - half_bin));
                v = log(fmax(cdf_delta, 1e-12));
            } else {                                                            // log_pdf_mid :57
                const double mid_in = inv * cy;
                v = mid_in - lsc - 2.0 * softplus_d(mid_in) - log_half;
            }
            v += (double)p[k] - lse_logit;                                      // :75-77
            lp[k] = v;
            mx = fmax(mx, v);
        }
        double s = 0.0;
        for (int k = 0; k < nr_mix; ++k) s += exp(lp[k] - mx);                  // log_sum_exp :6-12
        loss = -(mx + log(s));
    }
    // block sum in a fixed order
    for (int off = 32; off >= 1; off >>= 1) loss += __shfl_xor(loss, off, 64);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = loss;
    __syncthreads();
    if (threadIdx.x == 0) partial[blockIdx.x] = (part[0] + part[1]) + (part[2] + part[3]);
}

__global__ void __launch_bounds__(256) mean_kernel(const double *__restrict__ partial, long n, double inv_count, const int *__restrict__ bad,
                                                   float *__restrict__ out) {
    __shared__ double sh[256];
    double acc = 0.0;
    for (long i = threadIdx.x; i < n; i += 256) acc += partial[i];
    sh[threadIdx.x] = acc;
    __syncthreads();
    for (int s = 128; s >= 1; s >>= 1) {
        if ((int)threadIdx.x < s) sh[threadIdx.x] += sh[threadIdx.x + s];
        __syncthreads();
    }
    if (threadIdx.x == 0) *out = *bad ? __builtin_nanf("") : (float)(sh[0] * inv_count);   // a target outside [0, n_classes): NaN (torch raises)
}

}  // namespace

hipError_t wrnn_launch_loss(int mode, const float *y_hat, const void *y, int NC, long n_rows, double *partial, int *bad, float *out,
                            hipStream_t s) {
    (void)hipGetLastError();
    long nblk;
    if (mode == WRNN_MODE_RAW) {
        nblk = (n_rows + 3) / 4;
        hipLaunchKernelGGL(ce_rows_kernel, dim3((unsigned)nblk), dim3(256), 0, s, y_hat, (const int32_t *)y, NC, n_rows, partial, bad);
    } else {
        nblk = (n_rows + 255) / 256;
        hipLaunchKernelGGL(mol_rows_kernel, dim3((unsigned)nblk), dim3(256), 0, s, y_hat, (const float *)y, NC / 3, n_rows, 65536.0f,
                           -32.23619130191664, partial);
    }
    hipLaunchKernelGGL(mean_kernel, dim3(1), dim3(256), 0, s, partial, nblk, 1.0 / (double)n_rows, bad, out);
    return hipGetLastError();
}
