// Tacotron-2 inference on the device: symbol ids -> mel.  The definitions are in the header's section.
//   taco_embed_kernel    grid (Tx_max, B)                                  the embedding rows of an utterance's symbols, zeros past its end
//   taco_conv_kernel     grid (ceil(T_max / 8), B, ceil(Cout / 64))        conv1d 'same' + bias -> activation -> folded BatchNorm over 8 time
//                                                                          steps per workgroup, the input tile in LDS.  With one tap it is the
//                                                                          dense layer over time: the LSTM input projections for all t, the
//                                                                          memory-layer keys, the postnet's projection
//   taco_enc_lstm_kernel grid (2, B)                                       one workgroup per direction per utterance: h, c and the gates in LDS
//   taco_decoder_kernel  grid (B)                                          ONE persistent workgroup per utterance: the whole decoder loop, its
//                                                                          state in LDS, the weights streamed from L2; the stop is decided here
//   taco_finish_kernel   grid (ceil(S r M / 256), B)                       residual, clips, the map to [0, 1]
// A stream (wrnn_taco_stream_*) runs the same step and the same convolution from state kept in device memory between pushes:
//   taco_decoder_kernel<true>  grid (B)                                up to n more steps of every unfinished utterance: the other
//                                                                          instantiation of the decoder kernel, with a load at entry and a
//                                                                          store at exit
//   taco_conv_kernel<true>     grid (ceil((n r + held back) / 8) + 1, B, ..)  the conv kernel over the rows of a layer that this push made
//                                                                          final, the range read from the stream's state
//   taco_finish_window_kernel  grid (ceil((n r + halo) M / 256), B)        taco_finish_kernel's arithmetic over the released rows
// Nothing crosses workgroups, nothing spins, no atomics; every sum has a fixed order that does not depend on the batch, so an utterance of
// a ragged batch gives the bits of the call on it alone.  All layouts are the reference's own ([in, out] dense kernels, [tap, in, out]
// conv kernels): thread j of a layer owns output column j, and a wave reads 64 neighbouring floats of one weight row.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "device_util.h"
#include "handle_common.h"
#include "taco_internal.h"

namespace {

constexpr int CONV_THREADS = 256;
constexpr int CONV_TT = 8;          // time steps per workgroup of the conv kernel
constexpr int LOOP_THREADS = 1024;  // the recurrences: 16 waves on one CU
constexpr int MAX_DEC_LAYERS = 4;
constexpr int MAX_TAPS = 64;
constexpr size_t LDS_LIMIT = 64 * 1024;
// A stream's integers per utterance, in device memory between pushes.  WAS: the utterance had finished before this push (nothing is new).
enum { ST_MAX_ATT = 0, ST_POS_REC, ST_FIRST_STOP, ST_STEP, ST_FINISHED, ST_PREV, ST_WAS, ST_INTS = 8 };

__device__ inline float sigmoid_acc(float x) { return 1.0f / (1.0f + expf(-x)); }

// y[j] = init[j] + sum_i W[i N + j] x[i], j < N, i < K, by the whole workgroup.  x, y, scratch in LDS (scratch: 4 blockDim.x floats, 16-byte
// aligned); init in LDS or global, or null; W 16-byte aligned.  One CU streams the weights from beyond its L2, a microsecond or so per
// round of loads, so what counts is the bytes in flight per round: with N a multiple of 4 a thread owns 4 neighbouring columns (one
// 16-byte load per row) and the rows are cut into S = blockDim.x / (N / 4 padded to 64) slices, one per group of threads; the slices'
// partial sums are added in slice order.  Other N: one column per thread, the same slicing.  A fixed order either way.  Ends with a
// barrier: y is visible to every thread.  The caller has made x visible.
__device__ void matvec(const float *__restrict__ W, const float *init, const float *x, int K, int N, float *y, float *scratch) {
    const int NT = blockDim.x, tid = threadIdx.x;
    if ((N & 3) == 0 && (((N >> 2) + 63) & ~63) <= NT) {
        const int G = N >> 2, Gp = (G + 63) & ~63, S = NT / Gp;
        const int s = tid / Gp, j = tid - s * Gp;
        const int slice = (K + S - 1) / S;
        if (s < S && j < G) {
            const int i0 = s * slice, i1 = min(K, i0 + slice);
            float4 acc = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            const float4 *w = reinterpret_cast<const float4 *>(W) + j;
#pragma unroll 8
            for (int i = i0; i < i1; ++i) {
                const float4 v = w[(long)i * G];
                const float xi = x[i];
                acc.x += v.x * xi; acc.y += v.y * xi; acc.z += v.z * xi; acc.w += v.w * xi;
            }
            reinterpret_cast<float4 *>(scratch)[s * Gp + j] = acc;
        }
        __syncthreads();
        for (int n = tid; n < N; n += NT) {
            float acc = init ? init[n] : 0.0f;
            for (int q = 0; q < S; ++q) acc += scratch[(q * Gp + (n >> 2)) * 4 + (n & 3)];
            y[n] = acc;
        }
        __syncthreads();
        return;
    }
    const int Np = (N + 63) & ~63;
    const int S = NT / Np;
    if (S <= 1) {
        for (int j = tid; j < N; j += NT) {
            float acc = init ? init[j] : 0.0f;
            const float *w = W + j;
#pragma unroll 8
            for (int i = 0; i < K; ++i) acc += w[(long)i * N] * x[i];
            y[j] = acc;
        }
        __syncthreads();
        return;
    }
    const int s = tid / Np, j = tid - s * Np;
    const int slice = (K + S - 1) / S;
    if (s < S && j < N) {
        const int i0 = s * slice, i1 = min(K, i0 + slice);
        float acc = 0.0f;
        const float *w = W + j;
#pragma unroll 8
        for (int i = i0; i < i1; ++i) acc += w[(long)i * N] * x[i];
        scratch[s * Np + j] = acc;
    }
    __syncthreads();
    if (tid < N) {
        float acc = init ? init[tid] : 0.0f;
        for (int q = 0; q < S; ++q) acc += scratch[q * Np + tid];
        y[tid] = acc;
    }
    __syncthreads();
}

// The same value in every thread: the waves' partial results in wave order.  red: 16 floats of LDS.  Two barriers.
__device__ float block_sum(float v, float *red) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
    const int nw = blockDim.x >> 6;
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    float t = 0.0f;
    for (int w = 0; w < nw; ++w) t += red[w];
    return t;
}
__device__ float block_max(float v, float *red) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v = fmaxf(v, __shfl_xor(v, off, 64));
    const int nw = blockDim.x >> 6;
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    float t = red[0];
    for (int w = 1; w < nw; ++w) t = fmaxf(t, red[w]);
    return t;
}

struct EmbedArgs {
    const int32_t *ids;   // (B, Tx_max)
    const int32_t *tx;    // (B)
    const float *table;   // (V, E)
    float *out;           // (B, Tx_max, E)
    int32_t Tx_max, E, V;
};
__global__ void __launch_bounds__(CONV_THREADS) taco_embed_kernel(EmbedArgs g) {
    const int t = blockIdx.x, b = blockIdx.y;
    const int Tx = min(max(g.tx[b], 0), g.Tx_max);
    float *out = g.out + ((long)b * g.Tx_max + t) * g.E;
    int id = g.ids[(long)b * g.Tx_max + t];
    id = min(max(id, 0), g.V - 1);          // the host has refused ids outside the table; this keeps the read inside it regardless
    for (int e = threadIdx.x; e < g.E; e += CONV_THREADS) out[e] = t < Tx ? g.table[(long)id * g.E + e] : 0.0f;
}

struct ConvArgs {
    const float *in;      // (B, T_max, Cin)
    const float *w;       // (taps, Cin, Cout)
    const float *bias;    // (Cout) or null
    const float *bn_s;    // (Cout) or null: gamma / sqrt(var + eps)
    const float *bn_b;    // (Cout): beta - mean * bn_s
    float *out;           // (B, T_max, Cout)
    const int32_t *len;   // (B): the utterance's rows are len[b] * len_mul, clamped to 0 .. T_max
    int32_t len_mul, T_max, Cin, Cout, taps, act;   // act 0: none, 1: relu, 2: tanh
};
struct ConvWindow {       // the windowed variant's own arguments; ConvArgs.len is unused there
    const int32_t *win;   // the stream's integers (B, ST_INTS)
    int32_t held;         // rows this layer's output is held back behind the decoder while the utterance runs
};
// A workgroup takes CONV_TT time steps of 64 output channels; its 4 waves split the taps x Cin products between them (the chain of
// dependent weight loads is what a small grid waits for) and add their partial sums in wave order.  Row (q + k) of the tile, channel c,
// is tile[q Cin + (k Cin + c)]: the products of one output are one flat run of taps x Cin weights against a flat run of the tile.
// WINDOW: the rows [lo, hi) that became final at this layer in the stream's last push.  The tiles start at multiples of CONV_TT, as in
// the whole-utterance launch: the order of an output's sum does not depend on the tile, but the compiler fuses the multiply-adds of some
// of a tile's CONV_TT rows and not of others, so a row gives the offline bits only at the offline position in its tile.  Rows of the
// first tile below lo are computed again and not written.  L is the decoder's row count so far: while the utterance runs every row
// read lies below it, and once it has finished it is the true length.
template <bool WINDOW>
__global__ void __launch_bounds__(CONV_THREADS) taco_conv_kernel(ConvArgs g, ConvWindow cw) {
    extern __shared__ __align__(16) float tile[];         // (CONV_TT + taps - 1, Cin): rows t0 - left .. of the input, zeros outside the utterance
    __shared__ float part[CONV_THREADS / 64][CONV_TT][64];
    const int b = blockIdx.y, wave = threadIdx.x >> 6, lane = threadIdx.x & 63, co = blockIdx.z * 64 + lane;
    int t0 = blockIdx.x * CONV_TT, lo = 0, hi = g.T_max;
    long lraw;
    if constexpr (WINDOW) {
        const int32_t *si = cw.win + (long)b * ST_INTS;
        if (si[ST_WAS]) return;
        lraw = (long)si[ST_STEP] * g.len_mul;
    } else {
        lraw = (long)g.len[b] * g.len_mul;
    }
    const int L = (int)(lraw < 0 ? 0 : lraw > g.T_max ? g.T_max : lraw);
    if constexpr (WINDOW) {
        const int32_t *si = cw.win + (long)b * ST_INTS;
        const long praw = (long)si[ST_PREV] * g.len_mul - cw.held;
        lo = (int)(praw < 0 ? 0 : praw > L ? L : praw);
        hi = si[ST_FINISHED] ? L : max(0, L - cw.held);
        t0 += lo / CONV_TT * CONV_TT;
        if (t0 >= hi) return;   // the whole workgroup
    }
    const int left = (g.taps - 1) / 2, rows = CONV_TT + g.taps - 1;
    const float *in = g.in + (long)b * g.T_max * g.Cin;
    for (int x = threadIdx.x; x < rows * g.Cin; x += CONV_THREADS) {
        const int r = x / g.Cin, c = x - r * g.Cin, t = t0 - left + r;
        tile[x] = (t >= 0 && t < L) ? in[(long)t * g.Cin + c] : 0.0f;
    }
    __syncthreads();
    float acc[CONV_TT];
#pragma unroll
    for (int q = 0; q < CONV_TT; ++q) acc[q] = 0.0f;
    if (co < g.Cout) {
        const int KK = g.taps * g.Cin, slice = (KK + 3) / 4, k0 = wave * slice, k1 = min(KK, k0 + slice);
        const float *w = g.w + co;
#pragma unroll 4
        for (int kk = k0; kk < k1; ++kk) {
            const float wv = w[(long)kk * g.Cout];
#pragma unroll
            for (int q = 0; q < CONV_TT; ++q) acc[q] += wv * tile[q * g.Cin + kk];
        }
    }
#pragma unroll
    for (int q = 0; q < CONV_TT; ++q) part[wave][q][lane] = acc[q];
    __syncthreads();
    if (co >= g.Cout) return;
    const float bias = g.bias ? g.bias[co] : 0.0f;
    const float s = g.bn_s ? g.bn_s[co] : 1.0f, sh = g.bn_s ? g.bn_b[co] : 0.0f;
    for (int q = wave; q < CONV_TT; q += CONV_THREADS / 64) {
        const int t = t0 + q;
        if constexpr (WINDOW) {
            if (t >= hi) break;
            if (t < lo) continue;
        } else {
            if (t >= g.T_max) break;
        }
        float v = bias;
        for (int p = 0; p < CONV_THREADS / 64; ++p) v += part[p][q][lane];
        if (g.act == 1) v = fmaxf(v, 0.0f);
        else if (g.act == 2) v = tanhf(v);
        g.out[((long)b * g.T_max + t) * g.Cout + co] = t < L ? v * s + sh : 0.0f;
    }
}

struct EncLstmArgs {
    const float *xproj[2];   // (B, Tx_max, 4H) per direction: x W_x + bias
    const float *whh[2];     // (H, 4H): the rows of the cell's kernel that multiply h
    const int32_t *tx;       // (B)
    float *memory;           // (B, Tx_max, 2H): forward outputs, then backward
    int32_t Tx_max, H;
    float zoneout;
};
// LDS: scratch[4 blockDim.x], h[H], c[H], gates[4H]
__global__ void __launch_bounds__(LOOP_THREADS) taco_enc_lstm_kernel(EncLstmArgs g) {
    extern __shared__ __align__(16) float lds[];
    const int H = g.H, dir = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
    float *scratch = lds, *h = scratch + 4 * blockDim.x, *c = h + H, *gates = c + H;
    const int Tx = min(max(g.tx[b], 0), g.Tx_max);
    for (int j = tid; j < H; j += blockDim.x) { h[j] = 0.0f; c[j] = 0.0f; }
    __syncthreads();
    const float z = g.zoneout, keep = 1.0f - g.zoneout;
    for (int step = 0; step < Tx; ++step) {
        const int t = dir ? Tx - 1 - step : step;
        matvec(g.whh[dir], g.xproj[dir] + ((long)b * g.Tx_max + t) * 4 * H, h, H, 4 * H, gates, scratch);
        for (int j = tid; j < H; j += blockDim.x) {
            const float gi = gates[j], gj = gates[H + j], gf = gates[2 * H + j], go = gates[3 * H + j];
            const float cn = sigmoid_acc(gf + 1.0f) * c[j] + sigmoid_acc(gi) * tanhf(gj);
            const float hn = sigmoid_acc(go) * tanhf(cn);
            g.memory[((long)b * g.Tx_max + t) * 2 * H + dir * H + j] = hn;   // the cell's output is the un-mixed new h
            c[j] = keep * cn + z * c[j];
            h[j] = keep * hn + z * h[j];
        }
        __syncthreads();
    }
}

struct DecArgs {
    const float *memory;     // (B, Tx_max, E2)
    const float *keys;       // (B, Tx_max, A)
    const int32_t *tx;       // (B)
    const uint64_t *seeds;   // (B)
    const float *gta;        // null or (B, gta_max, M)
    const int32_t *gta_steps;   // (B) when gta
    const float *prenet_w[WRNN_TACO_MAX_PRENET], *prenet_b[WRNN_TACO_MAX_PRENET];
    const float *lstm_w[MAX_DEC_LAYERS], *lstm_b[MAX_DEC_LAYERS];
    const float *query_w;    // (D, A)
    const float *loc_m;      // (taps, A): the location convolution folded into the location layer
    const float *att_bias;   // (A): attention_bias + the convolution's bias through the location layer
    const float *att_v;      // (A)
    const float *mu_w, *mu_b;   // (E2 + D, 1), (1)
    const float *proj_w, *proj_b;   // (D + E2, r M + r): the frame projection's columns, then the stop projection's
    float *decoder, *alignments, *stop;
    int32_t *max_attentions, *steps, *mel_frames;
    int32_t Tx_max, E2, A, M, r, D, L, n_prenet, prenet[WRNN_TACO_MAX_PRENET], taps, gta_max, max_iters, steps_max, dropout, Pmax, Kmax;
    float zoneout, clip_lo, clip_hi;
};
// The resumable variant's own arguments: the state between pushes, floats (B, st_stride): xin[M] h[L D] c[L D] ctx[E2] al[Tx_max]
// cum[Tx_max] mu, integers (B, ST_INTS); a launch runs n_steps more steps at most.
struct DecState {
    float *st_f;
    int32_t *st_i;
    int32_t st_stride, n_steps;
};
// LDS (floats): scratch[4 blockDim.x] xin[M] pa[Pmax] pb[Pmax] vec[Kmax] h[L D] c[L D] gates[4D] y[D] ctx[E2] q[A] al[Tx_max] cum[Tx_max]
//               sm[Tx_max] fw[Tx_max] proj[r M + r] mu1[1] red[16], then int: flags[4]
// RESUME: steps s0 .. s0 + n_steps - 1 of the same loop, s0 and everything a step hands to the next read from st_f / st_i and written back.
// The dropout counters and the output rows are keyed by the absolute step, so a partition into launches gives the bits of one launch.
template <bool RESUME>
__global__ void __launch_bounds__(LOOP_THREADS) taco_decoder_kernel(DecArgs g, DecState ds) {
    extern __shared__ __align__(16) float lds[];
    const int tid = threadIdx.x, NT = blockDim.x, b = blockIdx.x, wave = tid >> 6, lane = tid & 63, nw = NT >> 6;
    const int M = g.M, D = g.D, E2 = g.E2, A = g.A, r = g.r, L = g.L, RM = g.r * g.M;
    float *scratch = lds, *xin = scratch + 4 * NT, *pa = xin + M, *pb = pa + g.Pmax, *vec = pb + g.Pmax, *h = vec + g.Kmax, *c = h + L * D, *gates = c + L * D;
    float *y = gates + 4 * D, *ctx = y + D, *q = ctx + E2, *al = q + A, *cum = al + g.Tx_max, *sm = cum + g.Tx_max, *fw = sm + g.Tx_max;
    float *proj = fw + g.Tx_max, *mu1 = proj + RM + r, *red = mu1 + 1;
    int *flags = (int *)(red + 16);   // 0: max_attentions, 1: pos_rec, 2: stop, 3: argmax
    const int Tx = min(max(g.tx[b], 1), g.Tx_max);
    const float *memory = g.memory + (long)b * g.Tx_max * E2, *keys = g.keys + (long)b * g.Tx_max * A;
    const uint64_t seed = g.seeds[b];
    int steps = g.max_iters;
    if (g.gta) steps = g.gta_steps[b];
    steps = min(max(steps, 0), g.steps_max);
    const int all_steps = steps;
    int s0 = 0;
    float *sf = nullptr;
    int32_t *si = nullptr;
    if constexpr (RESUME) {
        sf = ds.st_f + (long)b * ds.st_stride;
        si = ds.st_i + (long)b * ST_INTS;
        s0 = min(max(si[ST_STEP], 0), all_steps);
        if (si[ST_FINISHED]) {   // the whole workgroup: nothing is new for this utterance
            if (tid == 0) { si[ST_PREV] = s0; si[ST_WAS] = 1; }
            return;
        }
        steps = min(all_steps, s0 + min(max(ds.n_steps, 0), all_steps));
    }
    for (int j = tid; j < M; j += NT) xin[j] = 0.0f;
    for (int j = tid; j < L * D; j += NT) { h[j] = 0.0f; c[j] = 0.0f; }
    for (int j = tid; j < E2; j += NT) ctx[j] = 0.0f;
    for (int j = tid; j < Tx; j += NT) { al[j] = j == 0 ? 1.0f : 0.0f; cum[j] = al[j]; }
    if (tid == 0) { flags[0] = 0; flags[1] = 0; flags[2] = 0; flags[3] = 0; }
    float mu = 0.5f;
    int first_stop = -1, s = 0;
    const float z = g.zoneout, keep = 1.0f - g.zoneout;
    const int left = (g.taps - 1) / 2;
    if constexpr (RESUME) {
        float *sh = sf + M, *sc = sh + L * D, *sctx = sc + L * D, *sal = sctx + E2, *scum = sal + g.Tx_max;
        if (s0 > 0) {
            for (int j = tid; j < M; j += NT) xin[j] = sf[j];
            for (int j = tid; j < L * D; j += NT) { h[j] = sh[j]; c[j] = sc[j]; }
            for (int j = tid; j < E2; j += NT) ctx[j] = sctx[j];
            for (int j = tid; j < Tx; j += NT) { al[j] = sal[j]; cum[j] = scum[j]; }
            mu = scum[g.Tx_max];
            first_stop = si[ST_FIRST_STOP];
            s = s0;
        }
        if (tid == 0) {
            if (s0 > 0) { flags[0] = si[ST_MAX_ATT]; flags[1] = si[ST_POS_REC]; }
            si[ST_PREV] = s0;
            si[ST_WAS] = 0;
        }
    }
    __syncthreads();
    for (; s < steps; ++s) {
        // ---- prenet: dense -> relu -> dropout(0.5), always on
        const float *pin = xin;
        float *pout = pa;
        int Kin = M;
        for (int l = 0; l < g.n_prenet; ++l) {
            const int P = g.prenet[l];
            matvec(g.prenet_w[l], g.prenet_b[l], pin, Kin, P, pout, scratch);
            for (int j = tid; j < P; j += NT) {
                float v = fmaxf(pout[j], 0.0f);
                if (g.dropout) v = wrnn_uniform(seed, (uint64_t)s * g.n_prenet + l, 0u, (uint32_t)j) >= 0.5f ? 2.0f * v : 0.0f;
                pout[j] = v;
            }
            __syncthreads();
            pin = pout;
            pout = pout == pa ? pb : pa;
            Kin = P;
        }
        // ---- the zoneout LSTMs: layer 0 reads [prenet; context; h0], layer l [output of l - 1; h_l]
        for (int l = 0; l < L; ++l) {
            int K;
            if (l == 0) {
                for (int j = tid; j < Kin; j += NT) vec[j] = pin[j];
                for (int j = tid; j < E2; j += NT) vec[Kin + j] = ctx[j];
                K = Kin + E2;
            } else {
                for (int j = tid; j < D; j += NT) vec[j] = y[j];
                K = D;
            }
            for (int j = tid; j < D; j += NT) vec[K + j] = h[l * D + j];
            __syncthreads();
            matvec(g.lstm_w[l], g.lstm_b[l], vec, K + D, 4 * D, gates, scratch);
            for (int j = tid; j < D; j += NT) {
                const float gi = gates[j], gj = gates[D + j], gf = gates[2 * D + j], go = gates[3 * D + j];
                const float cp = c[l * D + j];
                const float cn = sigmoid_acc(gf + 1.0f) * cp + sigmoid_acc(gi) * tanhf(gj);
                const float hn = sigmoid_acc(go) * tanhf(cn);
                y[j] = hn;
                c[l * D + j] = keep * cn + z * cp;
                h[l * D + j] = keep * hn + z * h[l * D + j];
            }
            __syncthreads();
        }
        // ---- attention: energies, one wave per memory row
        matvec(g.query_w, nullptr, y, D, A, q, scratch);
        for (int t = wave; t < Tx; t += nw) {
            float e = 0.0f;
            for (int a = lane; a < A; a += 64) {
                float loc = 0.0f;
                for (int k = 0; k < g.taps; ++k) {
                    const int u = t + k - left;
                    if (u >= 0 && u < Tx) loc += cum[u] * g.loc_m[k * A + a];
                }
                e += g.att_v[a] * tanhf(keys[(long)t * A + a] + q[a] + loc + g.att_bias[a]);
            }
#pragma unroll
            for (int off = 32; off >= 1; off >>= 1) e += __shfl_xor(e, off, 64);
            if (lane == 0) sm[t] = e;
        }
        __syncthreads();
        float mx = -INFINITY;
        for (int t = tid; t < Tx; t += NT) mx = fmaxf(mx, sm[t]);
        mx = block_max(mx, red);
        float part = 0.0f;
        for (int t = tid; t < Tx; t += NT) { const float e = expf(sm[t] - mx); fw[t] = e; part += e; }
        const float den = block_sum(part, red);
        // softmax, the cumulated alignments, the forward recursion, its argmax (the lowest index on a tie)
        float bv = -INFINITY;
        int bi = 0x7fffffff;
        for (int t = tid; t < Tx; t += NT) {
            const float p = fw[t] / den;
            sm[t] = p;
            cum[t] += p;
        }
        __syncthreads();
        for (int t = tid; t < Tx; t += NT) {
            const float f = ((1.0f - mu) * al[t] + mu * (t > 0 ? al[t - 1] : 0.0f) + 1e-10f) * sm[t];
            fw[t] = f;
            if (f > bv) { bv = f; bi = t; }
        }
        wave_argmax(bv, bi);
        __syncthreads();
        if (lane == 0) { red[wave] = bv; ((int *)scratch)[wave] = bi; }
        __syncthreads();
        if (tid == 0) {
            float v = red[0];
            int am = ((int *)scratch)[0];
            for (int w = 1; w < nw; ++w) {
                const float ov = red[w];
                const int oi = ((int *)scratch)[w];
                if (ov > v || (ov == v && oi < am)) { v = ov; am = oi; }
            }
            // the inference-only block: no step back, at least 5 steps on a position beyond 2, at most 9
            const int mp = flags[0], pp = flags[1];
            int m = am <= mp ? mp : mp + 1;
            if (pp < 5 && 2 < m) m = mp;
            int pos = m == mp ? pp + 1 : 1;
            if (!(pos < 10)) { m = m + 1; pos = 1; }
            flags[0] = m; flags[1] = pos; flags[3] = am;
            g.max_attentions[(long)b * g.steps_max + s] = m;
        }
        __syncthreads();
        const int m = flags[0];
        const int mi = min(m, Tx - 1);
        part = 0.0f;
        for (int t = tid; t < Tx; t += NT) {
            const float f = (t >= m - 2 && t < m + 3) ? fw[t] : 0.0f;
            fw[t] = f;
            part += f;
        }
        float wsum = block_sum(part, red);
        if (wsum < 1e-10f) wsum = 1.0f;
        if (tid == 0) fw[mi] = wsum * 2.0f;
        __syncthreads();
        part = 0.0f;
        for (int t = tid; t < Tx; t += NT) part += fw[t];
        const float total = block_sum(part, red);
        float *al_out = g.alignments + ((long)b * g.steps_max + s) * g.Tx_max;
        for (int t = tid; t < Tx; t += NT) {
            const float a = fw[t] / total;
            al[t] = a;
            al_out[t] = a;
        }
        __syncthreads();
        // the context: only the window and index mi hold anything but 0
        const int lo = max(0, min(m - 2, mi)), hi = min(Tx, max(m + 3, mi + 1));
        for (int d = tid; d < E2; d += NT) {
            float acc = 0.0f;
            for (int t = lo; t < hi; ++t) acc += al[t] * memory[(long)t * E2 + d];
            ctx[d] = acc;
        }
        __syncthreads();
        for (int j = tid; j < E2; j += NT) vec[j] = ctx[j];
        for (int j = tid; j < D; j += NT) vec[E2 + j] = y[j];
        __syncthreads();
        matvec(g.mu_w, g.mu_b, vec, E2 + D, 1, mu1, scratch);
        mu = sigmoid_acc(mu1[0]);
        // ---- the projections of [output; context]
        for (int j = tid; j < D; j += NT) vec[j] = y[j];
        for (int j = tid; j < E2; j += NT) vec[D + j] = ctx[j];
        __syncthreads();
        matvec(g.proj_w, g.proj_b, vec, D + E2, RM + r, proj, scratch);
        for (int j = tid; j < RM; j += NT)
            g.decoder[((long)b * g.steps_max + s) * RM + j] = fminf(fmaxf(proj[j], g.clip_lo), g.clip_hi);
        if (tid < r) {
            const float p = sigmoid_acc(proj[RM + tid]);
            proj[RM + tid] = p;
            g.stop[((long)b * g.steps_max + s) * r + tid] = p;
        }
        __syncthreads();
        if (tid == 0) {
            int stop = 0;
            for (int k = 0; k < r; ++k)
                if (proj[RM + k] > 0.5f) {
                    if (first_stop < 0) first_stop = s * r + k;
                    stop = 1;
                }
            flags[2] = stop;
        }
        for (int j = tid; j < M; j += NT)
            xin[j] = g.gta ? (((s + 1) * r - 1) < g.gta_max ? g.gta[((long)b * g.gta_max + (s + 1) * r - 1) * M + j] : 0.0f) : proj[RM - M + j];
        __syncthreads();
        if (!g.gta && flags[2]) { ++s; break; }
    }
    if constexpr (RESUME) {   // every thread is past the last barrier of the last step
        float *sh = sf + M, *sc = sh + L * D, *sctx = sc + L * D, *sal = sctx + E2, *scum = sal + g.Tx_max;
        for (int j = tid; j < M; j += NT) sf[j] = xin[j];
        for (int j = tid; j < L * D; j += NT) { sh[j] = h[j]; sc[j] = c[j]; }
        for (int j = tid; j < E2; j += NT) sctx[j] = ctx[j];
        for (int j = tid; j < Tx; j += NT) { sal[j] = al[j]; scum[j] = cum[j]; }
        if (tid == 0) {
            scum[g.Tx_max] = mu;
            si[ST_MAX_ATT] = flags[0];
            si[ST_POS_REC] = flags[1];
            si[ST_FIRST_STOP] = first_stop;
            si[ST_STEP] = s;
            si[ST_FINISHED] = (flags[2] || s >= all_steps) ? 1 : 0;
        }
    }
    if (tid == 0) {
        g.steps[b] = s;
        g.mel_frames[b] = (!g.gta && first_stop >= 0) ? first_stop : s * r;
    }
}

struct FinishArgs {
    const float *decoder, *residual;   // (B, T_max, M) each
    const int32_t *steps;              // (B)
    float *mel_raw, *mel;
    int32_t T_max, M, r;
    float clip_lo, clip_hi;
};
__device__ inline void finish_element(const FinishArgs &g, long at) {
    const float raw = fminf(fmaxf(g.decoder[at] + g.residual[at], g.clip_lo), g.clip_hi);
    g.mel_raw[at] = raw;
    const float v = fminf(fmaxf(raw, -g.clip_hi), g.clip_hi);
    g.mel[at] = fminf(fmaxf((v + g.clip_hi) / (2.0f * g.clip_hi), 0.0f), 1.0f);
}
__global__ void __launch_bounds__(CONV_THREADS) taco_finish_kernel(FinishArgs g) {
    const int b = blockIdx.y;
    const long x = (long)blockIdx.x * CONV_THREADS + threadIdx.x, n = (long)g.T_max * g.M;
    if (x >= n) return;
    const long rows = (long)min(max(g.steps[b], 0), g.T_max / g.r) * g.r;
    const long at = (long)b * n + x;
    if (x / g.M >= rows) { g.mel_raw[at] = 0.0f; g.mel[at] = 0.0f; return; }
    finish_element(g, at);
}
// The rows a stream's last push released: [prev r - halo, steps r - halo), up to the true end once the utterance has finished.  The rows
// beyond stay the zeros the stream's buffers were opened with.
__global__ void __launch_bounds__(CONV_THREADS) taco_finish_window_kernel(FinishArgs g, const int32_t *win, int halo) {
    const int b = blockIdx.y;
    const int32_t *si = win + (long)b * ST_INTS;
    if (si[ST_WAS]) return;
    const long L = (long)min(max(si[ST_STEP], 0), g.T_max / g.r) * g.r;
    const long lo = min(max((long)si[ST_PREV] * g.r - halo, 0L), L), hi = si[ST_FINISHED] ? L : max(L - halo, 0L);
    const long x = lo * g.M + (long)blockIdx.x * CONV_THREADS + threadIdx.x;
    if (x >= hi * g.M) return;
    finish_element(g, (long)b * g.T_max * g.M + x);
}

using Tensor = TacoTensor;   // taco_internal.h

}  // namespace

struct wrnn_taco_stream {
    wrnn_taco_handle *h = nullptr;
    int B = 0, Tx_max = 0, S = 0, dropout = 0;
    char *ws = nullptr;           // everything the stream owns on the device, one allocation
    size_t ws_bytes = 0;
    int32_t *host_i = nullptr;    // pinned, (B, ST_INTS): the state's integers after a push
    int32_t *ids = nullptr, *tx = nullptr, *st_i = nullptr, *max_attentions = nullptr, *steps = nullptr, *mel_frames = nullptr;
    uint64_t *seeds = nullptr;
    float *mem = nullptr, *keys = nullptr, *st_f = nullptr, *decoder = nullptr, *residual = nullptr, *mel_raw = nullptr, *mel = nullptr;
    float *alignments = nullptr, *stop = nullptr;
    std::vector<float *> post;    // the postnet layers' activations, (B, S r, postnet_channels) each
    int st_stride = 0, Pmax = 0, Kmax = 0;
    size_t dec_lds = 0;
    bool done = false;            // every utterance has finished
    std::string err;
};

namespace {
size_t up64(size_t floats) { return (floats + 63) & ~(size_t)63; }

void add(wrnn_taco_handle *h, const std::string &name, std::vector<int64_t> shape) {
    Tensor t;
    t.name = name;
    t.shape = std::move(shape);
    h->tensors.push_back(std::move(t));
}
void add_conv_block(wrnn_taco_handle *h, const std::string &p, int taps, int cin, int cout) {
    add(h, p + "conv1d/kernel", {taps, cin, cout});
    add(h, p + "conv1d/bias", {cout});
    for (const char *n : {"gamma", "beta", "moving_mean", "moving_variance"}) add(h, p + "batch_normalization/" + n, {cout});
}
const Tensor *find(const wrnn_taco_handle *h, const std::string &name) {
    for (const Tensor &t : h->tensors)
        if (t.name == name) return &t;
    return nullptr;
}
std::string enc_conv(int i) { return "encoder_convolutions/conv_layer_" + std::to_string(i) + "_encoder_convolutions/"; }
std::string post_conv(int i) { return "postnet_convolutions/conv_layer_" + std::to_string(i) + "_postnet_convolutions/"; }
std::string dec_lstm(int l) { return "decoder/decoder_LSTM/multi_rnn_cell/cell_" + std::to_string(l) + "/decoder_LSTM_" + std::to_string(l + 1) + "/"; }
std::string enc_lstm(const char *d) { return std::string("encoder_LSTM/bidirectional_rnn/") + d + "/encoder_" + d + "_LSTM/"; }
const char *LSA = "decoder/Location_Sensitive_Attention/";
const char *FRAME = "decoder/linear_transform_projection/projection_linear_transform_projection/";
const char *STOP = "decoder/stop_token_projection/projection_stop_token_projection/";
const char *POSTP = "postnet_projection/projection_postnet_projection/";

void build_table(wrnn_taco_handle *h) {
    const wrnn_taco_dims &d = h->d;
    const int E2 = 2 * d.encoder_lstm_units, D = d.decoder_lstm_units, M = d.num_mels, r = d.outputs_per_step;
    add(h, "inputs_embedding", {d.n_symbols, d.embedding_dim});
    for (int i = 0; i < d.enc_conv_layers; ++i) add_conv_block(h, enc_conv(i + 1), d.enc_conv_kernel, i ? d.enc_conv_channels : d.embedding_dim, d.enc_conv_channels);
    for (const char *dir : {"fw", "bw"}) {
        add(h, enc_lstm(dir) + "kernel", {d.enc_conv_channels + d.encoder_lstm_units, 4 * d.encoder_lstm_units});
        add(h, enc_lstm(dir) + "bias", {4 * d.encoder_lstm_units});
    }
    add(h, "memory_layer/kernel", {E2, d.attention_dim});
    int in = M;
    for (int l = 0; l < d.prenet_layers; ++l) {
        add(h, "decoder/decoder_prenet/dense_" + std::to_string(l + 1) + "/kernel", {in, d.prenet_sizes[l]});
        add(h, "decoder/decoder_prenet/dense_" + std::to_string(l + 1) + "/bias", {d.prenet_sizes[l]});
        in = d.prenet_sizes[l];
    }
    for (int l = 0; l < d.decoder_layers; ++l) {
        add(h, dec_lstm(l) + "kernel", {(l ? D : in + E2) + D, 4 * D});
        add(h, dec_lstm(l) + "bias", {4 * D});
    }
    add(h, std::string(LSA) + "query_layer/kernel", {D, d.attention_dim});
    add(h, std::string(LSA) + "location_features_convolution/kernel", {d.attention_kernel, 1, d.attention_filters});
    add(h, std::string(LSA) + "location_features_convolution/bias", {d.attention_filters});
    add(h, std::string(LSA) + "location_features_layer/kernel", {d.attention_filters, d.attention_dim});
    add(h, std::string(LSA) + "attention_variable_projection", {d.attention_dim});
    add(h, std::string(LSA) + "attention_bias", {d.attention_dim});
    add(h, "decoder/dense/kernel", {E2 + D, 1});
    add(h, "decoder/dense/bias", {1});
    add(h, std::string(FRAME) + "kernel", {D + E2, r * M});
    add(h, std::string(FRAME) + "bias", {r * M});
    add(h, std::string(STOP) + "kernel", {D + E2, r});
    add(h, std::string(STOP) + "bias", {r});
    for (int i = 0; i < d.postnet_layers; ++i) add_conv_block(h, post_conv(i + 1), d.postnet_kernel, i ? d.postnet_channels : M, d.postnet_channels);
    add(h, std::string(POSTP) + "kernel", {d.postnet_channels, M});
    add(h, std::string(POSTP) + "bias", {M});
}

// LDS floats of the decoder kernel for a call whose longest utterance has Tx_max symbols
size_t decoder_lds_floats(const wrnn_taco_dims &d, int Tx_max, int *Pmax_out, int *Kmax_out) {
    const int E2 = 2 * d.encoder_lstm_units, D = d.decoder_lstm_units, M = d.num_mels, r = d.outputs_per_step;
    int Pmax = 1;
    for (int l = 0; l < d.prenet_layers; ++l) Pmax = std::max(Pmax, (int)d.prenet_sizes[l]);
    const int Plast = d.prenet_sizes[d.prenet_layers - 1];
    const int Kmax = std::max(Plast + E2 + D, std::max(2 * D, D + E2));
    if (Pmax_out) *Pmax_out = Pmax;
    if (Kmax_out) *Kmax_out = Kmax;
    return (size_t)M + 2 * (size_t)Pmax + Kmax + 2 * (size_t)d.decoder_layers * D + 4 * (size_t)D + D + E2 + d.attention_dim + 4 * (size_t)Tx_max +
           (size_t)r * M + r + 1 + 4 * LOOP_THREADS + 16 + 4;
}

// The derived tensors: BatchNorm folded to scale and shift, the location convolution folded into the location layer, the frame and stop
// projections side by side.  Sums in float64, one rounding to float32.
int upload(wrnn_taco_handle *h) {
    const wrnn_taco_dims &d = h->d;
    for (const Tensor &t : h->tensors)
        if (t.data.empty()) return wrnn_failf(h, WRNN_ERR_STATE, "tensor %s has not been loaded", t.name.c_str());
    std::vector<float> img;
    for (Tensor &t : h->tensors) {
        t.off = img.size();
        img.insert(img.end(), t.data.begin(), t.data.end());
        img.resize(up64(img.size()), 0.0f);
    }
    auto fold_bn = [&](const std::string &p, int C) {
        const Tensor *ga = find(h, p + "batch_normalization/gamma"), *be = find(h, p + "batch_normalization/beta");
        const Tensor *mm = find(h, p + "batch_normalization/moving_mean"), *mv = find(h, p + "batch_normalization/moving_variance");
        const size_t at = img.size();
        img.resize(at + 2 * up64(C), 0.0f);
        for (int c = 0; c < C; ++c) {
            const double s = (double)ga->data[c] / std::sqrt((double)mv->data[c] + (double)d.bn_epsilon);
            img[at + c] = (float)s;
            img[at + up64(C) + c] = (float)((double)be->data[c] - (double)mm->data[c] * s);
        }
        return at;
    };
    h->off_bn_enc = img.size();
    for (int i = 0; i < d.enc_conv_layers; ++i) fold_bn(enc_conv(i + 1), d.enc_conv_channels);
    h->off_bn_post = img.size();
    for (int i = 0; i < d.postnet_layers; ++i) fold_bn(post_conv(i + 1), d.postnet_channels);
    const int A = d.attention_dim, F = d.attention_filters, taps = d.attention_kernel;
    const Tensor *ck = find(h, std::string(LSA) + "location_features_convolution/kernel"), *cb = find(h, std::string(LSA) + "location_features_convolution/bias");
    const Tensor *ll = find(h, std::string(LSA) + "location_features_layer/kernel"), *ab = find(h, std::string(LSA) + "attention_bias");
    h->off_loc_m = img.size();
    img.resize(img.size() + up64((size_t)taps * A), 0.0f);
    for (int k = 0; k < taps; ++k)
        for (int a = 0; a < A; ++a) {
            double s = 0.0;
            for (int f = 0; f < F; ++f) s += (double)ck->data[(size_t)k * F + f] * (double)ll->data[(size_t)f * A + a];
            img[h->off_loc_m + (size_t)k * A + a] = (float)s;
        }
    h->off_att_bias = img.size();
    img.resize(img.size() + up64(A), 0.0f);
    for (int a = 0; a < A; ++a) {
        double s = ab->data[a];
        for (int f = 0; f < F; ++f) s += (double)cb->data[f] * (double)ll->data[(size_t)f * A + a];
        img[h->off_att_bias + a] = (float)s;
    }
    const int E2 = 2 * d.encoder_lstm_units, D = d.decoder_lstm_units, RM = d.outputs_per_step * d.num_mels, r = d.outputs_per_step, N = RM + r;
    const Tensor *fk = find(h, std::string(FRAME) + "kernel"), *fb = find(h, std::string(FRAME) + "bias");
    const Tensor *sk = find(h, std::string(STOP) + "kernel"), *sb = find(h, std::string(STOP) + "bias");
    h->off_proj_w = img.size();
    img.resize(img.size() + up64((size_t)(D + E2) * N), 0.0f);
    for (int i = 0; i < D + E2; ++i) {
        for (int j = 0; j < RM; ++j) img[h->off_proj_w + (size_t)i * N + j] = fk->data[(size_t)i * RM + j];
        for (int j = 0; j < r; ++j) img[h->off_proj_w + (size_t)i * N + RM + j] = sk->data[(size_t)i * r + j];
    }
    h->off_proj_b = img.size();
    img.resize(img.size() + up64(N), 0.0f);
    for (int j = 0; j < RM; ++j) img[h->off_proj_b + j] = fb->data[j];
    for (int j = 0; j < r; ++j) img[h->off_proj_b + RM + j] = sb->data[j];
    if (img.size() > h->img_cap) {
        if (h->img) WRNN_TRY(h, hipFree(h->img));
        h->img = nullptr;
        h->img_cap = 0;
        WRNN_TRY(h, hipMalloc((void **)&h->img, img.size() * sizeof(float)));
        h->img_cap = img.size();
    }
    WRNN_TRY(h, hipMemcpy(h->img, img.data(), img.size() * sizeof(float), hipMemcpyHostToDevice));
    h->dirty = false;
    return WRNN_OK;
}

int launch_conv(wrnn_taco_handle *h, hipStream_t s, const float *in, const float *w, const float *bias, const float *bn, int C_bn_stride, float *out,
                const int32_t *len, int len_mul, int B, int T_max, int Cin, int Cout, int taps, int act) {
    ConvArgs a{};
    a.in = in; a.w = w; a.bias = bias; a.bn_s = bn; a.bn_b = bn ? bn + C_bn_stride : nullptr; a.out = out; a.len = len; a.len_mul = len_mul;
    a.T_max = T_max; a.Cin = Cin; a.Cout = Cout; a.taps = taps; a.act = act;
    const size_t lds = (size_t)(CONV_TT + taps - 1) * Cin * sizeof(float);
    hipLaunchKernelGGL(taco_conv_kernel<false>, dim3((unsigned)((T_max + CONV_TT - 1) / CONV_TT), (unsigned)B, (unsigned)((Cout + 63) / 64)),
                       dim3(CONV_THREADS), lds, s, a, ConvWindow{});
    WRNN_TRY(h, hipGetLastError());
    return WRNN_OK;
}

// The host-side checks of a call's text, shared by the offline call and a stream's open (the offline call checks its output pointers
// and max_iters between the two).
int check_text(wrnn_taco_handle *h, int B, int Tx_max, const int32_t *ids_host, const int32_t *tx_host, const uint64_t *seeds_host) {
    if (B < 1 || B > WRNN_MAX_GRID_Y) return wrnn_failf(h, WRNN_ERR_INVALID, "B %d outside 1 .. 65535", B);
    if (Tx_max < 1 || Tx_max > WRNN_TACO_MAX_TX) return wrnn_failf(h, WRNN_ERR_INVALID, "Tx_max %d outside 1 .. %d symbols", Tx_max, WRNN_TACO_MAX_TX);
    if (!ids_host || !tx_host || !seeds_host) return wrnn_failf(h, WRNN_ERR_INVALID, "ids_host, tx_host or seeds_host is NULL");
    return WRNN_OK;
}
}  // namespace
int taco_refuse_length(wrnn_taco_handle *h, int b, int tx, int Tx_max) {
    return wrnn_failf(h, WRNN_ERR_INVALID, "utterance %d: %d symbols outside 1 .. Tx_max = %d (the limit is %d)", b, tx, Tx_max, WRNN_TACO_MAX_TX);
}
namespace {
int check_symbols(wrnn_taco_handle *h, int B, int Tx_max, const int32_t *ids_host, const int32_t *tx_host) {
    for (int b = 0; b < B; ++b) {
        const int tx = tx_host[b];
        if (tx < 1 || tx > Tx_max) return taco_refuse_length(h, b, tx, Tx_max);
        for (int t = 0; t < tx; ++t) {
            const int id = ids_host[(size_t)b * Tx_max + t];
            if (id < 0 || id >= h->d.n_symbols) return wrnn_failf(h, WRNN_ERR_INVALID, "utterance %d: symbol id %d at %d is outside the table of %d", b, id, t, h->d.n_symbols);
        }
    }
    return WRNN_OK;
}

const float *tensor_at(const wrnn_taco_handle *h, const std::string &n) { return h->img + find(h, n)->off; }

// ids, tx -> memory and keys.  a0, a1: B Tx_max max(enc_conv_channels, embedding_dim) floats each; xp: B Tx_max 4 H floats each;
// mem has been zeroed.
struct EncBufs {
    const int32_t *ids, *tx;
    float *a0, *a1, *xp[2], *mem, *keys;
};
int run_encoder(wrnn_taco_handle *h, hipStream_t s, const EncBufs &e, int B, int Tx_max) {
    const wrnn_taco_dims &d = h->d;
    const int C = d.enc_conv_channels, H = d.encoder_lstm_units, E2 = 2 * H, A = d.attention_dim;
    const float *img = h->img;
    EmbedArgs em{e.ids, e.tx, tensor_at(h, "inputs_embedding"), e.a0, Tx_max, d.embedding_dim, d.n_symbols};
    hipLaunchKernelGGL(taco_embed_kernel, dim3((unsigned)Tx_max, (unsigned)B), dim3(CONV_THREADS), 0, s, em);
    WRNN_TRY(h, hipGetLastError());
    float *cur = e.a0, *nxt = e.a1;
    int rc;
    for (int i = 0; i < d.enc_conv_layers; ++i) {
        const std::string p = enc_conv(i + 1);
        rc = launch_conv(h, s, cur, tensor_at(h, p + "conv1d/kernel"), tensor_at(h, p + "conv1d/bias"), img + h->off_bn_enc + (size_t)i * 2 * up64(C), (int)up64(C), nxt,
                         e.tx, 1, B, Tx_max, i ? C : d.embedding_dim, C, d.enc_conv_kernel, 1);
        if (rc != WRNN_OK) return rc;
        std::swap(cur, nxt);
    }
    EncLstmArgs el{};
    int di = 0;
    for (const char *dir : {"fw", "bw"}) {
        rc = launch_conv(h, s, cur, tensor_at(h, enc_lstm(dir) + "kernel"), tensor_at(h, enc_lstm(dir) + "bias"), nullptr, 0, e.xp[di], e.tx, 1, B, Tx_max, C, 4 * H, 1, 0);
        if (rc != WRNN_OK) return rc;
        el.xproj[di] = e.xp[di];
        el.whh[di] = tensor_at(h, enc_lstm(dir) + "kernel") + (size_t)C * 4 * H;
        ++di;
    }
    el.tx = e.tx; el.memory = e.mem; el.Tx_max = Tx_max; el.H = H; el.zoneout = d.zoneout;
    hipLaunchKernelGGL(taco_enc_lstm_kernel, dim3(2u, (unsigned)B), dim3(LOOP_THREADS), (size_t)(6 * H + 4 * LOOP_THREADS) * sizeof(float), s, el);
    WRNN_TRY(h, hipGetLastError());
    return launch_conv(h, s, e.mem, tensor_at(h, "memory_layer/kernel"), nullptr, nullptr, 0, e.keys, e.tx, 1, B, Tx_max, E2, A, 1, 0);
}

// The decoder's weights and the model's sizes; the caller adds the call's own pointers and counts.
void decoder_model_args(const wrnn_taco_handle *h, DecArgs &g) {
    const wrnn_taco_dims &d = h->d;
    const float *img = h->img;
    for (int l = 0; l < d.prenet_layers; ++l) {
        g.prenet_w[l] = tensor_at(h, "decoder/decoder_prenet/dense_" + std::to_string(l + 1) + "/kernel");
        g.prenet_b[l] = tensor_at(h, "decoder/decoder_prenet/dense_" + std::to_string(l + 1) + "/bias");
        g.prenet[l] = d.prenet_sizes[l];
    }
    for (int l = 0; l < d.decoder_layers; ++l) { g.lstm_w[l] = tensor_at(h, dec_lstm(l) + "kernel"); g.lstm_b[l] = tensor_at(h, dec_lstm(l) + "bias"); }
    g.query_w = tensor_at(h, std::string(LSA) + "query_layer/kernel");
    g.loc_m = img + h->off_loc_m; g.att_bias = img + h->off_att_bias; g.att_v = tensor_at(h, std::string(LSA) + "attention_variable_projection");
    g.mu_w = tensor_at(h, "decoder/dense/kernel"); g.mu_b = tensor_at(h, "decoder/dense/bias");
    g.proj_w = img + h->off_proj_w; g.proj_b = img + h->off_proj_b;
    g.E2 = 2 * d.encoder_lstm_units; g.A = d.attention_dim; g.M = d.num_mels; g.r = d.outputs_per_step; g.D = d.decoder_lstm_units; g.L = d.decoder_layers;
    g.n_prenet = d.prenet_layers; g.taps = d.attention_kernel;
    g.zoneout = d.zoneout; g.clip_lo = -d.max_abs_value - d.lower_bound_decay; g.clip_hi = d.max_abs_value;
}

// Rows a mel frame waits for: what the postnet's convolutions reach to the right ('same' padding puts (k - 1) / 2 taps on the left).
int postnet_reach(const wrnn_taco_dims &d) { return (d.postnet_kernel - 1) - (d.postnet_kernel - 1) / 2; }

void free_stream(wrnn_taco_stream *st) {
    if (st->ws) (void)hipFree(st->ws);
    if (st->host_i) (void)hipHostFree(st->host_i);
    delete st;
}
}  // namespace

// ---- taco_internal.h: what wrnn_taco_gta_corpus (taco_gta.hip) shares with wrnn_taco_synthesize
int taco_check_text(wrnn_taco_handle *h, int B, int Tx_max, const int32_t *ids_host, const int32_t *tx_host, const uint64_t *seeds_host) {
    return check_text(h, B, Tx_max, ids_host, tx_host, seeds_host);
}
int taco_check_symbols(wrnn_taco_handle *h, int B, int Tx_max, const int32_t *ids_host, const int32_t *tx_host) {
    return check_symbols(h, B, Tx_max, ids_host, tx_host);
}
int taco_check_decoder_lds(wrnn_taco_handle *h, int Tx_max) {
    if (decoder_lds_floats(h->d, Tx_max, nullptr, nullptr) * sizeof(float) > LDS_LIMIT)
        return wrnn_failf(h, WRNN_ERR_INVALID, "the decoder's state for Tx_max %d exceeds 64 KiB of LDS", Tx_max);
    return WRNN_OK;
}
int taco_upload_if_dirty(wrnn_taco_handle *h) { return h->dirty ? upload(h) : WRNN_OK; }

TacoBufs taco_layout(const wrnn_taco_dims &d, int B, int Tx_max, int S) {
    const int C = d.enc_conv_channels, H = d.encoder_lstm_units, E2 = 2 * H, A = d.attention_dim, PC = d.postnet_channels, M = d.num_mels;
    const size_t T_out = (size_t)S * d.outputs_per_step;
    const size_t act_floats = std::max((size_t)B * Tx_max * std::max(C, d.embedding_dim), (size_t)B * T_out * std::max(PC, M));
    size_t at = 0;
    auto take = [&at](size_t bytes) { const size_t o = at; at += wrnn_up256(bytes); return o; };
    TacoBufs o{};
    o.ids = take((size_t)B * Tx_max * 4); o.tx = take((size_t)B * 4); o.gs = take((size_t)B * 4); o.seeds = take((size_t)B * 8);
    o.a0 = take(act_floats * 4); o.a1 = take(act_floats * 4);
    o.xp0 = take((size_t)B * Tx_max * 4 * H * 4); o.xp1 = take((size_t)B * Tx_max * 4 * H * 4);
    o.mem = take((size_t)B * Tx_max * E2 * 4); o.keys = take((size_t)B * Tx_max * A * 4);
    o.end = at;
    return o;
}

int taco_run(wrnn_taco_handle *h, hipStream_t s, const TacoRun &c) {
    const wrnn_taco_dims &d = h->d;
    const int B = c.B, Tx_max = c.Tx_max, S = c.S, r = d.outputs_per_step, M = d.num_mels;
    const int E2 = 2 * d.encoder_lstm_units, PC = d.postnet_channels, T_out = S * r;
    int Pmax = 0, Kmax = 0, rc;
    const size_t dec_lds = decoder_lds_floats(d, Tx_max, &Pmax, &Kmax) * sizeof(float);
    char *ws = c.ws;
    const int32_t *ids = (const int32_t *)(ws + c.o.ids), *tx = (const int32_t *)(ws + c.o.tx), *gs = (const int32_t *)(ws + c.o.gs);
    const uint64_t *seeds = (const uint64_t *)(ws + c.o.seeds);
    float *a0 = (float *)(ws + c.o.a0), *a1 = (float *)(ws + c.o.a1), *xp[2] = {(float *)(ws + c.o.xp0), (float *)(ws + c.o.xp1)};
    float *mem = (float *)(ws + c.o.mem), *keys = (float *)(ws + c.o.keys);
    WRNN_TRY(h, hipMemsetAsync(mem, 0, (size_t)B * Tx_max * E2 * 4, s));
    WRNN_TRY(h, hipMemsetAsync(c.decoder, 0, (size_t)B * T_out * M * 4, s));
    WRNN_TRY(h, hipMemsetAsync(c.alignments, 0, (size_t)B * S * Tx_max * 4, s));
    WRNN_TRY(h, hipMemsetAsync(c.stop, 0, (size_t)B * T_out * 4, s));
    WRNN_TRY(h, hipMemsetAsync(c.max_attentions, 0, (size_t)B * S * 4, s));
    const float *img = h->img;
    auto T = [&](const std::string &n) { return img + find(h, n)->off; };
    // ---- encoder
    const EncBufs eb{ids, tx, a0, a1, {xp[0], xp[1]}, mem, keys};
    if ((rc = run_encoder(h, s, eb, B, Tx_max)) != WRNN_OK) return rc;
    if (c.encoder) WRNN_TRY(h, hipMemcpyAsync(c.encoder, mem, (size_t)B * Tx_max * E2 * 4, hipMemcpyDeviceToDevice, s));
    // ---- decoder
    DecArgs g{};
    g.memory = mem; g.keys = keys; g.tx = tx; g.seeds = seeds; g.gta = c.gta; g.gta_steps = gs;
    decoder_model_args(h, g);
    g.decoder = c.decoder; g.alignments = c.alignments; g.stop = c.stop;
    g.max_attentions = c.max_attentions; g.steps = c.steps; g.mel_frames = c.mel_frames;
    g.Tx_max = Tx_max; g.gta_max = c.gta ? c.gta_max : 0; g.max_iters = c.max_iters; g.steps_max = S; g.dropout = c.dropout;
    g.Pmax = Pmax; g.Kmax = Kmax;
    hipLaunchKernelGGL(taco_decoder_kernel<false>, dim3((unsigned)B), dim3(LOOP_THREADS), dec_lds, s, g, DecState{});
    WRNN_TRY(h, hipGetLastError());
    // ---- postnet over steps r rows per utterance, the count read from the device
    const float *pin = c.decoder;
    float *cur = a0, *nxt = a1;
    for (int i = 0; i < d.postnet_layers; ++i) {
        const std::string p = post_conv(i + 1);
        rc = launch_conv(h, s, pin, T(p + "conv1d/kernel"), T(p + "conv1d/bias"), img + h->off_bn_post + (size_t)i * 2 * up64(PC), (int)up64(PC), cur, c.steps, r, B,
                         T_out, i ? PC : M, PC, d.postnet_kernel, i + 1 < d.postnet_layers ? 2 : 0);
        if (rc != WRNN_OK) return rc;
        pin = cur;
        std::swap(cur, nxt);
    }
    rc = launch_conv(h, s, pin, T(std::string(POSTP) + "kernel"), T(std::string(POSTP) + "bias"), nullptr, 0, cur, c.steps, r, B, T_out, PC, M, 1, 0);
    if (rc != WRNN_OK) return rc;
    FinishArgs f{c.decoder, cur, c.steps, c.mel_raw, c.mel, T_out, M, r, g.clip_lo, g.clip_hi};
    hipLaunchKernelGGL(taco_finish_kernel, dim3((unsigned)(((size_t)T_out * M + CONV_THREADS - 1) / CONV_THREADS), (unsigned)B), dim3(CONV_THREADS), 0, s, f);
    WRNN_TRY(h, hipGetLastError());
    return WRNN_OK;
}

extern "C" {

int wrnn_taco_create(const wrnn_taco_dims *dims, wrnn_taco_handle **out) {
    if (!out) return WRNN_ERR_INVALID;
    *out = nullptr;
    if (!dims) return WRNN_ERR_INVALID;
    wrnn_taco_handle *h = new wrnn_taco_handle();
    *out = h;
    if (dims->struct_size != sizeof(wrnn_taco_dims))
        return wrnn_failf(h, WRNN_ERR_INVALID, "wrnn_taco_dims.struct_size %u, this library's is %zu", dims->struct_size, sizeof(wrnn_taco_dims));
    h->d = *dims;
    const wrnn_taco_dims &d = h->d;
    const int32_t sizes[] = {d.n_symbols, d.num_mels, d.outputs_per_step, d.embedding_dim, d.enc_conv_layers, d.enc_conv_channels, d.enc_conv_kernel,
                             d.encoder_lstm_units, d.attention_dim, d.attention_filters, d.attention_kernel, d.decoder_lstm_units, d.postnet_layers,
                             d.postnet_channels, d.postnet_kernel};
    for (int32_t v : sizes)
        if (v < 1 || v > 65536) return wrnn_failf(h, WRNN_ERR_INVALID, "unsupported dims: every size must be in 1 .. 65536 (got %d)", v);
    if (d.device < 0) return wrnn_failf(h, WRNN_ERR_INVALID, "device %d", d.device);
    if (d.prenet_layers < 1 || d.prenet_layers > WRNN_TACO_MAX_PRENET)
        return wrnn_failf(h, WRNN_ERR_INVALID, "unsupported dims: prenet_layers %d outside 1 .. %d", d.prenet_layers, WRNN_TACO_MAX_PRENET);
    for (int l = 0; l < d.prenet_layers; ++l)
        if (d.prenet_sizes[l] < 1 || d.prenet_sizes[l] > 65536) return wrnn_failf(h, WRNN_ERR_INVALID, "unsupported dims: prenet size %d", d.prenet_sizes[l]);
    if (d.decoder_layers < 1 || d.decoder_layers > MAX_DEC_LAYERS)
        return wrnn_failf(h, WRNN_ERR_INVALID, "unsupported dims: decoder_layers %d outside 1 .. %d", d.decoder_layers, MAX_DEC_LAYERS);
    if (d.enc_conv_kernel > MAX_TAPS || d.attention_kernel > MAX_TAPS || d.postnet_kernel > MAX_TAPS)
        return wrnn_failf(h, WRNN_ERR_INVALID, "unsupported dims: a convolution of more than %d taps", MAX_TAPS);
    if (!(d.zoneout >= 0.0f && d.zoneout <= 1.0f) || !(d.max_abs_value > 0.0f) || !(d.lower_bound_decay >= 0.0f) || !(d.bn_epsilon > 0.0f))
        return wrnn_failf(h, WRNN_ERR_INVALID, "zoneout outside [0, 1], max_abs_value <= 0, lower_bound_decay < 0 or bn_epsilon <= 0");
    const int cin_max = std::max(std::max(d.embedding_dim, d.enc_conv_channels), std::max(d.postnet_channels, std::max(d.num_mels, 2 * d.encoder_lstm_units)));
    const int taps_max = std::max(d.enc_conv_kernel, d.postnet_kernel);
    if ((size_t)(CONV_TT + taps_max - 1) * cin_max * sizeof(float) + sizeof(float) * CONV_THREADS * CONV_TT > LDS_LIMIT)
        return wrnn_failf(h, WRNN_ERR_INVALID, "unsupported dims: a convolution's input tile of %d rows x %d channels exceeds 64 KiB of LDS", CONV_TT + taps_max - 1, cin_max);
    if ((size_t)(6 * d.encoder_lstm_units + 4 * LOOP_THREADS) * sizeof(float) > LDS_LIMIT)
        return wrnn_failf(h, WRNN_ERR_INVALID, "unsupported dims: encoder_lstm_units %d: the recurrence's state exceeds 64 KiB of LDS", d.encoder_lstm_units);
    if (decoder_lds_floats(d, 1, nullptr, nullptr) * sizeof(float) > LDS_LIMIT)
        return wrnn_failf(h, WRNN_ERR_INVALID, "unsupported dims: the decoder's state exceeds 64 KiB of LDS");
    build_table(h);
    h->ok = true;
    return WRNN_OK;
}

int wrnn_taco_tensor_count(const wrnn_taco_handle *h) { return (h && h->ok) ? (int)h->tensors.size() : 0; }

const char *wrnn_taco_tensor_name(const wrnn_taco_handle *h, int index) {
    if (!h || !h->ok || index < 0 || index >= (int)h->tensors.size()) return nullptr;
    return h->tensors[index].name.c_str();
}

int wrnn_taco_tensor_shape(const wrnn_taco_handle *h, int index, int64_t *shape_out) {
    if (!h || !h->ok || index < 0 || index >= (int)h->tensors.size() || !shape_out) return WRNN_ERR_INVALID;
    const Tensor &t = h->tensors[index];
    for (size_t i = 0; i < t.shape.size(); ++i) shape_out[i] = t.shape[i];
    return (int)t.shape.size();
}

int wrnn_taco_load_tensor(wrnn_taco_handle *h, const char *name, const float *data_host, int ndim, const int64_t *shape) {
    if (!h) return WRNN_ERR_INVALID;
    if (!h->ok) return wrnn_failf(h, WRNN_ERR_INVALID, "the handle was refused at creation");
    if (h->destroyed) return wrnn_failf(h, WRNN_ERR_STATE, "the handle was destroyed: it lives only until its last stream is closed");
    if (!name || !data_host || !shape || ndim < 1 || ndim > 3) return wrnn_failf(h, WRNN_ERR_INVALID, "wrnn_taco_load_tensor: a NULL argument or a rank outside 1 .. 3");
    if (h->open_streams > 0) return wrnn_failf(h, WRNN_ERR_STATE, "%d open streams read the weights: close them before loading a tensor", h->open_streams);
    for (Tensor &t : h->tensors) {
        if (t.name != name) continue;
        bool same = (int)t.shape.size() == ndim;
        for (int i = 0; same && i < ndim; ++i) same = t.shape[i] == shape[i];
        if (!same) return wrnn_failf(h, WRNN_ERR_INVALID, "tensor %s: the shape does not match the model's", name);
        const size_t n = t.count();
        for (size_t i = 0; i < n; ++i)
            if (!std::isfinite(data_host[i])) return wrnn_failf(h, WRNN_ERR_INVALID, "tensor %s: element %zu is not finite", name, i);
        t.data.assign(data_host, data_host + n);
        h->dirty = true;
        return WRNN_OK;
    }
    return wrnn_failf(h, WRNN_ERR_MISSING_KEY, "no tensor named %s in this model", name);
}

int wrnn_taco_synthesize(wrnn_taco_handle *h, const wrnn_taco_call *c, void *stream) {
    if (!h) return WRNN_ERR_INVALID;
    if (!h->ok) return wrnn_failf(h, WRNN_ERR_INVALID, "the handle was refused at creation");
    if (h->destroyed) return wrnn_failf(h, WRNN_ERR_STATE, "the handle was destroyed: it lives only until its last stream is closed");
    if (!c) return wrnn_failf(h, WRNN_ERR_INVALID, "call is NULL");
    if (c->struct_size != sizeof(wrnn_taco_call))
        return wrnn_failf(h, WRNN_ERR_INVALID, "wrnn_taco_call.struct_size %u, this library's is %zu", c->struct_size, sizeof(wrnn_taco_call));
    const wrnn_taco_dims &d = h->d;
    const int B = c->B, Tx_max = c->Tx_max, r = d.outputs_per_step;
    int rc = check_text(h, B, Tx_max, c->ids_host, c->tx_host, c->seeds_host);
    if (rc != WRNN_OK) return rc;
    if (!c->decoder_dev || !c->mel_raw_dev || !c->mel_dev || !c->alignments_dev || !c->stop_dev || !c->max_attentions_dev || !c->steps_dev || !c->mel_frames_dev)
        return wrnn_failf(h, WRNN_ERR_INVALID, "an output pointer is NULL");
    if (c->max_iters < 1) return wrnn_failf(h, WRNN_ERR_INVALID, "max_iters %d < 1", c->max_iters);
    if ((rc = check_symbols(h, B, Tx_max, c->ids_host, c->tx_host)) != WRNN_OK) return rc;
    const bool gta = c->gta_dev != nullptr;
    int need_steps = c->max_iters;
    std::vector<int32_t> gsteps(B, 0);
    if (gta) {
        if (!c->gta_frames_host || c->gta_max < r) return wrnn_failf(h, WRNN_ERR_INVALID, "a target needs gta_frames_host and gta_max >= r");
        need_steps = 1;
        for (int b = 0; b < B; ++b) {
            const int f = c->gta_frames_host[b];
            if (f < r || f > c->gta_max || f % r) return wrnn_failf(h, WRNN_ERR_INVALID, "utterance %d: %d target frames: not a multiple of r = %d in r .. gta_max = %d", b, f, r, c->gta_max);
            gsteps[b] = f / r;
            need_steps = std::max(need_steps, f / r);
        }
    }
    const int S = c->steps_max;
    if (S < need_steps || (int64_t)S * r > (1 << 24)) return wrnn_failf(h, WRNN_ERR_INVALID, "steps_max %d: below the %d steps this call can run, or above 2^24 / r", S, need_steps);
    if ((rc = taco_check_decoder_lds(h, Tx_max)) != WRNN_OK) return rc;
    WRNN_TRY(h, hipSetDevice(d.device));
    hipStream_t s = (hipStream_t)stream;
    if ((rc = taco_upload_if_dirty(h)) != WRNN_OK) return rc;
    const TacoBufs o = taco_layout(d, B, Tx_max, S);
    WRNN_TRY(h, h->ws.reserve(o.end, s));
    char *ws = h->ws.p;
    // pageable host memory: these copies return once the source has been read
    WRNN_TRY(h, hipMemcpyAsync(ws + o.ids, c->ids_host, (size_t)B * Tx_max * 4, hipMemcpyHostToDevice, s));
    WRNN_TRY(h, hipMemcpyAsync(ws + o.tx, c->tx_host, (size_t)B * 4, hipMemcpyHostToDevice, s));
    WRNN_TRY(h, hipMemcpyAsync(ws + o.gs, gsteps.data(), (size_t)B * 4, hipMemcpyHostToDevice, s));
    WRNN_TRY(h, hipMemcpyAsync(ws + o.seeds, c->seeds_host, (size_t)B * 8, hipMemcpyHostToDevice, s));
    WRNN_TRY(h, hipStreamSynchronize(s));   // gsteps leaves scope; the caller's arrays may too
    TacoRun run{};
    run.B = B; run.Tx_max = Tx_max; run.S = S; run.gta_max = gta ? c->gta_max : 0; run.max_iters = c->max_iters; run.dropout = c->prenet_dropout ? 1 : 0;
    run.ws = ws; run.o = o; run.gta = c->gta_dev;
    run.encoder = c->encoder_dev; run.decoder = c->decoder_dev; run.mel_raw = c->mel_raw_dev; run.mel = c->mel_dev;
    run.alignments = c->alignments_dev; run.stop = c->stop_dev;
    run.max_attentions = c->max_attentions_dev; run.steps = c->steps_dev; run.mel_frames = c->mel_frames_dev;
    return taco_run(h, s, run);
}

const char *wrnn_taco_last_error(const wrnn_taco_handle *h) { return wrnn_last_error_of(h); }

int wrnn_taco_stream_halo(const wrnn_taco_dims *dims) {
    if (!dims || dims->postnet_layers < 0 || dims->postnet_kernel < 1) return WRNN_ERR_INVALID;
    return dims->postnet_layers * postnet_reach(*dims);
}

int wrnn_taco_stream_open(wrnn_taco_handle *h, const wrnn_taco_stream_opts *o, void *stream, wrnn_taco_stream **out) {
    if (out) *out = nullptr;
    if (!h) return WRNN_ERR_INVALID;
    if (!h->ok) return wrnn_failf(h, WRNN_ERR_INVALID, "the handle was refused at creation");
    if (h->destroyed) return wrnn_failf(h, WRNN_ERR_STATE, "the handle was destroyed: it lives only until its last stream is closed");
    if (!o || !out) return wrnn_failf(h, WRNN_ERR_INVALID, "opts or out is NULL");
    if (o->struct_size != sizeof(wrnn_taco_stream_opts))
        return wrnn_failf(h, WRNN_ERR_INVALID, "wrnn_taco_stream_opts.struct_size %u, this library's is %zu", o->struct_size, sizeof(wrnn_taco_stream_opts));
    if (o->gta_dev) return wrnn_failf(h, WRNN_ERR_INVALID, "a stream is free-running: teacher forcing has the whole target in hand, use wrnn_taco_synthesize");
    const wrnn_taco_dims &d = h->d;
    const int B = o->B, Tx_max = o->Tx_max, r = d.outputs_per_step, M = d.num_mels, S = o->max_iters;
    int rc = check_text(h, B, Tx_max, o->ids_host, o->tx_host, o->seeds_host);
    if (rc != WRNN_OK) return rc;
    if (S < 1) return wrnn_failf(h, WRNN_ERR_INVALID, "max_iters %d < 1", S);
    if ((rc = check_symbols(h, B, Tx_max, o->ids_host, o->tx_host)) != WRNN_OK) return rc;
    if ((int64_t)S * r > (1 << 24)) return wrnn_failf(h, WRNN_ERR_INVALID, "max_iters %d: above 2^24 / r", S);
    int Pmax = 0, Kmax = 0;
    const size_t dec_lds = decoder_lds_floats(d, Tx_max, &Pmax, &Kmax) * sizeof(float);
    if (dec_lds > LDS_LIMIT) return wrnn_failf(h, WRNN_ERR_INVALID, "the decoder's state for Tx_max %d exceeds 64 KiB of LDS", Tx_max);
    WRNN_TRY(h, hipSetDevice(d.device));
    hipStream_t s = (hipStream_t)stream;
    if (h->dirty && (rc = upload(h)) != WRNN_OK) return rc;
    const int C = d.enc_conv_channels, H = d.encoder_lstm_units, E2 = 2 * H, A = d.attention_dim, PC = d.postnet_channels, T_out = S * r, LD = d.decoder_layers * d.decoder_lstm_units;
    const size_t enc_act = (size_t)B * Tx_max * std::max(C, d.embedding_dim), frames = (size_t)B * T_out * M;
    const int st_stride = (int)up64((size_t)M + 2 * (size_t)LD + E2 + 2 * (size_t)Tx_max + 1);
    size_t at = 0;
    auto take = [&at](size_t bytes) { const size_t off = at; at += wrnn_up256(bytes); return off; };
    const size_t o_ids = take((size_t)B * Tx_max * 4), o_tx = take((size_t)B * 4), o_seed = take((size_t)B * 8);
    const size_t o_a0 = take(enc_act * 4), o_a1 = take(enc_act * 4), o_xp0 = take((size_t)B * Tx_max * 4 * H * 4), o_xp1 = take((size_t)B * Tx_max * 4 * H * 4);
    const size_t o_mem = take((size_t)B * Tx_max * E2 * 4), o_keys = take((size_t)B * Tx_max * A * 4);
    const size_t o_sf = take((size_t)B * st_stride * 4), o_si = take((size_t)B * ST_INTS * 4);
    const size_t o_dec = take(frames * 4), o_res = take(frames * 4), o_raw = take(frames * 4), o_mel = take(frames * 4);
    const size_t o_ali = take((size_t)B * S * Tx_max * 4), o_stop = take((size_t)B * T_out * 4), o_ma = take((size_t)B * S * 4);
    const size_t o_steps = take((size_t)B * 4), o_mf = take((size_t)B * 4);
    std::vector<size_t> o_post;
    for (int i = 0; i < d.postnet_layers; ++i) o_post.push_back(take((size_t)B * T_out * PC * 4));
    wrnn_taco_stream *st = new wrnn_taco_stream();
    auto fail = [&](int code) { free_stream(st); return code; };
    hipError_t e = hipMalloc((void **)&st->ws, at);
    if (e == hipSuccess) e = hipHostMalloc((void **)&st->host_i, (size_t)B * ST_INTS * 4, hipHostMallocDefault);
    if (e != hipSuccess) return fail(wrnn_failf(h, WRNN_ERR_HIP, "a stream's workspace of %zu bytes: %s", at, hipGetErrorString(e)));
    char *ws = st->ws;
    st->h = h; st->B = B; st->Tx_max = Tx_max; st->S = S; st->dropout = o->prenet_dropout ? 1 : 0; st->ws_bytes = at;
    st->ids = (int32_t *)(ws + o_ids); st->tx = (int32_t *)(ws + o_tx); st->seeds = (uint64_t *)(ws + o_seed);
    st->mem = (float *)(ws + o_mem); st->keys = (float *)(ws + o_keys); st->st_f = (float *)(ws + o_sf); st->st_i = (int32_t *)(ws + o_si);
    st->decoder = (float *)(ws + o_dec); st->residual = (float *)(ws + o_res); st->mel_raw = (float *)(ws + o_raw); st->mel = (float *)(ws + o_mel);
    st->alignments = (float *)(ws + o_ali); st->stop = (float *)(ws + o_stop); st->max_attentions = (int32_t *)(ws + o_ma);
    st->steps = (int32_t *)(ws + o_steps); st->mel_frames = (int32_t *)(ws + o_mf);
    for (size_t off : o_post) st->post.push_back((float *)(ws + off));
    st->st_stride = st_stride; st->Pmax = Pmax; st->Kmax = Kmax; st->dec_lds = dec_lds;
    // everything starts as zeros: the outputs past an utterance's end stay so, and step 0 of the state means "not begun"
    if ((e = hipMemsetAsync(ws, 0, at, s)) == hipSuccess) e = hipMemcpyAsync(st->ids, o->ids_host, (size_t)B * Tx_max * 4, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipMemcpyAsync(st->tx, o->tx_host, (size_t)B * 4, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipMemcpyAsync(st->seeds, o->seeds_host, (size_t)B * 8, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);   // the caller's arrays may leave scope
    if (e != hipSuccess) return fail(wrnn_failf(h, WRNN_ERR_HIP, "a stream's inputs: %s", hipGetErrorString(e)));
    const EncBufs eb{st->ids, st->tx, (float *)(ws + o_a0), (float *)(ws + o_a1), {(float *)(ws + o_xp0), (float *)(ws + o_xp1)}, st->mem, st->keys};
    if ((rc = run_encoder(h, s, eb, B, Tx_max)) != WRNN_OK) return fail(rc);
    ++h->open_streams;
    *out = st;
    return WRNN_OK;
}

int wrnn_taco_stream_step(wrnn_taco_stream *st, int32_t n_steps, void *stream, int32_t *decoded_host, int32_t *final_host, int32_t *finished_host) {
    if (!st) return WRNN_ERR_INVALID;
    if (n_steps < 1) return wrnn_failf(st, WRNN_ERR_INVALID, "n_steps %d < 1", n_steps);
    if (!decoded_host || !final_host || !finished_host) return wrnn_failf(st, WRNN_ERR_INVALID, "decoded_host, final_host or finished_host is NULL");
    if (st->done) return wrnn_failf(st, WRNN_ERR_STATE, "every utterance of the stream has finished");
    wrnn_taco_handle *h = st->h;
    const wrnn_taco_dims &d = h->d;
    const int B = st->B, S = st->S, r = d.outputs_per_step, M = d.num_mels, PC = d.postnet_channels, T_out = S * r;
    const int n = std::min(n_steps, S), reach = postnet_reach(d), halo = d.postnet_layers * reach;
    WRNN_TRY(st, hipSetDevice(d.device));
    hipStream_t s = (hipStream_t)stream;
    DecArgs g{};
    g.memory = st->mem; g.keys = st->keys; g.tx = st->tx; g.seeds = st->seeds;
    decoder_model_args(h, g);
    g.decoder = st->decoder; g.alignments = st->alignments; g.stop = st->stop;
    g.max_attentions = st->max_attentions; g.steps = st->steps; g.mel_frames = st->mel_frames;
    g.Tx_max = st->Tx_max; g.max_iters = S; g.steps_max = S; g.dropout = st->dropout; g.Pmax = st->Pmax; g.Kmax = st->Kmax;
    const DecState ds{st->st_f, st->st_i, st->st_stride, n};
    hipLaunchKernelGGL(taco_decoder_kernel<true>, dim3((unsigned)B), dim3(LOOP_THREADS), st->dec_lds, s, g, ds);
    WRNN_TRY(st, hipGetLastError());
    // layer i (1-based) is held i reach rows behind the decoder while the utterance runs; a push adds n r rows at most, and the rows held
    // back when it ends; one tile more, since the tiles are aligned and the range need not be
    const float *img = h->img, *pin = st->decoder;
    for (int i = 0; i <= d.postnet_layers; ++i) {
        const bool proj = i == d.postnet_layers;
        const std::string p = post_conv(i + 1);
        ConvArgs a{};
        a.in = pin;
        a.w = tensor_at(h, proj ? std::string(POSTP) + "kernel" : p + "conv1d/kernel");
        a.bias = tensor_at(h, proj ? std::string(POSTP) + "bias" : p + "conv1d/bias");
        a.bn_s = proj ? nullptr : img + h->off_bn_post + (size_t)i * 2 * up64(PC);
        a.bn_b = proj ? nullptr : a.bn_s + up64(PC);
        a.out = proj ? st->residual : st->post[i];
        a.len_mul = r; a.T_max = T_out; a.Cin = i ? PC : M; a.Cout = proj ? M : PC; a.taps = proj ? 1 : d.postnet_kernel;
        a.act = i + 1 < d.postnet_layers ? 2 : 0;
        const ConvWindow cw{st->st_i, std::min(i + 1, (int)d.postnet_layers) * reach};
        const long rows = std::min((long)n * r + cw.held, (long)T_out);
        hipLaunchKernelGGL(taco_conv_kernel<true>, dim3((unsigned)((rows + CONV_TT - 1) / CONV_TT + 1), (unsigned)B, (unsigned)((a.Cout + 63) / 64)), dim3(CONV_THREADS),
                           (size_t)(CONV_TT + a.taps - 1) * a.Cin * sizeof(float), s, a, cw);
        WRNN_TRY(st, hipGetLastError());
        pin = a.out;
    }
    FinishArgs f{st->decoder, st->residual, st->steps, st->mel_raw, st->mel, T_out, M, r, g.clip_lo, g.clip_hi};
    const long frows = std::min((long)n * r + halo, (long)T_out);
    hipLaunchKernelGGL(taco_finish_window_kernel, dim3((unsigned)((frows * M + CONV_THREADS - 1) / CONV_THREADS), (unsigned)B), dim3(CONV_THREADS), 0, s, f, st->st_i, halo);
    WRNN_TRY(st, hipGetLastError());
    WRNN_TRY(st, hipMemcpyAsync(st->host_i, st->st_i, (size_t)B * ST_INTS * 4, hipMemcpyDeviceToHost, s));
    WRNN_TRY(st, hipStreamSynchronize(s));   // the one wait of a push
    bool done = true;
    for (int b = 0; b < B; ++b) {
        const int32_t *si = st->host_i + (size_t)b * ST_INTS;
        const int frames = si[ST_STEP] * r, fin = si[ST_FINISHED];
        decoded_host[b] = frames;
        finished_host[b] = fin;
        final_host[b] = fin ? (si[ST_FIRST_STOP] >= 0 ? si[ST_FIRST_STOP] : frames) : std::max(frames - halo, 0);
        done = done && fin;
    }
    st->done = done;
    return WRNN_OK;
}

int wrnn_taco_stream_view(const wrnn_taco_stream *st, wrnn_taco_stream_outputs *v) {
    if (!st || !v) return WRNN_ERR_INVALID;
    if (v->struct_size != sizeof(wrnn_taco_stream_outputs)) return WRNN_ERR_INVALID;
    const wrnn_taco_dims &d = st->h->d;
    const int64_t T_out = (int64_t)st->S * d.outputs_per_step;
    v->encoder_dev = st->mem; v->decoder_dev = st->decoder; v->mel_raw_dev = st->mel_raw; v->mel_dev = st->mel;
    v->alignments_dev = st->alignments; v->stop_dev = st->stop; v->max_attentions_dev = st->max_attentions;
    v->steps_dev = st->steps; v->mel_frames_dev = st->mel_frames;
    v->encoder_stride = (int64_t)st->Tx_max * 2 * d.encoder_lstm_units;
    v->frames_stride = T_out * d.num_mels;
    v->alignments_stride = (int64_t)st->S * st->Tx_max;
    v->stop_stride = T_out;
    v->max_attentions_stride = st->S;
    return WRNN_OK;
}

int wrnn_taco_stream_info(const wrnn_taco_stream *st, int32_t *B, int32_t *Tx_max, int32_t *max_iters, int32_t *halo, int64_t *workspace_bytes) {
    if (!st) return WRNN_ERR_INVALID;
    if (B) *B = st->B;
    if (Tx_max) *Tx_max = st->Tx_max;
    if (max_iters) *max_iters = st->S;
    if (halo) *halo = wrnn_taco_stream_halo(&st->h->d);
    if (workspace_bytes) *workspace_bytes = (int64_t)st->ws_bytes;
    return WRNN_OK;
}

const char *wrnn_taco_stream_last_error(const wrnn_taco_stream *st) { return wrnn_last_error_of(st); }

void wrnn_taco_stream_close(wrnn_taco_stream *st) {
    if (!st) return;
    wrnn_taco_handle *h = st->h;
    (void)hipSetDevice(h->d.device);
    free_stream(st);   // hipFree waits for the work that still uses the allocation (the encoder of an open that was never stepped)
    if (--h->open_streams == 0 && h->destroyed) wrnn_taco_destroy(h);
}

void wrnn_taco_destroy(wrnn_taco_handle *h) {
    if (!h) return;
    if (h->open_streams > 0) {   // its streams read the weight image: the last wrnn_taco_stream_close frees the handle
        h->destroyed = true;
        return;
    }
    if (h->img || h->ws.p || h->gta_ws.p) {
        (void)hipSetDevice(h->d.device);
        if (h->img) (void)hipFree(h->img);
        h->ws.release();
        h->gta_ws.release();
    }
    delete h;
}

}  // extern "C"
