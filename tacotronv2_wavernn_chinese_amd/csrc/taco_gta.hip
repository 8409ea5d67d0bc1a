// The GTA corpus: a group of utterances of a device-resident mel table -> the mels the Tacotron predicts under teacher forcing, in a
// table of the same layout.  The definitions are in the header's section.
//   taco_gta_pack_kernel    grid (ceil(gta_max / 8), B)   the [0, 1] mel -> the (B, gta_max, M) target the decoder reads, the -A padding
//                                                         rows up to a multiple of r, zeros behind; the utterance's step count
//   (encoder, decoder, postnet, finish: taco_run of tacotron.hip, the launches of wrnn_taco_synthesize)
//   taco_gta_unpack_kernel  grid (B)                      the first frames[b] rows of the call's [0, 1] mel -> the output table; l1[b]
//   taco_gta_align_kernel   grid (B)                      focus[b], last_attention[b]; a wave per step's row
// The two sums are float64 with a fixed assignment (mel element x in thread x mod 256, step s in wave s mod 4), the threads' sums through
// block_sums' tree.
#include <algorithm>
#include <cstdint>

#include "dsp_device.h"
#include "taco_internal.h"

namespace {

constexpr int GTA_THREADS = 256;
constexpr int PACK_ROWS = 8;   // target rows per workgroup of the pack kernel

struct PackArgs {
    const float *mels;         // the ground-truth table
    const int64_t *mel_off;    // (B)
    const int32_t *frames;     // (B)
    float *target;             // (B, gta_max, M)
    int32_t *gs;               // (B): ceil(frames / r)
    int32_t gta_max, M, r;
    float A;
};
__global__ void __launch_bounds__(GTA_THREADS) taco_gta_pack_kernel(PackArgs g) {
    const int b = blockIdx.y, t0 = blockIdx.x * PACK_ROWS;
    const int frames = min(max(g.frames[b], 0), g.gta_max);   // the host has checked it; this keeps the reads inside the utterance regardless
    const int steps = (frames + g.r - 1) / g.r, padded = steps * g.r;
    if (blockIdx.x == 0 && threadIdx.x == 0) g.gs[b] = steps;
    const float *src = g.mels + g.mel_off[b];
    float *dst = g.target + (long)b * g.gta_max * g.M;
    const int n = min(PACK_ROWS, g.gta_max - t0) * g.M;
    for (int x = threadIdx.x; x < n; x += GTA_THREADS) {
        const int t = t0 + x / g.M;
        const long at = (long)t0 * g.M + x;
        float v = 0.0f;
        if (t < frames) v = fminf(fmaxf(__fsub_rn(__fmul_rn(2.0f * g.A, src[at]), g.A), -g.A), g.A);   // two roundings, never one fused
        else if (t < padded) v = -g.A;
        dst[at] = v;
    }
}

struct UnpackArgs {
    const float *mel;          // (B, T_out, M): the call's [0, 1] mel
    const float *truth;        // the ground-truth table
    const int64_t *mel_off, *out_off;   // (B)
    const int32_t *frames;     // (B)
    float *out;                // the output table
    double *l1;                // (B)
    int32_t T_out, M;
};
__global__ void __launch_bounds__(GTA_THREADS) taco_gta_unpack_kernel(UnpackArgs g) {
    __shared__ double acc[GTA_THREADS];
    const int b = blockIdx.x;
    const int frames = min(max(g.frames[b], 0), g.T_out);
    const long n = (long)frames * g.M;
    const float *mel = g.mel + (long)b * g.T_out * g.M, *truth = g.truth + g.mel_off[b];
    float *out = g.out + g.out_off[b];
    double v[1] = {0.0};
    for (long x = threadIdx.x; x < n; x += GTA_THREADS) {
        const float m = mel[x];
        out[x] = m;
        v[0] += fabs((double)m - (double)truth[x]);
    }
    block_sums<GTA_THREADS, 1>(v, acc);
    if (threadIdx.x == 0) g.l1[b] = n > 0 ? v[0] / (double)n : 0.0;
}

struct AlignArgs {
    const float *alignments;        // (B, S, Tx_max)
    const int32_t *max_attentions;  // (B, S)
    const int32_t *gs, *tx;         // (B)
    double *focus;                  // (B)
    int32_t *last_attention;        // (B)
    int32_t S, Tx_max;
};
// A wave takes a step's row (neighbouring lanes read neighbouring floats); step s is always wave s mod 4's, whose lane 0 adds the row's
// largest value to its sum; the four sums go through block_sums' tree with the other lanes' zeros.
__global__ void __launch_bounds__(GTA_THREADS) taco_gta_align_kernel(AlignArgs g) {
    __shared__ double acc[GTA_THREADS];
    const int b = blockIdx.x, wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int steps = min(max(g.gs[b], 0), g.S), Tx = min(max(g.tx[b], 1), g.Tx_max);
    const float *al = g.alignments + (long)b * g.S * g.Tx_max;
    double v[1] = {0.0};
    for (int s = wave; s < steps; s += GTA_THREADS / 64) {
        const float *row = al + (long)s * g.Tx_max;
        float mx = -INFINITY;
        for (int t = lane; t < Tx; t += 64) mx = fmaxf(mx, row[t]);
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) mx = fmaxf(mx, __shfl_xor(mx, off, 64));
        if (lane == 0) v[0] += (double)mx;
    }
    block_sums<GTA_THREADS, 1>(v, acc);
    if (threadIdx.x == 0) {
        g.focus[b] = steps > 0 ? v[0] / (double)steps : 0.0;
        g.last_attention[b] = steps > 0 ? g.max_attentions[(long)b * g.S + steps - 1] : 0;
    }
}

// Byte offsets of a group's scratch behind what taco_run keeps: the group's tables, the packed target and every output of the call.
// Every extent grows with B, Tx_max and S, so the need of the largest group covers every other group's.
struct GtaBufs {
    TacoBufs o;
    size_t fr, mo, oo, tg, dec, raw, mel, ali, stop, ma, steps, mf, end;
};
GtaBufs gta_layout(const wrnn_taco_dims &d, int B, int Tx_max, int S) {
    GtaBufs g{};
    g.o = taco_layout(d, B, Tx_max, S);
    size_t at = g.o.end;
    auto take = [&at](size_t bytes) { const size_t off = at; at += wrnn_up256(bytes); return off; };
    const size_t T_out = (size_t)S * d.outputs_per_step, frame_bytes = (size_t)B * T_out * d.num_mels * 4;
    g.fr = take((size_t)B * 4); g.mo = take((size_t)B * 8); g.oo = take((size_t)B * 8); g.tg = take(frame_bytes);
    g.dec = take(frame_bytes); g.raw = take(frame_bytes); g.mel = take(frame_bytes);
    g.ali = take((size_t)B * S * Tx_max * 4); g.stop = take((size_t)B * T_out * 4); g.ma = take((size_t)B * S * 4);
    g.steps = take((size_t)B * 4); g.mf = take((size_t)B * 4);
    g.end = at;
    return g;
}

}  // namespace

extern "C" int wrnn_taco_gta_reserve(wrnn_taco_handle *h, int32_t B, int32_t Tx_max, int32_t frames_max, void *stream) {
    if (!h) return WRNN_ERR_INVALID;
    if (!h->ok) return wrnn_failf(h, WRNN_ERR_INVALID, "the handle was refused at creation");
    if (h->destroyed) return wrnn_failf(h, WRNN_ERR_STATE, "the handle was destroyed: it lives only until its last stream is closed");
    if (B < 1 || B > WRNN_MAX_GRID_Y) return wrnn_failf(h, WRNN_ERR_INVALID, "B %d outside 1 .. 65535", B);
    if (Tx_max < 1 || Tx_max > WRNN_TACO_MAX_TX) return wrnn_failf(h, WRNN_ERR_INVALID, "Tx_max %d outside 1 .. %d symbols", Tx_max, WRNN_TACO_MAX_TX);
    if (frames_max < 1 || frames_max > (1 << 24)) return wrnn_failf(h, WRNN_ERR_INVALID, "frames_max %d outside 1 .. 2^24", frames_max);
    const int r = h->d.outputs_per_step;
    WRNN_TRY(h, hipSetDevice(h->d.device));
    WRNN_TRY(h, h->gta_ws.reserve(gta_layout(h->d, B, Tx_max, (frames_max + r - 1) / r).end, (hipStream_t)stream));
    return WRNN_OK;
}

extern "C" int64_t wrnn_taco_gta_workspace_bytes(const wrnn_taco_handle *h) { return h ? (int64_t)h->gta_ws.cap : 0; }

extern "C" int wrnn_taco_gta_corpus(wrnn_taco_handle *h, const wrnn_taco_gta_call *c, void *stream) {
    if (!h) return WRNN_ERR_INVALID;
    if (!h->ok) return wrnn_failf(h, WRNN_ERR_INVALID, "the handle was refused at creation");
    if (h->destroyed) return wrnn_failf(h, WRNN_ERR_STATE, "the handle was destroyed: it lives only until its last stream is closed");
    if (!c) return wrnn_failf(h, WRNN_ERR_INVALID, "call is NULL");
    if (c->struct_size != sizeof(wrnn_taco_gta_call))
        return wrnn_failf(h, WRNN_ERR_INVALID, "wrnn_taco_gta_call.struct_size %u, this library's is %zu", c->struct_size, sizeof(wrnn_taco_gta_call));
    const wrnn_taco_dims &d = h->d;
    const int B = c->B, Tx_max = c->Tx_max, r = d.outputs_per_step, M = d.num_mels;
    // a group is cut from a corpus: the utterance that is too long is named (the refusal of taco_check_symbols), before
    // taco_check_text refuses the group's Tx_max for it
    if (c->tx_host && B >= 1 && B <= WRNN_MAX_GRID_Y)
        for (int b = 0; b < B; ++b)
            if (c->tx_host[b] > WRNN_TACO_MAX_TX) return taco_refuse_length(h, b, c->tx_host[b], Tx_max);
    int rc = taco_check_text(h, B, Tx_max, c->ids_host, c->tx_host, c->seeds_host);
    if (rc != WRNN_OK) return rc;
    if (!c->gta_mels_dev || !c->l1_dev || !c->focus_dev || !c->last_attention_dev) return wrnn_failf(h, WRNN_ERR_INVALID, "an output pointer is NULL");
    if (!c->mels_dev || !c->frames_host || !c->mel_off_host || !c->out_off_host)
        return wrnn_failf(h, WRNN_ERR_INVALID, "mels_dev, frames_host, mel_off_host or out_off_host is NULL");
    if ((rc = taco_check_symbols(h, B, Tx_max, c->ids_host, c->tx_host)) != WRNN_OK) return rc;
    int S = 1;
    for (int b = 0; b < B; ++b) {
        const int64_t f = c->frames_host[b], n = f * M, mo = c->mel_off_host[b], oo = c->out_off_host[b];
        if (f < 1) return wrnn_failf(h, WRNN_ERR_INVALID, "utterance %d: %lld mel frames < 1", b, (long long)f);
        if (f > (1 << 24)) return wrnn_failf(h, WRNN_ERR_INVALID, "utterance %d: %lld mel frames above 2^24", b, (long long)f);
        if (mo < 0 || mo > c->mels_elems || n > c->mels_elems - mo)
            return wrnn_failf(h, WRNN_ERR_INVALID, "utterance %d: elements %lld .. %lld lie outside the mel table of %lld", b, (long long)mo, (long long)(mo + n),
                              (long long)c->mels_elems);
        if (oo < 0 || oo > c->out_elems || n > c->out_elems - oo)
            return wrnn_failf(h, WRNN_ERR_INVALID, "utterance %d: elements %lld .. %lld lie outside the output table of %lld", b, (long long)oo, (long long)(oo + n),
                              (long long)c->out_elems);
        S = std::max(S, (int)((f + r - 1) / r));
    }
    if ((int64_t)S * r > (1 << 24)) return wrnn_failf(h, WRNN_ERR_INVALID, "a group of up to %d decoder steps: above 2^24 / r", S);
    if ((rc = taco_check_decoder_lds(h, Tx_max)) != WRNN_OK) return rc;
    WRNN_TRY(h, hipSetDevice(d.device));
    hipStream_t s = (hipStream_t)stream;
    if ((rc = taco_upload_if_dirty(h)) != WRNN_OK) return rc;
    // the scratch: what taco_run keeps, then the tables of the group, the target and every output of the call
    const int gta_max = S * r, T_out = gta_max;
    const GtaBufs gb = gta_layout(d, B, Tx_max, S);
    const TacoBufs &o = gb.o;
    WRNN_TRY(h, h->gta_ws.reserve(gb.end, s));   // waits only when it grows: wrnn_taco_gta_reserve sizes it for a whole corpus beforehand
    char *ws = h->gta_ws.p;
    int32_t *frames = (int32_t *)(ws + gb.fr);
    int64_t *mel_off = (int64_t *)(ws + gb.mo), *out_off = (int64_t *)(ws + gb.oo);
    float *target = (float *)(ws + gb.tg);
    // queued, not waited for: the caller keeps the arrays until the stream has passed the call
    WRNN_TRY(h, hipMemcpyAsync(ws + o.ids, c->ids_host, (size_t)B * Tx_max * 4, hipMemcpyHostToDevice, s));
    WRNN_TRY(h, hipMemcpyAsync(ws + o.tx, c->tx_host, (size_t)B * 4, hipMemcpyHostToDevice, s));
    WRNN_TRY(h, hipMemcpyAsync(ws + o.seeds, c->seeds_host, (size_t)B * 8, hipMemcpyHostToDevice, s));
    WRNN_TRY(h, hipMemcpyAsync(frames, c->frames_host, (size_t)B * 4, hipMemcpyHostToDevice, s));
    WRNN_TRY(h, hipMemcpyAsync(mel_off, c->mel_off_host, (size_t)B * 8, hipMemcpyHostToDevice, s));
    WRNN_TRY(h, hipMemcpyAsync(out_off, c->out_off_host, (size_t)B * 8, hipMemcpyHostToDevice, s));
    PackArgs pk{c->mels_dev, mel_off, frames, target, (int32_t *)(ws + o.gs), gta_max, M, r, d.max_abs_value};
    hipLaunchKernelGGL(taco_gta_pack_kernel, dim3((unsigned)((gta_max + PACK_ROWS - 1) / PACK_ROWS), (unsigned)B), dim3(GTA_THREADS), 0, s, pk);
    WRNN_TRY(h, hipGetLastError());
    TacoRun run{};
    run.B = B; run.Tx_max = Tx_max; run.S = S; run.gta_max = gta_max; run.max_iters = S; run.dropout = c->prenet_dropout ? 1 : 0;
    run.ws = ws; run.o = o; run.gta = target;
    run.encoder = nullptr; run.decoder = (float *)(ws + gb.dec); run.mel_raw = (float *)(ws + gb.raw); run.mel = (float *)(ws + gb.mel);
    run.alignments = (float *)(ws + gb.ali); run.stop = (float *)(ws + gb.stop);
    run.max_attentions = (int32_t *)(ws + gb.ma); run.steps = (int32_t *)(ws + gb.steps); run.mel_frames = (int32_t *)(ws + gb.mf);
    if ((rc = taco_run(h, s, run)) != WRNN_OK) return rc;
    UnpackArgs up{run.mel, c->mels_dev, mel_off, out_off, frames, c->gta_mels_dev, c->l1_dev, T_out, M};
    hipLaunchKernelGGL(taco_gta_unpack_kernel, dim3((unsigned)B), dim3(GTA_THREADS), 0, s, up);
    WRNN_TRY(h, hipGetLastError());
    AlignArgs al{run.alignments, run.max_attentions, (const int32_t *)(ws + o.gs), (const int32_t *)(ws + o.tx), c->focus_dev, c->last_attention_dev, S, Tx_max};
    hipLaunchKernelGGL(taco_gta_align_kernel, dim3((unsigned)B), dim3(GTA_THREADS), 0, s, al);
    WRNN_TRY(h, hipGetLastError());
    return WRNN_OK;
}
