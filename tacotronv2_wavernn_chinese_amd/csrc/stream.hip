// Streaming generation (wrnn_stream_*, include/wavernn_amd.h): audio leaves while mel frames are still arriving.
//
// A push conditions only the frames whose steps became ready, on a compacted window: the window's mel frames
// [f0 - pad, f1 + pad) are gathered from the stream's bounded mel history and the new frames (zeros before frame 0 and,
// after the last push, past the end -- the zero padding generate() applies, :183-185) into one (B, feat, Tw + 2 pad)
// buffer, and the offline prologue kernels run on it in their `mels_padded` form.  Their per-frame arithmetic does not
// depend on where a frame sits in the clip, so the window's tables hold exactly the values the offline tables hold for
// those frames.  The loop kernels see the window through their row table: row r starts at position -f0 * hop, so the
// frame index they derive from (start + absolute step) is window-relative, while the Philox noise stays keyed by the
// absolute step.  The recurrent state crosses pushes through the stream's `state` like TEAM2 segments cross launches.
#include <climits>

#include "wrnn_internal.h"

struct wrnn_stream {
    wrnn_handle *h = nullptr;
    int device = 0;
    int B = 0, kernel = WRNN_KERNEL_SIMPLE, noise_mode = WRNN_NOISE_PHILOX;
    uint64_t seed = 0;
    int64_t frames_in = 0, steps_done = 0;
    bool ended = false, poisoned = false;
    // mel history: frames [hist0, frames_in) of every row, (B, F, frames_in - hist0), in hist[cur]; the other buffer receives
    // the next push's history
    float *hist[2] = {nullptr, nullptr};
    size_t hist_cap[2] = {0, 0};
    int cur = 0;
    int64_t hist0 = 0;
    float *win = nullptr, *aux = nullptr, *tab = nullptr, *cond = nullptr, *state = nullptr;
    size_t win_cap = 0, aux_cap = 0, tab_cap = 0, cond_cap = 0, state_cap = 0;
    WrnnRow *rows = nullptr;
    int32_t *sched = nullptr;
    int n_slots = 0;
    unsigned *err = nullptr;   // device error word of this stream's team launches
};

namespace {

// out[b][f][k] = frame o0 + k of row b: 0 outside [0, limit), else from the history (frames [h0, h0 + hn)) or the pushed mels
// (frames [p0, p0 + pn)).  Every frame the host asks for lies in one of the three ranges.
__global__ void stream_gather_kernel(const float *__restrict__ hist, int64_t h0, int hn, const float *__restrict__ push, int64_t p0,
                                     int pn, float *__restrict__ out, int64_t o0, int on, int F, int64_t limit) {
    const int b = blockIdx.y;
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= F * on) return;
    const int f = i / on, k = i - f * on;
    const int64_t fr = o0 + k;
    float v = 0.0f;
    if (fr >= 0 && fr < limit) {
        if (fr >= h0 && fr < h0 + hn) v = hist[((size_t)b * F + f) * hn + (fr - h0)];
        else if (fr >= p0 && fr < p0 + pn) v = push[((size_t)b * F + f) * pn + (fr - p0)];
    }
    out[((size_t)b * F + f) * on + k] = v;
}

hipError_t launch_gather(const float *hist, int64_t h0, int hn, const float *push, int64_t p0, int pn, float *out, int64_t o0, int on,
                         int B, int F, int64_t limit, hipStream_t s) {
    (void)hipGetLastError();
    if (on <= 0) return hipSuccess;
    dim3 grid((unsigned)((F * on + 255) / 256), B);
    hipLaunchKernelGGL(stream_gather_kernel, grid, dim3(256), 0, s, hist, h0, hn, push, p0, pn, out, o0, on, F, limit);
    return hipGetLastError();
}

// row table of a push: row r = utterance r, `steps` steps, first upsampled position `start` (= -f0 * hop: window-relative
// frames); sched = identity, -1 in the empty slots of the last pass (TEAM2's ragged instantiation, B > 1)
__global__ void stream_rows_kernel(WrnnRow *rows, int32_t *sched, int B, int n_slots, int32_t steps, int64_t start) {
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r < B) {
        WrnnRow w;
        w.utt = r; w.steps = steps; w.start = start;
        rows[r] = w;
    }
    if (r < n_slots) sched[r] = r < B ? r : -1;
}

size_t state_floats(const wrnn_handle *h) {
    const size_t simple = (size_t)wrnn_simple_state_floats(h->d);
    return simple > (size_t)WRNN_TEAM_STATE_FLOATS ? simple : (size_t)WRNN_TEAM_STATE_FLOATS;
}

}  // namespace

extern "C" {

int64_t wrnn_stream_ready_steps(int64_t frames_in, int32_t hop, int32_t pad, int32_t last) {
    if (frames_in < 0 || hop < 1 || pad < 0) return -1;
    if (last) return frames_in * hop;
    const int64_t r = (frames_in - pad) * (int64_t)hop;
    return r > 0 ? (r & ~(int64_t)31) : 0;
}

int wrnn_stream_open(wrnn_handle *h, int32_t B, const wrnn_sample_opts *opts, wrnn_stream **out) {
    if (!h || !opts || !out || B < 1) return wrnn_failf(h, WRNN_ERR_INVALID, "wrnn_stream_open: bad arguments");
    *out = nullptr;
    if (opts->struct_size != sizeof(wrnn_sample_opts))
        return wrnn_failf(h, WRNN_ERR_INVALID, "wrnn_sample_opts.struct_size is %u, this library (ABI %d) expects %zu", opts->struct_size,
                     WRNN_ABI_VERSION, sizeof(wrnn_sample_opts));
    if (!h->loaded) return wrnn_failf(h, WRNN_ERR_STATE, "weights not loaded");
    if (opts->noise_mode != WRNN_NOISE_PHILOX && opts->noise_mode != WRNN_NOISE_ARGMAX)
        return wrnn_failf(h, WRNN_ERR_INVALID, "a stream draws its noise on the device: noise_mode must be WRNN_NOISE_PHILOX or WRNN_NOISE_ARGMAX");
    if (opts->noise_mode == WRNN_NOISE_ARGMAX && h->d.mode != WRNN_MODE_RAW) return wrnn_failf(h, WRNN_ERR_INVALID, "WRNN_NOISE_ARGMAX is RAW-only");
    if (opts->mels_padded || opts->noise1_dev || opts->noise2_dev || opts->x_forced_dev || opts->logits_out_dev || opts->x_init_dev ||
        opts->frames_dev || opts->batch_rows || opts->team2_segment || opts->utt_seeds_dev)
        return wrnn_failf(h, WRNN_ERR_INVALID, "a stream takes noise_mode, kernel and seed only: mels_padded, the pointers (utt_seeds_dev included) and the tuning fields must be 0");
    const char *team_no = wrnn_loop_team_obstacle(h);
    int kernel = opts->kernel;
    if (kernel == WRNN_KERNEL_AUTO) kernel = team_no ? WRNN_KERNEL_SIMPLE : WRNN_KERNEL_TEAM2;
    if (kernel == WRNN_KERNEL_TEAM2 && team_no) return wrnn_failf(h, WRNN_ERR_INVALID, "%s", team_no);
    if (kernel != WRNN_KERNEL_TEAM2 && kernel != WRNN_KERNEL_SIMPLE)
        return wrnn_failf(h, WRNN_ERR_INVALID, "a stream runs WRNN_KERNEL_AUTO, TEAM2 or SIMPLE (kernel %d)", opts->kernel);
    WRNN_TRY(h, hipSetDevice(h->cfg.device));
    wrnn_stream *st = new wrnn_stream();
    st->h = h; st->device = h->cfg.device; st->B = B; st->kernel = kernel; st->noise_mode = opts->noise_mode; st->seed = opts->seed;
    const int teams = h->n_teams < 1 ? 1 : h->n_teams;
    st->n_slots = (B + teams - 1) / teams * teams;
    hipError_t e = hipMalloc(&st->rows, (size_t)B * sizeof(WrnnRow));
    if (e == hipSuccess) e = hipMalloc(&st->sched, (size_t)st->n_slots * sizeof(int32_t));
    if (e == hipSuccess) e = hipMalloc(&st->err, 64);
    if (e == hipSuccess) e = hipMemset(st->err, 0, 64);
    if (e == hipSuccess) {
        st->state_cap = (size_t)B * state_floats(h);
        e = hipMalloc(&st->state, st->state_cap * sizeof(float));
    }
    if (e != hipSuccess) {
        wrnn_stream_close(st);
        return wrnn_failf(h, WRNN_ERR_HIP, "wrnn_stream_open: %s", hipGetErrorString(e));
    }
    *out = st;
    return WRNN_OK;
}

int wrnn_stream_push(wrnn_stream *st, const float *mels_dev, int32_t n_frames, int32_t last, int32_t *labels_out_dev,
                     float *samples_out_dev, int64_t out_capacity, int64_t *steps_out, void *stream) {
    if (!st) return WRNN_ERR_INVALID;
    wrnn_handle *h = st->h;
    if (steps_out) *steps_out = 0;
    if (st->poisoned) return wrnn_failf(h, WRNN_ERR_STATE, "the stream reported a device-side error (wrnn_stream_sync): it cannot continue");
    if (st->ended) return wrnn_failf(h, WRNN_ERR_STATE, "push after the stream's last push");
    if (n_frames < 0 || (n_frames > 0 && !mels_dev) || !steps_out) return wrnn_failf(h, WRNN_ERR_INVALID, "wrnn_stream_push: bad arguments");
    if (!h->loaded) return wrnn_failf(h, WRNN_ERR_STATE, "weights not loaded");
    const WrnnDims &d = h->d;
    const int B = st->B, F = d.F, P = d.P, HOP = d.HOP;
    const int64_t fin = st->frames_in + n_frames;
    const int64_t ready = wrnn_stream_ready_steps(fin, HOP, P, last);
    const int64_t s0 = st->steps_done, s1 = ready > s0 ? ready : s0;
    const int64_t n = s1 - s0;
    if (n > 0 && (!samples_out_dev || out_capacity < (int64_t)B * n))
        return wrnn_failf(h, WRNN_ERR_INVALID, "wrnn_stream_push: %lld steps are ready, the outputs must hold B * steps = %lld elements (capacity %lld)",
                     (long long)n, (long long)B * n, (long long)out_capacity);
    if (n > INT32_MAX / 2) return wrnn_failf(h, WRNN_ERR_INVALID, "wrnn_stream_push: push too long");
    WRNN_TRY(h, hipSetDevice(h->cfg.device));
    hipStream_t s = (hipStream_t)stream;
    const int hn = (int)(st->frames_in - st->hist0);
    const float *hist = st->hist[st->cur];

    if (n > 0) {
        // window: frames [f0, f1) own the ready steps, their conditioning reads mel frames [f0 - P, f1 + P)
        const int64_t f0 = s0 / HOP, f1 = (s1 + HOP - 1) / HOP;
        const int Tw = (int)(f1 - f0), nW = Tw + 2 * P;
        if (f0 - P >= 0 && f0 - P < st->hist0) return wrnn_failf(h, WRNN_ERR_STATE, "internal: mel history lost frame %lld", (long long)(f0 - P));
        if (int rc = wrnn_grow(h, st->win, st->win_cap, (size_t)B * F * nW)) return rc;
        WRNN_TRY(h, launch_gather(hist, st->hist0, hn, mels_dev, st->frames_in, n_frames, st->win, f0 - P, nW, B, F, fin, s));
        if (int rc = wrnn_grow(h, st->aux, st->aux_cap, (size_t)B * Tw * d.R)) return rc;
        WRNN_TRY(h, wrnn_launch_resnet(h, st->win, B, Tw, nW, P, st->aux, s));
        const int32_t row_steps = st->kernel == WRNN_KERNEL_SIMPLE ? (int32_t)n : INT32_MAX;
        hipLaunchKernelGGL(stream_rows_kernel, dim3((st->n_slots + 255) / 256), dim3(256), 0, s, st->rows, st->sched, B, st->n_slots,
                           row_steps, -f0 * (int64_t)HOP);
        WRNN_TRY(h, hipGetLastError());
        // the loop arguments of the push; TEAM2 takes its sampling fields from them
        WrnnLoopArgs a{};
        a.w = h->wdev; a.off = h->off; a.d = d; a.mels = st->win; a.mel_T = nW; a.mel_off = P; a.aux_frames = st->aux; a.rows = st->rows;
        a.n_rows = B; a.T = Tw; a.total_len = (int64_t)Tw * HOP; a.steps = n;
        a.noise_mode = st->noise_mode; a.seed = st->seed;
        a.labels_out = labels_out_dev ? labels_out_dev - s0 : nullptr; a.samples_out = samples_out_dev - s0; a.err = st->err;
        a.seg0 = s0; a.state = st->state;
        if (st->kernel == WRNN_KERNEL_SIMPLE) {
            WRNN_TRY(h, wrnn_launch_loop_simple(a, s));
        } else {
            // the offline TEAM2 prologue and segment loop (launch.hip) on the window: T = Tw, mels (B, F, Tw + 2P) padded by P
            WrnnFrameTables t;
            if (int rc = wrnn_build_frame_tables(h, st->tab, st->tab_cap, st->win, nW, 0, st->aux, B, Tw, 28, t, s)) return rc;
            WRNN_TRY(h, wrnn_launch_pack_records(t.CM, t.CA, t.VM, t.VA, t.REC, B, Tw, P, nullptr, s));
            // every segment start s0 + k * seg lies on a 32-step boundary because s0 does
            const int64_t seg = wrnn_team2_segment_len(B, d.H, n, 0);
            if (int rc = wrnn_grow(h, st->cond, st->cond_cap, (size_t)B * (size_t)seg * d.H * 4)) return rc;
            WrnnTeamArgs ta{};
            ta.w = a.w; ta.off = a.off; ta.d = d; ta.team_w = h->team_w; ta.team_fc3 = h->team_fc3; ta.wI0 = h->wI0; ta.u1 = h->u1;
            ta.tabREC = t.REC; ta.tabC2 = t.C2; ta.tabC3 = t.C3; ta.tabC4 = t.C4;
            // B == 1: the uniform instantiation offline calls run, its outputs at [t] whatever a.steps is (a.steps past every step:
            // the state is always handed on); B > 1: the ragged one, whose rows end at rows[r].steps (never) and write at [r * n + t]
            ta.rows = st->rows; ta.sched = st->sched; ta.n_slots = st->n_slots; ta.ragged = B > 1; ta.n_rows = B; ta.n_teams = h->n_teams;
            ta.T = Tw; ta.total_len = a.total_len; ta.steps = B > 1 ? n : (int64_t)1 << 62;
            ta.state = st->state;
            wrnn_copy_sampling(ta, a);
            ta.mail = h->mail; ta.ctl = h->ctl; ta.err = st->err; ta.prof = nullptr;
            if (int rc = wrnn_run_team2_segments(h, ta, st->cond, s0, s1, seg, nullptr, s)) return rc;
        }
    }
    // mel history for the next push: frames [keep0, fin), keep0 = the first frame the next window can reach
    if (!last) {
        int64_t keep0 = s1 / HOP - P;
        if (keep0 < 0) keep0 = 0;
        if (keep0 > fin) keep0 = fin;
        const int nk = (int)(fin - keep0);
        const int nxt = 1 - st->cur;
        if (int rc = wrnn_grow(h, st->hist[nxt], st->hist_cap[nxt], (size_t)B * F * (nk > 0 ? nk : 1))) return rc;
        WRNN_TRY(h, launch_gather(hist, st->hist0, hn, mels_dev, st->frames_in, n_frames, st->hist[nxt], keep0, nk, B, F, fin, s));
        st->cur = nxt;
        st->hist0 = keep0;
    }
    st->frames_in = fin;
    st->steps_done = s1;
    st->ended = last != 0;
    *steps_out = n;
    return WRNN_OK;
}

int wrnn_stream_sync(wrnn_stream *st, void *stream) {
    if (!st) return WRNN_ERR_INVALID;
    wrnn_handle *h = st->h;
    WRNN_TRY(h, hipSetDevice(h->cfg.device));
    WRNN_TRY(h, hipStreamSynchronize((hipStream_t)stream));
    unsigned errw = 0;
    WRNN_TRY(h, hipMemcpy(&errw, st->err, sizeof(errw), hipMemcpyDeviceToHost));
    if (!errw) return WRNN_OK;
    st->poisoned = true;
    if (errw == WRNN_DEVERR_BUSY)
        return wrnn_failf(h, WRNN_ERR_BUSY, "the stream's team kernel could not get its workgroups resident (the GPU is shared with another kernel): "
                                       "the stream cannot continue; open a new one (WRNN_KERNEL_SIMPLE runs anywhere)");
    return wrnn_failf(h, WRNN_ERR_TIMEOUT, "device-side bounded spin gave up in a stream push (code %u)", errw);
}

int wrnn_stream_info(const wrnn_stream *st, int64_t *frames_in, int64_t *steps_done, int64_t *workspace_bytes) {
    if (!st) return WRNN_ERR_INVALID;
    if (frames_in) *frames_in = st->frames_in;
    if (steps_done) *steps_done = st->steps_done;
    if (workspace_bytes)
        *workspace_bytes = (int64_t)((st->hist_cap[0] + st->hist_cap[1] + st->win_cap + st->aux_cap + st->tab_cap + st->cond_cap + st->state_cap) *
                                     sizeof(float)) + (int64_t)(st->B * sizeof(WrnnRow) + st->n_slots * sizeof(int32_t) + 64);
    return WRNN_OK;
}

void wrnn_stream_close(wrnn_stream *st) {
    if (!st) return;
    (void)hipSetDevice(st->device);
    (void)hipDeviceSynchronize();
    for (float *p : {st->hist[0], st->hist[1], st->win, st->aux, st->tab, st->cond, st->state})
        if (p) (void)hipFree(p);
    if (st->rows) (void)hipFree(st->rows);
    if (st->sched) (void)hipFree(st->sched);
    if (st->err) (void)hipFree(st->err);
    delete st;
}

}  // extern "C"
