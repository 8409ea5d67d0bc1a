// Host launch path of the XCD-team loop kernels (declared in wrnn_internal.h): what an offline call (api.hip) and a stream's push
// (stream.hip) do alike between the resnet and the loop.  No kernels here.
#include <cstdarg>
#include <cstdio>

#include "team_common.h"

int wrnn_failf(wrnn_handle *h, int code, const char *fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    if (h) h->err = buf;
    return code;
}

int wrnn_build_frame_tables(wrnn_handle *h, float *&buf, size_t &cap, const float *mels, int mel_T, int mel_shift, const float *aux, int B,
                            int T, int rec_floats, WrnnFrameTables &t, hipStream_t s) {
    const WrnnDims &d = h->d;
    const int H = d.H, FC = d.FC, F = d.F, A = d.A, R = d.R, P = d.P;
    const int TP = T + 2 * P, T1 = T + 1;
    const size_t nCM = (size_t)B * TP * H, nCA = (size_t)B * T1 * H, nVM = (size_t)B * TP * 3 * H, nVA = (size_t)B * T1 * 3 * H;
    const size_t nC2 = (size_t)B * T1 * 3 * H, nC3 = (size_t)B * T1 * FC, nC4 = (size_t)B * T1 * FC, nREC = (size_t)B * T1 * H * rec_floats;
    if (int rc = wrnn_grow(h, buf, cap, nCM + nCA + nVM + nVA + nC2 + nC3 + nC4 + nREC)) return rc;
    t.CM = buf; t.CA = t.CM + nCM; t.VM = t.CA + nCA; t.VA = t.VM + nVM; t.C2 = t.VA + nVA; t.C3 = t.C2 + nC2; t.C4 = t.C3 + nC3; t.REC = t.C4 + nC4;
    const float *w = h->wdev;
    const WrnnPacked &o = h->off;
    WRNN_TRY(h, wrnn_launch_frame_linear(1, mels, (size_t)F * mel_T, 0, 0, w + o.I_t + (size_t)1 * H, H, nullptr, t.CM, (size_t)TP * H, TP, F, H, B, mel_T, mel_shift, s));
    WRNN_TRY(h, wrnn_launch_frame_linear(0, aux, (size_t)T * R, R, T, w + o.I_t + (size_t)(1 + F) * H, H, w + o.I_b, t.CA, (size_t)T1 * H, T1, A, H, B, T, P, s));
    WRNN_TRY(h, wrnn_launch_frame_linear(0, t.CM, (size_t)TP * H, H, TP, w + o.r1_wih_t, 3 * H, nullptr, t.VM, (size_t)TP * 3 * H, TP, H, 3 * H, B, T, P, s));
    WRNN_TRY(h, wrnn_launch_frame_linear(0, t.CA, (size_t)T1 * H, H, T1, w + o.r1_wih_t, 3 * H, w + o.r1_bih, t.VA, (size_t)T1 * 3 * H, T1, H, 3 * H, B, T, P, s));
    WRNN_TRY(h, wrnn_launch_frame_linear(0, aux + A, (size_t)T * R, R, T, w + o.r2_wih_t + (size_t)H * 3 * H, 3 * H, w + o.r2_bih, t.C2, (size_t)T1 * 3 * H, T1, A, 3 * H, B, T, P, s));
    WRNN_TRY(h, wrnn_launch_frame_linear(0, aux + 2 * A, (size_t)T * R, R, T, w + o.fc1_t + (size_t)H * FC, FC, w + o.fc1_b, t.C3, (size_t)T1 * FC, T1, A, FC, B, T, P, s));
    WRNN_TRY(h, wrnn_launch_frame_linear(0, aux + 3 * A, (size_t)T * R, R, T, w + o.fc2_t + (size_t)FC * FC, FC, w + o.fc2_b, t.C4, (size_t)T1 * FC, T1, A, FC, B, T, P, s));
    return WRNN_OK;
}

// The phase-A conditioning is streamed from HBM (8 KB per row and step).  A row is generated in segments, one stream chunk + one
// loop launch each, sized so that the chunk (~64 MB over all rows) is still resident in the memory-side cache when the loop reads
// it: against a stream written once for the whole clip (903 MB for 5 s of audio, read back from DRAM) this is 6.5 % faster at
// B=1, bounds the scratch to rows x seg x 8 KB, and costs one relaunch (~40 us) per segment.  Segment lengths are multiples of 32
// steps (the shadow waves regenerate their Philox state on those boundaries).
int64_t wrnn_team2_segment_len(int rows, int H, int64_t steps, int seg_override) {
    int64_t seg = ((int64_t)(64u << 20) / ((int64_t)rows * H * 4 * (int64_t)sizeof(float))) & ~(int64_t)31;
    if (seg > 16384) seg = 16384;
    if (seg < 2048) seg = 2048;
    if (seg_override > 0) { seg = (int64_t)seg_override & ~(int64_t)31; if (seg < 32) seg = 32; }
    return seg > steps ? steps : seg;
}

int wrnn_run_team2_segments(wrnn_handle *h, WrnnTeamArgs &ta, float *cond, int64_t t_begin, int64_t t_end, int64_t seg, int *launches,
                            hipStream_t s) {
    ta.tabCOND = cond;
    int n = 0;
    for (int64_t t0 = t_begin; t0 < t_end; t0 += seg, ++n) {
        const int64_t len = t_end - t0 < seg ? t_end - t0 : seg;
        WRNN_TRY(h, wrnn_launch_cond_stream(ta.tabREC, ta.w + ta.off.ktab, ta.rows, cond, ta.n_rows, ta.T, ta.d.HOP, ta.total_len, t0, len, s));
        ta.seg0 = t0; ta.seg_len = len;
        WRNN_TRY(h, wrnn_gated_launch(h->cfg.device, s, h->mail, WRNN_MAIL_BYTES, h->ctl, TEAM_CTL_WORDS * sizeof(unsigned), [&] { return wrnn_launch_loop_team2(ta, s); }));
    }
    if (launches) *launches = n;
    return WRNN_OK;
}
