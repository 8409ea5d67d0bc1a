// C-ABI entry points of libwavernn_amd.so (see include/wavernn_amd.h).
// Host-side work here is limited to: validating the configuration, repacking
// the reference state_dict into the device layouts the kernels want, and
// enqueueing kernels on the caller's stream.
#include <climits>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <map>
#include <mutex>

#include "mel_internal.h"
#include "resample_internal.h"
#include "team_common.h"

namespace {

// Composite taps of the stretch+conv chain (UpsampleNetwork, fatchord_version.py:73-88),
// computed in fp64 by pushing one impulse frame through the exact chain.
std::vector<float> build_ktab(const WrnnDims &d, const int *scales, int n_up, const std::vector<std::vector<double>> &taps) {
    const int P = d.P, HOP = d.HOP, ND = d.ND;
    const int f0 = P + 2, TS = 2 * P + 5;
    std::vector<double> a(TS, 0.0), c;
    a[f0] = 1.0;
    for (int li = 0; li < n_up; ++li) {
        const int s = scales[li], K = 2 * s + 1;
        const size_t n2 = a.size() * (size_t)s;
        c.assign(n2, 0.0);
        for (size_t i = 0; i < a.size(); ++i)
            for (int r = 0; r < s; ++r) c[i * s + r] = a[i];
        a.assign(n2, 0.0);
        for (size_t i = 0; i < n2; ++i) {
            double acc = 0.0;
            for (int k = 0; k < K; ++k) {
                const long jx = (long)i + k - s;
                if (jx >= 0 && (size_t)jx < n2) acc += taps[li][k] * c[jx];
            }
            a[i] = acc;
        }
    }
    std::vector<float> kt((size_t)HOP * ND);
    for (int r = 0; r < HOP; ++r)
        for (int dd = 0; dd < ND; ++dd) kt[(size_t)r * ND + dd] = (float)a[(size_t)HOP * (P + f0 - dd) + r];
    return kt;
}

struct TensorView {
    const wrnn_tensor_desc *t;
    int64_t numel() const {
        int64_t n = 1;
        for (int i = 0; i < t->ndim; ++i) n *= t->shape[i];
        return n;
    }
    const float *f() const { return (const float *)t->data; }
};

// Per-device ordering of team-kernel launches (wrnn_internal.h).  One slot per HIP device ordinal: the launch lock and an
// event recorded behind the last team kernel; the next launch (any handle, any stream) waits on that event on the device.
struct TeamGate {
    std::mutex mu;
    hipEvent_t tail = nullptr;
    bool recorded = false;
};
TeamGate g_team_gate[64];

// What keeps the generate loop off the XCD-team kernels for this handle (nullptr: nothing): the co-residency check of wrnn_create, the
// 5-frame upsampling support the team kernels are built for (pad = 2, hop <= 275), or the test hook.
const char *loop_team_obstacle(const wrnn_handle *h) {
    if (h->force_no_teams) return "team kernels disabled by wrnn_debug_force_no_teams (test hook)";
    if (!h->team_ok) return h->team_why.c_str();
    if (h->d.ND != 5 || h->d.HOP > 275) return "team kernels are built for pad=2 (5-frame upsampling support), hop <= 275";
    return nullptr;
}

}  // namespace

const char *wrnn_loop_team_obstacle(const wrnn_handle *h) { return loop_team_obstacle(h); }

hipError_t wrnn_team_gate_enter(int device, hipStream_t s) {
    TeamGate &g = g_team_gate[(unsigned)device % 64u];
    g.mu.lock();
    hipError_t e = hipSuccess;
    if (!g.tail) e = hipEventCreateWithFlags(&g.tail, hipEventDisableTiming);
    if (e == hipSuccess && g.recorded) e = hipStreamWaitEvent(s, g.tail, 0);
    if (e != hipSuccess) g.mu.unlock();
    return e;
}
hipError_t wrnn_team_gate_leave(int device, hipStream_t s) {
    TeamGate &g = g_team_gate[(unsigned)device % 64u];
    hipError_t e = g.tail ? hipEventRecord(g.tail, s) : hipSuccess;
    if (e == hipSuccess) g.recorded = true;
    g.mu.unlock();
    return e;
}

const char *wrnn_dims_from_config(const wrnn_config *cfg, WrnnDims &d) {
    d = WrnnDims{};
    d.H = cfg->rnn_dims; d.FC = cfg->fc_dims; d.F = cfg->feat_dims; d.C = cfg->compute_dims;
    d.R = cfg->res_out_dims; d.A = cfg->res_out_dims / 4; d.NBLK = cfg->res_blocks; d.P = cfg->pad;
    d.KS = 2 * cfg->pad + 1; d.ND = d.KS; d.mode = cfg->mode; d.HOP = cfg->hop_length;
    if (cfg->mode == WRNN_MODE_RAW) d.NC = 1 << cfg->bits;       // fatchord_version.py:98-99
    else if (cfg->mode == WRNN_MODE_MOL) d.NC = 30;             // :100-101
    else return "mode must be WRNN_MODE_RAW or WRNN_MODE_MOL";
    if (d.H < 1 || d.FC < 1 || d.F < 1 || d.C < 1 || d.R < 4 || d.NBLK < 0 || d.P < 0 || cfg->bits < 1 || cfg->bits > 16) return "bad dims";
    if (cfg->res_out_dims % 4 != 0) return "res_out_dims must be a multiple of 4 (aux split, :109)";
    if (d.H > 1024 || d.C > 1024 || d.R > 1024) return "unsupported dims: rnn_dims, compute_dims, res_out_dims up to 1024";
    return nullptr;
}

extern "C" {

int32_t wrnn_abi_version(void) { return WRNN_ABI_VERSION; }

int wrnn_create(const wrnn_config *cfg, wrnn_handle **out) {
    if (!cfg || !out) return WRNN_ERR_INVALID;
    *out = nullptr;
    wrnn_handle *h = new wrnn_handle();
    h->cfg = *cfg;
    WrnnDims &d = h->d;
    int hop = 1, reach = 0;
    if (cfg->n_upsample < 1 || cfg->n_upsample > WRNN_MAX_UP) { delete h; return WRNN_ERR_INVALID; }
    for (int i = 0; i < cfg->n_upsample; ++i) hop *= cfg->upsample_factors[i];
    {
        int later = hop;
        for (int i = 0; i < cfg->n_upsample; ++i) { later /= cfg->upsample_factors[i]; reach += cfg->upsample_factors[i] * later; }
    }
    if (cfg->mode != WRNN_MODE_RAW && cfg->mode != WRNN_MODE_MOL) { delete h; return WRNN_ERR_INVALID; }
    *out = h;  // from here on errors are reported through the handle
    // Any constructor dims (fatchord_version.py:93-129) run on the SIMPLE kernel as long as its activation vectors fit a
    // CU's LDS; the team kernels (TEAM2, BATCH) are built for the reference hparams (wavernn_hparams.py:18-57).
    if (const char *why = wrnn_dims_from_config(cfg, d)) return wrnn_failf(h, WRNN_ERR_INVALID, "%s", why);
    h->team_dims = d.H == 512 && d.FC == 512 && d.F == 80 && d.R == 128 && d.C == 128 && d.A == 32;
    if (hop != cfg->hop_length) return wrnn_failf(h, WRNN_ERR_INVALID, "prod(upsample_factors)=%d != hop_length=%d", hop, cfg->hop_length);
    if (reach > cfg->pad * hop || d.ND > WRNN_KTAB_MAXD)
        return wrnn_failf(h, WRNN_ERR_INVALID, "upsample edge reach %d exceeds indent %d: composite FIR not shift-invariant", reach, cfg->pad * hop);
    if (wrnn_simple_lds_bytes(d) > 160u * 1024u || ((size_t)(8 + d.KS - 1) * d.F + 16u * d.C) * sizeof(float) > 160u * 1024u)
        return wrnn_failf(h, WRNN_ERR_INVALID, "dims too large: the activation vectors of one row (%zu bytes) must fit 160 KB of LDS", wrnn_simple_lds_bytes(d));
    WRNN_TRY(h, hipSetDevice(cfg->device));
    {
        // team kernels: one team per XCD = 32 CUs (SPX: 256 CUs = 8 teams; a CPX/DPX partition exposes fewer)
        hipDeviceProp_t prop;
        WRNN_TRY(h, hipGetDeviceProperties(&prop, cfg->device));
        h->n_teams = prop.multiProcessorCount / 32;
        if (h->n_teams > 8) h->n_teams = 8;
    }
    {
        // The team kernels spin on each other inside one launch: all n_teams * 32 workgroups must be resident at once,
        // one per CU (they take most of a CU's LDS).  Establish that here, loudly, instead of discovering it as a
        // bounded-spin timeout: the runtime must admit >= 1 workgroup per CU for every team kernel.
        h->team_ok = true;
        if (!h->team_dims || d.NC > 1024) { h->team_ok = false; h->team_why = "the team kernels are built for rnn=fc=512, feat=80, compute=res_out=128, n_classes <= 1024"; }
        else if (h->n_teams < 1) { h->team_ok = false; h->team_why = "fewer than 32 CUs visible (one team = the 32 CUs of an XCD)"; }
        // the instantiations THIS handle launches (its mode; the instrumented builds are checked by wrnn_phase_profile)
        int blocks = 0;
        size_t lds = 0;
        if (h->team_ok) {
            hipError_t e = wrnn_team2_occupancy(cfg->mode, false, &blocks, &lds);
            if (e != hipSuccess || blocks < 1) { h->team_ok = false; h->team_why = "loop_team2_kernel cannot be resident (LDS/registers)"; }
        }
        for (int nq = 1; nq <= 2 && h->team_ok; ++nq) {
            hipError_t e = wrnn_batch_occupancy(cfg->mode, nq, false, &blocks, &lds);
            if (e != hipSuccess || blocks < 1) { h->team_ok = false; h->team_why = "loop_batch_kernel cannot be resident (LDS/registers)"; }
        }
        // its own flag (round-4 advisor): a toolchain that allocates this kernel's registers differently must not take TEAM2 and BATCH down with
        // it -- AUTO then runs the one-wave-per-SIMD batch kernel, only an explicit WRNN_KERNEL_BATCH_CS is an error
        h->cs_ok = h->team_ok;
        for (int nq = 1; nq <= wrnn_batch_cs_max_nq(cfg->mode) && h->cs_ok; ++nq) {
            hipError_t e = wrnn_batch_cs_occupancy(cfg->mode, nq, false, &blocks, &lds);
            if (e != hipSuccess || blocks < 1) h->cs_ok = false;
        }
        (void)hipGetLastError();
    }
    for (int i = 0; i < 3; ++i) WRNN_TRY(h, hipEventCreate(&h->ev[i]));
    WRNN_TRY(h, hipMalloc(&h->err_dev, 64));
    WRNN_TRY(h, hipMemset(h->err_dev, 0, 64));
    return WRNN_OK;
}

void wrnn_destroy(wrnn_handle *h) {
    if (!h) return;
    (void)hipSetDevice(h->cfg.device);
    if (h->wdev) (void)hipFree(h->wdev);
    if (h->aux_frames) (void)hipFree(h->aux_frames);
    if (h->rows_dev) (void)hipFree(h->rows_dev);
    if (h->order_dev) (void)hipFree(h->order_dev);
    if (h->sched_dev) (void)hipFree(h->sched_dev);
    if (h->keys_dev) (void)hipFree(h->keys_dev);
    if (h->fold0_dev) (void)hipFree(h->fold0_dev);
    if (h->prof) (void)hipFree(h->prof);
    if (h->err_dev) (void)hipFree(h->err_dev);
    if (h->team_w) (void)hipFree(h->team_w);
    if (h->team_fc3) (void)hipFree(h->team_fc3);
    if (h->teamg_img) (void)hipFree(h->teamg_img);
    if (h->teamg_sp_flags) (void)hipFree(h->teamg_sp_flags);
    if (h->batch_w) (void)hipFree(h->batch_w);
    if (h->batch_fc3) (void)hipFree(h->batch_fc3);
    if (h->batch_wn) (void)hipFree(h->batch_wn);
    if (h->wI0) (void)hipFree(h->wI0);
    if (h->u1) (void)hipFree(h->u1);
    if (h->tab) (void)hipFree(h->tab);
    if (h->cond) (void)hipFree(h->cond);
    if (h->team_state) (void)hipFree(h->team_state);
    if (h->epi_tab) (void)hipFree(h->epi_tab);
    if (h->loss_partial) (void)hipFree(h->loss_partial);
    if (h->train) wrnn_train_state_free(h->train);
    if (h->mail) (void)hipFree(h->mail);
    if (h->ctl) (void)hipFree(h->ctl);
    for (int i = 0; i < 3; ++i)
        if (h->ev[i]) (void)hipEventDestroy(h->ev[i]);
    delete h;
}

const char *wrnn_last_error(const wrnn_handle *h) { return wrnn_last_error_of(h); }

int32_t wrnn_team_info(const wrnn_handle *h, int32_t *n_teams_out, const char **why_not_out) {
    if (!h) return 0;
    const char *no = loop_team_obstacle(h);
    if (n_teams_out) *n_teams_out = h->n_teams;
    if (why_not_out) *why_not_out = no ? no : "";
    return no ? 0 : 1;
}

int wrnn_debug_force_no_teams(wrnn_handle *h, int32_t on) {
    if (!h) return WRNN_ERR_INVALID;
    h->force_no_teams = on != 0;
    return WRNN_OK;
}
int32_t wrnn_last_batch_rows(const wrnn_handle *h) { return h ? h->last_batch_rows : 1; }

int wrnn_debug_teamg_lds_budget(wrnn_handle *h, int64_t bytes) {
    if (!h) return WRNN_ERR_INVALID;
    h->teamg_budget = bytes < 0 ? -1 : bytes;
    return WRNN_OK;
}
int wrnn_teamg_set_weight_format(wrnn_handle *h, int32_t fmt) {
    if (!h) return WRNN_ERR_INVALID;
    if (fmt != WRNN_WEIGHTS_F32 && fmt != WRNN_WEIGHTS_F16 && fmt != WRNN_WEIGHTS_E4M3)   // 2 is reserved
        return wrnn_failf(h, WRNN_ERR_INVALID, "wrnn_teamg_set_weight_format: %d is none of WRNN_WEIGHTS_F32, WRNN_WEIGHTS_F16, WRNN_WEIGHTS_E4M3", fmt);
    if (fmt != h->teamg_fmt) { h->teamg_img_ok = false; h->teamg_sp_ok = false; }   // the next TEAMG / TEAMG_BATCH call packs the image in the new element type
    h->teamg_fmt = fmt;
    return WRNN_OK;
}
int32_t wrnn_teamg_weight_format(const wrnn_handle *h) { return h ? h->teamg_fmt : WRNN_WEIGHTS_F32; }
int wrnn_teamg_weight_scales(const wrnn_handle *h, float out[6]) {
    if (!h || !out) return WRNN_ERR_INVALID;
    for (int l = 0; l < WRNN_TEAMG_LAYERS; ++l) out[l] = h->teamg_scale[l];
    return WRNN_OK;
}
int wrnn_teamg_set_sparse(wrnn_handle *h, int32_t on) {
    if (!h) return WRNN_ERR_INVALID;
    if ((on != 0) != h->teamg_sparse) { h->teamg_img_ok = false; h->teamg_sp_ok = false; }   // the next TEAMG / TEAMG_BATCH call packs the other image
    h->teamg_sparse = on != 0;
    return WRNN_OK;
}
int32_t wrnn_teamg_sparse(const wrnn_handle *h) { return h && h->teamg_sparse ? 1 : 0; }
int wrnn_teamg_sparse_info(wrnn_handle *h, int64_t kept[6], int64_t dense[6], int32_t nb_a[6], int32_t nb_b[6], wrnn_teamg_plan_info *plan) {
    if (!h) return WRNN_ERR_INVALID;
    if (!h->teamg_sp_ok || !h->teamg_img_ok)
        return wrnn_failf(h, WRNN_ERR_STATE, "wrnn_teamg_sparse_info: no block-sparse image is packed (wrnn_teamg_set_sparse(h, 1), then a TEAMG / TEAMG_BATCH call)");
    for (int l = 0; l < WRNN_TEAMG_LAYERS; ++l) {
        if (kept) kept[l] = h->teamg_sp_kept[l];
        if (dense) dense[l] = h->teamg_sp_dense[l];
        if (nb_a) nb_a[l] = h->teamg_nb_a[l];
        if (nb_b) nb_b[l] = h->teamg_nb_b[l];
    }
    if (plan) return wrnn_teamg_plan_info_impl(&h->cfg, h->teamg_sp_rows, WRNN_WEIGHTS_F32, h->teamg_sp_budget, plan, h->teamg_nb_a, h->teamg_nb_b);
    return WRNN_OK;
}
int32_t wrnn_n_classes(const wrnn_handle *h) { return h ? h->d.NC : 0; }
int64_t wrnn_loop_weight_bytes(const wrnn_handle *h) { return h ? h->loop_weight_bytes : 0; }

int wrnn_load_weights(wrnn_handle *h, const wrnn_tensor_desc *tensors, int32_t n) {
    if (!h || !tensors) return WRNN_ERR_INVALID;
    const WrnnDims &d = h->d;
    std::map<std::string, TensorView> tv;
    for (int i = 0; i < n; ++i)
        if (tensors[i].name && tensors[i].data) tv[tensors[i].name] = TensorView{&tensors[i]};
    auto need = [&](const std::string &name, std::initializer_list<int64_t> shape, const float **out) -> int {
        auto it = tv.find(name);
        if (it == tv.end()) return wrnn_failf(h, WRNN_ERR_MISSING_KEY, "state_dict key missing: %s", name.c_str());
        const wrnn_tensor_desc *t = it->second.t;
        if (t->dtype != WRNN_DTYPE_F32) return wrnn_failf(h, WRNN_ERR_INVALID, "%s: expected float32", name.c_str());
        if ((size_t)t->ndim != shape.size()) return wrnn_failf(h, WRNN_ERR_INVALID, "%s: expected %d dimensions, got %d", name.c_str(), (int)shape.size(), (int)t->ndim);
        int di = 0;
        for (auto s : shape) {
            if (t->shape[di] != s) return wrnn_failf(h, WRNN_ERR_INVALID, "%s: dimension %d is %lld, expected %lld", name.c_str(), di, (long long)t->shape[di], (long long)s);
            ++di;
        }
        *out = it->second.f();
        return WRNN_OK;
    };
    const int H = d.H, FC = d.FC, F = d.F, A = d.A, C = d.C, R = d.R, KS = d.KS, NC = d.NC, NB = d.NBLK;
    const int IN_I = 1 + F + A;
#define NEED(name, out, ...) do { int rc__ = need(name, {__VA_ARGS__}, &out); if (rc__) return rc__; } while (0)

    // ---- layout ------------------------------------------------------------
    WrnnPacked &o = h->off;
    size_t cur = 0;
    auto take = [&](size_t nfl) { size_t at = cur; cur += (nfl + 63) & ~(size_t)63; return at; };  // 256-B aligned blocks
    o.conv_in_t = take((size_t)F * KS * C); o.conv_in_b = take(C);
    o.res_w1_t = take((size_t)NB * C * C); o.res_b1 = take((size_t)NB * C);
    o.res_w2_t = take((size_t)NB * C * C); o.res_b2 = take((size_t)NB * C);
    o.conv_out_t = take((size_t)C * R); o.conv_out_b = take(R);
    o.ktab = take((size_t)d.HOP * d.ND);
    o.I_t = take((size_t)IN_I * H); o.I_b = take(H);
    o.r1_wih_t = take((size_t)H * 3 * H); o.r1_whh_t = take((size_t)H * 3 * H);
    o.r1_bih = take(3 * H); o.r1_bhh = take(3 * H);
    o.r2_wih_t = take((size_t)(H + A) * 3 * H); o.r2_whh_t = take((size_t)H * 3 * H);
    o.r2_bih = take(3 * H); o.r2_bhh = take(3 * H);
    o.fc1_t = take((size_t)(H + A) * FC); o.fc1_b = take(FC);
    o.fc2_t = take((size_t)(FC + A) * FC); o.fc2_b = take(FC);
    o.fc3_t = take((size_t)FC * NC); o.fc3_b = take(NC);
    o.total = cur;
    std::vector<float> pk(o.total, 0.0f);

    // ---- prologue: fold BatchNorm1d(eval, eps=1e-5) into the preceding conv ---
    auto bn_fold = [&](const std::string &prefix, std::vector<double> &scale, std::vector<double> &shift) -> int {
        const float *g, *b, *m, *v;
        NEED(prefix + ".weight", g, C); NEED(prefix + ".bias", b, C);
        NEED(prefix + ".running_mean", m, C); NEED(prefix + ".running_var", v, C);
        scale.resize(C); shift.resize(C);
        for (int c = 0; c < C; ++c) {
            const double inv = 1.0 / std::sqrt((double)v[c] + 1e-5);
            scale[c] = (double)g[c] * inv;
            shift[c] = (double)b[c] - (double)m[c] * scale[c];
        }
        return WRNN_OK;
    };
    std::vector<double> sc, sh;
    {
        const float *wci;
        NEED("upsample.resnet.conv_in.weight", wci, C, F, KS);
        if (int rc = bn_fold("upsample.resnet.batch_norm", sc, sh)) return rc;
        for (int c = 0; c < C; ++c) {
            for (int f = 0; f < F; ++f)
                for (int k = 0; k < KS; ++k)
                    pk[o.conv_in_t + (size_t)(f * KS + k) * C + c] = (float)((double)wci[((size_t)c * F + f) * KS + k] * sc[c]);
            pk[o.conv_in_b + c] = (float)sh[c];
        }
    }
    for (int l = 0; l < NB; ++l) {
        const std::string p = "upsample.resnet.layers." + std::to_string(l);
        const float *w1, *w2;
        NEED(p + ".conv1.weight", w1, C, C, 1); NEED(p + ".conv2.weight", w2, C, C, 1);
        if (int rc = bn_fold(p + ".batch_norm1", sc, sh)) return rc;
        for (int co = 0; co < C; ++co) {
            for (int ci = 0; ci < C; ++ci) pk[o.res_w1_t + ((size_t)l * C + ci) * C + co] = (float)((double)w1[(size_t)co * C + ci] * sc[co]);
            pk[o.res_b1 + (size_t)l * C + co] = (float)sh[co];
        }
        if (int rc = bn_fold(p + ".batch_norm2", sc, sh)) return rc;
        for (int co = 0; co < C; ++co) {
            for (int ci = 0; ci < C; ++ci) pk[o.res_w2_t + ((size_t)l * C + ci) * C + co] = (float)((double)w2[(size_t)co * C + ci] * sc[co]);
            pk[o.res_b2 + (size_t)l * C + co] = (float)sh[co];
        }
    }
    {
        const float *wo, *bo;
        NEED("upsample.resnet.conv_out.weight", wo, R, C, 1); NEED("upsample.resnet.conv_out.bias", bo, R);
        for (int r = 0; r < R; ++r) {
            for (int c = 0; c < C; ++c) pk[o.conv_out_t + (size_t)c * R + r] = wo[(size_t)r * C + c];
            pk[o.conv_out_b + r] = bo[r];
        }
    }
    {
        std::vector<std::vector<double>> taps(h->cfg.n_upsample);
        for (int li = 0; li < h->cfg.n_upsample; ++li) {
            const int s = h->cfg.upsample_factors[li];
            const float *tw;
            NEED("upsample.up_layers." + std::to_string(2 * li + 1) + ".weight", tw, 1, 1, 1, 2 * s + 1);
            taps[li].assign(tw, tw + 2 * s + 1);
        }
        std::vector<float> kt = build_ktab(d, h->cfg.upsample_factors, h->cfg.n_upsample, taps);
        std::memcpy(&pk[o.ktab], kt.data(), kt.size() * sizeof(float));
    }
    // ---- loop parameters: transpose to [in][out] ---------------------------------
    auto put_t = [&](const std::string &name, size_t at, int rows, int cols) -> int {
        const float *src;
        NEED(name, src, rows, cols);
        for (int r = 0; r < rows; ++r)
            for (int c = 0; c < cols; ++c) pk[at + (size_t)c * rows + r] = src[(size_t)r * cols + c];
        return WRNN_OK;
    };
    auto put_v = [&](const std::string &name, size_t at, int nel) -> int {
        const float *src;
        NEED(name, src, nel);
        std::memcpy(&pk[at], src, (size_t)nel * sizeof(float));
        return WRNN_OK;
    };
    int rc;
    if ((rc = put_t("I.weight", o.I_t, H, IN_I)) || (rc = put_v("I.bias", o.I_b, H)) ||
        (rc = put_t("rnn1.weight_ih_l0", o.r1_wih_t, 3 * H, H)) || (rc = put_t("rnn1.weight_hh_l0", o.r1_whh_t, 3 * H, H)) ||
        (rc = put_v("rnn1.bias_ih_l0", o.r1_bih, 3 * H)) || (rc = put_v("rnn1.bias_hh_l0", o.r1_bhh, 3 * H)) ||
        (rc = put_t("rnn2.weight_ih_l0", o.r2_wih_t, 3 * H, H + A)) || (rc = put_t("rnn2.weight_hh_l0", o.r2_whh_t, 3 * H, H)) ||
        (rc = put_v("rnn2.bias_ih_l0", o.r2_bih, 3 * H)) || (rc = put_v("rnn2.bias_hh_l0", o.r2_bhh, 3 * H)) ||
        (rc = put_t("fc1.weight", o.fc1_t, FC, H + A)) || (rc = put_v("fc1.bias", o.fc1_b, FC)) ||
        (rc = put_t("fc2.weight", o.fc2_t, FC, FC + A)) || (rc = put_v("fc2.bias", o.fc2_b, FC)) ||
        (rc = put_t("fc3.weight", o.fc3_t, NC, FC)) || (rc = put_v("fc3.bias", o.fc3_b, NC)))
        return rc;
#undef NEED
    // hot-loop parameter bytes as the reference counts them: weights + biases, fp32
    h->loop_weight_bytes = 4LL * ((int64_t)H * IN_I + H + 2LL * 3 * H * H + 2LL * 3 * H + 3LL * H * (H + A) + 3LL * H * H + 2LL * 3 * H +
                                  (int64_t)FC * (H + A) + FC + (int64_t)FC * (FC + A) + FC + (int64_t)NC * FC + NC);
    if (h->team_dims && NC <= 1024) {
    // ---- team kernel layouts (loop_team2.hip): register-resident slices per (WG g, thread) -----
    // thread tid = wave*64 + r4*16 + q of WG g owns unit u = 16g + 4*wave + r4, columns 32q..32q+31
    const int TT = WRNN_TEAM_THREADS;
    std::vector<float> tw((size_t)32 * WRNN_TEAM_NWREG * TT), tf3((size_t)32 * 16384, 0.0f), vwI0(H), vu1(3 * H);
    {
        const float *whh1 = tv["rnn1.weight_hh_l0"].f(), *wih2 = tv["rnn2.weight_ih_l0"].f(), *whh2 = tv["rnn2.weight_hh_l0"].f();
        const float *wfc1 = tv["fc1.weight"].f(), *wfc2 = tv["fc2.weight"].f(), *wfc3 = tv["fc3.weight"].f();
        const float *wI = tv["I.weight"].f(), *wih1 = tv["rnn1.weight_ih_l0"].f();
        for (int g = 0; g < 32; ++g)
            for (int tid = 0; tid < TT; ++tid) {
                const int wave = tid >> 6, lane = tid & 63, r4 = lane >> 4, q = lane & 15;
                const int u = 16 * g + 4 * wave + r4;
                auto at = [&](int i) -> float & { return tw[((size_t)g * WRNN_TEAM_NWREG + i) * TT + tid]; };
                for (int gate = 0; gate < 3; ++gate)
                    for (int c = 0; c < 32; ++c) {
                        const int row = gate * H + u, col = 32 * q + c;
                        at(gate * 32 + c) = whh1[(size_t)row * H + col];
                        at(96 + gate * 32 + c) = wih2[(size_t)row * (H + A) + col];
                        at(192 + gate * 32 + c) = whh2[(size_t)row * H + col];
                    }
                for (int c = 0; c < 32; ++c) {
                    at(288 + c) = wfc2[(size_t)u * (FC + A) + 32 * q + c];
                    at(320 + c) = wfc1[(size_t)u * (H + A) + 32 * q + c];
                }
                // fc3 LDS image: [(wave*2 + rs)*8 + k][lane][e] <- W3[32g + 8 wave + 2 r4 + rs][32q + 4k + e]
                for (int rs = 0; rs < 2; ++rs) {
                    const int row = 32 * g + 8 * wave + 2 * r4 + rs;
                    if (row >= NC) continue;
                    for (int k = 0; k < 8; ++k)
                        for (int e = 0; e < 4; ++e)
                            tf3[(size_t)g * 16384 + ((size_t)((wave * 2 + rs) * 8 + k) * 64 + lane) * 4 + e] =
                                wfc3[(size_t)row * FC + 32 * q + 4 * k + e];
                }
            }
        for (int j = 0; j < H; ++j) vwI0[j] = wI[(size_t)j * IN_I];
        for (int r = 0; r < 3 * H; ++r) {   // u = W_ih1 . W_I[:,0]
            double acc = 0.0;
            for (int j = 0; j < H; ++j) acc += (double)wih1[(size_t)r * H + j] * (double)wI[(size_t)j * IN_I];
            vu1[r] = (float)acc;
        }
    }
    // ---- batch kernel layouts (loop_batch.hip): MFMA 4x4x1 A-operand images.  Lane (kp = lane>>2, i = lane&3) of wave
    // wl of WG g holds W[row(16g + 4wl + i)][k], k = 64 S + 16 e + kp for register slab s = 4 S + e.
    std::vector<float> bw((size_t)32 * 4 * 320 * 64, 0.0f), bf3((size_t)32 * 16384, 0.0f), bwn((size_t)32 * 8192, 0.0f);
    {
        const float *whh1 = tv["rnn1.weight_hh_l0"].f(), *wih2 = tv["rnn2.weight_ih_l0"].f(), *whh2 = tv["rnn2.weight_hh_l0"].f();
        const float *wfc1 = tv["fc1.weight"].f(), *wfc2 = tv["fc2.weight"].f(), *wfc3 = tv["fc3.weight"].f();
        for (int g = 0; g < 32; ++g)
            for (int wl = 0; wl < 4; ++wl)
                for (int lane = 0; lane < 64; ++lane) {
                    const int kp = lane >> 2, i = lane & 3;
                    const int u = 16 * g + 4 * wl + i;
                    // register r of the wave: W_ih2 r,z,n [0,96) | W_hh1 r,z,n [96,192) | W_hh2 r,z [192,256) | fc1 [256,288) | fc2 [288,320)
                    auto at = [&](int r) -> float & { return bw[(((size_t)g * 4 + wl) * 320 + r) * 64 + lane]; };
                    for (int s2 = 0; s2 < 32; ++s2) {
                        const int k = 64 * (s2 >> 2) + 16 * (s2 & 3) + kp;
                        for (int gate = 0; gate < 3; ++gate) {
                            const size_t row = (size_t)gate * H + u;
                            at(gate * 32 + s2) = wih2[row * (H + A) + k];
                            at(96 + gate * 32 + s2) = whh1[row * H + k];
                            if (gate < 2) at(192 + gate * 32 + s2) = whh2[row * H + k];
                            else bwn[(size_t)g * 8192 + ((size_t)(wl * 8 + (s2 >> 2)) * 64 + lane) * 4 + (s2 & 3)] = whh2[row * H + k];   // LDS image
                        }
                        at(256 + s2) = wfc1[(size_t)u * (H + A) + k];
                        at(288 + s2) = wfc2[(size_t)u * (FC + A) + k];
                        for (int set = 0; set < 2; ++set) {
                            const int row = 32 * g + 8 * wl + 4 * set + i;
                            if (row < NC)
                                bf3[(size_t)g * 16384 + ((size_t)((wl * 2 + set) * 8 + (s2 >> 2)) * 64 + lane) * 4 + (s2 & 3)] = wfc3[(size_t)row * FC + k];
                        }
                    }
                }
    }
    WRNN_TRY(h, hipSetDevice(h->cfg.device));
    auto upload = [&](float *&dst, const std::vector<float> &src) -> int {
        if (dst) { (void)hipFree(dst); dst = nullptr; }
        WRNN_TRY(h, hipMalloc(&dst, src.size() * sizeof(float)));
        WRNN_TRY(h, hipMemcpy(dst, src.data(), src.size() * sizeof(float), hipMemcpyHostToDevice));
        return WRNN_OK;
    };
    if ((rc = upload(h->team_w, tw)) || (rc = upload(h->team_fc3, tf3)) || (rc = upload(h->wI0, vwI0)) || (rc = upload(h->u1, vu1)) ||
        (rc = upload(h->batch_w, bw)) || (rc = upload(h->batch_fc3, bf3)) || (rc = upload(h->batch_wn, bwn))) return rc;
    }
    WRNN_TRY(h, hipSetDevice(h->cfg.device));
    if (!h->mail) {
        WRNN_TRY(h, hipMalloc(&h->mail, WRNN_MAIL_BYTES));
        WRNN_TRY(h, hipMalloc(&h->ctl, TEAM_CTL_WORDS * sizeof(unsigned)));
    }
    if (h->wdev) { (void)hipFree(h->wdev); h->wdev = nullptr; }
    WRNN_TRY(h, hipMalloc(&h->wdev, o.total * sizeof(float)));
    WRNN_TRY(h, hipMemcpy(h->wdev, pk.data(), o.total * sizeof(float), hipMemcpyHostToDevice));
    h->teamg_img_ok = false;   // the TEAMG image is packed from wdev by the next TEAMG call
    h->teamg_sp_ok = false;
    h->loaded = true;
    return WRNN_OK;
}

static int ensure_aux(wrnn_handle *h, int B, int T) { return wrnn_grow(h, h->aux_frames, h->aux_cap, (size_t)B * T * h->d.R); }

int wrnn_conditioning(wrnn_handle *h, const float *mels_dev, int32_t B, int32_t T, int32_t mels_padded, float *up_dev, float *aux_dev, void *stream) {
    if (!h || !mels_dev || B < 1 || T < 1) return wrnn_failf(h, WRNN_ERR_INVALID, "wrnn_conditioning: bad arguments");
    if (!h->loaded) return wrnn_failf(h, WRNN_ERR_STATE, "weights not loaded");
    WRNN_TRY(h, hipSetDevice(h->cfg.device));
    hipStream_t s = (hipStream_t)stream;
    if (int rc = ensure_aux(h, B, T)) return rc;
    const int mel_T = mels_padded ? T + 2 * h->d.P : T, mel_off = mels_padded ? h->d.P : 0;
    WRNN_TRY(h, wrnn_launch_resnet(h, mels_dev, B, T, mel_T, mel_off, h->aux_frames, s));
    if (up_dev || aux_dev) WRNN_TRY(h, wrnn_launch_materialize(h, mels_dev, h->aux_frames, B, T, mel_T, mel_off, up_dev, aux_dev, s));
    return WRNN_OK;
}

int wrnn_plan(wrnn_handle *h, int32_t B, int32_t T, int32_t batched, int32_t target, int32_t overlap, int32_t *rows_out, int64_t *steps_out) {
    if (!h || B < 1 || T < 1) return wrnn_failf(h, WRNN_ERR_INVALID, "wrnn_plan: bad arguments");
    const int64_t total = (int64_t)T * h->d.HOP;
    if (!batched) {
        if (rows_out) *rows_out = B;
        if (steps_out) *steps_out = total;
        return WRNN_OK;
    }
    // fold_with_overlap (fatchord_version.py:293-340) indexes folded[i] = x[:, start:end, :] with a
    // batch-1 x; any other batch size raises in the reference.
    if (B != 1) return wrnn_failf(h, WRNN_ERR_INVALID, "batched generation requires a single utterance (fold_with_overlap)");
    if (target < 1 || overlap < 0) return wrnn_failf(h, WRNN_ERR_INVALID, "bad target/overlap");
    // Python floor division like fatchord_version.py:319 (a clip shorter than `overlap` gives -1 -> 0 folds -> error)
    const int64_t fold_den = (int64_t)target + overlap, fold_num = total - overlap;
    int64_t num_folds = fold_num / fold_den;
    if (fold_num % fold_den != 0 && fold_num < 0) --num_folds;
    const int64_t extended = num_folds * ((int64_t)overlap + target) + overlap;
    if (total - extended != 0) num_folds += 1;
    if (num_folds < 1) return wrnn_failf(h, WRNN_ERR_INVALID, "sequence shorter than one fold");
    if (rows_out) *rows_out = (int32_t)num_folds;
    if (steps_out) *steps_out = (int64_t)target + 2LL * overlap;
    return WRNN_OK;
}

}  // extern "C"

// Row table of a call (rows, order, sched, keys under the one capacity rows_cap), built on the device: nothing is staged on the host,
// the call never waits for the stream.
static int build_row_table(wrnn_handle *h, int32_t B, int32_t T, int32_t batched, int32_t target, int32_t overlap, const wrnn_sample_opts *opts,
                           const int32_t *fold_frames, int32_t rows, int64_t steps, int sched_teams, hipStream_t s) {
    if ((size_t)rows > h->rows_cap) {
        size_t cap[4] = {0, 0, 0, 0};   // rows_cap stays 0 until all four buffers are there
        h->rows_cap = 0;
        int rc;
        if ((rc = wrnn_grow(h, h->rows_dev, cap[0], (size_t)rows)) || (rc = wrnn_grow(h, h->order_dev, cap[1], (size_t)rows)) ||
            (rc = wrnn_grow(h, h->sched_dev, cap[2], (size_t)rows + 64)) || (rc = wrnn_grow(h, h->keys_dev, cap[3], (size_t)rows)))
            return rc;
        h->rows_cap = rows;
    }
    WRNN_TRY(h, hipMemsetAsync(h->err_dev, 0, 64, s));
    if (!fold_frames) {
        WRNN_TRY(h, wrnn_launch_rows(h->rows_dev, h->order_dev, h->sched_dev, rows, sched_teams, batched, (long)target + overlap, (long)steps,
                                         opts->frames_dev, T, h->d.HOP, h->keys_dev, opts->utt_seeds_dev, s));
        return WRNN_OK;
    }
    h->fold_B = 0;   // the fold offsets on the handle are valid once the kernel that writes them is enqueued
    if (int rc = wrnn_grow(h, h->fold0_dev, h->fold0_cap, (size_t)B + 1)) return rc;
    WRNN_TRY(h, wrnn_launch_rows_folded(h->rows_dev, h->order_dev, h->sched_dev, h->fold0_dev, h->err_dev, fold_frames, B, rows, sched_teams,
                                            (long)target, (long)overlap, h->d.HOP, T, h->keys_dev, opts->utt_seeds_dev, s));
    h->fold_B = B; h->fold_target = target; h->fold_overlap = overlap; h->fold_rows = rows;
    return WRNN_OK;
}

// The batch kernels: R = 4 * nq rows per XCD team in lock-step on the matrix cores (loop_batch.hip); the rows are spread evenly over
// the teams first (rpb rows per batch), a team runs ceil(batches / n_teams) batches one after the other.  a: the call's loop arguments.
static int run_batch(wrnn_handle *h, const WrnnLoopArgs &a, const WrnnFrameTables &t, int B, bool cs, int batch_rows, int snake, int *rpb_out, hipStream_t s) {
    const int rows = a.n_rows;
    WRNN_TRY(h, wrnn_launch_pack_records32(t.CM, t.CA, t.VM, t.VA, t.C2, t.C3, t.C4, t.REC, B, a.T, a.d.P, a.frames, s));
    int rpb = (rows + h->n_teams - 1) / h->n_teams;
    if (rpb > WRNN_BATCH_MAX_ROWS) rpb = WRNN_BATCH_MAX_ROWS;
    if (batch_rows > 0) rpb = batch_rows;
    if (cs && rpb > 4 * wrnn_batch_cs_max_nq(a.d.mode)) rpb = 4 * wrnn_batch_cs_max_nq(a.d.mode);   // critical / shadow wave roles (loop_batch_cs.hip)
    WrnnBatchArgs ba{};
    ba.w = a.w; ba.off = a.off; ba.d = a.d; ba.batch_w = h->batch_w; ba.batch_fc3 = h->batch_fc3; ba.batch_wn = h->batch_wn; ba.wI0 = h->wI0; ba.u1 = h->u1;
    ba.tabREC32 = t.REC; ba.rows = a.rows; ba.order = h->order_dev; ba.snake = snake; ba.n_rows = rows; ba.n_teams = h->n_teams; ba.nq = rpb <= 4 ? 1 : 2; ba.rpb = rpb;
    ba.T = a.T; ba.total_len = a.total_len; ba.steps = a.steps;
    wrnn_copy_sampling(ba, a);
    ba.mail = h->mail; ba.ctl = h->ctl; ba.err = a.err; ba.prof = h->prof_on ? h->prof : nullptr;
    if (ba.prof) WRNN_TRY(h, hipMemsetAsync(h->prof, 0, 8 * WRNN_PROF_SLOTS * sizeof(unsigned long long), s));
    WRNN_TRY(h, hipEventRecord(h->ev[1], s));  // tables and records are prologue work
    WRNN_TRY(h, wrnn_gated_launch(h->cfg.device, s, h->mail, WRNN_MAIL_BYTES, h->ctl, TEAM_CTL_WORDS * sizeof(unsigned),
                                      [&] { return cs ? wrnn_launch_loop_batch_cs(ba, s) : wrnn_launch_loop_batch(ba, s); }));
    h->prof_div = (double)a.steps * ((((rows + rpb - 1) / rpb) + h->n_teams - 1) / h->n_teams);
    *rpb_out = rpb;
    return WRNN_OK;
}

// The latency kernel: one row per XCD team at a time, in segments (launch.hip)
static int run_team2(wrnn_handle *h, const WrnnLoopArgs &a, const WrnnFrameTables &t, int B, int team2_segment, int snake, int n_slots, int *launches,
                     hipStream_t s) {
    const int rows = a.n_rows;
    WRNN_TRY(h, wrnn_launch_pack_records(t.CM, t.CA, t.VM, t.VA, t.REC, B, a.T, a.d.P, a.frames, s));
    if (a.frames) WRNN_TRY(h, wrnn_launch_mask_frame_tables(t.C2, t.C3, t.C4, a.frames, B, a.T, s));
    const int64_t seg = wrnn_team2_segment_len(rows, a.d.H, a.steps, team2_segment);
    int rc;
    if ((rc = wrnn_grow(h, h->cond, h->cond_cap, (size_t)rows * (size_t)seg * a.d.H * 4)) ||
        (rc = wrnn_grow(h, h->team_state, h->team_state_cap, (size_t)rows * WRNN_TEAM_STATE_FLOATS)))
        return rc;
    WrnnTeamArgs ta{};
    ta.w = a.w; ta.off = a.off; ta.d = a.d; ta.team_w = h->team_w; ta.team_fc3 = h->team_fc3; ta.wI0 = h->wI0; ta.u1 = h->u1;
    ta.tabREC = t.REC; ta.tabC2 = t.C2; ta.tabC3 = t.C3; ta.tabC4 = t.C4;
    ta.rows = a.rows; ta.sched = h->sched_dev; ta.n_slots = n_slots; ta.ragged = snake; ta.n_rows = rows; ta.n_teams = h->n_teams; ta.T = a.T; ta.total_len = a.total_len; ta.steps = a.steps;
    ta.state = h->team_state;
    wrnn_copy_sampling(ta, a);
    ta.mail = h->mail; ta.ctl = h->ctl; ta.err = a.err; ta.prof = h->prof_on ? h->prof : nullptr;
    WRNN_TRY(h, hipEventRecord(h->ev[1], s));  // the tables are prologue work; the stream chunks are timed with the loop
    if (ta.prof) WRNN_TRY(h, hipMemsetAsync(h->prof, 0, 8 * WRNN_PROF_SLOTS * sizeof(unsigned long long), s));
    h->prof_div = (double)a.steps * ((rows + h->n_teams - 1) / h->n_teams);
    return wrnn_run_team2_segments(h, ta, h->cond, 0, a.steps, seg, launches, s);
}

// The weight image of both kernels for any dims, in the handle's format: packed by the first call after a load or a format change.  The
// fp16 pack waits once for its range check; a weight with no finite fp16 fails the call and leaves no image.
static int teamg_image(wrnn_handle *h, const WrnnTeamGPlan &plan, hipStream_t s) {
    if (h->teamg_img_ok) return WRNN_OK;
    if (h->teamg_img) { (void)hipFree(h->teamg_img); h->teamg_img = nullptr; }
    WRNN_TRY(h, hipMalloc(&h->teamg_img, wrnn_teamg_img_bytes(plan)));
    if (h->teamg_sparse) {
        // the census has run (teamg_plan): compaction by its flags, no further wait
        for (int l = 0; l < WRNN_TEAMG_LAYERS; ++l) h->teamg_scale[l] = 1.0f;
        WRNN_TRY(h, wrnn_teamg_sparse_pack(h, plan, h->teamg_nb_a, h->teamg_nb_b, h->teamg_sp_flags, h->teamg_img, s));
        h->teamg_img_ok = true;
        WRNN_TRY(h, hipEventRecord(h->ev[1], s));
        return WRNN_OK;
    }
    int bad = -1;
    WRNN_TRY(h, wrnn_teamg_pack(h, plan, h->teamg_img, s, &bad, h->teamg_scale));
    if (bad >= 0 && plan.esz == 1) {
        for (int l = 0; l < WRNN_TEAMG_LAYERS; ++l) h->teamg_scale[l] = 1.0f;
        return wrnn_failf(h, WRNN_ERR_UNSUPPORTED, "WRNN_WEIGHTS_E4M3: a weight of layer %s is not finite, the layer has no scale; the fp32 image runs whatever the weights",
                         wrnn_teamg_layer_names[bad]);
    }
    if (bad >= 0)
        return wrnn_failf(h, WRNN_ERR_UNSUPPORTED, "WRNN_WEIGHTS_F16: a weight of layer %s does not round to a finite fp16 (|w| >= 65520); use WRNN_WEIGHTS_F32 for this model",
                         wrnn_teamg_layer_names[bad]);
    h->teamg_img_ok = true;
    WRNN_TRY(h, hipEventRecord(h->ev[1], s));   // the one-time image is not loop time
    return WRNN_OK;
}
// The plan of a TEAMG / TEAMG_BATCH call in the handle's format and setting; nullptr or why not (*rc = the error).  With the sparse setting
// on and no image packed, the census runs first (one wait): the plan needs each layer's longest list.  `probe`: only whether a plan
// exists for rb rows, nothing is recorded.
static const char *teamg_plan(wrnn_handle *h, const WrnnDims &d, int rb, WrnnTeamGPlan &plan, hipStream_t s, int *rc, bool probe = false) {
    const int esz = h->teamg_fmt == WRNN_WEIGHTS_E4M3 ? 1 : h->teamg_fmt == WRNN_WEIGHTS_F16 ? 2 : 4;
    *rc = WRNN_ERR_UNSUPPORTED;
    if (!h->teamg_sparse) return wrnn_teamg_make_plan(d, h->teamg_budget, plan, rb, esz);
    if (esz != 4)
        return h->teamg_fmt == WRNN_WEIGHTS_F16 ? "the sparse weight image (wrnn_teamg_set_sparse) holds fp32 values: it cannot be combined with WRNN_WEIGHTS_F16; reset either setting"
                                                : "the sparse weight image (wrnn_teamg_set_sparse) holds fp32 values: it cannot be combined with WRNN_WEIGHTS_E4M3; reset either setting";
    if (!h->teamg_img_ok && !h->teamg_sp_ok) {
        if (h->teamg_sp_flags) { (void)hipFree(h->teamg_sp_flags); h->teamg_sp_flags = nullptr; }
        hipError_t e = hipMalloc(&h->teamg_sp_flags, wrnn_teamg_sparse_flag_bytes(d));
        if (e == hipSuccess) e = wrnn_teamg_sparse_census(h, h->teamg_sp_flags, s, h->teamg_nb_a, h->teamg_nb_b, h->teamg_sp_kept, h->teamg_sp_dense);
        if (e != hipSuccess) { *rc = WRNN_ERR_HIP; return hipGetErrorString(e); }
        h->teamg_sp_ok = true;
    }
    const char *why = wrnn_teamg_make_plan(d, h->teamg_budget, plan, rb, 4, h->teamg_nb_a, h->teamg_nb_b);
    if (!why && !probe) { h->teamg_sp_budget = h->teamg_budget; h->teamg_sp_rows = rb; }
    return why;
}
static void teamg_sparse_args(const wrnn_handle *h, WrnnTeamGSparse &sp) {
    sp = WrnnTeamGSparse{};
    sp.on = h->teamg_sparse ? 1 : 0;
    for (int l = 0; l < WRNN_TEAMG_LAYERS; ++l) { sp.nbA[l] = h->teamg_nb_a[l]; sp.nbB[l] = h->teamg_nb_b[l]; }
}
static int teamg_esz(const wrnn_handle *h) { return h->teamg_fmt == WRNN_WEIGHTS_E4M3 ? 1 : h->teamg_fmt == WRNN_WEIGHTS_F16 ? 2 : 4; }
// the scales of the packed image into a plan made for this call (wrnn_teamg_make_plan leaves them 1)
static void teamg_plan_scales(const wrnn_handle *h, WrnnTeamGPlan &p) {
    for (int l = 0; l < WRNN_TEAMG_LAYERS; ++l) p.L[l].scale = h->teamg_scale[l];
}

// The team kernel for any dims (loop_teamg.hip): one row per XCD team at a time, one launch.  Placement and residency are settled here,
// before the launch; whatever keeps the kernel from running is an error with its reason, never another kernel.
static int run_teamg(wrnn_handle *h, const WrnnLoopArgs &a, int snake, int n_slots, hipStream_t s) {
    if (h->force_no_teams) return wrnn_failf(h, WRNN_ERR_INVALID, "team kernels disabled by wrnn_debug_force_no_teams (test hook)");
    if (h->n_teams < 1) return wrnn_failf(h, WRNN_ERR_UNSUPPORTED, "WRNN_KERNEL_TEAMG: fewer than 32 CUs visible (one team = the 32 CUs of an XCD)");
    WrnnTeamGArgs ga{};
    int prc = 0;
    if (const char *why = teamg_plan(h, a.d, 1, ga.plan, s, &prc)) return wrnn_failf(h, prc, "%s", why);
    int blocks = 0;
    const hipError_t oe = wrnn_teamg_occupancy(ga.plan, &blocks, h->teamg_sparse);
    (void)hipGetLastError();
    if (oe != hipSuccess || blocks < 1)
        return wrnn_failf(h, WRNN_ERR_UNSUPPORTED, "WRNN_KERNEL_TEAMG: loop_teamg_kernel cannot be resident on a CU with %zu bytes of LDS (%s)",
                         wrnn_teamg_lds_bytes(ga.plan), oe != hipSuccess ? hipGetErrorString(oe) : "occupancy 0");
    if (int rc = teamg_image(h, ga.plan, s)) return rc;
    teamg_plan_scales(h, ga.plan);
    ga.a = a; ga.img = h->teamg_img; ga.sched = h->sched_dev; ga.n_slots = n_slots; ga.ragged = snake; ga.n_teams = h->n_teams;
    ga.mail = h->mail; ga.ctl = h->ctl;
    teamg_sparse_args(h, ga.sp);
    const size_t mail_bytes = (size_t)h->n_teams * ga.plan.mail_granules * sizeof(unsigned long long);   // sized from the dims; <= WRNN_MAIL_BYTES
    WRNN_TRY(h, wrnn_gated_launch(h->cfg.device, s, h->mail, mail_bytes, h->ctl, TEAM_CTL_WORDS * sizeof(unsigned), [&] { return wrnn_launch_loop_teamg(ga, s); }));
    return WRNN_OK;
}

// The same kernel with rpb > 1 rows per team in lock-step (loop_teamg_batch.hip) on its instantiation rb = 2, 4 or 8; the refusals of
// run_teamg, the weight image of run_teamg.
static int run_teamg_batch(wrnn_handle *h, const WrnnLoopArgs &a, int snake, int rpb, hipStream_t s) {
    if (h->force_no_teams) return wrnn_failf(h, WRNN_ERR_INVALID, "team kernels disabled by wrnn_debug_force_no_teams (test hook)");
    if (h->n_teams < 1) return wrnn_failf(h, WRNN_ERR_UNSUPPORTED, "WRNN_KERNEL_TEAMG_BATCH: fewer than 32 CUs visible (one team = the 32 CUs of an XCD)");
    const int rb = wrnn_teamg_batch_inst(rpb);
    WrnnTeamGBatchArgs ga{};
    int prc = 0;
    if (const char *why = teamg_plan(h, a.d, rb, ga.plan, s, &prc)) return wrnn_failf(h, prc, "%s (batch_rows %d runs as %d)", why, rpb, rb);
    int blocks = 0;
    const hipError_t oe = wrnn_teamg_batch_occupancy(ga.plan, rb, &blocks, h->teamg_sparse);
    (void)hipGetLastError();
    if (oe != hipSuccess || blocks < 1)
        return wrnn_failf(h, WRNN_ERR_UNSUPPORTED, "WRNN_KERNEL_TEAMG_BATCH: loop_teamg_batch_kernel<%d> cannot be resident on a CU with %zu bytes of LDS (%s)", rb,
                         wrnn_teamg_lds_bytes(ga.plan), oe != hipSuccess ? hipGetErrorString(oe) : "occupancy 0");
    if (int rc = teamg_image(h, ga.plan, s)) return rc;
    teamg_plan_scales(h, ga.plan);
    ga.a = a; ga.img = h->teamg_img; ga.order = h->order_dev; ga.rpb = rpb; ga.snake = snake; ga.n_teams = h->n_teams;
    ga.mail = h->mail; ga.ctl = h->ctl;
    teamg_sparse_args(h, ga.sp);
    const size_t mail_bytes = (size_t)h->n_teams * ga.plan.mail_granules * sizeof(unsigned long long);   // <= WRNN_MAIL_BYTES: the plan refuses more
    WRNN_TRY(h, wrnn_gated_launch(h->cfg.device, s, h->mail, mail_bytes, h->ctl, TEAM_CTL_WORDS * sizeof(unsigned), [&] { return wrnn_launch_loop_teamg_batch(ga, rb, s); }));
    return WRNN_OK;
}

// Body of wrnn_generate and wrnn_generate_folded.  fold_frames != null: the rows are the folds of ALL B utterances (rows_total of them,
// see rows_folded_kernel), every per-frame table entry past an utterance's own end is its zero-input entry T.
static int generate_impl(wrnn_handle *h, const float *mels_dev, int32_t B, int32_t T, int32_t batched, int32_t target, int32_t overlap,
                         const wrnn_sample_opts *opts, int32_t *labels_out_dev, float *samples_out_dev, void *stream,
                         const int32_t *fold_frames, int32_t rows_total) {
    if (!h || !mels_dev || !opts || !samples_out_dev) return wrnn_failf(h, WRNN_ERR_INVALID, "wrnn_generate: bad arguments");
    if (opts->struct_size != sizeof(wrnn_sample_opts))
        return wrnn_failf(h, WRNN_ERR_INVALID, "wrnn_sample_opts.struct_size is %u, this library (ABI %d) expects %zu: caller built against another revision of wavernn_amd.h",
                    opts->struct_size, WRNN_ABI_VERSION, sizeof(wrnn_sample_opts));
    if (!h->loaded) return wrnn_failf(h, WRNN_ERR_STATE, "weights not loaded");
    if (opts->frames_dev && batched) return wrnn_failf(h, WRNN_ERR_INVALID, "frames_dev (ragged batch) is for unbatched calls: folds of one utterance have one length");
    if (opts->batch_rows < 0 || opts->batch_rows > WRNN_BATCH_MAX_ROWS) return wrnn_failf(h, WRNN_ERR_INVALID, "batch_rows must be 0 (default) or 1..%d", WRNN_BATCH_MAX_ROWS);
    if (opts->team2_segment < 0) return wrnn_failf(h, WRNN_ERR_INVALID, "team2_segment must be >= 0");
    const WrnnDims &d = h->d;
    int32_t rows = 0;
    int64_t steps = 0;
    if (fold_frames) {
        if (B < 1 || T < 1 || rows_total < 1 || target < 1 || overlap < 0) return wrnn_failf(h, WRNN_ERR_INVALID, "wrnn_generate_folded: bad arguments");
        rows = rows_total;
        steps = (int64_t)target + 2LL * overlap;
    } else if (int rc = wrnn_plan(h, B, T, batched, target, overlap, &rows, &steps)) return rc;
    if (opts->noise_mode == WRNN_NOISE_INJECTED && (!opts->noise1_dev || (d.mode == WRNN_MODE_MOL && !opts->noise2_dev)))
        return wrnn_failf(h, WRNN_ERR_INVALID, "WRNN_NOISE_INJECTED needs noise pointers");
    if (opts->noise_mode == WRNN_NOISE_ARGMAX && d.mode != WRNN_MODE_RAW)
        return wrnn_failf(h, WRNN_ERR_INVALID, "WRNN_NOISE_ARGMAX is RAW-only");
    if (opts->noise_mode < 0 || opts->noise_mode > 2) return wrnn_failf(h, WRNN_ERR_INVALID, "bad noise_mode");
    if (opts->utt_seeds_dev && opts->noise_mode != WRNN_NOISE_PHILOX)
        return wrnn_failf(h, WRNN_ERR_INVALID, "utt_seeds_dev (per-utterance seeds) needs noise_mode WRNN_NOISE_PHILOX");
    if (opts->utt_seeds_dev && batched && !fold_frames)
        return wrnn_failf(h, WRNN_ERR_INVALID, "utt_seeds_dev is for unbatched calls and wrnn_generate_folded: a batched wrnn_generate has one utterance, `seed` is its key");
    WRNN_TRY(h, hipSetDevice(h->cfg.device));
    hipStream_t s = (hipStream_t)stream;

    const int sched_teams = h->n_teams < 1 ? 1 : h->n_teams;
    if (int rc = build_row_table(h, B, T, batched, target, overlap, opts, fold_frames, rows, steps, sched_teams, s)) return rc;
    const int snake = opts->frames_dev ? 1 : 0;
    if (int rc = ensure_aux(h, B, T)) return rc;

    WRNN_TRY(h, hipEventRecord(h->ev[0], s));
    const int mel_T = opts->mels_padded ? T + 2 * d.P : T, mel_off = opts->mels_padded ? d.P : 0;
    WRNN_TRY(h, wrnn_launch_resnet(h, mels_dev, B, T, mel_T, mel_off, h->aux_frames, s));
    WRNN_TRY(h, hipEventRecord(h->ev[1], s));

    WrnnLoopArgs a{};
    a.w = h->wdev; a.off = h->off; a.d = d; a.mels = mels_dev; a.mel_T = mel_T; a.mel_off = mel_off; a.aux_frames = h->aux_frames; a.rows = h->rows_dev;
    a.n_rows = rows; a.T = T; a.total_len = (int64_t)T * d.HOP; a.steps = steps;
    a.noise_mode = opts->noise_mode; a.seed = opts->seed; a.keys = opts->utt_seeds_dev ? h->keys_dev : nullptr; a.noise1 = opts->noise1_dev; a.noise2 = opts->noise2_dev;
    a.x_forced = opts->x_forced_dev; a.x_init = opts->x_init_dev; a.logits_out = opts->logits_out_dev; a.labels_out = labels_out_dev;
    a.samples_out = samples_out_dev; a.err = h->err_dev; a.frames = fold_frames;
    int kernel = opts->kernel;
    int launches = 1, batch_rows_run = 1;
    // what the team kernels (TEAM2, BATCH) need: co-residency (checked in wrnn_create), the 5-frame upsampling support
    // of pad = 2, hop <= 275, and 1024 or fewer classes.  AUTO falls back to the any-shape kernel otherwise;
    // an explicit request for a team kernel that cannot run is an error.
    const char *team_no = loop_team_obstacle(h);
    if (kernel == WRNN_KERNEL_AUTO) {
        if (team_no) kernel = WRNN_KERNEL_SIMPLE;
        // one row per XCD team: the latency kernel; more rows: the batch step with critical / shadow wave roles (round 4: 7.5 against 6.85
        // Msamples/s at RAW B = 64, 5.6 against 5.3 at MOL B = 32; WRNN_KERNEL_BATCH stays available by name)
        else kernel = rows <= h->n_teams ? WRNN_KERNEL_TEAM2 : (h->cs_ok ? WRNN_KERNEL_BATCH_CS : WRNN_KERNEL_BATCH);
    }
    if (kernel == WRNN_KERNEL_BATCH_CS && !team_no && !h->cs_ok) team_no = "loop_batch_cs_kernel cannot be resident (LDS/registers); WRNN_KERNEL_BATCH can";
    if (kernel == WRNN_KERNEL_SIMPLE) {
        WRNN_TRY(h, wrnn_launch_loop_simple(a, s));
    } else if (kernel == WRNN_KERNEL_TEAM2 || kernel == WRNN_KERNEL_BATCH || kernel == WRNN_KERNEL_BATCH_CS) {
        const bool batch_family = kernel != WRNN_KERNEL_TEAM2;
        if (team_no) return wrnn_failf(h, WRNN_ERR_INVALID, "%s", team_no);
        WrnnFrameTables t;
        if (int rc = wrnn_build_frame_tables(h, h->tab, h->tab_cap, mels_dev, mel_T, d.P - mel_off, h->aux_frames, B, T, batch_family ? 32 : 28, t, s)) return rc;
        if (int rc = batch_family ? run_batch(h, a, t, B, kernel == WRNN_KERNEL_BATCH_CS, opts->batch_rows, snake, &batch_rows_run, s)
                                  : run_team2(h, a, t, B, opts->team2_segment, snake, (rows + sched_teams - 1) / sched_teams * sched_teams, &launches, s))
            return rc;
    } else if (kernel == WRNN_KERNEL_TEAMG) {
        if (int rc = run_teamg(h, a, snake, (rows + sched_teams - 1) / sched_teams * sched_teams, s)) return rc;
    } else if (kernel == WRNN_KERNEL_TEAMG_BATCH) {
        // rows per team as run_batch spreads them; left to the library (batch_rows 0) it is lowered to the largest instantiation whose
        // activation vectors and mailbox regions the plan admits for these dims.  One row per team is WRNN_KERNEL_TEAMG itself.
        int rpb = (rows + sched_teams - 1) / sched_teams;
        if (rpb > WRNN_TEAMG_BATCH_MAX_ROWS) rpb = WRNN_TEAMG_BATCH_MAX_ROWS;
        if (opts->batch_rows > 0) rpb = opts->batch_rows;
        else {
            WrnnTeamGPlan probe;
            while (rpb > 1 && wrnn_teamg_make_plan(d, h->teamg_budget, probe, wrnn_teamg_batch_inst(rpb), teamg_esz(h))) rpb = wrnn_teamg_batch_inst(rpb) / 2;
        }
        if (rpb == 1) {
            kernel = WRNN_KERNEL_TEAMG;
            if (int rc = run_teamg(h, a, snake, (rows + sched_teams - 1) / sched_teams * sched_teams, s)) return rc;
        } else if (int rc = run_teamg_batch(h, a, snake, rpb, s)) return rc;
        batch_rows_run = rpb;
    } else {
        return wrnn_failf(h, WRNN_ERR_INVALID, "kernel %d not available", kernel);
    }
    WRNN_TRY(h, hipEventRecord(h->ev[2], s));
    h->timing_valid = true;
    h->last.kernel = kernel; h->last.rows = rows; h->last.steps = steps; h->last.launches = launches;
    h->last_batch_rows = batch_rows_run;
    return WRNN_OK;
}

extern "C" {

int wrnn_generate(wrnn_handle *h, const float *mels_dev, int32_t B, int32_t T, int32_t batched, int32_t target, int32_t overlap,
                  const wrnn_sample_opts *opts, int32_t *labels_out_dev, float *samples_out_dev, void *stream) {
    return generate_impl(h, mels_dev, B, T, batched, target, overlap, opts, labels_out_dev, samples_out_dev, stream, nullptr, 0);
}

int wrnn_plan_folded(const int32_t *frames_host, int32_t B, int32_t hop, int32_t target, int32_t overlap, int32_t *fold0_out,
                     int64_t *steps_out) {
    if (!frames_host || !fold0_out || B < 1 || hop < 1 || target < 1 || overlap < 0) return WRNN_ERR_INVALID;
    const int64_t stride = (int64_t)target + overlap;
    int64_t acc = 0;
    fold0_out[0] = 0;
    for (int32_t b = 0; b < B; ++b) {
        if (frames_host[b] < 1) return WRNN_ERR_INVALID;
        // Python floor division like fatchord_version.py:319-325 (see wrnn_plan)
        const int64_t total = (int64_t)frames_host[b] * hop, num = total - overlap;
        int64_t n = num / stride;
        if (num % stride != 0 && num < 0) --n;
        if (total - (n * stride + overlap) != 0) ++n;
        if (n < 1) return WRNN_ERR_INVALID;   // shorter than one fold
        acc += n;
        if (acc > INT32_MAX) return WRNN_ERR_INVALID;
        fold0_out[b + 1] = (int32_t)acc;
    }
    if (steps_out) *steps_out = (int64_t)target + 2LL * overlap;
    return WRNN_OK;
}

int wrnn_generate_folded(wrnn_handle *h, const float *mels_dev, int32_t B, int32_t T, const int32_t *frames_dev, int32_t rows_total,
                         int32_t target, int32_t overlap, const wrnn_sample_opts *opts, int32_t *labels_out_dev,
                         float *samples_out_dev, void *stream) {
    if (!h || !frames_dev) return wrnn_failf(h, WRNN_ERR_INVALID, "wrnn_generate_folded: bad arguments");
    if (opts && opts->struct_size == sizeof(wrnn_sample_opts) &&
        (opts->frames_dev || opts->mels_padded || opts->x_forced_dev || opts->x_init_dev || opts->logits_out_dev))
        return wrnn_failf(h, WRNN_ERR_INVALID, "wrnn_generate_folded: opts.frames_dev, mels_padded, x_forced_dev, x_init_dev and logits_out_dev must be unset");
    return generate_impl(h, mels_dev, B, T, 1, target, overlap, opts, labels_out_dev, samples_out_dev, stream, frames_dev, rows_total);
}

int wrnn_loss(wrnn_handle *h, const float *y_hat_dev, const void *y_dev, int64_t n_rows, float *loss_out_dev, void *stream) {
    if (!h || !y_hat_dev || !y_dev || !loss_out_dev || n_rows < 1) return wrnn_failf(h, WRNN_ERR_INVALID, "wrnn_loss: bad arguments");
    WRNN_TRY(h, hipSetDevice(h->cfg.device));
    hipStream_t s = (hipStream_t)stream;
    const size_t nblk = (size_t)(h->d.mode == WRNN_MODE_RAW ? (n_rows + 3) / 4 : (n_rows + 255) / 256);
    if (int rc = wrnn_grow(h, h->loss_partial, h->loss_cap, nblk + 1)) return rc;
    int *bad = (int *)(h->loss_partial + nblk);
    WRNN_TRY(h, hipMemsetAsync(bad, 0, sizeof(double), s));
    WRNN_TRY(h, wrnn_launch_loss(h->d.mode, y_hat_dev, y_dev, h->d.NC, (long)n_rows, h->loss_partial, bad, loss_out_dev, s));
    return WRNN_OK;
}

int wrnn_last_timing(wrnn_handle *h, wrnn_timing *out) {
    if (!h) return WRNN_ERR_INVALID;
    if (!h->timing_valid) return wrnn_failf(h, WRNN_ERR_STATE, "no generate call to time");
    WRNN_TRY(h, hipSetDevice(h->cfg.device));
    WRNN_TRY(h, hipEventSynchronize(h->ev[2]));
    WRNN_TRY(h, hipEventElapsedTime(&h->last.prologue_ms, h->ev[0], h->ev[1]));
    WRNN_TRY(h, hipEventElapsedTime(&h->last.loop_ms, h->ev[1], h->ev[2]));
    unsigned errw = 0;
    WRNN_TRY(h, hipMemcpy(&errw, h->err_dev, sizeof(errw), hipMemcpyDeviceToHost));
    if (out) *out = h->last;
    if (errw == WRNN_DEVERR_ROWS)
        return wrnn_failf(h, WRNN_ERR_INVALID, "wrnn_generate_folded: rows_total differs from the fold count of frames_dev on the device "
                                         "(wrnn_plan_folded gives it for the same frames, target and overlap)");
    if (errw == WRNN_DEVERR_BUSY)
        return wrnn_failf(h, WRNN_ERR_BUSY, "the team kernel's workgroups did not all become resident within its start-up wait: the GPU is shared with another "
                                      "kernel (another process?).  Retry, or use WRNN_KERNEL_SIMPLE");
    if (errw) return wrnn_failf(h, WRNN_ERR_TIMEOUT, "device-side bounded spin gave up (code %u)", errw);
    return WRNN_OK;
}

int wrnn_phase_profile(wrnn_handle *h, int32_t enable) {
    if (!h) return WRNN_ERR_INVALID;
    WRNN_TRY(h, hipSetDevice(h->cfg.device));
    if (enable) {
        // the instrumented instantiations have their own register / LDS footprint: check their residency like wrnn_create does
        int blocks = 0;
        size_t lds = 0;
        if (h->team_ok) {
            hipError_t e = wrnn_team2_occupancy(h->cfg.mode, true, &blocks, &lds);
            for (int nq = 1; nq <= 2 && e == hipSuccess && blocks >= 1; ++nq) e = wrnn_batch_occupancy(h->cfg.mode, nq, true, &blocks, &lds);
            for (int nq = 1; nq <= wrnn_batch_cs_max_nq(h->cfg.mode) && e == hipSuccess && blocks >= 1; ++nq) e = wrnn_batch_cs_occupancy(h->cfg.mode, nq, true, &blocks, &lds);
            (void)hipGetLastError();
            if (e != hipSuccess || blocks < 1) return wrnn_failf(h, WRNN_ERR_INVALID, "the instrumented team kernels cannot be resident on this device");
        }
        if (!h->prof) WRNN_TRY(h, hipMalloc(&h->prof, 8 * WRNN_PROF_SLOTS * sizeof(unsigned long long)));
        WRNN_TRY(h, hipMemset(h->prof, 0, 8 * WRNN_PROF_SLOTS * sizeof(unsigned long long)));
    }
    h->prof_on = enable != 0;
    return WRNN_OK;
}

int wrnn_phase_cycles(wrnn_handle *h, double *out) {
    if (!h || !out) return WRNN_ERR_INVALID;
    if (!h->prof_on || !h->prof || !h->timing_valid) return wrnn_failf(h, WRNN_ERR_STATE, "no instrumented call to report (wrnn_phase_profile(h, 1), then a TEAM2 / BATCH call)");
    WRNN_TRY(h, hipSetDevice(h->cfg.device));
    WRNN_TRY(h, hipEventSynchronize(h->ev[2]));
    unsigned long long pr[8 * WRNN_PROF_SLOTS];
    WRNN_TRY(h, hipMemcpy(pr, h->prof, sizeof(pr), hipMemcpyDeviceToHost));
    const double n = h->prof_div > 0 ? h->prof_div : 1.0;   // steps x rows (or batches) team 0 ran
    for (int i = 0; i < 8 * WRNN_PROF_SLOTS; ++i) out[i] = (double)pr[i] / n;
    return WRNN_OK;
}

}  // extern "C"

// ---- mel front end: a handle of its own, no weights ---------------------------------------------------------------

struct wrnn_mel_handle {
    wrnn_mel_config cfg{};
    wrnn_mel_features feat{};
    bool profile = false;         // feat differs from the default profile: the kernel's profile instantiation runs
    WrnnMelTables tab;
    void *dev = nullptr;          // one allocation: window | twiddle | rows | weights | peak workspace, made by the first wrnn_melspectrogram
    size_t o_tw = 0, o_rows = 0, o_w = 0, o_peak = 0;
    std::string err;
};

extern "C" {

int wrnn_mel_create(const wrnn_mel_config *cfg, wrnn_mel_handle **out) { return wrnn_mel_create_features(cfg, &WRNN_DEFAULT_MEL_FEATURES, out); }

int wrnn_mel_create_features(const wrnn_mel_config *cfg, const wrnn_mel_features *f, wrnn_mel_handle **out) {
    if (!cfg || !f || !out) return WRNN_ERR_INVALID;
    wrnn_mel_handle *h = new wrnn_mel_handle();
    *out = h;
    h->cfg = *cfg;
    if (f->struct_size != sizeof(wrnn_mel_features))
        return wrnn_failf(h, WRNN_ERR_INVALID, "features.struct_size = %u, this library's wrnn_mel_features has %zu bytes", f->struct_size, sizeof(wrnn_mel_features));
    h->feat = *f;
    if (const int rc = wrnn_mel_check(h, cfg, f, "the front end")) return rc;
    if (!wrnn_mel_build_tables(cfg->sample_rate, cfg->win_length, cfg->n_mels, (double)cfg->fmin, (double)f->fmax, &h->tab))
        return wrnn_failf(h, WRNN_ERR_INVALID, "bad configuration: 1 <= win_length <= n_fft, 1 <= n_mels <= %d, 0 <= fmin < sample_rate / 2", WRNN_MEL_MAX_MELS);
    // fmax lives in the filterbank table alone, so it needs no arm of the kernel
    h->profile = f->pad_mode != WRNN_MEL_PAD_REFLECT || f->magnitude_power != 1 || f->ref_level_db != 0.0f || f->preemphasis != 0.0f ||
                 f->preemph_rescale != 0.0f || f->max_abs_value != 0.0f;
    return WRNN_OK;
}

int64_t wrnn_mel_frames(const wrnn_mel_handle *h, int64_t n_samples) {
    if (!h || h->tab.window.empty()) return WRNN_ERR_INVALID;
    if (n_samples < (h->feat.pad_mode == WRNN_MEL_PAD_ZERO ? 1 : h->cfg.n_fft / 2 + 1)) return WRNN_ERR_INVALID;
    return 1 + n_samples / h->cfg.hop_length;
}

int wrnn_mel_tables(const wrnn_mel_handle *h, float *window, float *twiddle, int32_t *rows, float *weights, int32_t *n_weights) {
    if (!h || h->tab.window.empty()) return WRNN_ERR_INVALID;
    const WrnnMelTables &t = h->tab;
    if (window) std::copy(t.window.begin(), t.window.end(), window);
    if (twiddle) std::copy(t.twiddle.begin(), t.twiddle.end(), twiddle);
    if (rows) std::copy(t.rows.begin(), t.rows.end(), rows);
    if (weights) std::copy(t.weights.begin(), t.weights.end(), weights);
    if (n_weights) *n_weights = (int32_t)t.weights.size();
    return WRNN_OK;
}

int wrnn_melspectrogram(wrnn_mel_handle *h, const float *wav_dev, int64_t n_max, const int32_t *n_samples_dev, int32_t B, int32_t T_max,
                        float *mel_out_dev, void *stream) {
    if (!h) return WRNN_ERR_INVALID;
    if (h->tab.window.empty()) return wrnn_failf(h, WRNN_ERR_STATE, "the handle's configuration was refused by wrnn_mel_create");
    if (!wav_dev || !n_samples_dev || !mel_out_dev || n_max < 1 || B < 1 || B > WRNN_MAX_GRID_Y || T_max < 1)
        return wrnn_failf(h, WRNN_ERR_INVALID, "bad arguments: device pointers, n_max >= 1, 1 <= B <= 65535, T_max >= 1");
    WRNN_TRY(h, hipSetDevice(h->cfg.device));
    const WrnnMelTables &t = h->tab;
    if (!h->dev) {
        // window | twiddle | rows | weights | the peak workspace: one float per clip of the largest batch
        WrnnImage img;
        img.put(t.window.data(), t.window.size() * 4);
        h->o_tw = img.put(t.twiddle.data(), t.twiddle.size() * 4);
        h->o_rows = img.put(t.rows.data(), t.rows.size() * 4);
        h->o_w = img.put(t.weights.data(), t.weights.size() * 4);
        h->o_peak = h->feat.preemph_rescale > 0.0f ? img.take((size_t)WRNN_MAX_GRID_Y * 4) : img.bytes.size();
        const hipError_t e = img.upload(&h->dev);
        if (e != hipSuccess) return wrnn_failf(h, WRNN_ERR_HIP, "uploading the front-end tables: %s", hipGetErrorString(e));
    }
    WrnnMelArgs a{};
    const char *d = (const char *)h->dev;
    a.wav = wav_dev; a.n_samples = n_samples_dev; a.out = mel_out_dev;
    a.window = (const float *)d; a.twiddle = (const float2 *)(d + h->o_tw);
    a.rows = (const int32_t *)(d + h->o_rows); a.weights = (const float *)(d + h->o_w);
    a.n_max = n_max; a.T_max = T_max; a.n_mels = h->cfg.n_mels; a.hop = h->cfg.hop_length; a.win_length = h->cfg.win_length;
    a.min_level_db = h->cfg.min_level_db;
    if (h->profile) {
        const wrnn_mel_features &f = h->feat;
        a.pad_zero = f.pad_mode == WRNN_MEL_PAD_ZERO; a.power2 = f.magnitude_power == 2;
        a.preemph = f.preemphasis; a.rescale = f.preemph_rescale; a.ref_level_db = f.ref_level_db; a.max_abs = f.max_abs_value;
        a.floor_amp = (float)std::pow(10.0, (double)h->cfg.min_level_db / 20.0);
        if (f.preemph_rescale > 0.0f) {
            float *peak = (float *)((char *)h->dev + h->o_peak);
            a.peak = peak;
            WRNN_TRY(h, wrnn_launch_mel_peak(wav_dev, n_max, n_samples_dev, B, f.preemphasis, peak, (hipStream_t)stream));
        }
    }
    WRNN_TRY(h, wrnn_launch_melspec(a, B, h->profile, (hipStream_t)stream));
    return WRNN_OK;
}

const char *wrnn_mel_last_error(const wrnn_mel_handle *h) { return wrnn_last_error_of(h); }

void wrnn_mel_destroy(wrnn_mel_handle *h) {
    if (!h) return;
    if (h->dev) {
        (void)hipSetDevice(h->cfg.device);
        (void)hipFree(h->dev);
    }
    delete h;
}

}  // extern "C"

// ---- resampler: a handle of its own, like the mel front end ------------------------------------------------------------

struct wrnn_resample_handle {
    int32_t src_rate = 0, dst_rate = 0, device = 0;
    WrnnResamplePlan plan;
    void *bank_dev = nullptr;     // wrnn_resample_device_bank, uploaded by the first wrnn_resample
    std::string err;
};

extern "C" {

int wrnn_resample_create(int32_t src_rate, int32_t dst_rate, int32_t device, wrnn_resample_handle **out) {
    if (!out) return WRNN_ERR_INVALID;
    wrnn_resample_handle *h = new wrnn_resample_handle();
    *out = h;
    h->src_rate = src_rate; h->dst_rate = dst_rate; h->device = device;
    if (device < 0) return wrnn_failf(h, WRNN_ERR_INVALID, "bad configuration: device >= 0");
    const int rc = wrnn_resample_build_plan(src_rate, dst_rate, &h->plan);
    if (rc == WRNN_ERR_INVALID) return wrnn_failf(h, rc, "bad configuration: %d Hz -> %d Hz, both rates must be positive", src_rate, dst_rate);
    if (rc != WRNN_OK)
        return wrnn_failf(h, rc, "%d Hz -> %d Hz is outside what the resampler is built for: a ratio of at least 1/%d and a filter bank of at most "
                              "%d entries (the bank has one phase per output position of the reduced ratio)",
                       src_rate, dst_rate, WRNN_RS_MIN_SCALE_INV, WRNN_RS_MAX_BANK);
    return WRNN_OK;
}

int64_t wrnn_resample_out_len(const wrnn_resample_handle *h, int64_t n_in) {
    if (!h || h->plan.bank.empty() || n_in < 0 || n_in > INT32_MAX) return WRNN_ERR_INVALID;
    return (n_in * h->plan.p + h->plan.q - 1) / h->plan.q;
}

int wrnn_resample_bank(const wrnn_resample_handle *h, float *bank, int32_t *p, int32_t *q, int32_t *taps) {
    if (!h || h->plan.bank.empty()) return WRNN_ERR_INVALID;
    if (bank) std::copy(h->plan.bank.begin(), h->plan.bank.end(), bank);
    if (p) *p = h->plan.p;
    if (q) *q = h->plan.q;
    if (taps) *taps = h->plan.taps;
    return WRNN_OK;
}

int wrnn_resample(wrnn_resample_handle *h, const float *in_dev, int64_t n_in_max, const int32_t *n_in_dev, int32_t B, int64_t n_out_max,
                  float *out_dev, void *stream) {
    if (!h) return WRNN_ERR_INVALID;
    const WrnnResamplePlan &pl = h->plan;
    if (pl.bank.empty()) return wrnn_failf(h, WRNN_ERR_STATE, "the handle's rates were refused by wrnn_resample_create");
    if (pl.p == pl.q) return wrnn_failf(h, WRNN_ERR_INVALID, "equal rates: there is nothing to resample, and the filter is a low-pass that must not run at ratio 1");
    if (!in_dev || !n_in_dev || !out_dev || n_in_max < 1 || n_in_max > INT32_MAX || B < 1 || B > WRNN_MAX_GRID_Y || n_out_max < 1 ||
        n_out_max > (int64_t)INT32_MAX * WRNN_RS_TILE)
        return wrnn_failf(h, WRNN_ERR_INVALID, "bad arguments: device pointers, 1 <= n_in_max < 2^31, 1 <= B <= 65535, n_out_max >= 1");
    WRNN_TRY(h, hipSetDevice(h->device));
    if (!h->bank_dev) {
        const std::vector<float> bt = wrnn_resample_device_bank(pl);
        WrnnImage img;
        img.put(bt.data(), bt.size() * sizeof(float));
        const hipError_t e = img.upload(&h->bank_dev);
        if (e != hipSuccess) return wrnn_failf(h, WRNN_ERR_HIP, "uploading the filter bank: %s", hipGetErrorString(e));
    }
    WrnnResampleArgs a{};
    a.in = in_dev; a.n_in = n_in_dev; a.out = out_dev; a.bank = (const float *)h->bank_dev;
    a.n_in_max = n_in_max; a.n_out_max = n_out_max;
    a.p = pl.p; a.q = pl.q; a.half = pl.half; a.taps = pl.taps;
    WRNN_TRY(h, wrnn_launch_resample(a, B, pl.span_max, (hipStream_t)stream));
    return WRNN_OK;
}

const char *wrnn_resample_last_error(const wrnn_resample_handle *h) { return wrnn_last_error_of(h); }

void wrnn_resample_destroy(wrnn_resample_handle *h) {
    if (!h) return;
    if (h->bank_dev) {
        (void)hipSetDevice(h->device);
        (void)hipFree(h->bank_dev);
    }
    delete h;
}

}  // extern "C"
