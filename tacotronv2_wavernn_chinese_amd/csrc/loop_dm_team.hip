// Team kernel for the dual-softmax (coarse/fine) WaveRNN of wavernn/models/deepmind_version.py, generate() :75-165
// (SURVEY.md section 8a row A12).  The team protocol is team_common.h's: one team = the 32 workgroups of one XCD, fp32
// weights resident on chip, 8-byte {tag,value} granules exchanged through the XCD's L2, double-buffered by sample
// parity.  One sample = 6 exchanges:
//
//   R.h rows of the own hidden units (registers) -> coarse gates -> [h_c] -> O1 rows -> [t1] -> O2 rows + noise ->
//   [256 class values] -> argmax = coarse -> fine gates (need coarse) -> [h_f] -> O3 rows -> [t1] -> O4 rows + noise
//   -> [256 class values] -> argmax = fine
//
// Workgroup g owns hidden units {gU..gU+U-1} of each half (U = S/32; 14 for hidden_size 896), rows gU.. of O1/O3 and
// classes g*Q/32.. of O2/O4.  A quarter-wave (16 lanes) owns one hidden unit: its three R rows (u, r, e; H columns,
// H/16 per lane) live in VGPRs; the O slices live in LDS.  R(hidden) is evaluated once per sample with the hidden
// state of the previous sample, for both halves (:116-119), so the fine rows wait in registers until coarse is known.
// Sampling: Categorical(softmax(l)).sample() == argmax_k l_k - log q_k, q ~ Exp(1)  (as on the main path).
#include "dm_internal.h"
#include "team_common.h"

#define DMT_THREADS 512

namespace {

constexpr unsigned G_HC = 0, G_T1C = 1024, G_HF = 2048, G_T1F = 3072, G_C = 4096, G_F = 4608;   // x2 parities each

// A vector of N = 64*P floats in LDS, chunked for 16 lanes of P float4 each: element j (chunk q = j / (4P), float4 k
// inside the chunk, component e) -> plane k: [k][16 lanes][4].  Lane q reads its P float4 at stride 64 floats
// (conflict-free ds_read_b128); element j is written with one ds_write_b32.
template <int P>
__device__ __forceinline__ int chunk_idx(int j) { return ((j % (4 * P)) >> 2) * 64 + (j / (4 * P)) * 4 + (j & 3); }

// CPL = float4 per lane of an H-vector (H = 64 CPL); an S-vector (S = H/2) has CPL/2 per lane
template <int CPL>
__global__ void __launch_bounds__(DMT_THREADS, 2) dm_team_kernel(WrnnDmTeamArgs ta) {
    constexpr int H = 64 * CPL, S = H / 2, U = S / 32, PS = CPL / 2;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float *lds = (float *)smem;
    const WrnnDmArgs &a = ta.base;
    const int Q = a.Q, QW = Q / 32;
    // LDS carve-up (floats)
    float *hR = lds;                  // [2 parities][H]  hidden state in H-chunk order (input of R)
    float *hcS = hR + 2 * H;          // [S] new coarse half in S-chunk order (input of O1)
    float *hfS = hcS + S;             // [S] new fine half (input of O3)
    float *t1 = hfS + S;              // [S] relu(O1 / O3 output) (input of O2 / O4)
    float *misc = t1 + S;             // [128]: 0-2 team/rank/bail-out (team_common.h), 16-23 race partials, 32-95 sampling noise [parity][coarse 16 | fine 16]
    int *misc_i = (int *)misc;
    float *imgO1 = misc + 128, *imgO3 = imgO1 + U * S, *imgO2 = imgO3 + U * S, *imgO4 = imgO2 + QW * S;

    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int qw = tid >> 4, q = tid & 15;

    // ---- team formation (team_common.h): the grid covers every XCD, the first XCD to arrive is the team, the others leave at once ----
    int team, g;
    if (!join_team<true>(ta.ctl, ta.err, misc_i, 1, team, g) || team != 0) return;
    u64 *mail = ta.mail;
    const float *w = a.w;

    // ---- roles ----
    const bool isCq = qw < U, isFq = qw >= U && qw < 2 * U;
    const int hi = isCq ? g * U + qw : S + g * U + (qw - U);   // hidden index of this quarter-wave (valid if qw < 2U)
    const int orow = g * U + qw;                                // O1 / O3 row (valid if qw < U)
    const int cls = g * QW + qw;                                // O2 / O4 class (valid if qw < QW)

    // ---- resident weights ----
    float wR[3 * CPL * 4];
    {
        const float *src = ta.team_w + (size_t)g * (3 * CPL * 4) * DMT_THREADS + tid;
#pragma unroll
        for (int i = 0; i < 3 * CPL * 4; ++i) wR[i] = src[(size_t)i * DMT_THREADS];
        const int nimg = 2 * U * S + 2 * QW * S;
        const float4 *img = (const float4 *)(ta.team_lds + (size_t)g * nimg);
        float4 *dst = (float4 *)imgO1;
        for (int i = tid; i < nimg / 4; i += DMT_THREADS) dst[i] = img[i];
        for (int i = tid; i < 2 * H; i += DMT_THREADS) hR[i] = 0.0f;   // get_initial_hidden :168-170
    }
    float bu = 0.f, br = 0.f, be = 0.f, iw[9] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (qw < 2 * U) {
        bu = w[a.obu + hi]; br = w[a.obr + hi]; be = w[a.obe + hi];
        if (isCq) {
            const float *Ic = w + a.oIc;
            const int j = hi;
            iw[0] = Ic[j * 2]; iw[1] = Ic[j * 2 + 1]; iw[3] = Ic[(S + j) * 2]; iw[4] = Ic[(S + j) * 2 + 1];
            iw[6] = Ic[(2 * S + j) * 2]; iw[7] = Ic[(2 * S + j) * 2 + 1];
        } else {
            const float *If = w + a.oIf;
            const int j = hi - S;
#pragma unroll
            for (int c = 0; c < 3; ++c) { iw[c] = If[j * 3 + c]; iw[3 + c] = If[(S + j) * 3 + c]; iw[6 + c] = If[(2 * S + j) * 3 + c]; }
        }
    }
    const float bO1 = isCq ? w[a.oO1b + orow] : 0.f, bO3 = isCq ? w[a.oO3b + orow] : 0.f;
    const float bO2 = qw < QW ? w[a.oO2b + cls] : 0.f, bO4 = qw < QW ? w[a.oO4b + cls] : 0.f;
    __syncthreads();

    // -log q for the workgroup's QW classes of both softmaxes of sample ts, drawn one sample ahead by the otherwise
    // idle last wave (lanes 0..QW-1 coarse, 16..16+QW-1 fine) -> misc[32 + 32 * parity(ts) + lane]
    auto draw = [&](long ts) {
        if (wave != 7 || ts >= a.seq_len) return;
        const unsigned which = (unsigned)(lane >> 4) & 1u;
        const int c = lane & 15;
        if (lane >= 32 || c >= QW) return;
        const int k = g * QW + c;
        float nz = 0.f;
        if (a.noise_mode == WRNN_NOISE_INJECTED) nz = -logf(a.noise[((size_t)ts * 2 + which) * Q + k]);
        else if (a.noise_mode == WRNN_NOISE_PHILOX) nz = -logf(-logf(wrnn_uniform(a.seed, (uint64_t)ts, which, (uint32_t)k)));
        misc[32 + 32 * (int)((ts + 1) & 1) + lane] = nz;
    };
    // dot of an LDS-resident row (image [P planes][16 lanes] float4 per quarter-wave row) with an S-vector
    auto dotS = [&](const float *img, int row_in_wg, const float *vec) -> float {
        const float4 *wp = (const float4 *)img + (size_t)row_in_wg * PS * 16 + q;
        const float4 *xp = (const float4 *)vec + q;
        float s0 = 0.f, s1 = 0.f;
#pragma unroll
        for (int k = 0; k < PS; ++k) {
            const float4 ww = wp[k * 16], xx = xp[k * 16];
            s0 = fmaf(ww.x, xx.x, s0); s1 = fmaf(ww.y, xx.y, s1);
            s0 = fmaf(ww.z, xx.z, s0); s1 = fmaf(ww.w, xx.w, s1);
        }
        return row_sum(s0 + s1);
    };
    // argmax over the Q published class values (one granule per thread of the first Q/64 waves), ties -> lowest index
    auto race = [&](unsigned region, unsigned par, unsigned epoch, bool &dead) -> int {
        if (wave < Q / 64) {
            const float v = take_staggered(mail, region + par * 256 + tid, epoch, dead, ta.err, 21u);
            const float mx = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(wave_max(v)), 63));
            const u64 ball = __ballot(v == mx);
            const int src = (int)__builtin_ctzll(ball ? ball : 1ull);
            if (lane == 0) { misc[16 + 2 * wave] = mx; misc_i[17 + 2 * wave] = wave * 64 + src; }
        }
        __syncthreads();
        float bv = misc[16];
        int bi = misc_i[17];
        for (int i = 1; i < Q / 64; ++i) {
            const float v = misc[16 + 2 * i];
            if (v > bv) { bv = v; bi = misc_i[17 + 2 * i]; }
        }
        return bi;
    };

    // R(hidden) rows u, r, e of the own hidden unit (:116-119): evaluated as soon as the hidden state of a sample is
    // complete (after the fine half was exchanged), i.e. under the O3 / O4 phases, for the NEXT sample
    float ru = 0.f, rr = 0.f, re = 0.f;
    auto r_rows = [&](const float *hin) {
        const float4 *xp = (const float4 *)hin + q;
        float a0 = 0.f, a1 = 0.f, b0 = 0.f, b1 = 0.f, c0 = 0.f, c1 = 0.f;
#pragma unroll
        for (int k = 0; k < CPL; ++k) {
            const float4 x = xp[k * 16];
            a0 = fmaf(wR[4 * k + 0], x.x, a0); a1 = fmaf(wR[4 * k + 1], x.y, a1);
            b0 = fmaf(wR[CPL * 4 + 4 * k + 0], x.x, b0); b1 = fmaf(wR[CPL * 4 + 4 * k + 1], x.y, b1);
            c0 = fmaf(wR[CPL * 8 + 4 * k + 0], x.x, c0); c1 = fmaf(wR[CPL * 8 + 4 * k + 1], x.y, c1);
            a0 = fmaf(wR[4 * k + 2], x.z, a0); a1 = fmaf(wR[4 * k + 3], x.w, a1);
            b0 = fmaf(wR[CPL * 4 + 4 * k + 2], x.z, b0); b1 = fmaf(wR[CPL * 4 + 4 * k + 3], x.w, b1);
            c0 = fmaf(wR[CPL * 8 + 4 * k + 2], x.z, c0); c1 = fmaf(wR[CPL * 8 + 4 * k + 3], x.w, c1);
        }
        ru = row_sum(a0 + a1); rr = row_sum(b0 + b1); re = row_sum(c0 + c1);
    };

    bool dead = false;
    int oc = 0, of = 0;                      // out_coarse = out_fine = 0 :90-91
    float hown = 0.0f;                       // this quarter-wave's hidden unit
    draw(0);
    __syncthreads();
    for (long t = 0; t < a.seq_len; ++t) {
        const unsigned epoch = (unsigned)t + 1u, par = epoch & 1u;
        float *hout = hR + par * H;
        const float pc = (float)oc / 127.5f - 1.0f, pf = (float)of / 127.5f - 1.0f;   // :106-107
        draw(t + 1);

        // ---- coarse gates :111-125 ----
        if (isCq) {
            const float Iu = iw[0] * pc + iw[1] * pf, Ir = iw[3] * pc + iw[4] * pf, Ie = iw[6] * pc + iw[7] * pf;
            const float u = sigmoid_fast(ru + Iu + bu);
            const float r = sigmoid_fast(rr + Ir + br);
            const float e = tanh_fast(r * re + Ie + be);
            hown = u * hown + (1.0f - u) * e;
            if (q == 0) st_granule(mail, G_HC + par * 512 + hi, epoch, __float_as_uint(hown));
        }
        // ---- exchange 1: new coarse half ----
        if (wave < S / 64) {
            const float v = take_staggered(mail, G_HC + par * 512 + tid, epoch, dead, ta.err, 11u);
            hout[chunk_idx<CPL>(tid)] = v;
            hcS[chunk_idx<PS>(tid)] = v;
        }
        __syncthreads();
        // ---- out_coarse = O2(relu(O1(hidden_coarse))) :128 ----
        if (isCq) {
            const float s = dotS(imgO1, qw, hcS) + bO1;
            if (q == 0) st_granule(mail, G_T1C + par * 512 + orow, epoch, __float_as_uint(fmaxf(s, 0.0f)));
        }
        if (wave < S / 64) t1[chunk_idx<PS>(tid)] = take_staggered(mail, G_T1C + par * 512 + tid, epoch, dead, ta.err, 12u);
        __syncthreads();
        if (qw < QW) {
            const float s = dotS(imgO2, qw, t1) + bO2 + misc[32 + 32 * par + qw];
            if (q == 0) st_granule(mail, G_C + par * 256 + cls, epoch, __float_as_uint(s));
        }
        oc = race(G_C, par, epoch, dead);                                   // Categorical(...).sample() :130-131
        if (g == 0 && tid == 0) a.coarse[t] = oc;
        const float cp = (float)oc / 127.5f - 1.0f;                         // :135
        // ---- fine gates :136-145 ----
        if (isFq) {
            const float Iu = iw[0] * pc + iw[1] * pf + iw[2] * cp;
            const float Ir = iw[3] * pc + iw[4] * pf + iw[5] * cp;
            const float Ie = iw[6] * pc + iw[7] * pf + iw[8] * cp;
            const float u = sigmoid_fast(ru + Iu + bu);
            const float r = sigmoid_fast(rr + Ir + br);
            const float e = tanh_fast(r * re + Ie + be);
            hown = u * hown + (1.0f - u) * e;
            if (q == 0) st_granule(mail, G_HF + par * 512 + (hi - S), epoch, __float_as_uint(hown));
        }
        if (wave < S / 64) {
            const float v = take_staggered(mail, G_HF + par * 512 + tid, epoch, dead, ta.err, 13u);
            hout[chunk_idx<CPL>(S + tid)] = v;
            hfS[chunk_idx<PS>(tid)] = v;
        }
        __syncthreads();
        if (isFq) r_rows(hout);   // idle from here on: R.h of the next sample now
        // ---- out_fine = O4(relu(O3(hidden_fine))) :148 ----
        if (isCq) {
            const float s = dotS(imgO3, qw, hfS) + bO3;
            if (q == 0) st_granule(mail, G_T1F + par * 512 + orow, epoch, __float_as_uint(fmaxf(s, 0.0f)));
            r_rows(hout);         // under the t1 exchange
        }
        if (wave < S / 64) t1[chunk_idx<PS>(tid)] = take_staggered(mail, G_T1F + par * 512 + tid, epoch, dead, ta.err, 14u);
        __syncthreads();
        if (qw < QW) {
            const float s = dotS(imgO4, qw, t1) + bO4 + misc[32 + 32 * par + 16 + qw];
            if (q == 0) st_granule(mail, G_F + par * 256 + cls, epoch, __float_as_uint(s));
        }
        of = race(G_F, par, epoch, dead);                                   // :150-151
        if (g == 0 && tid == 0) a.fine[t] = of;
        if ((t & 63) == 63) {   // bounded-spin bail-out, checked workgroup-wide every 64 samples
            if (dead && lane == 0) misc_i[M_DEAD] = 1;
            __syncthreads();
            if (misc_i[M_DEAD]) return;
        }
    }
}

template <int CPL>
hipError_t launch_cpl(const WrnnDmTeamArgs &a, hipStream_t s) {
    const int H = 64 * CPL, S = H / 2, U = S / 32, QW = a.base.Q / 32;
    const size_t lds = (size_t)(2 * H + 3 * S + 128 + 2 * U * S + 2 * QW * S) * sizeof(float);
    hipError_t e = hipFuncSetAttribute((const void *)dm_team_kernel<CPL>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL((dm_team_kernel<CPL>), dim3(256), dim3(DMT_THREADS), lds, s, a);
    return hipGetLastError();
}

}  // namespace

// hidden_size in {512, 640, 768, 896}: H/128 integral (float4 chunks of both vector kinds), 3*H/16 <= 168 weight
// registers per lane; quantisation a multiple of 64 up to 256 (one class value per thread of the first Q/64 waves,
// Q/32 class rows per workgroup)
bool wrnn_dm_team_supported(int H, int Q) {
    return (H == 512 || H == 640 || H == 768 || H == 896) && Q >= 64 && Q <= 256 && Q % 64 == 0;
}

hipError_t wrnn_launch_dm_team(const WrnnDmTeamArgs &a, hipStream_t s) {
    (void)hipGetLastError();
    switch (a.base.H) {
        case 512: return launch_cpl<8>(a, s);
        case 640: return launch_cpl<10>(a, s);
        case 768: return launch_cpl<12>(a, s);
        case 896: return launch_cpl<14>(a, s);
        default: return hipErrorInvalidValue;
    }
}
