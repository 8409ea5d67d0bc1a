// WRNN_KERNEL_TEAMG: the per-sample loop of WaveRNN.generate (wavernn/models/fatchord_version.py:194-241) for ANY constructor
// dims, one row per XCD team.  The team protocol is team_common.h's: one team = the 32 workgroups of one XCD (formed by
// HW_REG_XCC_ID, co-residency checked at the start), 8-byte {tag, value} granules exchanged through the XCD's L2,
// double-buffered by step parity, every spin bounded (device error word, `dead`: all waves run to the end).  What is new is that
// nothing is a compile-time shape: the layer sizes arrive in WrnnTeamGPlan.
//
// Ownership.  Every layer is a list of units -- a hidden unit with its three gate rows (rnn1, rnn2) or one output row (I, fc1, fc2,
// fc3).  Workgroup g owns units [g U, min(N, (g + 1) U)) of a layer of N units, U = ceil(N / 32): possibly none (rnn 100: U = 4, the
// last seven workgroups own no hidden unit), and it still takes part in every exchange.  A 16-lane group (one DPP row) evaluates one
// unit: a row is K floats padded to a multiple of 64, lane q reads float4 q, q + 16, ... of the row and of the activation vector,
// the 16 partial sums are added with row_sum's DPP steps.  Where a workgroup owns 16 or fewer hidden units a group takes one gate
// row of a unit instead (gru_phase).
//
// Placement.  A workgroup's slice of the weights is one contiguous image in device memory (wrnn_teamg_pack); the first `nres` units
// of every layer are copied to LDS at the start of a launch and stay there, the rest is read every step from L2 / Infinity Cache with
// the same 16-byte loads.  Weights are read-only during a launch: plain loads.  wrnn_teamg_make_plan decides nres.
//
// Element type.  The kernel is templated on the type of the image's elements: float, or _Float16 (WRNN_WEIGHTS_F16) --
// half the bytes streamed, twice the units resident, rows permuted at pack time so that a lane's 16-byte load brings the weights of two
// steps (teamg_layout.h).  Only the six matrices change type; activations, sums, biases, W_I[:, 0], cells and samplers are fp32, and
// since a binary16 widens exactly and the multiply-adds keep their order, the outputs are those of the fp32 instantiation on the model
// with its matrices rounded to fp16.  TgE4m3 (WRNN_WEIGHTS_E4M3): OCP e4m3fn bytes with one power-of-two scale per layer,
// a quarter of the bytes, rows permuted so that a 16-byte load brings the weights of four steps; a row's segment sums are multiplied by
// the layer's scale, which commutes with every rounding: the outputs are the fp32 instantiation's on the dequantised model.
//
// One step = five exchanges on the serial chain plus one beside it:
//   [xc]  the conditioning's share of I, W_I[:, 1:] . [m_t | a1_t] + b_I, for step t + 1 -- published under exchange 2 of step t
//   x = xc + W_I[:, 0] x_{t-1}                                                             :208-209 (every workgroup, all H)
//   1. h1' of the own units from [W_ih1 | W_hh1] . [x | h1]          -> [h1']  x2 = x + h1'  :210-212
//   2. h2' from [W_ih2 | W_hh2] . [x2 | a2_t | h2]                   -> [h2']  x3 = x2 + h2' :213-216
//   3. relu(fc1 . [x3 | a3_t])                                       -> [fc1]                :217-218
//   4. relu(fc2 . [fc1 | a4_t])                                      -> [fc2]                :220-221
//   5. fc3 rows of the own classes; RAW: + noise, race inside the workgroup, -> [32 candidates (value, class)], every workgroup
//      picks the winner; MOL: -> [30 outputs], every workgroup runs the sampler                :223-237
#include <cstring>
#include <type_traits>

#include "team_common.h"
#include "teamg_layout.h"

namespace {

// G rows of one unit against one activation vector: wp = the unit's first row + lane q (float4), rows kp4 float4 apart; xp = the
// vector + q.  Segment A = float4 steps [0, nA), segment B = [nA, nK): sa / sb are their sums (the n gate of a GRU needs them apart)
template <int G>
__device__ __forceinline__ void tg_dot(const float4 *__restrict__ wp, int kp4, const float4 *xp, int nA, int nK, float (&sa)[G], float (&sb)[G]) {
    float a0[G], a1[G];
#pragma unroll
    for (int g = 0; g < G; ++g) a0[g] = a1[g] = 0.0f;
#pragma unroll 4
    for (int k = 0; k < nA; ++k) {
        const float4 x = xp[k * 16];
#pragma unroll
        for (int g = 0; g < G; ++g) {
            const float4 w = wp[(size_t)g * kp4 + k * 16];
            a0[g] = fmaf(w.x, x.x, a0[g]); a1[g] = fmaf(w.y, x.y, a1[g]);
            a0[g] = fmaf(w.z, x.z, a0[g]); a1[g] = fmaf(w.w, x.w, a1[g]);
        }
    }
#pragma unroll
    for (int g = 0; g < G; ++g) { sa[g] = row_sum(a0[g] + a1[g]); a0[g] = a1[g] = 0.0f; }
#pragma unroll 4
    for (int k = nA; k < nK; ++k) {
        const float4 x = xp[k * 16];
#pragma unroll
        for (int g = 0; g < G; ++g) {
            const float4 w = wp[(size_t)g * kp4 + k * 16];
            a0[g] = fmaf(w.x, x.x, a0[g]); a1[g] = fmaf(w.y, x.y, a1[g]);
            a0[g] = fmaf(w.z, x.z, a0[g]); a1[g] = fmaf(w.w, x.w, a1[g]);
        }
    }
#pragma unroll
    for (int g = 0; g < G; ++g) sb[g] = row_sum(a0[g] + a1[g]);
}

// tg_dot on the fp16 image (teamg_layout.h): rp = the unit's first row, rows kp8 16-byte pieces apart, row0 its index in the slice.  One
// 16-byte load per row and PAIR of steps, four pairs issued together -- tg_dot's bytes in flight --, an 8-byte load for the unpaired last step
// of a segment; per step the same four weights, widened exactly, into the same a0 / a1 chains in the same order.
template <int G>
__device__ __forceinline__ void tg_dot16(const TgHalf8 *__restrict__ rp, int kp8, int row0, int q, const float4 *xp, int nA, int nK, float (&sa)[G],
                                         float (&sb)[G]) {
    const TgHalf8 *wp[G];
#pragma unroll
    for (int g = 0; g < G; ++g) wp[g] = rp + (size_t)g * kp8 + (q ^ tg16_swz(row0 + g, kp8 * 8));
    float a0[G], a1[G];
#pragma unroll
    for (int g = 0; g < G; ++g) a0[g] = a1[g] = 0.0f;
    auto mac = [&](int g, const float4 &w, const float4 &x) {
        a0[g] = fmaf(w.x, x.x, a0[g]); a1[g] = fmaf(w.y, x.y, a1[g]);
        a0[g] = fmaf(w.z, x.z, a0[g]); a1[g] = fmaf(w.w, x.w, a1[g]);
    };
    // NP pairs of steps from step k: their weight loads are issued together
    auto block = [&](auto np, int k) {
        constexpr int NP = decltype(np)::value;
        TgHalf8 w[NP][G];
#pragma unroll
        for (int u = 0; u < NP; ++u)
#pragma unroll
            for (int g = 0; g < G; ++g) w[u][g] = wp[g][(k + 2 * u) * 8];
#pragma unroll
        for (int u = 0; u < NP; ++u) {
            const float4 x0 = xp[(k + 2 * u) * 16], x1 = xp[(k + 2 * u + 1) * 16];
#pragma unroll
            for (int g = 0; g < G; ++g) {
                mac(g, tg_lo4(w[u][g]), x0);
                mac(g, tg_hi4(w[u][g]), x1);
            }
        }
    };
    // four pairs at a time, then what is left as one block of two and one of one: a short segment (4 steps at rnn_dims 256) still has
    // all its loads in flight at once, as tg_dot's unrolled loop has them
    auto segment = [&](int k0, int k1) {
        int k = k0;
#pragma unroll 1
        for (; k + 8 <= k1; k += 8) block(std::integral_constant<int, 4>{}, k);
        if (k + 4 <= k1) { block(std::integral_constant<int, 2>{}, k); k += 4; }
        if (k + 2 <= k1) { block(std::integral_constant<int, 1>{}, k); k += 2; }
        if (k < k1) {
            const float4 x = xp[k * 16];
#pragma unroll
            for (int g = 0; g < G; ++g) mac(g, tg_w4(((const TgHalf4 *)(rp + (size_t)g * kp8))[k * 16 + q]), x);
        }
    };
    segment(0, nA);
#pragma unroll
    for (int g = 0; g < G; ++g) { sa[g] = row_sum(a0[g] + a1[g]); a0[g] = a1[g] = 0.0f; }
    segment(nA, nK);
#pragma unroll
    for (int g = 0; g < G; ++g) sb[g] = row_sum(a0[g] + a1[g]);
}

// tg_dot on the e4m3 image (teamg_layout.h): rp = the unit's first row, rows KP bytes apart, row0 its index in the slice.  One 16-byte load
// per row and QUAD of steps, a block of four quads issued together -- tg_dot's bytes in flight; two for a unit of three rows --; what is left
// of a segment (less than a block: quads, an
// 8-byte pair, a 4-byte single step) is loaded together before any of it is used, so a short segment has all its loads in flight at once.
// Per step the same four weights, widened exactly (two v_cvt_pk_f32_fp8), into the same a0 / a1 chains in the same order.  The sums are
// those of the stored bytes: the caller applies the layer's scale.
template <int G>
__device__ __forceinline__ void tg_dot8(const unsigned char *__restrict__ rp, int KP, int row0, int q, const float4 *xp, int nA, int nK, float (&sa)[G],
                                        float (&sb)[G]) {
    constexpr int NB = G == 1 ? 4 : 2;   // quads of a block: 64 bytes per lane in flight for a row, 2 x 3 x 16 for a unit (the registers' limit)
    const uint4 *wq[G];
#pragma unroll
    for (int g = 0; g < G; ++g) wq[g] = (const uint4 *)(rp + (size_t)g * KP) + ((q + tg8_rot(row0 + g, KP)) & 15);
    float a0[G], a1[G];
#pragma unroll
    for (int g = 0; g < G; ++g) a0[g] = a1[g] = 0.0f;
    auto mac = [&](int g, const float4 &w, const float4 &x) {
        a0[g] = fmaf(w.x, x.x, a0[g]); a1[g] = fmaf(w.y, x.y, a1[g]);
        a0[g] = fmaf(w.z, x.z, a0[g]); a1[g] = fmaf(w.w, x.w, a1[g]);
    };
    // the four steps of a quad from step k
    auto quad = [&](const uint4 (&w)[G], int k) {
        // two steps at a time, as tg_dot16 has them: the activation reads and the widened weights of a whole block, scheduled early,
        // would not fit the registers
        const float4 x0 = xp[k * 16], x1 = xp[(k + 1) * 16];
#pragma unroll
        for (int g = 0; g < G; ++g) { mac(g, tg8_w4(w[g].x), x0); mac(g, tg8_w4(w[g].y), x1); }
        __builtin_amdgcn_sched_barrier(0);
        const float4 x2 = xp[(k + 2) * 16], x3 = xp[(k + 3) * 16];
#pragma unroll
        for (int g = 0; g < G; ++g) { mac(g, tg8_w4(w[g].z), x2); mac(g, tg8_w4(w[g].w), x3); }
        __builtin_amdgcn_sched_barrier(0);
    };
    auto segment = [&](int k0, int k1) {
        int k = k0;
#pragma unroll 1
        for (; k + 4 * NB <= k1; k += 4 * NB) {
            uint4 w[NB][G];
#pragma unroll
            for (int u = 0; u < NB; ++u)
#pragma unroll
                for (int g = 0; g < G; ++g) w[u][g] = wq[g][(k + 4 * u) * 4];
#pragma unroll
            for (int u = 0; u < NB; ++u) quad(w[u], k + 4 * u);
        }
        // less than a block left: every load of it first
        const int rem = k1 - k, nq = rem >> 2, kp = k + 4 * nq, ks = kp + (rem & 2);
        uint4 w[NB - 1][G];
        uint2 wp[G];
        unsigned ws[G];
#pragma unroll
        for (int u = 0; u < NB - 1; ++u)
            if (u < nq) {
#pragma unroll
                for (int g = 0; g < G; ++g) w[u][g] = wq[g][(k + 4 * u) * 4];
            }
        if (rem & 2) {
#pragma unroll
            for (int g = 0; g < G; ++g) wp[g] = ((const uint2 *)(rp + (size_t)g * KP + 64 * kp))[q];
        }
        if (rem & 1) {
#pragma unroll
            for (int g = 0; g < G; ++g) ws[g] = ((const unsigned *)(rp + (size_t)g * KP + 64 * ks))[q];
        }
#pragma unroll
        for (int u = 0; u < NB - 1; ++u)
            if (u < nq) quad(w[u], k + 4 * u);
        if (rem & 2) {
            const float4 x0 = xp[kp * 16], x1 = xp[(kp + 1) * 16];
#pragma unroll
            for (int g = 0; g < G; ++g) { mac(g, tg8_w4(wp[g].x), x0); mac(g, tg8_w4(wp[g].y), x1); }
        }
        if (rem & 1) {
            const float4 x = xp[ks * 16];
#pragma unroll
            for (int g = 0; g < G; ++g) mac(g, tg8_w4(ws[g]), x);
        }
    };
    segment(0, nA);
#pragma unroll
    for (int g = 0; g < G; ++g) { sa[g] = row_sum(a0[g] + a1[g]); a0[g] = a1[g] = 0.0f; }
    segment(nA, nK);
#pragma unroll
    for (int g = 0; g < G; ++g) sb[g] = row_sum(a0[g] + a1[g]);
}

// tg_dot on the block-sparse image (WrnnTeamGSparse): rp = the unit's first image row, rows `rs` floats apart, each [nK 16-bit block
// indices, padded to 16 bytes][nK blocks of 64 floats].  List entry j stands for step idx[j] of the dense row: x = xp[idx * 16], w = block
// j's float4 q -- the four multiply-adds of that step into the same a0 / a1 chains.  A list ascends inside a segment (entries [0, nA) and
// [nA, nK)) and leaves out only steps whose 64 weights are zero, which change no chain (fmaf(0, x, a) == a for finite x); the zero blocks
// that pad a short list change none either.  Every row has its own list.  The indices and the weights of four entries are loaded together,
// then the activation reads, whose addresses wait for the indices: tg_dot's weight bytes in flight.
template <int G>
__device__ __forceinline__ void tg_dots(const float *__restrict__ rp, int rs, int q, const float4 *xp, int nA, int nK, float (&sa)[G], float (&sb)[G]) {
    const int idxf = (nK + 7) / 8 * 4;   // wrnn_teamg_sparse_idx_elems
    const unsigned short *ip[G];
    const float4 *wp[G];
#pragma unroll
    for (int g = 0; g < G; ++g) {
        ip[g] = (const unsigned short *)(rp + (size_t)g * rs);
        wp[g] = (const float4 *)(rp + (size_t)g * rs + idxf) + q;
    }
    float a0[G], a1[G];
#pragma unroll
    for (int g = 0; g < G; ++g) a0[g] = a1[g] = 0.0f;
    auto block = [&](auto nu, int j) {
        constexpr int NU = decltype(nu)::value;
        int id[NU][G];
        float4 w[NU][G];
#pragma unroll
        for (int u = 0; u < NU; ++u)
#pragma unroll
            for (int g = 0; g < G; ++g) id[u][g] = ip[g][j + u];
#pragma unroll
        for (int u = 0; u < NU; ++u)
#pragma unroll
            for (int g = 0; g < G; ++g) w[u][g] = wp[g][(j + u) * 16];
#pragma unroll
        for (int u = 0; u < NU; ++u)
#pragma unroll
            for (int g = 0; g < G; ++g) {
                const float4 x = xp[id[u][g] * 16];
                a0[g] = fmaf(w[u][g].x, x.x, a0[g]); a1[g] = fmaf(w[u][g].y, x.y, a1[g]);
                a0[g] = fmaf(w[u][g].z, x.z, a0[g]); a1[g] = fmaf(w[u][g].w, x.w, a1[g]);
            }
    };
    auto segment = [&](int j0, int j1) {
        int j = j0;
#pragma unroll 1
        for (; j + 4 <= j1; j += 4) block(std::integral_constant<int, 4>{}, j);
        if (j + 2 <= j1) { block(std::integral_constant<int, 2>{}, j); j += 2; }
        if (j < j1) block(std::integral_constant<int, 1>{}, j);
    };
    segment(0, nA);
#pragma unroll
    for (int g = 0; g < G; ++g) { sa[g] = row_sum(a0[g] + a1[g]); a0[g] = a1[g] = 0.0f; }
    segment(nA, nK);
#pragma unroll
    for (int g = 0; g < G; ++g) sb[g] = row_sum(a0[g] + a1[g]);
}

// G rows from row `row0` of a layer's slice at `base` (LDS or device memory), KP elements each, in the image's element type; `scale` is the
// layer's (e4m3 only: a power of two, so scaling the two sums equals scaling every weight).  TgSparse: KP = the floats of an image row,
// nA / nK count list entries
template <int G, typename WT>
__device__ __forceinline__ void tg_rows(const WT *base, int row0, int KP, float scale, int q, const float4 *xp, int nA, int nK, float (&sa)[G], float (&sb)[G]) {
    if constexpr (std::is_same<WT, TgSparse>::value) tg_dots<G>((const float *)base + (size_t)row0 * KP, KP, q, xp, nA, nK, sa, sb);
    else if constexpr (sizeof(WT) == 4) tg_dot<G>((const float4 *)(base + (size_t)row0 * KP) + q, KP / 4, xp, nA, nK, sa, sb);
    else if constexpr (sizeof(WT) == 2) tg_dot16<G>((const TgHalf8 *)(base + (size_t)row0 * KP), KP / 8, row0, q, xp, nA, nK, sa, sb);
    else {
        tg_dot8<G>((const unsigned char *)(base + (size_t)row0 * KP), KP, row0, q, xp, nA, nK, sa, sb);
#pragma unroll
        for (int g = 0; g < G; ++g) { sa[g] *= scale; sb[g] *= scale; }
    }
}

template <typename WT>
__global__ void __launch_bounds__(TG_THREADS) loop_teamg_kernel(WrnnTeamGArgs ta) {
    extern __shared__ __attribute__((aligned(16))) char smem_tg[];
    float *lds = (float *)smem_tg;
    const WrnnLoopArgs &a = ta.a;
    const WrnnDims d = a.d;
    const TgLay ly(d);
    const int H = d.H, FC = d.FC, F = d.F, A = d.A, R = d.R, NC = d.NC, HOP = d.HOP, ND = d.ND, P = d.P;
    const int HP = ly.HP, XAP = ly.XAP, FCP = ly.FCP;
    float *misc = lds + ly.misc;
    int *misc_i = (int *)misc;
    float *f1 = lds + ly.f1, *f2 = lds + ly.f2, *f3 = lds + ly.f3;
    WT *wres = (WT *)(lds + ly.total);   // resident weights, in the image's element type
    constexpr bool SP = std::is_same<WT, TgSparse>::value;   // the block-sparse image: a layer's steps are its list entries

    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int qw = tid >> 4, q = tid & 15;

    // ---- team formation (team_common.h) ----
    int team, g;
    if (!join_team(ta.ctl, a.err, misc_i, ta.n_teams, team, g) || team >= a.n_rows) return;
    u64 *mail = ta.mail + (size_t)team * ta.plan.mail_granules;
    // mailbox regions (granules), two parities each
    const unsigned M_XC = 0, M_H1 = 2 * HP, M_H2 = 4 * HP, M_F1 = 6 * HP, M_F2 = 6 * HP + 2 * FCP, M_CAND = 6 * HP + 4 * FCP;
    const float *w = a.w;
    const WT *img = (const WT *)ta.img + (size_t)g * ta.plan.img_elems_wg;

    // ---- resident weights, zeroed activations ----
    for (int l = 0; l < WRNN_TEAMG_LAYERS; ++l) {
        const WrnnTeamGLayer &L = ta.plan.L[l];
        const int n4 = L.nres * L.G * (L.KP / 4) / (int)(sizeof(float) / sizeof(WT));   // 16-byte pieces: KP is a multiple of 64 elements
        const float4 *src = (const float4 *)(img + L.img_off);
        float4 *dst = (float4 *)(wres + L.lds_off);
        for (int i = tid; i < n4; i += TG_THREADS) dst[i] = src[i];
    }
    for (int i = tid; i < ly.misc; i += TG_THREADS) lds[i] = 0.0f;
    __syncthreads();

    // units of layer l this workgroup owns
    auto owned = [&](const WrnnTeamGLayer &L) -> int {
        int n = L.N - g * L.U;
        return n < 0 ? 0 : (n > L.U ? L.U : n);
    };
    // m_t, a_t of step t of the row (:203-206), as loop_simple.hip: zero conditioning past the row's own utterance (:327-330)
    auto cond_fill = [&](const WrnnRow &rw, int64_t t, float *dst) {
        const float *mel_b = a.mels + (size_t)rw.utt * F * a.mel_T;
        const float *aux_b = a.aux_frames + (size_t)rw.utt * a.T * R;
        const float *ktab = w + a.off.ktab;
        const int64_t pos = rw.start + t;
        const bool live = a.frames ? pos < (int64_t)a.frames[rw.utt] * HOP && pos < a.total_len : pos < a.total_len;
        const int i = live ? (int)(pos / HOP) : 0;
        const int r = live ? (int)(pos - (int64_t)i * HOP) : 0;
        for (int j = tid; j < F + R; j += TG_THREADS) {
            float v = 0.0f;
            if (live) {
                if (j < F) {
                    for (int k = 0; k < ND; ++k) {
                        const int fr = i + k - P + a.mel_off;
                        const float mv = (fr >= 0 && fr < a.mel_T) ? mel_b[(size_t)j * a.mel_T + fr] : 0.0f;
                        v = fmaf(ktab[r * ND + k], mv, v);
                    }
                } else {
                    v = aux_b[(size_t)i * R + (j - F)];
                }
            }
            dst[j] = v;
        }
    };
    // the own rows of W_I[:, 1:] . [m | a1] + b_I for the step whose conditioning is in cbuf -> mailbox, tagged `tag`
    auto xc_publish = [&](const float *cbuf, unsigned tag) {
        const WrnnTeamGLayer &L = ta.plan.L[WRNN_TEAMG_COND];
        const int nown = owned(L), nK = SP ? tg_sp_nk(ta.plan, ta.sp, L) : L.KP / 64;
        for (int ul = qw; ul < nown; ul += 32) {
            float sa[1], sb[1];
            if (ul < L.nres) tg_rows<1>(wres + L.lds_off, ul, L.KP, L.scale, q, (const float4 *)cbuf + q, nK, nK, sa, sb);
            else tg_rows<1>(img + L.img_off, ul, L.KP, L.scale, q, (const float4 *)cbuf + q, nK, nK, sa, sb);
            const int j = g * L.U + ul;
            if (q == 0) tg_st_granule<WT>(mail, M_XC + (tag & 1u) * HP + j, tag, __float_as_uint(sa[0] + w[a.off.I_b + j]));
        }
    };
    // one GRU layer (get_gru_cell :273-279, gate rows [r; z; n]): h' of the own units -> mailbox.  xin = [input (KAP) | h (HP)]
    // With 16 or fewer units per workgroup (rnn_dims <= 512) a unit per 16-lane group would leave half the groups, and their loads in
    // flight, idle: then a group takes one gate ROW, the sums meet in LDS and one lane per unit finishes the cell.  Same sums either way.
    auto gru_phase = [&](const WrnnTeamGLayer &L, const float *xin, size_t obih, size_t obhh, unsigned region, unsigned epoch) {
        const int nown = owned(L), nA = SP ? tg_sp_na(ta.plan, ta.sp, L) : L.KAP / 64, nK = SP ? tg_sp_nk(ta.plan, ta.sp, L) : L.KP / 64;
        const bool by_row = L.U <= 16;
        if (by_row) {
            float *gs = lds + ly.gs;
            for (int task = qw; task < 3 * nown; task += 32) {
                const int ul = task / 3;
                float sa[1], sb[1];
                if (ul < L.nres) tg_rows<1>(wres + L.lds_off, task, L.KP, L.scale, q, (const float4 *)xin + q, nA, nK, sa, sb);
                else tg_rows<1>(img + L.img_off, task, L.KP, L.scale, q, (const float4 *)xin + q, nA, nK, sa, sb);
                if (q == 0) { gs[2 * task] = sa[0]; gs[2 * task + 1] = sb[0]; }
            }
            __syncthreads();
        }
        for (int ul = by_row ? tid : qw; ul < nown; ul += by_row ? TG_THREADS : 32) {
            float gi[3], gh[3];
            if (by_row) {
                const float *gs = lds + ly.gs + 6 * ul;
                gi[0] = gs[0]; gh[0] = gs[1]; gi[1] = gs[2]; gh[1] = gs[3]; gi[2] = gs[4]; gh[2] = gs[5];
            } else if (ul < L.nres) tg_rows<3>(wres + L.lds_off, ul * 3, L.KP, L.scale, q, (const float4 *)xin + q, nA, nK, gi, gh);
            else tg_rows<3>(img + L.img_off, ul * 3, L.KP, L.scale, q, (const float4 *)xin + q, nA, nK, gi, gh);
            const int j = g * L.U + ul;
            const float *bi = w + obih, *bh = w + obhh;
            const float rg = 1.0f / (1.0f + expf(-((gi[0] + bi[j]) + (gh[0] + bh[j]))));
            const float zg = 1.0f / (1.0f + expf(-((gi[1] + bi[H + j]) + (gh[1] + bh[H + j]))));
            const float ng = tanhf((gi[2] + bi[2 * H + j]) + rg * (gh[2] + bh[2 * H + j]));
            const float hn = (1.0f - zg) * ng + zg * xin[L.KAP + j];
            if (by_row || q == 0) tg_st_granule<WT>(mail, region + (epoch & 1u) * HP + j, epoch, __float_as_uint(hn));
        }
    };
    // relu(W . x + b) of the own rows -> mailbox
    auto fc_phase = [&](const WrnnTeamGLayer &L, const float *xin, size_t ob, unsigned region, unsigned epoch) {
        const int nown = owned(L), nK = SP ? tg_sp_nk(ta.plan, ta.sp, L) : L.KP / 64;
        for (int ul = qw; ul < nown; ul += 32) {
            float sa[1], sb[1];
            if (ul < L.nres) tg_rows<1>(wres + L.lds_off, ul, L.KP, L.scale, q, (const float4 *)xin + q, nK, nK, sa, sb);
            else tg_rows<1>(img + L.img_off, ul, L.KP, L.scale, q, (const float4 *)xin + q, nK, nK, sa, sb);
            const int j = g * L.U + ul;
            if (q == 0) tg_st_granule<WT>(mail, region + (epoch & 1u) * FCP + j, epoch, __float_as_uint(fmaxf(sa[0] + w[ob + j], 0.0f)));
        }
    };
    // all N values of an exchanged vector, element j to thread j (+ 512, ...); whole waves take part, lanes past N re-read granule N - 1
    auto gather = [&](unsigned region, int N, unsigned epoch, bool &dead, unsigned code, auto &&put) {
        for (int j0 = wave * 64; j0 < N; j0 += TG_THREADS) {
            const int j = j0 + lane;
            const float v = take_staggered(mail, region + (unsigned)(j < N ? j : N - 1), epoch, dead, a.err, code);
            if (j < N) put(j, v);
        }
    };

    bool dead = false;
    unsigned epoch = 0;
    for (int it = team; it < (ta.ragged ? ta.n_slots : a.n_rows); it += ta.n_teams) {
        int row = it;
        if (ta.ragged) {
            row = ta.sched[it];
            if (row < 0 || row >= a.n_rows) continue;
        }
        const WrnnRow rw = a.rows[row];
        if (rw.steps < 1) continue;
        uint64_t kseed = a.seed;
        uint32_t krow = (uint32_t)row;
        if (a.keys) { const WrnnRowKey k = a.keys[row]; kseed = k.seed; krow = k.row; }

        // h1 = h2 = 0, x = x_init or 0 (:194-196); conditioning and xc of the row's first step
        for (int j = tid; j < HP; j += TG_THREADS) {
            lds[ly.xh1 + HP + j] = 0.0f; lds[ly.xh1 + 3 * HP + j] = 0.0f;
            lds[ly.xh2 + XAP + j] = 0.0f; lds[ly.xh2 + 2 * XAP + HP + j] = 0.0f;
        }
        if (tid == 0) misc[8] = a.x_init ? a.x_init[row] : 0.0f;
        cond_fill(rw, a.seg0, lds + ly.cb + ((epoch + 1u) & 1u) * ly.CB);
        __syncthreads();
        xc_publish(lds + ly.cb + ((epoch + 1u) & 1u) * ly.CB, epoch + 1u);

        for (int64_t t = a.seg0; t < a.seg0 + rw.steps; ++t) {
            ++epoch;
            const unsigned par = epoch & 1u;
            float *xh1 = lds + ly.xh1 + par * 2 * HP, *xh1n = lds + ly.xh1 + (par ^ 1u) * 2 * HP;
            float *xh2 = lds + ly.xh2 + par * (XAP + HP), *xh2n = lds + ly.xh2 + (par ^ 1u) * (XAP + HP);
            float *cbp = lds + ly.cb + par * ly.CB, *cbn = lds + ly.cb + (par ^ 1u) * ly.CB;
            const bool more = t + 1 < a.seg0 + rw.steps;

            // ---- conditioning: a2 / a3 / a4 of this step into the layer inputs ----
            for (int j = tid; j < A; j += TG_THREADS) {
                xh2[H + j] = cbp[F + A + j];        // a2_t :213
                f1[H + j] = cbp[F + 2 * A + j];     // a3_t :217
                f2[FC + j] = cbp[F + 3 * A + j];    // a4_t :220
            }
            // ---- x = I(cat[x_{t-1}, m_t, a1_t]) :208-209: the exchanged conditioning share + the sample's column ----
            {
                const float xprev = misc[8];
                const float *wI0 = w + a.off.I_t;   // row 0 of the [in][out] layout = W_I[:, 0]
                gather(M_XC + par * HP, H, epoch, dead, 10u, [&](int j, float v) { xh1[j] = fmaf(wI0[j], xprev, v); });
            }
            __syncthreads();
            // ---- 1. h1 = rnn1(x, h1); x = x + h1 :210-212 ----
            gru_phase(ta.plan.L[WRNN_TEAMG_RNN1], xh1, a.off.r1_bih, a.off.r1_bhh, M_H1, epoch);
            if (more) cond_fill(rw, t + 1, cbn);     // m, a of the next step, under the round trip of exchange 1
            gather(M_H1 + par * HP, H, epoch, dead, 11u, [&](int j, float v) { xh1n[HP + j] = v; xh2[j] = xh1[j] + v; });
            __syncthreads();
            // ---- 2. h2 = rnn2(cat[x, a2_t], h2); x = x + h2 :213-216 ----
            gru_phase(ta.plan.L[WRNN_TEAMG_RNN2], xh2, a.off.r2_bih, a.off.r2_bhh, M_H2, epoch);
            if (more) xc_publish(cbn, epoch + 1u);   // beside the chain, under exchange 2: read at the start of the next step
            gather(M_H2 + par * HP, H, epoch, dead, 12u, [&](int j, float v) { xh2n[XAP + j] = v; f1[j] = xh2[j] + v; });
            __syncthreads();
            // ---- 3. / 4. x = relu(fc1(cat[x, a3_t])); x = relu(fc2(cat[x, a4_t])) :217-221 ----
            fc_phase(ta.plan.L[WRNN_TEAMG_FC1], f1, a.off.fc1_b, M_F1, epoch);
            gather(M_F1 + par * FCP, FC, epoch, dead, 13u, [&](int j, float v) { f2[j] = v; });
            __syncthreads();
            fc_phase(ta.plan.L[WRNN_TEAMG_FC2], f2, a.off.fc2_b, M_F2, epoch);
            gather(M_F2 + par * FCP, FC, epoch, dead, 14u, [&](int j, float v) { f3[j] = v; });
            __syncthreads();
            // ---- 5. logits = fc3(x) :223 of the own classes, and the sampler :225-237 ----
            {
                const WrnnTeamGLayer &L = ta.plan.L[WRNN_TEAMG_FC3];
                const int nown = owned(L), nK = SP ? tg_sp_nk(ta.plan, ta.sp, L) : L.KP / 64;
                float bv = -INFINITY;
                int bi = 0x7fffffff;
                for (int ul = qw; ul < nown; ul += 32) {
                    float sa[1], sb[1];
                    if (ul < L.nres) tg_rows<1>(wres + L.lds_off, ul, L.KP, L.scale, q, (const float4 *)f3 + q, nK, nK, sa, sb);
                    else tg_rows<1>(img + L.img_off, ul, L.KP, L.scale, q, (const float4 *)f3 + q, nK, nK, sa, sb);
                    const int c = g * L.U + ul;
                    const float lg = sa[0] + w[a.off.fc3_b + c];
                    if (a.logits_out && q == 0) a.logits_out[((size_t)t * a.n_rows + row) * NC + c] = lg;
                    if (d.mode == WRNN_MODE_RAW) {
                        // Categorical(softmax(logits)).sample() == argmax_k logit_k - log q_k, q ~ Exp(1) (loop_simple.hip)
                        float v = lg;
                        if (a.noise_mode == WRNN_NOISE_INJECTED) v -= logf(a.noise1[((size_t)t * a.n_rows + row) * NC + c]);
                        else if (a.noise_mode == WRNN_NOISE_PHILOX) v -= logf(-logf(wrnn_uniform_raw(kseed, (uint64_t)t, krow, (uint32_t)c)));
                        if (v > bv) { bv = v; bi = c; }   // classes ascend: ties keep the lowest
                    } else if (q == 0) {
                        tg_st_granule<WT>(mail, M_CAND + par * 64 + c, epoch, __float_as_uint(lg));
                    }
                }
                if (d.mode == WRNN_MODE_RAW) {
                    if (q == 0) { misc[32 + qw] = bv; misc_i[64 + qw] = bi; }
                    __syncthreads();
                    if (wave == 0) {
                        float v = lane < 32 ? misc[32 + lane] : -INFINITY;
                        int k = lane < 32 ? misc_i[64 + lane] : 0x7fffffff;
                        wave_argmax(v, k);
                        if (lane == 0) {   // the workgroup's candidate: granule g = value, 32 + g = class
                            tg_st_granule<WT>(mail, M_CAND + par * 64 + g, epoch, __float_as_uint(v));
                            tg_st_granule<WT>(mail, M_CAND + par * 64 + 32 + g, epoch, (unsigned)k);
                        }
                        const float pv = take_staggered(mail, M_CAND + par * 64 + lane, epoch, dead, a.err, 15u);
                        const int ck = __shfl(__float_as_int(pv), (lane + 32) & 63, 64);
                        v = lane < 32 ? pv : -INFINITY;
                        k = lane < 32 ? ck : 0x7fffffff;
                        wave_argmax(v, k);
                        if (lane == 0) {
                            const float smp = 2.0f * (float)k / ((float)NC - 1.0f) - 1.0f;   // :235
                            if (g == 0) {
                                if (a.labels_out) a.labels_out[(size_t)row * a.steps + t] = k;
                                a.samples_out[(size_t)row * a.steps + t] = smp;
                            }
                            misc[8] = a.x_forced ? a.x_forced[(size_t)t * a.n_rows + row] : smp;
                        }
                    }
                } else if (wave == 0) {
                    // sample_from_discretized_mix_logistic (wavernn/utils/distribution.py:87-123) on the 3 * nr exchanged outputs, in every workgroup
                    const int nr = NC / 3;
                    const float lg = take_staggered(mail, M_CAND + par * 64 + (lane < NC ? lane : NC - 1), epoch, dead, a.err, 15u);
                    float v = -INFINITY;
                    int k = 0x7fffffff;
                    if (lane < nr) {
                        float u1;
                        if (a.noise_mode == WRNN_NOISE_INJECTED) u1 = a.noise1[((size_t)t * a.n_rows + row) * nr + lane];
                        else u1 = wrnn_uniform_mol(kseed, (uint64_t)t, krow, (uint32_t)lane);
                        v = lg - logf(-logf(u1));   // :107
                        k = lane;
                    }
                    wave_argmax(v, k);
                    k = k < nr ? k : 0;   // only after a timed-out exchange
                    const float mean = __shfl(lg, nr + k, 64);                                  // :113
                    const float ls = fmaxf(__shfl(lg, 2 * nr + k, 64), -32.23619130191664f);   // log(1e-14) :114-115
                    if (lane == 0) {
                        float u2;
                        if (a.noise_mode == WRNN_NOISE_INJECTED) u2 = a.noise2[(size_t)t * a.n_rows + row];
                        else u2 = wrnn_uniform_mol(kseed, (uint64_t)t, krow, 10u);
                        float xs = mean + expf(ls) * (logf(u2) - logf(1.0f - u2));  // :119
                        xs = fminf(fmaxf(xs, -1.0f), 1.0f);                         // :121
                        if (g == 0) {
                            if (a.labels_out) a.labels_out[(size_t)row * a.steps + t] = k;
                            a.samples_out[(size_t)row * a.steps + t] = xs;
                        }
                        misc[8] = a.x_forced ? a.x_forced[(size_t)t * a.n_rows + row] : xs;
                    }
                }
            }
            if ((epoch & 63u) == 0u && dead && lane == 0) misc_i[M_DEAD] = 1;   // bounded-spin bail-out, checked workgroup-wide every 64 samples
            __syncthreads();
            if ((epoch & 63u) == 0u && misc_i[M_DEAD]) return;
        }
    }
}

// dst(g, ul, gate, kdst + k) = src_t[(k0 + k) * ld + row0 + g * U + ul] for the units that exist; the image was zeroed.
// WT = _Float16: element kdst + k of the row goes where teamg_layout.h's paired layout puts it (tg16_pos), rounded to nearest even with
// subnormals kept (the conversion instruction in the kernel's default modes); a result that is not finite -- |w| >= 65520, or a weight
// that was not finite -- sets *bad and is never clamped.
template <typename WT>
__global__ void __launch_bounds__(256) teamg_pack_kernel(const float *__restrict__ src_t, int ld, int row0, int k0, int K, WT *__restrict__ img,
                                                         size_t wg_stride, size_t layer_off, int N, int U, int G, int gate, int KAP, int KP, int kdst, int32_t *bad) {
    const int unit = blockIdx.x;   // < N
    const int g = unit / U, ul = unit - g * U;
    const int row = ul * G + gate;
    WT *dst = img + (size_t)g * wg_stride + layer_off + (size_t)row * KP;
    for (int k = threadIdx.x; k < K; k += 256) {
        const WT v = (WT)src_t[(size_t)(k0 + k) * ld + row0 + unit];
        if constexpr (sizeof(WT) == 2) {
            if (!(fabsf((float)v) <= 65504.0f)) *bad = 1;
            dst[tg16_pos(kdst + k, row, KAP, KP)] = v;
        } else {
            dst[kdst + k] = v;
        }
    }
}

// The e4m3 pack: the same element as RNE(w * inv) in OCP e4m3fn (v_cvt_pk_fp8_f32 in the default rounding mode, subnormals kept), where
// inv = 1 / the layer's scale, a power of two: |w| * inv <= 448, nothing saturates.  tg8_pos places the byte.
__global__ void __launch_bounds__(256) teamg_pack8_kernel(const float *__restrict__ src_t, int ld, int row0, int k0, int K, unsigned char *__restrict__ img,
                                                          size_t wg_stride, size_t layer_off, int N, int U, int G, int gate, int KAP, int KP, int kdst, float inv) {
    const int unit = blockIdx.x;   // < N
    const int g = unit / U, ul = unit - g * U;
    const int row = ul * G + gate;
    unsigned char *dst = img + (size_t)g * wg_stride + layer_off + (size_t)row * KP;
    for (int k = threadIdx.x; k < K; k += 256) {
        const float v = src_t[(size_t)(k0 + k) * ld + row0 + unit] * inv;
        dst[tg8_pos(kdst + k, row, KAP, KP)] = (unsigned char)(__builtin_amdgcn_cvt_pk_fp8_f32(v, 0.0f, 0, false) & 0xff);
    }
}

// The abs-max pass of the e4m3 pack: *out = max(*out, bits of |w|) over rows [k0, k0 + K) x columns [c0, c0 + N) of src_t.  The bits of
// non-negative floats order as the floats do, and those of an infinity or a NaN are at or above 0x7f800000: one word is the maximum
// and the non-finite flag.  One block per row of src_t, columns across the threads.
__global__ void __launch_bounds__(256) teamg_absmax_kernel(const float *__restrict__ src_t, int ld, int c0, int k0, int N, unsigned *out) {
    const float *src = src_t + (size_t)(k0 + blockIdx.x) * ld + c0;
    unsigned m = 0;
    for (int j = threadIdx.x; j < N; j += 256) {
        const unsigned b = __float_as_uint(src[j]) & 0x7fffffffu;
        m = b > m ? b : m;
    }
    if (m) atomicMax(out, m);
}

// The two sources of an image row of the sparse pack: element p < KAP of the padded row of unit u is a[(ka0 + p) * lda + ca + u] for
// p < KA, element KAP + p is b[p * ldb + cb + u] for p < KB (b = nullptr: no segment B); everything else is padding.
struct TgSpSrc {
    const float *a, *b;
    int lda, ca, ka0, KA, ldb, cb, KB;
};
__device__ __forceinline__ float tg_sp_elem(const TgSpSrc &s, int unit, int KAP, int p) {
    if (p < KAP) return p < s.KA ? s.a[(size_t)(s.ka0 + p) * s.lda + s.ca + unit] : 0.0f;
    p -= KAP;
    return p < s.KB ? s.b[(size_t)p * s.ldb + s.cb + unit] : 0.0f;
}
// counters of the census, per layer, behind the flags
struct TgSpStat { unsigned nbA, nbB; unsigned long long kept; };

// The census: one workgroup per unit and gate, thread t the blocks t, t + 256, ... of the padded row (nKd of them, the first nAd segment
// A's).  flags[(unit * G + gate) * nKd + block] = 1 where a weight of the block does not compare equal to zero (a NaN does not); the
// layer's counters take the row's counts.  Blocks of padding only are zero by tg_sp_elem.
__global__ void __launch_bounds__(256) teamg_sp_census_kernel(TgSpSrc src, int G, int gate, int KAP, int nAd, int nKd, unsigned char *flags, TgSpStat *st) {
    __shared__ unsigned cnt[2];
    const int unit = blockIdx.x;
    if (threadIdx.x < 2) cnt[threadIdx.x] = 0;
    __syncthreads();
    unsigned char *f = flags + ((size_t)unit * G + gate) * nKd;
    for (int b = threadIdx.x; b < nKd; b += 256) {
        bool nz = false;
        for (int c = 0; c < 64; ++c) nz |= !(tg_sp_elem(src, unit, KAP, b * 64 + c) == 0.0f);
        f[b] = nz;
        if (nz) atomicAdd(&cnt[b < nAd ? 0 : 1], 1u);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        if (cnt[0]) atomicMax(&st->nbA, cnt[0]);
        if (cnt[1]) atomicMax(&st->nbB, cnt[1]);
        if (cnt[0] + cnt[1]) atomicAdd(&st->kept, (unsigned long long)(cnt[0] + cnt[1]));
    }
}

// The compaction: one workgroup per unit and gate writes its image row -- rs floats: [nbA + nbB 16-bit indices, padded to 16 bytes][the
// blocks].  Thread 0 lists the flagged blocks in ascending order, segment A's from entry 0 and B's from entry nbA; the entries a short
// row leaves keep the zero blocks of the memset and get the index of their segment's first block.  Then all threads copy the listed blocks.
__global__ void __launch_bounds__(256) teamg_sp_pack_kernel(TgSpSrc src, int U, int G, int gate, int KAP, int nAd, int nKd, int nbA, int nbB, int rs,
                                                            const unsigned char *__restrict__ flags, float *__restrict__ img, size_t wg_stride, size_t layer_off) {
    __shared__ int n_list[2];
    const int unit = blockIdx.x;
    const int g = unit / U, ul = unit - g * U;
    float *row = img + (size_t)g * wg_stride + layer_off + (size_t)(ul * G + gate) * rs;
    unsigned short *idx = (unsigned short *)row;
    const int nb = nbA + nbB;
    float *blocks = row + (nb + 7) / 8 * 4;
    const unsigned char *f = flags + ((size_t)unit * G + gate) * nKd;
    if (threadIdx.x == 0) {
        int ja = 0, jb = 0;
        for (int b = 0; b < nAd; ++b)
            if (f[b] && ja < nbA) idx[ja++] = (unsigned short)b;
        for (int b = nAd; b < nKd; ++b)
            if (f[b] && jb < nbB) idx[nbA + jb++] = (unsigned short)b;
        n_list[0] = ja; n_list[1] = jb;
        for (int j = ja; j < nbA; ++j) idx[j] = 0;
        for (int j = jb; j < nbB; ++j) idx[nbA + j] = (unsigned short)nAd;
    }
    __syncthreads();   // the list is read back from the image: a workgroup's own global writes are visible to it behind the barrier
    const int ja = n_list[0], jb = n_list[1];
    for (int e = threadIdx.x; e < nb * 64; e += 256) {
        const int j = e >> 6, c = e & 63;
        if (j < nbA ? j >= ja : j - nbA >= jb) continue;
        blocks[e] = tg_sp_elem(src, unit, KAP, (int)idx[j] * 64 + c);
    }
}

}  // namespace

float wrnn_teamg_e4m3_scale(float amax) {
    if (!(amax > 0.0f)) return 1.0f;
    int e;
    const float f = frexpf(amax, &e);   // amax = f 2^e, 0.5 <= f < 1; 448 = 0.875 * 2^9
    e -= f <= 0.875f ? 9 : 8;
    return ldexpf(1.0f, e < -126 ? -126 : e);
}

const char *const wrnn_teamg_layer_names[WRNN_TEAMG_LAYERS] = {"fc3", "fc2", "fc1", "rnn2", "rnn1", "I"};

const char *wrnn_teamg_make_plan(const WrnnDims &d, int64_t budget, WrnnTeamGPlan &p, int rows_per_team, int esz, const int32_t *nb_a, const int32_t *nb_b) {
    const TgLay ly(d);
    const int RB = rows_per_team;
    p = WrnnTeamGPlan{};
    p.esz = esz;
    auto set = [&](int l, int N, int G, int KA, int KB) {
        WrnnTeamGLayer &L = p.L[l];
        L.N = N; L.G = G; L.KA = KA; L.KB = KB; L.KAP = tg_r64(KA); L.KP = L.KAP + (KB ? tg_r64(KB) : 0); L.U = (N + TEAM_WGS - 1) / TEAM_WGS;
        L.scale = 1.0f;
    };
    set(WRNN_TEAMG_FC3, d.NC, 1, d.FC, 0);
    set(WRNN_TEAMG_FC2, d.FC, 1, d.FC + d.A, 0);
    set(WRNN_TEAMG_FC1, d.FC, 1, d.H + d.A, 0);
    set(WRNN_TEAMG_RNN2, d.H, 3, d.H + d.A, d.H);
    set(WRNN_TEAMG_RNN1, d.H, 3, d.H, d.H);
    set(WRNN_TEAMG_COND, d.H, 1, d.F + d.A, 0);
    if (nb_a && nb_b) {
        // the block-sparse image: a row is its index list and its blocks (wrnn_internal.h); 16-bit indices
        for (int l = 0; l < WRNN_TEAMG_LAYERS; ++l) {
            WrnnTeamGLayer &L = p.L[l];
            if (L.KP / 64 > 65535) return "the block-sparse image: a row of more than 65535 blocks";
            if (nb_a[l] < 0 || nb_b[l] < 0 || nb_a[l] > L.KAP / 64 || nb_b[l] > (L.KP - L.KAP) / 64) return "the block-sparse image: more blocks than the dense row has";
            L.KP = wrnn_teamg_sparse_row_elems(nb_a[l] + nb_b[l]);
        }
    }
    // one row: TgLay as ever; RB rows in lock-step: TgbLay, and every mailbox region once per row
    const int64_t act_floats = RB == 1 ? ly.total : TgbLay(d, RB).total;
    const int64_t act_bytes = act_floats * 4;
    const int64_t granules = (int64_t)RB * 2LL * (3 * ly.HP + 2 * ly.FCP + 64);
    if (act_bytes > TG_LDS_MAX)
        return RB == 1 ? "WRNN_KERNEL_TEAMG: the activation vectors of one row exceed 160 KiB of LDS"
                       : "WRNN_KERNEL_TEAMG_BATCH: the activation vectors of this many rows per team exceed 160 KiB of LDS";
    if (granules > WRNN_MAIL_GRANULES_MAX)
        return RB == 1 ? "WRNN_KERNEL_TEAMG: fc_dims too large for the team mailbox"
                       : "WRNN_KERNEL_TEAMG_BATCH: the exchanges of this many rows per team exceed the team mailbox";
    p.act_floats = (int32_t)act_floats;
    p.mail_granules = (int32_t)granules;
    if (d.mode == WRNN_MODE_MOL && d.NC > 64) return "WRNN_KERNEL_TEAMG: more than 64 mixture outputs";
    const int64_t dflt = TG_LDS_MAX - act_bytes;
    if (budget < 0 || budget > dflt) budget = dflt;
    // Residency in layer order (shortest rows first): whole units, as many as still fit; the first layer that does not fit whole is the
    // last to get any (so a layer's resident share never shrinks when the budget grows).  Every workgroup gets the same count.
    // Counted in elements of esz bytes; a unit is a multiple of 64 elements, so every offset is a multiple of 16 bytes in every format.
    int64_t left = budget / esz, img = 0, res = 0;
    for (int l = 0; l < WRNN_TEAMG_LAYERS; ++l) {
        WrnnTeamGLayer &L = p.L[l];
        const int64_t unit = (int64_t)L.G * L.KP;
        int64_t n = unit ? left / unit : L.U;   // a layer with no block at all (the sparse image of an all-zero layer) takes no room
        if (n > L.U) n = L.U;
        L.nres = (int32_t)n;
        L.lds_off = (int32_t)res;
        L.img_off = img;
        res += n * unit; left -= n * unit;
        if (n < L.U) left = 0;
        img += (int64_t)L.U * unit;
    }
    p.img_elems_wg = img;
    p.res_elems = (int32_t)res;
    return nullptr;
}

hipError_t wrnn_teamg_pack(const wrnn_handle *h, const WrnnTeamGPlan &p, void *img, hipStream_t s, int *bad_layer, float scales[WRNN_TEAMG_LAYERS]) {
    const WrnnDims &d = h->d;
    const WrnnPacked &o = h->off;
    const float *w = h->wdev;
    const int H = d.H, A = d.A, FC = d.FC;
    *bad_layer = -1;
    for (int l = 0; l < WRNN_TEAMG_LAYERS; ++l) scales[l] = 1.0f;
    hipError_t e = hipMemsetAsync(img, 0, wrnn_teamg_img_bytes(p), s);   // padding elements and the words behind the slices
    if (e != hipSuccess) return e;
    (void)hipGetLastError();
    int32_t *flags = (int32_t *)((char *)img + (size_t)TEAM_WGS * p.img_elems_wg * p.esz);   // one word per layer behind the slices
    if (p.esz == 1) {
        // the six maxima, all gates and both matrices of a GRU layer together (they share image rows); the only wait of this pack
        auto amax = [&](int l, const float *src_t, int ld, int c0, int k0, int K, int N) {
            hipLaunchKernelGGL(teamg_absmax_kernel, dim3(K), dim3(256), 0, s, src_t, ld, c0, k0, N, (unsigned *)flags + l);
        };
        amax(WRNN_TEAMG_FC3, w + o.fc3_t, d.NC, 0, 0, FC, d.NC);
        amax(WRNN_TEAMG_FC2, w + o.fc2_t, FC, 0, 0, FC + A, FC);
        amax(WRNN_TEAMG_FC1, w + o.fc1_t, FC, 0, 0, H + A, FC);
        amax(WRNN_TEAMG_RNN2, w + o.r2_wih_t, 3 * H, 0, 0, H + A, 3 * H);
        amax(WRNN_TEAMG_RNN2, w + o.r2_whh_t, 3 * H, 0, 0, H, 3 * H);
        amax(WRNN_TEAMG_RNN1, w + o.r1_wih_t, 3 * H, 0, 0, H, 3 * H);
        amax(WRNN_TEAMG_RNN1, w + o.r1_whh_t, 3 * H, 0, 0, H, 3 * H);
        amax(WRNN_TEAMG_COND, w + o.I_t, H, 0, 1, d.F + A, H);
        e = hipGetLastError();
        uint32_t bits[WRNN_TEAMG_LAYERS];
        if (e == hipSuccess) e = hipMemcpyAsync(bits, flags, sizeof(bits), hipMemcpyDeviceToHost, s);
        if (e == hipSuccess) e = hipStreamSynchronize(s);
        if (e != hipSuccess) return e;
        for (int l = WRNN_TEAMG_LAYERS - 1; l >= 0; --l) {
            if (bits[l] >= 0x7f800000u) { *bad_layer = l; continue; }
            float m;
            memcpy(&m, &bits[l], sizeof(m));
            scales[l] = wrnn_teamg_e4m3_scale(m);
        }
        if (*bad_layer >= 0) return hipSuccess;
    }
    auto put = [&](int l, const float *src_t, int ld, int row0, int k0, int K, int gate, int kdst) {
        const WrnnTeamGLayer &L = p.L[l];
        if (p.esz == 1)
            hipLaunchKernelGGL(teamg_pack8_kernel, dim3(L.N), dim3(256), 0, s, src_t, ld, row0, k0, K, (unsigned char *)img, (size_t)p.img_elems_wg, (size_t)L.img_off,
                               L.N, L.U, L.G, gate, L.KAP, L.KP, kdst, 1.0f / scales[l]);
        else if (p.esz == 4)
            hipLaunchKernelGGL(teamg_pack_kernel<float>, dim3(L.N), dim3(256), 0, s, src_t, ld, row0, k0, K, (float *)img, (size_t)p.img_elems_wg, (size_t)L.img_off,
                               L.N, L.U, L.G, gate, L.KAP, L.KP, kdst, flags + l);
        else
            hipLaunchKernelGGL(teamg_pack_kernel<_Float16>, dim3(L.N), dim3(256), 0, s, src_t, ld, row0, k0, K, (_Float16 *)img, (size_t)p.img_elems_wg,
                               (size_t)L.img_off, L.N, L.U, L.G, gate, L.KAP, L.KP, kdst, flags + l);
    };
    put(WRNN_TEAMG_FC3, w + o.fc3_t, d.NC, 0, 0, FC, 0, 0);
    put(WRNN_TEAMG_FC2, w + o.fc2_t, FC, 0, 0, FC + A, 0, 0);
    put(WRNN_TEAMG_FC1, w + o.fc1_t, FC, 0, 0, H + A, 0, 0);
    for (int gate = 0; gate < 3; ++gate) {
        put(WRNN_TEAMG_RNN2, w + o.r2_wih_t, 3 * H, gate * H, 0, H + A, gate, 0);
        put(WRNN_TEAMG_RNN2, w + o.r2_whh_t, 3 * H, gate * H, 0, H, gate, p.L[WRNN_TEAMG_RNN2].KAP);
        put(WRNN_TEAMG_RNN1, w + o.r1_wih_t, 3 * H, gate * H, 0, H, gate, 0);
        put(WRNN_TEAMG_RNN1, w + o.r1_whh_t, 3 * H, gate * H, 0, H, gate, p.L[WRNN_TEAMG_RNN1].KAP);
    }
    put(WRNN_TEAMG_COND, w + o.I_t, H, 0, 1, d.F + A, 0, 0);   // column 0 (the fed-back sample) stays a vector
    e = hipGetLastError();
    if (e != hipSuccess || p.esz != 2) return e;
    // the range check of the fp16 image: once per pack, the only wait
    int32_t bad[WRNN_TEAMG_LAYERS];
    e = hipMemcpyAsync(bad, flags, sizeof(bad), hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) return e;
    for (int l = WRNN_TEAMG_LAYERS - 1; l >= 0; --l)
        if (bad[l]) *bad_layer = l;
    return hipSuccess;
}

// ---- the block-sparse pack ----

namespace {
struct TgSpLayer { int l; TgSpSrc src[3]; };
// the six layers' sources, gate by gate, as wrnn_teamg_pack's `put`s have them
void tg_sp_sources(const wrnn_handle *h, TgSpLayer (&out)[WRNN_TEAMG_LAYERS]) {
    const WrnnDims &d = h->d;
    const WrnnPacked &o = h->off;
    const float *w = h->wdev;
    const int H = d.H, A = d.A, FC = d.FC;
    auto one = [&](int l, const float *a, int lda, int ka0, int KA) {
        out[l].l = l;
        for (int gt = 0; gt < 3; ++gt) out[l].src[gt] = TgSpSrc{a, nullptr, lda, 0, ka0, KA, 0, 0, 0};
    };
    auto gru = [&](int l, const float *a, int KA, const float *b) {
        out[l].l = l;
        for (int gt = 0; gt < 3; ++gt) out[l].src[gt] = TgSpSrc{a, b, 3 * H, gt * H, 0, KA, 3 * H, gt * H, H};
    };
    one(WRNN_TEAMG_FC3, w + o.fc3_t, d.NC, 0, FC);
    one(WRNN_TEAMG_FC2, w + o.fc2_t, FC, 0, FC + A);
    one(WRNN_TEAMG_FC1, w + o.fc1_t, FC, 0, H + A);
    gru(WRNN_TEAMG_RNN2, w + o.r2_wih_t, H + A, w + o.r2_whh_t);
    gru(WRNN_TEAMG_RNN1, w + o.r1_wih_t, H, w + o.r1_whh_t);
    one(WRNN_TEAMG_COND, w + o.I_t, H, 1, d.F + A);   // column 0 (the fed-back sample) stays a vector
}
// offsets of the layers' flags, the counters behind them
size_t tg_sp_flag_offsets(const WrnnTeamGPlan &dense, size_t (&off)[WRNN_TEAMG_LAYERS]) {
    size_t n = 0;
    for (int l = 0; l < WRNN_TEAMG_LAYERS; ++l) {
        off[l] = n;
        n += (size_t)dense.L[l].N * dense.L[l].G * (dense.L[l].KP / 64);
    }
    return (n + 15) & ~(size_t)15;
}
// the dense layer table alone (no budget, one row: sizes that cannot fail for dims a handle holds)
void tg_sp_dense_layers(const WrnnDims &d, WrnnTeamGPlan &p) { (void)wrnn_teamg_make_plan(d, 0, p, 1, 4); }
}  // namespace

size_t wrnn_teamg_sparse_flag_bytes(const WrnnDims &d) {
    WrnnTeamGPlan dense;
    tg_sp_dense_layers(d, dense);
    size_t off[WRNN_TEAMG_LAYERS];
    return tg_sp_flag_offsets(dense, off) + WRNN_TEAMG_LAYERS * sizeof(TgSpStat);
}

hipError_t wrnn_teamg_sparse_census(const wrnn_handle *h, void *flags, hipStream_t s, int32_t nb_a[WRNN_TEAMG_LAYERS], int32_t nb_b[WRNN_TEAMG_LAYERS],
                                    int64_t kept[WRNN_TEAMG_LAYERS], int64_t dense_blocks[WRNN_TEAMG_LAYERS]) {
    WrnnTeamGPlan dense;
    tg_sp_dense_layers(h->d, dense);
    size_t off[WRNN_TEAMG_LAYERS];
    const size_t nflags = tg_sp_flag_offsets(dense, off);
    TgSpStat *st = (TgSpStat *)((char *)flags + nflags);
    hipError_t e = hipMemsetAsync(st, 0, WRNN_TEAMG_LAYERS * sizeof(TgSpStat), s);
    if (e != hipSuccess) return e;
    (void)hipGetLastError();
    TgSpLayer src[WRNN_TEAMG_LAYERS];
    tg_sp_sources(h, src);
    for (int l = 0; l < WRNN_TEAMG_LAYERS; ++l) {
        const WrnnTeamGLayer &L = dense.L[l];
        for (int gt = 0; gt < L.G; ++gt)
            hipLaunchKernelGGL(teamg_sp_census_kernel, dim3(L.N), dim3(256), 0, s, src[l].src[gt], L.G, gt, L.KAP, L.KAP / 64, L.KP / 64, (unsigned char *)flags + off[l],
                               st + l);
    }
    e = hipGetLastError();
    TgSpStat got[WRNN_TEAMG_LAYERS];
    if (e == hipSuccess) e = hipMemcpyAsync(got, st, sizeof(got), hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);   // the only wait of the sparse pack
    if (e != hipSuccess) return e;
    for (int l = 0; l < WRNN_TEAMG_LAYERS; ++l) {
        nb_a[l] = (int32_t)got[l].nbA; nb_b[l] = (int32_t)got[l].nbB; kept[l] = (int64_t)got[l].kept;
        dense_blocks[l] = (int64_t)dense.L[l].N * dense.L[l].G * (dense.L[l].KP / 64);
    }
    return hipSuccess;
}

hipError_t wrnn_teamg_sparse_pack(const wrnn_handle *h, const WrnnTeamGPlan &p, const int32_t *nb_a, const int32_t *nb_b, const void *flags, void *img, hipStream_t s) {
    WrnnTeamGPlan dense;
    tg_sp_dense_layers(h->d, dense);
    size_t off[WRNN_TEAMG_LAYERS];
    (void)tg_sp_flag_offsets(dense, off);
    hipError_t e = hipMemsetAsync(img, 0, wrnn_teamg_img_bytes(p), s);   // the zero blocks that pad a short row; units past N
    if (e != hipSuccess) return e;
    (void)hipGetLastError();
    TgSpLayer src[WRNN_TEAMG_LAYERS];
    tg_sp_sources(h, src);
    for (int l = 0; l < WRNN_TEAMG_LAYERS; ++l) {
        const WrnnTeamGLayer &L = p.L[l], &D = dense.L[l];
        if (nb_a[l] + nb_b[l] == 0) continue;
        for (int gt = 0; gt < L.G; ++gt)
            hipLaunchKernelGGL(teamg_sp_pack_kernel, dim3(L.N), dim3(256), 0, s, src[l].src[gt], L.U, L.G, gt, D.KAP, D.KAP / 64, D.KP / 64, nb_a[l], nb_b[l], L.KP,
                               (const unsigned char *)flags + off[l], (float *)img, (size_t)p.img_elems_wg, (size_t)L.img_off);
    }
    return hipGetLastError();
}

static const void *teamg_kernel_fn(const WrnnTeamGPlan &p, bool sparse = false) {
    if (sparse) return (const void *)loop_teamg_kernel<TgSparse>;
    return p.esz == 4 ? (const void *)loop_teamg_kernel<float> : p.esz == 2 ? (const void *)loop_teamg_kernel<_Float16> : (const void *)loop_teamg_kernel<TgE4m3>;
}

hipError_t wrnn_teamg_occupancy(const WrnnTeamGPlan &p, int *blocks_per_cu, bool sparse) {
    const size_t lds = wrnn_teamg_lds_bytes(p);
    hipError_t e = hipFuncSetAttribute(teamg_kernel_fn(p, sparse), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
    return hipOccupancyMaxActiveBlocksPerMultiprocessor(blocks_per_cu, teamg_kernel_fn(p, sparse), TG_THREADS, lds);
}

hipError_t wrnn_launch_loop_teamg(const WrnnTeamGArgs &a, hipStream_t s) {
    (void)hipGetLastError();
    const size_t lds = wrnn_teamg_lds_bytes(a.plan);
    hipError_t e = hipFuncSetAttribute(teamg_kernel_fn(a.plan, a.sp.on != 0), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
    if (a.sp.on) hipLaunchKernelGGL(loop_teamg_kernel<TgSparse>, dim3(a.n_teams * TEAM_WGS), dim3(TG_THREADS), lds, s, a);
    else if (a.plan.esz == 4) hipLaunchKernelGGL(loop_teamg_kernel<float>, dim3(a.n_teams * TEAM_WGS), dim3(TG_THREADS), lds, s, a);
    else if (a.plan.esz == 2) hipLaunchKernelGGL(loop_teamg_kernel<_Float16>, dim3(a.n_teams * TEAM_WGS), dim3(TG_THREADS), lds, s, a);
    else hipLaunchKernelGGL(loop_teamg_kernel<TgE4m3>, dim3(a.n_teams * TEAM_WGS), dim3(TG_THREADS), lds, s, a);
    return hipGetLastError();
}

// ---- C ABI: the plan, host only ----

// nb_a / nb_b: the plan of the block-sparse image with those blocks per row (fp32 only); the byte figures then count the image's rows,
// index lists included, so that resident + streamed == image bytes; k and k_padded stay the dense row's
int wrnn_teamg_plan_info_impl(const wrnn_config *cfg, int rows_per_team, int fmt, int64_t lds_budget_bytes, wrnn_teamg_plan_info *out, const int32_t *nb_a,
                              const int32_t *nb_b) {
    if (!cfg || !out || rows_per_team < 1 || rows_per_team > WRNN_TEAMG_BATCH_MAX_ROWS) return WRNN_ERR_INVALID;
    if (fmt != WRNN_WEIGHTS_F32 && fmt != WRNN_WEIGHTS_F16 && fmt != WRNN_WEIGHTS_E4M3) return WRNN_ERR_INVALID;   // 2 is reserved
    const int64_t esz = fmt == WRNN_WEIGHTS_E4M3 ? 1 : fmt == WRNN_WEIGHTS_F16 ? 2 : 4;
    WrnnDims d;
    if (wrnn_dims_from_config(cfg, d) || d.FC > (1 << 20) || d.F > (1 << 20)) return WRNN_ERR_INVALID;
    WrnnTeamGPlan p;
    const bool sparse = nb_a && nb_b;
    if (sparse) {
        if (fmt != WRNN_WEIGHTS_F32) return WRNN_ERR_INVALID;
        WrnnTeamGPlan dense;
        (void)wrnn_teamg_make_plan(d, 0, dense, 1, 4);   // the layer table: a count above the dense row's is the caller's mistake
        for (int l = 0; l < WRNN_TEAMG_LAYERS; ++l)
            if (nb_a[l] < 0 || nb_b[l] < 0 || nb_a[l] > dense.L[l].KAP / 64 || nb_b[l] > (dense.L[l].KP - dense.L[l].KAP) / 64) return WRNN_ERR_INVALID;
    }
    if (wrnn_teamg_make_plan(d, lds_budget_bytes, p, rows_per_team, (int)esz, nb_a, nb_b)) return WRNN_ERR_UNSUPPORTED;
    *out = wrnn_teamg_plan_info{};
    for (int l = 0; l < WRNN_TEAMG_LAYERS; ++l) {
        const WrnnTeamGLayer &L = p.L[l];
        wrnn_teamg_layer_info &o = out->layer[l];
        const int K = L.KA + L.KB;
        const int64_t KB_ = sparse ? L.KP : K;   // what a row counts in the byte figures
        o.units = L.N; o.rows_per_unit = L.G; o.k = K; o.k_padded = sparse ? L.KAP + tg_r64(L.KB) : L.KP; o.resident_units = L.nres;
        o.weight_bytes = esz * L.N * L.G * KB_;
        o.rows_min = INT32_MAX;
        for (int g = 0; g < TEAM_WGS; ++g) {
            int n = L.N - g * L.U;
            n = n < 0 ? 0 : (n > L.U ? L.U : n);
            o.own_first[g] = n ? g * L.U : L.N;
            o.own_count[g] = n;
            const int rows = n * L.G, res = (n < L.nres ? n : L.nres);
            if (rows < o.rows_min) o.rows_min = rows;
            if (rows > o.rows_max) o.rows_max = rows;
            const int64_t rb = esz * res * L.G * KB_;
            if (rb > o.resident_bytes_wg) o.resident_bytes_wg = rb;
            o.resident_bytes_team += rb;
        }
        o.streamed_bytes_step = o.weight_bytes - o.resident_bytes_team;
        o.lds_bytes = esz * L.nres * L.G * L.KP;
        out->streamed_bytes_step += o.streamed_bytes_step;
    }
    out->activation_bytes = 4LL * p.act_floats;
    out->lds_bytes = (int64_t)wrnn_teamg_lds_bytes(p);
    out->lds_budget_bytes = (lds_budget_bytes < 0 || lds_budget_bytes > TG_LDS_MAX - out->activation_bytes) ? TG_LDS_MAX - out->activation_bytes : lds_budget_bytes;
    out->mail_granules = p.mail_granules;
    return WRNN_OK;
}

static int teamg_plan_info(const wrnn_config *cfg, int rows_per_team, int fmt, int64_t lds_budget_bytes, wrnn_teamg_plan_info *out) {
    return wrnn_teamg_plan_info_impl(cfg, rows_per_team, fmt, lds_budget_bytes, out, nullptr, nullptr);
}

extern "C" int wrnn_teamg_sparse_plan(const wrnn_config *cfg, int32_t rows_per_team, const int32_t nb_a[6], const int32_t nb_b[6], int64_t lds_budget_bytes,
                                      wrnn_teamg_plan_info *out) {
    if (!nb_a || !nb_b) return WRNN_ERR_INVALID;
    return wrnn_teamg_plan_info_impl(cfg, rows_per_team, WRNN_WEIGHTS_F32, lds_budget_bytes, out, nb_a, nb_b);
}

extern "C" int wrnn_teamg_plan(const wrnn_config *cfg, int64_t lds_budget_bytes, wrnn_teamg_plan_info *out) {
    return teamg_plan_info(cfg, 1, WRNN_WEIGHTS_F32, lds_budget_bytes, out);
}

extern "C" int wrnn_teamg_batch_plan(const wrnn_config *cfg, int32_t rows_per_team, int64_t lds_budget_bytes, wrnn_teamg_plan_info *out) {
    return teamg_plan_info(cfg, rows_per_team, WRNN_WEIGHTS_F32, lds_budget_bytes, out);
}

extern "C" int wrnn_teamg_plan_fmt(const wrnn_config *cfg, int32_t rows_per_team, int32_t weight_format, int64_t lds_budget_bytes, wrnn_teamg_plan_info *out) {
    return teamg_plan_info(cfg, rows_per_team, weight_format, lds_budget_bytes, out);
}
