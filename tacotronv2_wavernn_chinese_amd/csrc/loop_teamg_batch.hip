// WRNN_KERNEL_TEAMG_BATCH: loop_teamg.hip's step with RB = 2, 4 or 8 rows per XCD team in lock-step, for ANY constructor dims.  One row
// per team leaves a streamed weight byte with one multiply-add and an exchange round trip with one row's values; here every weight
// float4, LDS resident or streamed, is loaded once per step and multiplied into RB activation vectors, and every exchange carries the
// RB rows' granules.  Everything else is that kernel's, unchanged: WrnnTeamGPlan's ownership of contiguous units, the SAME packed
// weight image (wrnn_teamg_pack), residency first and streaming for the rest, the five exchanges of a step plus [xc] beside the chain,
// and team_common.h's protocol (join_team, st_granule, take_staggered, the `dead` bail-out every 64 steps).  No new hand-off form.
//
// Per (row, output) the arithmetic is loop_teamg.hip's operand for operand -- tgb_dot keeps tg_dot's k order, its a0 / a1 split and
// row_sum, the cells use the same libm calls, Philox is keyed (seed or row key, step, row, class), the race keeps the lowest class of
// a tie -- so a row's labels, samples and logits are bit-equal to WRNN_KERNEL_TEAMG's whatever batch the row lands in.
// The kernel is templated on the element type of the image as loop_teamg.hip is (float, or _Float16 for WRNN_WEIGHTS_F16): the fp16
// instantiations are bit-equal to the fp16 instantiation of that kernel, and to the fp32 ones on the model rounded to fp16; likewise
// TgE4m3 (WRNN_WEIGHTS_E4M3) and the model dequantised from its e4m3 bytes and per-layer scales.
//
// Rows.  Batch b = schedule slots [b rpb, (b + 1) rpb) of `order` (longest first in a ragged call, identity otherwise), dealt to the
// teams round-robin, in snake order when ragged, as loop_batch_cs.hip deals them.  A batch runs for the steps of its longest row; a
// row past its own steps keeps its slot, goes on computing and writes nothing; slots past rpb or past the last row run on zeros and
// write nothing.  Exchanges never depend on a row's state: every workgroup publishes and takes every slot.
//
// LDS (TgbLay, teamg_layout.h).  Row r's vectors are TgLay's at r * rowf: a 16-lane group reads float4 q, q + 16, ... of a weight row
// once and of each of the RB vectors, RB + G ds_read_b128 (resident) or RB (streamed) per G weight float4 and 4 G RB multiply-adds;
// the three gate rows of a unit share the RB activation reads where a workgroup owns more than 16 units (G = 3), a group takes one
// gate row where it owns fewer (G = 1, more loads in flight) -- loop_teamg.hip's rule, the sums are the same either way.  After a
// dot product lane r of the group finishes row r: bias, cell or relu, noise, its granule.  The race of row r and the MOL sampler of
// row r run in wave r.
#include <type_traits>

#include "team_common.h"
#include "teamg_layout.h"

namespace {

// tg_dot (loop_teamg.hip) against RB activation vectors xs4 float4 apart: one load of every weight float4, RB uses.  The sums of a row
// are in every lane of the 16-lane group; lane q keeps those of row q (q < RB) in sa / sb -- selects, no indexed registers.
// The weight loads of UNR steps of k are issued together (they are what has latency to hide); a step's RB activation reads come from
// LDS right before its multiply-adds, and the scheduling barrier keeps the compiler from hoisting those of all UNR steps, which would
// not fit the registers of two waves per SIMD.  k ascends as in tg_dot, so do the a0 / a1 chains.
template <int G, int RB>
__device__ __forceinline__ void tgb_dot(const float4 *__restrict__ wp, int kp4, const float4 *lds4, int xi, int xs4, int nA, int nK, int q, float (&sa)[G], float (&sb)[G]) {
    constexpr int UNR = G == 1 ? 4 : 2;
    // The RB row addresses are made here, from an index the compiler cannot see through: as invariants of the step loop it would keep
    // RB address registers per call site alive across the whole step (LDS offsets beyond the instruction's immediate).
    asm volatile("" : "+v"(xi));
    const float4 *xp = lds4 + xi;
    float a0[RB][G], a1[RB][G];
#pragma unroll
    for (int r = 0; r < RB; ++r)
#pragma unroll
        for (int g = 0; g < G; ++g) a0[r][g] = a1[r][g] = 0.0f;
    auto mac = [&](const float4 (&w)[G], int k) {
#pragma unroll
        for (int r = 0; r < RB; ++r) {
            const float4 x = xp[r * xs4 + k * 16];
#pragma unroll
            for (int g = 0; g < G; ++g) {
                a0[r][g] = fmaf(w[g].x, x.x, a0[r][g]); a1[r][g] = fmaf(w[g].y, x.y, a1[r][g]);
                a0[r][g] = fmaf(w[g].z, x.z, a0[r][g]); a1[r][g] = fmaf(w[g].w, x.w, a1[r][g]);
            }
        }
    };
    auto segment = [&](int k0, int k1) {
        int k = k0;
#pragma unroll 1
        for (; k + UNR <= k1; k += UNR) {
            float4 w[UNR][G];
#pragma unroll
            for (int u = 0; u < UNR; ++u)
#pragma unroll
                for (int g = 0; g < G; ++g) w[u][g] = wp[(size_t)g * kp4 + (k + u) * 16];
#pragma unroll
            for (int u = 0; u < UNR; ++u) {
                mac(w[u], k + u);
                __builtin_amdgcn_sched_barrier(0);
            }
        }
#pragma unroll 1
        for (; k < k1; ++k) {
            float4 w[G];
#pragma unroll
            for (int g = 0; g < G; ++g) w[g] = wp[(size_t)g * kp4 + k * 16];
            mac(w, k);
        }
    };
    segment(0, nA);
#pragma unroll
    for (int r = 0; r < RB; ++r)
#pragma unroll
        for (int g = 0; g < G; ++g) {
            const float v = row_sum(a0[r][g] + a1[r][g]);
            sa[g] = (r == 0 || q == r) ? v : sa[g];
            a0[r][g] = a1[r][g] = 0.0f;
        }
    segment(nA, nK);
#pragma unroll
    for (int r = 0; r < RB; ++r)
#pragma unroll
        for (int g = 0; g < G; ++g) {
            const float v = row_sum(a0[r][g] + a1[r][g]);
            sb[g] = (r == 0 || q == r) ? v : sb[g];
        }
}

// tgb_dot on the fp16 image (teamg_layout.h), as tg_dot16 is tg_dot's: rp = the unit's first row, rows kp8 16-byte pieces apart, row0 its
// index in the slice.  One 16-byte load per row and PAIR of steps, UNP pairs issued together (tgb_dot's weight bytes in flight; with 8
// rows half of them, there are no registers for more), an 8-byte load for the unpaired last step of a segment.  Each step's weights are
// widened exactly right before its multiply-adds; per (row, lane) the chains are tgb_dot's.
template <int G, int RB>
__device__ __forceinline__ void tgb_dot16(const TgHalf8 *__restrict__ rp, int kp8, int row0, const float4 *lds4, int xi, int xs4, int nA, int nK, int q, float (&sa)[G],
                                          float (&sb)[G]) {
    constexpr int UNP = (G == 1 ? 4 : 2) / (RB <= 4 ? 1 : 2);
    asm volatile("" : "+v"(xi));
    const float4 *xp = lds4 + xi;
    const TgHalf8 *wp[G];
#pragma unroll
    for (int g = 0; g < G; ++g) wp[g] = rp + (size_t)g * kp8 + (q ^ tg16_swz(row0 + g, kp8 * 8));
    float a0[RB][G], a1[RB][G];
#pragma unroll
    for (int r = 0; r < RB; ++r)
#pragma unroll
        for (int g = 0; g < G; ++g) a0[r][g] = a1[r][g] = 0.0f;
    auto mac = [&](const float4 (&w)[G], int k) {
#pragma unroll
        for (int r = 0; r < RB; ++r) {
            const float4 x = xp[r * xs4 + k * 16];
#pragma unroll
            for (int g = 0; g < G; ++g) {
                a0[r][g] = fmaf(w[g].x, x.x, a0[r][g]); a1[r][g] = fmaf(w[g].y, x.y, a1[r][g]);
                a0[r][g] = fmaf(w[g].z, x.z, a0[r][g]); a1[r][g] = fmaf(w[g].w, x.w, a1[r][g]);
            }
        }
    };
    auto pair = [&](const TgHalf8 (&wv)[G], int k) {
        float4 w[G];
#pragma unroll
        for (int g = 0; g < G; ++g) w[g] = tg_lo4(wv[g]);
        mac(w, k);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int g = 0; g < G; ++g) w[g] = tg_hi4(wv[g]);
        mac(w, k + 1);
        __builtin_amdgcn_sched_barrier(0);
    };
    // NP pairs of steps from step k: their weight loads are issued together
    auto block = [&](auto np, int k) {
        constexpr int NP = decltype(np)::value;
        TgHalf8 wv[NP][G];
#pragma unroll
        for (int u = 0; u < NP; ++u)
#pragma unroll
            for (int g = 0; g < G; ++g) wv[u][g] = wp[g][(k + 2 * u) * 8];
#pragma unroll
        for (int u = 0; u < NP; ++u) pair(wv[u], k + 2 * u);
    };
    // UNP pairs at a time, then what is left in halving blocks: a short segment still has all its loads in flight at once
    auto segment = [&](int k0, int k1) {
        int k = k0;
#pragma unroll 1
        for (; k + 2 * UNP <= k1; k += 2 * UNP) block(std::integral_constant<int, UNP>{}, k);
        if constexpr (UNP > 2) {
            if (k + 4 <= k1) { block(std::integral_constant<int, 2>{}, k); k += 4; }
        }
        if constexpr (UNP > 1) {
            if (k + 2 <= k1) { block(std::integral_constant<int, 1>{}, k); k += 2; }
        }
        if (k < k1) {
            float4 w[G];
#pragma unroll
            for (int g = 0; g < G; ++g) w[g] = tg_w4(((const TgHalf4 *)(rp + (size_t)g * kp8))[k * 16 + q]);
            mac(w, k);
        }
    };
    segment(0, nA);
#pragma unroll
    for (int r = 0; r < RB; ++r)
#pragma unroll
        for (int g = 0; g < G; ++g) {
            const float v = row_sum(a0[r][g] + a1[r][g]);
            sa[g] = (r == 0 || q == r) ? v : sa[g];
            a0[r][g] = a1[r][g] = 0.0f;
        }
    segment(nA, nK);
#pragma unroll
    for (int r = 0; r < RB; ++r)
#pragma unroll
        for (int g = 0; g < G; ++g) {
            const float v = row_sum(a0[r][g] + a1[r][g]);
            sb[g] = (r == 0 || q == r) ? v : sb[g];
        }
}

// tgb_dot on the e4m3 image (teamg_layout.h), as tg_dot8 is tg_dot's: rp = the unit's first row, rows KP bytes apart, row0 its index in the
// slice.  One 16-byte load per row and QUAD of steps, UNQ quads issued together (tgb_dot16's weight bytes in flight at 2 rows per team,
// fewer with more rows), then what is left in halving blocks, and the 8-byte pair and the 4-byte single step of a segment's end loaded together.  Each step's weights are widened
// exactly right before its multiply-adds; per (row, lane) the chains are tgb_dot's.  The caller applies the layer's scale to the sums.
template <int G, int RB>
__device__ __forceinline__ void tgb_dot8(const unsigned char *__restrict__ rp, int KP, int row0, const float4 *lds4, int xi, int xs4, int nA, int nK, int q, float (&sa)[G],
                                         float (&sb)[G]) {
    constexpr int UNQ = G == 1 ? (RB <= 2 ? 4 : RB <= 4 ? 2 : 1) : (RB <= 2 ? 2 : 1);   // with 4 rows half, with 8 a quarter: no registers for more
    asm volatile("" : "+v"(xi));
    const float4 *xp = lds4 + xi;
    const unsigned char *row[G];
    const uint4 *wq[G];
#pragma unroll
    for (int g = 0; g < G; ++g) {
        row[g] = rp + (size_t)g * KP;
        wq[g] = (const uint4 *)row[g] + ((q + tg8_rot(row0 + g, KP)) & 15);
    }
    float a0[RB][G], a1[RB][G];
#pragma unroll
    for (int r = 0; r < RB; ++r)
#pragma unroll
        for (int g = 0; g < G; ++g) a0[r][g] = a1[r][g] = 0.0f;
    auto mac = [&](const float4 (&w)[G], int k) {
#pragma unroll
        for (int r = 0; r < RB; ++r) {
            const float4 x = xp[r * xs4 + k * 16];
#pragma unroll
            for (int g = 0; g < G; ++g) {
                a0[r][g] = fmaf(w[g].x, x.x, a0[r][g]); a1[r][g] = fmaf(w[g].y, x.y, a1[r][g]);
                a0[r][g] = fmaf(w[g].z, x.z, a0[r][g]); a1[r][g] = fmaf(w[g].w, x.w, a1[r][g]);
            }
        }
    };
    // one step from the dwords d[g] of the G rows
    auto step = [&](const unsigned (&d)[G], int k) {
        float4 w[G];
#pragma unroll
        for (int g = 0; g < G; ++g) w[g] = tg8_w4(d[g]);
        mac(w, k);
        __builtin_amdgcn_sched_barrier(0);
    };
    auto quad = [&](const uint4 (&wv)[G], int k) {
        unsigned d[G];
#pragma unroll
        for (int g = 0; g < G; ++g) d[g] = wv[g].x;
        step(d, k);
#pragma unroll
        for (int g = 0; g < G; ++g) d[g] = wv[g].y;
        step(d, k + 1);
#pragma unroll
        for (int g = 0; g < G; ++g) d[g] = wv[g].z;
        step(d, k + 2);
#pragma unroll
        for (int g = 0; g < G; ++g) d[g] = wv[g].w;
        step(d, k + 3);
    };
    // NQ quads of steps from step k: their weight loads are issued together
    auto block = [&](auto nq, int k) {
        constexpr int NQ = decltype(nq)::value;
        uint4 wv[NQ][G];
#pragma unroll
        for (int u = 0; u < NQ; ++u)
#pragma unroll
            for (int g = 0; g < G; ++g) wv[u][g] = wq[g][(k + 4 * u) * 4];
#pragma unroll
        for (int u = 0; u < NQ; ++u) quad(wv[u], k + 4 * u);
    };
    auto segment = [&](int k0, int k1) {
        int k = k0;
#pragma unroll 1
        for (; k + 4 * UNQ <= k1; k += 4 * UNQ) block(std::integral_constant<int, UNQ>{}, k);
        if constexpr (UNQ > 2) {
            if (k + 8 <= k1) { block(std::integral_constant<int, 2>{}, k); k += 8; }
        }
        if constexpr (UNQ > 1) {
            if (k + 4 <= k1) { block(std::integral_constant<int, 1>{}, k); k += 4; }
        }
        const int rem = k1 - k, ks = k + (rem & 2);
        uint2 wp[G];
        unsigned ws[G];
        if (rem & 2) {
#pragma unroll
            for (int g = 0; g < G; ++g) wp[g] = ((const uint2 *)(row[g] + 64 * k))[q];
        }
        if (rem & 1) {
#pragma unroll
            for (int g = 0; g < G; ++g) ws[g] = ((const unsigned *)(row[g] + 64 * ks))[q];
        }
        if (rem & 2) {
            unsigned d[G];
#pragma unroll
            for (int g = 0; g < G; ++g) d[g] = wp[g].x;
            step(d, k);
#pragma unroll
            for (int g = 0; g < G; ++g) d[g] = wp[g].y;
            step(d, k + 1);
        }
        if (rem & 1) step(ws, ks);
    };
    segment(0, nA);
#pragma unroll
    for (int r = 0; r < RB; ++r)
#pragma unroll
        for (int g = 0; g < G; ++g) {
            const float v = row_sum(a0[r][g] + a1[r][g]);
            sa[g] = (r == 0 || q == r) ? v : sa[g];
            a0[r][g] = a1[r][g] = 0.0f;
        }
    segment(nA, nK);
#pragma unroll
    for (int r = 0; r < RB; ++r)
#pragma unroll
        for (int g = 0; g < G; ++g) {
            const float v = row_sum(a0[r][g] + a1[r][g]);
            sb[g] = (r == 0 || q == r) ? v : sb[g];
        }
}

// tgb_dot on the block-sparse image, as tg_dots (loop_teamg.hip) is tg_dot's: rp = the unit's first image row, rows `rs` floats apart.  The
// index and the weight float4 of a list entry are loaded once and used by the RB rows; UNR entries' loads are issued together, then each
// entry's RB activation reads at the step its index names.  Per (row, lane) the chains are tgb_dot's without the steps of all-zero weights.
template <int G, int RB>
__device__ __forceinline__ void tgb_dots(const float *__restrict__ rp, int rs, const float4 *lds4, int xi, int xs4, int nA, int nK, int q, float (&sa)[G], float (&sb)[G]) {
    constexpr int UNR = G == 1 ? 4 : 2;
    asm volatile("" : "+v"(xi));
    const float4 *xp = lds4 + xi;
    const int idxf = (nK + 7) / 8 * 4;   // wrnn_teamg_sparse_idx_elems
    const unsigned short *ip[G];
    const float4 *wp[G];
#pragma unroll
    for (int g = 0; g < G; ++g) {
        ip[g] = (const unsigned short *)(rp + (size_t)g * rs);
        wp[g] = (const float4 *)(rp + (size_t)g * rs + idxf) + q;
    }
    float a0[RB][G], a1[RB][G];
#pragma unroll
    for (int r = 0; r < RB; ++r)
#pragma unroll
        for (int g = 0; g < G; ++g) a0[r][g] = a1[r][g] = 0.0f;
    // every row has its own list: the activation reads are per (row of the batch, row of the unit)
    auto mac = [&](const float4 (&w)[G], const int (&id)[G]) {
#pragma unroll
        for (int r = 0; r < RB; ++r) {
#pragma unroll
            for (int g = 0; g < G; ++g) {
                const float4 x = xp[r * xs4 + id[g] * 16];
                a0[r][g] = fmaf(w[g].x, x.x, a0[r][g]); a1[r][g] = fmaf(w[g].y, x.y, a1[r][g]);
                a0[r][g] = fmaf(w[g].z, x.z, a0[r][g]); a1[r][g] = fmaf(w[g].w, x.w, a1[r][g]);
            }
        }
    };
    auto segment = [&](int j0, int j1) {
        int j = j0;
#pragma unroll 1
        for (; j + UNR <= j1; j += UNR) {
            int id[UNR][G];
            float4 w[UNR][G];
#pragma unroll
            for (int u = 0; u < UNR; ++u)
#pragma unroll
                for (int g = 0; g < G; ++g) id[u][g] = ip[g][j + u];
#pragma unroll
            for (int u = 0; u < UNR; ++u)
#pragma unroll
                for (int g = 0; g < G; ++g) w[u][g] = wp[g][(j + u) * 16];
#pragma unroll
            for (int u = 0; u < UNR; ++u) {
                mac(w[u], id[u]);
                __builtin_amdgcn_sched_barrier(0);
            }
        }
#pragma unroll 1
        for (; j < j1; ++j) {
            int id[G];
            float4 w[G];
#pragma unroll
            for (int g = 0; g < G; ++g) { id[g] = ip[g][j]; w[g] = wp[g][j * 16]; }
            mac(w, id);
        }
    };
    segment(0, nA);
#pragma unroll
    for (int r = 0; r < RB; ++r)
#pragma unroll
        for (int g = 0; g < G; ++g) {
            const float v = row_sum(a0[r][g] + a1[r][g]);
            sa[g] = (r == 0 || q == r) ? v : sa[g];
            a0[r][g] = a1[r][g] = 0.0f;
        }
    segment(nA, nK);
#pragma unroll
    for (int r = 0; r < RB; ++r)
#pragma unroll
        for (int g = 0; g < G; ++g) {
            const float v = row_sum(a0[r][g] + a1[r][g]);
            sb[g] = (r == 0 || q == r) ? v : sb[g];
        }
}

// G rows from row `row0` of a layer's slice at `base` (LDS or device memory), KP elements each, in the image's element type; `scale` is the
// layer's (e4m3 only, a power of two).  TgSparse: KP = the floats of an image row, nA / nK count list entries
template <int G, int RB, typename WT>
__device__ __forceinline__ void tgb_rows(const WT *base, int row0, int KP, float scale, const float4 *lds4, int xi, int xs4, int nA, int nK, int q, float (&sa)[G],
                                         float (&sb)[G]) {
    if constexpr (std::is_same<WT, TgSparse>::value) tgb_dots<G, RB>((const float *)base + (size_t)row0 * KP, KP, lds4, xi, xs4, nA, nK, q, sa, sb);
    else if constexpr (sizeof(WT) == 4) tgb_dot<G, RB>((const float4 *)(base + (size_t)row0 * KP) + q, KP / 4, lds4, xi, xs4, nA, nK, q, sa, sb);
    else if constexpr (sizeof(WT) == 2) tgb_dot16<G, RB>((const TgHalf8 *)(base + (size_t)row0 * KP), KP / 8, row0, lds4, xi, xs4, nA, nK, q, sa, sb);
    else {
        tgb_dot8<G, RB>((const unsigned char *)(base + (size_t)row0 * KP), KP, row0, lds4, xi, xs4, nA, nK, q, sa, sb);
#pragma unroll
        for (int g = 0; g < G; ++g) { sa[g] *= scale; sb[g] *= scale; }
    }
}

template <int RB, typename WT>
__global__ void __launch_bounds__(TG_THREADS) loop_teamg_batch_kernel(WrnnTeamGBatchArgs ta) {
    extern __shared__ __attribute__((aligned(16))) char smem_tgb[];
    float *lds = (float *)smem_tgb;
    const WrnnLoopArgs &a = ta.a;
    const WrnnDims d = a.d;
    const TgbLay ly(d, RB);
    const int H = d.H, FC = d.FC, F = d.F, A = d.A, RA = d.R, NC = d.NC, HOP = d.HOP, ND = d.ND, P = d.P;
    const int HP = ly.v.HP, XAP = ly.v.XAP, FCP = ly.v.FCP, CB = ly.v.CB;
    const int rowf = ly.rowf, xs4 = ly.rowf / 4;
    float *misc = lds + ly.misc;
    int *misc_i = (int *)misc;
    float *gsum = lds + ly.gs, *race = lds + ly.race;
    int *race_i = (int *)race;
    WT *wres = (WT *)(lds + ly.total);   // resident weights, in the image's element type
    constexpr bool SP = std::is_same<WT, TgSparse>::value;   // the block-sparse image: a layer's steps are its list entries

    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    int qw = tid >> 4, q = tid & 15;   // not const: see the top of the step loop

    // ---- team formation (team_common.h) ----
    const int n_batches = (a.n_rows + ta.rpb - 1) / ta.rpb;
    int team, g;
    if (!join_team(ta.ctl, a.err, misc_i, ta.n_teams, team, g) || team >= n_batches) return;
    u64 *mail = ta.mail + (size_t)team * ta.plan.mail_granules;
    const unsigned G1 = (unsigned)(ta.plan.mail_granules / RB);   // granules of one row: row r's regions start at r * G1
    // mailbox regions of a row (granules), two parities each
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

    auto owned = [&](const WrnnTeamGLayer &L) -> int {
        int n = L.N - g * L.U;
        return n < 0 ? 0 : (n > L.U ? L.U : n);
    };
    // m_t, a_t of step t of every slot's row (:203-206) into parity `par` of its conditioning buffer, as loop_teamg.hip; zero past the
    // row's own utterance (:327-330) and for an empty slot
    auto cond_fill = [&](int64_t t, unsigned par) {
        const float *ktab = w + a.off.ktab;
        const int per = F + RA;
        for (int idx = tid; idx < RB * per; idx += TG_THREADS) {
            const int r = idx / per, j = idx - r * per;
            const int row = misc_i[MB_ROW + r];
            float v = 0.0f;
            if (row >= 0) {
                const int utt = misc_i[MB_UTT + r];
                const float *mel_b = a.mels + (size_t)utt * F * a.mel_T;
                const float *aux_b = a.aux_frames + (size_t)utt * a.T * RA;
                const int64_t pos = ((const int64_t *)(misc + MB_START))[r] + t;
                const bool live = a.frames ? pos < (int64_t)a.frames[utt] * HOP && pos < a.total_len : pos < a.total_len;
                if (live) {
                    const int i = (int)(pos / HOP);
                    const int rr = (int)(pos - (int64_t)i * HOP);
                    if (j < F) {
                        for (int k = 0; k < ND; ++k) {
                            const int fr = i + k - P + a.mel_off;
                            const float mv = (fr >= 0 && fr < a.mel_T) ? mel_b[(size_t)j * a.mel_T + fr] : 0.0f;
                            v = fmaf(ktab[rr * ND + k], mv, v);
                        }
                    } else {
                        v = aux_b[(size_t)i * RA + (j - F)];
                    }
                }
            }
            lds[r * rowf + ly.v.cb + par * CB + j] = v;
        }
    };
    // the own rows of W_I[:, 1:] . [m | a1] + b_I for the step whose conditioning is in parity `par` -> every row's mailbox, tagged `tag`
    auto xc_publish = [&](unsigned par, unsigned tag) {
        const WrnnTeamGLayer &L = ta.plan.L[WRNN_TEAMG_COND];
        const int nown = owned(L), nK = SP ? tg_sp_nk(ta.plan, ta.sp, L) : L.KP / 64;
        const int xi = (ly.v.cb + par * CB) / 4 + q;
        for (int ul = qw; ul < nown; ul += 32) {
            float sa[1], sb[1];
            if (ul < L.nres) tgb_rows<1, RB>(wres + L.lds_off, ul, L.KP, L.scale, (const float4 *)lds, xi, xs4, nK, nK, q, sa, sb);
            else tgb_rows<1, RB>(img + L.img_off, ul, L.KP, L.scale, (const float4 *)lds, xi, xs4, nK, nK, q, sa, sb);
            const int j = g * L.U + ul;
            if (q < RB) tg_st_granule<WT>(mail, q * G1 + M_XC + (tag & 1u) * HP + j, tag, __float_as_uint(sa[0] + w[a.off.I_b + j]));
        }
    };
    // one GRU layer (get_gru_cell :273-279, gate rows [r; z; n]): h' of the own units of every row -> mailbox.  A row's input is
    // [input (KAP) | h (HP)] at xoff of its vectors.  By gate row or by unit as in loop_teamg.hip.
    auto gru_phase = [&](const WrnnTeamGLayer &L, int xoff, size_t obih, size_t obhh, unsigned region, unsigned epoch) {
        const int nown = owned(L), nA = SP ? tg_sp_na(ta.plan, ta.sp, L) : L.KAP / 64, nK = SP ? tg_sp_nk(ta.plan, ta.sp, L) : L.KP / 64;
        const int xi = xoff / 4 + q;
        const float *bi = w + obih, *bh = w + obhh;
        auto cell = [&](int r, int j, const float (&gi)[3], const float (&gh)[3]) {
            const float rg = 1.0f / (1.0f + expf(-((gi[0] + bi[j]) + (gh[0] + bh[j]))));
            const float zg = 1.0f / (1.0f + expf(-((gi[1] + bi[H + j]) + (gh[1] + bh[H + j]))));
            const float ng = tanhf((gi[2] + bi[2 * H + j]) + rg * (gh[2] + bh[2 * H + j]));
            const float hn = (1.0f - zg) * ng + zg * lds[r * rowf + xoff + L.KAP + j];
            tg_st_granule<WT>(mail, r * G1 + region + (epoch & 1u) * HP + j, epoch, __float_as_uint(hn));
        };
        if (L.U <= 16) {
            for (int task = qw; task < 3 * nown; task += 32) {
                const int ul = task / 3;
                float sa[1], sb[1];
                if (ul < L.nres) tgb_rows<1, RB>(wres + L.lds_off, task, L.KP, L.scale, (const float4 *)lds, xi, xs4, nA, nK, q, sa, sb);
                else tgb_rows<1, RB>(img + L.img_off, task, L.KP, L.scale, (const float4 *)lds, xi, xs4, nA, nK, q, sa, sb);
                if (q < RB) { gsum[q * 128 + 2 * task] = sa[0]; gsum[q * 128 + 2 * task + 1] = sb[0]; }
            }
            __syncthreads();
            for (int idx = tid; idx < RB * nown; idx += TG_THREADS) {
                const int r = idx / nown, ul = idx - r * nown;
                const float *gs = gsum + r * 128 + 6 * ul;
                const float gi[3] = {gs[0], gs[2], gs[4]}, gh[3] = {gs[1], gs[3], gs[5]};
                cell(r, g * L.U + ul, gi, gh);
            }
        } else {
            for (int ul = qw; ul < nown; ul += 32) {
                float gi[3] = {0.0f, 0.0f, 0.0f}, gh[3] = {0.0f, 0.0f, 0.0f};
                if constexpr (RB <= 4) {
                    if (ul < L.nres) tgb_rows<3, RB>(wres + L.lds_off, ul * 3, L.KP, L.scale, (const float4 *)lds, xi, xs4, nA, nK, q, gi, gh);
                    else tgb_rows<3, RB>(img + L.img_off, ul * 3, L.KP, L.scale, (const float4 *)lds, xi, xs4, nA, nK, q, gi, gh);
                } else {
                    // 8 rows x 3 gates x (a0, a1) would not leave room for the loads in flight: gate by gate, the same sums
#pragma unroll 1
                    for (int gt = 0; gt < 3; ++gt) {
                        float sa[1], sb[1];
                        if (ul < L.nres) tgb_rows<1, RB>(wres + L.lds_off, ul * 3 + gt, L.KP, L.scale, (const float4 *)lds, xi, xs4, nA, nK, q, sa, sb);
                        else tgb_rows<1, RB>(img + L.img_off, ul * 3 + gt, L.KP, L.scale, (const float4 *)lds, xi, xs4, nA, nK, q, sa, sb);
                        gi[0] = gt == 0 ? sa[0] : gi[0]; gi[1] = gt == 1 ? sa[0] : gi[1]; gi[2] = gt == 2 ? sa[0] : gi[2];
                        gh[0] = gt == 0 ? sb[0] : gh[0]; gh[1] = gt == 1 ? sb[0] : gh[1]; gh[2] = gt == 2 ? sb[0] : gh[2];
                    }
                }
                if (q < RB) cell(q, g * L.U + ul, gi, gh);
            }
        }
    };
    // relu(W . x + b) of the own rows, every row -> mailbox
    auto fc_phase = [&](const WrnnTeamGLayer &L, int xoff, size_t ob, unsigned region, unsigned epoch) {
        const int nown = owned(L), nK = SP ? tg_sp_nk(ta.plan, ta.sp, L) : L.KP / 64;
        const int xi = xoff / 4 + q;
        for (int ul = qw; ul < nown; ul += 32) {
            float sa[1], sb[1];
            if (ul < L.nres) tgb_rows<1, RB>(wres + L.lds_off, ul, L.KP, L.scale, (const float4 *)lds, xi, xs4, nK, nK, q, sa, sb);
            else tgb_rows<1, RB>(img + L.img_off, ul, L.KP, L.scale, (const float4 *)lds, xi, xs4, nK, nK, q, sa, sb);
            const int j = g * L.U + ul;
            if (q < RB) tg_st_granule<WT>(mail, q * G1 + region + (epoch & 1u) * FCP + j, epoch, __float_as_uint(fmaxf(sa[0] + w[ob + j], 0.0f)));
        }
    };
    // all N values of an exchanged vector of every row: 64 granules of one row per wave and turn (RB * ceil(N / 64) turns over the 8
    // waves); whole waves take part, lanes past N re-read granule N - 1
    auto gather = [&](unsigned region, int N, unsigned epoch, bool &dead, unsigned code, auto &&put) {
        const int nch = (N + 63) >> 6;
        for (int task = wave; task < RB * nch; task += TG_THREADS / 64) {
            const int r = task / nch, j = (task - r * nch) * 64 + lane;
            const float v = take_staggered(mail, r * G1 + region + (unsigned)(j < N ? j : N - 1), epoch, dead, a.err, code);
            if (j < N) put(r, j, v);
        }
    };

    bool dead = false;
    unsigned epoch = 0;
    const int n_pass = (n_batches + ta.n_teams - 1) / ta.n_teams;
    for (int pass = 0; pass < n_pass; ++pass) {
        const int batch = pass * ta.n_teams + ((ta.snake && (pass & 1)) ? ta.n_teams - 1 - team : team);
        if (batch >= n_batches) continue;
        __syncthreads();
        // the batch's rows: slot r -> row, its steps, utterance, start and Philox key; x = x_init or 0, h1 = h2 = 0 (:194-196)
        if (tid < RB) {
            const int slot = batch * ta.rpb + tid;
            int row = (tid < ta.rpb && slot < a.n_rows) ? ta.order[slot] : -1;
            if (row >= a.n_rows) row = -1;
            WrnnRow rw{0, 0, 0};
            uint64_t kseed = a.seed;
            uint32_t krow = (uint32_t)row;
            if (row >= 0) {
                rw = a.rows[row];
                if (a.keys) { const WrnnRowKey k = a.keys[row]; kseed = k.seed; krow = k.row; }
            }
            misc_i[MB_ROW + tid] = row;
            misc_i[MB_STEPS + tid] = rw.steps;
            misc_i[MB_UTT + tid] = rw.utt;
            ((int64_t *)(misc + MB_START))[tid] = rw.start;
            ((uint64_t *)(misc + MB_SEED))[tid] = kseed;
            misc_i[MB_KROW + tid] = (int)krow;
            misc[MB_X + tid] = (row >= 0 && a.x_init) ? a.x_init[row] : 0.0f;
        }
        for (int idx = tid; idx < RB * HP; idx += TG_THREADS) {
            const int r = idx / HP, j = idx - r * HP;
            float *v = lds + r * rowf;
            v[ly.v.xh1 + HP + j] = 0.0f; v[ly.v.xh1 + 3 * HP + j] = 0.0f;
            v[ly.v.xh2 + XAP + j] = 0.0f; v[ly.v.xh2 + 2 * XAP + HP + j] = 0.0f;
        }
        __syncthreads();
        int bsteps = 0;
#pragma unroll
        for (int r = 0; r < RB; ++r) bsteps = misc_i[MB_STEPS + r] > bsteps ? misc_i[MB_STEPS + r] : bsteps;
        if (bsteps < 1) continue;
        cond_fill(a.seg0, (epoch + 1u) & 1u);
        __syncthreads();
        xc_publish((epoch + 1u) & 1u, epoch + 1u);

        for (int64_t t = a.seg0; t < a.seg0 + bsteps; ++t) {
            ++epoch;
            const unsigned par = epoch & 1u;
            // Everything a phase derives from the lane's place in its group is cheap to make and, as an invariant of this loop, would be
            // kept in registers across the whole step for every phase at once: hide the two values from the optimiser once per step.
            asm volatile("" : "+v"(q), "+v"(qw));
            // offsets inside a row's vectors
            const int xh1 = ly.v.xh1 + par * 2 * HP, xh1n = ly.v.xh1 + (par ^ 1u) * 2 * HP;
            const int xh2 = ly.v.xh2 + par * (XAP + HP), xh2n = ly.v.xh2 + (par ^ 1u) * (XAP + HP);
            const int cbp = ly.v.cb + par * CB, f1 = ly.v.f1, f2 = ly.v.f2, f3 = ly.v.f3;
            const bool more = t + 1 < a.seg0 + bsteps;

            // ---- conditioning: a2 / a3 / a4 of this step into the layer inputs ----
            for (int idx = tid; idx < RB * A; idx += TG_THREADS) {
                const int r = idx / A, j = idx - r * A;
                float *v = lds + r * rowf;
                v[xh2 + H + j] = v[cbp + F + A + j];        // a2_t :213
                v[f1 + H + j] = v[cbp + F + 2 * A + j];     // a3_t :217
                v[f2 + FC + j] = v[cbp + F + 3 * A + j];    // a4_t :220
            }
            // ---- x = I(cat[x_{t-1}, m_t, a1_t]) :208-209: the exchanged conditioning share + the sample's column ----
            {
                const float *wI0 = w + a.off.I_t;   // row 0 of the [in][out] layout = W_I[:, 0]
                gather(M_XC + par * HP, H, epoch, dead, 10u, [&](int r, int j, float v) { lds[r * rowf + xh1 + j] = fmaf(wI0[j], misc[MB_X + r], v); });
            }
            __syncthreads();
            // ---- 1. h1 = rnn1(x, h1); x = x + h1 :210-212 ----
            gru_phase(ta.plan.L[WRNN_TEAMG_RNN1], xh1, a.off.r1_bih, a.off.r1_bhh, M_H1, epoch);
            if (more) cond_fill(t + 1, par ^ 1u);    // m, a of the next step, under the round trip of exchange 1
            gather(M_H1 + par * HP, H, epoch, dead, 11u, [&](int r, int j, float v) {
                float *x = lds + r * rowf;
                x[xh1n + HP + j] = v; x[xh2 + j] = x[xh1 + j] + v;
            });
            __syncthreads();
            // ---- 2. h2 = rnn2(cat[x, a2_t], h2); x = x + h2 :213-216 ----
            gru_phase(ta.plan.L[WRNN_TEAMG_RNN2], xh2, a.off.r2_bih, a.off.r2_bhh, M_H2, epoch);
            if (more) xc_publish(par ^ 1u, epoch + 1u);   // beside the chain, under exchange 2: read at the start of the next step
            gather(M_H2 + par * HP, H, epoch, dead, 12u, [&](int r, int j, float v) {
                float *x = lds + r * rowf;
                x[xh2n + XAP + j] = v; x[f1 + j] = x[xh2 + j] + v;
            });
            __syncthreads();
            // ---- 3. / 4. x = relu(fc1(cat[x, a3_t])); x = relu(fc2(cat[x, a4_t])) :217-221 ----
            fc_phase(ta.plan.L[WRNN_TEAMG_FC1], f1, a.off.fc1_b, M_F1, epoch);
            gather(M_F1 + par * FCP, FC, epoch, dead, 13u, [&](int r, int j, float v) { lds[r * rowf + f2 + j] = v; });
            __syncthreads();
            fc_phase(ta.plan.L[WRNN_TEAMG_FC2], f2, a.off.fc2_b, M_F2, epoch);
            gather(M_F2 + par * FCP, FC, epoch, dead, 14u, [&](int r, int j, float v) { lds[r * rowf + f3 + j] = v; });
            __syncthreads();
            // ---- 5. logits = fc3(x) :223 of the own classes, and the sampler :225-237.  Lane r of a group: row r ----
            {
                const WrnnTeamGLayer &L = ta.plan.L[WRNN_TEAMG_FC3];
                const int nown = owned(L), nK = SP ? tg_sp_nk(ta.plan, ta.sp, L) : L.KP / 64;
                const int xi = f3 / 4 + q;
                const int qr = q < RB ? q : 0;
                const int row = q < RB ? misc_i[MB_ROW + qr] : -1;
                const bool act = row >= 0 && t < a.seg0 + misc_i[MB_STEPS + qr];   // the row is still running: it reads its noise and writes
                const uint64_t kseed = ((const uint64_t *)(misc + MB_SEED))[qr];
                const uint32_t krow = (uint32_t)misc_i[MB_KROW + qr];
                float bv = -INFINITY;
                int bi = 0x7fffffff;
                for (int ul = qw; ul < nown; ul += 32) {
                    float sa[1], sb[1];
                    if (ul < L.nres) tgb_rows<1, RB>(wres + L.lds_off, ul, L.KP, L.scale, (const float4 *)lds, xi, xs4, nK, nK, q, sa, sb);
                    else tgb_rows<1, RB>(img + L.img_off, ul, L.KP, L.scale, (const float4 *)lds, xi, xs4, nK, nK, q, sa, sb);
                    if (q < RB) {
                        const int c = g * L.U + ul;
                        const float lg = sa[0] + w[a.off.fc3_b + c];
                        if (a.logits_out && act) a.logits_out[((size_t)t * a.n_rows + row) * NC + c] = lg;
                        if (d.mode == WRNN_MODE_RAW) {
                            // Categorical(softmax(logits)).sample() == argmax_k logit_k - log q_k, q ~ Exp(1) (loop_simple.hip)
                            float v = lg;
                            if (act && a.noise_mode == WRNN_NOISE_INJECTED) v -= logf(a.noise1[((size_t)t * a.n_rows + row) * NC + c]);
                            else if (act && a.noise_mode == WRNN_NOISE_PHILOX) v -= logf(-logf(wrnn_uniform_raw(kseed, (uint64_t)t, krow, (uint32_t)c)));
                            if (v > bv) { bv = v; bi = c; }   // classes ascend: ties keep the lowest
                        } else {
                            tg_st_granule<WT>(mail, q * G1 + M_CAND + par * 64 + c, epoch, __float_as_uint(lg));
                        }
                    }
                }
                if (d.mode == WRNN_MODE_RAW && q < RB) { race[q * 64 + qw] = bv; race_i[q * 64 + 32 + qw] = bi; }
            }
            if (d.mode == WRNN_MODE_RAW) __syncthreads();
            if (wave < RB) {   // wave r: the race or the sampler of row r
                const int r = wave;
                const int row = misc_i[MB_ROW + r];
                const bool act = row >= 0 && t < a.seg0 + misc_i[MB_STEPS + r];
                const unsigned cand = r * G1 + M_CAND + par * 64;
                if (d.mode == WRNN_MODE_RAW) {
                    float v = lane < 32 ? race[r * 64 + lane] : -INFINITY;
                    int k = lane < 32 ? race_i[r * 64 + 32 + lane] : 0x7fffffff;
                    wave_argmax(v, k);
                    if (lane == 0) {   // the workgroup's candidate: granule g = value, 32 + g = class
                        tg_st_granule<WT>(mail, cand + g, epoch, __float_as_uint(v));
                        tg_st_granule<WT>(mail, cand + 32 + g, epoch, (unsigned)k);
                    }
                    const float pv = take_staggered(mail, cand + lane, epoch, dead, a.err, 15u);
                    const int ck = __shfl(__float_as_int(pv), (lane + 32) & 63, 64);
                    v = lane < 32 ? pv : -INFINITY;
                    k = lane < 32 ? ck : 0x7fffffff;
                    wave_argmax(v, k);
                    if (lane == 0) {
                        const float smp = 2.0f * (float)k / ((float)NC - 1.0f) - 1.0f;   // :235
                        if (g == 0 && act) {
                            if (a.labels_out) a.labels_out[(size_t)row * a.steps + t] = k;
                            a.samples_out[(size_t)row * a.steps + t] = smp;
                        }
                        misc[MB_X + r] = (a.x_forced && act) ? a.x_forced[(size_t)t * a.n_rows + row] : smp;
                    }
                } else {
                    // sample_from_discretized_mix_logistic (wavernn/utils/distribution.py:87-123) on the 3 * nr exchanged outputs, in every workgroup
                    const int nr = NC / 3;
                    const uint64_t kseed = ((const uint64_t *)(misc + MB_SEED))[r];
                    const uint32_t krow = (uint32_t)misc_i[MB_KROW + r];
                    const float lg = take_staggered(mail, cand + (lane < NC ? lane : NC - 1), epoch, dead, a.err, 15u);
                    float v = -INFINITY;
                    int k = 0x7fffffff;
                    if (lane < nr) {
                        float u1 = 0.5f;
                        if (act) {
                            if (a.noise_mode == WRNN_NOISE_INJECTED) u1 = a.noise1[((size_t)t * a.n_rows + row) * nr + lane];
                            else u1 = wrnn_uniform_mol(kseed, (uint64_t)t, krow, (uint32_t)lane);
                        }
                        v = lg - logf(-logf(u1));   // :107
                        k = lane;
                    }
                    wave_argmax(v, k);
                    k = k < nr ? k : 0;   // only after a timed-out exchange
                    const float mean = __shfl(lg, nr + k, 64);                                  // :113
                    const float ls = fmaxf(__shfl(lg, 2 * nr + k, 64), -32.23619130191664f);   // log(1e-14) :114-115
                    if (lane == 0) {
                        float u2 = 0.5f;
                        if (act) {
                            if (a.noise_mode == WRNN_NOISE_INJECTED) u2 = a.noise2[(size_t)t * a.n_rows + row];
                            else u2 = wrnn_uniform_mol(kseed, (uint64_t)t, krow, 10u);
                        }
                        float xs = mean + expf(ls) * (logf(u2) - logf(1.0f - u2));  // :119
                        xs = fminf(fmaxf(xs, -1.0f), 1.0f);                         // :121
                        if (g == 0 && act) {
                            if (a.labels_out) a.labels_out[(size_t)row * a.steps + t] = k;
                            a.samples_out[(size_t)row * a.steps + t] = xs;
                        }
                        misc[MB_X + r] = (a.x_forced && act) ? a.x_forced[(size_t)t * a.n_rows + row] : xs;
                    }
                }
            }
            if ((epoch & 63u) == 0u && dead && lane == 0) misc_i[M_DEAD] = 1;   // bounded-spin bail-out, checked workgroup-wide every 64 samples
            __syncthreads();
            if ((epoch & 63u) == 0u && misc_i[M_DEAD]) return;
        }
    }
}

template <int RB>
const void *tgb_fn(int esz, bool sparse) {
    if (sparse) return (const void *)loop_teamg_batch_kernel<RB, TgSparse>;
    return esz == 4 ? (const void *)loop_teamg_batch_kernel<RB, float>
                    : esz == 2 ? (const void *)loop_teamg_batch_kernel<RB, _Float16> : (const void *)loop_teamg_batch_kernel<RB, TgE4m3>;
}
const void *tgb_kernel_fn(int rb, int esz, bool sparse) {
    return rb == 2 ? tgb_fn<2>(esz, sparse) : rb == 4 ? tgb_fn<4>(esz, sparse) : rb == 8 ? tgb_fn<8>(esz, sparse) : nullptr;
}

template <int RB, typename WT>
void tgb_launch(const WrnnTeamGBatchArgs &a, size_t lds, hipStream_t s) {
    hipLaunchKernelGGL((loop_teamg_batch_kernel<RB, WT>), dim3(a.n_teams * TEAM_WGS), dim3(TG_THREADS), lds, s, a);
}
template <int RB>
void tgb_launch_fmt(const WrnnTeamGBatchArgs &a, size_t lds, hipStream_t s) {
    if (a.sp.on) tgb_launch<RB, TgSparse>(a, lds, s);
    else if (a.plan.esz == 4) tgb_launch<RB, float>(a, lds, s);
    else if (a.plan.esz == 2) tgb_launch<RB, _Float16>(a, lds, s);
    else tgb_launch<RB, TgE4m3>(a, lds, s);
}

}  // namespace

hipError_t wrnn_teamg_batch_occupancy(const WrnnTeamGPlan &p, int rb, int *blocks_per_cu, bool sparse) {
    const size_t lds = wrnn_teamg_lds_bytes(p);
    const void *fn = tgb_kernel_fn(rb, p.esz, sparse);
    if (!fn) return hipErrorInvalidValue;
    hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
    return hipOccupancyMaxActiveBlocksPerMultiprocessor(blocks_per_cu, fn, TG_THREADS, lds);
}

hipError_t wrnn_launch_loop_teamg_batch(const WrnnTeamGBatchArgs &a, int rb, hipStream_t s) {
    (void)hipGetLastError();
    const size_t lds = wrnn_teamg_lds_bytes(a.plan);
    const void *fn = tgb_kernel_fn(rb, a.plan.esz, a.sp.on != 0);
    if (!fn) return hipErrorInvalidValue;
    hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
    if (rb == 2) tgb_launch_fmt<2>(a, lds, s);
    else if (rb == 4) tgb_launch_fmt<4>(a, lds, s);
    else tgb_launch_fmt<8>(a, lds, s);
    return hipGetLastError();
}
