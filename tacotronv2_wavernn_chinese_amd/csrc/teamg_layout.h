// LDS carve-up of the two team kernels for any dims: TgLay (loop_teamg.hip, one row per team) and TgbLay (loop_teamg_batch.hip, RB rows
// per team in lock-step).  wrnn_teamg_make_plan sizes the resident weights by what these leave of 160 KiB.  The vectors are fp32 whatever
// the element type of the weight image.
#pragma once
#include <type_traits>

#include "team_common.h"
#include "wrnn_internal.h"

#define TG_THREADS WRNN_TEAMG_THREADS
#define TG_LDS_MAX (160 * 1024)

namespace {

__host__ __device__ inline int tg_r64(int n) { return (n + 63) & ~63; }

// LDS carve-up of the activation vectors (floats); every vector is padded with zeros to the padded row length of the layer it feeds
struct TgLay {
    int HP, XAP, FAP, FCP, CK, CB;
    int xh1, xh2, f1, f2, f3, cb, gs, misc, total;
    __host__ __device__ TgLay(const WrnnDims &d) {
        HP = tg_r64(d.H); XAP = tg_r64(d.H + d.A); FAP = tg_r64(d.FC + d.A); FCP = tg_r64(d.FC); CK = tg_r64(d.F + d.A);
        CB = tg_r64(d.F + d.R) > CK ? tg_r64(d.F + d.R) : CK;
        int o = 0;
        xh1 = o; o += 2 * (HP + HP);     // [parity][x (HP) | h1 (HP)]            input of rnn1
        xh2 = o; o += 2 * (XAP + HP);    // [parity][x2 | a2_t (XAP) | h2 (HP)]   input of rnn2
        f1 = o; o += XAP;                // [x3 | a3_t]                           input of fc1
        f2 = o; o += FAP;                // [relu(fc1) | a4_t]                    input of fc2
        f3 = o; o += FCP;                // relu(fc2)                             input of fc3
        cb = o; o += 2 * CB;             // [parity][m_t (F) | a_t (R)]           conditioning of a step; its head is the input of I
        gs = o; o += 128;                // [16 units][3 gates][segment A sum, segment B sum] of a GRU layer split by gate rows
        misc = o; o += 128;              // 0-2 team / rank / bail-out (team_common.h), 8 x_{t-1}, 32-63 race values, 64-95 race classes
        total = o;
    }
};

// RB rows in lock-step: row r's vectors are TgLay's, with the same offsets, at r * rowf; behind them what the workgroup keeps once per
// row (gate-row sums, race candidates) and once (misc).  Rows are the slow index, so a 16-lane group reads row r's float4 q, q + 16, ...
// exactly as the one-row kernel does: consecutive, conflict-free.
struct TgbLay {
    TgLay v;
    int rowf;      // floats of one row's vectors (v.xh1 .. v.cb)
    int gs;        // [RB][128]   gate-row sums of a GRU layer split by gate rows
    int race;      // [RB][64]    0-31 race values, 32-63 race classes of the 32 lane groups
    int misc;      // 128: 0-2 team / rank / bail-out, then per row (8 each): 8 x_{t-1}, 16 row index or -1, 24 steps, 32 utt, 40 start (int64),
                   // 56 Philox seed (uint64), 72 Philox row
    int total;
    __host__ __device__ TgbLay(const WrnnDims &d, int RB) : v(d) {
        rowf = v.gs;
        int o = RB * rowf;
        gs = o; o += RB * 128;
        race = o; o += RB * 64;
        misc = o; o += 128;
        total = o;
    }
};
// The fp16 image.  A row of the fp32 image is KP floats in order: at step k of a dot product lane q of a 16-lane group loads elements
// 4 (q + 16 k) .. + 3, one float4.  The fp16 image holds the same elements as IEEE binary16, permuted inside the row so that ONE 16-byte
// load covers the lane's elements of TWO consecutive steps -- the bytes in flight per load, and the width of an LDS read, stay those of
// the fp32 kernel:
//   * a row is two segments of steps, [0, nA) and [nA, nK) (the operands a GRU's n gate needs apart; nA = nK for the other layers), and
//     steps pair up inside a segment: pair j of the segment that starts at step k0 is steps k0 + 2 j and k0 + 2 j + 1.  It takes the 256
//     bytes from byte 128 (k0 + 2 j) of the row; lane q's 16 bytes are piece q ^ s of those 16 pieces: 4 halves of the first step, then 4
//     of the second;
//   * a segment with an odd number of steps ends in one unpaired step, stored as in the fp32 image: lane q's 4 halves at halves
//     64 k + 4 q .. + 3 (an 8-byte load);
//   * s = 8 for an odd row (counted inside the workgroup's slice of the layer) of a layer whose KP / 64 is odd, else 0.  Rows are
//     KP * 2 bytes apart, so consecutive rows of such a layer start 128 bytes apart modulo the 256 bytes the 64 LDS banks span, and the
//     16-lane groups that one ds_read_b128 serves together -- lanes 0-3 and 12-15 of one row with lanes 4-11 of the next -- would meet
//     on the same banks.  Swapping the two 128-byte halves of every pair in the odd rows puts them back on disjoint banks: every
//     resident row is read conflict-free, as in the fp32 kernel, whose rows are a multiple of 256 bytes apart.
// The permutation only moves bytes (tg16_pos below is what wrnn_teamg_pack writes by and the dot products read by): each lane still gets
// the elements 4 (q + 16 k) .. + 3 at step k, k ascending, and widens them exactly -- every binary16 value, subnormals included, is an
// fp32 value -- so its multiply-adds see the operands they would see with the rounded matrix stored as fp32.
typedef _Float16 TgHalf4 __attribute__((ext_vector_type(4)));
typedef _Float16 TgHalf8 __attribute__((ext_vector_type(8)));
__device__ __forceinline__ float4 tg_w4(const TgHalf4 &w) { return make_float4((float)w.x, (float)w.y, (float)w.z, (float)w.w); }
__device__ __forceinline__ float4 tg_lo4(const TgHalf8 &w) { return make_float4((float)w[0], (float)w[1], (float)w[2], (float)w[3]); }
__device__ __forceinline__ float4 tg_hi4(const TgHalf8 &w) { return make_float4((float)w[4], (float)w[5], (float)w[6], (float)w[7]); }
// 8 for the rows whose pairs are stored with their halves swapped
__host__ __device__ inline int tg16_swz(int row, int KP) { return (row & (KP >> 6) & 1) << 3; }
// where element p of row `row` (KAP = elements of segment A, KP = of the row; both multiples of 64) lives in the row of the fp16 image
__host__ __device__ inline int tg16_pos(int p, int row, int KAP, int KP) {
    const int k = p >> 6, q = (p >> 2) & 15, c = p & 3;
    const int k0 = p < KAP ? 0 : KAP >> 6, k1 = p < KAP ? KAP >> 6 : KP >> 6;
    const int rel = k - k0;
    if (((k1 - k0) & 1) && rel == k1 - k0 - 1) return p;   // the unpaired last step of a segment
    return 64 * (k - (rel & 1)) + 8 * (q ^ tg16_swz(row, KP)) + 4 * (rel & 1) + c;
}

// The e4m3 image (WRNN_WEIGHTS_E4M3).  The same elements as OCP e4m3fn bytes, each layer divided by its power-of-two scale
// beforehand; a row is KP bytes.  The steps of a segment go in QUADS: quad j of the segment that starts at step k0 is steps k0 + 4 j ..
// + 3 and takes the 256 bytes from byte 64 (k0 + 4 j) of the row; lane q's 16 bytes are piece (q + rot) & 15 of those 16 pieces: its 4
// bytes of the first step, then of the second, third and fourth -- ONE 16-byte load for four steps.  What is left of a segment goes as one
// PAIR (128 bytes, lane q's 8 bytes are piece q: 4 bytes of the first step, 4 of the second; an 8-byte load) and then one SINGLE step
// stored as in the fp32 image (lane q's bytes at 64 k + 4 q .. + 3; a 4-byte load), so k still ascends.
//   rot.  Rows are KP = 64 m bytes apart.  One ds_read_b128 serves lanes 0-3 and 12-15 of one 16-lane group together with lanes 4-11 of
// the next, i.e. pieces {12 .. 15, 0 .. 3} of one row with pieces {4 .. 11} of another, over the 16 pieces (256 bytes) the 64 banks span:
// two arcs of 8 that are disjoint only when the two rows start a multiple of 256 bytes apart.  Rows r and r' start 64 m (r' - r) bytes
// apart, any multiple of a quarter span, and an XOR of the piece index can only undo half a span.  So a row's pieces are ROTATED by
// rot = 4 ((-m row) mod 4), row counted inside the workgroup's slice of the layer: byte 64 m row + 16 rot is a multiple of 256 from the
// slice's start, every row of the layer has the same bank frame, and any two rows are read conflict-free, whether the groups of a wave
// take consecutive rows (G = 1) or rows three apart (the gates of consecutive units).  rot = 0 where m is a multiple of 4.  The pair and
// the single step are not rotated: a ds_read_b64 of two rows 64 m bytes apart is 2-way unless m = 2 (mod 4) -- at most one such read per
// segment.
// The permutation only moves bytes (tg8_pos below is what wrnn_teamg_pack writes by and the dot products read by): each lane still gets
// elements 4 (q + 16 k) .. + 3 at step k, k ascending, and v_cvt_pk_f32_fp8 widens them exactly.
struct TgE4m3 { unsigned char b; };
// two dwords of the conversion: bytes 0, 1 (word 0) and 2, 3 (word 1) of d, each an e4m3fn value, exactly
__device__ __forceinline__ float4 tg8_w4(unsigned d) {
    const auto lo = __builtin_amdgcn_cvt_pk_f32_fp8((int)d, false), hi = __builtin_amdgcn_cvt_pk_f32_fp8((int)d, true);
    return make_float4(lo[0], lo[1], hi[0], hi[1]);
}
// pieces a row's quads are rotated by
__host__ __device__ inline int tg8_rot(int row, int KP) { return ((-(row * (KP >> 6))) & 3) << 2; }
// where element p of row `row` (KAP = elements of segment A, KP = of the row; both multiples of 64) lives in the row of the e4m3 image
__host__ __device__ inline int tg8_pos(int p, int row, int KAP, int KP) {
    const int k = p >> 6, q = (p >> 2) & 15, c = p & 3;
    const int k0 = p < KAP ? 0 : KAP >> 6, k1 = p < KAP ? KAP >> 6 : KP >> 6;
    const int rel = k - k0, n = k1 - k0, nq = n & ~3;
    if (rel < nq) return 64 * (k - (rel & 3)) + 16 * ((q + tg8_rot(row, KP)) & 15) + 4 * (rel & 3) + c;   // a quad
    if ((n & 2) && rel - nq < 2) return 64 * (k - (rel - nq)) + 8 * q + 4 * (rel - nq) + c;              // the pair
    return p;                                                                                             // the single last step
}

// The block-sparse fp32 image (WrnnTeamGSparse): the element is a float, the type only selects the instantiation whose
// dot products walk a row's index list: in that instantiation segment A = list entries [0, nA), B = [nA, nK) of the
// layer, where the dense instantiations have the steps of the padded row.
struct TgSparse { float v; };
// list entries of a layer's segment A, and of the whole row, in the sparse instantiations
__device__ __forceinline__ int tg_sp_na(const WrnnTeamGPlan &plan, const WrnnTeamGSparse &sp, const WrnnTeamGLayer &L) { return sp.nbA[&L - plan.L]; }
__device__ __forceinline__ int tg_sp_nk(const WrnnTeamGPlan &plan, const WrnnTeamGSparse &sp, const WrnnTeamGLayer &L) {
    return sp.nbA[&L - plan.L] + sp.nbB[&L - plan.L];
}

// a granule of either kernel: the e4m3 instantiations are the ones short of scalar registers (team_common.h, st_granule_ws); the
// fp32 and fp16 ones keep st_granule
template <typename WT>
__device__ __forceinline__ void tg_st_granule(unsigned long long *base, unsigned idx, unsigned tag, unsigned payload) {
    if constexpr (sizeof(WT) == 1) st_granule_ws(base, idx, tag, payload);
    else st_granule(base, idx, tag, payload);
}

constexpr int MB_X = 8, MB_ROW = 16, MB_STEPS = 24, MB_UTT = 32, MB_START = 40, MB_SEED = 56, MB_KROW = 72;

}  // namespace
