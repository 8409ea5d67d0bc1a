// LDS carve-up of the two team kernels for any dims: TgLay (loop_teamg.hip, one row per team) and TgbLay (loop_teamg_batch.hip, RB rows
// per team in lock-step).  wrnn_teamg_make_plan sizes the resident weights by what these leave of 160 KiB.
#pragma once
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
constexpr int MB_X = 8, MB_ROW = 16, MB_STEPS = 24, MB_UTT = 32, MB_START = 40, MB_SEED = 56, MB_KROW = 72;

}  // namespace
