// Layout of persistent XCD-team GRU recurrences for ANY rnn_dims (the generalisation of train_team.hip, which has rnn_dims = 512
// compiled in): pure host arithmetic behind wrnn_train_teamg_plan.  It answers, before any kernel exists for it, which rnn_dims can keep
// a workgroup's slice of W_hh in LDS for the whole sequence, and what such kernels need.  The split is train_team.hip's:
//   forward   output-split: workgroup g owns units [U g, min(U g + U, H)) with U = ceil(H / 32) -- fewer than U, or none, at the end of
//             the team; a wave multiplies unit quads (v_mfma_f32_4x4x1), so the image holds NUQ = ceil(U / 4) quads of 3 gate rows over
//             K = H padded to HP = 64 NS with zeros; h_{t-1} of the R rows sits next to it in B-operand order
//   backward  K-split: the own 3 U gate rows (padded to K4 quads) times their rows of W_hh give a partial carry for all HP units; the
//             partials of a unit go to its owner through a mailbox [dest 32][row R][source 32][UP], UP = U rounded up to even (16-byte
//             loads take two granules)
#pragma once
#include <cstddef>
#include <cstdint>

#define WRNN_TTG_LDS_LIMIT (160 * 1024)
// bounds a kernel's unrolled register arrays would have; every one of them is implied by the LDS limit
#define WRNN_TTG_MAX_SLOTS 2    // unit quads per wave (forward): 4 waves x 2 x 4 = 32 units per workgroup
#define WRNN_TTG_MAX_M 9        // 16-byte loads per thread of the forward's all-gather (R x HP / 512)
#define WRNN_TTG_MAX_CH 3       // 64-unit output chunks per wave (backward): 4 x 3 x 64 = 768 units
#define WRNN_TTG_MAX_SRC 12     // source workgroups one thread of the backward's reduce-scatter sums

struct WrnnTrainTeamGPlan {
    int32_t H, rows;           // rnn_dims; rows of the instantiation (4 or 8)
    int32_t U;                 // units per workgroup
    int32_t n_owners;          // workgroups that own at least one unit
    int32_t NUQ;               // unit quads per workgroup (forward A operands), ceil(U / 4)
    int32_t NS;                // 64-wide K slabs (forward) = 64-unit output chunks (backward): HP = 64 NS
    int32_t K4;                // quads of own gate rows (backward K)
    int32_t UP;                // U rounded up to even
    int32_t TPI, NSRC;         // backward consumer: threads per (row, unit pair), sources per thread (TPI x NSRC >= 32)
    int64_t img_fwd, img_bwd;  // floats of one workgroup's image
    int64_t lds_fwd, lds_bwd;  // bytes
    int64_t mail_fwd, mail_bwd;   // granules per team (both parities)
    bool structural_ok;        // the compile-time bounds above hold
};

inline WrnnTrainTeamGPlan wrnn_train_teamg_layout(int32_t H, int32_t rows8) {
    WrnnTrainTeamGPlan p{};
    const int R = rows8 > 4 ? 8 : 4;
    p.H = H; p.rows = R;
    p.U = (H + 31) / 32;
    p.n_owners = (H + p.U - 1) / p.U;
    p.NUQ = (p.U + 3) / 4;
    p.NS = (H + 63) / 64;
    p.K4 = (3 * p.U + 3) / 4;
    p.UP = (p.U + 1) & ~1;
    const int nrp = R * (p.UP / 2);            // (row, unit pair) items of a workgroup's reduce-scatter
    p.TPI = 256 / nrp > 32 ? 32 : 256 / nrp;
    if (p.TPI < 1) p.TPI = 1;
    p.NSRC = (32 + p.TPI - 1) / p.TPI;
    const int64_t HP = 64 * (int64_t)p.NS;
    p.img_fwd = (int64_t)p.NUQ * 3 * p.NS * 256;
    p.img_bwd = (int64_t)p.K4 * p.NS * 256;
    // forward: image | h_{t-1} of R rows in B-operand order | misc;  backward: image | G [R][4 K4] | RED [TPI][R][UP] (<= 512 floats) | misc
    p.lds_fwd = 4 * (p.img_fwd + R * HP + 16);
    p.lds_bwd = 4 * (p.img_bwd + (int64_t)R * 4 * p.K4 + 512 + 16);
    p.mail_fwd = 2 * R * HP;
    p.mail_bwd = 2 * (int64_t)32 * R * 32 * p.UP;
    p.structural_ok = (p.NUQ + 3) / 4 <= WRNN_TTG_MAX_SLOTS && (R * HP + 511) / 512 <= WRNN_TTG_MAX_M && (p.NS + 3) / 4 <= WRNN_TTG_MAX_CH &&
                      p.NSRC <= WRNN_TTG_MAX_SRC && nrp <= 256 && p.U * R <= 256;
    return p;
}
