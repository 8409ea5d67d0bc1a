// Internal definitions shared by the HIP translation units of libwavernn_amd.so.
// Product code (gfx950 only).  Reference line citations are relative to
// /root/reference/.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string>
#include <vector>

#include "../../include/wavernn_amd.h"
#include "handle_common.h"

#define WRNN_MAX_UP 4
#define WRNN_PROF_SLOTS 32   // phase-cycle counters per wave (WRNN_TEAM_PROF=1)
#define WRNN_KTAB_MAXD 8

// Dimensions derived from wrnn_config (WaveRNN.__init__, fatchord_version.py:93-129).
struct WrnnDims {
    int H;        // rnn_dims
    int FC;       // fc_dims
    int F;        // feat_dims
    int A;        // aux_dims = res_out_dims / 4   (:109)
    int C;        // compute_dims
    int R;        // res_out_dims
    int NBLK;     // res_blocks
    int P;        // pad
    int KS;       // conv_in kernel = 2*pad+1      (:33)
    int HOP;      // prod(upsample_factors) (== hop_length)
    int NC;       // n_classes                      (:98-101)
    int mode;     // WRNN_MODE_*
    int ND;       // frames of support of the composite upsampling FIR
};
// d from cfg, as WaveRNN.__init__ derives the dims, bounded to what every kernel relies on (HOP = cfg->hop_length: whether the
// upsample factors multiply to it is wrnn_create's check); nullptr, or why cfg is refused (api.hip)
const char *wrnn_dims_from_config(const wrnn_config *cfg, WrnnDims &d);

// Offsets (in floats) into the single packed device allocation.
struct WrnnPacked {
    // prologue, BatchNorm(eval) folded into the adjacent conv (eps 1e-5)
    size_t conv_in_t;   // [F*KS][C]
    size_t conv_in_b;   // [C]
    size_t res_w1_t;    // [NBLK][C(in)][C(out)]
    size_t res_b1;      // [NBLK][C]
    size_t res_w2_t;    // [NBLK][C][C]
    size_t res_b2;      // [NBLK][C]
    size_t conv_out_t;  // [C][R]
    size_t conv_out_b;  // [R]
    size_t ktab;        // [HOP][ND] composite (5,5,11) stretch+FIR taps
    // loop parameters, transposed to [in][out] so that consecutive threads
    // (= consecutive output rows) read consecutive addresses
    size_t I_t, I_b;              // [1+F+A][H], [H]
    size_t r1_wih_t, r1_whh_t;    // [H][3H], [H][3H]
    size_t r1_bih, r1_bhh;        // [3H]
    size_t r2_wih_t, r2_whh_t;    // [H+A][3H], [H][3H]
    size_t r2_bih, r2_bhh;
    size_t fc1_t, fc1_b;          // [H+A][FC], [FC]
    size_t fc2_t, fc2_b;          // [FC+A][FC], [FC]
    size_t fc3_t, fc3_b;          // [FC][NC], [NC]
    size_t total;
};

// One loop row = one utterance (unbatched) or one fold (fold_with_overlap :293-340).
struct WrnnRow {
    int32_t utt;      // index into the mel batch
    int32_t steps;    // loop steps of this row: the call's `steps`, or frames[utt] * hop in a ragged batch (opts.frames_dev)
    int64_t start;    // first upsampled position of this row
};
// Philox key of one loop row when the call carries per-utterance seeds (opts.utt_seeds_dev): every draw of the row is keyed
// (seed, step, row, class) with the row's utterance seed and the row's index INSIDE its utterance (fold i of a folded call,
// 0 of an unbatched one) -- what a call on that utterance alone with that seed draws.  Indexed by the row, not by a schedule slot.
struct WrnnRowKey {
    uint64_t seed;
    uint32_t row;
    uint32_t pad;
};
// Device error word codes (first come, first kept): 3 = a team kernel's workgroups did not all become resident (WRNN_ERR_BUSY),
// everything else = a bounded exchange spin gave up (WRNN_ERR_TIMEOUT)
#define WRNN_DEVERR_BUSY 3u
// rows_folded_kernel: the fold count computed on the device differs from the call's rows_total (WRNN_ERR_INVALID)
#define WRNN_DEVERR_ROWS 4u

struct WrnnTrainState;   // train.hip: workspace + captured step graphs of wrnn_train_step
void wrnn_train_state_free(WrnnTrainState *st);

struct wrnn_handle {
    wrnn_config cfg;
    WrnnDims d;
    WrnnPacked off;
    float *wdev = nullptr;        // packed weights on device
    bool loaded = false;
    int64_t loop_weight_bytes = 0;
    // scratch (grown on demand)
    float *aux_frames = nullptr;  // (B, T, R)
    size_t aux_cap = 0;
    WrnnRow *rows_dev = nullptr;
    int32_t *order_dev = nullptr; // [rows] rows by length, longest first, in a ragged batch; identity otherwise (BATCH kernel)
    int32_t *sched_dev = nullptr; // [rows rounded up to n_teams] per-team row lists of the TEAM2 kernel (see WrnnTeamArgs)
    WrnnRowKey *keys_dev = nullptr;   // [rows] Philox keys of a call with opts.utt_seeds_dev (written next to the row table)
    size_t rows_cap = 0;
    // wrnn_generate_folded: first row of every utterance, [B + 1], written by rows_folded_kernel and read by wrnn_epilogue_folded;
    // fold_B > 0 once such a call ran: its B, target, overlap, rows_total
    int32_t *fold0_dev = nullptr;
    size_t fold0_cap = 0;
    int32_t fold_B = 0, fold_target = 0, fold_overlap = 0, fold_rows = 0;
    unsigned *err_dev = nullptr;  // device error word (bounded spins)
    // team kernel state
    float *team_w = nullptr, *team_fc3 = nullptr, *wI0 = nullptr, *u1 = nullptr;
    float *batch_w = nullptr, *batch_fc3 = nullptr, *batch_wn = nullptr;   // batch kernel images of the same weights
    bool team_dims = false;       // the constructor dims are the reference hparams the team kernels are built for
    bool team_ok = false;         // the 32-workgroup team kernels can be co-resident on this device (checked at create)
    std::string team_why;         // why not, when team_ok is false
    void *teamg_img = nullptr;    // TEAMG weight image [32 WGs][WrnnTeamGPlan::img_elems_wg] of fp32, fp16 or e4m3, packed on the device by the first TEAMG call
                                  // after a load or a change of teamg_fmt
    bool teamg_img_ok = false;
    int32_t teamg_fmt = 0;        // WRNN_WEIGHTS_F32 / _F16 / _E4M3 (wrnn_teamg_set_weight_format): the element type of the image
    float teamg_scale[6] = {1.0f, 1.0f, 1.0f, 1.0f, 1.0f, 1.0f};   // per-layer scales of the image last packed (wrnn_teamg_weight_scales)
    bool teamg_sparse = false;    // wrnn_teamg_set_sparse: both kernels run the block-sparse fp32 image
    bool teamg_sp_ok = false;     // the figures below are those of a packed sparse image (wrnn_teamg_sparse_info)
    int32_t teamg_nb_a[6] = {}, teamg_nb_b[6] = {};       // blocks per image row and segment: the layer's longest list
    int64_t teamg_sp_kept[6] = {}, teamg_sp_dense[6] = {};   // non-zero blocks, and blocks of the dense rows, per layer
    int64_t teamg_sp_budget = -1; // the plan in force: budget and rows per team of the call that last ran sparse
    int32_t teamg_sp_rows = 1;
    void *teamg_sp_flags = nullptr;   // census scratch: one byte per block of the dense rows, then the per-layer counters
    int64_t teamg_budget = -1;    // wrnn_debug_teamg_lds_budget: LDS bytes for resident weights, < 0 = the default
    int last_batch_rows = 1;      // rows per team batch of the last generate call's loop kernel (wrnn_last_batch_rows)
    bool force_no_teams = false;  // wrnn_debug_force_no_teams: AUTO behaves as if residency had failed (tests of the slow-path warning)
    bool cs_ok = false;           // ... and loop_batch_cs_kernel in particular (AUTO falls back to WRNN_KERNEL_BATCH without it)
    float *tab = nullptr;         // CM|CA|VM|VA|C2|C3|C4 for the current batch
    size_t tab_cap = 0;
    float *cond = nullptr;        // conditioning stream of the current segment (TEAM2)
    size_t cond_cap = 0;
    double *epi_tab = nullptr;    // epilogue tables [dec NC | fade_in | fade_out | tail] for epi_overlap
    long epi_overlap = -1;
    float *team_state = nullptr;  // recurrent state of every row between segment launches (TEAM2)
    size_t team_state_cap = 0;
    unsigned long long *mail = nullptr;
    unsigned *ctl = nullptr;
    int n_teams = 8;              // XCDs (32-CU teams) of this device
    unsigned long long *prof = nullptr;   // phase-cycle counters, allocated by wrnn_phase_profile(h, 1)
    bool prof_on = false;
    double prof_div = 0;
    double *loss_partial = nullptr;   // per-block partial sums of wrnn_loss
    size_t loss_cap = 0;
    WrnnTrainState *train = nullptr;
    bool train_force_steps = false;   // wrnn_train_force_step_kernels
    int32_t train_last_kernel = -1, train_last_rows = 0;   // what the recurrences of the last training call ran (wrnn_train_last_recurrence); -1 = none yet
    int32_t train_precision = 0;      // WRNN_TRAIN_F32 / WRNN_TRAIN_BF16 (wrnn_train_set_precision): which kernel the GEMMs of training run on
    int32_t train_n_f32 = -1, train_n_bf16 = -1;   // GEMM launches of the last training call by kernel (wrnn_train_last_gemms); -1 = none yet
    hipEvent_t ev[3] = {nullptr, nullptr, nullptr};
    bool timing_valid = false;
    wrnn_timing last{};
    std::string err;
};

// Arguments of the per-sample loop kernels.
struct WrnnLoopArgs {
    const float *w;           // packed weights
    WrnnPacked off;
    WrnnDims d;
    const float *mels;        // (B, F, mel_T)
    int32_t mel_T, mel_off;   // frames per mel row, index of frame 0 (see wrnn_launch_resnet)
    const float *aux_frames;  // (B, T, R)
    const WrnnRow *rows;
    int32_t n_rows;
    int32_t T;                // mel frames per utterance
    int64_t total_len;        // T * HOP
    int64_t steps;            // loop length per row (the longest row's in a ragged batch; row r runs rows[r].steps)
    int32_t noise_mode;
    uint64_t seed;
    const WrnnRowKey *keys;   // [n_rows] per-row Philox keys replacing (seed, row), or null (no opts.utt_seeds_dev; streams)
    const float *noise1;      // RAW (L, rows, NC) | MOL (L, rows, 10)
    const float *noise2;      // MOL (L, rows)
    const float *x_forced;    // (L, rows) or null
    const float *x_init;      // (rows) value fed to step 0 instead of 0, or null (teacher-forced forward())
    float *logits_out;        // (L, rows, NC) or null
    int32_t *labels_out;      // (rows, L) or null
    float *samples_out;       // (rows, L)
    unsigned *err;
    // streams (stream.hip): row r runs steps [seg0, seg0 + rows[r].steps) (Philox keyed by the absolute step, outputs at
    // [row * steps + t]) and, when state != null, starts from / leaves its recurrent state in
    // state[row * wrnn_simple_state_floats]: [h1 H | h2 H | x 1 | pad].  Offline calls: 0, null.
    int64_t seg0;
    float *state;
    // folds of several utterances (wrnn_generate_folded), B int32 or null: utterance u ends at frames[u] * HOP instead of total_len
    const int32_t *frames;
};
__host__ __device__ inline int wrnn_simple_state_floats(const WrnnDims &d) { return 2 * d.H + 4; }

// Team kernel (loop_team2.hip): mailbox size per team in 8-byte granules:
// x3, fc1, fc2, race winners (2 x 512 each), gh1 (2 x 1536)
#define WRNN_TEAM_MAIL_GRANULES (8 * 512 + 2 * 1536)
#define WRNN_TEAM_NWREG 352
#define WRNN_TEAM_STATE_FLOATS (8 * 512 + 64)
#define WRNN_TEAM_THREADS 256

struct WrnnTeamArgs {
    const float *w;           // packed weights (biases, ktab)
    WrnnPacked off;
    WrnnDims d;
    const float *team_w;      // [32 WGs][352][256 threads] register-resident weights
    const float *team_fc3;    // [32 WGs][16384] LDS image of the fc3 slices
    const float *wI0;         // [H]   W_I[:,0]
    const float *u1;          // [3H]  W_ih1 . W_I[:,0]
    // per-utterance conditioning pushed through the linear layers it feeds:
    //   CM (T+2P, H) = W_I[:,1:1+F] . melpad[f]     CA (T+1, H) = W_I[:,1+F:] . a1[i] + b_I (entry T: zeros in)
    //   VM (T+2P,3H) = W_ih1 . CM[f]                VA (T+1,3H) = W_ih1 . CA[i] + b_ih1
    // packed per frame and hidden unit, see pack_records_kernel (prologue.hip)
    const float *tabREC;      // (B, T+1, H, 28)
    const float *tabCOND;     // (rows, seg_len, H, 4) phase-A conditioning stream of steps [seg0, seg0+seg_len) (TEAM2) or null
    const float *tabC2;       // (B, T+1, 3H)   W_ih2[:,H:] . a2[i] + b_ih2
    const float *tabC3;       // (B, T+1, FC)   fc1.W[:,H:] . a3[i] + b1
    const float *tabC4;       // (B, T+1, FC)   fc2.W[:,FC:] . a4[i] + b2
    const WrnnRow *rows;
    const int32_t *sched;     // [n_slots] team t runs rows sched[t], sched[t + n_teams], ... (-1 = none): identity for a uniform batch,
    int32_t n_slots;          // longest-first rows dealt in snake order (0..n-1, n-1..0, ...) for a ragged one; n_slots = n_rows rounded
    int32_t ragged;           // up to a multiple of n_teams.  ragged != 0: use sched and the rows' own steps (opts.frames_dev)
    int32_t n_rows;
    int32_t n_teams;          // teams = XCDs in use; the launch grid is n_teams * 32 workgroups
    int32_t T;
    int64_t total_len;
    int64_t steps;
    // TEAM2 runs a row in segments (one launch each) so that the conditioning stream of a segment is still cache
    // resident when it is read; the recurrent state crosses launches through `state`:
    // per row [h1 H | h2 H | gh1 3H | gh2 3H | x 1 | pad] floats (WRNN_TEAM_STATE_FLOATS)
    int64_t seg0, seg_len;
    float *state;
    int32_t noise_mode;
    uint64_t seed;
    const WrnnRowKey *keys;   // as in WrnnLoopArgs
    const float *noise1;
    const float *noise2;
    const float *x_forced;
    const float *x_init;
    float *logits_out;
    int32_t *labels_out;
    float *samples_out;
    unsigned long long *mail;  // [n_teams][WRNN_TEAM_MAIL_GRANULES]
    unsigned *ctl;             // [TEAM_CTL_WORDS] team formation (team_common.h)
    unsigned *err;
    unsigned long long *prof;  // [8][WRNN_PROF_SLOTS] phase cycle counters (developer instrumentation) or null
};

// Batch kernel (loop_batch.hip): R = 4 * nq rows per team in lock-step on the matrix cores.
// mailbox per team: 5 gathered vectors (x2, h1', x3, fc1, fc2) x 2 parities x R*512 granules + race 2 x R*128
#define WRNN_BATCH_MAIL_GRANULES (10 * 8 * 512 + 2 * 8 * 128)
#define WRNN_BATCH_MAX_ROWS 8
#define WRNN_MAIL_GRANULES_MAX (WRNN_BATCH_MAIL_GRANULES > WRNN_TEAM_MAIL_GRANULES ? WRNN_BATCH_MAIL_GRANULES : WRNN_TEAM_MAIL_GRANULES)
#define WRNN_MAIL_BYTES ((size_t)8 * WRNN_MAIL_GRANULES_MAX * sizeof(unsigned long long))   // wrnn_handle::mail, 8 teams

struct WrnnBatchArgs {
    const float *w;           // packed weights (biases, ktab)
    WrnnPacked off;
    WrnnDims d;
    const float *batch_w;     // [32 WGs][4 waves][320][64 lanes] MFMA A-operand images of the register-resident weights
    const float *batch_fc3;   // [32 WGs][4 waves][2 sets][8][64 lanes][4] A-operand image of the fc3 slice (LDS)
    const float *batch_wn;    // [32 WGs][4 waves][8][64 lanes][4] A-operand image of gate n of W_hh2 (LDS)
    const float *wI0;         // [H]   W_I[:,0]
    const float *u1;          // [3H]  W_ih1 . W_I[:,0]
    const float *tabREC32;    // (B, T+1, H, 32): the 24 phase-A record floats (pack_records_kernel) | c2 r,z,n | c3 | c4 | pad
    const WrnnRow *rows;
    const int32_t *order;     // schedule slot -> row (longest first in a ragged batch, identity otherwise)
    int32_t snake;            // != 0: batches are dealt to the teams in snake order (ragged batch), else round-robin
    int32_t n_rows;
    int32_t n_teams;
    int32_t nq;               // row quads per team: 1 (4 rows) or 2 (8 rows)
    int32_t rpb;              // rows actually placed in one batch (<= 4 * nq): batch b = slots [b * rpb, (b + 1) * rpb); it runs
                              // for the steps of its first (longest) row
    int32_t T;
    int64_t total_len;
    int64_t steps;
    int32_t noise_mode;
    uint64_t seed;
    const WrnnRowKey *keys;   // as in WrnnLoopArgs; indexed by the row a.order[] maps a slot to
    const float *noise1;
    const float *noise2;
    const float *x_forced;
    const float *x_init;
    float *logits_out;
    int32_t *labels_out;
    float *samples_out;
    unsigned long long *mail;  // [n_teams][WRNN_BATCH_MAIL_GRANULES]
    unsigned *ctl;
    unsigned *err;
    unsigned long long *prof;
};

// Team kernel for any dims (loop_teamg.hip).  Every layer is a set of `N` units of `G` rows (3 gate rows of a hidden unit, or one
// row); a row is [segment A: KA weights, padded to KAP | segment B: KB weights, padded] = KP elements, both paddings multiples of 64
// (16 lanes x 4 elements).  Workgroup g owns units [g * U, min(N, (g + 1) * U)); its slice of the image is U * G rows of KP elements at
// img_off, of which the first nres units are copied to LDS (at lds_off elements behind the activation vectors) at the start of a launch.
// An element is a weight of plan.esz bytes: 4 (fp32), 2 (IEEE binary16) or 1 (OCP e4m3fn); offsets and counts are in elements in every format.
struct WrnnTeamGLayer {
    int32_t N, G, KA, KB, KAP, KP, U, nres;
    int64_t img_off;    // elements, inside a workgroup's image
    int32_t lds_off;    // elements, inside the resident-weight area
    float scale;        // WRNN_WEIGHTS_E4M3: the layer's power-of-two scale, applied to a row's segment sums; 1 in the other formats
};
struct WrnnTeamGPlan {
    WrnnTeamGLayer L[WRNN_TEAMG_LAYERS];
    int64_t img_elems_wg;      // image elements per workgroup (every workgroup the same)
    int32_t act_floats;        // LDS floats of the activation vectors (TgLay, loop_teamg.hip): fp32 in either format
    int32_t res_elems;         // LDS elements of the resident weights
    int32_t mail_granules;     // per team
    int32_t esz;               // bytes of a weight element: 4, 2 or 1
};
// The block-sparse fp32 image: behind the plan in the kernels' arguments, so that nothing the dense instantiations read
// moves.  A block = 64 consecutive elements of a padded row (one step of a 16-lane group's dot product).  An image row is
// [nbA + nbB 16-bit block indices, padded to 16 bytes][nbA + nbB blocks of 64 floats]: segment A's kept blocks in ascending order, padded
// to nbA with zero blocks of index 0, then segment B's (indices count from the row's start, so >= KAP / 64), padded to nbB with zero blocks
// of index KAP / 64.  In a sparse plan L.KP is the FLOATS OF AN IMAGE ROW (wrnn_teamg_sparse_row_elems), everything else is the dense plan's.
struct WrnnTeamGSparse {
    int32_t on, pad_;
    int32_t nbA[WRNN_TEAMG_LAYERS], nbB[WRNN_TEAMG_LAYERS];
};
inline int wrnn_teamg_sparse_idx_elems(int nb) { return (nb + 7) / 8 * 4; }                           // floats of the index list
inline int wrnn_teamg_sparse_row_elems(int nb) { return wrnn_teamg_sparse_idx_elems(nb) + 64 * nb; }  // floats of an image row
inline size_t wrnn_teamg_lds_bytes(const WrnnTeamGPlan &p) { return (size_t)p.act_floats * 4 + (size_t)p.res_elems * p.esz; }
#define WRNN_TEAMG_THREADS 512
struct WrnnTeamGArgs {
    WrnnLoopArgs a;            // the call's loop arguments (weights, conditioning inputs, rows, sampling)
    WrnnTeamGPlan plan;
    const void *img;           // [32][plan.img_elems_wg] of plan.esz bytes
    const int32_t *sched;      // as WrnnTeamArgs
    int32_t n_slots, ragged, n_teams, pad_;
    unsigned long long *mail;  // [n_teams][plan.mail_granules]
    unsigned *ctl;
    WrnnTeamGSparse sp;        // last: the dense instantiations never read it
};
// pure host: ownership and placement for dims d with `budget` LDS bytes for resident weights (< 0 or too large: 160 KiB minus the
// activation vectors); nullptr, or why the kernel cannot serve these dims.  rows_per_team = 1: loop_teamg.hip; 2, 4, 8: the lock-step
// rows of loop_teamg_batch.hip, whose activation vectors (TgbLay, teamg_layout.h) and mailbox regions are counted that many times --
// ownership and the weight image do not depend on it.  esz = bytes of a weight element (4: fp32, 2: fp16, 1: e4m3): only how many units fit;
// every layer's scale is 1 (the caller sets the scales of the packed e4m3 image).
// nb_a / nb_b (both or neither; esz = 4): the plan of the block-sparse image with that many blocks per row and segment of each layer;
// a count above the dense row's is refused.
const char *wrnn_teamg_make_plan(const WrnnDims &d, int64_t budget, WrnnTeamGPlan &p, int rows_per_team = 1, int esz = 4, const int32_t *nb_a = nullptr,
                                 const int32_t *nb_b = nullptr);
// bytes of the image allocation: the 32 slices and, behind them, one word per layer: the flag of the fp16 range check, or the bits of
// the layer's largest |w| of the e4m3 pack
inline size_t wrnn_teamg_img_bytes(const WrnnTeamGPlan &p) { return (size_t)32 * p.img_elems_wg * p.esz + WRNN_TEAMG_LAYERS * sizeof(int32_t); }
// Packs the image in the plan's element type.  fp16: round to nearest even on the device, then ONE wait for the range check;
// *bad_layer = the first layer holding a weight that does not round to a finite fp16, or -1.  fp32: no wait, *bad_layer = -1.
// e4m3: an abs-max pass per layer, ONE wait for the six maxima, the scales on the host (wrnn_teamg_e4m3_scale), then the pack proper;
// *bad_layer = the first layer holding a weight that is not finite, or -1.  scales[l] = the layer's scale (1 in the other formats).
hipError_t wrnn_teamg_pack(const wrnn_handle *h, const WrnnTeamGPlan &p, void *img, hipStream_t s, int *bad_layer, float scales[WRNN_TEAMG_LAYERS]);
// The scale of an e4m3 layer whose largest magnitude is amax (finite): 2^e with e the smallest integer such that amax / 2^e <= 448,
// clamped to e >= -126 so that the scale is a normal float (amax < 2^128 gives e <= 120, so 2^-e is normal too); 1 for amax = 0.
float wrnn_teamg_e4m3_scale(float amax);
extern const char *const wrnn_teamg_layer_names[WRNN_TEAMG_LAYERS];
// wrnn_teamg_plan_fmt's figures; with nb_a / nb_b those of the block-sparse plan (wrnn_teamg_sparse_plan)
int wrnn_teamg_plan_info_impl(const wrnn_config *cfg, int rows_per_team, int fmt, int64_t lds_budget_bytes, wrnn_teamg_plan_info *out, const int32_t *nb_a,
                              const int32_t *nb_b);
hipError_t wrnn_teamg_occupancy(const WrnnTeamGPlan &p, int *blocks_per_cu, bool sparse = false);
hipError_t wrnn_launch_loop_teamg(const WrnnTeamGArgs &a, hipStream_t s);
// The sparse pack.  Census: per image row and segment, which blocks of the dense row hold a weight that does not compare equal to zero
// (a NaN does not), into `flags` (wrnn_teamg_sparse_flag_bytes) -- one wait, then nb_a / nb_b = each layer's longest list, kept / dense =
// its non-zero blocks and the blocks of its dense rows.  Compaction: the image of a plan made from those counts, no wait.
size_t wrnn_teamg_sparse_flag_bytes(const WrnnDims &d);
hipError_t wrnn_teamg_sparse_census(const wrnn_handle *h, void *flags, hipStream_t s, int32_t nb_a[WRNN_TEAMG_LAYERS], int32_t nb_b[WRNN_TEAMG_LAYERS],
                                    int64_t kept[WRNN_TEAMG_LAYERS], int64_t dense[WRNN_TEAMG_LAYERS]);
hipError_t wrnn_teamg_sparse_pack(const wrnn_handle *h, const WrnnTeamGPlan &p, const int32_t *nb_a, const int32_t *nb_b, const void *flags, void *img, hipStream_t s);

// The same team kernel with RB = 2, 4 or 8 rows per team in lock-step (loop_teamg_batch.hip).  plan = wrnn_teamg_make_plan(.., RB).
#define WRNN_TEAMG_BATCH_MAX_ROWS 8
struct WrnnTeamGBatchArgs {
    WrnnLoopArgs a;
    WrnnTeamGPlan plan;
    const void *img;           // the image of WRNN_KERNEL_TEAMG, shared
    const int32_t *order;      // schedule slot -> row, as WrnnBatchArgs
    int32_t rpb;               // rows placed in one batch (<= RB): batch b = slots [b * rpb, (b + 1) * rpb), it runs for the steps of its longest row
    int32_t snake;             // != 0: batches are dealt to the teams in snake order (ragged batch), else round-robin
    int32_t n_teams, pad_;
    unsigned long long *mail;  // [n_teams][plan.mail_granules], row r of a team's batch at r * (plan.mail_granules / RB)
    unsigned *ctl;
    WrnnTeamGSparse sp;        // last, as in WrnnTeamGArgs
};
inline int wrnn_teamg_batch_inst(int rpb) { return rpb <= 2 ? 2 : (rpb <= 4 ? 4 : 8); }   // the instantiation that runs rpb rows
hipError_t wrnn_teamg_batch_occupancy(const WrnnTeamGPlan &p, int rb, int *blocks_per_cu, bool sparse = false);
hipError_t wrnn_launch_loop_teamg_batch(const WrnnTeamGBatchArgs &a, int rb, hipStream_t s);

// Persistent team kernels of the two GRU recurrences of wrnn_train_step (train_team.hip)
struct WrnnGruTeamArgs {
    const float *img;          // weight image of this recurrence for the kernel at hand (wrnn_gru_team_pack)
    const float *bhh;          // [3H] (forward)
    const float *GI;           // (B, L, 3H) forward: input part of the gates
    float *Hs, *HP, *Rs, *Zs, *Ns, *GHN;   // (B, L, H) saved by the forward, read by the backward
    const float *dHext;        // (B, L, H) backward: gradient flowing into h_t from the layers above
    float *dGI, *dGH;          // (B, L, 3H) backward outputs
    int32_t B;
    int64_t L;
    int32_t n_teams, rpb;      // rows per team batch (<= 4 * nq)
    unsigned long long *mail;  // [n_teams][wrnn_gru_team_mail_granules(nq, bwd)]
    unsigned *ctl, *err;
};
size_t wrnn_gru_team_mail_granules(int nq, bool bwd);
hipError_t wrnn_gru_team_pack(const float *Whh, float *img, bool bwd, hipStream_t s);
hipError_t wrnn_gru_team_launch(const WrnnGruTeamArgs &a, int nq, bool bwd, hipStream_t s);
hipError_t wrnn_gru_team_occupancy(int nq, bool bwd, int *blocks_per_cu);

// The batched GEMM of wrnn_train_step with operands rounded to bfloat16 on their way into LDS (train_gemm_bf16.hip): sgemm_kernel's
// arguments (train.hip), NT / NN / TN; hipErrorNotSupported for TT.  A split-K slice is a multiple of WRNN_GEMM_BF16_KTILE.
#define WRNN_GEMM_BF16_KTILE 32
hipError_t wrnn_gemm_bf16_launch(hipStream_t s, bool ta, bool tb, const float *A, long lda, const float *B, long ldb, float *C, long ldc, int M,
                                 int N, int K, int beta, const float *bias, int relu, int slices, int kper, long cslice);

// kernels / launchers (defined in the .hip files)
// mel_T = frames per row of `mels`, mel_off = index of frame 0 in it: (T, 0) for generate()'s unpadded mels (zero
// padding applied on the fly, :183), (T + 2 pad, pad) for mels already padded like WaveRNN.forward receives them (:143)
hipError_t wrnn_launch_resnet(const wrnn_handle *h, const float *mels, int B, int T, int mel_T, int mel_off, float *aux_frames,
                              hipStream_t s);
hipError_t wrnn_launch_materialize(const wrnn_handle *h, const float *mels, const float *aux_frames, int B,
                                   int T, int mel_T, int mel_off, float *up, float *aux_up, hipStream_t s);
hipError_t wrnn_launch_loop_simple(const WrnnLoopArgs &a, hipStream_t s);
size_t wrnn_simple_lds_bytes(const WrnnDims &d);
hipError_t wrnn_launch_loop_batch(const WrnnBatchArgs &a, hipStream_t s);
hipError_t wrnn_batch_occupancy(int mode, int nq, bool prof, int *blocks_per_cu, size_t *lds_bytes);
// loop_batch_cs.hip: the same step with critical / shadow wave roles (two waves per SIMD); nq as built (wrnn_batch_cs_max_nq)
hipError_t wrnn_launch_loop_batch_cs(const WrnnBatchArgs &a, hipStream_t s);
hipError_t wrnn_batch_cs_occupancy(int mode, int nq, bool prof, int *blocks_per_cu, size_t *lds_bytes);
int wrnn_batch_cs_max_nq(int mode);
hipError_t wrnn_team2_occupancy(int mode, bool prof, int *blocks_per_cu, size_t *lds_bytes);
// Per-device ordering of team-kernel launches inside this process (api.hip): enter() makes `s` wait for the previous team
// kernel launched on `device` by any handle / stream and takes the device's launch lock, leave() records the new tail and
// releases the lock.  Nothing blocks on the GPU's progress; only the launching threads are serialised.
hipError_t wrnn_team_gate_enter(int device, hipStream_t s);
hipError_t wrnn_team_gate_leave(int device, hipStream_t s);
// why the XCD-team kernels cannot run for this handle, or nullptr (api.hip; what AUTO and wrnn_team_info decide on)
const char *wrnn_loop_team_obstacle(const wrnn_handle *h);
hipError_t wrnn_launch_loss(int mode, const float *y_hat, const void *y, int NC, long n_rows, double *partial, int *bad, float *out,
                            hipStream_t s);
// rows[r] = {utt, steps, start}; order[] = rows sorted by steps, longest first (stable), when frames != null, else identity;
// sched[] (n_rows rounded up to n_teams entries) = the same order dealt to n_teams teams in snake order, -1 where empty;
// seeds (n_rows uint64, device; unbatched calls) != null: keys[r] = {seeds[r], 0}
hipError_t wrnn_launch_rows(WrnnRow *rows, int32_t *order, int32_t *sched, int n_rows, int n_teams, int batched, long stride, long steps,
                            const int32_t *frames, int T, int hop, WrnnRowKey *keys, const uint64_t *seeds, hipStream_t s);
// frames (B int32, device) or null: records fi >= frames[b] of utterance b are written as copies of record T (zero conditioning)
hipError_t wrnn_launch_pack_records32(const float *CM, const float *CA, const float *VM, const float *VA, const float *C2,
                                      const float *C3, const float *C4, float *rec, int B, int T, int P, const int32_t *frames,
                                      hipStream_t s);
// folds of several utterances: rows[fold0[b] + i] = {b, steps, i * stride}, identity order / sched, fold0[B + 1] (clamped to
// rows_total); a fold count that differs from rows_total sets *err = WRNN_DEVERR_ROWS and touches no row outside [0, rows_total);
// seeds (B uint64, device) != null: keys[fold0[b] + i] = {seeds[b], i}
hipError_t wrnn_launch_rows_folded(WrnnRow *rows, int32_t *order, int32_t *sched, int32_t *fold0, unsigned *err, const int32_t *frames,
                                   int B, int rows_total, int n_teams, long target, long overlap, int hop, int T, WrnnRowKey *keys,
                                   const uint64_t *seeds, hipStream_t s);
// TEAM2 reads C2 / C3 / C4 (B, T + 1, .) by frame: entries frames[b] <= f < T of utterance b become copies of entry T
hipError_t wrnn_launch_mask_frame_tables(float *C2, float *C3, float *C4, const int32_t *frames, int B, int T, hipStream_t s);
hipError_t wrnn_launch_loop_team2(const WrnnTeamArgs &a, hipStream_t s);
hipError_t wrnn_launch_cond_stream(const float *rec, const float *ktab, const WrnnRow *rows, float *cond, int n_rows, int T,
                                   int HOP, long total_len, long seg0, long seg_len, hipStream_t s);
hipError_t wrnn_launch_pack_records(const float *CM, const float *CA, const float *VM, const float *VA, float *rec, int B,
                                    int T, int P, const int32_t *frames, hipStream_t s);
// out[b][f][n] = bias[n] + sum_k in(b,f,k) * Wt[k*ldw + n]; mode 0: row-major src (rows >= valid read as 0),
// mode 1: src = mels (B,F,T) read as zero-padded frames melpad[f] = mel[:, f - P]
hipError_t wrnn_launch_frame_linear(int mode, const float *src, size_t src_bstride, int ld, int valid, const float *Wt,
                                    int ldw, const float *bias, float *out, size_t out_bstride, int frames, int K,
                                    int N, int B, int T, int P, hipStream_t s);

// ---- host launch path of the team kernels, shared by the offline calls (api.hip), the streams (stream.hip) and training (train.hip) ----

// The main handle's own formatter (launch.hip): its texts are cut at 511 characters, where handle_common.h's template cuts at 399.  A call
// of wrnn_failf or WRNN_TRY on a wrnn_handle picks this one (a non-template is preferred to the template).
int wrnn_failf(wrnn_handle *h, int code, const char *fmt, ...) __attribute__((format(printf, 3, 4)));

// Grow-only device scratch of `need` elements: kept while it is large enough, so a buffer stays at its high-water mark.  A failed
// allocation leaves p null and cap 0.
template <typename T>
int wrnn_grow(wrnn_handle *h, T *&p, size_t &cap, size_t need) {
    if (need <= cap) return WRNN_OK;
    if (p) (void)hipFree(p);
    p = nullptr; cap = 0;
    WRNN_TRY(h, hipMalloc(&p, need * sizeof(T)));
    cap = need;
    return WRNN_OK;
}

// One team-kernel launch inside the device's gate.  Team kernels of one device run one after the other, whatever handle / stream
// launches them (wavernn_amd.h); the mailbox and arrival-counter resets belong inside the gate: the previous team kernel on these
// buffers may still be reading them.  The gate is left on every path; the first error wins.
template <typename Launch>
hipError_t wrnn_gated_launch(int device, hipStream_t s, void *mail, size_t mail_bytes, void *ctl, size_t ctl_bytes, Launch launch) {
    hipError_t e = wrnn_team_gate_enter(device, s);
    if (e != hipSuccess) return e;
    e = hipMemsetAsync(mail, 0, mail_bytes, s);
    if (e == hipSuccess) e = hipMemsetAsync(ctl, 0, ctl_bytes, s);
    if (e == hipSuccess) e = launch();
    const hipError_t ge = wrnn_team_gate_leave(device, s);
    return e != hipSuccess ? e : ge;
}

// the ten sampling fields WrnnBatchArgs and WrnnTeamArgs share with the WrnnLoopArgs of the same call
template <typename Dst>
void wrnn_copy_sampling(Dst &dst, const WrnnLoopArgs &a) {
    dst.noise_mode = a.noise_mode; dst.seed = a.seed; dst.keys = a.keys; dst.noise1 = a.noise1; dst.noise2 = a.noise2;
    dst.x_forced = a.x_forced; dst.x_init = a.x_init; dst.logits_out = a.logits_out; dst.labels_out = a.labels_out; dst.samples_out = a.samples_out;
}

// Per-frame tables of the team kernels (see WrnnTeamArgs): the conditioning pushed through the linear layers it feeds, once per call
// or stream window.  CM | CA | VM | VA | C2 | C3 | C4 | REC in one allocation; REC (B, T+1, H, rec_floats) is left to the caller's
// wrnn_launch_pack_records (28 floats, TEAM2) / wrnn_launch_pack_records32 (32, the batch kernels).
struct WrnnFrameTables {
    float *CM, *CA, *VM, *VA, *C2, *C3, *C4, *REC;
};
// `mels` (B, F, mel_T) with frame 0 at index P - mel_shift (wrnn_launch_resnet's mel_off), aux (B, T, R); buf / cap grow on demand
int wrnn_build_frame_tables(wrnn_handle *h, float *&buf, size_t &cap, const float *mels, int mel_T, int mel_shift, const float *aux, int B,
                            int T, int rec_floats, WrnnFrameTables &t, hipStream_t s);
// TEAM2 runs steps [t_begin, t_end) of every row in segments of `seg` steps, one conditioning chunk + one gated launch each (the
// reasons are at wrnn_team2_segment_len, launch.hip); seg_override: wrnn_sample_opts.team2_segment, 0 = the library's choice
int64_t wrnn_team2_segment_len(int rows, int H, int64_t steps, int seg_override);
// ta complete but for seg0 / seg_len / tabCOND; cond holds n_rows * seg * H * 4 floats; *launches (may be null) = segments run
int wrnn_run_team2_segments(wrnn_handle *h, WrnnTeamArgs &ta, float *cond, int64_t t_begin, int64_t t_end, int64_t seg, int *launches,
                            hipStream_t s);
