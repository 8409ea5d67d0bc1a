/*
 * wavernn_amd.h -- C-ABI of the MI355X-native WaveRNN vocoder (mel -> wav).
 *
 * The reference (lturing/tacotronv2_wavernn_chinese) has NO native/FFI layer:
 * its boundary for this path is the Python class
 *   wavernn/models/fatchord_version.py:92-129  WaveRNN.__init__
 *   wavernn/models/fatchord_version.py:169-264 WaveRNN.generate
 *   wavernn/models/fatchord_version.py:414-417 WaveRNN.load  (flat state_dict)
 * and the script wavernn_gen.py:13-43 (gen_from_file).  This header is the
 * C-ABI a maintainer would bind from that class (ctypes stub in
 * INTEGRATION.md); every entry point cites the reference lines it replaces.
 *
 * Conventions: plain pointers and sizes, no torch/C++ types; integer status
 * returns (0 = ok, <0 = error, message via wrnn_last_error); no exceptions
 * cross the ABI; caller allocates outputs; the library owns packed weights and
 * scratch; one handle per device; a handle is not thread-safe, distinct
 * handles are independent.  All `*_dev` pointers are device (HBM) pointers on
 * the handle's device; everything is enqueued on the caller's `stream`
 * (a hipStream_t passed as void*) and is asynchronous unless stated
 * (wrnn_last_timing and wrnn_dm_sync_status wait; nothing else does).
 *
 * The TEAM2 / BATCH kernels keep n_teams * 32 workgroups spinning on each other inside one launch, so all of them
 * must be resident at once (one per CU).  Three layers make that a checked fact instead of a rule for the caller:
 *   1. wrnn_create asks the runtime's occupancy query about the instantiations this handle can launch (mode, profile
 *      build) and reads the CU count; where a team kernel cannot be resident (LDS / registers, fewer than 32 CUs) AUTO
 *      uses the SIMPLE kernel and an explicit request for a team kernel fails with WRNN_ERR_INVALID.
 *   2. Inside one process every team-kernel launch on a device -- any handle, any stream, wrnn_generate and
 *      wrnn_dm_generate alike -- is ordered behind the previous one with a per-device event (stream wait, nothing blocks
 *      on the host): two handles (RAW + MOL, two threads) share a GPU safely.
 *   3. Across processes nothing can be ordered; a team kernel whose workgroups do not all become resident within a short
 *      bounded wait at its start (another process holds CUs) gives up at once and the call reports WRNN_ERR_BUSY through
 *      wrnn_last_timing / wrnn_dm_sync_status -- retry, or use WRNN_KERNEL_SIMPLE.  The occupancy query cannot see other
 *      processes; this run-time check is what covers a shared GPU.
 */
#ifndef WAVERNN_AMD_H
#define WAVERNN_AMD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define WRNN_ABI_VERSION 9

/* mode: fatchord_version.py:98-103 */
#define WRNN_MODE_RAW 0 /* softmax over 2**bits classes */
#define WRNN_MODE_MOL 1 /* 10-component mixture of logistics, 30 outputs */

/* where the sampler's randomness comes from (fatchord_version.py:225-237,
 * wavernn/utils/distribution.py:87-123) */
#define WRNN_NOISE_PHILOX 0   /* device counter RNG keyed by (seed, step, row, class); utt_seeds_dev: per-utterance keys */
#define WRNN_NOISE_INJECTED 1 /* caller-supplied draws: parity protocol with the reference */
#define WRNN_NOISE_ARGMAX 2   /* RAW only: greedy (q == 1) */

/* which device implementation runs the per-sample loop */
#define WRNN_KERNEL_AUTO 0   /* rows <= XCD teams: TEAM2 (latency); more rows: BATCH_CS (throughput); SIMPLE when the team
                              * kernels cannot run on this device / configuration */
#define WRNN_KERNEL_SIMPLE 1 /* one workgroup per row, weights streamed from L2/HBM; any shape */
/* 2 was the 4-wave team kernel of ABI 2 (retired) */
#define WRNN_KERNEL_TEAM2 3  /* one XCD-resident 32-workgroup team per row, weights on chip, critical / shadow wave roles */
#define WRNN_KERNEL_BATCH 4  /* one team per 4 or 8 rows in lock-step on the matrix cores (v_mfma_f32_4x4x1) */
#define WRNN_KERNEL_BATCH_CS 5 /* ABI 5: the same batch step with two waves per SIMD -- critical / shadow wave roles, the shadow
                                * matrix products, noise and conditioning run beside the serial chain instead of inside it */
#define WRNN_KERNEL_TEAMG 6  /* added to ABI 9: one XCD team per row for ANY model dims -- layer shapes are run-time arguments, a workgroup
                              * keeps what fits of its weight slice in LDS and streams the rest; opt-in, AUTO never picks it */
#define WRNN_KERNEL_TEAMG_BATCH 7 /* added to ABI 9: the same kernel with 2..8 rows per team in lock-step (opts.batch_rows, 0 = the library's
                                   * choice) -- every weight load and every exchange serves all of them; each row is bit-equal to
                                   * WRNN_KERNEL_TEAMG's.  Opt-in; one row per team runs WRNN_KERNEL_TEAMG itself and reports 6 */

/* tensor dtypes accepted by wrnn_load_weights */
#define WRNN_DTYPE_F32 0
#define WRNN_DTYPE_I64 1

#define WRNN_OK 0
#define WRNN_ERR_INVALID -1     /* bad argument / unsupported configuration */
#define WRNN_ERR_HIP -2         /* a HIP runtime call failed */
#define WRNN_ERR_STATE -3       /* e.g. generate before load_weights */
#define WRNN_ERR_MISSING_KEY -4 /* state_dict key absent (strict load) */
#define WRNN_ERR_TIMEOUT -5     /* a bounded device spin gave up */
#define WRNN_ERR_BUSY -6        /* a team kernel could not get all its workgroups resident (GPU shared with another process) */
#define WRNN_ERR_UNSUPPORTED -7 /* a valid configuration this build has no kernel for (the mel front end: n_fft != 2048) */

typedef struct wrnn_handle wrnn_handle;

/* Constructor arguments of WaveRNN (fatchord_version.py:93-95) + device. */
typedef struct wrnn_config {
    int32_t rnn_dims;            /* 512  */
    int32_t fc_dims;             /* 512  */
    int32_t bits;                /* 10 (RAW) */
    int32_t pad;                 /* 2    */
    int32_t n_upsample;          /* 3    */
    int32_t upsample_factors[4]; /* 5,5,11 */
    int32_t feat_dims;           /* 80   */
    int32_t compute_dims;        /* 128  */
    int32_t res_out_dims;        /* 128  */
    int32_t res_blocks;          /* 10   */
    int32_t hop_length;          /* 275  */
    int32_t sample_rate;         /* 22050 */
    int32_t mode;                /* WRNN_MODE_* */
    int32_t device;              /* HIP device ordinal */
} wrnn_config;

/* One entry of the flat state_dict (fatchord_version.py:414-417; key names and
 * shapes listed in SURVEY.md section 8a).  `data` is a HOST pointer to a
 * contiguous row-major tensor; the library copies/repacks, the caller keeps
 * ownership. */
typedef struct wrnn_tensor_desc {
    const char *name;
    int32_t dtype; /* WRNN_DTYPE_* */
    int32_t ndim;
    int64_t shape[4];
    const void *data;
} wrnn_tensor_desc;

typedef struct wrnn_sample_opts {
    /* = sizeof(wrnn_sample_opts) of the CALLER.  The library refuses a size it does not know (WRNN_ERR_INVALID): a caller
     * built against another ABI revision fails loudly instead of having its fields read at shifted offsets. */
    uint32_t struct_size;
    int32_t noise_mode; /* WRNN_NOISE_* */
    int32_t kernel;     /* WRNN_KERNEL_* */
    /* != 0: mels_dev is (B, feat, T + 2*pad), already padded by `pad` frames on both sides with real context like the
     * training collate does and WaveRNN.forward receives it (:143); 0: (B, feat, T), zero padding applied on the fly
     * like generate() (:183-185).  T is the unpadded frame count either way.  It only moves where frame 0 lies in a row of
     * mels_dev, on every kernel: with batched != 0 the folds are cut from the conditioning of the T middle frames as before,
     * with frames_dev utterance b still runs frames_dev[b] * hop steps and its frames beyond frames_dev[b] are read as given
     * (zeros, as documented there).  A call whose 2*pad context frames are zero has the bits of the unpadded call in all three
     * forms (tests/test_gpu_forward_padded.py). */
    int32_t mels_padded;
    uint64_t seed;      /* WRNN_NOISE_PHILOX */
    /* WRNN_NOISE_INJECTED, device pointers, step-major like the reference's
     * RNG consumption (one sampler call per step, batch inside):
     *   RAW: noise1 = Exp(1) draws (L, rows, n_classes)   [torch.multinomial]
     *   MOL: noise1 = u_mix (L, rows, 10), noise2 = u_log (L, rows)          */
    const float *noise1_dev;
    const float *noise2_dev;
    /* teacher forcing: value fed back as x_t instead of the drawn sample,
     * (L, rows) device pointer or NULL */
    const float *x_forced_dev;
    /* optional dump of the fc3 outputs, (L, rows, n_classes) device or NULL */
    float *logits_out_dev;
    /* value fed to step 0 of every row instead of 0 (:196), (rows) device pointer or NULL.  With x_forced_dev this is
     * the teacher-forced pass of WaveRNN.forward (fatchord_version.py:131-167): input sequence x[0..L) = x_init,
     * x_forced[0..L-1), logits in logits_out_dev. */
    const float *x_init_dev;
    /* Ragged batch (unbatched mode only), device pointer to B int32 or NULL: utterance b has frames_dev[b] valid mel
     * frames (1 <= frames_dev[b] <= T; mels_dev stays (B, feat, T), zero beyond an utterance's own frames -- the padding
     * generate() itself applies, :183).  Row b then runs frames_dev[b] * hop steps instead of T * hop: its first
     * frames_dev[b] * hop outputs are exactly what a call on that clip alone produces under injected noise (rows are
     * independent, :194-196); under WRNN_NOISE_PHILOX the draws are keyed by (seed, step, row b), i.e. by the clip's place
     * in the batch, unless utt_seeds_dev gives every clip its own key.  The rest of the row is left unwritten.  The library orders the rows by length
     * on the device (longest first), fills team batches with rows of similar length and deals the batches to the teams
     * in snake order, so that no team idles behind a long clip. */
    const int32_t *frames_dev;
    /* tuning, 0 = the library's choice.  batch_rows: rows per team batch of WRNN_KERNEL_BATCH, 1..8 (default
     * ceil(rows / teams), at most 8).  team2_segment: steps per launch of WRNN_KERNEL_TEAM2 (a row is generated in
     * segments so that the conditioning stream of one segment stays cache resident; rounded down to a multiple of 32). */
    int32_t batch_rows;
    int32_t team2_segment;
    /* ABI 9.  Per-utterance seeds (WRNN_NOISE_PHILOX only), device pointer to B uint64 or NULL.  Every draw of utterance b is
     * keyed as a call on that clip ALONE with seed = utt_seeds_dev[b] keys it: key = all 64 bits of utt_seeds_dev[b], row word =
     * the row's index inside its utterance (fold i in wrnn_generate_folded, 0 in an unbatched wrnn_generate), step and class
     * words unchanged; `seed` is not read.  What a clip sounds like then does not depend on which clips share the call, on its
     * place among them, or on how a queue was dealt over devices: its rows are bit-equal to those of the solo call on the same
     * kernel with the same batch_rows / team2_segment.  The per-row keys are built on the device next to the row table (nothing
     * is staged on the host, the call never waits); the array must stay valid until that kernel has run.  NULL: the call-wide
     * `seed` and the row's index in the call, as before ABI 9.  WRNN_ERR_INVALID: with batched != 0 in wrnn_generate (one
     * utterance: `seed` already is its key), with any noise_mode other than WRNN_NOISE_PHILOX, and in wrnn_stream_open. */
    const uint64_t *utt_seeds_dev;
} wrnn_sample_opts;

typedef struct wrnn_timing {
    float prologue_ms; /* conditioning kernels of the last wrnn_generate */
    float loop_ms;     /* the per-sample loop kernel of the last wrnn_generate */
    int32_t kernel;    /* WRNN_KERNEL_* that actually ran */
    int32_t rows;      /* rows the loop processed (B or num_folds) */
    int64_t steps;     /* loop length per row */
    int32_t launches;  /* loop-kernel launches the call was split into (segments) */
    int32_t reserved_;
} wrnn_timing;

/* replaces WaveRNN.__init__ (fatchord_version.py:93-129) */
int wrnn_create(const wrnn_config *cfg, wrnn_handle **out);

/* replaces WaveRNN.load / load_state_dict (fatchord_version.py:414-417).  Every parameter the path reads must be
 * present with the reference's dtype and shape (WRNN_ERR_MISSING_KEY / WRNN_ERR_INVALID otherwise); keys the path does
 * not read (step, num_batches_tracked, optimizer leftovers) are ignored.  The reference's strict=False tolerance for
 * missing keys lives on the host side of the binding (nn.Module keeps its initial value for them). */
int wrnn_load_weights(wrnn_handle *h, const wrnn_tensor_desc *tensors, int32_t n);

/* Conditioning exactly as generate() builds it (fatchord_version.py:183-186:
 * pad_tensor 'both' + UpsampleNetwork.forward :82-89), materialised:
 *   mels_dev (B, feat, T) -> up_dev (B, T*hop, feat), aux_dev (B, T*hop, res_out)
 * mels_padded != 0: mels_dev is (B, feat, T + 2*pad) as WaveRNN.forward receives it (see wrnn_sample_opts).
 * Either output may be NULL.  Used by parity tests of the prologue; the loop
 * itself never materialises these tensors. */
int wrnn_conditioning(wrnn_handle *h, const float *mels_dev, int32_t B, int32_t T, int32_t mels_padded, float *up_dev,
                      float *aux_dev, void *stream);

/* Number of loop rows / steps generate() will run for (B, T, batched, target,
 * overlap): rows = B (unbatched) or num_folds (fold_with_overlap :293-340,
 * requires B == 1); steps = T*hop or target + 2*overlap. */
int wrnn_plan(wrnn_handle *h, int32_t B, int32_t T, int32_t batched, int32_t target, int32_t overlap,
              int32_t *rows_out, int64_t *steps_out);

/* replaces the device part of WaveRNN.generate (fatchord_version.py:183-241):
 * prologue + per-sample loop for all rows.
 *   labels_out_dev  (rows, steps) int32: RAW class index | MOL mixture index (may be NULL)
 *   samples_out_dev (rows, steps) fp32: the value appended to `output` (:227,:236)
 * The float64 epilogue (:243-258) and the wav write (:260) stay on the host
 * side of the binding. */
int wrnn_generate(wrnn_handle *h, const float *mels_dev, int32_t B, int32_t T, int32_t batched,
                  int32_t target, int32_t overlap, const wrnn_sample_opts *opts, int32_t *labels_out_dev,
                  float *samples_out_dev, void *stream);

/* replaces the float64 tail of generate() (fatchord_version.py:243-258): decode_mu_law (wavernn/utils/dsp.py:98-103)
 * when mu_law != 0 on a RAW model (needs labels_dev), xfade_and_unfold (:342-405) when batched != 0, the trim to
 * wave_len and the 20-hop linear fade-out (:255-258).  samples_dev / labels_dev: (rows, steps) as written by
 * wrnn_generate; wave_out_dev: wave_len doubles.  Unbatched calls use row 0 only, like :253.  wave_len shorter than
 * 20 hops is WRNN_ERR_INVALID (the reference raises ValueError for T < 21).  Asynchronous on `stream`. */
int wrnn_epilogue(wrnn_handle *h, const float *samples_dev, const int32_t *labels_dev, int32_t rows, int64_t steps,
                  int32_t batched, int32_t target, int32_t overlap, int32_t mu_law, int64_t wave_len,
                  double *wave_out_dev, void *stream);

/* The same tail for a batch of INDEPENDENT utterances (throughput mode, generate_many): every row r is finished like an
 * unbatched call finishes row 0 -- decode_mu_law (when mu_law != 0 on a RAW model), trim, 20-hop fade-out -- in ONE launch:
 *   wave_out_dev[r * out_stride + n], n < wave_len_r;  wave_len_r = wave_len, or (frames_dev[r] - 1) * hop when frames_dev
 *   (device, rows int32, the array given to wrnn_generate) is not NULL; out_stride >= wave_len doubles per row, entries
 *   [wave_len_r, out_stride) of a row are set to 0.  A row shorter than the 20-hop fade-out (the reference raises
 *   ValueError for T < 21, :256-258) is all zeros: the host side of the binding rejects such clips before the call. */
int wrnn_epilogue_rows(wrnn_handle *h, const float *samples_dev, const int32_t *labels_dev, int32_t rows, int64_t steps,
                       int32_t mu_law, int64_t wave_len, const int32_t *frames_dev, double *wave_out_dev, int64_t out_stride,
                       void *stream);

/* Host-only helper (no device): the float64 tables wrnn_epilogue gathers from, built in NumPy's evaluation order --
 * dec[n_classes] (decode_mu_law of 2k/(n_classes-1)-1, dsp.py:98-103), fade_in/fade_out[overlap] (:374-385, may be
 * NULL when overlap == 0), tail[20*hop] (np.linspace(1, 0, 20*hop_length), :256).  Caller-allocated. */
int wrnn_epilogue_tables(int32_t n_classes, int32_t overlap, int32_t hop, double *dec, double *fade_in, double *fade_out,
                         double *tail);

/* The loss the reference's training script applies to WaveRNN.forward's output (wavernn_train.py:82,112-121), forward value
 * only.  y_hat_dev (n_rows, n_classes) = the fc3 outputs of n_rows = B*L (batch, step) pairs, row-major.
 *   RAW model: F.cross_entropy -- y_dev = int32 class labels (n_rows); a label outside [0, n_classes) gives NaN.
 *   MOL model: discretized_mix_logistic_loss (wavernn/utils/distribution.py:16-84; num_classes 65536,
 *              log_scale_min log(1e-14), reduce=True) -- y_dev = float32 targets in [-1, 1] (n_rows).
 * loss_out_dev: one float32 on the device.  Asynchronous on `stream`. */
int wrnn_loss(wrnn_handle *h, const float *y_hat_dev, const void *y_dev, int64_t n_rows, float *loss_out_dev, void *stream);

/* ---- training step of the loop layers -------------------------------------------------------------------
 * WaveRNN.forward (fatchord_version.py:131-167) from the upsampled conditioning on, the training script's loss
 * (wavernn_train.py:82,112-121) and the backward pass of `loss.backward()` through I, rnn1, rnn2, fc1, fc2, fc3.
 * Every pointer is a DEVICE pointer to a contiguous float32 tensor in the reference's own layout (nn.Linear / nn.GRU:
 * weight (out, in), gate rows r | z | n) -- the parameters are used where torch keeps them, nothing is repacked, so an
 * optimizer step between two calls costs nothing here. */
typedef struct wrnn_loop_params {
    float *I_w, *I_b;                                   /* (rnn, 1 + feat + aux), (rnn)                 :115 */
    float *rnn1_w_ih, *rnn1_w_hh, *rnn1_b_ih, *rnn1_b_hh; /* (3 rnn, rnn) x2, (3 rnn) x2                  :117 */
    float *rnn2_w_ih, *rnn2_w_hh, *rnn2_b_ih, *rnn2_b_hh; /* (3 rnn, rnn + aux), (3 rnn, rnn), (3 rnn) x2 :118 */
    float *fc1_w, *fc1_b, *fc2_w, *fc2_b, *fc3_w, *fc3_b; /* (fc, rnn + aux), (fc, fc + aux), (n_classes, fc) :121-123 */
} wrnn_loop_params;

/*   w            parameters (read)
 *   g            gradients of the MEAN loss, same shapes (overwritten, not accumulated), or NULL: forward + loss only
 *   x_dev        (B, L) input samples                     mels_up_dev (B, L, feat), aux_dev (B, L, res_out): what
 *                self.upsample(mels) returns (:143), computed by the caller (the upsample network trains through the
 *                framework's autograd: BatchNorm in training mode needs batch statistics)
 *   y_dev        (B, L) targets: int32 class labels (RAW) / float32 in [-1, 1] (MOL); may be NULL when g and loss_out_dev are
 *   loss_out_dev one float32 (F.cross_entropy / discretized_mix_logistic_loss, as wrnn_loss) or NULL
 *   logits_out_dev (B, L, n_classes) fc3 outputs = forward()'s return value, or NULL
 *   d_mels_up_dev, d_aux_dev  gradients w.r.t. the conditioning (same shapes; written when g != NULL), or NULL
 * The handle supplies dims / mode and owns the workspace (grown on demand, ~86 KB per (batch, step) pair at the default
 * dims) and the captured step graphs; it needs no loaded weights.  Asynchronous on `stream`. */
int wrnn_train_step(wrnn_handle *h, const wrnn_loop_params *w, const wrnn_loop_params *g, const float *x_dev,
                    const float *mels_up_dev, const float *aux_dev, const void *y_dev, int32_t B, int64_t L,
                    float *loss_out_dev, float *logits_out_dev, float *d_mels_up_dev, float *d_aux_dev, void *stream);

/* The same computation split where autograd splits it -- so that the reference's own training loop runs unchanged
 * (`y_hat = model(x, m); loss = loss_func(y_hat, y); loss.backward()`, wavernn_train.py:103-122, with ANY loss on y_hat):
 *   wrnn_train_forward   forward() from the conditioning on (:145-167): logits_out_dev (B, L, n_classes); every activation stays in
 *                        the handle's workspace
 *   wrnn_train_backward  given d_logits_dev (B, L, n_classes) = d loss / d y_hat: the 16 parameter gradients g (overwritten) and the
 *                        gradients w.r.t. the conditioning (either may be NULL).  Must follow a wrnn_train_forward on the same handle
 *                        with the same B, L, inputs and parameters, with no other training call in between (WRNN_ERR_STATE otherwise). */
int wrnn_train_forward(wrnn_handle *h, const wrnn_loop_params *w, const float *x_dev, const float *mels_up_dev, const float *aux_dev,
                       int32_t B, int64_t L, float *logits_out_dev, void *stream);
int wrnn_train_backward(wrnn_handle *h, const wrnn_loop_params *w, const wrnn_loop_params *g, const float *d_logits_dev,
                        const float *x_dev, const float *mels_up_dev, const float *aux_dev, int32_t B, int64_t L,
                        float *d_mels_up_dev, float *d_aux_dev, void *stream);

/* Waits for `stream`, then reports the device-side error word of the team kernels wrnn_train_step launched (WRNN_ERR_BUSY,
 * WRNN_ERR_TIMEOUT) -- what wrnn_last_timing does for wrnn_generate. */
int wrnn_sync_status(wrnn_handle *h, void *stream);
/* The two GRU recurrences of wrnn_train_step run as one persistent XCD-team kernel each where rnn_dims is 512 and the device has
 * 32-CU teams, else as one kernel per time step replayed from a hipGraph.  on != 0 forces the per-step kernels (tests compare the two). */
int wrnn_train_force_step_kernels(wrnn_handle *h, int32_t on);
/* Added to ABI 9 (new entry points only).  What the two GRU recurrences of the last training call on h ran, and with how many rows per
 * team batch (0 for the step kernels); WRNN_ERR_STATE before any training call.  Either pointer may be NULL. */
#define WRNN_TRAIN_RAN_STEPS 0
#define WRNN_TRAIN_RAN_TEAM512 1
int wrnn_train_last_recurrence(const wrnn_handle *h, int32_t *kernel, int32_t *rows_per_team);
/* Host only, no device: the layout persistent team recurrences would have for a run-time rnn_dims at `rows` rows per team (1..4: a
 * 4-row instantiation, 5..8: an 8-row one), with the work split of the 512 kernels: units per workgroup = ceil(rnn_dims / 32), the
 * dynamic LDS of a forward and a backward kernel in bytes, and the 8-byte granules of one team's mailbox.  This build has no such
 * kernels yet; the plan says which rnn_dims they could take.  WRNN_ERR_INVALID: rnn_dims < 16 or no multiple of 16, rows outside 1..8
 * (nothing written).  WRNN_ERR_UNSUPPORTED: either kernel would need more than 160 KiB of LDS for its slice of W_hh (the figures are
 * written all the same); W_hh is not streamed from L2, such dims stay on the step kernels.  Any out pointer may be NULL. */
int wrnn_train_teamg_plan(int32_t rnn_dims, int32_t rows, int32_t *units_per_wg, int64_t *lds_fwd, int64_t *lds_bwd, int64_t *mail_granules);

/* Mixed-precision training, added to ABI 9 (new entry points only).  The precision belongs to the handle; the default is
 * WRNN_TRAIN_F32.  With WRNN_TRAIN_BF16 the batched GEMMs of the training calls -- forward, input gradients, weight gradients, the
 * d_aux / d_mels_up products -- round each operand element once to bfloat16 (nearest even) on its way to the matrix cores and
 * accumulate in fp32; memory stays fp32.  Not rounded: the two GEMMs that read x_dev (the sample input's column of I, forward and
 * gradient: they stay on the fp32 kernel), the recurrences and their W_hh, biases, bias gradients, losses and loss gradients.
 * bfloat16 keeps fp32's exponent range, so no loss scaling is involved.  WRNN_ERR_INVALID: fmt is neither value. */
#define WRNN_TRAIN_F32 0
#define WRNN_TRAIN_BF16 1
int wrnn_train_set_precision(wrnn_handle *h, int32_t fmt);
int wrnn_train_precision(const wrnn_handle *h, int32_t *fmt);
/* How many GEMMs the last training call on h launched on the fp32 and on the bf16 kernel (host-side counts; a split-K product counts
 * once).  WRNN_ERR_STATE before any training call.  Either pointer may be NULL. */
int wrnn_train_last_gemms(const wrnn_handle *h, int32_t *n_f32, int32_t *n_bf16);
/* Developer / test entry: one product C (M x N) = (beta) C + A.B (+ bias[N]) (relu) on the caller's device buffers through the GEMM
 * dispatcher and split-K wrapper of the training calls.  A(m,k) = ta ? A[k*lda + m] : A[m*lda + k], B(k,n) = tb ? B[n*ldb + k] :
 * B[k*ldb + n]; operands need 4-byte alignment only.  precision is taken literally.  slices: 1 = no split, 0 = the wrapper's own choice,
 * 2..64 = that many slices of K (slices past the end of K contribute zeros), summed in slice order from a temporary of this call's own --
 * a split product takes no bias and no relu, and the call then waits for the stream.  WRNN_ERR_UNSUPPORTED: ta and tb with
 * WRNN_TRAIN_BF16 (that kernel has the NT, NN and TN forms). */
int wrnn_debug_train_gemm(wrnn_handle *h, int32_t precision, int32_t ta, int32_t tb, const float *A, int64_t lda, const float *B,
                          int64_t ldb, float *C, int64_t ldc, int32_t M, int32_t N, int32_t K, int32_t beta, const float *bias,
                          int32_t relu, int32_t slices, void *stream);

/* Blocks until the last wrnn_generate on this handle finished, then reports
 * HIP-event timings and any device-side error (WRNN_ERR_TIMEOUT, WRNN_ERR_BUSY; WRNN_ERR_INVALID when the fold count a
 * folded call computed on the device differs from its rows_total). */
int wrnn_last_timing(wrnn_handle *h, wrnn_timing *out);

/* Developer instrumentation (replaces the WRNN_TEAM_PROF environment variable of ABI 3): enable != 0 makes the following
 * TEAM2 / BATCH calls of this handle run the instrumented instantiation of the loop kernel (s_memtime stamps between the
 * phases of a step; ~1 % slower).  wrnn_phase_cycles waits for the last call and returns, for workgroup 0 of team 0,
 * cycles per step of every phase marker: out[wave * 32 + marker], 8 waves x 32 markers (unused entries 0). */
int wrnn_phase_profile(wrnn_handle *h, int32_t enable);
int wrnn_phase_cycles(wrnn_handle *h, double *out /* [8 * 32] */);

/* n_classes (fatchord_version.py:98-101) and loop-parameter bytes (roofline) */
int32_t wrnn_n_classes(const wrnn_handle *h);
int64_t wrnn_loop_weight_bytes(const wrnn_handle *h);

/* ABI 6.  Can the XCD-team kernels (TEAM2 / BATCH / BATCH_CS: weights resident on chip) run for this handle on its device?  Returns 1 / 0;
 * *n_teams_out = number of 32-CU teams (8 on an MI355X in SPX mode; what the host side sizes fold counts and batches for),
 * *why_not_out = "" or the reason (points into the handle; valid until wrnn_destroy).  Either pointer may be NULL.  When the answer is 0,
 * WRNN_KERNEL_AUTO runs WRNN_KERNEL_SIMPLE -- reference-ordered, any dims, ~1 ms per step: slower than the reference on CPU cores -- and the
 * host side of the binding warns about it (the reference has no equivalent: this protects wavernn_gen.py:126's one call). */
int32_t wrnn_team_info(const wrnn_handle *h, int32_t *n_teams_out, const char **why_not_out);
/* Test hook: on != 0 makes this handle behave as if the residency check of wrnn_create had failed (AUTO -> SIMPLE, an explicit team kernel
 * -> WRNN_ERR_INVALID), so that the slow-path warning can be exercised on a healthy device. */
int wrnn_debug_force_no_teams(wrnn_handle *h, int32_t on);

/* ---- the team kernel for any dims (added to ABI 9: new entry points only, no existing entry or struct changes, so the number stays) ----
 * WRNN_KERNEL_TEAMG splits every loop layer by output rows over the 32 workgroups of an XCD team.  Layer order below = the order in
 * which layers are given LDS residency (shortest rows first): */
#define WRNN_TEAMG_FC3 0   /* fc3:  n_classes rows of fc_dims */
#define WRNN_TEAMG_FC2 1   /* fc2:  fc_dims rows of fc_dims + aux_dims */
#define WRNN_TEAMG_FC1 2   /* fc1:  fc_dims rows of rnn_dims + aux_dims */
#define WRNN_TEAMG_RNN2 3  /* rnn2: 3 rnn_dims gate rows of [W_ih2 (rnn_dims + aux_dims) | W_hh2 (rnn_dims)] */
#define WRNN_TEAMG_RNN1 4  /* rnn1: 3 rnn_dims gate rows of [W_ih1 (rnn_dims) | W_hh1 (rnn_dims)] */
#define WRNN_TEAMG_COND 5  /* I:    rnn_dims rows of feat_dims + aux_dims (the conditioning's share; the sample's column is a vector) */
#define WRNN_TEAMG_LAYERS 6
typedef struct wrnn_teamg_layer_info {
    int32_t units;           /* units owned as a whole: hidden units (rnn1, rnn2: the three gate rows of a unit stay together) or rows */
    int32_t rows_per_unit;   /* 3 (rnn1, rnn2) or 1 */
    int32_t k;               /* floats per row */
    int32_t k_padded;        /* as laid out for the kernel: every operand segment rounded up to 64 floats */
    int32_t own_first[32];   /* workgroup g owns units [own_first[g], own_first[g] + own_count[g]) */
    int32_t own_count[32];
    int32_t rows_min, rows_max;      /* output rows owned by a workgroup, over the 32 */
    int32_t resident_units;          /* the first resident_units of every workgroup's slice live in LDS, the rest is streamed */
    int32_t reserved_;
    int64_t weight_bytes;            /* units * rows_per_unit * k * 4 */
    int64_t resident_bytes_wg;       /* weight bytes resident in the fullest workgroup */
    int64_t resident_bytes_team;     /* ... summed over the 32 workgroups */
    int64_t streamed_bytes_step;     /* weight bytes the team reads from L2 / Infinity Cache every step;
                                      * resident_bytes_team + streamed_bytes_step == weight_bytes */
    int64_t lds_bytes;               /* LDS the resident part takes in every workgroup (padded rows) */
} wrnn_teamg_layer_info;
typedef struct wrnn_teamg_plan_info {
    wrnn_teamg_layer_info layer[WRNN_TEAMG_LAYERS];
    int64_t lds_budget_bytes;        /* the budget the placement was made for */
    int64_t activation_bytes;        /* LDS of the activation vectors */
    int64_t lds_bytes;               /* activation_bytes + sum of layer[].lds_bytes: the kernel's dynamic LDS, <= 160 KiB */
    int64_t streamed_bytes_step;     /* sum over the layers */
    int64_t mail_granules;           /* 8-byte {tag, value} granules of one team's mailbox */
} wrnn_teamg_plan_info;
/* Host only, no device: ownership and placement for the model `cfg` describes (device, sample_rate are not read).  lds_budget_bytes:
 * LDS a workgroup may spend on resident weights, < 0 = the default (160 KiB minus the activation vectors); a larger value is clamped to
 * the default.  WRNN_ERR_INVALID: bad arguments or dims wrnn_create refuses; WRNN_ERR_UNSUPPORTED: the activation vectors alone exceed
 * 160 KiB or the mailbox a team needs exceeds the library's (fc_dims far above 1024). */
int wrnn_teamg_plan(const wrnn_config *cfg, int64_t lds_budget_bytes, wrnn_teamg_plan_info *out);
/* Test hook in the style of wrnn_debug_force_no_teams: the following WRNN_KERNEL_TEAMG calls of this handle place their weights with
 * this LDS budget (< 0: back to the default), so that small models exercise the streamed and the mixed placement. */
int wrnn_debug_teamg_lds_budget(wrnn_handle *h, int64_t bytes);
/* WRNN_KERNEL_TEAMG_BATCH (added to ABI 9 like the above: new entry points and one kernel id, nothing existing changes).  The plan of
 * rows_per_team rows in lock-step: 1 = wrnn_teamg_plan itself; 2, 4, 8 = the kernel's instantiations (a batch of 3 rows runs on 4 with a
 * slot idle).  Ownership and the weight image are those of wrnn_teamg_plan; activation_bytes and mail_granules are for rows_per_team
 * rows, and the resident weights get what LDS the activation vectors leave.  WRNN_ERR_INVALID: also rows_per_team outside 1..8;
 * WRNN_ERR_UNSUPPORTED: the rows' activation vectors exceed 160 KiB, or their mailbox regions the library's mailbox.
 * wrnn_debug_teamg_lds_budget applies to both kernels. */
int wrnn_teamg_batch_plan(const wrnn_config *cfg, int32_t rows_per_team, int64_t lds_budget_bytes, wrnn_teamg_plan_info *out);
/* Rows per team batch of the last generate call's loop kernel (the batch kernels); 1 for the one-row kernels and before any call. */
int32_t wrnn_last_batch_rows(const wrnn_handle *h);
/* Half-precision weight image for WRNN_KERNEL_TEAMG and WRNN_KERNEL_TEAMG_BATCH (added to ABI 9 like the above: new entry points only).
 * WRNN_WEIGHTS_F16 stores the six matrices of the image as IEEE binary16, rounded to nearest even on the device with subnormals kept;
 * activations, accumulators, biases, the sample's column of I, cells and samplers stay fp32.  An fp16 weight converts to fp32 exactly and
 * the kernels multiply and add in the same order, so the outputs are bit-equal to the fp32 kernel's on a model whose matrices were
 * rounded to fp16 beforehand.  The format is a property of the handle, for both kernels; the default is WRNN_WEIGHTS_F32 and no other
 * kernel reads it.  Changing it drops the packed image, the next TEAMG / TEAMG_BATCH call packs again.  WRNN_ERR_INVALID: any other value.
 * A weight that does not round to a finite fp16 (|w| >= 65520) is found by the pack: the generate call that packs waits once for that
 * check and fails with WRNN_ERR_UNSUPPORTED, naming the layer; nothing is ever clamped, and the handle still generates in fp32. */
#define WRNN_WEIGHTS_F32 0
#define WRNN_WEIGHTS_F16 1
int wrnn_teamg_set_weight_format(wrnn_handle *h, int32_t fmt);
int32_t wrnn_teamg_weight_format(const wrnn_handle *h);
/* wrnn_teamg_batch_plan for a weight format.  WRNN_WEIGHTS_F32: that function byte for byte.  WRNN_WEIGHTS_F16: ownership, k and k_padded
 * (elements) are unchanged, every byte figure -- weight_bytes, resident_bytes_*, lds_bytes, streamed_bytes_step -- counts 2-byte
 * weights, and more units fit the same budget.  activation_bytes and mail_granules do not depend on the format. */
int wrnn_teamg_plan_fmt(const wrnn_config *cfg, int32_t rows_per_team, int32_t weight_format, int64_t lds_budget_bytes, wrnn_teamg_plan_info *out);
/* 8-bit weight image for the same two kernels (added to ABI 9: one new entry point, one new value).  WRNN_WEIGHTS_E4M3 stores the six
 * matrices as OCP e4m3fn bytes with ONE power-of-two scale per image layer (fc3, fc2, fc1, rnn2, rnn1, I[:, 1:]; a GRU layer is weight_ih
 * and weight_hh together, all three gates): s = 2^e, e the smallest integer with max|w| / 2^e <= 448, clamped to e >= -126 so that s
 * is a normal float; s = 1 for an all-zero layer.  A stored byte is RNE(w / s), subnormals kept; nothing can saturate.  The kernels
 * widen a byte exactly, multiply and add in the fp32 kernels' order and multiply a row's sums by s once; a power of two commutes with
 * every rounding, so the outputs are bit-equal to the fp32 kernels' on the dequantised model (byte * s), as long as no product of that
 * run is subnormal.  Weights below max|w| 2^-15 of their layer fall into e4m3's subnormals and lose relative precision; below
 * max|w| 2^-19 they become zero.  Everything else stays fp32 as with WRNN_WEIGHTS_F16.  The pack finds the six maxima on the device and
 * waits once for them; a weight that is not finite fails the generate call with WRNN_ERR_UNSUPPORTED, naming the layer, and the handle
 * still generates after WRNN_WEIGHTS_F32 is set.  A finite weight of any size is accepted: the scale absorbs it.
 * Value 2 is reserved and stays WRNN_ERR_INVALID in wrnn_teamg_set_weight_format and wrnn_teamg_plan_fmt.  With WRNN_WEIGHTS_E4M3
 * wrnn_teamg_plan_fmt counts 1-byte weights. */
#define WRNN_WEIGHTS_E4M3 3
/* The six scales of the image last packed on h, in the order fc3, fc2, fc1, rnn2, rnn1, I; 1.0 each for an fp32 or fp16 image, after a
 * refused pack and before any pack. */
int wrnn_teamg_weight_scales(const wrnn_handle *h, float out[6]);
/* Block-sparse weight image for the same two kernels (added to ABI 9: new entry points only).  A block is 64 consecutive
 * elements of one padded image row -- one gate row, segments A (the input's matrix) and B (W_hh) apart: 64-column chunks of fc3, fc2, fc1,
 * of every gate row of W_ih and, separately, of W_hh, and of I.weight[:, 1:] counted from column 1.  With the setting on, the pack reads
 * the pattern off the weights: a block is left out if and only if all its weights compare equal to zero (a NaN or an infinity is kept,
 * nothing is refused), the kernels walk every row's list of kept blocks in ascending order and feed the multiply-adds of the dense fp32
 * kernel in the same order.  fmaf(0, x, a) == a for finite x, so the outputs are equal, number for number, to the dense fp32 kernel's
 * on the same model, for any model.  Two caveats: where an activation is not finite the dense kernel yields NaN and the sparse one may
 * not, and a sum that is exactly zero may differ in the sign of zero.  The values stay fp32: with WRNN_WEIGHTS_F16 or WRNN_WEIGHTS_E4M3
 * also set, the generate call that would pack fails with WRNN_ERR_UNSUPPORTED naming both settings, and the handle generates again once
 * either is reset.  The setting is a property of the handle for both kernels, off by default, and no other kernel reads it; changing it
 * drops the packed image.  The pack waits once, for its census. */
int wrnn_teamg_set_sparse(wrnn_handle *h, int32_t on);
int32_t wrnn_teamg_sparse(const wrnn_handle *h);
/* Host only: wrnn_teamg_plan_fmt(.., WRNN_WEIGHTS_F32, ..) for the sparse image whose rows hold nb_a[l] blocks of segment A and nb_b[l] of
 * segment B in layer l (every row of a layer has its layer's longest list; shorter rows are padded with zero blocks).  An image row is
 * its 16-bit block indices, padded to 16 bytes, and its blocks of 64 floats; weight_bytes, resident_bytes_*, streamed_bytes_step and
 * lds_bytes count such rows, indices included (resident_bytes_team + streamed_bytes_step == weight_bytes, the image's bytes); k and
 * k_padded stay the dense row's.  WRNN_ERR_INVALID: also a count above the dense row's k_padded / 64 of its segment. */
int wrnn_teamg_sparse_plan(const wrnn_config *cfg, int32_t rows_per_team, const int32_t nb_a[6], const int32_t nb_b[6], int64_t lds_budget_bytes,
                           wrnn_teamg_plan_info *out);
/* The sparse image last packed on h, per layer in the order fc3, fc2, fc1, rnn2, rnn1, I: blocks kept (non-zero), blocks of the dense rows
 * (units * rows_per_unit * k_padded / 64), nb_a, nb_b, and the plan of the call that last ran it (its rows per team and LDS budget).
 * Any out pointer may be null.  WRNN_ERR_STATE: no sparse image has been packed since the setting, the format or the weights changed. */
int wrnn_teamg_sparse_info(wrnn_handle *h, int64_t kept[6], int64_t dense[6], int32_t nb_a[6], int32_t nb_b[6], wrnn_teamg_plan_info *plan);

/* ---- streaming generation (ABI 7) -------------------------------------------------------------------------------------------
 * Mel frames arrive a few at a time (Tacotron's decoder); audio leaves as soon as the frames it depends on are in.  A stream
 * fed the frames of mels (B, feat, T) in ANY partition into pushes and then ended produces exactly -- bit for bit -- the labels
 * and samples of wrnn_generate(mels, B, T, batched = 0, ...) with the same seed, noise mode and kernel: conditioning is local
 * in time (sample step t of frame i = t / hop reads mel frames i - pad .. i + pad only), the recurrent state crosses pushes
 * through device memory owned by the stream, and the Philox noise is keyed by (seed, absolute step, row, class).
 *
 * Planning rule (wrnn_stream_ready_steps): before the last push, (frames_in - pad) * hop steps are ready, rounded DOWN to a
 * multiple of 32 -- the TEAM2 kernel draws its Philox noise in 32-step blocks, so every resume point lies on a block boundary;
 * the last push releases all frames_in * hop steps (the frames after the end are the zero padding of generate(), :183-185).
 *
 * The stream owns its recurrent state, the conditioning tables of the frames in flight (a window of the newly ready frames
 * plus a `pad`-frame halo, recomputed from a bounded mel history: the workspace is bounded by the largest push, not by the
 * stream's length), its row table and its device error word; the handle lends only the team-kernel mailboxes inside the
 * per-device team gate.  Several streams and offline calls may be interleaved on one handle.  A stream is not thread-safe,
 * its pushes must be ordered on the device (one HIP stream), and it must be closed before its handle is destroyed. */
typedef struct wrnn_stream wrnn_stream;

/* B rows pushed in lock-step.  opts: struct_size as for wrnn_generate; noise_mode WRNN_NOISE_PHILOX (seed) or WRNN_NOISE_ARGMAX
 * (RAW); kernel WRNN_KERNEL_AUTO (TEAM2 where the team kernels can run, else SIMPLE), WRNN_KERNEL_TEAM2 or WRNN_KERNEL_SIMPLE.
 * WRNN_NOISE_INJECTED, the BATCH kernels, mels_padded, and every pointer / tuning field of opts set are WRNN_ERR_INVALID. */
int wrnn_stream_open(wrnn_handle *h, int32_t B, const wrnn_sample_opts *opts, wrnn_stream **out);

/* mels_dev (B, feat, n_frames) device, the next n_frames >= 0 frames of every row (may be NULL when n_frames == 0); last != 0
 * ends the utterance.  Enqueues every step that has become ready on `stream` and writes them to labels_out_dev (may be NULL)
 * and samples_out_dev as (B, *steps_out) row-major; out_capacity = elements each output array holds (>= B * *steps_out,
 * WRNN_ERR_INVALID otherwise; wrnn_stream_ready_steps tells the caller the size beforehand).  *steps_out is known on the host
 * at return, nothing waits.  mels_dev must stay valid until the push's work has run.  After the last push, or once the stream
 * is poisoned (see wrnn_stream_sync), a push is WRNN_ERR_STATE. */
int wrnn_stream_push(wrnn_stream *st, const float *mels_dev, int32_t n_frames, int32_t last, int32_t *labels_out_dev,
                     float *samples_out_dev, int64_t out_capacity, int64_t *steps_out, void *stream);

/* Waits for `stream`, then reports a device-side error of the pushes so far (WRNN_ERR_BUSY: a team kernel could not get its
 * workgroups resident; WRNN_ERR_TIMEOUT).  After either the stream is poisoned: later pushes return WRNN_ERR_STATE. */
int wrnn_stream_sync(wrnn_stream *st, void *stream);

/* frames pushed, steps enqueued, device bytes the stream owns (any pointer may be NULL) */
int wrnn_stream_info(const wrnn_stream *st, int64_t *frames_in, int64_t *steps_done, int64_t *workspace_bytes);

/* Host-only (no device): the planning rule above -- steps ready after frames_in frames; -1 for frames_in < 0, hop < 1, pad < 0. */
int64_t wrnn_stream_ready_steps(int64_t frames_in, int32_t hop, int32_t pad, int32_t last);

/* Waits for the device, then frees the stream's device memory.  NULL is a no-op. */
void wrnn_stream_close(wrnn_stream *st);

/* ---- fold mode for SEVERAL utterances in one call (ABI 8) --------------------------------------------------------------------
 * The reference folds one utterance (fold_with_overlap :293-340 indexes a batch-1 tensor).  A serving loop with several clips
 * queued folds ALL of them with one common fold length: every fold of every clip is one loop row of target + 2*overlap steps,
 * so the call fills the 8 x 8 rows of the batch kernel even when no single clip could.  Utterance b is cut exactly as a call
 * on that clip alone cuts it -- n_b folds by the rule of the plan entry above, fold i from position i * (target + overlap), zero
 * conditioning past the clip's OWN end frames[b] * hop (:327-330) -- and its folds are the consecutive rows
 * fold0[b] .. fold0[b + 1] - 1 of the outputs.
 *
 * Host only, no handle: fold0_out[b] = first row of utterance b, fold0_out[B] = rows in all (B + 1 entries); *steps_out =
 * target + 2*overlap (may be NULL).  total_b = frames_host[b] * hop samples.  WRNN_ERR_INVALID: bad arguments, frames_host[b] < 1, an
 * utterance that yields no fold (shorter than `overlap`), or more than INT32_MAX rows. */
int wrnn_plan_folded(const int32_t *frames_host, int32_t B, int32_t hop, int32_t target, int32_t overlap, int32_t *fold0_out,
                     int64_t *steps_out);

/* Prologue + loop of such a call.  mels_dev (B, feat, T), every clip right-zero-padded to T frames; frames_dev: B int32 on the
 * device, 1 <= frames_dev[b] <= T; rows_total = fold0_out[B] of the plan above for the same frames / target / overlap.
 *   labels_out_dev / samples_out_dev (rows_total, target + 2*overlap), as the generate entry writes them.
 * The row table is built on the device from frames_dev (nothing is staged on the host, the call never waits); when the
 * device's fold count differs from rows_total no row outside [0, rows_total) is touched and the timing entry reports
 * WRNN_ERR_INVALID.  Kernel choice, opts->batch_rows, opts->team2_segment, segmentation and the per-device team gate work as
 * for rows_total rows of one folded utterance; wrnn_timing.rows = rows_total.  Noise: WRNN_NOISE_INJECTED arrays are
 * (steps, rows_total, .); WRNN_NOISE_PHILOX keys fold i of utterance b by (opts->utt_seeds_dev[b], step, i) -- the draws of
 * wrnn_generate(clip b, batched = 1) with that seed, wherever the clip stands in the call -- or, when utt_seeds_dev is NULL, by
 * (opts->seed, step, GLOBAL row index fold0[b] + i): then a clip's draws depend on its position in the call.  The CUT of a
 * clip depends on `target` alone; a caller that derives target from the whole queue makes the audio depend on the queue
 * through the cut, whatever the seeds.  opts->frames_dev, mels_padded, x_forced_dev, x_init_dev and
 * logits_out_dev must be 0 / NULL (WRNN_ERR_INVALID). */
int wrnn_generate_folded(wrnn_handle *h, const float *mels_dev, int32_t B, int32_t T, const int32_t *frames_dev, int32_t rows_total,
                         int32_t target, int32_t overlap, const wrnn_sample_opts *opts, int32_t *labels_out_dev,
                         float *samples_out_dev, void *stream);

/* The float64 tail of every utterance of the last folded call on this handle, one launch: utterance b's rows are decoded,
 * crossfaded and unfolded with the arithmetic of the single-utterance tail (:342-405), trimmed to wave_len_b =
 * (frames_dev[b] - 1) * hop, faded out over the last 20 hops (:255-258) and written to wave_out_dev[b * out_stride + n];
 * entries [wave_len_b, out_stride) are set to 0, a clip shorter than the fade-out is all zeros (the host side rejects those).
 * Reads the fold offsets that call left on the handle: WRNN_ERR_STATE when there was none or its B, target, overlap or
 * rows_total differ.  steps must be target + 2*overlap. */
int wrnn_epilogue_folded(wrnn_handle *h, const float *samples_dev, const int32_t *labels_dev, int32_t B, int32_t rows_total,
                         int64_t steps, int32_t target, int32_t overlap, int32_t mu_law, const int32_t *frames_dev,
                         double *wave_out_dev, int64_t out_stride, void *stream);

const char *wrnn_last_error(const wrnn_handle *h);
int32_t wrnn_abi_version(void);
void wrnn_destroy(wrnn_handle *h);

/* ---- secondary model: wavernn/models/deepmind_version.py (unconditioned dual-softmax coarse/fine WaveRNN; no
 * reference script imports it).  Entry points mirror WaveRNN(hidden_size, quantisation) :9-31, load_state_dict and
 * generate(seq_len) :75-165.  noise_dev (WRNN_NOISE_INJECTED): Exp(1) draws (seq_len, 2, quantisation), [t][0] for the
 * coarse Categorical.sample() (:131), [t][1] for the fine one (:151).  Outputs: int32 (seq_len,) each; the signal is
 * coarse * 256 + fine - 2**15 (wavernn/utils/dsp.py:33-34), combined on the host side of the binding.  seq_len == 0 is
 * a successful no-op whose buffer pointers may be null. */
typedef struct wrnn_dm_handle wrnn_dm_handle;
int wrnn_dm_create(int32_t hidden_size, int32_t quantisation, int32_t device, wrnn_dm_handle **out);
int wrnn_dm_load_weights(wrnn_dm_handle *h, const wrnn_tensor_desc *tensors, int32_t n);
int wrnn_dm_generate(wrnn_dm_handle *h, int64_t seq_len, int32_t noise_mode, uint64_t seed, const float *noise_dev,
                     int32_t *coarse_out_dev, int32_t *fine_out_dev, void *stream);
/* kernel: 0 auto (the 32-workgroup team kernel when hidden_size is 512/640/768/896 and quantisation a multiple of
 * 64, else the single-workgroup kernel), 1 single workgroup (reference-ordered sums), 2 team */
int wrnn_dm_set_kernel(wrnn_dm_handle *h, int32_t kernel);
/* synchronises `stream` and reports the device-side error word of the team kernel (WRNN_ERR_TIMEOUT) */
int wrnn_dm_sync_status(wrnn_dm_handle *h, void *stream);
const char *wrnn_dm_last_error(const wrnn_dm_handle *h);
void wrnn_dm_destroy(wrnn_dm_handle *h);

/* ---- mel front end (added to ABI 9: new entry points only, no existing entry or struct changes, so the number stays): wav -> mel, the input side of wavernn_gen.py's `.wav` branch (:17-20) ----------------------------
 * melspectrogram(y) = normalize(amp_to_db(mel_basis @ |stft(y)|)) of wavernn/utils/dsp.py:41-43, 50-51, 58-59, 72-81 with the librosa
 * semantics of the reference's era: center=True with reflect padding of n_fft/2, a periodic Hann window of win_length centred in
 * n_fft, 1 + n / hop frames, n_fft/2 + 1 bins, the Slaney filterbank (htk=False, fmax = sample_rate/2, rows scaled by
 * 2 / (f[i+2] - f[i])), 20 log10(max(1e-5, .)) and clip((S - min_level_db) / -min_level_db, 0, 1); ref_level_db is NOT subtracted
 * (only spectrogram() does that, :66-69).  A front end of its own, not tied to a model handle: it needs no weights.
 * Supported: n_fft == 2048 (anything else: WRNN_ERR_UNSUPPORTED), 1 <= win_length <= n_fft, hop_length >= 1, 1 <= n_mels <= 128,
 * 0 <= fmin < sample_rate/2, min_level_db < 0 (else WRNN_ERR_INVALID).  The window, the twiddles and the sparse filterbank are built in
 * the create entry on the host in float64 and rounded to float32 once; that entry touches no device (a handle can be made and asked for
 * frame counts and tables on a machine without a GPU), the tables are uploaded by the first launch (one blocking copy; later calls are
 * asynchronous like the rest of the header). */
typedef struct wrnn_mel_handle wrnn_mel_handle;
typedef struct wrnn_mel_config {
    int32_t sample_rate;  /* 22050 */
    int32_t n_fft;        /* 2048  */
    int32_t hop_length;   /* 275   */
    int32_t win_length;   /* 1100  */
    int32_t n_mels;       /* 80    */
    float fmin;           /* 95    */
    float min_level_db;   /* -100  */
    int32_t device;       /* HIP device ordinal */
} wrnn_mel_config;
int wrnn_mel_create(const wrnn_mel_config *cfg, wrnn_mel_handle **out);
/* Host only: frames of a clip of n_samples, 1 + n_samples / hop_length; WRNN_ERR_INVALID (< 0) for a clip shorter than n_fft/2 + 1
 * samples, which cannot be reflect-padded (numpy refuses it too). */
int64_t wrnn_mel_frames(const wrnn_mel_handle *h, int64_t n_samples);
/* wav_dev: B float32 clips in one buffer, row stride n_max samples; n_samples_dev: B int32 on the device, the clips' own lengths
 * (ragged; a value above n_max is read as n_max); mel_out_dev (B, n_mels, T_max) float32 contiguous, the layout the generate entry
 * consumes.  Frames at or past a clip's own frame count are written as 0 -- the zero conditioning of a right-padded ragged batch --
 * and so is every frame of a clip too short to pad: the lengths live on the device and the call never waits, so the HOST side checks
 * them with the frames entry before the launch.  One launch, grid (T_max, B), asynchronous on `stream`. */
int wrnn_melspectrogram(wrnn_mel_handle *h, const float *wav_dev, int64_t n_max, const int32_t *n_samples_dev, int32_t B, int32_t T_max,
                        float *mel_out_dev, void *stream);
/* Host only (tests): copies of the float32 tables the kernel reads.  window[win_length]; twiddle[2 * n_fft] = (cos, -sin) of
 * 2 pi k / n_fft; rows[3 * n_mels] = (first_bin, n_bins, offset into weights) per filterbank row; weights[*n_weights] = the rows'
 * non-zero spans, packed.  Any pointer may be NULL (call once for *n_weights, then with buffers). */
int wrnn_mel_tables(const wrnn_mel_handle *h, float *window, float *twiddle, int32_t *rows, float *weights, int32_t *n_weights);
const char *wrnn_mel_last_error(const wrnn_mel_handle *h);
void wrnn_mel_destroy(wrnn_mel_handle *h);

/* Feature profiles of the mel front end (added to ABI 9 like the front end itself: one new struct and one new entry point, nothing
 * existing changes).  The features above are those of wavernn/utils/dsp.py.  The mels the reference's WaveRNN is trained on, and that
 * Tacotron hands it at synthesis time, come from another chain: tacotron/datasets/preprocessor.py:52-121, tacotron/datasets/audio.py:
 * 95-102, 203-207, 250-295, and the map to [0, 1] of wavernn_preprocess.py:149-159.  Every stage in which the two differ is a field
 * here, usable on its own.  For one clip x of n >= 1 samples:
 *   1. preemphasis k (0.97; 0 = off):        p[0] = x[0], p[i] = x[i] - k x[i-1]; p exists on [0, n) only.
 *   2. preemph_rescale r (0.999; 0 = off):   p <- p / max|p| * r; a clip with max|p| == 0 stays as it is.
 *   3. pad_mode:                              frame t reads p at t hop - n_fft/2 + i; outside [0, n) it is the reflection
 *                                             (WRNN_MEL_PAD_REFLECT, as above) or 0 (WRNN_MEL_PAD_ZERO, librosa pad_mode='constant').
 *                                             With zero padding a clip of any n >= 1 has 1 + n / hop frames.
 *   4. magnitude_power (2; 1 = as above):    the filterbank sees |X| or |X|^2 = re^2 + im^2.
 *   5. fmax (7600; 0 = sample_rate / 2):     the upper edge of the Slaney filterbank.
 *   6. ref_level_db (20; 0 = as above):      S = 20 log10(max(10^(min_level_db / 20), mel)) - ref_level_db.
 *   7. max_abs_value A (4; 0 = as above):    sym = clip(2 A ((S - min_level_db) / -min_level_db) - A, -A, A), the value Tacotron's
 *                                             preprocessing stores, then out = clip((sym + A) / (2 A), 0, 1).  A == 0: the direct
 *                                             clip((S - min_level_db) / -min_level_db, 0, 1).
 * The values in parentheses are the reference's (tacotron_hparams.py); the struct itself has no defaults.  All fields zero apart from
 * pad_mode = WRNN_MEL_PAD_REFLECT and magnitude_power = 1 is the profile of the plain create entry, and a handle made with it runs the
 * same kernel and gives the same bits (fmax changes the filterbank table only, and keeps that kernel too).  Any other profile runs a
 * second instantiation of that kernel, whose profile fields are run-time, workgroup-uniform switches; steps 1 to 3 are fused into its
 * tap gather (no pre-emphasised copy of a clip is written), and with preemph_rescale != 0 one reduction launch in front of it computes
 * the clips' pre-emphasised peaks into a workspace the handle owns (65535 floats, allocated with the tables), so calls on ONE handle
 * must be ordered by the caller (one stream at a time).  The call still never waits on the host.
 * WRNN_ERR_INVALID: struct_size other than sizeof(wrnn_mel_features), an unknown pad_mode, magnitude_power outside {1, 2}, fmax != 0
 * outside (fmin, sample_rate / 2], a negative (or NaN) preemphasis, preemph_rescale or max_abs_value, a ref_level_db that is not finite,
 * and whatever the plain create entry refuses.  n_fft != 2048 stays WRNN_ERR_UNSUPPORTED.  The frames, tables and launch entries above work
 * on either kind of handle; the frames entry refuses n < n_fft/2 + 1 under reflect padding and n < 1 under zero padding. */
#define WRNN_MEL_PAD_REFLECT 0
#define WRNN_MEL_PAD_ZERO 1
typedef struct wrnn_mel_features {
    uint32_t struct_size;    /* sizeof(wrnn_mel_features) */
    int32_t pad_mode;        /* WRNN_MEL_PAD_* */
    int32_t magnitude_power; /* 1 or 2 */
    float fmax;              /* Hz; 0 = sample_rate / 2 */
    float ref_level_db;
    float preemphasis;
    float preemph_rescale;
    float max_abs_value;
} wrnn_mel_features;
int wrnn_mel_create_features(const wrnn_mel_config *cfg, const wrnn_mel_features *features, wrnn_mel_handle **out);

/* ---- training data on the device (added to ABI 9 like the mel front end: two new functions, no struct and no existing entry changes,
 * so the number stays; a binding can tell a build from before them only by the missing symbols).  What wavernn_preprocess.py and
 * collate_vocoder (wavernn/utils/dataset.py:107-133) do on the host.  Neither entry takes a handle: there is no state and no error
 * text, only the status.  Both run on the device `stream` belongs to (the current device for the NULL stream), are asynchronous, and
 * check their arguments before any device call (WRNN_ERR_INVALID comes back on a machine without a GPU too).
 *
 * wrnn_quantise: labels_dev[i] = the class of sample wav_dev[i], 0 <= i < n, evaluated in float64 in the reference's operation order.
 * mu_law != 0: encode_mu_law(x, 2**bits) (wavernn/utils/dsp.py:92-95), floor((sign(x) log(1 + mu |x|) / log(1 + mu) + 1) / 2 * mu +
 * 0.5) with mu = 2**bits - 1; mu_law == 0: float_2_label(x, bits) (:12-15), (x + 1) * mu / 2, truncated like the collate's
 * .astype(int64).  Labels are clipped to [0, mu].  The reference asserts |x| <= 1; here every sample with |x| > 1 (or NaN) is ADDED to
 * *n_clipped_dev when that pointer is not NULL (the caller zeroes it and decides what the count means).  bits: 1 .. 16.  n == 0 is a
 * successful no-op whose pointers may be NULL; WRNN_ERR_INVALID for bits out of range, n < 0, or a NULL buffer with n > 0. */
int wrnn_quantise(const float *wav_dev, int64_t n, int32_t bits, int32_t mu_law, int32_t *labels_dev, int64_t *n_clipped_dev, void *stream);

/* One training batch cut from a corpus that lives on the device, one launch.  The corpus: labels_dev, the int32 labels of all
 * utterances, utterance u from element label_off_dev[u], at least (frames_dev[u] - 1) * hop of them (a wav of n samples has 1 + n / hop
 * frames); mels_dev, their mels, utterance u FRAMES-MAJOR (frames_dev[u], n_mels) float32 from element mel_off_dev[u] (the layout of the
 * reference's mel .npy files; a window is one contiguous run).  Row b of the batch takes utterance utt_dev[b] at mel frame
 * win_off_dev[b], as collate_vocoder does: with win = seq_len / hop + 2 * pad,
 *   mels_out[b] (n_mels, win) = frames win_off[b] .. win_off[b] + win, transposed;
 *   l = labels of the utterance from sample (win_off[b] + pad) * hop, seq_len + 1 of them;
 *   x_out[b, i] = label_2_float(l[i], sig_bits) = 2 * l[i] / (2**sig_bits - 1) - 1, every operation rounded to float32 (the divide
 *   correctly rounded): bit-equal to torch's float32 arithmetic;
 *   y_out[b, i] = l[i + 1] as int64 (y_float == 0, the RAW target), or label_2_float(l[i + 1], sig_bits) as float32 (the MOL target).
 * x_out, y_out (B, seq_len), mels_out (B, n_mels, win), contiguous.  The tables are on the device, so the caller validates utt and
 * win_off on the host before the call: 0 <= win_off[b] < frames[utt[b]] - 2 - (win + 2 * pad), the range collate_vocoder draws from
 * (:109-110).  The kernel re-checks that range against frames_dev and writes zeros for a row that fails; it never reads outside
 * an utterance of a valid table.  WRNN_ERR_INVALID: seq_len % hop != 0, B < 1 or > 65535, n_mels / hop / seq_len < 1, pad < 0,
 * sig_bits outside 1 .. 16, any NULL pointer. */
int wrnn_collate_windows(const int32_t *labels_dev, const float *mels_dev, const int64_t *label_off_dev, const int64_t *mel_off_dev,
                         const int32_t *frames_dev, const int32_t *utt_dev, const int32_t *win_off_dev, int32_t B, int32_t n_mels,
                         int32_t hop, int32_t pad, int32_t seq_len, int32_t sig_bits, int32_t y_float, float *x_out, void *y_out,
                         float *mels_out, void *stream);

/* ---- resampler (added to ABI 9 like the mel front end: new entry points only, so the number stays): wav at any integer sample rate ->
 * wav at the model's, what librosa.load(path, sr=hp.sample_rate) does in wavernn/utils/dsp.py:18-19 for a file at another rate.  For
 * src_rate -> dst_rate with g = gcd, p = dst / g, q = src / g, scale = min(1, p / q), half = ceil(64 / scale):
 *   y[t] = sum_{j = -half + 1 .. half} h(j - r / p) x[n + j],  n = (t q) / p,  r = (t q) % p  (64-bit integers; x is 0 outside the clip),
 *   h(u) = scale rolloff sinc(rolloff v) I0(beta sqrt(1 - (v / 64)^2)) / I0(beta) for v = scale |u| < 64, else 0,
 * rolloff = 0.9475937167399596, beta = 14.769656459379492: the Kaiser-windowed sinc with 64 zero crossings of the `kaiser_best` family
 * (the parameters of the reference's default resampler as far as we can tell; neither librosa nor resampy is available to compare with).
 * h is evaluated exactly at the p x 2 half tap positions in float64 and rounded to float32 once by the create entry (no table lookup, no
 * interpolation between table entries, no running float time register).  A clip of n samples gives ceil(n p / q) samples; librosa 0.7.2
 * computes int(n ratio) and pads to the ceiling, so the two differ in at most the last sample.
 * The create entry touches no device (WRNN_ERR_INVALID: a rate <= 0 or device < 0; WRNN_ERR_UNSUPPORTED: dst / src < 1/32, which bounds the
 * kernel's LDS span, or a bank of more than 2^24 entries); a refused handle is still returned, for its error text and the destroy entry.
 * The bank is uploaded by the first launch (one blocking copy; later calls are asynchronous). */
typedef struct wrnn_resample_handle wrnn_resample_handle;
int wrnn_resample_create(int32_t src_rate, int32_t dst_rate, int32_t device, wrnn_resample_handle **out);
/* Host only: ceil(n_in p / q); WRNN_ERR_INVALID (< 0) for n_in < 0 or >= 2^31, or a refused handle. */
int64_t wrnn_resample_out_len(const wrnn_resample_handle *h, int64_t n_in);
/* Host only (tests): the float32 bank, bank[r * taps + k] = h(k - half + 1 - r / p), p * taps entries with taps = 2 half; any pointer may
 * be NULL (call once for the sizes, then with a buffer). */
int wrnn_resample_bank(const wrnn_resample_handle *h, float *bank, int32_t *p, int32_t *q, int32_t *taps);
/* in_dev: B float32 clips in one buffer, row stride n_in_max samples; n_in_dev: B int32 on the device, the clips' own lengths (ragged; a
 * value above n_in_max is read as n_in_max).  Whatever the buffer holds past a clip's own length is never read.  out_dev (B, n_out_max)
 * float32: row b holds the ceil(n_in[b] p / q) samples of clip b (those below n_out_max) and ZEROS from there to n_out_max, the padding
 * the mel and quantise entries rely on; a row equals the call on that clip alone bit for bit.  One launch, grid (ceil(n_out_max / 256), B),
 * asynchronous on `stream`.  Equal rates: WRNN_ERR_INVALID (there is nothing to do, and the low-pass must not run at ratio 1). */
int wrnn_resample(wrnn_resample_handle *h, const float *in_dev, int64_t n_in_max, const int32_t *n_in_dev, int32_t B, int64_t n_out_max,
                  float *out_dev, void *stream);
const char *wrnn_resample_last_error(const wrnn_resample_handle *h);
void wrnn_resample_destroy(wrnn_resample_handle *h);

/* ---- wav conditioning (new entry points in ABI 9 again): the two steps the reference applies to every training wav between loading
 * it and the mel (tacotron/datasets/preprocessor.py:62-72): trim leading and trailing silence (audio.trim_silence =
 * librosa.effects.trim(wav, top_db, frame_length, hop)[0]), then wav / abs(wav).max() * rescaling_max.  For a clip x of n samples:
 *   p = x reflect-padded by frame_length / 2 on both sides (numpy mode='reflect'; needs n >= frame_length / 2 + 1),
 *   e[f] = mean(p[f hop : f hop + frame_length] ** 2) for the F = 1 + n / hop frames, summed in float64,
 *   frame f is non-silent when max(1e-10, e[f]) > 10 ** (-top_db / 10) * max(1e-10, max_f e), decided in float64
 *   (10 log10 of both sides is librosa's power_to_db(e, ref=np.max) > -top_db; librosa itself computes in float32),
 *   start = first_non_silent * hop, end = min(n, (last_non_silent + 1) * hop); digital silence is kept whole,
 *   peak = max |x[start : end]|,  y[i] = x[start + i] / peak * target: a correctly rounded float32 divide, then one float32 multiply;
 *   peak == 0 leaves the clip unscaled.
 * Non-finite samples promise nothing about values, only that nothing outside the clip is read and 0 <= start <= end <= n.
 * No handle, like wrnn_quantise: asynchronous on `stream`, nothing waits on the host, arguments are checked before any device call. */
/* Host only: the F = 1 + n / hop frames of a clip of n samples; WRNN_ERR_INVALID (< 0) for n < frame_length / 2 + 1 or a window
 * wrnn_condition refuses. */
int64_t wrnn_condition_frames(int64_t n, int32_t frame_length, int32_t hop);
/* wav_dev: B float32 clips in one buffer, row stride n_max; n_dev: B int32 on the device, the clips' own lengths (a value above n_max is
 * read as n_max, a negative one as 0; what lies past a clip is never read).  trim == 0: whole-clip bounds; peak_target == 0: no scaling;
 * both: WRNN_ERR_INVALID, there is nothing to do.  energy_ws_dev: caller-allocated workspace of B * F_max + B float64; the first
 * (B, F_max) are the frame energies (zeros at and past a clip's own F; frames past F_max are ignored, so F_max should be
 * wrnn_condition_frames of the longest clip; untouched when trim == 0), the last B are one 8-byte record per clip that the decision
 * launch leaves for the gather.  out_dev (B, n_out_max) float32 with n_out_max >= n_max: row b holds the end - start conditioned samples
 * from column 0 and ZEROS from there to n_out_max, the padding the mel and quantise entries rely on; it must not overlap wav_dev.
 * n_out_dev[b] = end - start, ready to be wrnn_melspectrogram's n_samples_dev.  bounds_dev (B, 2) int32 (start, end) and peak_dev (B)
 * float32 may be NULL.  A row equals the call on that clip alone bit for bit, energies included.  WRNN_ERR_INVALID: top_db <= 0 or
 * non-finite, frame_length outside 2 .. 8192, hop outside 1 .. frame_length, peak_target < 0 or non-finite, B outside 1 .. 65535,
 * n_max < 1, n_out_max < n_max or >= 2^31, F_max < 1, a NULL required pointer. */
int wrnn_condition(const float *wav_dev, int64_t n_max, const int32_t *n_dev, int32_t B, int32_t trim, double top_db, int32_t frame_length,
                   int32_t hop, float peak_target, double *energy_ws_dev, int32_t F_max, float *out_dev, int64_t n_out_max,
                   int32_t *n_out_dev, int32_t *bounds_dev, float *peak_dev, void *stream);

/* ---- Griffin-Lim (new entry points in ABI 9 again, and one new struct; nothing existing changes): [0, 1] mel -> wav with no trained
 * model, the inverse of the mel front end in either feature profile.  The chain is inv_mel_spectrogram of tacotron/datasets/audio.py:
 * 122-137, 176-186, 203-210, 256-260 (wavernn/utils/dsp.py:105-116 has a variant).  With the fields of wrnn_mel_config and
 * wrnn_mel_features above, for one mel column m of a clip of T frames:
 *   a. undo steps 7, 6 and 4 of the profile:  A = max_abs_value > 0: sym = clip(2 A m - A, -A, A),
 *                                               S_db = (sym + A) (-min_level_db) / (2 A) + min_level_db;
 *                                             A == 0: S_db = clip(m, 0, 1) (-min_level_db) + min_level_db;
 *                                             a = 10^((S_db + ref_level_db) / 20), then a^(1 / magnitude_power);
 *      lin = max(1e-10, P a), S = lin^power, with P the (n_fft/2 + 1) x n_mels pseudo-inverse of the profile's filterbank,
 *      P = B^T (B B^T)^-1 by a Cholesky factorisation of the Gram matrix, built in the create entry in float64 and kept in float64.
 *   b. first round: Z = S exp(2 pi i r), r per (frame, bin) zero, injected, or drawn on the device (below); y = istft(Z).
 *   c. n_iter rounds: X = stft(y), u = X / |X| (1 where |X| == 0), y = istft(S u).
 *   d. de-emphasis with k = preemphasis: out[i] = y[i] + k out[i-1] (k == 0: none).
 * stft is the profile's own (the window of win_length centred in n_fft, hop_length, frame t reads y at t hop - n_fft/2 + i, zeros or the
 * reflection outside the clip by pad_mode; the reflection repeats for a clip shorter than the pad, like numpy's).  istft is
 * librosa.istft with center=True: the inverse transforms times the window, overlap-added in ascending frame order, divided by the
 * window-sum-square where that exceeds FLT_MIN, and cut to the hop (T - 1) samples behind the first n_fft/2.  A clip of one frame is empty.
 * irfft reads the real parts of bins 0 and n_fft/2 only, as numpy's does.  The mel, the injected phases and the wav are float32;
 * everything between them is float64 (P, the window, the twiddles, S, the transforms, the frames and the wave between rounds, the
 * de-emphasis), rounded to float32 once per output sample: the rounds amplify rounding where a bin of the wave's spectrum passes near
 * zero, and a float32 chain drifts from the float64 one by far more than its one-round error.  Sums are gathers in a fixed order: two calls give the same bits, and a clip of a
 * ragged batch equals the call on it alone bit for bit.
 * The create entry touches no device.  It refuses what wrnn_mel_create_features refuses, a struct_size other than
 * sizeof(wrnn_griffin_config), power <= 0 and n_iter_default < 0 (WRNN_ERR_INVALID); n_fft != 2048, a filterbank with an empty row or
 * without full row rank (its Gram matrix does not factorise) are WRNN_ERR_UNSUPPORTED.  A refused handle is still returned, for its
 * error text and the destroy entry. */
#define WRNN_GRIFFIN_PHASE_ZERO 0      /* r = 0 */
#define WRNN_GRIFFIN_PHASE_PHILOX 1    /* r = the counter RNG's uniform in (0, 1) keyed (seed; frame, clip, bin): step = frame, row = clip,
                                        * element = bin of the generate entries' Philox4x32-10 stream */
#define WRNN_GRIFFIN_PHASE_INJECTED 2  /* r = phases_dev (B, T_max, n_fft/2 + 1) */
typedef struct wrnn_griffin_handle wrnn_griffin_handle;
typedef struct wrnn_griffin_config {
    uint32_t struct_size;    /* sizeof(wrnn_griffin_config) */
    float power;             /* 1.5: the exponent on the linear magnitudes (tacotron_hparams.py `power`) */
    int32_t n_iter_default;  /* 60: the rounds of a call with n_iter < 0 */
} wrnn_griffin_config;
int wrnn_griffin_create(const wrnn_mel_config *cfg, const wrnn_mel_features *features, const wrnn_griffin_config *griffin,
                        wrnn_griffin_handle **out);
/* Host only: hop_length (frames - 1), the samples of a clip of `frames` >= 1 mel frames; WRNN_ERR_INVALID (< 0) otherwise. */
int64_t wrnn_griffin_samples(const wrnn_griffin_handle *h, int64_t frames);
/* Host only (tests): pinv[(n_fft/2 + 1) * n_mels] = P row-major, window[win_length], and window_sumsquare[n_fft + hop (frames - 1)] =
 * the sum of the squared window over the frames that cover each position of the padded signal, summed as the overlap-add launch sums
 * it; all three are the float64 tables the kernels read, rounded to float32 here.  Any pointer may be NULL; `frames` is read for
 * window_sumsquare only. */
int wrnn_griffin_tables(const wrnn_griffin_handle *h, float *pinv, float *window, int32_t frames, float *window_sumsquare);
/* mel_dev (B, n_mels, T_max) float32 in [0, 1], the layout wrnn_melspectrogram writes and wrnn_generate reads; frames_dev: B int32 on the
 * device, the clips' own frame counts (ragged; read as clamped to 0 .. T_max).  n_iter < 0: the handle's n_iter_default.  phases_dev goes
 * with WRNN_GRIFFIN_PHASE_INJECTED and is NULL otherwise.  wav_out_dev (B, n_out_max) float32, n_out_max >= max(1, hop (T_max - 1)):
 * row b holds the hop (frames[b] - 1) samples of clip b and ZEROS from there on.  magnitude_out_dev: NULL, or (B, T_max, n_fft/2 + 1)
 * for S of step a (zero rows past a clip's own frames).  1 + 2 (1 + n_iter) + 1 launches (the last is the de-emphasis), asynchronous
 * on `stream`; nothing waits on the host and nothing is captured.  The handle owns the workspaces (S, the windowed frames, the wave)
 * and grows them when a call needs more -- the one case in which a call waits for `stream` -- so calls on ONE handle must be ordered by
 * the caller, as for a profile mel handle.  The tables are uploaded by the first call (one blocking copy). */
int wrnn_griffin_lim(wrnn_griffin_handle *h, const float *mel_dev, const int32_t *frames_dev, int32_t B, int32_t T_max, int32_t n_iter,
                     int32_t phase_mode, uint64_t seed, const float *phases_dev, float *wav_out_dev, int64_t n_out_max,
                     float *magnitude_out_dev, void *stream);
/* inv_preemphasis on its own, no handle (like wrnn_condition): out[b, i] = wav[b, i] + k out[b, i-1] for i < n_dev[b] (a value above
 * n_max is read as n_max, a negative one as 0), zeros from there to n_max; both buffers (B, n_max) float32, in place allowed.  The
 * recurrence runs in float64 as a blocked scan and is rounded to float32 once per sample.  One launch, one workgroup per clip.
 * WRNN_ERR_INVALID: |k| >= 1 or not finite, B outside 1 .. 65535, n_max < 1, a NULL pointer. */
int wrnn_deemphasis(const float *wav_dev, int64_t n_max, const int32_t *n_dev, int32_t B, double k, float *out_dev, void *stream);
const char *wrnn_griffin_last_error(const wrnn_griffin_handle *h);
void wrnn_griffin_destroy(wrnn_griffin_handle *h);

/* ---- spectral scores (new entry points in ABI 9 again, and one new struct; nothing existing changes): how far a TEST clip b is from a
 * TARGET clip a, both float32, compared over the n samples the caller passes for the pair (the shorter clip's length).
 * Mel scores.  Both clips go through the mel front end above, in either feature profile: Ma, Mb in [0, 1], (n_mels, T), T = 1 + n / hop_length.
 *   D = (Ma - Mb) (-min_level_db)                      dB, clipped at the floor as the front end clips
 *   lsd_t = sqrt(mean_m D[m, t]^2)                     the frame's log-mel distance in dB
 *   mcd_t = (10 / ln 10) sqrt(2 sum_{k = 1 .. K} c[k, t]^2),  c = C (D ln 10 / 20),  C[k, m] = sqrt(2 / n_mels) cos(pi k (m + 1/2) / n_mels)
 *                                                      (orthonormal DCT-II without c0), K = mcd_order; no time alignment
 * STFT scores, for every resolution r = (n_fft, hop, win): center=True with reflect padding of n_fft / 2, a periodic Hann window of win
 * centred in n_fft ((n_fft - win) / 2 zeros on its left), 1 + n / hop frames, n_fft / 2 + 1 bins; A = sqrt(max(re^2 + im^2, mag_floor))
 * of the target, B of the test:
 *   num_t = sum_k (B - A)^2,  den_t = sum_k A^2,  lm_t = sum_k |ln A - ln B|
 * The transform runs in float64 up to re^2 + im^2, which is rounded to float32 once per bin; the floor, the square root and the logarithm
 * are float32, and a frame's bin sums are carried in float64 and rounded once (|ln A - ln B| divides the transform's error by the bin's
 * magnitude, and a float32 transform does not keep the smallest bins of a noisy frame).
 * Per-frame values are float32.  The summaries are float64 sums of those float32 values, taken by a second launch in a fixed order (no
 * floating-point atomics: two calls give the same bits, and a clip of a ragged batch equals the call on it alone bit for bit):
 *   mel_lsd_db = mean_t lsd_t,  mcd_db = mean_t mcd_t,
 *   sc[r] = sqrt(sum_t num_t) / sqrt(sum_t den_t)      spectral convergence
 *   logmag[r] = sum_t lm_t / (frames bins)             log-magnitude distance
 *   mr_sc, mr_logmag = the means of sc[r], logmag[r] over the handle's resolutions.
 * Both clips of a frame run through the same instructions, so identical clips score exactly 0 everywhere, and so do two silences (both
 * sides sit at the floor; den_t is bins * mag_floor there, not 0).
 * The create entry touches no device.  `features` may be NULL: the default profile.  It refuses what the profile create entry of the
 * front end refuses (with that entry's status), and with WRNN_ERR_INVALID a struct_size other than the struct's own size, n_res outside
 * 1 .. 4, n_fft outside {256, 512, 1024, 2048}, win outside 1 .. n_fft, hop < 1, a mag_floor that is not finite and > 0, and mcd_order
 * outside 1 .. n_mels - 1.  A refused handle is still returned, for its error text and the destroy entry.
 * A clip needs max over the resolutions of n_fft / 2 + 1 samples (and the front end's own 1025 under reflect padding). */
#define WRNN_SCORE_MAX_RES 4
#define WRNN_SCORE_FIELDS 12       /* doubles per clip in summary_dev, in this order: */
#define WRNN_SCORE_MEL_LSD_DB 0
#define WRNN_SCORE_MCD_DB 1
#define WRNN_SCORE_MR_SC 2
#define WRNN_SCORE_MR_LOGMAG 3
#define WRNN_SCORE_SC0 4           /* sc[r] at 4 + r, 0 for r >= n_res */
#define WRNN_SCORE_LOGMAG0 8       /* logmag[r] at 8 + r, 0 for r >= n_res */
typedef struct wrnn_score_handle wrnn_score_handle;
typedef struct wrnn_score_config {
    uint32_t struct_size;    /* the size of this struct */
    int32_t n_res;           /* 1 .. WRNN_SCORE_MAX_RES */
    int32_t n_fft[4];        /* (512, 1024, 2048) */
    int32_t hop[4];          /* (50, 120, 240) */
    int32_t win[4];          /* (240, 600, 1200) */
    float mag_floor;         /* 1e-7: the floor under re^2 + im^2 */
    int32_t mcd_order;       /* 13 */
} wrnn_score_config;
int wrnn_score_create(const wrnn_mel_config *cfg, const wrnn_mel_features *features, const wrnn_score_config *score, wrnn_score_handle **out);
/* Host only: the frames of a clip of n samples at resolution r, 1 + n / hop[r]; r = -1: the mel's, 1 + n / hop_length.
 * WRNN_ERR_INVALID (< 0) for a clip shorter than the handle's shortest legal clip, r outside -1 .. n_res - 1, or a refused handle. */
int64_t wrnn_score_frames(const wrnn_score_handle *h, int32_t r, int64_t n);
/* target_dev, test_dev: B float32 clips each, row stride n_max; n_dev: B int32 on the device, the pairs' own lengths (ragged; a value
 * above n_max is read as n_max; a clip shorter than the shortest legal one has no frames and all-zero results: the lengths live on the
 * device and the call never waits, so the HOST side checks them with the frames entry).  summary_dev (B, WRNN_SCORE_FIELDS) float64.
 * frames_dev: NULL (the per-frame values go to the handle's scratch), or (B, frames_stride) float32.  A row holds, with F(r) the frames
 * entry's value for n_max samples: lsd[F(-1)] | mcd[F(-1)] | then for r = 0 .. n_res - 1: num[F(r)] | den[F(r)] | lm[F(r)]; frames_stride
 * is at least the sum of those.  Entries at or past a clip's own frame count are written as 0.  2 (+ 2 peak launches under a profile with
 * preemph_rescale) mel launches, 1 + n_res + 2 launches of this section, asynchronous on `stream`.  The handle owns the scratch (the two
 * mels, the sums, the per-frame values) and grows it when a call needs more -- the one case in which a call waits for `stream` -- so
 * calls on ONE handle must be ordered by the caller.  The tables are uploaded by the first call (one blocking copy). */
int wrnn_score(wrnn_score_handle *h, const float *target_dev, const float *test_dev, int64_t n_max, const int32_t *n_dev, int32_t B,
               double *summary_dev, float *frames_dev, int64_t frames_stride, void *stream);
/* Host only (tests): the tables the kernels read, as float32.  window[win[r]] and twiddle[2 * n_fft[r]] = (cos, -sin) of
 * 2 pi k / n_fft[r] of resolution r: the transform kernel reads these two in float64, they are rounded to float32 here;
 * dct[mcd_order * n_mels] = C rows 1 .. mcd_order, row-major, built in float64 and rounded once (the device copy is its transpose).
 * Any pointer may be NULL. */
int wrnn_score_tables(const wrnn_score_handle *h, int32_t r, float *window, float *twiddle, float *dct);
const char *wrnn_score_last_error(const wrnn_score_handle *h);
void wrnn_score_destroy(wrnn_score_handle *h);

/* ---- pitch (new entry points in ABI 9 again, and one new struct; nothing existing changes): a YIN F0 track (de Cheveigne & Kawahara
 * 2002) of float32 clips, and the F0 / voicing error scores of a TEST clip against a TARGET clip of the same length.  Every operation
 * after reading the float32 samples is float64: a threshold decision on a float32 difference function flips too easily.
 *   tau_min = ceil(sample_rate / fmax),  tau_max = floor(sample_rate / fmin)
 * Frames.  A clip of n >= 1 samples has T = 1 + n / hop frames (the mel front end's count at the same hop); frame t is the frame_length
 * samples from t hop - frame_length / 2, samples outside the clip read as zeros.  With x the frame and W = window:
 *   d(tau) = sum_{j < W} (x[j] - x[j + tau])^2                        tau = 0 .. tau_max + 1, the direct form
 *   d'(0) = 1,  d'(tau) = d(tau) tau / sum_{k = 1 .. tau} d(k)        1 wherever that sum is exactly 0 (silence, DC)
 *   candidate: the first tau in [tau_min, tau_max] with d'(tau) < threshold, then tau + 1 while tau + 1 <= tau_max and
 *              d'(tau + 1) < d'(tau) (both strict); none: no candidate
 *   voiced  <=>  a candidate exists and sqrt(mean_{j < W} x[j]^2) >= silence_rms
 *   a, b, c = d'(tau - 1), d'(tau), d'(tau + 1);  den = a - 2 b + c;  off = 0.5 (a - c) / den if den > 0 else 0, clamped to [-0.5, 0.5]
 *   f0 = sample_rate / (tau + off)                                     float32, rounded from float64 once; 0: unvoiced
 *   aperiodicity = min_{tau_min <= tau <= tau_max} d'(tau)             float32, rounded once
 * Pair scores over the tracks ft (target), fs (test), float64 from the float32 f0; V: the frames voiced in both clips:
 *   f0_rmse_cents = sqrt(mean_V (1200 log2(fs / ft))^2)
 *   gpe = #{t in V: |fs / ft - 1| > gpe_ratio} / #V                    gross pitch error
 *   vde = #{t: voiced_t != voiced_s} / T                               voicing decision error
 *   ffe = (#gpe frames + #vde frames) / T                              F0 frame error
 *   f0_corr = Pearson correlation of log2 f0 over V, in two passes: cov / sqrt(var_t var_s); 0 when #V < 2 or a variance is 0
 *   then the voiced frames of the target, of the test, and of both.
 * f0_rmse_cents, gpe and f0_corr are 0 when V is empty; a clip with n = 0 has no frames and an all-zero row.  The sums are taken by a
 * second launch in a fixed order (no floating-point atomics): two calls give the same bits, a clip of a ragged batch equals the call on
 * it alone bit for bit, and both clips of a pair run the same instructions, so identical clips (and two silences) score exactly 0 on
 * the first four fields. */
#define WRNN_PITCH_FIELDS 8        /* doubles per pair in summary_dev, in this order: */
#define WRNN_PITCH_F0_RMSE_CENTS 0
#define WRNN_PITCH_GPE 1
#define WRNN_PITCH_VDE 2
#define WRNN_PITCH_FFE 3
#define WRNN_PITCH_F0_CORR 4
#define WRNN_PITCH_VOICED_TARGET 5
#define WRNN_PITCH_VOICED_TEST 6
#define WRNN_PITCH_VOICED_BOTH 7
typedef struct wrnn_pitch_handle wrnn_pitch_handle;
typedef struct wrnn_pitch_config {
    uint32_t struct_size;    /* the size of this struct */
    int32_t sample_rate;     /* hp.sample_rate */
    int32_t hop;             /* hp.hop_length */
    int32_t frame_length;    /* 2048; one of 512, 1024, 2048, 4096 */
    int32_t window;          /* 1024: W, with window + tau_max + 1 <= frame_length */
    int32_t device;
    double fmin;             /* 60 */
    double fmax;             /* 600 */
    double threshold;        /* 0.15, inside (0, 1) */
    double silence_rms;      /* 1e-4 */
    double gpe_ratio;        /* 0.2 */
} wrnn_pitch_config;
/* Host only, touches no device.  A refused handle is still returned, for its error text and the destroy entry.  WRNN_ERR_INVALID: a
 * struct_size other than the struct's own size, sample_rate or hop < 1, fmin or fmax not finite or fmin >= fmax, tau_min < 1,
 * tau_min > tau_max, threshold outside (0, 1), silence_rms < 0 (or not finite), gpe_ratio <= 0 (or not finite), window < 1.
 * WRNN_ERR_UNSUPPORTED: frame_length outside {512, 1024, 2048, 4096}, window + tau_max + 1 > frame_length. */
int wrnn_pitch_create(const wrnn_pitch_config *cfg, wrnn_pitch_handle **out);
/* Host only: the frames of a clip of n samples, 1 + n / hop, and 0 for n = 0 (such a clip has no frames).  WRNN_ERR_INVALID (< 0) for
 * n < 0, n >= 2^31 or a refused handle. */
int64_t wrnn_pitch_frames(const wrnn_pitch_handle *h, int64_t n);
/* Host only: the lag range.  Either pointer may be NULL. */
int wrnn_pitch_lags(const wrnn_pitch_handle *h, int32_t *tau_min, int32_t *tau_max);
/* wav_dev: B float32 clips, row stride n_max >= 1; n_dev: B int32 on the device, the clips' own lengths (ragged; a value above n_max is
 * read as n_max, one below 1 as an empty clip).  f0_dev, aperiodicity_dev: (B, frames_stride) float32, frames_stride at least the
 * frames entry's value for n_max; aperiodicity_dev may be NULL.  Entries at or past a clip's own frame count are written as 0.  One
 * launch, asynchronous on `stream`; the entry owns no scratch. */
int wrnn_pitch_track(wrnn_pitch_handle *h, const float *wav_dev, int64_t n_max, const int32_t *n_dev, int32_t B, float *f0_dev,
                     float *aperiodicity_dev, int64_t frames_stride, void *stream);
/* target_dev, test_dev, n_dev: as above, pair by pair.  summary_dev (B, WRNN_PITCH_FIELDS) float64.  frames_dev: NULL (the per-frame
 * values go to the handle's scratch), or (B, frames_stride) float32; with F the frames entry's value for n_max a row holds
 * f0_t[F] | ap_t[F] | f0_s[F] | ap_s[F] | cents[F] (1200 log2(fs / ft) on the frames of V, 0 elsewhere) and frames_stride >= 5 F.
 * Three launches (the two tracks in one, the per-frame pair values, the summaries), asynchronous on `stream`.  The handle owns the
 * scratch and grows it when a call needs more -- the one case in which a call waits for `stream` -- so calls on ONE handle must be
 * ordered by the caller. */
int wrnn_pitch_score(wrnn_pitch_handle *h, const float *target_dev, const float *test_dev, int64_t n_max, const int32_t *n_dev, int32_t B,
                     double *summary_dev, float *frames_dev, int64_t frames_stride, void *stream);
const char *wrnn_pitch_last_error(const wrnn_pitch_handle *h);
void wrnn_pitch_destroy(wrnn_pitch_handle *h);

/* ---- time alignment (new entry points in ABI 9 again, and one new struct; nothing existing changes): the dynamic-time-warping path of
 * a TEST clip b (nb samples) against a TARGET clip a (na samples, need not equal nb) over their mel cepstra, and the scores along it.
 * The score and pitch sections above compare frame t with frame t; this one is for pairs that are not sample-aligned (trimmed clips, a
 * rendering of a predicted mel against the recording, two takes of a sentence).
 * Mels and cepstra.  Both clips go through the mel front end above, in either feature profile, exactly as wrnn_score runs it:
 * Ma (n_mels, Ta), Mb (n_mels, Tb) in [0, 1], T = 1 + n / hop_length.
 *   ca[k, i] = (sum_m C[k, m] Ma[m, i]) (-min_level_db) ln 10 / 20,  k = 1 .. K = mcd_order;  C = wrnn_score_tables' dct (the orthonormal
 *              DCT-II without row 0).  float32, rounded once from a float64 sum over m in ascending order; cb likewise.
 * Cost.
 *   d(i, j) = (10 / ln 10) sqrt(2 sum_k (ca[k, i] - cb[k, j])^2)     float32, rounded once from a float64 sum over k in ascending order.
 * Both clips' cepstra come out of the same instructions, so identical frames give d = 0 exactly.
 * Accumulated cost, float64.
 *   D(0, 0) = d(0, 0);  D(i, j) = d(i, j) + min(D(i - 1, j - 1), D(i - 1, j), D(i, j - 1)), leaving out predecessors outside the matrix.
 * The predecessor is picked in that order: the diagonal first, then (i - 1, j) if it is strictly smaller, then (i, j - 1) if it is
 * strictly smaller than the one held (so a NaN never displaces a held value).  One byte per cell records the choice.  The symmetric step
 * pattern with unit weights; no band, no slope constraint.
 * Path.  Backtracked from (Ta - 1, Tb - 1) to (0, 0) over the recorded choices, returned in ascending order: P pairs (i_p, j_p),
 * max(Ta, Tb) <= P <= Ta + Tb - 1.  The backtrack takes at most Ta + Tb - 1 steps whatever the matrix holds (NaN included): every step
 * lowers i + j and stays inside the matrix, and the loop has that bound of its own.
 * Summaries: WRNN_ALIGN_FIELDS float64 per pair, in a fixed order (no floating-point atomics: two calls give the same bits, and a pair
 * of a ragged batch equals the call on it alone bit for bit):
 *   total_cost = D(Ta - 1, Tb - 1),  path_len = P,  frames_target = Ta,  frames_test = Tb,  mcd_dtw_db = total_cost / P,
 *   mel_lsd_dtw_db = mean_p lsd_p,  lsd_p = sqrt(mean_m ((Ma[m, i_p] - Mb[m, j_p]) (-min_level_db))^2)      float64 from the float32 mels
 * and, with F0 tracks supplied (float32 as wrnn_pitch_track writes them, 0 = unvoiced; ft the target's, fs the test's; V the path pairs
 * voiced on both sides), in float64:
 *   f0_rmse_cents = sqrt(mean_V (1200 log2(fs[j_p] / ft[i_p]))^2),  gpe = #{p in V: |fs / ft - 1| > gpe_ratio} / #V,
 *   vde = #{p: voiced differs} / P,  ffe = (#gpe pairs + #vde pairs) / P,
 *   f0_corr = the Pearson correlation of log2 f0 over V in two passes, as wrnn_pitch_score defines it,  voiced_both = #V.
 * Without tracks these six are 0; f0_rmse_cents, gpe and f0_corr are 0 when V is empty.  A clip with no frames (shorter than the front
 * end can pad) gives an all-zero row, path_len = 0 and a path of -1.  Identical clips give the pure diagonal (P = T) and exactly 0 in
 * total_cost, mcd_dtw_db, mel_lsd_dtw_db, f0_rmse_cents, gpe, vde and ffe: equal frames cost exactly 0, every D is then >= 0 with 0 on
 * the diagonal, and the diagonal wins every tie.
 * Limits, checked on the host from B and the frames Ta_max, Tb_max of the longest clips (WRNN_ERR_UNSUPPORTED beyond them):
 *   min(Ta_max, Tb_max) <= 4096   one workgroup runs a pair's DP along the anti-diagonals and keeps three of them (s, s - 1, s - 2) in
 *                                 LDS as float64, indexed by the pair's shorter side: 3 x 4096 x 8 bytes = 96 KiB of the 160 KiB;
 *   B Ta_max Tb_max <= 2^28       a cell index fits 32 bits, and the scratch stays at 1 GiB of costs + 256 MiB of choice bytes.
 * and 1 <= B <= 65535 (WRNN_ERR_INVALID). */
#define WRNN_ALIGN_FIELDS 12       /* doubles per pair in summary_dev, in this order: */
#define WRNN_ALIGN_TOTAL_COST 0
#define WRNN_ALIGN_PATH_LEN 1
#define WRNN_ALIGN_FRAMES_TARGET 2
#define WRNN_ALIGN_FRAMES_TEST 3
#define WRNN_ALIGN_MCD_DTW_DB 4
#define WRNN_ALIGN_MEL_LSD_DTW_DB 5
#define WRNN_ALIGN_F0_RMSE_CENTS 6
#define WRNN_ALIGN_GPE 7
#define WRNN_ALIGN_VDE 8
#define WRNN_ALIGN_FFE 9
#define WRNN_ALIGN_F0_CORR 10
#define WRNN_ALIGN_VOICED_BOTH 11
typedef struct wrnn_align_handle wrnn_align_handle;
typedef struct wrnn_align_config {
    uint32_t struct_size;    /* the size of this struct */
    int32_t mcd_order;       /* 13 */
    double gpe_ratio;        /* 0.2 */
} wrnn_align_config;
/* Host only, touches no device.  `features` may be NULL: the default profile.  It refuses what the profile create entry of the front
 * end refuses (with that entry's status), and with WRNN_ERR_INVALID a struct_size other than the struct's own size, mcd_order outside
 * 1 .. n_mels - 1 and a gpe_ratio that is not finite and > 0.  A refused handle is still returned, for its error text and the destroy
 * entry. */
int wrnn_align_create(const wrnn_mel_config *cfg, const wrnn_mel_features *features, const wrnn_align_config *align, wrnn_align_handle **out);
/* Host only: the frames of a clip of n samples, 1 + n / hop_length.  WRNN_ERR_INVALID (< 0) for a clip the front end cannot pad (under
 * reflect padding fewer than n_fft / 2 + 1 samples, under zero padding none), n >= 2^31 or a refused handle. */
int64_t wrnn_align_frames(const wrnn_align_handle *h, int64_t n);
/* Host only: the bytes of scratch wrnn_align_score needs for B pairs whose longest clips have na_max and nb_max samples (the other
 * entries need less), or the negative status with which that call would be refused (the limits above; the text is in last_error). */
int64_t wrnn_align_workspace_bytes(wrnn_align_handle *h, int32_t B, int64_t na_max, int64_t nb_max);
/* target_dev: B float32 clips, row stride na_max; na_dev: B int32 on the device, their own lengths; test_dev, nb_max, nb_dev likewise
 * (ragged; a value above the stride is read as the stride; a clip too short to pad has no frames: the lengths live on the device and
 * the call never waits, so the HOST side checks them with the frames entry).  With Ta_max, Tb_max the frames entry's values for na_max,
 * nb_max: cost_dev (B, Ta_max, Tb_max) float32, d(i, j) of pair b at [b][i][j]; cells outside a pair's own Ta x Tb are written as 0.
 * 2 (+ 2 peak launches under a profile with preemph_rescale) mel launches and 2 of this section, asynchronous on `stream`. */
int wrnn_align_cost(wrnn_align_handle *h, const float *target_dev, int64_t na_max, const int32_t *na_dev, const float *test_dev, int64_t nb_max,
                    const int32_t *nb_dev, int32_t B, float *cost_dev, void *stream);
/* The generic part: the accumulated cost and the path over ANY float32 cost matrices.  cost_dev (B, Ta_max, Tb_max); ta_dev, tb_dev: B
 * int32 on the device, the pairs' own frame counts (read clamped to 0 .. Ta_max, 0 .. Tb_max).  path_dev (B, Ta_max + Tb_max - 1, 2)
 * int32, 8-byte aligned: (i_p, j_p) in ascending order, entries past P written as -1; path_len_dev (B) int32; total_dev (B) float64.
 * One launch, one workgroup per pair, asynchronous on `stream`. */
int wrnn_align_path(wrnn_align_handle *h, const float *cost_dev, int32_t B, int32_t Ta_max, int32_t Tb_max, const int32_t *ta_dev, const int32_t *tb_dev,
                    int32_t *path_dev, int32_t *path_len_dev, double *total_dev, void *stream);
/* The whole chain: mels, cepstra, costs, DP, path, the values along it, the summaries.  The clips as in wrnn_align_cost.
 * f0_target_dev, f0_test_dev: both NULL, or (B, f0_stride) float32 tracks at the mel's hop, f0_stride >= max(Ta_max, Tb_max).
 * summary_dev (B, WRNN_ALIGN_FIELDS) float64.  path_dev, path_len_dev: NULL, or as in wrnn_align_path.  per_path_dev: NULL, or
 * (B, 2, Ta_max + Tb_max - 1) float64: lsd_p, then 1200 log2(fs / ft) of the path pairs in V (0 elsewhere), zeros past P.
 * The mel launches, then 5 of this section, asynchronous on `stream`.  The handle owns the scratch and grows it when a call needs more
 * -- the one case in which a call waits for `stream` -- so calls on ONE handle must be ordered by the caller.  The DCT table is uploaded
 * by the first call (one blocking copy). */
int wrnn_align_score(wrnn_align_handle *h, const float *target_dev, int64_t na_max, const int32_t *na_dev, const float *test_dev, int64_t nb_max,
                     const int32_t *nb_dev, int32_t B, const float *f0_target_dev, const float *f0_test_dev, int64_t f0_stride, double *summary_dev,
                     int32_t *path_dev, int32_t *path_len_dev, double *per_path_dev, void *stream);
const char *wrnn_align_last_error(const wrnn_align_handle *h);
void wrnn_align_destroy(wrnn_align_handle *h);

/* ---- Tacotron-2: symbol ids -> mel ------------------------------------------------------------------------------------------------
 * Inference of the reference's default feature-prediction model (forward location-sensitive attention), free-running or
 * teacher-forced on a target (GTA).  Per utterance: embedding -> enc_conv_layers x (conv1d 'same' + bias -> ReLU -> BatchNorm) -> BiLSTM
 * (the memory) -> the decoder loop (prenet with dropout 0.5 always on, decoder_layers zoneout LSTMs, the attention with its
 * inference-only window block, the frame and stop projections) -> clip -> postnet -> projection + residual -> clip -> [0, 1].
 * Kernels: grid kernels for everything that is parallel in time; the encoder recurrences run one workgroup per direction per
 * utterance; the decoder loop runs ONE persistent workgroup per utterance with its state in LDS and decides the stop on the device
 * (p > 0.5 for any of a step's r tokens; that step's frames are still emitted), so a call never waits for the host per frame and no
 * workgroup waits for another.  Every loop is bounded by max_iters or Tx.  An utterance of a ragged batch gives the bits of the call
 * on it alone.  Prenet dropout: layer l of step s keeps unit k (scaled by 2) when the Philox uniform of the utterance's own seed at
 * counter (s * prenet_layers + l, row 0, k) is >= 0.5.
 * Limits (WRNN_ERR_INVALID with the reason in last_error): 1 <= Tx <= WRNN_TACO_MAX_TX symbols per utterance, ids inside
 * 0 .. n_symbols - 1, 1 <= B <= 65535, 1 <= prenet_layers <= WRNN_TACO_MAX_PRENET, 1 <= decoder_layers <= 4, every size >= 1,
 * conv kernels <= 64 taps, and a decoder state that fits 64 KiB of LDS. */
#define WRNN_TACO_MAX_TX 1024
#define WRNN_TACO_MAX_PRENET 4
typedef struct wrnn_taco_handle wrnn_taco_handle;
typedef struct wrnn_taco_dims {
    uint32_t struct_size;        /* the size of this struct */
    int32_t device;
    int32_t n_symbols, num_mels, outputs_per_step, embedding_dim;
    int32_t enc_conv_layers, enc_conv_channels, enc_conv_kernel, encoder_lstm_units;
    int32_t attention_dim, attention_filters, attention_kernel;
    int32_t prenet_layers, prenet_sizes[WRNN_TACO_MAX_PRENET];
    int32_t decoder_layers, decoder_lstm_units;
    int32_t postnet_layers, postnet_channels, postnet_kernel;
    float zoneout;               /* 0.1 */
    float max_abs_value;         /* 4 */
    float lower_bound_decay;     /* 0.1 */
    float bn_epsilon;            /* 1e-3 */
} wrnn_taco_dims;
typedef struct wrnn_taco_call {
    uint32_t struct_size;        /* the size of this struct */
    int32_t B, Tx_max;           /* utterances; the row stride of ids_host */
    int32_t max_iters;           /* decoder steps at most (free-running); >= 1 */
    int32_t prenet_dropout;      /* 0: no masks, no scaling */
    int32_t steps_max;           /* the step stride of the outputs: >= max_iters, with a target >= every gta_frames_host[b] / r */
    const int32_t *ids_host;     /* (B, Tx_max) */
    const int32_t *tx_host;      /* (B) symbols per utterance */
    const uint64_t *seeds_host;  /* (B) */
    const float *gta_dev;        /* NULL, or (B, gta_max, num_mels): step s >= 1 reads frame s r - 1 */
    int32_t gta_max;
    const int32_t *gta_frames_host; /* (B) multiples of r, 1 .. gta_max frames: the utterance runs gta_frames / r steps */
    /* caller-allocated, on the device; rows past an utterance's own length are written as 0 */
    float *encoder_dev;          /* NULL, or (B, Tx_max, 2 encoder_lstm_units) */
    float *decoder_dev;          /* (B, steps_max r, num_mels): the decoder's frames, clipped to [-max_abs - decay, max_abs] */
    float *mel_raw_dev;          /* (B, steps_max r, num_mels): after the postnet, the residual and the clip */
    float *mel_dev;              /* (B, steps_max r, num_mels): clip((clip(raw, -max_abs, max_abs) + max_abs) / (2 max_abs), 0, 1) */
    float *alignments_dev;       /* (B, steps_max, Tx_max) */
    float *stop_dev;             /* (B, steps_max r) probabilities */
    int32_t *max_attentions_dev; /* (B, steps_max) */
    int32_t *steps_dev;          /* (B) decoder steps run */
    int32_t *mel_frames_dev;     /* (B) free-running: the index of the first stop token > 0.5, else steps r; with a target: steps r */
} wrnn_taco_call;
/* Host only.  A refused handle is still returned, for its error text and the destroy entry. */
int wrnn_taco_create(const wrnn_taco_dims *dims, wrnn_taco_handle **out);
/* Host only: the tensors the model takes, named as the reference graph's variables below Tacotron_model/inference/.  The name entry
 * returns NULL and the shape entry a negative status outside 0 .. count - 1; shape_out takes up to 3 extents, the return is the rank. */
int wrnn_taco_tensor_count(const wrnn_taco_handle *h);
const char *wrnn_taco_tensor_name(const wrnn_taco_handle *h, int index);
int wrnn_taco_tensor_shape(const wrnn_taco_handle *h, int index, int64_t *shape_out);
/* One float32 tensor from host memory, C-contiguous, in the reference's own layout.  WRNN_ERR_MISSING_KEY: a name outside the table;
 * WRNN_ERR_INVALID: another shape, or a value that is not finite. */
int wrnn_taco_load_tensor(wrnn_taco_handle *h, const char *name, const float *data_host, int ndim, const int64_t *shape);
/* Checks everything on the host first, then uploads the weights (first call after a load), zeroes the outputs and launches; asynchronous
 * on `stream` but for the copies of ids, lengths and seeds.  WRNN_ERR_STATE: a tensor of the table has not been loaded (named). */
int wrnn_taco_synthesize(wrnn_taco_handle *h, const wrnn_taco_call *call, void *stream);
const char *wrnn_taco_last_error(const wrnn_taco_handle *h);
/* With streams still open the handle lives on until the last of them is closed (they read its weights); from then on
 * wrnn_taco_load_tensor, wrnn_taco_synthesize and wrnn_taco_stream_open on it are WRNN_ERR_STATE (the table queries and the error text
 * still answer). */
void wrnn_taco_destroy(wrnn_taco_handle *h);

/* ---- Tacotron-2, streaming: mel frames while the decoder is still running ---------------------------------------------------------
 * A stream is a free-running wrnn_taco_synthesize cut into pushes of decoder steps.  The encoder runs at open; every step entry
 * advances each unfinished utterance by up to n_steps steps from state kept in device memory (the last frame, h and c of every layer,
 * the context, the alignments and their sum, mu, the attention window's two counters, the first stop, the step count), then runs the
 * postnet over the rows that have become final, and waits once.  What comes out, concatenated over any partition into pushes, is what
 * wrnn_taco_synthesize writes for the same text, seeds, max_iters and prenet_dropout, bit for bit.
 * The release rule: a mel frame reads the decoder's frames up to halo = postnet_layers * ((k - 1) - (k - 1) / 2) rows ahead
 * (k = postnet_kernel, integer division: the right-hand reach of a 'same' convolution, once per layer; the 1-tap projection adds
 * nothing).  While an utterance runs, mel frames t < decoded - halo are final; once it has finished (a stop token above 0.5, or
 * max_iters steps) all mel_frames of them are.  decoder, alignments, stop and max_attentions of a step are final when it has run.
 * The stream owns all its memory (wrnn_taco_stream_info: workspace_bytes; each postnet layer keeps max_iters r rows per utterance),
 * the handle's scratch is not touched: offline calls and several streams of one handle may interleave on one HIP stream.  While a
 * stream is open wrnn_taco_load_tensor is WRNN_ERR_STATE.  Teacher forcing is not streamed. */
typedef struct wrnn_taco_stream wrnn_taco_stream;
typedef struct wrnn_taco_stream_opts {
    uint32_t struct_size;        /* the size of this struct */
    int32_t B, Tx_max;           /* utterances; the row stride of ids_host */
    int32_t max_iters;           /* decoder steps at most; >= 1; the step stride of the outputs */
    int32_t prenet_dropout;      /* 0: no masks, no scaling */
    const int32_t *ids_host;     /* (B, Tx_max) */
    const int32_t *tx_host;      /* (B) symbols per utterance */
    const uint64_t *seeds_host;  /* (B) */
    const float *gta_dev;        /* must be NULL: a target is WRNN_ERR_INVALID */
} wrnn_taco_stream_opts;
typedef struct wrnn_taco_stream_outputs {
    uint32_t struct_size;        /* the size of this struct, set by the caller */
    /* on the device, owned by the stream, full length, filled front to back; element strides between utterances */
    float *encoder_dev;          /* (B, Tx_max, 2 encoder_lstm_units), complete after open */
    float *decoder_dev;          /* (B, max_iters r, num_mels) */
    float *mel_raw_dev;          /* (B, max_iters r, num_mels) */
    float *mel_dev;              /* (B, max_iters r, num_mels) */
    float *alignments_dev;       /* (B, max_iters, Tx_max) */
    float *stop_dev;             /* (B, max_iters r) */
    int32_t *max_attentions_dev; /* (B, max_iters) */
    int32_t *steps_dev;          /* (B) decoder steps run so far */
    int32_t *mel_frames_dev;     /* (B) as wrnn_taco_call's once the utterance has finished */
    int64_t encoder_stride, frames_stride, alignments_stride, stop_stride, max_attentions_stride;
} wrnn_taco_stream_outputs;
/* Host only: the halo of the release rule for these dims; WRNN_ERR_INVALID (negative) for NULL, postnet_layers < 0 or
 * postnet_kernel < 1. */
int wrnn_taco_stream_halo(const wrnn_taco_dims *dims);
/* The host-side checks of wrnn_taco_synthesize, with its wording; then uploads the weights if a tensor was loaded since, allocates and
 * zeroes the stream's workspace and launches the encoder on `stream`.  A refusal leaves *out NULL and its reason in the HANDLE's
 * wrnn_taco_last_error. */
int wrnn_taco_stream_open(wrnn_taco_handle *h, const wrnn_taco_stream_opts *opts, void *stream, wrnn_taco_stream **out);
/* Up to n_steps >= 1 (WRNN_ERR_INVALID otherwise) more decoder steps of every unfinished utterance and the postnet rows they make
 * final, on `stream`; one wait; then per utterance (B entries each): decoder frames so far (steps r), final mel frames so far (the
 * release rule), finished (0 / 1).  A finished utterance's workgroups return at once.  WRNN_ERR_STATE once every utterance has
 * finished.  The pushes of one stream must be ordered on the device (one HIP stream). */
int wrnn_taco_stream_step(wrnn_taco_stream *st, int32_t n_steps, void *stream, int32_t *decoded_host, int32_t *final_host, int32_t *finished_host);
int wrnn_taco_stream_view(const wrnn_taco_stream *st, wrnn_taco_stream_outputs *out);
/* any pointer may be NULL */
int wrnn_taco_stream_info(const wrnn_taco_stream *st, int32_t *B, int32_t *Tx_max, int32_t *max_iters, int32_t *halo, int64_t *workspace_bytes);
const char *wrnn_taco_stream_last_error(const wrnn_taco_stream *st);
/* Frees the stream's memory (the free waits for work that still uses it).  NULL is a no-op.  Close a stream before its handle is destroyed (see
 * wrnn_taco_destroy for what happens otherwise). */
void wrnn_taco_stream_close(wrnn_taco_stream *st);

/* ---- Tacotron-2, the GTA corpus: a corpus's ground-truth mels -> the mels the model predicts under teacher forcing -------------------
 * What the reference's wavernn_preprocess.py does per utterance (feed the recording's own frames to the decoder, keep
 * mel[:target_length], map to [0, 1]), for a group of B utterances of a mel table that lives on the device, written into a table of the
 * same layout.  Utterance b is (frames_host[b], num_mels) float32 in [0, 1], frames-major, from element mel_off_host[b] of mels_dev;
 * its GTA mel goes to element out_off_host[b] of gta_mels_dev.
 * The target: the pack kernel builds the (B, gta_max, num_mels) target wrnn_taco_synthesize reads from the [0, 1] mel m, with
 * A = max_abs_value, gta_max = r ceil(max frames / r): row t < frames is clip(fl(fl(2A m) - A), -A, A) in float32 (fl: one rounding
 * each, no fused multiply-add); rows from frames up to the next multiple of r are -A (the reference's padding_targets); rows past that
 * are 0.  This formula IS the definition of the target.  The mel front end computes m = clip((sym + A) / 2A, 0, 1) from its internal
 * sym = clip(2A n - A, -A, A); the target equals that sym wherever sym <= -A / 2 and lies within one float32 spacing of 2A (ulp(2A))
 * of it elsewhere.  A corpus loaded from files has only m, which is why the target is defined from it.
 * Then encoder, decoder, postnet and finish run exactly as wrnn_taco_synthesize launches them with that target, gta_frames
 * r ceil(frames / r) and steps_max = gta_max / r, every intermediate output in scratch this entry owns (not the scratch of
 * wrnn_taco_synthesize).  The unpack kernel (one workgroup per utterance) copies the first frames[b] rows of that call's [0, 1] mel
 * to the output table and writes l1[b] = mean |gta - ground truth| over them; the alignment kernel (one workgroup per utterance)
 * writes focus[b] = the mean over the utterance's steps of max_t alignments[s, t], and last_attention[b] = max_attentions of the last
 * step.  Both sums are float64 with a fixed assignment of elements to threads and a fixed tree: a second call gives the same bits.
 * Waiting: the call never waits for the device.  Every host array is read by a copy queued on `stream`, so the arrays must stay
 * unchanged until the stream has passed the call; give page-locked memory, so that the copies are asynchronous.  The scratch grows on
 * demand, and growing it waits for `stream`: a group whose need exceeds what is reserved waits once.  The need grows with B, Tx_max and
 * the longest utterance, so wrnn_taco_gta_reserve for the largest B, Tx_max and frame count of a corpus, before its first group, leaves
 * no group a wait (wrnn_taco_gta_workspace_bytes reports what is reserved; it never shrinks).  The first call after a load uploads the
 * weights (one blocking copy).  Calls on one handle must be ordered by the caller (one HIP stream).
 * Refusals (WRNN_ERR_INVALID): those of wrnn_taco_synthesize in its wording; frames < 1; frames above 2^24; an offset or extent
 * outside mels_elems / out_elems; a NULL input table or output. */
typedef struct wrnn_taco_gta_call {
    uint32_t struct_size;        /* the size of this struct */
    int32_t B, Tx_max;           /* utterances; the row stride of ids_host */
    int32_t prenet_dropout;      /* 0: no masks, no scaling */
    const int32_t *ids_host;     /* (B, Tx_max) */
    const int32_t *tx_host;      /* (B) symbols per utterance */
    const uint64_t *seeds_host;  /* (B) */
    const int32_t *frames_host;  /* (B) mel frames per utterance, >= 1 */
    const int64_t *mel_off_host; /* (B) the utterance's first element in mels_dev */
    const int64_t *out_off_host; /* (B) the utterance's first element in gta_mels_dev */
    const float *mels_dev;       /* the ground-truth table, mels_elems float32 */
    int64_t mels_elems;
    float *gta_mels_dev;         /* the output table, out_elems float32; only the B utterances' own elements are written */
    int64_t out_elems;
    double *l1_dev;              /* (B) */
    double *focus_dev;           /* (B) */
    int32_t *last_attention_dev; /* (B) */
} wrnn_taco_gta_call;
int wrnn_taco_gta_corpus(wrnn_taco_handle *h, const wrnn_taco_gta_call *call, void *stream);
/* Grows the scratch of wrnn_taco_gta_corpus to what a group of B utterances of up to Tx_max symbols and frames_max mel frames needs
 * (the one wait, and only when it grows).  WRNN_ERR_INVALID: B, Tx_max or frames_max outside what wrnn_taco_gta_corpus serves. */
int wrnn_taco_gta_reserve(wrnn_taco_handle *h, int32_t B, int32_t Tx_max, int32_t frames_max, void *stream);
/* Host only: bytes of that scratch now (0 before the first reserve or call, and for NULL). */
int64_t wrnn_taco_gta_workspace_bytes(const wrnn_taco_handle *h);

#ifdef __cplusplus
}
#endif
#endif /* WAVERNN_AMD_H */
