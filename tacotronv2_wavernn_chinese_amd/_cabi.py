"""ctypes binding of libwavernn_amd.so (C-ABI: include/wavernn_amd.h).

The library is the product's only compute path: importing this module without
a built ``csrc/libwavernn_amd.so`` raises -- there is no CPU or PyTorch
fallback (the CPU restatement under ``oracle/`` is test infrastructure and is
never imported from here).
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Dict, Iterable, Optional, Tuple

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, 'csrc', 'libwavernn_amd.so')

MODE_RAW, MODE_MOL = 0, 1
NOISE_PHILOX, NOISE_INJECTED, NOISE_ARGMAX = 0, 1, 2
KERNEL_AUTO, KERNEL_SIMPLE, KERNEL_TEAM2, KERNEL_BATCH, KERNEL_BATCH_CS, KERNEL_TEAMG, KERNEL_TEAMG_BATCH = 0, 1, 3, 4, 5, 6, 7
KERNEL_NAMES = {KERNEL_AUTO: 'auto', KERNEL_SIMPLE: 'simple', KERNEL_TEAM2: 'team2', KERNEL_BATCH: 'batch', KERNEL_BATCH_CS: 'batch_cs',
                KERNEL_TEAMG: 'teamg', KERNEL_TEAMG_BATCH: 'teamg_batch'}
KERNEL_IDS = {v: k for k, v in KERNEL_NAMES.items()}
DTYPE_F32, DTYPE_I64 = 0, 1
ERR_NAMES = {0: 'WRNN_OK', -1: 'WRNN_ERR_INVALID', -2: 'WRNN_ERR_HIP', -3: 'WRNN_ERR_STATE',
             -4: 'WRNN_ERR_MISSING_KEY', -5: 'WRNN_ERR_TIMEOUT', -6: 'WRNN_ERR_BUSY', -7: 'WRNN_ERR_UNSUPPORTED'}
ERR_INVALID, ERR_STATE, ERR_TIMEOUT, ERR_BUSY, ERR_UNSUPPORTED = -1, -3, -5, -6, -7
ABI_VERSION = 9   # WRNN_ABI_VERSION of the include/wavernn_amd.h this binding was written against

# every symbol include/wavernn_amd.h declares (checked by tests/test_cabi_symbols.py)
EXPORTED_SYMBOLS = ('wrnn_create', 'wrnn_load_weights', 'wrnn_conditioning', 'wrnn_plan', 'wrnn_generate',
                    'wrnn_last_timing', 'wrnn_n_classes', 'wrnn_loop_weight_bytes', 'wrnn_last_error',
                    'wrnn_abi_version', 'wrnn_destroy', 'wrnn_epilogue', 'wrnn_epilogue_rows', 'wrnn_epilogue_tables', 'wrnn_loss',
                    'wrnn_phase_profile', 'wrnn_phase_cycles', 'wrnn_train_step', 'wrnn_train_forward', 'wrnn_train_backward', 'wrnn_sync_status', 'wrnn_train_force_step_kernels',
                    'wrnn_dm_create', 'wrnn_dm_load_weights', 'wrnn_dm_generate', 'wrnn_dm_last_error', 'wrnn_dm_destroy',
                    'wrnn_dm_set_kernel', 'wrnn_dm_sync_status', 'wrnn_team_info', 'wrnn_debug_force_no_teams',
                    'wrnn_stream_open', 'wrnn_stream_push', 'wrnn_stream_sync', 'wrnn_stream_info', 'wrnn_stream_ready_steps',
                    'wrnn_stream_close', 'wrnn_plan_folded', 'wrnn_generate_folded', 'wrnn_epilogue_folded',
                    'wrnn_mel_create', 'wrnn_mel_frames', 'wrnn_melspectrogram', 'wrnn_mel_tables', 'wrnn_mel_last_error', 'wrnn_mel_destroy',
                    'wrnn_mel_create_features',
                    'wrnn_quantise', 'wrnn_collate_windows',
                    'wrnn_resample_create', 'wrnn_resample_out_len', 'wrnn_resample_bank', 'wrnn_resample', 'wrnn_resample_last_error',
                    'wrnn_resample_destroy', 'wrnn_condition_frames', 'wrnn_condition', 'wrnn_teamg_plan', 'wrnn_debug_teamg_lds_budget',
                    'wrnn_teamg_batch_plan', 'wrnn_last_batch_rows', 'wrnn_teamg_set_weight_format', 'wrnn_teamg_weight_format',
                    'wrnn_teamg_plan_fmt', 'wrnn_teamg_weight_scales', 'wrnn_teamg_set_sparse', 'wrnn_teamg_sparse', 'wrnn_teamg_sparse_plan',
                    'wrnn_teamg_sparse_info', 'wrnn_train_last_recurrence', 'wrnn_train_teamg_plan',
                    'wrnn_train_set_precision', 'wrnn_train_precision', 'wrnn_train_last_gemms', 'wrnn_debug_train_gemm',
                    'wrnn_griffin_create', 'wrnn_griffin_samples', 'wrnn_griffin_tables', 'wrnn_griffin_lim', 'wrnn_deemphasis',
                    'wrnn_griffin_last_error', 'wrnn_griffin_destroy',
                    'wrnn_score_create', 'wrnn_score_frames', 'wrnn_score', 'wrnn_score_tables', 'wrnn_score_last_error',
                    'wrnn_score_destroy',
                    'wrnn_pitch_create', 'wrnn_pitch_frames', 'wrnn_pitch_lags', 'wrnn_pitch_track', 'wrnn_pitch_score',
                    'wrnn_pitch_last_error', 'wrnn_pitch_destroy',
                    'wrnn_align_create', 'wrnn_align_frames', 'wrnn_align_workspace_bytes', 'wrnn_align_cost', 'wrnn_align_path',
                    'wrnn_align_score', 'wrnn_align_last_error', 'wrnn_align_destroy',
                    'wrnn_taco_create', 'wrnn_taco_tensor_count', 'wrnn_taco_tensor_name', 'wrnn_taco_tensor_shape', 'wrnn_taco_load_tensor',
                    'wrnn_taco_synthesize', 'wrnn_taco_last_error', 'wrnn_taco_destroy',
                    'wrnn_taco_stream_halo', 'wrnn_taco_stream_open', 'wrnn_taco_stream_step', 'wrnn_taco_stream_view', 'wrnn_taco_stream_info',
                    'wrnn_taco_stream_last_error', 'wrnn_taco_stream_close', 'wrnn_taco_gta_corpus',
                    'wrnn_taco_gta_reserve', 'wrnn_taco_gta_workspace_bytes')


def epilogue_tables(n_classes: int, overlap: int, hop: int):
    """Host-only: (dec, fade_in, fade_out, tail) float64 arrays as ``wrnn_epilogue`` uses them."""
    lib = load_library()
    dec = np.empty(n_classes, np.float64)
    fin, fout = np.empty(max(overlap, 0), np.float64), np.empty(max(overlap, 0), np.float64)
    tail = np.empty(20 * hop, np.float64)
    rc = lib.wrnn_epilogue_tables(n_classes, overlap, hop, dec.ctypes.data, fin.ctypes.data if overlap else None,
                                  fout.ctypes.data if overlap else None, tail.ctypes.data)
    if rc != 0:
        raise WrnnError(rc, 'wrnn_epilogue_tables: invalid arguments')
    return dec, fin, fout, tail


class WrnnError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f'{ERR_NAMES.get(code, code)}: {msg}')
        self.code = code


class Config(C.Structure):
    _fields_ = [('rnn_dims', C.c_int32), ('fc_dims', C.c_int32), ('bits', C.c_int32), ('pad', C.c_int32),
                ('n_upsample', C.c_int32), ('upsample_factors', C.c_int32 * 4), ('feat_dims', C.c_int32),
                ('compute_dims', C.c_int32), ('res_out_dims', C.c_int32), ('res_blocks', C.c_int32),
                ('hop_length', C.c_int32), ('sample_rate', C.c_int32), ('mode', C.c_int32),
                ('device', C.c_int32)]


class TensorDesc(C.Structure):
    _fields_ = [('name', C.c_char_p), ('dtype', C.c_int32), ('ndim', C.c_int32), ('shape', C.c_int64 * 4),
                ('data', C.c_void_p)]


class SampleOpts(C.Structure):
    _fields_ = [('struct_size', C.c_uint32), ('noise_mode', C.c_int32), ('kernel', C.c_int32), ('mels_padded', C.c_int32),
                ('seed', C.c_uint64), ('noise1_dev', C.c_void_p), ('noise2_dev', C.c_void_p), ('x_forced_dev', C.c_void_p),
                ('logits_out_dev', C.c_void_p), ('x_init_dev', C.c_void_p), ('frames_dev', C.c_void_p),
                ('batch_rows', C.c_int32), ('team2_segment', C.c_int32), ('utt_seeds_dev', C.c_void_p)]


TACO_MAX_TX, TACO_MAX_PRENET = 1024, 4   # WRNN_TACO_MAX_TX, WRNN_TACO_MAX_PRENET


class TacoDims(C.Structure):
    """``wrnn_taco_dims``."""
    _fields_ = [('struct_size', C.c_uint32), ('device', C.c_int32), ('n_symbols', C.c_int32), ('num_mels', C.c_int32),
                ('outputs_per_step', C.c_int32), ('embedding_dim', C.c_int32), ('enc_conv_layers', C.c_int32), ('enc_conv_channels', C.c_int32),
                ('enc_conv_kernel', C.c_int32), ('encoder_lstm_units', C.c_int32), ('attention_dim', C.c_int32), ('attention_filters', C.c_int32),
                ('attention_kernel', C.c_int32), ('prenet_layers', C.c_int32), ('prenet_sizes', C.c_int32 * TACO_MAX_PRENET),
                ('decoder_layers', C.c_int32), ('decoder_lstm_units', C.c_int32), ('postnet_layers', C.c_int32), ('postnet_channels', C.c_int32),
                ('postnet_kernel', C.c_int32), ('zoneout', C.c_float), ('max_abs_value', C.c_float), ('lower_bound_decay', C.c_float),
                ('bn_epsilon', C.c_float)]


class TacoCall(C.Structure):
    """``wrnn_taco_call``."""
    _fields_ = [('struct_size', C.c_uint32), ('B', C.c_int32), ('Tx_max', C.c_int32), ('max_iters', C.c_int32), ('prenet_dropout', C.c_int32),
                ('steps_max', C.c_int32), ('ids_host', C.c_void_p), ('tx_host', C.c_void_p), ('seeds_host', C.c_void_p), ('gta_dev', C.c_void_p),
                ('gta_max', C.c_int32), ('gta_frames_host', C.c_void_p), ('encoder_dev', C.c_void_p), ('decoder_dev', C.c_void_p),
                ('mel_raw_dev', C.c_void_p), ('mel_dev', C.c_void_p), ('alignments_dev', C.c_void_p), ('stop_dev', C.c_void_p),
                ('max_attentions_dev', C.c_void_p), ('steps_dev', C.c_void_p), ('mel_frames_dev', C.c_void_p)]


class TacoStreamOpts(C.Structure):
    """``wrnn_taco_stream_opts``."""
    _fields_ = [('struct_size', C.c_uint32), ('B', C.c_int32), ('Tx_max', C.c_int32), ('max_iters', C.c_int32), ('prenet_dropout', C.c_int32),
                ('ids_host', C.c_void_p), ('tx_host', C.c_void_p), ('seeds_host', C.c_void_p), ('gta_dev', C.c_void_p)]


class TacoStreamOutputs(C.Structure):
    """``wrnn_taco_stream_outputs``."""
    _fields_ = [('struct_size', C.c_uint32), ('encoder_dev', C.c_void_p), ('decoder_dev', C.c_void_p), ('mel_raw_dev', C.c_void_p),
                ('mel_dev', C.c_void_p), ('alignments_dev', C.c_void_p), ('stop_dev', C.c_void_p), ('max_attentions_dev', C.c_void_p),
                ('steps_dev', C.c_void_p), ('mel_frames_dev', C.c_void_p), ('encoder_stride', C.c_int64), ('frames_stride', C.c_int64),
                ('alignments_stride', C.c_int64), ('stop_stride', C.c_int64), ('max_attentions_stride', C.c_int64)]


class TacoGtaCall(C.Structure):
    """``wrnn_taco_gta_call``."""
    _fields_ = [('struct_size', C.c_uint32), ('B', C.c_int32), ('Tx_max', C.c_int32), ('prenet_dropout', C.c_int32), ('ids_host', C.c_void_p),
                ('tx_host', C.c_void_p), ('seeds_host', C.c_void_p), ('frames_host', C.c_void_p), ('mel_off_host', C.c_void_p),
                ('out_off_host', C.c_void_p), ('mels_dev', C.c_void_p), ('mels_elems', C.c_int64), ('gta_mels_dev', C.c_void_p),
                ('out_elems', C.c_int64), ('l1_dev', C.c_void_p), ('focus_dev', C.c_void_p), ('last_attention_dev', C.c_void_p)]


LOOP_PARAM_FIELDS = ('I_w', 'I_b', 'rnn1_w_ih', 'rnn1_w_hh', 'rnn1_b_ih', 'rnn1_b_hh', 'rnn2_w_ih', 'rnn2_w_hh', 'rnn2_b_ih',
                     'rnn2_b_hh', 'fc1_w', 'fc1_b', 'fc2_w', 'fc2_b', 'fc3_w', 'fc3_b')
# wrnn_loop_params field -> state_dict key of the reference module (fatchord_version.py:115-123)
LOOP_PARAM_KEYS = ('I.weight', 'I.bias', 'rnn1.weight_ih_l0', 'rnn1.weight_hh_l0', 'rnn1.bias_ih_l0', 'rnn1.bias_hh_l0',
                   'rnn2.weight_ih_l0', 'rnn2.weight_hh_l0', 'rnn2.bias_ih_l0', 'rnn2.bias_hh_l0', 'fc1.weight', 'fc1.bias',
                   'fc2.weight', 'fc2.bias', 'fc3.weight', 'fc3.bias')


class LoopParams(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in LOOP_PARAM_FIELDS]


class Timing(C.Structure):
    _fields_ = [('prologue_ms', C.c_float), ('loop_ms', C.c_float), ('kernel', C.c_int32), ('rows', C.c_int32),
                ('steps', C.c_int64), ('launches', C.c_int32), ('reserved_', C.c_int32)]


class MelConfig(C.Structure):
    _fields_ = [('sample_rate', C.c_int32), ('n_fft', C.c_int32), ('hop_length', C.c_int32), ('win_length', C.c_int32),
                ('n_mels', C.c_int32), ('fmin', C.c_float), ('min_level_db', C.c_float), ('device', C.c_int32)]


MEL_PAD_MODES = {'reflect': 0, 'zero': 1}   # WRNN_MEL_PAD_*


class MelFeatures(C.Structure):
    """``wrnn_mel_features``; the values a fresh one holds are the default profile (``wrnn_mel_create``'s)."""
    _fields_ = [('struct_size', C.c_uint32), ('pad_mode', C.c_int32), ('magnitude_power', C.c_int32), ('fmax', C.c_float),
                ('ref_level_db', C.c_float), ('preemphasis', C.c_float), ('preemph_rescale', C.c_float), ('max_abs_value', C.c_float)]

    def __init__(self, pad_mode=0, magnitude_power=1, fmax=0.0, ref_level_db=0.0, preemphasis=0.0, preemph_rescale=0.0, max_abs_value=0.0):
        super().__init__(C.sizeof(MelFeatures), int(pad_mode), int(magnitude_power), float(fmax), float(ref_level_db), float(preemphasis),
                         float(preemph_rescale), float(max_abs_value))


GRIFFIN_PHASE_ZERO, GRIFFIN_PHASE_PHILOX, GRIFFIN_PHASE_INJECTED = 0, 1, 2   # WRNN_GRIFFIN_PHASE_*


class GriffinConfig(C.Structure):
    """``wrnn_griffin_config``."""
    _fields_ = [('struct_size', C.c_uint32), ('power', C.c_float), ('n_iter_default', C.c_int32)]

    def __init__(self, power=1.5, n_iter_default=60):
        super().__init__(C.sizeof(GriffinConfig), float(power), int(n_iter_default))


SCORE_MAX_RES, SCORE_FIELDS = 4, 12   # WRNN_SCORE_MAX_RES, WRNN_SCORE_FIELDS
# the order of the doubles in wrnn_score's summary: WRNN_SCORE_MEL_LSD_DB .. WRNN_SCORE_LOGMAG0 + 3
SCORE_FIELD_NAMES = ('mel_lsd_db', 'mcd_db', 'mr_sc', 'mr_logmag', 'sc0', 'sc1', 'sc2', 'sc3', 'logmag0', 'logmag1', 'logmag2', 'logmag3')
SCORE_DEFAULT_RESOLUTIONS = ((512, 50, 240), (1024, 120, 600), (2048, 240, 1200))   # (n_fft, hop, win)


class ScoreConfig(C.Structure):
    """``wrnn_score_config``; ``resolutions``: up to four ``(n_fft, hop, win)``."""
    _fields_ = [('struct_size', C.c_uint32), ('n_res', C.c_int32), ('n_fft', C.c_int32 * 4), ('hop', C.c_int32 * 4), ('win', C.c_int32 * 4),
                ('mag_floor', C.c_float), ('mcd_order', C.c_int32)]

    def __init__(self, resolutions=SCORE_DEFAULT_RESOLUTIONS, mag_floor=1e-7, mcd_order=13):
        res = [tuple(int(v) for v in r) for r in resolutions]
        if any(len(r) != 3 for r in res):
            raise ValueError(f'a resolution is (n_fft, hop, win), got {resolutions!r}')
        if len(res) > SCORE_MAX_RES:
            raise ValueError(f'a handle holds at most {SCORE_MAX_RES} resolutions, got {len(res)}')
        pad = [(0, 0, 0)] * (SCORE_MAX_RES - len(res))
        cols = list(zip(*(res + pad)))
        super().__init__(C.sizeof(ScoreConfig), len(res), (C.c_int32 * 4)(*cols[0]), (C.c_int32 * 4)(*cols[1]), (C.c_int32 * 4)(*cols[2]),
                         float(mag_floor), int(mcd_order))


PITCH_FIELDS = 8   # WRNN_PITCH_FIELDS
# the order of the doubles in wrnn_pitch_score's summary: WRNN_PITCH_F0_RMSE_CENTS .. WRNN_PITCH_VOICED_BOTH
PITCH_FIELD_NAMES = ('f0_rmse_cents', 'gpe', 'vde', 'ffe', 'f0_corr', 'voiced_target', 'voiced_test', 'voiced_both')
PITCH_FRAME_NAMES = ('f0_target', 'aperiodicity_target', 'f0_test', 'aperiodicity_test', 'cents')   # a row of frames_dev
PITCH_DEFAULTS = dict(sample_rate=22050, hop=275, frame_length=2048, window=1024, fmin=60.0, fmax=600.0, threshold=0.15, silence_rms=1e-4,
                      gpe_ratio=0.2)


class PitchConfig(C.Structure):
    """``wrnn_pitch_config``; a fresh one holds the defaults."""
    _fields_ = [('struct_size', C.c_uint32), ('sample_rate', C.c_int32), ('hop', C.c_int32), ('frame_length', C.c_int32), ('window', C.c_int32),
                ('device', C.c_int32), ('fmin', C.c_double), ('fmax', C.c_double), ('threshold', C.c_double), ('silence_rms', C.c_double),
                ('gpe_ratio', C.c_double)]

    def __init__(self, device=0, **settings):
        unknown = set(settings) - set(PITCH_DEFAULTS)
        if unknown:
            raise TypeError(f'unknown pitch settings {sorted(unknown)}')
        v = dict(PITCH_DEFAULTS, **settings)
        ints = [int(v[k]) for k in ('sample_rate', 'hop', 'frame_length', 'window')]
        if any(not -2 ** 31 <= i < 2 ** 31 for i in ints):
            raise ValueError(f'WRNN_ERR_INVALID: sample_rate, hop, frame_length, window = {ints} do not fit 32 bits')
        super().__init__(C.sizeof(PitchConfig), *ints, int(device), float(v['fmin']), float(v['fmax']), float(v['threshold']),
                         float(v['silence_rms']), float(v['gpe_ratio']))


ALIGN_FIELDS = 12   # WRNN_ALIGN_FIELDS
# the order of the doubles in wrnn_align_score's summary: WRNN_ALIGN_TOTAL_COST .. WRNN_ALIGN_VOICED_BOTH
ALIGN_FIELD_NAMES = ('total_cost', 'path_len', 'frames_target', 'frames_test', 'mcd_dtw_db', 'mel_lsd_dtw_db', 'f0_rmse_cents', 'gpe', 'vde', 'ffe',
                     'f0_corr', 'voiced_both')
ALIGN_COUNT_NAMES = ('path_len', 'frames_target', 'frames_test', 'voiced_both')   # the fields that are counts
ALIGN_PATH_NAMES = ('lsd', 'cents')   # the rows of per_path_dev
ALIGN_MAX_SIDE, ALIGN_MAX_CELLS = 4096, 2 ** 28   # min(Ta_max, Tb_max) and B Ta_max Tb_max of one call


class AlignConfig(C.Structure):
    """``wrnn_align_config``."""
    _fields_ = [('struct_size', C.c_uint32), ('mcd_order', C.c_int32), ('gpe_ratio', C.c_double)]

    def __init__(self, mcd_order=13, gpe_ratio=0.2):
        super().__init__(C.sizeof(AlignConfig), int(mcd_order), float(gpe_ratio))


WEIGHT_FORMATS = {'f32': 0, 'f16': 1}   # WRNN_WEIGHTS_*: the element type of the TEAMG / TEAMG_BATCH weight image
WEIGHT_FORMAT_NAMES = {v: k for k, v in WEIGHT_FORMATS.items()}
# every format of that image, WRNN_WEIGHTS_E4M3 included (code 2 is reserved): what the setters and teamg_plan_fmt validate against
TEAMG_WEIGHT_FORMATS = {**WEIGHT_FORMATS, 'e4m3': 3}
TEAMG_WEIGHT_FORMAT_NAMES = {v: k for k, v in TEAMG_WEIGHT_FORMATS.items()}
TEAMG_LAYER_NAMES = ('fc3', 'fc2', 'fc1', 'rnn2', 'rnn1', 'cond')   # WRNN_TEAMG_*: the order in which layers are given LDS residency


class TeamgLayerInfo(C.Structure):
    _fields_ = [('units', C.c_int32), ('rows_per_unit', C.c_int32), ('k', C.c_int32), ('k_padded', C.c_int32),
                ('own_first', C.c_int32 * 32), ('own_count', C.c_int32 * 32), ('rows_min', C.c_int32), ('rows_max', C.c_int32),
                ('resident_units', C.c_int32), ('reserved_', C.c_int32), ('weight_bytes', C.c_int64), ('resident_bytes_wg', C.c_int64),
                ('resident_bytes_team', C.c_int64), ('streamed_bytes_step', C.c_int64), ('lds_bytes', C.c_int64)]


class TeamgPlanInfo(C.Structure):
    _fields_ = [('layer', TeamgLayerInfo * 6), ('lds_budget_bytes', C.c_int64), ('activation_bytes', C.c_int64), ('lds_bytes', C.c_int64),
                ('streamed_bytes_step', C.c_int64), ('mail_granules', C.c_int64)]


def teamg_plan(lds_budget_bytes: int = -1, *, rnn_dims, fc_dims, bits, pad, upsample_factors, feat_dims, compute_dims, res_out_dims,
               res_blocks, hop_length, sample_rate=22050, mode='RAW', rows_per_team=None, weights=None, sparse_blocks=None) -> dict:
    """Host-only ``wrnn_teamg_plan``: how WRNN_KERNEL_TEAMG splits a model of these constructor dims over the 32 workgroups of a team and
    what it keeps in LDS with ``lds_budget_bytes`` for resident weights (< 0: the default, 160 KiB minus the activation vectors).
    ``layers``: name -> dict of the ``wrnn_teamg_layer_info`` fields (``own_first`` / ``own_count`` as lists of 32).
    ``rows_per_team``: ``wrnn_teamg_batch_plan`` instead (see :func:`teamg_batch_plan`); ``weights``: ``wrnn_teamg_plan_fmt`` instead (see
    :func:`teamg_plan_fmt`); ``sparse_blocks = (nb_a, nb_b)``: ``wrnn_teamg_sparse_plan`` instead (see :func:`teamg_sparse_plan`)."""
    cfg = Config()
    cfg.rnn_dims, cfg.fc_dims, cfg.bits, cfg.pad = rnn_dims, fc_dims, bits, pad
    cfg.n_upsample = len(upsample_factors)
    for i, s in enumerate(upsample_factors):
        cfg.upsample_factors[i] = int(s)
    cfg.feat_dims, cfg.compute_dims, cfg.res_out_dims = feat_dims, compute_dims, res_out_dims
    cfg.res_blocks, cfg.hop_length, cfg.sample_rate = res_blocks, hop_length, sample_rate
    cfg.mode = MODE_RAW if mode == 'RAW' else MODE_MOL
    info = TeamgPlanInfo()
    if sparse_blocks is not None:
        nb_a, nb_b = ([int(v) for v in nb] for nb in sparse_blocks)
        if len(nb_a) != 6 or len(nb_b) != 6:
            raise ValueError('sparse_blocks: six counts per segment, in the order of TEAMG_LAYER_NAMES')
        rows = 1 if rows_per_team is None else int(rows_per_team)
        rc = load_library().wrnn_teamg_sparse_plan(C.byref(cfg), rows, (C.c_int32 * 6)(*nb_a), (C.c_int32 * 6)(*nb_b), int(lds_budget_bytes), C.byref(info))
        what = f'wrnn_teamg_sparse_plan({rows} rows per team, blocks {nb_a} / {nb_b})'
    elif weights is not None:
        if not isinstance(weights, str) or weights not in TEAMG_WEIGHT_FORMATS:
            raise ValueError(f'weights must be one of {sorted(TEAMG_WEIGHT_FORMATS)}, not {weights!r}')
        rows = 1 if rows_per_team is None else int(rows_per_team)
        rc = load_library().wrnn_teamg_plan_fmt(C.byref(cfg), rows, TEAMG_WEIGHT_FORMATS[weights], int(lds_budget_bytes), C.byref(info))
        what = f'wrnn_teamg_plan_fmt({rows} rows per team, {weights} weights)'
    elif rows_per_team is None:
        rc, what = load_library().wrnn_teamg_plan(C.byref(cfg), int(lds_budget_bytes), C.byref(info)), 'wrnn_teamg_plan'
    else:
        rc = load_library().wrnn_teamg_batch_plan(C.byref(cfg), int(rows_per_team), int(lds_budget_bytes), C.byref(info))
        what = f'wrnn_teamg_batch_plan({rows_per_team} rows per team)'
    if rc != 0:
        raise WrnnError(rc, f'{what}: no plan for rnn_dims {rnn_dims}, fc_dims {fc_dims}, feat_dims {feat_dims}, res_out_dims {res_out_dims}, '
                            f'bits {bits}, mode {mode}')
    layers = {}
    for name, li in zip(TEAMG_LAYER_NAMES, info.layer):
        layers[name] = {f: (list(getattr(li, f)) if f.startswith('own_') else int(getattr(li, f))) for f, _ in TeamgLayerInfo._fields_ if f != 'reserved_'}
    out = {f: int(getattr(info, f)) for f, _ in TeamgPlanInfo._fields_ if f != 'layer'}
    out['layers'] = layers
    return out


def teamg_batch_plan(rows_per_team: int, lds_budget_bytes: int = -1, **dims) -> dict:
    """Host-only ``wrnn_teamg_batch_plan``: the plan of WRNN_KERNEL_TEAMG_BATCH with ``rows_per_team`` rows in lock-step (1: ``teamg_plan``'s;
    2, 4, 8: the kernel's instantiations).  Same dict as :func:`teamg_plan`; ``activation_bytes`` and ``mail_granules`` are for that many
    rows.  ``WrnnError``: WRNN_ERR_INVALID outside 1..8, WRNN_ERR_UNSUPPORTED when the rows' vectors or mailbox regions do not fit."""
    return teamg_plan(lds_budget_bytes, rows_per_team=int(rows_per_team), **dims)


# wrnn_train_last_recurrence: what the two GRU recurrences of the last training call ran
TRAIN_RAN_NAMES = {0: 'steps', 1: 'team512'}
TRAIN_PRECISIONS = {'f32': 0, 'bf16': 1}   # WRNN_TRAIN_*: the kernel the batched GEMMs of the training calls run on
TRAIN_PRECISION_NAMES = {v: k for k, v in TRAIN_PRECISIONS.items()}


def _train_precision_id(precision: str) -> int:
    if precision not in TRAIN_PRECISIONS:
        raise ValueError(f'train precision must be one of {sorted(TRAIN_PRECISIONS)}, not {precision!r}')
    return TRAIN_PRECISIONS[precision]


def check_train_gemm_args(precision: str, ta: bool, tb: bool, lda: int, ldb: int, ldc: int, M: int, N: int, K: int, bias_ptr: int, relu: bool,
                          slices: int) -> int:
    """The argument checks of :meth:`NativeVocoder.debug_train_gemm` that need no device (``ValueError``); returns the precision id."""
    prec = _train_precision_id(precision)
    if M < 1 or N < 1 or K < 0:
        raise ValueError(f'debug_train_gemm: bad shape M={M}, N={N}, K={K}')
    if not 0 <= slices <= 64:
        raise ValueError(f'debug_train_gemm: slices must be 0 (the wrapper chooses), 1 (no split) or 2..64, not {slices}')
    if lda < (M if ta else max(K, 1)) or ldb < (max(K, 1) if tb else N) or ldc < N:
        raise ValueError(f'debug_train_gemm: a leading dimension is shorter than its row (lda={lda}, ldb={ldb}, ldc={ldc})')
    if slices != 1 and (bias_ptr or relu):
        raise ValueError('debug_train_gemm: a split product takes no bias and no relu')
    return prec


def train_teamg_plan(rnn_dims: int, rows: int) -> dict:
    """Host-only ``wrnn_train_teamg_plan``: the layout persistent team recurrences of training would have for ``rnn_dims`` at ``rows`` rows
    per team.  Returns ``dict(status, units_per_wg, lds_fwd, lds_bwd, mail_granules)``; ``status`` is ``WRNN_OK`` (0) where a workgroup's
    slice of W_hh fits LDS, ``WRNN_ERR_UNSUPPORTED`` (-7) where it exceeds 160 KiB (the figures are still filled in) and
    ``WRNN_ERR_INVALID`` (-1) for an rnn_dims that is no multiple of 16 or rows outside 1..8 (figures 0).  Never raises."""
    u, lf, lb, mg = C.c_int32(0), C.c_int64(0), C.c_int64(0), C.c_int64(0)
    rc = load_library().wrnn_train_teamg_plan(int(rnn_dims), int(rows), C.byref(u), C.byref(lf), C.byref(lb), C.byref(mg))
    return dict(status=int(rc), units_per_wg=int(u.value), lds_fwd=int(lf.value), lds_bwd=int(lb.value), mail_granules=int(mg.value))


def teamg_plan_fmt(rows_per_team: int, weights: str, lds_budget_bytes: int = -1, **dims) -> dict:
    """Host-only ``wrnn_teamg_plan_fmt``: :func:`teamg_batch_plan` for the weight image format ``weights`` (a key of ``TEAMG_WEIGHT_FORMATS``).  Same dict;
    with 'f16' every byte figure counts 2-byte weights, with 'e4m3' 1-byte weights, and more units fit the same LDS budget; ownership and
    ``k_padded`` are unchanged."""
    return teamg_plan(lds_budget_bytes, rows_per_team=int(rows_per_team), weights=weights, **dims)


def teamg_sparse_plan(rows_per_team: int, nb_a, nb_b, lds_budget_bytes: int = -1, **dims) -> dict:
    """Host-only ``wrnn_teamg_sparse_plan``: :func:`teamg_batch_plan` for the block-sparse fp32 image whose rows hold ``nb_a[l]`` blocks of
    segment A and ``nb_b[l]`` of segment B in layer ``l`` (order of ``TEAMG_LAYER_NAMES``).  Same dict; the byte figures count the image's
    rows, 16-bit block indices included; ``k`` and ``k_padded`` stay the dense row's.  ``WrnnError`` (WRNN_ERR_INVALID) for a count above
    the dense row's."""
    return teamg_plan(lds_budget_bytes, rows_per_team=int(rows_per_team), sparse_blocks=(nb_a, nb_b), **dims)


_lib: Optional[C.CDLL] = None


def _preload_hip_runtime() -> str:
    """One HIP runtime per process.  libwavernn_amd.so is linked with -no-hip-rt (no DT_NEEDED on a
    specific libamdhip64): PyTorch-ROCm wheels bundle their own runtime, and mixing it with /opt/rocm's in
    one process gives two HSA instances that do not share streams or events.  So: use torch's copy when
    torch is importable (device pointers, streams and events then belong to the same runtime), else ROCm's."""
    cands = []
    try:
        import torch
        cands.append(os.path.join(os.path.dirname(torch.__file__), 'lib', 'libamdhip64.so'))
    except Exception:  # pragma: no cover - torch is a hard dependency of the host side
        pass
    cands += ['/opt/rocm/lib/libamdhip64.so', 'libamdhip64.so']
    for c in cands:
        try:
            C.CDLL(c, mode=C.RTLD_GLOBAL)
            return c
        except OSError:
            continue
    raise RuntimeError('no HIP runtime (libamdhip64.so) found')


def load_library() -> C.CDLL:
    global _lib
    if _lib is not None:
        return _lib
    _preload_hip_runtime()
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            f'{LIB_PATH} is missing: build it with `python -c "import __graft_entry__ as g; g.build()"` '
            '(hipcc --offload-arch=gfx950).  There is no fallback path.')
    lib = C.CDLL(LIB_PATH)
    lib.wrnn_abi_version.argtypes = []
    lib.wrnn_abi_version.restype = C.c_int32
    got = int(lib.wrnn_abi_version())
    if got != ABI_VERSION:   # the .so is a git-ignored build artefact: a stale one would read the structs at shifted offsets
        raise RuntimeError(f'{LIB_PATH} implements ABI {got}, this binding needs ABI {ABI_VERSION}: rebuild it '
                           '(`python -c "import __graft_entry__ as g; g.build()"`)')
    # entry points have joined ABI 9 without a new number (the mel front end, the dataset kernels, the resampler, the wav conditioning): a
    # build from before them reports 9 too
    missing = [s for s in EXPORTED_SYMBOLS if not hasattr(lib, s)]
    if missing:
        raise RuntimeError(f'{LIB_PATH} implements ABI {got} without {", ".join(missing)}: it was built from older sources, rebuild it '
                           '(`python -c "import __graft_entry__ as g; g.build()"`)')
    vp = C.c_void_p
    lib.wrnn_create.argtypes = [C.POINTER(Config), C.POINTER(vp)]
    lib.wrnn_create.restype = C.c_int
    lib.wrnn_load_weights.argtypes = [vp, C.POINTER(TensorDesc), C.c_int32]
    lib.wrnn_load_weights.restype = C.c_int
    lib.wrnn_conditioning.argtypes = [vp, vp, C.c_int32, C.c_int32, C.c_int32, vp, vp, vp]
    lib.wrnn_conditioning.restype = C.c_int
    lib.wrnn_plan.argtypes = [vp, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_int32),
                              C.POINTER(C.c_int64)]
    lib.wrnn_plan.restype = C.c_int
    lib.wrnn_generate.argtypes = [vp, vp, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                  C.POINTER(SampleOpts), vp, vp, vp]
    lib.wrnn_generate.restype = C.c_int
    lib.wrnn_epilogue.argtypes = [vp, vp, vp, C.c_int32, C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int64,
                                  vp, vp]
    lib.wrnn_epilogue.restype = C.c_int
    lib.wrnn_epilogue_rows.argtypes = [vp, vp, vp, C.c_int32, C.c_int64, C.c_int32, C.c_int64, vp, vp, C.c_int64, vp]
    lib.wrnn_epilogue_rows.restype = C.c_int
    lib.wrnn_phase_profile.argtypes = [vp, C.c_int32]
    lib.wrnn_phase_profile.restype = C.c_int
    lib.wrnn_phase_cycles.argtypes = [vp, C.POINTER(C.c_double)]
    lib.wrnn_phase_cycles.restype = C.c_int
    lib.wrnn_train_step.argtypes = [vp, C.POINTER(LoopParams), C.POINTER(LoopParams), vp, vp, vp, vp, C.c_int32, C.c_int64, vp, vp,
                                    vp, vp, vp]
    lib.wrnn_train_step.restype = C.c_int
    lib.wrnn_train_forward.argtypes = [vp, C.POINTER(LoopParams), vp, vp, vp, C.c_int32, C.c_int64, vp, vp]
    lib.wrnn_train_forward.restype = C.c_int
    lib.wrnn_train_backward.argtypes = [vp, C.POINTER(LoopParams), C.POINTER(LoopParams), vp, vp, vp, vp, C.c_int32, C.c_int64, vp, vp, vp]
    lib.wrnn_train_backward.restype = C.c_int
    lib.wrnn_sync_status.argtypes = [vp, vp]
    lib.wrnn_sync_status.restype = C.c_int
    lib.wrnn_train_force_step_kernels.argtypes = [vp, C.c_int32]
    lib.wrnn_train_force_step_kernels.restype = C.c_int
    lib.wrnn_epilogue_tables.argtypes = [C.c_int32, C.c_int32, C.c_int32, vp, vp, vp, vp]
    lib.wrnn_epilogue_tables.restype = C.c_int
    lib.wrnn_loss.argtypes = [vp, vp, vp, C.c_int64, vp, vp]
    lib.wrnn_loss.restype = C.c_int
    lib.wrnn_last_timing.argtypes = [vp, C.POINTER(Timing)]
    lib.wrnn_last_timing.restype = C.c_int
    lib.wrnn_n_classes.argtypes = [vp]
    lib.wrnn_n_classes.restype = C.c_int32
    lib.wrnn_loop_weight_bytes.argtypes = [vp]
    lib.wrnn_loop_weight_bytes.restype = C.c_int64
    lib.wrnn_last_error.argtypes = [vp]
    lib.wrnn_last_error.restype = C.c_char_p
    lib.wrnn_destroy.argtypes = [vp]
    lib.wrnn_destroy.restype = None
    lib.wrnn_team_info.argtypes = [vp, C.POINTER(C.c_int32), C.POINTER(C.c_char_p)]
    lib.wrnn_team_info.restype = C.c_int32
    lib.wrnn_debug_force_no_teams.argtypes = [vp, C.c_int32]
    lib.wrnn_debug_force_no_teams.restype = C.c_int
    lib.wrnn_teamg_plan.argtypes = [C.POINTER(Config), C.c_int64, C.POINTER(TeamgPlanInfo)]
    lib.wrnn_teamg_plan.restype = C.c_int
    lib.wrnn_debug_teamg_lds_budget.argtypes = [vp, C.c_int64]
    lib.wrnn_debug_teamg_lds_budget.restype = C.c_int
    lib.wrnn_teamg_batch_plan.argtypes = [C.POINTER(Config), C.c_int32, C.c_int64, C.POINTER(TeamgPlanInfo)]
    lib.wrnn_teamg_batch_plan.restype = C.c_int
    lib.wrnn_teamg_plan_fmt.argtypes = [C.POINTER(Config), C.c_int32, C.c_int32, C.c_int64, C.POINTER(TeamgPlanInfo)]
    lib.wrnn_teamg_plan_fmt.restype = C.c_int
    lib.wrnn_teamg_set_weight_format.argtypes = [vp, C.c_int32]
    lib.wrnn_teamg_set_weight_format.restype = C.c_int
    lib.wrnn_teamg_weight_format.argtypes = [vp]
    lib.wrnn_teamg_weight_format.restype = C.c_int32
    lib.wrnn_teamg_weight_scales.argtypes = [vp, C.POINTER(C.c_float)]
    lib.wrnn_teamg_weight_scales.restype = C.c_int
    lib.wrnn_teamg_set_sparse.argtypes = [vp, C.c_int32]
    lib.wrnn_teamg_set_sparse.restype = C.c_int
    lib.wrnn_teamg_sparse.argtypes = [vp]
    lib.wrnn_teamg_sparse.restype = C.c_int32
    lib.wrnn_teamg_sparse_plan.argtypes = [C.POINTER(Config), C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.c_int64, C.POINTER(TeamgPlanInfo)]
    lib.wrnn_teamg_sparse_plan.restype = C.c_int
    lib.wrnn_teamg_sparse_info.argtypes = [vp, C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(TeamgPlanInfo)]
    lib.wrnn_teamg_sparse_info.restype = C.c_int
    lib.wrnn_train_last_recurrence.argtypes = [vp, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
    lib.wrnn_train_last_recurrence.restype = C.c_int
    lib.wrnn_train_teamg_plan.argtypes = [C.c_int32, C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
    lib.wrnn_train_teamg_plan.restype = C.c_int
    lib.wrnn_train_set_precision.argtypes = [vp, C.c_int32]
    lib.wrnn_train_set_precision.restype = C.c_int
    lib.wrnn_train_precision.argtypes = [vp, C.POINTER(C.c_int32)]
    lib.wrnn_train_precision.restype = C.c_int
    lib.wrnn_train_last_gemms.argtypes = [vp, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
    lib.wrnn_train_last_gemms.restype = C.c_int
    lib.wrnn_debug_train_gemm.argtypes = [vp, C.c_int32, C.c_int32, C.c_int32, vp, C.c_int64, vp, C.c_int64, vp, C.c_int64, C.c_int32, C.c_int32,
                                          C.c_int32, C.c_int32, vp, C.c_int32, C.c_int32, vp]
    lib.wrnn_debug_train_gemm.restype = C.c_int
    lib.wrnn_last_batch_rows.argtypes = [vp]
    lib.wrnn_last_batch_rows.restype = C.c_int32
    lib.wrnn_stream_open.argtypes = [vp, C.c_int32, C.POINTER(SampleOpts), C.POINTER(vp)]
    lib.wrnn_stream_open.restype = C.c_int
    lib.wrnn_stream_push.argtypes = [vp, vp, C.c_int32, C.c_int32, vp, vp, C.c_int64, C.POINTER(C.c_int64), vp]
    lib.wrnn_stream_push.restype = C.c_int
    lib.wrnn_stream_sync.argtypes = [vp, vp]
    lib.wrnn_stream_sync.restype = C.c_int
    lib.wrnn_stream_info.argtypes = [vp, C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
    lib.wrnn_stream_info.restype = C.c_int
    lib.wrnn_stream_ready_steps.argtypes = [C.c_int64, C.c_int32, C.c_int32, C.c_int32]
    lib.wrnn_stream_ready_steps.restype = C.c_int64
    lib.wrnn_stream_close.argtypes = [vp]
    lib.wrnn_stream_close.restype = None
    lib.wrnn_plan_folded.argtypes = [vp, C.c_int32, C.c_int32, C.c_int32, C.c_int32, vp, C.POINTER(C.c_int64)]
    lib.wrnn_plan_folded.restype = C.c_int
    lib.wrnn_generate_folded.argtypes = [vp, vp, C.c_int32, C.c_int32, vp, C.c_int32, C.c_int32, C.c_int32, C.POINTER(SampleOpts), vp, vp, vp]
    lib.wrnn_generate_folded.restype = C.c_int
    lib.wrnn_epilogue_folded.argtypes = [vp, vp, vp, C.c_int32, C.c_int32, C.c_int64, C.c_int32, C.c_int32, C.c_int32, vp, vp, C.c_int64, vp]
    lib.wrnn_epilogue_folded.restype = C.c_int
    lib.wrnn_mel_create.argtypes = [C.POINTER(MelConfig), C.POINTER(vp)]
    lib.wrnn_mel_create.restype = C.c_int
    lib.wrnn_mel_create_features.argtypes = [C.POINTER(MelConfig), C.POINTER(MelFeatures), C.POINTER(vp)]
    lib.wrnn_mel_create_features.restype = C.c_int
    lib.wrnn_mel_frames.argtypes = [vp, C.c_int64]
    lib.wrnn_mel_frames.restype = C.c_int64
    lib.wrnn_melspectrogram.argtypes = [vp, vp, C.c_int64, vp, C.c_int32, C.c_int32, vp, vp]
    lib.wrnn_melspectrogram.restype = C.c_int
    lib.wrnn_mel_tables.argtypes = [vp, vp, vp, vp, vp, C.POINTER(C.c_int32)]
    lib.wrnn_mel_tables.restype = C.c_int
    lib.wrnn_mel_last_error.argtypes = [vp]
    lib.wrnn_mel_last_error.restype = C.c_char_p
    lib.wrnn_mel_destroy.argtypes = [vp]
    lib.wrnn_mel_destroy.restype = None
    lib.wrnn_resample_create.argtypes = [C.c_int32, C.c_int32, C.c_int32, C.POINTER(vp)]
    lib.wrnn_resample_create.restype = C.c_int
    lib.wrnn_resample_out_len.argtypes = [vp, C.c_int64]
    lib.wrnn_resample_out_len.restype = C.c_int64
    lib.wrnn_resample_bank.argtypes = [vp, vp, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
    lib.wrnn_resample_bank.restype = C.c_int
    lib.wrnn_resample.argtypes = [vp, vp, C.c_int64, vp, C.c_int32, C.c_int64, vp, vp]
    lib.wrnn_resample.restype = C.c_int
    lib.wrnn_resample_last_error.argtypes = [vp]
    lib.wrnn_resample_last_error.restype = C.c_char_p
    lib.wrnn_resample_destroy.argtypes = [vp]
    lib.wrnn_resample_destroy.restype = None
    lib.wrnn_condition_frames.argtypes = [C.c_int64, C.c_int32, C.c_int32]
    lib.wrnn_condition_frames.restype = C.c_int64
    lib.wrnn_condition.argtypes = [vp, C.c_int64, vp, C.c_int32, C.c_int32, C.c_double, C.c_int32, C.c_int32, C.c_float, vp, C.c_int32, vp,
                                   C.c_int64, vp, vp, vp, vp]
    lib.wrnn_condition.restype = C.c_int
    lib.wrnn_griffin_create.argtypes = [C.POINTER(MelConfig), C.POINTER(MelFeatures), C.POINTER(GriffinConfig), C.POINTER(vp)]
    lib.wrnn_griffin_create.restype = C.c_int
    lib.wrnn_griffin_samples.argtypes = [vp, C.c_int64]
    lib.wrnn_griffin_samples.restype = C.c_int64
    lib.wrnn_griffin_tables.argtypes = [vp, vp, vp, C.c_int32, vp]
    lib.wrnn_griffin_tables.restype = C.c_int
    lib.wrnn_griffin_lim.argtypes = [vp, vp, vp, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_uint64, vp, vp, C.c_int64, vp, vp]
    lib.wrnn_griffin_lim.restype = C.c_int
    lib.wrnn_deemphasis.argtypes = [vp, C.c_int64, vp, C.c_int32, C.c_double, vp, vp]
    lib.wrnn_deemphasis.restype = C.c_int
    lib.wrnn_griffin_last_error.argtypes = [vp]
    lib.wrnn_griffin_last_error.restype = C.c_char_p
    lib.wrnn_griffin_destroy.argtypes = [vp]
    lib.wrnn_griffin_destroy.restype = None
    lib.wrnn_score_create.argtypes = [C.POINTER(MelConfig), C.POINTER(MelFeatures), C.POINTER(ScoreConfig), C.POINTER(vp)]
    lib.wrnn_score_create.restype = C.c_int
    lib.wrnn_score_frames.argtypes = [vp, C.c_int32, C.c_int64]
    lib.wrnn_score_frames.restype = C.c_int64
    lib.wrnn_score.argtypes = [vp, vp, vp, C.c_int64, vp, C.c_int32, vp, vp, C.c_int64, vp]
    lib.wrnn_score.restype = C.c_int
    lib.wrnn_score_tables.argtypes = [vp, C.c_int32, vp, vp, vp]
    lib.wrnn_score_tables.restype = C.c_int
    lib.wrnn_score_last_error.argtypes = [vp]
    lib.wrnn_score_last_error.restype = C.c_char_p
    lib.wrnn_score_destroy.argtypes = [vp]
    lib.wrnn_score_destroy.restype = None
    lib.wrnn_pitch_create.argtypes = [C.POINTER(PitchConfig), C.POINTER(vp)]
    lib.wrnn_pitch_create.restype = C.c_int
    lib.wrnn_pitch_frames.argtypes = [vp, C.c_int64]
    lib.wrnn_pitch_frames.restype = C.c_int64
    lib.wrnn_pitch_lags.argtypes = [vp, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
    lib.wrnn_pitch_lags.restype = C.c_int
    lib.wrnn_pitch_track.argtypes = [vp, vp, C.c_int64, vp, C.c_int32, vp, vp, C.c_int64, vp]
    lib.wrnn_pitch_track.restype = C.c_int
    lib.wrnn_pitch_score.argtypes = [vp, vp, vp, C.c_int64, vp, C.c_int32, vp, vp, C.c_int64, vp]
    lib.wrnn_pitch_score.restype = C.c_int
    lib.wrnn_pitch_last_error.argtypes = [vp]
    lib.wrnn_pitch_last_error.restype = C.c_char_p
    lib.wrnn_pitch_destroy.argtypes = [vp]
    lib.wrnn_pitch_destroy.restype = None
    lib.wrnn_align_create.argtypes = [C.POINTER(MelConfig), C.POINTER(MelFeatures), C.POINTER(AlignConfig), C.POINTER(vp)]
    lib.wrnn_align_create.restype = C.c_int
    lib.wrnn_align_frames.argtypes = [vp, C.c_int64]
    lib.wrnn_align_frames.restype = C.c_int64
    lib.wrnn_align_workspace_bytes.argtypes = [vp, C.c_int32, C.c_int64, C.c_int64]
    lib.wrnn_align_workspace_bytes.restype = C.c_int64
    lib.wrnn_align_cost.argtypes = [vp, vp, C.c_int64, vp, vp, C.c_int64, vp, C.c_int32, vp, vp]
    lib.wrnn_align_cost.restype = C.c_int
    lib.wrnn_align_path.argtypes = [vp, vp, C.c_int32, C.c_int32, C.c_int32, vp, vp, vp, vp, vp, vp]
    lib.wrnn_align_path.restype = C.c_int
    lib.wrnn_align_score.argtypes = [vp, vp, C.c_int64, vp, vp, C.c_int64, vp, C.c_int32, vp, vp, C.c_int64, vp, vp, vp, vp, vp]
    lib.wrnn_align_score.restype = C.c_int
    lib.wrnn_align_last_error.argtypes = [vp]
    lib.wrnn_align_last_error.restype = C.c_char_p
    lib.wrnn_align_destroy.argtypes = [vp]
    lib.wrnn_align_destroy.restype = None
    lib.wrnn_taco_create.argtypes = [C.POINTER(TacoDims), C.POINTER(vp)]
    lib.wrnn_taco_create.restype = C.c_int
    lib.wrnn_taco_tensor_count.argtypes = [vp]
    lib.wrnn_taco_tensor_count.restype = C.c_int
    lib.wrnn_taco_tensor_name.argtypes = [vp, C.c_int]
    lib.wrnn_taco_tensor_name.restype = C.c_char_p
    lib.wrnn_taco_tensor_shape.argtypes = [vp, C.c_int, C.POINTER(C.c_int64)]
    lib.wrnn_taco_tensor_shape.restype = C.c_int
    lib.wrnn_taco_load_tensor.argtypes = [vp, C.c_char_p, vp, C.c_int, C.POINTER(C.c_int64)]
    lib.wrnn_taco_load_tensor.restype = C.c_int
    lib.wrnn_taco_synthesize.argtypes = [vp, C.POINTER(TacoCall), vp]
    lib.wrnn_taco_synthesize.restype = C.c_int
    lib.wrnn_taco_last_error.argtypes = [vp]
    lib.wrnn_taco_last_error.restype = C.c_char_p
    lib.wrnn_taco_destroy.argtypes = [vp]
    lib.wrnn_taco_destroy.restype = None
    i32p = C.POINTER(C.c_int32)
    lib.wrnn_taco_stream_halo.argtypes = [C.POINTER(TacoDims)]
    lib.wrnn_taco_stream_halo.restype = C.c_int
    lib.wrnn_taco_stream_open.argtypes = [vp, C.POINTER(TacoStreamOpts), vp, C.POINTER(vp)]
    lib.wrnn_taco_stream_open.restype = C.c_int
    lib.wrnn_taco_stream_step.argtypes = [vp, C.c_int32, vp, i32p, i32p, i32p]
    lib.wrnn_taco_stream_step.restype = C.c_int
    lib.wrnn_taco_stream_view.argtypes = [vp, C.POINTER(TacoStreamOutputs)]
    lib.wrnn_taco_stream_view.restype = C.c_int
    lib.wrnn_taco_stream_info.argtypes = [vp, i32p, i32p, i32p, i32p, C.POINTER(C.c_int64)]
    lib.wrnn_taco_stream_info.restype = C.c_int
    lib.wrnn_taco_stream_last_error.argtypes = [vp]
    lib.wrnn_taco_stream_last_error.restype = C.c_char_p
    lib.wrnn_taco_stream_close.argtypes = [vp]
    lib.wrnn_taco_stream_close.restype = None
    lib.wrnn_taco_gta_corpus.argtypes = [vp, C.POINTER(TacoGtaCall), vp]
    lib.wrnn_taco_gta_corpus.restype = C.c_int
    lib.wrnn_taco_gta_reserve.argtypes = [vp, C.c_int32, C.c_int32, C.c_int32, vp]
    lib.wrnn_taco_gta_reserve.restype = C.c_int
    lib.wrnn_taco_gta_workspace_bytes.argtypes = [vp]
    lib.wrnn_taco_gta_workspace_bytes.restype = C.c_int64
    lib.wrnn_quantise.argtypes = [vp, C.c_int64, C.c_int32, C.c_int32, vp, vp, vp]
    lib.wrnn_quantise.restype = C.c_int
    lib.wrnn_collate_windows.argtypes = [vp, vp, vp, vp, vp, vp, vp, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                         vp, vp, vp, vp]
    lib.wrnn_collate_windows.restype = C.c_int
    lib.wrnn_dm_create.argtypes = [C.c_int32, C.c_int32, C.c_int32, C.POINTER(vp)]
    lib.wrnn_dm_create.restype = C.c_int
    lib.wrnn_dm_load_weights.argtypes = [vp, C.POINTER(TensorDesc), C.c_int32]
    lib.wrnn_dm_load_weights.restype = C.c_int
    lib.wrnn_dm_generate.argtypes = [vp, C.c_int64, C.c_int32, C.c_uint64, vp, vp, vp, vp]
    lib.wrnn_dm_generate.restype = C.c_int
    lib.wrnn_dm_set_kernel.argtypes = [vp, C.c_int32]
    lib.wrnn_dm_set_kernel.restype = C.c_int
    lib.wrnn_dm_sync_status.argtypes = [vp, vp]
    lib.wrnn_dm_sync_status.restype = C.c_int
    lib.wrnn_dm_last_error.argtypes = [vp]
    lib.wrnn_dm_last_error.restype = C.c_char_p
    lib.wrnn_dm_destroy.argtypes = [vp]
    lib.wrnn_dm_destroy.restype = None
    _lib = lib
    return lib


class NativeVocoder:
    """Thin owner of one ``wrnn_handle`` (one per device)."""

    def __init__(self, *, rnn_dims, fc_dims, bits, pad, upsample_factors, feat_dims, compute_dims, res_out_dims,
                 res_blocks, hop_length, sample_rate, mode, device: int):
        self.lib = load_library()
        cfg = Config()
        cfg.rnn_dims, cfg.fc_dims, cfg.bits, cfg.pad = rnn_dims, fc_dims, bits, pad
        cfg.n_upsample = len(upsample_factors)
        for i, s in enumerate(upsample_factors):
            cfg.upsample_factors[i] = int(s)
        cfg.feat_dims, cfg.compute_dims, cfg.res_out_dims = feat_dims, compute_dims, res_out_dims
        cfg.res_blocks, cfg.hop_length, cfg.sample_rate = res_blocks, hop_length, sample_rate
        if mode not in ('RAW', 'MOL'):
            raise RuntimeError("Unknown model mode value - ", mode)
        cfg.mode = MODE_RAW if mode == 'RAW' else MODE_MOL
        cfg.device = int(device)
        self.device = int(device)
        self.hop = int(hop_length)
        self._dims = dict(rnn_dims=rnn_dims, fc_dims=fc_dims, bits=bits, pad=pad, upsample_factors=tuple(upsample_factors), feat_dims=feat_dims,
                          compute_dims=compute_dims, res_out_dims=res_out_dims, res_blocks=res_blocks, hop_length=hop_length,
                          sample_rate=sample_rate, mode=mode)
        self._h = C.c_void_p()
        rc = self.lib.wrnn_create(C.byref(cfg), C.byref(self._h))
        if rc != 0:
            msg = self.lib.wrnn_last_error(self._h).decode() if self._h else 'wrnn_create failed'
            if self._h:
                self.lib.wrnn_destroy(self._h)
                self._h = C.c_void_p()
            raise WrnnError(rc, msg)
        self.n_classes = int(self.lib.wrnn_n_classes(self._h))

    def _check(self, rc: int):
        if rc != 0:
            raise WrnnError(rc, self.lib.wrnn_last_error(self._h).decode())

    def close(self):
        if getattr(self, '_h', None):
            self.lib.wrnn_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def load_weights(self, state_dict: Dict[str, np.ndarray]):
        """state_dict: name -> contiguous numpy array (float32 / int64), reference key names.  Every parameter the
        path reads must be present with the reference's shape (WrnnError otherwise); other keys are ignored."""
        keep, descs = [], []
        for name, arr in state_dict.items():
            arr = np.ascontiguousarray(arr)
            if arr.dtype == np.float32:
                dt = DTYPE_F32
            elif arr.dtype == np.int64:
                dt = DTYPE_I64
            else:
                arr = arr.astype(np.float32)
                dt = DTYPE_F32
            if arr.ndim > 4:
                continue
            d = TensorDesc()
            d.name = name.encode()
            d.dtype, d.ndim = dt, arr.ndim
            for i, s in enumerate(arr.shape):
                d.shape[i] = s
            d.data = arr.ctypes.data
            keep.append(arr)
            descs.append(d)
        arr_t = (TensorDesc * len(descs))(*descs)
        self._check(self.lib.wrnn_load_weights(self._h, arr_t, len(descs)))
        self.loop_weight_bytes = int(self.lib.wrnn_loop_weight_bytes(self._h))

    def plan(self, B: int, T: int, batched: bool, target: int, overlap: int) -> Tuple[int, int]:
        rows, steps = C.c_int32(), C.c_int64()
        self._check(self.lib.wrnn_plan(self._h, B, T, int(bool(batched)), int(target), int(overlap),
                                       C.byref(rows), C.byref(steps)))
        return rows.value, steps.value

    def conditioning(self, mels_ptr: int, B: int, T: int, up_ptr: int, aux_ptr: int, stream: int, mels_padded: bool = False):
        self._check(self.lib.wrnn_conditioning(self._h, mels_ptr, B, T, int(bool(mels_padded)), up_ptr or None, aux_ptr or None,
                                               stream or None))

    def generate(self, mels_ptr: int, B: int, T: int, batched: bool, target: int, overlap: int, *,
                 labels_ptr: int, samples_ptr: int, stream: int, noise_mode: int = NOISE_PHILOX, seed: int = 0,
                 noise1_ptr: int = 0, noise2_ptr: int = 0, x_forced_ptr: int = 0, logits_ptr: int = 0,
                 kernel: int = KERNEL_AUTO, x_init_ptr: int = 0, mels_padded: bool = False, frames_ptr: int = 0,
                 batch_rows: int = 0, team2_segment: int = 0, utt_seeds_ptr: int = 0):
        o = SampleOpts()
        o.struct_size = C.sizeof(SampleOpts)
        o.frames_dev = frames_ptr or None
        o.utt_seeds_dev = utt_seeds_ptr or None   # B device uint64: per-utterance Philox keys (unbatched calls)
        o.batch_rows, o.team2_segment = int(batch_rows), int(team2_segment)
        o.noise_mode, o.kernel, o.seed = noise_mode, kernel, seed & 0xFFFFFFFFFFFFFFFF
        o.noise1_dev, o.noise2_dev = noise1_ptr or None, noise2_ptr or None
        o.x_forced_dev, o.logits_out_dev = x_forced_ptr or None, logits_ptr or None
        o.x_init_dev = x_init_ptr or None
        o.mels_padded = int(bool(mels_padded))
        self._check(self.lib.wrnn_generate(self._h, mels_ptr, B, T, int(bool(batched)), int(target), int(overlap),
                                           C.byref(o), labels_ptr or None, samples_ptr, stream or None))

    def generate_folded(self, mels_ptr: int, B: int, T: int, frames_ptr: int, rows_total: int, target: int, overlap: int, *,
                        labels_ptr: int, samples_ptr: int, stream: int, noise_mode: int = NOISE_PHILOX, seed: int = 0,
                        noise1_ptr: int = 0, noise2_ptr: int = 0, kernel: int = KERNEL_AUTO, batch_rows: int = 0, team2_segment: int = 0,
                        utt_seeds_ptr: int = 0):
        """``wrnn_generate_folded``: the folds of all B utterances as the rows of one call (rows_total from :func:`plan_folded`)."""
        o = SampleOpts()
        o.struct_size = C.sizeof(SampleOpts)
        o.batch_rows, o.team2_segment = int(batch_rows), int(team2_segment)
        o.noise_mode, o.kernel, o.seed = noise_mode, kernel, seed & 0xFFFFFFFFFFFFFFFF
        o.noise1_dev, o.noise2_dev = noise1_ptr or None, noise2_ptr or None
        o.utt_seeds_dev = utt_seeds_ptr or None
        self._check(self.lib.wrnn_generate_folded(self._h, mels_ptr, B, T, frames_ptr or None, int(rows_total), int(target), int(overlap),
                                                  C.byref(o), labels_ptr or None, samples_ptr, stream or None))

    def epilogue_folded(self, samples_ptr: int, labels_ptr: int, B: int, rows_total: int, steps: int, target: int, overlap: int,
                        mu_law: bool, frames_ptr: int, out_ptr: int, out_stride: int, stream: int):
        """Every utterance of the last ``generate_folded`` call crossfaded, unfolded, trimmed and faded out, one launch."""
        self._check(self.lib.wrnn_epilogue_folded(self._h, samples_ptr, labels_ptr or None, int(B), int(rows_total), int(steps), int(target),
                                                  int(overlap), int(bool(mu_law)), frames_ptr or None, out_ptr, int(out_stride), stream or None))

    def epilogue(self, samples_ptr: int, labels_ptr: int, rows: int, steps: int, batched: bool, target: int,
                 overlap: int, mu_law: bool, wave_len: int, out_ptr: int, stream: int):
        self._check(self.lib.wrnn_epilogue(self._h, samples_ptr, labels_ptr or None, rows, steps, int(bool(batched)),
                                           int(target), int(overlap), int(bool(mu_law)), int(wave_len), out_ptr,
                                           stream or None))

    def epilogue_rows(self, samples_ptr: int, labels_ptr: int, rows: int, steps: int, mu_law: bool, wave_len: int,
                      frames_ptr: int, out_ptr: int, out_stride: int, stream: int):
        """Every row finished as an independent unbatched utterance, one launch (``wrnn_epilogue_rows``)."""
        self._check(self.lib.wrnn_epilogue_rows(self._h, samples_ptr, labels_ptr or None, rows, steps, int(bool(mu_law)),
                                                int(wave_len), frames_ptr or None, out_ptr, int(out_stride), stream or None))

    def phase_profile(self, enable: bool = True):
        """Developer instrumentation: the following TEAM2 / BATCH calls run the instrumented loop kernel."""
        self._check(self.lib.wrnn_phase_profile(self._h, int(bool(enable))))

    def phase_cycles(self) -> np.ndarray:
        """(8 waves, 32 markers) cycles per step of workgroup 0 of team 0 for the last instrumented call."""
        out = np.zeros(8 * 32, np.float64)
        self._check(self.lib.wrnn_phase_cycles(self._h, out.ctypes.data_as(C.POINTER(C.c_double))))
        return out.reshape(8, 32)

    def train_step(self, w_ptrs, g_ptrs, x_ptr: int, mels_up_ptr: int, aux_ptr: int, y_ptr: int, B: int, L: int, loss_ptr: int,
                   logits_ptr: int, d_mels_up_ptr: int, d_aux_ptr: int, stream: int):
        """``wrnn_train_step``: w_ptrs / g_ptrs = sequences of 16 device pointers in ``LOOP_PARAM_FIELDS`` order (g_ptrs may be
        None: forward + loss only)."""
        w = LoopParams(*[int(p) for p in w_ptrs])
        g = LoopParams(*[int(p) for p in g_ptrs]) if g_ptrs is not None else None
        self._check(self.lib.wrnn_train_step(self._h, C.byref(w), C.byref(g) if g is not None else None, x_ptr, mels_up_ptr, aux_ptr,
                                             y_ptr or None, int(B), int(L), loss_ptr or None, logits_ptr or None,
                                             d_mels_up_ptr or None, d_aux_ptr or None, stream or None))

    def train_forward(self, w_ptrs, x_ptr: int, mels_up_ptr: int, aux_ptr: int, B: int, L: int, logits_ptr: int, stream: int):
        w = LoopParams(*[int(p) for p in w_ptrs])
        self._check(self.lib.wrnn_train_forward(self._h, C.byref(w), x_ptr, mels_up_ptr, aux_ptr, int(B), int(L), logits_ptr, stream or None))

    def train_backward(self, w_ptrs, g_ptrs, d_logits_ptr: int, x_ptr: int, mels_up_ptr: int, aux_ptr: int, B: int, L: int,
                       d_mels_up_ptr: int, d_aux_ptr: int, stream: int):
        w = LoopParams(*[int(p) for p in w_ptrs])
        g = LoopParams(*[int(p) for p in g_ptrs])
        self._check(self.lib.wrnn_train_backward(self._h, C.byref(w), C.byref(g), d_logits_ptr, x_ptr, mels_up_ptr, aux_ptr, int(B), int(L),
                                                 d_mels_up_ptr or None, d_aux_ptr or None, stream or None))

    def sync_status(self, stream: int):
        """Waits for the stream; raises WrnnError for a device-side team-kernel error of ``train_step`` (busy GPU / timeout)."""
        self._check(self.lib.wrnn_sync_status(self._h, stream or None))

    def train_force_step_kernels(self, on: bool):
        self._check(self.lib.wrnn_train_force_step_kernels(self._h, int(bool(on))))

    def train_last_recurrence(self) -> Tuple[str, int]:
        """('steps' | 'team512', rows per team batch) of the last training call on this handle (``wrnn_train_last_recurrence``)."""
        k, r = C.c_int32(), C.c_int32()
        self._check(self.lib.wrnn_train_last_recurrence(self._h, C.byref(k), C.byref(r)))
        return TRAIN_RAN_NAMES[int(k.value)], int(r.value)

    def set_train_precision(self, precision: str):
        """'f32' (default) or 'bf16': the kernel the batched GEMMs of the following training calls run on (``wrnn_train_set_precision``).
        The two GEMMs on the sample input ``x`` and the recurrences stay fp32 either way."""
        self._check(self.lib.wrnn_train_set_precision(self._h, _train_precision_id(precision)))

    @property
    def train_precision(self) -> str:
        fmt = C.c_int32()
        self._check(self.lib.wrnn_train_precision(self._h, C.byref(fmt)))
        return TRAIN_PRECISION_NAMES[int(fmt.value)]

    def train_last_gemms(self) -> Tuple[int, int]:
        """(GEMMs on the fp32 kernel, GEMMs on the bf16 kernel) of the last training call on this handle (``wrnn_train_last_gemms``);
        ``WrnnError`` (WRNN_ERR_STATE) before any."""
        a, b = C.c_int32(), C.c_int32()
        self._check(self.lib.wrnn_train_last_gemms(self._h, C.byref(a), C.byref(b)))
        return int(a.value), int(b.value)

    def debug_train_gemm(self, precision: str, ta: bool, tb: bool, a_ptr: int, lda: int, b_ptr: int, ldb: int, c_ptr: int, ldc: int, M: int,
                         N: int, K: int, *, beta: bool = False, bias_ptr: int = 0, relu: bool = False, slices: int = 1, stream: int = 0):
        """``wrnn_debug_train_gemm``: C (M, N) = (beta) C + A.B (+ bias) (relu) on device float32 buffers through the training calls' GEMM
        dispatcher and split-K wrapper, ``precision`` ('f32' / 'bf16') taken literally.  ``ValueError`` for arguments that are wrong on
        their face (:func:`check_train_gemm_args`), ``WrnnError`` (WRNN_ERR_UNSUPPORTED) for ta and tb in bf16."""
        prec = check_train_gemm_args(precision, bool(ta), bool(tb), int(lda), int(ldb), int(ldc), int(M), int(N), int(K), int(bias_ptr or 0),
                                     bool(relu), int(slices))
        if not (a_ptr and b_ptr and c_ptr):
            raise ValueError('debug_train_gemm: A, B and C are device pointers')
        self._check(self.lib.wrnn_debug_train_gemm(self._h, prec, int(bool(ta)), int(bool(tb)), a_ptr, int(lda), b_ptr, int(ldb), c_ptr, int(ldc),
                                                   int(M), int(N), int(K), int(bool(beta)), bias_ptr or None, int(bool(relu)), int(slices),
                                                   stream or None))

    def loss(self, y_hat_ptr: int, y_ptr: int, n_rows: int, out_ptr: int, stream: int):
        self._check(self.lib.wrnn_loss(self._h, y_hat_ptr, y_ptr, int(n_rows), out_ptr, stream or None))

    def team_info(self) -> Tuple[bool, int, str]:
        """(the XCD-team kernels can run for this handle, number of 32-CU teams, reason when they cannot) -- ``wrnn_team_info``."""
        n, why = C.c_int32(), C.c_char_p()
        ok = self.lib.wrnn_team_info(self._h, C.byref(n), C.byref(why))
        return bool(ok), int(n.value), (why.value or b'').decode()

    def debug_force_no_teams(self, on: bool):
        """Test hook: AUTO behaves as if the team kernels' residency check had failed."""
        self._check(self.lib.wrnn_debug_force_no_teams(self._h, int(bool(on))))

    def teamg_plan(self, lds_budget_bytes: int = -1) -> dict:
        """Ownership and weight placement of WRNN_KERNEL_TEAMG for this model (:func:`teamg_plan`; host only)."""
        return teamg_plan(lds_budget_bytes, **self._dims)

    def teamg_batch_plan(self, rows_per_team: int, lds_budget_bytes: int = -1) -> dict:
        """The plan of WRNN_KERNEL_TEAMG_BATCH for this model with ``rows_per_team`` rows in lock-step (:func:`teamg_batch_plan`; host only)."""
        return teamg_batch_plan(rows_per_team, lds_budget_bytes, **self._dims)

    def debug_teamg_lds_budget(self, lds_budget_bytes: int):
        """Test hook: the following WRNN_KERNEL_TEAMG / WRNN_KERNEL_TEAMG_BATCH calls place their weights with this LDS budget (< 0: the default)."""
        self._check(self.lib.wrnn_debug_teamg_lds_budget(self._h, int(lds_budget_bytes)))

    def set_teamg_weights(self, fmt: str):
        """The element type of the TEAMG / TEAMG_BATCH weight image, 'f32', 'f16' or 'e4m3' (``wrnn_teamg_set_weight_format``); a change makes
        the next call of either kernel pack the image again.  No other kernel reads it."""
        if not isinstance(fmt, str) or fmt not in TEAMG_WEIGHT_FORMATS:
            raise ValueError(f'teamg weights must be one of {sorted(TEAMG_WEIGHT_FORMATS)}, not {fmt!r}')
        self._check(self.lib.wrnn_teamg_set_weight_format(self._h, TEAMG_WEIGHT_FORMATS[fmt]))

    @property
    def teamg_weights(self) -> str:
        return TEAMG_WEIGHT_FORMAT_NAMES[int(self.lib.wrnn_teamg_weight_format(self._h))]

    def teamg_weight_scales(self) -> np.ndarray:
        """The six per-layer scales of the image last packed (``wrnn_teamg_weight_scales``), in the order fc3, fc2, fc1, rnn2, rnn1, I;
        ones unless that image was 'e4m3'."""
        out = (C.c_float * 6)()
        self._check(self.lib.wrnn_teamg_weight_scales(self._h, out))
        return np.array(out[:], np.float32)

    def set_teamg_sparse(self, on: bool):
        """Block-sparse fp32 weight image for TEAMG / TEAMG_BATCH (``wrnn_teamg_set_sparse``): the pack leaves out every 64-element block of
        an image row whose weights are all zero.  A change makes the next call of either kernel pack again.  No other kernel reads it."""
        if not isinstance(on, (bool, np.bool_)):
            raise ValueError(f'teamg sparse must be a bool, not {on!r}')
        self._check(self.lib.wrnn_teamg_set_sparse(self._h, 1 if on else 0))

    @property
    def teamg_sparse(self) -> bool:
        return bool(self.lib.wrnn_teamg_sparse(self._h))

    def teamg_sparse_info(self) -> dict:
        """``wrnn_teamg_sparse_info``: the sparse image last packed.  ``layers``: name -> ``dict(kept, dense, nb_a, nb_b)`` (non-zero blocks,
        blocks of the dense rows, blocks per image row and segment); ``kept`` / ``dense``: their sums; ``plan``: the plan in force (the
        dict of :func:`teamg_sparse_plan`).  ``WrnnError`` (WRNN_ERR_STATE) before a call has packed a sparse image."""
        kept, dense, nb_a, nb_b = (C.c_int64 * 6)(), (C.c_int64 * 6)(), (C.c_int32 * 6)(), (C.c_int32 * 6)()
        info = TeamgPlanInfo()
        self._check(self.lib.wrnn_teamg_sparse_info(self._h, kept, dense, nb_a, nb_b, C.byref(info)))
        layers = {n: dict(kept=int(kept[i]), dense=int(dense[i]), nb_a=int(nb_a[i]), nb_b=int(nb_b[i])) for i, n in enumerate(TEAMG_LAYER_NAMES)}
        plan = {f: int(getattr(info, f)) for f, _ in TeamgPlanInfo._fields_ if f != 'layer'}
        plan['layers'] = {}
        for name, li in zip(TEAMG_LAYER_NAMES, info.layer):
            plan['layers'][name] = {f: (list(getattr(li, f)) if f.startswith('own_') else int(getattr(li, f))) for f, _ in TeamgLayerInfo._fields_ if f != 'reserved_'}
        return dict(layers=layers, kept=sum(kept[:]), dense=sum(dense[:]), plan=plan)

    def last_timing(self) -> dict:
        t = Timing()
        self._check(self.lib.wrnn_last_timing(self._h, C.byref(t)))
        return dict(prologue_ms=t.prologue_ms, loop_ms=t.loop_ms, kernel=t.kernel, rows=t.rows, steps=t.steps,
                    launches=t.launches, batch_rows=int(self.lib.wrnn_last_batch_rows(self._h)), teamg_weights=self.teamg_weights,
                    teamg_sparse=self.teamg_sparse)


def plan_folded(frames, hop: int, target: int, overlap: int) -> Tuple[np.ndarray, int]:
    """Host-only ``wrnn_plan_folded``: (fold0 (B + 1,) int32 -- first row of every utterance, fold0[B] = rows in all --, steps per row) for
    a call that folds utterances of ``frames[b]`` mel frames with one ``target``.  ``WrnnError`` (WRNN_ERR_INVALID) for an utterance that
    yields no fold or bad arguments."""
    fr = np.ascontiguousarray(frames, dtype=np.int32).reshape(-1)
    fold0 = np.zeros(fr.size + 1, np.int32)
    steps = C.c_int64()
    rc = load_library().wrnn_plan_folded(fr.ctypes.data, int(fr.size), int(hop), int(target), int(overlap), fold0.ctypes.data, C.byref(steps))
    if rc != 0:
        raise WrnnError(rc, f'wrnn_plan_folded: no fold plan for frames {fr.tolist()[:8]}{"..." if fr.size > 8 else ""}, hop {hop}, target {target}, overlap {overlap}')
    return fold0, int(steps.value)


def stream_ready_steps(frames_in: int, hop: int, pad: int, last: bool) -> int:
    """Host-only ``wrnn_stream_ready_steps``: loop steps a stream can run after ``frames_in`` mel frames (-1 for bad arguments)."""
    return int(load_library().wrnn_stream_ready_steps(int(frames_in), int(hop), int(pad), int(bool(last))))


def quantise(wav_ptr: int, n: int, bits: int, mu_law: bool, labels_ptr: int, n_clipped_ptr: int, stream: int):
    """``wrnn_quantise``: n float32 samples -> int32 class labels on the device; samples with ``|x| > 1`` are added to the int64 at
    ``n_clipped_ptr`` (0: not counted).  ``WrnnError`` for a refused call (bad arguments are refused before any device call)."""
    rc = load_library().wrnn_quantise(wav_ptr or None, int(n), int(bits), int(bool(mu_law)), labels_ptr or None, n_clipped_ptr or None, stream or None)
    if rc != 0:
        raise WrnnError(rc, f'wrnn_quantise(n={int(n)}, bits={int(bits)})')


def collate_windows(labels_ptr: int, mels_ptr: int, label_off_ptr: int, mel_off_ptr: int, frames_ptr: int, utt_ptr: int, win_off_ptr: int,
                    B: int, n_mels: int, hop: int, pad: int, seq_len: int, sig_bits: int, y_float: bool, x_ptr: int, y_ptr: int,
                    mels_out_ptr: int, stream: int):
    """``wrnn_collate_windows``: one training batch cut from the device-resident corpus, one launch."""
    rc = load_library().wrnn_collate_windows(labels_ptr or None, mels_ptr or None, label_off_ptr or None, mel_off_ptr or None, frames_ptr or None,
                                             utt_ptr or None, win_off_ptr or None, int(B), int(n_mels), int(hop), int(pad), int(seq_len),
                                             int(sig_bits), int(bool(y_float)), x_ptr or None, y_ptr or None, mels_out_ptr or None, stream or None)
    if rc != 0:
        raise WrnnError(rc, f'wrnn_collate_windows(B={int(B)}, n_mels={int(n_mels)}, hop={int(hop)}, pad={int(pad)}, seq_len={int(seq_len)}, '
                            f'sig_bits={int(sig_bits)})')


def condition_frames(n: int, frame_length: int, hop: int) -> int:
    """Host-only ``wrnn_condition_frames``: the ``1 + n // hop`` energy frames of a clip of ``n`` samples; ``ValueError`` for a window the
    library refuses (``frame_length`` outside 2 .. 8192, ``hop`` outside 1 .. ``frame_length``) or a clip too short to reflect-pad."""
    fits = all(-2 ** 31 <= int(v) < 2 ** 31 for v in (frame_length, hop)) and -2 ** 63 <= int(n) < 2 ** 63
    f = int(load_library().wrnn_condition_frames(int(n), int(frame_length), int(hop))) if fits else -1
    if f < 0:
        raise ValueError(f'no energy frames for a clip of {int(n)} samples with frame_length {int(frame_length)}, hop {int(hop)}: the window '
                         f'must be 2 .. 8192 samples, the hop 1 .. frame_length, and the clip at least frame_length // 2 + 1 samples')
    return f


def condition(wav_ptr: int, n_max: int, n_ptr: int, B: int, trim: bool, top_db: float, frame_length: int, hop: int, peak_target: float,
              energy_ws_ptr: int, F_max: int, out_ptr: int, n_out_max: int, n_out_ptr: int, bounds_ptr: int, peak_ptr: int, stream: int):
    """``wrnn_condition``: silence trimming and peak normalisation of B ragged clips, three launches, nothing waits.  ``energy_ws_ptr``:
    ``B * F_max + B`` float64.  ``WrnnError`` for a refused call (bad arguments are refused before any device call)."""
    rc = load_library().wrnn_condition(wav_ptr or None, int(n_max), n_ptr or None, int(B), int(bool(trim)), float(top_db), int(frame_length),
                                       int(hop), float(peak_target), energy_ws_ptr or None, int(F_max), out_ptr or None, int(n_out_max),
                                       n_out_ptr or None, bounds_ptr or None, peak_ptr or None, stream or None)
    if rc != 0:
        raise WrnnError(rc, f'wrnn_condition(B={int(B)}, n_max={int(n_max)}, trim={bool(trim)}, top_db={float(top_db)}, frame_length={int(frame_length)}, '
                            f'hop={int(hop)}, peak_target={float(peak_target)}, F_max={int(F_max)}, n_out_max={int(n_out_max)})')


class NativeStream:
    """Owner of one ``wrnn_stream`` opened on a :class:`NativeVocoder`'s handle (which it keeps alive)."""

    def __init__(self, nat: NativeVocoder, B: int, *, noise_mode: int = NOISE_PHILOX, seed: int = 0, kernel: int = KERNEL_AUTO):
        self.nat, self.lib = nat, nat.lib
        o = SampleOpts()
        o.struct_size = C.sizeof(SampleOpts)
        o.noise_mode, o.kernel, o.seed = int(noise_mode), int(kernel), int(seed) & 0xFFFFFFFFFFFFFFFF
        self._s = C.c_void_p()
        nat._check(self.lib.wrnn_stream_open(nat._h, int(B), C.byref(o), C.byref(self._s)))

    def push(self, mels_ptr: int, n_frames: int, last: bool, labels_ptr: int, samples_ptr: int, capacity: int, stream: int) -> int:
        """Enqueues the steps that became ready; returns their count (known without waiting)."""
        n = C.c_int64()
        self.nat._check(self.lib.wrnn_stream_push(self._s, mels_ptr or None, int(n_frames), int(bool(last)), labels_ptr or None,
                                                  samples_ptr or None, int(capacity), C.byref(n), stream or None))
        return int(n.value)

    def sync(self, stream: int):
        """Waits for ``stream``; raises WrnnError for a device-side error of the pushes so far (the stream is then unusable)."""
        self.nat._check(self.lib.wrnn_stream_sync(self._s, stream or None))

    def info(self) -> dict:
        f, s, w = C.c_int64(), C.c_int64(), C.c_int64()
        self.nat._check(self.lib.wrnn_stream_info(self._s, C.byref(f), C.byref(s), C.byref(w)))
        return dict(frames_in=int(f.value), steps_done=int(s.value), workspace_bytes=int(w.value))

    def close(self):
        if getattr(self, '_s', None):
            self.lib.wrnn_stream_close(self._s)
            self._s = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _tensor_descs(state_dict: Dict[str, np.ndarray]):
    keep, descs = [], []
    for name, arr in state_dict.items():
        arr = np.ascontiguousarray(arr)
        if arr.dtype != np.float32 or arr.ndim > 4:
            continue
        d = TensorDesc()
        d.name = name.encode()
        d.dtype, d.ndim = DTYPE_F32, arr.ndim
        for i, sdim in enumerate(arr.shape):
            d.shape[i] = sdim
        d.data = arr.ctypes.data
        keep.append(arr)
        descs.append(d)
    return keep, (TensorDesc * len(descs))(*descs), len(descs)


class NativeDeepmind:
    """Owner of one ``wrnn_dm_handle`` (the secondary dual-softmax model)."""

    def __init__(self, hidden_size: int, quantisation: int, device: int):
        self.lib = load_library()
        self.device = int(device)
        self._h = C.c_void_p()
        rc = self.lib.wrnn_dm_create(hidden_size, quantisation, device, C.byref(self._h))
        if rc != 0:
            msg = self.lib.wrnn_dm_last_error(self._h).decode() if self._h else 'wrnn_dm_create failed'
            self.close()
            raise WrnnError(rc, msg)

    def _check(self, rc: int):
        if rc != 0:
            raise WrnnError(rc, self.lib.wrnn_dm_last_error(self._h).decode())

    def close(self):
        if getattr(self, '_h', None):
            self.lib.wrnn_dm_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def load_weights(self, state_dict: Dict[str, np.ndarray]):
        keep, arr, n = _tensor_descs(state_dict)
        self._check(self.lib.wrnn_dm_load_weights(self._h, arr, n))

    def generate(self, seq_len: int, coarse_ptr: int, fine_ptr: int, stream: int, noise_mode: int = NOISE_PHILOX,
                 seed: int = 0, noise_ptr: int = 0):
        self._check(self.lib.wrnn_dm_generate(self._h, int(seq_len), noise_mode, seed & 0xFFFFFFFFFFFFFFFF,
                                              noise_ptr or None, coarse_ptr, fine_ptr, stream or None))
        self._check(self.lib.wrnn_dm_sync_status(self._h, stream or None))   # waits; surfaces device-side errors

    def set_kernel(self, kernel: int):
        self._check(self.lib.wrnn_dm_set_kernel(self._h, int(kernel)))


class NativeMel:
    """Owner of one ``wrnn_mel_handle`` (the wav -> mel front end; no weights).  Creating it touches no device; a configuration the
    library refuses raises ``ValueError`` (n_fft other than 2048: WRNN_ERR_UNSUPPORTED; the rest: WRNN_ERR_INVALID).  ``features``: a
    ``MelFeatures`` (``wrnn_mel_create_features``); ``None`` is the default profile through ``wrnn_mel_create``."""

    def __init__(self, *, sample_rate, n_fft, hop_length, win_length, n_mels, fmin, min_level_db, device: int = 0, features=None):
        self.lib = load_library()
        cfg = MelConfig(int(sample_rate), int(n_fft), int(hop_length), int(win_length), int(n_mels), float(fmin), float(min_level_db), int(device))
        self.cfg = cfg
        self.features = features
        self.device = int(device)
        self._h = C.c_void_p()
        if features is None:
            rc = self.lib.wrnn_mel_create(C.byref(cfg), C.byref(self._h))
        else:
            rc = self.lib.wrnn_mel_create_features(C.byref(cfg), C.byref(features), C.byref(self._h))
        if rc != 0:
            msg = self.lib.wrnn_mel_last_error(self._h).decode() if self._h else 'wrnn_mel_create failed'
            self.close()
            raise ValueError(f'{ERR_NAMES.get(rc, rc)}: {msg}')

    def _check(self, rc: int):
        if rc != 0:
            raise WrnnError(rc, self.lib.wrnn_mel_last_error(self._h).decode())

    def frames(self, n_samples: int) -> int:
        """Host-only ``wrnn_mel_frames``: 1 + n // hop; ``ValueError`` for a clip too short to reflect-pad (an empty one under zero
        padding)."""
        t = int(self.lib.wrnn_mel_frames(self._h, int(n_samples)))
        if t < 0 and self.features is not None and self.features.pad_mode == MEL_PAD_MODES['zero']:
            raise ValueError(f'a clip of {int(n_samples)} samples has no frames: at least 1 sample is needed')
        if t < 0:
            raise ValueError(f'a clip of {int(n_samples)} samples cannot be reflect-padded by n_fft/2 = {self.cfg.n_fft // 2}: '
                             f'at least {self.cfg.n_fft // 2 + 1} samples are needed')
        return t

    def tables(self) -> dict:
        """The float32 tables the kernel reads (``wrnn_mel_tables``): window, twiddle (n_fft, 2), rows (n_mels, 3), weights."""
        nw = C.c_int32()
        self._check(self.lib.wrnn_mel_tables(self._h, None, None, None, None, C.byref(nw)))
        window = np.empty(self.cfg.win_length, np.float32)
        twiddle = np.empty((self.cfg.n_fft, 2), np.float32)
        rows = np.empty((self.cfg.n_mels, 3), np.int32)
        weights = np.empty(nw.value, np.float32)
        self._check(self.lib.wrnn_mel_tables(self._h, window.ctypes.data, twiddle.ctypes.data, rows.ctypes.data, weights.ctypes.data, None))
        return dict(window=window, twiddle=twiddle, rows=rows, weights=weights)

    def melspectrogram(self, wav_ptr: int, n_max: int, n_samples_ptr: int, B: int, T_max: int, out_ptr: int, stream: int):
        self._check(self.lib.wrnn_melspectrogram(self._h, wav_ptr, int(n_max), n_samples_ptr, int(B), int(T_max), out_ptr, stream or None))

    def close(self):
        if getattr(self, '_h', None):
            self.lib.wrnn_mel_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class NativeGriffinLim:
    """Owner of one ``wrnn_griffin_handle`` (mel -> wav by Griffin-Lim; no weights).  Creating it touches no device; a configuration the
    library refuses raises ``ValueError`` (n_fft other than 2048 or a filterbank that cannot be inverted: WRNN_ERR_UNSUPPORTED; the rest:
    WRNN_ERR_INVALID).  ``features``: a ``MelFeatures``; ``griffin``: a ``GriffinConfig``."""

    def __init__(self, *, sample_rate, n_fft, hop_length, win_length, n_mels, fmin, min_level_db, device: int = 0, features=None, griffin=None):
        self.lib = load_library()
        cfg = MelConfig(int(sample_rate), int(n_fft), int(hop_length), int(win_length), int(n_mels), float(fmin), float(min_level_db), int(device))
        self.cfg = cfg
        self.features = features if features is not None else MelFeatures()
        self.griffin = griffin if griffin is not None else GriffinConfig()
        self.device = int(device)
        self._h = C.c_void_p()
        rc = self.lib.wrnn_griffin_create(C.byref(cfg), C.byref(self.features), C.byref(self.griffin), C.byref(self._h))
        if rc != 0:
            msg = self.lib.wrnn_griffin_last_error(self._h).decode() if self._h else 'wrnn_griffin_create failed'
            self.close()
            raise ValueError(f'{ERR_NAMES.get(rc, rc)}: {msg}')

    def _check(self, rc: int):
        if rc != 0:
            raise WrnnError(rc, self.lib.wrnn_griffin_last_error(self._h).decode())

    def samples(self, frames: int) -> int:
        """Host-only ``wrnn_griffin_samples``: ``hop (frames - 1)``; ``ValueError`` for ``frames < 1``."""
        n = int(self.lib.wrnn_griffin_samples(self._h, int(frames))) if 1 <= int(frames) < 2 ** 31 else -1
        if n < 0:
            raise ValueError(f'a mel of {int(frames)} frames has no wav: at least 1 frame is needed')
        return n

    def tables(self, frames: int = 1) -> dict:
        """``wrnn_griffin_tables``: pinv (n_fft/2 + 1, n_mels), window, and the window-sum-square of a clip of ``frames`` frames over
        the ``n_fft + hop (frames - 1)`` positions of the padded signal, all float32."""
        pinv = np.empty((self.cfg.n_fft // 2 + 1, self.cfg.n_mels), np.float32)
        window = np.empty(self.cfg.win_length, np.float32)
        wss = np.empty(self.cfg.n_fft + self.cfg.hop_length * (int(frames) - 1), np.float32)
        self._check(self.lib.wrnn_griffin_tables(self._h, pinv.ctypes.data, window.ctypes.data, int(frames), wss.ctypes.data))
        return dict(pinv=pinv, window=window, window_sumsquare=wss)

    def griffin_lim(self, mel_ptr: int, frames_ptr: int, B: int, T_max: int, n_iter: int, phase_mode: int, seed: int, phases_ptr: int,
                    out_ptr: int, n_out_max: int, magnitude_ptr: int, stream: int):
        self._check(self.lib.wrnn_griffin_lim(self._h, mel_ptr or None, frames_ptr or None, int(B), int(T_max), int(n_iter), int(phase_mode),
                                              int(seed) & (2 ** 64 - 1), phases_ptr or None, out_ptr or None, int(n_out_max),
                                              magnitude_ptr or None, stream or None))

    def close(self):
        if getattr(self, '_h', None):
            self.lib.wrnn_griffin_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class NativeScore:
    """Owner of one ``wrnn_score_handle`` (spectral scores of a test clip against a target; no weights).  Creating it touches no device;
    a configuration the library refuses raises ``ValueError``.  ``features``: a ``MelFeatures`` or ``None`` (the default profile);
    ``score``: a ``ScoreConfig``."""

    def __init__(self, *, sample_rate, n_fft, hop_length, win_length, n_mels, fmin, min_level_db, device: int = 0, features=None, score=None):
        self.lib = load_library()
        cfg = MelConfig(int(sample_rate), int(n_fft), int(hop_length), int(win_length), int(n_mels), float(fmin), float(min_level_db), int(device))
        self.cfg = cfg
        self.features = features
        self.score_config = score if score is not None else ScoreConfig()
        self.device = int(device)
        self._h = C.c_void_p()
        rc = self.lib.wrnn_score_create(C.byref(cfg), C.byref(features) if features is not None else None, C.byref(self.score_config),
                                        C.byref(self._h))
        if rc != 0:
            msg = self.lib.wrnn_score_last_error(self._h).decode() if self._h else 'wrnn_score_create failed'
            self.close()
            raise ValueError(f'{ERR_NAMES.get(rc, rc)}: {msg}')
        self.n_res = int(self.score_config.n_res)
        self.resolutions = [(int(self.score_config.n_fft[r]), int(self.score_config.hop[r]), int(self.score_config.win[r])) for r in range(self.n_res)]
        reflect = features is None or features.pad_mode == MEL_PAD_MODES['reflect']
        self.min_samples = max([n // 2 + 1 for n, _, _ in self.resolutions] + ([cfg.n_fft // 2 + 1] if reflect else [1]))

    def _check(self, rc: int):
        if rc != 0:
            raise WrnnError(rc, self.lib.wrnn_score_last_error(self._h).decode())

    def frames(self, r: int, n: int) -> int:
        """Host-only ``wrnn_score_frames``: the frames of ``n`` samples at resolution ``r`` (``-1``: the mel); ``ValueError`` for a clip
        shorter than ``min_samples`` (it cannot be reflect-padded at every resolution) or an unknown ``r``."""
        if not -1 <= int(r) < self.n_res:
            raise ValueError(f'resolution {int(r)} is outside -1 .. {self.n_res - 1}')
        t = int(self.lib.wrnn_score_frames(self._h, int(r), int(n))) if 0 <= int(n) < 2 ** 31 else -1
        if t < 0:
            raise ValueError(f'a clip of {int(n)} samples cannot be scored: at least {self.min_samples} samples are needed')
        return t

    def layout(self, n_max: int):
        """The per-frame row of a call with ``n_max``: ``[(name, r, offset, frames)]`` in buffer order and the row's length."""
        segs, at = [], 0
        for name, r in [('lsd', -1), ('mcd', -1)] + [(q, r) for r in range(self.n_res) for q in ('num', 'den', 'lm')]:
            t = self.frames(r, n_max)
            segs.append((name, r, at, t))
            at += t
        return segs, at

    def tables(self) -> dict:
        """``wrnn_score_tables``: ``windows`` and ``twiddles`` (n_fft, 2) per resolution, and ``dct`` (mcd_order, n_mels), all float32."""
        K = int(self.score_config.mcd_order)
        dct = np.empty((K, self.cfg.n_mels), np.float32)
        windows, twiddles = [], []
        for r, (n_fft, _, win) in enumerate(self.resolutions):
            w, tw = np.empty(win, np.float32), np.empty((n_fft, 2), np.float32)
            self._check(self.lib.wrnn_score_tables(self._h, r, w.ctypes.data, tw.ctypes.data, dct.ctypes.data))
            windows.append(w)
            twiddles.append(tw)
        return dict(windows=windows, twiddles=twiddles, dct=dct)

    def score(self, target_ptr: int, test_ptr: int, n_max: int, n_ptr: int, B: int, summary_ptr: int, frames_ptr: int, frames_stride: int, stream: int):
        self._check(self.lib.wrnn_score(self._h, target_ptr or None, test_ptr or None, int(n_max), n_ptr or None, int(B), summary_ptr or None,
                                        frames_ptr or None, int(frames_stride), stream or None))

    def close(self):
        if getattr(self, '_h', None):
            self.lib.wrnn_score_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class NativePitch:
    """Owner of one ``wrnn_pitch_handle`` (a YIN F0 track and the F0 / voicing error scores of a pair; no weights, no tables).  Creating
    it touches no device; a configuration the library refuses raises ``ValueError``.  ``config``: a ``PitchConfig``."""

    def __init__(self, config=None):
        self.lib = load_library()
        self.config = config if config is not None else PitchConfig()
        self.device = int(self.config.device)
        self._h = C.c_void_p()
        rc = self.lib.wrnn_pitch_create(C.byref(self.config), C.byref(self._h))
        if rc != 0:
            msg = self.lib.wrnn_pitch_last_error(self._h).decode() if self._h else 'wrnn_pitch_create failed'
            self.close()
            raise ValueError(f'{ERR_NAMES.get(rc, rc)}: {msg}')
        lo, hi = C.c_int32(), C.c_int32()
        self._check(self.lib.wrnn_pitch_lags(self._h, C.byref(lo), C.byref(hi)))
        self.tau_min, self.tau_max = lo.value, hi.value

    def _check(self, rc: int):
        if rc != 0:
            raise WrnnError(rc, self.lib.wrnn_pitch_last_error(self._h).decode())

    def frames(self, n: int) -> int:
        """Host-only ``wrnn_pitch_frames``: ``1 + n // hop`` frames of ``n >= 1`` samples, none of an empty clip."""
        t = int(self.lib.wrnn_pitch_frames(self._h, int(n))) if 0 <= int(n) < 2 ** 31 else -1
        if t < 0:
            raise ValueError(f'a clip length of {int(n)} samples is outside 0 .. 2**31 - 1')
        return t

    def track(self, wav_ptr: int, n_max: int, n_ptr: int, B: int, f0_ptr: int, ap_ptr: int, frames_stride: int, stream: int):
        self._check(self.lib.wrnn_pitch_track(self._h, wav_ptr or None, int(n_max), n_ptr or None, int(B), f0_ptr or None, ap_ptr or None,
                                              int(frames_stride), stream or None))

    def score(self, target_ptr: int, test_ptr: int, n_max: int, n_ptr: int, B: int, summary_ptr: int, frames_ptr: int, frames_stride: int, stream: int):
        self._check(self.lib.wrnn_pitch_score(self._h, target_ptr or None, test_ptr or None, int(n_max), n_ptr or None, int(B), summary_ptr or None,
                                              frames_ptr or None, int(frames_stride), stream or None))

    def close(self):
        if getattr(self, '_h', None):
            self.lib.wrnn_pitch_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class NativeAlign:
    """Owner of one ``wrnn_align_handle`` (the DTW path of a test clip against a target over their mel cepstra, and the scores along it;
    no weights).  Creating it touches no device; a configuration the library refuses raises ``ValueError``.  ``features``: a
    ``MelFeatures`` or ``None`` (the default profile); ``align``: an ``AlignConfig``."""

    def __init__(self, *, sample_rate=22050, n_fft=2048, hop_length=275, win_length=1100, n_mels=80, fmin=95, min_level_db=-100, device: int = 0,
                 features=None, align=None):
        self.lib = load_library()
        cfg = MelConfig(int(sample_rate), int(n_fft), int(hop_length), int(win_length), int(n_mels), float(fmin), float(min_level_db), int(device))
        self.cfg = cfg
        self.features = features
        self.align_config = align if align is not None else AlignConfig()
        self.device = int(device)
        self._h = C.c_void_p()
        rc = self.lib.wrnn_align_create(C.byref(cfg), C.byref(features) if features is not None else None, C.byref(self.align_config),
                                        C.byref(self._h))
        if rc != 0:
            msg = self.lib.wrnn_align_last_error(self._h).decode() if self._h else 'wrnn_align_create failed'
            self.close()
            raise ValueError(f'{ERR_NAMES.get(rc, rc)}: {msg}')
        reflect = features is None or features.pad_mode == MEL_PAD_MODES['reflect']
        self.min_samples = cfg.n_fft // 2 + 1 if reflect else 1

    def _check(self, rc: int):
        if rc != 0:
            raise WrnnError(rc, self.lib.wrnn_align_last_error(self._h).decode())

    def frames(self, n: int) -> int:
        """Host-only ``wrnn_align_frames``: ``1 + n // hop_length``; ``ValueError`` for a clip shorter than ``min_samples``."""
        t = int(self.lib.wrnn_align_frames(self._h, int(n))) if 0 <= int(n) < 2 ** 31 else -1
        if t < 0:
            raise ValueError(f'a clip of {int(n)} samples cannot be aligned: at least {self.min_samples} samples are needed')
        return t

    def workspace_bytes(self, B: int, na_max: int, nb_max: int) -> int:
        """Host-only ``wrnn_align_workspace_bytes``: the scratch of a score call, or ``WrnnError`` with the status of its refusal."""
        if not (0 <= int(B) < 2 ** 31 and 0 <= int(na_max) < 2 ** 63 and 0 <= int(nb_max) < 2 ** 63):
            raise WrnnError(ERR_INVALID, f'B = {B}, na_max = {na_max}, nb_max = {nb_max} do not fit the entry')
        n = int(self.lib.wrnn_align_workspace_bytes(self._h, int(B), int(na_max), int(nb_max)))
        if n < 0:
            raise WrnnError(n, self.lib.wrnn_align_last_error(self._h).decode())
        return n

    def cost(self, target_ptr: int, na_max: int, na_ptr: int, test_ptr: int, nb_max: int, nb_ptr: int, B: int, cost_ptr: int, stream: int):
        self._check(self.lib.wrnn_align_cost(self._h, target_ptr or None, int(na_max), na_ptr or None, test_ptr or None, int(nb_max), nb_ptr or None,
                                             int(B), cost_ptr or None, stream or None))

    def path(self, cost_ptr: int, B: int, Ta_max: int, Tb_max: int, ta_ptr: int, tb_ptr: int, path_ptr: int, path_len_ptr: int, total_ptr: int,
             stream: int):
        self._check(self.lib.wrnn_align_path(self._h, cost_ptr or None, int(B), int(Ta_max), int(Tb_max), ta_ptr or None, tb_ptr or None,
                                             path_ptr or None, path_len_ptr or None, total_ptr or None, stream or None))

    def score(self, target_ptr: int, na_max: int, na_ptr: int, test_ptr: int, nb_max: int, nb_ptr: int, B: int, f0_target_ptr: int, f0_test_ptr: int,
              f0_stride: int, summary_ptr: int, path_ptr: int, path_len_ptr: int, per_path_ptr: int, stream: int):
        self._check(self.lib.wrnn_align_score(self._h, target_ptr or None, int(na_max), na_ptr or None, test_ptr or None, int(nb_max), nb_ptr or None,
                                              int(B), f0_target_ptr or None, f0_test_ptr or None, int(f0_stride), summary_ptr or None,
                                              path_ptr or None, path_len_ptr or None, per_path_ptr or None, stream or None))

    def close(self):
        if getattr(self, '_h', None):
            self.lib.wrnn_align_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def deemphasis(wav_ptr: int, n_max: int, n_ptr: int, B: int, k: float, out_ptr: int, stream: int):
    """``wrnn_deemphasis``: ``out[b, i] = wav[b, i] + k out[b, i-1]`` over B ragged clips, one launch, nothing waits."""
    rc = load_library().wrnn_deemphasis(wav_ptr or None, int(n_max), n_ptr or None, int(B), float(k), out_ptr or None, stream or None)
    if rc != 0:
        raise WrnnError(rc, f'wrnn_deemphasis(B={int(B)}, n_max={int(n_max)}, k={float(k)}) refused its arguments')


class NativeResampler:
    """Owner of one ``wrnn_resample_handle`` (``src_rate -> dst_rate``).  Creating it touches no device; rates the library refuses raise
    ``ValueError`` (a rate <= 0: WRNN_ERR_INVALID; a ratio below 1/32 or an oversized filter bank: WRNN_ERR_UNSUPPORTED)."""

    def __init__(self, src_rate: int, dst_rate: int, device: int = 0):
        self.lib = load_library()
        self.src_rate, self.dst_rate, self.device = int(src_rate), int(dst_rate), int(device)
        if not (-2 ** 31 <= self.src_rate < 2 ** 31 and -2 ** 31 <= self.dst_rate < 2 ** 31):
            raise ValueError(f'WRNN_ERR_INVALID: sample rates {src_rate} -> {dst_rate} do not fit 32 bits')
        self._h = C.c_void_p()
        rc = self.lib.wrnn_resample_create(self.src_rate, self.dst_rate, self.device, C.byref(self._h))
        if rc != 0:
            msg = self.lib.wrnn_resample_last_error(self._h).decode() if self._h else 'wrnn_resample_create failed'
            self.close()
            raise ValueError(f'{ERR_NAMES.get(rc, rc)}: {msg}')
        p, q, taps = C.c_int32(), C.c_int32(), C.c_int32()
        self._check(self.lib.wrnn_resample_bank(self._h, None, C.byref(p), C.byref(q), C.byref(taps)))
        self.p, self.q, self.taps = p.value, q.value, taps.value

    def _check(self, rc: int):
        if rc != 0:
            raise WrnnError(rc, self.lib.wrnn_resample_last_error(self._h).decode())

    def out_len(self, n_in: int) -> int:
        """Host-only ``wrnn_resample_out_len``: ceil(n p / q)."""
        n = int(self.lib.wrnn_resample_out_len(self._h, int(n_in))) if 0 <= int(n_in) < 2 ** 31 else -1
        if n < 0:
            raise ValueError(f'a clip length of {int(n_in)} samples is outside 0 .. 2**31 - 1')
        return n

    def bank(self) -> np.ndarray:
        """The float32 filter bank (``wrnn_resample_bank``), ``(p, taps)``: row r holds ``h(k - taps / 2 + 1 - r / p)``."""
        bank = np.empty((self.p, self.taps), np.float32)
        self._check(self.lib.wrnn_resample_bank(self._h, bank.ctypes.data, None, None, None))
        return bank

    def resample(self, in_ptr: int, n_in_max: int, n_in_ptr: int, B: int, n_out_max: int, out_ptr: int, stream: int):
        self._check(self.lib.wrnn_resample(self._h, in_ptr, int(n_in_max), n_in_ptr, int(B), int(n_out_max), out_ptr, stream or None))

    def close(self):
        if getattr(self, '_h', None):
            self.lib.wrnn_resample_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class NativeTacotron:
    """Owner of one ``wrnn_taco_handle`` (Tacotron-2 inference: symbol ids -> mel).  Creating it touches no device; dims the library
    refuses raise ``WrnnError`` with its reason."""

    def __init__(self, dims: TacoDims, lib=None):
        self.lib = lib if lib is not None else load_library()   # lib: another build of the library with its wrnn_taco_* argtypes set (A/B tools)
        self.dims = dims
        self._h = C.c_void_p()
        rc = self.lib.wrnn_taco_create(C.byref(dims), C.byref(self._h))
        if rc != 0:
            msg = self.lib.wrnn_taco_last_error(self._h).decode() if self._h else 'wrnn_taco_create failed'
            self.close()
            raise WrnnError(rc, msg)

    def _check(self, rc: int):
        if rc != 0:
            raise WrnnError(rc, self.lib.wrnn_taco_last_error(self._h).decode())

    def tensor_shapes(self) -> "Dict[str, Tuple[int, ...]]":
        """The library's own table: name -> shape, in its order."""
        out, shape = {}, (C.c_int64 * 3)()
        for i in range(self.lib.wrnn_taco_tensor_count(self._h)):
            nd = self.lib.wrnn_taco_tensor_shape(self._h, i, shape)
            out[self.lib.wrnn_taco_tensor_name(self._h, i).decode()] = tuple(int(shape[k]) for k in range(nd))
        return out

    def load_tensor(self, name: str, array: np.ndarray):
        a = np.ascontiguousarray(array, dtype=np.float32)
        shape = (C.c_int64 * max(a.ndim, 1))(*a.shape)
        self._check(self.lib.wrnn_taco_load_tensor(self._h, name.encode(), a.ctypes.data, a.ndim, shape))

    def synthesize(self, call: TacoCall, stream: int):
        self._check(self.lib.wrnn_taco_synthesize(self._h, C.byref(call), stream or None))

    def gta_corpus(self, call: TacoGtaCall, stream: int = 0) -> None:
        """``wrnn_taco_gta_corpus``: one group of a corpus; waits only if its scratch has to grow (``gta_reserve``)."""
        self._check(self.lib.wrnn_taco_gta_corpus(self._h, C.byref(call), stream or None))

    def gta_reserve(self, B: int, Tx_max: int, frames_max: int, stream: int = 0) -> int:
        """``wrnn_taco_gta_reserve``: the scratch for groups of up to this shape, grown now; returns ``gta_workspace_bytes()``."""
        self._check(self.lib.wrnn_taco_gta_reserve(self._h, int(B), int(Tx_max), int(frames_max), stream or None))
        return self.gta_workspace_bytes()

    def gta_workspace_bytes(self) -> int:
        return int(self.lib.wrnn_taco_gta_workspace_bytes(self._h))

    def stream_open(self, opts: 'TacoStreamOpts', stream: int) -> 'NativeTacotronStream':
        st = C.c_void_p()
        self._check(self.lib.wrnn_taco_stream_open(self._h, C.byref(opts), stream or None, C.byref(st)))
        return NativeTacotronStream(self, st, int(opts.B))

    def close(self):
        if getattr(self, '_h', None):
            self.lib.wrnn_taco_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def taco_stream_halo(dims: TacoDims) -> int:
    """Host only: ``wrnn_taco_stream_halo`` -- the decoder frames a mel frame waits for."""
    return int(load_library().wrnn_taco_stream_halo(C.byref(dims)))


class NativeTacotronStream:
    """Owner of one ``wrnn_taco_stream``; it keeps its ``NativeTacotron`` alive."""

    def __init__(self, owner: NativeTacotron, st, B: int):
        self.owner, self.lib, self._st, self.B = owner, owner.lib, st, B

    def _live(self):
        if not self._st:
            raise WrnnError(ERR_STATE, 'the stream is closed')
        return self._st

    def _check(self, rc: int):
        if rc != 0:
            raise WrnnError(rc, self.lib.wrnn_taco_stream_last_error(self._st).decode())

    def step(self, n: int, stream: int):
        """(decoder frames so far, final mel frames so far, finished) per utterance, after the one wait of the push."""
        st = self._live()
        dec, fin, done = ((C.c_int32 * self.B)() for _ in range(3))
        self._check(self.lib.wrnn_taco_stream_step(st, int(n), stream or None, dec, fin, done))
        return list(dec), list(fin), [bool(x) for x in done]

    def view(self) -> TacoStreamOutputs:
        v = TacoStreamOutputs()
        v.struct_size = C.sizeof(TacoStreamOutputs)
        self._check(self.lib.wrnn_taco_stream_view(self._live(), C.byref(v)))
        return v

    def info(self) -> dict:
        b, tx, it, halo, ws = C.c_int32(), C.c_int32(), C.c_int32(), C.c_int32(), C.c_int64()
        self._check(self.lib.wrnn_taco_stream_info(self._live(), C.byref(b), C.byref(tx), C.byref(it), C.byref(halo), C.byref(ws)))
        return dict(B=b.value, Tx_max=tx.value, max_iters=it.value, halo=halo.value, workspace_bytes=ws.value)

    def close(self):
        if getattr(self, '_st', None):
            self.lib.wrnn_taco_stream_close(self._st)
            self._st = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
