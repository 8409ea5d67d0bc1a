"""The feature profiles of the mel front end without a GPU: the tables of a ``tacotron`` handle against the restatement
``tests/taco_mel_ref.py`` bit for bit, the frame counts per padding mode, every argument error of ``wrnn_mel_create_features`` (returned
before any device is touched), the ctypes mirror of ``wrnn_mel_features`` against the header, and the command lines."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import mel_ref as mr
from tests import taco_mel_ref as tm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_INVALID, ERR_UNSUPPORTED = -1, -7


def _fe(**kw):
    from tacotronv2_wavernn_chinese_amd.frontend import MelFrontEnd
    return MelFrontEnd(**kw)


def _check_tables(tab, basis64):
    rows, weights = mr.sparse_rows(basis64.astype(np.float32))
    np.testing.assert_array_equal(tab['rows'], rows)
    np.testing.assert_array_equal(tab['weights'].view(np.uint32), weights.view(np.uint32))
    np.testing.assert_array_equal(tab['window'].view(np.uint32), mr.window(1100).astype(np.float32).view(np.uint32))
    np.testing.assert_array_equal(tab['twiddle'].view(np.uint32), mr.twiddles(2048).astype(np.float32).view(np.uint32))
    return rows


def test_tables_of_both_profiles_equal_the_restatements_bit_for_bit():
    rows = _check_tables(_fe(features='tacotron').tables(), tm.mel_basis(22050, 2048, 80, 95.0, 7600.0))
    assert int((rows[:, 0] + rows[:, 1]).max()) - 1 == 705          # the last non-zero bin of 1025 at fmax = 7600
    for fe in (_fe(), _fe(features='vocoder')):
        rows = _check_tables(fe.tables(), mr.mel_basis(22050, 2048, 80, 95.0))
        assert int((rows[:, 0] + rows[:, 1]).max()) - 1 == 1023
    _check_tables(_fe(fmax=7600.0).tables(), tm.mel_basis(22050, 2048, 80, 95.0, 7600.0))   # the one switch alone
    _check_tables(_fe(features='tacotron', fmax=0).tables(), mr.mel_basis(22050, 2048, 80, 95.0))


def test_profiles_and_overrides():
    from tacotronv2_wavernn_chinese_amd.frontend import FEATURE_PROFILES
    assert FEATURE_PROFILES == dict(vocoder=tm.VOCODER, tacotron=tm.TACOTRON)
    fe = _fe(features='tacotron', preemph_rescale=0, n_mels=40)
    assert fe.features == 'tacotron' and fe.feature_config == dict(tm.TACOTRON, preemph_rescale=0) and fe.n_mels == 40
    assert _fe().features == 'vocoder' and _fe().feature_config == tm.VOCODER
    with pytest.raises(ValueError, match='features'):
        _fe(features='linear')
    with pytest.raises(ValueError, match='pad_mode'):
        _fe(pad_mode='edge')
    with pytest.raises(TypeError):
        _fe(features='tacotron', griffin_lim=True)


@pytest.mark.parametrize('n', [1, 274, 275, 1024])
def test_short_clips_have_frames_under_zero_padding_only(n):
    for zero in (_fe(features='tacotron'), _fe(pad_mode='zero')):
        assert zero.frames(n) == 1 + n // 275 == tm.frames(n, 2048, 275, 'zero')
    for reflect in (_fe(), _fe(features='tacotron', pad_mode='reflect')):
        with pytest.raises(ValueError, match='reflect'):
            reflect.frames(n)


def test_frame_counts_of_legal_clips_and_the_empty_clip():
    for fe in (_fe(), _fe(features='tacotron')):
        assert [fe.frames(n) for n in (1025, 2749, 2750, 110250)] == [4, 10, 11, 401]
        with pytest.raises(ValueError):
            fe.frames(0)


def _create(cfg_over=None, **feat_over):
    """``wrnn_mel_create_features`` on the reference configuration with fields moved -> (status, error text)."""
    from tacotronv2_wavernn_chinese_amd import _cabi
    lib = _cabi.load_library()
    cfg = dict(sample_rate=22050, n_fft=2048, hop_length=275, win_length=1100, n_mels=80, fmin=95.0, min_level_db=-100.0, device=0)
    cfg.update(cfg_over or {})
    c = _cabi.MelConfig(*[cfg[k] for k, _ in _cabi.MelConfig._fields_])
    size = feat_over.pop('struct_size', None)
    f = _cabi.MelFeatures(**dict(tm.TACOTRON, pad_mode=_cabi.MEL_PAD_MODES['zero'], **feat_over) if 'pad_mode' not in feat_over else
                          dict(tm.TACOTRON, **feat_over))
    if size is not None:
        f.struct_size = size
    h = C.c_void_p()
    rc = lib.wrnn_mel_create_features(C.byref(c), C.byref(f), C.byref(h))
    msg = lib.wrnn_mel_last_error(h).decode() if h else ''
    lib.wrnn_mel_destroy(h)
    return rc, msg


@pytest.mark.parametrize('over', [dict(magnitude_power=0), dict(magnitude_power=3), dict(fmax=95.0), dict(fmax=50.0), dict(fmax=11025.5),
                                  dict(fmax=-1.0), dict(fmax=float('nan')), dict(preemphasis=-0.1), dict(preemph_rescale=-0.999),
                                  dict(max_abs_value=-4.0), dict(preemphasis=float('nan')), dict(pad_mode=2), dict(pad_mode=-1),
                                  dict(ref_level_db=float('inf')), dict(struct_size=28), dict(struct_size=36), dict(struct_size=0)])
def test_argument_errors_come_back_without_a_device(over):
    rc, msg = _create(**over)
    assert rc == ERR_INVALID and msg, (over, rc, msg)


def test_what_the_create_entry_accepts_and_what_stays_unsupported():
    assert _create()[0] == 0
    assert _create(fmax=11025.0)[0] == 0 and _create(fmax=0.0)[0] == 0            # the closed upper end; 0 = sample_rate / 2
    assert _create(preemphasis=0.0, preemph_rescale=0.0, max_abs_value=0.0, ref_level_db=-3.0)[0] == 0
    assert _create(dict(n_fft=1024))[0] == ERR_UNSUPPORTED                          # not lifted by a profile
    assert _create(dict(n_mels=129))[0] == ERR_INVALID and _create(dict(fmin=8000.0))[0] == ERR_INVALID   # fmin >= fmax = 7600
    with pytest.raises(ValueError, match='UNSUPPORTED|n_fft'):
        _fe(features='tacotron', n_fft=1024)
    with pytest.raises(ValueError):
        _fe(features='tacotron', magnitude_power=3)
    from tacotronv2_wavernn_chinese_amd import _cabi
    lib = _cabi.load_library()
    h = C.c_void_p()
    assert lib.wrnn_mel_create_features(None, None, C.byref(h)) == ERR_INVALID and not h


def test_ctypes_features_struct_matches_the_header_layout(tmp_path):
    from tacotronv2_wavernn_chinese_amd import _cabi
    st = _cabi.MelFeatures
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{ROOT}/include/wavernn_amd.h"', 'int main(void) {',
             '  printf("size %zu\\n", sizeof(wrnn_mel_features));']
    lines += [f'  printf("{name} %zu\\n", offsetof(wrnn_mel_features, {name}));' for name, _ in st._fields_]
    lines += ['  printf("reflect %d\\n", WRNN_MEL_PAD_REFLECT);', '  printf("zero %d\\n", WRNN_MEL_PAD_ZERO);', '  return 0;', '}']
    (tmp_path / 'layout.c').write_text('\n'.join(lines))
    subprocess.check_call(['gcc', '-std=c11', '-o', str(tmp_path / 'layout'), str(tmp_path / 'layout.c')])
    got = dict(l.split() for l in subprocess.check_output([str(tmp_path / 'layout')], text=True).splitlines())
    assert int(got['size']) == C.sizeof(st) == _cabi.MelFeatures().struct_size
    for name, _ in st._fields_:
        assert int(got[name]) == getattr(st, name).offset, name
    assert {k: int(got[k]) for k in ('reflect', 'zero')} == _cabi.MEL_PAD_MODES
    d = _cabi.MelFeatures()                                                         # a fresh one is the default profile
    assert (d.pad_mode, d.magnitude_power, d.fmax, d.ref_level_db, d.preemphasis, d.preemph_rescale, d.max_abs_value) == (0, 1, 0, 0, 0, 0, 0)


def test_command_lines_take_the_features_flag():
    from tacotronv2_wavernn_chinese_amd import dataset, gen, train
    parsers = {'gen': (gen.build_parser(), ['--file', 'clip.wav']), 'preprocess': (dataset.build_parser(), ['--wav_dir', 'a', '--out_dir', 'b']),
               'train': (train.build_parser(), ['--wav_dir', 'a'])}
    for name, (parser, base) in parsers.items():
        assert parser.parse_args(base).features == 'vocoder', name
        args = parser.parse_args(base + ['--features', 'tacotron'])
        assert args.features == 'tacotron' and not args.trim_silence and args.peak_norm is None, name     # independent of the conditioning
        args = parser.parse_args(base + ['--features', 'tacotron', '--trim_silence', '--peak_norm'])
        assert (args.features, args.trim_silence, args.peak_norm) == ('tacotron', True, 0.999), name
        with pytest.raises(SystemExit):
            parser.parse_args(base + ['--features', 'linear'])
        assert '--features tacotron --trim_silence --peak_norm' in ' '.join(parser.format_help().split()), name   # the reference's recipe


def test_saved_features_are_read_back_and_a_mismatch_is_named(tmp_path):
    from tacotronv2_wavernn_chinese_amd import dataset as D
    listing = tmp_path / D.LIST_NAME
    listing.write_text('')
    assert D.saved_features(listing) == 'vocoder'                                   # a corpus saved before the profiles
    D.check_saved_features(listing, 'vocoder')
    with pytest.raises(ValueError, match="holds 'vocoder' mel features, 'tacotron' were asked for"):
        D.check_saved_features(listing, 'tacotron')
    (tmp_path / D.FEATURES_NAME).write_text('tacotron\n')
    assert D.saved_features(listing) == 'tacotron'
    D.check_saved_features(listing, 'tacotron')
    with pytest.raises(ValueError, match="holds 'tacotron' mel features, 'vocoder' were asked for"):
        D.check_saved_features(listing, 'vocoder')


def test_train_cli_refuses_a_saved_corpus_of_other_features(tmp_path):
    """``wavernn_train.py`` on a corpus saved with ``--features tacotron``, asked for the default features: a message, before any device
    work (so it runs here)."""
    from tacotronv2_wavernn_chinese_amd import dataset as D
    from tacotronv2_wavernn_chinese_amd.hparams import DEFAULT_HPARAMS
    (tmp_path / D.LIST_NAME).write_text('')
    (tmp_path / D.FEATURES_NAME).write_text('tacotron\n')
    hp_file = tmp_path / 'hp.py'
    hp_file.write_text(open(DEFAULT_HPARAMS).read() + f'\nfeature_path = {str(tmp_path / D.LIST_NAME)!r}\n')
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'wavernn_train.py'), '--hp_file', str(hp_file)], cwd=tmp_path, capture_output=True,
                       text=True, timeout=300)
    assert r.returncode != 0 and "holds 'tacotron' mel features, 'vocoder' were asked for" in r.stderr, r.stderr[-2000:]
