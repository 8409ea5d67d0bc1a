"""CPU side of the spectral scores: analytic pins of the restatement ``tests/score_ref.py``, the host tables of ``csrc/score.hip``
against it, every refusal of ``wrnn_score_create`` / ``SpectralScore`` (none needs a device), the header against the binding, and the
command line's argument handling."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from tests import mel_ref as mr
from tests import score_ref as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RES = ((256, 64, 256), (1024, 100, 601), (2048, 240, 1200))
MEL = dict(sample_rate=22050, n_fft=2048, hop_length=275, win_length=1100, n_mels=80, fmin=95.0, min_level_db=-100.0)


# ---- the restatement ------------------------------------------------------------------------------------------------------------------

def _all_zero(s):
    assert s['mel_lsd_db'] == s['mcd_db'] == s['mr_sc'] == s['mr_logmag'] == 0.0
    assert not s['lsd'].any() and not s['mcd'].any()
    for r in s['stft']:
        assert r['sc'] == 0.0 and r['logmag'] == 0.0 and not r['num'].any() and not r['lm'].any() and (r['den'] > 0).all()


@pytest.mark.parametrize('dtype', [np.float64, np.float32])
def test_identical_clips_and_two_silences_are_exactly_zero(dtype):
    a = sr.parity_pair('scaled', 3000)[0]
    _all_zero(sr.score(a, a.copy(), RES, dtype=dtype))
    z = sr.score(np.zeros(2500, np.float32), np.zeros(2600, np.float32), RES, dtype=dtype)
    _all_zero(z)
    assert z['n'] == 2500
    for r in z['stft']:     # both sides sit at the floor
        np.testing.assert_allclose(r['den'], (r['n_fft'] // 2 + 1) * sr.MAG_FLOOR, rtol=1e-6)


def test_a_gain_moves_every_score_by_what_the_formulas_say():
    """b = g a on a broadband clip, no bin and no mel at a clip: sc = |1 - g|, logmag = |ln g|, lsd_t = 20 |log10 g|, and mcd_t = 0 up
    to rounding (a constant offset of the log-mel has no cepstrum above c0)."""
    a = mr.white(6000, 0.1, 3)
    for g in (0.5, 1.25):
        s = sr.score(a, (g * a.astype(np.float64)).astype(np.float32), RES)
        db = 20.0 * abs(np.log10(g))
        mel = sr.mel(a)
        assert mel.min() > db / 100.0 + 1e-3 and mel.max() < 1.0 - db / 100.0 - 1e-3     # the open range on both sides
        np.testing.assert_allclose(s['lsd'], db, rtol=1e-6)
        assert np.abs(s['mcd']).max() < 1e-5 * db
        for r in s['stft']:
            assert abs(r['sc'] - abs(1.0 - g)) < 1e-6 and abs(r['logmag'] - abs(np.log(g))) < 1e-6
        assert abs(s['mr_sc'] - abs(1.0 - g)) < 1e-6 and abs(s['mel_lsd_db'] - db) < 1e-5


def test_dct_rows_are_orthonormal_and_blind_to_a_constant():
    for n_mels, K in ((80, 13), (40, 39), (128, 127), (2, 1)):
        Cm = sr.dct_matrix(n_mels, K)
        np.testing.assert_allclose(Cm @ Cm.T, np.eye(K), atol=1e-12)
        assert np.abs(Cm @ np.ones(n_mels)).max() < 1e-12


def test_summaries_are_the_formulas_on_the_per_frame_values():
    a, b = sr.parity_pair('noise', 3000)
    s = sr.score(a, b, RES)
    assert s['mel_lsd_db'] == s['lsd'].mean() and s['mcd_db'] == s['mcd'].mean()
    for (n_fft, hop, win), r in zip(RES, s['stft']):
        A, B = sr.magnitudes(a, n_fft, hop, win), sr.magnitudes(b, n_fft, hop, win)
        assert A.shape == (n_fft // 2 + 1, 1 + 3000 // hop) == (n_fft // 2 + 1, r['frames'])
        np.testing.assert_allclose(r['sc'], np.linalg.norm(B - A) / np.linalg.norm(A), rtol=1e-12)
        np.testing.assert_allclose(r['logmag'], np.abs(np.log(A) - np.log(B)).mean(), rtol=1e-12)
    np.testing.assert_allclose(s['mr_sc'], np.mean([r['sc'] for r in s['stft']]), rtol=1e-15)
    with pytest.raises(ValueError):
        sr.score(a[:1024], b, RES)
    assert sr.min_samples(RES[:2], pad_mode='zero') == 513 and sr.min_samples(RES[:2]) == 1025


def test_mu_law_round_trip_moves_a_sample_by_less_than_a_class():
    y = np.linspace(-1, 1, 4001)
    x = sr.mu_law_round_trip(y)
    # half a class of 2 / mu in the companded domain, through the expansion's slope ln(1 + mu) (|y| + 1 / mu)
    half = np.log(1024.0) * (np.abs(y) + 1.0 / 1023.0) / 1023.0
    assert (np.abs(x - y) <= 1.01 * half + 1e-7).all() and np.abs(x - y).max() > 0.003 and x.dtype == np.float32


# ---- the library's host side -------------------------------------------------------------------------------------------------------------

def _native(score=None, features=None, **cfg):
    from tacotronv2_wavernn_chinese_amd import _cabi
    return _cabi.NativeScore(**dict(MEL, **cfg), features=features, score=score)


def test_tables_are_the_restatements_rounded_once():
    from tacotronv2_wavernn_chinese_amd import _cabi
    nat = _native(_cabi.ScoreConfig(RES + ((512, 50, 240),), mcd_order=39), n_mels=40)
    t = nat.tables()
    assert nat.resolutions == list(RES) + [(512, 50, 240)]
    for (n_fft, _, win), w, tw in zip(nat.resolutions, t['windows'], t['twiddles']):
        np.testing.assert_array_equal(w, mr.window(win).astype(np.float32))
        np.testing.assert_array_equal(tw, mr.twiddles(n_fft).astype(np.float32))
    assert t['dct'].shape == (39, 40)
    np.testing.assert_allclose(t['dct'], sr.dct_matrix(40, 39), atol=6e-8, rtol=0)   # half an ulp at 1: cos of another libm
    assert np.abs(t['dct'].astype(np.float64) @ t['dct'].astype(np.float64).T - np.eye(39)).max() < 1e-6


def test_frames_and_the_row_layout():
    nat = _native()
    assert nat.min_samples == 1025 and nat.n_res == 3
    assert [nat.frames(r, 22050) for r in (-1, 0, 1, 2)] == [81, 442, 184, 92]
    for bad in (1024, 0, -1, 2 ** 31):
        with pytest.raises(ValueError):
            nat.frames(0, bad)
    for r in (-2, 3):
        with pytest.raises(ValueError):
            nat.frames(r, 22050)
    segs, stride = nat.layout(22050)
    assert [s[0] for s in segs] == ['lsd', 'mcd'] + ['num', 'den', 'lm'] * 3 and stride == 2 * 81 + 3 * (442 + 184 + 92)
    assert [s[2] for s in segs] == list(np.cumsum([0] + [s[3] for s in segs[:-1]]))
    from tacotronv2_wavernn_chinese_amd import _cabi
    # zero padding lifts the front end's own limit; the transforms keep theirs
    zero = _native(_cabi.ScoreConfig(((256, 64, 256), (512, 50, 240))), _cabi.MelFeatures(pad_mode=_cabi.MEL_PAD_MODES['zero']))
    assert zero.min_samples == 257 and zero.frames(-1, 257) == 1 and zero.frames(0, 257) == 5
    with pytest.raises(ValueError):
        zero.frames(0, 256)


def test_create_refuses_what_the_definitions_exclude():
    from tacotronv2_wavernn_chinese_amd import _cabi
    S = _cabi.ScoreConfig
    cases = [
        (dict(score=S(())), 'n_res'),
        (dict(score=S(((500, 50, 240),))), 'n_fft'),
        (dict(score=S(((4096, 50, 240),))), 'n_fft'),
        (dict(score=S(((512, 50, 513),))), 'win'),
        (dict(score=S(((512, 50, 0),))), 'win'),
        (dict(score=S(((512, 0, 240),))), 'hop'),
        (dict(score=S(mag_floor=0.0)), 'mag_floor'),
        (dict(score=S(mag_floor=-1e-7)), 'mag_floor'),
        (dict(score=S(mag_floor=float('nan'))), 'mag_floor'),
        (dict(score=S(mag_floor=float('inf'))), 'mag_floor'),
        (dict(score=S(mcd_order=0)), 'mcd_order'),
        (dict(score=S(mcd_order=80)), 'mcd_order'),
        (dict(score=S(mcd_order=13), n_mels=13), 'mcd_order'),
        (dict(n_fft=1024), 'n_fft'),                                   # the front end's own refusals come through
        (dict(n_mels=129), 'n_mels'),
        (dict(hop_length=0), 'hop_length'),
        (dict(features=_cabi.MelFeatures(magnitude_power=3)), 'magnitude_power'),
    ]
    for kw, word in cases:
        with pytest.raises(ValueError, match=word):
            _native(**kw)
    bad = S()
    bad.struct_size -= 4
    with pytest.raises(ValueError, match='struct_size'):
        _native(bad)
    feat = _cabi.MelFeatures()
    feat.struct_size += 4
    with pytest.raises(ValueError, match='struct_size'):
        _native(features=feat)
    with pytest.raises(ValueError):
        S(((512, 50),))
    with pytest.raises(ValueError):
        S(((512, 50, 240),) * 5)
    # the C entries on a refused and on a null handle
    lib = _cabi.load_library()
    h = C.c_void_p()
    cfg = _cabi.MelConfig(22050, 2048, 275, 1100, 80, 95.0, -100.0, 0)
    assert lib.wrnn_score_create(C.byref(cfg), None, C.byref(S(mcd_order=0)), C.byref(h)) == _cabi.ERR_INVALID and h
    assert b'mcd_order' in lib.wrnn_score_last_error(h)
    assert lib.wrnn_score_frames(h, 0, 22050) == _cabi.ERR_INVALID and lib.wrnn_score_tables(h, 0, None, None, None) == _cabi.ERR_INVALID
    assert lib.wrnn_score(h, 1, 1, 22050, 1, 1, 1, None, 0, None) == _cabi.ERR_STATE
    lib.wrnn_score_destroy(h)
    assert lib.wrnn_score_create(None, None, None, None) == _cabi.ERR_INVALID
    assert lib.wrnn_score(None, 1, 1, 22050, 1, 1, 1, None, 0, None) == _cabi.ERR_INVALID
    lib.wrnn_score_destroy(None)
    # argument checks of the launch entry precede every device call
    nat = _native()
    for args in ((0, 1, 22050, 1, 1, 1, 0, 0), (1, 1, 1024, 1, 1, 1, 0, 0), (1, 1, 22050, 1, 0, 1, 0, 0), (1, 1, 22050, 1, 65536, 1, 0, 0),
                 (1, 1, 22050, 1, 1, 0, 0, 0), (1, 1, 22050, 1, 1, 1, 1, nat.layout(22050)[1] - 1)):
        with pytest.raises(_cabi.WrnnError) as e:
            nat.score(*args, 0)
        assert e.value.code == _cabi.ERR_INVALID


def test_spectral_score_refuses_without_a_device():
    from tacotronv2_wavernn_chinese_amd.frontend import SpectralScore
    sc = SpectralScore()
    assert sc.resolutions == [(512, 50, 240), (1024, 120, 600), (2048, 240, 1200)] and sc.min_samples == 1025 and sc.mcd_order == 13
    assert sc.frames(-1, 22050) == 81 and sc.tables()['dct'].shape == (13, 80)
    assert SpectralScore(features='tacotron', resolutions=((256, 64, 256),)).min_samples == 129
    for kw in (dict(resolutions=((300, 50, 240),)), dict(resolutions=()), dict(resolutions=((512, 50, 240),) * 5), dict(mcd_order=80),
               dict(mag_floor=0), dict(features='linear'), dict(n_fft=1024), dict(n_mels=13)):
        with pytest.raises(ValueError):
            SpectralScore(**kw)
    with pytest.raises(TypeError):
        SpectralScore(n_iter=3)
    ok = mr.white(3000, 0.1)
    for a, b in ((ok, ok[:1024]), ([ok, ok], [ok]), ([], []), (ok.reshape(2, 1500), ok)):
        with pytest.raises(ValueError):
            sc.score(a, b)
    with pytest.raises(ValueError, match='GPU only'):
        sc.score(ok, ok, device='cpu')


# ---- the boundary ------------------------------------------------------------------------------------------------------------------------

def test_header_binding_and_library_agree_on_the_score_entries(tmp_path):
    from tacotronv2_wavernn_chinese_amd import _cabi
    hdr = open(os.path.join(ROOT, 'include', 'wavernn_amd.h')).read()
    declared = sorted(s for s in set(re.findall(r'\b(wrnn_[a-z_]+)\s*\(', hdr)) if s.startswith('wrnn_score'))
    assert declared == sorted(s for s in _cabi.EXPORTED_SYMBOLS if s.startswith('wrnn_score'))
    assert declared == ['wrnn_score', 'wrnn_score_create', 'wrnn_score_destroy', 'wrnn_score_frames', 'wrnn_score_last_error', 'wrnn_score_tables']
    lib = _cabi.load_library()
    assert all(hasattr(lib, s) for s in declared)
    assert int(re.search(r'#define WRNN_ABI_VERSION (\d+)', hdr).group(1)) == 9 == lib.wrnn_abi_version()     # new entries, the old number
    macros = {m: int(v) for m, v in re.findall(r'#define (WRNN_SCORE_[A-Z0-9_]+) (\d+)', hdr)}
    assert macros['WRNN_SCORE_MAX_RES'] == _cabi.SCORE_MAX_RES and macros['WRNN_SCORE_FIELDS'] == _cabi.SCORE_FIELDS == len(_cabi.SCORE_FIELD_NAMES)
    order = dict(mel_lsd_db='MEL_LSD_DB', mcd_db='MCD_DB', mr_sc='MR_SC', mr_logmag='MR_LOGMAG', sc0='SC0', logmag0='LOGMAG0')
    for name, macro in order.items():
        assert _cabi.SCORE_FIELD_NAMES.index(name) == macros['WRNN_SCORE_' + macro]
    st = _cabi.ScoreConfig
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{ROOT}/include/wavernn_amd.h"', 'int main(void) {',
             '  printf("size %zu\\n", sizeof(wrnn_score_config));']
    lines += [f'  printf("{f} %zu\\n", offsetof(wrnn_score_config, {f}));' for f, _ in st._fields_]
    lines += ['  return 0;', '}']
    (tmp_path / 'layout.c').write_text('\n'.join(lines))
    subprocess.check_call(['gcc', '-std=c11', '-o', str(tmp_path / 'layout'), str(tmp_path / 'layout.c')])
    got = dict(l.split() for l in subprocess.check_output([str(tmp_path / 'layout')], text=True).splitlines())
    assert int(got['size']) == C.sizeof(st)
    for f, _ in st._fields_:
        assert int(got[f]) == getattr(st, f).offset, f


# ---- the command line ----------------------------------------------------------------------------------------------------------------------

def test_cli_arguments(tmp_path):
    from tacotronv2_wavernn_chinese_amd import score as cli
    p = cli.build_parser()
    a = p.parse_args(['--target', 'a.wav', '--test', 'b.wav'])
    assert (a.features, a.resample, a.json, a.per_frame) == ('vocoder', False, False, None)
    assert [(n, str(x), str(y)) for n, x, y in cli.pair_files(a)] == [('b', 'a.wav', 'b.wav')]
    a = p.parse_args(['--target', 'a.wav', '--test', 'b.wav', '--features', 'tacotron', '--resample', '--json', '--per_frame', 'o.npz'])
    assert (a.features, a.resample, a.json, a.per_frame) == ('tacotron', True, True, 'o.npz')
    with pytest.raises(SystemExit):
        p.parse_args(['--target', 'a.wav', '--test', 'b.wav', '--features', 'linear'])
    for name in ('x', 'y'):
        for d in ('t', 'g'):
            (tmp_path / d).mkdir(exist_ok=True)
            (tmp_path / d / f'{name}.wav').write_bytes(b'')
    a = p.parse_args(['--target_dir', str(tmp_path / 't'), '--test_dir', str(tmp_path / 'g')])
    assert [(n, x.parent.name, y.parent.name) for n, x, y in cli.pair_files(a)] == [('x', 't', 'g'), ('y', 't', 'g')]
    (tmp_path / 'g' / 'z.wav').write_bytes(b'')
    with pytest.raises(ValueError, match="'z'"):
        cli.pair_files(a)
    (tmp_path / 'empty').mkdir()
    for argv in (['--target', 'a.wav'], ['--target', 'a.wav', '--test_dir', 'd'], ['--target', 'a.wav', '--test', 'b.wav', '--target_dir', 'd'], [],
                 ['--target_dir', str(tmp_path / 'empty'), '--test_dir', str(tmp_path / 'empty')]):
        with pytest.raises(ValueError):
            cli.pair_files(p.parse_args(argv))
    with pytest.raises(SystemExit):          # main reports them as usage errors, before anything touches a device
        cli.main(['--target', 'a.wav'])
    assert os.path.exists(os.path.join(ROOT, 'wavernn_score.py'))
