"""Wav conditioning without a device: the float64 restatement on inputs one can check by hand, the argument checks of the C entry
points and of the Python surface, the new command-line flags, and the condition on the fixtures that lets the GPU tests ask for exact
bounds (every frame of every clip at least 0.1 dB from the threshold)."""
import argparse

import numpy as np
import pytest

from tests import condition_ref as cr


# ---------------------------------------------------------------------------------------------------------------- the restatement
def test_all_zero_clip_is_kept_whole_and_unscaled():
    x = np.zeros(5000, np.float32)
    y, (start, end), peak = cr.condition(x, 25.0, 0.999)
    assert (start, end) == (0, 5000) and peak == 0 and y.shape == (5000,) and not y.any()


def test_single_sample_keeps_four_hops_around_it():
    """Sample i of the clip is sample i + 1024 of the padded one: frame f covers it when f 512 <= i + 1024 < f 512 + 2048, four frames; the
    kept span runs from the first of them times the hop to the hop after the last."""
    n, i = 20000, 7000
    x = np.zeros(n, np.float32)
    x[i] = 0.25
    e = cr.frame_energies(x)
    loud = np.flatnonzero(e > 0)
    assert loud.tolist() == [12, 13, 14, 15] and np.allclose(e[loud], 0.0625 / 2048, rtol=1e-15)
    start, end = cr.trim_bounds(x, 25.0)
    assert (start, end) == (12 * 512, 16 * 512) and end - start == 4 * 512 and start <= i < end
    y, _, peak = cr.condition(x, 25.0, 0.999)
    assert peak == np.float32(0.25) and y[i - start] == np.float32(0.25) / np.float32(0.25) * np.float32(0.999) and np.count_nonzero(y) == 1


def test_bounds_clamp_to_the_clip():
    n = 5000                                    # 10 frames
    x = np.zeros(n, np.float32)
    x[n - 1] = 0.5
    start, end = cr.trim_bounds(x, 25.0)
    assert end == n and (9 + 1) * 512 > n and start == 8 * 512   # padded sample 6023 lies in frames 8 .. 11, the clip has frames 0 .. 9


def test_reflection_reaches_frame_zero():
    x = np.zeros(4096, np.float32)
    x[1] = 0.5                                  # padded samples 1023 (its reflection) and 1025
    e = cr.frame_energies(x)
    assert e[0] == 2 * 0.25 / 2048 and cr.trim_bounds(x, 25.0)[0] == 0


def test_scale_is_float32_divide_then_multiply():
    x = np.array([0.1, -0.3, 0.7], np.float32)
    y = cr.scale(x, np.float32(0.7), 0.999)
    assert y.dtype == np.float32 and y[2] == np.float32(1.0) * np.float32(0.999)
    assert y[0] == np.float32(np.float32(0.1) / np.float32(0.7)) * np.float32(0.999)


def test_short_clip_is_refused():
    with pytest.raises(ValueError):
        cr.frame_energies(np.zeros(1024, np.float32))
    assert cr.frame_energies(np.zeros(1025, np.float32)).shape == (3,)


# ---------------------------------------------------------------------------------------------------------------- the fixtures
def test_every_fixture_frame_is_clear_of_the_threshold():
    cases = cr.cases()
    assert len(cases) >= 40
    for name, x, top_db, L, h in cases:
        assert cr.margin_db(x, top_db, L, h) >= cr.MIN_MARGIN_DB, name


def test_fixtures_trim_at_both_ends_at_either_and_not_at_all():
    seen = set()
    expect = {'mid': 'both', 'tail': 'start', 'head': 'end', 'full': 'none'}
    for name, x, top_db, L, h in cr.cases():
        n, where = x.shape[0], name.split('_')[1]
        kind = cr.trim_kind(x, top_db, L, h)
        if n >= 4096:
            assert kind == expect[where], (name, kind)
        seen.add((top_db, kind))
    assert seen >= {(d, k) for d in cr.TOP_DBS for k in ('both', 'start', 'end', 'none')}
    assert {x.shape[0] for _, x, _, _, _ in cr.cases()} >= set(cr.LENGTHS)
    assert {(L, h) for _, _, _, L, h in cr.cases()} == set(cr.WINDOWS)


# ---------------------------------------------------------------------------------------------------------------- the C entry points
def test_condition_frames():
    from tacotronv2_wavernn_chinese_amd import _cabi
    lib = _cabi.load_library()
    assert lib.wrnn_condition_frames(1025, 2048, 512) == 3 and lib.wrnn_condition_frames(5120, 2048, 512) == 11
    assert lib.wrnn_condition_frames(501, 1000, 300) == 2
    assert lib.wrnn_condition_frames(1024, 2048, 512) == _cabi.ERR_INVALID
    for L, h in ((1, 1), (8193, 512), (2048, 0), (2048, 2049), (-2, 1)):
        assert lib.wrnn_condition_frames(100000, L, h) == _cabi.ERR_INVALID, (L, h)
    assert _cabi.condition_frames(12345, 2048, 512) == 25
    with pytest.raises(ValueError):
        _cabi.condition_frames(1024, 2048, 512)


GOOD = dict(wav=8, n_max=5000, n=8, B=2, trim=1, top_db=25.0, L=2048, h=512, target=0.999, ws=8, F_max=10, out=8, n_out_max=5000, n_out=8,
            bounds=0, peak=0)


def _call(**kw):
    from tacotronv2_wavernn_chinese_amd import _cabi
    a = dict(GOOD, **kw)
    return _cabi.load_library().wrnn_condition(a['wav'] or None, a['n_max'], a['n'] or None, a['B'], a['trim'], a['top_db'], a['L'], a['h'], a['target'],
                                               a['ws'] or None, a['F_max'], a['out'] or None, a['n_out_max'], a['n_out'] or None, a['bounds'] or None,
                                               a['peak'] or None, None)


@pytest.mark.parametrize('bad', [dict(trim=0, target=0.0), dict(top_db=0.0), dict(top_db=-1.0), dict(top_db=float('nan')), dict(top_db=float('inf')),
                                 dict(L=1), dict(L=8193), dict(h=0), dict(h=2049), dict(target=-0.5), dict(target=float('nan')),
                                 dict(target=float('inf')), dict(B=0), dict(B=65536), dict(n_out_max=4999), dict(F_max=0), dict(n_max=0),
                                 dict(wav=0), dict(n=0), dict(ws=0), dict(out=0), dict(n_out=0)],
                         ids=lambda d: ','.join(f'{k}={v}' for k, v in d.items()))
def test_condition_refuses_bad_arguments_before_any_device_call(bad):
    """Every WRNN_ERR_INVALID arm: the pointers are not device pointers (8 is no address at all), so an arm that let the call through to a
    launch would not come back with -1."""
    from tacotronv2_wavernn_chinese_amd import _cabi
    assert _call(**bad) == _cabi.ERR_INVALID
    with pytest.raises(_cabi.WrnnError):
        a = dict(GOOD, **bad)
        _cabi.condition(a['wav'], a['n_max'], a['n'], a['B'], a['trim'], a['top_db'], a['L'], a['h'], a['target'], a['ws'], a['F_max'], a['out'],
                        a['n_out_max'], a['n_out'], a['bounds'], a['peak'], 0)


# ---------------------------------------------------------------------------------------------------------------- the Python surface
def test_condition_settings():
    from tacotronv2_wavernn_chinese_amd.frontend import condition_settings
    assert condition_settings() == (None, None) and condition_settings(None, False) == (None, None)
    assert condition_settings(25, True) == (25.0, 0.999) and condition_settings(10.5, 0.5) == (10.5, 0.5)
    for bad in (0, -3, float('nan'), float('inf'), 'loud', True):
        with pytest.raises(ValueError):
            condition_settings(trim_top_db=bad)
    for bad in (0.0, -1.0, float('nan'), float('inf'), 1e39, 'yes'):
        with pytest.raises(ValueError):
            condition_settings(peak_norm=bad)


def test_wav_conditioner_arguments():
    from tacotronv2_wavernn_chinese_amd.frontend import WavConditioner
    c = WavConditioner(trim_top_db=25, peak_norm=True)
    assert (c.trim_top_db, c.peak_target, c.frame_length, c.hop_length) == (25.0, 0.999, 2048, 512)
    assert c.frames(1025) == 3 and WavConditioner(peak_norm=0.5).peak_target == 0.5
    with pytest.raises(ValueError, match='nothing to do'):
        WavConditioner()
    for kw in (dict(trim_top_db=-1), dict(peak_norm=-1.0), dict(trim_top_db=25, frame_length=1), dict(trim_top_db=25, frame_length=16384),
               dict(trim_top_db=25, hop_length=0), dict(trim_top_db=25, frame_length=1024, hop_length=1025)):
        with pytest.raises(ValueError):
            WavConditioner(**kw)
    with pytest.raises(ValueError):
        c.frames(1024)
    with pytest.raises(ValueError, match='GPU only'):
        c.condition(np.zeros(4096, np.float32), device='cpu')
    with pytest.raises(ValueError):   # refused before any device work
        c.condition([np.zeros(4096, np.float32), np.zeros(1000, np.float32)], device='cuda')
    with pytest.raises(ValueError, match='contiguous float32'):
        c.condition_padded(np.zeros((1, 4096), np.float32), [4096])


def test_load_wav_and_from_wavs_check_the_settings_first(tmp_path):
    from scipy.io import wavfile
    from tacotronv2_wavernn_chinese_amd.dataset import DeviceCorpus
    from tacotronv2_wavernn_chinese_amd.frontend import load_wav
    path = tmp_path / 'a.wav'
    wavfile.write(str(path), 22050, (np.zeros(4096)).astype(np.int16))
    assert load_wav(path, 22050).shape == (4096,)            # the defaults: the file as it is, no device
    assert load_wav(path, 22050, trim_top_db=None, peak_norm=False).shape == (4096,)
    for kw in (dict(trim_top_db=0), dict(peak_norm=-0.1), dict(trim_top_db='x')):
        with pytest.raises(ValueError):
            load_wav(path, 22050, **kw)
        with pytest.raises(ValueError):
            DeviceCorpus.from_wavs([np.zeros(30000, np.float32)], None, 'cuda', **kw)
        with pytest.raises(ValueError):
            load_wav(tmp_path / 'missing.wav', 22050, **kw)  # the settings are checked before the file is opened


def test_generate_entries_check_the_settings_first():
    from tacotronv2_wavernn_chinese_amd.synth import DEFAULT_DIMS
    from tacotronv2_wavernn_chinese_amd.vocoder import WaveRNN
    model = WaveRNN(**DEFAULT_DIMS, mode='RAW')
    with pytest.raises(ValueError, match='trim_top_db'):
        model.generate_from_wav(np.zeros(8000, np.float32), None, False, 11000, 550, True, trim_top_db=-5)
    with pytest.raises(ValueError, match='peak_norm'):
        model.generate_many(wavs=[np.zeros(8000, np.float32)], peak_norm=-1.0)
    with pytest.raises(ValueError, match='wavs='):
        model.generate_many([np.zeros((80, 30), np.float32)], peak_norm=True)


# ---------------------------------------------------------------------------------------------------------------- the command lines
def test_flags_parse():
    from tacotronv2_wavernn_chinese_amd.frontend import add_condition_arguments, condition_arguments
    parser = argparse.ArgumentParser()
    add_condition_arguments(parser)
    assert condition_arguments(parser.parse_args([])) == dict(trim_top_db=None, peak_norm=None)
    assert condition_arguments(parser.parse_args(['--trim_silence'])) == dict(trim_top_db=25.0, peak_norm=None)
    assert condition_arguments(parser.parse_args(['--trim_top_db', '40'])) == dict(trim_top_db=None, peak_norm=None)
    assert condition_arguments(parser.parse_args(['--trim_silence', '--trim_top_db', '40', '--peak_norm'])) == dict(trim_top_db=40.0, peak_norm=0.999)
    assert condition_arguments(parser.parse_args(['--peak_norm', '0.9'])) == dict(trim_top_db=None, peak_norm=0.9)
    for bad in (['--trim_silence', '--trim_top_db', '0'], ['--peak_norm', '-1']):
        with pytest.raises(ValueError):
            condition_arguments(parser.parse_args(bad))


@pytest.mark.parametrize('main, argv', [('gen', ['--file', 'clip.wav']), ('train', ['--wav_dir', 'wavs']),
                                        ('dataset', ['--wav_dir', 'wavs', '--out_dir', 'out'])])
def test_every_cli_takes_the_flags(main, argv, monkeypatch):
    """Each main() parses the new flags and refuses a bad value before it configures anything (a ValueError from the flags, not argparse's
    exit for an unknown option)."""
    import importlib
    mod = importlib.import_module(f'tacotronv2_wavernn_chinese_amd.{main}')
    with pytest.raises(ValueError, match='trim_top_db'):
        mod.main(argv + ['--trim_silence', '--trim_top_db', '-3', '--peak_norm'])
    with pytest.raises(ValueError, match='peak_norm'):
        mod.main(argv + ['--trim_silence', '--peak_norm', '-0.5'])
    with pytest.raises(SystemExit):
        mod.main(argv + ['--peak_norm', 'loud'])
