"""CPU side of the pitch tracker: analytic pins of the restatement ``tests/pitch_ref.py``, the margins of every fixture frame (what lets
``tests/test_gpu_pitch.py`` demand equal decisions), every refusal of ``wrnn_pitch_create`` and the Python wrappers (none needs a
device), the host-only entries against their formulas, the header against the binding, and the command line's argument handling."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

from tests import pitch_ref as pr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = pr.N


# ---- the restatement ------------------------------------------------------------------------------------------------------------------

def _interior(tr):
    return slice(6, len(tr['f0']) - 6)


@pytest.mark.parametrize('name, cents, aperiodicity', [('sine_60.5', 0.004, 4e-5), ('sine_100', 0.006, 1.1e-4), ('sine_220.5', 0.1, 1e-20),
                                                       ('sine_233.3', 0.04, 2e-6), ('sine_441', 0.4, 1e-20), ('sine_595', 0.7, 6e-5)])
def test_sines_track_their_frequency(name, cents, aperiodicity):
    """The bounds sit just above what a 40-line YIN gives at the defaults on these tones (0.003 .. 0.65 cents)."""
    tr = pr.case_track('default', name, N)
    i = _interior(tr)
    assert tr['voiced'][i].all()
    assert np.abs(1200 * np.log2(tr['f0_64'][i] / float(name[5:]))).max() < cents and tr['aperiodicity_64'][i].max() < aperiodicity


def test_harmonic_complexes_noise_silence_and_dc():
    c = pr.case_track('default', 'complex_110', N)       # a second harmonic of 5 x the power does not pull the track an octave up
    assert c['voiced'][_interior(c)].all() and np.abs(c['f0_64'][_interior(c)] - 110.0).max() < 0.05
    m = pr.case_track('default', 'missing_150', N)       # 300 / 450 / 600 Hz: the period is the missing fundamental's
    assert m['voiced'][_interior(m)].all() and np.abs(m['f0_64'][_interior(m)] - 150.0).max() < 0.05
    noise = pr.case_track('default', 'noise', N)
    assert not noise['voiced'].any() and noise['aperiodicity_64'].min() > 0.8 and not noise['f0'].any()
    for name in ('zeros', 'dc'):
        z = pr.case_track('default', name, N)
        assert not z['voiced'].any() and (z['aperiodicity_64'][_interior(z)] == 1.0).all()
    assert (pr.case_track('default', 'zeros', N)['rms'] == 0).all() and (pr.case_track('default', 'zeros', N)['aperiodicity'] == 1).all()
    sn = pr.case_track('default', 'sine_noise', N)
    assert sn['voiced'][_interior(sn)].all() and np.abs(1200 * np.log2(sn['f0_64'][_interior(sn)] / 200.0)).max() < 15.0
    stop = pr.case_track('default', 'stop_3100', N)       # the tone ends at sample 3100: voiced well before, unvoiced well after
    assert stop['voiced'][3:8].all() and not stop['voiced'][16:].any()
    quiet = pr.track(pr.sine(200.0, N, amp=5e-5))          # a clean tone under silence_rms has a candidate and is unvoiced
    assert (quiet['tau'][_interior(quiet)] == 110).all() and not quiet['voiced'].any() and not quiet['f0'].any()


def test_frames_zero_padding_and_the_cmnd_definition():
    assert [pr.frames_of(n, 275) for n in (0, 1, 274, 275, 276, 6000)] == [0, 1, 1, 2, 2, 22]
    assert pr.lags(22050, 60.0, 600.0) == (37, 367) and pr.lags(16000, 80.0, 600.0) == (27, 200) and pr.lags(22050, 220.0, 220.5) == (100, 100)
    d = np.array([0.0, 0.0, 0.0, 2.0, 1.0, 5.0])
    np.testing.assert_array_equal(pr.cmnd(d), [1.0, 1.0, 1.0, 2.0 * 3 / 2.0, 1.0 * 4 / 3.0, 5.0 * 5 / 8.0])   # 1 while the running sum is exactly 0
    x = np.random.default_rng(0).standard_normal(300)
    np.testing.assert_allclose(pr.difference(x, 100, 150)[[0, 7, 150]], [0.0, ((x[:100] - x[7:107]) ** 2).sum(), ((x[:100] - x[150:250]) ** 2).sum()], rtol=1e-14)
    # frame t starts at t hop - frame_length / 2 and reads zeros outside the clip: one impulse at sample 0 is x[1024] of frame 0 alone
    one = pr.track(np.array([1.0], np.float32))
    assert len(one['f0']) == 1 and one['rms'][0] == 0.0 and not one['voiced'][0] and one['aperiodicity_64'][0] == 1.0
    # a clip and the same clip followed by zeros agree on the frames they share, as far as the window and the lags reach into the clip
    a, b = pr.case_track('default', 'stop_3100', N), pr.track(pr.signal('stop_3100', N)[:3100])
    np.testing.assert_array_equal(a['f0_64'][:12], b['f0_64'])


def test_pair_scores_follow_their_formulas():
    f = np.float32
    ft = np.array([100, 100, 0, 200, 0, 150], f)
    fs = np.array([100, 125, 0, 0, 300, 75], f)
    s = pr.pair_scores(ft, fs)
    cents = 1200 * np.log2(np.array([1.0, 1.25, 0.5]))
    assert s['voiced_target'] == 4 and s['voiced_test'] == 4 and s['voiced_both'] == 3
    assert s['f0_rmse_cents'] == pytest.approx(math.sqrt((cents ** 2).mean()), rel=1e-14)
    assert s['gpe'] == 2 / 3 and s['vde'] == 2 / 6 and s['ffe'] == 4 / 6
    assert s['f0_corr'] == pytest.approx(np.corrcoef(np.log2([100, 100, 150]), np.log2([100, 125, 75]))[0, 1], rel=1e-12)
    np.testing.assert_allclose(s['cents'], [0, cents[1], 0, 0, 0, cents[2]], rtol=1e-14)
    assert s['m_gpe'] == pytest.approx(0.05)
    same = pr.pair_scores(ft, ft.copy())
    assert same['f0_rmse_cents'] == same['gpe'] == same['vde'] == same['ffe'] == 0.0 and same['f0_corr'] == 1.0
    z = np.zeros(5, f)
    assert all(pr.pair_scores(z, z)[k] == 0 for k in pr.FIELDS)                     # two silences
    none = pr.pair_scores(ft, np.where(ft > 0, 0, 100).astype(f))                   # V is empty: vde 1, nothing to rate
    assert none['vde'] == none['ffe'] == 1.0 and none['f0_rmse_cents'] == none['gpe'] == none['f0_corr'] == 0.0
    single = pr.pair_scores(np.array([100, 0], f), np.array([110, 0], f))           # #V < 2: no correlation
    assert single['f0_corr'] == 0.0 and single['f0_rmse_cents'] > 0
    flat = pr.pair_scores(np.array([100, 100], f), np.array([110, 120], f))         # a variance of 0: no correlation
    assert flat['f0_corr'] == 0.0
    assert all(pr.pair_scores(z[:0], z[:0])[k] == 0 for k in pr.FIELDS)             # n = 0: no frames, an all-zero row


def test_every_fixture_frame_decides_with_a_margin():
    """Conditions, not tolerances: a fixture that misses one gets another seed or frequency, so the share of excused frames is 0."""
    cases = list(pr.CASES) + [('default', name, N) for pair in pr.PAIRS for name in pair]
    frames = 0
    for config, name, n in cases:
        tr = pr.case_track(config, name, n)
        assert len(tr['f0']) == pr.frames_of(n, tr['settings']['hop'])
        pr.check_margins(tr)
        frames += len(tr['f0'])
    assert frames > 1500
    for a, b in pr.PAIRS:
        s = pr.pair_scores(pr.case_track('default', a, N)['f0'], pr.case_track('default', b, N)['f0'])
        assert s['m_gpe'] >= 1e-6
        if a != b and s['f0_corr'] != 0:
            assert s['voiced_both'] >= 2
    # every listed length and every config is in the cases
    assert {n for c, _, n in pr.CASES if c == 'default'} >= set(pr.LENGTHS) and {c for c, _, _ in pr.CASES} == set(pr.CONFIGS)
    for c in pr.CONFIGS.values():
        s = dict(pr.DEFAULTS, **c)
        assert s['window'] + pr.lags(s['sample_rate'], s['fmin'], s['fmax'])[1] + 1 <= s['frame_length']
    s = dict(pr.DEFAULTS, **pr.CONFIGS['edge'])
    assert s['frame_length'] - (s['window'] + pr.lags(22050, s['fmin'], s['fmax'])[1] + 1) == 3


def test_the_pairs_score_what_they_were_built_for():
    def score(a, b):
        return pr.pair_scores(pr.case_track('default', a, N)['f0'], pr.case_track('default', b, N)['f0'])
    T = pr.frames_of(N, 275)
    detuned = score('chirp', 'chirp_x%r' % (2 ** (10 / 1200)))
    assert abs(detuned['f0_rmse_cents'] - 10.0) < 0.1 and detuned['gpe'] == 0 and detuned['f0_corr'] > 0.9999
    gross = score('chirp', 'chirp_x1.3')
    assert gross['gpe'] == 1.0 and abs(gross['f0_rmse_cents'] - 1200 * math.log2(1.3)) < 5.0     # all gross errors
    vs_noise = score('chirp', 'noise')
    assert vs_noise['vde'] == vs_noise['voiced_target'] / T and vs_noise['voiced_both'] == 0
    switch = score('chirpstop_3100', 'chirpstop_4200')
    assert switch['vde'] == 4 / T and switch['voiced_both'] == switch['voiced_target']


# ---- the library's host side -------------------------------------------------------------------------------------------------------------

def _create(**kw):
    """wrnn_pitch_create on a config with ``kw`` over the defaults -> (status, error text); the handle is destroyed."""
    from tacotronv2_wavernn_chinese_amd import _cabi
    lib = _cabi.load_library()
    cfg = _cabi.PitchConfig()
    for k, v in kw.items():
        setattr(cfg, k, v)
    h = C.c_void_p()
    rc = lib.wrnn_pitch_create(C.byref(cfg), C.byref(h))
    assert h, 'a refused handle is still returned'
    msg = lib.wrnn_pitch_last_error(h).decode()
    lib.wrnn_pitch_destroy(h)
    return rc, msg


def test_create_refuses_what_the_definitions_exclude():
    from tacotronv2_wavernn_chinese_amd import _cabi
    inf, nan = float('inf'), float('nan')
    invalid = [
        (dict(struct_size=C.sizeof(_cabi.PitchConfig) - 8), 'struct_size'), (dict(struct_size=C.sizeof(_cabi.PitchConfig) + 8), 'struct_size'),
        (dict(sample_rate=0), 'sample_rate'), (dict(sample_rate=-22050), 'sample_rate'), (dict(hop=0), 'hop'), (dict(hop=-1), 'hop'),
        (dict(fmin=nan), 'fmin'), (dict(fmax=nan), 'fmax'), (dict(fmax=inf), 'fmax'), (dict(fmin=-inf), 'fmin'),
        (dict(fmin=600.0), 'fmin < fmax'), (dict(fmin=700.0), 'fmin < fmax'),
        (dict(fmin=-10.0, fmax=-5.0), 'tau_min'),                       # tau_min = ceil(sample_rate / fmax) < 1
        (dict(fmin=220.6, fmax=220.9), 'tau_min = 100 > tau_max = 99'),
        (dict(fmin=0.0), 'fmin'), (dict(fmin=-1.0), 'fmin'),
        (dict(threshold=0.0), 'threshold'), (dict(threshold=1.0), 'threshold'), (dict(threshold=-0.1), 'threshold'), (dict(threshold=nan), 'threshold'),
        (dict(silence_rms=-1e-9), 'silence_rms'), (dict(silence_rms=nan), 'silence_rms'),
        (dict(gpe_ratio=0.0), 'gpe_ratio'), (dict(gpe_ratio=-0.2), 'gpe_ratio'), (dict(gpe_ratio=nan), 'gpe_ratio'),
        (dict(window=0), 'window'), (dict(window=-1024), 'window'),
    ]
    for kw, word in invalid:
        rc, msg = _create(**kw)
        assert rc == _cabi.ERR_INVALID and word in msg, (kw, rc, msg)
    unsupported = [(dict(frame_length=fl), 'frame_length') for fl in (0, 256, 1000, 2047, 8192)]
    unsupported += [(dict(window=1681), 'window + tau_max + 1'),         # 1681 + 367 + 1 = 2049
                    (dict(frame_length=512, window=256), 'window + tau_max + 1'), (dict(fmin=13.0), 'window + tau_max + 1'),
                    (dict(frame_length=4096, window=4096 - 367), 'window + tau_max + 1')]
    for kw, word in unsupported:
        rc, msg = _create(**kw)
        assert rc == _cabi.ERR_UNSUPPORTED and word in msg, (kw, rc, msg)
    # the limits themselves are accepted
    for kw in (dict(window=1680), dict(frame_length=4096, window=4096 - 368), dict(fmin=220.0, fmax=220.5), dict(silence_rms=0.0),
               dict(frame_length=512, window=144), dict(sample_rate=1, hop=1, fmin=0.01, fmax=1.0, frame_length=512, window=1)):
        assert _create(**kw)[0] == 0, kw
    # null pointers, and the other entries on a refused and on a null handle
    lib = _cabi.load_library()
    h = C.c_void_p()
    assert lib.wrnn_pitch_create(None, C.byref(h)) == _cabi.ERR_INVALID and lib.wrnn_pitch_create(C.byref(_cabi.PitchConfig()), None) == _cabi.ERR_INVALID
    bad = _cabi.PitchConfig(threshold=2.0)
    assert lib.wrnn_pitch_create(C.byref(bad), C.byref(h)) == _cabi.ERR_INVALID and h and b'threshold' in lib.wrnn_pitch_last_error(h)
    assert lib.wrnn_pitch_frames(h, 6000) == _cabi.ERR_INVALID and lib.wrnn_pitch_lags(h, None, None) == _cabi.ERR_INVALID
    assert lib.wrnn_pitch_track(h, 1, 6000, 1, 1, 1, 1, 22, None) == _cabi.ERR_STATE
    assert lib.wrnn_pitch_score(h, 1, 1, 6000, 1, 1, 1, None, 0, None) == _cabi.ERR_STATE
    lib.wrnn_pitch_destroy(h)
    assert lib.wrnn_pitch_track(None, 1, 6000, 1, 1, 1, 1, 22, None) == _cabi.ERR_INVALID
    assert lib.wrnn_pitch_score(None, 1, 1, 6000, 1, 1, 1, None, 0, None) == _cabi.ERR_INVALID
    assert lib.wrnn_pitch_frames(None, 1) == _cabi.ERR_INVALID and lib.wrnn_pitch_last_error(None) == b'null handle'
    lib.wrnn_pitch_destroy(None)
    # argument checks of the launch entries precede every device call
    nat = _cabi.NativePitch()
    for args in ((0, 6000, 1, 1, 1, 1, 22), (1, 6000, 0, 1, 1, 1, 22), (1, 6000, 1, 1, 0, 1, 22), (1, 0, 1, 1, 1, 1, 22), (1, 2 ** 31, 1, 1, 1, 1, 2 ** 31),
                 (1, 6000, 1, 0, 1, 1, 22), (1, 6000, 1, 65536, 1, 1, 22), (1, 6000, 1, 1, 1, 1, 21)):
        with pytest.raises(_cabi.WrnnError) as e:
            nat.track(*args, 0)
        assert e.value.code == _cabi.ERR_INVALID, args
    for args in ((0, 1, 6000, 1, 1, 1, 0, 0), (1, 0, 6000, 1, 1, 1, 0, 0), (1, 1, 0, 1, 1, 1, 0, 0), (1, 1, 6000, 0, 1, 1, 0, 0), (1, 1, 6000, 1, 0, 1, 0, 0),
                 (1, 1, 6000, 1, 65536, 1, 0, 0), (1, 1, 6000, 1, 1, 0, 0, 0), (1, 1, 6000, 1, 1, 1, 1, 109)):
        with pytest.raises(_cabi.WrnnError) as e:
            nat.score(*args, 0)
        assert e.value.code == _cabi.ERR_INVALID, args


@pytest.mark.parametrize('sample_rate, hop', [(22050, 275), (16000, 256), (22050, 64)])
def test_frames_and_lags_are_the_formulas(sample_rate, hop):
    from tacotronv2_wavernn_chinese_amd import _cabi
    for fmin, fmax in ((60.0, 600.0), (80.0, 400.0), (50.0, 441.0), (220.0, 220.5) if sample_rate == 22050 else (160.0, 160.0 + 1e-9)):
        nat = _cabi.NativePitch(_cabi.PitchConfig(sample_rate=sample_rate, hop=hop, fmin=fmin, fmax=fmax))
        assert (nat.tau_min, nat.tau_max) == (math.ceil(sample_rate / fmax), math.floor(sample_rate / fmin)) == pr.lags(sample_rate, fmin, fmax)
        for n in (0, 1, hop - 1, hop, hop + 1, 6000, 2 ** 31 - 1):
            assert nat.frames(n) == (1 + n // hop if n >= 1 else 0) == pr.frames_of(n, hop)
        for bad in (-1, 2 ** 31):
            with pytest.raises(ValueError):
                nat.frames(bad)
        lo = C.c_int32()
        assert nat.lib.wrnn_pitch_lags(nat._h, C.byref(lo), None) == 0 and lo.value == nat.tau_min
    # the mel front end counts the same frames at the same hop
    from tacotronv2_wavernn_chinese_amd.frontend import SpectralScore
    if hop == 275:
        assert SpectralScore().frames(-1, 6000) == _cabi.NativePitch().frames(6000)


def test_wrappers_refuse_without_a_device():
    from tacotronv2_wavernn_chinese_amd.frontend import PitchScore, PitchTracker
    hp = type('hp', (), dict(sample_rate=16000, hop_length=200))
    for cls in (PitchTracker, PitchScore):
        p = cls()
        assert (p.sample_rate, p.hop, p.frame_length, p.window, p.tau_min, p.tau_max) == (22050, 275, 2048, 1024, 37, 367)
        assert [p.frames(n) for n in (0, 1, 275)] == [0, 1, 2]
        q = cls(hp, fmin=80)
        assert (q.sample_rate, q.hop, q.tau_min, q.tau_max) == (16000, 200, 27, 200) and cls(hp, hop=64, sample_rate=8000).hop == 64
        for kw in (dict(fmin=700), dict(fmax=float('nan')), dict(frame_length=1000), dict(window=2000), dict(threshold=1.5), dict(silence_rms=-1),
                   dict(gpe_ratio=0), dict(hop=0), dict(sample_rate=0), dict(window=0), dict(fmin=220.6, fmax=220.9), dict(hop=2 ** 31)):
            with pytest.raises(ValueError):
                cls(**kw)
        with pytest.raises(TypeError):
            cls(n_fft=2048)
    ok = pr.signal('chirp', 3000)
    with pytest.raises(ValueError, match='GPU only'):
        PitchTracker().track(ok, device='cpu')
    with pytest.raises(ValueError, match='the scores run on the GPU only'):      # SpectralScore's own message
        PitchScore().score(ok, ok, device='cpu')
    for a, b in (([ok, ok], [ok]), ([], []), (ok.reshape(2, 1500), ok)):
        with pytest.raises(ValueError):
            PitchScore().score(a, b)
    for bad in ([], ok.reshape(2, 3, 500)):
        with pytest.raises(ValueError):
            PitchTracker().track(bad)


# ---- the boundary ------------------------------------------------------------------------------------------------------------------------

def test_header_binding_and_library_agree_on_the_pitch_entries(tmp_path):
    from tacotronv2_wavernn_chinese_amd import _cabi
    hdr = open(os.path.join(ROOT, 'include', 'wavernn_amd.h')).read()
    declared = sorted(s for s in set(re.findall(r'\b(wrnn_[a-z_]+)\s*\(', hdr)) if s.startswith('wrnn_pitch'))
    assert declared == sorted(s for s in _cabi.EXPORTED_SYMBOLS if s.startswith('wrnn_pitch'))
    assert declared == ['wrnn_pitch_create', 'wrnn_pitch_destroy', 'wrnn_pitch_frames', 'wrnn_pitch_lags', 'wrnn_pitch_last_error', 'wrnn_pitch_score',
                        'wrnn_pitch_track']
    lib = _cabi.load_library()
    assert all(hasattr(lib, s) for s in declared)
    assert int(re.search(r'#define WRNN_ABI_VERSION (\d+)', hdr).group(1)) == 9 == lib.wrnn_abi_version()     # new entries, the old number
    assert C.sizeof(_cabi.SampleOpts) == 88
    macros = {m: int(v) for m, v in re.findall(r'#define (WRNN_PITCH_[A-Z0-9_]+) (\d+)', hdr)}
    assert macros.pop('WRNN_PITCH_FIELDS') == _cabi.PITCH_FIELDS == len(_cabi.PITCH_FIELD_NAMES) == len(macros) == 8
    assert _cabi.PITCH_FIELD_NAMES == pr.FIELDS
    for i, name in enumerate(_cabi.PITCH_FIELD_NAMES):
        assert macros['WRNN_PITCH_' + name.upper()] == i
    fresh = _cabi.PitchConfig()
    assert {k: getattr(fresh, k) for k in pr.DEFAULTS} == pr.DEFAULTS == _cabi.PITCH_DEFAULTS and fresh.struct_size == C.sizeof(_cabi.PitchConfig)
    st = _cabi.PitchConfig
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{ROOT}/include/wavernn_amd.h"', 'int main(void) {',
             '  printf("size %zu\\n", sizeof(wrnn_pitch_config));']
    lines += [f'  printf("{f} %zu\\n", offsetof(wrnn_pitch_config, {f}));' for f, _ in st._fields_]
    lines += ['  return 0;', '}']
    (tmp_path / 'layout.c').write_text('\n'.join(lines))
    subprocess.check_call(['gcc', '-std=c11', '-o', str(tmp_path / 'layout'), str(tmp_path / 'layout.c')])
    got = dict(l.split() for l in subprocess.check_output([str(tmp_path / 'layout')], text=True).splitlines())
    assert int(got['size']) == C.sizeof(st)
    for f, _ in st._fields_:
        assert int(got[f]) == getattr(st, f).offset, f
    assert st._fields_[0][0] == 'struct_size' and st.struct_size.offset == 0


# ---- the command lines ---------------------------------------------------------------------------------------------------------------------

def test_score_cli_pitch_arguments():
    from tacotronv2_wavernn_chinese_amd import score as cli
    p = cli.build_parser()
    a = p.parse_args(['--target', 'a.wav', '--test', 'b.wav'])
    assert (a.pitch, a.fmin, a.fmax, a.pitch_threshold) == (False, None, None, None) and cli.pitch_settings(a) == {}
    a = p.parse_args(['--target', 'a.wav', '--test', 'b.wav', '--pitch', '--fmin', '80', '--fmax', '400', '--pitch_threshold', '0.1'])
    assert a.pitch and cli.pitch_settings(a) == dict(fmin=80.0, fmax=400.0, threshold=0.1)
    assert cli.pitch_settings(p.parse_args(['--target', 'a.wav', '--test', 'b.wav', '--pitch'])) == {}
    with pytest.raises(ValueError, match='--pitch'):
        cli.pitch_settings(p.parse_args(['--target', 'a.wav', '--test', 'b.wav', '--fmin', '80']))
    with pytest.raises(SystemExit):           # a usage error, before anything touches a device
        cli.main(['--target', 'a.wav', '--test', 'b.wav', '--fmax', '400'])
    assert cli.PITCH_KEYS == pr.FIELDS
    # the table: without a pitch hop the three lines of before; with one, an empty line and the pitch fields after them
    s = dict(n=6000, mel_lsd_db=1.0, mcd_db=2.0, mr_sc=0.5, mr_logmag=0.25)
    before = cli.table(['b'], [s], s)
    assert before.splitlines() == ['clip    samples  mel_lsd_db      mcd_db       mr_sc   mr_logmag', 'b          6000    1.000000    2.000000    0.500000    0.250000',
                                   'mean               1.000000    2.000000    0.500000    0.250000']
    s.update(dict(zip(pr.FIELDS, (10.0, 0.0, 0.125, 0.125, 0.99, 18, 17, 16))))
    after = cli.table(['b'], [s], s, 275)
    assert after.startswith(before + '\n\n') and len(after.splitlines()) == 7
    assert after.splitlines()[5].split() == ['b', '22', '10.0000', '0.0000', '0.1250', '0.1250', '0.9900', '18,', '17,', '16']


def test_train_and_fold_quality_flags_are_opt_in():
    from tacotronv2_wavernn_chinese_amd import train as T
    p = T.build_parser()
    assert not p.parse_args(['--synthetic', '4']).score_pitch and not p.parse_args(['--synthetic', '4', '--score_at_checkpoint']).score_pitch
    assert p.parse_args(['--synthetic', '4', '--score_at_checkpoint', '--score_pitch']).score_pitch
    with pytest.raises(ValueError, match='--score_at_checkpoint'):          # before the hyperparameters are read or a device is touched
        T.main(['--synthetic', '4', '--score_pitch'])
    src = open(os.path.join(ROOT, 'tools', 'fold_quality.py')).read()
    assert "'--pitch'" in src and 'PitchScore' in src and os.path.exists(os.path.join(ROOT, 'tools', 'pitch_latency.py'))
