"""Griffin-Lim without a GPU: analytic pins of the restatement ``tests/griffin_lim_ref.py``, the host tables of the library against it,
and what the create entry and the class refuse."""
import ctypes as C

import numpy as np
import pytest

from tests import griffin_lim_ref as gr
from tests import mel_ref as mr
from tests import taco_mel_ref as tm

HOP, NFFT, WIN = 275, 2048, 1100
PROFILES = {'tacotron': tm.TACOTRON, 'vocoder': tm.VOCODER}


# ---- the restatement ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('pad_mode', ['zero', 'reflect'])
def test_a_bin_centred_sinusoid_survives_stft_and_istft(pad_mode):
    n = HOP * 12
    y = 0.5 * np.cos(2 * np.pi * 64 * np.arange(n) / NFFT + 0.3)      # 64 cycles per transform length: centred on bin 64
    D = gr.stft(y, pad_mode=pad_mode)
    assert D.shape == (NFFT // 2 + 1, 13)
    mid = np.abs(D[:, 6])
    # the peak is A / 2 times the window's sum (win / 2); Hann's side lobes fall with the cube of the distance: far bins are below 1e-3
    assert int(np.argmax(mid)) == 64 and abs(mid[64] - 0.25 * WIN / 2) < 1e-3 and mid[128:].max() < 1e-3 * mid[64]
    back = gr.istft(D)
    assert back.shape == (n,)
    np.testing.assert_allclose(back, y, atol=1e-13)                   # wss divides out the window exactly wherever it is not ~0
    b32 = gr.istft(gr.stft(y, pad_mode=pad_mode, dtype=np.float32), dtype=np.float32)
    assert b32.dtype == np.float32 and np.abs(b32 - y).max() < 2e-6


@pytest.mark.parametrize('hop,win', [(275, 1100), (200, 1100), (256, 2048)])
def test_window_sumsquare_is_the_analytic_sum(hop, win):
    T = 9
    w = 0.5 - 0.5 * np.cos(2 * np.pi * np.arange(win) / win)          # the periodic Hann window, written out
    off = (NFFT - win) // 2
    want = np.zeros(NFFT + hop * (T - 1))
    for p in range(want.size):
        for t in range(T):
            i = p - t * hop - off
            if 0 <= i < win:
                want[p] += w[i] ** 2
    np.testing.assert_allclose(gr.window_sumsquare(T, hop, win), want, atol=1e-12)
    if win % hop == 0:    # hop divides the window: the squares of a Hann window sum to 3 win / (8 hop) away from the edges
        inner = want[off + win:off + hop * (T - 1)]
        np.testing.assert_allclose(inner, 3 * win / (8 * hop), rtol=1e-12)


def test_a_consistent_spectrogram_is_a_fixed_point_from_its_own_phases():
    y = gr.harmonic_chirp(HOP * 10, 3).astype(np.float64)
    D = gr.stft(y)
    S = np.abs(D)
    r = (np.angle(D) / (2 * np.pi)).T                                  # exp(2 pi i r) are D's own phases
    waves = gr.griffin_lim(S, r, 3, keep=(0, 1, 3))
    for i, v in waves.items():
        np.testing.assert_allclose(v, y, atol=1e-12, err_msg=f'round {i}')


def test_spectral_convergence_falls_on_the_chirp():
    y = gr.harmonic_chirp(HOP * 40, 0)
    mel = tm.melspectrogram(y, **tm.TACOTRON)
    S = gr.mel_to_magnitude(mel, **tm.TACOTRON)
    waves = gr.griffin_lim(S, gr.philox_phases(1, 0, mel.shape[1]), 60, keep=(0, 1, 10, 60))
    sc = {i: gr.spectral_convergence(v, S) for i, v in waves.items()}
    print('spectral convergence', sc)
    assert sc[0] > sc[1] > sc[10] > sc[60]
    assert 0.5 < sc[0] < 0.9 and sc[1] < 0.5 and sc[60] < 0.3         # a CPU prototype: 0.73, 0.38, 0.24, 0.13 - 0.17


def test_unit_phase_of_zero_is_one_and_deemphasis_inverts_preemphasis():
    u = gr.unit_phase(np.array([0j, 3 + 4j, -2.0]))
    assert u[0] == 1 and u[2] == -1 and abs(u[1] - (0.6 + 0.8j)) < 1e-15
    x = gr.harmonic_chirp(3000, 5).astype(np.float64)
    p = tm.preemphasised(x, 0.97, 0.0)
    np.testing.assert_allclose(gr.deemphasis(p, 0.97), x, atol=1e-12)
    d32 = gr.deemphasis(p.astype(np.float32), 0.97, np.float32)
    assert d32.dtype == np.float32 and 0 < np.abs(d32 - x).max() < 1e-4


def test_mel_to_magnitude_inverts_the_forward_steps_on_a_mel_that_is_in_range():
    """Steps 7, 6 and 4 backwards give the forward chain's own mel amplitudes back: S equals max(1e-10, P a)^power with a taken from
    the forward restatement's intermediate values, up to the float32 rounding of the stored [-A, A] mel."""
    y = (0.02 * gr.harmonic_chirp(HOP * 6, 2)).astype(np.float32)      # quiet: the vocoder profile clips a loud clip's low bands at 1
    for name, f in PROFILES.items():
        mel = tm.melspectrogram(y, **f).astype(np.float64)
        assert 0 < mel.min() and mel.max() < 1, name                   # nothing clipped: every step is invertible
        p = tm.preemphasised(y, f['preemphasis'], f['preemph_rescale'])
        D = tm.stft(p, NFFT, HOP, WIN, f['pad_mode'])
        a = tm.mel_basis(22050, NFFT, 80, 95.0, f['fmax']) @ (np.abs(D) ** f['magnitude_power'])
        a = a ** (1.0 / f['magnitude_power'])
        want = np.maximum(1e-10, gr.pinv_basis(fmax=f['fmax']) @ a) ** 1.5
        S = gr.mel_to_magnitude(mel, power=1.5, **f)
        assert np.abs(S - want).max() < 1e-4 * want.max(), name


# ---- the library's host side ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('name', ['tacotron', 'vocoder'])
def test_library_tables_against_the_restatement(name):
    from tacotronv2_wavernn_chinese_amd.frontend import GriffinLim
    gl = GriffinLim(features=name)
    T = 7
    tab = gl.tables(T)
    P = gr.pinv_basis(fmax=PROFILES[name]['fmax'])
    assert tab['pinv'].shape == P.shape == (1025, 80) and tab['pinv'].dtype == np.float32
    assert np.abs(tab['pinv'] - P).max() <= 1e-6 * np.abs(P).max()
    np.testing.assert_array_equal(tab['window'], mr.window(WIN).astype(np.float32))
    wss = gr.window_sumsquare(T)
    assert tab['window_sumsquare'].shape == wss.shape == (NFFT + HOP * (T - 1),)
    np.testing.assert_allclose(tab['window_sumsquare'], wss, atol=4 * 2.0 ** -24 * wss.max())   # four float32 additions at most
    for t in (1, 2, 7, 401):
        assert gl.samples(t) == HOP * (t - 1)
    with pytest.raises(ValueError):
        gl.samples(0)


def test_other_framings_tables():
    from tacotronv2_wavernn_chinese_amd.frontend import GriffinLim
    for hop, win in ((6, 1100), (1100, 1100), (256, 2048)):
        gl = GriffinLim(features='tacotron', hop_length=hop, win_length=win)
        tab = gl.tables(5)
        wss = gr.window_sumsquare(5, hop, win)
        np.testing.assert_allclose(tab['window_sumsquare'], wss, atol=(WIN // hop + 2) * 2.0 ** -24 * wss.max())
        assert gl.samples(5) == 4 * hop


def test_refusals():
    from tacotronv2_wavernn_chinese_amd import _cabi
    from tacotronv2_wavernn_chinese_amd.frontend import FEATURE_PROFILES, GriffinLim
    with pytest.raises(ValueError, match='UNSUPPORTED'):
        GriffinLim(n_fft=1024)
    with pytest.raises(ValueError, match='INVALID'):
        GriffinLim(power=0)
    with pytest.raises(ValueError, match='INVALID'):
        GriffinLim(power=-1.5)
    with pytest.raises(ValueError):
        GriffinLim(n_iter=-1)
    with pytest.raises(ValueError):
        GriffinLim(features='linear')
    with pytest.raises(TypeError):
        GriffinLim(griffin_lim=True)
    # a filterbank finer than the bins: the restated basis really has empty rows for 128 mels below 400 Hz (the full band has none)
    assert (tm.mel_basis(22050, NFFT, 128, 0.0, 400.0).sum(axis=1) == 0).any()
    assert not (tm.mel_basis(22050, NFFT, 128, 95.0, 0.0).sum(axis=1) == 0).any()
    with pytest.raises(ValueError, match='UNSUPPORTED.*empty'):
        GriffinLim(n_mels=128, fmin=0.0, fmax=400.0)
    assert GriffinLim(n_mels=128, features='vocoder').tables()['pinv'].shape == (1025, 128)
    # the struct sizes, at the C entry itself
    lib = _cabi.load_library()
    cfg = _cabi.MelConfig(22050, 2048, 275, 1100, 80, 95.0, -100.0, 0)
    for bad in ('features', 'griffin'):
        feat, g, h = _cabi.MelFeatures(), _cabi.GriffinConfig(), C.c_void_p()
        (feat if bad == 'features' else g).struct_size -= 4
        assert lib.wrnn_griffin_create(C.byref(cfg), C.byref(feat), C.byref(g), C.byref(h)) == _cabi.ERR_INVALID
        assert b'struct_size' in lib.wrnn_griffin_last_error(h)
        assert lib.wrnn_griffin_samples(h, 5) < 0                      # a refused handle answers nothing
        lib.wrnn_griffin_destroy(h)
    assert FEATURE_PROFILES == {'vocoder': tm.VOCODER, 'tacotron': tm.TACOTRON}   # unchanged by the new class


def test_griffin_config_matches_the_header_layout(tmp_path):
    import os
    import subprocess
    from tacotronv2_wavernn_chinese_amd import _cabi
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    st = _cabi.GriffinConfig
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{root}/include/wavernn_amd.h"', 'int main(void) {',
             '  printf("size %zu\\n", sizeof(wrnn_griffin_config));']
    lines += [f'  printf("{f} %zu\\n", offsetof(wrnn_griffin_config, {f}));' for f, _ in st._fields_] + ['  return 0;', '}']
    (tmp_path / 'layout.c').write_text('\n'.join(lines))
    subprocess.check_call(['gcc', '-std=c11', '-o', str(tmp_path / 'layout'), str(tmp_path / 'layout.c')])
    got = dict(l.split() for l in subprocess.check_output([str(tmp_path / 'layout')], text=True).splitlines())
    assert int(got['size']) == C.sizeof(st)
    for f, _ in st._fields_:
        assert int(got[f]) == getattr(st, f).offset


def test_deemphasis_entry_refuses_bad_arguments_without_a_device():
    from tacotronv2_wavernn_chinese_amd import _cabi
    lib = _cabi.load_library()
    assert lib.wrnn_deemphasis(None, 10, None, 1, 0.97, None, None) == _cabi.ERR_INVALID
    assert lib.wrnn_deemphasis(1, 10, 1, 1, 1.0, 1, None) == _cabi.ERR_INVALID
    assert lib.wrnn_deemphasis(1, 0, 1, 1, 0.5, 1, None) == _cabi.ERR_INVALID


def test_command_line_flag_parses_and_stays_off_by_default():
    from tacotronv2_wavernn_chinese_amd.gen import build_parser
    p = build_parser()
    assert p.parse_args(['--file', 'x.npy']).griffin_lim is None
    assert p.parse_args(['--file', 'x.npy', '--griffin_lim']).griffin_lim == 60
    a = p.parse_args(['--file', 'x.npy', '--griffin_lim', '3', '--seed', '1', '--features', 'tacotron'])
    assert (a.griffin_lim, a.seed, a.features) == (3, 1, 'tacotron')
