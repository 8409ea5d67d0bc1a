"""The feature profiles of the mel front end on the GPU (``csrc/melspec.hip``, ``MelFrontEnd(features='tacotron')``) against the
restatement ``tests/taco_mel_ref.py``, and what is built on them: ``DeviceCorpus.from_wavs(features='tacotron')`` against the restated
chain of the reference's preprocessing, ``generate_from_wav`` and the command line.

Tolerance, as in ``tests/test_gpu_mel.py``: for every input g = max |ref32 - ref64| of the restatement evaluated in float32 and in
float64, the kernel passes with max |kernel - ref64| <= 8 g, and 0 < 8 g <= 1e-5 is asserted so that an ill-conditioned input cannot
loosen the bound.  Every parity check prints g, the kernel's error and their ratio before it asserts (``pytest -s``).  ``noise_1e-4`` of
``test_gpu_mel`` is left out of the profile cases: its g is 1.2e-6 under the full profile, too close to that cap."""
import os
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

from tests import condition_ref as cr
from tests import mel_ref as mr
from tests import taco_mel_ref as tm

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOP, NFFT, WIN = 275, 2048, 1100
NO_RESCALE = dict(tm.TACOTRON, preemph_rescale=0.0)
# name -> (clip, the profile it runs under)
SWITCHES = {'pad_zero': dict(pad_mode='zero'), 'power_ref': dict(magnitude_power=2, ref_level_db=20.0), 'preemphasis': dict(preemphasis=0.97),
            'fmax': dict(fmax=7600.0)}


def _clips():
    gap = mr.speech_like(3000, 2)
    gap[1200:2600] = 0.0
    return {'speech_1025': mr.speech_like(1025, 0), 'speech_tail': mr.speech_like(HOP * 9 + 17, 1), 'speech_gap': gap,
            'noise_0.3': mr.white(3000, 0.3, 3), 'speech_300': mr.speech_like(300, 8)}


@pytest.fixture(scope='module')
def cases():
    """name -> (clip, features, ref64, g), every restatement computed once."""
    out = {}
    for name, y in _clips().items():
        out[name] = (y, tm.TACOTRON) + tm.error_scale(y, **tm.TACOTRON)
    y = out['noise_0.3'][0]
    out['noise_0.3_norescale'] = (y, NO_RESCALE) + tm.error_scale(y, **NO_RESCALE)
    y = out['speech_tail'][0]
    for name, f in SWITCHES.items():
        out['switch_' + name] = (y, dict(tm.VOCODER, **f)) + tm.error_scale(y, **f)
    return out


_FRONT_ENDS = {}


def _fe(features):
    """One front end per profile (the handle owns device tables)."""
    from tacotronv2_wavernn_chinese_amd.frontend import MelFrontEnd
    key = tuple(sorted(features.items()))
    if key not in _FRONT_ENDS:
        _FRONT_ENDS[key] = MelFrontEnd(features='tacotron') if features == tm.TACOTRON else MelFrontEnd(**features)
    return _FRONT_ENDS[key]


def _check(name, got, r64, g):
    err = float(np.abs(got.astype(np.float64) - r64).max())
    print(f'taco mel parity {name}: frames {r64.shape[1]}, g = {g:.3e}, kernel error = {err:.3e} = {err / g:.2f} g, bound 8 g = {8 * g:.3e}')
    assert 0 < 8 * g <= 1e-5, (name, g)
    assert got.shape == r64.shape and got.dtype == np.float32
    assert err <= 8 * g, (name, err, g)


@pytest.mark.parametrize('name', ['speech_1025', 'speech_tail', 'speech_gap', 'noise_0.3', 'noise_0.3_norescale', 'speech_300'])
def test_parity_each_clip_alone_full_profile(cases, name):
    y, f, r64, g = cases[name]
    got = _fe(f).melspectrogram(y).cpu().numpy()
    assert got.shape[0] == 1 and r64.shape == (80, 1 + y.size // HOP)
    _check(name, got[0], r64, g)
    inside = ((r64 > 0) & (r64 < 1)).mean()
    if name != 'noise_0.3_norescale':
        assert inside > 0.8, (name, inside)                       # the speech clips and the rescaled noise use the open range
    if name == 'speech_gap':
        assert (r64 == 0).mean() > 0.05                           # the frames inside the gap sit on the floor ...
        assert not got[0][r64 == 0].any()                         # ... and come out as exact zeros
    if name == 'noise_0.3_norescale':
        assert (r64 == 1).mean() > 0.01 and inside > 0.5          # unscaled, the pre-emphasised noise reaches the clip at 1 ...
        assert (got[0][r64 == 1] == 1.0).all()                    # ... exactly
    if name == 'speech_300':
        assert r64.shape[1] == 2 and y.size < NFFT // 2 // 2      # shorter than half a window: legal under zero padding only
        with pytest.raises(ValueError):
            _fe(dict(tm.TACOTRON, pad_mode='reflect')).melspectrogram(y)
    if name == 'speech_tail':
        t = r64.shape[1] - 1                                      # the last frame's window taps straddle the clip's end
        assert t * HOP - WIN // 2 < y.size <= t * HOP + WIN // 2 - 1


@pytest.mark.parametrize('name', list(SWITCHES))
def test_one_switch_at_a_time(cases, name):
    """A handle with one field moved off today's profile against the restatement with that field moved: a failure names its stage."""
    y, f, r64, g = cases['switch_' + name]
    assert sum(f[k] != tm.VOCODER[k] for k in f) == (2 if name == 'power_ref' else 1)
    got = _fe(f).melspectrogram(y).cpu().numpy()[0]
    _check('switch/' + name, got, r64, g)
    assert np.abs(r64 - mr.melspectrogram(y, **mr.DEFAULT)).max() > 1e-3      # the switch does move the features


def test_ragged_batch_rows_are_bit_equal_to_the_solo_calls(cases):
    fe = _fe(tm.TACOTRON)
    names = ['speech_300', 'noise_0.3', 'speech_1025', 'speech_gap', 'speech_tail']
    clips = [cases[n][0] for n in names] + [(0.1 * mr.speech_like(3500, 11)).astype(np.float32)]
    peaks = [float(np.abs(tm.preemphasised(c, 0.97, 0.0)).max()) for c in clips]
    lens = [c.size for c in clips]
    assert int(np.argmax(peaks)) == 1 and int(np.argmax(lens)) == 5 and peaks[5] < 0.1 * peaks[1]    # the loudest clip is not the longest
    batch = fe.melspectrogram(clips).cpu().numpy()
    frames = [1 + n // HOP for n in lens]
    assert batch.shape == (6, 80, max(frames)) and fe.last_frames == frames and len(set(frames)) > 3
    for i, c in enumerate(clips):
        solo = fe.melspectrogram(c).cpu().numpy()[0]
        np.testing.assert_array_equal(batch[i, :, :frames[i]].view(np.uint32), solo.view(np.uint32))    # no peak leaks between rows
        assert not batch[i, :, frames[i]:].any()                  # exactly 0 past the clip's own end
    for i, n in enumerate(names):
        _check('ragged/' + n, batch[i, :, :frames[i]], cases[n][2], cases[n][3])


def test_all_zero_clip_is_finite_zero_and_leaves_its_neighbours_alone(cases):
    fe = _fe(tm.TACOTRON)
    a, b, zero = cases['speech_tail'][0], cases['noise_0.3'][0], np.zeros(2000, np.float32)
    solo = fe.melspectrogram(zero).cpu().numpy()
    assert solo.shape == (1, 80, 8) and np.isfinite(solo).all() and not solo.any()
    batch = fe.melspectrogram([a, zero, b]).cpu().numpy()
    assert np.isfinite(batch).all() and not batch[1].any()
    for row, c in ((0, a), (2, b)):
        s = fe.melspectrogram(c).cpu().numpy()[0]
        np.testing.assert_array_equal(batch[row, :, :s.shape[1]].view(np.uint32), s.view(np.uint32))


def test_default_profile_is_unchanged_by_its_name():
    from tacotronv2_wavernn_chinese_amd.frontend import MelFrontEnd
    plain, named = MelFrontEnd(), MelFrontEnd(features='vocoder')
    gap = mr.speech_like(3000, 2)
    gap[1200:2600] = 0.0
    inputs = [mr.speech_like(1025, 0), mr.speech_like(HOP * 9 + 17, 1), gap, mr.white(3000, 0.3, 3), mr.white(2200, 1e-4, 4)]
    for y in inputs:
        assert torch.equal(plain.melspectrogram(y), named.melspectrogram(y))
    assert torch.equal(plain.melspectrogram(inputs), named.melspectrogram(inputs))
    with pytest.raises(ValueError):                               # the default profile keeps refusing what it refused
        named.melspectrogram(mr.speech_like(300, 8))


def _hp():
    return types.SimpleNamespace(sample_rate=22050, n_fft=2048, hop_length=275, win_length=1100, num_mels=80, fmin=95, min_level_db=-100, bits=10,
                                 mu_law=True, voc_mode='RAW', voc_pad=2, voc_seq_len=550)


def test_corpus_from_wavs_is_the_restated_preprocessing_chain(tmp_path):
    """Trim, rescale, the mel of the pre-emphasised clip, and labels of the plain clip zero-padded to frames * hop samples."""
    from tacotronv2_wavernn_chinese_amd import dataset as D
    spans = [(7000, 1500, 5500), (6000, 0, 4000), (8001, 4000, 8001), (5000, 0, 5000)]
    clips = [cr.clear_clip(n, lo, hi, 1e-3, 25.0, seed0=900 + 10 * k) for k, (n, lo, hi) in enumerate(spans)]
    want = [tm.process_utterance(x) for x in clips]
    g = [float(np.abs(tm.process_utterance(x, dtype=np.float32)[1].astype(np.float64) - w[1]).max()) for x, w in zip(clips, want)]
    assert sum(w[2].size < x.size for x, w in zip(clips, want)) == 3           # three of the four are trimmed
    c = D.DeviceCorpus.from_wavs(clips, _hp(), 'cuda:0', batch_clips=2, features='tacotron', trim_top_db=25, peak_norm=True)
    assert len(c) == 4 and c.features == 'tacotron' and c.n_clipped == 0 and (c.trim_top_db, c.peak_norm) == (25.0, 0.999)
    frames = [1 + w[2].size // HOP for w in want]
    assert c.frames.tolist() == frames and c.label_len.tolist() == [t * HOP for t in frames]
    zero_label = int(tm.quantise(np.zeros(1), 10, True)[0])
    for u, (mel, lab) in enumerate(c.pairs()):
        labels, ref, wav = want[u]
        np.testing.assert_array_equal(lab, labels)                             # exactly, the padded tail included
        assert lab.shape == (frames[u] * HOP,) and frames[u] * HOP > wav.size and (lab[wav.size:] == zero_label).all()
        _check(f'chain/utt{u}', mel, ref.astype(np.float64), g[u])
    listing = c.save(tmp_path / 'corpus')
    assert D.saved_features(listing) == 'tacotron'
    back = D.DeviceCorpus.load(listing, 'cuda:0', hop_length=HOP)
    assert back.features == 'tacotron' and torch.equal(back.labels, c.labels) and torch.equal(back.mels, c.mels)
    assert back.label_len.tolist() == c.label_len.tolist() and back.frames.tolist() == c.frames.tolist()
    with pytest.raises(ValueError, match="holds 'tacotron' mel features"):
        D.check_saved_features(listing, 'vocoder')
    plain = D.DeviceCorpus.from_wavs(clips, _hp(), 'cuda:0', batch_clips=2, trim_top_db=25, peak_norm=True)   # the default corpus is as it was
    assert plain.features == 'vocoder' and plain.label_len.tolist() == [w[2].size for w in want]
    lone = D.DeviceCorpus.from_wavs([w[2] for w in want], _hp(), 'cuda:0', features='tacotron')       # the unconditioned path pads too
    assert torch.equal(lone.labels, c.labels) and torch.equal(lone.mels, c.mels)


@pytest.fixture(scope='module')
def model():
    from tacotronv2_wavernn_chinese_amd.synth import DEFAULT_DIMS, make_state_dict
    from tacotronv2_wavernn_chinese_amd.vocoder import WaveRNN
    sd = make_state_dict(0, variant='peaky')
    m = WaveRNN(**DEFAULT_DIMS, mode='RAW')
    m.verbose = False
    m.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in sd.items()})
    return m.to('cuda:0')


def test_generate_from_wav_and_the_cli_vocode_the_tacotron_mel(model, tmp_path):
    """Composition at 21 frames, the shortest clip ``generate`` accepts."""
    from scipy.io import wavfile
    from tacotronv2_wavernn_chinese_amd.dsp import save_wav
    from tacotronv2_wavernn_chinese_amd.frontend import MelFrontEnd
    x = mr.speech_like(HOP * 20 + 17, 6)
    torch.manual_seed(5)
    a = model.generate_from_wav(x, tmp_path / 'a.wav', False, 11000, 550, True, features='tacotron')
    mel = MelFrontEnd(features='tacotron').melspectrogram(x)
    assert mel.is_cuda and tuple(mel.shape) == (1, 80, 21)
    assert not torch.equal(mel, model.mel_front_end().melspectrogram(x))       # not the default features
    torch.manual_seed(5)
    b = model.generate(mel, tmp_path / 'b.wav', False, 11000, 550, True)
    assert a.shape == (20 * HOP,) and a.dtype == np.float64
    np.testing.assert_array_equal(a, b)
    many = model.generate_many(wavs=[x], seeds=[11], features='tacotron')
    ref = model.generate_many([mel[0].cpu().numpy()], seeds=[11])
    np.testing.assert_array_equal(many[0], ref[0])
    with pytest.raises(ValueError, match='wavs='):
        model.generate_many([mel[0].cpu().numpy()], features='tacotron')
    # the command line with the same weights and seed writes that wav
    save_wav(x, tmp_path / 'x.wav', 22050)
    model.save(tmp_path / 'weights.pyt')
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'wavernn_gen.py'), '--file', str(tmp_path / 'x.wav'), '-u', '--seed', '5', '--features',
                        'tacotron', '--voc_weights', str(tmp_path / 'weights.pyt')], cwd=tmp_path, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    written = sorted((tmp_path / 'wavernn_inference_output').glob('x_gen_NOT_BATCHED_step=*k.wav'))
    assert len(written) == 1
    sr, voc = wavfile.read(written[0])
    assert sr == 22050 and voc.dtype == np.float32
    np.testing.assert_array_equal(voc, a.astype(np.float32))
