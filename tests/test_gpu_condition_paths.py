"""The wav conditioning through the entries that use it: ``DeviceCorpus.from_wavs``, ``generate_from_wav``, ``generate_many(wavs=)``,
``load_wav`` and the command line.  Everything downstream of the conditioned wav is the same kernels on a bit-equal buffer, so every
comparison with the same entry fed the restatement's clip (``tests/condition_ref.py``) is for equality."""
import os
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

from tests import condition_ref as cr
from tests import mel_ref as mr
from tests import resample_ref as rr

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOP = 275


def _hp():
    return types.SimpleNamespace(sample_rate=22050, n_fft=2048, hop_length=275, win_length=1100, num_mels=80, fmin=95, min_level_db=-100, bits=10,
                                 mu_law=True, voc_mode='RAW', voc_pad=2, voc_seq_len=550)


def _host(x, trim_top_db=25.0, target=0.999):
    return cr.condition(x, trim_top_db, target)[0]


def _corpus_clips():
    """Bursts of different lengths in floors of different lengths; the last clip's burst is so short that what is left of it after
    trimming has fewer than the 12 frames a window of _hp() needs."""
    spans = [(12345, 3000, 9000), (9000, 0, 5000), (16001, 9000, 16001), (7000, 0, 7000), (10000, 4000, 4100)]
    return [cr.clear_clip(n, lo, hi, 1e-3, 25.0, seed0=500 + 10 * k) for k, (n, lo, hi) in enumerate(spans)]


def test_from_wavs_conditions_into_the_corpus_of_the_host_conditioned_clips():
    from tacotronv2_wavernn_chinese_amd import dataset as D
    clips = _corpus_clips()
    host = [_host(x) for x in clips]
    trimmed = [y.shape[0] for y in host]
    assert [1 + n // HOP >= 12 for n in trimmed] == [True, True, True, True, False] and 1 + clips[4].shape[0] // HOP >= 12
    assert sum(n < x.shape[0] for n, x in zip(trimmed, clips)) == 4 and trimmed[3] == 7000
    a = D.DeviceCorpus.from_wavs(clips, _hp(), 'cuda:0', batch_clips=2, trim_top_db=25, peak_norm=True)
    b = D.DeviceCorpus.from_wavs(host, _hp(), 'cuda:0', batch_clips=2)
    assert len(a) == len(b) == 4 and a.stems == b.stems == ['utt00000', 'utt00001', 'utt00002', 'utt00003']   # the short one is dropped
    assert a.label_len.tolist() == b.label_len.tolist() == trimmed[:4] and a.frames.tolist() == b.frames.tolist()
    assert a.label_off.tolist() == b.label_off.tolist() and a.mel_off.tolist() == b.mel_off.tolist()
    assert torch.equal(a.labels, b.labels) and torch.equal(a.mels, b.mels)
    assert a.n_clipped == b.n_clipped == 0 and (a.trim_top_db, a.peak_norm) == (25.0, 0.999) and (b.trim_top_db, b.peak_norm) == (None, None)
    one = D.DeviceCorpus.from_wavs(clips, _hp(), 'cuda:0', batch_clips=16, trim_top_db=25, peak_norm=True)     # one group: the same corpus
    assert torch.equal(one.labels, a.labels) and torch.equal(one.mels, a.mels)
    t = D.DeviceCorpus.from_wavs(clips, _hp(), 'cuda:0', trim_top_db=25)                                       # trimming alone
    u = D.DeviceCorpus.from_wavs([cr.condition(x, 25.0, None)[0] for x in clips], _hp(), 'cuda:0')
    assert torch.equal(t.labels, u.labels) and torch.equal(t.mels, u.mels) and t.label_len.tolist() == trimmed[:4] and t.peak_norm is None
    sub = a.subset([1, 2])
    assert (sub.trim_top_db, sub.peak_norm) == (25.0, 0.999)
    with pytest.raises(ValueError, match='after trimming'):
        D.DeviceCorpus.from_wavs(clips[4:], _hp(), 'cuda:0', trim_top_db=25)


def _full_scale_48k():
    """A full-scale square wave at 48 kHz: band-limiting it to 11 kHz overshoots (Gibbs), so the resampled clip leaves [-1, 1]."""
    t = np.arange(30000)
    return np.where((t // 40) % 2 == 0, 1.0, -1.0).astype(np.float32)


def test_peak_norm_after_the_resampler_leaves_nothing_to_clip():
    from tacotronv2_wavernn_chinese_amd import dataset as D
    x = _full_scale_48k()
    over = float(np.abs(rr.resample(x, 48000, 22050)).max())
    print(f'peak of the resampled full-scale clip in the float64 restatement: {over:.4f}')
    assert over > 1.05
    plain = D.DeviceCorpus.from_wavs([(x, 48000)], _hp(), 'cuda:0', resample=True)
    normed = D.DeviceCorpus.from_wavs([(x, 48000)], _hp(), 'cuda:0', resample=True, peak_norm=True)
    assert plain.n_clipped > 0 and normed.n_clipped == 0
    assert plain.label_len.tolist() == normed.label_len.tolist() == [rr.out_len(x.size, 48000, 22050)]
    from tacotronv2_wavernn_chinese_amd.frontend import Resampler
    y = Resampler(48000, 22050)(x)[0].cpu().numpy()                 # the device's resampled clip, conditioned on the host
    ref = D.DeviceCorpus.from_wavs([_host(y, None)], _hp(), 'cuda:0')
    assert torch.equal(normed.labels, ref.labels) and torch.equal(normed.mels, ref.mels)


@pytest.fixture(scope='module')
def model():
    from tacotronv2_wavernn_chinese_amd.synth import DEFAULT_DIMS, make_state_dict
    from tacotronv2_wavernn_chinese_amd.vocoder import WaveRNN
    sd = make_state_dict(0, variant='peaky')
    m = WaveRNN(**DEFAULT_DIMS, mode='RAW')
    m.verbose = False
    m.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in sd.items()})
    return m.to('cuda:0')


def _vocoder_clip(seed0=700):
    """12 hops of 512 samples stay after trimming, 6144 samples = 23 frames: the least a trimmed clip can have above the 21 frames
    ``generate`` needs (11 hops are 5632 samples, 21 frames)."""
    x = cr.clear_clip(9000, 2600, 7000, 1e-3, 25.0, seed0=seed0)
    start, end = cr.trim_bounds(x, 25.0)
    assert end - start == 12 * 512 and 1 + (end - start) // HOP == 23 and 1 + 11 * 512 // HOP == 21
    return x


def test_generate_from_wav_conditions_like_the_host(model, tmp_path):
    x = _vocoder_clip()
    y = _host(x)
    a = model.generate_from_wav(x, tmp_path / 'a.wav', False, 11000, 550, True, trim_top_db=25, peak_norm=True, seed=5)
    mel = model.mel_front_end().melspectrogram(y, device='cuda:0')
    b = model.generate(mel, tmp_path / 'b.wav', False, 11000, 550, True, seed=5)
    assert a.shape == (22 * HOP,) and a.dtype == np.float64
    np.testing.assert_array_equal(a, b)
    c = model.generate_from_wav(x, tmp_path / 'c.wav', False, 11000, 550, True, seed=5)        # the defaults: the clip as it is
    assert c.shape == ((9000 // HOP) * HOP,)


def test_generate_many_conditions_every_clip(model):
    xs = [_vocoder_clip(), cr.clear_clip(12000, 0, 8000, 1e-3, 25.0, seed0=720)]
    ys = [_host(x) for x in xs]
    got = model.generate_many(wavs=xs, seeds=[11, 12], trim_top_db=25, peak_norm=True)
    want = model.generate_many(wavs=ys, seeds=[11, 12])
    assert [g.shape for g in got] == [w.shape for w in want] == [((y.shape[0] // HOP) * HOP,) for y in ys] and ys[1].shape[0] < 12000
    for g, w in zip(got, want):
        np.testing.assert_array_equal(g, w)


def test_load_wav_round_trip(tmp_path):
    from scipy.io import wavfile
    from tacotronv2_wavernn_chinese_amd.frontend import load_wav
    x = _vocoder_clip()
    wavfile.write(str(tmp_path / 'x.wav'), 22050, x)                      # float32 samples: read back as they are
    np.testing.assert_array_equal(load_wav(tmp_path / 'x.wav', 22050), x)
    got = load_wav(tmp_path / 'x.wav', 22050, trim_top_db=25, peak_norm=True)
    assert got.dtype == np.float32 and got.shape == (6144,)
    np.testing.assert_array_equal(got.view(np.uint32), _host(x).view(np.uint32))
    np.testing.assert_array_equal(load_wav(tmp_path / 'x.wav', 22050, peak_norm=0.5).view(np.uint32), cr.condition(x, None, 0.5)[0].view(np.uint32))
    x48 = mr.speech_like(13000, 6, 48000)                                 # another rate: the resampler first, then the conditioning
    wavfile.write(str(tmp_path / 'x48.wav'), 48000, x48)
    got = load_wav(tmp_path / 'x48.wav', 22050, resample=True, peak_norm=True)
    plain = load_wav(tmp_path / 'x48.wav', 22050, resample=True)
    np.testing.assert_array_equal(got.view(np.uint32), _host(plain, None).view(np.uint32))


def test_cli_vocodes_a_conditioned_wav_file(tmp_path):
    """``wavernn_gen.py --file clip.wav --trim_silence --peak_norm``: the saved target file is the conditioned clip."""
    from scipy.io import wavfile
    x = _vocoder_clip()
    wavfile.write(str(tmp_path / 'clip.wav'), 22050, x)
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'wavernn_gen.py'), '--file', str(tmp_path / 'clip.wav'), '-u', '--seed', '5', '--trim_silence',
                        '--peak_norm'], cwd=tmp_path, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    out = tmp_path / 'wavernn_inference_output'
    sr, tgt = wavfile.read(out / '__clip__0k_steps_target.wav')
    assert sr == 22050
    np.testing.assert_array_equal(tgt.view(np.uint32), _host(x).view(np.uint32))
    sr, voc = wavfile.read(out / 'clip_gen_NOT_BATCHED_step=0k.wav')
    assert sr == 22050 and voc.shape == (22 * HOP,) and np.isfinite(voc).all()
