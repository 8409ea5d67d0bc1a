"""The training-data kernels on the MI355X (csrc/dataset.hip) and what is built on them: `wrnn_quantise` against the float64 NumPy
formulas, `wrnn_collate_windows` / `DeviceWindowLoader` against the host collate bit for bit, a corpus from wavs end to end, one training
step on a device-made batch, and the two command lines."""
import os
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

from tacotronv2_wavernn_chinese_amd import _cabi, dataset as D, train as T

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = 'cuda:0'
QUANT_CASES = [(9, 1), (10, 1), (10, 0), (16, 0)]
BAND = 1e-9


def ref_labels(x, bits, mu_law):
    """(labels, in_band): the reference formulas (wavernn/utils/dsp.py:12-15, 92-95 + the collate's astype(int64)) in float64 NumPy, and
    which samples' value before the floor / truncation lies within BAND of an integer (there a last-bit difference of `log` may move
    the label by one)."""
    mu = 2 ** bits - 1
    xd = np.asarray(x, np.float64)
    if mu_law:
        fx = np.sign(xd) * np.log(1 + mu * np.abs(xd)) / np.log(1 + mu)
        pre = (fx + 1) / 2 * mu + 0.5
        lab = np.floor(pre)
    else:
        pre = (xd + 1.) * mu / 2
        lab = pre.clip(0, mu)
    return lab.clip(0, mu).astype(np.int64), np.abs(pre - np.round(pre)) <= BAND


def quantise(x, bits, mu_law):
    """`wrnn_quantise` on a host float32 array -> (labels int64 on the host, n_clipped)."""
    wav = torch.from_numpy(np.array(x, np.float32)).to(DEV)
    lab = torch.full((wav.numel(),), -7, dtype=torch.int32, device=DEV)
    clipped = torch.zeros(1, dtype=torch.int64, device=DEV)
    _cabi.quantise(wav.data_ptr(), wav.numel(), bits, mu_law, lab.data_ptr(), clipped.data_ptr(), torch.cuda.current_stream().cuda_stream)
    return lab.cpu().numpy().astype(np.int64), int(clipped.item())


@pytest.fixture(scope='module')
def quant_input():
    rng = np.random.Generator(np.random.PCG64(2024))
    pcm = np.arange(-32768, 32768, dtype=np.float32) / np.float32(32768.0)           # every int16 sample as load_wav scales it
    rand = np.clip(np.float32(0.3) * rng.standard_normal(100_000, dtype=np.float32), -1, 1)
    x = np.concatenate([pcm, np.array([1.0], np.float32), rand]).astype(np.float32)
    x.setflags(write=False)
    return x


@pytest.mark.parametrize('bits,mu_law', QUANT_CASES)
def test_quantiser_equals_the_float64_formula(quant_input, bits, mu_law):
    """Equal labels wherever the float64 value before the floor is farther than 1e-9 from an integer; there a difference of 1 is allowed.
    So that the exemption hides nothing: x = 0 and x = +-1 must be exact anyway (they are the only values that land on an integer --
    0 under mu-law, +-1 on the linear scale, where the draw's clip puts ~90 samples), the band holds at most 2 distinct values, and
    at most 2 samples other than those three are exempt (none, in NumPy)."""
    x = quant_input
    want, band = ref_labels(x, bits, mu_law)
    got, n_clipped = quantise(x, bits, mu_law)
    pinned = (x == 0) | (np.abs(x) == 1)
    exempt = band & ~pinned
    print(f'\n[quantise bits {bits} mu_law {mu_law}] in band {int(band.sum())} (values {np.unique(x[band]).tolist()}), exempt {int(exempt.sum())}, '
          f'differing {int((got != want).sum())}')
    assert np.unique(x[band]).size <= 2 and int(exempt.sum()) <= 2
    assert n_clipped == 0
    assert got.min() >= 0 and got.max() <= 2 ** bits - 1
    np.testing.assert_array_equal(got[~exempt], want[~exempt])
    assert np.all(np.abs(got[exempt] - want[exempt]) <= 1)
    mu = 2 ** bits - 1
    hand, _ = quantise(np.array([0.0, 1.0, -1.0], np.float32), bits, mu_law)
    assert hand.tolist() == ([2 ** (bits - 1), mu, 0] if mu_law else [2 ** (bits - 1) - 1, mu, 0])


@pytest.mark.parametrize('bits,mu_law', QUANT_CASES)
def test_quantiser_clips_and_counts_samples_outside_the_unit_interval(bits, mu_law):
    x = np.linspace(-0.9, 0.9, 1000).astype(np.float32)          # more than one workgroup, not a multiple of 256
    x[[3, 500, 999]] = [1.5, -2.0, 1.0000001]
    got, n_clipped = quantise(x, bits, mu_law)
    want, band = ref_labels(x, bits, mu_law)
    assert n_clipped == 3
    assert got[[3, 500, 999]].tolist() == [2 ** bits - 1, 0, 2 ** bits - 1]
    np.testing.assert_array_equal(got[~band], want[~band])


# --------------------------------------------------------------------------------------------------------------- collate
def _pairs(frames, n_mels, hop, bits, seed):
    rng = np.random.Generator(np.random.PCG64(seed))
    return [(rng.random((n_mels, t), dtype=np.float32), rng.integers(0, 2 ** bits, size=t * hop).astype(np.int32)) for t in frames]


def _same_batches(dev_loader, host_loader, epochs=2):
    n = 0
    for _ in range(epochs):
        a, b = list(dev_loader), list(host_loader)
        assert len(a) == len(b) == len(dev_loader) == len(host_loader)
        for (x, y, m), (x0, y0, m0) in zip(a, b):
            assert x.is_cuda and y.is_cuda and m.is_cuda
            assert x.dtype == x0.dtype and y.dtype == y0.dtype and m.dtype == m0.dtype
            assert torch.equal(x.cpu(), x0) and torch.equal(y.cpu(), y0) and torch.equal(m.cpu(), m0)
            n += 1
    return n


def _check_loader(mode, batch_size, *, n_mels, **kw):
    sig_bits = 16 if mode == 'MOL' else 10
    pairs = _pairs([13, 14, 20, 31, 40], n_mels, kw['hop_length'], sig_bits, 7)
    corpus = D.DeviceCorpus.from_pairs(pairs, DEV, hop_length=kw['hop_length'])
    assert len(corpus) == 5 and corpus.frames.tolist() == [13, 14, 20, 31, 40]
    for (m, w), (m0, w0) in zip(corpus.pairs(), pairs):
        assert np.array_equal(m, m0) and np.array_equal(w, w0)
    dl = D.DeviceWindowLoader(corpus, batch_size, mode=mode, bits=10, seed=5, **kw)
    wl = T.WindowLoader(corpus.pairs(), batch_size, mode=mode, bits=10, seed=5, **kw)
    assert _same_batches(dl, wl) == 2 * ((5 + batch_size - 1) // batch_size)
    x, y, m = next(iter(dl))
    win = kw['seq_len'] // kw['hop_length'] + 2 * kw['pad']
    assert tuple(x.shape) == tuple(y.shape) == (batch_size, kw['seq_len']) and tuple(m.shape) == (batch_size, n_mels, win)
    assert y.dtype == (torch.float32 if mode == 'MOL' else torch.int64)


@pytest.mark.parametrize('mode', ['RAW', 'MOL'])
@pytest.mark.parametrize('batch_size', [2, 5])
def test_device_loader_equals_the_host_collate(mode, batch_size):
    """5 utterances of 13 .. 40 frames (13 is the shortest the window of 6 with pad 2 accepts: its only offset is 0), two epochs; batch
    size 2 ends every epoch on a short batch."""
    _check_loader(mode, batch_size, n_mels=80, hop_length=275, pad=2, seq_len=550)


def test_device_loader_hard_codes_no_stride():
    """Another hop, pad and band count: win = 5, 40 bands, 600 samples per row (13 frames leave offsets 0 .. 3)."""
    _check_loader('RAW', 2, n_mels=40, hop_length=200, pad=1, seq_len=600)


def test_a_subset_shares_the_buffers_and_serves_its_own_utterances():
    pairs = _pairs([13, 14, 20, 31, 40], 80, 275, 10, 8)
    corpus = D.DeviceCorpus.from_pairs(pairs, DEV, hop_length=275)
    train, test = corpus.split(2)
    assert len(train) == 3 and len(test) == 2 and train.labels.data_ptr() == corpus.labels.data_ptr()
    assert sorted(train.stems + test.stems) == sorted(corpus.stems)
    kw = dict(mode='RAW', bits=10, hop_length=275, pad=2, seq_len=550)
    assert _same_batches(D.DeviceWindowLoader(train, 2, seed=1, **kw), T.WindowLoader(train.pairs(), 2, seed=1, **kw), epochs=1) == 2


# --------------------------------------------------------------------------------------------------------------- end to end
def _clip(n, seed):
    """Sums of sinusoids plus noise, inside [-1, 1]."""
    rng = np.random.Generator(np.random.PCG64(seed))
    t = np.arange(n) / 22050.0
    x = sum(a * np.sin(2 * np.pi * f * t + p) for a, f, p in zip((0.3, 0.2, 0.1), rng.uniform(100, 3000, 3), rng.uniform(0, 6.28, 3)))
    return np.clip(x + 0.02 * rng.standard_normal(n), -1, 1).astype(np.float32)


def _hp(**over):
    base = dict(sample_rate=22050, n_fft=2048, hop_length=275, win_length=1100, num_mels=80, fmin=95, min_level_db=-100, bits=10, mu_law=True,
                voc_mode='RAW', voc_pad=2, voc_seq_len=550)
    base.update(over)
    return types.SimpleNamespace(**base)


@pytest.fixture(scope='module')
def clips():
    return [_clip(n, s) for n, s in ((4000, 1), (11000, 2), (7301, 3))]


@pytest.mark.parametrize('voc_mode', ['RAW', 'MOL'])
def test_corpus_from_wavs_end_to_end(clips, voc_mode, tmp_path):
    from tacotronv2_wavernn_chinese_amd.frontend import MelFrontEnd
    hp = _hp(voc_mode=voc_mode)
    short = _clip(275 * 10 + 5, 4)                                           # 11 frames < 12: dropped like get_vocoder_datasets drops it
    corpus = D.DeviceCorpus.from_wavs([clips[0], short, clips[1], clips[2]], hp, DEV, batch_clips=2)
    bits, mu_law = (16, False) if voc_mode == 'MOL' else (10, True)
    assert len(corpus) == 3 and (corpus.bits, corpus.mu_law, corpus.n_clipped) == (bits, mu_law, 0)
    assert corpus.frames.tolist() == [1 + len(c) // 275 for c in clips] and corpus.label_len.tolist() == [len(c) for c in clips]
    fe = MelFrontEnd(hp, device=DEV)
    pairs = corpus.pairs()
    for (mel, lab), clip in zip(pairs, clips):
        assert np.array_equal(mel, fe.melspectrogram(clip)[0].cpu().numpy())          # bit-equal to the clip on its own
        want, band = ref_labels(clip, bits, mu_law)
        assert lab.dtype == np.int32 and int(band.sum()) <= 2
        np.testing.assert_array_equal(lab[~band], want[~band])
        assert np.all(np.abs(lab[band] - want[band]) <= 1)
    kw = dict(mode=voc_mode, bits=10, hop_length=275, pad=2, seq_len=550)
    first = [tuple(t.cpu() for t in b) for b in D.DeviceWindowLoader(corpus, 2, seed=9, **kw)]
    # save, then load the list: the same corpus, the same batches
    listing = corpus.save(tmp_path / 'corpus')
    again = D.DeviceCorpus.load(listing, DEV, hop_length=275)
    assert again.stems == corpus.stems and torch.equal(again.labels, corpus.labels) and torch.equal(again.mels, corpus.mels)
    for b, b0 in zip(D.DeviceWindowLoader(again, 2, seed=9, **kw), first):
        assert all(torch.equal(t.cpu(), t0) for t, t0 in zip(b, b0))
    # and the path the parent commit has reads the same files: WindowLoader over read_feature_list of the saved list
    train, test = T.read_feature_list(listing, seq_len=550, hop_length=275, pad=2, test_samples=1)
    assert len(train) == 2 and len(test) == 1
    assert _same_batches(D.DeviceWindowLoader(D.DeviceCorpus.load(train, DEV, hop_length=275), 2, seed=4, **kw), T.WindowLoader(train, 2, seed=4, **kw)) == 2


def test_clipped_input_is_counted(clips):
    loud = clips[0].copy()
    loud[[10, 2000]] = [1.25, -3.0]
    corpus = D.DeviceCorpus.from_wavs([loud, clips[2]], _hp(), DEV)
    assert corpus.n_clipped == 2 and len(corpus) == 2
    lab = corpus.pairs()[0][1]
    assert lab[10] == 1023 and lab[2000] == 0


@pytest.mark.parametrize('mode', ['RAW', 'MOL'])
def test_training_loss_on_a_device_batch_equals_the_host_batch(mode):
    """The inputs are bit-equal, so the loss is: anything else is a bug in how the batch is laid out or handed over."""
    from tacotronv2_wavernn_chinese_amd.synth import DEFAULT_DIMS
    from tacotronv2_wavernn_chinese_amd.vocoder import WaveRNN
    torch.manual_seed(0)
    model = WaveRNN(**DEFAULT_DIMS, mode=mode)
    model.verbose = False
    model.to(DEV).train()
    kw = dict(mode=mode, bits=10, hop_length=275, pad=2, seq_len=550)
    corpus = D.DeviceCorpus.from_pairs(_pairs([14, 20, 31], 80, 275, 16 if mode == 'MOL' else 10, 3), DEV, hop_length=275)
    x, y, m = next(iter(D.DeviceWindowLoader(corpus, 2, seed=2, **kw)))
    x0, y0, m0 = next(iter(T.WindowLoader(corpus.pairs(), 2, seed=2, **kw)))
    a = model.training_loss(x, m, y).detach().cpu()
    b = model.training_loss(x0.to(DEV), m0.to(DEV), y0.to(DEV)).detach().cpu()
    print(f'\n[training_loss {mode}] device batch {float(a)!r}, host batch {float(b)!r}')
    assert torch.isfinite(a) and torch.equal(a, b)


def test_preprocess_and_train_command_lines(clips, tmp_path):
    """`wavernn_preprocess.py` writes the list and the arrays; `wavernn_train.py --wav_dir` trains from the same folder and leaves the
    latest checkpoint.  Each child has its own time limit; the second only starts after the first succeeded."""
    from tacotronv2_wavernn_chinese_amd.dsp import save_wav
    from tacotronv2_wavernn_chinese_amd.hparams import DEFAULT_HPARAMS
    wav_dir, out_dir = tmp_path / 'wavs', tmp_path / 'data'
    wav_dir.mkdir()
    for i, c in enumerate(clips):
        save_wav(c, wav_dir / f'clip{i}.wav', 22050)
    hp_file = tmp_path / 'tiny_hparams.py'
    hp_file.write_text(open(DEFAULT_HPARAMS).read() + '\nvoc_batch_size = 2\nvoc_seq_len = hop_length * 2\nvoc_test_samples = 1\n')
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'wavernn_preprocess.py'), '--wav_dir', str(wav_dir), '--out_dir', str(out_dir),
                        '--hp_file', str(hp_file)], cwd=tmp_path, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert '3 utterances of 3 files' in r.stdout and '0 clipped samples' in r.stdout
    lines = (out_dir / 'wavernn_training_data.txt').read_text().splitlines()
    assert [l.split('|')[3] for l in lines] == ['clip0', 'clip1', 'clip2']
    for l, c in zip(lines, clips):
        q, m = l.split('|')[0], l.split('|')[2]
        assert np.load(q).shape == (len(c),) and np.load(q).dtype == np.int32 and np.load(m).shape == (1 + len(c) // 275, 80)
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'wavernn_train.py'), '--wav_dir', str(wav_dir), '--hp_file', str(hp_file),
                        '--total_steps', '2'], cwd=tmp_path, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert 'Training Complete.' in r.stdout and '2 training utterances' in r.stdout
    assert (tmp_path / 'logs_wavernn' / 'checkpoints' / 'latest_weights.pyt').exists()
