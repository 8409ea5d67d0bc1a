"""The training-data side without a GPU: the two quantisers' NumPy mirrors, the draw `DeviceWindowLoader` shares with `WindowLoader`,
the errors that must fire before anything native runs, the argument checks of `wrnn_quantise` / `wrnn_collate_windows`, and the list
file `DeviceCorpus.save` writes.  The kernels themselves are tested on the MI355X in test_gpu_dataset.py."""

import numpy as np
import pytest
import torch

from tacotronv2_wavernn_chinese_amd import _cabi, dataset as D, dsp, train as T

KW = dict(hop_length=275, pad=2, seq_len=550)     # win = 6: 13 frames is the shortest utterance a window can be drawn from


@pytest.mark.parametrize('bits', [9, 10, 16])
def test_quantiser_mirrors_on_hand_values(bits):
    mu = 2 ** bits
    got = dsp.encode_mu_law(np.array([0.0, 1.0, -1.0], np.float32), mu)
    assert got.dtype == np.float64 and got.tolist() == [2 ** (bits - 1), mu - 1, 0]
    lin = dsp.float_2_label(np.array([0.0, 1.0, -1.0], np.float32), bits)
    assert lin.dtype == np.float64 and lin[0] == (mu - 1) / 2        # x.5: the collate's astype(int64) truncates it
    assert lin.astype(np.int64).tolist() == [2 ** (bits - 1) - 1, mu - 1, 0]
    with pytest.raises(AssertionError):
        dsp.float_2_label(np.array([1.5]), bits)                      # the reference asserts |x| <= 1 (dsp.py:13)


@pytest.mark.parametrize('bits', [9, 10])
def test_mu_law_round_trip_is_within_one_step(bits):
    """decode(encode(x)) lands in x's own quantisation cell or a neighbour: |error| <= the width of the cell around x, which is
    d(decode)/d(label) = (2 / mu) * ln(1 + mu) * (1 + mu |x|) / mu at x."""
    mu = 2 ** bits - 1
    x = np.concatenate([np.linspace(-1, 1, 4001), np.clip(0.3 * np.random.Generator(np.random.PCG64(5)).standard_normal(20000), -1, 1)])
    back = dsp.decode_mu_law(dsp.encode_mu_law(x, 2 ** bits), 2 ** bits)
    step = 2.0 / mu * np.log1p(mu) * (1.0 + mu * np.abs(x)) / mu
    assert np.all(np.abs(back - x) <= step)
    labels = dsp.encode_mu_law(x, 2 ** bits)
    assert labels.min() == 0 and labels.max() == mu and np.all(labels == np.floor(labels))


def _expected_draws(frames, batch_size, seed, *, hop_length, pad, seq_len):
    """What `WindowLoader.__iter__` + `collate_windows` consume from the generator, restated: one permutation per epoch, then per batch
    one integers(0, room) per utterance in the batch's order."""
    rng = np.random.Generator(np.random.PCG64(seed))
    win = seq_len // hop_length + 2 * pad
    while True:
        order = rng.permutation(len(frames))
        for i in range(0, len(order), batch_size):
            utt = order[i:i + batch_size]
            yield utt, np.array([int(rng.integers(0, frames[u] - 2 - (win + 2 * pad))) for u in utt])


@pytest.mark.parametrize('batch_size', [2, 5])
def test_device_loader_draws_what_window_loader_consumes(batch_size):
    frames = [13, 14, 20, 31, 40]
    rng = np.random.Generator(np.random.PCG64(0))
    pairs = [(rng.random((8, t), dtype=np.float32), rng.integers(0, 1024, size=t * 275)) for t in frames]

    class Hand:                                   # a hand-made corpus: the draw needs len() and frames only, no device
        frames = np.array([13, 14, 20, 31, 40], np.int32)

        def __len__(self):
            return len(self.frames)

    dl = D.DeviceWindowLoader(Hand(), batch_size, mode='RAW', bits=10, seed=3, **KW)
    wl = T.WindowLoader(pairs, batch_size, mode='RAW', bits=10, seed=3, **KW)
    assert len(dl) == len(wl) == (5 + batch_size - 1) // batch_size
    want = _expected_draws(frames, batch_size, 3, **KW)
    for epoch in range(2):
        drawn = list(dl.draws())
        batches = list(wl)
        assert len(drawn) == len(batches) == len(dl)
        for (utt, off), (x, y, m) in zip(drawn, batches):
            u_want, o_want = next(want)
            assert utt.dtype == off.dtype == np.int32
            assert utt.tolist() == u_want.tolist() and off.tolist() == o_want.tolist()
            # and WindowLoader's batch is the windows at exactly those (utterance, offset) pairs
            for r, (u, o) in enumerate(zip(utt, off)):
                s0 = (o + 2) * 275
                assert np.array_equal(m[r].numpy(), pairs[u][0][:, o:o + 6])
                assert np.array_equal(y[r].numpy(), pairs[u][1][s0 + 1:s0 + 551])
    assert len(drawn[-1][0]) == (5 % batch_size or batch_size)       # the last short batch is kept


def test_value_errors_fire_before_the_native_library_is_touched(monkeypatch):
    def boom(*a, **k):
        raise AssertionError('the native library was reached')
    monkeypatch.setattr(_cabi, 'load_library', boom)
    monkeypatch.setattr(_cabi, 'collate_windows', boom)

    class Hand:
        hop_length, n_mels = 275, 80

        def __init__(self, frames):
            self.frames = np.array(frames, np.int32)

        def __len__(self):
            return len(self.frames)

    with pytest.raises(ValueError, match='multiple of hop_length'):
        next(iter(D.DeviceWindowLoader(Hand([20, 20]), 2, mode='RAW', bits=10, hop_length=275, pad=2, seq_len=551)))
    with pytest.raises(ValueError, match='12 frames is too short'):      # one frame short of the 13 a window of 6 (+6) needs
        next(iter(D.DeviceWindowLoader(Hand([20, 12, 20]), 3, mode='RAW', bits=10, **KW)))
    # the same errors, the same text, as the host collate
    pairs = [(np.zeros((80, 12), np.float32), np.zeros(12 * 275, np.int64))]
    with pytest.raises(ValueError, match='12 frames is too short'):
        T.collate_windows(pairs, mode='RAW', bits=10, rng=np.random.Generator(np.random.PCG64(0)), **KW)
    assert D.min_frames(**KW) == 12       # get_vocoder_datasets keeps 12 frames (dataset.py:73-75); the collate then refuses them, as above


def test_native_entry_points_refuse_bad_arguments_without_a_device():
    lib = _cabi.load_library()
    p = 4096                                           # stands for a device pointer: a refused call never reads it
    assert lib.wrnn_quantise(p, 8, 0, 1, p, None, None) == _cabi.ERR_INVALID
    assert lib.wrnn_quantise(p, 8, 17, 1, p, None, None) == _cabi.ERR_INVALID
    assert lib.wrnn_quantise(p, -1, 10, 1, p, None, None) == _cabi.ERR_INVALID
    assert lib.wrnn_quantise(None, 8, 10, 1, p, None, None) == _cabi.ERR_INVALID
    assert lib.wrnn_quantise(p, 8, 10, 1, None, None, None) == _cabi.ERR_INVALID
    assert lib.wrnn_quantise(None, 0, 10, 1, None, None, None) == 0          # n == 0: nothing to do, nothing launched
    good = dict(B=2, n_mels=80, hop=275, pad=2, seq_len=550, sig_bits=10)

    def collate(ptrs=(p,) * 10, **over):
        a = {**good, **over}
        return lib.wrnn_collate_windows(*ptrs[:7], a['B'], a['n_mels'], a['hop'], a['pad'], a['seq_len'], a['sig_bits'], 0, *ptrs[7:], None)

    assert collate(seq_len=551) == _cabi.ERR_INVALID
    assert collate(B=0) == _cabi.ERR_INVALID
    assert collate(sig_bits=17) == _cabi.ERR_INVALID
    assert collate(hop=0) == _cabi.ERR_INVALID
    for k in range(10):
        assert collate(ptrs=tuple(None if i == k else p for i in range(10))) == _cabi.ERR_INVALID, k
    with pytest.raises(_cabi.WrnnError, match='WRNN_ERR_INVALID'):
        _cabi.quantise(p, 8, 17, True, p, 0, 0)
    with pytest.raises(_cabi.WrnnError, match='WRNN_ERR_INVALID'):
        _cabi.collate_windows(p, p, p, p, p, p, p, 2, 80, 275, 2, 551, 10, False, p, p, p, 0)


def test_a_library_without_the_new_symbols_is_named(monkeypatch):
    """An older build reports ABI 9 too: load_library says which symbol it lacks instead of failing later with an AttributeError."""
    monkeypatch.setattr(_cabi, '_lib', None)
    monkeypatch.setattr(_cabi, 'EXPORTED_SYMBOLS', _cabi.EXPORTED_SYMBOLS + ('wrnn_not_in_this_build',))
    with pytest.raises(RuntimeError, match='wrnn_not_in_this_build'):
        _cabi.load_library()
    monkeypatch.undo()
    assert hasattr(_cabi.load_library(), 'wrnn_collate_windows')


def test_saved_list_round_trips_through_read_feature_list(tmp_path):
    """`save` on a hand-made corpus (host tensors stand in for the device buffers): the files have the reference's layout and
    `read_feature_list` reads fields 0 and 2 of every line."""
    rng = np.random.Generator(np.random.PCG64(1))
    frames = [13, 11, 20]                              # 11 frames: too short for one window, read_feature_list drops it
    pairs = [(rng.random((80, t), dtype=np.float32), rng.integers(0, 1024, size=t * 275).astype(np.int32)) for t in frames]
    labels = torch.from_numpy(np.concatenate([w for _, w in pairs]))
    mels = torch.from_numpy(np.concatenate([np.ascontiguousarray(m.T).reshape(-1) for m, _ in pairs]))
    lens = [t * 275 for t in frames]
    corpus = D.DeviceCorpus(labels, mels, np.cumsum([0] + lens[:-1]), lens, np.cumsum([0] + frames[:-1]) * 80, frames, 80, ['a', 'b', 'c'],
                            hop_length=275, sample_rate=22050)
    assert len(corpus) == 3 and corpus.frames.tolist() == frames
    for (m, w), (m0, w0) in zip(corpus.pairs(), pairs):
        assert np.array_equal(m, m0) and np.array_equal(w, w0)
    listing = corpus.save(tmp_path / 'out')
    lines = listing.read_text().splitlines()
    assert listing.name == 'wavernn_training_data.txt' and len(lines) == 3
    q, m1, m2, stem = lines[0].split('|')
    assert m1 == m2 and stem == 'a' and q.endswith('quant/a.npy') and m1.endswith('mel/a.npy')
    assert np.load(q).dtype == np.int32 and np.load(m1).shape == (13, 80) and np.load(m1).dtype == np.float32
    train, test = T.read_feature_list(listing, test_samples=0, **KW)
    assert sorted(train) == sorted((l.split('|')[0], l.split('|')[2]) for l in (lines[0], lines[2])) and test == []
    batches = list(T.WindowLoader(train, 2, mode='RAW', bits=10, seed=0, **KW))
    assert len(batches) == 1 and tuple(batches[0][2].shape) == (2, 80, 6)
    with pytest.raises(ValueError, match='labels for 13 frames'):        # an utterance with fewer labels than its windows can reach
        D.DeviceCorpus(labels, mels, [0], [100], [0], [13], 80, ['a'], hop_length=275)
