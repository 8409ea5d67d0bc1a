"""Host side of per-request noise seeds (ABI 9, `seeds=`): the argument checks that must fire before the native library is touched, the
reduction of the seeds mod 2**64, the layout of the new `wrnn_sample_opts` field, and the sharding recipe of INTEGRATION.md -- the clip -> seed
pairing does not depend on the world size.  No GPU."""
import ctypes as C

import numpy as np
import pytest


def _cpu_model():
    from tacotronv2_wavernn_chinese_amd.synth import DEFAULT_DIMS
    from tacotronv2_wavernn_chinese_amd.vocoder import WaveRNN
    m = WaveRNN(**DEFAULT_DIMS, mode='RAW')
    m.verbose = False

    def no_native():
        raise AssertionError('the native library was asked before the arguments were checked')
    m.native = no_native
    return m


def _clips():
    from tacotronv2_wavernn_chinese_amd.synth import make_mels
    return [make_mels(1, 1, 30)[0], make_mels(2, 1, 24)[0]]


def test_seeds_are_reduced_mod_2_64():
    from tacotronv2_wavernn_chinese_amd.vocoder import request_seeds
    got = request_seeds([0, 2 ** 64 + 5, -1, 0xA5A5_0001_0000_F01D, 2 ** 63], 5)
    assert got.dtype == np.uint64
    assert got.tolist() == [0, 5, 2 ** 64 - 1, 0xA5A5_0001_0000_F01D, 2 ** 63]
    assert request_seeds(np.array([7, 8], np.uint64), 2, 'philox').tolist() == [7, 8]
    assert request_seeds((), 0).shape == (0,)


def test_request_seeds_refusals():
    from tacotronv2_wavernn_chinese_amd import _cabi
    from tacotronv2_wavernn_chinese_amd.vocoder import request_seeds
    with pytest.raises(ValueError, match='exclusive'):
        request_seeds([1, 2], 2, seed=0)
    with pytest.raises(ValueError, match='expected 3, got 2'):
        request_seeds([1, 2], 3)
    for mode in ('injected', 'argmax', 'reference', _cabi.NOISE_INJECTED, _cabi.NOISE_ARGMAX):
        with pytest.raises(ValueError, match='philox'):
            request_seeds([1, 2], 2, mode)


@pytest.mark.parametrize('batched', [False, True])
def test_generate_many_checks_seeds_before_any_device_work(batched):
    m = _cpu_model()
    kw = dict(batched=batched, target=550, overlap=100)
    with pytest.raises(ValueError, match='exclusive'):
        m.generate_many(_clips(), seeds=[1, 2], seed=3, **kw)
    with pytest.raises(ValueError, match='expected 2, got 3'):
        m.generate_many(_clips(), seeds=[1, 2, 3], **kw)
    with pytest.raises(ValueError, match='expected 2, got 1'):
        m.generate_many(_clips(), seeds=[1], **kw)
    for mode in ('injected', 'argmax', 'reference'):
        with pytest.raises(ValueError, match='philox'):
            m.generate_many(_clips(), seeds=[1, 2], noise_mode=mode, **kw)


def test_generate_raw_and_folded_check_seeds_before_any_device_work():
    from tacotronv2_wavernn_chinese_amd import _cabi
    m = _cpu_model()
    batch = np.zeros((2, 80, 30), np.float32)
    with pytest.raises(ValueError, match='exclusive'):
        m.generate_raw(batch, False, 11000, 550, seeds=[1, 2], seed=0)
    with pytest.raises(ValueError, match='expected 2, got 3'):
        m.generate_raw(batch, False, 11000, 550, seeds=[1, 2, 3])
    with pytest.raises(ValueError, match='unbatched'):
        m.generate_raw(batch[:1], True, 550, 100, seeds=[1])
    for mode in ('injected', 'argmax', 'reference', _cabi.NOISE_INJECTED):
        with pytest.raises(ValueError, match='philox'):
            m.generate_raw(batch, False, 11000, 550, seeds=[1, 2], noise_mode=mode)
    with pytest.raises(ValueError, match='exclusive'):
        m.generate_raw_folded(batch, [30, 24], 550, 100, seeds=[1, 2], seed=9)
    with pytest.raises(ValueError, match='expected 2, got 1'):
        m.generate_raw_folded(batch, [30, 24], 550, 100, seeds=[1])
    for mode in ('injected', 'argmax', _cabi.NOISE_ARGMAX):
        with pytest.raises(ValueError, match='philox'):
            m.generate_raw_folded(batch, [30, 24], 550, 100, seeds=[1, 2], noise_mode=mode)


def test_generate_many_without_seeds_still_draws_one_call_seed(monkeypatch):
    """`seeds=None` keeps the one draw from the torch generator; with `seeds` nothing is drawn and no call seed is passed on."""
    import torch
    m = _cpu_model()
    seen = []

    def fake_raw(batch, *a, **kw):
        seen.append(kw)
        raise RuntimeError('stop here')
    monkeypatch.setattr(m, 'generate_raw', fake_raw)
    torch.manual_seed(5)
    want = int(torch.randint(0, 2 ** 62, (1,)).item())
    after = int(torch.randint(0, 2 ** 62, (1,)).item())
    torch.manual_seed(5)
    with pytest.raises(RuntimeError, match='stop here'):
        m.generate_many(_clips())
    assert seen[-1]['seed'] == want and 'seeds' not in seen[-1]
    with pytest.raises(RuntimeError, match='stop here'):
        m.generate_many(_clips(), seeds=[2 ** 64 + 1, 4])
    assert 'seed' not in seen[-1] and [int(s) for s in seen[-1]['seeds']] == [1, 4]
    assert int(torch.randint(0, 2 ** 62, (1,)).item()) == after   # the seeded call consumed nothing from the generator


def test_sample_opts_carries_the_field_behind_team2_segment():
    from tacotronv2_wavernn_chinese_amd import _cabi
    assert _cabi.ABI_VERSION == 9
    names = [f[0] for f in _cabi.SampleOpts._fields_]
    assert names[-2:] == ['team2_segment', 'utt_seeds_dev']
    assert _cabi.SampleOpts.utt_seeds_dev.offset == _cabi.SampleOpts.team2_segment.offset + 4
    assert C.sizeof(_cabi.SampleOpts) == _cabi.SampleOpts.utt_seeds_dev.offset + 8 == 88


@pytest.mark.parametrize('balance', [False, True])
def test_the_sharding_recipe_pairs_clip_and_seed_at_every_world_size(monkeypatch, balance):
    import torch.distributed as dist
    from tacotronv2_wavernn_chinese_amd.sharding import generate_sharded
    lens = [30, 21, 45, 24, 60, 22, 33, 27, 51, 26, 38]
    mels = [np.full((80, t), float(i), np.float32) for i, t in enumerate(lens)]
    S = [0xC0DE_0000_0000_0000 + 977 * i for i in range(len(lens))]

    class StubModel:
        def __init__(self):
            self.calls = []

        def generate_many(self, ms, seeds=None):
            assert len(ms) == len(seeds)
            self.calls += [(int(m[0, 0]), int(s)) for m, s in zip(ms, seeds)]
            return [np.zeros(3) for _ in ms]
    pairings = {}
    for world in (1, 2, 8):
        seen = []
        for rank in range(world):
            monkeypatch.setattr(dist, 'is_initialized', lambda: True)
            monkeypatch.setattr(dist, 'get_rank', lambda r=rank: r)
            monkeypatch.setattr(dist, 'get_world_size', lambda w=world: w)
            monkeypatch.setattr(dist, 'barrier', lambda: None)
            model = StubModel()
            generate_sharded(None, mels, gather=False, balance=balance,
                             generate_many=lambda idx, ms: model.generate_many(ms, seeds=[S[i] for i in idx]))
            seen += model.calls
        assert sorted(c for c, _ in seen) == list(range(len(lens)))   # every clip once
        pairings[world] = dict(seen)
    assert pairings[1] == pairings[2] == pairings[8] == {i: S[i] for i in range(len(lens))}
