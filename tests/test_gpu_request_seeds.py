"""Per-request noise seeds (`wrnn_sample_opts.utt_seeds_dev`, `seeds=`; DESIGN.md 3.10 "Noise").

Contract: every Philox draw of utterance b is keyed as a call on that clip ALONE with `seed = S[b]` keys it -- key = all 64 bits of S[b], row word
= the row's index INSIDE its utterance (fold i of a folded call, 0 of an unbatched one).  So the oracle reference for utterance b is the oracle on
clip b alone, driven along the GPU's trajectory, with the noise `_philox_q(S[b], steps, range(n_b))`: LOCAL rows, the clip's own seed; and a clip's
rows are bit-equal to the solo call on the same kernel, whatever else is in the call and wherever the clip stands.  The seeds have their high 32 bits
set, and two seeds of every call share their low 32 bits: a key truncated to 32 bits gives those two clips the same draws where their rows have the
same index.  Shapes: the smallest of tests/test_gpu_fold_many.py; near-ties are bounded by `bound_near_ties`, unchanged.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from tests.parity_util import MOL_LSB, bound_near_ties, check_on_gpu_trajectory_mol, check_on_gpu_trajectory_raw, parity_report
from tests.test_gpu_fold_many import FOUR, _clips, _folds_of, _mol, _pad, _raw

pytestmark = pytest.mark.gpu
HOP = 275
# S[0] and S[2] differ above bit 32 only
S4 = [0xA5A5_0001_0000_F01D, 0x1234_5678_9ABC_DEF0, 0x5A5A_0002_0000_F01D, 0xFFFF_FFFF_0000_0007]
_SOLO = {}


def _q(seed, steps, n):
    from tests.test_gpu_baseline_sizes import _philox_q
    return _philox_q(seed, steps, list(range(n)))


def _check_folded_raw(tag, om, clips, seeds, res, target, overlap):
    """Every step of every row: utterance b against the oracle on clip b alone under (seeds[b], LOCAL fold index)."""
    from oracle import oracle as orc
    lab, smp, fold0 = res['labels'].cpu().numpy(), res['samples'].cpu().numpy(), res['fold0']
    steps = target + 2 * overlap
    assert lab.shape == (fold0[-1], steps)
    compared, near = 0, []
    for b, clip in enumerate(clips):
        cm, ca = _folds_of(om, clip, target, overlap)
        rs = list(range(fold0[b], fold0[b + 1]))
        assert cm.shape[0] == len(rs)
        q = _q(seeds[b], steps, len(rs))
        st = check_on_gpu_trajectory_raw(lab[rs].T, smp[rs].T, lambda xf: om.loop(cm, ca, orc.NOISE_EXPO, q, x_forced=xf))
        compared += st['compared']
        near += [(t, rs[r], d) for t, r, d in st['near_ties']]
    bound_near_ties(tag, compared, near)
    assert compared == lab.size


def _rows_of(res, b):
    f0 = res['fold0']
    return res['labels'][f0[b]:f0[b + 1]], res['samples'][f0[b]:f0[b + 1]]


def _four_cs4():
    """The folded call of case 1, run once and shared (read-only) by cases 1, 2 and 9."""
    if 'four' not in _SOLO:
        from tacotronv2_wavernn_chinese_amd import _cabi
        m, _, _ = _raw()
        clips = _clips(FOUR)
        batch, frames = _pad(clips)
        res = m.generate_raw_folded(batch, frames, 550, 100, seeds=S4, batch_rows=4)
        assert res['fold0'].tolist() == [0, 9, 22, 32, 42] and res['steps'] == 750
        assert m.last_timing['kernel'] == _cabi.KERNEL_BATCH_CS and m.last_timing['rows'] == 42
        _SOLO['four'] = (clips, res)
    return _SOLO['four']


def test_batch_cs_four_rows_per_team_every_step():
    _, om, _ = _raw()
    clips, res = _four_cs4()
    _check_folded_raw('request seeds: 4 utterances x 42 folds, batch_cs 4 rows/team', om, clips, S4, res, 550, 100)
    # S[0] and S[2] share their low 32 bits: the same local rows draw different noise
    l0, l2 = _rows_of(res, 0)[0], _rows_of(res, 2)[0]
    assert not torch.equal(l0[:9], l2[:9])


def test_position_and_company_do_not_matter():
    from tacotronv2_wavernn_chinese_amd import _cabi
    m, _, _ = _raw()
    clips, res = _four_cs4()
    batch_r, frames_r = _pad(clips[::-1])
    rev = m.generate_raw_folded(batch_r, frames_r, 550, 100, seeds=S4[::-1], batch_rows=4)
    assert rev['fold0'].tolist() == [0, 10, 20, 33, 42]
    batch_2, frames_2 = _pad([clips[1], clips[3]])
    two = m.generate_raw_folded(batch_2, frames_2, 550, 100, seeds=[S4[1], S4[3]], kernel='batch_cs', batch_rows=4)
    assert two['fold0'].tolist() == [0, 13, 23] and m.last_timing['kernel'] == _cabi.KERNEL_BATCH_CS
    for b, clip in enumerate(clips):
        lab, smp = _rows_of(res, b)
        lab_r, smp_r = _rows_of(rev, 3 - b)
        assert torch.equal(lab, lab_r) and torch.equal(smp, smp_r), b
        solo = m.generate_raw(clip[None], True, 550, 100, seed=S4[b], kernel=_cabi.KERNEL_BATCH_CS, batch_rows=4)
        assert torch.equal(solo['labels'], lab) and torch.equal(solo['samples'], smp), b
    for b, pos in ((1, 0), (3, 1)):
        lab, smp = _rows_of(res, b)
        lab_2, smp_2 = _rows_of(two, pos)
        assert torch.equal(lab, lab_2) and torch.equal(smp, smp_2), b


def test_batch_cs_eight_rows_per_team_two_passes_every_step():
    """250/50: 90 rows x 350 steps, 12 batches of 8 on 8 teams: the second quad of a team batch, finished by the shadow wave."""
    from tacotronv2_wavernn_chinese_amd import _cabi
    m, om, _ = _raw()
    clips = _clips(FOUR)
    batch, frames = _pad(clips)
    res = m.generate_raw_folded(batch, frames, 250, 50, seeds=S4)
    assert res['fold0'].tolist() == [0, 20, 48, 70, 90] and res['steps'] == 350
    assert m.last_timing['kernel'] == _cabi.KERNEL_BATCH_CS and m.last_timing['rows'] == 90
    _check_folded_raw('request seeds: 4 utterances x 90 folds, batch_cs 8 rows/team', om, clips, S4, res, 250, 50)
    assert not torch.equal(_rows_of(res, 0)[0][:20], _rows_of(res, 2)[0][:20])


def test_team2_segmented_every_step_and_equal_to_the_solo_call():
    """6 rows x 2 800 steps in three launches: the 32-step block draw and its resume behind a segment boundary."""
    from tacotronv2_wavernn_chinese_amd import _cabi
    m, om, _ = _raw()
    clips = _clips((21, 24), seed0=4100)
    seeds = [S4[0], S4[2]]
    batch, frames = _pad(clips)
    res = m.generate_raw_folded(batch, frames, 2600, 100, seeds=seeds, team2_segment=1024)
    assert res['fold0'].tolist() == [0, 3, 6] and res['steps'] == 2800
    assert m.last_timing['kernel'] == _cabi.KERNEL_TEAM2 and m.last_timing['launches'] == 3
    _check_folded_raw('request seeds: 2 utterances x 6 folds, team2 in 3 segments', om, clips, seeds, res, 2600, 100)
    assert not torch.equal(_rows_of(res, 0)[0], _rows_of(res, 1)[0])
    for b, clip in enumerate(clips):
        solo = m.generate_raw(clip[None], True, 2600, 100, seed=seeds[b], kernel=_cabi.KERNEL_TEAM2, team2_segment=1024)
        lab, smp = _rows_of(res, b)
        assert torch.equal(solo['labels'], lab) and torch.equal(solo['samples'], smp), b


def test_mol_9bit_batch_cs_every_step():
    """MOL: the noise is prepared for the rows whose sampler the C wave of the SIMD runs, not for the thread's own row."""
    from tacotronv2_wavernn_chinese_amd import _cabi
    from tests import philox_ref
    m, om, _ = _mol()
    clips = _clips((21, 30, 24), seed0=4200)
    seeds = S4[:3]
    batch, frames = _pad(clips)
    res = m.generate_raw_folded(batch, frames, 550, 100, seeds=seeds)
    assert res['fold0'].tolist() == [0, 9, 22, 32] and res['steps'] == 750
    assert m.last_timing['kernel'] == _cabi.KERNEL_BATCH_CS
    smp, mix, fold0 = res['samples'].cpu().numpy(), res['labels'].cpu().numpy(), res['fold0']
    compared = mism = 0
    worst = 0.0
    for b, clip in enumerate(clips):
        cm, ca = _folds_of(om, clip, 550, 100)
        rs = list(range(fold0[b], fold0[b + 1]))
        u_mix, u_log = philox_ref.philox_mol_uniforms(seeds[b], 0, 750, list(range(len(rs))))
        assert u_mix.min() >= 1e-5 and u_mix.max() <= 1.0 - 1e-5 and u_log.min() >= 1e-5 and u_log.max() <= 1.0 - 1e-5
        st = check_on_gpu_trajectory_mol(np.ascontiguousarray(smp[rs].T), np.ascontiguousarray(mix[rs].T),
                                         lambda xf: om.loop(cm, ca, 0, u_mix, u_log, x_forced=xf))
        compared, mism, worst = compared + st['compared'], mism + st['index_mismatches'], max(worst, st['max_err'])
    parity_report(f'request seeds MOL: 3 utterances x 32 folds x 750 steps, batch_cs, device Philox noise replayed: steps compared {compared}, '
                  f'mixture-index near-ties {mism}, max |sample error| {worst:.3e} = {worst / MOL_LSB:.5f} LSB(9 bit)')
    # the bounds of tests/test_gpu_philox_mol.py::_check (the 2e-5 sample bound is asserted inside check_on_gpu_trajectory_mol)
    assert compared == 32 * 750
    assert mism <= 1 + int(1e-5 * compared)
    assert np.abs(smp).max() <= 1.0
    assert not np.array_equal(smp[0:9], smp[22:31])   # seeds 0 and 2: equal low words, equal local rows


def test_simple_kernel_every_step():
    from tacotronv2_wavernn_chinese_amd import _cabi
    m, om, _ = _raw()
    clips = _clips((21, 23), seed0=4300)
    seeds = [S4[2], S4[0]]
    batch, frames = _pad(clips)
    res = m.generate_raw_folded(batch, frames, 550, 100, seeds=seeds, kernel='simple')
    assert res['fold0'].tolist() == [0, 9, 19] and m.last_timing['kernel'] == _cabi.KERNEL_SIMPLE
    _check_folded_raw('request seeds: 2 utterances x 19 folds, simple', om, clips, seeds, res, 550, 100)
    assert not torch.equal(_rows_of(res, 0)[0], _rows_of(res, 1)[0][:9])


def _ragged(m, clips, seeds, **kw):
    batch, frames = _pad(clips)
    return m.generate_raw(batch, False, 11000, 550, frames=np.asarray(frames, np.int32), seeds=seeds, **kw)


def test_ragged_latency_kernel_rows_equal_the_solo_calls_in_any_order():
    from tacotronv2_wavernn_chinese_amd import _cabi
    m, _, _ = _raw()
    clips = _clips((21, 24, 22), seed0=4500)
    seeds = [S4[0], S4[1], S4[2]]
    res = _ragged(m, clips, seeds)
    assert m.last_timing['kernel'] == _cabi.KERNEL_TEAM2
    perm = [2, 0, 1]
    res_p = _ragged(m, [clips[i] for i in perm], [seeds[i] for i in perm])
    for b, clip in enumerate(clips):
        n = clip.shape[1] * HOP
        solo = m.generate_raw(clip[None], False, 11000, 550, seed=seeds[b], kernel=_cabi.KERNEL_TEAM2)
        assert torch.equal(res['labels'][b, :n], solo['labels'][0]) and torch.equal(res['samples'][b, :n], solo['samples'][0]), b
        p = perm.index(b)
        assert torch.equal(res['labels'][b, :n], res_p['labels'][p, :n]) and torch.equal(res['samples'][b, :n], res_p['samples'][p, :n]), b
    assert not torch.equal(res['labels'][0, :21 * HOP], res['labels'][2, :21 * HOP])


def test_ragged_batch_kernel_every_step_and_any_order():
    """9 clips: more rows than teams, so the batch kernel runs them, ordered by length on the device: the key follows the ROW, not its slot."""
    from oracle import oracle as orc
    from tacotronv2_wavernn_chinese_amd import _cabi
    m, om, _ = _raw()
    frames = (21, 24, 22, 23, 21, 24, 22, 23, 21)
    clips = _clips(frames, seed0=4600)
    seeds = [S4[0], S4[1], S4[2], S4[3]] + [(0xC0DE_0000_0000_0000 + (i << 32) + 0xF01D) for i in range(5)]
    res = _ragged(m, clips, seeds)
    assert m.last_timing['kernel'] == _cabi.KERNEL_BATCH_CS
    lab, smp = res['labels'].cpu().numpy(), res['samples'].cpu().numpy()
    compared, near = 0, []
    for b, clip in enumerate(clips):
        n = frames[b] * HOP
        cm, ca = om.conditioning(clip[None])
        q = _q(seeds[b], n, 1)
        st = check_on_gpu_trajectory_raw(lab[b:b + 1, :n].T, smp[b:b + 1, :n].T, lambda xf: om.loop(cm, ca, orc.NOISE_EXPO, q, x_forced=xf))
        compared += st['compared']
        near += [(t, b, d) for t, _, d in st['near_ties']]
    bound_near_ties('request seeds: 9 ragged utterances, batch_cs, (S[b], row 0) noise', compared, near)
    assert compared == sum(frames) * HOP
    perm = [4, 8, 0, 3, 7, 1, 5, 2, 6]
    res_p = _ragged(m, [clips[i] for i in perm], [seeds[i] for i in perm])
    assert m.last_timing['kernel'] == _cabi.KERNEL_BATCH_CS
    for b in range(9):
        n, p = frames[b] * HOP, perm.index(b)
        assert torch.equal(res['labels'][b, :n], res_p['labels'][p, :n]) and torch.equal(res['samples'][b, :n], res_p['samples'][p, :n]), b
    assert not np.array_equal(lab[0, :21 * HOP], lab[2, :21 * HOP])   # seeds 0 and 2: equal low words, both row 0


def test_generate_many_returns_the_same_clip_wherever_it_is_queued():
    m, _, _ = _raw()
    clips, res = _four_cs4()
    perm = [2, 0, 3, 1]
    for kw in (dict(batched=True, target=550, overlap=100, batch_rows=4), dict(batched=False)):
        a = m.generate_many(clips, None, True, 'device', seeds=S4, **kw)
        p = m.generate_many([clips[i] for i in perm], None, True, 'device', seeds=[S4[i] for i in perm], **kw)
        for b in range(4):
            assert a[b].shape == ((FOUR[b] - 1) * HOP,)
            assert np.array_equal(a[b], p[perm.index(b)]), (kw['batched'], b)
        assert not np.array_equal(a[0][:5000], a[2][:5000])
        if kw['batched']:
            # element b = the tail of the solo folded call's rows
            from tacotronv2_wavernn_chinese_amd import _cabi
            for b, clip in enumerate(clips):
                solo = m.generate_many([clip], None, True, 'device', batched=True, target=550, overlap=100, seeds=[S4[b]], kernel=_cabi.KERNEL_BATCH_CS,
                                       batch_rows=4)
                assert np.array_equal(solo[0], a[b]), b


def test_the_c_abi_refuses_seeds_it_cannot_honour():
    from tacotronv2_wavernn_chinese_amd import _cabi
    m, _, _ = _raw()
    nat = m.native()
    clips = _clips((21, 24))
    batch, frames = _pad(clips)
    mels_t, fr_t = torch.from_numpy(batch).cuda(), torch.tensor(frames, dtype=torch.int32, device='cuda')
    seeds_t = torch.tensor([1, 2], dtype=torch.int64, device='cuda')
    noise = torch.ones((750, 19, 1024), dtype=torch.float32, device='cuda')
    out = torch.full((19, 750), -7.0, dtype=torch.float32, device='cuda')
    torch.cuda.synchronize()

    def opts(**kw):
        o = _cabi.SampleOpts()
        o.struct_size = C.sizeof(_cabi.SampleOpts)
        o.utt_seeds_dev = seeds_t.data_ptr()
        for k, v in kw.items():
            setattr(o, k, v)
        return o
    # injected noise
    o = opts(noise_mode=_cabi.NOISE_INJECTED, noise1_dev=noise.data_ptr())
    rc = nat.lib.wrnn_generate_folded(nat._h, mels_t.data_ptr(), 2, 24, fr_t.data_ptr(), 19, 550, 100, C.byref(o), None, out.data_ptr(), None)
    assert rc == _cabi.ERR_INVALID and 'utt_seeds_dev' in nat.lib.wrnn_last_error(nat._h).decode()
    rc = nat.lib.wrnn_generate(nat._h, mels_t.data_ptr(), 2, 24, 0, 550, 100, C.byref(opts(noise_mode=_cabi.NOISE_ARGMAX)), None, out.data_ptr(), None)
    assert rc == _cabi.ERR_INVALID and 'utt_seeds_dev' in nat.lib.wrnn_last_error(nat._h).decode()
    # one folded utterance through wrnn_generate: `seed` is its key
    rc = nat.lib.wrnn_generate(nat._h, mels_t.data_ptr(), 1, 24, 1, 550, 100, C.byref(opts()), None, out.data_ptr(), None)
    assert rc == _cabi.ERR_INVALID and 'utt_seeds_dev' in nat.lib.wrnn_last_error(nat._h).decode()
    # streams
    st = C.c_void_p()
    rc = nat.lib.wrnn_stream_open(nat._h, 1, C.byref(opts()), C.byref(st))
    assert rc == _cabi.ERR_INVALID and not st.value and 'utt_seeds_dev' in nat.lib.wrnn_last_error(nat._h).decode()
    torch.cuda.synchronize()
    assert bool((out == -7.0).all())   # nothing was launched
    # and the host side: before the library is asked
    with pytest.raises(ValueError, match='exclusive'):
        m.generate_raw_folded(batch, frames, 550, 100, seeds=[1, 2], seed=3)
    with pytest.raises(ValueError, match='unbatched'):
        m.generate_raw(batch[:1], True, 550, 100, seeds=[1])


def test_calls_without_seeds_are_unchanged():
    """The null path of the new branch: one call seed, GLOBAL row indices, as tests/test_gpu_fold_many.py checks it."""
    from oracle import oracle as orc
    from tacotronv2_wavernn_chinese_amd import _cabi
    from tests.test_gpu_baseline_sizes import _philox_q
    from tests.test_gpu_fold_many import _check_raw, _philox
    m, om, _ = _raw()
    seed = 0x0BAD_5EED_0000_F01D
    clips = _clips((21, 24))
    batch, frames = _pad(clips)
    res = m.generate_raw_folded(batch, frames, 550, 100, seed=seed, kernel='batch_cs', batch_rows=4)
    assert res['fold0'].tolist() == [0, 9, 19] and m.last_timing['kernel'] == _cabi.KERNEL_BATCH_CS
    _check_raw('no request seeds: 2 utterances x 19 folds, batch_cs, global rows', om, clips, res, 550, 100, _philox(seed, 750))
    rag = m.generate_raw(batch, False, 11000, 550, frames=np.asarray(frames, np.int32), seed=seed)
    assert m.last_timing['kernel'] == _cabi.KERNEL_TEAM2
    lab, smp = rag['labels'].cpu().numpy(), rag['samples'].cpu().numpy()
    compared, near = 0, []
    for b, clip in enumerate(clips):
        n = frames[b] * HOP
        cm, ca = om.conditioning(clip[None])
        q = _philox_q(seed, n, [b])
        st = check_on_gpu_trajectory_raw(lab[b:b + 1, :n].T, smp[b:b + 1, :n].T, lambda xf: om.loop(cm, ca, orc.NOISE_EXPO, q, x_forced=xf))
        compared += st['compared']
        near += [(t, b, d) for t, _, d in st['near_ties']]
    bound_near_ties('no request seeds: 2 ragged utterances, team2, global rows', compared, near)
    assert compared == sum(frames) * HOP
