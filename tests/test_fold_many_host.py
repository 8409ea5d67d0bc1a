"""Host side of fold mode for several utterances in one call (ABI 8): `wrnn_plan_folded` against `vocoder.fold_count`, the joint cost model
`fold_plan_many` against an independent enumeration of its candidates, and the argument checks of `generate_many(batched=True)` that must
fire before any device work.  No GPU."""
import numpy as np
import pytest

HOP = 275
# the five workloads of tools/fold_many_latency.py, in mel frames
WORKLOADS = {'4x401': [401] * 4, '401_240_160_80': [401, 240, 160, 80], '8x80': [80] * 8,
             'mixed8': [120, 90, 60, 45, 30, 200, 150, 100], '2x401': [401] * 2}


def _plan_or_none(frames, target, overlap):
    from tacotronv2_wavernn_chinese_amd import _cabi
    try:
        return _cabi.plan_folded(frames, HOP, target, overlap)
    except _cabi.WrnnError as e:
        assert e.code == _cabi.ERR_INVALID
        return None


def test_plan_folded_is_fold_count_on_2000_random_triples():
    from tacotronv2_wavernn_chinese_amd.vocoder import fold_count
    rng = np.random.Generator(np.random.PCG64(8))
    frames = rng.integers(1, 501, size=2000)
    target = rng.integers(1, 12001, size=2000)
    overlap = rng.integers(0, 601, size=2000)
    no_fold = 0
    for f, t, o in zip(frames.tolist(), target.tolist(), overlap.tolist()):
        want = fold_count(f * HOP, t, o)
        got = _plan_or_none([f], t, o)
        if want < 1:
            no_fold += 1
            assert got is None, (f, t, o)
        else:
            assert got is not None and got[0].tolist() == [0, want] and got[1] == t + 2 * o, (f, t, o, want, got)
    assert no_fold > 0   # frames = 1 or 2 with overlap > their length: the error path is part of the sample
    # several utterances: the prefix of the single-utterance counts
    for k in range(0, 2000, 8):
        fs, t, o = frames[k:k + 8].tolist(), int(target[k]), int(overlap[k])
        counts = [fold_count(f * HOP, t, o) for f in fs]
        got = _plan_or_none(fs, t, o)
        if min(counts) < 1:
            assert got is None
        else:
            assert got[0].tolist() == [0] + np.cumsum(counts).tolist()


def test_plan_folded_exact_division_no_fold_and_bad_arguments():
    from tacotronv2_wavernn_chinese_amd import _cabi
    fold0, steps = _cabi.plan_folded([24], HOP, 550, 100)   # (24 * 275 - 100) / 650 = 10 exactly: no remainder fold
    assert fold0.tolist() == [0, 10] and steps == 750
    assert _cabi.plan_folded([24, 24], HOP, 550, 100)[0].tolist() == [0, 10, 20]
    with pytest.raises(_cabi.WrnnError, match='WRNN_ERR_INVALID'):
        _cabi.plan_folded([30, 1], HOP, 550, 300)            # 275 samples < overlap: floor division gives -1, + 1 = 0 folds
    for bad in (dict(frames=[0]), dict(frames=[-3]), dict(target=0), dict(overlap=-1), dict(hop=0), dict(frames=[])):
        kw = dict(frames=[30], hop=HOP, target=550, overlap=100)
        kw.update(bad)
        with pytest.raises(_cabi.WrnnError):
            _cabi.plan_folded(kw['frames'], kw['hop'], kw['target'], kw['overlap'])
    lib = _cabi.load_library()
    assert lib.wrnn_plan_folded(None, 1, HOP, 550, 100, None, None) == _cabi.ERR_INVALID


@pytest.mark.parametrize('T,target,overlap', [(21, 550, 100), (401, 1165, 550), (24, 550, 100), (30, 11000, 550), (3, 400, 550), (401, 11000, 0)])
def test_plan_folded_with_one_utterance_is_wrnn_plans_formula(T, target, overlap):
    """wrnn_plan(h, 1, T, batched = 1, ...) needs a handle (a device); its formula (api.hip, fatchord_version.py:319-325) restated here."""
    total = T * HOP
    num_folds = (total - overlap) // (target + overlap)
    if total - (num_folds * (overlap + target) + overlap) != 0:
        num_folds += 1
    got = _plan_or_none([T], target, overlap)
    if num_folds < 1:
        assert got is None
    else:
        assert got[0].tolist() == [0, num_folds] and got[1] == target + 2 * overlap


def test_fold_plan_many_for_one_utterance_is_fold_plan():
    from tacotronv2_wavernn_chinese_amd.vocoder import fold_plan, fold_plan_many
    for T in (21, 30, 45, 80, 120, 240, 401, 1000):
        for overlap in (100, 550):
            for teams in (1, 4, 8):
                for mode in ('RAW', 'MOL'):
                    for min_target in (0, 5500):
                        assert fold_plan_many([T * HOP], overlap, teams, mode, min_target) == fold_plan(T * HOP, overlap, teams, mode, min_target), \
                            (T, overlap, teams, mode, min_target)


@pytest.mark.parametrize('name', sorted(WORKLOADS))
@pytest.mark.parametrize('mode', ['RAW', 'MOL'])
def test_fold_plan_many_is_the_cheapest_candidate(name, mode):
    from tacotronv2_wavernn_chinese_amd.vocoder import fold_count, fold_plan_many, fold_target, predicted_loop_us
    lens = [t * HOP for t in WORKLOADS[name]]
    overlap, teams = 550, 8
    target, rows, cost = fold_plan_many(lens, overlap, teams, mode)
    assert rows == sum(fold_count(t, target, overlap) for t in lens)
    assert cost == predicted_loop_us(rows, target + 2 * overlap, teams, mode)
    # every candidate target, enumerated independently: none is cheaper, and none as cheap is larger
    for t in lens:
        for n in range(1, 2 * 8 * teams + 1):
            cand = fold_target(t, overlap, n)
            counts = [fold_count(x, cand, overlap) for x in lens]
            if min(counts) < 1:
                continue
            c = predicted_loop_us(sum(counts), cand + 2 * overlap, teams, mode)
            assert cost <= c * (1.0 + 1e-9), (cand, c, cost)
            if c == cost:
                assert cand <= target   # ties go to the larger target (fewer crossfades)


def test_fold_plan_many_matches_the_predictions_the_feature_was_planned_on():
    """The joint plans of the four queued-clip workloads of DESIGN.md 3.10 (cost model on STEP_US, 8 teams, RAW, overlap 550)."""
    from tacotronv2_wavernn_chinese_amd.vocoder import fold_plan, fold_plan_many
    want = {'4x401': (6308, 64, 55.7, 68.1), '401_240_160_80': (3300, 64, 33.1, 48.2), '8x80': (2132, 64, 24.3, 69.7), 'mixed8': (None, 64, 31.3, 68.2)}
    for name, (target, rows, joint_ms, seq_ms) in want.items():
        lens = [t * HOP for t in WORKLOADS[name]]
        got = fold_plan_many(lens, 550, 8, 'RAW')
        assert got[1] == rows and (target is None or got[0] == target)
        assert round(got[2] / 1e3, 1) == joint_ms
        assert round(sum(fold_plan(t, 550, 8, 'RAW')[2] for t in lens) / 1e3, 1) == seq_ms


def test_fold_plan_many_respects_min_target():
    from tacotronv2_wavernn_chinese_amd.vocoder import fold_count, fold_plan_many, fold_target
    for name, frames in WORKLOADS.items():
        lens = [t * HOP for t in frames]
        free = fold_plan_many(lens, 550, 8, 'RAW')
        for min_target in (3000, 5500, 20000, 10 ** 7):
            target, rows, cost = fold_plan_many(lens, 550, 8, 'RAW', min_target)
            assert target >= min_target or target == fold_target(max(lens), 550, 1), (name, min_target, target)
            assert rows == sum(fold_count(t, target, 550) for t in lens)
            assert cost >= free[2] * (1.0 - 1e-9)
        assert fold_plan_many(lens, 550, 8, 'RAW', 10 ** 7)[1] == len(lens)   # nothing admissible but one fold per utterance


def _cpu_model():
    from tacotronv2_wavernn_chinese_amd.synth import DEFAULT_DIMS
    from tacotronv2_wavernn_chinese_amd.vocoder import WaveRNN
    m = WaveRNN(**DEFAULT_DIMS, mode='RAW')
    m.verbose = False
    return m


def test_generate_many_batched_rejects_short_clips_before_any_device_work():
    from tacotronv2_wavernn_chinese_amd.synth import make_mels
    m = _cpu_model()
    clips = [make_mels(1, 1, 30)[0], make_mels(2, 1, 20)[0]]
    with pytest.raises(ValueError, match=r'operands could not be broadcast together with shapes \(5225,\) \(5500,\) \(5225,\)'):
        m.generate_many(clips, batched=True, target=550, overlap=100)
    with pytest.raises(ValueError, match='broadcast'):
        m.generate_many(clips, batched=True, target='auto', epilogue='device')


def test_generate_many_batched_rejects_reference_noise_and_bad_arguments():
    from tacotronv2_wavernn_chinese_amd.synth import make_mels
    m = _cpu_model()
    clips = [make_mels(1, 1, 30)[0], make_mels(2, 1, 24)[0]]
    with pytest.raises(ValueError, match='reference'):
        m.generate_many(clips, batched=True, target=550, overlap=100, noise_mode='reference')
    with pytest.raises(ValueError, match='epilogue'):
        m.generate_many(clips, batched=True, target=550, overlap=100, epilogue='gpu')
    with pytest.raises(ValueError):
        m.generate_many([], batched=True)
