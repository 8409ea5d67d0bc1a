"""The time alignment on the GPU (``csrc/align.hip``) against the float64 restatement ``tests/align_ref.py``.

The DP and the backtrack (``wrnn_align_path``) add the same float64 numbers in the same order as the restatement: paths, lengths and
totals are compared with no tolerance.  The cost matrices (``wrnn_align_cost``) come out of a float32 chain (the float32 mel of
``melspec.hip``, float32 cepstra): for every fixture the test evaluates the restatement in float32 as well and takes g = the largest
|float32 restatement - float64 restatement| over the matrix; every cell of the kernel's matrix must lie within K g of the float64
one.  K is the smallest power of two at least twice the worst ratio measured on an MI355X (``profiles/align.txt``): the worst ratio
is 0.77 g (the white-noise pair under the 'tacotron' profile; 0.09 - 0.27 g on the others), so K = 2.  Every cost test prints g, the kernel's error and their ratio before it asserts (``pytest -s``).

The path of a whole-chain call must equal the float64 path on the fixtures ``tests/test_align_host.py`` qualified (every decision along
the path is led by at least 1000 (Ta + Tb) g); the summaries are checked against the float64 formulas applied to the device's own path,
mels and F0 tracks, within 1e-12 relative: only the order of a float64 sum differs."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import align_ref as ar
from tests import score_ref as sr
from tests import taco_mel_ref as tm

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOP = 275
K_BOUND = 2
# between them the anti-diagonals run one shorter than, equal to and one longer than a wave (64) and the workgroup (256)
SHAPES = [(1, 1), (1, 7), (7, 1), (2, 2), (3, 5), (5, 257), (257, 5), (63, 65), (64, 64), (65, 63), (255, 257), (256, 256), (257, 255), (300, 70)]
CONTENTS = ('integers', 'zeros', 'zero_run', 'random')


def matrix(kind, shape):
    rng = np.random.Generator(np.random.PCG64(1000 * shape[0] + shape[1]))
    if kind == 'integers':
        return rng.integers(0, 8, size=shape).astype(np.float32)
    if kind == 'zeros':
        return np.zeros(shape, np.float32)
    if kind == 'zero_run':                  # zeros along j - i = 2 where the matrix has that diagonal, small integers elsewhere
        c = rng.integers(1, 4, size=shape).astype(np.float32)
        i = np.arange(shape[0])
        ok = i + 2 < shape[1]
        c[i[ok], i[ok] + 2] = 0.0
        return c
    if kind == 'random':
        return rng.random(shape, dtype=np.float32) * np.float32(30.0)
    raise KeyError(kind)


_refs = {}


def ref_path(kind, shape):
    """(path, total) of the restatement, computed once and shared."""
    if (kind, shape) not in _refs:
        path, total, _ = ar.path_of(matrix(kind, shape))
        _refs[kind, shape] = (path, total)
    return _refs[kind, shape]


def device_paths(mats, Ta_max=None, Tb_max=None):
    """One ``dtw_path`` call over matrices of any shapes, padded with NaN to a common shape: (paths, totals, the raw path buffer)."""
    from tacotronv2_wavernn_chinese_amd.frontend import dtw_path
    Ta_max, Tb_max = Ta_max or max(m.shape[0] for m in mats), Tb_max or max(m.shape[1] for m in mats)
    buf = np.full((len(mats), Ta_max, Tb_max), np.nan, np.float32)      # whatever lies outside a pair's own matrix must not matter
    for b, m in enumerate(mats):
        buf[b, :m.shape[0], :m.shape[1]] = m
    paths, totals = dtw_path(torch.from_numpy(buf).cuda(), [m.shape[0] for m in mats], [m.shape[1] for m in mats])
    return [p.cpu().numpy() for p in paths], totals.cpu().numpy(), dtw_path.last_path_buffer.cpu().numpy()


def check_path_shape(path, Ta, Tb):
    assert max(Ta, Tb) <= len(path) <= Ta + Tb - 1
    assert tuple(path[0]) == (0, 0) and tuple(path[-1]) == (Ta - 1, Tb - 1)
    step = np.diff(path, axis=0)
    assert ((step >= 0) & (step <= 1)).all() and (step.sum(axis=1) >= 1).all()


# ---- 1. wrnn_align_path on chosen matrices -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: f'{s[0]}x{s[1]}')
def test_path_of_chosen_matrices_equals_the_restatement(shape):
    mats = [matrix(kind, shape) for kind in CONTENTS]
    paths, totals, raw = device_paths(mats)
    assert raw.shape == (len(mats), shape[0] + shape[1] - 1, 2) and raw.dtype == np.int32
    for b, kind in enumerate(CONTENTS):
        want, total = ref_path(kind, shape)
        assert paths[b].dtype == np.int32 and paths[b].tolist() == want.tolist(), (kind, shape)
        assert totals[b] == total, (kind, shape, totals[b], total)
        assert (raw[b, len(want):] == -1).all()
        check_path_shape(paths[b], *shape)


@pytest.mark.parametrize('shape', [(3, 5), (65, 63), (257, 255), (300, 70)], ids=lambda s: f'{s[0]}x{s[1]}')
def test_nan_and_infinity_terminate_inside_the_matrix(shape):
    c = matrix('random', shape)
    c[shape[0] // 2, shape[1] // 2], c[shape[0] // 3, shape[1] // 2] = np.nan, np.inf
    c[-1, -1] = np.nan
    paths, _, raw = device_paths([c, np.full(shape, np.nan, np.float32)])
    for p in paths:
        check_path_shape(p, *shape)
    assert (raw[0, len(paths[0]):] == -1).all()


def test_ragged_batch_equals_each_alone_and_a_second_call():
    picks = [('random', (255, 257)), ('integers', (300, 70)), ('zero_run', (5, 257)), ('zeros', (1, 7)), ('random', (64, 64)), ('integers', (257, 5))]
    mats = [matrix(k, s) for k, s in picks]
    paths, totals, raw = device_paths(mats)
    again = device_paths(mats)
    assert raw.tobytes() == again[2].tobytes() and totals.tobytes() == again[1].tobytes()
    assert raw.shape == (6, 300 + 257 - 1, 2)
    for b, (kind, shape) in enumerate(picks):
        alone_paths, alone_totals, _ = device_paths([mats[b]])
        want, total = ref_path(kind, shape)
        assert paths[b].tolist() == alone_paths[0].tolist() == want.tolist(), (kind, shape)
        assert totals[b].tobytes() == alone_totals[0].tobytes() and totals[b] == total
        assert (raw[b, len(want):] == -1).all()
    # a pair without frames on one side: no path, total 0
    from tacotronv2_wavernn_chinese_amd.frontend import dtw_path
    p, t = dtw_path(torch.ones((2, 4, 6), device='cuda'), [4, 0], [6, 6])
    assert len(p[0]) == 6 and len(p[1]) == 0 and t.cpu().tolist() == [6.0, 0.0]
    assert (dtw_path.last_path_buffer[1].cpu().numpy() == -1).all()


# ---- 2. the cost matrices ------------------------------------------------------------------------------------------------------------------

def _n_of(T):
    return HOP * (T - 1)


def cost_pair(name):
    """The fixtures of the cost test: the parity pairs of the score tests cut to unequal lengths, and the delayed fixtures."""
    if name.startswith('delayed'):
        _, T, m = name.split('_')
        return ar.delayed_pair(int(T), int(m))
    pair, Ta, Tb = name.split('_')
    a, b = sr.parity_pair(pair, _n_of(max(int(Ta), int(Tb))))
    return a[:_n_of(int(Ta))], b[:_n_of(int(Tb))]


COST_CASES = ('noise_41_44', 'mulaw_71_78', 'scaled_44_41', 'scaled_78_71', 'delayed_40_3', 'delayed_40_7', 'delayed_70_3', 'delayed_70_7')
_aligners = {}


def aligner(features='vocoder', pitch=False):
    from tacotronv2_wavernn_chinese_amd.frontend import AlignedScore
    if (features, pitch) not in _aligners:
        _aligners[features, pitch] = AlignedScore(features=features, pitch=pitch)
    return _aligners[features, pitch]


@pytest.mark.parametrize('features', ['vocoder', 'tacotron'])
@pytest.mark.parametrize('name', COST_CASES)
def test_cost_matrix_parity(name, features):
    a, b = cost_pair(name)
    f = None if features == 'vocoder' else tm.TACOTRON
    c64 = ar.cost(a, b, features=f)
    g = float(np.abs(ar.cost(a, b, features=f, dtype=np.float32).astype(np.float64) - c64).max())
    got = aligner(features).cost(a, b)[0].cpu().numpy()
    assert got.dtype == np.float32 and got.shape == c64.shape == (1 + a.size // HOP, 1 + b.size // HOP)
    err = float(np.abs(got.astype(np.float64) - c64).max())
    print(f'cost parity {name}/{features}: {got.shape[0]} x {got.shape[1]}, max cost {c64.max():.2f} dB, g = {g:.3e}, kernel error = {err:.3e} = '
          f'{err / g:.3f} g, bound {K_BOUND} g = {K_BOUND * g:.3e}')
    assert 0 < K_BOUND * g <= 1e-4 * c64.max(), (g, c64.max())     # an ill-conditioned input cannot hide a failure
    assert err <= K_BOUND * g


def test_cost_cells_outside_a_pair_are_zero_and_rows_equal_the_call_alone():
    al = aligner()
    pairs = [cost_pair(n) for n in ('noise_41_44', 'scaled_78_71', 'delayed_40_3')]
    batch = al.cost([p[0] for p in pairs], [p[1] for p in pairs])
    for (a, b), c in zip(pairs, batch):
        alone = al.cost(a, b)[0]
        assert c.shape == alone.shape and torch.equal(c, alone)
    full = batch[0]._base if batch[0]._base is not None else batch[0]
    assert full.shape == (3, 78, 71)
    for b, c in enumerate(batch):
        mask = torch.ones((78, 71), dtype=torch.bool, device=full.device)
        mask[:c.shape[0], :c.shape[1]] = False
        assert not full[b][mask].any()
    a = pairs[1][0]
    same = al.cost(a, a.copy())[0]
    assert not torch.diagonal(same).any() and (same >= 0).all()


# ---- 3. the whole score -------------------------------------------------------------------------------------------------------------------

def device_mels(features, clips):
    from tacotronv2_wavernn_chinese_amd.frontend import MelFrontEnd
    fe = MelFrontEnd(features=features)
    return [fe.melspectrogram(c)[0].cpu().numpy() for c in clips]


def check_against_own_path(got, b, Ma, Mb, with_pitch):
    """The summaries of pair b against the float64 formulas on the device's own path, mels and tracks."""
    path = got['path'][b].numpy()
    f0 = (got['f0_target'][b].numpy(), got['f0_test'][b].numpy()) if with_pitch else (None, None)
    want = ar.summaries(path, float(got['total_cost'][b]), Ma, Mb, f0_target=f0[0], f0_test=f0[1])
    for k in ar.FIELDS:
        v = float(got[k][b])
        if k in ('path_len', 'frames_target', 'frames_test', 'voiced_both'):
            assert v == want[k], (k, v, want[k])
        else:
            assert abs(v - want[k]) <= 1e-12 * abs(want[k]), (k, v, want[k])
    np.testing.assert_allclose(got['lsd'][b].numpy(), ar.lsd_along(Ma, Mb, path), rtol=1e-12, atol=0)
    if with_pitch:
        np.testing.assert_allclose(got['cents'][b].numpy(), ar.pitch_along(f0[0], f0[1], path)['cents'], rtol=1e-12, atol=0)
    else:
        assert not got['cents'][b].any()


@pytest.mark.parametrize('name', ar.QUALIFIED)
def test_score_of_the_qualified_fixtures(name):
    s = ar.qualified_case(name)
    a, b = s['a'], s['b']
    Ta, Tb = s['cost'].shape
    got = aligner(pitch=True).score(a, b, per_path=True)
    assert got['path'][0].numpy().tolist() == s['path'].tolist()
    assert (int(got['path_len'][0]), int(got['frames_target'][0]), int(got['frames_test'][0])) == (len(s['path']), Ta, Tb)
    err = abs(float(got['total_cost'][0]) - s['total_cost'])
    print(f'{name}: total_cost {float(got["total_cost"][0]):.6f} dB, error {err:.3e}, bound (Ta + Tb) K g = {(Ta + Tb) * K_BOUND * s["g"]:.3e}')
    assert err <= (Ta + Tb) * K_BOUND * s['g']
    Ma, Mb = device_mels('vocoder', [a, b])
    check_against_own_path(got, 0, Ma, Mb, True)
    plain = aligner().score(a, b, per_path=True)           # without tracks: the same path, the six pitch fields 0
    assert plain['path'][0].tolist() == got['path'][0].tolist() and float(plain['total_cost'][0]) == float(got['total_cost'][0])
    assert all(float(plain[k][0]) == 0.0 for k in ar.FIELDS[6:])
    check_against_own_path(plain, 0, Ma, Mb, False)


@pytest.mark.parametrize('T,m', ar.DELAYED)
def test_score_of_the_delayed_fixtures(T, m):
    from tacotronv2_wavernn_chinese_amd.frontend import SpectralScore
    s = ar.delayed_case(T, m)
    a, b = s['a'], s['b']
    got = aligner(pitch=True).score(a, b, per_path=True)
    path = got['path'][0].numpy()
    check_path_shape(path, T + 1, T + 1 + m)
    share, unaligned = ar.on_offset(path, m), SpectralScore(resolutions=((256, 64, 256),)).score(a, b)[0]['mcd_db']
    print(f'delayed T = {T}, m = {m}: share on j - i = m {share:.4f} (reference {ar.DELAYED_SHARE[T, m]:.4f}), mcd_dtw_db {float(got["mcd_dtw_db"][0]):.4f} '
          f'(reference {s["mcd_dtw_db"]:.4f}), unaligned mcd_db {unaligned:.4f}, path equals the reference: {path.tolist() == s["path"].tolist()}')
    assert share >= ar.DELAYED_SHARE[T, m]
    assert float(got['mcd_dtw_db'][0]) < unaligned / 3.0
    Ma, Mb = device_mels('vocoder', [a, b])
    check_against_own_path(got, 0, Ma, Mb, True)


def test_identical_clips_and_two_silences_give_the_diagonal_and_exact_zeros():
    a = sr.parity_pair('scaled', 6000)[0]
    z = np.zeros(4321, np.float32)
    for features in ('vocoder', 'tacotron'):
        for x in (a, z):
            got = (aligner(features, pitch=True) if features == 'vocoder' else aligner(features)).score(x, x.copy(), per_path=True)
            T = 1 + x.size // HOP
            assert got['path'][0].tolist() == [[t, t] for t in range(T)] and int(got['path_len'][0]) == T
            for k in ('total_cost', 'mcd_dtw_db', 'mel_lsd_dtw_db', 'f0_rmse_cents', 'gpe', 'vde', 'ffe'):
                assert float(got[k][0]) == 0.0, (features, k)
            assert not got['lsd'][0].any() and not got['cents'][0].any()
    voiced = aligner(pitch=True).score(a, a.copy())
    assert float(voiced['voiced_both'][0]) > 0 and float(voiced['f0_corr'][0]) == pytest.approx(1.0, abs=1e-12)


@pytest.mark.parametrize('name', sr.PAIR_NAMES)
def test_aligned_mcd_is_at_most_the_unaligned_one(name):
    from tacotronv2_wavernn_chinese_amd.frontend import SpectralScore
    a, b = sr.parity_pair(name, 6000)
    g = float(np.abs(ar.cost(a, b, dtype=np.float32).astype(np.float64) - ar.cost(a, b)).max())
    got = aligner().score(a, b)
    mcd = SpectralScore(resolutions=((256, 64, 256),)).score(a, b)[0]['mcd_db']
    print(f'{name}: mcd_dtw_db {float(got["mcd_dtw_db"][0]):.6f}, mcd_db {mcd:.6f}, K g = {K_BOUND * g:.3e}')
    assert float(got['mcd_dtw_db'][0]) <= mcd + K_BOUND * g


def test_ragged_batch_equals_the_calls_pair_by_pair():
    al = aligner(pitch=True)
    q = [ar.qualified_pair(n) for n in ('delay_s14_T12_m3', 'cut_s14_T7_m2')] + [ar.delayed_pair(40, 3), sr.parity_pair('mulaw', 6000)]
    targets = [p[0] for p in q] + [q[0][0], np.zeros(0, np.float32)]
    tests = [p[1] for p in q] + [np.zeros(0, np.float32), q[0][1]]              # the last two pairs have an empty clip
    batch = al.score(targets, tests, per_path=True)
    again = al.score(targets, tests, per_path=True)
    for k in ar.FIELDS:
        assert batch[k].numpy().tobytes() == again[k].numpy().tobytes(), k
    for b in range(len(targets)):
        alone = al.score(targets[b], tests[b], per_path=True)
        for k in ar.FIELDS:
            assert batch[k][b].numpy().tobytes() == alone[k][0].numpy().tobytes(), (b, k)
        for k in ('path', 'lsd', 'cents'):
            assert torch.equal(batch[k][b], alone[k][0]), (b, k)
    for b in (4, 5):
        assert all(float(batch[k][b]) == 0.0 for k in ar.FIELDS) and batch['path'][b].shape == (0, 2)
    assert (al.last_path_buffer[4:] == -1).all()
    assert all(int(batch['path_len'][b]) >= max(int(batch['frames_target'][b]), int(batch['frames_test'][b])) > 0 for b in range(4))


# ---- 4. the command line -------------------------------------------------------------------------------------------------------------------

def test_cli_align_prints_the_numbers_of_the_class(tmp_path):
    from tacotronv2_wavernn_chinese_amd.dsp import save_wav
    from tacotronv2_wavernn_chinese_amd.frontend import AlignedScore, read_wav
    a, b = ar.delayed_pair(40, 3)
    save_wav(a, tmp_path / 'a.wav', 22050)
    save_wav(b, tmp_path / 'b.wav', 22050)
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'wavernn_score.py'), '--target', str(tmp_path / 'a.wav'), '--test', str(tmp_path / 'b.wav'),
                        '--align', '--pitch', '--json', '--per_frame', str(tmp_path / 'p.npz')], cwd=tmp_path, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    want = AlignedScore(pitch=True).score(read_wav(tmp_path / 'a.wav')[0], read_wav(tmp_path / 'b.wav')[0], per_path=True)
    assert len(out['pairs']) == 1 and out['pairs'][0]['name'] == 'b'
    assert (out['pairs'][0]['n_target'], out['pairs'][0]['n_test']) == (a.size, b.size)
    for k in ar.FIELDS:
        assert out['pairs'][0][k] == float(want[k][0]) == out['mean'][k], k
    assert out['pairs'][0]['path_len'] >= 44 and out['pairs'][0]['mcd_dtw_db'] > 0
    with np.load(tmp_path / 'p.npz') as z:
        np.testing.assert_array_equal(z['b/path'], want['path'][0].numpy())
        np.testing.assert_array_equal(z['b/lsd'], want['lsd'][0].numpy())
        np.testing.assert_array_equal(z['b/f0_test'], want['f0_test'][0].numpy())
