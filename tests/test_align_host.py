"""Host-side checks of the time alignment: the restatement ``tests/align_ref.py`` against brute force, its properties, the conditions
the GPU tests' fixtures must keep, and the host-only entries of ``csrc/align.hip`` (create, frames, workspace limits, struct layout)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from tests import align_ref as ar
from tests import score_ref as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the restatement's DP against every monotone path --------------------------------------------------------------------------------

def _all_paths(Ta, Tb):
    """Every path from (0, 0) to (Ta - 1, Tb - 1) in steps (1, 1), (1, 0), (0, 1), each as a list of cells."""
    out = []

    def walk(i, j, cells):
        cells = cells + [(i, j)]
        if (i, j) == (Ta - 1, Tb - 1):
            out.append(cells)
            return
        if i + 1 < Ta and j + 1 < Tb:
            walk(i + 1, j + 1, cells)
        if i + 1 < Ta:
            walk(i + 1, j, cells)
        if j + 1 < Tb:
            walk(i, j + 1, cells)

    walk(0, 0, [])
    return out


def _backward_key(cells):
    """The steps of a path read from its end: 0 for a diagonal step, 1 from (i - 1, j), 2 from (i, j - 1).  Among minimal paths the tie
    order picks the smallest such sequence: at every cell, from the end, the first predecessor in that order that still lies on a
    minimal path."""
    key = []
    for (i0, j0), (i1, j1) in zip(cells[-2::-1], cells[::-1]):
        key.append(0 if (i1 - i0, j1 - j0) == (1, 1) else 1 if i1 - i0 == 1 else 2)
    return key


def _brute(cost):
    paths = _all_paths(*cost.shape)
    totals = [sum(float(cost[c]) for c in p) for p in paths]   # integer-valued costs: every sum is exact
    best = min(totals)
    minimal = [p for p, t in zip(paths, totals) if t == best]
    return best, min(minimal, key=_backward_key)


SHAPES = [(a, b) for a in range(1, 6) for b in range(1, 6)]


@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: f'{s[0]}x{s[1]}')
def test_dp_against_brute_force(shape):
    rng = np.random.Generator(np.random.PCG64(100 * shape[0] + shape[1]))
    mats = [rng.integers(0, 10, size=shape).astype(np.float32) for _ in range(6)]
    mats += [rng.integers(0, 2, size=shape).astype(np.float32) for _ in range(6)]           # deliberate ties
    mats += [np.zeros(shape, np.float32), np.ones(shape, np.float32), np.fromfunction(lambda i, j: (i == j) * 1.0, shape).astype(np.float32)]
    for c in mats:
        total, cells = _brute(c)
        path, got_total, D = ar.path_of(c)
        assert got_total == total, (c, got_total, total)
        assert [tuple(p) for p in path.tolist()] == cells, (c, path.tolist(), cells)
        assert D[-1, -1] == total


def _check_path_shape(path, Ta, Tb):
    P = len(path)
    assert max(Ta, Tb) <= P <= Ta + Tb - 1
    assert tuple(path[0]) == (0, 0) and tuple(path[-1]) == (Ta - 1, Tb - 1)
    step = np.diff(path, axis=0)
    assert ((step >= 0) & (step <= 1)).all() and (step.sum(axis=1) >= 1).all()


def test_path_properties_on_random_matrices():
    rng = np.random.Generator(np.random.PCG64(7))
    for Ta, Tb in [(1, 1), (1, 9), (9, 1), (7, 7), (13, 40), (40, 13), (64, 65)]:
        c = rng.random((Ta, Tb), dtype=np.float32)
        path, total, D = ar.path_of(c)
        _check_path_shape(path, Ta, Tb)
        assert total == D[-1, -1] and np.isclose(total, c.astype(np.float64)[path[:, 0], path[:, 1]].sum(), rtol=1e-13)
    # all zeros: the tie order's path is the diagonal, then (i - 1, j) or (i, j - 1) along the edge
    path, total, _ = ar.path_of(np.zeros((3, 5), np.float32))
    assert total == 0.0 and path.tolist() == [[0, 0], [0, 1], [0, 2], [1, 3], [2, 4]]
    path, _, _ = ar.path_of(np.zeros((5, 3), np.float32))
    assert path.tolist() == [[0, 0], [1, 0], [2, 0], [3, 1], [4, 2]]


def test_nan_and_infinity_terminate_inside_the_matrix():
    c = np.random.Generator(np.random.PCG64(3)).random((9, 12), dtype=np.float32)
    c[4, 5], c[2, 7] = np.nan, np.inf
    path, _, _ = ar.path_of(c)
    _check_path_shape(path, 9, 12)
    # the backtrack over arbitrary bytes: bounded, inside, monotone
    junk = np.random.Generator(np.random.PCG64(4)).integers(0, 256, size=(9, 12)).astype(np.uint8)
    _check_path_shape(ar.backtrack(junk), 9, 12)


def test_identical_clips_give_the_diagonal_and_zeros():
    a = sr.parity_pair('scaled', 6000)[0]
    s = ar.score(a, a.copy())
    T = 1 + 6000 // 275
    assert s['path'].tolist() == [[t, t] for t in range(T)]
    assert (np.diag(s['cost']) == 0).all() and (s['cost'] >= 0).all()
    for k in ('total_cost', 'mcd_dtw_db', 'mel_lsd_dtw_db'):
        assert s[k] == 0.0, k
    f0 = np.where(np.arange(T) % 3 == 0, 0.0, 150.0 + np.arange(T)).astype(np.float32)
    p = ar.pitch_along(f0, f0.copy(), s['path'])
    assert p['f0_rmse_cents'] == p['gpe'] == p['vde'] == p['ffe'] == 0.0 and p['voiced_both'] == float((f0 > 0).sum())


@pytest.mark.parametrize('name', sr.PAIR_NAMES)
def test_aligned_mcd_is_at_most_the_unaligned_one(name):
    """Clips of equal length: the diagonal is a candidate path of total T mcd_db, and P >= T."""
    a, b = sr.parity_pair(name, 6000)
    s = ar.score(a, b)
    mcd = float(sr.mel_frames(a, b)['mcd'].mean())
    assert np.isclose(np.diag(s['cost']).mean(), mcd, rtol=1e-12)
    assert s['mcd_dtw_db'] <= mcd * (1 + 1e-12)


def test_pitch_fields_along_a_path_against_the_pitch_restatement():
    """On the diagonal of equally long tracks the fields are ``pitch_ref.pair_scores``'s."""
    from tests import pitch_ref as pr
    rng = np.random.Generator(np.random.PCG64(11))
    T = 50
    ft = np.where(rng.random(T) < 0.2, 0.0, 120.0 + 40.0 * rng.random(T)).astype(np.float32)
    fs = np.where(rng.random(T) < 0.2, 0.0, ft * (1.0 + 0.3 * (rng.random(T) - 0.5)) + (ft == 0) * 130.0).astype(np.float32)
    path = np.stack([np.arange(T), np.arange(T)], axis=1).astype(np.int32)
    got, want = ar.pitch_along(ft, fs, path), pr.pair_scores(ft, fs)
    for k in ('f0_rmse_cents', 'gpe', 'vde', 'ffe', 'f0_corr'):
        assert np.isclose(got[k], want[k], rtol=1e-12, atol=0), (k, got[k], want[k])
    assert got['voiced_both'] == want['voiced_both']


# ---- the fixtures of the GPU tests -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('name', ar.QUALIFIED)
def test_qualified_fixtures_keep_their_condition(name):
    """On every decision along the float64 path the best predecessor leads the second best by at least 1000 (Ta + Tb) g, g the float32
    chain's worst cost error on the fixture: an error of the size the device may make in D, (Ta + Tb) K g with K <= 4, cannot turn a
    decision, so the device path must equal this one and tests/test_gpu_align.py demands equality."""
    s = ar.qualified_case(name)
    Ta, Tb = s['cost'].shape
    gaps = ar.decision_gaps(s['D'], s['path'])
    need = 1000.0 * (Ta + Tb) * s['g']
    print(f'{name}: {Ta} x {Tb}, P = {len(s["path"])}, smallest gap {gaps.min():.4f} dB, g = {s["g"]:.3e}, 1000 (Ta + Tb) g = {need:.4f} dB')
    assert s['g'] > 0 and gaps.min() >= need
    _check_path_shape(s['path'], Ta, Tb)


def test_some_qualified_fixture_leaves_the_diagonal():
    off = [n for n in ar.QUALIFIED if (np.diff(ar.qualified_case(n)['path'], axis=0) != 1).any()]
    assert len(off) >= 3
    assert any(ar.qualified_case(n)['cost'].shape[0] > ar.qualified_case(n)['cost'].shape[1] for n in off)


# (T, m): smallest gap in dB, share of the path on j - i = m, mcd_dtw_db, unaligned mcd_db; what the float64 restatement gives
DELAYED_TABLE = {(40, 3): (2.37, 0.93, 3.64, 15.2), (40, 7): (0.79, 0.85, 8.89, 29.2), (70, 3): (2.37, 0.96, 2.16, 14.2), (70, 7): (0.79, 0.91, 5.47, 27.2)}


@pytest.mark.parametrize('T,m', ar.DELAYED)
def test_delayed_fixtures_give_what_the_gpu_test_relies_on(T, m):
    s = ar.delayed_case(T, m)
    gap, share, mcd_dtw, mcd = DELAYED_TABLE[T, m]
    Ta, Tb = s['cost'].shape
    assert (Ta, Tb) == (T + 1, T + 1 + m)
    unaligned = float(sr.mel_frames(s['a'], s['b'])['mcd'].mean())
    gaps = ar.decision_gaps(s['D'], s['path'])
    print(f'delayed T = {T}, m = {m}: smallest gap {gaps.min():.4f} dB, g = {s["g"]:.3e}, share {ar.on_offset(s["path"], m):.4f}, '
          f'mcd_dtw_db {s["mcd_dtw_db"]:.4f}, unaligned {unaligned:.4f}')
    assert abs(gaps.min() - gap) <= 0.005 and abs(s['mcd_dtw_db'] - mcd_dtw) <= 0.005 and abs(unaligned - mcd) <= 0.05
    assert ar.on_offset(s['path'], m) == ar.DELAYED_SHARE[T, m] and round(ar.DELAYED_SHARE[T, m], 2) == share
    assert s['mcd_dtw_db'] < unaligned / 3.0
    # these do not qualify for path equality: the path absorbs the delay in a corner where the predecessors lie this close
    assert gaps.min() < 1000.0 * (Ta + Tb) * s['g']


# ---- the host-only entries ---------------------------------------------------------------------------------------------------------------

def test_abi_number_and_struct_layout(tmp_path):
    from tacotronv2_wavernn_chinese_amd import _cabi
    hdr = open(os.path.join(ROOT, 'include', 'wavernn_amd.h')).read()
    assert int(re.search(r'#define WRNN_ABI_VERSION (\d+)', hdr).group(1)) == 9 == _cabi.ABI_VERSION == _cabi.load_library().wrnn_abi_version()
    assert int(re.search(r'#define WRNN_ALIGN_FIELDS (\d+)', hdr).group(1)) == _cabi.ALIGN_FIELDS == len(_cabi.ALIGN_FIELD_NAMES) == len(ar.FIELDS)
    assert _cabi.ALIGN_FIELD_NAMES == ar.FIELDS
    for i, name in enumerate(_cabi.ALIGN_FIELD_NAMES):
        assert int(re.search(rf'#define WRNN_ALIGN_{name.upper()} (\d+)', hdr).group(1)) == i, name
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{ROOT}/include/wavernn_amd.h"', 'int main(void) {',
             '  printf("size %zu\\n", sizeof(wrnn_align_config));']
    for fname, _ in _cabi.AlignConfig._fields_:
        lines.append(f'  printf("{fname} %zu\\n", offsetof(wrnn_align_config, {fname}));')
    lines += ['  return 0;', '}']
    src, exe = tmp_path / 'layout.c', tmp_path / 'layout'
    src.write_text('\n'.join(lines))
    subprocess.check_call(['gcc', '-std=c11', '-o', str(exe), str(src)])
    got = {l.split()[0]: int(l.split()[1]) for l in subprocess.check_output([str(exe)], text=True).split('\n') if l.strip()}
    assert got['size'] == C.sizeof(_cabi.AlignConfig)
    for fname, _ in _cabi.AlignConfig._fields_:
        assert got[fname] == getattr(_cabi.AlignConfig, fname).offset, fname


def test_create_refusals():
    from tacotronv2_wavernn_chinese_amd import _cabi
    _cabi.NativeAlign().close()
    _cabi.NativeAlign(n_mels=40, align=_cabi.AlignConfig(mcd_order=39)).close()
    for kw, text in [(dict(align=_cabi.AlignConfig(mcd_order=0)), 'WRNN_ERR_INVALID: mcd_order'),
                     (dict(align=_cabi.AlignConfig(mcd_order=80)), 'WRNN_ERR_INVALID: mcd_order'),
                     (dict(n_mels=40, align=_cabi.AlignConfig(mcd_order=40)), 'WRNN_ERR_INVALID: mcd_order'),
                     (dict(align=_cabi.AlignConfig(gpe_ratio=0.0)), 'WRNN_ERR_INVALID: gpe_ratio'),
                     (dict(align=_cabi.AlignConfig(gpe_ratio=float('nan'))), 'WRNN_ERR_INVALID: gpe_ratio'),
                     (dict(align=_cabi.AlignConfig(gpe_ratio=float('inf'))), 'WRNN_ERR_INVALID: gpe_ratio'),
                     (dict(n_fft=1024), 'WRNN_ERR_UNSUPPORTED: n_fft'),                      # the front end's own refusals, with its status
                     (dict(n_mels=129), 'WRNN_ERR_INVALID'),
                     (dict(min_level_db=0.0), 'WRNN_ERR_INVALID'),
                     (dict(features=_cabi.MelFeatures(magnitude_power=3)), 'WRNN_ERR_INVALID: bad features')]:
        with pytest.raises(ValueError, match=text):
            _cabi.NativeAlign(**kw)
    bad = _cabi.AlignConfig()
    bad.struct_size -= 4
    with pytest.raises(ValueError, match='struct_size'):
        _cabi.NativeAlign(align=bad)
    # a refused handle is still returned, for its error text
    lib = _cabi.load_library()
    cfg, h = _cabi.MelConfig(22050, 2048, 275, 1100, 80, 95.0, -100.0, 0), C.c_void_p()
    assert lib.wrnn_align_create(C.byref(cfg), None, C.byref(_cabi.AlignConfig(mcd_order=99)), C.byref(h)) == _cabi.ERR_INVALID
    assert h and b'mcd_order = 99' in lib.wrnn_align_last_error(h)
    assert lib.wrnn_align_frames(h, 5000) == _cabi.ERR_INVALID and lib.wrnn_align_workspace_bytes(h, 1, 5000, 5000) == _cabi.ERR_STATE
    lib.wrnn_align_destroy(h)


def test_frames_entry():
    from tacotronv2_wavernn_chinese_amd import _cabi
    nat = _cabi.NativeAlign()
    assert nat.min_samples == 1025 and [nat.frames(n) for n in (1025, 1099, 1100, 22050)] == [4, 4, 5, 81]
    for n in (0, 1, 1024, 2 ** 31):
        with pytest.raises(ValueError):
            nat.frames(n)
    zero = _cabi.NativeAlign(hop_length=200, features=_cabi.MelFeatures(pad_mode=_cabi.MEL_PAD_MODES['zero']))
    assert zero.min_samples == 1 and [zero.frames(n) for n in (1, 199, 200)] == [1, 1, 2]
    with pytest.raises(ValueError):
        zero.frames(0)


def test_workspace_limits():
    """min(Ta_max, Tb_max) <= 4096 (three float64 diagonals in LDS) and B Ta_max Tb_max <= 2^28; the size grows with every argument."""
    from tacotronv2_wavernn_chinese_amd import _cabi
    nat = _cabi.NativeAlign()
    hop = 275
    n_of = lambda T: (T - 1) * hop          # the shortest clip of T frames (T >= 5)
    base = nat.workspace_bytes(1, n_of(401), n_of(401))
    # the cost matrix, the choice bytes, two mels, two cepstra, two paths and the per-path values are all in it
    assert base >= 401 * 401 * 5 + 2 * 80 * 401 * 4 + 2 * 13 * 401 * 4 + 801 * (16 + 16)
    assert nat.workspace_bytes(2, n_of(401), n_of(401)) > base and nat.workspace_bytes(1, n_of(401), n_of(500)) > base
    assert nat.workspace_bytes(1, n_of(4096), n_of(4096)) > 0                       # the largest square pair
    assert nat.workspace_bytes(1, n_of(4096), n_of(65536)) > 0                      # the longer side is free: 2^28 cells
    assert nat.workspace_bytes(16, n_of(4096), n_of(4096)) > 0
    for args in [(1, n_of(4097), n_of(4097)), (1, n_of(4096), n_of(65537)), (17, n_of(4096), n_of(4096)), (1, n_of(5000), n_of(60000))]:
        with pytest.raises(_cabi.WrnnError) as e:
            nat.workspace_bytes(*args)
        assert e.value.code == _cabi.ERR_UNSUPPORTED, args
    for args in [(0, n_of(401), n_of(401)), (65536, n_of(5), n_of(5)), (1, 1024, n_of(401)), (1, n_of(401), 2 ** 31)]:
        with pytest.raises(_cabi.WrnnError) as e:
            nat.workspace_bytes(*args)
        assert e.value.code == _cabi.ERR_INVALID, args


def test_frontend_checks_without_a_device():
    from tacotronv2_wavernn_chinese_amd.frontend import AlignedScore
    s = AlignedScore(mcd_order=20, pitch=True, pitch_fmin=70.0, threshold=0.2)
    assert s.frames(22050) == 81 and s.min_samples == 1025 and s.pitch.hop == s.hop_length and s.pitch.settings['fmin'] == 70.0 and s.pitch.settings['threshold'] == 0.2 and s.config['fmin'] == 95
    with pytest.raises(ValueError):
        AlignedScore(mcd_order=80)
    with pytest.raises(TypeError):
        AlignedScore(nonsense=1)
    with pytest.raises(TypeError):
        AlignedScore(threshold=0.1)           # a pitch setting without pitch=True
    with pytest.raises(ValueError):
        s.frames(100)
