"""The host replay of the device-drawn MOL / dual-softmax noise (tests/philox_ref.py) against csrc/device_util.h itself.

device_util.h is `__host__ __device__`: hipcc's host pass compiles wrnn_uniform / wrnn_uniform_mol into a small shared library (no
device code, no HIP runtime), and the replay that the GPU parity tests (tests/test_gpu_philox_mol.py) hand to the oracle must
reproduce it bit for bit.  No GPU needed.
"""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import philox_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'tacotronv2_wavernn_chinese_amd', 'csrc')

SHIM = r'''
#include "device_util.h"
extern "C" void shim_uniform(const uint64_t *seed, const uint64_t *t, const uint32_t *row, const uint32_t *k, int n, float *u, float *um) {
    for (int i = 0; i < n; ++i) {
        u[i] = wrnn_uniform(seed[i], t[i], row[i], k[i]);
        um[i] = wrnn_uniform_mol(seed[i], t[i], row[i], k[i]);
    }
}
extern "C" void shim_mol_map(uint32_t m0, uint32_t n, float *w, float *u) {   // the draw for the 23-bit values m0 .. m0 + n - 1
    for (uint32_t i = 0; i < n; ++i) {
        w[i] = u01_from_bits((m0 + i) << 9);
        u[i] = wrnn_mol_from_u01(w[i]);
    }
}
'''


@pytest.fixture(scope='module')
def shim(tmp_path_factory):
    """device_util.h compiled for the HOST by the compiler the library is built with (csrc/Makefile: HIPCC)."""
    hipcc = os.environ.get('HIPCC') or shutil.which('hipcc') or '/opt/rocm/bin/hipcc'
    d = tmp_path_factory.mktemp('philox_shim')
    src, so = d / 'shim.hip', d / 'libphilox_shim.so'
    src.write_text(SHIM)
    subprocess.check_call([hipcc, '-x', 'hip', '--cuda-host-only', '-O2', '-std=c++17', '-fPIC', '-shared', '-no-hip-rt', '-I', CSRC,
                           str(src), '-o', str(so)])
    return C.CDLL(str(so))


def _vp(a):
    return a.ctypes.data_as(C.c_void_p)


def test_mol_mapping_exhaustive_range_monotone_and_replay_bit_equal(shim):
    """All 2^23 values u01_from_bits can return, through wrnn_mol_from_u01: strictly inside (0, 1), inside the reference's
    uniform_(1e-5, 1 - 1e-5), strictly increasing (no two inputs collapse), and the numpy and torch replays of the mapping equal the
    compiled helper bit for bit.  The unfused form `1e-5f + w * c` is a different function (27 % of the inputs): the replay must not be it."""
    import torch
    n = 1 << 23
    w, u = np.empty(n, np.float32), np.empty(n, np.float32)
    shim.shim_mol_map(C.c_uint32(0), C.c_uint32(n), _vp(w), _vp(u))
    bits = np.arange(n, dtype=np.uint32) << np.uint32(9)
    np.testing.assert_array_equal(philox_ref._u01(bits), w)
    assert w[0] > 0.0 and w[-1] < 1.0
    assert u.min() > 0.0 and u.max() < 1.0
    assert u.min() >= np.float32(1e-5) and u.max() <= np.float32(1.0) - np.float32(1e-5)
    assert float(u.min()) >= 1e-5 and float(u.max()) <= 1.0 - 1e-5          # also against the double-precision bounds
    assert (np.diff(u) > 0).all()
    # both logs of the logistic draw stay finite at the ends
    assert np.isfinite(np.log(u[[0, -1]])).all() and np.isfinite(np.log(np.float32(1.0) - u[[0, -1]])).all()
    np.testing.assert_array_equal(philox_ref.mol_from_bits(bits).view(np.uint32), u.view(np.uint32))
    np.testing.assert_array_equal(philox_ref.mol_from_bits(bits | np.uint32(0x1FF)).view(np.uint32), u.view(np.uint32))   # the low 9 bits are unused
    ut = philox_ref.mol_from_bits_torch(torch.from_numpy(bits.astype(np.int64))).numpy()
    np.testing.assert_array_equal(ut.view(np.uint32), u.view(np.uint32))
    unfused = np.float32(1e-5) + w * (np.float32(1.0) - np.float32(2e-5))
    assert 0.25 < float((unfused != u).mean()) < 0.30


def test_wrnn_uniform_on_the_host_equals_the_numpy_replay(shim):
    """wrnn_uniform / wrnn_uniform_mol compiled for the host against philox_uniform_at / philox_mol_uniforms on 5 400 (seed, t, row, k):
    steps beyond 2^32 (the high counter word), seeds with high bits set (the second key word), every word of the first three blocks
    (k = 0 .. 10: the MOL draws) and the last block of the dual-softmax classes (k = 252 .. 255)."""
    seeds = [0, 1, 0xC0FFEE, 0x8000000000000001, 0xFFFFFFFF00000000 | 0x5EED]
    ts = [0, 1, 2, 95, 96, 11274, 110274, 2 ** 32 - 1, 2 ** 32, 2 ** 32 + 7, 2 ** 40 + 12345, 2 ** 63 + 5]
    rows = [0, 1, 3, 4, 39, 2 ** 31 + 63]
    ks = list(range(11)) + [252, 253, 254, 255]
    S, T, R, K = np.meshgrid(np.array(seeds, np.uint64), np.array(ts, np.uint64), np.array(rows, np.uint32), np.array(ks, np.uint32), indexing='ij')
    n = S.size
    assert n == 5400
    u, um = np.empty(n, np.float32), np.empty(n, np.float32)
    shim.shim_uniform(_vp(np.ascontiguousarray(S.reshape(-1))), _vp(np.ascontiguousarray(T.reshape(-1))), _vp(np.ascontiguousarray(R.reshape(-1))),
                      _vp(np.ascontiguousarray(K.reshape(-1))), n, _vp(u), _vp(um))
    u, um = u.reshape(S.shape), um.reshape(S.shape)
    for i, seed in enumerate(seeds):
        ref = philox_ref.philox_uniform_at(seed, ts, rows, 256)
        np.testing.assert_array_equal(ref[:, :, ks].view(np.uint32), u[i].view(np.uint32), err_msg=f'seed {seed:#x}')
        for j, t in enumerate(ts):
            if t + 1 < 2 ** 63:          # philox_mol_uniforms takes a window [t0, t0 + n)
                u_mix, u_log = philox_ref.philox_mol_uniforms(seed, t, 1, rows)
                np.testing.assert_array_equal(u_mix[0].view(np.uint32), um[i, j, :, :10].view(np.uint32))
                np.testing.assert_array_equal(u_log[0].view(np.uint32), um[i, j, :, 10].view(np.uint32))
    # the draws differ where they should: other seed word, other step word, other row, other class
    assert len(np.unique(u.view(np.uint32))) > 0.999 * n
    # philox_uniform (steps and rows from 0) is the same function
    np.testing.assert_array_equal(philox_ref.philox_uniform(seeds[2], 3, 2, 256), philox_ref.philox_uniform_at(seeds[2], [0, 1, 2], [0, 1], 256))


def test_mol_replays_agree_off_origin_and_on_unordered_rows():
    """numpy and torch replays of the MOL draws: a window that does not start at step 0, rows in no order, a seed with both key words."""
    seed = 0x1234ABCD5678
    a_mix, a_log = philox_ref.philox_mol_uniforms(seed, 0, 70, [0, 1, 2, 3, 4, 5, 6])
    b_mix, b_log = philox_ref.philox_mol_uniforms_torch(seed, 33, 37, [5, 0, 6, 2])
    np.testing.assert_array_equal(b_mix.numpy(), a_mix[33:, [5, 0, 6, 2]])
    np.testing.assert_array_equal(b_log.numpy(), a_log[33:, [5, 0, 6, 2]])
    c_mix, c_log = philox_ref.philox_mol_uniforms(seed, 33, 37, [5, 0, 6, 2])
    np.testing.assert_array_equal(c_mix, a_mix[33:, [5, 0, 6, 2]])
    np.testing.assert_array_equal(c_log, a_log[33:, [5, 0, 6, 2]])
    assert a_mix.shape == (70, 7, 10) and a_log.shape == (70, 7) and a_mix.dtype == a_log.dtype == np.float32
    big = 2 ** 32 - 5                        # the window crosses the carry into the high counter word
    d_mix, d_log = philox_ref.philox_mol_uniforms(seed, big, 10, [3, 1])
    e_mix, e_log = philox_ref.philox_mol_uniforms_torch(seed, big, 10, [3, 1])
    np.testing.assert_array_equal(d_mix, e_mix.numpy())
    np.testing.assert_array_equal(d_log, e_log.numpy())
    # the logistic draw is word 2 of block 2, not the tenth mixture draw
    assert not np.array_equal(a_log, a_mix[:, :, 9])


def test_rows_and_steps_of_one_call_share_no_philox_block():
    """Independence, on the replayed bits: in a 32-row, 1 000-step window the counters (t, row, k >> 2) are pairwise distinct, so no two
    (row, step) pairs see the same 11 draws (Philox is a bijection of the counter: a shared block is the only way to share a tuple) -- and
    no pair shares a single block either."""
    w = philox_ref._philox_words_at(0x5EED0032, np.arange(1000, dtype=np.uint64), np.arange(32), 3)     # (1000, 32, 12)
    tuples = np.ascontiguousarray(w[:, :, :11]).reshape(-1, 11)
    assert len(np.unique(tuples, axis=0)) == 32 * 1000
    blocks = w.reshape(-1, 4)
    assert len(np.unique(blocks, axis=0)) == 32 * 1000 * 3
    u_mix, u_log = philox_ref.philox_mol_uniforms(0x5EED0032, 0, 1000, range(32))
    # crude uniformity of what the oracle is handed (351 000 draws: mean 0.5 +- 0.0005, sd 1 / sqrt(12))
    allu = np.concatenate([u_mix.reshape(-1), u_log.reshape(-1)]).astype(np.float64)
    assert abs(allu.mean() - 0.5) < 0.003 and abs(allu.std() - 12 ** -0.5) < 0.003


def test_dual_softmax_replay_is_the_exponential_of_wrnn_uniform():
    """philox_dm_exponentials: q = -log u of wrnn_uniform(seed, t, which, k), which = 0 coarse / 1 fine, k < 256, laid out (n, 2, 256)."""
    seed = 0xABCDEF0123456789
    q = philox_ref.philox_dm_exponentials(seed, 5, 40)
    assert q.shape == (40, 2, 256) and q.dtype == np.float32 and (q > 0).all() and np.isfinite(q).all()
    u = philox_ref.philox_uniform_at(seed, np.arange(5, 45, dtype=np.uint64), [0, 1], 256)
    np.testing.assert_array_equal(q, (-np.log(u.astype(np.float64))).astype(np.float32))
    assert not np.array_equal(q[:, 0], q[:, 1])
    assert abs(float(q.mean()) - 1.0) < 0.03                   # Exp(1): 20 480 draws, sd of the mean 0.007
