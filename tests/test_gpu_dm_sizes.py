"""The dual-softmax model at every size the library dispatches differently, against the oracle, at every step.

Team kernel (loop_dm_team.hip): the four template instantiations CPL = hidden / 64 = 8, 10, 12, 14 (unit count U = CPL,
plane count PS = CPL / 2 -- 5, the odd one, at hidden 640 -- and the chunk_idx<P> LDS layouts), the host packing of R and
of the O1..O4 images, and the per-workgroup class count QW = quantisation / 32 = 2, 4, 6, 8 with the lane mapping of its
noise draws.  Single-workgroup kernel (loop_deepmind.hip): its size limits and sizes that are no multiple of a wave.

Every case runs on injected Exp(1) draws and on the device's own Philox draws replayed on the host.  coarse, fine and
output must equal the oracle's at EVERY step: the fixtures are chosen so that the oracle's race margin never falls below
1e-4 over the run (tests/size_fixtures.py; asserted on the CPU by tests/test_size_fixtures_host.py), so no step can be
excused as a near-tie and none is skipped.  The oracle itself is pinned to the unmodified reference at hidden 896 and
512 with 256 classes and at hidden 640 with 128 classes (tests/test_deepmind.py); at the other sizes it is the same C
code with other loop bounds.
"""
import numpy as np
import pytest
import torch

from tests.parity_util import parity_report
from tests.size_fixtures import (DM_NOISE_MODES, DM_RELOAD_CASE, DM_SINGLE_CASES, DM_STEPS, DM_TEAM_CASES, dm_distinct_bound,
                                 dm_fixture)

pytestmark = pytest.mark.gpu

TEAM_MESSAGE = 'team kernel needs hidden_size in {512,640,768,896} and quantisation in {64,128,192,256}'
_MODELS = {}


def _model(H, Q, sd=None, cached=True):
    from tacotronv2_wavernn_chinese_amd.deepmind import WaveRNN
    if cached and (H, Q) in _MODELS:
        return _MODELS[(H, Q)]
    if sd is None:
        sd = dm_fixture(H, Q, 'injected')['state_dict']
    m = WaveRNN(hidden_size=H, quantisation=Q)
    m.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in sd.items()})
    m.to('cuda:0')
    if cached:
        _MODELS[(H, Q)] = m
    return m


def _generate(m, fx, noise, kernel):
    if noise == 'injected':
        return m.generate(DM_STEPS, noise=np.array(fx['q']), kernel=kernel)
    return m.generate(DM_STEPS, seed=fx['seed'], kernel=kernel)


def _check(tag, got, fx, Q):
    """Figures first (printed and kept in the parity report), then exact equality at every step."""
    out, coarse, fine = got
    assert coarse.shape == fine.shape == out.shape == (DM_STEPS,) and coarse.dtype == fine.dtype == out.dtype == np.int64
    bad_c, bad_f = np.flatnonzero(coarse != fx['coarse']), np.flatnonzero(fine != fx['fine'])
    first = min([int(b[0]) for b in (bad_c, bad_f) if b.size], default=None)
    parity_report(f'{tag}: {DM_STEPS} steps x 2 softmaxes, every step compared, mismatches coarse {bad_c.size} fine {bad_f.size} '
                  f'(first at {first}), distinct values coarse {len(np.unique(coarse))} fine {len(np.unique(fine))}, '
                  f'oracle min margin {fx["min_margin"]:.2e}')
    np.testing.assert_array_equal(coarse, fx['coarse'])
    np.testing.assert_array_equal(fine, fx['fine'])
    np.testing.assert_array_equal(out, fx['output'])
    assert len(np.unique(coarse)) > dm_distinct_bound(Q) and len(np.unique(fine)) > dm_distinct_bound(Q)


@pytest.mark.parametrize('noise', DM_NOISE_MODES)
@pytest.mark.parametrize('H,Q', DM_TEAM_CASES)
def test_team_kernel_matches_oracle_at_every_size(H, Q, noise):
    fx = dm_fixture(H, Q, noise)
    _check(f'dual-softmax team kernel ({H},{Q}) {noise}', _generate(_model(H, Q), fx, noise, 2), fx, Q)


@pytest.mark.parametrize('noise', DM_NOISE_MODES)
@pytest.mark.parametrize('H,Q', DM_SINGLE_CASES)
def test_single_kernel_matches_oracle_at_its_limits(H, Q, noise):
    fx = dm_fixture(H, Q, noise)
    _check(f'dual-softmax single kernel ({H},{Q}) {noise}', _generate(_model(H, Q), fx, noise, 1), fx, Q)


@pytest.mark.parametrize('H,Q', [(130, 37), (512, 100)])
def test_team_kernel_is_refused_where_unsupported(H, Q):
    """set_kernel(2) on a size the team kernel was not built for fails with the library's message; kernel 0 (auto) runs
    the single-workgroup kernel there."""
    from tacotronv2_wavernn_chinese_amd import _cabi
    from tacotronv2_wavernn_chinese_amd.synth import make_dm_state_dict
    m = _model(H, Q, sd=make_dm_state_dict(0, hidden_size=H, quantisation=Q), cached=False)
    with pytest.raises(_cabi.WrnnError) as ei:
        m.generate(8, seed=1, kernel=2)
    assert _cabi.ERR_NAMES[ei.value.code] == 'WRNN_ERR_INVALID' and TEAM_MESSAGE in str(ei.value)
    auto = m.generate(200, seed=7, kernel=0)
    single = m.generate(200, seed=7, kernel=1)
    for a, s in zip(auto, single):
        np.testing.assert_array_equal(a, s)
    assert len(np.unique(auto[1])) > dm_distinct_bound(Q)


@pytest.mark.parametrize('kernel', [2, 1], ids=['team', 'single'])
def test_second_call_and_reloaded_weights(kernel):
    """Two calls on one handle give the same output (the mailbox and the control words are reset between launches), and
    after a parameter is changed in place the next call follows the new weights: the upload runs again."""
    H, Q = DM_RELOAD_CASE
    fx = dm_fixture(H, Q, 'injected')
    m = _model(H, Q, cached=False)
    first = _generate(m, fx, 'injected', kernel)
    second = _generate(m, fx, 'injected', kernel)
    for a, b in zip(first, second):
        np.testing.assert_array_equal(a, b)
    np.testing.assert_array_equal(first[1], fx['coarse'])
    fx2 = dm_fixture(H, Q, 'injected', True)
    with torch.no_grad():
        for k in ('R', 'O2'):
            getattr(m, k).weight.copy_(torch.from_numpy(np.array(fx2['state_dict'][k + '.weight'])))
    assert not np.array_equal(fx2['coarse'], fx['coarse'])
    _check(f'dual-softmax {"team" if kernel == 2 else "single"} kernel ({H},{Q}) after an in-place weight change',
           _generate(m, fx2, 'injected', kernel), fx2, Q)


@pytest.mark.parametrize('kernel', [2, 1], ids=['team', 'single'])
def test_shortest_runs_and_wrong_noise_shape(kernel):
    H, Q = 512, 64
    fx = dm_fixture(H, Q, 'injected')
    m = _model(H, Q)
    for n in (1, 0):
        for got in (m.generate(n, noise=np.array(fx['q'][:n]), kernel=kernel), m.generate(n, seed=fx['seed'], kernel=kernel)):
            assert all(a.shape == (n,) and a.dtype == np.int64 for a in got)
    out, coarse, fine = m.generate(1, noise=np.array(fx['q'][:1]), kernel=kernel)
    assert (int(coarse[0]), int(fine[0]), int(out[0])) == (int(fx['coarse'][0]), int(fx['fine'][0]), int(fx['output'][0]))
    for shape in ((10, 2, 256), (10, 2, Q - 1), (10, 1, Q), (9, 2, Q)):
        with pytest.raises(ValueError):
            m.generate(10, noise=np.ones(shape, np.float32), kernel=kernel)
