"""CPU: the chosen-logit fixtures of tests/mol_arms.py are what they claim to be.

The margins the builder promises, the arm `oracle.torch_ref.discretized_mix_logistic_loss` really takes at every (row, component) in
float32 and in float64 (its three comparisons are recorded while it runs, the function itself is untouched), every arm and the floor hit
where a group says so, finite float64 losses and gradients, and the sampler noise: Gumbel margin and a win for every component.  Where the
reference tree is present the threshold pair goes through the reference's own loss in float32 and must reproduce
tests/golden/mol_arms_threshold.json, which is what the GPU test expects for that pair."""
import json
import os

import numpy as np
import pytest
import torch
from torch.overrides import TorchFunctionMode

from oracle import ref_harness
from oracle import torch_ref as tr
from tests import mol_arms as ma

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'mol_arms_threshold.json')
NAMES = sorted(ma.GROUPS)


class _Compares(TorchFunctionMode):
    """Records (name, scalar, result) of every tensor < / > scalar comparison made while the mode is on."""

    def __init__(self):
        super().__init__()
        self.seen = []

    def __torch_function__(self, func, types, args=(), kwargs=None):
        out = func(*args, **(kwargs or {}))
        name = getattr(func, '__name__', '')
        if name in ('__gt__', 'gt', '__lt__', 'lt') and len(args) == 2 and not torch.is_tensor(args[1]):
            self.seen.append((name.strip('_'), float(args[1]), out.detach().clone()))
        return out


def arms_taken(loss_fn, logits, y, dtype, y_trailing_axis=False):
    """The arm `loss_fn` selects per (row, component), from its own `cdf_delta > 1e-5`, `y > 0.999`, `y < -0.999`: (n, 10) ints, and its loss."""
    yh = torch.from_numpy(logits).to(dtype)[None]
    yt = torch.from_numpy(y).to(dtype)[None]
    with _Compares() as rec:
        loss = loss_fn(yh, yt.unsqueeze(-1) if y_trailing_axis else yt)
    seen = {(n, s): m for n, s, m in rec.seen}
    assert set(seen) == {('gt', 1e-5), ('gt', 0.999), ('lt', -0.999)}, sorted(seen)
    n = logits.shape[0]
    log_arm, hi, lo = (seen[k].reshape(n, ma.NR).numpy() for k in (('gt', 1e-5), ('gt', 0.999), ('lt', -0.999)))
    arm = np.where(log_arm, ma.ARM_LOG, ma.ARM_MID)
    arm = np.where(hi, ma.ARM_EDGE_HI, arm)
    return np.where(lo, ma.ARM_EDGE_LO, arm), float(loss)


@pytest.mark.parametrize('name', NAMES)
def test_margins(name):
    logits, y = ma.rows_of(ma.GROUPS[name])
    assert logits.dtype == np.float32 and y.dtype == np.float32 and logits.shape == (y.size, 30)
    ay = np.abs(y.astype(np.float64))
    assert not ((ay > ma.Y_BAND[0]) & (ay < ma.Y_BAND[1])).any() and ay.max() <= 1.0
    cd = ma.cdf_delta64(logits, y)
    if name not in ma.EDGE_GROUPS:
        assert not ((cd >= ma.CDF_BAND[0]) & (cd <= ma.CDF_BAND[1])).any(), cd[(cd >= ma.CDF_BAND[0]) & (cd <= ma.CDF_BAND[1])]
    if name == 'edge_lo':
        assert (y <= -0.9995).all() and (y == -1.0).any()
    if name == 'edge_hi':
        assert (y >= 0.9995).all() and (y == 1.0).any()


@pytest.mark.parametrize('dtype', [torch.float32, torch.float64], ids=['float32', 'float64'])
@pytest.mark.parametrize('name', NAMES)
def test_the_restatement_takes_the_expected_arm(name, dtype):
    logits, y = ma.rows_of(ma.GROUPS[name])
    got, loss = arms_taken(tr.discretized_mix_logistic_loss, logits, y, dtype)
    np.testing.assert_array_equal(got, ma.expected_arms(logits, y))
    assert np.isfinite(loss)


def test_every_arm_and_the_floor_are_hit():
    """Per group, over all its rows AND over the rows of P[0] alone (what the gradient test loads)."""
    for part in ('all', 'first'):
        arms, floor, ls, cd = {}, {}, {}, {}
        for name, g in ma.GROUPS.items():
            logits, y = ma.rows_of(g if part == 'all' else dict(P=g['P'][:1], y=g['y'][:1]))
            arms[name], floor[name], ls[name], cd[name] = ma.expected_arms(logits, y), ma.at_floor(logits), logits[:, 20:], ma.cdf_delta64(logits, y)
        assert (arms['edge_lo'] == ma.ARM_EDGE_LO).all() and (arms['edge_hi'] == ma.ARM_EDGE_HI).all()
        assert (arms['sharp_near'] == ma.ARM_LOG).all() and ls['sharp_near'].min() >= -9.0 and ls['sharp_near'].max() <= -5.0
        assert cd['sharp_near'].max() > 1e-2 and cd['sharp_near'].min() < 1e-4          # large and small, both on the log arm
        assert (arms['sharp_far'] == ma.ARM_MID).all() and ls['sharp_far'].min() >= -9.0 and ls['sharp_far'].max() <= -5.0
        both = (arms['mixed'] == ma.ARM_LOG).any(axis=1) & (arms['mixed'] == ma.ARM_MID).any(axis=1)
        assert both.all()
        lp = ma.GROUPS['mixed']['P'][:, :10]
        assert (lp.min(axis=1) == -30.0).all() and (np.sort(lp, axis=1)[:, -1] - np.sort(lp, axis=1)[:, -2] >= 3.0).all()
        assert floor['floor'].any(axis=1).all() and (~floor['floor']).any(axis=1).all() and floor['floor'].sum(axis=1).min() >= 3
        assert ((arms['floor'] == ma.ARM_LOG) & floor['floor']).any() and ((arms['floor'] == ma.ARM_MID) & floor['floor']).any()
        assert (arms['floor_far'] == ma.ARM_MID).all()
        assert (floor['floor_far'].all() if part == 'first' else floor['floor_far'][:5].all() and not floor['floor_far'][5:].all())
        assert np.abs(ls['wide'][:ma.GROUPS['wide']['y'].shape[1]]).max() <= 2.0 and (arms['wide'] >= ma.ARM_LOG).all()
    assert (ma.expected_arms(*ma.rows_of(ma.GROUPS['wide'])) == ma.ARM_LOG).any()


@pytest.mark.parametrize('name', NAMES)
def test_float64_loss_and_gradient_are_finite(name):
    logits, y = ma.rows_of(ma.GROUPS[name])
    yh = torch.from_numpy(logits).double()[None].requires_grad_(True)
    loss = tr.discretized_mix_logistic_loss(yh, torch.from_numpy(y).double()[None])
    loss.backward()
    loss = float(loss.detach())
    assert np.isfinite(loss) and torch.isfinite(yh.grad).all()
    if name == 'floor_far':
        assert loss > 1e12
    else:
        assert abs(loss) < 1e3
    # a raw log-scale below the floor gets no gradient (torch.clamp)
    assert (yh.grad[0, :, 20:][torch.from_numpy(ma.at_floor(logits))] == 0).all()


def _threshold_rows():
    return np.tile(ma.THRESHOLD_P, (4, 1)), ma.THRESHOLD_Y


def _threshold_record(loss_fn, **kw):
    logits, y = _threshold_rows()
    rec = dict(y_bits=[int(v) for v in y.view(np.uint32)], edge_arm=[], loss_f32=[])
    for i in range(4):
        arm, loss = arms_taken(loss_fn, logits[i:i + 1], y[i:i + 1], torch.float32, **kw)
        assert (arm == arm[0, 0]).all()
        rec['edge_arm'].append(int(arm[0, 0]))
        rec['loss_f32'].append(loss)
    return rec


def _check_threshold_record(rec):
    with open(GOLDEN) as f:
        want = json.load(f)
    assert rec['y_bits'] == want['y_bits'] and rec['edge_arm'] == want['edge_arm']
    for a, b in zip(rec['loss_f32'], want['loss_f32']):
        assert abs(a - b) <= 2e-6 * max(1.0, abs(b)), (a, b)
    return want


def test_threshold_pair_fixture():
    """The pair on +-0.999: float32(0.999) is not above the float32 threshold, its successor is -- while in float64 BOTH are above 0.999,
    which is why the recorded float32 result, not the float64 restatement, is the expectation.  The two sides differ by nats, not by rounding."""
    want = _check_threshold_record(_threshold_record(tr.discretized_mix_logistic_loss))
    assert want['edge_arm'] == [ma.ARM_MID, ma.ARM_EDGE_HI, ma.ARM_MID, ma.ARM_EDGE_LO]
    logits, y = _threshold_rows()
    assert (ma.expected_arms(logits, y)[:, 0] == [ma.ARM_EDGE_HI, ma.ARM_EDGE_HI, ma.ARM_EDGE_LO, ma.ARM_EDGE_LO]).all()
    ls = want['loss_f32']
    assert abs(ls[0] - ls[1]) > 1.0 and abs(ls[2] - ls[3]) > 1.0


@pytest.mark.skipif(not ref_harness.reference_available(), reason='reference tree not present')
def test_threshold_pair_through_the_reference():
    """The reference's own discretized_mix_logistic_loss in float32 on the threshold pair reproduces the committed fixture."""
    ref = ref_harness.load_reference()
    _check_threshold_record(_threshold_record(ref.dist.discretized_mix_logistic_loss, y_trailing_axis=True))


@pytest.mark.skipif(not ref_harness.reference_available(), reason='reference tree not present')
@pytest.mark.parametrize('name', NAMES)
def test_the_reference_takes_the_expected_arm(name):
    """The reference's float32 loss takes the builder's arm at every (row, component) and agrees with the restatement's value."""
    ref = ref_harness.load_reference()
    logits, y = ma.rows_of(ma.GROUPS[name])
    got, loss = arms_taken(ref.dist.discretized_mix_logistic_loss, logits, y, torch.float32, y_trailing_axis=True)
    np.testing.assert_array_equal(got, ma.expected_arms(logits, y))
    mine = float(tr.discretized_mix_logistic_loss(torch.from_numpy(logits)[None], torch.from_numpy(y)[None]))
    assert abs(loss - mine) <= 2e-6 * max(1.0, abs(mine)), (loss, mine)


def test_sampler_noise_margins_and_coverage():
    nz = ma.sampler_noise(1100, 8)
    u_mix, u_log = nz['u_mix'], nz['u_log']
    assert u_mix.dtype == np.float32 and u_mix.shape == (1100, 8, 10) and u_log.shape == (1100, 8)
    assert u_mix.min() > 0.0 and u_mix.max() < 1.0 and u_log.min() >= np.float32(1e-5) and u_log.max() <= np.float32(1.0 - 1e-5)
    sc = ma.gumbel_scores(ma.SAMPLER_P, u_mix)
    np.testing.assert_array_equal(sc.argmax(axis=2), nz['winner'])
    top = np.sort(sc, axis=2)
    assert (top[..., -1] - top[..., -2]).min() >= ma.GUMBEL_MARGIN
    ls = ma.SAMPLER_P[20:]
    for r in range(8):
        for ph in range(4):
            assert set(nz['winner'][nz['phase'][:, r] == ph, r].tolist()) == set(range(10)), (r, ph)
        assert (u_log[nz['phase'][:, r] == 0, r] == np.float32(1e-5)).all() and (u_log[nz['phase'][:, r] == 1, r] == np.float32(1.0 - 1e-5)).all()
        assert (u_log[nz['phase'][:, r] == 2, r] == 0.5).all()
    assert (ls[[0, 4]] < ma.LOG_SCALE_MIN).all() and ls[1] == 0 and ls[2] == 0 and ls[3] == -9.0
    assert ma.SAMPLER_P[11] == np.float32(0.99) and ma.SAMPLER_P[12] == np.float32(-0.99)
    # rows get different noise
    assert len({u_mix[:, r].tobytes() for r in range(8)}) == 8
