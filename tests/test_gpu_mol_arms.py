"""MI355X: every arm of the MOL loss (`mol_rows_kernel`, csrc/losses.hip), of its gradient (`mol_grad_kernel`, csrc/train.hip) and the
floor / clamps of the MOL sampler in the four loop kernels, driven with the chosen logits of tests/mol_arms.py.

The loss takes logits directly.  For the gradient and the sampler the model is an ordinary seeded MOL state dict with fc3.weight = 0 and
fc3.bias = P: fc3 then outputs P at every row and step whatever the recurrent state is, all variation comes from y (loss, gradient) or from
the injected noise (sampler), and no gradient flows below fc3 (W_fc3^T . dY = 0) -- so every other gradient must be exactly zero, and a
NaN or inf anywhere in dY would show there.  tests/test_mol_arms_host.py asserts on the CPU that the fixtures reach the arms they claim."""
import json
import os

import numpy as np
import pytest
import torch

from oracle import oracle as orc
from oracle import torch_ref as tr
from tests import mol_arms as ma

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'mol_arms_threshold.json')
NAMES = sorted(ma.GROUPS)
ROW_COUNTS = [1, 255, 256, 257, 1000]     # one row; the 256-thread block edge from both sides; four blocks with a partial last one
# The kernel may be K times as far from the float64 loss as the float32 restatement (the reference's arithmetic) is.  Measured on the MI355X
# (DESIGN.md 3.8): error / g is 0.001 .. 1.000 over the 40 cases -- `mol_rows_kernel` evaluates the arm values in double and rounds once, so
# it returns the float nearest the float64 loss, which no float32 number (the restatement's result is one) beats.  K = 2: the smallest
# power of two at least twice the worst ratio.
K = 2.0
TRAIN_L = 64                              # the shortest length tried; wrnn_train_step accepts it (any L >= 1 at these dims)


def _state_dict(P=None):
    from tacotronv2_wavernn_chinese_amd.synth import make_state_dict
    sd = dict(make_state_dict(0, mode='MOL', variant='default', bits=9))
    if P is not None:
        sd['fc3.weight'] = np.zeros_like(np.asarray(sd['fc3.weight']))
        sd['fc3.bias'] = np.asarray(P, np.float32).copy()
    return sd


def _model(sd, kernel='auto', train=False):
    from tacotronv2_wavernn_chinese_amd import _cabi
    from tacotronv2_wavernn_chinese_amd.synth import DEFAULT_DIMS
    from tacotronv2_wavernn_chinese_amd.vocoder import WaveRNN
    dims = dict(DEFAULT_DIMS)
    dims['bits'] = 9
    m = WaveRNN(**dims, mode='MOL')
    m.verbose = False
    m.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in sd.items()})
    m.to('cuda:0')
    m.kernel = _cabi.KERNEL_IDS[kernel]
    m.train() if train else m.eval()
    return m


@pytest.fixture(scope='module')
def loss_model():
    return _model(_state_dict())


def _device_loss(m, logits, y):
    from tacotronv2_wavernn_chinese_amd.losses import voc_loss
    return float(voc_loss(m, logits[None], y[None]).item())


def _ref_loss(logits, y, dtype):
    return float(tr.discretized_mix_logistic_loss(torch.from_numpy(logits).to(dtype)[None], torch.from_numpy(y).to(dtype)[None]))


# ---- forward loss ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n_rows', ROW_COUNTS)
@pytest.mark.parametrize('name', NAMES)
def test_loss_of_every_arm(loss_model, name, n_rows):
    """wrnn_loss on one group per call (it returns a mean; floor_far would swamp any other group) against the float64 restatement on the
    same float32 inputs.  g = |float32 restatement - float64 restatement| is what the reference's own arithmetic loses on these rows; the
    kernel passes within K g, or within 2e-6 max(1, |loss|) (the bound of tests/test_forward_loss.py) where g is 0."""
    logits, y = ma.rows_of(ma.GROUPS[name], n_rows)
    ref64, ref32 = _ref_loss(logits, y, torch.float64), _ref_loss(logits, y, torch.float32)
    got = _device_loss(loss_model, logits, y)
    g, err = abs(ref32 - ref64), abs(got - ref64)
    print(f'\n[mol-arms loss] {name} rows {n_rows}: float64 {ref64:.9g}, float32 {ref32:.9g}, kernel {got:.9g}; g {g:.3e}, error {err:.3e}, '
          f'error / g {err / g if g > 0 else float("nan"):.3f}')
    assert np.isfinite(got)
    assert err <= (K * g if g > 0 else 2e-6 * max(1.0, abs(ref64))), (name, n_rows, got, ref64, ref32)


def test_loss_on_the_edge_threshold(loss_model):
    """y = float32(0.999), its float32 successor and both mirrored: the side the reference's float32 comparison takes, recorded from the
    reference itself (tests/golden/mol_arms_threshold.json).  The float64 restatement would put all four on the edge arm."""
    with open(GOLDEN) as f:
        want = json.load(f)
    assert [int(v) for v in ma.THRESHOLD_Y.view(np.uint32)] == want['y_bits']
    for i, ref in enumerate(want['loss_f32']):
        got = _device_loss(loss_model, ma.THRESHOLD_P[None], ma.THRESHOLD_Y[i:i + 1])
        print(f'\n[mol-arms threshold] y bits {want["y_bits"][i]:#x} (arm {want["edge_arm"][i]}): reference {ref:.7f}, kernel {got:.7f}')
        assert abs(got - ref) <= 2e-6 * max(1.0, abs(ref)), (i, got, ref)


# ---- gradient --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('B', [1, 5])
@pytest.mark.parametrize('name', NAMES)
def test_gradient_of_every_arm(name, B):
    """wrnn_train_step (g != NULL) on the fc3.weight = 0, fc3.bias = P[0] model, y cycling through the group's y[0]; L = 64."""
    from tacotronv2_wavernn_chinese_amd import _cabi
    from tacotronv2_wavernn_chinese_amd.synth import make_mels
    grp = ma.GROUPS[name]
    P, ys = grp['P'][0], grp['y'][0]
    L = TRAIN_L
    sd = _state_dict(P)
    m = _model(sd, train=True)
    dev = torch.device('cuda:0')
    rng = np.random.Generator(np.random.PCG64(100 + B))
    x = rng.uniform(-1.0, 1.0, size=(B, L)).astype(np.float32)
    y = ys[(np.arange(B * L) + B) % ys.size].reshape(B, L).astype(np.float32)
    # float32 conditioning from the float64 restatement (eval-mode upsample network on one frame + padding), shared by both sides
    sd64 = {}
    for k, v in sd.items():
        t = torch.as_tensor(np.asarray(v))
        if t.is_floating_point():
            t = t.to(dev, torch.float64).requires_grad_(not k.endswith(('running_mean', 'running_var')))
        sd64[k] = t
    with torch.no_grad():
        mu64, au64 = tr.upsample(sd64, torch.from_numpy(make_mels(40 + B, B, 5)).to(dev, torch.float64), training=False)
    mu, au = mu64[:, :L].float().contiguous(), au64[:, :L].float().contiguous()
    mu64, au64 = mu.double().requires_grad_(True), au.double().requires_grad_(True)
    y_hat64 = tr.loop_forward(sd64, torch.from_numpy(x).to(dev, torch.float64), mu64, au64)
    loss64 = tr.loss_of('MOL', y_hat64, torch.from_numpy(y).to(dev))
    loss64.backward()
    ref_loss = float(loss64.detach())

    xt, yt = torch.from_numpy(x).to(dev), torch.from_numpy(y).to(dev).contiguous()
    ps = [p.detach().contiguous() for p in m._loop_params()]
    gs = [torch.full_like(p, float('nan')) for p in ps]
    dm, da = torch.full_like(mu, float('nan')), torch.full_like(au, float('nan'))
    loss, loss2 = torch.empty((), device=dev), torch.empty((), device=dev)
    logits = torch.full((B, L, 30), float('nan'), device=dev)
    nat = m._native_handle()
    st = torch.cuda.current_stream(dev).cuda_stream
    nat.train_step([p.data_ptr() for p in ps], [g.data_ptr() for g in gs], xt.data_ptr(), mu.data_ptr(), au.data_ptr(), yt.data_ptr(), B, L,
                   loss.data_ptr(), logits.data_ptr(), dm.data_ptr(), da.data_ptr(), st)
    nat.train_step([p.data_ptr() for p in ps], None, xt.data_ptr(), mu.data_ptr(), au.data_ptr(), yt.data_ptr(), B, L, loss2.data_ptr(), 0, 0, 0, st)
    nat.sync_status(st)
    torch.cuda.synchronize()

    # fc3 outputs: P, bit for bit, at every row -- on both sides
    np.testing.assert_array_equal(logits.cpu().numpy().view(np.uint32), np.broadcast_to(P.view(np.uint32), (B, L, 30)))
    assert (y_hat64.detach() == torch.from_numpy(P).to(dev, torch.float64)).all()
    got_loss = float(loss)
    assert np.isfinite(got_loss) and float(loss2) == got_loss
    grads = {k: g.cpu().numpy() for g, k in zip(gs, _cabi.LOOP_PARAM_KEYS)}
    worst = {}
    for k in ('fc3.bias', 'fc3.weight'):
        want = sd64[k].grad.cpu().numpy()
        assert np.isfinite(grads[k]).all() and np.isfinite(want).all()
        worst[k] = float(np.abs(grads[k] - want).max() / max(np.abs(want).max(), 1e-300))
    print(f'\n[mol-arms grad] {name} B {B} L {L}: loss {got_loss:.9g} (float64 {ref_loss:.9g}, rel {abs(got_loss - ref_loss) / abs(ref_loss):.2e}); '
          f'error of the largest entry: fc3.bias {worst["fc3.bias"]:.2e}, fc3.weight {worst["fc3.weight"]:.2e}')
    assert worst['fc3.bias'] <= 2e-5 and worst['fc3.weight'] <= 2e-5, worst
    # nothing flows below fc3: exact zeros (a NaN or inf in dY times the zero weight would be a NaN here)
    for k in _cabi.LOOP_PARAM_KEYS[:-2]:
        assert not grads[k].any() and np.isfinite(grads[k]).all(), k
        assert not sd64[k].grad.any(), k
    for t_, nm in ((dm, 'd_mels_up'), (da, 'd_aux')):
        v = t_.cpu().numpy()
        assert not v.any() and np.isfinite(v).all(), nm
    # a raw log-scale below the floor gets no gradient
    below = np.flatnonzero(ma.at_floor(P[None])[0])
    if name in ('floor', 'floor_far'):
        assert below.size >= 3
    assert not grads['fc3.bias'][20 + below].any() and not sd64['fc3.bias'].grad.cpu().numpy()[20 + below].any()
    if name == 'floor':
        assert grads['fc3.bias'][20:][~ma.at_floor(P[None])[0]].any()
    if name == 'floor_far':
        assert got_loss > 1e12 and abs(got_loss - ref_loss) <= 1e-6 * abs(ref_loss), (got_loss, ref_loss)


# ---- sampler ---------------------------------------------------------------------------------------------------------------------------
_SAMPLER = {}


def _sampler_reference(B):
    """Oracle run (about a second) on the same weights, conditioning and noise: once per B."""
    from tacotronv2_wavernn_chinese_amd.synth import make_mels
    if 'sd' not in _SAMPLER:
        _SAMPLER['sd'] = _state_dict(ma.SAMPLER_P)
        _SAMPLER['noise'] = ma.sampler_noise(1100, 8)
        _SAMPLER['om'] = orc.OracleModel(_SAMPLER['sd'], mode='MOL', bits=9, fast=True)
    if B not in _SAMPLER:
        nz = _SAMPLER['noise']
        mels = make_mels(60 + B, B, 4)
        u_mix, u_log = np.ascontiguousarray(nz['u_mix'][:, :B]), np.ascontiguousarray(nz['u_log'][:, :B])
        cm, ca = _SAMPLER['om'].conditioning(mels)
        ref = _SAMPLER['om'].loop(cm, ca, 0, u_mix, u_log)
        xf = np.random.Generator(np.random.PCG64(B)).uniform(-1.0, 1.0, size=u_log.shape).astype(np.float32)
        _SAMPLER[B] = dict(mels=mels, u_mix=u_mix, u_log=u_log, ref=ref, xf=xf, winner=nz['winner'][:, :B], phase=nz['phase'][:, :B])
    return _SAMPLER['sd'], _SAMPLER[B]


@pytest.mark.parametrize('kernel,B,batch_rows', [('team2', 1, 0), ('batch_cs', 4, 0), ('batch_cs', 8, 8), ('batch', 4, 0), ('simple', 2, 0)])
def test_sampler_floor_and_clamps(kernel, B, batch_rows):
    """generate_raw with injected noise, 4 frames = 1 100 steps, free-running and with x_forced, against the oracle.  The noise makes
    component (t + row) % 10 win by at least 1e-3 and walks u_log through 1e-5, 1 - 1e-5, 0.5 and ordinary draws."""
    from tacotronv2_wavernn_chinese_amd import _cabi
    from tests.parity_util import check_mol
    sd, c = _sampler_reference(B)
    m = _model(sd, kernel)
    kw = dict(noise_mode=_cabi.NOISE_INJECTED, noise1=c['u_mix'], noise2=c['u_log'], batch_rows=batch_rows)
    free = m.generate_raw(c['mels'], False, 11000, 550, **kw)
    assert m.last_timing['kernel'] == _cabi.KERNEL_IDS[kernel]
    smp, mix = free['samples'].cpu().numpy().T, free['labels'].cpu().numpy().T        # (L, rows)
    forced = m.generate_raw(c['mels'], False, 11000, 550, x_forced=c['xf'], **kw)
    assert smp.shape == (1100, B)
    # the logits do not depend on the fed-back value: the forced run draws the very same samples
    np.testing.assert_array_equal(forced['samples'].cpu().numpy().T.view(np.uint32), smp.view(np.uint32))
    np.testing.assert_array_equal(forced['labels'].cpu().numpy().T, mix)
    ref = c['ref']
    np.testing.assert_array_equal(ref['labels'], c['winner'])
    np.testing.assert_array_equal(mix, ref['labels'])                                  # no near-tie allowance: the margins rule it out
    check_mol(smp, mix, ref, teacher_forced=True)                                      # 2e-5, the teacher-forced MOL bound
    err = float(np.abs(smp - ref['samples']).max())
    assert err <= 2e-5
    mean, raw_ls = ma.SAMPLER_P[10:20], ma.SAMPLER_P[20:]
    for k in np.flatnonzero(raw_ls < ma.LOG_SCALE_MIN):                               # at the floor: the sample IS the mean
        assert (mix == k).sum() >= 100
        np.testing.assert_array_equal(smp[mix == k].view(np.uint32), np.full(int((mix == k).sum()), mean[k], np.float32).view(np.uint32))
    hi, lo = (mix == 1) & (c['phase'] == 1), (mix == 2) & (c['phase'] == 0)            # mean +-0.99, log-scale 0, u_log at the matching extreme
    assert hi.sum() >= 20 and lo.sum() >= 20
    assert (smp[hi] == 1.0).all() and (smp[lo] == -1.0).all()
    sharp = mix == 3                                                                   # log-scale -9: |logit(u)| <= 11.513 for u in [1e-5, 1 - 1e-5]
    assert sharp.sum() >= 100 and (np.abs(smp[sharp].astype(np.float64) - float(mean[3])) <= np.exp(-9.0) * 11.6).all()
    assert np.abs(smp[sharp] - mean[3]).max() > np.exp(-9.0) * 5.0                     # and the scale is not zero either
    assert np.abs(smp).max() <= 1.0
    print(f'\n[mol-arms sampler] {kernel} B {B}: 1100 steps x {B} rows, mixture index equal everywhere, max |sample error| {err:.3e}')
