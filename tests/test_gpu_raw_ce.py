"""MI355X: the RAW cross-entropy loss (`ce_rows_kernel` + `mean_kernel`, csrc/losses.hip) and its gradient (`ce_grad_kernel`,
csrc/train.hip) on the chosen logits of tests/raw_ce.py: peaked like a trained model's, offset to 32 / 1024 / 30 000, underflowing,
masked with -inf, tied -- at the row counts where the two loss kernels branch and at every class count `wrnn_create` accepts.

    loss            every group x rows 1, 3, 4, 5 (the 4-row block from both sides), 1021, 1024, 1025 (256 per-block partials, a partial
                    last block, 257 partials: `mean_kernel` strides them by 256), 512 classes, through `voc_loss`; a masked target
                    gives +inf, a target of -1 or of exactly NC gives NaN
    class counts    bits 1 ... 16, 5 rows of `mixed` and of `offset_1k`, on handles of the smallest dims the suite has (h16); bits = 16
                    is refused by `wrnn_create` (65 536 logits of a row do not fit the LDS of the any-dims loop kernel): asserted
    pinned fc3      `wrnn_train_step` with fc3.weight = 0, fc3.bias = P[0] (the construction of test_gradient_of_every_arm): fc3 outputs
                    P[0] bit for bit at every row, nothing flows below fc3, the fc3 gradients are sums of softmax - onehot rows.  Default
                    dims on the team and on the step kernels, B in {1, 5} x L = 64, groups mixed, offset_1k, underflow, ties; h16 dims
                    at bits 1, 2, 4, 6, 10, 11, 15 and (refused) 16, (B, L) = (3, 3), `mixed`
    whole step      `train_steer.steered_peaky`: steered inputs with a peaky fc3 (bias = a `mixed` row, products +-5 around it, y on the
                    argmax in 3 of 4 positions), default dims (4 n + 1, 7) on both paths, generic dims (33, 3)

Expected loss: float64 F.cross_entropy on the same float32 rows.  Bound: `raw_ce.mean_bound` -- the mean of the derived row bounds
2^-24 (|p[t] - m| + 2 |log s| + |nll| + NC / 64 + 10) plus 2^-24 |mean| for the final rounding.  Derived from the float32 format and the
length of the sums, met by torch's float32 on every row (tests/test_raw_ce_host.py); nothing of the kernel goes into it.  Gradients of
the pinned construction: 2e-5 of the float64 tensor's largest entry, the project's bound for exactly this construction; whole step: TOL
and ROW_TOL of tests/test_gpu_train_steer.py.  What was measured is in DESIGN.md 3.8 and profiles/raw_ce.txt.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import torch_ref as tr
from tests import raw_ce as rc
from tests import train_steer as ts
from tests.parity_util import parity_report
from tests.test_gpu_train_steer import ROW_TOL, TOL, _Call, _check_grads

pytestmark = pytest.mark.gpu

BITS = 9                                      # 512 classes
ROW_COUNTS = [1, 3, 4, 5, 1021, 1024, 1025]
PINNED_TOL = 2e-5
PINNED_GROUPS = ('mixed', 'offset_1k', 'underflow', 'ties')
PINNED_TINY_BITS = (1, 2, 4, 6, 10, 11, 15, 16)
# `wrnn_create` takes bits 1 ... 16 as valid dims but then refuses 16 whatever the other dims are: a handle must be able to run the
# any-dims loop kernel, which keeps one row's activations (the 65 536 logits alone are 256 KiB) in 160 KiB of LDS.  32 768 classes is
# the largest count a handle exists for; the bits = 16 cases assert the refusal
REFUSED_BITS = 16
TRAIN_L = 64


@pytest.fixture(scope='module')
def loss_model():
    from tacotronv2_wavernn_chinese_amd.synth import DEFAULT_DIMS, make_state_dict
    from tacotronv2_wavernn_chinese_amd.vocoder import WaveRNN
    dims = dict(DEFAULT_DIMS, bits=BITS)
    m = WaveRNN(**dims, mode='RAW')
    m.verbose = False
    m.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in make_state_dict(0, mode='RAW', variant='default', bits=BITS).items()})
    m.to('cuda:0')
    m.eval()
    return m


@pytest.fixture(scope='module')
def handle_of():
    """dims name or ('h16', bits) -> native handle of a RAW model of those dims; kept for the module, closed after it."""
    from tacotronv2_wavernn_chinese_amd import _cabi
    handles = {}

    def get(key):
        if key not in handles:
            dims = dict(ts.dims_of('h16'), bits=key[1]) if isinstance(key, tuple) else ts.dims_of(key)
            handles[key] = _cabi.NativeVocoder(**dims, mode='RAW', device=0)
        return handles[key]

    yield get
    for nat in handles.values():
        nat.close()


def _assert_refused(bits):
    from tacotronv2_wavernn_chinese_amd import _cabi
    with pytest.raises(_cabi.WrnnError, match='must fit 160 KB of LDS'):
        _cabi.NativeVocoder(**dict(ts.dims_of('h16'), bits=bits), mode='RAW', device=0)
    parity_report(f'[raw-ce] bits {bits}: wrnn_create refuses ({1 << bits} logits of a row do not fit 160 KB of LDS); no kernel runs')


def _expected(logits, y):
    with torch.no_grad():
        return float(F.cross_entropy(torch.from_numpy(logits).double(), torch.from_numpy(y)))


def _handle_loss(nat, logits, y):
    dev = torch.device('cuda:0')
    yh, yt = torch.from_numpy(logits).to(dev).contiguous(), torch.from_numpy(y).to(dev).to(torch.int32).contiguous()
    out = torch.full((), float('nan'), device=dev)
    nat.loss(yh.data_ptr(), yt.data_ptr(), yh.shape[0], out.data_ptr(), torch.cuda.current_stream(dev).cuda_stream)
    return float(out)


def _check_loss(tag, got, logits, y):
    want, bound = _expected(logits, y), rc.mean_bound(logits, y)
    err = abs(got - want)
    parity_report(f'[raw-ce loss] {tag}: float64 {want:.9g}, kernel {got:.9g}, error {err:.3e}, bound {bound:.3e}, error / bound {err / bound:.3f}')
    assert np.isfinite(got) and err <= bound, (tag, got, want, err, bound)
    return err / bound


# ---- a. the loss, every group at the row-count edges -----------------------------------------------------------------------------------
@pytest.mark.parametrize('n_rows', ROW_COUNTS)
@pytest.mark.parametrize('name', rc.GROUP_NAMES)
def test_loss_of_every_group(loss_model, name, n_rows):
    from tacotronv2_wavernn_chinese_amd.losses import voc_loss
    logits, y = rc.rows_of(rc.group(name, BITS), n_rows)
    got = float(voc_loss(loss_model, logits[None], y[None]).item())
    _check_loss(f'{name} rows {n_rows}', got, logits, y)


def test_loss_with_a_masked_target_is_inf(loss_model):
    """Targets on -inf logits, in a call of their own: +inf, as torch returns; one such row among finite ones: +inf as well."""
    from tacotronv2_wavernn_chinese_amd.losses import voc_loss
    logits, y = rc.rows_of(rc.group('masked_target', BITS), 5)
    assert np.isposinf(_expected(logits, y))
    got = float(voc_loss(loss_model, logits[None], y[None]).item())
    assert np.isposinf(got), got
    lf, yf = rc.rows_of(rc.group('masked', BITS), 1025)
    lf, yf = np.concatenate([lf, logits[:1]]), np.concatenate([yf, y[:1]])
    assert np.isposinf(float(voc_loss(loss_model, lf[None], yf[None]).item()))
    parity_report(f'[raw-ce loss] masked_target rows 5: kernel {got}; one masked target after 1025 finite rows: inf')


@pytest.mark.parametrize('bad', [-1, 1 << BITS])
@pytest.mark.parametrize('n_rows,at', [(1, 0), (5, 4), (1025, 1024), (1025, 0)])
def test_loss_with_a_target_outside_the_classes_is_nan(loss_model, bad, n_rows, at):
    """A target of -1, and of exactly NC (torch raises for both): NaN, wherever the row stands; the same rows with a valid target: finite."""
    from tacotronv2_wavernn_chinese_amd.losses import voc_loss
    logits, y = rc.rows_of(rc.group('mixed', BITS), n_rows)
    assert np.isfinite(float(voc_loss(loss_model, logits[None], y[None]).item()))
    y = y.copy()
    y[at] = bad
    assert np.isnan(float(voc_loss(loss_model, logits[None], y[None]).item()))
    y[at] = (1 << BITS) - 1
    assert np.isfinite(float(voc_loss(loss_model, logits[None], y[None]).item()))    # the flag does not outlive the call


# ---- b. every class count ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('bits', range(1, 17))
def test_loss_at_every_class_count(handle_of, bits):
    if bits == REFUSED_BITS:
        return _assert_refused(bits)
    nat = handle_of(('h16', bits))
    for name in ('mixed', 'offset_1k'):
        logits, y = rc.rows_of(rc.group(name, bits), 5)
        _check_loss(f'{name} bits {bits} rows 5', _handle_loss(nat, logits, y), logits, y)


# ---- c. the gradient with fc3 pinned -------------------------------------------------------------------------------------------------------
def _pinned_inputs(dims, name, B, L, seed):
    """The `st` dict of tests/train_steer.py (sd, x, mels_up, aux, y) for a seeded model of `dims` with fc3.weight = 0, fc3.bias = P[0]
    and y cycling through the group's y[0]."""
    from tacotronv2_wavernn_chinese_amd.synth import make_state_dict
    g = rc.group(name, dims['bits'])
    full = make_state_dict(0, mode='RAW', variant='default', **dims)
    sd = {k: np.array(full[k], np.float32) for k in ts.GRAD_KEYS}
    sd['fc3.weight'] = np.zeros_like(sd['fc3.weight'])
    sd['fc3.bias'] = g['P'][0].copy()
    rng = np.random.Generator(np.random.PCG64(seed))
    A = dims['res_out_dims'] // 4
    ys = g['y'][0]
    return dict(sd=sd, x=rng.uniform(-1.0, 1.0, size=(B, L)).astype(np.float32), mels_up=rng.random((B, L, dims['feat_dims']), dtype=np.float32),
                aux=rng.standard_normal((B, L, 4 * A)).astype(np.float32), y=ys[(np.arange(B * L) + B) % ys.size].reshape(B, L).astype(np.int64))


def _pinned_check(tag, nat, st, path=None):
    from tacotronv2_wavernn_chinese_amd import _cabi
    dev = torch.device('cuda:0')
    P = st['sd']['fc3.bias']
    B, L = st['x'].shape
    NC = P.size
    # float64 autograd of the restatement on the same inputs
    t = {k: torch.as_tensor(v).to(dev, torch.float64).requires_grad_(True) for k, v in st['sd'].items()}
    mu = torch.as_tensor(st['mels_up']).to(dev, torch.float64).requires_grad_(True)
    au = torch.as_tensor(st['aux']).to(dev, torch.float64).requires_grad_(True)
    y_hat64 = tr.loop_forward(t, torch.as_tensor(st['x']).to(dev, torch.float64), mu, au)
    tr.loss_of('RAW', y_hat64, torch.as_tensor(st['y']).to(dev)).backward()
    assert (y_hat64.detach() == torch.from_numpy(P).to(dev, torch.float64)).all()

    c = _Call(st, 'RAW', dev)
    try:
        if path is not None:
            nat.train_force_step_kernels(path == 'steps')
        nat.train_step(c.ptrs(c.ps), c.ptrs(c.gs), c.x.data_ptr(), c.mu.data_ptr(), c.au.data_ptr(), c.y.data_ptr(), B, L, c.loss.data_ptr(),
                       c.logits.data_ptr(), c.dm.data_ptr(), c.da.data_ptr(), c.stream)
        nat.sync_status(c.stream)
        nat.train_step(c.ptrs(c.ps), None, c.x.data_ptr(), c.mu.data_ptr(), c.au.data_ptr(), c.y.data_ptr(), B, L, c.loss2.data_ptr(), 0, 0, 0, c.stream)
        nat.sync_status(c.stream)
    finally:
        if path is not None:
            nat.train_force_step_kernels(False)
    torch.cuda.synchronize()
    # fc3 outputs: P, bit for bit, at every row
    np.testing.assert_array_equal(c.logits.cpu().numpy().view(np.uint32), np.broadcast_to(P.view(np.uint32), (B, L, NC)))
    rows = np.ascontiguousarray(np.broadcast_to(P, (B * L, NC)))
    got_loss = float(c.loss)
    ratio = _check_loss(f'pinned {tag}', got_loss, rows, st['y'].reshape(-1))
    assert np.float32(got_loss).view(np.uint32) == np.float32(float(c.loss2)).view(np.uint32)      # g = NULL: the same bits
    grads = c.got()
    worst = {}
    for k in ('fc3.bias', 'fc3.weight'):
        want = t[k].grad.cpu().numpy()
        assert np.isfinite(grads[k]).all() and np.isfinite(want).all() and np.abs(want).max() > 0
        worst[k] = float(np.abs(grads[k] - want).max() / np.abs(want).max())
    parity_report(f'[raw-ce grad] pinned {tag}: loss error / bound {ratio:.3f}; error of the largest entry: fc3.bias {worst["fc3.bias"]:.2e}, '
                  f'fc3.weight {worst["fc3.weight"]:.2e}')
    assert worst['fc3.bias'] <= PINNED_TOL and worst['fc3.weight'] <= PINNED_TOL, worst
    # nothing flows below fc3: exact zeros (a NaN or inf in dY times the zero weight would be a NaN here)
    for k in _cabi.LOOP_PARAM_KEYS[:-2]:
        assert not grads[k].any() and np.isfinite(grads[k]).all(), k
        assert not t[k].grad.any(), k
    for k in ('d_mels_up', 'd_aux'):
        assert not grads[k].any() and np.isfinite(grads[k]).all(), k


@pytest.mark.parametrize('path', ['team', 'steps'])
@pytest.mark.parametrize('B', [1, 5])
@pytest.mark.parametrize('name', PINNED_GROUPS)
def test_gradient_with_fc3_pinned(loss_model, name, B, path):
    from tacotronv2_wavernn_chinese_amd.synth import DEFAULT_DIMS
    nat = loss_model._native_handle()
    ok, _, why = nat.team_info()
    if path == 'team' and not ok:
        pytest.skip(why or 'team_info: the team kernels cannot run')
    st = _pinned_inputs(dict(DEFAULT_DIMS, bits=BITS), name, B, TRAIN_L, 100 + B)
    _pinned_check(f'{name} B {B} L {TRAIN_L} {path}', nat, st, path)


@pytest.mark.parametrize('bits', PINNED_TINY_BITS)
def test_gradient_with_fc3_pinned_at_every_class_count(handle_of, bits):
    """h16 dims, (B, L) = (3, 3).  With fc3.weight = 0 the only contraction over NC multiplies by zeros and no long float32 sum is
    involved, so the 2e-5 holds at 32 768 classes as at 2."""
    if bits == REFUSED_BITS:
        return _assert_refused(bits)
    nat = handle_of(('h16', bits))
    st = _pinned_inputs(dict(ts.dims_of('h16'), bits=bits), 'mixed', 3, 3, 200 + bits)
    _pinned_check(f'mixed bits {bits} B 3 L 3', nat, st)
    assert nat.train_last_recurrence() == ('steps', 0)


# ---- d. the gradient through the whole step ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case,path', [(c, p) for c in ts.PEAKY_CASES for p in (('team', 'steps') if c[0] == 'default' else ('steps',))],
                         ids=lambda v: v if isinstance(v, str) else f'{v[0]}-B{ts.spec_id(v[1])}-L{v[2]}')
def test_train_step_on_peaky_steered_inputs(handle_of, case, path):
    dims_name, spec, L = case
    dev = torch.device('cuda:0')
    nat = handle_of(dims_name)
    ok, n, why = nat.team_info()
    if path == 'team' and not ok:
        pytest.skip(why or 'team_info: the team kernels cannot run')
    B = ts.batch_of(spec, n if n >= 1 else 8)
    st = ts.steered_peaky(B, L, ts.peaky_seed(case), ts.dims_of(dims_name), device=dev)
    ref = ts.reference(st, 'RAW', device=dev)
    c = _Call(st, 'RAW', dev)
    try:
        nat.train_force_step_kernels(path == 'steps')
        nat.train_step(c.ptrs(c.ps), c.ptrs(c.gs), c.x.data_ptr(), c.mu.data_ptr(), c.au.data_ptr(), c.y.data_ptr(), B, L, c.loss.data_ptr(),
                       c.logits.data_ptr(), c.dm.data_ptr(), c.da.data_ptr(), c.stream)
        nat.sync_status(c.stream)
        nat.train_step(c.ptrs(c.ps), None, c.x.data_ptr(), c.mu.data_ptr(), c.au.data_ptr(), c.y.data_ptr(), B, L, c.loss2.data_ptr(), 0, 0, 0, c.stream)
        nat.sync_status(c.stream)
    finally:
        nat.train_force_step_kernels(False)
    loss, loss2 = float(c.loss), float(c.loss2)
    e_loss = abs(loss - ref['loss']) / abs(ref['loss'])
    e_log = float(np.abs(c.logits.cpu().numpy() - ref['logits']).max() / np.abs(ref['logits']).max())
    got = c.got()
    worst, where, row_worst = ts.worst_errors(got, ref['grads'])
    tag = f'[raw-ce step] peaky steered {dims_name} B {B} L {L} {path}: loss {e_loss:.2e}, logits {e_log:.2e},'
    parity_report(f'{tag} gradients {worst:.2e} ({where}), per row of d_mels_up / d_aux {row_worst:.2e} (bounds {TOL:g}, {ROW_TOL:g})')
    _check_grads(tag, got, ref, L)
    assert e_loss <= TOL and loss2 == loss and e_log <= TOL, (tag, loss, loss2, ref['loss'])
