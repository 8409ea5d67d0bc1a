"""CPU: the chosen-logit fixtures of tests/raw_ce.py are what they claim to be, and the bound the GPU tests hold the kernels to is one
the reference's own float32 arithmetic meets.

Asserted, not assumed: the regime of every group from the float64 softmax of its rows (where s rounds to 1, which entries underflow to 0
or to a subnormal in float32, the loss range, the target coverage); torch's float32 `F.cross_entropy` and the oracle's
`cross_entropy_rows` within `raw_ce.row_bound` on every row of every group at every class count 2 ... 65 536; torch float32's fc3
gradients within 2e-6 of the float64 tensor's largest entry on the fc3-pinned fixtures of the gradient test; and for the peaky whole-step
inputs (`train_steer.steered_peaky`) the masks, the margins, the hit / miss mix and torch float32 within 2e-6 on every gradient.

The form `(m + log s) - p[t]`, which the oracle and `ce_rows_kernel` had, is evaluated here in float32 too, as a witness that the
fixtures can tell the two forms apart.  On the peaky rows log s is ~1e-8 and that form happens to be exact (m + log s rounds to m); the
spread rows of the offset groups are what it fails on.

Measured, worst error / bound over the rows of a group at 512 classes (torch float32 | oracle | the old form): uniform 0.19 | 0.19 |
0.23; peaky_hit 0.02 | 0.02 | 0.02; peaky_miss and mixed 0.36 | 0.36 | 0.36; offset_32 0.27 | 0.27 | 1.10; offset_1k 0.24 | 0.24 | 33;
offset_30k 0.22 | 0.20 | 532; underflow 0.39 | 0.39 | 0.27; masked 0.30 | 0.30 | 0.30; ties 0.19 | 0.19 | 0.23.  Over all class counts
torch float32 and the oracle stay under 0.61.  The mean of the first 5 rows in the old form: 4.7 bounds off at offset_1k, 69 at
offset_30k (512 classes).  Pinned fc3, torch float32 against float64: fc3.bias 7.5e-9 ... 4.2e-7, fc3.weight 4.3e-8 ... 6.9e-7 (bound
2e-6).  Peaky steered inputs: 6.4e-7 (default dims, B = 33, L = 7) and 5.6e-7 (generic, B = 33, L = 3) on the worst tensor, 7.1e-7 and
5.3e-6 per row of d_mels_up / d_aux.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import oracle as orc
from oracle import torch_ref as tr
from tests import raw_ce as rc
from tests import train_steer as ts

ALL_BITS = list(range(1, 17))
N_TEAMS = 8
PINNED_GROUPS = ('mixed', 'offset_1k', 'underflow', 'ties')          # the gradient cases of tests/test_gpu_raw_ce.py
PINNED_TINY_BITS = (1, 2, 4, 6, 10, 11, 15, 16)


def _torch_rows(logits, y, dtype):
    with torch.no_grad():
        return F.cross_entropy(torch.from_numpy(logits).to(dtype), torch.from_numpy(y), reduction='none').double().numpy()


def _old_form_rows(logits, y):
    """(m + log s) - p[t] in float32: what the oracle and the kernel evaluated before."""
    m = logits.max(axis=1, keepdims=True)
    with np.errstate(under='ignore', divide='ignore'):
        lse = (m[:, 0] + np.log(np.exp(logits - m).sum(axis=1, dtype=np.float32))).astype(np.float32)
    return (lse - logits[np.arange(logits.shape[0]), y]).astype(np.float64)


@pytest.mark.parametrize('bits', ALL_BITS)
def test_fixture_shapes_and_target_coverage(bits):
    nc = 1 << bits
    for name in rc.GROUP_NAMES + ('masked_target',):
        g = rc.group(name, bits)
        P, y = g['P'], g['y']
        assert P.dtype == np.float32 and y.dtype == np.int64 and P.shape[1] == nc and y.shape == (P.shape[0], rc.K)
        assert not np.signbit(P[P == 0]).any() and not np.isnan(P).any()
        assert y.min() >= 0 and y.max() < nc
        logits, yy = rc.rows_of(g)
        pi, pj = rc.pair_index(g)
        assert logits.shape == (y.size, nc) and np.array_equal(yy, y[pi, pj]) and len(set(zip(pi.tolist(), pj.tolist()))) == y.size
        assert np.array_equal(pi[:P.shape[0]], np.arange(P.shape[0]))          # a few rows already come from different P
        l5, y5 = rc.rows_of(g, 5)
        assert np.array_equal(l5, logits[:5]) and np.array_equal(y5, yy[:5])
        lf, yf = rc.rows_of(g, 2 * rc.K + 1, first_only=True)
        assert (lf.view(np.uint32) == P[0].view(np.uint32)).all() and np.array_equal(yf[:rc.K], y[0]) and yf[-1] == y[0, 0]
        if name == 'masked_target':
            assert np.isneginf(logits[np.arange(yy.size), yy]).all()
            continue
        assert np.isfinite(logits[np.arange(yy.size), yy]).all()
        fin = np.where(np.isfinite(logits), logits, np.nan)
        hit = set(yy.tolist())
        if name not in ('peaky_hit', 'masked'):                # peaky_hit: the target IS the peak, which walks over these classes
            assert {0, nc - 1} <= hit and (nc <= 64 or {63, 64} <= hit), (name, sorted(hit))
            assert (yy == np.nanargmin(fin, axis=1)).any(), name
        if name not in ('peaky_miss', 'masked'):
            assert (fin[np.arange(yy.size), yy] == np.nanmax(fin, axis=1)).any(), name
    peaks = set(rc.group('peaky_hit', bits)['y'][:, 0].tolist())
    assert {0, nc - 1} <= peaks and (nc <= 64 or {63, 64} <= peaks)
    ym = np.concatenate([rc.group('masked', bits)['y'].reshape(-1), rc.group('masked_target', bits)['y'].reshape(-1)])
    assert {0, nc - 1} <= set(ym.tolist())                     # an end of the row is a target in one of the two, whichever is masked


@pytest.mark.parametrize('bits', ALL_BITS)
def test_every_group_reaches_its_regime(bits):
    nc = 1 << bits
    T = {n: rc.row_terms64(*rc.rows_of(rc.group(n, bits))) for n in rc.GROUP_NAMES}
    R = {n: rc.rows_of(rc.group(n, bits)) for n in rc.GROUP_NAMES}
    I = {n: rc.pair_index(rc.group(n, bits)) for n in rc.GROUP_NAMES}      # (P row, target slot) of every row
    # uniform: equal logits give log NC exactly; N(0, 0.05) stays within 1.5 of it
    assert np.allclose(T['uniform']['nll'][I['uniform'][0] < 2], np.log(nc), rtol=0, atol=1e-12) and np.abs(T['uniform']['nll'] - np.log(nc)).max() < 1.5
    assert np.abs(R['uniform'][0]).max() <= 3.75
    # peaky_hit: the loss is NC e^-25 within a factor e^2 (NC - 1 terms of mean e^(-25 + 1) or lowered classes), s rounds to 1 up to 512
    t = T['peaky_hit']
    assert (t['pt'] == t['m']).all() and (t['nll'] > 0).all() or nc == 2
    assert (t['nll'] <= nc * np.exp(-25.0) * np.e ** 2).all() and (nc < 8 or (t['nll'] >= nc * np.exp(-25.0) / np.e ** 2).all())
    if nc <= 512:
        assert (t['s'].astype(np.float32) == 1.0).all()
    else:
        assert nc < 2048 or (t['s'].astype(np.float32) > 1.0).all()
    # peaky_miss: 25 ... 40 below the maximum, a loss of 25 ... 40 (+ log s < 1e-5)
    t = T['peaky_miss']
    gap = t['m'] - t['pt']
    assert gap.min() >= 25.0 - 1e-6 and gap.max() <= 40.0 and t['nll'].min() >= 25.0 - 1e-6 and t['nll'].max() <= 40.0 + 1e-5
    # mixed: hits and misses 3 to 1, in the whole group and in the rows of P[0]
    for first_only in (False, True):
        lg, yy = rc.rows_of(rc.group('mixed', bits), first_only=first_only)
        is_hit = lg[np.arange(yy.size), yy] == lg.max(axis=1)
        pi, pj = rc.pair_index(rc.group('mixed', bits), first_only=first_only)
        assert is_hit.mean() == 0.75 and np.array_equal(is_hit, (pj + 3 * pi) % 4 != 3) and is_hit[:3].all() == first_only
    # offsets: P rows in threes (mixed, spread, peaky_miss), the maximum where it says; the peaky rows keep the targets and -- up to the
    # rounding of the shifted rows -- the losses of mixed / peaky_miss; the spread rows have a log s that is not negligible and a
    # log-sum-exp 0.30 ... 0.45 of a float32 spacing above the grid at the size of m
    n_p = rc.group('mixed', bits)['P'].shape[0]
    for name, off in rc.OFFSETS.items():
        g, t, (lg, yy), (pi, pj) = rc.group(name, bits), T[name], R[name], I[name]
        signs = (1.0, -1.0) if name == 'offset_30k' else (1.0,)
        assert g['kinds'] == [(k, sg) for sg in signs for _ in range(n_p) for k in ('mixed', 'spread', 'miss')]
        kind, sign = np.array([k for k, _ in g['kinds']])[pi], np.array([sg for _, sg in g['kinds']])[pi]
        assert np.abs(t['m'] - sign * off).max() < 0.01
        u = float(np.spacing(np.float32(off)))
        for k, src in (('mixed', 'mixed'), ('miss', 'peaky_miss')):
            sel = kind == k
            assert np.array_equal(yy[sel], rc.group(src, bits)['y'][(pi[sel] // 3) % n_p, pj[sel]])
            assert np.abs(t['nll'][sel] - rc.row_terms64(rc.group(src, bits)['P'][(pi[sel] // 3) % n_p], yy[sel])['nll']).max() <= 2 * u + 1e-12
        sp = kind == 'spread'
        frac = ((t['m'][sp] + np.log(t['s'][sp])) / u) % 1.0
        assert (np.log(t['s'][sp]) > 0.02).all() and (frac >= 0.30).all() and (frac <= 0.45).all()
        with np.errstate(over='ignore'):
            assert off < 88 or np.isinf(np.exp(lg[sign > 0].max(axis=1))).all()  # a naive exp overflows ...
        assert (np.exp(lg[sign < 0].max(axis=1)) == 0).all()                     # ... or, mirrored, leaves log(0)
    assert np.isfinite(np.exp(R['offset_32'][0])).all()
    # underflow: all but two classes dead (exactly 0 in float32) in the first rows, subnormal in the later ones
    lg, yy = R['underflow']
    with np.errstate(under='ignore'):
        e32 = np.exp((lg - lg.max(axis=1, keepdims=True)).astype(np.float32))
    live = e32 >= np.finfo(np.float32).tiny
    assert (live.sum(axis=1) == 2).all()
    early = I['underflow'][0] < 2
    first, later = e32[early][~live[early]], e32[~early][~live[~early]]
    assert (first == 0).all() and (nc == 2 or ((later > 0) & (later < np.finfo(np.float32).tiny)).all())
    on_live = live[np.arange(yy.size), yy]
    assert on_live.any() and (nc == 2 or ((~on_live).any() and T['underflow']['nll'][~on_live].min() > 88.0))
    assert T['underflow']['nll'][on_live].max() < 1.2
    # masked: -inf among the logits of every row, finite targets, finite losses
    lg, yy = R['masked']
    assert np.isneginf(lg).any(axis=1).all() and np.isfinite(T['masked']['nll']).all()
    assert nc < 16 or (0.1 < np.isneginf(lg).mean() < 0.4)
    lt, yt = rc.rows_of(rc.group('masked_target', bits))
    assert np.isposinf(rc.row_terms64(lt, yt)['nll']).all()
    # ties: two at the maximum, then all
    P = rc.group('ties', bits)['P']
    n_top = (P == P.max(axis=1, keepdims=True)).sum(axis=1)
    assert n_top.tolist() == [2, 2, nc, nc]
    assert np.allclose(T['ties']['nll'][I['ties'][0] >= 2], np.log(nc), rtol=0, atol=1e-12)


@pytest.mark.parametrize('bits', ALL_BITS)
def test_float32_cross_entropy_stays_within_the_derived_bound(bits):
    """torch's float32 F.cross_entropy and the oracle's restatement, row by row, against float64 on the same float32 rows."""
    for name in rc.GROUP_NAMES:
        logits, y = rc.rows_of(rc.group(name, bits))
        ref = _torch_rows(logits, y, torch.float64)
        assert np.abs(ref - rc.row_terms64(logits, y)['nll']).max() <= 1e-12 * max(1.0, np.abs(ref).max())      # raw_ce's numpy float64 = torch's
        bound = rc.row_bound(logits, y)
        r_t = np.abs(_torch_rows(logits, y, torch.float32) - ref) / bound
        r_o = np.abs(orc.cross_entropy_rows(logits, y).astype(np.float64) - ref) / bound
        r_old = np.abs(_old_form_rows(logits, y) - ref) / bound
        print(f'\n[raw-ce host] {name} bits {bits}: worst error / bound over {y.size} rows: torch float32 {r_t.max():.3f}, oracle {r_o.max():.3f}, '
              f'(m + log s) - p[t] {r_old.max():.3f}')
        assert r_t.max() <= 1.0, (name, bits, r_t.max())
        assert r_o.max() <= 1.0, (name, bits, r_o.max())
        mean_err = abs(orc.cross_entropy(logits[None], y[None]) - ref.mean())
        assert mean_err <= rc.mean_bound(logits, y), (name, bits)
        if name in ('offset_1k', 'offset_30k'):                 # the fixtures tell the two forms apart: in a row, and in the mean of a few rows
            few = rc.rows_of(rc.group(name, bits), 5)
            old_mean = abs(float(np.float32(_old_form_rows(*few).mean())) - _torch_rows(*few, torch.float64).mean())
            print(f'[raw-ce host] {name} bits {bits}: 5 rows, (m + log s) - p[t]: error / bound of the mean {old_mean / rc.mean_bound(*few):.2f}')
            # a spread row loses >= 0.30 spacings of m: 3.7e-5 at 1024, against 2^-24 (NC / 64 + ~30) -- above the row bound up to
            # 2^15 classes, and with 2 spread rows in 5 above the mean bound up to 2^13; at 30 000 always
            if name == 'offset_30k' or bits <= 15:
                assert r_old.max() > 1.0, (name, bits)
            if name == 'offset_30k' or bits <= 13:
                assert old_mean > rc.mean_bound(*few), (name, bits)
    lt, yt = rc.rows_of(rc.group('masked_target', bits))
    assert np.isposinf(_torch_rows(lt, yt, torch.float32)).all() and np.isposinf(orc.cross_entropy_rows(lt, yt)).all()
    assert np.isposinf(orc.cross_entropy(lt[None], yt[None]))


def _pinned_fc3_grads(P, y, f2, dtype):
    """fc3.weight = 0, fc3.bias = P: the loss and both fc3 gradients by autograd, F2 (rows, FC) the layer's input."""
    w = torch.zeros(P.size, f2.shape[1], dtype=dtype, requires_grad=True)
    b = torch.from_numpy(P.copy()).to(dtype).requires_grad_(True)
    loss = F.cross_entropy(torch.from_numpy(f2).to(dtype) @ w.t() + b, torch.from_numpy(y))
    loss.backward()
    return float(loss.detach()), b.grad.double().numpy(), w.grad.double().numpy()


@pytest.mark.parametrize('name,bits,rows', [(n, 9, r) for n in PINNED_GROUPS for r in (64, 320)] + [('mixed', b, 9) for b in PINNED_TINY_BITS])
def test_pinned_fc3_gradients_in_float32(name, bits, rows):
    """The construction of the GPU gradient test (fc3.weight = 0, fc3.bias = P[0], y cycling through y[0]): torch float32's fc3.bias and
    fc3.weight gradients stay within 2e-6 of the float64 tensor's largest entry, at every class count and row count used there."""
    g = rc.group(name, bits)
    _, y = rc.rows_of(g, rows, first_only=True)
    f2 = np.abs(np.random.Generator(np.random.PCG64(rows)).standard_normal((rows, 8))).astype(np.float32)     # a ReLU output
    l64, b64, w64 = _pinned_fc3_grads(g['P'][0], y, f2, torch.float64)
    l32, b32, w32 = _pinned_fc3_grads(g['P'][0], y, f2, torch.float32)
    eb, ew = np.abs(b32 - b64).max() / np.abs(b64).max(), np.abs(w32 - w64).max() / np.abs(w64).max()
    print(f'\n[raw-ce host] pinned {name} bits {bits} rows {rows}: torch float32 vs float64, of the largest entry: fc3.bias {eb:.2e}, fc3.weight {ew:.2e}')
    assert eb <= 2e-6 and ew <= 2e-6, (eb, ew)
    logits = np.broadcast_to(g['P'][0], (rows, g['P'].shape[1]))
    assert abs(l32 - l64) <= rc.mean_bound(logits, y)


@pytest.mark.parametrize('case', ts.PEAKY_CASES, ids=lambda c: f'{c[0]}-B{ts.spec_id(c[1])}-L{c[2]}')
def test_peaky_steered_inputs(case):
    """`steered_peaky`: the masks and margins of the steering survive the new fc3, the logits are the peaky row +-5, y hits the float64
    argmax in 3 of 4 positions, and torch's float32 evaluation stays within 2e-6 of float64 on every gradient tensor."""
    dims_name, spec, L = case
    B = ts.batch_of(spec, N_TEAMS)
    dims = ts.dims_of(dims_name)
    st = ts.steered_peaky(B, L, ts.peaky_seed(case), dims)
    assert all(v.dtype == np.float32 for v in st['sd'].values()) and st['y'].dtype == np.int64
    for p, mask in zip(ts.pre_activations64(st), (st['mask1'], st['mask2'])):
        assert np.abs(p).min() >= ts.MARGIN and np.array_equal(p > 0, mask)
    r64 = ts.reference(st, 'RAW')
    bias = st['sd']['fc3.bias'].astype(np.float64)
    dev = r64['logits'] - bias
    assert abs(np.abs(dev).max() - ts.PEAKY_SPREAD) < 1e-3 and dev.std() > 0.3
    is_hit = np.take_along_axis(r64['logits'], st['y'][..., None], axis=2)[..., 0] == r64['logits'].max(axis=2)
    assert (is_hit | ~st['hit']).all() and (0.70 <= is_hit.mean() <= 0.80 if L >= 4 else 0.64 <= is_hit.mean() <= 0.70)
    assert (~st['hit']).any(axis=1).all()                                   # every batch row has a miss: no row of ~1e-8 gradients
    assert (r64['logits'].argmax(axis=2) == bias.argmax()).all()            # +-5 does not unseat a class that is 25 ahead
    r32 = ts.reference(st, 'RAW', dtype=torch.float32)
    worst, where, row_worst = ts.worst_errors(r32['grads'], r64['grads'])
    print(f'\n[raw-ce host] peaky steered {dims_name} B={B} L={L}: loss {r64["loss"]:.4f}, torch float32 vs float64 {worst:.2e} ({where}), '
          f'per row of d_mels_up / d_aux {row_worst:.2e}')
    assert np.isfinite(r64['loss']) and all(np.isfinite(g).all() and np.abs(g).max() > 0 for g in r64['grads'].values())
    assert worst <= 2e-6, (where, worst)
    assert row_worst <= 3.26e-5, row_worst                                  # the float32 row error ROW_TOL of the GPU tests is 4 x of
