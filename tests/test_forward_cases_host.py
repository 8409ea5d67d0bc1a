"""What tests/test_gpu_forward_padded.py relies on, checked on the CPU on the float64 reference alone, for every case of tests/forward_cases.py:
the fp32 reference is within an eighth of every bound (so `8 g` is nowhere in force and the bounds are the suite's constants); the context
frames, x[:, 0] and the loop's state all move the logits by orders of magnitude more than the bound, so a kernel that reads the wrong frame,
strides the batch by T in place of T + 2 pad, clamps against T or ignores x_init cannot stay inside it.
"""
import numpy as np
import pytest

from tests import forward_cases as fc


def _forward64(name, mode, mels=None, x=None):
    import torch
    c = fc.inputs(name, mode)
    return fc.forward_of(fc.state_dict(name, mode), fc.dims(name, mode), c['mels'] if mels is None else mels, c['x'] if x is None else x, torch.float64)


@pytest.mark.parametrize('name,mode', fc.CASES)
def test_the_logit_bound_is_the_constant_and_the_context_matters(name, mode):
    d, c = fc.dims(name, mode), fc.inputs(name, mode)
    bound, g = fc.logit_bound(name, mode)
    l64 = fc.float64_forward(name, mode)[2]
    assert l64.shape == (fc.B, c['L'], fc.n_classes(name, mode)) and np.isfinite(l64).all()
    const = 2e-5 * max(1.0, float(np.abs(l64).max()))
    z64 = _forward64(name, mode, mels=fc.zero_context(c['mels'], d['pad']))[2]    # the 2 pad context frames zeroed
    ctx = float(np.abs(z64 - l64).max())
    vary = float(np.ptp(l64, axis=1).max(axis=1).min())                          # over steps: the most mobile class of the stillest row
    print(f'\n[forward padded] {name} {mode} T={c["T"]} L={c["L"]}: max |logit| {float(np.abs(l64).max()):.3e}, g {g:.3e}, bound {bound:.3e} '
          f'(bound / g {bound / g:.1f}), context {ctx:.3e} ({ctx / bound:.0f} x), over steps {vary:.3e} ({vary / bound:.0f} x)')
    assert 8.0 * g <= const and bound == const, f'{name} {mode}: 8 g = {8 * g:.3e} is in force over {const:.3e}: pick another seed'
    assert ctx >= 1000.0 * bound
    assert vary > 100.0 * bound


@pytest.mark.parametrize('name,mode', fc.CASES)
def test_x_init_matters(name, mode):
    """With x[:, 0] = 0 the step-0 outputs of every row move by at least 1000 x the bound.

    On an unscaled 'default' MOL model no x[:, 0] in (-1, 1) does that (the outputs stay below 0.21 and the bound's floor of 1 is in force:
    129 x to 426 x at drawn values, below 1000 x even at |x[:, 0]| = 1 at the reference's loop dims); hence forward_cases.MOL_FC3_SCALE and the
    MOL seed of forward_cases.X_SEEDS."""
    c = fc.inputs(name, mode)
    bound, _ = fc.logit_bound(name, mode)
    l64 = fc.float64_forward(name, mode)[2]
    x0 = c['x'].copy()
    x0[:, 0] = 0.0
    init = float(np.abs(_forward64(name, mode, x=x0)[2][:, 0] - l64[:, 0]).max(axis=1).min())
    print(f'\n[forward padded] {name} {mode}: x_init {init:.3e} ({init / bound:.0f} x the bound {bound:.3e})')
    assert init >= 1000.0 * bound


def _misread(mels, T, pad, edit):
    """The padded mels as `cond_fill` of loop_teamg.hip / loop_teamg_batch.hip would see them under one wrong index (frame f of the result =
    what the kernel would read for tap position f): `+ a.mel_off` dropped, `a.T` for `a.mel_T` in the row stride, `a.T` for `a.mel_T` in the clamp.
    Every index stays inside the (B, F, T + 2 pad) allocation."""
    B, F, mT = mels.shape
    out = np.zeros_like(mels)
    if edit == 'no mel_off':
        out[:, :, pad:] = mels[:, :, :mT - pad]
    elif edit == 'row stride T':
        flat = mels.reshape(-1)
        for b in range(B):
            for j in range(F):
                out[b, j] = flat[b * F * T + j * mT:b * F * T + (j + 1) * mT]
    elif edit == 'clamp T':
        out[:, :, :T] = mels[:, :, :T]
    return out


@pytest.mark.parametrize('edit', ['no mel_off', 'row stride T', 'clamp T'])
@pytest.mark.parametrize('name,mode', [c for c in fc.CASES if c[0] in fc.TEAMG_SETS])
def test_a_wrong_index_in_cond_fill_moves_the_logits(name, mode, edit):
    """The three wrong indices of the two any-dims team kernels, restated on the float64 reference: the upsampled mels from the misread frames, aux
    (MelResNet, another kernel) from the true ones.  Every row the edit touches moves by more than 100 x the bound -- the kernels' own error is
    below 1 x -- so the GPU comparison cannot stay green under any of them; the row stride leaves row 0 alone, which is why the cases have B = 3."""
    import torch
    from oracle import torch_ref
    d, c = fc.dims(name, mode), fc.inputs(name, mode)
    bound, _ = fc.logit_bound(name, mode)
    up64, aux64, l64 = fc.float64_forward(name, mode)
    wrong = _misread(c['mels'], c['T'], d['pad'], edit)
    up_w = fc.conditioning_of(fc.state_dict(name, mode), d, wrong, torch.float64)[0]
    with torch.no_grad():
        t = {k: torch.as_tensor(np.asarray(v)).double() for k, v in fc.state_dict(name, mode).items() if np.asarray(v).dtype.kind == 'f'}
        lw = torch_ref.loop_forward(t, torch.as_tensor(c['x']).double(), torch.as_tensor(up_w), torch.as_tensor(aux64)).numpy()
    move = np.abs(lw - l64).max(axis=(1, 2))                                    # per row
    print(f'\n[forward padded] {name} {mode} cond_fill with {edit}: rows move by {", ".join(f"{v / bound:.0f} x" for v in move)} the bound {bound:.3e}')
    rows = range(fc.B)
    if edit == 'row stride T':
        assert move[0] == 0.0
        rows = range(1, fc.B)
    assert all(move[b] > 100.0 * bound for b in rows)


@pytest.mark.parametrize('T', fc.COND_FRAMES)
@pytest.mark.parametrize('name', list(fc.DIM_SETS))
def test_the_conditioning_bounds_are_the_constants_and_the_context_matters(name, T):
    d = fc.dims(name)
    mels = fc.inputs(name, 'RAW', T)['mels']
    (b_up, g_up), (b_aux, g_aux) = fc.conditioning_bounds(name, T)
    up64, aux64 = fc.float64_conditioning(name, T)
    L, edge = T * d['hop_length'], d['pad'] * d['hop_length']
    assert up64.shape == (fc.B, L, d['feat_dims']) and aux64.shape == (fc.B, L, d['res_out_dims'])
    import torch
    upz, auxz = fc.conditioning_of(fc.state_dict(name, 'RAW'), d, fc.zero_context(mels, d['pad']), torch.float64)
    dup = np.abs(upz - up64).max(axis=2)                                         # (B, L)
    head, tail = float(dup[:, :edge].max(axis=1).min()), float(dup[:, max(L - edge, 0):].max(axis=1).min())
    daux = float(np.abs(auxz - aux64).max(axis=(1, 2)).min())
    print(f'\n[forward padded] {name} conditioning T={T}: g_up {g_up:.3e} (bound {b_up:.3e}), g_aux {g_aux:.3e} (bound {b_aux:.3e}), '
          f'context: up head {head:.3e} tail {tail:.3e} ({min(head, tail) / b_up:.0f} x), aux {daux:.3e} ({daux / b_aux:.0f} x)')
    assert 8.0 * g_up <= 3e-6 and b_up == 3e-6 and 8.0 * g_aux <= 2e-5 and b_aux == 2e-5
    assert head >= 1000.0 * b_up and tail >= 1000.0 * b_up                       # within the first and the last pad frames' worth of positions
    assert daux >= 1000.0 * b_aux


def test_the_sets_reach_what_they_are_for():
    d = fc.DIM_SETS
    assert {n: 2 * d[n]['pad'] + 1 for n in ('Bp1', 'Bp1w', 'B', 'Bp3', 'S3b', 'S5')} == dict(Bp1=3, Bp1w=3, B=5, Bp3=7, S3b=3, S5=7)
    for n, s in d.items():
        assert int(np.prod(s['upsample_factors'])) == s['hop_length'], n
        assert fc.loop_frames(n) * s['hop_length'] <= 825
        # wrnn_create's rule restated: the upsample layers' edge reach against the indent pad * hop
        later, reach = s['hop_length'], 0
        for f in s['upsample_factors']:
            later //= f
            reach += f * later
        assert (reach > s['pad'] * s['hop_length']) == (n in fc.REFUSED), (n, reach)
    assert fc.REFUSED == {'Bp1': 'upsample edge reach 9 exceeds indent 6'}
    assert all((n, 'RAW') in fc.CASES for n in d) and fc.B == 3
    for T in fc.COND_FRAMES:
        c = fc.inputs('Bp3', 'RAW', T)
        assert c['mels'].shape == (3, 13, T + 6) and c['mels'][:, :, :3].all() and c['mels'][:, :, -3:].all()    # the context is real
    for name, mode in fc.CASES:
        c = fc.inputs(name, mode)
        assert (c['x'][:, 0] != 0).all() and np.abs(c['x']).max() <= 1.0
        assert c['x'].shape == c['y'].shape == (3, c['L'])


def test_the_refusals_the_gpu_file_asserts_are_the_librarys():
    """wrnn_teamg_plan_fmt on the host: which (set, rows per team) have no plan, in both modes and all three weight formats; wrnn_create's own
    refusal of Bp1 (it comes before the first device call)."""
    from tacotronv2_wavernn_chinese_amd import _cabi
    for name in fc.TEAMG_SETS:
        for mode in ('RAW', 'MOL'):
            for weights in ('f32', 'f16', 'e4m3'):
                _cabi.teamg_plan_fmt(1, weights, **fc.dims(name, mode), mode=mode)        # one row per team: every set has a plan
                for rows in fc.BATCH_ROWS:
                    if (name, rows) in fc.PLAN_REFUSED:
                        with pytest.raises(_cabi.WrnnError) as e:
                            _cabi.teamg_plan_fmt(rows, weights, **fc.dims(name, mode), mode=mode)
                        assert e.value.code == _cabi.ERR_UNSUPPORTED
                    else:
                        _cabi.teamg_plan_fmt(rows, weights, **fc.dims(name, mode), mode=mode)
    with pytest.raises(_cabi.WrnnError, match=fc.REFUSED['Bp1']) as e:
        _cabi.NativeVocoder(**fc.dims('Bp1'), mode='RAW', device=0)
    assert e.value.code == _cabi.ERR_INVALID


@pytest.mark.parametrize('name,mode', [('B', 'RAW'), ('Bp3', 'MOL')])
def test_the_float64_loss_is_finite(name, mode):
    loss = fc.float64_loss(name, mode)
    print(f'\n[forward padded] {name} {mode}: float64 loss {loss:.6f}')
    assert np.isfinite(loss)
