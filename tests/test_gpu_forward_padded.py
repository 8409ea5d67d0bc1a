"""The teacher-forced forward pass and pre-padded mels on every loop kernel, against the float64 reference of tests/forward_cases.py.

`WaveRNN.forward(x, mels)` in eval() runs the loop kernels with mels that carry `pad` real context frames on each side (`mels_padded`:
mel_T = T + 2 pad, mel_off = pad), `x_init` and `x_forced` + logits.  Every (B, L, n_classes) output is compared with
torch_ref.upsample(training=False) + torch_ref.loop_forward in float64 within `forward_cases.logit_bound`; what that bound rests on is asserted
on the CPU by tests/test_forward_cases_host.py (8 g is nowhere in force; zeroed context frames move the outputs by 10 690 x the bound or more, a
zeroed x[:, 0] by 1117 x or more).  One model per (dim set, mode, weight format, state dict) for the whole module: the weights are packed once.

Which test catches which wrong index (reasoned from the code; the shapes keep every such index inside the allocation):

  `+ a.mel_off` dropped in cond_fill (loop_teamg.hip / loop_teamg_batch.hip)   every frame read `pad` frames early: test_forward_matches_float64
      [*-teamg], test_teamg_batch_matches_float64, test_weight_images (the float64 half), test_loss_on_top; in materialize_kernel / resnet_kernel
      (prologue.hip): test_padded_conditioning (up / aux), and every forward test through aux
  `a.T` for `a.mel_T` in the row stride `mel_b = a.mels + utt * F * a.mel_T`        rows 1 and 2 read another row's frames (row 0 is unchanged, hence
      B = 3): the same tests; `j * a.T` for `j * a.mel_T` inside a row: the same tests, from feature 1 on
  `a.T` for `a.mel_T` in the clamp `fr < a.mel_T`                                 the last 2 pad frames read as zero, i.e. the trailing context is
      lost: the same tests at the steps of the last `pad` frames (host file: `tail`, 80 948 x the bound or more)
  `x_init` ignored                                                                step 0 of every row: every forward test (1117 x the bound or more)
  a padded call with `batched` or `frames_dev` that shifts or drops the offset       test_zero_context_is_the_unpadded_call[*-batched / *-ragged]

Today's suite stays green under the TEAMG edits: it runs those two kernels with mel_off = 0 and mel_T = T only.
"""
import numpy as np
import pytest
import torch

from tests import forward_cases as fc
from tests.parity_util import parity_report

pytestmark = pytest.mark.gpu

TEAM_KERNELS = ('team2', 'batch', 'batch_cs')
TEAM_SETS = ('H256', 'H6', 'H1', 'D')
TEAMG_SETS, BATCH_ROWS = fc.TEAMG_SETS, fc.BATCH_ROWS
SIMPLE_SETS = ('S1', 'S3b', 'S5', 'Bp1w', 'Bp3')
PLAN_REFUSED = fc.PLAN_REFUSED                                              # the plan's refusals: asserted with their reason, never skipped
PLAN_REASON = 'rows per team exceed'
MATRICES = ('I.weight', 'rnn1.weight_ih_l0', 'rnn1.weight_hh_l0', 'rnn2.weight_ih_l0', 'rnn2.weight_hh_l0', 'fc1.weight', 'fc2.weight', 'fc3.weight')
FOLD_TARGET, FOLD_OVERLAP = 50, 7
FOLD_FRAMES = {275: 2, 256: 2, 128: 2, 12: 17, 6: 33}      # by hop: one clip of at least 3 folds

_MODELS, _STATE, _RUNS, _REF = {}, {}, {}, {}


def _modes(name):
    return ('RAW', 'MOL') if name in fc.MOL_SETS else ('RAW',)


FORWARD = ([(n, m, k) for k in TEAM_KERNELS for n in TEAM_SETS for m in _modes(n)] + [(n, m, 'teamg') for n in TEAMG_SETS for m in _modes(n)]
           + [(n, m, 'simple') for n in SIMPLE_SETS for m in _modes(n)])
TEAMG_BATCH = [(n, m, r) for n in TEAMG_SETS for m in _modes(n) for r in BATCH_ROWS]


def _kid(kernel):
    from tacotronv2_wavernn_chinese_amd import _cabi
    return _cabi.KERNEL_IDS[kernel]


def _state(name, mode, variant='sd'):
    """The state dict of a case; 'sd16' / 'sd8': the matrices of the TEAMG weight image rounded to fp16 (the `_round_f16` recipe of
    tests/test_gpu_teamg_f16.py: column 0 of I.weight stays) / dequantised from e4m3 (tests/teamg_e4m3_ref.quantise)."""
    key = (name, mode, variant)
    if key not in _STATE:
        sd = fc.state_dict(name, mode)
        if variant == 'sd16':
            out = {k: np.array(v) for k, v in sd.items()}
            for k in MATRICES:
                r = torch.from_numpy(np.ascontiguousarray(out[k])).half().float().numpy()
                if k == 'I.weight':
                    r[:, 0] = out[k][:, 0]
                out[k] = r
            sd = out
        elif variant == 'sd8':
            from tests import teamg_e4m3_ref
            sd = teamg_e4m3_ref.quantise(sd)[0]
        _STATE[key] = sd
    return _STATE[key]


def _model(name, mode='RAW', weights='f32', variant='sd'):
    key = (name, mode, weights, variant)
    if key not in _MODELS:
        from tacotronv2_wavernn_chinese_amd.vocoder import WaveRNN
        m = WaveRNN(**fc.dims(name, mode), mode=mode)
        m.verbose = False
        m.teamg_weights = weights
        m.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in _state(name, mode, variant).items()})
        m.to('cuda:0')
        m.eval()
        _MODELS[key] = m
    return _MODELS[key]


def _forced(m, name, mode, kernel, batch_rows=0):
    """The call WaveRNN.forward makes (pre-padded mels, step 0 fed x[:, 0], every later step forced, the sampler's result ignored), with the
    kernel and batch_rows named: dict(logits (B, L, n_classes), labels (B, L), samples (B, L)) as numpy."""
    from tacotronv2_wavernn_chinese_amd import _cabi
    c = fc.inputs(name, mode)
    x_forced = np.zeros((c['L'], fc.B), np.float32)
    x_forced[:-1] = c['x'][:, 1:].T
    kw = dict(noise_mode=_cabi.NOISE_ARGMAX) if mode == 'RAW' else dict(noise_mode=_cabi.NOISE_PHILOX, seed=0)
    res = m.generate_raw(c['mels'], False, 11000, 550, x_forced=x_forced, x_init=c['x'][:, 0], want_logits=True, mels_padded=True, kernel=kernel,
                         batch_rows=batch_rows, **kw)
    assert m.last_timing['kernel'] == _kid(kernel) and m.last_timing['rows'] == fc.B and m.last_timing['steps'] == c['L']
    assert kernel != 'teamg_batch' or m.last_timing['batch_rows'] == batch_rows  # the instantiation asked for, no other
    return dict(logits=res['logits'].permute(1, 0, 2).cpu().numpy(), labels=res['labels'].cpu().numpy(), samples=res['samples'].cpu().numpy())


def _run(name, mode, kernel, batch_rows=0):
    key = (name, mode, kernel, batch_rows)
    if key not in _RUNS:
        _RUNS[key] = _forced(_model(name, mode), name, mode, kernel, batch_rows)
    return _RUNS[key]


def _within(what, got, l64, bound, g):
    assert got.shape == l64.shape and got.dtype == np.float32 and np.isfinite(got).all(), what
    err = float(np.abs(got.astype(np.float64) - l64).max())
    parity_report(f'[forward padded] {what}: max |kernel - float64| {err:.3e}, bound {bound:.3e}, g {g:.3e}, error / bound {err / bound:.3f}, '
                  f'error / g {err / g:.2f}')
    assert err <= bound, f'{what}: {err:.3e} > {bound:.3e}'


def _refused_plan(m, name, mode, rows, weights='f32'):
    """The host plan refuses (set, rows) and so does the call, with the plan's reason."""
    from tacotronv2_wavernn_chinese_amd import _cabi
    with pytest.raises(_cabi.WrnnError) as e:
        _cabi.teamg_plan_fmt(rows, weights, **fc.dims(name, mode), mode=mode)
    assert e.value.code == _cabi.ERR_UNSUPPORTED
    with pytest.raises(_cabi.WrnnError, match=PLAN_REASON) as e:
        _forced(m, name, mode, 'teamg_batch', rows)
    assert e.value.code == _cabi.ERR_UNSUPPORTED


# ---- 1. padded conditioning, whole tensors ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('T', fc.COND_FRAMES)
@pytest.mark.parametrize('name', [n for n in fc.DIM_SETS if n not in fc.REFUSED])
def test_padded_conditioning(name, T):
    """wrnn_conditioning(mels_padded=1) against up64 / aux64 over all positions; aux is constant inside a frame; with up or aux NULL the other
    output has the same bits."""
    m = _model(name)
    nat, d = m.native(), fc.dims(name)
    hop, F, R = d['hop_length'], d['feat_dims'], d['res_out_dims']
    L = T * hop
    mels = torch.from_numpy(fc.inputs(name, 'RAW', T)['mels']).cuda()
    assert tuple(mels.shape) == (fc.B, F, T + 2 * d['pad'])
    st = torch.cuda.current_stream().cuda_stream

    def call(want_up, want_aux):
        up = torch.full((fc.B, L, F), float('nan'), device='cuda')
        aux = torch.full((fc.B, L, R), float('nan'), device='cuda')
        nat.conditioning(mels.data_ptr(), fc.B, T, up.data_ptr() if want_up else 0, aux.data_ptr() if want_aux else 0, st, mels_padded=True)
        torch.cuda.synchronize()
        return up.cpu().numpy(), aux.cpu().numpy()
    up, aux = call(True, True)
    up64, aux64 = fc.float64_conditioning(name, T)
    (b_up, g_up), (b_aux, g_aux) = fc.conditioning_bounds(name, T)
    assert np.isfinite(up).all() and np.isfinite(aux).all()
    e_up, e_aux = float(np.abs(up - up64).max()), float(np.abs(aux - aux64).max())
    parity_report(f'[forward padded] {name} conditioning T={T}: up max |kernel - float64| {e_up:.3e}, bound {b_up:.3e}, g {g_up:.3e}, error / bound '
                  f'{e_up / b_up:.3f}; aux {e_aux:.3e}, bound {b_aux:.3e}, g {g_aux:.3e}, error / bound {e_aux / b_aux:.3f}')
    assert e_up <= b_up and e_aux <= b_aux
    fr = aux.reshape(fc.B, T, hop, R)
    np.testing.assert_array_equal(fr, np.broadcast_to(fr[:, :, :1], fr.shape))
    up_only, no_aux = call(True, False)
    no_up, aux_only = call(False, True)
    np.testing.assert_array_equal(up_only, up)
    np.testing.assert_array_equal(aux_only, aux)
    assert np.isnan(no_aux).all() and np.isnan(no_up).all()                     # nothing was written through the NULL side's buffer


def test_the_refused_set_is_refused_with_its_reason():
    """Bp1: pad 1 under the factors (2, 3).  The upsample layers reach 9 samples past an edge, the crop removes 6: the 3-tap form the kernels
    evaluate is not what the reference computes there, and wrnn_create says so -- on every path, forward() included."""
    from tacotronv2_wavernn_chinese_amd import _cabi
    from tacotronv2_wavernn_chinese_amd.vocoder import WaveRNN
    m = WaveRNN(**fc.dims('Bp1'), mode='RAW')
    m.verbose = False
    m.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in fc.state_dict('Bp1', 'RAW').items()})
    m.to('cuda:0')
    m.eval()
    c = fc.inputs('Bp1', 'RAW')
    for kernel in ('teamg', 'teamg_batch', 'simple'):
        m.kernel = _kid(kernel)
        with pytest.raises(_cabi.WrnnError, match=fc.REFUSED['Bp1']) as e:
            m.forward(c['x'], c['mels'])
        assert e.value.code == _cabi.ERR_INVALID


# ---- 2. forward() against float64, every step, every kernel that admits the dims ------------------------------------------------------------

@pytest.mark.parametrize('name,mode,kernel', FORWARD)
def test_forward_matches_float64(name, mode, kernel):
    from tacotronv2_wavernn_chinese_amd import _cabi
    m = _model(name, mode)
    c = fc.inputs(name, mode)
    m.kernel = _kid(kernel)
    try:
        assert not m.training
        y_hat = m.forward(c['x'], c['mels'])
    finally:
        m.kernel = _cabi.KERNEL_AUTO
    assert m.last_timing['kernel'] == _kid(kernel)                              # no other kernel in its place
    assert tuple(y_hat.shape) == (fc.B, c['L'], fc.n_classes(name, mode)) and y_hat.is_cuda
    bound, g = fc.logit_bound(name, mode)
    _within(f'{name} {mode} {kernel} f32 forward()', y_hat.cpu().numpy(), fc.float64_forward(name, mode)[2], bound, g)


@pytest.mark.parametrize('name,mode,batch_rows', TEAMG_BATCH)
def test_teamg_batch_matches_float64(name, mode, batch_rows):
    m = _model(name, mode)
    if (name, batch_rows) in PLAN_REFUSED:
        _refused_plan(m, name, mode, batch_rows)
        return
    got = _run(name, mode, 'teamg_batch', batch_rows)
    bound, g = fc.logit_bound(name, mode)
    _within(f'{name} {mode} teamg_batch rows {batch_rows} f32', got['logits'], fc.float64_forward(name, mode)[2], bound, g)


# ---- 3. weight images -------------------------------------------------------------------------------------------------------------------------

def _image_reference(name, variant):
    """(logits64, bound, g) of the RAW case on the rounded / dequantised state dict: that model's own float64 reference and bound."""
    key = (name, variant)
    if key not in _REF:
        c, d, sd = fc.inputs(name, 'RAW'), fc.dims(name), _state(name, 'RAW', variant)
        l64 = fc.forward_of(sd, d, c['mels'], c['x'], torch.float64)[2]
        l32 = fc.forward_of(sd, d, c['mels'], c['x'], torch.float32)[2]
        g = float(np.abs(l32.astype(np.float64) - l64).max())
        _REF[key] = (l64, fc.bound_of(l64, g), g)
    return _REF[key]


@pytest.mark.parametrize('fmt', ['f16', 'e4m3'])
@pytest.mark.parametrize('name,kernel,batch_rows', [('C', 'teamg', 0), ('C', 'teamg_batch', 4), ('C', 'teamg_batch', 2), ('Bp3', 'teamg', 0), ('Bp3', 'teamg_batch', 4)])
def test_weight_images(name, kernel, batch_rows, fmt):
    """The f16 / e4m3 image on `sd` under mels_padded: bit-equal to the fp32 image on the rounded / dequantised model, and within that model's
    own bound of its float64 logits.  C at 4 rows per team is refused by the plan in every format (asserted); C runs at 2."""
    variant = {'f16': 'sd16', 'e4m3': 'sd8'}[fmt]
    m_img, m_ref = _model(name, 'RAW', fmt, 'sd'), _model(name, 'RAW', 'f32', variant)
    if (name, batch_rows) in PLAN_REFUSED:
        _refused_plan(m_img, name, 'RAW', batch_rows, fmt)
        return
    got = _forced(m_img, name, 'RAW', kernel, batch_rows)
    assert m_img.last_timing['teamg_weights'] == fmt and (kernel == 'teamg' or m_img.last_timing['batch_rows'] == batch_rows)
    ref = _forced(m_ref, name, 'RAW', kernel, batch_rows)
    assert m_ref.last_timing['teamg_weights'] == 'f32'
    for k in ('logits', 'labels', 'samples'):
        np.testing.assert_array_equal(got[k], ref[k], err_msg=f'{name} {kernel} {fmt}: {k}')
    l64, bound, g = _image_reference(name, variant)
    _within(f'{name} RAW {kernel}{f" rows {batch_rows}" if batch_rows else ""} {fmt}', got['logits'], l64, bound, g)
    assert np.abs(l64 - fc.float64_forward(name, 'RAW')[2]).max() > bound        # the rounded model is another model: its own reference was needed


# ---- 4. row equality ----------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('name,mode,batch_rows', [c for c in TEAMG_BATCH if (c[0], c[2]) not in PLAN_REFUSED])
def test_teamg_batch_rows_are_bit_equal_to_teamg(name, mode, batch_rows):
    """What README.md states for unpadded calls, under mels_padded: logits, labels and samples of every row, whatever batch it lands in."""
    ref, got = _run(name, mode, 'teamg'), _run(name, mode, 'teamg_batch', batch_rows)
    for k in ('logits', 'labels', 'samples'):
        np.testing.assert_array_equal(got[k], ref[k], err_msg=f'{name} {mode} batch_rows {batch_rows}: {k}')


# ---- 5. zero context is the unpadded call ----------------------------------------------------------------------------------------------------------

ZERO_CONTEXT = ([(n, k, 0) for n in ('H256', 'D') for k in TEAM_KERNELS] + [(n, k, r) for n in ('A', 'Bp3') for k, r in (('teamg', 0), ('teamg_batch', 2))]
                + [('S5', 'simple', 0)])


@pytest.mark.parametrize('form', ['unbatched', 'batched', 'ragged'])
@pytest.mark.parametrize('name,kernel,batch_rows', ZERO_CONTEXT)
def test_zero_context_is_the_unpadded_call(name, kernel, batch_rows, form):
    """generate_raw(np.pad(mels, P zero frames each side), mels_padded=True) has the bits of generate_raw(mels): labels, samples and logits, under
    injected noise, free-running and teacher-forced with x_init.  `batched` (one clip, folds 50 / 7 that start inside a frame) and `frames=`
    (lengths (T, 1, ceil(T / 2)), zeros beyond each clip) take the same offset: wrnn_generate refuses neither, and this is what they compute."""
    from tacotronv2_wavernn_chinese_amd import _cabi
    from tacotronv2_wavernn_chinese_amd.synth import make_mels
    m = _model(name)
    d = fc.dims(name)
    P, hop, NC = d['pad'], d['hop_length'], fc.n_classes(name, 'RAW')
    batched = form == 'batched'
    B, T = (1, FOLD_FRAMES[hop]) if batched else (fc.B, fc.loop_frames(name))
    mels = make_mels(11, B, T, feat_dims=d['feat_dims'])
    frames = None
    if form == 'ragged':
        frames = np.asarray([T, 1, -(-T // 2)], np.int32)
        for b, t in enumerate(frames):
            mels[b, :, t:] = 0.0
    padded = np.pad(mels, ((0, 0), (0, 0), (P, P)))
    rows, steps = m.native().plan(B, T, batched, FOLD_TARGET, FOLD_OVERLAP)
    if batched:
        assert rows >= 3 and (FOLD_TARGET + FOLD_OVERLAP) % hop != 0 and (rows - 1) * (FOLD_TARGET + FOLD_OVERLAP) + steps > T * hop
    else:
        assert (rows, steps) == (B, T * hop)
    lens = [steps] * rows if frames is None else [int(t) * hop for t in frames]
    rng = np.random.Generator(np.random.PCG64(8))
    noise = rng.standard_exponential((steps, rows, NC), dtype=np.float32)
    x_init = np.asarray([0.5, -0.25, 1.0, -1.0, 0.125, -0.75, 0.25, 0.75, -0.5, 0.375, -0.125, 0.625][:rows], np.float32)
    assert x_init.shape == (rows,)

    def gen(mel, **kw):
        res = m.generate_raw(mel, batched, FOLD_TARGET, FOLD_OVERLAP, kernel=kernel, batch_rows=batch_rows, noise_mode=_cabi.NOISE_INJECTED, noise1=noise,
                             want_logits=True, frames=frames, **kw)
        assert m.last_timing['kernel'] == _kid(kernel) and m.last_timing['rows'] == rows and m.last_timing['steps'] == steps
        return res['labels'].cpu().numpy(), res['samples'].cpu().numpy(), res['logits'].cpu().numpy()

    def same(a, b, what):
        np.testing.assert_array_equal(a[0], b[0], err_msg=f'{what}: labels')
        np.testing.assert_array_equal(a[1], b[1], err_msg=f'{what}: samples')
        for r, n in enumerate(lens):                                            # a ragged row's logits past its own length are never written
            np.testing.assert_array_equal(a[2][:n, r], b[2][:n, r], err_msg=f'{what}: logits of row {r}')
    free = gen(mels)
    same(gen(padded, mels_padded=True), free, f'{name} {kernel} {form} free-running')
    assert all(np.unique(free[0][r, :n]).size > 1 for r, n in enumerate(lens))  # the run is not degenerate
    xf = np.ascontiguousarray(free[1].T)
    forced = gen(mels, x_forced=xf, x_init=x_init)
    same(gen(padded, mels_padded=True, x_forced=xf, x_init=x_init), forced, f'{name} {kernel} {form} teacher-forced')
    assert not np.array_equal(forced[2][0], free[2][0])                         # x_init reached step 0


# ---- 6. the loss on top ----------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('name,mode', [('B', 'RAW'), ('Bp3', 'MOL')])
def test_loss_on_top(name, mode):
    """voc_loss on forward()'s logits against torch_ref.loss_of on logits64, in float64: the tolerance of tests/test_forward_loss.py."""
    from tacotronv2_wavernn_chinese_amd import _cabi
    from tacotronv2_wavernn_chinese_amd.losses import voc_loss
    m = _model(name, mode)
    c = fc.inputs(name, mode)
    m.kernel = _kid('teamg')
    try:
        y_hat = m.forward(c['x'], c['mels'])
    finally:
        m.kernel = _cabi.KERNEL_AUTO
    assert m.last_timing['kernel'] == _kid('teamg')
    got, want = float(voc_loss(m, y_hat, c['y']).item()), fc.float64_loss(name, mode)
    parity_report(f'[forward padded] {name} {mode} teamg loss: kernel {got:.8f}, float64 {want:.8f}, |difference| {abs(got - want):.3e}, '
                  f'bound {2e-5 * max(1.0, abs(want)):.3e}')
    assert abs(got - want) <= 2e-5 * max(1.0, abs(want)), (got, want)
