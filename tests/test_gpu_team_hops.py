"""The XCD-team kernels at hop lengths other than 275.

`wrnn_create` sends a model to TEAM2 / BATCH / BATCH_CS whenever its loop dims are the reference's, pad = 2 and hop <= 275; the upsample
factors and res_blocks are free.  Every other GPU test builds its team-kernel model from DEFAULT_DIMS (hop 275, res_blocks 10), where a
frame change is rare and never lines up with a 64-step conditioning block, a 32-step Philox block, a TEAM2 segment or the stream's
32-step rounding.  Here the same kernels run at

    (4, 8, 8) hop 256   every frame edge on all of those strides at once
    (5, 5, 8) hop 200   a multiple of 8, not of 32
    (2, 3)    hop 6     many frames per 64-step block
    (2,)      hop 2     a frame change every second step
    (1,)      hop 1     a frame change on every step: the hand-off of the per-frame constants c2 / c3 / c4 has no slack

with res_blocks = 3, against the oracle built for the same factors, under the rules of tests/parity_util.py and the tolerances
test_gpu_parity.py applies at hop 275.  The RAW seeds are chosen so that the oracle's own run has NO step with a race margin below
NEAR_TIE (asserted on its output): the comparison leaves out no step and label equality is exact.
"""
import warnings

import numpy as np
import pytest
import torch

from oracle import oracle as orc
from tests.parity_util import (NEAR_TIE, bound_near_ties, check_free_run_raw, check_mol, check_on_gpu_trajectory_raw,
                               check_teacher_forced_raw, parity_report, stream_raw)

pytestmark = pytest.mark.gpu

HOPS = {256: (4, 8, 8), 200: (5, 5, 8), 6: (2, 3), 2: (2,), 1: (1,)}
FRAMES = {256: 6, 200: 6, 6: 40, 2: 64, 1: 64}          # loop tests: at most 1 536 steps
TEAM_KERNELS = ['team2', 'batch', 'batch_cs']

_MODELS, _CASES = {}, {}


def _dims(factors, mode='RAW', **over):
    from tacotronv2_wavernn_chinese_amd.synth import DEFAULT_DIMS
    return dict(DEFAULT_DIMS, upsample_factors=tuple(factors), hop_length=int(np.prod(factors)), res_blocks=3,
                bits=10 if mode == 'RAW' else 9, **over)


def _build(dims, mode, seed=7):
    """(WaveRNN on the GPU, its state_dict, the oracle for the same factors / pad)."""
    from tacotronv2_wavernn_chinese_amd.synth import make_state_dict
    from tacotronv2_wavernn_chinese_amd.vocoder import WaveRNN
    sd = make_state_dict(seed, mode, 'peaky' if mode == 'RAW' else 'default', **dims)
    m = WaveRNN(**dims, mode=mode)
    m.verbose = False
    m.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in sd.items()})
    m.to('cuda:0')
    om = orc.OracleModel(sd, mode=mode, bits=dims['bits'], upsample_factors=dims['upsample_factors'], pad=dims['pad'], fast=True)
    return m, sd, om


def _model(hop, mode='RAW'):
    """One model per (hop, mode) for the whole module: the weights are packed once."""
    key = (hop, mode)
    if key not in _MODELS:
        _MODELS[key] = _build(_dims(HOPS[hop], mode), mode)
    return _MODELS[key]


def _kid(name):
    from tacotronv2_wavernn_chinese_amd import _cabi
    return _cabi.KERNEL_IDS[name]


def _case(hop, mode, B, T):
    """Mels, injected noise and the oracle's free + teacher-forced runs of one (hop, mode, B, T), shared by every kernel."""
    key = (hop, mode, B, T)
    if key in _CASES:
        return _CASES[key]
    from tacotronv2_wavernn_chinese_amd.synth import make_mels
    _, _, om = _model(hop, mode)
    mels = make_mels(3, B, T)
    L = T * hop
    rng = np.random.Generator(np.random.PCG64(8))
    cm, ca = om.conditioning(mels)
    if mode == 'RAW':
        noise = (rng.standard_exponential((L, B, 1024)).astype(np.float32),)
        run = lambda **kw: om.loop(cm, ca, orc.NOISE_EXPO, noise[0], **kw)
    else:
        noise = (rng.uniform(1e-5, 1 - 1e-5, size=(L, B, 10)).astype(np.float32), rng.uniform(1e-5, 1 - 1e-5, size=(L, B)).astype(np.float32))
        run = lambda **kw: om.loop(cm, ca, 0, noise[0], noise[1], **kw)
    free = run()
    forced = run(x_forced=free['samples'], want_logits=True)
    _CASES[key] = dict(mels=mels, noise=noise, free=free, forced=forced, L=L)
    return _CASES[key]


def _noise_kw(c):
    from tacotronv2_wavernn_chinese_amd import _cabi
    kw = dict(noise_mode=_cabi.NOISE_INJECTED, noise1=c['noise'][0])
    if len(c['noise']) > 1:
        kw['noise2'] = c['noise'][1]
    return kw


def _batches(rows, batch_rows):
    """Rows of the batches a batch kernel forms from `rows` rows at `batch_rows` rows per batch (wrnn_sample_opts.batch_rows; more than
    4 rows in a batch = the two-quad instantiation)."""
    return [min(batch_rows, rows - r0) for r0 in range(0, rows, batch_rows)]


def _no_near_tie(ref, what):
    """The condition the seeds were picked for: the oracle's own run has no near-tie, so nothing is excused."""
    assert float(ref['margin'].min()) >= NEAR_TIE, f'{what}: the oracle has a near-tie (margin {float(ref["margin"].min()):.3e}): pick other seeds'


# ---- 1. conditioning -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('hop', list(HOPS))
def test_conditioning_at_every_hop(hop):
    """pad + MelResNet (3 blocks) + upsample network + aux stretch over the WHOLE tensors; T * hop is not a multiple of the 64 positions a
    block of the upsample kernel covers (hop 256 is one for every T: there the odd T leaves an odd number of blocks)."""
    from tacotronv2_wavernn_chinese_amd.synth import make_mels
    m, _, om = _model(hop)
    B, T = 2, 5 if hop >= 200 else 37
    L = T * hop
    assert L % 64 != 0 or hop % 64 == 0
    mels = make_mels(21, B, T)
    cm, ca = om.conditioning(mels)
    assert cm.shape == (B, L, 80) and ca.shape == (B, L, 128)
    up = torch.empty((B, L, 80), device='cuda')
    aux = torch.empty((B, L, 128), device='cuda')
    m.native().conditioning(torch.from_numpy(mels).cuda().data_ptr(), B, T, up.data_ptr(), aux.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    up, aux = up.cpu().numpy(), aux.cpu().numpy()
    np.testing.assert_allclose(up, cm, rtol=0, atol=3e-6)
    np.testing.assert_allclose(aux, ca, rtol=0, atol=2e-5)
    fr = aux.reshape(B, T, hop, 128)
    np.testing.assert_array_equal(fr, np.broadcast_to(fr[:, :, :1], fr.shape))     # nearest-neighbour stretch: constant inside a frame


# ---- 2. every step of every row, RAW ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('kernel', TEAM_KERNELS)
@pytest.mark.parametrize('hop', list(HOPS))
def test_raw_every_step_free_and_teacher_forced(hop, kernel):
    """Free run against the oracle's, then teacher-forced with the fc3 outputs under test_raw_teacher_forced_every_step's logit bound.
    B = 3 on the latency kernel.  B = 5 on the batch kernels, whose default would deal the five rows to five teams, one each: the rows
    per batch are set instead, to 4 (a full quad on one team, a single row on the next) and to 8 (one batch of five rows: the two-quad
    instantiation with a full quad and a partial one), so that every row lane of the frame hand-off runs at every hop."""
    m, _, _ = _model(hop)
    B, T = (3 if kernel == 'team2' else 5), FRAMES[hop]
    shapes = (0,) if kernel == 'team2' else (4, 8)
    if kernel != 'team2':
        assert _batches(B, 4) == [4, 1] and _batches(B, 8) == [5]
    c = _case(hop, 'RAW', B, T)
    free, forced = c['free'], c['forced']
    _no_near_tie(free, f'hop {hop} B={B}')
    np.testing.assert_array_equal(forced['labels'], free['labels'])
    bound = 2e-5 * max(1.0, float(np.abs(forced['logits']).max()))
    err, compared = 0.0, 0
    for batch_rows in shapes:
        kw = dict(kernel=_kid(kernel), batch_rows=batch_rows, **_noise_kw(c))
        res = m.generate_raw(c['mels'], False, 11000, 550, **kw)
        assert m.last_timing['kernel'] == _kid(kernel) and m.last_timing['rows'] == B    # no silent fallback
        got = res['labels'].cpu().numpy().T
        assert got.shape == (T * hop, B)
        first = check_free_run_raw(got, free)
        assert all(f is None for f in first), f'batch_rows={batch_rows}'      # no near-tie in the oracle: the rule excuses nothing
        smp = res['samples'].cpu().numpy().T
        np.testing.assert_array_equal(smp, 2.0 * got.astype(np.float32) / np.float32(m.n_classes - 1.0) - np.float32(1.0))
        res = m.generate_raw(c['mels'], False, 11000, 550, x_forced=free['samples'], want_logits=True, **kw)
        assert m.last_timing['kernel'] == _kid(kernel)
        gotf = res['labels'].cpu().numpy().T
        assert check_teacher_forced_raw(gotf, forced) == 0, f'batch_rows={batch_rows}'
        err = max(err, float(np.abs(res['logits'].cpu().numpy() - forced['logits']).max()))
        compared += got.size + gotf.size
    parity_report(f'team hops: hop {hop} {kernel} RAW B={B} T={T} res_blocks=3, rows per batch {shapes}: steps compared {compared} (free + forced), '
                  f'near-tie divergences 0 (oracle min margin {float(free["margin"].min()):.2e}), max |dlogit| {err:.3e} (bound {bound:.3e})')
    assert err <= bound


# ---- 3. MOL ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('kernel', ['team2', 'batch_cs'])
@pytest.mark.parametrize('hop', [256, 2])
def test_mol_free_and_teacher_forced(hop, kernel):
    """batch_cs: the four rows as ONE batch of four (the default deals them to four teams, one row each)."""
    m, _, _ = _model(hop, 'MOL')
    B, T = 4, FRAMES[hop]
    c = _case(hop, 'MOL', B, T)
    kw = dict(kernel=_kid(kernel), batch_rows=0 if kernel == 'team2' else 4, **_noise_kw(c))
    assert _batches(B, 4) == [4]
    res = m.generate_raw(c['mels'], False, 11000, 550, **kw)
    assert m.last_timing['kernel'] == _kid(kernel) and m.last_timing['rows'] == B
    smp, mix = res['samples'].cpu().numpy().T, res['labels'].cpu().numpy().T
    check_mol(smp, mix, c['free'], teacher_forced=False)
    same = mix == c['free']['labels']
    res = m.generate_raw(c['mels'], False, 11000, 550, x_forced=c['free']['samples'], **kw)
    smpf, mixf = res['samples'].cpu().numpy().T, res['labels'].cpu().numpy().T
    check_mol(smpf, mixf, c['forced'], teacher_forced=True)
    samef = mixf == c['forced']['labels']
    parity_report(f'team hops: hop {hop} {kernel} MOL B={B} T={T}: steps compared {mix.size} free + {mixf.size} forced, mixture-index '
                  f'mismatches {int((~same).sum())} / {int((~samef).sum())}, max |dsample| forced '
                  f'{float(np.abs(smpf - c["forced"]["samples"])[samef].max()):.3e} (tol 2.0e-05)')


# ---- 4. eight rows per team ------------------------------------------------------------------------------------------------------------

def test_batch_cs_two_quads_at_hop_256():
    """B = 40 on 8 teams = 5 rows per batch: the two-quad instantiation, whose shadow wave finishes the second quad's sampler.  Every step
    of all 40 rows, the oracle driven along the GPU's own trajectory in groups of 8 rows."""
    from tacotronv2_wavernn_chinese_amd import _cabi
    from tacotronv2_wavernn_chinese_amd.synth import make_mels
    hop, B, T = 256, 40, 3
    m, _, om = _model(hop)
    L = T * hop
    mels = make_mels(5, B, T)
    q = np.random.Generator(np.random.PCG64(9)).standard_exponential((L, B, 1024), dtype=np.float32)
    n_teams = m.native().team_info()[1]
    assert 5 <= min(8, -(-B // n_teams)) <= 8                              # the library's rows per batch: ceil(rows / teams), at most 8
    res = m.generate_raw(mels, False, 11000, 550, kernel=_cabi.KERNEL_BATCH_CS, noise_mode=_cabi.NOISE_INJECTED, noise1=q)
    assert m.last_timing['kernel'] == _cabi.KERNEL_BATCH_CS and m.last_timing['rows'] == B
    lab, smp = res['labels'].cpu().numpy().T, res['samples'].cpu().numpy().T
    compared, near = 0, []
    for r0 in range(0, B, 8):
        rows = list(range(r0, r0 + 8))
        cm, ca = om.conditioning(mels[rows])
        qg = np.ascontiguousarray(q[:, rows])
        st = check_on_gpu_trajectory_raw(lab[:, rows], smp[:, rows], lambda xf: om.loop(cm, ca, orc.NOISE_EXPO, qg, x_forced=xf))
        compared += st['compared']
        near += [(t, r0 + r, d) for t, r, d in st['near_ties']]
    assert compared == L * B
    bound_near_ties(f'team hops: hop {hop} batch_cs RAW B={B} T={T} (two quads)', compared, near)


# ---- 5. TEAM2 segments -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('hop,segment', [(256, 128), (256, 96), (2, 33)])
def test_team2_segments_on_and_off_frame_edges(hop, segment):
    """A row as a sequence of launches: 128 puts every second segment boundary on a frame edge of hop 256, 96 none but every eighth, 33
    cuts hop 2 inside a frame and inside a 32-step Philox block.  Bit-equal to the single launch, and the oracle's run."""
    from tacotronv2_wavernn_chinese_amd import _cabi
    from tacotronv2_wavernn_chinese_amd.synth import make_mels
    m, _, om = _model(hop)
    B, T = 3, FRAMES[hop]
    c = _case(hop, 'RAW', B, T)
    kw = dict(kernel=_cabi.KERNEL_TEAM2, **_noise_kw(c))
    whole = m.generate_raw(c['mels'], False, 11000, 550, **kw)
    assert m.last_timing['launches'] == 1
    parts = m.generate_raw(c['mels'], False, 11000, 550, team2_segment=segment, **kw)
    assert m.last_timing['kernel'] == _cabi.KERNEL_TEAM2 and m.last_timing['launches'] == -(-c['L'] // segment)
    np.testing.assert_array_equal(parts['labels'].cpu().numpy(), whole['labels'].cpu().numpy())
    np.testing.assert_array_equal(parts['samples'].cpu().numpy(), whole['samples'].cpu().numpy())
    _no_near_tie(c['free'], f'hop {hop} B={B}')
    assert all(f is None for f in check_free_run_raw(parts['labels'].cpu().numpy().T, c['free']))
    # more rows than teams (11 on at most 8): every (row, segment) hands its own state over; device Philox noise, so the block draw
    # resumes behind every boundary
    mels = make_mels(77, 11, T)
    one = m.generate_raw(mels, False, 11000, 550, kernel=_cabi.KERNEL_TEAM2, seed=41)
    seg = m.generate_raw(mels, False, 11000, 550, kernel=_cabi.KERNEL_TEAM2, seed=41, team2_segment=segment)
    assert m.last_timing['launches'] > 1
    np.testing.assert_array_equal(seg['labels'].cpu().numpy(), one['labels'].cpu().numpy())
    greedy = m.generate_raw(mels, False, 11000, 550, kernel=_cabi.KERNEL_TEAM2, noise_mode=_cabi.NOISE_ARGMAX, team2_segment=segment)
    cm, ca = om.conditioning(mels[8:11])                                  # the rows of the second pass
    check_free_run_raw(greedy['labels'].cpu().numpy()[8:11].T, om.loop(cm, ca, orc.NOISE_ARGMAX))


# ---- 6. folds --------------------------------------------------------------------------------------------------------------------------

def _fold_case(target, overlap):
    key = ('fold', target, overlap)
    if key not in _CASES:
        from tacotronv2_wavernn_chinese_amd.synth import make_mels
        _, _, om = _model(256)
        mels = make_mels(13, 1, 30)
        cm, ca = om.conditioning(mels)
        fm, fa = om.fold(cm, target, overlap), om.fold(ca, target, overlap)
        rows, steps = fm.shape[0], target + 2 * overlap
        q = np.random.Generator(np.random.PCG64(14)).standard_exponential((steps, rows, 1024), dtype=np.float32)
        _CASES[key] = dict(mels=mels, q=q, rows=rows, steps=steps, ref=om.loop(fm, fa, orc.NOISE_EXPO, q))
    return _CASES[key]


@pytest.mark.parametrize('kernel', ['team2', 'batch_cs'])
@pytest.mark.parametrize('target,overlap', [(1024, 256), (1000, 100)])
def test_folds_with_a_stride_that_is_and_is_not_a_multiple_of_the_hop(target, overlap, kernel):
    """T = 30 at hop 256 = 7 680 positions.  1024 / 256: the folds start every 1 280 = 5 frames; 1000 / 100: every 1 100, inside a frame.
    Both leave a last fold that runs past the clip's end: the zero record T from there on."""
    from tacotronv2_wavernn_chinese_amd import _cabi
    m, _, _ = _model(256)
    c = _fold_case(target, overlap)
    stride = target + overlap
    assert (stride % 256 == 0) == (target == 1024)
    assert (c['rows'] - 1) * stride + c['steps'] > 30 * 256                # the last fold is padded 'after'
    res = m.generate_raw(c['mels'], True, target, overlap, kernel=_kid(kernel), noise_mode=_cabi.NOISE_INJECTED, noise1=c['q'])
    assert m.last_timing['kernel'] == _kid(kernel)
    got = res['labels'].cpu().numpy().T
    assert got.shape == (c['steps'], c['rows'])
    _no_near_tie(c['ref'], f'hop 256 folds {target}/{overlap}')
    first = check_free_run_raw(got, c['ref'])
    assert all(f is None for f in first)                                  # every step of every fold compared, none excused
    parity_report(f'team hops: hop 256 {kernel} RAW folds {target}/{overlap} ({c["rows"]} rows x {c["steps"]}): steps compared {got.size}, '
                  f'near-tie divergences 0 (oracle min margin {float(c["ref"]["margin"].min()):.2e})')


def test_folded_generate_end_to_end_at_hop_256(tmp_path):
    """generate(batched=True) end to end: the float64 wave against the oracle's epilogue on the oracle's own samples under
    test_device_epilogue_matches_numpy_float64's rule (4 ulp of 1.0, at most 1 % of the samples different at all), its length, and the
    20-hop fade.

    The same call with epilogue='device' is held to the 4 ulp as well, and in place of the 1 % count to something stricter: it must be
    BIT-equal to NumPy's unfold / trim / fade on the library's own mu-law table (wrnn_epilogue_tables), and that table within one ulp of
    pow() of NumPy's decode_mu_law at every label (checked here, the count of differing labels reported), so only pow() can differ from the
    oracle.  The count says nothing about the hop: std::pow and NumPy's pow may disagree in the last bit for some labels whatever the
    hop (55 of 1024 when this was written), and how many samples carry such a label is a property of the weights (193 of 7 424)."""
    from tacotronv2_wavernn_chinese_amd import _cabi
    hop, T, target, overlap = 256, 30, 1024, 256
    eps4 = 4 * np.finfo(np.float64).eps
    m, _, _ = _model(hop)
    c = _fold_case(target, overlap)
    _no_near_tie(c['ref'], 'hop 256 folds 1024/256')
    kw = dict(kernel=_cabi.KERNEL_BATCH_CS, noise_mode=_cabi.NOISE_INJECTED, noise1=c['q'])
    wave_len = (T - 1) * hop
    smp = np.ascontiguousarray(c['ref']['samples'].T)
    want = orc.epilogue(smp, m.n_classes, True, True, target, overlap, wave_len, hop)
    unfaded = orc.xfade_and_unfold(orc.decode_mu_law(smp.astype(np.float64), m.n_classes), target, overlap)[:wave_len]
    assert np.abs(unfaded[-20 * hop - 1:-20 * hop + 1]).min() > 0.0        # a scaled sample would show
    dec, _, _, _ = _cabi.epilogue_tables(m.n_classes, overlap, hop)
    fed = (np.float32(2.0) * np.arange(m.n_classes, dtype=np.float32) / np.float32(m.n_classes - 1.0) - np.float32(1.0)).astype(np.float64)
    dec_np = orc.decode_mu_law(fed, m.n_classes)
    # dec = sign / mu * (p - 1), p = pow(1 + mu, |y|) >= 1: p - 1 is exact, so one ulp of p arrives as ulp(p) / mu, plus half an ulp of
    # the result for the product's rounding on either side
    mu = m.n_classes - 1.0
    assert (np.abs(dec - dec_np) <= np.spacing((1.0 + mu) ** np.abs(fed)) / mu + np.spacing(np.abs(dec_np))).all()
    parity_report(f'team hops: mu-law table against NumPy: {int(np.count_nonzero(dec != dec_np))} of {m.n_classes} labels differ, '
                  f'each by one ulp of pow() at most')
    want_tab = orc.xfade_and_unfold(dec[c['ref']['labels'].T], target, overlap)[:wave_len]
    want_tab[-20 * hop:] *= np.linspace(1, 0, 20 * hop)
    for epilogue in ('host', 'device'):
        wav = m.generate(c['mels'], tmp_path / 'fold.wav', True, target, overlap, True, epilogue=epilogue, **kw)
        assert m.last_timing['kernel'] == _cabi.KERNEL_BATCH_CS
        assert wav.dtype == np.float64 and wav.shape == (wave_len,)
        np.testing.assert_allclose(wav, want, rtol=0, atol=eps4)
        if epilogue == 'host':
            assert np.count_nonzero(wav != want) <= wav.size // 100       # pow() rounding only, if at all
        else:
            np.testing.assert_array_equal(wav, want_tab)
        assert wav[-1] == 0.0
        assert abs(wav[-20 * hop] - unfaded[-20 * hop]) <= eps4            # the fade starts at weight 1 ...
        assert abs(wav[-20 * hop - 1] - unfaded[-20 * hop - 1]) <= eps4    # ... behind an untouched sample
        parity_report(f'team hops: hop 256 folded generate 1024/256, epilogue {epilogue}: {wave_len} samples, max |d| vs the oracle '
                      f'{float(np.abs(wav - want).max()):.3e} (bound {eps4:.3e}), samples different at all {int(np.count_nonzero(wav != want))}')


# ---- 7. ragged batch -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('kernel', ['team2', 'batch_cs'])
def test_ragged_batch_at_hop_200(kernel):
    """Clips of 21, 22 and 25 frames in one call (steps = frames[b] * hop): every row's valid part is the solo call's, bit for bit, and
    nothing is written behind it (the output rows are handed over zeroed)."""
    from tacotronv2_wavernn_chinese_amd import _cabi
    from tacotronv2_wavernn_chinese_amd.synth import make_mels
    hop, lens = 200, [21, 22, 25]
    m, _, om = _model(hop)
    mels = np.zeros((3, 80, 25), np.float32)
    for i, t in enumerate(lens):
        mels[i, :, :t] = make_mels(500 + i, 1, t)[0]
    kw = dict(kernel=_kid(kernel), noise_mode=_cabi.NOISE_ARGMAX)
    # batch_cs: the three clips as ONE batch of mixed lengths (the default deals them to three teams, one row each)
    assert _batches(3, 4) == [3]
    rag = m.generate_raw(mels, False, 11000, 550, frames=np.asarray(lens, np.int32), batch_rows=0 if kernel == 'team2' else 4, **kw)
    assert m.last_timing['kernel'] == _kid(kernel) and m.last_timing['rows'] == 3
    lr, sr = rag['labels'].cpu().numpy(), rag['samples'].cpu().numpy()
    assert lr.shape == (3, 25 * hop)
    for i, t in enumerate(lens):
        solo = m.generate_raw(mels[i:i + 1, :, :t], False, 11000, 550, **kw)
        np.testing.assert_array_equal(lr[i, :t * hop], solo['labels'].cpu().numpy()[0], err_msg=f'row {i} (T={t})')
        np.testing.assert_array_equal(sr[i, :t * hop], solo['samples'].cpu().numpy()[0], err_msg=f'row {i} (T={t})')
        assert not lr[i, t * hop:].any() and not sr[i, t * hop:].any(), f'row {i}: written past its own length'
    if ('ragged', 0) not in _CASES:
        cm, ca = om.conditioning(mels[:1, :, :lens[0]])
        _CASES[('ragged', 0)] = om.loop(cm, ca, orc.NOISE_ARGMAX)
    check_free_run_raw(lr[:1, :lens[0] * hop].T, _CASES[('ragged', 0)])


# ---- 8. streaming ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('hop,mode', [(256, 'RAW'), (2, 'RAW'), (256, 'MOL')])
def test_stream_is_bit_exact_against_offline(hop, mode):
    """24 frames pushed as [1, 2, 3, 5, 13] and one by one, device Philox noise: labels and samples of the offline unbatched call.  At hop
    256 every count of ready steps is a frame edge and a multiple of the 32-step rounding."""
    from tacotronv2_wavernn_chinese_amd import _cabi
    from tacotronv2_wavernn_chinese_amd.synth import make_mels
    m, _, _ = _model(hop, mode)
    T, seed = 24, 1234567
    mels = make_mels(31, 1, T)
    off = m.generate_raw(mels, False, 11000, 550, noise_mode='philox', seed=seed, kernel=_cabi.KERNEL_TEAM2)
    assert m.last_timing['kernel'] == _cabi.KERNEL_TEAM2
    ol, os_ = off['labels'].cpu().numpy(), off['samples'].cpu().numpy()
    assert ol.shape == (1, T * hop)
    for sizes in ([1, 2, 3, 5, 13], [1] * T):
        lab, smp = stream_raw(m, mels, sizes, seed=seed, kernel='team2')
        np.testing.assert_array_equal(lab, ol, err_msg=f'labels, pushes {sizes}')
        np.testing.assert_array_equal(smp, os_, err_msg=f'samples, pushes {sizes}')


def test_argmax_stream_at_hop_256_equals_offline_and_the_oracle():
    from tacotronv2_wavernn_chinese_amd import _cabi
    from tacotronv2_wavernn_chinese_amd.synth import make_mels
    m, _, om = _model(256)
    mels = make_mels(32, 1, 24)
    off = m.generate_raw(mels, False, 11000, 550, noise_mode=_cabi.NOISE_ARGMAX, kernel=_cabi.KERNEL_TEAM2)
    lab, smp = stream_raw(m, mels, [3, 0, 5, 1, 7, 8], noise_mode='argmax', kernel='team2')
    np.testing.assert_array_equal(lab, off['labels'].cpu().numpy())
    np.testing.assert_array_equal(smp, off['samples'].cpu().numpy())
    cm, ca = om.conditioning(mels)
    check_free_run_raw(lab.T, om.loop(cm, ca, orc.NOISE_ARGMAX))


# ---- 9. the edge of eligibility --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('what', ['hop276', 'pad3'])
def test_just_outside_the_team_kernels_falls_back_loudly(what):
    """hop 276 = (4, 69) and pad = 3 (a 7-frame upsampling support) pass wrnn_create but not loop_team_obstacle: AUTO runs the any-shape
    kernel with the RuntimeWarning that carries the library's reason, an explicit team kernel is refused, the labels are the oracle's."""
    from tacotronv2_wavernn_chinese_amd import _cabi
    from tacotronv2_wavernn_chinese_amd.synth import make_mels
    dims = _dims((4, 69)) if what == 'hop276' else _dims((5, 5, 11), pad=3)
    m, _, om = _build(dims, 'RAW')
    hop, B, T = dims['hop_length'], 2, 4
    ok, _, why = m.native().team_info()
    assert not ok and 'pad=2' in why and 'hop <= 275' in why
    mels = make_mels(3, B, T)
    q = np.random.Generator(np.random.PCG64(8)).standard_exponential((T * hop, B, 1024), dtype=np.float32)
    with pytest.warns(RuntimeWarning, match='hop <= 275'):
        res = m.generate_raw(mels, False, 11000, 550, noise_mode=_cabi.NOISE_INJECTED, noise1=q)
    assert m.last_timing['kernel'] == _cabi.KERNEL_SIMPLE
    cm, ca = om.conditioning(mels)
    got = res['labels'].cpu().numpy().T
    assert got.shape == (T * hop, B)
    check_free_run_raw(got, om.loop(cm, ca, orc.NOISE_EXPO, q))
    for k in (_cabi.KERNEL_TEAM2, _cabi.KERNEL_BATCH, _cabi.KERNEL_BATCH_CS):
        with pytest.raises(_cabi.WrnnError):
            m.generate_raw(mels, False, 11000, 550, noise_mode=_cabi.NOISE_ARGMAX, kernel=k)


def test_hop_275_with_three_res_blocks_stays_on_a_team_kernel():
    from tacotronv2_wavernn_chinese_amd import _cabi
    from tacotronv2_wavernn_chinese_amd.synth import make_mels
    m, _, om = _build(_dims((5, 5, 11)), 'RAW')
    ok, _, why = m.native().team_info()
    assert ok and why == ''
    mels = make_mels(3, 2, 4)
    with warnings.catch_warnings():
        warnings.simplefilter('error', RuntimeWarning)                     # no slow-path warning
        res = m.generate_raw(mels, False, 11000, 550, noise_mode=_cabi.NOISE_ARGMAX)
    assert m.last_timing['kernel'] in (_cabi.KERNEL_TEAM2, _cabi.KERNEL_BATCH, _cabi.KERNEL_BATCH_CS)
    cm, ca = om.conditioning(mels)
    check_free_run_raw(res['labels'].cpu().numpy().T, om.loop(cm, ca, orc.NOISE_ARGMAX))
