"""Parity at the BASELINE.json config sizes, through the C-ABI, on the shipped kernels with default settings.

configs[1]: B=1, mel 80x401 (110 275 free-running steps = 14 default segments of the latency kernel), RAW 10-bit;
configs[2]: B=64 utterances (batch kernel, 8 rows per XCD team in lock-step), sampled with the production Philox noise: all 64
            rows at T=41 and 8 rows at the full T=401;
configs[4]: MOL 9-bit, B=32 (batch kernel, 4 rows per team), injected uniforms: all 32 rows at T=41, 4 rows at T=401;
configs[3]: tests/test_gpu_config3.py (the scatter -> generate -> device epilogue -> gather pipeline of bench.py).
Oracle = the C restatement pinned to the reference (tests/test_oracle_golden.py); the configs[1] clip is additionally
compared with labels minted from the unmodified reference itself (tests/golden/raw_peaky_b1_t401.npz).

The north star's contract is "within +-1 LSB at 10-bit".  Every test here drives the oracle along the GPU's own trajectory
(tests/parity_util.py: check_on_gpu_trajectory_*), so EVERY step of every checked row is compared -- `compared == L * rows` is
asserted -- under the per-step rule: label identical, or a near-tie of the sampler's race with the GPU on the oracle's
runner-up.  Zero near-ties means the GPU run is bit-identical to the oracle's free run (and, for the reference-minted
goldens, to the reference's own labels and wav).
"""
import os

import numpy as np
import pytest
import torch

from oracle import oracle as orc
from tests.golden_util import load_case
from tests.parity_util import (MOL_LSB, ROW_ROTATION, bound_near_ties, check_free_run_raw, check_on_gpu_trajectory_mol,
                               check_on_gpu_trajectory_raw, label_stats, near_tie_truth, parity_report)

# PARITY_ROWS=subset (developer sessions): the T = 401 tests check a rotating subset of the rows instead of all of them
SUBSET = os.environ.get('PARITY_ROWS', 'all') == 'subset'

pytestmark = pytest.mark.gpu


def _model(sd, mode='RAW', bits=10, kernel='auto'):
    from tacotronv2_wavernn_chinese_amd import _cabi
    from tacotronv2_wavernn_chinese_amd.synth import DEFAULT_DIMS
    from tacotronv2_wavernn_chinese_amd.vocoder import WaveRNN
    dims = dict(DEFAULT_DIMS)
    dims['bits'] = bits
    m = WaveRNN(**dims, mode=mode)
    m.verbose = False
    m.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in sd.items()})
    m.to('cuda:0')
    m.kernel = _cabi.KERNEL_IDS[kernel]
    return m


def _oracle_rows(om, mels, rows, noise_mode, n1=None, n2=None):
    """Oracle on a subset of the batch rows (rows are independent: state is per row, :194-196)."""
    cm, ca = om.conditioning(mels[rows])
    return om.loop(cm, ca, noise_mode, None if n1 is None else np.ascontiguousarray(n1[:, rows]),
                   None if n2 is None else np.ascontiguousarray(n2[:, rows]))


def _forced_raw(om, mels, rows, q):
    """oracle_loop(x_forced) for check_on_gpu_trajectory_raw: the oracle on `rows` of the batch with Exp(1) draws q
    (L, len(rows), n_classes), driven along the trajectory it is handed."""
    cm, ca = om.conditioning(mels[rows])
    return lambda xf: om.loop(cm, ca, orc.NOISE_EXPO, q, x_forced=xf)


def _report(tag, st):
    """Record the check and ASSERT the near-tie rate (tests/parity_util.py: at most 1 + 1e-5 of the compared steps)."""
    bound_near_ties(tag, st['compared'], st['near_ties'])


def test_config1_b1_t401_injected_noise_vs_reference_and_oracle(tmp_path):
    """configs[1]: the benchmarked clip, free-running over all 110 275 steps with the reference's own noise stream
    (452 MB of Exp(1) draws on the device), default segmentation (14 launches), against the labels of the unmodified
    reference and against the oracle driven along the GPU's own trajectory (every step compared)."""
    from tacotronv2_wavernn_chinese_amd import _cabi
    fx = load_case('raw_peaky_b1_t401')
    m = _model(fx['state_dict'])
    res = m.generate_raw(fx['mels'], False, 11000, 550, noise_mode=_cabi.NOISE_INJECTED, noise1=fx['noise']['expo'])
    assert m.last_timing['kernel'] == _cabi.KERNEL_TEAM2 and m.last_timing['launches'] >= 10
    got = res['labels'].cpu().numpy().T
    smp = res['samples'].cpu().numpy().T
    assert got.shape == (401 * 275, 1)
    om = orc.OracleModel(fx['state_dict'], fast=True)
    st = check_on_gpu_trajectory_raw(got, smp, _forced_raw(om, fx['mels'], [0], fx['noise']['expo']))
    _report('configs[1] injected', st)
    assert st['compared'] == 401 * 275
    if not st['near_ties']:
        # identical to the oracle's free run over the whole clip => must equal what the reference itself produced
        np.testing.assert_array_equal(got, fx['labels'].astype(np.int32))
        wav = m.generate(fx['mels'], str(tmp_path / 'c1.wav'), False, 11000, 550, True, noise_mode=_cabi.NOISE_INJECTED,
                         noise1=fx['noise']['expo'])
        assert wav.dtype == np.float64 and wav.shape == (400 * 275,)
        np.testing.assert_array_equal(wav.astype(np.float32), fx['wav'])


def test_config1_b1_t401_philox_production_mode():
    """configs[1] exactly as bench.py runs it (device Philox noise): the draws are reproduced on the host and fed to
    the oracle."""
    from tacotronv2_wavernn_chinese_amd import _cabi
    from tacotronv2_wavernn_chinese_amd.synth import make_mels, make_state_dict
    sd = make_state_dict(0, variant='peaky')
    mels = make_mels(1000, 1, 401)
    m = _model(sd)
    seed = 0xC0FFEE
    res = m.generate_raw(mels, False, 11000, 550, noise_mode=_cabi.NOISE_PHILOX, seed=seed)
    got = res['labels'].cpu().numpy().T
    L = got.shape[0]
    om = orc.OracleModel(sd, fast=True)
    st = check_on_gpu_trajectory_raw(got, res['samples'].cpu().numpy().T, _forced_raw(om, mels, [0], _philox_q(seed, L, [0])))
    _report('configs[1] philox', st)
    assert st['compared'] == L == 401 * 275
    assert len(np.unique(got)) > 100


def _philox_q(seed, L, rows, chunk=4096):
    """Exp(1) draws q = -log(u) of the device's Philox stream for steps [0, L) and the given GLOBAL rows, replayed with torch
    on the GPU (float64 log), as a float32 numpy array (L, len(rows), 1024) for the oracle."""
    from tests.philox_ref import philox_uniform_raw_torch
    q = np.empty((L, len(rows), 1024), np.float32)
    for t0 in range(0, L, chunk):
        n = min(chunk, L - t0)
        u = philox_uniform_raw_torch(seed, t0, n, rows, device='cuda')
        q[t0:t0 + n] = (-torch.log(u.to(torch.float64))).to(torch.float32).cpu().numpy()
    return q


def _philox_q_at(seed, t, row):
    """The 1024 Exp(1) draws of ONE (step, row) of the device's Philox stream, as the oracle is handed them."""
    from tests.philox_ref import philox_uniform_raw_torch
    u = philox_uniform_raw_torch(seed, int(t), 1, [int(row)], device='cuda')
    return (-torch.log(u.to(torch.float64))).to(torch.float32).cpu().numpy()[0, 0]


def _check_rows_raw(tag, sd, mels, lab, smp, seed, rows, group):
    """Rows `rows` of a Philox-sampled RAW batch against the oracle, `group` rows per oracle call (bounds the host copy of the
    replayed draws: L x group x 1024 floats).  Every step of every listed row is compared."""
    om = orc.OracleModel(sd, fast=True)
    L = lab.shape[1]
    compared, near = 0, []
    for i in range(0, len(rows), group):
        rs = rows[i:i + group]
        st = check_on_gpu_trajectory_raw(lab[rs].T, smp[rs].T, _forced_raw(om, mels, rs, _philox_q(seed, L, rs)))
        compared += st['compared']
        near += [(t, rs[r], d) for t, r, d in st['near_ties']]
        for t, r, _ in st['near_ties']:   # float64 verdict on every near-tie (tests/parity_util.near_tie_truth)
            q_t = _philox_q_at(seed, t, rs[r])
            near_tie_truth(tag, sd, mels[rs[r]], smp[rs[r]], t, q_t, lab[rs[r], t], st['ref'], r)
    _report(tag, dict(compared=compared, near_ties=near, max_abs_other=0))
    assert compared == L * len(rows)
    return near


def test_config2_b64_sampled_batch_kernel_all_rows():
    """configs[2]: 64 distinct utterances, sampled (not greedy) with the production Philox noise, T=41 (11 275 steps):
    AUTO picks the batch kernel (8 rows per XCD team in lock-step on the matrix cores).  ALL 64 rows are checked against
    the oracle with the host replay of their draws (the noise is keyed by the global row index, rows are independent):
    64 x 11 275 = 721 600 steps, each compared."""
    from tacotronv2_wavernn_chinese_amd import _cabi
    from tacotronv2_wavernn_chinese_amd.synth import make_mels, make_state_dict
    sd = make_state_dict(0, variant='peaky')
    B, T = 64, 41
    mels = make_mels(4321, B, T)
    m = _model(sd)
    seed = 0x5EED0064
    res = m.generate_raw(mels, False, 11000, 550, noise_mode=_cabi.NOISE_PHILOX, seed=seed)
    assert m.last_timing['kernel'] in (_cabi.KERNEL_BATCH, _cabi.KERNEL_BATCH_CS)
    lab, smp = res['labels'].cpu().numpy(), res['samples'].cpu().numpy()          # (64, L)
    assert lab.shape == (B, T * 275)
    _check_rows_raw('configs[2] B=64 T=41 philox, all rows', sd, mels, lab, smp, seed, list(range(B)), 16)
    # all 64 rows are different utterances with different noise: no two label sequences coincide
    assert len({lab[i, :2000].tobytes() for i in range(B)}) == B
    np.testing.assert_array_equal(smp, 2.0 * lab.astype(np.float32) / np.float32(1023.0) - np.float32(1.0))


def test_config2_b64_injected_reference_noise_all_rows():
    """configs[2] on the REFERENCE-EXACT noise path: B=64, T=41, the sampler fed with injected Exp(1) draws (11 275 x 64 x 1024
    floats = 2.96 GB on the device) exactly as torch.multinomial consumes them (fatchord_version.py:231-237) -- not through the
    Philox replay of tests/philox_ref.py.  All 64 rows, every step, against the oracle on the same draws."""
    from tacotronv2_wavernn_chinese_amd import _cabi
    from tacotronv2_wavernn_chinese_amd.synth import make_mels, make_state_dict
    sd = make_state_dict(0, variant='peaky')
    B, T = 64, 41
    L = T * 275
    mels = make_mels(2468, B, T)
    rng = np.random.Generator(np.random.PCG64(6464))
    q = rng.standard_exponential((L, B, 1024), dtype=np.float32)
    m = _model(sd)
    res = m.generate_raw(mels, False, 11000, 550, noise_mode=_cabi.NOISE_INJECTED, noise1=q)
    assert m.last_timing['kernel'] in (_cabi.KERNEL_BATCH, _cabi.KERNEL_BATCH_CS)
    lab, smp = res['labels'].cpu().numpy(), res['samples'].cpu().numpy()
    del res
    torch.cuda.empty_cache()
    om = orc.OracleModel(sd, fast=True)
    compared, near = 0, []
    for r0 in range(0, B, 16):
        rs = list(range(r0, r0 + 16))
        st = check_on_gpu_trajectory_raw(lab[rs].T, smp[rs].T, _forced_raw(om, mels, rs, np.ascontiguousarray(q[:, rs])))
        compared += st['compared']
        near += [(t, rs[r], d) for t, r, d in st['near_ties']]
    _report(f'configs[2] B=64 T=41 injected Exp(1), {_cabi.KERNEL_NAMES[m.last_timing["kernel"]]} kernel, all rows', dict(compared=compared, near_ties=near))
    assert compared == B * L


def test_config2_b64_t401_full_size_rows():
    """configs[2] at the BASELINE size itself: 64 utterances x mel 80x401 (110 275 steps each, the bench.py workload).
    ALL 64 rows are checked over all their 110 275 steps (round 5; rounds 3-4 checked 8 / 16 rotating rows): 7 057 600 steps, the
    oracle walking 16 rows at a time in parallel.  A near-tie, if one occurs, is re-evaluated in float64 and reported."""
    from tacotronv2_wavernn_chinese_amd import _cabi
    from tacotronv2_wavernn_chinese_amd.synth import make_mels, make_state_dict
    sd = make_state_dict(0, variant='peaky')
    B, T = 64, 401
    mels = make_mels(1000, B, T)
    m = _model(sd)
    seed = 0xC0FFEE
    res = m.generate_raw(mels, False, 11000, 550, noise_mode=_cabi.NOISE_PHILOX, seed=seed)
    assert m.last_timing['kernel'] in (_cabi.KERNEL_BATCH, _cabi.KERNEL_BATCH_CS)
    lab, smp = res['labels'].cpu().numpy(), res['samples'].cpu().numpy()
    rows = sorted(8 * k + (k + ROW_ROTATION + h) % 8 for k in range(8) for h in (0, 4)) if SUBSET else list(range(B))
    _check_rows_raw(f'configs[2] B=64 T=401 philox, {_cabi.KERNEL_NAMES[m.last_timing["kernel"]]} kernel, rows {rows if SUBSET else "all 64"}', sd, mels, lab, smp, seed,
                    rows, 4 if SUBSET else 16)
    assert len({lab[i, :4000].tobytes() for i in range(B)}) == B


def test_config2_b64_t401_injected_reference_noise_rows():
    """configs[2] at the BASELINE size on the REFERENCE-EXACT noise path: 64 utterances x mel 80x401 with injected Exp(1) draws consumed exactly as torch.multinomial consumes
    them (fatchord_version.py:231-237) -- 110 275 x 64 x 1024 floats = 28.9 GB, drawn ON the device (288 GB of HBM: that is what they are for) from a seeded generator.  16 OF THE 64
    rows (two per XCD team, rotating with ROW_ROTATION) are walked by the oracle on the same draws over all their 110 275 steps: the oracle needs its rows' draws on the HOST, 7.2 GB
    per 16 rows -- all 64 would be four such copies + four oracle passes (~4 min of the suite) for a path whose all-rows coverage exists at T = 41
    (test_config2_b64_injected_reference_noise_all_rows) and, with Philox noise, at T = 401 (test_config2_b64_t401_full_size_rows).  The report line says so."""
    from tacotronv2_wavernn_chinese_amd import _cabi
    from tacotronv2_wavernn_chinese_amd.synth import make_mels, make_state_dict
    sd = make_state_dict(0, variant='peaky')
    B, T = 64, 401
    L = T * 275
    mels = make_mels(1357, B, T)
    gen = torch.Generator(device='cuda')
    gen.manual_seed(6401)
    q = torch.empty((L, B, 1024), dtype=torch.float32, device='cuda')
    for t0 in range(0, L, 8192):       # chunks: one exponential_ call per < 2^31 elements
        q[t0:t0 + 8192].exponential_(1.0, generator=gen)
    q.clamp_(min=1e-30)                 # exponential_ can return 0; the reference's p / q would be inf there, the log-domain race needs a finite -log q
    m = _model(sd)
    res = m.generate_raw(mels, False, 11000, 550, noise_mode=_cabi.NOISE_INJECTED, noise1=q)
    assert m.last_timing['kernel'] in (_cabi.KERNEL_BATCH, _cabi.KERNEL_BATCH_CS)
    lab, smp = res['labels'].cpu().numpy(), res['samples'].cpu().numpy()
    del res
    rows = sorted(8 * k + (k + ROW_ROTATION + 2 + h) % 8 for k in range(8) for h in (0, 4))
    qr = q[:, rows].cpu().numpy()       # (L, 16, 1024): 7.2 GB on the host, the rows the oracle walks
    del q
    torch.cuda.empty_cache()
    om = orc.OracleModel(sd, fast=True)
    st = check_on_gpu_trajectory_raw(lab[rows].T, smp[rows].T, _forced_raw(om, mels, rows, qr))
    tag = (f'configs[2] B=64 T=401 injected Exp(1) (28.9 GB on the device), {_cabi.KERNEL_NAMES[m.last_timing["kernel"]]} kernel, 16 of 64 rows (host copy of the draws: 7.2 GB per 16 '
           f'rows; all 64 rows are covered at T=41 on this path and at T=401 with Philox) {rows}')
    for t, r, _ in st['near_ties']:
        near_tie_truth(tag, sd, mels[rows[r]], smp[rows[r]], t, qr[t, r], lab[rows[r], t], st['ref'], r)
    _report(tag, dict(compared=st['compared'], near_ties=[(t, rows[r], d) for t, r, d in st['near_ties']]))
    assert st['compared'] == L * len(rows)


def _mol_case(B, T, rows, tag):
    from tacotronv2_wavernn_chinese_amd import _cabi
    from tacotronv2_wavernn_chinese_amd.synth import make_mels, make_state_dict
    sd = make_state_dict(0, mode='MOL', variant='default', bits=9)
    L = T * 275
    mels = make_mels(777, B, T)
    rng = np.random.Generator(np.random.PCG64(2024))
    u_mix = rng.uniform(1e-5, 1.0 - 1e-5, size=(L, B, 10)).astype(np.float32)
    u_log = rng.uniform(1e-5, 1.0 - 1e-5, size=(L, B)).astype(np.float32)
    m = _model(sd, mode='MOL', bits=9)
    res = m.generate_raw(mels, False, 11000, 550, noise_mode=_cabi.NOISE_INJECTED, noise1=u_mix, noise2=u_log)
    assert m.last_timing['kernel'] in (_cabi.KERNEL_BATCH, _cabi.KERNEL_BATCH_CS)
    smp, mix = res['samples'].cpu().numpy(), res['labels'].cpu().numpy()
    om = orc.OracleModel(sd, mode='MOL', bits=9, fast=True)
    cm, ca = om.conditioning(mels[rows])
    n1, n2 = np.ascontiguousarray(u_mix[:, rows]), np.ascontiguousarray(u_log[:, rows])
    # every step from the GPU's own fed-back sample: mixture index equal (near-tie rule), sample within 2e-5
    st = check_on_gpu_trajectory_mol(smp[rows].T, mix[rows].T, lambda xf: om.loop(cm, ca, 0, n1, n2, x_forced=xf))
    parity_report(f'{tag} ({_cabi.KERNEL_NAMES[m.last_timing["kernel"]]} kernel) rows {rows if len(rows) <= 8 else "all"}: steps compared '
                  f'{st["compared"]}, mixture-index near-ties {st["index_mismatches"]}, max |sample error| {st["max_err"]:.3e} = '
                  f'{st["max_err"] / MOL_LSB:.5f} LSB(9 bit)')
    assert st['compared'] == L * len(rows)
    assert st['index_mismatches'] <= 1 + int(1e-5 * st['compared'])
    assert np.abs(smp).max() <= 1.0


def test_config4_mol_b32_batch_kernel_all_rows():
    """configs[4]: MOL 9-bit, B=32, injected u_mix / u_log, T=41; the batch kernel (4 rows per team).  ALL 32 rows, every
    step: mixture index identical (near-tie rule) and the continuous sample within 2e-5 of the oracle started from the
    GPU's own previous sample."""
    _mol_case(32, 41, list(range(32)), 'configs[4] MOL B=32 T=41')


def test_config4_mol_b32_t401_full_size_rows():
    """configs[4] at the BASELINE size: 32 utterances x mel 80x401; ALL 32 rows over all 110 275 steps (round 5; before: 8 rotating rows)."""
    _mol_case(32, 401, sorted(4 * k + (k + ROW_ROTATION) % 4 for k in range(8)) if SUBSET else list(range(32)), 'configs[4] MOL B=32 T=401')


def test_mol_eight_rows_per_team():
    """MOL at 8 rows per XCD team (B = 40 -> 5 rows per batch -> the two-quad instantiation loop_batch_cs_kernel<MOL, 2>; round-4 advisor: every MOL
    parity case had B <= 32, i.e. one quad): all 40 rows, every step, against the oracle -- and the same instantiation teacher-forced with its
    fc3 outputs (forward()'s path: x_forced + logits_out) against the 4-rows-per-team run of the same batch."""
    from tacotronv2_wavernn_chinese_amd import _cabi
    from tacotronv2_wavernn_chinese_amd.synth import make_mels, make_state_dict
    _mol_case(40, 21, list(range(40)), 'MOL B=40 T=21 (8 rows per team)')
    sd = make_state_dict(0, mode='MOL', variant='default', bits=9)
    B, T = 12, 6
    L = T * 275
    mels = make_mels(31, B, T)
    rng = np.random.Generator(np.random.PCG64(5))
    xf = rng.uniform(-1.0, 1.0, size=(L, B)).astype(np.float32)
    u_mix = rng.uniform(1e-5, 1.0 - 1e-5, size=(L, B, 10)).astype(np.float32)   # the fc3 outputs of a forced trajectory do not depend on the noise
    u_log = rng.uniform(1e-5, 1.0 - 1e-5, size=(L, B)).astype(np.float32)
    m = _model(sd, mode='MOL', bits=9, kernel='batch_cs')
    kw = dict(noise_mode=_cabi.NOISE_INJECTED, noise1=u_mix, noise2=u_log, x_forced=xf, want_logits=True)
    r8 = m.generate_raw(mels, False, 11000, 550, batch_rows=8, **kw)
    l8 = r8['logits'].cpu().numpy()
    r4 = m.generate_raw(mels, False, 11000, 550, batch_rows=4, **kw)
    l4 = r4['logits'].cpu().numpy()
    assert np.isfinite(l8).all() and np.abs(l8 - l4).max() <= 2e-5 * max(1.0, float(np.abs(l4).max()))
    om = orc.OracleModel(sd, mode='MOL', bits=9, fast=True)
    cm, ca = om.conditioning(mels)
    ref = om.loop(cm, ca, 0, u_mix, u_log, x_forced=xf, want_logits=True)
    assert np.abs(l8 - ref['logits']).max() <= 2e-5 * max(1.0, float(np.abs(ref['logits']).max()))


@pytest.mark.parametrize('kernel', ['team2', 'batch', 'batch_cs'])
def test_b8_t60_reference_golden(kernel):
    """A reference-minted golden long enough for several natural segments per row at B = 8 (16 500 steps, no developer
    knob): the latency kernel (one row per XCD team, 8 default segments) and the batch kernel (forced: 8 teams x 1 row
    would be AUTO's choice) against the labels of the unmodified reference."""
    from tacotronv2_wavernn_chinese_amd import _cabi
    fx = load_case('raw_peaky_b8_t60')
    m = _model(fx['state_dict'], kernel=kernel)
    res = m.generate_raw(fx['mels'], False, 11000, 550, noise_mode=_cabi.NOISE_INJECTED, noise1=fx['noise']['expo'])
    if kernel == 'team2':
        assert m.last_timing['launches'] >= 4
    got = res['labels'].cpu().numpy().T
    om = orc.OracleModel(fx['state_dict'], fast=True)
    st = check_on_gpu_trajectory_raw(got, res['samples'].cpu().numpy().T, _forced_raw(om, fx['mels'], list(range(8)), fx['noise']['expo']))
    _report(f'B=8 T=60 {kernel}', st)
    assert st['compared'] == got.size == 8 * 60 * 275
    if not st['near_ties']:   # = the oracle's free run = what the reference produced
        np.testing.assert_array_equal(got, fx['labels'].astype(np.int32))


@pytest.mark.parametrize('kernel', ['team2', 'batch', 'batch_cs', 'simple'])
def test_raw_9bit_has_no_phantom_classes(kernel):
    """RAW with bits < 10 (n_classes < 1024): workgroups / quarter-waves that own no class must not enter the race.
    Labels stay below n_classes and match the oracle."""
    from tacotronv2_wavernn_chinese_amd import _cabi
    from tacotronv2_wavernn_chinese_amd.synth import make_mels, make_state_dict
    bits = 9
    sd = make_state_dict(3, variant='peaky', bits=bits)
    B = 5 if kernel != 'team2' else 2
    mels = make_mels(55, B, 21)
    L = 21 * 275
    rng = np.random.Generator(np.random.PCG64(9))
    q = rng.standard_exponential((L, B, 512)).astype(np.float32)
    m = _model(sd, bits=bits, kernel=kernel)
    res = m.generate_raw(mels, False, 11000, 550, noise_mode=_cabi.NOISE_INJECTED, noise1=q)
    got = res['labels'].cpu().numpy().T
    assert got.min() >= 0 and got.max() < 512
    om = orc.OracleModel(sd, bits=bits, fast=True)
    cm, ca = om.conditioning(mels)
    ref = om.loop(cm, ca, orc.NOISE_EXPO, q)
    first = check_free_run_raw(got, ref)
    smp = res['samples'].cpu().numpy().T
    np.testing.assert_array_equal(smp, 2.0 * got.astype(np.float32) / np.float32(511.0) - np.float32(1.0))
    assert label_stats(got, ref['labels'], first)['max_abs'] <= 1


@pytest.mark.parametrize('kernel', ['team2', 'batch', 'batch_cs', 'simple'])
@pytest.mark.parametrize('bits', [8, 5, 1])
def test_raw_small_class_counts_match_oracle_at_every_step(bits, kernel):
    """RAW at 256, 32 and 2 classes: on the team kernels workgroups 8..31, workgroups 1..31, and all but one quarter-wave
    own no class (at 2 classes the second class slot `cls0 + 4` of the batch kernels is never valid).  Teacher-forced on
    the oracle's own samples and free-running, the labels equal the oracle's at EVERY step: the fixtures keep the oracle's
    race margin >= 1e-4 over the run (tests/size_fixtures.py, asserted by tests/test_size_fixtures_host.py), so there is no
    near-tie to allow for.  Two rows on team2 / simple; five on the batch kernels, so that a row quad is partly filled."""
    from tacotronv2_wavernn_chinese_amd import _cabi
    from tests.size_fixtures import raw_fixture, raw_rows
    B = raw_rows(kernel)
    fx = raw_fixture(bits, B)
    NC, free, forced = fx['n_classes'], fx['free'], fx['forced']
    m = _model(fx['state_dict'], bits=bits, kernel=kernel)
    assert m.n_classes == NC
    noise = dict(noise_mode=_cabi.NOISE_INJECTED, noise1=np.array(fx['q']))
    # teacher-forced on the oracle's samples, with logits
    res = m.generate_raw(fx['mels'], False, 11000, 550, x_forced=np.array(free['samples']), want_logits=True, **noise)
    got, smp, lg = res['labels'].cpu().numpy().T, res['samples'].cpu().numpy().T, res['logits'].cpu().numpy()
    scale = max(1.0, float(np.abs(forced['logits']).max()))
    err = float(np.abs(lg - forced['logits']).max()) if lg.shape == forced['logits'].shape else float('nan')
    parity_report(f'RAW {NC} classes {kernel} teacher-forced: {got.size} steps compared, label mismatches '
                  f'{int(np.count_nonzero(got != forced["labels"]))}, max label {int(got.max())}, max logit error {err:.3e} '
                  f'(bound {2e-5 * scale:.3e}), oracle min margin {fx["min_margin"]:.2e}')
    assert got.shape == (fx['L'], B) and lg.shape == (fx['L'], B, NC)
    assert got.min() >= 0 and got.max() < NC
    np.testing.assert_array_equal(got, forced['labels'])
    assert err <= 2e-5 * scale
    np.testing.assert_array_equal(smp, 2.0 * got.astype(np.float32) / np.float32(NC - 1.0) - np.float32(1.0))
    # free-running
    res = m.generate_raw(fx['mels'], False, 11000, 550, **noise)
    got, smp = res['labels'].cpu().numpy().T, res['samples'].cpu().numpy().T
    bad = np.argwhere(got != free['labels'])
    parity_report(f'RAW {NC} classes {kernel} free-running: {got.size} steps compared, label mismatches {len(bad)} '
                  f'(first at {bad[0].tolist() if len(bad) else None}), oracle min margin {fx["min_margin"]:.2e}')
    assert got.min() >= 0 and got.max() < NC
    np.testing.assert_array_equal(got, free['labels'])
    np.testing.assert_array_equal(smp, 2.0 * got.astype(np.float32) / np.float32(NC - 1.0) - np.float32(1.0))


def test_generate_many_fills_the_teams_with_ragged_utterances(tmp_path):
    """Serving extension: 5 utterances of different lengths in one device call (one per XCD team on the latency kernel).
    Row i, trimmed to its own length, must be what a single generate() call on clip i gives for the same noise."""
    from tacotronv2_wavernn_chinese_amd import _cabi
    from tacotronv2_wavernn_chinese_amd.synth import make_mels, make_state_dict
    sd = make_state_dict(0, variant='peaky')
    m = _model(sd)
    lens = [21, 33, 27, 40, 22]
    clips = [make_mels(300 + i, 1, t)[0] for i, t in enumerate(lens)]
    tmax = max(lens)
    rng = np.random.Generator(np.random.PCG64(77))
    q = rng.standard_exponential((tmax * 275, len(lens), 1024)).astype(np.float32)
    outs = m.generate_many(clips, [tmp_path / f'{i}.wav' for i in range(len(lens))], True, noise_mode=_cabi.NOISE_INJECTED, noise1=q)
    assert m.last_timing['kernel'] == _cabi.KERNEL_TEAM2 and m.last_timing['rows'] == len(lens)
    for i, t in enumerate(lens):
        assert outs[i].shape == ((t - 1) * 275,) and outs[i].dtype == np.float64
        single = m.generate(clips[i][None], tmp_path / 's.wav', False, 11000, 550, True, noise_mode=_cabi.NOISE_INJECTED,
                            noise1=np.ascontiguousarray(q[:t * 275, i:i + 1]))
        np.testing.assert_array_equal(outs[i], single)
        assert (tmp_path / f'{i}.wav').exists()
