"""Fold mode for SEVERAL utterances in one device call (`wrnn_generate_folded`, `generate_many(batched=True)`).

The reference for utterance b is always the oracle on clip b ALONE: `conditioning(mel_b[None])`, `fold`, then the loop driven along the GPU's own
trajectory with the noise of the utterance's GLOBAL rows fold0[b] .. fold0[b + 1] - 1.  Every step of every row is compared under the project's
rules (tests/parity_util.py): a fold that runs past its utterance's end must see ZERO conditioning from frames[b] * hop on, although the padded
batch goes on to frame T -- a table entry left unmasked there shows at the first such step.  Shapes: hop 275, the smallest clips (T >= 21) that
reach each kernel and each masking path; fold counts are asserted.
"""
import numpy as np
import pytest
import torch

from tests.parity_util import MOL_LSB, bound_near_ties, check_on_gpu_trajectory_mol, check_on_gpu_trajectory_raw, parity_report

pytestmark = pytest.mark.gpu
HOP = 275
EPS4 = 4 * np.finfo(np.float64).eps
_CACHE = {}


def _raw():
    """(model, oracle model, state_dict) for the RAW peaky weights, built once."""
    if 'raw' not in _CACHE:
        from oracle import oracle as orc
        from tacotronv2_wavernn_chinese_amd.synth import make_state_dict
        from tests.test_gpu_fold_latency import _model
        sd = make_state_dict(0, variant='peaky')
        _CACHE['raw'] = (_model(sd), orc.OracleModel(sd, fast=True), sd)
    return _CACHE['raw']


def _mol():
    if 'mol' not in _CACHE:
        from oracle import oracle as orc
        from tacotronv2_wavernn_chinese_amd.synth import make_state_dict
        from tests.test_gpu_fold_latency import _model
        sd = make_state_dict(0, mode='MOL', variant='default', bits=9)
        _CACHE['mol'] = (_model(sd, mode='MOL', bits=9), orc.OracleModel(sd, mode='MOL', bits=9, fast=True), sd)
    return _CACHE['mol']


def _clips(frames, seed0=4000):
    from tacotronv2_wavernn_chinese_amd.synth import make_mels
    return [make_mels(seed0 + i, 1, t)[0] for i, t in enumerate(frames)]


def _pad(clips):
    batch = np.zeros((len(clips), 80, max(c.shape[1] for c in clips)), np.float32)
    for i, c in enumerate(clips):
        batch[i, :, :c.shape[1]] = c
    return batch, [c.shape[1] for c in clips]


def _folds_of(om, clip, target, overlap):
    cm, ca = om.conditioning(clip[None])
    return om.fold(cm, target, overlap), om.fold(ca, target, overlap)


def _check_raw(tag, om, clips, res, target, overlap, q_of_rows):
    """Every step of every row of every utterance against the oracle on that clip alone.  q_of_rows(global rows) -> (steps, n, 1024) Exp(1)."""
    from oracle import oracle as orc
    lab, smp, fold0 = res['labels'].cpu().numpy(), res['samples'].cpu().numpy(), res['fold0']
    assert lab.shape == (fold0[-1], target + 2 * overlap)
    compared, near = 0, []
    for b, clip in enumerate(clips):
        cm, ca = _folds_of(om, clip, target, overlap)
        rs = list(range(fold0[b], fold0[b + 1]))
        assert cm.shape[0] == len(rs), (b, cm.shape[0], len(rs))
        q = q_of_rows(rs)
        st = check_on_gpu_trajectory_raw(lab[rs].T, smp[rs].T, lambda xf: om.loop(cm, ca, orc.NOISE_EXPO, q, x_forced=xf))
        compared += st['compared']
        near += [(t, rs[r], d) for t, r, d in st['near_ties']]
    bound_near_ties(tag, compared, near)
    assert compared == lab.size


def _philox(seed, steps):
    from tests.test_gpu_baseline_sizes import _philox_q
    return lambda rs: _philox_q(seed, steps, rs)


FOUR = (21, 30, 24, 22)   # longest not first; 21: last fold crosses its end by 175 samples, 22: by 550 = 2 frames, 24: divides exactly (550/100)


def test_batch_cs_four_rows_per_team_every_step():
    """42 folds (9 + 13 + 10 + 10) x 750 steps in batches of 4 rows: the one-quad batch kernel, 11 batches on 8 teams."""
    from tacotronv2_wavernn_chinese_amd import _cabi
    m, om, _ = _raw()
    clips = _clips(FOUR)
    batch, frames = _pad(clips)
    res = m.generate_raw_folded(batch, frames, 550, 100, seed=0xF01D, batch_rows=4)
    assert res['fold0'].tolist() == [0, 9, 22, 32, 42] and res['steps'] == 750
    assert m.last_timing['kernel'] == _cabi.KERNEL_BATCH_CS and m.last_timing['rows'] == 42 and m.last_timing['steps'] == 750
    _check_raw('fold many: 4 utterances x 42 folds, batch_cs 4 rows/team', om, clips, res, 550, 100, _philox(0xF01D, 750))


def test_batch_cs_eight_rows_per_team_two_passes_every_step():
    """The same clips at 250/50: 90 folds (20 + 28 + 22 + 20) x 350 steps = 12 batches of 8 on 8 teams; utterance 3 divides exactly."""
    from tacotronv2_wavernn_chinese_amd import _cabi
    m, om, _ = _raw()
    clips = _clips(FOUR)
    batch, frames = _pad(clips)
    res = m.generate_raw_folded(batch, frames, 250, 50, seed=0xBEE)
    assert res['fold0'].tolist() == [0, 20, 48, 70, 90] and res['steps'] == 350
    assert m.last_timing['kernel'] == _cabi.KERNEL_BATCH_CS and m.last_timing['rows'] == 90
    _check_raw('fold many: 4 utterances x 90 folds, batch_cs 8 rows/team', om, clips, res, 250, 50, _philox(0xBEE, 350))


def test_team2_segmented_every_step():
    """6 folds (3 + 3) x 2 800 steps on the latency kernel in three launches: utterance 0's last fold runs 2 425 samples past its own end --
    masked records through the conditioning stream, masked C2 / C3 / C4, and the call-wide limit beyond frame 24."""
    from tacotronv2_wavernn_chinese_amd import _cabi
    m, om, _ = _raw()
    clips = _clips((21, 24), seed0=4100)
    batch, frames = _pad(clips)
    res = m.generate_raw_folded(batch, frames, 2600, 100, seed=0x7EA, team2_segment=1024)
    assert res['fold0'].tolist() == [0, 3, 6] and res['steps'] == 2800
    assert m.last_timing['kernel'] == _cabi.KERNEL_TEAM2 and m.last_timing['launches'] == 3
    _check_raw('fold many: 2 utterances x 6 folds, team2 in 3 segments', om, clips, res, 2600, 100, _philox(0x7EA, 2800))


def _mol_case():
    m, om, _ = _mol()
    clips = _clips((21, 30, 24), seed0=4200)
    batch, frames = _pad(clips)
    rng = np.random.Generator(np.random.PCG64(99))
    u_mix = rng.uniform(1e-5, 1.0 - 1e-5, size=(750, 32, 10)).astype(np.float32)
    u_log = rng.uniform(1e-5, 1.0 - 1e-5, size=(750, 32)).astype(np.float32)
    res = m.generate_raw_folded(batch, frames, 550, 100, noise_mode='injected', noise1=u_mix, noise2=u_log)
    assert res['fold0'].tolist() == [0, 9, 22, 32] and res['steps'] == 750
    return m, om, clips, res, u_mix, u_log


def test_mol_9bit_every_step():
    from tacotronv2_wavernn_chinese_amd import _cabi
    m, om, clips, res, u_mix, u_log = _mol_case()
    assert m.last_timing['kernel'] == _cabi.KERNEL_BATCH_CS
    smp, mix, fold0 = res['samples'].cpu().numpy(), res['labels'].cpu().numpy(), res['fold0']
    compared = mism = 0
    worst = 0.0
    for b, clip in enumerate(clips):
        cm, ca = _folds_of(om, clip, 550, 100)
        rs = list(range(fold0[b], fold0[b + 1]))
        st = check_on_gpu_trajectory_mol(smp[rs].T, mix[rs].T, lambda xf: om.loop(cm, ca, 0, np.ascontiguousarray(u_mix[:, rs]), np.ascontiguousarray(u_log[:, rs]), x_forced=xf))
        compared, mism, worst = compared + st['compared'], mism + st['index_mismatches'], max(worst, st['max_err'])
    parity_report(f'fold many MOL: 3 utterances x 32 folds x 750 steps, batch_cs: steps compared {compared}, mixture-index near-ties {mism}, '
                  f'max |sample error| {worst:.3e} = {worst / MOL_LSB:.5f} LSB(9 bit)')
    assert compared == 32 * 750 and mism <= 1 and worst <= 2e-5


def test_simple_kernel_every_step():
    """The any-shape kernel reads mels and aux directly: its per-utterance limit (`WrnnLoopArgs.frames`), 6 folds x 2 800 steps."""
    from tacotronv2_wavernn_chinese_amd import _cabi
    m, om, _ = _raw()
    clips = _clips((21, 23), seed0=4300)
    batch, frames = _pad(clips)
    res = m.generate_raw_folded(batch, frames, 2600, 100, seed=0x51, kernel='simple')
    assert res['fold0'].tolist() == [0, 3, 6] and m.last_timing['kernel'] == _cabi.KERNEL_SIMPLE
    _check_raw('fold many: 2 utterances x 6 folds, simple', om, clips, res, 2600, 100, _philox(0x51, 2800))


def test_an_utterances_rows_do_not_depend_on_the_other_utterances():
    """Injected noise, batch_cs with 4 rows per batch: utterance b's rows are bit-equal to a solo folded call on clip b with its slice of the noise."""
    from tacotronv2_wavernn_chinese_amd import _cabi
    m, _, _ = _raw()
    clips = _clips(FOUR)
    batch, frames = _pad(clips)
    gen = torch.Generator(device='cuda').manual_seed(5)
    noise = torch.empty((750, 42, 1024), dtype=torch.float32, device='cuda').exponential_(1, generator=gen).clamp_(min=1.2e-38)
    res = m.generate_raw_folded(batch, frames, 550, 100, noise_mode='injected', noise1=noise, kernel='batch_cs', batch_rows=4)
    fold0 = res['fold0']
    for b, clip in enumerate(clips):
        solo = m.generate_raw(clip[None], True, 550, 100, noise_mode=_cabi.NOISE_INJECTED, noise1=noise[:, fold0[b]:fold0[b + 1]].contiguous(),
                              kernel=_cabi.KERNEL_BATCH_CS, batch_rows=4)
        assert solo['rows'] == fold0[b + 1] - fold0[b]
        assert torch.equal(solo['labels'], res['labels'][fold0[b]:fold0[b + 1]]), b
        assert torch.equal(solo['samples'], res['samples'][fold0[b]:fold0[b + 1]]), b


def _device_epilogue(m, res, mu_law, out_stride):
    nat = m.native()
    waves = torch.full((res['B'], out_stride), float('nan'), dtype=torch.float64, device='cuda')
    nat.epilogue_folded(res['samples'].data_ptr(), res['labels'].data_ptr(), res['B'], res['rows'], res['steps'], res['target'], res['overlap'],
                        mu_law, res['frames'].data_ptr(), waves.data_ptr(), out_stride, torch.cuda.current_stream().cuda_stream)
    return waves.cpu().numpy()


def _check_epilogue(m, res, frames, mu_law, n_classes):
    from oracle import oracle as orc
    stride = (max(frames) - 1) * HOP + 37
    waves = _device_epilogue(m, res, mu_law, stride)
    smp, fold0 = res['samples'].cpu().numpy(), res['fold0']
    for b, t_b in enumerate(frames):
        wl = (t_b - 1) * HOP
        want = orc.epilogue(smp[fold0[b]:fold0[b + 1]], n_classes, mu_law, True, res['target'], res['overlap'], wl, HOP)
        np.testing.assert_allclose(waves[b, :wl], want, rtol=0, atol=EPS4)
        assert np.all(waves[b, wl:] == 0.0)


def test_epilogue_folded_raw_and_generate_many(tmp_path):
    from tacotronv2_wavernn_chinese_amd import _cabi
    m, _, _ = _raw()
    clips = _clips(FOUR)
    batch, frames = _pad(clips)
    res = m.generate_raw_folded(batch, frames, 550, 100, seed=0xF01D, batch_rows=4)
    _check_epilogue(m, res, frames, True, m.n_classes)
    # the public call: device and host tails agree, shapes / dtype / length as generate() returns them, wavs written
    paths = [tmp_path / f'{i}.wav' for i in range(4)]
    dev = m.generate_many(clips, paths, True, 'device', batched=True, target=550, overlap=100, seed=7, batch_rows=4)
    host = m.generate_many(clips, None, True, 'host', batched=True, target=550, overlap=100, seed=7, batch_rows=4)
    assert m.training and all(p.exists() for p in paths)
    for t_b, a, b in zip(frames, dev, host):
        assert a.shape == b.shape == ((t_b - 1) * HOP,) and a.dtype == b.dtype == np.float64
        np.testing.assert_allclose(a, b, rtol=0, atol=EPS4)
    # the fold offsets on the handle belong to ONE plan: another folded call in between is WRNN_ERR_STATE for the old plan's tail
    other = m.generate_raw_folded(batch, frames, 250, 50, seed=1)
    with pytest.raises(_cabi.WrnnError) as ei:
        _device_epilogue(m, res, True, (max(frames) - 1) * HOP)
    assert ei.value.code == _cabi.ERR_STATE
    _check_epilogue(m, other, frames, True, m.n_classes)


def test_epilogue_folded_mol():
    m, _, _, res, _, _ = _mol_case()
    _check_epilogue(m, res, [21, 30, 24], False, m.n_classes)
    auto = m.generate_many(_clips((21, 30, 24), seed0=4200), None, True, 'device', batched=True, target='auto', overlap=100, seed=3)
    assert [a.shape for a in auto] == [((t - 1) * HOP,) for t in (21, 30, 24)] and all(np.isfinite(a).all() for a in auto)


def test_rows_total_mismatch_is_reported_and_touches_nothing_outside():
    """rows_total one too large / one too small: WRNN_ERR_INVALID from the timing call, the rows both calls have in common are the correct
    call's (same keys, valid (utt, start) everywhere), and the handle works afterwards."""
    from tacotronv2_wavernn_chinese_amd import _cabi
    m, _, _ = _raw()
    clips = _clips(FOUR)
    batch, frames = _pad(clips)
    good = m.generate_raw_folded(batch, frames, 550, 100, seed=0xF01D, batch_rows=4)
    for wrong in (43, 41):
        with pytest.raises(_cabi.WrnnError) as ei:
            m.generate_raw_folded(batch, frames, 550, 100, seed=0xF01D, batch_rows=4, rows_total=wrong)
        assert ei.value.code == _cabi.ERR_INVALID and 'rows_total' in str(ei.value)
    again = m.generate_raw_folded(batch, frames, 550, 100, seed=0xF01D, batch_rows=4)
    assert torch.equal(again['labels'], good['labels']) and torch.equal(again['samples'], good['samples'])
    # what the mismatched calls computed: driven through the binding so that the outputs survive the error
    nat = m.native()
    mels_t = torch.from_numpy(batch).cuda()
    for wrong in (43, 41):
        lab = torch.full((43, 750), -7, dtype=torch.int32, device='cuda')
        smp = torch.full((43, 750), -7.0, dtype=torch.float32, device='cuda')
        nat.generate_folded(mels_t.data_ptr(), 4, 30, good['frames'].data_ptr(), wrong, 550, 100, labels_ptr=lab.data_ptr(), samples_ptr=smp.data_ptr(),
                            stream=torch.cuda.current_stream().cuda_stream, seed=0xF01D, batch_rows=4)
        with pytest.raises(_cabi.WrnnError):
            nat.last_timing()
        n = min(wrong, 42)
        assert torch.equal(lab[:n], good['labels'][:n]) and torch.equal(smp[:n], good['samples'][:n])
        assert bool((lab[wrong:] == -7).all()) and bool((smp[wrong:] == -7.0).all())
        if wrong == 43:   # the extra row repeats the last valid (utt, start): real labels, not garbage
            assert int(lab[42].min()) >= 0 and int(lab[42].max()) < 1024


def test_a_single_clip_is_generate(tmp_path):
    from tacotronv2_wavernn_chinese_amd.synth import make_mels
    m, _, _ = _raw()
    mel = make_mels(4400, 1, 30)
    one = m.generate_many([mel[0]], None, True, 'host', batched=True, target=550, overlap=100, seed=21)
    ref = m.generate(mel, tmp_path / 'a.wav', True, 550, 100, True, seed=21)
    assert len(one) == 1
    np.testing.assert_array_equal(one[0], ref)
    one_d = m.generate_many([mel[0]], None, True, 'device', batched=True, target=550, overlap=100, seed=21)
    ref_d = m.generate(mel, tmp_path / 'b.wav', True, 550, 100, True, seed=21, epilogue='device')
    np.testing.assert_array_equal(one_d[0], ref_d)


def test_generate_folded_refuses_what_it_cannot_honour():
    from tacotronv2_wavernn_chinese_amd import _cabi
    import ctypes as C
    m, _, _ = _raw()
    nat = m.native()
    batch, frames = _pad(_clips((21, 24)))
    with pytest.raises(ValueError, match='reference'):
        m.generate_raw_folded(batch, frames, 550, 100, noise_mode='reference')
    with pytest.raises(ValueError, match='frames'):
        m.generate_raw_folded(batch, [21, 25], 550, 100)
    with pytest.raises(_cabi.WrnnError):   # the single-utterance entry points keep refusing B > 1 in fold mode
        m.generate_raw(batch, True, 550, 100)
    o = _cabi.SampleOpts()
    o.struct_size = C.sizeof(_cabi.SampleOpts)
    mels_t, fr_t = torch.from_numpy(batch).cuda(), torch.tensor(frames, dtype=torch.int32, device='cuda')
    out = torch.empty((19, 750), dtype=torch.float32, device='cuda')
    for field in ('frames_dev', 'x_forced_dev', 'x_init_dev', 'logits_out_dev', 'mels_padded'):
        setattr(o, field, 1 if field == 'mels_padded' else out.data_ptr())
        rc = nat.lib.wrnn_generate_folded(nat._h, mels_t.data_ptr(), 2, 24, fr_t.data_ptr(), 19, 550, 100, C.byref(o), None, out.data_ptr(), None)
        assert rc == _cabi.ERR_INVALID, field
        setattr(o, field, 0 if field == 'mels_padded' else None)
