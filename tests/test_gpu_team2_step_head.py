"""The latency kernel after the head of its step was tightened (csrc/loop_team2.hip: T2_HEAD_ONE_TRIP, T2_OUT_SHADOW, T2_PREB1_OPERANDS): kernel='team2',
2 rows x 21 frames (5 775 steps), device Philox noise replayed for the oracle, tests/parity_util.py's near-tie rule unchanged.

What the changes could break, and the case that looks at it:
  * the operands of a step are read behind the PREVIOUS step's last barrier, the first step's behind a barrier in front of the loop, and the outputs of
    a step are stored in window B2..B3 of the next step by a shadow wave, a segment's last step behind the loop: RAW 10 bit with team2_segment=1000 (segments of 992
    steps, six launches: the boundaries fall off the every-64-steps check, the state crosses five relaunches, and every segment's last step has no
    later window), every step against the oracle;
  * labels_out == nullptr stays legal: the same call without a labels buffer, samples bit-equal to the first;
  * samples_out receives the SAMPLED value when x_forced feeds another one: a teacher-forced call on levels drawn at random, every label against the
    oracle forced the same way, samples == the level of the label and != the forced values;
  * quarters that own no class (bits = 5) read their hand-over slots in the step head like every other;
  * MOL (its outputs are stored in window 4 as before; its step head is the rotated one).
"""
import numpy as np
import pytest
import torch

from oracle import oracle as orc
from tests import philox_ref
from tests.parity_util import (MOL_LSB, bound_near_ties, check_on_gpu_trajectory_mol, check_on_gpu_trajectory_raw, check_teacher_forced_raw,
                               parity_report)

pytestmark = pytest.mark.gpu

B, T = 2, 21
L = T * 275
SEED = 0x57E9EAD
SEGMENT = 1000


def _model(sd, mode, bits):
    from tacotronv2_wavernn_chinese_amd import _cabi
    from tacotronv2_wavernn_chinese_amd.synth import DEFAULT_DIMS
    from tacotronv2_wavernn_chinese_amd.vocoder import WaveRNN
    dims = dict(DEFAULT_DIMS)
    dims['bits'] = bits
    m = WaveRNN(**dims, mode=mode)
    m.verbose = False
    m.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in sd.items()})
    m.to('cuda:0')
    m.kernel = _cabi.KERNEL_IDS['team2']
    return m


def _levels(lab, NC):
    return 2.0 * lab.astype(np.float32) / np.float32(NC - 1.0) - np.float32(1.0)


class _Raw:
    """One RAW model at 2^bits classes with its oracle, conditioning and the Exp(1) draws the device makes under SEED."""

    def __init__(self, bits):
        from tacotronv2_wavernn_chinese_amd.synth import make_mels, make_state_dict
        self.NC = 2 ** bits
        self.mels = make_mels(56, B, T)
        sd = make_state_dict(3, variant='peaky', bits=bits)
        self.m = _model(sd, 'RAW', bits)
        assert self.m.n_classes == self.NC
        u = philox_ref.philox_uniform_raw_torch(SEED, 0, L, [0, 1], device='cuda')
        self.q = np.ascontiguousarray((-torch.log(u.to(torch.float64))).to(torch.float32).cpu().numpy()[:, :, :self.NC])
        self.om = orc.OracleModel(sd, bits=bits, fast=True)
        self.cm, self.ca = self.om.conditioning(self.mels)

    def run(self, **kw):
        """(labels, samples), (L, B) each, of one Philox call on kernel team2."""
        from tacotronv2_wavernn_chinese_amd import _cabi
        res = self.m.generate_raw(self.mels, False, 11000, 550, noise_mode=_cabi.NOISE_PHILOX, seed=SEED, **kw)
        assert self.m.last_timing['kernel'] == _cabi.KERNEL_TEAM2
        lab, smp = res['labels'].cpu().numpy().T, res['samples'].cpu().numpy().T
        assert lab.shape == smp.shape == (L, B)
        return lab, smp

    def oracle(self, x_forced):
        return self.om.loop(self.cm, self.ca, orc.NOISE_EXPO, self.q, x_forced=x_forced)

    def check_free_run(self, tag, lab, smp):
        assert lab.min() >= 0 and lab.max() < self.NC
        np.testing.assert_array_equal(smp, _levels(lab, self.NC))
        st = check_on_gpu_trajectory_raw(lab, smp, self.oracle)
        bound_near_ties(f'team2 step head: {tag}, B=2 T=21, philox', st['compared'], st['near_ties'])
        assert st['compared'] == L * B


@pytest.fixture(scope='module')
def raw10():
    return _Raw(10)


@pytest.fixture(scope='module')
def segmented(raw10):
    """The 10-bit run in segments of 992 steps, computed once and left unchanged."""
    lab, smp = raw10.run(team2_segment=SEGMENT)
    lab.setflags(write=False)
    smp.setflags(write=False)
    return lab, smp


def test_raw_10_bit_in_segments_off_the_64_step_check(raw10, segmented):
    assert (SEGMENT & ~31) % 64 != 0 and L > 5 * (SEGMENT & ~31)
    lab, smp = segmented
    raw10.check_free_run(f'RAW 1024 classes, team2_segment={SEGMENT}', lab, smp)
    assert len(np.unique(lab)) > 20
    # the same clip in the library's own segment length (one launch): bit-equal, whichever step a segment ends at
    lab1, smp1 = raw10.run()
    np.testing.assert_array_equal(lab, lab1)
    np.testing.assert_array_equal(smp.view(np.uint32), smp1.view(np.uint32))


def test_raw_10_bit_without_a_labels_buffer(raw10, segmented):
    nat = raw10.m.native()
    with_labels = nat.generate
    seen = []

    def without_labels(*a, **kw):
        seen.append(kw['labels_ptr'])
        kw['labels_ptr'] = 0
        return with_labels(*a, **kw)
    nat.generate = without_labels
    try:
        _, smp = raw10.run(team2_segment=SEGMENT)
    finally:
        del nat.generate
    assert len(seen) == 1 and seen[0] != 0
    np.testing.assert_array_equal(smp.view(np.uint32), segmented[1].view(np.uint32))


def test_teacher_forced_samples_are_the_sampled_values(raw10):
    rng = np.random.Generator(np.random.PCG64(17))
    xf = _levels(rng.integers(0, raw10.NC, size=(L, B)), raw10.NC)
    lab, smp = raw10.run(team2_segment=SEGMENT, x_forced=xf)
    np.testing.assert_array_equal(smp, _levels(lab, raw10.NC))
    assert np.count_nonzero(smp != xf) > 0.9 * L * B
    ref = raw10.oracle(xf)
    near = check_teacher_forced_raw(lab, ref)
    bound_near_ties('team2 step head: RAW 1024 classes, teacher-forced on random levels, B=2 T=21, philox', L * B,
                    [(int(t), int(r), int(abs(int(lab[t, r]) - int(ref['labels'][t, r])))) for t, r in np.argwhere(lab != ref['labels'])])
    assert near == np.count_nonzero(lab != ref['labels'])


def test_raw_5_bit_quarters_without_a_class():
    r = _Raw(5)
    lab, smp = r.run(team2_segment=SEGMENT)
    r.check_free_run(f'RAW 32 classes, team2_segment={SEGMENT}', lab, smp)


def test_mol_against_the_oracle():
    from tacotronv2_wavernn_chinese_amd import _cabi
    from tacotronv2_wavernn_chinese_amd.synth import make_mels, make_state_dict
    sd = make_state_dict(0, mode='MOL', variant='default', bits=9)
    mels = make_mels(56, B, T)
    m = _model(sd, 'MOL', 9)
    res = m.generate_raw(mels, False, 11000, 550, noise_mode=_cabi.NOISE_PHILOX, seed=SEED, team2_segment=SEGMENT)
    assert m.last_timing['kernel'] == _cabi.KERNEL_TEAM2
    smp, mix = res['samples'].cpu().numpy(), res['labels'].cpu().numpy()
    assert smp.shape == (B, L)
    u_mix, u_log = philox_ref.philox_mol_uniforms(SEED, 0, L, [0, 1])
    om = orc.OracleModel(sd, mode='MOL', bits=9, fast=True)
    cm, ca = om.conditioning(mels)
    st = check_on_gpu_trajectory_mol(np.ascontiguousarray(smp.T), np.ascontiguousarray(mix.T), lambda xf: om.loop(cm, ca, 0, u_mix, u_log, x_forced=xf))
    parity_report(f'team2 step head: MOL B=2 T=21, philox, team2_segment={SEGMENT}: steps compared {st["compared"]}, mixture-index near-ties '
                  f'{st["index_mismatches"]}, max |sample error| {st["max_err"]:.3e} = {st["max_err"] / MOL_LSB:.5f} LSB(9 bit)')
    assert st['compared'] == L * B
    assert st['index_mismatches'] <= 1 + int(1e-5 * st['compared'])
    assert np.abs(smp).max() <= 1.0
