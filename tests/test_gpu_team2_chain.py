"""The latency kernel after its per-quarter constants, hand-over slots and noise slots are read AHEAD of the dot products (csrc/loop_team2.hip,
T2_HOIST_LDS) and its polls fall straight through (T2_STRAIGHT_POLL): one process, kernel='team2', 2 rows x 21 frames (5 775 steps), device Philox
noise replayed for the oracle.

RAW at 10 bits, then 1, then 10 again, then 5.  At the low class counts most quarter-waves own no class: their noise slot is never written by the
shadow wave, and the hoisted read now READS it and discards it by select.  Whatever a previous launch left in that LDS -- the 10-bit run writes every
slot -- must not reach the race: every run matches the oracle at every step (tests/parity_util.py's rule, unchanged), and the two 10-bit runs are
bit-equal in labels and samples.  One MOL run of the same size against the oracle under the existing MOL tolerances.
"""
import numpy as np
import pytest
import torch

from oracle import oracle as orc
from tests import philox_ref
from tests.parity_util import MOL_LSB, bound_near_ties, check_on_gpu_trajectory_mol, check_on_gpu_trajectory_raw, parity_report

pytestmark = pytest.mark.gpu

B, T = 2, 21
L = T * 275
SEED = 0x7EA20C4A


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


def _raw_run(bits, mels):
    """One free-running Philox run at 2^bits classes against the oracle driven along the GPU's own trajectory: (labels, samples), (L, B)."""
    from tacotronv2_wavernn_chinese_amd import _cabi
    from tacotronv2_wavernn_chinese_amd.synth import make_state_dict
    NC = 2 ** bits
    sd = make_state_dict(3, variant='peaky', bits=bits)
    m = _model(sd, 'RAW', bits)
    assert m.n_classes == NC
    res = m.generate_raw(mels, False, 11000, 550, noise_mode=_cabi.NOISE_PHILOX, seed=SEED)
    assert m.last_timing['kernel'] == _cabi.KERNEL_TEAM2
    lab, smp = res['labels'].cpu().numpy().T, res['samples'].cpu().numpy().T
    assert lab.shape == smp.shape == (L, B)
    assert lab.min() >= 0 and lab.max() < NC
    np.testing.assert_array_equal(smp, 2.0 * lab.astype(np.float32) / np.float32(NC - 1.0) - np.float32(1.0))
    u = philox_ref.philox_uniform_raw_torch(SEED, 0, L, [0, 1], device='cuda')
    q = (-torch.log(u.to(torch.float64))).to(torch.float32).cpu().numpy()[:, :, :NC]
    om = orc.OracleModel(sd, bits=bits, fast=True)
    cm, ca = om.conditioning(mels)
    st = check_on_gpu_trajectory_raw(lab, smp, lambda xf: om.loop(cm, ca, orc.NOISE_EXPO, np.ascontiguousarray(q), x_forced=xf))
    bound_near_ties(f'team2 chain: RAW {NC} classes, B=2 T=21, philox', st['compared'], st['near_ties'])
    assert st['compared'] == L * B
    return lab, smp


def test_raw_class_counts_in_one_process_and_the_repeat_is_bit_equal():
    from tacotronv2_wavernn_chinese_amd.synth import make_mels
    mels = make_mels(55, B, T)
    first = _raw_run(10, mels)
    _raw_run(1, mels)
    again = _raw_run(10, mels)
    _raw_run(5, mels)
    np.testing.assert_array_equal(first[0], again[0])
    np.testing.assert_array_equal(first[1].view(np.uint32), again[1].view(np.uint32))
    assert len(np.unique(first[0])) > 20


def test_mol_same_size_against_the_oracle():
    from tacotronv2_wavernn_chinese_amd import _cabi
    from tacotronv2_wavernn_chinese_amd.synth import make_mels, make_state_dict
    sd = make_state_dict(0, mode='MOL', variant='default', bits=9)
    mels = make_mels(55, B, T)
    m = _model(sd, 'MOL', 9)
    res = m.generate_raw(mels, False, 11000, 550, noise_mode=_cabi.NOISE_PHILOX, seed=SEED)
    assert m.last_timing['kernel'] == _cabi.KERNEL_TEAM2
    smp, mix = res['samples'].cpu().numpy(), res['labels'].cpu().numpy()
    assert smp.shape == (B, L)
    u_mix, u_log = philox_ref.philox_mol_uniforms(SEED, 0, L, [0, 1])
    om = orc.OracleModel(sd, mode='MOL', bits=9, fast=True)
    cm, ca = om.conditioning(mels)
    st = check_on_gpu_trajectory_mol(np.ascontiguousarray(smp.T), np.ascontiguousarray(mix.T), lambda xf: om.loop(cm, ca, 0, u_mix, u_log, x_forced=xf))
    parity_report(f'team2 chain: MOL B=2 T=21, philox: steps compared {st["compared"]}, mixture-index near-ties {st["index_mismatches"]}, '
                  f'max |sample error| {st["max_err"]:.3e} = {st["max_err"] / MOL_LSB:.5f} LSB(9 bit)')
    assert st['compared'] == L * B
    assert st['index_mismatches'] <= 1 + int(1e-5 * st['compared'])
    assert np.abs(smp).max() <= 1.0
