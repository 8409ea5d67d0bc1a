"""SURVEY.md section 8a row A12 (secondary): the unconditioned dual-softmax WaveRNN of deepmind_version.py."""
import os

import numpy as np
import pytest

from oracle import oracle as orc
from oracle.noise import dm_noise_from_seed, noise_checksum
from tacotronv2_wavernn_chinese_amd.synth import make_dm_state_dict

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
DM_GOLDENS = sorted(f[:-4] for f in os.listdir(GOLDEN_DIR) if f.startswith('dm_') and f.endswith('.npz'))


def _golden(name='dm_h896_s2000'):
    z = np.load(os.path.join(GOLDEN_DIR, name + '.npz'))
    steps = int(z['steps'])
    # the first fixture carries no sizes: hidden 896, quantisation 256 (oracle/make_golden.py DM_CASES)
    hidden, quant = (int(z['hidden']), int(z['quant'])) if 'hidden' in z.files else (896, 256)
    q = dm_noise_from_seed(int(z['noise_seed']), steps, quant)
    if not np.array_equal(noise_checksum({'q': q}), z['noise_checksum']):
        pytest.skip('torch CPU RNG stream differs from the one the goldens were minted with')
    return z, steps, q, make_dm_state_dict(int(z['weight_seed']), hidden_size=hidden, quantisation=quant)


def test_dm_goldens_cover_a_second_hidden_size_and_a_smaller_quantisation():
    assert {'dm_h896_s2000', 'dm_h512_s1000', 'dm_h640_q128_s1000'} <= set(DM_GOLDENS)


@pytest.mark.parametrize('name', DM_GOLDENS)
def test_oracle_matches_reference_golden(name):
    """The C restatement against generate() of the unmodified reference, which runs at any quantisation: hidden 896 and 512
    at 256 classes, hidden 640 (the odd plane count of the team kernel) at 128.  Every other size of the GPU size sweep
    (tests/test_gpu_dm_sizes.py) rests on the oracle alone: the same code with other loop bounds."""
    z, steps, q, sd = _golden(name)
    assert q.shape == (steps, 2, sd['O2.weight'].shape[0])
    r = orc.DeepmindOracle(sd).generate(steps, q)
    np.testing.assert_array_equal(r['coarse'], z['coarse'].astype(np.int32))
    np.testing.assert_array_equal(r['fine'], z['fine'].astype(np.int32))
    np.testing.assert_array_equal(r['output'], z['output'])
    assert r['output'].min() >= -2 ** 15 and r['output'].max() < 2 ** 15


@pytest.mark.gpu
@pytest.mark.parametrize('kernel', [2, 1], ids=['team', 'single'])
def test_gpu_matches_oracle_and_reference(kernel):
    import torch
    from tacotronv2_wavernn_chinese_amd.deepmind import WaveRNN
    z, steps, q, sd = _golden()
    m = WaveRNN()
    m.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in sd.items()})
    m.to('cuda:0')
    out, coarse, fine = m.generate(steps, noise=q, kernel=kernel)
    ref = orc.DeepmindOracle(sd, fast=True).generate(steps, q)
    got = np.stack([coarse, fine], axis=1)
    want = np.stack([ref['coarse'], ref['fine']], axis=1)
    bad = np.argwhere(got != want)
    if bad.size:   # identical up to the first near-tie (a race between two classes closer than 1e-4)
        t, w = bad[0]
        assert ref['margin'][t, w] < 1e-4 and got[t, w] == ref['runner'][t, w]
    else:
        np.testing.assert_array_equal(coarse, z['coarse'].astype(np.int64))
        np.testing.assert_array_equal(fine, z['fine'].astype(np.int64))
        np.testing.assert_array_equal(out, z['output'].astype(np.int64))
    # own-RNG mode: reproducible under the seed, different across seeds, full 16-bit range format
    a = m.generate(300, seed=5, kernel=kernel)[0]
    b = m.generate(300, seed=5, kernel=kernel)[0]
    c = m.generate(300, seed=6, kernel=kernel)[0]
    np.testing.assert_array_equal(a, b)
    assert not np.array_equal(a, c) and a.dtype == np.int64
    with pytest.raises(ValueError):
        m.generate(10, noise=np.ones((10, 2, 255), np.float32))
    # own-RNG mode against the oracle: the device's draws u = wrnn_uniform(seed, t, coarse / fine, class) replayed on the host
    # (tests/philox_ref.py) and handed to the oracle as q = -log u -- the rule of the golden comparison above, with the suite's RAW
    # near-tie margin.  Both kernels against ONE replay: they draw the same stream (this replaces "> 90 % of 300 samples equal
    # between the two kernels").  A seed with both key words set.
    from tests.parity_util import NEAR_TIE, parity_report
    from tests.philox_ref import philox_dm_exponentials
    pseed = 0x0D0C0B0A00C0FFEE
    pout, pc, pf = m.generate(steps, seed=pseed, kernel=kernel)
    pref = orc.DeepmindOracle(sd, fast=True).generate(steps, philox_dm_exponentials(pseed, 0, steps))
    pgot = np.stack([pc, pf], axis=1)
    pwant = np.stack([pref['coarse'], pref['fine']], axis=1)
    pbad = np.argwhere(pgot != pwant)
    upto = 'the end' if not pbad.size else 'step %d (oracle margin %.3e)' % (int(pbad[0][0]), float(pref['margin'][tuple(pbad[0])]))
    parity_report(f'dual-softmax {"team" if kernel == 2 else "single"} kernel, device Philox noise replayed: {steps} steps x 2 softmaxes, '
                  f'identical up to {upto}')
    if pbad.size:
        t, w = pbad[0]
        assert pref['margin'][t, w] < NEAR_TIE and pgot[t, w] == pref['runner'][t, w], \
            f'step {t} softmax {w}: gpu {pgot[t, w]} oracle {pwant[t, w]} margin {pref["margin"][t, w]:.3e}'
    else:
        np.testing.assert_array_equal(pout, pref['output'])
    assert len(np.unique(pc)) > 20 and len(np.unique(pf)) > 20
