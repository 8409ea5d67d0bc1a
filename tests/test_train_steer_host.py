"""CPU, anywhere: the construction of tests/train_steer.py checked in float64, for every (mode, B, L) of tests/test_gpu_train_steer.py
with L <= 7 (n = 8 teams, the MI355X's).  What the GPU tests rely on is asserted here, not assumed: every fc1 / fc2 pre-activation at
least 0.25 from zero, the masks equal to the predicted s * u > 0 pattern, half the units on, the mask varying along rows, steps and
units, and -- the proof that the inputs carry no hidden flip -- torch's float32 evaluation of the same restatement within 2e-6 of the
largest entry of every gradient tensor of the float64 one (RAW; for MOL float32 is no yardstick: the loss gradient's cdf_plus - cdf_min
cancellation puts torch's float32 gradients 8e-4 ... 2.6e-3 off).

Measured (float32 vs float64, worst tensor, of its largest entry): default dims 5.4e-7 ... 8.3e-7 over the 20 RAW cases here
(9.4e-7 at B = 5, L = 64, which only the GPU file runs), generic dims 7.9e-7 ... 8.6e-7 (B = 1, L = 1: d_aux); c1 = 1.24 ... 1.95,
c2 = 1.80 ... 3.39; on-fraction exactly 0.5.  Per batch row of d_mels_up / d_aux, against the row's OWN largest entry, the same
float32 evaluation is off by up to 3.3e-5 (B = 130, L = 1; 3.6e-6 at most elsewhere): the source of ROW_TOL in the GPU file.
The six sets of the `<0>` branches (BRANCH_DIMS: rnn 16 ... 880), 18 RAW cases at (1, 1), (2, 2), (33, 3): 3.1e-7 ... 8.5e-7, but
1.31e-6 at h880 (1, 1) (d_mels_up), the worst of this file; per row 1.31e-6 at most (the same case; 1.03e-6 elsewhere);
c1 = 0.88 ... 2.12, c2 = 1.01 ... 2.93; on-fraction exactly 0.5, the MOL cases (h48, h272) included.
"""
import numpy as np
import pytest
import torch

from tests import train_steer as ts

N_TEAMS = 8
HOST_CASES = [c for c in ts.ALL_CASES if c[3] <= 7]


def test_the_case_list_covers_what_it_says():
    from tacotronv2_wavernn_chinese_amd import _cabi
    assert ts.GRAD_KEYS == _cabi.LOOP_PARAM_KEYS
    n = N_TEAMS
    rpb = lambda B: min(8, -(-B // n))
    rows = [ts.batch_of(c[2], n) for c in ts.ROWS_SWEEP]
    assert rows == [1, 9, 17, 25, 33, 41, 49, 57, 64, 70, 130] and [rpb(B) for B in rows[:8]] == list(range(1, 9))
    assert [B % rpb(B) for B in rows[1:8]] == [1, 2, 1, 3, 5, 0, 1]    # ragged last batch, but B = 49: 7 full batches, one team idle
    assert -(-130 // 8) == 17 and -(-70 // 8) == 9                      # batches: team 0 runs three / two of them
    assert {(ts.batch_of(c[2], n), c[3]) for c in ts.LENGTH_SWEEP} == {(B, L) for B in (5, 33, 130) for L in (1, 2, 3, 64, 65)}
    assert ts.SPLIT_CASE in ts.ALL_CASES and len(set(ts.ALL_CASES)) == len(ts.ALL_CASES)
    assert max(ts.batch_of(c[2], n) * c[3] for c in ts.ALL_CASES) == 8450
    # the branches of `gru_*_step_kernel<0>` (csrc/train.hip): what each set of BRANCH_DIMS is there for, as arithmetic on its dims
    bd = ts.BRANCH_DIMS
    assert list(bd) == ['h16', 'h48', 'h272', 'h320', 'h528', 'h880'] and all(bd[k]['rnn_dims'] == int(k[1:]) for k in bd)
    assert all(d['rnn_dims'] % 16 == 0 and d['rnn_dims'] != 512 and d['res_out_dims'] % 4 == 0 and d['fc_dims'] % 2 == 0 for d in bd.values())
    G = {k: 3 * d['rnn_dims'] for k, d in bd.items()}
    assert {k: (g // 768, g % 768) for k, g in G.items()} == \
        {'h16': (0, 48), 'h48': (0, 144), 'h272': (1, 48), 'h320': (1, 192), 'h528': (2, 48), 'h880': (3, 336)}   # full chunks, tail chunk
    assert 3 * ts.GENERIC_DIMS['rnn_dims'] == 768                      # the generic set: exactly one full chunk, no tail
    assert [k for k, d in bd.items() if (d['rnn_dims'] // 4) % 8 == 0] == ['h320']        # `xcd_tile` remaps; identity for the others
    assert bd['h16']['rnn_dims'] // 4 == 4 and 2 ** bd['h16']['bits'] == 32 < 64 and bd['h16']['res_out_dims'] // 4 == 1
    assert bd['h48']['res_out_dims'] // 4 == 5 and bd['h48']['res_out_dims'] % 8 != 0
    assert [k for k, d in bd.items() if d['fc_dims'] > max(3 * d['rnn_dims'], 2 ** d['bits'])] == ['h48']   # the column-sum scratch
    assert 44 * (880 + 4) * 4 + 8192 <= 160 * 1024 < 44 * (896 + 4) * 4 + 8192          # h880: the largest `train_impl` admits
    assert (32 * (768 + 4) + 4 * (3 * 896 + 4) + 512) * 4 <= 160 * 1024                 # the forward tile is what binds, not the backward
    assert ts.BRANCH_CASES == ts.ALL_CASES[-20:] and ts.BRANCH_SPLIT_CASE in ts.BRANCH_CASES
    assert {(c[0], c[2][1], c[3]) for c in ts.BRANCH_CASES if c[1] == 'h272'} == {('RAW', 1, 1), ('RAW', 2, 2), ('RAW', 33, 3), ('MOL', 33, 3)}
    assert all(sum(c[1] == k for c in ts.BRANCH_CASES) == (4 if k in ('h48', 'h272') else 3) for k in bd)
    assert all(c in HOST_CASES for c in ts.BRANCH_CASES)
    assert [ts.case_seed(c) for c in (ts.ALL_CASES[0], ts.GENERIC_CASES[-1], ts.BRANCH_CASES[0])] == [7, 34007, 35007]   # old seeds kept


@pytest.mark.parametrize('case', HOST_CASES, ids=ts.case_id)
def test_steered_inputs_have_the_masks_they_claim(case):
    mode, dims_name, spec, L = case
    B = ts.batch_of(spec, N_TEAMS)
    dims = ts.dims_of(dims_name)
    st = ts.steered(mode, B, L, ts.case_seed(case), dims)
    H, FC, A = dims['rnn_dims'], dims['fc_dims'], dims['res_out_dims'] // 4
    assert st['aux'].dtype == st['mels_up'].dtype == st['x'].dtype == np.float32 and all(v.dtype == np.float32 for v in st['sd'].values())
    assert st['aux'].shape == (B, L, 4 * A) and st['mask1'].shape == st['mask2'].shape == (B, L, FC)
    assert set(np.unique(st['aux'][:, :, 2 * A])) <= {-1.0, 1.0} and set(np.unique(st['aux'][:, :, 3 * A])) <= {-1.0, 1.0}
    assert np.all(np.abs(st['sd']['fc1.weight'][:, H]) == np.float32(st['c1'])) and np.all(np.abs(st['sd']['fc2.weight'][:, FC]) == np.float32(st['c2']))
    for p, mask in zip(ts.pre_activations64(st), (st['mask1'], st['mask2'])):
        assert np.abs(p).min() >= ts.MARGIN, float(np.abs(p).min())
        assert np.array_equal(p > 0, mask)
        assert 0.4 <= mask.mean() <= 0.6
        assert (mask != mask[:, :, :1]).any()                          # along the units
        assert L == 1 or (mask != mask[:, :1, :]).any()               # along the steps
        assert B == 1 or (mask != mask[:1, :, :]).any()               # along the rows
    r64 = ts.reference(st, mode)
    assert np.isfinite(r64['loss']) and all(np.isfinite(g).all() and np.abs(g).max() > 0 for k, g in r64['grads'].items()
                                            if L > 1 or 'weight_hh' not in k)
    if L == 1:   # h_{-1} = 0: nothing reaches the recurrent weights
        assert not r64['grads']['rnn1.weight_hh_l0'].any() and not r64['grads']['rnn2.weight_hh_l0'].any()
    if mode == 'RAW':
        r32 = ts.reference(st, mode, dtype=torch.float32)
        worst, where, row_worst = ts.worst_errors(r32['grads'], r64['grads'])
        print(f'\n[steer {ts.case_id(case)}] B={B} c1={st["c1"]:.2f} c2={st["c2"]:.2f}: torch float32 vs float64 {worst:.2e} ({where}), '
              f'per row of d_mels_up / d_aux {row_worst:.2e}')
        assert worst <= 2e-6, (where, worst)
