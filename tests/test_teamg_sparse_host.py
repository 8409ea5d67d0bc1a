"""Host side of the block-sparse weight image of WRNN_KERNEL_TEAMG / WRNN_KERNEL_TEAMG_BATCH: the new exports, the blocks
in model coordinates (`sparsity.block_layout`) against the dense plan, magnitude pruning in blocks (`sparsity.block_masks`) against a NumPy
sort written here, the plan of the sparse image (`wrnn_teamg_sparse_plan`, pure host code), the pruning schedule, the model property and
the two CLI flags.  No GPU."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest
import torch

from tests.teamg_cases import DIM_SETS, LDS_BYTES
from tests.test_teamg_host import CASES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ('wrnn_teamg_set_sparse', 'wrnn_teamg_sparse', 'wrnn_teamg_sparse_plan', 'wrnn_teamg_sparse_info')


def _dims(name, mode):
    d = dict(DIM_SETS[name])
    if mode == 'MOL' and name == 'D':
        d['bits'] = 9
    return d


def _full_counts(name, mode):
    """(nb_a, nb_b) of the dense rows, in the order of _cabi.TEAMG_LAYER_NAMES."""
    from tacotronv2_wavernn_chinese_amd import _cabi
    from tacotronv2_wavernn_chinese_amd.sparsity import block_layout
    lay = block_layout(_dims(name, mode), mode)
    segs = [lay[n]['segments'] for n in _cabi.TEAMG_LAYER_NAMES]
    return [s[0].blocks for s in segs], [s[1].blocks if len(s) > 1 else 0 for s in segs]


def _row_bytes(nb):
    """An image row: 16-bit indices padded to 16 bytes, then the blocks of 64 floats."""
    return (2 * nb + 15) // 16 * 16 + 256 * nb


def test_the_new_symbols_are_exported_and_declared_and_the_abi_stays_9():
    from tacotronv2_wavernn_chinese_amd import _cabi
    lib = _cabi.load_library()
    hdr = open(os.path.join(ROOT, 'include', 'wavernn_amd.h')).read()
    for s in NEW:
        assert re.fullmatch(r'wrnn_[a-z_]+', s)
        assert s in _cabi.EXPORTED_SYMBOLS and hasattr(lib, s) and re.search(rf'\b{s}\s*\(', hdr), s
    assert _cabi.ABI_VERSION == 9 and int(re.search(r'#define WRNN_ABI_VERSION (\d+)', hdr).group(1)) == 9 == lib.wrnn_abi_version()
    assert _cabi.WEIGHT_FORMATS == {'f32': 0, 'f16': 1}
    assert _cabi.TEAMG_WEIGHT_FORMATS == {'f32': 0, 'f16': 1, 'e4m3': 3}       # sparsity is a setting of its own, not a format
    assert _cabi.TEAMG_WEIGHT_FORMAT_NAMES == {0: 'f32', 1: 'f16', 3: 'e4m3'}
    assert C.sizeof(_cabi.SampleOpts) == 88
    assert lib.wrnn_teamg_set_sparse(None, 1) == _cabi.ERR_INVALID and lib.wrnn_teamg_sparse(None) == 0
    assert lib.wrnn_teamg_sparse_info(None, None, None, None, None, None) == _cabi.ERR_INVALID


@pytest.mark.parametrize('name,mode', CASES)
def test_block_layout_counts_are_the_dense_plans(name, mode):
    from tacotronv2_wavernn_chinese_amd import _cabi
    from tacotronv2_wavernn_chinese_amd.sparsity import LAYERS, block_layout
    assert LAYERS == _cabi.TEAMG_LAYER_NAMES
    lay = block_layout(_dims(name, mode), mode)
    p = _cabi.teamg_plan(-1, mode=mode, **_dims(name, mode))
    assert set(lay) == set(p['layers'])
    for lname, L in p['layers'].items():
        assert lay[lname]['blocks'] * 64 == L['k_padded']
        assert lay[lname]['rows'] == L['units'] * L['rows_per_unit']
        assert sum(s.cols for s in lay[lname]['segments']) == L['k']
        assert lay[lname]['blocks'] == sum(-(-s.cols // 64) for s in lay[lname]['segments'])
        assert len(lay[lname]['segments']) == (2 if lname.startswith('rnn') else 1)
    assert lay['cond']['segments'][0].col0 == 1 and all(s.col0 == 0 for n in lay if n != 'cond' for s in lay[n]['segments'])
    with pytest.raises(ValueError):
        block_layout(_dims(name, mode), 'raw')


def _state(name):
    from tacotronv2_wavernn_chinese_amd.synth import make_state_dict
    return {k: torch.from_numpy(np.array(v)) for k, v in make_state_dict(7, 'RAW', 'peaky', **DIM_SETS[name]).items()}


@pytest.mark.parametrize('name', ['B', 'A'])
@pytest.mark.parametrize('density', [0.25, 0.5, 0.3])
def test_block_masks_keep_the_largest_blocks_of_every_row(name, density):
    """Set B: rnn 100, K = 100 pads to 128, the second block of a row is part padding (36 weights)."""
    from tacotronv2_wavernn_chinese_amd.sparsity import block_layout, block_masks
    sd = _state(name)
    masks = block_masks(sd, density)
    lay = block_layout(DIM_SETS[name])
    assert set(masks) == {s.tensor for n in ('rnn1', 'rnn2', 'fc1', 'fc2') for s in lay[n]['segments']}
    for lname in ('rnn1', 'rnn2', 'fc1', 'fc2'):
        for seg in lay[lname]['segments']:
            w = sd[seg.tensor].numpy()[:, seg.col0:seg.col0 + seg.cols].astype(np.float64)
            m = masks[seg.tensor].numpy()
            assert m.shape == sd[seg.tensor].shape and m.dtype == np.bool_
            wp = np.zeros((w.shape[0], seg.blocks * 64))
            wp[:, :seg.cols] = w
            norms = (wp.reshape(w.shape[0], seg.blocks, 64) ** 2).sum(-1)
            n_keep = math.ceil(density * seg.blocks)
            order = np.argsort(-norms, axis=1, kind='stable')                   # largest first, ties to the lower index
            want = np.zeros((w.shape[0], seg.blocks), bool)
            np.put_along_axis(want, order[:, :n_keep], True, axis=1)
            got = np.zeros((w.shape[0], seg.blocks * 64), bool)
            got[:, :seg.cols] = m[:, seg.col0:seg.col0 + seg.cols]
            got = got.reshape(w.shape[0], seg.blocks, 64)
            np.testing.assert_array_equal(got.any(-1), want, err_msg=f'{seg.tensor}: kept blocks')
            np.testing.assert_array_equal(got.any(-1).sum(-1), n_keep)
            cols_of = np.minimum(64, seg.cols - 64 * np.arange(seg.blocks))     # a kept block is kept whole
            np.testing.assert_array_equal(got.sum(-1), want * cols_of[None, :])


def test_block_masks_apply_is_idempotent_and_touches_nothing_else():
    from tacotronv2_wavernn_chinese_amd.sparsity import apply_masks_, block_masks
    from tacotronv2_wavernn_chinese_amd.vocoder import WaveRNN
    m = WaveRNN(**DIM_SETS['B'], mode='RAW')
    m.load_state_dict(_state('B'))
    before = {k: v.clone() for k, v in m.state_dict().items()}
    assert all(bool(v.all()) for v in block_masks(m, 1).values()) and all(bool(v.all()) for v in block_masks(m, 1.0).values())   # density 1: the identity
    masks = block_masks(m, 0.25)
    assert apply_masks_(m, masks) is m
    once = {k: v.clone() for k, v in m.state_dict().items()}
    for k, v in once.items():
        if k in masks:
            assert torch.equal(v[masks[k]], before[k][masks[k]]) and not bool(v[~masks[k]].any()) and bool((~masks[k]).any())
        else:
            assert torch.equal(v, before[k]), k                                 # biases, I.weight, fc3, the upsample network: bit-equal
    assert 'I.weight' not in masks and 'fc3.weight' not in masks
    again = block_masks(m, 0.25)
    apply_masks_(m, again)
    for k, v in m.state_dict().items():
        assert torch.equal(v, once[k]), k
    for k in masks:
        assert torch.equal(again[k], masks[k])
    # a state dict works as a model does; the sample's column of I is never masked
    mi = block_masks(_state('B'), 0.5, layers=('cond',))
    assert set(mi) == {'I.weight'} and bool(mi['I.weight'][:, 0].all())
    # earlier masks stay: a pruned block stays pruned
    narrower = block_masks(m, 0.5, keep=masks)
    for k in masks:
        assert not bool((narrower[k] & ~masks[k]).any())
    for bad in (0, 0.0, -0.1, 1.01, 2, None, 'half', True):
        with pytest.raises(ValueError):
            block_masks(m, bad)
    with pytest.raises(ValueError):
        block_masks(m, 0.5, layers=('rnn3',))


@pytest.mark.parametrize('name,mode', CASES)
def test_sparse_plan_with_full_counts_is_the_dense_plan_apart_from_the_index_bytes(name, mode):
    from tacotronv2_wavernn_chinese_amd import _cabi
    dims = dict(mode=mode, **_dims(name, mode))
    nb_a, nb_b = _full_counts(name, mode)
    for rows in (1, 2):
        for budget in (-1, 0, 4096, 40000, 10 ** 9):
            try:
                dense = _cabi.teamg_batch_plan(rows, budget, **dims)
            except _cabi.WrnnError:
                with pytest.raises(_cabi.WrnnError):
                    _cabi.teamg_sparse_plan(rows, nb_a, nb_b, budget, **dims)
                continue
            sp = _cabi.teamg_sparse_plan(rows, nb_a, nb_b, budget, **dims)
            for f in ('activation_bytes', 'mail_granules', 'lds_budget_bytes'):
                assert sp[f] == dense[f]
            assert sp['lds_bytes'] <= LDS_BYTES and sp['lds_bytes'] == sp['activation_bytes'] + sum(L['lds_bytes'] for L in sp['layers'].values())
            assert sp['streamed_bytes_step'] == sum(L['streamed_bytes_step'] for L in sp['layers'].values())
            left, filled = sp['lds_budget_bytes'], True
            for i, lname in enumerate(_cabi.TEAMG_LAYER_NAMES):
                a, b = sp['layers'][lname], dense['layers'][lname]
                for f in ('units', 'rows_per_unit', 'k', 'k_padded', 'own_first', 'own_count', 'rows_min', 'rows_max'):
                    assert a[f] == b[f], (lname, f)
                # the placement rule of the dense plan with the sparse unit: whole units in layer order, the first layer that does not
                # fit whole is the last to get any
                unit = a['rows_per_unit'] * _row_bytes(nb_a[i] + nb_b[i])
                assert unit == a['rows_per_unit'] * (4 * a['k_padded'] + (2 * a['k_padded'] // 64 + 15) // 16 * 16)   # the dense unit + its index lists
                U = max(a['own_count'])
                want = min(U, left // unit) if filled else 0
                assert a['resident_units'] == want <= b['resident_units'], (lname, budget)
                left -= want * unit
                filled = filled and want == U
                assert a['lds_bytes'] == want * unit
                assert a['weight_bytes'] == a['units'] * unit
                assert a['resident_bytes_team'] + a['streamed_bytes_step'] == a['weight_bytes']
                assert a['resident_bytes_team'] == sum(min(n, want) for n in a['own_count']) * unit


@pytest.mark.parametrize('name,mode', CASES)
def test_fewer_blocks_never_lower_residency_nor_raise_the_streamed_bytes(name, mode):
    from tacotronv2_wavernn_chinese_amd import _cabi
    dims = dict(mode=mode, **_dims(name, mode))
    full_a, full_b = _full_counts(name, mode)
    for budget in (-1, 40000):
        prev = None
        for den in (1, 2, 4, 8, 16):
            nb_a, nb_b = [-(-v // den) for v in full_a], [-(-v // den) for v in full_b]
            p = _cabi.teamg_sparse_plan(1, nb_a, nb_b, budget, **dims)
            for L in p['layers'].values():
                assert L['resident_bytes_team'] + L['streamed_bytes_step'] == L['weight_bytes']
            if prev is not None:
                for lname in p['layers']:
                    assert p['layers'][lname]['resident_units'] >= prev['layers'][lname]['resident_units'], (lname, den)
                    assert p['layers'][lname]['streamed_bytes_step'] <= prev['layers'][lname]['streamed_bytes_step'], (lname, den)
                assert p['streamed_bytes_step'] <= prev['streamed_bytes_step']
            prev = p
    # a layer with no block at all takes no room and streams nothing
    z = _cabi.teamg_sparse_plan(1, [0] * 6, [0] * 6, -1, **dims)
    assert z['streamed_bytes_step'] == 0 and z['lds_bytes'] == z['activation_bytes']


def test_set_c_at_a_sixteenth_streams_little(capsys):
    from tacotronv2_wavernn_chinese_amd import _cabi
    dims = dict(mode='RAW', **DIM_SETS['C'])
    full_a, full_b = _full_counts('C', 'RAW')
    dense = _cabi.teamg_plan_fmt(1, 'f32', -1, **dims)
    p = _cabi.teamg_sparse_plan(1, [-(-v // 16) for v in full_a], [-(-v // 16) for v in full_b], -1, **dims)
    with capsys.disabled():
        print(f"\n[set C at 1/16] image {sum(L['weight_bytes'] for L in p['layers'].values())} bytes, streamed per step {p['streamed_bytes_step']} "
              f"(dense fp32 plan: {dense['streamed_bytes_step']})")
    assert p['streamed_bytes_step'] < dense['streamed_bytes_step'] / 8


def test_a_count_above_the_dense_rows_is_invalid():
    from tacotronv2_wavernn_chinese_amd import _cabi
    dims = dict(mode='RAW', **DIM_SETS['B'])
    full_a, full_b = _full_counts('B', 'RAW')
    _cabi.teamg_sparse_plan(1, full_a, full_b, -1, **dims)
    for i in range(6):
        for which in (0, 1):
            nb = [list(full_a), list(full_b)]
            nb[which][i] += 1
            with pytest.raises(_cabi.WrnnError) as ei:
                _cabi.teamg_sparse_plan(1, nb[0], nb[1], -1, **dims)
            assert ei.value.code == _cabi.ERR_INVALID
    with pytest.raises(_cabi.WrnnError) as ei:
        _cabi.teamg_sparse_plan(1, [-1] + full_a[1:], full_b, -1, **dims)
    assert ei.value.code == _cabi.ERR_INVALID
    with pytest.raises(_cabi.WrnnError) as ei:
        _cabi.teamg_sparse_plan(9, full_a, full_b, -1, **dims)
    assert ei.value.code == _cabi.ERR_INVALID


def test_sparsity_schedule_is_the_cubic_ramp():
    from tacotronv2_wavernn_chinese_amd.sparsity import SparsitySchedule
    s = SparsitySchedule(0.1, start=1000, end=3000, every=500)
    assert s.pruned_share(0) == 0.0 and s.pruned_share(999) == 0.0 and s.density(999) == 1.0
    assert s.pruned_share(1000) == 0.0                                          # the ramp starts at nothing pruned
    assert s.pruned_share(2000) == pytest.approx(0.9 * (1 - 0.5 ** 3))          # the middle: 7/8 of the way
    assert s.pruned_share(3000) == pytest.approx(0.9) and s.density(3000) == pytest.approx(0.1)
    assert s.pruned_share(10 ** 6) == pytest.approx(0.9)
    shares = [s.pruned_share(t) for t in range(900, 3200, 50)]
    assert shares == sorted(shares)
    assert [t for t in range(0, 4000, 250) if s.due(t)] == [1000, 1500, 2000, 2500, 3000]
    assert SparsitySchedule(0.5, 0, 10, every=4).due(10) and not SparsitySchedule(0.5, 0, 10, every=4).due(9)   # the end is always evaluated
    assert s.layers == ('rnn1', 'rnn2', 'fc1', 'fc2')
    for bad in (dict(target_density=0.0), dict(target_density=1.5), dict(start=5, end=4), dict(every=0), dict(start=-1)):
        with pytest.raises(ValueError):
            SparsitySchedule(**dict(dict(target_density=0.25, start=1, end=4, every=1), **bad))


def test_model_property_validates_without_a_device():
    from tacotronv2_wavernn_chinese_amd.vocoder import WaveRNN
    m = WaveRNN(**DIM_SETS['B'], mode='RAW')
    assert m.teamg_sparse is False
    m.teamg_sparse = True
    assert m.teamg_sparse is True
    for bad in (1, 0, 'on', None, 0.5, np.bool_(True)):
        with pytest.raises(ValueError):
            m.teamg_sparse = bad
    assert m.teamg_sparse is True and m.teamg_weights == 'f32'
    m.teamg_sparse = False
    assert m.teamg_sparse is False


def test_cli_flags():
    from tacotronv2_wavernn_chinese_amd import gen, train
    p = gen.build_parser()
    assert p.parse_args([]).teamg_sparse is False
    assert p.parse_args(['--kernel', 'teamg', '--teamg-sparse']).teamg_sparse is True
    assert p.parse_args(['--teamg-sparse']).kernel == 'auto'                    # accepted with any kernel, like --teamg-weights
    t = train.build_parser()
    a = t.parse_args([])
    assert a.sparse_density is None and train.sparsity_schedule(a) is None
    a = t.parse_args(['--sparse-density', '0.1', '--sparse-start', '1000', '--sparse-end', '200000'])
    s = train.sparsity_schedule(a)
    assert (s.target_density, s.start, s.end, s.every) == (0.1, 1000, 200000, 100)
    a = t.parse_args(['--sparse-density', '0.25', '--sparse-start', '1', '--sparse-end', '4', '--sparse-every', '1'])
    assert train.sparsity_schedule(a).every == 1
    for half in (['--sparse-density', '0.1'], ['--sparse-density', '0.1', '--sparse-start', '5'], ['--sparse-start', '5', '--sparse-end', '9']):
        with pytest.raises(ValueError):
            train.sparsity_schedule(t.parse_args(half))
    with pytest.raises(ValueError):
        train.sparsity_schedule(t.parse_args(['--sparse-density', '1.5', '--sparse-start', '1', '--sparse-end', '4']))
    for tool in ('any_dims_latency.py', 'any_dims_batch_latency.py'):
        assert '--sparse' in open(os.path.join(ROOT, 'tools', tool)).read(), tool
