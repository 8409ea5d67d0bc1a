"""The block-sparse weight image of WRNN_KERNEL_TEAMG / WRNN_KERNEL_TEAMG_BATCH (`teamg_sparse = True`).

A block is 64 consecutive elements of one padded image row.  The sparse instantiations leave out the steps of a row's dot product whose 64
weights are all zero and keep the others in ascending order; fmaf(0, x, a) == a for finite x, so every lane's chain of multiply-adds is
the dense fp32 kernel's.  Hence the one rule of this file: with the setting on, labels, samples and logits are `assert_array_equal` to
the SAME model with the setting off on the fp32 image -- for pruned models, for an unpruned one, for an irregular pattern, under every
placement, on both kernels.  No tolerance anywhere.

Call shapes, seeds and helpers are those of tests/test_gpu_teamg_e4m3.py (Philox noise, `want_logits=True`), three rows.
"""
import numpy as np
import pytest
import torch

from tests.teamg_cases import DIM_SETS

pytestmark = pytest.mark.gpu

FRAMES = {'A': 1, 'B': 20, 'C': 20, 'D': 1}      # A: 128 steps, B and C: 120, D: 275
ROWS = 3
SEED = 0x5EED5
DENSITY = 0.25

_STATE, _MODELS, _REF = {}, {}, {}


def _dims(name, mode):
    d = dict(DIM_SETS[name])
    if mode == 'MOL' and name == 'D':
        d['bits'] = 9
    return d


def _prune(sd, density):
    """sd (numpy) with sparsity.block_masks applied at `density`."""
    from tacotronv2_wavernn_chinese_amd.sparsity import block_masks
    sd = {k: np.array(v) for k, v in sd.items()}
    for k, m in block_masks({k: torch.from_numpy(v) for k, v in sd.items()}, density).items():
        sd[k][~m.numpy()] = 0.0
    return sd


def _dense_state(name, mode='RAW'):
    key = (name, mode)
    if key not in _STATE:
        from tacotronv2_wavernn_chinese_amd.synth import make_state_dict
        _STATE[key] = make_state_dict(7, mode, 'peaky' if mode == 'RAW' else 'default', **_dims(name, mode))
    return _STATE[key]


def _new_model(name, mode, sd, sparse=False):
    from tacotronv2_wavernn_chinese_amd.vocoder import WaveRNN
    m = WaveRNN(**_dims(name, mode), mode=mode)
    m.verbose = False
    m.teamg_sparse = sparse
    m.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in sd.items()})
    m.to('cuda:0')
    return m


def _pruned_model(name, mode='RAW'):
    """The model of set `name` pruned at DENSITY, once per module."""
    key = (name, mode)
    if key not in _MODELS:
        _MODELS[key] = _new_model(name, mode, _prune(_dense_state(name, mode), DENSITY))
    return _MODELS[key]


def _mels(name, seed=3, B=ROWS, T=None):
    from tacotronv2_wavernn_chinese_amd.synth import make_mels
    return make_mels(seed, B, FRAMES[name] if T is None else T, feat_dims=DIM_SETS[name]['feat_dims'])


def _call(m, sparse, mels, kernel='teamg', **kw):
    from tacotronv2_wavernn_chinese_amd import _cabi
    m.teamg_sparse = sparse
    kw.setdefault('noise_mode', 'philox')
    kw.setdefault('seed', SEED)
    kw.setdefault('want_logits', True)
    res = m.generate_raw(mels, False, 11000, 550, kernel=kernel, **kw)
    assert m.last_timing['kernel'] == _cabi.KERNEL_IDS[kernel]                 # no silent fallback
    assert m.last_timing['teamg_sparse'] is sparse and m.native().teamg_sparse is sparse and m.last_timing['teamg_weights'] == 'f32'
    if 'batch_rows' in kw:
        assert m.last_timing['batch_rows'] == kw['batch_rows']
    return {k: res[k].cpu().numpy() for k in ('labels', 'samples', 'logits')}


def _same(got, want, what):
    assert set(got) == set(want)
    for k in want:
        np.testing.assert_array_equal(got[k], want[k], err_msg=f'{what}: {k}')


def _batch_rows(name, mode):
    """Every rows-per-team count the plan admits for these dims."""
    from tacotronv2_wavernn_chinese_amd import _cabi
    out = []
    for r in (2, 4, 8):
        try:
            _cabi.teamg_batch_plan(r, -1, mode=mode, **_dims(name, mode))
            out.append(r)
        except _cabi.WrnnError:
            pass
    return out


def _sparse_against_dense(m, name, mode, what):
    """Sparse on, on teamg and on teamg_batch at every admitted batch_rows, against the same model with sparse off on teamg."""
    mels = _mels(name)
    want = _call(m, False, mels)
    assert want['labels'].shape == (ROWS, FRAMES[name] * DIM_SETS[name]['hop_length'])
    assert len({want['labels'][r].tobytes() for r in range(ROWS)}) == ROWS    # the rows are different signals: equality is not vacuous
    _same(_call(m, True, mels), want, f'{what}: teamg, sparse on against off')
    rows = _batch_rows(name, mode)
    assert rows
    for r in rows:
        _same(_call(m, True, mels, 'teamg_batch', batch_rows=r), want, f'{what}: teamg_batch, {r} rows per team, sparse on against teamg off')
    return want


def _census(sd, mode, name):
    """NumPy census of a state dict: layer -> dict(kept, dense, nb_a, nb_b), by the blocks of sparsity.block_layout."""
    from tacotronv2_wavernn_chinese_amd.sparsity import block_layout
    out = {}
    for layer, L in block_layout(_dims(name, mode), mode).items():
        counts = []
        for seg in L['segments']:
            w = np.asarray(sd[seg.tensor])[:, seg.col0:seg.col0 + seg.cols]
            wp = np.zeros((w.shape[0], seg.blocks * 64), w.dtype)
            wp[:, :seg.cols] = w
            counts.append((wp.reshape(w.shape[0], seg.blocks, 64) != 0).any(-1).sum(-1))
        out[layer] = dict(kept=int(sum(c.sum() for c in counts)), dense=L['rows'] * L['blocks'], nb_a=int(counts[0].max()),
                          nb_b=int(counts[1].max()) if len(counts) > 1 else 0)
    return out


# ---- 1. pruned models -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('name,mode', [(n, md) for n in 'ABD' for md in ('RAW', 'MOL')] + [('C', 'RAW')])
def test_a_pruned_model_runs_sparse_equal_to_dense(name, mode):
    m = _pruned_model(name, mode)
    _sparse_against_dense(m, name, mode, f'set {name} {mode} pruned at {DENSITY}')
    info = m.native().teamg_sparse_info()
    want = _census({k: v.cpu().numpy() for k, v in m.state_dict().items()}, mode, name)
    assert info['layers'] == want
    for layer in ('rnn1', 'rnn2', 'fc1', 'fc2'):
        assert info['layers'][layer]['kept'] < info['layers'][layer]['dense']
    print(f"\n[sparse {name} {mode}] kept {info['kept']} of {info['dense']} blocks, streamed {info['plan']['streamed_bytes_step']} bytes per step")


# ---- 2. an unpruned model: full rows and the padding tail -------------------------------------------------------------------------------

@pytest.mark.parametrize('name', ['B', 'A'])
def test_an_unpruned_model_runs_sparse_equal_to_dense(name):
    m = _new_model(name, 'RAW', _dense_state(name))
    _sparse_against_dense(m, name, 'RAW', f'set {name} unpruned')
    info = m.native().teamg_sparse_info()
    assert info['kept'] == info['dense']                                       # every block of these models holds a weight


# ---- 3. an irregular pattern ------------------------------------------------------------------------------------------------------------

def _irregular_state():
    from tacotronv2_wavernn_chinese_amd.sparsity import block_layout
    sd = {k: np.array(v) for k, v in _dense_state('B').items()}
    rng = np.random.Generator(np.random.PCG64(17))
    H = DIM_SETS['B']['rnn_dims']
    for layer, L in block_layout(DIM_SETS['B']).items():                       # a random block mask, every layer
        for seg in L['segments']:
            drop = rng.random((L['rows'], seg.blocks)) < 0.5
            cols = np.repeat(drop, 64, axis=1)[:, :seg.cols]
            sd[seg.tensor][:, seg.col0:seg.col0 + seg.cols][cols] = 0.0
    fresh = _dense_state('B')
    sd['rnn1.weight_ih_l0'][0, :] = 0.0                                         # a row with no kept block in segment A ...
    sd['rnn1.weight_hh_l0'][0, :] = fresh['rnn1.weight_hh_l0'][0, :]
    sd['rnn1.weight_hh_l0'][1, :] = 0.0                                         # ... and one with none in segment B
    sd['rnn1.weight_ih_l0'][1, :] = fresh['rnn1.weight_ih_l0'][1, :]
    sd['fc1.weight'][:] = 0.0                                                   # a layer entirely zero
    for gate, keep in enumerate(((0,), (1,), (0, 1))):                          # the gate rows of unit 2 of rnn2 with different lists
        row = gate * H + 2
        sd['rnn2.weight_ih_l0'][row, :] = 0.0
        for b in keep:
            sd['rnn2.weight_ih_l0'][row, 64 * b:64 * b + 64] = fresh['rnn2.weight_ih_l0'][row, 64 * b:64 * b + 64]
    sd['fc2.weight'][3, :] = 0.0                                                # a kept block holding a single non-zero weight
    sd['fc2.weight'][3, 64 + 5] = 0.37
    return sd


def test_an_irregular_pattern_runs_equal_to_dense_and_the_census_is_numpys():
    sd = _irregular_state()
    m = _new_model('B', 'RAW', sd)
    _sparse_against_dense(m, 'B', 'RAW', 'set B, irregular pattern')
    info = m.native().teamg_sparse_info()
    want = _census(sd, 'RAW', 'B')
    assert info['layers'] == want
    assert want['fc1'] == dict(kept=0, dense=want['fc1']['dense'], nb_a=0, nb_b=0)
    assert info['kept'] == sum(v['kept'] for v in want.values()) < info['dense']
    p = info['plan']
    for L in p['layers'].values():
        assert L['resident_bytes_team'] + L['streamed_bytes_step'] == L['weight_bytes']


# ---- 4. placements --------------------------------------------------------------------------------------------------------------------

def test_sparse_runs_equal_to_dense_under_every_placement():
    from tacotronv2_wavernn_chinese_amd import _cabi
    m = _pruned_model('B')
    mels = _mels('B')
    want = _call(m, False, mels)
    _same(_call(m, True, mels), want, 'set B pruned, default placement')
    nat = m.native()
    info = nat.teamg_sparse_info()
    nb_a = [info['layers'][n]['nb_a'] for n in _cabi.TEAMG_LAYER_NAMES]
    nb_b = [info['layers'][n]['nb_b'] for n in _cabi.TEAMG_LAYER_NAMES]
    L = info['plan']['layers']
    unit = lambda n: 4 * L[n]['rows_per_unit'] * ((info['layers'][n]['nb_a'] + info['layers'][n]['nb_b'] + 7) // 8 * 4 + 64 * (info['layers'][n]['nb_a'] + info['layers'][n]['nb_b']))
    assert all(L[n]['resident_units'] == max(L[n]['own_count']) for n in L)   # default: set B is resident
    half = sum(max(L[n]['own_count']) * unit(n) for n in ('fc3', 'fc2', 'fc1')) + max(L['rnn2']['own_count']) // 2 * unit('rnn2')
    dims = dict(mode='RAW', **_dims('B', 'RAW'))
    p = _cabi.teamg_sparse_plan(1, nb_a, nb_b, half, **dims)
    assert 0 < p['layers']['rnn2']['resident_units'] < max(L['rnn2']['own_count']) and p['layers']['rnn1']['resident_units'] == 0
    try:
        for budget in (0, half):
            nat.debug_teamg_lds_budget(budget)
            _same(_call(m, True, mels), want, f'set B pruned, teamg, LDS budget {budget}')
            got_plan = nat.teamg_sparse_info()['plan']
            assert got_plan['lds_budget_bytes'] == budget
            assert got_plan['layers']['rnn2']['resident_units'] == (0 if budget == 0 else p['layers']['rnn2']['resident_units'])
            _same(_call(m, True, mels, 'teamg_batch', batch_rows=2), want, f'set B pruned, teamg_batch, LDS budget {budget}')
    finally:
        nat.debug_teamg_lds_budget(-1)


# ---- 5. switching and reloading -----------------------------------------------------------------------------------------------------------

def test_switching_reloading_and_in_place_edits():
    from tacotronv2_wavernn_chinese_amd import _cabi
    sd = _prune(_dense_state('B'), DENSITY)
    m = _new_model('B', 'RAW', sd)
    mels = _mels('B')
    simple_before = _call(m, False, mels, 'simple')
    on = _call(m, True, mels)
    off = _call(m, False, mels)
    _same(on, off, 'on against off')
    _same(_call(m, True, mels), on, 'on -> off -> on')
    _same(_call(m, True, mels, 'simple'), simple_before, "kernel='simple' does not read the setting")
    assert m.last_timing['kernel'] == _cabi.KERNEL_SIMPLE
    # load_state_dict of a model with another pattern: the setting stays, the image follows
    other = _irregular_state()
    m.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in other.items()})
    assert m.teamg_sparse is True
    got = _call(m, True, mels)
    assert m.native().teamg_sparse_info()['layers'] == _census(other, 'RAW', 'B')
    _same(got, _call(_new_model('B', 'RAW', other), False, mels), 'after load_state_dict, against a fresh model with sparse off')
    # an in-place edit that turns a zero block non-zero is picked up
    before = m.native().teamg_sparse_info()['layers']['fc1']
    assert before['kept'] == 0
    with torch.no_grad():
        m.fc1.weight[5, 70] += 0.25
    got = _call(m, True, mels)
    after = m.native().teamg_sparse_info()['layers']['fc1']
    assert after['kept'] == 1 and after['nb_a'] == 1
    edited = {k: np.array(v) for k, v in other.items()}
    edited['fc1.weight'][5, 70] += np.float32(0.25)
    _same(got, _call(_new_model('B', 'RAW', edited), False, mels), 'after the in-place edit, against a fresh model with sparse off')


# ---- 6. refusals ----------------------------------------------------------------------------------------------------------------------

def test_sparse_with_f16_or_e4m3_is_refused_and_info_needs_a_pack():
    from tacotronv2_wavernn_chinese_amd import _cabi
    m = _new_model('B', 'RAW', _prune(_dense_state('B'), DENSITY), sparse=True)
    mels = _mels('B')
    with pytest.raises(_cabi.WrnnError) as ei:
        m.native().teamg_sparse_info()                                         # before any call
    assert ei.value.code == _cabi.ERR_STATE
    for fmt in ('f16', 'e4m3'):
        m.teamg_weights = fmt
        for kernel, kw in (('teamg', {}), ('teamg_batch', dict(batch_rows=2))):
            with pytest.raises(_cabi.WrnnError) as ei:
                m.generate_raw(mels, False, 11000, 550, kernel=kernel, noise_mode='philox', seed=SEED, **kw)
            assert ei.value.code == _cabi.ERR_UNSUPPORTED and 'sparse' in str(ei.value) and fmt.upper() in str(ei.value)
    m.teamg_weights = 'f32'
    got = _call(m, True, mels)
    _same(got, _call(m, False, mels), 'after teamg_weights = f32')
    m.teamg_sparse = True
    m.teamg_weights = 'f16'
    with pytest.raises(_cabi.WrnnError):
        m.generate_raw(mels, False, 11000, 550, kernel='teamg', noise_mode='philox', seed=SEED)
    m.teamg_sparse = False                                                     # resetting the other setting works too
    m.generate_raw(mels, False, 11000, 550, kernel='teamg', noise_mode='philox', seed=SEED)
    assert m.last_timing['teamg_weights'] == 'f16' and m.last_timing['teamg_sparse'] is False


# ---- 7. training ----------------------------------------------------------------------------------------------------------------------

def _train(tmp_path, tag, **kw):
    from tacotronv2_wavernn_chinese_amd import train as T
    from tacotronv2_wavernn_chinese_amd.vocoder import WaveRNN
    d = DIM_SETS['A']
    torch.manual_seed(0)
    m = WaveRNN(**d, mode='RAW')
    m.verbose = False
    m.to('cuda:0')
    opt = torch.optim.Adam(m.parameters())
    paths = T.VocPaths(tmp_path / tag)
    T.restore_checkpoint(paths, m, opt, create_if_missing=True)
    pairs = T.synthetic_pairs(6, 14, bits=d['bits'], n_mels=d['feat_dims'], hop_length=d['hop_length'], seed=11)
    loader = T.WindowLoader(pairs, 2, seed=1, mode='RAW', bits=d['bits'], hop_length=d['hop_length'], pad=d['pad'], seq_len=2 * d['hop_length'])
    losses = T.voc_train_loop(paths, m, None, opt, loader, None, 1e-4, 5, checkpoint_every=1000, **kw)
    assert len(losses) == 6 and m.get_step() == 6
    return m, paths, losses


def test_training_with_a_schedule_leaves_pruned_checkpoints_that_run_sparse(tmp_path):
    from tacotronv2_wavernn_chinese_amd.sparsity import SparsitySchedule, block_layout, kept_blocks
    from tacotronv2_wavernn_chinese_amd.vocoder import WaveRNN
    plain = _train(tmp_path, 'plain')[2]
    none = _train(tmp_path, 'none', sparsify=None)[2]
    assert none == plain                                                       # sparsify=None: the loop as it was
    m, paths, losses = _train(tmp_path, 'sparse', sparsify=SparsitySchedule(0.25, start=1, end=4, every=1))
    assert np.isfinite(losses).all()
    ckpt = torch.load(paths.voc_latest_weights, map_location='cpu')
    layout = block_layout(DIM_SETS['A'])
    for layer in ('rnn1', 'rnn2', 'fc1', 'fc2'):
        for seg in layout[layer]['segments']:
            w = ckpt[seg.tensor].numpy()[:, seg.col0:seg.col0 + seg.cols]
            wp = np.zeros((w.shape[0], seg.blocks * 64), np.float32)
            wp[:, :seg.cols] = w
            nz = (wp.reshape(w.shape[0], seg.blocks, 64) != 0).any(-1)
            # kept counts equal the target in every row; what is not kept is exactly zero (nz is False only for all-zero blocks)
            np.testing.assert_array_equal(nz.sum(-1), kept_blocks(0.25, seg.blocks), err_msg=f'{seg.tensor}: kept blocks per row')
    for key in ('fc3.weight', 'I.weight'):
        assert (ckpt[key].numpy() != 0).all()                                  # never touched
    g = WaveRNN(**DIM_SETS['A'], mode='RAW')
    g.verbose = False
    g.load_state_dict(ckpt)
    g.to('cuda:0').eval()
    mels = _mels('A')
    want = _call(g, False, mels)
    _same(_call(g, True, mels), want, 'the pruned checkpoint, sparse on against off')
    info = g.native().teamg_sparse_info()['layers']
    assert info['rnn1']['nb_a'] == kept_blocks(0.25, 4) and info['rnn1']['nb_b'] == kept_blocks(0.25, 4)
