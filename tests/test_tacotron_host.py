"""CPU checks of the Tacotron restatement (tests/tacotron_ref.py) on cases small enough to do by hand, of the text front end, of the
binding's structs, and the qualification of every fixture the GPU tests use: each discrete decision of its float64 run (is the largest
forward alignment at an index <= the previous max_attentions; each stop comparison; each dropout keep) leads by at least 1000 g, g the
largest |float32 restatement - float64 restatement| of the quantity the decision rests on."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tacotronv2_wavernn_chinese_amd import _cabi, tacotron
from tacotronv2_wavernn_chinese_amd.synth import make_tacotron_state
from tests import tacotron_fixtures as fx
from tests import tacotron_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_one_lstm_step_by_hand():
    """One unit, one input: z = [x; h] @ kernel + bias with the gates in the order i, j, f, o and 1.0 added to the forget gate."""
    kernel = np.array([[0.5, -1.0, 2.0, 0.25], [1.5, 0.5, -0.5, 1.0]])   # rows: x, h
    bias = np.array([0.1, 0.2, -0.3, 0.4])
    x, c, h = np.array([2.0]), np.array([0.7]), np.array([-0.4])
    i, j, f, o = 2.0 * 0.5 - 0.4 * 1.5 + 0.1, -2.0 - 0.2 + 0.2, 4.0 + 0.2 - 0.3, 0.5 - 0.4 + 0.4
    sg = lambda v: 1.0 / (1.0 + np.exp(-v))
    c_new = sg(f + 1.0) * 0.7 + sg(i) * np.tanh(j)
    h_new = sg(o) * np.tanh(c_new)
    got_c, got_h = ref.lstm_cell(x, c, h, kernel, bias)
    assert np.allclose([got_c[0], got_h[0]], [c_new, h_new], rtol=0, atol=1e-15)


def test_zoneout_output_is_unmixed_and_state_is_mixed():
    kernel = np.array([[0.5, -1.0, 2.0, 0.25], [1.5, 0.5, -0.5, 1.0]])
    bias = np.zeros(4)
    x, c, h = np.array([1.0]), np.array([0.3]), np.array([0.2])
    c_new, h_new = ref.lstm_cell(x, c, h, kernel, bias)
    out, c_state, h_state = ref.zoneout_lstm(x, c, h, kernel, bias, 0.1)
    assert out[0] == h_new[0]
    assert np.isclose(c_state[0], 0.9 * c_new[0] + 0.1 * 0.3, rtol=0, atol=1e-16)
    assert np.isclose(h_state[0], 0.9 * h_new[0] + 0.1 * 0.2, rtol=0, atol=1e-16)
    assert out[0] != h_state[0]


@pytest.mark.parametrize('T,k', [(1, 5), (2, 5), (4, 5), (3, 31), (3, 4)])
def test_conv_same_edges_shorter_than_the_kernel(T, k):
    """y[t] = sum_j x[t + j - (k - 1) // 2] w[j] with zeros outside 0 .. T - 1, written out element by element."""
    rng = np.random.Generator(np.random.PCG64(T * 100 + k))
    x, w = rng.standard_normal((T, 2)), rng.standard_normal((k, 2, 3))
    want = np.zeros((T, 3))
    for t in range(T):
        for j in range(k):
            u = t + j - (k - 1) // 2
            if 0 <= u < T:
                want[t] += x[u] @ w[j]
    assert np.allclose(ref.conv1d_same(x, w), want, rtol=0, atol=1e-14)


def _attention_weights(Tx, E2=3, A=2, D=2):
    """v_a = 0: every energy is 0, the softmax is flat, so the forward recursion alone decides the argmax."""
    rng = np.random.Generator(np.random.PCG64(5))
    w = {ref.LSA + 'query_layer/kernel': rng.standard_normal((D, A)), ref.LSA + 'location_features_convolution/kernel': rng.standard_normal((3, 1, 2)),
         ref.LSA + 'location_features_convolution/bias': np.zeros(2), ref.LSA + 'location_features_layer/kernel': rng.standard_normal((2, A)),
         ref.LSA + 'attention_variable_projection': np.zeros(A), ref.LSA + 'attention_bias': np.zeros(A),
         'decoder/dense/kernel': rng.standard_normal((E2 + D, 1)), 'decoder/dense/bias': np.zeros(1)}
    memory = rng.standard_normal((Tx, E2))
    return w, memory, memory @ rng.standard_normal((E2, A)), rng.standard_normal(D)


def _drive(Tx, at, mu, max_prev, pos_prev):
    """One attention step whose previous alignment is one-hot at ``at``: with a flat softmax the forward alignment is
    ((1 - mu) [t = at] + mu [t = at + 1] + 1e-10) / Tx, so mu = 0.1 puts the argmax at ``at`` and mu = 0.9 at ``at + 1``."""
    w, memory, keys, query = _attention_weights(Tx)
    alpha = np.zeros(Tx)
    alpha[at] = 1.0
    st = {'alpha': alpha, 'cum': alpha.copy(), 'mu': np.float64(mu), 'max_attentions': max_prev, 'pos_rec': pos_prev}
    return ref.attention_step(w, memory, keys, query, st, np.float64), memory


def test_every_arm_of_the_attention_window_block():
    Tx, seen = 8, set()
    # (previous one-hot, mu, max_prev, pos_prev) -> argmax, max_attentions, pos_rec, arms
    cases = [((0, 0.9, 0, 0), 1, 1, 1, {'advance'}),           # 1 > 0: advance; 1 is not beyond 2, so nothing holds it back
             ((1, 0.1, 1, 1), 1, 1, 2, {'stay'}),
             ((4, 0.9, 3, 2), 5, 3, 3, {'advance', 'hold'}),   # pos_rec 2 < 5 and 2 < 4: the advance is held back
             ((4, 0.9, 3, 6), 5, 4, 1, {'advance'}),           # pos_rec 6: the same advance goes through
             ((0, 0.1, 3, 9), 0, 4, 1, {'stay', 'push'}),      # the 10th step on one position pushes on
             ((2, 0.1, 6, 4), 2, 6, 5, {'stay'})]
    for (at, mu, mp, pp), am, m, pos, arms in cases:
        (a, new_mu, context, cum, got_m, got_pos, tr), memory = _drive(Tx, at, mu, mp, pp)
        assert (tr['argmax'], got_m, got_pos, set(tr['arm'])) == (am, m, pos, arms)
        seen |= set(tr['arm'])
        # the window [m - 2, m + 3), the doubled value at m, the renormalisation
        f = tr['forward']
        win = np.array([f[t] if m - 2 <= t < m + 3 else 0.0 for t in range(Tx)])
        S = win.sum() if win.sum() >= 1e-10 else 1.0
        win[min(m, Tx - 1)] = 2.0 * S
        assert np.allclose(a, win / win.sum(), rtol=0, atol=1e-16)
        assert np.all(a[:max(m - 2, 0)] == 0) and np.all(a[m + 3:] == 0)
        assert np.allclose(context, a @ memory, rtol=0, atol=1e-15)
        assert np.allclose(cum, tr['softmax'] + np.eye(Tx)[at], rtol=0, atol=1e-16) and np.allclose(tr['softmax'], 1.0 / Tx)
        assert 0.0 < new_mu < 1.0
    assert seen == {'stay', 'advance', 'hold', 'push'}


def test_attention_window_past_the_end_of_the_memory():
    """max_attentions keeps growing once pos_rec pushes it: beyond Tx + 1 the window is empty, its sum is replaced by 1 and index Tx - 1
    takes the doubled value, i.e. all of the alignment."""
    (a, _, context, _, m, pos, tr), memory = _drive(4, 3, 0.1, 6, 9)
    assert (m, pos) == (7, 1) and 'push' in tr['arm']
    assert np.array_equal(a, [0.0, 0.0, 0.0, 1.0]) and np.allclose(context, memory[3])
    (a, *_), _ = _drive(4, 3, 0.1, 4, 6)     # m = 4 = Tx: the window [2, 7) still holds rows 2 and 3, row Tx - 1 is the doubled one
    assert a[0] == a[1] == 0.0 and a[3] > a[2] >= 0.0 and np.isclose(a.sum(), 1.0)


def _small_decode(stop_bias, max_iters=4):
    dims = fx.SMALL
    state = {k: v.astype(np.float64) for k, v in make_tacotron_state(3, **dims).items()}
    sp = 'decoder/stop_token_projection/projection_stop_token_projection/'
    state[sp + 'kernel'] = np.zeros_like(state[sp + 'kernel'])
    state[sp + 'bias'] = np.full_like(state[sp + 'bias'], stop_bias)
    return fx.run_ref(state, dims, [3, 1, 4, 1, 5], np.float64, max_iters=max_iters, seed=1), state


def test_stop_at_exactly_one_half_does_not_stop():
    """round() is round-half-even: p = 0.5 rounds to 0, so only p > 0.5 stops."""
    res, _ = _small_decode(0.0)
    assert np.all(res['stop'] == 0.5) and res['steps'] == 4 and res['mel_length'] == 4 and res['mel'].shape == (4, 20)
    res, _ = _small_decode(1e-9)
    assert np.all(res['stop'] > 0.5) and res['steps'] == 1


def test_the_stopping_step_is_emitted_then_trimmed():
    """custom_decoder.step returns the outputs of the step together with `finished`, and dynamic_decode writes them before it looks at
    `finished`: the frame of the stopping step exists, the postnet sees it, and mel[:stop_token.index(1)] drops it."""
    res, state = _small_decode(1e-9)
    assert res['frames'].shape == (1, 20) and res['decoder_output'].shape == (1, 20) and res['mel_raw'].shape == (1, 20)
    assert res['mel_length'] == 0 and res['mel'].shape == (0, 20)
    w = {k: np.asarray(v) for k, v in state.items()}
    frames = np.linspace(-5, 5, 80).reshape(4, 20)
    out = ref.postprocess(w, frames, np.array([0.1, 0.2, 0.9, 0.3]), np.float64)
    assert out['mel_length'] == 2 and out['mel'].shape == (2, 20) and out['mel_raw'].shape == (4, 20)
    assert out['decoder_output'].min() == -4.1 and out['decoder_output'].max() == 4.0
    assert ref.postprocess(w, frames, np.array([0.1, 0.2, 0.5, 0.3]), np.float64)['mel_length'] == 4
    assert out['mel'].min() >= 0.0 and out['mel'].max() <= 1.0 and out['mel_raw'].min() >= -4.1


def test_text_to_sequence_and_symbols(tmp_path):
    p = tmp_path / 'train.txt'
    p.write_text('a.npy|b.npy|10|ni3 hao3 ,\nc.npy|d.npy|12|hao3 a5 .\n', encoding='utf-8')
    symbols = tacotron.load_symbols(str(p))
    assert symbols == ['_', '~', ',', '.', 'a5', 'hao3', 'ni3']
    assert tacotron.text_to_sequence('ni3 hao3 XX .', symbols) == [6, 5, 3, 1]      # the unknown token is dropped, EOS appended
    assert tacotron.text_to_sequence(['hao3'], symbols) == [5, 1]
    assert tacotron.text_to_sequence('', symbols) == [1]


def test_prenet_masks_restate_the_device_counter():
    """Layer l of step s reads wrnn_uniform(seed, s * layers + l, row 0, unit); no uniform is exactly 0.5 ((m + 0.5) 2^-23 never is), so a
    keep is decided by integers alone: its lead is not a matter of rounding."""
    from tests.philox_ref import philox_uniform_at
    masks, u = ref.prenet_masks(12345, 3, (5, 3))
    assert u.shape == (6, 5) and not np.any(u == np.float32(0.5))
    for s in range(3):
        for l, n in enumerate((5, 3)):
            want = philox_uniform_at(12345, [s * 2 + l], [0], n)[0, 0] >= np.float32(0.5)
            assert np.array_equal(masks[s][l], want)
    assert 0 < sum(int(m.sum()) for row in masks for m in row) < 24


@pytest.mark.parametrize('name', sorted(fx.FIXTURES))
def test_fixture_qualifies(name):
    f = fx.fixture(name)
    r64, r32, g, d = f['r64'], f['r32'], f['g'], f['full']
    r = d['outputs_per_step']
    for q in fx.INTS:
        assert np.array_equal(np.asarray(r64[q]), np.asarray(r32[q])), q
    assert all(np.isfinite(v) for v in g.values())
    assert len(f['leads']) >= (f['Tx'] > 1) * (r64['steps'] - 1)
    worst = None
    for kind, s, lead, q in f['leads']:
        assert lead >= fx.MARGIN * g[q], (kind, s, lead, g[q])
        worst = lead / g[q] if worst is None or (g[q] > 0 and lead / g[q] < worst) else worst
    print(f'{name}: {len(f["leads"])} decisions, smallest lead {worst:.3g} g' if worst is not None else f'{name}: no decisions')
    if f['dropout']:
        _, u = ref.prenet_masks(f['seed'], r64['steps'], tuple(d['prenet_layers']))
        assert not np.any(u == np.float32(0.5))
    if f['mode'] == 'gta':
        assert r64['steps'] == f['steps'] and r64['mel_length'] == f['steps'] * r
    elif f['stop'] == 'mid':
        s = f['stop_step']
        assert 5 <= s <= f['steps'] - 5 and r64['steps'] == s + 1 and s * r <= r64['mel_length'] < (s + 1) * r
        assert np.all(r64['stop'][:s * r] < 0.5)
    else:
        assert r64['steps'] == f['steps'] and r64['mel_length'] == f['steps'] * r and np.all(r64['stop'] < 0.5)


def test_fixtures_cover_the_issue_s_cases():
    F = fx.FIXTURES.values()
    assert {f['Tx'] for f in F} >= {1, 2, 5, 31, 63, 64, 65, 200}
    assert {f['steps'] for f in F} >= {1, 2, 24}
    assert any(f['dims'] is fx.REF for f in F) and any(f['dims'] is fx.SMALL2 for f in F)
    assert any(f['stop'] == 'mid' for f in F) and any(f['stop'] == 'never' and f['steps'] == 24 for f in F)
    assert any(f['mode'] == 'gta' and f['steps'] == 24 and f['dims'] is fx.REF for f in F) and any(not f['dropout'] for f in F)


def test_synthetic_state_matches_the_library_s_table():
    for dims in (fx.REF, fx.SMALL2):
        nat = _cabi.NativeTacotron(tacotron.make_dims(**dims))
        sd = make_tacotron_state(0, **dims)
        assert {k: v.shape for k, v in sd.items()} == nat.tensor_shapes()
        assert all(v.dtype == np.float32 for v in sd.values())
        again = make_tacotron_state(0, **dims)
        assert all(np.array_equal(sd[k], again[k]) for k in sd)
        for k, v in sd.items():
            nat.load_tensor(k, v)
        with pytest.raises(_cabi.WrnnError, match='MISSING_KEY'):
            nat.load_tensor('decoder/dense_1/kernel', sd['decoder/dense/kernel'])
        with pytest.raises(_cabi.WrnnError, match='shape'):
            nat.load_tensor('decoder/dense/kernel', sd['decoder/dense/bias'])
        bad = sd['decoder/dense/bias'].copy()
        bad[0] = np.nan
        with pytest.raises(_cabi.WrnnError, match='not finite'):
            nat.load_tensor('decoder/dense/bias', bad)


def test_create_refuses_dims_it_cannot_serve():
    for bad in (dict(prenet_layers=(8,) * 5), dict(decoder_layers=5), dict(num_mels=0), dict(attention_kernel=65), dict(decoder_lstm_units=8192),
                dict(zoneout=1.5)):
        with pytest.raises(_cabi.WrnnError, match='INVALID'):
            _cabi.NativeTacotron(tacotron.make_dims(**bad))
    d = tacotron.make_dims()
    d.struct_size -= 4
    with pytest.raises(_cabi.WrnnError, match='struct_size'):
        _cabi.NativeTacotron(d)


def test_tacotron_structs_match_the_header_layout(tmp_path):
    structs = {'wrnn_taco_dims': _cabi.TacoDims, 'wrnn_taco_call': _cabi.TacoCall}
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{ROOT}/include/wavernn_amd.h"', 'int main(void) {']
    for cname, st in structs.items():
        lines.append(f'  printf("{cname} size %zu\\n", sizeof({cname}));')
        for fname, _ in st._fields_:
            lines.append(f'  printf("{cname} {fname} %zu\\n", offsetof({cname}, {fname}));')
    lines += ['  return 0;', '}']
    src = tmp_path / 'layout.c'
    src.write_text('\n'.join(lines))
    exe = tmp_path / 'layout'
    subprocess.check_call(['gcc', '-std=c11', '-o', str(exe), str(src)])
    got = {tuple(l.split()[:2]): int(l.split()[2]) for l in subprocess.check_output([str(exe)], text=True).split('\n') if l.strip()}
    for cname, st in structs.items():
        assert got[(cname, 'size')] == C.sizeof(st), cname
        for fname, _ in st._fields_:
            assert got[(cname, fname)] == getattr(st, fname).offset, (cname, fname)
    assert (_cabi.TACO_MAX_TX, _cabi.TACO_MAX_PRENET) == (1024, 4) and _cabi.TACO_MAX_TX >= 512
