"""CPU checks of the Tacotron stream's host side: the release rule against brute force on the float64 restatement
(tests/tacotron_ref.py), the C halo, the new structs against the header, and the refusals ``wrnn_taco_stream_open`` makes before it
touches a device."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tacotronv2_wavernn_chinese_amd import _cabi, tacotron
from tests import tacotron_fixtures as fx
from tests import tacotron_ref as ref
from tests.tacotron_stream_cases import POSTNET_SHAPES, SEED
from tacotronv2_wavernn_chinese_amd.synth import make_tacotron_state

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T = 45


@pytest.mark.parametrize('shape', sorted(POSTNET_SHAPES))
def test_release_rule_is_tight_against_brute_force(shape):
    """The postnet of a prefix of d decoder frames against the postnet of all T: the rows the rule calls final are bit-equal, and the
    first row it withholds is not.  float64, so the convolution's own sums are the same whatever the length."""
    dims, halo = POSTNET_SHAPES[shape]
    d = fx.full_dims(dims)
    L, k = d['postnet_layers'], d['postnet_kernel']
    assert tacotron.stream_halo(L, k) == halo
    w = {name: np.asarray(v, dtype=np.float64) for name, v in make_tacotron_state(SEED, **dims).items()}
    frames = np.random.Generator(np.random.PCG64(SEED)).uniform(-4.0, 4.0, size=(T, d['num_mels']))
    never = np.zeros(T)
    whole = ref.postprocess(w, frames, never, np.float64, postnet_layers=L)
    for n in range(1, T):
        part = ref.postprocess(w, frames[:n], never[:n], np.float64, postnet_layers=L)
        final = tacotron.stream_release(n, False, 0, L, k)
        assert final == max(n - halo, 0) and final < n
        for q in ('mel_raw', 'mel'):
            assert np.array_equal(part[q][:final], whole[q][:final]), (shape, n, q)
        assert not np.array_equal(part['mel_raw'][final], whole['mel_raw'][final]), (shape, n)
    assert tacotron.stream_release(T, True, T, L, k) == T


def _decode(stop_bias, max_iters):
    state = {k: v.astype(np.float64) for k, v in make_tacotron_state(3, **fx.SMALL).items()}
    sp = 'decoder/stop_token_projection/projection_stop_token_projection/'
    state[sp + 'kernel'] = np.zeros_like(state[sp + 'kernel'])
    state[sp + 'bias'] = np.full_like(state[sp + 'bias'], stop_bias)
    return fx.run_ref(state, fx.SMALL, [3, 1, 4, 1, 5], np.float64, max_iters=max_iters, seed=1), state


def test_release_once_finished():
    # a stop in the very first step: one frame decoded, the postnet sees it, none is released
    res, state = _decode(1e-9, 4)
    assert (res['steps'], res['mel_length']) == (1, 0)
    assert tacotron.stream_release(res['steps'], True, res['mel_length'], 5, 5) == 0
    # a run into max_iters: nothing before the end (12 < halo + 1), everything at it
    res, _ = _decode(0.0, 12)
    assert (res['steps'], res['mel_length']) == (12, 12)
    assert [tacotron.stream_release(n, False, 0, 5, 5) for n in (1, 10, 11)] == [0, 0, 1]
    assert tacotron.stream_release(12, True, res['mel_length'], 5, 5) == 12
    # the first stop trims: the stopping frame and everything after it are decoded but never released
    w = {k: np.asarray(v) for k, v in state.items()}
    out = ref.postprocess(w, np.linspace(-5, 5, 14 * 20).reshape(14, 20), np.array([0.1] * 12 + [0.9, 0.3]), np.float64)
    assert out['mel_length'] == 12 and out['mel_raw'].shape[0] == 14
    assert tacotron.stream_release(14, True, out['mel_length'], 5, 5) == 12
    assert tacotron.stream_release(13, False, 0, 5, 5) == 3 <= out['mel_length']       # what was released while running stays inside


def test_c_halo_is_the_python_rule():
    for shape, (dims, halo) in POSTNET_SHAPES.items():
        d = fx.full_dims(dims)
        assert _cabi.taco_stream_halo(tacotron.make_dims(**dims)) == halo == tacotron.stream_halo(d['postnet_layers'], d['postnet_kernel']), shape
    for k in range(1, 12):
        assert _cabi.taco_stream_halo(tacotron.make_dims(postnet_layers=3, postnet_kernel=k)) == 3 * (k // 2)


def test_stream_structs_match_the_header_layout(tmp_path):
    structs = {'wrnn_taco_stream_opts': _cabi.TacoStreamOpts, 'wrnn_taco_stream_outputs': _cabi.TacoStreamOutputs}
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


def _opts(ids, max_iters=4, **over):
    ids = np.ascontiguousarray(ids, dtype=np.int32)
    tx = np.full(ids.shape[0], ids.shape[1], dtype=np.int32)
    seeds = np.zeros(ids.shape[0], dtype=np.uint64)
    o = _cabi.TacoStreamOpts()
    o.struct_size = C.sizeof(_cabi.TacoStreamOpts)
    o.B, o.Tx_max, o.max_iters, o.prenet_dropout = ids.shape[0], ids.shape[1], max_iters, 1
    o.ids_host, o.tx_host, o.seeds_host = ids.ctypes.data, tx.ctypes.data, seeds.ctypes.data
    for k, v in over.items():
        setattr(o, k, v)
    return o, (ids, tx, seeds)


def test_open_refuses_on_the_host():
    """Every one of these is decided before the first device call, with the wording of wrnn_taco_synthesize; no stream is returned and
    the reason is the handle's."""
    nat = _cabi.NativeTacotron(tacotron.make_dims(**fx.SMALL))
    good = [[1, 2, 3]]
    cases = [(_opts(good, struct_size=C.sizeof(_cabi.TacoStreamOpts) - 8), 'struct_size'),
             (_opts(good, gta_dev=1), 'teacher forcing'),
             (_opts(np.ones((1, _cabi.TACO_MAX_TX + 1))), r'Tx_max 1025 outside 1 \.\. 1024 symbols'),
             (_opts([[1, 30, 2]]), 'symbol id 30 at 1 is outside the table of 30'),
             (_opts([[1, -1, 2]]), 'outside the table'),
             (_opts(good, max_iters=0), 'max_iters 0 < 1'),
             (_opts(good, B=0), 'B 0 outside')]
    for (o, keep), why in cases:
        with pytest.raises(_cabi.WrnnError, match='INVALID.*' + why):
            nat.stream_open(o, 0)
    st = C.c_void_p(1)
    o, keep = _opts(good, max_iters=0)
    assert nat.lib.wrnn_taco_stream_open(nat._h, C.byref(o), None, C.byref(st)) == _cabi.ERR_INVALID and not st.value
    assert nat.lib.wrnn_taco_stream_step(None, 1, None, None, None, None) == _cabi.ERR_INVALID
    nat.lib.wrnn_taco_stream_close(None)
