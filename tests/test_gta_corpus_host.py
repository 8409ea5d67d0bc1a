"""CPU checks of the GTA corpus: the metadata reader, the pack rule's restatement (tests/gta_ref.py) against the padding
``Tacotron.synthesize`` applies to a target, the command lines' new options, the binding's struct, and the qualification of the fixtures
tests/test_gpu_gta_corpus.py runs: every attention argmax of a fixture's float64 run leads by at least MARGIN g."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tacotronv2_wavernn_chinese_amd import _cabi, tacotron
from tests import gta_ref
from tests import tacotron_fixtures as fx

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_read_metadata(tmp_path):
    p = tmp_path / 'train.txt'
    p.write_text('audio-000001.npy|mel-000001.npy|46200|168|你好。|n i3 h ao3 。\n'
                 'clip7.npy|mel-clip7.npy|100|2|好|h ao3\n'
                 'some/dir/audio-b.npy|mel-b.npy|300|3|你|n i3\n', encoding='utf-8')
    meta = tacotron.read_metadata(str(p))
    assert meta == {'000001': 'n i3 h ao3 。', 'clip7': 'h ao3', 'b': 'n i3'}
    symbols = tacotron.load_symbols(str(p))
    assert symbols == ['_', '~', 'ao3', 'h', 'i3', 'n', '。']
    seqs = tacotron.metadata_sequences(meta, ['clip7', '000001', 'audio-b'], symbols)
    assert seqs == [[3, 2, 1], [5, 4, 3, 2, 6, 1], [5, 4, 1]]
    with pytest.raises(ValueError, match="'000002'"):
        tacotron.metadata_sequences(meta, ['000001', '000002'], symbols)


@pytest.mark.parametrize('r', [1, 2])
def test_pack_rule_against_synthesize_s_own_padding(r):
    A = 4.0
    rng = np.random.Generator(np.random.PCG64(3))
    mels = [rng.random((n, 20), dtype=np.float32) for n in (7, 12, 1)]
    mels[0][0, :4] = [0.0, 1.0, 0.5, np.float32(1.0) - np.float32(2.0 ** -24)]
    packed, steps = gta_ref.pack(mels, r, A)
    assert steps == [-(-m.shape[0] // r) for m in mels] and packed.shape == (3, max(steps) * r, 20) and packed.dtype == np.float32
    for b, m in enumerate(mels):
        t = gta_ref.target(m, r, A)
        inner = np.clip(np.float32(8.0) * m - np.float32(4.0), -4.0, 4.0).astype(np.float32)
        # the rows of the mel itself, then what Tacotron.synthesize pads a target of that many rows with
        assert t.dtype == np.float32 and np.array_equal(t, tacotron.pad_gta_target(inner, r, A))
        assert t.shape[0] == steps[b] * r and t.shape[0] - m.shape[0] == -m.shape[0] % r
        assert np.all(t[m.shape[0]:] == -4.0)
        assert np.array_equal(packed[b, :t.shape[0]], t) and np.all(packed[b, t.shape[0]:] == 0.0)
        assert np.array_equal(gta_ref.cut(t, m.shape[0]), inner)
        # against float64: the two roundings stay within one spacing of 2A, and 0, 0.5, 1 are exact
        assert np.max(np.abs(inner.astype(np.float64) - np.clip(8.0 * m.astype(np.float64) - 4.0, -4.0, 4.0))) <= np.spacing(np.float32(8.0))
    assert gta_ref.target(mels[0], r)[0, :3].tolist() == [-4.0, 4.0, 0.0]


def test_parsers_accept_the_gta_options_and_refuse_the_bad_combinations():
    from tacotronv2_wavernn_chinese_amd import dataset, train
    full = ['--wav_dir', 'w', '--features', 'tacotron', '--gta_checkpoint', 'taco.npz', '--gta_metadata', 'train.txt', '--gta_seed', '7',
            '--gta_batch', '8', '--gta_report', 'r.tsv', '--gta_min_focus', '0.4']
    for parser, extra in ((dataset.build_parser(), ['--out_dir', 'o']), (train.build_parser(), [])):
        a = parser.parse_args(full + extra)
        assert (a.gta_checkpoint, a.gta_metadata, a.gta_seed, a.gta_batch, a.gta_report, a.gta_min_focus) == ('taco.npz', 'train.txt', 7, 8, 'r.tsv', 0.4)
        assert dataset.gta_arguments(a) is True
        plain = parser.parse_args(['--wav_dir', 'w'] + extra)
        assert dataset.gta_arguments(plain) is False and plain.gta_min_focus is None and plain.gta_batch == 64 and plain.gta_seed == 0
        with pytest.raises(ValueError, match='--features tacotron'):
            dataset.gta_arguments(parser.parse_args(['--wav_dir', 'w', '--gta_checkpoint', 't.npz', '--gta_metadata', 'm.txt'] + extra))
        with pytest.raises(ValueError, match='--gta_metadata'):
            dataset.gta_arguments(parser.parse_args(['--wav_dir', 'w', '--features', 'tacotron', '--gta_checkpoint', 't.npz'] + extra))
        with pytest.raises(ValueError, match='--gta_checkpoint'):
            dataset.gta_arguments(parser.parse_args(['--wav_dir', 'w', '--gta_min_focus', '0.5'] + extra))
    a = train.build_parser().parse_args(['-g'])          # the compatibility flag is still its own
    assert a.gta is True and a.gta_checkpoint is None
    with pytest.raises(ValueError, match='--wav_dir'):
        dataset.gta_arguments(train.build_parser().parse_args(['--features', 'tacotron', '--gta_checkpoint', 't.npz', '--gta_metadata', 'm.txt']))


def test_taco_structs_match_the_header_layout(tmp_path):
    """wrnn_taco_gta_call (and, once more, the call struct it was modelled on) against the C header itself."""
    structs = {'wrnn_taco_gta_call': _cabi.TacoGtaCall, 'wrnn_taco_call': _cabi.TacoCall}
    assert {'wrnn_taco_gta_corpus', 'wrnn_taco_gta_reserve', 'wrnn_taco_gta_workspace_bytes'} <= set(_cabi.EXPORTED_SYMBOLS)
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


def test_gta_call_is_refused_on_the_host_before_any_device_work():
    """struct_size, a NULL output and frames < 1 are host checks: they answer without a GPU."""
    nat = _cabi.NativeTacotron(tacotron.make_dims(**fx.SMALL))
    c = _cabi.TacoGtaCall()
    c.struct_size = C.sizeof(_cabi.TacoGtaCall) - 8
    with pytest.raises(_cabi.WrnnError, match='struct_size'):
        nat.gta_corpus(c)
    ids, tx, seeds = np.array([[1, 2]], np.int32), np.array([2], np.int32), np.array([0], np.uint64)
    frames, off = np.array([3], np.int32), np.array([0], np.int64)
    c.struct_size = C.sizeof(_cabi.TacoGtaCall)
    c.B, c.Tx_max, c.prenet_dropout = 1, 2, 1
    c.ids_host, c.tx_host, c.seeds_host, c.frames_host = ids.ctypes.data, tx.ctypes.data, seeds.ctypes.data, frames.ctypes.data
    c.mel_off_host, c.out_off_host = off.ctypes.data, off.ctypes.data
    c.mels_dev, c.gta_mels_dev, c.l1_dev, c.focus_dev, c.last_attention_dev = 256, 256, 256, 256, None   # never dereferenced: the call is refused
    c.mels_elems = c.out_elems = 60
    with pytest.raises(_cabi.WrnnError, match='an output pointer is NULL'):
        nat.gta_corpus(c)
    c.last_attention_dev = 256
    frames[0] = 0
    with pytest.raises(_cabi.WrnnError, match='utterance 0: 0 mel frames < 1'):
        nat.gta_corpus(c)
    frames[0] = 4
    with pytest.raises(_cabi.WrnnError, match='utterance 0: elements 0 .. 80 lie outside the mel table of 60'):
        nat.gta_corpus(c)
    frames[0], off[0] = 3, -1
    with pytest.raises(_cabi.WrnnError, match='outside the mel table'):
        nat.gta_corpus(c)
    off[0], tx[0] = 0, _cabi.TACO_MAX_TX + 1
    with pytest.raises(_cabi.WrnnError, match=f'utterance 0: {_cabi.TACO_MAX_TX + 1} symbols outside'):
        nat.gta_corpus(c)
    # the reserve entry checks its shape on the host too; nothing is reserved by a refusal
    for bad in ((0, 2, 3), (1, _cabi.TACO_MAX_TX + 1, 3), (1, 2, 0)):
        with pytest.raises(_cabi.WrnnError, match='INVALID'):
            nat.gta_reserve(*bad)
    assert nat.gta_workspace_bytes() == 0


def test_the_flag_of_a_gta_corpus_is_true_and_says_why_it_is_not_a_method():
    from tacotronv2_wavernn_chinese_amd.dataset import _GtaMade
    flag = _GtaMade()
    assert flag == True and bool(flag) and repr(flag) == 'True' and not flag == False   # noqa: E712
    with pytest.raises(ValueError, match='already holds GTA mels'):
        flag(None, [])


@pytest.mark.parametrize('name', sorted(gta_ref.DIMS))
@pytest.mark.parametrize('u', range(len(gta_ref.UTTERANCES)))
def test_fixture_qualifies(name, u):
    f = gta_ref.restated(name, u)
    r64, r32, g = f['r64'], f['r32'], f['g']
    frames, tx = gta_ref.UTTERANCES[u]
    r = fx.full_dims(gta_ref.DIMS[name])['outputs_per_step']
    assert r64['steps'] == r32['steps'] == -(-frames // r) and f['target'].shape[0] == r64['steps'] * r
    assert np.array_equal(np.asarray(r64['max_attentions']), np.asarray(r32['max_attentions']))
    assert all(np.isfinite(v) for v in g.values())
    assert len(f['leads']) >= (tx > 1) * (r64['steps'] - 1)
    worst = None
    for kind, s, lead, q in f['leads']:
        assert lead >= fx.MARGIN * g[q], (kind, s, lead, g[q])
        worst = lead / g[q] if worst is None or (g[q] > 0 and lead / g[q] < worst) else worst
    print(f'{name} u{u}: {len(f["leads"])} decisions, smallest lead {worst:.4g} g' if worst is not None else f'{name} u{u}: no decisions')
