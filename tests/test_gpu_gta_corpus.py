"""The GTA corpus on the GPU (``DeviceCorpus.gta`` -> ``wrnn_taco_gta_corpus``, ``csrc/taco_gta.hip``) on the fixtures
``tests/test_gta_corpus_host.py`` qualified: against ``Tacotron.synthesize`` teacher-forced on the restated target bit for bit, against
the float64 restatement within K g (the bound and the unit of ``tests/test_gpu_tacotron.py``), the report's two sums against NumPy
float64 sums, what the new corpus shares and owns, its files, its window batches, the refusals and the preprocessing command line."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tacotronv2_wavernn_chinese_amd import _cabi
from tacotronv2_wavernn_chinese_amd import dataset as D
from tacotronv2_wavernn_chinese_amd import train as T
from tacotronv2_wavernn_chinese_amd.tacotron import Tacotron
from tests import gta_ref
from tests import tacotron_fixtures as fx

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = 'cuda:0'
K_BOUND = 16   # tests/test_gpu_tacotron.py
NAMES = sorted(gta_ref.DIMS)
N = len(gta_ref.UTTERANCES)
_cache = {}


def model_for(name):
    if ('model', name) not in _cache:
        _cache['model', name] = Tacotron(**gta_ref.DIMS[name]).load_state(gta_ref.state(name))
    return _cache['model', name]


def corpus():
    """The five utterances as a corpus of Tacotron features; 4 * frames dummy labels each."""
    if 'corpus' not in _cache:
        pairs = []
        for u in range(N):
            _, mel, _ = gta_ref.utterance(u)
            pairs.append((mel.T, (np.arange(gta_ref.HOP * mel.shape[0]) % 512).astype(np.int32)))
        _cache['corpus'] = D.DeviceCorpus.from_pairs(pairs, DEV, hop_length=gta_ref.HOP, features='tacotron')
    return _cache['corpus']


def seqs():
    return [gta_ref.utterance(u)[0] for u in range(N)]


def made(name, batch_utts=5):
    """``corpus().gta`` once per (dims, batch_utts), shared by the tests."""
    key = ('made', name, batch_utts)
    if key not in _cache:
        _cache[key] = corpus().gta(model_for(name), seqs(), seed_base=900, batch_utts=batch_utts)
    return _cache[key]


def alone(name, u):
    """``synthesize`` of utterance u alone, teacher-forced on the restated target: the reference computed once."""
    key = ('alone', name, u)
    if key not in _cache:
        seq, mel, seed = gta_ref.utterance(u)
        d = fx.full_dims(gta_ref.DIMS[name])
        tg = gta_ref.target(mel, d['outputs_per_step'], d['max_abs_value'])
        _cache[key] = model_for(name).synthesize([seq], seeds=[seed], gta_targets=[tg])[0]
    return _cache[key]


def rows(c, u, table=None):
    t = c.mels if table is None else table
    mo, f = int(c.mel_off[u]), int(c.frames[u])
    return t[mo:mo + f * c.n_mels].cpu().numpy().reshape(f, c.n_mels)


@pytest.mark.parametrize('name', NAMES)
def test_gta_mels_equal_synthesize_on_each_utterance_alone(name):
    c, report = made(name)
    r = fx.full_dims(gta_ref.DIMS[name])['outputs_per_step']
    assert c.gta == True and c.gta_made and c.features == 'tacotron' and len(c) == N
    for u in range(N):
        want = alone(name, u)
        f = gta_ref.UTTERANCES[u][0]
        assert want['mel'].shape[0] == -(-f // r) * r           # 7 -> 8 decoded -> 7 kept and 1 -> 2 -> 1 under r = 2
        got = rows(c, u)
        assert got.shape == (f, 20) and got.tobytes() == gta_ref.cut(want['mel'], f).tobytes(), u
    assert report['tx'].tolist() == [t for _, t in gta_ref.UTTERANCES] and report['frames'].tolist() == [f for f, _ in gta_ref.UTTERANCES]


@pytest.mark.parametrize('name', NAMES)
def test_the_grouping_and_a_second_call_change_no_bit(name):
    base, rep0 = made(name)
    for batch_utts in (1, 2, 5):
        c, rep = corpus().gta(model_for(name), seqs(), seed_base=900, batch_utts=batch_utts)
        assert torch.equal(c.mels, base.mels), batch_utts
        for k in ('l1', 'focus', 'last_attention', 'steps'):
            assert rep[k].tobytes() == rep0[k].tobytes(), (batch_utts, k)
    c, _ = corpus().gta(model_for(name), seqs(), seeds=[900 + u for u in range(N)], batch_utts=2)
    assert torch.equal(c.mels, base.mels)
    other, _ = corpus().gta(model_for(name), seqs(), seed_base=901, batch_utts=5)
    assert not torch.equal(other.mels, base.mels)               # the seed keys the dropout masks


@pytest.mark.parametrize('name', NAMES)
def test_against_the_float64_restatement(name):
    c, report = made(name)
    lines, bad = [], []
    for u in range(N):
        f = gta_ref.restated(name, u)
        r64, g = f['r64'], f['g']['mel']
        frames = gta_ref.UTTERANCES[u][0]
        assert int(report['steps'][u]) == r64['steps']
        assert int(report['last_attention'][u]) == int(np.asarray(r64['max_attentions'])[-1])
        err = float(np.max(np.abs(rows(c, u).astype(np.float64) - np.asarray(r64['mel'], np.float64)[:frames])))
        ratio = err / g if g > 0 else (0.0 if err == 0 else float('inf'))
        lines.append(f'{name} u{u}: g {g:.3e}  error {err:.3e}  ratio {ratio:.3f}')
        if not err <= K_BOUND * g:
            bad.append(lines[-1])
    print('\n' + '\n'.join(lines))
    assert not bad, bad


@pytest.mark.parametrize('name', NAMES)
def test_the_report_s_sums_against_numpy_float64(name):
    c, report = made(name)
    for u in range(N):
        gt = gta_ref.utterance(u)[1]
        l1 = float(np.mean(np.abs(rows(c, u).astype(np.float64) - gt.astype(np.float64))))
        focus = float(np.mean(np.max(alone(name, u)['alignments'].astype(np.float64), axis=1)))
        print(f'{name} u{u}: l1 {report["l1"][u]!r} (numpy {l1!r})  focus {report["focus"][u]!r} (numpy {focus!r})')
        assert abs(report['l1'][u] - l1) <= 1e-12 * abs(l1)
        assert abs(report['focus'][u] - focus) <= 1e-12 * abs(focus)
        assert 0.0 < report['focus'][u] <= 1.0 and 0.0 <= report['l1'][u] <= 1.0


def test_what_the_gta_corpus_shares_and_what_it_owns():
    src = corpus()
    before = src.mels.clone()
    c, _ = src.gta(model_for('small2'), seqs(), seed_base=900, batch_utts=2)
    assert c.labels is src.labels and c.label_off is src.label_off and c.label_len is src.label_len
    assert all(a is b for a, b in zip(c.device_tables(), src.device_tables()))
    assert c.source_mels is src.mels and torch.equal(src.mels, before)
    assert c.mels.data_ptr() != src.mels.data_ptr() and c.mels.shape == src.mels.shape
    assert np.array_equal(c.mel_off, src.mel_off) and np.array_equal(c.frames, src.frames) and c.stems == src.stems
    assert not src.gta_made and src.source_mels is None and callable(src.gta)
    train, test = c.split(2)
    for part in (train, test):
        assert part.gta == True and part.gta_made and part.source_mels is src.mels and part.mels is c.mels and part.labels is src.labels
    assert len(train) == 3 and len(test) == 2
    with pytest.raises(ValueError, match='already holds GTA mels'):
        train.gta(model_for('small2'), seqs()[:3])


@pytest.mark.parametrize('batch_utts', [1, 2, 5])
def test_the_scratch_is_sized_once_for_the_largest_group(batch_utts):
    """The groups are queued shortest first and every one needs more scratch than the last; growing the scratch waits for the stream.
    So ``gta`` reserves the largest group's need before the first call: on a fresh handle the scratch after the whole ragged corpus is
    what one reserve for (largest B, largest Tx, most frames) gives another fresh handle, i.e. no group grew it."""
    fresh, probe = (Tacotron(**gta_ref.DIMS['small2']).load_state(gta_ref.state('small2')) for _ in range(2))
    assert fresh.native.gta_workspace_bytes() == 0
    c, _ = corpus().gta(fresh, seqs(), seed_base=900, batch_utts=batch_utts)
    want = probe.native.gta_reserve(min(batch_utts, N), max(t for _, t in gta_ref.UTTERANCES), max(f for f, _ in gta_ref.UTTERANCES))
    assert fresh.native.gta_workspace_bytes() == want > 0
    assert torch.equal(c.mels, made('small2')[0].mels)
    corpus().gta(fresh, seqs(), seed_base=900, batch_utts=1)          # smaller groups: nothing grows
    assert fresh.native.gta_workspace_bytes() == want


def test_save_then_load(tmp_path):
    c, _ = made('small2')
    c.gta_note['checkpoint'] = 'taco-77.npz'
    listing = c.save(tmp_path / 'gta')
    lines = listing.read_text().splitlines()
    assert len(lines) == N
    for u, line in enumerate(lines):
        q, m, g, stem = line.split('|')
        assert stem == c.stems[u] and os.path.dirname(g).endswith('mel_gta') and os.path.dirname(m).endswith('mel')
        assert np.load(m).tobytes() == gta_ref.utterance(u)[1].tobytes()                 # field 1: the ground truth
        assert np.load(g).dtype == np.float32 and np.load(g).tobytes() == rows(c, u).tobytes()   # field 2: the GTA mel
        assert np.load(q).shape == (gta_ref.HOP * gta_ref.UTTERANCES[u][0],)
    assert D.saved_features(listing) == 'tacotron'
    assert (tmp_path / 'gta' / 'wavernn_training_features.txt').read_text() == 'tacotron\n'
    assert (tmp_path / 'gta' / 'wavernn_training_gta.txt').read_text() == 'checkpoint taco-77.npz\nseed_base 900\n'
    again = D.DeviceCorpus.load(listing, DEV, hop_length=gta_ref.HOP)
    assert again.features == 'tacotron' and torch.equal(again.mels, c.mels) and torch.equal(again.labels, c.labels)
    # a corpus that is not GTA saves exactly as before
    plain = corpus().save(tmp_path / 'plain')
    assert not (tmp_path / 'plain' / 'mel_gta').exists() and not (tmp_path / 'plain' / 'wavernn_training_gta.txt').exists()
    assert all(l.split('|')[1] == l.split('|')[2] for l in plain.read_text().splitlines())


def test_window_batches_of_the_gta_corpus_equal_the_host_collate():
    c, _ = made('small')
    long = c.subset([1, 2, 3])                                   # 12, 13 and 24 frames: a window of 4 frames with pad 1 fits
    kw = dict(mode='RAW', bits=9, hop_length=gta_ref.HOP, pad=1, seq_len=2 * gta_ref.HOP)
    dev, host = list(D.DeviceWindowLoader(long, 2, seed=6, **kw)), list(T.WindowLoader(long.pairs(), 2, seed=6, **kw))
    assert len(dev) == len(host) == 2
    for (x, y, m), (x0, y0, m0) in zip(dev, host):
        assert torch.equal(x.cpu(), x0) and torch.equal(y.cpu(), y0) and torch.equal(m.cpu(), m0)
    assert np.array_equal(long.pairs()[0][0].T, rows(c, 1))      # the windows are cut from the GTA mels


def test_refusals():
    m, src = model_for('small'), corpus()
    pairs = src.pairs()
    vocoder = D.DeviceCorpus.from_pairs(pairs, DEV, hop_length=gta_ref.HOP, features='vocoder')
    with pytest.raises(ValueError, match="'vocoder'"):
        vocoder.gta(m, seqs())
    wide = D.DeviceCorpus.from_pairs([(np.zeros((21, 3), np.float32), np.zeros(12, np.int32))], DEV, hop_length=gta_ref.HOP, features='tacotron')
    with pytest.raises(ValueError, match='21 mel bands'):
        wide.gta(m, [[1, 2]])
    with pytest.raises(ValueError, match='4 symbol sequences for 5 utterances'):
        src.gta(m, seqs()[:4])
    too_long = seqs()
    too_long[3] = [1] * (_cabi.TACO_MAX_TX + 1)
    with pytest.raises(_cabi.WrnnError, match=f'INVALID.*{_cabi.TACO_MAX_TX + 1} symbols.*{src.stems[3]!r}'):
        src.gta(m, too_long, batch_utts=2)
    bad_id = seqs()
    bad_id[1] = [1, 30, 2]
    with pytest.raises(_cabi.WrnnError, match=f'INVALID.*outside the table.*{src.stems[1]!r}'):
        src.gta(m, bad_id, batch_utts=5)
    # a null output pointer through the binding
    ids, tx, seeds = np.array([[1, 2]], np.int32), np.array([2], np.int32), np.array([0], np.uint64)
    frames, off = np.array([7], np.int32), np.array([0], np.int64)
    out, l1 = torch.zeros(140, device=DEV), torch.zeros(1, dtype=torch.float64, device=DEV)
    call = _cabi.TacoGtaCall()
    call.struct_size = C.sizeof(_cabi.TacoGtaCall)
    call.B, call.Tx_max, call.prenet_dropout = 1, 2, 1
    call.ids_host, call.tx_host, call.seeds_host, call.frames_host = ids.ctypes.data, tx.ctypes.data, seeds.ctypes.data, frames.ctypes.data
    call.mel_off_host, call.out_off_host = off.ctypes.data, off.ctypes.data
    call.mels_dev, call.mels_elems, call.gta_mels_dev, call.out_elems = src.mels.data_ptr(), src.mels.numel(), out.data_ptr(), out.numel()
    call.l1_dev, call.focus_dev, call.last_attention_dev = l1.data_ptr(), None, None
    with pytest.raises(_cabi.WrnnError, match='INVALID.*an output pointer is NULL'):
        m.native.gta_corpus(call, torch.cuda.current_stream().cuda_stream)
    assert float(out.abs().sum()) == 0.0


def test_preprocess_command_line_writes_the_gta_corpus(tmp_path):
    """wavernn_preprocess.py --features tacotron --gta_checkpoint ...: three 0.6 s clips, the reference's dims."""
    from tacotronv2_wavernn_chinese_amd.dsp import save_wav
    from tacotronv2_wavernn_chinese_amd.hparams import DEFAULT_HPARAMS
    from tacotronv2_wavernn_chinese_amd.synth import make_tacotron_state
    from tacotronv2_wavernn_chinese_amd import tacotron
    wav_dir, out_dir = tmp_path / 'wavs', tmp_path / 'data'
    wav_dir.mkdir()
    rng = np.random.Generator(np.random.PCG64(8))
    t = np.arange(int(0.6 * 22050)) / 22050.0
    for i in range(3):
        x = 0.4 * np.sin(2 * np.pi * (200.0 + 150.0 * i) * t) + 0.02 * rng.standard_normal(t.size)
        save_wav(x.astype(np.float32), wav_dir / f'{i + 1:06d}.wav', 22050)
    texts = ['n i3 h ao3 。', 'h ao3 n i3 h ao3 ， n i3 。', 'n i3 。']
    meta = tmp_path / 'train.txt'
    meta.write_text(''.join(f'audio-{i + 1:06d}.npy|mel-{i + 1:06d}.npy|13230|49|x|{p}\n' for i, p in enumerate(texts)), encoding='utf-8')
    symbols = tacotron.load_symbols(str(meta))
    np.savez(tmp_path / 'taco-5.npz', **make_tacotron_state(2, 'peaked', n_symbols=len(symbols)))
    hp_file = tmp_path / 'tiny_hparams.py'
    hp_file.write_text(open(DEFAULT_HPARAMS).read() + '\nvoc_seq_len = hop_length * 2\n')
    report = tmp_path / 'report.tsv'
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'wavernn_preprocess.py'), '--wav_dir', str(wav_dir), '--out_dir', str(out_dir), '--hp_file',
                        str(hp_file), '--features', 'tacotron', '--gta_checkpoint', str(tmp_path / 'taco-5.npz'), '--gta_metadata', str(meta),
                        '--gta_seed', '3', '--gta_batch', '2', '--gta_report', str(report)], cwd=tmp_path, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert 'GTA mels of 3 utterances from taco-5.npz' in r.stdout and 'GTA mels in mel_gta/' in r.stdout
    lines = (out_dir / 'wavernn_training_data.txt').read_text().splitlines()
    assert [l.split('|')[3] for l in lines] == ['000001', '000002', '000003']
    for l in lines:
        q, m, g, stem = l.split('|')
        truth, gta = np.load(m), np.load(g)
        assert g.endswith(f'mel_gta/{stem}.npy') and truth.shape == gta.shape and gta.shape[1] == 80 and gta.dtype == np.float32
        assert gta.min() >= 0.0 and gta.max() <= 1.0 and not np.array_equal(truth, gta) and np.load(q).shape == (gta.shape[0] * 275,)
    assert (out_dir / 'wavernn_training_gta.txt').read_text() == 'checkpoint taco-5.npz\nseed_base 3\n'
    assert (out_dir / 'wavernn_training_features.txt').read_text() == 'tacotron\n'
    rep = report.read_text().splitlines()
    assert rep[0].split('\t') == ['stem', 'frames', 'tx', 'l1', 'focus', 'last_attention'] and [l.split('\t')[0] for l in rep[1:]] == ['000001', '000002', '000003']
    assert [int(l.split('\t')[2]) for l in rep[1:]] == [len(p.split(' ')) + 1 for p in texts]
