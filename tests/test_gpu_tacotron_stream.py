"""The Tacotron stream on the GPU (``wrnn_taco_stream_*``, ``Tacotron.stream``) against ``Tacotron.synthesize`` on the same handle:
everything is compared with ``np.array_equal``, so any seeded weights serve.  A stream's pieces, concatenated over any partition into
pushes, and its ``result()`` are the offline call's arrays bit for bit; what a push releases follows ``stream_release``."""
import os

import numpy as np
import pytest
import torch

from tacotronv2_wavernn_chinese_amd import _cabi, tacotron
from tacotronv2_wavernn_chinese_amd.tacotron import Tacotron, stream_release
from tests import tacotron_fixtures as fx
from tests.tacotron_stream_cases import POSTNET_SHAPES, never_stopping_state

pytestmark = pytest.mark.gpu
PIECES = ('mel', 'mel_raw', 'decoder_output', 'alignments', 'stop_tokens', 'max_attentions')
FREE = ('ref_stop', 'ref_max', 'small_tx1', 'small2_tx2', 'small_tx5', 'small2_stop')
_models = {}


def fixture_model(name):
    f = fx.fixture(name)
    if name not in _models:
        _models[name] = Tacotron(**f['dims']).load_state(f['state'])
    return _models[name], f


def interior_model(shape):
    """Weights that never stop, for runs long enough to release rows while the decoder is still going."""
    key = 'interior_' + shape
    dims = POSTNET_SHAPES[shape][0]
    if key not in _models:
        _models[key] = Tacotron(**dims).load_state(never_stopping_state(dims))
    return _models[key], fx.full_dims(dims)


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a, b)


def assert_equals_offline(got, off, keys, what):
    for k in keys:
        assert same(got[k], off[k]), (what, k, np.asarray(got[k]).shape, np.asarray(off[k]).shape)


def stream_in_parts(m, seq, parts, off, **kw):
    """One utterance stepped by ``parts`` (the last entry repeats until it is done), checked after every push.  Returns the log of
    (decoded, final, finished) per push."""
    L, k = m.dims['postnet_layers'], m.dims['postnet_kernel']
    log, pieces, i = [], {q: [] for q in PIECES}, 0
    with m.stream([seq], **kw) as st:
        assert st.info()['halo'] == m.halo and st.info()['workspace_bytes'] > 0
        while not st.done:
            out = st.step(parts[min(i, len(parts) - 1)])[0]
            i += 1
            for q in PIECES:
                pieces[q].append(out[q])
            dec, fin, done = st.decoded[0], st.final[0], st.finished[0]
            log.append((dec, fin, done))
            assert fin == stream_release(dec, done, off['mel_length'], L, k), (parts, log)
            # nothing that was released has changed since: the buffers against the pieces handed out so far
            assert same(st._buf['mel'][0, :fin].cpu().numpy(), np.concatenate(pieces['mel'])), (parts, log)
            assert same(st._buf['mel_raw'][0, :st.final_raw[0]].cpu().numpy(), np.concatenate(pieces['mel_raw'])), (parts, log)
        res = st.result()[0]
    assert_equals_offline({q: np.concatenate(pieces[q]) for q in PIECES}, off, PIECES, ('pieces', parts))
    assert_equals_offline(res, off, PIECES + ('encoder_outputs',), ('result', parts))
    assert (res['steps'], res['mel_length']) == (off['steps'], off['mel_length']) == (log[-1][0] // m.r, log[-1][1])
    return log


@pytest.mark.parametrize('name', FREE)
def test_every_free_running_fixture_at_every_chunk_size(name):
    m, f = fixture_model(name)
    kw = dict(seeds=[f['seed']], max_iters=f['steps'], prenet_dropout=f['dropout'])
    off = m.synthesize([f['seq']], **kw)[0]
    for chunk in (1, 3, 7, f['steps'], f['steps'] + 5):
        log = stream_in_parts(m, f['seq'], [chunk], off, **kw)
        assert len(log) == -(-off['steps'] // chunk)
    if f['stop'] == 'mid':
        assert off['steps'] < f['steps'] and off['mel_length'] < off['steps'] * m.r    # the stop came from the device, and it trims


@pytest.mark.parametrize('shape,parts', [('5x5', [1, 2, 10, 3, 29]), ('5x5', [11] * 5), ('5x5', [10] * 5),
                                         ('5x5_r2', [1, 2, 10, 3, 29]), ('5x5_r2', [11] * 5), ('5x5_r2', [10] * 5),
                                         ('2x3', [4, 4, 4, 33]), ('2x4', [4, 4, 4, 33]), ('1x5', [4, 4, 4, 33])])
def test_interior_rows_are_released_before_the_end(shape, parts):
    m, d = interior_model(shape)
    halo = POSTNET_SHAPES[shape][1]
    seq = np.random.Generator(np.random.PCG64(40)).integers(0, d['n_symbols'], size=40).tolist()
    kw = dict(seeds=[21], max_iters=45)
    off = m.synthesize([seq], **kw)[0]
    assert off['steps'] == 45 and off['mel_length'] == 45 * m.r and m.halo == halo
    log = stream_in_parts(m, seq, parts, off, **kw)
    assert [dec for dec, _, _ in log] == [min(int(n), 45) * m.r for n in np.cumsum(parts)]     # the last push runs what is left
    running = [(dec, fin) for dec, fin, done in log if not done]
    assert len(running) == len(parts) - 1 and all(fin == max(dec - halo, 0) for dec, fin in running)
    assert running[-1][1] > 0 and log[-1] == (45 * m.r, 45 * m.r, True)


def test_ragged_batch_equals_each_alone_and_the_offline_call():
    m, f = fixture_model('small2_stop')
    rng = np.random.Generator(np.random.PCG64(44))
    seqs = [rng.integers(0, f['full']['n_symbols'], size=7).tolist(), f['seq'], rng.integers(0, f['full']['n_symbols'], size=50).tolist()]
    seeds = [5, f['seed'], 6]
    off = m.synthesize(seqs, seeds=seeds, max_iters=24)
    assert off[1]['steps'] == f['stop_step'] + 1 < off[0]['steps'] == 24 and off[2]['steps'] != off[1]['steps']    # the crafted one stops mid-run, first
    pieces, empty_while_others_run = [{q: [] for q in PIECES} for _ in seqs], False
    with m.stream(seqs, seeds=seeds, max_iters=24) as st:
        while not st.done:
            was = list(st.finished)
            out = st.step(5)
            for b in range(3):
                for q in PIECES:
                    pieces[b][q].append(out[b][q])
                if was[b]:
                    assert all(out[b][q].shape[0] == 0 for q in PIECES)
                    empty_while_others_run = True
        res = st.result()
    assert empty_while_others_run
    for b in range(3):
        alone_off = m.synthesize([seqs[b]], seeds=[seeds[b]], max_iters=24)[0]
        stream_in_parts(m, seqs[b], [5], alone_off, seeds=[seeds[b]], max_iters=24)    # its own stream equals its own offline call
        for want in (off[b], alone_off):
            assert_equals_offline({q: np.concatenate(pieces[b][q]) for q in PIECES}, want, PIECES, ('ragged pieces', b))
            assert_equals_offline(res[b], want, PIECES + ('encoder_outputs',), ('ragged result', b))
            assert (res[b]['steps'], res[b]['mel_length']) == (want['steps'], want['mel_length'])


def test_two_streams_and_an_offline_call_on_one_handle_do_not_meet():
    m, f = fixture_model('small_tx5')
    rng = np.random.Generator(np.random.PCG64(45))
    sa, sb, sc = (rng.integers(0, f['full']['n_symbols'], size=n).tolist() for n in (33, 9, 70))
    want_a = m.synthesize([sa], seeds=[1], max_iters=20)[0]
    want_b = m.synthesize([sb], seeds=[2], max_iters=17)[0]
    want_c = m.synthesize([sc], seeds=[3], max_iters=6)[0]
    with m.stream([sa], seeds=[1], max_iters=20) as a, m.stream([sb], seeds=[2], max_iters=17) as b:
        got_c = None
        while not (a.done and b.done):
            if not a.done:
                a.step(3)
            if got_c is None:
                got_c = m.synthesize([sc], seeds=[3], max_iters=6)[0]
            if not b.done:
                b.step(4)
        assert_equals_offline(a.result()[0], want_a, PIECES + ('encoder_outputs',), 'a')
        assert_equals_offline(b.result()[0], want_b, PIECES + ('encoder_outputs',), 'b')
    assert_equals_offline(got_c, want_c, PIECES + ('encoder_outputs',), 'offline in between')


def test_refusals():
    m, f = fixture_model('small_tx5')
    with pytest.raises(_cabi.WrnnError, match='INVALID.*teacher forcing'):
        m.stream([[1, 2]], max_iters=2, gta_targets=[np.zeros((2, 20), np.float32)])
    with pytest.raises(_cabi.WrnnError, match='INVALID.*outside the table'):
        m.stream([[1, f['full']['n_symbols'], 2]], max_iters=1)
    st = m.stream([[1, 2, 3]], max_iters=3)
    with pytest.raises(_cabi.WrnnError, match='INVALID.*n_steps 0 < 1'):
        st.step(0)
    with pytest.raises(_cabi.WrnnError, match='STATE.*result'):
        st.result()
    st.step(2)
    assert not st.done and st.decoded == [2]
    st.step(2)                                  # one step is left: a push runs what there is
    assert st.done and st.decoded == [3]
    with pytest.raises(_cabi.WrnnError, match='STATE.*finished'):
        st.step(1)
    assert st.result()[0]['steps'] == 3
    st.close()
    for use in (lambda: st.step(1), st.result, st.info):
        with pytest.raises(_cabi.WrnnError, match='STATE.*closed'):
            use()
    st.close()                                  # twice is fine


def test_text_to_audio_with_both_halves_streaming(tmp_path):
    """A Tacotron stream in 4-step pushes into WaveRNN.stream(tail='reference') against synthesize, then generate, after the same
    torch.manual_seed.  The vocoder takes 80 channels, so the Tacotron is the interior-rows model with num_mels = 80."""
    from tacotronv2_wavernn_chinese_amd.synth import DEFAULT_DIMS, make_state_dict
    from tacotronv2_wavernn_chinese_amd.vocoder import WaveRNN
    dims = dict(fx.SMALL, num_mels=80)
    m = Tacotron(**dims).load_state(never_stopping_state(dims))
    seq = np.random.Generator(np.random.PCG64(40)).integers(0, dims['n_symbols'], size=40).tolist()
    voc = WaveRNN(**DEFAULT_DIMS, mode='RAW')
    voc.verbose = False
    voc.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in make_state_dict(0, variant='peaky').items()})
    voc.to('cuda:0')
    mel = m.synthesize([seq], seeds=[9], max_iters=45, return_device=True)[0]['mel']
    assert mel.shape == (45, 80)
    torch.manual_seed(1234)
    want = voc.generate(mel.T[None].contiguous(), str(tmp_path / 'offline.wav'), False, 11000, 550, True)
    torch.manual_seed(1234)
    got, t_mel, t_audio = tacotron.synthesize_stream_to_wav(m, voc, seq, str(tmp_path / 'stream.wav'), chunk_steps=4, seed=9, tail='reference', max_iters=45)
    assert want.shape == (44 * 275,) and same(got, want)
    assert 0 < t_mel <= t_audio
    assert (tmp_path / 'stream.wav').read_bytes() == (tmp_path / 'offline.wav').read_bytes()


def test_cli_stream_steps_writes_the_same_bytes(tmp_path):
    m, f = fixture_model('small2_stop')
    tokens = [f'w{i:02d}' for i in range(f['full']['n_symbols'] - 2)]
    (tmp_path / 'train.txt').write_text('a|b|3|' + ' '.join(tokens) + '\n', encoding='utf-8')
    symbols = tacotron.load_symbols(str(tmp_path / 'train.txt'))
    np.savez(tmp_path / 'taco-123.npz', **{tacotron.KEY_PREFIX + k + ':0': v for k, v in f['state'].items()})
    text = ' '.join(symbols[i] for i in f['seq'][:-1] if i >= 2)
    common = ['--pinyin', text, '--symbols', str(tmp_path / 'train.txt'), '--checkpoint', str(tmp_path / 'taco-123.npz'), '--seed', '5', '--max_iters', '24']
    plain = tacotron.main(common + ['--out_dir', str(tmp_path / 'plain')])
    streamed = tacotron.main(common + ['--out_dir', str(tmp_path / 'streamed'), '--stream-steps', '4'])
    assert os.path.basename(plain) == os.path.basename(streamed)
    assert open(plain, 'rb').read() == open(streamed, 'rb').read() and np.load(streamed).shape[0] > 0
