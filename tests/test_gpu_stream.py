"""Streaming generation (wrnn_stream_*, WaveRNN.stream): audio while mel frames are still arriving.

The contract: a stream fed the frames of a mel (B, n_mels, T) in ANY partition into pushes and then finished emits exactly the
labels / samples of the offline unbatched call with the same seed, noise mode and kernel, and -- with tail='reference' -- exactly
the float64 audio generate() returns after the same torch.manual_seed.  The offline path is oracle-checked elsewhere, so
equality carries its reference parity over to streams.
"""
import numpy as np
import pytest
import torch

from tests.parity_util import stream_raw as _stream_raw

pytestmark = pytest.mark.gpu

HOP = 275


def _model(mode='RAW', variant='peaky', seed=0):
    from tacotronv2_wavernn_chinese_amd.synth import DEFAULT_DIMS, make_state_dict
    from tacotronv2_wavernn_chinese_amd.vocoder import WaveRNN
    sd = make_state_dict(seed, mode=mode, variant=variant)
    m = WaveRNN(**DEFAULT_DIMS, mode=mode)
    m.verbose = False
    m.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in sd.items()})
    m.to('cuda:0')
    return m, sd


def _partition(kind, T, seed=0):
    if kind == 'whole':
        return [T]
    if kind == 'ones':
        return [1] * T
    if kind == 'two':
        return [2, T - 2]
    rng = np.random.Generator(np.random.PCG64(seed))
    sizes = []
    while sum(sizes) < T:
        sizes.append(int(min(rng.integers(0, 7), T - sum(sizes))))   # zero-frame pushes included
    sizes.insert(1, 0)
    return sizes


@pytest.mark.parametrize('B', [1, 3])
@pytest.mark.parametrize('mode,variant', [('RAW', 'peaky'), ('RAW', 'default'), ('MOL', 'default')])
def test_stream_is_bit_exact_against_offline_for_any_partition(mode, variant, B):
    from tacotronv2_wavernn_chinese_amd import _cabi
    from tacotronv2_wavernn_chinese_amd.synth import make_mels
    m, _ = _model(mode, variant)
    T = 23
    mels = make_mels(31, B, T)
    seed = 1234567
    off = m.generate_raw(mels, False, 11000, 550, noise_mode='philox', seed=seed, kernel=_cabi.KERNEL_TEAM2)
    ol, os_ = off['labels'].cpu().numpy(), off['samples'].cpu().numpy()
    for kind in ('whole', 'ones', 'two', 'random'):
        sizes = _partition(kind, T, seed=B)
        lab, smp = _stream_raw(m, mels, sizes, seed=seed, kernel='team2')
        np.testing.assert_array_equal(lab, ol, err_msg=f'labels, partition {kind} {sizes}')
        np.testing.assert_array_equal(smp, os_, err_msg=f'samples, partition {kind} {sizes}')


@pytest.mark.parametrize('mode', ['RAW', 'MOL'])
def test_stream_waveform_equals_generate_after_the_same_manual_seed(mode, tmp_path):
    from tacotronv2_wavernn_chinese_amd.dsp import decode_mu_law
    from tacotronv2_wavernn_chinese_amd.synth import make_mels
    m, _ = _model(mode, 'peaky' if mode == 'RAW' else 'default')
    T = 30
    mels = make_mels(5, 1, T)
    torch.manual_seed(77)
    ref = m.generate(mels, str(tmp_path / 'off.wav'), False, 11000, 550, True)
    torch.manual_seed(77)
    parts = [p for p in m.generate_stream([mels[0, :, f:f + 4] for f in range(0, T, 4)], mu_law=True)]
    got = np.concatenate(parts)
    assert got.dtype == np.float64 and got.shape == ref.shape == ((T - 1) * HOP,)
    np.testing.assert_array_equal(got, ref)
    # a frame's audio leaves before the clip ends: everything but the held-back 21 hops came out of the pushes
    assert sum(p.size for p in parts[:-1]) == (T - 21) * HOP
    # tail='none': every decoded sample as soon as it exists, T * hop of them, untrimmed and unfaded
    seed = 99
    raw = m.generate_raw(mels, False, 11000, 550, seed=seed)['samples'].cpu().numpy().astype(np.float64)
    want = decode_mu_law(raw, m.n_classes, False)[0] if mode == 'RAW' else raw[0]
    got_none = np.concatenate(list(m.generate_stream([mels[0, :, f:f + 3] for f in range(0, T, 3)], seed=seed, tail='none')))
    assert got_none.shape == (T * HOP,)
    np.testing.assert_array_equal(got_none, want)


def test_a_push_longer_than_the_conditioning_segment():
    """configs[1] length (401 frames = 110 275 steps: several TEAM2 segments inside one push) in one push and in 8-frame pushes."""
    from tacotronv2_wavernn_chinese_amd import _cabi
    from tacotronv2_wavernn_chinese_amd.synth import make_mels
    m, _ = _model()
    T = 401
    mels = make_mels(3, 1, T)
    off = m.generate_raw(mels, False, 11000, 550, seed=5, kernel=_cabi.KERNEL_TEAM2)
    ol, os_ = off['labels'].cpu().numpy(), off['samples'].cpu().numpy()
    for sizes in ([T], [8] * (T // 8) + [T % 8]):
        lab, smp = _stream_raw(m, mels, sizes, seed=5)
        np.testing.assert_array_equal(lab, ol)
        np.testing.assert_array_equal(smp, os_)


def test_argmax_stream_equals_offline_and_the_oracle():
    from oracle import oracle as orc
    from tacotronv2_wavernn_chinese_amd import _cabi
    from tacotronv2_wavernn_chinese_amd.vocoder import WaveRNN
    from tacotronv2_wavernn_chinese_amd.synth import DEFAULT_DIMS
    from tests.golden_util import load_case
    from tests.parity_util import check_free_run_raw
    fx = load_case('raw_peaky_b1_t24')
    m = WaveRNN(**DEFAULT_DIMS, mode='RAW')
    m.verbose = False
    m.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in fx['state_dict'].items()})
    m.to('cuda:0')
    mels = fx['mels']
    off = m.generate_raw(mels, False, 11000, 550, noise_mode=_cabi.NOISE_ARGMAX, kernel=_cabi.KERNEL_TEAM2)
    lab, smp = _stream_raw(m, mels, [3, 0, 5, 1, 7, 8], noise_mode='argmax')
    np.testing.assert_array_equal(lab, off['labels'].cpu().numpy())
    np.testing.assert_array_equal(smp, off['samples'].cpu().numpy())
    om = orc.OracleModel(fx['state_dict'], fast=True)
    cm, ca = om.conditioning(mels)
    check_free_run_raw(lab.T, om.loop(cm, ca, orc.NOISE_ARGMAX))


def test_streams_and_offline_calls_interleaved_on_one_model_do_not_disturb_each_other():
    from tacotronv2_wavernn_chinese_amd import _cabi
    from tacotronv2_wavernn_chinese_amd.synth import make_mels
    m, _ = _model()
    T = 25
    ma, mb, mc = make_mels(1, 1, T), make_mels(2, 1, T), make_mels(3, 1, 30)
    ref_a = m.generate_raw(ma, False, 11000, 550, seed=11)['labels'].cpu().numpy()
    ref_b = m.generate_raw(mb, False, 11000, 550, seed=12)['labels'].cpu().numpy()
    ref_c = m.generate_raw(mc, False, 11000, 550, seed=13)['labels'].cpu().numpy()
    got = {'a': [], 'b': []}
    with m.stream(seed=11, raw=True) as sa, m.stream(seed=12, raw=True) as sb:
        for f in range(0, T, 5):
            got['a'].append(sa.push(ma[0, :, f:f + 5])['labels'].cpu().numpy())
            c = m.generate_raw(mc, False, 11000, 550, seed=13, kernel=_cabi.KERNEL_TEAM2)['labels'].cpu().numpy()
            np.testing.assert_array_equal(c, ref_c)
            got['b'].append(sb.push(mb[0, :, f:f + 5])['labels'].cpu().numpy())
        got['b'].append(sb.finish()['labels'].cpu().numpy())
        got['a'].append(sa.finish()['labels'].cpu().numpy())
    np.testing.assert_array_equal(np.concatenate(got['a'], axis=1), ref_a)
    np.testing.assert_array_equal(np.concatenate(got['b'], axis=1), ref_b)


def test_simple_kernel_stream_equals_offline_simple():
    from tacotronv2_wavernn_chinese_amd import _cabi
    from tacotronv2_wavernn_chinese_amd.synth import make_mels
    m, _ = _model()
    T = 24
    mels = make_mels(8, 1, T)
    off = m.generate_raw(mels, False, 11000, 550, seed=21, kernel=_cabi.KERNEL_SIMPLE)
    lab, smp = _stream_raw(m, mels, [5] * 4 + [4], seed=21, kernel='simple')
    np.testing.assert_array_equal(lab, off['labels'].cpu().numpy())
    np.testing.assert_array_equal(smp, off['samples'].cpu().numpy())


def test_workspace_is_bounded_by_the_push_not_the_stream():
    from tacotronv2_wavernn_chinese_amd.synth import make_mels
    m, _ = _model()
    T = 2000
    mels = make_mels(4, 1, T)
    off = m.generate_raw(mels, False, 11000, 550, seed=3)['labels'].cpu().numpy()
    labs, ws = [], []
    with m.stream(seed=3, raw=True) as st:
        for f in range(0, T, 5):
            labs.append(st.push(mels[0, :, f:f + 5])['labels'])
            ws.append(st.info()['workspace_bytes'])
        labs.append(st.finish()['labels'])
        info = st.info()
    assert info['frames_in'] == T and info['steps_done'] == T * HOP
    assert len(set(ws[8:])) == 1, f'workspace grew after the first pushes: {sorted(set(ws))}'
    assert ws[-1] < 64 << 20, ws[-1]
    np.testing.assert_array_equal(torch.cat(labs, dim=1).cpu().numpy(), off)


def test_stream_error_contract(tmp_path):
    from tacotronv2_wavernn_chinese_amd import _cabi
    from tacotronv2_wavernn_chinese_amd.synth import make_mels
    m, _ = _model()
    mels = make_mels(6, 1, 22)
    st = m.stream(seed=1)
    st.push(mels[0])
    st.finish()
    with pytest.raises(_cabi.WrnnError) as ei:
        st.push(mels[0, :, :2])
    assert ei.value.code == -3
    st.close()
    with m.stream(seed=1) as st2:
        with pytest.raises(ValueError):
            st2.push(mels[0, :40])                    # wrong n_mels
        with pytest.raises(ValueError):
            st2.push(np.zeros((2, 80, 3), np.float32))   # wrong batch
    for nm in ('injected', 'reference'):
        with pytest.raises(ValueError):
            m.stream(noise_mode=nm)
    with pytest.raises(ValueError):
        m.stream(batched=True)
    with m.stream(seed=2) as st3:
        st3.push(mels[0, :, :20])
        with pytest.raises(ValueError, match='could not be broadcast'):
            st3.finish()
    with pytest.raises(ValueError, match='could not be broadcast'):   # generate() raises the same for T < 21
        m.generate(mels[:, :, :20], str(tmp_path / 'short.wav'), False, 11000, 550, True)


def test_cli_stream_frames_writes_the_unbatched_wav(tmp_path):
    """wavernn_gen.py --stream-frames N: the same wav as the unbatched path for the same --seed, plus the latency line."""
    import os
    import subprocess
    import sys
    from scipy.io import wavfile
    from tests.golden_util import load_case
    fx = load_case('raw_peaky_b1_t24')
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    ckpt = tmp_path / 'latest_weights.pyt'
    torch.save({k: torch.from_numpy(np.array(v)) for k, v in fx['state_dict'].items()}, ckpt)
    mel = tmp_path / 'mel-000.npy'
    np.save(mel, fx['mels'][0].T)
    out = tmp_path / 'wavernn_inference_output' / 'mel-000_gen_NOT_BATCHED_step=0k.wav'
    wavs = []
    for extra in ([], ['--stream-frames', '4']):
        r = subprocess.run([sys.executable, os.path.join(root, 'wavernn_gen.py'), '--file', str(mel), '-w', str(ckpt), '-u', '--seed', '5'] + extra,
                           cwd=tmp_path, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        wavs.append(wavfile.read(out)[1])
        out.unlink()
    assert 'first audio after' in r.stdout and 'real-time factor' in r.stdout, r.stdout[-1000:]
    assert wavs[0].shape == ((24 - 1) * HOP,)
    np.testing.assert_array_equal(wavs[1], wavs[0])
