"""Host side of the drop-in (no GPU): the reference's call surface, file formats and error behaviour."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import oracle as orc
from tacotronv2_wavernn_chinese_amd.synth import DEFAULT_DIMS, make_state_dict

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _model(mode='RAW'):
    from tacotronv2_wavernn_chinese_amd.vocoder import WaveRNN
    dims = dict(DEFAULT_DIMS)
    dims['bits'] = 10 if mode == 'RAW' else 9
    return WaveRNN(**dims, mode=mode)


def test_state_dict_layout_matches_the_contract(capsys):
    m = _model()
    assert 'Trainable Parameters: 4.744M' in capsys.readouterr().out      # num_params() print of the reference
    sd = m.state_dict()
    synth = make_state_dict(0)
    assert list(sd.keys()) == list(synth.keys()) and len(sd) == 148
    for k, v in sd.items():
        assert tuple(v.shape) == tuple(synth[k].shape), k
    assert m.n_classes == 1024 and _model('MOL').n_classes == 30
    assert m.get_step() == 0
    with pytest.raises(RuntimeError):
        from tacotronv2_wavernn_chinese_amd.vocoder import WaveRNN
        WaveRNN(**DEFAULT_DIMS, mode='XYZ')
    with pytest.raises(ValueError):          # forward(x, mels): x (B, L), mels (B, n_mels, T + 2*pad); shapes are checked before any device work
        m.forward(np.zeros((1, 275), np.float32), np.zeros((80, 5), np.float32))
    with pytest.raises(ValueError):
        m.forward(np.zeros((1, 100), np.float32), np.zeros((1, 80, 5), np.float32))
    assert m.get_step() == 0                 # a rejected call does not count as a step


def test_state_dict_and_default_init_equal_the_reference_module():
    """Same keys in the same order and bit-identical default initialisation under the same torch seed as the unmodified reference
    module (tests/golden/module_default_init.npz: sha256 of every tensor of its state_dict, `python -m oracle.make_golden module`)."""
    from oracle import make_golden as mg
    from tacotronv2_wavernn_chinese_amd.vocoder import WaveRNN
    z = np.load(os.path.join(ROOT, 'tests', 'golden', 'module_default_init.npz'))
    torch.manual_seed(mg.MODULE_INIT_SEED)
    sb = WaveRNN(*mg.MODULE_INIT_ARGS).state_dict()
    assert list(sb.keys()) == [str(k) for k in z['keys']]
    for k, h in zip(z['keys'], z['sha256']):
        assert mg.tensor_sha256(sb[str(k)].numpy()) == str(h), k


def test_load_is_strict_false_and_save_round_trips(tmp_path):
    m = _model()
    sd = {k: torch.from_numpy(np.array(v)) for k, v in make_state_dict(5).items()}
    partial = {k: v for k, v in sd.items() if not k.startswith('fc3')}
    partial['not_a_key'] = torch.zeros(3)
    p = tmp_path / 'w.pyt'
    torch.save(partial, p)
    before = m.fc3.weight.clone()
    m.load(p)                                      # strict=False: missing + unexpected keys are fine
    assert torch.equal(m.fc3.weight, before)
    assert torch.equal(m.I.weight, sd['I.weight'])
    m.save(p)
    again = torch.load(p)
    assert set(again.keys()) == set(m.state_dict().keys())


def test_generate_refuses_to_run_without_a_gpu(tmp_path):
    if torch.cuda.is_available():
        pytest.skip('GPU present')
    m = _model()
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        m.generate(np.zeros((1, 80, 21), np.float32), str(tmp_path / 'x.wav'), False, 11000, 550, True)


def test_epilogue_pieces_match_the_oracle_restatement():
    from tacotronv2_wavernn_chinese_amd.dsp import decode_mu_law, label_2_float
    m = _model()
    rng = np.random.default_rng(0)
    y = rng.uniform(-1, 1, (4, 2400))
    np.testing.assert_array_equal(m.xfade_and_unfold(y.copy(), 2000, 200), orc.xfade_and_unfold(y.copy(), 2000, 200))
    lab = rng.integers(0, 1024, 100).astype(np.float64)
    f = label_2_float(lab, 10)
    np.testing.assert_allclose(decode_mu_law(f, 1024, False), orc.decode_mu_law(f, 1024), rtol=0, atol=0)
    np.testing.assert_allclose(decode_mu_law(lab, 1024, True), orc.decode_mu_law(f, 1024), rtol=0, atol=1e-15)


def test_finish_host_is_the_inline_tail_it_replaced():
    """``_finish_host`` against the sequence generate(), generate_many() and the folded call each spelled out before they shared it:
    decode_mu_law -> xfade_and_unfold -> [:wave_len] -> last 20 hops times linspace(1, 0, 20 * hop), bit for bit in float64.  hop = 5,
    so that the three folds of the batched case (2 050 samples unfolded) are longer than the 20-hop fade."""
    from tacotronv2_wavernn_chinese_amd.dsp import decode_mu_law
    from tacotronv2_wavernn_chinese_amd.vocoder import WaveRNN
    m = WaveRNN(rnn_dims=16, fc_dims=16, bits=10, pad=2, upsample_factors=(5,), feat_dims=8, compute_dims=8, res_out_dims=8, res_blocks=1,
                hop_length=5, sample_rate=22050, mode='RAW')
    hop, target, overlap = m.hop_length, 550, 100
    rng = np.random.default_rng(7)
    for batched, shape, wave_len in ((False, (1, 21 * hop), 20 * hop), (True, (3, target + 2 * overlap), 3 * (target + overlap) + overlap - hop)):
        rows = rng.integers(-2, 3, shape).astype(np.float64)   # integer-valued and small: finite under the mu-law expansion
        for mu_law in (True, False):
            want = decode_mu_law(rows.copy(), m.n_classes, False) if mu_law else rows.copy()
            want = m.xfade_and_unfold(want, target, overlap) if batched else want[0]
            want = want[:wave_len]
            want[-20 * hop:] *= np.linspace(1, 0, 20 * hop)
            got = m._finish_host(rows.copy(), mu_law, batched, target, overlap, wave_len)
            assert got.dtype == np.float64 and got.shape == (wave_len,) and np.all(np.isfinite(got)) and np.any(got != 0)
            assert np.array_equal(got, want), (batched, mu_law)


def test_save_wav_is_a_float32_wav_at_the_sample_rate(tmp_path):
    from scipy.io import wavfile
    from tacotronv2_wavernn_chinese_amd.dsp import save_wav
    x = np.linspace(-0.5, 0.5, 1000)
    save_wav(x, tmp_path / 'a.wav', 22050)
    sr, data = wavfile.read(tmp_path / 'a.wav')
    assert sr == 22050 and data.dtype == np.float32
    np.testing.assert_array_equal(data, x.astype(np.float32))


def test_hparams_singleton_semantics(tmp_path):
    code = ("from tacotronv2_wavernn_chinese_amd.hparams import hparams as hp\n"
            "import sys\n"
            "try:\n    hp.bits\n    sys.exit(3)\nexcept AttributeError:\n    pass\n"
            "hp.configure()\n"
            "assert (hp.bits, hp.hop_length, hp.voc_upsample_factors, hp.voc_mode, hp.voc_target, hp.voc_overlap) == (10, 275, (5, 5, 11), 'RAW', 11000, 550)\n"
            "try:\n    hp.configure()\n    sys.exit(4)\nexcept RuntimeError:\n    pass\n")
    r = subprocess.run([sys.executable, '-c', code], cwd=ROOT, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_gen_from_file_validates_like_the_reference(tmp_path):
    code = (
        "import numpy as np, sys\n"
        "from tacotronv2_wavernn_chinese_amd.hparams import hparams as hp\n"
        "hp.configure()\n"
        "from tacotronv2_wavernn_chinese_amd.gen import gen_from_file\n"
        "class M:\n"
        "    def get_step(self): return 123456\n"
        "    def generate(self, mel, path, batched, target, overlap, mu_law):\n"
        "        print('CALL', tuple(mel.shape), path, batched, target, overlap, mu_law)\n"
        f"d = r'{tmp_path}'\n"
        "np.save(d + '/ok.npy', np.random.rand(33, 80).astype(np.float32))\n"
        "np.save(d + '/badshape.npy', np.random.rand(33, 79).astype(np.float32))\n"
        "np.save(d + '/badrange.npy', 2 * np.ones((33, 80), np.float32))\n"
        "gen_from_file(M(), d + '/ok.npy', d, False, 11000, 550)\n"
        "gen_from_file(M(), d + '/ok.npy', d, True, 2000, 200)\n"
        "for bad in ('badshape.npy', 'badrange.npy', 'x.txt', 'x.wav'):\n"
        "    try:\n        gen_from_file(M(), d + '/' + bad, d, False, 11000, 550)\n        sys.exit(5)\n"
        "    except ValueError:\n        pass\n")
    r = subprocess.run([sys.executable, '-c', code], cwd=ROOT, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr + r.stdout
    calls = [l for l in r.stdout.splitlines() if l.startswith('CALL')]
    # (1, n_mels, T) tensor, reference file-name pattern (wavernn_gen.py:35-39), hp.mu_law
    assert "(1, 80, 33)" in calls[0] and 'ok_gen_NOT_BATCHED_step=123k.wav' in calls[0] and calls[0].endswith('True')
    assert 'ok_gen_batched_target2000_overlap200_step=123k.wav' in calls[1]


def test_epilogue_tables_follow_numpy():
    """The float64 tables behind wrnn_epilogue (built on the host, no device needed) against NumPy evaluated the
    way fatchord_version.py:256,374-385 and dsp.py:98-103 evaluate them: linspace and sqrt bit-for-bit, the
    mu-law decode (pow) within 2 ulp."""
    from oracle import oracle as orc
    from tacotronv2_wavernn_chinese_amd._cabi import epilogue_tables
    for n_classes, overlap, hop in ((1024, 550, 275), (512, 101, 200), (1024, 0, 275)):
        dec, fin, fout, tail = epilogue_tables(n_classes, overlap, hop)
        np.testing.assert_array_equal(tail, np.linspace(1, 0, 20 * hop))
        if overlap:
            silence = overlap // 2
            t = np.linspace(-1, 1, overlap - silence, dtype=np.float64)
            np.testing.assert_array_equal(fin, np.concatenate([np.zeros(silence), np.sqrt(0.5 * (1 + t))]))
            np.testing.assert_array_equal(fout, np.concatenate([np.ones(silence), np.sqrt(0.5 * (1 - t))]))
        k = np.arange(n_classes, dtype=np.float32)
        fed_back = (np.float32(2.0) * k / np.float32(n_classes - 1.0) - np.float32(1.0)).astype(np.float64)   # :235
        want = orc.decode_mu_law(fed_back, n_classes)
        np.testing.assert_allclose(dec, want, rtol=4.5e-16, atol=1e-18)   # pow(); near 0 the "- 1" cancels
        assert dec[0] == -1.0 or abs(dec[0] + 1.0) < 1e-15


def test_fold_target_gives_at_most_one_fold_per_team():
    """target='per_xcd': the reference's fold count (:319-325) for the chosen target never exceeds the number of
    teams, and uses all of them once the clip is long enough."""
    from tacotronv2_wavernn_chinese_amd.vocoder import fold_target
    for n in (8, 4, 1):
        for T in (21, 30, 61, 401, 1200):
            for overlap in (100, 550):
                L = T * 275
                target = fold_target(L, overlap, n)
                num_folds, remaining = divmod(L - overlap, target + overlap)   # :319-322
                if remaining != 0:
                    num_folds += 1                                             # :324-325
                assert 1 <= num_folds <= n, (n, T, overlap, target, num_folds)
                if L >= n * 3 * overlap:
                    assert num_folds == n


def test_fold_plan_prices_the_fold_counts_like_the_library_runs_them():
    """target='auto' (round 6): the cost model behind it.  `fold_count` restates the reference's fold count (:319-325); `predicted_loop_us`
    mirrors WRNN_KERNEL_AUTO's row placement (api.hip: <= teams rows on the latency kernel, else ceil(rows / teams) <= 8 rows per team batch,
    batches back to back); `fold_plan` returns the cheapest count and reproduces the measured optimum of profiles/r06_fold_latency_raw.txt."""
    from tacotronv2_wavernn_chinese_amd.vocoder import STEP_US, fold_count, fold_plan, fold_target, predicted_loop_us
    for L, target, overlap in ((110275, 11000, 550), (8250, 2000, 200), (110275, 1165, 550), (5775, 550, 550), (30000, 29450, 550)):
        num_folds, remaining = divmod(L - overlap, target + overlap)
        assert fold_count(L, target, overlap) == num_folds + (1 if remaining else 0)
    assert fold_count(110275, 11000, 550) == 10 and fold_count(110275, 1165, 550) == 64
    us = STEP_US['RAW']
    assert predicted_loop_us(8, 1000, 8) == 1000 * us['team2']
    assert predicted_loop_us(10, 1000, 8) == 1000 * us['cs4']            # 2 rows per team in one quad
    assert predicted_loop_us(40, 1000, 8) == 1000 * us['cs8']            # 5 rows per team: two quads
    assert predicted_loop_us(80, 1000, 8) == 2 * 1000 * us['cs8']        # 10 batches of 8 rows on 8 teams: two passes
    assert predicted_loop_us(3, 1000, 1) == 1000 * us['cs4']             # a one-team device (CPX-like partition)
    target, folds, cost = fold_plan(401 * 275, 550, 8, 'RAW')
    assert (target, folds) == (1165, 64) and abs(cost - 2265 * us['cs8']) < 1e-6
    # min_target bounds the crossfade density from below; the latency optimum is what 0 gives
    t2, f2, c2 = fold_plan(401 * 275, 550, 8, 'RAW', min_target=5500)
    assert t2 >= 5500 and f2 < folds and c2 > cost and f2 == fold_count(401 * 275, t2, 550)
    assert fold_plan(21 * 275, 550, 8, 'RAW', min_target=10 ** 9)[1] == 1          # nothing admissible but one fold
    # the plan is never worse than one fold per team, never asks for a target below the overlap, and its count is what the reference's
    # fold arithmetic gives for the target
    for mode in ('RAW', 'MOL'):
        for n_teams in (8, 4, 1):
            for T in (21, 30, 61, 120, 401, 1200):
                for overlap in (100, 550):
                    L = T * 275
                    target, folds, cost = fold_plan(L, overlap, n_teams, mode)
                    assert target >= overlap and folds == fold_count(L, target, overlap) >= 1
                    t1 = fold_target(L, overlap, n_teams)
                    assert cost <= predicted_loop_us(fold_count(L, t1, overlap), t1 + 2 * overlap, n_teams, mode) + 1e-9


def test_reference_noise_is_the_stream_the_reference_consumes():
    """vocoder.reference_noise (PRODUCT code behind noise_mode='reference') against the test infrastructure's replay (oracle/noise.py), which the
    fixtures' checksums pin to the draws the unmodified reference consumed when the goldens were minted -- RAW and MOL, several rows, a
    chunk size that forces several host chunks."""
    import torch
    from oracle.noise import noise_checksum, noise_from_seed
    from tacotronv2_wavernn_chinese_amd.vocoder import reference_noise
    from tests.golden_util import GOLDEN_DIR
    for mode, rows, steps, nc in (('RAW', 1, 24 * 275, 1024), ('RAW', 3, 300, 1024), ('MOL', 1, 24 * 275, 30), ('MOL', 2, 500, 30)):
        want = noise_from_seed(42, mode, steps, rows)
        torch.manual_seed(42)
        n1, n2 = reference_noise(mode, rows, steps, nc, 512, 32, 'cpu', chunk_bytes=1 << 20)
        if mode == 'RAW':
            np.testing.assert_array_equal(n1.numpy(), np.maximum(want['expo'], np.float32(1.2e-38)))
            assert n2 is None
        else:
            np.testing.assert_array_equal(n1.numpy(), want['u_mix'])
            np.testing.assert_array_equal(n2.numpy(), want['u_log'])
    # ... and straight against a fixture's checksum of the reference's stream
    z = np.load(os.path.join(GOLDEN_DIR, 'raw_peaky_b1_t24.npz'))
    torch.manual_seed(int(z['noise_seed']))
    n1, _ = reference_noise('RAW', 1, 24 * 275, 1024, 512, 32, 'cpu')
    got = noise_checksum({'expo': n1.numpy()})
    if np.allclose(noise_checksum(noise_from_seed(int(z['noise_seed']), 'RAW', 24 * 275, 1)), z['noise_checksum'], rtol=0, atol=0):
        np.testing.assert_allclose(got, z['noise_checksum'], rtol=0, atol=0)   # (skipped where torch's CPU RNG differs from the minting build's)


def test_bench_launches_its_own_ranks(tmp_path):
    """`python bench.py --gpus 2` with no WORLD_SIZE around it must become the launcher (the driver's SCALE command): on this
    GPU-less box the ranks get as far as the device check and say so.  torchrun tears the sibling down as soon as the first rank
    exits 3, so only ONE such message is guaranteed (asking for both made this test fail 2 runs in 3 inside the full suite);
    that two ranks really start, meet and time together is tests/test_sharding.py's dry run of the same self-launch."""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k not in ('RANK', 'WORLD_SIZE', 'LOCAL_RANK')}
    r = subprocess.run([sys.executable, os.path.join(root, 'bench.py'), '--gpus', '2', '--steps', '1', '--warmup', '0'],
                       capture_output=True, text=True, timeout=600, env=env, cwd=tmp_path)
    import torch
    if torch.cuda.is_available() and torch.cuda.device_count() >= 2:
        assert r.returncode == 0, r.stderr[-2000:]
    else:
        assert r.returncode != 0
        assert r.stderr.count('no HIP device visible') >= 1 or 'invalid device ordinal' in r.stderr, r.stderr[-2000:]
        assert 'torch.distributed' in r.stderr or 'ChildFailedError' in r.stderr or 'exitcode' in r.stderr, r.stderr[-2000:]   # it WAS the launcher


def test_philox_replays_agree():
    """The numpy and the torch replay of the device RNG (tests/philox_ref.py) are two implementations of one specification:
    identical uniforms, strictly inside (0, 1)."""
    from tests.philox_ref import philox_uniform_raw, philox_uniform_raw_torch
    seed = 0x1234ABCD5678
    a = philox_uniform_raw(seed, 70, 3, 1024)
    b = philox_uniform_raw_torch(seed, 0, 70, [0, 1, 2]).numpy()
    np.testing.assert_array_equal(a, b)
    c = philox_uniform_raw_torch(seed, 33, 37, [2, 0]).numpy()
    np.testing.assert_array_equal(c, a[33:, [2, 0]])
    assert a.min() > 0.0 and a.max() < 1.0
    u_top = ((np.uint32(0xFFFFFFFF) >> np.uint32(9)).astype(np.float32) + np.float32(0.5)) * np.float32(1.0 / 8388608.0)
    assert u_top < 1.0


def test_counter_numbers_are_withheld_when_the_kernel_sources_changed(monkeypatch):
    """bench.py attaches HBM traffic and MFMA-busy cycles from a STATIC counter file (profiles/r05_pmc.json: rocprofv3 --pmc passes of one session) to
    its roofline objects.  The file records a hash of the kernel sources it was taken on; a tree whose sources hash differently gets null counters and the
    reason, not another kernel's numbers (round-4 review: the passes had been taken seven commits before the shipped kernel)."""
    import bench
    import warnings
    pmc = bench.load_pmc()
    if not pmc['ok']:   # round-5 advisor: a kernel or header edit must not fail a CPU test until somebody re-profiles; bench.py already degrades to null counters
        warnings.warn(f'bench.py will report null counter fields: {pmc["why"]} (re-run tools/profile_round.sh on the GPU box)')
    else:
        assert set(pmc['configs']) >= {1, 2, 4}
        for c in (2, 4):
            rec = pmc['configs'][c]
            assert 'loop_batch_cs_kernel' in rec['kernel'] and rec['mfma_busy_cycles_per_launch'] == 8 * rec['insts_mfma_per_launch']
            assert rec['fetch_bytes_per_launch'] > 0 and rec['kt_avg_ms'] > 0
    monkeypatch.setattr(bench, 'csrc_sha', lambda: '0' * 16)
    stale = bench.load_pmc()
    assert not stale['ok'] and stale['configs'] == {} and 'counters withheld' in stale['why']
