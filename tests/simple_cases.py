"""The dim sets WRNN_KERNEL_SIMPLE, the any-shape loop kernel, is tested at (tests/test_simple_cases_host.py, tests/test_gpu_simple_dims.py), with
the inputs and the oracle runs both files share.  Nothing here touches a GPU.

S1  rnn 520 / fc 520, 128 classes      threads 0..7 own two hidden units (and two fc rows), the rest one; A = 5; fewer classes than threads
S2  teamg_cases C, 1024 / 1024, 10 bit  every thread owns two units, two fc rows and two classes
S3  rnn 3 / fc 2, 2 classes             the minimum of every field wrnn_dims_from_config admits; pad 1 (3 taps); res_out 4 > compute 1
S3b the dims of S3 under weight seed 12   seed 7 leaves both ReLUs of S3 dead at every step (its logits are fc3's bias); here the logits move
S4  rnn 64 / fc 32, 32 768 classes      64 classes per thread, Philox class indices past 1024, 132 992 B of dynamic LDS (above 64 KB)
S5  rnn 1000 / fc 600, pad 3, hop 12    threads 0..487 own two units, 488..511 one; 7 taps over three upsample layers; A = 18

Weights make_state_dict(7, mode, 'peaky' for RAW else 'default'), mels make_mels(3, 3, T), one PCG64(8) generator for the injected noise: on these
the C oracle's own free run has no race margin below NEAR_TIE / NEAR_TIE_MOL (asserted by the host file), so the parity rules excuse nothing.
"""
import numpy as np

from tests.teamg_cases import DIM_SETS as _TEAMG_SETS

_SMALL = dict(bits=7, pad=2, upsample_factors=(2, 3), feat_dims=13, compute_dims=16, res_out_dims=20, res_blocks=1, hop_length=6, sample_rate=16000)
DIM_SETS = {
    'S1': dict(_SMALL, rnn_dims=520, fc_dims=520),
    'S2': dict(_TEAMG_SETS['C']),
    'S3': dict(rnn_dims=3, fc_dims=2, bits=1, pad=1, upsample_factors=(2,), feat_dims=1, compute_dims=1, res_out_dims=4, res_blocks=1,
               hop_length=2, sample_rate=16000),
    'S4': dict(_SMALL, rnn_dims=64, fc_dims=32, bits=15),
    'S5': dict(rnn_dims=1000, fc_dims=600, bits=9, pad=3, upsample_factors=(2, 2, 3), feat_dims=21, compute_dims=40, res_out_dims=72,
               res_blocks=2, hop_length=12, sample_rate=16000),
}
DIM_SETS['S3b'] = dict(DIM_SETS['S3'])
FRAMES = {'S1': 20, 'S2': 20, 'S3': 20, 'S3b': 20, 'S4': 2, 'S5': 20}
CASES = [(s, 'RAW') for s in ('S1', 'S2', 'S3', 'S3b', 'S4', 'S5')] + [(s, 'MOL') for s in ('S1', 'S2', 'S5')]
B = 3
WEIGHT_SEED, MEL_SEED, NOISE_SEED = 7, 3, 8
WEIGHT_SEEDS = {'S3b': 12}                   # every other set: WEIGHT_SEED
PHILOX_SEED = 0x5EED0A0B0000C0DE            # both 32-bit words of the key non-zero
PHILOX_CASES = [('S1', 'RAW'), ('S1', 'MOL'), ('S4', 'RAW')]
UTT_SEEDS = [0x1234567, 0xFEDCBA9800000000 + 0x1234567, 0x7700000077]
RAGGED_FRAMES = (20, 1, 7)                   # S5: the longest first, a one-frame row (shorter than the 3-frame look-ahead), a middle one
FOLD_TARGET, FOLD_OVERLAP = 50, 7            # S5: folds start every 57 positions, hop 12; 64 steps each
FOLD_FRAMES = (20, 9)
FOLD_SEED = 0xF01D000500000051
TIE_PAIRS = [(5, 517), (70, 200), (100, 522)]   # S2, class c -> thread c % 512: same thread; waves 1 and 3; the higher index in wave 0 lane 10
TIE_FRAMES = 4
STREAM_CHUNKS = (1, 7, 3, 9)
LDS_LIMIT = 160 * 1024

_SD, _OM, _CASE, _G64 = {}, {}, {}, {}


def n_classes(name, mode):
    return 2 ** DIM_SETS[name]['bits'] if mode == 'RAW' else 30


def simple_lay_bytes(dims, mode='RAW'):
    """`SimpleLay(d).total * sizeof(float)` of csrc/loop_simple.hip restated: the dynamic LDS of the kernel for these dims."""
    H, FC, F, R = dims['rnn_dims'], dims['fc_dims'], dims['feat_dims'], dims['res_out_dims']
    A, NC = R // 4, (2 ** dims['bits'] if mode == 'RAW' else 30)
    r4 = lambda n: (n + 3) & ~3
    floats = r4(1 + F + A) + r4(R) + 3 * r4(H) + 2 * r4(H + A) + r4(FC + A) + r4(FC) + r4(NC) + 32
    return 4 * floats


def state_dict(name, mode):
    if (name, mode) not in _SD:
        from tacotronv2_wavernn_chinese_amd.synth import make_state_dict
        _SD[name, mode] = make_state_dict(WEIGHT_SEEDS.get(name, WEIGHT_SEED), mode, 'peaky' if mode == 'RAW' else 'default', **DIM_SETS[name])
    return _SD[name, mode]


def oracle_of(sd, name, mode):
    from oracle import oracle as orc
    d = DIM_SETS[name]
    return orc.OracleModel(sd, mode=mode, bits=d['bits'], upsample_factors=d['upsample_factors'], pad=d['pad'], fast=True)


def oracle_model(name, mode):
    if (name, mode) not in _OM:
        _OM[name, mode] = oracle_of(state_dict(name, mode), name, mode)
    return _OM[name, mode]


def mels_of(name, seed=MEL_SEED, rows=B, T=None):
    from tacotronv2_wavernn_chinese_amd.synth import make_mels
    return make_mels(seed, rows, FRAMES[name] if T is None else T, feat_dims=DIM_SETS[name]['feat_dims'])


def oracle_loop(om, mode, cm, ca, noise, **kw):
    from oracle import oracle as orc
    if mode == 'RAW':
        return om.loop(cm, ca, orc.NOISE_EXPO, noise[0], **kw)
    return om.loop(cm, ca, 0, noise[0], noise[1], **kw)


def case(name, mode):
    """Mels, injected noise, the oracle's conditioning and its free + teacher-forced runs of one (dim set, mode), computed once."""
    key = (name, mode)
    if key not in _CASE:
        om = oracle_model(name, mode)
        T, hop = FRAMES[name], DIM_SETS[name]['hop_length']
        L = T * hop
        mels = mels_of(name)
        rng = np.random.Generator(np.random.PCG64(NOISE_SEED))
        if mode == 'RAW':
            noise = (rng.standard_exponential((L, B, n_classes(name, mode))).astype(np.float32),)
        else:
            noise = (rng.uniform(1e-5, 1 - 1e-5, size=(L, B, 10)).astype(np.float32), rng.uniform(1e-5, 1 - 1e-5, size=(L, B)).astype(np.float32))
        cm, ca = om.conditioning(mels)
        free = oracle_loop(om, mode, cm, ca, noise)
        forced = oracle_loop(om, mode, cm, ca, noise, x_forced=free['samples'], want_logits=True)
        _CASE[key] = dict(mels=mels, noise=noise, cm=cm, ca=ca, free=free, forced=forced, L=L, T=T, hop=hop)
    return _CASE[key]


def float64_logits(name, mode):
    """(L, B, NC) float64 logits along the oracle's own trajectory of case(name, mode): oracle/torch_ref.float64_logits_at per row, on the CPU."""
    key = (name, mode)
    if key not in _G64:
        from oracle import torch_ref
        c, d = case(name, mode), DIM_SETS[name]
        rows = [torch_ref.float64_logits_at(state_dict(name, mode), c['mels'][b], c['free']['samples'][:, b], range(c['L']), pad=d['pad'], device='cpu',
                                            upsample_factors=d['upsample_factors']) for b in range(B)]
        _G64[key] = np.stack(rows, axis=1)
    return _G64[key]


def logit_bound(name, mode):
    """(bound, g): the bound tests/test_gpu_teamg.py uses for 1024-wide sums, 2e-5 * max(1, max |oracle logits|), unless the fp32 oracle itself is
    further than an eighth of it from float64 -- g = max |oracle fp32 - float64| along the same forced trajectory -- then 8 g: both fp32 sums are
    legitimate orderings of the same terms.  Taken from the reference side alone."""
    lg = case(name, mode)['forced']['logits']
    g = float(np.abs(lg.astype(np.float64) - float64_logits(name, mode)).max())
    return max(2e-5 * max(1.0, float(np.abs(lg).max())), 8.0 * g), g


def float64_conditioning(name, mode):
    """(up, aux) of case(name, mode)'s mels in float64: `upsample_torch` on a .double() CPU copy of the model in eval()."""
    import torch
    from tacotronv2_wavernn_chinese_amd.vocoder import WaveRNN
    d = DIM_SETS[name]
    m = WaveRNN(**d, mode=mode)
    m.verbose = False
    m.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in state_dict(name, mode).items()})
    m = m.double().eval()
    with torch.no_grad():
        x = torch.nn.functional.pad(torch.from_numpy(case(name, mode)['mels']).double(), (d['pad'], d['pad']))
        up, aux = m.upsample_torch(x)
    return up.numpy(), aux.numpy()


def conditioning_bounds(name, mode):
    """((atol_up, g_up), (atol_aux, g_aux)): the atol of tests/test_gpu_any_dims.py (3e-6, 2e-5) or 8 g where the fp32 oracle's own distance g from
    float64 asks for more."""
    c = case(name, mode)
    up64, aux64 = float64_conditioning(name, mode)
    g_up, g_aux = float(np.abs(c['cm'] - up64).max()), float(np.abs(c['ca'] - aux64).max())
    return (max(3e-6, 8 * g_up), g_up), (max(2e-5, 8 * g_aux), g_aux)


# ---- device Philox noise, replayed (tests/philox_ref.py) -------------------------------------------------------------------------------

def philox_noise(mode, seed, L, rows, nc, n_rows=None):
    """What the kernel draws for steps [0, L) and the GLOBAL rows `rows` under the call-wide `seed`, as the oracle consumes it."""
    from tests import philox_ref
    rows = list(rows)
    if mode == 'RAW':
        u = philox_ref.philox_uniform_raw(seed, L, (max(rows) + 1) if n_rows is None else n_rows, nc)[:, rows]
        return (np.ascontiguousarray((-np.log(u.astype(np.float64))).astype(np.float32)),)
    return philox_ref.philox_mol_uniforms(seed, 0, L, rows)


def philox_case(name, mode):
    """case(name, mode) with the replayed Philox draws of PHILOX_SEED in place of the injected noise: the oracle's free run."""
    key = (name, mode, 'philox')
    if key not in _CASE:
        c, om = case(name, mode), oracle_model(name, mode)
        noise = philox_noise(mode, PHILOX_SEED, c['L'], range(B), n_classes(name, mode))
        _CASE[key] = dict(c, noise=noise, free=oracle_loop(om, mode, c['cm'], c['ca'], noise), forced=None)
    return _CASE[key]


# ---- S5 RAW: ragged rows and folds -------------------------------------------------------------------------------------------------------

def ragged_case():
    """S5 RAW, frames (20, 1, 7) of the case's mels, right-zero-padded, with the case's injected noise: per row the oracle on that clip alone."""
    key = 'ragged'
    if key not in _CASE:
        c, om, hop = case('S5', 'RAW'), oracle_model('S5', 'RAW'), DIM_SETS['S5']['hop_length']
        mels = c['mels'].copy()
        refs = []
        for b, t in enumerate(RAGGED_FRAMES):
            mels[b, :, t:] = 0.0
            cm, ca = om.conditioning(mels[b:b + 1, :, :t])
            q = np.ascontiguousarray(c['noise'][0][:t * hop, b:b + 1])
            refs.append(dict(q=q, free=oracle_loop(om, 'RAW', cm, ca, (q,))))
        _CASE[key] = dict(mels=mels, refs=refs, noise=c['noise'], hop=hop)
    return _CASE[key]


def fold_case():
    """S5 RAW folds at target 50 / overlap 7 of two clips (20 and 9 frames; the first is the case's row 0), Philox noise of FOLD_SEED keyed by the
    GLOBAL row: per clip the oracle's folds and its free run on them.  fold0 = the first global row of each clip."""
    key = 'fold'
    if key not in _CASE:
        c, om, hop = case('S5', 'RAW'), oracle_model('S5', 'RAW'), DIM_SETS['S5']['hop_length']
        steps = FOLD_TARGET + 2 * FOLD_OVERLAP
        clips = [c['mels'][0], mels_of('S5', seed=31, rows=1, T=FOLD_FRAMES[1])[0]]
        assert clips[0].shape[1] == FOLD_FRAMES[0]
        folds, fold0 = [], [0]
        for clip in clips:
            cm, ca = om.conditioning(clip[None])
            folds.append((om.fold(cm, FOLD_TARGET, FOLD_OVERLAP), om.fold(ca, FOLD_TARGET, FOLD_OVERLAP)))
            fold0.append(fold0[-1] + folds[-1][0].shape[0])
        refs = []
        for b, (fm, fa) in enumerate(folds):
            q = philox_noise('RAW', FOLD_SEED, steps, range(fold0[b], fold0[b + 1]), n_classes('S5', 'RAW'), n_rows=fold0[-1])
            refs.append(dict(fm=fm, fa=fa, q=q[0], free=oracle_loop(om, 'RAW', fm, fa, q)))
        batch = np.zeros((2, clips[0].shape[0], FOLD_FRAMES[0]), np.float32)
        for b, clip in enumerate(clips):
            batch[b, :, :clip.shape[1]] = clip
        _CASE[key] = dict(clips=clips, batch=batch, fold0=fold0, steps=steps, refs=refs, hop=hop)
    return _CASE[key]


# ---- S2 RAW: exact ties ------------------------------------------------------------------------------------------------------------------

def tie_state_dict(c1, c2):
    """S2 RAW weights with class c2 an exact copy of class c1 in fc3 and +50 on both biases: the two logits are the same fp32 sum of the same
    terms at every step, and far above the rest."""
    sd = dict(state_dict('S2', 'RAW'))
    w, b = np.array(sd['fc3.weight'], np.float32), np.array(sd['fc3.bias'], np.float32)
    w[c2], b[c2] = w[c1], b[c1]
    b[c1] += np.float32(50.0)
    b[c2] += np.float32(50.0)
    assert b[c1] == b[c2]
    sd['fc3.weight'], sd['fc3.bias'] = w, b
    return sd


# ---- streams: csrc/stream.hip's buffers restated -----------------------------------------------------------------------------------------

def stream_buffer_bytes(dims, rows, chunks):
    """Bytes of the buffers a SIMPLE stream has grown (mel history x 2, window, per-frame aux) after each push of `chunks` frames and after the
    last, empty one: wrnn_stream_push restated.  Each buffer is as large as the largest push so far needed it, never larger."""
    hop, P, F, R = dims['hop_length'], dims['pad'], dims['feat_dims'], dims['res_out_dims']
    frames_in = steps = cur = 0
    hist, win, aux, out = [0, 0], 0, 0, []
    for k, last in [(k, False) for k in chunks] + [(0, True)]:
        fin = frames_in + k
        ready = fin * hop if last else max((fin - P) * hop, 0) & ~31
        s0, s1 = steps, max(ready, steps)
        if s1 > s0:
            f0, f1 = s0 // hop, -(-s1 // hop)
            win, aux = max(win, rows * F * (f1 - f0 + 2 * P)), max(aux, rows * (f1 - f0) * R)
        if not last:
            keep0 = min(max(s1 // hop - P, 0), fin)
            cur = 1 - cur
            hist[cur] = max(hist[cur], rows * F * max(fin - keep0, 1))
        frames_in, steps = fin, s1
        out.append(4 * (hist[0] + hist[1] + win + aux))
    return out
