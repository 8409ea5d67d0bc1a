"""The cases of the teacher-forced forward pass on pre-padded mels (tests/test_forward_cases_host.py, tests/test_gpu_forward_padded.py): the dim
sets, the inputs and the float64 reference both files share.  Nothing here touches a GPU.

`WaveRNN.forward(x, mels)` in eval() hands the loop kernels mels that carry `pad` REAL context frames on each side (mel_T = T + 2 pad,
mel_off = pad), feeds step 0 x[:, 0] and forces every later step.  The reference is oracle/torch_ref.upsample(training=False) followed by
oracle/torch_ref.loop_forward on .double() copies of the state dict: no golden, no GPU, any dims.

A, B, C, D   tests/teamg_cases.py
Bp1          B with pad 1: its factors (2, 3) reach 9 samples past an edge, more than the indent 1 * 6 -- wrnn_create refuses the set (the
             composite FIR is not shift-invariant there); the reference side is checked like every other set, the GPU file asserts the refusal
Bp1w         B with pad 1 and one upsample layer (6,): reach 6 = indent 6, the 3-tap form (ND = 2 pad + 1 = 3) is exact and the kernels run it
Bp3          B with pad 3: 7 taps
S1, S3b, S5  tests/simple_cases.py (S3b: weight seed 12; seed 7 leaves both ReLUs dead)
H256, H6, H1 the reference's loop dims with res_blocks 3 at hops 256 (4, 8, 8), 6 (2, 3) and 1 (1,), as tests/test_gpu_team_hops.py builds them

B = 3 rows (the batch stride of the padded layout shows from the second row on; three rows leave a TEAMG_BATCH batch of 2, 4 or 8 part
empty).  All T + 2 pad frames of `mels` are random.  RAW x: class values of random labels (never 0: n_classes - 1 is odd); MOL x: uniform
in (-1, 1).  Weights: synth.make_state_dict, 'peaky' for RAW, 'default' with fc3.weight times MOL_FC3_SCALE for MOL.  The bounds are the rules and constants of tests/simple_cases.py and tests/test_gpu_parity.py, taken from the reference side alone.
"""
import numpy as np

from tests.simple_cases import DIM_SETS as _SIMPLE_SETS
from tests.teamg_cases import DIM_SETS as _TEAMG_SETS
from tacotronv2_wavernn_chinese_amd.synth import DEFAULT_DIMS

HOPS = {'H256': (4, 8, 8), 'H6': (2, 3), 'H1': (1,)}


def _hop_dims(factors):
    return dict(DEFAULT_DIMS, upsample_factors=tuple(factors), hop_length=int(np.prod(factors)), res_blocks=3)


DIM_SETS = {n: dict(_TEAMG_SETS[n]) for n in 'ABCD'}
DIM_SETS['Bp1'] = dict(_TEAMG_SETS['B'], pad=1)
DIM_SETS['Bp1w'] = dict(_TEAMG_SETS['B'], pad=1, upsample_factors=(6,))
DIM_SETS['Bp3'] = dict(_TEAMG_SETS['B'], pad=3)
DIM_SETS.update({n: dict(_SIMPLE_SETS[n]) for n in ('S1', 'S3b', 'S5')})
DIM_SETS.update({n: _hop_dims(f) for n, f in HOPS.items()})

REFUSED = {'Bp1': 'upsample edge reach 9 exceeds indent 6'}      # wrnn_create's own words for the set
TEAMG_SETS = ('A', 'B', 'C', 'D', 'Bp1w', 'Bp3', 'S5')                # what TEAMG and TEAMG_BATCH run
BATCH_ROWS = (2, 4, 8)
# wrnn_teamg_batch_plan's refusals among (set, rows per team), the same in both modes and all three weight formats (asserted by the host file)
PLAN_REFUSED = {('C', 4), ('C', 8), ('D', 8), ('S5', 4), ('S5', 8)}
MOL_SETS = ('B', 'Bp3', 'D', 'S5', 'H1')
CASES = [(n, 'RAW') for n in DIM_SETS] + [(n, 'MOL') for n in MOL_SETS]
B = 3
COND_FRAMES = (1, 7, 9)       # every tap but one is context; inside one 8-frame tile of resnet_kernel; across a tile boundary
LOOP_FRAMES = {275: 3, 256: 3, 128: 5, 12: 9, 6: 9, 2: 9, 1: 33}   # by hop: L = T * hop <= 825
WEIGHT_SEED, MEL_SEED = 7, 3
WEIGHT_SEEDS = {'S3b': 12}
X_SEEDS = {'RAW': 5, 'MOL': 4}   # MOL: the first seed from 0 under which no row of the five cases draws an x[:, 0] too small to move step 0 by 1000 x the bound
# The mixture parameters of a 'default' model stay below 0.21, a fifth of the 1 that is the floor of the bound 2e-5 * max(1, max |output|): the
# comparison would be five times blunter against the signal than the RAW one, and x[:, 0] could not move step 0 by 1000 x the bound at any
# value in (-1, 1).  fc3.weight times 16 (an exact scaling) brings the largest output to 1.5 ... 2.3: the bound is the relative one, as for RAW.
MOL_FC3_SCALE = 16.0

_SD, _IN, _FWD, _COND = {}, {}, {}, {}


def dims(name, mode='RAW'):
    """Constructor dims of one (set, mode); MOL at the reference's loop dims runs 9 bits as in tests/test_gpu_team_hops.py and test_gpu_teamg.py."""
    d = dict(DIM_SETS[name])
    if mode == 'MOL' and (name == 'D' or name in HOPS):
        d['bits'] = 9
    return d


def n_classes(name, mode):
    return 2 ** dims(name, mode)['bits'] if mode == 'RAW' else 30


def loop_frames(name):
    return LOOP_FRAMES[DIM_SETS[name]['hop_length']]


def state_dict(name, mode):
    if (name, mode) not in _SD:
        from tacotronv2_wavernn_chinese_amd.synth import make_state_dict
        sd = make_state_dict(WEIGHT_SEEDS.get(name, WEIGHT_SEED), mode, 'peaky' if mode == 'RAW' else 'default', **dims(name, mode))
        if mode == 'MOL':
            sd['fc3.weight'] = (sd['fc3.weight'] * np.float32(MOL_FC3_SCALE)).astype(np.float32)
        _SD[name, mode] = sd
    return _SD[name, mode]


def inputs(name, mode, T=None):
    """dict(mels (B, F, T + 2 pad) all random, x (B, L) with x[:, 0] != 0, y (B, L) the targets of the loss, T, L), once per (set, mode, T)."""
    T = loop_frames(name) if T is None else T
    key = (name, mode, T)
    if key not in _IN:
        from tacotronv2_wavernn_chinese_amd.synth import make_mels
        d = dims(name, mode)
        L = T * d['hop_length']
        mels = make_mels(MEL_SEED, B, T + 2 * d['pad'], feat_dims=d['feat_dims'])
        rng = np.random.Generator(np.random.PCG64(X_SEEDS[mode]))
        if mode == 'RAW':
            nc = n_classes(name, mode)
            lab = rng.integers(0, nc, size=(B, L + 1))
            x, y = (2.0 * lab[:, :-1] / (nc - 1.0) - 1.0).astype(np.float32), lab[:, 1:].astype(np.int64)
        else:
            v = rng.uniform(-1.0, 1.0, size=(B, L + 1)).astype(np.float32)
            x, y = np.ascontiguousarray(v[:, :-1]), np.ascontiguousarray(v[:, 1:])
        assert (x[:, 0] != 0).all()
        _IN[key] = dict(mels=mels, x=x, y=y, T=T, L=L)
    return _IN[key]


def zero_context(mels, pad):
    """`mels` with its 2 pad context frames zeroed: what the unpadded call computes on the middle T frames."""
    out = mels.copy()
    out[:, :, :pad] = 0.0
    out[:, :, mels.shape[2] - pad:] = 0.0
    return out


def conditioning_of(sd, d, mels, dtype):
    """(up (B, L, F), aux (B, L, R)) of padded mels: oracle/torch_ref.upsample in eval mode, every operation in `dtype`."""
    import torch
    from oracle import torch_ref
    with torch.no_grad():
        t = {k: torch.as_tensor(np.asarray(v)).to(dtype) for k, v in sd.items() if np.asarray(v).dtype.kind == 'f'}
        up, aux = torch_ref.upsample(t, torch.as_tensor(mels).to(dtype), upsample_factors=d['upsample_factors'], pad=d['pad'], training=False)
    return up.numpy(), aux.numpy()


def forward_of(sd, d, mels, x, dtype):
    """(up, aux, logits (B, L, n_classes)) of the teacher-forced pass: torch_ref.upsample(training=False) then torch_ref.loop_forward."""
    import torch
    from oracle import torch_ref
    with torch.no_grad():
        t = {k: torch.as_tensor(np.asarray(v)).to(dtype) for k, v in sd.items() if np.asarray(v).dtype.kind == 'f'}
        up, aux = torch_ref.upsample(t, torch.as_tensor(mels).to(dtype), upsample_factors=d['upsample_factors'], pad=d['pad'], training=False)
        y = torch_ref.loop_forward(t, torch.as_tensor(x).to(dtype), up, aux)
    return up.numpy(), aux.numpy(), y.numpy()


def _forward(name, mode, dtype_name):
    import torch
    key = (name, mode, dtype_name)
    if key not in _FWD:
        c = inputs(name, mode)
        _FWD[key] = forward_of(state_dict(name, mode), dims(name, mode), c['mels'], c['x'], getattr(torch, dtype_name))
    return _FWD[key]


def float64_forward(name, mode):
    """(up64, aux64, logits64) of inputs(name, mode)."""
    return _forward(name, mode, 'float64')


def fp32_forward(name, mode):
    """The same in float32: used only to measure g, the reference's own distance from float64."""
    return _forward(name, mode, 'float32')


def bound_of(logits64, g):
    """2e-5 * max(1, max |logits64|), unless the fp32 reference itself is further than an eighth of it from float64: then 8 g."""
    return max(2e-5 * max(1.0, float(np.abs(logits64).max())), 8.0 * g)


def logit_bound(name, mode):
    """(bound, g): max(2e-5 * max(1, max |logits64|), 8 g), g = max |fp32 reference - float64 reference| over all (B, L, n_classes)."""
    l64, l32 = float64_forward(name, mode)[2], fp32_forward(name, mode)[2]
    g = float(np.abs(l32.astype(np.float64) - l64).max())
    return bound_of(l64, g), g


def float64_conditioning(name, T, dtype_name='float64'):
    """(up64, aux64) of inputs(name, 'RAW', T)['mels'] (the upsample network's weights do not depend on the mode)."""
    import torch
    key = (name, T, dtype_name)
    if key not in _COND:
        _COND[key] = conditioning_of(state_dict(name, 'RAW'), dims(name), inputs(name, 'RAW', T)['mels'], getattr(torch, dtype_name))
    return _COND[key]


def conditioning_bounds(name, T):
    """((atol_up, g_up), (atol_aux, g_aux)): the atol of tests/test_gpu_any_dims.py (3e-6, 2e-5) or 8 g where the fp32 reference's own distance g
    from float64 asks for more."""
    up64, aux64 = float64_conditioning(name, T)
    up32, aux32 = float64_conditioning(name, T, 'float32')
    g_up, g_aux = float(np.abs(up32.astype(np.float64) - up64).max()), float(np.abs(aux32.astype(np.float64) - aux64).max())
    return (max(3e-6, 8 * g_up), g_up), (max(2e-5, 8 * g_aux), g_aux)


def float64_loss(name, mode):
    """The training script's loss (torch_ref.loss_of) on logits64 and the targets of inputs(name, mode), in float64."""
    import torch
    from oracle import torch_ref
    y = inputs(name, mode)['y']
    yt = torch.as_tensor(y) if mode == 'RAW' else torch.as_tensor(y).double()
    return float(torch_ref.loss_of(mode, torch.as_tensor(float64_forward(name, mode)[2]), yt))
