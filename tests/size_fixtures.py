"""Fixtures of the size sweeps: the dual-softmax model at every size the library dispatches differently
(tests/test_gpu_dm_sizes.py) and RAW at 256, 32 and 2 classes (tests/test_gpu_baseline_sizes.py).

These tests demand EXACT equality with the oracle at every step -- no near-tie allowance, no stopping at a first
divergence.  That rests on a property of the fixtures which tests/test_size_fixtures_host.py asserts on the CPU: over
the whole run the oracle's own race margin (relative gap of the two best p / q scores) never falls below MIN_MARGIN
= 1e-4, the near-tie bound of tests/test_deepmind.py and five times parity_util.NEAR_TIE; two correct fp32
evaluations differ by ~1e-6 there.  The seeds below were picked by that margin of the ORACLE alone (the first seed,
counting up from 11 / from the base Philox seed, whose run clears 2e-4); nothing here was chosen by looking at what
a kernel returns.  A fixture that drifts below the bound fails the CPU test; no GPU case is dropped for a tie.
"""
from __future__ import annotations

import functools

import numpy as np

from oracle import oracle as orc
from tacotronv2_wavernn_chinese_amd.synth import make_dm_state_dict, make_mels, make_state_dict

MIN_MARGIN = 1e-4

# ------------------------------------------------------------------------------------------------ dual-softmax model
DM_STEPS = 1000            # not a multiple of 64: the team kernel's 64-step bail-out check ends mid-block
DM_WEIGHT_SEED = 0
PHILOX_BASE = 0x0D0C0B0A00C0FFEE   # both key words set
PHILOX_STEP = 0x0000000100000001

# (hidden, quantisation) -> (PCG64 seed of the injected Exp(1) draws, device Philox seed)
DM_SEEDS = {
    (512, 256): (11, PHILOX_BASE),
    (640, 256): (11, PHILOX_BASE),
    (768, 256): (11, PHILOX_BASE),
    (896, 256): (13, PHILOX_BASE),
    (512, 64): (12, PHILOX_BASE),
    (640, 128): (11, PHILOX_BASE),
    (768, 192): (12, PHILOX_BASE),
    (896, 64): (13, PHILOX_BASE + PHILOX_STEP),
    (64, 256): (11, PHILOX_BASE + PHILOX_STEP),
    (130, 37): (11, PHILOX_BASE),
    (1024, 256): (11, PHILOX_BASE),
    (2, 2): (11, PHILOX_BASE),
}
# team kernel: every template instantiation (CPL = hidden / 64 = 8, 10, 12, 14) at 256 classes, and every other
# class count (QW = quantisation / 32 = 2, 4, 6) once, spread over the hidden sizes
DM_TEAM_CASES = [(512, 256), (640, 256), (768, 256), (896, 256), (512, 64), (640, 128), (768, 192), (896, 64)]
# single-workgroup kernel: its limits (hidden 2 and 1024, quantisation 2 and 256), sizes that are no multiple of a
# wave (hidden 130 -> split 65, quantisation 37), and one size both kernels run against one oracle pass
DM_SINGLE_CASES = [(64, 256), (130, 37), (1024, 256), (2, 2), (512, 64)]
DM_NOISE_MODES = ['injected', 'philox']
# the reload check: the (640, 128) weights with R and O2 replaced by those of another seed
DM_RELOAD_CASE, DM_RELOAD_WEIGHT_SEED, DM_RELOAD_KEYS, DM_RELOAD_NOISE_SEED = (640, 128), 1, ('R.weight', 'O2.weight'), 11


def dm_distinct_bound(Q: int) -> float:
    """A run must show MORE than this many distinct coarse and fine values: a collapsed sampler cannot pass."""
    return min(20, Q / 2)


def _freeze(d: dict) -> dict:
    for v in d.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return d


def dm_state_dict(H: int, Q: int, reload: bool = False):
    sd = make_dm_state_dict(DM_WEIGHT_SEED, hidden_size=H, quantisation=Q)
    if reload:
        other = make_dm_state_dict(DM_RELOAD_WEIGHT_SEED, hidden_size=H, quantisation=Q)
        for k in DM_RELOAD_KEYS:
            sd[k] = other[k]
    return sd


def dm_draws(H: int, Q: int, noise: str, reload: bool = False):
    """(seed, q): q (DM_STEPS, 2, Q) float32 Exp(1) draws as DeepmindOracle.generate consumes them."""
    pcg, phx = DM_SEEDS[(H, Q)]
    if reload:
        pcg = DM_RELOAD_NOISE_SEED
    if noise == 'injected':
        return pcg, np.random.Generator(np.random.PCG64(pcg)).standard_exponential((DM_STEPS, 2, Q)).astype(np.float32)
    from tests.philox_ref import philox_dm_exponentials
    return phx, philox_dm_exponentials(phx, 0, DM_STEPS, quant=Q)


@functools.lru_cache(maxsize=None)
def dm_fixture(H: int, Q: int, noise: str, reload: bool = False, fast: bool = True) -> dict:
    """One oracle run per (size, noise mode), shared by every test that needs it and left unchanged (read-only arrays)."""
    sd = dm_state_dict(H, Q, reload)
    seed, q = dm_draws(H, Q, noise, reload)
    ref = orc.DeepmindOracle(sd, fast=fast).generate(DM_STEPS, q)
    return _freeze(dict(state_dict=sd, seed=seed, q=q, min_margin=float(ref['margin'].min()), **ref))


# --------------------------------------------------------------------------------------------------- RAW class counts
RAW_BITS = [8, 5, 1]       # 256 classes: workgroups 8..31 own none; 32: workgroup 0 only; 2: one quarter-wave, `cls0 + 4` never valid
RAW_WEIGHT_SEED, RAW_MEL_SEED, RAW_FRAMES = 3, 55, 4      # 4 frames = 1 100 steps per row
# (bits, rows) -> PCG64 seed of the injected Exp(1) draws
RAW_NOISE_SEEDS = {(8, 2): 11, (8, 5): 13, (5, 2): 11, (5, 5): 11, (1, 2): 11, (1, 5): 11}


def raw_rows(kernel: str) -> int:
    """Two rows on the one-row-per-team kernels; five on the batch kernels, so that a row quad is partly filled."""
    return 5 if kernel in ('batch', 'batch_cs') else 2


@functools.lru_cache(maxsize=None)
def raw_fixture(bits: int, B: int) -> dict:
    """Oracle free run, and the teacher-forced pass (with logits) on the oracle's own samples."""
    sd = make_state_dict(RAW_WEIGHT_SEED, variant='peaky', bits=bits)
    mels = make_mels(RAW_MEL_SEED, B, RAW_FRAMES)
    L, NC = RAW_FRAMES * 275, 2 ** bits
    q = np.random.Generator(np.random.PCG64(RAW_NOISE_SEEDS[(bits, B)])).standard_exponential((L, B, NC)).astype(np.float32)
    om = orc.OracleModel(sd, bits=bits, fast=True)
    cm, ca = om.conditioning(mels)
    free = om.loop(cm, ca, orc.NOISE_EXPO, q)
    forced = om.loop(cm, ca, orc.NOISE_EXPO, q, x_forced=free['samples'], want_logits=True)
    return dict(state_dict=sd, mels=mels, q=q, L=L, n_classes=NC, free=_freeze(free), forced=_freeze(forced),
                min_margin=float(min(free['margin'].min(), forced['margin'].min())))
