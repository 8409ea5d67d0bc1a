"""What sits between a dot product and its publish, and between a poll's first look and its landing, in the latency kernel's generated code
(no GPU needed; skipped where hipcc is absent).

Same extraction as tests/test_team2_isa.py: csrc/loop_team2.hip compiled for gfx950, the step loop of the shipped instantiation
loop_team2_kernel<RAW, false, false>, split at its five workgroup barriers (window k = B_k .. B_k+1).  Asserted of it:

  * windows B1..B5, every granule publish (each `global_store_dwordx2`, and the shadow waves' `ds_write` of gh2 into the hand-over slot): no
    `ds_read*` between the publish and the nearest `v_pk_fma_f32` in front of it.  The constants and hand-over values that are added behind a dot
    product are read AHEAD of it (T2_HOIST_LDS); a read that the compiler sinks behind the row sums is a dependent LDS round trip with its own
    `s_waitcnt lgkmcnt(0)` on the serial chain;
  * window B4..B5: one `ds_read` of the noise slots, in front of the window's first `v_pk_fma_f32` (one 8-byte read of both slots of the step's
    parity, classes a quarter does not own discarded by select -- not two reads in two `exec` branches behind the fc3 row sums);
  * windows B1..B4: no `v_mov_b64` between the first `sc1` look of an exchange and the barrier that closes it (T2_STRAIGHT_POLL: the poll loop has
    one load site, so the granule is no phi of a first look and a re-read, and neither the success path nor the retry copies it);
  * scratch of the shipped instantiation: at most the 104 bytes per lane it had before the reads were hoisted.

Measured (profiles/team2_chain_lds.txt; configs[1], interleaved repetitions per build and session, medians): the hoisted reads +3.3 .. +4.1 % against
the parent in five sessions; the one-site polls on top of them -0.1 % (inside the session's 0.5 % spread).  With -DT2_STRAIGHT_POLL=0 the poll
assertion finds 4 `v_mov_b64` per exchange window, as in the parent.
"""
from __future__ import annotations

import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'tacotronv2_wavernn_chinese_amd', 'csrc')
HIPCC = shutil.which('hipcc') or '/opt/rocm/bin/hipcc'
SHIPPED = '_Z17loop_team2_kernelILi0ELb0ELb0EEv12WrnnTeamArgs'   # <WRNN_MODE_RAW, PROF = false, RAGGED = false>
PARENT_SCRATCH = 104

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason='hipcc is not installed')


def _instructions(body: str) -> list[str]:
    out = []
    for line in body.split('\n'):
        s = line.split(';')[0].strip()
        if s and not s.startswith('.') or re.match(r'^\.LBB\d+_\d+:', s):
            out.append(s)
    return out


def _lds_bytes(name: str) -> int:
    """Byte offset of an LDS region of csrc/loop_team2.hip, from the carve-up's own constexpr lines."""
    env = {}
    for m in re.finditer(r'constexpr int (L_\w+) = ([^;]+);', open(os.path.join(CSRC, 'loop_team2.hip')).read()):
        env[m.group(1)] = eval(m.group(2), {'__builtins__': {}}, dict(env, XB_VEC=8 * 68))
    return 4 * env[name]


@pytest.fixture(scope='module')
def compiled(tmp_path_factory):
    asm = str(tmp_path_factory.mktemp('isa') / 'loop_team2.s')
    r = subprocess.run([HIPCC, '--offload-arch=gfx950', '-O3', '-std=c++17', '-Wno-pass-failed', '--cuda-device-only', '-S', 'loop_team2.hip', '-o', asm,
                        '-Rpass-analysis=kernel-resource-usage'], cwd=CSRC, check=True, capture_output=True, text=True)
    return open(asm).read(), r.stderr


@pytest.fixture(scope='module')
def windows(compiled) -> list[list[str]]:
    """[window 0 (phase A), window 1 (B1..B2), ..., window 4 (B4..B5), what follows B5]"""
    m = re.search(r'\n' + SHIPPED + r':[^\n]*\n(.*?)\n\s*s_endpgm', compiled[0], re.S)
    assert m, 'the shipped instantiation is not in the ISA'
    ins = _instructions(m.group(1))
    label = {s[:-1]: i for i, s in enumerate(ins) if s.endswith(':') and s.startswith('.LBB')}
    loops = []
    for i, s in enumerate(ins):
        mm = re.match(r'(?:s_cbranch_\w+|s_branch)\s+(\.LBB\d+_\d+)', s)
        if mm and label.get(mm.group(1), i) < i:
            loops.append((label[mm.group(1)], i))
    # the step loop: the innermost loop with at least five workgroup barriers.  A poll's retry block that the compiler lays out behind the loop and
    # that branches back into it spans barriers too, but it CROSSES the loop (starts inside, ends outside): not a loop of the nest
    crosses = lambda a, b: any(a2 < a < b2 < b for a2, b2 in loops)
    cand = [(b - a, a, b) for a, b in loops if sum(s == 's_barrier' for s in ins[a:b + 1]) >= 5 and not crosses(a, b)]
    assert cand, 'no loop with five barriers'
    _, a, b = min(cand)
    loop = ins[a:b + 1]
    cuts = [i for i, s in enumerate(loop) if s == 's_barrier'][:5]
    assert len(cuts) == 5
    return [loop[x + 1:y] for x, y in zip([-1] + cuts, cuts + [len(loop)])]


def _offset(s: str):
    m = re.search(r'\boffset:(\d+)', s)
    return int(m.group(1)) if m else None


def test_no_lds_read_between_a_dot_product_and_its_publish(windows):
    hand = _lds_bytes('L_HAND')
    publishes = 0
    for w in (1, 2, 3, 4):
        win = windows[w]
        for i, s in enumerate(win):
            gh2 = w == 4 and s.startswith('ds_write') and _offset(s) is not None and hand <= _offset(s) < hand + 12
            if not (s.startswith('global_store_dwordx2') or gh2):
                continue
            publishes += 1
            fma = max((j for j in range(i) if win[j].startswith('v_pk_fma_f32')), default=None)
            assert fma is not None, f'window B{w}: no dot product in front of `{s}`'
            between = [x for x in win[fma + 1:i] if x.startswith('ds_read')]
            print(f'window B{w}..B{w + 1}: `{s}`: {i - fma - 1} instructions behind the last v_pk_fma_f32, ds_read among them: {between}')
            assert not between, f'window B{w}..B{w + 1}: LDS reads between the dot product and `{s}`: {between}'
    # x3 + 3 x gh1 | fc1 | fc2 | the race candidate + gh2 -> the hand-over slot
    assert publishes >= 8, f'only {publishes} publishes found in the step loop'


def test_one_early_read_of_the_noise_slots(windows):
    hand = _lds_bytes('L_HAND')
    win = windows[4]
    # hand[4 + 2 * parity], hand[5 + 2 * parity]: the parity is in the address register, the slots' base in the offset field
    noise = [i for i, s in enumerate(win) if s.startswith('ds_read') and _offset(s) is not None and hand + 16 <= _offset(s) < hand + 32]
    first_fma = next(i for i, s in enumerate(win) if s.startswith('v_pk_fma_f32'))
    print(f'window B4..B5: noise-slot reads {[(i, win[i]) for i in noise]}, first v_pk_fma_f32 at {first_fma}')
    assert len(noise) == 1, f'expected one read of the noise slots, found {[win[i] for i in noise]}'
    assert noise[0] < first_fma, 'the noise slots are read behind the fc3 dot product'


def test_no_register_copies_between_a_look_and_its_barrier(windows):
    found = {}
    for w in (1, 2, 3):
        win = windows[w]
        look = next((i for i, s in enumerate(win) if re.search(r'\bsc1\b', s)), None)
        assert look is not None, f'window B{w}..B{w + 1}: no sc1 look'
        found[w] = [s for s in win[look:] if s.startswith('v_mov_b64')]
        print(f'window B{w}..B{w + 1}: {len(win) - look} instructions from the first look to the barrier, v_mov_b64 among them: {len(found[w])}')
    assert not any(found.values()), 'v_mov_b64 between the first look and the barrier: ' + ', '.join(f'B{w}..B{w + 1}: {len(c)}' for w, c in found.items())


def test_scratch_does_not_exceed_the_parents(compiled):
    blk = compiled[1].split('Function Name: ' + SHIPPED)[1].split('Function Name:')[0]
    scratch = int(re.search(r'ScratchSize \[bytes/lane\]: (\d+)', blk).group(1))
    print(f'loop_team2_kernel<RAW, false, false>: scratch {scratch} bytes per lane (before: {PARENT_SCRATCH})')
    assert scratch <= PARENT_SCRATCH
