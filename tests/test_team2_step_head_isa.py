"""The head of the latency kernel's step, from barrier B5 (race result in LDS) to the first x2 read of phase B, in the generated code (no GPU needed;
skipped where hipcc is absent).

Same compile and window extraction as tests/test_team2_isa.py and tests/test_team2_chain_isa.py: csrc/loop_team2.hip for gfx950, the step loop of the
shipped instantiation loop_team2_kernel<RAW, false, false>, split at its five workgroup barriers.  "Between B5 and B1" is what follows B5 up to the
loop's back edge, then the loop top up to B1; the every-64-steps bail-out block (its own barrier, one LDS write and one LDS read) is not on the
per-step path and is cut out where the compiler lays it out inside the loop.  Asserted of the shipped build:

  * between B5 and B1 every `ds_read*` is issued in front of the first `s_waitcnt` that names `lgkmcnt`, and there are at least six of them: the
    fed-back sample and phase A's operands (L_CSTA, L_COND, three gh1 words) cost ONE LDS round trip (T2_HEAD_ONE_TRIP);
  * between B5 and B1 there is no `global_store*`: labels_out / samples_out are stored by a shadow wave of workgroup 0 in window B2..B3 of the
    next step (T2_OUT_SHADOW);
  * window B1..B2: no `ds_read_b96` / `ds_read2*` between the barrier and the first `ds_read_b128`: the phase-B operands that phase A does not
    produce were read with the step head (T2_PREB1_OPERANDS), the window opens with the x2 reads (one `ds_read_b32` of x2[unit] in front of them);
  * scratch of the shipped instantiation: at most 104 bytes per lane (the bound of tests/test_team2_chain_isa.py).

With each knob set to 0 (and the others as shipped) the matching assertion fails; that is asserted too, from one more compile per knob.  The parent
shows: `ds_read_b64` of {value, class}, `s_waitcnt lgkmcnt(0)`, the x_forced branch, two `global_store_dword` under an `exec` mask with 64-bit scalar
address arithmetic, the every-64-steps check, then at the loop top four more `ds_read*` and a second wait; window B1..B2 opens with `ds_read_b96`,
`ds_read_b96`, `ds_read2st64_b32` in front of the first `ds_read_b128`.

Measured: profiles/team2_step_head.txt.
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
SCRATCH_BOUND = 104
KNOBS = ('T2_HEAD_ONE_TRIP', 'T2_OUT_SHADOW', 'T2_PREB1_OPERANDS')

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason='hipcc is not installed')


def _instructions(body: str) -> list[str]:
    out = []
    for line in body.split('\n'):
        s = line.split(';')[0].strip()
        if s and not s.startswith('.') or re.match(r'^\.LBB\d+_\d+:', s):
            out.append(s)
    return out


def _windows(txt: str) -> list[list[str]]:
    """[window 0 (loop top .. B1), window 1 (B1..B2), ..., window 4 (B4..B5), what follows B5 up to the back edge]"""
    m = re.search(r'\n' + SHIPPED + r':[^\n]*\n(.*?)\n\s*s_endpgm', txt, re.S)
    assert m, 'the shipped instantiation is not in the ISA'
    ins = _instructions(m.group(1))
    label = {s[:-1]: i for i, s in enumerate(ins) if s.endswith(':') and s.startswith('.LBB')}
    loops = []
    for i, s in enumerate(ins):
        mm = re.match(r'(?:s_cbranch_\w+|s_branch)\s+(\.LBB\d+_\d+)', s)
        if mm and label.get(mm.group(1), i) < i:
            loops.append((label[mm.group(1)], i))
    crosses = lambda a, b: any(a2 < a < b2 < b for a2, b2 in loops)
    cand = [(b - a, a, b) for a, b in loops if sum(s == 's_barrier' for s in ins[a:b + 1]) >= 5 and not crosses(a, b)]
    assert cand, 'no loop with five barriers'
    _, a, b = min(cand)
    loop = ins[a:b + 1]
    cuts = [i for i, s in enumerate(loop) if s == 's_barrier'][:5]
    assert len(cuts) == 5
    return [loop[x + 1:y] for x, y in zip([-1] + cuts, cuts + [len(loop)])]


def _per_step(tail: list[str]) -> list[str]:
    """What follows B5 without the every-64-steps bail-out block, where that block lies inside the loop: it is entered by falling through the
    forward branch behind the `(t & 63) == 63` compare and holds the loop's sixth barrier."""
    bars = [i for i, s in enumerate(tail) if s == 's_barrier']
    if not bars:
        return tail
    assert len(bars) == 1, 'more than one barrier behind B5'
    br = max(i for i in range(bars[0]) if re.match(r's_cbranch_\w+\s+\.LBB\d+_\d+', tail[i]))
    assert any(re.match(r's_cmp_\w+_u64 s\[\d+:\d+\], 63$', s) for s in tail[:br]), 'the barrier behind B5 is not behind the every-64-steps check'
    target = tail[br].split()[-1] + ':'
    assert target in tail and tail.index(target) > bars[0], 'the branch behind the every-64-steps check does not skip the bail-out block'
    return tail[:br + 1] + tail[tail.index(target):]


def _head(w):
    return _per_step(w[5]) + w[0]


def late_reads(w) -> list[str]:
    """ds_read* between B5 and B1 that are issued behind the first wait for LDS (an empty list and at least six reads = one round trip)."""
    head = _head(w)
    reads = [i for i, s in enumerate(head) if s.startswith('ds_read')]
    wait = next((i for i, s in enumerate(head) if s.startswith('s_waitcnt') and 'lgkmcnt' in s), len(head))
    print(f'B5..B1: {len(head)} instructions, {len(reads)} ds_read at {reads}, first lgkmcnt wait at {wait}')
    if len(reads) < 6:
        return [f'only {len(reads)} ds_read between B5 and B1']
    return [head[i] for i in reads if i > wait]


def head_stores(w) -> list[str]:
    return [s for s in _head(w) if s.startswith('global_store')]


def slow_reads_in_front_of_x2(w) -> list[str]:
    win = w[1]
    first = next(i for i, s in enumerate(win) if s.startswith('ds_read_b128'))
    print(f'window B1..B2: first ds_read_b128 at {first}, in front of it: {[s for s in win[:first] if s.startswith("ds_")]}')
    return [s for s in win[:first] if s.startswith(('ds_read_b96', 'ds_read2'))]


CHECKS = {'T2_HEAD_ONE_TRIP': late_reads, 'T2_OUT_SHADOW': head_stores, 'T2_PREB1_OPERANDS': slow_reads_in_front_of_x2}


@pytest.fixture(scope='module')
def builds(tmp_path_factory):
    """{'shipped' | knob set to 0: (ISA, resource remarks)}; the four compiles run side by side."""
    td = tmp_path_factory.mktemp('isa')
    procs = {}
    for name, flags in [('shipped', [])] + [(k, [f'-D{k}=0']) for k in KNOBS]:
        asm = str(td / f'{name}.s')
        procs[name] = (asm, subprocess.Popen([HIPCC, '--offload-arch=gfx950', '-O3', '-std=c++17', '-Wno-pass-failed', '--cuda-device-only', '-S', 'loop_team2.hip',
                                              '-o', asm, '-Rpass-analysis=kernel-resource-usage'] + flags, cwd=CSRC, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True))
    out = {}
    for name, (asm, p) in procs.items():
        _, err = p.communicate()
        assert p.returncode == 0, err[-2000:]
        out[name] = (open(asm).read(), err)
    return out


def test_one_lds_round_trip_between_b5_and_phase_a(builds):
    late = late_reads(_windows(builds['shipped'][0]))
    assert not late, f'LDS reads between B5 and B1 behind the first wait for LDS: {late}'


def test_no_global_store_between_b5_and_b1(builds):
    st = head_stores(_windows(builds['shipped'][0]))
    assert not st, f'stores to global memory between B5 and B1: {st}'


def test_window_b1_opens_with_the_x2_reads(builds):
    slow = slow_reads_in_front_of_x2(_windows(builds['shipped'][0]))
    assert not slow, f'ds_read_b96 / ds_read2 between B1 and the first ds_read_b128: {slow}'


def test_scratch_within_the_bound(builds):
    blk = builds['shipped'][1].split('Function Name: ' + SHIPPED)[1].split('Function Name:')[0]
    scratch = int(re.search(r'ScratchSize \[bytes/lane\]: (\d+)', blk).group(1))
    print(f'loop_team2_kernel<RAW, false, false>: scratch {scratch} bytes per lane (bound {SCRATCH_BOUND})')
    assert scratch <= SCRATCH_BOUND


@pytest.mark.parametrize('knob', KNOBS)
def test_each_knob_at_zero_fails_its_assertion(builds, knob):
    found = CHECKS[knob](_windows(builds[knob][0]))
    print(f'-D{knob}=0: {found}')
    assert found, f'with -D{knob}=0 the generated code still passes the assertion the knob is there for'
