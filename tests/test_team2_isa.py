"""What the latency kernel's step loop looks like in the generated code (no GPU needed; skipped where hipcc is absent).

loop_team2_kernel<RAW, false, false> is one serial chain per step, so what sits on that chain is a property of the ISA, not of a
timing run.  This compiles csrc/loop_team2.hip for gfx950 and asserts of the shipped instantiation's step loop:

  * the per-step path holds exactly 5 workgroup barriers (B1..B5); the sixth `s_barrier` of the loop is the bounded-spin bail-out
    check that runs every 64th step;
  * behind the last per-step barrier (B5) there is no `v_div_*`: the sample value 2 k / (n_classes - 1) - 1 is looked up, not divided
    out, between the race result and phase A of the next step;
  * B5 is not fronted by `s_waitcnt vmcnt(0)`: it waits for the LDS hand-over only, never for vector memory.
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

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason='hipcc is not installed')


def _instructions(body: str) -> list[str]:
    out = []
    for line in body.split('\n'):
        s = line.split(';')[0].strip()
        if s and not s.startswith('.') or re.match(r'^\.LBB\d+_\d+:', s):
            out.append(s)
    return out


@pytest.fixture(scope='module')
def step_loop(tmp_path_factory) -> list[str]:
    asm = str(tmp_path_factory.mktemp('isa') / 'loop_team2.s')
    subprocess.run([HIPCC, '--offload-arch=gfx950', '-O3', '-std=c++17', '-Wno-pass-failed', '--cuda-device-only', '-S', 'loop_team2.hip', '-o', asm],
                   cwd=CSRC, check=True, capture_output=True)
    txt = open(asm).read()
    m = re.search(r'\n' + SHIPPED + r':[^\n]*\n(.*?)\n\s*s_endpgm', txt, re.S)
    assert m, 'the shipped instantiation is not in the ISA'
    ins = _instructions(m.group(1))
    label = {s[:-1]: i for i, s in enumerate(ins) if s.endswith(':') and s.startswith('.LBB')}
    loops = []
    for i, s in enumerate(ins):
        mm = re.match(r'(?:s_cbranch_\w+|s_branch)\s+(\.LBB\d+_\d+)', s)
        if mm and label.get(mm.group(1), i) < i:
            loops.append((label[mm.group(1)], i))
    # the step loop: the innermost loop with at least five workgroup barriers (the row loop around it holds more, the poll loops none)
    cand = [(b - a, a, b) for a, b in loops if sum(s == 's_barrier' for s in ins[a:b + 1]) >= 5]
    assert cand, 'no loop with five barriers'
    _, a, b = min(cand)
    return ins[a:b + 1]


def _barriers(loop):
    return [i for i, s in enumerate(loop) if s == 's_barrier']


def test_five_barriers_per_step(step_loop):
    bars = _barriers(step_loop)
    # the common back edge may leave the loop body in front of the bail-out block (5 barriers inside) or behind it (6)
    assert len(bars) in (5, 6), f'{len(bars)} s_barrier in the step loop, expected B1..B5 (+ the bail-out check)'
    if len(bars) == 6:
        # the sixth is reached on every 64th step only: (t & 63) == 63 is evaluated between B5 and it
        tail = step_loop[bars[4] + 1:bars[5]]
        assert any(re.match(r's_and_b32 s\d+, s\d+, 63$', s) for s in tail) and any(re.match(r's_cmp_\w+_u64 s\[\d+:\d+\], 63$', s) for s in tail), \
            'the last barrier of the loop is not behind the every-64-steps check'


def test_no_division_behind_b5(step_loop):
    bars = _barriers(step_loop)
    div = [s for s in step_loop[bars[4] + 1:] if s.startswith('v_div_')]
    assert not div, f'IEEE division behind B5, on the serial chain: {div}'


def test_b5_not_fronted_by_vmcnt0(step_loop):
    b5 = _barriers(step_loop)[4]
    i, waits = b5 - 1, []
    while i >= 0 and (step_loop[i].startswith('s_waitcnt') or step_loop[i].endswith(':')):   # the waits directly in front of the barrier
        waits.append(step_loop[i])
        i -= 1
    assert any('lgkmcnt(0)' in w for w in waits), 'B5 must order the shadow waves\' LDS writes'
    assert not any('vmcnt' in w for w in waits), f'B5 waits for vector memory: {waits}'
