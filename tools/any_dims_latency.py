#!/usr/bin/env python
"""Time the generate loop of models whose dims are not the reference hparams: WRNN_KERNEL_SIMPLE against WRNN_KERNEL_TEAMG, one session.

    python tools/any_dims_latency.py [--reps 5] [--warmup 2] [--out profiles/any_dims.txt]

Dim sets A (256 / 384), C (1024 / 1024) and D (the reference hparams, TEAMG forced) of tests/teamg_cases.py at B = 1 and B = 8 rows, the
same mels and the same Philox seed for both kernels, about 250 steps per row.  Timed: `wrnn_timing.loop_ms`, the HIP events around the
loop kernel of one call; warm-up calls first, then `--reps` timed calls per kernel, the two kernels alternating; every call is listed, the
median is what the ratio is made of.  Next to it the bytes TEAMG streams per step (`wrnn_teamg_plan`) and what that is per second and XCD."""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FRAMES = {'A': 2, 'C': 42, 'D': 1}      # 256, 252 and 275 steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise RuntimeError('any_dims_latency.py measures on an MI355X: no GPU, no figures')
    if args.reps < 5:
        raise ValueError('at least 5 timed calls per kernel')
    from tacotronv2_wavernn_chinese_amd import _cabi
    from tacotronv2_wavernn_chinese_amd.synth import make_mels, make_state_dict
    from tacotronv2_wavernn_chinese_amd.vocoder import WaveRNN
    from tests.teamg_cases import DIM_SETS
    lines = [f'generate loop on other dims, {torch.cuda.get_device_name(0)}, torch {torch.__version__}', '',
             f'loop_ms of one call (HIP events around the loop kernel), {args.warmup} warm-up + {args.reps} timed calls per kernel, alternating; RAW, Philox noise',
             'us/step = median loop time / steps per row; GB/s per XCD = the bytes TEAMG streams per step (wrnn_teamg_plan) / its us per step', '']
    worst = 0.0
    for name in ('A', 'C', 'D'):
        dims = DIM_SETS[name]
        sd = make_state_dict(7, 'RAW', 'peaky', **dims)
        m = WaveRNN(**dims, mode='RAW')
        m.verbose = False
        m.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in sd.items()})
        m.to('cuda:0')
        plan = m.native().teamg_plan()
        streamed = plan['streamed_bytes_step']
        total = sum(L['weight_bytes'] for L in plan['layers'].values())
        lines.append(f'set {name}: rnn {dims["rnn_dims"]}, fc {dims["fc_dims"]}, feat {dims["feat_dims"]}, res_out {dims["res_out_dims"]}, bits {dims["bits"]}, hop '
                     f'{dims["hop_length"]}; loop weights {total / 1e6:.2f} MB, TEAMG streams {streamed / 1e6:.2f} MB per step and team, LDS {plan["lds_bytes"]} bytes per workgroup')
        for B in (1, 8):
            T = FRAMES[name]
            steps = T * dims['hop_length']
            mels = torch.from_numpy(make_mels(5, B, T, feat_dims=dims['feat_dims'])).cuda()
            ms = {'simple': [], 'teamg': []}
            for rep in range(args.warmup + args.reps):
                for k in ('simple', 'teamg'):
                    m.generate_raw(mels, False, 11000, 550, noise_mode='philox', seed=99, kernel=k)
                    assert m.last_timing['kernel'] == _cabi.KERNEL_IDS[k] and m.last_timing['steps'] == steps
                    if rep >= args.warmup:
                        ms[k].append(float(m.last_timing['loop_ms']))
            us = {k: float(np.median(v)) * 1e3 / steps for k, v in ms.items()}
            ratio = us['teamg'] / us['simple']
            worst = max(worst, ratio)
            for k in ('simple', 'teamg'):
                lines.append(f'  B={B} {steps} steps  {k:6s} {us[k]:9.2f} us/step  {1e3 / us[k]:8.2f} ksamples/s per row  ({B * 1e3 / us[k]:8.2f} in all)   calls (ms): '
                             + ' '.join(f'{v:.3f}' for v in ms[k]))
            lines.append(f'  B={B}: TEAMG / SIMPLE time per step = {ratio:.4f} (required <= 0.25)   TEAMG streams {streamed / us["teamg"] / 1e3:.1f} GB/s per XCD')
        lines.append('')
        del m
        torch.cuda.empty_cache()
    lines.append(f'worst TEAMG / SIMPLE ratio over the six shapes: {worst:.4f} -> {"meets" if worst <= 0.25 else "MISSES"} the 4x requirement')
    text = '\n'.join(lines) + '\n'
    print(text)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(text)


if __name__ == '__main__':
    main()
