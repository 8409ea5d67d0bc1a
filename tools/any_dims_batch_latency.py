#!/usr/bin/env python
"""Time many-row calls of models whose dims are not 512 / 512: WRNN_KERNEL_TEAMG (one row per XCD team, rows beyond the team count one
after the other) against WRNN_KERNEL_TEAMG_BATCH at every rows-per-team count its plan admits, one session.

    python tools/any_dims_batch_latency.py [--reps 5] [--warmup 2] [--out profiles/any_dims_batch.txt]

Dim sets A (256 / 384), C (1024 / 1024) and D (the reference hparams on the generic kernels) of tests/teamg_cases.py, one call of
8 x n_teams rows of about 250 steps, the same mels and the same Philox seed for every kernel.  Timed: `wrnn_timing.loop_ms`, the HIP events
around the loop kernel of one call; warm-up calls first, then `--reps` timed calls per kernel, the kernels alternating; every call is
listed.  us/step/row = median loop time / (steps x rows): the time the call spends per row and step, all teams busy.  Next to each the bytes
a team streams per step and row (`wrnn_teamg_batch_plan`).  The last lines state, per dim set, whether the default rows per team
(batch_rows 0) beats TEAMG per row by more than the larger min-to-max spread of the two, and whether a smaller admitted count beats the
default by more than that.

    python tools/any_dims_batch_latency.py --weights f16 [--out FILE]

times WRNN_KERNEL_TEAMG_BATCH with the fp32 weight image against the fp16 image (`teamg_weights='f16'`) at every rows-per-team count both
plans admit: two handles of one model, the formats alternating call by call.

    python tools/any_dims_batch_latency.py --weights e4m3 [--out FILE]

adds a third handle with the e4m3 image: fp32, fp16 and e4m3 alternate call by call in one session; the verdict of a shape is e4m3
against fp16 in that session, the time ratio next to the ratio of the streamed bytes.

    python tools/any_dims_batch_latency.py --sparse 0.5,0.25,0.125,0.0625 [--sets CDA] [--out FILE]

times the block-sparse image (`teamg_sparse = True`) on WRNN_KERNEL_TEAMG_BATCH, 8 x n_teams rows at the most rows per team the plan admits (up to 8):
tools/any_dims_latency.py's `sparse_session` (dense fp32, fp16, e4m3 and the pruned copies alternating call by call, kept / total blocks
and streamed bytes from `teamg_sparse_info`)."""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FRAMES = {'A': 2, 'C': 42, 'D': 1}      # 256, 252 and 275 steps


def weights_session(args):
    """fp32 image against fp16 image (and, with --weights e4m3, the e4m3 image), WRNN_KERNEL_TEAMG_BATCH at every admitted rows-per-team
    count, 8 x n_teams rows."""
    fmts = ('f32', 'f16') if args.weights == 'f16' else ('f32', 'f16', 'e4m3')
    from tacotronv2_wavernn_chinese_amd import _cabi
    from tacotronv2_wavernn_chinese_amd.synth import make_mels, make_state_dict
    from tacotronv2_wavernn_chinese_amd.vocoder import WaveRNN
    from tests.teamg_cases import DIM_SETS
    lines = [f'{"fp16" if args.weights == "f16" else "fp16 and e4m3"} weight image, many rows on other dims, {torch.cuda.get_device_name(0)}, torch {torch.__version__}', '',
             f'loop_ms of one call (HIP events around the loop kernel), {args.warmup} warm-up + {args.reps} timed calls per format, alternating; RAW, Philox noise',
             'us/step/row = median loop time / (steps x rows); spread = (max - min) of the timed calls in the same unit; streamed = weight bytes a team reads per step', '']
    verdicts = []
    for name in args.sets:
        dims = DIM_SETS[name]
        sd = make_state_dict(7, 'RAW', 'peaky', **dims)
        models = {}
        for w in fmts:
            m = WaveRNN(**dims, mode='RAW')
            m.verbose = False
            m.teamg_weights = w
            m.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in sd.items()})
            m.to('cuda:0')
            models[w] = m
        teams = models['f32'].native().team_info()[1]
        B, T = 8 * teams, FRAMES[name]
        steps = T * dims['hop_length']
        plans = {}
        for R in (2, 4, 8):
            try:
                plans[R] = {w: _cabi.teamg_plan_fmt(R, w, -1, mode='RAW', **dims) for w in fmts}
            except _cabi.WrnnError:
                pass
        lines.append(f'set {name}: rnn {dims["rnn_dims"]}, fc {dims["fc_dims"]}, hop {dims["hop_length"]}; {B} rows x {steps} steps on {teams} teams; rows per team admitted: {sorted(plans)}')
        mels = torch.from_numpy(make_mels(5, B, T, feat_dims=dims['feat_dims'])).cuda()
        ms = {(R, w): [] for R in plans for w in fmts}
        for rep in range(args.warmup + args.reps):
            for R, w in ms:
                m = models[w]
                m.generate_raw(mels, False, 11000, 550, noise_mode='philox', seed=99, kernel='teamg_batch', batch_rows=R)
                lt = m.last_timing
                assert lt['kernel'] == _cabi.KERNEL_TEAMG_BATCH and lt['steps'] == steps and lt['rows'] == B and lt['batch_rows'] == R and lt['teamg_weights'] == w
                if rep >= args.warmup:
                    ms[(R, w)].append(float(lt['loop_ms']))
        us = {k: float(np.median(v)) * 1e3 / (steps * B) for k, v in ms.items()}
        spread = {k: (max(v) - min(v)) * 1e3 / (steps * B) for k, v in ms.items()}
        for R in sorted(plans):
            for w in fmts:
                p = plans[R][w]
                lines.append(f'  R={R} {w}  {us[(R, w)]:8.3f} us/step/row  {1e3 / us[(R, w)]:9.2f} ksamples/s in all  spread {spread[(R, w)]:.3f}   streamed {p["streamed_bytes_step"] / 1e6:6.2f} MB '
                             f'per step, LDS {p["lds_bytes"]}   calls (ms): ' + ' '.join(f'{v:.3f}' for v in ms[(R, w)]))
            if args.weights == 'e4m3':
                margin = max(spread[(R, 'f16')], spread[(R, 'e4m3')])
                d = us[(R, 'e4m3')] - us[(R, 'f16')]
                verdicts.append(f'set {name} R={R}: e4m3 / f16 time {us[(R, "e4m3")] / us[(R, "f16")]:.3f} (streamed bytes e4m3 / f16 '
                                f'{plans[R]["e4m3"]["streamed_bytes_step"] / max(plans[R]["f16"]["streamed_bytes_step"], 1):.3f}; e4m3 / f32 time '
                                f'{us[(R, "e4m3")] / us[(R, "f32")]:.3f}), margin {margin:.3f} -> '
                                f'{"e4m3 FASTER than f16 beyond the spread" if -d > margin else "e4m3 SLOWER than f16 beyond the spread" if d > margin else "e4m3 equal to f16 within the spread"}')
                continue
            margin = max(spread[(R, 'f32')], spread[(R, 'f16')])
            verdicts.append(f'set {name} R={R}: f16 / f32 time {us[(R, "f16")] / us[(R, "f32")]:.3f} (streamed bytes f16 / f32 '
                            f'{plans[R]["f16"]["streamed_bytes_step"] / max(plans[R]["f32"]["streamed_bytes_step"], 1):.3f}), margin {margin:.3f} -> '
                            f'{"f16 SLOWER than f32 beyond the spread" if us[(R, "f16")] - us[(R, "f32")] > margin else "f16 not slower than f32"}')
        lines.append('')
        del models
        torch.cuda.empty_cache()
    lines += verdicts
    text = '\n'.join(lines) + '\n'
    print(text)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(text)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--sets', default='ACD')
    ap.add_argument('--out', default=None)
    ap.add_argument('--weights', choices=('f32', 'f16', 'e4m3'), default='f32',
                    help="f16: time the fp32 image against the fp16 image of TEAMG_BATCH instead; e4m3: fp32, fp16 and e4m3 alternating")
    ap.add_argument('--sparse', metavar='DENSITY[,DENSITY..]', default=None,
                    help='time the block-sparse image at these densities next to the dense fp32, fp16 and e4m3 images, 8 rows per team')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise RuntimeError('any_dims_batch_latency.py measures on an MI355X: no GPU, no figures')
    if args.reps < 5:
        raise ValueError('at least 5 timed calls per kernel')
    if args.sparse is not None:
        sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
        from any_dims_latency import sparse_session
        return sparse_session(args, kernel='teamg_batch', rows=0, batch_rows=8)
    from tacotronv2_wavernn_chinese_amd import _cabi
    from tacotronv2_wavernn_chinese_amd.synth import make_mels, make_state_dict
    from tacotronv2_wavernn_chinese_amd.vocoder import WaveRNN
    from tests.teamg_cases import DIM_SETS
    if args.weights != 'f32':
        return weights_session(args)
    lines = [f'many rows on other dims, {torch.cuda.get_device_name(0)}, torch {torch.__version__}', '',
             f'loop_ms of one call (HIP events around the loop kernel), {args.warmup} warm-up + {args.reps} timed calls per kernel, alternating; RAW, Philox noise',
             'us/step/row = median loop time / (steps x rows); streamed = weight bytes a team reads per step, per row of its batch (wrnn_teamg_batch_plan)', '']
    verdicts = []
    for name in args.sets:
        dims = DIM_SETS[name]
        sd = make_state_dict(7, 'RAW', 'peaky', **dims)
        m = WaveRNN(**dims, mode='RAW')
        m.verbose = False
        m.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in sd.items()})
        m.to('cuda:0')
        nat = m.native()
        teams = nat.team_info()[1]
        B, T = 8 * teams, FRAMES[name]
        steps = T * dims['hop_length']
        plans = {1: nat.teamg_plan()}
        for R in (2, 4, 8):
            try:
                plans[R] = nat.teamg_batch_plan(R)
            except _cabi.WrnnError:
                pass
        lines.append(f'set {name}: rnn {dims["rnn_dims"]}, fc {dims["fc_dims"]}, feat {dims["feat_dims"]}, res_out {dims["res_out_dims"]}, bits {dims["bits"]}, hop '
                     f'{dims["hop_length"]}; {B} rows x {steps} steps on {teams} teams; rows per team admitted: {sorted(plans)}')
        mels = torch.from_numpy(make_mels(5, B, T, feat_dims=dims['feat_dims'])).cuda()
        kinds = [('teamg', 1, 0)] + [('teamg_batch', R, R) for R in sorted(plans) if R > 1]
        ms = {R: [] for _, R, _ in kinds}
        default_rows = None
        for rep in range(args.warmup + args.reps):
            for k, R, br in kinds:
                m.generate_raw(mels, False, 11000, 550, noise_mode='philox', seed=99, kernel=k, batch_rows=br)
                lt = m.last_timing
                assert lt['kernel'] == _cabi.KERNEL_IDS[k] and lt['steps'] == steps and lt['rows'] == B and lt['batch_rows'] == R
                if rep >= args.warmup:
                    ms[R].append(float(lt['loop_ms']))
        m.generate_raw(mels, False, 11000, 550, noise_mode='philox', seed=99, kernel='teamg_batch')
        default_rows = m.last_timing['batch_rows']
        us = {R: float(np.median(v)) * 1e3 / (steps * B) for R, v in ms.items()}
        spread = {R: (max(v) - min(v)) * 1e3 / (steps * B) for R, v in ms.items()}
        for k, R, _ in kinds:
            p = plans[R]
            lines.append(f'  {k:11s} R={R}  {us[R]:8.3f} us/step/row  {1e3 / us[R]:9.2f} ksamples/s in all  spread {spread[R]:.3f}   streamed {p["streamed_bytes_step"] / 1e6:6.2f} MB '
                         f'per step = {p["streamed_bytes_step"] / R / 1e6:6.2f} MB per row, LDS {p["lds_bytes"]} ({p["activation_bytes"]} vectors)   calls (ms): '
                         + ' '.join(f'{v:.3f}' for v in ms[R]))
        d = default_rows
        margin = max(spread[1], spread[d])
        ok = us[1] - us[d] > margin
        better = [R for R in ms if 1 < R < d and us[d] - us[R] > max(spread[R], spread[d])]
        verdicts.append(f'set {name}: default rows per team {d}: {us[d]:.3f} against TEAMG {us[1]:.3f} us/step/row (x{us[1] / us[d]:.2f}), margin needed {margin:.3f} -> '
                        f'{"faster" if ok else "NOT faster"} per row' + (f'; a smaller count beats the default by more than the spread: {better}' if better else
                                                                        '; no smaller admitted count beats the default by more than the spread'))
        lines.append('')
        del m
        torch.cuda.empty_cache()
    lines += verdicts
    text = '\n'.join(lines) + '\n'
    print(text)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(text)


if __name__ == '__main__':
    main()
