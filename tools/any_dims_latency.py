#!/usr/bin/env python
"""Time the generate loop of models whose dims are not the reference hparams: WRNN_KERNEL_SIMPLE against WRNN_KERNEL_TEAMG, one session.

    python tools/any_dims_latency.py [--reps 5] [--warmup 2] [--out profiles/any_dims.txt]

Dim sets A (256 / 384), C (1024 / 1024) and D (the reference hparams, TEAMG forced) of tests/teamg_cases.py at B = 1 and B = 8 rows, the
same mels and the same Philox seed for both kernels, about 250 steps per row.  Timed: `wrnn_timing.loop_ms`, the HIP events around the
loop kernel of one call; warm-up calls first, then `--reps` timed calls per kernel, the two kernels alternating; every call is listed, the
median is what the ratio is made of.  Next to it the bytes TEAMG streams per step (`wrnn_teamg_plan`) and what that is per second and XCD.

    python tools/any_dims_latency.py --weights f16 [--out profiles/any_dims_f16.txt]

times WRNN_KERNEL_TEAMG with the fp32 weight image against the same kernel with the fp16 image (`teamg_weights='f16'`) instead: two
handles of one model, the two formats alternating call by call, the same shapes, mels and seed; per shape the median, the min-to-max
spread of either, the bytes streamed per step in either format (`wrnn_teamg_plan_fmt`) and whether f16 is slower than f32 by more than the
larger spread.

    python tools/any_dims_latency.py --weights e4m3 [--out FILE]

adds a third handle with the e4m3 image (`teamg_weights='e4m3'`): fp32, fp16 and e4m3 alternate call by call in one session, same
protocol; the verdict of a shape is e4m3 against fp16 in that session (faster by more than the spread, equal, or slower), with the time
ratio next to the ratio of the streamed bytes.

    python tools/any_dims_latency.py --sparse 0.5,0.25,0.125,0.0625 [--sets CDA] [--lib build_variants/libX.so] [--out FILE]

times the block-sparse image (`teamg_sparse = True`): per density a copy of the synthetic model pruned with
`sparsity.block_masks` on rnn1, rnn2, fc1 and fc2, next to the dense model with the fp32, fp16 and e4m3 images -- all configurations
alternate call by call in one session, one row per team; kept / total blocks and the bytes streamed per step come from
`teamg_sparse_info`.  The verdict of a set is each sparse configuration against dense fp32.  `--lib` times another build of the library."""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FRAMES = {'A': 2, 'C': 42, 'D': 1}      # 256, 252 and 275 steps


def weights_session(args):
    """fp32 image against fp16 image (and, with --weights e4m3, the e4m3 image), WRNN_KERNEL_TEAMG, B = 1 and B = 8 rows."""
    fmts = ('f32', 'f16') if args.weights == 'f16' else ('f32', 'f16', 'e4m3')
    from tacotronv2_wavernn_chinese_amd import _cabi
    from tacotronv2_wavernn_chinese_amd.synth import make_mels, make_state_dict
    from tacotronv2_wavernn_chinese_amd.vocoder import WaveRNN
    from tests.teamg_cases import DIM_SETS
    lines = [f'{"fp16" if args.weights == "f16" else "fp16 and e4m3"} weight image of the any-dims team kernel, {torch.cuda.get_device_name(0)}, torch {torch.__version__}', '',
             f'loop_ms of one call (HIP events around the loop kernel), {args.warmup} warm-up + {args.reps} timed calls per format, alternating; RAW, Philox noise',
             'us/step = median loop time / steps per row; spread = (max - min) of the timed calls per step; GB/s per XCD = bytes streamed per step / us per step', '']
    verdicts = []
    for name in ('A', 'C', 'D'):
        dims = DIM_SETS[name]
        sd = make_state_dict(7, 'RAW', 'peaky', **dims)
        models, plans = {}, {}
        for w in fmts:
            m = WaveRNN(**dims, mode='RAW')
            m.verbose = False
            m.teamg_weights = w
            m.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in sd.items()})
            m.to('cuda:0')
            models[w] = m
            plans[w] = _cabi.teamg_plan_fmt(1, w, -1, mode='RAW', **dims)
        lines.append(f'set {name}: rnn {dims["rnn_dims"]}, fc {dims["fc_dims"]}, feat {dims["feat_dims"]}, res_out {dims["res_out_dims"]}, bits {dims["bits"]}, hop {dims["hop_length"]}; '
                     + '; '.join(f'{w}: weights {sum(L["weight_bytes"] for L in plans[w]["layers"].values()) / 1e6:.2f} MB, streamed {plans[w]["streamed_bytes_step"] / 1e6:.2f} MB '
                                 f'per step and team, LDS {plans[w]["lds_bytes"]}' for w in fmts))
        for B in (1, 8):
            T = FRAMES[name]
            steps = T * dims['hop_length']
            mels = torch.from_numpy(make_mels(5, B, T, feat_dims=dims['feat_dims'])).cuda()
            ms = {w: [] for w in fmts}
            for rep in range(args.warmup + args.reps):
                for w in fmts:
                    m = models[w]
                    m.generate_raw(mels, False, 11000, 550, noise_mode='philox', seed=99, kernel='teamg')
                    lt = m.last_timing
                    assert lt['kernel'] == _cabi.KERNEL_TEAMG and lt['steps'] == steps and lt['teamg_weights'] == w
                    if rep >= args.warmup:
                        ms[w].append(float(lt['loop_ms']))
            us = {w: float(np.median(v)) * 1e3 / steps for w, v in ms.items()}
            spread = {w: (max(v) - min(v)) * 1e3 / steps for w, v in ms.items()}
            for w in fmts:
                lines.append(f'  B={B} {steps} steps  {w}  {us[w]:8.2f} us/step  spread {spread[w]:.2f}  {1e3 / us[w]:7.2f} ksamples/s per row  '
                             f'{plans[w]["streamed_bytes_step"] / us[w] / 1e3:7.1f} GB/s per XCD   calls (ms): ' + ' '.join(f'{v:.3f}' for v in ms[w]))
            if args.weights == 'e4m3':
                margin = max(spread['f16'], spread['e4m3'])
                ratio_b = plans['e4m3']['streamed_bytes_step'] / max(plans['f16']['streamed_bytes_step'], 1)
                d = us['e4m3'] - us['f16']
                verdicts.append(f'set {name} B={B}: e4m3 / f16 time per step {us["e4m3"] / us["f16"]:.3f} (streamed bytes e4m3 / f16 {ratio_b:.3f}; e4m3 / f32 time '
                                f'{us["e4m3"] / us["f32"]:.3f}), margin {margin:.2f} us -> '
                                f'{"e4m3 FASTER than f16 beyond the spread" if -d > margin else "e4m3 SLOWER than f16 beyond the spread" if d > margin else "e4m3 equal to f16 within the spread"}; '
                                f'e4m3 {1e3 / us["e4m3"]:.2f} ksamples/s per row')
                continue
            margin = max(spread.values())
            ratio_b = plans['f16']['streamed_bytes_step'] / max(plans['f32']['streamed_bytes_step'], 1)
            verdicts.append(f'set {name} B={B}: f16 / f32 time per step {us["f16"] / us["f32"]:.3f} (streamed bytes f16 / f32 {ratio_b:.3f}), margin {margin:.2f} us -> '
                            f'{"f16 SLOWER than f32 beyond the spread" if us["f16"] - us["f32"] > margin else "f16 not slower than f32"}; '
                            f'f16 {1e3 / us["f16"]:.2f} ksamples/s per row ({"above" if 1e3 / us["f16"] > 22.05 else "below"} 22.05)')
        lines.append('')
        del models
        torch.cuda.empty_cache()
    lines += verdicts
    text = '\n'.join(lines) + '\n'
    print(text)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(text)


def sparse_session(args, kernel='teamg', rows=1, batch_rows=0):
    """Dense fp32 / fp16 / e4m3 and the sparse image at every density of --sparse, alternating call by call; `rows` rows on `kernel`."""
    from tacotronv2_wavernn_chinese_amd import _cabi
    from tacotronv2_wavernn_chinese_amd.sparsity import apply_masks_, block_masks
    from tacotronv2_wavernn_chinese_amd.synth import make_mels, make_state_dict
    from tacotronv2_wavernn_chinese_amd.vocoder import WaveRNN
    from tests.teamg_cases import DIM_SETS
    densities = [float(v) for v in args.sparse.split(',')]
    lines = [f'block-sparse weight image of the any-dims team kernels ({kernel}), {torch.cuda.get_device_name(0)}, torch {torch.__version__}', '',
             f'loop_ms of one call (HIP events around the loop kernel), {args.warmup} warm-up + {args.reps} timed calls per configuration, alternating; RAW, Philox noise',
             'us/step = median loop time / steps per row; spread = (max - min) of the timed calls per step; streamed = weight bytes a team reads per step;',
             'sparse D = rnn1, rnn2, fc1, fc2 pruned to the share D of blocks per row (sparsity.block_masks), fp32 values, teamg_sparse on', '']
    verdicts = []
    for name in args.sets:
        dims = DIM_SETS[name]
        sd = make_state_dict(7, 'RAW', 'peaky', **dims)
        configs = [('f32', 'f32', None), ('f16', 'f16', None), ('e4m3', 'e4m3', None)] + [(f'sparse {d:g}', 'f32', d) for d in densities]
        models = {}
        for tag, w, density in configs:
            m = WaveRNN(**dims, mode='RAW')
            m.verbose = False
            m.teamg_weights = w
            m.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in sd.items()})
            if density is not None:
                apply_masks_(m, block_masks(m, density))
                m.teamg_sparse = True
            m.to('cuda:0')
            models[tag] = m
        teams = models['f32'].native().team_info()[1]
        B = rows if rows > 0 else 8 * teams
        R = batch_rows   # the most rows per team the plan admits for these dims, up to batch_rows
        while R > 1:
            try:
                _cabi.teamg_batch_plan(R, -1, mode='RAW', **dims)
                break
            except _cabi.WrnnError:
                R //= 2
        T = FRAMES[name]
        steps = T * dims['hop_length']
        lines.append(f'set {name}: rnn {dims["rnn_dims"]}, fc {dims["fc_dims"]}, hop {dims["hop_length"]}; {B} rows x {steps} steps on {teams} teams'
                     + (f', {R} rows per team' if batch_rows else ''))
        mels = torch.from_numpy(make_mels(5, B, T, feat_dims=dims['feat_dims'])).cuda()
        kw = dict(batch_rows=R) if batch_rows else {}
        ms = {tag: [] for tag, _, _ in configs}
        for rep in range(args.warmup + args.reps):
            for tag, w, density in configs:
                m = models[tag]
                m.generate_raw(mels, False, 11000, 550, noise_mode='philox', seed=99, kernel=kernel, **kw)
                lt = m.last_timing
                assert lt['kernel'] == _cabi.KERNEL_IDS[kernel] and lt['steps'] == steps and lt['teamg_weights'] == w and lt['teamg_sparse'] is (density is not None)
                assert not batch_rows or lt['batch_rows'] == R
                if rep >= args.warmup:
                    ms[tag].append(float(lt['loop_ms']))
        us = {k: float(np.median(v)) * 1e3 / steps for k, v in ms.items()}
        spread = {k: (max(v) - min(v)) * 1e3 / steps for k, v in ms.items()}
        for tag, w, density in configs:
            if density is None:
                p = _cabi.teamg_plan_fmt(max(R, 1), w, -1, mode='RAW', **dims)
                what = f'streamed {p["streamed_bytes_step"] / 1e6:6.2f} MB per step, LDS {p["lds_bytes"]}'
            else:
                info = models[tag].native().teamg_sparse_info()
                p = info['plan']
                what = (f'streamed {p["streamed_bytes_step"] / 1e6:6.2f} MB per step, LDS {p["lds_bytes"]}, kept {info["kept"]} of {info["dense"]} blocks, image '
                        f'{sum(L["weight_bytes"] for L in p["layers"].values()) / 1e6:.2f} MB')
            lines.append(f'  {tag:14s} {us[tag]:8.2f} us/step  spread {spread[tag]:.2f}  {what}   calls (ms): ' + ' '.join(f'{v:.3f}' for v in ms[tag]))
        for tag, w, density in configs:
            if density is None:
                continue
            margin = max(spread[tag], spread['f32'])
            d = us[tag] - us['f32']
            verdicts.append(f'set {name} {tag}: time / dense fp32 {us[tag] / us["f32"]:.3f}, margin {margin:.2f} us -> '
                            f'{"sparse FASTER than dense fp32 beyond the spread" if -d > margin else "sparse SLOWER than dense fp32 beyond the spread" if d > margin else "equal within the spread"}'
                            f' (fp16 {us["f16"]:.2f}, e4m3 {us["e4m3"]:.2f} us/step)')
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
    ap.add_argument('--out', default=None)
    ap.add_argument('--weights', choices=('f32', 'f16', 'e4m3'), default='f32',
                    help="f16: time the fp32 image against the fp16 image of TEAMG instead; e4m3: fp32, fp16 and e4m3 alternating")
    ap.add_argument('--sparse', metavar='DENSITY[,DENSITY..]', default=None,
                    help='time the block-sparse image at these densities next to the dense fp32, fp16 and e4m3 images (sparse_session)')
    ap.add_argument('--sets', default='CDA', help='with --sparse: the dim sets of tests/teamg_cases.py to time')
    ap.add_argument('--lib', default=None, help='another build of libwavernn_amd.so to time')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise RuntimeError('any_dims_latency.py measures on an MI355X: no GPU, no figures')
    if args.reps < 5:
        raise ValueError('at least 5 timed calls per kernel')
    from tacotronv2_wavernn_chinese_amd import _cabi
    if args.lib:
        _cabi.LIB_PATH = os.path.abspath(args.lib)
    if args.sparse is not None:
        return sparse_session(args)
    from tacotronv2_wavernn_chinese_amd.synth import make_mels, make_state_dict
    from tacotronv2_wavernn_chinese_amd.vocoder import WaveRNN
    from tests.teamg_cases import DIM_SETS
    if args.weights != 'f32':
        return weights_session(args)
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
