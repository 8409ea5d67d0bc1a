"""`wrnn_train_step` in fp32 against `train_precision = 'bf16'` in one session: two handles of one model, alternating call by call, each
call between HIP events (no torch op in the timed region).  B = 32 x 1 375 (the reference's batch) RAW and MOL, and B = 64 RAW;
`--warmup` untimed + `--reps` timed calls per handle; median and spread per mode, the ratio of the medians, the GEMM launches per
kernel (`train_last_gemms`), and how far the bf16 gradients are from the fp32 ones.

    python tools/train_precision_latency.py [--reps 5] [--warmup 2] [--out profiles/train_bf16.txt]
    python tools/train_precision_latency.py --only bf16 --shapes RAW:32    (one mode, one shape: the run to put under a kernel trace)
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--frames', type=int, default=5, help='mel frames per window (5 x 275 = 1 375 steps)')
    ap.add_argument('--shapes', default='RAW:32,MOL:32,RAW:64', help='MODE:B, comma separated')
    ap.add_argument('--only', choices=('f32', 'bf16'), help='run one precision only (for a kernel trace of its own)')
    ap.add_argument('--out', help='also append the report to this file')
    args = ap.parse_args()
    import numpy as np
    import torch
    from tacotronv2_wavernn_chinese_amd import _cabi
    from tacotronv2_wavernn_chinese_amd.synth import DEFAULT_DIMS
    from tacotronv2_wavernn_chinese_amd.vocoder import WaveRNN
    dev = torch.device('cuda:0')
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say(f'# tools/train_precision_latency.py --reps {args.reps} --warmup {args.warmup}: wrnn_train_step, fp32 and bf16 handles alternating, '
        f'ms between HIP events; {torch.cuda.get_device_name(0)}')
    precs = (args.only,) if args.only else ('f32', 'bf16')
    L = args.frames * DEFAULT_DIMS['hop_length']
    for shape in args.shapes.split(','):
        mode, B = shape.split(':')[0], int(shape.split(':')[1])
        torch.manual_seed(0)
        m = WaveRNN(**DEFAULT_DIMS, mode=mode)
        m.verbose = False
        m.to(dev).train()
        rng = np.random.Generator(np.random.PCG64(1))
        x = torch.from_numpy(rng.uniform(-1, 1, (B, L)).astype(np.float32)).to(dev)
        y = torch.from_numpy(rng.integers(0, 1024, (B, L)).astype(np.int32)).to(dev) if mode == 'RAW' else \
            torch.from_numpy(rng.uniform(-1, 1, (B, L)).astype(np.float32)).to(dev)
        mu = torch.from_numpy(rng.random((B, L, DEFAULT_DIMS['feat_dims']), dtype=np.float32)).to(dev)
        au = torch.from_numpy(rng.standard_normal((B, L, DEFAULT_DIMS['res_out_dims'])).astype(np.float32)).to(dev)
        ps = [p.detach().contiguous() for p in m._loop_params()]
        st = torch.cuda.current_stream(dev).cuda_stream
        run = {}
        for prec in precs:
            nat = _cabi.NativeVocoder(device=0, mode=mode, **DEFAULT_DIMS)
            nat.set_train_precision(prec)
            run[prec] = dict(nat=nat, gs=[torch.zeros_like(p) for p in ps], dm=torch.zeros_like(mu), da=torch.zeros_like(au),
                             loss=torch.zeros((), device=dev), ms=[])

        def call(r):
            r['nat'].train_step([p.data_ptr() for p in ps], [g.data_ptr() for g in r['gs']], x.data_ptr(), mu.data_ptr(), au.data_ptr(), y.data_ptr(),
                                B, L, r['loss'].data_ptr(), 0, r['dm'].data_ptr(), r['da'].data_ptr(), st)

        for it in range(args.warmup + args.reps):
            for prec in precs:
                r = run[prec]
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                call(r)
                e1.record()
                r['nat'].sync_status(st)
                if it >= args.warmup:
                    r['ms'].append(e0.elapsed_time(e1))
        say(f'{mode} B={B} L={L} ({B * L} rows), recurrences: {run[precs[0]]["nat"].train_last_recurrence()[0]}')
        for prec in precs:
            r = run[prec]
            med = statistics.median(r['ms'])
            n32, n16 = r['nat'].train_last_gemms()
            say(f'  {prec:5s} median {med:7.3f} ms  (min {min(r["ms"]):.3f}, max {max(r["ms"]):.3f}; calls ' + ' '.join(f'{v:.3f}' for v in r['ms']) +
                f')  {B * L / med:.0f} ksamples/s  GEMMs fp32 {n32} / bf16 {n16}  loss {float(r["loss"]):.6f}')
        if len(precs) == 2:
            a, b = statistics.median(run['f32']['ms']), statistics.median(run['bf16']['ms'])
            worst = max(float((g16.double() - g32.double()).abs().max() / g32.double().abs().max().clamp_min(1e-300))
                        for g32, g16 in zip(run['f32']['gs'] + [run['f32']['dm'], run['f32']['da']], run['bf16']['gs'] + [run['bf16']['dm'], run['bf16']['da']]))
            say(f'  bf16 / f32 = {b / a:.3f}  ({a - b:+.3f} ms saved per step); largest |grad bf16 - grad f32| / max|grad f32| over the tensors {worst:.2e}')
        for r in run.values():
            r['nat'].close()
    if args.out:
        with open(args.out, 'a') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
