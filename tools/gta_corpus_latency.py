"""Developer tool (GPU): the GTA corpus (``DeviceCorpus.gta`` -> ``wrnn_taco_gta_corpus``) against a loop of
``Tacotron.synthesize(gta_targets=...)`` over the utterances one at a time, which is what the library offered before.

Workload: the reference's hparams, seeded synthetic weights, ``--utts`` (256) synthetic utterances of ``--frames`` (200) mel frames and
``--tx`` (40) symbols; the corpus's mels are uniform noise in [0, 1] (teacher forcing runs frames / r steps whatever the mel holds).
``corpus.gta`` at ``batch_utts`` 1, 8, 64 and 256 and the loop alternate in one session; wall time from a device synchronisation to the
end of the call (``gta`` ends with its one wait, the loop waits once per utterance); median [min .. max] of ``--reps`` repetitions after
a warm-up of each.  Reported: total ms, utterances per second, us per decoder step of a group (total / groups / steps: what one
utterance of the group pays per step while its neighbours stream the same weights) and us per step and utterance (total / utterances /
steps).

``--parent-lib FILE``: also the no-regression check against another build of the library (the parent commit's): ``synthesize`` on the
seeded sentence of ``tools/tacotron_latency.py`` (Tx = 60, 400 steps) by both builds alternating, the mel's bytes compared, both medians
with their [min .. max].

    python tools/gta_corpus_latency.py [--reps 5] [--parent-lib build_variants/libparent.so] [--out FILE]
    python tools/gta_corpus_latency.py --calls 3 --batch 256        # under rocprofv3 --kernel-trace --stats: the kernels' own times
"""
from __future__ import annotations

import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def other_build(path):
    """Another build of the library with the argtypes of the entries ``NativeTacotron`` and ``synthesize`` use."""
    from tacotronv2_wavernn_chinese_amd import _cabi
    lib, vp = C.CDLL(path), C.c_void_p
    for name, args, res in (('wrnn_taco_create', [C.POINTER(_cabi.TacoDims), C.POINTER(vp)], C.c_int), ('wrnn_taco_tensor_count', [vp], C.c_int),
                            ('wrnn_taco_tensor_name', [vp, C.c_int], C.c_char_p), ('wrnn_taco_tensor_shape', [vp, C.c_int, C.POINTER(C.c_int64)], C.c_int),
                            ('wrnn_taco_load_tensor', [vp, C.c_char_p, vp, C.c_int, C.POINTER(C.c_int64)], C.c_int),
                            ('wrnn_taco_synthesize', [vp, C.POINTER(_cabi.TacoCall), vp], C.c_int), ('wrnn_taco_last_error', [vp], C.c_char_p),
                            ('wrnn_taco_destroy', [vp], None)):
        getattr(lib, name).argtypes, getattr(lib, name).restype = args, res
    return lib


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--utts', type=int, default=256)
    ap.add_argument('--frames', type=int, default=200)
    ap.add_argument('--tx', type=int, default=40)
    ap.add_argument('--parent-lib', dest='parent_lib', default=None, help='another build of the library for the no-regression check')
    ap.add_argument('--calls', type=int, default=0, help='only a warm-up and this many corpus.gta runs at --batch (for rocprofv3 --kernel-trace --stats)')
    ap.add_argument('--batch', type=int, default=256, help='batch_utts of the --calls runs')
    ap.add_argument('--skip-corpus', dest='skip_corpus', action='store_true', help='only the no-regression check of --parent-lib')
    ap.add_argument('--out', default=None, help='also write the report to this file')
    args = ap.parse_args()
    import torch
    from tacotronv2_wavernn_chinese_amd.dataset import DeviceCorpus
    from tacotronv2_wavernn_chinese_amd.synth import make_tacotron_state
    from tacotronv2_wavernn_chinese_amd.tacotron import DEFAULT_TACOTRON_DIMS, Tacotron
    dev = torch.device('cuda', 0)
    torch.cuda.set_device(dev)
    dims = dict(DEFAULT_TACOTRON_DIMS, n_symbols=64)
    state = dict(make_tacotron_state(0, **dims))
    model = Tacotron(**dims).load_state(state)
    N, F, TX, r, A = args.utts, args.frames, args.tx, dims['outputs_per_step'], np.float32(dims['max_abs_value'])
    rng = np.random.Generator(np.random.PCG64(2))
    seqs = [rng.integers(0, 64, size=TX).tolist() for _ in range(N)]
    mels = [rng.random((F, dims['num_mels']), dtype=np.float32) for _ in range(N)]
    corpus = DeviceCorpus.from_pairs([(m.T, np.zeros(F, np.int32)) for m in mels], dev, hop_length=1, features='tacotron')
    targets = [np.clip(np.float32(2) * A * m - A, -A, A).astype(np.float32) for m in mels]
    steps = -(-F // r)
    lines = []

    def say(s=''):
        print(s, flush=True)
        lines.append(s)

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, out

    def fmt(v):
        return f'{np.median(v):10.2f} [{min(v):10.2f} .. {max(v):10.2f}]'

    def loop():
        return [model.synthesize([seqs[u]], seeds=[u], gta_targets=[targets[u]], return_device=True)[0]['mel'] for u in range(N)]

    if args.calls:
        for _ in range(args.calls + 1):
            corpus.gta(model, seqs, batch_utts=args.batch)
        torch.cuda.synchronize()
        return
    if not args.skip_corpus:
        corpus_section(say, timed, fmt, loop, corpus, model, seqs, args, N, F, TX, steps, torch, dev)
        say()
        ragged_section(say, timed, fmt, state, dims, args, torch, dev)
    if args.parent_lib:
        parent_section(say, fmt, state, dims, args, torch)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as fh:
            fh.write('\n'.join(lines) + '\n')


def corpus_section(say, timed, fmt, loop, corpus, model, seqs, args, N, F, TX, steps, torch, dev):
    say(f'GTA corpus: {N} utterances of {F} frames, Tx {TX}, reference hparams, synthetic weights, {torch.cuda.get_device_name(dev)}')
    say(f'wall time around the whole corpus; median [min .. max] of {args.reps} alternating repetitions after a warm-up, ms')
    say()
    batches = [b for b in (1, 8, 64, 256) if b <= N] or [N]
    made, _ = corpus.gta(model, seqs, batch_utts=batches[-1])
    ref = loop()
    same = all(torch.equal(made.mels[int(mo):int(mo) + F * made.n_mels].view(F, -1), ref[u][:F]) for u, mo in enumerate(made.mel_off))
    say(f'corpus.gta mels equal the loop\'s bit for bit: {same}')
    for b in batches[:-1]:
        corpus.gta(model, seqs, batch_utts=b)
    t = {b: [] for b in batches}
    tl = []
    for _ in range(args.reps):
        for b in batches:
            t[b].append(timed(lambda: corpus.gta(model, seqs, batch_utts=b))[0])
        tl.append(timed(loop)[0])
    for b in batches:
        med, groups = float(np.median(t[b])), -(-N // b)
        say(f'corpus.gta batch_utts {b:4d} ({groups:4d} calls)   {fmt(t[b])}   {N / med * 1e3:9.1f} utt/s   {med / groups / steps * 1e3:8.1f} us per step of a group   '
            f'{med / N / steps * 1e3:8.2f} us per step and utterance')
    med = float(np.median(tl))
    say(f'synthesize one by one  ({N:4d} calls)   {fmt(tl)}   {N / med * 1e3:9.1f} utt/s   {med / N / steps * 1e3:8.1f} us per step of a call    '
        f'{med / N / steps * 1e3:8.2f} us per step and utterance')
    say(f'corpus.gta at {batches[-1]} / one by one = {np.median(t[batches[-1]]) / med:.4f}')


def ragged_section(say, timed, fmt, state, dims, args, torch, dev):
    """A corpus of mixed lengths: the groups are formed by frame count and queued shortest first, so every group needs more scratch than
    the last.  ``gta`` reserves the largest group's need before the first; the first run on a fresh handle (which pays that one
    allocation and the weights' upload) against the later runs shows what is left of it."""
    from tacotronv2_wavernn_chinese_amd.dataset import DeviceCorpus
    from tacotronv2_wavernn_chinese_amd.tacotron import Tacotron
    N, r = args.utts, dims['outputs_per_step']
    rng = np.random.Generator(np.random.PCG64(3))
    frames = rng.integers(50, 401, size=N)
    seqs = [rng.integers(0, 64, size=int(n)).tolist() for n in rng.integers(10, 81, size=N)]
    corpus = DeviceCorpus.from_pairs([(rng.random((dims['num_mels'], int(f)), dtype=np.float32), np.zeros(int(f), np.int32)) for f in frames], dev,
                                     hop_length=1, features='tacotron')
    total_steps = int(sum(-(-int(f) // r) for f in frames))
    say(f'ragged corpus: {N} utterances of 50 .. 400 frames ({int(frames.sum())} in all), Tx 10 .. 80; wall time around corpus.gta, ms')
    for b in (8, 64):
        fresh = Tacotron(**dims).load_state(state)
        fresh.synthesize([seqs[0]], seeds=[0], max_iters=1)                       # the weights' upload is not the corpus's cost
        first = timed(lambda: corpus.gta(fresh, seqs, batch_utts=b))[0]
        later = [timed(lambda: corpus.gta(fresh, seqs, batch_utts=b))[0] for _ in range(args.reps)]
        groups = -(-N // b)
        say(f'corpus.gta batch_utts {b:4d} ({groups:4d} calls)   first run on a fresh handle {first:10.2f}   later runs {fmt(later)}   '
            f'{N / np.median(later) * 1e3:9.1f} utt/s   scratch {fresh.native.gta_workspace_bytes() / 2 ** 20:.0f} MiB, reserved once')
    say(f'(one by one the same corpus is {total_steps} decoder steps in a row)')


def parent_section(say, fmt, state, dims, args, torch):
    """``synthesize`` on the seeded sentence of tools/tacotron_latency.py by this build and by ``--parent-lib``: HIP events around the
    call, the two builds alternating and swapping who goes first every repetition."""
    from tacotronv2_wavernn_chinese_amd import _cabi
    from tacotronv2_wavernn_chinese_amd.tacotron import Tacotron, make_dims
    sp = 'decoder/stop_token_projection/projection_stop_token_projection/bias'
    st = dict(state)
    st[sp] = st[sp] - np.float32(30.0)
    seq = np.random.Generator(np.random.PCG64(1)).integers(0, 64, size=60).tolist()
    here, parent = Tacotron(**dims).load_state(st), Tacotron(**dims)
    parent.native.close()
    parent.native = _cabi.NativeTacotron(make_dims(0, **dims), lib=other_build(args.parent_lib))
    parent.load_state(st)
    run = lambda m: m.synthesize([seq], seeds=[100], max_iters=400, return_device=True)[0]['mel']

    def timed(m):
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        run(m)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)
    a, b = run(here), run(parent)
    t = {id(here): [], id(parent): []}
    for i in range(max(args.reps, 8)):
        for m in ((here, parent) if i % 2 == 0 else (parent, here)):
            t[id(m)].append(timed(m))
    th, tp = t[id(here)], t[id(parent)]
    say(f'no regression: synthesize, Tx = 60, 400 steps, seed 100, this build against {os.path.basename(args.parent_lib)}, {len(th)} alternating repetitions (HIP events, ms)')
    say(f'the mel\'s bytes are equal: {a.shape == b.shape and torch.equal(a, b)} over {tuple(a.shape)}')
    say(f'this build {fmt(th)}   parent {fmt(tp)}   this median inside the parent\'s [min .. max]: {min(tp) <= np.median(th) <= max(tp)}')


if __name__ == '__main__':
    main()
