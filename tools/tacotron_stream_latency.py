"""Developer tool (GPU): what streaming Tacotron costs and what it buys -- writes profiles/tacotron_stream.txt.

Workload: the sentence and the synthetic weights of tools/tacotron_latency.py (reference hparams, Tx = 60, 400 frames, a stop bias that
never stops).  One session, the alternatives alternating inside every repetition, ``--reps`` (>= 7) repetitions after a warm-up of each,
median [min .. max] of host wall-clock around calls that end with their own wait (a stream is host-driven: HIP events would miss the
host's share of a push).

    offline      Tacotron.synthesize of this build; with --parent-lib the same call through the parent commit's library built beside
                 it (``git worktree`` + ``make``), and a byte comparison of the two mels on the seeded input
    streamed     total and time to the first non-empty mel piece at chunk_steps 1, 4, 8, 32; the cost of one push is the slope of the
                 streamed total over the number of pushes
    first audio  synthesize_stream_to_wav (vocoder tail='none', synthetic weights) against offline synthesize followed by
                 WaveRNN.stream fed the finished mel in 8-frame pushes

    python tools/tacotron_stream_latency.py [--reps 8] [--parent-lib build_variants/libparent.so] [--out profiles/tacotron_stream.txt]
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

STEPS, TX, CHUNKS = 400, 60, (1, 4, 8, 32)


def parent_tacotron(path, dims, state):
    """A ``Tacotron`` whose native handle lives in another build of the library (the entries a synthesize call needs, by hand)."""
    from tacotronv2_wavernn_chinese_amd import _cabi
    from tacotronv2_wavernn_chinese_amd.tacotron import Tacotron, make_dims
    _cabi.load_library()                                   # the HIP runtime is in the process before the second library
    lib, vp = C.CDLL(os.path.abspath(path)), C.c_void_p
    for name, args, res in (('wrnn_taco_create', [C.POINTER(_cabi.TacoDims), C.POINTER(vp)], C.c_int), ('wrnn_taco_tensor_count', [vp], C.c_int),
                            ('wrnn_taco_tensor_name', [vp, C.c_int], C.c_char_p), ('wrnn_taco_tensor_shape', [vp, C.c_int, C.POINTER(C.c_int64)], C.c_int),
                            ('wrnn_taco_load_tensor', [vp, C.c_char_p, vp, C.c_int, C.POINTER(C.c_int64)], C.c_int),
                            ('wrnn_taco_synthesize', [vp, C.POINTER(_cabi.TacoCall), vp], C.c_int), ('wrnn_taco_last_error', [vp], C.c_char_p),
                            ('wrnn_taco_destroy', [vp], None)):
        fn = getattr(lib, name)
        fn.argtypes, fn.restype = args, res
    m = Tacotron(**dims)
    m.native.close()
    m.native = _cabi.NativeTacotron(make_dims(**dims), lib=lib)      # the same Python object over the other build's handle
    return m.load_state(state)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=8)
    ap.add_argument('--steps', type=int, default=STEPS)
    ap.add_argument('--parent-lib', default=None, help='libwavernn_amd.so built from the parent commit')
    ap.add_argument('--out', default=None, help='also write the report to this file')
    args = ap.parse_args()
    if args.reps < 7:
        ap.error('--reps must be at least 7')
    import torch
    from tacotronv2_wavernn_chinese_amd.synth import DEFAULT_DIMS, make_state_dict, make_tacotron_state
    from tacotronv2_wavernn_chinese_amd.tacotron import DEFAULT_TACOTRON_DIMS, Tacotron, synthesize_stream_to_wav
    from tacotronv2_wavernn_chinese_amd.vocoder import WaveRNN
    dev = torch.device('cuda', 0)
    torch.cuda.set_device(dev)
    dims = dict(DEFAULT_TACOTRON_DIMS, n_symbols=64)
    state = dict(make_tacotron_state(0, **dims))
    sp = 'decoder/stop_token_projection/projection_stop_token_projection/bias'
    state[sp] = state[sp] - np.float32(30.0)
    model = Tacotron(**dims).load_state(state)
    parent = parent_tacotron(args.parent_lib, dims, state) if args.parent_lib else None
    seq = np.random.Generator(np.random.PCG64(1)).integers(0, 64, size=TX).tolist()
    N, seed = args.steps, 100
    voc = WaveRNN(**DEFAULT_DIMS, mode='RAW')
    voc.verbose = False
    voc.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in make_state_dict(0, variant='peaky').items()})
    voc.to(dev)
    lines = []

    def say(s=''):
        print(s, flush=True)
        lines.append(s)

    def fmt(v):
        v = [x for x in v if x is not None]
        return f'{np.median(v):8.3f} [{min(v):8.3f} .. {max(v):8.3f}]' if v else '   never'.ljust(32)

    def wall(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, out

    def offline(m):
        return m.synthesize([seq], seeds=[seed], max_iters=N, return_device=True)[0]['mel']

    def streamed(chunk):
        """(ms to the first non-empty piece, pushes); the caller times the whole"""
        t0, first, pushes = time.perf_counter(), None, 0
        with model.stream([seq], seeds=[seed], max_iters=N, return_device=True) as st:
            while not st.done:
                mel = st.step(chunk)[0]['mel']
                pushes += 1
                if first is None and mel.shape[0]:
                    first = (time.perf_counter() - t0) * 1e3
        return first, pushes

    def push_spans(chunk):
        """host wall-clock of every step() of one stream (launches, the wait, the slicing), ms; without the first and the last push"""
        host = []
        with model.stream([seq], seeds=[seed], max_iters=N, return_device=True) as st:
            while not st.done:
                t0 = time.perf_counter()
                st.step(chunk)
                host.append((time.perf_counter() - t0) * 1e3)
        return host[1:-1]

    def offline_then_vocode():
        """ms to the first audio: the whole mel first, then the vocoder's stream in 8-frame pushes"""
        t0 = time.perf_counter()
        mel = offline(model)
        with voc.stream(tail='none') as vs:
            for a in range(0, mel.shape[0], 8):
                if vs.push(mel[a:a + 8].T.contiguous()).size:
                    return (time.perf_counter() - t0) * 1e3
            vs.finish()
        return float('nan')

    def stream_then_vocode():
        _, _, t_audio = synthesize_stream_to_wav(model, voc, seq, None, chunk_steps=8, seed=seed, tail='none', max_iters=N)
        return t_audio * 1e3

    say(f'Streaming Tacotron-2, reference hparams, synthetic weights, Tx = {TX}, {N} frames, {torch.cuda.get_device_name(dev)}')
    say(f'host wall-clock around calls that wait for their own results; median [min .. max] of {args.reps} repetitions after a warm-up, the')
    say('alternatives alternating inside every repetition; ms')
    say()
    # ---- the same bytes: offline of this build, of the parent's, and the stream
    want = offline(model).cpu().numpy()
    with model.stream([seq], seeds=[seed], max_iters=N) as st:
        while not st.done:
            st.step(8)
        got = st.result()[0]['mel']
        info = st.info()
    say(f'stream (8-step pushes) == offline synthesize on the {want.shape} mel: {np.array_equal(got, want)}; the stream owns {info["workspace_bytes"] / 2 ** 20:.1f} MiB '
        f'at max_iters = {N}, halo {info["halo"]}')
    if parent is not None:
        say(f'offline synthesize of this build == of the parent commit\'s library, byte for byte: {offline(parent).cpu().numpy().tobytes() == want.tobytes()}')
    # ---- warm-up of every alternative, then the repetitions
    offline(model), [streamed(c) for c in CHUNKS], offline_then_vocode(), stream_then_vocode()
    if parent is not None:
        offline(parent)
    t_off, t_par, t_tot, t_first, pushes = [], [], {c: [] for c in CHUNKS}, {c: [] for c in CHUNKS}, {}
    a_off, a_str = [], []
    spans = {c: [] for c in (1, 8)}
    for rep in range(args.reps):
        for who in ((model, parent) if rep % 2 == 0 else (parent, model)):      # the order of the two builds alternates too
            if who is not None:
                (t_off if who is model else t_par).append(wall(lambda: offline(who))[0])
        for c in CHUNKS:
            t, (first, pushes[c]) = wall(lambda: streamed(c))
            t_tot[c].append(t)
            t_first[c].append(first)
        for c in spans:
            spans[c].append(float(np.median(push_spans(c))))
        a_off.append(offline_then_vocode())
        torch.cuda.synchronize()
        a_str.append(stream_then_vocode())
        torch.cuda.synchronize()
    say()
    say(f'offline synthesize, this build        {fmt(t_off)}')
    if parent is not None:
        lo, hi = min(t_par), max(t_par)
        say(f'offline synthesize, parent\'s library  {fmt(t_par)}   this build\'s median inside the parent\'s [min .. max]: {lo <= np.median(t_off) <= hi}')
    say()
    say('chunk_steps  pushes   streamed total                      first non-empty mel piece          total - offline   first piece before offline returns')
    off_med = float(np.median(t_off))
    for c in CHUNKS:
        say(f'{c:11d}  {pushes[c]:6d}   {fmt(t_tot[c])}   {fmt(t_first[c])}   {np.median(t_tot[c]) - off_med:+15.3f}   {all(v is not None and v < off_med for v in t_first[c])}')
    # the cost of a push.  Measured: the slope of the streamed total over the number of pushes, and the spans of single pushes.
    # Derived (arithmetic on the measured figures, marked as such): the shares of a push.
    x = np.array([pushes[c] for c in CHUNKS], dtype=np.float64)
    y = np.array([np.median(t_tot[c]) for c in CHUNKS])
    slope, icpt = np.polyfit(x, y, 1)
    step_us = off_med / N * 1e3
    say()
    say(f'streamed total over pushes, least-squares line through the four chunk sizes: {icpt:.3f} ms + {slope * 1e3:.1f} us per push')
    say('one step() of a running stream, host wall-clock (median over the pushes of a stream, then over the repetitions), ms:')
    for c in spans:
        say(f'  {c} steps per push   {fmt(spans[c])}')
    w1, w8 = float(np.median(spans[1])), float(np.median(spans[8]))
    per_step = (w8 - w1) / 7
    say(f'derived from these two, not measured: a further step inside a push costs {per_step * 1e3:.1f} us (the offline call: {step_us:.1f} us per step all')
    say(f'told), so a push carries about {(w1 - per_step) * 1e3:.1f} us of its own: 8 launches, the state reloaded and stored, the postnet tiles of the new rows, the')
    say('copy of the counters, the wait, the slicing in Python')
    f8 = [v for v in t_first[8] if v is not None]
    if f8:
        f8 = float(np.median(f8))
        say(f'first piece at 8 steps per push: {f8:.3f} ms; the offline call returns after {off_med:.3f} ms: '
            f'{"earlier" if f8 < off_med else "NOT earlier"} by {off_med - f8:.3f} ms')
    say()
    say(f'time to first audio, vocoder tail=\'none\', synthetic vocoder weights, 8-step / 8-frame pushes, one HIP stream, the models taking turns:')
    say(f'  offline synthesize, then WaveRNN.stream   {fmt(a_off)}')
    say(f'  synthesize_stream_to_wav                  {fmt(a_str)}')
    if args.out:
        with open(args.out, 'w') as fh:
            fh.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
