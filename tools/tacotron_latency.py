"""Developer tool (GPU): Tacotron-2 by the library call against the same recipe from float32 PyTorch-ROCm ops.

Workload: the reference's hparams, seeded synthetic weights, a Tx = 60 sentence decoded for 400 frames (the stop projection's bias is
lowered so that neither side stops early), and a ragged queue of 8 sentences in ONE call against one call each.  The torch side restates
the same model with ``torch.nn.functional`` ops on the same GPU, one decoder step at a time like the reference's ``dynamic_decode``; it
reads the stop token on the host after every step, as a faithful port has to.  Both sides use the same dropout masks (the library's
Philox masks, handed to the torch side precomputed), so the two mels can be compared.

Timing: HIP events around the call; the two sides alternate in one session, ``--reps`` timed repetitions after a warm-up of each;
median [min .. max].  us per decoder step = (t(400 steps) - t(1 step)) / 399; the encoder's and the postnet's share come from the same
difference trick on the library side (a call with Tx = 1, a call with 1 step) and, exactly, from a kernel trace (``--calls N`` runs
nothing but N library calls for ``rocprofv3 --kernel-trace --stats``).

    python tools/tacotron_latency.py [--reps 8] [--out FILE]
    python tools/tacotron_latency.py --calls 3
"""
from __future__ import annotations

import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

QUEUE = (60, 12, 33, 47, 5, 58, 21, 40)
STEPS, HOP, SR = 400, 275, 22050


class TorchTacotron:
    """The restatement of tests/tacotron_ref.py in float32 torch ops on the GPU, batch 1."""

    def __init__(self, state, dims, dev):
        import torch
        self.t, self.d, self.dev = torch, dims, dev
        self.w = {k: torch.from_numpy(np.asarray(v)).to(dev) for k, v in state.items()}

    def conv_block(self, x, p, act):
        t, w = self.t, self.w
        k = w[p + 'conv1d/kernel']                                   # (taps, cin, cout)
        y = t.nn.functional.conv1d(x.T[None], k.permute(2, 1, 0), w[p + 'conv1d/bias'], padding=(k.shape[0] - 1) // 2)[0].T
        y = act(y)
        bn = p + 'batch_normalization/'
        return w[bn + 'gamma'] * (y - w[bn + 'moving_mean']) / t.sqrt(w[bn + 'moving_variance'] + 1e-3) + w[bn + 'beta']

    def lstm(self, x, c, h, p):
        t, w = self.t, self.w
        z = t.cat([x, h]) @ w[p + 'kernel'] + w[p + 'bias']
        i, j, f, o = z.chunk(4)
        cn = t.sigmoid(f + 1.0) * c + t.sigmoid(i) * t.tanh(j)
        hn = t.sigmoid(o) * t.tanh(cn)
        return hn, 0.9 * cn + 0.1 * c, 0.9 * hn + 0.1 * h

    def synthesize(self, seq, masks, max_iters):
        t, w, d, dev = self.t, self.w, self.d, self.dev
        x = w['inputs_embedding'][t.as_tensor(seq, device=dev)]
        for i in range(d['enc_conv_layers']):
            x = self.conv_block(x, f'encoder_convolutions/conv_layer_{i + 1}_encoder_convolutions/', t.relu)
        Tx, H = len(seq), d['encoder_lstm_units']
        outs = []
        for dr, order in (('fw', range(Tx)), ('bw', range(Tx - 1, -1, -1))):
            c, h, o = t.zeros(H, device=dev), t.zeros(H, device=dev), [None] * Tx
            for s in order:
                o[s], c, h = self.lstm(x[s], c, h, f'encoder_LSTM/bidirectional_rnn/{dr}/encoder_{dr}_LSTM/')
            outs.append(t.stack(o))
        memory = t.cat(outs, dim=1)
        keys = memory @ w['memory_layer/kernel']
        lsa = 'decoder/Location_Sensitive_Attention/'
        D, M, L = d['decoder_lstm_units'], d['num_mels'], d['decoder_layers']
        cs, hs = [t.zeros(D, device=dev) for _ in range(L)], [t.zeros(D, device=dev) for _ in range(L)]
        alpha = t.zeros(Tx, device=dev)
        alpha[0] = 1.0
        cum, mu, ctx, xin = alpha.clone(), t.tensor(0.5, device=dev), t.zeros(2 * H, device=dev), t.zeros(M, device=dev)
        mp, pp, frames, stops = 0, 0, [], []
        ck = w[lsa + 'location_features_convolution/kernel'].permute(2, 1, 0)
        idx = t.arange(Tx, device=dev)
        for s in range(max_iters):
            p = xin
            for l in range(len(d['prenet_layers'])):
                p = t.relu(p @ w[f'decoder/decoder_prenet/dense_{l + 1}/kernel'] + w[f'decoder/decoder_prenet/dense_{l + 1}/bias']) * masks[s][l]
            y = t.cat([p, ctx])
            for l in range(L):
                y, cs[l], hs[l] = self.lstm(y, cs[l], hs[l], f'decoder/decoder_LSTM/multi_rnn_cell/cell_{l}/decoder_LSTM_{l + 1}/')
            f = t.nn.functional.conv1d(cum[None, None], ck, w[lsa + 'location_features_convolution/bias'], padding=(ck.shape[2] - 1) // 2)[0].T
            e = (w[lsa + 'attention_variable_projection'] * t.tanh(keys + y @ w[lsa + 'query_layer/kernel'] + f @ w[lsa + 'location_features_layer/kernel']
                                                                 + w[lsa + 'attention_bias'])).sum(1)
            soft = t.softmax(e, 0)
            cum = cum + soft
            fwd = ((1 - mu) * alpha + mu * t.cat([alpha.new_zeros(1), alpha[:-1]]) + 1e-10) * soft
            am = int(t.argmax(fwd))                                  # the window block's integers live on the host, as in a plain port
            m = mp if am <= mp else mp + 1
            if pp < 5 and 2 < m:
                m = mp
            pos = pp + 1 if m == mp else 1
            if not pos < 10:
                m, pos = m + 1, 1
            mp, pp = m, pos
            a = t.where((idx >= m - 2) & (idx < m + 3), fwd, t.zeros_like(fwd))
            S = a.sum()
            S = t.where(S < 1e-10, t.ones_like(S), S)
            a = t.where(idx == min(m, Tx - 1), 2.0 * S, a)
            alpha = a / a.sum()
            ctx = alpha @ memory
            mu = t.sigmoid(t.cat([ctx, y]) @ w['decoder/dense/kernel'] + w['decoder/dense/bias'])[0]
            pin = t.cat([y, ctx])
            fr = pin @ w['decoder/linear_transform_projection/projection_linear_transform_projection/kernel'] + \
                w['decoder/linear_transform_projection/projection_linear_transform_projection/bias']
            st = t.sigmoid(pin @ w['decoder/stop_token_projection/projection_stop_token_projection/kernel'] +
                           w['decoder/stop_token_projection/projection_stop_token_projection/bias'])
            frames.append(fr)
            stops.append(st)
            xin = fr[-M:]
            if bool((st > 0.5).any()):
                break
        dec = t.clamp(t.stack(frames).reshape(-1, M), -4.1, 4.0)
        x = dec
        n = d['postnet_layers']
        for i in range(n):
            x = self.conv_block(x, f'postnet_convolutions/conv_layer_{i + 1}_postnet_convolutions/', t.tanh if i + 1 < n else (lambda v: v))
        raw = t.clamp(dec + x @ w['postnet_projection/projection_postnet_projection/kernel'] + w['postnet_projection/projection_postnet_projection/bias'], -4.1, 4.0)
        return t.clamp((t.clamp(raw, -4.0, 4.0) + 4.0) / 8.0, 0, 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=8)
    ap.add_argument('--steps', type=int, default=STEPS)
    ap.add_argument('--calls', type=int, default=0, help='only this many library calls on the Tx = 60 sentence (for rocprofv3 --kernel-trace)')
    ap.add_argument('--out', default=None, help='also write the report to this file')
    args = ap.parse_args()
    import torch
    from tacotronv2_wavernn_chinese_amd.synth import make_tacotron_state
    from tacotronv2_wavernn_chinese_amd.tacotron import DEFAULT_TACOTRON_DIMS, Tacotron
    from tests import tacotron_ref as ref
    dev = torch.device('cuda', 0)
    torch.cuda.set_device(dev)
    dims = dict(DEFAULT_TACOTRON_DIMS, n_symbols=64)
    state = dict(make_tacotron_state(0, **dims))
    sp = 'decoder/stop_token_projection/projection_stop_token_projection/bias'
    state[sp] = state[sp] - np.float32(30.0)                         # never stops: both sides run all the steps
    model = Tacotron(**dims).load_state(state)
    rng = np.random.Generator(np.random.PCG64(1))
    seqs = [rng.integers(0, 64, size=n).tolist() for n in QUEUE]
    seeds = list(range(100, 100 + len(QUEUE)))
    tt = TorchTacotron(state, dims, dev)
    sizes = tuple(dims['prenet_layers'])

    def masks_for(seed, steps):
        m, _ = ref.prenet_masks(seed, steps, sizes)
        return [[torch.from_numpy(np.where(k, np.float32(2), np.float32(0))).to(dev) for k in row] for row in m]
    lines = []

    def say(s=''):
        print(s, flush=True)
        lines.append(s)

    def timed(fn):
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1), out

    def lib(idx, steps):
        return model.synthesize([seqs[i] for i in idx], seeds=[seeds[i] for i in idx], max_iters=steps, return_device=True)

    if args.calls:
        lib([0], args.steps)
        torch.cuda.synchronize()
        for _ in range(args.calls):
            lib([0], args.steps)
        torch.cuda.synchronize()
        return

    def fmt(v):
        return f'{np.median(v):9.3f} [{min(v):9.3f} .. {max(v):9.3f}]'

    N = args.steps
    say(f'Tacotron-2, reference hparams, synthetic weights: ONE library call against float32 torch ops, {torch.cuda.get_device_name(dev)}')
    say(f'HIP events around the call; median [min .. max] of {args.reps} alternating repetitions after a warm-up, ms')
    say()
    m60 = {n: masks_for(seeds[0], n) for n in (1, N)}
    a, b = lib([0], N)[0]['mel'], tt.synthesize(seqs[0], m60[N], N)
    say(f'Tx = 60, {N} steps: max |library - torch| on the [0, 1] mel = {float((a - b).abs().max()):.3e} over {tuple(a.shape)}')
    med = {}
    for n in (1, N):
        lib([0], n), tt.synthesize(seqs[0], m60[n], n)
        tl, tr = [], []
        for _ in range(args.reps):
            tl.append(timed(lambda: lib([0], n))[0])
            tr.append(timed(lambda: tt.synthesize(seqs[0], m60[n], n))[0])
        med[n] = (float(np.median(tl)), float(np.median(tr)))
        say(f'Tx = 60, {n:3d} steps   library {fmt(tl)}   torch {fmt(tr)}   library / torch = {med[n][0] / med[n][1]:.4f}')
    step_us = [(med[N][i] - med[1][i]) / (N - 1) * 1e3 for i in (0, 1)]
    audio_ms = N * HOP / SR * 1e3
    say(f'per decoder step (postnet rows included): library {step_us[0]:.1f} us, torch {step_us[1]:.1f} us; {N} frames = {audio_ms:.0f} ms of audio: '
        f'real-time factor library {med[N][0] / audio_ms:.4f}, torch {med[N][1] / audio_ms:.4f}')
    t1 = [timed(lambda: model.synthesize([seqs[0][:1]], seeds=[1], max_iters=1, return_device=True))[0] for _ in range(args.reps + 1)][1:]
    say(f'Tx = 1, 1 step (the fixed cost of a call: 15 launches, 4 copies, 1 wait): library {fmt(t1)}; Tx = 60, 1 step is {med[1][0]:.3f}: '
        f'the encoder for 60 symbols is about {med[1][0] - float(np.median(t1)):.3f} ms')
    say()
    allm = [masks_for(s, N) for s in seeds]
    lib(range(len(QUEUE)), N)
    tq, to, tr = [], [], []
    for _ in range(args.reps):
        tq.append(timed(lambda: lib(range(len(QUEUE)), N))[0])
        to.append(timed(lambda: [lib([i], N) for i in range(len(QUEUE))])[0])
    for _ in range(2):
        tr.append(timed(lambda: [tt.synthesize(seqs[i], allm[i], N) for i in range(len(QUEUE))])[0])
    say(f'ragged queue {QUEUE}, {N} steps each: one call {fmt(tq)}   one by one {fmt(to)}   torch one by one (2 reps) {fmt(tr)}')
    say(f'one call / one by one = {np.median(tq) / np.median(to):.3f}')
    if args.out:
        with open(args.out, 'w') as fh:
            fh.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
