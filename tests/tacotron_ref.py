"""NumPy restatement of the reference's Tacotron-2 in synthesis mode (is_training=False), parametrised by dtype.

Restated from tacotron/models/tacotron.py, modules.py, Architecture_wrappers.py, forward_attention.py, helpers.py, custom_decoder.py and
the post-processing of tacotron_synthesize.py (TensorFlow runs on none of the project's machines, so nothing is copied or executed).
``dtype=np.float64`` is the yardstick, ``dtype=np.float32`` the same code in the device's precision: the largest difference between the
two, g, is the unit the GPU tests measure the kernels' error in.

Weights: a dict keyed by the reference graph's variable names below ``Tacotron_model/inference/`` (tacotron.tensor_shapes lists them).
The batch of the reference is 1; a batch here is a list of utterances, each computed alone (the ``reduce_all(axis=0)`` of
helpers.py:59, which would keep a finished utterance decoding until the whole batch has stopped, is deliberately not reproduced).
"""
import numpy as np

from tests.philox_ref import philox_uniform_at

ENC = 'encoder_convolutions/conv_layer_{}_encoder_convolutions/'
POST = 'postnet_convolutions/conv_layer_{}_postnet_convolutions/'
LSA = 'decoder/Location_Sensitive_Attention/'


def sigmoid(x):
    return 1.0 / (1.0 + np.exp(-x))


def conv1d_same(x, kernel, bias=None):
    """tf.layers.conv1d, padding='same', stride 1: x (T, Cin), kernel (k, Cin, Cout).  k - 1 zeros in all, (k - 1) // 2 of them in front."""
    k = kernel.shape[0]
    T = x.shape[0]
    left = (k - 1) // 2
    xp = np.zeros((T + k - 1, x.shape[1]), dtype=x.dtype)
    xp[left:left + T] = x
    y = np.zeros((T, kernel.shape[2]), dtype=x.dtype)
    for j in range(k):
        y = y + xp[j:j + T] @ kernel[j]
    return y if bias is None else y + bias


def batch_norm(x, w, prefix, eps=1e-3):
    """tf.layers.batch_normalization(training=False): gamma (x - moving_mean) / sqrt(moving_variance + eps) + beta."""
    bn = prefix + 'batch_normalization/'
    return w[bn + 'gamma'] * (x - w[bn + 'moving_mean']) / np.sqrt(w[bn + 'moving_variance'] + x.dtype.type(eps)) + w[bn + 'beta']


def conv_block(x, w, prefix, act):
    """modules.conv1d with batch_norm_position='after': conv + bias -> activation -> BatchNorm; no dropout in inference."""
    return batch_norm(act(conv1d_same(x, w[prefix + 'conv1d/kernel'], w[prefix + 'conv1d/bias'])), w, prefix)


def lstm_cell(x, c, h, kernel, bias):
    """tf.nn.rnn_cell.LSTMCell: [x; h] @ kernel + bias, gates i, j, f, o, forget_bias 1.0.  Returns the new (c, h)."""
    z = np.concatenate([x, h]) @ kernel + bias
    i, j, f, o = np.split(z, 4)
    one = z.dtype.type(1.0)
    c_new = sigmoid(f + one) * c + sigmoid(i) * np.tanh(j)
    return c_new, sigmoid(o) * np.tanh(c_new)


def zoneout_lstm(x, c, h, kernel, bias, z=0.1):
    """ZoneoutLSTMCell in inference: returns (output, c_state, h_state).  The output is the cell's un-mixed new h; the state that goes
    to the next step is (1 - z) new + z prev, for c and for h."""
    c_new, h_new = lstm_cell(x, c, h, kernel, bias)
    zz = x.dtype.type(z)
    one = x.dtype.type(1.0)
    return h_new, (one - zz) * c_new + zz * c, (one - zz) * h_new + zz * h


def encoder(w, seq, dtype, n_conv=3, zoneout=0.1):
    """(Tx,) symbol ids -> (Tx, 2 H) encoder outputs: embedding, the conv stack, the BiLSTM (backward over the reversed sequence)."""
    x = w['inputs_embedding'][np.asarray(seq)].astype(dtype)
    for i in range(n_conv):
        x = conv_block(x, w, ENC.format(i + 1), lambda v: np.maximum(v, 0))
    outs = []
    for d, order in (('fw', range(len(seq))), ('bw', range(len(seq) - 1, -1, -1))):
        k = w[f'encoder_LSTM/bidirectional_rnn/{d}/encoder_{d}_LSTM/kernel']
        b = w[f'encoder_LSTM/bidirectional_rnn/{d}/encoder_{d}_LSTM/bias']
        H = b.shape[0] // 4
        c, h = np.zeros(H, dtype), np.zeros(H, dtype)
        o = np.zeros((len(seq), H), dtype)
        for t in order:
            o[t], c, h = zoneout_lstm(x[t], c, h, k, b, zoneout)
        outs.append(o)
    return np.concatenate(outs, axis=1)


def attention_window(max_prev, pos_prev, argmax_now):
    """The integer part of forward_attention.py:171-196.  Returns (max_attentions, pos_rec, arm): arm names the path taken, a subset of
    'stay', 'advance', 'hold' (pos_rec < 5 keeps an advance back) and 'push' (pos_rec reaching 10 forces one)."""
    arm = []
    m = max_prev if argmax_now <= max_prev else max_prev + 1
    arm.append('stay' if argmax_now <= max_prev else 'advance')
    if pos_prev < 5 and 2 < m:
        if m != max_prev:
            arm.append('hold')
        m = max_prev
    pos = pos_prev + 1 if m == max_prev else 1
    if not pos < 10:
        m, pos = m + 1, 1
        arm.append('push')
    return m, pos, arm


def attention_step(w, memory, keys, query, st, dtype, inference_block=True):
    """ForwardLocationSensitiveAttention.__call__.  ``st``: dict with alignments (= alpha), cum, mu, max_attentions, pos_rec.
    Returns (alignments, new_mu, context, cum, max_attentions, pos_rec, trace)."""
    Tx = memory.shape[0]
    t = dtype
    pq = query @ w[LSA + 'query_layer/kernel']
    f = conv1d_same(st['cum'][:, None], w[LSA + 'location_features_convolution/kernel'], w[LSA + 'location_features_convolution/bias'])
    pl = f @ w[LSA + 'location_features_layer/kernel']
    energy = np.sum(w[LSA + 'attention_variable_projection'] * np.tanh(keys + pq[None, :] + pl + w[LSA + 'attention_bias']), axis=1)
    e = np.exp(energy - energy.max())
    soft = e / e.sum()
    cum = st['cum'] + soft
    mu, alpha = st['mu'], st['alpha']
    shift = np.concatenate([np.zeros(1, dtype), alpha[:-1]])
    fwd = ((t(1.0) - mu) * alpha + mu * shift + t(1e-10)) * soft
    am = int(np.argmax(fwd))
    trace = {'energy': energy, 'softmax': soft, 'forward': fwd, 'argmax': am}
    m, pos = am, st['pos_rec']
    a = fwd
    if inference_block:
        m, pos, trace['arm'] = attention_window(st['max_attentions'], st['pos_rec'], am)
        idx = np.arange(Tx)
        a = np.where((idx >= m - 2) & (idx < m + 3), fwd, t(0.0))
        s = a.sum()
        s = t(1.0) if s < t(1e-10) else s
        a = np.where(idx == min(max(m, 0), Tx - 1), s * t(2.0), a)
    a = a / a.sum()
    context = a @ memory
    new_mu = sigmoid(np.concatenate([context, query]) @ w['decoder/dense/kernel'] + w['decoder/dense/bias'])[0]
    return a, new_mu, context, cum, m, pos, trace


def prenet_masks(seed, steps, sizes):
    """The keep masks of the prenet's dropout (rate 0.5, always on): layer l of step s keeps unit k when
    wrnn_uniform(seed, s * len(sizes) + l, row 0, k) >= 0.5.  Returns [steps][layer] bool arrays and the uniforms themselves."""
    L = len(sizes)
    u = philox_uniform_at(seed, np.arange(steps * L, dtype=np.uint64), [0], max(sizes))[:, 0, :]
    return [[u[s * L + l, :sizes[l]] >= np.float32(0.5) for l in range(L)] for s in range(steps)], u


def decode(w, memory, dtype, *, num_mels, r, prenet_sizes, decoder_layers, max_iters, seed=0, prenet_dropout=True, gta_target=None,
           zoneout=0.1, force_masks=None):
    """The decoder loop (custom_decoder.step under dynamic_decode).  Every step emits its r frames and r stop probabilities; the loop
    ends AFTER the step whose stop rounds to 1 (round-half-even: p > 0.5) for any of its r tokens, so that step's frames are emitted
    too, or at max_iters.  With ``gta_target`` (T, num_mels), T a multiple of r, the input of step s >= 1 is target frame s r - 1 and the
    loop runs T / r steps whatever the stop says (TacoTrainingHelper).  Returns a dict of per-step arrays."""
    Tx = memory.shape[0]
    keys = memory @ w['memory_layer/kernel']
    D = w['decoder/decoder_LSTM/multi_rnn_cell/cell_0/decoder_LSTM_1/bias'].shape[0] // 4
    cs = [np.zeros(D, dtype) for _ in range(decoder_layers)]
    hs = [np.zeros(D, dtype) for _ in range(decoder_layers)]
    onehot = np.zeros(Tx, dtype)
    onehot[0] = 1
    st = {'alpha': onehot.copy(), 'cum': onehot.copy(), 'mu': dtype(0.5), 'max_attentions': 0, 'pos_rec': 0}
    context = np.zeros(memory.shape[1], dtype)
    x = np.zeros(num_mels, dtype)
    steps = max_iters if gta_target is None else gta_target.shape[0] // r
    masks = force_masks if force_masks is not None else (prenet_masks(seed, steps, prenet_sizes)[0] if prenet_dropout else None)
    out = {k: [] for k in ('frames', 'stop', 'alignments', 'max_attentions', 'pos_rec', 'argmax', 'forward', 'prenet', 'mu', 'arms', 'query', 'stop_logit')}
    for s in range(steps):
        p = x
        for l in range(len(prenet_sizes)):
            p = np.maximum(p @ w[f'decoder/decoder_prenet/dense_{l + 1}/kernel'] + w[f'decoder/decoder_prenet/dense_{l + 1}/bias'], 0)
            if masks is not None:
                p = np.where(masks[s][l], p * dtype(2.0), dtype(0.0))
        out['prenet'].append(p)
        y = np.concatenate([p, context])
        for l in range(decoder_layers):
            pre = f'decoder/decoder_LSTM/multi_rnn_cell/cell_{l}/decoder_LSTM_{l + 1}/'
            y, cs[l], hs[l] = zoneout_lstm(y, cs[l], hs[l], w[pre + 'kernel'], w[pre + 'bias'], zoneout)
        a, mu, context, cum, m, pos, tr = attention_step(w, memory, keys, y, st, dtype)
        st = {'alpha': a, 'cum': cum, 'mu': mu, 'max_attentions': m, 'pos_rec': pos}
        pin = np.concatenate([y, context])
        lp, sp = 'decoder/linear_transform_projection/projection_linear_transform_projection/', 'decoder/stop_token_projection/projection_stop_token_projection/'
        frames = pin @ w[lp + 'kernel'] + w[lp + 'bias']
        stop_logit = pin @ w[sp + 'kernel'] + w[sp + 'bias']
        stop = sigmoid(stop_logit)
        for k, v in (('frames', frames), ('stop', stop), ('alignments', a), ('max_attentions', m), ('pos_rec', pos), ('argmax', tr['argmax']),
                     ('forward', tr['forward']), ('mu', mu), ('arms', tr['arm']), ('query', y), ('stop_logit', stop_logit)):
            out[k].append(v)
        if gta_target is None:
            x = frames[-num_mels:]
            if np.any(np.round(stop) == 1):
                break
        else:
            x = gta_target[(s + 1) * r - 1].astype(dtype)
    n = len(out['frames'])
    res = {k: np.array(v) for k, v in out.items() if k != 'arms'}
    res['arms'] = out['arms']
    res['steps'] = n
    res['frames'] = res['frames'].reshape(n * r, num_mels)
    res['stop'] = res['stop'].reshape(n * r)
    return res


def postprocess(w, frames, stop, dtype, *, postnet_layers=5, max_abs=4.0, lower=0.1, trim=True):
    """tacotron.py:111-129 and tacotron_synthesize.py:100-116: clip, postnet, projection, residual, clip; then the trim to the first
    stop token that rounds to 1 (the stopping frame itself goes), clip to [-max_abs, max_abs], and the map to [0, 1]."""
    lo, hi = dtype(-max_abs - lower), dtype(max_abs)
    dec = np.minimum(np.maximum(frames, lo), hi)
    x = dec
    for i in range(postnet_layers - 1):
        x = conv_block(x, w, POST.format(i + 1), np.tanh)
    x = conv_block(x, w, POST.format(postnet_layers), lambda v: v)
    pp = 'postnet_projection/projection_postnet_projection/'
    raw = np.minimum(np.maximum(dec + (x @ w[pp + 'kernel'] + w[pp + 'bias']), lo), hi)
    hit = np.flatnonzero(np.round(stop) == 1)
    length = int(hit[0]) if (trim and hit.size) else len(stop)
    mel = np.clip(raw[:length], -hi, hi)
    return {'decoder_output': dec, 'mel_raw': raw, 'mel_length': length, 'mel': np.clip((mel + hi) / (dtype(2.0) * hi), 0, 1)}


def synthesize(w, seq, dtype, *, num_mels, r, prenet_sizes, decoder_layers=2, enc_conv_layers=3, postnet_layers=5, max_iters=2000, seed=0,
               prenet_dropout=True, gta_target=None, zoneout=0.1, force_masks=None):
    """One utterance, end to end, in ``dtype``.  Returns the decoder's per-step arrays, the encoder outputs and the post-processed mels."""
    w = {k: np.asarray(v).astype(dtype) for k, v in w.items()}
    dt = np.dtype(dtype).type
    memory = encoder(w, seq, dt, enc_conv_layers, zoneout)
    res = decode(w, memory, dt, num_mels=num_mels, r=r, prenet_sizes=prenet_sizes, decoder_layers=decoder_layers, max_iters=max_iters, seed=seed,
                 prenet_dropout=prenet_dropout, gta_target=gta_target, zoneout=zoneout, force_masks=force_masks)
    res['encoder_outputs'] = memory
    res.update(postprocess(w, res['frames'], res['stop'], dt, postnet_layers=postnet_layers, trim=gta_target is None))
    return res
