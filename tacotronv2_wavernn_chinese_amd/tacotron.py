"""Tacotron-2 inference on the device: pinyin symbols -> the (T, num_mels) mel in [0, 1] that ``WaveRNN.generate`` vocodes.

The model is the reference's default one (``tacotron/models/tacotron.py`` with ``ForwardLocationSensitiveAttention``), in synthesis
mode and in GTA (teacher-forced) mode; the kernels are in ``csrc/tacotron.hip``.  Weights are an ``.npz`` keyed by the reference graph's
variable names below ``Tacotron_model/inference/`` (``Tacotron.tensor_shapes()`` lists them with their shapes; INTEGRATION.md has the
table).  Hanzi -> pinyin is not done here: the input is the space-separated pinyin the reference's ``get_pyin`` returns.
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, List, Optional, Sequence

import numpy as np

from . import _cabi

# the reference's tacotron_hparams.py
DEFAULT_TACOTRON_DIMS = dict(n_symbols=256, num_mels=80, outputs_per_step=1, embedding_dim=128, enc_conv_layers=3, enc_conv_channels=256,
                             enc_conv_kernel=5, encoder_lstm_units=256, attention_dim=128, attention_filters=32, attention_kernel=31,
                             prenet_layers=(256, 256), decoder_layers=2, decoder_lstm_units=256, postnet_layers=5, postnet_channels=256,
                             postnet_kernel=5, zoneout=0.1, max_abs_value=4.0, lower_bound_decay=0.1, bn_epsilon=1e-3)
KEY_PREFIX = 'Tacotron_model/inference/'   # a key may carry it, and TensorFlow's ':0'


def load_symbols(path: str) -> List[str]:
    """The reference's ``utils/symbols.py``: ``['_', '~']`` + the sorted set of the tokens after the last ``|`` of every line of the
    training list."""
    chars = set()
    with open(path, 'r', encoding='utf-8') as f:
        for line in f:
            for w in line.strip().split('|')[-1].strip().split(' '):
                chars.add(w)
    return ['_', '~'] + sorted(chars)


def read_metadata(path: str) -> Dict[str, str]:
    """The reference's training list (``audio-000001.npy|mel-000001.npy|46200|168|text|pinyin``) as ``{key: pinyin}``: the key is the
    stem of field 0 with a leading ``audio-`` removed (the clip ``000001.wav`` the preprocessor made it from), the pinyin the last
    field.  ``load_symbols`` on the same file gives the symbol table."""
    import os
    out = {}
    with open(path, 'r', encoding='utf-8') as f:
        for line in f:
            parts = line.strip().split('|')
            if len(parts) < 2 or not parts[0].strip():
                continue
            key = os.path.splitext(os.path.basename(parts[0].strip()))[0]
            out[key[len('audio-'):] if key.startswith('audio-') else key] = parts[-1].strip()
    return out


def metadata_sequences(metadata: Dict[str, str], stems: Sequence[str], symbols: Sequence[str], source: str = 'the metadata') -> List[List[int]]:
    """The id sequence of every clip of ``stems`` (a clip's stem looks up its line of ``read_metadata``); a stem without a line is a
    ``ValueError`` that names it."""
    seqs = []
    for stem in stems:
        key = stem[len('audio-'):] if stem.startswith('audio-') else stem
        if key not in metadata:
            raise ValueError(f'clip {stem!r} has no line in {source}')
        seqs.append(text_to_sequence(metadata[key], symbols))
    return seqs


def text_to_sequence(pinyin, symbols: Sequence[str]) -> List[int]:
    """``utils/text.py:18-31``: a string is split at single spaces, tokens outside the table are dropped, ``~`` (EOS) is appended."""
    table = {s: i for i, s in enumerate(symbols)}
    words = pinyin.split(' ') if isinstance(pinyin, str) else pinyin
    return [table[w] for w in words if w in table] + [table['~']]


def make_dims(device: int = 0, **dims) -> _cabi.TacoDims:
    d = dict(DEFAULT_TACOTRON_DIMS)
    unknown = set(dims) - set(d)
    if unknown:
        raise TypeError(f'unknown Tacotron dims: {sorted(unknown)}')
    d.update(dims)
    pre = tuple(int(p) for p in d['prenet_layers'])
    if not 1 <= len(pre) <= _cabi.TACO_MAX_PRENET:
        raise _cabi.WrnnError(_cabi.ERR_INVALID, f'unsupported dims: {len(pre)} prenet layers, 1 .. {_cabi.TACO_MAX_PRENET} are served')
    t = _cabi.TacoDims()
    t.struct_size = C.sizeof(_cabi.TacoDims)
    t.device = int(device)
    for k in ('n_symbols', 'num_mels', 'outputs_per_step', 'embedding_dim', 'enc_conv_layers', 'enc_conv_channels', 'enc_conv_kernel',
              'encoder_lstm_units', 'attention_dim', 'attention_filters', 'attention_kernel', 'decoder_layers', 'decoder_lstm_units',
              'postnet_layers', 'postnet_channels', 'postnet_kernel'):
        setattr(t, k, int(d[k]))
    t.prenet_layers = len(pre)
    for i, p in enumerate(pre):
        t.prenet_sizes[i] = p
    for k in ('zoneout', 'max_abs_value', 'lower_bound_decay', 'bn_epsilon'):
        setattr(t, k, float(d[k]))
    return t


def pack_text(sequences, seeds):
    """A ragged list of id lists -> ids (B, Tx_max) int32 padded with 0, tx (B) int32, seeds (B) uint64 (default 0, 1, ...)."""
    seqs = [np.asarray(s, dtype=np.int64).reshape(-1) for s in sequences]
    B = len(seqs)
    if B < 1:
        raise _cabi.WrnnError(_cabi.ERR_INVALID, 'no utterances')
    tx = np.array([len(s) for s in seqs], dtype=np.int32)
    Tx_max = int(tx.max()) if tx.size else 0
    ids = np.zeros((B, Tx_max), dtype=np.int32)
    for b, s in enumerate(seqs):
        if s.size and (s.min() < -2 ** 31 or s.max() >= 2 ** 31):
            raise _cabi.WrnnError(_cabi.ERR_INVALID, f'utterance {b}: a symbol id does not fit 32 bits')
        ids[b, :len(s)] = s
    seeds_a = np.array(list(range(B)) if seeds is None else [int(x) & (2 ** 64 - 1) for x in seeds], dtype=np.uint64)
    if seeds_a.shape != (B,):
        raise _cabi.WrnnError(_cabi.ERR_INVALID, f'{seeds_a.size} seeds for {B} utterances')
    return ids, tx, seeds_a


def pad_gta_target(target: np.ndarray, r: int, max_abs_value: float) -> np.ndarray:
    """A (T, num_mels) target with T brought up to a multiple of ``r`` by rows of ``-max_abs_value``: the reference's
    ``padding_targets`` (``tacotron/feeder.py``), what ``synthesize(gta_targets=...)`` feeds the decoder."""
    if target.shape[0] % r:
        target = np.pad(target, [(0, r - target.shape[0] % r), (0, 0)], mode='constant', constant_values=-float(max_abs_value))
    return target


def stream_halo(postnet_layers: int, postnet_kernel: int) -> int:
    """Decoder frames a mel frame waits for: each postnet layer reaches ``(k - 1) - (k - 1) // 2`` rows to the right ('same' padding
    puts ``(k - 1) // 2`` of a kernel's taps on the left); the 1-tap projection adds nothing."""
    k = int(postnet_kernel)
    return int(postnet_layers) * ((k - 1) - (k - 1) // 2)


def stream_release(decoded_frames: int, finished: bool, mel_length: int, postnet_layers: int, postnet_kernel: int) -> int:
    """Leading mel frames of a stream that are final: ``decoded_frames - halo`` (floored at 0) while the utterance is running, all
    ``mel_length`` of them once it has finished (a stop token above 0.5, or ``max_iters`` steps).  ``wrnn_taco_stream_step`` reports
    the same number."""
    if finished:
        return int(mel_length)
    return max(int(decoded_frames) - stream_halo(postnet_layers, postnet_kernel), 0)


class _DeviceArray:
    """A device buffer the library owns, for ``torch.as_tensor`` (no copy)."""

    def __init__(self, ptr: int, shape, typestr: str):
        self.__cuda_array_interface__ = dict(shape=tuple(int(n) for n in shape), typestr=typestr, data=(int(ptr), False), version=2, strides=None)


class TacotronStream:
    """``Tacotron.stream(...)``: a free-running ``synthesize`` cut into pushes of decoder steps.  ``step(n)`` runs up to ``n`` more
    steps of every unfinished utterance and returns, per utterance, what became final: ``mel`` and ``mel_raw`` rows by the release
    rule (:func:`stream_release`), ``decoder_output``, ``stop_tokens``, ``alignments`` and ``max_attentions`` of the steps just run.
    The pieces of an utterance, concatenated over any partition into pushes, are ``synthesize``'s arrays bit for bit.  With
    ``return_device=True`` the pieces are views of the stream's own buffers, valid until ``close()``; ``result()`` returns copies."""

    def __init__(self, model: 'Tacotron', sequences, seeds, max_iters: int, prenet_dropout: bool, return_device: bool, gta_targets=None):
        import torch
        self._ns = None
        ids, tx, seeds_a = pack_text(sequences, seeds)
        self.model, self.return_device = model, bool(return_device)
        self.B, self.Tx_max, self.S = ids.shape[0], ids.shape[1], int(max_iters)
        self._tx = [int(t) for t in tx]
        self._dev = torch.device('cuda', model.device)
        o = _cabi.TacoStreamOpts()
        o.struct_size = C.sizeof(_cabi.TacoStreamOpts)
        o.B, o.Tx_max, o.max_iters, o.prenet_dropout = self.B, self.Tx_max, self.S, int(bool(prenet_dropout))
        o.ids_host, o.tx_host, o.seeds_host = ids.ctypes.data, tx.ctypes.data, seeds_a.ctypes.data
        if gta_targets is not None:
            o.gta_dev = ids.ctypes.data   # any address: the library refuses a target before it looks at it
        with torch.cuda.device(self._dev):
            self._ns = model.native.stream_open(o, torch.cuda.current_stream(self._dev).cuda_stream)
            v = self._ns.view()
            r, M, S, Tx, E2 = model.r, model.num_mels, self.S, self.Tx_max, 2 * int(model.dims['encoder_lstm_units'])
            view = lambda ptr, shape, t='<f4': torch.as_tensor(_DeviceArray(ptr, shape, t), device=self._dev)
            self._buf = dict(encoder_outputs=view(v.encoder_dev, (self.B, Tx, E2)), decoder_output=view(v.decoder_dev, (self.B, S * r, M)),
                             mel_raw=view(v.mel_raw_dev, (self.B, S * r, M)), mel=view(v.mel_dev, (self.B, S * r, M)),
                             alignments=view(v.alignments_dev, (self.B, S, Tx)), stop_tokens=view(v.stop_dev, (self.B, S * r)),
                             max_attentions=view(v.max_attentions_dev, (self.B, S), '<i4'))
        self.decoded = [0] * self.B        # decoder frames so far
        self.final = [0] * self.B          # mel frames released so far
        self.final_raw = [0] * self.B      # mel_raw rows released so far: the stopping step's rows too
        self.finished = [False] * self.B

    @property
    def done(self) -> bool:
        return all(self.finished)

    def info(self) -> dict:
        return self._live().info()

    def _live(self):
        if self._ns is None:
            raise _cabi.WrnnError(_cabi.ERR_STATE, 'the stream is closed')
        return self._ns

    def _out(self, t):
        return t if self.return_device else t.cpu().numpy()

    def step(self, n: int):
        import torch
        ns = self._live()
        with torch.cuda.device(self._dev):
            dec, fin, done = ns.step(int(n), torch.cuda.current_stream(self._dev).cuda_stream)
        r, halo, out, buf = self.model.r, self.model.halo, [], self._buf
        for b in range(self.B):
            d0, f0, w0 = self.decoded[b], self.final[b], self.final_raw[b]
            d1, f1 = dec[b], fin[b]
            w1 = d1 if done[b] else max(d1 - halo, 0)
            res = {'mel': buf['mel'][b, f0:f1], 'mel_raw': buf['mel_raw'][b, w0:w1], 'decoder_output': buf['decoder_output'][b, d0:d1],
                   'stop_tokens': buf['stop_tokens'][b, d0:d1], 'alignments': buf['alignments'][b, d0 // r:d1 // r, :self._tx[b]],
                   'max_attentions': buf['max_attentions'][b, d0 // r:d1 // r]}
            out.append({k: self._out(t) for k, t in res.items()})
            self.decoded[b], self.final[b], self.final_raw[b], self.finished[b] = d1, f1, w1, done[b]
        return out

    def result(self):
        """What ``synthesize`` returns for the same arguments, from the stream's buffers; only once every utterance has finished."""
        self._live()
        if not self.done:
            raise _cabi.WrnnError(_cabi.ERR_STATE, 'result() before every utterance has finished: call step() until .done')
        r, buf, out = self.model.r, self._buf, []
        for b in range(self.B):
            d, f, t = self.decoded[b], self.final[b], self._tx[b]
            res = {'mel': buf['mel'][b, :f], 'mel_raw': buf['mel_raw'][b, :d], 'decoder_output': buf['decoder_output'][b, :d],
                   'alignments': buf['alignments'][b, :d // r, :t], 'stop_tokens': buf['stop_tokens'][b, :d],
                   'max_attentions': buf['max_attentions'][b, :d // r], 'encoder_outputs': buf['encoder_outputs'][b, :t]}
            res = {k: (v.clone() if self.return_device else v.cpu().numpy()) for k, v in res.items()}
            res['steps'], res['mel_length'] = d // r, f
            out.append(res)
        return out

    def close(self):
        if self._ns is not None:
            self._buf = None
            self._ns.close()
            self._ns = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Tacotron:
    """``Tacotron(**dims)`` -> ``load(path)`` or ``load_state(dict)`` -> ``synthesize(sequences, ...)``."""

    def __init__(self, device: int = 0, **dims):
        self.dims = dict(DEFAULT_TACOTRON_DIMS)
        self.dims.update(dims)
        self.device = int(device)
        self.native = _cabi.NativeTacotron(make_dims(device, **dims))
        self.r, self.num_mels = int(self.dims['outputs_per_step']), int(self.dims['num_mels'])
        self.halo = stream_halo(self.dims['postnet_layers'], self.dims['postnet_kernel'])
        self.checkpoint = None   # the file ``load`` read, by name (a GTA corpus notes it)

    def tensor_shapes(self) -> Dict[str, tuple]:
        return self.native.tensor_shapes()

    def load_state(self, state: Dict[str, np.ndarray]) -> 'Tacotron':
        """Every tensor of the table must be there (``WRNN_ERR_MISSING_KEY`` names the first that is not); keys the model does not have
        (the optimiser's slots of a converted checkpoint) are ignored."""
        clean = {}
        for k, v in state.items():
            k = k[len(KEY_PREFIX):] if k.startswith(KEY_PREFIX) else k
            clean[k[:-2] if k.endswith(':0') else k] = v
        for name in self.tensor_shapes():
            if name not in clean:
                raise _cabi.WrnnError(-4, f'tensor {name} is missing from the checkpoint')
            self.native.load_tensor(name, np.asarray(clean[name]))
        return self

    def load(self, path: str) -> 'Tacotron':
        import os
        with np.load(path, allow_pickle=False) as z:
            self.load_state({k: z[k] for k in z.files})
        self.checkpoint = os.path.basename(str(path))
        return self

    def synthesize(self, sequences, seeds=None, max_iters: int = 2000, gta_targets=None, prenet_dropout: bool = True, return_device: bool = False):
        """``sequences``: a list of id lists (a ragged batch; each utterance comes out as the call on it alone).  ``seeds``: one int per
        utterance for its prenet dropout masks (default 0, 1, ...).  ``gta_targets``: ``None``, or one ``(T, num_mels)`` array per utterance
        in the model's own range (``[-max_abs_value, max_abs_value]``): teacher forcing, T / r steps whatever the stop token says; a T
        that is no multiple of r is padded with ``-max_abs_value`` rows first, as the reference's ``padding_targets`` would.
        Returns one dict per utterance: ``mel`` (T, num_mels) in [0, 1], trimmed at the first stop token above 0.5 when free-running,
        ``mel_raw``, ``decoder_output`` (all the frames the decoder emitted, the stopping one included), ``alignments`` (steps, Tx),
        ``stop_tokens``, ``max_attentions``, ``steps``, ``encoder_outputs`` -- numpy arrays, or torch tensors on the device with
        ``return_device=True`` (``mel`` then feeds ``WaveRNN.generate`` without a copy to the host)."""
        import torch
        ids, tx, seeds_a = pack_text(sequences, seeds)
        B, Tx_max = ids.shape
        dev = torch.device('cuda', self.device)
        r, M = self.r, self.num_mels
        call = _cabi.TacoCall()
        call.struct_size = C.sizeof(_cabi.TacoCall)
        gta_dev = gta_frames = None
        if gta_targets is not None:
            if len(gta_targets) != B:
                raise _cabi.WrnnError(_cabi.ERR_INVALID, f'{len(gta_targets)} targets for {B} utterances')
            tg = []
            for b, t in enumerate(gta_targets):
                t = np.asarray(t, dtype=np.float32)
                if t.ndim != 2 or t.shape[1] != M or t.shape[0] < 1:
                    raise _cabi.WrnnError(_cabi.ERR_INVALID, f'target {b}: shape {t.shape}, (T >= 1, {M}) is needed')
                tg.append(pad_gta_target(t, r, float(self.dims['max_abs_value'])))
            gta_frames = np.array([t.shape[0] for t in tg], dtype=np.int32)
            gmax = int(gta_frames.max())
            packed = np.zeros((B, gmax, M), dtype=np.float32)
            for b, t in enumerate(tg):
                packed[b, :t.shape[0]] = t
            gta_dev = torch.from_numpy(packed).to(dev)
            S = gmax // r
            call.gta_dev, call.gta_max, call.gta_frames_host = gta_dev.data_ptr(), gmax, gta_frames.ctypes.data
        else:
            S = int(max_iters)
            if S < 1:
                raise _cabi.WrnnError(_cabi.ERR_INVALID, f'max_iters {max_iters} < 1')
        E2 = 2 * int(self.dims['encoder_lstm_units'])
        with torch.cuda.device(dev):
            enc = torch.empty((B, Tx_max, E2), dtype=torch.float32, device=dev)
            dec = torch.empty((B, S * r, M), dtype=torch.float32, device=dev)
            raw, mel = torch.empty_like(dec), torch.empty_like(dec)
            ali = torch.empty((B, S, Tx_max), dtype=torch.float32, device=dev)
            stop = torch.empty((B, S * r), dtype=torch.float32, device=dev)
            maxatt = torch.empty((B, S), dtype=torch.int32, device=dev)
            steps = torch.empty((B,), dtype=torch.int32, device=dev)
            frames = torch.empty((B,), dtype=torch.int32, device=dev)
            call.B, call.Tx_max, call.max_iters, call.prenet_dropout, call.steps_max = B, Tx_max, max(int(max_iters), 1), int(bool(prenet_dropout)), S
            call.ids_host, call.tx_host, call.seeds_host = ids.ctypes.data, tx.ctypes.data, seeds_a.ctypes.data
            call.encoder_dev, call.decoder_dev, call.mel_raw_dev, call.mel_dev = enc.data_ptr(), dec.data_ptr(), raw.data_ptr(), mel.data_ptr()
            call.alignments_dev, call.stop_dev, call.max_attentions_dev = ali.data_ptr(), stop.data_ptr(), maxatt.data_ptr()
            call.steps_dev, call.mel_frames_dev = steps.data_ptr(), frames.data_ptr()
            self.native.synthesize(call, torch.cuda.current_stream(dev).cuda_stream)
            n_steps, n_frames = steps.cpu().numpy(), frames.cpu().numpy()   # the one wait of the call: the lengths the slices below need
        out = []
        for b in range(B):
            n, f, t = int(n_steps[b]), int(n_frames[b]), int(tx[b])
            res = {'mel': mel[b, :f], 'mel_raw': raw[b, :n * r], 'decoder_output': dec[b, :n * r], 'alignments': ali[b, :n, :t],
                   'stop_tokens': stop[b, :n * r], 'max_attentions': maxatt[b, :n], 'encoder_outputs': enc[b, :t]}
            if not return_device:
                res = {k: v.cpu().numpy() for k, v in res.items()}
            res['steps'], res['mel_length'] = n, f
            out.append(res)
        return out

    def stream(self, sequences, seeds=None, max_iters: int = 2000, prenet_dropout: bool = True, return_device: bool = False,
               gta_targets=None) -> TacotronStream:
        """A :class:`TacotronStream` over a free-running ``synthesize(sequences, seeds, max_iters, prenet_dropout=...)``: the encoder
        runs here, the decoder and the postnet in ``step(n)``.  A context manager.  ``gta_targets`` is refused (``WRNN_ERR_INVALID``):
        teacher forcing has the whole target in hand and is not streamed."""
        return TacotronStream(self, sequences, seeds, max_iters, prenet_dropout, return_device, gta_targets)

    def synthesize_stream(self, sequence, chunk_steps: int = 8, **kw):
        """Generator over one utterance: the non-empty ``mel`` pieces of ``stream([sequence], **kw)`` stepped ``chunk_steps`` at a time
        (``seeds=[seed]``, ``max_iters``, ``prenet_dropout``, ``return_device`` as for :meth:`stream`).  Concatenated they are
        ``synthesize([sequence], ...)[0]['mel']``.  The stream is closed when the generator ends, so with ``return_device=True`` the
        pieces are copies on the device, not views of the stream's buffers: a piece the consumer keeps stays valid."""
        with self.stream([sequence], **kw) as st:
            while not st.done:
                mel = st.step(chunk_steps)[0]['mel']
                if mel.shape[0]:
                    yield mel.clone() if st.return_device else mel


def synthesize_stream_to_wav(model: Tacotron, voc, seq, path, chunk_steps: int = 8, seed: int = 0, tail: str = 'reference', max_iters: int = 2000,
                             mu_law: bool = True, return_result: bool = False, **voc_kw):
    """Text to audio with both halves streaming: every ``mel`` piece of ``model.stream([seq], seeds=[seed])`` goes, transposed to
    ``(num_mels, k)`` and still on the device, into ``voc.stream(tail=tail, mu_law=mu_law, **voc_kw).push``; then ``finish()``.  The two
    models take turns on one HIP stream.  Writes the wav to ``path`` (``None``: no file) and returns (audio float64, seconds from the
    call to the first mel piece, seconds to the first audio samples; ``None`` for a time whose event never came).  With
    ``tail='reference'`` the audio is what ``voc.generate(mel.T[None], path, False, ..., mu_law)`` makes of ``synthesize``'s mel after the
    same ``torch.manual_seed``.  ``return_result=True`` appends the Tacotron stream's ``result()[0]`` (device copies): the text is
    decoded once for the mel and the audio."""
    import time
    from .dsp import save_wav
    t0 = time.perf_counter()
    t_mel = t_audio = None
    pieces = []
    with model.stream([seq], seeds=[seed], max_iters=max_iters, return_device=True) as ts, voc.stream(tail=tail, mu_law=mu_law, **voc_kw) as vs:
        while not ts.done:
            mel = ts.step(chunk_steps)[0]['mel']
            if not mel.shape[0]:
                continue
            if t_mel is None:
                t_mel = time.perf_counter() - t0
            pieces.append(vs.push(mel.T.contiguous()))
            if t_audio is None and pieces[-1].size:
                t_audio = time.perf_counter() - t0
        pieces.append(vs.finish())
        if t_audio is None and pieces[-1].size:
            t_audio = time.perf_counter() - t0
        res = ts.result()[0] if return_result else None
    audio = np.concatenate(pieces)
    if path is not None:
        save_wav(audio, path, voc.sample_rate)
    return (audio, t_mel, t_audio, res) if return_result else (audio, t_mel, t_audio)


def dims_from_state(state: Dict[str, np.ndarray]) -> dict:
    """The model's dims read off a checkpoint's tensor shapes (``zoneout`` and the clip range are not in it: the reference's values)."""
    s = {}
    for k, v in state.items():
        k = k[len(KEY_PREFIX):] if k.startswith(KEY_PREFIX) else k
        s[k[:-2] if k.endswith(':0') else k] = tuple(np.shape(v))

    def count(fmt):
        n = 0
        while fmt.format(n + 1) in s:
            n += 1
        return n
    enc, post = 'encoder_convolutions/conv_layer_{}_encoder_convolutions/conv1d/kernel', 'postnet_convolutions/conv_layer_{}_postnet_convolutions/conv1d/kernel'
    pre, lstm = 'decoder/decoder_prenet/dense_{}/kernel', 'decoder/decoder_LSTM/multi_rnn_cell/cell_{0}/decoder_LSTM_{1}/bias'
    n_dec = 0
    while lstm.format(n_dec, n_dec + 1) in s:
        n_dec += 1
    n_pre = count(pre)
    try:
        M = s[pre.format(1)][0]
        loc = s['decoder/Location_Sensitive_Attention/location_features_convolution/kernel']
        return dict(n_symbols=s['inputs_embedding'][0], embedding_dim=s['inputs_embedding'][1], num_mels=M,
                    outputs_per_step=s['decoder/stop_token_projection/projection_stop_token_projection/bias'][0],
                    enc_conv_layers=count(enc), enc_conv_kernel=s[enc.format(1)][0], enc_conv_channels=s[enc.format(1)][2],
                    encoder_lstm_units=s['encoder_LSTM/bidirectional_rnn/fw/encoder_fw_LSTM/bias'][0] // 4,
                    attention_dim=s['memory_layer/kernel'][1], attention_kernel=loc[0], attention_filters=loc[2],
                    prenet_layers=tuple(s[pre.format(i + 1)][1] for i in range(n_pre)), decoder_layers=n_dec,
                    decoder_lstm_units=s[lstm.format(0, 1)][0] // 4, postnet_layers=count(post), postnet_kernel=s[post.format(1)][0],
                    postnet_channels=s[post.format(1)][2])
    except KeyError as e:
        raise _cabi.WrnnError(-4, f'tensor {e.args[0]} is missing from the checkpoint') from None


def checkpoint_step(path: str) -> str:
    """``tacotron_synthesize.py:192``: what follows the last ``-`` of the checkpoint's name (``tacotron_model.ckpt-150000`` -> ``150000``)."""
    import os
    return os.path.splitext(os.path.basename(path))[0].split('-')[-1].strip()


def synthesize_to_file(model: Tacotron, pinyin: str, symbols: Sequence[str], out_dir: str, step: str, seed: int = 0, max_iters: int = 2000,
                       gta_target=None, return_device: bool = False, stream_steps: Optional[int] = None):
    """``Synthesizer.synthesize`` of ``tacotron_synthesize.py``: writes ``step-{step}-{md5 of the text}-mel-pred.npy``, the (T, num_mels) mel
    in [0, 1] that ``wavernn_gen.py --file`` reads.  Returns (path, the call's result).  ``stream_steps``: decode through
    ``Tacotron.stream`` in pushes of that many steps (the same bytes)."""
    seq = text_to_sequence(pinyin.split(' '), symbols)
    if stream_steps is not None:
        with model.stream([seq], seeds=[seed], max_iters=max_iters, return_device=return_device,
                          gta_targets=None if gta_target is None else [gta_target]) as st:
            while not st.done:
                st.step(stream_steps)
            res = st.result()[0]
    else:
        res = model.synthesize([seq], seeds=[seed], max_iters=max_iters, gta_targets=None if gta_target is None else [gta_target],
                               return_device=return_device)[0]
    return write_mel_file(res['mel'], pinyin, out_dir, step), res


def write_mel_file(mel, pinyin: str, out_dir: str, step: str) -> str:
    """``step-{step}-{md5 of the text}-mel-pred.npy`` in ``out_dir``; ``mel``: numpy, or a torch tensor on any device."""
    import hashlib
    import os
    idx = hashlib.md5(pinyin.encode('utf-8')).hexdigest()
    os.makedirs(out_dir, exist_ok=True)
    path = os.path.join(out_dir, f'step-{step}-{idx}-mel-pred.npy')
    np.save(path, mel if isinstance(mel, np.ndarray) else mel.cpu().numpy(), allow_pickle=False)
    return path


def build_parser():
    import argparse
    p = argparse.ArgumentParser(description='Tacotron-2 on the device: pinyin -> the mel wavernn_gen.py vocodes')
    p.add_argument('--pinyin', required=True, help='space-separated pinyin tokens with tone digits and punctuation, as the reference\'s get_pyin returns them')
    p.add_argument('--symbols', required=True, metavar='FILE', help='the training list (the tokens after the last | of every line make the symbol table)')
    p.add_argument('--checkpoint', required=True, metavar='NPZ', help='the weights, keyed by the reference graph\'s variable names (INTEGRATION.md "From text")')
    p.add_argument('--gta', metavar='MEL.npy', default=None, help='teacher-force on this (T, num_mels) target in [-4, 4]: the GTA mel a WaveRNN is trained on')
    p.add_argument('--seed', type=int, default=0, help='keys the prenet dropout masks')
    p.add_argument('--max_iters', type=int, default=2000)
    p.add_argument('--out_dir', default='./tacotron_inference_output')
    p.add_argument('--stream-steps', dest='stream_steps', type=int, default=None, metavar='N',
                   help='decode in pushes of N steps (Tacotron.stream): the same mel; with --vocode the vocoder streams too and the time to the first audio is printed')
    p.add_argument('--vocode', metavar='WAVERNN.pyt', default=None, help='also vocode the mel with these WaveRNN weights (the mel stays on the device)')
    p.add_argument('--griffin_lim', type=int, nargs='?', const=60, default=None, metavar='N_ITER', help='also vocode the mel by Griffin-Lim (no model)')
    return p


def main(argv=None):
    import os
    import torch
    args = build_parser().parse_args(argv)
    if not torch.cuda.is_available():
        raise RuntimeError('Tacotron runs on an MI355X only (no CPU path)')
    symbols = load_symbols(args.symbols)
    with np.load(args.checkpoint, allow_pickle=False) as z:
        state = {k: z[k] for k in z.files}
    dims = dims_from_state(state)
    if dims['n_symbols'] != len(symbols):
        raise ValueError(f'{args.symbols} makes {len(symbols)} symbols, the checkpoint\'s embedding has {dims["n_symbols"]} rows')
    model = Tacotron(**dims).load_state(state)
    target = np.load(args.gta) if args.gta else None
    voc = hp = None
    if args.vocode:
        from .gen import build_model_from_hparams
        from .hparams import hparams as hp
        if not hp.is_configured():
            hp.configure()
        voc = build_model_from_hparams().to(torch.device('cuda', model.device))
        voc.load(args.vocode)
    step = checkpoint_step(args.checkpoint)
    both_stream = voc is not None and args.stream_steps is not None and target is None
    if both_stream:   # one Tacotron stream feeds the mel file and the vocoder's stream
        from .dsp import save_wav
        seq = text_to_sequence(args.pinyin.split(' '), symbols)
        audio, t_mel, t_audio, res = synthesize_stream_to_wav(model, voc, seq, None, chunk_steps=args.stream_steps, seed=args.seed,
                                                              max_iters=args.max_iters, mu_law=hp.mu_law, return_result=True)
        path = write_mel_file(res['mel'], args.pinyin, args.out_dir, step)
    else:
        path, res = synthesize_to_file(model, args.pinyin, symbols, args.out_dir, step, seed=args.seed, max_iters=args.max_iters,
                                       gta_target=target, return_device=True, stream_steps=args.stream_steps)
    print(f'{res["steps"]} decoder steps, {res["mel_length"]} mel frames -> {path}')
    mel = res['mel']
    stem = path[:-len('-mel-pred.npy')]
    if voc is not None:
        if both_stream:
            save_wav(audio, stem + '-wavernn.wav', voc.sample_rate)
            ms = lambda t: 'never' if t is None else f'after {1e3 * t:.1f} ms'
            print(f'first mel frames {ms(t_mel)}, first audio {ms(t_audio)}')
        else:
            voc.generate(mel.T[None].contiguous(), stem + '-wavernn.wav', False, hp.voc_target, hp.voc_overlap, hp.mu_law)
        print(stem + '-wavernn.wav')
    if args.griffin_lim is not None:
        from .dsp import save_wav
        from .frontend import GriffinLim
        gl = GriffinLim(features='tacotron', n_iter=int(args.griffin_lim), device=mel.device)
        out = gl.reconstruct(mel.T.contiguous(), seed=args.seed, device=mel.device)
        wav = out[0, :gl.last_samples[0]].cpu().numpy()
        peak = float(np.abs(wav).max()) if wav.size else 0.0
        if peak > 1.0:
            wav = wav * np.float32(0.999 / peak)
        save_wav(wav, stem + '-griffin_lim.wav', gl.sample_rate)
        print(stem + '-griffin_lim.wav')
    return path


if __name__ == '__main__':
    main()
