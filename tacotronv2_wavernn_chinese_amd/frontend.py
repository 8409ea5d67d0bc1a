"""The mel front end on the device: wav -> the normalised mel spectrogram ``generate`` consumes.

``MelFrontEnd.melspectrogram`` is ``melspectrogram`` of ``wavernn/utils/dsp.py:72-81`` (``normalize(amp_to_db(mel_basis @ |stft(y)|))``,
librosa semantics of the reference's era) as one launch of the kernel in ``csrc/melspec.hip``; ``load_wav`` is ``dsp.py:18-19``, and with
``resample=True`` a file at another rate goes through ``Resampler`` (``csrc/resample.hip``), a Kaiser-windowed sinc on the device.
Pre-emphasis, ``spectrogram``, Griffin-Lim and the Tacotron-side recipe of ``tacotron/datasets/audio.py`` are not here.
"""
from __future__ import annotations

import numpy as np
import torch

from . import _cabi

# wavernn_hparams.py:18-26; the names `hparams` carries once a file that sets them is configured
MEL_DEFAULTS = dict(sample_rate=22050, n_fft=2048, hop_length=275, win_length=1100, num_mels=80, fmin=95, min_level_db=-100)


class MelFrontEnd:
    """``MelFrontEnd(hp)`` reads ``sample_rate, n_fft, hop_length, win_length, num_mels, fmin, min_level_db`` from an hparams-like object
    (a name it lacks takes the reference's default); keywords override (``n_mels`` is accepted for ``num_mels``).  ``ValueError`` for a
    configuration the library has no kernel for (``n_fft`` other than 2048) or refuses."""

    def __init__(self, hp=None, device=None, **kw):
        if 'n_mels' in kw:
            kw['num_mels'] = kw.pop('n_mels')
        unknown = set(kw) - set(MEL_DEFAULTS)
        if unknown:
            raise TypeError(f'unknown front-end parameters {sorted(unknown)}')
        cfg = {k: kw[k] if k in kw else getattr(hp, k, v) if hp is not None else v for k, v in MEL_DEFAULTS.items()}
        self.config = cfg
        self._device = device
        self._index = torch.device(device).index if device is not None and torch.device(device).index is not None else None
        self.n_mels, self.hop_length, self.sample_rate = int(cfg['num_mels']), int(cfg['hop_length']), int(cfg['sample_rate'])
        self._nat = {}
        self._native(self._index or 0)   # the configuration is checked here, without a device

    def _native(self, index: int) -> _cabi.NativeMel:
        if index not in self._nat:
            c = self.config
            self._nat[index] = _cabi.NativeMel(sample_rate=c['sample_rate'], n_fft=c['n_fft'], hop_length=c['hop_length'], win_length=c['win_length'],
                                               n_mels=c['num_mels'], fmin=c['fmin'], min_level_db=c['min_level_db'], device=index)
        return self._nat[index]

    def frames(self, n_samples: int) -> int:
        """``1 + n // hop``; ``ValueError`` for a clip shorter than ``n_fft // 2 + 1`` samples (it cannot be reflect-padded)."""
        return next(iter(self._nat.values())).frames(n_samples)

    def tables(self) -> dict:
        return next(iter(self._nat.values())).tables()

    def melspectrogram(self, wavs, device=None) -> torch.Tensor:
        """One 1-D array / tensor, or a list of them of different lengths -> ``(B, n_mels, T_max)`` float32 tensor on the device, ``T_b = 1 +
        n_b // hop`` frames per clip and zeros from there to ``T_max`` (the zero conditioning ``generate_many`` pads with).  One launch for
        the whole list; a row equals the call on that clip alone bit for bit.  Clips already on the device stay there.  ``ValueError``
        before any device work for a clip too short to pad.  ``self.last_frames`` keeps the clips' frame counts."""
        if isinstance(wavs, (list, tuple)):
            clips = list(wavs)
        else:
            shape = wavs.shape if hasattr(wavs, 'shape') else np.shape(wavs)
            clips = [wavs] if len(shape) == 1 else list(wavs)
        if not clips:
            raise ValueError('expected at least one clip')
        lens = []
        for c in clips:
            shape = tuple(c.shape) if hasattr(c, 'shape') else np.shape(c)
            if len(shape) != 1:
                raise ValueError(f'expected 1-D clips of samples, got shape {shape}')
            lens.append(int(shape[0]))
        frames = [self.frames(n) for n in lens]   # refuses a short clip before anything is launched
        dev = torch.device(device if device is not None else self._device if self._device is not None else 'cuda')
        if dev.type != 'cuda':
            raise ValueError(f'the front end runs on the GPU only, got device {dev}')
        index = dev.index if dev.index is not None else torch.cuda.current_device()
        dev = torch.device('cuda', index)
        n_max, B = max(lens), len(clips)
        with torch.cuda.device(dev):
            if B == 1:
                wav = torch.as_tensor(clips[0]).to(device=dev, dtype=torch.float32).contiguous().view(1, -1)
            elif all(isinstance(c, torch.Tensor) and c.is_cuda for c in clips):
                wav = torch.zeros((B, n_max), dtype=torch.float32, device=dev)
                for i, c in enumerate(clips):
                    wav[i, :lens[i]] = c
            else:
                host = np.zeros((B, n_max), np.float32)
                for i, c in enumerate(clips):
                    host[i, :lens[i]] = c.detach().cpu().numpy() if isinstance(c, torch.Tensor) else np.asarray(c)
                wav = torch.from_numpy(host).to(dev)
        return self.melspectrogram_padded(wav, lens)

    def melspectrogram_padded(self, wav: torch.Tensor, lens) -> torch.Tensor:
        """The launch behind :meth:`melspectrogram` for clips that already lie on the device: ``wav`` a contiguous float32 ``(B, n_max)`` tensor
        with clip b in ``wav[b, :lens[b]]`` -> ``(B, n_mels, T_max)``.  The caller keeps ``wav`` (``DeviceCorpus`` quantises the same buffer)."""
        if not (isinstance(wav, torch.Tensor) and wav.is_cuda and wav.dtype == torch.float32 and wav.dim() == 2 and wav.is_contiguous()):
            raise ValueError('expected a contiguous float32 (B, n_max) tensor on the GPU')
        lens = [int(n) for n in lens]
        B, n_max = wav.shape
        if len(lens) != B or not lens or max(lens) > n_max:
            raise ValueError(f'{len(lens)} lengths (max {max(lens, default=0)}) for a buffer of shape {tuple(wav.shape)}')
        frames = [self.frames(n) for n in lens]   # refuses a short clip before anything is launched
        dev, t_max = wav.device, max(frames)
        with torch.cuda.device(dev):
            n_dev = torch.tensor(lens, dtype=torch.int32).to(dev)
            out = torch.empty((B, self.n_mels, t_max), dtype=torch.float32, device=dev)
            self._native(dev.index).melspectrogram(wav.data_ptr(), n_max, n_dev.data_ptr(), B, t_max, out.data_ptr(),
                                                   torch.cuda.current_stream(dev).cuda_stream)
        self.last_frames = frames
        return out


def _clip_list(wavs):
    """One 1-D array / tensor, a 2-D one (its rows), or a list of 1-D ones -> (list of clips, their lengths)."""
    if isinstance(wavs, (list, tuple)):
        clips = list(wavs)
    else:
        shape = wavs.shape if hasattr(wavs, 'shape') else np.shape(wavs)
        clips = [wavs] if len(shape) == 1 else list(wavs)
    if not clips:
        raise ValueError('expected at least one clip')
    lens = []
    for c in clips:
        shape = tuple(c.shape) if hasattr(c, 'shape') else np.shape(c)
        if len(shape) != 1:
            raise ValueError(f'expected 1-D clips of samples, got shape {shape}')
        lens.append(int(shape[0]))
    return clips, lens


class Resampler:
    """``Resampler(src_rate, dst_rate)``: clips at ``src_rate`` -> clips at ``dst_rate`` on the device, one launch of the kernel in
    ``csrc/resample.hip`` for a whole ragged list.  The filter is a Kaiser-windowed sinc with 64 zero crossings (the ``kaiser_best``
    parameters, those of the reference's default resampler as far as we can tell), evaluated exactly at every tap position of the reduced
    ratio ``p / q``; a clip of ``n`` samples gives ``ceil(n p / q)`` (librosa 0.7.2 computes ``int(n ratio)`` samples and pads to the
    ceiling: at most the last sample differs).  Bit parity with librosa / resampy is not claimed.  Equal rates launch nothing and return
    the input object as it is (the filter is a low-pass).  ``ValueError`` for rates the library refuses (a rate <= 0, ``dst / src < 1/32``,
    a bank of more than 2**24 entries).  Resampled peaks may exceed the input's: a full-scale clip can leave [-1, 1]."""

    def __init__(self, src_rate, dst_rate, device=None):
        self.src_rate, self.dst_rate = int(src_rate), int(dst_rate)
        self._device = device
        self._index = torch.device(device).index if device is not None and torch.device(device).index is not None else None
        self._nat = {}
        nat = self._native(self._index or 0)   # the rates are checked here, without a device
        self.p, self.q, self.taps = nat.p, nat.q, nat.taps
        self.last_lens = None

    def _native(self, index: int) -> _cabi.NativeResampler:
        if index not in self._nat:
            self._nat[index] = _cabi.NativeResampler(self.src_rate, self.dst_rate, device=index)
        return self._nat[index]

    def out_len(self, n: int) -> int:
        """``ceil(n p / q)``, the length of a clip of ``n`` samples after resampling (``n`` itself at equal rates)."""
        return next(iter(self._nat.values())).out_len(n)

    def bank(self) -> np.ndarray:
        """The ``(p, taps)`` float32 filter bank the kernel reads."""
        return next(iter(self._nat.values())).bank()

    def resample(self, wavs, device=None):
        """One 1-D array / tensor, or a list of them of different lengths, on the host or the device -> ``(B, n_out_max)`` float32 tensor on
        the device, clip b in ``[b, :last_lens[b]]`` and zeros from there on.  One launch for the whole list; a row equals the call on that
        clip alone bit for bit.  Clips already on the device stay there."""
        if self.src_rate == self.dst_rate:
            return wavs
        clips, lens = _clip_list(wavs)
        if min(lens) < 1:
            raise ValueError('expected clips of at least one sample')
        dev = torch.device(device if device is not None else self._device if self._device is not None else 'cuda')
        if dev.type != 'cuda':
            raise ValueError(f'the resampler runs on the GPU only, got device {dev}')
        dev = torch.device('cuda', dev.index if dev.index is not None else torch.cuda.current_device())
        n_max, B = max(lens), len(clips)
        with torch.cuda.device(dev):
            if B == 1:
                wav = torch.as_tensor(clips[0]).to(device=dev, dtype=torch.float32).contiguous().view(1, -1)
            elif all(isinstance(c, torch.Tensor) and c.is_cuda for c in clips):
                wav = torch.zeros((B, n_max), dtype=torch.float32, device=dev)
                for i, c in enumerate(clips):
                    wav[i, :lens[i]] = c
            else:
                host = np.zeros((B, n_max), np.float32)
                for i, c in enumerate(clips):
                    host[i, :lens[i]] = c.detach().cpu().numpy() if isinstance(c, torch.Tensor) else np.asarray(c)
                wav = torch.from_numpy(host).to(dev)
        return self.resample_padded(wav, lens)

    __call__ = resample

    def resample_padded(self, wav: torch.Tensor, lens) -> torch.Tensor:
        """The launch behind :meth:`resample` for clips that already lie on the device: ``wav`` a contiguous float32 ``(B, n_in_max)`` tensor
        with clip b in ``wav[b, :lens[b]]`` (what lies past a clip is never read) -> ``(B, max out_len)``, zero past each clip's own
        ``out_len``: the buffer ``MelFrontEnd.melspectrogram_padded`` and ``wrnn_quantise`` read.  ``self.last_lens`` keeps the lengths."""
        if not (isinstance(wav, torch.Tensor) and wav.is_cuda and wav.dtype == torch.float32 and wav.dim() == 2 and wav.is_contiguous()):
            raise ValueError('expected a contiguous float32 (B, n_in_max) tensor on the GPU')
        lens = [int(n) for n in lens]
        B, n_max = wav.shape
        if len(lens) != B or not lens or max(lens) > n_max or min(lens) < 1:
            raise ValueError(f'{len(lens)} lengths ({min(lens, default=0)} .. {max(lens, default=0)}) for a buffer of shape {tuple(wav.shape)}')
        if self.src_rate == self.dst_rate:
            self.last_lens = lens
            return wav
        out_lens = [self.out_len(n) for n in lens]
        dev = wav.device
        with torch.cuda.device(dev):
            n_dev = torch.tensor(lens, dtype=torch.int32).to(dev)
            out = torch.empty((B, max(out_lens)), dtype=torch.float32, device=dev)
            self._native(dev.index).resample(wav.data_ptr(), n_max, n_dev.data_ptr(), B, out.shape[1], out.data_ptr(),
                                             torch.cuda.current_stream(dev).cuda_stream)
        self.last_lens = out_lens
        return out


def _decode(path, data) -> np.ndarray:
    if data.dtype == np.int16:
        y = data.astype(np.float32) / np.float32(32768.0)
    elif data.dtype == np.int32:
        y = (data.astype(np.float64) / 2147483648.0).astype(np.float32)
    elif data.dtype == np.uint8:
        y = (data.astype(np.float32) - np.float32(128.0)) / np.float32(128.0)
    elif data.dtype.kind == 'f':
        y = data.astype(np.float32)
    else:
        raise ValueError(f'{path}: unsupported sample format {data.dtype}')
    if y.ndim == 2:
        y = y.mean(axis=1, dtype=np.float32)
    return np.ascontiguousarray(y, dtype=np.float32)


def read_wav(path):
    """A wav file -> ``(float32 mono samples, its sample rate)``.  int16 / int32 / uint8 PCM is scaled to [-1, 1), float data is taken as
    it is, channels are averaged (``mono=True``)."""
    from scipy.io import wavfile
    sr, data = wavfile.read(str(path))
    return _decode(path, data), int(sr)


def load_wav(path, sample_rate, resample=False, device=None):
    """``librosa.load(path, sr=sample_rate)[0]`` (``dsp.py:18-19``): float32 mono (``read_wav``).  A file at another rate raises
    ``ValueError`` unless ``resample=True``: then it is resampled on the device (``Resampler``) and comes back as a host array of
    ``ceil(n sample_rate / rate)`` samples."""
    from scipy.io import wavfile
    sr, data = wavfile.read(str(path))
    if int(sr) != int(sample_rate) and not resample:
        raise ValueError(f'{path} is sampled at {int(sr)} Hz, the model needs {int(sample_rate)} Hz: resample the file first, or pass '
                         f'resample=True (--resample) for the resampler on the device')
    y = _decode(path, data)
    if int(sr) == int(sample_rate):
        return y
    if y.shape[0] < 1:
        raise ValueError(f'{path} holds no samples')
    rs = Resampler(int(sr), sample_rate, device=device)
    out = rs.resample(y)
    return np.ascontiguousarray(out[0, :rs.last_lens[0]].cpu().numpy())
