"""The mel front end on the device: wav -> the normalised mel spectrogram ``generate`` consumes.

``MelFrontEnd.melspectrogram`` is ``melspectrogram`` of ``wavernn/utils/dsp.py:72-81`` (``normalize(amp_to_db(mel_basis @ |stft(y)|))``,
librosa semantics of the reference's era) as one launch of the kernel in ``csrc/melspec.hip``; ``load_wav`` is ``dsp.py:18-19``, and with
``resample=True`` a file at another rate goes through ``Resampler`` (``csrc/resample.hip``), a Kaiser-windowed sinc on the device.
``WavConditioner`` (``csrc/condition.hip``) is the silence trimming and peak rescaling of ``tacotron/datasets/preprocessor.py:62-72``,
opt-in everywhere.  ``MelFrontEnd(features='tacotron')`` is the Tacotron-side mel of ``tacotron/datasets/audio.py`` (pre-emphasis fused
into the kernel's tap gather), the features the reference's vocoder is trained on.  ``GriffinLim`` (``csrc/griffin_lim.hip``) is the way back with no trained model:
``inv_mel_spectrogram`` of ``tacotron/datasets/audio.py:122-137`` in either profile.  ``SpectralScore`` (``csrc/score.hip``) rates a test clip
against its target: log-mel distance and mel-cepstral distortion over this front end's mel, spectral convergence and log-magnitude distance at
several STFT resolutions (the reference compares its ``*_target.wav`` files with nothing).  ``AlignedScore`` and ``dtw_path``
(``csrc/align.hip``) rate pairs that are not sample-aligned along the dynamic-time-warping path over their mel cepstra.  Linear ``spectrogram``
files and LWS are not here.
"""
from __future__ import annotations

import numpy as np
import torch

from . import _cabi

# wavernn_hparams.py:18-26; the names `hparams` carries once a file that sets them is configured
MEL_DEFAULTS = dict(sample_rate=22050, n_fft=2048, hop_length=275, win_length=1100, num_mels=80, fmin=95, min_level_db=-100)


# The feature profiles (``wrnn_mel_features``).  'vocoder': ``melspectrogram`` of ``wavernn/utils/dsp.py``, what this package has always
# made.  'tacotron': the mel the reference's WaveRNN is trained on and Tacotron hands it, ``tacotron/datasets/audio.py:95-102, 203-207,
# 250-295`` with ``tacotron_hparams.py``'s values, mapped to [0, 1] like ``wavernn_preprocess.py:149-159``.
FEATURE_PROFILES = {
    'vocoder': dict(pad_mode='reflect', magnitude_power=1, fmax=0.0, ref_level_db=0.0, preemphasis=0.0, preemph_rescale=0.0, max_abs_value=0.0),
    'tacotron': dict(pad_mode='zero', magnitude_power=2, fmax=7600.0, ref_level_db=20.0, preemphasis=0.97, preemph_rescale=0.999,
                     max_abs_value=4.0),
}
FEATURES_HELP = ("extension: the mel features of {what}: 'vocoder' (default) = melspectrogram of wavernn/utils/dsp.py; 'tacotron' = the mel "
                 "Tacotron's preprocessing makes and the reference's WaveRNN is trained on (pre-emphasis, zero padding, power spectrum, "
                 "fmax 7600, ref_level_db 20, [-4, 4] mapped to [0, 1]).  The reference's whole recipe: --features tacotron --trim_silence "
                 "--peak_norm")


def feature_settings(features='vocoder', **overrides) -> dict:
    """The profile ``features`` with ``overrides`` applied, checked: ``ValueError`` for an unknown profile name or ``pad_mode``,
    ``TypeError`` for an unknown field."""
    if features not in FEATURE_PROFILES:
        raise ValueError(f'features must be one of {sorted(FEATURE_PROFILES)}, got {features!r}')
    unknown = set(overrides) - set(FEATURE_PROFILES['vocoder'])
    if unknown:
        raise TypeError(f'unknown feature fields {sorted(unknown)}')
    out = dict(FEATURE_PROFILES[features], **overrides)
    if out['pad_mode'] not in _cabi.MEL_PAD_MODES:
        raise ValueError(f"pad_mode must be one of {sorted(_cabi.MEL_PAD_MODES)}, got {out['pad_mode']!r}")
    return out


def add_features_argument(parser, what='the wavs'):
    """``--features {vocoder,tacotron}`` for a command-line parser."""
    parser.add_argument('--features', choices=sorted(FEATURE_PROFILES), default='vocoder', help=FEATURES_HELP.format(what=what))


class MelFrontEnd:
    """``MelFrontEnd(hp)`` reads ``sample_rate, n_fft, hop_length, win_length, num_mels, fmin, min_level_db`` from an hparams-like object
    (a name it lacks takes the reference's default); keywords override (``n_mels`` is accepted for ``num_mels``).  ``ValueError`` for a
    configuration the library has no kernel for (``n_fft`` other than 2048) or refuses.

    ``features``: the feature profile, ``'vocoder'`` (default: what the class has always made) or ``'tacotron'`` (``FEATURE_PROFILES``);
    the keywords ``fmax, ref_level_db, preemphasis, preemph_rescale, magnitude_power, pad_mode, max_abs_value`` move single fields of it
    (``pad_mode``: ``'reflect'`` or ``'zero'``).  The profile's fields are not read from ``hp``.  ``self.features`` keeps the name,
    ``self.feature_config`` the fields."""

    def __init__(self, hp=None, device=None, features='vocoder', **kw):
        if 'n_mels' in kw:
            kw['num_mels'] = kw.pop('n_mels')
        self.feature_config = feature_settings(features, **{k: kw.pop(k) for k in list(kw) if k in FEATURE_PROFILES['vocoder']})
        self.features = features
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
            c, f = self.config, self.feature_config
            # the default profile goes through wrnn_mel_create itself, as before the profiles
            feat = None if f == FEATURE_PROFILES['vocoder'] else _cabi.MelFeatures(**dict(f, pad_mode=_cabi.MEL_PAD_MODES[f['pad_mode']]))
            self._nat[index] = _cabi.NativeMel(sample_rate=c['sample_rate'], n_fft=c['n_fft'], hop_length=c['hop_length'], win_length=c['win_length'],
                                               n_mels=c['num_mels'], fmin=c['fmin'], min_level_db=c['min_level_db'], device=index, features=feat)
        return self._nat[index]

    def frames(self, n_samples: int) -> int:
        """``1 + n // hop``; ``ValueError`` for a clip shorter than ``n_fft // 2 + 1`` samples (it cannot be reflect-padded); under
        ``pad_mode='zero'`` for an empty clip only."""
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
        return self.melspectrogram_padded(_padded_rows(clips, lens, dev), lens)

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


class GriffinLim:
    """``GriffinLim(hp, features='tacotron', power=1.5, n_iter=60)``: [0, 1] mels -> wavs on the device with no trained model, the
    reference's ``inv_mel_spectrogram`` (``tacotron/datasets/audio.py:122-137, 176-186``) on the kernels of ``csrc/griffin_lim.hip``:
    the profile's normalisation, dB and magnitude power undone, the pseudo-inverse of its filterbank, ``** power``, ``n_iter`` rounds of
    stft / istft that keep the magnitudes and take the wave's phases, and the de-emphasis with the profile's ``preemphasis``.  It is the
    inverse of ``MelFrontEnd(hp, features=features)`` and reads the same configuration (``hp``, the ``MEL_DEFAULTS`` names and the
    profile's fields as keywords); ``power`` and ``n_iter`` are arguments of this class only.  ``ValueError`` for a configuration the
    library refuses (``n_fft`` other than 2048, ``power <= 0``, a filterbank with an empty row)."""

    def __init__(self, hp=None, device=None, features='tacotron', power=1.5, n_iter=60, **kw):
        if 'n_mels' in kw:
            kw['num_mels'] = kw.pop('n_mels')
        self.feature_config = feature_settings(features, **{k: kw.pop(k) for k in list(kw) if k in FEATURE_PROFILES['vocoder']})
        self.features = features
        unknown = set(kw) - set(MEL_DEFAULTS)
        if unknown:
            raise TypeError(f'unknown Griffin-Lim parameters {sorted(unknown)}')
        self.config = {k: kw[k] if k in kw else getattr(hp, k, v) if hp is not None else v for k, v in MEL_DEFAULTS.items()}
        self.power, self.n_iter = float(power), int(n_iter)
        if self.n_iter < 0:
            raise ValueError(f'n_iter must be >= 0, got {n_iter!r}')
        self._device = device
        self._index = torch.device(device).index if device is not None and torch.device(device).index is not None else None
        self.n_mels, self.hop_length, self.sample_rate = int(self.config['num_mels']), int(self.config['hop_length']), int(self.config['sample_rate'])
        self.n_bins = int(self.config['n_fft']) // 2 + 1
        self._nat = {}
        self._native(self._index or 0, True)   # the configuration is checked here, without a device
        self.last_samples = self.last_seed = None

    def _native(self, index: int, deemphasis: bool) -> _cabi.NativeGriffinLim:
        """One handle per device and per de-emphasis switch: the library de-emphasises with the handle's ``preemphasis``."""
        key = (index, bool(deemphasis))
        if key not in self._nat:
            c, f = self.config, dict(self.feature_config)
            if not deemphasis:
                f['preemphasis'] = 0.0
            feat = _cabi.MelFeatures(**dict(f, pad_mode=_cabi.MEL_PAD_MODES[f['pad_mode']]))
            self._nat[key] = _cabi.NativeGriffinLim(sample_rate=c['sample_rate'], n_fft=c['n_fft'], hop_length=c['hop_length'],
                                                    win_length=c['win_length'], n_mels=c['num_mels'], fmin=c['fmin'],
                                                    min_level_db=c['min_level_db'], device=index, features=feat,
                                                    griffin=_cabi.GriffinConfig(self.power, self.n_iter))
        return self._nat[key]

    def samples(self, frames: int) -> int:
        """``hop_length * (frames - 1)``: the samples a mel of ``frames`` frames gives; ``ValueError`` for ``frames < 1``."""
        return next(iter(self._nat.values())).samples(frames)

    def tables(self, frames: int = 1) -> dict:
        """``pinv`` (n_fft/2 + 1, n_mels), ``window`` and the ``window_sumsquare`` of a clip of ``frames`` frames, as the kernels read them."""
        return next(iter(self._nat.values())).tables(frames)

    def reconstruct(self, mels, lens=None, *, n_iter=None, seed=None, phases=None, deemphasis=True, magnitude=False, device=None):
        """One ``(n_mels, T)`` mel, a list of them with different ``T``, or a ``(B, n_mels, T_max)`` batch with the clips' frame counts
        ``lens`` (the tensor ``MelFrontEnd.melspectrogram`` returns, with its ``last_frames``) -> ``(B, max samples)`` float32 tensor on
        the device, clip b in ``[b, :last_samples[b]]`` and zeros from there on; a row equals the call on that clip alone bit for bit.
        The first round's phases ``exp(2 pi i r)``: ``phases`` given: r injected, ``(B, T_max, n_fft/2 + 1)``; else ``seed`` given: r
        drawn on the device by the counter RNG, the same wav for the same seed; neither: a fresh seed from torch's generator
        (``self.last_seed`` keeps it).  ``phases='zero'``: r = 0.  ``deemphasis=False`` returns the pre-emphasised wave.
        ``magnitude=True``: returns ``(wav, S)`` with S ``(B, T_max, n_fft/2 + 1)``, the linear magnitudes the rounds aim at.  Nothing
        waits for the device."""
        dev = torch.device(device if device is not None else self._device if self._device is not None else 'cuda')
        if dev.type != 'cuda':
            raise ValueError(f'Griffin-Lim runs on the GPU only, got device {dev}')
        if isinstance(mels, torch.Tensor) and mels.is_cuda and device is None:
            dev = mels.device
        dev = torch.device('cuda', dev.index if dev.index is not None else torch.cuda.current_device())
        if isinstance(mels, (list, tuple)):
            clips = [torch.as_tensor(np.asarray(m) if not isinstance(m, torch.Tensor) else m) for m in mels]
        else:
            m = torch.as_tensor(np.asarray(mels) if not isinstance(mels, torch.Tensor) else mels)
            clips = [m] if m.dim() == 2 else None
        n_iter = self.n_iter if n_iter is None else int(n_iter)
        if n_iter < 0:
            raise ValueError(f'n_iter must be >= 0, got {n_iter}')
        with torch.cuda.device(dev):
            if clips is not None:
                if lens is not None:
                    raise ValueError('lens goes with a (B, n_mels, T_max) batch only')
                if not clips or any(c.dim() != 2 or c.shape[0] != self.n_mels or c.shape[1] < 1 for c in clips):
                    raise ValueError(f'expected mels shaped ({self.n_mels}, T >= 1)')
                frames = [int(c.shape[1]) for c in clips]
                if len(clips) == 1:
                    batch = clips[0].to(device=dev, dtype=torch.float32).contiguous().unsqueeze(0)
                else:
                    batch = torch.zeros((len(clips), self.n_mels, max(frames)), dtype=torch.float32, device=dev)
                    for i, c in enumerate(clips):
                        batch[i, :, :frames[i]] = c.to(device=dev, dtype=torch.float32)
            else:
                if m.dim() != 3 or m.shape[1] != self.n_mels or m.shape[2] < 1 or lens is None:
                    raise ValueError(f'expected one ({self.n_mels}, T) mel, a list of them, or a (B, {self.n_mels}, T_max) batch with lens')
                frames = [int(t) for t in lens]
                if len(frames) != m.shape[0] or min(frames) < 1 or max(frames) > m.shape[2]:
                    raise ValueError(f'{len(frames)} frame counts ({min(frames, default=0)} .. {max(frames, default=0)}) for a batch shaped {tuple(m.shape)}')
                batch = m.to(device=dev, dtype=torch.float32).contiguous()
            B, _, T_max = batch.shape
            nat = self._native(dev.index, deemphasis)
            n_out = max(1, nat.samples(T_max))
            if isinstance(phases, str):
                if phases != 'zero':
                    raise ValueError(f"phases must be an array, 'zero' or None, got {phases!r}")
                mode, r, seed_used = _cabi.GRIFFIN_PHASE_ZERO, None, 0
            elif phases is not None:
                r = torch.as_tensor(np.asarray(phases) if not isinstance(phases, torch.Tensor) else phases).to(device=dev, dtype=torch.float32).contiguous()
                if tuple(r.shape) != (B, T_max, self.n_bins):
                    raise ValueError(f'phases: expected shape {(B, T_max, self.n_bins)}, got {tuple(r.shape)}')
                mode, seed_used = _cabi.GRIFFIN_PHASE_INJECTED, 0
            else:
                seed_used = int(torch.randint(0, 2 ** 62, (1,)).item()) if seed is None else int(seed)
                mode, r = _cabi.GRIFFIN_PHASE_PHILOX, None
                self.last_seed = seed_used
            frames_dev = torch.tensor(frames, dtype=torch.int32).to(dev)
            out = torch.empty((B, n_out), dtype=torch.float32, device=dev)
            S = torch.empty((B, T_max, self.n_bins), dtype=torch.float32, device=dev) if magnitude else None
            nat.griffin_lim(batch.data_ptr(), frames_dev.data_ptr(), B, T_max, n_iter, mode, seed_used, r.data_ptr() if r is not None else 0,
                            out.data_ptr(), n_out, S.data_ptr() if S is not None else 0, torch.cuda.current_stream(dev).cuda_stream)
        self.last_samples = [nat.samples(t) for t in frames]
        return (out, S) if magnitude else out


def deemphasis(wav: torch.Tensor, lens, k: float) -> torch.Tensor:
    """``inv_preemphasis`` on the device (``wrnn_deemphasis``): ``wav`` a contiguous float32 ``(B, n_max)`` tensor on the GPU with clip b
    in ``wav[b, :lens[b]]`` -> ``out[b, i] = wav[b, i] + k out[b, i-1]``, zeros past each clip's own length."""
    if not (isinstance(wav, torch.Tensor) and wav.is_cuda and wav.dtype == torch.float32 and wav.dim() == 2 and wav.is_contiguous()):
        raise ValueError('expected a contiguous float32 (B, n_max) tensor on the GPU')
    lens = [int(n) for n in lens]
    B, n_max = wav.shape
    if len(lens) != B or not lens or max(lens) > n_max or min(lens) < 0 or n_max < 1:
        raise ValueError(f'{len(lens)} lengths ({min(lens, default=0)} .. {max(lens, default=0)}) for a buffer of shape {tuple(wav.shape)}')
    with torch.cuda.device(wav.device):
        n_dev = torch.tensor(lens, dtype=torch.int32).to(wav.device)
        out = torch.empty_like(wav)
        _cabi.deemphasis(wav.data_ptr(), n_max, n_dev.data_ptr(), B, float(k), out.data_ptr(), torch.cuda.current_stream(wav.device).cuda_stream)
    return out


def _padded_rows(clips, lens, dev) -> torch.Tensor:
    """Clips of different lengths, on the host or the device -> one zero-padded float32 ``(B, max(lens))`` tensor on ``dev``: a single clip
    as it is, device clips copied on the device, host clips through one padded host buffer and one upload."""
    n_max, B = max(lens), len(clips)
    with torch.cuda.device(dev):
        if B == 1:
            return torch.as_tensor(clips[0]).to(device=dev, dtype=torch.float32).contiguous().view(1, -1)
        if all(isinstance(c, torch.Tensor) and c.is_cuda for c in clips):
            wav = torch.zeros((B, n_max), dtype=torch.float32, device=dev)
            for i, c in enumerate(clips):
                wav[i, :lens[i]] = c
            return wav
        host = np.zeros((B, n_max), np.float32)
        for i, c in enumerate(clips):
            host[i, :lens[i]] = c.detach().cpu().numpy() if isinstance(c, torch.Tensor) else np.asarray(c)
        return torch.from_numpy(host).to(dev)


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
    a bank of more than 2**24 entries).  Resampled peaks may exceed the input's: a full-scale clip can leave [-1, 1]; ``peak_norm``
    (``WavConditioner``, applied after the resampler) brings it back."""

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
        return self.resample_padded(_padded_rows(clips, lens, dev), lens)

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


RESCALING_MAX = 0.999   # tacotron_hparams.py:69 rescaling_max, what peak_norm=True scales the peak to
TRIM_TOP_DB, TRIM_FRAME_LENGTH, TRIM_HOP_LENGTH = 25.0, 2048, 512   # tacotron_hparams.py:91-93


def condition_settings(trim_top_db=None, peak_norm=None):
    """The two conditioning switches as the library takes them: ``(trim_top_db or None, peak target or None)``.  ``trim_top_db``: ``None``
    (off) or a finite number of dB above 0.  ``peak_norm``: ``None`` / ``False`` (off), ``True`` (0.999, the reference's
    ``rescaling_max``) or a finite target above 0.  ``ValueError`` for anything else."""
    if trim_top_db is not None:
        if isinstance(trim_top_db, bool) or not isinstance(trim_top_db, (int, float, np.integer, np.floating)):
            raise ValueError(f'trim_top_db must be None or a number of dB, got {trim_top_db!r}')
        trim_top_db = float(trim_top_db)
        if not (np.isfinite(trim_top_db) and trim_top_db > 0):
            raise ValueError(f'trim_top_db must be finite and above 0, got {trim_top_db!r}')
    if peak_norm is None or peak_norm is False:
        target = None
    elif peak_norm is True:
        target = RESCALING_MAX
    elif isinstance(peak_norm, (int, float, np.integer, np.floating)):
        target = float(peak_norm)
        if not (np.isfinite(target) and 0 < target <= float(np.finfo(np.float32).max)):
            raise ValueError(f'peak_norm must be True or a finite float32 target above 0, got {peak_norm!r}')
    else:
        raise ValueError(f'peak_norm must be None, a bool or a target, got {peak_norm!r}')
    return trim_top_db, target


def add_condition_arguments(parser, what='the wavs'):
    """``--trim_silence``, ``--trim_top_db DB`` and ``--peak_norm [TARGET]`` for a command-line parser (``condition_arguments`` reads them)."""
    parser.add_argument('--trim_silence', action='store_true',
                        help=f'extension: trim leading and trailing silence of {what} on the device, like librosa.effects.trim with a '
                             f'{TRIM_FRAME_LENGTH} / {TRIM_HOP_LENGTH} window (default: off)')
    parser.add_argument('--trim_top_db', type=float, default=TRIM_TOP_DB, metavar='DB',
                        help='with --trim_silence: frames more than DB below the loudest frame are silence (default: %(default)s)')
    parser.add_argument('--peak_norm', type=float, nargs='?', const=RESCALING_MAX, default=None, metavar='TARGET',
                        help=f'extension: rescale {what} to a peak of TARGET on the device, after trimming (TARGET left out: '
                             f'{RESCALING_MAX}; default: off)')


def condition_arguments(args) -> dict:
    """The ``trim_top_db=`` / ``peak_norm=`` keywords for the flags of ``add_condition_arguments`` (checked: ``ValueError``)."""
    trim_top_db, target = condition_settings(args.trim_top_db if args.trim_silence else None, args.peak_norm)
    return dict(trim_top_db=trim_top_db, peak_norm=target)


class WavConditioner:
    """``WavConditioner(trim_top_db=25, peak_norm=True)``: the two steps the reference applies to every training wav between loading it
    and the mel (``tacotron/datasets/preprocessor.py:62-72``), on the device (``csrc/condition.hip``), for a whole ragged list at once.

    ``trim_top_db``: trim leading and trailing silence like ``librosa.effects.trim(wav, top_db, frame_length, hop_length)[0]``: frames
    of the reflect-padded clip whose mean square lies more than ``top_db`` dB below the loudest frame's are silent, and the clip is cut
    to ``[first_non_silent * hop, min(n, (last_non_silent + 1) * hop))``.  Energies and the decision are float64 (librosa's are
    float32); digital silence is kept whole.  ``peak_norm``: then ``wav / abs(wav).max() * target`` in float32 (``True``: 0.999); an
    all-zero clip is left as it is.  At least one of the two must be on; both are off by default everywhere else in the package, and
    nothing reads ``hp.peak_norm`` (``wavernn_hparams.py:29`` declares it, the reference reads it nowhere).  A clip needs
    ``frame_length // 2 + 1`` samples to be trimmed."""

    def __init__(self, trim_top_db=None, peak_norm=None, frame_length=TRIM_FRAME_LENGTH, hop_length=TRIM_HOP_LENGTH, device=None):
        self.trim_top_db, self.peak_target = condition_settings(trim_top_db, peak_norm)
        if self.trim_top_db is None and self.peak_target is None:
            raise ValueError('a WavConditioner with neither trim_top_db nor peak_norm has nothing to do')
        self.frame_length, self.hop_length = int(frame_length), int(hop_length)
        _cabi.condition_frames(2 ** 20, self.frame_length, self.hop_length)   # the window is checked here, without a device
        self._device = device
        self.last_lens = self.last_bounds = self.last_peaks = None

    def frames(self, n: int) -> int:
        """``1 + n // hop_length`` energy frames; ``ValueError`` for a clip shorter than ``frame_length // 2 + 1`` samples."""
        return _cabi.condition_frames(int(n), self.frame_length, self.hop_length)

    def condition(self, wavs, device=None) -> torch.Tensor:
        """One 1-D array / tensor, or a list of them of different lengths, on the host or the device -> ``(B, n_max)`` float32 tensor on
        the device, conditioned clip b in ``[b, :last_lens[b]]`` and zeros from there on.  A row equals the call on that clip alone bit
        for bit.  Sets ``last_lens``, ``last_bounds`` (``(B, 2)`` start and end in the input clip) and ``last_peaks`` (``max |x|`` over
        the kept span, before scaling); reading them is the one host wait of the call."""
        clips, lens = _clip_list(wavs)
        if min(lens) < 1:
            raise ValueError('expected clips of at least one sample')
        dev = torch.device(device if device is not None else self._device if self._device is not None else 'cuda')
        if dev.type != 'cuda':
            raise ValueError(f'the conditioning runs on the GPU only, got device {dev}')
        if self.trim_top_db is not None:
            for n in lens:
                self.frames(n)   # refuses a short clip before anything is launched
        dev = torch.device('cuda', dev.index if dev.index is not None else torch.cuda.current_device())
        wav = _padded_rows(clips, lens, dev)
        with torch.cuda.device(dev):
            bounds = torch.empty((len(clips), 2), dtype=torch.int32, device=dev)
            peaks = torch.empty(len(clips), dtype=torch.float32, device=dev)
        out, n_out = self.condition_padded(wav, lens, bounds=bounds, peaks=peaks)
        self.last_lens = [int(n) for n in n_out.cpu().numpy()]
        self.last_bounds, self.last_peaks = bounds.cpu().numpy(), peaks.cpu().numpy()
        return out

    __call__ = condition

    def condition_padded(self, wav: torch.Tensor, lens, bounds=None, peaks=None, energies=None):
        """The launches behind :meth:`condition` for clips that already lie on the device: ``wav`` a contiguous float32 ``(B, n_max)``
        tensor with clip b in ``wav[b, :lens[b]]`` (what lies past a clip is never read); ``lens`` a list, or an int32 ``(B,)`` device
        tensor such as the one this method returns.  Returns ``(out, n_out)``: ``out`` ``(B, n_max)`` float32, zero past each clip's own
        new length, the buffer ``MelFrontEnd.melspectrogram_padded`` and ``wrnn_quantise`` read, and ``n_out`` the int32 ``(B,)`` device
        tensor of the new lengths.  Nothing waits for the device.  ``bounds`` (int32 ``(B, 2)``), ``peaks`` (float32 ``(B,)``) and
        ``energies`` (float64 ``(B, frames(n_max))``, the frame energies; trimming only) are optional device tensors to fill.  Lengths
        given as a list are checked here; device lengths are the caller's to keep at ``frame_length // 2 + 1`` or more."""
        if not (isinstance(wav, torch.Tensor) and wav.is_cuda and wav.dtype == torch.float32 and wav.dim() == 2 and wav.is_contiguous()):
            raise ValueError('expected a contiguous float32 (B, n_max) tensor on the GPU')
        B, n_max = wav.shape
        dev = wav.device
        trim = self.trim_top_db is not None
        if isinstance(lens, torch.Tensor) and lens.is_cuda:
            if not (lens.dtype == torch.int32 and lens.dim() == 1 and lens.shape[0] == B and lens.is_contiguous() and lens.device == dev):
                raise ValueError(f'expected {B} int32 lengths on {dev}')
            n_dev = lens
        else:
            lens = [int(n) for n in lens]
            if len(lens) != B or not lens or max(lens) > n_max or min(lens) < 1:
                raise ValueError(f'{len(lens)} lengths ({min(lens, default=0)} .. {max(lens, default=0)}) for a buffer of shape {tuple(wav.shape)}')
            if trim:
                for n in lens:
                    self.frames(n)
            n_dev = None
        if B < 1 or n_max < 1:
            raise ValueError(f'an empty buffer of shape {tuple(wav.shape)}')
        F_max = 1 + n_max // self.hop_length
        if energies is not None and not trim:
            raise ValueError('frame energies are computed for trimming only')
        for name, t, dtype, shape in (('bounds', bounds, torch.int32, (B, 2)), ('peaks', peaks, torch.float32, (B,)),
                                      ('energies', energies, torch.float64, (B, F_max))):
            if t is not None and not (isinstance(t, torch.Tensor) and t.device == dev and t.dtype == dtype and tuple(t.shape) == shape
                                      and t.is_contiguous()):
                raise ValueError(f'{name}: expected a contiguous {dtype} tensor of shape {shape} on {dev}')
        with torch.cuda.device(dev):
            if n_dev is None:
                n_dev = torch.tensor(lens, dtype=torch.int32).to(dev)
            ws = torch.empty(B * F_max + B, dtype=torch.float64, device=dev)
            out = torch.empty((B, n_max), dtype=torch.float32, device=dev)
            n_out = torch.empty(B, dtype=torch.int32, device=dev)
            _cabi.condition(wav.data_ptr(), n_max, n_dev.data_ptr(), B, trim, self.trim_top_db if trim else TRIM_TOP_DB, self.frame_length,
                            self.hop_length, self.peak_target or 0.0, ws.data_ptr(), F_max, out.data_ptr(), n_max, n_out.data_ptr(),
                            bounds.data_ptr() if bounds is not None else 0, peaks.data_ptr() if peaks is not None else 0,
                            torch.cuda.current_stream(dev).cuda_stream)
            if energies is not None:
                energies.copy_(ws[:B * F_max].view(B, F_max))
        return out, n_out


class SpectralScore:
    """``SpectralScore(hp, features='vocoder', resolutions=..., mcd_order=13, mag_floor=1e-7)``: how far test clips are from their
    targets, on the device (``csrc/score.hip``): the per-frame log-mel distance and mel-cepstral distortion over the mel of
    ``MelFrontEnd(hp, features=features)`` (the same configuration: ``hp``, the ``MEL_DEFAULTS`` names and the profile's fields as
    keywords), and spectral convergence and log-magnitude distance at every ``(n_fft, hop, win)`` of ``resolutions`` (at most four,
    ``n_fft`` one of 256, 512, 1024, 2048).  The definitions are in ``include/wavernn_amd.h``.  No time alignment: the clips are compared
    sample for sample.  ``ValueError`` for a configuration the library refuses, without a device."""

    def __init__(self, hp=None, device=None, features='vocoder', resolutions=_cabi.SCORE_DEFAULT_RESOLUTIONS, mcd_order=13, mag_floor=1e-7, **kw):
        if 'n_mels' in kw:
            kw['num_mels'] = kw.pop('n_mels')
        self.feature_config = feature_settings(features, **{k: kw.pop(k) for k in list(kw) if k in FEATURE_PROFILES['vocoder']})
        self.features = features
        unknown = set(kw) - set(MEL_DEFAULTS)
        if unknown:
            raise TypeError(f'unknown score parameters {sorted(unknown)}')
        self.config = {k: kw[k] if k in kw else getattr(hp, k, v) if hp is not None else v for k, v in MEL_DEFAULTS.items()}
        self.mcd_order, self.mag_floor = int(mcd_order), float(mag_floor)
        self._score_config = _cabi.ScoreConfig(resolutions, self.mag_floor, self.mcd_order)   # ValueError: malformed or too many resolutions
        self._device = device
        self._index = torch.device(device).index if device is not None and torch.device(device).index is not None else None
        self.n_mels, self.hop_length, self.sample_rate = int(self.config['num_mels']), int(self.config['hop_length']), int(self.config['sample_rate'])
        self._nat = {}
        nat = self._native(self._index or 0)   # the configuration is checked here, without a device
        self.resolutions, self.min_samples = nat.resolutions, nat.min_samples

    def _native(self, index: int) -> _cabi.NativeScore:
        if index not in self._nat:
            c, f = self.config, self.feature_config
            feat = None if f == FEATURE_PROFILES['vocoder'] else _cabi.MelFeatures(**dict(f, pad_mode=_cabi.MEL_PAD_MODES[f['pad_mode']]))
            self._nat[index] = _cabi.NativeScore(sample_rate=c['sample_rate'], n_fft=c['n_fft'], hop_length=c['hop_length'], win_length=c['win_length'],
                                                 n_mels=c['num_mels'], fmin=c['fmin'], min_level_db=c['min_level_db'], device=index, features=feat,
                                                 score=self._score_config)
        return self._nat[index]

    def frames(self, r: int, n: int) -> int:
        """The frames of a clip of ``n`` samples at resolution ``r`` (``-1``: the mel); ``ValueError`` for a clip shorter than ``min_samples``."""
        return next(iter(self._nat.values())).frames(r, n)

    def tables(self) -> dict:
        """``windows``, ``twiddles`` (per resolution) and ``dct`` (mcd_order, n_mels) as the kernels read them."""
        return next(iter(self._nat.values())).tables()

    def score(self, targets, tests, device=None, per_frame=False):
        """``targets`` and ``tests``: what ``MelFrontEnd.melspectrogram`` accepts (one 1-D array / tensor, a 2-D one, or a list of clips of
        different lengths, on the host or the device), pair by pair; every pair is cut to its shorter clip.  One library call for the
        whole list.  Returns a list of dicts, one per pair: ``mel_lsd_db``, ``mcd_db``, ``mr_sc``, ``mr_logmag``, ``stft`` (a list of
        ``{n_fft, hop, win, sc, logmag, frames}``) and ``n``; with ``per_frame=True`` also ``lsd``, ``mcd`` (float32 arrays over the mel's
        frames) and ``num``, ``den``, ``lm`` in every entry of ``stft``.  ``ValueError`` before any device work for a pair shorter than
        ``min_samples``.  Reading the results back is the one host wait."""
        (ca, la), (cb, lb) = _clip_list(targets), _clip_list(tests)
        if len(ca) != len(cb):
            raise ValueError(f'{len(ca)} targets for {len(cb)} tests')
        lens = [min(a, b) for a, b in zip(la, lb)]
        for n in lens:
            self.frames(-1, n)                 # refuses a short pair before anything is launched
        dev = torch.device(device if device is not None else self._device if self._device is not None else 'cuda')
        if dev.type != 'cuda':
            raise ValueError(f'the scores run on the GPU only, got device {dev}')
        dev = torch.device('cuda', dev.index if dev.index is not None else torch.cuda.current_device())
        B, n_max = len(lens), max(lens)
        wa = _padded_rows([c[:n] for c, n in zip(ca, lens)], lens, dev)
        wb = _padded_rows([c[:n] for c, n in zip(cb, lens)], lens, dev)
        nat = self._native(dev.index)
        segs, stride = nat.layout(n_max)
        with torch.cuda.device(dev):
            n_dev = torch.tensor(lens, dtype=torch.int32).to(dev)
            summary = torch.empty((B, _cabi.SCORE_FIELDS), dtype=torch.float64, device=dev)
            frames = torch.empty((B, stride), dtype=torch.float32, device=dev) if per_frame else None
            nat.score(wa.data_ptr(), wb.data_ptr(), n_max, n_dev.data_ptr(), B, summary.data_ptr(), frames.data_ptr() if per_frame else 0,
                      stride, torch.cuda.current_stream(dev).cuda_stream)
            summary = summary.cpu().numpy()
            frames = frames.cpu().numpy() if per_frame else None
        # the raw per-frame rows as the library wrote them (zeros past a clip's own frames) and their segments (name, r, offset, frames)
        self.last_frames_buffer, self.last_layout = frames, segs
        out = []
        for b, n in enumerate(lens):
            s = dict(zip(_cabi.SCORE_FIELD_NAMES, (float(v) for v in summary[b])))
            d = dict(n=n, mel_lsd_db=s['mel_lsd_db'], mcd_db=s['mcd_db'], mr_sc=s['mr_sc'], mr_logmag=s['mr_logmag'], stft=[])
            for r, (n_fft, hop, win) in enumerate(self.resolutions):
                d['stft'].append(dict(n_fft=n_fft, hop=hop, win=win, sc=s[f'sc{r}'], logmag=s[f'logmag{r}'], frames=nat.frames(r, n)))
            if per_frame:
                for name, r, off, _ in segs:
                    t = nat.frames(r, n)
                    (d if r < 0 else d['stft'][r])[name] = frames[b, off:off + t].copy()
            out.append(d)
        return out


class _PitchBase:
    """The settings and the per-device handles ``PitchTracker`` and ``PitchScore`` share."""

    def __init__(self, hp=None, device=None, **settings):
        unknown = set(settings) - set(_cabi.PITCH_DEFAULTS)
        if unknown:
            raise TypeError(f'unknown pitch settings {sorted(unknown)}')
        s = dict(_cabi.PITCH_DEFAULTS)
        if hp is not None:
            s['sample_rate'], s['hop'] = getattr(hp, 'sample_rate', s['sample_rate']), getattr(hp, 'hop_length', s['hop'])
        s.update(settings)
        self.settings = s
        self.sample_rate, self.hop, self.frame_length, self.window = (int(s[k]) for k in ('sample_rate', 'hop', 'frame_length', 'window'))
        self._device = device
        self._index = torch.device(device).index if device is not None and torch.device(device).index is not None else None
        self._nat = {}
        nat = self._native(self._index or 0)   # the configuration is checked here, without a device
        self.tau_min, self.tau_max = nat.tau_min, nat.tau_max

    def _native(self, index: int) -> _cabi.NativePitch:
        if index not in self._nat:
            self._nat[index] = _cabi.NativePitch(_cabi.PitchConfig(device=index, **self.settings))
        return self._nat[index]

    def frames(self, n: int) -> int:
        """The frames of a clip of ``n`` samples: ``1 + n // hop``, and none of an empty clip."""
        return next(iter(self._nat.values())).frames(n)

    def _cuda(self, device, what):
        dev = torch.device(device if device is not None else self._device if self._device is not None else 'cuda')
        if dev.type != 'cuda':
            raise ValueError(f'{what} on the GPU only, got device {dev}')
        return torch.device('cuda', dev.index if dev.index is not None else torch.cuda.current_device())


class PitchTracker(_PitchBase):
    """``PitchTracker(hp, frame_length=2048, window=1024, fmin=60, fmax=600, threshold=0.15, silence_rms=1e-4)``: the YIN F0 track of
    clips on the device (``csrc/pitch.hip``; the definitions are in ``include/wavernn_amd.h``), one frame per ``hop`` samples, lined up
    with the mel's frames.  ``sample_rate`` and ``hop`` come from ``hp`` unless given.  ``ValueError`` for a configuration the library
    refuses, without a device."""

    def track(self, wavs, device=None):
        """``wavs``: what ``MelFrontEnd.melspectrogram`` accepts (one 1-D array / tensor, a 2-D one, or a list of clips of different
        lengths, on the host or the device).  One library call for the whole list.  Returns a list of ``(f0, aperiodicity)`` float32
        arrays over each clip's own ``frames(n)`` frames; ``f0`` is 0 on unvoiced frames."""
        clips, lens = _clip_list(wavs)
        T = [self.frames(n) for n in lens]
        dev = self._cuda(device, 'the pitch tracker runs')
        B, n_max = len(lens), max(max(lens), 1)
        wav = _padded_rows(clips, lens, dev) if max(lens) > 0 else torch.zeros((B, 1), dtype=torch.float32, device=dev)
        nat = self._native(dev.index)
        stride = nat.frames(n_max)
        with torch.cuda.device(dev):
            n_dev = torch.tensor(lens, dtype=torch.int32).to(dev)
            out = torch.empty((2, B, stride), dtype=torch.float32, device=dev)
            nat.track(wav.data_ptr(), n_max, n_dev.data_ptr(), B, out[0].data_ptr(), out[1].data_ptr(), stride,
                      torch.cuda.current_stream(dev).cuda_stream)
            out = out.cpu().numpy()
        self.last_buffer = out     # the raw rows as the library wrote them (zeros past a clip's own frames)
        return [(out[0, b, :t].copy(), out[1, b, :t].copy()) for b, t in enumerate(T)]


class PitchScore(_PitchBase):
    """``PitchScore(hp, gpe_ratio=0.2, ...)``: the F0 and voicing errors of test clips against their targets, on the device, over the
    tracks of ``PitchTracker`` with the same settings: ``f0_rmse_cents``, ``gpe`` (gross pitch error), ``vde`` (voicing decision
    error), ``ffe`` (F0 frame error), ``f0_corr`` and the voiced frame counts.  No time alignment: the clips are compared frame for frame."""

    def score(self, targets, tests, device=None, per_frame=False):
        """``targets`` and ``tests`` as ``SpectralScore.score`` takes them, pair by pair; every pair is cut to its shorter clip.  One
        library call for the whole list.  Returns a list of dicts, one per pair: the names of ``_cabi.PITCH_FIELD_NAMES`` (the three
        counts as ints), ``n`` and ``frames``; with ``per_frame=True`` also ``f0_target``, ``aperiodicity_target``, ``f0_test``,
        ``aperiodicity_test`` and ``cents`` (float32 arrays over the pair's frames).  Reading the results back is the one host wait."""
        (ca, la), (cb, lb) = _clip_list(targets), _clip_list(tests)
        if len(ca) != len(cb):
            raise ValueError(f'{len(ca)} targets for {len(cb)} tests')
        lens = [min(a, b) for a, b in zip(la, lb)]
        T = [self.frames(n) for n in lens]
        dev = self._cuda(device, 'the scores run')
        B, n_max = len(lens), max(max(lens), 1)
        if max(lens) > 0:
            wa = _padded_rows([c[:n] for c, n in zip(ca, lens)], lens, dev)
            wb = _padded_rows([c[:n] for c, n in zip(cb, lens)], lens, dev)
        else:
            wa = wb = torch.zeros((B, 1), dtype=torch.float32, device=dev)
        nat = self._native(dev.index)
        F = nat.frames(n_max)
        with torch.cuda.device(dev):
            n_dev = torch.tensor(lens, dtype=torch.int32).to(dev)
            summary = torch.empty((B, _cabi.PITCH_FIELDS), dtype=torch.float64, device=dev)
            frames = torch.empty((B, 5 * F), dtype=torch.float32, device=dev) if per_frame else None
            nat.score(wa.data_ptr(), wb.data_ptr(), n_max, n_dev.data_ptr(), B, summary.data_ptr(), frames.data_ptr() if per_frame else 0,
                      5 * F, torch.cuda.current_stream(dev).cuda_stream)
            summary = summary.cpu().numpy()
            frames = frames.cpu().numpy() if per_frame else None
        self.last_frames_buffer = frames
        out = []
        for b, n in enumerate(lens):
            d = dict(zip(_cabi.PITCH_FIELD_NAMES, (float(v) for v in summary[b])))
            for k in _cabi.PITCH_FIELD_NAMES[5:]:
                d[k] = int(d[k])
            d.update(n=n, frames=T[b])
            if per_frame:
                for i, name in enumerate(_cabi.PITCH_FRAME_NAMES):
                    d[name] = frames[b, i * F:i * F + T[b]].copy()
            out.append(d)
        return out


def _ragged_rows(clips, lens, n_max, dev) -> torch.Tensor:
    """``_padded_rows`` for a buffer that may be wider than the longest clip (a side whose clips are all empty still needs a legal row)."""
    if max(lens) == n_max:
        return _padded_rows(clips, lens, dev)
    with torch.cuda.device(dev):
        wav = torch.zeros((len(clips), n_max), dtype=torch.float32, device=dev)
        for i, c in enumerate(clips):
            if lens[i]:
                wav[i, :lens[i]] = torch.as_tensor(c).to(device=dev, dtype=torch.float32)
    return wav


class AlignedScore:
    """``AlignedScore(hp, features='vocoder', mcd_order=13, pitch=False, gpe_ratio=0.2, **pitch_settings)``: test clips rated against
    their targets along the dynamic-time-warping path over their mel cepstra, on the device (``csrc/align.hip``; the definitions are in
    ``include/wavernn_amd.h``): for pairs that are not sample-aligned -- a trimmed clip, a rendering of a predicted mel against the
    recording, two takes of a sentence -- where ``SpectralScore`` and ``PitchScore`` (frame t against frame t) mean nothing.  The mel is
    ``MelFrontEnd(hp, features=features)``'s (the same configuration: ``hp``, the ``MEL_DEFAULTS`` names and the profile's fields as
    keywords).  With ``pitch=True`` both clips also go through ``PitchTracker(hp, **pitch_settings)`` at the mel's hop and the F0 /
    voicing errors are taken along the path; the tracker's settings go by their own names (``frame_length, window, threshold,
    silence_rms``) or, where the mel has one of that name, with a prefix (``pitch_fmin, pitch_fmax``).  The clips of a pair may differ in length; batches are ragged; a clip of no samples has no
    frames and an all-zero row.  ``ValueError`` for a configuration the library refuses, without a device."""

    def __init__(self, hp=None, device=None, features='vocoder', mcd_order=13, pitch=False, gpe_ratio=0.2, **kw):
        if 'n_mels' in kw:
            kw['num_mels'] = kw.pop('n_mels')
        self.feature_config = feature_settings(features, **{k: kw.pop(k) for k in list(kw) if k in FEATURE_PROFILES['vocoder']})
        self.features = features
        # the tracker's settings under their own names, or with a `pitch_` prefix where the mel has a setting of that name (fmin, fmax)
        pitch_kw = {k[6:]: kw.pop(k) for k in list(kw) if k.startswith('pitch_') and k[6:] in _cabi.PITCH_DEFAULTS}
        pitch_kw.update({k: kw.pop(k) for k in list(kw) if k in _cabi.PITCH_DEFAULTS and k not in MEL_DEFAULTS and k != 'gpe_ratio'})
        unknown = set(kw) - set(MEL_DEFAULTS)
        if unknown:
            raise TypeError(f'unknown alignment parameters {sorted(unknown)}')
        if pitch_kw and not pitch:
            raise TypeError(f'the pitch settings {sorted(pitch_kw)} belong to pitch=True')
        self.config = {k: kw[k] if k in kw else getattr(hp, k, v) if hp is not None else v for k, v in MEL_DEFAULTS.items()}
        self.mcd_order, self.gpe_ratio = int(mcd_order), float(gpe_ratio)
        self._align_config = _cabi.AlignConfig(self.mcd_order, self.gpe_ratio)
        self._device = device
        self._index = torch.device(device).index if device is not None and torch.device(device).index is not None else None
        self.n_mels, self.hop_length, self.sample_rate = int(self.config['num_mels']), int(self.config['hop_length']), int(self.config['sample_rate'])
        self._nat = {}
        self.min_samples = self._native(self._index or 0).min_samples   # the configuration is checked here, without a device
        self.pitch = PitchTracker(device=device, **dict(dict(sample_rate=self.sample_rate, hop=self.hop_length), **pitch_kw)) if pitch else None

    def _native(self, index: int) -> _cabi.NativeAlign:
        if index not in self._nat:
            c, f = self.config, self.feature_config
            feat = None if f == FEATURE_PROFILES['vocoder'] else _cabi.MelFeatures(**dict(f, pad_mode=_cabi.MEL_PAD_MODES[f['pad_mode']]))
            self._nat[index] = _cabi.NativeAlign(sample_rate=c['sample_rate'], n_fft=c['n_fft'], hop_length=c['hop_length'], win_length=c['win_length'],
                                                 n_mels=c['num_mels'], fmin=c['fmin'], min_level_db=c['min_level_db'], device=index, features=feat,
                                                 align=self._align_config)
        return self._nat[index]

    def frames(self, n: int) -> int:
        """The frames of a clip of ``n`` samples, ``1 + n // hop_length``; ``ValueError`` for a clip shorter than ``min_samples``."""
        return next(iter(self._nat.values())).frames(n)

    def _stage(self, targets, tests, device):
        """The two sides as padded device rows: (dev, native handle, B, (wav, n_max, lens, n_dev, frames) per side)."""
        (ca, la), (cb, lb) = _clip_list(targets), _clip_list(tests)
        if len(ca) != len(cb):
            raise ValueError(f'{len(ca)} targets for {len(cb)} tests')
        T = [[self.frames(n) if n else 0 for n in lens] for lens in (la, lb)]   # refuses a short clip before anything is launched; an empty one has no frames
        dev = torch.device(device if device is not None else self._device if self._device is not None else 'cuda')
        if dev.type != 'cuda':
            raise ValueError(f'the alignment runs on the GPU only, got device {dev}')
        dev = torch.device('cuda', dev.index if dev.index is not None else torch.cuda.current_device())
        nat = self._native(dev.index)
        sides = []
        for clips, lens, frames in ((ca, la, T[0]), (cb, lb, T[1])):
            n_max = max(max(lens), self.min_samples)
            wav = _ragged_rows(clips, lens, n_max, dev)
            with torch.cuda.device(dev):
                n_dev = torch.tensor(lens, dtype=torch.int32).to(dev)
            sides.append((wav, n_max, lens, n_dev, frames))
        nat.workspace_bytes(len(ca), sides[0][1], sides[1][1])   # the library's limits, as a WrnnError before any launch
        return dev, nat, len(ca), sides

    def cost(self, targets, tests, device=None):
        """``targets`` and ``tests``: what ``MelFrontEnd.melspectrogram`` accepts, pair by pair.  A list of ``(Ta, Tb)`` float32 device
        tensors, one per pair: ``d(i, j)`` in dB between frame ``i`` of the target and frame ``j`` of the test."""
        dev, nat, B, ((wa, na_max, _, na_dev, Ta), (wb, nb_max, _, nb_dev, Tb)) = self._stage(targets, tests, device)
        with torch.cuda.device(dev):
            out = torch.empty((B, nat.frames(na_max), nat.frames(nb_max)), dtype=torch.float32, device=dev)
            nat.cost(wa.data_ptr(), na_max, na_dev.data_ptr(), wb.data_ptr(), nb_max, nb_dev.data_ptr(), B, out.data_ptr(),
                     torch.cuda.current_stream(dev).cuda_stream)
        return [out[b, :Ta[b], :Tb[b]] for b in range(B)]

    def align(self, targets, tests, device=None):
        """The DTW paths: a list of ``(P, 2)`` int32 tensors of ``(i_p, j_p)`` in ascending order, one per pair."""
        return self.score(targets, tests, device=device, per_path=True)['path']

    def score(self, targets, tests, device=None, per_path=False):
        """One library call for the whole list (plus the two pitch tracks under ``pitch=True``).  Returns a dict of float64 tensors of
        shape ``(B,)`` under the names of ``_cabi.ALIGN_FIELD_NAMES`` (``total_cost, path_len, frames_target, frames_test, mcd_dtw_db,
        mel_lsd_dtw_db, f0_rmse_cents, gpe, vde, ffe, f0_corr, voiced_both``; the pitch fields are 0 without ``pitch=True``); with
        ``per_path=True`` also ``path`` (a list of ``(P, 2)`` int32 tensors), ``lsd`` and ``cents`` (lists of ``(P,)`` float64 tensors:
        the log-mel distance of every path pair, and ``1200 log2(fs / ft)`` where both sides are voiced, 0 elsewhere) and, under
        ``pitch=True``, ``f0_target`` and ``f0_test`` (the tracks, float32).  Everything comes back on the host: reading the results
        is the one wait."""
        dev, nat, B, ((wa, na_max, la, na_dev, Ta), (wb, nb_max, lb, nb_dev, Tb)) = self._stage(targets, tests, device)
        Ta_max, Tb_max = nat.frames(na_max), nat.frames(nb_max)
        P_max, stride = Ta_max + Tb_max - 1, max(Ta_max, Tb_max)
        with torch.cuda.device(dev):
            stream = torch.cuda.current_stream(dev).cuda_stream
            f0 = None
            if self.pitch is not None:
                f0 = torch.empty((2, B, stride), dtype=torch.float32, device=dev)
                pn = self.pitch._native(dev.index)
                pn.track(wa.data_ptr(), na_max, na_dev.data_ptr(), B, f0[0].data_ptr(), 0, stride, stream)
                pn.track(wb.data_ptr(), nb_max, nb_dev.data_ptr(), B, f0[1].data_ptr(), 0, stride, stream)
            summary = torch.empty((B, _cabi.ALIGN_FIELDS), dtype=torch.float64, device=dev)
            path = torch.empty((B, P_max, 2), dtype=torch.int32, device=dev) if per_path else None
            plen = torch.empty((B,), dtype=torch.int32, device=dev) if per_path else None
            pp = torch.empty((B, 2, P_max), dtype=torch.float64, device=dev) if per_path else None
            nat.score(wa.data_ptr(), na_max, na_dev.data_ptr(), wb.data_ptr(), nb_max, nb_dev.data_ptr(), B, f0[0].data_ptr() if f0 is not None else 0,
                      f0[1].data_ptr() if f0 is not None else 0, stride, summary.data_ptr(), path.data_ptr() if per_path else 0,
                      plen.data_ptr() if per_path else 0, pp.data_ptr() if per_path else 0, stream)
            summary = summary.cpu()
            out = {name: summary[:, i].clone() for i, name in enumerate(_cabi.ALIGN_FIELD_NAMES)}
            if per_path:
                path, plen, pp = path.cpu(), plen.cpu().tolist(), pp.cpu()
                self.last_path_buffer = path       # the raw rows as the library wrote them (-1 past a pair's own path)
                out['path'] = [path[b, :plen[b]].clone() for b in range(B)]
                for i, name in enumerate(_cabi.ALIGN_PATH_NAMES):
                    out[name] = [pp[b, i, :plen[b]].clone() for b in range(B)]
                if f0 is not None:
                    f0 = f0.cpu()
                    out['f0_target'] = [f0[0, b, :Ta[b]].clone() for b in range(B)]
                    out['f0_test'] = [f0[1, b, :Tb[b]].clone() for b in range(B)]
        out['n_target'], out['n_test'] = list(la), list(lb)
        return out


_DTW_HANDLES = {}


def dtw_path(cost, lens_a=None, lens_b=None):
    """The generic entry (``wrnn_align_path``): dynamic time warping over ANY cost matrices, a float32 CUDA tensor ``(B, Ta, Tb)`` or
    ``(Ta, Tb)``; ``lens_a`` / ``lens_b``: the pairs' own frame counts (default: the whole matrix).  The symmetric step pattern with
    unit weights, ties to the diagonal first, then ``(i - 1, j)``.  Returns ``(paths, totals)``: a list of ``(P, 2)`` int32 device
    tensors in ascending order and a ``(B,)`` float64 device tensor of ``D(Ta - 1, Tb - 1)``.  Reading the path lengths is the one wait."""
    if not (isinstance(cost, torch.Tensor) and cost.is_cuda and cost.dtype == torch.float32 and cost.dim() in (2, 3)):
        raise ValueError('expected a float32 (B, Ta, Tb) or (Ta, Tb) tensor on the GPU')
    c = (cost if cost.dim() == 3 else cost.unsqueeze(0)).contiguous()
    B, Ta, Tb = c.shape
    la = [Ta] * B if lens_a is None else [int(v) for v in lens_a]
    lb = [Tb] * B if lens_b is None else [int(v) for v in lens_b]
    if len(la) != B or len(lb) != B or min(la + lb) < 0 or max(la) > Ta or max(lb) > Tb:
        raise ValueError(f'{len(la)} and {len(lb)} lengths (max {max(la)}, {max(lb)}) for cost matrices of shape {tuple(c.shape)}')
    dev = c.device
    if dev.index not in _DTW_HANDLES:
        _DTW_HANDLES[dev.index] = _cabi.NativeAlign(device=dev.index)
    nat = _DTW_HANDLES[dev.index]
    with torch.cuda.device(dev):
        ta, tb = torch.tensor(la, dtype=torch.int32).to(dev), torch.tensor(lb, dtype=torch.int32).to(dev)
        path = torch.empty((B, Ta + Tb - 1, 2), dtype=torch.int32, device=dev)
        plen = torch.empty((B,), dtype=torch.int32, device=dev)
        total = torch.empty((B,), dtype=torch.float64, device=dev)
        nat.path(c.data_ptr(), B, Ta, Tb, ta.data_ptr(), tb.data_ptr(), path.data_ptr(), plen.data_ptr(), total.data_ptr(),
                 torch.cuda.current_stream(dev).cuda_stream)
        P = plen.cpu().tolist()
    dtw_path.last_path_buffer = path
    return [path[b, :P[b]] for b in range(B)], total


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


def load_wav(path, sample_rate, resample=False, device=None, trim_top_db=None, peak_norm=None, features='vocoder'):
    """``librosa.load(path, sr=sample_rate)[0]`` (``dsp.py:18-19``): float32 mono (``read_wav``).  A file at another rate raises
    ``ValueError`` unless ``resample=True``: then it is resampled on the device (``Resampler``) and comes back as a host array of
    ``ceil(n sample_rate / rate)`` samples.  ``trim_top_db`` / ``peak_norm`` (both off by default): the clip is then conditioned on the
    device after the resampler (``WavConditioner``) and the trimmed, rescaled clip comes back.  ``features`` is checked and changes
    nothing here: under every profile the clip that comes back is the vocoder's target, never pre-emphasised (the ``'tacotron'``
    profile pre-emphasises inside the mel kernel)."""
    from scipy.io import wavfile
    feature_settings(features)
    trim_top_db, target = condition_settings(trim_top_db, peak_norm)
    sr, data = wavfile.read(str(path))
    if int(sr) != int(sample_rate) and not resample:
        raise ValueError(f'{path} is sampled at {int(sr)} Hz, the model needs {int(sample_rate)} Hz: resample the file first, or pass '
                         f'resample=True (--resample) for the resampler on the device')
    y = _decode(path, data)
    conditioned = trim_top_db is not None or target is not None
    if int(sr) == int(sample_rate) and not conditioned:
        return y
    if y.shape[0] < 1:
        raise ValueError(f'{path} holds no samples')
    if int(sr) != int(sample_rate):
        rs = Resampler(int(sr), sample_rate, device=device)
        y = rs.resample(y, device=device)
        y = y[0, :rs.last_lens[0]]
    if conditioned:
        cond = WavConditioner(trim_top_db, target, device=device)
        y = cond.condition(y, device=device)
        y = y[0, :cond.last_lens[0]]
    return np.ascontiguousarray(y.cpu().numpy())
