"""The training data on the device: a folder of wavs -> a corpus resident in HBM -> ``(x, y, mels)`` window batches.

What the reference spreads over ``wavernn_preprocess.py`` (quantise the wav, write ``quant/*.npy``, ``mel/*.npy`` and the list file),
``get_vocoder_datasets`` and ``collate_vocoder`` (``wavernn/utils/dataset.py:62-133``).  Here the mel comes from the device front end
(``csrc/melspec.hip``), the labels from ``wrnn_quantise`` and every batch from one ``wrnn_collate_windows`` launch over a corpus that
stays where the trainer is (``csrc/dataset.hip``): ten hours of 22.05 kHz audio are about 4 GB of int32 labels and 80-band mels.

``DeviceCorpus`` keeps two device allocations -- all labels back to back, and all mels back to back with every utterance
frames-major, ``(frames, n_mels)``, the layout of the reference's mel files, so that a training window is one contiguous run -- and
the per-utterance offset tables, on the host and on the device.  ``DeviceWindowLoader`` is ``train.WindowLoader`` over such a corpus:
the same draws from the same generator (``train.draw_window_offsets``), hence the same batches bit for bit, already on the device.
"""
from __future__ import annotations

import random
from pathlib import Path
from typing import List, Optional, Sequence, Tuple, Union

import numpy as np
import torch

from . import _cabi
from .train import draw_window_offsets

LIST_NAME = 'wavernn_training_data.txt'
FEATURES_NAME = 'wavernn_training_features.txt'   # next to the list file: the feature profile of the saved mels, one word
GTA_NAME = 'wavernn_training_gta.txt'             # next to the list file of a GTA corpus: the checkpoint's name and the seed base


def saved_features(list_file: Union[str, Path]) -> str:
    """The feature profile ``DeviceCorpus.save`` recorded next to ``list_file``; ``'vocoder'`` where nothing is recorded (a corpus saved
    before the profiles, or the reference's own files)."""
    note = Path(list_file).expanduser().parent / FEATURES_NAME
    return note.read_text(encoding='utf-8').strip() if note.is_file() else 'vocoder'


def check_saved_features(list_file: Union[str, Path], features: str) -> None:
    """``ValueError`` when the corpus saved at ``list_file`` holds other features than the requested ones."""
    have = saved_features(list_file)
    if have != features:
        raise ValueError(f'{list_file} holds {have!r} mel features, {features!r} were asked for: a vocoder trained on one kind cannot be '
                         f'driven with the other.  Pass --features {have}, or preprocess the wavs again with --features {features}')


def signal_bits(hp) -> Tuple[int, bool]:
    """(bits, mu_law) of the training labels for an hparams-like object: MOL trains on a 16-bit linear signal (dataset.py:126), RAW
    on ``hp.bits`` classes, mu-law when ``hp.mu_law`` says so."""
    if getattr(hp, 'voc_mode', 'RAW') == 'MOL':
        return 16, False
    return int(hp.bits), bool(getattr(hp, 'mu_law', True))


def min_frames(*, hop_length: int, pad: int, seq_len: int) -> int:
    """Utterances with fewer mel frames are dropped by ``get_vocoder_datasets`` (dataset.py:73-75)."""
    return seq_len // hop_length + 2 * pad + 2 * pad + 2


def _device(device) -> torch.device:
    dev = torch.device(device if device is not None else 'cuda')
    if dev.type != 'cuda':
        raise ValueError(f'a DeviceCorpus lives on the GPU, got device {dev}')
    return torch.device('cuda', dev.index if dev.index is not None else torch.cuda.current_device())


class _GtaMade:
    """``corpus.gta`` of a GTA corpus: equal to ``True`` and true, where every other corpus has the method ``gta``.  Calling it is a
    ``ValueError`` that says so (``gta_made`` is the plain flag every corpus has)."""

    def __eq__(self, other):
        return other is True or isinstance(other, _GtaMade)

    def __hash__(self):
        return hash(True)

    def __bool__(self):
        return True

    def __repr__(self):
        return 'True'

    def __call__(self, *args, **kw):
        raise ValueError('this corpus already holds GTA mels (gta_made): teacher-force the corpus it was made from, whose mels it keeps as '
                         'source_mels, not this one')


class DeviceCorpus:
    """Utterances as ``labels`` (int32, all utterances back to back) and ``mels`` (float32, utterance u as ``(frames[u], n_mels)``
    from element ``mel_off[u]``) on one device.  ``label_off / label_len / mel_off / frames`` are host arrays with one entry per
    utterance; ``stems`` names the utterances (file names of ``save``).  Make one with ``from_wavs``, ``from_pairs`` or ``load``."""

    def __init__(self, labels: torch.Tensor, mels: torch.Tensor, label_off, label_len, mel_off, frames, n_mels: int, stems: Sequence[str],
                 *, hop_length: int, sample_rate: Optional[int] = None, bits: Optional[int] = None, mu_law: Optional[bool] = None,
                 n_clipped: int = 0, trim_top_db: Optional[float] = None, peak_norm: Optional[float] = None, features: str = 'vocoder',
                 source_mels: Optional[torch.Tensor] = None, gta: bool = False, gta_note: Optional[dict] = None):
        self.labels, self.mels = labels, mels
        # a GTA corpus (``gta()``): ``mels`` are the Tacotron's teacher-forced predictions, ``source_mels`` the ground truth they were made
        # from, a table of the same offsets; ``gta_note`` is what ``save`` writes about their making
        self.source_mels, self.gta_made, self.gta_note = source_mels, bool(gta), dict(gta_note or {})
        if self.gta_made:
            self.gta = _GtaMade()   # on a GTA corpus the name is the flag, == True; called, it says why there is no second pass
        if source_mels is not None and source_mels.numel() != mels.numel():
            raise ValueError('source_mels and mels are tables of one layout: they differ in size')
        self.features = features   # the feature profile of the mels (frontend.FEATURE_PROFILES)
        self.trim_top_db, self.peak_norm = trim_top_db, peak_norm   # how from_wavs conditioned the clips (None: it did not)
        self.label_off, self.label_len = np.asarray(label_off, np.int64), np.asarray(label_len, np.int64)
        self.mel_off, self.frames = np.asarray(mel_off, np.int64), np.asarray(frames, np.int32)
        self.n_mels, self.stems, self.hop_length = int(n_mels), list(stems), int(hop_length)
        self.sample_rate, self.bits, self.mu_law, self.n_clipped = sample_rate, bits, mu_law, int(n_clipped)
        if not (len(self.label_off) == len(self.label_len) == len(self.mel_off) == len(self.frames) == len(self.stems)):
            raise ValueError('the offset tables and the names differ in length')
        # what wrnn_collate_windows relies on: every window the collate can draw lies inside the utterance's own labels and mel
        short = np.flatnonzero(self.label_len < (self.frames.astype(np.int64) - 1) * self.hop_length)
        if short.size:
            u = int(short[0])
            raise ValueError(f'utterance {self.stems[u]!r}: {int(self.label_len[u])} labels for {int(self.frames[u])} frames of hop '
                             f'{self.hop_length}, at least {(int(self.frames[u]) - 1) * self.hop_length} are needed')
        if len(self) and (int((self.label_off + self.label_len).max()) > labels.numel()
                          or int((self.mel_off + self.frames.astype(np.int64) * self.n_mels).max()) > mels.numel()
                          or int(self.label_off.min()) < 0 or int(self.mel_off.min()) < 0):
            raise ValueError('an offset table points outside the device buffers')
        self._tables = None

    # ------------------------------------------------------------------ what the loader and the callers read
    def __len__(self):
        return len(self.frames)

    @property
    def device(self) -> torch.device:
        return self.labels.device

    @property
    def hours(self) -> float:
        return float(self.label_len.sum()) / float(self.sample_rate or 22050) / 3600.0

    def device_tables(self):
        """(label_off int64, mel_off int64, frames int32) on the device, uploaded once."""
        if self._tables is None:
            dev = self.device
            self._tables = (torch.from_numpy(self.label_off).to(dev), torch.from_numpy(self.mel_off).to(dev), torch.from_numpy(self.frames).to(dev))
        return self._tables

    def pairs(self) -> List[Tuple[np.ndarray, np.ndarray]]:
        """Host ``(mel (n_mels, frames), labels)`` arrays, one pair per utterance: what ``train.WindowLoader`` takes."""
        out = []
        for lo, ln, mo, t in zip(self.label_off, self.label_len, self.mel_off, self.frames):
            mel = self.mels[int(mo):int(mo) + int(t) * self.n_mels].cpu().numpy().reshape(int(t), self.n_mels)
            out.append((mel.T, self.labels[int(lo):int(lo) + int(ln)].cpu().numpy()))
        return out

    def _meta(self) -> dict:
        return dict(hop_length=self.hop_length, sample_rate=self.sample_rate, bits=self.bits, mu_law=self.mu_law, n_clipped=self.n_clipped,
                    trim_top_db=self.trim_top_db, peak_norm=self.peak_norm, features=self.features)

    def subset(self, ids: Sequence[int]) -> 'DeviceCorpus':
        """The utterances ``ids`` as a corpus of their own that shares the device buffers (nothing is copied); of a GTA corpus, a GTA
        corpus."""
        ids = np.asarray(list(ids), np.int64)
        return DeviceCorpus(self.labels, self.mels, self.label_off[ids], self.label_len[ids], self.mel_off[ids], self.frames[ids], self.n_mels,
                            [self.stems[i] for i in ids], source_mels=self.source_mels, gta=self.gta_made, gta_note=self.gta_note, **self._meta())

    def split(self, test_samples: int) -> Tuple['DeviceCorpus', 'DeviceCorpus']:
        """(train, test) the way ``read_feature_list`` / ``get_vocoder_datasets`` (dataset.py:79-85) split: ids shuffled with seed
        1234, the last ``test_samples`` set aside."""
        ids = list(range(len(self)))
        random.Random(1234).shuffle(ids)
        if test_samples:
            return self.subset(ids[:-test_samples]), self.subset(ids[-test_samples:])
        return self.subset(ids), self.subset([])

    # ------------------------------------------------------------------ the Tacotron's own mels
    def gta(self, model, sequences, *, seeds=None, seed_base: int = 0, batch_utts: int = 64, prenet_dropout: bool = True):
        """``(corpus, report)``: this corpus with every mel replaced by the one ``model`` (a ``tacotron.Tacotron``) predicts when its
        decoder is fed the utterance's own frames -- the GTA mels the reference's ``wavernn_preprocess.py`` trains its vocoder on.
        ``sequences[u]`` is the symbol id list of utterance u.  Utterance u's dropout masks are keyed by ``seeds[u]``, or
        ``seed_base + u``: by its position in the corpus and not by its group, so its GTA mel does not depend on ``batch_utts``.  The
        utterances go through ``wrnn_taco_gta_corpus`` in groups of ``batch_utts`` formed by frame count, back to back on the current
        stream; the mels never leave the device.  The library's scratch is grown once, before the first group, to the need of the largest
        (that waits for the stream when it grows at all); no group waits, and the host waits once at the end, for the report.

        The new corpus shares ``labels`` and the label tables, owns a new ``mels`` table with the same offsets and frame counts, has
        ``gta_made == True`` and keeps this corpus's table as ``source_mels``.  ``report``: host arrays with one entry per utterance --
        ``l1`` (mean |GTA - ground truth| in [0, 1] units), ``focus`` (the mean over the decoder's steps of the largest alignment),
        ``last_attention`` (``max_attentions`` of the last step), ``tx``, ``frames``, ``steps``.
        ``ValueError``: the mels are not Tacotron's (``features``), ``n_mels`` is not the model's, or the sequences do not match the
        utterances in number.  A group the library refuses raises ``_cabi.WrnnError`` with its reason and the utterance's stem."""
        import ctypes as C
        import re
        if self.features != 'tacotron':
            raise ValueError(f'this corpus holds {self.features!r} mel features: a Tacotron is teacher-forced on its own kind, make the '
                             f'corpus with features=\'tacotron\'')
        if self.n_mels != int(model.num_mels):
            raise ValueError(f'the corpus has {self.n_mels} mel bands, the Tacotron predicts {int(model.num_mels)}')
        N = len(self)
        if len(sequences) != N:
            raise ValueError(f'{len(sequences)} symbol sequences for {N} utterances')
        dev = self.device
        if dev.index != int(model.device):
            raise ValueError(f'the corpus lives on {dev}, the Tacotron on device {model.device}')
        if seeds is not None and len(seeds) != N:
            raise ValueError(f'{len(seeds)} seeds for {N} utterances')
        seqs = [np.asarray(s, dtype=np.int64).reshape(-1) for s in sequences]
        for u, q in enumerate(seqs):
            if q.size and (q.min() < -2 ** 31 or q.max() >= 2 ** 31):
                raise ValueError(f'utterance {self.stems[u]!r}: a symbol id does not fit 32 bits')
        tx = np.array([len(q) for q in seqs], np.int32)
        seed_of = [(int(seeds[u]) if seeds is not None else int(seed_base) + u) & (2 ** 64 - 1) for u in range(N)]
        r, M = int(model.r), self.n_mels
        frames = self.frames.astype(np.int32)
        report = dict(l1=np.zeros(N, np.float64), focus=np.zeros(N, np.float64), last_attention=np.zeros(N, np.int32), tx=tx.copy(),
                      frames=frames.copy(), steps=((frames.astype(np.int64) + r - 1) // r).astype(np.int32))
        note = dict(checkpoint=getattr(model, 'checkpoint', None), seed_base=int(seed_base))
        step = max(1, int(batch_utts))
        order = np.argsort(frames, kind='stable')
        groups = [order[g:g + step] for g in range(0, N, step)]
        with torch.cuda.device(dev):
            stream = torch.cuda.current_stream(dev).cuda_stream
            out = torch.zeros_like(self.mels)
            made = DeviceCorpus(self.labels, out, self.label_off, self.label_len, self.mel_off, self.frames, M, self.stems,
                                source_mels=self.mels, gta=True, gta_note=note, **self._meta())
            made._tables = self.device_tables()
            if not N:
                return made, report
            widths = [max(int(tx[ids].max()), 1) for ids in groups]
            if max(widths) <= _cabi.TACO_MAX_TX:   # the scratch for the largest group now, so that no group waits for it to grow (an
                model.native.gta_reserve(min(step, N), max(widths), max(int(frames.max()), 1), stream)   # over-long text is refused below, by name)
            l1, focus = torch.zeros(N, dtype=torch.float64, device=dev), torch.zeros(N, dtype=torch.float64, device=dev)
            last = torch.zeros(N, dtype=torch.int32, device=dev)
            # page-locked host arrays for every group: the library's copies are queued, nothing waits for them
            pin32 = torch.zeros(sum(len(ids) * w for ids, w in zip(groups, widths)) + 2 * N, dtype=torch.int32).pin_memory()
            pin64 = torch.zeros(3 * N, dtype=torch.int64).pin_memory()
            h32, h64 = pin32.numpy(), pin64.numpy()
            at32 = at = 0
            for ids, w in zip(groups, widths):
                B = len(ids)
                ids_h, at32 = h32[at32:at32 + B * w].reshape(B, w), at32 + B * w
                tx_h, fr_h, at32 = h32[at32:at32 + B], h32[at32 + B:at32 + 2 * B], at32 + 2 * B
                seeds_h, off_h = h64[3 * at:3 * at + B].view(np.uint64), h64[3 * at + B:3 * at + 2 * B]
                for b, u in enumerate(ids):
                    ids_h[b, :len(seqs[u])] = seqs[u][:w]
                    seeds_h[b] = seed_of[u]
                tx_h[:], fr_h[:], off_h[:] = tx[ids], frames[ids], self.mel_off[ids]
                call = _cabi.TacoGtaCall()
                call.struct_size = C.sizeof(_cabi.TacoGtaCall)
                call.B, call.Tx_max, call.prenet_dropout = B, w, int(bool(prenet_dropout))
                call.ids_host, call.tx_host, call.seeds_host = ids_h.ctypes.data, tx_h.ctypes.data, seeds_h.ctypes.data
                call.frames_host, call.mel_off_host, call.out_off_host = fr_h.ctypes.data, off_h.ctypes.data, off_h.ctypes.data
                call.mels_dev, call.mels_elems = self.mels.data_ptr(), self.mels.numel()
                call.gta_mels_dev, call.out_elems = out.data_ptr(), out.numel()
                call.l1_dev, call.focus_dev, call.last_attention_dev = l1[at:].data_ptr(), focus[at:].data_ptr(), last[at:].data_ptr()
                try:
                    model.native.gta_corpus(call, stream)
                except _cabi.WrnnError as e:
                    torch.cuda.current_stream(dev).synchronize()   # the groups already queued read the page-locked arrays
                    reason = str(e).split(': ', 1)[-1]
                    named = re.search(r'utterance (\d+)', reason)
                    if named and int(named.group(1)) < B:
                        reason += f' (utterance {named.group(1)} of its group is {self.stems[int(ids[int(named.group(1))])]!r})'
                    raise _cabi.WrnnError(e.code, reason) from None
                at += B
            torch.cuda.current_stream(dev).synchronize()           # the one wait: the report, and the page-locked arrays may go
            report['l1'][order], report['focus'][order] = l1.cpu().numpy(), focus.cpu().numpy()
            report['last_attention'][order] = last.cpu().numpy()
        return made, report

    # ------------------------------------------------------------------ constructors
    @classmethod
    def from_pairs(cls, pairs, device=None, *, hop_length: int, stems: Optional[Sequence[str]] = None, **meta) -> 'DeviceCorpus':
        """From host ``(mel (n_mels, frames), labels)`` arrays (what ``pairs()`` returns, what ``WindowLoader`` takes)."""
        dev = _device(device)
        pairs = list(pairs)
        if not pairs:
            raise ValueError('expected at least one utterance')
        n_mels = int(pairs[0][0].shape[0])
        frames = [int(m.shape[1]) for m, _ in pairs]
        lens = [int(np.shape(w)[0]) for _, w in pairs]
        if any(m.ndim != 2 or m.shape[0] != n_mels for m, _ in pairs):
            raise ValueError(f'expected (n_mels = {n_mels}, frames) mels')
        label_off = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int64)
        mel_off = np.concatenate([[0], np.cumsum(frames)[:-1]]).astype(np.int64) * n_mels
        labels = np.concatenate([np.asarray(w).astype(np.int32) for _, w in pairs])
        mels = np.concatenate([np.ascontiguousarray(np.asarray(m, np.float32).T).reshape(-1) for m, _ in pairs])
        names = list(stems) if stems is not None else [f'utt{i:05d}' for i in range(len(pairs))]
        return cls(torch.from_numpy(labels).to(dev), torch.from_numpy(mels).to(dev), label_off, lens, mel_off, frames, n_mels, names,
                   hop_length=hop_length, **meta)

    @classmethod
    def from_wavs(cls, paths_or_arrays, hp, device=None, batch_clips: int = 16, resample: bool = False, trim_top_db=None,
                  peak_norm=None, features: str = 'vocoder') -> 'DeviceCorpus':
        """Wav files (``frontend.load_wav``) or float arrays in [-1, 1] -> corpus.  The clips go to the device in ragged groups of
        ``batch_clips`` (grouped by length, so that little of a group's buffer is padding); each group's buffer is read by one launch of
        the mel front end and one of ``wrnn_quantise``.  Bits and companding follow ``hp`` (``signal_bits``); utterances too short for
        ``hp.voc_seq_len`` / ``hp.voc_pad`` are dropped like ``get_vocoder_datasets`` does.  ``n_clipped`` counts samples with
        ``|x| > 1``: their labels are clipped, where the reference asserts.

        An array item may be an ``(array, rate)`` pair.  A file or a pair at another rate than ``hp.sample_rate`` raises ``ValueError``
        unless ``resample=True``: then the groups are formed per source rate, a group at another rate is uploaded at its own rate and one
        launch of ``frontend.Resampler`` writes the zero-padded buffer the two launches above read -- no host round trip is added.  Lengths,
        frame counts and the short-utterance filter use the resampled length.  Resampled peaks may exceed 1 (``n_clipped`` counts them)
        unless ``peak_norm`` is on.

        ``trim_top_db`` / ``peak_norm`` (both off by default; ``hp.peak_norm`` is not consulted, the reference reads it nowhere either):
        every group is conditioned on the device by ``frontend.WavConditioner`` between the resampler and the two launches above --
        leading and trailing silence trimmed like ``librosa.effects.trim(wav, top_db=trim_top_db, frame_length=2048, hop_length=512)``,
        then ``wav / abs(wav).max() * 0.999`` (``peak_norm=True``; a number is the target), the reference's
        ``tacotron/datasets/preprocessor.py:62-72``.  One host wait per group is added, for the trimmed lengths that size the corpus
        tables; lengths, frame counts and the short-utterance filter use the trimmed length.  The corpus keeps the two settings as
        ``trim_top_db`` and ``peak_norm`` (the target, or ``None``).

        ``features``: the feature profile of the mels (``frontend.FEATURE_PROFILES``), kept as ``self.features``.  Under ``'tacotron'``
        the mel is Tacotron's (of the pre-emphasised clip; the pre-emphasis happens inside the mel kernel) and the audio target is what
        ``tacotron/datasets/preprocessor.py:100-112`` stores: the conditioned, NOT pre-emphasised clip zero-padded on the right to
        ``frames * hop`` samples, so an utterance has ``frames * hop`` labels whose tail is the label of 0.0.  With ``trim_top_db=25,
        peak_norm=True`` that is the reference's whole recipe."""
        from .frontend import MelFrontEnd, Resampler, WavConditioner, condition_settings, load_wav, read_wav
        trim_top_db, peak_target = condition_settings(trim_top_db, peak_norm)
        cond = WavConditioner(trim_top_db, peak_target) if trim_top_db is not None or peak_target is not None else None
        dev = _device(device)
        fe = MelFrontEnd(hp, device=dev, features=features)
        padded = features == 'tacotron'                           # labels cover frames * hop samples, the tail being zeros
        hop, n_mels = fe.hop_length, fe.n_mels
        bits, mu_law = signal_bits(hp)
        least = min_frames(hop_length=hop, pad=int(hp.voc_pad), seq_len=int(hp.voc_seq_len))
        clips, stems, rates, out_lens, resamplers = [], [], [], [], {}
        for i, item in enumerate(paths_or_arrays):
            rate = fe.sample_rate
            if isinstance(item, (str, Path)):
                stem = Path(item).stem
                if resample:
                    wav, rate = read_wav(item)
                else:
                    wav = load_wav(item, fe.sample_rate)
            else:
                if isinstance(item, tuple) and len(item) == 2 and np.ndim(item[1]) == 0 and np.ndim(item[0]) == 1:
                    item, rate = item[0], int(item[1])
                wav = item.detach().cpu().numpy() if isinstance(item, torch.Tensor) else np.asarray(item)
                wav, stem = np.ascontiguousarray(wav, dtype=np.float32), f'utt{i:05d}'
            if wav.ndim != 1:
                raise ValueError(f'expected 1-D clips of samples, got shape {wav.shape}')
            n = int(wav.shape[0])
            if rate != fe.sample_rate:
                if not resample:
                    raise ValueError(f'clip {stem!r} is sampled at {rate} Hz, the model needs {fe.sample_rate} Hz: pass resample=True '
                                     f'for the resampler on the device')
                if rate not in resamplers:
                    resamplers[rate] = Resampler(rate, fe.sample_rate, device=dev)
                n = resamplers[rate].out_len(n)
            if 1 + n // hop < least or wav.shape[0] < 1:
                continue
            if trim_top_db is not None:
                cond.frames(n)   # ValueError for a clip too short for the trim window, before any device work
            clips.append(wav)
            stems.append(stem)
            rates.append(rate)
            out_lens.append(n)
        if not clips:
            raise ValueError(f'no utterance has the {least} mel frames one training window needs')
        lens = np.array(out_lens, np.int64)                       # at the model's rate
        src_lens = np.array([c.shape[0] for c in clips], np.int64)
        frames = np.array([fe.frames(int(n)) for n in lens], np.int64)
        label_len = frames * hop if padded else lens
        label_off = np.concatenate([[0], np.cumsum(label_len)[:-1]]).astype(np.int64)
        mel_off = np.concatenate([[0], np.cumsum(frames)[:-1]]).astype(np.int64) * n_mels
        by_len = np.argsort(lens, kind='stable')
        rates = np.array(rates, np.int64)
        step = max(1, int(batch_clips))
        groups = []                                               # the model's own rate first, then the others as they first appear
        for rate in [fe.sample_rate] + list(resamplers):
            ids = by_len[rates[by_len] == rate]
            groups += [(rate, ids[g:g + step]) for g in range(0, len(ids), step)]
        if cond is not None:
            return cls._from_wavs_conditioned(clips, stems, groups, src_lens, lens, resamplers, fe, cond, dev, bits, mu_law, least, padded)
        with torch.cuda.device(dev):
            stream = torch.cuda.current_stream(dev).cuda_stream
            labels = torch.empty(int(label_len.sum()), dtype=torch.int32, device=dev)
            mels = torch.empty(int(frames.sum()) * n_mels, dtype=torch.float32, device=dev)
            clipped = torch.zeros(1, dtype=torch.int64, device=dev)
            for rate, ids in groups:
                host = np.zeros((len(ids), int(src_lens[ids].max()) + (hop if padded and rate == fe.sample_rate else 0)), np.float32)
                for r, u in enumerate(ids):
                    host[r, :src_lens[u]] = clips[u]
                wav = torch.from_numpy(host).to(dev)
                if rate != fe.sample_rate:
                    wav = resamplers[rate].resample_padded(wav, src_lens[ids])      # (B, max lens[ids]), zero past each clip
                if padded:
                    wav = _widened(wav, int(label_len[ids].max()))
                n_max = int(wav.shape[1])
                mel = fe.melspectrogram_padded(wav, lens[ids])                      # (B, n_mels, T_max)
                lab = torch.empty((len(ids), n_max), dtype=torch.int32, device=dev)
                _cabi.quantise(wav.data_ptr(), wav.numel(), bits, mu_law, lab.data_ptr(), clipped.data_ptr(), stream)   # the padding is 0: never clipped
                for r, u in enumerate(ids):
                    n, t = int(label_len[u]), int(frames[u])
                    labels[int(label_off[u]):int(label_off[u]) + n] = lab[r, :n]
                    mels[int(mel_off[u]):int(mel_off[u]) + t * n_mels].view(t, n_mels).copy_(mel[r, :, :t].t())
            n_clipped = int(clipped.item())
        return cls(labels, mels, label_off, label_len, mel_off, frames, n_mels, stems, hop_length=hop, sample_rate=fe.sample_rate, bits=bits,
                   mu_law=mu_law, n_clipped=n_clipped, features=features)

    @classmethod
    def _from_wavs_conditioned(cls, clips, stems, groups, src_lens, lens, resamplers, fe, cond, dev, bits, mu_law, least,
                               padded=False) -> 'DeviceCorpus':
        """``from_wavs`` behind its first pass when trimming or peak normalisation is on.  Per group: upload -> resample (a group at
        another rate) -> condition -> mel and quantise, all reading device buffers; the trimmed lengths are read once per group, they decide
        which clips stay and size the tables.  The utterances keep the order they were given in.  ``padded``: an utterance's labels
        cover ``frames * hop`` samples of its zero-padded row, not the clip alone."""
        hop, n_mels = fe.hop_length, fe.n_mels
        kept = {}                                                 # utterance -> (labels, mel frames-major, samples, frames), its own tensors
        with torch.cuda.device(dev):
            stream = torch.cuda.current_stream(dev).cuda_stream
            clipped = torch.zeros(1, dtype=torch.int64, device=dev)
            for rate, ids in groups:
                host = np.zeros((len(ids), int(src_lens[ids].max()) + (hop if padded and rate == fe.sample_rate else 0)), np.float32)
                for r, u in enumerate(ids):
                    host[r, :src_lens[u]] = clips[u]
                wav = torch.from_numpy(host).to(dev)
                if rate != fe.sample_rate:
                    wav = resamplers[rate].resample_padded(wav, src_lens[ids])
                wav, n_out = cond.condition_padded(wav, lens[ids])                  # (B, max lens[ids]), zero past each trimmed clip
                new = n_out.cpu().numpy().astype(np.int64)                          # the group's one host wait
                rows = [r for r in range(len(ids)) if 1 + int(new[r]) // hop >= least]
                if not rows:
                    continue
                if len(rows) < len(ids):
                    wav = wav[torch.tensor(rows, device=dev)].contiguous()
                ids, new = ids[rows], new[rows]
                if padded:
                    wav = _widened(wav, (1 + int(new.max()) // hop) * hop)
                mel = fe.melspectrogram_padded(wav, new)
                lab = torch.empty(tuple(wav.shape), dtype=torch.int32, device=dev)
                _cabi.quantise(wav.data_ptr(), wav.numel(), bits, mu_law, lab.data_ptr(), clipped.data_ptr(), stream)
                for r, u in enumerate(ids):
                    t = int(fe.last_frames[r])
                    n = t * hop if padded else int(new[r])
                    kept[int(u)] = (lab[r, :n].clone(), mel[r, :, :t].t().contiguous().view(-1), n, t)
            if not kept:
                raise ValueError(f'no utterance has the {least} mel frames one training window needs after trimming')
            order = sorted(kept)
            new_lens = np.array([kept[u][2] for u in order], np.int64)
            frames = np.array([kept[u][3] for u in order], np.int64)
            label_off = np.concatenate([[0], np.cumsum(new_lens)[:-1]]).astype(np.int64)
            mel_off = np.concatenate([[0], np.cumsum(frames)[:-1]]).astype(np.int64) * n_mels
            labels = torch.empty(int(new_lens.sum()), dtype=torch.int32, device=dev)
            mels = torch.empty(int(frames.sum()) * n_mels, dtype=torch.float32, device=dev)
            for k, u in enumerate(order):
                lab, mel, n, t = kept.pop(u)
                labels[int(label_off[k]):int(label_off[k]) + n] = lab
                mels[int(mel_off[k]):int(mel_off[k]) + t * n_mels] = mel
            n_clipped = int(clipped.item())
        return cls(labels, mels, label_off, new_lens, mel_off, frames, n_mels, [stems[u] for u in order], hop_length=hop,
                   sample_rate=fe.sample_rate, bits=bits, mu_law=mu_law, n_clipped=n_clipped, trim_top_db=cond.trim_top_db,
                   peak_norm=cond.peak_target, features=fe.features)

    # ------------------------------------------------------------------ files
    def save(self, out_dir: Union[str, Path]) -> Path:
        """``quant/<stem>.npy`` (int32 labels), ``mel/<stem>.npy`` (``(frames, n_mels)`` float32, the reference's file layout) and
        ``wavernn_training_data.txt`` with one ``quant|mel|mel|stem`` line per utterance: fields 0 and 2 are what
        ``train.read_feature_list`` and the reference's ``get_vocoder_datasets`` read.  The feature profile of the mels goes into
        ``wavernn_training_features.txt`` next to it (``saved_features`` reads it back).  Returns the list file's path."""
        out = Path(out_dir).expanduser().resolve()
        (out / 'quant').mkdir(parents=True, exist_ok=True)
        (out / 'mel').mkdir(parents=True, exist_ok=True)
        if len(set(self.stems)) != len(self.stems):
            raise ValueError('two utterances share a name: their files would overwrite each other')
        if self.gta_made:
            return self._save_gta(out)
        lines = []
        for (mel, lab), stem in zip(self.pairs(), self.stems):
            q, m = out / 'quant' / f'{stem}.npy', out / 'mel' / f'{stem}.npy'
            np.save(q, lab.astype(np.int32), allow_pickle=False)
            np.save(m, np.ascontiguousarray(mel.T, dtype=np.float32), allow_pickle=False)
            lines.append(f'{q}|{m}|{m}|{stem}\n')
        listing = out / LIST_NAME
        listing.write_text(''.join(lines), encoding='utf-8')
        (out / FEATURES_NAME).write_text(self.features + '\n', encoding='utf-8')
        return listing

    def _save_gta(self, out: Path) -> Path:
        """``save`` of a GTA corpus: ``mel/<stem>.npy`` is the ground truth (``source_mels``), ``mel_gta/<stem>.npy`` the GTA mel, and
        the lines are ``quant|mel|mel_gta|stem`` -- the reference's own ``quant | mel | predicted mel | text``, of which
        ``read_feature_list``, ``load`` and the reference's ``get_vocoder_datasets`` read fields 0 and 2.  ``wavernn_training_gta.txt``
        notes the checkpoint's name and the seed base."""
        (out / 'mel_gta').mkdir(parents=True, exist_ok=True)
        lines = []
        for (gta, lab), stem, mo, t in zip(self.pairs(), self.stems, self.mel_off, self.frames):
            q, m, g = out / 'quant' / f'{stem}.npy', out / 'mel' / f'{stem}.npy', out / 'mel_gta' / f'{stem}.npy'
            truth = self.source_mels[int(mo):int(mo) + int(t) * self.n_mels].cpu().numpy().reshape(int(t), self.n_mels)
            np.save(q, lab.astype(np.int32), allow_pickle=False)
            np.save(m, np.ascontiguousarray(truth, dtype=np.float32), allow_pickle=False)
            np.save(g, np.ascontiguousarray(gta.T, dtype=np.float32), allow_pickle=False)
            lines.append(f'{q}|{m}|{g}|{stem}\n')
        listing = out / LIST_NAME
        listing.write_text(''.join(lines), encoding='utf-8')
        (out / FEATURES_NAME).write_text(self.features + '\n', encoding='utf-8')
        (out / GTA_NAME).write_text(f'checkpoint {self.gta_note.get("checkpoint")}\nseed_base {self.gta_note.get("seed_base")}\n', encoding='utf-8')
        return listing

    @classmethod
    def load(cls, list_file_or_pairs, device=None, *, hop_length: int, **meta) -> 'DeviceCorpus':
        """A saved corpus back on the device without recomputing anything: ``list_file_or_pairs`` is the list file ``save`` wrote
        (every line is taken, in order) or ``(quantised wav path, mel path)`` pairs such as ``train.read_feature_list`` returns.  A list
        file brings the features ``save`` recorded next to it; for pairs say ``features=`` (default ``'vocoder'``)."""
        if isinstance(list_file_or_pairs, (str, Path)):
            meta.setdefault('features', saved_features(list_file_or_pairs))
            items = []
            with open(list_file_or_pairs, 'r', encoding='utf-8') as f:
                for line in f:
                    parts = [p.strip() for p in line.strip().split('|')]
                    if len(parts) >= 3:
                        items.append((parts[0], parts[2], parts[3] if len(parts) > 3 and parts[3] else Path(parts[0]).stem))
        else:
            items = [(str(q), str(m), Path(q).stem) for q, m in list_file_or_pairs]
        if not items:
            raise ValueError('the list names no utterance')
        pairs = [(np.load(m).T, np.load(q)) for q, m, _ in items]
        return cls.from_pairs(pairs, device, hop_length=hop_length, stems=[s for _, _, s in items], **meta)


def _widened(wav: torch.Tensor, width: int) -> torch.Tensor:
    """``wav`` (B, n) as it is when ``n >= width``, else a copy zero-padded on the right to ``width`` columns."""
    return wav if wav.shape[1] >= width else torch.nn.functional.pad(wav, (0, width - wav.shape[1]))


class DeviceWindowLoader:
    """``train.WindowLoader`` over a :class:`DeviceCorpus`: a sized iterable, shuffled per epoch, a fresh random window per utterance,
    a last short batch kept -- and every batch ``(x, y, mels)`` built on the device by one ``wrnn_collate_windows`` launch after one
    small host-to-device copy of the batch's ``(utterance, offset)`` pairs.  The permutation and the offsets are drawn on the host from
    ``np.random.Generator(PCG64(seed))`` in ``WindowLoader``'s order, so batch k equals batch k of
    ``WindowLoader(corpus.pairs(), ...)`` with the same seed bit for bit.  ``corpus`` needs ``len()`` and ``frames`` for ``draws()``;
    iterating needs a real ``DeviceCorpus``."""

    def __init__(self, corpus, batch_size: int, *, mode: str, bits: int, hop_length: int, pad: int, seq_len: int, seed: int = 0):
        self.corpus, self.batch_size, self.mode = corpus, int(batch_size), mode
        self.sig_bits = 16 if mode == 'MOL' else int(bits)
        self.kw = dict(hop_length=int(hop_length), pad=int(pad), seq_len=int(seq_len))
        self.rng = np.random.Generator(np.random.PCG64(seed))

    def __len__(self):
        return (len(self.corpus) + self.batch_size - 1) // self.batch_size

    def draws(self):
        """One epoch of ``(utterance indices, window offsets)`` int32 array pairs, one per batch: host only.  Raises the
        ``ValueError``s of ``collate_windows`` (``seq_len`` against the hop, an utterance too short)."""
        frames = np.asarray(self.corpus.frames)
        order = self.rng.permutation(len(frames))
        for i in range(0, len(order), self.batch_size):
            utt = order[i:i + self.batch_size]
            yield utt.astype(np.int32), np.asarray(draw_window_offsets(frames[utt], rng=self.rng, **self.kw), np.int32)

    def __iter__(self):
        c, kw = self.corpus, self.kw
        if kw['hop_length'] != c.hop_length:
            raise ValueError(f'the corpus was made with hop {c.hop_length}, the loader asks for {kw["hop_length"]}')
        for utt, off in self.draws():      # validated on the host: utt is a permutation's slice, off inside the collate's range
            dev, B, win = c.device, len(utt), kw['seq_len'] // kw['hop_length'] + 2 * kw['pad']
            with torch.cuda.device(dev):
                label_off, mel_off, frames = c.device_tables()
                uo = torch.from_numpy(np.stack([utt, off])).to(dev)
                x = torch.empty((B, kw['seq_len']), dtype=torch.float32, device=dev)
                y = torch.empty((B, kw['seq_len']), dtype=torch.float32 if self.mode == 'MOL' else torch.int64, device=dev)
                mels = torch.empty((B, c.n_mels, win), dtype=torch.float32, device=dev)
                _cabi.collate_windows(c.labels.data_ptr(), c.mels.data_ptr(), label_off.data_ptr(), mel_off.data_ptr(), frames.data_ptr(),
                                      uo[0].data_ptr(), uo[1].data_ptr(), B, c.n_mels, kw['hop_length'], kw['pad'], kw['seq_len'], self.sig_bits,
                                      self.mode == 'MOL', x.data_ptr(), y.data_ptr(), mels.data_ptr(), torch.cuda.current_stream(dev).cuda_stream)
            yield x, y, mels


def add_gta_arguments(parser) -> None:
    """The ``--gta_*`` options of ``wavernn_preprocess.py`` and ``wavernn_train.py`` (with ``--wav_dir DIR --features tacotron``)."""
    parser.add_argument('--gta_checkpoint', metavar='TACO.npz', default=None,
                        help='replace the mels of the --wav_dir corpus by the ones this Tacotron predicts under teacher forcing (GTA): '
                             'the vocoder then learns from the mels it is given at synthesis time.  Needs --features tacotron and --gta_metadata')
    parser.add_argument('--gta_metadata', metavar='train.txt', default=None,
                        help='the Tacotron\'s training list (audio-NAME.npy|mel-NAME.npy|samples|frames|text|pinyin): the pinyin of clip NAME.wav, '
                             'and the symbol table')
    parser.add_argument('--gta_seed', type=int, default=0, metavar='N', help='utterance u draws its prenet dropout masks from seed N + u')
    parser.add_argument('--gta_batch', type=int, default=64, metavar='N', help='utterances per call of the teacher-forced decoder')
    parser.add_argument('--gta_report', metavar='FILE.tsv', default=None,
                        help='write one line per utterance: stem, frames, tx, l1, focus, last_attention')
    parser.add_argument('--gta_min_focus', type=float, default=None, metavar='F',
                        help='keep only the utterances whose attention focus is at least F (default: keep all)')


def gta_arguments(args) -> bool:
    """Whether the arguments ask for a GTA corpus; ``ValueError`` for a combination that cannot be served."""
    if args.gta_checkpoint is None:
        given = [n for n in ('gta_metadata', 'gta_report', 'gta_min_focus') if getattr(args, n) is not None]
        if given:
            raise ValueError(f'--{given[0]} belongs to --gta_checkpoint: without a Tacotron there are no GTA mels')
        return False
    if getattr(args, 'wav_dir', None) is None:
        raise ValueError('--gta_checkpoint teacher-forces the Tacotron on the corpus made from --wav_dir: give --wav_dir')
    if args.features != 'tacotron':
        raise ValueError(f'--gta_checkpoint needs --features tacotron: the decoder is fed the corpus\'s own mels, and those must be the '
                         f'features the Tacotron was trained on, not the {args.features!r} ones')
    if args.gta_metadata is None:
        raise ValueError('--gta_checkpoint needs --gta_metadata: the Tacotron reads each clip\'s pinyin, and the list also makes the symbol table')
    if args.gta_batch < 1:
        raise ValueError(f'--gta_batch {args.gta_batch} < 1')
    return True


def gta_from_arguments(corpus: 'DeviceCorpus', args) -> 'DeviceCorpus':
    """``corpus.gta`` as the ``--gta_*`` arguments ask for it: the checkpoint's dims are read off its tensors, a clip's stem looks up its
    line of the metadata, the report goes to ``--gta_report`` and ``--gta_min_focus`` drops the utterances below it."""
    import os
    from . import tacotron as taco
    symbols, metadata = taco.load_symbols(args.gta_metadata), taco.read_metadata(args.gta_metadata)
    with np.load(args.gta_checkpoint, allow_pickle=False) as z:
        state = {k: z[k] for k in z.files}
    dims = taco.dims_from_state(state)
    if dims['n_symbols'] != len(symbols):
        raise ValueError(f'{args.gta_metadata} makes {len(symbols)} symbols, the checkpoint\'s embedding has {dims["n_symbols"]} rows')
    seqs = taco.metadata_sequences(metadata, corpus.stems, symbols, args.gta_metadata)
    model = taco.Tacotron(device=corpus.device.index, **dims).load_state(state)
    model.checkpoint = os.path.basename(args.gta_checkpoint)
    made, report = corpus.gta(model, seqs, seed_base=args.gta_seed, batch_utts=args.gta_batch)
    if args.gta_report:
        with open(args.gta_report, 'w', encoding='utf-8') as f:
            f.write('stem\tframes\ttx\tl1\tfocus\tlast_attention\n')
            for u, stem in enumerate(made.stems):
                f.write(f'{stem}\t{report["frames"][u]}\t{report["tx"][u]}\t{report["l1"][u]:.6f}\t{report["focus"][u]:.6f}\t{report["last_attention"][u]}\n')
    print(f'GTA mels of {len(made)} utterances from {model.checkpoint} | mean l1 {float(report["l1"].mean()):.4f} | '
          f'mean focus {float(report["focus"].mean()):.4f}')
    if args.gta_min_focus is not None:
        keep = np.flatnonzero(report['focus'] >= args.gta_min_focus)
        print(f'--gta_min_focus {args.gta_min_focus}: {len(made) - len(keep)} of {len(made)} utterances dropped')
        made = made.subset(keep)
    return made


def build_parser():
    import argparse
    from .hparams import DEFAULT_HPARAMS
    parser = argparse.ArgumentParser(description='Preprocess a folder of wavs for WaveRNN vocoder training')
    parser.add_argument('--wav_dir', required=True, metavar='DIR', help='folder of wav files at hp.sample_rate (any rate with --resample)')
    parser.add_argument('--out_dir', required=True, metavar='DIR', help='where quant/, mel/ and the list file go')
    parser.add_argument('--hp_file', metavar='FILE', default=DEFAULT_HPARAMS, help='The file to use for the hyperparameters')
    parser.add_argument('--batch_clips', type=int, default=16, help='clips per launch of the front end')
    parser.add_argument('--resample', action='store_true', help='resample files at another rate to hp.sample_rate on the device '
                                                                '(default: such a file is an error)')
    from .frontend import add_condition_arguments, add_features_argument
    add_condition_arguments(parser, 'the files')
    add_features_argument(parser, 'the files')
    add_gta_arguments(parser)
    return parser


def main(argv=None):
    """``python wavernn_preprocess.py --wav_dir DIR --out_dir DIR``: every ``*.wav`` of the folder -> ``quant/``, ``mel/`` and the
    training list ``wavernn_train.py`` reads (``hp.feature_path``)."""
    from .frontend import condition_arguments
    from .hparams import hparams as hp
    args = build_parser().parse_args(argv)
    conditioning = condition_arguments(args)
    want_gta = gta_arguments(args)
    hp.configure(args.hp_file)
    if not torch.cuda.is_available():
        raise RuntimeError('the preprocessing runs on an MI355X only (no CPU path)')
    wavs = sorted(Path(args.wav_dir).expanduser().glob('*.wav'))
    if not wavs:
        raise FileNotFoundError(f'no *.wav files in {args.wav_dir}')
    corpus = DeviceCorpus.from_wavs(wavs, hp, 'cuda', batch_clips=args.batch_clips, resample=args.resample, features=args.features,
                                    **conditioning)
    if want_gta:
        corpus = gta_from_arguments(corpus, args)
    listing = corpus.save(args.out_dir)
    print(f'{len(corpus)} utterances of {len(wavs)} files | {corpus.hours:.3f} hours | {corpus.n_clipped} clipped samples | '
          f'{corpus.bits} bits {"mu-law" if corpus.mu_law else "linear"} | {corpus.features} features'
          f'{" | GTA mels in mel_gta/" if corpus.gta_made else ""} | {listing}')
    return listing


if __name__ == "__main__":
    main()
