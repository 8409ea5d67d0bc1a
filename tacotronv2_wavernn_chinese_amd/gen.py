"""Mirror of the reference's vocoder CLI ``wavernn_gen.py``.

``gen_from_file(model, load_path, save_path, batched, target, overlap)`` follows
``wavernn_gen.py:13-43``: a ``.npy`` mel shaped ``(T, n_mels)`` in ``[0, 1]`` (the format
``tacotron_synthesize.py:114-116`` writes) is transposed, validated, wrapped to ``(1, n_mels, T)`` and
handed to ``model.generate``; the output file name pattern is the reference's (:35-39).

Deliberate differences: the reference hard-overrides ``batched = False`` and
``device = cpu`` after parsing its flags (:76-77, :93); here ``--batched`` is honoured and the model
runs on the MI355X.  Extensions: ``--kernel NAME``, ``--teamg-weights f32|f16|e4m3``, ``--teamg-sparse``, ``--target auto|per_xcd``, ``--noise reference [--seed N]``, ``--stream-frames N`` (streaming generation)
(the reference's own noise stream: ``vocoder.reference_noise``).

The ``.wav`` branch (:17-20) does what the reference's intends: ``load_wav``, the input saved as ``__{idx}__{k}k_steps_target.wav`` (the
reference names an undefined ``file_name`` there; ``idx`` is the stem it computes at :38), then the mel of the clip -- built on the device by
``frontend.MelFrontEnd`` (``csrc/melspec.hip``) instead of librosa -- takes the same path as a ``.npy`` mel, ``--stream-frames`` included.  A file
at another sample rate raises ``ValueError`` unless ``resample=True`` / ``--resample``: then it is resampled on the device
(``frontend.Resampler``, ``csrc/resample.hip``) and the saved target file is the resampled clip at the model's rate, as the reference's is.
``trim_top_db=`` / ``peak_norm=`` (``--trim_silence [--trim_top_db DB]``, ``--peak_norm [TARGET]``; off by default): the clip is conditioned
on the device like the training wavs of a corpus made with the same settings (``frontend.WavConditioner``, ``csrc/condition.hip``), and the
saved target file is the conditioned clip.  ``features=`` (``--features {vocoder,tacotron}``): the feature profile of the mel;
``'tacotron'`` is the mel Tacotron's preprocessing makes, for a checkpoint trained the reference's way (``frontend.FEATURE_PROFILES``).
The saved target file is the same under both: the pre-emphasis happens inside the mel kernel.
"""
from __future__ import annotations

import argparse
import os
import time

import numpy as np
import torch

from .dsp import save_wav
from .frontend import add_condition_arguments, add_features_argument, condition_arguments, load_wav
from .hparams import hparams as hp
from .vocoder import WaveRNN


def gen_from_file(model: WaveRNN, load_path, save_path, batched, target, overlap, stream_frames=None, resample=False, trim_top_db=None,
                  peak_norm=None, features='vocoder', **generate_opts):
    k = model.get_step() // 1000
    load_path = str(load_path)
    if ".npy" in load_path:
        mel = np.load(load_path).T
        if mel.ndim != 2 or mel.shape[0] != hp.num_mels:
            raise ValueError(f'Expected a numpy array shaped (n_mels, n_hops), but got {mel.shape}!')
        _max, _min = np.max(mel), np.min(mel)
        if _max >= 1.01 or _min <= -0.01:
            raise ValueError(f'Expected spectrogram range in [0,1] but was instead [{_min}, {_max}]')
        mel = torch.tensor(mel).unsqueeze(0)
    elif ".wav" in load_path:
        if not os.path.isfile(load_path):   # an input check like the ones above, not an OSError from inside the wav reader
            raise ValueError(f'{load_path}: no such wav file')
        on_device = resample or trim_top_db is not None or (peak_norm is not None and peak_norm is not False)
        wav = load_wav(load_path, hp.sample_rate, resample=resample, device=torch.device('cuda', model._device_index()) if on_device else None,
                       trim_top_db=trim_top_db, peak_norm=peak_norm, features=features)
        idx = load_path.split('/')[-1].strip().split('.')[0]
        save_wav(wav, os.path.join(str(save_path), f'__{idx}__{k}k_steps_target.wav'), hp.sample_rate)
        fe = model.mel_front_end() if features == 'vocoder' else model.mel_front_end(features=features)   # a model-like object need not know profiles
        mel = fe.melspectrogram(wav, device=torch.device('cuda', model._device_index()))   # (1, n_mels, T) on the device
    else:
        raise ValueError(f"Expected an extension of .wav or .npy, but got {os.path.splitext(load_path)[1]}!")

    if stream_frames:
        return _gen_streamed(model, mel, load_path, save_path, int(stream_frames), generate_opts.get('noise_mode', 'philox'))
    batch_str = f'gen_batched_target{target}_overlap{overlap}' if batched else 'gen_NOT_BATCHED'
    idx = load_path.split('/')[-1].strip().split('.')[0]
    save_str = os.path.join(str(save_path), idx + '_' + batch_str + '_' + 'step={}k'.format(k) + '.wav')
    _ = model.generate(mel, save_str, batched, target, overlap, hp.mu_law, **generate_opts)
    print('\n\nstep = {}'.format(k * 1000))
    return save_str


def _gen_streamed(model: WaveRNN, mel, load_path, save_path, n, noise_mode):
    """--stream-frames N: the mel fed to ``model.stream`` in pushes of N frames, as a TTS front end would hand them over.  The wav is the
    one the unbatched path writes (same seed draw, same audio bit for bit); prints the time to first audio and the real-time factor."""
    if n < 1:
        raise ValueError(f'--stream-frames must be >= 1, got {n}')
    k = model.get_step() // 1000
    idx = load_path.split('/')[-1].strip().split('.')[0]
    save_str = os.path.join(str(save_path), idx + '_gen_NOT_BATCHED_step={}k'.format(k) + '.wav')
    T = mel.size(-1)
    parts, first = [], None
    start = time.perf_counter()
    with model.stream(mu_law=hp.mu_law, noise_mode=noise_mode) as st:
        for f in range(0, T, n):
            parts.append(st.push(mel[0, :, f:f + n]))
            if first is None and parts[-1].size:
                first = time.perf_counter() - start
        parts.append(st.finish())
    wall = time.perf_counter() - start
    if first is None:
        first = wall
    out = np.concatenate(parts)
    save_wav(out, save_str, model.sample_rate)
    model.train()   # what generate() leaves behind (:262)
    secs = out.size / model.sample_rate
    print(f'\nstreamed {T} frames in pushes of {n}: first audio after {first * 1e3:.1f} ms, {wall * 1e3:.1f} ms for {secs:.3f} s of audio '
          f'(real-time factor {wall / max(secs, 1e-9):.4f})')
    print('\n\nstep = {}'.format(k * 1000))
    return save_str


def griffin_lim_from_file(load_path, save_path, n_iter=60, features='vocoder', seed=None, resample=False, trim_top_db=None, peak_norm=None,
                          device=None):
    """``--griffin_lim``: the mel of ``gen_from_file`` -- a ``(T, n_mels)`` ``.npy`` in [0, 1], or the mel of a ``.wav`` through the front end
    -- vocoded by Griffin-Lim on the device (``frontend.GriffinLim``) instead of a model: no checkpoint, no weights.  ``features`` names the
    profile the mel is in.  Writes ``<stem>_griffin_lim.wav`` through ``save_wav`` and returns its path.  The de-emphasis has a gain of
    1 / (1 - k) = 33 at DC, so a wave may leave [-1, 1]: only then is it rescaled, to a peak of 0.999, with one line on stderr."""
    import sys
    from .frontend import GriffinLim, MelFrontEnd
    load_path = str(load_path)
    device = torch.device('cuda') if device is None else torch.device(device)
    if ".npy" in load_path:
        mel = np.load(load_path).T
        if mel.ndim != 2 or mel.shape[0] != hp.num_mels:
            raise ValueError(f'Expected a numpy array shaped (n_mels, n_hops), but got {mel.shape}!')
        _max, _min = np.max(mel), np.min(mel)
        if _max >= 1.01 or _min <= -0.01:
            raise ValueError(f'Expected spectrogram range in [0,1] but was instead [{_min}, {_max}]')
        mel = torch.tensor(mel)
    elif ".wav" in load_path:
        if not os.path.isfile(load_path):
            raise ValueError(f'{load_path}: no such wav file')
        wav = load_wav(load_path, hp.sample_rate, resample=resample, device=device, trim_top_db=trim_top_db, peak_norm=peak_norm, features=features)
        mel = MelFrontEnd(hp, features=features).melspectrogram(wav, device=device)[0]
    else:
        raise ValueError(f"Expected an extension of .wav or .npy, but got {os.path.splitext(load_path)[1]}!")
    gl = GriffinLim(hp, features=features, n_iter=int(n_iter))
    out = gl.reconstruct(mel, seed=seed, device=device)
    wav = out[0, :gl.last_samples[0]].cpu().numpy()
    peak = float(np.abs(wav).max()) if wav.size else 0.0
    if peak > 1.0:
        print(f'griffin_lim: peak {peak:.4g} exceeds 1, rescaled to 0.999', file=sys.stderr)
        wav = wav * np.float32(0.999 / peak)
    idx = load_path.split('/')[-1].strip().split('.')[0]
    save_str = os.path.join(str(save_path), idx + '_griffin_lim.wav')
    save_wav(wav, save_str, hp.sample_rate)
    print(f'\n{n_iter} Griffin-Lim iterations, seed {gl.last_seed}: {wav.size} samples -> {save_str}')
    return save_str


def default_weights_path(base: str = '.') -> str:
    """``Paths(hp.voc_model_id).voc_latest_weights`` of the reference (``wavernn/utils/paths.py:8-12``)."""
    return os.path.join(os.path.abspath(base), 'logs_wavernn', 'checkpoints', 'latest_weights.pyt')


def build_model_from_hparams() -> WaveRNN:
    """``wavernn_gen.py:99-110``."""
    return WaveRNN(rnn_dims=hp.voc_rnn_dims, fc_dims=hp.voc_fc_dims, bits=hp.bits, pad=hp.voc_pad,
                   upsample_factors=hp.voc_upsample_factors, feat_dims=hp.num_mels,
                   compute_dims=hp.voc_compute_dims, res_out_dims=hp.voc_res_out_dims,
                   res_blocks=hp.voc_res_blocks, hop_length=hp.hop_length, sample_rate=hp.sample_rate,
                   mode=hp.voc_mode)


KERNEL_CHOICES = ('auto', 'simple', 'team2', 'batch', 'batch_cs', 'teamg', 'teamg_batch')


def build_parser() -> argparse.ArgumentParser:
    from .hparams import DEFAULT_HPARAMS
    parser = argparse.ArgumentParser(description='Generate WaveRNN Samples')
    parser.add_argument('--batched', '-b', dest='batched', action='store_true', help='Fast Batched Generation')
    parser.add_argument('--unbatched', '-u', dest='batched', action='store_false', help='Slow Unbatched Generation')
    parser.add_argument('--samples', '-s', type=int, help='[int] number of utterances to generate')
    parser.add_argument('--target', '-t', type=lambda s: s if s in ('auto', 'per_xcd') else int(s),
                        help="[int] number of samples in each batch index ('auto': the fold length with the lowest predicted latency on this GPU; "
                             "'per_xcd': one fold per XCD)")
    parser.add_argument('--overlap', '-o', type=int, help='[int] number of crossover samples')
    parser.add_argument('--file', '-f', type=str, help='[string/path] (T, n_mels) .npy mel, or a .wav at the model sample rate (any rate with --resample), to vocode')
    parser.add_argument('--resample', action='store_true',
                        help='extension: resample a --file .wav at another rate to the model sample rate on the device (default: an error)')
    add_condition_arguments(parser, 'a --file .wav')
    add_features_argument(parser, 'a --file .wav')
    parser.add_argument('--voc_weights', '-w', type=str, help='[string/path] Load in different WaveRNN weights')
    parser.add_argument('--gta', '-g', dest='gta', action='store_true', help='Generate from GTA testset')
    parser.add_argument('--force_cpu', '-c', action='store_true',
                        help='accepted for compatibility; this package has no CPU path and will raise')
    parser.add_argument('--noise', choices=['philox', 'reference'], default='philox',
                        help="extension: 'reference' replays the reference's own draws from the torch CPU generator (with --seed: the wav the "
                             "reference script produces after torch.manual_seed(seed)); 'philox' (default) = the device counter RNG")
    parser.add_argument('--seed', type=int, default=None, help='extension: torch.manual_seed(SEED) before generating')
    parser.add_argument('--griffin_lim', type=int, nargs='?', const=60, default=None, metavar='N_ITER',
                        help='extension: vocode --file by N_ITER Griffin-Lim iterations on the device (N_ITER left out: 60) instead of the '
                             'model: no checkpoint is loaded; --features names the profile of the mel, --seed the first phases; writes '
                             '<stem>_griffin_lim.wav (default: off)')
    parser.add_argument('--stream-frames', type=int, default=None, metavar='N',
                        help='extension: feed the mel to a streaming generator in pushes of N frames (unbatched; the same wav as '
                             '--unbatched) and print the time to first audio and the real-time factor')
    parser.add_argument('--hp_file', metavar='FILE', default=DEFAULT_HPARAMS,
                        help='The file to use for the hyperparameters')
    parser.add_argument('--kernel', choices=KERNEL_CHOICES, default='auto',
                        help="extension: the device loop kernel ('auto': the library's choice; 'teamg': the XCD-team kernel for any model "
                             "dims, the fast path of a model whose dims are not the reference hparams; 'teamg_batch': the same kernel with "
                             "several rows per team in lock-step, for batched (fold) mode and other many-row calls of such a model)")
    parser.add_argument('--teamg-weights', choices=('f32', 'f16', 'e4m3'), default='f32',
                        help="extension: element type of the weight image of --kernel teamg / teamg_batch ('f16': the loop matrices as IEEE "
                             "binary16, half the bytes streamed per step; 'e4m3': as 8-bit OCP e4m3 with one power-of-two scale per layer, a "
                             "quarter of the bytes; activations and accumulators stay fp32); ignored by the other kernels")
    parser.add_argument('--teamg-sparse', dest='teamg_sparse', action='store_true',
                        help='extension: --kernel teamg / teamg_batch leave out every block of 64 weights of a row that is all zero (a model '
                             'pruned by wavernn_train.py --sparse-density); same outputs as without; fp32 weights only; ignored by the other kernels')
    parser.set_defaults(batched=None)
    return parser


def main(argv=None):
    args = build_parser().parse_args(argv)

    conditioning = condition_arguments(args)
    hp.configure(args.hp_file)
    if args.target is None:
        args.target = hp.voc_target
    if args.overlap is None:
        args.overlap = hp.voc_overlap
    if args.batched is None:
        args.batched = hp.voc_gen_batched
    if args.samples is None:
        args.samples = hp.voc_gen_at_checkpoint
    if args.force_cpu or not torch.cuda.is_available():
        raise RuntimeError('this vocoder runs on an MI355X only (no CPU path)')

    device = torch.device('cuda')
    print('Using device:', device)
    if args.griffin_lim is not None:
        if not args.file:
            raise ValueError('--griffin_lim vocodes a --file')
        if args.griffin_lim < 0:
            raise ValueError(f'--griffin_lim takes a number of iterations >= 0, got {args.griffin_lim}')
        out_dir = './wavernn_inference_output'
        os.makedirs(out_dir, exist_ok=True)
        griffin_lim_from_file(args.file, out_dir, n_iter=args.griffin_lim, features=args.features, seed=args.seed, resample=args.resample,
                              device=device, **conditioning)
        print('\n\nExiting...\n')
        return
    print('\nInitialising Model...\n')
    model = build_model_from_hparams().to(device)
    from . import _cabi
    model.kernel = _cabi.KERNEL_IDS[args.kernel]
    model.teamg_weights = args.teamg_weights
    model.teamg_sparse = args.teamg_sparse
    # wavernn_gen.py:112-117: `--voc_weights`, else the latest checkpoint of the training run
    # (Paths.voc_latest_weights = <base>/logs_wavernn/checkpoints/latest_weights.pyt, wavernn/utils/paths.py:11-12; <base> is
    # the directory the script is started from here).  The reference then dies in torch.load when that file is absent; no
    # checkpoint ships with the repository (.MISSING_LARGE_BLOBS), so an absent default falls back to the seeded random
    # initialisation, loudly.
    voc_weights = args.voc_weights if args.voc_weights else default_weights_path()
    print(voc_weights)
    if args.voc_weights or os.path.exists(voc_weights):
        model.load(voc_weights)
    else:
        print(f'{voc_weights} does not exist and no --voc_weights given: using the randomly initialised model')
    if args.file:
        out_dir = './wavernn_inference_output'
        os.makedirs(out_dir, exist_ok=True)
        if args.seed is not None:
            torch.manual_seed(args.seed)
        if args.stream_frames is not None and args.noise != 'philox':
            raise ValueError('--stream-frames draws its noise on the device: --noise reference needs the whole clip')
        gen_from_file(model, args.file, out_dir, args.batched, args.target, args.overlap, stream_frames=args.stream_frames,
                      noise_mode=args.noise, resample=args.resample, features=args.features, **conditioning)
    print('\n\nExiting...\n')


if __name__ == "__main__":
    main()
