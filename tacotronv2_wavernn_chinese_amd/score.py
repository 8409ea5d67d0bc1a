"""``wavernn_score.py``: rate vocoded audio against a target on the device (``frontend.SpectralScore``, ``csrc/score.hip``).

    wavernn_score.py --target a.wav --test b.wav [--features vocoder|tacotron] [--resample] [--json] [--per_frame out.npz]
    wavernn_score.py --target_dir DIR --test_dir DIR
    wavernn_score.py ... --pitch [--fmin HZ] [--fmax HZ] [--pitch_threshold X]
    wavernn_score.py ... --align [--pitch]

One line per pair (``mel_lsd_db``: the mean per-frame log-mel distance in dB; ``mcd_db``: the mean mel-cepstral distortion in dB, no
time alignment; ``mr_sc`` / ``mr_logmag``: spectral convergence and log-magnitude distance, averaged over the STFT resolutions) and the
mean over the pairs.  Directory mode pairs the ``*.wav`` files of the two folders by stem; a file without a partner is an error.  Every
pair is compared over the shorter of its two clips.  Files at another sample rate than ``hp.sample_rate`` are an error unless
``--resample``.  ``--pitch`` adds the F0 and voicing errors of ``frontend.PitchScore`` (``csrc/pitch.hip``) to every pair and to the
mean: ``f0_rmse_cents``, ``gpe``, ``vde``, ``ffe``, ``f0_corr`` and the voiced frame counts; without it the output is what it was before
the flag existed.  ``--align`` is for pairs that are NOT sample-aligned (a trimmed clip, a rendering of a predicted mel against the
recording, two takes of a sentence): the clips keep their own lengths and are rated along the dynamic-time-warping path over their mel
cepstra (``frontend.AlignedScore``, ``csrc/align.hip``): ``mcd_dtw_db``, ``mel_lsd_dtw_db``, the path's length and total cost and,
with ``--pitch``, the F0 and voicing errors along the path; the frame-for-frame scores are not printed then, and ``--per_frame`` stores
the paths and the values along them.  The reference has no such tool: its ``gen_testset`` writes the target next to the generated file and stops there."""
from __future__ import annotations

import argparse
import json
from pathlib import Path

import numpy as np

SUMMARY_KEYS = ('mel_lsd_db', 'mcd_db', 'mr_sc', 'mr_logmag')
ALIGN_KEYS = ('total_cost', 'path_len', 'frames_target', 'frames_test', 'mcd_dtw_db', 'mel_lsd_dtw_db')   # _cabi.ALIGN_FIELD_NAMES[:6]
ALIGN_PITCH_KEYS = ('f0_rmse_cents', 'gpe', 'vde', 'ffe', 'f0_corr', 'voiced_both')                    # _cabi.ALIGN_FIELD_NAMES[6:]
PITCH_KEYS = ('f0_rmse_cents', 'gpe', 'vde', 'ffe', 'f0_corr', 'voiced_target', 'voiced_test', 'voiced_both')   # _cabi.PITCH_FIELD_NAMES


def build_parser() -> argparse.ArgumentParser:
    from .frontend import add_features_argument
    from .hparams import DEFAULT_HPARAMS
    parser = argparse.ArgumentParser(description='Spectral scores of test wavs against target wavs, on the device')
    parser.add_argument('--target', metavar='WAV', help='the target clip')
    parser.add_argument('--test', metavar='WAV', help='the clip to rate against it')
    parser.add_argument('--target_dir', metavar='DIR', help='a folder of target *.wav files ...')
    parser.add_argument('--test_dir', metavar='DIR', help='... and the folder of the clips to rate, paired with them by file stem')
    add_features_argument(parser, 'the mel scores')
    parser.add_argument('--resample', action='store_true', help='resample files at another rate to hp.sample_rate on the device (default: such a '
                                                                'file is an error)')
    parser.add_argument('--json', action='store_true', help='print one JSON object (pairs, mean) instead of the table')
    parser.add_argument('--per_frame', metavar='NPZ', help='also write the per-frame arrays of every pair to this .npz file')
    parser.add_argument('--pitch', action='store_true', help='also report the F0 and voicing errors (a YIN track of both clips on the device)')
    parser.add_argument('--align', action='store_true', help='rate every pair along the dynamic-time-warping path over the mel cepstra instead of '
                                                             'frame for frame: for pairs that are not sample-aligned (the clips keep their own lengths)')
    parser.add_argument('--fmin', type=float, default=None, metavar='HZ', help='the lowest pitch the tracker looks for (default 60)')
    parser.add_argument('--fmax', type=float, default=None, metavar='HZ', help='the highest pitch the tracker looks for (default 600)')
    parser.add_argument('--pitch_threshold', type=float, default=None, metavar='X', help="YIN's threshold on the normalised difference "
                                                                                          '(default 0.15)')
    parser.add_argument('--hp_file', metavar='FILE', default=DEFAULT_HPARAMS, help='The file to use for the hyperparameters')
    return parser


def pair_files(args):
    """[(name, target path, test path)] of the arguments; ``ValueError`` for a mixed or incomplete set, or folders that do not pair up."""
    single, folder = (args.target, args.test), (args.target_dir, args.test_dir)
    if all(single) and not any(folder):
        return [(Path(args.test).stem, Path(args.target), Path(args.test))]
    if all(folder) and not any(single):
        a = {p.stem: p for p in sorted(Path(args.target_dir).expanduser().glob('*.wav'))}
        b = {p.stem: p for p in sorted(Path(args.test_dir).expanduser().glob('*.wav'))}
        if not a:
            raise ValueError(f'no *.wav files in {args.target_dir}')
        if set(a) != set(b):
            raise ValueError(f'the folders do not pair up by stem: without a partner {sorted(set(a) ^ set(b))}')
        return [(s, a[s], b[s]) for s in sorted(a)]
    raise ValueError('give --target and --test, or --target_dir and --test_dir')


def pitch_settings(args) -> dict:
    """The ``PitchScore`` settings the arguments name; ``ValueError`` for tracker settings without ``--pitch``."""
    given = {k: v for k, v in (('fmin', args.fmin), ('fmax', args.fmax), ('threshold', args.pitch_threshold)) if v is not None}
    if given and not args.pitch:
        raise ValueError('--fmin, --fmax and --pitch_threshold belong to --pitch')
    return given


def table(names, scores, mean, pitch_hop=None) -> str:
    """The table the command prints without ``--json``: one line per pair and the mean; with ``pitch_hop`` (the tracker's hop, under
    ``--pitch``) a second table of the pitch fields after an empty line."""
    width = max(len(name) for name in list(names) + ['mean'])
    lines = [f"{'clip':<{width}}  {'samples':>9}  {'mel_lsd_db':>10}  {'mcd_db':>10}  {'mr_sc':>10}  {'mr_logmag':>10}"]
    for name, s in zip(names, scores):
        lines.append(f"{name:<{width}}  {s['n']:>9}  {s['mel_lsd_db']:>10.6f}  {s['mcd_db']:>10.6f}  {s['mr_sc']:>10.6f}  {s['mr_logmag']:>10.6f}")
    lines.append(f"{'mean':<{width}}  {'':>9}  {mean['mel_lsd_db']:>10.6f}  {mean['mcd_db']:>10.6f}  {mean['mr_sc']:>10.6f}  {mean['mr_logmag']:>10.6f}")
    if pitch_hop is not None:
        lines += ['', f"{'clip':<{width}}  {'frames':>9}  {'f0_rmse_cents':>13}  {'gpe':>8}  {'vde':>8}  {'ffe':>8}  {'f0_corr':>8}  "
                      f"{'voiced (target, test, both)':>27}"]
        for name, frames, s in [(name, str(1 + s['n'] // pitch_hop), s) for name, s in zip(names, scores)] + [('mean', '', mean)]:
            voiced = f"{s['voiced_target']:g}, {s['voiced_test']:g}, {s['voiced_both']:g}"
            lines.append(f"{name:<{width}}  {frames:>9}  {s['f0_rmse_cents']:>13.4f}  {s['gpe']:>8.4f}  {s['vde']:>8.4f}  {s['ffe']:>8.4f}  "
                         f"{s['f0_corr']:>8.4f}  {voiced:>27}")
    return '\n'.join(lines)


def align_table(names, scores, mean, pitch) -> str:
    """The table ``--align`` prints without ``--json``: one line per pair and the mean; under ``--pitch`` the fields along the path too."""
    width = max(len(name) for name in list(names) + ['mean'])
    head = f"{'clip':<{width}}  {'frames (target, test)':>21}  {'path_len':>8}  {'mcd_dtw_db':>10}  {'mel_lsd_dtw_db':>14}"
    if pitch:
        head += f"  {'f0_rmse_cents':>13}  {'gpe':>8}  {'vde':>8}  {'ffe':>8}  {'f0_corr':>8}  {'voiced_both':>11}"
    lines = [head]
    for name, s in list(zip(names, scores)) + [('mean', mean)]:
        line = (f"{name:<{width}}  {format(s['frames_target'], 'g') + ', ' + format(s['frames_test'], 'g'):>21}  {s['path_len']:>8g}  "
                f"{s['mcd_dtw_db']:>10.6f}  {s['mel_lsd_dtw_db']:>14.6f}")
        if pitch:
            line += f"  {s['f0_rmse_cents']:>13.4f}  {s['gpe']:>8.4f}  {s['vde']:>8.4f}  {s['ffe']:>8.4f}  {s['f0_corr']:>8.4f}  {s['voiced_both']:>11g}"
        lines.append(line)
    return '\n'.join(lines)


def main_align(args, parser, pairs, pitch_kw, hp):
    """``--align``: every pair along its DTW path, the clips at their own lengths."""
    from .frontend import AlignedScore, load_wav
    try:
        scorer = AlignedScore(hp, features=args.features, pitch=args.pitch, **{('pitch_' + k if k in ('fmin', 'fmax') else k): v for k, v in pitch_kw.items()})
    except ValueError as e:
        parser.error(str(e))
    targets = [load_wav(a, scorer.sample_rate, resample=args.resample) for _, a, _ in pairs]
    tests = [load_wav(b, scorer.sample_rate, resample=args.resample) for _, _, b in pairs]
    res = scorer.score(targets, tests, per_path=bool(args.per_frame))
    keys = ALIGN_KEYS + (ALIGN_PITCH_KEYS if args.pitch else ())
    counts = ('path_len', 'frames_target', 'frames_test', 'voiced_both')
    scores = []
    for b in range(len(pairs)):
        s = {k: (int(res[k][b]) if k in counts else float(res[k][b])) for k in keys}
        s.update(n_target=res['n_target'][b], n_test=res['n_test'][b])
        scores.append(s)
    mean = {k: float(np.mean([s[k] for s in scores])) for k in keys}
    if args.per_frame:
        arrays = {}
        for b, (name, _, _) in enumerate(pairs):
            for k in ('path', 'lsd', 'cents') + (('f0_target', 'f0_test') if args.pitch else ()):
                arrays[f'{name}/{k}'] = res[k][b].numpy()
        np.savez(args.per_frame, **arrays)
    if args.json:
        print(json.dumps(dict(pairs=[dict(s, name=name) for (name, _, _), s in zip(pairs, scores)], mean=mean)))
    else:
        print(align_table([name for name, _, _ in pairs], scores, mean, args.pitch))
    return scores


def main(argv=None):
    parser = build_parser()
    args = parser.parse_args(argv)
    try:
        pairs = pair_files(args)
        pitch_kw = pitch_settings(args)
    except ValueError as e:
        parser.error(str(e))
    import torch
    from .frontend import PitchScore, SpectralScore, load_wav
    from .hparams import hparams as hp
    hp.configure(args.hp_file)
    if not torch.cuda.is_available():
        raise RuntimeError('the scores run on an MI355X only (no CPU path)')
    if args.align:
        return main_align(args, parser, pairs, pitch_kw, hp)
    scorer = SpectralScore(hp, features=args.features)
    try:
        pitch = PitchScore(hp, **pitch_kw) if args.pitch else None
    except ValueError as e:
        parser.error(str(e))
    targets = [load_wav(a, scorer.sample_rate, resample=args.resample) for _, a, _ in pairs]
    tests = [load_wav(b, scorer.sample_rate, resample=args.resample) for _, _, b in pairs]
    scores = scorer.score(targets, tests, per_frame=bool(args.per_frame))
    keys = SUMMARY_KEYS
    if pitch is not None:
        keys = SUMMARY_KEYS + PITCH_KEYS
        for s, p in zip(scores, pitch.score(targets, tests, per_frame=bool(args.per_frame))):
            s.update({k: p[k] for k in PITCH_KEYS})
            if args.per_frame:
                s['pitch_frames'] = {k: p[k] for k in ('f0_target', 'aperiodicity_target', 'f0_test', 'aperiodicity_test', 'cents')}
    mean = {k: float(np.mean([s[k] for s in scores])) for k in keys}
    if args.per_frame:
        arrays = {}
        for (name, _, _), s in zip(pairs, scores):
            arrays[f'{name}/lsd'], arrays[f'{name}/mcd'] = s.pop('lsd'), s.pop('mcd')
            for r in s['stft']:
                for q in ('num', 'den', 'lm'):
                    arrays[f"{name}/{q}_{r['n_fft']}_{r['hop']}_{r['win']}"] = r.pop(q)
            for k, v in s.pop('pitch_frames', {}).items():
                arrays[f'{name}/{k}'] = v
        np.savez(args.per_frame, **arrays)
    if args.json:
        print(json.dumps(dict(pairs=[dict(s, name=name) for (name, _, _), s in zip(pairs, scores)], mean=mean)))
    else:
        print(table([name for name, _, _ in pairs], scores, mean, pitch.hop if pitch is not None else None))
    return scores


if __name__ == '__main__':
    main()
