"""``wavernn_score.py``: rate vocoded audio against a target on the device (``frontend.SpectralScore``, ``csrc/score.hip``).

    wavernn_score.py --target a.wav --test b.wav [--features vocoder|tacotron] [--resample] [--json] [--per_frame out.npz]
    wavernn_score.py --target_dir DIR --test_dir DIR

One line per pair (``mel_lsd_db``: the mean per-frame log-mel distance in dB; ``mcd_db``: the mean mel-cepstral distortion in dB, no
time alignment; ``mr_sc`` / ``mr_logmag``: spectral convergence and log-magnitude distance, averaged over the STFT resolutions) and the
mean over the pairs.  Directory mode pairs the ``*.wav`` files of the two folders by stem; a file without a partner is an error.  Every
pair is compared over the shorter of its two clips.  Files at another sample rate than ``hp.sample_rate`` are an error unless
``--resample``.  The reference has no such tool: its ``gen_testset`` writes the target next to the generated file and stops there."""
from __future__ import annotations

import argparse
import json
from pathlib import Path

import numpy as np

SUMMARY_KEYS = ('mel_lsd_db', 'mcd_db', 'mr_sc', 'mr_logmag')


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


def main(argv=None):
    parser = build_parser()
    args = parser.parse_args(argv)
    try:
        pairs = pair_files(args)
    except ValueError as e:
        parser.error(str(e))
    import torch
    from .frontend import SpectralScore, load_wav
    from .hparams import hparams as hp
    hp.configure(args.hp_file)
    if not torch.cuda.is_available():
        raise RuntimeError('the scores run on an MI355X only (no CPU path)')
    scorer = SpectralScore(hp, features=args.features)
    targets = [load_wav(a, scorer.sample_rate, resample=args.resample) for _, a, _ in pairs]
    tests = [load_wav(b, scorer.sample_rate, resample=args.resample) for _, _, b in pairs]
    scores = scorer.score(targets, tests, per_frame=bool(args.per_frame))
    mean = {k: float(np.mean([s[k] for s in scores])) for k in SUMMARY_KEYS}
    if args.per_frame:
        arrays = {}
        for (name, _, _), s in zip(pairs, scores):
            arrays[f'{name}/lsd'], arrays[f'{name}/mcd'] = s.pop('lsd'), s.pop('mcd')
            for r in s['stft']:
                for q in ('num', 'den', 'lm'):
                    arrays[f"{name}/{q}_{r['n_fft']}_{r['hop']}_{r['win']}"] = r.pop(q)
        np.savez(args.per_frame, **arrays)
    if args.json:
        print(json.dumps(dict(pairs=[dict(s, name=name) for (name, _, _), s in zip(pairs, scores)], mean=mean)))
    else:
        width = max(len(name) for name, _, _ in pairs + [('mean', None, None)])
        print(f"{'clip':<{width}}  {'samples':>9}  {'mel_lsd_db':>10}  {'mcd_db':>10}  {'mr_sc':>10}  {'mr_logmag':>10}")
        for (name, _, _), s in zip(pairs, scores):
            print(f"{name:<{width}}  {s['n']:>9}  {s['mel_lsd_db']:>10.6f}  {s['mcd_db']:>10.6f}  {s['mr_sc']:>10.6f}  {s['mr_logmag']:>10.6f}")
        print(f"{'mean':<{width}}  {'':>9}  {mean['mel_lsd_db']:>10.6f}  {mean['mcd_db']:>10.6f}  {mean['mr_sc']:>10.6f}  {mean['mr_logmag']:>10.6f}")
    return scores


if __name__ == '__main__':
    main()
