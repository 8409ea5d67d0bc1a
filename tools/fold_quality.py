"""Developer tool (GPU): what folding one utterance costs in the spectral scores.

Vocodes one mel unbatched and in the reference's batched mode at three fold densities -- ``target='auto'`` (the latency optimum: a 5 s
clip becomes 64 folds), ``target='per_xcd'`` (one fold per XCD team) and the reference's own 11000 / 550 -- with the same seed, scores
every folded output against the unbatched one (``frontend.SpectralScore``), and lists the per-frame log-mel distance ``lsd`` at and away
from the fold boundaries: a frame is "at a boundary" when its centre ``t hop`` lies inside a crossfade of ``overlap`` samples.
``--pitch`` adds the F0 and voicing errors of every run against the unbatched output (``frontend.PitchScore``): what a cold-started
fold does to the pitch track, which the spectral distances hardly see.

    python tools/fold_quality.py --voc_weights CHECKPOINT.pyt --mel MEL.npy [--seed 1] [--overlap 550] [--pitch]
    python tools/fold_quality.py --frames 401                      # no checkpoint: the repository's seeded random weights, a synthetic mel

WHAT THIS DOES NOT SHOW.  No trained checkpoint ships with this repository.  Without ``--voc_weights`` the model carries seeded random
weights: its output is noise shaped by nothing a listener would call speech, and two samplings of it differ from each other about as
much as a folded output differs from the unbatched one.  Such a run demonstrates the tool, nothing else; it says nothing about the audio
quality of any fold density, and no default (``target='auto'``, ``fold_min_target``) should move because of it.  Even with a trained
checkpoint the sampler is stochastic: a folded output restarts the noise stream in every fold, so the distance to the unbatched output
contains the distance between two samplings of the same mel.  ``--baseline_seed`` prints that distance (unbatched, another seed) next to
the others; a fold density costs quality only where it exceeds that baseline.
"""
from __future__ import annotations

import argparse
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def boundary_frames(n, hop, target, overlap):
    """Boolean mask over the 1 + n // hop mel frames: the frame's centre lies inside a crossfade of the unfolded output.  Fold i >= 1
    fades in over ``[i (target + overlap), i (target + overlap) + overlap)``."""
    centres = np.arange(1 + n // hop) * hop
    pos = centres % (target + overlap)
    return (centres >= target + overlap) & (pos < overlap)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--voc_weights', help='a checkpoint of the configured model (default: seeded random weights, a demonstration only)')
    ap.add_argument('--mel', help='(T, n_mels) .npy mel (default: a synthetic one of --frames frames)')
    ap.add_argument('--frames', type=int, default=401)
    ap.add_argument('--seed', type=int, default=1)
    ap.add_argument('--baseline_seed', type=int, default=2, help='the unbatched output under this seed is scored too: the distance between two samplings')
    ap.add_argument('--overlap', type=int, default=550)
    ap.add_argument('--pitch', action='store_true', help='also report f0_rmse_cents, gpe, vde, ffe, f0_corr and the voiced frame counts of every run')
    ap.add_argument('--hp_file', default=None)
    args = ap.parse_args(argv)
    import torch
    from tacotronv2_wavernn_chinese_amd.frontend import PitchScore, SpectralScore
    from tacotronv2_wavernn_chinese_amd.synth import DEFAULT_DIMS, make_mels, make_state_dict
    from tacotronv2_wavernn_chinese_amd.vocoder import WaveRNN
    if args.voc_weights:
        from tacotronv2_wavernn_chinese_amd.gen import build_model_from_hparams
        from tacotronv2_wavernn_chinese_amd.hparams import DEFAULT_HPARAMS, hparams as hp
        hp.configure(args.hp_file or DEFAULT_HPARAMS)
        model = build_model_from_hparams().to('cuda')
        model.load(args.voc_weights)
        print(f'checkpoint {args.voc_weights}')
    else:
        model = WaveRNN(**DEFAULT_DIMS, mode='RAW')
        model.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in make_state_dict(0, variant='peaky').items()})
        model = model.to('cuda')
        print('NO CHECKPOINT: seeded random weights.  This run demonstrates the tool; it says nothing about audio quality (see the docstring).')
    model.verbose = False
    mel = np.load(args.mel).T.astype(np.float32)[None] if args.mel else make_mels(7, 1, args.frames)
    T, hop = mel.shape[-1], model.hop_length
    scorer = SpectralScore(n_mels=mel.shape[1], hop_length=hop, sample_rate=model.sample_rate)

    def vocode(batched, target, seed):
        torch.manual_seed(seed)
        with tempfile.TemporaryDirectory() as td:
            return model.generate(mel, os.path.join(td, 'x.wav'), batched, target, args.overlap, True).astype(np.float32)

    base = vocode(False, 11000, args.seed)
    n = base.shape[0]
    runs = [('unbatched, another seed', None, vocode(False, 11000, args.baseline_seed))]
    for policy in ('auto', 'per_xcd', 11000):
        target = model.fold_target_for_device(T, args.overlap, policy=policy) if isinstance(policy, str) else policy
        runs.append((f'target={policy!r} -> {target}', target, vocode(True, target, args.seed)))
    print(f'{T} frames, {n} samples, overlap {args.overlap}, seed {args.seed}; every row is scored against the unbatched output of that seed')
    print(f"{'run':<34} {'folds':>5} {'mel_lsd_db':>10} {'mcd_db':>8} {'mr_sc':>8} {'mr_logmag':>9} | {'lsd at boundaries':>26} {'lsd away from them':>26}")
    for name, target, wav in runs:
        s = scorer.score(base, wav, per_frame=True)[0]
        if target is None:
            folds, at, away = 1, 'n/a', f"{s['lsd'].mean():.4f} ({s['lsd'].size} frames)"
        else:
            from tacotronv2_wavernn_chinese_amd.vocoder import fold_count
            mask = boundary_frames(s['n'], hop, target, args.overlap)[:s['lsd'].size]
            folds = fold_count(T * hop, target, args.overlap)
            at = f"{s['lsd'][mask].mean():.4f} ({int(mask.sum())} frames)" if mask.any() else 'none'
            away = f"{s['lsd'][~mask].mean():.4f} ({int((~mask).sum())} frames)" if (~mask).any() else 'none'
        print(f"{name:<34} {folds:>5} {s['mel_lsd_db']:>10.4f} {s['mcd_db']:>8.4f} {s['mr_sc']:>8.4f} {s['mr_logmag']:>9.4f} | {at:>26} {away:>26}")
    if args.pitch:
        pitch = PitchScore(hop=hop, sample_rate=model.sample_rate)
        print()
        print(f"{'run':<34} {'f0_rmse_cents':>13} {'gpe':>8} {'vde':>8} {'ffe':>8} {'f0_corr':>8} {'voiced (unbatched, run, both)':>30}")
        for (name, _, _), p in zip(runs, pitch.score([base] * len(runs), [wav for _, _, wav in runs])):
            voiced = f"{p['voiced_target']}, {p['voiced_test']}, {p['voiced_both']} of {p['frames']}"
            print(f"{name:<34} {p['f0_rmse_cents']:>13.4f} {p['gpe']:>8.4f} {p['vde']:>8.4f} {p['ffe']:>8.4f} {p['f0_corr']:>8.4f} {voiced:>30}")


if __name__ == '__main__':
    main()
