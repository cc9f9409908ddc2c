"""python -m ldm.schedules --config=... --checkpoint_directory=... [--checkpoint N] --out=schedules.npz
                         [--num_batches 30] [--timesteps 128] [--bins 100]
                         [--embedding encoder|deterministic|shift:K] [--keep_curves 3]

Writes what a checkpoint's EMA parameters (Experiment_Colab) have learned as a noise schedule to one .npz: the summaries
of mulan_amd.evaluators.noise_schedule_summary over E embeddings and --timesteps times uniform in [0, 1] (`mean`, `std`,
`min`, `max`, `sigma2_mean` [E, T], `channel_mean` [E, T, 3], `hist` [E, T, bins], `time_steps` [T], `between` [T]), the
`embeddings` [E, latent_size], `curves` ([keep_curves, T, 3072]: every sub-pixel's gamma under the first --keep_curves
embeddings) and the run's `settings`.  Not in the reference, whose notebook draws these and keeps nothing.

--embedding names the embeddings: `encoder` (the default) the hard top-15 of the encoder's logits over --num_batches
evaluation batches (get_logits, logits_to_embeddings); `deterministic` the one embedding the samplers use by default;
`shift:K` the K embeddings get_embedding(1, shift=k), k = 0 .. K - 1.  The flags are checked before any device is
touched.  One process: the work is a few launches."""
import json
import logging
import sys

import numpy as np

from mulan_amd.config import Flags
from mulan_amd import checkpoint as ckpt_lib
from ldm.sample import write_npz

SUMMARY_KEYS = ('mean', 'std', 'min', 'max', 'sigma2_mean', 'channel_mean', 'hist', 'time_steps', 'between')
NPZ_KEYS = SUMMARY_KEYS + ('embeddings', 'curves', 'settings')


def make_flags():
    flags = Flags()
    flags.DEFINE_config_file('config', None, 'Training configuration.')
    flags.DEFINE_string('checkpoint_directory', None, 'Work unit directory.')
    flags.DEFINE_string('checkpoint', None, 'Checkpoint to read (default: the latest).')
    flags.DEFINE_string('out', None, 'Output file (.npz).')
    flags.DEFINE_integer('num_batches', 30, '--embedding=encoder: evaluation batches to encode.')
    flags.DEFINE_integer('timesteps', 128, 'Times, uniform in [0, 1] with both ends.')
    flags.DEFINE_integer('bins', 100, 'Histogram bins over [gamma_min, gamma_max], 1..256.')
    flags.DEFINE_string('embedding', 'encoder', 'encoder / deterministic / shift:K')
    flags.DEFINE_integer('keep_curves', 3, 'Embeddings whose full curves are written.')
    flags.DEFINE_string('log_level', 'info', 'info/warning/error')
    flags.mark_flags_as_required(['config', 'checkpoint_directory', 'out'])
    return flags


def parse_embedding(spec):
    """-> ('encoder' | 'deterministic', None) or ('shift', K) or ValueError"""
    if spec in ('encoder', 'deterministic'):
        return spec, None
    if spec.startswith('shift:') and spec[6:].isdigit() and int(spec[6:]) >= 1:
        return 'shift', int(spec[6:])
    raise ValueError(f"{spec!r} is not encoder, deterministic or shift:K with K >= 1")


def parse_flags(argv):
    """-> flags or SystemExit: every check that needs no device"""
    flags = make_flags().parse(argv)
    try:
        parse_embedding(flags.embedding)
    except ValueError as e:
        raise SystemExit(f"--embedding: {e}") from None
    if flags.num_batches < 1:
        raise SystemExit(f"--num_batches must be >= 1, got {flags.num_batches}")
    if flags.timesteps < 1:
        raise SystemExit(f"--timesteps must be >= 1, got {flags.timesteps}")
    if not 1 <= flags.bins <= 256:
        raise SystemExit(f"--bins must lie in 1..256, got {flags.bins}")
    if flags.keep_curves < 0:
        raise SystemExit(f"--keep_curves must be >= 0, got {flags.keep_curves}")
    if not flags.out.endswith('.npz'):
        raise SystemExit(f"--out must name a .npz file, got {flags.out!r}")
    if flags.config.get('vdm_type', 'vdm') == 'vdm':
        raise SystemExit("the schedule per embedding needs a MuLAN model (vdm_type mulan_velocity / mulan_epsilon)")
    if not ckpt_lib.checkpoint_numbers(flags.checkpoint_directory):
        raise SystemExit(f'no ckpt-* files in {flags.checkpoint_directory}')
    return flags


def embeddings_of(experiment, flags):
    """the [E, latent_size] embeddings --embedding names, on the experiment's device"""
    from mulan_amd import evaluators as ev
    kind, K = parse_embedding(flags.embedding)
    if kind == 'encoder':
        logits, _ = ev.get_logits(experiment, flags.num_batches)
        return ev.logits_to_embeddings(logits)
    if kind == 'deterministic':
        return experiment.model.deterministic_embedding(1, experiment.device)
    L = experiment.model.config.latent_size
    import torch
    return torch.cat([ev.get_embedding(1, L, shift=k) for k in range(K)]).to(experiment.device)


def run(experiment, flags):
    """the arrays of the output file"""
    from mulan_amd import evaluators as ev
    emb = embeddings_of(experiment, flags)
    t = np.linspace(0.0, 1.0, flags.timesteps)
    summary = ev.noise_schedule_summary(experiment, emb, t, bins=flags.bins)
    keep = min(flags.keep_curves, emb.shape[0])
    curves = ev.noise_schedule_per_embedding(experiment, emb[:keep], t) if keep else []
    arrays = {k: summary[k] for k in SUMMARY_KEYS}
    arrays['embeddings'] = emb.cpu().numpy()
    arrays['curves'] = np.stack(curves) if keep else np.zeros((0, flags.timesteps, 3072), dtype=np.float32)
    return arrays


def main(argv):
    flags = parse_flags(argv)
    logging.basicConfig(level=getattr(logging, flags.log_level.upper()))
    from mulan_amd.evaluators import Experiment_Colab
    ckpt_nums = ckpt_lib.checkpoint_numbers(flags.checkpoint_directory)
    ckpt_num = ckpt_nums[-1] if flags.checkpoint is None else flags.checkpoint
    experiment = Experiment_Colab(flags.config, flags.checkpoint_directory, ckpt_num)
    arrays = run(experiment, flags)
    if experiment.rank == 0:
        settings = dict(checkpoint=str(ckpt_num), vdm_type=flags.config.get('vdm_type', 'vdm'), embedding=flags.embedding,
                        num_batches=flags.num_batches, timesteps=flags.timesteps, bins=flags.bins,
                        keep_curves=int(arrays['curves'].shape[0]), n_embeddings=int(arrays['embeddings'].shape[0]))
        write_npz(flags.out, dict(arrays, settings=np.array(json.dumps(settings, sort_keys=True))))
        print(f"wrote the schedules of {settings['n_embeddings']} embeddings at {flags.timesteps} times to {flags.out}")
    return 0


if __name__ == '__main__':
    main(sys.argv[1:])
