"""python -m ldm.latent_map --config=... --checkpoint_directory=... [--checkpoint N] --out=map.npz
                          [--num_batches 30] [--on logits|embeddings|schedule:T] [--perplexity 30] [--iters 1000]
                          [--seed 0] [--pca 4]

What does a checkpoint's latent space look like?  Encodes --num_batches evaluation batches with the EMA parameters
(Experiment_Colab, get_logits) and writes to one .npz the exact t-SNE map of mulan_amd.latent_maps.latent_map: `Y`
[N, 2], the Kullback-Leibler trace `kl` at the iterations `kl_iter`, `beta` [N], `colour` [N] (the mean gamma at t = 0.5
under each point's embedding), `knn_agreement`, the PCA projection `pca` [N, --pca] of the same points with
`pca_variance_ratio` and `pca_singular_values`, and the run's `settings`.  --on names what is mapped: the encoder's
logits (the reference's plot_tsne_transformation), their hard top-15 embeddings, or the gamma map at time T under each
embedding.  The flags are checked before any device is touched.  One process."""
import json
import logging
import os
import sys

import numpy as np

from mulan_amd.config import Flags
from mulan_amd import checkpoint as ckpt_lib
from ldm.sample import write_npz

NPZ_KEYS = ('Y', 'kl', 'kl_iter', 'beta', 'colour', 'knn_agreement', 'pca', 'pca_variance_ratio', 'pca_singular_values',
            'settings')


def make_flags():
    flags = Flags()
    flags.DEFINE_config_file('config', None, 'Training configuration.')
    flags.DEFINE_string('checkpoint_directory', None, 'Work unit directory.')
    flags.DEFINE_string('checkpoint', None, 'Checkpoint to read (default: the latest).')
    flags.DEFINE_string('out', None, 'Output file (.npz).')
    flags.DEFINE_integer('num_batches', 30, 'Evaluation batches to encode.')
    flags.DEFINE_string('on', 'logits', 'logits / embeddings / schedule:T')
    flags.DEFINE_float('perplexity', 30.0, 'Perplexity of the affinities.')
    flags.DEFINE_integer('iters', 1000, 'Iterations (the first 250, or all if fewer, exaggerated).')
    flags.DEFINE_integer('seed', 0, 'Seed (read by a random init only; the default init is PCA).')
    flags.DEFINE_integer('pca', 4, 'Principal components written beside the map.')
    flags.DEFINE_string('log_level', 'info', 'info/warning/error')
    flags.mark_flags_as_required(['config', 'checkpoint_directory', 'out'])
    return flags


def parse_flags(argv):
    """-> flags or SystemExit: every check that needs no device"""
    from mulan_amd.latent_maps import parse_on
    flags = make_flags().parse(argv)
    if int(os.environ.get('WORLD_SIZE', '1')) > 1:
        raise SystemExit(f"ldm.latent_map runs in one process, WORLD_SIZE = {os.environ['WORLD_SIZE']}")
    try:
        parse_on(flags.on)
    except ValueError as e:
        raise SystemExit(f"--on: {e}") from None
    if flags.num_batches < 1:
        raise SystemExit(f"--num_batches must be >= 1, got {flags.num_batches}")
    if not flags.perplexity >= 1.0:
        raise SystemExit(f"--perplexity must be >= 1, got {flags.perplexity}")
    if flags.iters < 1:
        raise SystemExit(f"--iters must be >= 1, got {flags.iters}")
    if flags.seed < 0:
        raise SystemExit(f"--seed must be >= 0, got {flags.seed}")
    if flags.pca < 1:
        raise SystemExit(f"--pca must be >= 1, got {flags.pca}")
    if not flags.out.endswith('.npz'):
        raise SystemExit(f"--out must name a .npz file, got {flags.out!r}")
    if flags.config.get('vdm_type', 'vdm') == 'vdm':
        raise SystemExit("the latent map needs a MuLAN model (vdm_type mulan_velocity / mulan_epsilon)")
    if not ckpt_lib.checkpoint_numbers(flags.checkpoint_directory):
        raise SystemExit(f'no ckpt-* files in {flags.checkpoint_directory}')
    return flags


def run(experiment, flags):
    """the arrays of the output file, `settings` as a dict"""
    from mulan_amd import latent_maps as lm
    res = lm.latent_map(experiment, num_batches=flags.num_batches, on=flags.on, perplexity=flags.perplexity,
                        n_iter=flags.iters, exaggeration_iter=min(250, flags.iters), seed=flags.seed)
    arrays = {k: np.asarray(res[k]) for k in ('Y', 'kl', 'kl_iter', 'beta', 'colour', 'knn_agreement')}
    points = res.pop("points")
    pca, ratio, values = lm.pca_transformation(points, min(flags.pca, *points.shape), return_stats=True)
    arrays.update(pca=pca, pca_variance_ratio=ratio, pca_singular_values=values)
    return arrays, dict(res["settings"], on=flags.on, num_batches=flags.num_batches)


def main(argv):
    flags = parse_flags(argv)
    logging.basicConfig(level=getattr(logging, flags.log_level.upper()))
    from mulan_amd import evaluators as ev
    ckpt_nums = ckpt_lib.checkpoint_numbers(flags.checkpoint_directory)
    ckpt_num = ckpt_nums[-1] if flags.checkpoint is None else flags.checkpoint
    experiment = ev.Experiment_Colab(flags.config, flags.checkpoint_directory, ckpt_num)
    arrays, settings = run(experiment, flags)
    settings.update(checkpoint=str(ckpt_num), vdm_type=flags.config.get('vdm_type', 'vdm'))
    write_npz(flags.out, dict(arrays, settings=np.array(json.dumps(settings, sort_keys=True))))
    print(f"wrote the map of {arrays['Y'].shape[0]} latents ({flags.on}) to {flags.out}: KL {float(arrays['kl'][0]):.4f} -> "
          f"{float(arrays['kl'][-1]):.4f}, 10-nearest-neighbour agreement {float(arrays['knn_agreement']):.3f}")
    return 0


if __name__ == '__main__':
    main(sys.argv[1:])
