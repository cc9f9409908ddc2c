"""python -m ldm.sample --config=... --checkpoint_directory=... [--checkpoint N] --n_samples=N --out=FILE.npz
                      [--sampler dpm2m|sde2m|ddim|ancestral] [--eta 0.0] [--steps 25] [--batch_size B]
                      [--embedding deterministic|random] [--seed 0]

Writes a set of samples of a checkpoint's EMA parameters (Experiment_Colab) to one .npz: `images` (uint8
[n_samples, 32, 32, 3]) and the run's settings.  Not in the reference, which writes image grids only.  Global batch b
is drawn from PRNGKey(seed).fold_in(b) alone (the step noise of sde2m and of ddim with --eta > 0 from the third of its
three sub-keys, folded with the step index: Experiment_Colab.sample_batches); under torchrun the batches are dealt
round-robin to the ranks and rank 0 writes the file, so for a fixed --batch_size the file does not depend on the number
of ranks.  The flags are checked before any device is touched."""
import io
import json
import logging
import math
import os
import sys
import zipfile

import numpy as np

from mulan_amd.config import Flags
from mulan_amd import checkpoint as ckpt_lib
from mulan_amd.sampling import SAMPLERS

EMBEDDINGS = ('deterministic', 'random')


def make_flags():
    flags = Flags()
    flags.DEFINE_config_file('config', None, 'Training configuration.')
    flags.DEFINE_string('checkpoint_directory', None, 'Work unit directory.')
    flags.DEFINE_string('checkpoint', None, 'Checkpoint to sample from (default: the latest).')
    flags.DEFINE_string('sampler', 'dpm2m', 'dpm2m / sde2m / ddim / ancestral')
    flags.DEFINE_float('eta', 0.0, 'ddim only: 0 deterministic .. 1 the ancestral posterior step, in [0, 1].')
    flags.DEFINE_integer('steps', 25, 'Number of sampling steps (network evaluations per batch).')
    flags.DEFINE_integer('n_samples', None, 'Number of images to write.')
    flags.DEFINE_integer('batch_size', None, 'Images per batch (default: config.training.batch_size_eval).')
    flags.DEFINE_string('embedding', 'deterministic', 'deterministic / random latent embedding of the MuLAN models.')
    flags.DEFINE_integer('seed', 0, 'Global batch b is drawn from PRNGKey(seed).fold_in(b).')
    flags.DEFINE_string('out', None, 'Output file (.npz).')
    flags.DEFINE_string('log_level', 'info', 'info/warning/error')
    flags.mark_flags_as_required(['config', 'checkpoint_directory', 'n_samples', 'out'])
    return flags


def parse_flags(argv):
    """-> (flags, batch_size) or SystemExit: every check that needs no device"""
    flags = make_flags().parse(argv)
    if flags.sampler not in SAMPLERS:
        raise SystemExit(f"unknown --sampler {flags.sampler!r} (one of {', '.join(SAMPLERS)})")
    if not 0.0 <= flags.eta <= 1.0:
        raise SystemExit(f"--eta must lie in [0, 1], got {flags.eta!r}")
    if flags.eta != 0.0 and flags.sampler != 'ddim':
        raise SystemExit(f"--eta applies to --sampler=ddim; {flags.sampler!r} takes none")
    if flags.embedding not in EMBEDDINGS:
        raise SystemExit(f"unknown --embedding {flags.embedding!r} (one of {', '.join(EMBEDDINGS)})")
    if flags.steps < 1:
        raise SystemExit(f"--steps must be >= 1, got {flags.steps}")
    if flags.n_samples < 1:
        raise SystemExit(f"--n_samples must be >= 1, got {flags.n_samples}")
    batch_size = flags.batch_size if flags.batch_size is not None else int(flags.config.training.batch_size_eval)
    if batch_size < 1:
        raise SystemExit(f"--batch_size must be >= 1, got {batch_size}")
    if not flags.out.endswith('.npz'):
        raise SystemExit(f"--out must name a .npz file, got {flags.out!r}")
    if flags.embedding == 'random' and flags.config.get('vdm_type', 'vdm') == 'vdm':
        raise SystemExit("--embedding=random needs a MuLAN model (vdm_type mulan_velocity / mulan_epsilon)")
    if not ckpt_lib.checkpoint_numbers(flags.checkpoint_directory):
        raise SystemExit(f'no ckpt-* files in {flags.checkpoint_directory}')
    return flags, batch_size


def write_npz(path, arrays):
    """np.savez with fixed zip entry times: the same arrays give the same bytes"""
    tmp = path + '.tmp'
    with zipfile.ZipFile(tmp, 'w', compression=zipfile.ZIP_STORED) as zf:
        for name, value in arrays.items():
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(value), allow_pickle=False)
            zf.writestr(zipfile.ZipInfo(name + '.npy', date_time=(1980, 1, 1, 0, 0, 0)), buf.getvalue())
    os.replace(tmp, path)


def main(argv):
    flags, batch_size = parse_flags(argv)
    rank = int(os.environ.get("RANK", "0"))
    logging.basicConfig(level=getattr(logging, flags.log_level.upper()) if rank == 0 else logging.ERROR)
    import torch
    from mulan_amd import parallel
    from mulan_amd.evaluators import Experiment_Colab
    from mulan_amd.rng import PRNGKey
    ckpt_nums = ckpt_lib.checkpoint_numbers(flags.checkpoint_directory)
    ckpt_num = ckpt_nums[-1] if flags.checkpoint is None else flags.checkpoint
    experiment = Experiment_Colab(flags.config, flags.checkpoint_directory, ckpt_num)
    world, rank = experiment.world, experiment.rank
    n_batches = math.ceil(flags.n_samples / batch_size)
    mine = list(range(rank, n_batches, world))
    per_rank = math.ceil(n_batches / world)
    root = PRNGKey(flags.seed)
    images = experiment.sample_batches([root.fold_in(b) for b in mine], batch_size, flags.embedding, flags.sampler,
                                       flags.steps, flags.eta)
    local = torch.zeros((per_rank, batch_size, 32, 32, 3), dtype=torch.uint8, device=experiment.device)
    for j, x in enumerate(images):
        local[j].copy_(x)
    gathered = parallel.all_gather_tensor(local[None]).cpu().numpy()       # [world, per_rank, B, 32, 32, 3]
    if rank == 0:
        ordered = np.stack([gathered[b % world, b // world] for b in range(n_batches)])
        out = ordered.reshape(-1, 32, 32, 3)[:flags.n_samples]
        settings = dict(sampler=flags.sampler, eta=float(flags.eta), steps=flags.steps, n_samples=flags.n_samples,
                        batch_size=batch_size, embedding=flags.embedding, seed=flags.seed, checkpoint=str(ckpt_num),
                        vdm_type=flags.config.get('vdm_type', 'vdm'))
        write_npz(flags.out, dict(images=out, settings=np.array(json.dumps(settings, sort_keys=True))))
        print(f'wrote {out.shape[0]} samples ({flags.sampler}, {flags.steps} steps) to {flags.out}')
    return 0


if __name__ == '__main__':
    main(sys.argv[1:])
