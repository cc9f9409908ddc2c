"""python -m ldm.bound_profile --config=... --checkpoint_directory=... [--checkpoint N] --out=profile.npz
                             [--n_images 16] [--timesteps 128] [--keep_pixels 16]

Writes where the bits of the variational bound come from, for the first --n_images test images under a checkpoint's EMA
parameters (Experiment_Colab), to one .npz: the arrays of mulan_amd.evaluators.bound_profile -- per image and row `t`,
`diff`, `recon`, `klz`, `resid2`, `weight` [N, T] and `diff_channel` [N, T, 3]; per image `kl_z`, `bpd`, `diff_std` [N]
-- the sub-pixel maps `diff_pixel`, `recon_pixel`, `klz_pixel` ([keep_pixels, 3072], of the first --keep_pixels images)
and their means over all N images (`diff_pixel_mean`, `recon_pixel_mean`, `klz_pixel_mean` [3072]), the `images` (uint8
[N, 32, 32, 3]) and the run's `settings`.  Every image is scored as eval_bpd --bpd_eval_method=dense scores it: --timesteps
copies under PRNGKey(0).  Not in the reference.  The flags are checked before any device is touched.  One process."""
import json
import logging
import sys

import numpy as np

from mulan_amd.config import Flags
from mulan_amd import checkpoint as ckpt_lib
from ldm.sample import write_npz

ROW_KEYS = ('t', 'diff', 'diff_channel', 'recon', 'klz', 'kl_z', 'resid2', 'weight', 'bpd', 'diff_std')
PIXEL_KEYS = ('diff_pixel', 'recon_pixel', 'klz_pixel')
NPZ_KEYS = ROW_KEYS + PIXEL_KEYS + tuple(k + '_mean' for k in PIXEL_KEYS) + ('images', 'settings')


def make_flags():
    flags = Flags()
    flags.DEFINE_config_file('config', None, 'Training configuration.')
    flags.DEFINE_string('checkpoint_directory', None, 'Work unit directory.')
    flags.DEFINE_string('checkpoint', None, 'Checkpoint to read (default: the latest).')
    flags.DEFINE_string('out', None, 'Output file (.npz).')
    flags.DEFINE_integer('n_images', 16, 'Test images to profile, from the start of the test split.')
    flags.DEFINE_integer('timesteps', 128, 'Copies of each image: the rows of the antithetic time grid.')
    flags.DEFINE_integer('keep_pixels', 16, 'Images whose sub-pixel maps are written (their means always are).')
    flags.DEFINE_string('log_level', 'info', 'info/warning/error')
    flags.mark_flags_as_required(['config', 'checkpoint_directory', 'out'])
    return flags


def parse_flags(argv):
    """-> flags or SystemExit: every check that needs no device"""
    flags = make_flags().parse(argv)
    if flags.n_images < 1:
        raise SystemExit(f"--n_images must be >= 1, got {flags.n_images}")
    if flags.timesteps < 1:
        raise SystemExit(f"--timesteps must be >= 1, got {flags.timesteps}")
    if flags.keep_pixels < 0:
        raise SystemExit(f"--keep_pixels must be >= 0, got {flags.keep_pixels}")
    if not flags.out.endswith('.npz'):
        raise SystemExit(f"--out must name a .npz file, got {flags.out!r}")
    if not ckpt_lib.checkpoint_numbers(flags.checkpoint_directory):
        raise SystemExit(f'no ckpt-* files in {flags.checkpoint_directory}')
    return flags


def eval_images(experiment, config, n_images):
    """uint8 [N, 32, 32, 3]: the first n_images of the test split (fewer if it is shorter)"""
    import torch
    from mulan_amd import data as dataset
    images = []
    for batch in dataset.create_one_time_eval_dataset(config, 1, experiment.device, 0, 1):
        images.append(batch['images'].reshape(1, 32, 32, 3))
        if len(images) == n_images:
            break
    return torch.cat(images)


def run(experiment, flags, checkpoint=None):
    """the arrays of the output file: every key of NPZ_KEYS"""
    from mulan_amd import evaluators as ev
    images = eval_images(experiment, flags.config, flags.n_images)
    profile = ev.bound_profile(experiment, images, n_timesteps=flags.timesteps)
    arrays = {k: profile[k] for k in ROW_KEYS}
    for k in PIXEL_KEYS:
        arrays[k] = profile[k][:flags.keep_pixels]
        arrays[k + '_mean'] = profile[k].mean(axis=0)
    arrays['images'] = images.cpu().numpy()
    settings = dict(checkpoint=str(checkpoint), vdm_type=flags.config.get('vdm_type', 'vdm'), timesteps=flags.timesteps,
                    n_images=int(images.shape[0]), keep_pixels=int(arrays['diff_pixel'].shape[0]))
    arrays['settings'] = np.array(json.dumps(settings, sort_keys=True))
    return arrays


def main(argv):
    flags = parse_flags(argv)
    logging.basicConfig(level=getattr(logging, flags.log_level.upper()))
    from mulan_amd.evaluators import Experiment_Colab
    ckpt_nums = ckpt_lib.checkpoint_numbers(flags.checkpoint_directory)
    ckpt_num = ckpt_nums[-1] if flags.checkpoint is None else flags.checkpoint
    experiment = Experiment_Colab(flags.config, flags.checkpoint_directory, ckpt_num)
    arrays = run(experiment, flags, ckpt_num)
    write_npz(flags.out, arrays)
    print(f"wrote the bound profile of {arrays['images'].shape[0]} images at {flags.timesteps} times to {flags.out}: "
          f"mean bpd {arrays['bpd'].mean():.4f}, mean spread of the integrand {arrays['diff_std'].mean():.4f}")
    return 0


if __name__ == '__main__':
    main(sys.argv[1:])
