"""python -m ldm.sample --config=... --checkpoint_directory=... [--checkpoint N] --n_samples=N --out=FILE.npz
                      [--sampler dpm2m|sde2m|ddim|ancestral] [--eta 0.0] [--steps 25] [--batch_size B]
                      [--embedding deterministic|random] [--seed 0]
                      [--inpaint_images=FILE.npz [--mask box:y0,x0,y1,x1|half:left|right|top|bottom] [--resample 1]]

Writes a set of samples of a checkpoint's EMA parameters (Experiment_Colab) to one .npz: `images` (uint8
[n_samples, 32, 32, 3]) and the run's settings.  Not in the reference, which writes image grids only.  Global batch b
is drawn from PRNGKey(seed).fold_in(b) alone (the step noise of sde2m and of ddim with --eta > 0 from the third of its
three sub-keys, folded with the step index: Experiment_Colab.sample_batches); under torchrun the batches are dealt
round-robin to the ranks and rank 0 writes the file, so for a fixed --batch_size the file does not depend on the number
of ranks.  The flags are checked before any device is touched.

--inpaint_images=FILE.npz (array `images`, uint8 [N, 32, 32, 3], and optionally `mask`, [N, 32, 32] or [32, 32],
non-zero = keep) inpaints instead: image b B + j goes to slot j of global batch b, its kept pixels come back as they went
in and the rest is sampled (Experiment_Colab.sample_batches with known / mask; the known region's noise comes from a
fourth sub-key of the batch's key).  --mask names the mask where the file has none; --resample=U runs U passes per step;
--n_samples defaults to N; --embedding also takes `encoder`.  The output then holds `mask` (uint8 [n_samples, 32, 32])
too."""
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
    flags.DEFINE_string('inpaint_images', None, 'Inpaint the images of this .npz (images, optionally mask).')
    flags.DEFINE_string('mask', None, 'box:y0,x0,y1,x1 (unknown box) / half:left|right|top|bottom (kept half).')
    flags.DEFINE_integer('resample', 1, 'Inpainting: passes per step (1: no resampling).')
    flags.DEFINE_string('out', None, 'Output file (.npz).')
    flags.DEFINE_string('log_level', 'info', 'info/warning/error')
    flags.mark_flags_as_required(['config', 'checkpoint_directory', 'out'])
    return flags


def inpaint_inputs(flags):
    """-> (images uint8 [N, 32, 32, 3], mask bool [N, 32, 32]) named by --inpaint_images / --mask, None without
    --inpaint_images, or SystemExit"""
    from mulan_amd.sampling import mask_from_spec
    if flags.inpaint_images is None:
        if flags.mask is not None:
            raise SystemExit("--mask names the mask of --inpaint_images; there are no images")
        if flags.resample != 1:
            raise SystemExit("--resample applies to --inpaint_images")
        return None
    if flags.sampler == 'ancestral':
        raise SystemExit("--inpaint_images runs with --sampler=ddim, dpm2m or sde2m; the ancestral sampler takes no mask")
    if flags.resample < 1:
        raise SystemExit(f"--resample must be >= 1, got {flags.resample}")
    spec = None
    if flags.mask is not None:
        try:
            spec = mask_from_spec(flags.mask)
        except ValueError as e:
            raise SystemExit(f"--mask: {e}") from None
    try:
        with np.load(flags.inpaint_images, allow_pickle=False) as f:
            images = f['images'] if 'images' in f.files else None
            mask = f['mask'] if 'mask' in f.files else None
    except (OSError, ValueError) as e:
        raise SystemExit(f"--inpaint_images: cannot read {flags.inpaint_images!r} ({e})") from None
    if images is None or images.dtype != np.uint8 or images.ndim != 4 or images.shape[1:] != (32, 32, 3) or not len(images):
        raise SystemExit("--inpaint_images: the file needs an array `images`, uint8 [N, 32, 32, 3] with N >= 1")
    N = images.shape[0]
    if mask is None:
        if spec is None:
            raise SystemExit("--inpaint_images: the file has no `mask`; name one with --mask")
        mask = spec
    elif spec is not None:
        raise SystemExit("--mask given, but the file of --inpaint_images holds a `mask` of its own")
    if mask.shape not in ((32, 32), (N, 32, 32)) or mask.dtype.kind not in 'bui':
        raise SystemExit(f"--inpaint_images: `mask` is [{N}, 32, 32] or [32, 32] of bool or integers, got "
                         f"{mask.dtype} {list(mask.shape)}")
    return images, np.ascontiguousarray(np.broadcast_to(mask != 0, (N, 32, 32)))


def parse_flags(argv):
    """-> (flags, batch_size) or SystemExit: every check that needs no device"""
    return parse_all(argv)[:2]


def parse_all(argv):
    """-> (flags, batch_size, inpaint_inputs(flags)): parse_flags with the images and masks it read on the way"""
    flags = make_flags().parse(argv)
    if flags.sampler not in SAMPLERS:
        raise SystemExit(f"unknown --sampler {flags.sampler!r} (one of {', '.join(SAMPLERS)})")
    if not 0.0 <= flags.eta <= 1.0:
        raise SystemExit(f"--eta must lie in [0, 1], got {flags.eta!r}")
    if flags.eta != 0.0 and flags.sampler != 'ddim':
        raise SystemExit(f"--eta applies to --sampler=ddim; {flags.sampler!r} takes none")
    inpaint = inpaint_inputs(flags)
    embeddings = EMBEDDINGS + (('encoder',) if inpaint else ())
    if flags.embedding not in embeddings:
        raise SystemExit(f"unknown --embedding {flags.embedding!r} (one of {', '.join(embeddings)})")
    if flags.steps < 1:
        raise SystemExit(f"--steps must be >= 1, got {flags.steps}")
    if flags.n_samples is None and inpaint is None:
        raise SystemExit("flag --n_samples is required")
    if flags.n_samples is not None and flags.n_samples < 1:
        raise SystemExit(f"--n_samples must be >= 1, got {flags.n_samples}")
    if inpaint is not None and flags.n_samples is not None and flags.n_samples > len(inpaint[0]):
        raise SystemExit(f"--n_samples={flags.n_samples}, but --inpaint_images holds {len(inpaint[0])} images")
    batch_size = flags.batch_size if flags.batch_size is not None else int(flags.config.training.batch_size_eval)
    if batch_size < 1:
        raise SystemExit(f"--batch_size must be >= 1, got {batch_size}")
    if not flags.out.endswith('.npz'):
        raise SystemExit(f"--out must name a .npz file, got {flags.out!r}")
    if flags.embedding != 'deterministic' and flags.config.get('vdm_type', 'vdm') == 'vdm':
        raise SystemExit(f"--embedding={flags.embedding} needs a MuLAN model (vdm_type mulan_velocity / mulan_epsilon)")
    if not ckpt_lib.checkpoint_numbers(flags.checkpoint_directory):
        raise SystemExit(f'no ckpt-* files in {flags.checkpoint_directory}')
    return flags, batch_size, inpaint


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
    flags, batch_size, inpaint = parse_all(argv)
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
    n_samples = flags.n_samples if flags.n_samples is not None else len(inpaint[0])
    n_batches = math.ceil(n_samples / batch_size)
    mine = list(range(rank, n_batches, world))
    per_rank = math.ceil(n_batches / world)
    root = PRNGKey(flags.seed)
    kw = {}
    if inpaint is not None:
        # image b B + j in slot j of global batch b; the slots past the last image hold a black image with nothing kept
        pad = n_batches * batch_size
        known = np.zeros((pad, 32, 32, 3), dtype=np.uint8)
        keep = np.zeros((pad, 32, 32), dtype=bool)
        known[:n_samples], keep[:n_samples] = inpaint[0][:n_samples], inpaint[1][:n_samples]
        rows = lambda a, b: torch.from_numpy(a[b * batch_size:(b + 1) * batch_size])
        kw = dict(known=[rows(known, b) for b in mine], mask=[rows(keep, b) for b in mine], resample=flags.resample)
    images = experiment.sample_batches([root.fold_in(b) for b in mine], batch_size, flags.embedding, flags.sampler,
                                       flags.steps, flags.eta, **kw)
    local = torch.zeros((per_rank, batch_size, 32, 32, 3), dtype=torch.uint8, device=experiment.device)
    for j, x in enumerate(images):
        local[j].copy_(x)
    gathered = parallel.all_gather_tensor(local[None]).cpu().numpy()       # [world, per_rank, B, 32, 32, 3]
    if rank == 0:
        ordered = np.stack([gathered[b % world, b // world] for b in range(n_batches)])
        out = ordered.reshape(-1, 32, 32, 3)[:n_samples]
        settings = dict(sampler=flags.sampler, eta=float(flags.eta), steps=flags.steps, n_samples=n_samples,
                        batch_size=batch_size, embedding=flags.embedding, seed=flags.seed, checkpoint=str(ckpt_num),
                        vdm_type=flags.config.get('vdm_type', 'vdm'))
        arrays = dict(images=out)
        if inpaint is not None:
            settings.update(inpaint=True, resample=flags.resample, mask=flags.mask)
            arrays['mask'] = inpaint[1][:n_samples].astype(np.uint8)
        write_npz(flags.out, dict(arrays, settings=np.array(json.dumps(settings, sort_keys=True))))
        print(f'wrote {out.shape[0]} samples ({flags.sampler}, {flags.steps} steps) to {flags.out}')
    return 0


if __name__ == '__main__':
    main(sys.argv[1:])
