"""python -m ldm.sample --config=... --checkpoint_directory=... [--checkpoint N] --n_samples=N --out=FILE.npz
                      [--sampler dpm2m|sde2m|ddim|ancestral] [--eta 0.0] [--steps 25] [--batch_size B]
                      [--embedding deterministic|random] [--seed 0]
                      [--grid uniform|logsnr|karras|quadratic [--grid_rho 7]]
                      [--inpaint_images=FILE.npz [--mask box:y0,x0,y1,x1|half:left|right|top|bottom] [--resample 1]]
                      [--restore_images=FILE.npz [--degradation sr:4|gray|sr:4+gray] [--resample 1]]

Writes a set of samples of a checkpoint's EMA parameters (Experiment_Colab) to one .npz: `images` (uint8
[n_samples, 32, 32, 3]) and the run's settings.  Not in the reference, which writes image grids only.  Global batch b
is drawn from PRNGKey(seed).fold_in(b) alone (the step noise of sde2m and of ddim with --eta > 0 from the third of its
three sub-keys, folded with the step index: Experiment_Colab.sample_batches); under torchrun the batches are dealt
round-robin to the ranks and rank 0 writes the file, so for a fixed --batch_size the file does not depend on the number
of ranks.  The flags are checked before any device is touched.

--grid names the time grid of a few-step sampler (mulan_amd.sampling.make_grid): uniform in t (the default), quadratic
in t, or -- on the mean schedule of each batch's own embeddings, so a batch still depends on its key alone -- uniform in
the log signal-to-noise ratio (logsnr) or the EDM grid with --grid_rho (karras).

--inpaint_images=FILE.npz (array `images`, uint8 [N, 32, 32, 3], and optionally `mask`, [N, 32, 32] or [32, 32],
non-zero = keep) inpaints instead: image b B + j goes to slot j of global batch b, its kept pixels come back as they went
in and the rest is sampled (Experiment_Colab.sample_batches with known / mask; the known region's noise comes from a
fourth sub-key of the batch's key).  --mask names the mask where the file has none; --resample=U runs U passes per step;
--n_samples defaults to N; --embedding also takes `encoder`.  The output then holds `mask` (uint8 [n_samples, 32, 32])
too.

--restore_images=FILE.npz restores instead: the file holds either `images` (uint8 [N, 32, 32, 3]), which the run degrades
by --degradation (sr:f: f x f average pooling, f in 2, 4, 8, 16; gray: the channel mean; sr:f+gray: both; default sr:4),
or their `measurement` ([N, 32 / f, 32 / f, 3 or 1 with gray], uint8 levels or fp32 in the model's [-1, 1] scale).  Every
step's prediction is projected onto the measurement (Experiment_Colab.sample_batches with measurement / degradation);
--resample=U runs U passes per step, the jumps drawn from the fourth sub-key.  Slots, --n_samples and --embedding as with
--inpaint_images, which it excludes, as it does the ancestral sampler.  The output then holds `measurement` (fp32
[n_samples, ...], the scale above), `degradation` and `residual` (fp32 [n_samples]: the largest |A encode(image) - y|
per image in grey levels)."""
import io
import json
import logging
import math
import os
import sys
import zipfile
from collections import namedtuple

import numpy as np

from mulan_amd.config import Flags
from mulan_amd import checkpoint as ckpt_lib
from mulan_amd.sampling import SAMPLERS, check_grid

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
    flags.DEFINE_string('grid', 'uniform', 'Time grid of ddim / dpm2m / sde2m: uniform / logsnr / karras / quadratic.')
    flags.DEFINE_float('grid_rho', 7.0, '--grid=karras: the exponent rho, finite and > 0.')
    flags.DEFINE_string('inpaint_images', None, 'Inpaint the images of this .npz (images, optionally mask).')
    flags.DEFINE_string('mask', None, 'box:y0,x0,y1,x1 (unknown box) / half:left|right|top|bottom (kept half).')
    flags.DEFINE_integer('resample', 1, 'Inpainting and restoration: passes per step (1: no resampling).')
    flags.DEFINE_string('restore_images', None, 'Restore from this .npz (images to degrade, or their measurement).')
    flags.DEFINE_string('degradation', None, 'sr:f (f in 2, 4, 8, 16) / gray / sr:f+gray; default sr:4.')
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
        if flags.resample != 1 and flags.restore_images is None:
            raise SystemExit("--resample applies to --inpaint_images and --restore_images")
        return None
    if flags.restore_images is not None:
        raise SystemExit("--inpaint_images and --restore_images exclude each other: inpaint or restore")
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


# what --restore_images / --degradation name: `array` is the file's `images` (uint8 [N, 32, 32, 3], degrade True: the run
# degrades them) or its `measurement` ([N, 32 / f, 32 / f, 3 or 1], uint8 or float32, degrade False); (f, gray) is `spec` parsed
RestoreInputs = namedtuple("RestoreInputs", "array degrade f gray spec")


def restore_inputs(flags):
    """-> RestoreInputs named by --restore_images / --degradation, None without --restore_images, or SystemExit"""
    from mulan_amd.sampling import parse_degradation
    if flags.restore_images is None:
        if flags.degradation is not None:
            raise SystemExit("--degradation names what --restore_images went through; there are no images")
        return None
    if flags.sampler == 'ancestral':
        raise SystemExit("--restore_images runs with --sampler=ddim, dpm2m or sde2m; the ancestral sampler takes no "
                         "measurement")
    if flags.resample < 1:
        raise SystemExit(f"--resample must be >= 1, got {flags.resample}")
    spec = flags.degradation if flags.degradation is not None else 'sr:4'
    try:
        f, gray = parse_degradation(spec)
    except ValueError as e:
        raise SystemExit(f"--degradation: {e}") from None
    try:
        with np.load(flags.restore_images, allow_pickle=False) as z:
            images = z['images'] if 'images' in z.files else None
            y = z['measurement'] if 'measurement' in z.files else None
    except (OSError, ValueError) as e:
        raise SystemExit(f"--restore_images: cannot read {flags.restore_images!r} ({e})") from None
    if (images is None) == (y is None):
        raise SystemExit("--restore_images: the file needs `images` (to degrade) or `measurement`, one of the two")
    if images is not None and (images.dtype != np.uint8 or images.ndim != 4 or images.shape[1:] != (32, 32, 3)
                               or not len(images)):
        raise SystemExit("--restore_images: `images` is uint8 [N, 32, 32, 3] with N >= 1")
    shape = (32 // f, 32 // f, 1 if gray else 3)
    if y is not None and (y.dtype not in (np.uint8, np.float32) or y.ndim != 4 or y.shape[1:] != shape or not len(y)):
        raise SystemExit(f"--restore_images: the `measurement` of {spec} is uint8 or float32 [N, {shape[0]}, {shape[1]}, "
                         f"{shape[2]}] with N >= 1, got {y.dtype} {list(y.shape)}")
    return RestoreInputs(images if y is None else y, y is None, f, gray, spec)


def parse_flags(argv):
    """-> (flags, batch_size) or SystemExit: every check that needs no device"""
    return parse_all(argv)[:2]


def parse_all(argv):
    """-> (flags, batch_size, inpaint_inputs(flags), restore_inputs(flags), given): parse_flags with the arrays it read
    on the way; given: the array with one entry per image to produce (None: an unconditional run)"""
    flags = make_flags().parse(argv)
    if flags.sampler not in SAMPLERS:
        raise SystemExit(f"unknown --sampler {flags.sampler!r} (one of {', '.join(SAMPLERS)})")
    if not 0.0 <= flags.eta <= 1.0:
        raise SystemExit(f"--eta must lie in [0, 1], got {flags.eta!r}")
    if flags.eta != 0.0 and flags.sampler != 'ddim':
        raise SystemExit(f"--eta applies to --sampler=ddim; {flags.sampler!r} takes none")
    try:
        check_grid(flags.sampler, flags.grid, None, flags.grid_rho)
    except ValueError as e:
        raise SystemExit(f"--grid: {e}") from None
    inpaint = inpaint_inputs(flags)
    restore = restore_inputs(flags)
    given = inpaint[0] if inpaint else restore.array if restore else None     # the input images, or their measurements
    embeddings = EMBEDDINGS + (('encoder',) if given is not None else ())
    if flags.embedding not in embeddings:
        raise SystemExit(f"unknown --embedding {flags.embedding!r} (one of {', '.join(embeddings)})")
    if flags.steps < 1:
        raise SystemExit(f"--steps must be >= 1, got {flags.steps}")
    if flags.n_samples is None and given is None:
        raise SystemExit("flag --n_samples is required")
    if flags.n_samples is not None and flags.n_samples < 1:
        raise SystemExit(f"--n_samples must be >= 1, got {flags.n_samples}")
    if given is not None and flags.n_samples is not None and flags.n_samples > len(given):
        raise SystemExit(f"--n_samples={flags.n_samples}, but --{'inpaint' if inpaint else 'restore'}_images holds "
                         f"{len(given)} images")
    batch_size = flags.batch_size if flags.batch_size is not None else int(flags.config.training.batch_size_eval)
    if batch_size < 1:
        raise SystemExit(f"--batch_size must be >= 1, got {batch_size}")
    if not flags.out.endswith('.npz'):
        raise SystemExit(f"--out must name a .npz file, got {flags.out!r}")
    if flags.embedding != 'deterministic' and flags.config.get('vdm_type', 'vdm') == 'vdm':
        raise SystemExit(f"--embedding={flags.embedding} needs a MuLAN model (vdm_type mulan_velocity / mulan_epsilon)")
    if not ckpt_lib.checkpoint_numbers(flags.checkpoint_directory):
        raise SystemExit(f'no ckpt-* files in {flags.checkpoint_directory}')
    return flags, batch_size, inpaint, restore, given


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
    flags, batch_size, inpaint, restore, given = parse_all(argv)
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
    n_samples = flags.n_samples if flags.n_samples is not None else len(given)
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
    if restore is not None:
        # as above; the slots past the last image hold the measurement of a black image.  Every rank forms the whole
        # measurement (it is small), so the file does not depend on the number of ranks
        from mulan_amd import ops
        pad = n_batches * batch_size
        src = np.zeros((pad,) + given.shape[1:], dtype=given.dtype)
        src[:n_samples] = given[:n_samples]
        src = torch.from_numpy(src).to(experiment.device)
        enc = ops.encode_u8(src) if src.dtype == torch.uint8 else src
        y_all = ops.restore_measure(enc, restore.f, restore.gray) if restore.degrade else enc
        kw = dict(measurement=[y_all[b * batch_size:(b + 1) * batch_size].contiguous() for b in mine],
                  degradation=restore.spec, resample=flags.resample)
    images = experiment.sample_batches([root.fold_in(b) for b in mine], batch_size, flags.embedding, flags.sampler,
                                       flags.steps, flags.eta, grid=flags.grid, grid_rho=flags.grid_rho, **kw)
    local = torch.zeros((per_rank, batch_size, 32, 32, 3), dtype=torch.uint8, device=experiment.device)
    for j, x in enumerate(images):
        local[j].copy_(x)
    gathered = parallel.all_gather_tensor(local[None]).cpu().numpy()       # [world, per_rank, B, 32, 32, 3]
    if rank == 0:
        ordered = np.stack([gathered[b % world, b // world] for b in range(n_batches)])
        out = ordered.reshape(-1, 32, 32, 3)[:n_samples]
        settings = dict(sampler=flags.sampler, eta=float(flags.eta), steps=flags.steps, n_samples=n_samples,
                        batch_size=batch_size, embedding=flags.embedding, seed=flags.seed, checkpoint=str(ckpt_num),
                        vdm_type=flags.config.get('vdm_type', 'vdm'), grid=flags.grid, grid_rho=float(flags.grid_rho))
        arrays = dict(images=out)
        if inpaint is not None:
            settings.update(inpaint=True, resample=flags.resample, mask=flags.mask)
            arrays['mask'] = inpaint[1][:n_samples].astype(np.uint8)
        if restore is not None:
            settings.update(restore=True, resample=flags.resample, degradation=restore.spec)
            y = y_all[:n_samples]
            back = ops.restore_measure(ops.encode_u8(torch.from_numpy(out).to(experiment.device)), restore.f,
                                        restore.gray)
            residual = (back - y).abs().reshape(n_samples, -1).amax(dim=1) * 127.5
            arrays.update(measurement=y.cpu().numpy(), degradation=np.array(restore.spec),
                          residual=residual.cpu().numpy())
        write_npz(flags.out, dict(arrays, settings=np.array(json.dumps(settings, sort_keys=True))))
        print(f'wrote {out.shape[0]} samples ({flags.sampler}, {flags.steps} steps) to {flags.out}')
    return 0


if __name__ == '__main__':
    main(sys.argv[1:])
