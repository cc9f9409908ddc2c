"""python -m ldm.fidelity --restored=restored.npz --originals=in.npz --out=fidelity.npz [--gray] [--keep 16] [--plain]
                        [--chunk 16384]

How good is a restoration or an inpainting?  --restored is what `python -m ldm.sample --restore_images / --inpaint_images`
writes: `images` (uint8 [N, 32, 32, 3]) with `degradation` (and `measurement`), or with `mask` ([N, 32, 32], non-zero =
kept); --originals holds the `images` the run started from, in the same order.  Writes to one .npz the arrays of
mulan_amd.fidelity.restoration_quality: per image `psnr`, `ssim`, `mse`, `ssim_planes` (P = 1 with --gray: the SSIM of
the luma), their means and medians; for an inpainting `psnr_masked` over the UNKNOWN pixels; for a restoration the same
figures of the trivial baseline A+ y (the degraded original replicated back to 32 x 32 x 3), prefixed `baseline_`, and
`psnr_gain`, `ssim_gain` with their means.  For the --keep images of lowest SSIM it also writes `worst` (their indices),
`worst_originals`, `worst_restored` and, for a restoration, `worst_baseline`; and the run's `settings`.  A --restored
with neither a mask nor a degradation is refused unless --plain is given, which writes the plain pairwise figures
(and ignores a mask or a degradation that is there).  Not in the reference.  The flags and both files are checked
before any device is touched.  One process."""
import json
import os
import sys

import numpy as np

from mulan_amd.config import Flags
from ldm.sample import write_npz


def make_flags():
    flags = Flags()
    flags.DEFINE_string('restored', None, 'A .npz as python -m ldm.sample --restore_images / --inpaint_images writes it.')
    flags.DEFINE_string('originals', None, 'A .npz with the `images` the run started from.')
    flags.DEFINE_string('out', None, 'Output file (.npz).')
    flags.DEFINE_bool('gray', False, 'The SSIM of the luma (the weights of rgb2gray) instead of the three channels.')
    flags.DEFINE_bool('plain', False, 'The plain pairwise figures: no baseline, no masked PSNR.')
    flags.DEFINE_integer('keep', 16, 'Keep the triples of this many images of lowest SSIM (0: none).')
    flags.DEFINE_integer('chunk', 16384, 'Pairs per upload.')
    flags.mark_flags_as_required(['restored', 'originals', 'out'])
    return flags


def parse_flags(argv):
    """-> flags or SystemExit: every check that needs no device and no file's contents"""
    flags = make_flags().parse(argv)
    if int(os.environ.get('WORLD_SIZE', '1')) > 1:
        raise SystemExit(f"ldm.fidelity runs in one process, WORLD_SIZE = {os.environ['WORLD_SIZE']}")
    if flags.keep < 0 or flags.chunk < 1:
        raise SystemExit("--keep must be >= 0, --chunk >= 1")
    if not flags.out.endswith('.npz'):
        raise SystemExit(f"--out must name a .npz file, got {flags.out!r}")
    for name in ('restored', 'originals'):
        if not os.path.isfile(getattr(flags, name)):
            raise SystemExit(f"--{name}: no file {getattr(flags, name)!r}")
    return flags


def read_inputs(flags):
    """(originals, restored, degradation | None, mask | None) or SystemExit"""
    from mulan_amd.sampling import parse_degradation
    images = {}
    degradation = mask = None
    for name in ('restored', 'originals'):
        with np.load(getattr(flags, name)) as z:
            if 'images' not in z.files:
                raise SystemExit(f"--{name}: {getattr(flags, name)!r} holds no `images`")
            x = images[name] = np.asarray(z['images'])
            if x.dtype != np.uint8 or x.ndim != 4 or x.shape[1:] != (32, 32, 3) or len(x) < 1:
                raise SystemExit(f"--{name}: uint8 [n >= 1, 32, 32, 3] expected, got {x.dtype} {x.shape}")
            if name == 'restored' and not flags.plain:
                if 'degradation' in z.files:
                    degradation = str(z['degradation'])
                if 'mask' in z.files:
                    mask = np.asarray(z['mask'])
    if len(images['restored']) != len(images['originals']):
        raise SystemExit(f"--restored holds {len(images['restored'])} images, --originals {len(images['originals'])}")
    if not flags.plain:
        if degradation is None and mask is None:
            raise SystemExit("--restored holds neither a `degradation` nor a `mask`: not the output of a restoration or an "
                             "inpainting run (--plain gives the plain pairwise figures)")
        if degradation is not None:
            try:
                parse_degradation(degradation)
            except ValueError as e:
                raise SystemExit(f"--restored: {e}") from None
        if mask is not None and (mask.dtype not in (np.uint8, np.bool_) or mask.shape != (len(images['restored']), 32, 32)):
            raise SystemExit(f"--restored: `mask` is uint8 [{len(images['restored'])}, 32, 32], got {mask.dtype} {mask.shape}")
    return images['originals'], images['restored'], degradation, mask


def run(originals, restored, degradation, mask, flags):
    """the arrays of the output file"""
    from mulan_amd import fidelity as fd
    res = fd.restoration_quality(originals, restored, degradation=degradation, mask=mask, gray=bool(flags.gray),
                                 chunk=flags.chunk)
    arrays = {key: np.asarray(value) for key, value in res.items() if key != 'baseline_images'}
    keep = min(flags.keep, len(originals))
    if keep:
        worst = np.argsort(res['ssim'], kind='stable')[:keep]
        arrays.update(worst=worst, worst_originals=originals[worst], worst_restored=restored[worst])
        if 'baseline_images' in res:
            arrays['worst_baseline'] = res['baseline_images'][worst]
    settings = dict(restored=flags.restored, originals=flags.originals, n=int(len(originals)), gray=bool(flags.gray),
                    plain=bool(flags.plain), keep=int(keep), chunk=flags.chunk, degradation=degradation,
                    inpaint=mask is not None)
    arrays['settings'] = np.array(json.dumps(settings, sort_keys=True))
    return arrays


def main(argv):
    flags = parse_flags(argv)
    originals, restored, degradation, mask = read_inputs(flags)
    arrays = run(originals, restored, degradation, mask, flags)
    write_npz(flags.out, arrays)
    line = f"PSNR {float(arrays['psnr_mean']):.3f} dB, SSIM {float(arrays['ssim_mean']):.4f}"
    if 'psnr_gain_mean' in arrays:
        line += (f"; over the baseline A+ y {float(arrays['psnr_gain_mean']):+.3f} dB, "
                 f"{float(arrays['ssim_gain_mean']):+.4f} SSIM")
    if 'psnr_masked_mean' in arrays:
        line += f"; over the unknown pixels PSNR {float(arrays['psnr_masked_mean']):.3f} dB"
    print(f"wrote the fidelity of {len(restored)} images to {flags.out}: mean {line}")
    return 0


if __name__ == '__main__':
    main(sys.argv[1:])
