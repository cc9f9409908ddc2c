"""python -m ldm.spectrum --samples=samples.npz --reference=cifar10|imagenet32|npz:FILE --out=spectrum.npz
                        [--gray] [--max_reference N] [--chunk 16384]

Do the samples of `python -m ldm.sample` have the spatial spectrum of the training set?  Reads `images` (uint8
[S, 32, 32, 3]) from --samples and the training images of --reference (mulan_amd.data.load_arrays(name, train=True);
`synthetic` has no fixed set and is refused), the first --max_reference of them if given, and writes to one .npz the
arrays of mulan_amd.spectrum.image_spectrum of both sets, prefixed `samples_` and `reference_` (`power_mean`,
`coef_mean`, `coef_var` [32, 32, P], `radial_mean` [45, P], `n`; P = 1 with --gray, else 3), `radial_freq` [45], the
arrays of compare_spectra (`log_ratio` [45, P], `lsd_db`, `high_band_ratio`, `frechet_diag`: PIXEL-space figures for
comparing runs of one checkpoint, not comparable with published feature-space numbers) and the run's `settings`.  The
transform is the orthonormal 32 x 32 DCT of mulan_spectrum.  Not in the reference.  The flags are checked before any
device is touched.  One process."""
import json
import os
import sys

import numpy as np

from mulan_amd.config import Flags
from ldm.sample import write_npz

SET_KEYS = ('power_mean', 'coef_mean', 'coef_var', 'radial_mean', 'n')
COMPARE_KEYS = ('log_ratio', 'lsd_db', 'high_band_ratio', 'frechet_diag')


def make_flags():
    flags = Flags()
    flags.DEFINE_string('samples', None, 'A .npz with `images`, as python -m ldm.sample writes it.')
    flags.DEFINE_string('reference', None, 'cifar10, imagenet32 or npz:FILE: the training images to compare with.')
    flags.DEFINE_string('out', None, 'Output file (.npz).')
    flags.DEFINE_bool('gray', False, 'One grey plane (the weights of rgb2gray) instead of the three channels.')
    flags.DEFINE_integer('max_reference', 0, 'Use the first N reference images only (0: all).')
    flags.DEFINE_integer('chunk', 16384, 'Images per upload.')
    flags.mark_flags_as_required(['samples', 'reference', 'out'])
    return flags


def parse_flags(argv):
    """-> flags or SystemExit: every check that needs no device"""
    flags = make_flags().parse(argv)
    if int(os.environ.get('WORLD_SIZE', '1')) > 1:
        raise SystemExit(f"ldm.spectrum runs in one process, WORLD_SIZE = {os.environ['WORLD_SIZE']}")
    if flags.reference in ('synthetic', 'npz:') or not (flags.reference in ('cifar10', 'imagenet32') or
                                                        flags.reference.startswith('npz:')):
        raise SystemExit(f"--reference is cifar10, imagenet32 or npz:FILE (synthetic has no fixed set), got "
                         f"{flags.reference!r}")
    if flags.max_reference < 0 or flags.chunk < 1:
        raise SystemExit("--max_reference must be >= 0, --chunk >= 1")
    if not flags.out.endswith('.npz'):
        raise SystemExit(f"--out must name a .npz file, got {flags.out!r}")
    if not os.path.isfile(flags.samples):
        raise SystemExit(f"--samples: no file {flags.samples!r}")
    return flags


def read_inputs(flags):
    """(samples, reference): uint8 [S, 32, 32, 3], [R, 32, 32, 3]"""
    from mulan_amd import data
    with np.load(flags.samples) as z:
        if 'images' not in z.files:
            raise SystemExit(f"--samples: {flags.samples!r} holds no `images`")
        samples = np.asarray(z['images'])
    reference, _ = data.load_arrays(flags.reference, train=True)
    if flags.max_reference:
        reference = reference[:flags.max_reference]
    for name, x in (('samples', samples), ('reference', reference)):
        if x.dtype != np.uint8 or x.ndim != 4 or x.shape[1:] != (32, 32, 3) or len(x) < 1:
            raise SystemExit(f"--{name}: uint8 [n >= 1, 32, 32, 3] expected, got {x.dtype} {x.shape}")
    return samples, reference


def run(samples, reference, flags):
    """the arrays of the output file"""
    from mulan_amd import spectrum as sp
    a = sp.image_spectrum(samples, gray=bool(flags.gray), chunk=flags.chunk)
    b = sp.image_spectrum(reference, gray=bool(flags.gray), chunk=flags.chunk)
    cmp = sp.compare_spectra(a, b)
    arrays = {'radial_freq': a['radial_freq']}
    for prefix, d in (('samples_', a), ('reference_', b)):
        arrays.update({prefix + key: np.asarray(d[key]) for key in SET_KEYS})
    arrays.update({key: np.asarray(cmp[key]) for key in COMPARE_KEYS})
    settings = dict(samples=flags.samples, reference=flags.reference, n_samples=int(len(samples)),
                    n_reference=int(len(reference)), gray=bool(flags.gray), chunk=flags.chunk)
    arrays['settings'] = np.array(json.dumps(settings, sort_keys=True))
    return arrays


def main(argv):
    flags = parse_flags(argv)
    samples, reference = read_inputs(flags)
    arrays = run(samples, reference, flags)
    write_npz(flags.out, arrays)
    print(f"wrote the spectra of {len(samples)} samples and {len(reference)} reference images to {flags.out}: "
          f"log-spectral distance {float(arrays['lsd_db']):.3f} dB, high-band ratio {float(arrays['high_band_ratio']):.4f}, "
          f"diagonal Frechet distance in DCT space {float(arrays['frechet_diag']):.5g} (pixel-space figures)")
    return 0


if __name__ == '__main__':
    main(sys.argv[1:])
