"""python -m ldm.moments --samples=samples.npz --reference=cifar10|imagenet32|npz:FILE|moments:FILE --out=moments.npz
                       [--max_reference N] [--chunk 16384] [--eigen 16] [--save_reference_moments FILE]

How far is the distribution of the samples of `python -m ldm.sample` from the data?  Reads `images` (uint8 [S, 32, 32, 3])
from --samples and the training images of --reference (mulan_amd.data.load_arrays(name, train=True); `synthetic` has no
fixed set and is refused), the first --max_reference of them if given, or the saved integer moments of a reference set
(moments:FILE, as --save_reference_moments writes them; a file whose D differs from the samples' D is refused).  Writes
the arrays of mulan_amd.moments.compare_moments to one .npz: `distance`, `mean_term`, `cov_term`, `frechet_diag_pixel`,
`trace_ratio`, `eigenvalues_samples`, `eigenvalues_reference` [D]; both means `mean_samples`, `mean_reference`
[32, 32, 3]; the integers `n_samples`, `sum_samples`, `gram_samples`, `n_reference`, `sum_reference`, `gram_reference`;
the --eigen leading eigen-images of both sets, `eigen_images_samples`, `eigen_images_reference` [eigen, 32, 32, 3], with
`eigen_ratio_samples`, `eigen_ratio_reference`; and the run's `settings`.  The moments are exact integers
(mulan_set_moments_u8); the distance is the Frechet distance of the two fitted Gaussians in PIXEL space: for comparing
runs of one checkpoint against the same reference set, not comparable with published FID.  Not in the reference.  The
flags are checked before any device is touched.  One process."""
import json
import os
import sys

import numpy as np

from mulan_amd.config import Flags
from ldm.sample import write_npz

COMPARE_KEYS = ('distance', 'mean_term', 'cov_term', 'frechet_diag_pixel', 'trace_ratio')


def make_flags():
    flags = Flags()
    flags.DEFINE_string('samples', None, 'A .npz with `images`, as python -m ldm.sample writes it.')
    flags.DEFINE_string('reference', None, 'cifar10, imagenet32, npz:FILE or moments:FILE: the set to compare with.')
    flags.DEFINE_string('out', None, 'Output file (.npz).')
    flags.DEFINE_integer('max_reference', 0, 'Use the first N reference images only (0: all).')
    flags.DEFINE_integer('chunk', 16384, 'Rows per upload.')
    flags.DEFINE_integer('eigen', 16, 'Leading eigen-images of both sets written to the file.')
    flags.DEFINE_string('save_reference_moments', None, 'Also write the reference set\'s integer moments to this .npz.')
    flags.mark_flags_as_required(['samples', 'reference', 'out'])
    return flags


def parse_flags(argv):
    """-> flags or SystemExit: every check that needs no device"""
    flags = make_flags().parse(argv)
    if int(os.environ.get('WORLD_SIZE', '1')) > 1:
        raise SystemExit(f"ldm.moments runs in one process, WORLD_SIZE = {os.environ['WORLD_SIZE']}")
    ref = flags.reference
    if ref in ('synthetic', 'npz:', 'moments:') or not (ref in ('cifar10', 'imagenet32') or ref.startswith('npz:')
                                                       or ref.startswith('moments:')):
        raise SystemExit(f"--reference is cifar10, imagenet32, npz:FILE or moments:FILE (synthetic has no fixed set), got "
                         f"{ref!r}")
    if flags.max_reference < 0 or not 1 <= flags.chunk <= 2 ** 24:
        raise SystemExit("--max_reference must be >= 0, --chunk in [1, 2^24]")
    if not 0 <= flags.eigen <= 3072:
        raise SystemExit(f"--eigen must be in [0, 3072], got {flags.eigen}")
    if not flags.out.endswith('.npz'):
        raise SystemExit(f"--out must name a .npz file, got {flags.out!r}")
    if flags.save_reference_moments is not None and not flags.save_reference_moments.endswith('.npz'):
        raise SystemExit(f"--save_reference_moments must name a .npz file, got {flags.save_reference_moments!r}")
    if ref.startswith('moments:') and flags.max_reference:
        raise SystemExit("--max_reference has no meaning with saved moments")
    if not os.path.isfile(flags.samples):
        raise SystemExit(f"--samples: no file {flags.samples!r}")
    if ref.startswith('moments:') and not os.path.isfile(ref[len('moments:'):]):
        raise SystemExit(f"--reference: no file {ref[len('moments:'):]!r}")
    return flags


def _check_images(name, x):
    if x.dtype != np.uint8 or x.ndim != 4 or x.shape[1:] != (32, 32, 3) or len(x) < 2:
        raise SystemExit(f"--{name}: uint8 [n >= 2, 32, 32, 3] expected, got {x.dtype} {x.shape}")


def read_inputs(flags):
    """(samples, reference): uint8 [S, 32, 32, 3] and either [R, 32, 32, 3] or the dict of saved moments; no device"""
    from mulan_amd import moments as mo
    with np.load(flags.samples) as z:
        if 'images' not in z.files:
            raise SystemExit(f"--samples: {flags.samples!r} holds no `images`")
        samples = np.asarray(z['images'])
    _check_images('samples', samples)
    if flags.reference.startswith('moments:'):
        path = flags.reference[len('moments:'):]
        try:
            reference = mo.load_moments(path)
        except (ValueError, OSError) as e:
            raise SystemExit(f"--reference: {e}")
        D = int(np.prod(samples.shape[1:]))
        if reference['sum'].shape[0] != D:
            raise SystemExit(f"--reference: {path!r} holds moments of D = {reference['sum'].shape[0]}, the samples have "
                             f"D = {D}")
        return samples, reference
    from mulan_amd import data
    reference, _ = data.load_arrays(flags.reference, train=True)
    if flags.max_reference:
        reference = reference[:flags.max_reference]
    _check_images('reference', reference)
    return samples, reference


def run(samples, reference, flags):
    """the arrays of the output file"""
    from mulan_amd import moments as mo
    ms = mo.set_moments(samples, chunk=flags.chunk)
    mr = reference if isinstance(reference, dict) else mo.set_moments(reference, chunk=flags.chunk)
    settings = dict(samples=flags.samples, reference=flags.reference, n_samples=ms['n'], n_reference=mr['n'],
                    eigen=flags.eigen)
    if flags.save_reference_moments:
        mo.save_moments(flags.save_reference_moments, mr, settings=dict(reference=flags.reference, n=mr['n']))
    cmp = mo.compare_moments(ms, mr)
    arrays = {key: np.asarray(cmp[key]) for key in COMPARE_KEYS}
    arrays.update(eigenvalues_samples=cmp['eigenvalues_a'], eigenvalues_reference=cmp['eigenvalues_b'])
    for name, m in (('samples', ms), ('reference', mr)):
        arrays['mean_' + name] = m['mean'].reshape(samples.shape[1:])
        arrays['n_' + name] = np.asarray(m['n'], dtype=np.int64)
        arrays['sum_' + name] = m['sum']
        arrays['gram_' + name] = m['gram']
        if flags.eigen:
            e = mo.eigen_images(dict(m, shape=samples.shape[1:]), flags.eigen)
            arrays['eigen_images_' + name] = e['images']
            arrays['eigen_ratio_' + name] = e['ratio']
    arrays['settings'] = np.array(json.dumps(settings, sort_keys=True))
    return arrays


def main(argv):
    flags = parse_flags(argv)
    samples, reference = read_inputs(flags)
    arrays = run(samples, reference, flags)
    write_npz(flags.out, arrays)
    print(f"wrote the moments of {len(samples)} samples against {int(arrays['n_reference'])} images to {flags.out}: "
          f"pixel-space Frechet distance {float(arrays['distance']):.4f} (means {float(arrays['mean_term']):.4f}, "
          f"covariances {float(arrays['cov_term']):.4f}), diagonal form {float(arrays['frechet_diag_pixel']):.4f}, "
          f"trace ratio {float(arrays['trace_ratio']):.4f}; not comparable with published FID")
    return 0


if __name__ == '__main__':
    main(sys.argv[1:])
