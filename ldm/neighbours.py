"""python -m ldm.neighbours --samples=samples.npz --reference=cifar10|imagenet32|npz:FILE --out=neighbours.npz
                          [--k 5] [--precision_recall --pr_k 3] [--max_reference N] [--keep 16] [--duplicate_rms 1.0]

Are the samples of `python -m ldm.sample` new?  Reads `images` (uint8 [S, 32, 32, 3]) from --samples and the training
images of --reference (mulan_amd.data.load_arrays(name, train=True); `synthetic` has no fixed set and is refused), the
first --max_reference of them if given, and writes the arrays of mulan_amd.neighbours.novelty to one .npz: `nn_idx`,
`nn_dist2` [S, k], `nn_rms`, `self_idx`, `self_dist2`, `self_rms` [S], `duplicates`, `duplicate_rms`, `train_self_rms`,
`train_subset` [M]; with --precision_recall also `precision`, `recall`, `pr_k`, `covered_samples` [S], `covered_real` [R]
(k-NN precision and recall in PIXEL space: for comparing runs of one checkpoint, not comparable with published
feature-space numbers); for the --keep most suspicious samples (smallest nn_rms) `kept` [keep] (their indices),
`kept_samples` [keep, 32, 32, 3] and `kept_neighbours` [keep, k, 32, 32, 3]; and the run's `settings`.  Every distance is
an exact integer (mulan_knn_u8).  Not in the reference.  The flags are checked before any device is touched.  One process."""
import json
import os
import sys

import numpy as np

from mulan_amd.config import Flags
from ldm.sample import write_npz

NOVELTY_KEYS = ('nn_idx', 'nn_dist2', 'nn_rms', 'self_idx', 'self_dist2', 'self_rms', 'duplicates', 'duplicate_rms',
                'train_self_rms', 'train_subset')
PR_KEYS = ('precision', 'recall', 'pr_k', 'covered_samples', 'covered_real')
KEPT_KEYS = ('kept', 'kept_samples', 'kept_neighbours')


def make_flags():
    flags = Flags()
    flags.DEFINE_string('samples', None, 'A .npz with `images`, as python -m ldm.sample writes it.')
    flags.DEFINE_string('reference', None, 'cifar10, imagenet32 or npz:FILE: the training images to search.')
    flags.DEFINE_string('out', None, 'Output file (.npz).')
    flags.DEFINE_integer('k', 5, 'Training neighbours per sample.')
    flags.DEFINE_bool('precision_recall', False, 'Also k-NN precision and recall in pixel space.')
    flags.DEFINE_integer('pr_k', 3, 'The k of the precision / recall radii.')
    flags.DEFINE_integer('max_reference', 0, 'Use the first N reference images only (0: all).')
    flags.DEFINE_integer('keep', 16, 'Most suspicious samples written as images beside their neighbours.')
    flags.DEFINE_float('duplicate_rms', 1.0, 'Two samples this close (RMS grey levels) count as duplicates.')
    flags.DEFINE_integer('chunk', 16384, 'Reference rows per upload.')
    flags.mark_flags_as_required(['samples', 'reference', 'out'])
    return flags


def parse_flags(argv):
    """-> flags or SystemExit: every check that needs no device"""
    flags = make_flags().parse(argv)
    if int(os.environ.get('WORLD_SIZE', '1')) > 1:
        raise SystemExit(f"ldm.neighbours runs in one process, WORLD_SIZE = {os.environ['WORLD_SIZE']}")
    if flags.reference in ('synthetic', 'npz:') or not (flags.reference in ('cifar10', 'imagenet32') or
                                                        flags.reference.startswith('npz:')):
        raise SystemExit(f"--reference is cifar10, imagenet32 or npz:FILE (synthetic has no fixed set), got "
                         f"{flags.reference!r}")
    if not 1 <= flags.k <= 16:
        raise SystemExit(f"--k must be in [1, 16], got {flags.k}")
    if not 1 <= flags.pr_k <= 16:
        raise SystemExit(f"--pr_k must be in [1, 16], got {flags.pr_k}")
    if flags.max_reference < 0 or flags.keep < 0 or flags.chunk < 1:
        raise SystemExit("--max_reference and --keep must be >= 0, --chunk >= 1")
    if not flags.duplicate_rms >= 0:
        raise SystemExit(f"--duplicate_rms must be >= 0, got {flags.duplicate_rms}")
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
        if x.dtype != np.uint8 or x.ndim != 4 or x.shape[1:] != (32, 32, 3) or len(x) < 2:
            raise SystemExit(f"--{name}: uint8 [n >= 2, 32, 32, 3] expected, got {x.dtype} {x.shape}")
    return samples, reference


def run(samples, reference, flags):
    """the arrays of the output file"""
    from mulan_amd import neighbours as nb
    res = nb.novelty(samples, reference, k=flags.k, duplicate_rms=flags.duplicate_rms, chunk=flags.chunk)
    arrays = {key: np.asarray(res[key]) for key in NOVELTY_KEYS}
    if flags.precision_recall:
        pr = nb.precision_recall(samples, reference, k=flags.pr_k, chunk=flags.chunk)
        arrays.update(precision=np.asarray(pr['precision']), recall=np.asarray(pr['recall']), pr_k=np.asarray(flags.pr_k),
                      covered_samples=pr['covered_samples'], covered_real=pr['covered_real'])
    kept = np.argsort(res['nn_rms'], kind='stable')[:flags.keep]
    arrays['kept'] = kept.astype(np.int64)
    arrays['kept_samples'] = samples[kept]
    arrays['kept_neighbours'] = reference[np.maximum(res['nn_idx'][kept], 0)]
    settings = dict(samples=flags.samples, reference=flags.reference, n_samples=int(len(samples)),
                    n_reference=int(len(reference)), k=flags.k, duplicate_rms=flags.duplicate_rms, keep=int(len(kept)),
                    precision_recall=bool(flags.precision_recall), pr_k=flags.pr_k)
    arrays['settings'] = np.array(json.dumps(settings, sort_keys=True))
    return arrays


def main(argv):
    flags = parse_flags(argv)
    samples, reference = read_inputs(flags)
    arrays = run(samples, reference, flags)
    write_npz(flags.out, arrays)
    line = (f"wrote the neighbours of {len(samples)} samples among {len(reference)} images to {flags.out}: median nearest "
            f"training image at {np.median(arrays['nn_rms']):.2f} grey levels RMS (training images among themselves: "
            f"{np.median(arrays['train_self_rms']):.2f}), duplicates {float(arrays['duplicates']):.4f}")
    if flags.precision_recall:
        line += f", pixel-space precision {float(arrays['precision']):.4f} recall {float(arrays['recall']):.4f}"
    print(line)
    return 0


if __name__ == '__main__':
    main(sys.argv[1:])
