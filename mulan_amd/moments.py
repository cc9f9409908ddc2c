"""How far is the distribution of the samples from the data?  The exact mean and full covariance of sets of uint8 images
in pixel space (ops.set_moments_u8, mulan_set_moments_u8 on the int8 matrix cores) and what is read off them: the
Frechet distance of the two Gaussians fitted to two sets -- the form of FID, taken on the pixels because no outside
network is on hand -- and the eigen-images of a set.  Not in the reference.

The device gives integers: sum[j] and gram[j, k] of c = x - 128.  Everything here is host float64 arithmetic on those
integers, so it is tested without a device; integer moments add exactly, so those of a large reference set can be
computed once and kept in a file (`save_moments`, `merge_moments`).

These are PIXEL-space figures: they are not comparable with published feature-space numbers (FID) and are meant for
comparing runs (samplers, step counts, grids) of ONE checkpoint against the same reference set."""
import json

import numpy as np
import torch

from . import ops
from .neighbours import DEFAULT_CHUNK, _device_rows

MAX_N = 2 ** 24                # n gram - sum sum^T is exact in int64 up to here: n gram <= 2^24 2^24 2^14 = 2^62


def _moments_dict(n, total, gram, shape):
    """the dict of `set_moments` from its integers: mean = 128 + sum / n, cov = (n gram - sum sum^T) / (n (n - 1))"""
    total, gram = np.ascontiguousarray(total, dtype=np.int64), np.ascontiguousarray(gram, dtype=np.int64)
    n = int(n)
    D = total.shape[0]
    if total.ndim != 1 or gram.shape != (D, D):
        raise ValueError(f"moments: sum is int64 [D] and gram [D, D], got {total.shape} and {gram.shape}")
    if not 2 <= n <= MAX_N:
        raise ValueError(f"moments: a covariance needs 2 <= n <= 2^24 images, got n = {n}")
    shape = tuple(int(v) for v in shape)
    if int(np.prod(shape)) != D:
        raise ValueError(f"moments: image shape {shape} does not hold D = {D} values")
    num = n * gram - np.outer(total, total)                   # int64, exact: |n gram| <= 2^62, |sum sum^T| <= 2^62
    cov = num.astype(np.float64) / (float(n) * float(n - 1))
    return dict(n=n, sum=total, gram=gram, mean=128.0 + total.astype(np.float64) / n, cov=cov, shape=shape)


def set_moments(images, chunk=DEFAULT_CHUNK, splits=0, device=None):
    """The moments of a set of uint8 images [N, ...] (a host array or a tensor), flattened to [N, D]: a dict of
      n              the number of images
      sum [D], gram [D, D]   int64: the exact sums over the images of c and of c c^T, c = x - 128
      mean [D]       float64: 128 + sum / n
      cov [D, D]     float64: (n gram - sum sum^T) / (n (n - 1)), the unbiased covariance; the numerator is formed in
                     int64, where it is exact for n <= 2^24, and converted once
      shape          the shape of one image
    The set is uploaded `chunk` rows at a time and accumulated on the device; the answer does not depend on `chunk`.
    D must be a multiple of 64 in [64, 4096]; n = 1 has no covariance and is refused."""
    if not (isinstance(images, np.ndarray) or torch.is_tensor(images)) or str(images.dtype) not in ("uint8", "torch.uint8") \
            or len(images.shape) < 2:
        raise ValueError("set_moments: images is a uint8 array or tensor [N, ...], got "
                         f"{(images.dtype, tuple(images.shape)) if hasattr(images, 'dtype') else type(images).__name__}")
    if isinstance(chunk, bool) or not isinstance(chunk, (int, np.integer)) or not 1 <= chunk <= ops.MOMENTS_MAX_N:
        raise ValueError(f"set_moments: chunk is an int in [1, 2^24], got {chunk!r}")
    shape = tuple(images.shape[1:])
    x = images.reshape(images.shape[0], -1)
    N = x.shape[0]
    if not 2 <= N <= MAX_N:
        raise ValueError(f"set_moments: a covariance needs 2 <= n <= 2^24 images, got n = {N}")
    chunk = int(chunk)
    ops.set_moments_check(x[:min(chunk, N)], splits=splits)
    if device is None:
        device = x.device if torch.is_tensor(x) and x.is_cuda else torch.device("cuda", torch.cuda.current_device())
    out = None
    for lo in range(0, N, chunk):
        out = ops.set_moments_u8(_device_rows(x[lo:lo + chunk], device), out=out, splits=splits)
    return _moments_dict(N, out[0].cpu().numpy(), out[1].cpu().numpy(), shape)


def moments_from_integers(n, total, gram, shape=None):
    """the dict of `set_moments` from integers computed elsewhere (a file, another process)"""
    total = np.asarray(total)
    return _moments_dict(n, total, gram, shape if shape is not None else total.shape)


def _check_moments(m, name):
    if not isinstance(m, dict) or any(key not in m for key in ("n", "sum", "gram", "mean", "cov")):
        raise ValueError(f"moments: {name} is a dict of set_moments")
    return m


def merge_moments(a, b):
    """the moments of the union of two disjoint sets: their integers added"""
    _check_moments(a, "a"), _check_moments(b, "b")
    if a["sum"].shape != b["sum"].shape:
        raise ValueError(f"merge_moments: a has D = {a['sum'].shape[0]}, b has D = {b['sum'].shape[0]}")
    return _moments_dict(a["n"] + b["n"], a["sum"] + b["sum"], a["gram"] + b["gram"], a.get("shape", a["sum"].shape))


def save_moments(path, m, settings=None):
    """writes n, sum, gram, the image shape and `settings` (a dict, as JSON) to an .npz"""
    _check_moments(m, "m")
    if not str(path).endswith(".npz"):
        raise ValueError(f"save_moments: path names a .npz file, got {path!r}")
    with open(path, "wb") as f:
        np.savez(f, n=np.asarray(m["n"], dtype=np.int64), sum=m["sum"], gram=m["gram"],
                 shape=np.asarray(m.get("shape", m["sum"].shape), dtype=np.int64),
                 settings=np.array(json.dumps(settings or {}, sort_keys=True)))


def load_moments(path, return_settings=False):
    """the dict of `set_moments` from a file of `save_moments`"""
    with np.load(path) as z:
        if any(key not in z.files for key in ("n", "sum", "gram")):
            raise ValueError(f"load_moments: {path!r} holds no n, sum and gram")
        total = z["sum"]
        if total.dtype != np.int64 or z["gram"].dtype != np.int64:
            raise ValueError(f"load_moments: {path!r}: sum and gram are int64")
        shape = tuple(z["shape"]) if "shape" in z.files else total.shape
        m = _moments_dict(int(z["n"]), total, z["gram"], shape)
        settings = json.loads(str(z["settings"])) if "settings" in z.files else {}
    return (m, settings) if return_settings else m


def _eigh_clipped(s):
    """eigenvalues (ascending, clipped at 0) and eigenvectors of a symmetric positive semi-definite matrix.  The zero
    eigenvalues of a rank-deficient covariance (n < D) come back as +-D eps lambda_max of noise; a square root turns
    each into sqrt(eps), thousands of them into an error of 1e-8 of the trace, so eigenvalues below D eps lambda_max
    (the cut-off of numpy.linalg.matrix_rank) are taken as the zeros they are."""
    w, v = np.linalg.eigh((s + s.T) * 0.5)
    w = np.clip(w, 0.0, None)
    w[w <= w.shape[0] * np.finfo(np.float64).eps * w[-1]] = 0.0
    return w, v


def frechet_distance(a, b):
    """The Frechet distance of the Gaussians fitted to two sets (dicts of set_moments),
        |mu_a - mu_b|^2 + tr S_a + tr S_b - 2 tr (S_a^1/2 S_b S_a^1/2)^1/2,
    as a dict of `distance`, `mean_term` (the first summand) and `cov_term` (the rest).  Two symmetric eigendecompositions
    (numpy.linalg.eigh) with eigenvalues clipped at 0: S_a^1/2 from the first, the trace of the root of the symmetric
    S_a^1/2 S_b S_a^1/2 from the second -- not scipy's sqrtm of the non-symmetric S_a S_b -- which also handles the
    rank-deficient case n < D."""
    _check_moments(a, "a"), _check_moments(b, "b")
    if a["cov"].shape != b["cov"].shape:
        raise ValueError(f"frechet_distance: a has D = {a['cov'].shape[0]}, b has D = {b['cov'].shape[0]}")
    diff = a["mean"] - b["mean"]
    mean_term = float(diff @ diff)
    # the formula is symmetric in a and b, its rounding is not: the root is always taken of the covariance with the
    # larger trace, so that frechet_distance(a, b) and frechet_distance(b, a) are the same computation
    first, second = (a["cov"], b["cov"]) if np.trace(a["cov"]) >= np.trace(b["cov"]) else (b["cov"], a["cov"])
    wa, va = _eigh_clipped(first)
    root_a = (va * np.sqrt(wa)) @ va.T
    wm, _ = _eigh_clipped(root_a @ second @ root_a)
    cov_term = float(np.trace(a["cov"]) + np.trace(b["cov"]) - 2.0 * np.sqrt(wm).sum())
    return dict(distance=mean_term + cov_term, mean_term=mean_term, cov_term=cov_term)


def eigen_images(m, k=16):
    """The k leading eigen-images of a set (PCA in pixel space) from its moments: a dict of `eigenvalues` [k], descending,
    `ratio` [k], the share of the covariance's trace each holds, and `images` [k, *shape], the unit eigenvectors, each
    with the sign that makes its largest loading positive (the rule of pca_transformation, sklearn's svd_flip on v)."""
    _check_moments(m, "m")
    D = m["cov"].shape[0]
    if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or not 1 <= k <= D:
        raise ValueError(f"eigen_images: k is an int in [1, {D}], got {k!r}")
    w, v = _eigh_clipped(m["cov"])
    w, v = w[::-1][:k], v[:, ::-1][:, :k].T
    sign = np.sign(v[np.arange(k), np.abs(v).argmax(axis=1)])
    sign[sign == 0] = 1.0
    total = float(np.trace(m["cov"]))
    return dict(eigenvalues=w, ratio=w / total if total > 0 else np.zeros_like(w),
                images=(v * sign[:, None]).reshape((k,) + tuple(m.get("shape", (D,)))))


def compare_moments(a, b):
    """Two dicts of set_moments, a the samples and b the reference set, compared; host arithmetic only.
      distance, mean_term, cov_term   `frechet_distance`
      frechet_diag_pixel   sum over the sub-pixels of (mu_a - mu_b)^2 + (sigma_a - sigma_b)^2: the same distance with the
                           covariances cut to their diagonals, the formula of compare_spectra's frechet_diag on pixels
      trace_ratio          tr S_a / tr S_b: below 1, the samples vary less than the data
      eigenvalues_a, eigenvalues_b   the spectra of the two covariances, descending, clipped at 0
    These are PIXEL-space figures: they are not comparable with published feature-space numbers (FID and its kin) and
    are meant for comparing runs (samplers, step counts, grids) of ONE checkpoint against the same reference set."""
    out = frechet_distance(a, b)
    mu = a["mean"] - b["mean"]
    sd = np.sqrt(np.clip(np.diag(a["cov"]), 0, None)) - np.sqrt(np.clip(np.diag(b["cov"]), 0, None))
    tb = float(np.trace(b["cov"]))
    out.update(frechet_diag_pixel=float((mu * mu + sd * sd).sum()),
               trace_ratio=float(np.trace(a["cov"])) / tb if tb > 0 else float("nan"),
               eigenvalues_a=_eigh_clipped(a["cov"])[0][::-1].copy(), eigenvalues_b=_eigh_clipped(b["cov"])[0][::-1].copy())
    return out


def plot_eigen_images(m, k=16, cols=8, title=None):
    """a matplotlib figure of the k leading eigen-images of a set, each scaled to its own range, with its share of the
    variance; matplotlib is imported on use"""
    import matplotlib.pyplot as plt
    e = eigen_images(m, k)
    imgs = e["images"]
    rows = (k + cols - 1) // cols
    fig, axes = plt.subplots(rows, cols, figsize=(1.6 * cols, 1.8 * rows), squeeze=False)
    for i, ax in enumerate(axes.ravel()):
        ax.axis("off")
        if i < k:
            im = imgs[i] if imgs[i].ndim >= 2 else imgs[i][None]
            lo, hi = im.min(), im.max()
            ax.imshow((im - lo) / (hi - lo) if hi > lo else np.zeros_like(im))
            ax.set_title(f"{100 * e['ratio'][i]:.1f} %", fontsize=8)
    if title:
        fig.suptitle(title)
    return fig
