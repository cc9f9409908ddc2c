"""Are the samples new?  Exact nearest neighbours of uint8 images in pixel space (ops.knn_u8, mulan_knn_u8 on the int8
matrix cores) and what is read off them: the nearest training image of every sample, the nearest other sample, the
share of duplicates, and k-NN precision and recall (Kynkaanniemi et al., 2019) between two image sets.  Not in the
reference.

Everything here is integer arithmetic on squared distances (dist2 = sum of squared differences of grey levels); `rms`
figures are sqrt(dist2 / D), the root-mean-square difference per sub-pixel in grey levels.  The host reductions
(`novelty_from_lists`, `shares_from_covered`, `nearest_other`) take precomputed lists, so they are tested without a device."""
import numpy as np
import torch

from . import ops

DEFAULT_CHUNK = 16384          # reference rows per upload: 48 MiB of CIFAR-size images


def as_rows(x, name="images"):
    """uint8 [*, 32, 32, 3] or [*, D], array or tensor -> the same storage as [n, D]"""
    if not (isinstance(x, np.ndarray) or torch.is_tensor(x)):
        raise ValueError(f"{name}: a uint8 numpy array or tensor, got {type(x).__name__}")
    if str(x.dtype) not in ("uint8", "torch.uint8"):
        raise ValueError(f"{name}: uint8 images, got dtype {x.dtype}")
    if len(x.shape) == 4 and tuple(x.shape[1:]) == (32, 32, 3):
        x = x.reshape(x.shape[0], 32 * 32 * 3)
    if len(x.shape) != 2 or x.shape[0] < 1:
        raise ValueError(f"{name}: [n, 32, 32, 3] or [n, D] with n >= 1, got {tuple(x.shape)}")
    return x


def _device_rows(x, device):
    return (x if torch.is_tensor(x) else torch.from_numpy(np.ascontiguousarray(x))).to(device).contiguous()


def nearest(queries, reference, k=5, exclude_self=False, chunk=DEFAULT_CHUNK, radius2=None, splits=0, device=None):
    """(dist2, idx), int32 numpy [Q, k]: the k nearest rows of `reference` to every row of `queries`, ascending, equal
    distances to the smaller index, (2^31 - 1, -1) where fewer than k qualify.  The reference, a host array of any
    length, is uploaded `chunk` rows at a time and accumulated; the answer does not depend on `chunk`.
    exclude_self: query i IS reference i (a set against itself) and is not its own neighbour.
    radius2 (int32 [N]): also returns covered (bool [Q]): some reference j has dist2(i, j) <= radius2[j]."""
    q, r = as_rows(queries, "queries"), as_rows(reference, "reference")
    if isinstance(chunk, bool) or not isinstance(chunk, (int, np.integer)) or chunk < 1:
        raise ValueError(f"nearest: chunk is a positive int, got {chunk!r}")
    if radius2 is not None:
        radius2 = np.asarray(radius2.cpu() if torch.is_tensor(radius2) else radius2)
        if radius2.dtype != np.int32 or radius2.shape != (r.shape[0],):
            raise ValueError(f"nearest: radius2 is int32 [{r.shape[0]}], got {radius2.dtype} {radius2.shape}")
    ops.knn_check(q, r[:min(chunk, r.shape[0])], k, splits=splits)
    if exclude_self and q.shape[0] != r.shape[0]:
        raise ValueError(f"nearest: exclude_self compares a set with itself, got {q.shape[0]} and {r.shape[0]} rows")
    if device is None:
        device = q.device if torch.is_tensor(q) and q.is_cuda else torch.device("cuda", torch.cuda.current_device())
    qd = _device_rows(q, device)
    Q, N = q.shape[0], r.shape[0]
    dist2 = torch.full((Q, k), ops.KNN_EMPTY[0], device=device, dtype=torch.int32)
    idx = torch.full((Q, k), ops.KNN_EMPTY[1], device=device, dtype=torch.int32)
    covered = torch.zeros(Q, device=device, dtype=torch.uint8) if radius2 is not None else None
    for lo in range(0, N, chunk):
        hi = min(N, lo + chunk)
        rad = torch.from_numpy(np.ascontiguousarray(radius2[lo:hi])).to(device) if radius2 is not None else None
        ops.knn_u8(qd, _device_rows(r[lo:hi], device), k, idx_base=lo, self_offset=0 if exclude_self else -1,
                   out=(dist2, idx), radius2=rad, covered=covered, splits=splits)
    if radius2 is None:
        return dist2.cpu().numpy(), idx.cpu().numpy()
    return dist2.cpu().numpy(), idx.cpu().numpy(), covered.cpu().numpy().astype(bool)


def rms(dist2, D):
    """sqrt(dist2 / D) in grey levels; the empty slot gives inf"""
    d = np.asarray(dist2, dtype=np.float64)
    return np.where(np.asarray(dist2) == ops.KNN_EMPTY[0], np.inf, np.sqrt(d / D))


def nearest_other(dist2, idx, own):
    """(dist2, idx) [M] of the nearest row that is not row own[i] itself, from the lists [M, >= 2] of rows own [M] searched
    in the set they come from WITHOUT exclusion: the first entry whose index is not own[i].  If a row is not in its own
    first two slots, both hold exact duplicates of it with smaller indices, and the first is still the answer."""
    dist2, idx, own = np.asarray(dist2), np.asarray(idx), np.asarray(own)
    if dist2.ndim != 2 or dist2.shape[1] < 2 or idx.shape != dist2.shape or own.shape != dist2.shape[:1]:
        raise ValueError("nearest_other: lists [M, >= 2] and own [M]")
    pick = (idx[:, 0] == own).astype(np.int64)
    rows = np.arange(len(own))
    return dist2[rows, pick], idx[rows, pick]


def novelty_from_lists(nn_dist2, nn_idx, self_dist2, self_idx, train_self_dist2, D, duplicate_rms=1.0):
    """the dict of `novelty` from its lists: nn_* [S, k] into the training set, self_* [S] the nearest other sample,
    train_self_dist2 [M] the nearest other training image of the yardstick subset"""
    nn_dist2, nn_idx = np.asarray(nn_dist2), np.asarray(nn_idx)
    self_dist2, self_idx = np.asarray(self_dist2).reshape(-1), np.asarray(self_idx).reshape(-1)
    if nn_dist2.ndim != 2 or nn_idx.shape != nn_dist2.shape or self_dist2.shape != nn_dist2.shape[:1] or \
            self_idx.shape != self_dist2.shape:
        raise ValueError("novelty_from_lists: nn lists [S, k], self lists [S]")
    if not duplicate_rms >= 0:
        raise ValueError(f"novelty_from_lists: duplicate_rms >= 0, got {duplicate_rms}")
    self_rms = rms(self_dist2, D)
    # self_rms <= duplicate_rms in integers: dist2 <= duplicate_rms^2 D
    dup = self_dist2.astype(np.int64) <= np.floor(float(duplicate_rms) ** 2 * D + 1e-9)
    dup &= self_dist2 != ops.KNN_EMPTY[0]
    return dict(nn_idx=nn_idx, nn_dist2=nn_dist2, nn_rms=rms(nn_dist2[:, 0], D), self_idx=self_idx, self_dist2=self_dist2,
                self_rms=self_rms, duplicates=float(dup.mean()), duplicate_rms=float(duplicate_rms),
                train_self_rms=rms(np.asarray(train_self_dist2).reshape(-1), D))


def novelty(samples, train, k=5, duplicate_rms=1.0, yardstick=1000, seed=0, chunk=DEFAULT_CHUNK, device=None):
    """Are `samples` copies of `train` images, or of one another?  A dict of numpy arrays:
      nn_idx, nn_dist2 [S, k]  the k nearest training images of every sample;  nn_rms [S] = sqrt(nn_dist2[:, 0] / D)
      self_idx, self_dist2, self_rms [S]  the nearest OTHER sample
      duplicates      the share of samples whose nearest other sample is within duplicate_rms grey levels RMS
      duplicate_rms   that threshold, as given
      train_self_rms [M], train_subset [M]  the RMS distance from each of M = min(yardstick, len(train)) training images,
                      drawn without replacement under `seed`, to its nearest OTHER training image: what nn_rms of a fresh
                      image from the data distribution looks like, the yardstick to read nn_rms against."""
    s, t = as_rows(samples, "samples"), as_rows(train, "train")
    if s.shape[1] != t.shape[1]:
        raise ValueError(f"novelty: samples have D = {s.shape[1]}, train has D = {t.shape[1]}")
    if s.shape[0] < 2 or t.shape[0] < 2:
        raise ValueError("novelty: at least two samples and two training images")
    if isinstance(yardstick, bool) or not isinstance(yardstick, (int, np.integer)) or yardstick < 1:
        raise ValueError(f"novelty: yardstick is a positive int, got {yardstick!r}")
    ops.knn_check(s, t[:1], k)
    D = s.shape[1]
    nn_dist2, nn_idx = nearest(s, t, k, chunk=chunk, device=device)
    self_dist2, self_idx = nearest(s, s, 1, exclude_self=True, chunk=chunk, device=device)
    subset = np.sort(np.random.default_rng(seed).choice(t.shape[0], size=min(yardstick, t.shape[0]), replace=False))
    t_host = t.cpu().numpy() if torch.is_tensor(t) else t
    td2, tidx = nearest(t_host[subset], t, 2, chunk=chunk, device=device)
    out = novelty_from_lists(nn_dist2, nn_idx, self_dist2[:, 0], self_idx[:, 0], nearest_other(td2, tidx, subset)[0], D,
                             duplicate_rms)
    out["train_subset"] = subset
    return out


def shares_from_covered(covered_samples, covered_real):
    """(precision, recall): the share of samples inside the real set's balls, of real images inside the samples' balls"""
    cs, cr = np.asarray(covered_samples).astype(bool), np.asarray(covered_real).astype(bool)
    if cs.ndim != 1 or cr.ndim != 1 or not len(cs) or not len(cr):
        raise ValueError("shares_from_covered: two non-empty 1-D arrays")
    return float(cs.mean()), float(cr.mean())


def radii_from_lists(dist2, k):
    """int32 [n]: the squared distance to the k-th nearest other row, from within-set lists [n, >= k] (self excluded)"""
    dist2 = np.asarray(dist2)
    if dist2.ndim != 2 or dist2.shape[1] < k:
        raise ValueError(f"radii_from_lists: lists [n, >= {k}]")
    r = np.ascontiguousarray(dist2[:, k - 1], dtype=np.int32)
    if (r == ops.KNN_EMPTY[0]).any():
        raise ValueError(f"radii_from_lists: a row has fewer than {k} other rows")
    return r


def precision_recall(samples, real, k=3, chunk=DEFAULT_CHUNK, device=None):
    """k-NN precision and recall (Kynkaanniemi et al., 2019) IN PIXEL SPACE.  Around every image of a set lies the ball
    whose radius is the distance to its k-th nearest other image of that set.  precision: the share of samples inside
    some ball of the real set; recall: the share of real images inside some ball of the sample set.  Exact integers, one
    answer per pair of sets.
    Pixel space is not a feature space: the numbers are NOT comparable with published precision / recall, which are
    measured on network features.  They are meant for comparing runs (samplers, step counts, grids) of ONE checkpoint
    against the same real set.  Returns dict(precision, recall, k, radius2_real [R], radius2_samples [S],
    covered_samples [S], covered_real [R])."""
    s, t = as_rows(samples, "samples"), as_rows(real, "real")
    if s.shape[1] != t.shape[1]:
        raise ValueError(f"precision_recall: samples have D = {s.shape[1]}, real has D = {t.shape[1]}")
    ops.knn_check(s, t[:1], k)
    if min(s.shape[0], t.shape[0]) < k + 1:
        raise ValueError(f"precision_recall: each set needs more than k = {k} images")
    rad_real = radii_from_lists(nearest(t, t, k, exclude_self=True, chunk=chunk, device=device)[0], k)
    rad_samp = radii_from_lists(nearest(s, s, k, exclude_self=True, chunk=chunk, device=device)[0], k)
    cov_s = nearest(s, t, 1, radius2=rad_real, chunk=chunk, device=device)[2]
    cov_r = nearest(t, s, 1, radius2=rad_samp, chunk=chunk, device=device)[2]
    precision, recall = shares_from_covered(cov_s, cov_r)
    return dict(precision=precision, recall=recall, k=int(k), radius2_real=rad_real, radius2_samples=rad_samp,
                covered_samples=cov_s, covered_real=cov_r)


def plot_neighbours(samples, train, result, rows=8, order="suspicious"):
    """rows of a sample beside its k nearest training images (result: the dict of `novelty`); order 'suspicious' shows the
    samples with the smallest nn_rms first, 'first' the first ones"""
    import matplotlib.pyplot as plt
    s, t = as_rows(samples, "samples"), as_rows(train, "train")
    s = s.cpu().numpy() if torch.is_tensor(s) else s
    t = t.cpu().numpy() if torch.is_tensor(t) else t
    which = np.argsort(result["nn_rms"], kind="stable")[:rows] if order == "suspicious" else np.arange(min(rows, len(s)))
    k = result["nn_idx"].shape[1]
    fig, axes = plt.subplots(len(which), k + 1, figsize=(1.2 * (k + 1), 1.2 * len(which)), squeeze=False)
    for a, i in enumerate(which):
        panels = [(s[i], f"sample {i}")] + [(t[j], f"{float(rms(result['nn_dist2'][i, n], s.shape[1])):.1f}")
                                            for n, j in enumerate(result["nn_idx"][i]) if j >= 0]
        for b in range(k + 1):
            ax = axes[a][b]
            ax.set_xticks([])
            ax.set_yticks([])
            if b < len(panels):
                ax.imshow(panels[b][0].reshape(32, 32, 3), interpolation="nearest")
                ax.set_title(panels[b][1], fontsize=6)
    return fig
