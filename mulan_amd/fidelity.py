"""Image fidelity: how close is an image to the image it is meant to reproduce?  PSNR and SSIM of pairs of uint8 images
(ops.image_fidelity, mulan_image_fidelity), what they say about a restoration or an inpainting against the originals
and against the trivial baseline, and how much K restorations of one measurement differ among themselves.  None of it
is in the reference.

The squared errors are exact integers from the device and every PSNR is float64 host arithmetic on them
(`psnr_from_sse`), so it is tested without a device; the SSIM is that of Wang et al. (2004) with the 11 x 11 Gaussian
window of sigma 1.5 over the 22 x 22 windows inside the image (skimage's structural_similarity with gaussian_weights,
use_sample_covariance=False, data_range=255, cropped by 5), fp32 on the device."""
import numpy as np
import torch

from . import ops

DEFAULT_CHUNK = 16384          # pairs per upload: 96 MiB of CIFAR-size images
PEAK2 = 255.0 ** 2


def psnr_from_sse(sse, n):
    """10 log10(255^2 n / sse) in float64; n: the number of sub-pixels summed (scalar or array); inf where sse = 0, nan
    where n = 0 (nothing was summed)"""
    sse, n = np.asarray(sse, dtype=np.float64), np.asarray(n, dtype=np.float64)
    if (sse < 0).any() or (n < 0).any():
        raise ValueError("psnr_from_sse: sse and n are not negative")
    sse, n = np.broadcast_arrays(sse, n)
    out = np.full(sse.shape, np.nan)
    zero, some = (sse == 0) & (n > 0), (sse > 0) & (n > 0)
    out[zero] = np.inf
    out[some] = 10.0 * np.log10(PEAK2 * n[some] / sse[some])
    return out if out.ndim else float(out)


def _images(x, name):
    if not isinstance(x, np.ndarray) or x.dtype != np.uint8 or x.ndim != 4 or x.shape[1:] != (32, 32, 3) or len(x) < 1:
        raise ValueError(f"{name}: a uint8 numpy array [N >= 1, 32, 32, 3], got "
                         f"{(x.dtype, x.shape) if isinstance(x, np.ndarray) else type(x).__name__}")
    return x


def _mask(mask, N, name):
    """-> uint8 [32, 32] or [N, 32, 32] (non-zero: the pixel counts), or None"""
    if mask is None:
        return None
    m = np.asarray(mask)
    if m.dtype not in (np.bool_, np.uint8) or m.shape not in ((32, 32), (N, 32, 32)):
        raise ValueError(f"{name}: mask is bool or uint8 [32, 32] or [{N}, 32, 32], got {m.dtype} {m.shape}")
    return np.ascontiguousarray(m != 0).astype(np.uint8)


def _default_device():
    return torch.device("cuda", torch.cuda.current_device())


def _up(x, device):
    return torch.from_numpy(np.ascontiguousarray(x)).to(device)


def image_fidelity(a, b, mask=None, gray=False, chunk=DEFAULT_CHUNK, keep_map=False, device=None):
    """PSNR and SSIM of the pairs (a[n], b[n]), uint8 [N, 32, 32, 3] on the host, uploaded `chunk` pairs at a time.  A dict
    of numpy arrays, P = 1 with gray (the SSIM of the luma), else 3:
      mse [N, 3]          the mean squared error per channel;  psnr [N]  over all three channels, inf for equal images
      ssim [N]            the mean over the planes of ssim_planes [N, P]
      psnr_masked [N]     with a mask (bool or uint8, [32, 32] for all pairs or [N, 32, 32]): the PSNR over the pixels
                          where the mask is set; nan for a pair whose mask is empty
      ssim_map [N, 22, 22, P]   with keep_map
    The result does not depend on chunk."""
    a, b = _images(a, "image_fidelity: a"), _images(b, "image_fidelity: b")
    if len(a) != len(b):
        raise ValueError(f"image_fidelity: a has {len(a)} images, b has {len(b)}")
    if isinstance(chunk, bool) or not isinstance(chunk, (int, np.integer)) or chunk < 1:
        raise ValueError(f"image_fidelity: chunk is a positive int, got {chunk!r}")
    if not isinstance(gray, bool) or not isinstance(keep_map, bool):
        raise ValueError("image_fidelity: gray and keep_map are bools")
    N = len(a)
    m = _mask(mask, N, "image_fidelity")
    ops.image_fidelity_check(a, b, None, None, gray, m, True, True, keep_map)
    if device is None:
        device = _default_device()
    shared = _up(m, device) if m is not None and m.ndim == 2 else None
    sse, masked, planes, maps = [], [], [], []
    for lo in range(0, N, int(chunk)):
        hi = min(N, lo + int(chunk))
        mk = shared if m is None or m.ndim == 2 else _up(m[lo:hi], device)
        s, sm, q, qm = ops.image_fidelity(_up(a[lo:hi], device), _up(b[lo:hi], device), gray=gray, mask=mk, ssim_map=keep_map)
        sse.append(s.cpu().numpy())
        planes.append(q.cpu().numpy())
        if m is not None:
            masked.append(sm.cpu().numpy())
        if keep_map:
            maps.append(qm.cpu().numpy())
    sse, planes = np.concatenate(sse).astype(np.int64), np.concatenate(planes)
    out = dict(mse=sse / 1024.0, psnr=psnr_from_sse(sse.sum(axis=1), 3072), ssim=planes.astype(np.float64).mean(axis=1),
               ssim_planes=planes)
    if m is not None:
        count = m.reshape(-1, 1024).astype(np.int64).sum(axis=1)                  # [1] or [N] pixels
        out["psnr_masked"] = psnr_from_sse(np.concatenate(masked).astype(np.int64).sum(axis=1), np.broadcast_to(3 * count, (N,)))
    if keep_map:
        out["ssim_map"] = np.concatenate(maps)
    return out


def baseline(originals, degradation):
    """A+ y of the originals, uint8 [N, 32, 32, 3]: the measurement of `degradation` ('sr:f', 'gray', 'sr:f+gray' or a pair
    (f, gray): f x f block means per channel, gray the channel mean) replicated back to 32 x 32 x 3 and rounded to
    the nearest level (halves up) -- what a restoration has to beat.  Host arithmetic in float64 on the levels: the
    model's scale is affine in them, so the means are the same"""
    from .sampling import parse_degradation
    x = _images(originals, "baseline: originals")
    f, gray = parse_degradation(degradation)
    y = x.astype(np.float64).reshape(len(x), 32 // f, f, 32 // f, f, 3).mean(axis=(2, 4))
    if gray:
        y = np.repeat(y.mean(axis=3, keepdims=True), 3, axis=3)
    y = np.repeat(np.repeat(y, f, axis=1), f, axis=2)
    return np.clip(np.floor(y + 0.5), 0, 255).astype(np.uint8)


SUMMARY_KEYS = ("psnr", "ssim")


def _summarise(out, prefix, res):
    for key in SUMMARY_KEYS + (("psnr_masked",) if "psnr_masked" in res else ()):
        v = res[key]
        out[prefix + key] = v
        finite = v[np.isfinite(v)]
        # an equal pair has PSNR inf and an empty mask nan: the mean and median are over the finite values
        out[prefix + key + "_mean"] = float(finite.mean()) if finite.size else float("nan")
        out[prefix + key + "_median"] = float(np.median(finite)) if finite.size else float("nan")
    out[prefix + "mse"], out[prefix + "ssim_planes"] = res["mse"], res["ssim_planes"]


def restoration_quality(originals, restored, degradation=None, mask=None, gray=False, chunk=DEFAULT_CHUNK, device=None):
    """Per-image PSNR and SSIM of `restored` against `originals` (uint8 [N, 32, 32, 3]).  A dict:
      psnr, ssim [N], mse [N, 3], ssim_planes [N, P], and psnr_mean / psnr_median / ssim_mean / ssim_median (over the
      finite values: an exact reproduction has PSNR inf)
      with mask (inpainting: True = kept, as `inpaint` takes it; [32, 32] or [N, 32, 32]): psnr_masked [N] over the
      UNKNOWN pixels (the mask inverted), its mean and median
      with degradation ('sr:f', 'gray', 'sr:f+gray'): the same figures prefixed `baseline_` for A+ y, the degraded original
      replicated back (`baseline`), the array `baseline_images`, and psnr_gain / ssim_gain [N] (restored less baseline;
      nan where both PSNR are inf) with psnr_gain_mean / ssim_gain_mean: what the sampler adds to the measurement"""
    originals, restored = _images(originals, "restoration_quality: originals"), _images(restored, "restoration_quality: restored")
    if len(originals) != len(restored):
        raise ValueError(f"restoration_quality: {len(originals)} originals, {len(restored)} restored images")
    unknown = None
    if mask is not None:
        unknown = 1 - _mask(mask, len(originals), "restoration_quality")
    kw = dict(mask=unknown, gray=gray, chunk=chunk, device=device)
    out = {}
    _summarise(out, "", image_fidelity(restored, originals, **kw))
    if degradation is not None:
        base = baseline(originals, degradation)
        _summarise(out, "baseline_", image_fidelity(base, originals, **kw))
        out["baseline_images"] = base
        for key in SUMMARY_KEYS:
            with np.errstate(invalid="ignore"):
                gain = out[key] - out["baseline_" + key]
            out[key + "_gain"] = gain
            finite = gain[np.isfinite(gain)]
            out[key + "_gain_mean"] = float(finite.mean()) if finite.size else float("nan")
    return out


def pair_indices(K, N):
    """(ia, ib), int32 [N K (K - 1) / 2]: the rows of draws.reshape(K N, ...) of the pairs (k, l), k < l, of measurement n, the
    pairs of one measurement together, in (k, l) order"""
    k, l = np.triu_indices(K, 1)
    n = np.arange(N)[:, None]
    return (k[None, :] * N + n).reshape(-1).astype(np.int32), (l[None, :] * N + n).reshape(-1).astype(np.int32)


def diversity(draws, gray=False, device=None):
    """How much do K restorations of one measurement differ?  draws: uint8 [K >= 2, N, 32, 32, 3].  The set is uploaded
    once and the K (K - 1) / 2 pairs per measurement are addressed by index on the device.  A dict:
      ssim, psnr [N]      the mean pairwise SSIM (over the planes) and PSNR of each measurement's draws (PSNR inf for
                          identical draws); high values mean the draws agree
      pair_ssim, pair_psnr [N, K (K - 1) / 2]   the pairs in (k, l) order, k < l;  pairs [K (K - 1) / 2, 2]  the (k, l)"""
    if not isinstance(draws, np.ndarray) or draws.dtype != np.uint8 or draws.ndim != 5 or draws.shape[0] < 2 \
            or draws.shape[1] < 1 or draws.shape[2:] != (32, 32, 3):
        raise ValueError(f"diversity: draws is a uint8 numpy array [K >= 2, N >= 1, 32, 32, 3], got "
                         f"{(draws.dtype, draws.shape) if isinstance(draws, np.ndarray) else type(draws).__name__}")
    if not isinstance(gray, bool):
        raise ValueError("diversity: gray is a bool")
    K, N = draws.shape[:2]
    ia, ib = pair_indices(K, N)
    flat = draws.reshape(K * N, 32, 32, 3)
    ops.image_fidelity_check(flat, flat, ia, ib, gray)
    if device is None:
        device = _default_device()
    x = _up(flat, device)
    sse, _, planes, _ = ops.image_fidelity(x, x, ia=_up(ia, device), ib=_up(ib, device), gray=gray)
    pairs = K * (K - 1) // 2
    psnr = psnr_from_sse(sse.cpu().numpy().astype(np.int64).sum(axis=1), 3072).reshape(N, pairs)
    ssim = planes.cpu().numpy().astype(np.float64).mean(axis=1).reshape(N, pairs)
    return dict(ssim=ssim.mean(axis=1), psnr=psnr.mean(axis=1), pair_ssim=ssim, pair_psnr=psnr,
                pairs=np.stack(np.triu_indices(K, 1), axis=1))


def plot_fidelity(originals, restored, result, rows=8):
    """the rows // 2 worst and rows - rows // 2 best cases by SSIM, each as original | restored | SSIM map (the mean over
    the planes; `result` of image_fidelity(restored, originals, keep_map=True), or of restoration_quality, whose maps
    are then left out)"""
    import matplotlib.pyplot as plt
    order = np.argsort(result["ssim"])
    rows = min(int(rows), len(order))
    pick = list(order[:rows // 2]) + list(order[len(order) - (rows - rows // 2):])
    maps = result.get("ssim_map")
    cols = 3 if maps is not None else 2
    fig, axes = plt.subplots(rows, cols, figsize=(2 * cols, 2 * rows), squeeze=False)
    for r, n in enumerate(pick):
        axes[r][0].imshow(originals[n])
        axes[r][1].imshow(restored[n])
        axes[r][1].set_title(f"PSNR {result['psnr'][n]:.2f} dB, SSIM {result['ssim'][n]:.3f}", fontsize=7)
        if maps is not None:
            axes[r][2].imshow(np.asarray(maps[n]).mean(axis=-1), vmin=0.0, vmax=1.0, cmap="gray")
        for ax in axes[r]:
            ax.axis("off")
    return fig
