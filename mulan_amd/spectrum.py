"""Spatial frequency: the orthonormal 32 x 32 DCT of images (ops.spectrum, mulan_spectrum on the fp32 matrix cores) and
what is read off it -- the reference's dct2 (ldm/notebook_utils.py, there on skimage / scipy), the radial power spectrum
and the per-coefficient moments of an image set, the comparison of two such sets, and the spectrum of the learned noise
schedule's gamma maps.  Apart from dct2 none of it is in the reference.

u is the vertical frequency, v the horizontal one; radial bin r = floor(sqrt(u^2 + v^2) + 1/2) runs 0..44 and bin 0 is
the DC term alone.  `compare_spectra` is host arithmetic on two dicts, so it is tested without a device."""
import numpy as np
import torch

from . import ops

DEFAULT_CHUNK = 16384          # images per upload: 48 MiB of CIFAR-size images
BINS = ops.SPECTRUM_BINS
MODEL_SCALE, MODEL_OFFSET = 2.0 / 256.0, 1.0 / 256.0 - 1.0     # encode_u8: 2 (v + 1/2) / 256 - 1
HIGH_BAND = 16                 # compare_spectra's high band: bins r >= 16, half of the axis Nyquist


def radial_freq():
    """[45]: the bins' radii in cycles per pixel, r / 64 (a DCT-II index u is the frequency u / (2 * 32))"""
    return np.arange(BINS, dtype=np.float64) / 64.0


def _images(x, name, dtypes):
    """[32, 32, 3] or [n, 32, 32, 3], array or tensor, of one of `dtypes` -> (the same storage as [n, 32, 32, 3], batched)"""
    if not (isinstance(x, np.ndarray) or torch.is_tensor(x)):
        raise ValueError(f"{name}: a numpy array or tensor, got {type(x).__name__}")
    if str(x.dtype).replace("torch.", "") not in dtypes:
        raise ValueError(f"{name}: dtype {' or '.join(dtypes)}, got {x.dtype}")
    batched = len(x.shape) == 4
    if len(x.shape) == 3:
        x = x.reshape((1,) + tuple(x.shape))
    if len(x.shape) != 4 or tuple(x.shape[1:]) != (32, 32, 3) or x.shape[0] < 1:
        raise ValueError(f"{name}: [32, 32, 3] or [n >= 1, 32, 32, 3], got {tuple(x.shape)}")
    return x, batched


def _on_device(x, device):
    return (x if torch.is_tensor(x) else torch.from_numpy(np.ascontiguousarray(x))).to(device).contiguous()


def _default_device():
    return torch.device("cuda", torch.cuda.current_device())


def dct2(image, device=None):
    """notebook_utils.dct2: the orthonormal 2-D DCT of the grey image, numpy fp32 [32, 32], or [B, 32, 32] for a batch.
    image: uint8 (grey of v / 255, as skimage.color.rgb2gray reads uint8) or float32 (grey of the values as they are)
    [32, 32, 3] or [B, 32, 32, 3]."""
    x, batched = _images(image, "dct2", ("uint8", "float32"))
    ops.spectrum_check(x, gray=True, coef=True)
    if device is None:
        device = x.device if torch.is_tensor(x) and x.is_cuda else _default_device()
    coef, _, _ = ops.spectrum(_on_device(x, device), scale=1.0 / 255.0, offset=0.0, gray=True, coef=True)
    out = coef[..., 0].cpu().numpy()
    return out if batched else out[0]


def image_spectrum(images, gray=False, chunk=DEFAULT_CHUNK, keep_radial=False, device=None):
    """The spectrum of an image set, uint8 [N, 32, 32, 3] on the host, in the model's scale (encode_u8: 2 (v + 1/2) / 256
    - 1), uploaded `chunk` images at a time.  A dict of numpy arrays, P = 1 with gray, else 3:
      power_mean [32, 32, P]  the mean over the set of coef^2;  coef_mean, coef_var [32, 32, P] (population variance)
      radial_mean [45, P]     the mean radial power: power_mean summed over each bin
      radial_freq [45]        the bins' radii in cycles per pixel;  n  the number of images
      radial [N, 45, P]       with keep_radial: every image's radial power"""
    x, _ = _images(images, "image_spectrum", ("uint8",))
    if len(images.shape) != 4:
        raise ValueError(f"image_spectrum: a set [N, 32, 32, 3], got {tuple(images.shape)}")
    if isinstance(chunk, bool) or not isinstance(chunk, (int, np.integer)) or chunk < 1:
        raise ValueError(f"image_spectrum: chunk is a positive int, got {chunk!r}")
    if not isinstance(gray, bool) or not isinstance(keep_radial, bool):
        raise ValueError("image_spectrum: gray and keep_radial are bools")
    ops.spectrum_check(x, MODEL_SCALE, MODEL_OFFSET, gray, radial=keep_radial, sums=True)
    if device is None:
        device = _default_device()
    N = x.shape[0]
    sums, radial = None, []
    for lo in range(0, N, int(chunk)):
        _, rad, sums = ops.spectrum(_on_device(x[lo:lo + int(chunk)], device), scale=MODEL_SCALE, offset=MODEL_OFFSET,
                                    gray=gray, radial=keep_radial, sums=sums is None, accumulate_into=sums)
        if keep_radial:
            radial.append(rad.cpu().numpy())
    out = moments_from_sums(sums[0].cpu().numpy(), sums[1].cpu().numpy(), N)
    if keep_radial:
        out["radial"] = np.concatenate(radial)
    return out


def bin_table():
    """int [32, 32]: the radial bin of coefficient (u, v), the r with r^2 - r < u^2 + v^2 <= r^2 + r"""
    s = np.add.outer(np.arange(32) ** 2, np.arange(32) ** 2)
    r = np.arange(BINS)
    return np.searchsorted(r * r + r, s, side="left")


def moments_from_sums(sum1, sum2, n):
    """the dict of image_spectrum from the set sums [32, 32, P] of coef and coef^2 over n images"""
    sum1, sum2 = np.asarray(sum1, dtype=np.float64), np.asarray(sum2, dtype=np.float64)
    if sum1.ndim != 3 or sum1.shape[:2] != (32, 32) or sum2.shape != sum1.shape or n < 1:
        raise ValueError("moments_from_sums: sums [32, 32, P] and n >= 1")
    mean, power = sum1 / n, sum2 / n
    radial = np.zeros((BINS, sum1.shape[2]))
    np.add.at(radial, bin_table().reshape(-1), power.reshape(1024, -1))
    return dict(power_mean=power, coef_mean=mean, coef_var=np.maximum(power - mean * mean, 0.0), radial_mean=radial,
                radial_freq=radial_freq(), n=int(n))


def compare_spectra(a, b):
    """Two dicts of image_spectrum, a the samples and b the reference set, compared; host arithmetic only.
      log_ratio [45, P]   log10(a's radial_mean / b's)
      lsd_db              the log-spectral distance: the RMS over the AC bins (r >= 1) and planes of 10 log10 of that ratio
      high_band_ratio     the share of AC power in the bins r >= 16, a's share over b's: below 1, the samples lack detail
      frechet_diag        sum over the coefficients of (mu_a - mu_b)^2 + (sigma_a - sigma_b)^2, the Frechet distance of two
                          Gaussians with diagonal covariance in DCT space
    These are PIXEL-space figures: they are not comparable with published feature-space numbers (FID and its kin) and
    are meant for comparing runs (samplers, step counts, grids) of ONE checkpoint against the same reference set."""
    for name, d in (("a", a), ("b", b)):
        for key in ("radial_mean", "coef_mean", "coef_var"):
            if not isinstance(d, dict) or key not in d:
                raise ValueError(f"compare_spectra: {name} is a dict of image_spectrum (no {key!r})")
    ra, rb = np.asarray(a["radial_mean"], dtype=np.float64), np.asarray(b["radial_mean"], dtype=np.float64)
    if ra.ndim != 2 or ra.shape[0] != BINS or rb.shape != ra.shape or \
            np.shape(a["coef_mean"]) != np.shape(b["coef_mean"]):
        raise ValueError(f"compare_spectra: two spectra of the same planes, got radial_mean {ra.shape} and {rb.shape}")
    if not ((ra > 0).all() and (rb > 0).all()):
        raise ValueError("compare_spectra: a radial bin holds no power (a constant image set has no spectrum to compare)")
    log_ratio = np.log10(ra / rb)
    lsd = float(np.sqrt(np.mean((10.0 * log_ratio[1:]) ** 2)))
    share_a = ra[HIGH_BAND:].sum() / ra[1:].sum()
    share_b = rb[HIGH_BAND:].sum() / rb[1:].sum()
    mu = np.asarray(a["coef_mean"], dtype=np.float64) - np.asarray(b["coef_mean"], dtype=np.float64)
    sd = np.sqrt(np.asarray(a["coef_var"], dtype=np.float64)) - np.sqrt(np.asarray(b["coef_var"], dtype=np.float64))
    return dict(log_ratio=log_ratio, lsd_db=lsd, high_band_ratio=float(share_a / share_b),
                frechet_diag=float((mu * mu + sd * sd).sum()))


def schedule_spectrum(experiment, embeddings, time_steps=None):
    """At which spatial scale does the learned schedule vary?  The gamma maps of E embeddings at T times
    (ops.schedule_curves) go from the device straight into the DCT kernel as fp32 [E T, 32, 32, 3] images; no curve
    visits the host.  A dict of numpy arrays:
      radial [E, T, 45, 3]  the radial power of gamma(t) per channel
      ac_share [E, T, 3]    1 - DC power / total power: 0 for a spatially flat schedule
      radial_freq [45], time_steps [T]
    A model_vdm.VDM experiment (one scalar schedule) is refused."""
    from .evaluators import _schedule_chunks, _schedule_inputs
    emb, t = _schedule_inputs(experiment, embeddings, time_steps)
    cfg = experiment.model.config
    T = t.numel()
    out = []
    for _, a, b, c in _schedule_chunks(experiment, emb, T * 3072 * 4):
        gamma, _, _ = ops.schedule_curves(a, b, c, t, cfg.gamma_min, cfg.gamma_max)
        _, radial, _ = ops.spectrum(gamma.view(-1, 32, 32, 3), radial=True)
        out.append(radial.view(-1, T, BINS, 3).cpu().numpy())
    radial = np.concatenate(out)
    return dict(radial=radial, ac_share=ac_share(radial), radial_freq=radial_freq(), time_steps=t.cpu().numpy())


def ac_share(radial):
    """1 - DC power / total power over the bins' axis (the last but one) of radial [..., 45, P], in float64"""
    r = np.asarray(radial, dtype=np.float64)
    total = r.sum(axis=-2)
    return np.where(total > 0, r[..., 1:, :].sum(axis=-2) / np.where(total > 0, total, 1.0), 0.0)


def plot_spectra(spectra, labels=None, comparison=None):
    """the radial power (mean over the planes) of one or several dicts of image_spectrum over cycles per pixel, log-log;
    with `comparison` (compare_spectra of the first two) a second panel shows 10 log10 of their ratio in dB"""
    import matplotlib.pyplot as plt
    spectra = [spectra] if isinstance(spectra, dict) else list(spectra)
    labels = labels or [f"set {i}" for i in range(len(spectra))]
    fig, axes = plt.subplots(1, 2 if comparison is not None else 1, figsize=(5 * (2 if comparison is not None else 1), 3.5),
                             squeeze=False)
    ax = axes[0][0]
    for s, label in zip(spectra, labels):
        ax.loglog(s["radial_freq"][1:], np.asarray(s["radial_mean"])[1:].mean(axis=1), label=label)
    ax.set_xlabel("cycles per pixel")
    ax.set_ylabel("mean power per radial bin")
    ax.legend()
    if comparison is not None:
        ax = axes[0][1]
        ax.semilogx(radial_freq()[1:], 10.0 * np.asarray(comparison["log_ratio"])[1:])
        ax.axhline(0.0, color="k", linewidth=0.5)
        ax.set_xlabel("cycles per pixel")
        ax.set_ylabel("dB")
        ax.set_title(f"LSD {comparison['lsd_db']:.2f} dB, high band {comparison['high_band_ratio']:.3f}")
    return fig
