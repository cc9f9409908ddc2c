"""numpy oracle of mulan_image_fidelity (fidelity.hip): the squared errors in integers, the SSIM of Wang et al. (2004) with
the 11 x 11 Gaussian window of sigma 1.5 over the 22 x 22 windows inside a 32 x 32 image, in float64 -- and an fp32 twin of
the kernel's arithmetic whose own deviation from float64 sets the GPU tolerances at 4x, the convention of
spectrum_oracle.py: the kernel may order a sum differently from the twin, but it must not be a different algorithm.

The twin.  The same formula with every result rounded to fp32, the sums in the kernel's order and with the kernel's
centring (the moments are taken of x - 128, and 128 is put back into the means).  Where the kernel states a fused
multiply-add (fmaf: the filter chains after their first tap, the variances, the four factors of the quotient) the twin
fuses too: the product enters the sum unrounded and the sum is rounded once (`fma` below, through float64, where the
product of two fp32 is exact).  Elsewhere every product and every partial sum is rounded.  Fusing where the kernel
fuses makes the twin the kernel's own statement, so its deviation measures the kernel's formula and not a neighbour's.

The ceiling for identical pairs.  With a = b the twin's five maps coincide in pairs (mx = my, exx = eyy = exy), so
sxx = syy = sxy and n2 = d2 bit for bit, and the window's value is n1 n2 / (d1 d2) with n1 = fma(2 ux, ux, C1) and
d1 = fma(ux, ux, fma(ux, ux, C1)): 1 + 2 roundings in n1 and d1, one in each of the two products, one in the quotient --
6 roundings of relative size 2^-24 on a value of magnitude 1, so |map - 1| <= 6 2^-24.  The mean adds the 484 values in
10 + 43 additions (11 per thread, then the 44 partial sums), each rounded relative to a partial sum of at most 484, and
one division: (6 + 53 + 1) 2^-24 = 60 2^-24 on the mean.  `bounds` uses these two numbers where the twin's deviation is
exactly zero (it can be: a constant window gives n1 = d1), and 4 x the deviation everywhere else."""
import numpy as np

S = 32
W = 22
TAPS = 11
GRAY = (0.2125, 0.7154, 0.0721)          # skimage.color.rgb2gray; fp32 constants in the kernel
C1 = (0.01 * 255.0) ** 2
C2 = (0.03 * 255.0) ** 2
CENTRE = 128.0
MARGIN = 4.0
U = 2.0 ** -24
CEILING_MAP = 6 * U
CEILING_SSIM = 60 * U
f32, f64 = np.float32, np.float64


def taps():
    """float64 [11]: w_k = exp(-k^2 / 4.5) / sum, k = -5..5"""
    k = np.arange(TAPS, dtype=f64) - 5.0
    e = np.exp(-k * k / 4.5)
    return e / e.sum()


def pair_up(a, b, ia=None, ib=None):
    """the images of the M pairs, uint8 [M, 32, 32, 3] each, and which pairs have both indices in range"""
    a, b = np.asarray(a), np.asarray(b)
    assert a.dtype == np.uint8 and b.dtype == np.uint8 and a.shape[1:] == (S, S, 3) and b.shape[1:] == (S, S, 3)
    if ia is None and ib is None:
        assert len(a) == len(b)
    M = len(ia) if ia is not None else len(ib) if ib is not None else len(a)
    ia = np.arange(M) if ia is None else np.asarray(ia, dtype=np.int64)
    ib = np.arange(M) if ib is None else np.asarray(ib, dtype=np.int64)
    ok = (ia >= 0) & (ia < len(a)) & (ib >= 0) & (ib < len(b))
    return a[np.where(ok, ia, 0)], b[np.where(ok, ib, 0)], ok


def sse(a, b, ia=None, ib=None, mask=None):
    """(sse, sse_masked | None), int64 [M, 3]: the sums of (a - b)^2 per channel over all pixels and over the pixels whose
    mask (uint8 [32, 32] or [M, 32, 32]) is not 0; -1 for a pair with an index out of range"""
    x, y, ok = pair_up(a, b, ia, ib)
    d = x.astype(np.int64) - y.astype(np.int64)
    sq = d * d
    out = sq.sum(axis=(1, 2))
    out[~ok] = -1
    masked = None
    if mask is not None:
        m = np.asarray(mask) != 0
        m = np.broadcast_to(m if m.ndim == 3 else m[None], (len(x), S, S))
        masked = (sq * m[..., None]).sum(axis=(1, 2))
        masked[~ok] = -1
    return out, masked


def gray_mix(x):
    """float64 [M, 32, 32, 1] from float64 [M, 32, 32, 3]: the luma with the kernel's fp32 constants, not rounded"""
    w = np.asarray(GRAY, dtype=f32).astype(f64)
    return ((x[..., 0] * w[0] + x[..., 1] * w[1]) + x[..., 2] * w[2])[..., None]


def _windows(v, w):
    """[M, 32, 32, P] -> [M, 22, 22, P]: the separable filter over the windows inside the image"""
    h = sum(w[k] * v[:, :, k:k + W, :] for k in range(TAPS))
    return sum(w[k] * h[:, k:k + W, :, :] for k in range(TAPS))


def ssim_map(a, b, ia=None, ib=None, gray=False):
    """float64 [M, 22, 22, P]: biased moments; NaN for a pair with an index out of range.  The moments are taken of the
    grey levels less 128 and the means shifted back: the same numbers, and in float64 too the closer statement (at
    levels near 250 it stays within 3e-13 of an 80-bit evaluation, where E[x^2] - mu^2 of raw levels is 1e-12 off)"""
    x, y, ok = pair_up(a, b, ia, ib)
    x, y = x.astype(f64), y.astype(f64)
    if gray:
        x, y = gray_mix(x), gray_mix(y)
    x, y = x - CENTRE, y - CENTRE
    w = taps()
    mx, my = _windows(x, w), _windows(y, w)
    sxx, syy, sxy = _windows(x * x, w) - mx * mx, _windows(y * y, w) - my * my, _windows(x * y, w) - mx * my
    mx, my = mx + CENTRE, my + CENTRE
    out = ((2.0 * mx * my + C1) * (2.0 * sxy + C2)) / ((mx * mx + my * my + C1) * (sxx + syy + C2))
    out[~ok] = np.nan
    return out


def ssim(a, b, ia=None, ib=None, gray=False):
    """float64 [M, P]: the mean over the 484 windows"""
    return ssim_map(a, b, ia, ib, gray).mean(axis=(1, 2))


# ------------------------------------------------------------------------------------------------------- the fp32 twin
def fma(a, b, c):
    """fp32 fmaf(a, b, c): the product of two fp32 is exact in float64; one rounding of the sum to float64 and one to fp32
    (a double rounding that differs from the fused result only on a 2^-29 tie)"""
    return (np.asarray(a, dtype=f32).astype(f64) * np.asarray(b, dtype=f32).astype(f64)
            + np.asarray(c, dtype=f32).astype(f64)).astype(f32)


def _centred32(x, gray):
    """uint8 [M, 32, 32, 3] -> fp32 [M, 32, 32, P]: the plane less 128 as the kernel forms it"""
    v = x.astype(f32)
    if gray:
        r, g, b = (f32(c) for c in GRAY)
        luma = fma(b, v[..., 2], fma(g, v[..., 1], r * v[..., 0]))
        return (luma - f32(CENTRE))[..., None]
    return v - f32(CENTRE)


def _chain(v, axis, w):
    """out[j] = sum_k w[k] v[j + k], j = 0..21, along `axis`: the rounded product of tap 0, then fmaf in tap order"""
    take = lambda k: np.take(v, np.arange(k, k + W), axis=axis)      # noqa: E731
    s = w[0] * take(0)
    assert s.dtype == f32
    for k in range(1, TAPS):
        s = fma(w[k], take(k), s)
    return s


def ssim_map_fp32(a, b, ia=None, ib=None, gray=False):
    """fp32 [M, 22, 22, P]: the kernel's arithmetic"""
    x, y, ok = pair_up(a, b, ia, ib)
    fa, fb = _centred32(x, gray), _centred32(y, gray)
    w = taps().astype(f32)
    mx, my, exx, eyy, exy = (_chain(_chain(v, 2, w), 1, w) for v in (fa, fb, fa * fa, fb * fb, fa * fb))
    sxx, syy, sxy = fma(-mx, mx, exx), fma(-my, my, eyy), fma(-mx, my, exy)
    ux, uy = mx + f32(CENTRE), my + f32(CENTRE)
    c1, c2 = f32(C1), f32(C2)
    n1, n2 = fma(f32(2.0) * ux, uy, c1), fma(f32(2.0), sxy, c2)
    d1, d2 = fma(ux, ux, fma(uy, uy, c1)), (sxx + syy) + c2
    out = (n1 * n2) / (d1 * d2)
    assert out.dtype == f32
    out[~ok] = np.nan
    return out


def ssim_fp32(smap):
    """fp32 [M, P] from the twin's map: thread (half h2, column j) adds its 11 windows i = 11 h2 .. 11 h2 + 10 in order, the 44
    partial sums are added in (h2, j) order, and the sum is divided by 484"""
    total = None
    for h2 in range(2):
        for j in range(W):
            acc = smap[:, TAPS * h2, j, :]
            for i in range(1, TAPS):
                acc = acc + smap[:, TAPS * h2 + i, j, :]
            total = acc if total is None else total + acc
    out = total / f32(W * W)
    assert out.dtype == f32
    return out


def bounds(a, b, ia=None, ib=None, gray=False, mask=None):
    """dict of the float64 answers (ssim_map, ssim), the integer ones (sse, sse_masked) and the tolerances for this input:
    tol_map, tol_ssim = 4 x the twin's largest deviation from float64 over the pairs in range, or the analytic ceiling of
    the module docstring where that deviation is exactly zero"""
    exact_map = ssim_map(a, b, ia, ib, gray)
    twin_map = ssim_map_fp32(a, b, ia, ib, gray)
    exact, twin = exact_map.mean(axis=(1, 2)), ssim_fp32(twin_map)
    ok = ~np.isnan(exact[:, 0])
    dev_map = float(np.abs(twin_map[ok].astype(f64) - exact_map[ok]).max()) if ok.any() else 0.0
    dev_ssim = float(np.abs(twin[ok].astype(f64) - exact[ok]).max()) if ok.any() else 0.0
    s, sm = sse(a, b, ia, ib, mask)
    return dict(ssim_map=exact_map, ssim=exact, sse=s, sse_masked=sm, twin_map=twin_map, twin_ssim=twin,
                dev_map=dev_map, dev_ssim=dev_ssim,
                tol_map=MARGIN * dev_map if dev_map > 0.0 else CEILING_MAP,
                tol_ssim=MARGIN * dev_ssim if dev_ssim > 0.0 else CEILING_SSIM)
