"""numpy oracle of mulan_spectrum (spectrum.hip): the orthonormal 32 x 32 DCT-II of image planes, its radial bins and
set sums, in float64 -- and an fp32 restatement of the kernel's arithmetic (D rounded to fp32, both products accumulated
in fp32 in k order) whose own error against float64 sets the GPU tolerances at 4x, the convention of
bound_profile_oracle.py.  The 4x covers an accumulation order inside the MFMA that the restatement does not reproduce
(it rounds every product; the matrix core fuses)."""
import numpy as np

S = 32
BINS = 45
GRAY = (0.2125, 0.7154, 0.0721)          # skimage.color.rgb2gray
MARGIN = 4.0


def dct_matrix():
    """float64 [32, 32]: D[u][y] = c_u cos(pi (2 y + 1) u / 64), c_0 = sqrt(1 / 32), c_u = sqrt(2 / 32)"""
    u, y = np.arange(S)[:, None], np.arange(S)[None, :]
    c = np.where(u == 0, np.sqrt(1.0 / S), np.sqrt(2.0 / S))
    return c * np.cos(np.pi * (2 * y + 1) * u / (2.0 * S))


def bin_table():
    """int [32, 32]: the r with r^2 - r < u^2 + v^2 <= r^2 + r, in integers; (0, 0) is bin 0"""
    out = np.zeros((S, S), dtype=np.int64)
    for u in range(S):
        for v in range(S):
            s = u * u + v * v
            hits = [r for r in range(BINS) if (s == 0 and r == 0) or (r * r - r < s <= r * r + r)]
            assert len(hits) == 1, (u, v, hits)
            out[u, v] = hits[0]
    return out


def read(x, scale=1.0, offset=0.0, dtype=np.float64):
    """the values the kernel transforms: uint8 as scale v + offset, floats as they are; [N, 32, 32, 3] in `dtype`"""
    x = np.asarray(x)
    if x.dtype == np.uint8:
        if dtype == np.float32:                       # fmaf(scale, v, offset): one rounding
            return (np.float64(np.float32(scale)) * x.astype(np.float64) + np.float64(np.float32(offset))).astype(np.float32)
        return np.float64(np.float32(scale)) * x.astype(np.float64) + np.float64(np.float32(offset))
    return x.astype(dtype)


def gray_mix(x):
    """[N, 32, 32, 3] -> [N, 32, 32, 1] in x's dtype, term by term in that dtype"""
    w = np.asarray(GRAY, dtype=np.float32).astype(x.dtype)       # the kernel's constants are fp32
    return ((x[..., 0] * w[0] + x[..., 1] * w[1]) + x[..., 2] * w[2])[..., None]


def planes(x, scale=1.0, offset=0.0, gray=False, dtype=np.float64):
    """[N, 32, 32, P] in `dtype`: what enters the transform"""
    v = read(x, scale, offset, dtype)
    return gray_mix(v) if gray else v


def coef(x, scale=1.0, offset=0.0, gray=False):
    """float64 [N, 32, 32, P]: Y[n, u, v, p] = sum_yx D[u, y] X[n, y, x, p] D[v, x]"""
    D = dct_matrix()
    return np.ascontiguousarray(np.einsum("uy,nyxp,vx->nuvp", D, planes(x, scale, offset, gray), D, optimize=True))


def coef_fp32(x, scale=1.0, offset=0.0, gray=False):
    """the fp32 restatement, float32 [N, 32, 32, P]: D rounded to fp32; T = D X then Y = T D^T, each a sum over k = 0..31
    in that order with every product and every partial sum rounded to fp32"""
    D = dct_matrix().astype(np.float32)
    X = planes(x, scale, offset, gray, np.float32)
    T = np.zeros_like(X)
    for k in range(S):
        T = T + D[None, :, k, None, None] * X[:, k, None, :, :]          # T[n, u, x, p] += D[u, k] X[n, k, x, p]
    Y = np.zeros_like(X)
    for k in range(S):
        Y = Y + T[:, :, k, None, :] * D[None, None, :, k, None]          # Y[n, u, v, p] += T[n, u, k, p] D[v, k]
    assert Y.dtype == np.float32
    return Y


def radial(c):
    """[N, 45, P] in c's dtype: the sum of c^2 over each bin's coefficients, in (u, v) order"""
    N, P = c.shape[0], c.shape[3]
    out = np.zeros((N, BINS, P), dtype=c.dtype)
    b = bin_table()
    sq = c * c
    for u in range(S):
        for v in range(S):
            out[:, b[u, v], :] += sq[:, u, v, :]
    return out


def set_sums(c):
    """(sum1, sum2), float64 [32, 32, P]: the sums over n of c and c^2 taken in float64 (the kernel's sums are fp64)"""
    c = c.astype(np.float64)
    return c.sum(axis=0), (c * c).sum(axis=0)


def ceiling(max_abs):
    """the analytic ceiling of a coefficient's fp32 error: two 32-term fp32 dot products with a rounded D whose absolute
    row sums are at most sqrt(32) each: 68 2^-24 32 max|x|"""
    return 68.0 * 2.0 ** -24 * 32.0 * float(max_abs)


def bounds(x, scale=1.0, offset=0.0, gray=False):
    """dict of the float64 answers and the tolerances for x: tol_* = 4 x the largest error the fp32 restatement makes on
    this input (per output), with the restatement's coefficient error checked against the analytic ceiling"""
    exact = coef(x, scale, offset, gray)
    approx = coef_fp32(x, scale, offset, gray)
    err = float(np.abs(approx - exact).max())
    top = ceiling(np.abs(planes(x, scale, offset, gray)).max())
    assert err <= top, (err, top)
    r_exact, r_approx = radial(exact), radial(approx)
    s_exact, s_approx = set_sums(exact), set_sums(approx)
    return dict(coef=exact, radial=r_exact, sum1=s_exact[0], sum2=s_exact[1], ceiling=top, err_coef=err,
                tol_coef=MARGIN * err,
                tol_radial=MARGIN * float(np.abs(r_approx - r_exact).max()),
                tol_sum1=MARGIN * float(np.abs(s_approx[0] - s_exact[0]).max()),
                tol_sum2=MARGIN * float(np.abs(s_approx[1] - s_exact[1]).max()))
