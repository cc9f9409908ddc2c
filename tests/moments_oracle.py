"""numpy float64 oracle of the set moments (mulan_set_moments_u8, mulan_amd/moments.py) and of the Frechet distance.

Integer moments.  c = x - 128 as float64 and `c.T @ c` through BLAS: every product is an integer of at most 2^14 and every
partial sum an integer of at most N 2^14, which float64 holds exactly while N 2^14 < 2^53 (N < 2^39; asserted below), so
the result is exact whatever order BLAS adds in.  numpy's int64 matmul has no BLAS behind it and is far too slow even at
D = 3072 with a few thousand rows; `integer_moments_loops` is that plain int64 form, for cross-checking at D = 64.

Frechet distance.  Stated independently of the product's two-eigh form, as the well-known recipe
    |mu_a - mu_b|^2 + tr S_a + tr S_b - 2 tr sqrtm(S_a S_b)
with scipy.linalg.sqrtm of the non-symmetric product (the real part of its trace), trustworthy for well-conditioned
covariances (n > D)."""
import numpy as np


def integer_moments(x):
    """(sum [D], gram [D, D]) int64 of c = x - 128, x uint8 [N, D]; exact (see the header)"""
    x = np.asarray(x)
    assert x.dtype == np.uint8 and x.ndim == 2
    assert x.shape[0] * 2 ** 14 < 2 ** 53
    c = x.astype(np.float64) - 128.0
    gram = c.T @ c
    total = c.sum(axis=0)
    assert np.all(gram == np.rint(gram)) and np.all(total == np.rint(total))
    return total.astype(np.int64), gram.astype(np.int64)


def integer_moments_loops(x):
    """the same in plain int64 arithmetic, one row at a time"""
    c = np.asarray(x).astype(np.int64) - 128
    D = c.shape[1]
    total, gram = np.zeros(D, np.int64), np.zeros((D, D), np.int64)
    for row in c:
        total += row
        gram += row[:, None] * row[None, :]
    return total, gram


def mean_cov(n, total, gram):
    """(mean, cov) float64 from the integers: 128 + sum / n and (n gram - sum sum^T) / (n (n - 1)), the numerator in Python
    integers (arbitrary precision), converted once"""
    total = np.asarray(total).astype(object)
    num = int(n) * np.asarray(gram).astype(object) - np.outer(total, total)
    return 128.0 + total.astype(np.float64) / n, num.astype(np.float64) / (float(n) * float(n - 1))


def frechet_sqrtm(mu_a, cov_a, mu_b, cov_b):
    """(distance, mean_term, cov_term) by the sqrtm recipe"""
    from scipy.linalg import sqrtm
    d = np.asarray(mu_a, np.float64) - np.asarray(mu_b, np.float64)
    root = sqrtm(np.asarray(cov_a, np.float64) @ np.asarray(cov_b, np.float64))
    mean_term = float(d @ d)
    cov_term = float(np.trace(cov_a) + np.trace(cov_b) - 2.0 * np.trace(root).real)
    return mean_term + cov_term, mean_term, cov_term


def frechet_of_sets(xa, xb):
    """the sqrtm recipe on two uint8 sets [n, D], through this file's integers"""
    ma = mean_cov(len(xa), *integer_moments(xa))
    mb = mean_cov(len(xb), *integer_moments(xb))
    return frechet_sqrtm(ma[0], ma[1], mb[0], mb[1])


def frechet_low_rank(xa, xb):
    """(distance, mean_term, cov_term) of two uint8 sets [n, D] where the covariances are rank-deficient (n < D) and sqrtm
    of the singular product S_a S_b is not trustworthy: with C the centred rows over sqrt(n - 1), S = C^T C, the non-zero
    eigenvalues of S_a S_b are the squared singular values of C_a C_b^T, so tr sqrtm(S_a S_b) is their sum (one small
    SVD, no root of a zero eigenvalue); the traces are the sums of squares of C"""
    xa, xb = np.asarray(xa, np.float64), np.asarray(xb, np.float64)
    ca = (xa - xa.mean(axis=0)) / np.sqrt(len(xa) - 1.0)
    cb = (xb - xb.mean(axis=0)) / np.sqrt(len(xb) - 1.0)
    d = xa.mean(axis=0) - xb.mean(axis=0)
    mean_term = float(d @ d)
    cov_term = float((ca * ca).sum() + (cb * cb).sum() - 2.0 * np.linalg.svd(ca @ cb.T, compute_uv=False).sum())
    return mean_term + cov_term, mean_term, cov_term


def eigenvalues(cov):
    """descending, clipped at 0"""
    return np.clip(np.linalg.eigvalsh(np.asarray(cov, np.float64)), 0.0, None)[::-1]


def smoothed_bytes(seed, n, D, scale=40.0, width=3, lo=16, hi=239, offset=0.0):
    """uint8 [n, D]: Gaussian noise smoothed along D with a circular box of `width`, scaled, rounded, kept inside [lo, hi]
    (so that a shift by up to 16 grey levels does not clip): correlated, full-rank sets for n > D"""
    rng = np.random.default_rng(seed)
    z = rng.standard_normal((n, D))
    s = sum(np.roll(z, k, axis=1) for k in range(width)) / np.sqrt(width)
    gain = 1.0 + 0.5 * np.sin(np.arange(D) * 0.37 + seed)      # the variance differs from column to column and set to set
    return np.clip(np.rint(128.0 + offset + scale * gain * s), lo, hi).astype(np.uint8)
