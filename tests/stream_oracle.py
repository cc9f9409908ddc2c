"""Host restatement of the counter-based noise streams of mulan_randn (csrc/optim.hip) and mulan_noise (csrc/ode.hip),
built on the oracle's Philox4x32-10 (oracle.mulan_np.philox4x32_10, pinned to the Random123 vector by
tests/test_oracle_kat.py).

The stream law both kernels follow: element 4q + e of a draw of n elements at (seed, offset) is made from word e of
Philox(seed, counter = offset + q).  The uniforms are built here in np.float32 with the kernels' own operations (an
integer-to-float conversion, one addition, one multiplication by a power of two: all exactly rounded, so host and
device agree bit for bit); the transcendental part of each formula is evaluated in the dtype asked for -- float64 for
the reference, float32 to measure what fp32 evaluation of the same formula costs (the tests derive their bars from
that)."""
import numpy as np
import torch

from oracle import mulan_np as onp

TWO_PI_F32 = np.float32(6.283185307179586)
SQRT2_F32 = np.float32(1.41421356237309505)
RSQRT2_F32 = np.float32(0.70710678118654752)
HALF_STEP = np.float32(2.0 ** -25)              # added to the 24-bit uniform so that it is never 0
BELOW_ONE = np.float32(1.0 - 2.0 ** -24)        # the largest fp32 below 1


def words(seed, offset, n):
    """uint32 [n]: the word behind each of the n elements of a stream starting at counter `offset`"""
    nq = (int(n) + 3) // 4
    ctr = np.uint64(int(offset)) + np.arange(nq, dtype=np.uint64)
    return onp.philox4x32_10(seed, ctr).reshape(-1)[:int(n)]


def uniform24(w):
    """mulan_noise kind 0: (w >> 8) * 2^-24 in [0, 1), fp32 (exact: 24 bits)"""
    return (w >> np.uint32(8)).astype(np.float32) * np.float32(2.0 ** -24)


def rademacher(w):
    """mulan_noise kind 1: the top bit"""
    return np.where((w >> np.uint32(31)) != 0, np.float32(1.0), np.float32(-1.0)).astype(np.float32)


def open_uniform24(w, below_one=False):
    """the uniform of the truncated-normal and Gumbel kinds: fp32(u + 2^-25) in (0, 1].  For the largest u the sum is a
    tie that rounds to 1.0f; the Gumbel kind keeps it below 1 (below_one)"""
    u = uniform24(w) + HALF_STEP
    return np.minimum(u, BELOW_ONE) if below_one else u


def randn_uniform32(w):
    """mulan_randn: fp32((float)w + 0.5f) * 2^-32, then min(., 1)"""
    u = (w.astype(np.float32) + np.float32(0.5)) * np.float32(2.0 ** -32)
    return np.minimum(u, np.float32(1.0))


def randn_from_words(w, dtype):
    """Box-Muller as randn_kernel writes it: a quad (w0..w3) gives r0 cos a0, r0 sin a0, r1 cos a1, r1 sin a1 with
    r0 = sqrt(-2 log u0), a0 = 2 pi u1, r1 = sqrt(-2 log u2), a1 = 2 pi u3.  w: uint32 [n] (n need not be a multiple of
    4: the quad of the tail is completed by the caller passing the words of whole counters and slicing the result)."""
    assert w.size % 4 == 0
    u = randn_uniform32(w).reshape(-1, 4).astype(dtype)
    two_pi, two = dtype(TWO_PI_F32), dtype(2.0)
    r0, r1 = np.sqrt(-two * np.log(u[:, 0])), np.sqrt(-two * np.log(u[:, 2]))
    a0, a1 = two_pi * u[:, 1], two_pi * u[:, 3]
    z = np.stack([r0 * np.cos(a0), r0 * np.sin(a0), r1 * np.cos(a1), r1 * np.sin(a1)], axis=1)
    assert z.dtype == dtype
    return z.reshape(-1)


def randn(seed, offset, n, dtype=np.float64):
    nq = (int(n) + 3) // 4
    return randn_from_words(words(seed, offset, 4 * nq), dtype)[:int(n)]


def gumbel_from_words(w, dtype):
    """mulan_noise kind 3: -log(-log(u'))"""
    u = open_uniform24(w, below_one=True).astype(dtype)
    return -np.log(-np.log(u))


def truncated_normal_from_words(w, lo, hi, dtype):
    """mulan_noise kind 2: inverse CDF of the standard normal on [lo, hi]:
    p = Phi(lo) + (Phi(hi) - Phi(lo)) u',  x = clamp(sqrt(2) erfinv(2 p - 1), lo, hi),  Phi(x) = (1 + erf(x / sqrt 2)) / 2.
    The constants sqrt(2), 1 / sqrt(2) are the kernel's fp32 literals; erf / erfinv are torch's, in `dtype`."""
    td = torch.float64 if dtype == np.float64 else torch.float32
    u = torch.from_numpy(open_uniform24(w)).to(td)
    lo_t, hi_t = torch.tensor(np.float32(lo)).to(td), torch.tensor(np.float32(hi)).to(td)
    half, one, two = (torch.tensor(v, dtype=td) for v in (0.5, 1.0, 2.0))
    rs2, s2 = torch.tensor(RSQRT2_F32).to(td), torch.tensor(SQRT2_F32).to(td)
    plo, phi = half * (one + torch.erf(lo_t * rs2)), half * (one + torch.erf(hi_t * rs2))
    p = plo + (phi - plo) * u
    x = torch.minimum(torch.maximum(s2 * torch.special.erfinv(two * p - one), lo_t), hi_t)
    assert x.dtype == td
    return x.numpy()
