"""Oracles of mulan_schedule_curves (tests/test_schedule_curves.py on the CPU, tests/test_gpu_schedule_curves.py on the
GPU): the schedule on a time grid and its summaries in float64 through oracle.torch_ref.poly_gamma, and a numpy-fp32
restatement of the kernel's own arithmetic -- its ratios (formed in double, rounded once), its Horner form in the centred
time (an fmaf is a float64 product and sum rounded to fp32 once), its order of summation -- from which the error bounds
of the GPU tests are taken: the largest absolute error of the restatement against float64 over the input families below,
times 4 for what the restatement does not know (the compiler's contractions in the deviation, the device's expf and
division)."""
import numpy as np
import torch

from oracle import torch_ref as tr

D = 3072
GMIN, GMAX = -13.3, 5.0
STAT_NAMES = ("mean", "std", "min", "max", "channel_mean_0", "channel_mean_1", "channel_mean_2", "sigma2_mean")

# Largest absolute errors of kernel_fp32 against float64 over FAMILIES (seed 0, E = 3) at bound_times(): gamma, then the
# eight statistics in the order of STAT_NAMES; measured by measure_errors(), held to these values (rounded up to two
# digits) by tests/test_schedule_curves.py.  The GPU is allowed 4 x.
MEASURED_GAMMA = 7.3e-6                                    # (the cancel_100 family; 6.8e-6 normal, 1.2e-6 linear)
MEASURED_STATS = (3.8e-6, 2.9e-6, 6.2e-6, 4.4e-6, 2.7e-6, 2.7e-6, 2.7e-6, 3.0e-7)      # (the channels share their largest)
GAMMA_BOUND = 4 * MEASURED_GAMMA
STATS_BOUND = tuple(4 * v for v in MEASURED_STATS)

FAMILIES = ("normal", "cancel_1", "cancel_100", "linear", "large_a")


def family(name, E, seed=0):
    """fp32 (a, b, c) [E, 3072] of one input family"""
    rng = np.random.default_rng([seed, FAMILIES.index(name)])
    n = lambda: rng.standard_normal((E, D))
    if name == "normal":
        a, b, c = n(), n(), np.logaddexp(n(), 0.0) + 1e-3
    elif name in ("cancel_1", "cancel_100"):        # the direction in which the monomial S cancels
        s = 1.0 if name == "cancel_1" else 100.0
        a, b, c = (s * v * (1 + 1e-3 * n()) for v in (6.0, -6.0, 1.0))
    elif name == "linear":                          # gamma = gmin + R t for every sub-pixel
        a, b, c = np.zeros((E, D)), np.zeros((E, D)), np.full((E, D), 1e-3)
    elif name == "large_a":
        a, b, c = 1e3 * np.sign(n()) * (1 + 0.1 * n()), n(), np.logaddexp(n(), 0.0) + 1e-3
    else:
        raise KeyError(name)
    return tuple(np.ascontiguousarray(v, dtype=np.float32) for v in (a, b, c))


def channel_family(E, seed=0):
    """the normal family with three visibly different channels: a, b, c of channel k (sub-pixel i % 3 == k) are scaled so
    that the channel means of gamma lie far apart at mid times"""
    a, b, c = family("normal", E, seed)
    a, b, c = a.reshape(E, D // 3, 3).copy(), b.reshape(E, D // 3, 3).copy(), c.reshape(E, D // 3, 3).copy()
    a[..., 0], b[..., 0] = 8.0 + 0.1 * a[..., 0], 0.1 * b[..., 0]          # late riser
    a[..., 1], b[..., 1] = 0.1 * a[..., 1], 0.1 * b[..., 1]                # nearly linear
    a[..., 2], b[..., 2], c[..., 2] = 8.0 + 0.1 * a[..., 2], -8.0 + 0.1 * b[..., 2], 3.0 + c[..., 2]   # early riser
    return a.reshape(E, D), b.reshape(E, D), c.reshape(E, D)


def bound_times():
    """the times at which the bounds are measured: the default grid of noise_schedule_per_embedding and 32 random ones"""
    rng = np.random.default_rng(7)
    return np.concatenate([np.linspace(0.0, 1.0, 128), rng.random(32)]).astype(np.float32)


def grid_times(T):
    """fp32 [T] for the GPU tests: unsorted, with repeats, with 0.0 and 1.0 from T = 2 on"""
    if T == 1:
        return np.array([0.37], dtype=np.float32)
    if T == 2:
        return np.array([1.0, 0.0], dtype=np.float32)
    rng = np.random.default_rng(T)
    t = rng.random(T).astype(np.float32)
    t[:5] = [0.5, 0.0, 1.0, 0.25, 0.25]
    if T >= 128:
        t[5:5 + 123] = np.linspace(0.0, 1.0, 128, dtype=np.float32)[1:124]
        t = rng.permutation(t)
    return t


# ------------------------------------------------------------------------------------------------------ float64
def gamma64(a, b, c, t, gmin=GMIN, gmax=GMAX):
    """float64 [E, T, 3072] through oracle.torch_ref.poly_gamma"""
    a, b, c = (torch.as_tensor(np.asarray(v), dtype=torch.float64) for v in (a, b, c))
    t = torch.as_tensor(np.asarray(t), dtype=torch.float64)
    T = t.numel()
    return np.stack([tr.poly_gamma(a[e:e + 1].expand(T, D), b[e:e + 1].expand(T, D), c[e:e + 1].expand(T, D), t, gmin,
                                   gmax).numpy() for e in range(a.shape[0])])


def model_gamma64(ref_params, emb, t, gmin=GMIN, gmax=GMAX):
    """float64 [E, T, 3072] of a model's float64 parameters: poly_gamma(poly_coefficients(...)), row by row"""
    with torch.no_grad():
        a, b, c = tr.poly_coefficients(torch.as_tensor(np.asarray(emb), dtype=torch.float64), ref_params["gamma"])
    return gamma64(a, b, c, t, gmin, gmax)


def stats_of(g):
    """[E, T, 8] in the order of STAT_NAMES, in the dtype of g's float64 view"""
    g = np.asarray(g, dtype=np.float64)
    ch = g.reshape(*g.shape[:-1], D // 3, 3).mean(axis=-2)
    return np.concatenate([np.stack([g.mean(-1), g.std(-1), g.min(-1), g.max(-1)], -1), ch,
                           (1.0 / (1.0 + np.exp(-g))).mean(-1, keepdims=True)], -1)


def hist64(g, bins, gmin=GMIN, gmax=GMAX):
    """int64 [E, T, bins]: the counts of clip(floor((gamma - gmin) bins / R), 0, bins - 1) in float64 (the clip is the
    kernel's: a value a rounding below gmin still counts in bin 0, one at or above gmax in the last)"""
    k = np.clip(np.floor((np.asarray(g, np.float64) - gmin) * (bins / (gmax - gmin))), 0, bins - 1).astype(np.int64)
    return _count(k, bins)


def near_edge(g, bins, bound, gmin=GMIN, gmax=GMAX):
    """int [E, T]: sub-pixels whose float64 gamma lies within `bound` of an interior bin edge gmin + k R / bins,
    0 < k < bins (the two ends are no edges: see hist64)"""
    w = (gmax - gmin) / bins
    pos = (np.asarray(g, np.float64) - gmin) / w
    k = np.rint(pos)
    return (((k >= 1) & (k <= bins - 1)) & (np.abs(pos - k) * w <= bound)).sum(-1)


def _count(k, bins):
    out = np.zeros(k.shape[:-1] + (bins,), dtype=np.int64)
    for idx in np.ndindex(*k.shape[:-1]):
        out[idx] = np.bincount(k[idx], minlength=bins)
    return out


def linear_closed_form(t, gmin=GMIN, gmax=GMAX):
    """float64 [T, 8]: the statistics of the linear family, gamma = gmin + R t at every sub-pixel"""
    g = gmin + (gmax - gmin) * np.asarray(t, dtype=np.float64)
    return np.stack([g, np.zeros_like(g), g, g, g, g, g, 1.0 / (1.0 + np.exp(-g))], -1)


# ------------------------------------------------------------------------------------------------------ fp32 restatement
f32 = np.float32


def _fma(x, y, z):
    """fmaf on fp32 arrays: the product of two fp32 is exact in float64; the sum is rounded to float64, then to fp32"""
    return (x.astype(np.float64) * y.astype(np.float64) + np.float64(1) * z).astype(f32)


def _block_sum(v):
    """v fp32 [..., 256] per thread -> [...]: lanes by the xor butterfly, then the four waves in wave order"""
    w = v.reshape(*v.shape[:-1], 4, 64)
    lane = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        w = w + w[..., lane ^ o]
    w = w[..., 0]
    return ((w[..., 0] + w[..., 1]) + w[..., 2]) + w[..., 3]


def binning32(g32, bins, gmin=GMIN, gmax=GMAX):
    """int64 [E, T, bins]: the kernel's binning of fp32 gammas, restated in numpy fp32"""
    gmin32 = f32(gmin)
    scale = f32(bins) / (f32(gmax) - gmin32)
    k = ((np.asarray(g32, dtype=f32) - gmin32) * scale).astype(np.int32)          # (int): truncation
    return _count(np.clip(k, 0, bins - 1).astype(np.int64), bins)


def kernel_fp32(a, b, c, t, gmin=GMIN, gmax=GMAX):
    """(gamma fp32 [E, T, 3072], stats fp32 [E, T, 8]) as schedule_curves.hip forms them"""
    a, b, c, t = (np.asarray(v, dtype=f32) for v in (a, b, c, t))
    gmin32 = f32(gmin)
    R = f32(gmax) - gmin32
    # the five ratios of the centred form, in double as the kernel forms them, rounded to fp32 once
    ad, bd, cd = (v.astype(np.float64) for v in (a, b, c))
    u0, u1, u2 = cd + 0.5 * bd + ad * (1.0 / 3.0), 0.5 * (ad + bd), ad * (1.0 / 6.0)
    inv_s = 1.0 / (u0 * u0 + u1 * u1 * (1.0 / 3.0) + u2 * u2 * 0.2)
    al, be = 0.25 * ad, 0.5 * (ad + bd)
    ga = al + 0.5 * bd + cd
    d4 = al * al * 0.2
    d3 = al * be * 0.5 - d4
    d2 = (be * be + 2.0 * al * ga) * (1.0 / 3.0) - d3
    d1 = be * ga - d2
    d0 = ga * ga - d1
    r = [(v * inv_s).astype(f32)[:, None, :] for v in (d0, d1, d2, d3, d4)]
    tv = np.broadcast_to(t[None, :, None], (a.shape[0], t.size, D))
    z = _fma(np.full_like(tv, 2), tv, f32(-1))
    p = tv * _fma(z, _fma(z, _fma(z, _fma(z, r[4], r[3]), r[2]), r[1]), r[0])
    x = R * p
    g = _fma(np.broadcast_to(R, p.shape), p, gmin32)
    # thread tid owns 1024 j + 4 tid + q
    lay = lambda v: v.reshape(*v.shape[:-1], 3, 256, 4)
    xl = lay(x)
    sig_l = lay(f32(1) / (f32(1) + np.exp(-g)))
    zero = np.zeros(x.shape[:-1] + (256,), dtype=f32)
    s, sig, cs = zero.copy(), zero.copy(), [zero.copy() for _ in range(3)]
    for j in range(3):
        for q in range(4):
            s = s + xl[..., j, :, q]
            sig = sig + sig_l[..., j, :, q]
            cs[(j + q) % 3] = cs[(j + q) % 3] + xl[..., j, :, q]
    rot = np.arange(256) % 3                         # slot k of thread tid is channel (k + tid) % 3
    cs = np.stack(cs, -1)
    ch = [np.take_along_axis(cs, np.broadcast_to(((k - rot) % 3)[..., None], cs.shape[:-1] + (1,)), -1)[..., 0]
          for k in range(3)]
    mean_x = _block_sum(s) / f32(D)
    dev = zero.copy()
    for j in range(3):
        for q in range(4):
            d = xl[..., j, :, q] - mean_x[..., None]
            dev = dev + d * d
    var = _block_sum(dev) / f32(D)
    stats = np.stack([gmin32 + mean_x, np.sqrt(var), g.min(-1), g.max(-1)] +
                     [gmin32 + _block_sum(ch[k]) / f32(D // 3) for k in range(3)] + [_block_sum(sig) / f32(D)], -1)
    assert g.dtype == f32 and stats.dtype == f32
    return g, stats


def measure_errors(E=3, seed=0):
    """{family: (largest |gamma error|, [8] largest |statistic error|)} of kernel_fp32 against float64 at bound_times()"""
    t = bound_times()
    out = {}
    for name in FAMILIES:
        a, b, c = family(name, E, seed)
        g64 = gamma64(a, b, c, t)
        g32, s32 = kernel_fp32(a, b, c, t)
        out[name] = (float(np.abs(g32 - g64).max()), np.abs(s32 - stats_of(g64)).reshape(-1, 8).max(0))
    return out
