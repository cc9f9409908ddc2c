"""Oracles of mulan_bound_profile (tests/test_bound_profile.py on the CPU, tests/test_gpu_bound_profile.py on the GPU).

Float64.  The per-element terms of the variational bound, from oracle.torch_ref.encode / logprob and the formulas of
oracle.torch_ref.mulan_forward / plain_vdm_forward, with f = encode(x), sigma^2 = sigmoid(gamma):
  rho_i   = -logprob(x_i, z_0i, g_0i),  z_0 = f + exp(g_0 / 2) eps_0           the reconstruction term
  kappa_i = 1/2 ((1 - v1) f^2 + v1 - log v1 - 1),  v1 = sigmoid(g_1)            the prior KL
  d_i     = 1/2 w r^2,                  r = eps - eps_hat                         mode 2 (epsilon)
          = 1/2 (1 - sigma_t^2) w r^2,  r = v* - v_hat, v* = alpha eps - sigma f  mode 0 (v_hat the network output) and
            mode 1 (v_hat = -exp(g_t / 2) z_t + sqrt(1 + exp(g_t)) eps_hat)
  factor  = w (mode 2), (1 - sigma_t^2) w (modes 0, 1)
rows [B, 8] = sum d, sum d over channel 0, 1, 2 (sub-pixel i is channel i % 3), sum rho, sum kappa, sum r^2, mean
factor; cols [G, 3, 3072] = the mean over the R rows of group g of d, rho, kappa.

fp32.  kernel_fp32 restates the kernel's arithmetic in numpy fp32 and its order of summation: thread tid of 256 owns the
sub-pixels 1024 j + 4 tid + q and adds them in the order j, q; lanes by the xor butterfly, waves in wave order; a column
within a chunk of CHUNK = 8 rows in row order from 0, the chunks in chunk order, one division by R.  (The bin sums run
over all 256 bins: the kernel's window drops only terms that are exactly +0.)

Bounds.  ROWS_BOUND / COLS_BOUND are 4 x the largest error of kernel_fp32 against float64 over CASES x modes (the rule of
tests/schedule_curves_oracle.py; the factor is for what the restatement does not know: the device's expf / logf and
the compiler's fused multiply-adds).  The row sums (columns 0-6) are held relative to max(1, |value|), the mean factor
(column 7) and the column means absolutely."""
import functools

import numpy as np
import torch

from oracle import torch_ref as tr

D = 3072
CHUNK = 8                                   # rows per block of bound_profile.hip
GMIN, GMAX = -13.3, 5.0
ROW_NAMES = ("diff", "diff_ch0", "diff_ch1", "diff_ch2", "recon", "klz", "resid2", "factor_mean")
COL_NAMES = ("diff", "recon", "klz")

# Largest errors of kernel_fp32 against float64 over CASES x modes 0, 1, 2 (measure_errors(), rounded up to two digits;
# measured 2026-10-20 on the CPU), held to these values by tests/test_bound_profile.py.  The GPU is allowed 4 x.
# Who sets them: the per-row layout for the sums of d (one sigmoid and one weight per row: their rounding is the same at
# all 3072 sub-pixels and does not average out), the narrow window for the reconstruction sum and its column mean.
MEASURED_ROWS = (6.7e-6, 6.8e-6, 6.7e-6, 6.7e-6, 1.5e-5, 1.1e-5, 2.1e-7, 6.9e-6)
MEASURED_COLS = (2.8e-5, 6.7e-5, 7.9e-7)
ROWS_BOUND = tuple(4 * v for v in MEASURED_ROWS)
COLS_BOUND = tuple(4 * v for v in MEASURED_COLS)

FAMILIES = ("uniform", "narrow", "wide", "gt_lo", "gt_hi", "x0", "x255", "exact")
# (family, G, R, per-row gammas): every (G, R) of the issue in both layouts -- R = 1, 7 and 5 lie inside one chunk and
# are no multiple of it, R = 17 spans three chunks with a last one of a single row -- and every edge in one of them
CASES = tuple(("uniform", G, R, per_row) for per_row in (False, True) for G, R in ((1, 1), (1, 7), (3, 5), (2, 17))) + (
    ("narrow", 3, 5, False), ("narrow", 1, 7, True), ("wide", 1, 7, False), ("wide", 1, 1, True),
    ("gt_lo", 3, 5, False), ("gt_hi", 3, 5, False), ("x0", 1, 7, False), ("x255", 1, 7, False),
    ("exact", 2, 17, False), ("exact", 3, 5, True))


@functools.lru_cache(maxsize=None)
def inputs(family, G, R, per_row, seed=0):
    """a dict of read-only fp32 arrays (x uint8): x, g0, g1, gt, w ([B, 3072], or [B] with per_row), eps0, eps, zt and
    net0, net1, net2, the network output of each mode.
    uniform: gammas uniform in [gamma_min, gamma_max], w in [0, 40], the residual 0.3 N(0, 1); narrow / wide: g0 = -13.3
    (5-7 non-zero softmax terms) / +5 (all 256 bins); gt_lo / gt_hi: gt at the two ends of the schedule; x0 / x255: the
    edge bins; exact: eps_hat = eps bit for bit (net1 = net2 = eps; net0 = v* rounded to fp32)."""
    rng = np.random.default_rng([seed, FAMILIES.index(family), G, R, int(per_row)])
    B = G * R
    gs = (B,) if per_row else (B, D)
    x = rng.integers(0, 256, (B, D)).astype(np.uint8)
    g0, g1, gt = (rng.uniform(GMIN, GMAX, gs) for _ in range(3))
    w = rng.uniform(0.0, 40.0, gs)
    eps0, eps, noise = (rng.standard_normal((B, D)) for _ in range(3))
    noise *= 0.3
    if family == "narrow":
        g0[:] = GMIN
    elif family == "wide":
        g0[:] = GMAX
    elif family == "gt_lo":
        gt[:] = GMIN
    elif family == "gt_hi":
        gt[:] = GMAX
    elif family == "x0":
        x[:] = 0
    elif family == "x255":
        x[:] = 255
    elif family == "exact":
        noise[:] = 0.0
    out = dict(x=x, **{k: v.astype(np.float32) for k, v in dict(g0=g0, g1=g1, gt=gt, w=w, eps0=eps0, eps=eps).items()})
    # z_t and v* of the fp32 inputs, formed in float64 and rounded once
    f = 2.0 * ((x.astype(np.float64) + 0.5) / 256.0) - 1.0
    s = 1.0 / (1.0 + np.exp(-out["gt"].astype(np.float64).reshape(B, -1)))
    e = out["eps"].astype(np.float64)
    out["zt"] = (np.sqrt(1.0 - s) * f + np.sqrt(s) * e).astype(np.float32)
    out["net0"] = (np.sqrt(1.0 - s) * e - np.sqrt(s) * f + noise).astype(np.float32)
    out["net1"] = out["net2"] = (e + noise).astype(np.float32)
    for v in out.values():
        v.setflags(write=False)
    return out


# ------------------------------------------------------------------------------------------------------ float64
def terms64(mode, x, g0, g1, gt, w, eps0, eps, zt, net):
    """float64 torch [B, 3072] each: dict(d, rho, kappa, r, factor) of the formulas above; the gammas and w are
    [B, 3072] or [B]"""
    own = lambda v: v.detach().clone() if torch.is_tensor(v) else torch.as_tensor(np.array(v))
    t64 = lambda v: own(v).double()
    x = own(x)
    B = x.shape[0]
    g0, g1, gt, w = (t64(v).reshape(B, -1).expand(B, D) for v in (g0, g1, gt, w))
    eps0, eps, zt, net = (t64(v).reshape(B, D) for v in (eps0, eps, zt, net))
    f = tr.encode(x.reshape(B, D).double())
    z0 = f + torch.exp(0.5 * g0) * eps0
    col = lambda v: v.reshape(D, 1)
    rho = torch.stack([-tr.logprob(col(x[b].reshape(D)), col(z0[b]), col(g0[b])) for b in range(B)])
    v1 = torch.sigmoid(g1)
    kappa = 0.5 * ((1. - v1) * f * f + v1 - torch.log(v1) - 1.)
    if mode == 2:
        r, factor = eps - net, w
    else:
        var_t = torch.sigmoid(gt)
        v_hat = net if mode == 0 else -torch.exp(0.5 * gt) * zt + torch.sqrt(1 + torch.exp(gt)) * net
        r = torch.sqrt(1. - var_t) * eps - torch.sqrt(var_t) * f - v_hat
        factor = (1 - var_t) * w
    return dict(d=.5 * factor * r ** 2, rho=rho, kappa=kappa, r=r, factor=factor)


def rows_cols64(terms, G, R):
    """(rows float64 [B, 8], cols float64 [G, 3, 3072]) of terms64's output"""
    d, rho, kappa = (terms[k].numpy() for k in ("d", "rho", "kappa"))
    B = d.shape[0]
    ch = d.reshape(B, D // 3, 3).sum(1)
    rows = np.concatenate([d.sum(1, keepdims=True), ch, rho.sum(1, keepdims=True), kappa.sum(1, keepdims=True),
                           (terms["r"].numpy() ** 2).sum(1, keepdims=True), terms["factor"].numpy().mean(1, keepdims=True)], 1)
    cols = np.stack([v.reshape(G, R, D).mean(1) for v in (d, rho, kappa)], 1)
    return rows, cols


@functools.lru_cache(maxsize=None)
def case64(family, G, R, per_row, mode):
    """(rows, cols) in float64 of one case and mode: computed once, shared, read-only"""
    i = inputs(family, G, R, per_row)
    rows, cols = rows_cols64(terms64(mode, i["x"], i["g0"], i["g1"], i["gt"], i["w"], i["eps0"], i["eps"], i["zt"],
                                     i[f"net{mode}"]), G, R)
    rows.setflags(write=False)
    cols.setflags(write=False)
    return rows, cols


# ------------------------------------------------------------------------------------------------------ fp32 restatement
f32 = np.float32


def _sigmoid32(g):
    return f32(1) / (f32(1) + np.exp(-g))


def _block_sum(v):
    """v fp32 [..., 256] per thread -> [...]: lanes by the xor butterfly, then the four waves in wave order"""
    w = v.reshape(*v.shape[:-1], 4, 64)
    lane = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        w = w + w[..., lane ^ o]
    w = w[..., 0]
    return ((w[..., 0] + w[..., 1]) + w[..., 2]) + w[..., 3]


def _row_sum(v):
    """fp32 [B, 3072] -> [B] in the kernel's order"""
    lay = v.reshape(v.shape[0], 3, 256, 4)
    s = np.zeros((v.shape[0], 256), dtype=f32)
    for j in range(3):
        for q in range(4):
            s = s + lay[:, j, :, q]
    return _block_sum(s)


def terms32(mode, x, g0, g1, gt, w, eps0, eps, zt, net):
    """fp32 [B, 3072] each: (d, rho, kappa, r^2, factor) as bound_profile.hip forms them"""
    B = x.shape[0]
    g0, g1, gt, w = (np.broadcast_to(np.asarray(v, dtype=f32).reshape(B, -1), (B, D)) for v in (g0, g1, gt, w))
    bins = f32(2) * ((np.arange(256, dtype=f32) + f32(0.5)) / f32(256)) - f32(1)
    f = bins[x]
    z0 = f + np.exp(f32(0.5) * g0) * eps0
    istd = np.exp(f32(-0.5) * g0)
    logit = lambda v: f32(-0.5) * ((z0 - v) * istd) * ((z0 - v) * istd)
    mx = np.full((B, D), -np.inf, dtype=f32)
    for m in range(256):
        mx = np.maximum(mx, logit(bins[m]))
    se = np.zeros((B, D), dtype=f32)
    for m in range(256):
        se = se + np.exp(logit(bins[m]) - mx)
    rho = -((logit(f) - mx) - np.log(se))
    v1 = _sigmoid32(g1)
    kappa = f32(0.5) * ((f32(1) - v1) * f * f + v1 - np.log(v1) - f32(1))
    if mode == 2:
        r, factor = eps - net, w
    else:
        s = _sigmoid32(gt)
        al, sg = np.sqrt(f32(1) - s), np.sqrt(s)
        vhat = net if mode == 0 else -np.exp(f32(0.5) * gt) * zt + np.sqrt(f32(1) + np.exp(gt)) * net
        r = (al * eps - sg * f) - vhat
        factor = (f32(1) - s) * w
    out = (f32(0.5) * factor * r * r, rho, kappa, r * r, factor)
    assert all(v.dtype == f32 for v in out)
    return out


def kernel_fp32(mode, G, R, x, g0, g1, gt, w, eps0, eps, zt, net):
    """(rows fp32 [B, 8], cols fp32 [G, 3, 3072]) as bound_profile.hip forms them"""
    d, rho, kappa, r2, factor = terms32(mode, x, g0, g1, gt, w, eps0, eps, zt, net)
    B = G * R
    sub = np.arange(D)
    rows = np.stack([_row_sum(d)] + [_row_sum(np.where(sub % 3 == ch, d, f32(0))) for ch in range(3)] +
                    [_row_sum(rho), _row_sum(kappa), _row_sum(r2), _row_sum(factor) / f32(D)], 1)
    cols = np.zeros((G, 3, D), dtype=f32)
    for k, v in enumerate((d, rho, kappa)):
        v = v.reshape(G, R, D)
        total = None
        for c in range(0, R, CHUNK):
            part = np.zeros((G, D), dtype=f32)
            for r in range(c, min(R, c + CHUNK)):
                part = part + v[:, r]
            total = part if total is None else total + part
        cols[:, k] = total / f32(R)
    assert rows.dtype == f32 and rows.shape == (B, 8)
    return rows, cols


def errors(rows, cols, rows64, cols64):
    """([8], [3]): the largest error of rows against rows64 -- relative to max(1, |value|) for the sums, absolute for the
    mean factor -- and the largest absolute error of each of the three column means"""
    scale = np.maximum(1.0, np.abs(rows64))
    scale[:, 7] = 1.0
    return (np.abs(rows - rows64) / scale).max(0), np.abs(cols - cols64).max(axis=(0, 2))


def measure_errors():
    """{(case, mode): ([8], [3])} of kernel_fp32 against float64"""
    out = {}
    for case in CASES:
        i = inputs(*case)
        for mode in (0, 1, 2):
            got = kernel_fp32(mode, case[1], case[2], i["x"], i["g0"], i["g1"], i["gt"], i["w"], i["eps0"], i["eps"],
                              i["zt"], i[f"net{mode}"])
            out[case + (mode,)] = errors(*got, *case64(*case, mode))
    return out
