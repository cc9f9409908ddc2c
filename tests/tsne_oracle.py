"""numpy oracle of exact t-SNE as tsne.hip computes it (mulan_tsne_affinities / _gradient / _update), in float64 -- and an
fp32 restatement of the same arithmetic (every product and partial sum rounded to fp32, numpy's pairwise row sums, the
sums over the points in float64 as in the kernel) whose own error against float64 on the same input sets the GPU
tolerances at 4x, the convention of spectrum_oracle.py.  The 4x covers what the restatement does not reproduce: the
kernel's order of summation, its fused multiply-adds and its exp / log.  Nothing is taken from sklearn.

The search for beta is the kernel's: beta starts at 1, doubles or halves while a side of the bracket is open, then takes
64 midpoints, 100 steps in all at the most, no tolerance (in float64 the 64 midpoints end below 1e-12 of beta)."""
import functools

import numpy as np

MARGIN = 4.0
MAX_STEPS, BISECTIONS = 100, 64
AMBIGUOUS_CAP = 0.01          # the share of update elements whose gain branch may be left out of a comparison


# ------------------------------------------------------------------------------------------------ affinities
def sqdist(x, dtype=np.float64):
    """[N, N] in `dtype`: sum_d (x_id - x_jd)^2 from the differences, d ascending, every term rounded to `dtype`"""
    x = np.asarray(x).astype(dtype)
    out = np.zeros((x.shape[0], x.shape[0]), dtype=dtype)
    for d in range(x.shape[1]):
        diff = x[:, d, None] - x[None, :, d]
        out += diff * diff
    return out


def _search(dist, perplexity, dtype):
    """(conditional P [N, N], beta [N]) in `dtype` from squared distances: the kernel's search, all rows at once"""
    N = dist.shape[0]
    off = ~np.eye(N, dtype=bool)
    d = dist - np.where(off, dist, np.inf).min(axis=1, keepdims=True)
    d[~off] = 0
    d = d.astype(dtype)
    target = dtype(np.log(dtype(perplexity)))
    beta = np.ones(N, dtype=dtype)
    bmin, bmax = np.full(N, -np.inf, dtype=dtype), np.full(N, np.inf, dtype=dtype)
    nbis = np.zeros(N, dtype=np.int64)
    half, two = dtype(0.5), dtype(2)
    with np.errstate(over="ignore", under="ignore"):
        for _ in range(MAX_STEPS):
            act = np.nonzero(nbis < BISECTIONS)[0]
            if act.size == 0:
                break
            b = beta[act]
            p = np.exp(-d[act] * b[:, None]) * off[act]
            sp = p.sum(axis=1, dtype=dtype)
            H = np.log(sp) + b * (d[act] * p).sum(axis=1, dtype=dtype) / sp
            up = H - target > 0
            lo, hi = bmin[act], bmax[act]
            lo = np.where(up, b, lo)
            hi = np.where(up, hi, b)
            open_side = np.where(up, np.isinf(bmax[act]), np.isinf(bmin[act]))
            new = np.where(up, np.where(open_side, b * two, (b + bmax[act]) * half),
                           np.where(open_side, b * half, (b + bmin[act]) * half))
            beta[act], bmin[act], bmax[act] = new.astype(dtype), lo, hi
            nbis[act] += ~open_side
        p = np.exp(-d * beta[:, None]) * off
    P = (p / p.sum(axis=1, dtype=dtype, keepdims=True)).astype(dtype)
    return P, beta


def conditional_p(x, perplexity, dtype=np.float64):
    """(P_{j|i} [N, N], beta [N]) in `dtype` of the rows of x"""
    return _search(sqdist(x, dtype), perplexity, dtype)


def joint_p(cond):
    """(P_{j|i} + P_{i|j}) / (2 N) in cond's dtype"""
    return ((cond + cond.T) / cond.dtype.type(2 * cond.shape[0])).astype(cond.dtype)


def row_perplexity(cond):
    """[N] float64: exp of the entropy of every row of a conditional P"""
    c = np.asarray(cond, dtype=np.float64)
    c = c / c.sum(axis=1, keepdims=True)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.exp(-np.where(c > 0, c * np.log(c), 0.0).sum(axis=1))


@functools.lru_cache(maxsize=None)
def _affinity_bounds(key, perplexity):
    x = _KEPT[key]
    c64, b64 = conditional_p(x, perplexity)
    c32, b32 = conditional_p(x, perplexity, np.float32)
    j64, j32 = joint_p(c64), joint_p(c32)
    out = dict(cond=c64, joint=j64, beta=b64,
               tol_cond=MARGIN * float(np.abs(c32 - c64).max()), tol_P=MARGIN * float(np.abs(j32 - j64).max()),
               tol_beta=MARGIN * float((np.abs(b32 - b64) / b64).max()))
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


_KEPT = {}


def affinity_bounds(x, perplexity):
    """dict: cond, joint (float64 [N, N]), beta [N], and tol_cond, tol_P (absolute, 4 x the restatement's largest error on
    this x) and tol_beta (RELATIVE per row: the betas of one set span decades).  Computed once per input, read-only."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    key = (x.shape, x.tobytes())
    _KEPT.setdefault(key, x)
    return _affinity_bounds(key, float(perplexity))


# ------------------------------------------------------------------------------------------------ gradient, update
def gradient(P, Y, exaggeration, dtype=np.float64):
    """(grad [N, 2] in `dtype`, kl float): 4 (exaggeration sum_j P_ij w_ij (y_i - y_j) - sum_j w_ij^2 (y_i - y_j) / Z) and
    sum_{P > 0} P ln(P / (w / Z)) of P as it is.  Row sums in `dtype`, the sums over the rows in float64 (the kernel's
    fold)."""
    P, Y = np.asarray(P).astype(dtype), np.asarray(Y).astype(dtype)
    N = P.shape[0]
    off = ~np.eye(N, dtype=bool)
    with np.errstate(over="ignore", under="ignore", divide="ignore", invalid="ignore"):
        dx, dy = Y[:, None, 0] - Y[None, :, 0], Y[:, None, 1] - Y[None, :, 1]
        q = dtype(1) + (dx * dx + dy * dy)
        w = np.where(off, dtype(1) / q, dtype(0)).astype(dtype)
        pw, w2 = P * w, w * w
        a = np.stack([(pw * dx).sum(axis=1, dtype=dtype), (pw * dy).sum(axis=1, dtype=dtype)], axis=1)
        r = np.stack([(w2 * dx).sum(axis=1, dtype=dtype), (w2 * dy).sum(axis=1, dtype=dtype)], axis=1)
        Z = float(w.sum(axis=1, dtype=dtype).astype(np.float64).sum())
        k = np.where(P > 0, P * (np.log(np.where(P > 0, P, 1)) + np.log(q)), dtype(0)).astype(dtype).sum(axis=1, dtype=dtype)
        s = P.sum(axis=1, dtype=dtype)
    grad = (4.0 * (float(exaggeration) * a.astype(np.float64) - r.astype(np.float64) / Z)).astype(dtype)
    return grad, float(k.astype(np.float64).sum() + np.log(Z) * s.astype(np.float64).sum())


def kl(P, Y):
    """float64 KL(P || Q) of the map Y, Q_ij = w_ij / Z"""
    return gradient(P, Y, 1.0)[1]


def update(grad, Y, U, G, momentum, lr, dtype=np.float64):
    """sklearn's _gradient_descent body -> (Y, U, G) in `dtype`; nothing is modified in place"""
    grad, Y, U, G = (np.asarray(v).astype(dtype) for v in (grad, Y, U, G))
    inc = U * grad < 0
    G = np.maximum(np.where(inc, G + dtype(0.2), G * dtype(0.8)), dtype(0.01)).astype(dtype)
    U = (dtype(momentum) * U - dtype(lr) * (G * grad)).astype(dtype)
    return (Y + U).astype(dtype), U, G


def step(P, Y, U, G, exaggeration, momentum, lr, dtype=np.float64):
    """one iteration -> dict(Y, U, G, grad, kl): kl is that of the map BEFORE the update"""
    grad, k = gradient(P, Y, exaggeration, dtype)
    Yn, Un, Gn = update(grad, Y, U, G, momentum, lr, dtype)
    return dict(Y=Yn, U=Un, G=Gn, grad=grad, kl=k)


def run(P, Y0, n_iter, exaggeration_iter=250, early_exaggeration=12.0, lr=50.0, dtype=np.float64, keep=()):
    """free-running iterations from Y0 (U = 0, G = 1; momentum 0.5 under exaggeration, 0.8 after) -> dict(Y, kl (of the
    final map, float64 arithmetic on the final Y), kl0, states {it: (Y, U, G) BEFORE iteration it})"""
    P = np.asarray(P).astype(dtype)
    Y = np.asarray(Y0).astype(dtype)
    U, G = np.zeros_like(Y), np.ones_like(Y)
    states = {}
    for it in range(n_iter):
        if it in keep:
            states[it] = (Y.copy(), U.copy(), G.copy())
        early = it < exaggeration_iter
        s = step(P, Y, U, G, early_exaggeration if early else 1.0, 0.5 if early else 0.8, lr, dtype)
        Y, U, G = s["Y"], s["U"], s["G"]
    return dict(Y=Y, kl=kl(P.astype(np.float64), Y.astype(np.float64)), kl0=kl(P.astype(np.float64), np.asarray(Y0, np.float64)),
                states=states)


def gradient_bounds(P, Y, exaggeration):
    """dict(grad, kl, tol_grad, tol_kl) for fp32 P and Y: float64 on these very values, 4 x the restatement's error"""
    P, Y = np.asarray(P, dtype=np.float32), np.asarray(Y, dtype=np.float32)
    g64, k64 = gradient(P, Y, exaggeration)
    g32, k32 = gradient(P, Y, exaggeration, np.float32)
    return dict(grad=g64, kl=k64, grad32=g32, tol_grad=MARGIN * float(np.abs(g32 - g64).max()), tol_kl=MARGIN * abs(k32 - k64))


def update_bounds(P, Y, U, G, exaggeration, momentum, lr):
    """dict(Y, U, G (float64 after one step), tol_Y, tol_U, tol_G, keep): `keep` [N, 2] leaves out only the elements whose
    float64 |U grad| lies below the restatement's own error on that product -- there the gain's branch is a coin toss --
    and their share is asserted to stay within AMBIGUOUS_CAP; the tolerances are over the kept elements"""
    P, Y, U, G = (np.asarray(v, dtype=np.float32) for v in (P, Y, U, G))
    s64 = step(P, Y, U, G, exaggeration, momentum, lr)
    s32 = step(P, Y, U, G, exaggeration, momentum, lr, np.float32)
    ug64 = U.astype(np.float64) * s64["grad"]
    ug32 = (U * s32["grad"]).astype(np.float64)
    keep = ~(np.abs(ug64) < np.abs(ug32 - ug64))
    assert (~keep).mean() <= AMBIGUOUS_CAP, (~keep).mean()
    out = dict(Y=s64["Y"], U=s64["U"], G=s64["G"], keep=keep, grad=s64["grad"])
    for name in ("Y", "U", "G"):
        out["tol_" + name] = MARGIN * float(np.abs(s32[name] - s64[name])[keep].max())
    return out


def free_run_bounds(P, Y0, n_iter, **kw):
    """dict(Y, tol_Y): n_iter free iterations in float64 from fp32 P and Y0, 4 x the restatement's distance after them"""
    P, Y0 = np.asarray(P, dtype=np.float32), np.asarray(Y0, dtype=np.float32)
    y64 = run(P, Y0, n_iter, **kw)["Y"]
    y32 = run(P, Y0, n_iter, dtype=np.float32, **kw)["Y"]
    return dict(Y=y64, tol_Y=MARGIN * float(np.abs(y32 - y64).max()))


# ------------------------------------------------------------------------------------------------ the planted set
def planted(clusters=6, per=16, D=50, k=15, noise=0.15, seed=3):
    """(x fp32 [clusters per, D], labels): k-hot centres plus noise * normal"""
    rng = np.random.default_rng(seed)
    centres = np.zeros((clusters, D))
    for c in range(clusters):
        centres[c, rng.choice(D, k, replace=False)] = 1.0
    labels = np.repeat(np.arange(clusters), per)
    x = (centres[labels] + noise * rng.standard_normal((clusters * per, D))).astype(np.float32)
    return x, labels


def pca_init(x):
    """float32 [N, 2]: the first two principal components (each component's largest loading positive) / std of the first
    * 1e-4"""
    x = np.asarray(x, dtype=np.float64)
    u, s, vt = np.linalg.svd(x - x.mean(axis=0), full_matrices=False)
    sign = np.sign(vt[np.arange(vt.shape[0]), np.abs(vt).argmax(axis=1)])
    y = (u * sign * s)[:, :2]
    return (y / y[:, 0].std() * 1e-4).astype(np.float32)


def purity(Y, labels):
    """the share of points whose nearest map neighbour carries their label"""
    Y = np.asarray(Y, dtype=np.float64)
    d = ((Y[:, None] - Y[None]) ** 2).sum(-1)
    np.fill_diagonal(d, np.inf)
    return float((labels[d.argmin(axis=1)] == labels).mean())
