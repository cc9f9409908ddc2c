"""Float64 restatement of the time grids of the few-step samplers (mulan_amd.sampling.make_grid): the five moments of a
batch's mean polynomial schedule, the schedule itself, its inverse, the four grid kinds, and the analytic Gaussian
model of tests/test_gpu_fast_sampler.py::test_convergence_on_an_analytic_model on which a grid's discretisation error
can be measured without a network.  numpy only; nothing here imports the package under test.

`python -m tests.grid_oracle` prints the error table of DESIGN.md §3.7 (seed 11, B = 2)."""
import numpy as np

GAMMA_MIN, GAMMA_MAX = -13.3, 5.0


def scale(a, b, c):
    """S of the polynomial schedule, as oracle/mulan_np.py poly_gamma forms it"""
    return a * a / 5.0 + (b * b + 2.0 * a * c) / 3.0 + a * b / 2.0 + b * c + c * c


def ratios(a, b, c):
    """float64 [..., 5]: per element the coefficients of t .. t^5 in P(t) / S"""
    a, b, c = (np.asarray(v, dtype=np.float64) for v in (a, b, c))
    S = scale(a, b, c)
    return np.stack([c * c / S, b * c / S, (b * b + 2.0 * a * c) / (3.0 * S), a * b / (2.0 * S), a * a / (5.0 * S)], axis=-1)


def moments(a, b, c):
    """float64 [B, 5]: per sample the mean over its sub-pixels of ratios (a, b, c: [B, d])"""
    return ratios(a, b, c).mean(axis=1)


def gamma_bar(m, t, gmin=GAMMA_MIN, gmax=GAMMA_MAX):
    """the mean schedule of a batch at the times t, from its moments m [B, 5] (or their mean [5])"""
    m = np.asarray(m, dtype=np.float64).reshape(-1, 5).mean(axis=0)
    t = np.asarray(t, dtype=np.float64)
    return gmin + (gmax - gmin) * t * (m[0] + t * (m[1] + t * (m[2] + t * (m[3] + t * m[4]))))


def invert(m, targets, gmin=GAMMA_MIN, gmax=GAMMA_MAX, halvings=80):
    """float64 times in [0, 1] with gamma_bar(t) = targets, by bisection (gamma_bar is increasing); a target at or
    beyond gmax gives exactly 1, one at or below gmin exactly 0"""
    targets = np.asarray(targets, dtype=np.float64).reshape(-1)
    lo, hi = np.zeros_like(targets), np.ones_like(targets)
    for _ in range(halvings):
        mid = 0.5 * (lo + hi)
        below = gamma_bar(m, mid, gmin, gmax) < targets
        lo, hi = np.where(below, mid, lo), np.where(below, hi, mid)
    t = 0.5 * (lo + hi)
    return np.where(targets >= gmax, 1.0, np.where(targets <= gmin, 0.0, t))


def targets(kind, N, g0=GAMMA_MIN, g1=GAMMA_MAX, rho=7.0):
    """float64 [N + 1]: gamma_bar at the grid points i = 0 .. N of a 'logsnr' or 'karras' grid (g1 at i = 0, g0 at N)"""
    w = np.arange(N + 1, dtype=np.float64) / N
    if kind == "logsnr":
        return g1 + (g0 - g1) * w
    if kind == "karras":
        smax, smin = np.exp(g1 / 2.0), np.exp(g0 / 2.0)
        return 2.0 * np.log((smax ** (1.0 / rho) + w * (smin ** (1.0 / rho) - smax ** (1.0 / rho))) ** rho)
    raise ValueError(kind)


def grid(kind, N, m=None, gmin=GAMMA_MIN, gmax=GAMMA_MAX, rho=7.0):
    """float64 [N + 1] from 1 to 0"""
    if kind == "uniform":
        return 1.0 - np.arange(N + 1, dtype=np.float64) / N
    if kind == "quadratic":
        return (1.0 - np.arange(N + 1, dtype=np.float64) / N) ** 2
    inner = invert(m, targets(kind, N, gmin, gmax, rho)[1:-1], gmin, gmax)
    return np.concatenate([[1.0], inner, [0.0]])


# --------------------------------------------------------------------------------------------- the analytic model
class GaussianModel:
    """x ~ N(mu_i, sd_i^2) per coordinate under the per-element polynomial schedule of (a, b, c): the posterior mean is
    the exact denoiser and the probability-flow map z_1 -> z_0 is the per-coordinate quantile map"""

    def __init__(self, a, b, c, mu, sd, z1, gmin=GAMMA_MIN, gmax=GAMMA_MAX):
        self.a, self.b, self.c, self.mu, self.sd, self.z1 = (np.asarray(v, dtype=np.float64) for v in (a, b, c, mu, sd, z1))
        self.gmin, self.gmax = gmin, gmax
        self.S = scale(self.a, self.b, self.c)

    def gamma(self, t):
        a, b, c = self.a, self.b, self.c
        P = a * a * t ** 5 / 5 + (b * b + 2 * a * c) * t ** 3 / 3 + a * b * t ** 4 / 2 + b * c * t * t + c * c * t
        return self.gmin + (self.gmax - self.gmin) * P / self.S

    @staticmethod
    def alpha(g):
        return np.sqrt(1.0 / (1.0 + np.exp(g)))

    @staticmethod
    def sigma(g):
        return np.sqrt(1.0 / (1.0 + np.exp(-g)))

    def x_hat(self, z, g):
        A, S = self.alpha(g), self.sigma(g)
        return self.mu + A * self.sd ** 2 * (z - A * self.mu) / (A * A * self.sd ** 2 + S * S)

    def exact(self):
        g0, g1 = self.gamma(0.0), self.gamma(1.0)
        v = lambda g: self.alpha(g) ** 2 * self.sd ** 2 + self.sigma(g) ** 2
        return self.alpha(g0) * self.mu + (self.z1 - self.alpha(g1) * self.mu) * np.sqrt(v(g0)) / np.sqrt(v(g1))

    def run(self, times, sampler):
        """z_0 by 'ddim' or 'dpm2m' along `times` (taken as the fp32 values the device sees)"""
        times = np.asarray(times, dtype=np.float32).astype(np.float64)
        N = len(times) - 1
        z, gp, xp = self.z1.copy(), None, None
        for k in range(N):
            gt, gs = self.gamma(times[k]), self.gamma(times[k + 1])
            x, h = self.x_hat(z, gt), (gt - gs) / 2
            D = x
            if sampler == "dpm2m" and k > 0 and not (N < 15 and k == N - 1):
                w = h / (gp - gt)
                D = (1 + w) * x - w * xp
            z = self.sigma(gs) / self.sigma(gt) * z - self.alpha(gs) * np.expm1(-h) * D
            gp, xp = gt, x
        return z

    def error(self, times, sampler):
        """RMS error of z_0"""
        return float(np.sqrt(np.mean((self.run(times, sampler) - self.exact()) ** 2)))


def random_model(seed=11, B=2, d=3072):
    rng = np.random.default_rng(seed)
    a, b = rng.standard_normal((B, d)), rng.standard_normal((B, d))
    c = 1e-3 + np.log1p(np.exp(rng.standard_normal((B, d))))
    mu, sd = rng.random((B, d)) - 0.5, 0.05 + 0.45 * rng.random((B, d))
    return GaussianModel(a, b, c, mu, sd, rng.standard_normal((B, d)))


def error_table(seed=11, Ns=(8, 16, 32, 64)):
    model = random_model(seed)
    m = moments(model.a, model.b, model.c)
    return {(kind, sampler): [model.error(grid(kind, N, m), sampler) for N in Ns]
            for kind in ("uniform", "logsnr", "karras", "quadratic") for sampler in ("dpm2m", "ddim")}


if __name__ == "__main__":
    for (kind, sampler), e in error_table().items():
        print(f"{kind:10s} {sampler:6s}", " / ".join(f"{x:.2e}" for x in e),
              "  ratios", " ".join(f"{e[i] / e[i + 1]:.2f}" for i in range(len(e) - 1)))
