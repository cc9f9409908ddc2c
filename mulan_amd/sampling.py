"""Few-step samplers: DDIM and DPM-Solver++(2M) on the probability-flow ODE, and their stochastic forms, DDIM with
eta > 0 and SDE-DPM-Solver++(2M) ("sde2m": eta = 1 with the order schedule of dpm2m).

Not in the reference, whose samplers are the 1000-step ancestral loop and the RK45 ODE (both kept as they are).  MuLAN's
forward process is diagonal: every sub-pixel i has its own schedule gamma_i(t), strictly increasing in t, so
lambda_i = -gamma_i / 2 is a change of variable per coordinate and the DPM-Solver++ derivation holds element by element
with per-element step sizes.  The step itself is the HIP kernel
mulan_fast_sampler_step (ops.fast_sampler_step); this module holds the time grid, the order schedule, the history
(previous gamma and x_hat) and the loop.  `sample` takes a net_fn(z, t) and a gamma_fn(t), so an analytic denoiser can
stand in for the U-Net; the models drive the same loop through a stepper of their own (model._VDMBase.fast_stepper,
replayed as a HIP graph).  A stochastic step (eta > 0) is the HIP kernel mulan_stochastic_sampler_step
(ops.stochastic_sampler_step) on one standard normal per element, which the loop hands over step by step
(noise_fn(k)); eta = 0 keeps the deterministic kernel and its bits.  Second order at 0 < eta < 1 is an interpolation
of dpm2m and sde2m and no named method; no sampler here asks for it.
"""
import numpy as np
import torch

from . import ops

SAMPLERS = ("ancestral", "ddim", "dpm2m", "sde2m")
FAST_SAMPLERS = ("ddim", "dpm2m", "sde2m")
LOWER_ORDER_FINAL_BELOW = 15        # dpm2m: the last step is first order when N < 15 ("lower order final")


def check_sampler(sampler):
    if sampler not in SAMPLERS:
        raise ValueError(f"unknown sampler {sampler!r} (one of {', '.join(SAMPLERS)})")
    return sampler


def check_eta(sampler, eta=0.0):
    """the public keyword `eta` of a sampler -> step_eta, the eta its steps run with (what the steppers and the step
    kernel take): the keyword for ddim (0 <= eta <= 1), 1 for sde2m, 0 otherwise; a non-zero keyword with a sampler other
    than ddim is refused"""
    check_sampler(sampler)
    eta = float(eta)
    if not 0.0 <= eta <= 1.0:                   # (NaN fails both comparisons)
        raise ValueError(f"eta must lie in [0, 1], got {eta!r}")
    if eta != 0.0 and sampler != "ddim":
        raise ValueError(f"eta applies to the ddim sampler; {sampler!r} takes none")
    return 1.0 if sampler == "sde2m" else eta


def time_grid(steps=None, t_grid=None):
    """-> float64 array [N + 1] from 1 to 0: uniform in t over `steps` steps, or the explicit `t_grid` after checking that
    it is strictly decreasing, starts at 1 and ends at 0 (steps, if also given, must be len(t_grid) - 1)"""
    if t_grid is None:
        if steps is None or int(steps) != steps or steps < 1:
            raise ValueError(f"the number of sampling steps must be an integer >= 1, got {steps!r}")
        steps = int(steps)
        return 1.0 - np.arange(steps + 1, dtype=np.float64) / steps
    g = np.asarray(t_grid, dtype=np.float64).reshape(-1)
    if g.size < 2:
        raise ValueError("t_grid needs at least two points (one step)")
    if not np.all(np.isfinite(g)):
        raise ValueError("t_grid holds a value that is not finite")
    if g[0] != 1.0 or g[-1] != 0.0:
        raise ValueError(f"t_grid must run from 1 to 0, got {g[0]} .. {g[-1]}")
    if not np.all(np.diff(g) < 0):
        raise ValueError("t_grid must be strictly decreasing")
    if np.any(np.diff(g.astype(np.float32)) >= 0):
        raise ValueError("t_grid has two times that are equal in float32")
    if steps is not None and steps != g.size - 1:
        raise ValueError(f"steps = {steps} but t_grid has {g.size - 1} steps")
    return g


def step_orders(sampler, steps):
    """order of each of the `steps` steps: ddim all first order; dpm2m and sde2m second order except the first step
    and, for steps < 15, the last"""
    if sampler not in FAST_SAMPLERS:
        raise ValueError(f"step_orders: {sampler!r} is not a few-step sampler ({', '.join(FAST_SAMPLERS)})")
    if steps < 1:
        raise ValueError(f"steps must be >= 1, got {steps}")
    if sampler == "ddim":
        return [1] * steps
    orders = [1] + [2] * (steps - 1)
    if steps < LOWER_ORDER_FINAL_BELOW:
        orders[-1] = 1
    return orders


def f32(t):
    """a grid time as the fp32 value the device sees"""
    return float(np.float32(t))


class EagerStepper:
    """One solver step at a time through ops.fast_sampler_step, the history in tensors of its own.
    net_fn(z, t) -> network output shaped like z; gamma_fn(t) -> gamma at the (fp32) time t, per element (shaped like
    z) or per sample ([B]).  With step_eta > 0 (check_eta) the step is ops.stochastic_sampler_step on xi = noise_fn(k),
    one standard normal per element for step k (the fifth argument of the call)."""

    def __init__(self, net_fn, gamma_fn, mode, step_eta=0.0, noise_fn=None):
        self.net_fn, self.gamma_fn, self.mode = net_fn, gamma_fn, int(mode)
        self.step_eta, self.noise_fn = float(step_eta), noise_fn
        if self.step_eta > 0.0 and noise_fn is None:
            raise ValueError("a stochastic step (step_eta > 0) needs noise_fn(k) -> xi")
        self.g_prev = self.x_prev = None
        self._g = None              # (t, gamma(t)) of the last step's s: the next step's t

    def _gamma(self, t):
        if self._g is not None and self._g[0] == t:
            return self._g[1]
        return self.gamma_fn(t)

    def __call__(self, z, t, s, order, k=None):
        t, s = f32(t), f32(s)
        g_t = self._gamma(t)
        g_s = self.gamma_fn(s)
        net = self.net_fn(z, t)
        hist = (self.g_prev, self.x_prev) if order == 2 else (None, None)
        if order == 2 and self.g_prev is None:
            raise RuntimeError("a second-order step needs the history of a previous step")
        if self.step_eta > 0.0:
            if k is None:
                raise ValueError("a stochastic step needs its index k (the noise is drawn per step)")
            z_s, x0 = ops.stochastic_sampler_step(z, net, g_t, g_s, self.mode, self.noise_fn(k), self.step_eta,
                                                      *hist)
        else:
            z_s, x0 = ops.fast_sampler_step(z, net, g_t, g_s, self.mode, *hist)
        self.g_prev, self.x_prev, self._g = g_t, x0, (s, g_s)
        return z_s


def run(stepper, z, grid, orders):
    """the solver loop: stepper(z, t, s, order, k) -> z_s along the grid; the step's index k selects the noise of a
    stochastic step"""
    assert len(orders) == len(grid) - 1
    for k, order in enumerate(orders):
        z = stepper(z, grid[k], grid[k + 1], order, k)
    return z


def sample(net_fn, gamma_fn, z, mode, sampler="dpm2m", steps=None, t_grid=None, eta=0.0, noise_fn=None):
    """z_0 from z_1 = z by `sampler` (ddim | dpm2m | sde2m) over `steps` uniform steps or the explicit `t_grid`; mode as
    ops.fast_sampler_step (0: net_fn gives the velocity, 1: eps_hat, 2: x_hat).  eta (ddim only): 0 is the
    deterministic sampler; sde2m and ddim with eta > 0 need noise_fn(k) -> xi shaped like z, the noise of step k"""
    step_eta = check_eta(sampler, eta)
    grid = time_grid(steps, t_grid)
    orders = step_orders(sampler, len(grid) - 1)
    with torch.no_grad():
        return run(EagerStepper(net_fn, gamma_fn, mode, step_eta, noise_fn), z, grid, orders)
