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

Inpainting (the replacement method, with RePaint-style resampling): given a known image x and a mask, the known
sub-pixels of the state are overwritten with their own q(z_t | x) = alpha_t x + sigma_t eps -- a closed form per element,
by the same diagonal argument -- before the first step (at t = 1) and after every step t -> s (at gamma_s;
ops.inpaint_mix, mulan_inpaint_mix).  The last mix (s = 0) takes zero noise, so the known sub-pixels of z_0 are exactly
alpha_0 x and decode back to the input's integers.  With resample = U > 1 every step but the last is followed by U - 1
rounds of: the forward transition q(z_t | z_s) back to t on fresh noise (ops.forward_jump, mulan_forward_jump), the step
t -> s again at first order, and the mix; the history a repeated step leaves serves the next step as usual.
The noise of the known region and of the jumps is known_noise_fn(j), j a counter of its own (run states the law).

Restoration (range / null-space projection, DDNM): given a measurement y = A x of a degradation whose groups of
sub-pixels A averages -- super-resolution 'sr:f', colourisation 'gray', or both -- the prediction x_hat of every step is
replaced by x_hat' = x_hat + A+ (y - A x_hat) (ops.restore_project, mulan_restore_project) and the step runs on x_hat' as
a data prediction (mode 2 of the same step kernels); the multistep history is x_hat'.  The projection lives in data
space, so the different schedules inside a group do not enter.  resample = U > 1 is DDNM's time travel: U - 1 rounds of
jump and first-order step after every step but the last.

Time grids (make_grid; the keyword `grid`): uniform in t (the default), quadratic in t, or spaced on the mean schedule
of the batch -- uniform in its log signal-to-noise ratio ('logsnr') or the EDM grid ('karras').  The mean of the
polynomial schedules of a batch is a quintic in t, whose five coefficients and roots two HIP kernels give
(ops.schedule_moments, ops.schedule_invert; model.schedule_times); the times are read back once per batch and go
through time_grid's checks like an explicit t_grid, so the steppers never see which kind a grid was.

One loop (run) and one step body (solver_step) serve the plain, the inpainting and the restoring run, for the stepper of
this module and for the models' replayed one; check_guidance is the one place that decides which of the three a run is.
"""
import collections

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


GRIDS = ("uniform", "logsnr", "karras", "quadratic")
HOST_GRIDS = ("uniform", "quadratic")       # grids that need no schedule: the others invert the batch's mean schedule
BISECT_HALVINGS = 32


def check_grid(sampler, grid="uniform", t_grid=None, rho=7.0):
    """the public keywords `grid` and `grid_rho` of a sampler -> (grid, rho): the kind is one of GRIDS, anything but
    'uniform' excludes an explicit t_grid and the ancestral sampler, and rho (karras) is finite and > 0"""
    check_sampler(sampler)
    if grid not in GRIDS:
        raise ValueError(f"unknown grid {grid!r} (one of {', '.join(GRIDS)})")
    try:
        rho = float(rho)
    except (TypeError, ValueError):
        raise ValueError(f"grid_rho must be a finite number > 0, got {rho!r}") from None
    if not (np.isfinite(rho) and rho > 0.0):
        raise ValueError(f"grid_rho must be a finite number > 0, got {rho!r}")
    if grid != "uniform":
        if t_grid is not None:
            raise ValueError(f"grid = {grid!r} and an explicit t_grid both name the times: pass t_grid alone "
                             "(grid = 'uniform'), or drop it")
        if sampler not in FAST_SAMPLERS:
            raise ValueError(f"grid = {grid!r} belongs to the few-step samplers ({', '.join(FAST_SAMPLERS)}); the "
                             f"{sampler!r} sampler steps on its own T uniform times: use grid = 'uniform'")
    return grid, rho


def check_steps(steps):
    if steps is None or int(steps) != steps or steps < 1:
        raise ValueError(f"the number of sampling steps must be an integer >= 1, got {steps!r}")
    return int(steps)


def grid_targets(grid, steps, g0, g1, rho=7.0):
    """-> float64 [N - 1]: the values gamma_bar takes at the interior times t_1 .. t_{N-1} of a 'logsnr' or 'karras'
    grid, g0 = gamma_bar(0) and g1 = gamma_bar(1) its ends.  logsnr: linear in i from g1 to g0.  karras: with
    sigma / alpha = exp(gamma / 2), (sigma / alpha)^(1 / rho) is linear in i between its end values (the EDM grid)"""
    N = check_steps(steps)
    g0, g1 = float(g0), float(g1)
    w = np.arange(1, N, dtype=np.float64) / N
    if grid == "logsnr":
        return g1 + (g0 - g1) * w
    if grid == "karras":
        r1, r0 = np.exp(g1 / (2.0 * rho)), np.exp(g0 / (2.0 * rho))
        return 2.0 * rho * np.log(r1 + (r0 - r1) * w)
    raise ValueError(f"grid {grid!r} has no targets: it needs no schedule")


def bisect_times(gamma_fn, targets, halvings=BISECT_HALVINGS):
    """-> the times t in [0, 1] with gamma_fn(t) = targets, for an increasing gamma_fn that maps a tensor of times to
    the tensor of its values: all targets at once, `halvings` halvings of [0, 1], in the dtype and on the device of
    `targets` (a torch tensor).  A target at or beyond an end value gives that end exactly"""
    lo, hi = torch.zeros_like(targets), torch.ones_like(targets)
    g_lo, g_hi = gamma_fn(lo), gamma_fn(hi)
    for _ in range(halvings):
        mid = 0.5 * (lo + hi)
        below = gamma_fn(mid) < targets
        lo, hi = torch.where(below, mid, lo), torch.where(below, hi, mid)
    t = 0.5 * (lo + hi)
    t = torch.where(targets >= g_hi, torch.ones_like(t), t)
    return torch.where(targets <= g_lo, torch.zeros_like(t), t)


def make_grid(grid="uniform", steps=None, t_grid=None, rho=7.0, ends_fn=None, times_fn=None):
    """-> float64 [N + 1] from 1 to 0, through time_grid's checks: the grid kind `grid` over `steps` steps (or, with
    'uniform', the explicit t_grid).
      uniform ..... t_i = 1 - i / N (time_grid, as without the keyword)
      quadratic ... t_i = (1 - i / N)^2
      logsnr ...... gamma_bar(t_i) linear in i: uniform in the log signal-to-noise ratio of the mean schedule
      karras ...... (sigma / alpha)^(1 / rho) of the mean schedule linear in i
    The last two take the schedule from the caller: ends_fn() -> (gamma_bar(0), gamma_bar(1)) and times_fn(targets
    float64 [N - 1]) -> the times there, as fp32 values (array or tensor; read back here, once).  t_0 = 1 and t_N = 0
    are set here."""
    if grid == "uniform":
        return time_grid(steps, t_grid)
    N = check_steps(steps)
    if grid == "quadratic":
        return time_grid(N, (1.0 - np.arange(N + 1, dtype=np.float64) / N) ** 2)
    if ends_fn is None or times_fn is None:
        raise ValueError(f"grid = {grid!r} needs the schedule (its end values and its inverse)")
    inner = np.zeros(0)
    if N > 1:
        g0, g1 = ends_fn()
        inner = times_fn(grid_targets(grid, N, g0, g1, rho))
        inner = (inner.detach().cpu().numpy() if torch.is_tensor(inner) else np.asarray(inner)).astype(np.float64)
    try:
        return time_grid(N, np.concatenate([[1.0], inner.reshape(-1), [0.0]]))
    except ValueError as e:
        raise ValueError(f"the {grid!r} grid of {N} steps is no time grid on this schedule ({e}): use fewer steps or "
                         "another grid") from None


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


ZERO_NOISE = -1                     # the `mix` argument of an inpainting step whose mix takes no noise (the last step)


def check_resample(resample):
    """the passes per step of an inpainting run: an integer >= 1 (1: no resampling)"""
    try:
        ok = not isinstance(resample, bool) and int(resample) == resample and resample >= 1
    except (TypeError, ValueError, OverflowError):          # (None, a string, NaN, an infinity)
        ok = False
    if not ok:
        raise ValueError(f"resample must be an integer >= 1, got {resample!r}")
    return int(resample)


def check_inpaint(sampler, known, mask, resample=1):
    """-> whether the run inpaints: the known image and the mask go together, belong to the few-step samplers, and
    resample > 1 needs them"""
    check_sampler(sampler)
    resample = check_resample(resample)
    if (known is None) != (mask is None):
        raise ValueError("inpainting needs the known image and its mask together")
    if mask is None:
        if resample != 1:
            raise ValueError("resample applies to inpainting (a known image and a mask)")
        return False
    if sampler not in FAST_SAMPLERS:
        raise ValueError(f"inpainting runs with the few-step samplers ({', '.join(FAST_SAMPLERS)}); "
                         f"the {sampler!r} sampler takes no mask")
    return True


DEGRADATION_GRAMMAR = "'sr:f', 'gray' or 'sr:f+gray' with f one of 2, 4, 8, 16"


def parse_degradation(spec):
    """a degradation named in words -> (f, gray): 'sr:f' (f x f average pooling per channel, f in 2, 4, 8, 16) -> (f, False);
    'gray' (the channel mean) -> (1, True); 'sr:f+gray' (both) -> (f, True).  A pair (f, gray) passes through checked."""
    if isinstance(spec, (tuple, list)) and len(spec) == 2:
        f, gray = spec
        if not isinstance(f, bool) and f in ops.RESTORE_FACTORS + (1,) and (gray or f != 1):
            return int(f), bool(gray)
    elif isinstance(spec, str):
        sr, plus, tail = spec.partition("+")
        if spec == "gray":
            return 1, True
        kind, colon, arg = sr.partition(":")
        if kind == "sr" and colon and arg in tuple(str(f) for f in ops.RESTORE_FACTORS) and (not plus or tail == "gray"):
            return int(arg), bool(plus)
    raise ValueError(f"degradation {spec!r}: expected {DEGRADATION_GRAMMAR}")


def check_restore(sampler, measurement, degradation, resample=1, known=None, mask=None):
    """-> whether the run restores: the measurement and its degradation go together, belong to the few-step samplers, and
    exclude inpainting (a known image or a mask); resample must be an integer >= 1 either way"""
    check_sampler(sampler)
    check_resample(resample)
    if (measurement is None) != (degradation is None):
        raise ValueError("restoration needs the measurement and its degradation together")
    if measurement is None:
        return False
    if sampler not in FAST_SAMPLERS:
        raise ValueError(f"restoration runs with the few-step samplers ({', '.join(FAST_SAMPLERS)}); "
                         f"the {sampler!r} sampler takes no measurement")
    if known is not None or mask is not None:
        raise ValueError("a mask and a measurement in one run are not supported: inpaint or restore")
    parse_degradation(degradation)
    return True


Guidance = collections.namedtuple("Guidance", "inpaint restore resample")


def check_guidance(sampler, known=None, mask=None, measurement=None, degradation=None, resample=1):
    """what guides a run, checked once for every layer that takes these keywords -> Guidance(inpaint: whether it
    inpaints, restore: (f, gray) of a restoring run or None, resample: the passes per step as an int); raises what
    check_restore and then check_inpaint raise"""
    restoring = check_restore(sampler, measurement, degradation, resample, known, mask)
    inpaint = check_inpaint(sampler, known, mask, 1 if restoring else resample)
    return Guidance(inpaint, parse_degradation(degradation) if restoring else None, check_resample(resample))


def mask_from_spec(spec):
    """a mask named in words -> bool [32, 32] (True = keep):
    'box:y0,x0,y1,x1'  the rows y0 .. y1 - 1 and columns x0 .. x1 - 1 are unknown, the rest is kept
    'half:left|right|top|bottom'  that half of the image is kept"""
    kind, _, arg = str(spec).partition(":")
    keep = np.ones((32, 32), dtype=bool)
    if kind == "box":
        try:
            y0, x0, y1, x1 = (int(v) for v in arg.split(","))
        except ValueError:
            raise ValueError(f"mask {spec!r}: box takes four integers y0,x0,y1,x1") from None
        if not (0 <= y0 < y1 <= 32 and 0 <= x0 < x1 <= 32):
            raise ValueError(f"mask {spec!r}: the box needs 0 <= y0 < y1 <= 32 and 0 <= x0 < x1 <= 32")
        keep[y0:y1, x0:x1] = False
        return keep
    if kind == "half" and arg in ("left", "right", "top", "bottom"):
        keep[:] = False
        keep[{"left": np.s_[:, :16], "right": np.s_[:, 16:], "top": np.s_[:16], "bottom": np.s_[16:]}[arg]] = True
        return keep
    raise ValueError(f"mask {spec!r}: expected box:y0,x0,y1,x1 or half:left|right|top|bottom")


def expand_mask(mask, B, device=None):
    """a mask of shape [32, 32], [B, 32, 32] or [B, 32, 32, 3] (bool or uint8, non-zero = keep; array or tensor) -> uint8
    [B, 3072], one byte (0 / 1) per sub-pixel"""
    m = mask if torch.is_tensor(mask) else torch.tensor(np.asarray(mask))       # (a copy: the array may be read-only)
    if m.dtype not in (torch.bool, torch.uint8):
        raise ValueError(f"the mask is bool or uint8, got {m.dtype}")
    shape = tuple(m.shape)
    if shape == (32, 32):
        m = m[None, :, :, None]
    elif shape == (B, 32, 32):
        m = m[:, :, :, None]
    elif shape != (B, 32, 32, 3):
        raise ValueError(f"the mask has shape [32, 32], [{B}, 32, 32] or [{B}, 32, 32, 3], got {list(shape)}")
    m = (m != 0).expand(B, 32, 32, 3).reshape(B, 3072).to(torch.uint8)
    return m.contiguous() if device is None else m.to(device).contiguous()


class EagerStepper:
    """One solver step at a time through ops.fast_sampler_step, the history in tensors of its own.
    net_fn(z, t) -> network output shaped like z; gamma_fn(t) -> gamma at the (fp32) time t, per element (shaped like
    z) or per sample ([B]).  With step_eta > 0 (check_eta) the step is ops.stochastic_sampler_step on xi = noise_fn(k),
    one standard normal per element for step k (the fifth argument of the call).
    known / mask (both or neither; shaped like z, the image as ops.encode_u8 gives it and one byte per element): the
    inpainting stepper, whose steps end with the mix at gamma_s on known_noise_fn(j) (the call's `mix` argument names
    j; ZERO_NOISE: the noiseless mix of the last step), and which has mix() for z_1 and jump() for the resampling.
    measurement / degradation (both or neither, and not with a mask): the restoring stepper.  Its step is net ->
    ops.restore_project -> the step kernel at mode 2 on x_hat', which is also the history it keeps; measurement: fp32
    shaped ops.restore_y_shape, in the scale of ops.encode_u8; hwc = (H, W, C) where z is not [B, H, W, C]; jump() as
    above, on known_noise_fn(j) (needed for resample > 1 only)."""

    def __init__(self, net_fn, gamma_fn, mode, step_eta=0.0, noise_fn=None, known=None, mask=None, known_noise_fn=None,
                 measurement=None, degradation=None, hwc=None):
        self.net_fn, self.gamma_fn, self.mode, self.hwc = net_fn, gamma_fn, int(mode), hwc
        self.step_eta, self.noise_fn = float(step_eta), noise_fn
        if self.step_eta > 0.0 and noise_fn is None:
            raise ValueError("a stochastic step (step_eta > 0) needs noise_fn(k) -> xi")
        self.g_prev = self.x_prev = None
        self._g = None              # (t, gamma(t)) of the last step's s: the next step's t
        self.known = self.mask = self.known_noise_fn = self.measurement = self.degradation = None
        restoring = measurement is not None or degradation is not None
        if known is not None or mask is not None or (known_noise_fn is not None and not restoring):
            self.set_known(known, mask, known_noise_fn)
        if restoring:
            self.set_measurement(measurement, degradation, known_noise_fn)

    @property
    def inpaint(self):
        return self.mask is not None

    @property
    def restore(self):
        return self.measurement is not None

    def set_measurement(self, measurement, degradation, known_noise_fn=None):
        if self.inpaint:
            raise ValueError("a mask and a measurement in one run are not supported: inpaint or restore")
        if measurement is None or degradation is None:
            raise ValueError("restoration needs the measurement and its degradation together")
        self.measurement, self.degradation = measurement, parse_degradation(degradation)
        self.known_noise_fn = known_noise_fn

    def set_known(self, known, mask, known_noise_fn):
        if known is None or mask is None:
            raise ValueError("inpainting needs the known image and its mask together")
        if known_noise_fn is None:
            raise ValueError("inpainting needs known_noise_fn(j) -> the noise of the known region and of the jumps")
        self.known, self.mask, self.known_noise_fn = known, mask, known_noise_fn

    def _gamma(self, t):
        if self._g is not None and self._g[0] == t:
            return self._g[1]
        return self.gamma_fn(t)

    def _known_xi(self, j):
        return None if j == ZERO_NOISE else self.known_noise_fn(j)

    def mix(self, z, t, j):
        """the known sub-pixels of z replaced by alpha_t x + sigma_t known_noise_fn(j)"""
        return ops.inpaint_mix(z, self.known, self.mask, self._gamma(f32(t)), self._known_xi(j))

    def jump(self, z, s, t, j):
        """z_t ~ q(z_t | z_s = z) on known_noise_fn(j)"""
        s, t = f32(s), f32(t)
        if self.known_noise_fn is None:
            raise ValueError("a jump needs known_noise_fn(j) -> its noise")
        return ops.forward_jump(z, self._gamma(s), self.gamma_fn(t), self.known_noise_fn(j))

    def __call__(self, z, t, s, order, k=None, mix=None):
        if (mix is not None) != self.inpaint:
            raise ValueError("an inpainting stepper mixes after every step, and no other stepper does")
        t, s = f32(t), f32(s)
        g_t = self._gamma(t)
        g_s = self.gamma_fn(s)
        net = self.net_fn(z, t)
        if order == 2 and self.g_prev is None:
            raise RuntimeError("a second-order step needs the history of a previous step")
        if self.step_eta > 0.0 and k is None:
            raise ValueError("a stochastic step needs its index k (the noise is drawn per step)")
        z_s, x0 = solver_step(z, net, g_t, g_s, self.mode, (self.g_prev, self.x_prev) if order == 2 else (None, None),
                              (lambda: self.noise_fn(k)) if self.step_eta > 0.0 else None, self.step_eta, self.known,
                              self.mask, (lambda: self._known_xi(mix)) if self.inpaint else None, self.measurement,
                              self.degradation, self.hwc)
        self.g_prev, self.x_prev, self._g = g_t, x0, (s, g_s)       # (a restoring step's x0, the history, is x_hat')
        return z_s


def solver_step(z, net, g_t, g_s, mode, hist, xi=None, step_eta=0.0, known=None, mask=None, known_xi=None,
                measurement=None, restore=None, hwc=None):
    """the body of one step t -> s, behind the network: -> (z_s, x0).  restore = (f, gray) with its measurement: net is
    projected onto the measurement first (ops.restore_project; hwc where z is not [B, H, W, C]) and the step runs on
    x_hat' at mode 2, so x0 is x_hat'.  The step is ops.stochastic_sampler_step on the noise xi at step_eta where xi is
    given, else ops.fast_sampler_step; hist = (g_prev, x_prev), or (None, None) at first order.  With a mask the known
    sub-pixels of z_s are then replaced in place by alpha_s known + sigma_s known_xi (None: zero noise).  xi and known_xi
    are tensors (static buffers, under graph capture) or thunks that draw them, called where the noise is needed."""
    if restore is not None:
        net, mode = ops.restore_project(z, net, g_t, measurement, *restore, mode, hwc), 2
    if xi is not None:
        z_s, x0 = ops.stochastic_sampler_step(z, net, g_t, g_s, mode, xi() if callable(xi) else xi, step_eta, *hist)
    else:
        z_s, x0 = ops.fast_sampler_step(z, net, g_t, g_s, mode, *hist)
    if mask is not None:
        z_s = ops.inpaint_mix(z_s, known, mask, g_s, known_xi() if callable(known_xi) else known_xi, out=z_s)
    return z_s, x0


def run(stepper, z, grid, orders, resample=1, known=None, mask=None, known_noise_fn=None):
    """the solver loop, the only one: stepper(z, t, s, order, k[, mix]) -> z_s along the grid; the step's index k selects
    the noise of a stochastic step.  known / mask / known_noise_fn: handed to the stepper first (set_known).
    An inpainting stepper (stepper.inpaint) has z_1 mixed at t = 1 (stepper.mix) and every step t -> s followed by the
    mix at gamma_s, inside the stepper's call, which takes the `mix` argument: the draw j, or ZERO_NOISE at the last
    step.  With resample = U > 1 an inpainting or a restoring stepper (stepper.restore: every step projects its
    prediction onto the measurement) follows every step but the last with U - 1 rounds of jump s -> t (stepper.jump;
    DDNM's time travel) and the step t -> s again at first order, with its mix where there is one.  Any other stepper
    takes N plain steps, and resample != 1 is refused.
    Noise: the known region's and the jumps' noise is draw j of the stepper's known_noise_fn, one counter for both.  A
    deterministic run without resampling (step_eta = 0 and U = 1) uses j = 0 at every mix, so the known region follows
    alpha_t x + sigma_t eps with one eps: a consistent trajectory for an ODE solver.  Otherwise every mix and every jump
    takes the next j = 0, 1, 2, ... in the order they run (the mix of z_1 first; per round the jump, then the mix); a
    restoring run has no mixes, so j counts its jumps, and with U = 1 it draws nothing.  Round r = 1 .. U - 1 of step k
    draws the noise of its stochastic step under the step index k + r N (N steps), which no first pass uses."""
    assert len(orders) == len(grid) - 1
    if known is not None or mask is not None:
        stepper.set_known(known, mask, known_noise_fn)
    U, N = check_resample(resample), len(orders)
    inpaint = bool(getattr(stepper, "inpaint", False))
    if U != 1 and not inpaint and not getattr(stepper, "restore", False):
        raise ValueError("resample applies to inpainting (a known image and a mask) and to restoration (a measurement)")
    fresh = U > 1 or getattr(stepper, "step_eta", 0.0) > 0.0
    count = [0]

    def draw():
        j = count[0]
        count[0] += int(fresh)
        return j
    if inpaint:
        z = stepper.mix(z, grid[0], draw())
    for k, order in enumerate(orders):
        t, s, last = grid[k], grid[k + 1], k == N - 1
        for r in range(1 if last else U):
            if r > 0:
                z = stepper.jump(z, s, t, draw())
            mix = (ZERO_NOISE if last else draw(),) if inpaint else ()
            z = stepper(z, t, s, 1 if r > 0 else order, k + r * N, *mix)
    return z


def sample(net_fn, gamma_fn, z, mode, sampler="dpm2m", steps=None, t_grid=None, eta=0.0, noise_fn=None, known=None,
           mask=None, known_noise_fn=None, resample=1, measurement=None, degradation=None, hwc=None, grid="uniform",
           grid_rho=7.0, gamma_bar_fn=None):
    """z_0 from z_1 = z by `sampler` (ddim | dpm2m | sde2m) over `steps` uniform steps or the explicit `t_grid`; mode as
    ops.fast_sampler_step (0: net_fn gives the velocity, 1: eps_hat, 2: x_hat).  eta (ddim only): 0 is the
    deterministic sampler; sde2m and ddim with eta > 0 need noise_fn(k) -> xi shaped like z, the noise of step k.
    known, mask (shaped like z: the image as ops.encode_u8 gives it, one byte per element, non-zero = keep): inpainting
    with `resample` passes per step, on known_noise_fn(j) -> xi shaped like z (run states which j is drawn when).
    measurement, degradation (a spec of parse_degradation, or its pair): restoration instead, the measurement fp32
    shaped ops.restore_y_shape in the scale of ops.encode_u8; z is [B, H, W, C] or hwc names (H, W, C); `resample`
    passes per step on known_noise_fn(j), the noise of jump j (run).
    grid (one of GRIDS; make_grid) with grid_rho for 'karras': 'logsnr' and 'karras' space the steps on the mean
    schedule, which gamma_fn does not give: gamma_bar_fn(t float64 array [M]) -> gamma_bar there (array or tensor),
    increasing in t; its inverse is taken here by bisection on the host in float64 (bisect_times)"""
    step_eta = check_eta(sampler, eta)
    check_guidance(sampler, known, mask, measurement, degradation, resample)
    grid, grid_rho = check_grid(sampler, grid, t_grid, grid_rho)
    if grid not in HOST_GRIDS and gamma_bar_fn is None:
        raise ValueError(f"grid = {grid!r} is spaced on the mean schedule: pass gamma_bar_fn(t) -> gamma_bar, or use "
                         f"one of {', '.join(HOST_GRIDS)}")

    def gamma_bar(t):
        g = gamma_bar_fn(t.numpy())
        return (g.detach().cpu() if torch.is_tensor(g) else torch.as_tensor(np.asarray(g))).to(torch.float64).reshape(-1)
    grid = make_grid(grid, steps, t_grid, grid_rho, lambda: gamma_bar(torch.tensor([0.0, 1.0], dtype=torch.float64)).tolist(),
                     lambda targets: bisect_times(gamma_bar, torch.as_tensor(targets), 60).numpy().astype(np.float32))
    orders = step_orders(sampler, len(grid) - 1)
    with torch.no_grad():
        return run(EagerStepper(net_fn, gamma_fn, mode, step_eta, noise_fn, known, mask, known_noise_fn, measurement,
                                degradation, hwc), z, grid, orders, resample)
