"""Float64 restatement of restoration with the few-step samplers (mulan_amd.sampling.run_restore): the
degradations whose pseudo-inverse is replication (A: group means; A+: replicate), the projection of a data prediction
onto a measurement, and the whole loop on given noise.  The steps are those of tests/stochastic_sampler_oracle.py on the
projected prediction as a data prediction (kind 'input'); networks and schedules are set up as tests/inpaint_oracle.py
sets them up."""
import numpy as np
import torch

from oracle import torch_ref as tr
from tests import fast_sampler_oracle as fo
from tests import inpaint_oracle as io
from tests import stochastic_sampler_oracle as so

SPECS = {"gray": (1, True), "sr:2": (2, False), "sr:4": (4, False), "sr:8": (8, False), "sr:16": (16, False),
         "sr:2+gray": (2, True), "sr:4+gray": (4, True), "sr:8+gray": (8, True), "sr:16+gray": (16, True)}


def group_size(f, gray, C=3):
    return f * f * (C if gray else 1)


def measure(x, f, gray):
    """A x for x [B, H, W, C]: the mean over f x f pixel blocks per channel, then over the channels if gray"""
    B, H, W, C = x.shape
    y = x.reshape(B, H // f, f, W // f, f, C)
    # f is a power of two: a pairwise tree, whose partial sums of equal addends are exact, so that A A+ y == y holds
    # bit for bit; the channel mean is taken about the first channel for the same reason (fl(fl(3 v) / 3) is not always v)
    while y.shape[2] > 1:
        h = y.shape[2] // 2
        y = y[:, :, :h] + y[:, :, h:]
    while y.shape[4] > 1:
        h = y.shape[4] // 2
        y = y[:, :, :, :, :h] + y[:, :, :, :, h:]
    y = y[:, :, 0, :, 0] / (f * f)
    if gray:
        acc = torch.zeros_like(y[..., 0])
        for c in range(1, C):
            acc = acc + (y[..., c] - y[..., 0])
        y = (y[..., 0] + acc / C)[..., None]
    return y


def replicate(y, f, gray, C=3):
    """A+ y: every group's value at all of its sub-pixels"""
    up = y.repeat_interleave(f, dim=1).repeat_interleave(f, dim=2)
    return up.expand(*up.shape[:3], C).clone() if gray else up


def project(xh, y, f, gray):
    """x_hat + A+ (y - A x_hat)"""
    return xh + replicate(y - measure(xh, f, gray), f, gray, xh.shape[3])


def loop(gamma, net_fn, z_init, grid, sampler, eta, kind, y, f, gray, step_xi, jump_xi, resample=1):
    """the restoring loop of sampling.run_restore on given noise: step_xi(k) the noise of the stochastic step with index k
    (never called where eta = 0), jump_xi(j) the noise of jump j = 0, 1, 2, ... in run order (never called where
    resample = 1).  Every step forms x_hat from the network output, projects it, and takes the solver step on x_hat' as
    a data prediction; the history is x_hat'.  With resample = U > 1 every step but the last is followed by U - 1 rounds
    of jump s -> t and the step again at first order (step index k + r N).
    -> (z_0, events): one dict per operation, kind 'step' | 'jump', with what went in and what came out; a step's
    `budget` is max |d z_s / d net| x max |net| with the projection's factor taken as 1"""
    orders = so.orders(sampler, len(grid) - 1)
    N, U = len(orders), int(resample)
    f32 = lambda t: float(np.float32(t))
    events = []
    g_p = x_p = None
    z, j = z_init, 0

    def step(z, k, t, s, order, kk):
        nonlocal g_p, x_p
        g_t, g_s = gamma(t), gamma(s)
        net = net_fn(z, g_t)
        xh = project(fo.x_hat(z, net, g_t, kind), y, f, gray)
        xi = torch.zeros_like(z) if eta == 0 else step_xi(kk).reshape(z.shape).to(z.dtype)
        hist = (g_p, x_p) if order == 2 else (None, None)
        z_s, x0, gain, kn = so.stochastic_step(z, xh, g_t, g_s, "input", xi, eta, *hist)
        alpha_t, sigma_t = torch.sqrt(torch.sigmoid(-g_t)), torch.sqrt(torch.sigmoid(g_t))
        dx = {"velocity": sigma_t, "input": torch.ones_like(g_t)}.get(kind, sigma_t / alpha_t)
        events.append(dict(kind="step", k=k, kk=kk, t=t, s=s, order=order, z_in=z, g_p=hist[0], x_p=hist[1], z_out=z_s,
                           xh=x0, budget=float((gain * dx).max()) * float(net.abs().max()), noise=float(kn.max())))
        g_p, x_p = g_t, x0
        return z_s
    for k, order in enumerate(orders):
        t, s = f32(grid[k]), f32(grid[k + 1])
        z = step(z, k, t, s, order, k)
        if k < N - 1:
            for r in range(1, U):
                z_t = io.jump(z, gamma(s), gamma(t), jump_xi(j).reshape(z.shape).to(z.dtype))
                events.append(dict(kind="jump", s=s, t=t, j=j, z_in=z, z_out=z_t))
                j += 1
                z = step(z_t, k, t, s, 1, k + r * N)
    return z, events


def mulan_loop(params, cfg, z_init, grid, sampler, eta, y, f, gray, step_xi, jump_xi, resample=1, dtype=torch.float64):
    """the MuLAN models under the deterministic embedding, set up as inpaint_oracle.mulan_loop sets them up"""
    B = z_init.shape[0]
    shp = (B, 32, 32, 3)
    emb = tr.deterministic_embedding(B, cfg.get("latent_size", 50), cfg["latent_k"], dtype)
    a, b, c = tr.poly_coefficients(emb, params["gamma"])
    per_pixel = cfg.get("unet_type", "vdm") == "ldm"
    if cfg["vdm_type"] == "mulan_velocity":
        kind = "vfe" if cfg.get("velocity_from_epsilon", False) else "velocity"
    else:
        kind = "epsilon"
    gamma = lambda t: tr.poly_gamma(a, b, c, torch.full((B,), t, dtype=dtype)).reshape(shp)

    def net_fn(z, g_t):
        g_in = g_t if per_pixel else g_t.reshape(B, -1).mean(dim=1)
        return tr.score_unet(z, g_in, emb, params["score_model"], cfg["n_embd"], cfg["n_layer"], per_pixel)
    return loop(gamma, net_fn, z_init.reshape(shp).to(dtype), grid, sampler, eta, kind, y.to(dtype), f, gray, step_xi,
                jump_xi, resample)


def plain_loop(params, cfg, z_init, grid, sampler, eta, y, f, gray, step_xi, jump_xi, resample=1, gmin=tr.GAMMA_MIN,
               gmax=tr.GAMMA_MAX, dtype=torch.float64):
    """model_vdm.VDM with gamma_type 'fixed' (per-sample gamma, conditioning zeros), as inpaint_oracle.plain_loop"""
    B = z_init.shape[0]
    shp = (B, 32, 32, 3)
    kind = "input" if cfg.get("reparam_type") == "input" else "epsilon"
    gamma = lambda t: torch.tensor(gmin + (gmax - gmin) * t, dtype=dtype)

    def net_fn(z, g_t):
        return tr.score_unet(z, g_t * torch.ones(B, dtype=dtype), torch.zeros(B, 1, dtype=dtype), params["score_model"],
                             cfg["n_embd"], cfg["n_layer"], gmin=gmin, gmax=gmax)
    return loop(gamma, net_fn, z_init.reshape(shp).to(dtype), grid, sampler, eta, kind, y.to(dtype), f, gray, step_xi,
                jump_xi, resample)
