"""Float64 restatement of inpainting with the few-step samplers (mulan_amd.sampling.run_inpaint): the
mix that overwrites the known sub-pixels of a sampler state with their own q(z_t | x), the forward transition
q(z_t | z_s) of the resampling, the whole loop on given noise (the steps are those of tests/fast_sampler_oracle.py and
tests/stochastic_sampler_oracle.py, the networks and schedules those of their loops), and the exact law of the unknown
coordinates on a linear-Gaussian model."""
import numpy as np
import torch

from oracle import torch_ref as tr
from tests import stochastic_sampler_oracle as so


def mix(z, x, mask, g, xi=None):
    """mask ? alpha(g) x + sigma(g) xi : z  (xi None: zeros); a select, so what x and xi hold where mask is 0 is never
    read into the result"""
    alpha, sigma = torch.sqrt(torch.sigmoid(-g)), torch.sqrt(torch.sigmoid(g))
    known = alpha * x if xi is None else alpha * x + sigma * xi
    return torch.where(mask != 0, known * torch.ones_like(z), z)


def jump_coefficients(g_s, g_t):
    """(r, v) of q(z_t | z_s) = N(r z_s, v) for g_t >= g_s: r = alpha_t / alpha_s, v = sigma_t^2 (1 - e^(g_s - g_t))"""
    r = torch.sqrt(torch.sigmoid(-g_t) / torch.sigmoid(-g_s))
    return r, torch.sigmoid(g_t) * -torch.expm1(g_s - g_t)


def jump(z_s, g_s, g_t, xi):
    r, v = jump_coefficients(g_s, g_t)
    return r * z_s + torch.sqrt(v) * xi


def loop(gamma, net_fn, z_init, grid, sampler, eta, kind, x, mask, step_xi, known_xi, resample=1):
    """the inpainting loop of sampling.run_inpaint on given noise: step_xi(k) the noise of the stochastic step with index
    k (None where eta = 0), known_xi(j) draw j of the known region's and the jumps' noise.  z_1 is mixed at t = 1; every
    step t -> s ends with the mix at gamma_s, the last with zero noise; with resample = U > 1 every step but the last is
    followed by U - 1 rounds of jump s -> t, the step again at first order (step index k + r N), the mix.  eta = 0 and
    U = 1: j = 0 at every mix; otherwise j counts the draws in the order they run.
    -> (z_0, events): one dict per operation, kind 'mix' | 'step' | 'jump', with what went in and what came out"""
    orders = so.orders(sampler, len(grid) - 1)
    N, U = len(orders), int(resample)
    fresh = U > 1 or eta > 0
    count = [0]

    def draw():
        j = count[0]
        count[0] += int(fresh)
        return j
    f32 = lambda t: float(np.float32(t))
    events = []
    j = draw()
    z_in, z = z_init, mix(z_init, x, mask, gamma(f32(grid[0])), known_xi(j).reshape(z_init.shape))
    events.append(dict(kind="mix", t=f32(grid[0]), j=j, z_in=z_in, z_out=z))
    g_p = x_p = None

    def step(z, k, t, s, order, kk, j):
        nonlocal g_p, x_p
        g_t, g_s = gamma(t), gamma(s)
        net = net_fn(z, g_t)
        xi = torch.zeros_like(z) if eta == 0 else step_xi(kk).reshape(z.shape).to(z.dtype)
        hist = (g_p, x_p) if order == 2 else (None, None)
        z_s, xh, gain, kn = so.stochastic_step(z, net, g_t, g_s, kind, xi, eta, *hist)
        out = mix(z_s, x, mask, g_s, None if j is None else known_xi(j).reshape(z.shape))
        events.append(dict(kind="step", k=k, kk=kk, t=t, s=s, order=order, j=j, z_in=z, g_p=hist[0], x_p=hist[1],
                           z_out=out, budget=float(gain.max()) * float(net.abs().max()), noise=float(kn.max())))
        g_p, x_p = g_t, xh
        return out
    for k, order in enumerate(orders):
        t, s, last = f32(grid[k]), f32(grid[k + 1]), k == N - 1
        z = step(z, k, t, s, order, k, None if last else draw())
        if not last:
            for r in range(1, U):
                j = draw()
                z_t = jump(z, gamma(s), gamma(t), known_xi(j).reshape(z.shape))
                events.append(dict(kind="jump", s=s, t=t, j=j, z_in=z, z_out=z_t))
                z = step(z_t, k, t, s, 1, k + r * N, draw())
    return z, events


def mulan_loop(params, cfg, z_init, grid, sampler, eta, x, mask, step_xi, known_xi, resample=1, dtype=torch.float64):
    """the MuLAN models under the deterministic embedding, set up as stochastic_sampler_oracle.mulan_loop sets them up"""
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
    return loop(gamma, net_fn, z_init.reshape(shp).to(dtype), grid, sampler, eta, kind, x.reshape(shp).to(dtype),
                mask.reshape(shp), step_xi, known_xi, resample)


def plain_loop(params, cfg, z_init, grid, sampler, eta, x, mask, step_xi, known_xi, resample=1, gmin=tr.GAMMA_MIN,
               gmax=tr.GAMMA_MAX, dtype=torch.float64):
    """model_vdm.VDM with gamma_type 'fixed' (per-sample gamma, conditioning zeros), as plain_loop there sets it up"""
    B = z_init.shape[0]
    shp = (B, 32, 32, 3)
    kind = "input" if cfg.get("reparam_type") == "input" else "epsilon"
    gamma = lambda t: torch.tensor(gmin + (gmax - gmin) * t, dtype=dtype)

    def net_fn(z, g_t):
        return tr.score_unet(z, g_t * torch.ones(B, dtype=dtype), torch.zeros(B, 1, dtype=dtype), params["score_model"],
                             cfg["n_embd"], cfg["n_layer"], gmin=gmin, gmax=gmax)
    return loop(gamma, net_fn, z_init.reshape(shp).to(dtype), grid, sampler, eta, kind, x.reshape(shp).to(dtype),
                mask.reshape(shp), step_xi, known_xi, resample)


# ---------------------------------------------------------------------- linear-Gaussian model: the unknown coordinates
def jump_law(g_s, g_t, m, v):
    """the jump's affine map applied to N(m, v)"""
    r, vj = jump_coefficients(torch.tensor(g_s, dtype=torch.float64), torch.tensor(g_t, dtype=torch.float64))
    return float(r) * m, float(r) ** 2 * v + float(vj)


def inpaint_gaussian_law(gammas, mu, sd, eta, resample=1, m=0.0, v=1.0):
    """mean and variance of an unknown coordinate of z_0 when the first-order sampler with the exact posterior-mean
    denoiser (so.gaussian_law: every step affine in z_t) runs the inpainting loop over the float64 gammas (t = 1 down to
    0).  The denoiser acts per coordinate, so an unknown coordinate never sees a known one; the mixes leave it alone,
    and each resampling round composes the jump's affine map with the step's."""
    N = len(gammas) - 1
    for k in range(N):
        g_t, g_s = gammas[k], gammas[k + 1]
        m, v = so.gaussian_law([g_t, g_s], mu, sd, eta, m, v)
        if k < N - 1:
            for _ in range(1, int(resample)):
                m, v = jump_law(g_s, g_t, m, v)
                m, v = so.gaussian_law([g_t, g_s], mu, sd, eta, m, v)
    return m, v
