"""Float64 restatement of the stochastic few-step samplers (DDIM with eta in [0, 1], SDE-DPM-Solver++(2M) per element in
lambda = -gamma / 2; mulan_amd.sampling) on given noise, the ancestral posterior step it meets at
eta = 1, whole sampling loops of the models (the networks and schedules of tests/fast_sampler_oracle.py), and the exact
law of the first-order sampler on a linear-Gaussian model."""
import numpy as np
import torch

from oracle import torch_ref as tr
from tests import fast_sampler_oracle as fo


def stochastic_step(z, net, g_t, g_s, kind, xi, eta, g_p=None, x_p=None):
    """-> (z_s, x_hat_t, |d z_s / d net| per element, |k_n xi| per element); g_p / x_p None: first order.
    z_s = k_z z_t + k_x D + k_n xi with c = 1 - e^(-2h), k_z = (sigma_s / sigma_t) sqrt(1 - eta^2 c),
    k_x = alpha_s (1 - e^(-h) sqrt(1 - eta^2 c)), k_n = eta sigma_s sqrt(c)"""
    xh = fo.x_hat(z, net, g_t, kind)
    h = 0.5 * (g_t - g_s)
    alpha_s, sigma_s = torch.sqrt(torch.sigmoid(-g_s)), torch.sqrt(torch.sigmoid(g_s))
    alpha_t, sigma_t = torch.sqrt(torch.sigmoid(-g_t)), torch.sqrt(torch.sigmoid(g_t))
    c = -torch.expm1(-2 * h)
    om = (1 - eta ** 2) + eta ** 2 * torch.exp(-2 * h)                  # 1 - eta^2 c
    k_z = (sigma_s / sigma_t) * torch.sqrt(om)
    k_x = -alpha_s * torch.expm1(-h + 0.5 * torch.log(om))
    k_n = eta * sigma_s * torch.sqrt(c)
    d, dd = xh, torch.ones_like(xh)
    if g_p is not None:
        hp = 0.5 * (g_p - g_t)
        ok = (hp > 0) & torch.isfinite(hp)
        w = torch.where(ok, h / torch.where(ok, 2 * hp, torch.ones_like(hp)), torch.zeros_like(hp))
        d = torch.where(ok, (1 + w) * xh - w * x_p, xh)
        dd = torch.where(ok, 1 + w, dd)
    z_s = k_z * z + k_x * d + k_n * xi
    dx = {"velocity": sigma_t, "input": torch.ones_like(g_t)}.get(kind, sigma_t / alpha_t)
    return z_s, xh, (k_x.abs() * dd.abs() * dx) * torch.ones_like(z), (k_n * xi).abs()


def ancestral_step(z, net, g_t, g_s, kind, eps):
    """the posterior step as the header comment of ancestral_step_kernel states it:
    z_s = sqrt(a / b) (z_t - sigma_t c eps_hat) + sqrt((1 - a) c) eps, a = sigmoid(-g_s), b = sigmoid(-g_t),
    c = -expm1(g_s - g_t)"""
    a, b, c = torch.sigmoid(-g_s), torch.sigmoid(-g_t), -torch.expm1(g_s - g_t)
    alpha_t, sigma_t = torch.sqrt(b), torch.sqrt(torch.sigmoid(g_t))
    if kind == "velocity":
        eh = net * alpha_t + sigma_t * z
    elif kind == "input":
        eh = (z - alpha_t * net) / sigma_t
    else:
        eh = net
    return torch.sqrt(a / b) * (z - sigma_t * c * eh) + torch.sqrt((1 - a) * c) * eps


def orders(sampler, N):
    """sde2m runs the order schedule of dpm2m"""
    return fo.orders("dpm2m" if sampler == "sde2m" else sampler, N)


def _loop(gamma, net_fn, z_init, grid, sampler, eta, kind, xis):
    """the solver loop on the noise xis[k] of step k: (z_0, per-step z, per-step history (g_t, x_hat_t) after the
    step, per-step budget = max gain x max |net|, per-step max |k_n xi|)"""
    z = z_init
    traj, hist, budget, noise = [z], [(None, None)], [], []
    g_p = x_p = None
    for k, order in enumerate(orders(sampler, len(grid) - 1)):
        t, s = float(np.float32(grid[k])), float(np.float32(grid[k + 1]))
        g_t, g_s = gamma(t), gamma(s)
        net = net_fn(z, g_t)
        z, xh, gain, kn = stochastic_step(z, net, g_t, g_s, kind, xis[k].reshape(z.shape).to(z.dtype), eta,
                                          *((g_p, x_p) if order == 2 else (None, None)))
        g_p, x_p = g_t, xh
        traj.append(z)
        hist.append((g_p, x_p))
        budget.append(float(gain.max()) * float(net.abs().max()))
        noise.append(float(kn.max()))
    return z, traj, hist, budget, noise


def mulan_loop(params, cfg, z_init, grid, sampler, eta, xis, dtype=torch.float64):
    """the MuLAN models under the deterministic embedding, as fast_sampler_oracle.mulan_fast_loop sets them up"""
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
    return _loop(gamma, net_fn, z_init.reshape(shp).to(dtype), grid, sampler, eta, kind, xis)


def plain_loop(params, cfg, z_init, grid, sampler, eta, xis, gmin=tr.GAMMA_MIN, gmax=tr.GAMMA_MAX, dtype=torch.float64):
    """model_vdm.VDM with gamma_type 'fixed' (per-sample gamma, conditioning zeros), as plain_fast_loop sets it up"""
    B = z_init.shape[0]
    shp = (B, 32, 32, 3)
    kind = "input" if cfg.get("reparam_type") == "input" else "epsilon"
    gamma = lambda t: torch.tensor(gmin + (gmax - gmin) * t, dtype=dtype)

    def net_fn(z, g_t):
        return tr.score_unet(z, g_t * torch.ones(B, dtype=dtype), torch.zeros(B, 1, dtype=dtype), params["score_model"],
                             cfg["n_embd"], cfg["n_layer"], gmin=gmin, gmax=gmax)
    return _loop(gamma, net_fn, z_init.reshape(shp).to(dtype), grid, sampler, eta, kind, xis)


# ---------------------------------------------------------------------- linear-Gaussian model: the law of z_0
def posterior_mean(z, g, mu, sd):
    """E[x | z_t = z] for x ~ N(mu, sd^2), z_t = alpha x + sigma eps"""
    al2, si2 = torch.sigmoid(-g), torch.sigmoid(g)
    return mu + torch.sqrt(al2) * sd ** 2 * (z - torch.sqrt(al2) * mu) / (al2 * sd ** 2 + si2)


def gaussian_law(gammas, mu, sd, eta, m=0.0, v=1.0):
    """mean and variance of z_0 when z_1 ~ N(m, v) runs the first-order sampler with the exact posterior-mean denoiser
    over the float64 gammas (from t = 1 down to t = 0): every step is affine in z_t,
    z_s = (k_z + k_x alpha_t sd^2 / V) z_t + k_x mu sigma_t^2 / V + k_n xi with V = alpha_t^2 sd^2 + sigma_t^2, so
    m <- A m + b, v <- A^2 v + k_n^2, exactly"""
    for g_t, g_s in zip(gammas[:-1], gammas[1:]):
        g_t, g_s = torch.tensor(g_t, dtype=torch.float64), torch.tensor(g_s, dtype=torch.float64)
        h = 0.5 * (g_t - g_s)
        al2, si2 = torch.sigmoid(-g_t), torch.sigmoid(g_t)
        alpha_s, sigma_s = torch.sqrt(torch.sigmoid(-g_s)), torch.sqrt(torch.sigmoid(g_s))
        om = (1 - eta ** 2) + eta ** 2 * torch.exp(-2 * h)
        k_z = sigma_s / torch.sqrt(si2) * torch.sqrt(om)
        k_x = -alpha_s * torch.expm1(-h + 0.5 * torch.log(om))
        k_n2 = eta ** 2 * sigma_s ** 2 * -torch.expm1(-2 * h)
        V = al2 * sd ** 2 + si2
        A = float(k_z + k_x * torch.sqrt(al2) * sd ** 2 / V)
        b = float(k_x * mu * si2 / V)
        m, v = A * m + b, A * A * v + float(k_n2)
    return m, v
