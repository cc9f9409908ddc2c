"""Float64 restatement of the deterministic few-step samplers (DDIM with eta = 0, DPM-Solver++(2M) per element in
lambda = -gamma / 2; mulan_amd.sampling) composed with the oracle's own pieces (oracle.torch_ref: score_unet, poly_gamma,
poly_coefficients, deterministic_embedding) into whole sampling loops of the MuLAN models and of the plain VDM."""
import numpy as np
import torch

from oracle import torch_ref as tr


def x_hat(z, net, g_t, kind):
    """the data prediction from the network output: 'velocity' (mode 0), 'epsilon' / 'vfe' (mode 1), 'input' (mode 2)"""
    alpha, sigma = torch.sqrt(torch.sigmoid(-g_t)), torch.sqrt(torch.sigmoid(g_t))
    if kind == "velocity":
        return alpha * z - sigma * net
    if kind == "input":
        return net
    return (z - sigma * net) / alpha


def fast_step(z, net, g_t, g_s, kind, g_p=None, x_p=None):
    """-> (z_s, x_hat_t, |d z_s / d net| per element); g_p / x_p None: first order"""
    xh = x_hat(z, net, g_t, kind)
    h = 0.5 * (g_t - g_s)
    alpha_s = torch.sqrt(torch.sigmoid(-g_s))
    em = torch.expm1(-h)
    d, dd = xh, torch.ones_like(xh)
    if g_p is not None:
        hp = 0.5 * (g_p - g_t)
        ok = (hp > 0) & torch.isfinite(hp)
        w = torch.where(ok, h / torch.where(ok, 2 * hp, torch.ones_like(hp)), torch.zeros_like(hp))
        d = torch.where(ok, (1 + w) * xh - w * x_p, xh)
        dd = torch.where(ok, 1 + w, dd)
    z_s = torch.sqrt(torch.sigmoid(g_s) / torch.sigmoid(g_t)) * z - alpha_s * em * d
    alpha_t, sigma_t = torch.sqrt(torch.sigmoid(-g_t)), torch.sqrt(torch.sigmoid(g_t))
    dx = {"velocity": sigma_t, "input": torch.ones_like(g_t)}.get(kind, sigma_t / alpha_t)
    return z_s, xh, (alpha_s * em.abs() * dd.abs() * dx) * torch.ones_like(z)


def orders(sampler, N):
    if sampler == "ddim":
        return [1] * N
    o = [1] + [2] * (N - 1)
    if N < 15:
        o[-1] = 1
    return o


def _loop(gamma, net_fn, z_init, grid, sampler, kind):
    """the solver loop: gamma(t) broadcastable against z, net_fn(z, g_t) the network output; times as fp32 values"""
    z = z_init
    traj, hist, budget = [z], [(None, None)], []
    g_p = x_p = None
    for k, order in enumerate(orders(sampler, len(grid) - 1)):
        t, s = float(np.float32(grid[k])), float(np.float32(grid[k + 1]))
        g_t, g_s = gamma(t), gamma(s)
        net = net_fn(z, g_t)
        z, xh, gain = fast_step(z, net, g_t, g_s, kind, *((g_p, x_p) if order == 2 else (None, None)))
        g_p, x_p = g_t, xh
        traj.append(z)
        hist.append((g_p, x_p))
        budget.append(float(gain.max()) * float(net.abs().max()))
    return z, traj, hist, budget


def mulan_fast_loop(params, cfg, z_init, grid, sampler, dtype=torch.float64):
    """sample_fn with a few-step sampler for the MuLAN models (deterministic embedding): (z_0, decoded uint8, per-step
    z, per-step history (g_t, x_hat_t) after the step, per-step budget = max gain x max |net|)"""
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
    z, traj, hist, budget = _loop(gamma, net_fn, z_init.reshape(shp).to(dtype), grid, sampler, kind)
    return z, tr.decode_argmax(z, gamma(0.0)), traj, hist, budget


def plain_fast_loop(params, cfg, z_init, grid, sampler, gmin=tr.GAMMA_MIN, gmax=tr.GAMMA_MAX, dtype=torch.float64):
    """the same for model_vdm.VDM with gamma_type 'fixed' (per-sample gamma, conditioning zeros)"""
    B = z_init.shape[0]
    shp = (B, 32, 32, 3)
    kind = "input" if cfg.get("reparam_type") == "input" else "epsilon"
    gamma = lambda t: torch.tensor(gmin + (gmax - gmin) * t, dtype=dtype)

    def net_fn(z, g_t):
        return tr.score_unet(z, g_t * torch.ones(B, dtype=dtype), torch.zeros(B, 1, dtype=dtype), params["score_model"],
                             cfg["n_embd"], cfg["n_layer"], gmin=gmin, gmax=gmax)
    z, traj, hist, budget = _loop(gamma, net_fn, z_init.reshape(shp).to(dtype), grid, sampler, kind)
    return z, tr.decode_argmax(z, gamma(0.0) * torch.ones(shp, dtype=dtype)), traj, hist, budget
