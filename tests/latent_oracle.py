"""Float64 restatement of the two alternate MuLAN latents (latent_type 'gumbel' and 'gaussian') and of
UnetEncoderGaussian's two-headed output, composed with the oracle's own pieces (oracle.torch_ref) into a whole-model
forward pass: tr.mulan_forward with the latent swapped.

  gumbel   : ldm/model_mulan_velocity.py:68-92 (_get_gumbel_embedding, _gumbel_kl_loss, _gumbel_embedding_and_loss)
  gaussian : ldm/model_mulan_velocity.py:132-138 (_get_embedding_and_kl_z) with UnetEncoderGaussian
             (ldm/model_mulan_epsilon.py:24-80)
"""
import math

import numpy as np
import torch
import torch.nn.functional as F

from oracle import torch_ref as tr


def gumbel_tau(step):
    """max(0.5, exp(-1e-5 step)) in fp32, as jnp evaluates it"""
    return float(np.maximum(np.float32(0.5), np.exp(np.float32(-1e-5) * np.float32(step))))


def gumbel_latent(logits, gumbel, tau):
    """-> (embedding, kl): straight-through one-hot of (logits + g) / tau, first index on ties like jnp.argmax"""
    L = logits.shape[1]
    y = (logits + gumbel) / tau
    soft = torch.softmax(y, dim=1)
    hard = F.one_hot(torch.argmax(y, dim=1), L).to(logits.dtype)
    q = torch.softmax(logits, dim=1)
    kl = torch.sum(q * (torch.log_softmax(logits, dim=1) - math.log(1.0 / L)), dim=1)
    return (hard - soft).detach() + soft, kl


def gaussian_latent(mu, var, eps_z):
    """-> (embedding, kl) of the reparameterised draw mu + sqrt(var) eps_z"""
    emb = mu + torch.sqrt(var) * eps_z
    kl = 0.5 * torch.sum(mu ** 2 + var - torch.log(var) - 1., dim=1)
    return emb, kl


def unet_encoder_gaussian(f, p, n_embd, n_layers, masks=None, keep=1.0):
    """UnetEncoderGaussian.__call__ -> (mu, var = softplus(sigma head))"""
    B = f.shape[0]
    h, _, _ = tr.unet_stem(f, torch.zeros(B, dtype=f.dtype), torch.zeros(B, 1, dtype=f.dtype), p, n_embd, n_layers,
                           False, masks, keep)
    h = tr.conv3x3(tr.swish(tr.group_norm(h, p["GroupNorm_0"])), p["conv_out"])
    h = tr.swish(h.reshape(B, -1))
    return tr.dense(h, p["dense_layer_final_mu"]), F.softplus(tr.dense(h, p["dense_layer_final_sigma"]))


def gaussian_params(params, seed=0):
    """a gaussian-encoder tree from a tr.init_params tree: dense_layer_final replaced by the two heads"""
    g = torch.Generator().manual_seed(seed)
    enc = dict(params["encoder_model"])
    old = enc.pop("dense_layer_final")
    K, L = old["kernel"].shape
    for name in ("dense_layer_final_mu", "dense_layer_final_sigma"):
        enc[name] = {"kernel": (torch.randn(K, L, generator=g, dtype=torch.float64) / math.sqrt(K)).to(old["kernel"].dtype),
                     "bias": (0.1 * torch.randn(L, generator=g, dtype=torch.float64)).to(old["bias"].dtype)}
    return dict(params, encoder_model=enc)


def mulan_forward(params, cfg, x_u8, t0, latent_noise, eps_0, eps, latent_type, tau=1.0, enc_masks=None,
                  score_masks=None, keep=1.0, dtype=torch.float64, t=None, emb_value=None):
    """tr.mulan_forward with latent_type 'gumbel' (latent_noise: Gumbel draws [B,L]) or 'gaussian' (latent_noise: eps_z
    [B,L]); cfg as for tr.mulan_forward (vdm_type, n_embd, n_layer, forward_n_layer, unet_type, velocity_from_epsilon,
    n_timesteps).  emb_value (optional, [B,L]): the VALUE of the embedding the schedule and the score model see, the
    gradient still flowing to the encoder through this function's own embedding (straight-through).  The polynomial
    schedule is ill-conditioned in a continuous embedding: at a random initialisation a 1e-5 relative change of a
    gaussian draw moves the gamma network's weight gradients by 2 %, so a comparison of those gradients with an fp32
    model feeds both the same embedding."""
    B = x_u8.shape[0]
    x = x_u8.reshape(B, 32, 32, 3)
    if t is None:
        t = torch.remainder(t0 + torch.arange(B, dtype=dtype) / B, 1.)
    if cfg.get("n_timesteps", 0) > 0:
        t = torch.ceil(t * cfg["n_timesteps"]) / cfg["n_timesteps"]
    f = tr.encode(x.to(dtype))
    enc = params["encoder_model"]
    if latent_type == "gaussian":
        mu, var = unet_encoder_gaussian(f, enc, cfg["n_embd"], cfg["forward_n_layer"], enc_masks, keep)
        emb, kl_z = gaussian_latent(mu, var, latent_noise)
        logits = (mu, var)
    elif latent_type == "gumbel":
        logits = tr.unet_encoder(f, enc, cfg["n_embd"], cfg["forward_n_layer"], enc_masks, keep)
        emb, kl_z = gumbel_latent(logits, latent_noise, tau)
    else:
        raise ValueError(latent_type)
    if emb_value is not None:
        emb = emb_value.to(emb.dtype) + (emb - emb.detach())
    a, b, c = tr.poly_coefficients(emb, params["gamma"])
    shp = f.shape
    g_0 = tr.poly_gamma(a, b, c, torch.zeros(B, dtype=dtype)).reshape(shp)
    g_1 = tr.poly_gamma(a, b, c, torch.ones(B, dtype=dtype)).reshape(shp)
    g_t = tr.poly_gamma(a, b, c, t).reshape(shp)
    g_p = tr.poly_gamma_grad_t(a, b, c, t).reshape(shp)
    var_t, var_0, var_1 = torch.sigmoid(g_t), torch.sigmoid(g_0), torch.sigmoid(g_1)
    z_0 = f + torch.exp(0.5 * g_0) * eps_0
    loss_recon = -tr.logprob(x, z_0, g_0)
    loss_klz = 0.5 * ((1. - var_1) * f * f + var_1 - torch.log(var_1) - 1.).reshape(B, -1).sum(dim=1)
    z_t = torch.sqrt(1. - var_t) * f + torch.sqrt(var_t) * eps
    per_pixel = cfg.get("unet_type", "vdm") == "ldm"
    g_in = g_t if per_pixel else g_t.reshape(B, -1).mean(dim=1)
    net = tr.score_unet(z_t, g_in, emb, params["score_model"], cfg["n_embd"], cfg["n_layer"], per_pixel,
                        masks=score_masks, keep=keep)
    if cfg["vdm_type"] == "mulan_velocity":
        v_hat = net
        if cfg.get("velocity_from_epsilon", False):
            v_hat = -torch.exp(0.5 * g_t) * z_t + torch.sqrt(1 + torch.exp(g_t)) * net
        v_target = torch.sqrt(1. - var_t) * eps - torch.sqrt(var_t) * f
        loss_diff = .5 * ((1 - var_t) * g_p * (v_target - v_hat) ** 2).reshape(B, -1).sum(dim=1)
    elif cfg.get("n_timesteps", 0) == 0:
        loss_diff = .5 * (g_p * (eps - net) ** 2).reshape(B, -1).sum(dim=1)
    else:
        T = cfg["n_timesteps"]
        g_s = tr.poly_gamma(a, b, c, t - 1. / T).reshape(shp)
        loss_diff = .5 * T * (torch.expm1(g_t - g_s) * (eps - net) ** 2).reshape(B, -1).sum(dim=1)
    klz = kl_z + loss_klz
    r = 1. / (3072 * math.log(2.))
    return dict(loss_recon=loss_recon, loss_klz=klz, loss_diff=loss_diff, var_0=var_0.mean(), var_1=var_1.mean(),
                bpd=(loss_recon.mean() + klz.mean() + loss_diff.mean()) * r,
                aux=dict(logits=logits, emb=emb, z_t=z_t, net=net, g_t=g_t, g_p=g_p))
