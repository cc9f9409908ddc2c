#!/usr/bin/env python3
"""dev: SHA-256 of what every way of running a trained model computes -- the ancestral sampler, the few-step samplers
(plain, stochastic, inpainting and restoring, with and without resampling), one probability-flow ODE function evaluation
and decoding, eager and as replayed HIP graphs -- for each model flavour at B = 2, E = 128, one layer, fixed seeds and
random weights.  It calls public names of mulan_amd.model only, so the same
file runs before and after a change of the host code that drives these kernels: record both and compare the two files
(see profiles/README.md); equal digests mean equal bits.
    python tools/sampler_paths_digest.py --out digests.log
A replayed form prints the class that ran it, so a capture that fell back to the eager form shows in the file."""
import argparse
import dataclasses
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch

from mulan_amd import lib, ops, sampling
from mulan_amd import model as M
from mulan_amd.rng import PRNGKey

B, E = 2, 128
# (name, vdm_type, config fields): the five flavours the samplers tell apart, then the two MuLAN forms that take another
# branch of the step (the integer conditioning cast inside it; gamma per pixel into the ldm U-Net)
CONFIGS = [
    ("mulan_velocity", "mulan_velocity", dict(velocity_from_epsilon=False)),
    ("mulan_velocity velocity_from_epsilon", "mulan_velocity", dict(velocity_from_epsilon=True)),
    ("mulan_epsilon", "mulan_epsilon", {}),
    ("vdm reparam_type=noise", "vdm", dict(gamma_type='fixed', z_conditioning=False, reparam_type='noise')),
    ("vdm reparam_type=input", "vdm", dict(gamma_type='fixed', z_conditioning=False, reparam_type='input')),
    ("mulan_epsilon z_conditioning=False", "mulan_epsilon", dict(z_conditioning=False)),
    ("mulan_epsilon unet_type=ldm", "mulan_epsilon", dict(unet_type='ldm')),
]
LINES = []


def _config(**fields):
    base = dict(vocab_size=256, sample_softmax=False, antithetic_time_sampling=True, with_fourier_features=True,
                with_attention=False, gamma_type='poly_fixedend', gamma_min=-13.3, gamma_max=5.0, sm_n_timesteps=0,
                sm_n_embd=E, sm_n_layer=1, sm_pdrop=0.1, forward_n_layer=1, latent_size=50, latent_k=15, encoder='unet',
                latent_type='topk', z_conditioning=True, reparam_type='true', unet_type='vdm', condition='input')
    return M.VDMConfig(**dict(base, **fields))


def _params(model, seed):
    """the model's tree with every leaf drawn N(0, 0.03^2): zero-initialised layers would make the network output trivial"""
    gen = torch.Generator().manual_seed(seed)
    return M.tree_map(lambda t: (torch.randn(t.shape, generator=gen) * 0.03).cuda(), model.init(PRNGKey(0)))


def _digest(what, *tensors, by=""):
    torch.cuda.synchronize()
    h = hashlib.sha256()
    for t in tensors:
        h.update(t.detach().contiguous().cpu().numpy().tobytes())
    finite = all(bool(torch.isfinite(t.float()).all()) for t in tensors)
    LINES.append(f"{what}{' [' + by + ']' if by else ''}: {h.hexdigest()}{'' if finite else ' (not finite)'}")


def _paths(name, vdm_type, fields):
    LINES.append("# " + name)
    dev = torch.device("cuda")
    cfg = _config(**fields)
    model = M.make_vdm(vdm_type, cfg)
    params = _params(model, 7)
    mulan = vdm_type != "vdm"
    key = PRNGKey(11)
    cond = torch.zeros(B, dtype=torch.uint8, device=dev)
    z1 = key.normal((B, 3072), dev)
    T = 3
    with torch.no_grad():
        emb = model.deterministic_embedding(B, dev) if mulan else None
        coeffs = model.sample_coefficients(params, emb)
        z = z1.clone()
        for i in range(T):
            z = model.conditional_sample(params, i, T, z, emb, cond, key, coeffs) if mulan \
                else model.sample(params, i, T, z, cond, key, coeffs)
        _digest("ancestral, 3 steps, eager", z)
        if mulan:
            step = model.reverse_stepper(params, B, dev, emb, cond, coeffs, T, graph=True)
            z = z1.clone()
            for i in range(T):
                z = step(i, z, key).clone()
            _digest("ancestral, 3 steps, replayed", z, by=type(getattr(step, "__self__", step)).__name__)
        ctx = model.fast_context(params, emb, cond)
        for sampler in ("dpm2m", "ddim"):
            for graph in (False, True):
                stepper = model.fast_stepper(params, B, dev, ctx, graph=graph)
                z = model.fast_sample(params, z1.clone(), ctx, sampler, 4, stepper=stepper)
                _digest(f"{sampler}, 4 steps, {'replayed' if graph else 'eager'}", z, by=type(stepper).__name__)
        # the guided and the stochastic runs: a half:left mask and an sr:2+gray measurement of one seeded image
        image = torch.randint(0, 256, (B, 32, 32, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(17)).cuda()
        masked = dict(known=ops.encode_u8(image).reshape(B, 3072), known_noise=PRNGKey(19),
                      mask=sampling.expand_mask(sampling.mask_from_spec("half:left"), B, dev))
        measured = dict(measurement=ops.restore_measure(ops.encode_u8(image), 2, True), degradation="sr:2+gray",
                        known_noise=PRNGKey(19))
        runs = [("sde2m", 0.0, "", {}), ("ddim", 0.5, " eta = 0.5", {})]
        runs += [(sm, 0.0, f" under half:left, resample {U}", dict(masked, resample=U))
                 for sm, U in (("dpm2m", 1), ("dpm2m", 2), ("sde2m", 2))]
        runs += [(sm, 0.0, f" under sr:2+gray, resample {U}", dict(measured, resample=U))
                 for sm in ("dpm2m", "sde2m") for U in (1, 2)]
        for sampler, eta, what, kw in runs:
            step_eta = sampling.check_eta(sampler, eta)
            for graph in (False, True):
                stepper = model.fast_stepper(params, B, dev, ctx, graph=graph, step_eta=step_eta, inpaint="mask" in kw,
                                             restore=kw.get("degradation"))
                z = model.fast_sample(params, z1.clone(), ctx, sampler, 4, stepper=stepper, eta=eta,
                                      noise=PRNGKey(18) if step_eta > 0.0 else None, **kw)
                _digest(f"{sampler}{what}, 4 steps, {'replayed' if graph else 'eager'}", z, by=type(stepper).__name__)
        z0 = PRNGKey(13).normal((B, 3072), dev)
        _digest("generate_x, argmax", model.generate_x(params, z0, coeffs))
        softmax = M.make_vdm(vdm_type, dataclasses.replace(cfg, sample_softmax=True))
        _digest("generate_x, sample_softmax", softmax.generate_x(params, z0, coeffs, rng=PRNGKey(14)))
    if not cfg.z_conditioning and mulan:
        return                                   # (reverse_ode hands the embedding to the score model)
    gen = torch.Generator().manual_seed(5)
    images = torch.randint(0, 256, (B, 32, 32, 3), dtype=torch.uint8, generator=gen).cuda()
    octx = model.ode_context(params, images)
    x = PRNGKey(12).normal((B, 3072), dev)
    probe = ops.noise((B, 3072), 2, 0, dev, "rademacher")
    _digest("reverse_ode, t = 0.4, drift and divergence", *model.reverse_ode(params, x, octx, 0.4, probe))
    if mulan:
        _digest("reverse_ode, t = 0.4, high_precision",
                *model.reverse_ode(params, x, octx, 0.4, probe, high_precision=True))
        for hp in (False, True):
            f = M.ode_function(model, params, octx, B, dev, True, graph=True, high_precision=hp)
            drift, div = torch.empty_like(x), torch.empty(B, device=dev, dtype=x.dtype)
            f(0.4, x, probe, drift, div)
            _digest(f"ode_function, t = 0.4, replayed{', high_precision' if hp else ''}", drift, div, by=type(f).__name__)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    a = ap.parse_args()
    torch.cuda.set_device(0)
    lib.load()
    for cfg in CONFIGS:
        _paths(*cfg)
    with open(a.out, "w") as fh:
        fh.write("\n".join(LINES) + "\n")
    print("\n".join(LINES))


if __name__ == "__main__":
    main()
