"""The residual |A encode(restored) - y| (grey levels) of restoration on the tiny test model of tests/test_gpu_fast_sampler.py
(random weights, B = 2, N = 25): `sr:4`, `gray`, `sr:4+gray` under dpm2m and under sde2m at resample 1 and 2, the device's
run beside the float64 oracle loop (tests/restore_oracle.py) on the same inputs and noise, each decoded by generate_x; and
|A z_0 - y| x 127.5 before decoding (the table of DESIGN §3.7, profiles/restore_residuals.log).

    python tools/restore_residuals.py            (from the repository root)
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from tests import restore_oracle as ro
from tests.oracle_dev import run_oracle
from tests.test_gpu_fast_sampler import _ctx, _setup
from mulan_amd import ops
from mulan_amd.rng import PRNGKey
B, N = 2, 25
vdm, params, ref_params, ocfg = _setup("mulan_velocity", "vdm", False)
ctx = _ctx(vdm, params, B)
xu = torch.tensor(np.random.default_rng(2).integers(0, 256, (B, 32, 32, 3)).astype(np.uint8)).cuda()
z1 = PRNGKey(21).normal((B, 3072), "cuda")
grid = [1.0 - k / N for k in range(N + 1)]
d = lambda t: t.cpu().double()
def resid(z0, y, f, gray):
    img = vdm.generate_x(params, z0, ctx.get("coeffs")).reshape(B, 32, 32, 3)
    lat = (ops.restore_measure(z0.reshape(B, 32, 32, 3).contiguous(), f, gray) - y).abs().amax().item() * 127.5
    return (ops.restore_measure(ops.encode_u8(img), f, gray) - y).abs().reshape(B, -1).amax(1).cpu().numpy() * 127.5, lat
with torch.no_grad():
    for spec in ("sr:4", "gray", "sr:4+gray"):
        f, gray = ro.SPECS[spec]
        y = ops.restore_measure(ops.encode_u8(xu), f, gray)
        for sampler, eta, U in (("dpm2m", 0.0, 1), ("sde2m", 1.0, 1), ("sde2m", 1.0, 2)):
            sx = [ops.randn((B, 3072), PRNGKey(22).fold_in(k).v, 0, "cuda") for k in range(U * N)]
            kx = [ops.randn((B, 3072), PRNGKey(23).fold_in(j).v, 0, "cuda") for j in range(U * N)]
            z0 = vdm.fast_sample(params, z1, ctx, sampler, N, noise=(lambda k: sx[k]) if eta else None, measurement=y,
                                 degradation=spec, resample=U, known_noise=(lambda j: kx[j]) if U > 1 else None)
            z_ref, _ = run_oracle(lambda P, z_, y_, s_, k_: ro.mulan_loop(P, ocfg, z_, grid, sampler, eta, y_, f, gray,
                                  lambda k: s_[k], lambda j: k_[j], U), ref_params, d(z1), d(y), [d(t) for t in sx], [d(t) for t in kx])
            r_hip, l_hip = resid(z0, y, f, gray)
            r_ref, l_ref = resid(z_ref.reshape(B, -1).float().cuda(), y, f, gray)
            print(f"RESID {spec} {sampler} U={U}: hip {r_hip.max():.3f} oracle {r_ref.max():.3f} grey levels; "
                  f"|A z0 - y| before decoding: hip {l_hip:.3f} oracle {l_ref:.3f}; |z0 - z0_ref| {float((z0.cpu().double() - z_ref.reshape(B, -1)).abs().max()):.3g}", flush=True)
