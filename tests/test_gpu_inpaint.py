"""Inpainting with the few-step samplers (mulan_amd.sampling.run): the two HIP kernels against float64
(tests/inpaint_oracle.py), their exact cases, ragged sizes and refusals, the law of the jump and of the whole loop on a
linear-Gaussian model, the whole models against the float64 oracle loop on shared noise, the replayed stepper against the
eager one, the notebook front end and the `python -m ldm.sample` CLI."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import inpaint_oracle as io
from tests import stochastic_sampler_oracle as so
from tests.oracle_dev import run_oracle
from tests.test_gpu_fast_sampler import KINDS, ROOT, _config, _ctx, _experiment, _inputs, _randomise_ema, _rel, _setup

BAR = 2e-6                  # the bar of test_stochastic_sampler_step_kernel for this fp32 elementwise chain


def _dev(a):
    return torch.tensor(a).cuda()


def _d(t):
    return t.cpu().double()


def _mix_inputs(seed, B, per_sample, density):
    z, xi, g, _, _, _ = _inputs(seed, B, per_sample)
    rng = np.random.default_rng(100 + seed)
    x = rng.uniform(-1.0, 1.0, (B, 3072)).astype(np.float32)
    mask = (rng.random((B, 3072)) < density).astype(np.uint8)
    return z, x, mask, g, xi


# ---------------------------------------------------------------------------------- 1. the mix against float64
@pytest.mark.parametrize("per_sample", [False, True])
@pytest.mark.parametrize("density", [0.0, 0.5, 1.0])
def test_mix_kernel(per_sample, density):
    from mulan_amd import ops
    B = 5
    z, x, mask, g, xi = _mix_inputs(3, B, per_sample, density)
    known = mask != 0
    x_bad, xi_bad = x.copy(), xi.copy()
    x_bad[~known], xi_bad[~known] = np.nan, np.nan              # what the unknown positions hold never reaches out
    gd = (lambda a: torch.tensor(a, dtype=torch.float64)[:, None]) if per_sample else (lambda a: torch.tensor(a).double())
    ref = io.mix(torch.tensor(z).double(), torch.tensor(x).double(), torch.tensor(mask), gd(g), torch.tensor(xi).double())
    zd = _dev(z)
    out = ops.inpaint_mix(zd, _dev(x_bad), _dev(mask), _dev(g), _dev(xi_bad))
    inplace = zd.clone()
    assert ops.inpaint_mix(inplace, _dev(x_bad), _dev(mask), _dev(g), _dev(xi_bad), out=inplace) is inplace
    boolean = ops.inpaint_mix(zd, _dev(x_bad), _dev(mask).bool(), _dev(g), _dev(xi_bad))
    assert out.shape == zd.shape and out.data_ptr() != zd.data_ptr() and torch.equal(zd, _dev(z))
    assert torch.equal(out, inplace) and torch.equal(out, boolean)
    assert bool(torch.isfinite(out).all())
    kd = _dev(known)
    assert torch.equal(out[~kd], zd[~kd])
    if known.any():
        e = _rel(out.cpu().numpy()[known], ref.numpy()[known])
        print(f"per_sample {per_sample} density {density}: known {e:.3g}")
        assert e < BAR
        # zero noise: the same bits from a NULL xi and from a buffer of zeros (the product itself:
        # test_mix_at_zero_noise_is_the_product_alpha_x)
        none = ops.inpaint_mix(zd, _dev(x_bad), _dev(mask), _dev(g))
        zero = ops.inpaint_mix(zd, _dev(x_bad), _dev(mask), _dev(g), torch.zeros_like(zd))
        assert torch.equal(none, zero)
        a64 = torch.sqrt(torch.sigmoid(-gd(g))) * torch.tensor(x).double()
        assert _rel(none.cpu().numpy()[known], (a64 * torch.ones(B, 3072).double()).numpy()[known]) < BAR


def test_mix_at_zero_noise_is_the_product_alpha_x():
    """alpha is one fp32 value per element whatever the noise: out / x recovers it, and sigma xi is added to that
    product by one fused operation: with xi = 0 the product alone is left"""
    from mulan_amd import ops
    z, x, mask, g, xi = _mix_inputs(4, 2, False, 1.0)
    none = ops.inpaint_mix(_dev(z), _dev(x), _dev(mask), _dev(g))
    ones = ops.inpaint_mix(_dev(z), torch.ones_like(_dev(x)), _dev(mask), _dev(g))          # alpha itself
    assert torch.equal(none, ones * _dev(x))


# ---------------------------------------------------------------------------------- 2. the mix ties to qsample
def test_mix_ties_to_qsample():
    """uint8 images, everything known, the same eps, gamma_t per element: ops.qsample's z_t = alpha_t f(x) + sigma_t eps
    within twice the kernel bar, since each side carries that rounding against float64"""
    from mulan_amd import ops
    B = 5
    rng = np.random.default_rng(8)
    xu = _dev(rng.integers(0, 256, (B, 3072)).astype(np.uint8))
    gt = _dev(rng.uniform(-13.3, 5.0, (B, 3072)).astype(np.float32))
    g0, g1 = torch.full_like(gt, -13.3), torch.full_like(gt, 5.0)
    eps0, eps = (_dev(rng.standard_normal((B, 3072)).astype(np.float32)) for _ in range(2))
    zt = ops.qsample(xu, g0, g1, gt, eps0, eps)[0]
    out = ops.inpaint_mix(torch.zeros_like(zt), ops.encode_u8(xu), torch.ones_like(xu), gt, eps)
    e = _rel(out.cpu().numpy(), zt.cpu().numpy())
    print(f"qsample tie {e:.3g}")
    assert e < 2 * BAR


# ---------------------------------------------------------------------------------- 3. the jump against float64
@pytest.mark.parametrize("per_sample", [False, True])
def test_jump_kernel(per_sample):
    from mulan_amd import ops
    B = 5
    zs, xi, gt, gs, _, _ = _inputs(5, B, per_sample)                     # g_s < g_t
    gd = (lambda a: torch.tensor(a, dtype=torch.float64)[:, None]) if per_sample else (lambda a: torch.tensor(a).double())
    ref = io.jump(torch.tensor(zs).double(), gd(gs), gd(gt), torch.tensor(xi).double())
    out = ops.forward_jump(_dev(zs), _dev(gs), _dev(gt), _dev(xi))
    e = _rel(out.cpu().numpy(), ref.numpy())
    print(f"per_sample {per_sample}: jump {e:.3g}")
    assert out.shape == (B, 3072) and e < BAR
    # equal gammas: z_s bit for bit; a gamma_t one ulp and a little above gamma_s: finite, and close to z_s
    assert torch.equal(ops.forward_jump(_dev(zs), _dev(gs), _dev(gs), _dev(xi)), _dev(zs))
    zz = zs.copy()
    zz[:, ::5], zz[:, 1::5] = -0.0, 0.0                        # the sign of a zero too, whatever the sign of xi
    same = ops.forward_jump(_dev(zz), _dev(gs), _dev(gs), _dev(xi))
    assert torch.equal(same.view(torch.int32), _dev(zz).view(torch.int32))
    for up in (np.nextafter(gs, np.float32(np.inf)), (gs + np.float32(1e-6)).astype(np.float32),
               (gs + np.float32(1e-3)).astype(np.float32)):
        near = ops.forward_jump(_dev(zs), _dev(gs), _dev(up), _dev(xi))
        ref = io.jump(torch.tensor(zs).double(), gd(gs), gd(up), torch.tensor(xi).double())
        assert bool(torch.isfinite(near).all())
        assert _rel(near.cpu().numpy(), ref.numpy()) < BAR


# ---------------------------------------------------------------------------------- 4. ragged and unaligned
def test_ragged_and_unaligned():
    """n = 4099 with every buffer one element off the 16-byte grid and the mask one byte off a 4-byte boundary: the
    scalar path, 17 blocks, the last one partial"""
    from mulan_amd import ops
    n = 4099
    rng = np.random.default_rng(5)
    z, x, xi = (_dev(rng.standard_normal(n + 1).astype(np.float32))[1:] for _ in range(3))
    g_h = rng.uniform(-13.3, 5.0, n + 1).astype(np.float32)
    g, g_up = _dev(g_h)[1:], _dev(g_h + 0.3)[1:]
    mask = _dev((rng.random(n + 1) < 0.5).astype(np.uint8))[1:]
    assert all(t.data_ptr() % 16 == 4 for t in (z, x, xi, g, g_up)) and mask.data_ptr() % 4 == 1
    out = ops.inpaint_mix(z, x, mask, g, xi)
    ref = io.mix(_d(z), _d(x), mask.cpu(), _d(g), _d(xi))
    k = mask.cpu().numpy() != 0
    assert out.shape == (n,) and torch.equal(out[~_dev(k)], z[~_dev(k)])
    assert _rel(out.cpu().numpy()[k], ref.numpy()[k]) < BAR
    zt = ops.forward_jump(z, g, g_up, xi)
    assert zt.shape == (n,) and _rel(zt.cpu().numpy(), io.jump(_d(z), _d(g), _d(g_up), _d(xi)).numpy()) < BAR
    # per-sample gamma on the scalar path: one gamma for all 4099 elements, and 7 rows of 585 (odd, so no float4)
    for rows in (1, 7):
        m = rows * (n // rows)
        shp = (rows, m // rows)
        gr_h = rng.uniform(-13.3, 5.0, rows + 1).astype(np.float32)
        gr, gr_up = _dev(gr_h)[1:], _dev(gr_h + 0.3)[1:]
        zr, xr, xir, mr = (t[:m].view(shp) for t in (z, x, xi, mask))
        assert zr.data_ptr() % 16 == 4 and m % 4 != 0
        out = ops.inpaint_mix(zr, xr, mr, gr, xir)
        ref = io.mix(_d(zr), _d(xr), mr.cpu(), _d(gr)[:, None], _d(xir))
        kr = mr.cpu().numpy() != 0
        assert out.shape == shp and torch.equal(out[mr == 0], zr[mr == 0])
        assert _rel(out.cpu().numpy()[kr], ref.numpy()[kr]) < BAR
        zt = ops.forward_jump(zr, gr, gr_up, xir)
        assert _rel(zt.cpu().numpy(), io.jump(_d(zr), _d(gr)[:, None], _d(gr_up)[:, None], _d(xir)).numpy()) < BAR
    # a mask off its 4-byte boundary alone (everything else aligned, n % 4 == 0) takes the scalar path too
    n4 = 4096
    z4, x4, xi4, g4 = (_dev(rng.standard_normal(n4).astype(np.float32)) for _ in range(4))
    m4 = _dev((rng.random(n4 + 1) < 0.5).astype(np.uint8))
    assert torch.equal(ops.inpaint_mix(z4, x4, m4[1:], g4, xi4), ops.inpaint_mix(z4, x4, m4[1:].clone(), g4, xi4))


@pytest.mark.parametrize("per_sample", [False, True])
def test_float4_path_with_an_almost_empty_last_block(per_sample):
    """n = 4 * 256 * 3 + 4: 769 float4s, four blocks of which the last holds one thread's work"""
    from mulan_amd import ops
    n, rows = 4 * 256 * 3 + 4, 769                               # n = 769 * 4: per sample, every float4 has its gamma
    rng = np.random.default_rng(9)
    z, x, xi = (_dev(rng.standard_normal(n).astype(np.float32)) for _ in range(3))
    mask = _dev((rng.random(n) < 0.5).astype(np.uint8))
    g_h = rng.uniform(-13.3, 5.0, rows if per_sample else n).astype(np.float32)
    g, g_up = _dev(g_h), _dev(g_h + 0.3)
    if per_sample:
        z, x, xi, mask = (t.view(rows, -1) for t in (z, x, xi, mask))
    gd = (lambda t: _d(t)[:, None]) if per_sample else _d
    out = ops.inpaint_mix(z, x, mask, g, xi)
    ref = io.mix(_d(z), _d(x), mask.cpu(), gd(g), _d(xi))
    k = mask.cpu().numpy() != 0
    assert out.numel() == n and torch.equal(out[mask == 0], z[mask == 0])
    assert _rel(out.cpu().numpy()[k], ref.numpy()[k]) < BAR
    zt = ops.forward_jump(z, g, g_up, xi)
    assert zt.numel() == n and _rel(zt.cpu().numpy(), io.jump(_d(z), gd(g), gd(g_up), _d(xi)).numpy()) < BAR


# ---------------------------------------------------------------------------------- 5. refusals
def test_entry_points_refuse_bad_arguments():
    """n = 0, a NULL required pointer, a negative or non-dividing g_per_sample: hipErrorInvalidValue (1), before any
    launch; a NULL xi of the mix is the zero noise"""
    from mulan_amd import lib
    h = lib.load()
    buf = torch.randn(8, 16, device="cuda")
    mask = torch.ones(16, dtype=torch.uint8, device="cuda")
    p = lambda i: buf[i].data_ptr()

    def rc(fn, good, **kw):
        a = list(good)
        for k, v in kw.items():
            a[int(k[1:])] = v
        return fn(*a)
    mix = [p(0), p(1), mask.data_ptr(), p(2), p(3), p(4), 16, 0, None]
    assert rc(h.mulan_inpaint_mix, mix) == 0 and rc(h.mulan_inpaint_mix, mix, a7=4) == 0
    for i in (0, 1, 2, 3, 5):                                                # z, x, mask, g, out
        assert rc(h.mulan_inpaint_mix, mix, **{f"a{i}": None}) == 1, i
    assert rc(h.mulan_inpaint_mix, mix, a6=0) == 1
    assert rc(h.mulan_inpaint_mix, mix, a7=-1) == 1 and rc(h.mulan_inpaint_mix, mix, a7=5) == 1
    zero = torch.zeros(16, device="cuda")
    assert rc(h.mulan_inpaint_mix, mix, a4=zero.data_ptr(), a5=p(5)) == 0 and rc(h.mulan_inpaint_mix, mix, a4=None, a5=p(6)) == 0
    torch.cuda.synchronize()
    assert torch.equal(buf[5], buf[6])
    jump = [p(0), p(1), p(2), p(3), p(7), 16, 0, None]
    assert rc(h.mulan_forward_jump, jump) == 0 and rc(h.mulan_forward_jump, jump, a6=8) == 0
    for i in (0, 1, 2, 3, 4):                                                # zs, gs, gt, xi, zt
        assert rc(h.mulan_forward_jump, jump, **{f"a{i}": None}) == 1, i
    assert rc(h.mulan_forward_jump, jump, a5=0) == 1
    assert rc(h.mulan_forward_jump, jump, a6=-1) == 1 and rc(h.mulan_forward_jump, jump, a6=5) == 1
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------- 6. the law of the jump
def test_law_of_the_jump():
    """x ~ N(mu, sd^2) per coordinate, z_s drawn from q_s, one jump to t on independent noise: the jump maps the marginal
    q_s onto q_t exactly, so z_t ~ N(alpha_t mu, alpha_t^2 sd^2 + sigma_t^2).  Over n = 64 x 3072 coordinates the mean
    and the variance are held to five standard errors, as test_law_on_a_linear_gaussian_model holds them"""
    from mulan_amd import ops
    from mulan_amd.rng import PRNGKey
    B, mu, sd, gmin, gmax = 64, 0.3, 0.5, -13.3, 5.0
    n = B * 3072
    for i, (ts, tt) in enumerate(((0.25, 0.3125), (0.0, 1.0), (0.5, 0.9))):
        k_x, k_e, k_j = PRNGKey(41).fold_in(i).split(3)
        g_s = np.float32(gmin + (gmax - gmin) * ts)
        g_t = np.float32(gmin + (gmax - gmin) * tt)
        gs, gt = torch.full((B,), float(g_s), device="cuda"), torch.full((B,), float(g_t), device="cuda")
        x = mu + sd * ops.randn((B, 3072), k_x.v, 0, "cuda")
        z_s = ops.inpaint_mix(torch.zeros_like(x), x, torch.ones((B, 3072), dtype=torch.uint8, device="cuda"), gs,
                              ops.randn((B, 3072), k_e.v, 0, "cuda"))
        z_t = ops.forward_jump(z_s, gs, gt, ops.randn((B, 3072), k_j.v, 0, "cuda")).double()
        al2 = 1.0 / (1.0 + np.exp(np.float64(g_t)))
        m, v = np.sqrt(al2) * mu, al2 * sd ** 2 + (1 - al2)
        em, ev = float(z_t.mean()), float(z_t.var(unbiased=True))
        print(f"jump {ts} -> {tt}: mean {em:.6f} (law {m:.6f}, 5 se {5 * np.sqrt(v / n):.2g}), variance {ev:.6f} "
              f"(law {v:.6f}, 5 se {5 * v * np.sqrt(2 / n):.2g})")
        assert abs(em - m) < 5 * np.sqrt(v / n)
        assert abs(ev - v) < 5 * v * np.sqrt(2 / n)


# ---------------------------------------------------------------------------------- 7. the law of inpainting
@pytest.mark.parametrize("mode", [1, 2])
@pytest.mark.parametrize("resample", [1, 2])
def test_law_of_inpainting_on_a_linear_gaussian_model(mode, resample):
    """the model of test_law_on_a_linear_gaussian_model (independent coordinates x ~ N(mu, sd^2), the exact posterior
    mean as network, ddim with eta = 1, N = 16) under a checkerboard mask: the known coordinates of z_0 are alpha_0 x bit
    for bit; an unknown coordinate never sees a known one and every operation on it is affine, so it is Gaussian with
    the mean and variance inpaint_gaussian_law propagates in float64; both are held to five standard errors over the
    n = 64 x 1536 unknown coordinates"""
    from mulan_amd import ops, sampling
    from mulan_amd.rng import PRNGKey
    B, N, mu, sd, gmin, gmax, eta = 64, 16, 0.3, 0.5, -13.3, 5.0, 1.0
    k_z, k_s, k_k, k_x = PRNGKey(33).fold_in(10 * mode + resample).split(4)
    z1 = k_z.normal((B, 3072), "cuda")
    x = mu + sd * k_x.normal((B, 3072), "cuda")
    yy, xx = np.meshgrid(np.arange(32), np.arange(32), indexing="ij")
    mask = sampling.expand_mask((yy + xx) % 2 == 0, B, "cuda")
    known = mask != 0
    gamma32 = lambda t: float(np.float32(gmin + (gmax - gmin) * np.float64(np.float32(t))))

    def gamma_fn(t):
        return torch.full((B,), gamma32(t), device="cuda")

    def net_fn(z, t):
        g = gamma_fn(t).double()[:, None]
        xh = so.posterior_mean(z.double(), g, mu, sd)
        al, si = torch.sqrt(torch.sigmoid(-g)), torch.sqrt(torch.sigmoid(g))
        return ((z.double() - al * xh) / si if mode == 1 else xh).float()

    noise_fn = lambda k: ops.randn((B, 3072), k_s.fold_in(k).v, 0, "cuda")
    known_fn = lambda j: ops.randn((B, 3072), k_k.fold_in(j).v, 0, "cuda")
    z0 = sampling.sample(net_fn, gamma_fn, z1, mode, "ddim", steps=N, eta=eta, noise_fn=noise_fn, known=x, mask=mask,
                         known_noise_fn=known_fn, resample=resample)
    a0 = torch.sqrt(torch.sigmoid(-gamma_fn(0.0)))[:, None]
    assert torch.equal(z0[known], ops.inpaint_mix(z0, x, mask, gamma_fn(0.0))[known])
    assert _rel(z0[known].cpu().numpy(), (a0.double() * x.double())[known].cpu().numpy()) < BAR
    u = z0[~known].double()
    n = u.numel()
    assert n == B * 1536
    grid = sampling.time_grid(N)
    m, v = io.inpaint_gaussian_law([gamma32(sampling.f32(t)) for t in grid], mu, sd, eta, resample)
    em, ev = float(u.mean()), float(u.var(unbiased=True))
    print(f"mode {mode} resample {resample}: mean {em:.6f} (law {m:.6f}, 5 se {5 * np.sqrt(v / n):.2g}), "
          f"variance {ev:.6f} (law {v:.6f}, 5 se {5 * v * np.sqrt(2 / n):.2g})")
    assert abs(em - m) < 5 * np.sqrt(v / n)
    assert abs(ev - v) < 5 * v * np.sqrt(2 / n)


def test_sample_without_a_mask_is_the_sampler_of_before():
    """sampling.sample through the new signature, nothing known: the bits of run(EagerStepper(...)) built the old way"""
    from mulan_amd import ops, sampling
    from mulan_amd.rng import PRNGKey
    B = 2
    z1 = PRNGKey(3).normal((B, 3072), "cuda")
    k_s = PRNGKey(4)
    gamma_fn = lambda t: torch.full((B,), float(np.float32(-13.3 + 18.3 * t)), device="cuda")
    net_fn = lambda z, t: 0.3 * z
    noise_fn = lambda k: ops.randn((B, 3072), k_s.fold_in(k).v, 0, "cuda")
    for sampler, eta, N in (("dpm2m", 0.0, 5), ("sde2m", 0.0, 5), ("ddim", 0.5, 4)):
        step_eta = sampling.check_eta(sampler, eta)
        new = sampling.sample(net_fn, gamma_fn, z1, 1, sampler, steps=N, eta=eta, noise_fn=noise_fn, known=None, mask=None,
                              known_noise_fn=None, resample=1)
        grid, orders = sampling.time_grid(N), sampling.step_orders(sampler, N)
        z = z1
        stepper = sampling.EagerStepper(net_fn, gamma_fn, 1, step_eta, noise_fn)
        for k, order in enumerate(orders):
            z = stepper(z, grid[k], grid[k + 1], order, k)
        assert torch.equal(new, z) and torch.equal(new, sampling.run(sampling.EagerStepper(
            net_fn, gamma_fn, 1, step_eta, noise_fn), z1, grid, orders))


# ---------------------------------------------------------------------------------- 8. whole models, pathwise
MODELS = [("mulan_velocity", "vdm", False), ("mulan_epsilon", "ldm", False), ("plain", "vdm", False)]


@pytest.mark.parametrize("vdm_type,unet_type,vfe", MODELS)
def test_inpainting_matches_the_oracle_loop(vdm_type, unet_type, vfe):
    """dpm2m with resample 1 (four network evaluations, one eps for the known region) and sde2m with resample 2 (seven:
    the three repeated steps count) over N = 4 steps, the same noise on both sides: every operation of the oracle's
    loop from the oracle's input against the oracle's output.  A step (with the mix behind it) has the budget of
    test_stochastic_samplers_match_the_oracle for one network evaluation: 2e-4 of max |net| x the step's d z_s / d net,
    1e-5 of the result, and the kernel bar of the step's noise term; the known sub-pixels, the first mix and the jumps
    carry no network error and are held to the 1e-5 of the result alone (the fp32 schedule and the elementwise chain)"""
    from mulan_amd import ops
    from mulan_amd.rng import PRNGKey
    B, N = 2, 4
    rng = np.random.default_rng(2)
    z_init = PRNGKey(21).fold_in(1000).normal((B, 3072), "cuda")
    xu = _dev(rng.integers(0, 256, (B, 3072)).astype(np.uint8))
    x = ops.encode_u8(xu)
    mask = _dev((rng.random((B, 32, 32, 1)) < 0.5).repeat(3, axis=3).reshape(B, 3072).astype(np.uint8))
    k_s, k_k = PRNGKey(22), PRNGKey(23)
    f32 = lambda t: torch.full((B,), float(np.float32(t)), device="cuda")
    vdm, params, ref_params, ocfg = _setup(vdm_type, unet_type, vfe)
    ctx = _ctx(vdm, params, B)
    loop = io.plain_loop if vdm_type == "plain" else io.mulan_loop
    grid = [1.0 - k / N for k in range(N + 1)]
    for sampler, eta, U in (("dpm2m", 0.0, 1), ("sde2m", 1.0, 2)):
        sx = [ops.randn((B, 3072), k_s.fold_in(k).v, 0, "cuda") for k in range(U * N)]
        kx = [ops.randn((B, 3072), k_k.fold_in(j).v, 0, "cuda") for j in range(2 * U * N)]
        z_ref, events = run_oracle(
            lambda P, z_, x_, m_, s_, k_: loop(P, ocfg, z_, grid, sampler, eta, x_, m_, lambda k: s_[k], lambda j: k_[j], U),
            ref_params, _d(z_init), _d(x), mask.cpu(), [_d(t) for t in sx], [_d(t) for t in kx])
        steps = [e for e in events if e["kind"] == "step"]
        assert len(steps) == (N if U == 1 else 2 * N - 1) and sum(e["kind"] == "jump" for e in events) == (U - 1) * (N - 1)
        flat = lambda t: t.reshape(B, -1).float().cuda()
        with torch.no_grad():
            for e in events:
                want = e["z_out"].reshape(B, -1).numpy()
                scale = 1e-5 * float(np.abs(want).max())
                if e["kind"] == "mix":
                    got = ops.inpaint_mix(flat(e["z_in"]), x, mask, vdm._fast_gamma(params, ctx, f32(e["t"])), kx[e["j"]])
                    allowed = scale
                elif e["kind"] == "jump":
                    got = ops.forward_jump(flat(e["z_in"]), vdm._fast_gamma(params, ctx, f32(e["s"])),
                                           vdm._fast_gamma(params, ctx, f32(e["t"])), kx[e["j"]])
                    allowed = scale
                else:
                    if e["order"] == 2:
                        g_p, x_p = vdm._fast_gamma(params, ctx, f32(grid[e["k"] - 1])), flat(e["x_p"])
                    else:
                        g_p = x_p = None
                    got, _, _ = vdm._fast_step(params, flat(e["z_in"]), f32(e["t"]), f32(e["s"]), g_p, x_p, ctx,
                                               sx[e["kk"]] if eta > 0 else None, eta, x, mask,
                                               None if e["j"] is None else kx[e["j"]])
                    allowed = 2e-4 * e["budget"] + scale + BAR * e["noise"]
                    kn = (mask != 0).cpu().numpy()
                    ek = np.abs(got.cpu().double().numpy() - want)[kn].max()
                    assert ek < scale, (sampler, e["k"], e["kk"], ek, scale)
                err = np.abs(got.cpu().double().numpy() - want).max()
                print(f"{vdm_type} {sampler} x{U} {e['kind']} {e.get('kk', '')}: err {err:.3g} allowed {allowed:.3g}")
                assert err < allowed, (sampler, e["kind"], e.get("kk"), err, allowed)
        # the known sub-pixels of z_0 are alpha_0 x, and decode to the input's integers
        z0 = z_ref.reshape(B, -1).float().cuda()
        dec = vdm.generate_x(params, z0, ctx.get("coeffs")).reshape(B, 3072)
        assert torch.equal(dec[mask != 0], xu[mask != 0])


@pytest.mark.parametrize("vdm_type,unet_type,vfe", MODELS)
def test_inpainting_runs_match_the_oracle_loop(vdm_type, unet_type, vfe):
    """the product's own loop: fast_sample with a mask on the shared noise (callables k -> xi, j -> xi), eager and
    replayed, run free from z_1 against the z_0 of the oracle's loop, for dpm2m at resample 1 (4 network evaluations)
    and sde2m at resample 2 (7).  This holds what sampling.run decides -- which draw goes where, one eps throughout the
    deterministic run, first order and the step index k + r N on a repeated step, the history it leaves -- to the
    oracle's restatement.  On the damped network of test_fast_samplers_match_the_oracle's free run, with its bar taken
    over every network evaluation of the run, the repeated ones included: 4 x (2e-4 of the summed step budgets + the
    kernel bar of the summed step-noise maxima) + 1e-5.  The known sub-pixels of the device's z_0 decode to the input"""
    from mulan_amd import ops
    from mulan_amd.rng import PRNGKey
    B, N = 2, 4
    rng = np.random.default_rng(2)
    z_init = PRNGKey(21).fold_in(1000).normal((B, 3072), "cuda")
    xu = _dev(rng.integers(0, 256, (B, 3072)).astype(np.uint8))
    x = ops.encode_u8(xu)
    mask = _dev((rng.random((B, 32, 32, 1)) < 0.5).repeat(3, axis=3).reshape(B, 3072).astype(np.uint8))
    k_s, k_k = PRNGKey(22), PRNGKey(23)
    vdm, params, ref_params, ocfg = _setup(vdm_type, unet_type, vfe, damp=0.02)
    ctx = _ctx(vdm, params, B)
    loop = io.plain_loop if vdm_type == "plain" else io.mulan_loop
    grid = [1.0 - k / N for k in range(N + 1)]
    for sampler, eta, U in (("dpm2m", 0.0, 1), ("sde2m", 1.0, 2)):
        sx = [ops.randn((B, 3072), k_s.fold_in(k).v, 0, "cuda") for k in range(U * N)]
        kx = [ops.randn((B, 3072), k_k.fold_in(j).v, 0, "cuda") for j in range(2 * U * N)]
        z_ref, events = run_oracle(
            lambda P, z_, x_, m_, s_, k_: loop(P, ocfg, z_, grid, sampler, eta, x_, m_, lambda k: s_[k], lambda j: k_[j], U),
            ref_params, _d(z_init), _d(x), mask.cpu(), [_d(t) for t in sx], [_d(t) for t in kx])
        steps = [e for e in events if e["kind"] == "step"]
        assert len(steps) == N + (U - 1) * (N - 1)
        bar = 4 * (2e-4 * sum(e["budget"] for e in steps) + BAR * sum(e["noise"] for e in steps)) + 1e-5
        kw = dict(noise=(lambda k: sx[k]) if eta > 0 else None, known=x, mask=mask, resample=U, known_noise=lambda j: kx[j])
        za = vdm.fast_sample(params, z_init, ctx, sampler, N, graph=False, **kw)
        zb = vdm.fast_sample(params, z_init, ctx, sampler, N, graph=True, **kw)
        assert torch.equal(za, zb)
        free = np.abs(za.cpu().double().numpy() - z_ref.reshape(B, -1).numpy()).max()
        print(f"{vdm_type} {sampler} x{U}: free-run distance {free:.3g} allowed {bar:.3g} ({len(steps)} evaluations)")
        assert free < bar, (sampler, U, free, bar)
        dec = vdm.generate_x(params, za, ctx.get("coeffs")).reshape(B, 3072)
        assert torch.equal(dec[mask != 0], xu[mask != 0])
        if U == 1:                      # the deterministic run asks for draw 0 alone: what the others hold is never read
            wrong = dict(kw, known_noise=lambda j: kx[j] if j == 0 else kx[5])
            assert torch.equal(vdm.fast_sample(params, z_init, ctx, sampler, N, graph=False, **wrong), za)


# ---------------------------------------------------------------------------------- 9. replay equals eager
@pytest.mark.parametrize("vdm_type,unet_type", [("mulan_velocity", "vdm"), ("plain", "vdm")])
@pytest.mark.parametrize("sampler,resample", [("dpm2m", 1), ("sde2m", 2)])
def test_replayed_inpainting_equals_the_eager_run(vdm_type, unet_type, sampler, resample):
    """model.GraphedFastStep built with a mask (the known image, the mask and the known region's noise static buffers,
    the mix captured behind the step; the first mix and the jumps eager launches) against model.EagerFastStep: the same
    bits over two batches with other images, masks, contexts and keys through one stepper each, and what fresh steppers
    give; the known sub-pixels of z_0 are alpha_0 x; a stepper serves runs with a mask or without, never both"""
    from mulan_amd import ops
    from mulan_amd.rng import PRNGKey
    B, N = 2, 4
    vdm, params, _, _ = _setup(vdm_type, unet_type, False)
    rng = np.random.default_rng(6)
    cond = lambda v: torch.full((B,), v, dtype=torch.uint8, device="cuda")
    if hasattr(vdm, "deterministic_embedding"):
        emb2 = torch.zeros((B, 50), device="cuda"); emb2[:, 20:35] = 1.0
        ctxs = [_ctx(vdm, params, B), vdm.fast_context(params, emb2, cond(0))]
    else:
        ctxs = [_ctx(vdm, params, B), vdm.fast_context(params, None, cond(1))]
    batches = []
    for b in range(2):
        xu = _dev(rng.integers(0, 256, (B, 3072)).astype(np.uint8))
        mask = _dev((rng.random((B, 3072)) < (0.3, 0.7)[b]).astype(np.uint8))
        batches.append(dict(z=PRNGKey(11 + b).normal((B, 3072), "cuda"), ctx=ctxs[b], xu=xu,
                            kw=dict(known=ops.encode_u8(xu), mask=mask, resample=resample, known_noise=PRNGKey(40 + b),
                                    noise=PRNGKey(50 + b) if sampler == "sde2m" else None)))
    with torch.no_grad():
        eager = vdm.fast_stepper(params, B, "cuda", ctxs[0], graph=False, step_eta=float(sampler == "sde2m"), inpaint=True)
        replay = vdm.fast_stepper(params, B, "cuda", ctxs[0], graph=True, step_eta=float(sampler == "sde2m"), inpaint=True)
        assert type(eager).__name__ == "EagerFastStep" and type(replay).__name__ == "GraphedFastStep"
        outs = []
        for bt in batches:
            za = vdm.fast_sample(params, bt["z"], bt["ctx"], sampler, N, stepper=eager, **bt["kw"]).clone()
            zb = vdm.fast_sample(params, bt["z"], bt["ctx"], sampler, N, stepper=replay, **bt["kw"]).clone()
            zc = vdm.fast_sample(params, bt["z"], bt["ctx"], sampler, N, graph=False, **bt["kw"])
            assert torch.equal(za, zb), float((za - zb).abs().max())
            assert torch.equal(za, zc)
            assert bool(torch.isfinite(za).all())
            k = bt["kw"]["mask"] != 0
            g0 = vdm._fast_gamma(params, bt["ctx"], torch.zeros(B, device="cuda"))
            assert torch.equal(za[k], ops.inpaint_mix(za, bt["kw"]["known"], bt["kw"]["mask"], g0)[k])
            dec = vdm.generate_x(params, za, bt["ctx"].get("coeffs")).reshape(B, 3072)
            assert torch.equal(dec[k], bt["xu"][k])
            outs.append(za)
        assert not torch.equal(outs[0], outs[1])
        bt = batches[1]
        other = dict(bt["kw"], known_noise=PRNGKey(99))
        zd = vdm.fast_sample(params, bt["z"], bt["ctx"], sampler, N, stepper=replay, **other)
        assert not torch.equal(zd[bt["kw"]["mask"] == 0], outs[1][bt["kw"]["mask"] == 0])      # the known-region key matters
        plain_kw = dict(noise=bt["kw"]["noise"])
        with pytest.raises(ValueError, match="mask"):                # built with a mask, run without
            vdm.fast_sample(params, bt["z"], bt["ctx"], sampler, N, stepper=replay, **plain_kw)
        with pytest.raises(ValueError, match="mask"):
            replay(bt["z"], 1.0, 0.75, 1, 0)
        bare = vdm.fast_stepper(params, B, "cuda", ctxs[0], graph=False, step_eta=float(sampler == "sde2m"))
        with pytest.raises(ValueError, match="mask"):                # and the reverse
            vdm.fast_sample(params, bt["z"], bt["ctx"], sampler, N, stepper=bare, **bt["kw"])
        with pytest.raises(ValueError, match="mask"):
            bare.set_known(bt["kw"]["known"], bt["kw"]["mask"], PRNGKey(1))
        with pytest.raises(ValueError, match="known_noise"):
            vdm.fast_sample(params, bt["z"], bt["ctx"], sampler, N, graph=False, **dict(bt["kw"], known_noise=None))
        with pytest.raises(ValueError):                              # shapes
            vdm.fast_sample(params, bt["z"], bt["ctx"], sampler, N, graph=False,
                            **dict(bt["kw"], mask=bt["kw"]["mask"][:1]))
        with pytest.raises(ValueError, match="resample"):
            vdm.fast_sample(params, bt["z"], bt["ctx"], sampler, N, graph=False, **dict(bt["kw"], resample=0))


# ---------------------------------------------------------------------------------- 10. end to end
def _tiny_checkpoint(tmp_path, seed):
    from mulan_amd import checkpoint as ck
    from mulan_amd.experiment import Experiment_VDM
    exp = Experiment_VDM(_config("mulan_velocity", "vdm", 1))
    _randomise_ema(exp, seed)
    ck.save(str(tmp_path), exp.state.state_dict())
    del exp


def test_colab_inpaint_end_to_end(tmp_path):
    """Experiment_Colab.inpaint on 4 images under a half:left mask: the kept pixels come back as they went in (argmax
    decoding, no paste), the unknown half is drawn, the same rng gives the same bytes; every embedding form runs;
    sample_batches without a mask still draws its three sub-keys as before"""
    from mulan_amd import sampling
    from mulan_amd.evaluators import Experiment_Colab
    from mulan_amd.rng import PRNGKey
    _tiny_checkpoint(tmp_path, 6)
    colab = Experiment_Colab(_config("mulan_velocity", "vdm", 1), str(tmp_path))
    images = torch.from_numpy(np.random.default_rng(1).integers(0, 256, (4, 32, 32, 3)).astype(np.uint8))
    keep = sampling.mask_from_spec("half:left")
    out = colab.inpaint(images, keep, steps=3, rng=PRNGKey(7))
    assert out.dtype == torch.uint8 and tuple(out.shape) == (4, 32, 32, 3)
    got = out.cpu().numpy()
    assert np.array_equal(got[:, :, :16], images.numpy()[:, :, :16])
    assert not np.array_equal(got[:, :, 16:], images.numpy()[:, :, 16:])
    assert torch.equal(out, colab.inpaint(images, keep, steps=3, rng=PRNGKey(7)))
    assert not torch.equal(out, colab.inpaint(images, keep, steps=3, rng=PRNGKey(8)))
    emb = torch.zeros(50); emb[5:20] = 1.0
    for kw in (dict(embedding='random'), dict(embedding='encoder', sampler='dpm2m'), dict(embedding=emb, resample=2),
               dict(sampler='ddim', eta=0.5, mask_shape=4)):
        m = keep if "mask_shape" not in kw else np.broadcast_to(keep[None, :, :, None], (4, 32, 32, 3))
        kw.pop("mask_shape", None)
        o = colab.inpaint(images.cuda(), m, steps=3, rng=PRNGKey(7), **kw).cpu().numpy()
        assert np.array_equal(o[:, :, :16], images.numpy()[:, :, :16]) and not np.array_equal(o, got), kw
    with pytest.raises(ValueError, match="ancestral"):
        colab.inpaint(images, keep, sampler='ancestral', steps=3)
    with pytest.raises(ValueError, match="resample"):
        colab.inpaint(images, keep, steps=3, resample=1.5)
    with pytest.raises(ValueError, match="mask"):
        colab.inpaint(images, keep[:16], steps=3)
    with pytest.raises(ValueError, match="embedding"):
        colab.sample_batches([PRNGKey(1)], 2, "encoder", "dpm2m", 3)
    # without a mask: key.split(3) -> (z_1, embedding logits, step noise), generate_x under key.fold_in(steps)
    from mulan_amd import ops
    key = PRNGKey(4).fold_in(1)
    for sampler in ("dpm2m", "sde2m"):
        x = colab.sample_batches([key], 2, "random", sampler, 3)[0]
        k_z, k_e, k_s = key.split(3)
        emb = ops.topk_hard(k_e.normal((2, 50), colab.device), 15)[0]
        direct, _ = colab.draw_samples(colab.params, 2, emb, k_z, k_s, key.fold_in(3), sampler, 3,
                                       prior_scale=float(colab.config.model.sigma_prior))
        assert torch.equal(x, direct), sampler


# ---------------------------------------------------------------------------------- 11. the command line
def test_sample_cli_inpaints(tmp_path):
    """python -m ldm.sample --inpaint_images on a tiny checkpoint: the file holds the images, the mask and the
    settings; the kept pixels equal the input's; five images in batches of two (the last batch padded)"""
    _tiny_checkpoint(tmp_path / "ck", 8)
    rng = np.random.default_rng(2)
    images = rng.integers(0, 256, (5, 32, 32, 3)).astype(np.uint8)
    np.savez(tmp_path / "in.npz", images=images)
    over = ["--config.data.dataset=synthetic", "--config.model.sm_n_layer=1", "--config.model.forward_n_layer=1",
            "--config.training.batch_size_train=4", "--config.training.batch_size_eval=4", "--config.training.substeps=1"]
    out = tmp_path / "out.npz"
    args = [f"--config={os.path.join(ROOT, 'ldm', 'configs', 'cifar10-conditioned.py')}", *over,
            f"--checkpoint_directory={tmp_path / 'ck'}", f"--inpaint_images={tmp_path / 'in.npz'}", "--mask=box:8,4,24,30",
            "--resample=2", "--sampler=sde2m", "--batch_size=2", "--steps=3", "--seed=4", f"--out={out}"]
    env = {**os.environ, "MULAN_FORCE_DEVICE": "0", "PYTHONPATH": ROOT}
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, "-m", "ldm.sample", *args], capture_output=True, text=True, timeout=400, env=env,
                       cwd=ROOT)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    z = np.load(out)
    assert z["images"].shape == (5, 32, 32, 3) and z["images"].dtype == np.uint8
    assert z["mask"].shape == (5, 32, 32) and z["mask"].dtype == np.uint8
    keep = z["mask"] != 0
    assert not keep[:, 8:24, 4:30].any() and keep.sum() == 5 * (1024 - 16 * 26)
    assert np.array_equal(z["images"][keep], images[keep])
    assert not np.array_equal(z["images"][~keep], images[~keep])
    s = str(z["settings"])
    assert '"sampler": "sde2m"' in s and '"resample": 2' in s and '"mask": "box:8,4,24,30"' in s and '"n_samples": 5' in s
