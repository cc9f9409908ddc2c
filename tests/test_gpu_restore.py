"""Restoration with the few-step samplers (mulan_amd.sampling.run): the projection and measurement kernels
against float64 (tests/restore_oracle.py) on every degradation and group size, their refusals, the restoring step as
projection + the existing step kernel bit for bit, the whole models against the float64 oracle loop on shared noise, the
replayed stepper against the eager one, the front ends and the law A z_0 = k_z A z_t + k_x y on a linear-Gaussian model."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import restore_oracle as ro
from tests import stochastic_sampler_oracle as so
from tests.oracle_dev import run_oracle
from tests.test_gpu_fast_sampler import KINDS, ROOT, _config, _ctx, _randomise_ema, _setup
from tests.test_gpu_inpaint import BAR, MODELS, _d, _dev, _tiny_checkpoint

U24 = 2.0 ** -24
HWC = (32, 32, 3)
# (H, W, C, spec): every degradation at 32 x 32 x 3 (group sizes 3, 4, 16, 64, 256, 12, 768); one group spanning the
# whole image plane at 8 x 8 x 3; H != W
SHAPES = [(32, 32, 3, s) for s in ("gray", "sr:2", "sr:4", "sr:8", "sr:16", "sr:2+gray", "sr:16+gray")] + \
         [(8, 8, 3, "sr:8"), (8, 8, 3, "sr:8+gray"), (16, 32, 3, "sr:4")]
IDS = [f"{h}x{w}x{c}-{s}" for h, w, c, s in SHAPES]


def _bar(n_g, *tensors):
    """(n_g + 8) 2^-24 max(|x_hat|, |y|) per sample, shaped to broadcast over [B, H, W, C]: the sum of n_g values in any
    order errs by at most (n_g - 1) u of their largest, the division, the difference to y and the final sum by one
    rounding each of at most 1, 2 and 3 times that largest value: (n_g + 5) u, with 3 u to spare"""
    B = tensors[0].shape[0]
    top = torch.stack([t.double().abs().reshape(B, -1).amax(dim=1).cpu() for t in tensors]).amax(dim=0)
    return ((n_g + 8) * U24 * top).reshape(B, 1, 1, 1)


def _case(seed, B, H, W, C, spec, per_sample):
    f, gray = ro.SPECS[spec]
    rng = np.random.default_rng(seed)
    z, net = (_dev(rng.standard_normal((B, H, W, C)).astype(np.float32)) for _ in range(2))
    g = _dev(rng.uniform(-13.3, 5.0, (B,) if per_sample else (B, H, W, C)).astype(np.float32))
    y = _dev(rng.uniform(-1.0, 1.0, (B, H // f, W // f, 1 if gray else C)).astype(np.float32))
    return f, gray, z, net, g, y


# ---------------------------------------------------------------------------------- 1. the projection against float64
@pytest.mark.parametrize("H,W,C,spec", SHAPES, ids=IDS)
@pytest.mark.parametrize("per_sample", [False, True])
@pytest.mark.parametrize("mode", [0, 1, 2])
def test_project_kernel(H, W, C, spec, per_sample, mode):
    """x_hat is what the step kernel hands on as x0 for this mode (asked of it with the same inputs); the oracle projects
    those fp32 values in float64, so the bar covers the projection alone and holds for any summation order"""
    from mulan_amd import ops
    for B in (1, 3):
        f, gray, z, net, g, y = _case(10 * mode + B, B, H, W, C, spec, per_sample)
        n_g = ro.group_size(f, gray, C)
        xh = ops.fast_sampler_step(z, net, g, g - 0.25, mode)[1]
        if mode == 2:
            assert torch.equal(xh, net)
        ref = ro.project(_d(xh), _d(y), f, gray)
        out = ops.restore_project(z, net, g, y, f, gray, mode)
        assert out.shape == z.shape and out.dtype == torch.float32
        bar = _bar(n_g, xh, y)
        err = (_d(out) - ref).abs()
        back = (ro.measure(_d(out), f, gray) - _d(y)).abs()
        print(f"{spec} B {B} mode {mode} per_sample {per_sample}: n_g {n_g} err {float((err / bar).max()):.3g} of the bar, "
              f"A x' - y {float((back / bar).max()):.3g} of the bar")
        assert bool((err <= bar).all()), float((err / bar).max())
        assert bool((back <= bar).all()), float((back / bar).max())
        assert torch.equal(out, ops.restore_project(z, net, g, y, f, gray, mode))                # the same bits again
        # x_hat has the bits of the step kernel's x0: handing x0 over as the prediction (mode 2) fills the band with the
        # very values the kernel forms itself, so the two outputs agree bit for bit, and would not if one x_hat differed
        assert torch.equal(out, ops.restore_project(z, xh, g, y, f, gray, 2))
        flat = ops.restore_project(z.reshape(B, -1), net.reshape(B, -1), g, y, f, gray, mode, hwc=(H, W, C))
        assert flat.shape == (B, H * W * C) and torch.equal(flat.view(out.shape), out)
        inplace = net.clone()
        assert ops.restore_project(z, inplace, g, y, f, gray, mode, out=inplace) is inplace and torch.equal(inplace, out)


# ---------------------------------------------------------------------------------- 2. the measurement
@pytest.mark.parametrize("H,W,C,spec", SHAPES, ids=IDS)
def test_measure_kernel(H, W, C, spec):
    from mulan_amd import ops
    for B in (1, 3):
        f, gray, x, _, _, _ = _case(50 + B, B, H, W, C, spec, False)
        n_g = ro.group_size(f, gray, C)
        y = ops.restore_measure(x, f, gray)
        assert tuple(y.shape) == (B, H // f, W // f, 1 if gray else C) == ops.restore_y_shape(B, H, W, C, f, gray)
        bar = _bar(n_g, x)
        err = (_d(y) - ro.measure(_d(x), f, gray)).abs()
        print(f"{spec} B {B}: measure {float((err / bar).max()):.3g} of the bar")
        assert bool((err <= bar).all())
        assert torch.equal(y, ops.restore_measure(x, f, gray))
        assert torch.equal(y, ops.restore_measure(x.reshape(B, -1), f, gray, hwc=(H, W, C)))
        # the same reduction in the same order: projecting x onto its own measurement changes it by rounding at most
        same = ops.restore_project(torch.zeros_like(x), x, torch.zeros(B, device="cuda"), y, f, gray, 2)
        back = (_d(same) - _d(x)).abs()
        print(f"{spec} B {B}: project(x, measure(x)) - x {float(back.max()):.3g}")
        assert bool((back <= bar).all())
        # A A+ = I on the device too: a replicated measurement measures back to itself
        up = _dev(ro.replicate(_d(y), f, gray, C).float().numpy())
        assert bool(((_d(ops.restore_measure(up, f, gray)) - _d(y)).abs() <= _bar(n_g, y)).all())


# ---------------------------------------------------------------------------------- 3. refusals
def test_entry_points_refuse_bad_arguments():
    """every bad argument: hipErrorInvalidValue (1) from the library before any launch (the output keeps its bits), and
    a ValueError or the library's error through ops"""
    from mulan_amd import lib, ops
    h = lib.load()
    B, H, W, C = 2, 8, 8, 3
    buf = torch.randn(6, B * H * W * C, device="cuda")
    before = buf.clone()
    p = lambda i: buf[i].data_ptr()

    def rc(fn, good, **kw):
        a = list(good)
        for k, v in kw.items():
            a[int(k[1:])] = v
        return fn(*a)
    proj = [p(0), p(1), p(2), p(3), p(4), B, H, W, C, 4, 0, 1, 0, None]
    for i in range(5):                                                       # z, net, g_t, y, xh_out
        assert rc(h.mulan_restore_project, proj, **{f"a{i}": None}) == 1, i
    for mode in (-1, 3):
        assert rc(h.mulan_restore_project, proj, a11=mode) == 1
    for f in (0, 1, 3, 5, 32, -2):                                           # f outside the list (1 goes with gray only)
        assert rc(h.mulan_restore_project, proj, a9=f) == 1, f
    assert rc(h.mulan_restore_project, proj, a9=16) == 1                     # in the list, but 16 does not divide 8
    assert rc(h.mulan_restore_project, proj, a6=12, a9=8) == 1 and rc(h.mulan_restore_project, proj, a7=12, a9=8) == 1
    for i in (5, 6, 7, 8):                                                   # B H W C == 0
        assert rc(h.mulan_restore_project, proj, **{f"a{i}": 0}) == 1, i
    for per in (1, B, H * W * C - 1, -1, B * H * W * C):                     # neither 0 nor H W C
        assert rc(h.mulan_restore_project, proj, a12=per) == 1, per
    meas = [p(0), p(5), B, H, W, C, 4, 0, None]
    for i in (0, 1):
        assert rc(h.mulan_restore_measure, meas, **{f"a{i}": None}) == 1
    for f in (0, 1, 3, 16):
        assert rc(h.mulan_restore_measure, meas, a6=f) == 1
    assert rc(h.mulan_restore_measure, meas, a2=0) == 1
    torch.cuda.synchronize()
    assert torch.equal(buf.view(torch.int32), before.view(torch.int32))      # nothing was launched
    assert rc(h.mulan_restore_project, proj) == 0 and rc(h.mulan_restore_project, proj, a12=H * W * C) == 0
    assert rc(h.mulan_restore_project, proj, a9=1, a10=1) == 0 and rc(h.mulan_restore_measure, meas) == 0
    torch.cuda.synchronize()
    z, net = (torch.randn(B, H, W, C, device="cuda") for _ in range(2))
    g, y = torch.zeros(B, device="cuda"), torch.zeros(B, 2, 2, 3, device="cuda")
    err = (ValueError, lib.MulanHipError)
    for kw in (dict(f=3), dict(f=16), dict(f=1), dict(mode=3), dict(mode=-1), dict(y=y[:1]), dict(y=y.double()),
               dict(g=torch.zeros(5, device="cuda")), dict(net=net[:1]), dict(z=None), dict(y=None), dict(y=y.cpu()),
               dict(hwc=(8, 8, 4))):
        a = dict(z=z, net=net, g=g, y=y, f=4, gray=False, mode=1, hwc=None)
        a.update(kw)
        with pytest.raises(err):
            ops.restore_project(a["z"], a["net"], a["g"], a["y"], a["f"], a["gray"], a["mode"], hwc=a["hwc"])
    with pytest.raises(err):
        ops.restore_project(z.reshape(B, -1), net, g, y, 4, False, 1)        # no image shape
    for f, gray in ((3, False), (1, False), (16, True)):
        with pytest.raises(err):
            ops.restore_measure(z, f, gray)
    with pytest.raises(err):
        ops.restore_measure(z.double(), 4, False)


# ---------------------------------------------------------------------------------- 4. a restoring step
@pytest.mark.parametrize("step_eta", [0.0, 1.0])
def test_a_restoring_step_is_the_projection_and_the_step_kernel(step_eta):
    """model.EagerFastStep built with a degradation, one first-order and one second-order step, against
    ops.restore_project followed by the existing step kernel at mode 2 on x_hat', called by hand: the same bits, and the
    history is x_hat'"""
    from mulan_amd import ops
    from mulan_amd.rng import PRNGKey
    B = 2
    vdm, params, _, _ = _setup("mulan_velocity", "vdm", False)
    ctx = _ctx(vdm, params, B)
    f, gray = 4, False
    y = ops.restore_measure(ops.encode_u8(_dev(np.random.default_rng(3).integers(0, 256, (B, 32, 32, 3)).astype(np.uint8))),
                            f, gray)
    xis = [PRNGKey(5).fold_in(k).normal((B, 3072), "cuda") for k in range(2)]
    t32 = lambda t: torch.full((B,), float(np.float32(t)), device="cuda")
    with torch.no_grad():
        st = vdm.fast_stepper(params, B, "cuda", ctx, graph=False, step_eta=step_eta, restore=(f, gray))
        assert type(st).__name__ == "EagerFastStep" and st.restore == (f, gray)
        st.set_measurement(y)
        if step_eta > 0:
            st.set_noise(lambda k: xis[k])
        z = PRNGKey(6).normal((B, 3072), "cuda")
        g_p = x_p = None
        for k, (t, s, order) in enumerate(((1.0, 0.75, 1), (0.75, 0.5, 2))):
            got = st(z, t, s, order, k)
            g_t, g_s = vdm._fast_gamma(params, ctx, t32(t)), vdm._fast_gamma(params, ctx, t32(s))
            net = vdm._fast_net(params, z, g_t, ctx)
            xh = ops.restore_project(z, net, g_t, y, f, gray, vdm._fast_mode(), hwc=HWC)
            hist = (g_p, x_p) if order == 2 else (None, None)
            if step_eta > 0:
                want, x0 = ops.stochastic_sampler_step(z, xh, g_t, g_s, 2, xis[k], step_eta, *hist)
            else:
                want, x0 = ops.fast_sampler_step(z, xh, g_t, g_s, 2, *hist)
            assert torch.equal(got, want), (k, float((got - want).abs().max()))
            assert torch.equal(x0, xh) and torch.equal(st._step.x_prev, xh) and not torch.equal(xh, net)
            via = vdm._fast_step(params, z, t32(t), t32(s), *hist, ctx, xis[k] if step_eta > 0 else None, step_eta,
                                 measurement=y, restore=(f, gray))
            assert torch.equal(via[0], want) and torch.equal(via[1], xh)
            g_p, x_p, z = g_t, xh, got


# ---------------------------------------------------------------------------------- 5. whole models, pathwise
@pytest.mark.parametrize("spec", ["sr:4", "gray"])
@pytest.mark.parametrize("vdm_type,unet_type,vfe", MODELS)
def test_restoration_matches_the_oracle_loop(vdm_type, unet_type, vfe, spec):
    """dpm2m with resample 1 and sde2m with resample 2 over N = 4 steps, B = 2, the same noise on both sides: every
    operation of the oracle's loop from the oracle's input (and history) against the oracle's output.  A step has the
    budget of test_inpainting_matches_the_oracle_loop: 2e-4 of max |net| x the step's d z_s / d net (the projection is a
    contraction in x_hat and adds nothing), 1e-5 of the result, and the kernel bar of the step's noise term; a jump
    carries no network error and is held to the 1e-5 of the result alone"""
    from mulan_amd import ops
    from mulan_amd.rng import PRNGKey
    B, N = 2, 4
    f, gray = ro.SPECS[spec]
    z_init = PRNGKey(21).fold_in(1000).normal((B, 3072), "cuda")
    xu = _dev(np.random.default_rng(2).integers(0, 256, (B, 32, 32, 3)).astype(np.uint8))
    y = ops.restore_measure(ops.encode_u8(xu), f, gray)
    k_s, k_k = PRNGKey(22), PRNGKey(23)
    f32 = lambda t: torch.full((B,), float(np.float32(t)), device="cuda")
    vdm, params, ref_params, ocfg = _setup(vdm_type, unet_type, vfe)
    ctx = _ctx(vdm, params, B)
    loop = ro.plain_loop if vdm_type == "plain" else ro.mulan_loop
    grid = [1.0 - k / N for k in range(N + 1)]
    for sampler, eta, U in (("dpm2m", 0.0, 1), ("sde2m", 1.0, 2)):
        sx = [ops.randn((B, 3072), k_s.fold_in(k).v, 0, "cuda") for k in range(U * N)]
        kx = [ops.randn((B, 3072), k_k.fold_in(j).v, 0, "cuda") for j in range(U * N)]
        z_ref, events = run_oracle(
            lambda P, z_, y_, s_, k_: loop(P, ocfg, z_, grid, sampler, eta, y_, f, gray, lambda k: s_[k], lambda j: k_[j], U),
            ref_params, _d(z_init), _d(y), [_d(t) for t in sx], [_d(t) for t in kx])
        steps = [e for e in events if e["kind"] == "step"]
        assert len(steps) == N + (U - 1) * (N - 1) and sum(e["kind"] == "jump" for e in events) == (U - 1) * (N - 1)
        flat = lambda t: t.reshape(B, -1).float().cuda()
        with torch.no_grad():
            for e in events:
                want = e["z_out"].reshape(B, -1).numpy()
                scale = 1e-5 * float(np.abs(want).max())
                if e["kind"] == "jump":
                    got = ops.forward_jump(flat(e["z_in"]), vdm._fast_gamma(params, ctx, f32(e["s"])),
                                           vdm._fast_gamma(params, ctx, f32(e["t"])), kx[e["j"]])
                    allowed = scale
                else:
                    if e["order"] == 2:
                        g_p, x_p = vdm._fast_gamma(params, ctx, f32(grid[e["k"] - 1])), flat(e["x_p"])
                    else:
                        g_p = x_p = None
                    got, _, _ = vdm._fast_step(params, flat(e["z_in"]), f32(e["t"]), f32(e["s"]), g_p, x_p, ctx,
                                               sx[e["kk"]] if eta > 0 else None, eta, measurement=y, restore=(f, gray))
                    allowed = 2e-4 * e["budget"] + scale + BAR * e["noise"]
                err = np.abs(got.cpu().double().numpy() - want).max()
                print(f"{vdm_type} {spec} {sampler} x{U} {e['kind']} {e.get('kk', '')}: err {err:.3g} allowed {allowed:.3g}")
                assert err < allowed, (sampler, e["kind"], e.get("kk"), err, allowed)


# ---------------------------------------------------------------------------------- 6. replay equals eager
@pytest.mark.parametrize("vdm_type,unet_type", [("mulan_velocity", "vdm"), ("plain", "vdm")])
@pytest.mark.parametrize("sampler,resample", [("dpm2m", 1), ("sde2m", 2)])
def test_replayed_restoration_equals_the_eager_run(vdm_type, unet_type, sampler, resample):
    """model.GraphedFastStep built with a degradation (the measurement a static buffer, the projection captured between
    the network and the step kernel, the jumps eager launches) against model.EagerFastStep: the same bits over two
    batches with other measurements, contexts and keys through one stepper each, and what fresh steppers give; a run
    with resample 1 needs no key for the jumps; a stepper serves the degradation it was built for and no other run"""
    from mulan_amd import ops
    from mulan_amd.rng import PRNGKey
    B, N, spec = 2, 4, "sr:4+gray"
    f, gray = ro.SPECS[spec]
    vdm, params, _, _ = _setup(vdm_type, unet_type, False)
    rng = np.random.default_rng(6)
    cond = lambda v: torch.full((B,), v, dtype=torch.uint8, device="cuda")
    if hasattr(vdm, "deterministic_embedding"):
        emb2 = torch.zeros((B, 50), device="cuda"); emb2[:, 20:35] = 1.0
        ctxs = [_ctx(vdm, params, B), vdm.fast_context(params, emb2, cond(0))]
    else:
        ctxs = [_ctx(vdm, params, B), vdm.fast_context(params, None, cond(1))]
    eta = float(sampler == "sde2m")
    batches = []
    for b in range(2):
        y = ops.restore_measure(ops.encode_u8(_dev(rng.integers(0, 256, (B, 32, 32, 3)).astype(np.uint8))), f, gray)
        batches.append(dict(z=PRNGKey(11 + b).normal((B, 3072), "cuda"), ctx=ctxs[b],
                            kw=dict(measurement=y, degradation=spec, resample=resample,
                                    known_noise=PRNGKey(40 + b) if resample > 1 else None,
                                    noise=PRNGKey(50 + b) if eta else None)))
    with torch.no_grad():
        eager = vdm.fast_stepper(params, B, "cuda", ctxs[0], graph=False, step_eta=eta, restore=(f, gray))
        replay = vdm.fast_stepper(params, B, "cuda", ctxs[0], graph=True, step_eta=eta, restore=spec)
        assert type(eager).__name__ == "EagerFastStep" and type(replay).__name__ == "GraphedFastStep"
        outs = []
        for bt in batches:
            za = vdm.fast_sample(params, bt["z"], bt["ctx"], sampler, N, stepper=eager, **bt["kw"]).clone()
            zb = vdm.fast_sample(params, bt["z"], bt["ctx"], sampler, N, stepper=replay, **bt["kw"]).clone()
            zc = vdm.fast_sample(params, bt["z"], bt["ctx"], sampler, N, graph=False, **bt["kw"])
            assert torch.equal(za, zb), float((za - zb).abs().max())
            assert torch.equal(za, zc) and bool(torch.isfinite(za).all())
            outs.append(za)
        assert not torch.equal(outs[0], outs[1])
        bt = batches[1]
        plain = vdm.fast_sample(params, bt["z"], bt["ctx"], sampler, N, graph=False, noise=bt["kw"]["noise"])
        assert not torch.equal(plain, outs[1])                                # the measurement matters
        with pytest.raises(ValueError, match="degradation"):                  # built with a degradation, run without
            vdm.fast_sample(params, bt["z"], bt["ctx"], sampler, N, stepper=replay, noise=bt["kw"]["noise"])
        with pytest.raises(ValueError, match="degradation"):                  # ... or with another
            vdm.fast_sample(params, bt["z"], bt["ctx"], sampler, N, stepper=replay,
                            **dict(bt["kw"], degradation="gray", measurement=torch.zeros(B, 32, 32, 1, device="cuda")))
        bare = vdm.fast_stepper(params, B, "cuda", ctxs[0], graph=False, step_eta=eta)
        with pytest.raises(ValueError, match="degradation"):                  # and the reverse
            vdm.fast_sample(params, bt["z"], bt["ctx"], sampler, N, stepper=bare, **bt["kw"])
        with pytest.raises(ValueError, match="degradation"):
            bare.set_measurement(bt["kw"]["measurement"])
        with pytest.raises(ValueError, match="measurement"):                  # the y shape of the table
            vdm.fast_sample(params, bt["z"], bt["ctx"], sampler, N, graph=False,
                            **dict(bt["kw"], measurement=torch.zeros(B, 8, 8, 3, device="cuda")))
        with pytest.raises(ValueError, match="fp32"):
            vdm.fast_sample(params, bt["z"], bt["ctx"], sampler, N, graph=False,
                            **dict(bt["kw"], measurement=bt["kw"]["measurement"].double()))
        with pytest.raises(ValueError, match="mask and a measurement"):
            vdm.fast_sample(params, bt["z"], bt["ctx"], sampler, N, graph=False, known=torch.zeros(B, 3072, device="cuda"),
                            mask=torch.ones(B, 3072, dtype=torch.uint8, device="cuda"), **bt["kw"])
        with pytest.raises(ValueError, match="known_noise"):
            vdm.fast_sample(params, bt["z"], bt["ctx"], sampler, N, graph=False,
                            **dict(bt["kw"], resample=2, known_noise=None))


# ---------------------------------------------------------------------------------- 7. nothing measured: as before
def test_a_run_without_a_measurement_is_the_sampler_of_before():
    """the three few-step samplers through the new signatures with nothing measured: the z_0 bits of a loop over
    sampling.EagerStepper built and called the old way, which never meets the new keywords"""
    from mulan_amd import sampling
    from mulan_amd.rng import PRNGKey
    B, N = 2, 5
    vdm, params, _, _ = _setup("mulan_velocity", "vdm", False)
    ctx = _ctx(vdm, params, B)
    z1 = PRNGKey(3).normal((B, 3072), "cuda")
    xis = [PRNGKey(4).fold_in(k).normal((B, 3072), "cuda") for k in range(N)]
    times = lambda t: torch.full((B,), float(np.float32(t)), device="cuda")
    gamma_fn = lambda t: vdm._fast_gamma(params, ctx, times(t))
    net_fn = lambda z, t: vdm._fast_net(params, z, gamma_fn(t), ctx)
    with torch.no_grad():
        for sampler, eta in (("ddim", 0.0), ("ddim", 0.5), ("dpm2m", 0.0), ("sde2m", 0.0)):
            step_eta = sampling.check_eta(sampler, eta)
            noise = (lambda k: xis[k]) if step_eta > 0 else None
            grid, orders = sampling.time_grid(N), sampling.step_orders(sampler, N)
            old = sampling.EagerStepper(net_fn, gamma_fn, vdm._fast_mode(), step_eta, noise)
            z = z1
            for k, order in enumerate(orders):
                z = old(z, grid[k], grid[k + 1], order, k)
            for graph in (False, True):
                new = vdm.fast_sample(params, z1, ctx, sampler, N, graph=graph, eta=eta, noise=noise, measurement=None,
                                      degradation=None)
                assert torch.equal(new, z), (sampler, eta, graph)
            assert torch.equal(sampling.sample(net_fn, gamma_fn, z1, vdm._fast_mode(), sampler, steps=N, eta=eta,
                                               noise_fn=noise, measurement=None, degradation=None), z)


# ---------------------------------------------------------------------------------- 8. end to end
def test_colab_restore_end_to_end(tmp_path):
    """Experiment_Colab.restore on 3 images: uint8 images and a finite residual per image; the measurement of the
    images gives the same bits as the images; the same rng the same bytes; uint8 measurements, the other degradations,
    embeddings and resampling run; sample_batches without a measurement draws as before"""
    from mulan_amd import ops
    from mulan_amd.evaluators import Experiment_Colab
    from mulan_amd.rng import PRNGKey
    _tiny_checkpoint(tmp_path, 6)
    colab = Experiment_Colab(_config("mulan_velocity", "vdm", 1), str(tmp_path))
    images = torch.from_numpy(np.random.default_rng(1).integers(0, 256, (3, 32, 32, 3)).astype(np.uint8))
    out, res = colab.restore(images=images, degradation='sr:4', steps=3, rng=PRNGKey(7))
    assert out.dtype == torch.uint8 and tuple(out.shape) == (3, 32, 32, 3)
    assert res.dtype == torch.float32 and tuple(res.shape) == (3,) and bool(torch.isfinite(res).all())
    print("residual (grey levels), sr:4, sde2m, 3 steps:", res.cpu().numpy())
    y = ops.restore_measure(ops.encode_u8(images.cuda()), 4, False)
    out2, res2 = colab.restore(measurement=y, degradation='sr:4', steps=3, rng=PRNGKey(7))
    assert torch.equal(out, out2) and torch.equal(res, res2)
    out3, _ = colab.restore(measurement=y.cpu().numpy(), degradation='sr:4', steps=3, rng=PRNGKey(8))
    assert not torch.equal(out, out3)
    plain = colab.sample_batches([PRNGKey(7).fold_in(colab.rank)], 3, 'deterministic', 'sde2m', 3)[0]
    assert not torch.equal(out, plain)
    levels = torch.from_numpy(np.random.default_rng(2).integers(0, 256, (3, 16, 16, 1)).astype(np.uint8))
    emb = torch.zeros(50); emb[5:20] = 1.0
    for kw in (dict(measurement=levels, degradation='sr:2+gray', sampler='dpm2m'),
               dict(images=images, degradation='gray', embedding='encoder', resample=2),
               dict(images=images.cuda(), degradation='sr:16', embedding=emb, sampler='ddim', eta=0.5),
               dict(images=images, degradation='sr:8', embedding='random', sampler='dpm2m', resample=2)):
        o, r = colab.restore(steps=3, rng=PRNGKey(7), **kw)
        assert tuple(o.shape) == (3, 32, 32, 3) and bool(torch.isfinite(r).all()), kw
    with pytest.raises(ValueError, match="one of the two"):
        colab.restore(images=images, measurement=y)
    with pytest.raises(ValueError, match="one of the two"):
        colab.restore()
    with pytest.raises(ValueError, match="ancestral"):
        colab.restore(images=images, sampler='ancestral', steps=3)
    with pytest.raises(ValueError, match="sr:f"):
        colab.restore(images=images, degradation='sr:3')
    with pytest.raises(ValueError, match="measurement"):
        colab.restore(measurement=y, degradation='sr:8')
    with pytest.raises(ValueError, match="resample"):
        colab.restore(images=images, steps=3, resample=0)
    # without a measurement: key.split(3) -> (z_1, embedding logits, step noise), generate_x under key.fold_in(steps)
    key = PRNGKey(4).fold_in(1)
    for sampler in ("dpm2m", "sde2m"):
        x = colab.sample_batches([key], 2, "random", sampler, 3)[0]
        k_z, k_e, k_s = key.split(3)
        e = ops.topk_hard(k_e.normal((2, 50), colab.device), 15)[0]
        direct, _ = colab.draw_samples(colab.params, 2, e, k_z, k_s, key.fold_in(3), sampler, 3,
                                       prior_scale=float(colab.config.model.sigma_prior))
        assert torch.equal(x, direct), sampler
    # a restoring run with resample 1 draws nothing from the fourth sub-key: any known_rng gives the same bytes
    k_z, k_e, k_s = key.split(3)
    a, _ = colab.draw_samples(colab.params, 3, None, k_z, k_s, key.fold_in(3), "sde2m", 3, measurement=y,
                              degradation='sr:4', known_rng=PRNGKey(1))
    b, _ = colab.draw_samples(colab.params, 3, None, k_z, k_s, key.fold_in(3), "sde2m", 3, measurement=y,
                              degradation='sr:4')
    assert torch.equal(a, b)


def test_sample_cli_restores(tmp_path):
    """python -m ldm.sample --restore_images on a tiny checkpoint, one process: the file holds the images, the
    measurement, the degradation, the residual and the settings; five images in batches of two (the last batch padded);
    a file that holds that measurement in place of the images gives the same file"""
    _tiny_checkpoint(tmp_path / "ck", 8)
    images = np.random.default_rng(2).integers(0, 256, (5, 32, 32, 3)).astype(np.uint8)
    np.savez(tmp_path / "in.npz", images=images)
    over = ["--config.data.dataset=synthetic", "--config.model.sm_n_layer=1", "--config.model.forward_n_layer=1",
            "--config.training.batch_size_train=4", "--config.training.batch_size_eval=4", "--config.training.substeps=1"]
    env = {**os.environ, "MULAN_FORCE_DEVICE": "0", "PYTHONPATH": ROOT}
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        env.pop(k, None)

    def run(src, out):
        args = [f"--config={os.path.join(ROOT, 'ldm', 'configs', 'cifar10-conditioned.py')}", *over,
                f"--checkpoint_directory={tmp_path / 'ck'}", f"--restore_images={src}", "--degradation=sr:4",
                "--resample=2", "--sampler=sde2m", "--batch_size=2", "--steps=3", "--seed=4", f"--out={out}"]
        r = subprocess.run([sys.executable, "-m", "ldm.sample", *args], capture_output=True, text=True, timeout=400,
                           env=env, cwd=ROOT)
        assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
        return np.load(out)
    z = run(tmp_path / "in.npz", tmp_path / "out.npz")
    assert z["images"].shape == (5, 32, 32, 3) and z["images"].dtype == np.uint8
    assert z["measurement"].shape == (5, 8, 8, 3) and z["measurement"].dtype == np.float32
    assert str(z["degradation"]) == "sr:4"
    assert z["residual"].shape == (5,) and z["residual"].dtype == np.float32 and np.isfinite(z["residual"]).all()
    enc = 2.0 * (images.astype(np.float64) + 0.5) / 256.0 - 1.0
    want = enc.reshape(5, 8, 4, 8, 4, 3).mean(axis=(2, 4))
    assert np.abs(z["measurement"] - want).max() < 24 * U24
    back = (2.0 * (z["images"].astype(np.float64) + 0.5) / 256.0 - 1.0).reshape(5, 8, 4, 8, 4, 3).mean(axis=(2, 4))
    assert np.abs(np.abs(back - z["measurement"]).reshape(5, -1).max(axis=1) * 127.5 - z["residual"]).max() < 1e-3
    s = str(z["settings"])
    assert '"sampler": "sde2m"' in s and '"resample": 2' in s and '"degradation": "sr:4"' in s and '"n_samples": 5' in s
    np.savez(tmp_path / "y.npz", measurement=z["measurement"])
    z2 = run(tmp_path / "y.npz", tmp_path / "out2.npz")
    for k in ("images", "measurement", "residual"):
        assert np.array_equal(z2[k], z[k]), k


# ---------------------------------------------------------------------------------- 9. the law A z_0 = k_z A z_t + k_x y
@pytest.mark.parametrize("mode", [1, 2])
@pytest.mark.parametrize("spec", ["sr:4", "sr:2+gray"])
def test_law_of_restoration_on_a_linear_gaussian_model(mode, spec):
    """the model of test_law_of_inpainting_on_a_linear_gaussian_model (the exact posterior mean of x ~ N(mu, sd^2) as
    network, ddim with eta = 1, N = 16, gamma per sample, so the step's coefficients are uniform inside a group): a
    first-order step is z_s = k_z z_t + k_x x_hat' + k_n xi with A x_hat' = y, hence A z_0 = k_z A z_t + k_x y + k_n A xi
    for the last step, exactly in float64 (the oracle's step on the oracle's projection shows it to 1e-13).  The device's
    z_0 is held to it with the projection's bar, (n_g + 8) 2^-24 max(|x_hat|, |y|), scaled by k_x.  Measured on the
    MI355X: 4.1e-8 to 7.5e-8 against bars of 1.4e-6 to 1.8e-6"""
    from mulan_amd import ops, sampling
    from mulan_amd.rng import PRNGKey
    f, gray = ro.SPECS[spec]
    n_g = ro.group_size(f, gray)
    B, N, mu, sd, gmin, gmax, eta = 4, 16, 0.3, 0.5, -13.3, 5.0, 1.0
    k_z1, k_s, k_x = PRNGKey(35).fold_in(mode).split(3)
    z1 = k_z1.normal((B, 32, 32, 3), "cuda")
    y = ops.restore_measure(mu + sd * k_x.normal((B, 32, 32, 3), "cuda"), f, gray)
    gamma32 = lambda t: float(np.float32(gmin + (gmax - gmin) * np.float64(np.float32(t))))
    gamma_fn = lambda t: torch.full((B,), gamma32(t), device="cuda")
    seen = []

    def net_fn(z, t):
        g = gamma_fn(t).double().reshape(B, 1, 1, 1)
        xh = so.posterior_mean(z.double(), g, mu, sd)
        al, si = torch.sqrt(torch.sigmoid(-g)), torch.sqrt(torch.sigmoid(g))
        net = ((z.double() - al * xh) / si if mode == 1 else xh).float()
        seen.append((z.clone(), net))
        return net
    noise_fn = lambda k: ops.randn((B, 32, 32, 3), k_s.fold_in(k).v, 0, "cuda")
    z0 = sampling.sample(net_fn, gamma_fn, z1, mode, "ddim", steps=N, eta=eta, noise_fn=noise_fn, measurement=y,
                         degradation=spec)
    assert len(seen) == N and tuple(z0.shape) == (B, 32, 32, 3)
    grid = sampling.time_grid(N)
    z_t, net = seen[-1]
    g_t = torch.full((B, 1, 1, 1), gamma32(sampling.f32(grid[-2])), dtype=torch.float64)
    g_s = torch.full((B, 1, 1, 1), gamma32(0.0), dtype=torch.float64)
    xi = _d(noise_fn(N - 1))
    # the oracle: its own x_hat, projection and step; A z_s = k_z A z_t + k_x y + k_n A xi
    xh = ro.project(so.fo.x_hat(_d(z_t), _d(net), g_t, KINDS[mode]), _d(y), f, gray)
    z_ref, _, gain, _ = so.stochastic_step(_d(z_t), xh, g_t, g_s, "input", xi, eta)
    k_xc = float(gain.max())                                                   # |d z_s / d x_hat'| = k_x
    h = 0.5 * (g_t - g_s)
    k_zc = float((torch.sqrt(torch.sigmoid(g_s) / torch.sigmoid(g_t)) * torch.exp(-h)).max())
    k_nc = float(torch.sqrt(torch.sigmoid(g_s) * -torch.expm1(-2 * h)).max())
    law = k_zc * ro.measure(_d(z_t), f, gray) + k_xc * _d(y) + k_nc * ro.measure(xi, f, gray)
    assert float((ro.measure(z_ref, f, gray) - law).abs().max()) < 1e-13 * max(1.0, float(law.abs().max()))
    xh32 = ops.fast_sampler_step(z_t, net, gamma_fn(grid[-2]), gamma_fn(0.0), mode)[1]
    proj = (n_g + 8) * U24 * max(float(xh32.abs().max()), float(y.abs().max()))
    err = float((ro.measure(_d(z0), f, gray) - law).abs().max())
    print(f"mode {mode} {spec}: k_z {k_zc:.3g} k_x {k_xc:.3g} k_n {k_nc:.3g}; A z_0 - law {err:.3g}, allowed "
          f"{k_xc * proj:.3g}")
    assert err < k_xc * proj
