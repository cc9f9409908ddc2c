"""Deterministic few-step samplers (DDIM, DPM-Solver++(2M); mulan_amd.sampling): the HIP step kernel against float64,
convergence to the exact probability-flow map of an analytic model, the whole models against the float64 oracle
(tests/fast_sampler_oracle.py), the replayed stepper against the eager one, sample_fn and the `python -m ldm.sample` CLI."""
import dataclasses
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import torch_ref as tr
from tests import fast_sampler_oracle as fo
from tests.oracle_dev import run_oracle
from tests.test_gpu_model import make_cfg
from tests.test_gpu_sampler import _damp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KINDS = {0: "velocity", 1: "epsilon", 2: "input"}


def _rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.abs(a - b).max() / (np.abs(b).max() + 1e-30))


def _inputs(seed, B, per_sample):
    rng = np.random.default_rng(seed)
    gshape = (B,) if per_sample else (B, 3072)
    zt, net, xp = (rng.standard_normal((B, 3072)).astype(np.float32) for _ in range(3))
    gt = rng.uniform(-13.3, 5.0, gshape).astype(np.float32)
    gs = (gt - rng.uniform(1e-3, 0.5, gshape)).astype(np.float32)             # s < t: gamma_s < gamma_t
    gp = (gt + rng.uniform(0.2, 1.0, gshape)).astype(np.float32)              # the previous step's t > t
    return zt, net, gt, gs, gp, xp


@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("per_sample", [False, True])
@pytest.mark.parametrize("order", [1, 2])
def test_fast_sampler_step_kernel(mode, per_sample, order):
    from mulan_amd import ops
    B = 5
    zt, net, gt, gs, gp, xp = _inputs(7 + mode, B, per_sample)
    dev = lambda a: torch.tensor(a).cuda()
    hist = (dev(gp), dev(xp)) if order == 2 else (None, None)
    zs, x0 = ops.fast_sampler_step(dev(zt), dev(net), dev(gt), dev(gs), mode, *hist)
    d = lambda a: torch.tensor(a, dtype=torch.float64)
    g = (lambda a: d(a)[:, None]) if per_sample else d
    ref, xref, _ = fo.fast_step(d(zt), d(net), g(gt), g(gs), KINDS[mode], *((g(gp), d(xp)) if order == 2 else (None, None)))
    # fp32 elementwise chain: a few ulp of the result scale (the bars of test_ancestral_step_kernel)
    bar = 2e-5 if mode == 2 else 2e-6
    assert _rel(zs.cpu().numpy(), ref.numpy()) < bar
    assert _rel(x0.cpu().numpy(), xref.numpy()) < bar
    if mode == 2:
        assert torch.equal(x0, dev(net))


@pytest.mark.parametrize("order", [1, 2])
def test_fast_sampler_step_ragged_and_unaligned(order):
    """n not a multiple of 4 and buffers off the 16-byte grid: the scalar path, same numbers"""
    from mulan_amd import ops
    n = 4099
    rng = np.random.default_rng(5)
    base = [torch.tensor(rng.standard_normal(n + 1).astype(np.float32)).cuda() for _ in range(3)]
    zt, net, xp = (b[1:] for b in base)
    gt_h = rng.uniform(-13.3, 5.0, n + 1).astype(np.float32)
    gt = torch.tensor(gt_h).cuda()[1:]
    gs = torch.tensor(gt_h - 0.3).cuda()[1:]
    gp = torch.tensor(gt_h + 0.4).cuda()[1:]
    hist = (gp, xp) if order == 2 else (None, None)
    zs, x0 = ops.fast_sampler_step(zt, net, gt, gs, 1, *hist)
    d = lambda t: t.cpu().double()
    ref, xref, _ = fo.fast_step(d(zt), d(net), d(gt), d(gs), "epsilon", *((d(gp), d(xp)) if order == 2 else (None, None)))
    assert zs.shape == (n,) and _rel(zs.cpu().numpy(), ref.numpy()) < 2e-6 and _rel(x0.cpu().numpy(), xref.numpy()) < 2e-6


@pytest.mark.parametrize("per_sample", [False, True])
def test_equal_gammas_return_z_exactly(per_sample):
    from mulan_amd import ops
    zt, net, gt, _, gp, xp = _inputs(3, 3, per_sample)
    dev = lambda a: torch.tensor(a).cuda()
    for mode in (0, 1, 2):
        z1, _ = ops.fast_sampler_step(dev(zt), dev(net), dev(gt), dev(gt), mode)
        z2, _ = ops.fast_sampler_step(dev(zt), dev(net), dev(gt), dev(gt), mode, dev(gp), dev(xp))
        assert torch.equal(z1, dev(zt)) and torch.equal(z2, dev(zt)), mode


def test_zero_previous_step_falls_back_to_first_order():
    """an element whose previous step did not move its gamma (h_p = 0), or whose history is NaN: no NaN, and the
    first-order result bit for bit"""
    from mulan_amd import ops
    zt, net, gt, gs, gp, xp = _inputs(4, 4, False)
    gp[:, ::3] = gt[:, ::3]                          # h_p = 0
    gp[:, 1::7] = np.nan                             # no usable history
    dev = lambda a: torch.tensor(a).cuda()
    for mode in (0, 1, 2):
        z1, x1 = ops.fast_sampler_step(dev(zt), dev(net), dev(gt), dev(gs), mode)
        z2, x2 = ops.fast_sampler_step(dev(zt), dev(net), dev(gt), dev(gs), mode, dev(gp), dev(xp))
        assert bool(torch.isfinite(z2).all())
        fb = torch.tensor(~((gp - gt) > 0)).cuda()
        assert torch.equal(z2[fb], z1[fb]) and torch.equal(x1, x2)
        assert not torch.equal(z2[~fb], z1[~fb])


@pytest.mark.parametrize("mode", [0, 1, 2])
def test_convergence_on_an_analytic_model(mode):
    """x ~ N(mu_i, s_i^2) per coordinate, per-pixel gamma from ops.poly_gamma with random coefficients, the exact
    posterior-mean denoiser as the network: the probability-flow map is the per-coordinate quantile map.  RMS error of
    z_0 at N = 16 / 32 / 64: DPM-Solver++(2M) second order (>= 3x per doubling), DDIM first order (>= 1.7x)"""
    from mulan_amd import ops, sampling
    B, gmin, gmax = 2, -13.3, 5.0
    gen = torch.Generator(device="cuda").manual_seed(11 + mode)
    r = lambda *s: torch.randn(*s, device="cuda", generator=gen)
    a, b = r(B, 3072), r(B, 3072)
    c = 1e-3 + torch.nn.functional.softplus(r(B, 3072))
    mu = (torch.rand(B, 3072, device="cuda", generator=gen) - 0.5).double()
    sd = (0.05 + 0.45 * torch.rand(B, 3072, device="cuda", generator=gen)).double()
    z1 = r(B, 3072)

    def gamma_fn(t):
        return ops.poly_gamma(a, b, c, torch.full((B,), t, device="cuda"), gmin, gmax)[2]

    def net_fn(z, t):
        g = gamma_fn(t).double()
        al, si = torch.sqrt(torch.sigmoid(-g)), torch.sqrt(torch.sigmoid(g))
        zd = z.double()
        x = mu + al * sd ** 2 * (zd - al * mu) / (al ** 2 * sd ** 2 + si ** 2)
        out = {0: (al * zd - x) / si, 1: (zd - al * x) / si, 2: x}[mode]
        return out.float()

    al = lambda g: torch.sqrt(torch.sigmoid(-g))
    si = lambda g: torch.sqrt(torch.sigmoid(g))
    g0, g1 = gamma_fn(0.0).double(), gamma_fn(1.0).double()
    exact = al(g0) * mu + (z1.double() - al(g1) * mu) * torch.sqrt(al(g0) ** 2 * sd ** 2 + si(g0) ** 2) / \
        torch.sqrt(al(g1) ** 2 * sd ** 2 + si(g1) ** 2)
    err = {}
    for sampler in ("ddim", "dpm2m"):
        for N in (16, 32, 64):
            z0 = sampling.sample(net_fn, gamma_fn, z1.clone(), mode, sampler, steps=N)
            err[sampler, N] = float(torch.sqrt(torch.mean((z0.double() - exact) ** 2)))
    for N in (16, 32):
        assert err["dpm2m", N] / err["dpm2m", 2 * N] >= 3.0, err
        assert err["ddim", N] / err["ddim", 2 * N] >= 1.7, err
    assert err["dpm2m", 32] < err["ddim", 64], err


# ----------------------------------------------------------------------------- whole models against the oracle
CASES = [("mulan_velocity", "vdm", False), ("mulan_epsilon", "ldm", False), ("mulan_velocity", "vdm", True), ("plain", "vdm", False)]


def _setup(vdm_type, unet_type, vfe, damp=None):
    from mulan_amd import model as M
    from mulan_amd.rng import PRNGKey
    if vdm_type == "plain":
        cfg, ocfg = make_cfg()
        cfg = dataclasses.replace(cfg, gamma_type="fixed", z_conditioning=False, reparam_type="input")
        ocfg = dict(ocfg, reparam_type="input")
        full = tr.init_params(ocfg, seed=4, dtype=torch.float64)
        ref_params = {"score_model": full["score_model"]}
        ref_params["score_model"]["dense0"]["kernel"] = ref_params["score_model"]["dense0"]["kernel"][:129].clone()
        vdm = M.make_vdm("vdm", cfg)
    else:
        cfg, ocfg = make_cfg(vdm_type, unet_type, vfe=vfe)
        ocfg = dict(ocfg, latent_size=50)
        ref_params = tr.init_params(ocfg, seed=5, dtype=torch.float64)
        vdm = M.make_vdm(vdm_type, cfg)
    if damp is not None:
        _damp(ref_params, damp)
    params = M.tree_map(lambda t: t.cuda(), vdm.init(PRNGKey(0)))
    M.from_flax_layout(M.tree_map(lambda t: t.detach().float(), ref_params), params)
    return vdm, params, ref_params, ocfg


def _oracle(vdm_type, ref_params, ocfg, z_init, grid, sampler):
    loop = fo.plain_fast_loop if vdm_type == "plain" else fo.mulan_fast_loop
    return run_oracle(lambda P, z_: loop(P, ocfg, z_, grid, sampler), ref_params, z_init.cpu().double())


def _ctx(vdm, params, B):
    cond = torch.zeros(B, dtype=torch.uint8, device="cuda")
    emb = vdm.deterministic_embedding(B, "cuda") if hasattr(vdm, "deterministic_embedding") else None
    return vdm.fast_context(params, emb, cond)


@pytest.mark.parametrize("vdm_type,unet_type,vfe", CASES)
def test_fast_samplers_match_the_oracle(vdm_type, unet_type, vfe):
    """4 steps of dpm2m (orders 1, 2, 2, 1) and of ddim: every step from the oracle's z_t and history against the
    oracle's z_s, with the budget of tests/test_gpu_sampler.py::_check_steps (2e-4 of max |net| x the step's
    d z_s / d net, which the oracle reports); then the loop run free from z_1 on a damped network, and the decoded
    images up to bin-edge ties"""
    from mulan_amd.rng import PRNGKey
    B, N = 2, 4
    grid = [1.0, 0.75, 0.5, 0.25, 0.0]
    z_init = PRNGKey(21).fold_in(1000).normal((B, 3072), "cuda")
    f32 = lambda t: torch.full((B,), float(np.float32(t)), device="cuda")
    vdm, params, ref_params, ocfg = _setup(vdm_type, unet_type, vfe)
    ctx = _ctx(vdm, params, B)
    for sampler in ("dpm2m", "ddim"):
        z_ref, x_ref, traj, hist, budget = _oracle(vdm_type, ref_params, ocfg, z_init, grid, sampler)
        orders = fo.orders(sampler, N)
        with torch.no_grad():
            for k in range(N):
                z_t = traj[k].reshape(B, -1).float().cuda()
                if orders[k] == 2:
                    g_p = vdm._fast_gamma(params, ctx, f32(grid[k - 1]))
                    x_p = hist[k][1].reshape(B, -1).float().cuda()
                else:
                    g_p = x_p = None
                zs, _, _ = vdm._fast_step(params, z_t, f32(grid[k]), f32(grid[k + 1]), g_p, x_p, ctx)
                err = np.abs(zs.cpu().double().numpy() - traj[k + 1].reshape(B, -1).numpy()).max()
                assert err < 2e-4 * budget[k] + 1e-5 * float(traj[k + 1].abs().max()), (sampler, k, err, budget[k])
            x = vdm.generate_x(params, z_ref.reshape(B, -1).float().cuda(), ctx.get("coeffs"))
        d = np.abs(x.cpu().numpy().astype(np.int64) - x_ref.numpy())
        assert x.dtype == torch.uint8 and d.max() <= 1 and (d != 0).mean() < 2e-3
    vdm, params, ref_params, ocfg = _setup(vdm_type, unet_type, vfe, damp=0.02)
    ctx = _ctx(vdm, params, B)
    for sampler in ("dpm2m", "ddim"):
        z_ref, x_ref, traj, hist, budget = _oracle(vdm_type, ref_params, ocfg, z_init, grid, sampler)
        z = vdm.fast_sample(params, z_init, ctx, sampler, N, graph=False)
        free = np.abs(z.cpu().double().numpy() - z_ref.reshape(B, -1).numpy()).max()
        assert free < 2e-4 * sum(budget) * 4 + 1e-5, (sampler, free, budget)
        d = np.abs(vdm.generate_x(params, z, ctx.get("coeffs")).cpu().numpy().astype(np.int64) - x_ref.numpy())
        assert d.max() <= 1, (sampler, d.max())
        # a disagreement only where a bin edge lies between the two latents (the end-point error checked above, over
        # a bin width of 2 / 256: about 1 % of the sub-pixels at this budget); g_0 = gamma_min for every model here
        a0 = np.sqrt(1 - 1 / (1 + np.exp(13.3)))
        zr, zp = z_ref.reshape(B, -1).numpy() / a0, z.cpu().double().numpy() / a0
        edge = np.abs((zr + 1) * 128 - np.round((zr + 1) * 128)) / 128
        bad = d.reshape(B, -1) != 0
        assert np.all(edge[bad] <= np.abs(zp - zr)[bad] + 1e-6) and bad.mean() < 0.05, (sampler, bad.mean())


def _config(vdm_type, unet_type, sm_n_layer=2):
    from mulan_amd.config import load_config_file
    config = load_config_file(os.path.join(ROOT, "ldm", "configs", "cifar10-conditioned.py"))
    config.vdm_type = vdm_type
    config.model.unet_type = unet_type
    config.data.dataset = 'synthetic'
    config.model.sm_n_layer = sm_n_layer
    config.model.forward_n_layer = 1
    config.training.batch_size_train = 4
    config.training.batch_size_eval = 4
    return config


def _experiment(vdm_type, unet_type, sm_n_layer=2):
    from mulan_amd.experiment import Experiment_VDM
    return Experiment_VDM(_config(vdm_type, unet_type, sm_n_layer))


def _randomise_ema(exp, seed):
    gen = torch.Generator(device="cuda").manual_seed(seed)
    with torch.no_grad():          # (zero-initialised layers would make the network output trivial)
        exp.state.ema.copy_(torch.randn(exp.state.ema.shape, device="cuda", generator=gen) * 0.03)


@pytest.mark.parametrize("graph", [False, True])
def test_reused_stepper_takes_the_next_batch_context(graph):
    """a stepper built for one batch and re-used for the next (eager: EagerFastStep, replayed: GraphedFastStep) samples
    under the NEW context: the same latent as a fresh stepper built for it; a context of another batch size and a
    stepper that cannot be re-targeted are refused"""
    from mulan_amd import sampling
    from mulan_amd.rng import PRNGKey
    exp = _experiment("mulan_velocity", "vdm", sm_n_layer=1)
    _randomise_ema(exp, 5)
    model, params, B, N = exp.model, exp.state.ema_params, 3, 4
    packer = exp.state.param_packer("ema")
    with torch.no_grad():
        if packer is not None:
            packer.refresh()
        cond = torch.zeros(B, dtype=torch.uint8, device="cuda")
        emb2 = torch.zeros((B, 50), device="cuda")
        emb2[:, 20:35] = 1.0
        ctx1 = model.fast_context(params, model.deterministic_embedding(B, exp.device), cond)
        ctx2 = model.fast_context(params, emb2, cond)
        z0 = PRNGKey(2).normal((B, 3072), exp.device)
        stepper = model.fast_stepper(params, B, exp.device, ctx1, graph=graph)
        assert type(stepper).__name__ == ("GraphedFastStep" if graph else "EagerFastStep")
        z1 = model.fast_sample(params, z0, ctx1, "dpm2m", N, stepper=stepper).clone()
        z2 = model.fast_sample(params, z0, ctx2, "dpm2m", N, stepper=stepper).clone()
        fresh = model.fast_sample(params, z0, ctx2, "dpm2m", N, graph=graph)
        assert torch.equal(z2, fresh) and not torch.equal(z1, z2)
        with pytest.raises(ValueError):
            stepper.set_context(model.fast_context(params, emb2[:1], cond[:1]))
        plain = sampling.EagerStepper(lambda z, t: z, lambda t: torch.zeros(B, device="cuda"), 1)
        with pytest.raises(TypeError):
            model.fast_sample(params, z0, ctx2, "dpm2m", N, stepper=plain)
        if packer is not None:
            packer.invalidate()


def test_sample_batches_draw_each_batch_from_its_key_alone(tmp_path, monkeypatch):
    """Experiment_Colab.sample_batches (the CLI's loop) with random embeddings: batches drawn together through one
    re-used stepper equal the same batches drawn one by one, replayed and eager; the ancestral path too"""
    from mulan_amd import checkpoint as ck, model as M
    from mulan_amd.evaluators import Experiment_Colab
    from mulan_amd.experiment import Experiment_VDM
    from mulan_amd.rng import PRNGKey
    exp = Experiment_VDM(_config("mulan_velocity", "vdm", 1))
    _randomise_ema(exp, 6)
    ck.save(str(tmp_path), exp.state.state_dict())
    del exp
    colab = Experiment_Colab(_config("mulan_velocity", "vdm", 1), str(tmp_path))
    keys = [PRNGKey(4).fold_in(b) for b in range(3)]
    for graph in (False, True):
        monkeypatch.setattr(M, "SAMPLER_GRAPH", graph)
        together = colab.sample_batches(keys, 2, "random", "dpm2m", 3)
        for k, x in zip(keys, together):
            assert x.shape == (2, 32, 32, 3) and x.dtype == torch.uint8
            assert torch.equal(x, colab.sample_batches([k], 2, "random", "dpm2m", 3)[0]), graph
        assert not torch.equal(together[0], together[1])
    anc = colab.sample_batches(keys[:2], 2, "random", "ancestral", 2)
    assert anc[1].shape == (2, 32, 32, 3) and anc[1].dtype == torch.uint8
    assert torch.equal(anc[1], colab.sample_batches(keys[1:2], 2, "random", "ancestral", 2)[0])


@pytest.mark.parametrize("vdm_type,unet_type", [("mulan_velocity", "vdm"), ("mulan_epsilon", "ldm")])
def test_replayed_fast_step_equals_the_eager_step(vdm_type, unet_type, monkeypatch):
    """model.GraphedFastStep (static buffers for z_t, t, s and the history; NaN history for first-order steps) against
    the eager stepper: the latent after every one of six dpm2m steps (orders 1, 2, 2, 2, 2, 1) is bit-identical, and
    Experiment_VDM.sample_fn(sampler='dpm2m') gives uint8 [B, 32, 32, 3], the same images with the replay on and off"""
    from mulan_amd import model as M, sampling
    from mulan_amd.rng import PRNGKey
    exp = _experiment(vdm_type, unet_type)
    _randomise_ema(exp, 3)
    model, params, B, N = exp.model, exp.state.ema_params, 5, 6
    packer = exp.state.param_packer("ema")
    with torch.no_grad():
        if packer is not None:
            packer.refresh()
        cond = torch.zeros(B, dtype=torch.uint8, device="cuda")
        ctx = model.fast_context(params, model.deterministic_embedding(B, exp.device), cond)
        z0 = PRNGKey(11).normal((B, 3072), exp.device)
        eager = model.fast_stepper(params, B, exp.device, ctx, graph=False)
        replay = model.fast_stepper(params, B, exp.device, ctx, graph=True)
        assert type(replay).__name__ == "GraphedFastStep"
        grid, orders = sampling.time_grid(N), sampling.step_orders("dpm2m", N)
        za, zb = z0.clone(), z0.clone()
        for k in range(N):
            za = eager(za, grid[k], grid[k + 1], orders[k])
            zb = replay(zb, grid[k], grid[k + 1], orders[k]).clone()
            assert torch.equal(za, zb), (k, float((za - zb).abs().max()))
        assert bool(torch.isfinite(za).all()) and float(za.std()) > 0
        # re-targeted at another batch's context, the captured stepper gives the eager result again
        emb2 = torch.zeros_like(ctx["emb"]); emb2[:, 20:35] = 1.0
        ctx2 = model.fast_context(params, emb2, cond)
        zc = model.fast_sample(params, z0, ctx2, "dpm2m", N, stepper=replay).clone()
        zd = model.fast_sample(params, z0, ctx2, "dpm2m", N, graph=False)
        assert torch.equal(zc, zd) and not torch.equal(zc, za)
        if packer is not None:
            packer.invalidate()
    dummy = torch.zeros(3, 32, 32, 3, dtype=torch.uint8, device="cuda")
    monkeypatch.setattr(M, "SAMPLER_GRAPH", True)
    a = exp.sample_fn(dummy_inputs=dummy, rng=PRNGKey(1), params=exp.state.ema_params, T=5, sampler='dpm2m')
    monkeypatch.setattr(M, "SAMPLER_GRAPH", False)
    b = exp.sample_fn(dummy_inputs=dummy, rng=PRNGKey(1), params=exp.state.ema_params, T=5, sampler='dpm2m')
    assert a.shape == (3, 32, 32, 3) and a.dtype == torch.uint8 and torch.equal(a, b)
    c = exp.sample_fn(dummy_inputs=dummy, rng=PRNGKey(1), params=exp.state.ema_params, sampler='ddim',
                      t_grid=[1.0, 0.6, 0.3, 0.0])
    assert c.shape == (3, 32, 32, 3) and c.dtype == torch.uint8
    with pytest.raises(ValueError):
        exp.sample_fn(dummy_inputs=dummy, rng=PRNGKey(1), params=exp.state.ema_params, sampler='dpm2m',
                      t_grid=[1.0, 0.6, 0.7, 0.0])


def test_sample_cli_writes_the_same_file_on_one_and_two_ranks(tmp_path):
    """python -m ldm.sample on a tiny checkpoint (saved as test_colab_front_end_samplers saves it): an npz of uint8
    [n_samples, 32, 32, 3]; with two ranks sharing the one GPU (gloo, as test_bench_ranks_share_one_gpu) the batches
    are dealt round-robin and the file is byte-identical to the one-rank file (replayed on one rank, eager on two)"""
    from mulan_amd import checkpoint as ck
    from mulan_amd.config import load_config_file
    from mulan_amd.experiment import Experiment_VDM
    over = ["--config.data.dataset=synthetic", "--config.model.sm_n_layer=1", "--config.model.forward_n_layer=1",
            "--config.training.batch_size_train=4", "--config.training.batch_size_eval=4", "--config.training.substeps=1"]
    c = load_config_file(os.path.join(ROOT, "ldm", "configs", "cifar10-conditioned.py"))
    for o in over:
        k, v = o[len("--config."):].split("=")
        c.set_path(k, v)
    exp = Experiment_VDM(c)
    gen = torch.Generator(device="cuda").manual_seed(8)
    with torch.no_grad():
        exp.state.ema.copy_(torch.randn(exp.state.ema.shape, device="cuda", generator=gen) * 0.03)
    ckdir = tmp_path / "ck"
    ck.save(str(ckdir), exp.state.state_dict())
    del exp
    args = [f"--config={os.path.join(ROOT, 'ldm', 'configs', 'cifar10-conditioned.py')}", *over,
            f"--checkpoint_directory={ckdir}", "--n_samples=5", "--batch_size=2", "--steps=3", "--embedding=random",
            "--seed=4"]
    env = {**os.environ, "MULAN_DIST_BACKEND": "gloo", "MULAN_FORCE_DEVICE": "0", "PYTHONPATH": ROOT}
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        env.pop(k, None)
    one, two = tmp_path / "one.npz", tmp_path / "two.npz"
    r = subprocess.run([sys.executable, "-m", "ldm.sample", *args, f"--out={one}"], capture_output=True, text=True,
                       timeout=400, env=env, cwd=ROOT)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    # the two ranks sample eagerly (MULAN_SAMPLER_GRAPH=0: the eager stepper re-used over each rank's batches, which
    # start at global batch 0 and 1); the eager step is the replayed one's bits, so the file is still the same
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
                        "--master-addr", "127.0.0.1", "--master-port", str(port), "-m", "ldm.sample", *args,
                        f"--out={two}"], capture_output=True, text=True, timeout=400,
                       env={**env, "MULAN_SAMPLER_GRAPH": "0"}, cwd=ROOT)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    z = np.load(one)
    assert z["images"].shape == (5, 32, 32, 3) and z["images"].dtype == np.uint8
    assert '"sampler": "dpm2m"' in str(z["settings"]) and z["images"].std() > 0
    assert one.read_bytes() == two.read_bytes()
