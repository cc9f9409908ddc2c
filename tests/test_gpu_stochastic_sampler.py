"""Stochastic few-step samplers (DDIM with eta, SDE-DPM-Solver++(2M); mulan_amd.sampling): the HIP step kernel against
float64 (tests/stochastic_sampler_oracle.py) and against the two kernels it meets at eta = 0 and eta = 1, its exact
cases, the law of the first-order sampler on a linear-Gaussian model, the whole models against the float64 oracle on
shared noise, the replayed stepper against the eager one, and the key law of sample_batches."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import stochastic_sampler_oracle as so
from tests.oracle_dev import run_oracle
from tests.test_gpu_fast_sampler import KINDS, _config, _ctx, _experiment, _inputs, _randomise_ema, _rel, _setup

ETAS = (0.0, 0.37, 1.0)


def _bar(mode):
    """the bar of test_fast_sampler_step_kernel for the same fp32 elementwise chain"""
    return 2e-5 if mode == 2 else 2e-6


def _dev(a):
    return torch.tensor(a).cuda()


def _xi(seed, shape):
    return np.random.default_rng(1000 + seed).standard_normal(shape).astype(np.float32)


# ---------------------------------------------------------------------------------- 1. the kernel against float64
@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("per_sample", [False, True])
@pytest.mark.parametrize("order", [1, 2])
def test_stochastic_sampler_step_kernel(mode, per_sample, order):
    from mulan_amd import ops
    B = 5
    zt, net, gt, gs, gp, xp = _inputs(7 + mode, B, per_sample)
    xi = _xi(mode, (B, 3072))
    d = lambda a: torch.tensor(a, dtype=torch.float64)
    g = (lambda a: d(a)[:, None]) if per_sample else d
    for eta in ETAS:
        hist = (_dev(gp), _dev(xp)) if order == 2 else (None, None)
        zs, x0 = ops.stochastic_sampler_step(_dev(zt), _dev(net), _dev(gt), _dev(gs), mode, _dev(xi), eta, *hist)
        ref, xref, _, _ = so.stochastic_step(d(zt), d(net), g(gt), g(gs), KINDS[mode], d(xi), eta,
                                             *((g(gp), d(xp)) if order == 2 else (None, None)))
        ez, ex = _rel(zs.cpu().numpy(), ref.numpy()), _rel(x0.cpu().numpy(), xref.numpy())
        print(f"mode {mode} per_sample {per_sample} order {order} eta {eta}: z_s {ez:.3g} x_hat {ex:.3g}")
        assert ez < _bar(mode) and ex < _bar(mode), (eta, ez, ex)
        if mode == 2:
            assert torch.equal(x0, _dev(net))


# ---------------------------------------------------------------------------------- 2. ragged and unaligned
@pytest.mark.parametrize("order", [1, 2])
@pytest.mark.parametrize("eta", ETAS)
def test_ragged_and_unaligned(order, eta):
    """n = 4099 with every buffer one float off the 16-byte grid: the scalar path, 17 blocks, the last one partial"""
    from mulan_amd import ops
    n = 4099
    rng = np.random.default_rng(5)
    base = [torch.tensor(rng.standard_normal(n + 1).astype(np.float32)).cuda() for _ in range(4)]
    zt, net, xp, xi = (b[1:] for b in base)
    gt_h = rng.uniform(-13.3, 5.0, n + 1).astype(np.float32)
    gt = torch.tensor(gt_h).cuda()[1:]
    gs = torch.tensor(gt_h - 0.3).cuda()[1:]
    gp = torch.tensor(gt_h + 0.4).cuda()[1:]
    assert all(t.data_ptr() % 16 == 4 for t in (zt, net, xp, xi, gt, gs, gp))
    hist = (gp, xp) if order == 2 else (None, None)
    zs, x0 = ops.stochastic_sampler_step(zt, net, gt, gs, 1, xi, eta, *hist)
    d = lambda t: t.cpu().double()
    ref, xref, _, _ = so.stochastic_step(d(zt), d(net), d(gt), d(gs), "epsilon", d(xi), eta,
                                         *((d(gp), d(xp)) if order == 2 else (None, None)))
    ez, ex = _rel(zs.cpu().numpy(), ref.numpy()), _rel(x0.cpu().numpy(), xref.numpy())
    print(f"order {order} eta {eta}: z_s {ez:.3g} x_hat {ex:.3g}")
    assert zs.shape == (n,) and ez < 2e-6 and ex < 2e-6


@pytest.mark.parametrize("per_sample", [False, True])
@pytest.mark.parametrize("order", [1, 2])
def test_float4_path_with_an_almost_empty_last_block(per_sample, order):
    """n = 4 * 256 * 3 + 4: 769 float4s, four blocks of which the last holds one thread's work"""
    from mulan_amd import ops
    n, rows, mode = 4 * 256 * 3 + 4, 769, 0                     # n = 769 * 4: per sample, every float4 has its gamma
    assert n % rows == 0 and (n // rows) % 4 == 0
    rng = np.random.default_rng(9)
    zt, net, xp, xi = (_dev(rng.standard_normal(n).astype(np.float32)) for _ in range(4))
    gshape = rows if per_sample else n
    gt_h = rng.uniform(-13.3, 5.0, gshape).astype(np.float32)
    gt, gs, gp = _dev(gt_h), _dev(gt_h - 0.3), _dev(gt_h + 0.4)
    if per_sample:
        zt, net, xp, xi = (t.view(rows, -1) for t in (zt, net, xp, xi))
    d = lambda t: t.cpu().double()
    g = (lambda t: d(t)[:, None]) if per_sample else d
    for eta in ETAS:
        hist = (gp, xp) if order == 2 else (None, None)
        zs, x0 = ops.stochastic_sampler_step(zt, net, gt, gs, mode, xi, eta, *hist)
        ref, xref, _, _ = so.stochastic_step(d(zt), d(net), g(gt), g(gs), KINDS[mode], d(xi), eta,
                                             *((g(gp), d(xp)) if order == 2 else (None, None)))
        ez, ex = _rel(zs.cpu().numpy(), ref.numpy()), _rel(x0.cpu().numpy(), xref.numpy())
        print(f"per_sample {per_sample} order {order} eta {eta}: z_s {ez:.3g} x_hat {ex:.3g}")
        assert zs.numel() == n and ez < _bar(mode) and ex < _bar(mode)


def test_entry_point_refuses_bad_arguments():
    """eta outside [0, 1] (NaN too), a NULL xi, and what mulan_fast_sampler_step refuses: hipErrorInvalidValue (1),
    before any launch"""
    from mulan_amd import lib
    h = lib.load()
    buf = torch.zeros(8, 16, device="cuda")
    p = lambda i: buf[i].data_ptr()
    good = [p(0), p(1), p(2), p(3), None, None, p(4), 0.5, p(5), p(6), 16, 1, 0, None]

    def rc(**kw):
        a = list(good)
        for k, v in kw.items():
            a[int(k[1:])] = v
        return h.mulan_stochastic_sampler_step(*a)
    assert rc() == 0
    for eta in (-0.01, 1.01, float("nan"), float("inf")):
        assert rc(a7=eta) == 1, eta
    assert rc(a6=None) == 1                                      # xi
    assert rc(a10=0) == 1 and rc(a11=3) == 1 and rc(a12=-1) == 1 and rc(a12=5) == 1      # n, mode, g_per_sample
    assert rc(a4=p(7)) == 1 and rc(a5=p(7)) == 1                 # half a history
    assert rc(a0=None) == 1 and rc(a8=None) == 1
    assert rc(a9=None) == 0                                      # x0 is optional
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------- 3. ties to the existing kernels
@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("per_sample", [False, True])
def test_ties_to_the_ancestral_and_the_deterministic_kernel(mode, per_sample):
    """eta = 1 at first order is ops.ancestral_step on the same noise, eta = 0 is ops.fast_sampler_step at both orders:
    within twice the bar of the kernel test, since each side carries that rounding against float64"""
    from mulan_amd import ops
    zt, net, gt, gs, gp, xp = (_dev(a) for a in _inputs(17 + mode, 5, per_sample))
    xi = _dev(_xi(3 + mode, (5, 3072)))
    z1, _ = ops.stochastic_sampler_step(zt, net, gt, gs, mode, xi, 1.0)
    anc = ops.ancestral_step(zt, net, gt, gs, xi, mode)
    e = _rel(z1.cpu().numpy(), anc.cpu().numpy())
    print(f"mode {mode} per_sample {per_sample}: ancestral tie {e:.3g}")
    assert e < 2 * _bar(mode)
    for hist in ((None, None), (gp, xp)):
        z0, x0 = ops.stochastic_sampler_step(zt, net, gt, gs, mode, xi, 0.0, *hist)
        zf, xf = ops.fast_sampler_step(zt, net, gt, gs, mode, *hist)
        e = _rel(z0.cpu().numpy(), zf.cpu().numpy())
        print(f"mode {mode} per_sample {per_sample} order {1 if hist[0] is None else 2}: deterministic tie {e:.3g}")
        assert e < 2 * _bar(mode) and _rel(x0.cpu().numpy(), xf.cpu().numpy()) < 2 * _bar(mode)


# ---------------------------------------------------------------------------------- 4. exact cases
@pytest.mark.parametrize("per_sample", [False, True])
def test_equal_gammas_return_z_exactly(per_sample):
    from mulan_amd import ops
    zt, net, gt, _, gp, xp = (_dev(a) for a in _inputs(3, 3, per_sample))
    xi = _dev(_xi(0, (3, 3072)))
    for eta in (0.0, 0.5, 1.0):
        for mode in (0, 1, 2):
            z1, _ = ops.stochastic_sampler_step(zt, net, gt, gt, mode, xi, eta)
            z2, _ = ops.stochastic_sampler_step(zt, net, gt, gt, mode, xi, eta, gp, xp)
            assert torch.equal(z1, zt) and torch.equal(z2, zt), (eta, mode)


@pytest.mark.parametrize("eta", [0.0, 0.5, 1.0])
def test_zero_previous_step_falls_back_to_first_order(eta):
    """an element whose previous step did not move its gamma (h_p = 0), or whose history is NaN: no NaN, and the
    first-order result bit for bit"""
    from mulan_amd import ops
    zt, net, gt, gs, gp, xp = _inputs(4, 4, False)
    gp[:, ::3] = gt[:, ::3]                          # h_p = 0
    gp[:, 1::7] = np.nan                             # no usable history
    xi = _dev(_xi(1, (4, 3072)))
    for mode in (0, 1, 2):
        z1, x1 = ops.stochastic_sampler_step(_dev(zt), _dev(net), _dev(gt), _dev(gs), mode, xi, eta)
        z2, x2 = ops.stochastic_sampler_step(_dev(zt), _dev(net), _dev(gt), _dev(gs), mode, xi, eta, _dev(gp), _dev(xp))
        assert bool(torch.isfinite(z2).all())
        fb = torch.tensor(~((gp - gt) > 0)).cuda()
        assert torch.equal(z2[fb], z1[fb]) and torch.equal(x1, x2)
        assert not torch.equal(z2[~fb], z1[~fb])


# ---------------------------------------------------------------------------------- 5. the law of the sampler
@pytest.mark.parametrize("mode", [1, 2])
@pytest.mark.parametrize("eta", [0.5, 1.0])
def test_law_on_a_linear_gaussian_model(mode, eta):
    """every coordinate x ~ N(mu, sd^2), per-sample gamma on a fixed linear schedule, the exact posterior mean as the
    network, z_1 ~ N(0, 1): every step is affine in z_t, so z_0 is Gaussian with the mean m and variance v that
    gaussian_law propagates in float64.  Over n = 64 x 3072 independent coordinates the empirical mean has standard
    deviation sqrt(v / n) and the empirical variance v sqrt(2 / n): both are held to five of those (the fp32 rounding
    of 16 steps, about 1e-6, is far below either)"""
    from mulan_amd import ops, sampling
    from mulan_amd.rng import PRNGKey
    B, N, mu, sd, gmin, gmax = 64, 16, 0.3, 0.5, -13.3, 5.0
    n = B * 3072
    key = PRNGKey(31).fold_in(mode)
    k_z, k_s = key.split(2)
    z1 = k_z.normal((B, 3072), "cuda")
    gamma32 = lambda t: float(np.float32(gmin + (gmax - gmin) * np.float64(np.float32(t))))

    def gamma_fn(t):
        return torch.full((B,), gamma32(t), device="cuda")

    def net_fn(z, t):
        g = gamma_fn(t).double()[:, None]
        x = so.posterior_mean(z.double(), g, mu, sd)
        al, si = torch.sqrt(torch.sigmoid(-g)), torch.sqrt(torch.sigmoid(g))
        return ((z.double() - al * x) / si if mode == 1 else x).float()

    noise_fn = lambda k: ops.randn((B, 3072), k_s.fold_in(k).v, 0, "cuda")
    z0 = sampling.sample(net_fn, gamma_fn, z1, mode, "ddim", steps=N, eta=eta, noise_fn=noise_fn).double()
    grid = sampling.time_grid(N)
    m, v = so.gaussian_law([gamma32(sampling.f32(t)) for t in grid], mu, sd, eta)
    em, ev = float(z0.mean()), float(z0.var(unbiased=True))
    print(f"mode {mode} eta {eta}: mean {em:.6f} (law {m:.6f}, 5 sd {5 * np.sqrt(v / n):.2g}), "
          f"variance {ev:.6f} (law {v:.6f}, 5 sd {5 * v * np.sqrt(2 / n):.2g})")
    assert abs(em - m) < 5 * np.sqrt(v / n)
    assert abs(ev - v) < 5 * v * np.sqrt(2 / n)


# ---------------------------------------------------------------------------------- 6. whole models, pathwise
MODELS = [("mulan_velocity", "vdm", False), ("mulan_epsilon", "ldm", False), ("plain", "vdm", False)]


@pytest.mark.parametrize("vdm_type,unet_type,vfe", MODELS)
def test_stochastic_samplers_match_the_oracle(vdm_type, unet_type, vfe):
    """sde2m over 4 steps (orders 1, 2, 2, 1) and ddim with eta = 0.5 over 3, the same xi per step on both sides: every
    step from the oracle's z_t and history against the oracle's z_s.  The budget is that of
    test_fast_samplers_match_the_oracle (2e-4 of max |net| x the step's d z_s / d net, which the oracle reports, plus
    1e-5 of the result) and, for the noise term, which carries no network error, the kernel test's bar of
    max |k_n xi|"""
    from mulan_amd import ops
    from mulan_amd.rng import PRNGKey
    B = 2
    z_init = PRNGKey(21).fold_in(1000).normal((B, 3072), "cuda")
    k_s = PRNGKey(22)
    f32 = lambda t: torch.full((B,), float(np.float32(t)), device="cuda")
    vdm, params, ref_params, ocfg = _setup(vdm_type, unet_type, vfe)
    ctx = _ctx(vdm, params, B)
    loop = so.plain_loop if vdm_type == "plain" else so.mulan_loop
    bar = _bar(vdm._fast_mode())
    for sampler, eta, N in (("sde2m", 1.0, 4), ("ddim", 0.5, 3)):
        grid = [1.0 - k / N for k in range(N + 1)]
        xis = [ops.randn((B, 3072), k_s.fold_in(k).v, 0, "cuda") for k in range(N)]
        z_ref, traj, hist, budget, noise = run_oracle(
            lambda P, z_, *xs: loop(P, ocfg, z_, grid, sampler, eta, xs), ref_params, z_init.cpu().double(),
            *[x.cpu().double() for x in xis])
        orders = so.orders(sampler, N)
        with torch.no_grad():
            for k in range(N):
                z_t = traj[k].reshape(B, -1).float().cuda()
                if orders[k] == 2:
                    g_p = vdm._fast_gamma(params, ctx, f32(grid[k - 1]))
                    x_p = hist[k][1].reshape(B, -1).float().cuda()
                else:
                    g_p = x_p = None
                zs, _, _ = vdm._fast_step(params, z_t, f32(grid[k]), f32(grid[k + 1]), g_p, x_p, ctx, xis[k], eta)
                err = np.abs(zs.cpu().double().numpy() - traj[k + 1].reshape(B, -1).numpy()).max()
                allowed = 2e-4 * budget[k] + 1e-5 * float(traj[k + 1].abs().max()) + bar * noise[k]
                print(f"{vdm_type} {sampler} step {k}: err {err:.3g} allowed {allowed:.3g} (noise max {noise[k]:.3g})")
                assert err < allowed, (sampler, k, err, budget[k], noise[k])
        assert max(noise) > 0.1                        # the noise took part


# ---------------------------------------------------------------------------------- 7. replay equals eager
@pytest.mark.parametrize("vdm_type,unet_type", [("mulan_velocity", "vdm"), ("plain", "vdm")])
@pytest.mark.parametrize("sampler,eta", [("sde2m", 0.0), ("ddim", 0.5)])
def test_replayed_stochastic_step_equals_the_eager_step(vdm_type, unet_type, sampler, eta):
    """model.GraphedFastStep with eta > 0 (xi one more static buffer, filled by the eager stepper's Philox call before
    each replay) against model.EagerFastStep: bit-identical after each of four steps; re-used for the next batch
    (context, latent and step key) it gives what a fresh stepper gives; a second-order step without history raises"""
    from mulan_amd import sampling
    from mulan_amd.rng import PRNGKey
    B, N = 2, 4
    vdm, params, _, _ = _setup(vdm_type, unet_type, False)
    ctx = _ctx(vdm, params, B)
    eff = sampling.check_eta(sampler, eta)
    grid, orders = sampling.time_grid(N), sampling.step_orders(sampler, N)
    k1, k2 = PRNGKey(5).split(2)
    z0 = PRNGKey(11).normal((B, 3072), "cuda")
    with torch.no_grad():
        eager = vdm.fast_stepper(params, B, "cuda", ctx, graph=False, step_eta=eff)
        replay = vdm.fast_stepper(params, B, "cuda", ctx, graph=True, step_eta=eff)
        assert type(eager).__name__ == "EagerFastStep" and type(replay).__name__ == "GraphedFastStep"
        for st in (eager, replay):
            with pytest.raises(RuntimeError):
                st(z0, grid[1], grid[2], 2, 1)                   # before set_noise or any history
            st.set_noise(k1)
            with pytest.raises(RuntimeError):
                st(z0, grid[1], grid[2], 2, 1)                   # second order without history
        za, zb = z0.clone(), z0.clone()
        for k in range(N):
            za = eager(za, grid[k], grid[k + 1], orders[k], k)
            zb = replay(zb, grid[k], grid[k + 1], orders[k], k).clone()
            assert torch.equal(za, zb), (k, float((za - zb).abs().max()))
        assert bool(torch.isfinite(za).all()) and float(za.std()) > 0
        # the noise is the key's: another step key, another path; fast_sample drives the same steps
        assert torch.equal(za, vdm.fast_sample(params, z0, ctx, sampler, N, graph=False, eta=eta, noise=k1))
        assert not torch.equal(za, vdm.fast_sample(params, z0, ctx, sampler, N, graph=False, eta=eta, noise=k2))
        # the next batch through the used steppers: what fresh ones give
        if "emb" in ctx:
            emb2 = torch.zeros_like(ctx["emb"]); emb2[:, 20:35] = 1.0
            ctx2 = vdm.fast_context(params, emb2, torch.zeros(B, dtype=torch.uint8, device="cuda"))
        else:
            ctx2 = vdm.fast_context(params, None, torch.ones(B, dtype=torch.uint8, device="cuda"))
        z2 = PRNGKey(12).normal((B, 3072), "cuda")
        zc = vdm.fast_sample(params, z2, ctx2, sampler, N, stepper=replay, eta=eta, noise=k2).clone()
        zd = vdm.fast_sample(params, z2, ctx2, sampler, N, stepper=eager, eta=eta, noise=k2)
        ze = vdm.fast_sample(params, z2, ctx2, sampler, N, graph=True, eta=eta, noise=k2)
        zf = vdm.fast_sample(params, z2, ctx2, sampler, N, graph=False, eta=eta, noise=k2)
        assert torch.equal(zc, ze) and torch.equal(zd, zf) and torch.equal(zc, zd) and not torch.equal(zc, za)
        with pytest.raises(ValueError):
            one = torch.zeros(1, dtype=torch.uint8, device="cuda")
            replay.set_context(vdm.fast_context(params, ctx["emb"][:1], one) if "emb" in ctx else {})
        with pytest.raises(ValueError):                          # a stepper serves the eta it was built for
            vdm.fast_sample(params, z2, ctx2, "dpm2m", N, stepper=replay)
        with pytest.raises(ValueError):                          # a stochastic run names its noise
            vdm.fast_sample(params, z2, ctx2, sampler, N, graph=False, eta=eta)


def test_sampler_graph_switch_runs_the_stochastic_step_eagerly(monkeypatch):
    """MULAN_SAMPLER_GRAPH=0 (model.SAMPLER_GRAPH): sample_fn with sde2m and with ddim, eta = 0.5, samples eagerly and
    gives the images of the replayed run; eta = 0 is today's ddim; a misplaced eta is refused"""
    from mulan_amd import model as M
    from mulan_amd.rng import PRNGKey
    exp = _experiment("mulan_velocity", "vdm", sm_n_layer=1)
    _randomise_ema(exp, 3)
    dummy = torch.zeros(3, 32, 32, 3, dtype=torch.uint8, device="cuda")
    kw = dict(dummy_inputs=dummy, rng=PRNGKey(1), params=exp.state.ema_params)
    out = {}
    for graph in (True, False):
        monkeypatch.setattr(M, "SAMPLER_GRAPH", graph)
        out[graph] = (exp.sample_fn(T=4, sampler='sde2m', **kw), exp.sample_fn(T=3, sampler='ddim', eta=0.5, **kw),
                      exp.sample_fn(T=3, sampler='ddim', eta=0.0, **kw), exp.sample_fn(T=3, sampler='ddim', **kw))
    for a, b in zip(out[True], out[False]):
        assert a.shape == (3, 32, 32, 3) and a.dtype == torch.uint8 and torch.equal(a, b)
    assert torch.equal(out[True][2], out[True][3]) and not torch.equal(out[True][1], out[True][2])
    for sampler in ('sde2m', 'dpm2m', 'ancestral'):
        with pytest.raises(ValueError, match="eta"):
            exp.sample_fn(T=3, sampler=sampler, eta=0.5, **kw)
    with pytest.raises(ValueError, match="eta"):
        exp.sample_fn(T=3, sampler='ddim', eta=1.5, **kw)
    exp.config.training.sampler = 'sde2m'
    exp.config.training.sample_timesteps = 3
    x = exp.p_sample(exp.state.ema_params)
    assert x.dtype == torch.uint8 and tuple(x.shape[1:]) == (32, 32, 3)


# ---------------------------------------------------------------------------------- 8. keys
def test_sample_batches_draw_each_batch_from_its_key_alone(tmp_path, monkeypatch):
    """Experiment_Colab.sample_batches with sde2m under random embeddings: batches drawn together through one re-used
    stepper equal the same batches drawn one by one, replayed and eager (ddim with eta = 0.5: replayed); two seeds
    differ"""
    from mulan_amd import checkpoint as ck, model as M
    from mulan_amd.evaluators import Experiment_Colab
    from mulan_amd.experiment import Experiment_VDM
    from mulan_amd.rng import PRNGKey
    exp = Experiment_VDM(_config("mulan_velocity", "vdm", 1))
    _randomise_ema(exp, 6)
    ck.save(str(tmp_path), exp.state.state_dict())
    del exp
    colab = Experiment_Colab(_config("mulan_velocity", "vdm", 1), str(tmp_path))
    keys = [PRNGKey(4).fold_in(b) for b in range(2)]
    first = {}
    for graph in (False, True):
        monkeypatch.setattr(M, "SAMPLER_GRAPH", graph)
        together = colab.sample_batches(keys, 2, "random", "sde2m", 3)
        for k, x in zip(keys, together):
            assert x.shape == (2, 32, 32, 3) and x.dtype == torch.uint8
            assert torch.equal(x, colab.sample_batches([k], 2, "random", "sde2m", 3)[0]), graph
        assert not torch.equal(together[0], together[1])
        first.setdefault("sde2m", together)
        assert all(torch.equal(a, b) for a, b in zip(first["sde2m"], together))          # eager = replayed
    together = colab.sample_batches(keys, 2, "random", "ddim", 3, 0.5)
    assert torch.equal(together[1], colab.sample_batches(keys[1:], 2, "random", "ddim", 3, 0.5)[0])
    assert not torch.equal(together[0], colab.sample_batches(keys[:1], 2, "random", "ddim", 3)[0])      # eta = 0
    other = colab.sample_batches([PRNGKey(5).fold_in(0)], 2, "random", "sde2m", 3)[0]
    assert not torch.equal(other, first["sde2m"][0])
    # the step noise matters: the same prior and embedding under dpm2m give other images
    assert not torch.equal(colab.sample_batches(keys[:1], 2, "random", "dpm2m", 3)[0], first["sde2m"][0])
    with pytest.raises(ValueError, match="eta"):
        colab.sample_batches(keys[:1], 2, "random", "sde2m", 3, 0.5)
