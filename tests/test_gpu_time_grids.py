"""Time grids of the few-step samplers on the GPU: the two schedule kernels (mulan_schedule_moments,
mulan_schedule_invert) against float64 (tests/grid_oracle.py), the grids through the models' fast_sample, through
sampling.sample on the analytic model, and through the notebook front end.

Bounds.  A moment is a fixed-order fp32 sum of 3072 terms: (log2 3072 + 3) ~ 15 roundings of 2^-24, bound 2^-20, taken
relative to the mean of the absolute values where the terms change sign.  A root is judged in gamma, where the schedule
is flat a root may move in t without harm: the allowance is the rounding any fp32 time carries (the float64 root,
rounded) plus the moments' bound on the range."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import grid_oracle as go
from tests.test_gpu_fast_sampler import _config, _ctx, _randomise_ema, _setup

GMIN, GMAX = go.GAMMA_MIN, go.GAMMA_MAX
BOUND = 2.0 ** -20


def _coeffs(seed, B, family="unit"):
    """fp32 (a, b, c) [B, 3072]: random a, b and c = 1e-3 + softplus(randn); the same scaled by 1e3 / 1e-3; a = 0
    exactly (a freshly initialised model: dense_out_a is zero-initialised)"""
    rng = np.random.default_rng(seed)
    a, b = rng.standard_normal((B, 3072)), rng.standard_normal((B, 3072))
    c = 1e-3 + np.log1p(np.exp(rng.standard_normal((B, 3072))))
    s = {"unit": 1.0, "a0": 1.0, "ab0": 1.0, "1e3": 1e3, "1e-3": 1e-3}[family]
    a, b, c = (np.ascontiguousarray((v * s).astype(np.float32)) for v in (a, b, c))
    if family in ("a0", "ab0"):
        a[:] = 0.0
    if family == "ab0":
        b[:] = 0.0
    return a, b, c


def _dev(*arrays):
    return tuple(torch.from_numpy(v).cuda() for v in arrays)


# ------------------------------------------------------------------------------------------------- moments kernel
@pytest.mark.parametrize("family", ["unit", "1e3", "1e-3", "a0"])
@pytest.mark.parametrize("B", [1, 2, 3])
def test_schedule_moments_against_float64(B, family):
    """relative error per moment <= 2^-20 (mixed-sign moments: relative to the mean of the absolute ratios); two runs
    give the same bits; the five moments of the batch mean sum to 1 (gamma_bar(1) = gamma_max) to that bound"""
    from mulan_amd import ops
    a, b, c = _coeffs(40 + B, B, family)
    m = ops.schedule_moments(*_dev(a, b, c))
    again = ops.schedule_moments(*_dev(a, b, c))
    assert m.dtype == torch.float32 and tuple(m.shape) == (B, 5)
    assert torch.equal(m, again)
    got = m.cpu().double().numpy()
    r = go.ratios(a, b, c)                                   # float64 of the fp32 inputs
    ref, scale = r.mean(axis=1), np.abs(r).mean(axis=1)
    err = np.abs(got - ref)
    rel = np.where(scale > 0, err / np.where(scale > 0, scale, 1.0), err)
    total = abs(got.mean(axis=0).sum() - 1.0)
    print(f"moments B={B} {family}: max rel err {rel.max():.3e} (bound {BOUND:.3e}), |sum - 1| = {total:.3e}")
    assert np.all(err <= BOUND * scale), (rel.max(), BOUND)
    if family == "a0":
        assert np.all(got[:, 3:] == 0.0)
    assert total <= BOUND


def test_schedule_kernels_refuse_bad_arguments():
    from mulan_amd import ops
    from mulan_amd.lib import MulanHipError
    a, b, c = _dev(*_coeffs(1, 2))
    with pytest.raises(ValueError, match="3072"):
        ops.schedule_moments(a[:, :1024].contiguous(), b[:, :1024].contiguous(), c[:, :1024].contiguous())
    m = ops.schedule_moments(a, b, c)
    with pytest.raises(ValueError, match="no target"):
        ops.schedule_invert(m, np.zeros(0), GMIN, GMAX)
    with pytest.raises(ValueError, match=r"\[B, 5\]"):
        ops.schedule_invert(m[:, :4], [0.0], GMIN, GMAX)
    with pytest.raises(MulanHipError):
        ops.schedule_invert(m, [0.0], GMAX, GMIN)


# ----------------------------------------------------------------------------------------------- inversion kernel
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("M", [2, 9, 26, 65])
def test_schedule_invert_against_float64(M, B):
    """the targets of a logsnr and of a karras grid of M points, gamma_max and gamma_min themselves included (exactly 1
    and 0): max |gamma_bar64(t) - target| within the allowance of the module docstring; strictly decreasing times.
    Measured maximum over these cases: see the printed figures (DESIGN.md §3.7 records them)"""
    from mulan_amd import ops
    a, b, c = _coeffs(70 + B, B)
    m64 = go.moments(a, b, c)
    m = ops.schedule_moments(*_dev(a, b, c))
    for kind in ("logsnr", "karras"):
        tg = go.targets(kind, M - 1)
        tg[0], tg[-1] = GMAX, GMIN                          # (the karras end values round off gamma by an ulp)
        t = ops.schedule_invert(m, tg, GMIN, GMAX)
        assert t.dtype == torch.float32 and tuple(t.shape) == (M,)
        t = t.cpu().numpy()
        assert t[0] == np.float32(1.0) and t[-1] == np.float32(0.0)
        assert np.all(np.diff(t) < 0), t
        t_ref = go.invert(m64, tg).astype(np.float32).astype(np.float64)
        allowance = np.abs(go.gamma_bar(m64, t_ref) - tg).max() + (GMAX - GMIN) * BOUND
        miss = np.abs(go.gamma_bar(m64, t.astype(np.float64)) - tg).max()
        print(f"invert M={M} B={B} {kind}: max |gamma_bar64(t) - target| = {miss:.3e}, allowance {allowance:.3e}")
        assert miss <= allowance


@pytest.mark.parametrize("M", [2, 9, 26, 65])
def test_schedule_invert_of_a_linear_schedule_is_uniform(M):
    from mulan_amd import ops
    a, b, c = _coeffs(9, 2, "ab0")
    m = ops.schedule_moments(*_dev(a, b, c))
    t = ops.schedule_invert(m, go.targets("logsnr", M - 1), GMIN, GMAX).cpu().double().numpy()
    assert np.abs(t - go.grid("uniform", M - 1)).max() <= 2.0 ** -22


# -------------------------------------------------------------------------------------------------- sampler level
@pytest.fixture(scope="module")
def mulan():
    from mulan_amd.experiment import Experiment_VDM
    exp = Experiment_VDM(_config("mulan_velocity", "vdm"))
    _randomise_ema(exp, 3)
    return exp


def _mulan_ctx(exp, B, seed):
    """a context whose schedule is far from linear: random coefficients in place of the tiny model's own"""
    model, params = exp.model, exp.state.ema_params
    coeffs = _dev(*_coeffs(seed, B))
    cond = torch.zeros(B, dtype=torch.uint8, device="cuda")
    return model.fast_context(params, model.deterministic_embedding(B, exp.device), cond, coeffs=coeffs)


def _grid_of(model, params, ctx, kind, N, rho=7.0):
    from mulan_amd import sampling
    t = model.schedule_times(params, ctx, sampling.grid_targets(kind, N, *model.schedule_ends(params, ctx), rho))
    assert t.dtype == torch.float32 and t.is_cuda and tuple(t.shape) == (N - 1,)
    return np.concatenate([[1.0], t.cpu().double().numpy(), [0.0]])


@pytest.mark.parametrize("graph", [False, True])
def test_mulan_logsnr_run_is_the_run_on_its_grid(mulan, graph):
    """fast_sample(grid='logsnr') equals, bit for bit, fast_sample(t_grid=G) with G made of schedule_times; and the
    grid is not the uniform one"""
    from mulan_amd.rng import PRNGKey
    model, params, B, N = mulan.model, mulan.state.ema_params, 3, 6
    with torch.no_grad():
        ctx = _mulan_ctx(mulan, B, 17)
        z1 = PRNGKey(5).normal((B, 3072), "cuda")
        G = _grid_of(model, params, ctx, "logsnr", N)
        assert np.abs(G - go.grid("uniform", N)).max() > 1e-3
        assert np.array_equal(G, model.fast_grid(params, ctx, N, None, "logsnr"))
        a = model.fast_sample(params, z1, ctx, "dpm2m", N, graph=graph, grid="logsnr").clone()
        b = model.fast_sample(params, z1, ctx, "dpm2m", t_grid=G, graph=graph).clone()
        u = model.fast_sample(params, z1, ctx, "dpm2m", N, graph=graph).clone()
    assert torch.equal(a, b) and not torch.equal(a, u) and bool(torch.isfinite(a).all())


def test_plain_logsnr_and_karras_runs_are_the_runs_on_their_grids():
    """model_vdm.VDM with the fixed linear schedule: the bisection through _gamma gives the uniform grid back for
    'logsnr' up to fp32, another for 'karras'; each run equals the run on the explicit grid, bit for bit"""
    from mulan_amd.rng import PRNGKey
    vdm, params, _, _ = _setup("plain", "vdm", False)
    B, N = 2, 5
    with torch.no_grad():
        ctx = _ctx(vdm, params, B)
        z1 = PRNGKey(6).normal((B, 3072), "cuda")
        assert np.abs(np.subtract(vdm.schedule_ends(params, ctx), (vdm.config.gamma_min, vdm.config.gamma_max))).max() <= 1e-5
        for kind in ("logsnr", "karras"):
            G = _grid_of(vdm, params, ctx, kind, N)
            a = vdm.fast_sample(params, z1, ctx, "dpm2m", N, graph=False, grid=kind)
            b = vdm.fast_sample(params, z1, ctx, "dpm2m", t_grid=G, graph=False)
            assert torch.equal(a, b), kind
            if kind == "logsnr":
                assert np.abs(G - go.grid("uniform", N)).max() <= 2.0 ** -21
            else:
                assert np.abs(G - go.grid("uniform", N)).max() > 1e-2


def test_uniform_keyword_changes_no_bit(mulan):
    """grid='uniform' equals the call without the keyword: dpm2m, sde2m on the same noise key, an inpainting run"""
    from mulan_amd.rng import PRNGKey
    model, params, B, N = mulan.model, mulan.state.ema_params, 2, 4
    with torch.no_grad():
        ctx = _mulan_ctx(mulan, B, 18)
        z1 = PRNGKey(7).normal((B, 3072), "cuda")
        known = torch.rand(B, 3072, device="cuda") * 2 - 1
        mask = (torch.arange(3072, device="cuda") % 2 == 0).to(torch.uint8).expand(B, 3072).contiguous()
        for kw in (dict(sampler="dpm2m"), dict(sampler="sde2m", noise=PRNGKey(8)),
                   dict(sampler="sde2m", noise=PRNGKey(8), known=known, mask=mask, known_noise=PRNGKey(9), resample=2)):
            a = model.fast_sample(params, z1, ctx, steps=N, **kw).clone()
            b = model.fast_sample(params, z1, ctx, steps=N, grid="uniform", grid_rho=3.0, **kw).clone()
            assert torch.equal(a, b), kw["sampler"]
        with pytest.raises(ValueError, match="t_grid alone"):
            model.fast_sample(params, z1, ctx, "dpm2m", t_grid=[1.0, 0.5, 0.0], grid="logsnr")
        with pytest.raises(ValueError, match="unknown grid"):
            model.fast_sample(params, z1, ctx, "dpm2m", N, grid="cosine")


@pytest.mark.parametrize("mode", [0, 1, 2])
def test_convergence_on_the_analytic_model_on_a_logsnr_grid(mode):
    """the analytic Gaussian model of test_convergence_on_an_analytic_model, B = 2, sampling.sample on grid='logsnr' with
    gamma_bar_fn made of the moments kernel's output: dpm2m gains from N = 16 to 32 and 32 to 64 at least 0.85 x what
    the float64 oracle gains on the same inputs, ddim >= 1.7 x per doubling, and every error agrees with the oracle's
    error on the kernel's own grid (schedule_invert) to 5 %.  Nothing here ranks one grid against another."""
    from mulan_amd import ops, sampling
    B = 2
    gen = torch.Generator(device="cuda").manual_seed(11 + mode)
    r = lambda *s: torch.randn(*s, device="cuda", generator=gen)
    a, b = r(B, 3072), r(B, 3072)
    c = 1e-3 + torch.nn.functional.softplus(r(B, 3072))
    mu = (torch.rand(B, 3072, device="cuda", generator=gen) - 0.5).double()
    sd = (0.05 + 0.45 * torch.rand(B, 3072, device="cuda", generator=gen)).double()
    z1 = r(B, 3072)

    def gamma_fn(t):
        return ops.poly_gamma(a, b, c, torch.full((B,), t, device="cuda"), GMIN, GMAX)[2]

    def net_fn(z, t):
        g = gamma_fn(t).double()
        al, si = torch.sqrt(torch.sigmoid(-g)), torch.sqrt(torch.sigmoid(g))
        zd = z.double()
        x = mu + al * sd ** 2 * (zd - al * mu) / (al ** 2 * sd ** 2 + si ** 2)
        return {0: (al * zd - x) / si, 1: (zd - al * x) / si, 2: x}[mode].float()

    host = lambda t: t.cpu().double().numpy()
    model = go.GaussianModel(host(a), host(b), host(c), host(mu), host(sd), host(z1))
    exact = torch.from_numpy(model.exact()).cuda()
    m = ops.schedule_moments(a, b, c)
    m_host = host(m)
    gamma_bar_fn = lambda t: go.gamma_bar(m_host, t)
    err, ref = {}, {}
    for sampler in ("ddim", "dpm2m"):
        for N in (16, 32, 64):
            G = np.concatenate([[1.0], host(ops.schedule_invert(m, sampling.grid_targets("logsnr", N, GMIN, GMAX), GMIN, GMAX)),
                                [0.0]])
            G_host = sampling.make_grid("logsnr", N, None, 7.0, lambda: (GMIN, GMAX),
                                        lambda tg: go.invert(m_host, tg).astype(np.float32))
            assert np.abs(G - G_host).max() <= 2.0 ** -23                 # the kernel's roots are the float64 roots, rounded
            z0 = sampling.sample(net_fn, gamma_fn, z1.clone(), mode, sampler, steps=N, grid="logsnr",
                                 gamma_bar_fn=gamma_bar_fn)
            err[sampler, N] = float(torch.sqrt(torch.mean((z0.double() - exact) ** 2)))
            ref[sampler, N] = model.error(G, sampler)
            print(f"mode {mode} {sampler} N={N}: error {err[sampler, N]:.4e}, float64 oracle {ref[sampler, N]:.4e}")
    for key in err:
        assert abs(err[key] - ref[key]) <= 0.05 * ref[key], (key, err[key], ref[key])
    for N in (16, 32):
        assert err["dpm2m", N] / err["dpm2m", 2 * N] >= 0.85 * ref["dpm2m", N] / ref["dpm2m", 2 * N], (err, ref)
        assert err["ddim", N] / err["ddim", 2 * N] >= 1.7, err


# ------------------------------------------------------------------------------------------------------ front end
@pytest.fixture(scope="module")
def colab(mulan, tmp_path_factory):
    from mulan_amd import checkpoint as ck
    from mulan_amd.evaluators import Experiment_Colab
    d = tmp_path_factory.mktemp("grid_ckpt")
    ck.save(str(d), mulan.state.state_dict())
    return Experiment_Colab(_config("mulan_velocity", "vdm"), str(d))


def test_sample_batches_grid_comes_from_the_batch_alone(colab):
    """random embeddings, grid='logsnr', keys [k0, k1]: the images of k1 equal those of a call with [k1] alone"""
    from mulan_amd.rng import PRNGKey
    k0, k1 = PRNGKey(4).fold_in(0), PRNGKey(4).fold_in(1)
    both = colab.sample_batches([k0, k1], 2, "random", "dpm2m", 4, grid="logsnr")
    alone = colab.sample_batches([k1], 2, "random", "dpm2m", 4, grid="logsnr")[0]
    assert both[1].dtype == torch.uint8 and tuple(both[1].shape) == (2, 32, 32, 3)
    assert torch.equal(both[1], alone) and not torch.equal(both[0], both[1])
    with pytest.raises(ValueError, match="ancestral"):
        colab.sample_batches([k0], 2, "random", "ancestral", 4, grid="logsnr")
    grid = colab.sample_randomly(T=3, sampler="dpm2m", grid="karras", grid_rho=5.0)
    assert grid.dtype == np.uint8 and grid.size > 0


def test_inpaint_and_restore_take_a_grid(colab):
    """colab.inpaint(grid='karras') at N = 4 keeps the known pixels exactly; colab.restore('sr:4', grid='logsnr') leaves
    a residual within what the uniform grid leaves + 1 grey level"""
    from mulan_amd import sampling
    from mulan_amd.rng import PRNGKey
    images = torch.from_numpy(np.random.default_rng(1).integers(0, 256, (3, 32, 32, 3)).astype(np.uint8))
    keep = sampling.mask_from_spec("half:left")
    out = colab.inpaint(images, keep, steps=4, rng=PRNGKey(7), grid="karras")
    assert out.dtype == torch.uint8 and tuple(out.shape) == (3, 32, 32, 3)
    assert torch.equal(out.cpu()[:, :, :16], images[:, :, :16])
    assert not torch.equal(out.cpu(), colab.inpaint(images, keep, steps=4, rng=PRNGKey(7)).cpu())
    _, res_u = colab.restore(images=images, degradation="sr:4", steps=4, rng=PRNGKey(7))
    rest, res = colab.restore(images=images, degradation="sr:4", steps=4, rng=PRNGKey(7), grid="logsnr")
    print("residual (grey levels) sr:4, 4 steps: logsnr", res.cpu().numpy(), "uniform", res_u.cpu().numpy())
    assert rest.dtype == torch.uint8 and tuple(rest.shape) == (3, 32, 32, 3)
    assert bool((res <= res_u + 1.0).all())
