"""Inpainting with the few-step samplers (mulan_amd.sampling.run): the two C ABI entry points, the masks, the
refusals, the flags of `python -m ldm.sample` and the float64 oracle (tests/inpaint_oracle.py) against its known
answers -- everything that runs without a GPU."""
import os
import re

import numpy as np
import pytest
import torch

from tests import inpaint_oracle as io
from tests import stochastic_sampler_oracle as so

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONFIG = os.path.join(ROOT, "ldm", "configs", "cifar10-conditioned.py")


# ------------------------------------------------------------------------------------- the boundary
@pytest.mark.parametrize("entry,n_args,args", [
    ("mulan_inpaint_mix", 9, {2: "const unsigned char* mask", 4: "const float* xi", 5: "float* out", 6: "size_t n"}),
    ("mulan_forward_jump", 8, {3: "const float* xi", 4: "float* zt", 5: "size_t n", 6: "int g_per_sample"})])
def test_header_declares_the_entry_points_and_the_binding_has_their_arity(entry, n_args, args):
    from mulan_amd import lib
    with open(os.path.join(ROOT, "include", "mulan_hip.h")) as f:
        header = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    m = re.search(r"int\s+%s\s*\(([^;]*)\)\s*;" % entry, header)
    assert m, f"{entry} is not declared in include/mulan_hip.h"
    decl = [" ".join(a.split()) for a in m.group(1).split(",") if a.strip()]
    assert len(decl) == n_args and all(decl[i] == a for i, a in args.items()), decl
    assert len(lib.SIGNATURES[entry]) == n_args and lib.SIGNATURES[entry][-3] is lib.Z


def test_the_entry_points_launch_exact_cover_grids():
    """one thread per element (or float4), no cap: both stay out of the launch-cap table, whose members each need a
    case in tests/test_gpu_launch_geometry.py"""
    from tests.test_launch_geometry_table import capped_entry_points
    capped = capped_entry_points()
    assert "mulan_inpaint_mix" not in capped and "mulan_forward_jump" not in capped
    assert "mulan_fast_sampler_step" in capped


# ------------------------------------------------------------------------------------- the oracle's known answers
def _inputs(seed, per_sample, B=3, n=257):
    gen = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=gen, dtype=torch.float64)
    gshape = (B, 1) if per_sample else (B, n)
    g = -13.3 + 18.3 * torch.rand(*gshape, generator=gen, dtype=torch.float64)
    x = 2 * torch.rand(B, n, generator=gen, dtype=torch.float64) - 1
    mask = (torch.rand(B, n, generator=gen) < 0.5).to(torch.uint8)
    return r(B, n), x, mask, g, r(B, n)


@pytest.mark.parametrize("per_sample", [False, True])
def test_oracle_mix_known_answers(per_sample):
    z, x, mask, g, xi = _inputs(1, per_sample)
    assert torch.equal(io.mix(z, x, torch.zeros_like(mask), g, xi), z)                  # nothing known: the identity
    al, si = torch.sqrt(torch.sigmoid(-g)), torch.sqrt(torch.sigmoid(g))
    assert torch.equal(io.mix(z, x, torch.ones_like(mask), g, xi), al * x + si * xi)    # all known: q(z_t | x)
    assert torch.equal(io.mix(z, x, torch.ones_like(mask), g), al * x)                  # no noise: alpha x
    out = io.mix(z, x, mask, g, xi)
    assert torch.equal(out[mask == 0], z[mask == 0]) and torch.equal(out[mask != 0], (al * x + si * xi)[mask != 0])
    bad = torch.where(mask == 0, torch.full_like(x, float("nan")), x)                   # a select: nothing leaks
    assert torch.equal(io.mix(z, bad, mask, g, bad * 0 + xi), out)


@pytest.mark.parametrize("per_sample", [False, True])
def test_oracle_jump_known_answers(per_sample):
    z, _, _, g_s, xi = _inputs(2, per_sample)
    assert torch.equal(io.jump(z, g_s, g_s, xi), z)                                     # equal gammas: the identity
    g_t, g_u = g_s + 0.7, g_s + 2.9
    # s -> t -> u has the law of s -> u: the coefficients multiply, the variances compose to sigma_u^2 (1 - e^(g_s - g_u))
    (r1, v1), (r2, v2), (r, v) = (io.jump_coefficients(g_s, g_t), io.jump_coefficients(g_t, g_u),
                                  io.jump_coefficients(g_s, g_u))
    assert float((r1 * r2 - r).abs().max()) < 1e-14
    assert float(((r2 ** 2 * v1 + v2) / v - 1).abs().max()) < 1e-12
    assert float((v - torch.sigmoid(g_u) * (1 - torch.exp(g_s - g_u))).abs().max()) < 1e-14
    # the marginal q_s goes to q_t: alpha_s^2 r^2 = alpha_t^2 and sigma_s^2 r^2 + v = sigma_t^2
    assert float((torch.sigmoid(-g_s) * r1 ** 2 - torch.sigmoid(-g_t)).abs().max()) < 1e-14
    assert float((torch.sigmoid(g_s) * r1 ** 2 + v1 - torch.sigmoid(g_t)).abs().max()) < 1e-14


def test_oracle_jump_inverts_the_ancestral_posterior():
    """Bayes: q(z_s | z_t, x) q(z_t | x) = q(z_t | z_s) q(z_s | x).  For Gaussians with x fixed, the covariance of
    (z_s, z_t) built forwards (z_s from q_s, then the jump) equals the one built backwards (z_t from q_t, then the
    ancestral step with the true x, i.e. eps_hat = (z_t - alpha_t x) / sigma_t)"""
    d = lambda a: torch.tensor(a, dtype=torch.float64)
    for g_s, g_t in ((-3.0, -1.2), (-13.3, 5.0), (0.4, 0.5)):
        g_s, g_t = d(g_s), d(g_t)
        r, v = io.jump_coefficients(g_s, g_t)
        cov_fwd = torch.sigmoid(g_s) * r                                   # Cov(z_s, z_t | x) forwards
        # backwards: z_s = k z_t + (terms in x) + noise, k the z_t coefficient of the ancestral step with x known
        z0 = so.ancestral_step(d(0.0), d(0.0), g_t, g_s, "input", d(0.0))
        z1 = so.ancestral_step(d(1.0), d(0.0), g_t, g_s, "input", d(0.0))
        cov_bwd = (z1 - z0) * torch.sigmoid(g_t)
        assert abs(float(cov_fwd - cov_bwd)) < 1e-12


def test_gaussian_law_with_resampling_keeps_the_exact_marginal_mean():
    """started from the exact marginal mean at t = 1, the ancestral step (eta = 1) with the exact posterior mean keeps
    the marginal's mean at every time, and the jump maps the mean of q_s onto that of q_t: resampling leaves the mean
    of z_0 where it was; resample = 1 is so.gaussian_law"""
    mu, sd, N = 0.3, 0.5, 16
    al2 = lambda g: float(torch.sigmoid(torch.tensor(-g, dtype=torch.float64)))
    gam = [-13.3 + 18.3 * (1 - k / N) for k in range(N + 1)]
    start = (al2(gam[0]) ** 0.5 * mu, al2(gam[0]) * sd ** 2 + 1 - al2(gam[0]))
    assert io.inpaint_gaussian_law(gam, mu, sd, 1.0, 1, *start) == so.gaussian_law(gam, mu, sd, 1.0, *start)
    v = []
    for U in (1, 2, 5):
        m, vu = io.inpaint_gaussian_law(gam, mu, sd, 1.0, U, *start)
        assert abs(m - al2(gam[-1]) ** 0.5 * mu) < 1e-12
        v.append(vu)
    assert v[0] != v[1] != v[2]


def test_oracle_loop_order_of_operations():
    """the loop on a toy model: the events, their step indices and noise draws are those sampling.run states"""
    B, n, N = 1, 4, 3
    d = torch.float64
    gamma = lambda t: torch.full((B, 1), -13.3 + 18.3 * t, dtype=d)
    net_fn = lambda z, g: 0.5 * z
    x, mask = torch.full((B, n), 0.25, dtype=d), torch.tensor([[1, 0, 1, 0]], dtype=torch.uint8)
    grid = [1.0, 2 / 3, 1 / 3, 0.0]
    xi = lambda i: torch.full((B, n), 0.1 * (i + 1), dtype=d)
    z, ev = io.loop(gamma, net_fn, torch.ones(B, n, dtype=d), grid, "dpm2m", 0.0, "input", x, mask, None, xi, 1)
    assert [e["kind"] for e in ev] == ["mix", "step", "step", "step"]
    assert [e["j"] for e in ev] == [0, 0, 0, None] and [e["order"] for e in ev[1:]] == [1, 2, 1]
    a0 = torch.sqrt(torch.sigmoid(-gamma(0.0)))
    assert torch.equal(z[:, ::2], (a0 * x)[:, ::2])                              # the last mix takes no noise
    z, ev = io.loop(gamma, net_fn, torch.ones(B, n, dtype=d), grid, "sde2m", 1.0, "input", x, mask, xi, xi, 2)
    assert [e["kind"] for e in ev] == ["mix", "step", "jump", "step", "step", "jump", "step", "step"]
    assert [e["j"] for e in ev] == [0, 1, 2, 3, 4, 5, 6, None]
    assert [e.get("kk") for e in ev if e["kind"] == "step"] == [0, 3, 1, 4, 2]
    assert [e["order"] for e in ev if e["kind"] == "step"] == [1, 1, 2, 1, 1]
    assert torch.equal(z[:, ::2], (a0 * x)[:, ::2])


class _Recorder:
    """a stepper that computes nothing and writes down what the loop asks of it (tests/test_restore.py and
    tests/test_fast_sampler.py drive it as a restoring and as a plain stepper)"""

    def __init__(self, step_eta, inpaint=True, restore=False):
        self.step_eta, self.inpaint, self.restore, self.log = step_eta, inpaint, restore, []

    def mix(self, z, t, j):
        self.log.append(("mix", None, None, j, float(np.float32(t)), None))
        return z

    def jump(self, z, s, t, j):
        self.log.append(("jump", None, None, j, float(np.float32(t)), float(np.float32(s))))
        return z

    def __call__(self, z, t, s, order, k=None, mix=None):
        self.log.append(("step", order, k, mix, float(np.float32(t)), float(np.float32(s))))
        return z


@pytest.mark.parametrize("sampler,eta,U,N", [("dpm2m", 0.0, 1, 4), ("sde2m", 1.0, 2, 4), ("sde2m", 1.0, 3, 16),
                                             ("ddim", 0.0, 2, 3), ("ddim", 0.5, 1, 3), ("dpm2m", 0.0, 2, 15)])
def test_run_inpaint_asks_for_what_the_oracle_loop_does(sampler, eta, U, N):
    """sampling.run driven with a recording stepper: the sequence of operations with their order, step index,
    noise draw and times equals the events of the oracle's loop -- one eps (j = 0) throughout the deterministic run,
    consecutive draws otherwise, first order and the index k + r N on a repeated step, zero noise at the last mix"""
    from mulan_amd import sampling
    d = torch.float64
    gamma = lambda t: torch.full((1, 1), -13.3 + 18.3 * t, dtype=d)
    x, mask = torch.full((1, 4), 0.25, dtype=d), torch.tensor([[1, 0, 1, 0]], dtype=torch.uint8)
    xi = lambda i: torch.full((1, 4), 0.01 * (i + 1), dtype=d)
    grid = sampling.time_grid(N)
    _, ev = io.loop(gamma, lambda z, g: 0.5 * z, torch.ones(1, 4, dtype=d), list(grid), sampler, eta, "input", x, mask, xi,
                    xi, U)
    want = [(e["kind"], e.get("order"), e.get("kk"), sampling.ZERO_NOISE if (e["kind"] == "step" and e["j"] is None)
             else e["j"], e["t"], e.get("s")) for e in ev]
    rec = _Recorder(sampling.check_eta(sampler, eta if sampler == "ddim" else 0.0))
    z = torch.zeros(1, 4)
    assert sampling.run(rec, z, grid, sampling.step_orders(sampler, N), U) is z
    assert rec.log == want
    assert len([e for e in want if e[0] == "step"]) == N + (U - 1) * (N - 1)
    if eta == 0.0 and U == 1:
        assert {e[3] for e in want[:-1]} == {0}


# ------------------------------------------------------------------------------------- masks
def test_mask_specifications():
    from mulan_amd import sampling
    m = sampling.mask_from_spec("box:4,8,20,30")
    assert m.dtype == bool and m.shape == (32, 32) and not m[4:20, 8:30].any() and m.sum() == 1024 - 16 * 22
    for side, sl in (("left", np.s_[:, :16]), ("right", np.s_[:, 16:]), ("top", np.s_[:16]), ("bottom", np.s_[16:])):
        m = sampling.mask_from_spec(f"half:{side}")
        assert m[sl].all() and m.sum() == 512, side
    for bad in ("box:1,2,3", "box:a,b,c,d", "box:5,5,5,9", "box:0,0,33,4", "box:-1,0,4,4", "half:middle", "half", "disc:3",
                "", "box:1,2,3,4,5"):
        with pytest.raises(ValueError, match="mask"):
            sampling.mask_from_spec(bad)


def test_mask_broadcasting():
    from mulan_amd import sampling
    B = 3
    rng = np.random.default_rng(0)
    m2 = rng.random((32, 32)) < 0.5
    m3 = rng.random((B, 32, 32)) < 0.5
    m4 = (rng.random((B, 32, 32, 3)) < 0.5).astype(np.uint8) * 7              # non-zero = keep
    for m, want in ((m2, np.broadcast_to(m2[None, :, :, None], (B, 32, 32, 3))),
                    (m3, np.broadcast_to(m3[:, :, :, None], (B, 32, 32, 3))), (m4, m4 != 0)):
        for src in (m, torch.from_numpy(m)):
            out = sampling.expand_mask(src, B)
            assert out.dtype == torch.uint8 and tuple(out.shape) == (B, 3072) and out.is_contiguous()
            assert np.array_equal(out.numpy(), want.reshape(B, 3072).astype(np.uint8))
    for bad in (np.zeros((2, 32, 32), bool), np.zeros((B, 32, 32, 1), bool), np.zeros((32,), bool),
                np.zeros((B, 3072), bool)):
        with pytest.raises(ValueError, match="mask"):
            sampling.expand_mask(bad, B)
    with pytest.raises(ValueError, match="mask"):
        sampling.expand_mask(np.zeros((32, 32), np.float32), B)


# ------------------------------------------------------------------------------------- refusals
def test_ancestral_takes_no_mask():
    from mulan_amd import sampling
    x, m = torch.zeros(1, 4), torch.ones(1, 4, dtype=torch.uint8)
    with pytest.raises(ValueError, match="ancestral"):
        sampling.check_inpaint("ancestral", x, m)
    for sampler in sampling.FAST_SAMPLERS:
        assert sampling.check_inpaint(sampler, x, m, 2) is True
        assert sampling.check_inpaint(sampler, None, None) is False
    with pytest.raises(ValueError, match="together"):
        sampling.check_inpaint("dpm2m", x, None)
    with pytest.raises(ValueError, match="together"):
        sampling.check_inpaint("dpm2m", None, m)
    with pytest.raises(ValueError, match="resample"):
        sampling.check_inpaint("dpm2m", None, None, 2)


@pytest.mark.parametrize("resample", [0, 1.5, -1, True, float("nan")])
def test_resample_is_an_integer_from_one(resample):
    from mulan_amd import sampling
    x, m = torch.zeros(1, 4), torch.ones(1, 4, dtype=torch.uint8)
    with pytest.raises(ValueError, match="resample"):
        sampling.check_resample(resample)
    with pytest.raises(ValueError, match="resample"):
        sampling.sample(lambda z, t: z, lambda t: torch.zeros(1), torch.zeros(1, 4), 2, "dpm2m", steps=2, known=x, mask=m,
                        known_noise_fn=lambda j: x, resample=resample)
    assert sampling.check_resample(3) == 3 and sampling.check_resample(2.0) == 2


def test_an_inpainting_stepper_needs_all_three_and_mixes_every_step():
    from mulan_amd import sampling
    x, m = torch.zeros(1, 4), torch.ones(1, 4, dtype=torch.uint8)
    args = (lambda z, t: z, lambda t: torch.zeros(1), 2)
    with pytest.raises(ValueError, match="together"):
        sampling.EagerStepper(*args, known=x)
    with pytest.raises(ValueError, match="known_noise_fn"):
        sampling.EagerStepper(*args, known=x, mask=m)
    st = sampling.EagerStepper(*args, known=x, mask=m, known_noise_fn=lambda j: x)
    assert st.inpaint and not sampling.EagerStepper(*args).inpaint
    with pytest.raises(ValueError, match="mix"):
        st(x, 1.0, 0.5, 1, 0)                                   # no mix named
    with pytest.raises(ValueError, match="mix"):
        sampling.EagerStepper(*args)(x, 1.0, 0.5, 1, 0, 0)      # a mix where nothing is known


def _base_args(tmp_path):
    (tmp_path / "ckpt-3").mkdir(exist_ok=True)
    return [f"--config={CONFIG}", f"--checkpoint_directory={tmp_path}", f"--out={tmp_path}/s.npz"]


def _images(tmp_path, N=5, mask=None, name="in.npz"):
    rng = np.random.default_rng(3)
    arrays = dict(images=rng.integers(0, 256, (N, 32, 32, 3)).astype(np.uint8))
    if mask is not None:
        arrays["mask"] = mask
    np.savez(tmp_path / name, **arrays)
    return f"--inpaint_images={tmp_path / name}"


def test_sample_cli_takes_images_and_a_mask(tmp_path):
    from ldm import sample
    flags, _ = sample.parse_flags(_base_args(tmp_path) + [_images(tmp_path), "--mask=half:left", "--resample=2"])
    assert flags.n_samples is None and flags.resample == 2 and flags.sampler == "dpm2m"
    images, mask = sample.inpaint_inputs(flags)
    assert images.shape == (5, 32, 32, 3) and mask.shape == (5, 32, 32) and mask.dtype == bool
    assert mask[:, :, :16].all() and not mask[:, :, 16:].any()
    own = np.random.default_rng(1).random((5, 32, 32)) < 0.5
    flags, _ = sample.parse_flags(_base_args(tmp_path) + [_images(tmp_path, mask=own, name="own.npz"), "--n_samples=3",
                                                          "--embedding=encoder", "--sampler=sde2m"])
    assert flags.n_samples == 3 and np.array_equal(sample.inpaint_inputs(flags)[1], own)
    one = own[0].astype(np.uint8)
    flags, _ = sample.parse_flags(_base_args(tmp_path) + [_images(tmp_path, mask=one, name="one.npz")])
    assert np.array_equal(sample.inpaint_inputs(flags)[1], np.broadcast_to(own[0], (5, 32, 32)))
    flags, _ = sample.parse_flags(_base_args(tmp_path) + ["--n_samples=4"])             # as before
    assert flags.inpaint_images is None and flags.resample == 1 and sample.inpaint_inputs(flags) is None


def test_sample_cli_refusals(tmp_path):
    from ldm import sample
    base = _base_args(tmp_path)
    img = _images(tmp_path)
    own = _images(tmp_path, mask=np.ones((32, 32), bool), name="own.npz")
    bad_shape = _images(tmp_path, mask=np.ones((4, 32, 32), bool), name="bad.npz")
    np.savez(tmp_path / "noimages.npz", pictures=np.zeros((2, 32, 32, 3), np.uint8))
    for args, match in (
            (["--n_samples=4", "--mask=half:left"], "mask"),                      # a mask without images
            (["--n_samples=4", "--resample=2"], "resample"),
            ([], "n_samples"),                                                    # neither a count nor images
            ([img, "--mask=half:left", "--sampler=ancestral"], "ancestral"),
            ([img], "mask"),                                                      # no mask anywhere
            ([img, "--mask=half:middle"], "mask"),
            ([img, "--mask=box:1,2,3"], "mask"),
            ([img, "--mask=box:8,8,4,12"], "mask"),
            ([img, "--mask=half:left", "--resample=0"], "resample"),
            ([img, "--mask=half:left", "--n_samples=6"], "n_samples"),
            ([own, "--mask=half:left"], "mask"),                                  # two masks
            ([bad_shape], "mask"),
            ([f"--inpaint_images={tmp_path / 'noimages.npz'}", "--mask=half:top"], "images"),
            ([f"--inpaint_images={tmp_path / 'missing.npz'}", "--mask=half:top"], "cannot read"),
            (["--n_samples=4", "--embedding=encoder"], "embedding")):
        with pytest.raises(SystemExit, match=match):
            sample.parse_flags(base + args)
