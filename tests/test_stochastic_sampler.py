"""Stochastic few-step samplers (DDIM with eta, SDE-DPM-Solver++(2M); mulan_amd.sampling): the C ABI entry point, the
order schedule, the eta checks, the flags of `python -m ldm.sample` and the float64 oracle
(tests/stochastic_sampler_oracle.py) against its known answers -- everything that runs without a GPU."""
import os
import re

import pytest
import torch

from tests import fast_sampler_oracle as fo
from tests import stochastic_sampler_oracle as so

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONFIG = os.path.join(ROOT, "ldm", "configs", "cifar10-conditioned.py")
ENTRY = "mulan_stochastic_sampler_step"


def test_header_declares_the_entry_point_and_the_binding_has_its_arity():
    from mulan_amd import lib
    with open(os.path.join(ROOT, "include", "mulan_hip.h")) as f:
        header = f.read()
    m = re.search(r"int\s+%s\s*\(([^;]*)\)\s*;" % ENTRY, header)
    assert m, f"{ENTRY} is not declared in include/mulan_hip.h"
    args = [a.strip() for a in m.group(1).split(",") if a.strip()]
    assert len(args) == 14 and args[7] == "float eta" and args[6] == "const float* xi"
    assert len(lib.SIGNATURES[ENTRY]) == 14 and lib.SIGNATURES[ENTRY][7] is lib.F


def test_the_entry_point_launches_an_exact_cover_grid():
    """one thread per element (or float4), no cap: the entry point stays out of the launch-cap table, whose members
    each need a case in tests/test_gpu_launch_geometry.py"""
    from tests.test_launch_geometry_table import capped_entry_points
    capped = capped_entry_points()
    assert ENTRY not in capped and "mulan_fast_sampler_step" in capped


def test_order_schedule_of_sde2m():
    from mulan_amd import sampling
    assert "sde2m" in sampling.SAMPLERS and sampling.check_sampler("sde2m") == "sde2m"
    assert sampling.step_orders("sde2m", 1) == [1]
    assert sampling.step_orders("sde2m", 2) == [1, 1]
    assert sampling.step_orders("sde2m", 4) == [1, 2, 2, 1]
    assert sampling.step_orders("sde2m", 14) == [1] + [2] * 12 + [1]        # lower order final below 15 steps
    assert sampling.step_orders("sde2m", 15) == [1] + [2] * 14
    for n in (1, 2, 4, 14, 15):
        assert sampling.step_orders("sde2m", n) == sampling.step_orders("dpm2m", n) == so.orders("sde2m", n)
    with pytest.raises(ValueError):
        sampling.step_orders("ancestral", 4)
    with pytest.raises(ValueError):
        sampling.check_sampler("dpm3")


@pytest.mark.parametrize("eta", [-0.1, 1.5, float("nan"), float("inf")])
def test_eta_outside_the_unit_interval_is_refused(eta):
    from mulan_amd import sampling
    with pytest.raises(ValueError, match="eta"):
        sampling.check_eta("ddim", eta)
    with pytest.raises(ValueError, match="eta"):
        sampling.sample(lambda z, t: z, lambda t: torch.zeros(1), torch.zeros(1, 4), 2, "ddim", steps=2, eta=eta,
                        noise_fn=lambda k: torch.zeros(1, 4))


@pytest.mark.parametrize("sampler", ["dpm2m", "ancestral", "sde2m"])
def test_eta_belongs_to_ddim(sampler):
    from mulan_amd import sampling
    with pytest.raises(ValueError, match="eta"):
        sampling.check_eta(sampler, 0.5)
    assert sampling.check_eta(sampler, 0.0) == (1.0 if sampler == "sde2m" else 0.0)
    assert sampling.check_eta("ddim", 0.25) == 0.25 and sampling.check_eta("ddim") == 0.0
    with pytest.raises(ValueError):
        sampling.check_eta("dpm3", 0.0)


def test_a_stochastic_run_needs_its_noise():
    from mulan_amd import sampling
    args = (lambda z, t: z, lambda t: torch.zeros(1), torch.zeros(1, 4), 2)
    with pytest.raises(ValueError, match="noise_fn"):
        sampling.sample(*args, "sde2m", steps=2)
    with pytest.raises(ValueError, match="noise_fn"):
        sampling.sample(*args, "ddim", steps=2, eta=0.5)


def _base_args(tmp_path):
    (tmp_path / "ckpt-3").mkdir(exist_ok=True)
    return [f"--config={CONFIG}", f"--checkpoint_directory={tmp_path}", "--n_samples=4", f"--out={tmp_path}/s.npz"]


def test_sample_cli_takes_the_new_sampler_and_eta(tmp_path):
    from ldm import sample
    flags, _ = sample.parse_flags(_base_args(tmp_path))
    assert flags.sampler == "dpm2m" and flags.eta == 0.0
    flags, _ = sample.parse_flags(_base_args(tmp_path) + ["--sampler=sde2m"])
    assert flags.sampler == "sde2m" and flags.eta == 0.0
    flags, _ = sample.parse_flags(_base_args(tmp_path) + ["--sampler=ddim", "--eta=0.5"])
    assert flags.sampler == "ddim" and flags.eta == 0.5
    flags, _ = sample.parse_flags(_base_args(tmp_path) + ["--sampler=ddim", "--eta=1"])
    assert flags.eta == 1.0


@pytest.mark.parametrize("args", [["--sampler=sde2m", "--eta=1.0"], ["--sampler=dpm2m", "--eta=0.5"], ["--eta=0.3"],
                                  ["--sampler=ancestral", "--eta=1"], ["--sampler=ddim", "--eta=1.01"],
                                  ["--sampler=ddim", "--eta=-0.5"], ["--sampler=ddim", "--eta=nan"]])
def test_sample_cli_refuses_a_misplaced_eta(tmp_path, args):
    from ldm import sample
    with pytest.raises(SystemExit, match="eta"):
        sample.parse_flags(_base_args(tmp_path) + args)


def test_notebook_default_step_count():
    from mulan_amd.evaluators import Experiment_Colab
    assert Experiment_Colab._steps(None, "sde2m") == 25 and Experiment_Colab._steps(9, "sde2m") == 9


# ------------------------------------------------------------------------------------- the oracle's known answers
KINDS = ("velocity", "epsilon", "input")


def _inputs(seed, per_sample, B=3, n=257):
    gen = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=gen, dtype=torch.float64)
    u = lambda lo, hi, *s: lo + (hi - lo) * torch.rand(*s, generator=gen, dtype=torch.float64)
    gshape = (B, 1) if per_sample else (B, n)
    z, net, xp, xi = r(B, n), r(B, n), r(B, n), r(B, n)
    gt = u(-13.3, 5.0, *gshape)
    return z, net, gt, gt - u(1e-3, 4.0, *gshape), gt + u(0.2, 1.0, *gshape), xp, xi


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("per_sample", [False, True])
def test_oracle_at_eta_zero_is_the_deterministic_step(kind, per_sample):
    z, net, gt, gs, gp, xp, xi = _inputs(1, per_sample)
    for hist in ((None, None), (gp, xp)):
        ref, xref, gain = fo.fast_step(z, net, gt, gs, kind, *hist)
        got, xh, g2, kn = so.stochastic_step(z, net, gt, gs, kind, xi, 0.0, *hist)
        assert torch.equal(xh, xref) and float(kn.max()) == 0.0
        assert float((got - ref).abs().max()) <= 1e-14 * float(ref.abs().max())
        assert float((g2 - gain).abs().max()) <= 1e-14 * float(gain.max())


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("per_sample", [False, True])
def test_oracle_at_eta_one_first_order_is_the_ancestral_step(kind, per_sample):
    z, net, gt, gs, _, _, xi = _inputs(2, per_sample)
    ref = so.ancestral_step(z, net, gt, gs, kind, xi)
    got = so.stochastic_step(z, net, gt, gs, kind, xi, 1.0)[0]
    # (mode 1 forms x_hat = (z - sigma net) / alpha with alpha down to 0.08: the two orders of evaluation differ by a
    # few float64 roundings of that quotient)
    assert float((got - ref).abs().max()) <= 1e-12 * float(ref.abs().max())


@pytest.mark.parametrize("eta", [0.0, 0.37, 0.5, 1.0])
def test_oracle_returns_z_at_equal_gammas(eta):
    for kind in KINDS:
        for per_sample in (False, True):
            z, net, gt, _, gp, xp, xi = _inputs(3, per_sample)
            assert torch.equal(so.stochastic_step(z, net, gt, gt, kind, xi, eta)[0], z)
            assert torch.equal(so.stochastic_step(z, net, gt, gt, kind, xi, eta, gp, xp)[0], z)


def test_oracle_second_order_at_eta_one_is_the_midpoint_form():
    """z_s = (sigma_s / sigma_t) e^(-h) z_t + alpha_s (1 - e^(-2h)) D + sigma_s sqrt(1 - e^(-2h)) xi"""
    z, net, gt, gs, gp, xp, xi = _inputs(4, False)
    xh = fo.x_hat(z, net, gt, "epsilon")
    h, hp = 0.5 * (gt - gs), 0.5 * (gp - gt)
    w = h / (2 * hp)
    d = (1 + w) * xh - w * xp
    al_s, si_s, si_t = torch.sqrt(torch.sigmoid(-gs)), torch.sqrt(torch.sigmoid(gs)), torch.sqrt(torch.sigmoid(gt))
    e2h = torch.exp(-2 * h)
    ref = si_s / si_t * torch.exp(-h) * z + al_s * (1 - e2h) * d + si_s * torch.sqrt(1 - e2h) * xi
    got = so.stochastic_step(z, net, gt, gs, "epsilon", xi, 1.0, gp, xp)[0]
    assert float((got - ref).abs().max()) <= 1e-12 * float(ref.abs().max())


def test_gaussian_law_is_the_step_applied_to_a_gaussian():
    """one step from a point mass at z (v = 0): the law's mean is the step without noise, its variance the square of
    what the step adds for xi = 1 -- the step of stochastic_step with the posterior mean as the network"""
    mu, sd = 0.3, 0.5
    d = lambda a: torch.tensor(a, dtype=torch.float64)
    for eta in (0.0, 0.5, 1.0):
        for g_t, g_s in ((5.0, 3.7), (-2.0, -2.4), (-9.0, -13.3)):
            for z in (-1.2, 0.0, 0.8):
                m, v = so.gaussian_law([g_t, g_s], mu, sd, eta, z, 0.0)
                net = so.posterior_mean(d(z), d(g_t), mu, sd)
                z0 = float(so.stochastic_step(d(z), net, d(g_t), d(g_s), "input", d(0.0), eta)[0])
                z1 = float(so.stochastic_step(d(z), net, d(g_t), d(g_s), "input", d(1.0), eta)[0])
                assert abs(m - z0) < 1e-13 and abs(v - (z1 - z0) ** 2) < 1e-13


def test_gaussian_law_keeps_the_exact_mean_at_eta_one():
    """started from the exact marginal N(alpha_1 mu, alpha_1^2 sd^2 + sigma_1^2), the ancestral step with the exact
    posterior mean keeps the mean of every earlier marginal, whatever the number of steps; its variance falls short of
    the marginal's (a point estimate of x carries none of the posterior's spread) and closes in as the steps shrink"""
    mu, sd = 0.3, 0.5
    al2 = lambda g: float(torch.sigmoid(torch.tensor(-g, dtype=torch.float64)))
    target = al2(-13.3) * sd ** 2 + 1 - al2(-13.3)
    gap = []
    for N in (1, 16, 256, 4096):
        gam = [-13.3 + 18.3 * (1 - k / N) for k in range(N + 1)]
        m, v = so.gaussian_law(gam, mu, sd, 1.0, al2(gam[0]) ** 0.5 * mu, al2(gam[0]) * sd ** 2 + 1 - al2(gam[0]))
        assert abs(m - al2(gam[-1]) ** 0.5 * mu) < 1e-12
        gap.append(target - v)
    assert gap[0] > gap[1] > gap[2] > gap[3] > 0 and gap[3] < gap[2] / 4
