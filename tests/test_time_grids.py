"""CPU tests of the time grids of the few-step samplers: the keyword checks, the host grids, the binding of the two
schedule kernels, the float64 oracle (tests/grid_oracle.py) against itself, and the CLI's refusals."""
import os

import numpy as np
import pytest
import torch

from tests import grid_oracle as go

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONFIG = os.path.join(ROOT, "ldm", "configs", "cifar10-conditioned.py")


def test_check_grid_accepts_and_refuses():
    from mulan_amd import sampling
    assert sampling.GRIDS == ("uniform", "logsnr", "karras", "quadratic")
    for sampler in sampling.FAST_SAMPLERS:
        for grid in sampling.GRIDS:
            assert sampling.check_grid(sampler, grid, None, 7.0) == (grid, 7.0)
    assert sampling.check_grid("ancestral", "uniform", None, 7.0) == ("uniform", 7.0)
    assert sampling.check_grid("dpm2m", "uniform", [1.0, 0.5, 0.0], 3) == ("uniform", 3.0)
    assert sampling.check_grid("dpm2m") == ("uniform", 7.0)
    with pytest.raises(ValueError, match="unknown grid.*uniform, logsnr, karras, quadratic"):
        sampling.check_grid("dpm2m", "cosine", None, 7.0)
    for grid in ("logsnr", "karras", "quadratic"):
        with pytest.raises(ValueError, match="t_grid alone"):
            sampling.check_grid("dpm2m", grid, [1.0, 0.5, 0.0], 7.0)
        with pytest.raises(ValueError, match="ancestral.*grid = 'uniform'"):
            sampling.check_grid("ancestral", grid, None, 7.0)
    for rho in (0.0, -1.0, float("nan"), float("inf"), None, "seven"):
        with pytest.raises(ValueError, match="grid_rho must be a finite number > 0"):
            sampling.check_grid("dpm2m", "karras", None, rho)
    with pytest.raises(ValueError, match="unknown sampler"):
        sampling.check_grid("dpm3", "uniform", None, 7.0)


def test_uniform_and_quadratic_values():
    from mulan_amd import sampling
    for N in (1, 2, 7, 25, 64):
        i = np.arange(N + 1, dtype=np.float64)
        u = sampling.make_grid("uniform", N)
        assert u.dtype == np.float64 and np.array_equal(u, sampling.time_grid(N)) and np.array_equal(u, 1.0 - i / N)
        q = sampling.make_grid("quadratic", N)
        assert q.dtype == np.float64 and np.array_equal(q, (1.0 - i / N) ** 2)
        assert q[0] == 1.0 and q[-1] == 0.0 and np.all(np.diff(q) < 0)
    explicit = [1.0, 0.7, 0.2, 0.0]
    assert np.array_equal(sampling.make_grid("uniform", None, explicit), sampling.time_grid(None, explicit))
    with pytest.raises(ValueError, match="steps"):
        sampling.make_grid("quadratic", 0)
    with pytest.raises(ValueError, match="needs the schedule"):
        sampling.make_grid("logsnr", 8)


def test_make_grid_builds_on_a_schedule_and_names_a_collapsed_grid():
    """a linear gamma_bar: the logsnr grid is the uniform one, the karras grid follows its closed form; a schedule whose
    inverse returns two equal fp32 times is refused with the kind and N in the message"""
    from mulan_amd import sampling
    g0, g1 = -13.3, 5.0
    ends = lambda: (g0, g1)
    times = lambda tg: ((np.asarray(tg) - g0) / (g1 - g0)).astype(np.float32)
    for N in (1, 2, 9, 25):
        got = sampling.make_grid("logsnr", N, None, 7.0, ends, times)
        assert np.abs(got - sampling.time_grid(N)).max() <= 2.0 ** -24 and got[0] == 1.0 and got[-1] == 0.0
        k = sampling.make_grid("karras", N, None, 7.0, ends, times)
        want = (go.targets("karras", N, g0, g1, 7.0) - g0) / (g1 - g0)
        assert np.abs(k[1:-1] - want[1:-1]).max() <= 2.0 ** -23 if N > 1 else True
        assert np.array_equal(k[1:-1], times(sampling.grid_targets("karras", N, g0, g1, 7.0)).astype(np.float64))
    assert np.allclose(sampling.grid_targets("logsnr", 4, g0, g1), [g1 + (g0 - g1) * i / 4 for i in (1, 2, 3)], atol=1e-12)
    assert np.allclose(sampling.grid_targets("karras", 9, g0, g1, 3.0), go.targets("karras", 9, g0, g1, 3.0)[1:-1], atol=1e-12)
    flat = lambda tg: np.full(len(tg), 0.5, dtype=np.float32)
    with pytest.raises(ValueError, match="'logsnr' grid of 6 steps"):
        sampling.make_grid("logsnr", 6, None, 7.0, ends, flat)


def test_bisect_times_inverts_a_linear_schedule_in_fp32():
    from mulan_amd import sampling
    g0, g1 = -13.3, 5.0
    gamma = lambda t: g0 + (g1 - g0) * t
    tg = torch.tensor([g1, g0, g1 + 1.0, g0 - 1.0, -4.15, 0.0, 4.999], dtype=torch.float32)
    t = sampling.bisect_times(gamma, tg)
    assert t.dtype == torch.float32 and t[0] == 1.0 and t[1] == 0.0 and t[2] == 1.0 and t[3] == 0.0
    want = (tg.double() - g0) / (g1 - g0)
    assert float((t.double() - want)[4:].abs().max()) <= 2.0 ** -22      # fp32 rounding of gamma (18.3 x 2^-24) over its slope


def test_sample_refuses_a_schedule_grid_without_gamma_bar():
    from mulan_amd import sampling
    z = torch.zeros(1, 8)
    with pytest.raises(ValueError, match="gamma_bar_fn"):
        sampling.sample(lambda z, t: z, lambda t: z, z, 2, "dpm2m", steps=4, grid="logsnr")
    with pytest.raises(ValueError, match="t_grid alone"):
        sampling.sample(lambda z, t: z, lambda t: z, z, 2, "dpm2m", t_grid=[1.0, 0.0], grid="quadratic")
    with pytest.raises(ValueError, match="unknown grid"):
        sampling.sample(lambda z, t: z, lambda t: z, z, 2, "dpm2m", steps=4, grid="edm")


def test_binding_rows_of_the_schedule_kernels():
    from mulan_amd import lib
    assert lib.SIGNATURES["mulan_schedule_moments"] == [lib.P, lib.P, lib.P, lib.I, lib.I, lib.P, lib.P]
    assert lib.SIGNATURES["mulan_schedule_invert"] == [lib.P, lib.I, lib.P, lib.I, lib.D, lib.D, lib.P, lib.P]
    from mulan_amd import ops
    assert callable(ops.schedule_moments) and callable(ops.schedule_invert)


def test_every_public_layer_takes_the_keywords():
    import inspect
    from mulan_amd import evaluators, experiment, model, sampling
    fns = [sampling.sample, model._VDMBase.fast_sample, experiment.Experiment_VDM.sample_fn,
           experiment.Experiment_VDM.draw_samples, evaluators.Experiment_Colab.sample_conditionally,
           evaluators.Experiment_Colab.sample_randomly, evaluators.Experiment_Colab.sample_batches,
           evaluators.Experiment_Colab.inpaint, evaluators.Experiment_Colab.restore]
    for fn in fns:
        p = inspect.signature(fn).parameters
        assert p["grid"].default == "uniform" and p["grid_rho"].default == 7.0, fn
    assert inspect.signature(sampling.sample).parameters["gamma_bar_fn"].default is None
    for cls in (model.MulanVDM, model.PlainVDM):
        assert list(inspect.signature(cls.schedule_times).parameters) == ["self", "params", "ctx", "targets"]


# ------------------------------------------------------------------------------------------------------ the oracle
def _coefficients(seed, B, a_zero=False, b_zero=False):
    rng = np.random.default_rng(seed)
    a, b = rng.standard_normal((B, 3072)), rng.standard_normal((B, 3072))
    c = 1e-3 + np.log1p(np.exp(rng.standard_normal((B, 3072))))
    return a * (not a_zero), b * (not b_zero), c


def test_oracle_logsnr_grid_of_a_linear_schedule_is_uniform():
    a, b, c = _coefficients(3, 2, a_zero=True, b_zero=True)
    m = go.moments(a, b, c)
    assert np.abs(m - [1, 0, 0, 0, 0]).max() <= 1e-15
    for N in (1, 2, 9, 25, 64):
        assert np.abs(go.grid("logsnr", N, m) - go.grid("uniform", N)).max() <= 1e-12


@pytest.mark.parametrize("kind", ["logsnr", "karras"])
def test_oracle_roots_solve_the_schedule(kind):
    for seed, B in ((5, 1), (6, 3)):
        a, b, c = _coefficients(seed, B)
        m = go.moments(a, b, c)
        assert abs(m.mean(axis=0).sum() - 1.0) <= 1e-13                    # gamma_bar(1) = gamma_max
        for N in (2, 9, 25, 64):
            tg = go.targets(kind, N)
            t = go.grid(kind, N, m)
            assert t[0] == 1.0 and t[-1] == 0.0 and np.all(np.diff(t) < 0)
            assert np.abs(go.gamma_bar(m, t) - tg).max() <= 1e-10
    assert go.invert(m, [go.GAMMA_MAX, go.GAMMA_MIN, 9.0, -20.0]).tolist() == [1.0, 0.0, 1.0, 0.0]


def test_oracle_mean_schedule_is_the_mean_of_the_elements():
    model = go.random_model(seed=4, B=2, d=96)
    m = go.moments(model.a, model.b, model.c)
    for t in (0.0, 0.1, 0.5, 0.9, 1.0):
        assert abs(go.gamma_bar(m, t) - model.gamma(t).mean()) <= 1e-12


def test_oracle_samplers_converge_on_every_grid():
    """the orders the grids must not spoil: per doubling of N, ddim gains >= 1.7 and dpm2m >= 2.5 from 16 to 64 steps"""
    table = go.error_table(seed=11, Ns=(16, 32, 64))
    for kind in ("uniform", "logsnr"):
        e = table[kind, "ddim"]
        assert e[0] / e[1] >= 1.7 and e[1] / e[2] >= 1.7, (kind, e)
        e = table[kind, "dpm2m"]
        assert e[0] / e[1] >= 2.5 and e[1] / e[2] >= 2.5, (kind, e)


# --------------------------------------------------------------------------------------------------------- the CLI
def _base_args(tmp_path):
    return [f"--config={CONFIG}", f"--checkpoint_directory={tmp_path}", "--n_samples=4", f"--out={tmp_path}/s.npz"]


def test_sample_cli_checks_the_grid_before_the_device(tmp_path):
    from ldm import sample
    with pytest.raises(SystemExit, match="--grid.*ancestral"):
        sample.parse_flags(_base_args(tmp_path) + ["--grid=logsnr", "--sampler=ancestral"])
    with pytest.raises(SystemExit, match="--grid.*unknown grid"):
        sample.parse_flags(_base_args(tmp_path) + ["--grid=cosine"])
    with pytest.raises(SystemExit, match="grid_rho"):
        sample.parse_flags(_base_args(tmp_path) + ["--grid=karras", "--grid_rho=0"])
    (tmp_path / "ckpt-3").mkdir()
    flags, _ = sample.parse_flags(_base_args(tmp_path))
    assert flags.grid == "uniform" and flags.grid_rho == 7.0
    flags, _ = sample.parse_flags(_base_args(tmp_path) + ["--grid=karras", "--grid_rho=5"])
    assert flags.grid == "karras" and flags.grid_rho == 5.0
