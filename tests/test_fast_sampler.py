"""Deterministic few-step samplers (mulan_amd.sampling): the C ABI entry point, the time grid, the order schedule and the
flag checks of `python -m ldm.sample` -- everything that runs without a GPU."""
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONFIG = os.path.join(ROOT, "ldm", "configs", "cifar10-conditioned.py")


def test_header_declares_the_entry_point_and_the_binding_has_its_arity():
    from mulan_amd import lib
    with open(os.path.join(ROOT, "include", "mulan_hip.h")) as f:
        header = f.read()
    m = re.search(r"int\s+mulan_fast_sampler_step\s*\(([^;]*)\)\s*;", header)
    assert m, "mulan_fast_sampler_step is not declared in include/mulan_hip.h"
    n_args = len([a for a in m.group(1).split(",") if a.strip()])
    assert n_args == 12
    assert len(lib.SIGNATURES["mulan_fast_sampler_step"]) == n_args


def test_uniform_grid():
    from mulan_amd import sampling
    g = sampling.time_grid(4)
    assert np.array_equal(g, [1.0, 0.75, 0.5, 0.25, 0.0])
    assert sampling.time_grid(1).tolist() == [1.0, 0.0]
    g = sampling.time_grid(25)
    assert g.size == 26 and g[0] == 1.0 and g[-1] == 0.0 and np.all(np.diff(g) < 0)


@pytest.mark.parametrize("steps", [0, -3, 2.5, None])
def test_grid_rejects_a_step_count_below_one(steps):
    from mulan_amd import sampling
    with pytest.raises(ValueError):
        sampling.time_grid(steps)


@pytest.mark.parametrize("grid", [[1.0, 0.5, 0.5, 0.0], [1.0, 0.3, 0.6, 0.0], [0.9, 0.5, 0.0], [1.0, 0.5, 0.1],
                                  [1.0], [1.0, float("nan"), 0.0], [0.0, 0.5, 1.0], [1.0, 0.5 + 1e-12, 0.5, 0.0]])
def test_explicit_grid_validation(grid):
    from mulan_amd import sampling
    with pytest.raises(ValueError):
        sampling.time_grid(t_grid=grid)


def test_explicit_grid_accepted():
    from mulan_amd import sampling
    g = sampling.time_grid(t_grid=[1.0, 0.7, 0.2, 0.0])
    assert g.tolist() == [1.0, 0.7, 0.2, 0.0]
    assert sampling.time_grid(3, [1.0, 0.7, 0.2, 0.0]).tolist() == g.tolist()
    with pytest.raises(ValueError):
        sampling.time_grid(4, [1.0, 0.7, 0.2, 0.0])


def test_order_schedule():
    from mulan_amd import sampling
    assert sampling.step_orders("ddim", 5) == [1] * 5
    assert sampling.step_orders("dpm2m", 1) == [1]
    assert sampling.step_orders("dpm2m", 2) == [1, 1]
    assert sampling.step_orders("dpm2m", 4) == [1, 2, 2, 1]
    assert sampling.step_orders("dpm2m", 14) == [1] + [2] * 12 + [1]       # lower order final below 15 steps
    assert sampling.step_orders("dpm2m", 15) == [1] + [2] * 14
    assert sampling.step_orders("dpm2m", 25) == [1] + [2] * 24
    with pytest.raises(ValueError):
        sampling.step_orders("ancestral", 4)
    with pytest.raises(ValueError):
        sampling.step_orders("dpm2m", 0)
    with pytest.raises(ValueError):
        sampling.check_sampler("dpm3")


@pytest.mark.parametrize("sampler,N", [("dpm2m", 4), ("ddim", 3), ("dpm2m", 16), ("sde2m", 1)])
def test_run_asks_a_plain_stepper_for_the_steps_of_the_schedule(sampler, N):
    """sampling.run driven with a recording stepper that neither inpaints nor restores: N steps under the indices
    0 .. N - 1 at the schedule's orders, no mix and no jump; resample = 2 is refused"""
    import torch
    from mulan_amd import sampling
    from tests.test_inpaint import _Recorder
    f32 = lambda v: float(np.float32(v))
    grid, orders = sampling.time_grid(N), sampling.step_orders(sampler, N)
    rec = _Recorder(sampling.check_eta(sampler), inpaint=False, restore=False)
    z = torch.zeros(1, 4)
    assert sampling.run(rec, z, grid, orders) is z
    assert rec.log == [("step", orders[k], k, None, f32(grid[k]), f32(grid[k + 1])) for k in range(N)]
    with pytest.raises(ValueError, match=re.escape("resample applies to inpainting (a known image and a mask) and to "
                                                   "restoration (a measurement)")):
        sampling.run(rec, z, grid, orders, 2)
    assert len(rec.log) == N                                  # refused before any step


def test_a_stepper_refuses_the_runs_it_was_not_built_for():
    """the three refusals of a re-used stepper in fast_sample, on eager steppers built on the CPU (no launch)"""
    import types
    from mulan_amd import model as M
    build = lambda **kw: M.EagerFastStep(types.SimpleNamespace(_fast_mode=lambda: 1), None, 2, "cpu", {}, **kw)
    plain, sde, masked, sr4 = build(), build(step_eta=1.0), build(inpaint=True), build(restore="sr:4")
    assert plain.check_serves(0.0, False, None) is None and sde.check_serves(1.0, False, None) is None
    assert masked.check_serves(0.0, True, None) is None and sr4.check_serves(0.0, False, (4, False)) is None
    for stepper, args, text in (
            (plain, (1.0, False, None), "fast_sample: the stepper's steps run with eta = 0.0, this run asks for 1.0"),
            (sde, (0.5, True, None), "fast_sample: the stepper's steps run with eta = 1.0, this run asks for 0.5"),
            (plain, (0.0, True, None), "fast_sample: the stepper was built without a mask, this run comes with one"),
            (masked, (0.0, False, None), "fast_sample: the stepper was built with a mask, this run comes without one"),
            (plain, (0.0, False, (4, False)), "fast_sample: the stepper was built for no degradation, this run comes with "
                                              "the degradation (f, gray) = (4, False)"),
            (sr4, (0.0, False, (2, True)), "fast_sample: the stepper was built for the degradation (f, gray) = (4, False), "
                                           "this run comes with the degradation (f, gray) = (2, True)"),
            (sr4, (0.0, False, None), "fast_sample: the stepper was built for the degradation (f, gray) = (4, False), this "
                                      "run comes with no degradation")):
        with pytest.raises(ValueError, match="^" + re.escape(text) + "$"):
            stepper.check_serves(*args)


def _base_args(tmp_path):
    return [f"--config={CONFIG}", f"--checkpoint_directory={tmp_path}", "--n_samples=4", f"--out={tmp_path}/s.npz"]


def test_sample_cli_rejects_an_unknown_sampler(tmp_path):
    from ldm import sample
    with pytest.raises(SystemExit, match="sampler"):
        sample.parse_flags(_base_args(tmp_path) + ["--sampler=dpm3"])
    with pytest.raises(SystemExit, match="embedding"):
        sample.parse_flags(_base_args(tmp_path) + ["--embedding=uniform"])
    with pytest.raises(SystemExit, match="steps"):
        sample.parse_flags(_base_args(tmp_path) + ["--steps=0"])
    with pytest.raises(SystemExit, match="npz"):
        sample.parse_flags(_base_args(tmp_path)[:-1] + [f"--out={tmp_path}/s.png"])


@pytest.mark.parametrize("missing", ["--config", "--checkpoint_directory", "--n_samples", "--out"])
def test_sample_cli_rejects_a_missing_required_flag(tmp_path, missing):
    from ldm import sample
    args = [a for a in _base_args(tmp_path) if not a.startswith(missing + "=")]
    with pytest.raises(SystemExit, match=missing.lstrip("-")):
        sample.parse_flags(args)


def test_sample_cli_checks_the_checkpoint_directory_before_the_device(tmp_path):
    from ldm import sample
    with pytest.raises(SystemExit, match="ckpt"):
        sample.parse_flags(_base_args(tmp_path))
    (tmp_path / "ckpt-3").mkdir()
    flags, batch_size = sample.parse_flags(_base_args(tmp_path))
    assert flags.sampler == "dpm2m" and flags.steps == 25 and flags.embedding == "deterministic"
    assert batch_size == int(flags.config.training.batch_size_eval)


def test_notebook_samplers_default_step_counts():
    """sample_conditionally / sample_randomly without T: 1000 ancestral steps, 25 few-step steps (as p_sample)"""
    from mulan_amd.evaluators import Experiment_Colab
    assert Experiment_Colab._steps(None, "ancestral") == 1000
    assert Experiment_Colab._steps(None, "dpm2m") == 25 and Experiment_Colab._steps(None, "ddim") == 25
    assert Experiment_Colab._steps(7, "dpm2m") == 7
    with pytest.raises(ValueError):
        Experiment_Colab._steps(None, "dpm3")
