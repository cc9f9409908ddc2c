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
