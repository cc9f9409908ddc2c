"""CPU side of the bound profile: the binding, the argument checks of ops.bound_profile, the float64 oracle of
tests/bound_profile_oracle.py against oracle.torch_ref.mulan_forward, the bounds the GPU tests hold the kernel to
(measured here from the fp32 restatement), the evaluator's host arithmetic over a stubbed model, the flags of
python -m ldm.bound_profile, the re-exports and the plot."""
import math
import os
import re
import types

import numpy as np
import pytest
import torch

from oracle import torch_ref as tr
from tests import bound_profile_oracle as bo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONFIG = os.path.join(ROOT, "ldm", "configs", "cifar10-conditioned.py")


# ------------------------------------------------------------------------------------------------ binding and ops
def test_header_declares_the_entry_with_the_arity_of_the_binding_table():
    from mulan_amd import lib
    P, I = lib.P, lib.I
    assert lib.SIGNATURES["mulan_bound_profile"] == [I, P, P, P, P, P, I, P, P, P, P, P, P, P, I, I, I, P]
    assert lib.SIGNATURES["mulan_bound_profile_workspace"] == [I, I]
    assert lib._RESTYPES["mulan_bound_profile_workspace"] is lib.c_size_t
    src = open(os.path.join(ROOT, "include", "mulan_hip.h")).read()
    for name in ("mulan_bound_profile", "mulan_bound_profile_workspace"):
        decl = re.search(r"\b(?:int|size_t) " + name + r"\(([^;]*)\);", src)
        assert decl, name
        assert len(decl.group(1).split(",")) == len(lib.SIGNATURES[name]), name
    assert os.path.exists(os.path.join(ROOT, "mulan_amd", "csrc", "bound_profile.hip"))
    import inspect
    from mulan_amd import ops
    assert list(inspect.signature(ops.bound_profile).parameters) == [
        "mode", "x", "g0", "g1", "gt", "w", "eps0", "eps", "zt", "net", "rows_per_group", "rows", "cols"]


def test_ops_argument_checks_come_before_any_library_call(monkeypatch):
    from mulan_amd import lib, ops

    def no_call(*a, **k):
        raise AssertionError("the library was called")
    monkeypatch.setattr(ops, "call", no_call)
    monkeypatch.setattr(lib, "load", no_call)
    B = 6
    x = torch.zeros((B, 3072), dtype=torch.uint8)
    w = torch.zeros((B, 3072))
    r = torch.zeros(B)
    ok = dict(mode=2, x=x, g0=w, g1=w, gt=w, w=w, eps0=w, eps=w, zt=w, net=w, rows_per_group=3)
    bad = [(dict(mode=3), "mode"), (dict(x=x.float()), "uint8"), (dict(x=x[:, :1024]), "uint8"), (dict(x=x[0]), "uint8"),
           (dict(eps=w.double()), "eps is an fp32"), (dict(net=w[:, :100]), "net is fp32"), (dict(zt=w[:4]), "zt is fp32"),
           (dict(g0=r), "all"), (dict(gt=r), "all"), (dict(w=w[:, :8]), "all"), (dict(g1=w.double()), "g1 is an fp32"),
           (dict(eps0=None), "eps0"), (dict(rows_per_group=4), "rows_per_group"), (dict(rows_per_group=0), "rows_per_group"),
           (dict(rows_per_group=-3), "rows_per_group"), (dict(rows=False, cols=False), "nothing asked")]
    for change, what in bad:
        with pytest.raises(ValueError, match=what):
            ops.bound_profile(**{**ok, **change})
    with pytest.raises(AssertionError, match="library was called"):        # a good call gets as far as the library
        ops.bound_profile(**{**ok, "g0": r, "g1": r, "gt": r, "w": r})


# ------------------------------------------------------------------------------------------------ oracle and bounds
@pytest.mark.parametrize("vdm_type,vfe,T,mode", [("mulan_epsilon", False, 0, 2), ("mulan_epsilon", False, 10, 2),
                                                ("mulan_velocity", False, 0, 0), ("mulan_velocity", True, 0, 1)])
def test_oracle_terms_sum_to_the_float64_model_losses(vdm_type, vfe, T, mode):
    """the per-element terms, fed the float64 model's own gammas, noise, z_t and network output, sum per row to its
    loss_recon, loss_klz (less the latent KL) and loss_diff"""
    ocfg = dict(vdm_type=vdm_type, n_embd=32, n_layer=1, forward_n_layer=1, latent_k=15, unet_type="vdm",
                velocity_from_epsilon=vfe, n_timesteps=T)
    params = tr.init_params(ocfg, seed=2, dtype=torch.float64)
    B = 2
    g = torch.Generator().manual_seed(4)
    x = torch.randint(0, 256, (B, 32, 32, 3), generator=g, dtype=torch.uint8)
    raw = torch.distributions.Gamma(1.0 / 15, 1.0).sample((10, B, 50)).double()
    e0, e = (torch.randn((B, 32, 32, 3), generator=g, dtype=torch.float64) for _ in range(2))
    t0 = 0.31
    with torch.no_grad():
        out = tr.mulan_forward(params, ocfg, x, t0, raw, e0, e)
        aux = out["aux"]
        a, b, c = tr.poly_coefficients(aux["emb"], params["gamma"])
        t = torch.remainder(t0 + torch.arange(B, dtype=torch.float64) / B, 1.)
        if T:
            t = torch.ceil(t * T) / T
        g0, g1 = tr.poly_gamma(a, b, c, torch.zeros(B, dtype=torch.float64)), tr.poly_gamma(a, b, c, torch.ones(B, dtype=torch.float64))
        gt = aux["g_t"].reshape(B, -1)
        w = aux["g_p"].reshape(B, -1) if not T else T * torch.expm1(gt - tr.poly_gamma(a, b, c, t - 1. / T))
        _, kl_z = tr.topk_embedding_and_loss(aux["logits"], raw, 15)
        terms = bo.terms64(mode, x.reshape(B, -1), g0, g1, gt, w, e0.reshape(B, -1), e.reshape(B, -1),
                           aux["z_t"].reshape(B, -1), aux["net"].reshape(B, -1))
    rows, cols = bo.rows_cols64(terms, 1, B)
    assert np.allclose(rows[:, 4], out["loss_recon"].numpy(), rtol=1e-12, atol=0)
    assert np.allclose(rows[:, 5], (out["loss_klz"] - kl_z).numpy(), rtol=1e-12, atol=0)
    assert np.allclose(rows[:, 0], out["loss_diff"].numpy(), rtol=1e-12, atol=0)
    assert np.allclose(rows[:, 1:4].sum(1), rows[:, 0], rtol=1e-12, atol=0)
    assert np.allclose(cols.sum(-1)[0], rows[:, [0, 4, 5]].mean(0), rtol=1e-12, atol=0)


@pytest.fixture(scope="module")
def measured():
    return bo.measure_errors()


def test_recorded_bounds_are_the_measured_errors(measured):
    """the literals of the oracle helper are the largest errors of the fp32 restatement over every case and mode, rounded
    up to two digits (so at most 10 % above): the restatement stays within a quarter of the GPU's bounds, which are 4 x"""
    for key, (r, c) in measured.items():
        print(key, "rows", " ".join(f"{v:.2e}" for v in r), "cols", " ".join(f"{v:.2e}" for v in c))
    assert set(k[:4] for k in measured) == set(bo.CASES) and len(measured) == 3 * len(bo.CASES)
    r = np.max([v[0] for v in measured.values()], axis=0)
    c = np.max([v[1] for v in measured.values()], axis=0)
    assert (r <= np.array(bo.MEASURED_ROWS)).all() and (np.array(bo.MEASURED_ROWS) <= 1.1 * r).all(), r
    assert (c <= np.array(bo.MEASURED_COLS)).all() and (np.array(bo.MEASURED_COLS) <= 1.1 * c).all(), c
    assert bo.ROWS_BOUND == tuple(4 * v for v in bo.MEASURED_ROWS) and bo.COLS_BOUND == tuple(4 * v for v in bo.MEASURED_COLS)
    assert (r <= np.array(bo.ROWS_BOUND) / 4).all() and (c <= np.array(bo.COLS_BOUND) / 4).all()


def test_cases_cover_the_issue_and_the_restatement_keeps_the_exact_zero():
    grs = {(G, R) for _, G, R, _ in bo.CASES}
    assert {(1, 1), (1, 7), (3, 5), (2, 17)} <= grs
    assert any(R % bo.CHUNK for _, _, R, _ in bo.CASES) and any(R > bo.CHUNK for _, _, R, _ in bo.CASES)
    assert {f for f, *_ in bo.CASES} == set(bo.FAMILIES) and {p for *_, p in bo.CASES} == {False, True}
    case = ("exact", 2, 17, False)
    i = bo.inputs(*case)
    assert np.array_equal(i["net2"], i["eps"]) and (i["x"].min(), i["x"].max()) == (0, 255)
    assert (bo.inputs("x0", 1, 7, False)["x"] == 0).all() and (bo.inputs("x255", 1, 7, False)["x"] == 255).all()
    rows, cols = bo.kernel_fp32(2, 2, 17, *(i[k] for k in ("x", "g0", "g1", "gt", "w", "eps0", "eps", "zt", "net2")))
    assert (rows[:, 0:4] == 0).all() and (rows[:, 6] == 0).all() and (cols[:, 0] == 0).all()
    # three channels that differ by a hundred times any bound: an i % 3 slip cannot pass
    r64, _ = bo.case64("uniform", 3, 5, False, 0)
    gaps = np.abs(r64[:, [1, 2, 3]] - r64[:, [2, 3, 1]]) / np.abs(r64[:, 1:4]).max()
    assert np.median(gaps) > 100 * max(bo.ROWS_BOUND)


# ------------------------------------------------------------------------------------------------ evaluator
def _stub_experiment(T, world=1, seen=None):
    """an experiment whose apply_fn returns a made-up profile: rows = image value + row index in every column"""
    def apply_fn(params, images, labels, conditioning, step, rngs, deterministic, profile_rows, **kw):
        assert deterministic and profile_rows == T and tuple(images.shape) == (T, 32, 32, 3)
        assert bool((images == images[0]).all()) and labels.shape == (T,) and conditioning.shape == (T,)
        if seen is not None:
            seen.append((step, kw, rngs["sample"].v))
        v = float(images[0, 0, 0, 0])
        rows = (v + torch.arange(T, dtype=torch.float32))[:, None] * torch.arange(1.0, 9.0)[None]
        cols = torch.arange(3 * 3072, dtype=torch.float32).reshape(1, 3, 3072) * (v + 1)
        return None, dict(rows=rows, cols=cols, kl_z=torch.full((T,), 2.0 * v), t=torch.arange(T, dtype=torch.float32) / T)
    state = types.SimpleNamespace(apply_fn=apply_fn, ema_params=object(), params=object())
    return types.SimpleNamespace(state=state, orig_params=object(), device=torch.device("cpu"), world=world, rank=0,
                                 model=types.SimpleNamespace(parameterization="epsilon"))


def test_evaluator_host_arithmetic_over_a_stubbed_model():
    from mulan_amd import evaluators as ev
    from mulan_amd.rng import PRNGKey
    T, seen = 4, []
    images = torch.zeros((2, 32, 32, 3), dtype=torch.uint8)
    images[1] = 3
    p = ev.bound_profile(_stub_experiment(T, seen=seen), images, n_timesteps=T, eval_step0=5)
    assert [s[0] for s in seen] == [5, 6] and all(s[1] == {"same_image": True} for s in seen)
    assert all(s[2] == PRNGKey(0).split()[1].v for s in seen)
    c = 1.0 / (3072 * math.log(2.0))
    base = np.array([[0, 1, 2, 3], [3, 4, 5, 6]], dtype=np.float64)
    for key, col in (("diff", 1), ("recon", 5), ("klz", 6)):
        assert p[key].shape == (2, T) and np.allclose(p[key], base * col * c, rtol=1e-14)
    assert p["diff_channel"].shape == (2, T, 3) and np.allclose(p["diff_channel"], base[..., None] * np.array([2, 3, 4]) * c)
    assert np.array_equal(p["resid2"], base * 7) and np.array_equal(p["weight"], base * 8)
    assert np.allclose(p["kl_z"], np.array([0.0, 6.0]) * c) and p["t"].shape == (2, T) and p["t"][1, 1] == 0.25
    assert np.allclose(p["bpd"], p["recon"].mean(1) + p["klz"].mean(1) + p["kl_z"] + p["diff"].mean(1), rtol=1e-14)
    assert np.allclose(p["bpd"], (np.array([1.5, 4.5]) * 12 + np.array([0.0, 6.0])) * c, rtol=1e-14)
    assert np.allclose(p["diff_std"], base.std(1) * c, rtol=1e-14) and p["diff_std"][0] > 0
    pix = np.arange(3 * 3072, dtype=np.float64).reshape(3, 3072) / math.log(2.0)
    for k, key in enumerate(("diff_pixel", "recon_pixel", "klz_pixel")):
        assert p[key].shape == (2, 3072) and np.allclose(p[key], np.stack([pix[k], 4 * pix[k]]), rtol=1e-14)
    assert all(isinstance(v, np.ndarray) for v in p.values())
    # a plain VDM takes no same_image
    exp = _stub_experiment(T, seen=seen)
    exp.model = types.SimpleNamespace()
    ev.bound_profile(exp, images[:1], n_timesteps=T)
    assert seen[-1][:2] == (0, {})


def test_pixel_maps_add_up_to_the_row_means():
    """diff_pixel.sum(1) / 3072 == diff.mean(1) whenever cols are the row means of terms whose row sums are rows"""
    from mulan_amd import evaluators as ev
    rng = np.random.default_rng(0)
    terms = rng.random((3, 5, 3072))                           # d, rho, kappa of five rows
    rows = np.zeros((5, 8))
    rows[:, 0], rows[:, 4], rows[:, 5] = terms[0].sum(1), terms[1].sum(1), terms[2].sum(1)
    p = ev._profile_arrays([dict(rows=rows, cols=terms.mean(1)[None], kl_z=np.zeros(5), t=np.zeros(5))])
    for pixel, row in (("diff_pixel", "diff"), ("recon_pixel", "recon"), ("klz_pixel", "klz")):
        assert np.allclose(p[pixel].sum(1) / 3072, p[row].mean(1), rtol=1e-13)


def test_evaluator_refusals():
    from mulan_amd import evaluators as ev
    images = torch.zeros((1, 32, 32, 3), dtype=torch.uint8)
    seen = []
    with pytest.raises(ValueError, match="one rank"):
        ev.bound_profile(_stub_experiment(4, world=2, seen=seen), images, n_timesteps=4)
    assert not seen
    for bad in (images.float(), images[0], images[:, :16], images[:0]):
        with pytest.raises(ValueError, match="uint8"):
            ev.bound_profile(_stub_experiment(4), bad, n_timesteps=4)
    with pytest.raises(ValueError, match="n_timesteps"):
        ev.bound_profile(_stub_experiment(4), images, n_timesteps=0)


def test_notebook_utils_reexports_the_evaluators_objects():
    from ldm import notebook_utils as nu
    from mulan_amd import evaluators as ev
    assert nu.bound_profile is ev.bound_profile and nu.plot_bound_profile is ev.plot_bound_profile


# ------------------------------------------------------------------------------------------------ CLI
def _args(tmp_path, *more):
    return [f"--config={CONFIG}", f"--checkpoint_directory={tmp_path}", f"--out={tmp_path}/p.npz", *more]


def test_cli_flag_parsing(tmp_path):
    from ldm import bound_profile as cli
    with pytest.raises(SystemExit, match="ckpt"):
        cli.parse_flags(_args(tmp_path))
    (tmp_path / "ckpt-3").mkdir()
    flags = cli.parse_flags(_args(tmp_path))
    assert (flags.n_images, flags.timesteps, flags.keep_pixels, flags.checkpoint) == (16, 128, 16, None)
    assert cli.parse_flags(_args(tmp_path, "--config.vdm_type=vdm")).config.vdm_type == "vdm"      # the baseline is accepted
    for bad, what in (("--n_images=0", "n_images"), ("--timesteps=0", "timesteps"), ("--keep_pixels=-1", "keep_pixels")):
        with pytest.raises(SystemExit, match=what):
            cli.parse_flags(_args(tmp_path, bad))
    with pytest.raises(SystemExit, match="npz"):
        cli.parse_flags(_args(tmp_path)[:-1] + [f"--out={tmp_path}/p.txt"])
    for missing in ("--config", "--checkpoint_directory", "--out"):
        with pytest.raises(SystemExit, match=missing.lstrip("-")):
            cli.parse_flags([a for a in _args(tmp_path) if not a.startswith(missing + "=")])


def test_cli_writes_the_documented_keys_with_the_device_calls_stubbed(tmp_path, monkeypatch):
    import json
    from ldm import bound_profile as cli
    from mulan_amd import evaluators as ev
    (tmp_path / "ckpt-3").mkdir()
    T, N = 4, 3

    class FakeExperiment:
        rank, world, device = 0, 1, torch.device("cpu")

        def __init__(self, config, directory, num):
            stub = _stub_experiment(T)
            self.state, self.orig_params, self.model, self.num = stub.state, stub.orig_params, stub.model, num

    images = torch.arange(5, dtype=torch.uint8).reshape(5, 1, 1, 1).expand(5, 32, 32, 3).contiguous()
    monkeypatch.setattr(ev, "Experiment_Colab", FakeExperiment)
    monkeypatch.setattr(cli, "eval_images", lambda experiment, config, n: images[:n])
    out = tmp_path / "p.npz"
    assert cli.main(_args(tmp_path, f"--n_images={N}", f"--timesteps={T}", "--keep_pixels=2")) == 0
    with np.load(out) as f:
        assert sorted(f.files) == sorted(cli.NPZ_KEYS)
        assert f["diff"].shape == (N, T) and f["diff_channel"].shape == (N, T, 3) and f["bpd"].shape == (N,)
        assert f["diff_pixel"].shape == (2, 3072) and f["diff_pixel_mean"].shape == (3072,)
        assert np.allclose(f["diff_pixel_mean"], np.arange(3072) * 2.0 / math.log(2.0))          # the mean of v + 1 is 2
        assert f["images"].dtype == np.uint8 and np.array_equal(f["images"], images[:N].numpy())
        settings = json.loads(str(f["settings"]))
    assert (settings["checkpoint"], settings["timesteps"], settings["n_images"], settings["keep_pixels"]) == ("3", T, N, 2)


# ------------------------------------------------------------------------------------------------ plot
def test_plot_draws_the_integrand_and_the_pixel_maps():
    pytest.importorskip("matplotlib")
    import matplotlib
    matplotlib.use("Agg")
    import matplotlib.pyplot as plt
    from mulan_amd import evaluators as ev
    rng = np.random.default_rng(2)
    N, T = 4, 6
    p = dict(t=rng.random((N, T)), diff=rng.random((N, T)), diff_channel=rng.random((N, T, 3)),
             diff_pixel=rng.random((N, 3072)), bpd=rng.random(N), diff_std=rng.random(N))
    try:
        figs = ev.plot_bound_profile(p)
        assert len(figs) == 3 and len(figs[0].axes) == 4 and len(figs[0].axes[0].lines) == 4
        x, y = figs[1].axes[0].lines[0].get_data()
        assert np.array_equal(x, np.sort(p["t"][1])) and np.array_equal(y, p["diff"][1][np.argsort(p["t"][1])])
        assert np.allclose(figs[2].axes[3].images[0].get_array(), p["diff_pixel"][2].reshape(32, 32, 3)[..., 2])
        assert len(ev.plot_bound_profile(p, count=1)) == 1
    finally:
        plt.close("all")
