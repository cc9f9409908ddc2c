"""CPU tests of the latent maps (mulan_tsne_* / ops.tsne_* / mulan_amd.latent_maps / python -m ldm.latent_map): the
declarations and the binding rows, every refusal before any library call, PCA against sklearn, the float64 oracle's own
properties (row perplexities, a 500-iteration run on the planted set), the command line's flags and the animation.  The
kernels are held to the oracle in tests/test_gpu_tsne.py."""
import os
import re
import types

import numpy as np
import pytest
import torch

from tests import tsne_oracle as to

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONFIG = os.path.join(ROOT, "ldm", "configs", "cifar10-conditioned.py")


# ------------------------------------------------------------------------------------------------ the boundary
def test_header_declares_the_symbols_and_the_binding_table_binds_them():
    from mulan_amd import lib
    P, I, F, Z = lib.P, lib.I, lib.F, lib.Z
    want = {"mulan_tsne_workspace": [I], "mulan_tsne_affinities": [P, I, I, F, I, P, P, P],
            "mulan_tsne_gradient": [P, P, I, F, P, P, P, Z, P], "mulan_tsne_update": [P, P, P, P, I, F, F, P]}
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mulan_hip.h")).read(), flags=re.S)
    for name, row in want.items():
        assert lib.SIGNATURES[name] == row
        ret = "size_t" if name.endswith("workspace") else "int"
        m = re.search(rf"\b{ret}\s+{name}\s*\(([^;]*?)\)\s*;", src, flags=re.S)
        assert m and len(m.group(1).split(",")) == len(row), name
    assert lib._RESTYPES["mulan_tsne_workspace"] is lib.c_size_t
    assert "mulan_tsne_affinities" in open(os.path.join(ROOT, "INTEGRATION.md")).read()


def test_the_kernel_source_has_no_atomics_and_the_plain_gradient_no_logarithm():
    src = re.sub(r"//.*", "", open(os.path.join(ROOT, "mulan_amd", "csrc", "tsne.hip")).read())
    assert "atomic" not in src and "asm" not in src and "mfma" not in src
    body = src[src.index("void pair_term"):src.index("tsne_gradient_rows_kernel")]
    plain, guarded = body.split("if constexpr (KL)")
    assert "log" not in plain and "log(" in guarded
    from mulan_amd import ops
    assert (ops.TSNE_MIN_N, ops.TSNE_MAX_N) == (4, 16384) and "MAX_N = 16384" in src and "MIN_N = 4" in src
    assert f"MAX_STEPS = {to.MAX_STEPS}, BISECTIONS = {to.BISECTIONS}" in src


# ------------------------------------------------------------------------------------------------ refusals
def _no_library(monkeypatch):
    from mulan_amd import lib, ops

    def no_call(*a, **k):
        raise AssertionError("the library was called")
    monkeypatch.setattr(ops, "call", no_call)
    monkeypatch.setattr(ops, "stream", lambda: None)
    monkeypatch.setattr(lib, "load", no_call)
    monkeypatch.setattr(lib, "call", no_call)


def test_ops_argument_checks_come_before_any_library_call(monkeypatch):
    from mulan_amd import ops
    _no_library(monkeypatch)
    x = torch.zeros((12, 5))
    for bad, match in ((dict(x=x.double()), "fp32"), (dict(x=x[0]), "fp32"), (dict(x=x[:3]), "4 <= N"),
                       (dict(x=torch.zeros((16385, 1))), "N <= 16384"), (dict(x=torch.zeros((12, 0))), "D >= 1"),
                       (dict(perplexity=0.5), "perplexity"), (dict(perplexity=11), "perplexity"),
                       (dict(perplexity=float("nan")), "perplexity"), (dict(perplexity="5"), "perplexity"),
                       (dict(symmetrise=1), "symmetrise is a bool"), (dict(return_beta=0), "return_beta is a bool"),
                       (dict(x=x.numpy()), "tensor on the device"), (dict(), "tensor on the device")):
        kw = {**dict(x=x, perplexity=3.0), **bad}
        with pytest.raises(ValueError, match=match):
            ops.tsne_affinities(kw.pop("x"), **kw)
    P, Y = torch.zeros((12, 12)), torch.zeros((12, 2))
    ok = dict(P=P, Y=Y, U=Y.clone(), G=Y.clone(), exaggeration=12.0, momentum=0.5, lr=50.0)
    for bad, match in ((dict(P=torch.zeros((12, 11))), "P is fp32"), (dict(P=P.double()), "P is float32"),
                       (dict(P=torch.zeros((3, 3))), "P is fp32"), (dict(Y=torch.zeros((11, 2))), "Y is float32"),
                       (dict(U=Y.double()), "U is float32"), (dict(G=torch.zeros((2, 12)).t()), "G is contiguous"),
                       (dict(exaggeration=0), "exaggeration"), (dict(momentum=1.0), "momentum"), (dict(momentum=-0.1), "momentum"),
                       (dict(lr=0.0), "lr"), (dict(lr=float("inf")), "lr"), (dict(kl=1), "kl is float64"),
                       (dict(kl=torch.zeros(())), "kl is float64"), (dict(), "tensor on the device")):
        with pytest.raises(ValueError, match=match):
            ops.tsne_step(**{**ok, **bad})
    with pytest.raises(ValueError, match="tensor on the device"):
        ops.tsne_kl(P, Y)


def test_tsne_and_latent_map_refusals_come_before_any_library_call(monkeypatch):
    from mulan_amd import latent_maps as lm, model as M
    _no_library(monkeypatch)
    monkeypatch.setattr(torch.Tensor, "cuda", lambda *a, **k: (_ for _ in ()).throw(AssertionError("a device was asked for")))
    x = np.zeros((20, 5), dtype=np.float32)
    for bad, match in ((dict(data=x.astype(np.int32)), "float32 or float64"), (dict(data=x[0]), "float32 or float64"),
                       (dict(data=x[:3]), "4 <= N"), (dict(data=[[0.0]]), "float32 or float64"), (dict(perplexity=19), "perplexity"),
                       (dict(perplexity=0), "perplexity"), (dict(n_iter=0), "n_iter"), (dict(n_iter=2.5), "n_iter"),
                       (dict(exaggeration_iter=-1), "exaggeration_iter"), (dict(early_exaggeration=0), "early_exaggeration"),
                       (dict(learning_rate="fast"), "learning_rate"), (dict(learning_rate=-1.0), "learning_rate"),
                       (dict(init="spectral"), "init"), (dict(init=np.zeros((20, 3))), "init"), (dict(seed=-1), "seed"),
                       (dict(record_every=0), "record_every")):
        with pytest.raises(ValueError, match=match):
            lm.tsne(**{**dict(data=x, perplexity=5.0), **bad})
    assert lm.tsne_check(x, perplexity=5.0)[2] == 50.0 and lm.tsne_check(np.zeros((4800, 2), np.float32))[2] == 100.0
    assert lm.tsne_check(x, perplexity=5.0, learning_rate=7)[2] == 7.0
    with pytest.raises(ValueError, match="perplexity"):
        lm.plot_tsne_transformation(x, perplexities=(5, 25))
    for bad in ("pixels", "schedule:", "schedule:1.5", "schedule:x", 3):
        with pytest.raises(ValueError, match="on is"):
            lm.parse_on(bad)
    assert lm.parse_on("logits") == ("logits", None) and lm.parse_on("schedule:0.25") == ("schedule", 0.25)
    mulan = types.SimpleNamespace(model=types.SimpleNamespace(deterministic_embedding=None), world=2)
    plain = types.SimpleNamespace(model=object.__new__(M.PlainVDM))
    with pytest.raises(ValueError, match="MuLAN"):
        lm.latent_map(plain)
    with pytest.raises(ValueError, match="one process"):
        lm.latent_map(mulan)
    mulan.world = 1
    with pytest.raises(ValueError, match="on is"):
        lm.latent_map(mulan, on="pixels")
    with pytest.raises(ValueError, match="num_batches"):
        lm.latent_map(mulan, num_batches=0)


# ------------------------------------------------------------------------------------------------ PCA
def test_pca_transformation_equals_sklearn_signs_included(capsys):
    decomposition = pytest.importorskip("sklearn.decomposition")
    import sklearn
    from mulan_amd import latent_maps as lm
    x = np.random.default_rng(3).standard_normal((67, 50)) * np.linspace(3.0, 0.5, 50)
    pca = decomposition.PCA(n_components=4, svd_solver='full')
    want = pca.fit_transform(x)
    flip = "v" if tuple(int(v) for v in sklearn.__version__.split(".")[:2]) >= (1, 5) else "u"     # svd_flip's basis changed
    got, ratio, values = lm.pca_transformation(x, 4, return_stats=True, flip=flip)
    out = capsys.readouterr().out
    assert "variance ratio" in out and "singular values" in out
    assert np.abs(got - want).max() <= 1e-10
    assert np.abs(ratio - pca.explained_variance_ratio_).max() <= 1e-10 and np.abs(values - pca.singular_values_).max() <= 1e-10
    assert np.array_equal(lm.pca_transformation(x.astype(np.float32), 4, flip=flip), lm.pca_transformation(torch.tensor(x).float(), 4, flip=flip))
    other = lm.pca_transformation(x, 4, flip="u" if flip == "v" else "v")
    assert np.allclose(np.abs(other), np.abs(got), atol=1e-12)
    for bad in (0, 51, 2.0, True):
        with pytest.raises(ValueError, match="n_components"):
            lm.pca_transformation(x, bad)
    with pytest.raises(ValueError, match="not finite"):
        lm.pca_transformation(np.full((5, 3), np.nan))


def test_pca_init_is_the_oracles_and_has_the_stated_scale():
    from mulan_amd import latent_maps as lm
    x, _ = to.planted()
    y = lm.pca_init(x)
    assert y.dtype == np.float32 and y.shape == (96, 2) and np.array_equal(y, to.pca_init(x))
    assert abs(y[:, 0].std() / 1e-4 - 1) < 1e-6 and y[:, 1].std() < y[:, 0].std()
    assert (lm.pca_init(x[:, :1])[:, 1] == 0).all()
    with pytest.raises(ValueError, match="varies"):
        lm.pca_init(np.ones((8, 3)))


# ------------------------------------------------------------------------------------------------ the oracle
def test_oracle_row_perplexities_equal_the_request():
    x, _ = to.planted()
    for perplexity in (5.0, 10.0, 30.0):
        cond, beta = to.conditional_p(x, perplexity)
        assert np.abs(to.row_perplexity(cond) - perplexity).max() <= 1e-9
        assert (np.diag(cond) == 0).all() and np.abs(cond.sum(axis=1) - 1).max() <= 1e-14 and (beta > 0).all()
        joint = to.joint_p(cond)
        assert abs(joint.sum() - 1) <= 1e-14 and np.array_equal(joint, joint.T)
    b = to.affinity_bounds(x, 10.0)
    assert 0 < b["tol_P"] <= 1e-4 * b["joint"].max() and 0 < b["tol_beta"] < 1e-4
    assert to.affinity_bounds(x, 10.0) is b                                           # computed once


def test_oracle_gradient_is_the_derivative_of_its_kl():
    x, _ = to.planted()
    P = to.affinity_bounds(x, 10.0)["joint"]
    Y = np.random.default_rng(0).standard_normal((96, 2))
    grad, k = to.gradient(P, Y, 1.0)
    for i, c in ((0, 0), (17, 1), (95, 0)):
        h = np.zeros_like(Y)
        h[i, c] = 1e-6
        assert abs((to.kl(P, Y + h) - to.kl(P, Y - h)) / 2e-6 - grad[i, c]) <= 1e-8
    assert k == to.kl(P, Y) and k > 0


def test_oracle_long_run_separates_the_planted_clusters_and_ambiguous_updates_are_rare():
    from mulan_amd import latent_maps as lm
    x, labels = to.planted()
    P = to.affinity_bounds(x, 10.0)["joint"].astype(np.float32)
    run = to.run(P, lm.pca_init(x), 500, keep=(0, 100, 260, 499))
    print(f"KL {run['kl0']:.4f} -> {run['kl']:.4f}")
    assert to.purity(run["Y"], labels) == 1.0 and run["kl"] < run["kl0"] and run["kl"] < 0.25
    Y0, U0, G0 = run["states"][0]
    assert (U0 == 0).all() and (G0 == 1).all()
    for it, (Y, U, G) in run["states"].items():                       # update_bounds asserts the 1 % cap on its own
        ex, mom = (12.0, 0.5) if it < 250 else (1.0, 0.8)
        b = to.update_bounds(P, Y, U, G, ex, mom, 50.0)
        assert b["tol_Y"] > 0 and (~b["keep"]).mean() <= to.AMBIGUOUS_CAP
    first = to.update_bounds(P, Y0, U0, G0, 12.0, 0.5, 50.0)
    assert first["keep"].all() and (first["G"] == 0.8).all()


# ------------------------------------------------------------------------------------------------ CLI, animation
def _args(tmp_path, *more):
    return [f"--config={CONFIG}", f"--checkpoint_directory={tmp_path}", f"--out={tmp_path}/map.npz", *more]


def test_cli_flag_parsing(tmp_path, monkeypatch):
    from ldm import latent_map as cli
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    with pytest.raises(SystemExit, match="ckpt"):
        cli.parse_flags(_args(tmp_path))
    (tmp_path / "ckpt-3").mkdir()
    flags = cli.parse_flags(_args(tmp_path))
    assert (flags.num_batches, flags.on, flags.perplexity, flags.iters, flags.seed, flags.pca) == (30, "logits", 30.0, 1000, 0, 4)
    assert cli.parse_flags(_args(tmp_path, "--on=schedule:0.5", "--perplexity=12.5")).perplexity == 12.5
    for bad, what in (("--on=pixels", "on"), ("--on=schedule:2", "on"), ("--num_batches=0", "num_batches"),
                      ("--perplexity=0.5", "perplexity"), ("--iters=0", "iters"), ("--seed=-1", "seed"), ("--pca=0", "pca"),
                      ("--config.vdm_type=vdm", "MuLAN")):
        with pytest.raises(SystemExit, match=what):
            cli.parse_flags(_args(tmp_path, bad))
    with pytest.raises(SystemExit, match="npz"):
        cli.parse_flags(_args(tmp_path)[:-1] + [f"--out={tmp_path}/map.txt"])
    for missing in ("--config", "--checkpoint_directory", "--out"):
        with pytest.raises(SystemExit, match=missing.lstrip("-")):
            cli.parse_flags([a for a in _args(tmp_path) if not a.startswith(missing + "=")])
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(SystemExit, match="one process"):
        cli.parse_flags(_args(tmp_path))


def test_notebook_utils_exports_the_reference_names():
    import ldm.notebook_utils as nu
    from mulan_amd import latent_maps as lm
    for name in ("pca_transformation", "plot_tsne_transformation", "animate_scatter", "tsne", "latent_map"):
        assert getattr(nu, name) is getattr(lm, name)


def test_animate_scatter_returns_an_animation():
    matplotlib = pytest.importorskip("matplotlib")
    matplotlib.use("Agg")
    from matplotlib import animation
    import matplotlib.pyplot as plt
    from mulan_amd import latent_maps as lm
    rng = np.random.default_rng(0)
    xs, ys, cs = (list(rng.standard_normal((3, 20))) for _ in range(3))
    anim = lm.animate_scatter(xs, ys, cs)
    assert isinstance(anim, animation.FuncAnimation)
    anim._func(1)                                                      # a frame draws
    assert anim._fig.axes[0].get_title() == "60 k / 500k steps"
    plt.close(anim._fig)
    with pytest.raises(ValueError, match="per frame"):
        lm.animate_scatter(xs, ys[:2], cs)
