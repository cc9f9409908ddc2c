"""CPU side of the noise-schedule analysis: the bounds tests/test_gpu_schedule_curves.py holds the kernel to (measured
here, from the fp32 restatement of tests/schedule_curves_oracle.py against float64), the seeds of its histogram test, the
binding, and the host functions around the kernel (get_embedding, heat_map_panels, Clustering, the argument checks, the
python -m ldm.schedules CLI, the plot wrappers)."""
import json
import os
import types

import numpy as np
import pytest
import torch

from tests import schedule_curves_oracle as sco

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONFIG = os.path.join(ROOT, "ldm", "configs", "cifar10-conditioned.py")


# ------------------------------------------------------------------------------------------------ bounds and oracles
@pytest.fixture(scope="module")
def measured():
    return sco.measure_errors()


def test_recorded_bounds_are_the_measured_errors(measured):
    """the named constants of the oracle helper are the largest errors of the fp32 restatement against float64 over the
    five families, rounded up to two digits (so at most 10 % above), and the GPU's bounds are 4 x those"""
    for name, (g, s) in measured.items():
        print(name, f"gamma {g:.3e}", " ".join(f"{n} {v:.3e}" for n, v in zip(sco.STAT_NAMES, s)))
    g = max(v[0] for v in measured.values())
    s = np.max([v[1] for v in measured.values()], axis=0)
    s[4:7] = s[4:7].max()
    assert g <= sco.MEASURED_GAMMA <= 1.1 * g, g
    assert (s <= np.array(sco.MEASURED_STATS)).all() and (np.array(sco.MEASURED_STATS) <= 1.1 * s).all(), s
    assert sco.GAMMA_BOUND == 4 * sco.MEASURED_GAMMA and sco.STATS_BOUND == tuple(4 * v for v in sco.MEASURED_STATS)


def test_restatement_keeps_the_exact_properties():
    """t = 0 gives gamma_min bit for bit with deviation 0 and min == max == mean; every histogram row holds 3072"""
    a, b, c = sco.family("normal", 2)
    t = sco.grid_times(7)
    g, s = sco.kernel_fp32(a, b, c, t)
    zero = t == 0
    assert zero.any() and (g[:, zero] == np.float32(sco.GMIN)).all()
    assert (s[:, zero, 1] == 0).all() and (s[:, zero, 0] == np.float32(sco.GMIN)).all()
    assert (s[:, zero, 2] == s[:, zero, 3]).all() and (s[:, zero, 2] == s[:, zero, 0]).all()
    for bins in (1, 100, 256):
        assert (sco.binning32(g, bins).sum(-1) == sco.D).all()
    lin = sco.kernel_fp32(*sco.family("linear", 1), t)[1][0]
    assert (np.abs(lin - sco.linear_closed_form(t)) <= np.array(sco.STATS_BOUND)).all()


def test_channel_family_tells_the_channels_apart():
    """the three channel means lie far further apart than any bound at t = 0.25: an i % 3 slip cannot pass"""
    t = sco.grid_times(7)
    ch = sco.stats_of(sco.gamma64(*sco.channel_family(3), t))[..., 4:7]
    mid = t == 0.25
    gaps = np.abs(ch[:, mid][..., [0, 1, 2]] - ch[:, mid][..., [1, 2, 0]])
    assert gaps.min() > 1.0 > 1000 * max(sco.STATS_BOUND), gaps.min()


@pytest.mark.parametrize("T", [7, 130])
def test_histogram_seeds_keep_clear_of_the_bin_edges(T):
    """the float64 oracle alone: with the seeds of the GPU's histogram test, in no row do more than 1 % of the sub-pixels
    lie within the gamma bound of an interior bin edge"""
    a, b, c = sco.family("normal", 3, seed=1)
    g = sco.gamma64(a, b, c, sco.grid_times(T))
    for bins in (1, 100, 256):
        near = sco.near_edge(g, bins, sco.GAMMA_BOUND)
        assert near.max() <= 0.01 * sco.D, (bins, int(near.max()))
        assert (sco.hist64(g, bins).sum(-1) == sco.D).all()
    assert sco.near_edge(g, 1, sco.GAMMA_BOUND).max() == 0


def test_binding_row_and_ops_entry():
    from mulan_amd import lib, ops
    P, I, F = lib.P, lib.I, lib.F
    assert lib.SIGNATURES["mulan_schedule_curves"] == [P, P, P, I, I, P, I, F, F, P, P, P, I, P]
    src = open(os.path.join(ROOT, "include", "mulan_hip.h")).read()
    assert "int mulan_schedule_curves(" in src
    assert os.path.exists(os.path.join(ROOT, "mulan_amd", "csrc", "schedule_curves.hip"))
    import inspect
    assert list(inspect.signature(ops.schedule_curves).parameters) == ["a", "b", "c", "t", "gmin", "gmax", "curves",
                                                                       "stats", "bins"]


def test_ops_argument_checks_need_no_device():
    from mulan_amd import ops
    a = torch.zeros(2, 3072)
    t = torch.zeros(4)
    with pytest.raises(ValueError, match="3072"):
        ops.schedule_curves(a[:, :1024], a[:, :1024], a[:, :1024], t, -13.3, 5.0)
    with pytest.raises(ValueError, match="fp32 \\[T\\]"):
        ops.schedule_curves(a, a, a, t.double(), -13.3, 5.0)
    with pytest.raises(ValueError, match="nothing asked"):
        ops.schedule_curves(a, a, a, t, -13.3, 5.0, curves=False)
    for bins in (0, 257):
        with pytest.raises(ValueError, match="bins"):
            ops.schedule_curves(a, a, a, t, -13.3, 5.0, bins=bins)
    with pytest.raises(ValueError, match="gmin < gmax"):
        ops.schedule_curves(a, a, a, t, 5.0, 5.0)


# ------------------------------------------------------------------------------------------------ host functions
def test_notebook_utils_reexports_the_schedule_surface():
    from ldm import notebook_utils as nu
    from mulan_amd import evaluators as ev
    for name in ("noise_schedule_per_embedding", "noise_schedule_summary", "get_embedding", "heat_map_panels",
                 "Clustering", "plot_noise_schedule", "plot_heat_map", "plot_histogram"):
        assert getattr(nu, name) is getattr(ev, name)


@pytest.mark.parametrize("B, L, shift", [(2, 50, 0), (3, 50, 7), (1, 64, 60), (2, 50, -3)])
def test_get_embedding_is_the_reference_roll(B, L, shift):
    from mulan_amd.evaluators import get_embedding
    emb = get_embedding(B, L, shift)
    want = np.roll(np.concatenate([np.ones((B, 15)), np.zeros((B, L - 15))], axis=1), shift=shift, axis=1)
    assert emb.dtype == torch.float32 and tuple(emb.shape) == (B, L)
    assert np.array_equal(emb.numpy(), want)
    assert np.array_equal(get_embedding().numpy(), np.concatenate([np.ones((2, 15)), np.zeros((2, 35))], axis=1))


def test_heat_map_panels_shape_range_and_constant_panel():
    from mulan_amd.evaluators import REC709, heat_map_panels
    rng = np.random.default_rng(0)
    ns = rng.standard_normal((20, 3072))
    ns[0] = -13.3                                                        # t = 0: a constant panel
    p = heat_map_panels(ns)
    assert p.shape == (10, 28, 28) and np.isfinite(p).all()
    assert (p[0] == 0).all() and p.min() >= 0 and p.max() <= 1 + 1e-12
    # panel k is row int(T k / cols), cropped, min-max normalised, Rec. 709 luminance
    k = 3
    img = ns[int(20 * k / 10)].reshape(32, 32, 3)[2:-2, 2:-2]
    img = (img - img.min()) / (img.max() - img.min())
    assert np.allclose(p[k], img @ np.array([0.2125, 0.7154, 0.0721]), atol=1e-14) and REC709 == (0.2125, 0.7154, 0.0721)
    assert heat_map_panels(ns, cols=4, crop=0).shape == (4, 32, 32)
    with pytest.raises(ValueError):
        heat_map_panels(ns[:, :100])


def test_clustering_on_a_hand_built_case():
    """six embeddings: 0, 1, 4 share 15 set entries (0 and 1 are equal, 4 differs in one), 2 and 3 are equal and disjoint
    from them, 5 stands alone.  Dot products: 15 within {0, 1}, 14 to 4, 15 within {2, 3}; threshold 0.8 * 15 = 12"""
    from mulan_amd.evaluators import Clustering, get_embedding
    e = [get_embedding(1, 50, 0)[0], get_embedding(1, 50, 0)[0], get_embedding(1, 50, 20)[0], get_embedding(1, 50, 20)[0],
         get_embedding(1, 50, 1)[0], get_embedding(1, 50, 35)[0]]
    cl = Clustering(images=list("abcdef"), embeddings=torch.stack(e))
    assert cl.threshold == pytest.approx(12.0)
    assert cl.clusters() == [[0, 1, 4], [1, 0, 4], [2, 3], [3, 2], [4, 0, 1]]
    assert cl.clusters(cluster_count=2, cluster_size_max=2) == [[0, 1], [1, 0]]
    assert Clustering(None, np.stack([v.numpy() for v in e]), threshold=0.95).clusters() == [[0, 1], [1, 0], [2, 3], [3, 2]]


def _fake_experiment(model):
    return types.SimpleNamespace(model=model, orig_params={"gamma": None}, device=torch.device("cpu"))


def test_schedule_functions_refuse_bad_arguments_before_the_device():
    from mulan_amd import evaluators as ev
    mulan = types.SimpleNamespace(deterministic_embedding=None, config=types.SimpleNamespace(latent_size=50))
    plain = types.SimpleNamespace(config=types.SimpleNamespace(latent_size=50))
    emb = ev.get_embedding(2)
    for fn in (ev.noise_schedule_per_embedding, ev.noise_schedule_summary):
        with pytest.raises(ValueError, match="MuLAN"):
            fn(_fake_experiment(plain), emb)
        for bad in ([0.0, 1.5], [-0.1], [0.5, float("nan")], [float("inf")], []):
            with pytest.raises(ValueError, match="time_steps"):
                fn(_fake_experiment(mulan), emb, bad)
        for bad in (emb[0], emb[:, :49], emb[:0], emb[None]):
            with pytest.raises(ValueError, match="embeddings"):
                fn(_fake_experiment(mulan), bad)
    with pytest.raises(ValueError, match="bins"):
        ev.noise_schedule_summary(_fake_experiment(mulan), emb, bins=300)


# ------------------------------------------------------------------------------------------------ CLI
def _args(tmp_path, *more):
    return [f"--config={CONFIG}", f"--checkpoint_directory={tmp_path}", f"--out={tmp_path}/s.npz", *more]


def test_cli_flag_parsing(tmp_path):
    from ldm import schedules
    with pytest.raises(SystemExit, match="ckpt"):
        schedules.parse_flags(_args(tmp_path))
    (tmp_path / "ckpt-3").mkdir()
    flags = schedules.parse_flags(_args(tmp_path))
    assert (flags.num_batches, flags.timesteps, flags.bins, flags.embedding, flags.keep_curves) == (30, 128, 100, "encoder", 3)
    assert schedules.parse_embedding("shift:4") == ("shift", 4) and schedules.parse_embedding("encoder") == ("encoder", None)
    for bad, what in (("--embedding=random", "embedding"), ("--embedding=shift:0", "embedding"), ("--bins=0", "bins"),
                      ("--bins=257", "bins"), ("--timesteps=0", "timesteps"), ("--num_batches=0", "num_batches"),
                      ("--keep_curves=-1", "keep_curves"), ("--config.vdm_type=vdm", "MuLAN")):
        with pytest.raises(SystemExit, match=what):
            schedules.parse_flags(_args(tmp_path, bad))
    with pytest.raises(SystemExit, match="npz"):
        schedules.parse_flags(_args(tmp_path)[:-1] + [f"--out={tmp_path}/s.txt"])
    for missing in ("--config", "--checkpoint_directory", "--out"):
        with pytest.raises(SystemExit, match=missing.lstrip("-")):
            schedules.parse_flags([a for a in _args(tmp_path) if not a.startswith(missing + "=")])


def test_cli_writes_the_documented_keys_with_the_device_call_stubbed(tmp_path, monkeypatch):
    from ldm import schedules
    from mulan_amd import evaluators as ev
    (tmp_path / "ckpt-3").mkdir()
    seen = {}

    class FakeExperiment:
        rank, device = 0, torch.device("cpu")
        model = types.SimpleNamespace(config=types.SimpleNamespace(latent_size=50))

        def __init__(self, config, directory, num):
            seen["ckpt"] = num

    def summary(experiment, emb, t, bins=100):
        E, T = emb.shape[0], len(t)
        seen["summary"] = (E, T, bins)
        z = np.zeros((E, T), dtype=np.float32)
        return dict(mean=z, std=z, min=z, max=z, sigma2_mean=z, channel_mean=np.zeros((E, T, 3), np.float32),
                    hist=np.zeros((E, T, bins), np.int32), time_steps=np.asarray(t, np.float32), between=np.zeros(T))

    def curves(experiment, emb, t):
        seen["curves"] = emb.shape[0]
        return [np.zeros((len(t), 3072), np.float32) for _ in range(emb.shape[0])]

    monkeypatch.setattr(ev, "Experiment_Colab", FakeExperiment)
    monkeypatch.setattr(ev, "noise_schedule_summary", summary)
    monkeypatch.setattr(ev, "noise_schedule_per_embedding", curves)
    out = tmp_path / "s.npz"
    assert schedules.main(_args(tmp_path, "--embedding=shift:5", "--timesteps=9", "--bins=16", "--keep_curves=2")) == 0
    assert seen == dict(ckpt=3, summary=(5, 9, 16), curves=2)
    with np.load(out) as f:
        assert sorted(f.files) == sorted(schedules.NPZ_KEYS)
        assert f["embeddings"].shape == (5, 50) and f["curves"].shape == (2, 9, 3072) and f["hist"].shape == (5, 9, 16)
        assert np.array_equal(f["embeddings"][3], ev.get_embedding(1, 50, 3)[0].numpy())
        assert f["time_steps"][0] == 0 and f["time_steps"][-1] == 1
        settings = json.loads(str(f["settings"]))
    assert settings["embedding"] == "shift:5" and settings["n_embeddings"] == 5 and settings["keep_curves"] == 2
    assert settings["timesteps"] == 9 and settings["bins"] == 16 and settings["checkpoint"] == "3"


# ------------------------------------------------------------------------------------------------ plots
def test_plot_wrappers_draw_from_the_data_functions():
    pytest.importorskip("matplotlib")
    import matplotlib
    matplotlib.use("Agg")
    import matplotlib.pyplot as plt
    from mulan_amd import evaluators as ev
    rng = np.random.default_rng(1)
    ns = [rng.standard_normal((16, 3072)) for _ in range(2)]
    hist = rng.integers(0, 50, (2, 16, 20))
    try:
        assert len(ev.plot_noise_schedule(ns).axes[0].lines) == 3072
        figs = ev.plot_heat_map(ns, count=1)
        assert len(figs) == 1 and len(figs[0].axes) == 10
        assert np.allclose(figs[0].axes[4].images[0].get_array(), ev.heat_map_panels(ns[0])[4])
        figs = ev.plot_histogram(hist)
        assert len(figs) == 2 and len(figs[0].axes) == 5 and len(figs[0].axes[2].patches) == 20
        assert [p.get_height() for p in figs[1].axes[2].patches] == list(hist[1, int(16 * 2 / 5)])
        assert len(ev.plot_histogram(dict(hist=hist), count=1)) == 1
    finally:
        plt.close("all")
