"""tsne.hip on the MI355X against the float64 oracle (tests/tsne_oracle.py).  Every bound is 4 x the error the oracle's fp32
restatement makes on the same input (printed beside the measured error); trajectories are compared teacher-forced, one
step from states of the oracle's float64 run, or over five free steps: early exaggeration is chaotic and free-running
fp32 and float64 maps are unrelated after thirty.  No N is above 1031; every output has sentinel rows behind it."""
import functools
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import tsne_oracle as to

INVALID = 1                              # hipErrorInvalidValue
SENTINEL = 7.0
LR = 50.0                                # learning_rate='auto' below N = 2400


def dev(a, dtype=torch.float32):
    return torch.tensor(np.asarray(a), dtype=dtype).cuda()


def with_sentinels(rows, cols, extra=2, dtype=torch.float32):
    return torch.full((rows + extra, cols), SENTINEL, device="cuda", dtype=dtype)


def raw_affinities(x, N, D, perplexity, symmetrise=1, P="auto", beta="auto"):
    """the C entry point -> (hipError_t, P [N, N], beta [N]); the outputs carry sentinel rows that are checked here"""
    from mulan_amd import lib
    Pb = with_sentinels(N, N) if isinstance(P, str) else P
    bb = torch.full((N + 2,), SENTINEL, device="cuda") if isinstance(beta, str) else beta
    rc = lib.load().mulan_tsne_affinities(lib.ptr(x), N, D, perplexity, symmetrise, lib.ptr(Pb), lib.ptr(bb), lib.stream())
    torch.cuda.synchronize()
    if rc == 0:
        assert bool((Pb.view(-1)[N * N:] == SENTINEL).all()) and (bb is None or bool((bb[N:] == SENTINEL).all()))
    if rc != 0:
        return rc, None, None
    return rc, Pb.view(-1)[:N * N].view(N, N), (None if bb is None else bb[:N])


def raw_gradient(P, Y, N, exaggeration, want_kl=True, grad="auto", ws="auto", ws_bytes=None):
    from mulan_amd import lib
    L = lib.load()
    need = L.mulan_tsne_workspace(N)
    g = with_sentinels(N, 2) if isinstance(grad, str) else grad
    kl = torch.full((3,), SENTINEL, device="cuda", dtype=torch.float64) if want_kl else None
    if isinstance(ws, str):
        ws = torch.empty(need // 4 + 4, device="cuda", dtype=torch.float32)
    rc = L.mulan_tsne_gradient(lib.ptr(P), lib.ptr(Y), N, exaggeration, lib.ptr(g), lib.ptr(kl), lib.ptr(ws),
                               need if ws_bytes is None else ws_bytes, lib.stream())
    torch.cuda.synchronize()
    if rc == 0:
        assert bool((g[N:] == SENTINEL).all()) and (kl is None or bool((kl[1:] == SENTINEL).all()))
    if rc != 0:
        return rc, None, None
    return rc, g[:N], (None if kl is None else kl[0])


@functools.lru_cache(maxsize=None)
def inputs(N, D):
    x = np.random.default_rng(100 * N + D).standard_normal((N, D)).astype(np.float32)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def planted_run(N):
    """the planted set (96 points) or a larger one with 257 (a row spans several waves, N is no multiple of 64 or 4), the
    oracle's float64 affinities as fp32, the PCA init and the float64 run's states; computed once, read-only"""
    from mulan_amd import latent_maps as lm
    if N == 96:
        x, labels = to.planted()
    else:
        x, labels = to.planted(clusters=8, per=33, seed=4)
        x, labels = x[:N], labels[:N]
    assert x.shape[0] == N
    P = to.affinity_bounds(x, 10.0)["joint"].astype(np.float32)
    Y0 = lm.pca_init(x)
    run = to.run(P, Y0, 500, lr=LR, keep=(0, 100, 260, 499))
    for a in (x, P, Y0):
        a.setflags(write=False)
    return types.SimpleNamespace(x=x, labels=labels, P=P, Y0=Y0, run=run)


# ------------------------------------------------------------------------------------------------ 1-3: affinities
@pytest.mark.parametrize("N,D", ((67, 50), (96, 1), (130, 3), (257, 67), (1031, 50)))
@pytest.mark.parametrize("perplexity", (5.0, 30.0))
def test_t1_joint_affinities_against_the_oracle(N, D, perplexity):
    x = inputs(N, D)
    b = to.affinity_bounds(x, perplexity)
    rc, P, beta = raw_affinities(dev(x), N, D, perplexity)
    assert rc == 0
    P = P.cpu().numpy().astype(np.float64)
    err, top = np.abs(P - b["joint"]).max(), b["joint"].max()
    print(f"N={N} D={D} perplexity={perplexity}: P error {err:.3e}, bound {b['tol_P']:.3e} (ratio {err / b['tol_P']:.3f}), "
          f"max P {top:.3e}")
    assert err <= b["tol_P"]
    assert abs(P.sum() - 1.0) <= 1e-6 and np.abs(P - P.T).max() <= 1e-6 * top and (np.diag(P) == 0).all()
    from mulan_amd import ops
    again, beta2 = ops.tsne_affinities(dev(x), perplexity, return_beta=True)            # the op gives what the entry point gives
    assert np.array_equal(again.cpu().numpy(), P.astype(np.float32)) and torch.equal(beta2, beta)


@pytest.mark.parametrize("N,D", ((67, 50), (96, 1), (130, 3), (257, 67), (1031, 50)))
@pytest.mark.parametrize("perplexity", (5.0, 30.0))
def test_t2_conditional_rows_have_the_requested_perplexity(N, D, perplexity):
    x = inputs(N, D)
    b = to.affinity_bounds(x, perplexity)
    rc, P, beta = raw_affinities(dev(x), N, D, perplexity, symmetrise=0)
    assert rc == 0
    P, beta = P.cpu().numpy(), beta.cpu().numpy().astype(np.float64)
    perp = to.row_perplexity(P)
    rel = np.abs(beta - b["beta"]) / b["beta"]
    print(f"N={N} D={D} perplexity={perplexity}: row perplexity off by {np.abs(perp / perplexity - 1).max():.3e} (bound 1e-4), "
          f"beta off by {rel.max():.3e} relative, bound {b['tol_beta']:.3e}, cond error "
          f"{np.abs(P - b['cond']).max():.3e}, bound {b['tol_cond']:.3e}")
    assert np.abs(perp / perplexity - 1).max() <= 1e-4
    assert rel.max() <= b["tol_beta"]
    assert np.abs(P - b["cond"]).max() <= b["tol_cond"] and (np.diag(P) == 0).all()
    assert np.abs(P.astype(np.float64).sum(axis=1) - 1).max() <= 1e-5


def hard_sets():
    rng = np.random.default_rng(8)
    base = rng.standard_normal((40, 5)).astype(np.float32)
    dup = base.copy()
    dup[[3, 17, 29]] = dup[0]                                 # four coincident points
    outlier = base.copy()
    outlier[7] = 1e4 * np.abs(base).max()                     # the exponentials of its row underflow but at the minimum
    khot = np.zeros((48, 12), dtype=np.float32)
    for i in range(48):
        khot[i, rng.choice(12, 3, replace=False)] = 1.0       # integer distances 0, 2, 4, 6: ties everywhere
    simplex = np.eye(24, dtype=np.float32)                    # every pair at distance 2: uniform rows
    return dict(duplicates=dup, outlier=outlier, khot=khot, equidistant=simplex)


@pytest.mark.parametrize("kind", ("duplicates", "outlier", "khot", "equidistant"))
def test_t3_hard_rows(kind):
    x = hard_sets()[kind]
    N, D = x.shape
    b = to.affinity_bounds(x, 5.0)
    rc, C, beta = raw_affinities(dev(x), N, D, 5.0, symmetrise=0)
    assert rc == 0
    C, beta = C.cpu().numpy().astype(np.float64), beta.cpu().numpy().astype(np.float64)
    rel = (np.abs(beta - b["beta"]) / b["beta"]).max()
    print(f"{kind}: cond error {np.abs(C - b['cond']).max():.3e}, bound {b['tol_cond']:.3e}; beta {beta.min():.3e} .. "
          f"{beta.max():.3e}, off by {rel:.3e} relative, bound {b['tol_beta']:.3e}")
    assert np.isfinite(C).all() and np.isfinite(beta).all() and (beta > 0).all()
    assert np.abs(C.sum(axis=1) - 1).max() <= 1e-5 and (np.diag(C) == 0).all()
    assert np.abs(C - b["cond"]).max() <= b["tol_cond"] and rel <= b["tol_beta"]
    if kind == "equidistant":
        assert np.abs(C[~np.eye(N, dtype=bool)] - 1.0 / (N - 1)).max() <= 1e-7 and (beta == 2.0 ** 100).all()
    if kind == "duplicates":
        assert C[0, 3] == C[0, 17] == C[0, 29] == C[0].max()
    rc, P, _ = raw_affinities(dev(x), N, D, 5.0)
    P = P.cpu().numpy().astype(np.float64)
    assert rc == 0 and np.abs(P - b["joint"]).max() <= b["tol_P"] and abs(P.sum() - 1) <= 1e-6


# ------------------------------------------------------------------------------------------------ 4-6: gradient, update
STATES = (0, 100, 260, 499)


@pytest.mark.parametrize("N", (96, 257))
@pytest.mark.parametrize("it", STATES)
def test_t4_gradient_and_kl_teacher_forced(N, it):
    s = planted_run(N)
    Y = s.run["states"][it][0].astype(np.float32)
    Pd, Yd = dev(s.P), dev(Y)
    for ex in (12.0, 1.0):
        b = to.gradient_bounds(s.P, Y, ex)
        rc, g, kl = raw_gradient(Pd, Yd, N, ex)
        assert rc == 0
        g, kl = g.cpu().numpy().astype(np.float64), float(kl)
        err = np.abs(g - b["grad"]).max()
        print(f"N={N} it={it} exaggeration={ex}: grad error {err:.3e}, bound {b['tol_grad']:.3e} (ratio "
              f"{err / b['tol_grad']:.3f}), |grad| {np.abs(b['grad']).max():.3e}; kl {kl:.9f}, error {abs(kl - b['kl']):.3e}, "
              f"bound {b['tol_kl']:.3e}")
        assert err <= b["tol_grad"]
        assert abs(kl - b["kl"]) <= b["tol_kl"]
        assert abs(kl - to.kl(s.P.astype(np.float64), Y.astype(np.float64))) <= b["tol_kl"]
        rc, g2, none = raw_gradient(Pd, Yd, N, ex, want_kl=False)                  # the instantiation without the divergence
        assert rc == 0 and none is None and np.array_equal(g2.cpu().numpy(), g.astype(np.float32))


@pytest.mark.parametrize("N", (96, 257))
def test_t4_coincident_points_and_a_spread_of_1e6(N):
    s = planted_run(N)
    Y = s.run["states"][260][0].astype(np.float32)
    same = Y.copy()
    same[[1, 2, 50]] = same[0]                                                     # w = 1, zero difference
    wide = (Y / np.abs(Y).max() * 1e6).astype(np.float32)                         # w^2 underflows between the clusters
    for name, y in (("coincident", same), ("spread", wide)):
        b = to.gradient_bounds(s.P, y, 1.0)
        rc, g, kl = raw_gradient(dev(s.P), dev(y), N, 1.0)
        g, kl = g.cpu().numpy().astype(np.float64), float(kl)
        err = np.abs(g - b["grad"]).max()
        print(f"N={N} {name}: grad error {err:.3e}, bound {b['tol_grad']:.3e}; kl error {abs(kl - b['kl']):.3e}, bound "
              f"{b['tol_kl']:.3e}")
        assert rc == 0 and np.isfinite(g).all() and np.isfinite(kl)
        assert err <= b["tol_grad"] and abs(kl - b["kl"]) <= b["tol_kl"]


@pytest.mark.parametrize("N", (96, 257))
@pytest.mark.parametrize("it", STATES)
def test_t5_update_teacher_forced(N, it):
    from mulan_amd import ops
    s = planted_run(N)
    Y, U, G = (v.astype(np.float32) for v in s.run["states"][it])
    early = it < 250
    ex, mom = (12.0, 0.5) if early else (1.0, 0.8)
    b = to.update_bounds(s.P, Y, U, G, ex, mom, LR)                                # asserts the excluded share <= 1 %
    Yd, Ud, Gd = (with_sentinels(N, 2) for _ in range(3))
    for t, v in ((Yd, Y), (Ud, U), (Gd, G)):
        t[:N] = dev(v)
    kl = ops.tsne_step(dev(s.P), Yd[:N], Ud[:N], Gd[:N], ex, mom, LR, kl=True)
    torch.cuda.synchronize()
    assert kl.shape == () and kl.dtype == torch.float64 and abs(float(kl) - to.kl(s.P, Y)) <= to.gradient_bounds(s.P, Y, ex)["tol_kl"]
    keep = b["keep"]
    print(f"N={N} it={it}: {(~keep).sum()} of {keep.size} elements left out")
    for name, t in (("Y", Yd), ("U", Ud), ("G", Gd)):
        assert bool((t[N:] == SENTINEL).all())
        err = np.abs(t[:N].cpu().numpy().astype(np.float64) - b[name])[keep].max()
        print(f"  {name}: error {err:.3e}, bound {b['tol_' + name]:.3e} (ratio {err / max(b['tol_' + name], 1e-300):.3f})")
        assert err <= b["tol_" + name], name
    if it == 0:
        assert (U == 0).all() and bool((Gd[:N] == np.float32(0.8)).all())


def test_t6_five_free_iterations_from_the_pca_init():
    from mulan_amd import ops
    s = planted_run(96)
    b = to.free_run_bounds(s.P, s.Y0, 5, lr=LR)
    P, Y = dev(s.P), dev(s.Y0)
    U, G = torch.zeros_like(Y), torch.ones_like(Y)
    for _ in range(5):
        assert ops.tsne_step(P, Y, U, G, 12.0, 0.5, LR) is None
    err = np.abs(Y.cpu().numpy().astype(np.float64) - b["Y"]).max()
    print(f"five free steps: error {err:.3e}, bound {b['tol_Y']:.3e}, scale {np.abs(b['Y']).max():.3e}")
    assert err <= b["tol_Y"]


# ------------------------------------------------------------------------------------------------ 7-8: whole runs
def test_t7_the_same_inputs_give_the_same_bits():
    from mulan_amd import latent_maps as lm, ops
    s = planted_run(257)
    x, P = dev(s.x), dev(s.P)
    Y = dev(s.run["states"][100][0].astype(np.float32))
    a, b = ops.tsne_affinities(x, 10.0), ops.tsne_affinities(x, 10.0)
    assert torch.equal(a, b)
    (g1, k1), (g2, k2) = ops.tsne_gradient(P, Y, 12.0, kl=True), ops.tsne_gradient(P, Y, 12.0, kl=True)
    assert torch.equal(g1, g2) and torch.equal(k1, k2)
    r1, r2 = (lm.tsne(s.x, perplexity=10.0, n_iter=20, record_every=5) for _ in range(2))
    assert np.array_equal(r1["Y"], r2["Y"]) and np.array_equal(r1["kl"], r2["kl"]) and np.array_equal(r1["beta"], r2["beta"])
    assert list(r1["kl_iter"]) == [0, 5, 10, 15, 20] and np.isfinite(r1["kl"]).all()


def test_t8_long_run_on_the_planted_set():
    from mulan_amd import latent_maps as lm
    s = planted_run(96)
    finals = [s.run["kl"], to.run(s.P, s.Y0, 500, lr=LR, dtype=np.float32)["kl"]]
    for sign in (1, -1):                                                         # inits perturbed in the last bit
        y = np.nextafter(s.Y0, np.float32(sign) * np.float32(np.inf)).astype(np.float32)
        finals.append(to.run(s.P, y, 500, lr=LR)["kl"])
    m = 3.0 * (max(finals) - min(finals)) / s.run["kl"]
    res = lm.tsne(s.x, perplexity=10.0, n_iter=500, init=s.Y0)
    print(f"oracle final KL {s.run['kl']:.6f} (from {s.run['kl0']:.4f}); spread of the four host runs "
          f"{(max(finals) - min(finals)) / s.run['kl']:.3e}, m = {m:.3e}; device final KL {res['kl'][-1]:.6f} (from "
          f"{res['kl'][0]:.4f}), ratio {res['kl'][-1] / s.run['kl']:.5f}")
    assert to.purity(res["Y"], s.labels) == 1.0
    assert res["kl"][-1] <= (1.0 + m) * s.run["kl"]
    assert res["kl"][-1] < res["kl"][0] and res["settings"]["learning_rate"] == LR and len(res["kl"]) == 11


# ------------------------------------------------------------------------------------------------ 9: refusals
def test_t9_refusals_return_the_error_and_leave_the_outputs_alone():
    from mulan_amd import lib
    L = lib.load()
    N, D = 12, 3
    x = dev(inputs(67, 50)[:N, :D].copy())
    P = torch.full((N, N), SENTINEL, device="cuda")
    beta = torch.full((N,), SENTINEL, device="cuda")
    ok = dict(x=x, N=N, D=D, perplexity=3.0, P=P, beta=beta)
    for change in (dict(N=3), dict(N=16385), dict(D=0), dict(perplexity=0.5), dict(perplexity=11.0), dict(perplexity=float("nan")),
                   dict(x=None), dict(P=None), dict(symmetrise=2)):
        assert raw_affinities(**{**ok, **change})[0] == INVALID, change
    assert bool((P == SENTINEL).all()) and bool((beta == SENTINEL).all())
    assert raw_affinities(**{**ok, "beta": None})[0] == 0 and not bool((P == SENTINEL).any())      # beta may be NULL
    assert L.mulan_tsne_workspace(3) == 0 and L.mulan_tsne_workspace(16385) == 0 and L.mulan_tsne_workspace(N) >= 7 * N * 4
    Y = dev(np.random.default_rng(0).standard_normal((N, 2)))
    grad = torch.full((N, 2), SENTINEL, device="cuda")
    need = L.mulan_tsne_workspace(N)
    ws = torch.empty(need // 4, device="cuda", dtype=torch.float32)
    okg = dict(P=P, Y=Y, N=N, exaggeration=1.0, grad=grad)
    for change in (dict(N=3), dict(N=16385), dict(P=None), dict(Y=None), dict(grad=None), dict(ws=ws, ws_bytes=need - 1),
                   dict(ws=None), dict(exaggeration=0.0)):
        assert raw_gradient(**{**okg, **change})[0] == INVALID, change
    assert bool((grad == SENTINEL).all())
    U, G = torch.zeros_like(Y), torch.ones_like(Y)
    y0 = Y.clone()
    for args in ((None, Y, U, G, N, 0.5, 1.0), (grad, None, U, G, N, 0.5, 1.0), (grad, Y, None, G, N, 0.5, 1.0),
                 (grad, Y, U, None, N, 0.5, 1.0), (grad, Y, U, G, 3, 0.5, 1.0), (grad, Y, U, G, 16385, 0.5, 1.0),
                 (grad, Y, U, G, N, 0.5, 0.0), (grad, Y, U, G, N, 1.0, 1.0)):
        rc = L.mulan_tsne_update(*(lib.ptr(a) if torch.is_tensor(a) or a is None else a for a in args), lib.stream())
        assert rc == INVALID, args
    torch.cuda.synchronize()
    assert torch.equal(Y, y0) and bool((U == 0).all()) and bool((G == 1).all())


# ------------------------------------------------------------------------------------------------ 10: model level
def _mulan_experiment(batches=4, batch=24):
    """a small MuLAN model with random weights, built as tests/test_gpu_schedule_curves.py builds it, with an evaluation
    stream of random images"""
    from oracle import torch_ref as tr
    from mulan_amd import model as M
    from mulan_amd.model import VDMConfig
    from mulan_amd.rng import PRNGKey
    cfg = VDMConfig(vocab_size=256, sample_softmax=False, antithetic_time_sampling=True, with_fourier_features=True,
                    with_attention=False, gamma_type='poly_fixedend', gamma_min=-13.3, gamma_max=5.0, sm_n_timesteps=0,
                    sm_n_embd=128, sm_n_layer=1, sm_pdrop=0.1, forward_n_layer=1, latent_size=50, latent_k=15,
                    encoder='unet', latent_type='topk', z_conditioning=True, reparam_type='true', unet_type='vdm',
                    velocity_from_epsilon=False, condition='input', sigma_type='no_blur', sigma_prior=1.0)
    ocfg = dict(vdm_type='mulan_velocity', n_embd=128, n_layer=1, forward_n_layer=1, latent_k=15, unet_type='vdm',
                velocity_from_epsilon=False, n_timesteps=0)
    ref = tr.init_params(ocfg, seed=5, dtype=torch.float32)
    vdm = M.make_vdm('mulan_velocity', cfg)
    params = M.tree_map(lambda x: x.cuda(), vdm.init(PRNGKey(0)))
    M.from_flax_layout(M.tree_map(lambda x: x.detach().float(), ref), params)
    rng = np.random.default_rng(21)
    images = [torch.tensor(rng.integers(0, 256, (batch, 32, 32, 3)).astype(np.uint8)).cuda() for _ in range(batches)]

    class Stream:
        def __init__(self):
            self.i = 0

        def next(self):
            self.i += 1
            return dict(images=images[(self.i - 1) % len(images)])

    return types.SimpleNamespace(model=vdm, orig_params=params, device=torch.device("cuda"), eval_iter=Stream(), rank=0, world=1)


def test_t10_latent_map_and_the_command_line(tmp_path, monkeypatch):
    import json
    from ldm import latent_map as cli
    from mulan_amd import evaluators as ev, latent_maps as lm, model as M
    experiment = _mulan_experiment()
    N = 4 * 24
    for on, D in (("logits", 50), ("embeddings", 50), ("schedule:0.5", 3072)):
        res = lm.latent_map(experiment, num_batches=4, on=on, perplexity=8.0, n_iter=60, exaggeration_iter=30, record_every=20)
        assert res["Y"].shape == (N, 2) and res["points"].shape == (N, D) and res["colour"].shape == (N,)
        assert res["beta"].shape == (N,) and list(res["kl_iter"]) == [0, 20, 40, 60] and res["kl"].shape == (4,)
        for key in ("Y", "kl", "beta", "colour"):
            assert np.isfinite(res[key]).all(), (on, key)
        assert 0.0 <= res["knn_agreement"] <= 1.0 and res["on"] == on
        print(f"{on}: KL {res['kl'][0]:.4f} -> {res['kl'][-1]:.4f}, knn agreement {res['knn_agreement']:.3f}")
    plain = types.SimpleNamespace(model=object.__new__(M.PlainVDM), orig_params={}, device=torch.device("cuda"))
    with pytest.raises(ValueError, match="MuLAN"):
        lm.latent_map(plain)
    experiment.world = 2
    with pytest.raises(ValueError, match="one process"):
        lm.latent_map(experiment)
    experiment.world = 1
    (tmp_path / "ckpt-3").mkdir()
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    monkeypatch.setattr(ev, "Experiment_Colab", lambda config, directory, num: experiment)
    import os
    config = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "ldm", "configs", "cifar10-conditioned.py")
    out = tmp_path / "map.npz"
    assert cli.main([f"--config={config}", "--config.vdm_type=mulan_velocity", f"--checkpoint_directory={tmp_path}",
                     f"--out={out}", "--num_batches=4", "--perplexity=8", "--iters=40", "--pca=3"]) == 0
    with np.load(out) as f:
        assert sorted(f.files) == sorted(cli.NPZ_KEYS)
        assert f["Y"].shape == (N, 2) and f["pca"].shape == (N, 3) and f["pca_variance_ratio"].shape == (3,)
        assert np.isfinite(f["Y"]).all() and np.isfinite(f["kl"]).all() and 0.0 <= float(f["knn_agreement"]) <= 1.0
        settings = json.loads(str(f["settings"]))
    assert settings["n_iter"] == 40 and settings["on"] == "logits" and settings["checkpoint"] == "3" and settings["N"] == N
