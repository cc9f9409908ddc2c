"""latent_type 'gumbel' and 'gaussian' on the MI355X: the four latent kernels against float64, the whole model against
the float64 restatement of tests/latent_oracle.py, the replayed train step against the eager one (tau is a
stream-ordered device scalar), and the evaluation / sampling / CLI surface."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import torch_ref as tr

from tests import latent_oracle as lo
from tests.oracle_dev import run_oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = lambda a: torch.tensor(np.asarray(a), dtype=torch.float32).cuda()


def close(got, want, rtol, name):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    scale = np.abs(want).max() + 1e-30
    err = np.abs(got - want)
    ok = err <= rtol * np.abs(want) + rtol * 1e-2 * scale
    assert ok.all(), (name, float(err.max()), float((err / (np.abs(want) + 1e-30)).max()))


# ----------------------------------------------------------------------------- kernels against float64
@pytest.mark.parametrize("B", [1, 7, 128])
@pytest.mark.parametrize("L", [50, 64])
@pytest.mark.parametrize("tau", [1.0, 0.9048, 0.5])
def test_gumbel_kernels_against_float64(B, L, tau):
    from mulan_amd import ops
    rng = np.random.default_rng(B * 1000 + L + int(tau * 100))
    logits = rng.standard_normal((B, L)).astype(np.float32) * 2
    gum = rng.gumbel(size=(B, L)).astype(np.float32)
    if B > 1:       # exact ties of (logits + g) / tau: jnp.argmax takes the first index
        gum[0] = 0.0
        logits[0, 0] = logits[0, L - 1] = logits[0].max() + 1.0
        gum[1] = 0.0
        logits[1, L // 2] = logits[1, L // 2 + 3] = logits[1].max() + 1.0
    demb = rng.standard_normal((B, L)).astype(np.float32)
    dkl = rng.standard_normal(B).astype(np.float32)
    tau32 = float(np.float32(tau))
    lg = f32(logits).requires_grad_(True)
    emb, kl = ops.gumbel_embedding(lg, f32(gum), torch.full((), tau32, device="cuda"))
    torch.autograd.backward([emb, kl], [f32(demb), f32(dkl)])
    rl = torch.tensor(logits, dtype=torch.float64, requires_grad=True)
    remb, rkl = lo.gumbel_latent(rl, torch.tensor(gum, dtype=torch.float64), tau32)
    torch.autograd.backward([remb, rkl], [torch.tensor(demb, dtype=torch.float64), torch.tensor(dkl, dtype=torch.float64)])
    hard = np.round(emb.detach().cpu().numpy())
    assert np.array_equal(hard, np.round(remb.detach().numpy()))
    assert np.array_equal(hard.sum(1), np.ones(B))
    if B > 1:
        assert hard[0, 0] == 1 and hard[1, L // 2] == 1
    close(emb.detach().cpu(), remb.detach(), 1e-5, "emb")
    close(kl.detach().cpu(), rkl.detach(), 1e-5, "kl")
    close(lg.grad.cpu(), rl.grad, 1e-4, "dlogits")


@pytest.mark.parametrize("B", [1, 7, 128])
@pytest.mark.parametrize("L", [50, 64])
def test_gaussian_kernels_against_float64(B, L):
    from mulan_amd import ops
    rng = np.random.default_rng(B * 10 + L)
    mu = rng.standard_normal((B, L)).astype(np.float32)
    s = rng.standard_normal((B, L)).astype(np.float32) * 3
    s[0, :6] = [30.0, -30.0, 0.0, 1e-4, -1e-4, 1e-30]       # softplus at its two tails and near 0
    eps = rng.standard_normal((B, L)).astype(np.float32)
    demb = rng.standard_normal((B, L)).astype(np.float32)
    dkl = rng.standard_normal(B).astype(np.float32)
    m, sv = f32(mu).requires_grad_(True), f32(s).requires_grad_(True)
    emb, kl = ops.gaussian_embedding(m, sv, f32(eps))
    torch.autograd.backward([emb, kl], [f32(demb), f32(dkl)])
    rm = torch.tensor(mu, dtype=torch.float64, requires_grad=True)
    rs = torch.tensor(s, dtype=torch.float64, requires_grad=True)
    remb, rkl = lo.gaussian_latent(rm, torch.nn.functional.softplus(rs), torch.tensor(eps, dtype=torch.float64))
    torch.autograd.backward([remb, rkl], [torch.tensor(demb, dtype=torch.float64), torch.tensor(dkl, dtype=torch.float64)])
    close(emb.detach().cpu(), remb.detach(), 1e-5, "emb")
    close(kl.detach().cpu(), rkl.detach(), 1e-5, "kl")
    close(m.grad.cpu(), rm.grad, 1e-5, "dmu")
    close(sv.grad.cpu(), rs.grad, 1e-4, "ds")


# ----------------------------------------------------------------------------- whole model against float64
def make_cfg(vdm_type, latent_type, vfe=False, T=0, E=128, n_layer=1, fwd_layers=1):
    from mulan_amd.model import VDMConfig
    return VDMConfig(vocab_size=256, sample_softmax=False, antithetic_time_sampling=True, with_fourier_features=True,
                     with_attention=False, gamma_type='poly_fixedend', gamma_min=-13.3, gamma_max=5.0,
                     sm_n_timesteps=T, sm_n_embd=E, sm_n_layer=n_layer, sm_pdrop=0.1, forward_n_layer=fwd_layers,
                     latent_size=50, latent_k=15, encoder='unet', latent_type=latent_type, z_conditioning=True,
                     reparam_type='true', unet_type='vdm', velocity_from_epsilon=vfe, condition='input',
                     sigma_type='no_blur', sigma_prior=1.0), dict(
        vdm_type=vdm_type, n_embd=E, n_layer=n_layer, forward_n_layer=fwd_layers, latent_k=15, unet_type='vdm',
        velocity_from_epsilon=vfe, n_timesteps=T)


def model_and_oracle_params(vdm_type, cfg, ocfg, latent_type, seed):
    from mulan_amd import model as M
    from mulan_amd.rng import PRNGKey
    ref = tr.init_params(ocfg, seed=seed, dtype=torch.float64)
    if latent_type == "gaussian":
        ref = lo.gaussian_params(ref, seed=seed + 1)
    for _, leaf in tr.tree_leaves(ref):
        leaf.requires_grad_(True)
    vdm = M.make_vdm(vdm_type, cfg)
    params = M.tree_map(lambda t: t.cuda(), vdm.init(PRNGKey(0)))
    M.from_flax_layout(M.tree_map(lambda t: t.detach().float(), ref), params)
    for _, leaf in M.tree_leaves(params):
        leaf.requires_grad_(True)
    return vdm, params, ref


def latent_noise(rng, latent_type, B, L=50):
    if latent_type == "gaussian":
        return rng.standard_normal((B, L))
    g = rng.gumbel(size=(B, L))
    g[np.arange(B), rng.integers(0, L, B)] += 5.0      # a clear winner per row: no near-tie of the fp32 / fp64 argmax
    return g


@pytest.mark.parametrize("latent_type", ["gumbel", "gaussian"])
@pytest.mark.parametrize("vdm_type,vfe,T", [("mulan_velocity", False, 0), ("mulan_velocity", True, 0),
                                            ("mulan_epsilon", False, 0), ("mulan_epsilon", False, 1000)])
def test_whole_model_against_float64(latent_type, vdm_type, vfe, T):
    from mulan_amd import model as M
    cfg, ocfg = make_cfg(vdm_type, latent_type, vfe, T)
    vdm, params, ref_params = model_and_oracle_params(vdm_type, cfg, ocfg, latent_type, seed=3)
    B, step = 4, 60000
    tau = lo.gumbel_tau(step)
    rng = np.random.default_rng(17)
    x = rng.integers(0, 256, (B, 32, 32, 3)).astype(np.uint8)
    zn = latent_noise(rng, latent_type, B).astype(np.float32)
    e0, e = rng.standard_normal((B, 3072)), rng.standard_normal((B, 3072))
    t0 = 0.37
    nkey = "eps_z" if latent_type == "gaussian" else "gumbel"
    noise = {"t0": t0, nkey: f32(zn), "eps_0": f32(e0), "eps": f32(e)}
    out, aux = vdm.apply(params, torch.tensor(x).cuda(), None, None, step=step, rngs=None, deterministic=True,
                         noise=noise, return_aux=True)
    # the gaussian draw is continuous: the oracle's schedule and score model see the model's embedding (compared on its
    # own below), its encoder gets the gradient through its own float64 draw (latent_oracle.mulan_forward)
    emb_value = aux["emb"].detach().cpu().double() if latent_type == "gaussian" else None
    ref = run_oracle(lambda P, *a, **k: lo.mulan_forward(P, ocfg, *a, **k), ref_params, torch.tensor(x), t0,
                     torch.tensor(zn, dtype=torch.float64), torch.tensor(e0).view(B, 32, 32, 3),
                     torch.tensor(e).view(B, 32, 32, 3), latent_type=latent_type, tau=tau, backward="bpd",
                     emb_value=emb_value)
    rel = lambda a, b: float(np.abs(np.asarray(a) - np.asarray(b)).max() / (np.abs(np.asarray(b)).max() + 1e-30))
    np_ = lambda t: t.detach().cpu().numpy()
    if latent_type == "gumbel":
        assert np.array_equal(np.round(np_(aux["emb"])), np.round(ref["aux"]["emb"].numpy()))
        assert rel(np_(aux["emb"]), ref["aux"]["emb"].numpy()) < 2e-4
    else:
        mu, var = ref["aux"]["logits"]
        own = (mu + torch.sqrt(var) * torch.tensor(zn, dtype=torch.float64)).numpy()
        assert rel(np_(aux["emb"]), own) < 2e-4
    assert rel(np_(aux["zt"]), ref["aux"]["z_t"].numpy().reshape(B, -1)) < 1e-5
    assert rel(np_(out.loss_recon), ref["loss_recon"].numpy()) < 1e-4
    assert rel(np_(out.loss_klz), ref["loss_klz"].numpy()) < 1e-4
    assert rel(np_(out.loss_diff), ref["loss_diff"].numpy()) < (2e-3 if T else 5e-4)
    r = 1.0 / (3072 * np.log(2.0))
    bpd = (out.loss_recon.mean() + out.loss_klz.mean() + out.loss_diff.mean()) * r
    assert abs(float(bpd) - float(ref["bpd"])) < 0.005, (float(bpd), float(ref["bpd"]))
    bpd.backward()
    flax_grads = M.to_flax_layout(M.tree_map(lambda t: t.grad if t.grad is not None else torch.zeros_like(t), params))
    worst = []
    for path, leaf in tr.tree_leaves(ref_params):
        g = flax_grads
        for k in path:
            g = g[k]
        rg = leaf.grad.numpy() if leaf.grad is not None else np.zeros(tuple(leaf.shape))
        scale = np.abs(rg).max()
        err = np.abs(g.cpu().double().numpy() - rg).max()
        worst.append((err / (scale + 1e-12) if scale > 1e-12 else err, "/".join(path)))
    worst.sort(reverse=True)
    # the bars of tests/test_gpu_model.py: 2e-3 of each leaf's gradient scale (T > 0: the fp32 expm1 of a ~1e-2
    # difference of O(10) numbers, 2e-2 as for the topk T = 1000 case)
    assert worst[0][0] < (2e-2 if T else 2e-3), worst[:8]
    heads = ("dense_layer_final_mu", "dense_layer_final_sigma") if latent_type == "gaussian" else ("dense_layer_final",)
    for h in heads:
        assert float(flax_grads["encoder_model"][h]["kernel"].abs().max()) > 0, h


# ----------------------------------------------------------------------------- replayed step == eager step
def _experiment(latent_type, graph):
    from mulan_amd.config import load_config_file
    from mulan_amd.experiment import Experiment_VDM
    config = load_config_file(os.path.join(ROOT, "ldm", "configs", "cifar10-conditioned.py"))
    config.model.latent_type = latent_type
    config.model.sm_n_layer = 1
    config.model.forward_n_layer = 1
    config.data.dataset = "synthetic"
    config.training.batch_size_train = 4
    config.training.batch_size_eval = 4
    config.training.substeps = 1
    config.training.hip_graph = graph
    return Experiment_VDM(config)


def _train(latent_type, graph, start_step, n=3):
    exp = _experiment(latent_type, graph)
    exp.state.step = start_step
    g = torch.Generator().manual_seed(3)
    scal = []
    for _ in range(n):
        batch = {"images": torch.randint(0, 256, (4, 32, 32, 3), generator=g, dtype=torch.uint8).cuda(),
                 "labels": torch.zeros(4, dtype=torch.int32).cuda(),
                 "conditioning": torch.zeros(4, dtype=torch.uint8).cuda()}
        _, m = exp.train_step(exp._train_rng, exp.state, batch)
        scal.append({k: float(v) for k, v in m["scalars"].items()})
    torch.cuda.synchronize()
    st = exp.state
    return (st.flat.clone(), st.ema.clone(), st.mu.clone(), st.nu.clone(), st.step, scal, exp._graphed is not None)


@pytest.mark.parametrize("latent_type,start", [("gumbel", 0), ("gumbel", 60000), ("gaussian", 0)])
def test_replayed_steps_equal_eager_steps(latent_type, start, monkeypatch):
    e = _train(latent_type, False, start)
    g = _train(latent_type, True, start)
    assert not e[6] and g[6] and e[4] == g[4] == start + 3
    for a, b, name in zip(e[:4], g[:4], ("params", "ema", "mu", "nu")):
        assert torch.equal(a, b), (name, float((a - b).abs().max()))
    assert e[5] == g[5]
    assert len({s["train_bpd"] for s in g[5]}) == 3
    if latent_type == "gumbel" and start:
        # tau = exp(-0.6) reaches the replayed steps through device memory.  The same run with tau forced to 1 in the
        # replayed steps -- what a tau baked in at the capture (step = 0) would give -- shares the eager first step and
        # then departs: the straight-through forward value hardly depends on tau, its gradient does
        from mulan_amd.experiment import GraphedStep
        fill = GraphedStep._fill

        def fill_tau_1(self, *a):
            fill(self, *a)
            self.noise['tau'].fill_(1.0)
        monkeypatch.setattr(GraphedStep, "_fill", fill_tau_1)
        f = _train(latent_type, True, start)
        assert f[6] and f[5][0] == g[5][0]
        # the replayed steps' gradients differ (Adam moments, parameters); the logged forward metrics may agree to the
        # last bit: the one-hot forward value does not depend on tau
        assert not torch.equal(f[2], g[2]) and not torch.equal(f[0], g[0])


# ----------------------------------------------------------------------------- evaluation, sampling, CLI
def test_dense_evaluator_path_on_a_gaussian_model_matches_the_oracle():
    """the dense VLB evaluator's loss_fn(same_image=True): the encoder runs on one row, both heads are broadcast, eps_z
    still differs per row"""
    cfg, ocfg = make_cfg("mulan_epsilon", "gaussian")
    vdm, params, ref_params = model_and_oracle_params("mulan_epsilon", cfg, ocfg, "gaussian", seed=11)
    B = 6
    rng = np.random.default_rng(4)
    x = np.repeat(rng.integers(0, 256, (1, 32, 32, 3)).astype(np.uint8), B, axis=0)
    zn = rng.standard_normal((B, 50)).astype(np.float32)
    e0, e = rng.standard_normal((B, 3072)), rng.standard_normal((B, 3072))
    noise = {"t0": 0.1, "eps_z": f32(zn), "eps_0": f32(e0), "eps": f32(e)}
    with torch.no_grad():
        out, aux = vdm.apply(params, torch.tensor(x).cuda(), None, None, step=0, deterministic=True, noise=noise,
                             return_aux=True, same_image=True)
        full = vdm.apply(params, torch.tensor(x).cuda(), None, None, step=0, deterministic=True, noise=noise)
    ref = run_oracle(lambda P, *a, **k: lo.mulan_forward(P, ocfg, *a, **k), ref_params, torch.tensor(x), 0.1,
                     torch.tensor(zn, dtype=torch.float64), torch.tensor(e0).view(B, 32, 32, 3),
                     torch.tensor(e).view(B, 32, 32, 3), latent_type="gaussian")
    emb = aux["emb"].cpu()
    assert not torch.equal(emb[0], emb[1])
    assert torch.allclose(out.loss_klz.cpu(), full.loss_klz.cpu(), rtol=1e-5, atol=0)
    r = 1.0 / (3072 * np.log(2.0))
    bpd = float((out.loss_recon.mean() + out.loss_klz.mean() + out.loss_diff.mean()) * r)
    assert abs(bpd - float(ref["bpd"])) < 0.005
    close(out.loss_klz.cpu(), ref["loss_klz"], 1e-4, "loss_klz")


@pytest.mark.parametrize("latent_type", ["gumbel", "gaussian"])
def test_ancestral_sampler_uses_the_deterministic_embedding(latent_type):
    from mulan_amd.rng import PRNGKey
    cfg, ocfg = make_cfg("mulan_velocity", latent_type)
    vdm, params, _ = model_and_oracle_params("mulan_velocity", cfg, ocfg, latent_type, seed=5)
    B, T = 3, 4
    want_emb = torch.zeros(B, 50, device="cuda")
    if latent_type == "gumbel":
        want_emb[:, 1] = 1.0
    emb = vdm.deterministic_embedding(B, "cuda")
    assert torch.equal(emb, want_emb)
    z = PRNGKey(8).normal((B, 3072), "cuda").view(B, 32, 32, 3)
    rng = PRNGKey(9)
    with torch.no_grad():
        a = vdm.sample(params, 0, T, z, torch.zeros(B, device="cuda"), rng)
        b = vdm.conditional_sample(params, 0, T, z, want_emb, torch.zeros(B, device="cuda"), rng)
        other = torch.zeros(B, 50, device="cuda")
        other[:, :15] = 1.0
        c = vdm.conditional_sample(params, 0, T, z, other, torch.zeros(B, device="cuda"), rng)
    assert torch.equal(a, b) and not torch.equal(a, c)


def test_ode_context_on_a_gaussian_model_raises():
    cfg, ocfg = make_cfg("mulan_velocity", "gaussian")
    vdm, params, _ = model_and_oracle_params("mulan_velocity", cfg, ocfg, "gaussian", seed=5)
    with pytest.raises(NotImplementedError, match="gaussian"):
        vdm.ode_context(params, torch.zeros(2, 32, 32, 3, dtype=torch.uint8, device="cuda"))
    # gumbel keeps the hard top-k context of the encoder logits (notebook_utils.logits_to_embeddings)
    cfg, ocfg = make_cfg("mulan_velocity", "gumbel")
    vdm, params, _ = model_and_oracle_params("mulan_velocity", cfg, ocfg, "gumbel", seed=5)
    ctx = vdm.ode_context(params, torch.zeros(2, 32, 32, 3, dtype=torch.uint8, device="cuda"))
    assert ctx["emb"].shape == (2, 50) and float(ctx["emb"].sum()) == 30.0


@pytest.mark.parametrize("latent_type", ["gumbel", "gaussian"])
def test_cli_train_checkpoint_and_dense_eval(latent_type, tmp_path):
    import importlib
    import ldm.main
    import ldm.eval_bpd
    from mulan_amd import checkpoint as ck
    cfgp = os.path.join(ROOT, "ldm", "configs", "cifar10-conditioned.py")
    imgs = np.random.default_rng(0).integers(0, 256, (4, 32, 32, 3)).astype(np.uint8)
    np.savez(tmp_path / "test.npz", images=imgs)
    common = ["--config=" + cfgp, "--config.model.latent_type=" + latent_type, "--config.model.sm_n_layer=1",
              "--config.model.forward_n_layer=1", "--config.training.batch_size_train=4",
              "--config.training.batch_size_eval=2", "--config.training.substeps=1",
              "--config.training.num_steps_train=3", "--config.training.num_steps_eval=1",
              "--config.training.steps_per_logging=1", "--config.training.steps_per_eval=3",
              "--config.training.steps_per_save=3", "--config.training.sample_timesteps=2"]
    ldm.main.main(common + ["--config.data.dataset=synthetic", "--workdir=" + str(tmp_path / "run")])
    ckdirs = [os.path.join(dp, d) for dp, dn, _ in os.walk(tmp_path / "run") for d in dn if d == "checkpoints"]
    assert len(ckdirs) == 1 and ck.checkpoint_numbers(ckdirs[0]) == [1]
    sd = ck.restore_dict(ckdirs[0])
    assert sd["step"] == 3
    heads = {k for k in sd["ema_params"]["encoder_model"] if k.startswith("dense_layer_final")}
    assert heads == ({"dense_layer_final_mu", "dense_layer_final_sigma"} if latent_type == "gaussian"
                     else {"dense_layer_final"})
    ldm.eval_bpd.FLAGS.__init__()
    importlib.reload(ldm.eval_bpd)
    bpd = ldm.eval_bpd.main(common + ["--config.data.dataset=npz:" + str(tmp_path / "test.npz"),
                                      "--checkpoint_directory=" + ckdirs[0], "--bpd_eval_method=dense",
                                      "--n_timesteps=4", "--max_images=2"])
    assert np.isfinite(float(bpd)) and float(bpd) > 0
