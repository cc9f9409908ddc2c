"""latent_type 'gumbel' and 'gaussian' of the two MuLAN models (ldm/model_mulan_velocity.py:41-44, 68-92, 125-139;
ldm/model_mulan_epsilon.py:24-80, 170-173): construction, parameter trees, checkpoints, the C ABI and the Gumbel
temperature schedule.  No GPU needed."""
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("mulan_gumbel_latent_fwd", "mulan_gumbel_latent_bwd", "mulan_gaussian_latent_fwd",
               "mulan_gaussian_latent_bwd")


def make_cfg(latent_type, **kw):
    from mulan_amd.model import VDMConfig
    base = dict(vocab_size=256, sample_softmax=False, antithetic_time_sampling=True, with_fourier_features=True,
                with_attention=False, gamma_type='poly_fixedend', gamma_min=-13.3, gamma_max=5.0, sm_n_timesteps=0,
                sm_n_embd=32, sm_n_layer=1, sm_pdrop=0.1, forward_n_layer=1, latent_size=50, latent_k=15,
                encoder='unet', latent_type=latent_type, z_conditioning=True, reparam_type='true', unet_type='vdm',
                condition='input')
    base.update(kw)
    return VDMConfig(**base)


@pytest.mark.parametrize("vdm_type", ["mulan_velocity", "mulan_epsilon"])
@pytest.mark.parametrize("latent_type", ["gumbel", "gaussian"])
def test_both_latents_construct_for_both_models(vdm_type, latent_type):
    from mulan_amd import model as M
    m = M.make_vdm(vdm_type, make_cfg(latent_type))
    assert m.config.latent_type == latent_type
    # topk_noise_type is a topk setting: 'gumbel' there does not stop the velocity model from taking another latent
    M.make_vdm(vdm_type, make_cfg(latent_type, topk_noise_type='gumbel'))


@pytest.mark.parametrize("latent_type", ["topk", "gumbel", "gaussian"])
def test_other_encoders_and_schedules_still_raise(latent_type):
    from mulan_amd import model as M
    with pytest.raises(NotImplementedError):
        M.make_vdm("mulan_velocity", make_cfg(latent_type, encoder='cnn'))
    for gamma_type in ('linear', 'learnable_nnet'):
        with pytest.raises(NotImplementedError):
            M.make_vdm("mulan_epsilon", make_cfg(latent_type, gamma_type=gamma_type))
    with pytest.raises(NotImplementedError):
        M.make_vdm("mulan_epsilon", make_cfg('categorical'))


def test_topk_checks_stay():
    from mulan_amd import model as M
    with pytest.raises(ValueError):
        M.make_vdm("mulan_velocity", make_cfg('topk', topk_noise_type='gumbel'))
    with pytest.raises(ValueError):
        M.make_vdm("mulan_epsilon", make_cfg('topk', topk_noise_type='uniform'))


@pytest.mark.parametrize("latent_type", ["topk", "gumbel", "gaussian"])
def test_init_tree_has_the_flax_names_and_shapes(latent_type):
    from mulan_amd import model as M
    from mulan_amd.rng import PRNGKey
    cfg = make_cfg(latent_type)
    p = M.make_vdm("mulan_velocity", cfg).init(PRNGKey(0))
    enc = p["encoder_model"]
    heads = {k for k in enc if k.startswith("dense_layer_final")}
    if latent_type == 'gaussian':
        assert heads == {"dense_layer_final_mu", "dense_layer_final_sigma"}
    else:
        assert heads == {"dense_layer_final"}
    for h in heads:
        assert set(enc[h]) == {"kernel", "bias"}
        assert tuple(enc[h]["kernel"].shape) == (1024, cfg.latent_size)
        assert tuple(enc[h]["bias"].shape) == (cfg.latent_size,)
        assert float(enc[h]["bias"].abs().max()) == 0.0 and float(enc[h]["kernel"].std()) > 0
    # everything else is the topk tree, name for name and shape for shape
    ref = M.make_vdm("mulan_velocity", make_cfg('topk')).init(PRNGKey(0))
    strip = lambda t: {path: tuple(v.shape) for path, v in M.tree_leaves(t) if not path[1].startswith("dense_layer_final")}
    assert strip(p) == strip(ref)


def test_gaussian_heads_rank_with_the_topk_head_in_the_gradient_buckets():
    from mulan_amd.train_state import grad_ready_rank
    first = grad_ready_rank(("encoder_model", "dense_layer_final", "kernel"))
    for head in ("dense_layer_final_mu", "dense_layer_final_sigma"):
        r = grad_ready_rank(("encoder_model", head, "kernel"))
        assert r[:3] == first[:3]
        assert r < grad_ready_rank(("encoder_model", "conv_out", "kernel"))


def test_gaussian_tree_round_trips_the_flax_checkpoint(tmp_path):
    from mulan_amd import checkpoint as ck
    from mulan_amd import model as M
    from mulan_amd.rng import PRNGKey
    p = M.make_vdm("mulan_epsilon", make_cfg('gaussian')).init(PRNGKey(3))
    p["encoder_model"]["dense_layer_final_sigma"]["bias"] += torch.linspace(-1, 1, 50)
    flax = M.to_flax_layout(p)
    path = str(tmp_path / "checkpoint_1")
    ck.save_flax(path, {"step": 1, "params": flax, "ema_params": flax})
    back = ck.load_flax(path)
    got = {path: np.asarray(v) for path, v in M.tree_leaves(back["params"])}
    want = {path: v.numpy() for path, v in M.tree_leaves(flax)}
    assert set(got) == set(want)
    for k in want:
        assert np.array_equal(got[k], want[k]), k
    # and back into a product-layout tree
    like = M.make_vdm("mulan_epsilon", make_cfg('gaussian')).init(PRNGKey(4))
    M.from_flax_layout(M.tree_map(torch.as_tensor, back["ema_params"]), like)
    for path, v in M.tree_leaves(p):
        t = like
        for k in path:
            t = t[k]
        assert torch.equal(t, v), path


def _header_decls():
    src = open(os.path.join(ROOT, "include", "mulan_hip.h")).read()
    return {m.group(1): m.group(2) for m in re.finditer(r"\bint\s+(mulan_\w+)\s*\(([^)]*)\)\s*;", src)}


def test_new_entry_points_are_declared_and_bound():
    from mulan_amd import lib
    decls = _header_decls()
    for name in NEW_SYMBOLS:
        assert name in decls and name in lib.SIGNATURES, name
        assert len(lib.SIGNATURES[name]) == len(decls[name].split(",")), name
    # tau of the Gumbel kernels is a device pointer, not a by-value float
    for name in NEW_SYMBOLS[:2]:
        assert "const float* tau" in decls[name]


def test_model_step_tau_matches_fp32_numpy():
    from mulan_amd.model import gumbel_tau
    for step in (0, 1, 69315, 10 ** 6):
        want = np.maximum(np.float32(0.5), np.exp(np.float32(-1e-5) * np.float32(step)))
        assert want.dtype == np.float32
        got = gumbel_tau(step)
        assert np.float32(got) == want and float(want) == got, (step, got, want)
    assert gumbel_tau(0) == 1.0 and gumbel_tau(10 ** 6) == 0.5
    # the floor takes over between 69 314 (exp = 0.50000364) and 69 315 (0.49999863)
    assert gumbel_tau(69314) > 0.5 and gumbel_tau(69315) == 0.5


def test_deterministic_embeddings():
    from mulan_amd import model as M
    B = 3
    e = M.make_vdm("mulan_velocity", make_cfg('gumbel')).deterministic_embedding(B, "cpu")
    assert torch.equal(e, torch.nn.functional.one_hot(torch.ones(B, dtype=torch.long), 50).float())
    e = M.make_vdm("mulan_epsilon", make_cfg('gaussian')).deterministic_embedding(B, "cpu")
    assert torch.equal(e, torch.zeros(B, 50))
    e = M.make_vdm("mulan_epsilon", make_cfg('topk')).deterministic_embedding(B, "cpu")
    assert float(e.sum()) == 15 * B and torch.equal(e[:, :15], torch.ones(B, 15))


def test_ode_context_refuses_the_gaussian_latent():
    from mulan_amd import model as M
    m = M.make_vdm("mulan_velocity", make_cfg('gaussian'))
    with pytest.raises(NotImplementedError, match="apply_encoder"):
        m.ode_context({}, torch.zeros(1, 32, 32, 3, dtype=torch.uint8))
