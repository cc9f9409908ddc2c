"""mulan_bound_profile on the MI355X against float64 (tests/bound_profile_oracle.py: the per-element terms from
oracle.torch_ref, the bounds measured on the CPU as 4 x the error of the fp32 restatement), its exact properties (zero
residual, determinism, rows-only / cols-only, refusals), the parent's loss heads as a yardstick, and the models' and the
evaluator's profile against loss_fn and the float64 models."""
import math
import os
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import torch_ref as tr
from tests import bound_profile_oracle as bo
from tests import latent_oracle as lo
from tests.oracle_dev import run_oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROWS_BOUND, COLS_BOUND = np.array(bo.ROWS_BOUND), np.array(bo.COLS_BOUND)
KEYS = ("x", "g0", "g1", "gt", "w", "eps0", "eps", "zt")


def dev(v):
    return torch.from_numpy(np.array(v)).cuda()


def run(case, mode, **kw):
    """(rows, cols) of ops.bound_profile on one case of the oracle helper, as numpy"""
    from mulan_amd import ops
    i = bo.inputs(*case)
    out = ops.bound_profile(mode, *(dev(i[k]) for k in KEYS), dev(i[f"net{mode}"]), case[2], **kw)
    return tuple(None if o is None else o.cpu().numpy() for o in out)


@pytest.mark.parametrize("case", bo.CASES, ids=lambda c: f"{c[0]}-{c[1]}x{c[2]}-{'row' if c[3] else 'elem'}")
def test_kernel_against_float64(case):
    """every family, (G, R), gamma layout and mode within the bounds; with eps_hat = eps (mode 2, where the network
    output is eps_hat and the residual is formed by one subtraction) the diffusion columns are exactly zero -- in modes 0
    and 1 the residual v* - v_hat of that family is rounding, not zero, and is held to float64 like any other"""
    family, G, R, per_row = case
    for mode in (0, 1, 2):
        rows, cols = run(case, mode)
        assert rows.shape == (G * R, 8) and cols.shape == (G, 3, bo.D)
        rerr, cerr = bo.errors(rows, cols, *bo.case64(*case, mode))
        print(f"mode {mode} rows", " ".join(f"{v:.2e}" for v in rerr), "cols", " ".join(f"{v:.2e}" for v in cerr))
        assert (rerr <= ROWS_BOUND).all(), (mode, dict(zip(bo.ROW_NAMES, rerr)))
        assert (cerr <= COLS_BOUND).all(), (mode, dict(zip(bo.COL_NAMES, cerr)))
        if family == "exact" and mode == 2:
            assert (rows[:, 0:4] == 0).all() and (rows[:, 6] == 0).all() and (cols[:, 0] == 0).all()
            assert (rows[:, 4] > 0).all() and (rows[:, 7] > 0).all()


def test_runs_are_bit_identical_and_outputs_independent():
    for case, mode in ((("uniform", 2, 17, False), 1), (("uniform", 3, 5, True), 2)):
        rows, cols = run(case, mode)
        again = run(case, mode)
        assert np.array_equal(rows, again[0]) and np.array_equal(cols, again[1])
        only = run(case, mode, cols=False)
        assert only[1] is None and np.array_equal(only[0], rows)
        only = run(case, mode, rows=False)
        assert only[0] is None and np.array_equal(only[1], cols)


def test_chunks_do_not_depend_on_the_other_groups():
    """the bits of a group are those of the same rows profiled alone: nothing depends on how rows are dealt to blocks"""
    from mulan_amd import ops
    case = ("uniform", 2, 17, False)
    i = bo.inputs(*case)
    rows, cols = run(case, 0)
    tail = ops.bound_profile(0, *(dev(i[k][17:]) for k in KEYS), dev(i["net0"][17:]), 17)
    assert np.array_equal(tail[0].cpu().numpy(), rows[17:]) and np.array_equal(tail[1].cpu().numpy()[0], cols[1])


def _raw(L, a, mode=2, B=None, d=bo.D, R=None, per_elem=1, **change):
    p = lambda v: None if v is None else v.data_ptr()
    a = {**a, **change}
    return L.mulan_bound_profile(mode, *(p(a[k]) for k in ("x", "g0", "g1", "gt", "w")), per_elem,
                                 *(p(a[k]) for k in ("eps0", "eps", "zt", "net", "rows", "cols", "ws")),
                                 a["B"] if B is None else B, d, a["R"] if R is None else R,
                                 torch.cuda.current_stream().cuda_stream)


def test_invalid_arguments_return_the_error_without_launching():
    from mulan_amd import lib
    L = lib.load()
    INVALID = 1                                        # hipErrorInvalidValue
    B, R = 6, 3
    i = bo.inputs("uniform", 1, 7, False)
    a = {k: dev(i[k][:B]) for k in KEYS}
    a.update(net=dev(i["net2"][:B]), rows=torch.full((B, 8), 7.0, device="cuda"),
             cols=torch.full((B // R, 3, bo.D), 7.0, device="cuda"), B=B, R=R)
    assert L.mulan_bound_profile_workspace(B, R) == (B // R) * 1 * 3 * bo.D * 4
    assert L.mulan_bound_profile_workspace(34, 17) == 2 * 3 * 3 * bo.D * 4
    assert L.mulan_bound_profile_workspace(B, 4) == 0 and L.mulan_bound_profile_workspace(0, 1) == 0
    a["ws"] = torch.full((L.mulan_bound_profile_workspace(B, R) // 4,), 7.0, device="cuda")
    bad = [dict(d=1024), dict(B=0), dict(B=-6), dict(R=0), dict(R=-3), dict(R=4), dict(mode=-1), dict(mode=3),
           dict(rows=None, cols=None), dict(ws=None)] + [{k: None} for k in KEYS[:-1] + ("net",)] + [dict(mode=1, zt=None)]
    for change in bad:
        assert _raw(L, a, **change) == INVALID, change
    torch.cuda.synchronize()
    assert bool((a["rows"] == 7).all()) and bool((a["cols"] == 7).all()) and bool((a["ws"] == 7).all())
    assert _raw(L, a, zt=None) == 0                    # z_t is read in mode 1 only
    assert _raw(L, a, cols=None, ws=None) == 0         # the workspace serves cols_out alone
    torch.cuda.synchronize()
    assert bool((a["rows"] != 7).all()) and bool((a["cols"] != 7).all())


@pytest.mark.parametrize("case", [("uniform", 2, 17, False), ("narrow", 3, 5, False), ("uniform", 3, 5, True)],
                         ids=lambda c: f"{c[0]}-{'row' if c[3] else 'elem'}")
def test_row_sums_agree_with_the_loss_heads(case):
    """yardstick: ops.qsample's loss_recon / loss_klz and ops.diffusion_loss on the same inputs are the same terms in
    another fp32 summation order, so the two agree within the sum of both sides' bounds"""
    from mulan_amd import ops
    i = bo.inputs(*case)
    d = {k: dev(i[k]) for k in KEYS}
    _, _, recon, klz, _, _ = ops.qsample(d["x"], d["g0"], d["g1"], d["gt"], d["eps0"], d["eps"])
    for mode in (0, 1, 2):
        rows, _ = run(case, mode, cols=False)
        diff = ops.diffusion_loss(mode, d["x"], d["gt"], d["w"], d["eps"], d["zt"], dev(i[f"net{mode}"]))
        for col, want in ((0, diff), (4, recon), (5, klz)):
            want = want.cpu().numpy().astype(np.float64)
            err = np.abs(rows[:, col] - want) / np.maximum(1.0, np.abs(want))
            print(f"mode {mode} column {col}: {err.max():.2e} (bound 2 x {ROWS_BOUND[col]:.2e})")
            assert err.max() <= 2 * ROWS_BOUND[col], (mode, col)


# ----------------------------------------------------------------------------- model level
# sm_n_embd = 128 is the narrowest model the GroupNorm kernels take (32 groups of at least 4 channels)
N_IMAGES, T_ROWS, E = 2, 8, 128
VARIANTS = {  # name: (vdm_type, model overrides, latent_type)
    "epsilon": ("mulan_epsilon", {}, "topk"),
    "epsilon-T10": ("mulan_epsilon", dict(sm_n_timesteps=10), "topk"),
    "velocity": ("mulan_velocity", {}, "topk"),
    "velocity-from-epsilon": ("mulan_velocity", dict(velocity_from_epsilon=True), "topk"),
    "plain": ("vdm", dict(gamma_type="fixed", z_conditioning=False, reparam_type="noise"), None),
    "gumbel": ("mulan_epsilon", dict(latent_type="gumbel"), "gumbel"),
}


def _experiment(tmp_path, name):
    """(Experiment_VDM at sm_n_embd = 128, one layer, on an npz of two random images; its float64 parameters; the
    oracle's configuration)"""
    from mulan_amd import model as M
    from mulan_amd.config import load_config_file
    from mulan_amd.experiment import Experiment_VDM
    vdm_type, over, latent = VARIANTS[name]
    images = np.random.default_rng(21).integers(0, 256, (N_IMAGES, 32, 32, 3)).astype(np.uint8)
    np.savez(tmp_path / "val.npz", images=images)
    config = load_config_file(os.path.join(ROOT, "ldm", "configs", "cifar10-conditioned.py"))
    config.vdm_type = vdm_type
    config.model.sm_n_embd, config.model.sm_n_layer, config.model.forward_n_layer = E, 1, 1
    for k, v in over.items():
        config.model[k] = v
    config.data.dataset = f"npz:{tmp_path / 'val.npz'}"
    config.training.batch_size_train = config.training.batch_size_eval = 2
    config.training.substeps = 1
    exp = Experiment_VDM(config)
    exp.orig_params = exp.state.ema_params
    ocfg = dict(vdm_type=vdm_type, n_embd=E, n_layer=1, forward_n_layer=1, latent_k=15, unet_type="vdm",
                velocity_from_epsilon=bool(over.get("velocity_from_epsilon", False)),
                n_timesteps=over.get("sm_n_timesteps", 0))
    ref = tr.init_params(ocfg, seed=13, dtype=torch.float64)
    if latent is None:
        ref = {"score_model": ref["score_model"]}
        ref["score_model"]["dense0"]["kernel"] = ref["score_model"]["dense0"]["kernel"][:E + 1].clone()
    M.from_flax_layout(M.tree_map(lambda t: t.detach().float(), ref), exp.state.ema_params)
    return exp, config, ref, ocfg, images


def _oracle(exp, ref, ocfg, latent, image, step):
    """float64 loss_recon, loss_klz, loss_diff [T] of one tiled image under the evaluator's noise"""
    from mulan_amd.rng import PRNGKey
    _, sample_rng = PRNGKey(0).split()
    noise = exp.model._noise({"sample": sample_rng}, None, T_ROWS, exp.device, latent is not None)
    x = torch.as_tensor(np.repeat(image[None], T_ROWS, axis=0))
    f64 = lambda t: t.double().cpu()
    e0, e = f64(noise["eps_0"]).view(T_ROWS, 32, 32, 3), f64(noise["eps"]).view(T_ROWS, 32, 32, 3)
    with torch.no_grad():
        if latent is None:
            out = run_oracle(lambda P, *a: tr.plain_vdm_forward(P, ocfg, *a), ref, x, float(noise["t0"]), e0, e)
        elif latent == "topk":
            out = run_oracle(lambda P, *a: tr.mulan_forward(P, ocfg, *a), ref, x, float(noise["t0"]),
                             f64(noise["gamma_raw"]), e0, e)
        else:
            out = run_oracle(lambda P, *a, **k: lo.mulan_forward(P, ocfg, *a, **k), ref, x, float(noise["t0"]),
                             f64(noise["gumbel"]), e0, e, latent_type="gumbel", tau=lo.gumbel_tau(step))
    return {k: out[k].numpy() for k in ("loss_recon", "loss_klz", "loss_diff")}


@pytest.mark.parametrize("name", list(VARIANTS))
def test_model_profile_against_loss_fn_and_float64(name, tmp_path):
    from ldm import bound_profile as cli
    from mulan_amd import evaluators as ev
    from mulan_amd.rng import PRNGKey
    exp, config, ref, ocfg, images = _experiment(tmp_path, name)
    latent = VARIANTS[name][2]
    prof = ev.bound_profile(exp, images, n_timesteps=T_ROWS)
    shapes = dict(t=(T_ROWS,), diff=(T_ROWS,), diff_channel=(T_ROWS, 3), recon=(T_ROWS,), klz=(T_ROWS,), kl_z=(),
                  resid2=(T_ROWS,), weight=(T_ROWS,), diff_pixel=(bo.D,), recon_pixel=(bo.D,), klz_pixel=(bo.D,), bpd=(),
                  diff_std=())
    assert set(prof) == set(shapes) and all(prof[k].shape == (N_IMAGES,) + s for k, s in shapes.items())
    rel = lambda a, b: float(np.abs(a - b).max() / np.abs(b).max())
    per_dim = 1.0 / (3072 * math.log(2.0))
    for n in range(N_IMAGES):
        tiled = {"images": torch.tensor(np.repeat(images[n:n + 1], T_ROWS, axis=0)).cuda(),
                 "labels": torch.zeros(T_ROWS, dtype=torch.int32).cuda(),
                 "conditioning": torch.zeros(T_ROWS, dtype=torch.uint8).cuda()}
        with torch.no_grad():
            bpd, _ = exp.loss_fn(exp.orig_params, tiled, n, rng=PRNGKey(0), is_train=False, same_image=True)
        print(f"{name} image {n}: bpd {prof['bpd'][n]:.7f} loss_fn {float(bpd):.7f} diff_std {prof['diff_std'][n]:.4f}")
        assert abs(prof["bpd"][n] - float(bpd)) <= 1e-5 * abs(float(bpd))
        want = _oracle(exp, ref, ocfg, latent, images[n], n)
        errs = dict(diff=rel(prof["diff"][n], want["loss_diff"] * per_dim),
                    recon=rel(prof["recon"][n], want["loss_recon"] * per_dim),
                    klz=rel(prof["klz"][n] + prof["kl_z"][n], want["loss_klz"] * per_dim))
        print(f"{name} image {n}: against the float64 model", " ".join(f"{k} {v:.2e}" for k, v in errs.items()))
        assert max(errs.values()) < 1e-4, errs
    assert np.allclose(prof["diff_pixel"].sum(1) / 3072, prof["diff"].mean(1), rtol=1e-5, atol=0)
    assert np.allclose(prof["diff_channel"].sum(2), prof["diff"], rtol=1e-5, atol=0)
    assert np.allclose(prof["diff_std"], prof["diff"].std(1)) and (prof["kl_z"] == 0).all() == (latent is None)
    t = np.sort(prof["t"], axis=1)
    if not config.model.sm_n_timesteps:
        assert np.allclose(np.diff(t, axis=1), 1.0 / T_ROWS, atol=1e-6)        # the antithetic grid
    flags = types.SimpleNamespace(config=config, n_images=N_IMAGES, timesteps=T_ROWS, keep_pixels=1)
    arrays = cli.run(exp, flags)
    assert sorted(arrays) == sorted(cli.NPZ_KEYS)
    assert arrays["diff_pixel"].shape == (1, bo.D) and arrays["diff_pixel_mean"].shape == (bo.D,)
    assert np.array_equal(arrays["images"], images) and np.array_equal(arrays["bpd"], prof["bpd"])
