"""mulan_spectrum on the MI355X against the float64 oracle (tests/spectrum_oracle.py).  Tolerances: a coefficient may
differ from float64 by 4 x the largest error the oracle's fp32 restatement makes on the same input (never more than the
analytic ceiling 68 2^-24 32 max|x|, which the oracle asserts); radial, sum1 and sum2 by 4 x the restatement's own error
on them.  No shape is larger than N = 67; `blocks` below N makes a block take several images, as it does at set sizes."""
import functools
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import spectrum_oracle as so

INVALID = 1                              # hipErrorInvalidValue
MODEL = dict(scale=2.0 / 256, offset=1.0 / 256 - 1)
SENTINEL = 7.0


def dev(a):
    return torch.tensor(np.asarray(a)).cuda()                                    # (a copy: the shared inputs are read-only)


def raw(x, N, *, is_u8, scale=1.0, offset=0.0, gray=0, coef=None, radial=None, sum1=None, sum2=None, accumulate=0,
        blocks=0, ws="auto", ws_bytes=None):
    """the C entry point itself -> hipError_t; ws 'auto': a workspace of the size the library asks for"""
    from mulan_amd import lib
    L = lib.load()
    if isinstance(ws, str):
        need = L.mulan_spectrum_workspace(max(N, 1), gray, blocks if 0 <= blocks <= 4096 else 0)
        ws = torch.empty(need // 8 + 1, device="cuda", dtype=torch.float64)
        ws_bytes = need if ws_bytes is None else ws_bytes
    rc = L.mulan_spectrum(lib.ptr(x), 0 if is_u8 else 1, scale, offset, N, gray, lib.ptr(coef), lib.ptr(radial),
                          lib.ptr(sum1), lib.ptr(sum2), accumulate, blocks, lib.ptr(ws), ws_bytes or 0, lib.stream())
    torch.cuda.synchronize()
    return rc


@functools.lru_cache(maxsize=None)
def case(kind, N, gray=False):
    """(x, kwargs, bounds) of one input family: computed once, shared, never written"""
    rng = np.random.default_rng(1000 * N + (kind == "f32"))
    if kind == "u8":
        x, kw = rng.integers(0, 256, (N, 32, 32, 3)).astype(np.uint8), dict(MODEL)
    else:
        x, kw = rng.standard_normal((N, 32, 32, 3)).astype(np.float32), {}
    assert len({v.tobytes() for v in x}) == N                                   # every image is distinct
    x.setflags(write=False)
    return x, kw, so.bounds(x, gray=gray, **kw)


def check(got, b, names=("coef", "radial", "sum1", "sum2"), label=""):
    for name in names:
        err = float(np.abs(got[name].astype(np.float64) - b[name]).max())
        print(f"{label} {name}: error {err:.3e}, bound {b['tol_' + name]:.3e}"
              + (f", ceiling {b['ceiling']:.3e}" if name == "coef" else ""))
    for name in names:
        assert np.abs(got[name].astype(np.float64) - b[name]).max() <= b["tol_" + name], name


def run_all(x, N, P, is_u8, kw, gray=0, blocks=0, extra=2):
    """every output through the C entry point, each with `extra` sentinel rows behind it that must not change"""
    coef = torch.full((N + extra, 32, 32, P), SENTINEL, device="cuda")
    radial = torch.full((N + extra, 45, P), SENTINEL, device="cuda")
    sums = torch.full((2, 32 + extra, 32, P), SENTINEL, device="cuda", dtype=torch.float64)
    assert raw(x, N, is_u8=is_u8, gray=gray, coef=coef, radial=radial, sum1=sums[0], sum2=sums[1], blocks=blocks, **kw) == 0
    assert bool((coef[N:] == SENTINEL).all()) and bool((radial[N:] == SENTINEL).all())
    assert bool((sums[:, 32:] == SENTINEL).all())
    return dict(coef=coef[:N].cpu().numpy(), radial=radial[:N].cpu().numpy(), sum1=sums[0, :32].cpu().numpy(),
                sum2=sums[1, :32].cpu().numpy())


def test_t1_synthesised_basis_images_give_one_hot_coefficients():
    """x = D^T e_u e_v^T D per channel: a swapped u / v, a wrong accumulator-row map or mixed channels move the ones"""
    from mulan_amd import ops
    D = so.dct_matrix()
    where = ((3, 17), (17, 3), (0, 31))
    x = np.stack([np.outer(D[u], D[v]) for u, v in where], axis=-1)[None].astype(np.float32)
    coef, radial, _ = ops.spectrum(dev(x), coef=True, radial=True)
    coef, radial = coef.cpu().numpy(), radial.cpu().numpy()
    want = np.zeros((1, 32, 32, 3))
    for p, (u, v) in enumerate(where):
        want[0, u, v, p] = 1.0
    bd = so.bounds(x)
    print(f"one-hot: error {np.abs(coef - want).max():.3e}, bound {bd['tol_coef']:.3e}")
    assert np.abs(coef - want).max() <= bd["tol_coef"]
    b = so.bin_table()
    for p, (u, v) in enumerate(where):
        assert int(radial[0, :, p].argmax()) == b[u, v] and abs(radial[0, b[u, v], p] - 1.0) <= bd["tol_radial"]


def test_t2_constant_uint8_images_have_a_dc_term_only():
    from mulan_amd import ops
    levels = np.array([0, 1, 127, 128, 200, 255], dtype=np.uint8)
    x = np.broadcast_to(levels[:, None, None, None], (6, 32, 32, 3)).copy()
    coef, _, _ = ops.spectrum(dev(x), coef=True, **MODEL)
    coef = coef.cpu().numpy().astype(np.float64)
    value = so.read(levels, **MODEL)
    b = so.bounds(x, **MODEL)
    assert np.abs(coef[:, 0, 0, :] - 32.0 * value[:, None]).max() <= b["tol_coef"]
    ac = coef.copy()
    ac[:, 0, 0, :] = 0
    print(f"constant images: largest AC coefficient {np.abs(ac).max():.3e}, bound {b['tol_coef']:.3e}")
    assert np.abs(ac).max() <= b["tol_coef"] <= 4 * so.ceiling(1.0)


@pytest.mark.parametrize("kind", ("u8", "f32"))
@pytest.mark.parametrize("N", (1, 2, 3, 5, 9, 17, 33, 67))
def test_t3_random_images_every_output_against_the_oracle(kind, N):
    x, kw, b = case(kind, N)
    xd = dev(x)
    got = run_all(xd, N, 3, kind == "u8", kw)
    check(got, b, label=f"{kind} N={N}")
    if N > 4:                                   # four blocks: a block takes N / 4 images and one of them one more
        again = run_all(xd, N, 3, kind == "u8", kw, blocks=4)
        assert np.array_equal(again["coef"], got["coef"]) and np.array_equal(again["radial"], got["radial"])
        check(again, b, names=("sum1", "sum2"), label=f"{kind} N={N} blocks=4")
    from mulan_amd import ops
    c, r, s = ops.spectrum(xd, coef=True, radial=True, sums=True, **kw)            # the op gives what the entry point gives
    assert np.array_equal(c.cpu().numpy(), got["coef"]) and np.array_equal(r.cpu().numpy(), got["radial"])
    assert np.array_equal(s[0].cpu().numpy(), got["sum1"]) and np.array_equal(s[1].cpu().numpy(), got["sum2"])
    assert c.shape == (N, 32, 32, 3) and r.shape == (N, 45, 3) and s[0].dtype == torch.float64


@pytest.mark.parametrize("kind", ("u8", "f32"))
def test_t4_gray_against_the_oracle_and_dct2s_definition(kind):
    from mulan_amd import spectrum as sp
    N = 9
    x, kw, _ = case(kind, N)
    kw = dict(scale=1.0 / 255, offset=0.0) if kind == "u8" else {}
    b = so.bounds(x, gray=True, **kw)
    got = run_all(dev(x), N, 1, kind == "u8", kw, gray=1, blocks=2)
    check(got, b, label=f"gray {kind}")
    grey = (so.read(x, **kw) @ np.array(so.GRAY, dtype=np.float32).astype(np.float64))    # rgb2gray of v / 255
    want = np.einsum("uy,nyx,vx->nuv", so.dct_matrix(), grey, so.dct_matrix())
    x = x.copy()
    out = sp.dct2(x)
    assert out.shape == (N, 32, 32) and np.array_equal(out, got["coef"][..., 0])
    assert np.abs(out - want).max() <= b["tol_coef"]
    assert np.array_equal(sp.dct2(x[4]), out[4])


def test_t5_parseval_on_the_device():
    from mulan_amd import ops
    for kind in ("u8", "f32"):
        x, kw, b = case(kind, 17)
        _, radial, _ = ops.spectrum(dev(x), radial=True, **kw)
        v = so.read(x, **kw)
        energy = (v * v).sum(axis=(1, 2))
        err = np.abs(radial.cpu().numpy().astype(np.float64).sum(axis=1) - energy).max()
        print(f"Parseval {kind}: error {err:.3e}, bound {45 * b['tol_radial']:.3e}")
        assert err <= 45 * b["tol_radial"]                                          # 45 bins, each within its bound


def test_t6_accumulate_in_two_parts_equals_one_call_and_the_oracle():
    from mulan_amd import ops
    x, kw, b = case("u8", 37)
    xd = dev(x)
    _, _, whole = ops.spectrum(xd, sums=True, **kw)
    _, _, part = ops.spectrum(xd[:20], sums=True, **kw)
    keep = (part[0].data_ptr(), part[1].data_ptr())
    _, rad, both = ops.spectrum(xd[20:], radial=True, accumulate_into=part, **kw)
    assert (both[0].data_ptr(), both[1].data_ptr()) == keep and rad.shape == (17, 45, 3)          # in place
    got = dict(sum1=both[0].cpu().numpy(), sum2=both[1].cpu().numpy())
    check(got, b, names=("sum1", "sum2"), label="20 + 17")
    check(dict(sum1=whole[0].cpu().numpy(), sum2=whole[1].cpu().numpy()), b, names=("sum1", "sum2"), label="37")
    # the two differ by the order of fp64 additions only
    assert np.allclose(got["sum1"], whole[0].cpu().numpy(), rtol=0, atol=1e-12 * np.abs(b["sum1"]).max())
    assert np.allclose(got["sum2"], whole[1].cpu().numpy(), rtol=1e-13, atol=0)


def test_t7_the_same_call_twice_gives_the_same_bits():
    x, kw, _ = case("u8", 67)
    xd = dev(x)
    for blocks in (0, 5):
        a = run_all(xd, 67, 3, True, kw, blocks=blocks)
        b = run_all(xd, 67, 3, True, kw, blocks=blocks)
        assert all(a[k].tobytes() == b[k].tobytes() for k in a)
    f, kwf, _ = case("f32", 33)
    a, b = (run_all(dev(f), 33, 1, False, kwf, gray=1) for _ in range(2))
    assert all(a[k].tobytes() == b[k].tobytes() for k in a)


def test_t8_gamma_like_input_keeps_its_small_ac_part():
    """values in [-13.3, 5]: a large DC part and an AC part a thousand times smaller"""
    from mulan_amd import ops
    rng = np.random.default_rng(8)
    level = np.array([-13.3, -9.0, -4.15, 0.5, 4.9])[:, None, None, None]
    ramp = np.linspace(-1, 1, 32)[None, :, None, None] * np.linspace(1, -1, 32)[None, None, :, None]
    x = np.clip(level + 0.01 * ramp + 0.003 * rng.standard_normal((5, 32, 32, 3)), -13.3, 5.0).astype(np.float32)
    assert np.abs(x).max() == np.float32(13.3)
    b = so.bounds(x)
    coef, radial, _ = ops.spectrum(dev(x), coef=True, radial=True)
    coef = coef.cpu().numpy().astype(np.float64)
    mask = np.ones((32, 32), dtype=bool)
    mask[0, 0] = False
    err_ac = np.abs(coef - b["coef"])[:, mask].max()
    print(f"gamma-like: AC error {err_ac:.3e}, DC error {np.abs(coef - b['coef'])[:, 0, 0].max():.3e}, bound "
          f"{b['tol_coef']:.3e}, ceiling {b['ceiling']:.3e}, largest AC coefficient {np.abs(b['coef'][:, mask]).max():.3e}")
    assert b["ceiling"] == so.ceiling(np.float32(13.3)) and b["tol_coef"] <= 4 * b["ceiling"]
    assert err_ac <= b["tol_coef"] and np.abs(coef - b["coef"]).max() <= b["tol_coef"]
    assert np.abs(radial.cpu().numpy() - b["radial"]).max() <= b["tol_radial"]


def test_t9_refusals_return_the_error_and_leave_the_outputs_alone():
    """every refused call returns before a launch"""
    from mulan_amd import lib
    L = lib.load()
    N = 3
    x = torch.zeros((N, 32, 32, 3), device="cuda", dtype=torch.uint8)
    coef = torch.full((N, 32, 32, 3), SENTINEL, device="cuda")
    radial = torch.full((N, 45, 3), SENTINEL, device="cuda")
    s1, s2 = (torch.full((32, 32, 3), SENTINEL, device="cuda", dtype=torch.float64) for _ in range(2))
    ok = dict(x=x, N=N, is_u8=True, coef=coef, radial=radial, sum1=s1, sum2=s2)
    need = L.mulan_spectrum_workspace(N, 0, 0)
    assert need == N * 2 * 32 * 32 * 3 * 8 and L.mulan_spectrum_workspace(0, 0, 0) == 0
    assert L.mulan_spectrum_workspace(1100, 0, 0) == 1024 * 2 * 3072 * 8 and L.mulan_spectrum_workspace(600, 1, 7) == 7 * 2 * 1024 * 8
    small = torch.empty(need // 8, device="cuda", dtype=torch.float64)
    bad = [dict(N=0), dict(N=-1), dict(x=None), dict(coef=None, radial=None, sum1=None, sum2=None),
           dict(sum1=None, sum2=None, accumulate=1), dict(ws=small, ws_bytes=need - 8), dict(ws=None, ws_bytes=need),
           dict(ws=small, ws_bytes=0), dict(gray=2), dict(accumulate=2), dict(blocks=-1), dict(blocks=4097),
           dict(coef=coef.view(-1)[1:])]
    for change in bad:
        assert raw(**{**ok, **change}) == INVALID, change
    for t in (coef, radial, s1, s2):
        assert bool((t == SENTINEL).all())
    assert raw(**{**ok, "sum1": None, "sum2": None, "ws": None, "ws_bytes": 0}) == 0      # no sums: no workspace is read
    assert bool((s1 == SENTINEL).all()) and not bool((coef == SENTINEL).any()) and not bool((radial == SENTINEL).any())
    assert raw(**{**ok, "coef": None, "radial": None, "sum1": None}) == 0                   # one sum alone
    assert bool((s1 == SENTINEL).all()) and bool((s2 == 0).all())


# ----------------------------------------------------------------------------- model level
def _mulan_experiment():
    """a small MuLAN model with random gamma-network weights, built as tests/test_gpu_schedule_curves.py builds it"""
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
    return types.SimpleNamespace(model=vdm, orig_params=params, device=torch.device("cuda"))


def test_t10_schedule_spectrum_equals_the_oracle_on_the_curves_and_is_flat_for_a_flat_schedule():
    from mulan_amd import evaluators as ev, model as M, ops, spectrum as sp
    experiment = _mulan_experiment()
    cfg = experiment.model.config
    emb = torch.cat([ev.get_embedding(1, 50, shift=k) for k in (0, 7, 31)])
    t = np.array([0.0, 0.1, 0.35, 0.5, 0.8, 1.0], dtype=np.float32)
    res = sp.schedule_spectrum(experiment, emb, t)
    assert res["radial"].shape == (3, 6, 45, 3) and res["ac_share"].shape == (3, 6, 3) and res["radial_freq"].shape == (45,)
    assert np.array_equal(res["time_steps"], t)
    with torch.no_grad():
        a, b, c = M.poly_coefficients(experiment.orig_params["gamma"], emb.cuda())
    gamma, _, _ = ops.schedule_curves(a, b, c, dev(t), cfg.gamma_min, cfg.gamma_max)
    curves = gamma.cpu().numpy().reshape(18, 32, 32, 3)
    bd = so.bounds(curves)
    err = np.abs(res["radial"].reshape(18, 45, 3) - bd["radial"]).max()
    print(f"schedule radial: error {err:.3e}, bound {bd['tol_radial']:.3e}")
    assert err <= bd["tol_radial"]
    r64 = res["radial"].astype(np.float64)
    assert np.allclose(res["ac_share"], 1.0 - r64[:, :, 0] / r64.sum(axis=2), rtol=0, atol=1e-12)       # host arithmetic
    tol = 1023 * (so.ceiling(1.0) / 32.0) ** 2       # every AC coefficient of a flat map is an error: the ceiling beside 32 |x|
    # the fixed ends: gamma(0) = gamma_min and gamma(1) = gamma_max for every sub-pixel; in between the maps vary
    assert res["ac_share"][:, [0, -1]].max() <= tol and res["ac_share"][:, 1:-1].min() > tol
    # a schedule head that does not look at its input and has no per-pixel offsets: gamma(t) is one number per time
    flat = M.tree_map(lambda x: x.clone(), experiment.orig_params)
    for name in ("dense_out_a", "dense_out_b", "dense_out_c"):
        flat["gamma"][name]["kernel"].zero_()
        flat["gamma"][name]["bias"].zero_()
    flat_exp = types.SimpleNamespace(model=experiment.model, orig_params=flat, device=experiment.device)
    res = sp.schedule_spectrum(flat_exp, emb, t)
    print(f"flat schedule: largest ac_share {res['ac_share'].max():.3e}, bound {tol:.3e}")
    assert res["ac_share"].max() <= tol
    plain = types.SimpleNamespace(model=object.__new__(M.PlainVDM), orig_params={}, device=torch.device("cuda"))
    with pytest.raises(ValueError, match="MuLAN"):
        sp.schedule_spectrum(plain, ev.get_embedding(2))


def test_t11_image_spectrum_in_chunks_and_the_command_line(tmp_path, monkeypatch):
    from ldm import spectrum as cli
    from mulan_amd import spectrum as sp
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    rng = np.random.default_rng(12)
    samples = rng.integers(0, 256, (50, 32, 32, 3)).astype(np.uint8)
    train = (samples[::-1] // 2 + rng.integers(0, 128, samples.shape)).astype(np.uint8)
    b = so.bounds(samples, **MODEL)
    one = sp.image_spectrum(samples, chunk=1000, keep_radial=True)
    parts = sp.image_spectrum(samples, chunk=16, keep_radial=True)
    for got in (one, parts):
        assert np.abs(got["coef_mean"] - b["sum1"] / 50).max() <= b["tol_sum1"] / 50
        assert np.abs(got["power_mean"] - b["sum2"] / 50).max() <= b["tol_sum2"] / 50
        assert np.abs(got["radial"] - b["radial"]).max() <= b["tol_radial"] and got["n"] == 50
        assert np.abs(got["radial_mean"] - b["radial"].mean(axis=0)).max() <= 50 * b["tol_sum2"] / 50   # <= 50 members a bin
    assert np.array_equal(one["radial"], parts["radial"])
    assert np.allclose(one["power_mean"], parts["power_mean"], rtol=1e-13, atol=0)
    np.savez(tmp_path / "s.npz", images=samples)
    np.savez(tmp_path / "t.npz", images=train)
    out = tmp_path / "spectrum.npz"
    assert cli.main([f"--samples={tmp_path / 's.npz'}", f"--reference=npz:{tmp_path / 't.npz'}", f"--out={out}",
                     "--chunk=32"]) == 0
    want = sp.compare_spectra(parts, sp.image_spectrum(train))
    with np.load(out) as f:
        assert int(f["samples_n"]) == 50 and int(f["reference_n"]) == 50 and f["log_ratio"].shape == (45, 3)
        assert np.isclose(float(f["lsd_db"]), want["lsd_db"], rtol=1e-9)
        assert np.isclose(float(f["frechet_diag"]), want["frechet_diag"], rtol=1e-9)
        assert np.isclose(float(f["high_band_ratio"]), want["high_band_ratio"], rtol=1e-9)
