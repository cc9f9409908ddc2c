"""tests/loss_head_oracle.py without a device: its float64 functions against oracle/torch_ref.py where they overlap and
against the golden fixture tests/test_gpu_golden.py reads, and every case of its table against the usability condition --
the twin (the same functions in float32) deviates from float64, by the measure the GPU test uses, by a finite amount
below 1e-4.  A case that broke the condition was narrowed (the comment on G1_ROWS in the oracle states the one
exclusion); the bound stays."""
import os

import numpy as np
import pytest
import torch

from oracle import torch_ref as tr
from tests import loss_head_oracle as lo

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
t64 = lambda a: torch.tensor(np.asarray(a), dtype=torch.float64)


def test_new_functions_agree_with_torch_ref_and_the_golden_fixture():
    z = np.load(os.path.join(GOLD, "closed_forms.npz"))
    B = z["t"].shape[0]
    a, b, c, t = (t64(z[k]) for k in "abct")
    flat = lambda k: t64(z[k]).reshape(B, -1)
    g0 = tr.poly_gamma(a, b, c, torch.zeros(B, dtype=torch.float64))
    g1 = tr.poly_gamma(a, b, c, torch.ones(B, dtype=torch.float64))
    gt, gp = tr.poly_gamma(a, b, c, t), tr.poly_gamma_grad_t(a, b, c, t)
    assert np.abs(gt.numpy() - z["g_t"].reshape(B, -1)).max() < 1e-12
    x = torch.tensor(z["x"].reshape(B, -1).astype(np.int64))
    out, add = lo.qsample_terms(x, g0, g1, gt, flat("eps_0"), flat("eps"))
    rel = lambda got, want: float(np.abs(np.asarray(got) - np.asarray(want)).max() / np.abs(np.asarray(want)).max())
    assert rel(out["zt"].numpy(), z["z_t"].reshape(B, -1)) < 1e-12
    assert rel(out["recon"].numpy(), z["loss_recon"]) < 1e-12 and rel(out["klz"].numpy(), z["loss_klz"]) < 1e-12
    assert rel(out["var0"].mean().numpy(), z["var_0"].mean()) < 1e-12 and rel(out["var1"].mean().numpy(), z["var_1"].mean()) < 1e-12
    for mode, key in ((0, "loss_diff_velocity"), (1, "loss_diff_vfe"), (2, "loss_diff_epsilon")):
        el = lo.diffusion_loss_elements(mode, x, gt, gp, flat("eps"), out["zt"], flat("net"))
        assert rel(el.sum(1).numpy(), z[key]) < 1e-12, key
    # torch_ref's own pieces: encode and logprob (whole samples at once), and the sums against their addends
    f = tr.encode(x.double())
    z0 = f + torch.exp(0.5 * g0) * flat("eps_0")
    assert rel(out["recon"].numpy(), -tr.logprob(x, z0, g0).numpy()) < 1e-13
    assert rel(add["klz"].sum(1).numpy(), out["klz"].numpy()) < 1e-15 and rel(add["gbar"].sum(1).numpy(), out["gbar"].numpy()) < 1e-13
    # the exact target leaves no residual, in every mode
    for mode in (0, 1, 2):
        net = lo.exact_net(mode, x, gt, flat("eps"), out["zt"])
        assert float(lo.diffusion_loss_elements(mode, x, gt, gp, flat("eps"), out["zt"], net).abs().max()) < 1e-25
    # T expm1 is torch_ref.mulan_forward's weight
    w = lo.expm1_weight(gt, gt - 0.01, 1000.0)
    assert rel(w.numpy(), (1000.0 * torch.expm1(torch.full_like(gt, 0.01))).numpy()) < 1e-12


def test_the_case_table_has_every_row_with_every_kernel():
    qs, dl = lo.QSAMPLE_CASES, lo.DIFFLOSS_CASES
    for pe in (0, 1):
        sel = [c for c in qs if c.per_elem == pe and c.B == 6]
        assert {c.image for c in sel} == set(lo.IMAGES) and {c.g0 for c in sel} == set(lo.G0_MEANS)
        assert {c.g1 for c in sel} == set(lo.G1_ROWS)
    assert {c.B for c in qs} == {1, 6} and all(c.g1 == "2" for c in qs if c.image == "128")
    for mode in (0, 1, 2):
        sel = [c for c in dl if c.mode == mode]
        assert {(c.per_elem, c.weight) for c in sel if c.B == 6} == {(p, w) for p in (0, 1) for w in ("uniform", "expm1")}
        assert {c.B for c in sel} == {1, 6} and (mode == 2 or {c.image for c in sel} == set(lo.IMAGES))
    assert {(c.noise, c.L, c.k) for c in lo.TOPK_CASES} == {(n, L, k) for n in ("gamma", "additive", "none")
                                                            for L in (50, 64) for k in (1, 15, L)}
    assert {c.B for c in lo.TOPK_CASES} == {1, 7}
    for cases in (qs, dl, lo.POLY_CASES, lo.TOPK_CASES):
        assert len(lo.by_name(cases)) == len(cases)
    # the scalar layout gives every sample another gamma_t; the per-element layout has the five rows and the drawn one
    inp = lo.qsample_inputs(next(c for c in qs if c.B == 6 and not c.per_elem))
    assert inp["gt"].shape == (6,) and len(set(inp["gt"].tolist())) == 6
    assert inp["gt"][:5].tolist() == [float(np.float32(v)) for v in lo.GAMMA_T_ROWS]
    halves = lo.image("halves", 1, np.random.default_rng(0)).reshape(32, 32, 3)
    assert (halves[:, :16] == 0).all() and (halves[:, 16:] == 255).all()


def usable(family, name, names=None):
    _, ref, twin = lo.reference(family, name)
    dev = lo.errors(twin, ref, names or [n for n in ref if n not in ("hard", "gap")])
    for n, e in dev.items():
        print(f"{family} {name} {n}: twin deviation per sample {np.array2string(e, precision=2)}")
    for n, e in dev.items():
        assert np.isfinite(e).all() and float(e.max()) < lo.USABLE, (name, n, e)
    return ref, twin


@pytest.mark.parametrize("name", [c.name for c in lo.QSAMPLE_CASES])
def test_qsample_cases_are_usable(name):
    usable("qsample", name)


@pytest.mark.parametrize("name", [c.name for c in lo.DIFFLOSS_CASES])
def test_diffloss_cases_are_usable(name):
    usable("diffloss", name)


@pytest.mark.parametrize("name", [c.name for c in lo.POLY_CASES])
def test_poly_cases_are_usable(name):
    ref, _ = usable("poly", name)
    assert np.abs(ref["g1"] - 5.0).max() < 1e-12 and np.abs(ref["gt"][1] - 5.0).max() < 1e-12


@pytest.mark.parametrize("name", [c.name for c in lo.TOPK_CASES])
def test_topk_cases_are_usable(name):
    """and the hard set is the same in fp32: no threshold sits within rounding of the next logit"""
    ref, twin = usable("topk", name)
    c = lo.by_name(lo.TOPK_CASES)[name]
    assert np.array_equal(ref["hard"], twin["hard"])
    ones = ref["hard"].sum(1)
    want = np.full(c.B, c.k)
    if c.noise == "none" and c.B > lo.TIE_ROW and c.k < c.L:
        want[lo.TIE_ROW] = c.k + 1
    assert np.array_equal(ones, want)
    if "gap" in ref:
        assert float(ref["gap"].min()) > 1e-4
