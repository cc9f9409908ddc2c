"""The convolution half of tests/f16x3_oracle.py held to its own definitions and to the project's float64 oracles, and
the condition that keeps the bars of tests/test_gpu_conv_f16x3.py honest: on every non-integer input set the GPU tests
use (tests/f16x3_conv_cases.py), the kernels' arithmetic WITH AN EXACT ACCUMULATOR already lies within half of the bar.
What a GPU run may add to that is the fp32 accumulation and the result's own rounding."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import mulan_np as onp
from oracle import torch_ref as tr
from tests import f16x3_conv_cases as cases
from tests import f16x3_oracle as fo


@pytest.mark.parametrize("C,N", [(16, 128), (48, 128), (128, 256)])
def test_conv_pack_index_is_a_bijection(C, N):
    idx = fo.conv_pack_index(C, N)
    assert idx.shape == (9, C, N, 2)
    assert np.array_equal(np.sort(idx.ravel()), np.arange(9 * C * N * 2))
    # the documented nesting [9][C/16][N][plane][16]
    t, kin, o = 7, C - 3, N - 5
    assert idx[t, kin, o, 1] == ((((t * (C // 16) + kin // 16) * N + o) * 2) + 1) * 16 + kin % 16


def test_pack_conv_flip_is_the_pack_of_the_flipped_and_transposed_tensor():
    rng = np.random.default_rng(0)
    w = (rng.standard_normal((3, 3, 48, 32)) * 0.1).astype(np.float32)
    wt = np.empty((3, 3, 32, 48), np.float32)
    for t in range(9):
        for c in range(48):
            wt[t // 3, t % 3, :, c] = w[(8 - t) // 3, (8 - t) % 3, c, :]            # wT[t][n][c] = w[8 - t][c][n], spelt out
    assert np.array_equal(wt, fo.flip_conv(w))
    a, ma = fo.pack_conv(w, 1)
    b, mb = fo.pack_conv(wt, 0)
    assert ma == mb and np.array_equal(a.view(np.uint16), b.view(np.uint16))
    h, l = fo.unpack_conv(a, 32, 48)
    vs = wt.reshape(9, 32, 48) * fo.scale_of(ma)[0]
    assert np.all(np.abs(h.astype(np.float64) + l.astype(np.float64) - vs) <= fo.split_bound(vs))
    c, _ = fo.pack_conv(w, 0)
    assert not np.array_equal(a.view(np.uint16), c.view(np.uint16))


def test_conv_planes_are_the_dense_planes_with_rows_h_times_w():
    rng = np.random.default_rng(1)
    x = rng.standard_normal((2, 8, 32, 48)).astype(np.float32)
    x[1] *= 1e-7
    planes = fo.conv_planes(x)
    h, l = fo.unplane(planes, 2, 48, 256)
    vs = fo.scaled(x.reshape(2, 256, 48))
    assert np.all(np.abs(h.astype(np.float64) + l.astype(np.float64) - vs) <= fo.split_bound(vs))
    assert planes[fo.plane_index(2, 48, 256)[1, 5 * 32 + 7, 33, 0]] == fo.split2(vs[1, 5 * 32 + 7, 33])[0]


@pytest.mark.parametrize("H", [8, 24, 32])
def test_references_agree_with_the_float64_oracles(H):
    """conv_ref, dgrad_ref, wgrad_ref against oracle.mulan_np.conv3x3 (same nine products), against a direct float64
    conv2d and its autograd, and at H = 32 against oracle.torch_ref.conv3x3"""
    rng = np.random.default_rng(H)
    B, C, N = 2, 16, 24
    x, w = rng.standard_normal((B, H, 32, C)), rng.standard_normal((3, 3, C, N))
    dy = rng.standard_normal((B, H, 32, N))
    bias, cb, res = rng.standard_normal(N), rng.standard_normal((B, N)), rng.standard_normal((B, H, 32, N))
    x, w, dy, bias, cb, res = (fo.f32(t) for t in (x, w, dy, bias, cb, res))
    ref, mag = fo.conv_ref(x, w, bias, cb, res)
    assert np.allclose(ref, onp.conv3x3(x, w, bias) + cb[:, None, None, :] + res, rtol=1e-12, atol=1e-12)
    assert np.allclose(mag, onp.conv3x3(np.abs(x), np.abs(w), np.abs(bias)) + np.abs(cb)[:, None, None, :] + np.abs(res),
                       rtol=1e-12, atol=1e-12)
    ref2, _ = fo.conv_ref(x, w, None, res, None)                                # a per-pixel cbias
    assert np.allclose(ref2, onp.conv3x3(x, w) + res, rtol=1e-12, atol=1e-12)
    xt, wt = torch.tensor(x, requires_grad=True), torch.tensor(w, requires_grad=True)
    y = F.conv2d(xt.permute(0, 3, 1, 2), wt.permute(3, 2, 0, 1), padding=1).permute(0, 2, 3, 1)
    y.backward(torch.tensor(dy))
    assert np.allclose(fo.conv_ref(x, w)[0], y.detach().numpy(), rtol=1e-12, atol=1e-12)
    dx, dmag = fo.dgrad_ref(dy, w)
    dw, wmag = fo.wgrad_ref(x, dy)
    assert np.allclose(dx, xt.grad.numpy(), rtol=1e-12, atol=1e-12)
    assert np.allclose(dw, wt.grad.numpy(), rtol=1e-12, atol=1e-11)
    assert np.all(dmag >= np.abs(dx)) and np.all(wmag >= np.abs(dw))
    if H == 32:
        xt2, wt2 = torch.tensor(x, requires_grad=True), torch.tensor(w, requires_grad=True)
        y2 = tr.conv3x3(xt2, {"kernel": wt2})
        y2.backward(torch.tensor(dy))
        assert np.allclose(fo.conv_ref(x, w)[0], y2.detach().numpy(), rtol=1e-12, atol=1e-12)
        assert np.allclose(dx, xt2.grad.numpy(), rtol=1e-12, atol=1e-12)
        assert np.allclose(dw, wt2.grad.numpy(), rtol=1e-12, atol=1e-11)


def test_models_are_exact_on_integers():
    rng = np.random.default_rng(3)
    x = rng.integers(-3, 4, (2, 8, 32, 16)) * 2.0 ** np.array([0, 20])[:, None, None, None]
    w = rng.integers(-2, 3, (3, 3, 16, 8)).astype(np.float64)
    dy = rng.integers(-2, 3, (2, 8, 32, 8)) * 2.0 ** np.array([-7, 3])[:, None, None, None]
    assert np.array_equal(fo.model_conv(x, w), fo.conv_ref(x, w)[0])
    assert np.array_equal(fo.model_dgrad(dy, w), fo.dgrad_ref(dy, w)[0])
    for per_image in (False, True):
        assert np.array_equal(fo.model_wgrad(x, dy, per_image), fo.wgrad_ref(x, dy)[0])


def test_the_clamp_sets_are_what_they_claim():
    s = cases.conv_case("clamp_small")
    m = np.abs(s["x"]).reshape(4, -1).max(axis=1)
    assert m[0] == 1.0 and m[1] == 2.0 ** -120 and 0 < m[2] < 2.0 ** -126 and m[3] == 0.0
    assert fo.clamped(s["x"]).tolist() == [False, True, True, True]
    assert fo.clamped(s["dy"]).tolist() == [False, True, True, True]
    b = cases.conv_case("clamp_big")
    assert np.abs(b["x"]).reshape(4, -1).max(axis=1).tolist() == [1.0, 2.0 ** 120, 2.0 ** -120, np.float32(1e-3)]
    for s in (s, b):                                        # every reference of the set is finite in fp32
        for ref in (fo.conv_ref(s["x"], s["w"])[0], fo.conv_ref(s["x"], s["w"], s["bias"], s["cbias"], s["res"])[0],
                    fo.dgrad_ref(s["dy"], s["w"])[0], fo.wgrad_ref(s["x"], s["g"])[0], fo.wgrad_ref(s["xg"], s["dy"])[0]):
            assert np.all(np.isfinite(ref.astype(np.float32)))


@pytest.mark.parametrize("name", sorted(cases.CASES))
def test_the_exact_accumulator_model_lies_within_half_of_every_bar(name):
    """the condition behind the bars of tests/test_gpu_conv_f16x3.py.  Forward and input gradient: per image and element
    within MODEL_SHARE of 3e-6 mag (+ the floor of the split for the images under the clamp); weight gradients, with the
    tensor-wide scales of the nine-tap kernel and the per-image scales of the plane-fed one: within MODEL_SHARE of
    3e-6 |x|^T |dy| per element and tap."""
    s = cases.conv_case(name)
    x, w, dy = s["x"], s["w"], s["dy"]
    for got, (ref, mag), img in ((fo.model_conv(x, w), fo.conv_ref(x, w), x),
                                 (fo.model_conv(x, w, s["bias"], s["cbias"], s["res"]),
                                  fo.conv_ref(x, w, s["bias"], s["cbias"], s["res"]), x),
                                 (fo.model_dgrad(dy, w), fo.dgrad_ref(dy, w), dy)):
        bar = cases.image_bar(fo, img, fo.flip_conv(w) if img is dy else w, mag)
        err = np.abs(got - ref)
        ratio = np.where(bar > 0, err / np.where(bar > 0, bar, 1), np.where(err > 0, np.inf, 0.0))
        print(name, "model: worst error / bar per image", ratio.reshape(s["B"], -1).max(axis=1))
        assert float(ratio.max()) <= cases.MODEL_SHARE
    zero = np.abs(x).reshape(s["B"], -1).max(axis=1) == 0
    assert not np.any(fo.model_conv(x, w)[zero])
    for a, b in ((x, s["g"]), (s["xg"], dy)):
        ref, mag = fo.wgrad_ref(a, b)
        for per_image in (False, True):
            ratio = float((np.abs(fo.model_wgrad(a, b, per_image) - ref) / mag).max())
            print(name, "model dw, per-image scales" if per_image else "model dw, tensor scales", f"{ratio:.3e}")
            assert ratio <= cases.MODEL_SHARE * cases.BAR
