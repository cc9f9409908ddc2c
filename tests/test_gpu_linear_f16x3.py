"""The f16x3 per-pixel dense kernels (mulan_amd/csrc/linear_f16x3.hip: mulan_linear_f16x3, its batched form and the two
pack entry points) and the weight gradients that read the planes they hand on (mulan_linear_wgrad_f16x3_planes / _x32,
mulan_bmm_tn_f16x3_planes), off the model's shapes: rows per image from 128, odd stage counts and uneven concats,
every pairing of one or two outputs with the 128- and 256-column blocks, bias with two outputs, `res` on the batched
call, `accumulate`, the scale clamps, and the argument checks.  The reference is the host model tests/f16x3_oracle.py:
float64 on the fp32-rounded inputs for the results, the bits of the documented layouts for packs and planes.

Every output buffer is followed by a guard band of 4096 sentinel bytes that must survive the launch.  The four
instantiations of the dense kernel (128 / 256 columns x 64 / 128 rows per block) are selected with tune keys 11 and 28.

Bars: integer data is exact; Gaussian data is held to the bars of tests/test_gpu_f16x3.py for these kernels (2e-6 of
sum |x||w| + |bias| + |res| for the products, 3e-6 of |x|^T |dy| for the weight gradients); planes and packs of Gaussian
data to the reconstruction bound of the split, 2^-22 |vs| + 2^-25 (tests/test_f16x3_oracle.py)."""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import f16x3_oracle as fo

GUARD = 4096
FILL = 0xA5
TUNES = ((0, 0), (1, 0), (0, 1), (1, 1))          # (tune[11]: 128-column blocks everywhere, tune[28]: 128-row blocks everywhere)


@pytest.fixture()
def ops(monkeypatch):
    from mulan_amd import ops as _ops
    _ops.lib.load()
    monkeypatch.setattr(_ops, "CONV_MODE", "f16x3")
    yield _ops
    _ops.call("mulan_set_tuning", 11, 0)
    _ops.call("mulan_set_tuning", 28, 0)


def set_tune(ops, t11, t28):
    ops.call("mulan_set_tuning", 11, t11)
    ops.call("mulan_set_tuning", 28, t28)


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a)).float().cuda()


class Buf:
    """an output buffer of nbytes, filled with the sentinel byte and followed by a guard band of the same"""

    def __init__(self, nbytes):
        self.n = int(nbytes)
        self.raw = torch.full((self.n + GUARD,), FILL, dtype=torch.uint8, device="cuda")

    @property
    def ptr(self):
        return self.raw.data_ptr()

    @property
    def body(self):
        return self.raw[:self.n]

    def f32(self, *shape):
        return self.body.view(torch.float32).view(*shape)

    def np_f32(self, *shape):
        return self.f32(*shape).cpu().numpy()

    def np_f16(self):
        return self.body.cpu().numpy().view(np.float16)

    def guard_ok(self):
        return bool((self.raw[self.n:] == FILL).all())

    def untouched(self):
        return bool((self.raw == FILL).all())


def bufptr(b):
    return None if b is None else b.ptr


def maxima(ops, t, B):
    return ops.absmax_rows(t.reshape(B, -1))


def pack(ops, w, transpose):
    """w [K, N], or [N, K] with transpose -> (Buf of the packed operand, wmax [1][16])"""
    K, N = (w.shape[1], w.shape[0]) if transpose else w.shape
    wmax = maxima(ops, w, 1)
    wp = Buf(ops.lib.load().mulan_linear_pack_f16x3_bytes(K, N))
    ops.call("mulan_linear_pack_f16x3", ops.ptr(w), wp.ptr, ops.ptr(wmax), K, N, int(transpose), ops.stream())
    torch.cuda.synchronize()
    assert wp.guard_ok()
    return wp, wmax


def pack_batched(ops, w, transpose):
    """w [B, K, N], or [B, N, K] with transpose -> (Buf of the B packed operands, wmax [B][16])"""
    B = w.shape[0]
    K, N = (w.shape[2], w.shape[1]) if transpose else (w.shape[1], w.shape[2])
    wmax = maxima(ops, w, B)
    wp = Buf(B * K * N * 4)
    ops.call("mulan_linear_pack_f16x3_batched", ops.ptr(w), wp.ptr, ops.ptr(wmax), K, N, int(transpose), B, ops.stream())
    torch.cuda.synchronize()
    assert wp.guard_ok()
    return wp, wmax


def dense(ops, x1, x2, wp, wmax, N1, N2, rows, bias=None, res=None, want_xs=False, batched=False):
    """the C entry points on tensors allocated here: x1 [M, K1], x2 [M, K2] or None -> (y1, y2, xs) as Bufs"""
    M, K1 = x1.shape
    K2 = 0 if x2 is None else x2.shape[1]
    B = M // rows
    m1 = maxima(ops, x1, B)
    m2 = maxima(ops, x2, B) if K2 else None
    y1 = Buf(M * N1 * 4)
    y2 = Buf(M * N2 * 4) if N2 else None
    xs = Buf(M * (K1 + K2) * 4) if want_xs else None
    if batched:
        assert K2 == 0 and N2 == 0 and bias is None
        ops.call("mulan_linear_f16x3_batched", ops.ptr(x1), ops.ptr(m1), K1, wp.ptr, ops.ptr(wmax), ops.ptr(res), y1.ptr,
                 bufptr(xs), N1, M, rows, ops.stream())
    else:
        ops.call("mulan_linear_f16x3", ops.ptr(x1), ops.ptr(m1), ops.ptr(x2), ops.ptr(m2), K1, K2, wp.ptr, ops.ptr(wmax),
                 ops.ptr(bias), ops.ptr(res), y1.ptr, bufptr(y2), bufptr(xs), N1, N2, M, rows, ops.stream())
    torch.cuda.synchronize()
    for b in (y1, y2, xs):
        assert b is None or b.guard_ok()
    return y1, y2, xs


def outputs(y1, y2, M, N1, N2):
    y = y1.np_f32(M, N1)
    return y if y2 is None else np.concatenate([y, y2.np_f32(M, N2)], axis=1)


def img_pow(b):
    """image b is multiplied by 2^(20 (-1)^b (b % 3)): neighbours differ by up to 2^40"""
    return 20 * (-1) ** b * (b % 3)


# (rows_per_img, B, K1, K2, N1, N2, bias, res, xs): every value of every axis of the issue's lists, and the pairings
# (rows 128, K 32, N (128, 128)), (rows 384, K (32, 96), N (128, 384)), (rows 256, K (256, 128), N 384, bias + res)
SHAPES = [
    (128, 6, 32, 0, 128, 128, 1, 0, 1),
    (384, 4, 32, 96, 128, 384, 1, 0, 1),
    (256, 3, 256, 128, 384, 0, 1, 1, 0),
    (128, 1, 64, 0, 128, 0, 0, 0, 0),
    (1024, 1, 96, 0, 256, 0, 1, 1, 1),
    (128, 6, 160, 0, 512, 0, 0, 1, 1),
    (256, 3, 32, 32, 128, 256, 1, 0, 0),
    (384, 4, 96, 32, 256, 128, 0, 0, 1),
    (128, 6, 128, 256, 128, 0, 1, 1, 1),
    (1024, 1, 256, 128, 128, 128, 0, 0, 0),
    (256, 3, 32, 0, 256, 0, 0, 0, 1),
    (128, 6, 32, 96, 384, 0, 1, 0, 1),
    (384, 4, 160, 0, 128, 384, 1, 0, 0),
    (128, 1, 96, 0, 512, 0, 0, 1, 1),
    (128, 6, 256, 128, 256, 128, 1, 0, 1),
]


# ------------------------------------------------------------------------------------------------ a. exact on integers
@pytest.mark.parametrize("rows,B,K1,K2,N1,N2,use_bias,use_res,want_xs", SHAPES)
def test_dense_exact_on_integers_under_all_four_instantiations(ops, rows, B, K1, K2, N1, N2, use_bias, use_res, want_xs):
    """x in [-3, 3], w in [-2, 2], bias and res in [-3, 3]; image b (and its res) times 2^(20 (-1)^b (b % 3)), the second
    concat half times 2^+-4 so that either half's maximum decides the scale.  Every product and partial sum is an
    integer times a power of two below 2^24, so the kernel's only rounding is the final fp32 add of bias + res: under
    all four instantiations the result equals the float64 reference rounded once to fp32, which IS the float64 reference
    wherever that is an fp32 number (asserted for every case without a bias; with a bias a 2^40 image cannot hold
    n 2^40 + 3 in 24 bits).  The planes are the oracle's bits, with l == 0."""
    rng = np.random.default_rng(rows + 7 * B + K1 + 3 * K2 + 5 * N1 + 11 * N2)
    M, K, N = rows * B, K1 + K2, N1 + N2
    f = 2.0 ** np.array([img_pow(b) for b in range(B)])[:, None, None]
    x = rng.integers(-3, 4, (B, rows, K)).astype(np.float64)
    x[..., K1:] *= 2.0 ** (4 if (K1 // 32) % 2 else -4)
    x = (x * f).reshape(M, K)
    w = rng.integers(-2, 3, (K, N)).astype(np.float64)
    bias = rng.integers(-3, 4, N).astype(np.float64) if use_bias else None
    # (res follows its image's power of two, except beside a bias: bias + res must stay one exact fp32 number)
    res = (rng.integers(-3, 4, (B, rows, N1)) * (1.0 if use_bias else f)).reshape(M, N1) if use_res else None
    assert not (use_res and N2)
    ref, _ = fo.dense_ref(x[:, :K1], x[:, K1:] if K2 else None, w, bias, res)
    want = ref.astype(np.float32)
    if not use_bias:
        assert np.array_equal(want.astype(np.float64), ref)
    x1d, x2d = dev(x[:, :K1]), (dev(x[:, K1:]) if K2 else None)
    wp, wmax = pack(ops, dev(w), False)
    planes = fo.planes_of(x[:, :K1], x[:, K1:] if K2 else None, rows)
    assert not np.any(fo.unplane(planes, B, K, rows)[1])
    for t11, t28 in TUNES:
        set_tune(ops, t11, t28)
        y1, y2, xs = dense(ops, x1d, x2d, wp, wmax, N1, N2, rows, bias=None if bias is None else dev(bias),
                           res=None if res is None else dev(res), want_xs=bool(want_xs))
        got = outputs(y1, y2, M, N1, N2)
        bad = np.argwhere(got != want)
        assert bad.size == 0, (t11, t28, len(bad), bad[:4].tolist())
        if want_xs:
            assert np.array_equal(xs.np_f16().view(np.uint16), planes.view(np.uint16)), (t11, t28)


# ------------------------------------------------------------------------------------------------ b. accuracy
@pytest.mark.parametrize("rows,B,K1,K2,N1,N2,use_bias,use_res,want_xs", SHAPES)
def test_dense_accuracy_on_gaussian_data(ops, rows, B, K1, K2, N1, N2, use_bias, use_res, want_xs):
    """per image max |y - ref| / (|x| @ |w| + |bias| + |res|) < 2e-6 (the bar of
    test_f16x3_linear_exact_on_integers_and_accuracy) with per-image magnitudes from 1e-4 to 1e3, the same bar on
    dx = dy @ w^T split into two outputs where the concat halves allow it, and the planes within the split's
    reconstruction bound of x * s"""
    rng = np.random.default_rng(rows + 7 * B + K1 + 3 * K2 + 5 * N1 + 11 * N2 + 1)
    M, K, N = rows * B, K1 + K2, N1 + N2
    scales = np.resize(np.array([1.0, 1e-4, 300.0, 1e3, 1e-2, 30.0]), B)[:, None, None]
    x = rng.standard_normal((B, rows, K)) * scales
    if (K1, K2) == (32, 96):
        x[..., K1:] *= 1e-3                                  # the second half far below the first: one scale serves both
    x = x.reshape(M, K).astype(np.float32)
    w = (rng.standard_normal((K, N)) / math.sqrt(K)).astype(np.float32)
    bias = rng.standard_normal(N).astype(np.float32) if use_bias else None
    res = (rng.standard_normal((B, rows, N1)) * scales).reshape(M, N1).astype(np.float32) if use_res else None
    ref, mag = fo.dense_ref(x[:, :K1], x[:, K1:] if K2 else None, w, bias, res)
    x1d, x2d = dev(x[:, :K1]), (dev(x[:, K1:]) if K2 else None)
    wd = dev(w)
    wp, wmax = pack(ops, wd, False)
    worst = 0.0
    for t11, t28 in ((0, 0), (1, 1)):
        set_tune(ops, t11, t28)
        y1, y2, xs = dense(ops, x1d, x2d, wp, wmax, N1, N2, rows, bias=None if bias is None else dev(bias),
                           res=None if res is None else dev(res), want_xs=True)
        got = outputs(y1, y2, M, N1, N2).astype(np.float64)
        assert np.all(np.isfinite(got))
        err = (np.abs(got - ref) / mag).reshape(B, -1).max(axis=1)
        worst = max(worst, float(err.max()))
    print(f"dense y: worst per-image error / mag = {worst:.3e} (bar 2e-6)")
    h, l = fo.unplane(xs.np_f16(), B, K, rows)
    vs = fo.scaled(x.reshape(B, rows, K))
    rec = np.abs(h.astype(np.float64) + l.astype(np.float64) - vs) / fo.split_bound(vs)
    print(f"planes: worst reconstruction error / bound = {float(rec.max()):.3f}")
    worst_dx = None
    if K1 % 128 == 0 and K2 % 128 == 0:
        dscales = np.resize(np.array([1e-5, 1.0, 7.0, 1e2, 3e-3, 1.0]), B)[:, None, None]
        dy = (rng.standard_normal((B, rows, N)) * dscales).reshape(M, N).astype(np.float32)
        wpt, wmaxt = pack(ops, wd, True)                    # w is [K, N]: the operand of dy @ w^T has N input channels
        set_tune(ops, 0, 0)
        d1, d2, _ = dense(ops, dev(dy), None, wpt, wmaxt, K1, K2, rows)
        dxr, dmag = fo.dense_ref(dy, None, w.T)
        gdx = outputs(d1, d2, M, K1, K2).astype(np.float64)
        assert np.all(np.isfinite(gdx))
        worst_dx = float((np.abs(gdx - dxr) / dmag).max())
        print(f"dense dx: worst error / mag = {worst_dx:.3e} (bar 2e-6)")
    assert worst < 2e-6
    assert float(rec.max()) <= 1.0
    assert worst_dx is None or worst_dx < 2e-6


# ------------------------------------------------------------------------------------------------ c. covariance
COV = ((-60, 40), (60, -40), (-60, -40), (60, 40), (0, 0))


def _in_range(ref):
    a = np.abs(ref)
    return bool(np.all((a == 0) | ((a >= 2.0 ** -100) & (a <= 2.0 ** 100))))


@pytest.mark.parametrize("rows,B,K1,K2,N1,N2", [(128, 3, 32, 96, 128, 128), (256, 3, 160, 0, 384, 0), (128, 2, 64, 0, 256, 0)])
def test_dense_power_of_two_covariance_is_bitwise(ops, rows, B, K1, K2, N1, N2):
    """what the power-of-two scales buy: image j of x times 2^a and w times 2^c gives image j times exactly 2^(a + c) and
    every other image times exactly 2^c (unchanged for c = 0), bit for bit, as long as no value leaves the normal range.
    The base magnitude of image j is chosen per (a, c) so that the float64 reference of the scaled run lies in
    [2^-100, 2^100] (asserted)."""
    rng = np.random.default_rng(rows + B + K1 + N1)
    M, K, N = rows * B, K1 + K2, N1 + N2
    j = B - 2
    x0 = rng.standard_normal((B, rows, K)).astype(np.float32)
    w0 = (rng.standard_normal((K, N)) / math.sqrt(K)).astype(np.float32)
    for a, c in COV:
        xb = x0.copy()
        xb[j] *= np.float32(2.0 ** (-(a + c) * 3 // 10))
        xs_, ws_ = xb.copy(), w0 * np.float32(2.0 ** c)
        xs_[j] *= np.float32(2.0 ** a)
        for t in (xb, xs_, w0, ws_):                               # the scalings themselves were exact
            assert np.all(np.isfinite(t)) and np.all((t == 0) | (np.abs(t) >= 2.0 ** -126))
        ref, _ = fo.dense_ref(xs_.reshape(M, K)[:, :K1], xs_.reshape(M, K)[:, K1:] if K2 else None, ws_)
        assert _in_range(ref), (a, c)
        outs = []
        for xv, wv in ((xb, w0), (xs_, ws_)):
            xv = xv.reshape(M, K)
            wp, wmax = pack(ops, dev(wv), False)
            y1, y2, _ = dense(ops, dev(xv[:, :K1]), dev(xv[:, K1:]) if K2 else None, wp, wmax, N1, N2, rows)
            outs.append(torch.cat([y1.f32(M, N1)] + ([y2.f32(M, N2)] if N2 else []), dim=1).view(B, rows, N).clone())
        y0, ys = outs
        assert bool(torch.isfinite(ys).all())
        for b in range(B):
            want = y0[b] * (2.0 ** (a + c) if b == j else 2.0 ** c)
            assert torch.equal(ys[b], want), (a, c, b)


@pytest.mark.parametrize("rows,B,K,N,transpose", [(128, 3, 128, 256, False), (256, 3, 32, 128, True)])
def test_batched_power_of_two_covariance_is_bitwise(ops, rows, B, K, N, transpose):
    """the batched call, the scales on x[j] and on w[j] alone: image j times exactly 2^(a + c), all others the same bits"""
    rng = np.random.default_rng(rows + B + K + N)
    M, j = rows * B, 1
    x0 = rng.standard_normal((B, rows, K)).astype(np.float32)
    w0 = (rng.standard_normal((B, K, N)) / math.sqrt(K)).astype(np.float32)
    stored = (lambda w: np.ascontiguousarray(w.transpose(0, 2, 1))) if transpose else (lambda w: w)
    for a, c in COV:
        xb, ws_ = x0.copy(), w0.copy()
        xb[j] *= np.float32(2.0 ** (-(a + c) * 3 // 10))
        xs_ = xb.copy()
        xs_[j] *= np.float32(2.0 ** a)
        ws_[j] *= np.float32(2.0 ** c)
        for t in (xb, xs_, ws_):
            assert np.all(np.isfinite(t)) and np.all((t == 0) | (np.abs(t) >= 2.0 ** -126))
        ref, _ = fo.dense_ref(xs_, None, ws_)
        assert _in_range(ref), (a, c)
        outs = []
        for xv, wv in ((xb, w0), (xs_, ws_)):
            wp, wmax = pack_batched(ops, dev(stored(wv)), transpose)
            y1, _, _ = dense(ops, dev(xv.reshape(M, K)), None, wp, wmax, N, 0, rows, batched=True)
            outs.append(y1.f32(B, rows, N).clone())
        y0, ys = outs
        assert bool(torch.isfinite(ys).all())
        for b in range(B):
            assert torch.equal(ys[b], y0[b] * 2.0 ** (a + c) if b == j else y0[b]), (a, c, b)


# ------------------------------------------------------------------------------------------------ d. clamp edges
def test_dense_all_zero_image_and_all_zero_weight(ops):
    """an all-zero image among non-zero ones (maximum 0: the scale clamps at exponent 14): its outputs are bias + res
    exactly, its planes are zero, the neighbours keep their accuracy; an all-zero w: y == bias + res everywhere"""
    rng = np.random.default_rng(3)
    rows, B, K1, K2, N = 128, 3, 32, 32, 256
    M, K = rows * B, K1 + K2
    x = rng.standard_normal((B, rows, K)).astype(np.float32)
    x[1] = 0.0
    x = x.reshape(M, K)
    w = (rng.standard_normal((K, N)) / math.sqrt(K)).astype(np.float32)
    bias, res = rng.standard_normal(N).astype(np.float32), rng.standard_normal((M, N)).astype(np.float32)
    add = (dev(bias)[None, :] + dev(res)).cpu().numpy()          # one fp32 add, as the epilogue forms it
    ref, mag = fo.dense_ref(x[:, :K1], x[:, K1:], w, bias, res)
    for t11, t28 in TUNES:
        set_tune(ops, t11, t28)
        wp, wmax = pack(ops, dev(w), False)
        y1, _, xs = dense(ops, dev(x[:, :K1]), dev(x[:, K1:]), wp, wmax, N, 0, rows, bias=dev(bias), res=dev(res),
                          want_xs=True)
        y = y1.np_f32(M, N)
        assert np.all(np.isfinite(y))
        assert np.array_equal(y[rows:2 * rows], add[rows:2 * rows])
        err = float((np.abs(y - ref) / mag).max())
        assert err < 2e-6, err
        planes = xs.np_f16().view(np.uint16).reshape(B, -1)
        assert not np.any(planes[1]) and np.any(planes[0]) and np.any(planes[2])
        h, l = fo.unplane(xs.np_f16(), B, K, rows)
        vs = fo.scaled(x.reshape(B, rows, K))
        assert np.all(np.abs(h.astype(np.float64) + l.astype(np.float64) - vs) <= fo.split_bound(vs))
        wz, wzmax = pack(ops, torch.zeros(K, N, device="cuda"), False)
        assert not np.any(wz.np_f16().view(np.uint16))
        y1, _, _ = dense(ops, dev(x[:, :K1]), dev(x[:, K1:]), wz, wzmax, N, 0, rows, bias=dev(bias), res=dev(res))
        assert np.array_equal(y1.np_f32(M, N), add)
    print(f"zero image among others: worst error / mag = {err:.3e} (bar 2e-6)")


def test_dense_image_with_a_denormal_maximum(ops):
    """an image whose maximum is an fp32 denormal (biased exponent 0, clamped to 14: s = 2^126): every output finite and
    within 2e-6 mag + 2^-120 of the reference; the normal neighbours keep the 2e-6 bar"""
    rng = np.random.default_rng(4)
    rows, B, K, N = 128, 3, 96, 128
    M = rows * B
    x = rng.standard_normal((B, rows, K))
    x[1] *= 2.0 ** -140
    x = x.astype(np.float32)
    m = np.abs(x[1]).max()
    assert 0 < m < 2.0 ** -126
    x = x.reshape(M, K)
    w = (rng.standard_normal((K, N)) / math.sqrt(K)).astype(np.float32)
    for with_add in (False, True):
        bias = rng.standard_normal(N).astype(np.float32) if with_add else None
        res = rng.standard_normal((M, N)).astype(np.float32) if with_add else None
        ref, mag = fo.dense_ref(x, None, w, bias, res)
        wp, wmax = pack(ops, dev(w), False)
        y1, _, xs = dense(ops, dev(x), None, wp, wmax, N, 0, rows, bias=None if bias is None else dev(bias),
                          res=None if res is None else dev(res), want_xs=True)
        y = y1.np_f32(M, N).astype(np.float64)
        assert np.all(np.isfinite(y)) and np.all(np.isfinite(xs.np_f16().astype(np.float32)))
        excess = np.abs(y - ref) - (2e-6 * mag + 2.0 ** -120)
        print(f"denormal image (bias + res: {with_add}): max |y - ref| = {float(np.abs(y - ref)[rows:2 * rows].max()):.3e}, "
              f"max mag = {float(mag[rows:2 * rows].max()):.3e}")
        assert np.all(excess <= 0)
        others = np.r_[0:rows, 2 * rows:M]
        assert float((np.abs(y - ref) / mag)[others].max()) < 2e-6


# ------------------------------------------------------------------------------------------------ e. batched form
@pytest.mark.parametrize("transpose", [False, True])
@pytest.mark.parametrize("rows,B,K,N", [(128, 6, 32, 128), (128, 6, 1024, 128), (256, 3, 128, 256), (256, 3, 128, 1024),
                                        (1024, 2, 1024, 128), (1024, 2, 32, 256)])
def test_batched_exact_on_integers_with_and_without_res(ops, rows, B, K, N, transpose):
    """y[b] = x[b] @ W[b] (+ res): integers with independent powers of two per image on x and on w[b] (a wrong operand
    stride, image index or wmax row cannot pass), exact under the four instantiations, planes equal to the oracle's"""
    rng = np.random.default_rng(rows + B + K + N)
    M = rows * B
    px = np.array([0, 20, -30, 7, -12, 33])[:B]
    pw = np.array([5, -25, 0, 18, -7, -40])[:B]
    x = rng.integers(-3, 4, (B, rows, K)) * 2.0 ** px[:, None, None]
    w = rng.integers(-2, 3, (B, K, N)) * 2.0 ** pw[:, None, None]
    res = rng.integers(-3, 4, (B, rows, N)) * 2.0 ** (px + pw)[:, None, None]
    ref0, _ = fo.dense_ref(x, None, w)
    ref1 = ref0 + res
    for r in (ref0, ref1):
        assert np.array_equal(r.astype(np.float32).astype(np.float64), r)
    stored = np.ascontiguousarray(w.transpose(0, 2, 1)) if transpose else w
    wp, wmax = pack_batched(ops, dev(stored), transpose)
    for b in range(B):                                             # the packs are the oracle's bits, image by image
        want, _ = fo.pack_linear(stored[b], transpose)
        assert np.array_equal(wp.np_f16().view(np.uint16).reshape(B, -1)[b], want.view(np.uint16)), b
    xd, resd = dev(x.reshape(M, K)), dev(res.reshape(M, N))
    planes = fo.planes_of(x.reshape(M, K), None, rows)
    for t11, t28 in TUNES:
        set_tune(ops, t11, t28)
        for r, ref in ((None, ref0), (resd, ref1)):
            y1, _, xs = dense(ops, xd, None, wp, wmax, N, 0, rows, res=r, want_xs=r is None, batched=True)
            bad = np.argwhere(y1.np_f32(B, rows, N) != ref.astype(np.float32))
            assert bad.size == 0, (t11, t28, r is not None, len(bad), bad[:4].tolist())
            if xs is not None:
                assert np.array_equal(xs.np_f16().view(np.uint16), planes.view(np.uint16))
    if rows == 1024:                                               # the wrapper hands `res` through
        y = ops.linear_batched_raw(xd.view(B, rows, K), maxima(ops, xd, B), wp.body, wmax, N, res=resd.view(B, rows, N))
        assert np.array_equal(y.cpu().numpy(), ref1.astype(np.float32))


# ------------------------------------------------------------------------------------------------ f. pack kernels
PACKS = [(16, 40), (32, 128), (128, 128), (1024, 1024)]            # the last: more elements than 1024 (256) blocks cover at once


@pytest.mark.parametrize("transpose", [False, True])
@pytest.mark.parametrize("K,N", PACKS)
def test_pack_against_the_host_split(ops, K, N, transpose):
    """mulan_linear_pack_f16x3 against pack_linear: bit for bit on integer weights, within the reconstruction bound on
    Gaussian weights"""
    rng = np.random.default_rng(K + N)
    shape = (N, K) if transpose else (K, N)
    wi = (rng.integers(-4, 5, shape) * 2.0 ** -7).astype(np.float32)
    wp, wmax = pack(ops, dev(wi), transpose)
    want, maxbits = fo.pack_linear(wi, transpose)
    assert int(wmax.max()) == maxbits
    assert np.array_equal(wp.np_f16().view(np.uint16), want.view(np.uint16))
    wg = (rng.standard_normal(shape) * 0.05).astype(np.float32)
    wp, wmax = pack(ops, dev(wg), transpose)
    _, maxbits = fo.pack_linear(wg, transpose)
    assert int(wmax.max()) == maxbits
    h, l = fo.unpack_linear(wp.np_f16(), K, N)
    vs = (wg.T if transpose else wg) * fo.scale_of(maxbits)[0]
    rec = np.abs(h.astype(np.float64) + l.astype(np.float64) - vs) / fo.split_bound(vs)
    print(f"pack: worst reconstruction error / bound = {float(rec.max()):.3f}")
    assert float(rec.max()) <= 1.0


@pytest.mark.parametrize("transpose", [False, True])
@pytest.mark.parametrize("K,N", PACKS)
def test_batched_pack_against_the_host_split(ops, K, N, transpose):
    """mulan_linear_pack_f16x3_batched, 3 images of different magnitudes, checked per image with its own maximum"""
    rng = np.random.default_rng(K + N + 1)
    shape = (3, N, K) if transpose else (3, K, N)
    mags = np.array([1.0, 2.0 ** -31, 2.0 ** 22])[:, None, None]
    wi = (rng.integers(-4, 5, shape) * mags).astype(np.float32)
    wp, wmax = pack_batched(ops, dev(wi), transpose)
    got = wp.np_f16().view(np.uint16).reshape(3, -1)
    for b in range(3):
        want, maxbits = fo.pack_linear(wi[b], transpose)
        assert int(wmax[b].max()) == maxbits
        assert np.array_equal(got[b], want.view(np.uint16)), b
    wg = (rng.standard_normal(shape) * np.array([1.0, 1e-9, 4e5])[:, None, None]).astype(np.float32)
    wp, wmax = pack_batched(ops, dev(wg), transpose)
    got = wp.np_f16().reshape(3, -1)
    worst = 0.0
    for b in range(3):
        _, maxbits = fo.pack_linear(wg[b], transpose)
        assert int(wmax[b].max()) == maxbits
        h, l = fo.unpack_linear(got[b], K, N)
        vs = (wg[b].T if transpose else wg[b]) * fo.scale_of(maxbits)[0]
        worst = max(worst, float((np.abs(h.astype(np.float64) + l.astype(np.float64) - vs) / fo.split_bound(vs)).max()))
    print(f"batched pack: worst reconstruction error / bound = {worst:.3f}")
    assert worst <= 1.0


# ------------------------------------------------------------------------------------------------ g. weight gradients
def planes_by_product(ops, t, rows=1024):
    """t [B, rows, C] -> (planes of t as a uint8 tensor, maxima): the by-product of the batched product with the first
    128 columns of an identity"""
    B, _, C = t.shape
    eye = torch.eye(C, 128, device="cuda").expand(B, C, 128).contiguous()
    wp, wmax = pack_batched(ops, eye, False)
    _, _, xs = dense(ops, t.reshape(B * rows, C), None, wp, wmax, 128, 0, rows, want_xs=True, batched=True)
    return xs.body, maxima(ops, t, B)


def wgrad(ops, form, B, C1, C2, N, acc, share, dw0, x1=None, x2=None, m1=None, m2=None, xs=None, dys=None, dymax=None):
    """one weight-gradient launch into a workspace of exactly the size the _workspace function names, guards behind
    the workspace and dw"""
    L = ops.lib.load()
    C = C1 + C2
    nbytes = getattr(L, f"mulan_linear_wgrad_f16x3_{form}_workspace")(B, 32, 32, C, N, share)
    assert nbytes > 0 and nbytes % (C * N * 4) == 0
    ws, dw = Buf(nbytes), Buf(C * N * 4)
    if dw0 is not None:
        dw.f32(C, N).copy_(dw0)
    if form == "planes":
        xmax = m1 if m2 is None else torch.maximum(m1, m2)
        ops.call("mulan_linear_wgrad_f16x3_planes", ops.ptr(xs), ops.ptr(xmax), ops.ptr(dys), ops.ptr(dymax), dw.ptr, ws.ptr,
                 B, 32, 32, C, N, acc, share, ops.stream())
    else:
        ops.call("mulan_linear_wgrad_f16x3_x32", ops.ptr(x1), ops.ptr(x2), C1, C2, ops.ptr(m1), ops.ptr(m2), ops.ptr(dys),
                 ops.ptr(dymax), dw.ptr, ws.ptr, B, 32, 32, N, acc, share, ops.stream())
    torch.cuda.synchronize()
    assert ws.guard_ok() and dw.guard_ok()
    return dw.f32(C, N).clone(), nbytes // (C * N * 4)


@pytest.mark.parametrize("B,C1,C2,N", [(1, 128, 0, 128), (2, 128, 256, 128), (7, 256, 128, 128), (7, 256, 256, 256),
                                       (2, 256, 256, 384), (7, 128, 0, 384), (1, 128, 256, 256)])
def test_dense_weight_gradients_accumulate_share_and_uneven_slabs(ops, B, C1, C2, N):
    """dw (+)= [x1 | x2]^T dy from planes and from fp32 x, share_chip and accumulate in {0, 1}: the two forms give the same
    bits; on integers (images at different powers of two) dw is exact, dw0 + sum included; on Gaussian data within 3e-6
    of |x|^T |dy| (+ |dw0|), the bar of test_f16x3_dense_weight_gradient_from_planes.  B = 7 gives 112 row pairs that the
    slab counts of 3 and more tiles do not divide."""
    rng = np.random.default_rng(B + C1 + C2 + N)
    C = C1 + C2
    slabs = set()
    for ints in (True, False):
        if ints:
            x = rng.integers(-3, 4, (B, 1024, C)) * 2.0 ** (np.arange(B) % 4)[:, None, None]
            dy = rng.integers(-2, 3, (B, 1024, N)) * 2.0 ** ((np.arange(B) + 1) % 3)[:, None, None]
            dw0 = rng.integers(-3, 4, (C, N)).astype(np.float64)
        else:
            x = rng.standard_normal((B, 1024, C)) * np.resize(np.array([1.0, 1e-3, 50.0]), B)[:, None, None]
            dy = rng.standard_normal((B, 1024, N)) * np.resize(np.array([2.0, 30.0, 1e-2, 1.0]), B)[:, None, None]
            dw0 = rng.standard_normal((C, N)) * 100
        x, dy, dw0 = fo.f32(x), fo.f32(dy), fo.f32(dw0)
        xf, dyf = x.reshape(-1, C), dy.reshape(-1, N)
        ref = xf.T @ dyf
        mag = np.abs(xf).T @ np.abs(dyf)
        x1d, x2d, dyd, dw0d = dev(x[..., :C1]), (dev(x[..., C1:]) if C2 else None), dev(dy), dev(dw0)
        m1, m2 = maxima(ops, x1d, B), (maxima(ops, x2d, B) if C2 else None)
        dys, dymax = planes_by_product(ops, dyd)
        # the planes of [x1 | x2]: the by-product of the layer's forward call (any weight)
        wp, wmax = pack(ops, torch.ones(C, 128, device="cuda"), False)
        _, _, xsb = dense(ops, x1d.view(-1, C1), x2d.view(-1, C2) if C2 else None, wp, wmax, 128, 0, 1024, want_xs=True)
        if ints:
            assert np.array_equal(xsb.np_f16().view(np.uint16),
                                  fo.planes_of(xf[:, :C1], xf[:, C1:] if C2 else None, 1024).view(np.uint16))
            assert np.array_equal(dys.cpu().numpy().view(np.uint16), fo.planes_of(dyf, None, 1024).view(np.uint16))
        worst = 0.0
        for share in (0, 1):
            for acc in (0, 1):
                dwp, S = wgrad(ops, "planes", B, C1, C2, N, acc, share, dw0d if acc else None, m1=m1, m2=m2, xs=xsb.body,
                               dys=dys, dymax=dymax)
                dwx, _ = wgrad(ops, "x32", B, C1, C2, N, acc, share, dw0d if acc else None, x1=x1d, x2=x2d, m1=m1, m2=m2,
                               dys=dys, dymax=dymax)
                slabs.add(S)
                assert torch.equal(dwp, dwx), (share, acc)
                got = dwp.cpu().double().numpy()
                assert np.all(np.isfinite(got))
                want = ref + (dw0 if acc else 0)
                if ints:
                    assert np.array_equal(got, want), (share, acc)
                else:
                    worst = max(worst, float((np.abs(got - want) / (mag + (np.abs(dw0) if acc else 0))).max()))
        if not ints:
            print(f"dense dw: worst error / mag = {worst:.3e} (bar 3e-6), slab counts {sorted(slabs)}")
            assert worst < 3e-6
    if B == 7 and (C // 128) * (N // 128) >= 3:
        assert any((B * 16) % s for s in slabs)


@pytest.mark.parametrize("B,C,N", [(1, 128, 128), (5, 256, 256), (5, 1024, 128), (1, 1024, 256), (5, 128, 256)])
def test_bmm_tn_planes_exact_on_integers_image_by_image(ops, B, C, N):
    """out[b] = x[b]^T @ g[b] from the planes of both operands, per-image powers of two on both sides"""
    rng = np.random.default_rng(B + C + N)
    px = np.array([0, 20, -30, 7, -12])[:B]
    pg = np.array([-9, 3, 25, -18, 0])[:B]
    x = rng.integers(-3, 4, (B, 1024, C)) * 2.0 ** px[:, None, None]
    g = rng.integers(-2, 3, (B, 1024, N)) * 2.0 ** pg[:, None, None]
    xs, xm = planes_by_product(ops, dev(x))
    gs, gm = planes_by_product(ops, dev(g))
    out = Buf(B * C * N * 4)
    ops.call("mulan_bmm_tn_f16x3_planes", ops.ptr(xs), ops.ptr(xm), ops.ptr(gs), ops.ptr(gm), out.ptr, B, 32, 32, C, N,
             ops.stream())
    torch.cuda.synchronize()
    assert out.guard_ok()
    got = out.np_f32(B, C, N).astype(np.float64)
    for b in range(B):
        assert np.array_equal(got[b], x[b].T @ g[b]), b


# ------------------------------------------------------------------------------------------------ h. rejected arguments
REJECTS = {
    "M % 128": dict(M=320),
    "rows_per_img % 128": dict(rows=64),
    "M % rows_per_img": dict(M=384, rows=256),
    "K1 % 32": dict(K1=48),
    "K2 % 32": dict(K2=16),
    "N1 % 128": dict(N1=64),
    "N2 % 128": dict(N2=192),
    "res with N2 > 0": dict(res=True),
    "K2 > 0 with a null x2": dict(x2=None),
    "K2 > 0 with a null x2max": dict(x2max=None),
    "a null wmax": dict(wmax=None),
}


@pytest.mark.parametrize("what", list(REJECTS))
def test_dense_rejects_documented_violations_and_writes_nothing(ops, what):
    """each violation of the header's contract returns non-zero from the argument check, before any launch: the
    sentinel-filled outputs are untouched.  (All pointers are valid and all buffers large enough for any of the sizes.)"""
    L = ops.lib.load()
    a = dict(M=256, rows=128, K1=32, K2=32, N1=128, N2=128, res=False)
    big = 512 * 512
    t = dict(x1=torch.ones(big, device="cuda"), x2=torch.ones(big, device="cuda"), res=torch.ones(big, device="cuda"),
             bias=torch.ones(1024, device="cuda"), x1max=torch.zeros(64, 16, dtype=torch.int32, device="cuda"),
             x2max=torch.zeros(64, 16, dtype=torch.int32, device="cuda"),
             wmax=torch.zeros(64, 16, dtype=torch.int32, device="cuda"), wp=torch.zeros(4 * big, dtype=torch.uint8, device="cuda"))
    y1, y2, xs = Buf(4 * big), Buf(4 * big), Buf(4 * big)

    def launch(a, t):
        return L.mulan_linear_f16x3(ops.ptr(t["x1"]), ops.ptr(t["x1max"]), ops.ptr(t["x2"]), ops.ptr(t["x2max"]), a["K1"], a["K2"],
                                    ops.ptr(t["wp"]), ops.ptr(t["wmax"]), ops.ptr(t["bias"]), ops.ptr(t["res"]) if a["res"] else None,
                                    y1.ptr, y2.ptr, xs.ptr, a["N1"], a["N2"], a["M"], a["rows"], ops.stream())

    for k, v in REJECTS[what].items():
        (a if k in a else t)[k] = v
    assert launch(a, t) != 0
    torch.cuda.synchronize()
    assert y1.untouched() and y2.untouched() and xs.untouched()


def test_batched_and_pack_reject_documented_violations_and_write_nothing(ops):
    L = ops.lib.load()
    w = torch.ones(128 * 128, device="cuda")
    wmax = torch.zeros(4, 16, dtype=torch.int32, device="cuda")
    x, xmax = torch.ones(256 * 128, device="cuda"), torch.zeros(4, 16, dtype=torch.int32, device="cuda")
    wp, y, xs = Buf(4 * 128 * 128 * 4), Buf(256 * 128 * 4), Buf(256 * 128 * 4)
    s = ops.stream()
    assert L.mulan_linear_pack_f16x3(ops.ptr(w), wp.ptr, ops.ptr(wmax), 24, 128, 0, s) != 0            # K % 16
    assert L.mulan_linear_pack_f16x3(ops.ptr(w), wp.ptr, None, 32, 128, 0, s) != 0                       # a null wmax
    assert L.mulan_linear_pack_f16x3_batched(ops.ptr(w), wp.ptr, ops.ptr(wmax), 24, 128, 0, 2, s) != 0  # K % 16
    assert L.mulan_linear_pack_f16x3_batched(ops.ptr(w), wp.ptr, ops.ptr(wmax), 32, 128, 0, 0, s) != 0  # batch = 0
    zeros = torch.zeros(4 * 128 * 128 * 4, dtype=torch.uint8, device="cuda")
    for M, rows, K, N, wm in ((320, 128, 32, 128, wmax), (256, 64, 32, 128, wmax), (256, 128, 48, 128, wmax),
                              (256, 128, 32, 64, wmax), (256, 128, 32, 128, None)):
        assert L.mulan_linear_f16x3_batched(ops.ptr(x), ops.ptr(xmax), K, ops.ptr(zeros), ops.ptr(wm), None, y.ptr, xs.ptr,
                                            N, M, rows, s) != 0, (M, rows, K, N)
    torch.cuda.synchronize()
    assert wp.untouched() and y.untouched() and xs.untouched()
