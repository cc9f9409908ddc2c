"""The f16x3 3x3 convolution family off the model's height and scales: the weight pack (f16x3_prep.hip), the forward /
input-gradient kernels (conv3x3_f16x3.hip, conv3x3_f16x3_v3.hip) and the nine-tap and plane-fed weight gradients
(wgrad_f16x3.hip), through the C entry points on buffers allocated here.  Every output (y, xs, ymax, dw, the workspace --
sized by the _workspace function) is a Buf of tests/test_gpu_linear_f16x3.py: its guard band must survive the launch.

The reference is the host model tests/f16x3_oracle.py: the bits of the documented layouts for packs and planes, float64
on the fp32-rounded inputs for results.  Integer data is exact.  Non-integer data comes from tests/f16x3_conv_cases.py and
is held per element to 3e-6 of the magnitude sum (+ the floor of the split for images under the scale clamp);
tests/test_f16x3_conv_oracle.py shows that the kernels' arithmetic with an exact accumulator lies within half of those
bars on the very same inputs.

The input gradient is the forward entry point on the flip = 1 pack with C and N swapped, so it needs C % 128 == 0: the
(48, 128) shape has no f16x3 input gradient."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import f16x3_conv_cases as cases
from tests import f16x3_oracle as fo
from tests.test_gpu_linear_f16x3 import Buf, bufptr, dev, maxima

TUNE_KEYS = (1, 3, 13, 23, 27)


@pytest.fixture()
def ops(monkeypatch):
    from mulan_amd import ops as _ops
    _ops.lib.load()
    monkeypatch.setattr(_ops, "CONV_MODE", "f16x3")
    yield _ops
    for k in TUNE_KEYS:
        _ops.call("mulan_set_tuning", k, 0)


def tune(ops, key, value):
    ops.call("mulan_set_tuning", key, value)


def pack(ops, w, flip):
    """w [3, 3, C, N] on the device -> (Buf of the packed operand, wmax [1][16])"""
    C, N = w.shape[2:]
    wmax = maxima(ops, w, 1)
    wp = Buf(ops.lib.load().mulan_conv3x3_pack_f16x3_bytes(C, N))
    ops.call("mulan_conv3x3_pack_f16x3", ops.ptr(w), wp.ptr, ops.ptr(wmax), C, N, flip, ops.stream())
    torch.cuda.synchronize()
    assert wp.guard_ok()
    return wp, wmax


def fwd(ops, x, wp, wmax, N, bias=None, cbias=None, res=None, want_xs=False, want_ymax=False, xplanes=None, xmax=None):
    """one forward launch, x [B, H, 32, C] on the device (or its planes, with the maxima they were scaled with) ->
    (y, xs, ymax) as Bufs and xmax.  cbias [B, N] is per sample, [B, H, 32, N] per pixel."""
    B, H, W, C = x.shape
    xmax = maxima(ops, x, B) if xmax is None else xmax
    y = Buf(B * H * W * N * 4)
    xs = Buf(ops.lib.load().mulan_conv3x3_planes_bytes(B, H, W, C)) if want_xs else None
    ymax = Buf(B * 16 * 4) if want_ymax else None
    mode = 0 if cbias is None else (1 if cbias.dim() == 2 else 2)
    if xplanes is None:
        ops.call("mulan_conv3x3_fwd_f16x3", ops.ptr(x), ops.ptr(xmax), wp.ptr, ops.ptr(wmax), ops.ptr(bias), ops.ptr(cbias), mode,
                 ops.ptr(res), y.ptr, bufptr(xs), bufptr(ymax), B, H, W, C, N, ops.stream())
    else:
        ops.call("mulan_conv3x3_fwd_f16x3_planes_in", xplanes.ptr, ops.ptr(xmax), wp.ptr, ops.ptr(wmax), ops.ptr(bias),
                 ops.ptr(cbias), mode, ops.ptr(res), y.ptr, bufptr(ymax), B, H, W, C, N, ops.stream())
    torch.cuda.synchronize()
    for b in (y, xs, ymax):
        assert b is None or b.guard_ok()
    return y, xs, ymax, xmax


def same_planes(buf, x):
    """the planes in `buf` are fo.conv_planes(x) bit for bit -- up to the sign of a zero piece, which carries no value: for
    x = -0.0 the device leaves l = -0 where the host's IEEE subtraction (-0) - (-0) gives +0 (seen on the all-zero image of
    the clamp set, whose elements are signed zeros)"""
    canon = lambda u: np.where(u == 0x8000, 0, u)
    return np.array_equal(canon(buf.np_f16().view(np.uint16)), canon(fo.conv_planes(x).view(np.uint16)))


def check_ymax(ymax, y, B, nparts):
    """the 16 slots reduce to max |y| of the launch's own output; the slots past the launch's parts are zero"""
    slots = ymax.body.cpu().numpy().view(np.uint32).reshape(B, 16)
    want = np.abs(y.reshape(B, -1)).max(axis=1).astype(np.float32).view(np.uint32)
    assert np.array_equal(slots.max(axis=1), want)
    assert not np.any(slots[:, nparts:])


def wgrad9(ops, x, dy, acc=0, dw0=None, xmax=None, dymax=None):
    """the nine-tap weight gradient from fp32 x [B, H, 32, C] and dy [B, H, 32, N] -> (dw [3, 3, C, N], slab count)"""
    B, H, W, C = x.shape
    N = dy.shape[-1]
    nbytes = ops.lib.load().mulan_conv3x3_wgrad_f16x3_workspace(B, H, W, C, N)
    assert nbytes > 0 and nbytes % (9 * C * N * 4) == 0
    ws, dw = Buf(nbytes), Buf(9 * C * N * 4)
    if dw0 is not None:
        dw.f32(3, 3, C, N).copy_(dw0)
    xmax = maxima(ops, x, B) if xmax is None else xmax
    dymax = maxima(ops, dy, B) if dymax is None else dymax
    ops.call("mulan_conv3x3_wgrad_f16x3", ops.ptr(x), ops.ptr(xmax), ops.ptr(dy), ops.ptr(dymax), dw.ptr, ws.ptr, B, H, W, C, N,
             acc, ops.stream())
    torch.cuda.synchronize()
    assert ws.guard_ok() and dw.guard_ok()
    return dw.np_f32(3, 3, C, N).astype(np.float64), nbytes // (9 * C * N * 4)


def wgrad_planes(ops, xs, xmax, dys, dymax, B, H, C, N, acc=0, share=0, dw0=None):
    """the plane-fed weight gradient -> (dw [3, 3, C, N], slab count)"""
    nbytes = ops.lib.load().mulan_conv3x3_wgrad_f16x3_planes_workspace(B, H, 32, C, N, share)
    assert nbytes > 0 and nbytes % (9 * C * N * 4) == 0
    ws, dw = Buf(nbytes), Buf(9 * C * N * 4)
    if dw0 is not None:
        dw.f32(3, 3, C, N).copy_(dw0)
    ops.call("mulan_conv3x3_wgrad_f16x3_planes", xs.ptr, ops.ptr(xmax), dys.ptr, ops.ptr(dymax), dw.ptr, ws.ptr, B, H, 32, C, N,
             acc, share, ops.stream())
    torch.cuda.synchronize()
    assert ws.guard_ok() and dw.guard_ok()
    return dw.np_f32(3, 3, C, N).astype(np.float64), nbytes // (9 * C * N * 4)


def planes_by_product(ops, t):
    """t [B, H, 32, C] on the device -> (planes Buf, maxima): the by-product of a forward launch (all-zero weights)"""
    wp, wmax = pack(ops, torch.zeros(3, 3, t.shape[-1], 128, device="cuda"), 0)
    _, xs, _, tmax = fwd(ops, t, wp, wmax, 128, want_xs=True)
    return xs, tmax


# ------------------------------------------------------------------------------------------------ a. pack and planes as bits
@pytest.mark.parametrize("flip", [0, 1])
@pytest.mark.parametrize("C,N", [(16, 128), (48, 128), (128, 128), (128, 256), (256, 128)])
def test_pack_is_the_documented_layout_bit_for_bit(ops, C, N, flip):
    """wp[t][cc][o][plane][k] = split2(s_w Wl[t][cc 16 + k][o]); flip = 1: Wl[t][k][o] = w[8 - t][o][k] -- needs N % 16 == 0
    only, the entry point checks the input channels of Wl"""
    rng = np.random.default_rng(C + N + flip)
    w = (rng.standard_normal((3, 3, C, N)) * 0.05).astype(np.float32)
    wp, wmax = pack(ops, dev(w), flip)
    want, maxbits = fo.pack_conv(w, flip)
    assert int(wmax.max()) == maxbits
    assert np.array_equal(wp.np_f16().view(np.uint16), want.view(np.uint16))


@pytest.mark.parametrize("B,H,C,N,t3", [(2, 8, 32, 128, 0), (1, 24, 128, 128, 0), (2, 32, 48, 256, 0), (1, 16, 256, 128, 0),
                                        (2, 24, 128, 256, 2), (1, 40, 128, 256, 0)])
def test_planes_and_output_maxima_of_a_forward_launch(ops, B, H, C, N, t3):
    """xs is [B][C/16][H W][plane][16] of split2(x s_x[b]), bit for bit, from the fp32-input instantiation of both kernels
    (C % 32 != 0, or tune[3] = 2: the 32x32x16 kernel); ymax reduces to max |y| of the launch's own output, its unused
    slots are zero"""
    rng = np.random.default_rng(B + H + C + N)
    x = rng.standard_normal((B, H, 32, C)) * np.resize(np.array([1.0, 1e-5]), B)[:, None, None, None]
    x = x.astype(np.float32)
    w = (rng.standard_normal((3, 3, C, N)) * 0.05).astype(np.float32)
    tune(ops, 3, t3)
    wp, wmax = pack(ops, dev(w), 0)
    y, xs, ymax, _ = fwd(ops, dev(x), wp, wmax, N, want_xs=True, want_ymax=True)
    assert same_planes(xs, x)
    rows = 8 if (t3 or C % 32) else ops.lib.load().mulan_conv3x3_f16x3_tile_rows(B, H, N, 1)
    got = y.np_f32(B, H, 32, N)
    check_ymax(ymax, got, B, (H // rows) * (N // 128))


# ------------------------------------------------------------------------------------------------ b. heights, exact on integers
def int_case(B, H, C, N, seed):
    """integers with a power of two of its own per image: every product and partial sum is an integer times a power of
    two below 2^24, the float64 reference is an fp32 number"""
    rng = np.random.default_rng(seed)
    px = 2.0 ** np.resize(np.array([0, 9, -6]), B)[:, None, None, None]
    x = rng.integers(-3, 4, (B, H, 32, C)) * px
    w = rng.integers(-2, 3, (3, 3, C, N)).astype(np.float64)
    # (x dy carries 2^3, 2^4, 2^2 in images 0, 1, 2: the weight gradient's sum over images stays within 24 bits)
    dy = rng.integers(-2, 3, (B, H, 32, N)) * 2.0 ** np.resize(np.array([3, -5, 8]), B)[:, None, None, None]
    bias = rng.integers(-3, 4, N).astype(np.float64)
    cb = rng.integers(-3, 4, (B, N)).astype(np.float64)
    res = rng.integers(-3, 4, (B, H, 32, N)) * px
    cb2 = rng.integers(-3, 4, (B, H, 32, N)) * px
    return x, w, dy, bias, cb, res, cb2


def exact(got, ref):
    bad = np.argwhere(got != ref)
    assert bad.size == 0, (len(bad), bad[:4].tolist())


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("C,N", [(128, 128), (48, 128), (128, 256)])
@pytest.mark.parametrize("H", [8, 16, 24, 40, 64])
def test_every_entry_point_is_exact_on_integers_at_heights_other_than_32(ops, H, C, N, B):
    """forward with bias + per-sample cbias + res and with a per-pixel cbias alone, input gradient, nine-tap weight
    gradient and (C, N multiples of 128) the plane-fed weight gradient on the planes the two convolutions wrote.  At
    H = 8 a block is the first and the last tile of its image; 24 and 40 give tile counts that are no power of two."""
    x, w, dy, bias, cb, res, cb2 = int_case(B, H, C, N, H + C + N + B)
    xd, wd, dyd = dev(x), dev(w), dev(dy)
    wp, wmax = pack(ops, wd, 0)
    big = C % 128 == 0
    # (a per-image power of two on bias + cbias would not be one fp32 number beside the products: the sums stay below 2^24)
    ref = fo.conv64(x, w) + bias + cb[:, None, None, :] + res
    assert np.array_equal(ref.astype(np.float32).astype(np.float64), ref)
    y, xs, ymax, xmax = fwd(ops, xd, wp, wmax, N, bias=dev(bias), cbias=dev(cb), res=dev(res), want_xs=big, want_ymax=True)
    exact(y.np_f32(B, H, 32, N), ref)
    rows = ops.lib.load().mulan_conv3x3_f16x3_tile_rows(B, H, N, 1) if C % 32 == 0 else 8
    check_ymax(ymax, ref, B, (H // rows) * (N // 128))
    y2, _, _, _ = fwd(ops, xd, wp, wmax, N, cbias=dev(cb2))
    exact(y2.np_f32(B, H, 32, N), fo.conv64(x, w) + cb2)
    dwr = fo.wgrad64(x, dy)
    dw, _ = wgrad9(ops, xd, dyd)
    exact(dw, dwr)
    if big:
        assert same_planes(xs, x)
        wpf, _ = pack(ops, wd, 1)
        dx, dys, _, dymax = fwd(ops, dyd, wpf, wmax, C, want_xs=True)
        exact(dx.np_f32(B, H, 32, C), fo.conv64(dy, fo.flip_conv(w)))
        assert same_planes(dys, dy)
        dwp, _ = wgrad_planes(ops, xs, xmax, dys, dymax, B, H, C, N)
        exact(dwp, dwr)


@pytest.mark.parametrize("H,key,value", [(8, 23, 8), (8, 23, 4), (8, 23, 2), (24, 23, 8), (24, 23, 4), (24, 23, 2), (8, 27, 2),
                                         (8, 0, 0), (24, 0, 0)])
def test_tile_heights_k_split_and_plane_fed_forward_are_exact_on_integers(ops, H, key, value):
    """tune[23]: forced tile height; tune[27] = 2 (H = 8): the k-split blocks; and the plane-fed forward on the xs of the
    fp32-input launch -- every one against the same reference, with and without the maxima by-product"""
    B, C, N = 3, 128, 256
    x, w, dy, bias, cb, res, cb2 = int_case(B, H, C, N, H)
    ref = fo.conv64(x, w) + bias + cb[:, None, None, :] + res
    xd = dev(x)
    wp, wmax = pack(ops, dev(w), 0)
    if key:
        tune(ops, key, value)
    for want_ymax in (False, True):
        y, xs, ymax, xmax = fwd(ops, xd, wp, wmax, N, bias=dev(bias), cbias=dev(cb), res=dev(res), want_xs=True, want_ymax=want_ymax)
        exact(y.np_f32(B, H, 32, N), ref)
        assert same_planes(xs, x)
        yp, _, ypmax, _ = fwd(ops, xd, wp, wmax, N, bias=dev(bias), cbias=dev(cb), res=dev(res), want_ymax=want_ymax, xplanes=xs, xmax=xmax)
        exact(yp.np_f32(B, H, 32, N), ref)
        if want_ymax:
            rows = ops.lib.load().mulan_conv3x3_f16x3_tile_rows(B, H, N, 1)
            # (with the maxima a forced height holds only while its H / rows x N / 128 parts fit the 16 slots)
            assert key != 23 or rows == value or (H // value) * (N // 128) > 16
            check_ymax(ymax, ref, B, (H // rows) * (N // 128))
            check_ymax(ypmax, ref, B, (H // rows) * (N // 128))


@pytest.mark.parametrize("H", [8, 24])
def test_dense_plane_fed_weight_gradient_reads_planes_of_any_height(ops, H):
    """mulan_linear_wgrad_f16x3_planes and mulan_bmm_tn_f16x3_planes accept any even H and read the same plane layout
    [B][C/16][H W][plane][16]: exact on integers on the planes a convolution wrote"""
    B, C, N = 3, 128, 256
    x, _, dy, *_ = int_case(B, H, C, N, H + 1)
    xs, xmax = planes_by_product(ops, dev(x))
    dys, dymax = planes_by_product(ops, dev(dy))
    L = ops.lib.load()
    nbytes = L.mulan_linear_wgrad_f16x3_planes_workspace(B, H, 32, C, N, 0)
    assert nbytes > 0 and nbytes % (C * N * 4) == 0
    ws, dw, out = Buf(nbytes), Buf(C * N * 4), Buf(B * C * N * 4)
    ops.call("mulan_linear_wgrad_f16x3_planes", xs.ptr, ops.ptr(xmax), dys.ptr, ops.ptr(dymax), dw.ptr, ws.ptr, B, H, 32, C, N, 0, 0,
             ops.stream())
    ops.call("mulan_bmm_tn_f16x3_planes", xs.ptr, ops.ptr(xmax), dys.ptr, ops.ptr(dymax), out.ptr, B, H, 32, C, N, ops.stream())
    torch.cuda.synchronize()
    assert ws.guard_ok() and dw.guard_ok() and out.guard_ok()
    per_image = np.einsum("bpc,bpn->bcn", x.reshape(B, -1, C), dy.reshape(B, -1, N))
    exact(out.np_f32(B, C, N).astype(np.float64), per_image)
    exact(dw.np_f32(C, N).astype(np.float64), per_image.sum(axis=0))


# ------------------------------------------------------------------------------------------------ c. accumulate, share_chip, splits
def wgrad_operands(ops, B, C, N, ints, seed):
    rng = np.random.default_rng(seed)
    if ints:
        x = rng.integers(-3, 4, (B, 32, 32, C)) * 2.0 ** (np.arange(B) % 4)[:, None, None, None]
        dy = rng.integers(-2, 3, (B, 32, 32, N)) * 2.0 ** ((np.arange(B) + 1) % 3)[:, None, None, None]
        dw0 = rng.integers(-3, 4, (3, 3, C, N)).astype(np.float64)
    else:
        x = rng.standard_normal((B, 32, 32, C)) * np.resize(np.array([1.0, 1e-3, 50.0]), B)[:, None, None, None]
        dy = rng.standard_normal((B, 32, 32, N)) * np.resize(np.array([2.0, 30.0, 1e-2, 1.0]), B)[:, None, None, None]
        dw0 = rng.standard_normal((3, 3, C, N)) * 100
    x, dy, dw0 = fo.f32(x), fo.f32(dy), fo.f32(dw0)
    xd, dyd = dev(x), dev(dy)
    xs, xmax = planes_by_product(ops, xd)
    dys, dymax = planes_by_product(ops, dyd)
    return x, dy, dw0, xd, dyd, xs, xmax, dys, dymax


# (B, C, N) -> slab counts wgrad_splits_w8 gives with share_chip = 0 / 1: target 256 (120 shared, up to two tiles) over
# 3 kernel rows x tiles, at most the B * 16 row pairs
SPLITS = {(3, 128, 128): (48, 40), (5, 256, 128): (42, 20), (7, 256, 256): (21, 21)}


@pytest.mark.parametrize("B,C,N", list(SPLITS))
def test_weight_gradients_accumulate_and_share_the_chip(ops, B, C, N):
    """accumulate = 1 on an integer-valued dw0 gives dw0 + ref exactly, accumulate = 0 on a NaN-filled dw gives ref exactly,
    for the nine-tap kernel and for the plane-fed one under share_chip 0 / 1; the workspace function names the slab count
    this table predicts"""
    x, dy, dw0, xd, dyd, xs, xmax, dys, dymax = wgrad_operands(ops, B, C, N, True, B + C + N)
    ref = fo.wgrad64(x, dy)
    nan = torch.full((3, 3, C, N), float("nan"), device="cuda")
    for acc in (0, 1):
        want = ref + dw0 if acc else ref
        dw, _ = wgrad9(ops, xd, dyd, acc, dev(dw0) if acc else nan, xmax, dymax)
        exact(dw, want)
        for share in (0, 1):
            dw, S = wgrad_planes(ops, xs, xmax, dys, dymax, B, 32, C, N, acc, share, dev(dw0) if acc else nan)
            assert S == SPLITS[(B, C, N)][share]
            exact(dw, want)


def test_forced_split_counts(ops):
    """tune[1] = v: the one-tile plane-fed kernel runs S = min(max(v / 3, 1), pairs) slabs, the nine-tap kernel
    S = v / tiles of 64 x 64.  Plane-fed S = 1, S = pairs = 48 and S = 7 (48 pairs in ranges of 6 and 7 that cross the
    images' borders), nine-tap S = 1: exact on integers.

    On Gaussian data two split counts differ in the order of the fp32 sums alone (the products are the same).  A slab
    over p row pairs is a chain of 6 p accumulator updates (2 k steps x 3 terms per pair, each adding a 32-pixel sum) and
    the reduction adds S slabs in a row, so an element goes through n(S) = 6 ceil(pairs / S) + S roundings of at most
    2^-24 of a partial sum, which |x|^T |dy| bounds: two runs agree to (n(S_a) + n(S_b)) 2^-24 |x|^T |dy|.  (For S = 1
    against 48 that is 343 x 2^-24 = 2^-15.6, not the 2^-22 one might hope for: the worst case grows with the chain.
    Measured on an MI355X: 3.2e-7 for S = 1 against 48, 2.9e-7 for 1 against 7, 8.6e-8 for 7 against 48 -- the first two
    above 2^-22 = 2.4e-7.)"""
    B, C, N = 3, 128, 128
    pairs = B * 16
    x, dy, _, xd, dyd, xs, xmax, dys, dymax = wgrad_operands(ops, B, C, N, True, 1)
    ref = fo.wgrad64(x, dy)
    for v, S_want in ((3, 1), (3 * pairs, pairs), (21, 7)):
        tune(ops, 1, v)
        dw, S = wgrad_planes(ops, xs, xmax, dys, dymax, B, 32, C, N)
        assert S == S_want
        exact(dw, ref)
    tune(ops, 1, 4)
    dw, S = wgrad9(ops, xd, dyd, xmax=xmax, dymax=dymax)
    assert S == 1
    exact(dw, ref)
    tune(ops, 1, 0)
    x, dy, _, xd, dyd, xs, xmax, dys, dymax = wgrad_operands(ops, B, C, N, False, 2)
    mag = fo.wgrad_ref(x, dy)[1]
    runs = {}
    for v in (3, 3 * pairs, 21, 0):
        tune(ops, 1, v)
        dw, S = wgrad_planes(ops, xs, xmax, dys, dymax, B, 32, C, N)
        runs[S] = dw
    assert sorted(runs) == [1, 7, 48]                          # (the default count is the 48 pairs as well)
    n = lambda S: 6 * -(-pairs // S) + S
    for a, b in ((1, 48), (1, 7), (7, 48)):
        ratio = float((np.abs(runs[a] - runs[b]) / mag).max())
        print(f"plane-fed dw, S = {a} against {b}: worst difference / mag = {ratio:.3e} (bar {(n(a) + n(b)) * 2.0 ** -24:.3e})")
        assert ratio <= (n(a) + n(b)) * 2.0 ** -24


# ------------------------------------------------------------------------------------------------ d, e. scales and bars
def held(name, got, ref, bar, B):
    err = np.abs(got - ref)
    ratio = np.where(bar > 0, err / np.where(bar > 0, bar, 1.0), np.where(err > 0, np.inf, 0.0)).reshape(B, -1).max(axis=1)
    print(f"{name}: worst error / bar per image {np.array2string(ratio, precision=3)}")
    assert np.all(np.isfinite(got))
    assert np.all(err <= bar), name


@pytest.mark.parametrize("name", sorted(cases.CASES))
def test_forward_and_input_gradient_per_image_and_element(ops, name):
    """every element of every image within 3e-6 mag of float64, plus the floor of the split for the images under the
    scale clamp (a maximum below 2^-113, subnormal or zero); an all-zero image gives exact zeros, or exactly
    (bias + cbias) + res in fp32; the planes are the host's bits whatever the scale"""
    s = cases.conv_case(name)
    B, H, C, N, x, w, dy = s["B"], s["H"], s["C"], s["N"], s["x"], s["w"], s["dy"]
    wd = dev(w)
    wp, wmax = pack(ops, wd, 0)
    ref, mag = fo.conv_ref(x, w)
    y, xs, _, _ = fwd(ops, dev(x), wp, wmax, N, want_xs=True)
    got = y.np_f32(B, H, 32, N)
    held(name + " forward", got, ref, cases.image_bar(fo, x, w, mag), B)
    assert same_planes(xs, x)
    ref, mag = fo.conv_ref(x, w, s["bias"], s["cbias"], s["res"])
    y, _, ymax, _ = fwd(ops, dev(x), wp, wmax, N, bias=dev(s["bias"]), cbias=dev(s["cbias"]), res=dev(s["res"]), want_ymax=True)
    got2 = y.np_f32(B, H, 32, N)
    held(name + " forward + bias + cbias + res", got2, ref, cases.image_bar(fo, x, w, mag), B)
    check_ymax(ymax, got2, B, (H // ops.lib.load().mulan_conv3x3_f16x3_tile_rows(B, H, N, 1)) * (N // 128))
    for b in np.flatnonzero(np.abs(x).reshape(B, -1).max(axis=1) == 0):
        assert not np.any(got[b])
        assert np.array_equal(got2[b], (s["bias"] + s["cbias"][b])[None, None, :] + s["res"][b])
    wpf, _ = pack(ops, wd, 1)
    ref, mag = fo.dgrad_ref(dy, w)
    dx, dys, _, _ = fwd(ops, dev(dy), wpf, wmax, C, want_xs=True)
    held(name + " input gradient", dx.np_f32(B, H, 32, C), ref, cases.image_bar(fo, dy, fo.flip_conv(w), mag), B)
    assert same_planes(dys, dy)


@pytest.mark.parametrize("name", sorted(cases.CASES))
def test_weight_gradients_per_element_beside_the_fp32_kernel(ops, name):
    """dw from (x, g) and from (xg, dy) -- the scale extremes on either operand -- by the nine-tap and the plane-fed kernel:
    every element and tap within 3e-6 |x|^T |dy| of float64.  At H = 32 the fp32 kernel (mulan_conv3x3_wgrad) runs on the
    same inputs and both worst ratios are printed: the bar would be 2 e32 + the model's own error if e32 exceeded 3e-6.
    Measured on an MI355X (worst error / |x|^T |dy|): gauss_h32 nine-tap 1.41e-7 / 1.38e-7, plane-fed 1.22e-7 / 1.20e-7,
    fp32 kernel 2.02e-7 / 1.83e-7 for the two operand pairs, so the 3e-6 bar stands; gauss_h24 1.8e-7 / 1.0e-7, the clamp
    sets 1.9e-7 / 7.1e-8 (nine-tap / plane-fed); the exact-accumulator model alone 4e-8 to 7.5e-8."""
    s = cases.conv_case(name)
    B, H, C, N = s["B"], s["H"], s["C"], s["N"]
    L = ops.lib.load()
    for what, a, g in (("dw(x, g)", s["x"], s["g"]), ("dw(xg, dy)", s["xg"], s["dy"])):
        ref, mag = fo.wgrad_ref(a, g)
        ad, gd = dev(a), dev(g)
        d9, _ = wgrad9(ops, ad, gd)
        xs, xmax = planes_by_product(ops, ad)
        dys, dymax = planes_by_product(ops, gd)
        dp, _ = wgrad_planes(ops, xs, xmax, dys, dymax, B, H, C, N)
        e9, ep = float((np.abs(d9 - ref) / mag).max()), float((np.abs(dp - ref) / mag).max())
        line = f"{name} {what}: worst error / mag nine-tap {e9:.3e}, plane-fed {ep:.3e}"
        if H == 32:
            ws, dw = Buf(L.mulan_conv3x3_wgrad_workspace(B, H, 32, C, N)), Buf(9 * C * N * 4)
            ops.call("mulan_conv3x3_wgrad", ops.ptr(ad), ops.ptr(gd), dw.ptr, ws.ptr, B, H, 32, C, N, 0, ops.stream())
            torch.cuda.synchronize()
            assert ws.guard_ok() and dw.guard_ok()
            e32 = float((np.abs(dw.np_f32(3, 3, C, N) - ref) / mag).max())
            line += f", fp32 kernel {e32:.3e}"
        print(line + f" (bar {cases.BAR:.0e})")
        assert np.all(np.isfinite(d9)) and np.all(np.isfinite(dp))
        assert e9 < cases.BAR and ep < cases.BAR


def test_a_non_finite_value_stays_inside_its_image(ops):
    """one +Inf in image 2: the outputs and planes of images 0, 1 and 3 keep their bits (one scale per image)"""
    s = cases.conv_case("clamp_small")
    B, H, N = s["B"], s["H"], s["N"]
    wp, wmax = pack(ops, dev(s["w"]), 0)
    x = dev(s["x"])
    y0, xs0, _, _ = fwd(ops, x, wp, wmax, N, want_xs=True)
    x[2, 3, 5, 7] = float("inf")
    y1, xs1, _, _ = fwd(ops, x, wp, wmax, N, want_xs=True)
    a, b = y0.body.view(B, -1), y1.body.view(B, -1)
    pa, pb = xs0.body.view(B, -1), xs1.body.view(B, -1)
    for i in (0, 1, 3):
        assert torch.equal(a[i], b[i]) and torch.equal(pa[i], pb[i]), i
    assert not bool(torch.isfinite(y1.f32(B, H * 32 * N)[2]).all())
