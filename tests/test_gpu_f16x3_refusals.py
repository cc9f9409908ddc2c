"""The argument checks of the f16x3 forward convolutions (mulan_amd/csrc/conv3x3_f16x3.hip) and of the f16x3 weight
gradients (mulan_amd/csrc/wgrad_f16x3.hip), entry point by entry point.

The two tables below were read off the conditions each entry point carried while they were written out one by one (the
comments above the tables list them), not off the shared checks the entry points call now.  R = the call returns
hipErrorInvalidValue and every output buffer still holds its sentinel bytes; A = the call returns 0 and its result is
exact on integer data (the bar of tests/test_gpu_f16x3.py and tests/test_gpu_linear_f16x3.py for integers); - = the entry
point has no such argument, or does not look at it.  Accepted rows run at the smallest shapes the kernels take.

Plane tensors that a weight-gradient kernel reads have the layout the header documents and the forward kernels write,
[B][C/16][H * W][plane][16]: H * 32 pixels per image (tests/test_gpu_conv_f16x3.py holds writers and readers to it at
other heights); the images differ by powers of two, so a kernel that read past an image's end would sum the next one.

The 2 GiB limit is held without a device (test_two_gib_tensors_are_refused_without_a_device): a wrongly accepted call
would launch over buffers far smaller than its shape claims."""
import numpy as np
import pytest
import torch

from oracle import mulan_np as onp
from tests import f16x3_oracle as fo
from tests.test_gpu_linear_f16x3 import Buf, bufptr, dev

INVALID = 1                      # hipErrorInvalidValue


@pytest.fixture()
def ops(monkeypatch):
    from mulan_amd import ops as _ops
    _ops.lib.load()
    monkeypatch.setattr(_ops, "CONV_MODE", "f16x3")
    yield _ops
    _ops.call("mulan_set_tuning", 1, 0)


def maxima_of(value, B=1):
    """[B][16] maxima array with `value` as the only partial of every row"""
    m = np.zeros((B, 16), np.uint32)
    m[:, 0] = fo.bits_of(value)
    return torch.as_tensor(m.view(np.int32)).cuda()


def planes_dev(x, rows):
    """x [B, rows, C] -> (its split planes [B][C/16][rows][2][16] on the device, the [B][16] maxima they are scaled with);
    C off the 16-channel chunks (refused everywhere): a stand-in of 16 bytes"""
    B, _, C = x.shape
    if C % 16 != 0:
        return torch.zeros(16, dtype=torch.uint8, device="cuda"), maxima_of(1.0, B)
    pl = fo.planes_of(x.reshape(B * rows, C), None, rows)
    m = np.zeros((B, 16), np.uint32)
    m[:, 0] = fo.row_max16(x)
    return torch.as_tensor(pl.view(np.uint8)).cuda(), torch.as_tensor(m.view(np.int32)).cuda()


def null(t, name, nulls):
    return None if name in nulls else (t.ptr if isinstance(t, Buf) else t.data_ptr())


# ------------------------------------------------------------------------------------------------ forward
FWD = ("fwd", "fwd_alone", "planes_in", "planes_in_stats", "gn_in")
# The conditions as each entry point stated them:
#   fwd, fwd_alone:             W == 32, H % 8, B > 0, C > 0, C % 16, N > 0, N % 128, xmax, wmax; with xs: below 2 GiB;
#                               with ymax: (H / 8) * (N / 128) <= 16
#   planes_in, planes_in_stats: W == 32, B, C, N > 0, xplanes, xmax, wmax, H % 8, C % 32, N % 128, below 2 GiB, the ymax cap
#   gn_in:                      as planes_in with x1, gamma, beta, mean, rstd, bound in place of xplanes / xmax, and G > 0,
#                               C2 == C1 with x2, G | C, 4 | C / G, C <= 512, xstats2 with xstats1 and x2, not ystats together
#                               with yplanes_out, xstats_tiles in {H / 8, H / 4, H / 2} with xstats1
# row -> (what it changes on the valid call B = 1, H = 8, W = 32, C = 32, N = 128 with ymax, per entry point of FWD)
FWD_ROWS = {
    "valid":            (dict(),                                  "AAAAA"),
    "W=16":             (dict(W=16),                              "RRRRR"),
    "H=12":             (dict(H=12),                              "RRRRR"),
    "B=0":              (dict(B=0),                               "RRRRR"),
    "C=16":             (dict(C=16),                              "AARRR"),   # the 32x32x16 kernel's own shape
    "C=24":             (dict(C=24),                              "RRRRR"),
    "N=64":             (dict(N=64),                              "RRRRR"),
    "no xmax":          (dict(nulls=("xmax",)),                   "RRRRR"),   # (gn_in: its bound)
    "no wmax":          (dict(nulls=("wmax",)),                   "RRRRR"),
    "no planes":        (dict(nulls=("xplanes",)),                "--RR-"),
    "ymax, 20 blocks":  (dict(H=32, N=640),                       "RRRRR"),
    "C2!=C1":           (dict(C2=64),                             "----R"),
    "C=640":            (dict(C=640, G=32),                       "----R"),
    "ystats+planes":    (dict(ystats=True, yplanes=True),         "----R"),
    "xstats_tiles=3":   (dict(xstats=True, tiles=3),              "----R"),
    "xstats_tiles=0":   (dict(xstats=True, tiles=0),              "----R"),
    "no x1":            (dict(nulls=("x1",)),                     "----R"),
}
FWD_CELLS = [pytest.param(e, row, want[i], id=f"{e}-{row}")
             for row, (_, want) in FWD_ROWS.items() for i, e in enumerate(FWD) if want[i] != "-"]


def run_fwd(ops, entry, B=1, H=8, W=32, C=32, N=128, nulls=(), C2=0, G=4, ystats=False, yplanes=False, xstats=False, tiles=0):
    """one call of a forward entry point on integer data of the claimed shape -> (rc, outputs as Bufs, reference or None)"""
    L, s = ops.lib.load(), ops.stream()
    rng = np.random.default_rng(H + C + N)
    Bm = max(B, 1)
    x = rng.integers(-3, 4, (Bm, H, 32, C)).astype(np.float64)
    w = rng.integers(-2, 3, (3, 3, C, N)).astype(np.float64)
    bias, cb = rng.integers(-3, 4, N).astype(np.float64), rng.integers(-3, 4, (Bm, N)).astype(np.float64)
    res = rng.integers(-3, 4, (Bm, H, 32, N)).astype(np.float64)
    xd, wd, biasd, cbd, resd = dev(x), dev(w), dev(bias), dev(cb), dev(res)
    wmax = ops.absmax_rows(wd.view(1, -1))
    wp = Buf(L.mulan_conv3x3_pack_f16x3_bytes(C, N))
    if C % 16 == 0:
        ops.call("mulan_conv3x3_pack_f16x3", wd.data_ptr(), wp.ptr, wmax.data_ptr(), C, N, 0, s)
    rows = L.mulan_conv3x3_f16x3_tile_rows(Bm, H, N, 1)
    out = dict(y=Buf(Bm * H * 32 * N * 4), ymax=Buf(Bm * 16 * 4), xs=Buf(Bm * 1024 * (C + C2) * 4),
               ystats=Buf(Bm * max(H // rows, 1) * (N // 4) * 2 * 4))
    gn = None
    if entry in ("fwd", "fwd_alone"):
        xmax = ops.absmax_rows(xd.view(Bm, -1))
        args = (xd.data_ptr(), null(xmax, "xmax", nulls), wp.ptr, null(wmax, "wmax", nulls), biasd.data_ptr(), cbd.data_ptr(), 1,
                resd.data_ptr(), out["y"].ptr, out["xs"].ptr, out["ymax"].ptr)
        rc = (L.mulan_conv3x3_fwd_f16x3(*args, B, H, W, C, N, s) if entry == "fwd" else
              L.mulan_conv3x3_fwd_f16x3_alone(*args, 1, B, H, W, C, N, s))
    elif entry in ("planes_in", "planes_in_stats"):
        xpl, xmax = planes_dev(x.reshape(Bm, H * 32, C), H * 32)
        args = (null(xpl, "xplanes", nulls), null(xmax, "xmax", nulls), wp.ptr, null(wmax, "wmax", nulls), biasd.data_ptr(),
                cbd.data_ptr(), 1, resd.data_ptr(), out["y"].ptr, out["ymax"].ptr)
        rc = (L.mulan_conv3x3_fwd_f16x3_planes_in(*args, B, H, W, C, N, s) if entry == "planes_in" else
              L.mulan_conv3x3_fwd_f16x3_planes_in_stats(*args, out["ystats"].ptr, 1, B, H, W, C, N, s))
    else:
        # statistics and affine parameters in integers and powers of two: (x - mean) * rstd * gamma + beta is exact in fp32
        # in whichever order it is formed; no activation
        cpg = max(C // G, 1)
        mean = rng.integers(-1, 2, (Bm, G)).astype(np.float64)
        rstd = 2.0 ** rng.integers(-1, 2, (Bm, G))
        gamma, beta = 2.0 ** rng.integers(0, 2, C), rng.integers(-2, 3, C).astype(np.float64)
        grp = np.minimum(np.arange(C) // cpg, G - 1)
        gn = (x - mean[:, None, None, grp]) * rstd[:, None, None, grp] * gamma + beta
        meand, rstdd, gammad, betad = dev(mean), dev(rstd), dev(gamma), dev(beta)
        bound = maxima_of(np.abs(gn).reshape(Bm, -1).max(1), Bm)
        x2 = torch.zeros(Bm * H * 32 * C2, device="cuda") if C2 else None
        st = torch.zeros(Bm * 4 * (C // 4) * 2, device="cuda") if xstats else None
        rc = L.mulan_conv3x3_fwd_f16x3_gn_in(
            null(xd, "x1", nulls), ops.ptr(x2), C, C2, gammad.data_ptr(), betad.data_ptr(), meand.data_ptr(), rstdd.data_ptr(), G, 0,
            1e-6, null(bound, "xmax", nulls), ops.ptr(st), None, tiles, wp.ptr, null(wmax, "wmax", nulls), biasd.data_ptr(),
            cbd.data_ptr(), 1, resd.data_ptr(), out["y"].ptr, out["ymax"].ptr, out["ystats"].ptr if ystats else None,
            out["xs"].ptr if yplanes else None, B, H, W, N, s)
    torch.cuda.synchronize()
    ref = onp.conv3x3(x if gn is None else gn, w, bias) + cb[:, None, None, :] + res
    return rc, out, ref


@pytest.mark.gpu
@pytest.mark.parametrize("entry,row,want", FWD_CELLS)
def test_forward_refusals_are_per_entry_point(ops, entry, row, want):
    """FWD_ROWS, cell by cell: C = 16 is accepted by mulan_conv3x3_fwd_f16x3 (the 32x32x16 kernel) and refused by the
    plane-fed and GroupNorm-fed entry points; the GroupNorm and statistics rules are _gn_in's own.  Accepted: y is exact,
    the maxima of y are its maximum, the partial sums of _planes_in_stats are those of y (the sums exactly; the sums of
    squares, 256 positive terms each, to 256 * 2^-24), and nothing writes past a buffer."""
    rc, out, ref = run_fwd(ops, entry, **FWD_ROWS[row][0])
    assert all(b.guard_ok() for b in out.values())
    if want == "R":
        assert rc == INVALID, (entry, row, rc)
        assert all(b.untouched() for b in out.values()), {k: b.untouched() for k, b in out.items()}
        return
    assert rc == 0, (entry, row, rc)
    B, H, _, N = ref.shape
    y = out["y"].np_f32(B, H, 32, N).astype(np.float64)
    assert np.array_equal(y, ref)
    ymax = out["ymax"].body.view(torch.int32).cpu().numpy().view(np.uint32).reshape(B, 16)
    assert np.array_equal(ymax.max(1), fo.row_max16(ref))
    if entry == "planes_in_stats":
        rows = ops.lib.load().mulan_conv3x3_f16x3_tile_rows(B, H, N, 1)
        st = out["ystats"].np_f32(B, H // rows, N // 4, 2).astype(np.float64)
        tiles = ref.reshape(B, H // rows, rows * 32, N // 4, 4)
        assert np.array_equal(st[..., 0], tiles.sum((2, 4)))
        assert np.allclose(st[..., 1], (tiles * tiles).sum((2, 4)), rtol=256 * 2.0 ** -24, atol=0)
    else:
        assert out["ystats"].untouched()


# ------------------------------------------------------------------------------------------------ weight gradients
WG = ("wgrad", "wgrad_planes", "linear_planes", "linear_x32", "bmm_tn")
# The conditions as each entry point stated them:
#   wgrad (fp32 operands):       W == 32, H % 2, B > 0, C % 4, N % 4, xmax, dymax  (x, dy and dw are not looked at)
#   wgrad_planes, linear_planes: W == 32, H % 2, B > 0, C % 128, N % 128, xs, dys, xmax, dymax, below 2 GiB
#   linear_x32:                  W == 32, H == 32, B > 0, C1 > 0, C1 % 128, C2 >= 0, C2 % 128, N % 128, x1, with C2 > 0: x2
#                                and xmax2, dys, xmax, dymax, below 2 GiB
#   bmm_tn:                      as linear_planes, and out
# Valid calls: wgrad and wgrad_planes B = 2, H = 4, linear_planes and bmm_tn B = 2, H = 2, linear_x32 B = 1, H = 32,
# C1 = 128, C2 = 0; C = N = 128 throughout.
WG_ROWS = {
    "valid":            (dict(),                                  "AAAAA"),
    "W=16":             (dict(W=16),                              "RRRRR"),
    "H=3":              (dict(H=3),                               "RRRRR"),
    "H=4":              (dict(H=4),                               "---R-"),   # (accepted by the others: their valid call)
    "B=0":              (dict(B=0),                               "RRRRR"),
    "C=64":             (dict(C=64),                              "ARRRR"),
    "N=64":             (dict(N=64),                              "ARRRR"),
    "C=6":              (dict(C=6),                               "RRRRR"),
    "N=130":            (dict(N=130),                             "RRRRR"),
    "no xmax":          (dict(nulls=("xmax",)),                   "RRRRR"),
    "no dymax":         (dict(nulls=("dymax",)),                  "RRRRR"),
    "no x":             (dict(nulls=("x",)),                      "-RRRR"),   # (planes of x; linear_x32: x1)
    "no dys":           (dict(nulls=("dys",)),                    "-RRRR"),
    "no out":           (dict(nulls=("out",)),                    "----R"),
    "C2=128":           (dict(C2=128),                            "---A-"),
    "C2=64":            (dict(C2=64),                             "---R-"),
    "C2=128, no x2":    (dict(C2=128, nulls=("x2",)),             "---R-"),
    "C2=128, no xmax2": (dict(C2=128, nulls=("xmax2",)),          "---R-"),
}
WG_CELLS = [pytest.param(e, row, want[i], id=f"{e}-{row}")
            for row, (_, want) in WG_ROWS.items() for i, e in enumerate(WG) if want[i] != "-"]
WG_VALID = dict(wgrad=(2, 4), wgrad_planes=(2, 4), linear_planes=(2, 2), linear_x32=(1, 32), bmm_tn=(2, 2))


def wgrad3x3_ref(x, dy):
    """dw[kh][kw][c][n] = sum over images and pixels of x[h + kh - 1][w + kw - 1][c] dy[h][w][n], zero padding"""
    H = x.shape[1]
    xp = np.pad(x, ((0, 0), (1, 1), (1, 1), (0, 0)))
    return np.stack([np.stack([np.einsum("bhwc,bhwn->cn", xp[:, kh:kh + H, kw:kw + 32], dy) for kw in range(3)])
                     for kh in range(3)])


def run_wg(ops, entry, B=None, H=None, W=32, C=128, N=128, C2=0, nulls=()):
    """one call of a weight-gradient entry point on integer data of the claimed shape -> (rc, outputs, reference)"""
    L, s = ops.lib.load(), ops.stream()
    B = WG_VALID[entry][0] if B is None else B
    H = WG_VALID[entry][1] if H is None else H
    rng = np.random.default_rng(H + C + N + C2)
    Bm, Ct, px = max(B, 1), C + C2, H * 32
    # [Bm, 1024, channels] with image b at the power of two 2^b; the first H * 32 pixels of an image are the call's operand
    x = rng.integers(-3, 4, (Bm, 1024, Ct)) * 2.0 ** np.arange(Bm)[:, None, None]
    dy = rng.integers(-2, 3, (Bm, 1024, N)) * 2.0 ** (3 * np.arange(Bm))[:, None, None]
    xin, dyin = x[:, :px], dy[:, :px]
    nine = entry in ("wgrad", "wgrad_planes")
    # the 3x3 kernels at a block target of 3 (tune key 1): one split, so that a block's pixel range crosses from image 0
    # into image 1 (at their default targets four row pairs make four splits of one pair each)
    ops.call("mulan_set_tuning", 1, 3 if nine else 0)
    if entry == "wgrad":
        nbytes = L.mulan_conv3x3_wgrad_f16x3_workspace(B, H, W, C, N)
    elif entry == "wgrad_planes":
        nbytes = L.mulan_conv3x3_wgrad_f16x3_planes_workspace(B, H, W, C, N, 0)
    else:
        nbytes = getattr(L, "mulan_linear_wgrad_f16x3_" + ("x32" if entry == "linear_x32" else "planes") + "_workspace")(
            B, H, W, Ct, N, 0)
    n_out = (Bm if entry == "bmm_tn" else 1) * (9 if nine else 1) * Ct * N
    out = dict(dw=Buf(n_out * 4), ws=Buf(nbytes))
    dw = null(out["dw"], "out", nulls)
    if entry == "wgrad":
        xd, dyd = dev(xin), dev(dyin)
        xmax, dymax = ops.absmax_rows(xd.view(Bm, -1)), ops.absmax_rows(dyd.view(Bm, -1))
        rc = L.mulan_conv3x3_wgrad_f16x3(xd.data_ptr(), null(xmax, "xmax", nulls), dyd.data_ptr(), null(dymax, "dymax", nulls),
                                         dw, out["ws"].ptr, B, H, W, C, N, 0, s)
    else:
        dys, dymax = planes_dev(dyin, px)
        dysp, dymaxp = null(dys, "dys", nulls), null(dymax, "dymax", nulls)
        if entry == "linear_x32":
            x1, x2 = dev(xin[..., :C]), (dev(xin[..., C:]) if C2 else None)
            m1, m2 = ops.absmax_rows(x1.view(Bm, -1)), (ops.absmax_rows(x2.view(Bm, -1)) if C2 else None)
            rc = L.mulan_linear_wgrad_f16x3_x32(
                null(x1, "x", nulls), None if x2 is None or "x2" in nulls else x2.data_ptr(), C, C2, null(m1, "xmax", nulls),
                None if m2 is None or "xmax2" in nulls else m2.data_ptr(), dysp, dymaxp, dw, out["ws"].ptr, B, H, W, N, 0, 0, s)
        else:
            xs, xmax = planes_dev(xin, px)
            a = (null(xs, "x", nulls), null(xmax, "xmax", nulls), dysp, dymaxp, dw)
            if entry == "bmm_tn":
                rc = L.mulan_bmm_tn_f16x3_planes(*a, B, H, W, C, N, s)
            else:
                fn = L.mulan_conv3x3_wgrad_f16x3_planes if nine else L.mulan_linear_wgrad_f16x3_planes
                rc = fn(*a, out["ws"].ptr, B, H, W, C, N, 0, 0, s)
    torch.cuda.synchronize()
    if nine:
        ref = wgrad3x3_ref(xin.reshape(Bm, H, 32, Ct), dyin.reshape(Bm, H, 32, N))
    else:
        ref = np.einsum("bpc,bpn->bcn", xin, dyin)
        ref = ref if entry == "bmm_tn" else ref.sum(0)
    return rc, out, ref


@pytest.mark.gpu
@pytest.mark.parametrize("entry,row,want", WG_CELLS)
def test_weight_gradient_refusals_are_per_entry_point(ops, entry, row, want):
    """WG_ROWS, cell by cell: C = 64 is accepted by the fp32-fed kernel and refused by the plane-fed ones, H = 4 is refused
    by _x32 alone, a second input needs its tensor and its maxima.  Accepted: dw (bmm_tn: every image's product) is exact on
    integers with the images at different powers of two, and nothing writes past dw or past the workspace the _workspace
    function sized."""
    rc, out, ref = run_wg(ops, entry, **WG_ROWS[row][0])
    assert all(b.guard_ok() for b in out.values())
    if want == "R":
        assert rc == INVALID, (entry, row, rc)
        assert all(b.untouched() for b in out.values()), {k: b.untouched() for k, b in out.items()}
        return
    assert rc == 0, (entry, row, rc)
    assert np.array_equal(out["dw"].np_f32(*ref.shape).astype(np.float64), ref)


@pytest.mark.gpu
def test_workspaces_answer_zero_off_the_grid(ops):
    """the _workspace functions: 0 where W, H % 2 (all) or the 128-grids of C and N (plane-fed) fail, whole slabs otherwise"""
    L = ops.lib.load()
    plane_fed = (L.mulan_conv3x3_wgrad_f16x3_planes_workspace, L.mulan_linear_wgrad_f16x3_planes_workspace,
                 L.mulan_linear_wgrad_f16x3_x32_workspace)
    for i, fn in enumerate(plane_fed):
        slab = (9 if i == 0 else 1) * 128 * 256 * 4
        for share in (0, 1):
            n = fn(2, 4, 32, 128, 256, share)
            assert n > 0 and n % slab == 0 and n // slab <= 4          # (at most one slab per row pair)
            for bad in ((2, 4, 16, 128, 256), (2, 3, 32, 128, 256), (2, 4, 32, 64, 256), (2, 4, 32, 128, 192)):
                assert fn(*bad, share) == 0, (i, bad)
    n = L.mulan_conv3x3_wgrad_f16x3_workspace(2, 4, 32, 64, 12)
    assert n > 0 and n % (9 * 64 * 12 * 4) == 0
    assert L.mulan_conv3x3_wgrad_f16x3_workspace(2, 4, 16, 64, 12) == 0 and L.mulan_conv3x3_wgrad_f16x3_workspace(2, 3, 32, 64, 12) == 0


# ------------------------------------------------------------------------------------------------ 2 GiB, no device
@pytest.mark.skipif(torch.cuda.is_available(), reason="a wrongly accepted call would launch over buffers it does not own")
def test_two_gib_tensors_are_refused_without_a_device():
    """B = 1024, H = W = 32, C = 512: 2^31 bytes of fp32 input (or of planes).  The plane-fed forward entry points, the
    fp32-fed ones when they are to write planes, and every plane-fed weight gradient refuse before any HIP call; the
    pointers are never followed.  (mulan_conv3x3_fwd_f16x3 without `xs` accepts the shape: not run here.)"""
    from mulan_amd import lib
    L = lib.load()
    p, s = 4096, None
    B, H, W, C, N = 1024, 32, 32, 512, 128
    conv = (p, p, p, p, None, None, 0, None, p)
    assert L.mulan_conv3x3_fwd_f16x3(*conv, p, None, B, H, W, C, N, s) == INVALID
    assert L.mulan_conv3x3_fwd_f16x3_alone(*conv, p, None, 1, B, H, W, C, N, s) == INVALID
    assert L.mulan_conv3x3_fwd_f16x3_planes_in(*conv, None, B, H, W, C, N, s) == INVALID
    assert L.mulan_conv3x3_fwd_f16x3_planes_in_stats(*conv, None, None, 0, B, H, W, C, N, s) == INVALID
    assert L.mulan_conv3x3_fwd_f16x3_gn_in(p, None, C, 0, p, p, p, p, 32, 1, 1e-6, p, None, None, 0, p, p, None, None, 0, None,
                                           p, None, None, None, B, H, W, N, s) == INVALID
    for c, n in ((C, N), (N, C)):                   # the larger of the two tensors counts
        assert L.mulan_conv3x3_wgrad_f16x3_planes(p, p, p, p, p, p, B, H, W, c, n, 0, 0, s) == INVALID
        assert L.mulan_linear_wgrad_f16x3_planes(p, p, p, p, p, p, B, H, W, c, n, 0, 0, s) == INVALID
        assert L.mulan_linear_wgrad_f16x3_x32(p, None, c, 0, p, None, p, p, p, p, B, H, W, n, 0, 0, s) == INVALID
        assert L.mulan_bmm_tn_f16x3_planes(p, p, p, p, p, B, H, W, c, n, s) == INVALID
