"""The reduction kernels off the model's shapes, against float64: the column sums (colsum_kernel, colsum_vec_kernel
behind mulan_colsum, mulan_colsum_pair and ops.colsum_raw), the row softmax with its rowmax by-product, the per-row
maxima (mulan_absmax_rows, mulan_add_absmax_rows, mulan_add_absmax_rows_colsum) and the kernels that reduce one row
per wave (mulan_rowmean, mulan_attention_delta, mulan_temb_bwd with mulan_temb_fwd).

Data, references and bars come from tests/reduction_oracle.py (its header derives every bar; tests/test_reduction_oracle.py
holds them without a device).  Every reduction runs on small integers (bit-equal to the exact sum) and on cancelling
floats (|sum| ~ 1e-5 sum |x|) at the derived bars; softmax and the timestep embedding at a bar measured inside the test
from an fp32 numpy twin (4 x the twin's worst error, at least 4 ulp of the row's largest reference value).  Every output
lies in a poisoned buffer whose bytes outside the result must come back unchanged; a refusal returns
hipErrorInvalidValue and writes nothing.  Each test prints its worst error / bar.

Defect found by this file: mulan_temb_fwd / mulan_temb_bwd accepted col0 + E > ld (the table's ld = E, col0 = 8), where
a row's last 8 columns are the next row's first 8 (and the last row ends 8 floats past the buffer); the entry points
now refuse it and test_temb holds the refusal."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import reduction_oracle as ro

INVALID = 1                          # hipErrorInvalidValue
POISON = 0x7FC0DEAD                  # a NaN with a payload: never the result of arithmetic
GUARD = 64                           # floats in front of and behind an output (a multiple of 4: alignment is kept)
KINDS = ("ints", "floats")


@pytest.fixture(scope="module")
def ops():
    from mulan_amd import ops as _ops
    _ops.lib.load()
    return _ops


def dev(a, dtype=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(a)).to(dtype).cuda()


def poisoned(*shape):
    return torch.full(shape, POISON, dtype=torch.int32, device="cuda").view(torch.float32)


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32).numpy()


def is_poison(t):
    return bool((bits(t) == POISON).all())


def host(t):
    return t.detach().cpu().double().numpy()


def raw(ops, name, *args):
    """the entry point's return code, unchecked"""
    rc = getattr(ops.lib.load(), name)(*args, ops.stream())
    torch.cuda.synchronize()
    return rc


def worst(err, bar):
    return float((np.asarray(err) / np.asarray(bar)).max())


# ====================================================================================================== 1. mulan_colsum
@pytest.mark.parametrize("cfg,seg", ro.COLSUM_TABLE, ids=[f"{c.kernel}-C{c.C}-ld{c.ld}-x{c.x_off}-o{c.out_off}-seg{s}"
                                                         for c, s in ro.COLSUM_TABLE])
def test_colsum_direct(ops, cfg, seg):
    """nseg in {1, 3} x accumulate in {0, 1} x {ints, floats}: the kernel the dispatch condition selects is the one the
    table names; integers exact; floats at f64_bar (scalar kernel: float64 accumulation) or the fp32 bound with the old
    value as one more term (vector kernel); the guards around the pre-filled output come back bit-unchanged.
    MI355X: worst error / bar 0.998 (scalar: the one rounding to fp32 can use all of u |ref|), 0.25 (vector)."""
    C, ld = cfg.C, cfg.ld
    ratio = 0.0
    for nseg in ro.COLSUM_NSEG:
        for kind in KINDS:
            x, terms, old = ro.colsum_data(kind, nseg, seg, C, ld)
            xbuf = torch.empty(cfg.x_off + x.size, dtype=torch.float32, device="cuda")
            xd = xbuf[cfg.x_off:]
            xd.copy_(dev(x).view(-1))
            for acc in (0, 1):
                buf = poisoned(2 * GUARD + nseg * C + 4)
                lo = GUARD + cfg.out_off
                out = buf[lo:lo + nseg * C]
                out.copy_(dev(old).view(-1))
                assert ro.colsum_vec_dispatch(C, ld, xd.data_ptr(), out.data_ptr()) == (cfg.kernel == "vector")
                ops.call("mulan_colsum", xd.data_ptr(), out.data_ptr(), nseg, seg, C, ld, acc, ops.stream())
                assert is_poison(buf[:lo]) and is_poison(buf[lo + nseg * C:]), (nseg, kind, acc)
                got = host(out).reshape(nseg, C)
                ref = terms.sum(axis=1) + (old if acc else 0.0)
                if kind == "ints":
                    assert np.array_equal(got, ref), (nseg, acc)
                    continue
                sabs = np.abs(terms).sum(axis=1)
                if cfg.kernel == "scalar":
                    bar = ro.f64_bar(terms.sum(axis=1), seg, sabs, total=ref if acc else None)
                else:
                    bar = (seg + acc + 2) * ro.U * (sabs + acc * np.abs(old))
                r = worst(np.abs(got - ref), bar)
                ratio = max(ratio, r)
                assert r <= 1.0, (nseg, acc, r)
    print(f"colsum {cfg} seg {seg}: worst error / bar {ratio:.3g}")


# ====================================================================================================== 2. ops.colsum_raw
@pytest.mark.parametrize("seg,C,ld", ro.RAW_TABLE)
def test_colsum_raw_routes(ops, seg, C, ld):
    """seg = 2048, 2560: two launches with fp32 partials of 512 rows in between; seg = 2047: one.  Every route is held to
    the fp32 bound with n = seg; the scalar kernel (C = 3) besides to f64_bar (one stage) or two_stage_bar.
    MI355X: worst error / bar 0.48 (C = 3 against its route's own bar; 8.4e-6 of the fp32 bound), 1.9e-4 (C = 132)."""
    nseg = ro.RAW_NSEG
    for kind in KINDS:
        x, terms, _ = ro.colsum_data(kind, nseg, seg, C, ld, tag="raw")
        got = host(ops.colsum_raw(dev(x), nseg, seg, C, ld=ld))
        ref = terms.sum(axis=1)
        if kind == "ints":
            assert np.array_equal(got, ref)
            continue
        err, sabs = np.abs(got - ref), np.abs(terms).sum(axis=1)
        loose = worst(err, ro.fp32_bar(terms, 1, n=seg))
        tight = loose
        if C % 4:
            tight = worst(err, ro.two_stage_bar(terms) if ro.raw_two_stage(seg) else ro.f64_bar(ref, seg, sabs))
        print(f"colsum_raw seg {seg} C {C} ld {ld}: error / fp32 bound {loose:.3g}, / the route's own bar {tight:.3g}")
        assert loose <= 1.0 and tight <= 1.0


# ====================================================================================================== 3. mulan_colsum_pair
def _pair_buffer(C):
    """out1 in front of out0, a gap between them, guards around both"""
    buf = poisoned(3 * GUARD + 2 * C)
    return buf, buf[2 * GUARD + C:2 * GUARD + 2 * C], buf[GUARD:GUARD + C]


@pytest.mark.parametrize("seg,C", ro.PAIR_TABLE)
def test_colsum_pair(ops, seg, C):
    """segment 0 to out0, segment 1 to out1 (which lies BEFORE out0 here, so out0 + C is never its address); everything
    outside the two slices bit-unchanged.  MI355X: worst error / bar 0.047."""
    for kind in KINDS:
        x, terms, _ = ro.colsum_data(kind, 2, seg, C, C, tag="pair")
        xd = dev(x)
        buf, out0, out1 = _pair_buffer(C)
        ops.call("mulan_colsum_pair", xd.data_ptr(), out0.data_ptr(), out1.data_ptr(), seg, C, ops.stream())
        assert is_poison(buf[:GUARD]) and is_poison(buf[GUARD + C:2 * GUARD + C]) and is_poison(buf[2 * GUARD + 2 * C:])
        got = np.stack([host(out0), host(out1)])
        ref = terms.sum(axis=1)
        if kind == "ints":
            assert np.array_equal(got, ref)
        else:
            r = worst(np.abs(got - ref), ro.fp32_bar(terms, 1))
            print(f"colsum_pair seg {seg} C {C}: worst error / bar {r:.3g}")
            assert r <= 1.0


def test_colsum_pair_refusals(ops):
    xd = dev(np.ones((2 * 17, 8)))
    for seg, C, off1 in ((17, 6, 0), (17, 8, 1), (0, 8, 0)):               # C % 4, out1 off 16 bytes, no rows
        buf, out0, out1 = _pair_buffer(8)
        rc = raw(ops, "mulan_colsum_pair", xd.data_ptr(), out0.data_ptr(), out1.data_ptr() + 4 * off1, seg, C)
        assert rc == INVALID and is_poison(buf), (seg, C, off1)


# ====================================================================================================== 4. softmax
def _softmax_fwd(ops, x, y, rows, cols, alpha):
    if alpha == 1.0:
        return raw(ops, "mulan_softmax_fwd", x.data_ptr(), y.data_ptr(), rows, cols)
    return raw(ops, "mulan_softmax_scaled_fwd", x.data_ptr(), y.data_ptr(), rows, cols, alpha)


@pytest.mark.parametrize("cols", ro.SOFTMAX_COLS)
def test_softmax_forward(ops, cols):
    """rows in {1, 3} x alpha in {1 (plain entry point), 1/sqrt(128), 1/sqrt(256)} x {normal, peak, equal, spread}
    against float64 per row at the twin bar; rows sum to 1 within cols 2^-24; the guard row behind the last row and the
    in-place call (y == x) are held bit for bit.
    MI355X: worst device error / bar 0.59 (normal rows: twin error up to 1.0e-7, device 1.4e-7; 'spread' rows, where the
    fp32 product alpha x carries the error: twin 7.9e-6, device 8.0e-6; 'equal' rows: both 2.3e-10; 'peak': both 1.3e-40)."""
    top = 0.0
    for rows, alpha, kind in ro.softmax_cases(cols):
        a = float(np.float32(alpha))
        x, _ = ro.softmax_rows(kind, rows, cols, alpha)
        ref = ro.softmax_ref(x, a)
        terr, bar = ro.twin_bar(ro.softmax_twin(x, a), ref)
        xd = dev(x)
        y = poisoned(rows + 1, cols)
        assert _softmax_fwd(ops, xd, y, rows, cols, a) == 0
        assert is_poison(y[rows])
        got = host(y[:rows])
        derr = np.abs(got - ref).max(axis=1)
        r = worst(derr, bar)
        top = max(top, r)
        print(f"softmax fwd cols {cols} rows {rows} alpha {a:.4g} {kind}: twin {terr.max():.3g} bar {bar.max():.3g} "
              f"device {derr.max():.3g} ratio {r:.3g}")
        assert r <= 1.0
        assert (np.abs(got.sum(axis=1) - 1.0) <= cols * ro.U).all()
        if kind == "peak":
            assert (np.sort(got, axis=1)[:, -2] <= bar).all() and (got.max(axis=1) >= 1.0 - bar).all()   # one-hot to the bar
        inplace = poisoned(rows + 1, cols)
        inplace[:rows].copy_(xd)
        assert _softmax_fwd(ops, inplace, inplace, rows, cols, a) == 0
        assert np.array_equal(bits(inplace), bits(y))
    print(f"softmax fwd cols {cols}: worst device error / bar {top:.3g}")


@pytest.mark.parametrize("cols", ro.SOFTMAX_COLS)
def test_softmax_backward(ops, cols):
    """ds against the float64 gradient of sum(softmax(alpha x) dp) with respect to x, at the twin bar (the twin reads the
    same fp32 probabilities); rowmax[r] bit-equal to max |ds[r]| as written; rowmax = NULL and, at alpha = 1, the plain
    entry point give the same ds bits; guard rows bit-unchanged.
    MI355X: worst device error / bar 0.39 (normal rows: twin error up to 6.9e-8, device 5.9e-8; 'equal' rows both 1.6e-8;
    'peak' rows both 3.4e-42: p rounds to one-hot and ds at the peak is 0 where float64 has ~1e-41)."""
    top = 0.0
    for rows, alpha, kind in ro.softmax_cases(cols):
        a = float(np.float32(alpha))
        x, dp = ro.softmax_rows(kind, rows, cols, alpha)
        p32 = ro.f32(ro.softmax_ref(x, a))
        ref = ro.softmax_bwd_ref(x, dp, a)
        terr, bar = ro.twin_bar(ro.softmax_bwd_twin(p32, dp, a), ref)
        pd, dd = dev(p32), dev(dp)
        ds, rowmax = poisoned(rows + 1, cols), poisoned(rows + 1)
        assert raw(ops, "mulan_softmax_scaled_bwd", pd.data_ptr(), dd.data_ptr(), ds.data_ptr(), rows, cols, a,
                   rowmax.data_ptr()) == 0
        assert is_poison(ds[rows]) and is_poison(rowmax[rows:])
        got = host(ds[:rows])
        derr = np.abs(got - ref).max(axis=1)
        r = worst(derr, bar)
        top = max(top, r)
        print(f"softmax bwd cols {cols} rows {rows} alpha {a:.4g} {kind}: twin {terr.max():.3g} bar {bar.max():.3g} "
              f"device {derr.max():.3g} ratio {r:.3g}")
        assert r <= 1.0
        want_max = np.abs(ds[:rows].cpu().numpy()).max(axis=1)
        assert np.array_equal(want_max.view(np.uint32), rowmax[:rows].cpu().numpy().view(np.uint32))
        ds2 = poisoned(rows + 1, cols)
        assert raw(ops, "mulan_softmax_scaled_bwd", pd.data_ptr(), dd.data_ptr(), ds2.data_ptr(), rows, cols, a, None) == 0
        assert np.array_equal(bits(ds2), bits(ds))
        if alpha == 1.0:
            ds3 = poisoned(rows + 1, cols)
            assert raw(ops, "mulan_softmax_bwd", pd.data_ptr(), dd.data_ptr(), ds3.data_ptr(), rows, cols) == 0
            assert np.array_equal(bits(ds3), bits(ds))
    print(f"softmax bwd cols {cols}: worst device error / bar {top:.3g}")


@pytest.mark.parametrize("rows,cols", [(2, 6), (2, 4100), (0, 8)])
def test_softmax_refusals(ops, rows, cols):
    n = 2 * max(cols, 8)
    x, dp = dev(np.ones(n)), dev(np.ones(n))
    y, rm = poisoned(n), poisoned(4)
    xp, dpp, yp = x.data_ptr(), dp.data_ptr(), y.data_ptr()
    assert raw(ops, "mulan_softmax_fwd", xp, yp, rows, cols) == INVALID
    assert raw(ops, "mulan_softmax_scaled_fwd", xp, yp, rows, cols, 0.5) == INVALID
    assert raw(ops, "mulan_softmax_bwd", xp, dpp, yp, rows, cols) == INVALID
    assert raw(ops, "mulan_softmax_scaled_bwd", xp, dpp, yp, rows, cols, 0.5, rm.data_ptr()) == INVALID
    assert is_poison(y) and is_poison(rm)


# ====================================================================================================== 5. mulan_absmax_rows
def _absmax(ops, xd, rows, row_len):
    out = torch.full((rows * ro.PARTS + GUARD,), POISON, dtype=torch.int32, device="cuda")
    ops.call("mulan_absmax_rows", xd.data_ptr(), out.data_ptr(), rows, row_len, ops.stream())
    got = out.cpu().numpy()
    assert (got[rows * ro.PARTS:] == POISON).all()
    return got[:rows * ro.PARTS].view(np.uint32).reshape(rows, ro.PARTS)


def _check_maxima(got, x):
    """every one of the 16 parts is the maximum of the float4s its block owns; their maximum is the row's"""
    assert np.array_equal(got, ro.absmax_parts(x))
    row_max = (np.ascontiguousarray(x, dtype=np.float32).view(np.uint32) & np.uint32(0x7fffffff)).max(axis=1)
    assert np.array_equal(got.max(axis=1), row_max) and (got <= row_max[:, None]).all()


@pytest.mark.parametrize("row_len", ro.ABSMAX_ROW_LENS)
def test_absmax_rows_planted_maximum(ops, row_len):
    """rows in {1, 3}; the maximum (+4 or -4 among values in (-1, 1)) at the first element, the last, in the last float4
    of the 4 x unrolled loop and in the first of the remainder loop (where the row has them: 12288 float4 never enter
    the unrolled loop, 12289 enter it once): the 16 parts bit-equal to the maxima of the float4s each block owns"""
    places = ro.absmax_plants(row_len)
    for rows in ro.ABSMAX_ROWS:
        base = ro.f32(ro.rng_of("absmax", rows, row_len).uniform(-1.0, 1.0, (rows, row_len)))
        bd = dev(base)
        for name, idx in places.items():
            for v in (4.0, -4.0):
                x, xd = base.copy(), bd.clone()
                x[rows - 1, idx] = v
                xd[rows - 1, idx] = v
                got = _absmax(ops, xd, rows, row_len)
                _check_maxima(got, x)
                assert got.max(axis=1)[rows - 1] == np.float32(4.0).view(np.uint32), (rows, name, v)
    print(f"absmax_rows row_len {row_len}: maximum planted at {places}")


@pytest.mark.parametrize("row_len", (1020, 65548))
def test_absmax_rows_special_values(ops, row_len):
    """a row of -0.0 gives 0; a row of denormals (+-1e-42) gives their exact bits, not a flushed zero; +inf is a maximum"""
    rng = ro.rng_of("absmax special", row_len)
    x = np.zeros((3, row_len), np.float32)
    x[0] = -0.0
    x[1] = np.float32(1e-42) * np.where(rng.random(row_len) < 0.5, -1, 1).astype(np.float32)
    x[2] = rng.uniform(-1.0, 1.0, row_len).astype(np.float32)
    x[2, row_len - 3] = np.inf
    assert np.signbit(x[0]).all() and 0 < np.float32(1e-42) < np.finfo(np.float32).tiny
    got = _absmax(ops, torch.from_numpy(x).cuda(), 3, row_len)
    _check_maxima(got, x)
    assert (got[0] == 0).all()
    assert got[1].max() == np.float32(1e-42).view(np.uint32) and got[2].max() == 0x7F800000


@pytest.mark.parametrize("rows,row_len", [(2, 6), (0, 8)])
def test_absmax_rows_refusals(ops, rows, row_len):
    x, out = dev(np.ones(64)), poisoned(64)
    assert raw(ops, "mulan_absmax_rows", x.data_ptr(), out.data_ptr(), rows, row_len) == INVALID
    assert is_poison(out)


# ====================================================================================================== 6. add + maxima
def _run_add(ops, a, b, rows, row_len, alias, ncols=None):
    """-> (c bits [rows, row_len] as float32, maxima [rows, 16] uint32, colpart [rows, 16, ncols] float64 or None)"""
    ad, bd = dev(a), dev(b)
    cbuf = poisoned(rows * row_len + GUARD)
    cd = {"none": cbuf[:rows * row_len], "a": ad.view(-1), "b": bd.view(-1)}[alias]
    out = torch.full((rows * ro.PARTS + GUARD,), POISON, dtype=torch.int32, device="cuda")
    if ncols is None:
        part = None
        ops.call("mulan_add_absmax_rows", ad.data_ptr(), bd.data_ptr(), cd.data_ptr(), out.data_ptr(), rows, row_len,
                 ops.stream())
    else:
        part = poisoned(rows * ro.PARTS * ncols + GUARD)
        ops.call("mulan_add_absmax_rows_colsum", ad.data_ptr(), bd.data_ptr(), cd.data_ptr(), out.data_ptr(),
                 part.data_ptr(), rows, row_len, ncols, ops.stream())
        assert is_poison(part[rows * ro.PARTS * ncols:])
        part = host(part[:rows * ro.PARTS * ncols]).reshape(rows, ro.PARTS, ncols)
    assert is_poison(cbuf[rows * row_len:]) and (alias == "none" or is_poison(cbuf))
    m = out.cpu().numpy()
    assert (m[rows * ro.PARTS:] == POISON).all()
    return (cd.cpu().numpy().reshape(rows, row_len), m[:rows * ro.PARTS].view(np.uint32).reshape(rows, ro.PARTS), part)


@pytest.mark.parametrize("rows,row_len", ro.ADD_TABLE)
def test_add_absmax_rows(ops, rows, row_len):
    """c bit-equal to the fp32 sum, out of place and with c aliasing a or b; the maxima bit-equal to
    mulan_absmax_rows(c) and to the oracle's parts"""
    for kind in KINDS:
        a, b, c = ro.add_data(kind, rows, row_len)
        c32 = c.astype(np.float32)
        for alias in ("none", "a", "b"):
            got_c, got_m, _ = _run_add(ops, a, b, rows, row_len, alias)
            assert np.array_equal(got_c.view(np.uint32), c32.view(np.uint32)), (kind, alias)
            assert np.array_equal(got_m, _absmax(ops, dev(c), rows, row_len)), (kind, alias)
            _check_maxima(got_m, c)


@pytest.mark.parametrize("ncols,row_len,rows", ro.ADD_COLSUM_TABLE)
def test_add_absmax_rows_colsum(ops, ncols, row_len, rows):
    """ncols = 4 (one column quad: thread 0 sums all 256 partials) to 1024 (256 quads: no partial to add); rows shorter
    than one pass: the blocks without data write zeros to their maxima and partials, not the poison they found.  c and
    the maxima as above; the 16 partials of an image, summed in float64, are its column sums: exact on integers, within
    the fp32 bound with n = row_len / ncols on cancelling floats.  MI355X: worst error / bar 0.10."""
    n = row_len // ncols
    empty = [p for p in range(ro.PARTS) if p * 256 >= row_len // 4]
    for kind in KINDS:
        a, b, c = ro.add_data(kind, rows, row_len, ncols)
        terms = c.reshape(rows, n, ncols)
        for alias in ("none", "a"):
            got_c, got_m, part = _run_add(ops, a, b, rows, row_len, alias, ncols)
            assert np.array_equal(got_c.view(np.uint32), c.astype(np.float32).view(np.uint32)), (kind, alias)
            _check_maxima(got_m, c)
            assert (got_m[:, empty] == 0).all() and (part[:, empty] == 0).all()
            got, ref = part.sum(axis=1), terms.sum(axis=1)
            if kind == "ints":
                assert np.array_equal(got, ref), alias
            else:
                r = worst(np.abs(got - ref), ro.fp32_bar(terms, 1))
                print(f"add_absmax_rows_colsum ncols {ncols} row_len {row_len} rows {rows} c={alias}: error / bar {r:.3g}")
                assert r <= 1.0


@pytest.mark.parametrize("row_len,ncols,null_part", [(48, 6, False), (48, 12, False), (20, 8, False), (16, 8, True)])
def test_add_absmax_rows_colsum_refusals(ops, row_len, ncols, null_part):
    """ncols % 4; ncols / 4 = 3 does not divide 256; row_len % ncols; no colpart"""
    a, b = dev(np.ones((2, row_len))), dev(np.ones((2, row_len)))
    c, out, part = poisoned(2 * row_len), poisoned(2 * ro.PARTS), poisoned(2 * ro.PARTS * 16)
    rc = raw(ops, "mulan_add_absmax_rows_colsum", a.data_ptr(), b.data_ptr(), c.data_ptr(), out.data_ptr(),
             None if null_part else part.data_ptr(), 2, row_len, ncols)
    assert rc == INVALID and is_poison(c) and is_poison(out) and is_poison(part)


# ====================================================================================================== 7. rows per wave
@pytest.mark.parametrize("rows,cols", ro.ROWMEAN_TABLE)
def test_rowmean(ops, rows, cols):
    """rows in {1, 4, 5}: a full block of four waves, one wave, one wave past a block; cols around the 64 lanes.
    Integers: bit-equal to fp32(sum) / fp32(cols); floats: the fp32 bound over cols.  MI355X: worst error / bar 0.006."""
    for kind in KINDS:
        x = ro.rowmean_data(kind, rows, cols)
        xd, out = dev(x), poisoned(rows + GUARD)
        ops.call("mulan_rowmean", xd.data_ptr(), out.data_ptr(), rows, cols, ops.stream())
        assert is_poison(out[rows:])
        got = out[:rows].cpu().numpy()
        if kind == "ints":
            want = x.sum(axis=1).astype(np.float32) / np.float32(cols)
            assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
        else:
            r = worst(np.abs(got.astype(np.float64) - x.mean(axis=1)), ro.fp32_bar(x, 1) / cols)
            print(f"rowmean rows {rows} cols {cols}: worst error / bar {r:.3g}")
            assert r <= 1.0


@pytest.mark.parametrize("B,C", ro.DELTA_TABLE)
def test_attention_delta(ops, B, C):
    """delta[b, s] = sum_c dout * o per row; the images 2^12 apart in scale and every row judged against its own
    sum |dout o| (n = C products).  MI355X: worst error / bar 0.003."""
    for kind in KINDS:
        dout, o = ro.delta_data(kind, B, C)
        dd, od, out = dev(dout), dev(o), poisoned(B * ro.DELTA_S + GUARD)
        ops.call("mulan_attention_delta", dd.data_ptr(), od.data_ptr(), out.data_ptr(), B, ro.DELTA_S, C, ops.stream())
        assert is_poison(out[B * ro.DELTA_S:])
        got = host(out[:B * ro.DELTA_S]).reshape(B, ro.DELTA_S)
        terms = dout * o
        if kind == "ints":
            assert np.array_equal(got, terms.sum(axis=2))
        else:
            r = worst(np.abs(got - terms.sum(axis=2)), ro.fp32_bar(terms, 2))
            print(f"attention_delta B {B} C {C}: worst error / bar {r:.3g}")
            assert r <= 1.0


@pytest.mark.parametrize("n,E,ld_extra,col0", ro.TEMB_TABLE)
def test_temb(ops, n, E, ld_extra, col0):
    """forward and backward at ld = E + ld_extra, column offset col0, against the float64 formula (nlw and 1000 t rounded
    to fp32 as in the kernel) at the twin bar over the case; the columns of out outside [col0, col0 + E) bit-unchanged.
    ld = E with col0 = 8 does not fit (a row would end in the next one -- accepted before this test existed): both entry
    points refuse it and write nothing.
    MI355X: forward twin error 4.0e-8 (E = 4) .. 8.8e-5 (E = 512: the fp32 product k nlw carries it), device 4.0e-8 ..
    4.6e-5, device / bar at most 0.25; backward twin error 2.1e-4 (E = 4) .. 0.12 (E = 512), device 2.1e-4 .. 0.069,
    device / bar at most 0.68."""
    ld = E + ld_extra
    t, dout = ro.temb_data(n, E)
    td = dev(t)
    out, dt = poisoned(n * ld + GUARD), poisoned(n + GUARD)
    wide = np.full((n, ld), np.nan)
    if ro.temb_fits(E, ld, col0):
        wide[:, col0:col0 + E] = dout
    dd = dev(wide)
    rc_f = raw(ops, "mulan_temb_fwd", td.data_ptr(), out.data_ptr(), n, E, ld, col0)
    rc_b = raw(ops, "mulan_temb_bwd", td.data_ptr(), dd.data_ptr(), dt.data_ptr(), n, E, ld, col0)
    if not ro.temb_fits(E, ld, col0):
        assert rc_f == INVALID and rc_b == INVALID and is_poison(out) and is_poison(dt)
        return
    assert rc_f == 0 and rc_b == 0
    rows = out[:n * ld].view(n, ld)
    assert is_poison(out[n * ld:]) and is_poison(rows[:, :col0]) and is_poison(rows[:, col0 + E:]) and is_poison(dt[n:])
    ref = ro.temb_fwd(t, E)
    terr, bar = ro.twin_bar(ro.temb_fwd(t, E, ro.F32), ref, axis=None)
    derr = np.abs(host(rows[:, col0:col0 + E]) - ref).max()
    print(f"temb fwd n {n} E {E} ld {ld} col0 {col0}: twin {terr:.3g} bar {bar:.3g} device {derr:.3g} ratio {derr / bar:.3g}")
    assert derr <= bar
    ref = ro.temb_bwd(t, dout, E)
    terr, bar = ro.twin_bar(ro.temb_bwd(t, dout, E, ro.F32), ref, axis=None)
    derr = np.abs(host(dt[:n]) - ref).max()
    print(f"temb bwd n {n} E {E} ld {ld} col0 {col0}: twin {terr:.3g} bar {bar:.3g} device {derr:.3g} ratio {derr / bar:.3g}")
    assert derr <= bar
