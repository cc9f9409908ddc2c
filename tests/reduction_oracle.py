"""Data, float64 references and bars for the reduction kernels off the model's shapes: the column sums
(colsum_kernel, colsum_vec_kernel behind mulan_colsum / mulan_colsum_pair / ops.colsum_raw), the row softmax, the
per-row maxima (mulan_absmax_rows, mulan_add_absmax_rows[_colsum]) and the one-row-per-wave kernels (mulan_rowmean,
mulan_attention_delta, mulan_temb_fwd / _bwd).  numpy only, no device: tests/test_gpu_reductions.py runs the kernels
against it, tests/test_reduction_oracle.py holds its own claims.

Every input is fp32-valued: drawn in float64, rounded to float32, widened again (f32), so a float64 reference starts from
the very numbers a kernel reads.  Every reduction gets two kinds of data:

  ints      small integers in [-2, 3): every fp32 partial sum is exact, so the result is bit-equal to the exact sum and a
            dropped, doubled or misplaced term shows at any shape.
  floats    the terms of one output are standard normal, shifted so that |sum| ~ 1e-5 sum |x| (the bias sums of the
            conv_out layers, see colsum_kernel); the bars below are derived, not tuned.

The bars (u = 2^-24, the unit roundoff of fp32):

  fp32_bar      |got - ref| <= (n + 2) u sum |terms|.  A sum of n terms in fp32, in ANY order, sends every term through
                at most n - 1 additions, each with relative error <= u: the error is at most ((1 + u)^(n-1) - 1) sum |terms|
                (Higham, Accuracy and Stability, 4.2), which is below (n + 2) u sum |terms| for every n used here (n u < 1e-3).
                The two spare roundings pay for a product in front (attention_delta: at most one rounding per product)
                or a division behind (rowmean), and for an old value that is one more term (accumulate).
  f64_bar       |got - ref| <= u |ref| + seg 2^-52 sum |x|  (+ u |old + ref| with accumulate).  colsum_kernel adds in
                float64: seg - 1 additions with relative error 2^-53 each cost at most seg 2^-53 sum |x|, doubled for
                slack, and the one rounding to fp32 at the end costs u |ref|.  On the cancelling data u |ref| is 1e-5 of
                u sum |x|, so an fp32 accumulation misses this bar by orders of magnitude (test_reduction_oracle.py).
  two_stage_bar ops.colsum_raw reduces seg >= 2048 (seg % 512 == 0) in two launches with fp32 partials of 512 rows in
                between.  Through colsum_kernel each partial is rounded once (u |partial_j|), then summed in float64 and
                rounded once more: |got - ref| <= u (|ref| + sum_j |partial_j|) + 2 seg 2^-52 sum |x|.

Softmax and the timestep embedding go through expf / sinf / cosf and have no such bound: their bar is measured in the
test from an fp32 numpy twin of the same formula on the same inputs (twin_bar): 4 x the twin's worst error against
float64, at least 4 ulp of the row's largest reference value."""
import math
import zlib
from collections import namedtuple

import numpy as np

U = 2.0 ** -24
F32 = np.float32


def f32(a):
    """the float32 rounding of a, as float64"""
    return np.asarray(a, dtype=np.float64).astype(np.float32).astype(np.float64)


def seed_of(*key):
    return zlib.crc32(repr(key).encode())


def rng_of(*key):
    return np.random.default_rng(seed_of(*key))


# ------------------------------------------------------------------------------------------------------ data
INT_LO, INT_HI = -2, 3


def ints(rng, shape, lo=INT_LO, hi=INT_HI):
    return rng.integers(lo, hi, size=shape).astype(np.float64)


CANCEL = 1e-5


def cancelling(rng, shape, axis):
    """standard normal terms along `axis`, shifted so that the sum over `axis` is CANCEL x the sum of the magnitudes
    (one term cannot cancel: it stays as drawn)"""
    x = rng.standard_normal(shape)
    n = shape[axis]
    if n > 1:
        x = x - x.mean(axis=axis, keepdims=True)
        x = x + CANCEL * np.abs(x).sum(axis=axis, keepdims=True) / n
    return f32(x)


def draw(kind, rng, shape, axis):
    return ints(rng, shape) if kind == "ints" else cancelling(rng, shape, axis)


# ------------------------------------------------------------------------------------------------------ bars
def fp32_bar(terms, axis, n=None):
    """(n + 2) u sum |terms| over `axis`; n defaults to the number of terms"""
    n = terms.shape[axis] if n is None else n
    return (n + 2) * U * np.abs(terms).sum(axis=axis)


def f64_bar(ref, seg, sabs, total=None):
    """ref: the float64 column sum, sabs: sum |x|; total = old + ref with accumulate"""
    bar = U * np.abs(ref) + seg * 2.0 ** -52 * sabs
    return bar if total is None else bar + U * np.abs(total)


def two_stage_bar(terms, chunk=512):
    """terms [nseg, seg, C] with seg % chunk == 0, reduced over axis 1"""
    nseg, seg, C = terms.shape
    parts = terms.reshape(nseg, seg // chunk, chunk, C).sum(axis=2)
    return U * (np.abs(terms.sum(axis=1)) + np.abs(parts).sum(axis=1)) + 2 * seg * 2.0 ** -52 * np.abs(terms).sum(axis=1)


def sum32_sequential(terms, axis):
    """fp32 accumulation, one term after the other"""
    t = np.moveaxis(np.asarray(terms), axis, 0).astype(np.float32)
    acc = np.zeros(t.shape[1:], np.float32)
    for row in t:
        acc = acc + row
    return acc.astype(np.float64)


def sum32_numpy(terms, axis):
    """np.sum in float32 along a contiguous axis (numpy's pairwise order)"""
    t = np.ascontiguousarray(np.moveaxis(np.asarray(terms), axis, -1).astype(np.float32))
    return np.sum(t, axis=-1, dtype=np.float32).astype(np.float64)


def ulp32(v):
    """the spacing of float32 at |v|"""
    return np.spacing(np.abs(np.asarray(v, dtype=np.float64)).astype(np.float32)).astype(np.float64)


def twin_bar(twin, ref, axis=-1):
    """(twin's worst |twin - ref| along axis, the bar: 4 x that, at least 4 ulp of the largest |ref| along axis)"""
    err = np.abs(np.asarray(twin, dtype=np.float64) - ref).max(axis=axis)
    return err, np.maximum(4.0 * err, 4.0 * ulp32(np.abs(ref).max(axis=axis)))


# ------------------------------------------------------------------------------------------------------ 1. mulan_colsum
# x_off / out_off: the operand starts that many floats into a 16-byte aligned buffer
ColsumCfg = namedtuple("ColsumCfg", "kernel C ld x_off out_off")
SCALAR_CFGS = [ColsumCfg("scalar", 1, 1, 0, 0), ColsumCfg("scalar", 3, 3, 0, 0), ColsumCfg("scalar", 5, 5, 0, 0),
               ColsumCfg("scalar", 130, 130, 0, 0), ColsumCfg("scalar", 3, 7, 0, 0), ColsumCfg("scalar", 64, 65, 0, 0),
               ColsumCfg("scalar", 64, 64, 1, 0), ColsumCfg("scalar", 64, 64, 0, 1)]
VECTOR_CFGS = [ColsumCfg("vector", 4, 4, 0, 0), ColsumCfg("vector", 60, 60, 0, 0), ColsumCfg("vector", 64, 64, 0, 0),
               ColsumCfg("vector", 68, 68, 0, 0), ColsumCfg("vector", 132, 132, 0, 0), ColsumCfg("vector", 256, 256, 0, 0),
               ColsumCfg("vector", 68, 72, 0, 0)]
COLSUM_SEGS = (1, 2, 15, 16, 17, 127, 128, 129, 300)      # across the vector kernel's 16-lane and 8 x 16 unrolled steps
COLSUM_NSEG = (1, 3)


def _colsum_table():
    """every configuration at seg 17 and 129, every other seg with one configuration per kernel (walking through them)"""
    table = [(cfg, seg) for cfg in SCALAR_CFGS + VECTOR_CFGS for seg in (17, 129)]
    rest = [s for s in COLSUM_SEGS if s not in (17, 129)]
    for cfgs in (SCALAR_CFGS, VECTOR_CFGS):
        table += [(cfgs[(3 * i + 1) % len(cfgs)], seg) for i, seg in enumerate(rest)]
    return table


COLSUM_TABLE = _colsum_table()


def colsum_vec_dispatch(C, ld, x_ptr, out_ptr):
    """mulan_colsum's own condition for the float4 kernel"""
    return C % 4 == 0 and ld % 4 == 0 and x_ptr % 16 == 0 and out_ptr % 16 == 0


def colsum_data(kind, nseg, seg, C, ld, tag="colsum"):
    """(x [nseg * seg, ld] with NaN in the padding columns, terms [nseg, seg, C], old [nseg, C])"""
    rng = rng_of(tag, kind, nseg, seg, C, ld)
    terms = draw(kind, rng, (nseg, seg, C), 1)
    old = ints(rng, (nseg, C)) if kind == "ints" else f32(rng.standard_normal((nseg, C)))
    x = np.full((nseg * seg, ld), np.nan)
    x[:, :C] = terms.reshape(nseg * seg, C)
    return x, terms, old


# ------------------------------------------------------------------------------------------------------ 2. ops.colsum_raw
RAW_SEGS = (2048, 2560, 2047)            # two stages (seg >= 2048, seg % 512 == 0) twice, one stage
RAW_NSEG = 2
RAW_TABLE = [(seg, C, ld) for seg in RAW_SEGS for C in (3, 132) for ld in (C, C + 4)]


def raw_two_stage(seg):
    return seg >= 2048 and seg % 512 == 0


# ------------------------------------------------------------------------------------------------------ 3. mulan_colsum_pair
PAIR_TABLE = [(seg, C) for seg in (1, 17, 129) for C in (4, 68, 256)]


# ------------------------------------------------------------------------------------------------------ 4. softmax
SOFTMAX_COLS = (4, 8, 252, 1024, 1028, 2052, 4092, 4096)
SOFTMAX_ROWS = (1, 3)
SOFTMAX_ALPHAS = (1.0, 1.0 / math.sqrt(128.0), 1.0 / math.sqrt(256.0))       # 1.0: the plain entry points
SOFTMAX_KINDS = ("normal", "peak", "equal", "spread")                        # spread under alpha = 1 / sqrt(128) only


def softmax_cases(cols):
    return [(rows, a, kind) for rows in SOFTMAX_ROWS for a in SOFTMAX_ALPHAS for kind in SOFTMAX_KINDS
            if kind != "spread" or a == SOFTMAX_ALPHAS[1]]


def softmax_rows(kind, rows, cols, alpha):
    """normal: N(0, 4^2); peak: one logit 80 (in units of alpha x) above the largest of the rest; equal: one value;
    spread: uniform over [0, 1e4)"""
    rng = rng_of("softmax", kind, rows, cols, alpha)
    if kind == "normal":
        x = 4.0 * rng.standard_normal((rows, cols))
    elif kind == "peak":
        x = rng.standard_normal((rows, cols))
        k = rng.integers(0, cols, size=rows)
        x[np.arange(rows), k] = x.max(axis=1) + 80.0 / alpha
    elif kind == "equal":
        x = np.full((rows, cols), 1.5)
    else:
        x = 1e4 * rng.random((rows, cols))
    return f32(x), f32(rng.standard_normal((rows, cols)))        # logits, dp


def softmax_ref(x, alpha):
    """float64 softmax(alpha x) over the last axis; alpha is the fp32-valued scalar the kernel receives"""
    v = alpha * np.asarray(x, dtype=np.float64)
    e = np.exp(v - v.max(axis=-1, keepdims=True))
    return e / e.sum(axis=-1, keepdims=True)


def softmax_twin(x, alpha):
    """the kernel's formula in fp32 numpy"""
    v = x.astype(F32) * F32(alpha)
    e = np.exp(v - v.max(axis=-1, keepdims=True))
    inv = F32(1.0) / e.sum(axis=-1, keepdims=True, dtype=F32)
    return e * inv


def softmax_bwd_ref(x, dp, alpha):
    """d/dx of sum(softmax(alpha x) * dp): alpha p (dp - sum p dp), float64 from the exact p"""
    p = softmax_ref(x, alpha)
    return alpha * p * (dp - (p * dp).sum(axis=-1, keepdims=True))


def softmax_bwd_twin(p32, dp, alpha):
    """the kernel's formula in fp32 numpy on the fp32 probabilities it reads"""
    p, d = p32.astype(F32), dp.astype(F32)
    dot = (p * d).sum(axis=-1, keepdims=True, dtype=F32)
    return F32(alpha) * (p * (d - dot))


# ------------------------------------------------------------------------------------------------------ 5. mulan_absmax_rows
PARTS = 16
ABSMAX_STRIDE4 = PARTS * 256                               # float4s per pass of a row's 16 blocks
ABSMAX_ROW_LENS = (4, 1020, 16384, 16388, 49152, 49156, 65548, 81928)
ABSMAX_ROWS = (1, 3)


def absmax_loops(row_len):
    """which float4 of a row the 4 x unrolled loop of absmax_rows_kernel takes and which its remainder loop:
    (unrolled [row_len / 4] bool, remainder [row_len / 4] bool), from the loop conditions as written"""
    n4 = row_len // 4
    unrolled = np.zeros(n4, bool)
    for i0 in range(min(ABSMAX_STRIDE4, n4)):
        i = i0
        while i + 3 * ABSMAX_STRIDE4 < n4:
            unrolled[[i, i + ABSMAX_STRIDE4, i + 2 * ABSMAX_STRIDE4, i + 3 * ABSMAX_STRIDE4]] = True
            i += 4 * ABSMAX_STRIDE4
    return unrolled, ~unrolled


def absmax_plants(row_len):
    """name -> element index of the places a maximum is planted at"""
    unrolled, rest = absmax_loops(row_len)
    places = {"first": 0, "last": row_len - 1}
    if unrolled.any():
        places["last_unrolled"] = 4 * int(np.flatnonzero(unrolled).max()) + 2
    if unrolled.any() and rest.any():
        places["first_remainder"] = 4 * int(np.flatnonzero(rest).min()) + 1
    return places


def absmax_parts(x):
    """x [rows, row_len] -> [rows, 16] uint32: bits of the maximum |x| of the float4s each of the 16 blocks owns"""
    rows, row_len = x.shape
    bits = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32) & np.uint32(0x7fffffff)
    owner = (np.arange(row_len // 4) % ABSMAX_STRIDE4) // 256
    out = np.zeros((rows, PARTS), np.uint32)
    for p in range(PARTS):
        sel = np.repeat(owner == p, 4)
        if sel.any():
            out[:, p] = bits[:, sel].max(axis=1)
    return out


# ------------------------------------------------------------------------------------------------------ 6. add + maxima
ADD_TABLE = [(rows, row_len) for rows in (1, 3) for row_len in (4, 1020, 16388, 49156)]
ADD_COLSUM_NCOLS = (4, 8, 64, 1024)


def add_colsum_row_lens(ncols):
    return (ncols, 5 * ncols, (16384 // ncols + 1) * ncols)


ADD_COLSUM_TABLE = [(ncols, row_len, rows) for ncols in ADD_COLSUM_NCOLS for row_len in add_colsum_row_lens(ncols)
                    for rows in (1, 3)]


def add_data(kind, rows, row_len, ncols=None):
    """(a, b, c = fl32(a + b)) [rows, row_len]; with ncols the rows of c, seen as [row_len / ncols, ncols], cancel
    down their columns"""
    rng = rng_of("add", kind, rows, row_len, ncols)
    if kind == "ints":
        a, b = ints(rng, (rows, row_len)), ints(rng, (rows, row_len))
    else:
        b = f32(rng.standard_normal((rows, row_len)))
        want = (cancelling(rng, (rows, row_len // ncols, ncols), 1).reshape(rows, row_len) if ncols
                else rng.standard_normal((rows, row_len)))
        a = f32(want - b)
    c = (a.astype(F32) + b.astype(F32)).astype(np.float64)
    return a, b, c


# ------------------------------------------------------------------------------------------------------ 7. rows per wave
ROWMEAN_TABLE = [(rows, cols) for rows in (1, 4, 5) for cols in (1, 63, 64, 65, 3072)]
DELTA_TABLE = [(B, C) for B in (1, 3) for C in (128, 256)]
DELTA_S = 1024


def rowmean_data(kind, rows, cols):
    return draw(kind, rng_of("rowmean", kind, rows, cols), (rows, cols), 1)


def delta_data(kind, B, C):
    """(dout, o) [B, 1024, C]; floats: the products dout * o of a row cancel, and image b is 2^12 times image b - 1 in
    dout (one image 2^12 above the other two with B = 3)"""
    rng = rng_of("delta", kind, B, C)
    shape = (B, DELTA_S, C)
    if kind == "ints":
        return ints(rng, shape), ints(rng, shape)
    o = f32(np.where(rng.random(shape) < 0.5, -1.0, 1.0) * (0.5 + np.abs(rng.standard_normal(shape))))
    scale = (2.0 ** 12) ** (np.arange(B) % 2)
    dout = f32(cancelling(rng, shape, 2) / o * scale[:, None, None])
    return dout, o


TEMB_TABLE = [(n, E, ld_extra, col0) for n in (1, 4, 5) for E in (4, 6, 128, 130, 512) for ld_extra in (0, 8)
              for col0 in (0, 8)]


def temb_fits(E, ld, col0):
    """a row [col0, col0 + E) inside its stride; anything else the entry points refuse"""
    return col0 >= 0 and col0 + E <= ld


def temb_data(n, E):
    rng = rng_of("temb", n, E)
    return f32(rng.random(n)), f32(rng.standard_normal((n, E)))          # t in [0, 1), dout


def _temb_angles(t, E, dtype):
    half = E // 2
    nlw = F32(-math.log(10000.0) / (half - 1))                           # rounded to fp32, as the kernel states
    tv = t.astype(F32) * F32(1000.0)                                     # t * 1000 in fp32, as the kernel states
    k = np.arange(half)
    if dtype is F32:
        w = np.exp(k.astype(F32) * nlw)
        return w, tv[:, None] * w[None, :]
    w = np.exp(k.astype(np.float64) * float(nlw))
    return w, tv.astype(np.float64)[:, None] * w[None, :]


def temb_fwd(t, E, dtype=np.float64):
    """[n, E]: [sin(a), cos(a)], a = (1000 t) w_k, w_k = exp(k nlw); dtype F32 gives the twin"""
    _, a = _temb_angles(t, E, dtype)
    return np.concatenate([np.sin(a), np.cos(a)], axis=1)


def temb_bwd(t, dout, E, dtype=np.float64):
    """[n]: sum_k 1000 w_k (dsin_k cos(a) - dcos_k sin(a))"""
    w, a = _temb_angles(t, E, dtype)
    half = E // 2
    d = dout.astype(dtype)
    term = dtype(1000.0) * w[None, :] * (d[:, :half] * np.cos(a) - d[:, half:] * np.sin(a))
    return term.sum(axis=1, dtype=dtype)


# ------------------------------------------------------------------------------------------------------ all float data
def float_datasets():
    """(name, terms, axis, kernel accumulates in: "f32" | "f64") of every cancelling data set of the GPU tables"""
    for cfg, seg in COLSUM_TABLE:
        for nseg in COLSUM_NSEG:
            _, terms, _ = colsum_data("floats", nseg, seg, cfg.C, cfg.ld)
            yield f"colsum {cfg.kernel} C{cfg.C} ld{cfg.ld} seg{seg} nseg{nseg}", terms, 1, "f64" if cfg.kernel == "scalar" else "f32"
    for seg, C, ld in RAW_TABLE:
        _, terms, _ = colsum_data("floats", RAW_NSEG, seg, C, ld, tag="raw")
        yield f"colsum_raw seg{seg} C{C} ld{ld}", terms, 1, "f64" if (C % 4 and not raw_two_stage(seg)) else "f32"
    for seg, C in PAIR_TABLE:
        _, terms, _ = colsum_data("floats", 2, seg, C, C, tag="pair")
        yield f"colsum_pair seg{seg} C{C}", terms, 1, "f32"
    for ncols, row_len, rows in ADD_COLSUM_TABLE:
        c = add_data("floats", rows, row_len, ncols)[2]
        yield f"add_colsum ncols{ncols} row_len{row_len} rows{rows}", c.reshape(rows, row_len // ncols, ncols), 1, "f32"
    for rows, cols in ROWMEAN_TABLE:
        yield f"rowmean rows{rows} cols{cols}", rowmean_data("floats", rows, cols), 1, "f32"
    for B, C in DELTA_TABLE:
        dout, o = delta_data("floats", B, C)
        yield f"delta B{B} C{C}", dout * o, 2, "f32"
