"""mulan_gemm (mulan_amd/csrc/gemm.hip) through the C ABI, with every parameter of the call the test's to choose: the three
tiles (128 x 128, 128 x 32, 64 x 64) direct and under split-K, leading dimensions and batch strides that are not tight,
alpha / beta, the float4 (VEC) against the scalar loaders, and the accuracy on random data against float64.

Every call goes through run(), which
  * asserts with tests/gemm_plan.py (held against the library and the source by tests/test_gemm_plan.py) that the shape
    lands on the tile and the split count the case was written for, and on the loaders it was written for;
  * lays the operands out with NaN in every element a leading dimension or a stride skips, so a read outside the
    operand poisons the result;
  * writes C into a sentinel-filled [batch][M + gap][ldc] buffer and requires every element outside the M x N windows
    to hold the sentinel bit for bit afterwards;
  * hands split-K a NaN-filled workspace of exactly mulan_gemm_workspace bytes, so a slab element that is reduced
    without having been written shows.

CASES lists (M, N, K, batch, workspace given, tile, splits) of every call made here, for the CPU sweep."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import gemm_plan as gp
from tests.gemm_plan import T64, T128, T128x32

SENTINEL = -12345.678
TT = [(0, 0), (0, 1), (1, 0), (1, 1)]
U = 2.0 ** -24                 # unit roundoff of fp32


@pytest.fixture(scope="module")
def ops():
    from mulan_amd import ops as _ops
    _ops.lib.load()
    saved = _ops.CONV_MODE
    _ops.CONV_MODE = "f32"
    yield _ops
    _ops.CONV_MODE = saved


def ints(rng, shape, lo=-3, hi=4):
    return rng.integers(lo, hi, size=shape).astype(np.float64)


def layout(x, ld, stride, lead=0):
    """x [nb, rows, cols] -> flat fp32 buffer with element (b, r, c) at lead + b * stride + r * ld + c, NaN elsewhere"""
    nb, rows, cols = x.shape
    assert ld >= cols and (nb == 1 or stride >= (rows - 1) * ld + cols)
    buf = np.full(lead + (nb - 1) * stride + (rows - 1) * ld + cols, np.nan, dtype=np.float32)
    idx = (lead + np.arange(nb)[:, None, None] * stride + np.arange(rows)[None, :, None] * ld
           + np.arange(cols)[None, None, :])
    buf[idx] = x
    return torch.from_numpy(buf).cuda()[lead:]


def reference(A, B, bias, R, alpha, beta, batch):
    """float64: alpha * A @ B + bias + beta * R, over [batch, M, N]; A, B and R may be shared by the batch (leading 1)"""
    ref = alpha * np.matmul(A, B)
    ref = np.broadcast_to(ref, (batch,) + ref.shape[1:]).copy()
    if bias is not None:
        ref += bias
    if R is not None:
        ref += beta * R
    return ref


def run(ops, A, B, *, ta, tb, batch, expect, expect_vec=None, bias=None, R=None, alpha=1.0, beta=1.0, lda_pad=0, ldb_pad=0,
        sa_extra=0, sb_extra=0, a_lead=0, b_lead=0, ldc_pad=0, gap_rows=0, ldr_pad=0, ws=True):
    """One mulan_gemm call.  A [nbA, M, K], B [nbB, K, N], R [nbR, M, N] in mathematical layout (nb* = 1: shared by the
    batch, stride 0); returns the [batch, M, N] windows of C as a device tensor."""
    M, K, N = A.shape[1], A.shape[2], B.shape[2]
    a_st = A.transpose(0, 2, 1) if ta else A
    b_st = B.transpose(0, 2, 1) if tb else B
    lda, ldb = a_st.shape[2] + lda_pad, b_st.shape[2] + ldb_pad
    sA = 0 if (A.shape[0] == 1 and batch > 1) else a_st.shape[1] * lda + sa_extra
    sB = 0 if (B.shape[0] == 1 and batch > 1) else b_st.shape[1] * ldb + sb_extra
    a_dev, b_dev = layout(a_st, lda, sA, a_lead), layout(b_st, ldb, sB, b_lead)
    ldc, ldr = N + ldc_pad, N + ldr_pad
    sC = (M + gap_rows) * ldc
    r_dev, sR = None, 0
    if R is not None:
        sR = 0 if (R.shape[0] == 1 and batch > 1) else M * ldr
        r_dev = layout(R, ldr, sR)
    bias_dev = None if bias is None else torch.from_numpy(bias.astype(np.float32)).cuda()
    w_dev = None
    if ws:
        nbytes = ops.lib.load().mulan_gemm_workspace(M, N, K, batch)
        assert nbytes == gp.workspace_bytes(M, N, K, batch)
        if nbytes:
            w_dev = torch.full((nbytes // 4,), float("nan"), device="cuda", dtype=torch.float32)
    # the case runs on the kernel it was written for
    tile, splits, _ = gp.plan(M, N, K, batch, w_dev is not None)
    assert (tile, splits) == tuple(expect), ((M, N, K, batch), (tile, splits), expect)
    if expect_vec is not None:
        assert gp.vec(a_dev.data_ptr(), b_dev.data_ptr(), M, N, K, lda, ldb, ta, tb, sA, sB) == expect_vec
    C = torch.full((batch, M + gap_rows, ldc), SENTINEL, device="cuda", dtype=torch.float32)
    ops.call("mulan_gemm", a_dev.data_ptr(), b_dev.data_ptr(), C.data_ptr(), ops.ptr(bias_dev),
             None if r_dev is None else r_dev.data_ptr(), M, N, K, lda, ldb, ldc, ldr, int(ta), int(tb), batch, sA, sB, sC,
             sR, float(alpha), float(beta), ops.ptr(w_dev), ops.stream())
    torch.cuda.synchronize()
    out = C[:, :M, :N].clone()
    C[:, :M, :N] = SENTINEL
    untouched = torch.full_like(C, SENTINEL).view(torch.int32)
    assert torch.equal(C.view(torch.int32), untouched), "C written outside its M x N windows"
    return out


def exact(out, ref):
    got = out.cpu().double().numpy()
    if not np.array_equal(got, ref):
        bad = np.argwhere(got != ref)
        raise AssertionError("%d of %d elements differ; first (batch, m, n) %s got %r want %r; last %s" % (
            len(bad), ref.size, bad[0].tolist(), got[tuple(bad[0])], ref[tuple(bad[0])], bad[-1].tolist()))


def int_operands(seed, M, N, K, batch, nba=None, nbb=None, nbr=None):
    rng = np.random.default_rng(seed)
    nba, nbb, nbr = (batch if v is None else v for v in (nba, nbb, nbr))
    return ints(rng, (nba, M, K)), ints(rng, (nbb, K, N), -2, 3), ints(rng, (N,)), ints(rng, (nbr, M, N))


# ====================================================================================================== the cases
# (M, N, K, batch, tile)
BIG_DIRECT = [(1000, 900, 40, 4, T128),     # 8 x 8 x 4 = 256 tiles; VEC; ragged in M, N and the last k chunk
              (2050, 1930, 37, 1, T128)]    # 17 x 16 tiles; no dimension a multiple of 4: the scalar loaders
THIN_DIRECT = [(300, 32, 72, 1, T128x32), (129, 17, 33, 3, T128x32), (4100, 8, 20, 1, T128x32)]
# (M, N, K, tile, splits, transposes, lda_pad): with a workspace
SPLIT = [(128, 128, 512, T64, 8, [(0, 1), (1, 1)], 0),
         (64, 256, 500, T64, 7, TT, 0),                  # kchunk 80: the last split holds 20
         (100, 60, 509, T64, 7, TT, 1),                  # kchunk 80, last split 29; lda = contig + 1: scalar loaders
         (128, 128, 8192, T128, 16, [(0, 1)], 0),        # the big tile
         (128, 128, 4100, T128, 8, [(1, 0), (1, 1)], 0)]  # the big tile, kchunk 528, last split 404
SPLIT_PARAMS = [(M, N, K, tile, s, ta, tb, pad) for M, N, K, tile, s, tts, pad in SPLIT for ta, tb in tts]
STRIDED = [(130, 50, 178), (256, 128, 128)]              # the 64 x 64 tile, direct
# M = 130 is no multiple of 4, so under transA (m contiguous) the gate can never open: there (132, 52, 180) stands in
LOADERS = [(256, 128, 128, 1, T64), (130, 52, 180, 1, T64), (132, 52, 180, 1, T64), (1000, 900, 40, 4, T128)]
LOADER_PARAMS = [c + (ta, tb) for c in LOADERS for ta, tb in TT if not (ta and c[0] % 4)]
# (M, N, K, batch, workspace, tile, splits)
ACCURACY = [(130, 50, 178, 1, False, T64, 1), (1000, 900, 40, 4, False, T128, 1), (300, 32, 72, 1, False, T128x32, 1),
            (64, 64, 4096, 1, True, T64, 8), (128, 128, 8192, 1, True, T128, 16)]

CASES = ([(M, N, K, b, False, t, 1) for M, N, K, b, t in BIG_DIRECT + THIN_DIRECT + LOADERS]
         + [(M, N, K, max(b, 2), False, t, 1) for M, N, K, b, t in LOADERS]
         + [(M, N, K, 1, True, t, s) for M, N, K, t, s, _, _ in SPLIT]
         + [(M, N, K, 1, False, T64, 1) for M, N, K, _, _, _, _ in SPLIT]
         + [(M, N, K, b, False, T64, 1) for M, N, K in STRIDED for b in (1, 3)]
         + ACCURACY)


# ====================================================================================================== exact, on integers
@pytest.mark.parametrize("ta,tb", TT)
@pytest.mark.parametrize("M,N,K,batch,tile", BIG_DIRECT)
def test_big_tile_direct_exact(ops, M, N, K, batch, tile, ta, tb):
    """the 128 x 128 direct tile (every unfused attention product at B >= 4): its 2 x 2 fragment loop and its ragged-edge
    masks in M, N and k, on the float4 loaders (batch 4) and on the scalar ones (batch 1)"""
    A, B, bias, R = int_operands(M + N + K + 2 * ta + tb, M, N, K, batch)
    out = run(ops, A, B, ta=ta, tb=tb, batch=batch, expect=(tile, 1), expect_vec=(batch == 4), bias=bias, R=R, alpha=0.5,
              beta=-1.0)
    exact(out, reference(A, B, bias, R, 0.5, -1.0, batch))


@pytest.mark.parametrize("ta,tb", TT)
@pytest.mark.parametrize("M,N,K,batch,tile", THIN_DIRECT)
def test_thin_tile_exact(ops, M, N, K, batch, tile, ta, tb):
    """the 128 x 32 tile (N <= 32) over several blocks of M with a ragged last one, batched, and at N < 32"""
    A, B, bias, R = int_operands(M + N + K + 2 * ta + tb, M, N, K, batch)
    out = run(ops, A, B, ta=ta, tb=tb, batch=batch, expect=(tile, 1), bias=bias, R=R, alpha=0.5, beta=-1.0)
    exact(out, reference(A, B, bias, R, 0.5, -1.0, batch))


@pytest.mark.parametrize("M,N,K,tile,splits,ta,tb,pad", SPLIT_PARAMS)
def test_split_k_exact_and_reproducible(ops, M, N, K, tile, splits, ta, tb, pad):
    """split-K with transB, a ragged last split, the scalar loaders, and alpha / bias / beta * R / ldc / ldr in the reduce
    kernel, which does its own addressing; twice, for the same bits (the fixed reduction order is the contract)"""
    A, B, bias, R = int_operands(M + N + K + 2 * ta + tb, M, N, K, 1)
    kw = dict(ta=ta, tb=tb, batch=1, expect=(tile, splits), expect_vec=(pad == 0), bias=bias, R=R, alpha=2.0, beta=0.5,
              lda_pad=pad, ldc_pad=5, ldr_pad=2)
    out = run(ops, A, B, **kw)
    exact(out, reference(A, B, bias, R, 2.0, 0.5, 1))
    assert torch.equal(run(ops, A, B, **kw), out)


@pytest.mark.parametrize("M,N,K,tile,splits,ta,tb,pad", SPLIT_PARAMS)
def test_split_shapes_without_a_workspace_run_direct(ops, M, N, K, tile, splits, ta, tb, pad):
    """workspace = NULL: the same shapes on the direct path (one block walks the whole K), the same exact result"""
    A, B, bias, R = int_operands(M + N + K + 2 * ta + tb, M, N, K, 1)
    out = run(ops, A, B, ta=ta, tb=tb, batch=1, expect=(T64, 1), expect_vec=(pad == 0), bias=bias, R=R, alpha=2.0, beta=0.5,
              lda_pad=pad, ldc_pad=5, ldr_pad=2, ws=False)
    exact(out, reference(A, B, bias, R, 2.0, 0.5, 1))


# layout variants of the strided test: batch, pads of lda / ldb, which of A / B / R the batch shares
STRIDE_VARIANTS = {
    "slices": dict(batch=1, lda_pad=6, ldb_pad=10),                   # column slices of wider matrices
    "slices_vec": dict(batch=1, lda_pad=8, ldb_pad=12),               # multiples of 4: the float4 loaders stay on
    "batched_shared_r": dict(batch=3, lda_pad=6, ldb_pad=10, share="R"),
    "shared_a": dict(batch=3, lda_pad=8, ldb_pad=12, share="A"),      # the FiLM layout: one A, three B's
    "shared_b": dict(batch=3, lda_pad=6, ldb_pad=12, share="B"),
}


@pytest.mark.parametrize("ta,tb", TT)
@pytest.mark.parametrize("variant", sorted(STRIDE_VARIANTS))
@pytest.mark.parametrize("M,N,K", STRIDED)
def test_leading_dimensions_and_strides(ops, M, N, K, variant, ta, tb):
    """lda, ldb, ldc, ldr and the four batch strides as free parameters: operands that are column slices of wider
    matrices, C with ldc = N + 7 and 3 rows between batches (run() requires the columns >= N and the gap rows to keep the
    sentinel), R with ldr = N + 3, and stride 0 on A, on B and on R"""
    v = dict(STRIDE_VARIANTS[variant])
    batch, share = v.pop("batch"), v.pop("share", None)
    A, B, bias, R = int_operands(M + N + K + 2 * ta + tb + len(variant), M, N, K, batch, nba=1 if share == "A" else None,
                                 nbb=1 if share == "B" else None, nbr=1 if share == "R" else None)
    vec = v["lda_pad"] % 4 == 0 and v["ldb_pad"] % 4 == 0 and M % 4 == 0 and N % 4 == 0 and K % 4 == 0
    out = run(ops, A, B, ta=ta, tb=tb, batch=batch, expect=(T64, 1), expect_vec=vec, bias=bias, R=R, alpha=-0.25, beta=2.0,
              ldc_pad=7, gap_rows=3, ldr_pad=3, **v)
    exact(out, reference(A, B, bias, R, -0.25, 2.0, batch))


@pytest.mark.parametrize("M,N,K,ws,tile,splits", [(130, 50, 178, False, T64, 1), (128, 128, 512, True, T64, 8)])
def test_alpha_beta(ops, M, N, K, ws, tile, splits):
    """alpha x beta on the direct epilogue and on the split-K reduce kernel.  beta = 0 is left out on purpose: the kernel
    computes beta * R, so a non-finite R would reach C, and the header does not promise the BLAS rule that beta = 0
    ignores R; nothing is asserted either way."""
    A, B, bias, R = int_operands(M + N + K, M, N, K, 1)
    for alpha in (1.0, -1.0, 0.5):
        for beta in (1.0, -0.5, 2.0):
            out = run(ops, A, B, ta=0, tb=0, batch=1, expect=(tile, splits), bias=bias, R=R, alpha=alpha, beta=beta,
                      ldc_pad=1, ldr_pad=2, ws=ws)
            exact(out, reference(A, B, bias, R, alpha, beta, 1))


def test_nonpositive_sizes_are_rejected(ops):
    """M, N, K or batch <= 0: hipErrorInvalidValue (1), nothing launched, C untouched"""
    M = N = K = 64
    A = torch.ones(M * K, device="cuda")
    B = torch.ones(K * N, device="cuda")
    C = torch.full((M, N), SENTINEL, device="cuda")
    fn = ops.lib.load().mulan_gemm
    for bad in (0, -1):
        for which in range(4):
            m, n, k, batch = [bad if i == which else v for i, v in enumerate((M, N, K, 1))]
            rc = fn(A.data_ptr(), B.data_ptr(), C.data_ptr(), None, None, m, n, k, K, N, N, N, 0, 0, batch, M * K, K * N,
                    M * N, M * N, 1.0, 1.0, None, ops.stream())
            assert rc == 1, (m, n, k, batch, rc)
    torch.cuda.synchronize()
    assert torch.equal(C.view(torch.int32), torch.full_like(C, SENTINEL).view(torch.int32))


# ====================================================================================================== loaders
def float_operands(seed, M, N, K, batch, row_scale=None):
    """fp32-valued operands, held as float64 so the reference starts from the very numbers the kernel reads"""
    rng = np.random.default_rng(seed)
    A = rng.standard_normal((batch, M, K), dtype=np.float32).astype(np.float64)
    B = rng.standard_normal((batch, K, N), dtype=np.float32).astype(np.float64)
    bias = rng.standard_normal((N,), dtype=np.float32).astype(np.float64)
    R = rng.standard_normal((batch, M, N), dtype=np.float32).astype(np.float64)
    if row_scale is not None:
        s = row_scale.astype(np.float32).astype(np.float64)[None, :, None]
        A = (A * s).astype(np.float32).astype(np.float64)
        R = (R * s).astype(np.float32).astype(np.float64)
    return A, B, bias, R


@pytest.mark.parametrize("M,N,K,batch,tile,ta,tb", LOADER_PARAMS)
def test_vec_and_scalar_loaders_give_the_same_bits(ops, M, N, K, batch, tile, ta, tb):
    """the float4 loaders and the scalar ones stage the same values into the same LDS positions of one shared MFMA loop:
    switching off one condition of the gate at a time (base pointer of A, of B, lda, ldb, strideA, strideB) must not
    change a bit of the result on random data"""
    nb = max(batch, 2)
    A, B, bias, R = float_operands(M + N + K + 2 * ta + tb, M, N, K, nb)
    kw = dict(ta=ta, tb=tb, expect=(tile, 1), bias=bias, alpha=0.75, beta=-1.5)
    one = dict(batch=batch, R=R[:batch], **kw)
    base = run(ops, A[:batch], B[:batch], expect_vec=True, **one)
    for off in (dict(a_lead=1), dict(b_lead=1), dict(lda_pad=1), dict(ldb_pad=1)):
        out = run(ops, A[:batch], B[:batch], expect_vec=False, **one, **off)
        assert torch.equal(out, base), (off, int((out != base).sum()), (out != base).nonzero()[0].tolist())
    many = dict(batch=nb, R=R, **kw)
    base = base if nb == batch else run(ops, A, B, expect_vec=True, **many)
    for off in (dict(sa_extra=1), dict(sb_extra=1)):
        out = run(ops, A, B, expect_vec=False, **many, **off)
        assert torch.equal(out, base), (off, int((out != base).sum()), (out != base).nonzero()[0].tolist())


# ====================================================================================================== accuracy
def host_fp32(A, B, bias, R, alpha, beta):
    """the same product in fp32 on the host, accumulated over k in sequence, with the kernel's epilogue association
    alpha * acc + (bias + beta * R)"""
    A32, B32 = A.astype(np.float32), B.astype(np.float32)
    acc = np.zeros((A.shape[0], A.shape[1], B.shape[2]), dtype=np.float32)
    for k in range(A.shape[2]):
        acc += A32[:, :, k, None] * B32[:, k, None, :]
    add = np.float32(beta) * R.astype(np.float32)
    if bias is not None:
        add = bias.astype(np.float32) + add
    out = np.float32(alpha) * acc + add
    assert out.dtype == np.float32
    return out


@pytest.mark.parametrize("ta,tb", [(0, 1), (1, 0)])
@pytest.mark.parametrize("M,N,K,batch,ws,tile,splits,scaled", [c + (False,) for c in ACCURACY] + [ACCURACY[0] + (True,)])
def test_accuracy_against_float64(ops, M, N, K, batch, ws, tile, splits, scaled, ta, tb):
    """Random fp32 data against the float64 product of the same fp32 numbers, element by element, relative to
    mag = |alpha| |A| @ |B| + |bias| + |beta| |R|; `scaled` spreads the rows of A and R over 1e-2 .. 1e2 (no bias, so that
    the small rows are measured against their own magnitude).  Two bars, neither taken from the kernel:
      * the ceiling (K + 4) * 2^-24: the a-priori bound of an fp32 dot product of length K in any order, plus the
        roundings of alpha, bias and beta * R;
      * 4 x the error of the same product evaluated on the host in fp32 with sequential accumulation over k, by the same
        measure against the same reference.  The kernel's order (two k per MFMA in a permuted sequence, then a fixed-order
        sum of the splits) is a different but equally long fp32 accumulation.
    Observed on an MI355X, in units of 2^-24, kernel / host / ceiling (the same figures under both transpose pairs):
      (130, 50, 178)    64x64   direct     2.885 / 2.681 / 182
      (1000, 900, 40)x4 128x128 direct     4.714 / 5.336 / 44
      (300, 32, 72)     128x32  direct     3.377 / 3.404 / 76
      (64, 64, 4096)    64x64   8 splits   0.807 / 4.000 / 4100
      (128, 128, 8192)  128x128 16 splits  0.633 / 4.204 / 8196
      (130, 50, 178)    64x64   rows 1e-2 .. 1e2   3.229 / 3.641 / 182
    so the kernel is within 1.08 x the host's sequential sum where it runs direct, and well below it under split-K (the
    splits make the sum partly pairwise); no case comes near either bar.  With the operands of the 128 x 128 tile passed
    through fp16 on their way to LDS (a trial build) the direct case on that tile fails this test and the integer tests
    do not."""
    alpha, beta = 0.75, -1.5
    scale = 10.0 ** np.linspace(-2.0, 2.0, M) if scaled else None
    A, B, bias, R = float_operands(M + N + K + int(scaled), M, N, K, batch, scale)
    if scaled:
        bias = None
    ref = reference(A, B, bias, R, alpha, beta, batch)
    mag = abs(alpha) * np.matmul(np.abs(A), np.abs(B)) + (0 if bias is None else np.abs(bias)) + abs(beta) * np.abs(R)
    out = run(ops, A, B, ta=ta, tb=tb, batch=batch, expect=(tile, splits), bias=bias, R=R, alpha=alpha, beta=beta, ws=ws)
    err = float((np.abs(out.cpu().double().numpy() - ref) / mag).max())
    host = float((np.abs(host_fp32(A, B, bias, R, alpha, beta).astype(np.float64) - ref) / mag).max())
    print("gemm accuracy %s batch %d ta %d tb %d %s splits %d scaled %d: kernel %.3f host %.3f ceiling %d (x 2^-24)" % (
        (M, N, K), batch, ta, tb, tile, splits, scaled, err / U, host / U, K + 4))
    assert host <= (K + 4) * U
    assert err <= (K + 4) * U
    assert err <= 4 * host
