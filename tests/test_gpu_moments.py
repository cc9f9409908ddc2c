"""GPU tests of mulan_set_moments_u8 (moments.hip), ops.set_moments_u8, mulan_amd.moments.set_moments and
python -m ldm.moments against tests/moments_oracle.py.  Every comparison of `sum` and `gram` is exact integer equality.

t8 and the sqrtm recipe.  The whole-path sets have n = 200 and 150 images of D = 3072: rank-deficient covariances, whose
product S_a S_b has about 2 900 zero eigenvalues.  scipy.linalg.sqrtm is not trustworthy there (the oracle's header says
so): measured on the CPU on these very sets it takes 13 s and its trace is 4.4e-8 of tr S_a + tr S_b away from the module,
against a bar of 4.9e-14.  The distance is therefore held, at that same bar, to the oracle's rank-aware statement of the
same quantity (`frechet_low_rank`: tr sqrtm(S_a S_b) is the nuclear norm of C_a C_b^T), measured 3e-16 away."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import moments_oracle as mo
from tests.test_moments import BAR_RECIPE

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIP_INVALID = 1                    # hipErrorInvalidValue


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def _run(x, splits=0, out=None):
    from mulan_amd import ops
    total, gram = ops.set_moments_u8(_dev(x) if isinstance(x, np.ndarray) else x, out=out, splits=splits)
    torch.cuda.synchronize()
    return total.cpu().numpy(), gram.cpu().numpy()


def _same(got, want):
    assert got[0].dtype == np.int64 and got[1].dtype == np.int64
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])


# ---------------------------------------------------------------------------------------------- t1: fill and lane map
ONE_HOT_ROWS = (0, 1, 3, 4, 15, 16, 31, 32, 63, 64 + 5)
ONE_HOT_COLS = ((4, 6),            # the same 4-byte group
                (33, 58),          # the same 32-column MFMA block
                (10, 100),         # the two halves of a tile
                (70, 200),         # two different tiles
                (129, 129))        # j0 = k0


@pytest.mark.parametrize("j0,k0", ONE_HOT_COLS)
def test_t1_one_hot_rows_reach_the_right_entries(j0, k0):
    N, D = 70, 256
    for i0 in ONE_HOT_ROWS:
        x = np.full((N, D), 128, np.uint8)
        x[i0, j0] = 129
        x[i0, k0] = 130                                       # with j0 = k0 this is the one that stays
        total, gram = _run(x)
        want_g, want_s = np.zeros((D, D), np.int64), np.zeros(D, np.int64)
        if j0 == k0:
            want_g[j0, j0], want_s[j0] = 4, 2
        else:
            want_g[j0, j0], want_g[k0, k0], want_g[j0, k0], want_g[k0, j0] = 1, 4, 2, 2
            want_s[j0], want_s[k0] = 1, 2
        assert np.array_equal(gram, want_g), (i0, np.argwhere(gram != want_g)[:8], gram[gram != want_g][:8])
        assert np.array_equal(total, want_s), (i0, np.flatnonzero(total != want_s)[:8])


# ---------------------------------------------------------------------------------------------- t2: edges of every loop
@pytest.mark.parametrize("D", [64, 192, 128 + 64 * 3])
@pytest.mark.parametrize("N", [1, 63, 64, 65, 2 * 64 + 1])
def test_t2_edges_of_rows_columns_and_slices(N, D):
    x = np.random.default_rng(1000 * N + D).integers(0, 256, (N, D), dtype=np.uint8)
    want = mo.integer_moments(x)
    if D == 64:
        _same(mo.integer_moments_loops(x), want)
    xd = _dev(x)
    for splits in (0, 1, 3, 7):                               # at N <= 129 there are at most 3 chunks: some slices are empty
        _same(_run(xd, splits), want)


def test_t2_the_production_width():
    x = np.random.default_rng(5).integers(0, 256, (130, 3072), dtype=np.uint8)
    _same(_run(x), mo.integer_moments(x))


# ---------------------------------------------------------------------------------------------- t3: the int32 hand-over
@pytest.mark.parametrize("pattern", ["zeros", "255", "alternating"])
def test_t3_more_rows_than_an_int32_accumulator_holds(pattern):
    N, D = 131073, 64
    if pattern == "zeros":
        x = torch.zeros((N, D), dtype=torch.uint8, device="cuda")
        col = np.full(D, -128, np.int64)
        row_sign_sum, row_count = N, N
    elif pattern == "255":
        x = torch.full((N, D), 255, dtype=torch.uint8, device="cuda")
        col = np.full(D, 127, np.int64)
        row_sign_sum, row_count = N, N
    else:                                                     # byte 255 where row + column is odd, else 0
        i, j = torch.arange(N, device="cuda")[:, None], torch.arange(D, device="cuda")[None, :]
        x = (((i + j) & 1) * 255).to(torch.uint8).contiguous()
        col = None
    total, gram = _run(x, splits=1)
    if col is not None:
        assert np.array_equal(total, col * N) and np.array_equal(gram, np.outer(col, col) * N)
        if pattern == "zeros":
            assert gram[0, 0] == N * 16384 > 2 ** 31 and total[0] == -128 * N
    else:
        even_rows, odd_rows = (N + 1) // 2, N // 2            # column j holds -128 on rows of j's parity, else 127
        v = lambda rows_parity, j: np.where((rows_parity + j) & 1, 127, -128).astype(np.int64)
        jj = np.arange(D)
        want_s = even_rows * v(0, jj) + odd_rows * v(1, jj)
        want_g = even_rows * np.outer(v(0, jj), v(0, jj)) + odd_rows * np.outer(v(1, jj), v(1, jj))
        assert np.array_equal(total, want_s) and np.array_equal(gram, want_g)
        assert gram.min() < 0 < gram.max()


# ---------------------------------------------------------------------------------------------- t4: splits
def test_t4_the_result_does_not_depend_on_splits():
    x = np.random.default_rng(7).integers(0, 256, (1000, 192), dtype=np.uint8)
    xd = _dev(x)
    first = _run(xd, 1)
    _same(first, mo.integer_moments(x))
    for splits in (2, 5, 0):
        got = _run(xd, splits)
        assert got[0].tobytes() == first[0].tobytes() and got[1].tobytes() == first[1].tobytes(), splits


# ---------------------------------------------------------------------------------------------- t5: accumulation
def test_t5_chunks_accumulate_and_a_fresh_call_overwrites():
    from mulan_amd import lib, ops
    x = np.random.default_rng(8).integers(0, 256, (700, 192), dtype=np.uint8)
    want = mo.integer_moments(x)
    out = None
    for lo, hi in ((0, 300), (300, 301), (301, 700)):
        out = ops.set_moments_u8(_dev(x[lo:hi]), out=out)
    torch.cuda.synchronize()
    _same((out[0].cpu().numpy(), out[1].cpu().numpy()), want)
    # accumulate = 0 overwrites arrays pre-filled with garbage
    D = 192
    xd = _dev(x)
    total = torch.full((D,), -(2 ** 40) - 12345, dtype=torch.int64, device="cuda")
    gram = torch.randint(-2 ** 60, 2 ** 60, (D, D), dtype=torch.int64, device="cuda")
    ws = torch.empty(lib.load().mulan_set_moments_u8_workspace(700, D, 0) // 8, dtype=torch.int64, device="cuda")
    lib.call("mulan_set_moments_u8", lib.ptr(xd), 700, D, 0, 0, lib.ptr(total), lib.ptr(gram), lib.ptr(ws), lib.stream())
    torch.cuda.synchronize()
    _same((total.cpu().numpy(), gram.cpu().numpy()), want)
    # the module: chunks of any size, the same integers
    from mulan_amd import moments as pm
    m = pm.set_moments(x.reshape(700, 8, 8, 3), chunk=256)
    assert m["n"] == 700 and m["shape"] == (8, 8, 3)
    _same((m["sum"], m["gram"]), want)
    assert np.array_equal(m["cov"], mo.mean_cov(700, *want)[1]) and np.array_equal(m["mean"], mo.mean_cov(700, *want)[0])


# ---------------------------------------------------------------------------------------------- t6: symmetry
def test_t6_gram_is_its_own_transpose_and_its_diagonal_the_sums_of_squares():
    x = np.random.default_rng(9).integers(0, 256, (333, 128 + 64 * 3), dtype=np.uint8)
    total, gram = _run(x)
    assert gram.tobytes() == np.ascontiguousarray(gram.T).tobytes()
    c = x.astype(np.int64) - 128
    assert np.array_equal(np.diag(gram), (c * c).sum(axis=0)) and np.array_equal(total, c.sum(axis=0))


# ---------------------------------------------------------------------------------------------- t7: refusals
def test_t7_refusals_come_before_any_launch():
    from mulan_amd import lib, ops
    h = lib.load()
    x = torch.zeros((8, 128), dtype=torch.uint8, device="cuda")
    good = (torch.zeros(128, dtype=torch.int64, device="cuda"), torch.zeros((128, 128), dtype=torch.int64, device="cuda"))
    for bad, match in ((x.int(), "uint8"), (x[:, :64], "contiguous"), (x[:, :96].contiguous(), "multiple of 64"),
                       (x.reshape(8, 2, 64), "uint8"), (x.cpu().numpy(), "tensor on the device")):
        with pytest.raises(ValueError, match=match):
            ops.set_moments_u8(bad)
    for out, match in (((good[0].cpu(), good[1]), "out is on"), ((good[0], good[1].cpu()), "out is on"),
                       ((good[0].int(), good[1]), "sum"), ((good[0], good[1][:, :64]), "gram"), (good[:1], "pair")):
        with pytest.raises(ValueError, match=match):
            ops.set_moments_u8(x, out=out)
    with pytest.raises(ValueError, match="splits"):
        ops.set_moments_u8(x, splits=4097)
    # the library called directly: hipErrorInvalidValue, a workspace of 0, the outputs untouched
    N, D = 8, 128
    for args in ((0, D, 0), (2 ** 24 + 1, D, 0), (N, 32, 0), (N, 96, 0), (N, 4160, 0), (N, D, -1), (N, D, 4097)):
        assert h.mulan_set_moments_u8_workspace(*args) == 0, args
    assert h.mulan_set_moments_u8_workspace(N, D, 3) == 3 * (128 * 128 + D) * 8
    assert h.mulan_set_moments_u8_workspace(2 ** 24, 4096, 1) == (528 * 128 * 128 + 4096) * 8
    total = torch.full((D,), 77, dtype=torch.int64, device="cuda")
    gram = torch.full((D, D), -5, dtype=torch.int64, device="cuda")
    ws = torch.zeros(h.mulan_set_moments_u8_workspace(N, D, 0) // 8 + 2, dtype=torch.int64, device="cuda")
    s = lib.stream()
    px, pt, pg, pw = lib.ptr(x), lib.ptr(total), lib.ptr(gram), lib.ptr(ws)
    cases = [(px, 0, D, 0, 0, pt, pg, pw), (px, 2 ** 24 + 1, D, 0, 0, pt, pg, pw), (px, N, 32, 0, 0, pt, pg, pw),
             (px, N, 96, 0, 0, pt, pg, pw), (px, N, 4160, 0, 0, pt, pg, pw), (px, N, D, 2, 0, pt, pg, pw),
             (px, N, D, -1, 0, pt, pg, pw), (px, N, D, 0, -1, pt, pg, pw), (px, N, D, 0, 4097, pt, pg, pw),
             (None, N, D, 0, 0, pt, pg, pw), (px, N, D, 0, 0, None, pg, pw), (px, N, D, 0, 0, pt, None, pw),
             (px, N, D, 0, 0, pt, pg, None), (px + 4, N, D, 0, 0, pt, pg, pw), (px, N, D, 0, 0, pt + 4, pg, pw),
             (px, N, D, 0, 0, pt, pg + 4, pw), (px, N, D, 0, 0, pt, pg, pw + 4)]
    for case in cases:
        assert h.mulan_set_moments_u8(*case, s) == HIP_INVALID, case
    torch.cuda.synchronize()
    assert bool((total == 77).all()) and bool((gram == -5).all()) and bool((ws == 0).all())


# ---------------------------------------------------------------------------------------------- t8: whole path, CLI
def test_t8_command_line_writes_the_oracles_integers_and_distance(tmp_path):
    xa = mo.smoothed_bytes(11, 200, 3072, width=5).reshape(200, 32, 32, 3)
    xb = mo.smoothed_bytes(12, 150, 3072, scale=30.0, width=7, offset=5.0).reshape(150, 32, 32, 3)
    np.savez(tmp_path / "s.npz", images=xa)
    np.savez(tmp_path / "r.npz", images=xb)
    env = dict(os.environ, PYTHONPATH=ROOT)
    env.pop("WORLD_SIZE", None)
    base = [sys.executable, "-m", "ldm.moments", "--samples=" + str(tmp_path / "s.npz"), "--eigen", "4", "--chunk", "128"]
    r = subprocess.run(base + ["--reference=npz:" + str(tmp_path / "r.npz"), "--out=" + str(tmp_path / "m1.npz"),
                               "--save_reference_moments=" + str(tmp_path / "ref.npz")],
                       capture_output=True, text=True, timeout=600, cwd=ROOT, env=env)
    assert r.returncode == 0 and "not comparable with published FID" in r.stdout, (r.stdout[-2000:], r.stderr[-3000:])
    r = subprocess.run(base + ["--reference=moments:" + str(tmp_path / "ref.npz"), "--out=" + str(tmp_path / "m2.npz")],
                       capture_output=True, text=True, timeout=600, cwd=ROOT, env=env)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    with np.load(tmp_path / "m1.npz") as z1, np.load(tmp_path / "m2.npz") as z2:
        a, b = dict(z1), dict(z2)
    assert sorted(a) == sorted(b)
    for key in a:
        if key != "settings":
            assert a[key].dtype == b[key].dtype and a[key].tobytes() == b[key].tobytes(), key
    Ia, Ib = mo.integer_moments(xa.reshape(200, -1)), mo.integer_moments(xb.reshape(150, -1))
    assert int(a["n_samples"]) == 200 and int(a["n_reference"]) == 150
    _same((a["sum_samples"], a["gram_samples"]), Ia)
    _same((a["sum_reference"], a["gram_reference"]), Ib)
    A, B = mo.mean_cov(200, *Ia), mo.mean_cov(150, *Ib)
    tr = float(np.trace(A[1]) + np.trace(B[1]))
    bar = max(BAR_RECIPE.values())
    want = mo.frechet_low_rank(xa.reshape(200, -1), xb.reshape(150, -1))
    rel = [abs(float(a[k]) - w) / tr for k, w in zip(("distance", "mean_term", "cov_term"), want)]
    print(f"t8: distance {float(a['distance']):.6f}, {rel[0]:.3e} {rel[1]:.3e} {rel[2]:.3e} of the traces, bar {bar:.3e}")
    assert max(rel) <= bar
    for name, cov in (("samples", A[1]), ("reference", B[1])):
        dev = np.abs(a["eigenvalues_" + name] - mo.eigenvalues(cov)).max() / tr
        print(f"t8: eigenvalues of the {name}: {dev:.3e} of the traces")
        assert dev <= bar
    assert np.array_equal(a["mean_samples"].reshape(-1), A[0]) and np.array_equal(a["mean_reference"].reshape(-1), B[0])
    assert a["eigen_images_samples"].shape == (4, 32, 32, 3) and a["eigen_ratio_reference"].shape == (4,)
    v = a["eigen_images_samples"].reshape(4, -1)
    assert np.abs(A[1] @ v.T - v.T * a["eigenvalues_samples"][:4]).max() <= 1e-9 * a["eigenvalues_samples"][0]
