"""CPU tests of mulan_amd/moments.py (host float64 arithmetic on exact integers), of ops.set_moments_check and of the
flags of python -m ldm.moments.  The integers come from tests/moments_oracle.py; no device is touched.

Rounding bars.  The checks "a set against itself gives 0", "a shift by c gives D c^2 with cov_term 0" and "the distance is
symmetric" hold only to float64 rounding.  Their bars are 8 x the deviation of the ORACLE's own recipe
(scipy.linalg.sqrtm of S_a S_b) measured on the CPU at this file's shapes and seeds, relative to tr S_a + tr S_b:

    shape            self = 0      shift = D c^2    cov_term = 0    symmetric
    D = 64, n = 300   3.715e-15     3.715e-15        3.715e-15       2.436e-15
    D = 192, n = 600  8.888e-16     8.888e-16        8.888e-16       1.119e-16

(the module, measured at the same time: 5.23e-15 / 2.31e-15 for the first three, 0 for symmetry, which it has by
construction).  Agreement of the module with the sqrtm recipe on the well-conditioned sets (condition numbers 3e3 to
3e4): the difference measured on the CPU is 6.091e-15 (D = 64, n = 300) and 2.351e-15 (D = 192, n = 600) of
tr S_a + tr S_b, and the margin is 8 x that.  The integer checks are exact."""
import os

import numpy as np
import pytest
import torch

from tests import moments_oracle as mo

SHIFT = 10
SHAPES = ((64, 300), (192, 600))
# 8 x the oracle recipe's own deviation (header), relative to tr S_a + tr S_b
BAR_SELF = {64: 8 * 3.715e-15, 192: 8 * 8.888e-16}
BAR_SHIFT = {64: 8 * 3.715e-15, 192: 8 * 8.888e-16}
BAR_SYMMETRIC = {64: 8 * 2.436e-15, 192: 8 * 1.119e-16}
# 8 x the measured difference between the module and the sqrtm recipe (header)
BAR_RECIPE = {64: 8 * 6.091e-15, 192: 8 * 2.351e-15}


def _sets(D, n):
    xa, xb = mo.smoothed_bytes(1, n, D), mo.smoothed_bytes(2, n, D, scale=30.0, offset=5.0)
    return xa, xb, (xa.astype(np.int64) + SHIFT).astype(np.uint8)      # [16, 239] + 10: no clipping


@pytest.fixture(scope="module")
def sets():
    """per D: the three byte sets, their oracle integers and the module's dicts; computed once, never modified"""
    from mulan_amd import moments as pm
    out = {}
    for D, n in SHAPES:
        xs = dict(zip("abs", _sets(D, n)))
        ints = {k: mo.integer_moments(x) for k, x in xs.items()}
        out[D] = dict(x=xs, ints=ints, m={k: pm.moments_from_integers(n, *ints[k]) for k in xs},
                      o={k: mo.mean_cov(n, *ints[k]) for k in xs}, n=n)
    return out


def _traces(s, p, q):
    return float(np.trace(s["o"][p][1]) + np.trace(s["o"][q][1]))


def test_oracle_integer_forms_agree():
    x = np.random.default_rng(0).integers(0, 256, (130, 64), dtype=np.uint8)
    a, b = mo.integer_moments(x), mo.integer_moments_loops(x)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    assert a[1].dtype == np.int64 and np.array_equal(a[1], a[1].T)


@pytest.mark.parametrize("D", [64, 192])
def test_a_set_against_itself_gives_zero(sets, D):
    from mulan_amd import moments as pm
    s = sets[D]
    r = pm.frechet_distance(s["m"]["a"], s["m"]["a"])
    rel = abs(r["distance"]) / _traces(s, "a", "a")
    print(f"self D = {D}: {rel:.3e} of the traces, bar {BAR_SELF[D]:.3e}")
    assert r["mean_term"] == 0.0 and rel <= BAR_SELF[D]


@pytest.mark.parametrize("D", [64, 192])
def test_a_shift_of_every_byte_gives_D_c_squared(sets, D):
    from mulan_amd import moments as pm
    s = sets[D]
    assert np.array_equal(s["ints"]["a"][1] * s["n"] - np.outer(s["ints"]["a"][0], s["ints"]["a"][0]),
                          s["ints"]["s"][1] * s["n"] - np.outer(s["ints"]["s"][0], s["ints"]["s"][0]))   # same covariance, exactly
    r = pm.frechet_distance(s["m"]["a"], s["m"]["s"])
    tr = _traces(s, "a", "s")
    rel, rel_cov = abs(r["distance"] - D * SHIFT ** 2) / tr, abs(r["cov_term"]) / tr
    print(f"shift D = {D}: {rel:.3e}, cov_term {rel_cov:.3e} of the traces, bar {BAR_SHIFT[D]:.3e}")
    assert rel <= BAR_SHIFT[D] and rel_cov <= BAR_SHIFT[D]
    assert abs(r["mean_term"] - D * SHIFT ** 2) <= 4 * np.finfo(np.float64).eps * D * 255.0 ** 2      # D differences of bytes


@pytest.mark.parametrize("D", [64, 192])
def test_the_distance_is_symmetric(sets, D):
    from mulan_amd import moments as pm
    s = sets[D]
    ab, ba = pm.frechet_distance(s["m"]["a"], s["m"]["b"]), pm.frechet_distance(s["m"]["b"], s["m"]["a"])
    rel = abs(ab["distance"] - ba["distance"]) / _traces(s, "a", "b")
    print(f"symmetry D = {D}: {rel:.3e} of the traces, bar {BAR_SYMMETRIC[D]:.3e}")
    assert rel <= BAR_SYMMETRIC[D] and ab["distance"] > 0


@pytest.mark.parametrize("D", [64, 192])
def test_agreement_with_the_sqrtm_recipe(sets, D):
    from mulan_amd import moments as pm
    s = sets[D]
    got = pm.compare_moments(s["m"]["a"], s["m"]["b"])
    want = mo.frechet_sqrtm(*s["o"]["a"], *s["o"]["b"])
    tr = _traces(s, "a", "b")
    rel = [abs(got[k] - w) / tr for k, w in zip(("distance", "mean_term", "cov_term"), want)]
    print(f"sqrtm recipe D = {D}: {rel[0]:.3e} {rel[1]:.3e} {rel[2]:.3e} of the traces, bar {BAR_RECIPE[D]:.3e}")
    assert max(rel) <= BAR_RECIPE[D]
    assert abs(got["distance"] - (got["mean_term"] + got["cov_term"])) <= 1e-15 * tr
    for key, cov in (("eigenvalues_a", s["o"]["a"][1]), ("eigenvalues_b", s["o"]["b"][1])):
        assert got[key].shape == (D,) and np.all(np.diff(got[key]) <= 0)
        assert np.abs(got[key] - mo.eigenvalues(cov)).max() <= BAR_RECIPE[D] * tr
    sd = np.sqrt(np.diag(s["o"]["a"][1])) - np.sqrt(np.diag(s["o"]["b"][1]))
    mu = s["o"]["a"][0] - s["o"]["b"][0]
    assert abs(got["frechet_diag_pixel"] - float((mu * mu + sd * sd).sum())) <= 1e-12 * tr
    assert abs(got["trace_ratio"] - np.trace(s["o"]["a"][1]) / np.trace(s["o"]["b"][1])) <= 1e-14


def test_diagonal_covariances_give_the_sum_of_squared_sigma_differences():
    """integers with sum = 0 and a diagonal gram: cov = gram / (n - 1) is diagonal, the means are equal, and the distance
    is sum (sigma_a - sigma_b)^2.  Bar: the eigendecomposition of a diagonal matrix returns its entries, so what is left
    is D square roots, products and sums: 8 D eps of tr S_a + tr S_b."""
    from mulan_amd import moments as pm
    D, n = 96, 50
    rng = np.random.default_rng(3)
    ga, gb = rng.integers(1, 10 ** 6, D), rng.integers(1, 10 ** 6, D)
    a = pm.moments_from_integers(n, np.zeros(D, np.int64), np.diag(ga))
    b = pm.moments_from_integers(n, np.zeros(D, np.int64), np.diag(gb))
    want = float(((np.sqrt(ga / (n - 1)) - np.sqrt(gb / (n - 1))) ** 2).sum())
    tr = float((ga.sum() + gb.sum()) / (n - 1))
    r = pm.compare_moments(a, b)
    bar = 8 * D * np.finfo(np.float64).eps
    assert r["mean_term"] == 0.0 and abs(r["distance"] - want) <= bar * tr
    assert abs(r["frechet_diag_pixel"] - want) <= bar * tr          # on diagonal covariances the two forms coincide


@pytest.mark.parametrize("D", [64, 192])
def test_merge_of_two_halves_is_the_whole_and_cov_is_numpy_cov(sets, D):
    """Bar of the covariance against numpy.cov: numpy centres and multiplies in float64, n products of at most 128^2 per
    entry, each rounded: n eps 128^2 / (n - 1) < 1e-11; the module's own entry is one rounding of an exact integer."""
    from mulan_amd import moments as pm
    s = sets[D]
    x, n = s["x"]["a"], s["n"]
    h = n // 3
    lo, hi = (pm.moments_from_integers(len(p), *mo.integer_moments(p)) for p in (x[:h], x[h:]))
    whole = pm.merge_moments(lo, hi)
    assert whole["n"] == n and np.array_equal(whole["sum"], s["ints"]["a"][0]) and np.array_equal(whole["gram"], s["ints"]["a"][1])
    assert whole["sum"].dtype == np.int64 and whole["gram"].dtype == np.int64
    assert np.array_equal(whole["cov"], s["m"]["a"]["cov"]) and np.array_equal(whole["mean"], s["m"]["a"]["mean"])
    assert np.abs(whole["cov"] - np.cov(x.T.astype(np.float64))).max() <= 1e-11
    assert np.abs(whole["mean"] - x.astype(np.float64).mean(axis=0)).max() <= 1e-12
    assert np.array_equal(whole["cov"], mo.mean_cov(n, *s["ints"]["a"])[1])
    with pytest.raises(ValueError, match="D ="):
        pm.merge_moments(lo, sets[256 - D]["m"]["a"])


def test_one_image_has_no_covariance_and_bad_integers_are_refused():
    from mulan_amd import moments as pm
    with pytest.raises(ValueError, match="2 <= n"):
        pm.moments_from_integers(1, np.zeros(64, np.int64), np.zeros((64, 64), np.int64))
    with pytest.raises(ValueError, match="2 <= n"):
        pm.set_moments(np.zeros((1, 64), np.uint8))
    with pytest.raises(ValueError, match="gram"):
        pm.moments_from_integers(5, np.zeros(64, np.int64), np.zeros((64, 32), np.int64))
    with pytest.raises(ValueError, match="uint8"):
        pm.set_moments(np.zeros((4, 64), np.float32))
    with pytest.raises(ValueError, match="chunk"):
        pm.set_moments(np.zeros((4, 64), np.uint8), chunk=0)
    with pytest.raises(ValueError, match="multiple of 64"):
        pm.set_moments(np.zeros((4, 5, 5, 3), np.uint8))          # refused on the shape, before any device is looked for
    with pytest.raises(ValueError, match="dict of set_moments"):
        pm.frechet_distance({}, {})


def test_eigen_images_shape_order_sign_and_share(sets):
    from mulan_amd import moments as pm
    s = sets[192]
    m = dict(s["m"]["a"], shape=(8, 8, 3))
    e = pm.eigen_images(m, k=5)
    assert e["images"].shape == (5, 8, 8, 3) and e["eigenvalues"].shape == (5,) and np.all(np.diff(e["eigenvalues"]) <= 0)
    tr = float(np.trace(s["o"]["a"][1]))
    assert np.abs(e["eigenvalues"] - mo.eigenvalues(s["o"]["a"][1])[:5]).max() <= BAR_RECIPE[192] * tr
    assert np.abs(e["ratio"] - e["eigenvalues"] / tr).max() <= 1e-15
    v = e["images"].reshape(5, -1)
    assert np.abs(v @ v.T - np.eye(5)).max() <= 1e-12
    assert np.abs(s["o"]["a"][1] @ v.T - v.T * e["eigenvalues"]).max() <= 1e-9 * e["eigenvalues"][0]
    assert np.all(v[np.arange(5), np.abs(v).argmax(axis=1)] > 0)        # pca_transformation's sign rule
    for k in (0, 193, True, 2.0):
        with pytest.raises(ValueError, match="eigen_images: k"):
            pm.eigen_images(m, k=k)


def test_save_and_load_round_trip(sets, tmp_path):
    from mulan_amd import moments as pm
    m = dict(sets[192]["m"]["b"], shape=(8, 8, 3))
    path = str(tmp_path / "ref.npz")
    pm.save_moments(path, m, settings=dict(reference="npz:x", n=m["n"]))
    back, settings = pm.load_moments(path, return_settings=True)
    assert back["n"] == m["n"] and back["shape"] == (8, 8, 3) and settings == dict(reference="npz:x", n=m["n"])
    for key in ("sum", "gram", "mean", "cov"):
        assert back[key].dtype == m[key].dtype and np.array_equal(back[key], m[key]), key
    with pytest.raises(ValueError, match=".npz"):
        pm.save_moments(str(tmp_path / "ref.txt"), m)
    np.savez(tmp_path / "other.npz", images=np.zeros(3))
    with pytest.raises(ValueError, match="holds no n, sum and gram"):
        pm.load_moments(str(tmp_path / "other.npz"))


class _Shape:
    """something with dtype and shape: ops.set_moments_check needs no more"""

    def __init__(self, shape, dtype="uint8"):
        self.shape, self.dtype = tuple(shape), dtype


def test_set_moments_check_on_shapes_alone():
    from mulan_amd import ops
    assert ops.set_moments_check(_Shape((50000, 3072))) == (50000, 3072)
    assert ops.set_moments_check(_Shape((1, 64)), splits=4096) == (1, 64)
    assert ops.set_moments_check(_Shape((2 ** 24, 4096))) == (2 ** 24, 4096)
    for bad, match in ((_Shape((4, 64), "int8"), "uint8"), (_Shape((4, 8, 8)), "uint8"), (_Shape((0, 64)), "uint8"),
                       (np.zeros((4, 64), np.float32), "uint8"), ([[1]], "uint8"),
                       (_Shape((4, 32)), "multiple of 64"), (_Shape((4, 100)), "multiple of 64"),
                       (_Shape((4, 4160)), "multiple of 64"), (_Shape((2 ** 24 + 1, 64)), "2\\^24")):
        with pytest.raises(ValueError, match=match):
            ops.set_moments_check(bad)
    for splits in (-1, 4097, 1.0, True):
        with pytest.raises(ValueError, match="splits"):
            ops.set_moments_check(_Shape((4, 64)), splits=splits)
    with pytest.raises(ValueError, match="contiguous"):
        ops.set_moments_check(torch.zeros((64, 8), dtype=torch.uint8).t())
    good = (torch.zeros(64, dtype=torch.int64), torch.zeros((64, 64), dtype=torch.int64))
    assert ops.set_moments_check(_Shape((4, 64)), out=good) == (4, 64)
    for out, match in ((good[0], "pair"), (good + good, "pair"), ((good[0].int(), good[1]), "sum"),
                       ((good[0], good[1][:, :32]), "gram"), ((good[0], good[1].t()[::1].double()), "gram"),
                       ((torch.zeros(128, dtype=torch.int64), good[1]), "sum"), ((good[0], np.zeros((64, 64), np.int64)), "gram")):
        with pytest.raises(ValueError, match=match):
            ops.set_moments_check(_Shape((4, 64)), out=out)
    with pytest.raises(ValueError, match="tensor on the device"):
        ops.set_moments_u8(np.zeros((4, 64), np.uint8))            # a host array passes the shape check, not the call


def _args(tmp_path, *more, reference=None):
    return ["--samples=" + str(tmp_path / "s.npz"), "--reference=" + (reference or "npz:" + str(tmp_path / "r.npz")),
            "--out=" + str(tmp_path / "m.npz"), *more]


def test_cli_flag_refusals(tmp_path, monkeypatch, sets):
    from ldm import moments as cli
    from mulan_amd import moments as pm
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    with pytest.raises(SystemExit, match="no file"):
        cli.parse_flags(_args(tmp_path))
    np.savez(tmp_path / "s.npz", images=np.zeros((2, 32, 32, 3), np.uint8))
    f = cli.parse_flags(_args(tmp_path))
    assert (f.max_reference, f.chunk, f.eigen, f.save_reference_moments) == (0, 16384, 16, None)
    f = cli.parse_flags(_args(tmp_path, "--max_reference", "100", "--eigen=4", "--chunk=64",
                              "--save_reference_moments=" + str(tmp_path / "ref.npz")))
    assert (f.max_reference, f.chunk, f.eigen) == (100, 64, 4) and f.save_reference_moments.endswith("ref.npz")
    assert cli.parse_flags(_args(tmp_path, reference="imagenet32")).reference == "imagenet32"
    with pytest.raises(SystemExit, match="synthetic has no fixed set"):
        cli.parse_flags(_args(tmp_path, reference="synthetic"))
    with pytest.raises(SystemExit, match="--reference"):
        cli.parse_flags(_args(tmp_path, reference="mnist"))
    for more, match in ((["--chunk=0"], "--chunk"), (["--eigen=-1"], "--eigen"), (["--eigen=3073"], "--eigen"),
                        (["--max_reference=-1"], "--max_reference"), (["--save_reference_moments=r.txt"], ".npz")):
        with pytest.raises(SystemExit, match=match):
            cli.parse_flags(_args(tmp_path, *more))
    with pytest.raises(SystemExit, match=".npz"):
        cli.parse_flags(_args(tmp_path)[:2] + ["--out=m.txt"])
    with pytest.raises(SystemExit, match="required"):
        cli.parse_flags(_args(tmp_path)[:2])
    with pytest.raises(SystemExit, match="no file"):
        cli.parse_flags(_args(tmp_path, reference="moments:" + str(tmp_path / "none.npz")))
    # saved moments of another D are refused when they are read, before any device is touched
    pm.save_moments(str(tmp_path / "d192.npz"), sets[192]["m"]["a"])
    f = cli.parse_flags(_args(tmp_path, reference="moments:" + str(tmp_path / "d192.npz")))
    with pytest.raises(SystemExit, match="D = 192, the samples have D = 3072"):
        cli.read_inputs(f)
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(SystemExit, match="one process"):
        cli.parse_flags(_args(tmp_path))
