"""CPU tests of the nearest-neighbour analysis (mulan_knn_u8 / ops.knn_u8 / mulan_amd.neighbours / python -m
ldm.neighbours): the declaration and the binding rows, the brute-force oracle on a hand-made case, every refusal before
any library call, the host reductions on hand-made lists, the chunked walk over a stand-in for the kernel (the oracle
itself), and the command line.  The kernel itself is held to the oracle in tests/test_gpu_neighbours.py."""
import json
import os
import re

import numpy as np
import pytest
import torch

from tests import neighbours_oracle as no

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------ the boundary
def test_header_declares_both_symbols_and_the_binding_table_binds_them():
    from mulan_amd import lib
    P, I = lib.P, lib.I
    assert lib.SIGNATURES["mulan_knn_u8"] == [P, P, I, I, I, I, I, I, I, I, P, P, P, P, P, P]
    assert lib.SIGNATURES["mulan_knn_u8_workspace"] == [I, I, I]
    assert lib._RESTYPES["mulan_knn_u8_workspace"] is lib.c_size_t
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mulan_hip.h")).read(), flags=re.S)
    m = re.search(r"\bint\s+mulan_knn_u8\s*\(([^;]*?)\)\s*;", src, flags=re.S)
    assert m and len(m.group(1).split(",")) == 16
    m = re.search(r"\bsize_t\s+mulan_knn_u8_workspace\s*\(([^;]*?)\)\s*;", src, flags=re.S)
    assert m and len(m.group(1).split(",")) == 3
    assert "mulan_knn_u8" in open(os.path.join(ROOT, "INTEGRATION.md")).read()


def test_the_kernel_source_uses_the_int8_matrix_builtin():
    src = open(os.path.join(ROOT, "mulan_amd", "csrc", "neighbours.hip")).read()
    assert "__builtin_amdgcn_mfma_i32_32x32x32_i8" in src and "asm" not in re.sub(r"//.*", "", src)
    assert "atomic" not in re.sub(r"//.*", "", src)


# ------------------------------------------------------------------------------------------------ the oracle
def hand_made():
    """six references in D = 64 around a query set: planted ties and a planted self-match"""
    r = np.full((6, 64), 100, dtype=np.uint8)
    r[1, 0] = 103            # d2 9 to the base row
    r[2, 5] = 97             # d2 9 as well: a tie with row 1
    r[3, :2] = (101, 102)    # d2 5
    r[4] = r[0]              # a copy of row 0: d2 0, tie with row 0 itself
    r[5, 63] = 110           # d2 100
    return r


def test_oracle_on_a_hand_made_case_with_ties_and_a_self_match():
    r = hand_made()
    q = r[:1].copy()
    d, i = no.knn(q, r, 6)
    assert d.tolist() == [[0, 0, 5, 9, 9, 100]] and i.tolist() == [[0, 4, 3, 1, 2, 5]]      # ties in index order
    d, i = no.knn(q, r, 3, idx_base=10)
    assert d.tolist() == [[0, 0, 5]] and i.tolist() == [[10, 14, 13]]
    d, i = no.knn(r, r, 2, self_offset=0)                                                   # no row reports itself
    assert i[:, 0].tolist() == [4, 3, 0, 0, 0, 0] and d[:, 0].tolist() == [0, 8, 9, 5, 0, 100]
    assert (i != np.arange(6)[:, None]).all()
    d, i = no.knn(q, r, 2, idx_base=7, self_offset=7)                                       # the self pair, shifted
    assert i.tolist() == [[11, 10]] and d.tolist() == [[0, 5]]
    d, i = no.knn(q, r[:3], 5)                                                              # fewer references than k
    assert d.tolist() == [[0, 9, 9, no.EMPTY_D, no.EMPTY_D]] and i.tolist() == [[0, 1, 2, -1, -1]]
    assert no.EMPTY_D == 2 ** 31 - 1 and no.EMPTY_I == -1
    # radius coverage: <= is inside, one more is outside; the excluded pair does not cover
    rad = np.array([0, 8, 9, 4, 0, 99], dtype=np.int32)
    assert no.covered(q, r, rad).tolist() == [True]
    assert no.covered(q, r, rad, self_offset=0).tolist() == [True]                          # row 4, the copy
    assert no.covered(q, r[:4], rad[:4], self_offset=0).tolist() == [True]                  # row 2 at exactly 9
    assert no.covered(q, r[:4], np.array([0, 8, 8, 4], dtype=np.int32), self_offset=0).tolist() == [False]
    # chunks merged equal one call; the table is symmetric when a set meets itself
    whole = no.knn(r, r, 3)
    parts = no.knn(r, r[:2], 3)
    for lo in (2, 4):
        parts = no.merge(parts, no.knn(r, r[lo:lo + 2], 3, idx_base=lo), 3)
    assert np.array_equal(parts[0], whole[0]) and np.array_equal(parts[1], whole[1])
    assert np.array_equal(no.dist2_table(r, r), no.dist2_table(r, r.copy()))
    assert no.dist2_table(np.zeros((1, 64), np.uint8), np.full((1, 64), 255, np.uint8))[0, 0] == 64 * 255 ** 2


# ------------------------------------------------------------------------------------------------ refusals
def _no_library(monkeypatch):
    from mulan_amd import lib, ops

    def no_call(*a, **k):
        raise AssertionError("the library was called")
    monkeypatch.setattr(ops, "call", no_call)
    monkeypatch.setattr(lib, "load", no_call)
    monkeypatch.setattr(lib, "call", no_call)


def test_ops_argument_checks_come_before_any_library_call(monkeypatch):
    from mulan_amd import ops
    _no_library(monkeypatch)
    q, r = torch.zeros((4, 128), dtype=torch.uint8), torch.zeros((7, 128), dtype=torch.uint8)
    ok = dict(q=q, r=r, k=3)
    bad = [
        (dict(q=q.float()), "uint8"), (dict(r=r.to(torch.int8)), "uint8"), (dict(q=q[0]), "uint8"),
        (dict(r=torch.zeros((7, 192), dtype=torch.uint8)), "D = 128"),
        (dict(q=torch.zeros((4, 96), dtype=torch.uint8), r=torch.zeros((7, 96), dtype=torch.uint8)), "multiple of 64"),
        (dict(q=torch.zeros((4, 16448), dtype=torch.uint8), r=torch.zeros((7, 16448), dtype=torch.uint8)), "multiple of 64"),
        (dict(k=0), r"k is"), (dict(k=17), r"k is"), (dict(k=2.0), r"k is"),
        (dict(covered=torch.zeros(4, dtype=torch.uint8)), "needs radius2"),
        (dict(radius2=torch.zeros(7, dtype=torch.int64)), "radius2 is int32"),
        (dict(radius2=torch.zeros(6, dtype=torch.int32)), "radius2 is int32"),
        (dict(radius2=torch.zeros(7, dtype=torch.int32), covered=torch.zeros(5, dtype=torch.uint8)), "covered is uint8"),
        (dict(idx_base=-1), "idx_base"), (dict(idx_base=2 ** 31 - 7), "idx_base"), (dict(self_offset=-2), "self_offset"),
        (dict(splits=-1), "splits"), (dict(splits=5000), "splits"),
        (dict(out=(torch.zeros((4, 3), dtype=torch.int32),)), "pair"),
        (dict(out=(torch.zeros((4, 3), dtype=torch.int32), torch.zeros((4, 2), dtype=torch.int32))), "idx is"),
        (dict(out=(torch.zeros((4, 3), dtype=torch.int64), torch.zeros((4, 3), dtype=torch.int32))), "dist2 is"),
    ]
    for change, match in bad:
        with pytest.raises(ValueError, match=match):
            ops.knn_u8(**{**ok, **change})
    with pytest.raises(ValueError, match="tensors on one device"):
        ops.knn_u8(q.numpy(), r, 3)
    with pytest.raises(AssertionError, match="the library was called"):      # and a good call does reach the library
        ops.knn_u8(**ok)


def test_neighbours_argument_checks_come_before_any_library_call(monkeypatch):
    from mulan_amd import neighbours as nb
    _no_library(monkeypatch)
    img = np.zeros((5, 32, 32, 3), dtype=np.uint8)
    flat = np.zeros((5, 128), dtype=np.uint8)
    for fn in (lambda **kw: nb.nearest(kw.pop("a"), kw.pop("b"), **kw), lambda **kw: nb.novelty(kw.pop("a"), kw.pop("b"), **kw),
               lambda **kw: nb.precision_recall(kw.pop("a"), kw.pop("b"), **kw)):
        with pytest.raises(ValueError, match="uint8"):
            fn(a=img.astype(np.float32), b=img)
        with pytest.raises(ValueError, match="uint8"):
            fn(a=img, b=torch.zeros((5, 32, 32, 3)))
        with pytest.raises(ValueError, match="D = "):
            fn(a=img, b=flat)
        with pytest.raises(ValueError, match="multiple of 64"):
            fn(a=np.zeros((5, 96), np.uint8), b=np.zeros((5, 96), np.uint8))
        for k in (0, 17):
            with pytest.raises(ValueError, match="k is"):
                fn(a=img, b=img, k=k)
        with pytest.raises(ValueError):
            fn(a=[[1, 2]], b=img)
        with pytest.raises(ValueError):
            fn(a=np.zeros((5, 32, 32), np.uint8), b=img)
    with pytest.raises(ValueError, match="chunk"):
        nb.nearest(img, img, chunk=0)
    with pytest.raises(ValueError, match="exclude_self"):
        nb.nearest(img[:3], img, exclude_self=True)
    with pytest.raises(ValueError, match="radius2 is int32"):
        nb.nearest(img, img, radius2=np.zeros(5, dtype=np.int64))
    with pytest.raises(ValueError, match="more than k"):
        nb.precision_recall(img[:3], img, k=3)
    with pytest.raises(ValueError, match="at least two"):
        nb.novelty(img[:1], img)
    with pytest.raises(ValueError, match="yardstick"):
        nb.novelty(img, img, yardstick=0)


# ------------------------------------------------------------------------------------------------ host reductions
def test_novelty_reduces_hand_made_lists_to_the_right_figures():
    from mulan_amd import neighbours as nb
    D = 64
    nn_d = np.array([[0, 64, 256], [64, 64, 640], [6400, 6400, 6400], [16, 1600, 1600]], dtype=np.int32)
    nn_i = np.array([[7, 1, 2], [3, 4, 0], [9, 8, 5], [2, 6, 1]], dtype=np.int32)
    self_d = np.array([64, 64, 65, no.EMPTY_D], dtype=np.int32)        # rms 1, 1, just above 1, nothing found
    self_i = np.array([1, 0, 0, -1], dtype=np.int32)
    out = nb.novelty_from_lists(nn_d, nn_i, self_d, self_i, np.array([256, 1024]), D)
    assert out["nn_rms"].tolist() == [0.0, 1.0, 10.0, 0.5]
    assert out["self_rms"][:2].tolist() == [1.0, 1.0] and out["self_rms"][2] > 1.0 and np.isinf(out["self_rms"][3])
    assert out["duplicates"] == 0.5 and out["duplicate_rms"] == 1.0
    assert out["train_self_rms"].tolist() == [2.0, 4.0]
    assert out["nn_idx"] is not None and np.array_equal(out["nn_idx"], nn_i) and np.array_equal(out["nn_dist2"], nn_d)
    assert nb.novelty_from_lists(nn_d, nn_i, self_d, self_i, [256], D, duplicate_rms=1.01)["duplicates"] == 0.75
    assert nb.novelty_from_lists(nn_d, nn_i, self_d, self_i, [256], D, duplicate_rms=0.0)["duplicates"] == 0.0
    with pytest.raises(ValueError):
        nb.novelty_from_lists(nn_d, nn_i[:, :2], self_d, self_i, [256], D)
    # the nearest OTHER row from lists searched without exclusion
    d = np.array([[0, 9], [0, 0], [0, 0], [0, 4]])
    i = np.array([[5, 2], [3, 6], [1, 2], [0, 8]])                     # rows 5, 6, 9, 8 of their set
    od, oi = nb.nearest_other(d, i, np.array([5, 6, 9, 8]))
    assert od.tolist() == [9, 0, 0, 0] and oi.tolist() == [2, 3, 1, 0]
    with pytest.raises(ValueError):
        nb.nearest_other(d[:, :1], i[:, :1], np.arange(4))


def test_precision_and_recall_reduce_hand_made_tables_to_the_right_shares():
    from mulan_amd import neighbours as nb
    assert nb.shares_from_covered([1, 0, 0, 1], [True, True, False]) == (0.5, 2 / 3)
    assert nb.shares_from_covered(np.zeros(3, np.uint8), np.ones(2, bool)) == (0.0, 1.0)
    with pytest.raises(ValueError):
        nb.shares_from_covered([], [1])
    lists = np.array([[1, 4, 9], [2, 2, 7]], dtype=np.int32)
    assert nb.radii_from_lists(lists, 2).tolist() == [4, 2] and nb.radii_from_lists(lists, 2).dtype == np.int32
    with pytest.raises(ValueError, match="fewer than"):
        nb.radii_from_lists(np.array([[1, no.EMPTY_D]], dtype=np.int32), 2)
    # a hand-made distance table: 3 samples x 4 real images, radii of both sets given
    table = np.array([[5, 9, 9, 20], [30, 30, 30, 30], [11, 2, 50, 50]])
    rad_real, rad_samp = np.array([4, 9, 8, 19]), np.array([5, 29, 1])
    cs = no.covered(None, None, rad_real, table=table)
    cr = no.covered(None, None, rad_samp, table=table.T)
    assert cs.tolist() == [True, False, True] and cr.tolist() == [True, False, False, False]
    assert nb.shares_from_covered(cs, cr) == (2 / 3, 0.25)


# ------------------------------------------------------------------------------------------------ the walk in chunks
def _stand_in(monkeypatch, calls):
    """ops.knn_u8 answered by the oracle on CPU tensors: what nearest / novelty / precision_recall do around the kernel"""
    from mulan_amd import ops

    def fake(q, r, k, idx_base=0, self_offset=-1, out=None, radius2=None, covered=None, splits=0):
        ops.knn_check(q, r, k, idx_base, self_offset, out, radius2, covered, splits)
        calls.append((tuple(q.shape), tuple(r.shape), k, idx_base, self_offset))
        d, i = no.knn(q.numpy(), r.numpy(), k, idx_base, self_offset)
        if out is not None:
            d, i = no.merge((out[0].numpy(), out[1].numpy()), (d, i), k)
            out[0].copy_(torch.from_numpy(d))
            out[1].copy_(torch.from_numpy(i))
            d, i = out
        else:
            d, i = torch.from_numpy(d), torch.from_numpy(i)
        if radius2 is None:
            return d, i
        c = torch.from_numpy(no.covered(q.numpy(), r.numpy(), radius2.numpy(), idx_base, self_offset).astype(np.uint8))
        covered |= c
        return d, i, covered
    monkeypatch.setattr(ops, "knn_u8", fake)


def small_sets(S=12, T=30, D=64, seed=3):
    rng = np.random.default_rng(seed)
    train = rng.integers(100, 110, (T, D)).astype(np.uint8)
    samples = rng.integers(100, 110, (S, D)).astype(np.uint8)
    samples[:3] = train[[4, 4, 17]]             # copies (two of one image: duplicates of one another as well)
    samples[3] = train[9]
    samples[3, 0] += 1                          # one level off
    return samples, train


def test_nearest_walks_the_reference_in_chunks_and_equals_one_call(monkeypatch):
    from mulan_amd import neighbours as nb
    calls = []
    _stand_in(monkeypatch, calls)
    samples, train = small_sets()
    want = no.knn(samples, train, 5)
    for chunk in (7, 30, 1000):
        calls.clear()
        d, i = nb.nearest(samples, train, 5, chunk=chunk, device="cpu")
        assert np.array_equal(d, want[0]) and np.array_equal(i, want[1]) and d.dtype == np.int32
        assert [c[3] for c in calls] == list(range(0, 30, chunk)) and all(c[4] == -1 for c in calls)
    d, i = nb.nearest(torch.from_numpy(train), train, 2, exclude_self=True, chunk=8, device="cpu")
    want = no.knn(train, train, 2, self_offset=0)
    assert np.array_equal(d, want[0]) and np.array_equal(i, want[1]) and all(c[4] == 0 for c in calls[-4:])
    rad = np.full(30, 40, dtype=np.int32)
    d, i, c = nb.nearest(samples, train, 1, radius2=rad, chunk=11, device="cpu")
    assert c.dtype == bool and np.array_equal(c, no.covered(samples, train, rad))
    d, i = nb.nearest(samples[:, :64].reshape(12, 64), train[:3], 5, device="cpu")          # fewer references than k
    assert (d[:, 3:] == no.EMPTY_D).all() and (i[:, 3:] == -1).all()


def test_novelty_and_precision_recall_equal_the_oracle_over_the_stand_in(monkeypatch):
    from mulan_amd import neighbours as nb
    _stand_in(monkeypatch, [])
    samples, train = small_sets()
    res = nb.novelty(samples, train, k=3, duplicate_rms=0.5, yardstick=10, seed=1, chunk=9, device="cpu")
    want = no.novelty(samples, train, 3, 0.5, res["train_subset"])
    for key in ("nn_dist2", "nn_idx", "nn_rms", "self_dist2", "self_idx", "self_rms", "train_self_rms"):
        assert np.array_equal(res[key], want[key]), key
    assert res["duplicates"] == want["duplicates"] == 2 / 12 and res["duplicate_rms"] == 0.5
    assert res["nn_dist2"][:4, 0].tolist() == [0, 0, 0, 1] and res["nn_idx"][:4, 0].tolist() == [4, 4, 17, 9]
    assert res["self_idx"][:2].tolist() == [1, 0]
    assert len(res["train_subset"]) == 10 and len(set(res["train_subset"].tolist())) == 10
    assert np.array_equal(res["train_subset"], nb.novelty(samples, train, k=3, yardstick=10, seed=1, device="cpu")["train_subset"])
    pr = nb.precision_recall(samples, train, k=2, chunk=13, device="cpu")
    p, r, rad_real, rad_samp = no.precision_recall(samples, train, 2)
    assert (pr["precision"], pr["recall"]) == (p, r) and pr["k"] == 2
    assert np.array_equal(pr["radius2_real"], rad_real) and np.array_equal(pr["radius2_samples"], rad_samp)
    assert "PIXEL SPACE" in nb.precision_recall.__doc__ and "NOT comparable" in nb.precision_recall.__doc__


def test_notebook_utils_reexports_the_module_objects():
    from ldm import notebook_utils as nu
    from mulan_amd import neighbours as nb
    assert nu.nearest_neighbours is nb.nearest and nu.sample_novelty is nb.novelty
    assert nu.precision_recall is nb.precision_recall and nu.plot_neighbours is nb.plot_neighbours


def test_plot_draws_a_sample_beside_its_neighbours(monkeypatch):
    pytest.importorskip("matplotlib")
    import matplotlib
    matplotlib.use("Agg")
    import matplotlib.pyplot as plt
    from mulan_amd import neighbours as nb
    _stand_in(monkeypatch, [])
    rng = np.random.default_rng(0)
    train = rng.integers(0, 256, (6, 32, 32, 3)).astype(np.uint8)
    samples = train[[2, 5, 0]].copy()
    res = nb.novelty(samples, train, k=2, device="cpu")
    fig = nb.plot_neighbours(samples, train, res, rows=2)
    assert len(fig.axes) == 2 * 3
    plt.close(fig)


# ------------------------------------------------------------------------------------------------ the command line
def _args(tmp_path, *more, reference=None):
    return [f"--samples={tmp_path / 's.npz'}", f"--reference={reference or 'npz:' + str(tmp_path / 't.npz')}",
            f"--out={tmp_path / 'n.npz'}", *more]


def test_cli_flag_parsing(tmp_path, monkeypatch):
    from ldm import neighbours as cli
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    with pytest.raises(SystemExit, match="no file"):
        cli.parse_flags(_args(tmp_path))
    np.savez(tmp_path / "s.npz", images=np.zeros((2, 32, 32, 3), np.uint8))
    f = cli.parse_flags(_args(tmp_path))
    assert (f.k, f.precision_recall, f.pr_k, f.max_reference, f.keep, f.duplicate_rms) == (5, False, 3, 0, 16, 1.0)
    f = cli.parse_flags(_args(tmp_path, "--k", "7", "--precision_recall", "--pr_k=4", "--max_reference", "100", "--keep=3"))
    assert (f.k, f.precision_recall, f.pr_k, f.max_reference, f.keep) == (7, True, 4, 100, 3)
    assert cli.parse_flags(_args(tmp_path, reference="cifar10")).reference == "cifar10"
    for more, match in ((["--k=0"], "--k"), (["--k=17"], "--k"), (["--pr_k=0"], "--pr_k"), (["--keep=-1"], "--keep"),
                        (["--duplicate_rms=-1"], "--duplicate_rms"), (["--chunk=0"], "--chunk")):
        with pytest.raises(SystemExit, match=match):
            cli.parse_flags(_args(tmp_path, *more))
    with pytest.raises(SystemExit, match="synthetic has no fixed set"):
        cli.parse_flags(_args(tmp_path, reference="synthetic"))
    with pytest.raises(SystemExit, match="--reference"):
        cli.parse_flags(_args(tmp_path, reference="mnist"))
    with pytest.raises(SystemExit, match=".npz"):
        cli.parse_flags(_args(tmp_path)[:2] + ["--out=n.txt"])
    with pytest.raises(SystemExit, match="required"):
        cli.parse_flags(_args(tmp_path)[:2])
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(SystemExit, match="one process"):
        cli.parse_flags(_args(tmp_path))


def test_cli_writes_the_documented_keys_over_the_stand_in(tmp_path, monkeypatch):
    from ldm import neighbours as cli
    from mulan_amd import neighbours as nb
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    _stand_in(monkeypatch, [])
    monkeypatch.setattr(nb.torch.cuda, "current_device", lambda: 0)
    real_nearest = nb.nearest
    monkeypatch.setattr(nb, "nearest", lambda *a, **kw: real_nearest(*a, **{**kw, "device": "cpu"}))
    rng = np.random.default_rng(5)
    train = rng.integers(0, 256, (9, 32, 32, 3)).astype(np.uint8)
    samples = rng.integers(0, 256, (5, 32, 32, 3)).astype(np.uint8)
    samples[3] = train[6]
    np.savez(tmp_path / "s.npz", images=samples)
    np.savez(tmp_path / "t.npz", images=train)
    assert cli.main(_args(tmp_path, "--k=2", "--precision_recall", "--pr_k=2", "--keep=2", "--max_reference=8")) == 0
    with np.load(tmp_path / "n.npz") as f:
        assert sorted(f.files) == sorted(cli.NOVELTY_KEYS + cli.PR_KEYS + cli.KEPT_KEYS + ("settings",))
        assert f["nn_idx"].shape == (5, 2) and f["nn_idx"][3, 0] == 6 and f["nn_dist2"][3, 0] == 0
        assert f["kept"][0] == 3 and np.array_equal(f["kept_samples"][0], samples[3])
        assert f["kept_neighbours"].shape == (2, 2, 32, 32, 3) and np.array_equal(f["kept_neighbours"][0, 0], train[6])
        want = no.precision_recall(samples.reshape(5, -1), train[:8].reshape(8, -1), 2)
        assert (float(f["precision"]), float(f["recall"])) == want[:2]
        s = json.loads(str(f["settings"]))
        assert s["n_reference"] == 8 and s["n_samples"] == 5 and s["k"] == 2 and s["keep"] == 2 and s["pr_k"] == 2
    assert cli.main(_args(tmp_path, "--keep=0")) == 0
    with np.load(tmp_path / "n.npz") as f:
        assert "precision" not in f.files and f["kept"].shape == (0,) and f["nn_idx"].shape == (5, 5)
