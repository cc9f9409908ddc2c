"""mulan_knn_u8 on the MI355X against the brute-force oracle (tests/neighbours_oracle.py): every comparison is integer
equality, no tolerance anywhere.  T = 128 queries and U = 128 references per tile, C = 64 bytes per K-chunk
(neighbours.hip); the shapes are the smallest that reach each loop's edges."""
import json

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import neighbours_oracle as no

T, U, C = 128, 128, 64


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def run(q, r, k, **kw):
    from mulan_amd import ops
    out = ops.knn_u8(dev(q), dev(r), k, **kw)
    torch.cuda.synchronize()
    return tuple(o.cpu().numpy() for o in out)


def same(got, want):
    assert got[0].dtype == np.int32 and got[1].dtype == np.int32
    bad = np.flatnonzero((got[0] != want[0]).any(1) | (got[1] != want[1]).any(1))
    assert bad.size == 0, (bad[:5], got[0][bad[:2]], want[0][bad[:2]], got[1][bad[:2]], want[1][bad[:2]])


def rand(rng, n, D, lo=0, hi=256):
    return rng.integers(lo, hi, (n, D)).astype(np.uint8)


def test_t1_lane_map_of_the_int8_operands():
    """asymmetric one-hot rows: d2(i, j) = 10, or 4 where i == 2 j + 1 -- a transposed or permuted operand map moves the 4s"""
    q = np.full((32, 64), 128, dtype=np.uint8)
    r = np.full((32, 64), 128, dtype=np.uint8)
    q[np.arange(32), np.arange(32)] = 129
    r[np.arange(32), 2 * np.arange(32) + 1] = 131
    table = no.dist2_table(q, r)
    assert all(table[i, j] == (4 if i == 2 * j + 1 else 10) for i in range(32) for j in range(32))
    same(run(q, r, 5), no.knn(q, r, 5, table=table))
    same(run(r, q, 5), no.knn(r, q, 5, table=table.T))
    rng = np.random.default_rng(1)
    q, r = rand(rng, 32, 64), rand(rng, 32, 64)
    same(run(q, r, 5), no.knn(q, r, 5))


@pytest.fixture(scope="module")
def edge_tables():
    rng = np.random.default_rng(2)
    out = {}
    for Q, N in ((1, 1), (T + 1, 2 * U + 1), (T - 1, U - 1)):
        for D in (64, C + 64, 3072):
            q, r = rand(rng, Q, D), rand(rng, N, D)
            out[Q, N, D] = (q, r, no.dist2_table(q, r))
    return out


@pytest.mark.parametrize("k", (1, 5, 16))
@pytest.mark.parametrize("D", (64, C + 64, 3072))
@pytest.mark.parametrize("QN", ((1, 1), (T + 1, 2 * U + 1), (T - 1, U - 1)))
def test_t2_edges_of_every_loop(edge_tables, QN, D, k):
    q, r, table = edge_tables[QN[0], QN[1], D]
    same(run(q, r, k), no.knn(q, r, k, table=table))


def test_t3_fewer_references_than_k():
    rng = np.random.default_rng(3)
    q, r = rand(rng, 5, 64), rand(rng, 3, 64)
    got = run(q, r, 5)
    same(got, no.knn(q, r, 5))
    assert (got[0][:, 3:] == 2 ** 31 - 1).all() and (got[1][:, 3:] == -1).all() and (got[1][:, :3] >= 0).all()
    got = run(q, r, 5, idx_base=4, self_offset=5)                  # query i loses reference i + 1
    same(got, no.knn(q, r, 5, idx_base=4, self_offset=5))
    assert (got[1][:2, 2:] == -1).all() and (got[1][2:, 3:] == -1).all() and (got[1][2:, 2] >= 0).all()


def test_t4_ties_go_to_the_smaller_index_and_the_largest_distance_fits():
    rng = np.random.default_rng(4)
    N = 2 * U + 5
    r = rand(rng, N, 128, 0, 3)                                    # three grey levels: distances tie all over
    for j in (U - 1, U, N - 1):
        r[j] = r[0]
    q = np.concatenate([r[:1], rand(rng, 6, 128, 0, 3)])
    got = run(q, r, 5)
    same(got, no.knn(q, r, 5))
    assert got[1][0, :4].tolist() == [0, U - 1, U, N - 1] and got[0][0, :4].tolist() == [0, 0, 0, 0]
    same(run(q, r, 16), no.knn(q, r, 16))
    for D in (3072, 16384):
        q, r = np.zeros((3, D), dtype=np.uint8), np.full((U + 2, D), 255, dtype=np.uint8)
        got = run(q, r, 2)
        assert (got[0] == D * 255 ** 2).all() and (got[1] == np.array([0, 1])).all()


def test_t5_the_answer_does_not_depend_on_the_slices():
    rng = np.random.default_rng(5)
    q, r = rand(rng, T + 1, 128, 0, 8), rand(rng, 5 * U + 3, 128, 0, 8)
    table = no.dist2_table(q, r)
    rad = np.full(len(r), int(np.median(table.min(1))), dtype=np.int32)     # about half of the queries are inside a ball
    outs = [run(q, r, 5, splits=s, radius2=dev(rad)) for s in (1, 2, 7, 0)]
    for o in outs[1:]:
        assert all(a.tobytes() == b.tobytes() for a, b in zip(o, outs[0]))
    same(outs[0][:2], no.knn(q, r, 5, table=table))
    assert np.array_equal(outs[0][2].astype(bool), no.covered(q, r, rad, table=table))
    assert 0 < outs[0][2].sum() < len(q)


def test_t6_chunks_accumulated_equal_one_call():
    from mulan_amd import ops
    rng = np.random.default_rng(6)
    q, r = rand(rng, 70, 192, 0, 6), rand(rng, 300, 192, 0, 6)
    k = 7
    dist2 = torch.full((70, k), 2 ** 31 - 1, dtype=torch.int32, device="cuda")
    idx = torch.full((70, k), -1, dtype=torch.int32, device="cuda")
    qd = dev(q)
    for lo, hi in ((0, 100), (100, 230), (230, 300)):
        out = ops.knn_u8(qd, dev(r[lo:hi]), k, idx_base=lo, out=(dist2, idx))
        assert out[0] is dist2 and out[1] is idx
    torch.cuda.synchronize()
    whole = run(q, r, k)
    same((dist2.cpu().numpy(), idx.cpu().numpy()), whole)
    same(whole, no.knn(q, r, k))
    # the chunks in another order give the same lists
    dist2.fill_(2 ** 31 - 1)
    idx.fill_(-1)
    for lo, hi in ((230, 300), (0, 100), (100, 230)):
        ops.knn_u8(qd, dev(r[lo:hi]), k, idx_base=lo, out=(dist2, idx), splits=3)
    same((dist2.cpu().numpy(), idx.cpu().numpy()), whole)


def test_t7_a_set_against_itself():
    rng = np.random.default_rng(7)
    r = rand(rng, 200, 64)
    r[150] = r[3]
    r[199] = r[3]
    r[130] = r[129]
    got = run(r, r, 3, self_offset=0)
    same(got, no.knn(r, r, 3, self_offset=0))
    assert (got[1] != np.arange(200)[:, None]).all()
    assert got[1][3, :2].tolist() == [150, 199] and got[0][3, :2].tolist() == [0, 0]
    assert got[1][150, :2].tolist() == [3, 199] and got[1][129, 0] == 130 and got[0][130, 0] == 0
    # the second half of the set as queries: self_offset shifts the excluded pair
    got = run(r[100:], r, 3, self_offset=100)
    same(got, no.knn(r[100:], r, 3, self_offset=100))
    assert (got[1] != 100 + np.arange(100)[:, None]).all()


def test_t8_radius_mode_at_the_radius_and_one_above():
    from mulan_amd import ops
    rng = np.random.default_rng(8)
    q, r = rand(rng, 40, 64, 0, 16), rand(rng, U + 72, 64, 0, 16)
    table = no.dist2_table(q, r)
    rad = (table.min(0) - 1).astype(np.int32)                      # every nearest pair sits at radius2 + 1: outside
    at = [5, U - 1, U, U + 71]                                     # these at radius2 exactly: inside, either side of a tile
    rad[at] += 1
    want = no.covered(q, r, rad, table=table)
    assert (table == rad[None] + 1).any() and all((table[:, j] == rad[j]).any() for j in at) and 0 < want.sum() < 40
    got = run(q, r, 2, radius2=dev(rad))
    same(got[:2], no.knn(q, r, 2, table=table))
    assert got[2].dtype == np.uint8 and np.array_equal(got[2].astype(bool), want)
    # accumulate ORs: the two tiles as two calls, each alone covers fewer
    qd = dev(q)
    first = ops.knn_u8(qd, dev(r[:U]), 2, radius2=dev(rad[:U]))
    assert np.array_equal(first[2].cpu().numpy().astype(bool), no.covered(q, r[:U], rad[:U]))
    both = ops.knn_u8(qd, dev(r[U:]), 2, idx_base=U, out=first[:2], radius2=dev(rad[U:]), covered=first[2])
    assert both[2] is first[2] and np.array_equal(both[2].cpu().numpy().astype(bool), want)
    assert want.sum() > no.covered(q, r[:U], rad[:U]).sum() > 0
    same((both[0].cpu().numpy(), both[1].cpu().numpy()), got[:2])
    # the excluded pair does not cover: a set against itself with radii 0 is covered only where a duplicate exists
    r[U + 3] = r[7]
    got = run(r, r, 1, self_offset=0, radius2=dev(np.zeros(len(r), dtype=np.int32)))
    assert np.flatnonzero(got[2]).tolist() == [7, U + 3]


def test_refusals_at_the_boundary_come_before_any_launch():
    from mulan_amd import lib
    L = lib.load()
    q = torch.zeros((4, 128), dtype=torch.uint8, device="cuda")
    d = torch.full((4, 3), 5, dtype=torch.int32, device="cuda")
    i = torch.full((4, 3), 5, dtype=torch.int32, device="cuda")
    ws = torch.zeros(L.mulan_knn_u8_workspace(4, 3, 0) // 8 + 1, dtype=torch.int64, device="cuda")
    cov = torch.zeros(4, dtype=torch.uint8, device="cuda")
    rad = torch.zeros(4, dtype=torch.int32, device="cuda")
    good = dict(q=q.data_ptr(), r=q.data_ptr(), Q=4, N=4, D=128, k=3, idx_base=0, self_offset=-1, accumulate=0, splits=0,
                radius2=None, covered=None, dist2=d.data_ptr(), idx=i.data_ptr(), ws=ws.data_ptr())
    bad = [dict(D=96), dict(D=32), dict(D=16448), dict(k=0), dict(k=17), dict(Q=-1), dict(N=-1), dict(Q=0), dict(q=None),
           dict(r=None), dict(dist2=None), dict(idx=None), dict(ws=None), dict(covered=cov.data_ptr()),
           dict(radius2=rad.data_ptr()), dict(accumulate=2), dict(splits=-1), dict(idx_base=-1), dict(self_offset=-2),
           dict(q=q.data_ptr() + 1)]
    for change in bad:
        a = {**good, **change}
        assert L.mulan_knn_u8(*a.values(), lib.stream()) == 1, change          # hipErrorInvalidValue
    assert L.mulan_knn_u8_workspace(4, 0, 0) == 0 and L.mulan_knn_u8_workspace(-1, 3, 0) == 0
    torch.cuda.synchronize()
    assert (d == 5).all() and (i == 5).all()
    assert L.mulan_knn_u8(*good.values(), lib.stream()) == 0
    torch.cuda.synchronize()
    assert (d == 0).all() and (i.cpu() == torch.tensor([0, 1, 2], dtype=torch.int32)).all()


def test_t9_whole_path_and_the_command_line(tmp_path, monkeypatch):
    from ldm import neighbours as cli
    from mulan_amd import neighbours as nb
    rng = np.random.default_rng(9)
    train = rng.integers(0, 256, (1000, 32, 32, 3)).astype(np.uint8)
    # samples around a common image, so that the balls of the two sets overlap in part
    base = rng.integers(0, 256, (1, 32, 32, 3))
    samples = np.clip(base + rng.integers(-40, 41, (300, 32, 32, 3)), 0, 255).astype(np.uint8)
    train[500:800] = np.clip(base + rng.integers(-40, 41, (300, 32, 32, 3)), 0, 255).astype(np.uint8)
    planted = np.arange(0, 300, 15)                                 # 20 samples, from 20 training rows
    source = rng.choice(1000, 20, replace=False)
    samples[planted] = train[source]
    for n in range(10, 20):                                         # half of them one grey level off, up or down
        s = samples[planted[n]].astype(np.int16)
        s += np.where(s < 128, 1, -1).astype(np.int16) * rng.integers(0, 2, s.shape, dtype=np.int16)
        samples[planted[n]] = s.astype(np.uint8)
    samples[7] = samples[planted[2]]                                # and two samples that copy one another
    tab = no.tables(samples.reshape(300, -1), train.reshape(1000, -1))
    res = nb.novelty(samples, train, k=5, chunk=400)
    want = no.novelty(samples, train, 5, 1.0, res["train_subset"], tab)
    for key in ("nn_dist2", "nn_idx", "nn_rms", "self_dist2", "self_idx", "self_rms", "train_self_rms"):
        assert np.array_equal(res[key], want[key]), key
    assert np.array_equal(res["nn_idx"][planted, 0], source) and (res["nn_dist2"][planted[:10], 0] == 0).all()
    assert (res["nn_rms"][planted] <= 1.0).all() and res["nn_rms"][np.setdiff1d(np.arange(300), list(planted) + [7])].min() > 10
    assert res["duplicates"] == want["duplicates"] == 2 / 300
    pr = nb.precision_recall(samples, train, k=3, chunk=400)
    p, r, rad_real, rad_samp = no.precision_recall(samples, train, 3, tab)
    print(f"precision {p} recall {r} duplicates {res['duplicates']}")
    assert (pr["precision"], pr["recall"]) == (p, r) and 0 < p <= 1 and 0 < r < 1
    assert np.array_equal(pr["radius2_real"], rad_real) and np.array_equal(pr["radius2_samples"], rad_samp)
    # the command line gives the same through .npz files
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    np.savez(tmp_path / "s.npz", images=samples)
    np.savez(tmp_path / "t.npz", images=train)
    assert cli.main([f"--samples={tmp_path / 's.npz'}", f"--reference=npz:{tmp_path / 't.npz'}", f"--out={tmp_path / 'n.npz'}",
                     "--chunk=400", "--precision_recall", "--keep=4"]) == 0
    with np.load(tmp_path / "n.npz") as f:
        for key in cli.NOVELTY_KEYS:
            assert np.array_equal(f[key], np.asarray(res[key])), key
        assert (float(f["precision"]), float(f["recall"])) == (p, r)
        assert np.array_equal(f["covered_samples"], pr["covered_samples"])
        assert set(f["kept"].tolist()) <= set(planted[:10].tolist()) | {7}
        assert np.array_equal(f["kept_neighbours"][:, 0], f["kept_samples"])
        assert json.loads(str(f["settings"]))["n_reference"] == 1000
