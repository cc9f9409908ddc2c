"""Brute-force numpy statement of mulan_knn_u8 and of what mulan_amd.neighbours reads off it.  No norms, no matrix
product: differences in int64, summed per pair, a block of reference rows at a time; then np.argsort(kind="stable") on the distance,
which keeps equal distances in index order -- the smaller-index tie rule.  Every comparison against this file is exact."""
import numpy as np

EMPTY_D, EMPTY_I = 2 ** 31 - 1, -1


def dist2_table(q, r, block=32):
    """int64 [Q, N]: sum_c (q[i, c] - r[j, c])^2, the differences taken in int64, `block` reference rows at a time (a
    block of differences stays in cache).  `r is q`: only the pairs i <= j are computed, the rest mirrored."""
    same = r is q
    q = np.asarray(q).reshape(len(q), -1).astype(np.int64)
    r = q if same else np.asarray(r).reshape(len(r), -1).astype(np.int64)
    out = np.zeros((len(q), len(r)), dtype=np.int64)
    buf = np.empty((block, q.shape[1]), dtype=np.int64)
    for lo in range(0, len(r), block):
        blk = r[lo:lo + block]
        diff = buf[:len(blk)]
        for i in range(min(len(q), lo + len(blk)) if same else len(q)):
            np.subtract(blk, q[i], out=diff)
            out[i, lo:lo + len(blk)] = np.einsum("jc,jc->j", diff, diff)
    return np.triu(out) + np.triu(out, 1).T if same else out


def qualifies(Q, N, idx_base=0, self_offset=-1):
    """bool [Q, N]: pair (i, j) takes part unless j + idx_base == i + self_offset (self_offset >= 0)"""
    ok = np.ones((Q, N), dtype=bool)
    if self_offset >= 0:
        i, j = np.arange(Q)[:, None], np.arange(N)[None, :]
        ok &= (j + idx_base) != (i + self_offset)
    return ok


def knn(q, r, k, idx_base=0, self_offset=-1, table=None):
    """(dist2, idx) int32 [Q, k]: ascending, ties to the smaller index, (EMPTY_D, EMPTY_I) where fewer than k qualify"""
    d = dist2_table(q, r) if table is None else np.asarray(table, dtype=np.int64)
    Q, N = d.shape
    ok = qualifies(Q, N, idx_base, self_offset)
    dist2 = np.full((Q, k), EMPTY_D, dtype=np.int32)
    idx = np.full((Q, k), EMPTY_I, dtype=np.int32)
    for i in range(Q):
        js = np.flatnonzero(ok[i])
        order = js[np.argsort(d[i, js], kind="stable")][:k]
        dist2[i, :len(order)] = d[i, order]
        idx[i, :len(order)] = order + idx_base
    return dist2, idx


def merge(lists_a, lists_b, k):
    """the accumulate rule: the k smallest (dist2, idx) pairs of two list pairs, rows apart"""
    d = np.concatenate([lists_a[0], lists_b[0]], axis=1).astype(np.int64)
    i = np.concatenate([lists_a[1], lists_b[1]], axis=1).astype(np.int64)
    key = d * 2 ** 32 + (i & 0xffffffff)          # the empty slot (EMPTY_D, -1) is the largest key
    order = np.argsort(key, axis=1, kind="stable")[:, :k]
    return np.take_along_axis(d, order, 1).astype(np.int32), np.take_along_axis(i, order, 1).astype(np.int32)


def covered(q, r, radius2, idx_base=0, self_offset=-1, table=None):
    """bool [Q]: some qualifying j has d2(i, j) <= radius2[j]"""
    d = dist2_table(q, r) if table is None else np.asarray(table, dtype=np.int64)
    ok = qualifies(*d.shape, idx_base, self_offset)
    return ((d <= np.asarray(radius2, dtype=np.int64)[None, :]) & ok).any(1)


def tables(samples, train):
    """the three distance tables the whole path needs, each computed once: st [S, T], ss [S, S], tt [T, T]"""
    return dict(st=dist2_table(samples, train), ss=dist2_table(samples, samples), tt=dist2_table(train, train))


def novelty(samples, train, k, duplicate_rms, subset, tab=None):
    """the figures of mulan_amd.neighbours.novelty, restated"""
    tab = tab or tables(samples, train)
    D = int(np.prod(samples.shape[1:]))
    nn_d, nn_i = knn(None, None, k, table=tab["st"])
    self_d, self_i = knn(None, None, 1, self_offset=0, table=tab["ss"])
    t = tab["tt"][subset].astype(np.float64)
    t[np.arange(len(subset)), subset] = np.inf
    self_rms = np.sqrt(self_d[:, 0] / D)
    return dict(nn_dist2=nn_d, nn_idx=nn_i, nn_rms=np.sqrt(nn_d[:, 0] / D), self_dist2=self_d[:, 0], self_idx=self_i[:, 0],
                self_rms=self_rms, duplicates=float((self_rms <= duplicate_rms).mean()),
                train_self_rms=np.sqrt(t.min(1) / D))


def precision_recall(samples, real, k, tab=None):
    """(precision, recall, radius2_real, radius2_samples)"""
    tab = tab or tables(samples, real)
    rad_real = knn(None, None, k, self_offset=0, table=tab["tt"])[0][:, k - 1]
    rad_samp = knn(None, None, k, self_offset=0, table=tab["ss"])[0][:, k - 1]
    cs = covered(None, None, rad_real, table=tab["st"])
    cr = covered(None, None, rad_samp, table=tab["st"].T)
    return float(cs.mean()), float(cr.mean()), rad_real, rad_samp
