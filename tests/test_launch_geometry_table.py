"""CPU side of tests/test_gpu_launch_geometry.py: the stream helper (tests/stream_oracle.py) against the oracle's own use
of the generator, and the table of capped kernels against the sources."""
import glob
import os
import re

import numpy as np

from oracle import mulan_np as onp
from tests import stream_oracle as so
from tests import test_gpu_launch_geometry as geo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------ stream helper
def test_words_agree_with_the_oracles_dropout_mask():
    """onp.dropout_mask keeps element e where word e % 4 of Philox(seed, offset + e // 4) is below keep * 2^32: the same
    word order and counter law, through the helper"""
    seed, offset, shape = 0x1234ABCD5678, 5 << 34, (3, 8, 8, 20)
    n = int(np.prod(shape))
    for keep in (0.9, 0.5, 0.1):
        thr = np.uint32(np.float64(np.float32(keep)) * 4294967296.0)
        mask = onp.dropout_mask(shape, keep, seed, offset)
        assert np.array_equal(so.words(seed, offset, n) < thr, mask.reshape(-1))
        assert 0.5 * keep < mask.mean() < min(1.0, 1.5 * keep)
    # the Random123 known answer (tests/test_oracle_kat.py pins the generator; this pins the helper's word order to it)
    assert np.array_equal(so.words(0, 0, 4), onp.philox4x32_10(0, np.zeros(1, dtype=np.uint64))[0])


def test_slicing_is_self_consistent():
    seed, offset = 77, (1 << 40) + 9
    for n, k in ((1023, 100), (7, 1), (4096, 1023), (5, 0)):
        w = so.words(seed, offset, n)
        assert w.dtype == np.uint32 and w.shape == (n,)
        assert np.array_equal(w[4 * k:], so.words(seed, offset + k, n - 4 * k))
        for m in (1, 2, 3, n):
            assert np.array_equal(so.words(seed, offset, m), w[:m])
        assert np.array_equal(so.randn(seed, offset, n)[4 * k:], so.randn(seed, offset + k, n - 4 * k))
    assert not np.array_equal(so.words(seed, offset, 64), so.words(seed + 1, offset, 64))
    assert not np.array_equal(so.words(seed, offset, 64), so.words(seed, offset + 1, 64))


def test_variates_are_what_they_claim():
    n = 1 << 18
    w = so.words(3, 0, n)
    u = so.uniform24(w)
    assert u.dtype == np.float32 and u.min() >= 0 and u.max() < 1 and abs(u.mean() - 0.5) < 5e-3
    assert np.array_equal(u.astype(np.float64) * 2.0 ** 24, (w >> np.uint32(8)).astype(np.float64))
    r = so.rademacher(w)
    assert set(np.unique(r)) == {-1.0, 1.0} and np.array_equal(r > 0, w >= np.uint32(1 << 31))
    z = so.randn(3, 0, n)
    assert z.dtype == np.float64 and abs(z.mean()) < 1e-2 and abs(z.std() - 1) < 1e-2
    z32 = so.randn(3, 0, n, np.float32)
    assert z32.dtype == np.float32 and np.abs(z32 - z).max() < 1e-4
    g = so.gumbel_from_words(w, np.float64)
    assert np.isfinite(g).all() and abs(g.mean() - 0.5772156649) < 2e-2
    t = so.truncated_normal_from_words(w, -3.0, 3.0, np.float64)
    assert t.dtype == np.float64 and t.min() >= -3 and t.max() <= 3 and abs(t.mean()) < 1e-2
    # the largest 24-bit uniform: u + 2^-25 rounds to 1.0f; the Gumbel form stays below 1 and finite
    top = np.array([0xFFFFFF00, 0xFFFFFFFF, 0], dtype=np.uint32)
    assert so.open_uniform24(top)[0] == np.float32(1.0) and so.open_uniform24(top, below_one=True)[1] < 1
    assert np.isfinite(so.gumbel_from_words(top, np.float32)).all()
    assert so.randn_uniform32(top)[1] == np.float32(1.0) and so.randn_uniform32(top)[2] > 0


# ------------------------------------------------------------------------------------------------ the table
CAP = re.compile(r"\bnblocks\(|\bgrid_for\(|\bgrid_capped\(|\bblocks\s*>")
DEFN = re.compile(r"^(MULAN_API|static)\s[^;{]*?\b(\w+)\s*\(", re.M)


def _functions(text):
    """(exported?, name, body) of every function defined at column 0 as `MULAN_API ...` or `static ...`"""
    out = []
    for m in DEFN.finditer(text):
        start = text.find("{", m.end())
        semi = text.find(";", m.end())
        if start < 0 or (0 <= semi < start):
            continue                                        # a declaration
        depth, i = 0, start
        while True:
            depth += {"{": 1, "}": -1}.get(text[i], 0)
            if depth == 0:
                break
            i += 1
        out.append((m.group(1) == "MULAN_API", m.group(2), text[start:i + 1]))
    return out


def capped_entry_points():
    found = set()
    for path in sorted(glob.glob(os.path.join(ROOT, "mulan_amd", "csrc", "*.hip"))):
        with open(path) as f:
            fns = _functions(f.read())
        helpers = {name for exported, name, body in fns if not exported and CAP.search(body)}
        for exported, name, body in fns:
            if exported and (CAP.search(body) or any(re.search(r"\b%s\(" % h, body) for h in helpers)):
                found.add(name)
    return found


def test_every_capped_kernel_has_a_geometry_case():
    """an exported function whose launch goes through nblocks( / grid_for( / grid_capped( or an explicit `blocks >` cap
    (directly or through a static launcher) must be named in GEOMETRY_CASES with the test that crosses its cap"""
    found = capped_entry_points()
    assert {"mulan_adamw_ema_step_dyn", "mulan_randn", "mulan_noise", "mulan_axpby", "mulan_fast_sampler_step"} <= found
    assert found == set(geo.GEOMETRY_CASES), (sorted(found - set(geo.GEOMETRY_CASES)),
                                              sorted(set(geo.GEOMETRY_CASES) - found))
    for entry, test in geo.GEOMETRY_CASES.items():
        assert callable(getattr(geo, test, None)), (entry, test)
