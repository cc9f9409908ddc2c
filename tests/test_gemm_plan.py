"""CPU side of tests/test_gpu_gemm.py: the host restatement of mulan_gemm's launch plan (tests/gemm_plan.py) against the
built library's mulan_gemm_workspace and against the text of mulan_amd/csrc/gemm.hip, and the tile and split count that
every GPU case is written for against the port."""
import ctypes
import itertools
import os
import re

import pytest

from tests import gemm_plan as gp
from tests import test_gpu_gemm as gg
from tests import test_gpu_kernels as gk

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GEMM_SRC = os.path.join(ROOT, "mulan_amd", "csrc", "gemm.hip")


@pytest.fixture(scope="module")
def workspace_fn():
    from mulan_amd import build
    h = ctypes.CDLL(build.build_library())
    fn = h.mulan_gemm_workspace
    fn.argtypes = [ctypes.c_int] * 4
    fn.restype = ctypes.c_size_t
    return fn


def _params(test):
    """the argument tuples of a test's first-listed pytest.mark.parametrize"""
    marks = [m for m in test.pytestmark if m.name == "parametrize"]
    return [tuple(v) for v in marks[-1].args[1]]


def existing_gemm_shapes():
    shapes = [(M, N, K, 1) for M, N, K in _params(gk.test_gemm_exact)]
    shapes += [(M, N, K, 1) for M, N, K, _ in _params(gk.test_gemm_split_k_exact)]
    shapes += [(1024, 1024, 128, 3), (1024, 128, 1024, 3)]          # test_gemm_batched_attention_shapes
    assert (4096, 128, 256, 1) in shapes and (128, 3072, 3072, 1) in shapes
    return shapes


def boundary_sweep():
    """every branch of plan_ksplit from both sides: K 255/256, 1023/1024, 4095/4096; 64 x 64 tiles 8/9, 127/128, 255/256;
    128 x 128 tiles 128/129 and 255/256; batch 1/2; shapes that just miss the big tile"""
    Ms = [1, 7, 64, 100, 128, 129, 512, 513, 576, 64 * 127, 64 * 128, 64 * 255, 64 * 256, 128 * 128, 128 * 129, 128 * 255,
          128 * 256]
    Ns = [1, 3, 32, 33, 64, 128, 200, 256]
    Ks = [1, 255, 256, 257, 500, 1023, 1024, 4095, 4096, 4100, 8192, 131072]
    return [(M, N, K, b) for M, N, K in itertools.product(Ms, Ns, Ks) for b in (1, 2)]


def test_port_agrees_with_the_librarys_workspace_size(workspace_fn):
    shapes = [c[:4] for c in gg.CASES] + existing_gemm_shapes() + boundary_sweep()
    split = 0
    for M, N, K, batch in shapes:
        s, kc = gp.plan_ksplit(M, N, K, batch)
        want = s * M * N * 4 if s > 1 else 0
        assert workspace_fn(M, N, K, batch) == want == gp.workspace_bytes(M, N, K, batch), (M, N, K, batch, s)
        if s > 1:
            split += 1
            assert batch == 1 and kc % 16 == 0 and (s - 1) * kc < K <= s * kc, (M, N, K, s, kc)
        else:
            assert kc == K
    assert 100 < split < len(shapes) - 100      # the sweep sees both outcomes many times over


def test_sweep_reaches_every_branch_boundary():
    """the sweep holds the pairs it claims: one side of each threshold splits differently from the other"""
    p = gp.plan_ksplit
    assert p(128, 128, 255, 1)[0] == 1 and p(128, 128, 256, 1)[0] == 4                  # K < 256
    assert p(576, 64, 1023, 1)[0] == 1 and p(576, 64, 1024, 1)[0] == 4                  # tiles > 8: K < 1024
    assert p(512, 64, 1023, 1)[0] > 1 and p(576, 64, 1023, 1)[0] == 1                   # tiles 8 / 9
    assert p(64 * 127, 64, 1024, 1)[0] > 1 and p(64 * 128, 64, 1024, 1)[0] == 1         # tiles 127 / 128
    assert p(64 * 255, 64, 4100, 1)[0] > 1 and p(64 * 256, 64, 4100, 1)[0] == 1         # 64-tiles 255 / 256, K >= 4096
    assert p(128 * 128, 128, 4096, 1)[0] == 2 and p(128 * 129, 128, 4096, 1)[0] == 1    # 128-tiles: 256 / tiles < 2 ...
    assert p(128 * 255, 128, 4096, 1)[0] == 1 and p(128 * 256, 128, 4096, 1)[0] == 1    # ... so 255 / 256 both run direct
    assert p(128, 128, 4095, 1) == (52, 80) and p(128, 128, 4096, 1) == (8, 512)        # K 4095 / 4096
    assert p(128, 128, 8192, 1)[0] > 1 and p(128, 128, 8192, 2)[0] == 1                 # batch 1 / 2
    sweep = set(boundary_sweep())
    for shape in [(128, 128, 255, 1), (128, 128, 256, 1), (576, 64, 1023, 1), (576, 64, 1024, 1), (512, 64, 1023, 1),
                  (64 * 127, 64, 1024, 1), (64 * 128, 64, 1024, 1), (64 * 255, 64, 4100, 1), (64 * 256, 64, 4100, 1),
                  (128 * 128, 128, 4096, 1), (128 * 129, 128, 4096, 1), (128 * 255, 128, 4096, 1), (128 * 256, 128, 4096, 1),
                  (128, 128, 4095, 1), (128, 128, 4096, 1), (128, 128, 8192, 1), (128, 128, 8192, 2)]:
        assert shape in sweep, shape


def tile_choice_in_source(text):
    """the three-way tile choice at the end of mulan_gemm, as written: the thresholds and the tile each branch launches"""
    body = text[text.index("MULAN_API int mulan_gemm("):]
    m = re.search(r"const long long tiles128 = \(long long\)\(\(M \+ 127\) / 128\) \* \(\(N \+ 127\) / 128\) \* batch;\s*"
                  r"if \(M >= (\d+) && N >= (\d+) && tiles128 >= (\d+)\) \{\s*launch<(\d+), (\d+), \d+, \d+>\(a,[^;]*;\s*"
                  r"\} else if \(N <= (\d+)\) \{\s*launch<(\d+), (\d+), \d+, \d+>\(a,[^;]*;\s*"
                  r"\} else \{\s*launch<(\d+), (\d+), \d+, \d+>\(a,", body)
    assert m, "the tile choice of mulan_gemm no longer reads as tests/gemm_plan.py restates it"
    g = [int(v) for v in m.groups()]
    return dict(big_min_m=g[0], big_min_n=g[1], big_min_tiles=g[2], big_tile="%dx%d" % (g[3], g[4]), thin_max_n=g[5],
                thin_tile="%dx%d" % (g[6], g[7]), else_tile="%dx%d" % (g[8], g[9]))


def test_tile_thresholds_are_the_sources():
    """a threshold that moves in gemm.hip fails here, instead of silently moving a GPU case onto another kernel"""
    with open(GEMM_SRC) as f:
        text = f.read()
    assert tile_choice_in_source(text) == dict(
        big_min_m=gp.BIG_MIN_M, big_min_n=gp.BIG_MIN_N, big_min_tiles=gp.BIG_MIN_TILES, big_tile=gp.T128,
        thin_max_n=gp.THIN_MAX_N, thin_tile=gp.T128x32, else_tile=gp.T64)
    # the split path's two tiles, and that a split returns before the direct choice
    m = re.search(r"if \(ksplit_big_tile\(M, N, K\)\) launch<(\d+), (\d+), \d+, \d+>\(a,[^;]*, s, stream\);\s*"
                  r"else launch<(\d+), (\d+), \d+, \d+>\(a,[^;]*, s, stream\);", text)
    assert m and [int(v) for v in m.groups()] == [128, 128, 64, 64]
    assert re.search(r"bool ksplit_big_tile\(int M, int N, int K\) \{ return K >= 4096 && M % 128 == 0 && N % 128 == 0; \}",
                     text)
    # the tile choice in numbers, from both sides of each threshold
    assert gp.direct_tile(1024, 1024, 3) == gp.T64 and gp.direct_tile(1024, 1024, 4) == gp.T128
    assert gp.direct_tile(127, 4096, 256) == gp.T64 and gp.direct_tile(4096, 127, 256) == gp.T64
    assert gp.direct_tile(128, 128, 255) == gp.T64 and gp.direct_tile(128, 128, 256) == gp.T128
    assert gp.direct_tile(4096, 32, 1) == gp.T128x32 and gp.direct_tile(4096, 33, 1) == gp.T64


def test_every_gpu_case_is_on_its_kernel():
    tiles = set()
    for M, N, K, batch, ws, tile, splits in gg.CASES:
        assert gp.plan(M, N, K, batch, ws)[:2] == (tile, splits), (M, N, K, batch, ws)
        tiles.add((tile, splits > 1))
    assert tiles == {(gp.T128, False), (gp.T128x32, False), (gp.T64, False), (gp.T128, True), (gp.T64, True)}
    # what the existing kernel tests leave out: no 128 x 128 direct launch
    assert all(gp.direct_tile(M, N, b) != gp.T128 for M, N, K, b in existing_gemm_shapes())
