"""tests/reduction_oracle.py without a device: the bars it derives hold for fp32 sums formed on the host in two orders
(so they are bars of the arithmetic, not of one kernel's tree), the float64-accumulation bar of colsum_kernel really
separates float64 from fp32 accumulation on the cancelling data, the builders are deterministic, the integers stay
exact in fp32, and the tables hold the cases they were written for."""
import numpy as np
import pytest
import torch

from tests import reduction_oracle as ro

DATASETS = list(ro.float_datasets())


def test_fp32_sums_in_two_orders_stay_inside_the_fp32_bound():
    """sequential np.float32 accumulation and np.sum in float32 (pairwise), for every cancelling data set of the GPU
    tables: |sum32 - ref| <= (n + 2) u sum |terms| -- the bound needs nothing a kernel computes"""
    worst = 0.0
    for name, terms, axis, _ in DATASETS:
        ref, bar = terms.sum(axis=axis), ro.fp32_bar(terms, axis)
        for order in (ro.sum32_sequential, ro.sum32_numpy):
            ratio = float((np.abs(order(terms, axis) - ref) / bar).max())
            worst = max(worst, ratio)
            assert ratio <= 1.0, (name, order.__name__, ratio)
    print("fp32 sums on the host: worst error / bar", worst)


def test_fp32_accumulation_misses_the_float64_bar():
    """on every cancelling data set a kernel that accumulates in float64 is held to, of 15 terms or more: both fp32
    orders miss f64_bar in some column (two cancelling terms add exactly in fp32, so the shortest segments cannot
    tell), a float64 sum rounded once to fp32 stays inside it"""
    seen = 0
    for name, terms, axis, acc in DATASETS:
        if acc != "f64":
            continue
        seg = terms.shape[axis]
        ref, sabs = terms.sum(axis=axis), np.abs(terms).sum(axis=axis)
        bar = ro.f64_bar(ref, seg, sabs)
        assert (np.abs(ro.f32(ref) - ref) <= bar).all(), name
        if seg < 15:
            continue
        seen += 1
        for order in (ro.sum32_sequential, ro.sum32_numpy):
            ratio = float((np.abs(order(terms, axis) - ref) / bar).max())
            print(name, order.__name__, "error / float64 bar", ratio)
            assert ratio > 1.0, (name, order.__name__, ratio)
    assert seen >= 20


def test_cancelling_data_cancels():
    for name, terms, axis, _ in DATASETS:
        if terms.shape[axis] < 15:
            continue
        r = np.abs(terms.sum(axis=axis)) / np.abs(terms).sum(axis=axis)
        assert 0.5 * ro.CANCEL < r.min() and r.max() < 2 * ro.CANCEL, (name, r.min(), r.max())


def test_two_stage_bar_sits_between_the_float64_and_the_fp32_bound():
    _, terms, _ = ro.colsum_data("floats", ro.RAW_NSEG, 2048, 3, 3, tag="raw")
    two = ro.two_stage_bar(terms)
    assert (two < ro.fp32_bar(terms, 1)).all()
    assert (two > ro.f64_bar(terms.sum(1), 2048, np.abs(terms).sum(1))).all()
    # fp32 partials of 512 rows, summed in float64 and rounded once: what the two launches of colsum_kernel do
    parts = ro.f32(terms.reshape(ro.RAW_NSEG, 4, 512, 3).sum(axis=2))
    assert (np.abs(ro.f32(parts.sum(axis=1)) - terms.sum(1)) <= two).all()


def test_builders_are_deterministic_and_fp32_valued():
    for build in (lambda: ro.colsum_data("floats", 3, 129, 68, 72), lambda: ro.colsum_data("ints", 3, 129, 68, 72),
                  lambda: ro.add_data("floats", 3, 20, 4), lambda: ro.delta_data("floats", 3, 128),
                  lambda: ro.softmax_rows("peak", 3, 252, ro.SOFTMAX_ALPHAS[1]), lambda: ro.temb_data(5, 130),
                  lambda: (ro.rowmean_data("floats", 5, 65),)):
        one, two = build(), build()
        for a, b in zip(one, two):
            assert np.array_equal(a, b, equal_nan=True)
            assert np.array_equal(a, ro.f32(a), equal_nan=True)
    assert not np.array_equal(ro.colsum_data("floats", 3, 129, 68, 72)[1], ro.colsum_data("floats", 3, 129, 68, 68)[1])


def test_integer_sums_are_exact_in_fp32():
    """|value| <= 2 (4 for a sum a + b, 4 for a product): no partial sum of the longest reduction of the tables reaches
    2^24, so every fp32 order gives the exact sum"""
    longest = max([seg for _, seg in ro.COLSUM_TABLE] + list(ro.RAW_SEGS) + [seg for seg, _ in ro.PAIR_TABLE]
                  + [row_len // ncols for ncols, row_len, _ in ro.ADD_COLSUM_TABLE] + [c for _, c in ro.ROWMEAN_TABLE]
                  + [C for _, C in ro.DELTA_TABLE])
    assert max(abs(ro.INT_LO), abs(ro.INT_HI - 1)) == 2
    assert 4 * (longest + 1) < 2 ** 24
    x = ro.ints(ro.rng_of("ints"), (longest, 7))
    assert set(np.unique(x)) == {-2.0, -1.0, 0.0, 1.0, 2.0}
    assert np.array_equal(ro.sum32_sequential(x, 0), x.sum(0)) and np.array_equal(ro.sum32_numpy(x, 0), x.sum(0))


def test_colsum_table_reaches_both_kernels_at_every_seg():
    table = ro.COLSUM_TABLE
    assert 40 <= len(table) <= 48 and len(set(table)) == len(table)
    for kernel, cfgs in (("scalar", ro.SCALAR_CFGS), ("vector", ro.VECTOR_CFGS)):
        assert {seg for cfg, seg in table if cfg.kernel == kernel} == set(ro.COLSUM_SEGS)
        for cfg in cfgs:
            assert {17, 129} <= {seg for c, seg in table if c == cfg}
            # the dispatch condition on aligned buffers, shifted by the offsets in floats
            assert ro.colsum_vec_dispatch(cfg.C, cfg.ld, 4096 + 4 * cfg.x_off, 8192 + 4 * cfg.out_off) == (kernel == "vector")
    assert {(c.C, c.ld) for c in ro.SCALAR_CFGS if not (c.x_off or c.out_off)} == {(1, 1), (3, 3), (5, 5), (130, 130), (3, 7), (64, 65)}
    assert {(c.C, c.ld) for c in ro.VECTOR_CFGS} == {(4, 4), (60, 60), (64, 64), (68, 68), (132, 132), (256, 256), (68, 72)}


def test_absmax_places_follow_the_kernel_loops():
    """12288 float4 never enter the unrolled loop (i + 3 * 4096 < 12288 fails for i = 0); one more float4 enters it once,
    for thread 0 of block 0 alone"""
    for row_len in (4, 1020, 16384, 16388, 49152):
        assert set(ro.absmax_plants(row_len)) == {"first", "last"}, row_len
    assert ro.absmax_plants(49156) == {"first": 0, "last": 49155, "last_unrolled": 4 * 12288 + 2, "first_remainder": 4 * 1 + 1}
    assert ro.absmax_plants(65548) == {"first": 0, "last": 65547, "last_unrolled": 4 * 16383 + 2, "first_remainder": 4 * 16384 + 1}
    unrolled, rest = ro.absmax_loops(81928)                      # 20482 float4: 16384 unrolled, 4098 in the remainder
    assert unrolled[:16384].all() and rest[16384:].all() and unrolled.sum() == 16384
    x = np.zeros((1, 81928))
    x[0, 4 * 16384 + 1], x[0, 4 * 300] = -3.0, 2.0
    parts = ro.absmax_parts(x).view(np.float32)
    assert parts[0, 0] == 3.0 and parts[0, 1] == 2.0 and (parts[0, 2:] == 0).all()
    assert [(16384 // n + 1) * n for n in ro.ADD_COLSUM_NCOLS] == [16388, 16392, 16448, 17408]


@pytest.mark.parametrize("alpha", ro.SOFTMAX_ALPHAS)
def test_softmax_references_against_autograd(alpha):
    a = float(np.float32(alpha))
    x, dp = ro.softmax_rows("normal", 3, 252, alpha)
    xt = torch.tensor(x, dtype=torch.float64, requires_grad=True)
    p = torch.softmax(a * xt, dim=-1)
    (p * torch.tensor(dp)).sum().backward()
    assert np.abs(ro.softmax_ref(x, a) - p.detach().numpy()).max() < 1e-15
    assert np.abs(ro.softmax_bwd_ref(x, dp, a) - xt.grad.numpy()).max() < 1e-14
    # the twins compute the same thing, to fp32
    assert np.abs(ro.softmax_twin(x, a) - ro.softmax_ref(x, a)).max() < 1e-6
    p32 = ro.f32(ro.softmax_ref(x, a))
    assert np.abs(ro.softmax_bwd_twin(p32, dp, a) - ro.softmax_bwd_ref(x, dp, a)).max() < 1e-6
    for kind in ro.SOFTMAX_KINDS:
        xk, _ = ro.softmax_rows(kind, 3, 1028, alpha)
        assert np.isfinite(ro.softmax_twin(xk, a)).all() and abs(ro.softmax_ref(xk, a).sum(-1) - 1).max() < 1e-12
    xp, _ = ro.softmax_rows("peak", 3, 1028, alpha)
    assert (1 - ro.softmax_ref(xp, a).max(-1) < 1028 * np.exp(-80.0)).all()         # saturated under every alpha


def test_temb_references_against_autograd():
    n, E = 5, 130
    t, dout = ro.temb_data(n, E)
    half = E // 2
    tt = torch.tensor(t, dtype=torch.float64, requires_grad=True)
    nlw = float(np.float32(-np.log(10000.0) / (half - 1)))
    w = torch.exp(torch.arange(half, dtype=torch.float64) * nlw)
    tv = torch.tensor((t.astype(np.float32) * np.float32(1000.0)).astype(np.float64))
    a = (tv + 1000.0 * (tt - tt.detach()))[:, None] * w[None, :]       # value from fp32(1000 t), slope 1000
    out = torch.cat([torch.sin(a), torch.cos(a)], dim=1)
    (out * torch.tensor(dout)).sum().backward()
    assert np.abs(ro.temb_fwd(t, E) - out.detach().numpy()).max() < 1e-12
    assert np.abs(ro.temb_bwd(t, dout, E) - tt.grad.numpy()).max() < 1e-9 * np.abs(tt.grad.numpy()).max()
    assert np.abs(ro.temb_fwd(t, E, ro.F32) - ro.temb_fwd(t, E)).max() < 2e-3
    assert ro.temb_fwd(t, E, ro.F32).dtype == np.float32 and ro.temb_bwd(t, dout, E, ro.F32).dtype == np.float32
    assert [ro.temb_fits(E, E + x, c) for x in (0, 8) for c in (0, 8)] == [True, False, True, True]
