"""tests/f16x3_oracle.py (the host model the GPU tests of the f16x3 dense kernels compare against) held to its own
definitions: the scale and its two clamps, the reconstruction bound of the two-piece split, exactness on small integers,
and the two layouts' index maps."""
import numpy as np

from tests import f16x3_oracle as fo


def test_scale_of_puts_every_normal_maximum_into_2_13_to_2_14():
    for e in range(14, 255):
        for mant in (0, 1, 0x400000, 0x7FFFFF):
            bits = (e << 23) | mant
            m = np.array([bits], np.uint32).view(np.float32)[0]
            s, inv = fo.scale_of(bits)
            assert s.dtype == np.float32 and inv.dtype == np.float32
            p = np.float64(m) * np.float64(s)
            assert 2.0 ** 13 <= p < 2.0 ** 14, (e, mant)
            assert np.float32(m) * s == np.float32(p)            # the product is exact in fp32 (a power of two)
            assert np.float64(s) * np.float64(inv) == 1.0
            assert np.float64(s) == 2.0 ** (140 - e)


def test_scale_of_clamps():
    lo = fo.scale_of(14 << 23)
    hi = fo.scale_of(254 << 23)
    assert lo == (np.float32(2.0 ** 126), np.float32(2.0 ** -126))
    assert hi == (np.float32(2.0 ** -114), np.float32(2.0 ** 114))
    assert fo.scale_of(0) == lo                                  # an all-zero tensor
    assert fo.scale_of(int(fo.bits_of(1e-42))) == lo             # an fp32 denormal: biased exponent 0
    assert fo.scale_of(int(fo.bits_of(2.0 ** -120))) == lo       # a normal maximum below the clamp (e = 7)
    assert fo.scale_of(int(fo.bits_of(np.inf))) == hi            # inf: biased exponent 255
    for s, inv in (lo, hi):                                      # both ends are normal fp32 numbers
        assert np.isfinite(s) and np.isfinite(inv) and min(s, inv) >= 2.0 ** -126


def test_split2_reconstruction_bound():
    """|f64(h) + f64(l) - vs| <= 2^-22 |vs| + 2^-25 for |vs| < 2^14.

    h = RNE_16(vs) keeps 11 significant bits, so |vs - h| <= 2^-11 |vs| while h is a normal fp16 number; the difference
    r = vs - f32(h) is exact in fp32 (it fits the low 13 bits of vs), and l = RNE_16(r) again keeps 11 bits of r:
    |r - l| <= 2^-11 |r| <= 2^-22 |vs|.  That is the first term: two roundings of 11 bits each.  Where l is an fp16
    subnormal the spacing is 2^-24 and the rounding error is at most half of it, 2^-25, whatever r is: the second term.
    (Where h itself is subnormal, |vs - h| <= 2^-25 already, r is exact, and l is 0 or +-2^-24: again at most 2^-25.)"""
    rng = np.random.default_rng(0)
    parts = [rng.standard_normal(200000) * 2.0 ** rng.integers(-30, 12, 200000),
             rng.uniform(-2.0 ** 14, 2.0 ** 14, 200000),
             np.array([0.0, 2.0 ** -24, 2.0 ** -25, 3 * 2.0 ** -26, 2.0 ** -14, 2.0 ** 14 - 1, 16383.998, -16383.998,
                       2.0 ** 13, 1 + 2.0 ** -11, 1 + 2.0 ** -12, 1 + 3 * 2.0 ** -12, 2049.0, 2051.0])]
    vs = np.concatenate(parts).astype(np.float32)
    vs = vs[np.abs(vs) < 2.0 ** 14]
    h, l = fo.split2(vs)
    assert h.dtype == np.float16 and l.dtype == np.float16
    assert np.all(np.isfinite(h.astype(np.float64))) and np.all(np.isfinite(l.astype(np.float64)))
    err = np.abs(h.astype(np.float64) + l.astype(np.float64) - vs.astype(np.float64))
    bound = fo.split_bound(vs)
    assert np.all(err <= bound), float((err / bound).max())
    print("worst split error / bound:", float((err / bound).max()))
    assert float((err / bound).max()) > 0.2                      # the bound is not slack by an order of magnitude
    # round to nearest EVEN, in both pieces: ties of h go to the even 11-bit significand
    h, l = fo.split2(np.array([2049.0, 2051.0], np.float32))
    assert h.tolist() == [2048.0, 2052.0] and l.tolist() == [1.0, -1.0]


def test_split2_is_exact_on_small_integers_times_a_power_of_two():
    for p in range(-20, 12):
        vs = (np.arange(-4, 5) * 2.0 ** p).astype(np.float32)
        h, l = fo.split2(vs)
        assert np.array_equal(h.astype(np.float32), vs) and not np.any(l), p
    # through the scale: integers of magnitude <= 4 times ANY power of two, maximum 1 .. 4 times that power
    for p in (-100, -20, 0, 40, 90):
        for top in (1, 2, 3, 4):
            x = (np.arange(-top, top + 1) * 2.0 ** p).astype(np.float32).reshape(1, -1, 1)
            vs = fo.scaled(x)
            assert 2.0 ** 13 <= np.abs(vs).max() < 2.0 ** 14
            h, l = fo.split2(vs)
            assert np.array_equal(h.astype(np.float32), vs) and not np.any(l), (p, top)


def test_row_max16():
    x = np.zeros((4, 5, 3), np.float32)
    x[0, 2, 1] = -7.5
    x[1] = 1e-42
    x[3, 4, 2] = 3.0
    x[3, 0, 0] = -2.0
    got = fo.row_max16(x)
    assert got.dtype == np.uint32
    assert got.view(np.float32).tolist() == [7.5, np.float32(1e-42), 0.0, 3.0]


def test_pack_and_plane_index_maps_are_bijections():
    for K, N in ((16, 40), (32, 128), (48, 8)):
        idx = fo.pack_index(K, N)
        assert idx.shape == (K, N, 2)
        assert np.array_equal(np.sort(idx.ravel()), np.arange(K * N * 2))
        # the documented nesting [K/16][N][plane][16]: 16 consecutive input channels are contiguous
        assert idx[17 % K, 3, 1] == (((17 % K) // 16 * N + 3) * 2 + 1) * 16 + (17 % K) % 16
    for B, K, rows in ((1, 16, 128), (3, 32, 128), (2, 48, 256)):
        idx = fo.plane_index(B, K, rows)
        assert idx.shape == (B, rows, K, 2)
        assert np.array_equal(np.sort(idx.ravel()), np.arange(B * K * rows * 2))
        assert idx[B - 1, 5, K - 1, 1] == ((((B - 1) * (K // 16) + (K - 1) // 16) * rows + 5) * 2 + 1) * 16 + 15


def test_pack_linear_and_planes_of_round_trip():
    rng = np.random.default_rng(1)
    w = rng.standard_normal((32, 24)).astype(np.float32) * 0.1
    for transpose in (False, True):
        packed, maxbits = fo.pack_linear(w.T.copy() if transpose else w, transpose)
        assert maxbits == int(fo.bits_of(np.abs(w).max()))
        h, l = fo.unpack_linear(packed, 32, 24)
        vs = w * fo.scale_of(maxbits)[0]
        err = np.abs(h.astype(np.float64) + l.astype(np.float64) - vs)
        assert np.all(err <= fo.split_bound(vs))
    x1 = rng.standard_normal((256, 16)).astype(np.float32)
    x2 = rng.standard_normal((256, 32)).astype(np.float32) * 100
    x1[128:] *= 1e-6
    x2[128:] *= 1e-9
    planes = fo.planes_of(x1, x2, 128)
    h, l = fo.unplane(planes, 2, 48, 128)
    x = np.concatenate([x1, x2], -1).reshape(2, 128, 48)
    for b in range(2):
        s, _ = fo.scale_of(max(fo.row_max16(x1.reshape(2, -1))[b], fo.row_max16(x2.reshape(2, -1))[b]))
        vs = x[b] * s
        assert 2.0 ** 13 <= np.abs(vs).max() < 2.0 ** 14
        err = np.abs(h[b].astype(np.float64) + l[b].astype(np.float64) - vs)
        assert np.all(err <= fo.split_bound(vs))


def test_dense_ref():
    rng = np.random.default_rng(2)
    x1, x2 = rng.standard_normal((2, 8, 16)), rng.standard_normal((2, 8, 32))
    w, bias, res = rng.standard_normal((48, 5)), rng.standard_normal(5), rng.standard_normal((2, 8, 5))
    ref, mag = fo.dense_ref(x1, x2, w, bias, res)
    want = np.einsum("brk,kn->brn", fo.f32(np.concatenate([x1, x2], -1)), fo.f32(w)) + fo.f32(bias) + fo.f32(res)
    assert ref.dtype == np.float64 and np.allclose(ref, want, rtol=1e-14, atol=0)
    assert np.all(mag >= np.abs(ref))
    wb = rng.standard_normal((2, 16, 5))
    ref, _ = fo.dense_ref(x1, None, wb)
    assert np.allclose(ref[1], fo.f32(x1[1]) @ fo.f32(wb[1]), rtol=1e-14, atol=0)
