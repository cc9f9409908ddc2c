"""mulan_image_fidelity on the MI355X against the float64 oracle (tests/fidelity_oracle.py).  sse and sse_masked must equal
the oracle's integers; ssim and ssim_map must lie within tol_ssim and tol_map of it, 4 x the deviation of the oracle's
fp32 twin on the same input (the analytic ceiling where that is zero).  Every comparison prints the error beside the
bar.  A block handles one pair at a time and the library launches at most 512 blocks, so 513 pairs make one block take
two."""
import numpy as np
import pytest
import torch

from tests import fidelity_oracle as fo
from tests.test_fidelity import flat_images, random_images, smooth_images

pytestmark = pytest.mark.gpu


def dev(x):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).cuda()


def run(a, b, **kw):
    from mulan_amd import ops
    kw = {k: dev(v) if isinstance(v, np.ndarray) else v for k, v in kw.items()}
    return tuple(None if t is None else t.cpu().numpy() for t in ops.image_fidelity(dev(a), dev(b), **kw))


def hold(label, got, a, b, ia=None, ib=None, gray=False, mask=None):
    """(sse, sse_masked, ssim, ssim_map) of the kernel against the oracle's bounds for this input"""
    want = fo.bounds(a, b, ia, ib, gray, mask)
    sse, masked, ssim, smap = got
    assert sse.dtype == np.int32 and np.array_equal(sse, want["sse"]), label
    if mask is not None:
        assert masked.dtype == np.int32 and np.array_equal(masked, want["sse_masked"]), label
    ok = ~np.isnan(want["ssim"][:, 0])
    assert np.isnan(ssim[~ok]).all() and (smap is None or np.isnan(smap[~ok]).all()), label
    err = float(np.abs(ssim[ok] - want["ssim"][ok]).max())
    twin = float(np.abs(ssim[ok] - want["twin_ssim"][ok]).max())
    print(f"{label}: |ssim - oracle| = {err:.3g} (bar {want['tol_ssim']:.3g}; from the twin {twin:.3g})")
    assert err <= want["tol_ssim"], label
    if smap is not None:
        assert smap.shape == want["ssim_map"].shape and smap.dtype == np.float32
        err = float(np.abs(smap[ok] - want["ssim_map"][ok]).max())
        print(f"{label}: |ssim_map - oracle| = {err:.3g} (bar {want['tol_map']:.3g})")
        assert err <= want["tol_map"], label
    return want


@pytest.mark.parametrize("M", [1, 3, 513])
def test_pair_counts(M):
    a = np.concatenate([random_images(M - M // 2, 100 + M), smooth_images(M // 2, 101 + M)]) if M > 1 else random_images(1, 100)
    b = np.concatenate([smooth_images(M - M // 2, 102 + M, noise=20.0), smooth_images(M // 2, 101 + M, noise=3.0)]) if M > 1 \
        else smooth_images(1, 103)
    mask = np.random.default_rng(M).integers(0, 2, (M, 32, 32)).astype(np.uint8) * 255
    hold(f"M = {M}", run(a, b, mask=mask, ssim_map=True), a, b, mask=mask)


def test_hard_images():
    full = lambda v: np.full((1, 32, 32, 3), v, np.uint8)                           # noqa: E731
    got = run(full(0), full(255), ssim_map=True)
    hold("0 against 255", got, full(0), full(255))
    assert (got[0] == 1024 * 255 * 255).all()
    board = ((np.add.outer(np.arange(32), np.arange(32)) & 1) * 255).astype(np.uint8)
    board = np.repeat(board[None, :, :, None], 3, axis=3)
    hold("checkerboard against its inverse", run(board, 255 - board, ssim_map=True), board, 255 - board)
    for p, q in ((200, 60), (255, 254), (1, 0)):
        got = run(full(p), full(q), ssim_map=True)
        want = hold(f"constant {p} / {q}", got, full(p), full(q))
        closed = (2.0 * p * q + fo.C1) / (p * p + q * q + fo.C1)
        err = float(np.abs(got[3] - closed).max())
        print(f"constant {p} / {q}: |ssim_map - closed form| = {err:.3g} (bar {want['tol_map']:.3g})")
        assert err <= want["tol_map"] and abs(got[2] - closed).max() <= want["tol_ssim"]
    x = np.concatenate([random_images(2, 110), smooth_images(1, 111), full(250)])
    got = run(x, x, ssim_map=True)
    want = hold("identical pairs", got, x, x)
    assert (got[0] == 0).all() and np.abs(got[3] - 1.0).max() <= max(want["tol_map"], fo.CEILING_MAP)
    a, b = flat_images(4, 112), flat_images(4, 113)
    hold("nearly flat 250 +- 2", run(a, b, ssim_map=True), a, b)


def test_gray():
    a, b = np.concatenate([random_images(2, 120), flat_images(1, 121)]), np.concatenate([smooth_images(2, 122), flat_images(1, 123)])
    got = run(a, b, gray=True, ssim_map=True)
    assert got[2].shape == (3, 1) and got[3].shape == (3, 22, 22, 1) and got[0].shape == (3, 3)
    hold("gray", got, a, b, gray=True)


def test_map_mean_outputs_alone_and_determinism():
    from mulan_amd import ops
    a, b = random_images(5, 130), smooth_images(5, 131)
    mask = np.random.default_rng(132).integers(0, 2, (5, 32, 32)).astype(np.uint8)
    for gray in (False, True):
        both = run(a, b, gray=gray, mask=mask, ssim_map=True)
        want = fo.bounds(a, b, gray=gray)
        err = float(np.abs(both[3].astype(np.float64).mean(axis=(1, 2)) - both[2]).max())
        print(f"gray = {gray}: |mean of ssim_map - ssim| = {err:.3g} (bar {want['tol_ssim']:.3g})")
        assert err <= want["tol_ssim"]
        again = run(a, b, gray=gray, mask=mask, ssim_map=True)
        assert all(x.tobytes() == y.tobytes() for x, y in zip(both, again))
        alone = [run(a, b, gray=gray, sse=True, ssim=False)[0], run(a, b, gray=gray, sse=False, ssim=False, mask=mask)[1],
                 run(a, b, gray=gray, sse=False, ssim=True)[2], run(a, b, gray=gray, sse=False, ssim=False, ssim_map=True)[3]]
        assert all(x.tobytes() == y.tobytes() for x, y in zip(both, alone))
        assert run(a, b, gray=gray, sse=False, ssim=False, mask=mask)[0] is None
    assert ops.image_fidelity(dev(a), dev(b))[0].device.type == "cuda"


def test_masks():
    a, b = random_images(4, 140), random_images(4, 141)
    one = np.random.default_rng(142).integers(0, 2, (32, 32)).astype(np.uint8) * 7
    shared = run(a, b, mask=one, ssim=False)
    copies = run(a, b, mask=np.repeat(one[None], 4, axis=0), ssim=False)
    assert np.array_equal(shared[1], copies[1]) and np.array_equal(shared[1], fo.sse(a, b, mask=one)[1])
    assert (run(a, b, mask=np.zeros((32, 32), np.uint8), ssim=False)[1] == 0).all()
    all_one = run(a, b, mask=np.ones((4, 32, 32), np.uint8), ssim=False)
    assert np.array_equal(all_one[1], all_one[0])
    pixel = np.zeros((4, 32, 32), np.uint8)
    pixel[0, 0, 0] = pixel[1, 31, 31] = pixel[2, 15, 16] = pixel[3, 16, 15] = 1
    got = run(a, b, mask=pixel, ssim=False)[1]
    d = (a.astype(np.int64) - b.astype(np.int64)) ** 2
    assert np.array_equal(got, np.stack([d[0, 0, 0], d[1, 31, 31], d[2, 15, 16], d[3, 16, 15]]))


def test_indices():
    a, b = random_images(5, 150), smooth_images(7, 151)
    perm = np.random.default_rng(152).permutation(5).astype(np.int32)
    ib = np.array([6, 0, 3, 3, 5], np.int32)                                        # a repeated index, Na != Nb
    mask = np.random.default_rng(153).integers(0, 2, (5, 32, 32)).astype(np.uint8)
    hold("ia and ib", run(a, b, ia=perm, ib=ib, mask=mask, ssim_map=True), a, b, perm, ib, mask=mask)
    hold("ia alone", run(a, b, ia=perm, ssim_map=True), a, b, perm, None)
    hold("ib alone", run(a, b, ib=ib, ssim_map=True), a, b, None, ib)
    more = np.array([0, 4, 4, 1, 2, 3, 0, 0, 2], np.int32)                         # M > Na, M > Nb
    hold("more pairs than images", run(a, b, ia=more, ib=more[::-1].copy()), a, b, more, more[::-1])
    bad_a, bad_b = np.array([0, 5, 2, 3, 4], np.int32), np.array([0, 1, 2, -1, 4], np.int32)     # 5 = Na; a negative index
    got = run(a, b, ia=bad_a, ib=bad_b, mask=mask, ssim_map=True)
    hold("indices out of range", got, a, b, bad_a, bad_b, mask=mask)
    assert (got[0][[1, 3]] == -1).all() and (got[1][[1, 3]] == -1).all() and np.isnan(got[2][[1, 3]]).all()
    assert np.isnan(got[3][[1, 3]]).all() and np.isfinite(got[3][[0, 2, 4]]).all() and (got[0][[0, 2, 4]] >= 0).all()
    clean = run(a, b, ia=np.array([0, 2, 4], np.int32), ib=np.array([0, 2, 4], np.int32), mask=mask[[0, 2, 4]], ssim_map=True)
    assert all(x[[0, 2, 4]].tobytes() == y.tobytes() for x, y in zip(got, clean))    # the neighbours are untouched


def test_refusals():
    from mulan_amd import lib, ops
    L = lib.load()
    a, b = dev(random_images(4, 160)), dev(random_images(4, 161))
    sse = torch.empty((8, 3), dtype=torch.int32, device="cuda")                      # room for the largest M below
    ssim = torch.empty((8, 3), dtype=torch.float32, device="cuda")
    smap = torch.empty((8, 22, 22, 3), dtype=torch.float32, device="cuda")
    mask = torch.ones((32, 32), dtype=torch.uint8, device="cuda")
    idx = torch.zeros(8, dtype=torch.int32, device="cuda")
    p = lib.ptr

    def rc(a_=None, Na=4, b_=None, Nb=4, ia=None, ib=None, M=4, gray=0, mask_=None, per=0, sse_=sse, masked=None, ssim_=ssim,
           smap_=None):
        return L.mulan_image_fidelity(p(a) if a_ is None else a_, Na, p(b) if b_ is None else b_, Nb, p(ia), p(ib), M, gray,
                                      p(mask_), per, p(sse_), p(masked), p(ssim_), p(smap_), lib.stream())

    assert rc() == 0 and rc(ia=idx, ib=idx, M=8, sse_=None, ssim_=None, smap_=None, mask_=mask,
                            masked=torch.empty((8, 3), dtype=torch.int32, device="cuda")) == 0
    invalid = 1                                                                      # hipErrorInvalidValue
    raw = torch.empty(4 * 3072 + 16, dtype=torch.uint8, device="cuda")
    assert rc(a_=raw.data_ptr() + 1) == invalid and rc(b_=raw.data_ptr() + 8) == invalid     # views offset by 1 and 8 bytes
    assert rc(mask_=mask) == invalid and rc(masked=sse) == invalid                   # a mask without sse_masked, and the reverse
    assert rc(sse_=None, ssim_=None) == invalid                                      # all outputs off
    assert rc(M=5) == invalid and rc(M=5, ia=idx) == invalid and rc(M=5, ib=idx) == invalid and rc(M=5, ia=idx, ib=idx) == 0
    assert rc(M=0) == invalid and rc(Na=0, ia=idx) == invalid and rc(Nb=0, ib=idx) == invalid
    assert rc(a_=0) == invalid and rc(gray=2) == invalid and rc(mask_=mask, masked=sse, per=2) == invalid and rc(gray=-1) == invalid
    assert rc(smap_=smap.view(-1)[1:]) == invalid and rc(ssim_=None, sse_=None, smap_=smap) == 0
    odd = torch.empty(64, dtype=torch.uint8, device="cuda")
    assert L.mulan_image_fidelity(p(a), 4, p(b), 4, odd.data_ptr() + 2, None, 4, 0, None, 0, p(sse), None, None, None,
                                  lib.stream()) == invalid
    assert L.mulan_image_fidelity(p(a), 4, p(b), 4, None, None, 4, 0, None, 0, odd.data_ptr() + 1, None, None, None,
                                  lib.stream()) == invalid
    torch.cuda.synchronize()
    with pytest.raises(lib.MulanHipError):
        ops.image_fidelity(raw[1:1 + 4 * 3072].view(4, 32, 32, 3), b)                # the same view through the op
    with pytest.raises(ValueError, match="nothing asked for"):
        ops.image_fidelity(a, b, sse=False, ssim=False)
    with pytest.raises(ValueError, match="ia is needed"):
        ops.image_fidelity(a[:3], b, ib=idx[:4])
    with pytest.raises(ValueError, match="one device"):
        ops.image_fidelity(a, b.cpu())


def test_image_fidelity_in_chunks_and_diversity():
    from mulan_amd import fidelity as fd
    a, b = random_images(20, 170), smooth_images(20, 171)
    mask = np.random.default_rng(172).integers(0, 2, (20, 32, 32)).astype(bool)
    one = fd.image_fidelity(a, b, mask=mask, keep_map=True)
    parts = fd.image_fidelity(a, b, mask=mask, keep_map=True, chunk=7)
    assert set(one) == {"mse", "psnr", "ssim", "ssim_planes", "psnr_masked", "ssim_map"}
    assert all(one[k].tobytes() == parts[k].tobytes() for k in one)
    want = fo.bounds(a, b, mask=mask)
    assert np.array_equal(one["mse"] * 1024, want["sse"]) and np.abs(one["ssim_planes"] - want["ssim"]).max() <= want["tol_ssim"]
    assert np.array_equal(one["psnr_masked"], fd.psnr_from_sse(want["sse_masked"].sum(axis=1), 3 * mask.reshape(20, -1).sum(axis=1)))
    draws = np.stack([smooth_images(2, 173 + k, noise=4.0 + k) for k in range(3)])  # K = 3, N = 2
    res = fd.diversity(draws)
    for n in range(2):
        for j, (k, l) in enumerate(res["pairs"]):
            x, y = draws[k, n:n + 1], draws[l, n:n + 1]
            w = fo.bounds(x, y)
            err = abs(res["pair_ssim"][n, j] - w["ssim"].mean())
            print(f"diversity n = {n}, pair ({k}, {l}): |ssim - oracle| = {err:.3g} (bar {w['tol_ssim']:.3g})")
            assert err <= w["tol_ssim"] and res["pair_psnr"][n, j] == fd.psnr_from_sse(w["sse"].sum(), 3072)
    assert np.allclose(res["ssim"], res["pair_ssim"].mean(axis=1), rtol=0, atol=1e-15)


def test_restoration_quality_of_the_baseline_gains_nothing():
    import os
    from mulan_amd import fidelity as fd
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "tiny_model.npz")
    x = None
    if os.path.exists(path):
        with np.load(path) as z:
            for key in z.files:
                if z[key].dtype == np.uint8 and z[key].ndim == 4 and z[key].shape[1:] == (32, 32, 3):
                    x = np.asarray(z[key])
    if x is None:                                                                   # the fixture holds no images
        x = smooth_images(6, 180)
    base = fd.baseline(x, "sr:4")
    res = fd.restoration_quality(x, base, degradation="sr:4")
    assert (res["psnr_gain"] == 0).all() and (res["ssim_gain"] == 0).all() and res["psnr_gain_mean"] == 0 == res["ssim_gain_mean"]
    assert np.array_equal(res["baseline_images"], base) and np.isfinite(res["psnr"]).all()
    want = fo.bounds(base, x)
    assert np.abs(res["ssim_planes"] - want["ssim"]).max() <= want["tol_ssim"]
    assert np.array_equal(res["psnr"], fd.psnr_from_sse(want["sse"].sum(axis=1), 3072))
