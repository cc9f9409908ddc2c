"""CPU tests of the image-fidelity analysis (mulan_image_fidelity / ops.image_fidelity / mulan_amd.fidelity / python -m
ldm.fidelity): the float64 oracle against an independent recipe and against closed forms, the fp32 twin's protocol, the
argument checks, and the host arithmetic around the kernel with ops.image_fidelity answered by the oracle.  The kernel
itself is held to the oracle in tests/test_gpu_fidelity.py."""
import json
import os
import re

import numpy as np
import pytest
import torch

from tests import fidelity_oracle as fo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def random_images(n, seed):
    return np.random.default_rng(seed).integers(0, 256, (n, 32, 32, 3), dtype=np.uint8)


def smooth_images(n, seed, noise=6.0):
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:32, 0:32] / 32.0
    base = 128 + 90 * np.sin(2 * np.pi * (x[None, ..., None] * rng.uniform(0.5, 2, (n, 1, 1, 3))
                                          + y[None, ..., None] * rng.uniform(0.5, 2, (n, 1, 1, 3))))
    return np.clip(np.rint(base + rng.normal(0, noise, base.shape)), 0, 255).astype(np.uint8)


def flat_images(n, seed, level=250, spread=2):
    return np.random.default_rng(seed).integers(level - spread, level + spread + 1, (n, 32, 32, 3)).astype(np.uint8)


# ------------------------------------------------------------------------------------------------------ the oracle
def recipe(a, b):
    """the independent statement: scipy's Gaussian filter of the five maps, cropped by 5 (what skimage does)"""
    from scipy.ndimage import gaussian_filter
    filt = lambda v: np.stack([np.stack([gaussian_filter(v[n, :, :, c], 1.5, truncate=3.5) for c in range(v.shape[3])], -1)  # noqa: E731
                               for n in range(len(v))])[:, 5:-5, 5:-5]
    x, y = a.astype(np.float64), b.astype(np.float64)
    mx, my = filt(x), filt(y)
    sxx, syy, sxy = filt(x * x) - mx * mx, filt(y * y) - my * my, filt(x * y) - mx * my
    return ((2 * mx * my + fo.C1) * (2 * sxy + fo.C2)) / ((mx * mx + my * my + fo.C1) * (sxx + syy + fo.C2))


@pytest.mark.parametrize("make", [random_images, smooth_images, flat_images])
def test_oracle_agrees_with_the_scipy_recipe(make):
    a, b = make(3, 1), make(3, 2)
    got, want = fo.ssim_map(a, b), recipe(a, b)
    assert got.shape == (3, 22, 22, 3)
    err = np.abs(got - want).max()
    print(f"{make.__name__}: |oracle - recipe| = {err:.3g} (bar 1e-12)")
    assert err <= 1e-12
    g = fo.ssim_map(a, b, gray=True)
    assert g.shape == (3, 22, 22, 1)
    luma = lambda v: fo.gray_mix(v.astype(np.float64))                      # noqa: E731
    from scipy.ndimage import gaussian_filter
    mu = gaussian_filter(luma(a)[0, :, :, 0], 1.5, truncate=3.5)[5:-5, 5:-5]
    assert abs(mu - fo._windows(luma(a), fo.taps())[0, :, :, 0]).max() <= 1e-12


def test_closed_forms():
    x = random_images(2, 3)
    assert np.abs(fo.ssim_map(x, x) - 1.0).max() <= 1e-12
    for p, q in ((200, 60), (0, 255), (17, 17)):
        a, b = np.full((1, 32, 32, 3), p, np.uint8), np.full((1, 32, 32, 3), q, np.uint8)
        want = (2.0 * p * q + fo.C1) / (p * p + q * q + fo.C1)
        assert np.abs(fo.ssim_map(a, b) - want).max() <= 1e-10                # the filtered squares cancel to 1e-12 of 255^2
        assert abs(fo.ssim(a, b) - want).max() <= 1e-10
    from mulan_amd import fidelity as fd
    black, white = np.zeros((1, 32, 32, 3), np.uint8), np.full((1, 32, 32, 3), 255, np.uint8)
    s, _ = fo.sse(black, white)
    assert (s == 1024 * 255 * 255).all() and s.max() < 2 ** 31
    assert fd.psnr_from_sse(s.sum(), 3072) == 0.0
    assert fd.psnr_from_sse(0, 3072) == float("inf")
    assert fo.C1 == pytest.approx(6.5025) and fo.C2 == pytest.approx(58.5225) and abs(fo.taps().sum() - 1) < 1e-15


def test_sse_and_masks_of_the_oracle():
    a, b = random_images(3, 4), random_images(3, 5)
    mask = np.zeros((32, 32), np.uint8)
    mask[3, 7] = 9
    s, sm = fo.sse(a, b, mask=mask)
    d = a.astype(np.int64) - b.astype(np.int64)
    assert (s == (d * d).sum(axis=(1, 2))).all() and (sm == (d * d)[:, 3, 7]).all()
    s2, sm2 = fo.sse(a, b, ia=[2, 5, -1], ib=[0, 1, 2], mask=np.ones((3, 32, 32), np.uint8))
    assert (s2[1:] == -1).all() and (sm2[1:] == -1).all() and (s2[0] == ((a[2].astype(int) - b[0]) ** 2).sum(axis=(0, 1))).all()
    assert (sm2[0] == s2[0]).all()
    m = fo.ssim_map(a, b, ia=[2, 5, -1], ib=[0, 1, 2])
    assert np.isnan(m[1:]).all() and np.isfinite(m[0]).all()


def test_twin_protocol_and_the_centring():
    """the twin stays within the analytic ceiling on identical pairs, and on the cancellation cases the bars are 4 x its
    deviation, which is printed (DESIGN.md section 3.13 records it)"""
    x = random_images(2, 6)
    same = fo.bounds(x, x)
    print(f"identical: twin map dev {same['dev_map']:.3g} (ceiling {fo.CEILING_MAP:.3g}), mean {same['dev_ssim']:.3g} "
          f"(ceiling {fo.CEILING_SSIM:.3g})")
    assert same["dev_map"] <= fo.CEILING_MAP and same["dev_ssim"] <= fo.CEILING_SSIM
    const = fo.bounds(np.full((1, 32, 32, 3), 200, np.uint8), np.full((1, 32, 32, 3), 60, np.uint8))
    flat = fo.bounds(flat_images(4, 7), flat_images(4, 8))
    print(f"constant 200 / 60: twin dev {const['dev_map']:.3g}; nearly flat 250 +- 2: {flat['dev_map']:.3g}")
    assert const["dev_map"] > 0 and flat["dev_map"] > 0
    assert const["tol_map"] == 4 * const["dev_map"] and flat["tol_ssim"] == 4 * flat["dev_ssim"]
    g = fo.bounds(random_images(2, 9), random_images(2, 10), gray=True)
    assert g["twin_map"].shape == (2, 22, 22, 1) and g["twin_map"].dtype == np.float32 and 0 < g["dev_map"] < 1e-4
    weights = re.search(r"GRAY_R = ([\d.]+)f, GRAY_G = ([\d.]+)f, GRAY_B = ([\d.]+)f",
                        open(os.path.join(ROOT, "mulan_amd", "csrc", "fidelity.hip")).read())
    from mulan_amd import ops
    assert tuple(float(v) for v in weights.groups()) == fo.GRAY == ops.SPECTRUM_GRAY and ops.FIDELITY_WINDOWS == fo.W


def test_binding_row_matches_the_header():
    from mulan_amd import lib
    P, I = lib.P, lib.I
    assert lib.SIGNATURES["mulan_image_fidelity"] == [P, I, P, I, P, P, I, I, P, I, P, P, P, P, P]
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mulan_hip.h")).read(), flags=re.S)
    m = re.search(r"\bint\s+mulan_image_fidelity\s*\(([^;]*?)\)\s*;", src, flags=re.S)
    assert m and len(m.group(1).split(",")) == 15


# ---------------------------------------------------------------------------------------------------- argument checks
def test_image_fidelity_check_refuses_what_the_entry_point_refuses():
    from mulan_amd import ops
    a, b = torch.zeros((4, 32, 32, 3), dtype=torch.uint8), torch.zeros((6, 32, 32, 3), dtype=torch.uint8)
    idx = torch.zeros(5, dtype=torch.int32)
    assert ops.image_fidelity_check(a, a) == (4, 3, 0)
    assert ops.image_fidelity_check(a, b, ib=idx[:4], gray=True) == (4, 1, 0)
    assert ops.image_fidelity_check(a, b, ia=idx, ib=idx, mask=torch.zeros((5, 32, 32), dtype=torch.uint8)) == (5, 3, 1)
    assert ops.image_fidelity_check(a.numpy(), a.numpy(), mask=np.zeros((32, 32), np.uint8), sse=False, ssim=False) == (4, 3, 0)
    bad = [
        (dict(a=a.float()), "a is uint8"), (dict(b=b[:, :16]), "b is uint8"), (dict(a=a[:0]), "a is uint8"),
        (dict(a=a[0]), "a is uint8"), (dict(a=None), "a is uint8"),
        (dict(b=b), "neither ia nor ib"),                                             # Na != Nb, no indices
        (dict(b=b, ib=idx), "ia is needed"),                                          # M = 5 > Na = 4 without ia
        (dict(b=b, ia=torch.zeros(7, dtype=torch.int32)), "ib is needed"),            # M = 7 > Nb = 6 without ib
        (dict(ia=idx.long()), "ia is int32"), (dict(ib=idx.float()), "ib is int32"), (dict(ia=idx[:0]), "ia is int32"),
        (dict(ia=idx.view(5, 1)), "ia is int32"), (dict(ia=idx, ib=idx[:3]), "ia has 5 pairs"),
        (dict(gray=1), "gray is a bool"), (dict(sse=None), "sse is a bool"), (dict(ssim=0), "ssim is a bool"),
        (dict(ssim_map="yes"), "ssim_map is a bool"),
        (dict(mask=torch.zeros((32, 32))), "mask is uint8"), (dict(mask=torch.zeros((3, 32, 32), dtype=torch.uint8)), "mask is uint8"),
        (dict(mask=torch.zeros((4, 32, 32, 1), dtype=torch.uint8)), "mask is uint8"),
        (dict(mask=torch.zeros((32, 32), dtype=torch.bool)), "mask is uint8"),
        (dict(sse=False, ssim=False), "nothing asked for"),
    ]
    for change, words in bad:
        kw = dict(a=a, b=a)
        kw.update(change)
        with pytest.raises(ValueError, match=words):
            ops.image_fidelity_check(**kw)
    with pytest.raises(ValueError, match="one device"):
        ops.image_fidelity(a.numpy(), a.numpy())
    with pytest.raises(TypeError):
        ops.image_fidelity(a, a, None)                                               # the options are keyword-only


# --------------------------------------------------------------------------------------------------- host arithmetic
@pytest.fixture
def oracle_ops(monkeypatch):
    """ops.image_fidelity answered by the float64 oracle on CPU tensors: what the modules do around the kernel"""
    from mulan_amd import ops
    calls = []

    def fake(a, b, *, ia=None, ib=None, gray=False, mask=None, sse=True, ssim=True, ssim_map=False):
        M, P, _ = ops.image_fidelity_check(a, b, ia, ib, gray, mask, sse, ssim, ssim_map)
        n = lambda t: None if t is None else t.numpy()                              # noqa: E731
        s, sm = fo.sse(n(a), n(b), n(ia), n(ib), n(mask))
        q = fo.ssim_map(n(a), n(b), n(ia), n(ib), gray)
        calls.append(M)
        t = lambda v, dt: torch.from_numpy(np.ascontiguousarray(v)).to(dt)         # noqa: E731
        return (t(s, torch.int32) if sse else None, t(sm, torch.int32) if mask is not None else None,
                t(q.mean(axis=(1, 2)), torch.float32) if ssim else None, t(q, torch.float32) if ssim_map else None)

    monkeypatch.setattr(ops, "image_fidelity", fake)
    return calls


def test_psnr_from_sse():
    from mulan_amd import fidelity as fd
    got = fd.psnr_from_sse(np.array([0, 3072, 3072 * 255 * 255, 7]), 3072)
    assert got.dtype == np.float64 and got[0] == np.inf and got[2] == 0.0
    assert got[1] == 10 * np.log10(255.0 ** 2) and got[3] == 10 * np.log10(255.0 ** 2 * 3072 / 7)
    assert np.isnan(fd.psnr_from_sse(0, 0)) and fd.psnr_from_sse(5, np.array([10, 0]))[0] == 10 * np.log10(65025 * 10 / 5)
    with pytest.raises(ValueError):
        fd.psnr_from_sse(-1, 3072)


def test_image_fidelity_chunks_masks_and_counts(oracle_ops):
    from mulan_amd import fidelity as fd
    a, b = random_images(20, 11), smooth_images(20, 12)
    b[3] = a[3]
    mask = np.zeros((20, 32, 32), bool)
    mask[:, 4:9, 10:20] = True                                                      # 50 pixels
    mask[5] = False                                                                 # an empty mask
    mask[6] = True
    one = fd.image_fidelity(a, b, mask=mask, keep_map=True, device="cpu")
    assert oracle_ops == [20]
    parts = fd.image_fidelity(a, b, mask=mask, keep_map=True, chunk=7, device="cpu")
    assert oracle_ops == [20, 7, 7, 6]
    for key in ("mse", "psnr", "ssim", "ssim_planes", "psnr_masked", "ssim_map"):
        assert np.array_equal(one[key], parts[key], equal_nan=True), key
    s, sm = fo.sse(a, b, mask=mask)
    assert np.array_equal(one["mse"], s / 1024.0) and one["psnr"][3] == np.inf and one["ssim"][3] == pytest.approx(1.0, abs=1e-6)
    assert one["psnr"][0] == 10 * np.log10(65025.0 * 3072 / s[0].sum())
    assert one["psnr_masked"][0] == 10 * np.log10(65025.0 * 150 / sm[0].sum())           # 50 pixels, three channels
    assert np.isnan(one["psnr_masked"][5]) and one["psnr_masked"][6] == one["psnr"][6] and one["psnr_masked"][3] == np.inf
    assert one["ssim_planes"].shape == (20, 3) and one["ssim_map"].shape == (20, 22, 22, 3)
    assert np.allclose(one["ssim"], fo.ssim(a, b).mean(axis=1), atol=1e-6)
    shared = fd.image_fidelity(a, b, mask=mask[0], chunk=8, device="cpu")
    assert shared["psnr_masked"][7] == one["psnr_masked"][7]
    g = fd.image_fidelity(a[:5], b[:5], gray=True, device="cpu")
    assert g["ssim_planes"].shape == (5, 1) and "ssim_map" not in g and "psnr_masked" not in g
    for kw, words in ((dict(chunk=0), "chunk"), (dict(gray=1), "bools"), (dict(mask=np.zeros((2, 32, 32), bool)), "mask is")):
        with pytest.raises(ValueError, match=words):
            fd.image_fidelity(a, b, device="cpu", **kw)
    with pytest.raises(ValueError, match="uint8 numpy"):
        fd.image_fidelity(a.astype(np.float32), b, device="cpu")
    with pytest.raises(ValueError, match="a has 20 images"):
        fd.image_fidelity(a, b[:19], device="cpu")


@pytest.mark.parametrize("spec", ["sr:2", "gray", "sr:4+gray"])
def test_baseline_is_the_degraded_original_replicated_back(spec, oracle_ops):
    from mulan_amd import fidelity as fd
    from mulan_amd.sampling import parse_degradation
    x = smooth_images(3, 13)
    f, gray = parse_degradation(spec)
    want = np.zeros(x.shape, np.float64)
    for n in range(3):                                                              # spelled out, pixel by pixel
        for by in range(32 // f):
            for bx in range(32 // f):
                block = x[n, by * f:(by + 1) * f, bx * f:(bx + 1) * f].astype(np.float64)
                mean = block.mean(axis=(0, 1))
                want[n, by * f:(by + 1) * f, bx * f:(bx + 1) * f] = mean.mean() if gray else mean
    base = fd.baseline(x, spec)
    assert base.dtype == np.uint8 and np.array_equal(base, np.floor(want + 0.5).astype(np.uint8))
    assert np.abs(base.astype(np.float64) - want).max() <= 0.5
    res = fd.restoration_quality(x, base, degradation=spec, device="cpu")         # a restoration that is the baseline itself
    assert np.array_equal(res["baseline_images"], base)
    assert (res["psnr_gain"] == 0).all() and (res["ssim_gain"] == 0).all() and res["psnr_gain_mean"] == 0.0 == res["ssim_gain_mean"]
    better = fd.restoration_quality(x, x, degradation=spec, device="cpu")           # a perfect restoration
    assert (better["psnr"] == np.inf).all() and (better["ssim_gain"] > 0).all() and np.isnan(better["psnr_mean"])
    assert better["baseline_psnr_mean"] == pytest.approx(fd.psnr_from_sse(fo.sse(base, x)[0].sum(axis=1), 3072).mean())


def test_restoration_quality_inverts_the_inpainting_mask(oracle_ops):
    from mulan_amd import fidelity as fd
    x = random_images(4, 14)
    keep = np.ones((32, 32), bool)
    keep[8:24, 8:24] = False                                                        # the unknown box
    filled = x.copy()
    filled[:, 8:24, 8:24] = random_images(4, 15)[:, 8:24, 8:24]
    res = fd.restoration_quality(x, filled, mask=keep, device="cpu")
    s, _ = fo.sse(filled, x)
    assert np.array_equal(res["psnr_masked"], fd.psnr_from_sse(s.sum(axis=1), 3 * 256))    # every error lies in the box
    assert (res["psnr_masked"] < res["psnr"]).all() and "psnr_gain" not in res
    assert res["psnr_masked_mean"] == pytest.approx(res["psnr_masked"].mean()) and res["ssim_median"] == np.median(res["ssim"])
    with pytest.raises(ValueError, match="4 originals, 3 restored"):
        fd.restoration_quality(x, filled[:3], device="cpu")
    with pytest.raises(ValueError, match="degradation"):
        fd.restoration_quality(x, filled, degradation="blur", device="cpu")


def test_diversity_addresses_the_pairs_by_index(oracle_ops):
    from mulan_amd import fidelity as fd
    draws = np.stack([random_images(2, 20 + k) for k in range(3)])                  # K = 3, N = 2
    ia, ib = fd.pair_indices(3, 2)
    assert ia.dtype == np.int32 and ia.tolist() == [0, 0, 2, 1, 1, 3] and ib.tolist() == [2, 4, 4, 3, 5, 5]
    res = fd.diversity(draws, device="cpu")
    assert oracle_ops == [6] and res["pairs"].tolist() == [[0, 1], [0, 2], [1, 2]]
    for n in range(2):
        for j, (k, l) in enumerate(res["pairs"]):
            assert res["pair_ssim"][n, j] == pytest.approx(fo.ssim(draws[k, n:n + 1], draws[l, n:n + 1]).mean(), abs=1e-6)
            assert res["pair_psnr"][n, j] == fd.psnr_from_sse(fo.sse(draws[k, n:n + 1], draws[l, n:n + 1])[0].sum(), 3072)
    assert np.allclose(res["ssim"], res["pair_ssim"].mean(axis=1)) and np.allclose(res["psnr"], res["pair_psnr"].mean(axis=1))
    with pytest.raises(ValueError, match="K >= 2"):
        fd.diversity(draws[:1], device="cpu")


def test_notebook_exports():
    from ldm import notebook_utils as nu
    from mulan_amd import fidelity as fd
    assert nu.image_fidelity is fd.image_fidelity and nu.restoration_quality is fd.restoration_quality
    assert nu.diversity is fd.diversity and nu.plot_fidelity is fd.plot_fidelity and nu.psnr_from_sse is fd.psnr_from_sse


# ------------------------------------------------------------------------------------------------------ command line
def _write(path, **arrays):
    np.savez(path, **arrays)
    return str(path)


def test_command_line_refusals_and_outputs(tmp_path, monkeypatch, oracle_ops, capsys):
    from ldm import fidelity as cli
    from mulan_amd import fidelity as fd
    monkeypatch.setattr(fd, "_default_device", lambda: torch.device("cpu"))
    x = smooth_images(6, 30)
    base = fd.baseline(x, "sr:4")
    orig = _write(tmp_path / "in.npz", images=x)
    rest = _write(tmp_path / "restored.npz", images=base, degradation=np.array("sr:4"), measurement=np.zeros((6, 8, 8, 3), np.float32))
    bare = _write(tmp_path / "bare.npz", images=base)
    out = str(tmp_path / "fidelity.npz")
    args = lambda r, *more: [f"--restored={r}", f"--originals={orig}", f"--out={out}", *more]      # noqa: E731
    with pytest.raises(SystemExit, match="neither a `degradation` nor a `mask`"):
        cli.main(args(bare))
    with pytest.raises(SystemExit, match="holds 5 images"):
        cli.main(args(_write(tmp_path / "short.npz", images=base[:5], degradation=np.array("sr:4"))))
    with pytest.raises(SystemExit, match="no `images`"):
        cli.main(args(_write(tmp_path / "none.npz", mask=np.zeros((6, 32, 32), np.uint8))))
    with pytest.raises(SystemExit, match="degradation"):
        cli.main(args(_write(tmp_path / "odd.npz", images=base, degradation=np.array("blur"))))
    with pytest.raises(SystemExit, match="no file"):
        cli.main(args(str(tmp_path / "missing.npz")))
    with pytest.raises(SystemExit, match=".npz"):
        cli.main([f"--restored={rest}", f"--originals={orig}", "--out=fidelity.txt"])
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(SystemExit, match="one process"):
        cli.main(args(rest))
    monkeypatch.setenv("WORLD_SIZE", "1")
    assert not os.path.exists(out) and oracle_ops == []

    assert cli.main(args(rest, "--keep=2")) == 0
    with np.load(out) as z:
        assert (z["psnr_gain"] == 0).all() and (z["ssim_gain"] == 0).all() and z["psnr"].shape == (6,)
        worst = z["worst"]
        assert worst.tolist() == np.argsort(z["ssim"], kind="stable")[:2].tolist()
        assert np.array_equal(z["worst_originals"], x[worst]) and np.array_equal(z["worst_baseline"], base[worst])
        assert np.array_equal(z["worst_restored"], base[worst])
        settings = json.loads(str(z["settings"]))
        assert settings["degradation"] == "sr:4" and settings["n"] == 6 and settings["keep"] == 2 and not settings["inpaint"]
    assert "over the baseline" in capsys.readouterr().out

    assert cli.main(args(bare, "--plain", "--gray", "--keep=0")) == 0
    with np.load(out) as z:
        assert "psnr_gain" not in z.files and "worst" not in z.files and z["ssim_planes"].shape == (6, 1)
    keep = np.ones((6, 32, 32), np.uint8)
    keep[:, :16] = 0
    assert cli.main(args(_write(tmp_path / "filled.npz", images=base, mask=keep))) == 0
    with np.load(out) as z:
        assert z["psnr_masked"].shape == (6,) and "baseline_psnr" not in z.files
        top = ((base[:, :16].astype(np.int64) - x[:, :16]) ** 2).sum(axis=(1, 2, 3))
        assert np.array_equal(z["psnr_masked"], fd.psnr_from_sse(top, 3 * 512))
