"""CPU tests of the spectrum analysis (mulan_spectrum / ops.spectrum / mulan_amd.spectrum / python -m ldm.spectrum): the
declaration and the binding rows, the float64 oracle against scipy and against its own identities, the radial bins,
every refusal before any library call, the host arithmetic on hand-made dicts, the chunked upload and dct2 over a
stand-in for the kernel (the oracle itself), and the command line.  The kernel itself is held to the oracle in
tests/test_gpu_spectrum.py."""
import json
import os
import re

import numpy as np
import pytest
import torch

from tests import spectrum_oracle as so

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------ the boundary
def test_header_declares_both_symbols_and_the_binding_table_binds_them():
    from mulan_amd import lib
    P, I, F, Z = lib.P, lib.I, lib.F, lib.Z
    assert lib.SIGNATURES["mulan_spectrum"] == [P, I, F, F, I, I, P, P, P, P, I, I, P, Z, P]
    assert lib.SIGNATURES["mulan_spectrum_workspace"] == [I, I, I]
    assert lib._RESTYPES["mulan_spectrum_workspace"] is lib.c_size_t
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mulan_hip.h")).read(), flags=re.S)
    m = re.search(r"\bint\s+mulan_spectrum\s*\(([^;]*?)\)\s*;", src, flags=re.S)
    assert m and len(m.group(1).split(",")) == 15
    m = re.search(r"\bsize_t\s+mulan_spectrum_workspace\s*\(([^;]*?)\)\s*;", src, flags=re.S)
    assert m and len(m.group(1).split(",")) == 3
    assert "mulan_spectrum" in open(os.path.join(ROOT, "INTEGRATION.md")).read()


def test_the_kernel_source_uses_the_fp32_matrix_core_and_no_atomics():
    src = re.sub(r"//.*", "", open(os.path.join(ROOT, "mulan_amd", "csrc", "spectrum.hip")).read())
    assert "mfma32(" in src and "mfma32_row(" in src and "asm" not in src and "atomic" not in src
    for w in so.GRAY:                                      # the grey weights are written as constants
        assert f"{w}f" in src
    from mulan_amd import ops
    assert ops.SPECTRUM_GRAY == so.GRAY and ops.SPECTRUM_BINS == so.BINS


# ------------------------------------------------------------------------------------------------ the oracle
@pytest.fixture(scope="module")
def images():
    rng = np.random.default_rng(11)
    return rng.integers(0, 256, (50, 32, 32, 3)).astype(np.uint8)


def test_oracle_equals_scipy_dctn(images):
    fft = pytest.importorskip("scipy.fft")
    x = so.read(images[:4], 2.0 / 256, 1.0 / 256 - 1)
    want = fft.dctn(x, axes=(1, 2), norm="ortho")
    assert np.abs(so.coef(images[:4], 2.0 / 256, 1.0 / 256 - 1) - want).max() < 1e-12
    g = so.coef(images[:4], 1.0 / 255, 0.0, gray=True)
    assert g.shape == (4, 32, 32, 1)
    assert np.abs(g - fft.dctn(so.planes(images[:4], 1.0 / 255, 0.0, gray=True), axes=(1, 2), norm="ortho")).max() < 1e-12
    f = np.random.default_rng(0).standard_normal((2, 32, 32, 3)).astype(np.float32)
    assert np.abs(so.coef(f) - fft.dctn(f.astype(np.float64), axes=(1, 2), norm="ortho")).max() < 1e-12


def test_dct_matrix_is_orthonormal_and_parseval_holds(images):
    D = so.dct_matrix()
    assert np.abs(D @ D.T - np.eye(32)).max() < 1e-14 and np.abs(D.T @ D - np.eye(32)).max() < 1e-14
    assert np.abs(np.abs(D).sum(axis=1)).max() <= np.sqrt(32) + 1e-12          # the ceiling's row-sum premise
    x = so.read(images[:5], 2.0 / 256, 1.0 / 256 - 1)
    c = so.coef(images[:5], 2.0 / 256, 1.0 / 256 - 1)
    assert np.allclose((c * c).sum(axis=(1, 2)), (x * x).sum(axis=(1, 2)), rtol=1e-13)
    assert np.allclose(so.radial(c).sum(axis=1), (x * x).sum(axis=(1, 2)), rtol=1e-13)
    assert np.allclose(c[:, 0, 0], x.sum(axis=(1, 2)) / 32.0, rtol=1e-13)       # DC = 32 x the mean


def test_every_coefficient_falls_into_exactly_one_bin_and_the_integer_rule_is_the_rounded_root():
    from mulan_amd import spectrum as sp
    b = so.bin_table()                                                          # asserts "exactly one" per (u, v)
    u, v = np.arange(32)[:, None], np.arange(32)[None, :]
    assert np.array_equal(b, np.floor(np.sqrt(u * u + v * v) + 0.5).astype(np.int64))
    assert b.min() == 0 and b.max() == so.BINS - 1 == 44 and (b == 0).sum() == 1 and b[0, 0] == 0
    assert set(np.unique(b)) == set(range(45))
    assert np.array_equal(sp.bin_table(), b)
    assert sp.radial_freq().shape == (45,) and sp.radial_freq()[32] == 0.5


def test_the_fp32_restatement_sits_below_the_analytic_ceiling(images):
    rng = np.random.default_rng(5)
    gamma_like = (-4.0 + 0.05 * rng.standard_normal((3, 32, 32, 3))).astype(np.float32)
    for x, kw in ((images[:9], dict(scale=2.0 / 256, offset=1.0 / 256 - 1)), (images[:9], dict(scale=1.0 / 255, gray=True)),
                  (rng.standard_normal((9, 32, 32, 3)).astype(np.float32), {}), (gamma_like, {})):
        b = so.bounds(x, **kw)                                                  # asserts err <= ceiling
        assert 0 < b["err_coef"] <= b["ceiling"] and b["tol_coef"] == 4 * b["err_coef"]
        assert b["tol_radial"] > 0 and b["tol_sum1"] > 0 and b["tol_sum2"] > 0
    assert so.ceiling(13.3) == 68 * 2.0 ** -24 * 32 * 13.3


# ------------------------------------------------------------------------------------------------ refusals
def _no_library(monkeypatch):
    from mulan_amd import lib, ops

    def no_call(*a, **k):
        raise AssertionError("the library was called")
    monkeypatch.setattr(ops, "call", no_call)
    monkeypatch.setattr(ops, "stream", lambda: None)          # an argument of `call`: no device is asked for a stream
    monkeypatch.setattr(lib, "load", no_call)
    monkeypatch.setattr(lib, "call", no_call)


def test_ops_argument_checks_come_before_any_library_call(monkeypatch):
    from mulan_amd import ops
    _no_library(monkeypatch)
    x = torch.zeros((4, 32, 32, 3), dtype=torch.uint8)
    s64 = lambda p=3, dt=torch.float64: torch.zeros((32, 32, p), dtype=dt)       # noqa: E731
    ok = dict(x=x, radial=True)
    bad = [
        (dict(x=x.to(torch.int8)), "uint8 or fp32"), (dict(x=x.double()), "uint8 or fp32"), (dict(x=x[0]), "uint8 or fp32"),
        (dict(x=torch.zeros((4, 3, 32, 32), dtype=torch.uint8)), "uint8 or fp32"),
        (dict(x=torch.zeros((0, 32, 32, 3), dtype=torch.uint8)), "uint8 or fp32"),
        (dict(x=torch.zeros((4, 16, 16, 3), dtype=torch.float32)), "uint8 or fp32"),
        (dict(radial=False), "nothing asked for"), (dict(scale=float("nan")), "scale"), (dict(offset="0"), "offset"),
        (dict(gray=1), "gray is a bool"), (dict(coef=1), "coef is a bool"), (dict(blocks=-1), "blocks"),
        (dict(blocks=5000), "blocks"), (dict(blocks=2.0), "blocks"),
        (dict(accumulate_into=(s64(),)), "pair"), (dict(accumulate_into=(s64(), s64(1))), "sum2 is"),
        (dict(accumulate_into=(s64(dt=torch.float32), s64())), "sum1 is"),
        (dict(gray=True, accumulate_into=(s64(), s64())), "sum1 is"),
    ]
    for change, match in bad:
        kw = {**ok, **change}
        with pytest.raises(ValueError, match=match):
            ops.spectrum(kw.pop("x"), **kw)
    with pytest.raises(ValueError, match="tensor on the device"):
        ops.spectrum(x.numpy(), radial=True)
    with pytest.raises(TypeError):                                              # the options are keyword-only
        ops.spectrum(x, 1.0, 0.0)
    for good in (dict(radial=True), dict(coef=True, gray=True), dict(sums=True), dict(accumulate_into=(s64(), s64()))):
        with pytest.raises(AssertionError, match="the library was called"):     # and a good call does reach the library
            ops.spectrum(x, **good)


def test_module_argument_checks_come_before_any_library_call(monkeypatch):
    from mulan_amd import spectrum as sp
    _no_library(monkeypatch)
    img = np.zeros((5, 32, 32, 3), dtype=np.uint8)
    for fn in (sp.dct2, sp.image_spectrum):
        with pytest.raises(ValueError, match="dtype"):
            fn(img.astype(np.float64))
        with pytest.raises(ValueError, match="32, 32, 3"):
            fn(np.zeros((5, 3, 32, 32), dtype=np.uint8))
        with pytest.raises(ValueError, match="32, 32, 3"):
            fn(np.zeros((0, 32, 32, 3), dtype=np.uint8))
        with pytest.raises(ValueError, match="array or tensor"):
            fn([[1, 2, 3]])
    with pytest.raises(ValueError, match="dtype"):
        sp.image_spectrum(img.astype(np.float32))                               # a set is uint8
    with pytest.raises(ValueError, match="a set"):
        sp.image_spectrum(img[0])
    for chunk in (0, -3, 2.5, True):
        with pytest.raises(ValueError, match="chunk"):
            sp.image_spectrum(img, chunk=chunk)
    with pytest.raises(ValueError, match="bools"):
        sp.image_spectrum(img, gray=1)
    with pytest.raises(AssertionError, match="the library was called"):
        sp.image_spectrum(img, device="cpu")
    with pytest.raises(AssertionError, match="the library was called"):
        sp.dct2(img[0], device="cpu")

    class Plain:                                                                # a model_vdm.VDM has no latent embedding
        model = object()
    with pytest.raises(ValueError, match="needs a MuLAN model"):
        sp.schedule_spectrum(Plain(), np.zeros((1, 50), np.float32))


# ------------------------------------------------------------------------------------------------ host arithmetic
def _spectrum_dict(power, mean=None):
    from mulan_amd import spectrum as sp
    power = np.asarray(power, dtype=np.float64)
    mean = np.zeros_like(power) if mean is None else mean
    return sp.moments_from_sums(mean * 10, power * 10, 10)


def test_compare_spectra_on_hand_made_dicts():
    from mulan_amd import spectrum as sp
    b = so.bin_table()
    power = np.repeat((1.0 / (1.0 + b.astype(np.float64)))[..., None], 3, axis=2)       # a falling spectrum
    ref = _spectrum_dict(power, mean=np.full_like(power, 0.01))
    assert ref["n"] == 10 and np.allclose(ref["coef_var"], power - 1e-4) and np.allclose(ref["power_mean"], power)
    counts = np.bincount(b.reshape(-1), minlength=45)
    assert np.allclose(ref["radial_mean"][:, 0], counts / (1.0 + np.arange(45)))
    same = sp.compare_spectra(ref, dict(ref))
    assert same["lsd_db"] == 0 and same["frechet_diag"] == 0 and same["high_band_ratio"] == 1
    assert same["log_ratio"].shape == (45, 3) and (same["log_ratio"] == 0).all()
    # the bins r >= 16 halved in power
    low = np.where((b >= 16)[..., None], 0.5, 1.0)
    smp = _spectrum_dict(power * low, mean=np.full_like(power, 0.01))
    got = sp.compare_spectra(smp, ref)
    want = np.where(np.arange(45) >= 16, np.log10(0.5), 0.0)
    assert np.allclose(got["log_ratio"], want[:, None], atol=1e-14)
    assert np.isclose(got["lsd_db"], np.sqrt(29 / 44) * 10 * np.log10(2.0))                  # 29 of the 44 AC bins at -3.01 dB
    r = ref["radial_mean"].sum(axis=1)
    h, ac = r[16:].sum(), r[1:].sum()
    assert np.isclose(got["high_band_ratio"], (0.5 * h / (ac - 0.5 * h)) / (h / ac))
    sd_a, sd_b = np.sqrt(power * low - 1e-4), np.sqrt(power - 1e-4)
    assert np.isclose(got["frechet_diag"], ((sd_a - sd_b) ** 2).sum())
    moved = _spectrum_dict(power, mean=np.full_like(power, 0.03))                            # the means moved by 0.02
    d = sp.compare_spectra(moved, ref)["frechet_diag"]
    assert np.isclose(d, 3072 * 0.02 ** 2 + ((np.sqrt(power - 9e-4) - np.sqrt(power - 1e-4)) ** 2).sum())
    with pytest.raises(ValueError, match="dict of image_spectrum"):
        sp.compare_spectra(ref, dict(radial_mean=ref["radial_mean"]))
    with pytest.raises(ValueError, match="same planes"):
        sp.compare_spectra(ref, _spectrum_dict(power[..., :1]))
    with pytest.raises(ValueError, match="no power"):
        sp.compare_spectra(ref, _spectrum_dict(np.zeros_like(power)))
    assert "PIXEL-space" in sp.compare_spectra.__doc__ and "not comparable" in sp.compare_spectra.__doc__
    assert sp.ac_share(np.concatenate([np.ones((2, 1, 3)), np.zeros((2, 44, 3))], axis=1)).tolist() == [[0.0] * 3] * 2
    assert np.allclose(sp.ac_share(np.ones((45, 3))), 44 / 45)


# ------------------------------------------------------------------------------------------------ over a stand-in
def _stand_in(monkeypatch, calls):
    """ops.spectrum answered by the float64 oracle on CPU tensors: what the module does around the kernel"""
    from mulan_amd import ops

    def fake(x, *, scale=1.0, offset=0.0, gray=False, coef=False, radial=False, sums=False, accumulate_into=None, blocks=0):
        ops.spectrum_check(x, scale, offset, gray, coef, radial, sums, accumulate_into, blocks)
        calls.append((tuple(x.shape), scale, offset, gray, accumulate_into is not None))
        c = so.coef(x.numpy(), scale, offset, gray)
        out_s = None
        if sums or accumulate_into is not None:
            s1, s2 = (torch.from_numpy(v) for v in so.set_sums(c))
            if accumulate_into is not None:
                accumulate_into[0].add_(s1)
                accumulate_into[1].add_(s2)
                out_s = tuple(accumulate_into)
            else:
                out_s = (s1, s2)
        return (torch.from_numpy(c.astype(np.float32)) if coef else None,
                torch.from_numpy(so.radial(c).astype(np.float32)) if radial else None, out_s)
    monkeypatch.setattr(ops, "spectrum", fake)


def test_image_spectrum_in_chunks_equals_one_chunk_and_the_oracle(monkeypatch, images):
    from mulan_amd import spectrum as sp
    calls = []
    _stand_in(monkeypatch, calls)
    one = sp.image_spectrum(images, chunk=1000, keep_radial=True, device="cpu")
    assert calls == [((50, 32, 32, 3), 2.0 / 256, 1.0 / 256 - 1, False, False)]
    calls.clear()
    parts = sp.image_spectrum(images, chunk=16, keep_radial=True, device="cpu")
    assert [c[0][0] for c in calls] == [16, 16, 16, 2] and [c[4] for c in calls] == [False, True, True, True]
    c = so.coef(images, 2.0 / 256, 1.0 / 256 - 1)
    for key, want in (("power_mean", (c * c).mean(axis=0)), ("coef_mean", c.mean(axis=0)), ("coef_var", c.var(axis=0)),
                      ("radial_mean", so.radial(c).mean(axis=0))):
        assert one[key].shape == want.shape and np.allclose(one[key], want, rtol=1e-9, atol=1e-12), key
        assert np.allclose(parts[key], one[key], rtol=1e-12, atol=1e-14), key
    assert one["n"] == parts["n"] == 50 and one["radial_freq"].shape == (45,)
    assert one["radial"].shape == (50, 45, 3) and np.array_equal(one["radial"], parts["radial"])
    assert "radial" not in sp.image_spectrum(images[:3], device="cpu")
    g = sp.image_spectrum(images[:7], gray=True, chunk=4, device="cpu")
    assert g["power_mean"].shape == (32, 32, 1) and g["radial_mean"].shape == (45, 1) and calls[-1][3] is True


def test_dct2_equals_grey_then_dctn(monkeypatch, images):
    fft = pytest.importorskip("scipy.fft")
    from mulan_amd import spectrum as sp
    _stand_in(monkeypatch, [])
    img = images[7]
    grey = (img / 255.0) @ np.array(so.GRAY)                                     # skimage.color.rgb2gray of a uint8 image
    want = fft.dctn(grey, norm="ortho")
    got = sp.dct2(img, device="cpu")
    assert got.shape == (32, 32) and got.dtype == np.float32 and np.abs(got - want).max() < 2e-6
    batch = sp.dct2(images[:3], device="cpu")
    assert batch.shape == (3, 32, 32) and np.array_equal(batch[0], sp.dct2(images[0], device="cpu"))
    f = (img / 255.0).astype(np.float32)                                        # floats are taken as they are
    assert np.abs(sp.dct2(torch.from_numpy(f), device="cpu") - want).max() < 2e-6


def test_notebook_utils_reexports_the_module_objects():
    from ldm import notebook_utils as nu
    from mulan_amd import spectrum as sp
    assert nu.dct2 is sp.dct2 and nu.image_spectrum is sp.image_spectrum and nu.compare_spectra is sp.compare_spectra
    assert nu.schedule_spectrum is sp.schedule_spectrum and nu.plot_spectra is sp.plot_spectra


def test_plot_draws_both_panels(monkeypatch, images):
    pytest.importorskip("matplotlib")
    import matplotlib
    matplotlib.use("Agg")
    import matplotlib.pyplot as plt
    from mulan_amd import spectrum as sp
    _stand_in(monkeypatch, [])
    a, b = sp.image_spectrum(images[:5], device="cpu"), sp.image_spectrum(images[5:12], device="cpu")
    fig = sp.plot_spectra([a, b], labels=["samples", "train"], comparison=sp.compare_spectra(a, b))
    assert len(fig.axes) == 2
    plt.close(fig)
    fig = sp.plot_spectra(a)
    assert len(fig.axes) == 1
    plt.close(fig)


# ------------------------------------------------------------------------------------------------ the command line
def _args(tmp_path, *more, reference=None):
    return [f"--samples={tmp_path / 's.npz'}", f"--reference={reference or 'npz:' + str(tmp_path / 't.npz')}",
            f"--out={tmp_path / 'n.npz'}", *more]


def test_cli_flag_parsing(tmp_path, monkeypatch):
    from ldm import spectrum as cli
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    with pytest.raises(SystemExit, match="no file"):
        cli.parse_flags(_args(tmp_path))
    np.savez(tmp_path / "s.npz", images=np.zeros((2, 32, 32, 3), np.uint8))
    f = cli.parse_flags(_args(tmp_path))
    assert (f.gray, f.max_reference, f.chunk) == (False, 0, 16384)
    f = cli.parse_flags(_args(tmp_path, "--gray", "--max_reference", "100", "--chunk=64"))
    assert (f.gray, f.max_reference, f.chunk) == (True, 100, 64)
    assert cli.parse_flags(_args(tmp_path, reference="imagenet32")).reference == "imagenet32"
    for more, match in ((["--chunk=0"], "--chunk"), (["--max_reference=-1"], "--max_reference")):
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


def test_cli_writes_the_documented_keys_over_the_stand_in(tmp_path, monkeypatch, images):
    from ldm import spectrum as cli
    from mulan_amd import spectrum as sp
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    _stand_in(monkeypatch, [])
    monkeypatch.setattr(sp, "_default_device", lambda: "cpu")
    samples, train = images[:5], images[5:14]
    np.savez(tmp_path / "s.npz", images=samples)
    np.savez(tmp_path / "t.npz", images=train)
    assert cli.main(_args(tmp_path, "--max_reference=8", "--chunk=3")) == 0
    keys = ["samples_" + k for k in cli.SET_KEYS] + ["reference_" + k for k in cli.SET_KEYS] + list(cli.COMPARE_KEYS)
    with np.load(tmp_path / "n.npz") as f:
        assert sorted(f.files) == sorted(keys + ["radial_freq", "settings"])
        assert f["samples_radial_mean"].shape == (45, 3) and f["reference_power_mean"].shape == (32, 32, 3)
        assert int(f["samples_n"]) == 5 and int(f["reference_n"]) == 8 and f["log_ratio"].shape == (45, 3)
        want = sp.compare_spectra(sp.image_spectrum(samples), sp.image_spectrum(train[:8]))
        assert np.isclose(float(f["lsd_db"]), want["lsd_db"]) and np.isclose(float(f["frechet_diag"]), want["frechet_diag"])
        s = json.loads(str(f["settings"]))
        assert s["n_reference"] == 8 and s["n_samples"] == 5 and s["gray"] is False and s["chunk"] == 3
    assert cli.main(_args(tmp_path, "--gray")) == 0
    with np.load(tmp_path / "n.npz") as f:
        assert f["samples_coef_var"].shape == (32, 32, 1) and int(f["reference_n"]) == 9
    np.savez(tmp_path / "s.npz", pictures=samples)
    with pytest.raises(SystemExit, match="holds no `images`"):
        cli.main(_args(tmp_path))
