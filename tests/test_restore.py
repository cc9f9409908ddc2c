"""Restoration with the few-step samplers (mulan_amd.sampling.run): the degradation grammar, the refusals, the
two C ABI entry points in the header and the binding table, the flags of `python -m ldm.sample` and the float64 oracle
(tests/restore_oracle.py) against its known answers -- everything that runs without a GPU."""
import os
import re

import numpy as np
import pytest
import torch

from tests import restore_oracle as ro
from tests import stochastic_sampler_oracle as so

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONFIG = os.path.join(ROOT, "ldm", "configs", "cifar10-conditioned.py")


# ------------------------------------------------------------------------------------- the boundary
@pytest.mark.parametrize("entry,n_args,args", [
    ("mulan_restore_project", 14, {3: "const float* y", 4: "float* xh_out", 5: "int B", 9: "int f", 10: "int gray",
                                   11: "int mode", 12: "int g_per_sample", 13: "mulan_stream_t stream"}),
    ("mulan_restore_measure", 9, {0: "const float* x", 1: "float* y_out", 6: "int f", 7: "int gray"})])
def test_header_declares_the_entry_points_and_the_binding_has_their_arity(entry, n_args, args):
    from mulan_amd import lib
    with open(os.path.join(ROOT, "include", "mulan_hip.h")) as f:
        header = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    m = re.search(r"int\s+%s\s*\(([^;]*)\)\s*;" % entry, header)
    assert m, f"{entry} is not declared in include/mulan_hip.h"
    decl = [" ".join(a.split()) for a in m.group(1).split(",") if a.strip()]
    assert len(decl) == n_args and all(decl[i] == a for i, a in args.items()), decl
    sig = lib.SIGNATURES[entry]
    n_ptr = sum('*' in d for d in decl)
    assert len(sig) == n_args and sig[-1] is lib.P and [t is lib.P for t in sig[:-1]] == [i < n_ptr for i in range(n_args - 1)]
    assert all(t is lib.I for t in sig[n_ptr:-1])


# ------------------------------------------------------------------------------------- the grammar and the refusals
def test_parse_degradation():
    from mulan_amd import sampling
    assert sampling.parse_degradation("sr:4") == (4, False)
    assert sampling.parse_degradation("gray") == (1, True)
    assert sampling.parse_degradation("sr:4+gray") == (4, True)
    for f in (2, 4, 8, 16):
        assert sampling.parse_degradation(f"sr:{f}") == (f, False) and sampling.parse_degradation(f"sr:{f}+gray") == (f, True)
        assert sampling.parse_degradation((f, True)) == (f, True)
    for spec, (f, gray) in ro.SPECS.items():
        assert sampling.parse_degradation(spec) == (f, gray)
    for bad in ("sr:3", "sr:1", "sr:32", "sr:", "sr", "sr4", "sr:4+", "sr:4+grey", "gray+sr:4", "grey", "GRAY", "", "sr:04",
                "sr:4+gray+gray", "blur", None, 4, (1, False), (3, True), (4,)):
        with pytest.raises(ValueError) as e:
            sampling.parse_degradation(bad)
        msg = str(e.value)                                  # the grammar is in the message
        assert "'sr:f'" in msg and "'gray'" in msg and "'sr:f+gray'" in msg and "2, 4, 8, 16" in msg, msg


def test_check_restore():
    from mulan_amd import sampling
    y, x, m = torch.zeros(1, 8, 8, 3), torch.zeros(1, 3072), torch.ones(1, 3072, dtype=torch.uint8)
    assert sampling.check_restore("dpm2m", None, None) is False
    assert sampling.check_restore("ancestral", None, None, 1, None, None) is False
    for sampler in sampling.FAST_SAMPLERS:
        assert sampling.check_restore(sampler, y, "sr:4") is True
        assert sampling.check_restore(sampler, y, "sr:4", 3) is True            # resample > 1 is allowed
    assert sampling.check_restore("dpm2m", None, None, 2, x, m) is False        # ... with inpainting too
    assert sampling.check_inpaint("dpm2m", x, m, 2) is True
    with pytest.raises(ValueError, match="together"):
        sampling.check_restore("dpm2m", y, None)
    with pytest.raises(ValueError, match="together"):
        sampling.check_restore("dpm2m", None, "sr:4")
    with pytest.raises(ValueError, match="ancestral"):
        sampling.check_restore("ancestral", y, "sr:4")
    with pytest.raises(ValueError, match="mask and a measurement"):
        sampling.check_restore("dpm2m", y, "sr:4", 1, x, m)
    with pytest.raises(ValueError, match="mask and a measurement"):
        sampling.check_restore("dpm2m", y, "sr:4", 1, None, m)
    for resample in (0, -1, 1.5, None, True, "2", float("nan")):
        with pytest.raises(ValueError, match="resample"):
            sampling.check_restore("dpm2m", y, "sr:4", resample)
    with pytest.raises(ValueError, match="sr:f"):
        sampling.check_restore("dpm2m", y, "sr:3")
    with pytest.raises(ValueError, match="unknown sampler"):
        sampling.check_restore("dpm3", y, "sr:4")
    # the same refusals from the loop's front door, before any kernel runs
    net, gam, z = (lambda z, t: z), (lambda t: torch.zeros(1)), torch.zeros(1, 32, 32, 3)
    with pytest.raises(ValueError, match="together"):
        sampling.sample(net, gam, z, 2, "dpm2m", steps=2, measurement=y)
    with pytest.raises(ValueError, match="mask and a measurement"):
        sampling.sample(net, gam, z, 2, "dpm2m", steps=2, measurement=y, degradation="sr:4", known=x, mask=m,
                        known_noise_fn=lambda j: x)
    with pytest.raises(ValueError, match="resample"):
        sampling.sample(net, gam, z, 2, "dpm2m", steps=2, measurement=y, degradation="sr:4", resample=0)
    with pytest.raises(ValueError, match="resample"):            # and without a measurement or a mask, as before
        sampling.sample(net, gam, z, 2, "dpm2m", steps=2, resample=2)


def test_a_restoring_stepper_needs_both_and_excludes_a_mask():
    from mulan_amd import sampling
    y, x, m = torch.zeros(1, 8, 8, 3), torch.zeros(1, 4), torch.ones(1, 4, dtype=torch.uint8)
    args = (lambda z, t: z, lambda t: torch.zeros(1), 2)
    with pytest.raises(ValueError, match="together"):
        sampling.EagerStepper(*args, measurement=y)
    with pytest.raises(ValueError, match="together"):
        sampling.EagerStepper(*args, degradation="sr:4")
    with pytest.raises(ValueError, match="mask and a measurement"):
        sampling.EagerStepper(*args, known=x, mask=m, known_noise_fn=lambda j: x, measurement=y, degradation="sr:4")
    st = sampling.EagerStepper(*args, measurement=y, degradation="sr:4+gray")
    assert st.restore and not st.inpaint and st.degradation == (4, True)
    assert not sampling.EagerStepper(*args).restore
    with pytest.raises(ValueError, match="known_noise_fn"):            # a jump needs its noise
        st.jump(x, 0.5, 1.0, 0)


# ------------------------------------------------------------------------------------- the oracle's known answers
def _image(seed, B=3, H=32, W=32, C=3):
    gen = torch.Generator().manual_seed(seed)
    return 2 * torch.rand(B, H, W, C, generator=gen, dtype=torch.float64) - 1


@pytest.mark.parametrize("spec", sorted(ro.SPECS))
def test_oracle_known_answers(spec):
    f, gray = ro.SPECS[spec]
    x = _image(1)
    B, H, W, C = x.shape
    y = ro.measure(_image(2), f, gray)
    assert tuple(y.shape) == (B, H // f, W // f, 1 if gray else C)
    n_g = ro.group_size(f, gray)
    assert x.numel() // y.numel() == n_g
    # the groups are what the table says: the mean of the members named one by one
    h, w, c = 5, 9, 1
    members = [x[0, (h // f) * f + dy, (w // f) * f + dx, cc] for dy in range(f) for dx in range(f)
               for cc in (range(C) if gray else [c])]
    assert len(members) == n_g
    assert abs(float(ro.measure(x, f, gray)[0, h // f, w // f, 0 if gray else c]) - float(sum(members)) / n_g) < 1e-15
    # A A+ y == y exactly
    up = ro.replicate(y, f, gray)
    assert up.shape == x.shape and torch.equal(ro.measure(up, f, gray), y)
    # A x' == y to 1e-14, projection idempotent, within-group differences preserved
    p = ro.project(x, y, f, gray)
    assert float((ro.measure(p, f, gray) - y).abs().max()) < 1e-14
    assert float((ro.project(p, y, f, gray) - p).abs().max()) < 1e-14
    shift = p - x                                          # one value per group: x' - x is constant on a group
    assert float((shift - ro.replicate(ro.measure(shift, f, gray), f, gray)).abs().max()) < 1e-14
    # a prediction that already satisfies the measurement stays where it is
    assert float((ro.project(up, y, f, gray) - up).abs().max()) == 0.0


@pytest.mark.parametrize("sampler", ["ddim", "dpm2m"])
@pytest.mark.parametrize("spec", ["sr:4", "gray", "sr:2+gray"])
def test_closed_form_on_a_constant_denoiser(sampler, spec):
    """a denoiser that returns the constant image c as x_hat (kind 'input'), per-element gammas drawn at random and
    increasing in t: every step's projected prediction is c' = c + A+ (y - A c), a constant prediction makes D = x_hat'
    at both orders, and the DDIM steps telescope:  z_0 = (sigma_0 / sigma_1) z_1 + (alpha_0 - alpha_1 sigma_0 / sigma_1) c'
    element by element, where 0 and 1 name the schedule's ends"""
    f, gray = ro.SPECS[spec]
    B, N = 2, 5
    gen = torch.Generator().manual_seed(7)
    shp = (B, 32, 32, 3)
    g0 = -13.3 + torch.rand(shp, generator=gen, dtype=torch.float64)
    rate = 10.0 + 8.0 * torch.rand(shp, generator=gen, dtype=torch.float64)
    bend = torch.rand(shp, generator=gen, dtype=torch.float64)
    gamma = lambda t: g0 + rate * (t + bend * t * t) / (1 + bend)             # strictly increasing in t, per element
    c, z1 = _image(3, B), torch.randn(shp, generator=gen, dtype=torch.float64)
    y = ro.measure(_image(4, B), f, gray)
    grid = [1.0 - k / N for k in range(N + 1)]
    calls = []

    def net_fn(z, g_t):
        calls.append(1)
        return c
    z0, events = ro.loop(gamma, net_fn, z1, grid, sampler, 0.0, "input", y, f, gray, None, None)
    assert len(calls) == N and [e["order"] for e in events] == so.orders(sampler, N)
    cp = ro.project(c, y, f, gray)
    assert all(torch.equal(e["xh"], cp) for e in events)                     # the history is x_hat', not x_hat
    al = lambda g: torch.sqrt(torch.sigmoid(-g))
    si = lambda g: torch.sqrt(torch.sigmoid(g))
    ga, gb = gamma(0.0), gamma(1.0)
    want = si(ga) / si(gb) * z1 + (al(ga) - al(gb) * si(ga) / si(gb)) * cp
    assert float((z0 - want).abs().max()) < 1e-12 * float(want.abs().max())
    # with time travel (U = 2, zero jump noise is not the identity: the jump rescales z), the loop still only ever
    # predicts c': after the last step z_0 = (sigma_0 / sigma_t) z_t + (alpha_0 - alpha_t sigma_0 / sigma_t) c'
    xi = torch.randn(shp, generator=gen, dtype=torch.float64)
    z0u, ev = ro.loop(gamma, net_fn, z1, grid, sampler, 0.0, "input", y, f, gray, None, lambda j: xi, resample=2)
    steps = [e for e in ev if e["kind"] == "step"]
    assert len(steps) == 2 * N - 1 and [e["j"] for e in ev if e["kind"] == "jump"] == list(range(N - 1))
    assert [e["kk"] for e in steps] == [v for k in range(N - 1) for v in (k, k + N)] + [N - 1]
    assert all(e["order"] == 1 for e in steps if e["kk"] >= N)
    last = steps[-1]
    gt = gamma(last["t"])
    want = si(ga) / si(gt) * last["z_in"] + (al(ga) - al(gt) * si(ga) / si(gt)) * cp
    assert float((z0u - want).abs().max()) < 1e-12 * float(want.abs().max())


# ------------------------------------------------------------------------------------- the command line
def _base_args(tmp_path):
    (tmp_path / "ckpt-3").mkdir(exist_ok=True)
    return [f"--config={CONFIG}", f"--checkpoint_directory={tmp_path}", f"--out={tmp_path}/s.npz"]


def _file(tmp_path, name="in.npz", **arrays):
    if not arrays:
        arrays = dict(images=np.random.default_rng(3).integers(0, 256, (5, 32, 32, 3)).astype(np.uint8))
    np.savez(tmp_path / name, **arrays)
    return f"--restore_images={tmp_path / name}"


def test_sample_cli_takes_images_or_a_measurement(tmp_path):
    from ldm import sample
    flags, _, inpaint, restore, given = sample.parse_all(_base_args(tmp_path) + [_file(tmp_path), "--resample=2"])
    assert inpaint is None and flags.n_samples is None and flags.resample == 2
    assert restore.array.shape == (5, 32, 32, 3) and restore.degrade and given is restore.array
    assert (restore.f, restore.gray, restore.spec) == (4, False, "sr:4")                                  # the default
    meas = _file(tmp_path, "y.npz", measurement=np.zeros((3, 8, 8, 1), np.float32))
    flags, _, _, restore, given = sample.parse_all(_base_args(tmp_path) + [meas, "--degradation=sr:4+gray",
                                                                           "--sampler=sde2m", "--embedding=encoder",
                                                                           "--n_samples=2"])
    assert not restore.degrade and restore.array.shape == (3, 8, 8, 1) and given is restore.array
    assert (restore.f, restore.gray) == (4, True) and flags.n_samples == 2
    levels = _file(tmp_path, "u8.npz", measurement=np.zeros((3, 32, 32, 1), np.uint8))
    assert sample.parse_all(_base_args(tmp_path) + [levels, "--degradation=gray"])[3].array.dtype == np.uint8
    flags, _, inpaint, restore, given = sample.parse_all(_base_args(tmp_path) + ["--n_samples=4"])      # as before
    assert inpaint is None and restore is None and given is None and flags.restore_images is None and flags.degradation is None


def test_sample_cli_refusals(tmp_path):
    from ldm import sample
    base = _base_args(tmp_path)
    img = _file(tmp_path)
    np.savez(tmp_path / "inp.npz", images=np.zeros((5, 32, 32, 3), np.uint8))
    both = _file(tmp_path, "both.npz", images=np.zeros((2, 32, 32, 3), np.uint8), measurement=np.zeros((2, 8, 8, 3), np.float32))
    none = _file(tmp_path, "none.npz", pictures=np.zeros((2, 32, 32, 3), np.uint8))
    shape = _file(tmp_path, "shape.npz", measurement=np.zeros((2, 8, 8, 3), np.float32))
    f64 = _file(tmp_path, "f64.npz", measurement=np.zeros((2, 8, 8, 3), np.float64))
    for args, match in (
            ([img, f"--inpaint_images={tmp_path / 'inp.npz'}", "--mask=half:left"], "exclude"),
            (["--n_samples=4", "--degradation=sr:4"], "degradation"),                # a degradation without images
            ([img, "--sampler=ancestral"], "ancestral"),
            ([img, "--degradation=sr:3"], "sr:f"),
            ([img, "--degradation=blur"], "degradation"),
            ([img, "--resample=0"], "resample"),
            ([img, "--mask=half:left"], "mask"),                                     # a mask belongs to inpainting
            ([img, "--n_samples=6"], "n_samples"),
            ([both], "one of the two"),
            ([none], "one of the two"),
            ([shape, "--degradation=sr:4+gray"], "measurement"),
            ([shape, "--degradation=sr:2"], "measurement"),
            ([f64], "measurement"),
            ([f"--restore_images={tmp_path / 'missing.npz'}"], "cannot read"),
            (["--n_samples=4", "--resample=2"], "resample"),
            ([], "n_samples")):
        with pytest.raises(SystemExit, match=match):
            sample.parse_flags(base + args)


# ------------------------------------------------------------------------------------- the loop and the one check
@pytest.mark.parametrize("sampler,eta,U,N", [("dpm2m", 0.0, 1, 4), ("sde2m", 1.0, 2, 4), ("ddim", 0.5, 3, 3),
                                             ("dpm2m", 0.0, 2, 15)])
def test_run_asks_a_restoring_stepper_for_steps_and_jumps_only(sampler, eta, U, N):
    """sampling.run driven with a recording stepper that restores: step k at the schedule's order and no `mix`; after
    every step but the last, rounds r = 1 .. U - 1 of a jump s -> t on j = 0, 1, 2, ... counted over the whole run,
    then the step again at first order under the index k + r N; U = 1 draws no j at all"""
    from mulan_amd import sampling
    from tests.test_inpaint import _Recorder
    f32 = lambda v: float(np.float32(v))
    grid, orders = sampling.time_grid(N), sampling.step_orders(sampler, N)
    want, j = [], 0
    for k in range(N):
        t, s = f32(grid[k]), f32(grid[k + 1])
        want.append(("step", orders[k], k, None, t, s))
        for r in range(1, U if k < N - 1 else 1):
            want += [("jump", None, None, j, t, s), ("step", 1, k + r * N, None, t, s)]
            j += 1
    rec = _Recorder(sampling.check_eta(sampler, eta if sampler == "ddim" else 0.0), inpaint=False, restore=True)
    z = torch.zeros(1, 4)
    assert sampling.run(rec, z, grid, orders, U) is z
    assert rec.log == want
    steps, jumps = ([e for e in rec.log if e[0] == kind] for kind in ("step", "jump"))
    assert len(steps) == N + (U - 1) * (N - 1) and len(jumps) == (U - 1) * (N - 1)
    assert [e[3] for e in jumps] == list(range(len(jumps))) and not any(e[0] == "mix" for e in rec.log)


def _guidance_on_the_parent(sampler, known, mask, measurement, degradation, resample):
    """the three public checks in the order every layer used to spell out -> (inpaint, restore, resample)"""
    from mulan_amd import sampling
    restoring = sampling.check_restore(sampler, measurement, degradation, resample, known, mask)
    inpaint = sampling.check_inpaint(sampler, known, mask, 1 if restoring else resample)
    return inpaint, sampling.parse_degradation(degradation) if restoring else None, sampling.check_resample(resample)


_X, _M, _Y = torch.zeros(1, 4), torch.ones(1, 4, dtype=torch.uint8), torch.zeros(1, 2, 2, 3)


@pytest.mark.parametrize("sampler,known,mask,measurement,degradation,resample", [
    ("dpm2m", None, None, None, None, 1),                     # nothing given
    ("ancestral", None, None, None, None, 1),
    ("dpm3", None, None, None, None, 1),                      # no such sampler
    ("dpm2m", _X, _M, None, None, 1), ("sde2m", _X, _M, None, None, 3),
    ("dpm2m", None, None, _Y, "sr:4", 1), ("ddim", None, None, _Y, (2, True), 2), ("sde2m", None, None, _Y, "gray", 1),
    ("dpm2m", None, _M, None, None, 1), ("dpm2m", _X, None, None, None, 1),           # one without the other
    ("dpm2m", None, None, _Y, None, 1), ("dpm2m", None, None, None, "sr:4", 1),
    ("dpm2m", _X, _M, _Y, "sr:4", 1), ("dpm2m", None, _M, _Y, "sr:4", 2),             # both kinds at once
    ("dpm2m", _X, _M, None, "sr:4", 1), ("dpm2m", _X, _M, _Y, None, 1),
    ("ancestral", _X, _M, None, None, 1), ("ancestral", None, None, _Y, "sr:4", 1),
    ("ancestral", _X, _M, _Y, "sr:4", 1),
    ("dpm2m", None, None, None, None, 0), ("dpm2m", None, None, None, None, 1.5), ("dpm2m", None, None, None, None, True),
    ("dpm2m", None, None, None, None, None), ("dpm2m", None, None, None, None, 2),    # resample without guidance
    ("dpm2m", _X, _M, None, None, 0), ("dpm2m", None, None, _Y, "sr:4", 1.5), ("dpm2m", None, None, _Y, "sr:4", None),
    ("dpm2m", _X, _M, None, None, 2.0),
    ("dpm2m", None, None, _Y, "sr:3", 1), ("dpm2m", None, None, _Y, "gray+sr:2", 2), ("dpm2m", None, None, _Y, (1, False), 1),
    ("dpm2m", _X, _M, _Y, "sr:3", 1)])                        # a malformed degradation
def test_check_guidance_is_the_three_checks_in_their_order(sampler, known, mask, measurement, degradation, resample):
    """check_guidance returns what check_restore, check_inpaint and parse_degradation decide, or raises the first
    error that sequence raises: the same type and the same text"""
    from mulan_amd import sampling
    args = (sampler, known, mask, measurement, degradation, resample)
    try:
        want = _guidance_on_the_parent(*args)
    except (ValueError, TypeError) as e:
        with pytest.raises(type(e)) as got:
            sampling.check_guidance(*args)
        assert type(got.value) is type(e) and str(got.value) == str(e)
        return
    got = sampling.check_guidance(*args)
    assert tuple(got) == want and (got.inpaint, got.restore, got.resample) == want
    assert type(got.resample) is int and type(got.inpaint) is bool
    with pytest.raises(AttributeError):
        got.resample = 7                                      # the record is immutable
