"""mulan_schedule_curves on the MI355X against float64 (tests/schedule_curves_oracle.py: oracle.torch_ref.poly_gamma and
the bounds measured by tests/test_schedule_curves.py on the CPU, 4 x the error of the fp32 restatement), its exact
properties (t = 0, histogram rows, determinism, summary-only mode, refusals), the parent's ops.poly_gamma as a yardstick,
and noise_schedule_per_embedding / noise_schedule_summary on a small MuLAN model against its float64 parameters."""
import functools
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import torch_ref as tr
from tests import schedule_curves_oracle as sco

GMIN, GMAX = sco.GMIN, sco.GMAX
GAMMA_BOUND, STATS_BOUND = sco.GAMMA_BOUND, np.array(sco.STATS_BOUND)
TUNE_CHUNK = 30                        # mulan_set_tuning word: times per block (0: the launch chooses)


def dev(v):
    return torch.from_numpy(np.array(v)).cuda()


@functools.lru_cache(maxsize=None)
def case(name, E, T, seed=0):
    """(a, b, c, t) fp32 and the float64 gamma [E, T, 3072] of one family: computed once, shared, never written"""
    a, b, c = sco.channel_family(E, seed) if name == "channels" else sco.family(name, E, seed)
    t = sco.grid_times(T)
    g64 = sco.gamma64(a, b, c, t)
    for v in (a, b, c, t, g64):
        v.setflags(write=False)
    return a, b, c, t, g64


def run(a, b, c, t, **kw):
    from mulan_amd import ops
    out = ops.schedule_curves(dev(a), dev(b), dev(c), dev(t), GMIN, GMAX, **kw)
    return tuple(None if o is None else o.cpu().numpy() for o in out)


@pytest.fixture
def chunk():
    """forces the times per block (the launch's own choice gives these small shapes one time per block)"""
    from mulan_amd import ops

    def force(n):
        ops.call("mulan_set_tuning", TUNE_CHUNK, n)
    yield force
    ops.call("mulan_set_tuning", TUNE_CHUNK, 0)


def check_against_float64(g, s, h, t, g64, bins):
    gmin32 = np.float32(GMIN)
    err = np.abs(g - g64).max()
    serr = np.abs(s - sco.stats_of(g64)).reshape(-1, 8).max(0)
    print(f"gamma {err:.3e} (bound {GAMMA_BOUND:.3e}) stats", " ".join(f"{v:.2e}" for v in serr))
    assert err <= GAMMA_BOUND
    assert (serr <= STATS_BOUND).all(), dict(zip(sco.STAT_NAMES, serr))
    zero, one = t == 0, t == 1
    assert (g[:, zero] == gmin32).all()                                   # bit for bit
    assert (s[:, zero, 1] == 0).all() and (s[:, zero, 0] == gmin32).all()
    assert (s[:, zero, 2] == gmin32).all() and (s[:, zero, 3] == gmin32).all()
    assert (np.abs(g[:, one] - GMAX) <= GAMMA_BOUND).all()
    assert (h.sum(-1) == sco.D).all()
    assert np.array_equal(h, sco.binning32(g, bins))                      # the kernel's own gammas, binned in numpy fp32
    l1 = np.abs(h - sco.hist64(g64, bins)).sum(-1)
    near = sco.near_edge(g64, bins, GAMMA_BOUND)
    assert (near <= 0.01 * sco.D).all() and (l1 <= 2 * near).all(), (int(l1.max()), int(near.max()))


@pytest.mark.parametrize("E", [1, 3])
@pytest.mark.parametrize("T", [1, 2, 7, 128, 130])
def test_all_outputs_against_float64(E, T, chunk):
    """every (E, T): the launch's own geometry (one time per block at these sizes), then 8 and 16 times per block -- one
    block per embedding up to T = 7, a ragged last chunk at T = 7, 130 and more than one chunk at T = 128, 130; all three
    geometries give the same bits"""
    a, b, c, t, g64 = case("normal", E, T, seed=1)
    bins = 100
    first = None
    for n in (0, 8, 16):
        chunk(n)
        g, s, h = run(a, b, c, t, curves=True, stats=True, bins=bins)
        assert g.shape == (E, T, sco.D) and s.shape == (E, T, 8) and h.shape == (E, T, bins) and h.dtype == np.int32
        if first is None:
            first = (g, s, h)
            check_against_float64(g, s, h, t, g64, bins)
        else:
            assert all(np.array_equal(x, y) for x, y in zip(first, (g, s, h))), n


@pytest.mark.parametrize("bins", [1, 100, 256])
@pytest.mark.parametrize("T", [7, 130])
def test_histogram_bin_counts(bins, T, chunk):
    a, b, c, t, g64 = case("normal", 3, T, seed=1)
    chunk(8)
    g, s, h = run(a, b, c, t, curves=True, stats=True, bins=bins)
    check_against_float64(g, s, h, t, g64, bins)
    if bins == 1:
        assert (h == sco.D).all()


@pytest.mark.parametrize("name", sco.FAMILIES + ("channels",))
def test_families_against_float64_and_the_parent(name):
    """per family: gamma and the statistics within the bounds, and gamma at least as close to float64 as the parent's
    ops.poly_gamma on the same inputs (one launch per time, one t per row)"""
    from mulan_amd import ops
    E, T = 3, 7
    a, b, c, t, g64 = case(name, E, T)
    g, s, h = run(a, b, c, t, curves=True, stats=True, bins=100)
    err = np.abs(g - g64).max()
    serr = np.abs(s - sco.stats_of(g64)).reshape(-1, 8).max(0)
    da, db, dc = dev(a), dev(b), dev(c)
    parent = np.stack([ops.poly_gamma(da, db, dc, torch.full((E,), float(tv), device="cuda"), GMIN, GMAX)[2].cpu().numpy()
                       for tv in t], axis=1)
    perr = np.abs(parent - g64).max()
    print(f"{name}: gamma {err:.3e}, parent {perr:.3e}, stats", " ".join(f"{v:.2e}" for v in serr))
    assert err <= GAMMA_BOUND and (serr <= STATS_BOUND).all(), dict(zip(sco.STAT_NAMES, serr))
    assert err <= perr
    assert (g[:, t == 0] == np.float32(GMIN)).all() and (h.sum(-1) == sco.D).all()
    if name == "linear":
        closed = np.abs(s - sco.linear_closed_form(t)[None]).reshape(-1, 8).max(0)
        assert (closed <= STATS_BOUND).all(), dict(zip(sco.STAT_NAMES, closed))
    if name == "channels":      # a rotation of the channels would miss by more than 1
        want = sco.stats_of(g64)[..., 4:7]
        assert np.abs(s[..., 4:7] - want).max() <= STATS_BOUND[4]
        assert np.abs(s[..., [5, 6, 4]] - want).max() > 1.0 and np.abs(s[..., [6, 4, 5]] - want).max() > 1.0


def test_each_output_alone_and_twice(chunk):
    """each of the three outputs alone equals its part of the launch with all three; a second launch gives the same bits"""
    a, b, c, t, _ = case("normal", 3, 130, seed=1)
    chunk(16)
    g, s, h = run(a, b, c, t, curves=True, stats=True, bins=256)
    g2, s2, h2 = run(a, b, c, t, curves=True, stats=True, bins=256)
    assert np.array_equal(g, g2) and np.array_equal(s, s2) and np.array_equal(h, h2)
    only = run(a, b, c, t)
    assert only[1] is None and only[2] is None and np.array_equal(only[0], g)
    only = run(a, b, c, t, curves=False, stats=True)
    assert only[0] is None and only[2] is None and np.array_equal(only[1], s)
    only = run(a, b, c, t, curves=False, bins=256)
    assert only[0] is None and only[1] is None and np.array_equal(only[2], h)


def _raw(lib_, a, b, c, t, E, T, gamma, stats, hist, bins, gmin=GMIN, gmax=GMAX, d=sco.D):
    p = lambda x: None if x is None else x.data_ptr()
    return lib_.mulan_schedule_curves(p(a), p(b), p(c), E, d, p(t), T, gmin, gmax, p(gamma), p(stats), p(hist), bins,
                                      torch.cuda.current_stream().cuda_stream)


def test_summary_only_leaves_a_poisoned_curve_buffer_alone():
    """summary-only through the C ABI (gamma_out NULL): the statistics and the histogram lie inside one poisoned buffer of
    the caller's, with room for a whole [E, T, 3072] set of curves before and after them; only the E T (8 + bins) words
    asked for change"""
    from mulan_amd import lib
    L = lib.load()
    E, T, bins = 3, 7, 100
    a, b, c, t, g64 = case("normal", E, T, seed=1)
    da, db, dc, dt = dev(a), dev(b), dev(c), dev(t)
    G, S, H = E * T * sco.D, E * T * 8, E * T * bins
    POISON = 0x7FC0DEAD                                                  # (a NaN as a float)
    arena = torch.full((G + S + H + G,), POISON, device="cuda", dtype=torch.int32)
    stats = arena[G:G + S].view(torch.float32).view(E, T, 8)
    hist = arena[G + S:G + S + H].view(E, T, bins)
    assert _raw(L, da, db, dc, dt, E, T, None, stats, hist, bins) == 0
    torch.cuda.synchronize()
    assert bool((arena[:G] == POISON).all()) and bool((arena[G + S + H:] == POISON).all())
    assert (np.abs(stats.cpu().numpy() - sco.stats_of(g64)).reshape(-1, 8).max(0) <= STATS_BOUND).all()
    assert bool((hist.sum(-1) == sco.D).all())
    from mulan_amd import ops
    before = torch.cuda.memory_allocated()
    g, s, h = ops.schedule_curves(da, db, dc, dt, GMIN, GMAX, curves=False, stats=True, bins=bins)
    assert g is None and torch.cuda.memory_allocated() - before < G * 4   # no curve buffer behind the caller's back
    assert np.array_equal(s.cpu().numpy(), stats.cpu().numpy()) and bool((h == hist).all())


def test_invalid_arguments_return_the_error_without_launching():
    from mulan_amd import lib
    L = lib.load()
    INVALID = 1                                        # hipErrorInvalidValue
    E, T = 2, 3
    a = torch.ones((E, sco.D), device="cuda")
    t = torch.zeros(T, device="cuda")
    gamma = torch.full((E, T, sco.D), 7.0, device="cuda")
    stats = torch.full((E, T, 8), 7.0, device="cuda")
    hist = torch.full((E, T, 16), 7, device="cuda", dtype=torch.int32)
    ok = dict(a=a, b=a, c=a, t=t, E=E, T=T, gamma=gamma, stats=stats, hist=hist, bins=16)
    bad = [dict(a=None), dict(b=None), dict(c=None), dict(t=None), dict(gamma=None, stats=None, hist=None),
           dict(d=1024), dict(E=0), dict(T=0), dict(bins=0), dict(bins=257), dict(gmin=5.0, gmax=5.0),
           dict(gmin=5.0, gmax=-13.3)]
    for change in bad:
        assert _raw(L, **{**ok, **change}) == INVALID, change
    torch.cuda.synchronize()
    assert bool((gamma == 7).all()) and bool((stats == 7).all()) and bool((hist == 7).all())
    assert _raw(L, **{**ok, "hist": None, "bins": 0}) == 0          # bins is read only with hist_out
    torch.cuda.synchronize()
    assert bool((gamma[:, 0] == np.float32(GMIN)).all())


# ----------------------------------------------------------------------------- model level
@pytest.fixture(scope="module")
def mulan():
    """a small MuLAN model and its float64 parameters, built as tests/test_gpu_latent_types.py builds them: the oracle's
    init_params in float64, copied into the model's layout in fp32"""
    from mulan_amd import model as M
    from mulan_amd.model import VDMConfig
    from mulan_amd.rng import PRNGKey
    cfg = VDMConfig(vocab_size=256, sample_softmax=False, antithetic_time_sampling=True, with_fourier_features=True,
                    with_attention=False, gamma_type='poly_fixedend', gamma_min=GMIN, gamma_max=GMAX, sm_n_timesteps=0,
                    sm_n_embd=128, sm_n_layer=1, sm_pdrop=0.1, forward_n_layer=1, latent_size=50, latent_k=15,
                    encoder='unet', latent_type='topk', z_conditioning=True, reparam_type='true', unet_type='vdm',
                    velocity_from_epsilon=False, condition='input', sigma_type='no_blur', sigma_prior=1.0)
    ocfg = dict(vdm_type='mulan_velocity', n_embd=128, n_layer=1, forward_n_layer=1, latent_k=15, unet_type='vdm',
                velocity_from_epsilon=False, n_timesteps=0)
    ref = tr.init_params(ocfg, seed=5, dtype=torch.float64)
    vdm = M.make_vdm('mulan_velocity', cfg)
    params = M.tree_map(lambda x: x.cuda(), vdm.init(PRNGKey(0)))
    M.from_flax_layout(M.tree_map(lambda x: x.detach().float(), ref), params)
    experiment = types.SimpleNamespace(model=vdm, orig_params=params, device=torch.device("cuda"))
    return experiment, ref


def test_model_curves_and_summary(mulan, monkeypatch):
    from mulan_amd import evaluators as ev
    experiment, ref = mulan
    emb = torch.cat([ev.get_embedding(1, 50, shift=k) for k in (0, 7, 31)])
    t = sco.grid_times(7)
    want = sco.model_gamma64(ref, emb.numpy(), t)
    # the coefficient MLP runs in fp32 ahead of the kernel: its error is the parent's, measured here through poly_gamma
    with torch.no_grad():
        coeffs = experiment.model.sample_coefficients(experiment.orig_params, emb.cuda())
    a64, b64, c64 = (v.double().cpu().numpy() for v in coeffs)
    kernel_only = sco.gamma64(a64, b64, c64, t)
    got = ev.noise_schedule_per_embedding(experiment, emb, t)
    assert len(got) == 3 and all(g.shape == (7, sco.D) and g.dtype == np.float32 for g in got)
    for e in range(3):
        assert np.abs(got[e] - kernel_only[e]).max() <= GAMMA_BOUND
        rel = np.abs(got[e] - want[e]).max() / np.abs(want[e]).max()
        print(f"embedding {e}: against the float64 model {rel:.3e} (relative)")
        assert rel < 1e-5                                                  # the bar test_gpu_model holds the schedule to
    default = ev.noise_schedule_per_embedding(experiment, emb[:1])
    assert default[0].shape == (128, sco.D) and (default[0][0] == np.float32(GMIN)).all()
    monkeypatch.setattr(ev, "SCHEDULE_BUFFER_BYTES", 1)                    # one embedding per launch
    again = ev.noise_schedule_per_embedding(experiment, emb, t)
    assert all(np.array_equal(x, y) for x, y in zip(got, again))
    small = ev.noise_schedule_summary(experiment, emb, t, bins=64)
    monkeypatch.undo()
    summ = ev.noise_schedule_summary(experiment, emb, t, bins=64)
    assert all(np.array_equal(summ[k], small[k]) for k in summ)
    host = sco.stats_of(np.stack(got))                                     # statistics of the kernel's own curves
    keys = ("mean", "std", "min", "max", "sigma2_mean")
    for k, col in zip(keys, (0, 1, 2, 3, 7)):
        assert summ[k].shape == (3, 7) and np.abs(summ[k] - host[..., col]).max() <= STATS_BOUND[col], k
    assert summ["channel_mean"].shape == (3, 7, 3)
    assert np.abs(summ["channel_mean"] - host[..., 4:7]).max() <= STATS_BOUND[4]
    assert summ["hist"].shape == (3, 7, 64) and np.array_equal(summ["hist"], sco.binning32(np.stack(got), 64))
    assert np.array_equal(summ["time_steps"], t)
    assert summ["between"].shape == (7,) and np.allclose(summ["between"], summ["mean"].astype(np.float64).std(axis=0))
    assert summ["between"][t == 0].max() == 0


def test_plain_vdm_experiment_is_refused():
    from mulan_amd import evaluators as ev
    from mulan_amd import model as M
    plain = types.SimpleNamespace(model=object.__new__(M.PlainVDM), orig_params={}, device=torch.device("cuda"))
    for fn in (ev.noise_schedule_per_embedding, ev.noise_schedule_summary):
        with pytest.raises(ValueError, match="MuLAN"):
            fn(plain, ev.get_embedding(2))
