"""The memory-bound kernels at the sizes where their launch geometry changes: every kernel behind a block cap is run
above one pass of its capped grid (the grid-stride loop is entered a second time, the last pass is partial), the
float4 bodies with their scalar tails, and the counter-based noise streams against the oracle's Philox words.

References are float64 numpy / torch (the oracle's own function where it has one).  A bar is either the bar of the
kernel's existing small-shape test, unchanged, or derived inside the test from something independent of the kernel
(fp32 evaluation of the same formula on the host, two float64 summation orders of the same data, the precision of the
number format); each such test prints the figure it measured and its docstring records it.

GEOMETRY_CASES names, for every exported entry point whose launch is capped, the test here that crosses its cap;
tests/test_launch_geometry_table.py (CPU) holds the table against the sources."""
import math
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import mulan_np as onp
from oracle import torch_ref as tr
from tests import fast_sampler_oracle as fo
from tests import stream_oracle as so

# exported entry point -> the test below that runs it above one pass of its capped grid
GEOMETRY_CASES = {
    "mulan_adamw_ema_step": "test_adamw_multi_pass_decay_boundaries",
    "mulan_adamw_ema_step_scaled": "test_adamw_dyn_is_the_host_scalar_step",
    "mulan_adamw_ema_step_dyn": "test_adamw_dyn_is_the_host_scalar_step",
    "mulan_randn": "test_randn_matches_float64_box_muller",
    "mulan_noise": "test_uniform_and_rademacher_are_the_oracle_words",
    "mulan_act_fwd": "test_activations_above_one_pass",
    "mulan_act_bwd": "test_activations_above_one_pass",
    "mulan_fourier_fwd": "test_fourier_above_one_pass",
    "mulan_fourier_bwd": "test_fourier_above_one_pass",
    "mulan_temb_fwd": "test_cond_input_above_one_pass",
    "mulan_rowbcast": "test_row_broadcast_is_a_copy",
    "mulan_encode_u8": "test_encode_u8_exact",
    "mulan_axpby": "test_axpby_exact",
    "mulan_poly_gamma_fwd": "test_poly_gamma_above_one_pass",
    "mulan_poly_gamma_bwd": "test_poly_gamma_above_one_pass",
    "mulan_expm1_weight_fwd": "test_expm1_weight",
    "mulan_expm1_weight_bwd": "test_expm1_weight",
    "mulan_ode_drift": "test_ode_drift_above_one_pass",
    "mulan_rk_combine": "test_rk_combine",
    "mulan_dequantize": "test_dequantize_above_one_pass",
    "mulan_ancestral_step": "test_ancestral_step_above_one_pass",
    "mulan_fast_sampler_step": "test_fast_sampler_step_above_one_pass",
    "mulan_decode_argmax": "test_decode_argmax_and_sample_above_one_pass",
    "mulan_decode_sample": "test_decode_argmax_and_sample_above_one_pass",
    "mulan_decode_logprobs": "test_decode_logprobs_above_one_pass",
}

PASS = 4096 * 256                      # elements per pass of nblocks() / grid_for()
N_IMG = 400 * 3072                     # B = 400 images: above one pass
ADAM_PASS = 8192 * 256 * 4             # elements per pass of adamw_ema_kernel (one float4 per thread)
N_ADAM = 3 * ADAM_PASS + 4 * 1000 + 3  # several full passes, a partial last pass, a scalar tail of 3


@pytest.fixture(scope="module")
def ops():
    from mulan_amd import ops as _ops
    _ops.lib.load()
    return _ops


def dev(a, dtype=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(a)).to(dtype).cuda()


def host(t):
    return t.detach().cpu().double().numpy()


def rel_err(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.abs(a - b).max() / (np.abs(b).max() + 1e-30))


def t64(a):
    return torch.tensor(np.asarray(a), dtype=torch.float64)


# ====================================================================================================== 1. optimizer
HYPER = dict(b1=0.9, b2=0.99, eps=1e-8, ema_rate=0.9999)


@pytest.fixture(scope="module")
def adam_data():
    """fp32-valued inputs (so the float64 reference starts from the very numbers the kernel reads), on the host as
    float64 and on the device as pristine copies"""
    rng = np.random.default_rng(31)
    n = N_ADAM
    p = rng.standard_normal(n, dtype=np.float32)
    g = rng.standard_normal(n, dtype=np.float32)
    m = np.float32(0.1) * rng.standard_normal(n, dtype=np.float32)
    v = np.abs(rng.standard_normal(n, dtype=np.float32)) * np.float32(0.01) + np.float32(1e-4)
    ema = p + np.float32(0.01) * rng.standard_normal(n, dtype=np.float32)
    h = [a.astype(np.float64) for a in (p, g, m, v, ema)]
    d = [torch.from_numpy(a).cuda() for a in (p, g, m, v, ema)]
    return types.SimpleNamespace(n=n, host=h, dev=d)


def _adam_reference(data, n_decay, lr, wd, step, gscale=1.0):
    p, g, m, v, ema = data.host
    mask = (np.arange(data.n) < n_decay).astype(np.float64)
    # the hyperparameters reach the kernel as C floats: the reference gets those values (1 - fp32(0.99) is 9.5e-7 off 0.01
    # in relative terms, which alone would use up the 1e-6 bar on v)
    f32 = lambda x: float(np.float32(x))
    return onp.adamw_ema_step(p, gscale * g, m, v, ema, f32(lr), step, mask, b1=f32(HYPER["b1"]), b2=f32(HYPER["b2"]),
                              eps=f32(HYPER["eps"]), wd=f32(wd), ema_rate=f32(HYPER["ema_rate"]))    # (p, m, v, ema)


def _adam_run(ops, data, n_decay, lr, wd, step, **kw):
    p, g, m, v, ema = (t.clone() for t in data.dev)
    out = ops.adamw_ema_step(p, g, m, v, ema, n_decay, lr, HYPER["b1"], HYPER["b2"], HYPER["eps"], wd, step,
                             HYPER["ema_rate"], **kw)
    assert torch.equal(g, data.dev[1])                                               # the gradient is read only
    return (p, m, v, ema), out


# n_decay % 4 in {1, 2, 3} inside the second pass, in the partial last pass, on the float4 / tail boundary, inside the
# scalar tail, and the two ends
DECAY_BOUNDARIES = [ADAM_PASS + 4 * 777 + 1, ADAM_PASS + 4 * 777 + 2, ADAM_PASS + 4 * 777 + 3,
                    3 * ADAM_PASS + 4 * 500 + 2, N_ADAM - 3, N_ADAM - 2, 0, N_ADAM]


@pytest.mark.parametrize("n_decay", DECAY_BOUNDARIES)
def test_adamw_multi_pass_decay_boundaries(ops, adam_data, n_decay):
    """n = 3 x 8 388 608 + 4 x 1000 + 3 against onp.adamw_ema_step in float64 at the bar of
    test_adamw_ema_matches_oracle (max-norm relative 1e-6), with the suite's lr = 2e-4, wd = 0.01"""
    ref = _adam_reference(adam_data, n_decay, 2e-4, 0.01, 7, gscale=0.5)
    got, _ = _adam_run(ops, adam_data, n_decay, 2e-4, 0.01, 7, grad_scale=0.5)
    errs = [rel_err(a.cpu().numpy(), r) for a, r in zip(got, ref)]
    print("adamw n_decay", n_decay, "rel err p m v ema", errs)
    assert max(errs) < 1e-6


@pytest.mark.parametrize("n_decay", DECAY_BOUNDARIES)
def test_adamw_decay_mask_is_exact_at_the_boundary(ops, adam_data, n_decay):
    """lr = 0.1, wd = 0.5 and |p| >= 0.5 in the 16 elements either side of n_decay: an element on the wrong side of the
    mask moves by lr wd |p| >= 2.5e-2, so each of the 32 is held to float64 individually (1e-6 of the window's largest
    |p|; the window's p are O(1))"""
    n = adam_data.n
    lo, hi = max(0, n_decay - 16), min(n, n_decay + 16)
    data = types.SimpleNamespace(n=n, host=[adam_data.host[0].copy()] + adam_data.host[1:],
                                 dev=[adam_data.dev[0].clone()] + adam_data.dev[1:])
    w = data.host[0][lo:hi]
    w = np.where(np.abs(w) < 0.5, np.copysign(0.5 + np.abs(w), w), w).astype(np.float32)
    data.host[0][lo:hi] = w
    data.dev[0][lo:hi] = torch.from_numpy(w).cuda()
    ref = _adam_reference(data, n_decay, 0.1, 0.5, 3)
    got, _ = _adam_run(ops, data, n_decay, 0.1, 0.5, 3)
    assert np.abs(data.host[0][lo:hi]).min() >= 0.5
    for name, a, r in zip(("p", "m", "v", "ema"), got, ref):
        aw, rw = a[lo:hi].cpu().double().numpy(), r[lo:hi]
        bar = 1e-6 * np.abs(rw).max()
        worst = float(np.abs(aw - rw).max())
        print("adamw window", name, "n_decay", n_decay, "worst", worst, "bar", bar)
        for i in range(hi - lo):
            assert abs(aw[i] - rw[i]) <= bar, (name, lo + i, n_decay, aw[i], rw[i])
    # what a mask that is off by one element would miss by
    assert 0.1 * 0.5 * np.abs(data.host[0][lo:hi]).min() > 1e-2
    assert max(rel_err(a.cpu().numpy(), r) for a, r in zip(got, ref)) < 1e-6


def test_adamw_variants_and_block_caps(ops, adam_data):
    """tune[25] in {0, 1, 2, 3} (plain / non-temporal accesses, one or two float4 in flight) x tune[26] in {0, 7} (block
    cap 8192 / 7): each against float64 at 1e-6, and bit-identical to the default instantiation -- they share one
    arithmetic body.  Regression: with the body written as a b + c d and left to the compiler, the two-float4
    instantiations contracted m and v as fma(c, d, a b) where the default has fma(a, b, c d), and p, m, v differed in the
    last bit (each still 6e-8 .. 8e-8 from float64); adamw_ema_update now spells the roundings out."""
    n_decay = ADAM_PASS + 4 * 777 + 3
    ref = _adam_reference(adam_data, n_decay, 0.1, 0.5, 3)
    results = {}
    try:
        for var in (0, 1, 2, 3):
            for cap in (0, 7):
                ops.call("mulan_set_tuning", 25, var)
                ops.call("mulan_set_tuning", 26, cap)
                got, _ = _adam_run(ops, adam_data, n_decay, 0.1, 0.5, 3)
                torch.cuda.synchronize()
                results[(var, cap)] = got
    finally:
        ops.call("mulan_set_tuning", 25, 0)
        ops.call("mulan_set_tuning", 26, 0)
    for key, got in results.items():
        errs = [rel_err(a.cpu().numpy(), r) for a, r in zip(got, ref)]
        print("adamw variant", key, errs)
        assert max(errs) < 1e-6, key
    for key, got in results.items():
        for name, a, d in zip(("p", "m", "v", "ema"), got, results[(0, 0)]):
            assert torch.equal(a, d), (key, name, float((a - d).abs().max()))


@pytest.mark.parametrize("clip", [None, 0.3, 1e9])
def test_adamw_dyn_is_the_host_scalar_step(ops, adam_data, clip):
    """mulan_adamw_ema_step_dyn reading [lr, 1 - b1^t, 1 - b2^t] from the device (TrainState.dynamic_scalars) against
    mulan_adamw_ema_step / _scaled deriving them on the host from (lr, step): the same bits, with and without the
    global-norm clip in front; the host-scalar result against float64 at 1e-6 (2e-6 with the clip, the bar of
    test_adamw_with_global_norm_clipping)"""
    from mulan_amd.train_state import TrainState
    lr, step, n_decay = 2e-4, 11, 2 * ADAM_PASS + 4 * 123 + 1
    vals = TrainState.dynamic_scalars(types.SimpleNamespace(opt=dict(b1=HYPER["b1"], b2=HYPER["b2"])), lr, step)
    dyn = torch.tensor(vals, dtype=torch.float32).cuda()
    kw = dict(grad_scale=0.5) if clip is None else dict(grad_scale=0.5, clip_norm=clip)
    a, out_a = _adam_run(ops, adam_data, n_decay, lr, 0.01, step, **kw)
    b, out_b = _adam_run(ops, adam_data, n_decay, 0.0, 0.01, 0, dyn=dyn, **kw)
    for name, x, y in zip(("p", "m", "v", "ema"), a, b):
        assert torch.equal(x, y), (name, float((x - y).abs().max()))
    factor = 1.0
    if clip is not None:
        assert torch.equal(out_a, out_b)
        norm = math.sqrt(float(((0.5 * adam_data.host[1]) ** 2).sum()))
        factor = min(1.0, clip / norm)
        got_factor, got_norm = out_a.cpu().numpy()
        assert abs(got_norm - norm) < 1e-5 * norm and abs(got_factor - factor) < 1e-5
        assert (factor < 1.0) == (clip < 1.0)
    ref = _adam_reference(adam_data, n_decay, lr, 0.01, step, gscale=0.5 * factor)
    errs = [rel_err(x.cpu().numpy(), r) for x, r in zip(a, ref)]
    print("adamw dyn clip", clip, errs)
    assert max(errs) < (1e-6 if clip is None else 2e-6)


@pytest.mark.parametrize("n", [5 * 262144 + 131, 1])
@pytest.mark.parametrize("active", [True, False])
def test_global_norm_clip(ops, n, active):
    """sumsq_kernel (1024 blocks x 256 threads = 262 144 elements per pass) over five passes and a partial one, and on
    a single element; a gradient spanning 8 decades (a few elements at 1e3 among 1e-5); norm and factor against float64
    at the 1e-5 bar of test_adamw_with_global_norm_clipping, clip active and inactive"""
    rng = np.random.default_rng(n % 1000)
    g = (np.float32(1e-5) * rng.standard_normal(n, dtype=np.float32)).astype(np.float32)
    big = [k * 262144 + 1000 * k + 5 for k in range(5)] if n > 1 else [0]      # one in each full pass
    g[big] = np.float32(1e3) * np.sign(rng.standard_normal(len(big))).astype(np.float32)
    if n > 1:
        g[-1] = np.float32(-1e3)                                      # the last element of the partial pass counts
    pre = 0.5
    norm = pre * math.sqrt(float((g.astype(np.float64) ** 2).sum()))
    clip = 0.25 * norm if active else 4.0 * norm
    factor = min(1.0, clip / norm)
    ws = torch.empty(ops.lib.load().mulan_global_norm_clip_workspace() // 8, device="cuda", dtype=torch.float64)
    out = torch.empty(2, device="cuda", dtype=torch.float32)
    ops.call("mulan_global_norm_clip", ops.ptr(dev(g)), n, float(clip), pre, ops.ptr(ws), ops.ptr(out), ops.stream())
    got_factor, got_norm = out.cpu().numpy()
    print("global norm n", n, "norm", got_norm, norm, "factor", got_factor, factor)
    assert abs(got_norm - norm) < 1e-5 * norm and abs(got_factor - factor) < 1e-5
    assert (got_factor < 1.0) == active


# ====================================================================================================== 2. streams
SEED = 0x1234ABCD5678
OFFSET = (5 << 34) + 3                      # above 32 bits: the counter's high word is in use
STREAM_SIZES = [9_000_001, 1, 2, 3, 5, 1023]
KINDS = ("uniform", "rademacher", "truncated_normal", "gumbel")


@pytest.mark.parametrize("n", STREAM_SIZES)
def test_uniform_and_rademacher_are_the_oracle_words(ops, n):
    """element 4q + e is word e of Philox(seed, offset + q): U[0,1) = (w >> 8) 2^-24 and the sign = the top bit, equal
    bit for bit to the values derived from onp.philox4x32_10; n = 9 000 001 is above the cap (4096 blocks x 256 threads x
    4 elements = 4 194 304) with a tail of 1"""
    w = so.words(SEED, OFFSET, n)
    u = ops.noise((n,), SEED, OFFSET, "cuda", "uniform").cpu().numpy()
    assert np.array_equal(u, so.uniform24(w))
    r = ops.noise((n,), SEED, OFFSET, "cuda", "rademacher").cpu().numpy()
    assert np.array_equal(r, so.rademacher(w))


def _draw(ops, kind, n, seed, offset):
    if kind == "randn":
        return ops.randn((n,), seed, offset, "cuda")
    return ops.noise((n,), seed, offset, "cuda", kind)


@pytest.mark.parametrize("kind", ("randn",) + KINDS)
def test_offset_law(ops, kind):
    """f(n, seed, o)[4k:] is f(n - 4k, seed, o + k) bit for bit (every consumer derives disjoint streams from `offset`),
    across the grid cap and for ragged n; another seed gives other words"""
    for n, k in ((9_000_001, 1_100_000), (9_000_001, 1), (1023, 255), (7, 1), (4_194_304 + 6, 1_048_576)):
        whole = _draw(ops, kind, n, SEED, OFFSET)
        part = _draw(ops, kind, n - 4 * k, SEED, OFFSET + k)
        assert torch.equal(whole[4 * k:], part), (kind, n, k)
    a, b = _draw(ops, kind, 4096, SEED, OFFSET), _draw(ops, kind, 4096, SEED + 1, OFFSET)
    assert float((a == b).float().mean()) < (0.6 if kind == "rademacher" else 0.01)
    assert not torch.equal(_draw(ops, kind, 4096, SEED, OFFSET + 1)[:4092], a[:4092])


@pytest.mark.parametrize("kind", ("randn",) + KINDS)
@pytest.mark.parametrize("n", [1, 2, 3, 1021, 4_194_304 + 1, 4_194_304 + 2, 4_194_304 + 3])
def test_no_write_past_the_end(ops, kind, n):
    """n % 4 in {1, 2, 3}: the last counter's unused words are not stored"""
    buf = torch.full((n + 8,), -777.0, device="cuda")
    if kind == "randn":
        ops.randn((n,), SEED, OFFSET, "cuda", out=buf[:n])
    else:
        code = {"uniform": 0, "rademacher": 1, "truncated_normal": 2, "gumbel": 3}[kind]
        ops.call("mulan_noise", ops.ptr(buf), n, SEED, OFFSET, code, -3.0, 3.0, ops.stream())
    assert torch.equal(buf[n:], torch.full((8,), -777.0, device="cuda"))
    assert not bool((buf[:n] == -777.0).any())


N_FORMULA = 9_000_001


def test_randn_matches_float64_box_muller(ops):
    """mulan_randn against float64 Box-Muller on the kernel's own fp32 uniforms ((float)w + 0.5f) 2^-32, all
    9 000 001 elements.  Bar: 4 x the largest deviation of the same formula evaluated in np.float32 on the host from its
    float64 evaluation over the same counters (the margin covers device against host logf / sincosf).
    Measured on the host over these counters: fp32 deviation 1.10e-6 -> bar 4.40e-6."""
    n = N_FORMULA
    ref = so.randn(SEED, OFFSET, n, np.float64)
    dev32 = float(np.abs(so.randn(SEED, OFFSET, n, np.float32).astype(np.float64) - ref).max())
    bar = 4.0 * dev32
    got = ops.randn((n,), SEED, OFFSET, "cuda").cpu().double().numpy()
    err = float(np.abs(got - ref).max())
    print(f"randn: host fp32 deviation {dev32:.3e}, bar {bar:.3e}, device error {err:.3e}")
    assert np.isfinite(got).all() and err <= bar
    for m in (1, 2, 3, 5, 1023):
        small = ops.randn((m,), SEED, OFFSET, "cuda").cpu().double().numpy()
        assert np.abs(small - ref[:m]).max() <= bar


def test_gumbel_matches_float64(ops):
    """mulan_noise kind 3 against float64 -log(-log(u')) on the kernel's own fp32 uniform u' = min(fp32(u + 2^-25),
    1 - 2^-24), all 9 000 001 elements (seed 5: element 8 036 761 draws the largest u).  Bar: 4 x the host's fp32
    deviation from float64 on the same counters.  Measured on the host: 5.94e-7 -> bar 2.38e-6."""
    n, seed = N_FORMULA, 5
    w = so.words(seed, 0, n)
    assert int((w[8_036_761] >> np.uint32(8))) == 0xFFFFFF
    ref = so.gumbel_from_words(w, np.float64)
    dev32 = float(np.abs(so.gumbel_from_words(w, np.float32).astype(np.float64) - ref).max())
    bar = 4.0 * dev32
    got = ops.noise((n,), seed, 0, "cuda", "gumbel").cpu().double().numpy()
    err = float(np.abs(got - ref).max())
    print(f"gumbel: host fp32 deviation {dev32:.3e}, bar {bar:.3e}, device error {err:.3e}")
    assert np.isfinite(got).all() and err <= bar


def test_gumbel_of_the_largest_uniform_is_finite(ops):
    """regression: for w >> 8 = 0xFFFFFF the sum u + 2^-25 is a tie that rounds to 1.0f, and -log(-log(1)) = +inf went
    into the Gumbel-softmax latent once per 2^24 draws.  Word 2 of Philox(seed 8, counter 932 279) is such a word."""
    seed, counter = 8, 932_279
    w = so.words(seed, counter, 4)
    assert int(w[2] >> np.uint32(8)) == 0xFFFFFF
    got = ops.noise((4,), seed, counter, "cuda", "gumbel").cpu().double().numpy()
    ref = so.gumbel_from_words(w, np.float64)
    assert np.isfinite(got).all() and np.abs(got - ref).max() < 1e-5
    assert abs(got[2] - 24 * math.log(2.0)) < 1e-5                     # -log(-log(1 - 2^-24)) = 24 ln 2 (+ 3e-8)


@pytest.mark.parametrize("lo,hi", [(-3.0, 3.0), (-1.0, 2.5)])
def test_truncated_normal_matches_float64(ops, lo, hi):
    """mulan_noise kind 2 against the float64 inverse CDF on the kernel's own fp32 uniform, all 9 000 001 variates, none
    excluded; the error is that of the variate.  Bar: 4 x the host's fp32 deviation from float64 on the same counters
    (near the upper end 2 p - 1 is rounded to fp32 where erfinv has slope 80: this is where the fp32 formula loses most).
    Measured on the host, [-3, 3]: 2.60e-5 (at x = 2.993) -> bar 1.04e-4; [-1, 2.5]: 4.79e-6 -> bar 1.92e-5."""
    n = N_FORMULA
    w = so.words(SEED, OFFSET, n)
    ref = so.truncated_normal_from_words(w, lo, hi, np.float64)
    dev32 = float(np.abs(so.truncated_normal_from_words(w, lo, hi, np.float32).astype(np.float64) - ref).max())
    bar = 4.0 * dev32
    got = ops.noise((n,), SEED, OFFSET, "cuda", "truncated_normal", lo, hi).cpu().double().numpy()
    err = float(np.abs(got - ref).max())
    print(f"truncated normal [{lo}, {hi}]: host fp32 deviation {dev32:.3e}, bar {bar:.3e}, device error {err:.3e}")
    assert got.min() >= lo and got.max() <= hi and err <= bar


# ====================================================================================================== 3. capped grids
def test_activations_above_one_pass(ops):
    """act_fwd / act_bwd at 4 passes + 77 elements, bars of test_activations_colsum_softmax (1e-6)"""
    rng = np.random.default_rng(41)
    n = 4 * PASS + 77
    x32, dy32 = (rng.standard_normal(n, dtype=np.float32) * 3).astype(np.float32), rng.standard_normal(n, dtype=np.float32)
    for fn_ref, fn in ((tr.swish, ops.silu), (lambda v: 1e-3 + torch.nn.functional.softplus(v),
                                              lambda v: ops.softplus_shift(v, 1e-3))):
        x = t64(x32).requires_grad_()
        y = fn_ref(x)
        y.backward(t64(dy32))
        g = dev(x32).requires_grad_()
        o = fn(g)
        o.backward(dev(dy32))
        assert rel_err(host(o), y.detach().numpy()) < 1e-6
        assert rel_err(host(g.grad), x.grad.numpy()) < 1e-6


def test_fourier_above_one_pass(ops):
    """fourier_fwd / fourier_bwd at npix = one pass + 333 (raw launches: the pixel count need not be whole images), bars
    of test_fourier_and_timestep_embedding; the accumulate form of the backward on top of an integer-valued dz"""
    rng = np.random.default_rng(42)
    npix = PASS + 333
    z = (rng.standard_normal((npix, 3)) * 1.5).astype(np.float32)
    dout = rng.standard_normal((npix, 16)).astype(np.float32)
    zt = t64(z).requires_grad_()
    ref = torch.cat([zt, tr.fourier_features(zt)], dim=-1)
    ref.backward(t64(dout[:, :15]))
    zd, dd = dev(z), dev(dout)
    out = torch.full((npix + 1, 16), -777.0, device="cuda")
    ops.call("mulan_fourier_fwd", ops.ptr(zd), ops.ptr(out), npix, ops.stream())
    o = out[:npix].cpu().numpy()
    assert np.all(o[:, 15] == 0) and bool((out[npix] == -777.0).all())
    f32 = np.concatenate([z, onp.fourier_features(z, np.float32)], axis=-1)
    assert np.abs(o[:, :15] - f32).max() < 2e-6
    assert np.abs(o[:, :15] - ref.detach().numpy()).max() < 5e-4
    dz = torch.full((npix + 1, 3), -777.0, device="cuda")
    ops.call("mulan_fourier_bwd", ops.ptr(zd), ops.ptr(dd), ops.ptr(dz), npix, 0, ops.stream())
    assert rel_err(host(dz[:npix]), zt.grad.numpy()) < 1e-3 and bool((dz[npix] == -777.0).all())
    base = rng.integers(-3, 4, (npix, 3)).astype(np.float32) * 4096.0
    acc = dev(base)
    ops.call("mulan_fourier_bwd", ops.ptr(zd), ops.ptr(dd), ops.ptr(acc), npix, 1, ops.stream())
    assert rel_err(host(acc) - base, zt.grad.numpy()) < 1e-3


def test_cond_input_above_one_pass(ops):
    """temb_fwd at 17 017 rows x 64 frequencies = 1 089 088 (above one pass, not a multiple of 256) writing into rows of
    width E + K, and rowbcast behind it (rep = 1001, 1 191 190 elements): the bars of
    test_fourier_and_timestep_embedding; the conditioning columns are a copy"""
    rng = np.random.default_rng(43)
    rep, nb, K, E = 1001, 17, 70, 128
    n = nb * rep
    t = rng.uniform(0, 1, size=n).astype(np.float32)
    cond = rng.standard_normal((nb, K)).astype(np.float32)
    with torch.no_grad():
        out = ops.cond_input(dev(t), dev(cond), E, rep).cpu().numpy()
    assert out.shape == (n, E + K)
    e32 = onp.timestep_embedding(t, E, np.float32)
    e64 = tr.timestep_embedding(t64(t), E).numpy()
    assert np.abs(out[:, :E] - e32).max() < 2e-4
    assert np.abs(out[:, :E] - e64).max() < 5e-4
    assert np.array_equal(out[:, E:], np.repeat(cond, rep, axis=0))


def test_row_broadcast_is_a_copy(ops):
    """rowbcast at 22 x 1000 rows x 51 columns = 1 122 000 elements: y[r] = x[r // rep], exactly"""
    rng = np.random.default_rng(44)
    nb, rep, K = 22, 1000, 51
    x = rng.standard_normal((nb, K)).astype(np.float32)
    with torch.no_grad():
        y = ops.row_broadcast(dev(x), rep).cpu().numpy()
    assert y.shape == (nb * rep, K) and np.array_equal(y, np.repeat(x, rep, axis=0))
    # into a wider matrix at a column offset (the form cond_input uses), the other columns untouched
    rows, ld, col0 = nb * rep + 3, K + 5, 2
    src = rng.standard_normal(((rows + rep - 1) // rep, K)).astype(np.float32)
    wide = torch.full((rows + 1, ld), -777.0, device="cuda")
    ops.call("mulan_rowbcast", ops.ptr(dev(src)), ops.ptr(wide), rows, K, rep, ld, col0, ops.stream())
    want = np.full((rows + 1, ld), -777.0, dtype=np.float32)
    want[:rows, col0:col0 + K] = np.repeat(src, rep, axis=0)[:rows]
    assert np.array_equal(wide.cpu().numpy(), want)


def test_encode_u8_exact(ops):
    """encode_u8 at 400 x 3072 + 5 elements against the same expression in np.float32 (every step of it is exact in
    fp32: 9 significant bits) and against the oracle's float64 encode"""
    rng = np.random.default_rng(45)
    n = N_IMG + 5
    x = rng.integers(0, 256, n).astype(np.uint8)
    x[:256] = np.arange(256)
    f = ops.encode_u8(torch.from_numpy(x).cuda()).cpu().numpy()
    want = np.float32(2.0) * ((x.astype(np.float32) + np.float32(0.5)) / np.float32(256.0)) - np.float32(1.0)
    assert f.dtype == np.float32 and np.array_equal(f, want)
    assert np.array_equal(f.astype(np.float64), onp.encode(x))


@pytest.mark.parametrize("a,b", [(0.5, -2.0), (1.0, 0.0), (4.0, 0.25)])
def test_axpby_exact(ops, a, b):
    """y <- a x + b y at 400 x 3072 + 5 elements with a, b powers of two: both products are exact, so the result is
    the one correctly rounded sum whether or not the compiler contracts it into an fma -- equal to float64 rounded
    once"""
    rng = np.random.default_rng(46)
    n = N_IMG + 5
    x, y = rng.standard_normal(n, dtype=np.float32), rng.standard_normal(n, dtype=np.float32)
    buf = torch.full((n + 4,), -777.0, device="cuda")
    buf[:n] = dev(y)
    ops.call("mulan_axpby", ops.ptr(dev(x)), ops.ptr(buf), n, a, b, ops.stream())
    want = (a * x.astype(np.float64) + b * y.astype(np.float64)).astype(np.float32)
    assert np.array_equal(buf[:n].cpu().numpy(), want) and bool((buf[n:] == -777.0).all())


def test_poly_gamma_above_one_pass(ops):
    """poly_gamma_fwd / bwd at B = 400 (400 x 3072 elements), bars of test_poly_gamma"""
    rng = np.random.default_rng(47)
    B = 400
    a = (rng.standard_normal((B, 3072)) * 0.5).astype(np.float32)
    b = (rng.standard_normal((B, 3072)) * 0.5).astype(np.float32)
    c = (1e-3 + np.logaddexp(rng.standard_normal((B, 3072)), 0)).astype(np.float32)
    t = rng.uniform(0, 1, B).astype(np.float32)
    ta, tb, tc = (t64(v).requires_grad_() for v in (a, b, c))
    gt, gp = tr.poly_gamma(ta, tb, tc, t64(t)), tr.poly_gamma_grad_t(ta, tb, tc, t64(t))
    d1, d2 = rng.standard_normal((B, 3072)).astype(np.float32), rng.standard_normal((B, 3072)).astype(np.float32)
    ((gt * t64(d1)).sum() + (gp * t64(d2)).sum()).backward()
    ga, gb, gc = (dev(v).requires_grad_() for v in (a, b, c))
    g0, g1, ogt, ogp = ops.poly_gamma(ga, gb, gc, dev(t), -13.3, 5.0)
    ((ogt * dev(d1)).sum() + (ogp * dev(d2)).sum()).backward()
    assert np.abs(host(g0) + 13.3).max() < 1e-5 and np.abs(host(g1) - 5.0).max() < 1e-5
    assert rel_err(host(ogt), gt.detach().numpy()) < 5e-5
    assert rel_err(host(ogp), gp.detach().numpy()) < 5e-5
    for g, r in ((ga, ta), (gb, tb), (gc, tc)):
        assert rel_err(host(g.grad), r.grad.numpy()) < 1e-4


@pytest.mark.parametrize("n", [N_IMG + 5, 255])
def test_expm1_weight(ops, n):
    """w = T expm1(gamma_t - gamma_s), the discrete-time loss weight (ldm/model_mulan_epsilon.py:348-355), forward and
    both gradients against float64 autograd.  Bar: 4 x the max-norm relative deviation of torch.float32 evaluation of
    the same expression on the host from float64 (the fp32 difference gamma_t - gamma_s is the larger part of it).
    Measured on the host, n = 1 228 805: forward 1.25e-7 -> bar 4.99e-7, gradients 1.03e-7 -> bar 4.13e-7; n = 255:
    8.83e-8 -> 3.53e-7 and 5.94e-8 -> 2.38e-7."""
    rng = np.random.default_rng(48)
    T = 1000.0
    gt = rng.uniform(-13.3, 5.0, n).astype(np.float32)
    gs = (gt - rng.uniform(1e-4, 0.5, n)).astype(np.float32)
    dw = rng.standard_normal(n).astype(np.float32)

    def run(dtype, device):
        a = torch.tensor(gt, dtype=dtype, device=device).requires_grad_()
        b = torch.tensor(gs, dtype=dtype, device=device).requires_grad_()
        w = ops.expm1_weight(a, b, T) if device == "cuda" else T * torch.expm1(a - b)
        w.backward(torch.tensor(dw, dtype=dtype, device=device))
        return [host(v) for v in (w, a.grad, b.grad)]

    ref, emu, got = run(torch.float64, "cpu"), run(torch.float32, "cpu"), run(torch.float32, "cuda")
    for name, r, e, g in zip(("w", "dgt", "dgs"), ref, emu, got):
        dev32 = rel_err(e, r)
        err = rel_err(g, r)
        print(f"expm1_weight n {n} {name}: host fp32 deviation {dev32:.3e}, bar {4 * dev32:.3e}, device error {err:.3e}")
        assert err <= 4.0 * dev32, name
    assert np.array_equal(got[1], -got[2])


@pytest.mark.parametrize("mode,kind", [(0, "velocity"), (1, "vfe"), (2, "epsilon")])
@pytest.mark.parametrize("per_sample", [False, True])
def test_ode_drift_above_one_pass(ops, mode, kind, per_sample):
    """ode_drift at 400 x 3072 (+ 5 with a gamma per element): drift at the 5e-6 of test_ode_drift_and_div_kernels, the
    cotangent at the 2e-6 of test_ode_drift_and_divergence_high_precision"""
    rng = np.random.default_rng(49 + mode)
    B, D = 400, 3072
    n = B * D if per_sample else B * D + 5
    shape = (B, D) if per_sample else (n,)
    x, net = rng.standard_normal(shape).astype(np.float32), rng.standard_normal(shape).astype(np.float32)
    h = (rng.integers(0, 2, shape) * 2.0 - 1.0).astype(np.float32)
    gshape = (B,) if per_sample else shape
    gt = rng.uniform(-13.3, 5.0, gshape).astype(np.float32)
    gp = rng.uniform(1.0, 40.0, gshape).astype(np.float32)
    drift, cot = ops.ode_drift(dev(net), dev(x), dev(gt), dev(gp), dev(h), mode)
    bc = (lambda g: t64(g)[:, None]) if per_sample else t64
    n64 = t64(net).requires_grad_()
    f = tr.ode_drift(n64, t64(x), bc(gt), bc(gp), kind)
    (dn,) = torch.autograd.grad(f.sum(), n64)
    assert rel_err(host(drift), f.detach().numpy()) < 5e-6
    assert rel_err(host(cot), (dn * t64(h)).numpy()) < 2e-6


# Dormand-Prince 5(4): the rows of scipy.integrate._ivp.rk.RK45 (A, B, E)
RK_ROWS = [[1 / 5], [3 / 40, 9 / 40], [44 / 45, -56 / 15, 32 / 9], [19372 / 6561, -25360 / 2187, 64448 / 6561, -212 / 729],
           [9017 / 3168, -355 / 33, 46732 / 5247, 49 / 176, -5103 / 18656],
           [35 / 384, 0, 500 / 1113, 125 / 192, -2187 / 6784, 11 / 84],
           [-71 / 57600, 0, 71 / 16695, -71 / 1920, 17253 / 339200, -22 / 525, 1 / 40]]


def _seq_sum(terms):
    acc = terms[0]
    for t in terms[1:]:
        acc = acc + t
    return acc


def _pair_sum(terms):
    terms = list(terms)
    while len(terms) > 1:
        terms = [terms[i] + terms[i + 1] if i + 1 < len(terms) else terms[i] for i in range(0, len(terms), 2)]
    return terms[0]


@pytest.mark.parametrize("n", [N_IMG, 255])
def test_rk_combine(ops, n):
    """out = y + h sum_j c_j K_j for ncoef = 0 ... 7 (rows of the Dormand-Prince tableau), float64 and fp32 outputs,
    against numpy float64 of scipy's formula y + h (K^T c).  Bar (float64 output): 4 x the deviation between two float64
    summation orders of the same terms -- sequential y + h (c_0 K_0 + c_1 K_1 + ...) as scipy's dot, and a pairwise
    tree over y, (h c_0) K_0, (h c_1) K_1, ... -- a few 1e-16 of |y|; the fp32 output adds half an fp32 ulp.
    Measured: deviation 4.4e-16 (ncoef 1) and 8.9e-16 (ncoef 2 ... 7) at n = 1 228 800, half of that at n = 255 -> bars
    1.8e-15 / 3.6e-15 and 8.9e-16 / 1.8e-15; ncoef 0 has no arithmetic: deviation and bar 0, out = y exactly."""
    rng = np.random.default_rng(50)
    y = rng.standard_normal(n)
    K = rng.standard_normal((7, n)).astype(np.float32)
    h = 0.037
    yd, Kd = dev(y, torch.float64), dev(K)
    for coef in [[]] + RK_ROWS:
        k64 = [K[j].astype(np.float64) for j in range(len(coef))]
        seq = y + h * _seq_sum([c * k for c, k in zip(coef, k64)]) if coef else y.copy()
        pair = _pair_sum([y] + [(h * c) * k for c, k in zip(coef, k64)])
        order_dev = float(np.abs(seq - pair).max())
        bar = 4.0 * order_dev
        out = torch.full((n + 1,), -777.0, device="cuda", dtype=torch.float64)
        out32 = torch.full((n + 1,), -777.0, device="cuda")
        ops.rk_combine(yd, Kd, coef, h, out=out[:n], out32=out32[:n])
        err = float(np.abs(host(out[:n]) - seq).max())
        print(f"rk_combine n {n} ncoef {len(coef)}: order deviation {order_dev:.3e}, bar {bar:.3e}, device error {err:.3e}")
        assert err <= bar, len(coef)
        assert float(out[n]) == -777.0 and float(out32[n]) == -777.0
        e32 = np.abs(host(out32[:n]) - seq)
        assert np.all(e32 <= 2.0 ** -24 * np.abs(seq) + bar), len(coef)
        only32 = torch.empty(n, device="cuda")
        ops.rk_combine(yd, Kd, coef, h, out32=only32)
        assert torch.equal(only32, out32[:n])


def _sum_orders(v):
    """(pairwise, sequential) float64 sums of the same data; sequential: first to last or last to first, whichever lies
    further from the pairwise sum (at n = 255 one direction alone is within an ulp or two of it, by luck exactly on it)"""
    pw, fwd, bwd = float(np.sum(v)), float(np.cumsum(v)[-1]), float(np.cumsum(v[::-1])[-1])
    return pw, (fwd if abs(fwd - pw) >= abs(bwd - pw) else bwd)


@pytest.mark.parametrize("n", [N_IMG, 255])
def test_rk_error_norm(ops, n):
    """sum_i (h sum_j E_j K_j[i] / (atol + rtol max(|y_i|, |ynew_i|)))^2 (scipy RK45._estimate_error_norm, squared and
    unnormalised) over 256 blocks that stride 19 times at n = 400 x 3072.  Bar: 4 x |pairwise - sequential| float64 sum of
    the same squares.  Measured (rtol 1e-3, atol 1e-2: the terms vary):
    n = 1 228 800: relative 2.8e-14 (166 ulp) -> bar 1.1e-13; n = 255: 3.3e-16 (3 ulp) -> bar 1.3e-15 (12 ulp)."""
    rng = np.random.default_rng(51)
    y, ynew = rng.standard_normal(n), rng.standard_normal(n)
    K = rng.standard_normal((7, n)).astype(np.float32)
    E, h, rtol, atol = RK_ROWS[6], 0.037, 1e-3, 1e-2
    scale = atol + rtol * np.maximum(np.abs(y), np.abs(ynew))
    r = h * (K.astype(np.float64).T @ np.array(E)) / scale
    pw, sq = _sum_orders(r * r)
    bar = 4.0 * abs(pw - sq)
    ws, out = ops.rk_workspace("cuda"), torch.full((3,), -777.0, device="cuda", dtype=torch.float64)
    ops.rk_error_norm(dev(y, torch.float64), dev(ynew, torch.float64), dev(K), E, h, rtol, atol, ws, out)
    got = float(out[0])
    print(f"rk_error_norm n {n}: pairwise {pw!r} sequential {sq!r} bar {bar:.3e} ({bar / pw:.3e} rel), "
          f"device error {abs(got - pw):.3e}")
    assert abs(got - pw) <= bar
    assert float(out[1]) == -777.0


@pytest.mark.parametrize("n", [N_IMG, 255])
@pytest.mark.parametrize("with_f1", [True, False])
def test_rk_init_norms(ops, n, with_f1):
    """the three sums of scipy's select_initial_step, (y0 / s)^2, (f0 / s)^2, ((f1 - f0) / s)^2 with s = atol + rtol |y0|;
    without f1 the third is exactly 0.  Bar per sum: 4 x |pairwise - sequential| float64 sum of the same squares.
    Measured: n = 1 228 800: relative 2.9e-14, 4.1e-14, 1.8e-14 (142, 227, 103 ulp); n = 255: 2.6e-16, 6.5e-16, 8.5e-16
    (2, 3, 4 ulp); the bars are 4 x that."""
    rng = np.random.default_rng(52)
    y0 = rng.standard_normal(n)
    f0, f1 = rng.standard_normal(n).astype(np.float32), rng.standard_normal(n).astype(np.float32)
    rtol, atol = 1e-3, 1e-2
    s = atol + rtol * np.abs(y0)
    terms = [y0 / s, f0.astype(np.float64) / s, (f1.astype(np.float64) - f0.astype(np.float64)) / s]
    ws, out = ops.rk_workspace("cuda"), torch.full((4,), -777.0, device="cuda", dtype=torch.float64)
    ops.rk_init_norms(dev(y0, torch.float64), dev(f0), dev(f1) if with_f1 else None, rtol, atol, ws, out)
    got = out.cpu().numpy()
    for j, term in enumerate(terms):
        if j == 2 and not with_f1:
            assert got[2] == 0.0
            continue
        pw, sq = _sum_orders(term * term)
        bar = 4.0 * abs(pw - sq)
        print(f"rk_init_norms n {n} sum {j}: pairwise {pw!r} sequential {sq!r} bar {bar:.3e} ({bar / pw:.3e} rel), "
              f"device error {abs(got[j] - pw):.3e}")
        assert abs(got[j] - pw) <= bar, j
    assert got[3] == -777.0


def test_dequantize_above_one_pass(ops):
    """dequantize at 400 x 3072 + 5 elements, both noise forms, bars of test_noise_kinds_and_dequantisation"""
    rng = np.random.default_rng(53)
    n = N_IMG + 5
    x = rng.integers(0, 256, n).astype(np.uint8)
    x[:4] = [0, 0, 255, 255]
    u = rng.uniform(0, 1, n).astype(np.float32)
    tn = (np.clip(rng.standard_normal(n), -3, 3) * 40).astype(np.float32)
    for uniform, noise, s in ((True, u, 1.0), (False, tn, math.exp(-6.65))):
        data, rq = ops.dequantize(torch.from_numpy(x).cuda(), dev(noise), uniform, s)
        f = tr.encode(t64(x))
        nz = 2 * (t64(noise) - 0.5) / 256 if uniform else t64(noise) * s
        ref = f + nz
        assert rel_err(host(data), ref.numpy()) < 2e-7
        ref_q = torch.round(torch.clamp(128 * (ref + 1) - 0.5, 0, 255)).numpy()
        got = rq.cpu().numpy().astype(np.float64)
        edge = np.abs((128 * (ref.numpy() + 1) - 0.5) % 1 - 0.5) < 1e-3          # fp32 vs fp64 exactly at .5
        assert np.array_equal(got[~edge], ref_q[~edge]) and np.abs(got - ref_q).max() <= 1
        if uniform:
            assert (got == x).mean() > 0.999 and np.abs(got - x).max() <= 1


@pytest.mark.parametrize("mode,kind", [(0, "velocity"), (1, "epsilon"), (2, "input")])
@pytest.mark.parametrize("per_sample", [False, True])
def test_ancestral_step_above_one_pass(ops, mode, kind, per_sample):
    """ancestral_step at 400 x 3072 (+ 5 with a gamma per element), bars of test_ancestral_step_kernel"""
    rng = np.random.default_rng(54 + mode)
    B, D = 400, 3072
    shape = (B, D) if per_sample else (B * D + 5,)
    zt, net, eps = (rng.standard_normal(shape).astype(np.float32) for _ in range(3))
    gshape = (B,) if per_sample else shape
    gt = rng.uniform(-13.3, 5.0, gshape).astype(np.float32)
    gs = (gt - rng.uniform(1e-3, 0.5, gshape)).astype(np.float32)
    zs = ops.ancestral_step(dev(zt), dev(net), dev(gt), dev(gs), dev(eps), mode)
    bc = (lambda g: t64(g)[:, None]) if per_sample else t64
    ref = tr.ancestral_step(t64(zt), t64(net), bc(gt), bc(gs), t64(eps), kind).numpy()
    assert rel_err(host(zs), ref) < (2e-5 if mode == 2 else 2e-6)


FAST_KINDS = {0: "velocity", 1: "epsilon", 2: "input"}


@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("order", [1, 2])
@pytest.mark.parametrize("path", ["vec_per_sample", "vec_per_elem", "scalar"])
def test_fast_sampler_step_above_one_pass(ops, mode, order, path):
    """fast_sampler_step above its cap of 2048 blocks: the float4 path at B = 700 (2 150 400 elements; one pass is
    2 097 152) with a gamma per sample and per element, the scalar path at 400 x 3072 + 1 (one pass is 524 288); bars of
    test_fast_sampler_step_kernel"""
    rng = np.random.default_rng(60 + mode + 3 * order)
    B, D = 700, 3072
    shape = (B, D) if path != "scalar" else (N_IMG + 1,)
    gshape = (B,) if path == "vec_per_sample" else shape
    zt, net, xp = (rng.standard_normal(shape).astype(np.float32) for _ in range(3))
    gt = rng.uniform(-13.3, 5.0, gshape).astype(np.float32)
    gs = (gt - rng.uniform(1e-3, 0.5, gshape)).astype(np.float32)
    gp = (gt + rng.uniform(0.2, 1.0, gshape)).astype(np.float32)
    hist = (dev(gp), dev(xp)) if order == 2 else (None, None)
    zs, x0 = ops.fast_sampler_step(dev(zt), dev(net), dev(gt), dev(gs), mode, *hist)
    g = (lambda a: t64(a)[:, None]) if path == "vec_per_sample" else t64
    ref, xref, _ = fo.fast_step(t64(zt), t64(net), g(gt), g(gs), FAST_KINDS[mode],
                                *((g(gp), t64(xp)) if order == 2 else (None, None)))
    bar = 2e-5 if mode == 2 else 2e-6
    assert rel_err(host(zs), ref.numpy()) < bar
    assert rel_err(host(x0), xref.numpy()) < bar


@pytest.mark.parametrize("per_sample", [False, True])
def test_decode_argmax_and_sample_above_one_pass(ops, per_sample):
    """decode_argmax and decode_sample at 400 x 3072 (+ 5 with a gamma per element).  z_0 sits strictly inside bin x
    after the 1 / alpha_0 rescale (the construction of test_decode_argmax_kernel), so the argmax is x; with gamma_0 in
    [-17, -16] the bins are 20 standard deviations apart (neighbouring logits differ by more than 70, a Gumbel difference
    of probability e^-70), so the categorical draw is x as well -- every one of the 3e8 Gumbel draws has to be finite
    (about 19 of them come from the largest uniform, whose Gumbel was +inf)"""
    rng = np.random.default_rng(70)
    B, D = 400, 3072
    shape = (B, D) if per_sample else (B * D + 5,)
    x = rng.integers(0, 256, shape)
    g0 = rng.uniform(-17.0, -16.0, (B,) if per_sample else shape).astype(np.float32)
    g0b = g0[:, None] if per_sample else g0
    v = 2 * ((x + 0.5) / 256) - 1
    z0 = ((v + rng.uniform(-0.3, 0.3, shape) * (2 / 256)) * np.sqrt(1 - 1 / (1 + np.exp(-g0b.astype(np.float64)))))
    z0 = z0.astype(np.float32)
    out = ops.decode_argmax(dev(z0), dev(g0)).cpu().numpy()
    assert out.dtype == np.uint8 and np.array_equal(out, x)
    smp = ops.decode_sample(dev(z0), dev(g0), SEED, OFFSET).cpu().numpy()
    wrong = np.flatnonzero(smp.reshape(-1) != x.reshape(-1))
    assert wrong.size == 0, (wrong[:8], smp.reshape(-1)[wrong[:8]], x.reshape(-1)[wrong[:8]])


def test_decode_sample_of_the_largest_uniform(ops):
    """regression: element 0, bin 2 of decode_sample(seed 8, offset 932 279) draws w >> 8 = 0xFFFFFF, for which
    fp32(k + 0.5) 2^-24 rounds to 1.0f and the Gumbel was +inf: bin 2 won whatever the logits"""
    seed, counter = 8, 932_279
    assert int(so.words(seed, counter, 4)[2] >> np.uint32(8)) == 0xFFFFFF
    g0 = np.full(4, -16.5, dtype=np.float32)
    x = np.array([200, 2, 100, 31])
    z0 = ((2 * ((x + 0.5) / 256) - 1) * np.sqrt(1 - 1 / (1 + np.exp(16.5)))).astype(np.float32)
    smp = ops.decode_sample(dev(z0), dev(g0), seed, counter).cpu().numpy()
    assert np.array_equal(smp, x), smp


def test_decode_logprobs_above_one_pass(ops):
    """decode_logprobs at 262 144 + 77 elements (one wave per element, 65 536 blocks of 4: one pass is 262 144), every
    row against onp.decode_logprobs at the bar of the EncDec.decode test in tests/test_gpu_model.py"""
    rng = np.random.default_rng(71)
    n = 65536 * 4 + 77
    z = rng.uniform(-1.3, 1.3, n).astype(np.float32)
    g0 = rng.uniform(-13.5, -6.0, n).astype(np.float32)
    got = ops.decode_logprobs(dev(z), dev(g0))
    assert got.shape == (n, 256)
    for lo in range(0, n, 32768):
        hi = min(n, lo + 32768)
        want = onp.decode_logprobs(z[lo:hi].astype(np.float64), g0[lo:hi].astype(np.float64))
        g = host(got[lo:hi])
        bad = np.abs(g - want) - (1e-4 + 1e-5 * np.abs(want).max(axis=-1, keepdims=True))
        assert float(bad.max()) < 0, (lo, float(np.abs(g - want).max()))
        assert float(np.abs(np.exp(g).sum(-1) - 1).max()) < 1e-5


# ====================================================================================================== column sums
@pytest.mark.parametrize("C,vec", [(1, False), (3, False), (68, False), (260, False), (68, True), (260, True)])
@pytest.mark.parametrize("accumulate", [0, 1])
def test_colsum_paths(ops, C, accumulate, vec):
    """mulan_colsum on rows of a wider matrix (ld > C, the padding holds NaN): the float4 path (C and ld multiples of 4)
    and the scalar path (ld = C + 3), writing and accumulating, integer-valued data so the sums are exact.  seg = 1000
    leaves the float4 path's 128-row unrolled loop with a remainder."""
    rng = np.random.default_rng(80 + C)
    nseg, seg = 5, 1000
    ld = C + 4 if vec else C + 3
    x = np.full((nseg * seg, ld), np.nan, dtype=np.float32)
    x[:, :C] = rng.integers(-3, 4, (nseg * seg, C))
    base = rng.integers(-5, 6, (nseg, C)).astype(np.float32)
    out = torch.full((nseg * C + 4,), -777.0, device="cuda")
    out[:nseg * C] = dev(base).reshape(-1)
    xd = dev(x)
    assert xd.data_ptr() % 16 == 0 and out.data_ptr() % 16 == 0
    ops.call("mulan_colsum", xd.data_ptr(), ops.ptr(out), nseg, seg, C, ld, accumulate, ops.stream())
    want = x[:, :C].astype(np.float64).reshape(nseg, seg, C).sum(axis=1) + (base if accumulate else 0)
    assert np.array_equal(host(out[:nseg * C]).reshape(nseg, C), want)
    assert bool((out[nseg * C:] == -777.0).all())
