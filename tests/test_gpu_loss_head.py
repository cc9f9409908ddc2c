"""The loss-head kernels (mulan_amd/csrc/vdm_loss.hip with loss_terms.h) through their C entry points, on buffers the
test allocates, against tests/loss_head_oracle.py in float64 -- per output and per sample, on every case of the oracle's
table: the schedule's ends and beyond them, constant images, the scalar schedule, wide reconstruction noise, an
exact-target sample beside ordinary ones, every optional-pointer form and every refusal.

Bars are not written here.  Each is computed at run time: 4 x the error of the twin (the oracle's own functions in
float32 on the host) by the same measure on the same inputs, never below 2^-20; every comparison prints
`kernel error / twin error / bar` of its worst sample.  Every output buffer is NaN before the call.

Worst kernel error / bar per entry point and output over all cases, MI355X (the table the module prints when it ends):

  diffloss_bwd mode 0:dgprime          0.257  (mode0-128-scalar-expm1)
  diffloss_bwd mode 0:dgt              0.251  (mode0-random-elem-uniform)
  diffloss_bwd mode 0:dnet             0.256  (mode0-halves-elem-uniform)
  diffloss_bwd mode 1:dgprime          0.257  (mode1-random-elem-uniform)
  diffloss_bwd mode 1:dgt              0.333  (mode1-255-elem-expm1)
  diffloss_bwd mode 1:dnet             0.256  (mode1-255-elem-expm1)
  diffloss_bwd mode 1:dzt              0.262  (mode1-random-elem-uniform)
  diffloss_bwd mode 2:dgprime          0.179  (mode2-128-scalar-expm1)
  diffloss_bwd mode 2:dgt              0.000  (mode2-random-elem-uniform)
  diffloss_bwd mode 2:dnet             0.104  (mode2-128-scalar-expm1)
  diffloss_fwd mode 0:loss             0.256  (mode0-128-scalar-expm1)
  diffloss_fwd mode 1:loss             0.255  (mode1-random-elem-uniform)
  diffloss_fwd mode 2:loss             0.087  (mode2-zeros-scalar-uniform)
  ops.diffusion_loss:dgprime           0.254  (mode1-random-scalar-uniform)
  ops.diffusion_loss:dgt               0.339  (mode1-random-scalar-uniform)
  ops.diffusion_loss:dnet              0.250  (mode1-random-scalar-uniform)
  ops.diffusion_loss:dzt               0.250  (mode1-random-scalar-uniform)
  ops.diffusion_loss:loss              0.250  (mode1-random-scalar-uniform)
  ops.poly_gamma:da                    0.299  (abc)
  ops.poly_gamma:db                    0.348  (abc)
  ops.poly_gamma:dc                    0.293  (abc)
  ops.poly_gamma:g0                    0.000  (abc)
  ops.poly_gamma:g1                    0.250  (abc)
  ops.poly_gamma:gprime                0.250  (abc)
  ops.poly_gamma:gt                    0.417  (abc)
  ops.qsample:dg0                      0.277  (random-scalar-g0-13.3-g15)
  ops.qsample:dg1                      0.262  (random-scalar-g0-13.3-g15)
  ops.qsample:dgt                      0.255  (random-scalar-g0-13.3-g15)
  ops.qsample:gbar                     0.150  (random-scalar-g0-13.3-g15)
  ops.qsample:klz                      0.293  (random-scalar-g0-13.3-g15)
  ops.qsample:recon                    0.297  (random-scalar-g0-13.3-g15)
  ops.qsample:var0                     0.031  (random-scalar-g0-13.3-g15)
  ops.qsample:var1                     0.210  (random-scalar-g0-13.3-g15)
  ops.qsample:zt                       0.213  (random-scalar-g0-13.3-g15)
  ops.topk_embedding:dlogits           0.196  (gamma-L50-k15-B7)
  ops.topk_embedding:emb               0.000  (gamma-L50-k15-B7)
  ops.topk_embedding:kl                0.359  (gamma-L50-k15-B7)
  poly_gamma_bwd:da                    0.316  (opposite)
  poly_gamma_bwd:da_p                  0.317  (opposite)
  poly_gamma_bwd:da_t                  0.293  (abc)
  poly_gamma_bwd:db                    0.366  (opposite)
  poly_gamma_bwd:db_p                  0.348  (abc)
  poly_gamma_bwd:db_t                  0.273  (opposite)
  poly_gamma_bwd:dc                    0.324  (opposite)
  poly_gamma_bwd:dc_p                  0.332  (opposite)
  poly_gamma_bwd:dc_t                  0.279  (opposite)
  poly_gamma_fwd:g0                    0.000  (abc)
  poly_gamma_fwd:g1                    0.250  (abc)
  poly_gamma_fwd:gprime                0.252  (opposite)
  poly_gamma_fwd:gt                    0.417  (abc)
  qsample_bwd:dg0                      0.341  (128-elem-g0-13.3-g12)
  qsample_bwd:dg1                      0.307  (zeros-scalar-g0-9.0-g12)
  qsample_bwd:dgt                      0.255  (128-scalar-g0-2.0-g12)
  qsample_bwd:dgt_nogbar               0.256  (random-elem-B1)
  qsample_fwd:gbar                     0.167  (halves-scalar-g0+3.0-g12)
  qsample_fwd:klz                      0.300  (random-elem-B1)
  qsample_fwd:recon                    0.308  (random-elem-B1)
  qsample_fwd:var0                     0.225  (halves-scalar-g0+3.0-g12)
  qsample_fwd:var1                     0.210  (random-scalar-g0-13.3-g15)
  qsample_fwd:zt                       0.244  (random-elem-g0-6.0-g12)
  topk_bwd:dlogits                     0.283  (additive-L50-k15-B7)
  topk_fwd:emb                         0.062  (gamma-L50-k50-B7)
  topk_fwd:kl                          0.410  (gamma-L50-k1-B7)
  topk_fwd:nrm                         0.166  (gamma-L50-k1-B7)
  topk_fwd:soft                        0.313  (gamma-L64-k1-B7)
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import loss_head_oracle as lo

D = lo.D
INVALID = 1                      # hipErrorInvalidValue
WORST = {}


@pytest.fixture(scope="module")
def ops():
    from mulan_amd import ops as _ops
    _ops.lib.load()
    yield _ops
    print("\nworst kernel error / bar per entry point and output")
    for key in sorted(WORST):
        print(f"  {key:36s} {WORST[key][0]:.3f}   ({WORST[key][1]})")


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a)).cuda()


def nans(*shape):
    return torch.full(shape, float("nan"), device="cuda")


def host(t):
    return t.detach().cpu().double().numpy()


def written(t):
    return bool(torch.isfinite(t).all())


def untouched(t):
    return bool(torch.isnan(t).all())


def rc(ops, name, *args):
    """the entry point's return code, unchecked"""
    return getattr(ops.lib.load(), name)(*args)


def held(entry, case, got, ref, twin, names=None):
    names = list(names or got.keys())
    e_k, e_t = lo.errors(got, ref, names), lo.errors(twin, ref, names)
    bad = []
    for n in names:
        bar = lo.bars(e_t[n])
        ratio = e_k[n] / bar
        b = int(np.argmax(ratio))
        print(f"{entry} {case} {n}: kernel {e_k[n][b]:.3e} / twin {e_t[n][b]:.3e} / bar {bar[b]:.3e} (sample {b})")
        key = f"{entry}:{n}"
        if key not in WORST or ratio[b] > WORST[key][0]:
            WORST[key] = (float(ratio[b]), case)
        if not (e_k[n] <= bar).all():
            bad.append((n, b, float(e_k[n][b]), float(bar[b])))
    assert not bad, (entry, case, bad)


# ------------------------------------------------------------------------------------------------ q-sample
@pytest.mark.parametrize("name", [c.name for c in lo.QSAMPLE_CASES])
def test_qsample_fwd_and_bwd(ops, name):
    inp, ref, twin = lo.reference("qsample", name)
    c = lo.by_name(lo.QSAMPLE_CASES)[name]
    B, P, S = c.B, ops.ptr, ops.stream()
    x, g0, g1, gt, e0, e = (dev(inp[k]) for k in ("x", "g0", "g1", "gt", "eps0", "eps"))
    out = nans(B * D + 5 * B)                                   # zt | gbar | recon | klz | var0 | var1, side by side
    zt, small = out[:B * D].view(B, D), out[B * D:].view(5, B)
    ops.call("mulan_qsample_fwd", P(x), P(g0), P(g1), P(gt), c.per_elem, P(e0), P(e), P(zt), *(P(small[i]) for i in range(5)),
             B, D, S)
    assert written(out)
    got = dict(zt=host(zt), **{k: host(small[i]) for i, k in enumerate(("gbar", "recon", "klz", "var0", "var1"))})
    held("qsample_fwd", name, got, ref, twin)

    up = {k: dev(inp[k]) for k in ("dzt", "dgbar", "drecon", "dklz")}
    full = {}
    for with_gbar in (1, 0):
        for want0, want1 in ((1, 1), (1, 0), (0, 1), (0, 0)):
            buf = nans(3, B, D)                                 # dgt | dg0 | dg1, side by side
            ops.call("mulan_qsample_bwd", P(x), P(g0), P(g1), P(gt), c.per_elem, P(e0), P(e), P(up["dzt"]),
                     P(up["dgbar"]) if with_gbar else None, P(up["drecon"]) if want0 else None,
                     P(up["dklz"]) if want1 else None, P(buf[0]), P(buf[1]) if want0 else None,
                     P(buf[2]) if want1 else None, B, D, S)
            assert written(buf[0])
            assert written(buf[1]) if want0 else untouched(buf[1])
            assert written(buf[2]) if want1 else untouched(buf[2])
            if want0 and want1:
                full[with_gbar] = buf
            else:                                               # an output does not depend on which others are asked for
                for i in (0,) + ((1,) if want0 else ()) + ((2,) if want1 else ()):
                    assert torch.equal(buf[i], full[with_gbar][i]), (with_gbar, want0, want1, i)
    assert torch.equal(full[0][1:], full[1][1:])
    got = dict(dgt=host(full[1][0]), dgt_nogbar=host(full[0][0]), dg0=host(full[1][1]), dg1=host(full[1][2]))
    held("qsample_bwd", name, got, ref, twin)


def test_qsample_refusals(ops):
    P, S = ops.ptr, ops.stream()
    B = 1
    x = torch.zeros(B, D, dtype=torch.uint8, device="cuda")
    g, e = torch.zeros(B, D, device="cuda"), torch.zeros(B, D, device="cuda")
    one = torch.ones(B, device="cuda")
    out, small, buf = nans(B, D), nans(5, B), nans(3, B, D)
    fwd = lambda B_, d_: rc(ops, "mulan_qsample_fwd", P(x), P(g), P(g), P(g), 1, P(e), P(e), P(out),
                            *(P(small[i]) for i in range(5)), B_, d_, S)
    bwd = lambda B_, d_, dr, dk, d0, d1: rc(ops, "mulan_qsample_bwd", P(x), P(g), P(g), P(g), 1, P(e), P(e), P(e), P(one),
                                            dr, dk, P(buf[0]), d0, d1, B_, d_, S)
    assert fwd(1, 3071) == INVALID and fwd(1, 3073) == INVALID and fwd(0, D) == INVALID and fwd(-1, D) == INVALID
    assert bwd(1, 3071, P(one), P(one), P(buf[1]), P(buf[2])) == INVALID
    assert bwd(0, D, P(one), P(one), P(buf[1]), P(buf[2])) == INVALID
    assert bwd(1, D, None, P(one), P(buf[1]), P(buf[2])) == INVALID          # dg0 without drecon
    assert bwd(1, D, P(one), None, P(buf[1]), P(buf[2])) == INVALID          # dg1 without dklz
    torch.cuda.synchronize()
    assert untouched(out) and untouched(small) and untouched(buf)
    assert fwd(1, D) == 0 and bwd(1, D, P(one), P(one), P(buf[1]), P(buf[2])) == 0
    assert written(out) and written(small) and written(buf)


# ------------------------------------------------------------------------------------------------ diffusion loss
@pytest.mark.parametrize("name", [c.name for c in lo.DIFFLOSS_CASES])
def test_diffloss_fwd_and_bwd(ops, name):
    inp, ref, twin = lo.reference("diffloss", name)
    c = lo.by_name(lo.DIFFLOSS_CASES)[name]
    B, P, S = c.B, ops.ptr, ops.stream()
    x, gt, gp, e, zt, net, dl = (dev(inp[k]) for k in ("x", "gt", "gp", "eps", "zt", "net", "dloss"))
    loss = nans(2, B)
    ops.call("mulan_diffloss_fwd", c.mode, P(x), P(gt), P(gp), c.per_elem, P(e), P(zt), P(net), P(loss[0]), B, D, S)
    assert written(loss[0]) and untouched(loss[1])
    held(f"diffloss_fwd mode {c.mode}", name, dict(loss=host(loss[0])), ref, twin)
    buf = nans(4, B, D)                                          # dnet | dgt | dgprime | dzt
    ops.call("mulan_diffloss_bwd", c.mode, P(x), P(gt), P(gp), c.per_elem, P(e), P(zt), P(net), P(dl), P(buf[0]), P(buf[1]),
             P(buf[2]), P(buf[3]), B, D, S)
    assert written(buf[:3])
    got = dict(dnet=host(buf[0]), dgt=host(buf[1]), dgprime=host(buf[2]))
    if c.mode == 1:
        assert written(buf[3])
        got["dzt"] = host(buf[3])
    else:                                                        # dzt is written in mode 1 only
        assert untouched(buf[3])
    if c.mode == 2:
        assert not buf[1].any()
    held(f"diffloss_bwd mode {c.mode}", name, got, ref, twin)


def test_diffloss_refusals(ops):
    P, S = ops.ptr, ops.stream()
    x = torch.zeros(1, D, dtype=torch.uint8, device="cuda")
    g = torch.ones(1, D, device="cuda")
    loss, buf = nans(1), nans(4, 1, D)
    fwd = lambda mode, B_, d_: rc(ops, "mulan_diffloss_fwd", mode, P(x), P(g), P(g), 1, P(g), P(g), P(g), P(loss), B_, d_, S)
    bwd = lambda mode, B_, d_: rc(ops, "mulan_diffloss_bwd", mode, P(x), P(g), P(g), 1, P(g), P(g), P(g), P(g[0, :1]), P(buf[0]),
                                  P(buf[1]), P(buf[2]), P(buf[3]), B_, d_, S)
    for f in (fwd, bwd):
        assert [f(-1, 1, D), f(3, 1, D), f(0, 0, D), f(0, -2, D), f(0, 1, 3071), f(0, 1, 2 * D)] == [INVALID] * 6
    torch.cuda.synchronize()
    assert untouched(loss) and untouched(buf)
    assert [fwd(m, 1, D) for m in (0, 1, 2)] == [0, 0, 0] and written(loss)


# ------------------------------------------------------------------------------------------------ polynomial schedule
@pytest.mark.parametrize("name", [c.name for c in lo.POLY_CASES])
def test_poly_gamma_fwd_and_bwd(ops, name):
    inp, ref, twin = lo.reference("poly", name)
    B, P, S = len(lo.POLY_T), ops.ptr, ops.stream()
    a, b, c, t, dgt, dgp = (dev(inp[k]) for k in ("a", "b", "c", "t", "dgt", "dgp"))
    buf = nans(4, B, D)                                          # g0 | g1 | gt | gprime
    ops.call("mulan_poly_gamma_fwd", P(a), P(b), P(c), P(t), P(buf[0]), P(buf[1]), P(buf[2]), P(buf[3]), B, D, lo.GMIN,
             lo.GMAX, S)
    assert written(buf)
    alone = nans(4, B, D)
    ops.call("mulan_poly_gamma_fwd", P(a), P(b), P(c), P(t), None, None, P(alone[2]), None, B, D, lo.GMIN, lo.GMAX, S)
    assert torch.equal(alone[2], buf[2]) and untouched(alone[:2]) and untouched(alone[3])
    # gamma(0) is gamma_min bit for bit: the polynomial at t = 0 is exactly 0
    gmin = torch.full((B, D), float(np.float32(lo.GMIN)), device="cuda")
    assert torch.equal(buf[0], gmin) and torch.equal(buf[2][0], gmin[0])
    held("poly_gamma_fwd", name, dict(g0=host(buf[0]), g1=host(buf[1]), gt=host(buf[2]), gprime=host(buf[3])), ref, twin)
    got = {}
    for tag, u, w in (("", dgt, dgp), ("_t", dgt, None), ("_p", None, dgp)):
        g = nans(3, B, D)
        ops.call("mulan_poly_gamma_bwd", P(a), P(b), P(c), P(t), P(u), P(w), P(g[0]), P(g[1]), P(g[2]), B, D, lo.GMIN,
                 lo.GMAX, S)
        assert written(g)
        got.update({n + tag: host(g[i]) for i, n in enumerate(("da", "db", "dc"))})
    held("poly_gamma_bwd", name, got, ref, twin)


def test_poly_gamma_refusals(ops):
    P, S = ops.ptr, ops.stream()
    a, t, buf = torch.ones(1, D, device="cuda"), torch.ones(1, device="cuda"), nans(4, 1, D)
    fwd = lambda B_, d_: rc(ops, "mulan_poly_gamma_fwd", P(a), P(a), P(a), P(t), P(buf[0]), P(buf[1]), P(buf[2]), P(buf[3]),
                            B_, d_, lo.GMIN, lo.GMAX, S)
    bwd = lambda B_, d_: rc(ops, "mulan_poly_gamma_bwd", P(a), P(a), P(a), P(t), P(a), P(a), P(buf[0]), P(buf[1]), P(buf[2]),
                            B_, d_, lo.GMIN, lo.GMAX, S)
    for f in (fwd, bwd):
        assert [f(0, D), f(-3, D), f(1, 3071), f(1, 1)] == [INVALID] * 4
    torch.cuda.synchronize()
    assert untouched(buf)


# ------------------------------------------------------------------------------------------------ relaxed top-k
def run_topk(ops, c, inp, logits=None):
    """-> (emb, kl, soft, nrm, dlogits) device tensors; noise "none": soft, nrm and dlogits None"""
    P, S = ops.ptr, ops.stream()
    B, L = c.B, c.L
    lg = dev(inp["logits"]) if logits is None else logits
    wide, thin = nans(2, B, L), nans(2, B)                       # emb | soft and kl | nrm, side by side
    if c.noise == "none":
        ops.call("mulan_topk_fwd", P(lg), None, P(wide[0]), P(thin[0]), None, None, B, L, c.k, 10.0, S)
        assert written(wide[0]) and written(thin[0]) and untouched(wide[1]) and untouched(thin[1])
        return wide[0], thin[0], None, None, None
    noise, demb, dkl = dev(inp["noise"]), dev(inp["demb"]), dev(inp["dkl"])      # named: they live until the kernels ran
    ops.call("mulan_topk_fwd", P(lg), P(noise), P(wide[0]), P(thin[0]), P(wide[1]), P(thin[1]), B, L, c.k,
             10.0 if c.noise == "gamma" else -1.0, S)
    assert written(wide) and written(thin)
    dl = nans(2, B, L)
    ops.call("mulan_topk_bwd", P(lg), P(wide[1]), P(thin[1]), P(demb), P(dkl), P(dl[0]), B, L, S)
    assert written(dl[0]) and untouched(dl[1])
    return wide[0], thin[0], wide[1], thin[1], dl[0]


@pytest.mark.parametrize("name", [c.name for c in lo.TOPK_CASES])
def test_topk_fwd_and_bwd(ops, name):
    inp, ref, twin = lo.reference("topk", name)
    c = lo.by_name(lo.TOPK_CASES)[name]
    emb, kl, soft, nrm, dl = run_topk(ops, c, inp)
    hard = np.round(host(emb))
    assert np.array_equal(hard, ref["hard"])                     # the reference's l >= kth set, ties included
    ones = np.full(c.B, c.k)
    if c.noise == "none":
        assert np.array_equal(host(emb), ref["hard"])
        if c.B > lo.TIE_ROW and c.k < c.L:
            ones[lo.TIE_ROW] += 1
    assert np.array_equal(hard.sum(1), ones)
    got = dict(emb=host(emb), kl=host(kl))
    if c.noise != "none":
        got.update(soft=host(soft), nrm=host(nrm)[:, None])
    held("topk_fwd", name, got, ref, twin)
    if c.noise != "none":
        held("topk_bwd", name, dict(dlogits=host(dl)), ref, twin)


@pytest.mark.parametrize("noise", ["gamma", "additive", "none"])
def test_topk_rows_do_not_leak(ops, noise):
    """L = 50 leaves 14 lanes of the wave off; a following row of large logits changes no other row, bit for bit"""
    c = next(c for c in lo.TOPK_CASES if c.noise == noise and c.L == 50 and c.k == 15 and c.B == 7)
    inp = lo.reference("topk", c.name)[0]
    before = run_topk(ops, c, inp)
    lg = dev(inp["logits"]).clone()
    lg[3] = 1e4 * (1 + torch.arange(c.L, device="cuda") % 7)
    after = run_topk(ops, c, inp, lg)
    keep = [r for r in range(c.B) if r != 3]
    for x, y in zip(before, after):
        if x is not None:
            assert torch.equal(x[keep], y[keep])
    assert not torch.equal(before[0][3], after[0][3])


def test_topk_refusals(ops):
    P, S = ops.ptr, ops.stream()
    lg, out, kl = torch.zeros(2, 64, device="cuda"), nans(2, 64), nans(2)
    fwd = lambda B, L, k: rc(ops, "mulan_topk_fwd", P(lg), None, P(out), P(kl), None, None, B, L, k, 10.0, S)
    bwd = lambda B, L: rc(ops, "mulan_topk_bwd", P(lg), P(lg), P(kl), P(lg), P(kl), P(out), B, L, S)
    assert [fwd(2, 65, 1), fwd(2, 0, 1), fwd(2, 64, 0), fwd(2, 64, 65), fwd(0, 64, 1)] == [INVALID] * 5
    assert [bwd(2, 65), bwd(2, 0), bwd(0, 64)] == [INVALID] * 3
    torch.cuda.synchronize()
    assert untouched(out) and untouched(kl)


# ------------------------------------------------------------------------------------------------ the autograd wrappers
def _sums(res, names, ordinary=None):
    """per-sample gradients of a scalar schedule: the sums of the per-element gradients, which are their addends"""
    out = lo.Result({n: res[n].sum(1) for n in names})
    out.add = {n: res[n] for n in names}
    if ordinary is not None:
        out.scale = {n: np.where(np.arange(len(out[n])) == lo.EXACT, np.abs(ordinary[n]).sum(1), np.nan) for n in names}
    return out


def test_ops_wrappers_on_a_scalar_schedule(ops):
    """ops.qsample, ops.diffusion_loss, ops.poly_gamma and ops.topk_embedding once each: the scalar schedule's
    per-element gradients are reduced to one per sample (colsum_raw)"""
    c = next(c for c in lo.QSAMPLE_CASES if c.B == 6 and not c.per_elem and c.image == "random")
    inp, ref, twin = lo.reference("qsample", c.name)
    g0, g1, gt = (dev(inp[k]).requires_grad_() for k in ("g0", "g1", "gt"))
    out = ops.qsample(dev(inp["x"]), g0, g1, gt, dev(inp["eps0"]), dev(inp["eps"]))
    ((out[0] * dev(inp["dzt"])).sum() + (out[1] * dev(inp["dgbar"])).sum() + (out[2] * dev(inp["drecon"])).sum()
     + (out[3] * dev(inp["dklz"])).sum()).backward()
    held("ops.qsample", c.name, dict(zip(("zt", "gbar", "recon", "klz", "var0", "var1"), map(host, out))), ref, twin)
    names = ("dgt", "dg0", "dg1")
    held("ops.qsample", c.name, dict(dgt=host(gt.grad), dg0=host(g0.grad), dg1=host(g1.grad)), _sums(ref, names),
         _sums(twin, names))

    c = next(c for c in lo.DIFFLOSS_CASES if c.B == 6 and not c.per_elem and c.mode == 1 and c.image == "random")
    inp, ref, twin = lo.reference("diffloss", c.name)
    gt, gp, zt, net = (dev(inp[k]).requires_grad_() for k in ("gt", "gp", "zt", "net"))
    loss = ops.diffusion_loss(1, dev(inp["x"]), gt, gp, dev(inp["eps"]), zt, net)
    (loss * dev(inp["dloss"])).sum().backward()
    held("ops.diffusion_loss", c.name, dict(loss=host(loss), dnet=host(net.grad), dzt=host(zt.grad)), ref, twin)
    names = ("dgt", "dgprime")
    held("ops.diffusion_loss", c.name, dict(dgt=host(gt.grad), dgprime=host(gp.grad)), _sums(ref, names, ref.ordinary),
         _sums(twin, names))

    inp, ref, twin = lo.reference("poly", "abc")
    a, b, cc = (dev(inp[k]).requires_grad_() for k in "abc")
    g0_, g1_, ogt, ogp = ops.poly_gamma(a, b, cc, dev(inp["t"]), lo.GMIN, lo.GMAX)
    ((ogt * dev(inp["dgt"])).sum() + (ogp * dev(inp["dgp"])).sum()).backward()
    held("ops.poly_gamma", "abc", dict(g0=host(g0_), g1=host(g1_), gt=host(ogt), gprime=host(ogp), da=host(a.grad),
                                       db=host(b.grad), dc=host(cc.grad)), ref, twin)

    c = next(c for c in lo.TOPK_CASES if c.noise == "gamma" and c.L == 50 and c.k == 15 and c.B == 7)
    inp, ref, twin = lo.reference("topk", c.name)
    lg = dev(inp["logits"]).requires_grad_()
    emb, kl = ops.topk_embedding(lg, dev(inp["noise"]), c.k)
    ((emb * dev(inp["demb"])).sum() + (kl * dev(inp["dkl"])).sum()).backward()
    assert np.array_equal(np.round(host(emb)), ref["hard"])
    held("ops.topk_embedding", c.name, dict(emb=host(emb), kl=host(kl), dlogits=host(lg.grad)), ref, twin)
