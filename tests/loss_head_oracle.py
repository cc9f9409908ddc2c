"""The loss head (mulan_amd/csrc/vdm_loss.hip) restated once over torch tensors of whatever dtype they are given, the
case table its tests share, and the error measure.

Called with float64 tensors the functions are the reference; called with the same fp32-valued inputs as float32 CPU
tensors they are the TWIN: the reference's own arithmetic at the precision the original JAX code runs in.  The twin's
deviation from float64 is the yardstick of every bar in tests/test_gpu_loss_head.py (4 x the twin's error by the same
measure on the same inputs, never below 2^-20 = 16 fp32 ulps; tests/test_gpu_launch_geometry.py::test_expm1_weight is the
precedent for the factor).  tests/test_loss_head_oracle.py holds the functions to oracle/torch_ref.py and to the golden
fixtures, and every case to the usability condition: twin deviation finite and below 1e-4.

encode, logprob, poly_gamma, poly_gamma_grad_t, topk_embedding_and_loss and logits_to_embeddings are torch_ref's; what is
added here is q-sampling, the prior KL, the three diffusion losses and the T expm1 weight, written as
tests/test_gpu_kernels.py spells them out inline.  Every per-sample sum comes with its per-element addends.

The measure, per output and PER SAMPLE (a sample near t = 0 is orders of magnitude smaller than its neighbour near
t = 1, and a max-norm over the batch does not see it):
  sums      |got - want| / sum_i |addend_i| of that sample, addends from the float64 run
  elements  max_i |got - want| / max_i |want| over the sample
  a zero denominator (gamma_t = 0 in every element: gbar; mode 2: dgt) asks for equality
  the exact-target sample of the diffusion loss (net = the target, every output ~ 0 in float64): the denominators of
  the same sample with net = 0, i.e. with a residual of its ordinary size -- the sample is held to zero on its own scale,
  not on its neighbours'.
"""
import functools
import math
import types

import numpy as np
import torch

from oracle import torch_ref as tr

D = 3072
GMIN, GMAX = -13.3, 5.0
FLOOR = 2.0 ** -20        # 16 fp32 ulps: the twin can be exact on a case by accident
MARGIN = 4.0
USABLE = 1e-4             # a case whose twin deviates more says nothing: fp32 itself is ill-conditioned there
T_DISCRETE = 1000.0

f32 = np.float32


# ------------------------------------------------------------------------------------------------ formulas
def q_sample(f, GT, eps):
    """z_t = alpha f + sigma eps (ldm/model_mulan_velocity.py:226-228)"""
    vt = torch.sigmoid(GT)
    return torch.sqrt(1. - vt) * f + torch.sqrt(vt) * eps


def prior_kl(f, G1):
    """per-element KL(q(z_1 | x) || N(0, 1)) (ldm/model_mulan_velocity.py:219-221)"""
    v1 = torch.sigmoid(G1)
    return 0.5 * ((1. - v1) * f * f + v1 - torch.log(v1) - 1.)


def recon_elements(x_int, f, G0, eps0):
    """per-element -log p(x | z_0): tr.logprob with every element as a row of its own"""
    z0 = f + torch.exp(0.5 * G0) * eps0
    return -tr.logprob(x_int.reshape(-1, 1), z0.reshape(-1, 1), G0.reshape(-1, 1)).reshape(f.shape)


def qsample_terms(x_int, G0, G1, GT, eps0, eps):
    """everything mulan_qsample_fwd writes; all [B, D].  -> (outputs, addends of the per-sample sums)"""
    f = tr.encode(x_int.to(eps.dtype))
    add = dict(recon=recon_elements(x_int, f, G0, eps0), klz=prior_kl(f, G1), gbar=GT / D,
               var0=torch.sigmoid(G0) / D, var1=torch.sigmoid(G1) / D)
    out = dict(zt=q_sample(f, GT, eps), recon=add["recon"].sum(1), klz=add["klz"].sum(1), gbar=GT.mean(1),
               var0=torch.sigmoid(G0).mean(1), var1=torch.sigmoid(G1).mean(1))
    return out, add


def velocity_target(f, GT, eps):
    vt = torch.sigmoid(GT)
    return torch.sqrt(1. - vt) * eps - torch.sqrt(vt) * f


def diffusion_loss_elements(mode, x_int, GT, GP, eps, zt, net):
    """mode 0 velocity, 1 velocity from epsilon, 2 epsilon (ldm/model_mulan_velocity.py:246-260,
    ldm/model_mulan_epsilon.py:338-347); the per-element addends of loss_diff"""
    if mode == 2:
        return 0.5 * GP * (eps - net) ** 2
    f = tr.encode(x_int.to(eps.dtype))
    vhat = net if mode == 0 else -torch.exp(0.5 * GT) * zt + torch.sqrt(1. + torch.exp(GT)) * net
    return 0.5 * (1. - torch.sigmoid(GT)) * GP * (velocity_target(f, GT, eps) - vhat) ** 2


def exact_net(mode, x_int, GT, eps, zt):
    """the network output whose residual is zero"""
    if mode == 2:
        return eps.clone()
    v = velocity_target(tr.encode(x_int.to(eps.dtype)), GT, eps)
    return v if mode == 0 else (v + torch.exp(0.5 * GT) * zt) / torch.sqrt(1. + torch.exp(GT))


def expm1_weight(gt, gs, T):
    """discrete-time loss weight (ldm/model_mulan_epsilon.py:348-355)"""
    return T * torch.expm1(gt - gs)


# ------------------------------------------------------------------------------------------------ the measure
def err_sum(got, want, addends):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return _ratio(np.abs(got - want), np.abs(np.asarray(addends, np.float64)).sum(axis=1))


def err_elem(got, want, scale=None):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    B = want.shape[0]
    den = np.abs(want.reshape(B, -1)).max(axis=1) if scale is None else np.asarray(scale, np.float64)
    return _ratio(np.abs(got - want).reshape(B, -1).max(axis=1), den)


def _ratio(num, den):
    with np.errstate(divide="ignore", invalid="ignore"):
        r = num / den
    r = np.where(den == 0, np.where(num == 0, 0.0, np.inf), r)
    return np.where(np.isfinite(num), r, np.inf)


def bars(twin_err):
    return np.maximum(MARGIN * np.asarray(twin_err), FLOOR)


class Result(dict):
    """name -> float64 array; .add: addends of the sums, .scale: denominators that replace max |want| (see above)"""

    def __init__(self, *a, **k):
        super().__init__(*a, **k)
        self.add, self.scale = {}, {}


def errors(got, ref, names=None):
    """per-sample error of every output of `got` (a dict of arrays) against the float64 Result `ref`"""
    out = {}
    for n in names or got.keys():
        if n in ref.add:
            e = err_sum(got[n], ref[n], ref.add[n])
            if n in ref.scale:      # exact-target sample: the sum of |addend| of its ordinary-size residual
                e = np.where(np.isnan(ref.scale[n]), e, _ratio(np.abs(np.asarray(got[n], np.float64) - ref[n]), ref.scale[n]))
        else:
            e = err_elem(got[n], ref[n])
            if n in ref.scale:
                e = np.where(np.isnan(ref.scale[n]), e, err_elem(got[n], ref[n], np.nan_to_num(ref.scale[n], nan=1.0)))
        out[n] = e
    return out


# ------------------------------------------------------------------------------------------------ inputs
IMAGES = ("random", "zeros", "255", "128", "halves")
GAMMA_T_ROWS = (-13.3, 5.0, -15.0, 7.0, 0.0)          # one value per sample; the sixth sample: see gamma_t()
G0_MEANS = (-13.3, -9.0, -6.0, -2.0, 3.0)
# gamma_1 rows: "5" = 5 +- 0.5, "2" = 2 exactly, "max" = G1_MAX: the largest half-integer the usability condition
# admits.  The prior KL's addend is 0.5 ((1 - v1) f^2 + v1 - log v1 - 1) with v1 = sigmoid(gamma_1): fp32 carries 1 - v1
# with an absolute error up to an ulp of 1 (6e-8), and the sum v1 - log v1 likewise, against an addend of about
# (1 - v1) f^2 / 2 + (1 - v1)^2 / 4.  With one gamma_1 for a whole sample the error is systematic, not averaged:
#   natural images (mean f^2 = 1/3): relative 6e-8 / (1 - v1) < 1e-4 / 2  <=>  1 - v1 > 1.2e-3  <=>  gamma_1 <= 6.5
#   the constant image 128 (f^2 = 1.5e-5): only the cancelling (1 - v1)^2 / 4 is left, 6e-8 / ((1 - v1)^2 / 4) < 1e-4 / 2
#     <=> 1 - v1 > 0.07 <=> gamma_1 <= 2.5: image 128 is paired with gamma_1 = 2 only, in the twin and the kernel alike.
G1_MAX = 6.5
G1_ROWS = ("5", "2", "max")
# Two more exclusions the usability condition forced (tests/test_loss_head_oracle.py), for the twin and the kernel alike:
#  - eps0 outliers (x 50 on 32 elements of sample 0) go on the random image (with x = 0 and x = 255 under sixteen each, as
#    tests/test_gpu_kernels.py's bin-window test has them) and on the image 128, not on the images whose every element is
#    0 or 255: there -log p and its gamma_0 gradient are ~0 everywhere but under the outliers, where fp32 forms the
#    gradient as the difference of two numbers near u^2 / 2 = 4500 that agree to 1e-4 (twin deviation 8e-4 at
#    gamma_0 = -9).
#  - one gamma_0 per sample (scalar layout) is not below -13.3: the bins are then more than 6 standard deviations apart
#    in every element, -log p is log(1 + 1e-7) per element and 1e-3 .. 1e-5 per sample, below what fp32 resolves (twin
#    deviation 1e-3 at gamma_0 = -14.2).  The draw is max(-13.3, mean + 0.7 n); a per-element gamma_0 keeps its spread.
OUTLIER_IMAGES = ("random", "128")
TIE_ROW = 2               # the row of a top-k case without noise that has a tie at the threshold
EXACT = 4                 # the sample of a B = 6 batch whose net is the exact target (gamma_t = 0)


def image(kind, B, rng):
    x = rng.integers(0, 256, (B, D)).astype(np.uint8)       # drawn always: the other draws do not depend on the image
    if kind == "random":
        return x
    if kind == "halves":                                     # 32 x 32 x 3 rows: the left 16 columns 0, the right 255
        return np.tile(np.repeat(np.array([0, 255], np.uint8), 48), (B, 32))
    return np.full((B, D), {"zeros": 0, "255": 255, "128": 128}[kind], np.uint8)


def gamma_t(B, per_elem, rng, rows=GAMMA_T_ROWS):
    """B = 6: the five rows and a sixth sample, drawn over [-13.3, 5] per element (per-element layout) or once (scalar
    layout: every sample of the batch has another gamma, so one read through a wrong index changes the answer).
    B = 1: the drawn row alone."""
    drawn = rng.uniform(GMIN, GMAX, D).astype(f32)
    if per_elem:
        rows = [np.full(D, v, f32) for v in rows] + [drawn]
        return np.stack(rows[-B:] if B < 6 else rows)
    vals = np.array(list(rows) + [drawn[0]], f32)
    return vals[-B:] if B < 6 else vals


def schedule_end(mean, spread, B, per_elem, rng, floor=None):
    g = mean + spread * rng.standard_normal((B, D) if per_elem else (B,))
    return (g if floor is None else np.maximum(g, floor)).astype(f32)


def Case(**kw):
    return types.SimpleNamespace(**kw)


def _qsample_cases():
    """images x layouts with the gamma_0 and gamma_1 rows dealt round: every image, gamma_0 mean and gamma_1 row meets
    both layouts; gamma_t brings all its rows in every B = 6 batch"""
    cases = []
    for pe in (1, 0):
        for i, img in enumerate(IMAGES):
            g1 = "2" if img == "128" else G1_ROWS[(i + pe) % 3]
            cases.append(Case(name=f"{img}-{'elem' if pe else 'scalar'}-g0{G0_MEANS[(i + 2 * pe) % 5]:+.1f}-g1{g1}", B=6,
                              image=img, per_elem=pe, g0=G0_MEANS[(i + 2 * pe) % 5], g1=g1, seed=100 + 10 * pe + i))
    cases.append(Case(name="random-elem-B1", B=1, image="random", per_elem=1, g0=-13.3, g1="5", seed=130))
    cases.append(Case(name="halves-scalar-B1", B=1, image="halves", per_elem=0, g0=-6.0, g1="max", seed=131))
    return cases


# mode 1 on the image 128 has gamma_t = 6 in place of 7: with f ~ 0 the target alpha eps is 1/1000 of the prediction
# -e^(g/2) z_t + sqrt(1 + e^g) net, the loss is sigmoid(g) (...)^2 / 2 up to that, and its gamma_t gradient the difference
# of two terms that agree to 1e-3 -- on top of the 6e-5 that fp32 loses in 1 - sigmoid(7) (twin deviation 2.3e-4).  The
# other four images carry the row 7 into mode 1.
GAMMA_T_ROWS_128 = (-13.3, 5.0, -15.0, 6.0, 0.0)


def _diffloss_cases():
    """modes 0 and 1 read the image: each meets all five, both layouts and both weights; mode 2 does not read it"""
    cases = []
    for mode in (0, 1, 2):
        for i in range(6 if mode < 2 else 4):
            pe, wt = 1 - i % 2, ("uniform", "expm1")[(i // 2) % 2]
            img = IMAGES[i % 5]
            rows = GAMMA_T_ROWS_128 if (mode == 1 and img == "128") else GAMMA_T_ROWS
            cases.append(Case(name=f"mode{mode}-{img}-{'elem' if pe else 'scalar'}-{wt}", mode=mode, B=6, image=img,
                              per_elem=pe, weight=wt, seed=200 + 10 * mode + i, rows=rows))
        cases.append(Case(name=f"mode{mode}-random-{'elem' if mode != 1 else 'scalar'}-B1", mode=mode, B=1, image="random",
                          per_elem=int(mode != 1), weight="uniform", seed=240 + mode, rows=GAMMA_T_ROWS))
    return cases


QSAMPLE_CASES = _qsample_cases()
DIFFLOSS_CASES = _diffloss_cases()
# poly_gamma: t per sample; "abc" draws the coefficients as tests/test_gpu_kernels.py::_abc does, "opposite" has a and b
# of opposite sign with c at its floor of 1e-3: S = integral of (a t^2 + b t + c)^2 is then some 1/50 of its addends
POLY_T = (0.0, 1.0, 2.0 ** -24, 1.0 - 2.0 ** -24, 0.5)
POLY_CASES = [Case(name="abc", kind="abc", seed=300), Case(name="opposite", kind="opposite", seed=301)]
# top-k: noise "gamma" = ten Gamma(1/k) draws with tau = 10, "additive" = [B, L] noise added as it is (tau < 0),
# "none" = the hard k-hot of the plain logits
TOPK_CASES = [Case(name=f"{noise}-L{L}-k{k}-B{B}", noise=noise, L=L, k=k, B=B, seed=400 + 7 * L + k + B)
              for noise in ("gamma", "additive", "none") for L in (50, 64) for k in (1, 15, L)
              for B in ((7, 1) if k == 15 else (7,))]


def by_name(cases):
    return {c.name: c for c in cases}


def qsample_inputs(c):
    """fp32-valued numpy inputs of a q-sample case: the float64 reference starts from the numbers the kernel reads"""
    rng = np.random.default_rng(c.seed)
    B = c.B
    x = image(c.image, B, rng)
    gt = gamma_t(B, c.per_elem, rng)
    g0 = schedule_end(c.g0, 0.7, B, c.per_elem, rng, None if c.per_elem else GMIN)
    if c.g1 == "5":
        g1 = schedule_end(5.0, 0.5, B, c.per_elem, rng)
    else:
        g1 = schedule_end(2.0 if c.g1 == "2" else G1_MAX, 0.0, B, c.per_elem, rng)
    e0, e = rng.standard_normal((B, D)).astype(f32), rng.standard_normal((B, D)).astype(f32)
    if c.image in OUTLIER_IMAGES:
        e0[0, :32] *= f32(50.0)                              # z_0 far outside the bins
        if c.image == "random":                              # ... of the end bins too, where the window clamps
            x[0, :16], x[0, 16:32] = 0, 255
    e0[B - 1, 40:48] = 0.0
    up = dict(dzt=rng.standard_normal((B, D)).astype(f32), dgbar=rng.standard_normal(B).astype(f32),
              drecon=rng.standard_normal(B).astype(f32), dklz=rng.standard_normal(B).astype(f32))
    return dict(x=x, g0=g0, g1=g1, gt=gt, eps0=e0, eps=e, **up)


def diffloss_inputs(c):
    rng = np.random.default_rng(c.seed)
    B = c.B
    x = image(c.image, B, rng)
    gt = gamma_t(B, c.per_elem, rng, c.rows)
    shape = (B, D) if c.per_elem else (B,)
    if c.weight == "uniform":
        gp = rng.uniform(5, 30, shape).astype(f32)
    else:                                                   # T expm1(gamma_t - gamma_s), gamma_s up to 0.5 below gamma_t
        gs = gt.astype(np.float64) - rng.uniform(1e-4, 0.5, shape)
        gp = expm1_weight(torch.tensor(gt, dtype=torch.float64), torch.tensor(gs), T_DISCRETE).numpy().astype(f32)
    e, zt, net = (rng.standard_normal((B, D)).astype(f32) for _ in range(3))
    t64 = lambda a: torch.tensor(a, dtype=torch.float64)
    G = t64(gt) if c.per_elem else t64(gt)[:, None] * torch.ones(B, D, dtype=torch.float64)
    if B == 6:
        net[EXACT] = exact_net(c.mode, torch.tensor(x.astype(np.int64)), G, t64(e), t64(zt)).numpy()[EXACT].astype(f32)
    return dict(x=x, gt=gt, gp=gp, eps=e, zt=zt, net=net, dloss=rng.standard_normal(B).astype(f32))


def poly_inputs(c):
    rng = np.random.default_rng(c.seed)
    B = len(POLY_T)
    a = (rng.standard_normal((B, D)) * 0.5).astype(f32)
    if c.kind == "abc":
        b = (rng.standard_normal((B, D)) * 0.5).astype(f32)
        cc = (1e-3 + np.logaddexp(rng.standard_normal((B, D)), 0)).astype(f32)
    else:
        b = (-a * rng.uniform(0.5, 1.0, (B, D))).astype(f32)
        cc = np.full((B, D), 1e-3, f32)
    return dict(a=a, b=b, c=cc, t=np.array(POLY_T, f32), dgt=rng.standard_normal((B, D)).astype(f32),
                dgp=rng.standard_normal((B, D)).astype(f32))


def topk_inputs(c):
    rng = np.random.default_rng(c.seed)
    logits = (rng.standard_normal((c.B, c.L)) * 2).astype(f32)
    noise = None
    if c.noise == "none" and c.B > TIE_ROW and c.k < c.L:    # two logits tied at the threshold: k + 1 ones
        order = np.argsort(-logits[TIE_ROW])
        logits[TIE_ROW, order[c.k]] = logits[TIE_ROW, order[c.k - 1]]
    if c.noise == "gamma":
        noise = rng.gamma(1.0 / c.k, size=(10, c.B, c.L)).astype(f32)
    elif c.noise == "additive":
        noise = rng.gumbel(size=(c.B, c.L)).astype(f32)
    return dict(logits=logits, noise=noise, demb=rng.standard_normal((c.B, c.L)).astype(f32),
                dkl=rng.standard_normal(c.B).astype(f32))


# ------------------------------------------------------------------------------------------------ running a case
def _T(a, dtype, grad=False):
    return torch.tensor(np.asarray(a), dtype=dtype).requires_grad_(grad)


def _np(t):
    return t.detach().double().numpy()


def _spread(g, B, dtype):
    """[B] or [B, D] fp32 schedule -> the [B, D] leaf the per-element gradients are taken at"""
    t = _T(g, dtype)
    return (t if t.dim() == 2 else t[:, None] * torch.ones(B, D, dtype=dtype)).clone().requires_grad_(True)


def run_qsample(inp, dtype):
    """forward outputs and the per-element gradients mulan_qsample_bwd writes, with (dgt) and without (dgt_nogbar) the
    upstream gradient of gbar"""
    B = inp["x"].shape[0]
    x = torch.tensor(inp["x"].astype(np.int64))
    G0, G1, GT = (_spread(inp[k], B, dtype) for k in ("g0", "g1", "gt"))
    out, add = qsample_terms(x, G0, G1, GT, _T(inp["eps0"], dtype), _T(inp["eps"], dtype))
    up = {k: _T(inp[k], dtype) for k in ("dzt", "dgbar", "drecon", "dklz")}
    (dgt_z,) = torch.autograd.grad((out["zt"] * up["dzt"]).sum(), GT, retain_graph=True)
    (dgt_b,) = torch.autograd.grad((out["gbar"] * up["dgbar"]).sum(), GT, retain_graph=True)
    (dg0,) = torch.autograd.grad((out["recon"] * up["drecon"]).sum(), G0, retain_graph=True)
    (dg1,) = torch.autograd.grad((out["klz"] * up["dklz"]).sum(), G1)
    res = Result({k: _np(v) for k, v in out.items()})
    res.update(dgt=_np(dgt_z + dgt_b), dgt_nogbar=_np(dgt_z), dg0=_np(dg0), dg1=_np(dg1))
    res.add = {k: _np(v) for k, v in add.items()}
    return res


def _run_diffloss(mode, inp, net, dtype):
    B = inp["x"].shape[0]
    x = torch.tensor(inp["x"].astype(np.int64))
    GT, GP = _spread(inp["gt"], B, dtype), _spread(inp["gp"], B, dtype)
    zt, nt = _T(inp["zt"], dtype, True), _T(net, dtype, True)
    el = diffusion_loss_elements(mode, x, GT, GP, _T(inp["eps"], dtype), zt, nt)
    loss = el.sum(1)
    grads = torch.autograd.grad((loss * _T(inp["dloss"], dtype)).sum(), [nt, GT, GP, zt], allow_unused=True)
    res = Result(loss=_np(loss))
    for n, g in zip(("dnet", "dgt", "dgprime", "dzt"), grads):
        if g is not None:
            res[n] = _np(g)
    if mode == 2:
        res["dgt"] = np.zeros((B, D))
    res.add = dict(loss=_np(el))
    return res


def run_diffloss(mode, inp, dtype):
    res = _run_diffloss(mode, inp, inp["net"], dtype)
    B = inp["x"].shape[0]
    if B == 6 and dtype == torch.float64:      # the exact-target sample's denominators: the same sample with net = 0
        net0 = inp["net"].copy()
        net0[EXACT] = 0
        ordinary = _run_diffloss(mode, inp, net0, dtype)
        res.ordinary = ordinary
        for n in res:
            full = np.abs(ordinary.add["loss"]).sum(1) if n == "loss" else np.abs(ordinary[n]).reshape(B, -1).max(1)
            res.scale[n] = np.where(np.arange(B) == EXACT, full, np.nan)
        res.scale.pop("dgt") if mode == 2 else None
    return res


def run_poly(inp, dtype):
    """g0, g1, gt, gprime and (da, db, dc) for both upstream gradients, for dgt alone and for dgprime alone.  The limits
    reach the kernel as C floats; the reference takes those values."""
    gmin, gmax = float(f32(GMIN)), float(f32(GMAX))
    a, b, c = (_T(inp[k], dtype, True) for k in "abc")
    t = _T(inp["t"], dtype)
    B = a.shape[0]
    gt, gp = tr.poly_gamma(a, b, c, t, gmin, gmax), tr.poly_gamma_grad_t(a, b, c, t, gmin, gmax)
    res = Result(gt=_np(gt), gprime=_np(gp), g0=_np(tr.poly_gamma(a, b, c, torch.zeros(B, dtype=dtype), gmin, gmax)),
                 g1=_np(tr.poly_gamma(a, b, c, torch.ones(B, dtype=dtype), gmin, gmax)))
    s_t, s_p = (gt * _T(inp["dgt"], dtype)).sum(), (gp * _T(inp["dgp"], dtype)).sum()
    for tag, s in (("", s_t + s_p), ("_t", s_t), ("_p", s_p)):
        for n, g in zip(("da", "db", "dc"), torch.autograd.grad(s, [a, b, c], retain_graph=True)):
            res[n + tag] = _np(g)
    # gamma(1) = gamma_max whatever the coefficients: with dgt alone the quotient rule's two addends R dgt P_a / S and
    # R dgt P S_a / S^2 cancel at t = 1 (and to 1e-7 at t = 1 - 2^-24).  There the denominator is the largest sum of the two
    # addends' magnitudes over the sample, not the largest of their differences.
    S = poly_scale(a, b, c)
    RP = (gt - gmin) * S                                                   # R P, a function of (a, b, c) through autograd
    up = _T(inp["dgt"], dtype).abs()
    for n, pa, sa in zip(("da_t", "db_t", "dc_t"), torch.autograd.grad(RP.sum(), [a, b, c], retain_graph=True),
                         torch.autograd.grad(S.sum(), [a, b, c], retain_graph=True)):
        addends = up * (pa.abs() / S + RP.abs() * sa.abs() / S ** 2)
        res.scale[n] = np.where(np.asarray(inp["t"], np.float64) >= 1.0 - 2.0 ** -24, _np(addends).max(axis=1), np.nan)
    return res


def poly_scale(a, b, c):
    """the scale of tr.poly_gamma: the polynomial at t = 1"""
    return (a ** 2) / 5.0 + (b ** 2 + 2 * a * c) / 3.0 + a * b / 2.0 + b * c + c ** 2


def run_topk(c, inp, dtype):
    """emb, hard, kl (with addends), soft, nrm and dlogits; noise "none": the hard k-hot of tr.logits_to_embeddings and
    the KL alone"""
    lg = _T(inp["logits"], dtype, True)
    q = torch.softmax(lg, dim=1)
    kl_add = q * (torch.log_softmax(lg, dim=1) - math.log(1.0 / c.L))
    if c.noise == "none":
        hard = tr.logits_to_embeddings(lg.detach(), c.k)
        res = Result(emb=_np(hard), hard=_np(hard), kl=_np(tr.gumbel_kl_loss(lg)))
        res.add = dict(kl=_np(kl_add))
        return res
    noise = _T(inp["noise"], dtype)
    kw = dict(gumbel=noise) if c.noise == "additive" else {}
    emb, kl = tr.topk_embedding_and_loss(lg, None if c.noise == "additive" else noise, c.k, **kw)
    (dl,) = torch.autograd.grad((emb * _T(inp["demb"], dtype)).sum() + (kl * _T(inp["dkl"], dtype)).sum(), lg)
    with torch.no_grad():       # the by-products the kernel hands to its backward pass
        l = lg + (noise if c.noise == "additive" else
                  10.0 * (((noise / (c.k / torch.arange(1., 11., dtype=dtype))[:, None, None]).sum(0) - math.log(10.0)) / c.k))
        l = l - l.mean(dim=1, keepdim=True)
        nrm = torch.linalg.norm(l, dim=1)
        soft = l / nrm[:, None]
        srt = torch.sort(l, dim=1, descending=True).values
        gap = (srt[:, c.k - 1] - srt[:, c.k]) if c.k < c.L else torch.full((c.B,), float("inf"), dtype=dtype)
    res = Result(emb=_np(emb), hard=np.round(_np(emb)), kl=_np(kl), soft=_np(soft), nrm=_np(nrm)[:, None], dlogits=_np(dl),
                 gap=_np(gap))
    res.add = dict(kl=_np(kl_add))
    return res


@functools.lru_cache(maxsize=None)
def reference(family, name):
    """(inputs, float64 Result, twin Result) of a case, computed once per process and left unchanged"""
    cases, make, run = {"qsample": (QSAMPLE_CASES, qsample_inputs, lambda c, i, d: run_qsample(i, d)),
                        "diffloss": (DIFFLOSS_CASES, diffloss_inputs, lambda c, i, d: run_diffloss(c.mode, i, d)),
                        "poly": (POLY_CASES, poly_inputs, lambda c, i, d: run_poly(i, d)),
                        "topk": (TOPK_CASES, topk_inputs, run_topk)}[family]
    c = by_name(cases)[name]
    inp = make(c)
    return inp, run(c, inp, torch.float64), run(c, inp, torch.float32)
