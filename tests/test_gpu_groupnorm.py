"""Every exported mulan_groupnorm_* entry point against float64, per (image, group).

Reference: float64 torch from the fp32-valued inputs the kernels read -- oracle/torch_ref.py group_norm + swish and
oracle/mulan_np.py dropout_mask for the forward pass and (through autograd) dx / dgamma / dbeta; mean, rstd, the per-sample
partials, dxsum and the maxima are a few float64 lines here.

Metric: y and dx per (image, group): max|got - ref| over the group's elements / max|ref| over the same elements, so an
error confined to one image, group or slab cannot hide behind a larger neighbour.  mean / rstd / dgamma / dbeta / dxsum
per element, relative to their own reference value (+ fp32 eps x max|reference| where the true value is exactly zero).

Bars.  Well-conditioned data: BAR = 2e-5 (that of test_groupnorm_fwd_bwd, here per group and per element).  Planes:
2^-21 of the bound the kernel reports + BAR; the bound against its closed form, and it must bound the float64 |y|.
Ill-conditioned data (test_cancellation): never fixed in advance -- see its docstring.

Figures the tests print (MI355X, this commit) are recorded in the docstrings of the tests that print them.
"""
import copy
import functools

import numpy as np
import pytest
import torch

from oracle import mulan_np as onp
from oracle import torch_ref as tr

pytestmark = pytest.mark.gpu

HW = 1024
EPS = float(np.float32(1e-6))
BAR = 2e-5
F32_EPS = float(np.finfo(np.float32).eps)
INVALID = 1                      # hipErrorInvalidValue
SEED, OFFSET = 0x1234ABCD5678, 5 << 34
POISON_F, POISON_I = -7.0e37, 0x7F0F0F0F
TUNE_KEYS = (14, 20, 21, 22)

# exported entry point -> the float64-referenced test here that calls it (tests/test_groupnorm_table.py holds it to the header)
COVERAGE = {
    "mulan_groupnorm_fwd": "test_forward_grid",
    "mulan_groupnorm_fwd_dyn": "test_forward_grid",
    "mulan_groupnorm_stats": "test_forward_grid",
    "mulan_groupnorm_fwd_planes": "test_forward_grid",
    "mulan_groupnorm_fwd_planes_keepbits": "test_forward_grid",
    "mulan_groupnorm_fwd_stream": "test_forward_grid",
    "mulan_groupnorm_bwd": "test_backward_grid",
    "mulan_groupnorm_bwd_dyn": "test_backward_grid",
    "mulan_groupnorm_bwd_fused": "test_backward_grid",
    "mulan_groupnorm_bwd_fused_planes": "test_backward_grid",
    "mulan_groupnorm_bwd_stream": "test_backward_grid",
}


@pytest.fixture()
def ops():
    from mulan_amd import ops as _ops
    _ops.lib.load()
    try:
        yield _ops
    finally:
        TUNE.clear()
        for k in TUNE_KEYS:
            _ops.call("mulan_set_tuning", k, 0)


TUNE = {}


def set_tune(ops, k, v):
    TUNE[k] = v
    ops.call("mulan_set_tuning", k, v)


def z_blocks(tune, slabs, fits=True):
    """blocks per slab of a streaming launch: 1 (default), 4 / 2 under tune = 1 / 2, halved until (slabs) x (blocks) fits
    the 16 entries of a maxima array (where one is written)"""
    z = {1: 4, 2: 2}.get(tune, 1)
    while fits and slabs * z > 16:
        z //= 2
    return z


def rc_of(ops, name, *args):
    """the entry point's return code (ops.call raises on a non-zero one)"""
    return int(getattr(ops.lib.load(), name)(*args))


# ------------------------------------------------------------------------------------------------ data
def scale_of(b, g):
    return 10.0 ** ((5 * b + 3 * g) % 7 - 3)


def make_x(B, Ct, G, kind, gen):
    """[B, HW, Ct] fp32.  plain: the 2 N(0,1) + 0.5 of test_groupnorm_fwd_bwd plus a fixed channel offset; scales: image b,
    group g scaled by 10^((5 b + 3 g) mod 7 - 3) (1e-3 .. 1e3 across the tensor, every image and group its own), means of
    both signs, |mean / std| in 0.6 .. 1.0"""
    cpg = Ct // G
    x = torch.randn(B, HW, Ct, device="cuda", generator=gen)
    if kind == "plain":
        return x * 2 + 0.5 + 0.2 * torch.cos(torch.arange(Ct, device="cuda", dtype=torch.float32))
    s = torch.tensor([[scale_of(b, g) for g in range(G)] for b in range(B)], device="cuda")
    m = torch.tensor([[(-1.0) ** (b + g) * (0.6 + 0.1 * (g % 5)) for g in range(G)] for b in range(B)], device="cuda")
    return ((x.view(B, HW, G, cpg) + m[:, None, :, None]) * s[:, None, :, None]).view(B, HW, Ct).contiguous()


@functools.lru_cache(maxsize=8)
def mask_of(shape, keep, seed, offset):
    return torch.from_numpy(onp.dropout_mask(shape, keep, seed, offset)).cuda()


class Case:
    """inputs (fp32, device) and the float64 reference of one (shape, act, keep, data kind)"""

    def __init__(self, B, C1, C2, G, act, keep, kind="plain", seed_word=0, x=None):
        self.B, self.C1, self.C2, self.G, self.act, self.keep = B, C1, C2, G, act, keep
        Ct = self.Ct = C1 + C2
        cpg = self.cpg = Ct // G
        gen = torch.Generator(device="cuda").manual_seed(1000 * C1 + 10 * C2 + G + B)
        x = make_x(B, Ct, G, kind, gen) if x is None else x
        self.x = x
        self.x1 = x[..., :C1].contiguous()
        self.x2 = x[..., C1:].contiguous() if C2 else None
        self.gamma = 1 + 0.2 * torch.randn(Ct, device="cuda", generator=gen)
        self.beta = 0.3 * torch.randn(Ct, device="cuda", generator=gen)
        self.seed_word = seed_word
        self.seed_dev = torch.tensor([seed_word], dtype=torch.int64, device="cuda") if seed_word else None
        k32 = float(np.float32(keep))
        self.mask = mask_of((B, HW, Ct), keep, SEED ^ seed_word, OFFSET) if keep < 1 else None

        # ---- float64: statistics by hand, y through the oracle
        xd = x.double()
        xg = xd.view(B, HW, G, cpg)
        self.mean = xg.mean((1, 3))
        self.var = ((xg - self.mean[:, None, :, None]) ** 2).mean((1, 3))      # (two-pass: exact zero for a constant group)
        self.rstd = 1 / torch.sqrt(self.var + EPS)
        xin = xd.clone().requires_grad_()
        gd, bd = self.gamma.double().requires_grad_(), self.beta.double().requires_grad_()
        y = tr.group_norm(xin.view(B, 32, 32, Ct), {"scale": gd, "bias": bd}, groups=G, eps=EPS).view(B, HW, Ct)
        if act:
            y = tr.swish(y)
        if self.mask is not None:
            y = torch.where(self.mask, y / k32, torch.zeros_like(y))
        self.y = y.detach()
        # ---- an incoming gradient whose channel sums do not cancel: dbeta ~ 0.4 n, dgamma ~ 0.5 n E[act' xhat^2]
        xhat = ((xg - self.mean[:, None, :, None]) * self.rstd[:, None, :, None]).view(B, HW, Ct)
        t = torch.tensor([[scale_of(b + 1, g + 2) for g in range(G)] for b in range(B)], device="cuda")
        if kind == "plain":
            t = torch.ones_like(t)
        dy = (0.7 * torch.randn(B, HW, Ct, device="cuda", generator=gen) + 0.4 + 0.5 * xhat.float())
        self.dy = (dy.view(B, HW, G, cpg) * t[:, None, :, None]).view(B, HW, Ct).contiguous()
        y.backward(self.dy.double())
        self.dx, self.dgamma, self.dbeta = xin.grad, gd.grad, bd.grad
        # ---- by hand: the per-sample partials and the group sums' partial form
        u = xhat * self.gamma.double() + self.beta.double()
        sg = torch.sigmoid(u)
        g = self.dy.double() * (sg * (1 + u * (1 - sg)) if act else 1.0)
        if self.mask is not None:
            g = g * self.mask / k32
        self.dgamma_part, self.dbeta_part = (g * xhat).sum(1), g.sum(1)
        assert float((self.dgamma_part.sum(0) - self.dgamma).abs().max()) <= 1e-7 * float(self.dgamma.abs().max())
        assert float((self.dbeta_part.sum(0) - self.dbeta).abs().max()) <= 1e-7 * float(self.dbeta.abs().max())
        da = g * self.gamma.double()
        part = lambda v: v.view(B, 4, 256, Ct // 4, 4).sum((2, 4))
        self.gstats = torch.stack((part(da), part(da * xhat)), -1).float().contiguous()
        # ---- skip-path gradients of the size of dx in every (image, group), non-zero mean
        dxm = self.dx.abs().view(B, HW, G, cpg).amax((1, 3))[:, None, :, None]
        adds = [((0.3 * torch.randn(B, HW, G, cpg, device="cuda", generator=gen) + 0.2) * dxm.float()).view(B, HW, Ct)
                for _ in range(3)]
        self.add1, self.add1b = adds[0][..., :C1].contiguous(), adds[1][..., :C1].contiguous()
        self.add2 = adds[2][..., C1:].contiguous() if C2 else None
        self.mean32, self.rstd32 = self.mean.float().contiguous(), self.rstd.float().contiguous()

    def xstats(self, tiles):
        """the partial sums a producing convolution leaves: [B][tiles][C / 4][2] per input, formed in float64"""
        out = []
        for v in (self.x1, self.x2):
            if v is None:
                out.append(None)
                continue
            C = v.shape[-1]
            vd = v.double().view(self.B, tiles, HW // tiles, C // 4, 4)
            out.append(torch.stack((vd.sum((2, 4)), (vd * vd).sum((2, 4))), -1).float().contiguous())
        return out

    def dx_total(self, add1=False, add2=False, add1b=False, old=None):
        dx = self.dx.clone()
        if add1:
            dx[..., :self.C1] += self.add1.double()
        if add1b:
            dx[..., :self.C1] += self.add1b.double()
        if add2 and self.C2:
            dx[..., self.C1:] += self.add2.double()
        if old is not None:
            dx += old.double()
        return dx


@functools.lru_cache(maxsize=3)
def case(*a, **k):
    return Case(*a, **k)


# ------------------------------------------------------------------------------------------------ metrics
def group_err(got, ref, G):
    """[B, G]: max|got - ref| / max|ref| over each (image, group)"""
    B, _, C = ref.shape
    d = (got.double() - ref).abs().view(B, HW, G, C // G).amax((1, 3))
    return d / ref.abs().view(B, HW, G, C // G).amax((1, 3)).clamp_min(1e-300)


def each_err(got, ref):
    """max over the elements of |got - ref| / |ref| (floor fp32 eps x max|ref| where the reference is exactly zero)"""
    ref = ref.double()
    floor = (ref == 0).double() * F32_EPS * float(ref.abs().max())
    return float(((got.double() - ref).abs() / (ref.abs() + floor)).max())


def check_groups(tag, got, ref, G, bar=BAR, extra=None):
    e = group_err(got, ref, G)
    lim = torch.full_like(e, bar) if extra is None else bar + extra
    worst = float((e / lim).max())
    print(f"{tag}: worst (image, group) error {float(e.max()):.3g} (bar {bar:g}{'' if extra is None else ' + extra'})")
    assert torch.isfinite(got).all(), tag
    assert worst <= 1.0, (tag, float(e.max()), (e > lim).nonzero()[:4].tolist())


def check_each(tag, got, ref, bar=BAR):
    e = each_err(got, ref)
    print(f"{tag}: worst element error {e:.3g} (bar {bar:g})")
    assert e <= bar, (tag, e)


def decode_planes(planes, bound_bits, B, C):
    """split planes [B][C/16][1024][2][16] fp16 scaled by 2^(140 - e(bound)) -> [B, 1024, C] float64 (as in
    test_gn_planes_bound_and_precision)"""
    raw = planes.view(torch.float16).view(B, C // 16, HW, 2, 16)
    assert torch.isfinite(raw).all()
    p = raw.double()
    bnd = bound_bits.cpu().numpy().view(np.float32).max(1)
    out = torch.empty(B, HW, C, dtype=torch.float64, device=planes.device)
    for b in range(B):
        e = min(max(int(np.frexp(bnd[b])[1]) - 1 + 127, 14), 254)
        out[b] = (p[b, :, :, 0] + p[b, :, :, 1]).permute(1, 0, 2).reshape(HW, C) * 2.0 ** (e - 140)
    return out


def decode_keepbits(kb, B, Ct):
    """[B][Ct/32][prow 32][quad 8][word 4], bit 4 j + e of word w: element e of pixel prow + 32 (8 w + j) -> [B, HW, Ct] bool"""
    S = Ct // 32
    w = kb.view(B, S, 32, 8, 4, 1).to(torch.int64) & 0xFFFFFFFF
    bits = (w >> torch.arange(32, device=kb.device)) & 1                          # [B, S, prow, quad, w, 4 j + e]
    bits = bits.view(B, S, 32, 8, 4, 8, 4).permute(0, 4, 5, 2, 1, 3, 6)          # [B, w, j, prow, S, quad, e]
    return bits.reshape(B, HW, Ct).bool()


def bits_of_max(t):
    """[B] int32: the bit pattern of max|t[b]| (the maxima arrays hold |.| as unsigned bit patterns)"""
    return t.abs().flatten(1).amax(1).view(torch.int32)


def check_maxima(tag, mx, out, used):
    """[B][16] maxima of `out`: the row maximum is the bit pattern of max|out[b]|, entries behind the `used` parts are 0"""
    B = out.shape[0]
    mx = mx.view(B, 16)
    assert torch.equal(mx.amax(1), bits_of_max(out)), tag
    assert int(mx[:, used:].abs().sum()) == 0, (tag, used, mx[:, used:].tolist())
    assert int((mx[:, :used] == POISON_I).sum()) == 0, tag


def fwd_bound(c):
    k32 = np.float32(c.keep)
    return (np.sqrt(np.float32(HW * c.cpg)) * float(c.gamma.abs().max()) + float(c.beta.abs().max())) / float(k32)


def check_fwd_planes(tag, c, planes, bound, extra=None, bar=BAR):
    """decoded planes against float64: 2^-21 of the reported bound + the fp32 bar; the bound against its closed form; it bounds |y|"""
    bnd = bound.cpu().numpy().view(np.float32).reshape(c.B, 16).max(1)
    want = fwd_bound(c)
    assert np.allclose(bnd, want, rtol=1e-6), (tag, bnd, want)
    assert float(c.y.abs().max()) <= bnd.min(), tag
    dec = decode_planes(planes, bound, c.B, c.Ct)
    assert float(dec.abs().max()) <= bnd.max(), tag
    ymax = c.y.abs().view(c.B, HW, c.G, c.cpg).amax((1, 3)).clamp_min(1e-300)
    split = 2.0 ** -21 * torch.tensor(bnd, device="cuda", dtype=torch.float64)[:, None] / ymax
    check_groups(tag, dec, c.y, c.G, bar, split if extra is None else split + extra)
    return dec


def new(*shape, dtype=torch.float32):
    t = torch.empty(*shape, device="cuda", dtype=dtype)
    return t.fill_(POISON_I if dtype == torch.int32 else (0xA5 if dtype == torch.uint8 else POISON_F))


def written(t):
    return bool((t != (POISON_I if t.dtype == torch.int32 else POISON_F)).all())


# ------------------------------------------------------------------------------------------------ launch helpers
def run_fwd(ops, c, name, *, planes=False, ymax=True, keepbits=False, xstats=0, given=False, seed_dev=True, hw=HW):
    """one forward entry point on case c with poisoned outputs -> dict of what it wrote"""
    p, B, Ct = ops.ptr, c.B, c.Ct
    o = {"mean": new(B, c.G), "rstd": new(B, c.G)}
    o["y"] = None if planes else new(B, HW, Ct)
    o["planes"] = new(B * HW * Ct * 4, dtype=torch.uint8) if planes else None
    o["ymax"] = new(B, 16, dtype=torch.int32) if ymax else None
    o["kb"] = new(B * (Ct // 32) * 1024, dtype=torch.int32) if keepbits else None
    sd = c.seed_dev if seed_dev else None
    head = (p(c.x1), p(c.x2), c.C1, c.C2, p(c.gamma), p(c.beta))
    tail = (B, hw, c.G, EPS, c.act, c.keep, SEED, OFFSET)
    if name == "mulan_groupnorm_fwd":
        args = head + (p(o["y"]), p(o["mean"]), p(o["rstd"])) + tail + (p(o["ymax"]), ops.stream())
    elif name == "mulan_groupnorm_fwd_dyn":
        args = head + (p(o["y"]), p(o["mean"]), p(o["rstd"])) + tail + (p(sd), p(o["ymax"]), ops.stream())
    elif name == "mulan_groupnorm_fwd_planes":
        args = head + (p(o["planes"]), p(o["mean"]), p(o["rstd"])) + tail + (p(sd), p(o["ymax"]), ops.stream())
    elif name == "mulan_groupnorm_fwd_planes_keepbits":
        args = head + (p(o["planes"]), p(o["mean"]), p(o["rstd"])) + tail + (p(sd), p(o["ymax"]), p(o["kb"]), ops.stream())
    elif name == "mulan_groupnorm_stats":
        args = head + (p(o["mean"]), p(o["rstd"]), p(o["ymax"]), B, hw, c.G, EPS, ops.stream())
    else:
        assert name == "mulan_groupnorm_fwd_stream"
        xs1, xs2 = c.xstats(xstats) if xstats else (None, None)
        if given:
            o["mean"], o["rstd"] = c.mean32.clone(), c.rstd32.clone()
        args = head + (p(o["y"]), p(o["planes"]), p(o["mean"]), p(o["rstd"]), p(xs1), p(xs2), xstats) + tail + \
            (p(sd), p(o["ymax"]), p(o["kb"]), ops.stream())
    o["rc"] = rc_of(ops, name, *args)
    torch.cuda.synchronize()
    return o


def run_bwd(ops, c, name, *, planes=False, maxima=True, adds=(), accumulate=False, kb=None, sums=True, seed_dev=True,
            bufs=None, hw=HW, null=()):
    """one backward entry point on case c (mean / rstd: the float64 ones rounded to fp32) with poisoned outputs; null:
    buffers ("tick", "dymax") handed over as NULL"""
    p, B, Ct, C1, C2 = ops.ptr, c.B, c.Ct, c.C1, c.C2
    rows = 4 * B if name == "mulan_groupnorm_bwd_stream" else B          # the streaming form leaves up to 4 rows per image
    o = bufs or {}
    if not bufs:
        o["dx1"] = None if planes else new(B, HW, C1)
        o["dx2"] = new(B, HW, C2) if C2 else None
        o["planes"] = new(B * HW * Ct * 4, dtype=torch.uint8) if planes else None
        o["dgp"], o["dbp"] = new(rows, Ct), new(rows, Ct)
        o["dxsp"] = new(rows, Ct) if sums else None
        o["mx1"] = new(B, 16, dtype=torch.int32) if maxima else None
        o["mx2"] = new(B, 16, dtype=torch.int32) if maxima and C2 else None
        o["dg"], o["db"] = new(Ct), new(Ct)
        o["dxs"], o["dxs2"] = (new(C1), new(C1)) if sums else (None, None)
        o["tick"] = torch.zeros(16, device="cuda", dtype=torch.int32)
        if accumulate:
            gen = torch.Generator(device="cuda").manual_seed(5)
            o["old"] = torch.randn(B, HW, Ct, device="cuda", generator=gen) * c.dx.abs().amax((1, 2), keepdim=True).float()
            o["dx1"] = o["old"][..., :C1].clone(memory_format=torch.contiguous_format)
            o["dx2"] = o["old"][..., C1:].clone(memory_format=torch.contiguous_format) if C2 else None
    a1 = c.add1 if "add1" in adds else None
    a2 = c.add2 if "add2" in adds else None
    a1b = c.add1b if "add1b" in adds else None
    sd = c.seed_dev if seed_dev else None
    dymax = ops.absmax_rows(c.dy.view(B, -1)) if planes and "dymax" not in null else None
    if "tick" in null:
        o["tick"] = None
    o["dymax"] = dymax
    stats = (p(c.gamma), p(c.beta), p(c.mean32), p(c.rstd32))
    mid = (B, hw, c.G, c.act, c.keep, SEED, OFFSET)
    tot = (p(o["dxsp"]), p(o["dg"]), p(o["db"]), p(o["dxs"]), p(o["dxs2"]), p(o["tick"]))
    if name in ("mulan_groupnorm_bwd", "mulan_groupnorm_bwd_dyn"):
        args = (p(c.dy), p(c.x1), p(c.x2), C1, C2) + stats + (p(o["dx1"]), p(o["dx2"]), p(o["dgp"]), p(o["dbp"])) + mid + \
            ((p(sd),) if name.endswith("dyn") else ()) + (int(accumulate), p(o["mx1"]), p(o["mx2"]), p(a1), p(a2), p(o["dxsp"]),
                                                          ops.stream())
    elif name == "mulan_groupnorm_bwd_fused":
        args = (p(c.dy), p(c.x1), p(c.x2), C1, C2) + stats + (p(o["dx1"]), p(o["dx2"]), p(o["dgp"]), p(o["dbp"])) + mid + \
            (p(sd), p(o["mx1"]), p(o["mx2"]), p(a1), p(a2), p(a1b)) + tot + (ops.stream(),)
    elif name == "mulan_groupnorm_bwd_fused_planes":
        args = (p(c.dy), p(dymax), p(c.x1), C1) + stats + (p(o["planes"]), p(o["dgp"]), p(o["dbp"])) + mid + \
            (p(sd), p(o["mx1"])) + tot + (p(kb), ops.stream())
    else:
        assert name == "mulan_groupnorm_bwd_stream"
        args = (p(c.dy), p(dymax), p(c.x1), p(c.x2), C1, C2) + stats + \
            (p(c.gstats), p(o["dx1"]), p(o["dx2"]), p(o["planes"]), p(o["dgp"]), p(o["dbp"])) + mid + \
            (p(sd), p(o["mx1"]), p(o["mx2"]), p(a1), p(a2), p(a1b)) + tot + (p(kb), ops.stream())
    o["rc"] = rc_of(ops, name, *args)
    torch.cuda.synchronize()
    if o["rc"] == 0 and not planes:
        o["dx"] = o["dx1"] if o["dx2"] is None else torch.cat((o["dx1"], o["dx2"]), -1)
    return o


def bwd_bound(c):
    """[B]: ((sqrt(n) + 2) (1.1 with SiLU)) max_g rstd[b, g] max|gamma| max|dy[b]| / keep (gn_bwd_kernel_1pass)"""
    f = (np.sqrt(np.float32(HW * c.cpg)) + 2.0) * (np.float32(1.1) if c.act else 1.0)
    return f * c.rstd32.amax(1).double() * float(c.gamma.abs().max()) * c.dy.abs().flatten(1).amax(1).double() / \
        float(np.float32(c.keep))


def check_bwd(tag, c, o, *, adds=(), planes=False, totals=False):
    """what a backward launch left, against float64.  The channel sums of dx (dxsum_part, dxsum) are held to their own
    reference values where the skip-path gradients make them sums that do not cancel (add1, and add2 for a concat): the
    channel sums of a bare GroupNorm gradient add up to zero over every group, so single ones come arbitrarily close to it"""
    assert o["rc"] == 0, (tag, o["rc"])
    B, C1, C2, G = c.B, c.C1, c.C2, c.G
    stream = "stream" in tag
    z = z_blocks(TUNE.get(21, 0), max(C1, C2) // 32, o["mx1"] is not None or o["mx2"] is not None) if stream else 1
    ref = c.dx_total("add1" in adds, "add2" in adds, "add1b" in adds, o.get("old"))
    if planes:
        mx = o["mx1"].view(B, 16)
        bnd = mx.cpu().numpy().view(np.float32).max(1)
        want = bwd_bound(c).cpu().numpy()
        assert np.allclose(bnd, want, rtol=2e-6), (tag, bnd, want)
        assert bool((ref.abs().flatten(1).amax(1).cpu().numpy() <= bnd).all()), tag
        parts = (C1 // 32) * z
        assert bool((mx[:, :parts] == mx[:, :1]).all()) and int(mx[:, parts:].abs().sum()) == 0, (tag, mx.tolist())
        dec = decode_planes(o["planes"], o["mx1"], B, C1)
        assert bool((dec.abs().flatten(1).amax(1).cpu().numpy() <= bnd).all()), tag
        dmax = ref.abs().view(B, HW, G, c.cpg).amax((1, 3)).clamp_min(1e-300)
        check_groups(tag + " dx planes", dec, ref, G, BAR, 2.0 ** -21 * torch.tensor(bnd, device="cuda", dtype=torch.float64)[:, None] / dmax)
    else:
        check_groups(tag + " dx", o["dx"], ref, G)
    sums_ok = "add1" in adds and (C2 == 0 or "add2" in adds)
    # the per-sample partials: row b z + (z block) of [B z][Ct] (z = 1 but in the streaming forms)
    fold = lambda t: t[:B * z].double().view(B, z, -1).sum(1)
    assert written(o["dgp"][:B * z]) and written(o["dbp"][:B * z]), tag
    check_each(tag + " dgamma_part", fold(o["dgp"]), c.dgamma_part)
    check_each(tag + " dbeta_part", fold(o["dbp"]), c.dbeta_part)
    if o["dxsp"] is not None:
        assert written(o["dxsp"][:B * z]), tag
        if sums_ok:
            check_each(tag + " dxsum_part", fold(o["dxsp"]), ref.sum(1))
    if totals:
        assert written(o["dg"]) and written(o["db"]), tag
        check_each(tag + " dgamma", o["dg"], c.dgamma)
        check_each(tag + " dbeta", o["db"], c.dbeta)
        if o["dxs"] is not None:
            assert written(o["dxs"]) and torch.equal(o["dxs"], o["dxs2"]), tag
            if sums_ok:
                check_each(tag + " dxsum", o["dxs"], ref[..., :C1].sum((0, 1)))
        assert int(o["tick"].abs().sum()) == 0, tag
    if not planes:
        for mx, out, C in ((o["mx1"], o["dx"][..., :C1], C1), (o["mx2"], o["dx"][..., C1:], C2)):
            if mx is not None:
                check_maxima(tag + " dxmax", mx, out, (C // 32) * z)


# ------------------------------------------------------------------------------------------------ A: width / split grid
SHAPES = [(128, 0, 32), (256, 0, 32), (512, 0, 32), (1024, 0, 32), (128, 0, 4), (64, 64, 4), (96, 32, 32), (32, 96, 32),
          (384, 128, 32), (128, 384, 32), (256, 256, 32)]
GRID = [pytest.param(C1, C2, G, act, keep, id=f"{C1}+{C2}/{G}-act{act}-keep{keep}")
        for (C1, C2, G) in SHAPES for act in (0, 1) for keep in (1.0, 0.9)]


def check_fwd(tag, c, o, *, ymax_parts=None, stats=True, y=True):
    assert o["rc"] == 0, (tag, o["rc"])
    if stats:
        assert written(o["mean"]) and written(o["rstd"]), tag
        check_each(tag + " mean", o["mean"], c.mean)
        check_each(tag + " rstd", o["rstd"], c.rstd)
    if y:
        check_groups(tag + " y", o["y"], c.y, c.G)
        if c.mask is not None:       # the kept set is the oracle's, bit for bit
            assert torch.equal(o["y"] != 0, c.mask & (c.y != 0)), tag
        if o["ymax"] is not None:
            check_maxima(tag + " ymax", o["ymax"], o["y"], ymax_parts)


def forward_entry_points(ops, c, tag=""):
    """every forward entry point that accepts case c, each against float64; returns the outputs by name"""
    S = c.Ct // 32
    wide = S > 16                                                     # no maxima array, hence no planes
    outs = {}
    o = outs["fwd"] = run_fwd(ops, c, "mulan_groupnorm_fwd", ymax=not wide, seed_dev=False) if not c.seed_word else None
    if o:
        check_fwd(tag + "fwd", c, o, ymax_parts=S)
    d = outs["dyn"] = run_fwd(ops, c, "mulan_groupnorm_fwd_dyn", ymax=not wide)
    check_fwd(tag + "fwd_dyn", c, d, ymax_parts=S)
    if o:
        assert all(torch.equal(o[k], d[k]) for k in ("y", "mean", "rstd")), "fwd / fwd_dyn: the same kernel"
    for tiles in (4, 16) if c.act else (8,):
        s = outs["stream"] = run_fwd(ops, c, "mulan_groupnorm_fwd_stream", ymax=not wide, xstats=tiles)
        check_fwd(tag + f"fwd_stream[xstats {tiles}]", c, s, ymax_parts=S * z_blocks(TUNE.get(20, 0), S))
    s = run_fwd(ops, c, "mulan_groupnorm_fwd_stream", ymax=False, given=True)
    check_fwd(tag + "fwd_stream[given]", c, s, stats=False)
    if wide:
        return outs
    st = outs["stats"] = run_fwd(ops, c, "mulan_groupnorm_stats")
    assert st["rc"] == 0 and bool((st["y"] == POISON_F).all())
    assert torch.equal(st["mean"], d["mean"]) and torch.equal(st["rstd"], d["rstd"])      # promised: same summation order
    bnd = st["ymax"].cpu().numpy().view(np.float32).reshape(c.B, 16)
    want = fwd_bound(c) * float(np.float32(c.keep))                # (no dropout in the statistics pass)
    assert np.allclose(bnd[:, :S], want, rtol=1e-6) and not bnd[:, S:].any(), (bnd, want)
    pl = outs["planes"] = run_fwd(ops, c, "mulan_groupnorm_fwd_planes", planes=True)
    assert pl["rc"] == 0
    check_fwd(tag + "fwd_planes", c, pl, y=False)
    check_fwd_planes(tag + "fwd_planes", c, pl["planes"], pl["ymax"])
    assert int(pl["ymax"][:, S:].abs().sum()) == 0
    assert torch.equal(pl["mean"], d["mean"]) and torch.equal(pl["rstd"], d["rstd"])
    sp = outs["stream_planes"] = run_fwd(ops, c, "mulan_groupnorm_fwd_stream", planes=True, xstats=4, keepbits=c.keep < 1)
    check_fwd(tag + "fwd_stream[planes]", c, sp, y=False)
    check_fwd_planes(tag + "fwd_stream[planes]", c, sp["planes"], sp["ymax"])
    zs = S * z_blocks(TUNE.get(20, 0), S)
    assert torch.equal(sp["ymax"].amax(1), pl["ymax"].amax(1)) and int(sp["ymax"][:, zs:].abs().sum()) == 0
    assert bool((sp["ymax"][:, :zs] == sp["ymax"][:, :1]).all())
    if c.keep < 1:
        kb = outs["keepbits"] = run_fwd(ops, c, "mulan_groupnorm_fwd_planes_keepbits", planes=True, keepbits=True)
        assert kb["rc"] == 0
        assert torch.equal(kb["planes"], pl["planes"]) and torch.equal(kb["ymax"], pl["ymax"])
        assert torch.equal(decode_keepbits(kb["kb"], c.B, c.Ct), c.mask), "stored keep-bits: the oracle's mask"
        assert torch.equal(sp["kb"], kb["kb"])
        dec = decode_planes(kb["planes"], kb["ymax"], c.B, c.Ct)
        assert torch.equal(dec != 0, c.mask & (c.y != 0))
    return outs


@pytest.mark.parametrize("C1,C2,G,act,keep", GRID)
def test_forward_grid(ops, C1, C2, G, act, keep):
    """A (forward): group widths 4, 8, 16, 32 and even / uneven concats through every forward entry point that accepts
    them, per (image, group) against float64.  Observed on MI355X: y <= 1.5e-6, mean <= 2.4e-6, rstd <= 4e-7 (bar 2e-5);
    planes within 2^-21 bound + 2e-5."""
    c = case(2, C1, C2, G, act, keep)
    forward_entry_points(ops, c)
    if c.Ct // 32 > 16:      # more slabs than the maxima array has entries: refused, nothing written
        for name, kw in (("mulan_groupnorm_fwd", dict(seed_dev=False)), ("mulan_groupnorm_fwd_dyn", {}),
                         ("mulan_groupnorm_fwd_stream", dict(given=True)), ("mulan_groupnorm_stats", {}),
                         ("mulan_groupnorm_fwd_planes", dict(planes=True)),
                         ("mulan_groupnorm_fwd_stream", dict(planes=True, given=True))):
            o = run_fwd(ops, c, name, ymax=True, **kw)
            assert o["rc"] == INVALID, (name, o["rc"])
            assert bool((o["ymax"] == POISON_I).all()), name
            assert all((o[k] == (0xA5 if k == "planes" else POISON_F)).all() for k in ("y", "planes") if o[k] is not None), name
            if not kw.get("given"):
                assert (o["mean"] == POISON_F).all() and (o["rstd"] == POISON_F).all(), name


def backward_entry_points(ops, c, tag=""):
    S, wide = c.Ct // 32, c.Ct // 32 > 16
    o = run_bwd(ops, c, "mulan_groupnorm_bwd", maxima=not wide, seed_dev=False) if not c.seed_word else None
    if o:
        check_bwd(tag + "bwd", c, o)
        o = run_bwd(ops, c, "mulan_groupnorm_bwd", maxima=False, sums=False, accumulate=True, adds=("add1", "add2"), seed_dev=False)
        check_bwd(tag + "bwd[acc]", c, o, adds=("add1", "add2"))
    d = run_bwd(ops, c, "mulan_groupnorm_bwd_dyn", maxima=not wide, adds=("add1", "add2"))
    check_bwd(tag + "bwd_dyn[add]", c, d, adds=("add1", "add2"))
    d = run_bwd(ops, c, "mulan_groupnorm_bwd_dyn", maxima=not wide, accumulate=True)
    check_bwd(tag + "bwd_dyn[acc]", c, d)
    if wide:
        return
    adds = ("add1", "add2", "add1b")
    f = run_bwd(ops, c, "mulan_groupnorm_bwd_fused", adds=adds)
    check_bwd(tag + "bwd_fused", c, f, adds=adds, totals=True)
    f0 = run_bwd(ops, c, "mulan_groupnorm_bwd_fused", adds=("add1",))
    check_bwd(tag + "bwd_fused[add1]", c, f0, adds=("add1",), totals=True)
    s = run_bwd(ops, c, "mulan_groupnorm_bwd_stream", adds=adds)
    check_bwd(tag + "bwd_stream", c, s, adds=adds, totals=True)
    if c.C2 == 0:
        fp = run_bwd(ops, c, "mulan_groupnorm_bwd_fused_planes", planes=True)
        check_bwd(tag + "bwd_fused_planes", c, fp, planes=True, totals=True)
        sp = run_bwd(ops, c, "mulan_groupnorm_bwd_stream", planes=True)
        check_bwd(tag + "bwd_stream[planes]", c, sp, planes=True, totals=True)
        assert torch.equal(sp["mx1"].amax(1), fp["mx1"].amax(1))


@pytest.mark.parametrize("C1,C2,G,act,keep", GRID)
def test_backward_grid(ops, C1, C2, G, act, keep):
    """A (backward): the same grid through every backward entry point that accepts it, with add1 / add2 / add1b where it
    takes them and accumulate = 1 onto a non-zero dx.  Observed on MI355X: dx <= 3e-6 per (image, group), dgamma / dbeta /
    dxsum and their per-sample partials <= 6e-6 per element (bar 2e-5)."""
    c = case(2, C1, C2, G, act, keep)
    backward_entry_points(ops, c)
    if c.Ct // 32 > 16:
        for name in ("mulan_groupnorm_bwd", "mulan_groupnorm_bwd_dyn", "mulan_groupnorm_bwd_fused", "mulan_groupnorm_bwd_stream"):
            o = run_bwd(ops, c, name, maxima=True, seed_dev=False)
            assert o["rc"] == INVALID, (name, o["rc"])
            assert all((o[k] == POISON_F).all() for k in ("dx1", "dgp", "dbp", "dg", "db")), name
            assert (o["mx1"] == POISON_I).all(), name


# ------------------------------------------------------------------------------------------------ B: scales
@pytest.mark.parametrize("C1,C2,G", [(128, 128, 32), (96, 32, 32), (128, 0, 4), (512, 0, 32)])
@pytest.mark.parametrize("act,keep", [(1, 1.0), (0, 0.9)])
def test_scales_per_image_and_group(ops, C1, C2, G, act, keep):
    """B: every image and group has its own scale (1e-3 .. 1e3 across the tensor) and means of both signs; with the
    per-(image, group) metric an error in a small image / group is as visible as in a large one.  Forward (all entry points)
    and backward (all entry points).  Observed on MI355X: y <= 1.6e-6, dx <= 3e-6 (bar 2e-5)."""
    c = case(3, C1, C2, G, act, keep, "scales")
    outs = forward_entry_points(ops, c)
    backward_entry_points(ops, c)
    # the planes carry one scale per IMAGE (the a-priori bound): they cannot resolve below 2^-21 of it, which the bar grants


# ------------------------------------------------------------------------------------------------ C: cancellation
def host_fp32_stats(x, G):
    """mean and RAW (unclamped) variance E[x^2] - E[x]^2 per (image, group) in fp32 on the host, in four summation orders:
    0: the slab kernel's tree (per thread 32 pixels of a float4 in order, butterfly over the 8 pixel rows of a wave, then
    the group's quads x 4 waves in order); 1: numpy's pairwise sums over (pixel, channel)"""
    x = np.asarray(x, dtype=np.float32)
    B, _, Ct = x.shape
    cpg, f = Ct // G, np.float32
    inv_n = f(1.0) / f(HW * cpg)
    out = []
    v = x.reshape(B, 32, 32, Ct // 4, 4)                               # [b, i, prow, quad (global), e]
    s1, s2 = np.zeros((B, 32, Ct // 4), f), np.zeros((B, 32, Ct // 4), f)
    for i in range(32):
        w = v[:, i]
        s1 = s1 + ((w[..., 0] + w[..., 1]) + (w[..., 2] + w[..., 3]))
        s2 = s2 + ((w[..., 0] * w[..., 0] + w[..., 1] * w[..., 1]) + (w[..., 2] * w[..., 2] + w[..., 3] * w[..., 3]))
    tree = lambda s: (lambda r: ((r[:, :, 0] + r[:, :, 1]) + (r[:, :, 2] + r[:, :, 3])) +
                      ((r[:, :, 4] + r[:, :, 5]) + (r[:, :, 6] + r[:, :, 7])))(s.reshape(B, 4, 8, Ct // 4))   # [b, wave, quad]
    t1, t2 = tree(s1).reshape(B, 4, G, cpg // 4), tree(s2).reshape(B, 4, G, cpg // 4)
    a1, a2 = np.zeros((B, G), f), np.zeros((B, G), f)
    for q in range(cpg // 4):
        for wv in range(4):
            a1, a2 = a1 + t1[:, wv, :, q], a2 + t2[:, wv, :, q]
    xg = x.reshape(B, HW, G, cpg)
    sums = [(a1, a2), (xg.sum((1, 3), dtype=f), (xg * xg).sum((1, 3), dtype=f))]
    xd = x.astype(np.float64)
    for tiles in (4, 8):            # 2, 3: the streaming kernel's order over a producer's partial sums (exact, rounded to fp32)
        t = xd.reshape(B, tiles, HW // tiles, G, cpg // 4, 4)
        p1, p2 = t.sum((2, 5)).astype(f), (t * t).sum((2, 5)).astype(f)       # [b, tile, group, quad]
        b1, b2 = np.zeros((B, G), f), np.zeros((B, G), f)
        for q in range(cpg // 4):
            for tl in range(tiles):
                b1, b2 = b1 + p1[:, tl, :, q], b2 + p2[:, tl, :, q]
        sums.append((b1, b2))
    for (u1, u2) in sums:
        mean = (u1 * inv_n).astype(f)
        out.append((mean, ((u2 * inv_n).astype(f) - (mean * mean).astype(f)).astype(f)))
    return out


CANCEL = {"r300": 300.0, "r3000": 3000.0}


def make_cancel_x(B, Ct, G):
    """ordinary groups (1.5 N(0,1) + 0.3) with, in every image, four special groups whose slab neighbours are ordinary:
    group 1: mean / std = 300, group 3: mean / std = 3000, group 4: exactly constant (a generic fp32 value, another in every
    image), group 6: all zero.  At cpg 4 groups 1, 3, 4, 6 share slab 0 with groups 0, 2, 5, 7; at cpg 8 slabs 0 and 1."""
    cpg = Ct // G
    gen = torch.Generator(device="cuda").manual_seed(77 + Ct)
    x = (torch.randn(B, HW, Ct, device="cuda", generator=gen) * 1.5 + 0.3).view(B, HW, G, cpg)
    z = torch.randn(B, HW, 2, cpg, device="cuda", generator=gen)
    for b in range(B):
        sd = 0.5 * (b + 1)
        x[b, :, 1] = z[b, :, 0] * sd + 300.0 * sd
        x[b, :, 3] = z[b, :, 1] * sd - 3000.0 * sd
        x[b, :, 4] = (3.7, -1000.3, 0.0123)[b % 3]
        x[b, :, 6] = 0.0
    return x.view(B, HW, Ct).contiguous()


@pytest.mark.parametrize("C1,C2,G", [(128, 0, 32), (128, 128, 32), (96, 32, 32)])
@pytest.mark.parametrize("act", [0, 1])
def test_cancellation(ops, C1, C2, G, act):
    """C: groups with mean / std = 300 and 3000, an exactly constant group and an all-zero group next to ordinary groups in
    the same slab (cpg 4 and 8), through every forward entry point.

    Bar (never fixed in advance): delta_var[b, g] = 4 x the largest deviation from float64 of the fp32 host evaluation of
    E[x^2] - E[x]^2 (the slab kernel's order, numpy's, and the streaming kernel's over 4 and 8 row tiles: host_fp32_stats),
    delta_mean likewise.  A kernel may then report any
    rstd in [1 / sqrt(var + delta_var + eps), 1 / sqrt(max(0, var - delta_var) + eps)] (+ 2e-5), and y may deviate by what
    that interval and delta_mean do to (x - mean) rstd gamma (times 1.1, the Lipschitz constant of SiLU), on top of 2e-5.
    Checked on the host here: the fp32 evaluation is finite for every group.  Its raw variance is <= 0 -- the clamp acts --
    in the constant and the all-zero groups and, in some images and orders, ALSO in the mean / std = 3000 group: there
    var / mean^2 = 1.1e-7 is one ulp of E[x^2], the fp32 difference comes out anywhere in about -18 .. +15 times the true
    variance (so that group is held to finiteness, the interval above and the planes' bound only).  The ordinary groups
    and the mean / std = 300 group never hit it; ordinary groups get delta_var / var < 1e-5, so their bar stays 2e-5: a
    bad group leaking into its slab neighbours fails.
    Host figures: delta_var / var = 4 x 0.003 .. 0.25 (mean / std 300), 4 x 1 .. 19 (3000); raw fp32 variance of the
    constant groups 3.7 / -1000.3 / 0.0123: +9.5e-6 / -0.625 / -7e-11 (kernel order), +4e-4 / -25.8 / +5e-9 (numpy order).
    Planes on this input: no inf / NaN in any plane, decoded |y| <= the reported bound (the fmed3 clamp: a group whose
    fp32 variance collapsed has |xhat| far above sqrt(n))."""
    B, Ct, cpg = 3, C1 + C2, (C1 + C2) // G
    c = Case(B, C1, C2, G, act, 1.0, "cancel", 0, make_cancel_x(B, Ct, G))
    orders = host_fp32_stats(c.x.cpu().numpy(), G)
    mean64, var64 = c.mean.cpu().numpy(), c.var.cpu().numpy()
    special = np.zeros((B, G), bool)
    special[:, [3, 4, 6]] = True
    dvar, dmean = np.zeros((B, G)), np.zeros((B, G))
    for mean32, raw32 in orders:
        assert np.isfinite(mean32).all() and np.isfinite(raw32).all()
        assert not (raw32[~special] <= 0).any(), "ordinary groups and mean / std = 300 never hit the clamp"
        assert (raw32[:, 6] == 0).all()
        dvar = np.maximum(dvar, np.abs(raw32.astype(np.float64) - var64))
        dmean = np.maximum(dmean, np.abs(mean32.astype(np.float64) - mean64))
    assert (np.minimum.reduce([r[1][:, 4] for r in orders]) < 0).any(), "a constant group whose raw fp32 variance is negative"
    dvar, dmean = 4 * dvar, 4 * dmean
    plain = np.ones((B, G), bool)
    plain[:, [1, 3, 4, 6]] = False
    assert (dvar[plain] / var64[plain]).max() < 1e-5
    print("host fp32 deviation of E[x^2] - E[x]^2, x 4, relative to the variance: mean / std 300: %.3g, 3000: %.3g; of the "
          "constant groups (absolute): %s" % ((dvar[:, 1] / var64[:, 1]).max(), (dvar[:, 3] / var64[:, 3]).max(), dvar[:, 4]))
    dv, dm = (torch.tensor(a, device="cuda") for a in (dvar, dmean))
    r_lo = 1 / torch.sqrt(c.var + dv + EPS) * (1 - BAR)
    r_hi = 1 / torch.sqrt((c.var - dv).clamp_min(0) + EPS) * (1 + BAR)
    xg = c.x.double().view(B, HW, G, cpg)
    spread = (xg - c.mean[:, None, :, None]).abs().amax((1, 3))
    gmax = c.gamma.double().abs().view(G, cpg).amax(1)
    ymax = c.y.abs().view(B, HW, G, cpg).amax((1, 3)).clamp_min(1e-300)
    extra = 1.1 * gmax * (dm * r_hi + (spread + dm) * (r_hi - r_lo)) / ymax
    m_bar = dm + BAR * c.mean.abs()

    def check(tag, o, y=None, planes=False):
        assert o["rc"] == 0, tag
        assert torch.isfinite(o["mean"]).all() and torch.isfinite(o["rstd"]).all(), tag
        assert bool(((o["mean"].double() - c.mean).abs() <= m_bar).all()), (tag, "mean")
        r = o["rstd"].double()
        assert bool(((r >= r_lo) & (r <= r_hi)).all()), (tag, "rstd", ((r < r_lo) | (r > r_hi)).nonzero().tolist())
        if planes:
            check_fwd_planes(tag, c, o["planes"], o["ymax"], extra)
        elif y is not False:
            check_groups(tag + " y", o["y"], c.y, G, BAR, extra)

    check("fwd_dyn", run_fwd(ops, c, "mulan_groupnorm_fwd_dyn"))
    check("fwd", run_fwd(ops, c, "mulan_groupnorm_fwd", seed_dev=False))
    check("stats", run_fwd(ops, c, "mulan_groupnorm_stats"), y=False)
    check("fwd_planes", run_fwd(ops, c, "mulan_groupnorm_fwd_planes", planes=True), planes=True)
    check("fwd_stream[xstats]", run_fwd(ops, c, "mulan_groupnorm_fwd_stream", xstats=8))
    check("fwd_stream[planes]", run_fwd(ops, c, "mulan_groupnorm_fwd_stream", planes=True, xstats=4), planes=True)


# ------------------------------------------------------------------------------------------------ D: by-products
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("C1,C2,G", [(96, 32, 32), (128, 384, 32), (256, 0, 32)])
def test_byproducts_written_zeroed_and_rearmed(ops, B, C1, C2, G):
    """D: poisoned outputs; afterwards every entry the contract names is written, the maxima behind the used parts are 0,
    their maximum is the bit pattern of max|output|, the tickets are back at zero, and a second launch on the same buffers
    leaves the same totals bit for bit.  (The float64 checks of the same quantities: check_bwd / check_fwd.)"""
    c = case(B, C1, C2, G, 1, 0.9)
    outs = forward_entry_points(ops, c)
    S = c.Ct // 32
    for k in ("fwd", "dyn", "planes", "stream_planes"):
        assert written(outs[k]["mean"]) and written(outs[k]["rstd"]), k
        assert written(outs[k]["ymax"][:, :S]), k
    adds = ("add1", "add2", "add1b")
    for name in ("mulan_groupnorm_bwd_fused", "mulan_groupnorm_bwd_stream"):
        o = run_bwd(ops, c, name, adds=adds)
        check_bwd(name, c, o, adds=adds, totals=True)
        for k in ("dx1", "dx2", "dg", "db", "dxs", "dxs2"):
            assert o[k] is None or written(o[k]), (name, k)
        first = {k: o[k].clone() for k in ("dx1", "dx2", "dg", "db", "dxs", "dxs2", "mx1", "mx2", "dgp", "dbp", "dxsp")
                 if o[k] is not None}
        o2 = run_bwd(ops, c, name, adds=adds, bufs=o)
        assert o2["rc"] == 0 and int(o2["tick"].abs().sum()) == 0
        for k, v in first.items():
            assert torch.equal(v, o2[k]), (name, k)
    if C2 == 0:
        for name in ("mulan_groupnorm_bwd_fused_planes", "mulan_groupnorm_bwd_stream"):
            o = run_bwd(ops, c, name, planes=True)
            check_bwd(name + "[planes]", c, o, planes=True, totals=True)
            assert written(o["dg"]) and written(o["db"]) and written(o["dxs"]) and int(o["tick"].abs().sum()) == 0


def test_fused_backward_reduces_65_samples_in_the_launch(ops):
    """D: the in-launch reduction over the samples of mulan_groupnorm_bwd_fused (16 interleaved sample lanes, batches of 8
    per lane: 65 samples leave the last batch ragged) against the float64 sum over samples"""
    c = case(65, 32, 0, 8, 1, 1.0)
    adds = ("add1", "add1b")
    o = run_bwd(ops, c, "mulan_groupnorm_bwd_fused", adds=adds)
    check_bwd("bwd_fused B=65", c, o, adds=adds, totals=True)
    s = run_bwd(ops, c, "mulan_groupnorm_bwd_stream", adds=adds)
    check_bwd("bwd_stream B=65", c, s, adds=adds, totals=True)


# ------------------------------------------------------------------------------------------------ E: dropout
@pytest.mark.parametrize("C1,C2", [(96, 32), (128, 384)])
def test_dropout_offsets_seed_word_and_keepbits(ops, C1, C2):
    """E: offset 5 << 34, a seed_dev word that changes the seed, an uneven concat.  The kept set is onp.dropout_mask bit for
    bit (forward_entry_points checks every fp32 output and the decoded keep-bits of _fwd_planes_keepbits and _fwd_stream
    against it); the backward pass fed with the stored keep-bits equals the one that re-draws, bit for bit."""
    word = 0x5DEECE66D1234
    c = case(2, C1, C2, 32, 1, 0.9, "plain", word)
    assert not torch.equal(c.mask, mask_of((2, HW, c.Ct), 0.9, SEED, OFFSET))     # the word does change the mask
    outs = forward_entry_points(ops, c)
    backward_entry_points(ops, c)
    kb = outs["keepbits"]["kb"]
    plain = run_fwd(ops, c, "mulan_groupnorm_fwd_dyn", seed_dev=False)            # without the word: another kept set
    assert not torch.equal(plain["y"] != 0, outs["dyn"]["y"] != 0)
    adds = ("add1", "add2", "add1b")
    a = run_bwd(ops, c, "mulan_groupnorm_bwd_stream", adds=adds)
    b = run_bwd(ops, c, "mulan_groupnorm_bwd_stream", adds=adds, kb=kb)
    for k in ("dx1", "dx2", "dg", "db", "dxs", "mx1", "mx2"):
        assert torch.equal(a[k], b[k]), k
    wrong = run_bwd(ops, c, "mulan_groupnorm_bwd_stream", adds=adds, kb=torch.full_like(kb, -1))   # (the bits ARE read)
    assert not torch.equal(a["dx1"], wrong["dx1"])


def test_dropout_keepbits_feed_the_planes_backward(ops):
    """E: single input (the planes backward takes no concat): _bwd_fused_planes and _bwd_stream with planes, stored
    keep-bits against the re-draw, bit for bit, both against float64"""
    c = case(2, 128, 0, 32, 1, 0.9, "plain", 0x77)
    kb = run_fwd(ops, c, "mulan_groupnorm_fwd_planes_keepbits", planes=True, keepbits=True)
    assert torch.equal(decode_keepbits(kb["kb"], c.B, c.Ct), c.mask)
    for name in ("mulan_groupnorm_bwd_fused_planes", "mulan_groupnorm_bwd_stream"):
        a = run_bwd(ops, c, name, planes=True)
        b = run_bwd(ops, c, name, planes=True, kb=kb["kb"])
        check_bwd(name + "[planes, keep-bits]", c, b, planes=True, totals=True)
        for k in ("planes", "dg", "db", "dxs", "mx1"):
            assert torch.equal(a[k], b[k]), (name, k)


# ------------------------------------------------------------------------------------------------ F: variants
VARIANTS = ["14=1", "20=1", "20=2", "21=1", "21=2", "22=1", "22=2", "21=1,22=2"]


@pytest.mark.parametrize("C1,C2", [(128, 128), (96, 32)])
@pytest.mark.parametrize("tune", VARIANTS)
def test_dev_variants_hold_the_same_bars(ops, C1, C2, tune):
    """F: the kernels behind tune[14] (plain loads), tune[20] / tune[21] (quarters of a slab per block) and tune[22] (load
    batches) on the scales case, same float64 bars; bit for bit the default where the code promises the same order:
    tune[14] (the same kernel but for the load policy: everything) and tune[20] (mean / rstd from the partial sums in a
    fixed order, the keep-bits)."""
    c = case(3, C1, C2, 32, 1, 0.9, "scales")
    adds = ("add1", "add2", "add1b")
    base_f = run_fwd(ops, c, "mulan_groupnorm_fwd_dyn")
    base_s = run_fwd(ops, c, "mulan_groupnorm_fwd_stream", planes=True, xstats=4, keepbits=True)
    keys = []
    for kv in tune.split(","):
        k, v = kv.split("=")
        keys.append(int(k))
        set_tune(ops, int(k), int(v))
    if 14 in keys:
        outs = forward_entry_points(ops, c)
        assert all(torch.equal(outs["dyn"][k], base_f[k]) for k in ("y", "mean", "rstd", "ymax"))
    elif 20 in keys:      # statistics from the partial sums in a fixed order, the keep-bits are integers: the same bits
        outs = forward_entry_points(ops, c)
        s = outs["stream_planes"]
        assert all(torch.equal(s[k], base_s[k]) for k in ("mean", "rstd", "kb"))
        assert torch.equal(s["ymax"].amax(1), base_s["ymax"].amax(1))
    else:
        o = run_bwd(ops, c, "mulan_groupnorm_bwd_stream", adds=adds)
        check_bwd("bwd_stream[" + tune + "]", c, o, adds=adds, totals=True)
        assert torch.equal(o["mx1"].amax(1), bits_of_max(o["dx"][..., :C1]))
        o = run_bwd(ops, c, "mulan_groupnorm_bwd_stream", adds=adds, maxima=False)      # no maxima array: nothing caps the z blocks
        check_bwd("bwd_stream[" + tune + ", no maxima]", c, o, adds=adds, totals=True)


# ------------------------------------------------------------------------------------------------ G: past 2^31 bytes
def test_images_past_two_gigabytes(ops):
    """G: Ct = 512, B = 1025: image 1024 starts 2^31 bytes into x, y, dy and dx.  The fp32 entry points (_fwd_dyn, _bwd_dyn,
    _bwd_fused, _fwd_stream with fp32 output) form every image's base address in 64 bits (size_t b * HW * ld; the
    streaming kernels build one buffer resource per image from it and keep only the in-image offset, < 2^21 bytes, in 32
    bits), so they must compute it: images 0 and 1024 and their by-product rows against float64."""
    B, C, G = 1025, 512, 32
    gen = torch.Generator(device="cuda").manual_seed(9)
    x = torch.empty(B, HW, C, device="cuda").normal_(generator=gen).mul_(2).add_(0.5)
    dy = torch.empty(B, HW, C, device="cuda").normal_(generator=gen).mul_(0.7).add_(0.275).add_(x, alpha=0.25)
    add1 = torch.empty(B, HW, C, device="cuda").normal_(generator=gen).mul_(0.3).add_(0.5)    # (channel sums that do not cancel)
    assert x.data_ptr() and (B - 1) * HW * C * 4 >= 2 ** 31
    pick = [0, B - 1]
    c = Case(2, C, 0, G, 1, 1.0, x=x[pick].contiguous())                 # gamma, beta and the float64 reference of two images
    dyd = dy[pick].double()
    p = ops.ptr
    y, mean, rstd = new(B, HW, C), new(B, G), new(B, G)
    ymax = new(B, 16, dtype=torch.int32)
    ops.call("mulan_groupnorm_fwd_dyn", p(x), None, C, 0, p(c.gamma), p(c.beta), p(y), p(mean), p(rstd), B, HW, G, EPS, 1, 1.0, 0, 0,
             None, p(ymax), ops.stream())
    check_groups("2 GB fwd_dyn y", y[pick], c.y, G)
    check_each("2 GB fwd_dyn mean", mean[pick], c.mean)
    check_each("2 GB fwd_dyn rstd", rstd[pick], c.rstd)
    check_maxima("2 GB fwd_dyn ymax", ymax[pick].contiguous(), y[pick], 16)
    y2, ymax2 = y.fill_(POISON_F), new(B, 16, dtype=torch.int32)
    ops.call("mulan_groupnorm_fwd_stream", p(x), None, C, 0, p(c.gamma), p(c.beta), p(y2), None, p(mean), p(rstd), None, None, 0,
             B, HW, G, EPS, 1, 1.0, 0, 0, None, p(ymax2), None, ops.stream())
    check_groups("2 GB fwd_stream y", y2[pick], c.y, G)
    check_maxima("2 GB fwd_stream ymax", ymax2[pick].contiguous(), y2[pick], 16)
    del y, y2
    # backward: float64 from the two images' x and dy (sum over samples: of the whole batch only for these two rows)
    xin = c.x.double().requires_grad_()
    gd, bd = c.gamma.double(), c.beta.double()
    tr.swish(tr.group_norm(xin.view(2, 32, 32, C), {"scale": gd, "bias": bd}, groups=G, eps=EPS)).view(2, HW, C).backward(dyd)
    ref_dx = xin.grad + add1[pick].double()
    xhat = ((c.x.double().view(2, HW, G, C // G) - c.mean[:, None, :, None]) * c.rstd[:, None, :, None]).view(2, HW, C)
    u = xhat * gd + bd
    sg = torch.sigmoid(u)
    g = dyd * sg * (1 + u * (1 - sg))
    for name in ("mulan_groupnorm_bwd_dyn", "mulan_groupnorm_bwd_fused"):
        dx, dgp, dbp, dxsp = new(B, HW, C), new(B, C), new(B, C), new(B, C)
        mx = new(B, 16, dtype=torch.int32)
        if name.endswith("dyn"):
            ops.call(name, p(dy), p(x), None, C, 0, p(c.gamma), p(c.beta), p(mean), p(rstd), p(dx), None, p(dgp), p(dbp), B, HW, G, 1,
                     1.0, 0, 0, None, 0, p(mx), None, p(add1), None, p(dxsp), ops.stream())
        else:
            dg, db, dxs = new(C), new(C), new(C)
            tick = torch.zeros(16, device="cuda", dtype=torch.int32)
            ops.call(name, p(dy), p(x), None, C, 0, p(c.gamma), p(c.beta), p(mean), p(rstd), p(dx), None, p(dgp), p(dbp), B, HW, G, 1,
                     1.0, 0, 0, None, p(mx), None, p(add1), None, None, p(dxsp), p(dg), p(db), p(dxs), None, p(tick), ops.stream())
            assert int(tick.abs().sum()) == 0
            # the totals over all 1025 samples: the float64 sum of the per-sample partials the launch left (each checked
            # for the two images below)
            check_each("2 GB bwd_fused dgamma", dg, dgp.double().sum(0))
            check_each("2 GB bwd_fused dbeta", db, dbp.double().sum(0))
            check_each("2 GB bwd_fused dxsum", dxs, dxsp.double().sum(0))
        check_groups("2 GB " + name + " dx", dx[pick], ref_dx, G)
        check_each("2 GB " + name + " dgamma_part", dgp[pick], (g * xhat).sum(1))
        check_each("2 GB " + name + " dbeta_part", dbp[pick], g.sum(1))
        check_each("2 GB " + name + " dxsum_part", dxsp[pick], ref_dx.sum(1))
        check_maxima("2 GB " + name + " dxmax", mx[pick].contiguous(), dx[pick], 16)
        del dx


# ------------------------------------------------------------------------------------------------ H: refusals
# label -> (entry point, the launch helper's keywords); the streaming forms twice each: fp32 output (forward: mean / rstd
# given), and planes (forward: + stored keep-bits)
ENTRIES = {
    "fwd": ("mulan_groupnorm_fwd", dict(seed_dev=False)),
    "fwd_dyn": ("mulan_groupnorm_fwd_dyn", {}),
    "fwd_planes": ("mulan_groupnorm_fwd_planes", dict(planes=True)),
    "fwd_planes_keepbits": ("mulan_groupnorm_fwd_planes_keepbits", dict(planes=True, keepbits=True)),
    "stats": ("mulan_groupnorm_stats", {}),
    "fwd_stream": ("mulan_groupnorm_fwd_stream", dict(given=True)),
    "fwd_stream[planes,keepbits]": ("mulan_groupnorm_fwd_stream", dict(given=True, planes=True, keepbits=True)),
    "bwd": ("mulan_groupnorm_bwd", dict(seed_dev=False)),
    "bwd_dyn": ("mulan_groupnorm_bwd_dyn", {}),
    "bwd_fused": ("mulan_groupnorm_bwd_fused", {}),
    "bwd_fused_planes": ("mulan_groupnorm_bwd_fused_planes", dict(planes=True)),
    "bwd_stream": ("mulan_groupnorm_bwd_stream", {}),
    "bwd_stream[planes]": ("mulan_groupnorm_bwd_stream", dict(planes=True)),
}
# One row per argument set: what it changes on the valid call (B = 1, 64 channels, 16 groups, keep 0.9; "case": fields of
# the case, "fwd" / "bwd": keywords of run_fwd / run_bwd) and, per entry point in the order of ENTRIES, A = accepted
# (returns 0 and writes), R = refused (hipErrorInvalidValue, every output still poison), - = the entry point has no such
# argument.  Read off the entry points' conditions in groupnorm.hip as they stood before they shared gn_shape_ok:
#   every one:  hw == 1024, B > 0, G > 0, G | Ct, cpg in {4, 8, 16, 32}, 32 | C1, 32 | C2
#   keep:       _fwd / _fwd_dyn / _bwd / _bwd_dyn / _bwd_fused take any; _fwd_planes, _fwd_stream, _bwd_fused_planes and
#               _bwd_stream keep > 0; _fwd_planes_keepbits 0 < keep < 1; _fwd_stream with keepbits keep < 1
#   pointers:   ymax / bound required by _fwd_planes, _fwd_planes_keepbits, _stats and _fwd_stream with planes, the
#               maxima and dymax by _bwd_fused_planes and _bwd_stream with planes, tickets by the fused and the
#               streaming backward; the maxima are optional everywhere else
REFUSALS = {
    #                                                                                  forward  backward
    "valid":        (dict(),                                                           "AAAAAAA" "AAAAAA"),
    "hw=512":       (dict(fwd=dict(hw=512), bwd=dict(hw=512)),                         "RRRRRRR" "RRRRRR"),
    "G=5":          (dict(case=dict(G=5)),                                             "RRRRRRR" "RRRRRR"),   # 5 does not divide 64
    "cpg=2":        (dict(case=dict(G=32)),                                            "RRRRRRR" "RRRRRR"),
    "C1=48":        (dict(case=dict(C1=48, C2=48, Ct=96, G=12)),                       "RRRRRRR" "RRRRRR"),   # (whole groups: 96 / 12, and 48 / 12 alone)
    "keep=0":       (dict(case=dict(keep=0.0)),                                        "AARR-RR" "AAARRR"),
    "keep=1":       (dict(case=dict(keep=1.0)),                                        "AAAR-AR" "AAAAAA"),
    "no maxima":    (dict(fwd=dict(ymax=False), bwd=dict(maxima=False)),               "AARRRAR" "AAARAR"),
    "no tickets":   (dict(bwd=dict(null=("tick",))),                                   "-------" "--RRRR"),
    "no dymax":     (dict(bwd=dict(null=("dymax",))),                                  "-------" "---R-R"),
}
REFUSAL_CELLS = [pytest.param(label, row, want[i], id=f"{label}-{row}")
                 for row, (_, want) in REFUSALS.items() for i, label in enumerate(ENTRIES) if want[i] != "-"]


@pytest.mark.parametrize("label,row,want", REFUSAL_CELLS)
def test_refusals_are_per_entry_point(ops, label, row, want):
    """H: the argument checks, entry point by entry point (REFUSALS above).  The shape conditions are common to the family;
    the keep ranges, the required pointers and the caps are each entry point's own: keep = 1 is accepted by _fwd_planes and
    refused by _fwd_planes_keepbits, keep = 0 is accepted by _bwd_fused and refused by _bwd_fused_planes, a missing maxima
    array is accepted by _fwd_dyn and refused by _stats.  A refused call leaves every output at its poison value (and the
    tickets at zero).  (More than 16 slabs: test_forward_grid / test_backward_grid.)
    An accepted row is held to return code 0 and to a main output that is no longer poison, not to its values (those are
    the other tests'): with keep = 0 the accepting kernels scale by 1 / keep and mask everything out."""
    name, kw = ENTRIES[label]
    change = REFUSALS[row][0]
    # a shallow copy of the cached case with the row's fields overwritten: its tensors and derived fields (x1, mean32, ...)
    # keep the valid shape.  The rows that change a shape (G, C1 / C2 / Ct) are refused everywhere, before any launch, so
    # nothing reads them; the rows that launch change only keep, which no buffer size depends on
    c = copy.copy(case(1, 64, 0, 16, 1, 0.9))
    for k, v in change.get("case", {}).items():
        setattr(c, k, v)
    fwd = "fwd" in name or name.endswith("stats")
    o = (run_fwd if fwd else run_bwd)(ops, c, name, **{**kw, **change.get("fwd" if fwd else "bwd", {})})
    outs = ("y", "planes", "ymax", "kb") + (() if kw.get("given") else ("mean", "rstd")) if fwd else \
        ("dx1", "dx2", "planes", "dgp", "dbp", "dxsp", "mx1", "mx2", "dg", "db", "dxs", "dxs2")
    poison = {torch.float32: POISON_F, torch.int32: POISON_I, torch.uint8: 0xA5}
    untouched = {k: bool((o[k] == poison[o[k].dtype]).all()) for k in outs if o[k] is not None}
    if want == "R":
        assert o["rc"] == INVALID, (label, row, o["rc"])
        assert all(untouched.values()), (label, row, untouched)
        assert o.get("tick") is None or int(o["tick"].abs().sum()) == 0
    else:
        assert o["rc"] == 0, (label, row, o["rc"])
        main = "mean" if name.endswith("stats") else ("planes" if kw.get("planes") else ("y" if fwd else "dx1"))
        assert not untouched[main], (label, row, untouched)


# ------------------------------------------------------------------------------------------------ autograd wiring
def test_autograd_wiring_of_group_norm_and_skip(ops):
    """ops.group_norm / ops.group_norm_skip on an uneven concat at cpg 32: the output and all four gradients per (image,
    group) / per element against the same float64 reference; the skip aliases carry add1 / add2 into the kernel"""
    c = case(2, 96, 32, 4, 1, 0.9)
    kw = dict(groups=4, eps=EPS, act=True, keep=0.9, seed=SEED, offset=OFFSET)
    for skip in (False, True):
        x1, x2, gamma, beta = (t.clone().requires_grad_() for t in (c.x1, c.x2, c.gamma, c.beta))
        if skip:
            out, s1, s2 = ops.group_norm_skip(x1, x2, gamma, beta, **kw)
            ((out * c.dy).sum() + (s1 * c.add1).sum() + (s2 * c.add2).sum()).backward()
        else:
            out = ops.group_norm(x1, x2, gamma, beta, **kw)
            out.backward(c.dy)
        tag = "group_norm_skip" if skip else "group_norm"
        check_groups(tag + " y", out.detach(), c.y, c.G)
        assert torch.equal(out.detach() != 0, c.mask & (c.y != 0))
        check_groups(tag + " dx", torch.cat((x1.grad, x2.grad), -1), c.dx_total(skip, skip), c.G)
        check_each(tag + " dgamma", gamma.grad, c.dgamma)
        check_each(tag + " dbeta", beta.grad, c.dbeta)


@pytest.mark.parametrize("sinks", ["fresh", "unaligned"])
def test_autograd_wiring_off_the_in_kernel_reduction_grid(ops, monkeypatch, sinks):
    """ops.group_norm_skip over 17 slabs of 32 channels (512 + 32, the narrowest concat the family's shape check takes
    that has more slabs than the in-kernel reductions have slots): the backward is mulan_groupnorm_bwd_dyn with the sums
    over the samples in launches of their own -- mulan_colsum_pair into fresh gradients, two mulan_colsum where the
    registered sinks are not 16-byte aligned.  Output and all four gradients against the float64 reference at the bars of
    test_autograd_wiring_of_group_norm_and_skip, the skip-path gradients added in the kernel."""
    c = case(2, 512, 32, 17, 1, 0.9)
    names = []
    real = ops.call
    monkeypatch.setattr(ops, "call", lambda n, *a: (names.append(n), real(n, *a))[1])
    x1, x2, gamma, beta = (t.clone().requires_grad_() for t in (c.x1, c.x2, c.gamma, c.beta))
    if sinks == "unaligned":        # views of a gradient buffer one float past a 16-byte boundary, as TrainState registers them
        gamma._gview, beta._gview = (torch.zeros(c.Ct + 4, device="cuda")[1:1 + c.Ct] for _ in range(2))
        assert gamma._gview.data_ptr() % 16 == 4
    out, s1, s2 = ops.group_norm_skip(x1, x2, gamma, beta, groups=c.G, eps=EPS, act=True, keep=0.9, seed=SEED, offset=OFFSET)
    ((out * c.dy).sum() + (s1 * c.add1).sum() + (s2 * c.add2).sum()).backward()
    bwd = [n for n in names if n.startswith(("mulan_groupnorm_bwd", "mulan_colsum"))]
    assert bwd == ["mulan_groupnorm_bwd_dyn"] + (["mulan_colsum_pair"] if sinks == "fresh" else ["mulan_colsum"] * 2), bwd
    check_groups("off-grid y", out.detach(), c.y, c.G)
    assert torch.equal(out.detach() != 0, c.mask & (c.y != 0))
    check_groups("off-grid dx", torch.cat((x1.grad, x2.grad), -1), c.dx_total(True, True), c.G)
    check_each("off-grid dgamma", gamma.grad, c.dgamma)
    check_each("off-grid dbeta", beta.grad, c.dbeta)
    if sinks == "unaligned":        # written where the parameters' gradients live, adopted without a copy
        assert gamma.grad.data_ptr() == gamma._gview.data_ptr() and beta.grad.data_ptr() == beta._gview.data_ptr()
