"""torch.autograd wiring over the C ABI (include/mulan_hip.h).

Each Function's forward and backward are launches of hand-written HIP kernels through
`mulan_amd.lib`; torch supplies device buffers, the current stream and the autograd tape only.
Shapes: images are [B, 1024, C] (NHWC with H = W = 32 flattened), matrices row-major, all fp32.
By-products that one node leaves on a tensor for the next (maxima, statistics, channel sums, planes ...) go through
_leave / _left / _carry below; DESIGN.md section 2 ("By-products travel with the tensor") lists the tags.
"""
import math
import weakref
from typing import NamedTuple, Optional

import torch
from torch.autograd.function import once_differentiable

from . import lib
from .lib import call, ptr, stream

H = W = 32
HW = H * W
D = HW * 3
KERNEL_TIMER = None   # bench.py sets this to a list to time the dominant kernel with HIP events
# "f32": exact-fp32 MFMA (v_mfma_f32_32x32x2_f32).  "f16x3": 3-pass fp16 split (two scaled fp16 pieces per fp32 operand)
# with fp32-equivalent products, for the eligible convolutions and dense layers.  MULAN_CONV_MODE overrides; any other
# value would otherwise fall through every `CONV_MODE == "f16x3"` test into the fp32 kernels, so it is refused here.
import os as _os
CONV_MODES = ("f16x3", "f32")
CONV_MODE = _os.environ.get("MULAN_CONV_MODE", "f16x3")
if CONV_MODE not in CONV_MODES:
    raise ValueError(f"MULAN_CONV_MODE must be one of {', '.join(CONV_MODES)}; got {CONV_MODE!r}")


def _flag(name, default):
    """the import-time value of an on/off switch: the environment variable MULAN_<name> ("1" = on), else `default`.  The
    switch itself is the module attribute the result is assigned to, read wherever it is used."""
    return _os.environ.get("MULAN_" + name, default) == "1"


def _c(t):
    return t if (t is None or t.is_contiguous()) else t.contiguous()


def _chk(t, name="tensor"):
    if t.dtype != torch.float32 or not t.is_cuda:
        raise lib.MulanHipError(f"{name}: expected a float32 CUDA(HIP) tensor, got {t.dtype} on {t.device}")


# ----------------------------------------------------------------------------- raw launches
def _timed(name, flops, launch):
    """runs launch(); under bench.py's KERNEL_TIMER brackets it with HIP events on the launch stream"""
    if KERNEL_TIMER is None:
        launch()
        return
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    launch()
    e.record()
    KERNEL_TIMER.append((name, s, e, flops))


MAX_PARTS = 16

# ----------------------------------------------------------------------------- weight-gradient side stream
# Nothing in the backward pass waits for a weight gradient (only the all-reduce of its bucket and the optimizer do), while
# the input-gradient chain is strictly serial.  The weight-gradient kernels therefore go to a second HIP stream and
# run beside the GroupNorm backward / input-gradient convolution of the layers in front (see SIDE_WGRAD_SHARE for the
# split of the chip between the two streams), instead of taking their own slot in one queue.  Only gradients with
# a sink in the flat gradient buffer take this path (nothing on the main stream reads them before side_join()).
# Scope: `with weight_gradient_stream(): loss.backward()` (the train step does this); outside such a block everything
# stays on the current stream.
SIDE_STREAM = _flag("SIDE_STREAM", "1")
# side launches whose operands are kept alive before the main stream waits for the oldest (2: +1.0 ms, 16: +0.2 ms per step)
SIDE_DEPTH = int(_os.environ.get("MULAN_SIDE_DEPTH", "6"))
# While the weight-gradient launches share the chip with the input-gradient chain they aim for 120 blocks instead of
# 240 (the `share_chip` argument of the plane-fed weight-gradient entry points, see wgrad_splits_w8; no library-global
# state is involved): a weight-gradient block owns its CU, so 240 of them leave 16 CUs to the
# main stream; with 120 the launch takes about as long as the main stream's kernels of the same layer (GroupNorm
# backward + input-gradient convolution) and both streams keep running side by side: -2.9 % per step (scan 96 ... 240,
# profiles/DESIGN_r04.md 3.2).  MULAN_SIDE_WGRAD_SHARE=0 keeps 240.
SIDE_WGRAD_SHARE = _flag("SIDE_WGRAD_SHARE", "1")
_SIDE = {"stream": None, "pending": None, "active": False, "scope": False}


class weight_gradient_stream:
    """context manager around a backward pass: weight gradients with a sink run on the side stream; on exit the current
    stream waits for all of them"""

    def __enter__(self):
        _SIDE["active"] = SIDE_STREAM
        _SIDE["scope"] = True
        return self

    def __exit__(self, *exc):
        _SIDE["active"] = False
        _SIDE["scope"] = False
        side_join()
        return False


def _alone():
    """the `alone` argument of the convolution entry points: 1 unless the launch is part of the backward pass of a train
    step (a weight_gradient_stream() scope, with or without MULAN_SIDE_STREAM, so that both modes sum in the same order):
    forward passes, evaluators and the ODE likelihood's vector-Jacobian products have the chip to themselves, and small
    launches may then run as k-split blocks (conv3x3_f16x3_v3.hip)"""
    return 0 if _SIDE["scope"] else 1


def _share_chip():
    """the share_chip argument of the plane-fed weight-gradient launches: 1 inside a weight_gradient_stream() scope"""
    return int(bool(_SIDE["active"] and SIDE_WGRAD_SHARE))


def side_stream():
    """the weight-gradient stream (None until the first launch went there)"""
    return _SIDE["stream"]


def _on_side(launch, keep):
    """launch() on the side stream, ordered after everything issued so far on the current stream.  `keep`: the tensors
    the launch reads -- referenced until the current stream has waited for the launch, so that the caching allocator
    (stream-ordered on the current stream) cannot hand their memory out underneath it."""
    import collections
    main = torch.cuda.current_stream()
    if _SIDE["stream"] is None:
        _SIDE["stream"], _SIDE["pending"] = torch.cuda.Stream(), collections.deque()
    side, pending = _SIDE["stream"], _SIDE["pending"]
    ev = torch.cuda.Event()
    ev.record(main)
    side.wait_event(ev)
    with torch.cuda.stream(side):
        launch()
        done = torch.cuda.Event()
        done.record(side)
    pending.append((done, keep))
    while len(pending) > SIDE_DEPTH:
        main.wait_event(pending.popleft()[0])


def side_join():
    """the current stream waits for every weight gradient issued so far (before the optimizer / a gradient read)"""
    pending = _SIDE["pending"]
    if pending:
        main = torch.cuda.current_stream()
        while pending:
            main.wait_event(pending.popleft()[0])


def _side_ok(sink):
    return _SIDE["active"] and sink is not None and sink.is_cuda


def _wgrad_to_sink(sink, launch, keep, ok=True):
    """a weight gradient written where its parameter's gradient lives: launch(out=a fresh view of `sink`, the parameter's
    view of the flat gradient buffer; None without one: the launch then allocates) -- on the side stream when the scope
    is active, the sink exists and `ok` (the caller's own condition) holds, in line otherwise.  `keep`: the tensors the
    launch reads (_on_side).  Returns the very object it passed as `out` (or what launch allocated): autograd's
    AccumulateGrad adopts a gradient without a copy only while nothing else refers to it."""
    if ok and _side_ok(sink):
        dw = _fresh(sink)
        _on_side(lambda: launch(out=dw), keep)
        return dw
    return launch(out=_fresh(sink) if sink is not None else None)


def _maxima_slots(B, blocks, dev, want=True):
    """the optional [B, MAX_PARTS] maxima by-product of a launch with `blocks` blocks per image (one slot each): None
    where the slots do not suffice, or where the caller does not `want` it"""
    return torch.empty((B, MAX_PARTS), device=dev, dtype=torch.int32) if want and blocks <= MAX_PARTS else None


def _leave_maxima(t, maxima):
    """the counterpart of _maxima_slots: leaves the array the launch filled, if there was one, on its output; returns t"""
    return t if maxima is None else _leave(t, "_absmax", maxima)


def absmax_rows(x):
    """[B,16] int32: fp32 bit patterns of 16 partial maxima of |x[b]| (the per-image maximum is the max of a row);
    they feed the per-image operand scales of the f16x3 kernels"""
    B = x.shape[0]
    out = torch.empty((B, MAX_PARTS), device=x.device, dtype=torch.int32)
    call("mulan_absmax_rows", ptr(x), ptr(out), B, x.numel() // B, stream())
    return out


# ----------------------------------------------------------------------------- by-products carried on tensors
# What a kernel computed on the side travels to the next autograd node as a Python attribute of the tensor it describes
# (DESIGN.md section 2).  Every tag is stored as payload + (version of the tensor when it was left,): an in-place write to
# the tensor makes it stale.  Shape and compatibility checks differ per consumer and stay with the reader.
def _leave(t, tag, *payload):
    """leaves `payload` on t under the attribute `tag`, stamped with t's version; returns t.  An object that cannot take
    an attribute goes without (its consumer then takes its own pass)."""
    try:
        setattr(t, tag, payload + (t._version,))
    except (AttributeError, RuntimeError):
        pass
    return t


def _payload(t, tag):
    """the payload tuple left on t under `tag`, or None: t is None, nothing was left, or t was written to since"""
    c = getattr(t, tag, None) if t is not None else None
    return c[:-1] if (c is not None and c[-1] == t._version) else None


def _left(t, tag):
    """what _leave(t, tag, ...) left, if still valid: the bare value of a single payload, the tuple of several, True
    for a tag without payload; else None"""
    p = _payload(t, tag)
    if p is None:
        return None
    return p[0] if len(p) == 1 else (p if p else True)


# What an alias or a view of the same numbers may keep: `_absmax` (per-image maxima do not depend on how the trailing
# dimensions are folded as long as dim 0 stays the batch) and `_gnstats` (per image, row tile and channel quad: a view
# folded otherwise fails the reader's shape check).  `_colsum` describes the numbers too, but no alias site hands a
# gradient on.  The other tags are not about the numbers but about one tensor's place in the graph -- a gradient sink
# (`_bias_sink`, `_bias_twin`, `_biasdone`, `_biasgrad`), a layout bound to the shape (`_colsum_parts`, `_planes`,
# `_grad_planes`) or a promise of the producing node (`_accepts_grad_planes`) -- and never move to another object.
_VIEW_TAGS = ("_absmax", "_gnstats")


def _carry(src, dst, tags=_VIEW_TAGS):
    """re-stamps what is still valid of `tags` on src onto dst, an alias or view of src (a new Python object, which would
    lose them); returns dst"""
    for tag in tags:
        p = _payload(src, tag)
        if p is not None and not (tag == "_absmax" and p[0].shape[0] != dst.shape[0]):
            _leave(dst, tag, *p)
    return dst


def cached_absmax(x):
    """maxima a producer kernel (GroupNormFn) or an earlier consumer left on the tensor, if still valid; else a pass
    over x, remembered on the tensor for its other consumers (a gradient that feeds a convolution and a 1x1 layer)"""
    m = _left(x, "_absmax")
    if m is not None and m.shape[0] == x.shape[0]:
        return m
    m = absmax_rows(x)
    _leave(x, "_absmax", m)
    return m


def view_keep_absmax(x, *shape):
    """x.view(shape) that keeps the maxima found on x"""
    return _carry(x, x.view(*shape), tags=("_absmax",))


TEE_COLSUM = _flag("TEE_COLSUM", "1")     # A/B switch: 0 = the bias gradient takes its own pass


class TeeFn(torch.autograd.Function):
    """(x, x) for a tensor with two consumers (a U-Net skip connection): the backward pass forms the sum of the two
    gradients itself, in one kernel that also leaves the maxima of the sum for the convolution behind it (instead of
    autograd's elementwise add followed by a separate maxima pass)"""

    @staticmethod
    def forward(ctx, x):
        return _carry(x, x.view_as(x)), _carry(x, x.view_as(x))

    @staticmethod
    @once_differentiable
    def backward(ctx, ga, gb):
        if ga is None or gb is None:
            return gb if ga is None else ga
        ga, gb = _c(ga), _c(gb)
        if CONV_MODE != "f16x3" or ga.dim() < 2 or (ga.numel() // ga.shape[0]) % 4 != 0:
            return ga + gb
        out = torch.empty_like(ga)
        m = torch.empty((ga.shape[0], MAX_PARTS), device=ga.device, dtype=torch.int32)
        N = ga.shape[-1]
        if TEE_COLSUM and ga.dim() == 3 and N % 4 == 0 and 256 % (N // 4) == 0:
            # the sum is the output gradient of the convolution that produced x: leave its column sums (16 partial vectors
            # per image) for that convolution's bias gradient, which then needs no pass of its own over the tensor
            parts = torch.empty((ga.shape[0] * MAX_PARTS, N), device=ga.device, dtype=torch.float32)
            call("mulan_add_absmax_rows_colsum", ptr(ga), ptr(gb), ptr(out), ptr(m), ptr(parts), ga.shape[0],
                 ga.numel() // ga.shape[0], N, stream())
            _leave(out, "_colsum_parts", parts)
        else:
            call("mulan_add_absmax_rows", ptr(ga), ptr(gb), ptr(out), ptr(m), ga.shape[0], ga.numel() // ga.shape[0], stream())
        return _leave(out, "_absmax", m)


# The gradient sum of a block output with two consumers inside the GroupNorm backward kernel of the first consumer
# (mulan_groupnorm_bwd_fused, add1b) instead of in a kernel of its own (TeeFn): the skip-connection gradient, which the
# backward pass produces first, waits in a box until that kernel runs.  A/B switch: 0 = TeeFn.
TEE_MAILBOX = _flag("TEE_MAILBOX", "1")


class _GradBox:
    """where the gradient that reaches a tensor through its second consumer waits for the first consumer's backward.
    The hand-over is only right if, in every backward pass, the deposit (MailFn.backward) comes before the claiming
    consumer's backward takes the box's content: `deposits` / `takes` count both, and a deposit that finds more takes
    than deposits has missed its consumer -- an error, not a silently dropped gradient."""
    __slots__ = ("grad", "claimed", "deposits", "takes", "__weakref__")

    def __init__(self):
        self.grad = None
        self.claimed = False
        self.deposits = 0
        self.takes = 0

    def take(self):
        """the claiming consumer's backward: the waiting gradient (or None), the box empty again"""
        g, self.grad = self.grad, None
        self.takes += 1
        _PENDING_BOXES.discard(self)
        return g


_PENDING_BOXES = weakref.WeakSet()      # boxes that hold a gradient nobody has taken yet


def _check_no_gradient_left_waiting():
    """at the next forward pass: a box still holding a gradient means the last backward pass ended without the claiming
    consumer's backward (it was not on the differentiated path): that gradient never reached the tensor"""
    left = [b for b in _PENDING_BOXES if b.grad is not None]
    if left:
        _PENDING_BOXES.clear()
        for b in left:
            b.grad = None
        raise RuntimeError(
            f"{len(left)} skip-connection gradient(s) were left waiting in their tee() mailbox when the backward pass ended: "
            "the consumer that claimed the box (GnConv3x3Fn with skip=True) was not part of that backward pass, so the "
            "gradient of the tee()'d tensor is incomplete.  Differentiate through both consumers, or set MULAN_TEE_MAILBOX=0.")


class MailFn(torch.autograd.Function):
    """alias of x for its second consumer (tee_take): the gradient goes into the box instead of to x"""

    @staticmethod
    def forward(ctx, x, box):
        ctx.box = box
        return _carry(x, x.view_as(x))

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        if g is not None:
            box = ctx.box
            if box.takes > box.deposits:
                raise RuntimeError(
                    "tee() mailbox: the skip-connection gradient arrived AFTER the backward of the consumer that adds it "
                    "in-kernel (GnConv3x3Fn with skip=True) had run, so it would be dropped.  The mailbox needs the second "
                    "consumer's gradient first (true for the shipped U-Nets: the up path is differentiated before the "
                    "down path); set MULAN_TEE_MAILBOX=0 for graphs with another order.")
            box.deposits += 1
            box.grad = _c(g) if box.grad is None else box.grad + g       # (a second arrival: not in the U-Nets)
            _PENDING_BOXES.add(box)
        return None, None


def tee(x):
    """x for its two consumers (a block output that also feeds a U-Net skip connection): (a, b).  With TEE_MAILBOX both
    are x itself, carrying a box: if the first consumer claims it (GnConv3x3Fn with skip=True: the next ResnetBlock),
    tee_take(b) -- called where the second alias is consumed -- diverts b's gradient into the box and the first
    consumer's GroupNorm backward adds it in-kernel.  Unclaimed (another kind of first consumer): autograd sums the two
    gradients itself.  Without TEE_MAILBOX: two aliases whose gradients TeeFn.backward adds (mulan_add_absmax_rows)."""
    if not (torch.is_grad_enabled() and x.requires_grad):
        return x, x
    if TEE_MAILBOX:
        _check_no_gradient_left_waiting()
        x._grad_box = _GradBox()
        return x, x
    return TeeFn.apply(x)


def tee_take(b):
    """the second alias of tee(x), at the place where it is consumed (after the first consumer's forward)"""
    box = getattr(b, "_grad_box", None)
    if box is None or not box.claimed or not (torch.is_grad_enabled() and b.requires_grad):
        return b
    return MailFn.apply(b, box)


class ParamPacker:
    """Once-per-step weight preparation (f16x3 mode): maxima and both packed operands of every eligible parameter
    leaf of a TrainState in two launches; the leaves carry views of the result (`_prepacked`), valid until the
    optimizer touches the parameters again (`invalidate`)."""

    def __init__(self, flat, leaves_with_offsets):
        """leaves_with_offsets: [(leaf tensor (view of flat), element offset)]"""
        recs, self.items, off = [], [], 0
        for leaf, eoff in leaves_with_offsets:
            if leaf.dim() == 4 and tuple(leaf.shape[:2]) == (3, 3):
                kind, C, N = 0, leaf.shape[2], leaf.shape[3]
                fwd_ok, bwd_ok = C % 16 == 0 and N % 128 == 0, N % 16 == 0 and C % 128 == 0
            elif leaf.dim() == 2 and leaf.shape[0] % 128 == 0 and leaf.shape[1] % 128 == 0 and leaf.numel() <= 512 * 512:
                kind, C, N = 1, leaf.shape[0], leaf.shape[1]
                fwd_ok = bwd_ok = True
            else:
                continue
            if not (fwd_ok or bwd_ok):
                continue
            nb = leaf.numel() * 4
            d0 = off if fwd_ok else -1
            off += nb if fwd_ok else 0
            d1 = off if bwd_ok else -1
            off += nb if bwd_ok else 0
            recs.append([eoff, kind, C, N, d0, d1, leaf.numel(), 0])
            self.items.append((leaf, d0, d1, nb))
        self.n = len(recs)
        self.flat = flat
        self.valid = False
        if self.n:
            self.table = torch.tensor(recs, dtype=torch.int64, device=flat.device)
            self.maxima = torch.empty((self.n, MAX_PARTS), dtype=torch.int32, device=flat.device)
            self.packed = torch.empty(off, dtype=torch.uint8, device=flat.device)
            for i, (leaf, d0, d1, nb) in enumerate(self.items):
                leaf._prepacked = (self, self.packed[d0:d0 + nb] if d0 >= 0 else None,
                                   self.packed[d1:d1 + nb] if d1 >= 0 else None, self.maxima[i:i + 1])

    def refresh(self):
        if self.n:
            call("mulan_param_maxima", ptr(self.flat), ptr(self.table), self.n, ptr(self.maxima), stream())
            call("mulan_param_pack_f16x3", ptr(self.flat), ptr(self.table), self.n, ptr(self.maxima), ptr(self.packed),
                 stream())
            self.valid = True

    def invalidate(self):
        self.valid = False


def _prepacked(w, direction):
    """(wp, wmax) prepared by a ParamPacker for this leaf, if still valid"""
    pre = getattr(w, "_prepacked", None)
    if pre is not None and pre[0].valid and CONV_MODE == "f16x3" and pre[1 + direction] is not None:
        return pre[1 + direction], pre[3]
    return None


def _pack_weights(w, C, N, flip, wmax=None):
    """weights pre-split into the LDS tile layout of the f16x3 convolution kernels; returns (wp, wmax)"""
    L = lib.load()
    pre = _prepacked(w, int(flip))
    if pre is not None:
        return pre
    wp = torch.empty(L.mulan_conv3x3_pack_f16x3_bytes(C, N), device=w.device, dtype=torch.uint8)
    if wmax is None:
        wmax = absmax_rows(w.view(1, -1))
    call("mulan_conv3x3_pack_f16x3", ptr(w), ptr(wp), ptr(wmax), C, N, flip, stream())
    return wp, wmax


def planes_eligible(C, N):
    """the plane-fed weight-gradient kernel (f16x3 mode) covers 128-multiples of channels"""
    return CONV_MODE == "f16x3" and C % 128 == 0 and N % 128 == 0


def _cbias_mode(cbias):
    """the cbias mode of the convolution entry points: 0 none, 1 per sample [B,N], 2 per pixel [B,1024,N]"""
    return 0 if cbias is None else (1 if cbias.dim() == 2 else 2)


def _has(bias, cbias, res):
    """which of a convolution's optional addends exist, as its backward reads it: (bias?, cbias.dim() or None, res?)"""
    return bias is not None, None if cbias is None else cbias.dim(), res is not None


def conv3x3_raw(x, w, bias=None, cbias=None, res=None, xmax=None, planes=False, wmax=None):
    """x [B,1024,C], w [3,3,C,N] -> [B,1024,N]   (xmax: absmax_rows(x) if the caller already has it, f16x3 mode).
    planes=True (f16x3 mode): returns (y, xs) with xs the split fp16 planes of x for conv3x3_wgrad_planes_raw."""
    _chk(x, "conv input")
    B, C, N = x.shape[0], x.shape[-1], w.shape[-1]
    assert w.shape[:3] == (3, 3, C), (w.shape, C)
    y = torch.empty((B, HW, N), device=x.device, dtype=torch.float32)
    mode = _cbias_mode(cbias)
    fast = CONV_MODE == "f16x3" and C % 16 == 0 and N % 128 == 0
    flops = 2.0 * B * HW * 9 * C * N
    if not fast:
        variant = "<128,2,2>" if N > 64 else ("<64,2,2>" if N > 32 else "<32,4,1>")
        _timed("conv3x3_fwd_kernel" + variant, flops,
               lambda: call("mulan_conv3x3_fwd", ptr(x), ptr(w), ptr(bias), ptr(cbias), mode, ptr(res), ptr(y), B, H, W,
                            C, N, stream()))
        return y
    assert fast or not planes
    wp, wmax = _pack_weights(w, C, N, 0, wmax)
    if xmax is None:
        xmax = absmax_rows(x)
    xs = torch.empty(B * HW * C * 4, device=x.device, dtype=torch.uint8) if planes else None
    # by-product: the maxima of y, left on the tensor for whichever f16x3 kernel reads it next
    ymax = _maxima_slots(B, (H // 8) * (N // 128), x.device)
    _timed("conv3x3_f16x3_kernel", flops,
           lambda: call("mulan_conv3x3_fwd_f16x3_alone", ptr(x), ptr(xmax), ptr(wp), ptr(wmax), ptr(bias), ptr(cbias), mode,
                        ptr(res), ptr(y), ptr(xs), ptr(ymax), _alone(), B, H, W, C, N, stream()))
    _leave_maxima(y, ymax)
    return (y, xs) if planes else y


def conv3x3_dgrad_raw(dy, w, dymax=None, planes=False, wmax=None, want_max=False):
    """dx = conv3x3(dy, flipped w).  planes=True (f16x3 mode): returns (dx, dys), dys = the split planes of dy.
    want_max (f16x3 mode): the kernel leaves the maxima of dx on the tensor (a GroupNorm backward that hands its own
    result on as planes needs them for its bound)."""
    C, N = w.shape[2], w.shape[3]
    if CONV_MODE == "f16x3" and N % 16 == 0 and C % 128 == 0:
        B = dy.shape[0]
        dx = torch.empty((B, HW, C), device=dy.device, dtype=torch.float32)
        wp, wmax = _pack_weights(w, C, N, 1, wmax)
        flops = 2.0 * B * HW * 9 * C * N
        if dymax is None:
            dymax = absmax_rows(dy)
        dys = torch.empty(B * HW * N * 4, device=dy.device, dtype=torch.uint8) if planes else None
        dxmax = _maxima_slots(B, (H // 8) * (C // 128), dy.device, want_max)
        _timed("conv3x3_f16x3_kernel", flops,
               lambda: call("mulan_conv3x3_fwd_f16x3_alone", ptr(dy), ptr(dymax), ptr(wp), ptr(wmax), None, None, 0, None,
                            ptr(dx), ptr(dys), ptr(dxmax), _alone(), B, H, W, N, C, stream()))
        _leave_maxima(dx, dxmax)
        return (dx, dys) if planes else dx
    wT = torch.empty((3, 3, N, C), device=w.device, dtype=torch.float32)
    call("mulan_conv3x3_wflip", ptr(w), ptr(wT), C, N, stream())
    return conv3x3_raw(dy, wT)


def conv3x3_dgrad_planes_raw(dys, dymax, w, wmax=None, want_max=False):
    """dx = conv3x3(dy, flipped w) with dy given as split planes (scaled with dymax: what a GroupNorm backward hands on,
    mulan_groupnorm_bwd_fused_planes): the plane-fed instantiation of the convolution kernel -- no split, no plane stores"""
    C, N = w.shape[2], w.shape[3]
    B = dymax.shape[0]
    dx = torch.empty((B, HW, C), device=dys.device, dtype=torch.float32)
    wp, wmax = _pack_weights(w, C, N, 1, wmax)
    dxmax = _maxima_slots(B, (H // 8) * (C // 128), dys.device, want_max)
    # alone: no weight-gradient stream beside this launch (the ODE evaluator's vector-Jacobian product, not the backward
    # pass of a train step -- with or without MULAN_SIDE_STREAM, so that both modes sum in the same order): small launches
    # may then run as k-split blocks (conv3x3_f16x3_v3.hip)
    alone = _alone()
    _timed("conv3x3_f16x3_kernel<planes_in,dgrad>", 2.0 * B * HW * 9 * C * N,
           lambda: call("mulan_conv3x3_fwd_f16x3_planes_in_stats", ptr(dys), ptr(dymax), ptr(wp), ptr(wmax), None, None, 0,
                        None, ptr(dx), ptr(dxmax), None, alone, B, H, W, N, C, stream()))
    return _leave_maxima(dx, dxmax)


def grad_planes_eligible(C, N):
    """a convolution C -> N whose output gradient may arrive as split planes only: plane-fed weight gradient (128-grids)
    and the two-blocks-per-CU kernel for the input gradient (N % 32 == 0, C % 128 == 0)"""
    return GRAD_PLANES and planes_eligible(C, N) and N % 32 == 0 and C % 128 == 0 and N // 32 <= MAX_PARTS


_NAN = {}


def _planes_only_grad(shape, device, planes, bound):
    """The stand-in autograd carries for a gradient that exists only as split planes: a NaN scalar expanded to the
    gradient's shape (4 bytes; anything that consumed it as numbers would turn NaN at once -- loud, not silent) with the
    real content left on it as `_grad_planes` (planes, bound maxima)"""
    n = _NAN.get(device)
    if n is None:
        n = _NAN[device] = torch.full((1,), float("nan"), device=device, dtype=torch.float32)
    return _leave(n.expand(*shape), "_grad_planes", planes, bound)


def _gv(t):
    """flat-gradient-buffer view registered for a parameter leaf by TrainState (None for ordinary tensors)"""
    return getattr(t, "_gview", None) if t is not None else None


def _fresh(view):
    """a new tensor object over the same storage: lets autograd's AccumulateGrad adopt it without a copy"""
    return view.view(view.shape)


def _wgrad_launch(name, fn, operands, B, C, N, taps, out, dev, share=None, dims=None):
    """what the slab weight-gradient launches share: the workspace that `fn`_workspace asks for, dw (`out`, or a fresh
    [3,3,C,N] for taps = 9, [C,N] for taps = 1) and the timed call fn(*operands, dw, workspace, *dims, accumulate = 0
    [, share]); dims = (B, H, W, C, N) unless the entry point takes another list.  Returns dw."""
    tail = () if share is None else (share,)
    nbytes = getattr(lib.load(), fn + "_workspace")(B, H, W, C, N, *tail)
    ws = torch.empty(nbytes // 4, device=dev, dtype=torch.float32)
    dw = out if out is not None else torch.empty((3, 3, C, N) if taps == 9 else (C, N), device=dev, dtype=torch.float32)
    dims = (B, H, W, C, N) if dims is None else dims
    _timed(name, 2.0 * B * HW * taps * C * N, lambda: call(fn, *operands, ptr(dw), ptr(ws), *dims, 0, *tail, stream()))
    return dw


def conv3x3_wgrad_raw(x, dy, out=None, xmax=None, dymax=None):
    B, C, N = x.shape[0], x.shape[-1], dy.shape[-1]
    infix, operands = "", (ptr(x), ptr(dy))
    if CONV_MODE == "f16x3" and C % 4 == 0 and N % 4 == 0:
        xmax = absmax_rows(x) if xmax is None else xmax
        dymax = absmax_rows(dy) if dymax is None else dymax
        infix, operands = "_f16x3", (ptr(x), ptr(xmax), ptr(dy), ptr(dymax))
    return _wgrad_launch("conv3x3_wgrad" + infix + "_kernel+slab_reduce", "mulan_conv3x3_wgrad" + infix, operands, B, C, N, 9,
                         out, x.device)


def conv3x3_wgrad_planes_raw(xs, xmax, dys, dymax, B, C, N, out=None):
    """dw from the split planes of x (written by the forward conv) and of dy (written by the input-gradient conv)"""
    return _wgrad_launch("conv3x3_wgrad_f16x3_planes_kernel+slab_reduce", "mulan_conv3x3_wgrad_f16x3_planes",
                         (ptr(xs), ptr(xmax), ptr(dys), ptr(dymax)), B, C, N, 9, out, xs.device, _share_chip())


def gemm_raw(A, Bm, M, N, K, *, bias=None, R=None, transA=False, transB=False, alpha=1.0, beta=1.0,
             lda=None, ldb=None, batch=1, sA=0, sB=0, out=None):
    """C = alpha * op(A) op(B) + bias + beta * R.  Returns [batch, M, N] (or [M, N] when batch == 1)."""
    lda = lda if lda is not None else (M if transA else K)
    ldb = ldb if ldb is not None else (K if transB else N)
    if out is None:
        out = torch.empty((batch, M, N) if batch > 1 else (M, N), device=A.device, dtype=torch.float32)
    ws = None
    if batch == 1 and K >= 256:
        nbytes = lib.load().mulan_gemm_workspace(M, N, K, batch)
        if nbytes:
            ws = torch.empty(nbytes // 4, device=A.device, dtype=torch.float32)
    call("mulan_gemm", ptr(A), ptr(Bm), ptr(out), ptr(bias), ptr(R), M, N, K, lda, ldb, N, N, int(transA),
         int(transB), batch, sA, sB, M * N, M * N, float(alpha), float(beta), ptr(ws), stream())
    return out


def colsum_raw(x2d, nseg, seg, C, out=None, ld=None):
    """out[s][c] = sum of `seg` consecutive rows (row stride ld, default C); long segments are reduced in two stages so
    the grid always has enough blocks to stream from HBM (fixed order => deterministic)."""
    chunk = 512
    ld = C if ld is None else ld
    src = ptr(x2d) if ld == C else x2d.data_ptr()       # rows of a wider matrix: the stride goes to the kernel
    if seg >= 4 * chunk and seg % chunk == 0:
        part = torch.empty((nseg * (seg // chunk), C), device=x2d.device, dtype=torch.float32)
        call("mulan_colsum", src, ptr(part), nseg * (seg // chunk), chunk, C, ld, 0, stream())
        src, seg, ld = ptr(part), seg // chunk, C
    if out is None:
        out = torch.empty((nseg, C), device=x2d.device, dtype=torch.float32)
    call("mulan_colsum", src, ptr(out), nseg, seg, C, ld, 0, stream())
    return out


def randn(shape, seed, offset, device, out=None):
    if out is None:
        out = torch.empty(shape, device=device, dtype=torch.float32)
    call("mulan_randn", ptr(out), out.numel(), int(seed) & (2**64 - 1), int(offset), stream())
    return out


# ----------------------------------------------------------------------------- conv
class _ConvBwd(NamedTuple):
    """what _conv3x3_backward reads.  Conv3x3Fn and GnConv3x3Fn build it in forward, where every field is known; the
    tensors that go through save_for_backward (`saved`, and GnConv3x3Fn's `xmax`) are emptied out of the copy kept on the
    context and put back at the top of backward."""
    saved: tuple                   # (x, or its split planes where `planes`, w)
    planes: bool                   # saved[0] is the plane tensor: plane-fed weight gradient, dy's planes handed on
    xmax: Optional[torch.Tensor]   # maxima (or the a-priori bound) the forward kernel scaled x with; None: fp32 kernels
    wmax: Optional[torch.Tensor]
    has: tuple                     # _has(bias, cbias, res)
    gv: tuple                      # (_gv(w), _gv(bias)): the gradient sinks
    need: tuple                    # needs_input_grad of (x, w, bias, cbias, res)
    want_dx_max: bool = False      # the kernel leaves the maxima of dx on it (for a GroupNorm backward that writes planes)


class Conv3x3Fn(torch.autograd.Function):
    """y = conv3x3(x, w) + bias + cbias + res   (ldm/model_vdm.py:633-656)"""

    @staticmethod
    def forward(ctx, x, w, bias, cbias, res):
        x, w = _c(x), _c(w)
        need = ctx.needs_input_grad
        f16 = CONV_MODE == "f16x3" and x.shape[-1] % 4 == 0        # per-image maxima: shared by fwd and wgrad
        xmax = cached_absmax(x) if f16 else None
        pre = _prepacked(w, 0)
        wmax = (pre[1] if pre is not None else absmax_rows(w.view(1, -1))) if f16 else None   # shared by both packs
        # the forward kernel hands its split input planes to the weight-gradient kernel: saved instead of x (same bytes)
        planes = bool(planes_eligible(x.shape[-1], w.shape[-1]) and need[0] and need[1])
        y = conv3x3_raw(x, w, _c(bias), _c(cbias), _c(res), xmax=xmax, planes=planes, wmax=wmax)
        if planes:
            y, x = y
        gvb = _gv(bias)
        conv = _ConvBwd(saved=(x, w), planes=planes, xmax=xmax, wmax=wmax, has=_has(bias, cbias, res), gv=(_gv(w), gvb),
                        need=tuple(need[:5]))
        ctx.save_for_backward(*conv.saved)
        ctx.conv = conv._replace(saved=())
        if gvb is not None and need[2]:
            _leave_bias_sink(y, gvb, res)
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, dy):
        return _conv3x3_backward(ctx.conv._replace(saved=ctx.saved_tensors), dy)


def _leave_bias_sink(y, gvb, res):
    """A GroupNorm that consumes y writes the gradient of the bias behind y (gvb: its sink; the channel sums of the dy it
    produces) from inside its backward kernel; the twin: the bias of the shortcut layer whose output is `res` sees the
    same gradient."""
    _leave(y, "_bias_sink", gvb, _left(res, "_bias_twin"))


def _bias_sink_of(x1, C1):
    """(sink, twin sink or None) left by the convolution that produced x1 (_leave_bias_sink), or None"""
    bs = _left(x1, "_bias_sink")
    return bs if (bs is not None and bs[0].numel() == C1) else None


def _conv3x3_backward(rec, dy):
    """backward of y = conv3x3(x, w) + bias + cbias + res -> (dx, dw, dbias, dcbias, dres); rec: the _ConvBwd of
    Conv3x3Fn or GnConv3x3Fn"""
    (x, w), x_is_planes, xmax, wmax, (has_bias, cb_dim, has_res), (gvw, gvb), need, want_max = rec
    B, N = dy.shape[0], dy.shape[-1]

    def wgrad_from_planes(dys, dymax):
        return _wgrad_to_sink(gvw, lambda out: conv3x3_wgrad_planes_raw(x, xmax, dys, dymax, B, w.shape[2], N, out=out),
                              (x, xmax, dys, dymax))

    gp = _left(dy, "_grad_planes")
    if gp is not None:
        # dy exists only as split planes (written by the GroupNorm backward behind this convolution,
        # mulan_groupnorm_bwd_fused_planes): the plane-fed convolution kernel forms dx, the weight-gradient kernel
        # reads the same planes, bias / FiLM gradients come from the channel sums that kernel left.  Nothing here
        # may read dy's numbers (the tensor is a NaN stand-in).
        assert not has_res and cb_dim != 3 and _left(dy, "_colsum") is not None, "planes-only gradient misrouted"
        dys, dymax = gp
        dx = conv3x3_dgrad_planes_raw(dys, dymax, w, wmax=wmax, want_max=want_max)
        dw = wgrad_from_planes(dys, dymax) if need[1] else None
    else:
        nan = _NAN.get(dy.device)
        if nan is not None and dy.numel() > 1 and dy.data_ptr() == nan.data_ptr() and all(s == 0 for s in dy.stride()):
            # the NaN stand-in of _planes_only_grad without (valid) planes: autograd handed on another tensor object than
            # the GroupNorm backward returned (a tensor hook, retain_grad or an accumulation on conv1's output)
            raise RuntimeError("planes-only gradient arrived without its planes: hooks / retain_grad / a second consumer "
                               "on the output of a ResnetBlock's conv1 are not supported with MULAN_GRAD_PLANES=1")
        dy = _c(dy)
        dymax = cached_absmax(dy) if (CONV_MODE == "f16x3" and N % 4 == 0) else None   # shared by dgrad and wgrad
        if x_is_planes:                  # x is the plane tensor here
            dx, dys = conv3x3_dgrad_raw(dy, w, dymax=dymax, planes=True, wmax=wmax, want_max=want_max)
            _leave(dy, "_planes", dys, dymax)   # the shortcut layer that shares this dy takes its weight gradient from them
            dw = wgrad_from_planes(dys, dymax)
        else:
            dx = conv3x3_dgrad_raw(dy, w, dymax=dymax, wmax=wmax, want_max=want_max) if need[0] else None
            dw = None
            if need[1]:   # written straight into the flat gradient buffer when the weight is a leaf
                dw = _wgrad_to_sink(gvw, lambda out: conv3x3_wgrad_raw(x, dy, out=out, xmax=xmax, dymax=dymax),
                                    (x, dy, xmax, dymax), ok=dymax is None or xmax is not None)
    dbias = dcb = None
    per_sample = None
    parts = _left(dy, "_colsum_parts")                 # left by TeeFn.backward's add: 16 partial column sums per image
    if parts is not None and parts.shape[1] != N:
        parts = None
    if parts is not None and has_bias and need[2] and not (cb_dim == 2 and need[3]):
        dbias = colsum_raw(parts, 1, parts.shape[0], N, out=_fresh(gvb).view(1, N) if gvb is not None else None).view(N)
        _leave(dy, "_biasgrad", dbias.view(N), None)
    elif (has_bias and need[2]) or (cb_dim == 2 and need[3]):
        cs = _left(dy, "_colsum")                      # left by the GroupNorm backward that produced dy
        per_sample = cs if (cs is not None and cs.shape == (B, N)) else colsum_raw(dy, B, HW, N)    # [B,N]
    if dbias is None and has_bias and need[2]:
        done = _left(dy, "_biasdone")                  # the GroupNorm backward already summed it into the sink
        twin = None
        if done is not None and gvb is not None and done[0].data_ptr() == gvb.data_ptr():
            dbias, twin = _fresh(gvb), done[1]
        else:
            dbias = colsum_raw(per_sample, 1, B, N, out=_fresh(gvb).view(1, N) if gvb is not None else None,
                               ld=per_sample.stride(0)).view(N)
        # the shortcut layer that shares this dy (nin_shortcut + bias) needs the very same column sum; twin: the sink it
        # was written into as well (a separate view: autograd adopts `dbias` itself)
        _leave(dy, "_biasgrad", dbias.view(N), twin)
    if cb_dim is not None and need[3]:
        dcb = per_sample if cb_dim == 2 else dy
    dres = dy if (has_res and need[4]) else None
    assert gp is None or (dres is None and dcb is not dy)
    return dx, dw, dbias, dcb, dres


def conv3x3(x, w, bias=None, cbias=None, res=None):
    return Conv3x3Fn.apply(x, w, bias, cbias, res)


# ----------------------------------------------------------------------------- dense
def _tag_bias_twin(y, gvb, wanted):
    """A dense layer whose output becomes the residual input of a 3x3 convolution (nin_shortcut, ldm/model_vdm.py:652-656)
    has the same bias gradient as that convolution: the convolution passes this sink on (Conv3x3Fn.forward)."""
    if gvb is not None and wanted:
        _leave(y, "_bias_twin", gvb)


def _dense_bias_grad(dy, M, N, gvb):
    """sum of dy over all rows; re-used from the convolution that consumed the same dy when there is one"""
    out = _fresh(gvb) if gvb is not None else None
    c = _left(dy, "_biasgrad")              # (the column sum, the twin sink it went to as well or None)
    if c is not None and c[0].numel() == N:
        if out is None:
            return c[0].view(N)
        if not (c[1] is not None and c[1].data_ptr() == out.data_ptr()):   # else: written there already
            out.view(N).copy_(c[0].view(N))
        return out.view(N)
    return colsum_raw(dy.reshape(M, N), 1, M, N, out=out.view(1, N) if out is not None else None).view(N)


def linear_fast_ok(x, K1, K2, N1, N2):
    """per-pixel dense layers go through the f16x3 kernel (linear_f16x3.hip) when the shapes are image shaped"""
    return (CONV_MODE == "f16x3" and x.dim() == 3 and x.shape[1] == HW and K1 % 32 == 0 and K2 % 32 == 0 and
            N1 % 128 == 0 and N2 % 128 == 0)


def linear_pack(w, transpose, wmax=None):
    """w [K,N] -> packed operand of y = x @ w (transpose=False) or of dx = dy @ w^T (transpose=True)"""
    K, N = (w.shape[1], w.shape[0]) if transpose else (w.shape[0], w.shape[1])
    pre = _prepacked(w, int(transpose))
    if pre is not None:
        return pre
    if wmax is None:
        wmax = absmax_rows(w.reshape(1, -1))
    wp = torch.empty(lib.load().mulan_linear_pack_f16x3_bytes(K, N), device=w.device, dtype=torch.uint8)
    call("mulan_linear_pack_f16x3", ptr(w), ptr(wp), ptr(wmax), K, N, int(transpose), stream())
    return wp, wmax


def linear_f16x3_raw(x1, x2, wp, wmax, N1, N2, *, bias=None, res=None, planes=False):
    """[x1 | x2] @ W + bias + res -> (y1 [B,1024,N1], y2 [B,1024,N2] or None); x* are [B,1024,K*] pixel tensors.
    planes=True: also returns (xs, xmax): the split planes of [x1 | x2] and the per-image maxima they were scaled with
    (the input of linear_wgrad_planes_raw)."""
    B, K1 = x1.shape[0], x1.shape[-1]
    K2 = 0 if x2 is None else x2.shape[-1]
    M = B * HW
    y1 = torch.empty((B, HW, N1), device=x1.device, dtype=torch.float32)
    y2 = torch.empty((B, HW, N2), device=x1.device, dtype=torch.float32) if N2 else None
    m1 = cached_absmax(x1)
    m2 = cached_absmax(x2) if x2 is not None else None
    xs = torch.empty(M * (K1 + K2) * 4, device=x1.device, dtype=torch.uint8) if planes else None
    _timed("linear_f16x3_kernel", 2.0 * M * (K1 + K2) * (N1 + N2),
           lambda: call("mulan_linear_f16x3", ptr(x1), ptr(m1), ptr(x2), ptr(m2), K1, K2, ptr(wp), ptr(wmax), ptr(bias),
                        ptr(res), ptr(y1), ptr(y2), ptr(xs), N1, N2, M, HW, stream()))
    if planes:
        return y1, y2, xs, (m1 if m2 is None else torch.maximum(m1, m2))
    return y1, y2


def linear_wgrad_planes_raw(xs, xmax, dys, dymax, B, K, N, out=None):
    """dw[K,N] = [x1|x2]^T dy from the planes handed on by linear_f16x3_raw (xs) and by the convolution that consumed
    the same dy (dys)"""
    return _wgrad_launch("linear_wgrad_f16x3_planes_kernel+slab_reduce", "mulan_linear_wgrad_f16x3_planes",
                         (ptr(xs), ptr(xmax), ptr(dys), ptr(dymax)), B, K, N, 1, out, xs.device, _share_chip())


def linear_wgrad_x32_raw(x1, x2, xmax, xmax2, dys, dymax, B, N, *, out=None):
    """dw[K1 + K2, N] = [x1 | x2]^T dy with x in fp32 (split while staged: the kernel is memory bound) and dy as the
    planes handed on by the convolution that consumed the same dy; xmax / xmax2 = the maxima of x1 / x2 (the kernel
    scales the concat with their elementwise max, as the forward kernel did: no separate launch for it).  Bit-identical to
    linear_wgrad_planes_raw on the planes the forward kernel would have written -- which it then need not write."""
    K1 = x1.shape[-1]
    K2 = 0 if x2 is None else x2.shape[-1]
    return _wgrad_launch("linear_wgrad_f16x3_planes_kernel+slab_reduce", "mulan_linear_wgrad_f16x3_x32",
                         (ptr(x1), ptr(x2), K1, K2, ptr(xmax), ptr(xmax2), ptr(dys), ptr(dymax)), B, K1 + K2, N, 1, out,
                         x1.device, _share_chip(), dims=(B, H, W, N))


# the dense weight gradient reads the layer's fp32 input and splits it in its staging path (round 3) instead of taking
# planes the forward kernel wrote as a by-product; A/B switch: 0 = the round-2 plane hand-over
LINEAR_WGRAD_X32 = _flag("LINEAR_WGRAD_X32", "1")


class LinearFn(torch.autograd.Function):
    """y[M,N] = x[M,K] @ w[K,N] + bias + res   (flax nn.Dense: y = x @ kernel + bias)"""

    @staticmethod
    def forward(ctx, x, w, bias, res):
        x, w = _c(x), _c(w)
        K, N = w.shape
        x2 = x.reshape(-1, K)
        M = x2.shape[0]
        ctx.fast = linear_fast_ok(x, K, 0, N, 0) and K % 128 == 0
        ctx.wmax = None
        if ctx.fast:
            wp, ctx.wmax = linear_pack(w, False)
            y, _ = linear_f16x3_raw(x, None, wp, ctx.wmax, N, 0, bias=_c(bias), res=_c(res))
        else:
            y = gemm_raw(x2, w, M, N, K, bias=_c(bias), R=None if res is None else _c(res).reshape(M, N))
        ctx.save_for_backward(x2, w)
        ctx.meta = (x.shape, bias is not None, res is not None)
        ctx.gv = (_gv(w), _gv(bias))
        y = y.view(*x.shape[:-1], N)
        _tag_bias_twin(y, ctx.gv[1], ctx.needs_input_grad[2])
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, dy):
        x2, w = ctx.saved_tensors
        xshape, has_bias, has_res = ctx.meta
        K, N = w.shape
        M = x2.shape[0]
        dy = _c(dy)
        dy2 = dy.reshape(M, N)
        dx = dw = db = None
        if ctx.needs_input_grad[0]:
            if ctx.fast:
                wpt, _ = linear_pack(w, True, ctx.wmax)
                dx = linear_f16x3_raw(view_keep_absmax(dy, -1, HW, N), None, wpt, ctx.wmax, K, 0)[0].view(xshape)
            else:
                dx = gemm_raw(dy2, w, M, K, N, transB=True).view(xshape)
        gvw, gvb = ctx.gv
        if ctx.needs_input_grad[1]:
            dw = _wgrad_to_sink(gvw, lambda out: gemm_raw(x2, dy2, K, N, M, transA=True, out=out), (x2, dy2),
                                ok=M >= 4096)          # (the small per-sample layers stay in line: nothing to overlap)
        if has_bias and ctx.needs_input_grad[2]:
            db = _dense_bias_grad(dy, M, N, gvb)
        dres = dy if (has_res and ctx.needs_input_grad[3]) else None
        return dx, dw, db, dres


def linear(x, w, bias=None, res=None):
    return LinearFn.apply(x, w, bias, res)


class CondProjAllFn(torch.autograd.Function):
    """outs[g] = cond @ W[g] for all G FiLM projections of a U-Net at once (cond_proj of every ResnetBlock,
    ldm/model_vdm.py:639-641: they share their input): one batched GEMM forward, two backward, instead of three small
    latency-bound GEMMs per block."""

    @staticmethod
    def forward(ctx, cond, W):
        cond, W = _c(cond), _c(W)
        G, K, N = W.shape
        B = cond.shape[0]
        out = gemm_raw(cond, W, B, N, K, batch=G, sA=0, sB=K * N)            # [G,B,N]
        ctx.save_for_backward(cond, W)
        ctx.gv = _gv(W)
        return tuple(out[g] for g in range(G))

    @staticmethod
    @once_differentiable
    def backward(ctx, *douts):
        cond, W = ctx.saved_tensors
        G, K, N = W.shape
        B = cond.shape[0]
        zero = None
        parts = []
        for d in douts:
            if d is None:
                if zero is None:
                    zero = torch.zeros((B, N), device=cond.device, dtype=torch.float32)
                d = zero
            parts.append(d)
        dO = torch.stack(parts)                                              # [G,B,N]
        dcond = dW = None
        if ctx.needs_input_grad[0]:
            dcond = gemm_raw(dO, W, B, K, N, transB=True, batch=G, sA=B * N, sB=K * N).sum(0)
        if ctx.needs_input_grad[1]:
            gvw = ctx.gv
            dW = gemm_raw(cond, dO, K, N, B, transA=True, batch=G, sA=0, sB=B * N,
                          out=_fresh(gvw) if gvw is not None else None)
        return dcond, dW


class CondProjGroup:
    """The strided super-parameter [G,K,N] over G back-to-back cond_proj kernels (TrainState lays them out that way)
    and the per-forward cache of their outputs."""

    def __init__(self, weight):
        self.weight = weight
        self._cond = None
        self._key = None
        self._outs = None

    def clear(self):
        """drops the cached outputs (and with them the autograd graph they hold, including the AccumulateGrad node of
        the super-parameter, which remembers the stream it was created on)"""
        self._cond = self._key = self._outs = None

    def outputs(self, cond):
        import weakref
        key = (cond._version, torch.is_grad_enabled())
        if self._cond is None or self._cond() is not cond or self._key != key:
            self._outs = CondProjAllFn.apply(cond, self.weight)
            self._cond, self._key = weakref.ref(cond), key
        return self._outs


GROUP_COND_PROJ = _flag("GROUP_COND_PROJ", "1")


def cond_proj(cond, w):
    """cond @ w for a ResnetBlock's FiLM projection; grouped over all blocks of the U-Net when the parameters come
    from a TrainState (per-sample conditioning only; the per-pixel ldm variant is an ordinary per-pixel dense layer)"""
    grp = getattr(w, "_group", None)
    if grp is None or cond.dim() != 2 or not GROUP_COND_PROJ:
        return linear(cond, w)
    return grp[0].outputs(cond)[grp[1]]


class Linear2Fn(torch.autograd.Function):
    """y = [x1 | x2] @ w + bias over a virtual channel concat (nin_shortcut on concat[h, skip],
    ldm/model_vdm.py:369,652-653) without materialising the concat."""

    @staticmethod
    def forward(ctx, x1, x2, w, bias):
        x1, x2, w = _c(x1), _c(x2), _c(w)
        K1, K2, N = x1.shape[-1], x2.shape[-1], w.shape[1]
        a1, a2 = x1.reshape(-1, K1), x2.reshape(-1, K2)
        M = a1.shape[0]
        ctx.fast = linear_fast_ok(x1, K1, K2, N, 0) and K1 % 128 == 0 and K2 % 128 == 0
        ctx.wmax = None
        # what the weight gradient takes its x operand from: x32 = the maxima of (x1, x2), the kernel splits the fp32
        # inputs itself; xs / xsmax = the planes the forward kernel wrote and their maxima; neither: the fp32 GEMM
        ctx.x32 = ctx.xs = ctx.xsmax = None
        if ctx.fast:      # one pass over both inputs, no intermediate
            wp, ctx.wmax = linear_pack(w, False)
            want_xs = bool(ctx.needs_input_grad[2] and not LINEAR_WGRAD_X32)    # (fast: K1, K2, N are 128-multiples)
            out = linear_f16x3_raw(x1, x2, wp, ctx.wmax, N, 0, bias=_c(bias), planes=want_xs)
            y = out[0].view(M, N)
            if want_xs:
                ctx.xs, ctx.xsmax = out[2:]
            elif ctx.needs_input_grad[2]:
                ctx.x32 = (cached_absmax(x1), cached_absmax(x2))      # the maxima the forward kernel just used: [B, 16] each
        else:
            y = gemm_raw(a1, w[:K1], M, N, K1, bias=_c(bias))
            y = gemm_raw(a2, w[K1:], M, N, K2, R=y, out=torch.empty_like(y))
        ctx.save_for_backward(a1, a2, w)
        ctx.shape = x1.shape[:-1]
        ctx.gv = (_gv(w), _gv(bias))
        y = y.view(*x1.shape[:-1], N)
        _tag_bias_twin(y, ctx.gv[1], ctx.needs_input_grad[3])
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, dy):
        a1, a2, w = ctx.saved_tensors
        K1, K2, N = a1.shape[1], a2.shape[1], w.shape[1]
        M = a1.shape[0]
        dy = _c(dy)
        dy2 = dy.reshape(M, N)
        if ctx.fast and ctx.needs_input_grad[0] and ctx.needs_input_grad[1]:
            wpt, _ = linear_pack(w, True, ctx.wmax)          # dy @ w^T, split into the two inputs' gradients on the way out
            dx1, dx2 = linear_f16x3_raw(view_keep_absmax(dy, -1, HW, N), None, wpt, ctx.wmax, K1, K2)
            dx1, dx2 = dx1.view(*ctx.shape, K1), dx2.view(*ctx.shape, K2)
        else:
            dx1 = gemm_raw(dy2, w[:K1], M, K1, N, transB=True).view(*ctx.shape, K1) if ctx.needs_input_grad[0] else None
            dx2 = gemm_raw(dy2, w[K1:], M, K2, N, transB=True).view(*ctx.shape, K2) if ctx.needs_input_grad[1] else None
        dw = None
        gvw, gvb = ctx.gv
        if ctx.needs_input_grad[2]:
            pl = _left(dy, "_planes")       # (planes of dy, its maxima) left by the convolution that consumed the same dy
            x32 = ctx.x32
            if x32 is not None and pl is not None and pl[0].numel() == M * N * 4:
                B_ = M // HW
                x1v, x2v = a1.view(B_, HW, K1), a2.view(B_, HW, K2)
                dw = _wgrad_to_sink(
                    gvw, lambda out: linear_wgrad_x32_raw(x1v, x2v, x32[0], x32[1], pl[0], pl[1], B_, N, out=out),
                    (x1v, x2v, x32[0], x32[1], pl[0], pl[1]))
            elif ctx.xs is not None and pl is not None and pl[0].numel() == M * N * 4:
                xs, xsmax = ctx.xs, ctx.xsmax
                dw = _wgrad_to_sink(
                    gvw, lambda out: linear_wgrad_planes_raw(xs, xsmax, pl[0], pl[1], M // HW, K1 + K2, N, out=out),
                    (xs, xsmax, pl[0], pl[1]))
            else:
                def both(out):
                    out = torch.empty_like(w) if out is None else out
                    gemm_raw(a1, dy2, K1, N, M, transA=True, out=out[:K1])
                    gemm_raw(a2, dy2, K2, N, M, transA=True, out=out[K1:])
                    return out
                dw = _wgrad_to_sink(gvw, both, (a1, a2, dy2))
        db = None
        if ctx.needs_input_grad[3]:
            db = _dense_bias_grad(dy, M, N, gvb)
        return dx1, dx2, dw, db


def linear2(x1, x2, w, bias):
    return Linear2Fn.apply(x1, x2, w, bias)


# ----------------------------------------------------------------------------- activations
class ActFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, kind, shift):
        x = _c(x)
        y = torch.empty_like(x)
        call("mulan_act_fwd", ptr(x), ptr(y), x.numel(), kind, float(shift), stream())
        ctx.save_for_backward(x)
        ctx.kind = kind
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, dy):
        (x,) = ctx.saved_tensors
        dy = _c(dy)
        dx = torch.empty_like(x)
        call("mulan_act_bwd", ptr(x), ptr(dy), ptr(dx), x.numel(), ctx.kind, stream())
        return dx, None, None


def silu(x):
    return ActFn.apply(x, 1, 0.0)


def softplus_shift(x, shift):
    return ActFn.apply(x, 2, shift)


# ----------------------------------------------------------------------------- group norm
def _seed_args(seed):
    """(seed by value, device pointer or None): a seed given as a 1-element int64 device tensor is read by the kernel
    when it runs (stream-ordered parameter: HIP-graph replay draws a fresh dropout mask per step)"""
    if torch.is_tensor(seed):
        return 0, seed
    return int(seed), None


GN_FUSED_REDUCE = _flag("GN_FUSED_REDUCE", "1")   # A/B switch: 0 = separate mulan_colsum launches
_TICKETS = {}


def _gn_tickets(device):
    """arrival counters of the in-kernel reductions (zero between launches).  One array per (device, stream): launches
    on one stream are ordered and each leaves its counters zero; two streams must never share them."""
    key = (device, torch.cuda.current_stream(device).cuda_stream if torch.device(device).type == "cuda" else 0)
    t = _TICKETS.get(key)
    if t is None:
        t = _TICKETS[key] = torch.zeros(16, device=device, dtype=torch.int32)
    return t


def reset_tickets():
    """zeroes the arrival counters (TrainState.zero_grad calls this once per step: a launch that died half-way in an
    earlier step must not leave a count behind)"""
    for t in _TICKETS.values():
        t.zero_()


class _GnBwd(NamedTuple):
    """what _gn_backward reads.  GroupNormFn, GroupNormSkipFn (_gn_forward) and GnConv3x3Fn build it in forward; `saved`
    goes through save_for_backward and is put back at the top of backward, as in _ConvBwd."""
    saved: tuple                   # (x1, x2 or None, gamma, beta, mean, rstd)
    meta: tuple                    # (groups, act, keep, seed: int or 1-element device tensor, offset)
    gv: tuple                      # (_gv(gamma), _gv(beta)): the gradient sinks
    bias_sink: Optional[tuple]     # _bias_sink_of(x1): the bias sinks of the convolution that produced x1
    keepbits: Optional[torch.Tensor] = None    # the dropout keep-bits the forward kernel stored; None: drawn again


def gn_reduce_grid_ok(C1, C2, groups):
    """the channel grid of the GroupNorm kernels that reduce over the samples inside the launch
    (mulan_groupnorm_bwd_fused, _fused_planes) and write planes (GnConv3x3Fn): both inputs in 32-channel slices, one
    maxima slot per slice, groups of 4 ... 32 channels that do not straddle a slice"""
    Ct = C1 + C2
    cpg = Ct // groups
    return C1 % 32 == 0 and C2 % 32 == 0 and Ct // 32 <= MAX_PARTS and cpg % 4 == 0 and 32 % cpg == 0


def _gn_forward(ctx, x1, x2, gamma, beta, norm):
    """norm = (groups, eps, act, keep, seed, offset)"""
    groups, eps, act, keep, seed, offset = norm
    x1, x2 = _c(x1), _c(x2)
    B, C1 = x1.shape[0], x1.shape[-1]
    C2 = 0 if x2 is None else x2.shape[-1]
    y = torch.empty((B, HW, C1 + C2), device=x1.device, dtype=torch.float32)
    mean = torch.empty((B, groups), device=x1.device, dtype=torch.float32)
    rstd = torch.empty_like(mean)
    # by-product for a following f16x3 convolution: the per-image maxima of y
    ymax = _maxima_slots(B, (C1 + C2) // 32, x1.device, CONV_MODE == "f16x3")
    sv, sd = _seed_args(seed)
    call("mulan_groupnorm_fwd_dyn", ptr(x1), ptr(x2), C1, C2, ptr(gamma), ptr(beta), ptr(y), ptr(mean), ptr(rstd), B,
         HW, groups, float(eps), int(act), float(keep), sv, int(offset), ptr(sd), ptr(ymax), stream())
    _leave_maxima(y, ymax)
    gn = _GnBwd(saved=(x1, x2, gamma, beta, mean, rstd), meta=(groups, int(act), float(keep), seed, int(offset)),
                gv=(_gv(gamma), _gv(beta)), bias_sink=_bias_sink_of(x1, C1))
    ctx.save_for_backward(*gn.saved)
    ctx.gn = gn._replace(saved=())
    return y, x1, x2


def _gn_backward(rec, dy, add1=None, add2=None, planes_out=False, add1b=None):
    """dx1, dx2 (+ the gradients add1 / add2 that reach x1 / x2 through a skip path), dgamma, dbeta; rec: the _GnBwd of
    the node.  The written dx1 carries its maxima and per-sample channel sums for the convolution in front (whose dy it
    is).
    planes_out: the caller vouches that dx1 is consumed ONLY by the f16x3 kernels of the convolution that produced x1
    (GnConv3x3Fn with x1_grad_planes): where the kernel variant applies (single input, no skip-path gradient, dy with
    its maxima) dx1 is then written as split planes and returned as a planes-only stand-in (_planes_only_grad)."""
    x1, x2, gamma, beta, mean, rstd = rec.saved
    groups, act, keep, seed, offset = rec.meta
    dy = _c(dy)
    dev = dy.device
    B, C1 = x1.shape[0], x1.shape[-1]
    C2 = 0 if x2 is None else x2.shape[-1]
    Ct = C1 + C2
    dymax_in = _left(dy, "_absmax")
    if add1b is not None and add1 is None:
        add1, add1b = add1b, None
    sv, sd = _seed_args(seed)
    gvg, gvb = rec.gv
    sink, sink2 = rec.bias_sink if rec.bias_sink is not None else (None, None)
    # the sums over the samples (dgamma, dbeta, the bias gradient of the convolution in front) inside the launch
    fused = GN_FUSED_REDUCE and gn_reduce_grid_ok(C1, C2, groups)
    planes = bool(planes_out and fused and x2 is None and add1 is None and dymax_in is not None and
                  B * HW * C1 * 4 < 2 ** 31)
    if planes:
        dxp = torch.empty(B * HW * C1 * 4, device=dev, dtype=torch.uint8)
        bound = torch.empty((B, MAX_PARTS), device=dev, dtype=torch.int32)
    else:
        dx1 = torch.empty_like(x1)
        dx2 = torch.empty_like(x2) if x2 is not None else None
    parts = torch.empty((2, B, Ct), device=dev, dtype=torch.float32)     # dgamma / dbeta per-sample partials
    dgp, dbp = parts[0], parts[1]
    f16 = CONV_MODE == "f16x3" and not planes          # (the plane variant leaves the maxima of dx1 in `bound`)
    m1 = _maxima_slots(B, C1 // 32, dev, f16)
    m2 = _maxima_slots(B, C2 // 32, dev, f16 and x2 is not None)
    csum = torch.empty((B, Ct), device=dev, dtype=torch.float32)
    dgamma = _fresh(gvg) if gvg is not None else torch.empty(Ct, device=dev, dtype=torch.float32)
    dbeta = _fresh(gvb) if gvb is not None else torch.empty(Ct, device=dev, dtype=torch.float32)
    if planes:
        call("mulan_groupnorm_bwd_fused_planes", ptr(dy), ptr(dymax_in), ptr(x1), C1, ptr(gamma), ptr(beta), ptr(mean),
             ptr(rstd), ptr(dxp), ptr(dgp), ptr(dbp), B, HW, groups, act, keep, sv, offset, ptr(sd), ptr(bound),
             ptr(csum), ptr(dgamma), ptr(dbeta), ptr(sink), ptr(sink2), ptr(_gn_tickets(dev)), ptr(rec.keepbits), stream())
        dx1, dx2 = _planes_only_grad(x1.shape, dev, dxp, bound), None
    elif fused:
        call("mulan_groupnorm_bwd_fused", ptr(dy), ptr(x1), ptr(x2), C1, C2, ptr(gamma), ptr(beta), ptr(mean), ptr(rstd),
             ptr(dx1), ptr(dx2), ptr(dgp), ptr(dbp), B, HW, groups, act, keep, sv, offset, ptr(sd), ptr(m1), ptr(m2),
             ptr(_c(add1)), ptr(_c(add2)), ptr(_c(add1b)), ptr(csum), ptr(dgamma), ptr(dbeta), ptr(sink), ptr(sink2),
             ptr(_gn_tickets(dev)), stream())
    else:
        if add1b is not None:
            add1 = add1 + add1b
        call("mulan_groupnorm_bwd_dyn", ptr(dy), ptr(x1), ptr(x2), C1, C2, ptr(gamma), ptr(beta), ptr(mean), ptr(rstd),
             ptr(dx1), ptr(dx2), ptr(dgp), ptr(dbp), B, HW, groups, act, keep, sv, offset, ptr(sd), 0, ptr(m1), ptr(m2),
             ptr(_c(add1)), ptr(_c(add2)), ptr(csum), stream())
        if Ct % 4 == 0 and dgamma.data_ptr() % 16 == 0 and dbeta.data_ptr() % 16 == 0:
            call("mulan_colsum_pair", ptr(parts), ptr(dgamma), ptr(dbeta), B, Ct, stream())     # both sums, one launch
        else:
            colsum_raw(dgp, 1, B, Ct, out=dgamma.view(1, Ct))
            colsum_raw(dbp, 1, B, Ct, out=dbeta.view(1, Ct))
    if fused and sink is not None:
        _leave(dx1, "_biasdone", sink, sink2)
    if m1 is not None:
        _leave(dx1, "_absmax", m1)
    if m2 is not None:
        _leave(dx2, "_absmax", m2)
    _leave(dx1, "_colsum", csum[:, :C1])                # a strided view when there is an x2: consumers take its row stride
    return dx1, dx2, dgamma, dbeta


class GroupNormFn(torch.autograd.Function):
    """y = dropout(act(GroupNorm([x1|x2])))  -> [B,1024,C1+C2]"""

    @staticmethod
    def forward(ctx, x1, x2, gamma, beta, groups, eps, act, keep, seed, offset):
        return _gn_forward(ctx, x1, x2, gamma, beta, (groups, eps, act, keep, seed, offset))[0]

    @staticmethod
    @once_differentiable
    def backward(ctx, dy):
        return _gn_backward(ctx.gn._replace(saved=ctx.saved_tensors), dy) + (None,) * 6


def _skip_outputs(y, x1, x2, tagged=None):
    """(y, s1) or (y, s1, s2): y with the aliases of x1 (, x2) for the block's skip path.  The maxima a producer left on
    x (on `tagged`, where x1 / x2 are contiguous copies of what the caller was given) stay valid for the alias."""
    t1, t2 = (x1, x2) if tagged is None else tagged
    s1 = _carry(t1, x1.view_as(x1), tags=("_absmax",))
    s2 = _carry(t2, x2.view_as(x2), tags=("_absmax",)) if x2 is not None else None
    return (y, s1) if x2 is None else (y, s1, s2)


class GroupNormSkipFn(torch.autograd.Function):
    """(y, s1, s2) with y as GroupNormFn and s1 / s2 aliases of x1 / x2 for the block's skip path (the ResnetBlock
    residual or nin_shortcut, ldm/model_vdm.py:652-656): the gradients that come back through s1 / s2 are added
    inside the GroupNorm backward kernel instead of by a separate accumulation pass."""

    @staticmethod
    def forward(ctx, x1, x2, gamma, beta, groups, eps, act, keep, seed, offset):
        y, x1c, x2c = _gn_forward(ctx, x1, x2, gamma, beta, (groups, eps, act, keep, seed, offset))
        return _skip_outputs(y, x1c, x2c, tagged=(x1, x2))

    @staticmethod
    @once_differentiable
    def backward(ctx, dy, ds1, ds2=None):
        if dy is None:     # only the skip path was used downstream
            return (ds1, ds2) + (None,) * 8
        return _gn_backward(ctx.gn._replace(saved=ctx.saved_tensors), dy, ds1, ds2) + (None,) * 6


def group_norm(x1, x2, gamma, beta, *, groups=32, eps=1e-6, act=True, keep=1.0, seed=0, offset=0):
    return GroupNormFn.apply(x1, x2, gamma, beta, groups, eps, int(act), keep, seed, offset)   # seed: int or device tensor


def group_norm_skip(x1, x2, gamma, beta, *, groups=32, eps=1e-6, act=True, keep=1.0, seed=0, offset=0):
    """-> (y, s1, s2): use s1 / s2 instead of x1 / x2 on the skip path of the block (see GroupNormSkipFn)"""
    out = GroupNormSkipFn.apply(x1, x2, gamma, beta, groups, eps, int(act), keep, seed, offset)
    return out if len(out) == 3 else (out[0], out[1], None)


GN_CONV_PLANES = _flag("GN_CONV_PLANES", "1")    # A/B switch: 0 = fp32 hand-over (two ops)
# Backward counterpart (round 3): the gradient a GroupNorm backward hands to the convolution in front of it (norm2 ->
# conv1 of a ResnetBlock) goes as split planes too -- the input-gradient convolution then runs on the plane-fed
# instantiation of the kernel (no split, no plane stores out of the MFMA kernel).  A/B switch: 0 = fp32 hand-over.
GRAD_PLANES = _flag("GRAD_PLANES", "1")
# the dropout keep-bits of norm2 are stored by the forward kernel and re-used by the backward kernel (A/B: 0 = re-drawn)
KEEP_BITS = _flag("KEEP_BITS", "1")
# GroupNorm normalised inside the convolution's patch fill (mulan_groupnorm_stats + mulan_conv3x3_fwd_f16x3_gn_in) where no
# dropout is drawn.  GN_FILL: wherever the convolution's weight needs no gradient (evaluators, sampler, the ODE
# evaluator's input-only differentiation) and the convolution has one 128-wide block of output channels: the normalised
# tensor never reaches HBM (with the statistics hand-over below: sampler step -15 %, ODE function evaluation -7.5 % at E = 128).  With N = 256 every input
# element is normalised by two blocks and the fill's arithmetic costs more than the GroupNorm pass it saves (dense
# evaluation at E = 256: +4.5 %), so those layers keep the plane hand-over; GN_FILL_MAX_N is that limit.
# GN_FILL_TRAIN (A/B switch, off: the train step is 1.2 % slower with it, profiles/DESIGN_r04.md 3.2): also in training, the convolution
# then stores the planes for its weight gradient.
GN_FILL = _flag("GN_FILL", "1")
GN_FILL_MAX_N = int(_os.environ.get("MULAN_GN_FILL_MAX_N", "128"))
GN_FILL_TRAIN = _flag("GN_FILL_TRAIN", "0")
# ... and the statistics handed from convolution to convolution: a GroupNorm-fed convolution leaves the partial sums of
# its output (per image, 8-row tile, channel quad) on the tensor, the next one forms mean / rstd from them in its prologue:
# no pass over the tensor between two convolutions of a forward-only chain.  A/B switch: 0 = mulan_groupnorm_stats in
# front of every convolution (bit-identical to the plane hand-over; with the hand-over the statistics agree to rounding).
GN_FILL_STATS = _flag("GN_FILL_STATS", "1")
# training step: GroupNorm forward as the streaming kernel on the statistics the producing convolution left, where that
# kernel is the faster one (GnConv3x3Fn.forward): dropout layers and the 2 x 128-channel concat, at 32 <= images per launch
# <= 96 -- the per-GPU batches of an 8-GPU job.  Measured in the train step of BASELINE configs[2]
# (profiles/r05_gn_fwd_stream_in_step.log): 64 images 42.78 -> 42.50 ms, 32 images 28.52 -> 28.42, 16 images 23.42 -> 23.65,
# 128 images 78.98 -> 79.08 (what the kernel gains alone, 4 us per launch, the statistics in the convolution epilogue cost
# back).  MULAN_GN_FWD_STREAM=0: the slab kernel everywhere (the round-4 path); GN_FWD_STREAM_B: the batch window.
GN_FWD_STREAM = _flag("GN_FWD_STREAM", "1")
GN_FWD_STREAM_B = tuple(int(v) for v in _os.environ.get("MULAN_GN_FWD_STREAM_B", "32,96").split(","))


def _gn_fwd_stream_on(B):
    return GN_FWD_STREAM and GN_FWD_STREAM_B[0] <= B <= GN_FWD_STREAM_B[1]


def _gn_stats_of(x, C):
    """the partial sums the convolution that produced x left on it: [B, row tiles (4, 8 or 16), C / 4, 2], or None"""
    c = _left(x, "_gnstats")
    if (c is not None and c.dim() == 4 and c.shape[0] == x.shape[0] and
            c.shape[1] in (H // 8, H // 4, H // 2) and tuple(c.shape[2:]) == (C // 4, 2)):
        return c
    return None


def _gn_stats_pair(x1, x2, C1, C2):
    """(st1, st2) of [x1 | x2] -- st2 None without an x2 -- or (None, None): the statistics must be there for both inputs
    and over the same number of row tiles"""
    st1 = _gn_stats_of(x1, C1)
    st2 = _gn_stats_of(x2, C2) if (st1 is not None and x2 is not None) else None
    if st1 is None or (x2 is not None and (st2 is None or st2.shape[1] != st1.shape[1])):
        return None, None
    return st1, st2


def _conv_outputs(B, N, dev, bias, cbias, res, want_stats):
    """what a GroupNorm-fed convolution launch writes and reads besides its operands: y, ymax (None where the launch has
    more blocks per image than maxima slots), the cbias mode, contiguous bias / cbias / res, and -- want_stats -- ystats:
    one row of partial sums per row tile of that launch (8, 4 or 2 image rows) for the GroupNorm behind it"""
    y = torch.empty((B, HW, N), device=dev, dtype=torch.float32)
    ymax = _maxima_slots(B, (H // 8) * (N // 128), dev)
    bias_c, cb_c, res_c = _c(bias), _c(cbias), _c(res)
    ystats = None
    if want_stats:
        rows = lib.load().mulan_conv3x3_f16x3_tile_rows(B, H, N, int(ymax is not None))
        ystats = torch.empty((B, H // rows, N // 4, 2), device=dev, dtype=torch.float32)
    return y, ymax, _cbias_mode(cbias), bias_c, cb_c, res_c, ystats


def gn_conv_ok(C1, C2, N, groups):
    """GroupNorm -> 3x3 convolution with the normalised tensor handed over as split fp16 planes (GnConv3x3Fn)"""
    Ct = C1 + C2
    return (GN_CONV_PLANES and CONV_MODE == "f16x3" and Ct % 128 == 0 and N % 128 == 0 and Ct % groups == 0 and
            gn_reduce_grid_ok(C1, C2, groups))


def _gn_conv_norm(x1, x2, gamma, beta, norm, fill, want_planes, want_bits):
    """The GroupNorm stage of GnConv3x3Fn.forward; norm = (groups, eps, act, keep, seed, offset).  Returns what the
    convolution stage and the backward pass need: (ys, bound, mean, rstd, keepbits, st1, st2).
    fill: only the statistics here (mulan_groupnorm_stats -- or none at all: st1 / st2, the partial sums the producing
    convolutions left, go to the convolution, which normalises inside its patch fill); ys is then the plane tensor that
    convolution writes for its weight gradient (want_planes; else empty).
    Otherwise ys = the normalised tensor as split planes scaled with `bound`, and keepbits (want_bits) the dropout bits as
    drawn."""
    groups, eps, act, keep, seed, offset = norm
    B, C1 = x1.shape[0], x1.shape[-1]
    C2 = 0 if x2 is None else x2.shape[-1]
    Ct, dev = C1 + C2, x1.device
    bound = torch.empty((B, MAX_PARTS), device=dev, dtype=torch.int32)
    mean = torch.empty((B, groups), device=dev, dtype=torch.float32)
    rstd = torch.empty_like(mean)
    gn_in = (ptr(x1), ptr(x2), C1, C2, ptr(gamma), ptr(beta))
    if fill:
        st1, st2 = _gn_stats_pair(x1, x2, C1, C2) if GN_FILL_STATS and not want_planes else (None, None)
        if st1 is None:
            call("mulan_groupnorm_stats", *gn_in, ptr(mean), ptr(rstd), ptr(bound), B, HW, groups, eps, stream())
        ys = torch.empty(B * HW * Ct * 4 if want_planes else 0, device=dev, dtype=torch.uint8)
        return ys, bound, mean, rstd, None, st1, st2
    ys = torch.empty(B * HW * Ct * 4, device=dev, dtype=torch.uint8)
    sv, sd = _seed_args(seed)
    # the convolutions that produced x1 (, x2) left the partial sums of the statistics: the streaming kernel (no
    # statistics phase, 62 registers) where it is the faster one -- dropout layers and the 2 x 128-channel concat
    # (profiles/r05_gn_stream_bench.log: 31.8 vs 36.0 us and 52.4 vs 55.6 us at B = 128; 128 channels without
    # dropout: 30.2 vs 27.7 us, the slab kernel stays), see GN_FWD_STREAM
    st1 = st2 = None
    if _gn_fwd_stream_on(B) and (keep < 1.0 or C2 > 0) and Ct // 32 <= MAX_PARTS:
        st1, st2 = _gn_stats_pair(x1, x2, C1, C2)
    # dropout layer whose backward will write planes (x1_grad_planes): keep the 4 keep-bits per float4 as drawn (2 MB at
    # B = 128, C = 128), so that the backward kernel does not repeat the Philox rounds
    keepbits = torch.empty(B * (Ct // 32) * 1024, device=dev, dtype=torch.int32) if want_bits else None
    out = (ptr(ys), ptr(mean), ptr(rstd))
    tail = (B, HW, groups, eps, act, keep, sv, offset, ptr(sd), ptr(bound))
    if st1 is not None:
        call("mulan_groupnorm_fwd_stream", *gn_in, None, *out, ptr(st1), ptr(st2), int(st1.shape[1]), *tail, ptr(keepbits),
             stream())
    elif want_bits:
        call("mulan_groupnorm_fwd_planes_keepbits", *gn_in, *out, *tail, ptr(keepbits), stream())
    else:
        call("mulan_groupnorm_fwd_planes", *gn_in, *out, *tail, stream())
    return ys, bound, mean, rstd, keepbits, None, None


class GnConv3x3Fn(torch.autograd.Function):
    """y = conv3x3(dropout(act(GroupNorm([x1|x2]))), w) + bias + cbias + res  (norm1 + swish -> conv1 and norm2 + swish +
    dropout -> conv2 of the ResnetBlock, ldm/model_vdm.py:622-656) as ONE autograd node, so that the normalised tensor
    never exists in fp32: the GroupNorm kernel writes it as the split fp16 operand planes of the f16x3 kernels (scaled by
    an a-priori bound, mulan_groupnorm_fwd_planes), the convolution copies them into LDS (no split, no plane stores out
    of the MFMA kernel: 5-13 % of a launch) and its weight-gradient kernel reads the same tensor.  With skip=True also
    returns the aliases s1 (, s2) of x1 (, x2) for the block's skip path, whose gradients are added inside the
    GroupNorm backward kernel (as GroupNormSkipFn)."""

    @staticmethod
    def forward(ctx, x1, x2, gamma, beta, w, bias, cbias, res, groups, eps, act, keep, seed, offset, skip,
                x1_grad_planes=False):
        need = ctx.needs_input_grad
        # x1_grad_planes: the caller vouches that x1 has no consumer besides this op (conv1's output inside a
        # ResnetBlock); if x1's producer accepts it (tag below), d x1 then travels as split planes only
        ctx.x1_grad_planes = bool(x1_grad_planes and not skip and x2 is None and _left(x1, "_accepts_grad_planes"))
        # x1 is a block output that also feeds a skip connection (tee): this op's GroupNorm backward will add the gradient
        # that arrives through that connection (it is there first: the up path runs first in the backward pass)
        box = getattr(x1, "_grad_box", None)
        ctx.grad_box = None
        if box is not None and skip and not box.claimed and need[0]:
            box.claimed = True
            ctx.grad_box = box
        x1, x2, w = _c(x1), _c(x2), _c(w)
        B, C1 = x1.shape[0], x1.shape[-1]
        C2 = 0 if x2 is None else x2.shape[-1]
        Ct, N, dev = C1 + C2, w.shape[-1], x1.device
        eps, act, keep, offset = float(eps), int(act), float(keep), int(offset)
        # fill: statistics pass + the convolution that normalises inside its patch fill (no dropout): bit for bit the
        # result of the two-kernel path
        fill = (keep >= 1.0 and (C2 == 0 or C2 == C1) and Ct <= 512 and N <= GN_FILL_MAX_N and
                (GN_FILL_TRAIN if need[4] else GN_FILL))
        want_planes = bool(need[4])      # (the weight gradient reads them)
        want_bits = bool(KEEP_BITS and keep < 1.0 and ctx.x1_grad_planes and any(need[:5]))
        ys, bound, mean, rstd, keepbits, st1, st2 = _gn_conv_norm(x1, x2, gamma, beta, (groups, eps, act, keep, seed, offset),
                                                                  fill, want_planes, want_bits)
        wp, wmax = _pack_weights(w, Ct, N, 0)
        # ystats: by-product for the GroupNorm behind this convolution (GN_FILL_STATS, GN_FWD_STREAM)
        want_stats = (GN_FILL_STATS and not want_planes) if fill else (_gn_fwd_stream_on(B) and N // 32 <= MAX_PARTS)
        y, ymax, mode, bias_c, cb_c, res_c, ystats = _conv_outputs(B, N, dev, bias, cbias, res, want_stats)
        epilogue = (ptr(bias_c), ptr(cb_c), mode, ptr(res_c), ptr(y), ptr(ymax), ptr(ystats))
        if fill:
            name, fn = "gn_in", "mulan_conv3x3_fwd_f16x3_gn_in"
            operands = (ptr(x1), ptr(x2), C1, C2, ptr(gamma), ptr(beta), ptr(mean), ptr(rstd), groups, act, eps, ptr(bound),
                        ptr(st1), ptr(st2), 0 if st1 is None else int(st1.shape[1]), ptr(wp), ptr(wmax), *epilogue,
                        ptr(ys) if want_planes else None, B, H, W, N)
        else:
            name, fn = "planes_in", "mulan_conv3x3_fwd_f16x3_planes_in_stats"
            operands = (ptr(ys), ptr(bound), ptr(wp), ptr(wmax), *epilogue, 1, B, H, W, Ct, N)
        _timed(f"conv3x3_f16x3_kernel<{name}>", 2.0 * B * HW * 9 * Ct * N, lambda: call(fn, *operands, stream()))
        _leave_maxima(y, ymax)
        if ystats is not None:
            _leave(y, "_gnstats", ystats)
        gn = _GnBwd(saved=(x1, x2, gamma, beta, mean, rstd), gv=(_gv(gamma), _gv(beta)), bias_sink=_bias_sink_of(x1, C1),
                    meta=(groups, act, 1.0, 0, 0) if fill else (groups, act, keep, seed, offset), keepbits=keepbits)
        # (planes = False when the kernel needs no gradient -- the ODE evaluator differentiates with respect to the input
        # only: input gradient without plane output, no weight-gradient launch)
        conv = _ConvBwd(saved=(ys, w), planes=want_planes, xmax=bound, wmax=wmax, has=_has(bias, cbias, res),
                        gv=(_gv(w), _gv(bias)), need=(True,) + tuple(need[4:8]))
        return GnConv3x3Fn._finish_forward(ctx, gn, conv, y, res, skip)

    @staticmethod
    def _finish_forward(ctx, gn, conv, y, res, skip):
        """keeps the two records for backward (their tensors through save_for_backward) and tags the output"""
        ctx.save_for_backward(*gn.saved, *conv.saved, conv.xmax)
        ctx.gn = gn._replace(saved=())
        ctx.conv = conv._replace(saved=(), xmax=None)
        if conv.gv[1] is not None and conv.need[2]:
            _leave_bias_sink(y, conv.gv[1], res)
        Ct, N = conv.saved[1].shape[2:]
        if res is None and conv.has[1] in (None, 2) and grad_planes_eligible(Ct, N):      # (no per-pixel cbias)
            _leave(y, "_accepts_grad_planes")        # this op's backward understands a planes-only output gradient
        return _skip_outputs(y, *gn.saved[:2]) if skip else y

    @staticmethod
    @once_differentiable
    def backward(ctx, dy, ds1=None, ds2=None):
        nones = (None,) * 8
        add1b = None
        if ctx.grad_box is not None:
            add1b = ctx.grad_box.take()
        if dy is None:     # only the skip path was used downstream
            if add1b is not None:
                ds1 = add1b if ds1 is None else ds1 + add1b
            return (ds1, ds2) + (None,) * 6 + nones
        *gn_saved, ys, w, bound = ctx.saved_tensors
        planes_out = bool(ctx.x1_grad_planes and GRAD_PLANES and ds1 is None and add1b is None)
        conv = ctx.conv._replace(saved=(ys, w), xmax=bound, want_dx_max=planes_out)
        dh, dw, dbias, dcb, dres = _conv3x3_backward(conv, dy)
        gn = ctx.gn._replace(saved=tuple(gn_saved))
        dx1, dx2, dgamma, dbeta = _gn_backward(gn, dh, ds1, ds2, planes_out=planes_out, add1b=add1b)
        return (dx1, dx2, dgamma, dbeta, dw, dbias, dcb, dres) + nones


def gn_conv3x3(x1, x2, gamma, beta, w, bias=None, cbias=None, res=None, *, groups=32, eps=1e-6, act=True, keep=1.0,
               seed=0, offset=0, skip=False, x1_grad_planes=False):
    """-> y, or (y, s1, s2) with skip=True.  Falls back to group_norm(_skip) + conv3x3 where the plane hand-over does not
    apply (other arithmetic modes, channel counts off the 128 grid)."""
    C1 = x1.shape[-1]
    C2 = 0 if x2 is None else x2.shape[-1]
    if gn_conv_ok(C1, C2, w.shape[-1], groups) and x1.is_cuda:
        out = GnConv3x3Fn.apply(x1, x2, gamma, beta, w, bias, cbias, res, groups, eps, int(act), keep, seed, offset, skip,
                                x1_grad_planes)
        if not skip:
            return out
        return out if len(out) == 3 else (out[0], out[1], None)
    if skip:
        h, s1, s2 = group_norm_skip(x1, x2, gamma, beta, groups=groups, eps=eps, act=act, keep=keep, seed=seed, offset=offset)
        return conv3x3(h, w, bias, cbias, res), s1, s2
    return conv3x3(group_norm(x1, x2, gamma, beta, groups=groups, eps=eps, act=act, keep=keep, seed=seed, offset=offset),
                   w, bias, cbias, res)


# ----------------------------------------------------------------------------- attention core
ATTN_F16X3 = True      # attention products on the split-operand kernels in f16x3 mode (else the exact-fp32 MFMA GEMM)


def _attn_fast_ok(q):
    B, S, C = q.shape
    return CONV_MODE == "f16x3" and ATTN_F16X3 and S == HW and C % 128 == 0 and B * S * S * 4 < 2 ** 31


def _const_max(B, value, device):
    """[B,16] maxima array holding an a-priori bound (softmax outputs are <= 1): the split scheme is accurate relative
    to each element, so a loose bound costs nothing until values fall 2^-24 below it"""
    import struct
    return torch.full((B, MAX_PARTS), struct.unpack('<i', struct.pack('<f', float(value)))[0], device=device,
                      dtype=torch.int32)


def _pack_batched(w, transpose, wmax):
    """w [B, K, N] (or [B, N, K] with transpose) -> packed per-image operands of linear_batched_raw"""
    B = w.shape[0]
    K, N = (w.shape[2], w.shape[1]) if transpose else (w.shape[1], w.shape[2])
    wp = torch.empty(B * K * N * 4, device=w.device, dtype=torch.uint8)
    call("mulan_linear_pack_f16x3_batched", ptr(w), ptr(wp), ptr(wmax), K, N, int(transpose), B, stream())
    return wp


def linear_batched_raw(x, xmax, wp, wmax, N, planes=False, res=None):
    """y[b] = x[b] @ W[b] (+ res [B, 1024, N]): x [B, 1024, K]; returns y [B, 1024, N] (+ the split planes of x when
    planes=True)"""
    B, R, K = x.shape
    y = torch.empty((B, R, N), device=x.device, dtype=torch.float32)
    xs = torch.empty(B * R * K * 4, device=x.device, dtype=torch.uint8) if planes else None
    _timed("linear_f16x3_kernel(batched)", 2.0 * B * R * K * N,
           lambda: call("mulan_linear_f16x3_batched", ptr(x), ptr(xmax), K, ptr(wp), ptr(wmax), ptr(res), ptr(y), ptr(xs), N,
                        B * R, R, stream()))
    return (y, xs) if planes else y


def bmm_tn_planes_raw(xs, xmax, dys, dymax, B, C, N):
    """out[b] = x[b]^T @ dy[b] -> [B, C, N] from split planes"""
    out = torch.empty((B, C, N), device=xs.device, dtype=torch.float32)
    _timed("bmm_tn_f16x3_planes", 2.0 * B * HW * C * N,
           lambda: call("mulan_bmm_tn_f16x3_planes", ptr(xs), ptr(xmax), ptr(dys), ptr(dymax), ptr(out), B, H, W, C, N,
                        stream()))
    return out


ATTN_FUSED = True      # fused (flash-style) attention kernels, C = 128 and 256: S and P never reach HBM


def _attn_fused_ok(q):
    """forward and backward kernels exist for C = 128 and, since round 4, C = 256 (the ImageNet-32 width: the backward
    pass with its output channels split over blocks, attention_f16x3.hip); blockIdx.y carries the image"""
    B, S, C = q.shape
    return CONV_MODE == "f16x3" and ATTN_F16X3 and ATTN_FUSED and S == HW and C in (128, 256) and B <= 65535


def _attn_fused_fwd_only_ok(q, k, v):
    """kept for callers that want the bare forward kernel (no autograd node at all)"""
    B, S, C = q.shape
    return (_attn_fused_ok(q) and
            not (torch.is_grad_enabled() and (q.requires_grad or k.requires_grad or v.requires_grad)))


def fused_attention_forward(q, k, v):
    """softmax((q / sqrt(C)) k^T) v by the fused forward kernel alone (no tape): C = 128 or 256"""
    q, k, v = _c(q), _c(k), _c(v)
    B, S, C = q.shape
    qm, km, vm = cached_absmax(q), cached_absmax(k), cached_absmax(v)
    qt, _ = _attn_packs(q, qm, True, False)
    kt, _ = _attn_packs(k, km, True, False)
    _, vn = _attn_packs(v, vm, False, True)
    o = torch.empty_like(q)
    lse = torch.empty((B, S), device=q.device, dtype=torch.float32)
    _timed("attn_f16x3_kernel<fwd>", 4.0 * B * S * S * C,
           lambda: call("mulan_attention_fwd_f16x3", ptr(qt), ptr(kt), ptr(vn), ptr(qm), ptr(km), ptr(vm), ptr(o), ptr(lse),
                        B, S, C, 1.0 / math.sqrt(C), stream()))
    return o


def _attn_packs(x, xmax, want_t=True, want_n=True):
    """("T" pack, "N" pack) of x [B, 1024, C] (C = 128 / 256) for the fused attention kernels, one pass over x"""
    B, S, C = x.shape
    xt = torch.empty(B * S * C * 4, device=x.device, dtype=torch.uint8) if want_t else None
    xn = torch.empty(B * S * C * 4, device=x.device, dtype=torch.uint8) if want_n else None
    call("mulan_attention_pack_f16x3", ptr(x), ptr(xmax), ptr(xt), ptr(xn), B, S, C, stream())
    return xt, xn


class FusedAttentionFn(torch.autograd.Function):
    """softmax((q / sqrt(C)) k^T) v on the fused f16x3 kernels (attention_f16x3.hip): the forward kernel keeps the online
    softmax state and writes o + the per-query log-sum-exp, the backward kernels recompute the probabilities from it.
    Saved for backward: the split packs of q, k, v (which replace the fp32 tensors), o and lse -- no [B, 1024, 1024]
    tensor."""

    @staticmethod
    def forward(ctx, q, k, v):
        q, k, v = _c(q), _c(k), _c(v)
        B, S, C = q.shape
        alpha = 1.0 / math.sqrt(C)
        need = any(ctx.needs_input_grad)          # (grad mode is off inside Function.forward: this is the signal)
        qm, km, vm = cached_absmax(q), cached_absmax(k), cached_absmax(v)
        qt, qn = _attn_packs(q, qm, True, need)
        kt, kn = _attn_packs(k, km, True, need)
        vt, vn = _attn_packs(v, vm, need, True)
        o = torch.empty_like(q)
        lse = torch.empty((B, S), device=q.device, dtype=torch.float32)
        _timed("attn_f16x3_kernel<fwd>", 4.0 * B * S * S * C,
               lambda: call("mulan_attention_fwd_f16x3", ptr(qt), ptr(kt), ptr(vn), ptr(qm), ptr(km), ptr(vm), ptr(o),
                            ptr(lse), B, S, C, alpha, stream()))
        if need:
            ctx.save_for_backward(o, lse, qt, qn, kt, kn, vt, qm, km, vm)
        return o

    @staticmethod
    @once_differentiable
    def backward(ctx, do):
        o, lse, qt, qn, kt, kn, vt, qm, km, vm = ctx.saved_tensors
        do = _c(do)
        B, S, C = o.shape
        alpha = 1.0 / math.sqrt(C)
        dom = cached_absmax(do)
        delta = torch.empty((B, S), device=o.device, dtype=torch.float32)
        call("mulan_attention_delta", ptr(do), ptr(o), ptr(delta), B, S, C, stream())
        dm = absmax_rows(delta)
        dot, don = _attn_packs(do, dom)
        dq, dk, dv = torch.empty_like(o), torch.empty_like(o), torch.empty_like(o)
        _timed("attn_f16x3_kernel<bwd>", 14.0 * B * S * S * C,
               lambda: call("mulan_attention_bwd_f16x3", ptr(qt), ptr(qn), ptr(kt), ptr(kn), ptr(vt), ptr(dot), ptr(don),
                            ptr(qm), ptr(km), ptr(vm), ptr(dom), ptr(dm), ptr(lse), ptr(delta), ptr(dq), ptr(dk),
                            ptr(dv), B, S, C, alpha, stream()))
        return dq, dk, dv


class AttentionFn(torch.autograd.Function):
    """softmax((q / sqrt(C)) k^T) v for one head over 1024 positions (ldm/model_vdm.py:679-683,704-802).
    f16x3 mode: S = q k^T, O = P v, dP = dO v^T and dQ = dS k run on the split-operand kernel with one packed operand
    per image; the 1/sqrt(C) is folded into the softmax kernels."""

    @staticmethod
    def forward(ctx, q, k, v):
        q, k, v = _c(q), _c(k), _c(v)
        B, S, C = q.shape
        alpha = 1.0 / math.sqrt(C)
        ctx.fast = _attn_fast_ok(q)
        if not ctx.fast:
            s = gemm_raw(q, k, S, S, C, transB=True, alpha=alpha, batch=B, sA=S * C, sB=S * C)
            p = torch.empty_like(s)
            call("mulan_softmax_fwd", ptr(s), ptr(p), B * S, S, stream())
            del s
            o = gemm_raw(p, v, S, C, S, batch=B, sA=S * S, sB=S * C)
            ctx.save_for_backward(q, k, v, p)
            return o.view(B, S, C)
        qm, km, vm = cached_absmax(q), cached_absmax(k), cached_absmax(v)
        s = linear_batched_raw(q, qm, _pack_batched(k, True, km), km, S)                   # q @ k^T
        p = torch.empty_like(s)
        call("mulan_softmax_scaled_fwd", ptr(s), ptr(p), B * S, S, alpha, stream())
        del s
        o = linear_batched_raw(p, _const_max(B, 1.0, q.device), _pack_batched(v, False, vm), vm, C)   # P @ v
        ctx.save_for_backward(q, k, v, p)
        ctx.aux = (km, vm)
        return o

    @staticmethod
    @once_differentiable
    def backward(ctx, do):
        q, k, v, p = ctx.saved_tensors
        do = _c(do)
        B, S, C = q.shape
        alpha = 1.0 / math.sqrt(C)
        if not ctx.fast:
            dv = gemm_raw(p, do, S, C, S, transA=True, batch=B, sA=S * S, sB=S * C).view(B, S, C)
            dp = gemm_raw(do, v, S, S, C, transB=True, batch=B, sA=S * C, sB=S * C)
            ds = torch.empty_like(dp)
            call("mulan_softmax_bwd", ptr(p), ptr(dp), ptr(ds), B * S, S, stream())
            del dp
            dq = gemm_raw(ds, k, S, C, S, alpha=alpha, batch=B, sA=S * S, sB=S * C).view(B, S, C)
            dk = gemm_raw(ds, q, S, C, S, transA=True, alpha=alpha, batch=B, sA=S * S, sB=S * C).view(B, S, C)
            return dq, dk, dv
        # The four products whose long operand is read once (S, O, dP, dQ) run on the split-operand kernel.  The two
        # transposed ones (dV = P^T dO, dK = dS^T q) would need P and dS as split planes (mulan_bmm_tn_f16x3_planes):
        # writing and re-reading those 4 B S^2-byte tensors costs as much as the exact-fp32 GEMM they would replace
        # (measured at B = 128: 203 us + 150 us of plane traffic against 338 us), so they stay on the fp32 MFMA GEMM.
        km, vm = ctx.aux
        ctx.aux = None
        dv = gemm_raw(p, do, S, C, S, transA=True, batch=B, sA=S * S, sB=S * C).view(B, S, C)      # P^T @ dO
        dp = linear_batched_raw(do, cached_absmax(do), _pack_batched(v, True, vm), vm, S)          # dO @ v^T
        ds = torch.empty_like(dp)
        rowmax = torch.empty((B, S), device=q.device, dtype=torch.float32)
        call("mulan_softmax_scaled_bwd", ptr(p), ptr(dp), ptr(ds), B * S, S, alpha, ptr(rowmax), stream())
        dsm = absmax_rows(rowmax)
        del dp
        dq = linear_batched_raw(ds, dsm, _pack_batched(k, False, km), km, C)                       # dS @ k
        dk = gemm_raw(ds, q, S, C, S, transA=True, batch=B, sA=S * S, sB=S * C).view(B, S, C)      # dS^T @ q
        return dq, dk, dv


def attention(q, k, v):
    if _attn_fused_ok(q):
        return FusedAttentionFn.apply(q, k, v)
    if _attn_fused_fwd_only_ok(q, k, v):
        return fused_attention_forward(q, k, v)
    return AttentionFn.apply(q, k, v)


# ----------------------------------------------------------------------------- embeddings
class FourierFn(torch.autograd.Function):
    """[z, sin(2^{6,7} 2pi z), cos(...), 0] -> 16 channels (ldm/model_vdm.py:341-343,812-829)"""

    @staticmethod
    def forward(ctx, z):
        z = _c(z)
        B = z.shape[0]
        out = torch.empty((B, HW, 16), device=z.device, dtype=torch.float32)
        call("mulan_fourier_fwd", ptr(z), ptr(out), B * HW, stream())
        ctx.save_for_backward(z)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, dout):
        (z,) = ctx.saved_tensors
        dout = _c(dout)
        dz = torch.empty_like(z)
        call("mulan_fourier_bwd", ptr(z), ptr(dout), ptr(dz), z.shape[0] * HW, 0, stream())
        return dz


def fourier_features(z):
    return FourierFn.apply(z)


class CondInputFn(torch.autograd.Function):
    """concat([timestep_embedding(t, E), conditioning]) -> [n, E + K]  (ldm/model_vdm.py:335-336).
    With rep > 1 the conditioning rows are broadcast `rep` times (ldm/ldm_unet.py:82-88)."""

    @staticmethod
    def forward(ctx, t, cond, E, rep):
        t, cond = _c(t), _c(cond)
        n, K = t.numel(), cond.shape[-1]
        out = torch.empty((n, E + K), device=t.device, dtype=torch.float32)
        call("mulan_temb_fwd", ptr(t), ptr(out), n, E, E + K, 0, stream())
        call("mulan_rowbcast", ptr(cond), ptr(out), n, K, rep, E + K, E, stream())
        ctx.save_for_backward(t)
        ctx.meta = (E, K, rep, cond.shape)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, dout):
        (t,) = ctx.saved_tensors
        E, K, rep, cshape = ctx.meta
        dout = _c(dout)
        n = t.numel()
        dt = dc = None
        if ctx.needs_input_grad[0]:
            dt = torch.empty_like(t)
            call("mulan_temb_bwd", ptr(t), ptr(dout), ptr(dt), n, E, E + K, 0, stream())
        if ctx.needs_input_grad[1]:
            dcr = dout[:, E:].contiguous()               # [n, K]
            dc = dcr if rep == 1 else colsum_raw(dcr, n // rep, rep, K)
            dc = dc.view(cshape)
        return dt, dc, None, None


def cond_input(t, cond, E, rep=1):
    return CondInputFn.apply(t, cond, E, rep)


class RowBcastFn(torch.autograd.Function):
    """y[r] = x[r // rep]: per-pixel broadcast of a per-sample vector (ldm/ldm_unet.py:85-87)"""

    @staticmethod
    def forward(ctx, x, rep):
        x = _c(x)
        n, K = x.shape
        y = torch.empty((n * rep, K), device=x.device, dtype=torch.float32)
        call("mulan_rowbcast", ptr(x), ptr(y), n * rep, K, rep, K, 0, stream())
        ctx.meta = (n, K, rep)
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, dy):
        n, K, rep = ctx.meta
        return colsum_raw(_c(dy), n, rep, K), None


def row_broadcast(x, rep):
    return RowBcastFn.apply(x, rep)


def encode_u8(x_u8):
    """EncDec.encode (ldm/model_vdm.py:274-280): uint8 [B, ...] -> fp32 in (-1, 1), same shape"""
    x_u8 = _c(x_u8)
    f = torch.empty(x_u8.shape, device=x_u8.device, dtype=torch.float32)
    call("mulan_encode_u8", ptr(x_u8), ptr(f), x_u8.numel(), stream())
    return f


# ----------------------------------------------------------------------------- MuLAN closed forms
class PolyGammaFn(torch.autograd.Function):
    """gamma_0, gamma_1, gamma_t, gamma'_t of NoiseSchedule_polynomial_fixedend
    (ldm/model_mulan_epsilon.py:514-555); gradients flow into (a, b, c) through gamma_t and gamma'_t."""

    @staticmethod
    def forward(ctx, a, b, c, t, gmin, gmax):
        a, b, c, t = _c(a), _c(b), _c(c), _c(t)
        B = a.shape[0]
        g0, g1, gt, gp = (torch.empty_like(a) for _ in range(4))
        call("mulan_poly_gamma_fwd", ptr(a), ptr(b), ptr(c), ptr(t), ptr(g0), ptr(g1), ptr(gt), ptr(gp), B, D,
             float(gmin), float(gmax), stream())
        ctx.save_for_backward(a, b, c, t)
        ctx.lim = (float(gmin), float(gmax))
        ctx.mark_non_differentiable(g0, g1)
        return g0, g1, gt, gp

    @staticmethod
    @once_differentiable
    def backward(ctx, _d0, _d1, dgt, dgp):
        a, b, c, t = ctx.saved_tensors
        B = a.shape[0]
        da, db, dc = (torch.empty_like(a) for _ in range(3))
        call("mulan_poly_gamma_bwd", ptr(a), ptr(b), ptr(c), ptr(t), ptr(_c(dgt)) if dgt is not None else None,
             ptr(_c(dgp)) if dgp is not None else None, ptr(da), ptr(db), ptr(dc), B, D, ctx.lim[0], ctx.lim[1],
             stream())
        return da, db, dc, None, None, None


def poly_gamma(a, b, c, t, gmin, gmax):
    return PolyGammaFn.apply(a, b, c, t, gmin, gmax)


class Expm1WeightFn(torch.autograd.Function):
    """w = T * expm1(gamma_t - gamma_s): discrete-time loss weight (ldm/model_mulan_epsilon.py:348-355)"""

    @staticmethod
    def forward(ctx, gt, gs, T):
        gt, gs = _c(gt), _c(gs)
        w = torch.empty_like(gt)
        call("mulan_expm1_weight_fwd", ptr(gt), ptr(gs), ptr(w), gt.numel(), float(T), stream())
        ctx.save_for_backward(gt, gs)
        ctx.T = float(T)
        return w

    @staticmethod
    @once_differentiable
    def backward(ctx, dw):
        gt, gs = ctx.saved_tensors
        dgt, dgs = torch.empty_like(gt), torch.empty_like(gs)
        call("mulan_expm1_weight_bwd", ptr(gt), ptr(gs), ptr(_c(dw)), ptr(dgt), ptr(dgs), gt.numel(), ctx.T, stream())
        return dgt, dgs, None


def expm1_weight(gt, gs, T):
    return Expm1WeightFn.apply(gt, gs, T)


class QSampleFn(torch.autograd.Function):
    """(z_t, mean gamma_t, loss_recon, loss_klz, var0, var1) from (x, gamma_0, gamma_1, gamma_t, eps0, eps)
    (ldm/model_mulan_velocity.py:208-236; ldm/model_vdm.py:119-151,274-303)."""

    @staticmethod
    def forward(ctx, x_u8, g0, g1, gt, eps0, eps):
        g0, g1, gt = _c(g0), _c(g1), _c(gt)
        B = x_u8.shape[0]
        per_elem = int(gt.numel() == B * D)
        dev = x_u8.device
        zt = torch.empty((B, D), device=dev, dtype=torch.float32)
        gbar, recon, klz, v0, v1 = (torch.empty(B, device=dev, dtype=torch.float32) for _ in range(5))
        call("mulan_qsample_fwd", ptr(x_u8), ptr(g0), ptr(g1), ptr(gt), per_elem, ptr(eps0), ptr(eps), ptr(zt),
             ptr(gbar), ptr(recon), ptr(klz), ptr(v0), ptr(v1), B, D, stream())
        ctx.save_for_backward(x_u8, g0, g1, gt, eps0, eps)
        ctx.per_elem = per_elem
        ctx.mark_non_differentiable(v0, v1)
        return zt, gbar, recon, klz, v0, v1

    @staticmethod
    @once_differentiable
    def backward(ctx, dzt, dgbar, drecon, dklz, _dv0, _dv1):
        x, g0, g1, gt, eps0, eps = ctx.saved_tensors
        B = x.shape[0]
        dev = x.device
        need0, need1 = ctx.needs_input_grad[1], ctx.needs_input_grad[2]
        dzt = _c(dzt) if dzt is not None else torch.zeros((B, D), device=dev)
        dgt = torch.empty((B, D), device=dev, dtype=torch.float32)
        dg0 = torch.empty((B, D), device=dev, dtype=torch.float32) if need0 else None
        dg1 = torch.empty((B, D), device=dev, dtype=torch.float32) if need1 else None
        zero = None
        if (need0 and drecon is None) or (need1 and dklz is None):
            zero = torch.zeros(B, device=dev)
        call("mulan_qsample_bwd", ptr(x), ptr(g0), ptr(g1), ptr(gt), ctx.per_elem, ptr(eps0), ptr(eps), ptr(dzt),
             ptr(_c(dgbar)) if dgbar is not None else None,
             ptr(_c(drecon) if drecon is not None else zero) if need0 else None,
             ptr(_c(dklz) if dklz is not None else zero) if need1 else None,
             ptr(dgt), ptr(dg0), ptr(dg1), B, D, stream())
        if not ctx.per_elem:   # scalar schedule: reduce the per-element gradients to per-sample
            dgt = colsum_raw(dgt.view(B, D, 1), B, D, 1).view(gt.shape)
            dg0 = colsum_raw(dg0.view(B, D, 1), B, D, 1).view(g0.shape) if need0 else None
            dg1 = colsum_raw(dg1.view(B, D, 1), B, D, 1).view(g1.shape) if need1 else None
        else:
            dgt = dgt.view(gt.shape)
        return None, dg0, dg1, dgt, None, None


def qsample(x_u8, g0, g1, gt, eps0, eps):
    return QSampleFn.apply(x_u8, g0, g1, gt, eps0, eps)


class DiffLossFn(torch.autograd.Function):
    """loss_diff[B].  mode 0 velocity, 1 velocity_from_epsilon, 2 epsilon
    (ldm/model_mulan_velocity.py:246-260; ldm/model_mulan_epsilon.py:338-355; ldm/model_vdm.py:156-170)."""

    @staticmethod
    def forward(ctx, mode, x_u8, gt, gp, eps, zt, net):
        gt, gp, zt, net = _c(gt), _c(gp), _c(zt), _c(net)
        B = x_u8.shape[0]
        per_elem = int(gt.numel() == B * D)
        loss = torch.empty(B, device=x_u8.device, dtype=torch.float32)
        call("mulan_diffloss_fwd", mode, ptr(x_u8), ptr(gt), ptr(gp), per_elem, ptr(eps), ptr(zt), ptr(net),
             ptr(loss), B, D, stream())
        ctx.save_for_backward(x_u8, gt, gp, eps, zt, net)
        ctx.meta = (mode, per_elem)
        return loss

    @staticmethod
    @once_differentiable
    def backward(ctx, dloss):
        x, gt, gp, eps, zt, net = ctx.saved_tensors
        mode, per_elem = ctx.meta
        B = x.shape[0]
        dev = x.device
        dnet, dgt, dgp = (torch.empty((B, D), device=dev, dtype=torch.float32) for _ in range(3))
        dzt = torch.empty((B, D), device=dev, dtype=torch.float32) if mode == 1 else None
        call("mulan_diffloss_bwd", mode, ptr(x), ptr(gt), ptr(gp), per_elem, ptr(eps), ptr(zt), ptr(net),
             ptr(_c(dloss)), ptr(dnet), ptr(dgt), ptr(dgp), ptr(dzt), B, D, stream())
        if not per_elem:
            dgt = colsum_raw(dgt.view(B, D, 1), B, D, 1).view(gt.shape)
            dgp = colsum_raw(dgp.view(B, D, 1), B, D, 1).view(gp.shape)
        else:
            dgt, dgp = dgt.view(gt.shape), dgp.view(gp.shape)
        return None, None, dgt, dgp, None, (dzt.view(zt.shape) if dzt is not None else None), dnet.view(net.shape)


def diffusion_loss(mode, x_u8, gt, gp, eps, zt, net):
    return DiffLossFn.apply(mode, x_u8, gt, gp, eps, zt, net)


class TopKFn(torch.autograd.Function):
    """(embedding, kl_z) = relaxed top-k straight-through latent (ldm/model_mulan_velocity.py:78-120)."""

    @staticmethod
    def forward(ctx, logits, gnoise, k, tau):
        logits, gnoise = _c(logits), _c(gnoise)
        B, L = logits.shape
        emb, soft = torch.empty_like(logits), torch.empty_like(logits)
        kl = torch.empty(B, device=logits.device, dtype=torch.float32)
        nrm = torch.empty_like(kl)
        call("mulan_topk_fwd", ptr(logits), ptr(gnoise), ptr(emb), ptr(kl), ptr(soft), ptr(nrm), B, L, int(k),
             float(tau), stream())
        ctx.save_for_backward(logits, soft, nrm)
        return emb, kl

    @staticmethod
    @once_differentiable
    def backward(ctx, demb, dkl):
        logits, soft, nrm = ctx.saved_tensors
        B, L = logits.shape
        demb = _c(demb) if demb is not None else torch.zeros_like(logits)
        dkl = _c(dkl) if dkl is not None else torch.zeros(B, device=logits.device)
        dl = torch.empty_like(logits)
        call("mulan_topk_bwd", ptr(logits), ptr(soft), ptr(nrm), ptr(demb), ptr(dkl), ptr(dl), B, L, stream())
        return dl, None, None, None


def topk_embedding(logits, gnoise, k, tau=10.0):
    return TopKFn.apply(logits, gnoise, k, tau)


class GumbelLatentFn(torch.autograd.Function):
    """(embedding, kl_z) = straight-through Gumbel-softmax one-hot latent (ldm/model_mulan_velocity.py:68-92).
    tau: 0-dim fp32 device tensor, read by the kernels when they run (a stream-ordered parameter under graph replay)."""

    @staticmethod
    def forward(ctx, logits, gnoise, tau):
        logits, gnoise = _c(logits), _c(gnoise)
        B, L = logits.shape
        emb, soft = torch.empty_like(logits), torch.empty_like(logits)
        kl = torch.empty(B, device=logits.device, dtype=torch.float32)
        call("mulan_gumbel_latent_fwd", ptr(logits), ptr(gnoise), ptr(tau), ptr(emb), ptr(kl), ptr(soft), B, L, stream())
        ctx.save_for_backward(logits, soft, tau)
        return emb, kl

    @staticmethod
    @once_differentiable
    def backward(ctx, demb, dkl):
        logits, soft, tau = ctx.saved_tensors
        B, L = logits.shape
        demb = _c(demb) if demb is not None else torch.zeros_like(logits)
        dkl = _c(dkl) if dkl is not None else torch.zeros(B, device=logits.device)
        dl = torch.empty_like(logits)
        call("mulan_gumbel_latent_bwd", ptr(logits), ptr(soft), ptr(tau), ptr(demb), ptr(dkl), ptr(dl), B, L, stream())
        return dl, None, None


def gumbel_embedding(logits, gnoise, tau):
    """tau: 0-dim fp32 tensor on the logits' device"""
    if not (torch.is_tensor(tau) and tau.dtype == torch.float32 and tau.numel() == 1 and tau.device == logits.device):
        raise TypeError("gumbel_embedding: tau must be a one-element fp32 tensor on the logits' device")
    return GumbelLatentFn.apply(logits, gnoise, _c(tau))


class GaussianLatentFn(torch.autograd.Function):
    """(embedding, kl_z) = mu + sqrt(softplus(s)) eps_z and its KL to N(0, I) (ldm/model_mulan_velocity.py:132-138 with
    the softplus of UnetEncoderGaussian, ldm/model_mulan_epsilon.py:80)."""

    @staticmethod
    def forward(ctx, mu, s, eps_z):
        mu, s, eps_z = _c(mu), _c(s), _c(eps_z)
        B, L = mu.shape
        emb = torch.empty_like(mu)
        kl = torch.empty(B, device=mu.device, dtype=torch.float32)
        call("mulan_gaussian_latent_fwd", ptr(mu), ptr(s), ptr(eps_z), ptr(emb), ptr(kl), B, L, stream())
        ctx.save_for_backward(mu, s, eps_z)
        return emb, kl

    @staticmethod
    @once_differentiable
    def backward(ctx, demb, dkl):
        mu, s, eps_z = ctx.saved_tensors
        B, L = mu.shape
        demb = _c(demb) if demb is not None else torch.zeros_like(mu)
        dkl = _c(dkl) if dkl is not None else torch.zeros(B, device=mu.device)
        dmu, ds = torch.empty_like(mu), torch.empty_like(s)
        call("mulan_gaussian_latent_bwd", ptr(mu), ptr(s), ptr(eps_z), ptr(demb), ptr(dkl), ptr(dmu), ptr(ds), B, L,
             stream())
        return dmu, ds, None


def gaussian_embedding(mu, s, eps_z):
    """s: the pre-softplus head of the Gaussian encoder"""
    return GaussianLatentFn.apply(mu, s, eps_z)


# ----------------------------------------------------------------------------- optimiser
def adamw_ema_step(p, g, m, v, ema, n_decay, lr, b1, b2, eps, wd, step, ema_rate, grad_scale=1.0, clip_norm=None, dyn=None):
    """one AdamW + EMA step on the flat buffers; clip_norm: optax.clip_by_global_norm in front (the factor is
    computed and applied on the device).  Returns the [2] device tensor (factor, gradient norm) when clipping.
    dyn: optional fp32 device tensor [lr, 1 - b1^t, 1 - b2^t] read by the kernel when it runs (graph replay); lr / step
    are ignored then."""
    if dyn is not None:
        out = None
        if clip_norm is not None:
            ws = torch.empty(lib.load().mulan_global_norm_clip_workspace() // 8, device=p.device, dtype=torch.float64)
            out = torch.empty(2, device=p.device, dtype=torch.float32)
            call("mulan_global_norm_clip", ptr(g), g.numel(), float(clip_norm), float(grad_scale), ptr(ws), ptr(out), stream())
        call("mulan_adamw_ema_step_dyn", ptr(p), ptr(g), ptr(m), ptr(v), ptr(ema), p.numel(), int(n_decay), float(b1),
             float(b2), float(eps), float(wd), float(ema_rate), float(grad_scale), ptr(out), ptr(dyn), stream())
        return out
    if clip_norm is None:
        call("mulan_adamw_ema_step", ptr(p), ptr(g), ptr(m), ptr(v), ptr(ema), p.numel(), int(n_decay), float(lr),
             float(b1), float(b2), float(eps), float(wd), int(step), float(ema_rate), float(grad_scale), stream())
        return None
    ws = torch.empty(lib.load().mulan_global_norm_clip_workspace() // 8, device=p.device, dtype=torch.float64)
    out = torch.empty(2, device=p.device, dtype=torch.float32)
    call("mulan_global_norm_clip", ptr(g), g.numel(), float(clip_norm), float(grad_scale), ptr(ws), ptr(out), stream())
    call("mulan_adamw_ema_step_scaled", ptr(p), ptr(g), ptr(m), ptr(v), ptr(ema), p.numel(), int(n_decay), float(lr),
         float(b1), float(b2), float(eps), float(wd), int(step), float(ema_rate), float(grad_scale), ptr(out), stream())
    return out


# ----------------------------------------------------------------------------- ancestral sampler (eval only)
def ancestral_step(zt, net, gt, gs, eps, mode):
    """one reverse step z_t -> z_s (mulan_ancestral_step); mode 0: net is the velocity, 1: net is eps_hat; gt / gs per
    element ([B,3072]) or per sample ([B])"""
    zt, net, gt, gs, eps = _c(zt), _c(net), _c(gt), _c(gs), _c(eps)
    zs = torch.empty_like(zt)
    per = zt.numel() // gt.numel()
    call("mulan_ancestral_step", ptr(zt), ptr(net), ptr(gt), ptr(gs), ptr(eps), ptr(zs), zt.numel(), int(mode),
         0 if per == 1 else per, stream())
    return zs


def fast_sampler_step(zt, net, gt, gs, mode, gprev=None, xprev=None, x0=True):
    """one deterministic step z_t -> z_s of DDIM (gprev = xprev = None) or DPM-Solver++(2M) (mulan_fast_sampler_step);
    mode 0: net is the velocity, 1: eps_hat, 2: x_hat; gt / gs / gprev per element ([B,3072]) or per sample ([B]).
    Returns (z_s, x_hat_t) (x_hat_t None when x0=False)"""
    if (gprev is None) != (xprev is None):
        raise ValueError("fast_sampler_step: gprev and xprev go together (both None: first order)")
    zt, net, gt, gs = _c(zt), _c(net), _c(gt), _c(gs)
    gprev, xprev = (None, None) if gprev is None else (_c(gprev), _c(xprev))
    zs = torch.empty_like(zt)
    xh = torch.empty_like(zt) if x0 else None
    per = zt.numel() // gt.numel()
    call("mulan_fast_sampler_step", ptr(zt), ptr(net), ptr(gt), ptr(gs), ptr(gprev), ptr(xprev), ptr(zs), ptr(xh),
         zt.numel(), int(mode), 0 if per == 1 else per, stream())
    return zs, xh


def stochastic_sampler_step(z, net, g_t, g_s, mode, xi, eta, g_prev=None, x_prev=None):
    """one step z_t -> z_s of DDIM with eta in [0, 1] (g_prev = x_prev = None) or, at second order, of its 2M form:
    SDE-DPM-Solver++(2M) at eta = 1 (mulan_stochastic_sampler_step).  xi: one standard normal per element, shaped like
    z; mode and the gamma layouts as fast_sampler_step.  Returns (z_s, x_hat_t)"""
    if (g_prev is None) != (x_prev is None):
        raise ValueError("stochastic_sampler_step: g_prev and x_prev go together (both None: first order)")
    eta = float(eta)
    if not 0.0 <= eta <= 1.0:
        raise ValueError(f"stochastic_sampler_step: eta must lie in [0, 1], got {eta!r}")
    if xi is None or xi.numel() != z.numel():
        raise ValueError("stochastic_sampler_step: xi must hold one standard normal per element of z")
    z, net, g_t, g_s, xi = _c(z), _c(net), _c(g_t), _c(g_s), _c(xi)
    g_prev, x_prev = (None, None) if g_prev is None else (_c(g_prev), _c(x_prev))
    zs, xh = torch.empty_like(z), torch.empty_like(z)
    per = z.numel() // g_t.numel()
    call("mulan_stochastic_sampler_step", ptr(z), ptr(net), ptr(g_t), ptr(g_s), ptr(g_prev), ptr(x_prev), ptr(xi), eta,
         ptr(zs), ptr(xh), z.numel(), int(mode), 0 if per == 1 else per, stream())
    return zs, xh


def inpaint_mix(z, x, mask, g, xi=None, out=None):
    """the known sub-pixels of a sampler state z replaced by their q(z_t | x) (mulan_inpaint_mix):
    mask ? alpha(g) x + sigma(g) xi : z.  x: the known image as encode_u8 gives it, shaped like z; mask: uint8 (or
    bool), one byte per element, non-zero = known; g per element or per sample ([B]); xi: one standard normal per
    element, None = zeros (a known element is then exactly alpha x).  Returns a new tensor shaped like z (out: the
    tensor to write, which may be z)"""
    if x.numel() != z.numel() or mask.numel() != z.numel() or (xi is not None and xi.numel() != z.numel()):
        raise ValueError("inpaint_mix: x, mask and xi hold one value per element of z")
    if mask.dtype == torch.bool:
        mask = mask.view(torch.uint8) if mask.is_contiguous() else mask.to(torch.uint8)
    if mask.dtype != torch.uint8:
        raise ValueError(f"inpaint_mix: the mask is bool or uint8, got {mask.dtype}")
    if g.numel() == 0 or z.numel() % g.numel():
        raise ValueError("inpaint_mix: gamma is per element or per sample")
    z, x, mask, g = _c(z), _c(x), _c(mask), _c(g)
    xi = None if xi is None else _c(xi)
    if out is None:
        out = torch.empty_like(z)
    elif (out.shape != z.shape or out.dtype != torch.float32 or out.device != z.device or not out.is_contiguous()):
        raise ValueError("inpaint_mix: out is a contiguous fp32 tensor shaped like z, on its device")
    per = z.numel() // g.numel()
    call("mulan_inpaint_mix", ptr(z), ptr(x), ptr(mask), ptr(g), ptr(xi), ptr(out), z.numel(), 0 if per == 1 else per,
         stream())
    return out


def forward_jump(z_s, g_s, g_t, xi):
    """z_t ~ q(z_t | z_s) for g_t >= g_s on the noise xi (mulan_forward_jump):
    sqrt(sigmoid(-g_t) / sigmoid(-g_s)) z_s + sqrt(sigmoid(g_t) (1 - e^(g_s - g_t))) xi; gamma per element or per
    sample ([B]); xi: one standard normal per element.  Returns a new tensor shaped like z_s"""
    if xi is None or xi.numel() != z_s.numel():
        raise ValueError("forward_jump: xi must hold one standard normal per element of z_s")
    if g_s.numel() == 0 or g_s.numel() != g_t.numel() or z_s.numel() % g_s.numel():
        raise ValueError("forward_jump: gamma is per element or per sample, the same layout at s and at t")
    z_s, g_s, g_t, xi = _c(z_s), _c(g_s), _c(g_t), _c(xi)
    z_t = torch.empty_like(z_s)
    per = z_s.numel() // g_s.numel()
    call("mulan_forward_jump", ptr(z_s), ptr(g_s), ptr(g_t), ptr(xi), ptr(z_t), z_s.numel(), 0 if per == 1 else per,
         stream())
    return z_t


RESTORE_FACTORS = (2, 4, 8, 16)


def restore_y_shape(B, H, W, C, f, gray):
    """shape of the measurement y = A x of the degradation (f, gray) on B images [H, W, C] (mulan_restore_project):
    f x f average pooling per channel (f in RESTORE_FACTORS; 1: none, with gray only), then the channel mean if gray"""
    gray = bool(gray)
    if isinstance(f, bool) or int(f) != f or not (f in RESTORE_FACTORS or (f == 1 and gray)):
        raise ValueError(f"restore: the factor is one of {RESTORE_FACTORS} (or 1 with gray), got f = {f!r}, gray = {gray}")
    if min(B, H, W, C) < 1 or H % f or W % f:
        raise ValueError(f"restore: f = {f} must divide H = {H} and W = {W}, and no extent may be zero (B = {B}, C = {C})")
    return (B, H // f, W // f, 1 if gray else C)


def _restore_dims(x, hwc, name):
    if hwc is None:
        if x.dim() != 4:
            raise ValueError(f"{name}: an input that is not [B, H, W, C] needs hwc = (H, W, C)")
        return tuple(x.shape)
    H, W, C = (int(v) for v in hwc)
    if min(H, W, C) < 1 or x.numel() == 0 or x.numel() % (H * W * C):
        raise ValueError(f"{name}: {x.numel()} elements are no batch of [{H}, {W}, {C}] images")
    return (x.numel() // (H * W * C), H, W, C)


def restore_measure(x, f, gray, hwc=None):
    """y = A x (mulan_restore_measure): the group means of the degradation (f, gray), fp32 shaped restore_y_shape.
    x: fp32 [B, H, W, C], or any shape holding B images with hwc = (H, W, C)"""
    _chk(x, "restore_measure: x")
    B, H, W, C = _restore_dims(x, hwc, "restore_measure")
    y = torch.empty(restore_y_shape(B, H, W, C, f, gray), device=x.device, dtype=torch.float32)
    call("mulan_restore_measure", ptr(_c(x)), ptr(y), B, H, W, C, int(f), int(bool(gray)), stream())
    return y


def restore_project(z, net, g_t, y, f, gray, mode, hwc=None, out=None):
    """x_hat' = x_hat + A+ (y - A x_hat) (mulan_restore_project): x_hat formed from (z, net, g_t) as fast_sampler_step
    forms it for `mode` (0: net is the velocity, 1: eps_hat, 2: x_hat, and z is not used), projected onto the measurement
    y (fp32, restore_y_shape elements) of the degradation (f, gray).  z: fp32 [B, H, W, C], or any shape holding B images
    with hwc = (H, W, C); g_t per element or per sample ([B]).  Returns a new tensor shaped like z (out: the tensor to
    write, which may be z or net)"""
    for t, name in ((z, "z"), (net, "net"), (g_t, "g_t"), (y, "y")):
        if not torch.is_tensor(t):
            raise ValueError(f"restore_project: {name} is a tensor, got {type(t).__name__}")
        _chk(t, f"restore_project: {name}")
    if mode not in (0, 1, 2):
        raise ValueError(f"restore_project: mode is 0 (velocity), 1 (eps_hat) or 2 (x_hat), got {mode!r}")
    B, H, W, C = _restore_dims(z, hwc, "restore_project")
    if net.numel() != z.numel():
        raise ValueError("restore_project: net holds one value per element of z")
    if g_t.numel() not in (B, z.numel()):
        raise ValueError("restore_project: gamma is per element or per sample")
    ys = restore_y_shape(B, H, W, C, f, gray)
    if y.numel() != math.prod(ys):
        raise ValueError(f"restore_project: the measurement holds {list(ys)} values, got {list(y.shape)}")
    z, net, g_t, y = _c(z), _c(net), _c(g_t), _c(y)
    if out is None:
        out = torch.empty_like(z)
    elif out.shape != z.shape or out.dtype != torch.float32 or out.device != z.device or not out.is_contiguous():
        raise ValueError("restore_project: out is a contiguous fp32 tensor shaped like z, on its device")
    per = 0 if g_t.numel() == z.numel() else H * W * C
    call("mulan_restore_project", ptr(z), ptr(net), ptr(g_t), ptr(y), ptr(out), B, H, W, C, int(f), int(bool(gray)),
         int(mode), per, stream())
    return out


def decode_argmax(z0, g0):
    """uint8 argmax over the 256 decoder bins at z_0 / sqrt(1 - sigmoid(g_0)) (VDM.generate_x, sample_softmax=False)"""
    z0, g0 = _c(z0), _c(g0)
    out = torch.empty(z0.shape, device=z0.device, dtype=torch.uint8)
    per = z0.numel() // g0.numel()
    call("mulan_decode_argmax", ptr(z0), ptr(g0), ptr(out), z0.numel(), 0 if per == 1 else per, stream())
    return out


def decode_logprobs(z, g0):
    """[..., 256] decoder log-probabilities of every element of z (EncDec.decode, ldm/model_vdm.py:282-296); g0 per
    element or one value per sample (broadcast over the trailing elements)"""
    z, g0 = _c(z.to(torch.float32)), _c(g0.to(torch.float32))
    out = torch.empty(tuple(z.shape) + (256,), device=z.device, dtype=torch.float32)
    per = z.numel() // g0.numel()
    call("mulan_decode_logprobs", ptr(z), ptr(g0), ptr(out), z.numel(), 0 if per == 1 else per, stream())
    return out


def decode_sample(z0, g0, seed, offset=0):
    """uint8 categorical draw over the 256 decoder bins (VDM.generate_x with sample_softmax=True)"""
    z0, g0 = _c(z0), _c(g0)
    out = torch.empty(z0.shape, device=z0.device, dtype=torch.uint8)
    per = z0.numel() // g0.numel()
    call("mulan_decode_sample", ptr(z0), ptr(g0), ptr(out), z0.numel(), 0 if per == 1 else per,
         int(seed) & (2**64 - 1), int(offset), stream())
    return out


def rowmean(x):
    x = _c(x)
    rows = x.shape[0]
    out = torch.empty(rows, device=x.device, dtype=torch.float32)
    call("mulan_rowmean", ptr(x), ptr(out), rows, x.numel() // rows, stream())
    return out


def schedule_moments(a, b, c):
    """fp32 [B, 5]: per sample the means over its 3072 sub-pixels of (c^2, b c, (b^2 + 2 a c) / 3, a b / 2, a^2 / 5) / S,
    the coefficients of t .. t^5 in the sample's mean schedule (gamma_bar - gamma_min) / (gamma_max - gamma_min)
    (mulan_schedule_moments); a, b, c fp32 [B, 3072], the coefficients of the polynomial schedule"""
    a, b, c = _c(a), _c(b), _c(c)
    if not (a.dtype == b.dtype == c.dtype == torch.float32) or a.dim() != 2 or a.shape[1] != D \
            or b.shape != a.shape or c.shape != a.shape:
        raise ValueError(f"schedule_moments: a, b, c are fp32 [B, {D}]; got {[tuple(x.shape) for x in (a, b, c)]}")
    m = torch.empty((a.shape[0], 5), device=a.device, dtype=torch.float32)
    call("mulan_schedule_moments", ptr(a), ptr(b), ptr(c), a.shape[0], D, ptr(m), stream())
    return m


def schedule_invert(m, targets, gmin, gmax):
    """fp32 [M]: the times t in [0, 1] at which the mean schedule of the batch, gamma_bar(t) = gmin + (gmax - gmin)
    sum_k mean_b(m[b, k]) t^(k + 1), takes the values `targets` (float64 [M], any array or tensor; a target >= gmax
    gives exactly 1, one <= gmin exactly 0); m fp32 [B, 5] from schedule_moments (mulan_schedule_invert)"""
    m = _c(m)
    if m.dtype != torch.float32 or m.dim() != 2 or m.shape[1] != 5 or m.shape[0] < 1:
        raise ValueError(f"schedule_invert: m is fp32 [B, 5]; got {m.dtype} {tuple(m.shape)}")
    tg = torch.as_tensor(targets, dtype=torch.float64).reshape(-1).to(m.device).contiguous()
    if tg.numel() < 1:
        raise ValueError("schedule_invert: no target")
    out = torch.empty(tg.numel(), device=m.device, dtype=torch.float32)
    call("mulan_schedule_invert", ptr(m), m.shape[0], ptr(tg), tg.numel(), float(gmin), float(gmax), ptr(out), stream())
    return out


def schedule_curves(a, b, c, t, gmin, gmax, *, curves=True, stats=False, bins=None):
    """(gamma | None, stats | None, hist | None) of E embeddings at the T times of `t` (fp32 [T], any order), one launch
    (mulan_schedule_curves); a, b, c fp32 [E, 3072].  curves: gamma fp32 [E, T, 3072].  stats: fp32 [E, T, 8] over the
    sub-pixels -- mean, population standard deviation, min, max, the three channel means, the mean of sigmoid(gamma).
    bins (1..256): int32 [E, T, bins], the histogram over [gmin, gmax] in `bins` equal bins.  Without curves none is
    written."""
    a, b, c, t = _c(a), _c(b), _c(c), _c(t)
    if not (a.dtype == b.dtype == c.dtype == torch.float32) or a.dim() != 2 or a.shape[1] != D or a.shape[0] < 1 \
            or b.shape != a.shape or c.shape != a.shape:
        raise ValueError(f"schedule_curves: a, b, c are fp32 [E, {D}]; got {[tuple(x.shape) for x in (a, b, c)]}")
    if t.dtype != torch.float32 or t.dim() != 1 or t.numel() < 1 or t.device != a.device:
        raise ValueError(f"schedule_curves: t is an fp32 [T] tensor on {a.device}; got {t.dtype} {tuple(t.shape)}")
    if not (curves or stats or bins is not None):
        raise ValueError("schedule_curves: nothing asked for (curves, stats and bins are all off)")
    if bins is not None and not 1 <= int(bins) <= 256:
        raise ValueError(f"schedule_curves: bins lies in 1..256, got {bins}")
    if not float(gmin) < float(gmax):
        raise ValueError(f"schedule_curves: gmin < gmax, got {gmin}, {gmax}")
    E, T = a.shape[0], t.numel()
    gamma = torch.empty((E, T, D), device=a.device, dtype=torch.float32) if curves else None
    st = torch.empty((E, T, 8), device=a.device, dtype=torch.float32) if stats else None
    hist = torch.empty((E, T, int(bins)), device=a.device, dtype=torch.int32) if bins is not None else None
    call("mulan_schedule_curves", ptr(a), ptr(b), ptr(c), E, D, ptr(t), T, float(gmin), float(gmax), ptr(gamma), ptr(st),
         ptr(hist), int(bins) if bins is not None else 0, stream())
    return gamma, st, hist


def bound_profile(mode, x, g0, g1, gt, w, eps0, eps, zt, net, rows_per_group, rows=True, cols=True):
    """(rows | None, cols | None): the loss heads of B rows kept per element long enough to be reduced both ways, one
    entry point (mulan_bound_profile).  mode, x (uint8 [B, 3072]), gt, w, eps, zt, net as diffusion_loss takes them (w its
    `gp`: gamma'(t), or expm1_weight), g0, g1, eps0 as qsample takes them; the four gammas fp32 [B, 3072], or all [B]
    (the scalar schedule).  Rows g R .. g R + R - 1 form group g, R = rows_per_group.
    rows: fp32 [B, 8] -- the sum of the diffusion term d, its three channel sums (sub-pixel i is channel i % 3), the sums
    of the reconstruction and the prior-KL term, the sum of the squared residual, the mean of the factor of r^2 / 2 in d.
    cols: fp32 [G, 3, 3072] -- per group, the row means of d, the reconstruction and the prior-KL term per sub-pixel."""
    if mode not in (0, 1, 2):
        raise ValueError(f"bound_profile: mode is 0 (velocity), 1 (velocity from epsilon) or 2 (epsilon), got {mode!r}")
    if not torch.is_tensor(x) or x.dtype != torch.uint8 or x.dim() != 2 or x.shape[1] != D or x.shape[0] < 1:
        raise ValueError(f"bound_profile: x is uint8 [B, {D}]; got "
                         f"{(x.dtype, tuple(x.shape)) if torch.is_tensor(x) else type(x).__name__}")
    B = x.shape[0]
    wide = {"eps0": eps0, "eps": eps, "zt": zt, "net": net}
    gammas = {"g0": g0, "g1": g1, "gt": gt, "w": w}
    for name, v in {**wide, **gammas}.items():
        if not torch.is_tensor(v) or v.dtype != torch.float32 or v.device != x.device:
            raise ValueError(f"bound_profile: {name} is an fp32 tensor on {x.device}; got "
                             f"{(v.dtype, v.device) if torch.is_tensor(v) else type(v).__name__}")
    for name, v in wide.items():
        if tuple(v.shape) != (B, D):
            raise ValueError(f"bound_profile: {name} is fp32 [{B}, {D}]; got {tuple(v.shape)}")
    per_elem = tuple(gt.shape) == (B, D)
    for name, v in gammas.items():
        if tuple(v.shape) != ((B, D) if per_elem else (B,)):
            raise ValueError(f"bound_profile: g0, g1, gt, w are all [{B}, {D}] or all [{B}]; {name} is {tuple(v.shape)}")
    R = int(rows_per_group)
    if R < 1 or B % R:
        raise ValueError(f"bound_profile: {B} rows are no whole number of groups of rows_per_group = {rows_per_group}")
    if not (rows or cols):
        raise ValueError("bound_profile: nothing asked for (rows and cols are both off)")
    x, g0, g1, gt, w, eps0, eps, zt, net = (_c(v) for v in (x, g0, g1, gt, w, eps0, eps, zt, net))
    dev = x.device
    rows_out = torch.empty((B, 8), device=dev, dtype=torch.float32) if rows else None
    cols_out = ws = None
    if cols:
        cols_out = torch.empty((B // R, 3, D), device=dev, dtype=torch.float32)
        ws = torch.empty(lib.load().mulan_bound_profile_workspace(B, R) // 4, device=dev, dtype=torch.float32)
    call("mulan_bound_profile", int(mode), ptr(x), ptr(g0), ptr(g1), ptr(gt), ptr(w), int(per_elem), ptr(eps0), ptr(eps),
         ptr(zt), ptr(net), ptr(rows_out), ptr(cols_out), ptr(ws), B, D, R, stream())
    return rows_out, cols_out


KNN_MAX_K = 16
KNN_EMPTY = (2 ** 31 - 1, -1)      # (dist2, idx) of a slot no reference qualified for


def knn_check(q, r, k, idx_base=0, self_offset=-1, out=None, radius2=None, covered=None, splits=0):
    """every check of knn_u8 that needs no library call; q, r: anything with dtype, shape (and, for tensors, device)"""
    for name, v in (("q", q), ("r", r)):
        if not hasattr(v, "dtype") or str(v.dtype) not in ("torch.uint8", "uint8") or len(v.shape) != 2 or v.shape[0] < 1:
            raise ValueError(f"knn_u8: {name} is uint8 [rows >= 1, D]; got "
                             f"{(v.dtype, tuple(v.shape)) if hasattr(v, 'dtype') else type(v).__name__}")
    Q, D = q.shape
    N = r.shape[0]
    if r.shape[1] != D:
        raise ValueError(f"knn_u8: q has D = {D}, r has D = {r.shape[1]}")
    if D % 64 or not 64 <= D <= 16384:
        raise ValueError(f"knn_u8: D is a multiple of 64 in [64, 16384], got {D}")
    if isinstance(k, bool) or not isinstance(k, int) or not 1 <= k <= KNN_MAX_K:
        raise ValueError(f"knn_u8: k is an int in [1, {KNN_MAX_K}], got {k!r}")
    if idx_base < 0 or idx_base + N > 2 ** 31 - 1:
        raise ValueError(f"knn_u8: idx_base >= 0 and idx_base + N <= 2^31 - 1, got idx_base = {idx_base}, N = {N}")
    if self_offset < -1:
        raise ValueError(f"knn_u8: self_offset is -1 (none) or >= 0, got {self_offset}")
    if not 0 <= splits <= 4096:
        raise ValueError(f"knn_u8: splits is 0 (the library chooses) or in [1, 4096], got {splits}")
    if covered is not None and radius2 is None:
        raise ValueError("knn_u8: covered is an output of the radius mode and needs radius2")
    if radius2 is not None and (not torch.is_tensor(radius2) or radius2.dtype != torch.int32 or tuple(radius2.shape) != (N,)):
        raise ValueError(f"knn_u8: radius2 is int32 [{N}]")
    if covered is not None and (not torch.is_tensor(covered) or covered.dtype != torch.uint8 or tuple(covered.shape) != (Q,)):
        raise ValueError(f"knn_u8: covered is uint8 [{Q}]")
    if out is not None:
        if not isinstance(out, (tuple, list)) or len(out) != 2:
            raise ValueError("knn_u8: out is the pair (dist2, idx) of an earlier call")
        for name, v in zip(("dist2", "idx"), out):
            if not torch.is_tensor(v) or v.dtype != torch.int32 or tuple(v.shape) != (Q, k) or not v.is_contiguous():
                raise ValueError(f"knn_u8: out's {name} is a contiguous int32 [{Q}, {k}]")
    return Q, N, D


def knn_u8(q, r, k, idx_base=0, self_offset=-1, out=None, radius2=None, covered=None, splits=0):
    """(dist2, idx), int32 [Q, k]: for every row of q (uint8 [Q, D]) the k smallest squared Euclidean distances to the rows of
    r (uint8 [N, D]), ascending, and the rows' indices + idx_base; exact integers from the int8 matrix cores
    (mulan_knn_u8).  Equal distances go to the smaller index; slots no reference qualified for hold KNN_EMPTY.
    self_offset >= 0 leaves out the pair with j + idx_base == i + self_offset.  out = (dist2, idx) of earlier calls:
    this call's references are merged into those lists, in place (a reference set walked in chunks).
    radius2 (int32 [N]): also returns covered (uint8 [Q]), 1 where some qualifying j has d2(i, j) <= radius2[j]; a
    `covered` passed in is OR-ed into (only together with out, or it is overwritten).  splits: slices of the reference
    range, 0 for the library's choice; the result does not depend on it."""
    Q, N, D = knn_check(q, r, k, idx_base, self_offset, out, radius2, covered, splits)
    if not torch.is_tensor(q) or not torch.is_tensor(r) or q.device != r.device:
        raise ValueError("knn_u8: q and r are tensors on one device")
    dev = q.device
    for name, v in (("radius2", radius2), ("covered", covered), ("dist2", out and out[0]), ("idx", out and out[1])):
        if v is not None and v.device != dev:
            raise ValueError(f"knn_u8: {name} is on {v.device}, q on {dev}")
    q, r, radius2 = _c(q), _c(r), _c(radius2)
    accumulate = out is not None
    dist2, idx = out if accumulate else (torch.empty((Q, k), device=dev, dtype=torch.int32) for _ in range(2))
    if radius2 is not None and covered is None:
        covered = torch.zeros(Q, device=dev, dtype=torch.uint8)
    ws = torch.empty(lib.load().mulan_knn_u8_workspace(Q, k, int(splits)) // 8 + 1, device=dev, dtype=torch.int64)
    call("mulan_knn_u8", ptr(q), ptr(r), Q, N, D, k, int(idx_base), int(self_offset), int(accumulate), int(splits),
         ptr(radius2), ptr(covered), ptr(dist2), ptr(idx), ptr(ws), stream())
    return (dist2, idx) if radius2 is None else (dist2, idx, covered)


MOMENTS_MAX_D = 4096               # mulan_set_moments_u8: D a multiple of 64 in [64, 4096], at most 2^24 rows per call
MOMENTS_MAX_N = 2 ** 24


def set_moments_check(x, out=None, splits=0):
    """every check of set_moments_u8 that needs no library call; x: anything with dtype and shape -> (N, D)"""
    if not hasattr(x, "dtype") or str(x.dtype) not in ("torch.uint8", "uint8") or len(x.shape) != 2 or x.shape[0] < 1:
        raise ValueError(f"set_moments_u8: x is uint8 [N >= 1, D]; got "
                         f"{(x.dtype, tuple(x.shape)) if hasattr(x, 'dtype') else type(x).__name__}")
    N, D = x.shape
    if D % 64 or not 64 <= D <= MOMENTS_MAX_D:
        raise ValueError(f"set_moments_u8: D is a multiple of 64 in [64, {MOMENTS_MAX_D}], got {D}")
    if N > MOMENTS_MAX_N:
        raise ValueError(f"set_moments_u8: at most 2^24 rows per call (accumulate with out=), got {N}")
    if torch.is_tensor(x) and not x.is_contiguous():
        raise ValueError("set_moments_u8: x is contiguous")
    if isinstance(splits, bool) or not isinstance(splits, int) or not 0 <= splits <= 4096:
        raise ValueError(f"set_moments_u8: splits is 0 (the library chooses) or in [1, 4096], got {splits!r}")
    if out is not None:
        if not isinstance(out, (tuple, list)) or len(out) != 2:
            raise ValueError("set_moments_u8: out is the pair (sum, gram) of an earlier call")
        for name, v, shape in (("sum", out[0], (D,)), ("gram", out[1], (D, D))):
            if not torch.is_tensor(v) or v.dtype != torch.int64 or tuple(v.shape) != shape or not v.is_contiguous():
                raise ValueError(f"set_moments_u8: out's {name} is a contiguous int64 {list(shape)}")
    return N, D


def set_moments_u8(x, out=None, splits=0):
    """(sum, gram), int64 [D] and [D, D] on x's device: the exact moments of the rows of x (uint8 [N, D]) about 128,
    sum[j] = sum_i c[i, j] and gram[j, k] = sum_i c[i, j] c[i, k] with c = x - 128, from the int8 matrix cores
    (mulan_set_moments_u8).  gram is written whole and equals its transpose bit for bit.  out = (sum, gram) of earlier
    calls: this call's rows are added to them, in place (a set walked in chunks).  splits: slices of the rows, 0 for the
    library's choice; the result does not depend on it."""
    N, D = set_moments_check(x, out, splits)
    if not torch.is_tensor(x):
        raise ValueError("set_moments_u8: x is a tensor on the device")
    dev = x.device
    if out is not None and any(v.device != dev for v in out):
        raise ValueError(f"set_moments_u8: out is on {[str(v.device) for v in out]}, x on {dev}")
    accumulate = out is not None
    total, gram = out if accumulate else (torch.empty(D, device=dev, dtype=torch.int64),
                                          torch.empty((D, D), device=dev, dtype=torch.int64))
    ws = torch.empty(lib.load().mulan_set_moments_u8_workspace(N, D, int(splits)) // 8, device=dev, dtype=torch.int64)
    call("mulan_set_moments_u8", ptr(x), N, D, int(accumulate), int(splits), ptr(total), ptr(gram), ptr(ws), stream())
    return total, gram


SPECTRUM_BINS = 45                 # radial bins of a 32 x 32 DCT: floor(sqrt(u^2 + v^2) + 1/2) = 0 .. 44
SPECTRUM_GRAY = (0.2125, 0.7154, 0.0721)   # skimage.color.rgb2gray; the kernel holds the same constants


def spectrum_check(x, scale=1.0, offset=0.0, gray=False, coef=False, radial=False, sums=False, accumulate_into=None,
                   blocks=0):
    """every check of spectrum that needs no library call; x: anything with dtype and shape -> (N, P)"""
    if not hasattr(x, "dtype") or str(x.dtype) not in ("torch.uint8", "uint8", "torch.float32", "float32") \
            or len(x.shape) != 4 or tuple(x.shape[1:]) != (32, 32, 3) or x.shape[0] < 1:
        raise ValueError(f"spectrum: x is uint8 or fp32 [N >= 1, 32, 32, 3]; got "
                         f"{(x.dtype, tuple(x.shape)) if hasattr(x, 'dtype') else type(x).__name__}")
    for name, v in (("scale", scale), ("offset", offset)):
        if isinstance(v, bool) or not isinstance(v, (int, float)) or v != v or abs(v) == float("inf"):
            raise ValueError(f"spectrum: {name} is a finite number, got {v!r}")
    for name, v in (("gray", gray), ("coef", coef), ("radial", radial), ("sums", sums)):
        if not isinstance(v, bool):
            raise ValueError(f"spectrum: {name} is a bool, got {v!r}")
    if isinstance(blocks, bool) or not isinstance(blocks, int) or not 0 <= blocks <= 4096:
        raise ValueError(f"spectrum: blocks is 0 (the library chooses) or in [1, 4096], got {blocks!r}")
    P = 1 if gray else 3
    if accumulate_into is not None:
        if not isinstance(accumulate_into, (tuple, list)) or len(accumulate_into) != 2:
            raise ValueError("spectrum: accumulate_into is the pair (sum1, sum2) of an earlier call")
        for name, v in zip(("sum1", "sum2"), accumulate_into):
            if not torch.is_tensor(v) or v.dtype != torch.float64 or tuple(v.shape) != (32, 32, P) or not v.is_contiguous():
                raise ValueError(f"spectrum: accumulate_into's {name} is a contiguous fp64 [32, 32, {P}]")
    if not (coef or radial or sums or accumulate_into is not None):
        raise ValueError("spectrum: nothing asked for (coef, radial and sums are all off)")
    return x.shape[0], P


def spectrum(x, *, scale=1.0, offset=0.0, gray=False, coef=False, radial=False, sums=False, accumulate_into=None, blocks=0):
    """(coef | None, radial | None, (sum1, sum2) | None) of N images x [N, 32, 32, 3]: the orthonormal 2-D DCT-II of every
    image and plane, scipy.fft.dctn(norm='ortho'), on the fp32 matrix cores (mulan_spectrum).  uint8 x is read as
    scale v + offset, fp32 x as it is; gray mixes the channels (SPECTRUM_GRAY) into one plane first: P = 1, else 3.
    coef: fp32 [N, 32, 32, P], [n, u, v, p] with u the vertical frequency.  radial: fp32 [N, 45, P], the sum of coef^2
    over radial bin r = floor(sqrt(u^2 + v^2) + 1/2).  sums: fp64 [32, 32, P] each, the sums over n of coef and coef^2.
    accumulate_into = (sum1, sum2) of an earlier call: this call's images are added to them, in place, and they are
    returned (a set uploaded in chunks).  blocks: 0 for the library's choice; only the rounding of the sums depends on
    it.  One fixed order per sum: the same call gives the same bits."""
    N, P = spectrum_check(x, scale, offset, gray, coef, radial, sums, accumulate_into, blocks)
    if not torch.is_tensor(x):
        raise ValueError("spectrum: x is a tensor on the device")
    dev = x.device
    if accumulate_into is not None and any(v.device != dev for v in accumulate_into):
        raise ValueError(f"spectrum: accumulate_into is on {accumulate_into[0].device}, x on {dev}")
    x = _c(x)
    coef_out = torch.empty((N, 32, 32, P), device=dev, dtype=torch.float32) if coef else None
    radial_out = torch.empty((N, SPECTRUM_BINS, P), device=dev, dtype=torch.float32) if radial else None
    sum1 = sum2 = ws = None
    nbytes = 0
    if accumulate_into is not None:
        sum1, sum2 = accumulate_into
    elif sums:
        sum1, sum2 = (torch.empty((32, 32, P), device=dev, dtype=torch.float64) for _ in range(2))
    if sum1 is not None:
        nbytes = lib.load().mulan_spectrum_workspace(N, int(gray), int(blocks))
        ws = torch.empty(nbytes // 8, device=dev, dtype=torch.float64)
    call("mulan_spectrum", ptr(x), 0 if x.dtype == torch.uint8 else 1, float(scale), float(offset), N, int(gray),
         ptr(coef_out), ptr(radial_out), ptr(sum1), ptr(sum2), int(accumulate_into is not None), int(blocks), ptr(ws),
         nbytes, stream())
    return coef_out, radial_out, (sum1, sum2) if sum1 is not None else None


FIDELITY_WINDOWS = 22              # SSIM windows per side: the 11 x 11 Gaussian inside a 32 x 32 image


def _fidelity_kind(v):
    return (str(v.dtype).replace("torch.", ""), tuple(v.shape)) if hasattr(v, "dtype") else type(v).__name__


def image_fidelity_check(a, b, ia=None, ib=None, gray=False, mask=None, sse=True, ssim=True, ssim_map=False):
    """every check of image_fidelity that needs no library call; a, b, ia, ib, mask: anything with dtype and shape
    -> (M, P, mask_per_pair)"""
    for name, v in (("a", a), ("b", b)):
        if not hasattr(v, "dtype") or str(v.dtype) not in ("torch.uint8", "uint8") or len(v.shape) != 4 \
                or tuple(v.shape[1:]) != (32, 32, 3) or v.shape[0] < 1:
            raise ValueError(f"image_fidelity: {name} is uint8 [N >= 1, 32, 32, 3]; got {_fidelity_kind(v)}")
    for name, v in (("gray", gray), ("sse", sse), ("ssim", ssim), ("ssim_map", ssim_map)):
        if not isinstance(v, bool):
            raise ValueError(f"image_fidelity: {name} is a bool, got {v!r}")
    for name, v in (("ia", ia), ("ib", ib)):
        if v is not None and (not hasattr(v, "dtype") or str(v.dtype) not in ("torch.int32", "int32")
                              or len(v.shape) != 1 or v.shape[0] < 1):
            raise ValueError(f"image_fidelity: {name} is int32 [M >= 1]; got {_fidelity_kind(v)}")
    if ia is not None and ib is not None and ia.shape[0] != ib.shape[0]:
        raise ValueError(f"image_fidelity: ia has {ia.shape[0]} pairs, ib has {ib.shape[0]}")
    Na, Nb = a.shape[0], b.shape[0]
    if ia is not None:
        M = ia.shape[0]
    elif ib is not None:
        M = ib.shape[0]
    else:
        if Na != Nb:
            raise ValueError(f"image_fidelity: a has {Na} images, b has {Nb}, and neither ia nor ib says which are paired")
        M = Na
    if ia is None and M > Na:
        raise ValueError(f"image_fidelity: ia is needed for {M} pairs out of the {Na} images of a")
    if ib is None and M > Nb:
        raise ValueError(f"image_fidelity: ib is needed for {M} pairs out of the {Nb} images of b")
    mask_per_pair = 0
    if mask is not None:
        if not hasattr(mask, "dtype") or str(mask.dtype) not in ("torch.uint8", "uint8") \
                or tuple(mask.shape) not in ((32, 32), (M, 32, 32)):
            raise ValueError(f"image_fidelity: mask is uint8 [32, 32] or [{M}, 32, 32]; got {_fidelity_kind(mask)}")
        mask_per_pair = int(len(mask.shape) == 3)
    if not (sse or ssim or ssim_map or mask is not None):
        raise ValueError("image_fidelity: nothing asked for (sse, ssim and ssim_map are off and there is no mask)")
    return M, (1 if gray else 3), mask_per_pair


def image_fidelity(a, b, *, ia=None, ib=None, gray=False, mask=None, sse=True, ssim=True, ssim_map=False):
    """(sse | None, sse_masked | None, ssim | None, ssim_map | None) of M pairs of uint8 images, a [Na, 32, 32, 3] against
    b [Nb, 32, 32, 3], on the device (mulan_image_fidelity).  Pair m is (a[ia[m]], b[ib[m]]), int32 [M] on the device, or
    (a[m], b[m]) where the index tensor is None.  sse: int32 [M, 3], the exact sum of squared differences per channel;
    sse_masked (returned with a mask: uint8 [32, 32] for all pairs or [M, 32, 32]): the same over the pixels whose
    mask byte is not 0.  ssim: fp32 [M, P], the mean SSIM (Wang et al. 2004: 11 x 11 Gaussian of sigma 1.5, biased moments,
    data range 255) over the 22 x 22 windows inside the image, per channel, or of the luma (SPECTRUM_GRAY) with gray:
    P = 1.  ssim_map: fp32 [M, 22, 22, P], the per-window values.  An index out of range is not read: that pair's sums
    are -1 and its SSIM NaN.  One fixed order per sum: the same call gives the same bits."""
    M, P, per_pair = image_fidelity_check(a, b, ia, ib, gray, mask, sse, ssim, ssim_map)
    tensors = [("a", a), ("b", b), ("ia", ia), ("ib", ib), ("mask", mask)]
    if not torch.is_tensor(a) or any(v is not None and (not torch.is_tensor(v) or v.device != a.device) for _, v in tensors):
        raise ValueError("image_fidelity: a, b, ia, ib and mask are tensors on one device")
    dev = a.device
    a, b, ia, ib, mask = _c(a), _c(b), _c(ia), _c(ib), _c(mask)
    W = FIDELITY_WINDOWS
    sse_out = torch.empty((M, 3), device=dev, dtype=torch.int32) if sse else None
    masked_out = torch.empty((M, 3), device=dev, dtype=torch.int32) if mask is not None else None
    ssim_out = torch.empty((M, P), device=dev, dtype=torch.float32) if ssim else None
    map_out = torch.empty((M, W, W, P), device=dev, dtype=torch.float32) if ssim_map else None
    call("mulan_image_fidelity", ptr(a), a.shape[0], ptr(b), b.shape[0], ptr(ia), ptr(ib), M, int(gray), ptr(mask),
         per_pair, ptr(sse_out), ptr(masked_out), ptr(ssim_out), ptr(map_out), stream())
    return sse_out, masked_out, ssim_out, map_out


TSNE_MIN_N, TSNE_MAX_N = 4, 16384     # the range of mulan_tsne_*: P is dense, 1 GiB at the cap


def _tsne_number(name, v, lo=None, lo_open=False, hi=None):
    """a finite real (not a bool) with lo <= v (lo < v with lo_open) and v < hi -> float"""
    if isinstance(v, bool) or not isinstance(v, (int, float)) or v != v or abs(v) == float("inf"):
        raise ValueError(f"tsne: {name} is a finite number, got {v!r}")
    if (lo is not None and (v <= lo if lo_open else v < lo)) or (hi is not None and v >= hi):
        raise ValueError(f"tsne: {name} lies in {'(' if lo_open else '['}{lo}, {hi if hi is not None else 'inf'}), got {v!r}")
    return float(v)


def _tsne_array(name, v, shape, dtype="float32"):
    if not hasattr(v, "dtype") or str(v.dtype).replace("torch.", "") != dtype or tuple(v.shape) != tuple(shape):
        raise ValueError(f"tsne: {name} is {dtype} {list(shape)}; got "
                         f"{(v.dtype, tuple(v.shape)) if hasattr(v, 'dtype') else type(v).__name__}")
    if torch.is_tensor(v) and not v.is_contiguous():
        raise ValueError(f"tsne: {name} is contiguous")


def tsne_affinities_check(x, perplexity, symmetrise=True, return_beta=False):
    """every check of tsne_affinities that needs no library call; x: anything with dtype and shape -> (N, D)"""
    if not hasattr(x, "dtype") or str(x.dtype) not in ("torch.float32", "float32") or len(x.shape) != 2 \
            or not TSNE_MIN_N <= x.shape[0] <= TSNE_MAX_N or x.shape[1] < 1:
        raise ValueError(f"tsne: x is fp32 [N, D] with {TSNE_MIN_N} <= N <= {TSNE_MAX_N} and D >= 1; got "
                         f"{(x.dtype, tuple(x.shape)) if hasattr(x, 'dtype') else type(x).__name__}")
    N, D = x.shape
    _tsne_number("perplexity", perplexity, lo=1, hi=N - 1)
    for name, v in (("symmetrise", symmetrise), ("return_beta", return_beta)):
        if not isinstance(v, bool):
            raise ValueError(f"tsne: {name} is a bool, got {v!r}")
    return N, D


def tsne_affinities(x, perplexity, symmetrise=True, return_beta=False):
    """P, fp32 [N, N], of the rows of x (fp32 [N, D] on the device): the affinities of exact t-SNE (mulan_tsne_affinities).
    Row i holds P_{j|i}, the Gaussian around x_i whose perplexity is `perplexity` (1 <= perplexity < N - 1), from squared
    distances taken from the differences; with symmetrise (P_{j|i} + P_{i|j}) / (2 N), which sums to 1.  return_beta:
    (P, beta) with beta fp32 [N], the precisions 1 / (2 sigma_i^2) the search ended at.  The same call gives the same
    bits."""
    N, D = tsne_affinities_check(x, perplexity, symmetrise, return_beta)
    if not torch.is_tensor(x) or not x.is_cuda:
        raise ValueError("tsne: x is a tensor on the device")
    x = _c(x)
    P = torch.empty((N, N), device=x.device, dtype=torch.float32)
    beta = torch.empty(N, device=x.device, dtype=torch.float32) if return_beta else None
    call("mulan_tsne_affinities", ptr(x), N, D, float(perplexity), int(symmetrise), ptr(P), ptr(beta), stream())
    return (P, beta) if return_beta else P


def tsne_step_check(P, Y, U, G, exaggeration, momentum, lr, kl=False):
    """every check of tsne_step that needs no library call -> N"""
    if not hasattr(P, "shape") or len(P.shape) != 2 or P.shape[0] != P.shape[1] or not TSNE_MIN_N <= P.shape[0] <= TSNE_MAX_N:
        raise ValueError(f"tsne: P is fp32 [N, N] with {TSNE_MIN_N} <= N <= {TSNE_MAX_N}; got "
                         f"{tuple(P.shape) if hasattr(P, 'shape') else type(P).__name__}")
    N = P.shape[0]
    _tsne_array("P", P, (N, N))
    for name, v in (("Y", Y), ("U", U), ("G", G)):
        _tsne_array(name, v, (N, 2))
    _tsne_number("exaggeration", exaggeration, lo=0, lo_open=True)
    _tsne_number("momentum", momentum, lo=0, hi=1)
    _tsne_number("lr", lr, lo=0, lo_open=True)
    if not isinstance(kl, bool):
        _tsne_array("kl", kl, (), "float64")
    return N


def tsne_step(P, Y, U, G, exaggeration, momentum, lr, kl=False):
    """One iteration of exact t-SNE, in place on the map Y, its update U and the gains G (fp32 [N, 2] each) under the
    affinities P (fp32 [N, N]): mulan_tsne_gradient (one pass over P, then the fold) and mulan_tsne_update (sklearn's
    delta-bar-delta body; no recentring).  kl: True returns the Kullback-Leibler divergence of the map BEFORE the update,
    of P as passed, as a 0-d fp64 tensor on the device (no host read); a 0-d fp64 device tensor is written instead of a
    fresh one; False returns None and the launch holds no logarithm."""
    N = tsne_step_check(P, Y, U, G, exaggeration, momentum, lr, kl)
    for name, v in (("P", P), ("U", U), ("G", G)):
        if not torch.is_tensor(v) or not v.is_cuda or v.device != P.device:
            raise ValueError(f"tsne: {name} is a tensor on the device of P")
    grad, out = tsne_gradient(P, Y, exaggeration, kl)
    call("mulan_tsne_update", ptr(grad), ptr(Y), ptr(U), ptr(G), N, float(momentum), float(lr), stream())
    return out


def tsne_gradient(P, Y, exaggeration=1.0, kl=False):
    """(grad fp32 [N, 2], kl): the gradient pass of tsne_step alone, nothing updated; kl as in tsne_step"""
    N = tsne_step_check(P, Y, Y, Y, exaggeration, 0.5, 1.0, kl)
    for name, v in dict(P=P, Y=Y, **({} if isinstance(kl, bool) else dict(kl=kl))).items():
        if not torch.is_tensor(v) or not v.is_cuda or v.device != P.device:
            raise ValueError(f"tsne: {name} is a tensor on the device of P")
    dev = P.device
    out = torch.empty((), device=dev, dtype=torch.float64) if kl is True else (None if kl is False else kl)
    nbytes = lib.load().mulan_tsne_workspace(N)
    ws = torch.empty(nbytes // 4, device=dev, dtype=torch.float32)
    grad = torch.empty((N, 2), device=dev, dtype=torch.float32)
    call("mulan_tsne_gradient", ptr(P), ptr(Y), N, float(exaggeration), ptr(grad), ptr(out), ptr(ws), nbytes, stream())
    return grad, out


def tsne_kl(P, Y, out=None):
    """the Kullback-Leibler divergence of the map Y under P: a 0-d fp64 device tensor (`out`, if given, is written)"""
    return tsne_gradient(P, Y, 1.0, kl=True if out is None else out)[1]


# ----------------------------------------------------------------------------- exact-likelihood ODE (eval only)
def topk_hard(logits, k):
    """(k-hot embedding of the plain logits, KL(softmax(logits) || uniform)): notebook_utils.logits_to_embeddings and
    _gumbel_kl_loss (ldm/notebook_utils.py:548-551, 222-229)"""
    logits = _c(logits)
    B, L = logits.shape
    emb = torch.empty_like(logits)
    kl = torch.empty(B, device=logits.device, dtype=torch.float32)
    call("mulan_topk_fwd", ptr(logits), None, ptr(emb), ptr(kl), None, None, B, L, int(k), 0.0, stream())
    return emb, kl


def ode_drift(net, x, gt, gp, hutch, mode, drift_out=None, want_cot=True):
    """(drift, cotangent for net) of VDM.reverse_ode; gamma per element or per sample"""
    net, x, gt, gp = _c(net), _c(x), _c(gt), _c(gp)
    hutch = _c(hutch) if hutch is not None else None
    drift = drift_out if drift_out is not None else torch.empty_like(net)
    cot = torch.empty_like(net) if (want_cot and hutch is not None) else None
    per = net.numel() // gt.numel()
    call("mulan_ode_drift", ptr(net), ptr(x), ptr(gt), ptr(gp), ptr(hutch) if hutch is not None else None, ptr(drift),
         ptr(cot), net.numel(), int(mode), 0 if per == 1 else per, stream())
    return drift, cot


def ode_div(gx, gt, gp, hutch, mode, div_out=None):
    gx, gt, gp, hutch = _c(gx), _c(gt), _c(gp), _c(hutch)
    B = gx.shape[0]
    d = gx.numel() // B
    div = div_out if div_out is not None else torch.empty(B, device=gx.device, dtype=torch.float32)
    call("mulan_ode_div", ptr(gx), ptr(gt), ptr(gp), ptr(hutch), ptr(div), B, d, int(mode),
         0 if gt.numel() == gx.numel() else d, stream())
    return div


def _coef(values):
    import ctypes
    return (ctypes.c_double * 7)(*(list(values) + [0.0] * (7 - len(values))))


def rk_combine(y, K, coef, h, out=None, out32=None):
    """out = y + h sum_j coef_j K[j] as float64 and / or fp32; K [7, n] fp32"""
    call("mulan_rk_combine", ptr(y), ptr(K), K.stride(0), _coef(coef), len(coef), float(h), ptr(out), ptr(out32),
         y.numel(), stream())


def rk_workspace(device):
    from .lib import load
    return torch.empty(load().mulan_rk_workspace_bytes() // 8, device=device, dtype=torch.float64)


def rk_error_norm(y, ynew, K, e, h, rtol, atol, ws, out):
    call("mulan_rk_error_norm", ptr(y), ptr(ynew), ptr(K), K.stride(0), _coef(e), float(h), float(rtol), float(atol),
         ptr(ws), ptr(out), y.numel(), stream())


def rk_init_norms(y0, f0, f1, rtol, atol, ws, out3):
    call("mulan_rk_init_norms", ptr(y0), ptr(f0), ptr(f1) if f1 is not None else None, float(rtol), float(atol), ptr(ws),
         ptr(out3), y0.numel(), stream())


def normal_logp(x):
    x = _c(x)
    rows = x.shape[0]
    out = torch.empty(rows, device=x.device, dtype=torch.float32)
    call("mulan_normal_logp", ptr(x), ptr(out), rows, x.numel() // rows, stream())
    return out


def noise(shape, seed, offset, device, kind, lo=-3.0, hi=3.0):
    """kind: 'uniform' U[0,1) | 'rademacher' +-1 | 'truncated_normal' on [lo, hi]"""
    out = torch.empty(shape, device=device, dtype=torch.float32)
    call("mulan_noise", ptr(out), out.numel(), int(seed) & (2**64 - 1), int(offset),
         {"uniform": 0, "rademacher": 1, "truncated_normal": 2, "gumbel": 3}[kind], float(lo), float(hi), stream())
    return out


def dequantize(x_u8, u, uniform, scale=1.0):
    """(data = encode(x) + noise as fp32, the re-quantised uint8 image the encoder sees)"""
    x_u8, u = _c(x_u8), _c(u)
    data = torch.empty(x_u8.shape, device=x_u8.device, dtype=torch.float32)
    rq = torch.empty_like(x_u8)
    call("mulan_dequantize", ptr(x_u8), ptr(u), ptr(data), ptr(rq), x_u8.numel(), 1 if uniform else 0, float(scale),
         stream())
    return data, rq
