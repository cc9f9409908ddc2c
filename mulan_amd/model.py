"""MuLAN / VDM models over the HIP kernels (host-side mirror of the reference's Flax modules).

Functional, Flax-like API: `VDM(config).init(rng)` returns a parameter tree whose names and shapes
are the reference's (the only layout difference is conv_in, stored with a 16th
zero input channel for aligned loads), `VDM.apply(params, images, labels, conditioning, step, rngs,
deterministic)` returns a VDMOutput.  Mirrors:
  VDMConfig / VDMOutput ............ ldm/model_vdm.py:33-92
  ScoreUNet / ldm UNet / UnetEncoder  ldm/model_vdm.py:309-388, ldm/ldm_unet.py:64-142,
                                     ldm/model_mulan_epsilon.py:101-154
  ResnetBlock / AttnBlock .......... ldm/model_vdm.py:610-701, ldm/ldm_unet.py:10-61
  NoiseSchedule_polynomial_fixedend  ldm/model_mulan_epsilon.py:481-613
  NoiseSchedule_{Scalar,FixedLinear,NNet} (plain VDM) ldm/model_vdm.py:418-509
  VDM.__call__ ...................... ldm/model_mulan_velocity.py:188-268,
                                     ldm/model_mulan_epsilon.py:280-363, ldm/model_vdm.py:110-180
All tensor math runs in libmulan_hip.so (mulan_amd.ops); there is no CPU path.
"""
import dataclasses
import functools
import logging
import math
import os
import numpy as np
from typing import Any, Optional

import torch

from . import ops
from .rng import Key

HW = 1024
D = 3072
HWC = (32, 32, 3)           # an image of D sub-pixels, in the order the samplers' [B, D] states hold it


# ----------------------------------------------------------------------------- config / output
@dataclasses.dataclass(frozen=True)
class VDMConfig:
    """Same fields as the reference dataclass (ldm/model_vdm.py:33-82); unknown keys raise TypeError."""
    vocab_size: int
    sample_softmax: bool
    antithetic_time_sampling: bool
    with_fourier_features: bool
    with_attention: bool
    gamma_type: str
    gamma_min: float
    gamma_max: float
    sm_n_timesteps: int
    sm_n_embd: int
    sm_n_layer: int
    sm_pdrop: float
    sm_kernel_init: Any = None
    forward_n_layer: int = 4
    forward_type: int = 1
    sigma_type: str = 'learnable_scalar'
    sigma_min: float = 0
    sigma_max: float = 20.0
    sm_mult: float = 1.0
    sigma_prior: float = 1.0
    blur_noise: bool = False
    sigma_recons_type: str = 'sigmoid'
    loss_type: str = 'recons'
    reparam_type: str = 'noise'
    nn_input: str = 'gamma'
    condition: str = 'label'
    latent_size: int = 10
    epsilon: float = 0.0
    encoder: str = 'cnn'
    model_time: bool = False
    monotone_layer: str = 'dense_monotone'
    latent_type: str = 'gumbel'
    z_conditioning: bool = False
    importance_sampling: bool = False
    velocity_from_epsilon: bool = False
    unet_type: str = 'vdm'
    topk_noise_type: str = 'gamma'
    latent_k: int = 15
    trace_matching: bool = False


@dataclasses.dataclass
class VDMOutput:
    loss_recon: torch.Tensor   # [B]
    loss_klz: torch.Tensor     # [B]
    loss_diff: torch.Tensor    # [B]
    var_0: torch.Tensor
    var_1: torch.Tensor


# ----------------------------------------------------------------------------- initialisers
def _lecun_normal(gen, shape, fan_in):
    """jax.nn.initializers.lecun_normal (flax Dense/Conv default): truncated normal, var = 1/fan_in"""
    std = math.sqrt(1.0 / fan_in) / .87962566103423978
    t = torch.empty(shape, dtype=torch.float32)
    torch.nn.init.trunc_normal_(t, mean=0.0, std=std, a=-2 * std, b=2 * std, generator=gen)
    return t


def _dense(gen, cin, cout, bias=True, zero=False):
    p = {"kernel": torch.zeros(cin, cout) if zero else _lecun_normal(gen, (cin, cout), cin)}
    if bias:
        p["bias"] = torch.zeros(cout)
    return p


def _conv(gen, cin, cout, zero=False, pad_in=0):
    k = torch.zeros(3, 3, cin, cout) if zero else _lecun_normal(gen, (3, 3, cin, cout), 9 * cin)
    if pad_in:
        k = torch.cat([k, torch.zeros(3, 3, pad_in, cout)], dim=2)
    return {"kernel": k, "bias": torch.zeros(cout)}


def _gn(C):
    return {"scale": torch.ones(C), "bias": torch.zeros(C)}


def _resblock_init(gen, cin, cout, cond_dim):
    p = {"GroupNorm_0": _gn(cin), "conv1": _conv(gen, cin, cout), "cond_proj": _dense(gen, cond_dim, cout, False, True),
         "GroupNorm_1": _gn(cout), "conv2": _conv(gen, cout, cout, zero=True)}
    if cin != cout:
        p["nin_shortcut"] = _dense(gen, cin, cout)
    return p


def _attn_init(gen, C):
    return {"GroupNorm_0": _gn(C), "q": _dense(gen, C, C), "k": _dense(gen, C, C), "v": _dense(gen, C, C),
            "proj_out": _dense(gen, C, C, zero=True)}


def _unet_init(gen, E, n_layers, cond_in, out_ch, with_up, with_attention=False):
    p = {"dense0": _dense(gen, cond_in, 4 * E), "dense1": _dense(gen, 4 * E, 4 * E),
         "conv_in": _conv(gen, 15, E, pad_in=1)}
    for i in range(n_layers):
        p[f"down.block_{i}"] = _resblock_init(gen, E, E, 4 * E)
        if with_attention:                      # AttnBlock after every block (ldm/model_vdm.py:356-357, 371-372)
            p[f"down.attn_{i}"] = _attn_init(gen, E)
    p["mid.block_1"] = _resblock_init(gen, E, E, 4 * E)
    p["mid.attn_1"] = _attn_init(gen, E)
    p["mid.block_2"] = _resblock_init(gen, E, E, 4 * E)
    if with_up:
        for i in range(n_layers + 1):
            p[f"up.block_{i}"] = _resblock_init(gen, 2 * E, E, 4 * E)
            if with_attention:
                p[f"up.attn_{i}"] = _attn_init(gen, E)
    p["GroupNorm_0"] = _gn(E)
    p["conv_out"] = _conv(gen, E, out_ch, zero=True)
    return p


# ----------------------------------------------------------------------------- blocks
class _Drop:
    """Per-apply dropout context: one Philox seed, a distinct counter window per dropout site."""

    def __init__(self, key: Optional[Key], rate: float):
        self.on = key is not None and rate > 0.0
        self.keep = 1.0 - rate if self.on else 1.0
        # a Key bound to a device slot (rng.Key.dev, graph capture) hands the kernels the slot instead of the value
        self.seed = 0 if key is None else (key.dev if getattr(key, "dev", None) is not None else key.v)
        self.site = 0

    def next(self):
        self.site += 1
        return self.keep, self.seed, self.site << 34


SAMPLER_GRAPH = os.environ.get("MULAN_SAMPLER_GRAPH", "1") == "1"


def _capture(run):
    """run() as a HIP graph -> (the graph, what run() returned inside the capture).  Two eager runs come first: every
    kernel configured, the allocator warm."""
    for _ in range(2):
        run()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    # (thread_local: the RCCL watchdog thread of a multi-rank job keeps polling its events during the capture)
    with torch.cuda.graph(graph, capture_error_mode="thread_local"):
        out = run()
    return graph, out


def _graphed_or_eager(graph, device, graphed, eager, warning):
    """graphed() where `graph` asks for a replayed HIP graph and `device` is a GPU, else eager(); the replay is an
    optimisation, so a capture that fails falls back to eager() loudly (`warning`: the log line, with the exception's
    type and text as its two arguments)"""
    if graph and torch.device(device).type == "cuda":
        try:
            return graphed()
        except Exception as e:      # noqa: BLE001
            logging.getLogger("mulan").warning(warning, type(e).__name__, e)
    return eager()


class GraphedReverseStep:
    """One reverse step of the ancestral sampler (VDM.sample / conditional_sample, ldm/model_mulan_velocity.py:281-350)
    captured as a HIP graph and replayed T times.  What changes from step to step reaches the kernels through static
    buffers written before each replay: z_t, the step's noise (drawn by the same Philox call as the eager step, into the
    buffer) and the two times t, s; the replayed step is bit-identical to conditional_sample
    (tests/test_gpu_sampler.py::test_replayed_reverse_step_equals_the_eager_step).  The weights must stay as they are
    while the stepper lives (the caller holds the ParamPacker refresh, as the eager loop does)."""

    def __init__(self, model, params, B, device, embedding, conditioning, coeffs, T):
        self.model, self.T, self.B = model, T, B
        f32 = dict(device=device, dtype=torch.float32)
        self.z_in, self.eps = torch.zeros((B, D), **f32), torch.zeros((B, D), **f32)
        self.t, self.s = torch.full((B,), 1.0, **f32), torch.full((B,), 1.0 - 1.0 / T, **f32)
        ctx = dict(emb=embedding, cond=conditioning, coeffs=coeffs)     # (as conditional_sample hands it over)
        with torch.no_grad():
            self.graph, self.z_out = _capture(
                lambda: model._reverse_step(params, self.z_in, self.eps, self.t, self.s, ctx))

    def step(self, i, z, rng):
        B, T = self.B, self.T
        self.z_in.copy_(z.reshape(B, D))
        ops.randn(None, rng.fold_in(i).v, 0, self.z_in.device, out=self.eps)
        self.t.fill_(float(np.float32((T - i) / T)))
        self.s.fill_(float(np.float32((T - i - 1) / T)))
        self.graph.replay()
        return self.z_out.view(z.shape)


def _check_fast_context(like, ctx):
    """a stepper built for one context takes another only with the same keys and shapes (no broadcast of a [1, 50]
    embedding over a stepper of B rows)"""
    if set(like) != set(ctx):
        raise ValueError(f"sampler context keys {sorted(ctx)} differ from the stepper's {sorted(like)}")
    for k, v in ctx.items():
        a, b = like[k], v
        pairs = zip(a, b) if isinstance(a, tuple) else [(a, b)]
        if isinstance(a, tuple) and (not isinstance(b, tuple) or len(a) != len(b)):
            raise ValueError(f"sampler context {k!r}: expected {len(a)} tensors")
        for x, y in pairs:
            if (x is None) != (y is None) or (x is not None and tuple(x.shape) != tuple(y.shape)):
                raise ValueError(f"sampler context {k!r}: shape {None if y is None else tuple(y.shape)} where the "
                                 f"stepper was built for {None if x is None else tuple(x.shape)}")


def _fill_noise(buf, noise, i, missing, zeros=False):
    """draw i of a few-step run into buf [B, 3072]: `noise` is a key of the batch (the draw is ops.randn under
    key.fold_in(i), as the ancestral steppers draw theirs) or a callable i -> xi; `missing`: what to say where the batch
    has set none.  zeros: a negative i (sampling.ZERO_NOISE, the mix of the last step) fills zeros"""
    if zeros and i < 0:
        return buf.zero_()
    if noise is None:
        raise RuntimeError(missing)
    if i is None:
        raise ValueError("a stochastic step needs its index k (the noise is drawn per step)")
    if callable(noise):
        buf.copy_(noise(i).reshape(buf.shape))
    else:
        ops.randn(None, noise.fold_in(i).v, 0, buf.device, out=buf)
    return buf


class _FastStepState:
    """What the two steppers of the few-step samplers keep per batch, in static buffers [B, 3072] where a kernel reads it:
    step_eta > 0: the noise xi of the stochastic step, drawn for step k from the key (or callable) set_noise() names;
    inpaint: the known image (as ops.encode_u8 gives it) and the mask (one byte per sub-pixel, non-zero = keep) of
    set_known(); restore = (f, gray): the measurement y (shaped ops.restore_y_shape) of set_measurement().  kxi takes
    draw j of the key (or callable) either of the two names: the noise of the known region at a mix and of a jump, one
    buffer for both in both steppers (a jump's noise is read before the next mix is drawn)."""

    def __init__(self, B, device, step_eta, inpaint, restore):
        from . import sampling
        self.B, self.step_eta, self.inpaint = B, float(step_eta), bool(inpaint)
        self.restore = None if restore is None else sampling.parse_degradation(restore)
        if self.inpaint and self.restore is not None:
            raise ValueError("a mask and a measurement in one run are not supported: inpaint or restore")
        f32 = lambda on, *shape: torch.zeros(shape or (B, D), device=device, dtype=torch.float32) if on else None
        self.noise = self.known_noise = None
        self.xi, self.known = f32(self.step_eta > 0.0), f32(self.inpaint)
        self.mask = torch.zeros((B, D), device=device, dtype=torch.uint8) if self.inpaint else None
        self.kxi = f32(self.inpaint or self.restore is not None)
        self.y = None if self.restore is None else f32(True, *ops.restore_y_shape(B, *HWC, *self.restore))

    def check_serves(self, step_eta, inpaint, restore):
        """a stepper serves the runs it was built for: the same step_eta, with or without a mask, the same degradation"""
        if self.step_eta != step_eta:
            raise ValueError(f"fast_sample: the stepper's steps run with eta = {self.step_eta}, this run asks for "
                             f"{step_eta}")
        if self.inpaint != inpaint:
            raise ValueError("fast_sample: the stepper was built %s a mask, this run comes %s one"
                             % (("without", "with") if inpaint else ("with", "without")))
        if self.restore != restore:
            name = lambda r: "no degradation" if r is None else f"the degradation (f, gray) = {r}"
            raise ValueError(f"fast_sample: the stepper was built for {name(self.restore)}, this run comes with "
                             f"{name(restore)}")

    def set_noise(self, noise):
        self.noise = noise

    def set_known(self, known, mask, noise=None):
        """this batch's known image and mask (B x 3072 elements each) and its known-region noise"""
        if not self.inpaint:
            raise ValueError("this stepper was built without a mask (fast_stepper(..., inpaint=True) builds one with)")
        if known.numel() != self.known.numel() or mask.numel() != self.mask.numel():
            raise ValueError(f"the known image and the mask hold {tuple(self.known.shape)} elements each, got "
                             f"{tuple(known.shape)} and {tuple(mask.shape)}")
        self.known.copy_(known.reshape(self.known.shape))
        self.mask.copy_(mask.reshape(self.mask.shape))
        self.known_noise = noise

    def set_measurement(self, y, noise=None):
        """this batch's measurement (fp32, ops.restore_y_shape values) and the key (or callable j -> xi) of its jumps"""
        if self.restore is None:
            raise ValueError("this stepper was built without a degradation (fast_stepper(..., restore=(f, gray)) builds "
                             "one with)")
        if y.dtype != torch.float32 or y.numel() != self.y.numel():
            raise ValueError(f"the measurement is fp32 {list(self.y.shape)}, got {y.dtype} {list(y.shape)}")
        self.y.copy_(y.reshape(self.y.shape))
        self.known_noise = noise

    def _check_mix(self, mix):
        if (mix is not None) != self.inpaint:
            raise ValueError("a stepper built with a mask mixes after every step, and one built without never does")

    def _step_xi(self, k):
        return _fill_noise(self.xi, self.noise, k,
                           "a stochastic step needs the batch's noise (set_noise: a Key, or a callable k -> xi)")

    def _known_xi(self, j):
        return _fill_noise(self.kxi, self.known_noise, j, "inpainting needs the batch's known-region noise (set_known: a "
                           "Key, or a callable j -> xi)", zeros=True)


class EagerFastStep(_FastStepState):
    """The eager form of GraphedFastStep (MULAN_SAMPLER_GRAPH=0, or a failed capture): sampling.EagerStepper over the
    model's network and schedule and over the buffers of _FastStepState, reading the context through this object so that
    set_context() re-targets it at the next batch like the replayed stepper.  It shares no step code with the replayed
    form beyond sampling.solver_step: gamma(s) is cached for the next step, and the history is the step's own output."""

    def __init__(self, model, params, B, device, ctx, step_eta=0.0, inpaint=False, restore=None):
        from . import sampling
        super().__init__(B, device, step_eta, inpaint, restore)
        self.ctx = ctx
        times = lambda t: torch.full((B,), float(np.float32(t)), device=device, dtype=torch.float32)
        gamma_fn = lambda t: model._fast_gamma(params, self.ctx, times(t))
        net_fn = lambda z, t: model._fast_net(params, z.reshape(B, D), gamma_fn(t), self.ctx).view(z.shape)
        self._make = lambda: sampling.EagerStepper(
            net_fn, gamma_fn, model._fast_mode(), self.step_eta, self._step_xi if self.xi is not None else None, self.known,
            self.mask, self._known_xi if self.kxi is not None else None, self.y, self.restore, HWC)
        self._step = self._make()

    def set_context(self, ctx):
        _check_fast_context(self.ctx, ctx)
        self.ctx = ctx
        self._step = self._make()             # no history and no cached gamma of the previous batch

    def mix(self, z, t, j):
        return self._step.mix(z, t, j)

    def jump(self, z, s, t, j):
        return self._step.jump(z, s, t, j)

    def __call__(self, z, t, s, order, k=None, mix=None):
        self._check_mix(mix)
        return self._step(z, t, s, order, k, mix)


class GraphedFastStep(_FastStepState):
    """One step of the deterministic few-step samplers (DDIM / DPM-Solver++(2M), mulan_amd.sampling) captured as a HIP
    graph and replayed N times.  What changes from step to step reaches the kernels through static buffers written
    before each replay: z_t, the two times t, s and the history (the previous step's gamma and x_hat, copied from the
    graph's outputs after each replay); a first-order step fills the previous gamma with NaN, which mulan_fast_sampler_step
    reads as "no usable history" (the same code path as its NULL form, so the same bits).  The per-batch context (the
    embedding and the schedule coefficients of the MuLAN models) sits in buffers of its own: set_context() re-targets the
    graph at the next batch.  The replayed step is bit-identical to the eager one
    (tests/test_gpu_fast_sampler.py::test_replayed_fast_step_equals_the_eager_step).  The weights must stay as they are
    while the stepper lives (the caller holds the ParamPacker refresh).
    step_eta > 0 captures the stochastic step (DDIM with eta, SDE-DPM-Solver++(2M)) instead: its noise xi is one more static
    buffer, filled before each replay by the Philox call of the eager stepper (_fill_noise, the pattern of
    GraphedReverseStep.step); step_eta is an argument of the captured launch, so a stepper serves the one it was built
    for.
    inpaint captures the mix behind the step kernel (mulan_inpaint_mix at gamma_s): the known image, the mask and the
    known region's noise are static buffers, the first two set per batch (set_known), the noise filled before each
    replay (zeros for the last step, which the kernel reads as it reads a NULL xi).  The mix of z_1 and the jumps of the
    resampling are eager launches between replays, on the same noise buffer.
    restore = (f, gray) captures the projection (mulan_restore_project) between the network and the step kernel, which
    then runs at mode 2 on x_hat'; the measurement is a static buffer set per batch (set_measurement), and the history
    copied after each replay is x_hat'.  The jumps are eager launches as above."""

    def __init__(self, model, params, B, device, ctx, step_eta=0.0, inpaint=False, restore=None):
        super().__init__(B, device, step_eta, inpaint, restore)
        self.model, self.params = model, params
        f32 = dict(device=device, dtype=torch.float32)
        self.ctx = {k: (None if v is None else tuple(c.detach().clone() for c in v) if isinstance(v, tuple)
                        else v.detach().clone()) for k, v in ctx.items()}
        self.z_in, self.x_prev = torch.zeros((B, D), **f32), torch.zeros((B, D), **f32)
        self.t, self.s = torch.full((B,), 1.0, **f32), torch.full((B,), 0.5, **f32)
        self.g_prev = torch.full(model._fast_gamma_shape(B), float("nan"), **f32)
        run = lambda: model._fast_step(params, self.z_in, self.t, self.s, self.g_prev, self.x_prev, self.ctx, self.xi,
                                       self.step_eta, self.known, self.mask, self.kxi, self.y, self.restore)
        with torch.no_grad():
            self.graph, (self.z_out, self.x_out, self.g_out) = _capture(run)
        self.has_history = False

    def set_context(self, ctx):
        _check_fast_context(self.ctx, ctx)
        for k, v in ctx.items():
            if isinstance(v, tuple):
                for dst, src in zip(self.ctx[k], v):
                    dst.copy_(src)
            elif v is not None:
                self.ctx[k].copy_(v)
        self.has_history = False

    def _gamma_at(self, buf, t):
        buf.fill_(float(np.float32(t)))
        return self.model._fast_gamma(self.params, self.ctx, buf)

    def mix(self, z, t, j):
        g = self._gamma_at(self.t, t)
        return ops.inpaint_mix(z.reshape(self.B, D), self.known, self.mask, g, self._known_xi(j)).view(z.shape)

    def jump(self, z, s, t, j):
        g_s, g_t = self._gamma_at(self.s, s), self._gamma_at(self.t, t)
        return ops.forward_jump(z.reshape(self.B, D), g_s, g_t, self._known_xi(j)).view(z.shape)

    def __call__(self, z, t, s, order, k=None, mix=None):
        self._check_mix(mix)
        if order == 2 and not self.has_history:
            raise RuntimeError("a second-order step needs the history of a previous step")
        if self.xi is not None:
            self._step_xi(k)
        if mix is not None:
            self._known_xi(mix)
        self.z_in.copy_(z.reshape(self.B, D))
        self.t.fill_(float(np.float32(t)))
        self.s.fill_(float(np.float32(s)))
        if order != 2:
            self.g_prev.fill_(float("nan"))
        self.graph.replay()
        self.x_prev.copy_(self.x_out)
        self.g_prev.copy_(self.g_out)
        self.has_history = True
        return self.z_out.view(z.shape)


ODE_GRAPH = os.environ.get("MULAN_ODE_GRAPH", "1") == "1"      # A/B switch: 0 = every function evaluation issued eagerly


class GraphedOdeFunction:
    """One function evaluation of the probability-flow ODE -- VDM.reverse_ode and, for the likelihood, the Hutchinson term
    hutch^T (d drift / d x) hutch through the U-Net's input gradient (ldm/model_mulan_velocity.py:393-421,
    ldm/notebook_utils.py:203-215) -- captured as a HIP graph and replayed at every stage of every Dormand-Prince step.
    Eagerly an evaluation is ~1100 dependent launches that the host needs ~25 ms to issue whatever the batch (measured:
    25.1 ms per evaluation at 16 AND at 64 images); replayed, the device's own time is left.  What changes between
    evaluations reaches the kernels through static buffers: the state x, the probe, the time (a [B] tensor read by
    mulan_poly_gamma).  Same kernels, same order: results are bit-identical to the eager evaluation
    (tests/test_gpu_ode.py::test_replayed_ode_function_equals_the_eager_one).  The weights must stay as they are while the
    object lives (the caller holds the ParamPacker refresh)."""

    def __init__(self, model, params, ctx, B, device, with_div, high_precision=False):
        self.model, self.B, self.with_div, self.params = model, B, with_div, params
        f32 = dict(device=device, dtype=torch.float32)
        # the per-batch context (embedding, schedule coefficients) in buffers of its own: set_context() re-targets a
        # captured graph at the next batch / importance sample instead of capturing again
        self.ctx = dict(emb=ctx["emb"].detach().clone(), coeffs=tuple(c.detach().clone() for c in ctx["coeffs"]))
        ctx = self.ctx
        self.x, self.tt = torch.zeros((B, D), **f32), torch.full((B,), 0.5, **f32)
        self.probe = torch.ones((B, D), **f32) if with_div else None
        self.drift = torch.empty((B, D), **f32)
        self.div = torch.empty((B,), **f32) if with_div else None
        run = lambda: model.reverse_ode(params, self.x, ctx, None, self.probe, drift_out=self.drift, div_out=self.div,
                                        tt=self.tt, **({"high_precision": True} if high_precision else {}))
        self.graph, _ = _capture(run)          # (no no_grad around it: the Hutchinson term differentiates the U-Net)

    def set_context(self, ctx):
        self.ctx["emb"].copy_(ctx["emb"])
        for dst, src in zip(self.ctx["coeffs"], ctx["coeffs"]):
            dst.copy_(src)

    def __call__(self, t, x, probe, drift_out, div_out=None):
        self.x.copy_(x.reshape(self.B, D))
        if self.with_div:
            self.probe.copy_(probe.reshape(self.B, D))
        self.tt.fill_(float(np.float32(t)))
        self.graph.replay()
        drift_out.copy_(self.drift.view_as(drift_out))
        if self.with_div:
            div_out.copy_(self.div.view_as(div_out))


def ode_function(model, params, ctx, B, device, with_div, graph=None, cache=None, high_precision=False):
    """-> f(t, x [B, 3072], probe | None, drift_out, div_out | None): VDM.reverse_ode as the ODE solvers call it; a
    replayed HIP graph by default (MULAN_ODE_GRAPH), eager where the capture fails (logged).  cache (a dict the caller
    keeps while the weights stay as they are): the captured graph of a batch size is re-used for the next batch / the
    next importance sample with its context re-targeted (the packed weights live in persistent buffers, ops.ParamPacker)"""
    def graphed():
        # the key names what the captured kernels were chosen by: batch, with / without the divergence term and the
        # arithmetic mode (as GraphedStep.matches does; the developer tuning words of mulan_set_tuning are not product
        # state: a caller that flips them drops the cache); the parameter tree is held by the entry and compared by identity -- an id() alone could be re-used by a new tree once the old one is freed
        # (ADVICE r05).  drop_ode_graphs(cache) releases the graph's private pool (a forward + backward pass of
        # activations) when the caller goes back to training.
        key = (B, bool(with_div), ops.CONV_MODE, bool(high_precision))
        hit = cache.get(key) if cache is not None else None
        if hit is not None and hit.params is params:
            hit.set_context(ctx)
            return hit
        g = GraphedOdeFunction(model, params, ctx, B, device, with_div, high_precision)
        if cache is not None:
            cache.clear()            # (one graph at a time: its pool holds a forward + backward pass of activations)
            cache[key] = g
        return g

    hp = {"high_precision": True} if high_precision else {}
    eager = lambda t, x, probe, drift_out, div_out=None: model.reverse_ode(params, x, ctx, t, probe,
                                                                           drift_out=drift_out, div_out=div_out, **hp)
    return _graphed_or_eager(ODE_GRAPH if graph is None else graph, device, graphed, lambda: eager,
                             "HIP-graph capture of the ODE function evaluation failed (%s: %s); evaluating eagerly")


def drop_ode_graphs(cache):
    """Release the captured ODE function evaluations of `cache` (the dict handed to ode_function) and their private
    memory pools: call it when the likelihood evaluation is over and training continues."""
    if cache:
        cache.clear()
        torch.cuda.empty_cache()


def resnet_block(p, x1, x2, cond, drop):
    """ResnetBlock.__call__ (ldm/model_vdm.py:618-657 / ldm/ldm_unet.py:18-61) on [x1|x2]."""
    # Each (norm + swish [+ dropout]) -> conv pair is one op: the normalised tensor goes from the GroupNorm kernel to the
    # convolution as split fp16 planes (ops.GnConv3x3Fn; two ops with an fp32 tensor in between where that does not
    # apply).  s1 / s2 alias x1 / x2 for the skip path: their gradients are added inside the GroupNorm backward kernel.
    cb = ops.cond_proj(cond, p["cond_proj"]["kernel"])       # [B,E] or [B,1024,E]
    h, s1, s2 = ops.gn_conv3x3(x1, x2, p["GroupNorm_0"]["scale"], p["GroupNorm_0"]["bias"], p["conv1"]["kernel"],
                               p["conv1"]["bias"], cbias=cb, act=True, skip=True)
    keep, seed, off = drop.next()
    if "nin_shortcut" in p:
        if x2 is None:
            res = ops.linear(s1, p["nin_shortcut"]["kernel"], p["nin_shortcut"]["bias"])
        else:
            res = ops.linear2(s1, s2, p["nin_shortcut"]["kernel"], p["nin_shortcut"]["bias"])
    else:
        res = s1
    # (h = conv1's output has no other consumer: its gradient may travel as split planes only, ops.GRAD_PLANES)
    return ops.gn_conv3x3(h, None, p["GroupNorm_1"]["scale"], p["GroupNorm_1"]["bias"], p["conv2"]["kernel"],
                          p["conv2"]["bias"], res=res, act=True, keep=keep, seed=seed, offset=off, x1_grad_planes=True)


def attn_block(p, x):
    """AttnBlock.__call__ with num_heads = 1 (ldm/model_vdm.py:668-701)."""
    h = ops.group_norm(x, None, p["GroupNorm_0"]["scale"], p["GroupNorm_0"]["bias"], act=False)
    q = ops.linear(h, p["q"]["kernel"], p["q"]["bias"])
    k = ops.linear(h, p["k"]["kernel"], p["k"]["bias"])
    v = ops.linear(h, p["v"]["kernel"], p["v"]["bias"])
    o = ops.attention(q, k, v)
    return ops.linear(o, p["proj_out"]["kernel"], p["proj_out"]["bias"], res=x)


def _unet_stem(p, z, t, conditioning, E, n_layers, per_pixel, with_attention, drop, with_skips=True):
    """conv_in .. mid.block_2 shared by ScoreUNet, ldm UNet and UnetEncoder."""
    if per_pixel:
        # ldm_unet.py:82-90: temb over t.reshape(-1) -> [B,32,32,3E]; dense0(concat[temb, c]) is evaluated as
        # temb @ W[:3E] + broadcast(c @ W[3E:] + b) so the per-pixel concat is never materialised.
        B = z.shape[0]
        none = torch.empty((B * D, 0), device=z.device, dtype=torch.float32)
        temb3 = ops.cond_input(t.reshape(-1), none, E).view(B * HW, 3 * E)
        w0 = p["dense0"]["kernel"]
        cs = ops.linear(conditioning, w0[3 * E:], p["dense0"]["bias"])
        cond = ops.silu(ops.linear(temb3, w0[:3 * E], None, res=ops.row_broadcast(cs, HW)))
    else:
        cond = ops.silu(ops.linear(ops.cond_input(t, conditioning, E), p["dense0"]["kernel"], p["dense0"]["bias"]))
    cond = ops.silu(ops.linear(cond, p["dense1"]["kernel"], p["dense1"]["bias"]))
    if per_pixel:
        cond = cond.view(z.shape[0], HW, -1)
    h = ops.conv3x3(ops.fourier_features(z), p["conv_in"]["kernel"], p["conv_in"]["bias"])
    # every level output feeds the next block and (in the U-Nets with an up path) a skip connection: ops.tee /
    # ops.tee_take arrange for the two gradients to be summed inside the next block's GroupNorm backward kernel
    h, skip = ops.tee(h) if with_skips else (h, h)
    hs = [skip]
    for i in range(n_layers):
        h = resnet_block(p[f"down.block_{i}"], h, None, cond, drop)
        if with_attention:
            h = attn_block(p[f"down.attn_{i}"], h)
        h, skip = ops.tee(h) if with_skips else (h, h)
        hs.append(skip)
    h = resnet_block(p["mid.block_1"], h, None, cond, drop)
    h = attn_block(p["mid.attn_1"], h)
    h = resnet_block(p["mid.block_2"], h, None, cond, drop)
    return h, hs, cond


def score_unet(p, cfg, z, g_t, conditioning, drop, time=False):
    """ScoreUNet.__call__ (ldm/model_vdm.py:314-388) / ldm_unet.UNet.__call__ (ldm/ldm_unet.py:69-142).
    z [B,1024,3]; g_t [B] (vdm) or [B,1024,3] (ldm); conditioning [B,K]."""
    per_pixel = cfg.unet_type == 'ldm'
    E, L = cfg.sm_n_embd, cfg.sm_n_layer
    t = g_t if (time and not per_pixel) else (g_t - cfg.gamma_min) / (cfg.gamma_max - cfg.gamma_min)
    h, hs, cond = _unet_stem(p, z, t, conditioning, E, L, per_pixel, cfg.with_attention, drop)
    for i in range(L + 1):
        h = resnet_block(p[f"up.block_{i}"], h, ops.tee_take(hs.pop()), cond, drop)
        if cfg.with_attention:
            h = attn_block(p[f"up.attn_{i}"], h)
    assert not hs
    h = ops.group_norm(h, None, p["GroupNorm_0"]["scale"], p["GroupNorm_0"]["bias"], act=True)
    return ops.conv3x3(h, p["conv_out"]["kernel"], p["conv_out"]["bias"], res=z)


def unet_encoder(p, cfg, f, drop):
    """UnetEncoder.__call__ (ldm/model_mulan_epsilon.py:101-154): f [B,1024,3] -> logits [B,latent_size]; latent_type
    'gaussian': UnetEncoderGaussian (ldm/model_mulan_epsilon.py:24-80) -> (mu, s) with s the pre-softplus head"""
    B = f.shape[0]
    E = cfg.sm_n_embd
    t = torch.zeros(B, device=f.device)
    conditioning = torch.zeros((B, 1), device=f.device)
    h, _, _ = _unet_stem(p, f, t, conditioning, E, cfg.forward_n_layer, False, cfg.with_attention, drop, with_skips=False)
    h = ops.group_norm(h, None, p["GroupNorm_0"]["scale"], p["GroupNorm_0"]["bias"], act=True)
    h = ops.conv3x3(h, p["conv_out"]["kernel"], p["conv_out"]["bias"])          # [B,1024,1]
    h = ops.silu(h.view(B, HW))
    if cfg.latent_type == 'gaussian':
        return (ops.linear(h, p["dense_layer_final_mu"]["kernel"], p["dense_layer_final_mu"]["bias"]),
                ops.linear(h, p["dense_layer_final_sigma"]["kernel"], p["dense_layer_final_sigma"]["bias"]))
    return ops.linear(h, p["dense_layer_final"]["kernel"], p["dense_layer_final"]["bias"])


LATENT_TYPES = ('topk', 'gumbel', 'gaussian')


def gumbel_tau(step):
    """the Gumbel-softmax temperature max(0.5, exp(-1e-5 step)) in fp32, as jnp evaluates it
    (ldm/model_mulan_velocity.py:87-90)"""
    return float(np.maximum(np.float32(0.5), np.exp(np.float32(-1e-5) * np.float32(step))))


def poly_coefficients(p, emb):
    """NoiseSchedule_polynomial_fixedend._compute_coefficients (ldm/model_mulan_epsilon.py:531-538)"""
    h = ops.silu(ops.linear(emb, p["dense_1"]["kernel"], p["dense_1"]["bias"]))
    h = ops.silu(ops.linear(h, p["dense_2"]["kernel"], p["dense_2"]["bias"]))
    a = ops.linear(h, p["dense_out_a"]["kernel"], p["dense_out_a"]["bias"])
    b = ops.linear(h, p["dense_out_b"]["kernel"], p["dense_out_b"]["bias"])
    c = ops.softplus_shift(ops.linear(h, p["dense_out_c"]["kernel"], p["dense_out_c"]["bias"]), 1e-3)
    return a, b, c


def encode_images(images_u8):
    """EncDec.encode (ldm/model_vdm.py:274-280) as a device tensor [B,1024,3] (exact in fp32)."""
    return ops.encode_u8(images_u8.reshape(images_u8.shape[0], HW, 3))


# ----------------------------------------------------------------------------- VDM variants
class _VDMBase:
    """What runs a trained model -- the ancestral step (_reverse_step), the few-step samplers (_fast_step), the
    probability-flow ODE (_ode_eval) and decoding (generate_x) -- is written once here, over what a model supplies (ctx:
    its per-batch context, fast_context / ode_context):
      _fast_gamma(params, ctx, t) ...... gamma at the times of a [B] device tensor; _fast_gamma_shape(B): its shape
      _ode_gamma(params, ctx, t) ....... (gamma, d gamma / d t) there
      _fast_net(params, z, g_t, ctx) ... the network output at z [B, 3072] for that gamma
      _fast_mode(), _ancestral_mode(), _ode_mode() ... how mulan_fast_sampler_step, mulan_ancestral_step and
          mulan_ode_drift / mulan_ode_div read that output: three words, since each kernel numbers its own forms
      _g_0(params, coeffs, B, device) .. gamma at t = 0, for decoding
      reverse_ode(params, x, ctx, t, hutch, drift_out, div_out) ... forms the inputs of _ode_eval"""

    def __init__(self, config: VDMConfig):
        self.config = config

    def _noise(self, rngs, noise, B, device, need_gamma):
        """Draw (t0, raw Gamma, eps_0, eps) in the reference's make_rng('sample') order
        (ldm/model_mulan_velocity.py:195, :95-96 via :210, :223, :235) unless given explicitly.  The latent's draw takes
        the second slot whatever the latent: Gumbel noise [B,L] for latent_type 'gumbel' (:70), eps_z [B,L] for
        'gaussian' (:134)."""
        noise = dict(noise or {})
        key = rngs.get("sample") if rngs else None
        gkey = self._latent_noise_key()
        tkey = "t0" if self.config.antithetic_time_sampling else "t"
        if any(k not in noise for k in (tkey, "eps_0", "eps")) or (need_gamma and gkey not in noise):
            if key is None:
                raise ValueError("VDM.apply needs rngs={'sample': Key} or explicit noise")
            k_t, k_g, k_0, k_e = key.split(4)
            noise.setdefault("t0", k_t.uniform())
            if not self.config.antithetic_time_sampling:    # t ~ U[0,1)^B (ldm/model_mulan_velocity.py:199-200)
                noise.setdefault("t", ops.noise((B,), k_t.v, 0, device, "uniform"))
            if need_gamma:
                cfg = self.config
                if gkey == "eps_z":
                    noise.setdefault("eps_z", k_g.normal((B, cfg.latent_size), device))
                elif gkey == "gumbel":
                    noise.setdefault("gumbel", ops.noise((B, cfg.latent_size), k_g.v, 0, device, "gumbel"))
                else:
                    noise.setdefault("gamma_raw", k_g.gamma(1.0 / cfg.latent_k, (10, B, cfg.latent_size), device))
            noise.setdefault("eps_0", k_0.normal((B, D), device))
            noise.setdefault("eps", k_e.normal((B, D), device))
        return noise

    def _latent_noise_key(self):
        cfg = self.config
        if getattr(cfg, 'latent_type', 'topk') == 'gaussian':
            return "eps_z"
        if getattr(cfg, 'latent_type', 'topk') == 'gumbel' or cfg.topk_noise_type == 'gumbel':
            return "gumbel"
        return "gamma_raw"

    def _times(self, noise, B, device):
        cfg = self.config
        T = cfg.sm_n_timesteps
        if not cfg.antithetic_time_sampling:
            t = noise["t"].to(device=device, dtype=torch.float32).reshape(B)
            return torch.ceil(t * T) / T if T > 0 else t
        t0 = noise["t0"]
        # t = mod(t0 + arange(0, 1, 1/B), 1)  (ldm/model_mulan_velocity.py:196-198), built in fp32 like jnp
        # (evaluated on the device: the same IEEE fp32 multiply / add / floor as on the host, and no blocking
        # host-to-device copy, which would make the host wait for the whole previous step)
        # (t0 may be a 0-dim fp32 device tensor: a stream-ordered parameter under HIP-graph replay)
        t0v = t0.to(device=device, dtype=torch.float32) if torch.is_tensor(t0) else float(np.float32(t0))
        t = torch.remainder(torch.arange(B, dtype=torch.float32, device=device) * float(np.float32(1.0 / B)) + t0v, 1.0)
        if T > 0:
            t = torch.ceil(t * T) / T
        return t

    def __call__(self, params, *a, **kw):
        return self.apply(params, *a, **kw)

    # ---- ancestral sampler and decoding ---------------------------------------------------------------------------
    def _step_inputs(self, i, T, z_t, rng):
        """-> reverse step i of T: z_t as [B, 3072], its noise (rng folded with i), t = (T-i)/T, s = (T-i-1)/T as [B]"""
        B = z_t.shape[0]
        z = z_t.reshape(B, D).contiguous()
        eps = rng.fold_in(i).normal((B, D), z.device)
        t = torch.full((B,), float(np.float32((T - i) / T)), device=z.device, dtype=torch.float32)
        s = torch.full((B,), float(np.float32((T - i - 1) / T)), device=z.device, dtype=torch.float32)
        return z, eps, t, s

    def _reverse_step(self, params, z, eps, t, s, ctx):
        """the device work of one reverse step t -> s: z, eps [B, 3072]; t, s [B] device tensors"""
        g_t = self._fast_gamma(params, ctx, t)
        g_s = self._fast_gamma(params, ctx, s)
        net = self._fast_net(params, z, g_t, ctx)
        return ops.ancestral_step(z, net, g_t, g_s, eps, self._ancestral_mode())

    def generate_x(self, params, z_0, coeffs=None, rng=None):
        """argmax of the decoder logits, or with sample_softmax a categorical draw (rng: the 'sample' Key)"""
        if self.config.sample_softmax and rng is None:
            raise ValueError("sample_softmax=True needs rng (the reference's make_rng('sample'))")
        with torch.no_grad():
            B = z_0.shape[0]
            g_0 = self._g_0(params, coeffs, B, z_0.device)
            if self.config.sample_softmax:
                return ops.decode_sample(z_0.reshape(B, D), g_0, rng.v).view(B, 32, 32, 3)
            return ops.decode_argmax(z_0.reshape(B, D), g_0).view(B, 32, 32, 3)

    # ---- probability-flow ODE ---------------------------------------------------------------------------------------
    def _ode_eval(self, params, x, gt, gp, g_in, cond, mode, hutch, drift_out, div_out):
        """the drift at x [B, 3072] for gamma gt and its time derivative gp (g_in: gamma as the network takes it); with
        `hutch` also the Hutchinson estimate hutch^T (d drift / d x) hutch per sample through the U-Net's input
        gradient (notebook_utils._get_value_div_fn): -> (drift, div | None)"""
        cfg = self.config
        B = x.shape[0]
        xin = x.detach().reshape(B, D).contiguous()
        if hutch is None:
            with torch.no_grad():
                net = score_unet(params["score_model"], cfg, xin.view(B, HW, 3), g_in, cond, _Drop(None, 0.0))
                drift, _ = ops.ode_drift(net.reshape(B, D), xin, gt, gp, None, mode, drift_out)
            return drift, None
        xin.requires_grad_(True)
        with torch.enable_grad():
            net = score_unet(params["score_model"], cfg, xin.view(B, HW, 3), g_in, cond, _Drop(None, 0.0))
        drift, cot = ops.ode_drift(net.detach().reshape(B, D), xin.detach(), gt, gp, hutch, mode, drift_out)
        (gx,) = torch.autograd.grad(net, xin, cot.view_as(net))
        return drift, ops.ode_div(gx.reshape(B, D), gt, gp, hutch, mode, div_out)

    # ---- few-step samplers (mulan_amd.sampling; not in the reference) ----------------------------------------------
    def _fast_step(self, params, z, t, s, g_prev, x_prev, ctx, xi=None, step_eta=0.0, known=None, mask=None,
                   known_xi=None, measurement=None, restore=None):
        """the device work of one step t -> s: (z_s, x_hat_t, gamma_t); g_prev / x_prev None: first order; xi [B, 3072]
        with step_eta > 0: the stochastic step on that noise; known / mask [B, 3072] (inpainting): the known sub-pixels
        of z_s are then replaced by alpha_s known + sigma_s known_xi (known_xi None: zero noise); measurement with
        restore = (f, gray): the prediction is projected onto the measurement and the step runs on x_hat' at mode 2, so
        the x_hat_t returned is x_hat'"""
        from . import sampling
        g_t = self._fast_gamma(params, ctx, t)
        g_s = self._fast_gamma(params, ctx, s)
        z_s, x0 = sampling.solver_step(z, self._fast_net(params, z, g_t, ctx), g_t, g_s, self._fast_mode(),
                                       (g_prev, x_prev), xi, step_eta, known, mask, known_xi, measurement, restore, HWC)
        return z_s, x0, g_t

    def fast_stepper(self, params, B, device, ctx, graph=None, step_eta=0.0, inpaint=False, restore=None):
        """-> step(z, t, s, order[, k]) of the few-step samplers: a replayed HIP graph (GraphedFastStep) by default
        (MULAN_SAMPLER_GRAPH), eager where the capture fails (logged) or graph=False (EagerFastStep); both take the next
        batch's context through set_context().  step_eta > 0 (the eta the steps run with, what sampling.check_eta
        makes of a sampler and its `eta` keyword: 1 for sde2m): the stochastic step, whose noise the
        stepper draws for step k from what set_noise() names.  inpaint: a stepper that replaces the known sub-pixels
        after every step, on the image, mask and known-region noise of set_known(); it serves inpainting runs only,
        and a stepper built without serves none.  restore = (f, gray) (sampling.parse_degradation): a stepper that
        projects every prediction onto the measurement of set_measurement(); it serves restoring runs of that
        degradation only"""
        return _graphed_or_eager(SAMPLER_GRAPH if graph is None else graph, device,
                                 lambda: GraphedFastStep(self, params, B, device, ctx, step_eta, inpaint, restore),
                                 lambda: EagerFastStep(self, params, B, device, ctx, step_eta, inpaint, restore),
                                 "HIP-graph capture of the few-step sampler's step failed (%s: %s); sampling eagerly")

    def schedule_ends(self, params, ctx):
        """-> (gamma_bar(0), gamma_bar(1)) of the batch's mean schedule, as floats"""
        raise NotImplementedError

    def schedule_times(self, params, ctx, targets):
        """-> fp32 [M] on the device: the times in [0, 1] at which the batch's mean schedule gamma_bar takes the values
        `targets` (float64 [M]); what the 'logsnr' and 'karras' grids of the few-step samplers are made of
        (sampling.make_grid)"""
        raise NotImplementedError

    def fast_grid(self, params, ctx, steps=None, t_grid=None, grid="uniform", grid_rho=7.0):
        """-> the time grid of a few-step run on this batch (sampling.make_grid): float64 [N + 1].  A 'logsnr' or
        'karras' grid costs schedule_times on the batch's context and one read of N - 1 floats"""
        from . import sampling
        return sampling.make_grid(grid, steps, t_grid, grid_rho, lambda: self.schedule_ends(params, ctx),
                                  lambda targets: self.schedule_times(params, ctx, targets))

    def fast_sample(self, params, z, ctx, sampler="dpm2m", steps=None, t_grid=None, graph=None, stepper=None, eta=0.0,
                    noise=None, known=None, mask=None, resample=1, known_noise=None, measurement=None,
                    degradation=None, grid="uniform", grid_rho=7.0):
        """z_0 from z_1 = z [B, 3072] by `sampler` (ddim | dpm2m | sde2m) over `steps` steps on the grid kind `grid`
        (sampling.GRIDS; 'uniform': uniform in t; 'logsnr' and 'karras', with grid_rho, are spaced on the mean schedule
        of this batch: fast_grid) or the explicit t_grid; stepper: one from fast_stepper to re-use (its set_context re-targets it at this batch's ctx).
        eta: for ddim (0: the deterministic sampler).  noise (sde2m, ddim with eta > 0): the batch's step key -- step k
        draws xi = randn under noise.fold_in(k) -- or a callable k -> xi [B, 3072].
        known (fp32 [B, 3072], the image as ops.encode_u8 gives it) and mask (uint8 or bool [B, 3072], non-zero = keep):
        inpainting (sampling.run) with `resample` passes per step.  known_noise: the batch's known-region key --
        draw j of the run (the noise of the known region at a mix, or of a jump; sampling.run states which j is drawn
        when) is randn under known_noise.fold_in(j) -- or a callable j -> xi [B, 3072].  It is a key of its own: step k
        keeps drawing under noise.fold_in(k), and round r of a resampled step k under noise.fold_in(k + r N).
        measurement (fp32, shaped ops.restore_y_shape(B, 32, 32, 3, f, gray), in the scale of ops.encode_u8) and
        degradation ('sr:f', 'gray', 'sr:f+gray' or the pair (f, gray)): restoration instead (sampling.run) with
        `resample` passes per step; jump j of a run with resample > 1 draws under known_noise.fold_in(j), and a run with
        resample = 1 needs no known_noise"""
        from . import sampling
        step_eta = sampling.check_eta(sampler, eta)
        inpaint, restore, resample = sampling.check_guidance(sampler, known, mask, measurement, degradation, resample)
        grid, grid_rho = sampling.check_grid(sampler, grid, t_grid, grid_rho)
        B = z.shape[0]
        if restore is not None:
            shape = ops.restore_y_shape(B, *HWC, *restore)
            if not torch.is_tensor(measurement) or measurement.dtype != torch.float32 or tuple(measurement.shape) != shape:
                got = (f"{measurement.dtype} {list(measurement.shape)}" if torch.is_tensor(measurement)
                       else type(measurement).__name__)
                raise ValueError(f"fast_sample: the measurement of {degradation!r} is fp32 {list(shape)}; got {got}")
            if resample > 1 and known_noise is None:
                raise ValueError("fast_sample: resample > 1 needs `known_noise` (the key of the jumps' noise)")
        if inpaint:
            if known.dtype != torch.float32 or tuple(known.shape) != (B, D):
                raise ValueError(f"fast_sample: known is the encoded image, fp32 [{B}, {D}]; got {known.dtype} "
                                 f"{tuple(known.shape)}")
            if mask.dtype not in (torch.uint8, torch.bool) or tuple(mask.shape) != (B, D):
                raise ValueError(f"fast_sample: mask is uint8 or bool [{B}, {D}]; got {mask.dtype} {tuple(mask.shape)}")
            if known_noise is None:
                raise ValueError("fast_sample: inpainting needs `known_noise` (the batch's known-region key)")
        with torch.no_grad():
            grid = self.fast_grid(params, ctx, steps, t_grid, grid, grid_rho)
        orders = sampling.step_orders(sampler, len(grid) - 1)
        if step_eta > 0.0 and noise is None:
            raise ValueError(f"fast_sample: {sampler!r} with eta = {step_eta} is stochastic and needs `noise`")
        with torch.no_grad():
            if stepper is None:
                stepper = self.fast_stepper(params, B, z.device, ctx, graph, step_eta, inpaint, restore)
            elif not hasattr(stepper, "set_context"):
                raise TypeError("fast_sample: a re-used stepper must take the batch's context (set_context): "
                                f"{type(stepper).__name__} cannot be re-targeted")
            else:
                stepper.check_serves(step_eta, inpaint, restore)
                stepper.set_context(ctx)
            if step_eta > 0.0:
                stepper.set_noise(noise)
            if inpaint:
                stepper.set_known(known, mask, known_noise)
            if restore is not None:
                stepper.set_measurement(measurement, known_noise)
            return sampling.run(stepper, z.reshape(B, D).contiguous(), grid, orders, resample)


class MulanVDM(_VDMBase):
    """model_mulan_velocity.VDM / model_mulan_epsilon.VDM selected by `parameterization`."""

    def __init__(self, config: VDMConfig, parameterization: str):
        super().__init__(config)
        assert parameterization in ("velocity", "epsilon")
        self.parameterization = parameterization
        c = config
        if c.latent_type not in LATENT_TYPES or c.encoder != 'unet' or c.gamma_type != 'poly_fixedend':
            raise NotImplementedError(
                "hot path covers latent_type=topk|gumbel|gaussian, encoder=unet, gamma_type=poly_fixedend; "
                f"got {c.latent_type}/{c.encoder}/{c.gamma_type}")
        if c.latent_type == 'topk' and (c.topk_noise_type not in ('gamma', 'gumbel') or
                                        (c.topk_noise_type == 'gumbel' and parameterization != "epsilon")):
            raise ValueError("topk_noise_type: 'gamma' (both models) or 'gumbel' (model_mulan_epsilon only, "
                             "ldm/model_mulan_epsilon.py:236-239)")
        if parameterization == "velocity" and c.sm_n_timesteps != 0:
            raise AssertionError("model_mulan_velocity asserts T == 0 (ldm/model_mulan_velocity.py:255)")

    def init(self, rng: Key):
        c = self.config
        gen = torch.Generator().manual_seed(rng.v & ((1 << 63) - 1))
        E = c.sm_n_embd
        K = c.latent_size if c.z_conditioning else 1
        temb = 3 * E if c.unet_type == 'ldm' else E
        score = _unet_init(gen, E, c.sm_n_layer, temb + K, 3, True, c.with_attention)
        enc = _unet_init(gen, E, c.forward_n_layer, E + 1, 1, False, c.with_attention)
        if c.latent_type == 'gaussian':      # UnetEncoderGaussian (ldm/model_mulan_epsilon.py:76-79)
            enc["dense_layer_final_mu"] = _dense(gen, HW, c.latent_size)
            enc["dense_layer_final_sigma"] = _dense(gen, HW, c.latent_size)
        else:
            enc["dense_layer_final"] = _dense(gen, HW, c.latent_size)
        lat = c.latent_size if c.reparam_type == 'true' else 10
        gamma = {"dense_1": _dense(gen, lat, D), "dense_2": _dense(gen, D, D),
                 "dense_out_a": _dense(gen, D, D, zero=True), "dense_out_b": _dense(gen, D, D),
                 "dense_out_c": _dense(gen, D, D)}
        return {"score_model": score, "encoder_model": enc, "gamma": gamma}

    def apply(self, params, images, labels=None, conditioning=None, step=0, rngs=None, deterministic=True,
              noise=None, return_aux=False, same_image=False, profile_rows=0):
        """same_image (not in the reference): the caller vouches that every row of `images` is the same image (the dense
        variational-bound evaluator tiles one test image n_timesteps times, ldm/notebook_utils.py:181-186).  The encoder
        U-Net sees neither t nor the noise, so in evaluation mode its logits are identical for all rows: it then runs on
        one row and the logits are broadcast (7 % of the evaluator's FLOPs; same bits).
        profile_rows = R > 0 (not in the reference; B a multiple of R): returns (output, profile) instead, the profile
        of this very pass -- its noise, times and network output -- as a dict: rows [B, 8] and cols [B / R, 3, 3072] of
        ops.bound_profile, the latent KL kl_z [B] (which loss_klz includes) and the times t [B]."""
        cfg = self.config
        dev = images.device
        x = images.reshape(-1, D).contiguous()
        if x.dtype != torch.uint8:
            x = torch.round(x).to(torch.uint8)
        B = x.shape[0]
        noise = self._noise(rngs, noise, B, dev, cfg.reparam_type == 'true')
        t = self._times(noise, B, dev)
        f = encode_images(x)
        # rngs['dropout_pair']: the two sub-keys already split (and bound to device slots) by a graphed train step
        pair = None if deterministic else (rngs or {}).get("dropout_pair")
        drop_key = None if deterministic else (rngs or {}).get("dropout")
        if not deterministic and drop_key is None and pair is None:
            raise ValueError("training mode needs rngs['dropout']")
        k_enc, k_score = pair if pair is not None else (drop_key.split(2) if drop_key is not None else (None, None))
        if cfg.reparam_type == 'true':
            if same_image and deterministic and B > 1:
                logits = unet_encoder(params["encoder_model"], cfg, f[:1].contiguous(), _Drop(None, 0.0))
                if cfg.latent_type == 'gaussian':        # both heads; eps_z still differs per row
                    logits = tuple(h.expand(B, h.shape[1]).contiguous() for h in logits)
                else:
                    logits = logits.expand(B, logits.shape[1]).contiguous()
            else:
                logits = unet_encoder(params["encoder_model"], cfg, f, _Drop(k_enc, cfg.sm_pdrop))
            if cfg.latent_type == 'gaussian':           # ldm/model_mulan_velocity.py:132-138
                emb, kl_z = ops.gaussian_embedding(logits[0], logits[1], noise["eps_z"])
            elif cfg.latent_type == 'gumbel':           # ldm/model_mulan_velocity.py:85-92
                tau = noise.get("tau")
                if tau is None:
                    tau = torch.full((), gumbel_tau(step), device=dev, dtype=torch.float32)
                emb, kl_z = ops.gumbel_embedding(logits, noise["gumbel"], tau)
            elif cfg.topk_noise_type == 'gumbel':
                emb, kl_z = ops.topk_embedding(logits, noise["gumbel"], cfg.latent_k, tau=-1.0)
            else:
                emb, kl_z = ops.topk_embedding(logits, noise["gamma_raw"], cfg.latent_k)
        else:   # ldm/model_mulan_velocity.py:212-214
            emb = torch.nn.functional.one_hot(labels.long(), 10).to(torch.float32)
            kl_z = torch.zeros(B, device=dev)
        a, b, c = poly_coefficients(params["gamma"], emb)
        g0, g1, gt, gp = ops.poly_gamma(a, b, c, t, cfg.gamma_min, cfg.gamma_max)
        zt, gbar, loss_recon, loss_klz, v0, v1 = ops.qsample(x, g0, g1, gt, noise["eps_0"], noise["eps"])
        if cfg.z_conditioning:
            cond = emb
        else:
            cond = conditioning.reshape(B, 1).to(torch.float32)
        g_in = gt.view(B, HW, 3) if cfg.unet_type == 'ldm' else gbar
        net = score_unet(params["score_model"], cfg, zt.view(B, HW, 3), g_in, cond, _Drop(k_score, cfg.sm_pdrop))
        net = net.reshape(B, D)
        T = cfg.sm_n_timesteps
        mode, w = 2, gp
        if self.parameterization == "velocity":
            mode = 1 if cfg.velocity_from_epsilon else 0
        elif T > 0:
            # finite depth T (ldm/model_mulan_epsilon.py:348-355): s = t - 1/T, weight T * expm1(g_t - g_s)
            _, _, gs, _ = ops.poly_gamma(a, b, c, t - 1.0 / T, cfg.gamma_min, cfg.gamma_max)
            w = ops.expm1_weight(gt, gs, T)
        loss_diff = ops.diffusion_loss(mode, x, gt, w, noise["eps"], zt, net)
        out = VDMOutput(loss_recon=loss_recon, loss_klz=kl_z + loss_klz, loss_diff=loss_diff, var_0=v0.mean(),
                        var_1=v1.mean())
        if profile_rows:
            rows, cols = ops.bound_profile(mode, x, g0, g1, gt, w, noise["eps_0"], noise["eps"], zt, net, profile_rows)
            return out, dict(rows=rows, cols=cols, kl_z=kl_z, t=t)
        if return_aux:
            return out, dict(emb=emb, zt=zt, net=net, gt=gt, gp=gp, t=t, logits=logits if cfg.reparam_type == 'true' else None)
        return out

    # ---- ancestral sampler (ldm/model_mulan_velocity.py:270-368, ldm/model_mulan_epsilon.py:365-460) ----------
    def deterministic_embedding(self, B, device):
        """_get_deterministic_embedding (ldm/model_mulan_velocity.py:270-279): topk: the first latent_k entries set;
        gumbel: one_hot(ones(B)), i.e. entry 1 set; gaussian: zeros"""
        c = self.config
        emb = torch.zeros((B, c.latent_size), device=device, dtype=torch.float32)
        if c.latent_type == 'gumbel':
            emb[:, 1] = 1.0
        elif c.latent_type == 'topk':
            emb[:, :c.latent_k] = 1.0
        return emb

    def sample_coefficients(self, params, embedding):
        """(a, b, c) of the per-pixel schedule for an embedding: constant over the T steps of a sampling run"""
        with torch.no_grad():
            return poly_coefficients(params["gamma"], embedding)

    def _ancestral_mode(self):
        return 0 if self.parameterization == "velocity" else 1      # (velocity_from_epsilon does not reach the sampler)

    def conditional_sample(self, params, i, T, z_t, embedding, conditioning, rng, coeffs=None):
        """one reverse step t = (T-i)/T -> s = (T-i-1)/T given the latent embedding; z_t [B,32,32,3] (any layout with
        B x 3072 elements); rng: Key, folded with i like the reference"""
        with torch.no_grad():
            z, eps, t, s = self._step_inputs(i, T, z_t, rng)
            if coeffs is None:
                coeffs = self.sample_coefficients(params, embedding)
            z_s = self._reverse_step(params, z, eps, t, s, dict(emb=embedding, cond=conditioning, coeffs=coeffs))
        return z_s.view(z_t.shape)

    def reverse_stepper(self, params, B, device, embedding, conditioning, coeffs, T, graph=None):
        """-> step(i, z, rng) running conditional_sample's reverse step; with `graph` (default: MULAN_SAMPLER_GRAPH, on)
        as a replayed HIP graph (GraphedReverseStep): five launches per step from the host instead of ~450.  Measured on
        an idle host it buys nothing (9.66 vs 9.67 ms per step at 16 images, 10.9 vs 10.9 at 64, 18.6 vs 18.7 at 128): below
        ~100 images the step is bound by the latency of its ~450 dependent launches (every one a single round of at most
        256 blocks), not by the host; the replay keeps it that way when the host is busy (data loading, other ranks)."""
        graphed = lambda: GraphedReverseStep(self, params, B, device, embedding, conditioning, coeffs, T).step
        eager = lambda i, z, rng: self.conditional_sample(params, i, T, z, embedding, conditioning, rng, coeffs)
        return _graphed_or_eager(SAMPLER_GRAPH if graph is None else graph, device, graphed, lambda: eager,
                                 "HIP-graph capture of the sampler's reverse step failed (%s: %s); sampling eagerly")

    def sample(self, params, i, T, z_t, conditioning, rng, coeffs=None):
        emb = self.deterministic_embedding(z_t.shape[0], z_t.device)
        return self.conditional_sample(params, i, T, z_t, emb, conditioning, rng, coeffs)

    def _g_0(self, params, coeffs, B, device):
        if coeffs is None:
            coeffs = self.sample_coefficients(params, self.deterministic_embedding(B, device))
        return self._fast_gamma(params, dict(coeffs=coeffs), torch.zeros(B, device=device, dtype=torch.float32))

    # ---- the samplers' context and hooks (_VDMBase): the few-step samplers read the network output as
    # velocity_from_epsilon reads it in reverse_ode (mode 1 = eps_hat)
    def fast_context(self, params, embedding, conditioning, coeffs=None):
        """the per-batch context of fast_sample: the embedding, the conditioning and the schedule coefficients"""
        B = embedding.shape[0]
        if coeffs is None:
            coeffs = self.sample_coefficients(params, embedding)
        return dict(emb=embedding.contiguous(), cond=conditioning.reshape(B, 1).to(torch.float32).contiguous(),
                    coeffs=tuple(coeffs))

    def schedule_ends(self, params, ctx):
        """the fixed end points of the polynomial schedule: every sub-pixel's, so the mean's"""
        return float(self.config.gamma_min), float(self.config.gamma_max)

    def schedule_times(self, params, ctx, targets):
        """the mean over the batch's sub-pixels of the polynomial schedule is a quintic in t: its five coefficients by
        ops.schedule_moments on the batch's coefficients, its roots by ops.schedule_invert"""
        cfg = self.config
        return ops.schedule_invert(ops.schedule_moments(*ctx["coeffs"]), targets, cfg.gamma_min, cfg.gamma_max)

    def _ode_gamma(self, params, ctx, t):
        cfg = self.config
        _, _, gt, gp = ops.poly_gamma(*ctx["coeffs"], t, cfg.gamma_min, cfg.gamma_max)
        return gt, gp                                                      # [B, 3072] each

    def _fast_gamma(self, params, ctx, t):
        return self._ode_gamma(params, ctx, t)[0]

    def _fast_gamma_shape(self, B):
        return (B, D)

    def _fast_mode(self):
        if self.parameterization == "velocity":
            return 1 if self.config.velocity_from_epsilon else 0
        return 1

    def _fast_net(self, params, z, g_t, ctx):
        cfg = self.config
        B = z.shape[0]
        # (the cast: the ancestral step hands over the caller's integer conditioning; fast_context's fp32 passes as is)
        cond = ctx["emb"] if cfg.z_conditioning else ctx["cond"].reshape(B, 1).to(torch.float32)
        return score_unet(params["score_model"], cfg, z.view(B, HW, 3), self._g_in(g_t), cond,
                          _Drop(None, 0.0)).reshape(B, D)

    def _g_in(self, g_t):
        """gamma as the score model takes it: per pixel (ldm U-Net) or its mean per image"""
        return g_t.view(g_t.shape[0], HW, 3) if self.config.unet_type == 'ldm' else ops.rowmean(g_t)

    # ---- probability-flow ODE (ldm/model_mulan_velocity.py:51-53, 393-421; ldm/model_mulan_epsilon.py:459-478) ----
    def apply_encoder(self, params, images_u8):
        """VDM.apply_encoder: encoder logits [B, latent_size] of integer images (latent_type 'gaussian': the heads
        (mu, s), s before the softplus)"""
        x = images_u8.reshape(-1, D).contiguous()
        with torch.no_grad():
            return unet_encoder(params["encoder_model"], self.config, encode_images(x), _Drop(None, 0.0))

    def ode_context(self, params, images_u8):
        """per batch, constant along the ODE: hard top-k embedding of the encoder logits
        (notebook_utils.logits_to_embeddings), its KL term (_gumbel_kl_loss) and the schedule coefficients"""
        if not self.config.z_conditioning:
            raise NotImplementedError("reverse_ode hands the embedding to the score model (z_conditioning=True)")
        if self.config.latent_type == 'gaussian':
            raise NotImplementedError(
                "ODE likelihood with latent_type='gaussian': the reference's apply_encoder returns (mu, var) there and "
                "its ODE code (notebook_utils.logits_to_embeddings) cannot consume that")
        logits = self.apply_encoder(params, images_u8)
        emb, kl = ops.topk_hard(logits, self.config.latent_k)
        with torch.no_grad():
            coeffs = poly_coefficients(params["gamma"], emb)
        return dict(emb=emb, kl=kl, coeffs=coeffs, logits=logits)

    def ode_context_from_embedding(self, params, emb):
        """the same context for a given k-hot embedding (the ODE sampler draws it from random logits)"""
        with torch.no_grad():
            return dict(emb=emb, kl=None, coeffs=poly_coefficients(params["gamma"], emb), logits=None)

    def _ode_mode(self, high_precision=False):
        hp = 4 if high_precision else 0       # mulan_ode_drift / mulan_ode_div: mode | 4 = the high_precision selects
        if self.parameterization == "velocity":
            return (1 if self.config.velocity_from_epsilon else 0) | hp
        return 2 | hp

    def reverse_ode(self, params, x, ctx, t, hutch=None, drift_out=None, div_out=None, tt=None, high_precision=False):
        """VDM.reverse_ode at time t for x [B, 3072]; with `hutch` also the Hutchinson estimate
        hutch^T (d drift / d x) hutch per sample (notebook_utils._get_value_div_fn): returns (drift, div | None).
        tt (optional, [B] fp32 device tensor): the time as a stream-ordered parameter (GraphedOdeFunction) instead of t.
        high_precision: the alpha / sigma selects of ldm/model_mulan_velocity.py:410-417, model_mulan_epsilon.py:472-475"""
        if tt is None:
            tt = torch.full((x.shape[0],), float(np.float32(t)), device=x.device, dtype=torch.float32)
        with torch.no_grad():
            gt, gp = self._ode_gamma(params, ctx, tt)
            g_in = self._g_in(gt)
        return self._ode_eval(params, x, gt, gp, g_in, ctx["emb"], self._ode_mode(high_precision), hutch, drift_out,
                              div_out)


class PlainVDM(_VDMBase):
    """model_vdm.VDM (ldm/model_vdm.py:95-180): scalar noise schedule, epsilon prediction, T = 0 or T > 0
    with reparam_type 'noise' | 'input'.  gamma_type in {'fixed', 'learnable_scalar', 'learnable_nnet'}."""

    N_FEATURES = 1024      # NoiseSchedule_NNet.n_features

    def __init__(self, config: VDMConfig):
        super().__init__(config)
        if config.gamma_type not in ('fixed', 'learnable_scalar', 'learnable_nnet'):
            raise NotImplementedError(f"model_vdm.VDM gamma_type={config.gamma_type} "
                                      "(supported: fixed, learnable_scalar, learnable_nnet; the reference raises on "
                                      "poly_fixedend, ldm/model_vdm.py:101-108)")
        if config.unet_type != 'vdm':
            raise NotImplementedError("model_vdm.VDM always uses ScoreUNet")
        if config.sm_n_timesteps > 0 and config.reparam_type not in ('noise', 'input'):
            raise ValueError(f"model_vdm.VDM with T > 0 needs reparam_type noise | input, got {config.reparam_type} "
                             "(the reference leaves loss_diff undefined there, ldm/model_vdm.py:166-169)")

    def init(self, rng: Key):
        c = self.config
        gen = torch.Generator().manual_seed(rng.v & ((1 << 63) - 1))
        E = c.sm_n_embd
        p = {"score_model": _unet_init(gen, E, c.sm_n_layer, E + 1, 3, True, c.with_attention)}
        if c.gamma_type == 'learnable_scalar':   # NoiseSchedule_Scalar, ldm/model_vdm.py:418-431
            p["gamma"] = {"w": torch.tensor([c.gamma_max - c.gamma_min], dtype=torch.float32),
                          "b": torch.tensor([c.gamma_min], dtype=torch.float32)}
        elif c.gamma_type == 'learnable_nnet':   # NoiseSchedule_NNet, ldm/model_vdm.py:471-509 (normal init: stddev 0.01)
            F = self.N_FEATURES
            p["gamma"] = {"l1": {"kernel": torch.full((1, 1), c.gamma_max - c.gamma_min, dtype=torch.float32),
                                 "bias": torch.tensor([c.gamma_min], dtype=torch.float32)},
                          "l2": {"kernel": torch.randn((1, F), generator=gen) * 0.01, "bias": torch.zeros(F)},
                          "l3": {"kernel": torch.randn((F, 1), generator=gen) * 0.01}}
        return p

    def _gamma(self, params, t):
        """(gamma(t), d gamma / d t) for t [B]"""
        c = self.config
        if c.gamma_type == 'fixed':
            return c.gamma_min + (c.gamma_max - c.gamma_min) * t, torch.full_like(t, c.gamma_max - c.gamma_min)
        if c.gamma_type == 'learnable_nnet':
            # monotone network of one scalar input (DenseMonotone = |kernel|): [B, 1024] host-side autograd glue like the
            # two scalars below; the derivative the reference takes by jax.jvp is written out
            g = params["gamma"]
            F = self.N_FEATURES
            t2 = t.reshape(-1, 1)
            w1, w2, w3 = torch.abs(g["l1"]["kernel"]), torch.abs(g["l2"]["kernel"]), torch.abs(g["l3"]["kernel"])
            sg = torch.sigmoid((2.0 * (t2 - 0.5)) * w2 + g["l2"]["bias"])
            h = t2 * w1 + g["l1"]["bias"] + ((2.0 * (sg - 0.5)) @ w3) / F
            dh = w1 + ((4.0 * sg * (1.0 - sg) * w2) @ w3) / F
            return h.reshape(-1), dh.reshape(-1)
        w, b = params["gamma"]["w"], params["gamma"]["b"]
        aw = torch.abs(w)     # tiny [1]-element host-side autograd glue for the 2 schedule scalars
        return b + aw * t, aw.expand_as(t)

    def apply(self, params, images, labels=None, conditioning=None, step=0, rngs=None, deterministic=True,
              noise=None, return_aux=False, profile_rows=0):
        """profile_rows: as MulanVDM.apply takes it (per-row gammas; kl_z is zero: there is no latent)"""
        cfg = self.config
        dev = images.device
        x = images.reshape(-1, D).contiguous()
        if x.dtype != torch.uint8:
            x = torch.round(x).to(torch.uint8)
        B = x.shape[0]
        noise = self._noise(rngs, noise, B, dev, False)
        t = self._times(noise, B, dev)
        ones = torch.ones(B, device=dev)
        g0, _ = self._gamma(params, 0.0 * ones)
        g1, _ = self._gamma(params, ones)
        gt, gp = self._gamma(params, t)
        T = cfg.sm_n_timesteps
        if T > 0:   # ldm/model_vdm.py:162-170
            gs, _ = self._gamma(params, t - 1.0 / T)
            gp = T * torch.expm1(gt - gs)
            if cfg.reparam_type == 'input':
                gp = gp * torch.exp(-gt)
        zt, gbar, loss_recon, loss_klz, v0, v1 = ops.qsample(x, g0.contiguous(), g1.contiguous(), gt.contiguous(),
                                                             noise["eps_0"], noise["eps"])
        drop_key = None if deterministic else (rngs or {}).get("dropout")
        if not deterministic and drop_key is None:
            raise ValueError("training mode needs rngs['dropout']")
        cond = conditioning.reshape(B, 1).to(torch.float32)
        net = score_unet(params["score_model"], cfg, zt.view(B, HW, 3), gt, cond, _Drop(drop_key, cfg.sm_pdrop))
        loss_diff = ops.diffusion_loss(2, x, gt.contiguous(), gp.contiguous(), noise["eps"], zt, net.reshape(B, D))
        out = VDMOutput(loss_recon=loss_recon, loss_klz=loss_klz, loss_diff=loss_diff, var_0=v0.mean(), var_1=v1.mean())
        if profile_rows:
            rows, cols = ops.bound_profile(2, x, g0.contiguous(), g1.contiguous(), gt.contiguous(), gp.contiguous(),
                                           noise["eps_0"], noise["eps"], zt, net.reshape(B, D), profile_rows)
            return out, dict(rows=rows, cols=cols, kl_z=torch.zeros(B, device=dev), t=t)
        if return_aux:
            return out, dict(zt=zt, net=net, gt=gt, gp=gp, t=t)
        return out

    # ---- ancestral sampler (ldm/model_vdm.py:182-210), few-step samplers, decoding: the hooks of _VDMBase ------------
    def sample_coefficients(self, params, embedding):
        """the scalar schedule has no per-batch coefficients"""
        return None

    def fast_context(self, params, embedding, conditioning, coeffs=None):
        """the samplers' context of model_vdm.VDM: the conditioning (there is no embedding and no coefficient)"""
        B = conditioning.shape[0]
        return dict(cond=conditioning.reshape(B, 1).to(torch.float32).contiguous())

    def sample(self, params, i, T, z_t, conditioning, rng, coeffs=None):
        """model_vdm.VDM.sample (ldm/model_vdm.py:182-210)"""
        with torch.no_grad():
            z, eps, t, s = self._step_inputs(i, T, z_t, rng)
            z_s = self._reverse_step(params, z, eps, t, s, self.fast_context(params, None, conditioning))
        return z_s.view(z_t.shape)

    def _ode_gamma(self, params, ctx, t):
        gt, gp = self._gamma(params, t)
        return gt.contiguous(), gp.contiguous()                            # [B] each

    def _fast_gamma(self, params, ctx, t):
        return self._gamma(params, t)[0].contiguous()

    def schedule_ends(self, params, ctx):
        g = self._gamma(params, torch.tensor([0.0, 1.0], device=ctx["cond"].device))[0]
        return tuple(float(v) for v in g.tolist())

    def schedule_times(self, params, ctx, targets):
        """the scalar schedule gamma(t) is every sample's, so the mean's: all targets at once by bisection on [0, 1]
        through _gamma, 32 halvings in fp32 (sampling.bisect_times) -- exact up to fp32 for the linear schedules.  A
        handful of elementwise operations on [M] values per halving: no kernel of its own is needed here"""
        from . import sampling
        tg = torch.as_tensor(targets, dtype=torch.float32).reshape(-1).to(ctx["cond"].device)
        return sampling.bisect_times(lambda t: self._gamma(params, t)[0], tg)

    def _fast_gamma_shape(self, B):
        return (B,)

    def _fast_mode(self):
        return 2 if self.config.reparam_type == 'input' else 1

    def _ancestral_mode(self):
        return 2 if self.config.reparam_type == 'input' else 1

    def _ode_mode(self):
        return 2

    def _fast_net(self, params, z, g_t, ctx):
        """the network of sample: eps_hat (reparam_type 'noise') or x_hat ('input') at the per-sample gamma"""
        B = z.shape[0]
        return score_unet(params["score_model"], self.config, z.view(B, HW, 3), g_t, ctx["cond"],
                          _Drop(None, 0.0)).reshape(B, D)

    def _g_0(self, params, coeffs, B, device):
        return self._fast_gamma(params, None, torch.zeros(B, device=device))

    # ---- probability-flow ODE (ldm/model_vdm.py:240-260) -----------------------------------------------------------
    def apply_encoder(self, params, images_u8):
        """model_vdm.VDM.apply_encoder (ldm/model_vdm.py:240-241): zeros"""
        return torch.zeros((images_u8.reshape(-1, D).shape[0], 50), device=images_u8.device, dtype=torch.float32)

    def ode_context(self, params, images_u8):
        """the all-ones embedding of the zero logits and its KL term (0); no coefficients"""
        logits = self.apply_encoder(params, images_u8)
        emb, kl = ops.topk_hard(logits, 15)          # all-equal logits: every entry >= the 15th largest -> ones; KL = 0
        return dict(emb=emb, kl=kl, coeffs=None, logits=logits)

    def ode_context_from_embedding(self, params, emb):
        """the same context for a given embedding"""
        return dict(emb=emb, kl=None, coeffs=None, logits=None)

    def reverse_ode(self, params, x, ctx, t, hutch=None, drift_out=None, div_out=None):
        """model_vdm.VDM.reverse_ode (ldm/model_vdm.py:243-260): drift - 0.5 g^2 score with score = -eps_hat / sigma;
        the score model is conditioned on embeddings[:, :1] like the reference"""
        with torch.no_grad():
            gt, gp = self._ode_gamma(params, ctx, torch.full((x.shape[0],), float(np.float32(t)), device=x.device))
        return self._ode_eval(params, x, gt, gp, gt, ctx["emb"][:, :1].contiguous(), self._ode_mode(), hutch, drift_out,
                              div_out)


# ----------------------------------------------------------------------------- reference-shaped module surface
class _Module:
    """Flax-style handle of one sub-network: Module(config).apply(params, *args) with the reference's call signature, or
    Module(config).bind(params)(*args).  `params` is that sub-network's tree (e.g. state.params['score_model']);
    `rngs={'dropout': Key}` is needed with deterministic=False, like Flax's apply(..., rngs=...)."""

    def __init__(self, config: VDMConfig):
        self.config = config

    def bind(self, params, rngs=None):
        return functools.partial(self.apply, params, rngs=rngs)

    def _drop(self, deterministic, rngs):
        if deterministic:
            return _Drop(None, 0.0)
        key = (rngs or {}).get("dropout")
        if key is None:
            raise ValueError("deterministic=False needs rngs={'dropout': Key}")
        return _Drop(key, self.config.sm_pdrop)


def _pixels(z, ch):
    """[B,32,32,ch] (reference layout) or [B,1024,ch] -> [B,1024,ch] fp32"""
    return z.reshape(z.shape[0], HW, ch).to(torch.float32)


class ScoreUNet(_Module):
    """model_vdm.ScoreUNet (ldm/model_vdm.py:309-388): __call__(z, g_t, conditioning, deterministic=True, time=False)
    -> eps_hat with the shape of z.  z [B,32,32,3]; g_t [B] (or a scalar); conditioning [B,K]."""
    unet_type = 'vdm'

    def apply(self, params, z, g_t, conditioning, deterministic=True, time=False, rngs=None):
        cfg = self.config if self.config.unet_type == self.unet_type else dataclasses.replace(self.config, unet_type=self.unet_type)
        B = z.shape[0]
        g = torch.as_tensor(g_t, dtype=torch.float32, device=z.device)
        if self.unet_type == 'ldm':
            g = g.expand(z.shape).reshape(B, HW, 3).contiguous() if g.dim() < 4 and g.numel() != z.numel() \
                else g.reshape(B, HW, 3)
        else:
            g = g.expand(B).contiguous() if g.dim() == 0 else g.reshape(B)    # model_vdm.py:329-332: g_t * ones(B)
        cond = torch.as_tensor(conditioning, dtype=torch.float32, device=z.device).reshape(B, -1)
        out = score_unet(params, cfg, _pixels(z, 3), g, cond, self._drop(deterministic, rngs), time=time)
        return out.reshape(z.shape)

    __call__ = apply


class UNet(ScoreUNet):
    """ldm_unet.UNet (ldm/ldm_unet.py:64-142): the same topology with per-pixel FiLM conditioning; g_t [B,32,32,3]."""
    unet_type = 'ldm'


class UnetEncoder(_Module):
    """model_mulan_epsilon.UnetEncoder (ldm/model_mulan_epsilon.py:101-154): __call__(z, deterministic=True) ->
    logits [B, latent_size]; z = EncDec.encode(images) [B,32,32,3]."""

    def apply(self, params, z, deterministic=True, rngs=None):
        return unet_encoder(params, self.config, _pixels(z, 3), self._drop(deterministic, rngs))

    __call__ = apply


class NoiseSchedule_polynomial_fixedend(_Module):
    """model_mulan_epsilon.NoiseSchedule_polynomial_fixedend (ldm/model_mulan_epsilon.py:481-613):
    __call__(embedding [B,latent], t [B] or scalar) -> gamma [B,3072]; grad_t(embedding, t) = d gamma / dt (:540-555)."""

    def _eval(self, params, embedding, t):
        emb = torch.as_tensor(embedding, dtype=torch.float32)
        B = emb.shape[0]
        t = torch.as_tensor(t, dtype=torch.float32, device=emb.device)
        t = t.expand(B).contiguous() if t.dim() == 0 else t.reshape(B)
        a, b, c = poly_coefficients(params, emb)
        return ops.poly_gamma(a, b, c, t, self.config.gamma_min, self.config.gamma_max)

    def apply(self, params, embedding, t, rngs=None):
        return self._eval(params, embedding, t)[2]

    def grad_t(self, params, embedding, t):
        return self._eval(params, embedding, t)[3]

    __call__ = apply


class EncDec:
    """model_vdm.EncDec (ldm/model_vdm.py:265-303): no parameters.  encode(x uint8) -> f in (-1, 1);
    decode(z, g_0) -> [..., 256] decoder log-probabilities; logprob(x, z, g_0) -> [B] sum over sub-pixels of the
    log-probability of x's bin (the fused q-sample kernel, which never builds the 256-bin table)."""

    def __init__(self, config: VDMConfig):
        self.config = config

    def __call__(self, x, g_0):
        """EncDec.__call__ (:269-272): decode(encode(x), g_0)"""
        return self.decode(self.encode(x), g_0)

    def encode(self, x):
        return encode_images(x.reshape(x.shape[0], D).to(torch.uint8)).reshape(*x.shape)

    def _g(self, g_0, z):
        """g_0 as the reference accepts it -- a scalar, [B], or the shape of z -- as [B] or [B, D] fp32"""
        B = z.shape[0]
        g = torch.as_tensor(g_0, dtype=torch.float32, device=z.device)
        if g.numel() == 1:
            return g.reshape(1).expand(B).contiguous()
        if g.numel() == B:
            return g.reshape(B).contiguous()
        if g.numel() != z.numel():
            raise ValueError(f"g_0 of shape {tuple(g.shape)} does not broadcast over z {tuple(z.shape)}")
        return g.reshape(B, D).contiguous()

    def decode(self, z, g_0):
        """EncDec.decode (:282-296): log_softmax over the 256 bins of -0.5 ((z - v_j) exp(-g_0 / 2))^2, shape
        z.shape + (256,)"""
        return ops.decode_logprobs(z.reshape(z.shape[0], D), self._g(g_0, z)).reshape(*z.shape, self.config.vocab_size)

    def logprob(self, x, z, g_0):
        """EncDec.logprob (:298-303): sum over (H, W, C) of decode(z, g_0)[x] -> [B].  Evaluated by mulan_qsample_fwd
        (its reconstruction term at z_0 = f + exp(g_0 / 2) eps_0 with eps_0 chosen so that z_0 = z), no [.., 256]
        tensor.  z may carry a gradient (the kernel's backward covers g_0; z is a leaf here, like in the train path
        where z_0 is sampled, not learned)."""
        B = z.shape[0]
        xu = x.reshape(B, D).round().to(torch.uint8).contiguous()
        g = self._g(g_0, z)
        g = g if g.dim() == 2 else g[:, None].expand(B, D).contiguous()
        f = encode_images(xu).reshape(B, D)
        eps_0 = (z.reshape(B, D).to(torch.float32) - f) * torch.exp(-0.5 * g)
        _, _, recon, _, _, _ = ops.qsample(xu, g, g, g, eps_0, torch.zeros_like(eps_0))
        return -recon

    def decode_argmax(self, z, g_0):
        """argmax over the 256 bins of decode(z, g_0) (:282-293); g_0 per sample [B] or per element"""
        B = z.shape[0]
        g = torch.as_tensor(g_0, dtype=torch.float32, device=z.device)
        g = g.expand(B).contiguous() if g.dim() == 0 else g.reshape(B, -1).squeeze(-1) if g.numel() == B else g.reshape(B, D)
        return ops.decode_argmax(z.reshape(B, D).to(torch.float32).contiguous(), g.contiguous()).reshape(z.shape)


def make_vdm(vdm_type: str, config: VDMConfig):
    """Experiment_VDM.get_model_and_params dispatch (ldm/experiment_vdm.py:32-38)."""
    if vdm_type == 'mulan_velocity':
        return MulanVDM(config, "velocity")
    if vdm_type == 'mulan_epsilon':
        return MulanVDM(config, "epsilon")
    if vdm_type == 'vdm':
        return PlainVDM(config)
    raise KeyError(vdm_type)


# ----------------------------------------------------------------------------- tree utilities
def tree_leaves(tree, prefix=()):
    for k, v in tree.items():
        if isinstance(v, dict):
            yield from tree_leaves(v, prefix + (k,))
        else:
            yield prefix + (k,), v


def tree_map(fn, tree):
    return {k: tree_map(fn, v) if isinstance(v, dict) else fn(v) for k, v in tree.items()}


def tree_set(tree, path, value):
    for k in path[:-1]:
        tree = tree[k]
    tree[path[-1]] = value


def to_flax_layout(tree):
    """Product tree -> reference (Flax) layout: drops the zero 16th input channel of conv_in."""
    def fix(path, v):
        if path[-2:] == ("conv_in", "kernel") and v.shape[2] == 16:
            return v[:, :, :15, :]
        return v
    out = {}
    for path, v in tree_leaves(tree):
        d = out
        for k in path[:-1]:
            d = d.setdefault(k, {})
        d[path[-1]] = fix(path, v)
    return out


def from_flax_layout(flax_tree, like):
    """Copies a reference-layout tree into the leaves of `like` (in place, under no_grad)."""
    with torch.no_grad():
        for path, dst in tree_leaves(like):
            src = flax_tree
            for k in path:
                src = src[k]
            src = torch.as_tensor(src, dtype=torch.float32)
            if path[-2:] == ("conv_in", "kernel") and src.shape[2] == 15:
                src = torch.cat([src, torch.zeros(3, 3, 1, src.shape[3])], dim=2)
            if tuple(src.shape) != tuple(dst.shape):
                raise ValueError(f"shape mismatch at {'/'.join(path)}: {tuple(src.shape)} vs {tuple(dst.shape)}")
            dst.copy_(src.to(dst.device))
    return like
