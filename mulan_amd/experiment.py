"""Experiment harness on PyTorch-ROCm + libmulan_hip (mirror of ldm/experiment.py + ldm/experiment_vdm.py).

Kept surface: Experiment(config) -> .train_step(base_rng, state, batch), .eval_step(base_rng, params,
batch, eval_step), .loss_fn(params, inputs, step, rng, is_train), .get_model_and_params(rng),
.train_and_evaluate(workdir), .evaluate(logdir, checkpoint_dir), .p_train_step / .p_eval_step.
jax.pmap/lax.scan/lax.pmean become: one process per GPU (torchrun), a host loop over sub-steps, and a
bucketed RCCL all-reduce of the flat gradient buffer overlapped with backward (mulan_amd.parallel).
"""
import abc
import contextlib
import functools
import logging
import math
import os
import time

import numpy as np
import torch

from . import checkpoint as ckpt_lib
from . import data as dataset
from . import parallel
from . import profiling
from . import sampling
from .model import VDMConfig, make_vdm, tree_leaves
from .rng import PRNGKey
from .train_state import TrainState, tree_leaves_in_layout

log = logging.getLogger("mulan")


def restore_partial(state, state_restore_dict):
    """Key-wise overlay of a checkpoint onto the state (ldm/experiment.py:377-393)."""
    state.load_state_dict(state_restore_dict, strict=False)
    return state


# Several ranks, replayed step: all-reduce every bucket behind the signal word a kernel node of the graph sets after it
# (hipStreamWaitValue32: the collectives run under the rest of the replayed backward pass), instead of behind the whole
# graph.  OPT-IN (MULAN_GRAPH_OVERLAP=1 or config.training.graph_overlap=True) since round 5: the hand-off has only ever run
# with a stand-in collective and with RCCL on ONE rank (no multi-GPU box is available to the build; tests/test_gpu_rccl.py
# is skipped there), and on the stand-in it is no faster than the eager overlapped step at the headline batch (79.4 vs
# 78.8 ms, profiles/r04_overlap_timing_probe.log).  The default is what rounds 1-3 shipped and what plain
# torch.distributed semantics cover: see Experiment.__init__.
GRAPH_OVERLAP = os.environ.get("MULAN_GRAPH_OVERLAP", "0") == "1"
# Several ranks, RCCL only (opt-in, round 5 experiment): the bucket all-reduces are CAPTURED INTO the graph -- the hooks
# launch them during the capture as they do in the eager step, on the collective stream, so the graph itself carries every
# dependency (bucket ready -> all-reduce -> optimizer): no signal words, no stream calibration, no release lag, and the
# optimizer is part of the graph as on one rank.  torch's ProcessGroupNCCL supports capture; gloo does not.  Run on ONE
# rank of RCCL only (tools/overlap_timing_probe.py --rccl): never on a multi-GPU box, hence opt-in.
GRAPH_COLLECTIVES = os.environ.get("MULAN_GRAPH_COLLECTIVES", "0") == "1"


def ops_kernel_timer_off():
    from . import ops
    return ops.KERNEL_TIMER is None


class GraphedStep:
    """One train step captured as a HIP graph and replayed: the build's counterpart of the reference's
    jax.pmap(lax.scan(train_step)) (ldm/experiment.py:89-91), which dispatches 1000 sub-steps per host call.

    The step issues ~1950 kernel launches; from Python that is ~45 ms of host time, more than the GPU needs at small
    per-GPU batches.  Captured once (forward, backward, gradient collection and -- on one rank -- AdamW/EMA), the step
    is replayed with a single launch.  Everything that changes from step to step reaches the kernels through device
    memory written before the replay ("stream-ordered parameters"):
      * the uint8 batch and the noise tensors (eps_0, eps, Gamma draws) live in static buffers filled eagerly;
      * t0 of the antithetic time grid is a 0-dim device tensor, and so is the Gumbel-softmax temperature tau of
        latent_type 'gumbel' (annealed with the step count, which the capture does not see);
      * the two dropout seeds are int64 device slots read by the GroupNorm kernels (mulan_groupnorm_*_dyn);
      * learning rate and Adam bias corrections are a float device array read by mulan_adamw_ema_step_dyn.
    The keys are derived on the host exactly as the eager step derives them (Experiment_VDM.step_keys), so a replayed
    step is bit-identical to the eager one.  With more than one rank the graph ends after the gradients; the bucketed
    all-reduce and the optimizer launch follow eagerly (the collective stays outside the capture).
    """

    def __init__(self, exp, state, batch):
        from . import ops
        from .rng import Key
        self.exp = exp
        dev = exp.device
        self.shape = tuple(batch['images'].shape)
        B = self.shape[0]
        cfg = exp.model.config
        self.inputs = {k: torch.empty_like(v) for k, v in batch.items()}
        self.need_gamma = getattr(cfg, 'reparam_type', 'true') == 'true' and hasattr(cfg, 'latent_k')
        self.latent_type = getattr(cfg, 'latent_type', 'topk')
        self.gumbel = self.latent_type == 'gumbel' or (self.latent_type == 'topk' and
                                                        getattr(cfg, 'topk_noise_type', 'gamma') == 'gumbel')
        self.noise = {'t0': torch.zeros((), device=dev, dtype=torch.float32),
                      'eps_0': torch.empty((B, 3072), device=dev, dtype=torch.float32),
                      'eps': torch.empty((B, 3072), device=dev, dtype=torch.float32)}
        if not cfg.antithetic_time_sampling:
            self.noise['t'] = torch.empty((B,), device=dev, dtype=torch.float32)
        if self.need_gamma:
            if self.latent_type == 'gaussian':
                self.noise['eps_z'] = torch.empty((B, cfg.latent_size), device=dev, dtype=torch.float32)
            elif self.gumbel:
                self.noise['gumbel'] = torch.empty((B, cfg.latent_size), device=dev, dtype=torch.float32)
            else:
                self.noise['gamma_raw'] = torch.empty((10, B, cfg.latent_size), device=dev, dtype=torch.float32)
            if self.latent_type == 'gumbel':
                self.noise['tau'] = torch.ones((), device=dev, dtype=torch.float32)
        self.seeds = torch.zeros(2, device=dev, dtype=torch.int64)
        self.dyn = torch.zeros(4, device=dev, dtype=torch.float32)
        self.h_seeds = torch.zeros(2, dtype=torch.int64).pin_memory()
        self.h_dyn = torch.zeros(6, dtype=torch.float32).pin_memory()       # lr, bc1, bc2, 0, t0, tau
        # collectives inside the graph (see GRAPH_COLLECTIVES): RCCL process groups only
        self.captured_collectives = bool(exp.world > 1 and exp.graph_collectives and exp.reducer.enabled and
                                         exp.reducer.sync_ops)
        self.whole = exp.world == 1 or self.captured_collectives      # optimizer inside the graph
        self.mode = ops.CONV_MODE
        self.copied = torch.cuda.Event()             # the pinned staging buffers have been read by the device
        self.graph = torch.cuda.CUDAGraph()
        self.metrics = None
        rngs = {'dropout_pair': (Key(0, dev=self.seeds[0:1]), Key(0, dev=self.seeds[1:2]))}
        exp.reducer.paused = not self.captured_collectives
        try:
            self._fill(exp._train_rng, state, batch)         # valid contents while capturing (nothing executes)
            state.zero_grad()
            state.drop_graph_refs()                          # no autograd node of the eager stream may survive
            torch.cuda.synchronize()
            # several ranks: the hooks that launch a bucket's all-reduce in the eager step plant a signal (a one-thread
            # kernel node) per bucket instead (parallel.GradReducer._mark); after the replay the collectives wait for
            # those signals, i.e. they run under the rest of the replayed backward pass (MULAN_GRAPH_OVERLAP=0: behind
            # the whole graph)
            if exp.graph_overlap and not self.captured_collectives:
                exp.reducer.begin_capture()
            mode = "global"
            if exp.world > 1:
                # other threads of a multi-rank process keep talking to the runtime while this one captures (the RCCL
                # process group's watchdog polls the events of the collectives it still tracks): thread-local capture
                # mode keeps their calls out of the capture; the device is idle (synchronize above: every collective of
                # the eager step before has completed)
                mode = "thread_local"
            with torch.cuda.graph(self.graph, capture_error_mode=mode):
                state.zero_grad()
                if self.captured_collectives:
                    exp.reducer.prepare()
                packer = state.param_packer()
                if packer is not None:
                    packer.refresh()
                bpd, metrics = exp.loss_fn(state.params, self.inputs, step=0, rng=None, is_train=True, rngs=rngs,
                                           noise=self.noise)
                with ops.weight_gradient_stream():
                    bpd.backward()
                if self.captured_collectives:
                    state.collect_grads()
                    exp.reducer.finish()                     # (captured: the compute stream waits for the collective stream)
                else:
                    exp.reducer.end_capture()
                    state.collect_grads()
                if packer is not None:
                    packer.invalidate()
                if self.whole:
                    state.apply_gradients(lr=0.0, ema_rate=exp.config.optimizer.ema_rate, grad_scale=1.0 / exp.world,
                                          clip_norm=exp.config.optimizer.get('gradient_clip_norm', None), dyn=self.dyn,
                                          count_step=False)
                self.metrics = metrics
        finally:
            exp.reducer.paused = False
        if not self.whole and exp.graph_overlap and not self.captured_collectives:
            # several ranks: make sure the collective stream is one on which the signals really release the
            # collectives early (parallel.GradReducer.calibrate_stream: a few trial replays, once per capture).  Any
            # failure here leaves the plain schedule: collectives behind the whole graph (allreduce_now), logged.
            try:
                leads = exp.reducer.calibrate_stream(self.graph.replay)
                if leads is not None:
                    log.info("collective stream released %s ms before the end of the replayed graph (trial replays)", leads)
            except Exception as e:      # noqa: BLE001
                log.warning("overlap calibration failed (%s: %s): collectives run behind the replayed graph", type(e).__name__, e)
                exp.reducer.capture = None

    def matches(self, batch):
        from . import ops
        return tuple(batch['images'].shape) == self.shape and ops.CONV_MODE == self.mode

    def _fill(self, base_rng, state, batch):
        """everything that differs from step to step, written where the captured kernels read it"""
        from . import ops
        exp = self.exp
        rng = base_rng.fold_in(exp.rank).fold_in(state.step)
        keys = exp.step_keys(rng, True)
        for k, v in batch.items():
            self.inputs[k].copy_(v, non_blocking=True)
        B = self.shape[0]
        dev = exp.device
        if 't' in self.noise:
            self.noise['t'].copy_(ops.noise((B,), keys['t'].v, 0, dev, "uniform"))
        if 'gamma_raw' in self.noise:
            cfg = exp.model.config
            self.noise['gamma_raw'].copy_(keys['gamma'].gamma(1.0 / cfg.latent_k, (10, B, cfg.latent_size), dev))
        if 'gumbel' in self.noise:
            self.noise['gumbel'].copy_(ops.noise(tuple(self.noise['gumbel'].shape), keys['gamma'].v, 0, dev, "gumbel"))
        if 'eps_z' in self.noise:
            self.noise['eps_z'].copy_(keys['gamma'].normal(tuple(self.noise['eps_z'].shape), dev))
        ops.randn(None, keys['eps_0'].v, 0, dev, out=self.noise['eps_0'])
        ops.randn(None, keys['eps'].v, 0, dev, out=self.noise['eps'])
        to_i64 = lambda v: v - (1 << 64) if v >= (1 << 63) else v
        self.h_seeds[0], self.h_seeds[1] = to_i64(keys['enc'].v), to_i64(keys['score'].v)
        lr = exp.lr_schedule(state.step)
        vals = state.dynamic_scalars(lr, state.step + 1)
        for i, v in enumerate(vals):
            self.h_dyn[i] = v
        self.h_dyn[4] = float(np.float32(keys['t'].uniform()))
        self.seeds.copy_(self.h_seeds, non_blocking=True)
        self.dyn.copy_(self.h_dyn[:4], non_blocking=True)
        self.noise['t0'].copy_(self.h_dyn[4], non_blocking=True)
        if 'tau' in self.noise:
            from .model import gumbel_tau
            self.h_dyn[5] = gumbel_tau(state.step)
            self.noise['tau'].copy_(self.h_dyn[5], non_blocking=True)
        self.copied.record()

    def step(self, base_rng, state, batch):
        exp = self.exp
        self.copied.synchronize()      # the pinned staging buffers are rewritten below: the last copies must be done
        self._fill(base_rng, state, batch)
        if not self.whole:
            exp.reducer.before_replay()
        self.graph.replay()
        if self.whole:
            state.step += 1
        else:
            exp.reducer.allreduce_captured()
            state.apply_gradients(lr=exp.lr_schedule(state.step), ema_rate=exp.config.optimizer.ema_rate,
                                  grad_scale=1.0 / exp.world,
                                  clip_norm=exp.config.optimizer.get('gradient_clip_norm', None))
        scalars = parallel.allreduce_mean_scalars({k: v.clone() for k, v in self.metrics['scalars'].items()}, exp.device)
        metrics = {'scalars': {'train_' + k: v for k, v in scalars.items()}, 'images': {'inputs': batch['images']}}
        return state, metrics


def choose_step_form(cfg_hip_graph, env, world, batch_size_train, n_embd, opt_in_overlap):
    """-> (replay the step as a HIP graph?, is a failed capture an error?).  cfg_hip_graph: config.training.hip_graph
    (True / False / None), env: MULAN_HIP_GRAPH ('1' / '0' / anything else = unset).
    Asked for explicitly (config or environment): a failed capture is an error.  Chosen by default -- the multi-rank
    heuristic included: a warning and the eager step (a training run must not lose the replay without anybody noticing,
    and on several ranks one rank raising while the others enter their collectives would hang the job:
    parallel.GradReducer.eager_order exists so that a rank CAN fall back).  `required` is therefore decided from the
    explicit inputs only, before the heuristic turns `want` into a bool."""
    want = cfg_hip_graph
    required = want is True or (env == "1" and want is not False)
    if want is None and env not in ("0", "1") and world > 1 and not opt_in_overlap:
        local = max(1, int(batch_size_train) // world)
        want = local * (float(n_embd) / 128.0) ** 2 < 96
    if env in ("0", "1"):
        want = env == "1" and want is not False
    elif want is None:
        want = True
    return bool(want), required


class Experiment(abc.ABC):
    """Boilerplate for training and evaluating VDM models (ldm/experiment.py:42-104)."""

    def __init__(self, config, device=None):
        self.config = config
        self.rank, self.world, local = parallel.init_distributed()
        if device is None:
            if not torch.cuda.is_available():
                raise RuntimeError("the MuLAN hot path needs an MI355X (no CPU fallback); no HIP device visible")
            device = torch.device("cuda", local if self.world > 1 else torch.cuda.current_device())
            torch.cuda.set_device(device)
        self.device = device

        # Set seed before initializing model (ldm/experiment.py:48-50).
        self.rng = PRNGKey(config.training.seed)
        self.rng, data_rng = self.rng.split()
        self.train_iter, self.eval_iter = dataset.create_dataset(config, device, data_rng.v % (1 << 31), self.rank,
                                                                 self.world)
        self.rng, model_rng = self.rng.split()
        self.model, params = self.get_model_and_params(model_rng)
        n_params = sum(v.numel() for _, v in tree_leaves(params))
        log.info("parameters: %.2f M", n_params / 1e6)

        self.state = TrainState.create(apply_fn=self.model.apply, variables={"params": params}, device=device,
                                       optimizer_args=dict(config.optimizer.args.items()))
        self.lr_schedule = self.get_lr_schedule()

        ckpt_restore_dir = self.config.get('ckpt_restore_dir', 'None')
        if ckpt_restore_dir != 'None':
            self.state = restore_partial(self.state, ckpt_lib.restore_dict(ckpt_restore_dir))

        self.reducer = parallel.GradReducer(self.state.grad, self.state.reducer_leaves())

        self.rng, train_rng = self.rng.split()
        self._train_rng = train_rng
        self.rng, eval_rng, sample_rng = self.rng.split(3)
        self._eval_rng, self._sample_rng = eval_rng, sample_rng
        self._sample_dummy = None
        self._profile = None                 # profiling.Profile while config.training.profile is set (train_and_evaluate)
        # the lax.scan of the reference (ldm/experiment.py:89-91: `substeps` train steps per host dispatch) becomes a
        # HIP-graph replay per step (GraphedStep), on one rank and on several.  With several ranks the collectives stay
        # outside the graph, but every bucket's all-reduce waits only for the signal the capture planted behind that
        # bucket (parallel.GradReducer.begin_capture / allreduce_captured), so it runs under the rest of the replayed
        # backward pass like the eager step's does -- and the host, which needs ~54 ms to issue the ~1100 launches of an
        # eager step whatever the batch, is out of the picture at every batch size (rounds 1-3 chose between the replay
        # with exposed collectives and the eager step by batch size).
        # MULAN_HIP_GRAPH=1 / 0 or config.training.hip_graph=True / False override.
        # Several ranks (round 5): the DEFAULT is again the round-3 choice, which needs nothing beyond
        # torch.distributed's documented stream semantics -- below local_batch * (E / 128)^2 = 96 images the replayed
        # step with the collectives behind the graph (the host cannot issue an eager step as fast as the GPU runs it:
        # ~54 ms of launches), from there on the eager step whose bucketed all-reduce overlaps the backward pass.  The
        # replay WITH overlap (signal words, GRAPH_OVERLAP above) is opt-in until it has run on a multi-GPU RCCL box.
        self.graph_overlap = bool(config.training.get("graph_overlap", GRAPH_OVERLAP)) and self.world > 1
        self.graph_collectives = bool(config.training.get("graph_collectives", GRAPH_COLLECTIVES)) and self.world > 1
        want, self.hip_graph_required = choose_step_form(
            config.training.get("hip_graph", None), os.environ.get("MULAN_HIP_GRAPH", ""), self.world,
            int(config.training.batch_size_train), float(config.model.sm_n_embd),
            self.graph_overlap or self.graph_collectives)
        self.hip_graph = bool(want) and torch.device(self.device).type == "cuda"
        self._graphed = None
        self._eager_steps = 0
        self.graph_capture_error = None      # set when a default-on capture failed and the run fell back to eager steps

    # ---- schedules / optimiser ------------------------------------------------------------------
    def get_lr_schedule(self):
        """ldm/experiment.py:106-129: optax.linear_schedule(0 -> lr over num_steps_lr_warmup), joined at the warm-up
        boundary with linear_schedule(lr -> 0 over num_steps_train - warm-up) when optimizer.lr_decay is set.  optax's
        linear_schedule with transition_steps <= 0 is the CONSTANT init_value, so num_steps_lr_warmup <= 0 without
        decay trains at lr 0.0 in the reference; reproduced (with a warning), not repaired."""
        lr = float(self.config.optimizer.learning_rate)
        tr = self.config.training
        warm = int(tr.num_steps_lr_warmup)
        decay = bool(self.config.optimizer.lr_decay)
        span = int(tr.num_steps_train) - warm

        def ramp(first, last, steps, count):
            if steps <= 0:
                return first
            return first + (last - first) * (min(max(count, 0), steps) / steps)

        if warm <= 0 and not decay:
            log.warning("num_steps_lr_warmup <= 0 without lr_decay: the reference's schedule is the constant 0.0")

        def schedule(step):
            if decay and step >= warm:
                return ramp(lr, 0.0, span, step - warm)
            return ramp(0.0, lr, warm, step)
        return schedule

    @abc.abstractmethod
    def get_model_and_params(self, rng):
        ...

    @abc.abstractmethod
    def sample_fn(self, *, dummy_inputs, rng, params):
        ...

    @abc.abstractmethod
    def loss_fn(self, params, inputs, step, rng, is_train):
        ...

    # ---- steps ----------------------------------------------------------------------------------
    def _profiling_now(self):
        """True while the profile window of config.training.profile is open: those steps run eagerly, one roctx range
        per phase; before and after the window the HIP-graph step is used"""
        return self._profile is not None and self._profile.active

    def train_step(self, base_rng, state, batch):
        """Experiment.train_step (ldm/experiment.py:335-356): fold rank + step into the rng, value_and_grad,
        gradient mean over ranks, lr schedule, AdamW+EMA, scalar mean over ranks."""
        if self.hip_graph and not self._profiling_now() and ops_kernel_timer_off() and hasattr(self.model, "parameterization"):
            g = self._graphed
            if g is None or not g.matches(batch):
                if self._eager_steps >= 1:           # one eager step first: every kernel configured, allocator warm
                    try:
                        self._graphed = g = GraphedStep(self, state, batch)
                    except Exception as e:           # noqa: BLE001  capture is an optimisation: fall back loudly, once
                        if self.hip_graph_required:
                            raise RuntimeError("HIP-graph capture of the train step failed although it was requested "
                                               "(config.training.hip_graph / MULAN_HIP_GRAPH=1)") from e
                        log.warning("HIP-graph capture of the train step failed (%s: %s); running eagerly from now on "
                                    "(steps_per_sec will show it)", type(e).__name__, e)
                        self.hip_graph = False
                        self.graph_capture_error = f"{type(e).__name__}: {e}"
                        g = None
                else:
                    g = None
            if g is not None:
                return g.step(base_rng, state, batch)
        self._eager_steps += 1
        rng = base_rng.fold_in(self.rank).fold_in(state.step)
        phase = self._profile.phase if self._profiling_now() else (lambda name: contextlib.nullcontext())
        state.zero_grad()
        self.reducer.prepare()
        packer = state.param_packer()        # f16x3 mode: weight maxima + packed operands of all layers, two launches
        if packer is not None:
            packer.refresh()
        with phase("forward"):
            bpd, metrics = self.loss_fn(state.params, batch, step=state.step, rng=rng, is_train=True)
        with phase("backward"):
            from . import ops
            with ops.weight_gradient_stream():       # weight gradients beside the input-gradient chain (ops._on_side)
                bpd.backward()
            state.collect_grads()
        with phase("all-reduce"):
            self.reducer.finish()
        learning_rate = self.lr_schedule(state.step)
        if packer is not None:
            packer.invalidate()              # the optimizer rewrites the parameters
        with phase("optimizer"):
            state.apply_gradients(lr=learning_rate, ema_rate=self.config.optimizer.ema_rate,
                                  grad_scale=1.0 / self.world,
                                  clip_norm=self.config.optimizer.get('gradient_clip_norm', None))
        scalars = parallel.allreduce_mean_scalars(metrics['scalars'], self.device)
        metrics['scalars'] = {'train_' + k: v for k, v in scalars.items()}
        return state, metrics

    def eval_step(self, base_rng, params, batch, eval_step=0):
        """Experiment.eval_step (ldm/experiment.py:358-374)."""
        rng = base_rng.fold_in(self.rank).fold_in(eval_step)
        with torch.no_grad():
            _, metrics = self.loss_fn(params, batch, eval_step, rng=rng, is_train=False)
        scalars = parallel.allreduce_mean_scalars(metrics['scalars'], self.device)
        metrics['scalars'] = {'eval_' + k: v for k, v in scalars.items()}
        return metrics

    def p_train_step(self, state, batch):
        """pmap(scan(train_step)) analogue (ldm/experiment.py:88-91): `batch` leaves carry a leading
        sub-step axis; returns the state and metrics stacked over sub-steps."""
        substeps = batch['images'].shape[0]
        stacked = {}
        for s in range(substeps):
            sub = {k: v[s] for k, v in batch.items()}
            state, m = self.train_step(self._train_rng, state, sub)
            for k, v in m['scalars'].items():
                stacked.setdefault(k, []).append(v.detach() if torch.is_tensor(v) else torch.tensor(v))
        return state, {'scalars': {k: torch.stack(v) for k, v in stacked.items()}}

    def p_eval_step(self, params, batch, eval_step):
        return self.eval_step(self._eval_rng, params, batch, eval_step)

    # ---- loops ----------------------------------------------------------------------------------
    def train_and_evaluate(self, workdir):
        """Experiment.train_and_evaluate (ldm/experiment.py:199-294)."""
        config = self.config.training
        state = self.state
        checkpoint_dir = os.path.join(workdir, 'checkpoints')
        latest = ckpt_lib.latest_checkpoint(checkpoint_dir)
        if latest:
            state.load_state_dict(ckpt_lib.restore_dict(latest))
        step = initial_step = int(state.step)
        substeps = config.substeps
        if initial_step and hasattr(self.train_iter, "seek"):        # resume: the data stream continues where it was
            self.train_iter.seek(initial_step * self.train_iter.local)
        writer = ckpt_lib.ScalarWriter(workdir if self.rank == 0 else None)
        if initial_step == 0:
            writer.write_hparams(self.config.to_dict())
        t_last, s_last = time.time(), step
        if config.get('profile', False):
            self._profile = profiling.Profile(num_profile_steps=5, first_profile=initial_step + 10 * substeps)
        while step < config.num_steps_train:
            is_last_step = step + substeps >= config.num_steps_train
            batch = next(self.train_iter)
            with profiling.trace_range(f"train step {step}"):        # jax.profiler.StepTraceAnnotation('train', step_num)
                state, _train_metrics = self.p_train_step(state, batch)
            if self._profile is not None:                            # hooks: periodic_actions.Profile (experiment.py:230-232)
                self._profile(step + substeps)
            new_step = int(state.step)
            assert new_step == step + substeps
            step = new_step
            if step % config.steps_per_logging == 0 or is_last_step:
                metrics = {k: float(v.mean()) for k, v in _train_metrics['scalars'].items()}
                now = time.time()
                metrics['steps_per_sec'] = (step - s_last) / max(now - t_last, 1e-9)
                t_last, s_last = now, step
                writer.write_scalars(step, metrics)
            if step % config.steps_per_eval == 0 or is_last_step or step == 1000:
                eval_metrics = []
                for eval_step in range(config.num_steps_eval):
                    batch = self.eval_iter.next()
                    metrics = self.p_eval_step(state.ema_params, batch, eval_step)
                    eval_metrics.append({k: float(v) for k, v in metrics['scalars'].items()})
                writer.write_scalars(step, {k: float(np.mean([m[k] for m in eval_metrics])) for k in eval_metrics[0]})
                self._write_samples(writer, step, state.ema_params)          # ldm/experiment.py:287-289
            if step % config.steps_per_save == 0 or is_last_step:
                if self.rank == 0:
                    ckpt_lib.save(checkpoint_dir, state.state_dict(), max_to_keep=100)
        writer.close()
        return state

    def p_sample(self, params, T=None):
        """self.p_sample of the reference (ldm/experiment.py:96-102): sample_fn on a batch shaped like one eval
        micro-batch, samples of all ranks concatenated.  T: config.training.sample_timesteps, default 1000 like the
        reference's hard-coded value; 0 disables sampling at evaluation points.  config.training.sampler (optional, not in
        the reference): 'ancestral' (the default), 'ddim', 'dpm2m' or 'sde2m', which then run sample_timesteps steps
        (default 25); config.training.sampler_grid (optional): the kind of time grid of those three (sampling.GRIDS,
        default 'uniform'), config.training.sampler_grid_rho the rho of 'karras' (default 7)."""
        sampler = sampling.check_sampler(self.config.training.get('sampler', 'ancestral'))
        grid, rho = sampling.check_grid(sampler, self.config.training.get('sampler_grid', 'uniform'), None,
                                        self.config.training.get('sampler_grid_rho', 7.0))
        if T is None:
            T = int(self.config.training.get('sample_timesteps', 1000 if sampler == 'ancestral' else 25))
        if T <= 0:
            return None
        if self._sample_dummy is None:
            self._sample_dummy = torch.empty((self.eval_iter.local, 32, 32, 3), dtype=torch.uint8, device=self.device)
        if sampler == 'ancestral':
            return self.sample_fn(dummy_inputs=self._sample_dummy, rng=self._sample_rng, params=params, T=T)
        return self.sample_fn(dummy_inputs=self._sample_dummy, rng=self._sample_rng, params=params, T=T, sampler=sampler,
                              grid=grid, grid_rho=rho)

    def _write_samples(self, writer, step, params):
        samples = self.p_sample(params)
        if samples is not None:
            writer.write_images(step, {'samples': ckpt_lib.generate_image_grids(samples)[None]})

    def evaluate(self, logdir, checkpoint_dir):
        """Experiment.evaluate (ldm/experiment.py:296-332): num_steps_eval batches on the EMA parameters."""
        sd = ckpt_lib.restore_dict(checkpoint_dir)
        self.state.load_state_dict({"ema_params": sd["ema_params"], "step": sd.get("step", 0)}, strict=True)
        step = int(sd.get("step", 0))
        eval_metrics = []
        for eval_step in range(self.config.training.num_steps_eval):
            batch = self.eval_iter.next()
            metrics = self.p_eval_step(self.state.ema_params, batch, eval_step)
            eval_metrics.append({k: float(v) for k, v in metrics['scalars'].items()})
        out = {k: float(np.mean([m[k] for m in eval_metrics])) for k in eval_metrics[0]}
        writer = ckpt_lib.ScalarWriter(os.path.join(logdir, 'eval') if self.rank == 0 else None)
        writer.write_scalars(step, out)
        self._write_samples(writer, step, self.state.ema_params)             # ldm/experiment.py:328-332
        writer.close()
        return out


class Experiment_VDM(Experiment):
    """Train and evaluate a VDM model (ldm/experiment_vdm.py:27-110)."""

    def get_model_and_params(self, rng):
        config = VDMConfig(**self.config.model.to_dict())
        model = make_vdm(self.config.vdm_type, config)
        rng1, _rng2 = rng.split()
        return model, model.init(rng1)

    @staticmethod
    def step_keys(rng, is_train=True):
        """The keys one loss_fn call consumes, derived exactly as loss_fn / VDM._noise / VDM.apply derive them:
        {'t', 'gamma', 'eps_0', 'eps'} from the 'sample' stream, {'enc', 'score'} from the 'dropout' stream."""
        rng, sample_rng = rng.split()
        k_t, k_g, k_0, k_e = sample_rng.split(4)
        keys = {'t': k_t, 'gamma': k_g, 'eps_0': k_0, 'eps': k_e}
        if is_train:
            rng, dropout_rng = rng.split()
            keys['enc'], keys['score'] = dropout_rng.split(2)
        return keys

    def loss_fn(self, params, inputs, step, rng, is_train, rngs=None, noise=None, same_image=False):
        """Experiment_VDM.loss_fn (ldm/experiment_vdm.py:47-78).  rngs / noise (not in the reference): the already
        derived keys / noise tensors of this step, used by the graph-captured train step (GraphedStep).  same_image: all
        rows of the batch are one image (the dense evaluator): see MulanVDM.apply."""
        if rngs is None:
            rng, sample_rng = rng.split()
            rngs = {'sample': sample_rng}
            if is_train:
                rng, dropout_rng = rng.split()
                rngs['dropout'] = dropout_rng
        outputs = self.state.apply_fn(params, inputs['images'], inputs.get('labels'), inputs.get('conditioning'),
                                      step=step, rngs=rngs, deterministic=not is_train,
                                      **({} if noise is None else {'noise': noise}),
                                      **({'same_image': True} if (same_image and hasattr(self.model, "parameterization")) else {}))
        rescale_to_bpd = 1. / (float(np.prod(inputs['images'].shape[1:])) * math.log(2.))
        bpd_latent = outputs.loss_klz.mean() * rescale_to_bpd
        bpd_recon = outputs.loss_recon.mean() * rescale_to_bpd
        bpd_diff = outputs.loss_diff.mean() * rescale_to_bpd
        bpd = bpd_recon + bpd_latent + bpd_diff
        scalar_dict = {'bpd': bpd.detach(), 'bpd_latent': bpd_latent.detach(), 'bpd_recon': bpd_recon.detach(),
                       'bpd_diff': bpd_diff.detach(), 'var0': outputs.var_0.detach(), 'var': outputs.var_1.detach()}
        metrics = {'scalars': scalar_dict, 'images': {'inputs': inputs['images']}}
        return bpd, metrics

    def sample_fn(self, *, dummy_inputs, rng, params, T=1000, gather=True, sampler='ancestral', t_grid=None, eta=0.0,
                  grid='uniform', grid_rho=7.0):
        """Experiment_VDM.sample_fn (ldm/experiment_vdm.py:80-110): z_T ~ sigma_prior N(0, I), T ancestral steps
        (`model.sample`), `model.generate_x`; returns uint8 samples [B (* world), 32, 32, 3].  The noise stream is this
        build's Philox, folded with the rank like the reference folds axis_index.
        sampler (not in the reference): 'ancestral' (the reference's loop), or the deterministic few-step samplers 'ddim' /
        'dpm2m' (mulan_amd.sampling) over T uniform steps or the explicit t_grid (1 -> 0, strictly decreasing: it sets
        the step count); generate_x then draws with rng.fold_in(N) like the ancestral loop with fold_in(T).
        'sde2m' (SDE-DPM-Solver++(2M)) and 'ddim' with eta in (0, 1] are the stochastic few-step samplers: step k draws
        its noise under the key the ancestral loop folds with its step index (rng.fold_in(k) after the split below).
        grid, grid_rho: the kind of time grid of a few-step sampler (sampling.GRIDS; 'logsnr' and 'karras' are spaced
        on the mean schedule of the batch, model.fast_grid) -- over T steps, so not together with t_grid."""
        sampling.check_eta(sampler, eta)
        if sampler == 'ancestral' and t_grid is not None:
            raise ValueError("t_grid applies to the few-step samplers; the ancestral sampler runs T uniform steps")
        kind, grid_rho = sampling.check_grid(sampler, grid, t_grid, grid_rho)
        grid = None                                  # (a grid kind other than 'uniform' is made per batch, in fast_sample)
        if sampler != 'ancestral' and kind == 'uniform':
            grid = sampling.time_grid(None if t_grid is not None else T, t_grid)
        N = T if grid is None else len(grid) - 1
        rng = rng.fold_in(self.rank)
        B = dummy_inputs.shape[0]
        rng, sample_rng = rng.split()
        samples, _ = self.draw_samples(params, B, None, sample_rng, rng, rng.fold_in(N), sampler, N, t_grid=grid,
                                       prior_scale=float(self.config.model.sigma_prior), eta=eta, grid=kind,
                                       grid_rho=grid_rho)
        return parallel.all_gather_tensor(samples) if gather else samples

    def _packer_for(self, params):
        if params is self.state.ema_params:
            return self.state.param_packer("ema")
        if params is self.state.params:
            return self.state.param_packer("params")
        return None

    def draw_samples(self, params, B, embedding, prior_rng, step_rng, decode_rng, sampler, steps, t_grid=None,
                     prior_scale=1.0, stepper=None, eta=0.0, known=None, mask=None, resample=1, known_rng=None,
                     measurement=None, degradation=None, grid='uniform', grid_rho=7.0):
        """One batch of B images, the loop every sampling entry point runs: z_1 = prior_scale * N(0, I) from prior_rng,
        `steps` steps of `sampler` under `embedding` (MuLAN models; None: model.deterministic_embedding) with the per-step
        noise of the ancestral sampler from step_rng (rng.fold_in(i) at step i), generate_x with decode_rng (needed by
        sample_softmax).  The weights are packed once for the whole loop.  ancestral: the reverse step is a replayed HIP
        graph (model.GraphedReverseStep); ddim / dpm2m / sde2m (t_grid, if given, sets the step count):
        model.fast_sample, the stepper re-used when one is given (re-targeted at this batch's context) and returned for
        the next batch; sde2m and ddim with eta > 0 draw the noise of step k under step_rng.fold_in(k) as well.
        known (uint8 [B, 32, 32, 3]) and mask (bool or uint8 [32, 32], [B, 32, 32] or [B, 32, 32, 3], True = keep; it
        is broadcast to one byte per sub-pixel): inpainting with the few-step samplers (sampling.run), `resample`
        passes per step.  The noise of the known region and of the jumps comes from known_rng alone, a key that neither
        z_1 nor the step noise uses: draw j under known_rng.fold_in(j).  With argmax decoding the kept sub-pixels of
        the result are the input's, with no paste-over.
        measurement (fp32, in the scale of ops.encode_u8, shaped ops.restore_y_shape(B, 32, 32, 3, f, gray)) and
        degradation ('sr:f', 'gray', 'sr:f+gray'): restoration with the few-step samplers instead (sampling.run):
        every step's prediction is projected onto the measurement.  resample > 1 draws jump j under known_rng.fold_in(j);
        resample = 1 draws nothing from known_rng and needs none.  A mask and a measurement in one run are refused.
        grid, grid_rho: the kind of time grid of a few-step sampler (sampling.GRIDS; not with t_grid); 'logsnr' and
        'karras' are spaced on the mean schedule of this batch's embeddings (model.fast_grid).
        -> (uint8 [B, 32, 32, 3], stepper or None)"""
        step_eta = sampling.check_eta(sampler, eta)          # what the steps run with: 1 for sde2m
        inpaint, restore, resample = sampling.check_guidance(sampler, known, mask, measurement, degradation, resample)
        grid, grid_rho = sampling.check_grid(sampler, grid, t_grid, grid_rho)
        if restore is not None:
            if resample > 1 and known_rng is None:
                raise ValueError("draw_samples: resample > 1 needs known_rng, the key of the jumps' noise")
            measurement = torch.as_tensor(measurement)
            if measurement.dtype != torch.float32:
                raise ValueError(f"draw_samples: the measurement is fp32 in the encoded scale, got {measurement.dtype}")
        if inpaint:
            if known_rng is None:
                raise ValueError("draw_samples: inpainting needs known_rng, the key of the known region's noise")
            known = torch.as_tensor(known)
            if known.dtype != torch.uint8 or tuple(known.shape) != (B, 32, 32, 3):
                raise ValueError(f"draw_samples: known is uint8 [{B}, 32, 32, 3], got {known.dtype} "
                                 f"{list(known.shape)}")
            mask = sampling.expand_mask(mask, B, self.device)
        packer = self._packer_for(params)
        conditioning = torch.zeros(B, dtype=torch.uint8, device=self.device)
        mulan = hasattr(self.model, "reverse_stepper")
        with torch.no_grad():
            if packer is not None:
                packer.refresh()                     # weights are constant over the steps: prepare them once
            try:
                z = float(prior_scale) * prior_rng.normal((B, 3072), self.device)
                if mulan and embedding is None:
                    embedding = self.model.deterministic_embedding(B, self.device)
                coeffs = None
                if sampler == 'ancestral':
                    if mulan:
                        # MuLAN models: the embedding of the sampler is fixed, so the schedule's coefficients are formed
                        # once, and the reverse step is a replayed HIP graph (MULAN_SAMPLER_GRAPH=0: eager)
                        coeffs = self.model.sample_coefficients(params, embedding)
                        step = self.model.reverse_stepper(params, B, self.device, embedding, conditioning, coeffs, steps)
                        for i in range(steps):
                            z = step(i, z, step_rng)
                    else:
                        for i in range(steps):
                            z = self.model.sample(params, i, steps, z, conditioning, step_rng, coeffs)
                else:
                    ctx = self.model.fast_context(params, embedding if mulan else None, conditioning)
                    if stepper is None:
                        stepper = self.model.fast_stepper(params, B, self.device, ctx, step_eta=step_eta,
                                                          inpaint=inpaint, restore=restore)
                    kw = {}                          # what guides the run: a measurement, or a known image, or nothing
                    if restore is not None:
                        kw = dict(measurement=measurement.to(self.device), degradation=restore)
                    elif inpaint:
                        from . import ops
                        kw = dict(known=ops.encode_u8(known.to(self.device)).reshape(B, 3072), mask=mask)
                    if kw:
                        kw.update(resample=resample, known_noise=known_rng)
                    z = self.model.fast_sample(params, z, ctx, sampler, None if t_grid is not None else steps, t_grid,
                                               stepper=stepper, eta=eta, noise=step_rng if step_eta > 0.0 else None,
                                               grid=grid, grid_rho=grid_rho, **kw)
                    coeffs = ctx.get("coeffs")
                samples = self.model.generate_x(params, z, coeffs, rng=decode_rng)
            finally:
                if packer is not None:
                    packer.invalidate()
        return samples, stepper
