"""Variational-bound BPD evaluators (mirror of ldm/notebook_utils.py:28-39,157-191).

dense : per test image, a batch of `n_timesteps` copies -> antithetic t covers [0,1) with spacing
        1/n_timesteps, i.e. a Riemann estimate of the diffusion-loss integral; the SAME rng key for every
        image (PRNGKey(0), notebook_utils.py:178).  Images are independent, so under torchrun the test set
        is sharded by index across ranks and (sum bpd, count) is all-reduced once at the end.
sparse: batches of batch_size_eval distinct images, same fixed key (notebook_utils.py:157-173).
"""
import contextlib
import os

import numpy as np
import torch
import torch.distributed as dist

from . import checkpoint as ckpt_lib
from . import data as dataset
from . import parallel
from . import sampling
from .experiment import Experiment_VDM
from .rng import PRNGKey


class Experiment_Colab(Experiment_VDM):
    """Experiment_VDM + EMA parameters restored from `<dir>/ckpt-<N>` (ldm/notebook_utils.py:28-39)."""

    def __init__(self, config, checkpoint_dir, checkpoint_num=None):
        super().__init__(config)
        if checkpoint_num is None:
            sd = ckpt_lib.restore_dict(checkpoint_dir)
        else:
            sd = ckpt_lib.restore_dict(os.path.join(checkpoint_dir, f'ckpt-{checkpoint_num}'))
        self.state.load_state_dict({"ema_params": sd["ema_params"]}, strict=True)
        self.orig_params = self.state.ema_params
        self.params = self.orig_params
        self.rng, sample_rng = self.rng.split()
        self.rngs = {'sample': sample_rng}

    # ---- samplers of the notebook front end (ldm/notebook_utils.py:54-135) --------------------------------------
    def _embedding_samples(self, embedding, rng, T, sampler='ancestral', eta=0.0, grid='uniform', grid_rho=7.0):
        """T steps of `sampler` under a fixed [B, 50] embedding (ancestral: model.conditional_sample), then generate_x
        (Experiment_VDM.draw_samples; z_1 ~ N(0, I) as the notebook draws it)"""
        rng = rng.fold_in(self.rank)
        rng, sample_rng = rng.split()
        samples, _ = self.draw_samples(self.params, embedding.shape[0], embedding, sample_rng, rng, rng.fold_in(T),
                                       sampling.check_sampler(sampler), T, eta=eta, grid=grid, grid_rho=grid_rho)
        return parallel.all_gather_tensor(samples)

    @staticmethod
    def _steps(T, sampler):
        """T of the notebook samplers: 1000 ancestral steps by default, 25 for ddim / dpm2m / sde2m (as p_sample)"""
        if T is not None:
            return T
        return 1000 if sampling.check_sampler(sampler) == 'ancestral' else 25

    def sample_conditionally(self, embedding, T=None, sampler='ancestral', eta=0.0, grid='uniform', grid_rho=7.0):
        """Experiment_Colab.sample_conditionally: an image grid sampled under one 50-dim k-hot embedding (sampler, eta,
        grid, grid_rho: see Experiment_VDM.sample_fn; T is the step count, by default 1000 ancestral / 25 few-step)"""
        sampling.check_eta(sampler, eta)
        sampling.check_grid(sampler, grid, None, grid_rho)
        B = self.eval_iter.local
        emb = torch.as_tensor(embedding, dtype=torch.float32, device=self.device).reshape(1, -1)
        assert emb.shape[1] == 50
        samples = self._embedding_samples(emb.expand(B, 50).contiguous(), self.rng, self._steps(T, sampler), sampler,
                                          eta, grid, grid_rho)
        return ckpt_lib.generate_image_grids(samples).astype(np.uint8)

    def sample_randomly(self, T=None, sampler='ancestral', eta=0.0, grid='uniform', grid_rho=7.0):
        """Experiment_Colab.sample_randomly: every image under the hard top-15 embedding of its own random logits
        (grid, grid_rho: the time grid of a few-step sampler, see Experiment_VDM.sample_fn)"""
        from . import ops
        sampling.check_eta(sampler, eta)
        sampling.check_grid(sampler, grid, None, grid_rho)
        B = self.eval_iter.local
        _, embeddings_rng = self.rng.fold_in(self.rank).split()
        emb, _ = ops.topk_hard(embeddings_rng.normal((B, 50), self.device), 15)
        samples = self._embedding_samples(emb, self.rng, self._steps(T, sampler), sampler, eta, grid, grid_rho)
        return ckpt_lib.generate_image_grids(samples).astype(np.uint8)

    KNOWN_NOISE_FOLD = 0x6B6E6F776E5F7869        # fold_in tag of a batch's known-region key: no step count reaches it

    def _check_embedding(self, embedding, batch_size, inpaint):
        """the refusals of sample_batches' `embedding`, before anything is drawn"""
        mulan = hasattr(self.model, "deterministic_embedding")
        if torch.is_tensor(embedding) or isinstance(embedding, np.ndarray):
            if not inpaint:
                raise ValueError("embedding must be 'deterministic' or 'random' where nothing is inpainted")
            if not mulan:
                raise ValueError("an explicit embedding needs a MuLAN model (model_vdm.VDM has no latent embedding)")
            if tuple(embedding.shape) not in ((50,), (batch_size, 50)):
                raise ValueError(f"an explicit embedding is [50] or [{batch_size}, 50], got {list(embedding.shape)}")
            return
        names = ('deterministic', 'random', 'encoder') if inpaint else ('deterministic', 'random')
        if embedding not in names:
            raise ValueError(f"embedding must be {' or '.join(repr(n) for n in names)}, got {embedding!r}")
        if embedding != 'deterministic' and not mulan:
            raise ValueError(f"embedding={embedding!r} needs a MuLAN model (model_vdm.VDM has no latent embedding)")
        if embedding == 'encoder' and self.model.config.latent_type == 'gaussian':
            raise ValueError("embedding='encoder' takes the hard top-k of the encoder's logits; latent_type 'gaussian' "
                             "has none")

    def _batch_embedding(self, embedding, k_e, batch_size, known=None, mask=None, measurement=None, restore=None):
        """the [B, 50] embedding of one batch (None: draw_samples takes the model's deterministic one)"""
        from . import ops
        if not isinstance(embedding, str):
            emb = torch.as_tensor(embedding, dtype=torch.float32, device=self.device)
            return emb.reshape(-1, 50).expand(batch_size, 50).contiguous()
        if embedding == 'random':
            return ops.topk_hard(k_e.normal((batch_size, 50), self.device), 15)[0]
        if embedding == 'encoder' and restore is not None:
            # the encoder sees A+ y: every group's measured value at all of its sub-pixels, as 8-bit levels
            f, gray = restore
            y = torch.as_tensor(measurement).to(self.device)
            up = y.repeat_interleave(f, 1).repeat_interleave(f, 2).expand(batch_size, 32, 32, 3)
            levels = ((up + 1.0) * 128.0 - 0.5).round().clamp(0, 255).to(torch.uint8).contiguous()   # encode_u8 inverted
            return ops.topk_hard(self.model.apply_encoder(self.params, levels), self.model.config.latent_k)[0]
        if embedding == 'encoder':
            keep = sampling.expand_mask(mask, batch_size, self.device).view(batch_size, 32, 32, 3) != 0
            known = torch.as_tensor(known).to(self.device)
            grey = torch.where(keep, known, torch.full_like(known, 128))
            return ops.topk_hard(self.model.apply_encoder(self.params, grey), self.model.config.latent_k)[0]
        return None

    def sample_batches(self, keys, batch_size, embedding='deterministic', sampler='dpm2m', steps=25, eta=0.0, known=None,
                       mask=None, resample=1, measurement=None, degradation=None, grid='uniform', grid_rho=7.0):
        """uint8 [batch_size, 32, 32, 3] per key, each batch drawn from its key alone (the python -m ldm.sample CLI):
        key.split(3) -> (prior z_1 ~ sigma_prior N(0, I), random embedding logits, per-step noise); generate_x with
        key.fold_in(steps).  The per-step noise of the ancestral sampler, of sde2m and of ddim with eta > 0 comes from
        the third sub-key alone, folded with the step index, so neither z_1 nor the embedding shares a draw with it.
        embedding 'deterministic': model.deterministic_embedding (as sample_fn); 'random': the hard top-15 of random
        normal logits (as sample_randomly).  The few-step samplers re-use one stepper, re-targeted at every batch's
        context.
        known, mask (optional, one per key: uint8 [batch_size, 32, 32, 3] and a mask as draw_samples takes it; one
        mask alone serves every batch): inpainting, `resample` passes per step.  The noise of the known region and of
        the jumps comes from a fourth sub-key, key.fold_in(KNOWN_NOISE_FOLD), folded with the draw's own counter
        (sampling.run); the three sub-keys above and their draws are as without a mask.  Inpainting also takes
        embedding 'encoder' (the hard top-k of apply_encoder on the images with the unknown pixels set to 128) or an
        explicit k-hot tensor [50] or [batch_size, 50].
        measurement (one per key: fp32 in the scale of ops.encode_u8, shaped ops.restore_y_shape) and degradation
        ('sr:f', 'gray' or 'sr:f+gray', one for all): restoration instead (draw_samples), `resample` passes per step.
        The jumps of resample > 1 draw from the same fourth sub-key; resample = 1 draws nothing from it.  The embeddings
        of inpainting apply, 'encoder' on the replicated measurement A+ y rounded to 8-bit levels.
        grid, grid_rho: the kind of time grid of a few-step sampler (sampling.GRIDS).  'logsnr' and 'karras' are spaced
        on the mean schedule of the batch's own embeddings, so a batch still depends on its key alone."""
        sampling.check_eta(sampler, eta)
        sampling.check_grid(sampler, grid, None, grid_rho)
        keys = list(keys)
        inpaint, restore, resample = sampling.check_guidance(sampler, known, mask, measurement, degradation, resample)
        if restore is not None:
            if torch.is_tensor(measurement) or isinstance(measurement, np.ndarray) or len(measurement) != len(keys):
                raise ValueError(f"{len(keys)} keys need a list of {len(keys)} measurements, one per batch")
        if inpaint:
            if torch.is_tensor(mask) or isinstance(mask, np.ndarray):
                mask = [mask] * len(keys)
            if len(known) != len(keys) or len(mask) != len(keys):
                raise ValueError(f"{len(keys)} keys, but {len(known)} batches of known images and {len(mask)} masks")
        self._check_embedding(embedding, batch_size, inpaint or restore is not None)
        out, stepper = [], None
        for b, key in enumerate(keys):
            k_z, k_e, k_s = key.split(3)
            kw = {}                                  # what guides batch b: a measurement, or a known image, or nothing
            if restore is not None:
                kw = dict(measurement=measurement[b], degradation=degradation)
            elif inpaint:
                kw = dict(known=known[b], mask=mask[b])
            if kw:
                kw.update(resample=resample, known_rng=key.fold_in(self.KNOWN_NOISE_FOLD))
            emb = self._batch_embedding(embedding, k_e, batch_size, kw.get("known"), kw.get("mask"),
                                        kw.get("measurement"), restore)
            x, stepper = self.draw_samples(self.params, batch_size, emb, k_z, k_s, key.fold_in(steps), sampler, steps,
                                           prior_scale=float(self.config.model.sigma_prior), stepper=stepper, eta=eta,
                                           grid=grid, grid_rho=grid_rho, **kw)
            out.append(x)
        return out

    def inpaint(self, images, mask, embedding='deterministic', sampler='sde2m', steps=25, eta=0.0, resample=1, rng=None,
                grid='uniform', grid_rho=7.0):
        """uint8 [B, 32, 32, 3]: `images` (uint8 [B, 32, 32, 3]) with the sub-pixels outside `mask` (bool or uint8
        [32, 32], [B, 32, 32] or [B, 32, 32, 3], True = keep) drawn by a few-step sampler (ddim with eta, dpm2m, sde2m)
        that overwrites the kept ones after every step with their own alpha_t x + sigma_t eps (sampling.run;
        resample > 1: that many passes per step).  With argmax decoding (sample_softmax False) the kept sub-pixels come
        back as they went in, with no paste-over.  embedding: 'deterministic', 'random', 'encoder' (MuLAN models: the hard
        top-k of apply_encoder on the images with the unknown pixels set to 128) or a k-hot tensor [50] or [B, 50].
        rng (default: the experiment's key) is folded with the rank and then split as sample_batches splits a batch's
        key, so the same rng gives the same bytes.  grid, grid_rho: the time grid, as sample_batches takes it."""
        images = torch.as_tensor(images)
        if images.dtype != torch.uint8 or images.dim() != 4 or tuple(images.shape[1:]) != (32, 32, 3):
            raise ValueError(f"images are uint8 [B, 32, 32, 3], got {images.dtype} {list(images.shape)}")
        key = (self.rng if rng is None else rng).fold_in(self.rank)
        return self.sample_batches([key], images.shape[0], embedding, sampler, steps, eta, known=[images], mask=[mask],
                                   resample=resample, grid=grid, grid_rho=grid_rho)[0]

    def restore(self, images=None, measurement=None, degradation='sr:4', embedding='deterministic', sampler='sde2m',
                steps=25, eta=0.0, resample=1, rng=None, grid='uniform', grid_rho=7.0):
        """(restored uint8 [B, 32, 32, 3], residual fp32 [B]): images consistent with a degraded observation, drawn by a
        few-step sampler whose every prediction is projected onto the measurement (sampling.run).
        degradation: 'sr:f' (the f x f average-pooled image, f in 2, 4, 8, 16), 'gray' (the channel mean) or 'sr:f+gray'.
        Exactly one of: images (uint8 [B, 32, 32, 3]), which are degraded here (ops.restore_measure on their encoding),
        or measurement ([B, 32 / f, 32 / f, 3 or 1 with gray]; fp32 in the scale of ops.encode_u8, or uint8 levels, which
        are encoded like an image).  residual: the largest |A encode(restored) - y| of each image in grey levels
        (x 127.5): what per-pixel schedules inside a group and the 8-bit decoding leave of A x = y; reported, not
        asserted.  resample = U > 1: U passes per step.  embedding as inpaint takes it, 'encoder' on the replicated
        measurement.  rng as inpaint.  grid, grid_rho: the time grid, as sample_batches takes it."""
        from . import ops
        f, gray = sampling.parse_degradation(degradation)
        if (images is None) == (measurement is None):
            raise ValueError("restore takes the images to degrade or their measurement, one of the two")
        if images is not None:
            images = torch.as_tensor(images)
            if images.dtype != torch.uint8 or images.dim() != 4 or tuple(images.shape[1:]) != (32, 32, 3):
                raise ValueError(f"images are uint8 [B, 32, 32, 3], got {images.dtype} {list(images.shape)}")
            B = images.shape[0]
            y = ops.restore_measure(ops.encode_u8(images.to(self.device)), f, gray)
        else:
            y = torch.as_tensor(measurement)
            B = y.shape[0] if y.dim() == 4 else 0
            if B < 1 or tuple(y.shape) != ops.restore_y_shape(B, 32, 32, 3, f, gray) or \
                    y.dtype not in (torch.uint8, torch.float32):
                raise ValueError(f"the measurement of {degradation!r} is uint8 or fp32 "
                                 f"{['B', *ops.restore_y_shape(1, 32, 32, 3, f, gray)[1:]]}, got {y.dtype} {list(y.shape)}")
            y = y.to(self.device)
            y = ops.encode_u8(y) if y.dtype == torch.uint8 else y.contiguous()
        key = (self.rng if rng is None else rng).fold_in(self.rank)
        out = self.sample_batches([key], B, embedding, sampler, steps, eta, resample=resample, measurement=[y],
                                  degradation=degradation, grid=grid, grid_rho=grid_rho)[0]
        back = ops.restore_measure(ops.encode_u8(out), f, gray)
        return out, (back - y).abs().reshape(B, -1).amax(dim=1) * 127.5

    def test(self, loader):
        """Experiment_Colab.test: mean of the eval scalars over a loader"""
        eval_metrics = []
        for eval_step, batch in enumerate(loader):
            m = self.p_eval_step(self.params, batch, eval_step)
            eval_metrics.append({k: float(v) for k, v in m['scalars'].items()})
        return {k: float(np.mean([m[k] for m in eval_metrics])) for k in eval_metrics[0]}


@contextlib.contextmanager
def _packed_weights(experiment):
    """The evaluated weights are constant over an evaluation: their maxima and split fp16 operands are prepared once
    (ParamPacker, two launches) instead of per layer and call."""
    st = experiment.state
    params = getattr(experiment, "orig_params", None)
    which = "ema" if params is st.ema_params else ("params" if params is st.params else None)
    packer = st.param_packer(which) if which else None
    if packer is not None:
        packer.refresh()
    try:
        yield
    finally:
        if packer is not None:
            packer.invalidate()


def _reduce_mean(total, count, device):
    if parallel.world_size() > 1:
        t = torch.tensor([total, float(count)], dtype=torch.float64, device=device)
        dist.all_reduce(t, op=dist.ReduceOp.SUM)
        total, count = float(t[0]), int(t[1])
    return total / max(count, 1), count


def _dense_partial(experiment, config, n_timesteps, rank, world, max_images=0):
    """(sum of per-image BPDs, image count) of the images rank `rank` of `world` evaluates: image i goes to rank
    i % world; every image is a batch of n_timesteps copies under the SAME key PRNGKey(0) (notebook_utils.py:176-191)"""
    loader = dataset.create_one_time_eval_dataset(config, 1, experiment.device, rank, world)
    rng = PRNGKey(0)
    total, count = 0.0, 0
    with _packed_weights(experiment):
        for eval_step, batch in enumerate(loader):
            if max_images and eval_step * world + rank >= max_images:
                break
            images = batch['images'].reshape(1, 32, 32, 3).expand(n_timesteps, 32, 32, 3).contiguous()
            tiled = {'images': images, 'labels': batch['labels'].expand(n_timesteps),
                     'conditioning': torch.zeros(n_timesteps, dtype=torch.uint8, device=experiment.device)}
            with torch.no_grad():
                bpd, _ = experiment.loss_fn(experiment.orig_params, tiled, eval_step, rng=rng, is_train=False,
                                            same_image=True)
            total += float(bpd)
            count += 1
            if count % 100 == 0 and rank == 0:
                print(f'eval_step {count} cum_avg_bpd {total / count} ')
    return total, count


def eval_bpd_dense_sampling(experiment, config, n_timesteps=128, max_images=0):
    total, count = _dense_partial(experiment, config, n_timesteps, experiment.rank, experiment.world, max_images)
    mean, n = _reduce_mean(total, count, experiment.device)
    if experiment.rank == 0:
        print('Num eval steps:', n)
    return mean


def _sparse_partial(experiment, config, rank, world, max_images=0):
    """(sum of per-batch BPDs, batch count): batches of config.training.batch_size_eval DISTINCT images, the reference's
    global batch on every rank that evaluates one (the antithetic time grid spans the whole batch,
    notebook_utils.py:157-173), whole batches dealt round-robin to the ranks"""
    batch_size = config.training.batch_size_eval
    loader = dataset.create_one_time_eval_dataset(config, batch_size, experiment.device, rank, world)
    rng = PRNGKey(0)
    total, count = 0.0, 0
    with _packed_weights(experiment):
        for eval_step, batch in enumerate(loader):
            if max_images and (eval_step * world + rank) * batch_size >= max_images:
                break
            with torch.no_grad():
                bpd, _ = experiment.loss_fn(experiment.orig_params, batch, eval_step, rng=rng, is_train=False)
            total += float(bpd)
            count += 1
            if count % 100 == 0 and rank == 0:
                print(f'eval_step {count} cum_avg_bpd {total / count} ')
    return total, count


def eval_bpd_sparse_sampling(experiment, config, max_images=0):
    total, count = _sparse_partial(experiment, config, experiment.rank, experiment.world, max_images)
    mean, n = _reduce_mean(total, count, experiment.device)
    if experiment.rank == 0:
        print('Num eval steps:', n)
    return mean


# ------------------------------------------------------------------ exact likelihood (probability-flow ODE)
GAMMA_TN = -13.3                  # `gt` hard-coded in get_ode_likelihood_fn / _get_bpd_offset (notebook_utils.py:321,452)
TN_LOG_Z = float(np.log(0.9974613))          # mass of N(0,1) on [-3, 3] as the reference rounds it (:331)


class Hutchinson:
    """notebook_utils.Hutchinson (:232-260): one probe per function evaluation, or one fixed probe"""

    def __init__(self, hutchinson_type, shape, rng, device, deterministic=False):
        if hutchinson_type not in ('Rademacher', 'Gaussian'):
            raise ValueError(f'hutchinson_type {hutchinson_type}')
        self.kind, self.shape, self.rng, self.device = hutchinson_type, shape, rng, device
        self.deterministic = deterministic
        if deterministic:
            self.det_noise = self._draw(rng)

    def _draw(self, key):
        from . import ops
        if self.kind == 'Gaussian':
            return key.normal(self.shape, self.device)
        return ops.noise(self.shape, key.v, 0, self.device, 'rademacher')

    def noise(self):
        if self.deterministic:
            return self.det_noise
        self.rng, key = self.rng.split()
        return self._draw(key)


def get_ode_likelihood_fn(experiment, hutchinson_type='Rademacher', rtol=1e-5, atol=1e-5, method='RK45',
                          dequantization='uniform', high_precision=False):
    """get_ode_likelihood_fn (ldm/notebook_utils.py:263-373).  Returns likelihood_fn(rng, data_u8 [B,32,32,3],
    deterministic_noise=False, u=None, probes=None) -> (log_p [B] float64, log_q_eps [B] | None, aux_loss [B], info).
    `u` (dequantisation noise: U[0,1) for 'uniform', standard normal on [-3, 3] for 'tn') and `probes` (a callable
    returning the Hutchinson probe of each function evaluation) override the Philox draws and `t_grid` replaces the
    adaptive controller by fixed Dormand-Prince steps: parity tests pass them."""
    from . import ops
    from .model import ode_function
    from .ode import solve_fixed, solve_rk45
    if method != 'RK45':
        raise NotImplementedError("the reference only ever passes method='RK45' (ldm/notebook_utils.py:264)")
    if dequantization not in ('uniform', 'tn'):
        raise AssertionError(dequantization)
    model, params, dev = experiment.model, experiment.orig_params, experiment.device
    packer = experiment.state.param_packer("ema") if params is experiment.state.ema_params else None
    graphs = {}          # captured function evaluations, re-used from batch to batch (model.ode_function)

    def likelihood_fn(rng, data, deterministic_noise=False, u=None, probes=None, t_grid=None):
        rng, init_noise_rng = rng.split()
        x = data.reshape(-1, 3072).contiguous()
        B = x.shape[0]
        if dequantization == 'uniform':
            if u is None:
                u = ops.noise((B, 3072), init_noise_rng.v, 0, dev, 'uniform')
            y, requant = ops.dequantize(x, u, True)
            log_q_eps = None
        else:
            if u is None:
                u = ops.noise((B, 3072), init_noise_rng.v, 0, dev, 'truncated_normal', -3.0, 3.0)
            log_q_eps = ops.normal_logp(u).double() - 3072 * TN_LOG_Z
            y, requant = ops.dequantize(x, u, False, float(np.exp(np.float32(0.5 * GAMMA_TN))))
        if packer is not None:
            packer.refresh()
        try:
            ctx = model.ode_context(params, requant)
            rng, hutchinson_rng = rng.split()
            hutch = Hutchinson(hutchinson_type, (B, 3072), hutchinson_rng, dev, deterministic=deterministic_noise)
            draw = probes if probes is not None else hutch.noise
            n_x = B * 3072

            f = ode_function(model, params, ctx, B, dev, True, cache=graphs, high_precision=high_precision)   # a replayed HIP graph

            def ode_func(t, y32, out):
                f(t, y32[:n_x].view(B, 3072), draw(), out[:n_x].view(B, 3072), out[n_x:])

            y0 = torch.cat([y.reshape(-1).double(), torch.zeros(B, device=dev, dtype=torch.float64)])
            sol = (solve_rk45(ode_func, y0, (0.0, 1.0), rtol=rtol, atol=atol) if t_grid is None
                   else solve_fixed(ode_func, y0, t_grid))
        finally:
            if packer is not None:
                packer.invalidate()
        z = sol.y[:n_x].float().view(B, 3072)
        log_p = ops.normal_logp(z).double() + sol.y[n_x:].float().double()
        return log_p, log_q_eps, ctx["kl"], dict(nfev=sol.nfev, steps=sol.steps, rejected=sol.rejected, z=z)

    return likelihood_fn


def get_sample_fn(experiment, hutchinson_type='Rademacher', rtol=1e-5, atol=1e-5, method='RK45', high_precision=False):
    """get_sample_fn (ldm/notebook_utils.py:376-443): samples by integrating the probability-flow ODE from the prior
    at t = 1 down to t = 0, conditioned on the hard top-k embedding of random normal logits.  Returns
    sample_fn(rng, deterministic_noise=False, sample_size=32, t_grid=None) -> (z [sample_size, 32, 32, 3] fp32, nfev).
    The reference evaluates the Hutchinson divergence at every step and throws it away; only the drift is computed
    here (so hutchinson_type / deterministic_noise have no effect on the result, as in the reference)."""
    from . import ops
    from .model import ode_function
    from .ode import solve_fixed, solve_rk45
    if method != 'RK45':
        raise NotImplementedError("the reference only ever passes method='RK45'")
    model, params, dev = experiment.model, experiment.orig_params, experiment.device
    packer = experiment.state.param_packer("ema") if params is experiment.state.ema_params else None

    def sample_fn(rng, deterministic_noise=False, sample_size=32, t_grid=None):
        rng, logits_rng = rng.split()
        emb, _ = ops.topk_hard(logits_rng.normal((sample_size, 50), dev), 15)
        rng, _hutchinson_rng = rng.split()
        rng, prior_rng = rng.split()
        prior = prior_rng.normal((sample_size, 3072), dev)
        if packer is not None:
            packer.refresh()
        try:
            ctx = model.ode_context_from_embedding(params, emb)

            f = ode_function(model, params, ctx, sample_size, dev, False, high_precision=high_precision)

            def ode_func(t, y32, out):
                f(t, y32.view(sample_size, 3072), None, out.view(sample_size, 3072))

            y0 = prior.reshape(-1).double()
            sol = (solve_rk45(ode_func, y0, (1.0, 0.0), rtol=rtol, atol=atol) if t_grid is None
                   else solve_fixed(ode_func, y0, t_grid))
        finally:
            if packer is not None:
                packer.invalidate()
        return sol.y.float().view(sample_size, 32, 32, 3), sol.nfev

    return sample_fn


def get_logits(experiment, num_batches=30):
    """notebook_utils.get_logits (:534-545): encoder logits and the images they belong to, over eval batches"""
    logits, images = [], []
    for _ in range(num_batches):
        batch = experiment.eval_iter.next()
        logits.append(experiment.model.apply_encoder(experiment.orig_params, batch['images']))
        images.append(batch['images'])
    return torch.cat(logits), torch.cat(images)


def logits_to_embeddings(logits):
    """notebook_utils.logits_to_embeddings (:548-551): hard top-15 k-hot"""
    from . import ops
    return ops.topk_hard(logits, 15)[0]


def _get_bpd_offset(dequantization, num_is):
    """notebook_utils._get_bpd_offset (:446-458)"""
    if dequantization == 'uniform':
        return float(np.log2(128))
    if dequantization == 'tn':
        log_sigma = 0.5 * (GAMMA_TN - float(np.logaddexp(GAMMA_TN, 0.0)))
        extra = 0.5 * (1 + float(np.log(2 * np.pi))) - 0.01522 if num_is == 1 else 0.0
        return -(extra + log_sigma) / float(np.log(2))
    raise AssertionError(dequantization)


def _logsumexp0(a):
    m = a.max(axis=0)
    return m + np.log(np.exp(a - m).sum(axis=0))


def _eval_bpd_ode(experiment, config, rng, deterministic_noise, hutchinson_type, dequantization='tn', num_is=1,
                  rtol=1e-5, atol=1e-5, max_images=0):
    """notebook_utils._eval_bpd_ode (:480-531): per batch, num_is likelihood draws, importance-weighted bound,
    running mean over batches.  Under torchrun whole global batches (config.training.batch_size_eval images, as in the
    reference) are dealt round-robin to the ranks: every batch is integrated by one rank exactly as a single device
    would (same step-size controller input), so the result does not depend on the world size."""
    batch_size = config.training.batch_size_eval
    loader = dataset.create_one_time_eval_dataset(config, batch_size, experiment.device, experiment.rank,
                                                  experiment.world)
    likelihood_function = get_ode_likelihood_fn(experiment, rtol=rtol, atol=atol, hutchinson_type=hutchinson_type,
                                                dequantization=dequantization)
    bpd_offset = _get_bpd_offset(dequantization, num_is)
    total, count = 0.0, 0
    for eval_step, batch in enumerate(loader):
        if max_images and (eval_step * experiment.world + experiment.rank) * batch_size >= max_images:
            break
        log_ps, log_qs, aux_loss = [], [], None
        for _ in range(num_is):
            rng, likelihood_rng = rng.split()
            log_p, log_q_eps, aux, _ = likelihood_function(likelihood_rng, batch['images'],
                                                           deterministic_noise=deterministic_noise)
            log_ps.append(log_p.cpu().numpy())
            log_qs.append(None if log_q_eps is None else log_q_eps.cpu().numpy())
            aux_loss = aux.double().cpu().numpy()
        log_ps = np.asarray(log_ps)
        if num_is == 1:
            iws = log_ps[0]
        else:
            if log_qs[0] is None:
                raise TypeError("importance weighting needs dequantization='tn' (the reference subtracts None here)")
            iws = _logsumexp0(log_ps - np.asarray(log_qs)) - np.log(num_is)
        bpd = float(np.mean(-iws + aux_loss) / (32 * 32 * 3 * np.log(2)) + bpd_offset)
        total += bpd
        count += 1
        if experiment.rank == 0:
            print('Eval step:{}\tcum. bpd: {:.3f}'.format(eval_step, total / count))
    mean, n = _reduce_mean(total, count, experiment.device)
    if experiment.rank == 0:
        print('Num eval steps:', n)
    return mean


def eval_bpd_ode(experiment, config, deterministic_noise, hutchinson_type, dequantization='tn', num_is=1, num_iters=1,
                 rtol=1e-5, atol=1e-5, max_images=0):
    """notebook_utils.eval_bpd_ode (:461-477)"""
    bpd_means = []
    rng = PRNGKey(0)
    for i in range(num_iters):
        rng, iter_rng = rng.split()
        mean = _eval_bpd_ode(experiment=experiment, config=config, rng=iter_rng, deterministic_noise=deterministic_noise,
                             hutchinson_type=hutchinson_type, dequantization=dequantization, num_is=num_is, rtol=rtol,
                             atol=atol, max_images=max_images)
        if experiment.rank == 0:
            print(f'[Iter {i}] Test BPD:{mean}')
        bpd_means.append(mean)
    return float(np.mean(bpd_means))


# ------------------------------------------------------------------ the learned noise schedule (notebook_utils.py:554-711)
SCHEDULE_BUFFER_BYTES = 1 << 30   # device budget of one launch's outputs (1 GiB): the embeddings go through in chunks of it
REC709 = (0.2125, 0.7154, 0.0721)            # the luminance weights of skimage.color.rgb2gray


def _schedule_inputs(experiment, embeddings, time_steps):
    """(embeddings fp32 [E, latent_size] on the device, times fp32 [T] on the device) or ValueError"""
    model = experiment.model
    if not hasattr(model, "deterministic_embedding"):
        raise ValueError("the schedule per embedding needs a MuLAN model (model_vdm.VDM has one scalar schedule and no "
                         "latent embedding)")
    if not torch.is_tensor(embeddings):
        embeddings = torch.as_tensor(np.asarray(embeddings, dtype=np.float32))
    L = model.config.latent_size
    if embeddings.dim() != 2 or embeddings.shape[0] < 1 or embeddings.shape[1] != L:
        raise ValueError(f"embeddings are [E, {L}] with E >= 1, got {list(embeddings.shape)}")
    if time_steps is None:
        time_steps = np.linspace(0.0, 1.0, 128)
    if torch.is_tensor(time_steps):
        time_steps = time_steps.detach().cpu().numpy()
    t = np.asarray(time_steps, dtype=np.float32).reshape(-1)
    if t.size < 1 or not np.isfinite(t).all() or t.min() < 0.0 or t.max() > 1.0:
        raise ValueError("time_steps are finite times in [0, 1], at least one")
    dev = experiment.device
    return embeddings.to(device=dev, dtype=torch.float32).contiguous(), torch.from_numpy(t).to(dev)


def _schedule_chunks(experiment, emb, bytes_per_embedding):
    """(first index, a, b, c) of consecutive chunks of the embeddings, each chunk's outputs within SCHEDULE_BUFFER_BYTES;
    the coefficient MLP (poly_coefficients) runs once per embedding"""
    from .model import poly_coefficients
    step = max(1, SCHEDULE_BUFFER_BYTES // bytes_per_embedding)
    for i in range(0, emb.shape[0], step):
        with torch.no_grad():
            yield (i, *poly_coefficients(experiment.orig_params["gamma"], emb[i:i + step].contiguous()))


def noise_schedule_per_embedding(experiment, embeddings, time_steps=None):
    """notebook_utils.noise_schedule_per_embedding (:554-568): a list of E numpy arrays [T, 3072], gamma of every
    sub-pixel at the T times (default linspace(0, 1, 128); any T -- the reference's repeat(128) ties T to 128) under each
    row of `embeddings` [E, latent_size].  One launch of mulan_schedule_curves per chunk of embeddings."""
    from . import ops
    emb, t = _schedule_inputs(experiment, embeddings, time_steps)
    cfg = experiment.model.config
    out = []
    for _, a, b, c in _schedule_chunks(experiment, emb, t.numel() * 3072 * 4):
        gamma, _, _ = ops.schedule_curves(a, b, c, t, cfg.gamma_min, cfg.gamma_max)
        out.extend(gamma.cpu().numpy())
    return out


def noise_schedule_summary(experiment, embeddings, time_steps=None, bins=100):
    """What the reference's schedule plots show, without a curve leaving the device: a dict of numpy arrays -- mean, std
    (population), min, max, sigma2_mean (the mean of sigmoid(gamma)), each [E, T], over the 3072 sub-pixels of embedding e
    at time t; channel_mean [E, T, 3]; hist [E, T, bins], the counts over [gamma_min, gamma_max] in equal bins (what
    plot_histogram draws); time_steps [T]; between [T], the standard deviation over the embeddings of `mean`: zero for a
    schedule that does not look at its input."""
    from . import ops
    emb, t = _schedule_inputs(experiment, embeddings, time_steps)
    if not 1 <= int(bins) <= 256:
        raise ValueError(f"bins lies in 1..256, got {bins}")
    cfg = experiment.model.config
    stats, hist = [], []
    for _, a, b, c in _schedule_chunks(experiment, emb, t.numel() * (8 + int(bins)) * 4):
        _, s, h = ops.schedule_curves(a, b, c, t, cfg.gamma_min, cfg.gamma_max, curves=False, stats=True, bins=int(bins))
        stats.append(s.cpu().numpy())
        hist.append(h.cpu().numpy())
    s = np.concatenate(stats)
    return dict(mean=s[..., 0], std=s[..., 1], min=s[..., 2], max=s[..., 3], channel_mean=s[..., 4:7],
                sigma2_mean=s[..., 7], hist=np.concatenate(hist), time_steps=t.cpu().numpy(),
                between=s[..., 0].astype(np.float64).std(axis=0))


def get_embedding(batch_size=2, latent_size=50, shift=0):
    """notebook_utils.get_embedding (:582-586): 15 ones then zeros, rolled by `shift`; fp32 [batch_size, latent_size]"""
    emb = torch.zeros((batch_size, latent_size), dtype=torch.float32)
    emb[:, :15] = 1.0
    return torch.roll(emb, shifts=shift, dims=1)


def heat_map_panels(schedule, cols=10, crop=2):
    """The data of notebook_utils.plot_heat_map (:630-651) for one schedule [T, 3072]: fp [cols, 32 - 2 crop,
    32 - 2 crop]; panel k is the row int(T k / cols) as a (32, 32, 3) image, cropped, min-max normalised (a constant
    panel: zeros) and turned to luminance with the Rec. 709 weights of skimage.color.rgb2gray"""
    ns = np.asarray(schedule, dtype=np.float64)
    if ns.ndim != 2 or ns.shape[1] != 3072 or cols < 1 or not 0 <= crop < 16:
        raise ValueError(f"a schedule is [T, 3072], cols >= 1, 0 <= crop < 16; got {list(ns.shape)}, {cols}, {crop}")
    panels = np.zeros((cols, 32 - 2 * crop, 32 - 2 * crop))
    for k in range(cols):
        p = ns[int(ns.shape[0] * k / cols)].reshape(32, 32, 3)[crop:32 - crop, crop:32 - crop]
        span = p.max() - p.min()
        if span > 0:
            panels[k] = ((p - p.min()) / span) @ np.asarray(REC709)
    return panels


class Clustering:
    """notebook_utils.Clustering (:669-695) without the drawing: embeddings whose dot product exceeds `threshold` times
    the largest one belong together"""

    def __init__(self, images, embeddings, threshold=0.8):
        self.images = images
        emb = embeddings.detach().cpu().numpy() if torch.is_tensor(embeddings) else np.asarray(embeddings)
        self.dotp = emb.astype(np.float64) @ emb.astype(np.float64).T
        self.threshold = threshold * np.max(self.dotp)

    def clusters(self, cluster_count=20, cluster_size_max=10):
        """a list of index lists: for each of the first `cluster_count` embeddings i that have a neighbour, i and then
        its neighbours in index order, `cluster_size_max` entries at the most (print_clusters' rule)"""
        near = self.dotp > self.threshold
        out = []
        for i in np.where(near.sum(axis=0) > 1)[0][:cluster_count]:
            cluster = [int(i)]
            for j in np.where(near[i])[0]:
                if j == i:
                    continue
                cluster.append(int(j))
                if len(cluster) == cluster_size_max:
                    break
            out.append(cluster)
        return out


def _time_ticks(plt, T):
    plt.xticks((np.linspace(0, 1, 10) * T).astype(int), ['{:.1f}'.format(i) for i in np.linspace(0, 1, 10)])
    plt.ylabel(r'$\gamma(t)$')
    plt.xlabel('$t$')


def plot_noise_schedule(noise_schedules, epoch=''):
    """notebook_utils.plot_noise_schedule (:571-579): every sub-pixel's curve of the first schedule"""
    import matplotlib.pyplot as plt
    fig = plt.figure()
    plt.plot(noise_schedules[0])
    plt.title(f'Noise Schedule per pixel for an input epoch:{epoch}')
    _time_ticks(plt, len(noise_schedules[0]))
    return fig


def plot_heat_map(noise_schedules, count=3, cols=10):
    """notebook_utils.plot_heat_map (:630-651): heat_map_panels of the first `count` schedules"""
    import matplotlib.pyplot as plt
    figs = []
    for ns in noise_schedules[:count]:
        fig = plt.figure(figsize=(6, 6))
        for k, panel in enumerate(heat_map_panels(ns, cols)):
            fig.add_subplot(1, cols, k + 1)
            plt.imshow(panel, cmap='hot', interpolation='nearest')
            plt.title('t={:.1f}'.format(k / cols), fontsize=8)
            plt.xticks([], [])
            plt.yticks([], [])
        figs.append(fig)
    return figs


def plot_histogram(hist, count=3, cols=5):
    """notebook_utils.plot_histogram (:655-666) from noise_schedule_summary's `hist` [E, T, bins] (or the summary itself):
    for the first `count` embeddings, the histogram at the rows int(T k / cols)"""
    import matplotlib.pyplot as plt
    hist = np.asarray(hist['hist'] if isinstance(hist, dict) else hist)
    figs = []
    for h in hist[:count]:
        fig = plt.figure(figsize=(cols, 1))
        for k in range(cols):
            fig.add_subplot(1, cols, k + 1)
            plt.bar(np.arange(h.shape[1]), h[int(h.shape[0] * k / cols)], width=1.0)
            plt.xticks([])
            plt.yticks([])
        figs.append(fig)
    return figs


# ------------------------------------------------------------------ the bound taken apart (not in the reference)
BITS = 1.0 / float(np.log(2.0))


def bound_profile(experiment, images, n_timesteps=128, eval_step0=0):
    """Where the bits of the dense evaluator's bound come from: each uint8 image of `images` [N, 32, 32, 3] is tiled
    n_timesteps = T times under PRNGKey(0) with same_image=True inside _packed_weights, exactly as _dense_partial scores
    it (image n at step eval_step0 + n, labels 0), and the pass's loss heads are reduced per row and per sub-pixel on the
    device (ops.bound_profile through the models' profile_rows).  A dict of numpy arrays, in bits per dimension (divided
    by 3072 ln 2) unless stated:
      t [N, T] the antithetic times of the rows;  diff [N, T] the diffusion integrand, diff_channel [N, T, 3] its three
      channel parts;  recon, klz [N, T] the reconstruction and prior-KL terms;  kl_z [N] the latent KL;  resid2, weight
      [N, T] the raw sum of squared residuals and mean loss weight of each row;  diff_pixel, recon_pixel, klz_pixel
      [N, 3072] the row means per sub-pixel, in bits (diff_pixel.sum(1) / 3072 == diff.mean(1));  bpd [N] = recon + klz +
      kl_z + diff as row means, what loss_fn returns for the image;  diff_std [N] the population standard deviation of
      diff over the rows.
    model_vdm.VDM (no per-pixel schedule) is accepted: the baseline to compare with.  One rank only."""
    if getattr(experiment, "world", 1) > 1:
        raise ValueError(f"bound_profile runs on one rank, this experiment has world = {experiment.world}: evaluate a "
                         "slice of the images per process instead")
    images = torch.as_tensor(images)
    if images.dtype != torch.uint8 or images.dim() != 4 or tuple(images.shape[1:]) != (32, 32, 3) or images.shape[0] < 1:
        raise ValueError(f"images are uint8 [N, 32, 32, 3] with N >= 1, got {images.dtype} {list(images.shape)}")
    T = int(n_timesteps)
    if T < 1:
        raise ValueError(f"n_timesteps must be >= 1, got {n_timesteps}")
    dev = experiment.device
    _, sample_rng = PRNGKey(0).split()                    # loss_fn's split of the evaluators' key
    same = {'same_image': True} if hasattr(experiment.model, "parameterization") else {}
    labels = torch.zeros(T, dtype=torch.int32, device=dev)
    conditioning = torch.zeros(T, dtype=torch.uint8, device=dev)
    per_image = []
    with _packed_weights(experiment):
        for n in range(images.shape[0]):
            tiled = images[n:n + 1].to(dev).expand(T, 32, 32, 3).contiguous()
            with torch.no_grad():
                _, prof = experiment.state.apply_fn(experiment.orig_params, tiled, labels, conditioning,
                                                    step=eval_step0 + n, rngs={'sample': sample_rng}, deterministic=True,
                                                    profile_rows=T, **same)
            per_image.append({k: prof[k].detach().double().cpu().numpy() for k in ("rows", "cols", "kl_z", "t")})
    return _profile_arrays(per_image)


def _profile_arrays(per_image):
    """the host arithmetic of bound_profile: per image rows [T, 8], cols [1, 3, 3072], kl_z [T], t [T] as float64"""
    per_dim = BITS / 3072.0
    rows = np.stack([p["rows"] for p in per_image])                          # [N, T, 8]
    cols = np.stack([p["cols"][0] for p in per_image])                       # [N, 3, 3072]
    out = dict(t=np.stack([p["t"] for p in per_image]).astype(np.float32),
               diff=rows[..., 0] * per_dim, diff_channel=rows[..., 1:4] * per_dim, recon=rows[..., 4] * per_dim,
               klz=rows[..., 5] * per_dim, kl_z=np.stack([p["kl_z"].mean() for p in per_image]) * per_dim,
               resid2=rows[..., 6], weight=rows[..., 7],
               diff_pixel=cols[:, 0] * BITS, recon_pixel=cols[:, 1] * BITS, klz_pixel=cols[:, 2] * BITS)
    out["bpd"] = out["recon"].mean(1) + out["klz"].mean(1) + out["kl_z"] + out["diff"].mean(1)
    out["diff_std"] = out["diff"].std(1)
    return out


def plot_bound_profile(profile, count=3):
    """for the first `count` images of a bound_profile: the diffusion integrand over t (the whole and its three
    channels) and the 32 x 32 maps of diff_pixel per channel"""
    import matplotlib.pyplot as plt
    figs = []
    for n in range(min(count, len(profile["bpd"]))):
        order = np.argsort(profile["t"][n])
        t = profile["t"][n][order]
        fig = plt.figure(figsize=(12, 3))
        ax = fig.add_subplot(1, 4, 1)
        ax.plot(t, profile["diff"][n][order], color='k', label='all')
        for ch, colour in enumerate(('r', 'g', 'b')):
            ax.plot(t, profile["diff_channel"][n][order, ch], color=colour, label=f'channel {ch}')
        ax.set_xlabel('$t$')
        ax.set_ylabel('bits / dim')
        ax.set_title(f"bpd {profile['bpd'][n]:.3f}  std {profile['diff_std'][n]:.3f}", fontsize=8)
        ax.legend(fontsize=6)
        maps = np.asarray(profile["diff_pixel"][n]).reshape(32, 32, 3)
        for ch in range(3):
            ax = fig.add_subplot(1, 4, 2 + ch)
            ax.imshow(maps[..., ch], cmap='hot', interpolation='nearest', vmin=0.0, vmax=float(maps.max()))
            ax.set_title(f'diffusion bits, channel {ch}', fontsize=8)
            ax.set_xticks([])
            ax.set_yticks([])
        figs.append(fig)
    return figs
