"""What does the latent space look like?  The reference's views of the latents the encoder assigns to images
(ldm/notebook_utils.py:713-753: plot_tsne_transformation, pca_transformation, animate_scatter; there on sklearn, five
host fits of N = 3840 points) with exact t-SNE on the device (ops.tsne_affinities / ops.tsne_step, tsne.hip) and PCA as
a float64 SVD on the host; `latent_map` (not in the reference) builds the map of a checkpoint.

`tsne` follows sklearn.manifold.TSNE(2, method='exact') at its defaults from version 1.2 on (PCA init scaled to a
standard deviation of 1e-4, learning rate max(N / 48, 50) with early exaggeration 12, 250 exaggerated iterations at
momentum 0.5 and the rest at 0.8) with one stated deviation: the iteration count is fixed and the Kullback-Leibler
divergence is recorded on the device every `record_every` iterations, where sklearn stops on min_grad_norm /
n_iter_without_progress, which would need a host read every 50 steps.  The divergence reported is that of P itself (not of
the exaggerated P, which sklearn reports while it exaggerates)."""
import numpy as np
import torch

from . import ops

INIT_STD = 1e-4
KNN_K = 10


# ------------------------------------------------------------------------------------------------ PCA (host, float64)
def _matrix(data, name, min_rows=2):
    """array or tensor [N, D] of real numbers -> float64 numpy [N, D]"""
    if torch.is_tensor(data):
        data = data.detach().cpu().numpy()
    if not isinstance(data, np.ndarray) or data.ndim != 2 or data.dtype.kind not in "fiu" or data.shape[0] < min_rows \
            or data.shape[1] < 1:
        raise ValueError(f"{name}: data is a real array [N >= {min_rows}, D >= 1], got "
                         f"{(data.dtype, data.shape) if isinstance(data, np.ndarray) else type(data).__name__}")
    data = data.astype(np.float64)
    if not np.isfinite(data).all():
        raise ValueError(f"{name}: data holds a value that is not finite")
    return data


def _pca(data, flip="v"):
    """(scores [N, R], singular values [R], variance ratio [R]) of centred float64 data, R = min(N, D); the sign of every
    component by sklearn's svd_flip: 'v' makes the component's largest loading positive (PCA from sklearn 1.5 on), 'u'
    the largest score (before)"""
    u, s, vt = np.linalg.svd(data - data.mean(axis=0), full_matrices=False)
    if flip == "v":
        sign = np.sign(vt[np.arange(vt.shape[0]), np.abs(vt).argmax(axis=1)])
    elif flip == "u":
        sign = np.sign(u[np.abs(u).argmax(axis=0), np.arange(u.shape[1])])
    else:
        raise ValueError(f"pca: flip is 'v' or 'u', got {flip!r}")
    sign[sign == 0] = 1.0
    var = s * s / (data.shape[0] - 1)
    total = var.sum()
    return u * sign * s, s, var / total if total > 0 else np.zeros_like(var)


def pca_transformation(data, n_components=4, return_stats=False, flip="v"):
    """notebook_utils.pca_transformation (:722-727), PCA(n_components, svd_solver='full'): prints the variance ratios and
    the singular values as the reference does and returns the projection, float64 [N, n_components]; return_stats:
    (projection, variance ratio, singular values)."""
    x = _matrix(data, "pca_transformation")
    if isinstance(n_components, bool) or not isinstance(n_components, (int, np.integer)) \
            or not 1 <= n_components <= min(x.shape):
        raise ValueError(f"pca_transformation: n_components is an int in [1, {min(x.shape)}], got {n_components!r}")
    scores, s, ratio = _pca(x, flip)
    ratio, s = ratio[:n_components], s[:n_components]
    print('variance ratio', ratio)
    print('singular values', s)
    out = scores[:, :n_components]
    return (out, ratio, s) if return_stats else out


def pca_init(data, flip="v"):
    """fp32 [N, 2]: the first two principal components divided by the standard deviation of the first, times 1e-4 (sklearn's
    init='pca' from 1.2 on); a second column of zeros for D = 1"""
    scores = _pca(_matrix(data, "tsne"), flip)[0]
    y = np.zeros((scores.shape[0], 2))
    y[:, :min(2, scores.shape[1])] = scores[:, :2]
    sd = y[:, 0].std()
    if not sd > 0:
        raise ValueError("tsne: init='pca' needs data that varies (every row is the same)")
    return (y / sd * INIT_STD).astype(np.float32)


# ------------------------------------------------------------------------------------------------ t-SNE (device)
def _int(name, v, lo):
    if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v < lo:
        raise ValueError(f"tsne: {name} is an int >= {lo}, got {v!r}")
    return int(v)


def tsne_check(data, perplexity=30.0, n_iter=1000, exaggeration_iter=250, early_exaggeration=12.0, learning_rate='auto',
               init='pca', seed=0, record_every=50):
    """every check of tsne that touches neither the library nor a device -> (N, D, learning rate)"""
    if not (isinstance(data, np.ndarray) or torch.is_tensor(data)) or len(data.shape) != 2 or \
            str(data.dtype).replace("torch.", "") not in ("float32", "float64"):
        raise ValueError(f"tsne: data is a float32 or float64 array or tensor [N, D], got "
                         f"{(data.dtype, tuple(data.shape)) if hasattr(data, 'dtype') else type(data).__name__}")
    N, D = data.shape
    if not ops.TSNE_MIN_N <= N <= ops.TSNE_MAX_N or D < 1:
        raise ValueError(f"tsne: {ops.TSNE_MIN_N} <= N <= {ops.TSNE_MAX_N} points of D >= 1 (P is dense), got {N} x {D}")
    ops._tsne_number("perplexity", perplexity, lo=1, hi=N - 1)
    _int("n_iter", n_iter, 1)
    _int("exaggeration_iter", exaggeration_iter, 0)          # beyond n_iter: every iteration is exaggerated, as in sklearn
    ops._tsne_number("early_exaggeration", early_exaggeration, lo=0, lo_open=True)
    _int("seed", seed, 0)
    _int("record_every", record_every, 1)
    if isinstance(learning_rate, str):
        if learning_rate != 'auto':
            raise ValueError(f"tsne: learning_rate is 'auto' or a positive number, got {learning_rate!r}")
        lr = max(N / 48.0, 50.0)
    else:
        lr = ops._tsne_number("learning_rate", learning_rate, lo=0, lo_open=True)
    if isinstance(init, str):
        if init not in ('pca', 'random'):
            raise ValueError(f"tsne: init is 'pca', 'random' or an array [N, 2], got {init!r}")
    elif not (isinstance(init, np.ndarray) or torch.is_tensor(init)) or tuple(init.shape) != (N, 2):
        raise ValueError(f"tsne: init is 'pca', 'random' or an array [{N}, 2]")
    return N, D, lr


def tsne(data, perplexity=30.0, n_iter=1000, exaggeration_iter=250, early_exaggeration=12.0, learning_rate='auto',
         init='pca', seed=0, record_every=50, device=None):
    """Exact t-SNE of the rows of data [N, D] (4 <= N <= 16384) into the plane, on the device.  A dict:
      Y [N, 2]      the map, fp32
      kl, kl_iter   the Kullback-Leibler divergence of the map before iteration 0, record_every, 2 record_every, ... and of
                    the final map (kl_iter ends with n_iter), float64; read from the device once, at the end
      beta [N]      the precisions the perplexity search found
      settings      every argument, with the learning rate that was used
    learning_rate 'auto' is max(N / 48, 50); init 'pca' is pca_init, 'random' 1e-4 x normals of mulan_amd.rng under `seed`,
    or an array [N, 2].  The same call gives the same bits."""
    N, D, lr = tsne_check(data, perplexity, n_iter, exaggeration_iter, early_exaggeration, learning_rate, init, seed,
                          record_every)
    if device is None:
        device = data.device if torch.is_tensor(data) and data.is_cuda else torch.device("cuda", torch.cuda.current_device())
    x = (data if torch.is_tensor(data) else torch.tensor(data)).to(device=device, dtype=torch.float32).contiguous()
    if isinstance(init, str) and init == 'pca':
        Y = torch.from_numpy(pca_init(data)).to(device)
    elif isinstance(init, str):
        from .rng import PRNGKey
        Y = (INIT_STD * PRNGKey(seed).normal((N, 2), device)).contiguous()
    else:
        Y = (init if torch.is_tensor(init) else torch.tensor(init)).to(device=device, dtype=torch.float32).clone().contiguous()
    P, beta = ops.tsne_affinities(x, perplexity, symmetrise=True, return_beta=True)
    U, G = torch.zeros_like(Y), torch.ones_like(Y)
    kl_iter = list(range(0, n_iter, record_every)) + [n_iter]
    trace = torch.zeros(len(kl_iter), device=device, dtype=torch.float64)
    for it in range(n_iter):
        early = it < exaggeration_iter
        ops.tsne_step(P, Y, U, G, early_exaggeration if early else 1.0, 0.5 if early else 0.8, lr,
                      kl=trace[it // record_every] if it % record_every == 0 else False)
    ops.tsne_kl(P, Y, out=trace[len(kl_iter) - 1])
    settings = dict(N=N, D=D, perplexity=float(perplexity), n_iter=int(n_iter), exaggeration_iter=int(exaggeration_iter),
                    early_exaggeration=float(early_exaggeration), learning_rate=float(lr),
                    init=init if isinstance(init, str) else 'array', seed=int(seed), record_every=int(record_every))
    return dict(Y=Y.cpu().numpy(), kl=trace.cpu().numpy(), kl_iter=np.asarray(kl_iter), beta=beta.cpu().numpy(),
                settings=settings)


def plot_tsne_transformation(data, perplexities=range(5, 55, 10), colour=None, **tsne_kw):
    """notebook_utils.plot_tsne_transformation (:713-719): one figure per perplexity (the reference's 5, 15, ..., 45), the
    affinities recomputed for each; returns the list of (figure, result of tsne)"""
    perplexities = list(perplexities)
    for p in perplexities:
        tsne_check(data, perplexity=p, **tsne_kw)
    import matplotlib.pyplot as plt
    out = []
    for p in perplexities:
        res = tsne(data, perplexity=p, **tsne_kw)
        fig = plt.figure()
        plt.title(f'perplexity: {p}')
        plt.scatter(res["Y"][:, 0], res["Y"][:, 1], c=colour)
        out.append((fig, res))
    return out


def animate_scatter(xs, ys, cs, dpi=100.0):
    """notebook_utils.animate_scatter (:736-753): frame i scatters (xs[i], ys[i]) coloured by cs[i] > mean(cs[i]).  Returns
    the FuncAnimation (the reference displays it as HTML5 video; that is left to the caller)."""
    if not (len(xs) == len(ys) == len(cs)) or len(xs) < 1:
        raise ValueError(f"animate_scatter: xs, ys and cs hold one entry per frame, got {len(xs)}, {len(ys)}, {len(cs)}")
    import matplotlib.pyplot as plt
    from matplotlib import animation
    fig, ax = plt.subplots(dpi=dpi)

    def animate(i):
        ax.clear()
        ax.set_title(f'{3 * 10 * (i + 1)} k / 500k steps')
        ax.axis([-2, 2, -2, 2])
        ax.scatter(xs[i], ys[i], c=(np.asarray(cs[i]) > np.mean(cs[i])))

    return animation.FuncAnimation(fig, animate, frames=len(xs), interval=800, repeat_delay=1, repeat=True)


# ------------------------------------------------------------------------------------------------ a checkpoint's map
def parse_on(on):
    """-> ('logits' | 'embeddings', None) or ('schedule', t) or ValueError"""
    if on in ('logits', 'embeddings'):
        return on, None
    if isinstance(on, str) and on.startswith('schedule:'):
        try:
            t = float(on[9:])
        except ValueError:
            t = float('nan')
        if 0.0 <= t <= 1.0:
            return 'schedule', t
    raise ValueError(f"latent_map: on is 'logits', 'embeddings' or 'schedule:t' with t in [0, 1], got {on!r}")


def knn_agreement(x, y, k=KNN_K, chunk=2048):
    """The mean over the points of the share of a point's k nearest neighbours in y (the map) that are among its k nearest
    in x (the input space); fp32 device tensors [N, D] and [N, 2].  Distances from the differences, `chunk` rows at a time."""
    N = x.shape[0]
    if N <= k:
        raise ValueError(f"knn_agreement: more than k = {k} points are needed, got {N}")
    hits = 0
    for lo in range(0, N, chunk):
        own = torch.arange(lo, min(lo + chunk, N), device=x.device)
        near = []
        for v in (x, y):
            d = torch.cdist(v[lo:lo + chunk], v, compute_mode='donot_use_mm_for_euclid_dist')
            d[torch.arange(own.numel(), device=x.device), own] = float('inf')
            near.append(d.topk(k, dim=1, largest=False).indices)
        hits += int((near[0][:, :, None] == near[1][:, None, :]).any(dim=2).sum())
    return hits / float(N * k)


def latent_map(experiment, num_batches=30, on='logits', perplexity=30.0, **tsne_kw):
    """The map of a checkpoint's latent space: the encoder's logits over num_batches evaluation batches (get_logits), or
    their hard top-k embeddings, or (on='schedule:t') the gamma map at time t under each embedding, D = 3072, through
    `tsne`.  A dict: the keys of tsne, `colour` [N] (the mean gamma at t = 0.5 under each point's embedding,
    noise_schedule_summary), `knn_agreement` (the mean share of a point's 10 nearest map neighbours that are among its 10
    nearest in the input space), `on` and `points` [N, D] (what was mapped).  A model_vdm.VDM experiment (no latent) and several ranks are refused."""
    from . import evaluators as ev
    kind, t = parse_on(on)
    if not hasattr(experiment.model, "deterministic_embedding"):
        raise ValueError("latent_map needs a MuLAN model (model_vdm.VDM has one scalar schedule and no latent embedding)")
    if getattr(experiment, "world", 1) > 1:
        raise ValueError(f"latent_map runs in one process, the experiment spans {experiment.world} ranks")
    _int("num_batches", num_batches, 1)
    with torch.no_grad():
        logits, _ = ev.get_logits(experiment, num_batches)
        emb = ev.logits_to_embeddings(logits)
    if kind == 'logits':
        x = logits.float()
    elif kind == 'embeddings':
        x = emb.float()
    else:
        curves = ev.noise_schedule_per_embedding(experiment, emb, np.array([t], dtype=np.float32))
        x = torch.from_numpy(np.stack([c[0] for c in curves])).to(experiment.device)
    x = x.contiguous()
    tsne_check(x, perplexity=perplexity, **tsne_kw)
    res = tsne(x, perplexity=perplexity, device=experiment.device, **tsne_kw)
    summary = ev.noise_schedule_summary(experiment, emb, np.array([0.5], dtype=np.float32), bins=1)
    res["colour"] = summary["mean"][:, 0]
    res["knn_agreement"] = knn_agreement(x, torch.from_numpy(res["Y"]).to(experiment.device))
    res["on"] = on
    res["points"] = x.cpu().numpy()
    return res
