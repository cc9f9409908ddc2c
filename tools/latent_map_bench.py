"""Exact t-SNE on the device (tsne.hip) beside two baselines, by HIP events, alternated, medians (the timing of DESIGN 3.12).

python tools/latent_map_bench.py [--n 3840 --rounds 7 --inner 400 --perplexity 30 --sklearn_iters 250 --sklearn 0|1|2]

For D = 50 (the encoder's logits) and D = 3072 (a gamma map): mulan_tsne_affinities once per window, and one iteration
(mulan_tsne_gradient + mulan_tsne_update through ops.tsne_step, without and with the divergence) beside the same
iteration written with dense torch ops on the same device (torch.cdist, the elementwise products, row sums; it has to
materialise five N x N arrays).  Prints one JSON line: seconds per call of each (median, min, max of the windows' means),
the device-to-device copy rate measured here on 1 GiB (bytes read plus bytes written over the time), the share of that
rate the pass over P reaches (4 N^2 bytes at that rate over the iteration's time; P at N = 3840 is 59 MB and stays in the
Infinity Cache between iterations, so the share can exceed 1), the largest difference between the two formulations'
gradients, and -- where sklearn imports -- the host's seconds per iteration of sklearn.manifold.TSNE, method 'exact'
and 'barnes_hut', from one fit of --sklearn_iters iterations each at D = 50 (the affinities are not separable from a fit:
the figure is the whole fit over its iterations).  --sklearn 0 leaves the host baseline out, 2 runs it alone, on a set
drawn on the host, and touches no device.  No time is a pass / fail condition."""
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from mulan_amd import ops  # noqa: E402


def arg(name, default):
    return type(default)(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


def torch_step(P, Y, U, G, exaggeration, momentum, lr):
    """the iteration of ops.tsne_step with dense torch ops, in place on Y, U, G; returns the gradient"""
    d2 = torch.cdist(Y, Y, compute_mode='donot_use_mm_for_euclid_dist').square_()
    w = 1.0 / (1.0 + d2)
    w.fill_diagonal_(0.0)
    Z = w.sum(dtype=torch.float64)
    pw, w2 = P * w, w * w
    a = pw.sum(1, keepdim=True) * Y - pw @ Y
    r = w2.sum(1, keepdim=True) * Y - w2 @ Y
    grad = 4.0 * (exaggeration * a - r / Z.float())
    inc = U * grad < 0
    G.copy_(torch.where(inc, G + 0.2, G * 0.8).clamp_(min=0.01))
    U.mul_(momentum).sub_(lr * G * grad)
    Y.add_(U)
    return grad


def window(fn, inner):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(inner):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e-3 / inner


def stats(ts):
    return dict(median=statistics.median(ts), min=min(ts), max=max(ts))


def sklearn_seconds_per_iteration(x, perplexity, iters):
    try:
        from sklearn.manifold import TSNE
    except ImportError:
        return None
    out = {}
    for method in ("exact", "barnes_hut"):
        kw = dict(n_components=2, perplexity=perplexity, method=method, init="pca", random_state=0)
        try:
            model = TSNE(max_iter=iters, **kw)
        except TypeError:                                          # before 1.5 the argument was n_iter
            model = TSNE(n_iter=iters, **kw)
        t0 = time.perf_counter()
        model.fit_transform(x)
        out[method] = dict(fit_s=time.perf_counter() - t0, iterations=int(model.n_iter_),
                           s_per_iteration=(time.perf_counter() - t0) / max(1, int(model.n_iter_)), kl=float(model.kl_divergence_))
    return out


def main():
    N, rounds, inner = arg("--n", 3840), arg("--rounds", 7), arg("--inner", 400)
    perplexity, sk_iters, with_sklearn = arg("--perplexity", 30.0), arg("--sklearn_iters", 250), arg("--sklearn", 1)
    lr = max(N / 48.0, 50.0)
    if with_sklearn == 2:                                          # the host baseline alone: no device is touched
        rng = np.random.default_rng(50)
        x = (rng.standard_normal((16, 50))[np.arange(N) % 16] + 0.5 * rng.standard_normal((N, 50))).astype(np.float32)
        print(json.dumps(dict(N=N, D=50, perplexity=perplexity, sklearn_host=sklearn_seconds_per_iteration(x, perplexity, sk_iters))))
        return
    src = torch.empty(1 << 28, dtype=torch.float32, device="cuda").normal_()     # 1 GiB: beyond the Infinity Cache
    dst = torch.empty_like(src)
    run_copy = lambda: dst.copy_(src)                             # noqa: E731
    res = dict(N=N, rounds=rounds, inner=inner, perplexity=perplexity, P_bytes=4 * N * N)
    t_copy = []
    for D in (50, 3072):
        g = torch.Generator(device="cuda").manual_seed(D)
        centres = torch.randn((16, D), device="cuda", generator=g)
        x = (centres[torch.arange(N, device="cuda") % 16] + 0.5 * torch.randn((N, D), device="cuda", generator=g)).contiguous()
        P = ops.tsne_affinities(x, perplexity)
        Y0 = 1e-4 * torch.randn((N, 2), device="cuda", generator=g)
        U, G = torch.zeros_like(Y0), torch.ones_like(Y0)
        for _ in range(100):                                       # a map in mid-exaggeration, not the 1e-4 blob
            ops.tsne_step(P, Y0, U, G, 12.0, 0.5, lr)
        state = lambda: (Y0.clone(), U.clone(), G.clone())         # noqa: E731
        Yh, Uh, Gh = state()
        Yt, Ut, Gt = state()
        gh = ops.tsne_gradient(P, Yh, 12.0)[0]
        gt = torch_step(P, Yt, Ut, Gt, 12.0, 0.5, lr)
        Yt, Ut, Gt = state()
        run_copy()
        torch.cuda.synchronize()
        diff = dict(grad=float((gh - gt).abs().max()), grad_scale=float(gt.abs().max()))
        run_aff = lambda: ops.tsne_affinities(x, perplexity)       # noqa: E731
        run_hip = lambda: ops.tsne_step(P, Yh, Uh, Gh, 12.0, 0.5, lr)             # noqa: E731
        run_hip_kl = lambda: ops.tsne_step(P, Yh, Uh, Gh, 12.0, 0.5, lr, kl=True)  # noqa: E731
        run_torch = lambda: torch_step(P, Yt, Ut, Gt, 12.0, 0.5, lr)              # noqa: E731
        t_aff, t_hip, t_kl, t_torch = [], [], [], []
        for _ in range(rounds):
            t_aff.append(window(run_aff, max(1, inner // 10)))
            t_hip.append(window(run_hip, inner))
            t_kl.append(window(run_hip_kl, inner))
            t_torch.append(window(run_torch, max(1, inner // 4)))
            t_copy.append(window(run_copy, 4))
        entry = dict(affinities_s=stats(t_aff), iteration_s=stats(t_hip), iteration_with_kl_s=stats(t_kl),
                     torch_iteration_s=stats(t_torch), max_abs_difference=diff)
        if with_sklearn and D == 50:
            entry["sklearn_host"] = sklearn_seconds_per_iteration(x.cpu().numpy(), perplexity, sk_iters)
        res[f"D{D}"] = entry
    copy_rate = 2.0 * src.numel() * 4 / statistics.median(t_copy)
    res["copy_bytes_per_s"] = copy_rate
    for D in (50, 3072):
        res[f"D{D}"]["share_of_copy_rate"] = 4.0 * N * N / copy_rate / res[f"D{D}"]["iteration_s"]["median"]
    print(json.dumps(res))


if __name__ == "__main__":
    np.seterr(all="ignore")
    main()
