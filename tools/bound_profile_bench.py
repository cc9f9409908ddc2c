"""Seconds per image of evaluators.bound_profile beside eval_bpd_dense_sampling on the same images (the timing pair of
DESIGN §3.9): the shipped CIFAR-10 configuration at its full depth, random parameters, --images random images in an npz,
--timesteps copies of each.  Both score every image with the same launches up to the loss heads; the profile adds one
mulan_bound_profile (and its fold) per image and copies [T, 8] + [3, 3072] words to the host instead of one float.
Three alternated rounds of each, one warm-up call ahead; the medians and the spread are printed as one JSON line.  Also
the kernel alone at B = --timesteps rows, by HIP events.

  python tools/bound_profile_bench.py [--images 8] [--timesteps 128]"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=8)
    ap.add_argument("--timesteps", type=int, default=128)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bound_profile_bench needs the GPU: a CPU run says nothing about these times")
    from mulan_amd import evaluators as ev
    from mulan_amd import ops
    from mulan_amd.config import load_config_file
    from mulan_amd.experiment import Experiment_VDM
    N, T = args.images, args.timesteps
    images = np.random.default_rng(0).integers(0, 256, (N, 32, 32, 3)).astype(np.uint8)
    with tempfile.TemporaryDirectory() as tmp:
        np.savez(os.path.join(tmp, "val.npz"), images=images)
        config = load_config_file(os.path.join(ROOT, "ldm", "configs", "cifar10-conditioned.py"))
        config.data.dataset = f"npz:{os.path.join(tmp, 'val.npz')}"
        config.training.batch_size_train = config.training.batch_size_eval = 2
        exp = Experiment_VDM(config)
        exp.orig_params = exp.state.ema_params

        def dense():
            return ev.eval_bpd_dense_sampling(exp, config, n_timesteps=T, max_images=N)

        def profile():
            return ev.bound_profile(exp, torch.from_numpy(images), n_timesteps=T)

        def timed(fn):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = fn()
            torch.cuda.synchronize()
            return time.perf_counter() - t0, out
        bpd, prof = dense(), profile()                   # warm-up: every kernel configured, the allocator warm
        r = {"dense": [], "profile": []}
        for _ in range(3):
            r["dense"].append(timed(dense)[0] / N)
            r["profile"].append(timed(profile)[0] / N)
    # the kernel alone: the loss heads of T rows, per-element gammas
    g = torch.Generator(device="cuda").manual_seed(0)
    rnd = lambda: torch.randn((T, 3072), device="cuda", generator=g)
    x = torch.randint(0, 256, (T, 3072), device="cuda", dtype=torch.uint8, generator=g)
    # gamma_0 near -13.3 (the narrow bin window of a trained schedule), gamma_1 near 5, gamma_t across the range
    a = [-13.3 + 0.1 * rnd().abs(), 5.0 - 0.1 * rnd().abs(), -13.3 + 18.3 * torch.rand((T, 3072), device="cuda", generator=g),
         rnd().abs() * 10] + [rnd() for _ in range(4)]
    ops.bound_profile(1, x, *a, T)
    times = []
    for _ in range(20):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        ops.bound_profile(1, x, *a, T)
        e.record()
        e.synchronize()
        times.append(s.elapsed_time(e))
    print(json.dumps(dict(images=N, timesteps=T, dense_bpd=bpd, profile_bpd=float(prof["bpd"].mean()),
                          dense_s_per_image=float(np.median(r["dense"])), profile_s_per_image=float(np.median(r["profile"])),
                          spread={k: [min(v), max(v)] for k, v in r.items()},
                          kernel_ms=float(np.median(times)), kernel_bytes_read=T * 3072 * (8 * 4 + 1))))


if __name__ == "__main__":
    main()
