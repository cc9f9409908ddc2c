"""Times the noise-schedule analysis at the size of the reference's own use (get_logits over 30 batches of 128:
E = 3840 embeddings, T = 128 times) on one MI355X, three ways, alternated within one run:

  summary   ops.schedule_curves(curves=False, stats=True, bins=100) over all E: E T (8 + bins) words written
  curves    ops.schedule_curves() in chunks of evaluators.SCHEDULE_BUFFER_BYTES, each chunk copied to the host
            (what noise_schedule_per_embedding does after the coefficient MLP)
  loop      the way without the kernel: per embedding, NoiseSchedule_polynomial_fixedend.apply on the embedding repeated
            T times (the coefficient MLP on T identical rows, one launch with one t per row), then [T, 3072] to the host;
            timed over --loop_embeddings embeddings and scaled to E

The coefficient MLP of `summary` and `curves` (poly_coefficients on [E, 50], once) is timed on its own and added to both.
Random parameters of the CIFAR-10 model size; the times do not depend on the values.  Prints one JSON line.

  python tools/schedule_curves_bench.py [--embeddings 3840] [--timesteps 128] [--bins 100] [--repeats 5]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def timed(fn, repeats):
    """median wall time of fn() in seconds, each call ending in a device synchronise; one call ahead to warm up"""
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append(time.perf_counter() - t0)
    return float(np.median(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--embeddings", type=int, default=3840)
    ap.add_argument("--timesteps", type=int, default=128)
    ap.add_argument("--bins", type=int, default=100)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--loop_embeddings", type=int, default=64)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("schedule_curves_bench needs the GPU: a CPU run says nothing about these times")
    from mulan_amd import evaluators as ev
    from mulan_amd import model as M
    from mulan_amd import ops
    from mulan_amd.rng import PRNGKey
    E, T = args.embeddings, args.timesteps
    cfg = M.VDMConfig(vocab_size=256, sample_softmax=False, antithetic_time_sampling=True, with_fourier_features=True,
                      with_attention=False, gamma_type='poly_fixedend', gamma_min=-13.3, gamma_max=5.0, sm_n_timesteps=0,
                      sm_n_embd=128, sm_n_layer=1, sm_pdrop=0.1, forward_n_layer=1, latent_size=50, latent_k=15,
                      encoder='unet', latent_type='topk', z_conditioning=True, reparam_type='true', unet_type='vdm',
                      velocity_from_epsilon=False, condition='input', sigma_type='no_blur', sigma_prior=1.0)
    vdm = M.make_vdm('mulan_velocity', cfg)
    params = M.tree_map(lambda x: x.cuda(), vdm.init(PRNGKey(0)))["gamma"]
    emb = ops.topk_hard(PRNGKey(1).normal((E, 50), torch.device("cuda")), 15)[0]
    t = torch.linspace(0.0, 1.0, T, device="cuda")
    schedule = M.NoiseSchedule_polynomial_fixedend(cfg)
    per_launch = max(1, ev.SCHEDULE_BUFFER_BYTES // (T * 3072 * 4))

    with torch.no_grad():
        a, b, c = M.poly_coefficients(params, emb)

        def coefficients():
            M.poly_coefficients(params, emb)

        def summary():
            _, s, h = ops.schedule_curves(a, b, c, t, cfg.gamma_min, cfg.gamma_max, curves=False, stats=True,
                                          bins=args.bins)
            s.cpu(), h.cpu()

        def curves_device():
            for i in range(0, E, per_launch):
                ops.schedule_curves(a[i:i + per_launch], b[i:i + per_launch], c[i:i + per_launch], t, cfg.gamma_min,
                                    cfg.gamma_max)

        def curves():
            for i in range(0, E, per_launch):
                ops.schedule_curves(a[i:i + per_launch], b[i:i + per_launch], c[i:i + per_launch], t, cfg.gamma_min,
                                    cfg.gamma_max)[0].cpu()

        def loop():
            for i in range(args.loop_embeddings):
                schedule.apply(params, emb[i:i + 1].expand(T, 50).contiguous(), t).cpu()

        r = {k: [] for k in ("coefficients", "summary", "curves_device", "curves", "loop")}
        for _ in range(3):                              # alternated: three rounds of each, the median of the rounds
            for k, fn in (("coefficients", coefficients), ("summary", summary), ("curves_device", curves_device),
                          ("curves", curves), ("loop", loop)):
                r[k].append(timed(fn, args.repeats))
    med = {k: float(np.median(v)) for k, v in r.items()}
    out = dict(embeddings=E, timesteps=T, bins=args.bins, embeddings_per_launch=per_launch,
               coefficients_ms=1e3 * med["coefficients"],
               summary_ms=1e3 * (med["summary"] + med["coefficients"]),
               curves_device_only_ms=1e3 * (med["curves_device"] + med["coefficients"]),
               curves_ms=1e3 * (med["curves"] + med["coefficients"]),
               loop_ms=1e3 * med["loop"] * E / args.loop_embeddings, loop_embeddings_timed=args.loop_embeddings,
               curve_bytes=E * T * 3072 * 4, spread={k: [1e3 * min(v), 1e3 * max(v)] for k, v in r.items()})
    print(json.dumps(out))


if __name__ == "__main__":
    main()
