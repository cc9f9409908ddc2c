"""Wall time per batch of the samplers on one MI355X at the full CIFAR-10 configuration (random-init weights: the time
does not depend on them).  Forms, alternated within one run after one untimed warm-up pass of each:
  ancestral T = 1000 (replayed reverse step), ddim N = 50 (replayed), dpm2m N = 25 replayed, dpm2m N = 25 eager,
  sde2m N = 25 replayed (the stochastic step: one randn and one more read of the latent's size per step);
  with --inpaint also dpm2m N = 25 replayed under a half:left mask at resample 1 (25 network evaluations, one mix per
  step) and at resample 2 (49 evaluations, a jump and a mix more per repeated step);
  with --restore also dpm2m N = 25 replayed under an sr:4 measurement at resample 1 (25 evaluations, one projection per
  step);
  with --grid KIND also dpm2m N = 25 replayed on that time grid (logsnr | karras | quadratic; the first two add two
  small launches and one read of 24 floats per batch: ops.schedule_moments, ops.schedule_invert).
Each time is one batch from z_1 to the uint8 images (the loop plus generate_x) with the stepper built beforehand (what
`python -m ldm.sample` pays per batch), between two device synchronisations.  One JSON line per timed batch, then a
summary line (median ms per batch).

    python tools/fast_sampler_timing.py [--batch 64] [--rounds 3] [--few-step-only] [--inpaint] [--restore] [--grid logsnr]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--few-step-only", action="store_true", help="leave the 1000-step ancestral form out")
    ap.add_argument("--inpaint", action="store_true", help="add dpm2m with a mask at resample 1 and 2")
    ap.add_argument("--restore", action="store_true", help="add dpm2m with an sr:4 measurement at resample 1")
    ap.add_argument("--grid", default=None, help="add dpm2m on this time grid (logsnr, karras or quadratic)")
    args = ap.parse_args()
    import torch
    from mulan_amd.config import load_config_file
    from mulan_amd.experiment import Experiment_VDM
    from mulan_amd.rng import PRNGKey
    config = load_config_file(os.path.join(ROOT, "ldm", "configs", "cifar10-conditioned.py"))
    config.data.dataset = 'synthetic'
    config.training.batch_size_eval = args.batch
    exp = Experiment_VDM(config)
    model, params, B, dev = exp.model, exp.state.ema_params, args.batch, exp.device
    packer = exp.state.param_packer("ema")
    if packer is not None:
        packer.refresh()
    cond = torch.zeros(B, dtype=torch.uint8, device=dev)
    emb = model.deterministic_embedding(B, dev)
    ctx = model.fast_context(params, emb, cond)
    rng = PRNGKey(0)
    z1 = rng.normal((B, 3072), dev)
    T = 1000
    with torch.no_grad():
        ancestral = model.reverse_stepper(params, B, dev, emb, cond, ctx["coeffs"], T, graph=True)
        fast_replay = model.fast_stepper(params, B, dev, ctx, graph=True)
        fast_eager = model.fast_stepper(params, B, dev, ctx, graph=False)
        sde_replay = model.fast_stepper(params, B, dev, ctx, graph=True, step_eta=1.0)
    assert type(fast_replay).__name__ == "GraphedFastStep" and type(sde_replay).__name__ == "GraphedFastStep"
    assert type(getattr(ancestral, "__self__", None)).__name__ == "GraphedReverseStep"

    def run_ancestral():
        z = z1
        for i in range(T):
            z = ancestral(i, z, rng)
        return model.generate_x(params, z, ctx["coeffs"])

    def fast(sampler, N, stepper, noise=None):
        return lambda: model.generate_x(params, model.fast_sample(params, z1, ctx, sampler, N, stepper=stepper,
                                                                  noise=noise), ctx["coeffs"])

    forms = [("ancestral_T1000_replayed", run_ancestral), ("ddim_N50_replayed", fast("ddim", 50, fast_replay)),
             ("dpm2m_N25_replayed", fast("dpm2m", 25, fast_replay)), ("dpm2m_N25_eager", fast("dpm2m", 25, fast_eager)),
             ("sde2m_N25_replayed", fast("sde2m", 25, sde_replay, rng.fold_in(1)))]
    if args.inpaint:
        from mulan_amd import ops, sampling
        with torch.no_grad():
            mask_replay = model.fast_stepper(params, B, dev, ctx, graph=True, inpaint=True)
        assert type(mask_replay).__name__ == "GraphedFastStep"
        known = ops.encode_u8(torch.randint(0, 256, (B, 3072), dtype=torch.uint8, device=dev))
        mask = sampling.expand_mask(sampling.mask_from_spec("half:left"), B, dev)

        def inpaint(U):
            return lambda: model.generate_x(params, model.fast_sample(
                params, z1, ctx, "dpm2m", 25, stepper=mask_replay, known=known, mask=mask, resample=U,
                known_noise=rng.fold_in(2)), ctx["coeffs"])
        forms += [("dpm2m_N25_inpaint_resample1_replayed", inpaint(1)), ("dpm2m_N25_inpaint_resample2_replayed", inpaint(2))]
    if args.restore:
        from mulan_amd import ops
        with torch.no_grad():
            restore_replay = model.fast_stepper(params, B, dev, ctx, graph=True, restore="sr:4")
        assert type(restore_replay).__name__ == "GraphedFastStep"
        y = ops.restore_measure(ops.encode_u8(torch.randint(0, 256, (B, 32, 32, 3), dtype=torch.uint8, device=dev)), 4, False)
        forms += [("dpm2m_N25_restore_sr4_replayed", lambda: model.generate_x(params, model.fast_sample(
            params, z1, ctx, "dpm2m", 25, stepper=restore_replay, measurement=y, degradation="sr:4"), ctx["coeffs"]))]
    if args.grid is not None:
        forms += [(f"dpm2m_N25_{args.grid}_replayed", lambda: model.generate_x(params, model.fast_sample(
            params, z1, ctx, "dpm2m", 25, stepper=fast_replay, grid=args.grid), ctx["coeffs"]))]
    if args.few_step_only:
        forms = forms[1:]
    times = {name: [] for name, _ in forms}
    print(json.dumps({"tool": "tools/fast_sampler_timing.py", "batch": B, "rounds": args.rounds,
                      "few_step_only": args.few_step_only, "forms": [name for name, _ in forms]}), flush=True)
    with torch.no_grad():
        for name, fn in forms:                 # warm-up: one untimed batch of each form
            fn()
        torch.cuda.synchronize()
        for r in range(args.rounds):
            for name, fn in forms:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                x = fn()
                torch.cuda.synchronize()
                ms = (time.perf_counter() - t0) * 1e3
                times[name].append(ms)
                assert x.shape == (B, 32, 32, 3) and x.dtype == torch.uint8
                print(json.dumps({"round": r, "form": name, "batch": B, "ms_per_batch": round(ms, 2)}), flush=True)
    med = {k: round(statistics.median(v), 2) for k, v in times.items()}
    print(json.dumps({"summary": "median ms per batch", "batch": B, "rounds": args.rounds, **med,
                      **({} if args.few_step_only else {"ancestral_over_dpm2m_replayed": round(
                          med["ancestral_T1000_replayed"] / med["dpm2m_N25_replayed"], 1)}),
                      "sde2m_over_dpm2m_replayed": round(med["sde2m_N25_replayed"] / med["dpm2m_N25_replayed"], 4),
                      "device": torch.cuda.get_device_name(0)}), flush=True)
    if packer is not None:
        packer.invalidate()


if __name__ == "__main__":
    main()
