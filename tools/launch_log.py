#!/usr/bin/env python3
"""dev: the launch sequence of the eager paths, one line per call of a library entry point (its name and its non-pointer
arguments; pointers as `*`, NULL as `-`), at the configuration of __graft_entry__.smoke (E = 128, one layer, B = 4; fixed
seeds).  What the Python wiring in ops.py decides -- which kernel runs, with which by-product of the one before -- is
all in this sequence: a by-product lost on the way shows as an extra mulan_absmax_rows / mulan_colsum* /
mulan_groupnorm_stats / mulan_add_absmax_rows* line, one wrongly accepted as a missing line or a changed argument.
Record it before and after a change of that wiring and compare the two files (see profiles/README.md).
    python tools/launch_log.py --out launches.log
Paths: an eager train step with dropout, the same without the weight-gradient stream, an ancestral reverse step and two
fast-sampler steps (orders 1 and 2), an ODE function evaluation with the divergence term, a train step at B = 32 (inside
the GN_FWD_STREAM window)."""
import argparse
import collections
import ctypes
import os
import sys

for k in ("MULAN_HIP_GRAPH", "MULAN_SAMPLER_GRAPH", "MULAN_ODE_GRAPH"):
    os.environ[k] = "0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch

from mulan_amd import lib, ops, sampling
from mulan_amd import model as M
from mulan_amd.config import load_config_file
from mulan_amd.experiment import Experiment_VDM
from mulan_amd.rng import PRNGKey

LINES = []
_real = lib.call


def _logged(name, *args):
    out = []
    for a, ty in zip(args, lib.SIGNATURES[name]):
        if ty is ctypes.c_void_p:
            out.append("-" if a is None else "*")
        else:
            out.append(repr(float(a)) if ty in (ctypes.c_float, ctypes.c_double) else str(int(a)))
    LINES.append(name + " " + " ".join(out))
    return _real(name, *args)


def _wrap():
    for name, mod in list(sys.modules.items()):
        if name.startswith("mulan_amd") and getattr(mod, "call", None) is _real:
            mod.call = _logged


def _experiment(B):
    config = load_config_file(os.path.join(ROOT, "ldm", "configs", "cifar10-conditioned.py"))
    config.data.dataset = "synthetic"
    config.model.sm_n_layer = 1
    config.model.forward_n_layer = 1
    config.training.batch_size_train = B
    config.training.batch_size_eval = B
    config.training.substeps = 1
    config.training.hip_graph = False
    return Experiment_VDM(config)


def _batch(B):
    gen = torch.Generator().manual_seed(B)
    return {"images": torch.randint(0, 256, (B, 32, 32, 3), dtype=torch.uint8, generator=gen).cuda(),
            "labels": torch.zeros(B, dtype=torch.int32).cuda(), "conditioning": torch.zeros(B, dtype=torch.uint8).cuda()}


def _section(title, fn):
    torch.cuda.synchronize()
    LINES.append("# " + title)
    fn()
    torch.cuda.synchronize()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    a = ap.parse_args()
    torch.cuda.set_device(0)
    lib.load()
    exp = _experiment(4)
    _wrap()
    B, dev = 4, exp.device
    batch = _batch(B)

    def train(e, b):
        e.state, _ = e.train_step(e._train_rng, e.state, b)

    train(exp, batch)                            # (the first step also prepares what later steps re-use)
    _section("train step, eager, dropout, B = 4", lambda: train(exp, batch))
    ops.SIDE_STREAM = False
    _section("train step, eager, dropout, B = 4, MULAN_SIDE_STREAM=0", lambda: train(exp, batch))
    ops.SIDE_STREAM = True

    gen = torch.Generator(device="cuda").manual_seed(3)
    with torch.no_grad():                        # (zero-initialised layers would make the network output trivial)
        exp.state.ema.copy_(torch.randn(exp.state.ema.shape, device="cuda", generator=gen) * 0.03)
    model, params = exp.model, exp.state.ema_params
    packer = exp.state.param_packer("ema")
    if packer is not None:
        packer.refresh()
    key = PRNGKey(11)
    cond = torch.zeros(B, dtype=torch.uint8, device=dev)
    emb = model.deterministic_embedding(B, dev)
    z0 = key.normal((B, 3072), dev)
    with torch.no_grad():
        coeffs = model.sample_coefficients(params, emb)
        step = model.reverse_stepper(params, B, dev, emb, cond, coeffs, 6, graph=False)
        _section("ancestral reverse step, eager", lambda: step(0, z0.clone(), key))
        ctx = model.fast_context(params, emb, cond)
        fast = model.fast_stepper(params, B, dev, ctx, graph=False)
        grid, orders = sampling.time_grid(4), sampling.step_orders("dpm2m", 4)
        z1 = []
        _section("fast sampler step (dpm2m, order 1), eager", lambda: z1.append(fast(z0.clone(), grid[0], grid[1], orders[0])))
        _section("fast sampler step (dpm2m, order 2), eager", lambda: fast(z1[0], grid[1], grid[2], orders[1]))

    img = _batch(B)["images"]
    octx = model.ode_context(params, img)
    f = M.ode_function(model, params, octx, B, dev, True, graph=False)
    x = PRNGKey(12).normal((B, 3072), dev)
    probe = ops.noise((B, 3072), 2, 0, dev, "rademacher")
    drift, div = torch.empty_like(x), torch.empty(B, device=dev, dtype=x.dtype)
    _section("ODE function evaluation with divergence, eager", lambda: f(0.123, x, probe, drift, div))
    if packer is not None:
        packer.invalidate()

    big = _experiment(32)
    _wrap()
    batch32 = _batch(32)
    train(big, batch32)
    _section("train step, eager, dropout, B = 32 (GN_FWD_STREAM window)", lambda: train(big, batch32))

    with open(a.out, "w") as fh:
        fh.write("\n".join(LINES) + "\n")
    count = collections.Counter(l.split(" ", 1)[0] for l in LINES if not l.startswith("#"))
    watch = sorted(n for n in count if n.startswith(("mulan_absmax_rows", "mulan_colsum", "mulan_groupnorm_stats",
                                                     "mulan_add_absmax_rows")))
    print(f"{len(LINES)} lines -> {a.out}; " + ", ".join(f"{n} x{count[n]}" for n in watch))


if __name__ == "__main__":
    main()
