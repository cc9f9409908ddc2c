"""mulan_spectrum beside the formulation a user would otherwise write in torch on the same device (bytes to fp32, two
torch.matmul with the DCT matrix, the square, an index_add over the radial bins, the set sums in fp64), by HIP events,
alternated, medians (the timing of DESIGN 3.11).

python tools/spectrum_bench.py [--n 50000 --rounds 7 --inner 20 --gray 0 --blocks 0]

Both produce the per-image radial power [N, 45, P] and the set sums of Y and Y^2 [32, 32, P] in fp64; no coefficient is
written by the kernel (the torch formulation has to materialise them).  A timed window is `inner` calls, each allocating
its outputs as a user's call does.  Prints one JSON line: seconds per call of each (median, min, max of the windows'
means), the device-to-device copy rate measured here on 1 GiB (bytes read plus bytes written over the time), the
kernel's share of it for the image bytes it reads (N 3072 bytes at that rate over the kernel's time), the flops of the
two products (N P 2 2 32^3) over the kernel's time, and the largest differences between the two formulations'
results."""
import json
import math
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from mulan_amd import ops  # noqa: E402

SCALE, OFFSET = 2.0 / 256.0, 1.0 / 256.0 - 1.0


def arg(name, default):
    return type(default)(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


def dct_matrix(device):
    u = torch.arange(32, dtype=torch.float64)[:, None]
    y = torch.arange(32, dtype=torch.float64)[None, :]
    d = torch.cos(math.pi * (2 * y + 1) * u / 64.0) * math.sqrt(2.0 / 32.0)
    d[0] = math.sqrt(1.0 / 32.0)
    return d.float().to(device)


def bin_index(device):
    s = torch.arange(32)[:, None] ** 2 + torch.arange(32)[None, :] ** 2
    r = torch.arange(45)
    return torch.searchsorted(r * r + r, s.reshape(-1)).to(device)


def torch_spectrum(x, d, bins, gray):
    v = x.float() * SCALE + OFFSET                                  # [N, 32, 32, 3]
    if gray:
        v = (v * torch.tensor(ops.SPECTRUM_GRAY, device=x.device)).sum(-1, keepdim=True)
    v = v.permute(0, 3, 1, 2)                                       # [N, P, y, x]
    y = torch.matmul(torch.matmul(d, v), d.T)                       # [N, P, u, v]
    p = y * y
    radial = torch.zeros((x.shape[0], p.shape[1], 45), device=x.device)
    radial.index_add_(2, bins, p.reshape(x.shape[0], p.shape[1], 1024))
    return radial.permute(0, 2, 1), y.sum(0, dtype=torch.float64).permute(1, 2, 0), p.sum(0, dtype=torch.float64).permute(1, 2, 0)


def window(fn, inner):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(inner):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e-3 / inner


def main():
    N, rounds, inner = arg("--n", 50000), arg("--rounds", 7), arg("--inner", 20)
    gray, blocks = bool(arg("--gray", 0)), arg("--blocks", 0)
    P = 1 if gray else 3
    g = torch.Generator(device="cuda").manual_seed(0)
    x = torch.randint(0, 256, (N, 32, 32, 3), dtype=torch.uint8, device="cuda", generator=g)
    d, bins = dct_matrix("cuda"), bin_index("cuda")
    run_hip = lambda: ops.spectrum(x, scale=SCALE, offset=OFFSET, gray=gray, radial=True, sums=True, blocks=blocks)  # noqa: E731
    run_torch = lambda: torch_spectrum(x, d, bins, gray)          # noqa: E731
    src = torch.empty(1 << 28, dtype=torch.float32, device="cuda").normal_()     # 1 GiB: beyond the Infinity Cache
    dst = torch.empty_like(src)
    run_copy = lambda: dst.copy_(src)                             # noqa: E731
    (_, hr, (h1, h2)), (tr, t1, t2) = run_hip(), run_torch()      # warm-up, and the results to compare
    run_copy()
    torch.cuda.synchronize()
    agree = dict(radial=float((hr - tr).abs().max()), radial_scale=float(tr.abs().max()),
                 sum1=float((h1 - t1).abs().max()), sum2=float((h2 - t2).abs().max()), sum2_scale=float(t2.abs().max()))
    t_hip, t_torch, t_copy = [], [], []
    for _ in range(rounds):
        t_hip.append(window(run_hip, inner))
        t_torch.append(window(run_torch, max(1, inner // 4)))
        t_copy.append(window(run_copy, 4))
    med = statistics.median
    copy_rate = 2.0 * src.numel() * 4 / med(t_copy)
    image_bytes = N * 3072
    res = dict(N=N, P=P, rounds=rounds, inner=inner, blocks=blocks,
               hip_s=dict(median=med(t_hip), min=min(t_hip), max=max(t_hip)),
               torch_s=dict(median=med(t_torch), min=min(t_torch), max=max(t_torch)),
               copy_bytes_per_s=copy_rate, image_bytes=image_bytes,
               share_of_copy_rate=image_bytes / copy_rate / med(t_hip),
               flops=N * P * 2 * 2 * 32 ** 3, flops_per_s=N * P * 2 * 2 * 32 ** 3 / med(t_hip), max_abs_difference=agree)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
