"""mulan_image_fidelity beside the formulation a user would otherwise write in torch on the same device (bytes to fp32,
F.conv2d with the grouped separable Gaussian window on the five maps x, y, x^2, y^2, x y, the SSIM quotient and its
mean; the squared errors summed exactly through int32), by HIP events, alternated, medians (the timing of DESIGN 3.13).

python tools/fidelity_bench.py [--n 50000 --rounds 7 --inner 10 --gray 0]

Both produce sse [N, 3] and ssim [N, P]; no map is written by the kernel (the torch formulation has to materialise
all five, twice).  A timed window is `inner` calls, each allocating its outputs as a user's call does.  Prints one JSON
line: seconds per call of each (median, min, max of the windows' means), their ratio, the device-to-device copy rate
measured here on 1 GiB (bytes read plus bytes written over the time), the kernel's share of it for the image bytes it
reads (N 6144 bytes at that rate over the kernel's time), the flops of the two filter passes over the kernel's time,
and the largest differences between the two formulations' results."""
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from mulan_amd import ops  # noqa: E402

C1, C2 = (0.01 * 255.0) ** 2, (0.03 * 255.0) ** 2


def arg(name, default):
    return type(default)(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


def window_taps(device):
    k = torch.arange(11, dtype=torch.float64) - 5.0
    e = torch.exp(-k * k / 4.5)
    return (e / e.sum()).float().to(device)


def torch_fidelity(a, b, w, gray):
    d = a.to(torch.int32) - b.to(torch.int32)
    sse = (d * d).sum(dim=(1, 2), dtype=torch.int32)                # exact: at most 1024 255^2 < 2^31
    x, y = a.float(), b.float()
    if gray:
        mix = torch.tensor(ops.SPECTRUM_GRAY, device=a.device)
        x, y = (x * mix).sum(-1, keepdim=True), (y * mix).sum(-1, keepdim=True)
    x, y = x.permute(0, 3, 1, 2) - 128.0, y.permute(0, 3, 1, 2) - 128.0      # [N, P, 32, 32], centred as the kernel centres
    P = x.shape[1]
    maps = torch.cat([x, y, x * x, y * y, x * y], dim=1)            # [N, 5 P, 32, 32]
    wh = w.view(1, 1, 1, 11).expand(5 * P, 1, 1, 11).contiguous()
    wv = w.view(1, 1, 11, 1).expand(5 * P, 1, 11, 1).contiguous()
    f = F.conv2d(F.conv2d(maps, wh, groups=5 * P), wv, groups=5 * P)         # [N, 5 P, 22, 22]
    mx, my, exx, eyy, exy = f.split(P, dim=1)
    sxx, syy, sxy = exx - mx * mx, eyy - my * my, exy - mx * my
    mx, my = mx + 128.0, my + 128.0
    s = ((2 * mx * my + C1) * (2 * sxy + C2)) / ((mx * mx + my * my + C1) * (sxx + syy + C2))
    return sse, s.mean(dim=(2, 3))


def window(fn, inner):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(inner):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e-3 / inner


def main():
    N, rounds, inner = arg("--n", 50000), arg("--rounds", 7), arg("--inner", 10)
    gray = bool(arg("--gray", 0))
    P = 1 if gray else 3
    g = torch.Generator(device="cuda").manual_seed(0)
    a = torch.randint(0, 256, (N, 32, 32, 3), dtype=torch.uint8, device="cuda", generator=g)
    noise = torch.randint(-20, 21, (N, 32, 32, 3), dtype=torch.int16, device="cuda", generator=g)
    b = (a.to(torch.int16) + noise).clamp_(0, 255).to(torch.uint8)  # a noisy copy: SSIM away from both 0 and 1
    w = window_taps("cuda")
    run_hip = lambda: ops.image_fidelity(a, b, gray=gray)          # noqa: E731
    run_torch = lambda: torch_fidelity(a, b, w, gray)             # noqa: E731
    src = torch.empty(1 << 28, dtype=torch.float32, device="cuda").normal_()     # 1 GiB: beyond the Infinity Cache
    dst = torch.empty_like(src)
    run_copy = lambda: dst.copy_(src)                             # noqa: E731
    (h_sse, _, h_ssim, _), (t_sse, t_ssim) = run_hip(), run_torch()           # warm-up, and the results to compare
    run_copy()
    torch.cuda.synchronize()
    agree = dict(sse=int((h_sse - t_sse).abs().max()), ssim=float((h_ssim - t_ssim).abs().max()),
                 ssim_mean=float(h_ssim.mean()))
    t_hip, t_torch, t_copy = [], [], []
    for _ in range(rounds):
        t_hip.append(window(run_hip, inner))
        t_torch.append(window(run_torch, max(1, inner // 4)))
        t_copy.append(window(run_copy, 4))
    med = statistics.median
    copy_rate = 2.0 * src.numel() * 4 / med(t_copy)
    image_bytes = N * 2 * 3072
    flops = N * P * 2 * 5 * 11 * (32 * 22 + 22 * 22)              # 2 flops per tap, five maps, rows then columns
    res = dict(N=N, P=P, rounds=rounds, inner=inner,
               hip_s=dict(median=med(t_hip), min=min(t_hip), max=max(t_hip)),
               torch_s=dict(median=med(t_torch), min=min(t_torch), max=max(t_torch)),
               torch_over_hip=med(t_torch) / med(t_hip),
               copy_bytes_per_s=copy_rate, image_bytes=image_bytes,
               share_of_copy_rate=image_bytes / copy_rate / med(t_hip),
               flops=flops, flops_per_s=flops / med(t_hip), max_abs_difference=agree)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
