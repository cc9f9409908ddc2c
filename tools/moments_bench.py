"""mulan_set_moments_u8 beside the two formulations a user would otherwise write in torch on the same device, by HIP
events, alternated, medians (the timing of DESIGN 3.14).

python tools/moments_bench.py [--n 50000 --d 3072 --rounds 7 --inner 5]

  exact    c = x.double() - 128;  c.T @ c       float64 holds every partial sum (N 2^14 < 2^53): the same integers
  fp32     c = x.float() - 128;   c.T @ c       inexact: its largest deviation from the integers is printed

A timed window is `inner` calls, each allocating its outputs (and, for torch, its converted copy of x) as a user's call
does.  Prints one JSON line: seconds per call of each (median, min, max of the windows' means), the ratios, whether the
kernel's integers equal the exact formulation's, the fp32 formulation's largest deviation, the device-to-device copy
rate measured here on 1 GiB (bytes read plus bytes written over the time), the time that rate needs for the N D bytes
of x and the kernel's multiple of it, and the int8 multiply-adds of the computed tiles over the kernel's time."""
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from mulan_amd import ops  # noqa: E402


def arg(name, default):
    return type(default)(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


def window(fn, inner):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(inner):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e-3 / inner


def torch_exact(x):
    c = x.double() - 128.0
    return c.sum(dim=0), c.T @ c


def torch_fp32(x):
    c = x.float() - 128.0
    return c.sum(dim=0), c.T @ c


def main():
    N, D, rounds, inner = arg("--n", 50000), arg("--d", 3072), arg("--rounds", 7), arg("--inner", 5)
    g = torch.Generator(device="cuda").manual_seed(0)
    x = torch.randint(0, 256, (N, D), dtype=torch.uint8, device="cuda", generator=g)
    run_hip = lambda: ops.set_moments_u8(x)                       # noqa: E731
    run_exact = lambda: torch_exact(x)                            # noqa: E731
    run_fp32 = lambda: torch_fp32(x)                              # noqa: E731
    src = torch.empty(1 << 28, dtype=torch.float32, device="cuda").normal_()     # 1 GiB: beyond the Infinity Cache
    dst = torch.empty_like(src)
    run_copy = lambda: dst.copy_(src)                             # noqa: E731
    (h_sum, h_gram), (e_sum, e_gram), (f_sum, f_gram) = run_hip(), run_exact(), run_fp32()   # warm-up, and the results
    run_copy()
    torch.cuda.synchronize()
    agree = dict(kernel_equals_exact=bool((h_gram.double() == e_gram).all()) and bool((h_sum.double() == e_sum).all()),
                 fp32_max_deviation=float((f_gram.double() - e_gram).abs().max()), gram_max=float(e_gram.abs().max()))
    del e_sum, e_gram, f_sum, f_gram
    t_hip, t_exact, t_fp32, t_copy = [], [], [], []
    for _ in range(rounds):
        t_hip.append(window(run_hip, inner))
        t_exact.append(window(run_exact, max(1, inner // 4)))
        t_fp32.append(window(run_fp32, inner))
        t_copy.append(window(run_copy, 4))
    med = statistics.median
    stats = lambda t: dict(median=med(t), min=min(t), max=max(t))  # noqa: E731
    copy_rate = 2.0 * src.numel() * 4 / med(t_copy)
    T = (D + 127) // 128
    macs = (T * (T + 1) // 2) * 128 * 128 * N                     # the tiles on and above the diagonal
    res = dict(N=N, D=D, rounds=rounds, inner=inner, hip_s=stats(t_hip), torch_exact_s=stats(t_exact),
               torch_fp32_s=stats(t_fp32), exact_over_hip=med(t_exact) / med(t_hip), fp32_over_hip=med(t_fp32) / med(t_hip),
               copy_bytes_per_s=copy_rate, x_bytes=N * D, copy_time_of_x_s=N * D / copy_rate,
               hip_over_copy_time=med(t_hip) / (N * D / copy_rate), int8_macs=macs, int8_ops_per_s=2.0 * macs / med(t_hip),
               **agree)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
