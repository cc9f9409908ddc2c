"""mulan_knn_u8 beside the formulation a user would otherwise write (chunked fp32 torch.matmul + torch.topk), by HIP
events, alternated, medians (the timing of DESIGN 3.10).

python tools/neighbours_bench.py [--q 50000 --n 50000 --d 3072 --k 5 --rounds 5 --splits 0 --torch_chunk 4096]

Prints one JSON line: seconds per search of each (median, min, max), the int8 operations per second the kernel reaches
(2 Q N D / t), the bytes its blocks request (every 128 x 128 tile pair streams both of its operands once: L2 / Infinity
Cache traffic, of which HBM sees the part that misses), the two floors (the operations at the int8 peak, the two arrays
read once from HBM), and whether the two formulations agree (fp32 products of recentred bytes are exact below 2^24 only,
so the torch lists may differ in ties and, at large D, in the last place: reported, not asserted)."""
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from mulan_amd import ops  # noqa: E402

INT8_PEAK = 5.0e15          # dense int8 op/s of one MI355X: twice the bf16 figure of 2.5e15
HBM_RATE = 8.0e12           # bytes/s, the vendor's figure


def arg(name, default):
    return type(default)(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


def torch_knn(q, r, k, chunk):
    rf = r.float() - 128.0
    rn = (rf * rf).sum(1)
    ds, js = [], []
    for lo in range(0, q.shape[0], chunk):
        qf = q[lo:lo + chunk].float() - 128.0
        d = (qf * qf).sum(1)[:, None] + rn[None, :] - 2.0 * (qf @ rf.T)
        v, j = torch.topk(d, k, dim=1, largest=False)
        ds.append(v)
        js.append(j)
    return torch.cat(ds), torch.cat(js)


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e-3, out


def main():
    Q, N, D, k = arg("--q", 50000), arg("--n", 50000), arg("--d", 3072), arg("--k", 5)
    rounds, splits, chunk = arg("--rounds", 5), arg("--splits", 0), arg("--torch_chunk", 4096)
    g = torch.Generator(device="cuda").manual_seed(0)
    q = torch.randint(0, 256, (Q, D), dtype=torch.uint8, device="cuda", generator=g)
    r = torch.randint(0, 256, (N, D), dtype=torch.uint8, device="cuda", generator=g)
    run_hip = lambda: ops.knn_u8(q, r, k, splits=splits)          # noqa: E731  (allocates its lists and workspace, as a user's call)
    run_torch = lambda: torch_knn(q, r, k, chunk)                 # noqa: E731
    hip_out, torch_out = run_hip(), run_torch()                   # warm-up, and the lists to compare
    torch.cuda.synchronize()
    t_hip, t_torch = [], []
    for _ in range(rounds):
        t_hip.append(timed(run_hip)[0])
        t_torch.append(timed(run_torch)[0])
    med = statistics.median
    tiles = -(-Q // 128) * -(-N // 128)
    res = dict(Q=Q, N=N, D=D, k=k, rounds=rounds, splits=splits,
               hip_s=dict(median=med(t_hip), min=min(t_hip), max=max(t_hip)),
               torch_s=dict(median=med(t_torch), min=min(t_torch), max=max(t_torch)),
               int8_ops_per_s=2.0 * Q * N * D / med(t_hip), requested_bytes=tiles * 256 * D, hbm_floor_bytes=(Q + N) * D,
               floor_s=dict(int8_peak=2.0 * Q * N * D / INT8_PEAK, hbm=(Q + N) * D / HBM_RATE),
               same_indices=float((hip_out[1].long() == torch_out[1]).float().mean()),
               same_dist2=float((hip_out[0].float() == torch_out[0]).float().mean()))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
