"""Times top_moments and the NMS metric (compute_ious(..., nms_thresh)) against top_moments_torch on the device, with device
events after warm-up, at the ActivityNet eval shape (B = 64, L = 64, k = 5) and the long-video shape (B = 16, L = 512,
k = 5 and 64).  Prints one JSON line per case; `pm_gbps` is the B*L*L*4 bytes of pm over the top_moments call time (the kernel
time comes from a separate rocprofv3 --kernel-trace --stats run).

    python tools/moments_bench.py [--iters 50] [--torch-iters 3] [--out path.json]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import models  # noqa: E402

api = models.vml_amd
CASES = [("anet_eval", 64, 64, 5), ("long_video", 16, 512, 5), ("long_video", 16, 512, 64)]


def inputs(B, L, dev, seed=0):
    g = torch.Generator().manual_seed(seed)
    lm = torch.ones(B, L, dtype=torch.bool)
    mm = torch.triu(lm.unsqueeze(2) & lm.unsqueeze(1))
    pm = torch.rand(B, L, L, generator=g) * mm
    ps, pe = torch.rand(B, L, generator=g), torch.rand(B, L, generator=g)
    sm = torch.rand(B, L, L, generator=g) * mm
    return [x.to(dev) for x in (pm, ps, pe, mm, sm)]


def time_ms(fn, iters, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--torch-iters", type=int, default=2)
    ap.add_argument("--thr", type=float, default=0.5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "moments_bench needs a HIP device"
    dev = torch.device("cuda:0")
    rows = []
    for name, B, L, k in CASES:
        pm, ps, pe, mm, sm = inputs(B, L, dev)
        top = time_ms(lambda: api.top_moments(pm, ps, pe, mm, k=k, nms_thresh=a.thr), a.iters, 5)
        metric = time_ms(lambda: api.compute_ious(pm, ps, pe, mm, sm, n=(1, k), m=(0.3, 0.5, 0.7), nms_thresh=a.thr), a.iters, 5)
        ref = time_ms(lambda: api.top_moments_torch(pm, ps, pe, mm, k=k, nms_thresh=a.thr), a.torch_iters, 1)
        got, want = api.top_moments(pm, ps, pe, mm, k=k, nms_thresh=a.thr), api.top_moments_torch(pm, ps, pe, mm, k=k, nms_thresh=a.thr)
        same = all(torch.equal(got[x], want[x]) for x in ("idx", "score", "count"))
        row = dict(case=name, B=B, L=L, k=k, nms_thresh=a.thr, top_moments_ms=round(top, 4), compute_ious_nms_ms=round(metric, 4),
                   top_moments_torch_ms=round(ref, 2), speedup=round(ref / top, 1), pm_gbps=round(B * L * L * 4 / (top * 1e-3) / 1e9, 1),
                   equal_to_torch=same)
        print(json.dumps(row), flush=True)
        rows.append(row)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
