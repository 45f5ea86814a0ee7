#!/usr/bin/env python3
"""The contrastive loss over a pair plan, in one process:
  (a) forward and backward of training.pair_rank_loss (smin_pair_rank_fwd: three launches, smin_pair_rank_bwd: one) against forward
      and backward of training.pair_rank_loss_torch in fp32 on the device -- the restatement reads the plan back once per call and
      loops over the queries on the host, which is part of what it costs --, at (P, Q, L) = (64, 16, 32), (64, 16, 64), (256, 64, 64):
      each query's own video and P / Q - 1 others, synthetic scores, full upper-triangular masks;
  (b) a 64-pair training step without the optimizer at tacos.yml (V = Q = 16 full-length videos, each query's own video and three
      drawn once; gradients to None, forward_pairs, loss_fn over pair_targets, backward) with rank_weight = 0.5 against the same step
      with rank_weight = 0, the parent's step: what the term costs.
After a warm-up of every side, alternating blocks of the sides; every timed call lies between two HIP events (host issue time is
inside them).
    python tools/pair_rank_bench.py [--calls 100] [--warmup 5] [--block 10] [--runs 2] [--skip-steps]
Prints one JSON line per part, shape and run: the median and the 10-90 % spread of each side in microseconds."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from mine_pairs_bench import SHAPES, alternate  # noqa: E402

LOSS_SHAPES = [(64, 16, 32), (64, 16, 64), (256, 64, 64)]


def loss_sides(A, dev, P, Q, L, tau=0.1, gamma=0.1):
    S = P // Q
    g = torch.Generator().manual_seed(P + L)
    pm, ps, pe = (torch.rand(*shape, generator=g).to(dev).requires_grad_(True) for shape in ((P, L, L), (P, L), (P, L)))
    mm = torch.triu(torch.ones(L, L, dtype=torch.bool)).expand(P, L, L).contiguous().to(dev)
    rng = np.random.RandomState(P)
    qi = np.repeat(np.arange(Q), S)
    vi = np.concatenate([[q] + list(rng.choice([v for v in range(Q) if v != q], S - 1, replace=False)) for q in range(Q)])
    plan = A.PairPlan(vi, qi, Q, Q, dev, gt_video=np.arange(Q))

    def side(fn):
        def run():
            pm.grad = ps.grad = pe.grad = None
            fn(pm, ps, pe, mm, plan, tau, gamma).backward()
            return pm.grad, ps.grad, pe.grad
        return run

    return {"kernel": side(A.pair_rank_loss), "torch": side(A.pair_rank_loss_torch)}


def check_loss(sides):
    """the two routes agree to fp32 rounding before anything is timed"""
    a, b = sides["kernel"](), sides["torch"]()
    torch.cuda.synchronize()
    for x, y in zip(a, b):
        assert (x - y).abs().max().item() <= 1e-4 * y.abs().max().item() + 1e-9, "the kernel and the torch route disagree"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--block", type=int, default=10)
    ap.add_argument("--runs", type=int, default=2)
    ap.add_argument("--skip-steps", action="store_true", help="part (a) only")
    args = ap.parse_args()
    import models
    from oracle import smin_oracle as O
    from tests import helpers as H
    A = models.vml_amd
    assert torch.cuda.is_available(), "pair_rank_bench needs a HIP device"
    dev = torch.device("cuda:0")
    A._lib.load_torch()
    for P, Q, L in LOSS_SHAPES:
        sides = loss_sides(A, dev, P, Q, L)
        check_loss(sides)
        for run in range(args.runs):
            res = alternate(sides, args.calls, args.block, args.warmup)
            print(json.dumps({"part": "loss", "P": P, "Q": Q, "L": L, "run": run, "calls": args.calls, "us": res,
                              "torch_over_kernel": round(res["torch"]["median"] / res["kernel"]["median"], 3)}), flush=True)
    if args.skip_steps:
        return
    V = Q = 16
    N = 3
    name = "tacos_yml"
    T, L, C, D, dl, layers, Din, Nq, Hh = shape = SHAPES[name]
    m = models.SMIN(*shape, dev)
    m.load_state_dict(O.formula_state_dict(H.smin_shapes(*shape), gain=1.3))
    m = m.to(dev).train()
    vb = {k: v.to(dev) for k, v in O.synthetic_batch(V, T, L, Nq, Din, seed=1, with_labels=False, full_length=True).items()}
    qb = {k: v.to(dev) for k, v in O.synthetic_batch(Q, T, L, Nq, Din, seed=2, full_length=True).items()}
    vid = {k: vb[k] for k in ("video_features", "video_mask", "length_mask", "moment_mask")}
    inputs = [vid["video_features"], vid["video_mask"], qb["query_features"], qb["query_mask"], vid["length_mask"], vid["moment_mask"]]
    cells = vid["moment_mask"].reshape(V, -1).sum(1).tolist()
    assert len(set(cells)) == 1
    gt = np.arange(Q)
    rng = np.random.RandomState(7)
    qi = np.repeat(np.arange(Q), 1 + N)
    vi = np.concatenate([[q] + list(rng.choice([v for v in range(V) if v != q], N, replace=False)) for q in range(Q)])

    def step(weight):
        def fn():
            for p in m.parameters():
                p.grad = None
            plan = A.PairPlan(vi, qi, V, Q, dev, gt_video=gt)
            out = m.forward_pairs(*inputs, None, None, cell_counts=cells, plan=plan)
            t = A.pair_targets(vid, qb, None, None, None, plan=plan)
            loss = A.loss_fn(out[0], t["ym"], t["sm"], t["moment_mask"], out[1], t["ys"], t["ss"], out[2], t["ye"], t["se"], out[3], t["ya"], t["length_mask"])
            if weight:
                loss = loss + weight * A.pair_rank_loss(out[0], out[1], out[2], t["moment_mask"], plan)
            loss.backward()
        return fn

    sides = {"rank_weight_0.5": step(0.5), "rank_weight_0": step(0.0)}
    for run in range(args.runs):
        res = alternate(sides, args.calls, args.block, args.warmup)
        print(json.dumps({"part": "step", "shape": name, "run": run, "pairs": len(vi), "gemm_mode": A.get_gemm_mode(), "calls": args.calls, "us": res,
                          "with_over_without": round(res["rank_weight_0.5"]["median"] / res["rank_weight_0"]["median"], 4)}), flush=True)


if __name__ == "__main__":
    main()
