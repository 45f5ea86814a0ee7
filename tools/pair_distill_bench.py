#!/usr/bin/env python3
"""What distilling the full model's video ranking into the first-stage score costs, in one process:
  (a) term:  forward + backward of training.pair_distill_loss (smin_pair_distill_fwd: three launches, smin_pair_rank_bwd: one) against
             training.pair_distill_loss_torch in fp32 on the device -- the restatement reads the plan back and loops over the queries on
             the host, which is part of what it costs -- and against training.pair_rank_loss, at pair_rank_bench's shapes (P, Q, L) =
             (64, 16, 32), (64, 16, 64), (256, 64, 64);
  (b) step:  a mined step (V = Q = 16, three negatives per query, equal cell counts, mine_pool="lme"; no optimizer, no meter) through
             train_epoch_mined with distill_weight 0 and 0.5, each with prefilter_weight 0 and 0.5, and beside them the parent's step
             written out (encode, mine_pairs, forward_pairs, pair_targets, loss_fn, prefilter_rank_loss, backward): the distill_weight
             = 0 rows against it, the 0.5 rows as the increase over it;
  (c) first: a train_epoch_prefilter step (16 x 16, no optimizer; its one host read included on every side) with the contrastive term
             alone, with the soft-target term added and the model as its own teacher -- a full-model scoring pass over Q * V pairs under
             no_grad per step --, and the two terms over a teacher table computed beforehand: what the teacher pass costs.
Shapes of (b) and (c): tacos.yml and activitynet.yml (BASELINE.json configs).  After a warm-up of all sides, alternating blocks; every
timed call lies between two HIP events (host issue time is inside them).
    python tools/pair_distill_bench.py [--calls 100] [--warmup 5] [--block 10] [--runs 2] [--shapes tacos_yml,anet_yml] [--parts a,b,c]
Prints one JSON line per part, shape and run: the median and the 10-90 % spread of each side in microseconds.

Measured on an MI355X (exact fp32 mode, 60 calls, medians of run 1 / run 2 in microseconds; INTEGRATION.md 3z has the spreads):
  (a) (64, 16, 32): distill 118 / 81, torch 8 699 / 7 572, rank 116 / 84;  (64, 16, 64): 79 / 148, 8 065 / 10 502, 119 / 147;
      (256, 64, 64): 146 / 146, 34 764 / 36 896, 153 / 151 -- the term costs what pair_rank_loss costs, inside a spread of a factor two;
  (b) tacos.yml, prefilter_weight 0: parent 15 340 / 15 365, loop at distill_weight 0 15 418 / 15 416, at 0.5 16 824 / 16 821 (+1.5 ms: the
      first stage's encoder pass); prefilter_weight 0.5: 16 736 / 16 752, 16 803 / 16 836, 16 870 / 16 906 (+0.13 to 0.16 ms);
      activitynet.yml, 0: 44 950 / 44 937, 45 004 / 44 959, 46 489 / 46 435;  0.5: 46 473 / 46 486, 46 458 / 46 462, 46 630 / 46 614;
      the distill_weight = 0 rows lie within the parent's 10-90 % spread (-24 to +84 us of its median);
  (c) tacos.yml: contrastive term alone 2 003 / 1 967, both terms over a given table 2 163 / 1 950, with the teacher pass 9 964 / 9 844;
      activitynet.yml: 1 893 / 1 822, 1 884 / 1 835, 25 615 / 25 756 -- the teacher pass is where the term is slow.
Not measured: other sizes, the bf16 modes, the kernels without the Python call."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from pair_rank_bench import LOSS_SHAPES, loss_sides  # noqa: E402
from prefilter_train_bench import SHAPES, build, clear, timed_blocks  # noqa: E402

TAU = GAMMA = 0.1
N = 3


class NoOptimizer:
    """what the loops ask of an optimizer, with nothing updated: the gradients dropped, no step"""

    def __init__(self, model):
        self.model = model

    def zero_grad(self):
        clear(self.model)

    def step(self):
        pass


class NoMeter:
    def update(self, *args, **kw):
        pass

    def result(self):
        return {"loss": 0.0}


def bench_term(A, args, dev):
    for P, Q, L in LOSS_SHAPES:
        run_rank = loss_sides(A, dev, P, Q, L)["kernel"]                  # pair_rank_loss on pair_rank_bench's own tensors and plan
        g = torch.Generator().manual_seed(P + L)
        pm, ps, pe = (torch.rand(*shape, generator=g).to(dev).requires_grad_(True) for shape in ((P, L, L), (P, L), (P, L)))
        mm = torch.triu(torch.ones(L, L, dtype=torch.bool)).expand(P, L, L).contiguous().to(dev)
        S = P // Q
        plan = A.PairPlan(np.arange(P) % Q, np.arange(P) // S, Q, Q, dev)
        teacher = torch.rand(P, generator=g).to(dev)

        def side(fn):
            def run():
                pm.grad = ps.grad = pe.grad = None
                fn(pm, ps, pe, mm, plan, teacher, TAU, GAMMA).backward()
                return pm.grad, ps.grad, pe.grad
            return run
        ours = {"distill_kernel": side(A.pair_distill_loss), "distill_torch": side(A.pair_distill_loss_torch), "rank_kernel": run_rank}
        a, b = ours["distill_kernel"](), ours["distill_torch"]()
        torch.cuda.synchronize()
        for x, y in zip(a, b):
            assert (x - y).abs().max().item() <= 1e-4 * y.abs().max().item() + 1e-9, "the kernel and the torch route disagree"
        for run in range(args.runs):
            res = timed_blocks(ours, args.calls, args.warmup, args.block)
            print(json.dumps({"bench": "term", "P": P, "Q": Q, "L": L, "run": run, "calls": args.calls, "us": res,
                              "torch_over_kernel": round(res["distill_torch"]["median"] / res["distill_kernel"]["median"], 3),
                              "distill_over_rank": round(res["distill_kernel"]["median"] / res["rank_kernel"]["median"], 3)}), flush=True)


def bench_step(A, models, args, dev):
    V = Q = 16
    for name in args.shapes.split(","):
        m, g = build(models, A, SHAPES[name], V, Q, dev)
        inputs = [g[k] for k in A.training.MODEL_INPUTS]
        opt, meter = NoOptimizer(m), NoMeter()

        def parent(weight):
            def fn():
                clear(m)
                with torch.no_grad():
                    videos = m.encode_videos(g["video_features"], g["video_mask"], g["length_mask"], g["moment_mask"], cell_counts=g["cell_counts"])
                    queries = m.encode_queries(g["query_features"], g["query_mask"])
                    plan = m.mine_pairs(videos, queries, g["gt_video"], N, pool="lme", tau=TAU)
                out = m.forward_pairs(*inputs, None, None, cell_counts=g["cell_counts"], plan=plan)
                t = A.pair_targets(g, g, None, None, None, plan=plan)
                loss = A.loss_fn(out[0], t["ym"], t["sm"], t["moment_mask"], out[1], t["ys"], t["ss"], out[2], t["ye"], t["se"], out[3], t["ya"],
                                 t["length_mask"])
                if weight != 0.0:
                    loss = loss + weight * A.prefilter_rank_loss(m, g, TAU, GAMMA)
                loss.backward()
            return fn

        def loop(distill, prefilter):
            return lambda: A.train_epoch_mined(m, opt, [g], N, meter=meter, tau=TAU, gamma=GAMMA, mine_pool="lme", prefilter_weight=prefilter,
                                               distill_weight=distill)
        sides = {"parent_pw0": parent(0.0), "loop_dw0_pw0": loop(0.0, 0.0), "loop_dw0.5_pw0": loop(0.5, 0.0),
                 "parent_pw0.5": parent(0.5), "loop_dw0_pw0.5": loop(0.0, 0.5), "loop_dw0.5_pw0.5": loop(0.5, 0.5)}
        for run in range(args.runs):
            res = timed_blocks(sides, args.calls, args.warmup, args.block)
            med = {k: v["median"] for k, v in res.items()}
            print(json.dumps({"bench": "step", "shape": name, "run": run, "Q": Q, "V": V, "N": N, "gemm_mode": A.get_gemm_mode(), "calls": args.calls,
                              "us": res, "dw0_minus_parent_us": [round(med["loop_dw0_pw0"] - med["parent_pw0"], 2),
                                                                 round(med["loop_dw0_pw0.5"] - med["parent_pw0.5"], 2)],
                              "dw0.5_added_us": [round(med["loop_dw0.5_pw0"] - med["parent_pw0"], 2),
                                                 round(med["loop_dw0.5_pw0.5"] - med["parent_pw0.5"], 2)]}), flush=True)
        del m, g
        torch.cuda.empty_cache()


def bench_first(A, models, args, dev):
    V = Q = 16
    for name in args.shapes.split(","):
        m, g = build(models, A, SHAPES[name], V, Q, dev)
        opt = NoOptimizer(m)
        with torch.no_grad():
            videos = m.encode_videos(g["video_features"], g["video_mask"], g["length_mask"], g["moment_mask"], cell_counts=g["cell_counts"])
            table = m.pair_scores(videos, m.encode_queries(g["query_features"], g["query_mask"]), pool="lme", tau=TAU)

        def given_table():
            clear(m)
            loss, rank_stats, distill_stats = A.training._first_stage_terms("pair_distill_bench", m, g, TAU, GAMMA, 1.0, 0.5, table, None)
            loss.backward()
            return torch.cat([loss.detach().reshape(1), rank_stats, distill_stats]).tolist()      # the loop's one host read
        sides = {"rank_only": lambda: A.train_epoch_prefilter(m, opt, [g], TAU, GAMMA),
                 "rank_and_distill_teacher_pass": lambda: A.train_epoch_prefilter(m, opt, [g], TAU, GAMMA, distill_weight=0.5),
                 "rank_and_distill_given_table": given_table}
        for run in range(args.runs):
            res = timed_blocks(sides, args.calls, args.warmup, args.block)
            med = {k: v["median"] for k, v in res.items()}
            print(json.dumps({"bench": "first", "shape": name, "run": run, "Q": Q, "V": V, "gemm_mode": A.get_gemm_mode(), "calls": args.calls, "us": res,
                              "term_added_us": round(med["rank_and_distill_given_table"] - med["rank_only"], 2),
                              "teacher_pass_us": round(med["rank_and_distill_teacher_pass"] - med["rank_and_distill_given_table"], 2)}), flush=True)
        del m, g
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--block", type=int, default=10)
    ap.add_argument("--runs", type=int, default=2)
    ap.add_argument("--shapes", default="tacos_yml,anet_yml")
    ap.add_argument("--parts", default="a,b,c")
    args = ap.parse_args()
    import models
    A = models.vml_amd
    assert torch.cuda.is_available(), "pair_distill_bench needs a HIP device"
    dev = torch.device("cuda:0")
    A._lib.load_torch()
    parts = args.parts.split(",")
    if "a" in parts:
        bench_term(A, args, dev)
    if "b" in parts:
        bench_step(A, models, args, dev)
    if "c" in parts:
        bench_first(A, models, args, dev)


if __name__ == "__main__":
    main()
