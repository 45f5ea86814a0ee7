"""The video-level contrastive loss over a pair plan: csrc/pair_rank.hip smin_pair_rank_fwd / smin_pair_rank_bwd,
the operator smin_hip::smin_pair_rank_loss, functional.PairRankFn, training.pair_rank_loss / pair_rank_loss_torch and the
``rank_weight`` of train_epoch_pairs / train_epoch_mined.

Host: the C ABI and operator surface, pair_rank_loss_torch in fp64 against a hand-written loop over queries and cells (loss, stats,
pair scores, the three gradients) on the VI9 plan and on a mined layout, the degenerate plans, the refusals.
GPU: the kernels against pair_rank_loss_torch in fp64, gated by the error of pair_rank_loss_torch in fp32 on the same device
(e_kernel <= 32 * e_torch32 + 1e-6, e = max|x - x64| / max|x64|); every output written over a sentinel, the same bits twice and on
both routes, the rejections through the C ABI; through the tiny model against the fp64 oracle (e_new <= 2 * e_ref32 + 1e-6); the two
loops without a host read and, at rank_weight 0, the parent's step bit for bit.
Small gamma (saturated_pairs, tests/support/corpora.py): a query whose own video lies d = 50, 95, 120 and 800 temperatures below its best
negative, against the definition in stable form -- on the host the restatement in fp64 and fp32 (and the formula it had before, which
gives inf and NaN from d = 120 on), on the GPU the kernels.

Figures measured on an MI355X (printed by the tests): in the docstrings of test_kernels_against_fp64 and the two model tests, and in
INTEGRATION.md 3q."""
import math
import os
import re

import pytest
import torch

from tests.support.device import dev  # noqa: F401  (the module's device fixture)
from tests.support.device import vml as V
from tests.support.compare import bits, gate
from tests.support.corpora import world  # noqa: F401  (fixture)
from tests.support.corpora import (
    checked, expand, full_group, hand_step, loss_of, mined_plan, p19_lists, pair_args, plan_of, probe, same_parameters, saturated_pairs,
    stable_rank_loss, synthetic, tiny_model, GT_VIDEO, NQ, NV, QI9, RANK_DEPTHS, VI9)
from tests.support.references import abi_call

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TEMPS = [(1.0, 1.0), (0.1, 0.1), (0.01, 0.05)]
NAMES = ("smin_pair_rank_fwd", "smin_pair_rank_bwd", "smin_pair_rank_ws_bytes")


def by_hand(pm, ps, pe, mm, q_ptr, q_pairs, positive, tau, gamma):
    """The issue's formulas as a Python loop over queries and cells in float64: loss, [Nc, hits], s, dpm, dps, dpe."""
    pm, ps, pe, mm = pm.tolist(), ps.tolist(), pe.tolist(), mm.tolist()
    P, L = len(ps), len(ps[0])
    a = [[math.sqrt(max(ps[p][i], 1e-12)) for i in range(L)] for p in range(P)]
    b = [[math.sqrt(max(pe[p][j], 1e-12)) for j in range(L)] for p in range(P)]
    f = [[[(pm[p][i][j] * a[p][i]) * b[p][j] for j in range(L)] for i in range(L)] for p in range(P)]
    cells = [[(i, j) for i in range(L) for j in range(L) if mm[p][i][j]] for p in range(P)]
    s, top, z = [0.0] * P, [0.0] * P, [0.0] * P
    for p in range(P):
        if cells[p]:
            top[p] = max(f[p][i][j] for i, j in cells[p])
            z[p] = sum(math.exp((f[p][i][j] - top[p]) / tau) for i, j in cells[p])
            s[p] = top[p] + tau * math.log(z[p] / len(cells[p]))
    total, counted, hits, coef = 0.0, 0, 0, [0.0] * P
    for q in range(len(q_ptr) - 1):
        seg = q_pairs[q_ptr[q]:q_ptr[q + 1]]
        pos = [p for p in seg if positive[p]]
        if not pos:
            continue
        neg = [p for p in seg if not positive[p]]
        big = max(s[p] for p in seg)
        za, zp = sum(math.exp((s[p] - big) / gamma) for p in seg), sum(math.exp((s[p] - big) / gamma) for p in pos)
        total += math.log(za) - math.log(zp)
        counted += 1
        hits += int(not neg or max(s[p] for p in pos) >= max(s[p] for p in neg))
        for p in seg:
            x = math.exp((s[p] - big) / gamma)
            coef[p] += (x / za - (x / zp if positive[p] else 0.0)) / gamma
    loss = total / counted if counted else 0.0
    dpm = [[[0.0] * L for _ in range(L)] for _ in range(P)]
    dps, dpe = [[0.0] * L for _ in range(P)], [[0.0] * L for _ in range(P)]
    for p in range(P):
        if not counted:
            break
        for i, j in cells[p]:
            df = coef[p] / counted * math.exp((f[p][i][j] - top[p]) / tau) / z[p]
            dpm[p][i][j] = df * a[p][i] * b[p][j]
            if ps[p][i] >= 1e-12:
                dps[p][i] += df * pm[p][i][j] * b[p][j] * 0.5 / a[p][i]
            if pe[p][j] >= 1e-12:
                dpe[p][j] += df * pm[p][i][j] * a[p][i] * 0.5 / b[p][j]
    t = lambda x: torch.tensor(x, dtype=torch.float64)
    return t(loss), [counted, hits], t(s), t(dpm), t(dps), t(dpe)


def torch_route(x, plan, tau, gamma, dtype, dev="cpu", upstream=1.0):
    """pair_rank_loss_torch in ``dtype`` on ``dev``: loss, stats, pair_score, dpm, dps, dpe (as float64 on the host)"""
    pm, ps, pe = (t.to(device=dev, dtype=dtype).requires_grad_(True) for t in x[:3])
    loss, stats, score = V().pair_rank_loss_torch(pm, ps, pe, x[3].to(dev), plan, tau, gamma, return_stats=True)
    (upstream * loss).backward()
    return [t.detach().cpu().double() for t in (loss, stats, score, pm.grad, ps.grad, pe.grad)]


# ---------------------------------------------------------------- host
def test_surface():
    text = open(os.path.join(ROOT, "include", "smin_hip.h")).read()
    assert re.search(r"\bint\s+smin_pair_rank_fwd\s*\(", text) and re.search(r"\bint\s+smin_pair_rank_bwd\s*\(", text)
    assert re.search(r"\bsize_t\s+smin_pair_rank_ws_bytes\s*\(\s*int\s+P\s*,\s*int\s+Q\s*,\s*int\s+L\s*\)", text)
    lib = V()._lib.load()
    for name in NAMES:
        assert name in V()._lib.SIGNATURES, name
        assert hasattr(lib, name)
    assert "#define SMIN_HIP_ABI_VERSION 2" in text and lib.smin_abi_version() == 2
    assert lib.smin_pair_rank_ws_bytes(64, 16, 32) == 16 * 16 and lib.smin_pair_rank_ws_bytes(0, 16, 32) == 0
    ops = V()._lib.load_torch()
    assert hasattr(ops, "smin_pair_rank_loss")
    schema = str(torch.ops.smin_hip.smin_pair_rank_loss.default._schema)
    assert ("smin_pair_rank_loss(Tensor pm, Tensor ps, Tensor pe, Tensor moment_mask, Tensor q_ptr, Tensor q_pairs, Tensor positive, float tau, "
            "float gamma) -> (Tensor loss, Tensor stats, Tensor pair_score)") in schema, schema
    assert callable(V().pair_rank_loss) and callable(V().pair_rank_loss_torch)
    assert hasattr(V().functional, "PairRankFn")


@pytest.mark.parametrize("layout", ["vi9", "mined"])
@pytest.mark.parametrize("tau,gamma", [(1.0, 1.0), (0.1, 0.1)])
def test_torch_route_by_hand(layout, tau, gamma):
    plan = plan_of(9, 4) if layout == "vi9" else mined_plan()
    if layout == "vi9":
        assert plan.q_ptr.tolist() == [0, 3, 7, 9, 9] and plan.positive.tolist() == [1, 1, 1, 0, 0, 0, 1, 0, 0]
    else:
        assert plan.P == 9 and plan.Q == 3 and plan.vi is None
    x = synthetic(9, 3, seed=5, dtype=torch.float64)
    assert not x[3][4].any() and x[3].reshape(9, -1).sum(1).min().item() == 0 and len({int(c) for c in x[3].reshape(9, -1).sum(1)}) > 2
    want = by_hand(*x, plan.q_ptr.tolist(), plan.q_pairs.tolist(), plan.positive.tolist(), tau, gamma)
    got = torch_route(x, plan, tau, gamma, torch.float64)
    assert got[1].tolist() == [float(v) for v in want[1]]
    if layout == "vi9":
        assert want[1][0] == 2                             # queries 0 and 1 are counted; 2 has no positive, 3 no pair
    else:
        assert want[1][0] == 3
    for name, g, w in zip(("loss", "pair_score", "dpm", "dps", "dpe"), [got[0]] + got[2:], [want[0]] + list(want[2:])):
        assert g.shape == w.shape, name
        assert (g - w).abs().max().item() <= 1e-12 * max(w.abs().max().item(), 1.0), (name, (g - w).abs().max().item())
    assert want[2][4].item() == 0.0 and got[3][4].abs().max().item() == 0.0          # the pair without a valid cell
    assert got[3][~x[3]].abs().max().item() == 0.0
    assert want[3].abs().max().item() > 0 and want[4].abs().max().item() > 0 and want[5].abs().max().item() > 0
    # plain return value, and fp32 runs too
    pm, ps, pe, mm = x
    assert torch.equal(V().pair_rank_loss_torch(pm, ps, pe, mm, plan, tau, gamma), got[0].reshape(()))
    l32 = V().pair_rank_loss_torch(pm.float(), ps.float(), pe.float(), mm, plan, tau, gamma)
    assert l32.dtype == torch.float32 and abs(l32.item() - want[0].item()) <= 1e-4 * max(abs(want[0].item()), 1.0)


def test_degenerate_plans():
    api = V()
    x = synthetic(9, 3, seed=6, dtype=torch.float64)
    nobody = api.PairPlan(VI9, QI9, NV, NQ, "cpu", gt_video=[3, 3, 3, 3])        # video 3 has no pair: no query has a positive
    assert nobody.num_positive == 0
    got = torch_route(x, nobody, 0.1, 0.1, torch.float64)
    assert got[0].item() == 0.0 and got[1].tolist() == [0.0, 0.0]
    for g in got[3:]:
        assert g.abs().max().item() == 0.0
    # a query whose only pair is its positive: l_q = 0 and a hit; the other query has one positive and one negative
    lone = api.PairPlan([0, 1, 2], [0, 1, 1], 3, 2, "cpu", gt_video=[0, 1])
    y = tuple(t[:3] for t in x)
    loss, stats, s = api.pair_rank_loss_torch(*y, lone, 0.1, 0.1, return_stats=True)
    only_q1 = api.PairPlan.from_device(lone.video_index, lone.query_index, lone.v_ptr, lone.v_pairs, lone.q_ptr, lone.q_pairs, 3, 2,
                                       positive=torch.tensor([0, 1, 0], dtype=torch.int32))
    l1, st1, _ = api.pair_rank_loss_torch(*y, only_q1, 0.1, 0.1, return_stats=True)
    assert st1.tolist()[0] == 1.0 and stats.tolist()[0] == 2.0
    assert abs(loss.item() * 2 - l1.item()) <= 1e-15                             # query 0 adds l_q = 0 to the sum
    assert stats.tolist()[1] == 1.0 + st1.tolist()[1]                            # ... and a hit
    want = by_hand(*y, lone.q_ptr.tolist(), lone.q_pairs.tolist(), lone.positive.tolist(), 0.1, 0.1)
    assert abs(loss.item() - want[0].item()) <= 1e-14 and stats.tolist() == [float(v) for v in want[1]]


SEGMENTS, POSITIVES = [[0, 2, 4], [1, 3, 5]], [[2], [5]]                       # plan_of(6, 2)


def saturated_want(d, upstream=1.0):
    """(x, plan-free fp64 results) of saturated_pairs(d) from the definition in stable form on the constants: loss, dpm, dps, dpe.  With
    constant maps and ps = pe = 1 the cells of a pair share its gradient equally: dpm = coef_p / n on the n = 10 valid cells, and a row's
    dps (a column's dpe) is half the sum of its cells' dpm * c_p."""
    x, gamma, c = saturated_pairs(d, torch.float64)
    loss, coef = stable_rank_loss(c, SEGMENTS, POSITIVES, gamma)
    mm = x[3].double()
    dpm = upstream * torch.tensor(coef, dtype=torch.float64).reshape(-1, 1, 1) * mm / 10
    dps, dpe = 0.5 * (dpm * x[0]).sum(2), 0.5 * (dpm * x[0]).sum(1)
    return x, gamma, c, [torch.tensor(loss, dtype=torch.float64), dpm, dps, dpe]


def parent_form(c, gamma, dtype):
    """The formula this loss had before it shifted the positives' sum by their own maximum, on query 1 of saturated_pairs: both sums
    shifted by the segment's maximum.  Returns (l_q, the positive pair's coefficient)."""
    s = torch.tensor([c[p] for p in SEGMENTS[1]], dtype=dtype)
    x = torch.exp((s - s.max()) / gamma)
    zall, zpos = x.sum(), x[2:].sum()
    return torch.log(zall) - torch.log(zpos), (x[2] / zall - x[2] / zpos) / gamma


@pytest.mark.parametrize("d", sorted(RANK_DEPTHS))
def test_saturated_plans_hold_what_they_claim(d):
    """Each plan is in the regime it names, measured on the fp64 reference: query 0's own video is its best pair, query 1's lies d * gamma
    below its best negative, the pooled scores are the constants exactly, and the loss is (about) d / 2.  The restatement in fp64 equals the
    definition written out on the constants; in fp32 on the host it is finite and within fp32's reach of it, where the parent's formula --
    both sums shifted by the segment's maximum -- gives inf and NaN from d = 120 on (and inf even in fp64 at d = 800)."""
    x, gamma, c, want = saturated_want(d)
    plan = plan_of(6, 2)
    assert [plan.q_pairs.tolist()[a:b] for a, b in zip(plan.q_ptr.tolist(), plan.q_ptr.tolist()[1:])] == SEGMENTS
    assert [p for p in range(6) if plan.positive.tolist()[p]] == [2, 5]
    assert 4 <= plan.P <= 6 and plan.Q == 2 and x[0].shape == (6, 4, 4) and 0.0 < gamma < 0.0115
    assert torch.tensor(gamma, dtype=torch.float32).item() == gamma
    got = torch_route(x, plan, 0.1, gamma, torch.float64)
    assert got[2].tolist() == c and got[1].tolist() == [2.0, 1.0]
    s = got[2]
    assert s[2] == s[SEGMENTS[0]].max() and (s[SEGMENTS[1]].max() - s[5]).item() / gamma == d
    assert abs(got[0].item() - d / 2) <= 1e-7                                    # l_0 < exp(-48), l_1 = d + log(1 + exp(-16 or less))
    for name, g, w in zip(("loss", "dpm", "dps", "dpe"), [got[0]] + got[3:], want):
        assert torch.isfinite(g).all() and (g - w).abs().max().item() <= 1e-12 * w.abs().max().item(), (d, name)
    # fp32 on the host: the restatement holds the definition to a few roundings (every input and s / gamma are exact in fp32) ...
    got32 = torch_route(saturated_pairs(d)[0], plan, 0.1, gamma, torch.float32)
    for name, g, w in zip(("loss", "dpm", "dps", "dpe"), [got32[0]] + got32[3:], want):
        e = (g - w).abs().max().item() / w.abs().max().item()
        print(f"d = {d} {name}: e_torch32 on the host {e:.2e}")
        assert torch.isfinite(g).all() and e <= 1e-6, (d, name, e)
    # ... and the parent's formula does not
    l32, c32 = parent_form(c, gamma, torch.float32)
    l64, c64 = parent_form(c, gamma, torch.float64)
    if d >= 120:
        assert not torch.isfinite(l32) and not torch.isfinite(c32), (d, l32, c32)
    assert bool(torch.isfinite(l64)) == (d < 800)


def test_refusals():
    api = V()
    x = synthetic(9, 3, seed=7)
    plan = plan_of(9, 4)
    with pytest.raises(api._lib.SminHipError, match="no CPU fallback"):
        api.pair_rank_loss(*x, plan)
    api._lib.load_torch()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        torch.ops.smin_hip.smin_pair_rank_loss(*x, plan.q_ptr, plan.q_pairs, plan.positive, 0.1, 0.1)
    bare = api.PairPlan(VI9, QI9, NV, NQ, "cpu")
    for fn in (api.pair_rank_loss, api.pair_rank_loss_torch):
        with pytest.raises(ValueError, match="positive flags"):
            fn(*x, bare)
        with pytest.raises(ValueError, match="lists 9 pairs"):
            fn(x[0][:8], x[1][:8], x[2][:8], x[3][:8], plan)
        with pytest.raises(ValueError, match="tau"):
            fn(*x, plan, tau=0)
        with pytest.raises(ValueError, match="gamma"):
            fn(*x, plan, gamma=-1)
    with pytest.raises(ValueError, match="rank_weight"):
        api.train_epoch_pairs(None, None, [], rank_weight=-0.1)
    with pytest.raises(ValueError, match="rank_weight"):
        api.train_epoch_mined(None, None, [], 2, rank_weight=-0.1)
    with pytest.raises(ValueError, match="tau"):
        api.train_epoch_pairs(None, None, [], rank_weight=0.5, tau=0)


# ---------------------------------------------------------------- GPU
def kernel_route(x, plan, tau, gamma, dev, upstream=3.0):
    pm, ps, pe = (t.to(dev).requires_grad_(True) for t in x[:3])
    loss, stats, score = V().pair_rank_loss(pm, ps, pe, x[3].to(dev), plan, tau, gamma, return_stats=True)
    (upstream * loss).backward()
    torch.cuda.synchronize()
    return [loss, stats, score, pm.grad, ps.grad, pe.grad]


CASES = [(1, 1, 1), (9, 4, 3), (9, 4, 8), (19, 4, 17), (6, 2, 64), (2, 1, 260), ("mined", 3, 8)]


@pytest.mark.gpu
@pytest.mark.parametrize("tau,gamma", TEMPS)
@pytest.mark.parametrize("P,Q,L", CASES)
def test_kernels_against_fp64(dev, P, Q, L, tau, gamma):
    """e = max|x - x64| / max|x64| of the kernels and of pair_rank_loss_torch in fp32, both against pair_rank_loss_torch in fp64 on the
    device, for the loss, pair_score, dpm, dps, dpe with the upstream gradient 3; gate e_kernel <= 32 * e_torch32 + 1e-6.  A quantity
    whose fp64 value is identically 0 ((1, 1, 1): the lone positive pair) must come out exactly 0.

    Measured on an MI355X, e_kernel / e_torch32, the worst of dpm, dps, dpe and in brackets the loss (INTEGRATION.md 3q has the table):
        (P, Q, L)      (tau, gamma) = (1, 1)                   (0.1, 0.1)                              (0.01, 0.05)
        (9, 4, 3)      1.2e-7 / 1.1e-7 (1.2e-7 / 1.2e-7)       2.0e-7 / 2.0e-7 (2.2e-8 / 1.3e-7)       1.3e-7 / 1.3e-7 (4.1e-8 / 3.4e-8)
        (9, 4, 8)      1.6e-7 / 1.1e-7 (2.6e-8 / 2.6e-8)       3.5e-7 / 5.0e-7 (9.1e-8 / 1.1e-7)       1.6e-6 / 7.0e-7 (9.2e-7 / 3.7e-7)
        (19, 4, 17)    1.5e-7 / 5.7e-8 (1.9e-9 / 1.9e-9)       1.1e-7 / 1.9e-7 (1.2e-8 / 1.2e-8)       3.0e-7 / 2.0e-7 (1.2e-7 / 6.9e-8)
        (6, 2, 64)     1.7e-7 / 1.2e-7 (7.5e-8 / 7.5e-8)       4.9e-7 / 2.1e-7 (6.5e-8 / 6.5e-8)       2.4e-6 / 2.5e-6 (1.7e-7 / 1.7e-7)
        (2, 1, 260)    2.8e-7 / 1.4e-7 (1.8e-7 / 8.3e-8)       5.9e-7 / 3.2e-7 (1.7e-7 / 1.7e-8)       1.2e-6 / 1.3e-6 (7.8e-8 / 7.1e-7)
        mined, L = 8   9.3e-8 / 2.3e-7 (5.0e-8 / 5.0e-8)       3.4e-7 / 4.1e-7 (1.3e-7 / 2.3e-7)       7.5e-7 / 6.4e-7 (2.0e-7 / 2.0e-7)
    (1, 1, 1): loss and gradients identically 0, exactly 0 on the device; pair_score 1.1e-7 / 1.1e-7.  pair_score elsewhere: 1.8e-8 to
    8.5e-7 on both sides.  The largest e_kernel / e_torch32 of any quantity: 10.4.  (Figures of the kernel and the restatement that
    shift each sum by its own maximum.)"""
    if P == "mined":
        plan, P = mined_plan(dev), 9
    else:
        plan = plan_of(P, Q, dev)
    x = synthetic(P, L, seed=100 * P + L)
    want = torch_route(x, plan, tau, gamma, torch.float64, dev, upstream=3.0)
    ref32 = torch_route(x, plan, tau, gamma, torch.float32, dev, upstream=3.0)
    got = kernel_route(x, plan, tau, gamma, dev)
    assert got[0].dtype == torch.float32 and got[0].shape == () and got[1].shape == (2,) and got[2].shape == (P,)
    assert not got[1].requires_grad and not got[2].requires_grad
    assert got[1].cpu().tolist() == want[1].tolist(), (got[1].tolist(), want[1].tolist())
    for k, name in ((0, "loss"), (2, "pair_score"), (3, "dpm"), (4, "dps"), (5, "dpe")):
        g, r, w = got[k].detach().cpu().double(), ref32[k], want[k]
        assert g.shape == w.shape and torch.isfinite(g).all(), name
        scale = w.abs().max().item()
        if scale == 0.0:
            print(f"(P, Q, L) = ({P}, {Q}, {L}) tau {tau} gamma {gamma} {name}: identically zero")
            assert g.abs().max().item() == 0.0, name
            continue
        e_k, e_t = (g - w).abs().max().item() / scale, (r - w).abs().max().item() / scale
        print(f"(P, Q, L) = ({P}, {Q}, {L}) tau {tau} gamma {gamma} {name}: e_kernel {e_k:.2e}  e_torch32 {e_t:.2e}")
        assert e_k <= 32 * e_t + 1e-6, (name, e_k, e_t)
    if not x[3].all():
        assert got[3].cpu()[~x[3]].abs().max().item() == 0.0


@pytest.mark.gpu
@pytest.mark.parametrize("d", sorted(RANK_DEPTHS))
def test_kernels_at_small_gamma(dev, d):
    """saturated_pairs(d): the hard query's own video d * gamma below its best negative, d in {50, 95, 120, 800}.  Every output finite,
    masked cells of dpm exactly 0, stats the fp64 reference's, and the project's gate for the loss, pair_score, dpm, dps and dpe against
    the definition in stable form in fp64 (written out on the constants: saturated_want; pair_rank_loss_torch in fp64 equals it to 1e-12
    on the host), e_torch32 from pair_rank_loss_torch in fp32 on the device, the upstream gradient 3.  With both sums shifted by the
    segment's maximum the kernel returned loss inf and NaN gradients from d = 120 on.

    Measured on an MI355X: INTEGRATION.md, "Saturated inputs"."""
    _, gamma, c, want = saturated_want(d, upstream=3.0)
    x = saturated_pairs(d)[0]
    plan = plan_of(6, 2, dev)
    ref32 = torch_route(x, plan, 0.1, gamma, torch.float32, dev, upstream=3.0)
    got = kernel_route(x, plan, 0.1, gamma, dev)
    assert all(torch.isfinite(t).all() for t in got)
    assert got[1].cpu().tolist() == [2.0, 1.0] and got[2].cpu().tolist() == c
    for name, g, w, r in zip(("loss", "dpm", "dps", "dpe"), [got[0]] + got[3:], want, [ref32[0]] + ref32[3:]):
        gate(f"pair_rank d = {d} {name}", g, w, r)
    assert bits(got[3].cpu()[~x[3]]).eq(0).all()


def abi_bwd(dev, a, fill=float("nan"), **kw):
    L_ = V()._lib
    lib = L_.load()
    P, L = a["ps"].shape
    full = lambda *shape: torch.full(shape, fill, dtype=torch.float32, device=dev)
    b = dict(a, dloss=torch.tensor([3.0], device=dev), dpm=full(P, L, L), dps=full(P, L), dpe=full(P, L))
    b.update(kw)
    p = lambda k: L_.ptr(b[k])
    rc = lib.smin_pair_rank_bwd(L_.stream(), p("dloss"), p("stats"), p("coef"), p("pool"), p("pm"), p("ps"), p("pe"), p("mm"), b["P"], b["L"], b["tau"],
                                p("dpm"), p("dps"), p("dpe"))
    torch.cuda.synchronize()
    return rc, [b["dpm"], b["dps"], b["dpe"]]


@pytest.mark.gpu
def test_every_output_is_written_and_repeats(dev):
    plan = plan_of(19, 4, dev)
    x = synthetic(19, 17, seed=3)
    rc, outs, a = abi_call(dev, x, plan)
    assert rc == 0
    for k, t in outs.items():
        assert torch.isfinite(t).all(), k
    rc, grads = abi_bwd(dev, a)
    assert rc == 0
    for t in grads:
        assert torch.isfinite(t).all()
    mm = x[3].to(dev)
    assert bits(grads[0][~mm]).eq(0).all()                                       # masked cells: +0.0
    dead_rows, dead_cols = ~mm.any(dim=2), ~mm.any(dim=1)
    assert dead_rows.any() and dead_cols.any() and not mm[19 // 2].any()
    assert bits(grads[1][dead_rows]).eq(0).all() and bits(grads[2][dead_cols]).eq(0).all()
    assert grads[0].abs().max().item() > 0 and grads[1].abs().max().item() > 0 and grads[2].abs().max().item() > 0
    rc2, outs2, a2 = abi_call(dev, x, plan)
    _, grads2 = abi_bwd(dev, a2)
    assert rc2 == 0
    for k in outs:
        assert torch.equal(bits(outs[k]), bits(outs2[k])), k
    for g1, g2 in zip(grads, grads2):
        assert torch.equal(bits(g1), bits(g2))
    # the operator's values are the C ABI's
    got = kernel_route(x, plan, 0.1, 0.1, dev)
    assert torch.equal(bits(got[0].reshape(1)), bits(outs["loss"])) and torch.equal(bits(got[1]), bits(outs["stats"]))
    assert torch.equal(bits(got[2]), bits(outs["score"]))
    for g1, g2 in zip(got[3:], grads):
        assert torch.equal(bits(g1), bits(g2))
    # a plan in which no query has a positive: loss 0, zero gradients over the sentinel
    nobody = V().PairPlan(*p19_lists(), NV, NQ, dev, gt_video=[3, 3, 3, 3])
    nobody.positive.zero_()
    rc, outs, a = abi_call(dev, x, nobody)
    rc_b, grads = abi_bwd(dev, a)
    assert rc == 0 and rc_b == 0 and outs["loss"].item() == 0.0 and outs["stats"].tolist() == [0.0, 0.0]
    for t in grads:
        assert t.abs().max().item() == 0.0


@pytest.mark.gpu
def test_both_routes_give_the_same_bits(dev):
    tr = V().training
    plan = plan_of(9, 4, dev)
    x = synthetic(9, 8, seed=4)
    assert tr.NATIVE_LOSS is True
    ext = kernel_route(x, plan, 0.1, 0.1, dev)
    tr.NATIVE_LOSS = False
    try:
        cty = kernel_route(x, plan, 0.1, 0.1, dev)
    finally:
        tr.NATIVE_LOSS = True
    for name, a, b in zip(("loss", "stats", "pair_score", "dpm", "dps", "dpe"), ext, cty):
        assert a.shape == b.shape and torch.equal(bits(a), bits(b)), name
    assert not cty[1].requires_grad and not cty[2].requires_grad


@pytest.mark.gpu
def test_rejections_leave_the_outputs_untouched(dev):
    plan = plan_of(9, 4, dev)
    x = synthetic(9, 8, seed=4)
    nbytes = V()._lib.load().smin_pair_rank_ws_bytes(9, 4, 8)
    assert nbytes == 4 * 16
    bad = [dict(P=0), dict(Q=0), dict(L=0), dict(P=-1), dict(tau=0.0), dict(tau=-1.0), dict(tau=float("nan")), dict(tau=float("inf")), dict(gamma=0.0),
           dict(gamma=-1.0), dict(gamma=float("nan")), dict(gamma=float("inf")), dict(ws_bytes=nbytes - 1), dict(ws=None)]
    bad += [{k: None} for k in ("pm", "ps", "pe", "mm", "q_ptr", "q_pairs", "positive")]
    for kw in bad:
        rc, outs, _ = abi_call(dev, x, plan, fill=-7.0, **kw)
        assert rc != 0, kw
        for k, t in outs.items():
            assert t.eq(-7.0).all(), (kw, k)
    for hole in ("loss", "stats", "score", "coef", "pool"):
        rc, outs, _ = abi_call(dev, x, plan, fill=-7.0, **{hole: None})
        assert rc != 0, hole
        for k, t in outs.items():
            assert k == hole or t.eq(-7.0).all(), (hole, k)
    rc, _, a = abi_call(dev, x, plan)
    assert rc == 0
    for kw in [dict(P=0), dict(L=0), dict(tau=0.0), dict(tau=float("nan"))] + [{k: None} for k in ("dloss", "stats", "coef", "pool", "pm", "ps", "pe", "mm")]:
        rc, grads = abi_bwd(dev, a, fill=-7.0, **kw)
        assert rc != 0, kw
        for t in grads:
            assert t.eq(-7.0).all(), kw
    for hole in ("dpm", "dps", "dpe"):
        rc, _ = abi_bwd(dev, a, fill=-7.0, **{hole: None})
        assert rc != 0, hole


# ---------------------------------------------------------------- through the model
def oracle_grads(w, vi, qi, weight=0.5):
    """the fp64 oracle with autograd on the expanded pairs, loss_fn + weight * pair_rank_loss_torch in fp64: {name: gradient}"""
    from oracle import smin_oracle as O
    api = V()
    sd = {k: v.double().requires_grad_(True) for k, v in w["sd"].items()}
    xs = expand(w["vid"], w["qry"], vi, qi)
    xs[0], xs[2] = xs[0].double(), xs[2].double()
    out = O.smin_forward(sd, dict(T=16, L=8, C=4), *xs)
    t = api.pair_targets(w["vid"], {k: (v.double() if v.is_floating_point() else v) for k, v in w["tg"].items()}, vi, qi, GT_VIDEO)
    plan = api.PairPlan(vi, qi, NV, NQ, "cpu", gt_video=GT_VIDEO)
    loss = loss_of(O.loss_fn, out, t) + weight * api.pair_rank_loss_torch(out[0], out[1], out[2], t["moment_mask"], plan)
    loss.backward()
    return {k: v.grad for k, v in sd.items()}


def model_grads(w, plan, rank, weight=0.5):
    api, m = V(), w["m"]
    for p in m.parameters():
        p.grad = None
    out = m.forward_pairs(*pair_args(w["vid_d"], w["qry_d"]), None, None, plan=plan)
    t = api.pair_targets(w["vid_d"], w["tg_d"], None, None, None, plan=plan)
    loss = loss_of(api.loss_fn, out, t) + weight * rank(out[0], out[1], out[2], t["moment_mask"], plan)
    loss.backward()
    torch.cuda.synchronize()
    return {k: p.grad.detach().clone() for k, p in m.named_parameters()}


def gate_model(w, plan, vi, qi, tag):
    api = V()
    g64 = oracle_grads(w, vi, qi)
    g_new = model_grads(w, plan, api.pair_rank_loss)
    g_ref = model_grads(w, plan, api.pair_rank_loss_torch)
    assert set(g_new) == set(g64) == set(g_ref)
    worst, zero = [0.0, 0.0], 0
    for k, r in g64.items():
        scale = r.abs().max().item()
        a, b = g_new[k].cpu().double(), g_ref[k].cpu().double()
        if scale < 1e-9:                               # the key biases the softmax is invariant to (test_pair_training's rule)
            assert k.endswith("W_k.bias"), k
            assert a.abs().max().item() <= 2 * b.abs().max().item() + 1e-9, k
            zero += 1
            continue
        e_new, e_ref = (a - r).abs().max().item() / scale, (b - r).abs().max().item() / scale
        worst = [max(worst[0], e_new), max(worst[1], e_ref)]
        assert e_new <= 2 * e_ref + 1e-6, (k, e_new, e_ref)
    assert zero == 4
    print(api.get_gemm_mode(), tag, f"P = {len(vi)}", f"worst e_new {worst[0]:.2e}  worst e_ref32 {worst[1]:.2e}")


@pytest.mark.gpu
def test_model_gradients_on_the_vi9_plan(dev, world):
    """Measured on an MI355X, the worst parameter tensor: e_new 2.22e-06 / e_ref32 2.39e-06 (f32), 6.27e-06 / 6.10e-06 (f32e)."""
    plan = V().PairPlan(VI9, QI9, NV, NQ, dev, gt_video=GT_VIDEO)
    gate_model(world, plan, VI9, QI9, "vi9")


@pytest.mark.gpu
def test_model_gradients_on_a_mined_plan(dev, world):
    """Measured on an MI355X, the worst parameter tensor: e_new 2.62e-06 / e_ref32 2.55e-06 (f32), 2.47e-06 / 2.46e-06 (f32e)."""
    m, vd, qd = world["m"], world["vid_d"], world["qry_d"]
    with torch.no_grad():
        videos = m.encode_videos(vd["video_features"], vd["video_mask"], vd["length_mask"], vd["moment_mask"])
        queries = m.encode_queries(qd["query_features"], qd["query_mask"])
        plan = m.mine_pairs(videos, queries, GT_VIDEO, 2)
    vi, qi = plan.video_index.tolist(), plan.query_index.tolist()
    assert plan.P == 12 and plan.vi is None and vi[::3] == GT_VIDEO
    gate_model(world, plan, vi, qi, "mined")


# ---------------------------------------------------------------- the loops
@pytest.mark.gpu
def test_train_epoch_pairs_with_the_term(dev, world):
    api = V()
    Probe = probe(api)
    g = full_group(dev)
    plan = api.PairPlan(VI9, QI9, NV, NQ, dev, gt_video=GT_VIDEO)
    twin, _ = tiny_model(dev)
    twin.train()
    want = hand_step(api, twin, g, plan, 0.5).item()
    plain = hand_step(api, twin, g, plan, None).item()
    assert want > plain                                                         # the term is positive here: query 0 and 1 have negatives
    m, _ = tiny_model(dev)
    opt = api.FusedAdam(m.parameters(), lr=1e-3)
    api.train_epoch_pairs(m, opt, [g], Probe(device=dev), rank_weight=0.5)       # (first use outside the checked region)
    m.load_state_dict(world["sd"])
    opt = api.FusedAdam(m.parameters(), lr=1e-3)
    Probe.reads = 0
    loss, metrics = checked(lambda: api.train_epoch_pairs(m, opt, [g], Probe(device=dev), rank_weight=0.5))
    print("train_epoch_pairs rank_weight 0.5: loss", loss, "by hand", want, "loss_fn alone", plain)
    assert Probe.reads == 1 and m.known_cell_count is None
    assert abs(loss - want) <= 1e-6 * abs(want) and loss == metrics["loss"]
    assert int(api._lib.load_torch().layout_status(dev)[0]) == 0
    # rank_weight 0.0, or omitted: the parent's step, bit for bit
    opt_t = api.FusedAdam(twin.parameters(), lr=1e-3)
    hand_step(api, twin, g, plan, None, opt_t)
    for kw in (dict(), dict(rank_weight=0.0)):
        m.load_state_dict(world["sd"])
        opt = api.FusedAdam(m.parameters(), lr=1e-3)
        api.train_epoch_pairs(m, opt, [g], Probe(device=dev), **kw)
        same_parameters(m, twin)


@pytest.mark.gpu
def test_train_epoch_mined_with_the_term(dev, world):
    api = V()
    Probe = probe(api)
    g = full_group(dev, lists=False)
    twin, _ = tiny_model(dev)
    twin.train()
    with torch.no_grad():
        videos = twin.encode_videos(g["video_features"], g["video_mask"], g["length_mask"], g["moment_mask"], cell_counts=g["cell_counts"])
        queries = twin.encode_queries(g["query_features"], g["query_mask"])
        plan = twin.mine_pairs(videos, queries, GT_VIDEO, 2)
    want = hand_step(api, twin, g, plan, 0.5).item()
    m, _ = tiny_model(dev)
    opt = api.FusedAdam(m.parameters(), lr=1e-3)
    api.train_epoch_mined(m, opt, [g], 2, meter=Probe(device=dev), rank_weight=0.5)
    m.load_state_dict(world["sd"])
    opt = api.FusedAdam(m.parameters(), lr=1e-3)
    Probe.reads = 0
    loss, metrics = checked(lambda: api.train_epoch_mined(m, opt, [g], 2, meter=Probe(device=dev), rank_weight=0.5))
    print("train_epoch_mined rank_weight 0.5: loss", loss, "by hand", want)
    assert Probe.reads == 1 and m.known_cell_count is None and metrics["num_samples"] == NQ
    assert abs(loss - want) <= 1e-6 * abs(want) and loss == metrics["loss"]
    assert int(api._lib.load_torch().layout_status(dev)[0]) == 0
    opt_t = api.FusedAdam(twin.parameters(), lr=1e-3)
    hand_step(api, twin, g, plan, None, opt_t)
    for kw in (dict(), dict(rank_weight=0.0)):
        m.load_state_dict(world["sd"])
        opt = api.FusedAdam(m.parameters(), lr=1e-3)
        api.train_epoch_mined(m, opt, [g], 2, meter=Probe(device=dev), **kw)
        same_parameters(m, twin)
