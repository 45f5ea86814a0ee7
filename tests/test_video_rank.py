"""Video ranking by the pooled pair score and its use in corpus search: csrc/video_rank.hip smin_pair_pool /
smin_group_pool / smin_video_rank / smin_moment_reweight, moments.pair_pool / group_pool / rank_videos / reweight_moments and their
``*_torch`` restatements, SMIN.rank_videos, the video-level options of SMIN.search / search_windows / pair_scores / mine_pairs,
meter.VideoRankMeter and the options of training.test_model_corpus.

Host: the C ABI surface; the restatements in fp64 against hand-written Python loops (segments of 0, 1 and 5 pairs, a tie between two
videos, a pair without cells, a gt_video that is not listed, alpha 0 and 7.5, max_videos 0, 1, 2, 99); the refusals.
GPU: smin_pair_pool's score against smin_pair_rank_fwd's pair_score bit for bit; pool, cells, the group scores and the weights
against the fp64 restatement, gated by the error of the fp32 restatement on the same device (e_kernel <= 32 * e_torch32 + 1e-6, e =
max|x - x64| / max|x64|, the gate of test_pair_rank_loss); smin_video_rank against rank_videos_torch bit for bit, a segment longer than
the kernel's LDS tile of VR_TILE = 2048 order words included; search at neutral settings against today's search bit for bit; the
weighted, cut search against its restatement on equal numbers; mining by the pooled score; the meter and the test loop with one host
read; the rejections through the C ABI."""
import math
import os
import re

import numpy as np
import pytest
import torch

from tests.support import corpora as WS
from tests.support.device import dev  # noqa: F401  (the module's device fixture)
from tests.support.device import vml as V
from tests.support.compare import bits, gate, same
from tests.support.corpora import (
    corpus_inputs, synthetic, tied_maps, tied_pool_by_hand, tiny_model, window_host_banks, DURATION_TENSOR, GT_VIDEO, SEARCH_KEYS)
from tests.support.references import abi_call

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"smin_pair_pool": 11, "smin_group_pool": 9, "smin_video_rank": 16, "smin_moment_reweight": 10}
VR_TILE = 2048                                         # csrc/video_rank.hip: order words staged in LDS at a time
TAUS = [1.0, 0.1, 0.01]


# ---------------------------------------------------------------- host
def test_surface():
    text = open(os.path.join(ROOT, "include", "smin_hip.h")).read()
    A = V()
    lib = A._lib.load()
    for name, nargs in NAMES.items():
        assert re.search(r"\bint\s+" + name + r"\s*\(", text), name
        assert len(A._lib.SIGNATURES[name]) == nargs and hasattr(lib, name), name
    assert "#define SMIN_HIP_ABI_VERSION 2" in text and lib.smin_abi_version() == 2
    src = open(os.path.join(ROOT, "video-moment-localization_amd", "csrc", "video_rank.hip")).read()
    assert f"VR_TILE = {VR_TILE};" in src
    for name in ("pair_pool", "group_pool", "rank_videos", "reweight_moments"):
        assert callable(getattr(A, name)) and callable(getattr(A, name + "_torch")), name
    assert hasattr(A, "VideoRankMeter") and hasattr(A.SMIN, "rank_videos")


def hand_case():
    """Q = 3 queries with 0, 1 and 5 pairs (P = 6).  Query 2: videos 4 and 1 tie on the score 0.5 (video 1 goes first), video 3 has no
    cell, +0 and -0 are both there (equal, so the lower video 0 goes first).  gt_video: query 0 has no pair, query 1's is its only pair,
    query 2's (video 9) is not listed."""
    score = torch.tensor([0.25, 0.5, -0.0, 0.9, 0.5, 0.0], dtype=torch.float64)
    cells = torch.tensor([3.0, 36.0, 1.0, 0.0, 2.0, 5.0], dtype=torch.float64)
    video = torch.tensor([2, 4, 6, 3, 1, 0], dtype=torch.int32)
    ptr = torch.tensor([0, 0, 1, 6], dtype=torch.int32)
    gt = torch.tensor([1, 2, 9], dtype=torch.int32)
    return score, cells, video, ptr, gt


def rank_by_hand(score, cells, video, ptr, gt, n, alpha):
    s, c, v, pp, g = score.tolist(), cells.tolist(), video.tolist(), ptr.tolist(), gt.tolist()
    P, Q = len(s), len(pp) - 1
    rank, weight = [-1] * P, [0.0] * P
    out_v, out_s = [[-1] * n for _ in range(Q)], [[0.0] * n for _ in range(Q)]
    count, gt_rank = [0] * Q, [-1] * Q
    for q in range(Q):
        seg = [e for e in range(pp[q], pp[q + 1]) if c[e] > 0]
        for e in seg:
            ahead = 0
            for o in seg:                                  # by counting: a higher score, or the same score and a lower video, or both the same and earlier
                ahead += s[o] > s[e] or (s[o] == s[e] and (v[o] < v[e] or (v[o] == v[e] and o < e)))
            rank[e] = ahead
            weight[e] = math.exp(alpha * (s[e] - max(s[o] for o in seg)))
            if ahead < n:
                out_v[q][ahead], out_s[q][ahead] = v[e], s[e]
            if v[e] == g[q]:
                gt_rank[q] = ahead
        count[q] = min(len(seg), n)
    return out_v, out_s, count, rank, weight, gt_rank


@pytest.mark.parametrize("alpha", [0.0, 7.5, -2.0])
@pytest.mark.parametrize("n", [1, 3, 64])
def test_rank_videos_torch_by_hand(n, alpha):
    A = V()
    case = hand_case()
    want = rank_by_hand(*case, n, alpha)
    got = A.rank_videos_torch(*case[:4], n=n, alpha=alpha, gt_video=case[4])
    assert got["video"].tolist() == want[0] and got["count"].tolist() == want[2] and got["pair_rank"].tolist() == want[3]
    assert got["gt_rank"].tolist() == want[5] == [-1, 0, -1]
    assert want[3] == [0, 1, 3, -1, 0, 2]                  # the tie 0.5 / 0.5: video 1 before video 4; -0 == +0: video 0 before video 6
    assert got["score"].dtype == torch.float64 and got["weight"].dtype == torch.float64
    assert (got["score"] - torch.tensor(want[1], dtype=torch.float64)).abs().max().item() == 0.0
    assert (got["weight"] - torch.tensor(want[4], dtype=torch.float64)).abs().max().item() <= 1e-15
    if alpha == 0.0:
        assert got["weight"].tolist() == [1.0, 1.0, 1.0, 0.0, 1.0, 1.0]
    assert A.rank_videos_torch(*case[:4], n=n, alpha=alpha)["gt_rank"].tolist() == [-1, -1, -1]      # no gt_video
    # the moment lists: weighted, and cut to the best max_videos videos of each query
    k = 3
    lists = torch.arange(1.0, 6 * k + 1, dtype=torch.float64).reshape(6, k) / 7
    cnt = torch.tensor([3, 2, 0, 1, 3, 3], dtype=torch.int32)
    for cut in (0, 1, 2, 99):
        sc, cn = A.reweight_moments_torch(lists, cnt, got["pair_rank"], got["weight"], cut)
        for p in range(6):
            keep = cut == 0 or 0 <= want[3][p] < cut
            assert cn[p].item() == (cnt[p].item() if keep else 0), (cut, p)
            for j in range(k):
                assert sc[p, j].item() == lists[p, j].item() * got["weight"][p].item()
    assert torch.equal(A.reweight_moments_torch(lists, cnt, got["pair_rank"], got["weight"], None)[1], cnt)


def test_pool_restatements_by_hand():
    A = V()
    P, L, tau = 7, 5, 0.1
    pm, ps, pe, mm = synthetic(P, L, seed=2, dtype=torch.float64)
    score, pool, cells = A.pair_pool_torch(pm, ps, pe, mm, tau)
    assert score.dtype == torch.float64 and tuple(pool.shape) == (P, 2) and not mm[P // 2].any()
    f = [[[pm[p, i, j].item() * math.sqrt(max(ps[p, i].item(), 1e-12)) * math.sqrt(max(pe[p, j].item(), 1e-12)) for j in range(L)]
          for i in range(L)] for p in range(P)]
    want = []
    for p in range(P):
        vals = [f[p][i][j] for i in range(L) for j in range(L) if mm[p, i, j]]
        if not vals:
            want.append((0.0, 0.0, 0.0, 0.0))
            continue
        top = max(vals)
        z = sum(math.exp((x - top) / tau) for x in vals)
        want.append((top + tau * math.log(z / len(vals)), top, z, float(len(vals))))
    for p in range(P):
        got = (score[p].item(), pool[p, 0].item(), pool[p, 1].item(), cells[p].item())
        assert all(abs(g - w) <= 1e-12 * max(abs(w), 1.0) for g, w in zip(got, want[p])), (p, got, want[p])
    assert want[P // 2] == (0.0, 0.0, 0.0, 0.0) and cells[P // 2].item() == 0.0
    # groups of 0, 1, 2 and 4 windows; window 3 (no cell) lies in the last: the group's score is the log-mean-exp over all its cells
    gp = torch.tensor([0, 0, 1, 3, 7], dtype=torch.int32)
    gs, gc = A.group_pool_torch(pool, cells, gp, tau)
    assert gs[0].item() == 0.0 and gc.tolist() == [0.0, cells[0].item(), (cells[1] + cells[2]).item(), cells[3:].sum().item()]
    for g in range(1, 4):
        vals = [f[p][i][j] for p in range(int(gp[g]), int(gp[g + 1])) for i in range(L) for j in range(L) if mm[p, i, j]]
        top = max(vals)
        want_g = top + tau * math.log(sum(math.exp((x - top) / tau) for x in vals) / len(vals))
        assert abs(gs[g].item() - want_g) <= 1e-12, (g, gs[g].item(), want_g)
    assert abs(gs[1].item() - score[0].item()) <= 1e-14
    none = A.group_pool_torch(pool, torch.zeros_like(cells), gp, tau)
    assert none[0].eq(0).all() and none[1].eq(0).all()


SAT_TAUS = [1e-3, 1e-4]
SAT_POOL = [(7, 5), (5, 33)]                           # the smallest case with more than one pair, and the strided walk
SAT_ALPHAS = [50.0, 500.0, -500.0]
GROUP_PTR = [0, 0, 1, 3, 7]                            # test_group_pool's groups


@pytest.mark.parametrize("tau", SAT_TAUS)
@pytest.mark.parametrize("P,L", SAT_POOL + [(7, 8)])
def test_tied_maps_hold_what_they_claim(P, L, tau):
    """On the fp64 restatement: every cell below a pair's maximum lies at least 125 temperatures under it (its exponential is below
    1e-54, and exactly 0 in fp32), some pair has several cells at the maximum and some pair has one, and the pooled score is
    m + tau * log(k / n) with k the number of cells at the maximum; a group's score is the same over all its windows' cells."""
    A = V()
    x = tied_maps(P, L, seed=21 if L == 8 else 100 * P + L, dtype=torch.float64)
    score, top, ties, cells = tied_pool_by_hand(x[0], x[3], tau)
    for p in range(P):
        below = [v for v in x[0][p][x[3][p]].tolist() if v != top[p]]
        assert not below or (top[p] - max(below)) / tau >= 125.0
    assert max(ties) > 1 and len(set(top)) > 2 and any(0 < k < n for k, n in zip(ties, cells)) and 0 in cells
    got = A.pair_pool_torch(*x, tau=tau)
    assert got[2].tolist() == [float(n) for n in cells] and got[1][:, 0].tolist() == top
    assert (got[1][:, 1] - torch.tensor(ties, dtype=torch.float64)).abs().max().item() <= 1e-50
    assert (got[0] - torch.tensor(score, dtype=torch.float64)).abs().max().item() <= 1e-15
    if L == 8:
        gs, gc = A.group_pool_torch(got[1], got[2], torch.tensor(GROUP_PTR, dtype=torch.int32), tau)
        for g, (a, b) in enumerate(zip(GROUP_PTR, GROUP_PTR[1:])):
            n = sum(cells[a:b])
            m = max([top[w] for w in range(a, b) if cells[w]], default=0.0)
            k = sum(ties[w] for w in range(a, b) if cells[w] and top[w] == m)
            assert gc[g].item() == n and abs(gs[g].item() - (m + tau * math.log(k / n) if n else 0.0)) <= 1e-15, g
        assert len({top[w] for w in range(3, 7) if cells[w]}) > 1                  # the last group's windows do not share a maximum


def weight_case(alpha):
    """rank_case(3, 5)'s lists under pair scores in [0, 1] on a grid of 1/64: over the whole interval for alpha > 0, within 1/8 of 0.875 for
    alpha < 0 (a weight exp(|alpha| * gap) leaves fp32 at a gap of 88.7 / |alpha|: 0.177 at -500)"""
    _, cells, video, ptr, gt = rank_case(3, 5, seed=7 * 3 + 5)
    g = torch.Generator().manual_seed(int(abs(alpha)))
    steps = torch.randint(0, 65 if alpha > 0 else 9, (cells.shape[0],), generator=g)
    if alpha > 0:
        steps[ptr[:-1].long()] = torch.tensor([0, 1, 64])                            # a best pair, its neighbour on the grid, the far end
    return (64 - steps if alpha > 0 else 56 - steps).float() / 64, cells, video, ptr, gt


@pytest.mark.parametrize("alpha", SAT_ALPHAS)
def test_weight_cases_hold_what_they_claim(alpha):
    A = V()
    score, cells, video, ptr, gt = weight_case(alpha)
    assert 0.0 <= score.min().item() and score.max().item() <= 1.0
    r = A.rank_videos_torch(score.double(), cells.double(), video, ptr, n=5, alpha=alpha)
    w, listed = r["weight"], r["pair_rank"] >= 0
    assert listed.sum().item() >= 9 and not listed.all() and torch.isfinite(w).all()
    assert all(w[listed & (r["pair_rank"] == 0)].tolist()) and (w[listed & (r["pair_rank"] == 0)] == 1.0).all()
    if alpha > 0:
        assert w.max().item() == 1.0 and (w[listed] < 1.0).any()
        if alpha == 500.0:
            assert (w[listed] < 1e-45).any() and ((w[listed] > 1e-30) & (w[listed] < 1.0)).any()      # gone in fp32, and alive
        else:
            assert w[listed].min().item() > 1e-30
    else:
        assert w[listed].min().item() == 1.0 and 1e10 < w.max().item() < 3e38                         # large, and inside fp32


def test_refusals():
    A = V()
    err = A._lib.SminHipError
    case = hand_case()
    f32 = [case[0].float(), case[1].float(), case[2], case[3]]
    for n in (0, 65, 2.0, True):
        with pytest.raises(ValueError, match="1 <= n <= 64"):
            A.rank_videos_torch(*f32, n=n)
    for alpha in (float("nan"), float("inf"), float("-inf"), "7.5", True):
        with pytest.raises(ValueError, match="video weight"):
            A.rank_videos_torch(*f32, alpha=alpha)
    x = synthetic(3, 4, seed=1)
    for tau in (0, -0.1, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="tau"):
            A.pair_pool_torch(*x, tau=tau)
        with pytest.raises(ValueError, match="tau"):
            A.group_pool_torch(torch.zeros(2, 2), torch.zeros(2), torch.tensor([0, 2]), tau=tau)
    with pytest.raises(ValueError, match="max_videos"):
        A.reweight_moments_torch(torch.zeros(2, 3), torch.zeros(2, dtype=torch.int32), torch.zeros(2, dtype=torch.int32), torch.zeros(2), -1)
    # the HIP names fail loudly on CPU tensors
    with pytest.raises(err, match="no CPU fallback"):
        A.pair_pool(*x)
    with pytest.raises(err, match="no CPU fallback"):
        A.group_pool(torch.zeros(2, 2), torch.zeros(2), torch.tensor([0, 2]))
    with pytest.raises(err, match="no CPU fallback"):
        A.rank_videos(*f32)
    with pytest.raises(err, match="no CPU fallback"):
        A.reweight_moments(torch.zeros(2, 3), torch.zeros(2, dtype=torch.int32), torch.zeros(2, dtype=torch.int32), torch.zeros(2))
    m, _ = tiny_model()
    wb, qb = window_host_banks()
    for kw in (dict(video_weight=float("nan")), dict(video_weight=0.5, tau=0), dict(max_videos=0), dict(video_weight=0.5, n_videos=65),
               dict(video_weight=0.5, gt_video=[0, 1])):
        with pytest.raises(ValueError, match="video weight|tau|max_videos|n_videos|gt_video"):
            m.search_windows(wb, qb, **kw)
    with pytest.raises(ValueError, match="must be an integer"):
        m.rank_videos(wb, qb, n=0)
    for k in (None, "x", 0, 2.0):                                                      # k is checked before the video-level options read it
        for f in (m.search, m.search_windows):
            with pytest.raises(ValueError, match="must be an integer"):
                f(wb, qb, k=k, video_weight=0.5)
    with pytest.raises(err, match="no CPU fallback"):
        m.rank_videos(wb, qb)
    with pytest.raises(err, match="no CPU fallback"):
        m.search_windows(wb, qb, video_weight=0.5)
    with pytest.raises(ValueError, match="pool must be"):
        m.pair_scores(None, None, pool="max")
    # more than one shard with the video-level options
    for kw in (dict(video_weight=7.5), dict(max_videos=2), dict(video_meter=A.VideoRankMeter(device="cpu"))):
        with pytest.raises(ValueError, match="one shard"):
            A.test_model_corpus(None, [dict(), dict()], None, [0], [[0.0, 1.0]], **kw)
    with pytest.raises(ValueError, match="positive integers"):
        A.VideoRankMeter(n=(1, 0), device="cpu")


def meter_by_hand(updates, n):
    num, rr, hits = 0, 0.0, [0] * len(n)
    for ranks in updates:
        for r in ranks:
            num += 1
            rr += 1.0 / (r + 1) if r >= 0 else 0.0
            for a, n_ in enumerate(n):
                hits[a] += 0 <= r < n_
    out = {f"VR@{n_}": hits[a] / num for a, n_ in enumerate(n)}
    out.update(MRR=rr / num, num_samples=num)
    return out


UPDATES = ([0, 3, -1, 1], [-1, -1], [120, 0, 9, 10, 4])


def check_meter(device):
    n = (1, 5, 10, 100, 1000)
    meter = V().VideoRankMeter(n=n, device=device)
    assert meter.state.dtype == torch.float64 and meter.state.device.type == torch.device(device).type
    for ranks in UPDATES:
        meter.update(torch.tensor(ranks, dtype=torch.int32).to(device))
    got, want = meter.result(), meter_by_hand(UPDATES, n)
    assert set(got) == set(want) and got["num_samples"] == 11
    for key in want:
        assert abs(got[key] - want[key]) <= 1e-15, (key, got[key], want[key])
    meter.reset()
    assert meter.state.eq(0).all()


def test_video_rank_meter_on_the_host():
    check_meter("cpu")


# ---------------------------------------------------------------- GPU
def pool_abi(dev, x, temp, fill=float("nan"), **kw):
    """smin_pair_pool at tau = temp through the C ABI over outputs pre-filled with ``fill``; kw overrides arguments by name"""
    L_ = V()._lib
    (P, L), tau = x[1].shape, temp
    a = dict(pm=x[0].to(dev).contiguous(), ps=x[1].to(dev).contiguous(), pe=x[2].to(dev).contiguous(), mm=x[3].to(dev).contiguous(), P=P, L=L, tau=tau,
             score=torch.full((P,), fill, device=dev), pool=torch.full((P, 2), fill, device=dev), cells=torch.full((P,), fill, device=dev))
    a.update(kw)
    p = lambda key: L_.ptr(a[key])
    rc = L_.load().smin_pair_pool(L_.stream(), p("pm"), p("ps"), p("pe"), p("mm"), a["P"], a["L"], a["tau"], p("score"), p("pool"), p("cells"))
    torch.cuda.synchronize()
    return rc, a


@pytest.mark.gpu
@pytest.mark.parametrize("tau", TAUS)
@pytest.mark.parametrize("P,L", [(1, 1), (7, 5), (7, 16), (5, 33)])
def test_pair_pool_has_the_bits_of_the_loss(dev, P, L, tau):
    """33 * 33 = 1089 > 4 * 256: the strided walk of a thread and its row wrap.  Measured on an MI355X: in the table of INTEGRATION.md 3t."""
    A = V()
    assert (P, L) != (5, 33) or L * L > 4 * 256
    x = synthetic(P, L, seed=100 * P + L)
    plan = A.PairPlan(list(range(P)), [0] * P, P, 1, dev, gt_video=[0])
    rc, loss_outs, _ = abi_call(dev, x, plan, tau=tau, gamma=0.1)
    assert rc == 0
    rc, a = pool_abi(dev, x, tau)
    assert rc == 0
    for key in ("score", "pool", "cells"):
        assert torch.isfinite(a[key]).all(), key                                   # every element written over the NaN
    assert torch.equal(bits(a["score"]), bits(loss_outs["score"]))
    assert torch.equal(bits(a["pool"]), bits(loss_outs["pool"]))
    rc, again = pool_abi(dev, x, tau, fill=-7.0)
    assert rc == 0 and all(torch.equal(bits(a[key]), bits(again[key])) for key in ("score", "pool", "cells"))
    score, pool, cells = A.pair_pool(*[t.to(dev) for t in x], tau=tau)
    assert torch.equal(bits(score), bits(a["score"])) and torch.equal(bits(pool), bits(a["pool"])) and torch.equal(bits(cells), bits(a["cells"]))
    x64 = [t.to(dev).double() for t in x[:3]] + [x[3].to(dev)]
    want, ref32 = A.pair_pool_torch(*x64, tau=tau), A.pair_pool_torch(*[t.to(dev) for t in x], tau=tau)
    assert torch.equal(cells.double(), want[2]) and cells.cpu().tolist() == x[3].reshape(P, -1).sum(1).float().tolist()
    tag = f"(P, L) = ({P}, {L}) tau {tau}"
    gate(tag + " score", score, want[0], ref32[0])
    gate(tag + " pool.m", pool[:, 0], want[1][:, 0], ref32[1][:, 0])
    gate(tag + " pool.sum", pool[:, 1], want[1][:, 1], ref32[1][:, 1])
    if P > 2:
        assert bits(score[P // 2]).item() == 0 and bits(pool[P // 2]).eq(0).all() and cells[P // 2].item() == 0.0


@pytest.mark.gpu
@pytest.mark.parametrize("tau", TAUS)
def test_group_pool(dev, tau):
    A = V()
    L_ = A._lib
    x = synthetic(7, 8, seed=21)
    xd = [t.to(dev) for t in x]
    gp = torch.tensor([0, 0, 1, 3, 7], dtype=torch.int32, device=dev)                  # groups of 0, 1, 2 and 4 windows; window 3 has no cell
    score, pool, cells = A.pair_pool(*xd, tau=tau)
    assert cells[3].item() == 0.0
    gs, gc = A.group_pool(pool, cells, gp, tau)
    w_pool = A.pair_pool_torch(*[t.double() for t in xd[:3]], xd[3], tau=tau)
    want = A.group_pool_torch(w_pool[1], w_pool[2], gp, tau)
    r_pool = A.pair_pool_torch(*xd, tau=tau)
    ref32 = A.group_pool_torch(r_pool[1], r_pool[2], gp, tau)
    gate(f"tau {tau} group score", gs, want[0], ref32[0])
    assert torch.equal(gc.double(), want[1]) and bits(gs[0]).item() == 0 and gc[0].item() == 0.0
    # a group of one window reproduces that window's pair_pool score to within the gate
    e_t = abs(ref32[0][1].item() - want[0][1].item()) / abs(want[0][1].item())
    e_g = abs(gs[1].item() - score[0].item()) / abs(score[0].item())
    print(f"tau {tau} single-window group against its window: e {e_g:.2e}  e_torch32 {e_t:.2e}")
    assert e_g <= 32 * e_t + 1e-6
    # through the C ABI over a sentinel, twice
    outs = []
    for fill in (float("nan"), -7.0):
        o = [torch.full((4,), fill, device=dev), torch.full((4,), fill, device=dev)]
        rc = L_.load().smin_group_pool(L_.stream(), L_.ptr(pool), L_.ptr(cells), L_.ptr(gp), 4, 7, tau, L_.ptr(o[0]), L_.ptr(o[1]))
        torch.cuda.synchronize()
        assert rc == 0 and torch.equal(bits(o[0]), bits(gs)) and torch.equal(bits(o[1]), bits(gc))
        outs.append(o)
    # malformed pointers are clamped: nothing outside the seven windows is read
    wild = torch.tensor([-5, 3, 2, 99, 7], dtype=torch.int32, device=dev)
    got = A.group_pool(pool, cells, wild, tau)
    ref = A.group_pool_torch(r_pool[1], r_pool[2], wild, tau)
    assert torch.isfinite(got[0]).all() and torch.equal(got[1].double(), ref[1].double())


@pytest.mark.gpu
@pytest.mark.parametrize("tau", SAT_TAUS)
@pytest.mark.parametrize("P,L", SAT_POOL)
def test_pair_pool_at_small_tau(dev, P, L, tau):
    """tied_maps: only the cells at a pair's maximum survive the exponential.  The score is m + tau * log(k / n); pool holds m and k
    exactly (every other exponential is 0 in fp32); the pair without a cell gives +0.0 throughout; the project's gate against the fp64
    restatement.  Measured on an MI355X: INTEGRATION.md, "Saturated inputs"."""
    A = V()
    x = tied_maps(P, L, seed=100 * P + L)
    by_hand, top, ties, n = tied_pool_by_hand(x[0].double(), x[3], tau)
    xd = [t.to(dev) for t in x]
    score, pool, cells = A.pair_pool(*xd, tau=tau)
    want, ref32 = A.pair_pool_torch(*[t.double() for t in xd[:3]], xd[3], tau=tau), A.pair_pool_torch(*xd, tau=tau)
    assert all(torch.isfinite(t).all() for t in (score, pool, cells))
    assert pool[:, 0].cpu().tolist() == top and pool[:, 1].cpu().tolist() == [float(k) for k in ties] and cells.cpu().tolist() == [float(c) for c in n]
    tag = f"pair_pool (P, L) = ({P}, {L}) tau {tau}"
    gate(tag + " score", score, want[0], ref32[0])
    gate(tag + " score by hand", score, torch.tensor(by_hand, dtype=torch.float64), ref32[0])
    assert bits(score[P // 2]).item() == 0 and bits(pool[P // 2]).eq(0).all() and cells[P // 2].item() == 0.0


@pytest.mark.gpu
@pytest.mark.parametrize("tau", SAT_TAUS)
def test_group_pool_at_small_tau(dev, tau):
    """test_group_pool's groups over tied_maps: windows whose maximum lies below their group's drop out of its sum.  Measured on an
    MI355X: INTEGRATION.md, "Saturated inputs"."""
    A = V()
    xd = [t.to(dev) for t in tied_maps(7, 8, seed=21)]
    gp = torch.tensor(GROUP_PTR, dtype=torch.int32, device=dev)
    _, pool, cells = A.pair_pool(*xd, tau=tau)
    gs, gc = A.group_pool(pool, cells, gp, tau)
    w_pool = A.pair_pool_torch(*[t.double() for t in xd[:3]], xd[3], tau=tau)
    want = A.group_pool_torch(w_pool[1], w_pool[2], gp, tau)
    r_pool = A.pair_pool_torch(*xd, tau=tau)
    ref32 = A.group_pool_torch(r_pool[1], r_pool[2], gp, tau)
    assert torch.isfinite(gs).all() and torch.equal(gc.double(), want[1])
    gate(f"group_pool tau {tau} score", gs, want[0], ref32[0])
    assert bits(gs[0]).item() == 0 and gc[0].item() == 0.0


@pytest.mark.gpu
@pytest.mark.parametrize("alpha", SAT_ALPHAS)
def test_video_rank_weights_at_large_alpha(dev, alpha):
    """weight_case: exp(alpha * (s - s_max)) at alpha 50, 500 (most weights underflow; none may exceed 1) and -500 (weights up to
    exp(62.5)).  Finite, exactly 1 for each query's best pair, +0.0 for the pairs that are no candidates, never above 1 for alpha > 0,
    and the project's gate against the fp64 restatement.  Measured on an MI355X: INTEGRATION.md, "Saturated inputs"."""
    A = V()
    case = weight_case(alpha)
    on = [t.to(dev) for t in case]
    got = A.rank_videos(*on[:4], n=5, alpha=alpha, gt_video=on[4])
    want = A.rank_videos_torch(case[0].double(), case[1].double(), case[2], case[3], n=5, alpha=alpha, gt_video=case[4])
    r32 = A.rank_videos_torch(*on[:4], n=5, alpha=alpha)["weight"]
    for key in ("video", "count", "pair_rank", "gt_rank"):
        assert torch.equal(got[key].cpu(), want[key]), key
    w, listed = got["weight"].cpu(), want["pair_rank"] >= 0
    assert torch.isfinite(w).all() and bits(w[~listed]).eq(0).all() and (w[want["pair_rank"] == 0] == 1.0).all()
    assert (w <= 1.0).all() if alpha > 0 else (w[listed] >= 1.0).all()
    gate(f"video_rank alpha {alpha} weight", got["weight"], want["weight"], r32)


def rank_case(Q, Vn, seed):
    """Q queries over Vn videos: each lists the videos but max(1, Vn // 32) it skips (none at Vn = 1), scores from 8 distinct values
    with both zeros among them, max(1, listed // 32) of a query's pairs without cells (none where it lists one), gt_video anywhere in
    [0, Vn)."""
    g = torch.Generator().manual_seed(seed)
    values = torch.tensor([0.0, -0.0, 0.5, -0.5, 0.25, 1.0, 0.75, -1.5, 0.125])           # 8 distinct values: the two zeros are one
    vids, ptr, live = [], [0], []
    for q in range(Q):
        keep = torch.ones(Vn, dtype=torch.bool)
        if Vn > 1:
            keep[torch.randperm(Vn, generator=g)[:max(1, Vn // 32)]] = False
        n = int(keep.sum())
        has = torch.ones(n)
        if n > 1:
            has[torch.randperm(n, generator=g)[:max(1, n // 32)]] = 0.0
        vids.append(torch.nonzero(keep).reshape(-1))
        live.append(has)
        ptr.append(ptr[-1] + n)
    video = torch.cat(vids).to(torch.int32)
    P = video.shape[0]
    score = values[torch.randint(0, values.shape[0], (P,), generator=g)]
    cells = torch.randint(1, 37, (P,), generator=g).float() * torch.cat(live)
    gt = torch.randint(0, Vn, (Q,), generator=g).to(torch.int32)
    return score, cells, video, torch.tensor(ptr, dtype=torch.int32), gt


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 5, 64])
@pytest.mark.parametrize("Q,Vn", [(1, 1), (3, 5), (4, 70), (2, 9000)])
def test_video_rank_bit_exact(dev, Q, Vn, n):
    """70 videos: more than n = 64; 9000: more than one LDS tile of VR_TILE = 2048 order words, and more pairs than a workgroup has threads."""
    A = V()
    assert 9000 > VR_TILE
    case = rank_case(Q, Vn, seed=7 * Q + Vn)
    score, cells, video, ptr, gt = case
    if Vn >= 70:
        per_query = [int((cells[ptr[q]:ptr[q + 1]] > 0).sum()) for q in range(Q)]
        assert min(per_query) > 64 >= n and bits(score).eq(-2 ** 31).any() and bits(score).eq(0).any() and cells.eq(0).any()
    if Vn == 9000:
        assert int((ptr[1:] - ptr[:-1]).min()) > 4 * VR_TILE
    on = [t.to(dev) for t in case]
    for alpha in (0.0, 7.5, -2.0):                                                    # (a negative alpha is allowed: weights >= 1)
        want = A.rank_videos_torch(score, cells, video, ptr, n=n, alpha=alpha, gt_video=gt)
        got = A.rank_videos(*on[:4], n=n, alpha=alpha, gt_video=on[4])
        for key in ("video", "count", "pair_rank", "gt_rank"):
            assert got[key].dtype == want[key].dtype and torch.equal(got[key].cpu(), want[key]), (key, alpha)
        assert torch.equal(bits(got["score"]), bits(want["score"])), alpha              # a copy: -0 stays -0
        listed = want["pair_rank"] >= 0
        if alpha == 0.0:
            assert torch.equal(bits(got["weight"]), bits(listed.float()))               # exactly 1.0 for every candidate, +0.0 elsewhere
        else:
            w64 = A.rank_videos_torch(score.double(), cells.double(), video, ptr, n=n, alpha=alpha)["weight"]
            r32 = A.rank_videos_torch(*on[:4], n=n, alpha=alpha)["weight"]
            gate(f"(Q, V) = ({Q}, {Vn}) n {n} weight", got["weight"], w64, r32)
            assert bits(got["weight"].cpu()[~listed]).eq(0).all()
        again = A.rank_videos(*on[:4], n=n, alpha=alpha, gt_video=on[4])
        assert all(torch.equal(again[key], got[key]) for key in got)
    none = A.rank_videos(*on[:4], n=n)
    assert none["gt_rank"].eq(-1).all()
    if Vn > 1:
        assert (want["gt_rank"] >= 0).any()


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 64])
def test_video_rank_repeated_videos(dev, n):
    """What rank_case leaves out: a query that lists a video twice, at one score (the earlier pair goes first) and at -0 against +0;
    Q = 3 with a query without pairs between the others; the last query has no candidate."""
    A = V()
    score = torch.tensor([0.5, 0.75, 0.5, -0.0, 0.0, 0.75, 0.25, 0.25])
    cells = torch.tensor([3.0, 2.0, 3.0, 1.0, 1.0, 0.0, 0.0, 0.0])
    video = torch.tensor([4, 9, 4, 2, 2, 1, 7, 7], dtype=torch.int32)
    ptr = torch.tensor([0, 6, 6, 8], dtype=torch.int32)
    gt = torch.tensor([4, 0, 7], dtype=torch.int32)
    want = A.rank_videos_torch(score, cells, video, ptr, n=n, gt_video=gt)
    assert want["pair_rank"].tolist() == [1, 0, 2, 3, 4, -1, -1, -1] and want["gt_rank"].tolist() == [1, -1, -1] and want["count"].tolist() == [min(n, 5), 0, 0]
    got = A.rank_videos(*[t.to(dev) for t in (score, cells, video, ptr)], n=n, gt_video=gt.to(dev))
    for key in ("video", "count", "pair_rank", "gt_rank", "score", "weight"):
        assert got[key].dtype == want[key].dtype and torch.equal(bits(got[key]), bits(want[key])), key


def video_rank_abi(dev, case, top, scale, fill, **kw):
    """smin_video_rank at n = top, alpha = scale through the C ABI over outputs pre-filled with ``fill``; kw overrides arguments by name"""
    L_ = V()._lib
    score, cells, video, ptr, gt = [t.to(dev) for t in case]
    P, Q, n, alpha = score.shape[0], ptr.shape[0] - 1, top, scale
    a = dict(pair_score=score, pair_cells=cells, pair_video=video, pair_ptr=ptr, gt_video=gt, P=P, Q=Q, n=n, alpha=alpha,
             out_video=torch.full((Q, n), int(fill), dtype=torch.int64, device=dev), out_score=torch.full((Q, n), fill, device=dev),
             out_count=torch.full((Q,), int(fill), dtype=torch.int32, device=dev), pair_rank=torch.full((P,), int(fill), dtype=torch.int32, device=dev),
             weight=torch.full((P,), fill, device=dev), gt_rank=torch.full((Q,), int(fill), dtype=torch.int32, device=dev))
    a.update(kw)
    p = lambda key: L_.ptr(a[key])
    rc = L_.load().smin_video_rank(L_.stream(), p("pair_score"), p("pair_cells"), p("pair_video"), p("pair_ptr"), p("gt_video"), a["P"], a["Q"], a["n"],
                                   a["alpha"], p("out_video"), p("out_score"), p("out_count"), p("pair_rank"), p("weight"), p("gt_rank"))
    torch.cuda.synchronize()
    return rc, a


OUTS = ("out_video", "out_score", "out_count", "pair_rank", "weight", "gt_rank")


@pytest.mark.gpu
def test_c_abi_writes_everything_and_rejects_before_any_launch(dev):
    A = V()
    L_ = A._lib
    lib = L_.load()
    case = rank_case(3, 5, seed=4)
    rc, a = video_rank_abi(dev, case, 5, 7.5, -7.0)
    want = A.rank_videos_torch(*case[:4], n=5, alpha=7.5, gt_video=case[4])
    assert rc == 0 and torch.equal(a["out_video"].cpu(), want["video"]) and torch.equal(a["pair_rank"].cpu(), want["pair_rank"])
    assert not a["weight"].eq(-7.0).any() and not a["out_score"].eq(-7.0).any() and not a["gt_rank"].eq(-7).any()
    # a pair_ptr that leaves pairs in front of the first segment and behind the last: they come out as non-candidates
    inner = case[3].clone()
    inner[0], inner[-1] = 2, int(inner[-1]) - 1
    rc, b = video_rank_abi(dev, (case[0], case[1], case[2], inner, case[4]), 5, 7.5, -7.0)
    assert rc == 0 and b["pair_rank"][:2].eq(-1).all() and b["pair_rank"][-1].item() == -1 and b["weight"][:2].eq(0).all()
    assert not b["pair_rank"].eq(-7).any() and not b["weight"].eq(-7.0).any()
    bad = [dict(n=0), dict(n=65), dict(Q=-1), dict(P=-1), dict(alpha=float("nan")), dict(alpha=float("inf")), dict(alpha=float("-inf"))]
    bad += [{key: None} for key in ("pair_score", "pair_cells", "pair_video", "pair_ptr") + OUTS]
    for kw in bad:
        rc, a = video_rank_abi(dev, case, 5, 7.5, -7.0, **kw)
        assert rc != 0, kw
        for key in OUTS:
            assert a[key] is None or a[key].eq(-7).all(), (kw, key)
    rc, a = video_rank_abi(dev, case, 5, 7.5, -7.0, Q=0)                              # Q == 0 launches nothing
    assert rc == 0 and all(a[key].eq(-7).all() for key in OUTS)
    rc, a = video_rank_abi(dev, case, 5, 7.5, -7.0, gt_video=None)                    # gt_video may be NULL
    assert rc == 0 and a["gt_rank"].eq(-1).all()
    # smin_pair_pool
    x = synthetic(7, 5, seed=9)
    bad = [dict(P=0), dict(P=-1), dict(L=0), dict(L=4097), dict(tau=0.0), dict(tau=-1.0), dict(tau=float("nan")), dict(tau=float("inf"))]
    bad += [{key: None} for key in ("pm", "ps", "pe", "mm", "score", "pool", "cells")]
    for kw in bad:
        rc, a = pool_abi(dev, x, 0.1, fill=-7.0, **kw)
        assert rc != 0, kw
        for key in ("score", "pool", "cells"):
            assert a[key] is None or a[key].eq(-7.0).all(), (kw, key)
    # smin_group_pool
    pool, cells, gp = torch.rand(7, 2, device=dev), torch.ones(7, device=dev), torch.tensor([0, 0, 1, 3, 7], dtype=torch.int32, device=dev)
    for kw in (dict(G2=-1), dict(W=-1), dict(tau=0.0), dict(tau=float("nan")), dict(tau=float("inf")), dict(pool=None), dict(cells=None), dict(gp=None),
               dict(score=None), dict(out=None)):
        a = dict(pool=pool, cells=cells, gp=gp, G2=4, W=7, tau=0.1, score=torch.full((4,), -7.0, device=dev), out=torch.full((4,), -7.0, device=dev))
        a.update(kw)
        rc = lib.smin_group_pool(L_.stream(), L_.ptr(a["pool"]), L_.ptr(a["cells"]), L_.ptr(a["gp"]), a["G2"], a["W"], a["tau"], L_.ptr(a["score"]), L_.ptr(a["out"]))
        torch.cuda.synchronize()
        assert rc != 0, kw
        assert all(a[key] is None or a[key].eq(-7.0).all() for key in ("score", "out")), kw
    assert lib.smin_group_pool(L_.stream(), None, None, None, 0, 0, 0.1, None, None) == 0          # G2 == 0 launches nothing
    # smin_moment_reweight: the values over a sentinel, then the rejections
    P, k = 6, 3
    lists, cnt = torch.rand(P, k, device=dev), torch.tensor([3, 2, 0, 1, 3, 3], dtype=torch.int32, device=dev)
    rank, weight = torch.tensor([0, 1, 2, -1, 0, 3], dtype=torch.int32, device=dev), torch.rand(P, device=dev)
    for cut in (0, -3, 1, 2, 99):
        o = [torch.full((P, k), float("nan"), device=dev), torch.full((P,), -7, dtype=torch.int32, device=dev)]
        rc = lib.smin_moment_reweight(L_.stream(), L_.ptr(lists), L_.ptr(cnt), L_.ptr(rank), L_.ptr(weight), P, k, cut, L_.ptr(o[0]), L_.ptr(o[1]))
        torch.cuda.synchronize()
        want = A.reweight_moments_torch(lists, cnt, rank, weight, max(cut, 0))
        assert rc == 0 and torch.equal(bits(o[0]), bits(want[0])) and torch.equal(o[1], want[1]), cut
        if cut > 0:
            got = A.reweight_moments(lists, cnt, rank, weight, cut)
            assert torch.equal(bits(got[0]), bits(want[0])) and torch.equal(got[1], want[1])
    for kw in (dict(P=-1), dict(k=0), dict(k=65), dict(lists=None), dict(cnt=None), dict(rank=None), dict(weight=None), dict(o0=None), dict(o1=None)):
        a = dict(lists=lists, cnt=cnt, rank=rank, weight=weight, P=P, k=k, o0=torch.full((P, k), -7.0, device=dev),
                 o1=torch.full((P,), -7, dtype=torch.int32, device=dev))
        a.update(kw)
        rc = lib.smin_moment_reweight(L_.stream(), L_.ptr(a["lists"]), L_.ptr(a["cnt"]), L_.ptr(a["rank"]), L_.ptr(a["weight"]), a["P"], a["k"], 2,
                                      L_.ptr(a["o0"]), L_.ptr(a["o1"]))
        torch.cuda.synchronize()
        assert rc != 0, kw
        assert all(a[key] is None or a[key].eq(-7).all() for key in ("o0", "o1")), kw
    assert lib.smin_moment_reweight(L_.stream(), None, None, None, None, 0, k, 2, None, None) == 0  # P == 0 launches nothing


TAU = 0.1


@pytest.fixture(scope="module")
def world(dev):
    """the tiny model and corpus of test_pair_training (V = 5, Q = 4, L = 8) as banks, and the small window corpus of test_window_search"""
    m, _ = tiny_model(dev)
    vid, qry, _ = corpus_inputs()
    vid_d, qry_d = {k: v.to(dev) for k, v in vid.items()}, {k: v.to(dev) for k, v in qry.items()}
    vb = m.encode_videos(vid_d["video_features"], vid_d["video_mask"], vid_d["length_mask"], vid_d["moment_mask"])
    qb = m.encode_queries(qry_d["query_features"], qry_d["query_mask"])
    raw, qf, qm = WS.corpus_rows(WS.SEED)
    raw_d, qf_d, qm_d = raw.to(dev), qf.to(dev), qm.to(dev)
    wqb = m.encode_queries(qf_d, qm_d)
    wb = m.encode_windows(raw_d, WS.LENGTHS, WS.WINDOW, WS.STRIDE)
    return dict(m=m, vid_d=vid_d, qry_d=qry_d, vb=vb, qb=qb, raw=raw_d, wqf=qf_d, wqm=qm_d, wqb=wqb, wb=wb)


@pytest.mark.gpu
def test_search_at_neutral_settings_is_todays_search(dev, world):
    m, vb, qb = world["m"], world["vb"], world["qb"]
    want = m.search(vb, qb, k=7, k_video=3)
    assert set(want) == {"video", "idx", "score", "count"} and int(want["count"].min()) >= 1
    for kw in (dict(video_weight=0.0), dict(max_videos=5), dict(video_weight=0.0, max_videos=5)):
        got = m.search(vb, qb, k=7, k_video=3, **kw)
        same(got, want, SEARCH_KEYS, kw)
        assert set(got) == set(want) | {"video_rank", "video_score", "video_count", "gt_rank"}
        assert tuple(got["video_rank"].shape) == (4, 7) and got["video_count"].tolist() == [5] * 4 and got["gt_rank"].tolist() == [-1] * 4
    listed = [(3, 4), (0, 2), (2, 3), (0, 0)]
    same(m.search(vb, qb, pairs=listed, k=7, k_video=3, video_weight=0.0), m.search(vb, qb, pairs=listed, k=7, k_video=3), SEARCH_KEYS, "listed pairs")
    wb, wqb = world["wb"], world["wqb"]
    kw0 = dict(duration=DURATION_TENSOR.to(dev), max_batch=7, **WS.KW)
    want = m.search_windows(wb, wqb, **kw0)
    for kw in (dict(video_weight=0.0), dict(max_videos=5)):
        got = m.search_windows(wb, wqb, **kw0, **kw)
        same(got, want, WS.KEYS + ("times",), kw)
        assert got["video_count"].tolist() == [4] * 4                                  # video 3 has no rows: no window, no candidate


def pooled_ranks(m, world, alpha, n, gt):
    """the kernels' rank and weight of every (query, video) pair of the bank, from pair_scores(pool="lme")"""
    A = V()
    vb, qb = world["vb"], world["qb"]
    dev = vb.device
    Q, Vn = len(qb), len(vb)
    score = m.pair_scores(vb, qb, pool="lme", tau=TAU).reshape(-1)
    cells = torch.tensor(vb.cell_counts, dtype=torch.float32).repeat(Q).to(dev)
    video = torch.arange(Vn, dtype=torch.int32).repeat(Q).to(dev)
    ptr = (torch.arange(Q + 1, dtype=torch.int32) * Vn).to(dev)
    return A.rank_videos(score, cells, video, ptr, n=n, alpha=alpha, gt_video=None if gt is None else torch.tensor(gt, dtype=torch.int32).to(dev))


def check_cut(r, gt, cut):
    """every listed video lies within the query's first ``cut`` of video_rank; gt_rank agrees with video_rank"""
    vr, n = r["video_rank"].cpu(), r["video_rank"].shape[1]
    for q in range(vr.shape[0]):
        listed = r["video"][q, :int(r["count"][q])].cpu().tolist()
        assert listed and set(listed) <= set(vr[q, :cut].tolist()), (q, listed, vr[q].tolist())
        g = int(r["gt_rank"][q])
        ranked = vr[q, :int(r["video_count"][q])].tolist()
        if 0 <= g < n:
            assert ranked[g] == gt[q]
        else:
            assert gt[q] not in ranked


@pytest.mark.gpu
def test_weighted_search_with_the_video_cut(dev, world):
    A = V()
    m, vb, qb = world["m"], world["vb"], world["qb"]
    gt = [2, 0, 3, 1]
    kw = dict(k=7, k_video=3)
    r = m.search(vb, qb, video_weight=7.5, max_videos=2, tau=TAU, gt_video=gt, **kw)
    vr = pooled_ranks(m, world, 7.5, 7, gt)
    want = m.search_torch(vb, qb, scorer=lambda vi, qi: m.score_pairs(vb, qb, vi, qi), pair_rank=vr["pair_rank"], weight=vr["weight"], max_videos=2, **kw)
    same(r, want, SEARCH_KEYS, "search(video_weight=7.5, max_videos=2)")
    same(dict(video_rank=r["video_rank"], video_score=r["video_score"], video_count=r["video_count"], gt_rank=r["gt_rank"]),
         dict(video_rank=vr["video"], video_score=vr["score"], video_count=vr["count"], gt_rank=vr["gt_rank"]),
         ("video_rank", "video_score", "video_count", "gt_rank"), "the video ranking")
    check_cut(r, gt, 2)
    assert sorted(r["gt_rank"].tolist()) != [-1] * 4 and r["video_rank"].shape == (4, 7) and r["video_count"].tolist() == [5] * 4
    plain = m.search(vb, qb, **kw)
    assert not torch.equal(plain["score"], r["score"])                                # the weight moved scores ...
    assert (r["score"] <= plain["score"][:, :1] + 0).all()                            # ... down: every weight is <= 1
    # SMIN.rank_videos: the same ranking, video retrieval only
    rv = m.rank_videos(vb, qb, n=7, tau=TAU, gt_video=gt)
    assert set(rv) == {"video", "score", "count", "pair_score", "pair_rank", "gt_rank"}
    same(rv, vr, ("video", "score", "count", "pair_rank", "gt_rank"), "SMIN.rank_videos")
    assert torch.equal(bits(rv["pair_score"]), bits(m.pair_scores(vb, qb, pool="lme", tau=TAU).reshape(-1)))


@pytest.mark.gpu
def test_weighted_window_search_with_the_video_cut(dev, world):
    A = V()
    m, wb, qb = world["m"], world["wb"], world["wqb"]
    gt = [0, 4, 2, 3]                                                                # video 3 has no rows: never a candidate
    kw = dict(max_batch=7, **WS.KW)
    r = m.search_windows(wb, qb, video_weight=7.5, max_videos=2, tau=TAU, gt_video=gt, duration=DURATION_TENSOR.to(dev), **kw)
    # the restatement: the same expansion, pools and groups from the public pieces, then search_windows_torch with the kernels' rank and weight
    _, p = m._window_search_plan("test", wb, qb, None, 5, 3, 3, 7, None)
    on = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev).to(torch.int32)
    scorer = lambda wi, wq: m.score_pairs(wb, qb, wi, wq)
    pool, cells = [], []
    for c0 in range(0, p["wi"].shape[0], 7):
        x = scorer(p["wi"][c0:c0 + 7], p["wq"][c0:c0 + 7])
        _, pl, cl = A.pair_pool(x[0], x[1], x[2], wb.moment_mask.index_select(0, on(p["wi"][c0:c0 + 7])), tau=TAU)
        pool.append(pl)
        cells.append(cl)
    gs, gc = A.group_pool(torch.cat(pool), torch.cat(cells), on(p["group_ptr"]), TAU)
    vr = A.rank_videos(gs, gc, on(p["vi"]), on(p["query_ptr"]), n=5, alpha=7.5, gt_video=on(np.asarray(gt)))
    want = m.search_windows_torch(wb, qb, scorer=scorer, pair_rank=vr["pair_rank"], weight=vr["weight"], max_videos=2, duration=DURATION_TENSOR.to(dev), **kw)
    same(r, want, WS.KEYS + ("times",), "search_windows(video_weight=7.5, max_videos=2)")
    same(dict(video_rank=r["video_rank"], gt_rank=r["gt_rank"], video_count=r["video_count"]),
         dict(video_rank=vr["video"], gt_rank=vr["gt_rank"], video_count=vr["count"]), ("video_rank", "gt_rank", "video_count"), "the video ranking")
    check_cut(r, gt, 2)
    assert r["gt_rank"].tolist()[3] == -1 and r["video_count"].tolist() == [4] * 4
    rv = m.rank_videos(wb, qb, n=5, tau=TAU, gt_video=gt, max_batch=7)
    same(rv, vr, ("video", "score", "count", "pair_rank", "gt_rank"), "SMIN.rank_videos over a window bank")
    assert torch.equal(bits(rv["pair_score"]), bits(gs))


@pytest.mark.gpu
def test_mining_by_the_pooled_score(dev, world):
    A = V()
    m, vb, qb = world["m"], world["vb"], world["qb"]
    Q, Vn = len(qb), len(vb)
    vi, qi = np.tile(np.arange(Vn), Q), np.repeat(np.arange(Q), Vn)
    x = m.score_pairs(vb, qb, vi, qi)
    mm = vb.moment_mask.index_select(0, torch.from_numpy(vi).to(dev))
    pooled = m.pair_scores(vb, qb, pool="lme", tau=TAU)
    assert tuple(pooled.shape) == (Q, Vn)
    assert torch.equal(bits(pooled.reshape(-1)), bits(A.pair_pool(x[0], x[1], x[2], mm, tau=TAU)[0]))
    best = m.pair_scores(vb, qb)
    assert torch.equal(bits(best), bits(m.pair_scores(vb, qb, pool=None)))
    assert torch.equal(bits(best.reshape(-1)), bits(A.top_moments(x[0], x[1], x[2], mm, k=1, nms_thresh=1.0)["score"][:, 0]))
    assert (pooled <= best).all() and not torch.equal(pooled, best)                  # a log-mean-exp lies below the maximum
    names = ("video_index", "query_index", "v_ptr", "v_pairs", "q_ptr", "q_pairs")
    for pool, matrix in (("lme", pooled), (None, best)):
        plan = m.mine_pairs(vb, qb, GT_VIDEO, 2, pool=pool, tau=TAU)
        want = A.mine_pairs_torch(matrix.cpu(), GT_VIDEO, 2)
        for name, w in zip(names, want):
            assert torch.equal(getattr(plan, name).cpu(), w), (pool, name)
    default = m.mine_pairs(vb, qb, GT_VIDEO, 2)
    assert torch.equal(default.video_index, plan.video_index)


@pytest.mark.gpu
def test_video_rank_meter_on_the_device(dev):
    check_meter(dev)


@pytest.mark.gpu
def test_model_corpus_with_the_video_weight_reads_once(dev, world):
    A = V()
    m, vid_d, qry_d, vb = world["m"], world["vid_d"], world["qry_d"], world["vb"]
    duration = np.array([10.0, 3.5, 60.0, 7.25, 100.0])
    gt_video = np.array([2, 0, 3, 1])
    gt_times = np.stack([np.array([1.0, 0.5, 2.0, 0.0]), np.array([6.0, 3.0, 30.0, 5.0])], axis=1)
    shard = dict(vid_d, duration=duration, cell_counts=vb.cell_counts)
    kw = dict(k=10, k_video=2, video_weight=7.5, tau=TAU)
    # by hand: search, the times, the two meters
    bank = m.encode_videos(vid_d["video_features"], vid_d["video_mask"], vid_d["length_mask"], vid_d["moment_mask"], cell_counts=vb.cell_counts)
    r = m.search(bank, m.encode_queries(qry_d["query_features"], qry_d["query_mask"]), gt_video=gt_video, **kw)
    r["times"] = A.moments.search_times(r["video"], r["idx"], torch.from_numpy(duration).to(dev), m.L)
    hand, hand_v = A.CorpusMeter(n=(1, 5), device=dev), A.VideoRankMeter(n=(1, 2, 5), device=dev)
    hand.update(r, torch.from_numpy(gt_video).to(dev), torch.from_numpy(gt_times).float().to(dev))
    hand_v.update(r["gt_rank"])
    want, want_v = hand.result(), hand_v.result()

    class Counting(A.CorpusMeter):
        reads = 0

        def result(self):
            torch.cuda.set_sync_debug_mode(mode)                                     # everything before this point ran without a host read
            Counting.reads += 1
            return super().result()

    A.test_model_corpus(m, [shard], qry_d, gt_video, gt_times, video_meter=A.VideoRankMeter(n=(1, 2, 5), device=dev), **kw)   # first use outside the checked region
    video_meter = A.VideoRankMeter(n=(1, 2, 5), device=dev)
    torch.cuda.synchronize()
    mode = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        got = A.test_model_corpus(m, [shard], qry_d, gt_video, gt_times, Counting(n=(1, 5), device=dev), video_meter=video_meter, **kw)
    finally:
        torch.cuda.set_sync_debug_mode(mode)
    got_v = video_meter.result()
    print("test_model_corpus(video_weight=7.5)", got, got_v)
    assert Counting.reads == 1 and got == want and got_v == want_v and got_v["num_samples"] == 4
    assert got_v["VR@1"] <= got_v["VR@2"] <= got_v["VR@5"] == 1.0 and 0.0 < got_v["MRR"] <= 1.0     # five videos, all candidates
    with pytest.raises(ValueError, match="one shard"):
        A.test_model_corpus(m, [shard, shard], qry_d, gt_video, gt_times, **kw)
    # the window loop takes the same options
    raw, queries = world["raw"], dict(query_features=world["wqf"], query_mask=world["wqm"])
    vm = A.VideoRankMeter(n=(1, 2), device=dev)
    wkw = dict(window=WS.WINDOW, stride=WS.STRIDE, k=25, k_video=5)
    out = A.test_model_corpus_windows(m, raw, WS.LENGTHS, queries, [0, 4, 2, 1], gt_times, duration, video_weight=7.5, max_videos=2, video_meter=vm, **wkw)
    rw = m.search_windows(world["wb"], world["wqb"], k=25, k_video=5, video_weight=7.5, max_videos=2, gt_video=[0, 4, 2, 1])
    assert out["num_samples"] == 4 and vm.state[0].item() == 4.0
    assert vm.result()["VR@1"] == rw["gt_rank"].eq(0).sum().item() / 4


@pytest.mark.gpu
def test_loops_with_the_video_meter_alone(dev, world):
    """video_meter without video_weight / max_videos: the search runs at the neutral weight 0.0, so the corpus metrics are the plain
    loop's and the meter gets the video ranking's gt_rank"""
    A = V()
    m, vid_d, qry_d, vb = world["m"], world["vid_d"], world["qry_d"], world["vb"]
    duration = np.array([10.0, 3.5, 60.0, 7.25, 100.0])
    gt_video = np.array([2, 0, 3, 1])
    gt_times = np.stack([np.array([1.0, 0.5, 2.0, 0.0]), np.array([6.0, 3.0, 30.0, 5.0])], axis=1)
    shard = dict(vid_d, duration=duration, cell_counts=vb.cell_counts)
    kw = dict(k=10, k_video=2)
    plain = A.test_model_corpus(m, [shard], qry_d, gt_video, gt_times, **kw)
    vm = A.VideoRankMeter(n=(1, 2, 5), device=dev)
    got = A.test_model_corpus(m, [shard], qry_d, gt_video, gt_times, video_meter=vm, tau=TAU, **kw)
    assert got == plain and got["num_samples"] == 4
    want = A.VideoRankMeter(n=(1, 2, 5), device=dev)
    want.update(m.rank_videos(vb, world["qb"], n=5, tau=TAU, gt_video=gt_video)["gt_rank"])
    got_v = vm.result()
    assert got_v == want.result() and got_v["num_samples"] == 4 and got_v["VR@5"] == 1.0
    # the window loop
    raw, queries = world["raw"], dict(query_features=world["wqf"], query_mask=world["wqm"])
    wkw = dict(window=WS.WINDOW, stride=WS.STRIDE, k=25, k_video=5)
    gt_w = [0, 4, 2, 3]                                                              # video 3 has no rows: never ranked
    plain = A.test_model_corpus_windows(m, raw, WS.LENGTHS, queries, gt_w, gt_times, duration, **wkw)
    vm = A.VideoRankMeter(n=(1, 4), device=dev)
    got = A.test_model_corpus_windows(m, raw, WS.LENGTHS, queries, gt_w, gt_times, duration, video_meter=vm, tau=TAU, **wkw)
    assert got == plain
    want = A.VideoRankMeter(n=(1, 4), device=dev)
    want.update(m.rank_videos(world["wb"], world["wqb"], n=5, tau=TAU, gt_video=gt_w)["gt_rank"])
    got_v = vm.result()
    assert got_v == want.result() and got_v["num_samples"] == 4 and got_v["VR@4"] == 0.75
