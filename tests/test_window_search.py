"""Corpus search over long videos: csrc/corpus.hip (smin_corpus_span_topk), the operator
smin_hip::smin_corpus_span_topk, moments.corpus_span_topk, SMIN.encode_windows / search_windows and training.test_model_corpus_windows.

Host: the restated ranking on hand-made lists, search_windows' expansion by hand, the refusals, the C ABI and operator surface, the
restated search on a CPU bank with a scorer.
GPU: the kernel bit for bit against its restatement; the window bank against encode_videos of each window; search_windows end to end
against search_windows_torch (scores of differently composed batches: entries are compared where the restatement's scores separate
them), against localize_windows on listed pairs, without host reads, repeatably, off the one-node path; test_model_corpus_windows
against CorpusMeterTorch; and nothing else moved."""
import os
import re

import numpy as np
import pytest
import torch

from tests import helpers as H
from tests.support.device import dev  # noqa: F401  (the module's device fixture)
from tests.support.device import checked_no_sync, vml as V
from tests.support.compare import bits
from tests.support.guards import WORD_SENTINEL as SENTINEL
from tests.support.corpora import (
    corpus_rows, host_masks, random_span_lists, same_lists, same_search, separated, tiny_model, window_host_banks as host_banks, DIN,
    DURATION_TENSOR as DURATION, KEYS, KW, L, LENGTHS, LENS, NAN_BITS, SEED, STARTS, STRIDE, T, TINY_SHAPE, VPTR, WINDOW)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------- host: surface
def test_header_and_table_declare_the_span_kernel():
    text = open(os.path.join(ROOT, "include", "smin_hip.h")).read()
    assert re.search(r"\bint\s+smin_corpus_span_topk\s*\(", text)
    assert "smin_corpus_span_topk" in V()._lib.SIGNATURES and len(V()._lib.SIGNATURES["smin_corpus_span_topk"]) == 17
    assert hasattr(V()._lib.load(), "smin_corpus_span_topk")
    ops = V()._lib.load_torch()
    assert hasattr(ops, "smin_corpus_span_topk")
    schema = str(torch.ops.smin_hip.smin_corpus_span_topk.default._schema)
    for name in ("Tensor span", "Tensor score", "Tensor window", "Tensor cell", "Tensor count", "Tensor group_video", "Tensor group_ptr", "int k"):
        assert name in schema, schema
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.smin_corpus_span_topk(torch.zeros(1, 2, 2), torch.zeros(1, 2), torch.zeros(1, 2, dtype=torch.int64), torch.zeros(1, 2, 2, dtype=torch.int64),
                                  torch.zeros(1, dtype=torch.int32), torch.zeros(1, dtype=torch.int32), torch.tensor([0, 1], dtype=torch.int32), 5)
    A = V()
    for name in ("WindowBank", "corpus_span_topk", "corpus_span_topk_torch", "test_model_corpus_windows"):
        assert hasattr(A, name), name
    assert issubclass(A.WindowBank, A.VideoBank)


def test_methods_fail_loudly_on_cpu():
    m, _ = tiny_model()
    err = V()._lib.SminHipError
    raw, qf, qm = corpus_rows(0)
    with pytest.raises(err, match="no CPU fallback"):
        m.encode_windows(raw, LENGTHS, WINDOW, STRIDE)
    wb, qb = host_banks()
    with pytest.raises(err, match="no CPU fallback"):
        m.search_windows(wb, qb)
    with pytest.raises(err, match="no CPU fallback"):
        V().corpus_span_topk(*span_lists([0.5, 0.25], [2], [0], [0, 1], 2))


def test_refusals():
    m, _ = tiny_model()
    wb, qb = host_banks()
    assert len(wb) == 8 and wb.n_videos == 5
    for kw in (dict(k=0), dict(k=65), dict(k_video=0), dict(k_video=65), dict(k_window=0), dict(k_window=65), dict(max_batch=0), dict(k=2.0)):
        for f in (m.search_windows, m.search_windows_torch):
            with pytest.raises(ValueError, match="must be an integer"):
                f(wb, qb, **kw)
    with pytest.raises(ValueError, match="more than once"):
        m.search_windows(wb, qb, pairs=[(0, 1), (2, 3), (0, 1)])
    with pytest.raises(ValueError, match="video_index must lie"):
        m.search_windows(wb, qb, pairs=[(0, 5)])                                     # 5 videos, though the bank has 8 rows
    with pytest.raises(ValueError, match="video_index must lie"):
        m.search_windows(wb, qb, pairs=[(4, 0)])
    with pytest.raises(ValueError, match="duration must be"):
        m.search_windows(wb, qb, duration=torch.ones(8))
    with pytest.raises(ValueError, match="duration must be"):
        m.search_windows_torch(wb, qb, duration=torch.ones(5, 1), scorer=lambda wi, wq: None)
    plain = V().VideoBank(None, torch.zeros(8, T, DIN), wb.video_mask, wb.length_mask, wb.moment_mask, wb.cell_counts)
    with pytest.raises(ValueError, match="WindowBank"):
        m.search_windows(plain, qb)
    with pytest.raises(ValueError, match="needs raw"):
        m.search_windows_torch(wb, qb)
    raw = torch.zeros(sum(LENGTHS), DIN)
    for kw in (dict(window=0), dict(stride=0), dict(max_batch=0)):
        with pytest.raises(ValueError, match="must be an integer"):
            m.encode_windows(raw, LENGTHS, **kw)
    with pytest.raises(ValueError, match="mode must be"):
        m.encode_windows(raw, LENGTHS, mode="max")


def test_model_corpus_windows_refuses_a_short_list():
    """k < max(n) * k_video: refused before anything runs (CPU tensors would raise SminHipError first otherwise)"""
    A = V()
    m, _ = tiny_model()
    raw, qf, qm = corpus_rows(0)
    queries = dict(query_features=qf, query_mask=qm)
    gt = np.tile([0.0, 1.0], (4, 1))
    for kw in (dict(k=24, k_video=5), dict(k=4, k_video=1), dict(k=25, k_video=6)):
        with pytest.raises(ValueError, match="needs k >= max"):
            A.test_model_corpus_windows(m, raw, LENGTHS, queries, [0, 1, 2, 4], gt, np.ones(5), **kw)
    with pytest.raises(ValueError, match="needs k >= max"):
        A.test_model_corpus_windows(m, raw, LENGTHS, queries, [0, 1, 2, 4], gt, np.ones(5), A.CorpusMeterTorch(n=(1, 10)), k=25, k_video=5)
    with pytest.raises(ValueError, match="gt_video"):
        A.test_model_corpus_windows(m, raw, LENGTHS, queries, [0, 1, 2], gt, np.ones(5))


# ---------------------------------------------------------------- host: the restated ranking on hand-made lists
def span_lists(score, count, video, ptr, kv, garbage=None):
    """merge_window_moments-shaped lists of len(video) groups with recognisable spans / windows / cells; ``garbage``: the score behind the
    counts (their spans NaN, windows and cells -1, as the merge leaves them)"""
    G2 = len(video)
    score = torch.tensor(score, dtype=torch.float32).reshape(G2, kv)
    span = torch.arange(G2 * kv * 2, dtype=torch.float32).reshape(G2, kv, 2) * 0.5
    window = torch.arange(G2 * kv, dtype=torch.int64).reshape(G2, kv) % 7
    cell = torch.arange(G2 * kv * 2, dtype=torch.int64).reshape(G2, kv, 2) + 1000
    count = torch.tensor(count, dtype=torch.int32)
    if garbage is not None:
        unused = torch.arange(kv).unsqueeze(0) >= count.unsqueeze(1)
        score = torch.where(unused, torch.full_like(score, garbage), score)
        span = torch.where(unused.unsqueeze(2), torch.full_like(span, float("nan")), span)
        window = torch.where(unused, torch.full_like(window, -1), window)
        cell = torch.where(unused.unsqueeze(2), torch.full_like(cell, -1), cell)
    return span, score, window, cell, count, torch.tensor(video, dtype=torch.int32), torch.tensor(ptr, dtype=torch.int32)


def py_span_topk(lists, k):
    """the order by hand: a Python sort of (-score, video, slot, group) over the counted slots (-0 -> +0 by the float comparison)"""
    span, score, window, cell, count, video, ptr = lists
    kv = score.shape[1]
    out = []
    for q in range(len(ptr) - 1):
        g0 = max(int(ptr[q]), 0)
        g1 = max(int(ptr[q + 1]), g0)
        cand = [(-float(score[g, s]) + 0.0, int(video[g]), s, g) for g in range(g0, g1) for s in range(min(max(int(count[g]), 0), kv))]
        cand.sort()
        out.append([(g, s) for _, _, s, g in cand[:k]])
    return out


def check_against_picks(r, lists, picks, k):
    span, score, window, cell, count, video, ptr = lists
    for q, row in enumerate(picks):
        n = len(row)
        assert int(r["count"][q]) == n
        for j, (g, s) in enumerate(row):
            assert int(r["video"][q, j]) == int(video[g])
            assert torch.equal(bits(r["span"][q, j]), bits(span[g, s])) and torch.equal(bits(r["score"][q, j]), bits(score[g, s]))
            assert int(r["window"][q, j]) == int(window[g, s]) and r["cell"][q, j].tolist() == cell[g, s].tolist()
        assert r["video"][q, n:].eq(-1).all() and r["window"][q, n:].eq(-1).all() and r["cell"][q, n:].eq(-1).all()
        assert bits(r["span"][q, n:]).eq(NAN_BITS).all() and bits(r["score"][q, n:]).eq(0).all()


def hand_lists():
    # query 0: videos 7, 2, 4 (ties across videos and within a group, -0 against +0, garbage behind the counts);
    # query 1: no groups; query 2: one group with count 0
    score = [0.5, 0.25, 0.25,   0.5, -0.0, 9.0,   0.0, 0.5, 0.5,   9.0, 9.0, 9.0]
    return span_lists(score, [3, 2, 3, 0], [7, 2, 4, 1], [0, 3, 3, 4], 3, garbage=1e30)


def test_corpus_span_topk_torch_by_hand():
    f = V().corpus_span_topk_torch
    a = hand_lists()
    assert torch.isnan(a[0][1, 2]).all() and float(a[1][1, 2]) > 1e29 and float(a[1][3, 0]) > 1e29       # the garbage is there
    r = f(*a, k=5)
    assert r["count"].tolist() == [5, 0, 0]
    # 0.5: video 2 (group 1 slot 0), video 4 slots 1 and 2, video 7 slot 0; then 0.25: video 7 slot 1
    assert r["video"].tolist() == [[2, 4, 4, 7, 7], [-1] * 5, [-1] * 5]
    assert py_span_topk(a, 5)[0] == [(1, 0), (2, 1), (2, 2), (0, 0), (0, 1)]
    for k in (1, 5, 64):
        r = f(*a, k=k)
        check_against_picks(r, a, py_span_topk(a, k), k)
        assert r["video"].dtype == torch.int64 and r["window"].dtype == torch.int64 and r["cell"].dtype == torch.int64 and r["count"].dtype == torch.int32
    # K larger than the candidates: all 8 in order, -0 (video 2) ahead of +0 (video 4) as equals, by video
    r = f(*a, k=64)
    assert r["count"].tolist() == [8, 0, 0] and r["video"][0, :8].tolist() == [2, 4, 4, 7, 7, 7, 2, 4]
    assert bits(r["score"][0, 6:8]).tolist() == [-2 ** 31, 0]                        # the scores leave as stored: -0 stays -0
    # two groups of one query naming one video: the earlier group first; a count above k_video is clamped, a negative one lists nothing
    b = span_lists([2.0, 1.0, 2.0, 1.0, 3.0, 4.0], [9, 2, -1], [3, 3, 0], [0, 3], 2)
    r = f(*b, k=5)
    check_against_picks(r, b, [[(0, 0), (1, 0), (0, 1), (1, 1)]], 5)
    # a descending or negative pointer gives an empty range
    c = list(hand_lists())
    c[6] = torch.tensor([3, 0, -2, 4], dtype=torch.int32)
    r = f(*c, k=5)
    assert r["count"].tolist() == [0, 0, 5]                                          # (3, 0) and (0, -2): descending, empty; (-2, 4): groups 0 .. 3
    check_against_picks(r, c, py_span_topk(c, 5), 5)
    for bad in (0, 65, 2.0):
        with pytest.raises(ValueError):
            f(*a, k=bad)
    with pytest.raises(ValueError, match="score and window"):
        f(a[0], a[1][:, :2], *a[2:], k=5)


# ---------------------------------------------------------------- host: the expansion of search_windows by hand
def test_expansion_plan_by_hand():
    A = V()
    m, _ = tiny_model()
    wb, qb = host_banks()
    assert [x.tolist() for x in A.window_plan(LENGTHS, WINDOW, STRIDE)] == [STARTS, LENS, VPTR]
    assert wb.cell_counts == tuple(A.cell_count(min(n, T), T, L) for n in LENS) == (36, 36, 36, 36, 36, 15, 36, 36)
    plan = lambda pairs: m._window_search_plan("search_windows", wb, qb, pairs, 5, None, None, 64, None)
    o, p = plan(None)
    assert (o.k, o.k_video, o.k_window) == (5, 5, 5)
    per_video = [[0, 1, 2, 3], [4], [5], [], [6, 7]]
    assert p["qi"].tolist() == [q for q in range(4) for _ in range(5)] and p["vi"].tolist() == [0, 1, 2, 3, 4] * 4
    assert p["wi"].tolist() == [w for _ in range(4) for v in range(5) for w in per_video[v]]
    assert p["wq"].tolist() == [q for q in range(4) for _ in range(8)]
    assert p["group_ptr"].tolist() == [8 * q + o for q in range(4) for o in (0, 4, 5, 6, 6)] + [32]     # the video of 0 rows: an empty group
    assert p["query_ptr"].tolist() == [0, 5, 10, 15, 20]
    # a shuffled list: query 1 has no pair, query 2 only the video without rows
    pairs = np.array([(3, 4), (0, 2), (3, 0), (2, 3), (0, 0), (0, 4)])
    _, p = plan(pairs)
    assert p["qi"].tolist() == [0, 0, 0, 2, 3, 3] and p["vi"].tolist() == [0, 2, 4, 3, 0, 4]
    assert p["wi"].tolist() == [0, 1, 2, 3, 5, 6, 7, 0, 1, 2, 3, 6, 7]
    assert p["wq"].tolist() == [0] * 7 + [3] * 6
    assert p["group_ptr"].tolist() == [0, 4, 5, 7, 7, 11, 13]
    assert p["query_ptr"].tolist() == [0, 3, 3, 4, 6]
    o, p = m._window_search_plan("search_windows", wb, qb, np.zeros((0, 2), dtype=np.int64), 7, 3, None, 64, None)
    assert (o.k_video, o.k_window) == (3, 3) and p["wi"].shape == (0,) and p["group_ptr"].tolist() == [0] and p["query_ptr"].tolist() == [0] * 5


def fake_scorer(wb):
    """scores that are a fixed function of (window, query): what the selection is checked on without a model"""
    def scorer(wi, wq):
        pm, ps, pe = [], [], []
        for w, q in zip(wi.tolist(), wq.tolist()):
            g = torch.Generator().manual_seed(1000 * q + w)
            pm.append(torch.rand(L, L, generator=g) * wb.moment_mask[w])
            ps.append(torch.rand(L, generator=g))
            pe.append(torch.rand(L, generator=g))
        return torch.stack(pm), torch.stack(ps), torch.stack(pe), None
    return scorer


@pytest.mark.parametrize("max_batch", [7, 64])
def test_restated_search_on_a_cpu_bank(max_batch):
    """search_windows_torch with a scorer, on the CPU: the two stages spelled out group by group give its list, and the list has the
    properties of a search (ordered, within the video's rows, times by the stated formula)"""
    A = V()
    m, _ = tiny_model()
    wb, qb = host_banks()
    scorer = fake_scorer(wb)
    duration = torch.tensor([10.0, 3.5, 60.0, 7.25, 100.0])
    r = m.search_windows_torch(wb, qb, k=6, k_video=3, k_window=2, duration=duration, max_batch=max_batch, scorer=scorer)
    assert set(r) == {"video", "span", "score", "window", "cell", "count", "times"} and r["count"].tolist() == [6] * 4
    cand = []
    for q in range(4):
        rows = []
        for v in range(5):
            ws = list(range(VPTR[v], VPTR[v + 1]))
            if not ws:
                continue
            pm, ps, pe, _ = scorer(np.array(ws), np.array([q] * len(ws)))
            t = A.top_moments_torch(pm, ps, pe, wb.moment_mask[ws], k=2, nms_thresh=0.5)
            g = A.merge_window_moments_torch(t["idx"], t["score"], t["count"], torch.tensor([STARTS[w] for w in ws]),
                                             torch.tensor([LENS[w] for w in ws], dtype=torch.int32), torch.tensor([0, len(ws)]), T, L, k=3, nms_thresh=0.5)
            rows += [(-float(g["score"][0, s]), v, s) + tuple(g["span"][0, s].tolist()) + (int(g["window"][0, s]),) for s in range(int(g["count"][0]))]
        rows.sort()
        cand.append(rows[:6])
    for q in range(4):
        for j, (neg, v, s, st, en, w) in enumerate(cand[q]):
            assert int(r["video"][q, j]) == v and float(r["score"][q, j]) == -neg and r["span"][q, j].tolist() == [st, en] and int(r["window"][q, j]) == w
    vid = r["video"]
    assert (vid != 3).all()                                                          # the video without rows is never listed
    n_rows = torch.tensor(LENGTHS, dtype=torch.float32)[vid]
    assert (r["span"][..., 0] >= 0).all() and (r["span"][..., 1] <= n_rows).all() and (r["span"][..., 0] < r["span"][..., 1]).all()
    assert (r["score"][:, :-1] >= r["score"][:, 1:]).all()
    assert torch.equal(r["times"], (r["span"] * duration[vid].unsqueeze(-1)) / n_rows.unsqueeze(-1))
    # listed pairs: a query without pairs and one whose only video has no rows come out empty
    r = m.search_windows_torch(wb, qb, pairs=[(3, 4), (0, 2), (2, 3)], k=4, duration=duration, max_batch=max_batch, scorer=scorer)
    assert r["count"].tolist()[1:3] == [0, 0] and r["video"][1:3].eq(-1).all() and torch.isnan(r["times"][1:3]).all() and torch.isnan(r["span"][1:3]).all()
    assert set(r["video"][0, :int(r["count"][0])].tolist()) == {2} and set(r["video"][3, :int(r["count"][3])].tolist()) == {4}


def test_corpus_meter_takes_the_result_as_it_stands():
    """CorpusMeterTorch.update reads video, count and times of a search_windows-shaped result: no idx"""
    A = V()
    m, _ = tiny_model()
    wb, qb = host_banks()
    r = m.search_windows_torch(wb, qb, k=5, k_video=1, duration=torch.tensor([10.0, 3.5, 60.0, 7.25, 100.0]), scorer=fake_scorer(wb))
    assert "idx" not in r
    meter = A.CorpusMeterTorch(n=(1, 5))
    meter.update(r, r["video"][:, 0], r["times"][:, 0])                              # planted truth: rank 1
    got = meter.result()
    assert got["num_samples"] == 4 and all(got[key] == 1.0 for key in got if key != "num_samples"), got


# ---------------------------------------------------------------- GPU
def through_ctypes(lists, K, dev):
    """smin_corpus_span_topk into buffers pre-filled with a sentinel and four spare words behind each: every element written, none beyond"""
    L_ = V()._lib
    kv, Q = lists[1].shape[1], lists[6].shape[0] - 1
    t = [x.to(dev).contiguous() for x in lists]
    shapes = dict(video=(Q, K), span=(Q, K, 2), score=(Q, K), window=(Q, K), cell=(Q, K, 2), count=(Q,))
    words = {key: (2 if key in ("video", "window", "cell") else 1) * int(np.prod(s)) for key, s in shapes.items()}
    raw = {key: torch.full((n + 4,), SENTINEL, dtype=torch.int32, device=dev) for key, n in words.items()}
    L_.call("smin_corpus_span_topk", L_.stream(), *[L_.ptr(x) if x.numel() else None for x in t], Q, kv, K, *[L_.ptr(raw[key]) for key in KEYS])
    torch.cuda.synchronize()
    out = {}
    for key in KEYS:
        assert raw[key][words[key]:].eq(SENTINEL).all(), key + ": written past the end"
        body = raw[key][:words[key]].cpu()
        out[key] = (body.view(torch.int64) if key in ("video", "window", "cell") else body.view(torch.float32) if key in ("span", "score") else body).reshape(shapes[key])
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("kv", [1, 3, 64])
@pytest.mark.parametrize("K", [1, 5, 64])
def test_corpus_span_topk_bit_exact(dev, K, kv):
    A = V()
    per_query = [0, 1, 7, 3]                                                         # a query without groups among them
    a = random_span_lists(per_query, kv, seed=11 + kv, garbage=1e30)
    b = random_span_lists(per_query, kv, seed=11 + kv, garbage=float("nan"))
    assert (a[4] == 0).any() and (a[4] == kv).any()
    want = A.corpus_span_topk_torch(*a, k=K)
    assert want["count"].tolist() == [min(K, int(a[4][a[6][q]:a[6][q + 1]].sum())) for q in range(4)]
    for name, x in (("huge", a), ("nan", b)):                                        # the garbage behind the counts does not matter
        same_lists(through_ctypes(x, K, dev), want, name)
        same_lists(A.corpus_span_topk(*[t.to(dev) for t in x], k=K), want, name + " (operator)")
    one = random_span_lists([4], kv, seed=3, garbage=1e30)                           # Q = 1
    same_lists(through_ctypes(one, K, dev), A.corpus_span_topk_torch(*one, k=K), "Q = 1")


@pytest.mark.gpu
@pytest.mark.parametrize("K", [1, 64])
def test_corpus_span_topk_edges(dev, K):
    """What random_span_lists leaves out, Q = 1 at k_video = 64 and Q = 3 (the middle query without groups) at k_video = 3: a count above
    k_video and one below 0; the query's last two groups name one video and hold the same scores slot by slot, two of them equal
    within the group, so the slot and then the group ordinal decide; their last slot holds a NaN score, which has the highest order
    word, under a NaN span with a payload of its own, which leaves as it came."""
    A = V()
    for per_query, kv in (([4], 64), ([3, 0, 5], 3)):
        span, score, window, cell, count, video, ptr = random_span_lists(per_query, kv, seed=40 + kv, garbage=1e30)
        count[0], count[1], count[-2], count[-1] = kv + 3, -2, kv, kv
        video[-1] = video[-2]
        score[-2, 1] = score[-2, 0]
        score[-2, kv - 1] = float("nan")
        score[-1] = score[-2]
        span.view(torch.int32)[-2:, kv - 1, 0] = 0x7FC12345
        a = (span, score, window, cell, count, video, ptr)
        want = A.corpus_span_topk_torch(*a, k=K)
        last = len(per_query) - 1
        assert torch.isnan(want["score"][last, 0]) and int(bits(want["span"])[last, 0, 0]) == 0x7FC12345
        assert int(want["count"][last]) == min(K, 2 * kv + int(count[ptr[last]:-2].clamp(0, kv).sum()))
        assert len(per_query) == 1 or int(want["count"][1]) == 0
        same_lists(through_ctypes(a, K, dev), want, (per_query, kv))
        same_lists(A.corpus_span_topk(*[t.to(dev) for t in a], k=K), want, (per_query, kv, "operator"))


@pytest.mark.gpu
def test_corpus_span_topk_many_groups_none_and_rejections(dev):
    A = V()
    a = random_span_lists([700], 5, seed=5, garbage=float("nan"))
    assert int(a[4].sum()) > 1024 and 700 * 5 > 64 * 5                               # several trips of the strided loop, more than K * k_video
    want = A.corpus_span_topk_torch(*a, k=64)
    same_lists(through_ctypes(a, 64, dev), want, "700 groups")
    same_lists(A.corpus_span_topk(*[t.to(dev) for t in a], k=64), want, "700 groups (operator)")
    e = random_span_lists([0], 5, seed=1, garbage=0.0)
    assert e[0].shape == (0, 5, 2)
    got = A.corpus_span_topk(*[t.to(dev) for t in e], k=5)
    same_lists(got, A.corpus_span_topk_torch(*e, k=5), "no groups")
    same_lists(through_ctypes(e, 5, dev), got, "no groups")
    assert got["count"].tolist() == [0] and got["video"].eq(-1).all() and bits(got["span"]).eq(NAN_BITS).all() and got["score"].eq(0).all()
    empty = A.corpus_span_topk(*[t.to(dev) for t in e[:6]], torch.zeros(1, dtype=torch.int32, device=dev), k=5)     # Q = 0
    assert empty["video"].shape == (0, 5) and empty["count"].shape == (0,)
    # rejected before any launch
    L_ = A._lib
    t = [x.to(dev) for x in a]
    outs = [torch.empty(1, 64, dtype=torch.int64, device=dev), torch.empty(1, 64, 2, device=dev), torch.empty(1, 64, device=dev),
            torch.empty(1, 64, dtype=torch.int64, device=dev), torch.empty(1, 64, 2, dtype=torch.int64, device=dev), torch.empty(1, dtype=torch.int32, device=dev)]
    p, o = [L_.ptr(x) for x in t], [L_.ptr(x) for x in outs]
    lib = L_.load()
    f = lib.smin_corpus_span_topk
    assert f(L_.stream(), *p, 1, 5, 0, *o) != 0
    assert f(L_.stream(), *p, 1, 5, 65, *o) != 0
    assert f(L_.stream(), *p, 1, 0, 5, *o) != 0
    assert f(L_.stream(), *p, 1, 65, 5, *o) != 0
    assert f(L_.stream(), *p, -1, 5, 5, *o) != 0
    assert f(L_.stream(), *p[:6], None, 1, 5, 5, *o) != 0
    for j in range(6):
        assert f(L_.stream(), *p, 1, 5, 5, *[None if i == j else x for i, x in enumerate(o)]) != 0, KEYS[j]
    assert f(L_.stream(), *p, 0, 5, 5, *[None] * 6) == 0                             # Q == 0 launches nothing
    torch.cuda.synchronize()


@pytest.fixture(scope="module")
def world(dev):
    """the tiny model, LENGTHS' rows, four ragged queries, the two banks, and the restated search at KW (computed once)"""
    m, _ = tiny_model(dev)
    raw, qf, qm = corpus_rows(SEED)
    raw_d, qf_d, qm_d = raw.to(dev), qf.to(dev), qm.to(dev)
    qb = m.encode_queries(qf_d, qm_d)
    wb = m.encode_windows(raw_d, LENGTHS, WINDOW, STRIDE)
    want = {key: v.cpu() for key, v in m.search_windows_torch(wb, qb, raw_d, duration=DURATION, **KW).items()}
    return dict(m=m, raw=raw_d, qf=qf_d, qm=qm_d, qb=qb, wb=wb, want=want)


@pytest.mark.gpu
@pytest.mark.parametrize("max_batch", [2, 64])
def test_window_bank(dev, world, max_batch):
    A = V()
    m, raw = world["m"], world["raw"]
    assert m._plan(raw.new_empty((0, T, DIN)), world["qf"]) == "node"
    wb = m.encode_windows(raw, LENGTHS, WINDOW, STRIDE, max_batch=max_batch)
    torch.cuda.synchronize()
    again = checked_no_sync(lambda: m.encode_windows(raw, LENGTHS, WINDOW, STRIDE, max_batch=max_batch))     # building the bank reads nothing back
    W = 8
    assert isinstance(wb, A.WindowBank) and len(wb) == W and wb.n_videos == 5 and (wb.window, wb.stride, wb.mode) == (WINDOW, STRIDE, "pick")
    assert wb.start.tolist() == STARTS and wb.len.tolist() == LENS and wb.start.dtype == torch.int64 and wb.len.dtype == torch.int32
    assert wb.video_ptr.tolist() == VPTR and wb.video_ptr_d.tolist() == VPTR and wb.video_ptr_d.dtype == torch.int64 and wb.video_ptr_d.is_cuda
    assert wb.n_rows.tolist() == list(LENGTHS) and wb.starts.tolist() == STARTS and wb.lens.tolist() == LENS
    # each window against encode_videos of sample_windows of its row range
    offs = np.concatenate([[0], np.cumsum(LENGTHS)])
    begin = [int(offs[v]) + STARTS[w] for v in range(5) for w in range(VPTR[v], VPTR[v + 1])]
    vf, nf = A.sample_windows(raw, begin, LENS, T)
    masks = A.build_masks_hip(nf, T, L)
    ref = m.encode_videos(vf, masks["video_mask"], masks["length_mask"], masks["moment_mask"])
    assert tuple(wb.fv.shape) == (W, T, TINY_SHAPE[3]) and torch.equal(bits(wb.fv), bits(ref.fv)) and torch.equal(bits(again.fv), bits(ref.fv))
    vmask, lmask, mmask, cells = host_masks(LENS)
    for name, want, have in (("video_mask", vmask, wb.video_mask), ("length_mask", lmask, wb.length_mask), ("moment_mask", mmask, wb.moment_mask)):
        assert have.shape == want.shape and torch.equal(have.cpu().to(torch.uint8), want.to(torch.uint8)), name
        assert torch.equal(have, getattr(ref, name)), name
    assert wb.cell_counts == tuple(cells) == ref.cell_counts == tuple(A.cell_count(min(n, T), T, L) for n in LENS)
    # on the one-node path the bank holds no (W, T, Din) tensor
    assert wb.video_features is None and tuple(wb.plan_features.shape) == (0, T, DIN)
    assert not any(isinstance(x, torch.Tensor) and tuple(x.shape) == (W, T, DIN) for x in vars(wb).values())
    assert int(A._lib.load_torch().layout_status(dev)[0]) == 0


@pytest.mark.gpu
def test_window_bank_mean_mode(dev, world):
    """windows of 32 rows: two rows per clip, averaged"""
    A = V()
    m, raw = world["m"], world["raw"]
    wb = m.encode_windows(raw, LENGTHS, 32, mode="mean", max_batch=2)
    starts, lens, vptr = (x.tolist() for x in A.window_plan(LENGTHS, 32, 16))
    assert starts == [0, 8, 0, 0, 0] and lens == [32, 32, 16, 9, 23] and vptr == [0, 2, 3, 4, 4, 5]
    assert wb.start.tolist() == starts and wb.len.tolist() == lens and wb.video_ptr.tolist() == vptr and (wb.window, wb.stride, wb.mode) == (32, 16, "mean")
    offs = np.concatenate([[0], np.cumsum(LENGTHS)])
    begin = [int(offs[v]) + starts[w] for v in range(5) for w in range(vptr[v], vptr[v + 1])]
    vf, nf = A.sample_windows(raw, begin, lens, T, mode="mean")
    assert torch.equal(vf[0, 3].cpu(), A.sample_windows_torch(raw, begin[:1], lens[:1], T, mode="mean")[0][0, 3]) and nf.tolist() == [16, 16, 16, 9, 16]
    masks = A.build_masks_hip(nf, T, L)
    ref = m.encode_videos(vf, masks["video_mask"], masks["length_mask"], masks["moment_mask"])
    assert torch.equal(bits(wb.fv), bits(ref.fv)) and torch.equal(wb.moment_mask, ref.moment_mask) and wb.cell_counts == ref.cell_counts
    assert wb.video_features is None


@pytest.mark.gpu
@pytest.mark.parametrize("max_batch", [7, 64])
def test_search_windows_end_to_end(dev, world, max_batch):
    m, wb, qb, want = world["m"], world["wb"], world["qb"], world["want"]
    # the restatement alone: at least three quarters of all listed entries are separated by more than the margin
    sep = separated(want["score"], want["count"])
    listed = int(want["count"].sum())
    print("seed", SEED, "listed", listed, "separated", int(sep.sum()), "counts", want["count"].tolist())
    assert listed >= 16 and int(sep.sum()) >= 0.75 * listed
    got = m.search_windows(wb, qb, duration=DURATION.to(dev), max_batch=max_batch, **KW)
    assert set(got) == {"video", "span", "score", "window", "cell", "count", "times"}
    assert got["video"].shape == (4, 5) and got["span"].shape == (4, 5, 2) and got["cell"].shape == (4, 5, 2) and got["count"].dtype == torch.int32
    _, diff = same_search(got, want)
    print("max_batch", max_batch, "sorted scores against the restatement: max difference", diff)
    restated = m.search_windows_torch(wb, qb, world["raw"], max_batch=max_batch, **KW)      # the restatement's own chunking does not matter either
    same_search(restated, want)
    # the same selection on equal scores: bit for bit
    scorer = lambda wi, wq: m.score_pairs(wb, qb, wi, wq)
    equal = m.search_windows_torch(wb, qb, duration=DURATION, max_batch=max_batch, scorer=scorer, **KW)
    for key in KEYS + ("times",):
        assert torch.equal(got[key].cpu().contiguous().view(torch.uint8), equal[key].cpu().contiguous().view(torch.uint8)), key
    # times: the stated formula on the returned spans, on each entry's own video
    vid, span = got["video"].cpu(), got["span"].cpu()
    n_rows = torch.tensor(LENGTHS, dtype=torch.float32)
    t = (span * DURATION[vid.clamp_min(0)].unsqueeze(-1)) / n_rows[vid.clamp_min(0)].unsqueeze(-1)
    assert torch.equal(bits(got["times"]), bits(t))
    s = got["score"].cpu()
    assert (s[:, :-1] >= s[:, 1:]).all() and (vid != 3).all()
    assert int(V()._lib.load_torch().layout_status(dev)[0]) == 0


@pytest.mark.gpu
def test_listed_pairs_equal_localize_windows(dev, world):
    m, wb, qb = world["m"], world["wb"], world["qb"]
    v_q = [0, 4, 3, 2]                                                              # query 2's video has no rows
    pairs = np.array([(q, v) for q, v in enumerate(v_q)])[[2, 0, 3, 1]]
    got = m.search_windows(wb, qb, pairs=pairs, k=5, k_video=5, k_window=5, max_batch=3)
    want = m.localize_windows(world["raw"], LENGTHS, world["qf"], world["qm"], video_index=v_q, window=WINDOW, stride=STRIDE, k=5, k_window=5, max_batch=3)
    want = {key: v.cpu() for key, v in want.items()}
    assert want["n_windows"].tolist() == [4, 2, 0, 1]
    sep, diff = same_search(got, want, keys=("window", "cell", "span"))
    print("listed pairs against localize_windows: max score difference", diff, "separated", int(sep.sum()), "of", int(want["count"].sum()))
    assert int(sep.sum()) >= 0.5 * int(want["count"].sum())                         # (the comparison is not vacuous)
    n = got["count"].cpu()
    assert n.tolist()[2] == 0 and got["video"][2].eq(-1).all() and torch.isnan(got["span"][2]).all()
    for q in range(4):
        assert got["video"][q, :int(n[q])].eq(v_q[q]).all() and got["video"][q, int(n[q]):].eq(-1).all()


@pytest.mark.gpu
def test_search_windows_reads_nothing_back_and_repeats(dev, world):
    m, wb, qb = world["m"], world["wb"], world["qb"]
    kw = dict(duration=DURATION.to(dev), max_batch=7, **KW)
    first = m.search_windows(wb, qb, **kw)                                           # first use outside the checked region
    torch.cuda.synchronize()
    second = checked_no_sync(lambda: m.search_windows(wb, qb, **kw))
    listed = checked_no_sync(lambda: m.search_windows(wb, qb, pairs=[(3, 4), (0, 2), (2, 3)], **kw))
    for key in KEYS + ("times",):
        assert torch.equal(second[key].cpu().contiguous().view(torch.uint8), first[key].cpu().contiguous().view(torch.uint8)), key
    assert listed["count"].tolist()[1:3] == [0, 0]
    assert m.known_cell_count is None and int(V()._lib.load_torch().layout_status(dev)[0]) == 0


@pytest.mark.gpu
def test_search_windows_with_keep_attention(dev, world):
    """off the one-node path the bank keeps the sampled features and the pairs are expanded and scored by score()"""
    m, qb, want = world["m"], world["qb"], world["want"]
    m.keep_attention = True
    try:
        wb = m.encode_windows(world["raw"], LENGTHS, WINDOW, STRIDE, max_batch=3)
        assert tuple(wb.video_features.shape) == (8, T, DIN) and wb.plan_features is wb.video_features
        got = m.search_windows(wb, qb, duration=DURATION.to(dev), max_batch=7, **KW)
        assert m.smis[0].content_unit.attn_layer.attn_weights.shape[0] == 32 % 7      # the forward ran, on the last chunk's expanded pairs
        with pytest.raises(ValueError, match="keeps no features"):
            m.search_windows(world["wb"], qb, **KW)                                  # a bank of the one-node path has nothing to expand
    finally:
        m.keep_attention = False
    vf, _ = V().sample_windows(world["raw"], [0, 8, 16, 24, 40, 56, 65, 72], LENS, T)
    assert torch.equal(bits(wb.video_features), bits(vf))
    _, diff = same_search(got, want)
    print("keep_attention: sorted scores against the restatement: max difference", diff)
    assert set(got) == {"video", "span", "score", "window", "cell", "count", "times"}


@pytest.mark.gpu
def test_model_corpus_windows_end_to_end(dev, world):
    A = V()
    m, raw = world["m"], world["raw"]
    queries = dict(query_features=world["qf"], query_mask=world["qm"])
    kw = dict(window=WINDOW, stride=STRIDE, k=25, k_video=5)
    r = {key: v.cpu() for key, v in m.search_windows(world["wb"], world["qb"], k=25, k_video=5, duration=DURATION.to(dev)).items()}
    gt_video = np.array([0, 4, 2, 1])
    gt_times = np.stack([np.array([1.0, 20.0, 0.5, 0.0]), np.array([6.0, 70.0, 30.0, 3.0])], axis=1)
    want = A.CorpusMeterTorch(n=(1, 5))
    want.update(r, torch.from_numpy(gt_video), torch.from_numpy(gt_times).float())
    want = want.result()

    class Counting(A.CorpusMeter):
        reads = 0

        def result(self):
            torch.cuda.set_sync_debug_mode(mode)                                     # everything before this point ran without a host read
            Counting.reads += 1
            return super().result()

    A.test_model_corpus_windows(m, raw, LENGTHS, queries, gt_video, gt_times, DURATION.numpy(), **kw)       # first use outside the checked region
    torch.cuda.synchronize()
    mode = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        got = A.test_model_corpus_windows(m, raw, LENGTHS, queries, gt_video, gt_times, DURATION.numpy(), Counting(n=(1, 5), device=dev), **kw)
    finally:
        torch.cuda.set_sync_debug_mode(mode)
    print("test_model_corpus_windows", got)
    assert Counting.reads == 1 and got == want and got["num_samples"] == 4
    for c in (0.1, 0.3, 0.5, 0.7):
        assert got[f"R@1, IoU={c}"] <= got[f"R@5, IoU={c}"]                          # R@n is non-decreasing in n
        for n in (1, 5):
            assert got[f"VR@{n}"] >= got[f"R@{n}, IoU={c}"]                          # the right moment is in the right video
    assert got["VR@1"] <= got["VR@5"]
    # planted truth: rank 1 of each query's list
    top = A.test_model_corpus_windows(m, raw, LENGTHS, queries, r["video"][:, 0].numpy(), r["times"][:, 0].numpy(), DURATION.numpy(), **kw)
    assert all(top[key] == 1.0 for key in top if key != "num_samples"), top
    assert int(A._lib.load_torch().layout_status(dev)[0]) == 0


@pytest.mark.gpu
def test_nothing_else_moved(dev):
    """a train step's scores and gradients, a whole-bank search and localize_windows give the same bits before and after a window search"""
    A = V()
    cfg, sd, batch, _, _, _ = H.split_tiny(H.load_npz(H.TINY[0]))
    import models
    m = models.SMIN(cfg["T"], cfg["L"], cfg["C"], cfg["D"], cfg["dl"], cfg["layers"], cfg["Din"], cfg["Nq"], cfg["H"], dev)
    m.load_state_dict(sd, strict=True)
    m = m.to(dev)
    b = {k: v.to(dev) for k, v in batch.items()}
    xs = H.model_inputs(b)
    B = xs[0].shape[0]
    g = torch.Generator().manual_seed(6)
    lengths = [cfg["T"] + 5, 3, 0, 2 * cfg["T"]]
    raw = torch.randn(sum(lengths), cfg["Din"], generator=g).to(dev)
    vi = [v % 4 for v in range(B)]

    def step():
        m.train()
        m.zero_grad(set_to_none=True)
        out = m(*xs)
        A.loss_fn(out[0], b["ym"], b["sm"], b["moment_mask"], out[1], b["ys"], b["ss"], out[2], b["ye"], b["se"], out[3], b["ya"], b["length_mask"]).backward()
        torch.cuda.synchronize()
        m.eval()
        vb, qb = m.encode_videos(xs[0], xs[1], xs[4], xs[5]), m.encode_queries(xs[2], xs[3])
        r = m.search(vb, qb, k=3, max_batch=3)
        w = m.localize_windows(raw, lengths, xs[2], xs[3], video_index=vi, k=3, max_batch=3)
        sp = m.score_pairs(vb, qb, list(range(B)), list(range(B)))
        return [bits(t) for t in m.score(*xs)] + [bits(t) for t in out] + [bits(p.grad) for p in m.parameters()] + [bits(t) for t in sp] + \
            [r["video"].cpu(), r["idx"].cpu(), bits(r["score"]), r["count"].cpu(), bits(w["span"]), bits(w["score"]), w["cell"].cpu(), w["count"].cpu()]

    before = step()
    wb, qb = m.encode_windows(raw, lengths, max_batch=3), m.encode_queries(xs[2], xs[3])
    r = m.search_windows(wb, qb, k=3, max_batch=3)
    assert r["count"].shape == (B,) and int(r["count"].min()) == 3
    got = A.test_model_corpus_windows(m, raw, lengths, dict(query_features=xs[2], query_mask=xs[3]), vi, np.tile([0.0, 1.0], (B, 1)), np.ones(4), k=10, k_video=2)
    assert got["num_samples"] == B
    after = step()
    assert len(before) == len(after) and all(torch.equal(x, y) for x, y in zip(before, after))
