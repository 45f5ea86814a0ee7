"""Pruning a window search with the first-stage cut: csrc/window_prune.hip smin_window_expand,
moments.expand_survivor_windows and its restatement, moments.survivor_window_capacity, SMIN.search_windows(prefilter=M, trim=...) and
training.test_model_corpus_windows(prefilter=M).

Host: the C ABI surface; expand_survivor_windows_torch against a plain Python loop; the capacity on hand-checked cases; the refusals.
GPU: the kernel against its restatement bit for bit in every output, between canaries, at every tile boundary it has (groups per
query, queries, slots of a group), clamped, rejected and repeated; search_windows(prefilter=M) with trim=True against
search_windows(pairs=the surviving pairs) bit for bit; trim=False against trim=True; M = V against the unpruned search; an int8 bank
against its decoded values; no host read with trim=False; the evaluation loop.

trim=False against trim=True: the two differ only in the length of the chunk that holds the last real slot (the padding rides in it),
and in whole chunks of padding behind it.  They are compared bit for bit at every max_batch."""
import inspect
import os
import re

import numpy as np
import pytest
import torch

from tests.support import corpora as WS
from tests.support.device import dev  # noqa: F401  (the module's device fixture)
from tests.support.device import checked_no_sync, vml as V
from tests.support.compare import byte_bits as bits, same
from tests.support.corpora import host_pairs, tiny_model, window_host_banks, DURATION_TENSOR, KW

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CANARY = 0x5A5A5A5A
BAND = 64
KEYS = WS.KEYS + ("times",)
VIDEO_KEYS = ("video_rank", "video_score", "video_count", "gt_rank")
PF_KEYS = ("prefilter_video", "prefilter_score", "prefilter_gt_rank")
GT_VIDEO = [0, 4, 2, 1]
EQUAL_LENGTHS = (40, 16, 16, 0, 24)                    # window 16, stride 8: 4, 1, 1, 0, 2 windows of 16 rows each -- one cell count


def py_expand(sel, vptr, W, cap):
    """the plan by hand: a Python loop over the groups in (query, video) order"""
    V_ = len(vptr) - 1
    group_ptr, wi, wq = [0], [], []
    for q, row in enumerate(sel):
        for v in row:
            if 0 <= v < V_:
                lo = min(max(vptr[v], 0), W)
                hi = min(max(vptr[v + 1], lo), W)
                wi += list(range(lo, hi))
                wq += [q] * (hi - lo)
            group_ptr.append(len(wi))
    total = len(wi)
    wi, wq = (wi + [0] * cap)[:cap], (wq + [0] * cap)[:cap]
    return [[min(p, cap) for p in group_ptr], wi, wq, [total]]


WORLD_SEL = [[0, 4], [1, 3], [-1, 2], [0, 1]]          # over WS.VPTR (counts 4, 1, 1, 0, 2): a -1 entry, the video without windows


def expand_cases():
    """name -> (sel_video (Q, Ms) int32, video_ptr (V + 1,) int64, W, [caps])"""
    g = torch.Generator().manual_seed(5)
    i32, i64 = (lambda x: torch.tensor(x, dtype=torch.int32)), (lambda x: torch.tensor(x, dtype=torch.int64))
    ptr_of = lambda counts: torch.cat([torch.zeros(1, dtype=torch.int64), counts.to(torch.int64).cumsum(0)])
    cases = {"one": (i32([[0]]), i64([0, 3]), 3, [3, 4])}
    cases["world"] = (i32(WORLD_SEL), i64(WS.VPTR), 8, [13, 24, 7, 0])             # total 13: exact, padded, clamped, no slot
    counts = torch.randint(0, 4, (600,), generator=g)
    sel = torch.stack([torch.randperm(600, generator=g)[:300].sort().values for _ in range(3)]).to(torch.int32)
    cases["groups_past_a_tile"] = (sel, ptr_of(counts), int(counts.sum()), [3 * int(counts.sort().values[-300:].sum())])
    counts = torch.randint(0, 5, (7,), generator=g)
    sel = torch.randint(-1, 9, (1025, 1), generator=g).to(torch.int32)              # -1, 7 and 8 are outside [0, 7)
    cases["queries_past_a_tile"] = (sel, ptr_of(counts), int(counts.sum()), [1025 * int(counts.max()), 1500])
    cases["slots_past_a_tile"] = (i32([[0, 1], [1, 0]]), i64([0, 700, 701]), 701, [1402, 1500, 900, 701])
    cases["no_windows"] = (i32([[0, 1, 2], [2, 1, 0]]), i64([4, 4, 4, 4]), 9, [0, 5])
    cases["not_a_plan"] = (i32([[0, 1, 2], [2, 0, 1]]), i64([5, 2, 100, -3]), 8, [16, 3])   # descending, outside the bank: clamped into it
    return cases


# ---------------------------------------------------------------- host
def test_header_table_and_names():
    A = V()
    text = open(os.path.join(ROOT, "include", "smin_hip.h")).read()
    assert re.search(r"\bint\s+smin_window_expand\s*\(", text)
    assert len(A._lib.SIGNATURES["smin_window_expand"]) == 12 and hasattr(A._lib.load(), "smin_window_expand")
    assert "#define SMIN_HIP_ABI_VERSION 2" in text and A._lib.ABI_VERSION == 2
    for name in ("expand_survivor_windows", "expand_survivor_windows_torch", "survivor_window_capacity"):
        assert callable(getattr(A, name)) and callable(getattr(A.moments, name)), name
    import models
    p = inspect.signature(models.SMIN.search_windows).parameters
    assert p["prefilter"].default is None and p["trim"].default is False
    p = inspect.signature(A.test_model_corpus_windows).parameters
    assert p["prefilter"].default is None and p["trim"].default is False
    with pytest.raises(A._lib.SminHipError, match="no CPU fallback"):
        A.expand_survivor_windows(torch.zeros(1, 1, dtype=torch.int32), torch.tensor([0, 1]), 1, 1)


@pytest.mark.parametrize("name", sorted(expand_cases()))
def test_expand_restatement_against_a_loop(name):
    A = V()
    sel, vptr, W, caps = expand_cases()[name]
    for cap in caps:
        got = A.expand_survivor_windows_torch(sel, vptr, W, cap)
        want = py_expand(sel.tolist(), vptr.tolist(), W, cap)
        assert [t.dtype for t in got] == [torch.int64, torch.int32, torch.int32, torch.int64]
        assert [t.tolist() for t in got] == want, (name, cap)
    if name == "world":
        gp, wi, wq, total = A.expand_survivor_windows_torch(sel, vptr, W, 24)
        assert total.tolist() == [13] and gp.tolist() == [0, 4, 6, 7, 7, 7, 8, 12, 13]
        assert wi.tolist() == [0, 1, 2, 3, 6, 7, 4, 5, 0, 1, 2, 3, 4] + [0] * 11 and wq.tolist() == [0] * 6 + [1] + [2] + [3] * 5 + [0] * 11
        assert A.expand_survivor_windows_torch(sel, vptr, W, 7)[0].tolist() == [0, 4, 6, 7, 7, 7, 7, 7, 7]     # clamped


def test_expand_equals_the_host_plan():
    """group order, window order and pointers are _window_search_plan's for the same pairs sorted by (query, video)"""
    m, _ = tiny_model()
    wb, qb = window_host_banks()
    sel = [[0, 4], [1, 3], [2, 4], [0, 1]]
    pairs = [(q, v) for q, row in enumerate(sel) for v in row]
    _, plan = m._window_search_plan("search_windows", wb, qb, pairs[::-1], 5, None, None, 64, None)
    gp, wi, wq, total = V().expand_survivor_windows_torch(torch.tensor(sel, dtype=torch.int32), wb.video_ptr_d, len(wb), 24)
    n = int(total)
    assert n == len(plan["wi"]) and gp.tolist() == plan["group_ptr"].tolist()
    assert wi[:n].tolist() == plan["wi"].tolist() and wq[:n].tolist() == plan["wq"].tolist()


def test_survivor_window_capacity():
    cap = V().survivor_window_capacity
    assert cap(WS.VPTR, 1, 4) == 16 and cap(WS.VPTR, 2, 4) == 24 and cap(WS.VPTR, 3, 4) == 28 and cap(WS.VPTR, 5, 4) == 32
    assert cap(np.array(WS.VPTR), 9, 1) == 8 and cap(WS.VPTR, 0, 4) == 0 and cap(WS.VPTR, 2, 0) == 0
    assert cap([0, 7, 14, 21], 2, 16) == 224                                         # equal counts: exact
    assert cap([0, 1, 3, 60, 61], 2, 3) == 3 * 59 and cap([0], 3, 2) == 0
    assert cap(torch.tensor([0, 57, 58]), 1, 2) == 114
    with pytest.raises(ValueError, match="must be an integer"):
        cap(WS.VPTR, -1, 4)


def test_refusals_on_the_host():
    A = V()
    m, _ = tiny_model()
    wb, qb = window_host_banks()
    with pytest.raises(ValueError, match="prefilter takes pairs=None and carry=False"):
        m.search_windows(wb, qb, prefilter=2, pairs=[(0, 1)])
    with pytest.raises(ValueError, match="prefilter takes pairs=None and carry=False"):
        m.search_windows(wb, qb, prefilter=2, carry=True)
    for M in (0, -1, 2.0):
        with pytest.raises(ValueError, match="prefilter must be an integer"):
            m.search_windows(wb, qb, prefilter=M)
    plain = A.VideoBank(None, torch.zeros(8, WS.T, WS.DIN), wb.video_mask, wb.length_mask, wb.moment_mask, wb.cell_counts)
    with pytest.raises(ValueError, match="WindowBank"):
        m.search_windows(plain, qb, prefilter=2)
    with pytest.raises(ValueError, match="must be an integer"):
        m.search_windows(wb, qb, prefilter=2, k_window=0)
    with pytest.raises(ValueError, match="duration must be"):
        m.search_windows(wb, qb, prefilter=2, duration=torch.ones(8))
    with pytest.raises(ValueError, match=r"search_windows\(prefilter=M\)"):          # the whole-video search names the method that prunes windows
        m.search(wb, qb, prefilter=2)
    huge = A.WindowBank(None, None, wb.video_mask, wb.length_mask, wb.moment_mask, wb.cell_counts, WS.STARTS, WS.LENS, [0, 2 ** 25, 2 ** 25 + 1],
                        [1, 1], wb.start, wb.len, torch.tensor([0, 2 ** 25, 2 ** 25 + 1]), WS.WINDOW, WS.STRIDE)
    with pytest.raises(ValueError, match="exceed the merges"):
        m.search_windows(huge, qb, prefilter=1, k_window=64)                         # cap * k_window = 4 * 2**25 * 64 = 2**33
    for bad in (dict(W=2 ** 31), dict(cap=-1), dict(cap=2 ** 31), dict(W=-1)):
        with pytest.raises(ValueError, match="must be an integer"):
            A.expand_survivor_windows_torch(torch.zeros(1, 1, dtype=torch.int32), torch.tensor([0, 1]), **{**dict(W=1, cap=1), **bad})
    with pytest.raises(ValueError, match=r"\(Q, Ms\)"):
        A.expand_survivor_windows_torch(torch.zeros(3, dtype=torch.int32), torch.tensor([0, 1]), 1, 1)


# ---------------------------------------------------------------- GPU: the kernel
def buffers(G, cap, dev):
    """the four outputs with BAND canary words behind each: (raw tensors, their real lengths)"""
    sizes = (G + 1, cap, cap, 1)
    dtypes = (torch.int64, torch.int32, torch.int32, torch.int64)
    return [torch.full((n + BAND,), CANARY, dtype=dt, device=dev) for n, dt in zip(sizes, dtypes)], sizes


def raw_expand(sel, vptr, W, cap, dev, Q=None, Ms=None, null=None):
    """smin_window_expand through the C ABI into canaried buffers: (status, outputs cut to their lengths, raw buffers)"""
    L_ = V()._lib
    sel_d, vp_d = sel.to(dev).contiguous(), vptr.to(dev).contiguous()
    Q = sel.shape[0] if Q is None else Q
    Ms = sel.shape[1] if Ms is None else Ms
    raw, sizes = buffers(sel.shape[0] * sel.shape[1], max(cap, 0) if cap < 2 ** 31 else 0, dev)
    args = [L_.ptr(sel_d), L_.ptr(vp_d), Q, Ms, vptr.shape[0] - 1, W, cap] + [L_.ptr(r) for r in raw]
    if null is not None:
        args[null] = None
    with torch.cuda.device(dev):
        rc = L_.load().smin_window_expand(L_.stream(), *args)
    torch.cuda.synchronize()
    for r, n in zip(raw, sizes):
        assert r[n:].eq(CANARY).all(), "written past the end"
    return rc, [r[:n].cpu() for r, n in zip(raw, sizes)], raw


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(expand_cases()))
def test_window_expand_kernel(dev, name):
    A = V()
    sel, vptr, W, caps = expand_cases()[name]
    for cap in caps:
        want = A.expand_survivor_windows_torch(sel, vptr, W, cap)
        total = int(want[3])
        rc, got, _ = raw_expand(sel, vptr, W, cap, dev)
        assert rc == 0
        for g, w, what in zip(got, want, ("group_ptr", "win_index", "win_query", "total")):
            assert g.dtype == w.dtype and torch.equal(g, w), (name, cap, what)
        if cap > total:                                                              # the padding: window 0, query 0
            assert got[1][total:].eq(0).all() and got[2][total:].eq(0).all()
        if cap < total:                                                              # clamped: the canaries behind cap are checked in raw_expand
            assert got[0].max().item() == cap and got[3].item() == total
        again = raw_expand(sel, vptr, W, cap, dev)[1]
        assert all(torch.equal(a, b) for a, b in zip(again, got)), "a second run"
        mine = A.expand_survivor_windows(sel.to(dev), vptr.to(dev), W, cap)         # the Python entry point: the same bits
        assert all(torch.equal(a.cpu(), b) for a, b in zip(mine, got))
    if name == "world":
        assert [int(A.expand_survivor_windows_torch(sel, vptr, W, c)[3]) for c in caps] == [13] * 4 and caps[0] == 13 < caps[1] and caps[2] < 13


@pytest.mark.gpu
def test_window_expand_rejections_leave_the_outputs_untouched(dev):
    sel, vptr, W, _ = expand_cases()["world"]
    for kw in (dict(cap=-1), dict(cap=2 ** 31), dict(W=2 ** 31), dict(W=-1), dict(Q=-1), dict(Ms=-2), dict(null=0), dict(null=1), dict(null=7),
               dict(null=8), dict(null=9), dict(null=10)):
        a = {**dict(W=W, cap=13), **kw}
        rc, _, raw = raw_expand(sel, vptr, a.pop("W"), a.pop("cap"), dev, **a)
        assert rc != 0, kw
        assert all(r.eq(CANARY).all() for r in raw), kw
    # nothing to do: no launch, no write, status 0 -- and the lists may be NULL where there is no slot
    rc, _, raw = raw_expand(sel, vptr, W, 13, dev, Q=0)
    assert rc == 0 and all(r.eq(CANARY).all() for r in raw)
    L_ = V()._lib
    gp, total = torch.full((9,), CANARY, dtype=torch.int64, device=dev), torch.full((1,), CANARY, dtype=torch.int64, device=dev)
    sel_d, vp_d = sel.to(dev), vptr.to(dev)
    rc = L_.load().smin_window_expand(L_.stream(), L_.ptr(sel_d), L_.ptr(vp_d), 4, 2, 5, W, 0, L_.ptr(gp), None, None, L_.ptr(total))
    assert rc == 0 and gp.tolist() == [0] * 9 and total.item() == 13


# ---------------------------------------------------------------- GPU: the pruned search
@pytest.fixture(scope="module")
def world(dev):
    """the tiny model and test_window_search's corpus (5 videos, 8 windows, counts 4, 1, 1, 0, 2; 4 ragged queries) as banks, and a
    corpus of the same counts whose windows all have 16 rows"""
    m, _ = tiny_model(dev)
    raw, qf, qm = WS.corpus_rows(WS.SEED)
    raw_d, qf_d, qm_d = raw.to(dev), qf.to(dev), qm.to(dev)
    qb = m.encode_queries(qf_d, qm_d)
    wb = m.encode_windows(raw_d, WS.LENGTHS, WS.WINDOW, WS.STRIDE)
    eraw = torch.randn(sum(EQUAL_LENGTHS), WS.DIN, generator=torch.Generator().manual_seed(9)).to(dev)
    ewb = m.encode_windows(eraw, EQUAL_LENGTHS, WS.WINDOW, WS.STRIDE)
    return dict(m=m, raw=raw_d, qf=qf_d, qm=qm_d, qb=qb, wb=wb, ewb=ewb, duration=DURATION_TENSOR.to(dev))


def plan_of(wb, video, cap):
    return V().expand_survivor_windows_torch(video.cpu().to(torch.int32), torch.from_numpy(wb.video_ptr), len(wb), cap)


@pytest.mark.gpu
def test_the_world_exercises_the_pruned_search(dev, world):
    """what the comparisons below rest on, from the restatement alone: padding at M = 2, an empty group at M = V, survivors that differ"""
    A = V()
    m, wb, qb = world["m"], world["wb"], world["qb"]
    assert wb.video_ptr.tolist() == WS.VPTR and len(qb) == 4 and wb.cell_count is None
    for M in (1, 2):
        video = m.prefilter_videos(wb, qb, M)["video"]
        cap = A.survivor_window_capacity(wb.video_ptr, M, 4)
        total = int(plan_of(wb, video, cap)[3])
        print("M", M, "survivors", video.tolist(), "cap", cap, "total", total)
        assert len({tuple(row) for row in video.tolist()}) > 1, "every query keeps the same videos"
        if M == 2:
            assert cap == 24 and total < cap, "no padding"
    video = m.prefilter_videos(wb, qb, 5)["video"]
    gp = plan_of(wb, video, 32)[0]
    assert video.tolist() == [[0, 1, 2, 3, 4]] * 4 and int(gp[-1]) == 32 and (gp[1:] == gp[:-1]).sum().item() == 4      # video 3: an empty group
    assert world["ewb"].video_ptr.tolist() == WS.VPTR and world["ewb"].cell_count == 36


@pytest.mark.gpu
@pytest.mark.parametrize("max_batch", [1, 3, 64])
@pytest.mark.parametrize("M", [1, 2, 5])
def test_search_windows_prefilter(dev, world, M, max_batch):
    A = V()
    m, wb, qb, duration = world["m"], world["wb"], world["qb"], world["duration"]
    Q, Vn = 4, 5
    pf = m.prefilter_videos(wb, qb, M, gt_video=GT_VIDEO)
    cap = A.survivor_window_capacity(wb.video_ptr, min(M, Vn), Q)
    gp, _, _, total = plan_of(wb, pf["video"], cap)
    total = int(total)
    # what the comparisons rest on, from the restatement alone
    if M == 2:
        assert cap > total, "no padding"
    if M < Vn:
        assert len({tuple(row) for row in pf["video"].tolist()}) > 1, "every query keeps the same videos"
    else:
        assert (gp[1:] == gp[:-1]).any(), "no empty group"
    for kw in (dict(), dict(video_weight=7.5, max_videos=2, gt_video=GT_VIDEO)):
        base = dict(duration=duration, max_batch=max_batch, **KW, **kw)
        keys = KEYS + (VIDEO_KEYS if kw else ())
        trimmed = m.search_windows(wb, qb, prefilter=M, trim=True, **base)
        assert set(trimmed) == set(keys) | set(PF_KEYS) | {"window_pairs"}
        assert torch.equal(trimmed["prefilter_video"], pf["video"]) and torch.equal(bits(trimmed["prefilter_score"]), bits(pf["score"]))
        assert trimmed["prefilter_gt_rank"].tolist() == (pf["gt_rank"].tolist() if kw else [-1] * Q)
        assert trimmed["window_pairs"].dtype == torch.int64 and trimmed["window_pairs"].tolist() == [total]
        # the same chunks as the host route over the surviving pairs: bit for bit
        want = m.search_windows(wb, qb, pairs=host_pairs(pf["video"]), **base)
        assert set(want) == set(keys)
        same(trimmed, want, keys, ("pairs", M, max_batch, kw))
        for q in range(Q):
            assert set(trimmed["video"][q, :int(trimmed["count"][q])].tolist()) <= set(pf["video"][q].tolist())
        # trim=False: the chunk of the last real slot is longer, chunks of padding follow
        padded = m.search_windows(wb, qb, prefilter=M, trim=False, **base)
        assert set(padded) == set(trimmed)
        diff = (padded["score"] - trimmed["score"]).abs().max().item()
        print("M", M, "max_batch", max_batch, "weighted", bool(kw), "cap", cap, "total", total, "trim=False against trim=True: max score difference", diff)
        same(padded, trimmed, keys + PF_KEYS + ("window_pairs",), ("trim=False", M, max_batch, kw))
        if M == Vn:                                                                  # every video survives: the unpruned search
            same(trimmed, m.search_windows(wb, qb, **base), keys, ("prefilter=V", max_batch, kw))
    assert m.known_cell_count is None


@pytest.mark.gpu
def test_search_windows_prefilter_int8_bank(dev, world):
    m, qb = world["m"], world["qb"]
    wb8 = world["wb"].compact("int8")
    assert wb8.storage == "int8" and wb8.fv.dtype == torch.int8
    kw = dict(prefilter=2, duration=world["duration"], max_batch=3, video_weight=7.5, max_videos=2, gt_video=GT_VIDEO, **KW)
    for trim in (False, True):
        got, want = m.search_windows(wb8, qb, trim=trim, **kw), m.search_windows(wb8.dequantized(), qb, trim=trim, **kw)
        same(got, want, KEYS + VIDEO_KEYS + PF_KEYS + ("window_pairs",), ("int8", trim))
    assert got["count"].sum().item() > 0


@pytest.mark.gpu
def test_search_windows_prefilter_reads_nothing_back(dev, world):
    m, wb, qb = world["m"], world["ewb"], world["qb"]
    assert wb.cell_counts == (36,) * 8
    kw = dict(prefilter=2, duration=world["duration"], max_batch=3, **KW)
    weighted = dict(video_weight=7.5, max_videos=1, gt_video=GT_VIDEO, **kw)
    first, first_w = m.search_windows(wb, qb, **kw), m.search_windows(wb, qb, **weighted)          # first use outside the checked region
    torch.cuda.synchronize()
    second, second_w = checked_no_sync(lambda: (m.search_windows(wb, qb, **kw), m.search_windows(wb, qb, **weighted)))
    same(second, first, KEYS + PF_KEYS + ("window_pairs",), "second run")
    same(second_w, first_w, KEYS + VIDEO_KEYS + PF_KEYS + ("window_pairs",), "second weighted run")
    assert int(V()._lib.load_torch().layout_status(dev)[0]) == 0                     # the handed-over counts matched the masks, padding included
    assert m.known_cell_count is None
    cap, total = 24, int(first["window_pairs"])
    print("equal windows: cap", cap, "total", total)
    same(first, m.search_windows(wb, qb, pairs=host_pairs(first["prefilter_video"]), duration=world["duration"], max_batch=3, **KW), KEYS, "equal windows")
    with pytest.raises(RuntimeError, match="synchroniz"):                            # trim=True is the documented host read
        checked_no_sync(lambda: m.search_windows(wb, qb, trim=True, **kw))


@pytest.mark.gpu
def test_model_corpus_windows_prefilter(dev, world):
    A = V()
    m, raw, wb, qb = world["m"], world["raw"], world["wb"], world["qb"]
    queries = dict(query_features=world["qf"], query_mask=world["qm"])
    gt_video = np.array(GT_VIDEO)
    gt_times = np.stack([np.array([1.0, 20.0, 0.5, 0.0]), np.array([6.0, 70.0, 30.0, 3.0])], axis=1)
    kw = dict(window=WS.WINDOW, stride=WS.STRIDE, k=25, k_video=5)

    def totals(r):
        meter = A.CorpusMeterTorch(n=(1, 5))
        meter.update({key: v.cpu() for key, v in r.items()}, torch.from_numpy(gt_video), torch.from_numpy(gt_times).float())
        return meter.result()

    args = (m, raw, WS.LENGTHS, queries, gt_video, gt_times, DURATION_TENSOR.numpy())
    for M in (1, 2):
        pf = m.prefilter_videos(wb, qb, M, gt_video=GT_VIDEO)
        by_hand = totals(m.search_windows(wb, qb, pairs=host_pairs(pf["video"]), k=25, k_video=5, duration=world["duration"]))
        rank_meter, want_rank = A.VideoRankMeter(n=(M,), device=dev), A.VideoRankMeter(n=(M,), device=dev)
        want_rank.update(pf["gt_rank"])
        for trim in (False, True):
            got = A.test_model_corpus_windows(*args, prefilter=M, trim=trim, **kw)
            assert got == by_hand and got["num_samples"] == 4, (M, trim)
        assert A.test_model_corpus_windows(*args, prefilter=M, video_meter=rank_meter, **kw) == by_hand
        assert rank_meter.result() == want_rank.result()
    plain = totals(m.search_windows(wb, qb, k=25, k_video=5, duration=world["duration"]))
    assert A.test_model_corpus_windows(*args, prefilter=None, **kw) == plain == A.test_model_corpus_windows(*args, **kw)
    assert int(A._lib.load_torch().layout_status(dev)[0]) == 0
