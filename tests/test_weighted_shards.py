"""Sharded corpus search with the video-level score: shard lists that carry their unweighted scores and their
(query, video) pooled scores, merged under the corpus-wide video weights and ranks by smin_search_merge_weighted /
smin_span_search_merge_weighted.

Host: the torch restatements, whole corpus against shards at once and folded (0 mismatches), refusals, exports.
GPU: the kernels against the restatement bit for bit over sentinels and twice, the rejections, and the model-level loops against the
one-bank weighted search."""
import ctypes
import itertools
import multiprocessing as mp
import os
import re

import numpy as np
import pytest
import torch

from tests.support import corpora as WS
from tests.support.device import dev  # noqa: F401  (the module's device fixture)
from tests.support.device import checked_no_sync, free_port, to_cpu, to_dev, vml as V
from tests.support.compare import bits
from tests.support.guards import WORD_SENTINEL as SENTINEL
from tests.support.corpora import corpus_inputs, shard_dicts, tiny_model, video_shards, DURATION, GT_TIMES, SHARD_SPLITS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NV, NQ, KV = 7, 3, 3
SPLITS = ([3, 4], [1, 1, 5], [7], [2, 2, 2, 1])
RAW_VALUES = torch.tensor([0.0, -0.0, 0.25, 0.5, 0.75])                                # both zeros: exact ties under any weight
POOLED = torch.tensor([0.05, 0.2, 0.35, 0.5, 0.8])                                     # well separated: exp(alpha * 0.15) is far from 1
ALPHAS = (0.0, 7.5, -2.0)
CUTS = (None, 1, 2, 99)
IDX_KEYS = ("video", "idx", "score", "raw", "count")
SPAN_KEYS = ("video", "span", "score", "raw", "window", "cell", "count")
RANK_KEYS = ("video_rank", "video_score", "video_count", "gt_rank")
TALLY = {"cases": 0, "mismatches": 0}


def same(got, want, keys, what=""):
    for key in keys:
        assert got[key].dtype == want[key].dtype and got[key].shape == want[key].shape, (what, key, got[key].dtype, want[key].dtype)
        assert torch.equal(got[key].cpu().contiguous().view(torch.uint8), want[key].cpu().contiguous().view(torch.uint8)), (what, key)


def equal_lists(got, want, keys):
    return all(got[key].shape == want[key].shape and torch.equal(got[key].contiguous().view(torch.uint8), want[key].contiguous().view(torch.uint8))
               for key in keys)


# ---------------------------------------------------------------- host: surface
def test_header_library_and_package_declare_the_weighted_merges():
    A = V()
    sig = A._lib.SIGNATURES
    assert len(sig["smin_search_merge_weighted"]) == 19 and len(sig["smin_span_search_merge_weighted"]) == 23
    with open(os.path.join(ROOT, "include", "smin_hip.h")) as f:
        header = f.read()
    assert re.search(r"#define SMIN_HIP_ABI_VERSION 2\b", header) and A._lib.ABI_VERSION == 2      # exports only
    lib = A._lib.load()
    assert lib.smin_search_merge_weighted and lib.smin_span_search_merge_weighted
    for name in ("merge_search_weighted", "merge_search_weighted_torch", "merge_search_windows_weighted", "merge_search_windows_weighted_torch",
                 "search_shards_weighted", "search_window_shards_weighted", "test_model_corpus_weighted_shards",
                 "test_model_corpus_window_shards_weighted"):
        assert callable(getattr(A, name)), name
    assert callable(A.distributed.gather_search_weighted) and callable(A.distributed.gather_search_windows_weighted)
    for fn in (A.SMIN.search, A.SMIN.search_windows):
        assert fn.__kwdefaults__ is None and fn.__defaults__[-1] is False and fn.__code__.co_varnames[fn.__code__.co_argcount - 1] == "carry"


# ---------------------------------------------------------------- host: the corpus of the exactness check
def corpus(seed, spans):
    """Every (query, video) pair's moment list, query-major, and its pooled score and cell count: raw scores from RAW_VALUES in
    descending order within a pair, counts in [-1, KV + 1] with NaN and -1 behind them, pooled scores from POOLED; video 4 has no cells
    (and so no moment) for every query, video 2 none for query 1."""
    g = torch.Generator().manual_seed(seed)
    P = NQ * NV
    score = RAW_VALUES[torch.randint(0, 5, (P, KV), generator=g)]
    score = torch.gather(score, 1, torch.where(score == 0, torch.zeros_like(score), score).sort(dim=1, descending=True, stable=True).indices)
    count = torch.randint(-1, KV + 2, (P,), generator=g, dtype=torch.int32)
    pooled = POOLED[torch.randint(0, 5, (P,), generator=g)]
    cells = torch.randint(1, 30, (P,), generator=g).float()
    for q, v in [(q, 4) for q in range(NQ)] + [(1, 2)]:
        cells[q * NV + v], pooled[q * NV + v], count[q * NV + v] = 0.0, 0.0, 0
    unused = torch.arange(KV).unsqueeze(0) >= count.unsqueeze(1)
    nan = float("nan")
    slot = torch.arange(KV, dtype=torch.int64).expand(P, KV)                             # a field that makes each entry of a pair distinct
    a = torch.randint(0, 9, (P, KV), generator=g, dtype=torch.int64)
    lists = {"score": torch.where(unused, torch.full_like(score, nan), score), "count": count}
    if spans:
        span = torch.rand(P, KV, 2, generator=g) * 100
        lists.update(span=torch.where(unused.unsqueeze(2), torch.full_like(span, nan), span), window=torch.where(unused, torch.full_like(a, -1), a),
                     cell=torch.where(unused.unsqueeze(2), torch.full((P, KV, 2), -1, dtype=torch.int64), torch.stack([a + 3, slot], dim=2)))
    else:
        lists.update(idx=torch.where(unused.unsqueeze(2), torch.full((P, KV, 2), -1, dtype=torch.int64), torch.stack([a, slot + 9], dim=2)))
    return lists, pooled, cells


def ranked(lists, pooled, cells, v0, v1, K, alpha, cut, n, gt, spans, carry):
    """search(video_weight=alpha, max_videos=cut) restated over the videos v0 .. v1 of the corpus, numbered from 0: rank_videos_torch ->
    reweight_moments_torch -> corpus_topk_torch / corpus_span_topk_torch; with ``carry`` also raw and the pooled matrices."""
    A = V()
    nv = v1 - v0
    rows = torch.tensor([q * NV + v for q in range(NQ) for v in range(v0, v1)], dtype=torch.int64)
    video = torch.arange(nv, dtype=torch.int32).repeat(NQ)
    ptr = torch.arange(NQ + 1, dtype=torch.int32) * nv
    gt_t = None if gt is None else torch.tensor(gt, dtype=torch.int32)
    vr = A.rank_videos_torch(pooled[rows], cells[rows], video, ptr, n=n, alpha=alpha, gt_video=gt_t)
    sub = {key: t[rows] for key, t in lists.items()}
    w_score, w_count = A.reweight_moments_torch(sub["score"], sub["count"], vr["pair_rank"], vr["weight"], cut)
    if spans:
        r = A.corpus_span_topk_torch(sub["span"], w_score, sub["window"], sub["cell"], w_count, video, ptr, k=K)
    else:
        r = A.corpus_topk_torch(w_score, sub["idx"], w_count, video, ptr, k=K)
    r.update(video_rank=vr["video"], video_score=vr["score"], video_count=vr["count"], gt_rank=vr["gt_rank"])
    if carry:
        fields = ((r["window"].unsqueeze(-1), r["cell"]), (sub["window"].unsqueeze(-1), sub["cell"])) if spans else ((r["idx"],), (sub["idx"],))
        r["raw"] = A.retrieval._carry_raw(r["video"], *fields, sub["score"], sub["count"], nv)
        r["pair_score"], r["pair_cells"] = pooled[rows].reshape(NQ, nv), cells[rows].reshape(NQ, nv)
    return r


def precondition_holds(lists, pooled, alpha):
    """No two of a query's candidate values are near-ties: two candidates either have the same |raw| and the same pooled score (an exact
    tie under ANY weight: the tie rules decide) or a zero raw score each, or their values raw * exp(alpha * s) differ by more than 1e-4
    of the larger -- a thousand times what fp32 rounding of the weight and the product can move.  At alpha = 0 every weight is exactly 1
    and nothing is asked of the inputs."""
    for q in range(NQ if alpha != 0.0 else 0):
        cand = set()
        for v in range(NV):
            p = q * NV + v
            for s in range(max(min(int(lists["count"][p]), KV), 0)):
                cand.add((abs(float(lists["score"][p, s])), float(pooled[p])))
        for (ra, sa), (rb, sb) in itertools.combinations(sorted(cand), 2):
            va, vb = ra * np.exp(alpha * sa), rb * np.exp(alpha * sb)
            if (ra == 0 and rb == 0) or abs(va - vb) > 1e-4 * max(va, vb):
                continue
            return False
    return True


@pytest.mark.parametrize("spans", [False, True], ids=["cells", "spans"])
@pytest.mark.parametrize("K", [1, 3, 5, 9])
@pytest.mark.parametrize("split", SPLITS, ids=str)
def test_sharding_is_exact(split, K, spans):
    """The whole corpus against its shards, at once and folded, over alpha, the cut and two seeds: every key of the merged carry is the
    one-bank list's, bit for bit, and the video ranking too; raw is what the whole corpus' entries had before the weight."""
    A = V()
    merge = A.merge_search_windows_weighted_torch if spans else A.merge_search_weighted_torch
    keys = [k for k in (SPAN_KEYS if spans else IDX_KEYS) if k != "raw"]
    edges = np.concatenate([[0], np.cumsum(split)]).tolist()
    gt = [edges[q % len(split)] for q in range(NQ)]                                    # a query's own video in each of the first shards
    for seed, alpha, cut in itertools.product((1, 2), ALPHAS, CUTS):
        lists, pooled, cells = corpus(seed, spans)
        assert precondition_holds(lists, pooled, alpha)
        whole = ranked(lists, pooled, cells, 0, NV, K, alpha, cut, 3, gt, spans, carry=True)
        assert int(whole["count"].max()) >= 1
        slots = A.moments.carry_slots(K, KV, cut)                                      # K without a cut; what the cut needs (3u) with one
        shards = [ranked(lists, pooled, cells, a, b, slots, alpha, cut, 3, None, spans, carry=True) for a, b in zip(edges[:-1], edges[1:])]
        kw = dict(video_weight=alpha, max_videos=cut, n_videos=3, gt_video=gt)
        at_once = merge(shards, edges[:-1], k=K, **kw)
        carry = merge(shards[:1], [0], k=slots, **kw)
        for r, off in zip(shards[1:], edges[1:-1]):
            carry = merge([carry, r], [0, off], k=slots, **kw)
        for got in (at_once, A.moments.truncate_search(carry, K)):
            TALLY["cases"] += 1
            ok = equal_lists(got, whole, keys + list(RANK_KEYS) + ["raw", "pair_score", "pair_cells"])
            TALLY["mismatches"] += not ok
            assert ok, (seed, alpha, cut)
    print("weighted sharding: cases compared so far", TALLY["cases"], "mismatches", TALLY["mismatches"])
    assert TALLY["mismatches"] == 0


def test_fold_search_takes_the_weighted_merge_through_a_closure():
    A = V()
    lists, pooled, cells = corpus(5, False)
    slots = A.moments.carry_slots(5, KV, 2)
    assert slots == 8 and A.moments.carry_slots(5, KV) == 5 and A.moments.carry_slots(9, KV, 99) == 64
    shards = [ranked(lists, pooled, cells, v, v + 1, slots, 7.5, 2, 3, None, False, carry=True) for v in range(NV)]
    whole = ranked(lists, pooled, cells, 0, NV, 5, 7.5, 2, 3, None, False, carry=True)
    bound = lambda ls, off, k: A.merge_search_weighted_torch(ls, off, k=k, video_weight=7.5, max_videos=2, n_videos=3)
    got = A.moments.truncate_search(A.moments.fold_search(shards, list(range(NV)), slots, bound), 5)
    same(got, whole, IDX_KEYS + RANK_KEYS[:3] + ("pair_score", "pair_cells"), "fold_search")
    # the tables it is given: a rank table that names no video leaves every query empty
    none = A.merge_search_weighted_torch(shards, list(range(NV)), k=5, tables=(torch.full((NQ, NV), -1, dtype=torch.int32), torch.ones(NQ, NV)))
    assert none["count"].tolist() == [0] * NQ and int(none["video"].max()) == -1 and not none["raw"].any()


def test_refusals():
    A = V()
    lists, pooled, cells = corpus(1, False)
    a = ranked(lists, pooled, cells, 0, 3, 5, 0.0, None, 3, None, False, carry=True)
    b = ranked(lists, pooled, cells, 3, 7, 5, 0.0, None, 3, None, False, carry=True)
    sl, sp, sc = corpus(1, True)
    c = ranked(sl, sp, sc, 0, 7, 5, 0.0, None, 3, None, True, carry=True)
    for merge, x, y in ((A.merge_search_weighted_torch, a, b), (A.merge_search_weighted, a, b), (A.merge_search_windows_weighted_torch, c, c),
                        (A.merge_search_windows_weighted, c, c)):
        for key in ("raw", "pair_score", "pair_cells"):
            with pytest.raises(ValueError, match="carry=True"):
                merge([{k_: v for k_, v in x.items() if k_ != key}], [0])
        with pytest.raises(ValueError, match="tile"):
            merge([x, y], [0, x["pair_score"].shape[1] + 1])                               # a gap
        with pytest.raises(ValueError, match="tile"):
            merge([x, y], [0, 0])                                                       # an overlap
        with pytest.raises(ValueError, match="tile"):
            merge([x], [2])                                                             # not from 0
        with pytest.raises(ValueError, match="1..16"):
            merge([x] * 17, [0] * 17)
        with pytest.raises(ValueError, match="k <= 64"):
            merge([x], [0], k=0)
        with pytest.raises(ValueError, match="max_videos"):
            merge([x], [0], max_videos=-1)
        with pytest.raises(ValueError, match="n_videos"):
            merge([x], [0], n_videos=65)
        with pytest.raises(ValueError, match="finite"):
            merge([x], [0], video_weight=float("inf"))
        with pytest.raises(ValueError, match="pair_score"):
            merge([dict(x, pair_cells=x["pair_cells"][:, :1])], [0])
    with pytest.raises(A._lib.SminHipError, match="HIP device only"):
        A.merge_search_weighted([a, b], [0, 3])
    with pytest.raises(A._lib.SminHipError, match="HIP device only"):
        A.merge_search_windows_weighted([c], [0])
    for search in (A.retrieval._Retrieval.search, A.retrieval._Retrieval.search_windows):
        with pytest.raises(ValueError, match="carry=True takes pairs=None"):
            search(None, None, None, pairs=[[0, 0]], carry=True)
    with pytest.raises(ValueError, match="carry=True"):
        A.distributed.gather_search_weighted({k_: v for k_, v in a.items() if k_ != "raw"})
    with pytest.raises(ValueError, match="num_videos"):
        A.distributed.gather_search_weighted(a, 4, merge=A.merge_search_weighted_torch)
    alone = A.distributed.gather_search_weighted(a, merge=A.merge_search_weighted_torch)  # no process group: the rank's own list, merged alone
    same(alone, a, IDX_KEYS, "gather alone")


def test_the_cut_needs_the_extra_slots():
    """Why carry_slots: shard lists of only K entries, cut by the shard's own best M videos, can hold entries of videos the corpus-wide
    rank drops in place of entries that stay.  Seed 1, split [3, 4], K = 1, M = 2, alpha = 0: query 0's shard 0 lists video 0 (a tie
    with video 2 at 0.75, the lower video first), the corpus' best two videos are 2 and 5, and the merge is left with video 5's 0.25."""
    A = V()
    lists, pooled, cells = corpus(1, False)
    whole = ranked(lists, pooled, cells, 0, NV, 1, 0.0, 2, 3, None, False, carry=True)
    short = [ranked(lists, pooled, cells, a, b, 1, 0.0, 2, 3, None, False, carry=True) for a, b in ((0, 3), (3, 7))]
    got = A.merge_search_weighted_torch(short, [0, 3], k=1, max_videos=2, n_videos=3)
    assert (whole["video"][0, 0], float(whole["score"][0, 0])) == (2, 0.75) and (got["video"][0, 0], float(got["score"][0, 0])) == (5, 0.25)
    enough = [ranked(lists, pooled, cells, a, b, A.moments.carry_slots(1, KV, 2), 0.0, 2, 3, None, False, carry=True) for a, b in ((0, 3), (3, 7))]
    same(A.merge_search_weighted_torch(enough, [0, 3], k=1, max_videos=2, n_videos=3), whole, IDX_KEYS, "with carry_slots")


# ---------------------------------------------------------------- host: two gloo ranks
GLOO = dict(K=5, seed=4, split=[3, 4], alpha=7.5, cut=2, gt=[0, 3, 6])


def _gloo_shards(spans):
    c = GLOO
    lists, pooled, cells = corpus(c["seed"], spans)
    slots = V().moments.carry_slots(c["K"], KV, c["cut"])
    edges = np.concatenate([[0], np.cumsum(c["split"])]).tolist()
    shards = [ranked(lists, pooled, cells, a, b, slots, c["alpha"], c["cut"], 3, None, spans, carry=True) for a, b in zip(edges[:-1], edges[1:])]
    return shards, edges[:-1], ranked(lists, pooled, cells, 0, NV, c["K"], c["alpha"], c["cut"], 3, c["gt"], spans, carry=True)


def _gather_worker(rank, world, port, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), WORLD_SIZE=str(world), RANK=str(rank), LOCAL_RANK=str(rank))
    torch.set_num_threads(2)
    A = V()
    D = A.distributed
    D.init(backend="gloo")
    c = GLOO
    kw = dict(k=c["K"], video_weight=c["alpha"], n_videos=3, gt_video=c["gt"])
    out = {}
    for spans, gather, merge in ((False, D.gather_search_weighted, A.merge_search_weighted_torch),
                                 (True, D.gather_search_windows_weighted, A.merge_search_windows_weighted_torch)):
        shards, _, _ = _gloo_shards(spans)
        got = gather(shards[rank], max_videos=c["cut"], merge=merge, **kw)
        refused = 0
        for bad in (dict(max_videos=c["cut"] + rank), dict(max_videos=c["cut"], num_videos=c["split"][rank] + rank)):
            try:
                gather(shards[rank], merge=merge, **dict(kw, **bad))
            except ValueError as e:
                refused += "every rank" in str(e)
        out[spans] = (refused, {key: v.numpy() for key, v in got.items()})
    D.barrier()
    q.put((rank, out))
    torch.distributed.destroy_process_group()


@pytest.mark.timeout(300)
def test_two_gloo_ranks_return_the_one_bank_list():
    """Each of two ranks holds the carry list of its shard ([3, 4] of the 7 videos): gather_search_weighted and the window form return
    the one-bank weighted list on both, bitwise equal in every key; ranks that pass different max_videos, or a num_videos that is not
    their matrices' width, raise ValueError on both."""
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = free_port()
    procs = [ctx.Process(target=_gather_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = sorted([q.get(timeout=240) for _ in procs], key=lambda x: x[0])
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    for spans in (False, True):
        _, _, whole = _gloo_shards(spans)
        keys = (SPAN_KEYS if spans else IDX_KEYS) + RANK_KEYS + ("pair_score", "pair_cells")
        assert int(whole["video"].max()) >= 3                                           # the second rank's videos are listed, with their offset
        for rank, out in res:
            refused, got = out[spans]
            assert refused == 2, (rank, spans)
            for key in keys:
                assert got[key].tobytes() == whole[key].numpy().tobytes() == res[0][1][spans][1][key].tobytes(), (rank, spans, key)


# ---------------------------------------------------------------- GPU: the kernels against the restatement
def carry_lists(ks, Q, seed, spans, empty_query=None, full_query=None):
    """len(ks) lists in NO particular order: raw scores from a few values and random, local videos in [-2, 8) (a negative id inside a
    count: g outside [0, V)), counts in [-1, k_s + 1], NaN and -1 behind them."""
    g = torch.Generator().manual_seed(seed)
    values = torch.tensor([0.9, 0.5, 0.25, 0.0, -0.0, 1e-3, -0.5])
    out = []
    for k in ks:
        raw = torch.where(torch.rand(Q, k, generator=g) < 0.5, values[torch.randint(0, 7, (Q, k), generator=g)], torch.rand(Q, k, generator=g))
        video = torch.randint(-2, 8, (Q, k), generator=g, dtype=torch.int64)
        count = torch.randint(-1, k + 2, (Q,), generator=g, dtype=torch.int32)
        if empty_query is not None and empty_query < Q:
            count[empty_query] = [0, -1][len(out) % 2]
        if full_query is not None:
            count[full_query] = k
        unused = torch.arange(k).unsqueeze(0) >= count.unsqueeze(1)
        nan = float("nan")
        a = torch.randint(0, 64, (Q, k, 2), generator=g, dtype=torch.int64)
        r = {"video": torch.where(unused, torch.full_like(video, -1), video), "raw": torch.where(unused, torch.full_like(raw, nan), raw),
             "score": torch.where(unused, torch.full_like(raw, nan), raw * 0.5), "count": count}
        if spans:
            r.update(span=torch.where(unused.unsqueeze(2), torch.full((Q, k, 2), nan), torch.rand(Q, k, 2, generator=g) * 100),
                     window=torch.where(unused, torch.full_like(video, -1), torch.randint(0, 9, (Q, k), generator=g, dtype=torch.int64)),
                     cell=torch.where(unused.unsqueeze(2), torch.full_like(a, -1), a))
        else:
            r.update(idx=torch.where(unused.unsqueeze(2), torch.full_like(a, -1), a))
        out.append(r)
    return out


def video_tables(Q, Vn, seed, reverse):
    """a rank table with -1 entries and a weight table: random, or descending in the video so that the lists' order is reversed"""
    g = torch.Generator().manual_seed(seed)
    rank = torch.stack([torch.randperm(Vn, generator=g) for _ in range(Q)]).to(torch.int32)
    rank = torch.where(torch.rand(Q, Vn, generator=g) < 0.2, torch.full_like(rank, -1), rank)
    weight = torch.rand(Q, Vn, generator=g) * 3 if not reverse else (1.0 / (1.0 + torch.arange(Vn).float())).expand(Q, Vn).contiguous()
    return rank, weight


SHAPES = dict(video=(), idx=(2,), span=(2,), score=(), raw=(), window=(), cell=(2,))
WIDE = ("video", "idx", "window", "cell")                                               # int64 fields


def through_ctypes(lists, offsets, K, rank, weight, Vn, cut, dev, spans, expect=0, fill=None):
    """the C entry point into buffers pre-filled with a sentinel and four spare words behind each; returns (status, outputs, buffers)"""
    L_ = V()._lib
    lib = L_.load()
    S, Q = len(lists), lists[0]["video"].shape[0]
    order = ("video", "span", "raw", "window", "cell", "count") if spans else ("video", "idx", "raw", "count")
    cols = [[r[key].to(dev).contiguous() for r in lists] for key in order]
    tables = [(ctypes.c_void_p * S)(*[t.data_ptr() for t in col]) for col in cols]
    k_list = (ctypes.c_int32 * S)(*[r["video"].shape[1] for r in lists])
    off = (ctypes.c_int64 * S)(*offsets)
    out_keys = SPAN_KEYS if spans else IDX_KEYS
    shapes = {key: (Q,) if key == "count" else (Q, K) + SHAPES[key] for key in out_keys}
    words = {key: (2 if key in WIDE else 1) * int(np.prod(s)) for key, s in shapes.items()}
    buf = {key: torch.full((n + 4,), SENTINEL, dtype=torch.int32, device=dev) for key, n in words.items()}
    rank_d, weight_d = rank.to(dev).contiguous(), weight.to(dev).contiguous()
    name = "smin_span_search_merge_weighted" if spans else "smin_search_merge_weighted"
    args = [L_.stream(), S, *[ctypes.cast(t, ctypes.c_void_p) for t in tables], ctypes.cast(k_list, ctypes.c_void_p), ctypes.cast(off, ctypes.c_void_p),
            L_.ptr(rank_d), L_.ptr(weight_d), Vn, cut, Q, K, *[L_.ptr(buf[key]) for key in out_keys]]
    if fill is not None:
        fill(args, cols, buf)
    rc = getattr(lib, name)(*args)
    torch.cuda.synchronize()
    assert (rc == 0) == (expect == 0), (name, rc)
    out = {}
    for key in out_keys:
        assert buf[key][words[key]:].eq(SENTINEL).all(), key + ": written past the end"
        body = buf[key][:words[key]].cpu()
        if rc != 0:
            assert body.eq(SENTINEL).all(), key + ": a rejected call wrote"
            continue
        out[key] = (body.view(torch.int64) if key in WIDE else body.view(torch.float32) if key != "count" else body).reshape(shapes[key])
    return rc, out


K_LISTS = {1: ([3], [64]), 2: ([1, 64], [3, 3]), 3: ([64, 1, 3],), 16: ([64] * 16, [1, 3, 64] * 5 + [3])}
V_OF = {1: (1, 9), 2: (7, 70), 3: (33,), 16: (38, 40)}                                   # V from 1 to 70: g = local + 2 * s reaches 37


@pytest.mark.gpu
@pytest.mark.parametrize("spans", [False, True], ids=["cells", "spans"])
@pytest.mark.parametrize("S", [1, 2, 3, 16])
@pytest.mark.parametrize("K", [1, 5, 64])
def test_merge_kernel_bit_exact(dev, S, K, spans):
    """The kernel against the restated sort on every output, Q = 1 and 5, over sentinels and twice: lists in no order, weights that
    reverse a list's order, rank -1 videos, global videos below 0 and at or above V, the cut at 0 / 1 / 2 / 99, counts below 0 and above
    k_s, a query with every list empty, NaN and -1 behind the counts; S = 16 with every k_s = 64 and a full query is the whole
    1024-word stage."""
    A = V()
    M = A.moments
    fields = M._WEIGHTED_SPAN_FIELDS if spans else M._WEIGHTED_SEARCH_FIELDS
    keys = SPAN_KEYS if spans else IDX_KEYS
    offsets = [2 * s for s in range(S)]
    n = 0
    for ks, Vn in zip(K_LISTS[S], V_OF[S]):
        for Q, cut in itertools.product((1, 5), (0, 1, 2, 99)):
            n += 1
            lists = carry_lists(ks, Q, seed=1000 * S + 10 * K + Q + cut, spans=spans, empty_query=2, full_query=0)
            rank, weight = video_tables(Q, Vn, seed=n, reverse=cut in (0, 2))
            if cut == 99 and Q == 5:
                rank = rank.clamp_min(0)                                                # every video a candidate: the full stage survives
            want = M._merge_weighted_torch(lists, offsets, Q, K, fields, rank, weight, Vn, cut)
            assert Q == 1 or int(want["count"][2]) == 0
            for again in range(2):
                rc, got = through_ctypes(lists, offsets, K, rank, weight, Vn, cut, dev, spans)
                same(got, want, keys, (ks, Q, cut, "ctypes", again))
            got = M._merge_weighted("test", [to_dev(r, dev) for r in lists], offsets, Q, K, fields, rank.to(dev), weight.to(dev), Vn, cut)
            same(got, want, keys, (ks, Q, cut, "_merge_weighted"))
            if S == 16 and ks == [64] * 16 and cut == 99 and Q == 5:
                assert int(want["count"][0]) == min(K, 64)
    # V == 0: no video table is read, every query comes out empty
    lists = carry_lists([3], 2, seed=7, spans=spans)
    empty = M._merge_weighted("test", [to_dev(r, dev) for r in lists], [0], 2, K, fields, torch.empty((2, 0), dtype=torch.int32, device=dev),
                              torch.empty((2, 0), device=dev), 0, 0)
    assert empty["count"].tolist() == [0, 0] and int(empty["video"].max()) == -1


@pytest.mark.gpu
@pytest.mark.parametrize("spans", [False, True], ids=["cells", "spans"])
@pytest.mark.parametrize("S", [1, 2, 16])
@pytest.mark.parametrize("K", [1, 64])
def test_merge_kernel_nan_scores_full_cuts_and_no_videos(dev, S, K, spans):
    """What test_merge_kernel_bit_exact leaves out, every output against the restatement: a NaN raw score inside the counts (NaN under
    any weight: the highest order word) and, for spans, a NaN span with a payload of its own; ranks that all lie behind the cut, so
    every candidate drops out; and V == 0, where no video table exists.  k_s mixing 1 and 64, Q = 1 and 3."""
    M = V().moments
    fields = M._WEIGHTED_SPAN_FIELDS if spans else M._WEIGHTED_SEARCH_FIELDS
    keys = SPAN_KEYS if spans else IDX_KEYS
    ks, offsets, Vn = [(64, 1)[s % 2] for s in range(S)], [2 * s for s in range(S)], 8 + 2 * S
    for Q in (1, 3):
        lists = carry_lists(ks, Q, seed=50 * S + Q, spans=spans, full_query=0)
        for r in lists:
            r["raw"][:, 0] = float("nan")
            r["video"][:, 0] = 1
            if spans:
                r["span"].view(torch.int32)[:, 0, 0] = 0x7FC12345
        rank, weight = video_tables(Q, Vn, seed=S, reverse=False)
        rank = rank.clamp_min(0)
        on = [to_dev(r, dev) for r in lists]
        for what, (rk, cut, vn) in dict(nan=(rank, 99, Vn), cut=(rank + 2, 2, Vn), none=(rank[:, :0], 0, 0)).items():
            wt = weight[:, :vn]
            want = M._merge_weighted_torch(lists, offsets, Q, K, fields, rk, wt, vn, cut)
            if what == "nan":
                assert torch.isnan(want["score"][0, 0]) and torch.isnan(want["raw"][0, 0]) and int(want["video"][0, 0]) == 1
                assert not spans or int(bits(want["span"])[0, 0, 0]) == 0x7FC12345
            else:
                assert want["count"].eq(0).all() and want["video"].eq(-1).all()
            same(M._merge_weighted("test", on, offsets, Q, K, fields, rk.to(dev), wt.to(dev), vn, cut), want, keys, (Q, what))


@pytest.mark.gpu
@pytest.mark.parametrize("spans", [False, True], ids=["cells", "spans"])
def test_rejections_leave_the_outputs_untouched(dev, spans):
    lists = carry_lists([3, 5], 2, seed=3, spans=spans)
    rank, weight = video_tables(2, 12, seed=1, reverse=False)
    ok = lambda **kw: through_ctypes(kw.pop("lists", lists), kw.pop("offsets", [0, 2]), kw.pop("K", 5), rank, weight, kw.pop("Vn", 12), 2, dev, spans, **kw)
    assert ok()[0] == 0
    n_tab = 6 if spans else 4
    cases = [dict(K=0), dict(K=65), dict(Vn=-1), dict(offsets=[0, -1]), dict(offsets=[0, 2 ** 31]), dict(lists=lists * 9, offsets=[0] * 18)]

    def set_arg(i, value):
        def fill(args, cols, buf):
            args[i] = value
        return fill

    def null_entry(args, cols, buf):
        args[2 + 1] = ctypes.cast((ctypes.c_void_p * 2)(cols[1][0].data_ptr(), None), ctypes.c_void_p)

    def alias(args, cols, buf):
        args[-2] = ctypes.c_void_p(cols[2][1].data_ptr())                               # an output that is list 1's raw

    def bad_k(args, cols, buf):
        args[2 + n_tab] = ctypes.cast((ctypes.c_int32 * 2)(3, 65), ctypes.c_void_p)

    n_args = 2 + n_tab + 8 + (7 if spans else 5)
    fills = [set_arg(1, 0), set_arg(2, None), null_entry, alias, bad_k, set_arg(2 + n_tab + 2, None), set_arg(2 + n_tab + 3, None),
             set_arg(n_args - 1, None), set_arg(n_args - 3, None), set_arg(2 + n_tab + 6, -1)]
    for kw in cases + [dict(fill=f) for f in fills]:
        rc, _ = ok(expect=1, **kw)
        assert rc != 0, kw
    # Q == 0 launches nothing and returns 0
    L_ = V()._lib
    assert L_.load().smin_search_merge_weighted(L_.stream(), 1, None, None, None, None, None, None, None, None, 3, 0, 0, 5, None, None, None, None, None) == 0


@pytest.mark.gpu
def test_merge_past_the_rank_tile_and_without_a_host_read(dev):
    """V = 2100 global videos -- past smin_video_rank's 2048-word tile -- in two lists of widths 1000 and 1100: merge_search_weighted
    against the restatement fed the kernel's rank and weight tables, every key; and the call reads nothing back."""
    A = V()
    g = torch.Generator().manual_seed(11)
    Q, widths, K = 2, (1000, 1100), 9
    lists = carry_lists([5, 7], Q, seed=21, spans=False, full_query=0)
    for r, w in zip(lists, widths):
        r["video"] = torch.where(r["video"] >= 0, torch.randint(0, w, r["video"].shape, generator=g), r["video"])
        r["pair_score"] = POOLED[torch.randint(0, 5, (Q, w), generator=g)] + torch.rand(Q, w, generator=g) * 0.01
        r["pair_cells"] = (torch.rand(Q, w, generator=g) < 0.9).float() * 7
    on = [to_dev(r, dev) for r in lists]
    gt = [1500, 3]
    kw = dict(k=K, video_weight=7.5, max_videos=700, n_videos=64, gt_video=gt)
    got = A.merge_search_weighted(on, [0, 1000], **kw)
    torch.cuda.synchronize()
    gt_d = torch.tensor(gt, dtype=torch.int32, device=dev)
    again = checked_no_sync(lambda: A.merge_search_weighted(on, [0, 1000], **dict(kw, gt_video=gt_d)))
    vr = A.rank_videos(got["pair_score"].reshape(-1), got["pair_cells"].reshape(-1), torch.arange(2100, dtype=torch.int32, device=dev).repeat(Q),
                       torch.arange(Q + 1, dtype=torch.int32, device=dev) * 2100, n=64, alpha=7.5)
    want = A.merge_search_weighted_torch(lists, [0, 1000], tables=(vr["pair_rank"].cpu(), vr["weight"].cpu()), **kw)
    assert int(want["count"].min()) >= 1 and int(want["video"].max()) >= 1000
    for r in (got, again):
        same(r, want, IDX_KEYS + RANK_KEYS + ("pair_score", "pair_cells"), "V = 2100")


# ---------------------------------------------------------------- GPU: the model-level routes

TAU = 0.1
MARGIN = 4e-5                                                                            # 2 * SCORE_TOL


@pytest.fixture(scope="module")
def world(dev):
    """the tiny model and corpus of test_pair_training (V = 5, Q = 4, L = 8) as banks, and the window corpus of test_window_search"""
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


class FixedScores:
    """``_score_pairs`` replaced by a fixed function of (global bank row, query): the banks are numbered in the order they are first
    seen, so the rows of a sequence of shard banks are the rows of the whole bank."""

    def __init__(self, m, rows, Q, dev, seed):
        g = torch.Generator().manual_seed(seed)
        L = m.L
        self.pm, self.ps, self.pe = (torch.rand(*s, generator=g).to(dev) for s in ((rows, Q, L, L), (rows, Q, L), (rows, Q, L)))
        self.m, self.first, self.seen = m, {}, 0

    def restart(self):
        self.first, self.seen = {}, 0

    def __call__(self, videos, queries, vi, qi, vi_d, qi_d):
        if id(videos) not in self.first:
            self.first[id(videos)] = (self.seen, videos)                                # (the bank is kept alive: its id stays its own)
            self.seen += len(videos)
        r, q = vi_d.to(torch.int64) + self.first[id(videos)][0], qi_d.to(torch.int64)
        mm = videos.moment_mask.index_select(0, vi_d).float()
        return self.pm[r, q] * mm, self.ps[r, q], self.pe[r, q], None

    def __enter__(self):
        self.m._score_pairs = self
        self.restart()
        return self

    def __exit__(self, *exc):
        del self.m._score_pairs


@pytest.mark.gpu
@pytest.mark.parametrize("split", SHARD_SPLITS, ids=str)
def test_sharded_weighted_search_on_equal_scores(dev, world, split):
    """Scores a fixed function of (video, query): search_shards_weighted and search_window_shards_weighted give the one-bank weighted
    search, bit for bit in every key, and so does one merge of all the shards' carry lists."""
    A = V()
    m, vid_d, qb, vb = world["m"], world["vid_d"], world["qb"], world["vb"]
    gt = [2, 0, 3, 1]
    for alpha, cut in ((7.5, 2), (0.0, None), (-2.0, 3)):
        kw = dict(k=7, k_video=3, video_weight=alpha, max_videos=cut, tau=TAU)
        slots = A.moments.carry_slots(7, 3, cut)
        with FixedScores(m, 5, 4, dev, seed=31) as fixed:
            whole = m.search(vb, qb, gt_video=gt, carry=True, **kw)
            fixed.restart()
            carry, duration = A.search_shards_weighted(m, video_shards(vid_d, split, vb.cell_counts), qb, gt_video=gt, **kw)
            fixed.restart()
            banks = [m.encode_videos(s["video_features"], s["video_mask"], s["length_mask"], s["moment_mask"], cell_counts=s["cell_counts"])
                     for s in video_shards(vid_d, split, vb.cell_counts)]
            lists = [m.search(b, qb, carry=True, **dict(kw, k=slots, n_videos=7)) for b in banks]
        assert duration.tolist() == DURATION.tolist() and int(whole["count"].min()) >= 1
        same(carry, whole, IDX_KEYS + RANK_KEYS + ("pair_score", "pair_cells"), ("folded", alpha, cut))
        at_once = A.merge_search_weighted(lists, np.concatenate([[0], np.cumsum(split)])[:-1].tolist(), k=7, video_weight=alpha, max_videos=cut,
                                          gt_video=gt)
        same(at_once, whole, IDX_KEYS + RANK_KEYS + ("pair_score", "pair_cells"), ("at once", alpha, cut))
        # raw is the entry's score before the weight: score = raw * weight of its video, the product of smin_moment_reweight
        if alpha == 0.0:
            same(dict(raw=whole["raw"]), dict(raw=whole["score"]), ("raw",), "alpha = 0")
    wb, wqb, raw = world["wb"], world["wqb"], world["raw"]
    gt_w = [0, 4, 2, 3]
    wkw = dict(video_weight=7.5, max_videos=2, tau=TAU, max_batch=7, **WS.KW)
    with FixedScores(m, len(wb), 4, dev, seed=32) as fixed:
        whole = m.search_windows(wb, wqb, gt_video=gt_w, carry=True, **wkw)
        fixed.restart()
        carry, duration, n_rows = A.search_window_shards_weighted(m, shard_dicts(raw, split), wqb, window=WS.WINDOW, stride=WS.STRIDE, gt_video=gt_w, **wkw)
    assert n_rows.tolist() == list(WS.LENGTHS) and int(whole["count"].min()) >= 1
    same(carry, whole, SPAN_KEYS + RANK_KEYS + ("pair_score", "pair_cells"), "windows, folded")


def separated(score, count, margin=MARGIN):
    """(Q, k) bool: the listed entries whose score lies more than ``margin`` from both neighbours'"""
    Q, k = score.shape
    listed = torch.arange(k).unsqueeze(0) < count.to(torch.int64).unsqueeze(1)
    gap = (score[:, :-1] - score[:, 1:]).abs() > margin
    gap = gap | ~listed[:, 1:]
    ok = torch.ones(Q, k, dtype=torch.bool)
    ok[:, 1:] &= gap
    ok[:, :-1] &= gap
    return ok & listed


def pooled_apart(video_score, video_count, margin=MARGIN):
    """every query's ranked pooled scores lie more than ``margin`` apart"""
    s, n = video_score.cpu(), video_count.cpu()
    return all(float(s[q, j] - s[q, j + 1]) > margin for q in range(s.shape[0]) for j in range(int(n[q]) - 1))


@pytest.mark.gpu
@pytest.mark.parametrize("split", SHARD_SPLITS, ids=str)
def test_sharded_weighted_search_on_its_own_scores(dev, world, split):
    """The model's own scores come from differently composed batches: sorted scores within 4e-5 (3s's tolerance), every entry separated
    from its neighbours by more than that is the same entry, and the video ranking is the bank's where the pooled scores are separated
    likewise.  With video_weight = 0.0 and no cut the carry is search_shards' plain list in the shared keys."""
    A = V()
    m, vid_d, qb, vb = world["m"], world["vid_d"], world["qb"], world["vb"]
    gt = [2, 0, 3, 1]
    kw = dict(k=7, k_video=3, video_weight=7.5, max_videos=2, tau=TAU)
    whole = to_cpu(m.search(vb, qb, gt_video=gt, **kw))
    carry, _ = A.search_shards_weighted(m, video_shards(vid_d, split, vb.cell_counts), qb, gt_video=gt, **kw)
    carry = to_cpu(carry)
    diff = (carry["score"] - whole["score"]).abs().max().item()
    sep = separated(whole["score"], whole["count"])
    print("split", split, "sorted weighted scores against the one bank: max difference", diff, "separated", int(sep.sum()), "of", int(whole["count"].sum()))
    assert torch.equal(carry["count"], whole["count"]) and diff < MARGIN
    assert int(sep.sum()) >= 0.5 * int(whole["count"].sum())                           # (the comparison is not vacuous)
    for key in ("video", "idx"):
        assert torch.equal(carry[key][sep], whole[key][sep]), key
    pdiff = (carry["video_score"] - whole["video_score"]).abs().max().item()
    print("pooled scores: max difference", pdiff, "apart", pooled_apart(whole["video_score"], whole["video_count"]))
    assert pdiff < MARGIN and torch.equal(carry["video_count"], whole["video_count"])
    if pooled_apart(whole["video_score"], whole["video_count"]):
        assert torch.equal(carry["video_rank"], whole["video_rank"]) and torch.equal(carry["gt_rank"], whole["gt_rank"])
    # the neutral setting: the plain sharded list, bit for bit, and raw is the score
    plain, _ = A.training.search_shards(m, video_shards(vid_d, split, vb.cell_counts), qb, k=7, k_video=3)
    neutral, _ = A.search_shards_weighted(m, video_shards(vid_d, split, vb.cell_counts), qb, k=7, k_video=3, video_weight=0.0, max_videos=None, tau=TAU)
    same(neutral, plain, ("video", "idx", "score", "count"), "neutral")
    same(dict(raw=neutral["raw"]), dict(raw=plain["score"]), ("raw",), "neutral raw")
    # the window route, the same way
    wb, wqb, raw = world["wb"], world["wqb"], world["raw"]
    wkw = dict(video_weight=7.5, max_videos=2, tau=TAU, **WS.KW)
    whole = to_cpu(m.search_windows(wb, wqb, gt_video=[0, 4, 2, 3], **wkw))
    carry, _, _ = A.search_window_shards_weighted(m, shard_dicts(raw, split), wqb, window=WS.WINDOW, stride=WS.STRIDE, gt_video=[0, 4, 2, 3], **wkw)
    carry = to_cpu(carry)
    diff = (carry["score"] - whole["score"]).abs().max().item()
    sep = separated(whole["score"], whole["count"])
    print("windows: max difference", diff, "separated", int(sep.sum()), "of", int(whole["count"].sum()))
    assert torch.equal(carry["count"], whole["count"]) and diff < MARGIN
    for key in ("video", "window", "cell"):
        assert torch.equal(carry[key][sep], whole[key][sep]), key
    assert torch.equal(bits(carry["span"])[sep], bits(whole["span"])[sep])
    if pooled_apart(whole["video_score"], whole["video_count"]):
        assert torch.equal(carry["video_rank"], whole["video_rank"]) and torch.equal(carry["gt_rank"], whole["gt_rank"])
    plain, _, _ = A.training.search_window_shards(m, shard_dicts(raw, split), wqb, window=WS.WINDOW, stride=WS.STRIDE, **WS.KW)
    neutral, _, _ = A.search_window_shards_weighted(m, shard_dicts(raw, split), wqb, window=WS.WINDOW, stride=WS.STRIDE, **WS.KW)
    same(neutral, plain, WS.KEYS, "neutral windows")


@pytest.mark.gpu
def test_the_loops_read_once_and_equal_the_one_bank_loop(dev, world):
    """test_model_corpus_weighted_shards and the window form: one host read, and -- on scores that are a fixed function of (video,
    query) -- every metric and the VideoRankMeter state of test_model_corpus / test_model_corpus_windows on the concatenated corpus."""
    A = V()
    m, vid_d, qry_d, vb = world["m"], world["vid_d"], world["qry_d"], world["vb"]
    gt_video = np.array([2, 0, 3, 1])
    kw = dict(k=10, k_video=2, video_weight=7.5, max_videos=3, tau=TAU)

    class Counting(A.CorpusMeter):
        reads = 0

        def result(self):
            torch.cuda.set_sync_debug_mode(mode)                                     # everything before this point ran without a host read
            Counting.reads += 1
            return super().result()

    whole_shard = dict(vid_d, duration=DURATION, cell_counts=vb.cell_counts)
    raw, queries = world["raw"], dict(query_features=world["wqf"], query_mask=world["wqm"])
    wkw = dict(window=WS.WINDOW, stride=WS.STRIDE, k=25, k_video=5, video_weight=7.5, max_videos=2, tau=TAU)
    gt_w = [0, 4, 2, 1]
    with FixedScores(m, 5, 4, dev, seed=33) as fixed:
        want_v = A.VideoRankMeter(n=(1, 2, 5), device=dev)
        want = A.test_model_corpus(m, [whole_shard], qry_d, gt_video, GT_TIMES, video_meter=want_v, **kw)
        for split in SHARD_SPLITS:
            fixed.restart()
            first = A.test_model_corpus_weighted_shards(m, video_shards(vid_d, split, vb.cell_counts), qry_d, gt_video, GT_TIMES, **kw)   # first use outside the checked region
            assert first == want
            fixed.restart()
            got_v = A.VideoRankMeter(n=(1, 2, 5), device=dev)
            torch.cuda.synchronize()
            Counting.reads = 0
            mode = torch.cuda.get_sync_debug_mode()
            torch.cuda.set_sync_debug_mode("error")
            try:
                got = A.test_model_corpus_weighted_shards(m, video_shards(vid_d, split, vb.cell_counts), qry_d, gt_video, GT_TIMES,
                                                          Counting(n=(1, 5), device=dev), video_meter=got_v, **kw)
            finally:
                torch.cuda.set_sync_debug_mode(mode)
            print("split", split, got, got_v.result())
            assert Counting.reads == 1 and got == want and got["num_samples"] == 4
            assert torch.equal(got_v.state.cpu(), want_v.state.cpu()) and got_v.result() == want_v.result()
    with FixedScores(m, len(world["wb"]), 4, dev, seed=34) as fixed:
        want_v = A.VideoRankMeter(n=(1, 2), device=dev)
        want = A.test_model_corpus_windows(m, raw, WS.LENGTHS, queries, gt_w, GT_TIMES, DURATION, video_meter=want_v, **wkw)
        for split in SHARD_SPLITS:
            fixed.restart()
            first = A.test_model_corpus_window_shards_weighted(m, shard_dicts(raw, split), queries, gt_w, GT_TIMES, **wkw)
            assert first == want
            fixed.restart()
            got_v = A.VideoRankMeter(n=(1, 2), device=dev)
            torch.cuda.synchronize()
            Counting.reads = 0
            mode = torch.cuda.get_sync_debug_mode()
            torch.cuda.set_sync_debug_mode("error")
            try:
                got = A.test_model_corpus_window_shards_weighted(m, shard_dicts(raw, split), queries, gt_w, GT_TIMES, Counting(n=(1, 5), device=dev),
                                                                 video_meter=got_v, **wkw)
            finally:
                torch.cuda.set_sync_debug_mode(mode)
            assert Counting.reads == 1 and got == want and got["num_samples"] == 4
            assert torch.equal(got_v.state.cpu(), want_v.state.cpu())
    with pytest.raises(ValueError, match="one shard"):                                   # the plain loop still refuses
        A.test_model_corpus(m, video_shards(vid_d, [2, 3], vb.cell_counts), qry_d, gt_video, GT_TIMES, **kw)
    assert int(A._lib.load_torch().layout_status(dev)[0]) == 0


@pytest.mark.gpu
def test_nothing_else_moved(dev, world):
    """search, search_windows (plain and weighted), merge_search, merge_search_windows and the plain loops give the same bits before
    and after a weighted sharded run"""
    A = V()
    m, vid_d, qry_d, vb, qb = world["m"], world["vid_d"], world["qry_d"], world["vb"], world["qb"]
    wb, wqb, raw = world["wb"], world["wqb"], world["raw"]
    queries = dict(query_features=world["wqf"], query_mask=world["wqm"])
    gt_video = np.array([2, 0, 3, 1])

    def everything():
        a = m.search(vb, qb, k=7, k_video=3)
        b = m.search(vb, qb, k=7, k_video=3, video_weight=7.5, max_videos=2, tau=TAU, gt_video=gt_video)
        c = m.search_windows(wb, wqb, max_batch=7, **WS.KW)
        d = m.search_windows(wb, wqb, max_batch=7, video_weight=7.5, max_videos=2, tau=TAU, **WS.KW)
        assert set(a) == {"video", "idx", "score", "count"} and "raw" not in b and "pair_score" not in d
        e = A.merge_search([a, a], [0, 5], k=7)
        f = A.merge_search_windows([c, c], [0, 5], k=5)
        g = A.test_model_corpus(m, video_shards(vid_d, [2, 3], vb.cell_counts), qry_d, gt_video, GT_TIMES, k=10, k_video=2)
        h = A.test_model_corpus_windows(m, raw, WS.LENGTHS, queries, [0, 4, 2, 1], GT_TIMES, DURATION, window=WS.WINDOW, stride=WS.STRIDE, k=25, k_video=5)
        return [v.cpu().contiguous().view(torch.uint8) for r in (a, b, c, d, e, f) for v in r.values()] + \
            [torch.tensor(list(x.values()), dtype=torch.float64) for x in (g, h)]

    before = everything()
    A.test_model_corpus_weighted_shards(m, video_shards(vid_d, [2, 3], vb.cell_counts), qry_d, gt_video, GT_TIMES, k=10, k_video=2, video_weight=7.5,
                                        max_videos=2)
    A.test_model_corpus_window_shards_weighted(m, shard_dicts(raw, [1, 1, 3]), queries, [0, 4, 2, 1], GT_TIMES, window=WS.WINDOW, stride=WS.STRIDE, k=25,
                                               k_video=5, video_weight=7.5)
    after = everything()
    assert len(before) == len(after) and all(torch.equal(x, y) for x, y in zip(before, after))
