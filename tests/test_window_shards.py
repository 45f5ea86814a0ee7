"""Span-valued search results merged across shards of a long-video corpus: csrc/corpus.hip (smin_span_search_merge),
moments.merge_search_windows / merge_search_windows_torch, distributed.gather_search_windows, training.search_window_shards and
training.test_model_corpus_window_shards.

Host: the C ABI surface and its rejections, the exactness of merging the span lists of disjoint shards (at once, folded, more than
sixteen lists), times, the refusals, two gloo ranks.
GPU: the one-pass rank kernel bit for bit against the restated sort, every element written and none beyond; folded against at once;
sharded search_windows end to end against the whole bank, on equal scores bit for bit and on its own scores where the scores separate
the entries; the sharded test loop against test_model_corpus_windows, without host reads; and nothing else moved."""
import ctypes
import multiprocessing as mp
import os
import re

import numpy as np
import pytest
import torch

from tests.support.device import dev  # noqa: F401  (the module's device fixture)
from tests.support.device import checked_no_sync, free_port, to_cpu, to_dev, vml as V
from tests.support.compare import bits
from tests.support.guards import WORD_SENTINEL as SENTINEL
from tests.support.corpora import (
    corpus_rows, host_masks, pair_lists, random_span_lists, same_lists, same_search, shard_dicts, shards_of as cell_shards, tiny_model, DURATION,
    KEYS, KW, L, LENGTHS, LENS, MARGIN, NAN_BITS, SEED, SHARD_SPLITS, STRIDE, VPTR, WINDOW)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SPLITS = ([3, 4], [1, 1, 5], [7], [2, 2, 2, 1])
VALUES = torch.tensor([0.9, 0.5, 0.25, 0.0, -0.0, 1e-3])                              # six scores, both zeros among them: ties everywhere


# ---------------------------------------------------------------- shared data
def group_lists(nv, Q, kv, seed):
    """merge_window_moments-shaped lists of all Q * nv (query, video) groups, query-major: scores from VALUES in descending order within
    a group (as stage A leaves them), random counts in [-1, kv + 1]; behind a count NaN spans, -1 and a NaN score"""
    g = torch.Generator().manual_seed(seed)
    G2 = Q * nv
    score = VALUES[torch.randint(0, 6, (G2, kv), generator=g)]
    score = torch.gather(score, 1, torch.where(score == 0, torch.zeros_like(score), score).sort(dim=1, descending=True, stable=True).indices)
    span = torch.rand(G2, kv, 2, generator=g) * 100
    window = torch.randint(0, 9, (G2, kv), generator=g, dtype=torch.int64)
    cell = torch.randint(0, 64, (G2, kv, 2), generator=g, dtype=torch.int64)
    count = torch.randint(-1, kv + 2, (G2,), generator=g, dtype=torch.int32)
    unused = torch.arange(kv).unsqueeze(0) >= count.unsqueeze(1)
    nan = float("nan")
    return (torch.where(unused.unsqueeze(2), torch.full_like(span, nan), span), torch.where(unused, torch.full_like(score, nan), score),
            torch.where(unused, torch.full_like(window, -1), window), torch.where(unused.unsqueeze(2), torch.full_like(cell, -1), cell), count)


def topk_of(lists, nv, Q, v0, v1, K):
    """corpus_span_topk_torch(k=K) of the videos v0 .. v1 of ``lists`` (group_lists), numbered from 0 within the shard"""
    rows = torch.tensor([q * nv + v for q in range(Q) for v in range(v0, v1)], dtype=torch.int64)
    video = torch.arange(v1 - v0, dtype=torch.int32).repeat(Q)
    ptr = torch.arange(Q + 1, dtype=torch.int32) * (v1 - v0)
    return V().corpus_span_topk_torch(*[t[rows] for t in lists], video, ptr, k=K)


def shards_of(lists, nv, Q, split, K):
    edges = np.concatenate([[0], np.cumsum(split)]).tolist()
    assert edges[-1] == nv
    return [topk_of(lists, nv, Q, a, b, K) for a, b in zip(edges[:-1], edges[1:])], edges[:-1]


# ---------------------------------------------------------------- host: surface
def test_header_table_library_and_package_declare_the_span_merge():
    text = open(os.path.join(ROOT, "include", "smin_hip.h")).read()
    assert re.search(r"\bint\s+smin_span_search_merge\s*\(", text)
    A = V()
    assert len(A._lib.SIGNATURES["smin_span_search_merge"]) == 18
    assert hasattr(A._lib.load(), "smin_span_search_merge")
    assert "#define SMIN_HIP_ABI_VERSION 2" in text and A._lib.ABI_VERSION == 2
    for name in ("merge_search_windows", "merge_search_windows_torch", "test_model_corpus_window_shards"):
        assert hasattr(A, name), name
    assert A.test_model_corpus_window_shards.__test__ is False
    assert hasattr(A.distributed, "gather_search_windows") and hasattr(A.training, "search_window_shards") and hasattr(A.moments, "window_times")


# ---------------------------------------------------------------- host: rejection before any launch
def test_c_abi_rejects_before_any_launch():
    """smin_span_search_merge returns a nonzero status without launching anything (so this runs without a device, on addresses that are
    never dereferenced); Q = 0 is accepted and does nothing."""
    lib = V()._lib.load()
    fake, out = 0x10000, 0x20000
    good = tuple(out + 0x100 * j for j in range(6))
    names = "vpswcn"                                                                 # video, span, score, window, cell, count

    def merge(S=2, K=5, Q=3, ks=(3, 3), off=(0, 4), tables=names, outs=good, k_list=True, entry=fake, one=None):
        def table(c):
            if c not in tables:
                return None
            t = (ctypes.c_void_p * 17)(*([entry] * 17))
            if one is not None and one[0] == c:
                t[one[1]] = None                                                     # a single NULL entry
            return t
        kl = (ctypes.c_int32 * 17)(*(list(ks) + [3] * (17 - len(ks)))) if k_list else None
        ol = (ctypes.c_int64 * 17)(*(list(off) + [0] * (17 - len(off))))
        return lib.smin_span_search_merge(None, S, *[table(c) for c in names], kl, ol, Q, K, *outs)

    assert merge(S=0) != 0 and merge(S=17) != 0 and merge(S=-1) != 0
    assert merge(K=0) != 0 and merge(K=65) != 0
    assert merge(ks=(3, 0)) != 0 and merge(ks=(65, 3)) != 0 and merge(ks=(3, 0), Q=0) != 0
    assert merge(Q=-1) != 0
    assert merge(off=(0, -1)) != 0 and merge(off=(0, 2 ** 31)) != 0 and merge(off=(-1, 0)) != 0
    for c in names:
        assert merge(tables=names.replace(c, "")) != 0, c                            # a NULL table
        assert merge(one=(c, 1)) != 0, c                                             # a NULL entry of list 1
    assert merge(k_list=False) != 0 and merge(entry=None) != 0
    for o in range(6):
        outs = list(good)
        outs[o] = None
        assert merge(outs=tuple(outs)) != 0, o
        outs[o] = fake                                                               # an output that is one of the inputs
        assert merge(outs=tuple(outs)) != 0, o
    assert merge(Q=0) == 0 and merge(Q=0, tables="", outs=(None,) * 6) == 0 and merge(S=16, Q=0, ks=(64,) * 16) == 0


# ---------------------------------------------------------------- host: the restated merge
@pytest.mark.parametrize("K", [1, 3, 5, 9])
def test_sharding_is_exact(K):
    """merge_search_windows_torch of the shards' corpus_span_topk_torch(k=K) lists is corpus_span_topk_torch on the whole corpus, bit for
    bit on all six outputs, merged at once and folded one shard after another: V = 7, Q = 3, k_video = 3, scores from six values with
    both zeros, counts in -1 .. k_video + 1."""
    A = V()
    nv, Q, kv = 7, 3, 3
    for seed in range(25):
        lists = group_lists(nv, Q, kv, seed)
        whole = topk_of(lists, nv, Q, 0, nv, K)
        for split in SPLITS:
            shards, offsets = shards_of(lists, nv, Q, split, K)
            same_lists(A.merge_search_windows_torch(shards, offsets, k=K), whole, (seed, split, "at once"))
            carry = shards[0]
            for r, off in zip(shards[1:], offsets[1:]):
                carry = A.merge_search_windows_torch([carry, r], [0, off], k=K)
            same_lists(carry if len(shards) > 1 else A.merge_search_windows_torch([carry], [0], k=K), whole, (seed, split, "folded"))
    assert not torch.isnan(whole["score"]).any() and bits(whole["span"]).eq(NAN_BITS).sum() == 2 * whole["video"].eq(-1).sum()


def test_fold_of_more_than_sixteen_lists():
    """moments.fold_search as it is, over span lists: 17, 31 and 40 one-video shards give the one sort of all entries"""
    A = V()
    for nv, K in ((17, 5), (31, 3), (40, 9)):
        lists = group_lists(nv, 3, 3, seed=nv)
        shards, offsets = shards_of(lists, nv, 3, [1] * nv, K)
        calls = []

        def merge(ls, off, k):
            calls.append(len(ls))
            return A.merge_search_windows_torch(ls, off, k=k)

        same_lists(A.moments.fold_search(shards, offsets, K, merge), topk_of(lists, nv, 3, 0, nv, K), nv)
        assert calls[0] == 16 and len(calls) == 1 + -(-(nv - 16) // 15) and max(calls) <= 16


def test_times_follow_the_one_formula():
    A = V()
    nv, Q = 4, 3
    lists = group_lists(nv, Q, 3, seed=2)
    shards, offsets = shards_of(lists, nv, Q, [1, 3], 9)
    duration, n_rows = torch.tensor([10.0, 3.5, 60.0, 7.25]), torch.tensor([40, 16, 9, 23])
    r = A.merge_search_windows_torch(shards, offsets, k=9, duration=duration, n_rows=n_rows)
    assert set(r) == set(KEYS) | {"times"} and (r["count"] < 9).any() and (r["count"] > 0).all()
    v = r["video"].clamp_min(0)
    want = (r["span"] * duration[v].unsqueeze(-1)) / n_rows.float()[v].unsqueeze(-1)     # search_windows' formula on the merged entries
    assert torch.equal(bits(r["times"]), bits(want))
    listed = torch.arange(9).unsqueeze(0) < r["count"].unsqueeze(1)
    assert torch.isnan(r["times"][~listed]).all() and not torch.isnan(r["times"][listed]).any()
    assert torch.equal(bits(r["times"]), bits(A.moments.window_times(r["video"], r["span"], duration, n_rows)))
    assert "times" not in A.merge_search_windows_torch(shards, offsets, k=9)


# ---------------------------------------------------------------- host: refusals
def test_refusals():
    A = V()
    err = A._lib.SminHipError
    lists, _ = shards_of(group_lists(4, 2, 3, seed=1), 4, 2, [2, 2], 3)
    with pytest.raises(err, match="no CPU fallback"):
        A.merge_search_windows(lists, [0, 2], k=4)
    for f in (A.merge_search_windows, A.merge_search_windows_torch):
        with pytest.raises(ValueError, match="1..16"):
            f([lists[0]] * 17)
        with pytest.raises(ValueError, match="1..16"):
            f([])
        with pytest.raises(ValueError, match="one Q"):
            f([lists[0], {key: v[:1] for key, v in lists[1].items()}])
        for k in (0, 65, 2.0):
            with pytest.raises(ValueError, match="integer 1 <= k"):
                f(lists, k=k)
        wide = {"video": torch.zeros(2, 65, dtype=torch.int64), "span": torch.zeros(2, 65, 2), "score": torch.zeros(2, 65),
                "window": torch.zeros(2, 65, dtype=torch.int64), "cell": torch.zeros(2, 65, 2, dtype=torch.int64), "count": torch.zeros(2, dtype=torch.int32)}
        with pytest.raises(ValueError, match="slots per query"):
            f([lists[0], wide])
        with pytest.raises(ValueError, match="must hold"):
            f([lists[0], dict(lists[1], cell=lists[1]["cell"][:, :, :1])])
        for off in ([0, -1], [0], [0, 2 ** 31]):
            with pytest.raises(ValueError, match="video_offset"):
                f(lists, off)
        with pytest.raises(ValueError, match="both duration and n_rows"):
            f(lists, [0, 2], duration=torch.ones(4))
        with pytest.raises(ValueError, match="both duration and n_rows"):
            f(lists, [0, 2], n_rows=torch.ones(4))
    # test_model_corpus_window_shards: before any device work (a host model and host tensors would raise SminHipError at the first encoder)
    m, _ = tiny_model()
    raw, qf, qm = corpus_rows(0)
    shards = [dict(raw=raw, lengths=LENGTHS, duration=np.ones(5))]
    queries = dict(query_features=qf, query_mask=qm)
    gv, gt = [0, 1, 2, 4], np.tile([0.0, 1.0], (4, 1))
    for kw in (dict(k=24, k_video=5), dict(k=4, k_video=1), dict(k=25, k_video=6)):
        with pytest.raises(ValueError, match="needs k >= max"):
            A.test_model_corpus_window_shards(m, shards, queries, gv, gt, **kw)
    with pytest.raises(ValueError, match="needs k >= max"):
        A.test_model_corpus_window_shards(m, shards, queries, gv, gt, A.CorpusMeterTorch(n=(1, 10)), k=25, k_video=5)
    with pytest.raises(ValueError, match="gt_video"):
        A.test_model_corpus_window_shards(m, shards, queries, gv[:3], gt)
    with pytest.raises(err, match="no CPU fallback"):
        A.test_model_corpus_window_shards(m, shards, queries, gv, gt)                  # the defaults hold and reach the encoders


# ---------------------------------------------------------------- host: two gloo ranks
GLOO = dict(nv=7, Q=3, kv=3, K=5, seed=4, split=[3, 4])


def _gather_worker(rank, world, port, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), WORLD_SIZE=str(world), RANK=str(rank), LOCAL_RANK=str(rank))
    torch.set_num_threads(2)
    A = V()
    D = A.distributed
    D.init(backend="gloo")
    c = GLOO
    shards, _ = shards_of(group_lists(c["nv"], c["Q"], c["kv"], c["seed"]), c["nv"], c["Q"], c["split"], c["K"])
    got = D.gather_search_windows(shards[rank], c["split"][rank], merge=A.merge_search_windows_torch)
    refused = False
    try:
        D.gather_search_windows(shards[rank], c["split"][rank], k=3 + rank, merge=A.merge_search_windows_torch)
    except ValueError as e:
        refused = "same queries" in str(e) and "gather_search_windows" in str(e)
    D.barrier()
    q.put((rank, refused, sorted(got), {key: got[key].numpy() for key in KEYS}))
    torch.distributed.destroy_process_group()


@pytest.mark.timeout(300)
def test_two_gloo_ranks_return_the_whole_corpus_list():
    """Each of two ranks holds the corpus_span_topk_torch list of its shard ([3, 4] of the 7 videos): gather_search_windows(merge=
    merge_search_windows_torch) returns the single-process merge on both, bitwise equal and without times; ranks that pass different k
    raise ValueError on both."""
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
    c = GLOO
    lists = group_lists(c["nv"], c["Q"], c["kv"], c["seed"])
    shards, offsets = shards_of(lists, c["nv"], c["Q"], c["split"], c["K"])
    single = V().merge_search_windows_torch(shards, offsets, k=c["K"])
    same_lists(single, topk_of(lists, c["nv"], c["Q"], 0, c["nv"], c["K"]))
    assert int(single["video"].max()) >= 3                                           # the second rank's videos are listed, with their offset
    for rank, refused, keys, got in res:
        assert refused and keys == sorted(KEYS), rank
        for key in KEYS:
            assert got[key].tobytes() == single[key].numpy().tobytes() == res[0][3][key].tobytes(), (rank, key)


# ---------------------------------------------------------------- GPU
def ranked_lists(ks, Q, seed, empty_query=None, full_query=None):
    """len(ks) ranked span lists ordered as search_windows orders them (score, then video, through the order word), list s of ks[s]
    slots over 6 local videos: counts in [-1, k_s + 1], behind them NaN spans and scores and -1; ``empty_query``: no list has an entry,
    ``full_query``: every list is full"""
    g = torch.Generator().manual_seed(seed)
    out = []
    for k in ks:
        score = VALUES[torch.randint(0, 6, (Q, k), generator=g)]
        video = torch.randint(0, 6, (Q, k), generator=g, dtype=torch.int64)
        plus = torch.where(score == 0, torch.zeros_like(score), score)                   # -0 counts as +0
        order = torch.tensor([sorted(range(k), key=lambda p: (-float(plus[q, p]), int(video[q, p]), p)) for q in range(Q)], dtype=torch.int64)
        score, video = torch.gather(score, 1, order), torch.gather(video, 1, order)
        count = torch.randint(-1, k + 2, (Q,), generator=g, dtype=torch.int32)
        if empty_query is not None and empty_query < Q:
            count[empty_query] = [0, -1][len(out) % 2]
        if full_query is not None:
            count[full_query] = k
        unused = torch.arange(k).unsqueeze(0) >= count.unsqueeze(1)
        nan = float("nan")
        out.append({"video": torch.where(unused, torch.full_like(video, -1), video),
                    "span": torch.where(unused.unsqueeze(2), torch.full((Q, k, 2), nan), torch.rand(Q, k, 2, generator=g) * 100),
                    "score": torch.where(unused, torch.full_like(score, nan), score),
                    "window": torch.where(unused, torch.full_like(video, -1), torch.randint(0, 9, (Q, k), generator=g, dtype=torch.int64)),
                    "cell": torch.where(unused.unsqueeze(2), torch.full((Q, k, 2), -1, dtype=torch.int64), torch.randint(0, 64, (Q, k, 2), generator=g, dtype=torch.int64)),
                    "count": count})
    return out


def through_ctypes(lists, offsets, K, dev):
    """smin_span_search_merge into buffers pre-filled with a sentinel and four spare words behind each: every element written, none beyond"""
    L_ = V()._lib
    S, Q = len(lists), lists[0]["video"].shape[0]
    cols = [[r[key].to(dev).contiguous() for r in lists] for key in KEYS]
    tables = [(ctypes.c_void_p * S)(*[t.data_ptr() for t in col]) for col in cols]
    k_list = (ctypes.c_int32 * S)(*[r["video"].shape[1] for r in lists])
    off = (ctypes.c_int64 * S)(*offsets)
    shapes = dict(video=(Q, K), span=(Q, K, 2), score=(Q, K), window=(Q, K), cell=(Q, K, 2), count=(Q,))
    words = {key: (2 if key in ("video", "window", "cell") else 1) * int(np.prod(s)) for key, s in shapes.items()}
    raw = {key: torch.full((n + 4,), SENTINEL, dtype=torch.int32, device=dev) for key, n in words.items()}
    L_.call("smin_span_search_merge", L_.stream(), S, *[ctypes.cast(t, ctypes.c_void_p) for t in tables], ctypes.cast(k_list, ctypes.c_void_p),
            ctypes.cast(off, ctypes.c_void_p), Q, K, *[L_.ptr(raw[key]) for key in KEYS])
    torch.cuda.synchronize()
    out = {}
    for key in KEYS:
        assert raw[key][words[key]:].eq(SENTINEL).all(), key + ": written past the end"
        body = raw[key][:words[key]].cpu()
        out[key] = (body.view(torch.int64) if key in ("video", "window", "cell") else body.view(torch.float32) if key in ("span", "score") else body).reshape(shapes[key])
    return out


K_LISTS = {1: ([3], [64]), 2: ([1, 64], [3, 3]), 3: ([64, 1, 3],), 16: ([64] * 16, [1, 3, 64] * 5 + [3])}


@pytest.mark.gpu
@pytest.mark.parametrize("S", [1, 2, 3, 16])
@pytest.mark.parametrize("K", [1, 5, 64])
def test_merge_kernel_bit_exact(dev, S, K):
    """The kernel against the restated sort on every output, Q = 1 and 5: overlapping global videos between the lists (offsets 0, 2, 4,
    ... over 6 local videos each, so the (list, position) tie-break decides everywhere), counts below 0, 0 and above k_s, a query with
    every list empty, NaN and -1 behind the counts; S = 16 with every k_s = 64 and a full query is the whole 1024-word stage."""
    A = V()
    offsets = [2 * s for s in range(S)]
    for ks in K_LISTS[S]:
        for Q in (1, 5):
            lists = ranked_lists(ks, Q, seed=100 * S + K + Q, empty_query=2, full_query=0)
            want = A.merge_search_windows_torch(lists, offsets, k=K)
            assert int(want["count"][0]) == min(K, sum(ks)) and (Q == 1 or int(want["count"][2]) == 0)
            assert not torch.isnan(want["score"]).any() and int(want["video"].min()) >= -1
            same_lists(through_ctypes(lists, offsets, K, dev), want, (ks, Q, "ctypes"))
            same_lists(A.merge_search_windows([to_dev(r, dev) for r in lists], offsets, k=K), want, (ks, Q, "merge_search_windows"))
    if S == 2:                                                                       # a carry and a next list that name the same global videos
        lists = ranked_lists([5, 64], 5, seed=K, full_query=1)
        same_lists(through_ctypes(lists, [0, 0], K, dev), A.merge_search_windows_torch(lists, [0, 0], k=K), "equal offsets")


@pytest.mark.gpu
@pytest.mark.parametrize("S", [1, 2, 16])
@pytest.mark.parametrize("K", [1, 64])
def test_merge_kernel_nan_scores_and_payloads(dev, S, K):
    """What ranked_lists leaves out: every list opens with a NaN score (the highest order word, so the list stays ordered) on local
    video 1 -- with equal offsets one global video at one score in every list -- under a NaN span with a payload of its own, which
    leaves as it came; k_s mixing 1 and 64, Q = 1 and 3, equal and overlapping offsets."""
    A = V()
    ks = [(64, 1)[s % 2] for s in range(S)]
    for Q in (1, 3):
        lists = ranked_lists(ks, Q, seed=7 * S + Q, full_query=0)
        for r in lists:
            r["score"][:, 0] = float("nan")
            r["video"][:, 0] = 1
            r["span"].view(torch.int32)[:, 0, 0] = 0x7FC12345
        for offsets in ([0] * S, [2 * s for s in range(S)]):
            want = A.merge_search_windows_torch(lists, offsets, k=K)
            assert int(want["count"][0]) == min(K, sum(ks)) and torch.isnan(want["score"][0, 0]) and int(bits(want["span"])[0, 0, 0]) == 0x7FC12345
            assert int(want["video"][0, 0]) == 1 and torch.isnan(want["score"][0, :min(K, S)]).all()
            same_lists(through_ctypes(lists, offsets, K, dev), want, (Q, offsets, "ctypes"))
            same_lists(A.merge_search_windows([to_dev(r, dev) for r in lists], offsets, k=K), want, (Q, offsets, "merge_search_windows"))


@pytest.mark.gpu
def test_folded_equals_at_once_on_the_device(dev):
    A = V()
    nv, Q, K = 7, 3, 5
    lists = group_lists(nv, Q, 3, seed=6)
    shards, offsets = shards_of(lists, nv, Q, [2, 2, 3], K)
    whole = topk_of(lists, nv, Q, 0, nv, K)
    on = [to_dev(s, dev) for s in shards]
    same_lists(A.merge_search_windows(on, offsets, k=K), whole, "at once")
    carry = on[0]
    for r, off in zip(on[1:], offsets[1:]):
        carry = A.merge_search_windows([carry, r], [0, off], k=K)
    same_lists(carry, whole, "folded")
    same_lists(A.moments.fold_search(on, offsets, K, A.merge_search_windows), whole, "fold_search")
    duration, n_rows = torch.arange(1.0, 8.0, device=dev), torch.arange(10, 17, device=dev)
    torch.cuda.synchronize()
    timed = checked_no_sync(lambda: A.merge_search_windows(on, offsets, k=K, duration=duration, n_rows=n_rows))     # reads nothing back
    same_lists(timed, whole, "with times")
    assert torch.equal(bits(timed["times"]), bits(A.merge_search_windows_torch(shards, offsets, k=K, duration=duration.cpu(), n_rows=n_rows.cpu())["times"]))
    empty = A.merge_search_windows([{key: v[:0] for key, v in s.items()} for s in on], offsets, k=K)             # Q = 0
    assert empty["video"].shape == (0, K) and empty["count"].shape == (0,)


# ---------------------------------------------------------------- GPU: sharded search_windows
@pytest.fixture(scope="module")
def world(dev):
    """the tiny model, LENGTHS' rows (40, 16, 9, 0 and 23: 4, 1, 1, 0 and 2 windows), four ragged queries, the whole bank and its search"""
    m, _ = tiny_model(dev)
    raw, qf, qm = corpus_rows(SEED)
    raw_d, qf_d, qm_d = raw.to(dev), qf.to(dev), qm.to(dev)
    qb = m.encode_queries(qf_d, qm_d)
    wb = m.encode_windows(raw_d, LENGTHS, WINDOW, STRIDE)
    whole = to_cpu(m.search_windows(wb, qb, duration=torch.from_numpy(DURATION).to(dev), **KW))
    return dict(m=m, raw=raw_d, qf=qf_d, qm=qm_d, qb=qb, wb=wb, whole=whole)


@pytest.mark.gpu
@pytest.mark.parametrize("split", SHARD_SPLITS)
def test_sharded_search_on_equal_scores(dev, world, split):
    """Scores that are a fixed function of (global window, query), so the shards and the whole bank rank the same numbers: the shards'
    search_windows_torch lists, merged by the kernel at once and folded, are the whole bank's list, bit for bit."""
    A = V()
    m, raw, qb = world["m"], world["raw"], world["qb"]
    g = torch.Generator().manual_seed(17)
    W, Q = len(LENS), 4
    mmask = host_masks(LENS)[2]
    pm = (torch.rand(W, Q, L, L, generator=g) * mmask.unsqueeze(1)).to(dev)
    ps, pe = torch.rand(W, Q, L, generator=g).to(dev), torch.rand(W, Q, L, generator=g).to(dev)

    def scorer(w0):
        def f(wi, wq):
            wi, wq = torch.from_numpy(wi + w0).to(dev), torch.from_numpy(wq).to(dev)
            return pm[wi, wq], ps[wi, wq], pe[wi, wq], None
        return f

    whole = to_cpu(m.search_windows_torch(world["wb"], qb, scorer=scorer(0), **KW))
    assert whole["count"].tolist() == [5] * 4 and len(set(whole["video"].flatten().tolist())) >= 3
    lists, offsets, seen = [], [], 0
    for shard in shard_dicts(raw, split):
        bank = m.encode_windows(shard["raw"], shard["lengths"], WINDOW, STRIDE)
        lists.append(m.search_windows_torch(bank, qb, scorer=scorer(VPTR[seen]), **KW))
        offsets.append(seen)
        seen += len(shard["lengths"])
    same_lists(A.merge_search_windows(lists, offsets, k=5), whole, "at once")
    carry = lists[0]
    for r, off in zip(lists[1:], offsets[1:]):
        carry = A.merge_search_windows([carry, r], [0, off], k=5)
    same_lists(carry, whole, "folded")


@pytest.mark.gpu
@pytest.mark.parametrize("split", SHARD_SPLITS)
def test_sharded_search_on_its_own_scores(dev, world, split):
    """search_window_shards against search_windows on the whole bank: scores of differently composed batches, so sorted scores within
    2 * SCORE_TOL and, wherever the whole bank's neighbouring scores lie further apart than that, the same entry with the same span
    bits; and the carry is the restated fold of the shards' own lists, bit for bit."""
    A = V()
    m, raw, qb, whole = world["m"], world["raw"], world["qb"], world["whole"]
    carry, duration, n_rows = A.training.search_window_shards(m, shard_dicts(raw, split), qb, window=WINDOW, stride=STRIDE, **KW)
    assert duration.tolist() == DURATION.tolist() and n_rows.tolist() == list(LENGTHS) and "times" not in carry
    sep, diff = same_search(carry, whole)
    print("split", split, "sorted scores against the whole bank: max difference", diff, "separated", int(sep.sum()), "of", int(whole["count"].sum()))
    assert int(sep.sum()) >= 0.5 * int(whole["count"].sum())                         # (the comparison is not vacuous)
    # the same flow restated: per-shard search, lists to the CPU, merge_search_windows_torch fold
    want, seen = None, 0
    for shard in shard_dicts(raw, split):
        bank = m.encode_windows(shard["raw"], shard["lengths"], WINDOW, STRIDE)
        r = to_cpu(m.search_windows(bank, qb, **KW))
        want = r if want is None else A.merge_search_windows_torch([want, r], [0, seen], k=5)
        seen += len(shard["lengths"])
    same_lists(carry, want, "the folded list")
    t = A.moments.window_times(carry["video"], carry["span"], torch.from_numpy(DURATION).to(dev), torch.tensor(LENGTHS, device=dev))
    assert torch.equal(bits(t)[sep], bits(whole["times"])[sep])
    assert int(A._lib.load_torch().layout_status(dev)[0]) == 0


# ---------------------------------------------------------------- GPU: the sharded test loop
def gaps_hold(r, ranks):
    """every query's listed scores at the given boundaries (rank j against j + 1, from 1) lie more than MARGIN apart"""
    s, n = r["score"], r["count"]
    return all(int(n[q]) <= j or float(s[q, j - 1] - s[q, j]) > MARGIN for q in range(s.shape[0]) for j in ranks)


@pytest.mark.gpu
def test_model_corpus_window_shards_end_to_end(dev, world):
    A = V()
    m, raw = world["m"], world["raw"]
    queries = dict(query_features=world["qf"], query_mask=world["qm"])
    kw = dict(window=WINDOW, stride=STRIDE, k=25, k_video=5)
    # the metrics read rank 1 and the set of the first five: on the whole bank these are separated from what follows by more than the
    # scores of differently composed batches can move, so both loops must see them alike
    r = to_cpu(m.search_windows(world["wb"], world["qb"], k=25, k_video=5, duration=torch.from_numpy(DURATION).to(dev)))
    print("whole bank: scores of ranks 1, 2, 5, 6", r["score"][:, [0, 1, 4, 5]].tolist(), "counts", r["count"].tolist())
    assert gaps_hold(r, (1, 5))
    gt_video = np.array([0, 4, 2, 1])
    gt_times = np.stack([np.array([1.0, 20.0, 0.5, 0.0]), np.array([6.0, 70.0, 30.0, 3.0])], axis=1)
    want = A.test_model_corpus_windows(m, raw, LENGTHS, queries, gt_video, gt_times, DURATION, **kw)

    class Counting(A.CorpusMeter):
        reads = 0

        def result(self):
            torch.cuda.set_sync_debug_mode(mode)                                     # everything before this point ran without a host read
            Counting.reads += 1
            return super().result()

    for split in SHARD_SPLITS:
        first = A.test_model_corpus_window_shards(m, shard_dicts(raw, split), queries, gt_video, gt_times, **kw)     # first use outside the checked region
        torch.cuda.synchronize()
        Counting.reads = 0
        mode = torch.cuda.get_sync_debug_mode()
        torch.cuda.set_sync_debug_mode("error")
        try:
            got = A.test_model_corpus_window_shards(m, shard_dicts(raw, split), queries, gt_video, gt_times, Counting(n=(1, 5), device=dev), **kw)
        finally:
            torch.cuda.set_sync_debug_mode(mode)
        print("split", split, got)
        assert Counting.reads == 1 and got == want == first and got["num_samples"] == 4
    # planted truth: rank 1 of each query's whole-bank list
    top = A.test_model_corpus_window_shards(m, shard_dicts(raw, [2, 3]), queries, r["video"][:, 0].numpy(), r["times"][:, 0].numpy(), **kw)
    assert all(top[key] == 1.0 for key in top if key != "num_samples"), top
    # an empty shard of zero-row videos leaves the meter's state as it is
    a, b = A.CorpusMeter(n=(1, 5), device=dev), A.CorpusMeter(n=(1, 5), device=dev)
    shards = shard_dicts(raw, [2, 3])
    A.test_model_corpus_window_shards(m, shards, queries, gt_video, gt_times, a, **kw)
    A.test_model_corpus_window_shards(m, shards + [dict(raw=raw[:0], lengths=[0, 0], duration=np.ones(2))], queries, gt_video, gt_times, b, **kw)
    assert torch.equal(a.state.cpu().view(torch.int64), b.state.cpu().view(torch.int64)) and a.state[0].item() == 4
    assert int(A._lib.load_torch().layout_status(dev)[0]) == 0


@pytest.mark.gpu
def test_nothing_else_moved(dev, world):
    """merge_search, corpus_span_topk, search_windows (with and without duration) and test_model_corpus_windows give the bits of their
    restatements, before and after a sharded run, and the same bits both times"""
    A = V()
    m, raw, qb, wb = world["m"], world["raw"], world["qb"], world["wb"]
    queries = dict(query_features=world["qf"], query_mask=world["qm"])
    cells, cell_off = cell_shards(pair_lists(6, 4, 3, seed=3), 6, 4, [2, 4], 5)
    spans = random_span_lists([0, 1, 7, 3], 3, seed=14, garbage=float("nan"))
    duration = torch.from_numpy(DURATION).to(dev)
    scorer = lambda wi, wq: m.score_pairs(wb, qb, wi, wq)
    gt_video, gt_times = np.array([0, 4, 2, 1]), np.tile([1.0, 6.0], (4, 1))

    def everything():
        a = A.merge_search([to_dev(s, dev) for s in cells], cell_off, k=5)
        want = A.merge_search_torch(cells, cell_off, k=5)
        assert all(torch.equal(a[key].cpu(), want[key]) for key in ("video", "idx", "count")) and torch.equal(bits(a["score"]), bits(want["score"]))
        b = A.corpus_span_topk(*[t.to(dev) for t in spans], k=5)
        same_lists(b, A.corpus_span_topk_torch(*spans, k=5), "corpus_span_topk")
        c = m.search_windows(wb, qb, duration=duration, max_batch=7, **KW)
        d = m.search_windows(wb, qb, max_batch=7, **KW)
        equal = m.search_windows_torch(wb, qb, duration=torch.from_numpy(DURATION), max_batch=7, scorer=scorer, **KW)
        for key in KEYS + ("times",):
            assert torch.equal(c[key].cpu().contiguous().view(torch.uint8), equal[key].cpu().contiguous().view(torch.uint8)), key
        same_lists(d, c, "without duration")
        assert "times" not in d
        e = A.test_model_corpus_windows(m, raw, LENGTHS, queries, gt_video, gt_times, DURATION, window=WINDOW, stride=STRIDE, k=25, k_video=5)
        big = to_cpu(m.search_windows(wb, qb, k=25, k_video=5, duration=duration))
        meter = A.CorpusMeterTorch(n=(1, 5))
        meter.update(big, torch.from_numpy(gt_video), torch.from_numpy(gt_times).float())
        assert e == meter.result()
        return [v.cpu().contiguous().view(torch.uint8) for r in (a, b, c, d) for v in r.values()] + [torch.tensor(list(e.values()), dtype=torch.float64)]

    before = everything()
    A.test_model_corpus_window_shards(m, shard_dicts(raw, [2, 3]), queries, gt_video, gt_times, window=WINDOW, stride=STRIDE, k=25, k_video=5)
    after = everything()
    assert len(before) == len(after) and all(torch.equal(x, y) for x, y in zip(before, after))
