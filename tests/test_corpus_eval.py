"""Evaluation of corpus search: moments.merge_search (csrc/corpus.hip, smin_search_merge), distributed.gather_search,
meter.CorpusMeter (csrc/metrics.hip, smin_corpus_meter_update) and training.test_model_corpus.

Host: the C ABI surface and its rejections, merge_search_torch and CorpusMeterTorch on hand-made lists, the exactness of merging the
lists of disjoint shards (at once and folded), the refusals, two gloo ranks.
GPU: the two kernels bit for bit against their restatements, corpus_topk and merge_search on the same data, test_model_corpus end to
end against the flow restated on the CPU and against planted ground truth, without host reads and without moving anything else."""
import ctypes
import multiprocessing as mp
import os
import re

import numpy as np
import pytest
import torch

from tests import helpers as H
from tests.support.device import dev  # noqa: F401  (the module's device fixture)
from tests.support.device import free_port, to_dev, vml as V
from tests.support.compare import bits, same_merge
from tests.support.corpora import build_model, cell_topk_of as topk_of, corpus_inputs, pair_lists, shards_of, tiny_model, DURATION, SCORE_TOL

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = ("video", "idx", "score", "count")
SPLITS = ([3, 4], [1, 1, 5], [7], [2, 2, 2, 1])


def same_lists(got, want, what=""):
    same_merge(got, {key: want[key].cpu() for key in KEYS}, what)


# ---------------------------------------------------------------- shared data
def with_garbage(r, garbage):
    """the ranked list r with ``garbage`` scores (and foreign ids) behind its counts"""
    k = r["score"].shape[1]
    unused = torch.arange(k).unsqueeze(0) >= r["count"].to(torch.int64).unsqueeze(1)
    return {"score": torch.where(unused, torch.full_like(r["score"], garbage), r["score"]),
            "video": torch.where(unused, torch.full_like(r["video"], 777), r["video"]),
            "idx": torch.where(unused.unsqueeze(2), torch.full_like(r["idx"], 777), r["idx"]), "count": r["count"]}


def hand_meter_case():
    """Three queries of 5 entries (n = (1, 2, 5), m = (0.3, 0.5, 0.7)), worked out on paper.
    Query 0, truth video 3 at (2, 6): videos [7, 3, 7, 3, 9]; rank 1 is the truth's span in another video (IoU 0); rank 2 is (2, 10):
      inter 4 / union 8 = 0.5 exactly -- a hit at 0.3, a miss at 0.5 (strict); rank 4 is (2, 6): IoU 1.  One distinct video (7) lies
      ahead of video 3: VR@1 misses, VR@2 and VR@5 hit.  Top-1 IoU 0.
    Query 1, truth video 3 at (0, 4): videos [3, 3, 7, 9, 9]; rank 1 is (0, 3): IoU 0.75: every R@n and VR@n hits.  Top-1 IoU 0.75.
    Query 2, truth video 3: videos [1, 2, 1, 2, 1]: a miss everywhere."""
    video = torch.tensor([[7, 3, 7, 3, 9], [3, 3, 7, 9, 9], [1, 2, 1, 2, 1]], dtype=torch.int64)
    times = torch.tensor([[[2, 6], [2, 10], [0, 1], [2, 6], [2, 6]],
                          [[0, 3], [0, 4], [0, 4], [0, 4], [0, 4]],
                          [[0, 4], [0, 4], [0, 4], [0, 4], [0, 4]]], dtype=torch.float32)
    result = {"video": video, "idx": torch.zeros(3, 5, 2, dtype=torch.int64), "score": torch.zeros(3, 5), "times": times,
              "count": torch.tensor([5, 5, 5], dtype=torch.int32)}
    gt_video = torch.tensor([3, 3, 3], dtype=torch.int64)
    gt = torch.tensor([[2.0, 6.0], [0.0, 4.0], [0.0, 4.0]])
    want = {"R@1, IoU=0.3": 1 / 3, "R@1, IoU=0.5": 1 / 3, "R@1, IoU=0.7": 1 / 3,
            "R@2, IoU=0.3": 2 / 3, "R@2, IoU=0.5": 1 / 3, "R@2, IoU=0.7": 1 / 3,
            "R@5, IoU=0.3": 2 / 3, "R@5, IoU=0.5": 2 / 3, "R@5, IoU=0.7": 2 / 3,
            "VR@1": 1 / 3, "VR@2": 2 / 3, "VR@5": 2 / 3, "mIoU": 0.75 / 3, "num_samples": 3}
    return result, gt_video, gt, want


# ---------------------------------------------------------------- host: surface
def test_header_and_table_declare_the_entry_points():
    text = open(os.path.join(ROOT, "include", "smin_hip.h")).read()
    for name, ret in (("smin_search_merge", "int"), ("smin_corpus_meter_update", "int"), ("smin_corpus_meter_ws_bytes", "size_t")):
        assert re.search(r"\b" + ret + r"\s+" + name + r"\s*\(", text), name
        assert name in V()._lib.SIGNATURES, name
        assert hasattr(V()._lib.load(), name)
    assert "#define SMIN_HIP_ABI_VERSION 2" in text and V()._lib.ABI_VERSION == 2
    for name in ("merge_search", "merge_search_torch", "CorpusMeter", "CorpusMeterTorch", "test_model_corpus"):
        assert hasattr(V(), name), name
    assert hasattr(V().distributed, "gather_search") and V().test_model_corpus.__test__ is False


# ---------------------------------------------------------------- host: the restated merge
def hand_lists(count0):
    nan = float("nan")
    a = {"video": torch.tensor([[5, 5, 3], [12, 99, 99]]), "score": torch.tensor([[0.5, 0.5, 0.25], [-0.0, nan, nan]]),
         "idx": torch.arange(12).reshape(2, 3, 2), "count": torch.tensor(count0, dtype=torch.int32)}
    b = {"video": torch.tensor([[0, 2, 99], [1, 3, 4]]), "score": torch.tensor([[0.5, 0.25, nan], [0.5, 0.0, -1.0]]),
         "idx": 100 + torch.arange(12).reshape(2, 3, 2), "count": torch.tensor([2, 5], dtype=torch.int32)}
    return [a, b]


def test_merge_search_torch_by_hand():
    f = V().merge_search_torch
    r = f(hand_lists([3, 1]), [0, 10], k=4)
    # query 0: 0.5 on videos 5 (twice, in list order) and 0 + 10; then 0.25 on video 3 ahead of 2 + 10.  Without the offsets video 0 led.
    # query 1: 0.5 (1 + 10); -0 on video 12 ties with +0 on 3 + 10 and goes first by video; then -1 (count 5 is clamped to the 3 slots)
    assert r["video"].tolist() == [[5, 5, 10, 3], [11, 12, 13, 14]]
    assert r["idx"].tolist() == [[[0, 1], [2, 3], [100, 101], [4, 5]], [[106, 107], [6, 7], [108, 109], [110, 111]]]
    assert r["score"][0].tolist() == [0.5, 0.5, 0.5, 0.25] and r["score"][1].tolist() == [0.5, 0.0, 0.0, -1.0]
    assert r["score"][1, 1:3].view(torch.int32).tolist() == [-2 ** 31, 0]                # the scores leave as stored: -0 stays -0
    assert r["count"].tolist() == [4, 4] and r["count"].dtype == torch.int32 and r["video"].dtype == torch.int64
    # a count of 0 lists nothing: query 1 is list 1's three entries and an empty slot
    r = f(hand_lists([3, 0]), [0, 10], k=4)
    assert r["video"].tolist() == [[5, 5, 10, 3], [11, 13, 14, -1]] and r["count"].tolist() == [4, 3]
    assert r["idx"][1, 3].tolist() == [-1, -1] and r["score"][1].tolist() == [0.5, 0.0, -1.0, 0.0]
    for count0 in ([3, 1], [3, 0], [0, 0]):
        for k in (1, 4, 64):
            r = f(hand_lists(count0), [0, 10], k=k)
            assert not torch.isnan(r["score"]).any() and not (r["video"] == 99).any()  # nothing behind the counts is ever listed
    # times: search's formula on the global video
    duration = torch.arange(1.0, 16.0)
    r = f(hand_lists([3, 1]), [0, 10], k=4, duration=duration, L=8)
    want = (r["idx"].float() + torch.tensor([0.0, 1.0])) * duration[r["video"]].reshape(2, 4, 1) / 8
    assert torch.equal(r["times"], want)


@pytest.mark.parametrize("K", [1, 3, 5, 9])
def test_sharding_is_exact(K):
    """merge_search_torch of the shards' corpus_topk_torch(k=K) lists is corpus_topk_torch on the whole corpus, bit for bit, merged at
    once and folded one shard after another: V = 7, Q = 3, k_video = 3, scores from six values, random counts."""
    A = V()
    nv, Q, kv = 7, 3, 3
    for seed in range(25):
        lists = pair_lists(nv, Q, kv, seed)
        whole = topk_of(lists, nv, Q, 0, nv, K)
        for split in SPLITS:
            shards, offsets = shards_of(lists, nv, Q, split, K)
            same_lists(A.merge_search_torch(shards, offsets, k=K), whole, (seed, split, "at once"))
            carry = shards[0]
            for r, off in zip(shards[1:], offsets[1:]):
                carry = A.merge_search_torch([carry, r], [0, off], k=K)
            same_lists(carry if len(shards) > 1 else A.merge_search_torch([carry], [0], k=K), whole, (seed, split, "folded"))


def test_fold_of_more_than_sixteen_lists():
    """moments.fold_search, what gather_search runs over the ranks' lists: 17, 31 and 40 one-video shards folded 16, then 15 at a time
    with the carry at offset 0, give the whole corpus' list"""
    A = V()
    for nv, K in ((17, 5), (31, 3), (40, 9)):
        lists = pair_lists(nv, 3, 3, seed=nv)
        shards, offsets = shards_of(lists, nv, 3, [1] * nv, K)
        calls = []

        def merge(ls, off, k):
            calls.append((len(ls), off[0], off[1] if len(off) > 1 else None))
            return A.merge_search_torch(ls, off, k=k)

        same_lists(A.moments.fold_search(shards, offsets, K, merge), topk_of(lists, nv, 3, 0, nv, K), nv)
        assert calls[0] == (16, 0, 1) and calls[1][:2] == (min(16, nv - 15), 0) and calls[1][2] == 16
        assert len(calls) == 1 + -(-(nv - 16) // 15) and all(n <= 16 for n, _, _ in calls)


# ---------------------------------------------------------------- host: the restated meter
def test_corpus_meter_torch_by_hand():
    A = V()
    result, gt_video, gt, want = hand_meter_case()
    meter = A.CorpusMeterTorch(n=(1, 2, 5), m=(0.3, 0.5, 0.7))
    meter.update(result, gt_video, gt)
    got = meter.result()
    assert list(got) == list(want)                                                   # R@n, IoU=m, then VR@n, mIoU, num_samples
    assert got == want
    assert meter.state.tolist() == [3.0, 0.0, 0.0, 0.75, 1, 1, 1, 2, 1, 1, 2, 2, 2, 1, 2, 2]
    # clip edges (i, j + 1) from idx when the list carries no times: the same numbers
    by_idx = {key: v for key, v in result.items() if key != "times"}
    by_idx["idx"] = (result["times"] - torch.tensor([0.0, 1.0])).to(torch.int64)
    again = A.CorpusMeterTorch(n=(1, 2, 5), m=(0.3, 0.5, 0.7))
    again.update(by_idx, gt_video, gt)
    assert torch.equal(again.state, meter.state)
    # a second update accumulates; a count of 0 is a miss that still counts as a query; reset() zeroes
    result["count"] = torch.tensor([5, 0, 5], dtype=torch.int32)
    meter.update(result, gt_video, gt)
    assert meter.state.tolist() == [6.0, 0.0, 0.0, 0.75, 1, 1, 1, 3, 1, 1, 3, 3, 3, 1, 3, 3]
    meter.reset()
    assert meter.state.eq(0).all()


def random_meter_case(Q, k, seed, nan_behind=True):
    g = torch.Generator().manual_seed(seed)
    video = torch.randint(0, 6, (Q, k), generator=g, dtype=torch.int64)
    st = torch.randint(0, 12, (Q, k), generator=g).float()
    times = torch.stack([st, st + torch.randint(1, 9, (Q, k), generator=g).float()], dim=2)
    count = torch.randint(0, k + 1, (Q,), generator=g, dtype=torch.int32)
    if nan_behind:
        unused = torch.arange(k).unsqueeze(0) >= count.unsqueeze(1)
        times = torch.where(unused.unsqueeze(2), torch.full_like(times, float("nan")), times)
    gt_video = torch.randint(0, 7, (Q,), generator=g, dtype=torch.int64)           # video 6 is in no list
    gs = torch.randint(0, 12, (Q,), generator=g).float()
    gt = torch.stack([gs, gs + torch.randint(1, 9, (Q,), generator=g).float()], dim=1)
    result = {"video": video, "idx": torch.zeros(Q, k, 2, dtype=torch.int64), "score": torch.zeros(Q, k), "times": times, "count": count}
    return result, gt_video, gt


def brute_force_hits(result, gt_video, gt, n, m):
    """the definitions as a Python loop, the IoU in numpy fp32 scalars"""
    f = np.float32
    Q, k = result["video"].shape
    out = {f"R@{a}, IoU={c}": 0 for a in n for c in m}
    out.update({f"VR@{a}": 0 for a in n})
    for q in range(Q):
        cnt = min(max(int(result["count"][q]), 0), k)
        vids = result["video"][q, :cnt].tolist()
        gs, ge = f(gt[q, 0].item()), f(gt[q, 1].item())
        ious = []
        for r in range(cnt):
            st, en = f(result["times"][q, r, 0].item()), f(result["times"][q, r, 1].item())
            inter, uni = max(f(0), min(en, ge) - max(st, gs)), max(en, ge) - min(st, gs)
            ious.append(f(inter) / f(uni) if vids[r] == int(gt_video[q]) and uni > 0 else f(0))
        for a in n:
            for c in m:
                out[f"R@{a}, IoU={c}"] += any(x > f(c) for x in ious[:a])
            if int(gt_video[q]) in vids:
                out[f"VR@{a}"] += len(set(vids[:vids.index(int(gt_video[q]))])) < a
    return out


def test_corpus_meter_torch_against_brute_force():
    n, m = (1, 2, 5, 8), (0.1, 0.3, 0.5, 0.7)
    result, gt_video, gt = random_meter_case(50, 8, seed=2)
    assert (result["count"] == 0).any() and (gt_video == 6).any()
    meter = V().CorpusMeterTorch(n=n, m=m)
    meter.update(result, gt_video, gt)
    want = brute_force_hits(result, gt_video, gt, n, m)
    print(want)
    assert 0 < want["VR@1"] < want["VR@8"] < 50 and want["R@1, IoU=0.1"] < want["R@8, IoU=0.1"] and want["R@8, IoU=0.7"] < want["R@8, IoU=0.1"]
    got = dict(zip(meter.keys, meter.state[4:].tolist()))
    assert got == {key: float(v) for key, v in want.items()}
    assert meter.state[0].item() == 50.0


# ---------------------------------------------------------------- host: rejection before any launch
def test_c_abi_rejects_before_any_launch():
    """smin_search_merge and smin_corpus_meter_update return a nonzero status without launching anything (so this runs without a device,
    on addresses that are never dereferenced); Q = 0 is accepted and does nothing."""
    lib = V()._lib.load()
    fake, out = 0x10000, 0x20000

    def merge(S=2, K=5, Q=3, ks=(3, 3), off=(0, 4), tables="visc", outs=(out, out + 0x100, out + 0x200, out + 0x300), k_list=True, entry=fake):
        table = lambda on: (ctypes.c_void_p * 17)(*([entry] * 17)) if on else None
        kl = (ctypes.c_int32 * 17)(*(list(ks) + [3] * (17 - len(ks)))) if k_list else None
        ol = (ctypes.c_int64 * 17)(*(list(off) + [0] * (17 - len(off))))
        return lib.smin_search_merge(None, S, *[table(c in tables) for c in "visc"], kl, ol, Q, K, *outs)

    assert merge(S=0) != 0 and merge(S=17) != 0 and merge(S=-1) != 0
    assert merge(K=65) != 0 and merge(K=0) != 0
    assert merge(ks=(3, 0)) != 0 and merge(ks=(65, 3)) != 0 and merge(ks=(3, 0), Q=0) != 0
    assert merge(Q=-1) != 0
    for tables in ("isc", "vsc", "vic", "vis"):
        assert merge(tables=tables) != 0, tables
    assert merge(k_list=False) != 0 and merge(entry=None) != 0
    for o in range(4):
        outs = [out, out + 0x100, out + 0x200, out + 0x300]
        outs[o] = None
        assert merge(outs=tuple(outs)) != 0, o
        outs[o] = fake                                                               # an output that is one of the inputs
        assert merge(outs=tuple(outs)) != 0, o
    assert merge(off=(0, -1)) != 0
    assert merge(Q=0) == 0 and merge(Q=0, tables="", outs=(None,) * 4) == 0 and merge(S=16, Q=0, ks=(64,) * 16) == 0

    def meter(Q=8, k=5, n=(1, 5), m=(0.1, 0.5), ptrs=(fake,) * 5, acc=fake, ws=fake, ws_bytes=None, nn=None, nm=None):
        nl, ml = (ctypes.c_int * 65)(*(list(n) + [1] * (65 - len(n)))), (ctypes.c_float * 17)(*(list(m) + [0.5] * (17 - len(m))))
        need = lib.smin_corpus_meter_ws_bytes(max(Q, 1), len(n), len(m))
        return lib.smin_corpus_meter_update(None, *ptrs, Q, k, ctypes.cast(nl, ctypes.c_void_p), len(n) if nn is None else nn,
                                            ctypes.cast(ml, ctypes.c_void_p), len(m) if nm is None else nm, acc, ws, need if ws_bytes is None else ws_bytes)

    assert lib.smin_corpus_meter_ws_bytes(8, 2, 4) >= 8 * (8 + 2) * 4 + 8 * 4
    for bad in ((0, 2, 4), (-1, 2, 4), (8, 0, 4), (8, 65, 4), (8, 2, 0), (8, 2, 17)):
        assert lib.smin_corpus_meter_ws_bytes(*bad) == 0, bad
    assert meter(n=(1, 6)) != 0 and meter(n=(0, 5)) != 0                             # an n outside 1..k
    assert meter(k=0) != 0 and meter(k=65, n=(1, 5)) != 0
    assert meter(nn=0) != 0 and meter(nn=65) != 0 and meter(nm=0) != 0 and meter(nm=17) != 0
    assert meter(Q=-1) != 0
    assert meter(ws_bytes=lib.smin_corpus_meter_ws_bytes(8, 2, 2) - 1) != 0
    for p in range(5):
        ptrs = [fake] * 5
        ptrs[p] = None
        assert meter(ptrs=tuple(ptrs)) != 0, p
    assert meter(acc=None) != 0 and meter(ws=None) != 0
    assert meter(Q=0) == 0 and meter(Q=0, ptrs=(None,) * 5, acc=None, ws=None, ws_bytes=0) == 0


# ---------------------------------------------------------------- host: refusals
def test_refusals():
    A = V()
    err = A._lib.SminHipError
    lists = hand_lists([3, 1])
    with pytest.raises(err, match="no CPU fallback"):
        A.merge_search(lists, [0, 10], k=4)
    for f in (A.merge_search, A.merge_search_torch):
        with pytest.raises(ValueError, match="1..16"):
            f([lists[0]] * 17)
        with pytest.raises(ValueError, match="1..16"):
            f([])
        with pytest.raises(ValueError, match="one Q"):
            f([lists[0], {key: v[:1] for key, v in lists[1].items()}])
        for k in (0, 65, 2.0):
            with pytest.raises(ValueError, match="integer 1 <= k"):
                f(lists, k=k)
        wide = {"video": torch.zeros(2, 65, dtype=torch.int64), "idx": torch.zeros(2, 65, 2, dtype=torch.int64), "score": torch.zeros(2, 65),
                "count": torch.zeros(2, dtype=torch.int32)}
        with pytest.raises(ValueError, match="slots per query"):
            f([lists[0], wide])
        with pytest.raises(ValueError, match="video_offset"):
            f(lists, [0, -1])
        with pytest.raises(ValueError, match="video_offset"):
            f(lists, [0])
        with pytest.raises(ValueError, match="need L"):
            f(lists, [0, 10], duration=torch.ones(15))
    result, gt_video, gt, _ = hand_meter_case()
    with pytest.raises(err, match="CorpusMeterTorch"):
        A.CorpusMeter(n=(1, 5), device="cpu").update(result, gt_video, gt)
    for cls in (A.CorpusMeter, A.CorpusMeterTorch):
        with pytest.raises(ValueError, match="R@6"):
            cls(n=(1, 6), device="cpu").update(result, gt_video, gt)                 # lists of 5 entries
        with pytest.raises(ValueError, match=r"\(Q,\)"):
            cls(n=(1, 5), device="cpu").update(result, gt_video[:2], gt)
        with pytest.raises(ValueError):
            cls(n=(1, 65), device="cpu")
        with pytest.raises(ValueError):
            cls(m=(0.5,) * 17, device="cpu")
    # test_model_corpus: before any device work (a host model and host tensors would raise SminHipError at the first encoder)
    m, _ = tiny_model()
    vid, qry, _ = corpus_inputs()
    shards = [dict(vid, duration=np.ones(5))]
    gv, gtimes = np.zeros(4, dtype=np.int64), np.ones((4, 2))
    with pytest.raises(ValueError, match="max\\(n\\) \\* k_video"):
        A.test_model_corpus(m, shards, qry, gv, gtimes, k=9, k_video=2)                  # the default meter: n = (1, 5)
    with pytest.raises(ValueError, match="max\\(n\\) \\* k_video"):
        A.test_model_corpus(m, shards, qry, gv, gtimes, A.CorpusMeterTorch(n=(1, 5)), k=4, k_video=1)
    with pytest.raises(err, match="no CPU fallback"):
        A.test_model_corpus(m, shards, qry, gv, gtimes)                                  # the defaults hold (k = 25 = 5 * 5) and reach the encoders


# ---------------------------------------------------------------- host: two gloo ranks
GLOO = dict(nv=7, Q=3, kv=3, K=5, seed=4, split=[3, 4])


def _gather_worker(rank, world, port, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), WORLD_SIZE=str(world), RANK=str(rank), LOCAL_RANK=str(rank))
    torch.set_num_threads(2)
    A = V()
    D = A.distributed
    D.init(backend="gloo")
    c = GLOO
    lists = pair_lists(c["nv"], c["Q"], c["kv"], c["seed"])
    shards, _ = shards_of(lists, c["nv"], c["Q"], c["split"], c["K"])
    got = D.gather_search(shards[rank], c["split"][rank], merge=A.merge_search_torch)
    cut = D.gather_search(shards[rank], c["split"][rank], k=2, merge=A.merge_search_torch)
    refused = False
    try:
        D.gather_search(shards[rank], c["split"][rank], k=3 + rank, merge=A.merge_search_torch)
    except ValueError as e:
        refused = "same queries" in str(e)
    D.barrier()
    q.put((rank, refused, {key: got[key].numpy() for key in KEYS}, {key: cut[key].numpy() for key in KEYS}))
    torch.distributed.destroy_process_group()


@pytest.mark.timeout(300)
def test_two_gloo_ranks_return_the_whole_corpus_list():
    """Each of two ranks holds the corpus_topk_torch list of its shard ([3, 4] of the 7 videos): gather_search(merge=merge_search_torch)
    returns the whole corpus' list on both, bitwise equal; ranks that pass different k raise ValueError on both."""
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
    lists = pair_lists(c["nv"], c["Q"], c["kv"], c["seed"])
    whole, whole2 = topk_of(lists, c["nv"], c["Q"], 0, c["nv"], c["K"]), topk_of(lists, c["nv"], c["Q"], 0, c["nv"], 2)
    assert int(whole["video"].max()) >= 3                                            # the second rank's videos are listed, with their offset
    for rank, refused, got, cut in res:
        assert refused, rank
        for key in KEYS:
            assert got[key].tobytes() == whole[key].numpy().tobytes() == res[0][2][key].tobytes(), (rank, key)
            assert cut[key].tobytes() == whole2[key].numpy().tobytes(), (rank, key)


# ---------------------------------------------------------------- GPU
@pytest.mark.gpu
@pytest.mark.parametrize("S", [1, 2, 3])
@pytest.mark.parametrize("K", [1, 5, 64])
def test_merge_kernel_small(dev, S, K):
    """Q = 4 (query 2 with every count 0), S lists of k_s = 3 over shards of 3 videos, non-zero offsets, ties everywhere; NaN or 1e30
    behind the counts give the same list, merge_search_torch's, bit for bit."""
    A = V()
    nv, Q = 3 * S, 4
    lists = pair_lists(nv, Q, 3, seed=10 + S, empty_query=2)
    shards, offsets = shards_of(lists, nv, Q, [3] * S, 3)
    offsets = [o + 5 for o in offsets]
    want = A.merge_search_torch(shards, offsets, k=K)
    assert want["count"][2] == 0 and int(want["count"].max()) == min(K, max(int(sum(s["count"][q] for s in shards)) for q in range(Q)))
    for garbage in (float("nan"), 1e30):
        dirty = [with_garbage(s, garbage) for s in shards]
        assert sum(int((d["video"] == 777).sum()) for d in dirty) > 0
        got = A.merge_search([to_dev(d, dev) for d in dirty], offsets, k=K)
        same_lists(got, want, garbage)
    if S == 1:                                                                       # one list: itself plus its offset, cut or padded to K
        n = min(K, 3)
        got = {key: v.cpu() for key, v in got.items()}
        filled = torch.arange(n).unsqueeze(0) < shards[0]["count"].unsqueeze(1)
        assert torch.equal(got["video"][:, :n], torch.where(filled, shards[0]["video"][:, :n] + 5, torch.full((Q, n), -1)))
        assert torch.equal(got["idx"][:, :n], shards[0]["idx"][:, :n]) and torch.equal(bits(got["score"][:, :n]), bits(shards[0]["score"][:, :n]))
        assert got["video"][:, n:].eq(-1).all() and got["idx"][:, n:].eq(-1).all() and got["score"][:, n:].eq(0).all()
        assert torch.equal(got["count"], shards[0]["count"].clamp(max=K))


@pytest.mark.gpu
def test_merge_kernel_sixteen_lists_of_64(dev):
    """S = 16, k_s = 64, K = 64: 1024 candidates per query, four passes of the 256-thread loop (query 0 has every slot filled)"""
    A = V()
    nv, Q = 16 * 8, 3
    lists = pair_lists(nv, Q, 8, seed=7, full_query=0)
    shards, offsets = shards_of(lists, nv, Q, [8] * 16, 64)
    assert all(int(s["count"][0]) == 64 for s in shards) and any(int(s["count"][1]) < 64 for s in shards)
    want = A.merge_search_torch(shards, offsets, k=64)
    got = A.merge_search([to_dev(with_garbage(s, float("nan")), dev) for s in shards], offsets, k=64)
    same_lists(got, want)
    assert want["count"].tolist()[0] == 64 and len(set(want["video"][0].tolist())) > 16     # from well past the first 256 candidates
    same_lists(got, topk_of(lists, nv, Q, 0, nv, 64), "the whole corpus")


@pytest.mark.gpu
def test_merge_kernel_lists_of_different_k(dev):
    A = V()
    nv, Q = 12, 5
    lists = pair_lists(nv, Q, 8, seed=9, full_query=1)
    edges = [0, 2, 12]
    shards = [topk_of(lists, nv, Q, 0, 2, 2), topk_of(lists, nv, Q, 2, 12, 64)]
    for K in (3, 64):
        want = A.merge_search_torch(shards, edges[:2], k=K)
        same_lists(A.merge_search([to_dev(with_garbage(s, 1e30), dev) for s in shards], edges[:2], k=K), want, K)
    assert int(want["count"][1]) == 64


def edge_lists(ks, Q, seed):
    """len(ks) lists of ks[s] slots: scores from six values with a NaN, both zeros and a repeated value among them, local videos in
    [0, 3) (with equal or overlapping offsets the lists name the same global videos: the list and the position decide), counts that
    walk through k_s + 2, -1, 0, k_s and 1; query 1, where there is one, has no entry in any list"""
    g = torch.Generator().manual_seed(seed)
    values = torch.tensor([float("nan"), 0.5, 0.5, 0.0, -0.0, -0.25])
    out = []
    for s, k in enumerate(ks):
        count = torch.tensor([(k + 2, -1, 0, k, 1)[(q + s) % 5] for q in range(Q)], dtype=torch.int32)
        if Q > 1:
            count[1] = (0, -1)[s % 2]
        out.append({"video": torch.randint(0, 3, (Q, k), generator=g, dtype=torch.int64), "idx": torch.randint(0, 64, (Q, k, 2), generator=g, dtype=torch.int64),
                    "score": values[torch.randint(0, 6, (Q, k), generator=g)], "count": count})
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("S", [1, 2, 16])
@pytest.mark.parametrize("K", [1, 64])
def test_merge_kernel_edges(dev, S, K):
    """What the lists cut from corpus_topk_torch leave out: k_s mixing 1 and 64, Q = 1 and 3, counts below 0 and above k_s, a query
    without an entry, one global video at one score in several lists and in several slots of a list, -0 against +0 and NaN scores
    (the highest order word) -- every output against merge_search_torch, bit for bit."""
    A = V()
    nans = 0
    for ks in ([(64, 1)[s % 2] for s in range(S)], [(1, 64)[s % 2] for s in range(S)]):
        for Q in (1, 3):
            lists = edge_lists(ks, Q, seed=100 * S + Q + ks[0])
            for offsets in ([0] * S, list(range(S))):
                want = A.merge_search_torch(lists, offsets, k=K)
                assert int(want["count"][0]) == min(K, sum(min(max(int(r["count"][0]), 0), k) for r, k in zip(lists, ks)))
                assert Q == 1 or int(want["count"][1]) == 0
                nans += int(torch.isnan(want["score"]).sum())
                same_lists(A.merge_search([to_dev(r, dev) for r in lists], offsets, k=K), want, (ks, Q, offsets))
    assert nans > 0


@pytest.mark.gpu
@pytest.mark.parametrize("K", [1, 5, 64])
def test_corpus_topk_and_merge_search_agree(dev, K):
    """One list per video (k_s = k_video, offset = the video) through merge_search is corpus_topk of the pair lists: the shared K-round
    loop serves both ways of reading a candidate."""
    A = V()
    nv, Q, kv = 7, 4, 3
    score, idx, count = pair_lists(nv, Q, kv, seed=21, empty_query=3)
    video = torch.arange(nv, dtype=torch.int32).repeat(Q)
    ptr = torch.arange(Q + 1, dtype=torch.int32) * nv
    top = A.corpus_topk(*[t.to(dev) for t in (score, idx, count, video, ptr)], k=K)
    per_video = [{"video": torch.zeros(Q, kv, dtype=torch.int64), "idx": idx[v::nv], "score": score[v::nv], "count": count[v::nv]} for v in range(nv)]
    merged = A.merge_search([to_dev(r, dev) for r in per_video], list(range(nv)), k=K)
    same_lists(merged, top)
    same_lists(top, A.corpus_topk_torch(score, idx, count, video, ptr, k=K))


def state_bits(meter):
    return meter.state.detach().cpu().view(torch.int64)


@pytest.mark.gpu
@pytest.mark.parametrize("Q", [1, 5, 67])
@pytest.mark.parametrize("k", [1, 5, 64])
def test_meter_kernel_against_torch(dev, Q, k):
    """CorpusMeter's state after two updates is CorpusMeterTorch's, bit for bit: queries whose video is absent, counts of 0, NaN spans
    behind the counts; Q = 67 is two workgroups, the second partial."""
    A = V()
    n, m = tuple(sorted({1, min(5, k), k})), (0.1, 0.5, 0.7)
    a, b = A.CorpusMeter(n=n, m=m, device=dev), A.CorpusMeterTorch(n=n, m=m)
    for seed in (Q * 100 + k, Q * 100 + k + 1):
        result, gt_video, gt = random_meter_case(Q, k, seed)
        if seed % 2:                                                                 # clip edges from idx instead of times
            result = {"video": result["video"], "count": result["count"], "idx": torch.nan_to_num(result["times"]).to(torch.int64) - torch.tensor([0, 1])}
        a.update(to_dev(result, dev), gt_video.to(dev), gt.to(dev))
        b.update(result, gt_video, gt)
    assert a.state.shape == (4 + len(n) * 3 + len(n),) and torch.equal(state_bits(a), state_bits(b))
    assert a.state[0].item() == 2 * Q and a.state[1].item() == 0 and a.state[2].item() == 0
    if Q == 67:
        assert 0 < a.state[4 + len(n) * 3].item() < 2 * Q                              # VR@1: some hit, some miss
    assert a.result() == b.result()


@pytest.mark.gpu
def test_meter_kernel_hand_case(dev):
    A = V()
    result, gt_video, gt, want = hand_meter_case()
    meter = A.CorpusMeter(n=(1, 2, 5), m=(0.3, 0.5, 0.7), device=dev)
    meter.update(to_dev(result, dev), gt_video.to(dev), gt.to(dev))
    got = meter.result()
    assert list(got) == list(want) and got == want
    meter.update({key: v[:0] for key, v in to_dev(result, dev).items()}, gt_video[:0].to(dev), gt[:0].to(dev))     # Q = 0: a no-op
    assert meter.result() == want
    meter.reset()
    assert meter.state.eq(0).all()


def shard_dicts(vid_d, split):
    edges = np.concatenate([[0], np.cumsum(split)]).tolist()
    return [dict({key: v[a:b] for key, v in vid_d.items()}, duration=DURATION[a:b]) for a, b in zip(edges[:-1], edges[1:])]


@pytest.fixture(scope="module")
def tiny(dev):
    m, _ = tiny_model(dev)
    # seed 1: in the oracle's scores three of the four queries have their second-best moment in another video than their best (by
    # 5e-3 or more, far above SCORE_TOL) and one has both in one video, which test_model_corpus_end_to_end's planted truth needs
    vid, qry, _ = corpus_inputs(seed=1)
    return dict(m=m, vid_d={key: v.to(dev) for key, v in vid.items()}, qry_d={key: v.to(dev) for key, v in qry.items()})


@pytest.mark.gpu
@pytest.mark.parametrize("split", [[2, 3], [1, 1, 1, 1, 1]])
def test_model_corpus_end_to_end(dev, tiny, split):
    A = V()
    m, vid_d, qry_d = tiny["m"], tiny["vid_d"], tiny["qry_d"]
    kw = dict(k=10, k_video=2)
    # the same flow restated: per-shard search, lists to the CPU, merge_search_torch fold, CorpusMeterTorch
    qb = m.encode_queries(qry_d["query_features"], qry_d["query_mask"])
    carry, seen = None, 0
    for shard in shard_dicts(vid_d, split):
        vb = m.encode_videos(shard["video_features"], shard["video_mask"], shard["length_mask"], shard["moment_mask"])
        r = {key: v.cpu() for key, v in m.search(vb, qb, **kw).items()}
        carry = r if carry is None else A.merge_search_torch([carry, r], [0, seen], k=10)
        seen += len(vb)
    carry["times"] = A.moments.search_times(carry["video"], carry["idx"], torch.from_numpy(DURATION), m.L)
    merged, duration = A.training.search_shards(m, shard_dicts(vid_d, split), qb, **kw)
    same_lists(merged, carry, "the folded list")
    assert duration.tolist() == DURATION.tolist() and int(carry["count"].min()) >= 5
    # against the whole bank: scores of differently composed batches, so only the sorted score vectors are compared
    vb = m.encode_videos(vid_d["video_features"], vid_d["video_mask"], vid_d["length_mask"], vid_d["moment_mask"])
    whole = m.search(vb, qb, **kw)
    diff = (whole["score"].cpu() - carry["score"]).abs().max().item()
    print("split", split, "sorted scores against the whole bank: max difference", diff)
    assert diff < 2 * SCORE_TOL

    def run(meter, gt_video, gt_times):
        return A.test_model_corpus(m, shard_dicts(vid_d, split), qry_d, gt_video, gt_times, meter, **kw)

    # an arbitrary truth: equal to the restated flow
    g = torch.Generator().manual_seed(1)
    gt_video = torch.randint(0, 5, (4,), generator=g).numpy()
    gt_times = np.stack([np.array([1.0, 0.5, 2.0, 0.0]), np.array([6.0, 3.0, 30.0, 5.0])], axis=1)
    want = A.CorpusMeterTorch(n=(1, 5))
    want.update(carry, torch.from_numpy(gt_video), torch.from_numpy(gt_times).float())
    got = run(A.CorpusMeter(n=(1, 5), device=dev), gt_video, gt_times)
    print("arbitrary truth", got)
    assert got == want.result() and got["num_samples"] == 4
    assert run(None, gt_video, gt_times) == got                                      # the default meter: n = (1, 5), the reference's m
    # planted truth: rank 1 of the merged list
    got = run(None, carry["video"][:, 0].numpy(), carry["times"][:, 0].numpy())
    assert all(got[key] == 1.0 for key in got if key != "num_samples"), got
    # rank 2: where it lies in another video than rank 1, the video is second and the moment is in the top 5 but not first
    other = carry["video"][:, 1] != carry["video"][:, 0]
    print("queries whose rank 2 is in another video than rank 1:", other.tolist())
    assert other.any()
    got = run(None, carry["video"][:, 1].numpy(), carry["times"][:, 1].numpy())
    assert got["VR@1"] == 1.0 - other.sum().item() / 4 and all(got[f"R@5, IoU={c}"] == 1.0 for c in (0.1, 0.3, 0.5, 0.7)) and got["VR@5"] == 1.0
    sub = A.CorpusMeter(device=dev)
    rows = other.nonzero().flatten()
    sub.update({key: v[rows].to(dev) for key, v in carry.items()}, carry["video"][rows, 1].to(dev), carry["times"][rows, 1].to(dev))
    got = sub.result()
    assert got["VR@1"] == 0.0 and got["R@1, IoU=0.7"] == 0.0 and got["mIoU"] == 0.0
    assert all(got[f"R@5, IoU={c}"] == 1.0 for c in (0.1, 0.3, 0.5, 0.7)) and got["VR@5"] == 1.0


@pytest.mark.gpu
def test_no_host_synchronisation(dev):
    A = V()
    lists = pair_lists(6, 4, 3, seed=3)
    shards, offsets = shards_of(lists, 6, 4, [2, 4], 5)
    shards = [to_dev(s, dev) for s in shards]
    duration = torch.arange(1.0, 7.0, device=dev)
    result, gt_video, gt = random_meter_case(4, 5, seed=8)
    result, gt_video, gt = to_dev(result, dev), gt_video.to(dev), gt.to(dev)
    meter = A.CorpusMeter(n=(1, 5), device=dev)
    first = A.merge_search(shards, offsets, k=5, duration=duration, L=8)             # first use outside the checked region
    meter.update(result, gt_video, gt)
    meter.update(first, gt_video, gt)
    torch.cuda.synchronize()
    mode = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        second = A.merge_search(shards, offsets, k=5, duration=duration, L=8)
        meter.update(result, gt_video, gt)
        meter.update(second, gt_video, gt)                                           # with times
        meter.update({key: second[key] for key in KEYS}, gt_video, gt)               # clip edges from idx
    finally:
        torch.cuda.set_sync_debug_mode(mode)
    same_lists(second, first)
    assert meter.state[0].item() == 20.0
    assert int(A._lib.load_torch().layout_status(dev)[0]) == 0


@pytest.mark.gpu
def test_nothing_else_moved(dev):
    """a train step's scores and gradients and a whole-bank search give the same bits before and after a test_model_corpus run"""
    A = V()
    cfg, sd, batch, _, _, _ = H.split_tiny(H.load_npz(H.TINY[0]))
    m = build_model(cfg, sd, dev)
    b = {k: v.to(dev) for k, v in batch.items()}
    xs = H.model_inputs(b)
    B = xs[0].shape[0]

    def step():
        m.train()
        m.zero_grad(set_to_none=True)
        out = m(*xs)
        A.loss_fn(out[0], b["ym"], b["sm"], b["moment_mask"], out[1], b["ys"], b["ss"], out[2], b["ye"], b["se"], out[3], b["ya"], b["length_mask"]).backward()
        torch.cuda.synchronize()
        vb, qb = m.encode_videos(xs[0], xs[1], xs[4], xs[5]), m.encode_queries(xs[2], xs[3])
        r = m.search(vb, qb, k=3, max_batch=3)
        return [bits(t) for t in m.score(*xs)] + [bits(t) for t in out] + [bits(p.grad) for p in m.parameters()] + \
            [r["video"].cpu(), r["idx"].cpu(), bits(r["score"]), r["count"].cpu()]

    before = step()
    shards = [dict(video_features=xs[0][a:c], video_mask=xs[1][a:c], length_mask=xs[4][a:c], moment_mask=xs[5][a:c], duration=np.ones(c - a))
              for a, c in ((0, 1), (1, B))]
    got = A.test_model_corpus(m, shards, dict(query_features=xs[2], query_mask=xs[3]), np.arange(B), np.tile([0.0, 1.0], (B, 1)), k=10, k_video=2)
    assert got["num_samples"] == B
    after = step()
    assert len(before) == len(after) and all(torch.equal(x, y) for x, y in zip(before, after))
