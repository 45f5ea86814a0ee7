"""The corpus-wide first-stage cut over shards: csrc/prefilter_fold.hip smin_prefilter_fold / smin_survivors_admit /
smin_prefilter_gt_rank, moments.prefilter_fold / survivors_admit / prefilter_gt_rank and their restatements, SurvivorBank with
SMIN.new_survivors / fold_survivors / search_survivors, and training.search_shards_prefiltered / test_model_corpus_prefiltered_shards.
Everything is bit for bit: no tolerance anywhere.

Host: prefilter_fold_torch applied shard after shard -- after every shard each query's slot videos are prefilter_select_torch of
rank_videos_torch on the scores concatenated so far, the slots are those of a hand-written loop of the slot rule, and the filled slots
are 0 .. min(M, seen) - 1 --; prefilter_gt_rank_torch against a loop; the C ABI surface and the refusals.
GPU, through the C ABI: smin_prefilter_fold against its restatement over M in {1, 5, 300} x Vs in {1, 5, 300, 700} from an empty, a
short and a 400-video history, on NaN / -7 pre-filled outputs between sentinel bands, twice, and every rejection; smin_survivors_admit
against the source bits with unaligned byte rows; smin_prefilter_gt_rank at V in {1, 5, 2500}.
GPU, end to end: search_shards_prefiltered over three splits against search(prefilter=M) on one bank, the loop without a host read,
test_model_corpus_prefiltered_shards against test_model_corpus fed the whole-bank pruned list."""
import inspect
import os
import re

import numpy as np
import pytest
import torch

from tests.support.device import dev  # noqa: F401  (the module's device fixture)
from tests.support.device import vml as V
from tests.support.compare import byte_bits as bits, same
from tests.support.guards import BAND, SENTINEL
from tests.support.corpora import corpus_inputs, tiny_model, video_shards, DURATION, GT_TIMES, GT_VIDEO, NO_ROWS, SEARCH_KEYS, TINY_SHAPE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PREFILTER_KEYS = ("prefilter_video", "prefilter_score", "prefilter_gt_rank")
VIDEO_KEYS = ("video_rank", "video_score", "video_count", "gt_rank")
SPLITS = [(5,), (1, 1, 1, 1, 1), (2, 3)]


# ---------------------------------------------------------------- host: surface
def test_header_table_and_names():
    A = V()
    text = open(os.path.join(ROOT, "include", "smin_hip.h")).read()
    lib = A._lib.load()
    for name, nargs in (("smin_prefilter_fold", 12), ("smin_survivors_admit", 15), ("smin_prefilter_gt_rank", 7)):
        assert re.search(r"\bint\s+%s\s*\(" % name, text), name
        assert name in A._lib.SIGNATURES and hasattr(lib, name), name
        assert len(A._lib.SIGNATURES[name]) == nargs, name
    assert "#define SMIN_HIP_ABI_VERSION 2" in text and lib.smin_abi_version() == 2          # exports only
    assert A.moments.PREFILTER_FOLD_MAX_M >= 1024 and "M <= %d" % A.moments.PREFILTER_FOLD_MAX_M in text
    for name in ("prefilter_fold", "survivors_admit", "prefilter_gt_rank"):
        for n in (name, name + "_torch"):
            assert callable(getattr(A, n)) and callable(getattr(A.moments, n)), n
    for name in ("search_shards_prefiltered", "test_model_corpus_prefiltered_shards"):
        assert callable(getattr(A, name)) and callable(getattr(A.training, name)), name
    assert A.test_model_corpus_prefiltered_shards.__test__ is False
    assert issubclass(A.SurvivorBank, A.VideoBank)
    import models
    for name in ("new_survivors", "fold_survivors", "search_survivors"):
        assert callable(getattr(models.SMIN, name)), name
    p = inspect.signature(models.SMIN.search_survivors).parameters
    assert [n for n in p][3:] == ["k", "k_video", "nms_thresh", "duration", "max_batch", "video_weight", "max_videos", "n_videos", "gt_video"]
    assert inspect.signature(models.SMIN.new_survivors).parameters["tau"].default == 0.1


# ---------------------------------------------------------------- host: the fold's restatement
def empty_state(Q, M):
    return torch.zeros(Q, M), torch.zeros(Q, M), torch.full((Q, M), -1, dtype=torch.int32)


def corpus_cut(A, S, C, M):
    """each query's kept videos of the scores / cells (Q, seen) concatenated so far, by the two existing restatements"""
    Q, seen = S.shape
    vr = A.rank_videos_torch(S.reshape(-1), C.reshape(-1), torch.arange(seen, dtype=torch.int32).repeat(Q),
                             torch.arange(Q + 1, dtype=torch.int32) * seen, n=1)
    return A.prefilter_select_torch(vr["pair_rank"].reshape(Q, seen), M)[0].tolist()


def slot_rule(old_video, kept, seen, M, Vs):
    """the slot rule by hand, for one query: ``(slot_video, copy_src)`` after a shard of Vs videos whose first is ``seen``, given the
    videos ``kept`` of everything seen"""
    n_old, n_new = min(M, seen), min(M, seen + Vs)
    video, copy_src = list(old_video), [-1] * M
    free = []
    for slot in range(n_new):                                                        # evicted and empty slots, ascending
        if slot >= n_old or video[slot] not in kept:
            free.append(slot)
    newcomers = [v for v in sorted(kept) if v >= seen]                               # admitted shard videos, ascending local index
    assert len(free) == len(newcomers)
    for slot, v in zip(free, newcomers):
        video[slot], copy_src[slot] = v, v - seen
    return video, copy_src


def fold_sequence(A, M, shards):
    """prefilter_fold_torch over ``shards`` = [(score (Q, Vs), cells (Q, Vs)), ...], checked after every shard; returns the copy_src's"""
    Q = shards[0][0].shape[0]
    ss, sc, sv = empty_state(Q, M)
    seen, S, C, out = 0, [], [], []
    for score, cells in shards:
        Vs = score.shape[1]
        before = (ss.clone(), sc.clone(), sv.clone())
        ns, nc, nv, cp = A.prefilter_fold_torch(ss, sc, sv, score, cells, seen)
        assert all(torch.equal(a, b) for a, b in zip(before, (ss, sc, sv))), "the restatement is out of place"
        assert ns.dtype == torch.float32 and nv.dtype == torch.int32 and cp.dtype == torch.int32 and tuple(cp.shape) == (Q, M)
        S.append(score)
        C.append(cells)
        allS, allC = torch.cat(S, 1), torch.cat(C, 1)
        kept = corpus_cut(A, allS, allC, M)
        n_new = min(M, seen + Vs)
        for q in range(Q):
            assert sorted(nv[q, :n_new].tolist()) == kept[q], (M, seen, q)                       # the set is the corpus-wide cut
            want_v, want_c = slot_rule(sv[q].tolist(), set(kept[q]), seen, M, Vs)
            assert nv[q].tolist() == want_v and cp[q].tolist() == want_c, (M, seen, q)            # the placement is the slot rule's
            assert (nv[q, :n_new] >= 0).all() and (nv[q, n_new:] == -1).all()                     # the invariant
            assert ns[q, n_new:].eq(0).all() and nc[q, n_new:].eq(0).all()
            g = nv[q, :n_new].long()                                                              # a slot holds its video's own bits
            assert torch.equal(bits(ns[q, :n_new]), bits(allS[q, g])) and torch.equal(bits(nc[q, :n_new]), bits(allC[q, g]))
        ss, sc, sv, seen = ns, nc, nv, seen + Vs
        out.append(cp)
    return out


def tied_shards(split, seed, Q=3):
    """scores drawn from three values (ties within a shard and between an incumbent and a newcomer); query 1 has no candidate at all,
    query 2 two candidates in all (fewer than M = 3, 5), query 0 candidates at random"""
    g = torch.Generator().manual_seed(seed)
    total = sum(split)
    score = torch.randint(0, 3, (Q, total), generator=g).float() / 2 - 0.5                        # -0.5, 0.0, 0.5
    cells = (torch.rand(Q, total, generator=g) < 0.7).float() * 3
    cells[1] = 0
    cells[2] = 0
    cells[2, torch.randperm(total, generator=g)[:2]] = 6
    e = np.concatenate([[0], np.cumsum(split)])
    return [(score[:, a:b].contiguous(), cells[:, a:b].contiguous()) for a, b in zip(e[:-1], e[1:])]


@pytest.mark.parametrize("split", [(1, 1, 1, 1), (2, 5, 1), (8,)])
@pytest.mark.parametrize("M", [1, 3, 5])
def test_fold_restatement_is_the_corpus_wide_cut(M, split):
    """(1, 1, 1, 1) with M = 5: fewer videos than M in all"""
    A = V()
    for seed in range(6):
        fold_sequence(A, M, tied_shards(split, 10 * M + seed))


def test_fold_restatement_on_named_events():
    A = V()
    one = lambda xs, cells=4.0: (torch.tensor([xs], dtype=torch.float32), torch.full((1, len(xs)), cells))
    # a shard that admits nothing (lower scores; an equal score loses to the lower video), then one that evicts every incumbent
    cps = fold_sequence(A, 3, [one([1.0, 1.0, 1.0]), one([0.5, 1.0]), one([2.0, 2.0, 2.0, 2.0])])
    assert cps[0].tolist() == [[0, 1, 2]] and cps[1].tolist() == [[-1, -1, -1]] and cps[2].tolist() == [[0, 1, 2]]
    # an incumbent in the middle stays where it is; -0 ties with +0 and the lower video wins
    cps = fold_sequence(A, 3, [one([0.0, 3.0, -0.0]), one([0.0, 1.0])])
    assert cps[1].tolist() == [[-1, -1, 1]]
    # non-candidates fill by ascending video and leave for any candidate, however low its score
    cps = fold_sequence(A, 2, [one([9.0, 9.0], cells=0.0), one([-5.0]), one([7.0], cells=0.0), one([-6.0, -7.0])])
    assert [c.tolist() for c in cps] == [[[0, 1]], [[-1, 0]], [[-1, -1]], [[0, -1]]]


def test_gt_rank_restatement_against_a_loop():
    A = V()
    g = torch.Generator().manual_seed(5)
    Q, Vn = 6, 9
    score = torch.randint(0, 3, (Q, Vn), generator=g).float() / 2
    score[0, 0] = -0.0
    cand = torch.rand(Vn, generator=g) < 0.7
    cand[4] = False
    gt = torch.tensor([0, 4, 8, -1, Vn, 3])
    want = []
    for q in range(Q):
        v = int(gt[q])
        if not (0 <= v < Vn) or not cand[v]:
            want.append(-1)
            continue
        want.append(sum(1 for u in range(Vn) if cand[u] and (score[q, u] > score[q, v] or (score[q, u] == score[q, v] and u < v))))
    got = A.prefilter_gt_rank_torch(score, cand, gt)
    assert got.dtype == torch.int32 and got.tolist() == want and want[1] == -1 and want[3] == -1 and want[4] == -1
    assert A.prefilter_gt_rank_torch(score, cand).tolist() == [-1] * Q
    # it is rank_videos_torch's gt_rank over the (Q, V) pairs
    vr = A.rank_videos_torch(score.reshape(-1), cand.float().repeat(Q), torch.arange(Vn, dtype=torch.int32).repeat(Q),
                             torch.arange(Q + 1, dtype=torch.int32) * Vn, n=1, gt_video=gt)
    assert vr["gt_rank"].tolist() == want
    assert A.prefilter_gt_rank_torch(score.double(), cand.to(torch.uint8), gt).tolist() == want


def test_refusals_on_the_host():
    import models
    A = V()
    T, L, C, D = TINY_SHAPE[:4]
    ss, sc, sv = empty_state(2, 3)
    score, cells = torch.zeros(2, 4), torch.ones(2, 4)
    with pytest.raises(A._lib.SminHipError):
        A.prefilter_fold(ss, sc, sv, score, cells, 0)
    with pytest.raises(A._lib.SminHipError):
        A.prefilter_gt_rank(score, torch.ones(4, dtype=torch.bool))
    shard = (torch.zeros(4, T, D), torch.ones(4, T, 1, dtype=torch.uint8), torch.ones(4, L, dtype=torch.bool), torch.ones(4, L, L, dtype=torch.bool))
    out = tuple(torch.zeros((6,) + tuple(t.shape[1:]), dtype=t.dtype) for t in shard)
    with pytest.raises(A._lib.SminHipError):
        A.survivors_admit(torch.zeros(2, 3, dtype=torch.int32), shard, out)
    for bad_seen in (-1, 1.0, None, 2 ** 31 - 4):
        with pytest.raises(ValueError, match="seen"):
            A.prefilter_fold_torch(ss, sc, sv, score, cells, bad_seen)
    with pytest.raises(ValueError, match="M"):
        A.prefilter_fold_torch(*empty_state(2, A.moments.PREFILTER_FOLD_MAX_M + 1), score, cells, 0)
    with pytest.raises(ValueError):
        A.prefilter_fold_torch(ss, sc, sv, score[:1], cells[:1], 0)                               # another Q
    with pytest.raises(ValueError):
        A.prefilter_fold_torch(ss, sc, sv, score, cells[:, :3], 0)
    with pytest.raises(ValueError):
        A.survivors_admit_torch(torch.zeros(2, 3, dtype=torch.int32), shard, out[:3])
    with pytest.raises(ValueError):
        A.survivors_admit_torch(torch.zeros(2, 3, dtype=torch.int32), shard, (out[0][:5],) + out[1:])          # 5 rows for 6 slots
    with pytest.raises(ValueError):
        A.prefilter_gt_rank_torch(score, torch.ones(3, dtype=torch.bool))
    with pytest.raises(ValueError, match="gt_video"):
        A.prefilter_gt_rank_torch(score, torch.ones(4, dtype=torch.bool), torch.zeros(3, dtype=torch.int64))
    m = models.SMIN(*TINY_SHAPE)
    fs = torch.zeros(3, D)
    vb = A.VideoBank(shard[0], torch.zeros(4, T, 24), *shard[1:], (36,) * 4)
    qb = A.QueryBank(torch.zeros(3, 5, D), fs, torch.zeros(3, 5, 300), torch.ones(3, 5, dtype=torch.uint8))
    for bad_m in (0, -3, 1.5, A.moments.PREFILTER_FOLD_MAX_M + 1):
        with pytest.raises(ValueError, match="M"):
            m.new_survivors(qb, bad_m)
    with pytest.raises(ValueError, match="tau"):
        m.new_survivors(qb, 2, tau=0.0)
    with pytest.raises(A._lib.SminHipError):
        m.new_survivors(qb, 2)                                                                    # CPU banks
    sb = A.SurvivorBank(3, 2, 0.1, "cpu", torch.empty(0, T, 24))
    assert len(sb) == 6 and sb.seen == 0 and sb.fv is None and sb.video_features is None and tuple(sb.plan_features.shape) == (0, T, 24)
    assert sb.slot_video.eq(-1).all() and sb.cell_count is None
    wb = A.WindowBank(shard[0], None, *shard[1:], (36,) * 4, [0] * 4, [T] * 4, [0, 1, 2, 3, 4], [T] * 4, None, None, None, T, T // 2)
    with pytest.raises(ValueError, match="VideoBank of whole videos"):
        m.fold_survivors(sb, wb, qb)
    with pytest.raises(ValueError, match="Q = 3"):
        m.fold_survivors(sb, vb, A.QueryBank(torch.zeros(2, 5, D), fs[:2], torch.zeros(2, 5, 300), torch.ones(2, 5, dtype=torch.uint8)))
    with pytest.raises(A._lib.SminHipError):
        m.fold_survivors(sb, vb, qb)                                                              # CPU banks
    with pytest.raises(ValueError, match="no shard"):
        m.search_survivors(sb, qb)
    with pytest.raises(ValueError, match="at least one shard"):
        A.search_shards_prefiltered(_FakeSurvivorModel(), [], qb, prefilter=2)


class _FakeSurvivorModel:
    """what search_shards_prefiltered asks of a model before the first shard"""

    def new_survivors(self, queries, M, tau):
        return object()


# ---------------------------------------------------------------- GPU
def banded_like(t, dev):
    """``t`` (a host tensor) on the device between two bands of a sentinel of its dtype: ``(the whole buffer, the view)``"""
    n = t.numel()
    sentinel = SENTINEL if t.dtype.is_floating_point else 93
    buf = torch.full((n + 2 * BAND,), sentinel, dtype=t.dtype, device=dev)
    buf[BAND:BAND + n] = t.reshape(-1).to(dev)
    return buf, buf[BAND:BAND + n].view(t.shape)


def bands_ok(buf):
    sentinel = SENTINEL if buf.dtype.is_floating_point else 93
    return bool(buf[:BAND].eq(sentinel).all()) and bool(buf[-BAND:].eq(sentinel).all())


def kernel_shard(Q, Vs, seed):
    """a shard's scores from five values and per-query cells: query 1 without a candidate, query 2 with two candidates at most"""
    g = torch.Generator().manual_seed(seed)
    score = torch.randint(0, 5, (Q, Vs), generator=g).float() / 4 - 0.5
    cells = (torch.rand(Q, Vs, generator=g) < 0.8).float() * 3
    cells[1] = 0
    cells[2] = 0
    cells[2, torch.randperm(Vs, generator=g)[:2]] = 6
    return score, cells


def fold_abi(dev, state, score, cells, seen, fill, over=()):
    """smin_prefilter_fold through the C ABI on a copy of ``state`` whose slots behind min(M, seen) are pre-filled with ``fill`` = (float,
    int), between sentinel bands; ``over`` overrides arguments by name.  Returns (rc, state and copy_src after the call, their buffers)"""
    L_ = V()._lib
    Q, M = state[0].shape
    Vs = score.shape[1]
    n_old = min(M, seen)
    pre = [s.clone() for s in state] + [torch.zeros(Q, M, dtype=torch.int32)]
    pre[0][:, n_old:], pre[1][:, n_old:], pre[2][:, n_old:], pre[3][:] = fill[0], fill[0], fill[1], fill[1]
    bufs, views = zip(*[banded_like(t, dev) for t in pre])
    a = dict(score=score.to(dev), cells=cells.to(dev), Q=Q, Vs=Vs, M=M, seen=seen, n_old=n_old, slot_score=views[0], slot_cells=views[1],
             slot_video=views[2], copy_src=views[3])
    a.update(over)
    p = lambda key: L_.ptr(a[key])
    rc = L_.load().smin_prefilter_fold(L_.stream(), p("score"), p("cells"), a["Q"], a["Vs"], a["M"], a["seen"], a["n_old"], p("slot_score"),
                                       p("slot_cells"), p("slot_video"), p("copy_src"))
    torch.cuda.synchronize()
    return rc, views, bufs, pre


def history(A, Q, M, V0, seed):
    """the state after one shard of V0 videos (V0 = 0: the empty state), by the restatement"""
    state = empty_state(Q, M)
    if V0:
        state = A.prefilter_fold_torch(*state, *kernel_shard(Q, V0, seed), 0)[:3]
    return state


@pytest.mark.gpu
@pytest.mark.parametrize("Vs", [1, 5, 300, 700])
@pytest.mark.parametrize("M", [1, 5, 300])
def test_prefilter_fold_kernel(dev, M, Vs):
    """300 and 700 lie past one and two 256-wide tiles of the scans; M = 300 with Vs = 1 and the reverse both occur; the history of 400
    videos fills all 300 slots (more than one 256-wide batch of incumbents), the one of 3 leaves empty slots to fill"""
    A = V()
    Q = 4
    for V0 in (0, 3, 400):
        state = history(A, Q, M, V0, 1000 + M + V0)
        score, cells = kernel_shard(Q, Vs, 7 * M + Vs + V0)
        want = A.prefilter_fold_torch(*state, score, cells, V0)
        rc, got, bufs, _ = fold_abi(dev, state, score, cells, V0, (float("nan"), -7))
        assert rc == 0
        for name, g, w, b in zip(("slot_score", "slot_cells", "slot_video", "copy_src"), got, want, bufs):
            assert torch.equal(bits(g), bits(w)), (name, M, Vs, V0)
            assert bands_ok(b), (name, M, Vs, V0)
        rc, again, _, _ = fold_abi(dev, state, score, cells, V0, (-7.0, 123456))                 # a second run, over another fill
        assert rc == 0 and all(torch.equal(bits(g), bits(h)) for g, h in zip(got, again)), (M, Vs, V0)
        n_new = min(M, V0 + Vs)
        assert (got[2][:, :n_new] >= 0).all() and (got[2][:, n_new:] == -1).all()
        assert got[2][1, :n_new].sort().values.tolist() == list(range(n_new))                    # no candidate: the lowest videos
    if (M, Vs) == (5, 300):
        # the Python entry point updates the state in place and writes into the copy_src it is given
        state = [s.to(dev) for s in history(A, Q, M, 3, 1)]
        score, cells = kernel_shard(Q, Vs, 2)
        want = A.prefilter_fold_torch(*[s.cpu() for s in state], score, cells, 3)
        cp = torch.full((Q, M), -9, dtype=torch.int32, device=dev)
        assert A.prefilter_fold(*state, score.to(dev), cells.to(dev), 3, copy_src=cp) is cp
        assert all(torch.equal(bits(g), bits(w)) for g, w in zip(state + [cp], want))
        state2 = [s.to(dev) for s in history(A, Q, M, 3, 1)]
        assert torch.equal(A.prefilter_fold(*state2, score.to(dev), cells.to(dev), 3).cpu(), want[3])
        with pytest.raises(ValueError, match="in place"):
            A.prefilter_fold(state[0].double(), state[1], state[2], score.to(dev), cells.to(dev), 3)


@pytest.mark.gpu
@pytest.mark.parametrize("M", [1, 5])
def test_prefilter_fold_signed_zeros(dev, M):
    """What kernel_shard leaves out: -0 against +0 (equal: the lower video goes first), in the incumbents and in the shard, among scores
    of both signs; Q = 3, the shard past one 256-wide tile."""
    A = V()
    Q, V0, Vs = 3, 7, 300
    g = torch.Generator().manual_seed(M)
    values = torch.tensor([0.0, -0.0, 0.25, -0.25])
    draw = lambda n: (values[torch.randint(0, 4, (Q, n), generator=g)], (torch.rand(Q, n, generator=g) < 0.8).float() * 3)
    state = A.prefilter_fold_torch(*empty_state(Q, M), *draw(V0), 0)[:3]
    score, cells = draw(Vs)
    assert score.view(torch.int32).eq(-2 ** 31).any() and score.view(torch.int32).eq(0).any()
    want = A.prefilter_fold_torch(*state, score, cells, V0)
    rc, got, bufs, _ = fold_abi(dev, state, score, cells, V0, (float("nan"), -7))
    assert rc == 0
    for name, x, w, b in zip(("slot_score", "slot_cells", "slot_video", "copy_src"), got, want, bufs):
        assert torch.equal(bits(x), bits(w)) and bands_ok(b), (name, M)


@pytest.mark.gpu
def test_prefilter_fold_rejections(dev):
    A = V()
    Q, M, Vs, seen = 3, 5, 7, 9
    state = history(A, Q, M, seen, 3)
    score, cells = kernel_shard(Q, Vs, 4)
    limit = A.moments.PREFILTER_FOLD_MAX_M
    bad = [dict(M=limit + 1, n_old=9), dict(M=0), dict(Q=0), dict(Vs=0), dict(seen=-1), dict(n_old=4), dict(n_old=6), dict(n_old=9),
           dict(seen=2 ** 31 - 1 - Vs + 1), dict(seen=2 ** 31 - 1)]
    bad += [{name: None} for name in ("score", "cells", "slot_score", "slot_cells", "slot_video", "copy_src")]
    for kw in bad:
        rc, got, bufs, pre = fold_abi(dev, state, score, cells, seen, (float("nan"), -7), kw)
        assert rc != 0, kw
        assert all(bands_ok(b) for b in bufs), kw
        assert all(torch.equal(bits(g), bits(p)) for g, p in zip(got, pre)), kw                  # the outputs untouched
    rc, got, bufs, _ = fold_abi(dev, state, score, cells, 2 ** 31 - 1 - Vs, (float("nan"), -7), dict(n_old=M))   # the last ids an int32 holds
    assert rc == 0 and all(bands_ok(b) for b in bufs)
    # M at the limit
    big = history(A, 3, limit, 5, 5)
    s2, c2 = kernel_shard(3, 3, 6)
    want = A.prefilter_fold_torch(*big, s2, c2, 5)
    rc, got, bufs, _ = fold_abi(dev, big, s2, c2, 5, (float("nan"), -7))
    assert rc == 0 and all(torch.equal(bits(g), bits(w)) for g, w in zip(got, want)) and all(bands_ok(b) for b in bufs)


@pytest.mark.gpu
@pytest.mark.parametrize("T,L,D", [(20, 5, 20), (16, 8, 32), (72, 5, 128)])
def test_survivors_admit_kernel(dev, T, L, D):
    """(20, 5, 20): L L = 25 bytes per moment-mask row and T = 20, L = 5 bytes per video- and length-mask row, so the byte copies are
    unaligned; (72, 5, 128): T D / 4 = 2304 float4, past the 2048 of one workgroup"""
    A = V()
    L_ = A._lib
    g = torch.Generator().manual_seed(T + D)
    Vs, Q, M = 6, 3, 4
    R = Q * M
    shard = (torch.randn(Vs, T, D, generator=g), torch.randint(0, 256, (Vs, T, 1), generator=g).to(torch.uint8),
             torch.randint(0, 256, (Vs, L), generator=g).to(torch.uint8), torch.randint(0, 256, (Vs, L, L), generator=g).to(torch.uint8))
    pre = (torch.randn(R, T, D, generator=g), torch.randint(0, 256, (R, T, 1), generator=g).to(torch.uint8),
           torch.randint(0, 256, (R, L), generator=g).to(torch.uint8), torch.randint(0, 256, (R, L, L), generator=g).to(torch.uint8))
    copy_src = torch.tensor([[0, -1, 5, 2], [-1, -1, -1, -1], [3, 3, -1, 0]], dtype=torch.int32)
    want = A.survivors_admit_torch(copy_src, shard, pre)
    flat = copy_src.reshape(-1).tolist()
    for w, s, p in zip(want, shard, pre):
        assert w.dtype == p.dtype and w.shape == p.shape
        for r, src in enumerate(flat):                                                # the restatement against the rule itself
            assert torch.equal(w[r], s[src] if src >= 0 else p[r]), r
    bufs, views = zip(*[banded_like(t, dev) for t in pre])
    shard_d, cp_d = [t.to(dev) for t in shard], copy_src.to(dev)
    rc = L_.load().smin_survivors_admit(L_.stream(), L_.ptr(cp_d), *[L_.ptr(t) for t in shard_d], R, Vs, T, L, D, *[L_.ptr(t) for t in views])
    torch.cuda.synchronize()
    assert rc == 0
    for name, got, w, b in zip(("fv", "video_mask", "length_mask", "moment_mask"), views, want, bufs):
        assert torch.equal(bits(got), bits(w)), name                                  # admitted rows: the source bits; the others: kept
        assert bands_ok(b), name
    # the Python entry point, bool masks included, in place
    bool_shard = [shard_d[0]] + [t != 0 for t in shard_d[1:]]
    out = [pre[0].to(dev)] + [(t != 0).to(dev) for t in pre[1:]]
    want_b = A.survivors_admit_torch(copy_src, [shard[0]] + [t != 0 for t in shard[1:]], [pre[0]] + [t != 0 for t in pre[1:]])
    A.survivors_admit(cp_d, bool_shard, out)
    assert all(torch.equal(bits(g), bits(w)) for g, w in zip(out, want_b))
    # rejections: nothing is written
    bufs, views = zip(*[banded_like(t, dev) for t in pre])
    args = [L_.ptr(cp_d)] + [L_.ptr(t) for t in shard_d] + [R, Vs, T, L, D] + [L_.ptr(t) for t in views]
    bad = [(0, None), (1, None), (4, None), (10, None), (13, None), (5, 0), (6, 0), (7, 0), (8, 0), (9, 0), (9, D + 2), (10, L_.ptr(views[0].reshape(-1)[1:]))]
    for i, value in bad:
        rc = L_.load().smin_survivors_admit(L_.stream(), *[value if j == i else x for j, x in enumerate(args)])
        assert rc != 0, (i, value)
    torch.cuda.synchronize()
    assert all(torch.equal(bits(g), bits(p)) for g, p in zip(views, pre)) and all(bands_ok(b) for b in bufs)


@pytest.mark.gpu
@pytest.mark.parametrize("Vn", [1, 5, 2500])
def test_prefilter_gt_rank_kernel(dev, Vn):
    A = V()
    L_ = A._lib
    Q = 7
    g = torch.Generator().manual_seed(Vn)
    score = torch.randint(0, 6, (Q, Vn), generator=g).float() / 4 - 0.5               # six values: ties everywhere; -0.0 beside 0.0
    score[0, 0] = -0.0
    cand = torch.rand(Vn, generator=g) < 0.8
    cand[Vn // 2] = Vn == 1
    gt = torch.tensor([0, Vn // 2, Vn - 1, -1, Vn, int(torch.randint(Vn, (1,), generator=g)), 2 ** 31 - 1], dtype=torch.int32)
    want = A.prefilter_gt_rank_torch(score, cand, gt)
    assert want[3] == -1 and want[4] == -1 and want[6] == -1 and (Vn == 1 or want[1] == -1)
    vr = A.rank_videos_torch(score.reshape(-1), cand.float().repeat(Q), torch.arange(Vn, dtype=torch.int32).repeat(Q),
                             torch.arange(Q + 1, dtype=torch.int32) * Vn, n=1, gt_video=gt)
    assert torch.equal(want, vr["gt_rank"])                                           # what prefilter_videos gives on the whole bank
    got = A.prefilter_gt_rank(score.to(dev), cand.to(dev), gt.to(dev))
    assert got.dtype == torch.int32 and torch.equal(got.cpu(), want), Vn
    assert A.prefilter_gt_rank(score.to(dev), cand.to(dev)).tolist() == [-1] * Q
    # through the C ABI between sentinels, twice, and the rejections
    s_d, c_d, g_d = score.to(dev), cand.to(torch.uint8).to(dev), gt.to(dev)
    for fill in (-9, 123456):
        buf = torch.full((Q + 2 * BAND,), fill, dtype=torch.int32, device=dev)
        out = buf[BAND:BAND + Q]
        assert L_.load().smin_prefilter_gt_rank(L_.stream(), L_.ptr(s_d), L_.ptr(c_d), L_.ptr(g_d), Q, Vn, L_.ptr(out)) == 0
        torch.cuda.synchronize()
        assert torch.equal(out.cpu(), want) and buf[:BAND].eq(fill).all() and buf[-BAND:].eq(fill).all()
    out = torch.full((Q,), -9, dtype=torch.int32, device=dev)
    for args in ((None, L_.ptr(c_d), L_.ptr(g_d), Q, Vn, L_.ptr(out)), (L_.ptr(s_d), None, L_.ptr(g_d), Q, Vn, L_.ptr(out)),
                 (L_.ptr(s_d), L_.ptr(c_d), L_.ptr(g_d), 0, Vn, L_.ptr(out)), (L_.ptr(s_d), L_.ptr(c_d), L_.ptr(g_d), Q, 0, L_.ptr(out)),
                 (L_.ptr(s_d), L_.ptr(c_d), L_.ptr(g_d), Q, Vn, None)):
        assert L_.load().smin_prefilter_gt_rank(L_.stream(), *args) != 0
    torch.cuda.synchronize()
    assert out.eq(-9).all()


# ---------------------------------------------------------------- GPU: end to end
@pytest.fixture(scope="module")
def world(dev):
    """the tiny model; the ragged corpus of test_pair_training with a video without rows (V = 5, Q = 4) and a corpus of equal videos,
    as device inputs and as whole banks"""
    m, _ = tiny_model(dev)

    def corpus(snips):
        vid, qry, _ = corpus_inputs(snips=snips)
        vid_d, qry_d = {k: v.to(dev) for k, v in vid.items()}, {k: v.to(dev) for k, v in qry.items()}
        vb = m.encode_videos(vid_d["video_features"], vid_d["video_mask"], vid_d["length_mask"], vid_d["moment_mask"])
        return vid_d, qry_d, vb, m.encode_queries(qry_d["query_features"], qry_d["query_mask"])

    vid_d, qry_d, vb, qb = corpus(NO_ROWS)
    evid_d, eqry_d, evb, eqb = corpus((8, 8, 8, 8, 8))
    return dict(m=m, vid_d=vid_d, qry_d=qry_d, vb=vb, qb=qb, evid_d=evid_d, eqry_d=eqry_d, evb=evb, eqb=eqb)


def same_lists(got, want, keys, what):
    same(got, want, [k for k in keys if k != "times"], what)
    if "times" in keys:
        assert torch.equal(torch.isnan(got["times"]), torch.isnan(want["times"])), what
        assert torch.equal(bits(torch.nan_to_num(got["times"])), bits(torch.nan_to_num(want["times"]))), what


@pytest.mark.gpu
@pytest.mark.parametrize("split", SPLITS)
@pytest.mark.parametrize("M", [1, 2, 5])
def test_sharded_pruned_search_is_the_one_bank_search(dev, world, M, split):
    A = V()
    m, vid_d, vb, qb = world["m"], world["vid_d"], world["vb"], world["qb"]
    Q, Vn = len(qb), len(vb)
    assert vb.cell_counts == (36, 1, 0, 36, 6) and sum(split) == Vn                   # video 2 has no rows
    gt = [g % Vn for g in GT_VIDEO]
    duration = torch.as_tensor(DURATION, dtype=torch.float32, device=dev)
    for kw in (dict(), dict(gt_video=gt), dict(video_weight=7.5, max_videos=2, gt_video=gt), dict(max_batch=3),
               dict(max_batch=3, video_weight=7.5, max_videos=2)):
        base = dict(k=5, k_video=3, **kw)
        assert "max_batch" not in kw or kw["max_batch"] < Q * min(M, Vn)
        want = m.search(vb, qb, prefilter=M, duration=duration, **base)
        got, d = A.search_shards_prefiltered(m, video_shards(vid_d, split, vb.cell_counts), qb, prefilter=M, **base)
        assert d.tolist() == DURATION.tolist() and set(got) == set(want) - {"times"}
        got["times"] = A.moments.search_times(got["video"], got["idx"], duration, m.L)
        keys = SEARCH_KEYS + PREFILTER_KEYS + ("times",) + (VIDEO_KEYS if "video_weight" in kw else ())
        same_lists(got, want, keys, (M, split, kw))
        assert "gt_video" in kw or got["prefilter_gt_rank"].tolist() == [-1] * Q
    # the methods themselves: duration handed to search_survivors, the survivors' bookkeeping
    sb = m.new_survivors(qb, M)
    banks = [m.encode_videos(s["video_features"], s["video_mask"], s["length_mask"], s["moment_mask"]) for s in video_shards(vid_d, split, vb.cell_counts)]
    for bank in banks:
        assert m.fold_survivors(sb, bank, qb) is sb
    Ms = min(M, Vn)
    assert sb.seen == Vn and len(sb) == Q * M and tuple(sb.fv.shape) == (Q * M,) + tuple(vb.fv.shape[1:]) and sb.cell_count is None
    assert tuple(sb.score.shape) == (Q, Vn) and sb.candidate.tolist() == [True, True, False, True, True]
    for q in range(Q):                                                                # each filled row holds its video's bits
        for slot in range(Ms):
            v = int(sb.slot_video[q, slot])
            for mine, theirs in ((sb.fv, vb.fv), (sb.video_mask, vb.video_mask), (sb.length_mask, vb.length_mask), (sb.moment_mask, vb.moment_mask)):
                assert torch.equal(bits(mine[q * M + slot]), bits(theirs[v])), (q, slot)
    got = m.search_survivors(sb, qb, k=5, k_video=3, duration=duration, gt_video=gt)
    same_lists(got, m.search(vb, qb, prefilter=M, k=5, k_video=3, duration=duration, gt_video=gt), SEARCH_KEYS + PREFILTER_KEYS + ("times",), "methods")
    assert m.known_cell_count is None
    with pytest.raises(ValueError, match="duration"):
        m.search_survivors(sb, qb, duration=duration[:3])
    off = A.VideoBank(None, vb.video_features, vb.video_mask, vb.length_mask, vb.moment_mask, vb.cell_counts)
    with pytest.raises(ValueError, match="off the one-node path"):
        m.fold_survivors(sb, off, qb)
    with pytest.raises(ValueError, match="VideoBank of whole videos"):
        m.fold_survivors(sb, sb, qb)


@pytest.mark.gpu
def test_sharded_pruned_search_reads_nothing_back(dev, world):
    A = V()
    m, vid_d, vb, qb = world["m"], world["evid_d"], world["evb"], world["eqb"]
    assert vb.cell_counts == (36,) * 5
    kw = dict(prefilter=2, k=5, k_video=3, max_batch=3)
    wkw = dict(kw, video_weight=7.5, max_videos=1, gt_video=[0, 1, 2, 3])
    shards = lambda: video_shards(vid_d, (2, 1, 2), vb.cell_counts)
    first, _ = A.search_shards_prefiltered(m, shards(), qb, **kw)                     # first use outside the checked region
    weighted, _ = A.search_shards_prefiltered(m, shards(), qb, **wkw)
    torch.cuda.synchronize()
    mode = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        second, _ = A.search_shards_prefiltered(m, shards(), qb, **kw)
        second_w, _ = A.search_shards_prefiltered(m, shards(), qb, **wkw)
    finally:
        torch.cuda.set_sync_debug_mode(mode)
    same(second, first, SEARCH_KEYS + PREFILTER_KEYS, "second run")
    same(second_w, weighted, SEARCH_KEYS + PREFILTER_KEYS + VIDEO_KEYS, "second weighted run")
    assert int(A._lib.load_torch().layout_status(dev)[0]) == 0                        # the handed-over counts matched the masks
    same(first, m.search(vb, qb, **kw), SEARCH_KEYS + PREFILTER_KEYS, "equal videos")
    same(weighted, m.search(vb, qb, **wkw), SEARCH_KEYS + PREFILTER_KEYS + VIDEO_KEYS, "equal videos, weighted")


@pytest.mark.gpu
def test_the_loop_reads_once_and_equals_the_one_bank_loop(dev, world, monkeypatch):
    """test_model_corpus_prefiltered_shards against test_model_corpus whose shard search is replaced by the whole-bank pruned list"""
    A = V()
    m, vid_d, qry_d, vb, qb = world["m"], world["evid_d"], world["eqry_d"], world["evb"], world["eqb"]
    gt_video = np.array([2, 0, 3, 1])
    M = 2

    class Counting(A.CorpusMeter):
        reads = 0

        def result(self):
            torch.cuda.set_sync_debug_mode(mode)                                      # everything before this point ran without a host read
            Counting.reads += 1
            return super().result()

    for kw in (dict(k=10, k_video=2), dict(k=10, k_video=2, video_weight=7.5, max_videos=2)):
        video_kw = {k: v for k, v in kw.items() if k in ("video_weight", "max_videos")}
        pruned = lambda model, shards, bank, **skw: (model.search(vb, bank, prefilter=M, gt_video=gt_video, **video_kw, **skw), np.asarray(DURATION, np.float64))
        with monkeypatch.context() as mp:
            mp.setattr(A.training, "search_shards", pruned)
            want = A.test_model_corpus(m, [dict(vid_d, duration=DURATION)], qry_d, gt_video, GT_TIMES, k=10, k_video=2)
        want_v = A.VideoRankMeter(n=(1, M), device=dev)
        want_v.update(m.prefilter_videos(vb, qb, M, gt_video=gt_video)["gt_rank"])
        for split in SPLITS:
            first = A.test_model_corpus_prefiltered_shards(m, video_shards(vid_d, split, vb.cell_counts), qry_d, gt_video, GT_TIMES, prefilter=M, **kw)
            assert first == want, (split, kw)
            got_v = A.VideoRankMeter(n=(1, M), device=dev)
            torch.cuda.synchronize()
            Counting.reads = 0
            mode = torch.cuda.get_sync_debug_mode()
            torch.cuda.set_sync_debug_mode("error")
            try:
                got = A.test_model_corpus_prefiltered_shards(m, video_shards(vid_d, split, vb.cell_counts), qry_d, gt_video, GT_TIMES,
                                                             Counting(n=(1, 5), device=dev), prefilter=M, video_meter=got_v, **kw)
            finally:
                torch.cuda.set_sync_debug_mode(mode)
            print("split", split, got, got_v.result())
            assert Counting.reads == 1 and got == want and got["num_samples"] == 4
            assert torch.equal(got_v.state.cpu(), want_v.state.cpu()) and got_v.result() == want_v.result()
    with pytest.raises(ValueError, match="gt_video must lie"):
        A.test_model_corpus_prefiltered_shards(m, video_shards(vid_d, (5,), vb.cell_counts), qry_d, [0, 1, 2, 5], GT_TIMES, prefilter=M, k=10, k_video=2)
