"""Hard-negative mining on the device: csrc/corpus.hip smin_mine_pairs, moments.mine_pairs / mine_pairs_torch,
PairPlan.from_device, SMIN.pair_scores / SMIN.mine_pairs, forward_pairs and train_epoch_pairs over a device-built plan and
training.train_epoch_mined.

Host: the C ABI surface, mine_pairs_torch against a hand-written sort of (-score, video) and PairPlan's own groupings, the refusals,
a wrapped plan through pair_targets and train_epoch_pairs' argument checks.
GPU: the kernels through the C ABI against mine_pairs_torch (all six arrays, over a sentinel, twice, and the rejections), pair_scores
against score_pairs + top_moments, a mined plan through forward_pairs against the same lists from the host (same bits for the
outputs and every gradient), no host read on full-length videos, and train_epoch_mined."""
import os
import re
from unittest import mock

import numpy as np
import pytest
import torch

from tests.support.device import dev  # noqa: F401  (the module's device fixture)
from tests.support.device import vml as V
from tests.support.compare import bits
from tests.support.corpora import corpus_inputs, expand, loss_of, on, pair_args, tiny_model, FULL, GT_VIDEO, NQ, NV

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENTINEL = -7


def case(Q, Vn, seed):
    """score (Q, V) and gt_video of a case: even rows rounded to halves (many ties), odd rows as drawn; the first query's own video is
    video 0 and the last one's video V - 1.  (3, 5): row 0 all equal -- ties go to the lower video --, row 1 holds -0.0 and +0.0."""
    g = torch.Generator().manual_seed(seed)
    score = torch.randn(Q, Vn, generator=g)
    score[0::2] = torch.round(score[0::2] * 2) / 2
    gt = torch.randint(0, Vn, (Q,), generator=g).tolist()
    gt[0], gt[-1] = 0, Vn - 1 if Q > 1 else 0
    if (Q, Vn) == (3, 5):
        score[0] = 0.25
        score[1] = torch.tensor([-0.0, 0.0, -1.0, 0.0, -0.0])
        gt[1] = 3
    return score, gt


def by_hand(score, gt, N, skip):
    """The six arrays from a Python sort of (-score, video) per query and PairPlan's host groupings of the resulting lists."""
    Q, Vn = score.shape
    rows = score.tolist()
    vi, qi = [], []
    for q in range(Q):
        wrong = sorted((v for v in range(Vn) if v != gt[q]), key=lambda v: (-rows[q][v], v))      # -0.0 == 0.0: a tie, to the lower video
        vi += [gt[q]] + wrong[skip:skip + N]
        qi += [q] * (1 + N)
    plan = V().PairPlan(vi, qi, Vn, Q, "cpu", gt_video=gt)
    assert plan.positive_rows.tolist() == [q * (1 + N) for q in range(Q)] and plan.num_positive == Q
    return [plan.video_index, plan.query_index, plan.v_ptr, plan.v_pairs, plan.q_ptr, plan.q_pairs]


NAMES = ("video_index", "query_index", "v_ptr", "v_pairs", "q_ptr", "q_pairs")


# ---------------------------------------------------------------- host
def test_header_and_table_declare_the_miner():
    text = open(os.path.join(ROOT, "include", "smin_hip.h")).read()
    assert re.search(r"\bint\s+smin_mine_pairs\s*\(", text) and re.search(r"\bsize_t\s+smin_mine_pairs_ws_bytes\s*\(", text)
    lib = V()._lib.load()
    for name in ("smin_mine_pairs", "smin_mine_pairs_ws_bytes"):
        assert name in V()._lib.SIGNATURES, name
        assert hasattr(lib, name)
    assert len(V()._lib.SIGNATURES["smin_mine_pairs"]) == 15
    assert "#define SMIN_HIP_ABI_VERSION 2" in text and lib.smin_abi_version() == 2
    assert lib.smin_mine_pairs_ws_bytes(16, 16, 3) == 16 * 4 and lib.smin_mine_pairs_ws_bytes(2, 300, 8) == 300 * 4
    assert lib.smin_mine_pairs_ws_bytes(0, 16, 3) == 0 and lib.smin_mine_pairs_ws_bytes(4, 1, 1) == 0 and lib.smin_mine_pairs_ws_bytes(4, 4, 0) == 0


@pytest.mark.parametrize("Q,Vn,N,skip", [(1, 2, 1, 0), (3, 5, 2, 0), (3, 5, 2, 2), (4, 9, 8, 0)])
def test_mine_pairs_torch_by_hand(Q, Vn, N, skip):
    score, gt = case(Q, Vn, 100 * Q + Vn)
    assert gt[0] == 0 and (Q == 1 or gt[-1] == Vn - 1)
    got = V().mine_pairs_torch(score, gt, N, skip)
    want = by_hand(score, gt, N, skip)
    assert len(got) == 6
    for name, a, b in zip(NAMES, got, want):
        assert a.dtype == torch.int32 and torch.equal(a, b), (name, a.tolist(), b.tolist())
    if (Q, Vn, skip) == (3, 5, 0):
        assert got[0].tolist()[:3] == [0, 1, 2]                    # all equal: the two lowest wrong videos
        assert got[0].tolist()[3:6] == [3, 0, 1]                   # the zeros of either sign tie above -1: videos 0, 1 (4 is next)
    if (Q, Vn, skip) == (3, 5, 2):
        assert got[0].tolist()[:3] == [0, 3, 4] and got[0].tolist()[3:6] == [3, 4, 2]
    if N == Vn - 1:                                                # every negative is taken: each query pairs with every video
        assert got[2].tolist() == [Q * v for v in range(Vn + 1)]


def test_refusals():
    api = V()
    score, gt = case(3, 5, 1)
    for kw in (dict(gt_video=[0, 5, 1]), dict(gt_video=[0, -1, 1]), dict(gt_video=[0, 1]), dict(gt_video=[0, 1, 2, 3]), dict(negatives=0),
               dict(negatives=-1), dict(negatives=2.0), dict(skip=-1), dict(negatives=3, skip=2), dict(negatives=5), dict(score=score[0]),
               dict(score=score.reshape(3, 5, 1)), dict(score=score[:, :1], gt_video=[0, 0, 0], negatives=1)):
        args = dict(dict(score=score, gt_video=gt, negatives=2, skip=0), **kw)
        with pytest.raises(ValueError):
            api.mine_pairs_torch(**args)
    wide = torch.zeros(2, 80)
    for kw in (dict(negatives=65), dict(negatives=60, skip=5), dict(negatives=1, skip=64)):
        with pytest.raises(ValueError):
            api.mine_pairs_torch(wide, [0, 1], **kw)
    assert len(api.mine_pairs_torch(wide, [0, 1], 60, 4)) == 6     # skip + negatives = 64 is allowed
    with pytest.raises(api._lib.SminHipError, match="no CPU fallback"):
        api.mine_pairs(score, gt, 2)
    m, _ = tiny_model()
    with pytest.raises(TypeError, match="VideoBank"):
        m.mine_pairs(None, None, GT_VIDEO, 2)


def test_wrapped_plan_through_pair_targets_and_group_checks():
    api = V()
    vid, qry, tg = corpus_inputs()
    score, _ = case(NQ, NV, 9)
    arrays = api.mine_pairs_torch(score, GT_VIDEO, 2, 1)
    vi, qi = arrays[0].tolist(), arrays[1].tolist()
    host = api.PairPlan(vi, qi, NV, NQ, "cpu", gt_video=GT_VIDEO)
    plan = api.PairPlan.from_device(*arrays, NV, NQ, positive=host.positive, positive_rows=host.positive_rows, num_positive=host.num_positive)
    assert plan.vi is None and plan.qi is None and plan.P == 12 and plan.fits(NV, NQ, "cpu")
    assert host.positive.tolist() == [int(p % 3 == 0) for p in range(12)] and host.positive_rows.tolist() == [0, 3, 6, 9]
    got, want = api.pair_targets(vid, tg, None, None, None, plan=plan), api.pair_targets(vid, tg, vi, qi, GT_VIDEO)
    assert set(got) == set(want)
    for k in want:
        assert got[k].dtype == want[k].dtype and torch.equal(got[k], want[k]), k
    with pytest.raises(ValueError, match="v_ptr"):
        api.PairPlan.from_device(arrays[0], arrays[1], arrays[2][:-1], *arrays[3:], NV, NQ)
    bare = api.PairPlan.from_device(*arrays, NV, NQ)
    with pytest.raises(ValueError, match="built with gt_video"):
        api.pair_targets(vid, tg, None, None, None, plan=bare)

    class Stub:                                                    # an optimizer / a meter that is never reached past zero_grad
        def zero_grad(self):
            pass

    m, _ = tiny_model()
    group = dict(**vid, **qry, **tg, plan=plan)                    # no video_index / query_index / gt_video
    with pytest.raises(api._lib.SminHipError, match="no CPU fallback"):   # past the argument checks: the CPU tensors are what is refused
        api.train_epoch_pairs(m, Stub(), [group], Stub())
    wrong_size = api.PairPlan.from_device(*arrays, NV, NQ, positive=host.positive, positive_rows=host.positive_rows, num_positive=NQ)
    wrong_size.V = NV + 1
    for bad in (bare, wrong_size, "plan"):
        with pytest.raises(ValueError, match="positive flags"):
            api.train_epoch_pairs(m, Stub(), [dict(group, plan=bad)], Stub())
    # forward_pairs' cell count of a device-built plan: P * c for equal counts, none otherwise (read by the node)
    seen = []

    def stop(*a):                                                  # where forward_pairs picks its route: the count is in place by then
        seen.append(m.known_cell_count)
        raise RuntimeError("stop")

    m._bank_plan = stop
    with mock.patch.object(api.retrieval, "require_hip_tensors", lambda *a, **k: None), mock.patch.object(torch.cuda, "device", lambda d: mock.MagicMock()):
        for counts, want_cells in (([36] * NV, 12 * 36), ([36, 1, 15, 36, 6], None), (None, None)):
            with pytest.raises(RuntimeError, match="stop"):
                m.forward_pairs(*pair_args(vid, qry), None, None, cell_counts=counts, plan=plan)
            assert seen[-1] == want_cells and m.known_cell_count is None


# ---------------------------------------------------------------- GPU
@pytest.mark.gpu
@pytest.mark.parametrize("Q,Vn,N,skip", [(1, 2, 1, 0), (3, 5, 2, 0), (4, 65, 3, 1), (2, 300, 8, 2), (5, 9, 8, 0), (2, 70, 60, 4)])
def test_kernel_against_torch(dev, Q, Vn, N, skip):
    L_ = V()._lib
    lib = L_.load()
    score, gt = case(Q, Vn, 100 * Q + Vn)
    want = V().mine_pairs_torch(score, gt, N, skip)
    P = Q * (1 + N)
    sizes = [P, P, Vn + 1, P, Q + 1, P]
    sc_d, gt_d = score.to(dev), torch.tensor(gt, dtype=torch.int32, device=dev)
    nbytes = lib.smin_mine_pairs_ws_bytes(Q, Vn, N)
    assert nbytes == 4 * Vn
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)

    def run(args=None, dims=(Q, Vn, N, skip), outs=None, ws_=ws, ws_bytes=nbytes):
        args = [sc_d, gt_d] if args is None else args
        outs = [torch.full((n,), SENTINEL, dtype=torch.int32, device=dev) for n in sizes] if outs is None else outs
        rc = lib.smin_mine_pairs(L_.stream(), *[L_.ptr(a) for a in args], *dims, *[L_.ptr(o) for o in outs], L_.ptr(ws_), ws_bytes)
        torch.cuda.synchronize()
        return rc, outs

    rc, got = run()
    assert rc == 0
    for name, a, b in zip(NAMES, got, want):
        assert torch.equal(a.cpu(), b), (name, a.tolist(), b.tolist())
    rc, again = run()
    assert rc == 0
    for a, b in zip(got, again):
        assert torch.equal(a, b)
    # rejected before any launch: the sentinel stays
    bad = [dict(dims=(0, Vn, N, skip)), dict(dims=(Q, 1, N, skip)), dict(dims=(Q, Vn, 0, skip)), dict(dims=(Q, Vn, N, -1)), dict(dims=(Q, Vn, Vn - skip, skip)),
           dict(dims=(Q, Vn, N, 65 - N)), dict(dims=(Q, Vn, 65, 0)), dict(dims=(2 ** 30, Vn, N, skip)), dict(args=[None, gt_d]), dict(args=[sc_d, None]),
           dict(ws_bytes=nbytes - 1), dict(ws_=None)]
    for kw in bad:
        rc, o = run(**kw)
        assert rc != 0, kw
        for t in o:
            assert t.eq(SENTINEL).all(), kw
    for hole in range(6):
        outs = [torch.full((n,), SENTINEL, dtype=torch.int32, device=dev) for n in sizes]
        rc, _ = run(outs=outs[:hole] + [None] + outs[hole + 1:])
        assert rc != 0, hole
        for k, t in enumerate(outs):
            assert k == hole or t.eq(SENTINEL).all(), hole


@pytest.fixture(scope="module")
def world(dev):
    """the tiny model on the device and the V = 5 / Q = 4 inputs, ragged and at full length, on both sides"""
    m, sd = tiny_model(dev)
    w = dict(m=m, sd=sd)
    for tag, snips in (("ragged", (8, 1, 5, 8, 3)), ("full", FULL)):
        vid, qry, tg = corpus_inputs(snips=snips)
        w[tag] = dict(vid=vid, qry=qry, tg=tg, vid_d=on(dev, vid), qry_d=on(dev, qry), tg_d=on(dev, tg),
                      counts=vid["moment_mask"].reshape(NV, -1).sum(1).tolist())
    assert w["ragged"]["counts"] == [36, 1, 15, 36, 6] and w["full"]["counts"] == [36] * NV
    return w


def banks(m, d, counts=None):
    vd = d["vid_d"]
    return (m.encode_videos(vd["video_features"], vd["video_mask"], vd["length_mask"], vd["moment_mask"], cell_counts=counts),
            m.encode_queries(d["qry_d"]["query_features"], d["qry_d"]["query_mask"]))


@pytest.mark.gpu
def test_pair_scores(dev, world):
    m, d = world["m"], world["ragged"]
    assert d["vid"]["length_mask"][1].sum().item() == 1            # a one-snippet video
    videos, queries = banks(m, d)
    got = m.pair_scores(videos, queries)
    assert got.shape == (NQ, NV) and got.dtype == torch.float32 and not got.requires_grad
    qi, vi = np.repeat(np.arange(NQ), NV), np.tile(np.arange(NV), NQ)
    pm, ps, pe, _ = m.score_pairs(videos, queries, vi, qi)
    mm = d["vid_d"]["moment_mask"][torch.as_tensor(vi, device=dev)]
    want = V().top_moments(pm, ps, pe, mm, k=1)["score"][:, 0].reshape(NQ, NV)
    assert torch.equal(bits(got), bits(want))
    assert got.abs().max().item() > 0
    # chunks of 3 pairs (20 = 6 * 3 + 2): the same calls by hand, every row written
    parts = []
    for c0 in range(0, NQ * NV, 3):
        pm, ps, pe, _ = m.score_pairs(videos, queries, vi[c0:c0 + 3], qi[c0:c0 + 3])
        parts.append(V().top_moments(pm, ps, pe, mm[c0:c0 + 3], k=1)["score"][:, 0])
    assert torch.equal(bits(m.pair_scores(videos, queries, max_batch=3)), bits(torch.cat(parts).reshape(NQ, NV)))


def grads(m, out, targets):
    for p in m.parameters():
        p.grad = None
    loss_of(V().loss_fn, out, targets).backward()
    torch.cuda.synchronize()
    return {k: p.grad.detach().clone() for k, p in m.named_parameters()}


@pytest.mark.gpu
@pytest.mark.parametrize("N", [2, 4])
def test_mined_plan_is_the_host_plan(dev, world, N):
    api, m, d = V(), world["m"], world["ragged"]
    videos, queries = banks(m, d)
    plan = m.mine_pairs(videos, queries, GT_VIDEO, N)
    S, P = 1 + N, NQ * (1 + N)
    assert plan.vi is None and plan.P == P and plan.num_positive == NQ and plan.fits(NV, NQ, dev)
    vi, qi = plan.video_index.tolist(), plan.query_index.tolist()  # (read back in the test only)
    assert vi[::S] == GT_VIDEO and qi == [p // S for p in range(P)]
    assert all(len(set(vi[q * S:q * S + S])) == S for q in range(NQ))
    want = api.mine_pairs_torch(m.pair_scores(videos, queries), GT_VIDEO, N)
    host = api.PairPlan(vi, qi, NV, NQ, dev, gt_video=GT_VIDEO)
    for name, w_ in zip(NAMES, want):
        assert torch.equal(getattr(plan, name), w_), name
        assert torch.equal(getattr(plan, name), getattr(host, name)), name
    assert torch.equal(plan.positive, host.positive) and torch.equal(plan.positive_rows, host.positive_rows)
    if N == 4:
        assert sorted(vi[:S]) == list(range(NV))                   # all negatives
    args = pair_args(d["vid_d"], d["qry_d"])
    out_a = m.forward_pairs(*args, None, None, plan=plan)
    tg_a = api.pair_targets(d["vid_d"], d["tg_d"], None, None, None, plan=plan)
    g_a = grads(m, out_a, tg_a)
    out_b = m.forward_pairs(*args, vi, qi)
    tg_b = api.pair_targets(d["vid_d"], d["tg_d"], vi, qi, GT_VIDEO)
    g_b = grads(m, out_b, tg_b)
    for name, a, b in zip(("pm", "ps", "pe", "pa"), out_a, out_b):
        assert a.shape[0] == P and torch.equal(bits(a), bits(b)), name
    for k in tg_b:
        assert torch.equal(tg_a[k], tg_b[k]), k
    assert len(g_a) == len(g_b) > 0
    for k in g_b:
        assert torch.equal(bits(g_a[k]), bits(g_b[k])), k
    assert int(api._lib.load_torch().layout_status(dev)[0]) == 0


def mined_step(m, d, videos, queries, counts):
    api = V()
    for p in m.parameters():
        p.grad = None
    plan = m.mine_pairs(videos, queries, GT_VIDEO, 2)
    out = m.forward_pairs(*pair_args(d["vid_d"], d["qry_d"]), None, None, cell_counts=counts, plan=plan)
    loss_of(api.loss_fn, out, api.pair_targets(d["vid_d"], d["tg_d"], None, None, None, plan=plan)).backward()
    return {k: p.grad for k, p in m.named_parameters()}


@pytest.mark.gpu
def test_no_host_read_on_full_length_videos(dev, world):
    api, m = V(), world["m"]
    d = world["full"]
    videos, queries = banks(m, d, d["counts"])
    first = {k: g.clone() for k, g in mined_step(m, d, videos, queries, d["counts"]).items()}    # first use outside the checked region
    torch.cuda.synchronize()
    mode = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        second = mined_step(m, d, videos, queries, d["counts"])
    finally:
        torch.cuda.set_sync_debug_mode(mode)
    torch.cuda.synchronize()
    for k, g in second.items():
        assert torch.equal(bits(g), bits(first[k])), k
    assert int(api._lib.load_torch().layout_status(dev)[0]) == 0 and m.known_cell_count is None
    # ragged videos: no count can be handed over, the node reads it
    d = world["ragged"]
    videos, queries = banks(m, d)
    g = mined_step(m, d, videos, queries, d["counts"])
    torch.cuda.synchronize()
    assert m.known_cell_count is None and int(api._lib.load_torch().layout_status(dev)[0]) == 0
    assert all(torch.isfinite(x).all() for x in g.values())


@pytest.mark.gpu
def test_train_epoch_mined(dev, world):
    api, w = V(), world
    m, _ = tiny_model(dev)
    twin, _ = tiny_model(dev)
    N = 2
    groups = []
    for seed in (3, 4):
        vid, qry, tg = corpus_inputs(snips=FULL, seed=seed)
        groups.append(dict(**on(dev, vid), **on(dev, qry), **on(dev, tg), gt_video=GT_VIDEO, cell_counts=[36] * NV))

    class Probe(api.EpochMeter):
        reads = 0

        def result(self, group=None):
            Probe.reads += 1
            torch.cuda.set_sync_debug_mode("default")
            return super().result(group)

    # the first step by hand on the twin: the mined plan read back, its pairs expanded through SMIN.forward
    g0 = groups[0]
    twin.train()
    with torch.no_grad():
        videos = twin.encode_videos(g0["video_features"], g0["video_mask"], g0["length_mask"], g0["moment_mask"])
        queries = twin.encode_queries(g0["query_features"], g0["query_mask"])
        plan = twin.mine_pairs(videos, queries, GT_VIDEO, N)
    vi, qi = plan.video_index.tolist(), plan.query_index.tolist()
    assert len(vi) == NQ * (1 + N) and vi[::1 + N] == GT_VIDEO
    t = api.pair_targets(g0, g0, vi, qi, GT_VIDEO)
    want = loss_of(api.loss_fn, twin(*expand(g0, g0, vi, qi)), t).item()
    opt = api.FusedAdam(m.parameters(), lr=1e-3)
    first, metrics = api.train_epoch_mined(m, opt, groups[:1], N, meter=Probe(device=dev))       # (first use outside the checked region)
    print("train_epoch_mined first loss", first, "by hand on the expanded pairs", want)
    assert abs(first - want) <= 1e-5 * abs(want)
    assert metrics["num_samples"] == NQ
    m.load_state_dict(w["sd"])
    opt = api.FusedAdam(m.parameters(), lr=1e-3)
    Probe.reads = 0
    meter = Probe(device=dev)
    torch.cuda.synchronize()
    mode = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        loss, metrics = api.train_epoch_mined(m, opt, groups, N, meter=meter)
    finally:
        torch.cuda.set_sync_debug_mode(mode)
    assert Probe.reads == 1 and m.known_cell_count is None and m.training
    assert metrics["num_samples"] == 2 * NQ and loss == metrics["loss"] and np.isfinite(loss)
    assert int(api._lib.load_torch().layout_status(dev)[0]) == 0
