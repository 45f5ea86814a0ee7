"""Training and evaluating on windows of long videos: the span metric's torch restatement against a
plain-Python definition in numpy fp32 scalars, window annotations against the per-sample targets of dataset.py:95-155, the window
draw against its rule written out; on the GPU the feeder's window form against its raw form and ``test_model_windows`` against the
metric computed by hand from ``localize_windows``' outputs."""
import math

import numpy as np
import pytest
import torch

from tests import helpers as H
from tests.support.device import dev  # noqa: F401  (the module's device fixture)
from tests.support.device import vml as V
from tests.support.compare import bits64
from tests.support.references import edge_cases, py_span_hits, py_span_ious, random_spans


# ---------------------------------------------------------------- the definition, in numpy fp32 scalars
def py_acc(acc, ious, count, n, m):
    """One update_spans on a float64 accumulator, in the order include/smin_hip.h fixes."""
    B = ious.shape[0]
    acc[0] += np.float64(B)
    s = np.float64(0.0)
    for b in range(B):
        s += np.float64(ious[b, 0] if count[b] > 0 else np.float32(0))
    acc[3] += s
    hits = py_span_hits(ious, count, n, m)
    for a, n_ in enumerate(n):
        for c, m_ in enumerate(m):
            acc[4 + a * len(m) + c] += np.float64(hits[f"R@{n_}, IoU={m_}"])


CASES = [("edge", (1, 5), (0.1, 0.3, 0.5, 0.7)), ("edge", (1, 2, 3, 4), (0.5, 0.75, 0.0, 0.9999)), ("rand5", (1, 5), (0.1, 0.3, 0.5, 0.7)),
         ("rand1", (1,), (0.5,)), ("rand64", (1, 5, 10, 64), (0.25, 0.5, 0.75))]


def case_inputs(name):
    if name == "edge":
        return edge_cases()
    return {"rand5": lambda: random_spans(41, 5, 1), "rand1": lambda: random_spans(9, 1, 2), "rand64": lambda: random_spans(23, 64, 3)}[name]()


# ---------------------------------------------------------------- CPU 1: the torch restatement equals the definition
def test_edge_cases_hold_what_they_claim():
    span, count, gt = edge_cases()
    iou = V().span_ious_torch(span, count, gt).numpy()
    assert np.array_equal(iou.view(np.int32), py_span_ious(span, count, gt).view(np.int32))
    assert iou[0, 0] == 1 and iou[0, 1] == 0                                     # equal, disjoint
    assert not iou[1].any() and not iou[0, 2:].any()                             # count = 0; NaN slots -> exactly 0
    assert iou[3, 0] == 0 and iou[3, 1] == 0                                     # uni == 0
    assert iou[4, 0] == np.float32(0.5) and iou[4, 1] == np.float32(0.75) and iou[4, 2] == 1 and 0.75 < iou[4, 3] < 1
    hits = V().compute_span_ious_torch(span[4:5], count[4:5], gt[4:5], (1, 2), (0.5, 0.75))
    assert hits == py_span_hits(iou[4:5], count[4:5].numpy(), (1, 2), (0.5, 0.75))
    assert hits == {"R@1, IoU=0.5": 0.0, "R@1, IoU=0.75": 0.0, "R@2, IoU=0.5": 1.0, "R@2, IoU=0.75": 0.0}      # iou == m is not a hit


@pytest.mark.parametrize("name,n,m", CASES)
def test_span_ious_torch_equals_definition(name, n, m):
    api = V()
    span, count, gt = case_inputs(name)
    want = py_span_ious(span.numpy(), count.numpy(), gt.numpy())
    got = api.span_ious_torch(span, count, gt)
    assert got.dtype == torch.float32 and tuple(got.shape) == tuple(span.shape[:2])
    assert not torch.isnan(got).any()
    assert np.array_equal(got.numpy().view(np.int32), want.view(np.int32))
    assert api.compute_span_ious_torch(span, count, gt, n, m) == py_span_hits(want, count.numpy(), n, m)
    assert list(api.compute_span_ious_torch(span, count, gt, n, m)) == [f"R@{n_}, IoU={m_}" for n_ in n for m_ in m]


def test_torch_meter_update_spans_equals_written_out_sums():
    api = V()
    n, m = (1, 2, 5), (0.3, 0.5, 0.75)
    meter = api.EpochMeterTorch(n=n, m=m, nms_thresh=0.5)                        # the rule plays no part in update_spans
    acc = np.zeros(4 + len(n) * len(m), np.float64)
    for span, count, gt in (edge_cases(), random_spans(41, 5, 1), random_spans(3, 7, 4), random_spans(23, 64, 3)):
        meter.update_spans(span, count, gt)
        py_acc(acc, py_span_ious(span.numpy(), count.numpy(), gt.numpy()), count.numpy(), n, m)
    assert acc[3] > 0 and acc[4:].any()
    assert np.array_equal(meter.state.numpy().view(np.int64), acc.view(np.int64)), (meter.state.tolist(), acc.tolist())
    r = meter.result()
    assert r["num_samples"] == 7 + 41 + 3 + 23 and "loss" not in r and r["mIoU"] == acc[3] / acc[0]
    assert r["R@2, IoU=0.5"] == acc[4 + 1 * 3 + 1] / acc[0]
    # the reference rule's meter takes spans too, with its own n / m; and both kinds of update mix in one state
    ref = api.EpochMeterTorch()
    span, count, gt = random_spans(41, 5, 1)
    ref.update_spans(span, count, gt)
    acc = np.zeros(12, np.float64)
    py_acc(acc, py_span_ious(span.numpy(), count.numpy(), gt.numpy()), count.numpy(), (1, 5), (0.1, 0.3, 0.5, 0.7))
    assert np.array_equal(ref.state.numpy().view(np.int64), acc.view(np.int64))
    L = 8
    g = torch.Generator().manual_seed(5)
    lm = torch.ones(2, L, dtype=torch.bool)
    mm = torch.triu(lm.unsqueeze(2) & lm.unsqueeze(1))
    cells = (torch.rand(2, L, L, generator=g), torch.rand(2, L, generator=g) * 0.9 + 0.05, torch.rand(2, L, generator=g) * 0.9 + 0.05, mm,
             torch.rand(2, L, L, generator=g) * mm)
    only = api.EpochMeterTorch()
    only.update(*cells, loss=torch.tensor(1.5))
    ref.update(*cells, loss=torch.tensor(1.5))
    assert torch.equal(bits64(ref.state), bits64(torch.from_numpy(acc) + only.state))
    assert ref.result()["num_samples"] == 43 and ref.result()["loss"] == 1.5


def test_span_argument_checks():
    api = V()
    span, count, gt = random_spans(4, 5, 6)
    for bad in ((span[:, :, :1], count, gt), (span, count[:3], gt), (span, count, gt[:, :1]), (span.reshape(4, 10), count, gt),
                (torch.zeros(4, 65, 2), count, gt)):
        with pytest.raises(ValueError):
            api.span_ious_torch(*bad)
        with pytest.raises(ValueError):
            api.EpochMeterTorch().update_spans(*bad)
    with pytest.raises(ValueError, match="slots"):
        api.EpochMeterTorch().update_spans(span[:, :4], count.clamp(max=4), gt)  # k = 4 < max(n) = 5
    with pytest.raises(ValueError, match="slots"):
        api.compute_span_ious_torch(span, count, gt, n=(1, 6))
    with pytest.raises(ValueError):
        api.compute_span_ious_torch(span, count, gt, m=tuple(0.01 * q for q in range(17)))
    meter = api.EpochMeter(device="cpu")
    with pytest.raises(api._lib.SminHipError, match="no CPU fallback"):
        meter.update_spans(span, count, gt)
    with pytest.raises(api._lib.SminHipError, match="no CPU fallback"):
        api.span_ious(span, count, gt)
    with pytest.raises(api._lib.SminHipError, match="no CPU fallback"):
        api.compute_span_ious(span, count, gt)
    assert not meter.state.any()
    wild = torch.tensor([-3, 9, 2, 5], dtype=torch.int32)                        # counts outside [0, k] are read clamped
    assert torch.equal(api.span_ious_torch(span.nan_to_num(1.0), wild, gt), api.span_ious_torch(span.nan_to_num(1.0), wild.clamp(0, 5), gt))
    assert not api.span_ious_torch(span, wild, gt)[0].any()
    empty = api.EpochMeterTorch()
    empty.update_spans(span[:0], count[:0], gt[:0])                              # B = 0: a no-op
    assert not empty.state.any()


# ---------------------------------------------------------------- CPU 2: window annotations give the reference's targets in window time
def test_window_annotations_definition():
    api = V()
    times = np.array([[10.0, 20.0], [0.0, 3.0]])
    tw, dw = api.window_annotations(times, [100.0, 6.0], [1000, 50], [64, 0], [128, 50], 64)
    assert tw.dtype == np.float64 and dw.dtype == np.float64
    assert np.array_equal(tw, np.array([[100.0 - 64, 200.0 - 64], [0.0, 25.0]])) and np.array_equal(dw, np.array([128.0, 64.0]))
    tw2, dw2 = api.window_annotations(torch.tensor(times), torch.tensor([100.0, 6.0]), torch.tensor([1000, 50]), np.array([64, 0]), [128, 50], 64)
    assert np.array_equal(tw, tw2) and np.array_equal(dw, dw2)
    with pytest.raises(ValueError):
        api.window_annotations(times, [100.0], [1000, 50], [64, 0], [128, 50], 64)


@pytest.mark.parametrize("T,L", [(64, 16), (256, 64), (128, 32)])
def test_window_targets_equal_oracle_in_window_time(T, L):
    """window_annotations + labels.build_targets against dataset.py's per-sample functions fed (ts_w, te_w, duration_w,
    min(len, T)); tolerances of test_target_kernel_and_feeder.  The ground truth is not clipped: windows that miss the moment have
    sm = 0 everywhere, and no NaN arises."""
    from oracle import labels_oracle as LO
    api = V()
    rng = np.random.default_rng(100 + T)
    flips = cells = missed = 0
    worst = 0.0
    for window in (T, 2 * T, T // 2):
        B = 40
        n = rng.integers(1, 9001, B)
        n[:4] = [window // 3 + 1, window, window + 1, 9000]
        dur = rng.uniform(5.0, 600.0, B)
        ts = rng.uniform(0.0, 0.8, B) * dur
        te = np.minimum(ts + rng.uniform(0.01, 0.3, B) * dur + 0.5, dur)
        times = np.stack([ts, te], 1)
        ws, wl = api.draw_windows(n, times / dur[:, None] * n[:, None], window, max(window // 2, 1), rng, 0.25)
        tw, dw = api.window_annotations(times, dur, n, ws, wl, T)
        nf = np.minimum(wl, T)
        got = api.build_targets(tw, dw, nf, T, L)
        for b in range(B):
            ref = LO.sample_targets(float(tw[b, 0]), float(tw[b, 1]), float(dw[b]), int(nf[b]), T, L)
            over = min(ws[b] + wl[b], tw[b, 1] + ws[b]) - max(ws[b], tw[b, 0] + ws[b]) > 0
            missed += not over
            if tw[b, 1] <= 0 or tw[b, 0] >= dw[b]:
                assert not got["sm"][b].any() and not got["ym"][b].any()          # the window's cells never meet the moment
            for k, v in ref.items():
                a = got[k][b]
                if v.dtype.is_floating_point:
                    assert not torch.isnan(a).any() and not torch.isnan(v).any(), (window, b, k)
                    worst = max(worst, float((a - v.reshape(a.shape)).abs().max()))
                    assert torch.allclose(a, v.reshape(a.shape), rtol=1e-5, atol=1e-6), (window, b, k)
                else:
                    a = a.to(v.dtype).reshape(v.shape)
                    cells += a.numel()
                    if not torch.equal(a, v):
                        src = {"ym": "sm", "ys": "ss", "ye": "se"}.get(k)
                        assert src is not None, (window, b, k)
                        flips += int((a != v).sum())
                        assert ((ref[src][a != v] - 0.5).abs() < 1e-5).all(), (window, b, k)
    print(f"T={T} L={L}: worst abs diff {worst:.3g}, {flips} label flips of {cells}, {missed} of 120 windows miss the moment")
    assert missed > 0 and missed < 120


# ---------------------------------------------------------------- CPU 3: the draw
def py_draw(api, lengths, gt_rows, window, stride, rng, p_overlap):
    out = []
    for b, n in enumerate(lengths):
        starts, lens, _ = (x.tolist() for x in api.window_plan([int(n)], window, stride))
        u = rng.random()
        over = [q for q, (s, w) in enumerate(zip(starts, lens)) if min(s + w, gt_rows[b][1]) - max(s, gt_rows[b][0]) > 0]
        cand = over if (u < p_overlap and over) else list(range(len(starts)))
        q = cand[int(rng.integers(0, len(cand)))]
        out.append((starts[q], lens[q]))
    return out


def draw_inputs(seed, B=200):
    rng = np.random.default_rng(seed)
    n = rng.integers(1, 3000, B)
    a = rng.uniform(0, 1, (B, 2)) * n[:, None]
    gt = np.stack([a.min(1), a.max(1) + 0.25], 1)
    return n, gt


@pytest.mark.parametrize("window,stride", [(64, 32), (100, 7), (256, 256), (50, 80)])
@pytest.mark.parametrize("p", [0.0, 0.3, 1.0])
def test_draw_windows_equals_its_rule(window, stride, p):
    api = V()
    n, gt = draw_inputs(window + stride)
    ws, wl = api.draw_windows(n, gt, window, stride, np.random.default_rng(77), p)
    assert ws.dtype == np.int64 and wl.dtype == np.int32 and ws.shape == wl.shape == n.shape
    want = py_draw(api, n.tolist(), gt.tolist(), window, stride, np.random.default_rng(77), p)
    assert list(zip(ws.tolist(), wl.tolist())) == want
    assert ((ws >= 0) & (ws + wl <= n)).all()
    small = n <= window
    assert small.any() and (ws[small] == 0).all() and (wl[small] == n[small]).all()          # n <= window: the one window (0, n)
    assert (wl[~small] == window).all()
    over = np.minimum(ws + wl, gt[:, 1]) - np.maximum(ws, gt[:, 0]) > 0
    if p == 1.0:
        for b in range(n.shape[0]):                                              # only overlapping windows where one exists
            starts, lens, _ = (x.numpy() for x in api.window_plan([int(n[b])], window, stride))
            exists = (np.minimum(starts + lens, gt[b, 1]) - np.maximum(starts, gt[b, 0]) > 0).any()
            assert over[b] == exists, b
    if p == 0.0:                                                                 # uniform over the plan: the overlap set is never consulted
        rng = np.random.default_rng(77)
        for b in range(n.shape[0]):
            starts, lens, _ = (x.numpy() for x in api.window_plan([int(n[b])], window, stride))
            rng.random()
            q = int(rng.integers(0, starts.shape[0]))
            assert (ws[b], wl[b]) == (starts[q], lens[q]), b
        assert not over.all()


def test_draw_windows_argument_checks():
    api = V()
    with pytest.raises(ValueError, match="no rows"):
        api.draw_windows([5, 0], [[0, 1], [0, 1]], 4, 2, np.random.default_rng(0), 0.5)
    with pytest.raises(ValueError):
        api.draw_windows([5, 3], [[0, 1]], 4, 2, np.random.default_rng(0), 0.5)
    with pytest.raises(TypeError):
        api.draw_windows([5], [[0, 1]], 4, 2, np.random.default_rng(0))           # p_overlap is required


def test_loop_is_exported_and_not_collected():
    api = V()
    assert api.test_model_windows.__test__ is False and api.training.test_model_windows is api.test_model_windows


# ---------------------------------------------------------------- GPU


KEYS = ["video_features", "video_mask", "query_features", "query_mask", "length_mask", "moment_mask", "sm", "ym", "ss", "ys", "se", "ye", "ya"]


def window_batches(api, T, Nq, Din, Vn, sizes, seed, window, stride):
    """Host batches in the window form (whole videos, alternately a list and a packed array) with their drawn windows."""
    rng, g = np.random.default_rng(seed), torch.Generator().manual_seed(seed)
    out = []
    for s, B in enumerate(sizes):
        n = rng.integers(1, 6 * T + 1, B)
        n[0] = max(window // 3, 1)
        ql = rng.integers(1, Nq + 1, B)
        tok = rng.integers(0, Vn - 1, (B, Nq))
        tok[np.arange(Nq)[None, :] >= ql[:, None]] = Vn - 1
        dur = rng.uniform(5.0, 300.0, B)
        ts = rng.uniform(0.0, 0.7, B) * dur
        te = np.minimum(ts + rng.uniform(0.02, 0.3, B) * dur + 0.5, dur)
        times = np.stack([ts, te], 1)
        ws, wl = api.draw_windows(n, times / dur[:, None] * n[:, None], window, stride, rng, 0.7)
        videos = [torch.randn(int(k), Din, generator=g).numpy() for k in n]
        hb = dict(raw_features=videos, tokens=tok, times=times, duration=dur, win_start=ws, win_len=wl)
        if s % 2:
            hb["raw_lengths"], hb["raw_features"] = n, np.concatenate(videos, 0)
        if s == 2:
            hb["spos"] = api.draw_offsets(wl, T, rng)                            # offsets in the window's own range
        out.append((hb, videos, n))
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("window,stride", [(64, 32), (160, 48), (40, 40)])
def test_feeder_window_form_equals_raw_form_of_the_rows(dev, window, stride):
    import models
    api = V()
    T, L, Nq, Din, Vn = 64, 16, 9, 40, 53
    g = torch.Generator().manual_seed(8)
    table = torch.cat([torch.randn(Vn - 2, 300, generator=g), torch.zeros(2, 300)]).to(dev)
    hbs = window_batches(api, T, Nq, Din, Vn, (6, 3, 7, 4), seed=window, window=window, stride=stride)
    raws = []
    for hb, videos, n in hbs:
        tw, dw = api.window_annotations(hb["times"], hb["duration"], n, hb["win_start"], hb["win_len"], T)
        rb = dict(raw_features=[v[int(s):int(s + w)].copy() for v, s, w in zip(videos, hb["win_start"], hb["win_len"])], tokens=hb["tokens"],
                  times=tw, duration=dw)
        if "spos" in hb:
            rb["spos"] = hb["spos"]
        raws.append(rb)
    torch.manual_seed(3)
    model = models.SMIN(T, L, 4, 64, 32, 2, Din, Nq, 32, dev).to(dev)
    status = api._lib.load_torch().layout_status(dev)
    seen = 0
    for pool in ("pick", "mean"):
        want = []
        for fed in api.BatchFeeder(T, L, Nq, dev, embedding=table, pool=pool).feed([dict(r, spos=None) if pool == "mean" else r for r in raws]):
            want.append({k: v.clone() for k, v in fed.items()})
        batches = [dict(h[0], spos=None) if pool == "mean" else h[0] for h in hbs]
        for q, fed in enumerate(api.BatchFeeder(T, L, Nq, dev, embedding=table, pool=pool).feed(batches)):
            assert list(fed.keys()) == KEYS and isinstance(fed, api.FedBatch) and isinstance(fed.cell_count, int)
            for k in KEYS:
                a, b = fed[k], want[q][k]
                assert a.dtype == b.dtype and a.shape == b.shape, (pool, q, k)
                assert torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8)), (pool, q, k)
            assert not torch.isnan(fed["sm"]).any()
            # ... and the targets are the window-time targets: labels.build_targets of window_annotations' values (which the CPU
            # tests compare with dataset.py's per-sample functions), tolerances of test_target_kernel_and_feeder
            hb = hbs[q][0]
            tw, dw = api.window_annotations(hb["times"], hb["duration"], hbs[q][2], hb["win_start"], hb["win_len"], T)
            ref = api.build_targets(tw, dw, np.minimum(hb["win_len"], T), T, L)
            for k, v in ref.items():
                a = fed[k].cpu()
                if v.dtype.is_floating_point:
                    assert torch.allclose(a, v, rtol=1e-5, atol=1e-6), (pool, q, k)
                elif not torch.equal(a.to(v.dtype), v):
                    src = {"ym": "sm", "ys": "ss", "ye": "se"}.get(k)
                    assert src is not None, (pool, q, k)
                    assert ((ref[src][a.to(v.dtype) != v] - 0.5).abs() < 1e-5).all(), (pool, q, k)
            assert fed.cell_count == int(fed["moment_mask"].sum())
            assert fed.cell_count == api.cell_count(np.minimum(hbs[q][0]["win_len"], T), T, L)
            model.known_cell_count = fed.cell_count
            out = model(*H.model_inputs(fed))
            model.known_cell_count = None
            loss = api.loss_fn(out[0], fed["ym"], fed["sm"], fed["moment_mask"], out[1], fed["ys"], fed["ss"], out[2], fed["ye"], fed["se"], out[3],
                               fed["ya"], fed["length_mask"])
            loss.backward()
            assert math.isfinite(float(loss)) and int(status[0]) == 0, (pool, q)
            seen += 1
    assert seen == 8


@pytest.mark.gpu
def test_feeder_window_form_refuses_windows_outside_their_video(dev):
    api = V()
    T, L, Nq, Din, Vn = 64, 16, 9, 40, 53
    table = torch.zeros(Vn, 300, device=dev)
    base = dict(raw_features=[np.zeros((100, Din), np.float32), np.zeros((30, Din), np.float32)], tokens=np.zeros((2, Nq), np.int64),
                times=np.array([[1.0, 2.0], [0.5, 3.0]]), duration=np.array([10.0, 5.0]))
    for ws, wl in (([50, 0], [64, 30]), ([-1, 0], [10, 30]), ([0, 10], [64, 21]), ([0], [64])):
        with pytest.raises(ValueError, match="window|win_start"):
            list(api.BatchFeeder(T, L, Nq, dev, embedding=table).feed([dict(base, win_start=ws, win_len=wl)]))
    with pytest.raises(ValueError, match="spos"):                                # validated against win_len (64 rows: only 0), not the video's 100
        list(api.BatchFeeder(T, L, Nq, dev, embedding=table).feed([dict(base, win_start=[0, 0], win_len=[64, 30], spos=[1, 0])]))
    fed = list(api.BatchFeeder(T, L, Nq, dev, embedding=table).feed([dict(base, win_start=[36, 0], win_len=[64, 30])]))
    assert len(fed) == 1 and fed[0]["video_mask"].sum().item() == 64 + 30


def eval_groups(dev, T, Din, Nq, seed):
    """Two groups: several videos of a few hundred rows (one shorter than T), several queries per video."""
    g = torch.Generator().manual_seed(seed)
    rng = np.random.default_rng(seed)
    groups = []
    for lengths, per_video in (([300, 45, 521], 3), ([410, 257], 4)):
        n = np.array(lengths)
        vi = np.repeat(np.arange(n.shape[0]), per_video)
        B = vi.shape[0]
        ql = rng.integers(2, Nq + 1, B)
        qf = torch.randn(B, Nq, 300, generator=g)
        qm = (torch.arange(Nq).unsqueeze(0) < torch.as_tensor(ql).unsqueeze(1)).to(torch.uint8).unsqueeze(-1)
        qf = qf * qm
        dur = rng.uniform(20.0, 200.0, n.shape[0])[vi]
        ts = rng.uniform(0.0, 0.7, B) * dur
        te = np.minimum(ts + rng.uniform(0.05, 0.3, B) * dur, dur)
        groups.append(dict(raw=torch.randn(int(n.sum()), Din, generator=g).to(dev), lengths=n, query_features=qf.to(dev), query_mask=qm.to(dev),
                           video_index=vi, times=np.stack([ts, te], 1), duration=dur))
    return groups


@pytest.mark.gpu
@pytest.mark.parametrize("forward_only", [False, True])
def test_test_model_windows_equals_metric_by_hand(dev, forward_only):
    import models
    api = V()
    T, L, Nq, Din = 64, 16, 9, 40
    torch.manual_seed(11)
    model = models.SMIN(T, L, 4, 64, 32, 2, Din, Nq, 32, dev).to(dev)
    model.forward_only_scoring = forward_only
    groups = eval_groups(dev, T, Din, Nq, seed=21)
    n_list, m_list = (1, 3, 5), (0.1, 0.3, 0.5, 0.7)
    opts = dict(window=64, stride=32, k=5, nms_thresh=0.5)
    # by hand: localize_windows' outputs copied to the host, the definition of this file's CPU tests
    acc = np.zeros(4 + len(n_list) * len(m_list), np.float64)
    model.eval()
    for gr in groups:
        out = model.localize_windows(gr["raw"], gr["lengths"], gr["query_features"], gr["query_mask"], video_index=gr["video_index"], **opts)
        gt = (gr["times"] / gr["duration"][:, None] * gr["lengths"][gr["video_index"]].astype(np.float64)[:, None]).astype(np.float32)
        span, count = out["span"].cpu().numpy(), out["count"].cpu().numpy()
        assert count.max() > 0
        py_acc(acc, py_span_ious(span, count, gt), count, n_list, m_list)
    want = {f"R@{n_}, IoU={m_}": acc[4 + a * len(m_list) + c] / acc[0] for a, n_ in enumerate(n_list) for c, m_ in enumerate(m_list)}
    want.update(mIoU=acc[3] / acc[0], num_samples=int(acc[0]))
    assert want["num_samples"] == 17 and want["mIoU"] > 0

    class Reading(api.EpochMeter):
        """The loop may read the device here and nowhere else."""
        reads = 0

        def result(self, group=None):
            Reading.reads += 1
            torch.cuda.set_sync_debug_mode("default")
            return super().result(group)

    meter = Reading(n=n_list, m=m_list, nms_thresh=0.5, device=dev)
    torch.cuda.synchronize()
    mode = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        got = api.test_model_windows(model, groups, meter, **opts)
    finally:
        torch.cuda.set_sync_debug_mode(mode)
    print("forward_only", forward_only, got)
    assert Reading.reads == 1
    assert got == want
    assert np.array_equal(meter.state.cpu().numpy().view(np.int64), acc.view(np.int64))
    assert model.known_cell_count is None and not model.training
    assert int(api._lib.load_torch().layout_status(dev)[0]) == 0
    with pytest.raises(ValueError, match="R@5"):                                 # refused before any retrieval
        api.test_model_windows(model, groups, api.EpochMeter(device=dev), **dict(opts, k=3))
    # a default meter (the reference's n / m) is made when none is given
    r = api.test_model_windows(model, groups[:1], **opts)
    assert r["num_samples"] == 9 and r["R@1, IoU=0.1"] == want_first(api, model, groups[0], opts)


def want_first(api, model, gr, opts):
    out = model.localize_windows(gr["raw"], gr["lengths"], gr["query_features"], gr["query_mask"], video_index=gr["video_index"], **opts)
    gt = (gr["times"] / gr["duration"][:, None] * gr["lengths"][gr["video_index"]].astype(np.float64)[:, None]).astype(np.float32)
    span, count = out["span"].cpu().numpy(), out["count"].cpu().numpy()
    return py_span_hits(py_span_ious(span, count, gt), count, (1,), (0.1,))["R@1, IoU=0.1"] / 9
