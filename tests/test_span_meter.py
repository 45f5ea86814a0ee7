"""The span metric on the device (csrc/metrics.hip: smin_span_ious, smin_span_meter_update) against its torch restatement, which
tests/test_window_training.py pins to the definition on the CPU: IoUs bit for bit, counts exactly, the fp64 accumulator bit for bit
over updates of different B and k mixed with ordinary cell updates; and the argument refusals of the C entries and of Python."""
import ctypes

import pytest
import torch

from tests.support.device import dev  # noqa: F401  (the module's device fixture)
from tests.support.device import vml as V
from tests.support.compare import bits64
from tests.support.references import edge_cases, py_span_hits, py_span_ious, random_spans, NAN


def cells(B, L, seed):
    g = torch.Generator().manual_seed(seed)
    lens = torch.randint(1, L + 1, (B,), generator=g)
    lens[0] = L
    lm = torch.arange(L).unsqueeze(0) < lens.unsqueeze(1)
    mm = torch.triu(lm.unsqueeze(2) & lm.unsqueeze(1))
    return (torch.rand(B, L, L, generator=g), torch.rand(B, L, generator=g) * 0.9 + 0.05, torch.rand(B, L, generator=g) * 0.9 + 0.05, mm,
            torch.rand(B, L, L, generator=g) * mm)


@pytest.mark.gpu
@pytest.mark.parametrize("B,k,seed", [(1, 1, 1), (1, 5, 2), (7, 5, 3), (64, 1, 4), (65, 64, 5), (1000, 5, 6), (3000, 64, 7), (4097, 1, 8)])
def test_span_ious_equal_torch_bitwise(dev, B, k, seed):
    api = V()
    span, count, gt = random_spans(B, k, seed)
    want = api.span_ious_torch(span, count, gt)
    got = api.span_ious(span.to(dev), count.to(dev), gt.to(dev))
    assert got.dtype == torch.float32 and tuple(got.shape) == (B, k) and got.is_cuda
    assert torch.equal(got.cpu().view(torch.int32), want.view(torch.int32))
    assert not torch.isnan(got).any() and float(got.max()) <= 1.0
    on_dev = api.span_ious_torch(span.to(dev), count.to(dev), gt.to(dev))        # the restatement runs on any device, same bits
    assert torch.equal(on_dev.cpu().view(torch.int32), want.view(torch.int32))
    n = tuple(x for x in (1, 5, 64) if x <= k)
    m = (0.1, 0.3, 0.5, 0.7, 0.75)
    assert api.compute_span_ious(span.to(dev), count.to(dev), gt.to(dev), n, m) == api.compute_span_ious_torch(span, count, gt, n, m)


@pytest.mark.gpu
def test_edge_cases_on_the_device(dev):
    api = V()
    span, count, gt = edge_cases()
    got = api.span_ious(span.to(dev), count.to(dev), gt.to(dev))
    assert torch.equal(got.cpu().view(torch.int32), api.span_ious_torch(span, count, gt).view(torch.int32))
    n, m = (1, 2, 3, 4), (0.5, 0.75, 0.0, 0.9999)
    hits = api.compute_span_ious(span.to(dev), count.to(dev), gt.to(dev), n, m)
    assert hits == api.compute_span_ious_torch(span, count, gt, n, m)
    assert hits == py_span_hits(py_span_ious(span.numpy(), count.numpy(), gt.numpy()), count.numpy(), n, m)
    # NaN in a FILLED slot leaves through fminf / fmaxf and the uni > 0 test the same way on both sides
    span[2, 0, 1] = NAN
    span[4, 1] = NAN
    got = api.span_ious(span.to(dev), count.to(dev), gt.to(dev))
    assert not torch.isnan(got).any()
    assert torch.equal(got.cpu().view(torch.int32), api.span_ious_torch(span, count, gt).view(torch.int32))
    # counts outside [0, k] are read clamped, by both entries and by the restatement
    wild = torch.tensor([-3, 9, 2, 5, 64, 0, -1], dtype=torch.int32)
    full = span.nan_to_num(1.0)
    w = api.span_ious(full.to(dev), wild.to(dev), gt.to(dev))
    assert torch.equal(w.cpu().view(torch.int32), api.span_ious_torch(full, wild, gt).view(torch.int32))
    assert api.compute_span_ious(full.to(dev), wild.to(dev), gt.to(dev), n, m) == api.compute_span_ious_torch(full, wild.clamp(0, 5), gt, n, m)
    # int64 counts and float64 spans are converted, not refused
    a = api.span_ious(span.double().to(dev), count.long().to(dev), gt.double().to(dev))
    assert torch.equal(a, got)


RULES = [(None, (1, 5), (0.1, 0.3, 0.5, 0.7)), (0.5, (1, 5), (0.1, 0.3, 0.5, 0.7)), (0.45, (1, 3, 5), (0.1, 0.5, 0.9))]


@pytest.mark.gpu
@pytest.mark.parametrize("nms_thresh,n,m", RULES)
def test_update_spans_equals_torch_meter_bitwise(dev, nms_thresh, n, m):
    """The same updates, spans of different B and k mixed with ordinary cell updates, through EpochMeter and EpochMeterTorch."""
    api = V()
    hip, ref = api.EpochMeter(n=n, m=m, nms_thresh=nms_thresh, device=dev), api.EpochMeterTorch(n=n, m=m, nms_thresh=nms_thresh)
    steps = [("span", 1, 5), ("cell", 6, 16), ("span", 2500, 5), ("span", 77, 64), ("cell", 3, 16), ("span", 64, 7), ("span", 129, 5)]
    totals = dict.fromkeys(hip.keys, 0.0)
    for q, (kind, B, k) in enumerate(steps):
        if kind == "span":
            args = random_spans(B, k, seed=50 + q)
            hip.update_spans(*[x.to(dev) for x in args])
            ref.update_spans(*args)
            per = api.compute_span_ious(*[x.to(dev) for x in args], n=n, m=m)
        else:
            args = cells(B, k, seed=50 + q)
            loss = torch.tensor(0.25 * (q + 1))
            hip.update(*[x.to(dev) for x in args], loss=loss.to(dev))
            ref.update(*args, loss=loss)
            per = api.compute_ious(*[x.to(dev) for x in args], n=n, m=m, nms_thresh=nms_thresh)
        for key, v in per.items():
            totals[key] += v
        assert torch.equal(bits64(hip.state), bits64(ref.state)), (q, hip.state.tolist(), ref.state.tolist())
    print("state", hip.state.tolist())
    assert hip.state[0] == sum(B for _, B, _ in steps) and hip.state[2] == 9
    assert hip.state[4:].tolist() == [totals[key] for key in hip.keys]
    assert hip.result() == ref.result()
    hip.update_spans(*[x[:0].to(dev) for x in random_spans(4, 5, 1)])             # B = 0: a no-op
    assert torch.equal(bits64(hip.state), bits64(ref.state))


@pytest.mark.gpu
def test_update_spans_does_not_wait_for_the_device(dev):
    api = V()
    batches = [[x.to(dev) for x in random_spans(B, 5, seed=B)] for B in (5, 900, 3)]
    meter = api.EpochMeter(device=dev)
    meter.update_spans(*batches[0])                                              # first use outside the checked region
    meter.reset()
    torch.cuda.synchronize()
    mode = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        for b in batches:
            meter.update_spans(*b)
            api.span_ious(*b)
    finally:
        torch.cuda.set_sync_debug_mode(mode)
    assert meter.result()["num_samples"] == 908


@pytest.mark.gpu
def test_argument_refusals(dev):
    api = V()
    lib = api._lib.load()
    span, count, gt = (x.to(dev) for x in random_spans(8, 5, 9))
    iou = torch.full((8, 5), -1.0, device=dev)
    acc = torch.zeros(12, dtype=torch.float64, device=dev)
    p = api._lib.ptr
    st = api._lib.stream()
    assert lib.smin_span_meter_ws_bytes(8, 2, 4) >= 8 * 8 * 4 + 8 * 4
    for bad in ((0, 2, 4), (-1, 2, 4), (8, 0, 4), (8, 65, 4), (8, 2, 0), (8, 2, 17)):
        assert lib.smin_span_meter_ws_bytes(*bad) == 0, bad
    for B, k in ((8, 0), (8, 65), (-1, 5)):
        assert lib.smin_span_ious(st, p(span), p(count), p(gt), B, k, p(iou)) < 0, (B, k)
    assert lib.smin_span_ious(st, None, p(count), p(gt), 8, 5, p(iou)) < 0
    assert lib.smin_span_ious(st, None, None, None, 0, 5, None) == 0             # B = 0: a no-op
    nbytes = lib.smin_span_meter_ws_bytes(8, 2, 4)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)

    def update(B=8, k=5, n=(1, 5), m=(0.1, 0.3, 0.5, 0.7), nn=None, nm=None, ws_bytes=nbytes, acc_=acc):
        nl, ml = (ctypes.c_int * max(len(n), 1))(*n), (ctypes.c_float * max(len(m), 1))(*m)
        return lib.smin_span_meter_update(st, p(span), p(count), p(gt), B, k, ctypes.cast(nl, ctypes.c_void_p), len(n) if nn is None else nn,
                                          ctypes.cast(ml, ctypes.c_void_p), len(m) if nm is None else nm, p(acc_), p(ws), ws_bytes)

    for kw in (dict(k=0), dict(k=65), dict(B=-1), dict(n=(0, 5)), dict(n=(1, 6)), dict(nn=0), dict(nn=65), dict(nm=0), dict(nm=17),
               dict(ws_bytes=nbytes - 1), dict(acc_=None)):
        assert update(**kw) < 0, kw
    assert update(B=0) == 0
    torch.cuda.synchronize()
    assert not acc.any() and bool((iou == -1).all())                            # nothing was launched
    assert update() == 0
    assert acc[0].item() == 8
    with pytest.raises(ValueError):
        api.span_ious(span[:, :, :1], count, gt)
    with pytest.raises(ValueError):
        api.span_ious(span, count[:4], gt)
    with pytest.raises(ValueError, match="slots"):
        api.EpochMeter(device=dev).update_spans(span[:, :4], count, gt)
    with pytest.raises(ValueError, match="slots"):
        api.compute_span_ious(span, count, gt, n=(1, 6))
    with pytest.raises(ValueError):
        api.EpochMeter(device=dev).update_spans(span, count, gt[:, :1])
    with pytest.raises(api._lib.SminHipError, match="no CPU fallback"):
        api.EpochMeter(device=dev).update_spans(span.cpu(), count.cpu(), gt.cpu())
    with pytest.raises(api._lib.SminHipError, match="no CPU fallback"):
        api.span_ious(span.cpu(), count, gt)
