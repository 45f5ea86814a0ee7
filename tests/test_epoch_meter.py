"""An epoch without host reads: the device epoch meter (meter.py, csrc/metrics.hip smin_epoch_meter_update), the cell count that
travels with a fed batch (feeder.cell_count, FedBatch) and the reference's three loops over them (training.train_epoch /
eval_epoch / test_model).

``EpochMeterTorch`` is pinned on the CPU to sums written out here in float64 in the order include/smin_hip.h fixes, to the
per-batch ``compute_ious_torch`` counts and to the reference's recorded counts (g6_ious.npz); ``EpochMeter`` (HIP) is then
compared to it bit for bit."""
import os

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from tests import helpers as H
from tests.support.device import dev  # noqa: F401  (the module's device fixture)
from tests.support.device import free_port, vml as V
from tests.support.compare import bits64

REF_N, REF_M = (1, 5), (0.1, 0.3, 0.5, 0.7)
OTHER_N, OTHER_M = (1, 3, 10), (0.5, 0.9)


def ragged(B, L, seed):
    """Scores and IoU targets of B samples of ragged lengths: seeded random values (no ties among the valid cells); sm is 0 outside
    the mask, so the reference rule's choice among masked cells (all score 0) changes no hit."""
    g = torch.Generator().manual_seed(seed)
    lens = torch.randint(1, L + 1, (B,), generator=g)
    lens[0] = L
    lm = torch.arange(L).unsqueeze(0) < lens.unsqueeze(1)
    mm = torch.triu(lm.unsqueeze(2) & lm.unsqueeze(1))
    pm = torch.rand(B, L, L, generator=g)
    ps = torch.rand(B, L, generator=g) * 0.9 + 0.05
    pe = torch.rand(B, L, generator=g) * 0.9 + 0.05
    sm = torch.rand(B, L, L, generator=g) * mm
    return pm, ps, pe, mm, sm


def fake_loss(seed):
    return torch.rand((), generator=torch.Generator().manual_seed(1000 + seed)) * 3 + 0.1


# ---------------------------------------------------------------- CPU: the cell count
@pytest.mark.parametrize("T,L", [(64, 16), (128, 32), (256, 64), (1024, 512)])
def test_cell_count_equals_oracle_mask_sum(T, L):
    from oracle import labels_oracle as LO
    api = V()
    counts = []
    for nf in range(T + 1):
        mask = LO.sample_targets(1.0, 4.0, 10.0, nf, T, L)["moment_mask"]
        counts.append(int(mask.sum()))
        assert api.cell_count(nf, T, L) == counts[-1], (T, L, nf)
    nfs = np.random.default_rng(T).integers(0, T + 1, 9)
    assert api.cell_count(nfs, T, L) == sum(counts[int(x)] for x in nfs)
    assert api.cell_count(torch.as_tensor(nfs), T, L) == api.cell_count(list(nfs), T, L)
    assert isinstance(api.cell_count(nfs, T, L), int)


def test_fed_batch_is_a_dict_with_a_count():
    fb = V().FedBatch((k, i) for i, k in enumerate(("a", "b")))
    fb.cell_count = 7
    assert isinstance(fb, dict) and list(fb.keys()) == ["a", "b"] and dict(fb) == {"a": 0, "b": 1} and fb.cell_count == 7


# ---------------------------------------------------------------- CPU: the torch restatement
def top1_by_hand(api, pm, ps, pe, mm, sm, nms_thresh):
    """Per sample: sm at the first kept cell (numpy fp32 products are correctly rounded; ties -> lower flat index)."""
    out = []
    for b in range(pm.shape[0]):
        s = (pm[b].numpy() * np.sqrt(ps[b].numpy())[:, None]) * np.sqrt(pe[b].numpy())[None, :]
        if nms_thresh is None:
            s = s * mm[b].numpy().astype(np.float32)
        else:
            s = np.where(mm[b].numpy(), s, -np.inf)
        c = int(np.flatnonzero(s.reshape(-1) == s.max())[0])
        out.append(float(sm[b].reshape(-1)[c]) if np.isfinite(s.max()) else 0.0)
    return out


@pytest.mark.parametrize("nms_thresh,n,m", [(None, REF_N, REF_M), (0.5, REF_N, REF_M), (0.4, OTHER_N, OTHER_M), (1.0, OTHER_N, OTHER_M)])
def test_torch_meter_equals_written_out_sums(nms_thresh, n, m):
    api = V()
    meter = api.EpochMeterTorch(n=n, m=m, nms_thresh=nms_thresh)
    assert meter.state.dtype == torch.float64 and meter.state.shape == (4 + len(n) * len(m),) and not meter.state.any()
    acc = np.zeros(4 + len(n) * len(m), dtype=np.float64)
    for q, (B, L) in enumerate([(5, 16), (3, 16), (8, 12)]):
        pm, ps, pe, mm, sm = ragged(B, L, seed=10 * q + 1)
        loss = fake_loss(q) if q != 1 else None                                  # the middle batch carries no loss
        meter.update(pm, ps, pe, mm, sm, loss=loss)
        counts = api.compute_ious_torch(pm, ps, pe, mm, sm, n, m, nms_thresh=nms_thresh)
        s = np.float64(0.0)
        for b in range(B):
            s += np.float64(1.0)
        acc[0] += s
        if loss is not None:
            acc[1] += np.float64(np.float32(loss.item())) * np.float64(B)
            acc[2] += s
        s = np.float64(0.0)
        for v in top1_by_hand(api, pm, ps, pe, mm, sm, nms_thresh):
            s += np.float64(np.float32(v))
        acc[3] += s
        for a, n_ in enumerate(n):
            for c, m_ in enumerate(m):
                acc[4 + a * len(m) + c] += np.float64(counts[f"R@{n_}, IoU={m_}"])
    got = meter.state.numpy()
    assert got[1] == acc[1] and got[3] == acc[3]
    assert np.array_equal(got, acc)
    r = meter.result()
    assert r["num_samples"] == 16 and isinstance(r["num_samples"], int)
    for a, n_ in enumerate(n):
        for c, m_ in enumerate(m):
            assert r[f"R@{n_}, IoU={m_}"] == acc[4 + a * len(m) + c] / 16                       # main.py:163: / num_samples
    assert r["mIoU"] == acc[3] / 16
    assert r["loss"] == acc[1] / 13                                                              # main.py:162, over the batches with a loss
    assert list(r.keys()) == [f"R@{n_}, IoU={m_}" for n_ in n for m_ in m] + ["mIoU", "num_samples", "loss"]
    meter.reset()
    assert not meter.state.any()
    pm, ps, pe, mm, sm = ragged(2, 8, seed=3)
    meter.update(pm, ps, pe, mm, sm)
    assert "loss" not in meter.result()


def test_torch_meter_reproduces_reference_counts():
    """g6_ious.npz: the reference's own compute_ious on a fixed input; fed in two pieces, the totals survive the batch boundary."""
    api = V()
    z = H.load_npz("g6_ious")
    pm, ps, pe, mm, sm = (torch.from_numpy(z[k]) for k in ("pm", "ps", "pe", "mm", "sm"))
    meter = api.EpochMeterTorch()
    for sl in (slice(0, 4), slice(4, 6)):
        meter.update(pm[sl], ps[sl], pe[sl], mm[sl], sm[sl])
    assert meter.state[0] == 6 and meter.state[1] == 0 and meter.state[2] == 0
    assert meter.state[4:].tolist() == [float(v) for v in z["vals"]]
    r = meter.result()
    for k, v in zip(z["keys"], z["vals"]):
        assert r[str(k)] == float(v) / 6
    assert 0.0 < r["mIoU"] <= 1.0


def test_meter_argument_checks():
    api = V()
    with pytest.raises(ValueError, match="reference rule"):
        api.EpochMeter(n=(1, 3), device="cpu")
    with pytest.raises(ValueError, match="reference rule"):
        api.EpochMeterTorch(m=(0.5,))
    with pytest.raises(ValueError):
        api.EpochMeter(n=(1, 65), nms_thresh=0.5, device="cpu")                  # k = max(n) > 64
    with pytest.raises(ValueError):
        api.EpochMeterTorch(n=(1, 65), nms_thresh=0.5)
    with pytest.raises(ValueError):
        api.EpochMeter(n=(1, 5), m=tuple(0.01 * q for q in range(17)), nms_thresh=0.5, device="cpu")
    pm, ps, pe, mm, sm = ragged(2, 8, seed=1)
    meter = api.EpochMeter(device="cpu")
    with pytest.raises(api._lib.SminHipError, match="no CPU fallback"):
        meter.update(pm, ps, pe, mm, sm)
    assert not meter.state.any()


def test_result_raises_on_status_words(monkeypatch):
    api = V()
    M = api.meter
    pm, ps, pe, mm, sm = ragged(2, 8, seed=1)
    meter = api.EpochMeterTorch()
    meter.update(pm, ps, pe, mm, sm)
    word = torch.ones(1, dtype=torch.int32)
    monkeypatch.setattr(M, "_status_word", lambda device: word)
    with pytest.raises(RuntimeError, match="layout_status"):
        meter.result()
    assert int(word[0]) == 0                                                     # cleared, as CapturedStep does
    assert meter.result()["num_samples"] == 2                                    # ... so the next read passes
    monkeypatch.setattr(M, "_lstm_cluster_error", lambda device: 1)
    with pytest.raises(RuntimeError, match="smin_lstm_cluster_error") as e:
        meter.result()
    assert "layout_status" not in str(e.value)
    word.fill_(1)
    with pytest.raises(RuntimeError, match="layout_status.*and smin_lstm_cluster_error"):
        meter.result()
    monkeypatch.setattr(M, "_lstm_cluster_error", lambda device: 0)
    assert meter.result()["num_samples"] == 2


GLOO_BATCHES = [(4, 12, 31), (3, 12, 32), (5, 12, 33), (2, 12, 34)]             # (B, L, seed); rank r takes batches r, r + 2


def _gloo_worker(rank, world, port, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), WORLD_SIZE=str(world), RANK=str(rank), LOCAL_RANK=str(rank))
    torch.set_num_threads(2)
    import models
    api = models.vml_amd
    torch.distributed.init_process_group("gloo", rank=rank, world_size=world)
    meter = api.EpochMeterTorch(n=OTHER_N, m=OTHER_M, nms_thresh=0.5)
    for i in range(rank, len(GLOO_BATCHES), world):
        B, L, seed = GLOO_BATCHES[i]
        meter.update(*ragged(B, L, seed), loss=fake_loss(seed))
    own = meter.state.clone()
    r = meter.result(torch.distributed.group.WORLD)
    assert torch.equal(meter.state, own)                                         # the reduction leaves the rank's own state alone
    torch.distributed.barrier()
    q.put((rank, r))
    torch.distributed.destroy_process_group()


@pytest.mark.timeout(300)
def test_result_over_two_gloo_ranks():
    api = V()
    single = api.EpochMeterTorch(n=OTHER_N, m=OTHER_M, nms_thresh=0.5)
    cat = [torch.cat(x) for x in zip(*[ragged(B, L, seed) for B, L, seed in GLOO_BATCHES])]
    single.update(*cat)
    want = single.result()
    loss_sum = sum(float(np.float32(fake_loss(seed).item())) * B for B, L, seed in GLOO_BATCHES)
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = free_port()
    procs = [ctx.Process(target=_gloo_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = [q.get(timeout=240) for _ in procs]
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    assert sorted(r for r, _ in res) == [0, 1]
    for _, got in res:
        loss = got.pop("loss")
        assert got["num_samples"] == 14
        for k, v in want.items():
            # hit counts are integers: exact in any order; the top-1 sum is re-associated across ranks (fp64, 14 terms in [0, 1])
            assert got[k] == v if k != "mIoU" else abs(got[k] - v) <= 14 * 2.0 ** -52, k
        assert abs(loss - loss_sum / 14) <= 8 * 2.0 ** -52 * loss_sum / 14


# ---------------------------------------------------------------- GPU


RULES = [(None, REF_N, REF_M), (0.5, REF_N, REF_M), (0.45, (1, 3, 10, 64), (0.1, 0.5, 0.9))]


@pytest.mark.gpu
@pytest.mark.parametrize("nms_thresh,n,m", RULES)
@pytest.mark.parametrize("L,sizes", [(16, (64, 7, 1)), (64, (64, 13)), (512, (2, 2))])
def test_device_meter_equals_torch_meter_bitwise(dev, L, sizes, nms_thresh, n, m):
    """The same updates through EpochMeter (HIP) and EpochMeterTorch: identical fp64 state; the hit totals are also the sums of the
    per-batch HIP compute_ious calls, which in turn equal their torch forms (the per-sample stage is shared with the meter)."""
    api = V()
    hip, ref = api.EpochMeter(n=n, m=m, nms_thresh=nms_thresh, device=dev), api.EpochMeterTorch(n=n, m=m, nms_thresh=nms_thresh)
    assert hip.state.is_cuda and hip.state.dtype == torch.float64
    totals = dict.fromkeys(hip.keys, 0.0)
    for q, B in enumerate(sizes):
        args = ragged(B, L, seed=7 * L + q)
        loss = fake_loss(q) if q != 1 else None
        d = [x.to(dev) for x in args]
        hip.update(*d, loss=None if loss is None else loss.to(dev))
        ref.update(*args, loss=loss)
        per_batch = api.compute_ious(*d, n=n, m=m, nms_thresh=nms_thresh)
        assert per_batch == api.compute_ious_torch(*args, n=n, m=m, nms_thresh=nms_thresh), (L, B)
        for k, v in per_batch.items():
            totals[k] += v
    print("state", hip.state.tolist())
    assert torch.equal(bits64(hip.state), bits64(ref.state)), (hip.state.tolist(), ref.state.tolist())
    assert hip.state[4:].tolist() == [totals[k] for k in hip.keys]
    assert hip.result() == ref.result()
    hip.reset()
    assert not hip.state.any()


@pytest.mark.gpu
def test_updates_do_not_wait_for_the_device(dev):
    api = V()
    batches = [[x.to(dev) for x in ragged(B, 32, seed=B)] for B in (5, 9, 3)]
    losses = [fake_loss(q).to(dev) for q in range(3)]
    meters = [api.EpochMeter(device=dev), api.EpochMeter(n=(1, 5, 20), m=(0.3, 0.7), nms_thresh=0.5, device=dev)]
    for mt in meters:
        mt.update(*batches[0], loss=losses[0])                                   # first use outside the checked region (library load)
        mt.reset()
    torch.cuda.synchronize()
    mode = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        for mt in meters:
            for b, l in zip(batches, losses):
                mt.update(*b, loss=l)
    finally:
        torch.cuda.set_sync_debug_mode(mode)
    for mt in meters:
        assert mt.result()["num_samples"] == 17


def host_batches(T, L, Nq, Din, sizes, seed):
    g = torch.Generator().manual_seed(seed)
    out = []
    for B in sizes:
        dur = torch.rand(B, generator=g) * 100 + 5
        ts = torch.rand(B, generator=g) * dur * 0.5
        te = ts + 1.0 + torch.rand(B, generator=g) * (dur - ts - 1.0).clamp(min=0)
        nf = torch.randint(1, T + 1, (B,), generator=g)
        nf[0] = T
        vf = torch.randn(B, T, Din, generator=g)
        vf[torch.arange(T).unsqueeze(0) >= nf.unsqueeze(1)] = 0
        out.append(dict(video_features=vf.numpy(), query_features=torch.randn(B, Nq, 300, generator=g), nfeats=nf,
                        qlen=torch.randint(2, Nq + 1, (B,), generator=g), times=torch.stack([ts, te], 1), duration=dur))
    return out


KEYS = ["video_features", "video_mask", "query_features", "query_mask", "length_mask", "moment_mask", "sm", "ym", "ss", "ys", "se", "ye", "ya"]


@pytest.mark.gpu
def test_fed_batches_carry_their_cell_count(dev):
    api = V()
    T, L, Nq, Din, Vn = 64, 16, 9, 40, 53
    n = 0
    for fed in api.BatchFeeder(T, L, Nq, dev).feed(host_batches(T, L, Nq, Din, (6, 3, 8, 1, 5), seed=4)):
        assert list(fed.keys()) == KEYS and isinstance(fed, dict) and isinstance(fed.cell_count, int)
        assert fed.cell_count == int(fed["moment_mask"].sum())
        n += 1
    rng, g = np.random.default_rng(8), torch.Generator().manual_seed(8)
    table = torch.cat([torch.randn(Vn - 2, 300, generator=g), torch.zeros(2, 300)]).to(dev)
    raws = []
    for s, B in enumerate((6, 2, 7, 4)):
        lens = rng.integers(1, 4 * T + 1, B)
        lens[0] = T // 3
        ql = rng.integers(1, Nq + 1, B)
        tok = rng.integers(0, Vn - 1, (B, Nq))
        tok[np.arange(Nq)[None, :] >= ql[:, None]] = Vn - 1
        dur = torch.rand(B, generator=g) * 100 + 5
        ts = torch.rand(B, generator=g) * dur * 0.5
        rb = dict(raw_features=[torch.randn(int(k), Din, generator=g).numpy() for k in lens], tokens=tok,
                  times=torch.stack([ts, ts + 1.0], 1), duration=dur)
        if s % 2:
            rb["raw_lengths"], rb["raw_features"] = lens, np.concatenate(rb["raw_features"], 0)
        raws.append(rb)
    for pool in ("pick", "mean"):
        for fed in api.BatchFeeder(T, L, Nq, dev, embedding=table, pool=pool).feed(raws):
            assert list(fed.keys()) == KEYS and isinstance(fed.cell_count, int)
            assert fed.cell_count == int(fed["moment_mask"].sum())
            n += 1
    assert n == 13


def twin_models(dev, T, L, Din, Nq):
    import models
    torch.manual_seed(11)
    a = models.SMIN(T, L, 4, 64, 32, 2, Din, Nq, 32, dev).to(dev)
    b = models.SMIN(T, L, 4, 64, 32, 2, Din, Nq, 32, dev).to(dev)
    b.load_state_dict(a.state_dict())
    return a, b


def reference_style_epoch(api, model, optimizer, batches):
    """main.py:135-165 (optimizer given) / 167-191 as it runs without this feature: no count handed in, loss.item(), compute_ious."""
    total, metrics, num, items = 0.0, {}, 0, []
    model.train() if optimizer is not None else model.eval()
    for b in batches:
        B = b["video_features"].shape[0]
        if optimizer is not None:
            optimizer.zero_grad()
        with torch.enable_grad() if optimizer is not None else torch.no_grad():
            pm, ps, pe, pa = model(*H.model_inputs(b))
            loss = api.loss_fn(pm, b["ym"], b["sm"], b["moment_mask"], ps, b["ys"], b["ss"], pe, b["ye"], b["se"], pa, b["ya"], b["length_mask"])
        items.append((loss.item(), B))
        total += loss.item() * B
        iou = api.compute_ious(pm, ps, pe, b["moment_mask"], b["sm"])
        metrics = {k: metrics.get(k, 0.0) + v for k, v in iou.items()}
        if optimizer is not None:
            loss.backward()
            optimizer.step()
        num += B
    return total / num, {k: v / num for k, v in metrics.items()}, items, num


def loss_restated(items):
    """acc[1] / acc[2] of the meter in float64: sum of float64(loss) * B in batch order, over the samples."""
    s, n = np.float64(0.0), np.float64(0.0)
    for v, B in items:
        s += np.float64(v) * np.float64(B)                                       # loss.item() is the fp32 value widened
        n += np.float64(B)
    return float(s / n)


def fed_copies(api, dev, T, L, Nq, Din, sizes, seed):
    """The fed batches of one feeder run, cloned (a slot's tensors are reused) with their counts kept."""
    out = []
    for fed in api.BatchFeeder(T, L, Nq, dev).feed(host_batches(T, L, Nq, Din, sizes, seed)):
        c = api.FedBatch((k, v.clone()) for k, v in fed.items())
        c.cell_count = fed.cell_count
        out.append(c)
    return out


def status_word(api, dev):
    return int(api._lib.load_torch().layout_status(dev)[0])


@pytest.mark.gpu
def test_train_epoch_equals_reference_style_loop(dev):
    api = V()
    T, L, Nq, Din = 64, 16, 9, 40
    batches = fed_copies(api, dev, T, L, Nq, Din, (6, 3, 8, 5), seed=12)
    assert all(b.cell_count < b["moment_mask"].numel() for b in batches)          # ragged
    ma, mb = twin_models(dev, T, L, Din, Nq)
    oa, ob = (torch.optim.Adam(m.parameters(), lr=1e-3, fused=True) for m in (ma, mb))
    want_loss, want_metrics, items, num = reference_style_epoch(api, ma, oa, batches)
    meter = api.EpochMeter(device=dev)
    got_loss, got = api.train_epoch(mb, ob, batches, meter)
    assert mb.known_cell_count is None and mb.training
    for (k, p), (_, r) in zip(mb.named_parameters(), ma.named_parameters()):
        assert torch.equal(p.detach().view(torch.int32), r.detach().view(torch.int32)), k
    print("train loss", got_loss, want_loss, loss_restated(items))
    assert got_loss == loss_restated(items) == got["loss"]
    assert abs(got_loss - want_loss) <= 4 * 2.0 ** -52 * abs(want_loss)           # the reference's own sum: Python doubles, same terms
    assert got["num_samples"] == num == 22
    for k, v in want_metrics.items():
        assert got[k] == v, k
    assert 0.0 <= got["mIoU"] <= 1.0
    assert status_word(api, dev) == 0
    # a default meter is made when none is given
    loss2, got2 = api.train_epoch(mb, ob, batches[:1])
    assert got2["num_samples"] == 6 and np.isfinite(loss2)


@pytest.mark.gpu
@pytest.mark.parametrize("forward_only", [False, True])
def test_eval_epoch_and_test_model_equal_reference_style_loop(dev, forward_only):
    api = V()
    T, L, Nq, Din = 64, 16, 9, 40
    batches = fed_copies(api, dev, T, L, Nq, Din, (6, 3, 8, 5), seed=13)
    ma, mb = twin_models(dev, T, L, Din, Nq)
    mb.forward_only_scoring = forward_only
    want_loss, want_metrics, items, num = reference_style_epoch(api, ma, None, batches)
    got_loss, got = api.eval_epoch(mb, batches, api.EpochMeter(device=dev))
    assert mb.known_cell_count is None and not mb.training
    assert status_word(api, dev) == 0
    assert got["num_samples"] == num
    if not forward_only:
        assert got_loss == loss_restated(items) == got["loss"]
        for k, v in want_metrics.items():
            assert got[k] == v, k
        tm = api.test_model(mb, batches, api.EpochMeter(device=dev))
        assert "loss" not in tm and all(tm[k] == v for k, v in want_metrics.items()) and tm["mIoU"] == got["mIoU"]
    else:
        # score() agrees with forward to fp32 rounding in pm and exactly in ps / pe; the loops must hand over
        # exactly what score() returns with the count given, so compare the loop against score() driven by hand, bit for bit
        hand = api.EpochMeter(device=dev)
        with torch.no_grad():
            for b in batches:
                mb.known_cell_count = b.cell_count
                pm, ps, pe, pa = mb.score(*H.model_inputs(b))
                mb.known_cell_count = None
                fpm, fps, fpe, _ = ma(*H.model_inputs(b))
                assert torch.equal(ps, fps) and torch.equal(pe, fpe)
                err = float((pm - fpm).abs().max())
                print("score vs forward pm", err)
                assert err < 2e-6                                                # fp32 rounding (tests/test_score_path.py's bound)
                loss = api.loss_fn(pm, b["ym"], b["sm"], b["moment_mask"], ps, b["ys"], b["ss"], pe, b["ye"], b["se"], pa, b["ya"], b["length_mask"])
                hand.update(pm, ps, pe, b["moment_mask"], b["sm"], loss=loss)
        want = hand.result()
        assert got == want and got_loss == want["loss"]
        print("eval loss: forward-only", got_loss, "forward", want_loss)


@pytest.mark.gpu
def test_overcounted_batch_makes_result_raise(dev):
    """A cell_count raised by 7 (an OVER-count only: the forward then pads its cell list with inert cells and stays in bounds):
    the device's status word is set, result() raises naming it and clears it."""
    api = V()
    T, L, Nq, Din = 64, 16, 9, 40
    batches = fed_copies(api, dev, T, L, Nq, Din, (4, 3), seed=14)
    _, m = twin_models(dev, T, L, Din, Nq)
    meter = api.EpochMeter(device=dev)
    api.eval_epoch(m, batches, meter)                                            # clean epoch first
    assert status_word(api, dev) == 0
    batches[1].cell_count += 7
    meter.reset()
    with pytest.raises(RuntimeError, match="layout_status"):
        api.eval_epoch(m, batches, meter)
    assert status_word(api, dev) == 0 and m.known_cell_count is None
    batches[1].cell_count -= 7
    meter.reset()
    assert api.eval_epoch(m, batches, meter)[1]["num_samples"] == 7


@pytest.mark.gpu
def test_undercounted_batch_makes_result_raise(dev):
    """A cell_count lowered by 7: the forward runs on the layout of the mask's first count cells (csrc/layout.hip clamps row_ptr to the
    count, so every per-cell index stays in bounds), the status word is set, result() raises naming it and clears it.  The layout of
    that mask under that count is built alone first, and the epoch is not run if a row_ptr entry exceeds the count."""
    api = V()
    T, L, Nq, Din = 64, 16, 9, 40
    batches = fed_copies(api, dev, T, L, Nq, Din, (4, 3), seed=14)
    n = batches[1].cell_count - 7
    assert n > 0
    assert H.fail_unless_row_ptr_is_clamped(dev, batches[1]["moment_mask"], n) == 1
    _, m = twin_models(dev, T, L, Din, Nq)
    meter = api.EpochMeter(device=dev)
    api.eval_epoch(m, batches, meter)                                            # clean epoch first
    assert status_word(api, dev) == 0
    batches[1].cell_count -= 7
    meter.reset()
    try:
        with pytest.raises(RuntimeError, match="layout_status"):
            api.eval_epoch(m, batches, meter)
        assert status_word(api, dev) == 0 and m.known_cell_count is None
    finally:
        api._lib.load_torch().layout_status(dev).zero_()
    batches[1].cell_count += 7
    meter.reset()
    assert api.eval_epoch(m, batches, meter)[1]["num_samples"] == 7
