"""Top-k moment retrieval with greedy temporal NMS (moments.py, csrc/moments.hip): top_moments, SMIN.localize and
compute_ious(..., nms_thresh=t).  The independent reference is `py_nms` below, plain Python + numpy fp32 written from the
definition; `top_moments_torch` is checked against it on the CPU and the device kernels against `top_moments_torch`."""

import numpy as np
import pytest
import torch

from tests import helpers as H
from tests.support.device import dev  # noqa: F401  (the module's device fixture)
from tests.support.references import _api, check_against_py, py_nms, py_scores


# ---------------------------------------------------------------- independent reference (definition, plain Python)
def ragged(B, L, seed, dense_pm=False):
    g = torch.Generator().manual_seed(seed)
    lens = torch.randint(1, L + 1, (B,), generator=g)
    lens[0] = L
    lm = torch.arange(L).unsqueeze(0) < lens.unsqueeze(1)
    mm = torch.triu(lm.unsqueeze(2) & lm.unsqueeze(1))
    pm = torch.rand(B, L, L, generator=g)
    if not dense_pm:
        pm = pm * mm
    return pm, torch.rand(B, L, generator=g), torch.rand(B, L, generator=g), mm


# ---------------------------------------------------------------- CPU
@pytest.mark.parametrize("L", [1, 3, 16, 64])
def test_torch_restatement_equals_python_nms(L):
    api = _api()
    pm, ps, pe, mm = ragged(4, L, seed=L)
    for k in (1, 5, 64):
        for thr in (0.3, 0.5, 0.7, 1.0):
            r = api.top_moments_torch(pm, ps, pe, mm, k=k, nms_thresh=thr)
            assert r["idx"].dtype == torch.int64 and r["idx"].shape == (4, k, 2)
            assert r["score"].dtype == torch.float32 and r["count"].dtype == torch.int32
            check_against_py(r, pm, ps, pe, mm, k, thr)


def test_hand_worked_l4():
    """L = 4, full mask, hand-chosen scores (ps = pe = 1, so score = pm exactly)."""
    api = _api()
    L = 4
    mm = torch.triu(torch.ones(1, L, L, dtype=torch.bool))
    pm = torch.zeros(1, L, L)
    pm[0, 0, 3] = 0.9          # [0, 4): the whole video
    pm[0, 0, 2] = 0.8          # [0, 3): IoU 3/4 with (0, 3) -> suppressed at 0.5
    pm[0, 2, 3] = 0.7          # [2, 4): IoU 2/4 with (0, 3) -> kept at 0.5 (not > 0.5)
    pm[0, 1, 1] = 0.6          # [1, 2): IoU 1/4 with (0, 3), 0 with (2, 3) -> kept
    pm[0, 3, 3] = 0.5          # [3, 4): IoU 1/4, 1/2, 0 -> kept
    pm[0, 1, 0] = 0.99         # masked (below the diagonal): never returned
    ones = torch.ones(1, L)
    r = api.top_moments_torch(pm, ones, ones, mm, k=5, nms_thresh=0.5)
    assert r["idx"][0].tolist() == [[0, 3], [2, 3], [1, 1], [3, 3], [0, 0]]      # then score 0 ties by index: (0, 0) first
    assert r["score"][0].tolist() == [pytest.approx(0.9), pytest.approx(0.7), pytest.approx(0.6), pytest.approx(0.5), 0.0]
    # at 0.4: (0, 2) and (2, 3) (IoU 3/4 and 1/2 with the whole video) are suppressed; (1, 1) and (3, 3) (IoU 1/4) are kept
    r = api.top_moments_torch(pm, ones, ones, mm, k=3, nms_thresh=0.4)
    assert r["idx"][0].tolist() == [[0, 3], [1, 1], [3, 3]]
    # nothing suppressed at 1.0: the plain order, masked cell excluded
    r = api.top_moments_torch(pm, ones, ones, mm, k=4, nms_thresh=1.0)
    assert r["idx"][0].tolist() == [[0, 3], [0, 2], [2, 3], [1, 1]]
    # fewer valid cells than k: empty slots
    mm1 = torch.zeros(1, L, L, dtype=torch.bool)
    mm1[0, 0, 3] = mm1[0, 2, 3] = True
    r = api.top_moments_torch(pm, ones, ones, mm1, k=4, nms_thresh=0.3)
    assert r["idx"][0].tolist() == [[0, 3], [-1, -1], [-1, -1], [-1, -1]] and int(r["count"][0]) == 1
    assert r["score"][0, 1:].tolist() == [0.0, 0.0, 0.0]
    r = api.top_moments_torch(pm, ones, ones, mm1, k=4, nms_thresh=0.5, duration=torch.tensor([8.0]))
    assert r["times"][0, 0].tolist() == [0.0, 8.0] and r["times"][0, 1].tolist() == [4.0, 8.0]
    assert torch.isnan(r["times"][0, 2:]).all()


def test_no_suppression_equals_topk_over_valid_cells():
    api = _api()
    pm, ps, pe, mm = ragged(6, 16, seed=3)
    k = 10
    r = api.top_moments_torch(pm, ps, pe, mm, k=k, nms_thresh=1.0)
    s = torch.from_numpy(np.stack([py_scores(pm[b], ps[b], pe[b]) for b in range(6)])).reshape(6, -1)
    s = torch.where(mm.reshape(6, -1), s, torch.full_like(s, -1.0))
    for b in range(6):
        nv = int(mm[b].sum())
        val, top = s[b].topk(min(k, nv))
        assert int(r["count"][b]) == min(k, nv)
        assert torch.equal(r["score"][b, :len(val)], val)
        assert (r["idx"][b, :len(top), 0] * 16 + r["idx"][b, :len(top), 1]).tolist() == top.tolist()


def _py_hits(z, n, m, thr):
    pm, ps, pe, mm, sm = (z[k] for k in ("pm", "ps", "pe", "mm", "sm"))
    out = {}
    kept = [py_nms(pm[b], ps[b], pe[b], mm[b], max(n), thr) for b in range(pm.shape[0])]
    for n_ in n:
        for m_ in m:
            out[f"R@{n_}, IoU={m_}"] = float(sum(any(sm[b][i, j] > np.float32(m_) for i, j, _ in kept[b][:n_]) for b in range(len(kept))))
    return out


@pytest.mark.parametrize("thr", [0.3, 0.5, 0.7, 1.0])
def test_compute_ious_torch_nms_on_golden(thr):
    api = _api()
    z = H.load_npz("g6_ious")
    args = [torch.from_numpy(z[k]) for k in ("pm", "ps", "pe", "mm", "sm")]
    for n, m in (((1, 5), (0.1, 0.3, 0.5, 0.7)), ((1, 3, 10), (0.5, 0.9))):
        got = api.compute_ious_torch(*args, n=n, m=m, nms_thresh=thr)
        assert got == _py_hits(z, n, m, thr)


def test_top_moments_refuses_cpu_tensors_and_bad_arguments():
    api = _api()
    pm, ps, pe, mm = ragged(2, 8, seed=1)
    with pytest.raises(api._lib.SminHipError, match="no CPU fallback"):
        api.top_moments(pm, ps, pe, mm)
    for k in (0, 65):
        with pytest.raises(ValueError, match="k"):
            api.top_moments_torch(pm, ps, pe, mm, k=k)
    with pytest.raises(api._lib.SminHipError, match="no CPU fallback"):
        api.compute_ious(pm, ps, pe, mm, pm, nms_thresh=0.5)


def test_localize_adds_no_parameters():
    import models
    m = models.SMIN(16, 8, 4, 32, 16, 2, 24, 5, 16)
    assert hasattr(m, "localize")
    keys = set(m.state_dict())
    assert not any("local" in k and "localization" not in k for k in keys)


# ---------------------------------------------------------------- GPU
def _same(got, want):
    assert torch.equal(got["count"].cpu(), want["count"])
    assert torch.equal(got["idx"].cpu(), want["idx"])
    assert torch.equal(got["score"].cpu().view(torch.int32), want["score"].view(torch.int32))


@pytest.mark.gpu
@pytest.mark.parametrize("L", [3, 16, 64, 197, 512])
def test_top_moments_parity(dev, L):
    api = _api()
    pm, ps, pe, mm = ragged(7, L, seed=100 + L, dense_pm=(L == 64))
    dpm, dps, dpe, dmm = (x.to(dev) for x in (pm, ps, pe, mm))
    for k in (1, 5, 10, 64):
        for thr in (0.3, 0.5, 0.7, 1.0):
            got = api.top_moments(dpm, dps, dpe, dmm, k=k, nms_thresh=thr)
            want = api.top_moments_torch(pm, ps, pe, mm, k=k, nms_thresh=thr)
            _same(got, want)
    again = api.top_moments(dpm, dps, dpe, dmm, k=64, nms_thresh=0.5)
    assert torch.equal(again["idx"], api.top_moments(dpm, dps, dpe, dmm, k=64, nms_thresh=0.5)["idx"])


CAND = 4096          # csrc/moments.hip: candidate keys the NMS workgroup holds (and the bands hand it at most)


@pytest.mark.gpu
def test_top_moments_adversarial_continuation(dev):
    """L = 512, longer moments score higher: the whole video is kept first and the 32 896 moments longer than 256 clips
    (IoU > 0.5 with it) are all suppressed -- 8x the kernel's candidate buffer, so the continuation path must run."""
    api = _api()
    B, L = 2, 512
    i = torch.arange(L).view(L, 1)
    j = torch.arange(L).view(1, L)
    mm = (j >= i).unsqueeze(0).expand(B, L, L).contiguous()
    length = (j - i + 1).clamp_min(0).float()
    pm = (length / L).unsqueeze(0).expand(B, L, L).contiguous()
    pm[1] = pm[1] * (1 + 1e-3 * torch.rand(L, L, generator=torch.Generator().manual_seed(2)))
    ps, pe = torch.ones(B, L), torch.ones(B, L)
    n_long = int(((length > 256) & mm[0]).sum())
    assert n_long == 32896 and n_long > 8 * CAND
    for k, thr in ((5, 0.5), (64, 0.5), (64, 0.3)):
        got = api.top_moments(pm.to(dev), ps.to(dev), pe.to(dev), mm.to(dev), k=k, nms_thresh=thr)
        want = api.top_moments_torch(pm, ps, pe, mm, k=k, nms_thresh=thr)
        _same(got, want)
        assert got["idx"][0, 0].tolist() == [0, L - 1]
        assert int(got["idx"][0, 1, 1] - got["idx"][0, 1, 0]) + 1 <= 256
    # constant scores: pure index order, NMS applied in that order
    c = torch.full((B, L, L), 0.25)
    got = api.top_moments(c.to(dev), ps.to(dev), pe.to(dev), mm.to(dev), k=64, nms_thresh=0.5)
    want = api.top_moments_torch(c, ps, pe, mm, k=64, nms_thresh=0.5)
    _same(got, want)
    assert got["idx"][0, 0].tolist() == [0, 0]
    got = api.top_moments(c.to(dev), ps.to(dev), pe.to(dev), mm.to(dev), k=64, nms_thresh=1.0)
    assert got["idx"][0].tolist() == [[0, j_] for j_ in range(64)]


@pytest.mark.gpu
@pytest.mark.parametrize("thr", [0.3, 0.5, 0.7, 1.0])
def test_compute_ious_nms_on_device(dev, thr):
    api = _api()
    z = H.load_npz("g6_ious")
    args = [torch.from_numpy(z[k]) for k in ("pm", "ps", "pe", "mm", "sm")]
    for n, m in (((1, 5), (0.1, 0.3, 0.5, 0.7)), ((1, 3, 10, 64), (0.1, 0.5, 0.9))):
        got = api.compute_ious(*(x.to(dev) for x in args), n=n, m=m, nms_thresh=thr)
        assert got == api.compute_ious_torch(*args, n=n, m=m, nms_thresh=thr)
    pm, ps, pe, mm = ragged(5, 512, seed=7)
    sm = torch.rand(5, 512, 512, generator=torch.Generator().manual_seed(8)) * mm
    got = api.compute_ious(*(x.to(dev) for x in (pm, ps, pe, mm, sm)), nms_thresh=thr)
    assert got == api.compute_ious_torch(pm, ps, pe, mm, sm, nms_thresh=thr)
    if thr == 1.0:
        # every valid cell outscores every masked one (pm > 0 on valid cells, 0 on masked ones): equal to the reference metric
        assert got == api.compute_ious(*(x.to(dev) for x in (pm, ps, pe, mm, sm)))
        dz = [x.to(dev) for x in args]
        assert api.compute_ious(*dz, nms_thresh=1.0) == api.compute_ious(*dz)


@pytest.mark.gpu
def test_localize_end_to_end(dev):
    from oracle import smin_oracle as O            # test infrastructure: input / weight generators only
    import models
    api = _api()
    T, L, C, D, dl, layers, Din, Nq, Hh = H.FULL["tacos_d500"]
    sd = O.formula_state_dict(H.smin_shapes(T, L, C, D, dl, layers, Din, Nq, Hh), gain=1.3)
    m = models.SMIN(T, L, C, D, dl, layers, Din, Nq, Hh, dev)
    m.load_state_dict(sd)
    m = m.to(dev)
    keys = sorted(m.state_dict())
    batch = O.synthetic_batch(2, T, L, Nq, Din, seed=9)
    b = {k: v.to(dev) for k, v in batch.items()}
    dur = torch.tensor([37.5, 120.25], device=dev)
    got = m.localize(*H.model_inputs(b), k=10, nms_thresh=0.5, duration=dur)
    with torch.no_grad():
        pm, ps, pe, _ = m(*H.model_inputs(b))
    want = api.top_moments_torch(pm.cpu(), ps.cpu(), pe.cpu(), batch["moment_mask"], k=10, nms_thresh=0.5)
    _same(got, want)
    assert got["idx"].requires_grad is False and got["score"].requires_grad is False
    idx = got["idx"].cpu().double()
    d = dur.cpu().double().view(-1, 1)
    ok = idx[..., 0] >= 0
    for e, off in ((0, 0.0), (1, 1.0)):
        ref = (idx[..., e] + off) * d / L
        assert torch.allclose(got["times"].cpu()[..., e].double()[ok], ref[ok], rtol=1e-6, atol=0)
    assert torch.isnan(got["times"].cpu()[~ok]).all()
    assert sorted(m.state_dict()) == keys


@pytest.mark.gpu
def test_top_moments_graph_capture(dev):
    api = _api()
    pm, ps, pe, mm = (x.to(dev) for x in ragged(7, 197, seed=5))
    eager = api.top_moments(pm, ps, pe, mm, k=10, nms_thresh=0.5)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(2):
            api.top_moments(pm, ps, pe, mm, k=10, nms_thresh=0.5)
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = api.top_moments(pm, ps, pe, mm, k=10, nms_thresh=0.5)
    for x in out.values():
        x.zero_()
    g.replay()
    torch.cuda.synchronize()
    for key in ("idx", "score", "count"):
        assert torch.equal(out[key], eager[key]), key
    # new inputs copied into the captured buffers: the replay follows them
    pm2, ps2, pe2, mm2 = ragged(7, 197, seed=6)
    pm.copy_(pm2.to(dev)); ps.copy_(ps2.to(dev)); pe.copy_(pe2.to(dev)); mm.copy_(mm2.to(dev))
    g.replay()
    torch.cuda.synchronize()
    _same(out, api.top_moments_torch(pm2, ps2, pe2, mm2, k=10, nms_thresh=0.5))
