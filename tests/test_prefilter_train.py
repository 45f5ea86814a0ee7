"""Training the first-stage video score: csrc/prefilter.hip smin_prefilter_maps_bwd / smin_prefilter_bwd_ws_bytes,
functional.PrefilterMapsFn, moments.prefilter_maps, SMIN.prefilter_forward, training.prefilter_rank_loss / train_epoch_prefilter and the
``prefilter_weight`` of train_epoch_pairs / train_epoch_mined.

Host: the C ABI surface and the workspace layout, the defaults, the refusals, the all-pairs plan.
GPU, C ABI: the backward against fp64 autograd of prefilter_scores_torch under e_kernel <= 32 * e_torch32 + 1e-6 (e = max|x - x64| /
max|x64|, e_torch32 from fp32 autograd of the restatement on the device: the gate of tests/test_prefilter.py) for each of dfv, dfs, dw
and db, in the default mode and under f32e; the exact zeros; repeatability; NaN-prefilled outputs between sentinel bands; the exact
workspace; every rejection.
GPU, Python: prefilter_maps against prefilter_scores and the C ABI bit for bit; prefilter_forward on the tiny model; prefilter_rank_loss
against the fp64 restatement (the oracle's encoders -> prefilter_scores_torch -> pair_rank_loss_torch) under e_new <= 2 * e_ref32 + 1e-6
per parameter tensor (the gate of tests/test_pair_rank_loss.py's model-level tests); the two loops with prefilter_weight; twenty steps of
train_epoch_prefilter; and what did not move."""
import inspect
import os
import re

import numpy as np
import pytest
import torch

from tests.support.device import dev  # noqa: F401  (the module's device fixture)
from tests.support.device import vml as V
from tests.support.compare import byte_bits as bits
from tests.support.guards import banded, bands_intact, untouched, BAND
from tests.support.corpora import world  # noqa: F401  (fixture)
from tests.support.corpora import (
    checked, corpus_inputs, full_group, hand_step, on, pair_args, probe, same_parameters, tiny_model, GT_VIDEO, NO_ROWS, NQ, NV, TINY_SHAPE)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GRADS = ("dfv", "dfs", "dw", "db")
# Q, V, T, L, C, D: the base case; 15 operand rows padded to 16, dropped trailing frames and a partial K step; T % L != 0; two tiles each
# way in both contractions and three row splits; every lane of the row wave; the LDS limit
SHAPES = [(4, 5, 16, 8, 4, 32), (5, 3, 20, 5, 3, 20), (3, 2, 22, 5, 3, 20), (44, 9, 16, 8, 4, 32), (2, 2, 64, 64, 4, 8), (1, 1, 2048, 64, 8, 4)]


# ---------------------------------------------------------------- host
def test_header_table_and_names():
    import models
    A = V()
    text = open(os.path.join(ROOT, "include", "smin_hip.h")).read()
    assert re.search(r"\bsize_t\s+smin_prefilter_bwd_ws_bytes\s*\(\s*int\s+Q\s*,\s*int\s+V\s*,\s*int\s+T\s*,\s*int\s+D\s*\)", text)
    assert re.search(r"\bint\s+smin_prefilter_maps_bwd\s*\(", text)
    lib = A._lib.load()
    for name in ("smin_prefilter_bwd_ws_bytes", "smin_prefilter_maps_bwd"):
        assert name in A._lib.SIGNATURES and hasattr(lib, name), name
    assert len(A._lib.SIGNATURES["smin_prefilter_maps_bwd"]) == 24 and len(A._lib.SIGNATURES["smin_prefilter_bwd_ws_bytes"]) == 4
    assert "#define SMIN_HIP_ABI_VERSION 2" in text and lib.smin_abi_version() == 2
    # the forward's rejected sizes
    for bad in ((0, 3, 20, 20), (5, 0, 20, 20), (5, 3, 20, 18), (5, 3, 2049, 20), (65536, 3, 20, 20), (5, 3, 0, 20)):
        assert lib.smin_prefilter_bwd_ws_bytes(*bad) == 0 and lib.smin_prefilter_ws_bytes(*bad) == 0, bad
    # the layout of INTEGRATION.md 3w, by hand: da [V T][N3], the operand transposed [D][N3], sp slabs [N3][D], dop [N3][D], [Q V][4] fp64
    # (5, 3, 20, 20): N3 = 16, V T = 60, one output tile, sp = min(768, ceil(60 / 64)) = 1
    assert lib.smin_prefilter_bwd_ws_bytes(5, 3, 20, 20) == 4 * (60 * 16 + 20 * 16 + 1 * 16 * 20 + 16 * 20 + 8 * 15) == 8160
    # (44, 9, 16, 32): N3 = 132 (two tiles), V T = 144, sp = min(ceil(768 / 2), ceil(144 / 64)) = 3
    assert lib.smin_prefilter_bwd_ws_bytes(44, 9, 16, 32) == 4 * (144 * 132 + 32 * 132 + 3 * 132 * 32 + 132 * 32 + 8 * 396) == 173184
    for name in ("prefilter_maps", "prefilter_rank_loss", "train_epoch_prefilter"):
        assert callable(getattr(A, name)), name
    assert callable(A.moments.prefilter_maps) and callable(A.functional.PrefilterMapsFn.apply) and callable(models.SMIN.prefilter_forward)
    for loop in (A.train_epoch_pairs, A.train_epoch_mined):
        assert inspect.signature(loop).parameters["prefilter_weight"].default == 0.0


def cpu_group():
    vid, qry, tg = corpus_inputs()
    return dict(**vid, **qry, **tg, gt_video=GT_VIDEO)


def test_refusals_on_the_host():
    import models
    A = V()
    T, L, C, D = TINY_SHAPE[:4]
    fv, fs, w, b = torch.zeros(2, T, D), torch.zeros(3, D), torch.zeros(3, D), torch.zeros(3)
    lm, mm = torch.ones(2, L, dtype=torch.bool), torch.ones(2, L, L, dtype=torch.bool)
    with pytest.raises(A._lib.SminHipError):
        A.prefilter_maps(fv, fs, w, b, lm, mm, T, L, C)
    m, _ = tiny_model()
    g = cpu_group()
    xs = pair_args(g, g)
    with pytest.raises(A._lib.SminHipError):
        m.prefilter_forward(*xs)                                                                        # CPU tensors
    with pytest.raises(ValueError, match="fused"):
        m.prefilter_forward(xs[0].double(), *xs[1:])
    with pytest.raises(ValueError, match="fused"):
        m.prefilter_forward(xs[0], xs[1], xs[2].double(), *xs[3:])
    with pytest.raises(ValueError, match="fused"):
        m.prefilter_forward(xs[0][:, :T - 1], xs[1][:, :T - 1], *xs[2:])                                # T differs from the model's
    m.backbone.queryencoder.fused_lstm = False
    with pytest.raises(ValueError, match="fused"):
        m.prefilter_forward(*xs)
    m.backbone.queryencoder.fused_lstm = True
    with pytest.raises(ValueError, match="tau"):
        m.prefilter_forward(*xs, tau=0.0)
    with pytest.raises(ValueError, match="moment_mask"):
        m.prefilter_forward(xs[0], xs[1], xs[2], xs[3], xs[4], xs[5][:2])
    for bad in (dict(tau=0.0), dict(gamma=float("inf")), dict(tau=None)):
        with pytest.raises(ValueError):
            A.prefilter_rank_loss(m, g, **bad)
    for gt in (None, [0, 1, 2], [0, 1, 2, 5]):
        with pytest.raises(ValueError, match="gt_video"):
            A.prefilter_rank_loss(m, dict(g, gt_video=gt))

    def never():
        raise AssertionError("the weight is checked ahead of the first step")
        yield
    for bad in (-0.5, float("inf"), float("nan"), None, "1"):
        with pytest.raises(ValueError, match="prefilter_weight"):
            A.train_epoch_pairs(m, None, never(), prefilter_weight=bad)
        with pytest.raises(ValueError, match="prefilter_weight"):
            A.train_epoch_mined(m, None, never(), 2, prefilter_weight=bad)
    with pytest.raises(ValueError):
        A.train_epoch_prefilter(m, None, never(), tau=-1.0)
    with pytest.raises(ValueError, match="no group"):
        A.train_epoch_prefilter(m, None, [])
    assert isinstance(m, models.SMIN)


def test_all_pairs_plan():
    A = V()
    Q, Vn = 4, 5
    plan = A.training.all_pairs_plan(Vn, Q, GT_VIDEO, "cpu")
    assert plan.P == Q * Vn and plan.V == Vn and plan.Q == Q and plan.num_positive == Q
    assert plan.q_ptr.tolist() == [q * Vn for q in range(Q + 1)] and plan.q_pairs.tolist() == list(range(Q * Vn))
    assert plan.query_index.tolist() == [p // Vn for p in range(Q * Vn)] and plan.video_index.tolist() == [p % Vn for p in range(Q * Vn)]
    assert plan.positive.tolist() == [int(p % Vn == GT_VIDEO[p // Vn]) for p in range(Q * Vn)]
    assert plan.positive_rows.tolist() == [q * Vn + GT_VIDEO[q] for q in range(Q)]
    assert A.training.all_pairs_plan(Vn, Q, np.array(GT_VIDEO), "cpu") is plan                          # kept: one copy per group
    assert A.training.all_pairs_plan(Vn, Q, [2, 0, 3, 2], "cpu") is not plan


# ---------------------------------------------------------------- GPU, C ABI


_INPUTS = {}


def inputs(shape, dev):
    """random fp32 banks, heads and upstream gradients and ragged masks of a shape: video 0 is full, video V // 2 has no valid cell (V
    >= 2) and the last video a single clip (V >= 3).  Made once per shape, with the references' gradients."""
    if shape in _INPUTS:
        return _INPUTS[shape]
    A = V()
    Q, Vn, T, L, C, D = shape
    g = torch.Generator().manual_seed(sum(shape))
    fv, fs = torch.randn(Vn, T, D, generator=g), torch.randn(Q, D, generator=g)
    w, b = torch.randn(3, D, generator=g) / D ** 0.5, torch.randn(3, generator=g) / 2
    lens = torch.randint(1, L + 1, (Vn,), generator=g)
    lens[0] = L
    if Vn >= 2:
        lens[Vn // 2] = 0
    if Vn >= 3:
        lens[Vn - 1] = 1
    lm = torch.arange(L).unsqueeze(0) < lens.unsqueeze(1)
    mm = torch.triu(lm.unsqueeze(2) & lm.unsqueeze(1))
    up = [torch.randn(Q * Vn, L, L, generator=g), torch.randn(Q * Vn, L, generator=g), torch.randn(Q * Vn, L, generator=g)]
    x = dict(fv=fv.to(dev), fs=fs.to(dev), w=w.to(dev), b=b.to(dev), lm=lm.to(dev), mm=mm.to(dev), up=[u.to(dev) for u in up], shape=shape, lens=lens)

    def autograd(dtype):
        leaves = [x[k].to(dtype).requires_grad_(True) for k in ("fv", "fs", "w", "b")]
        out = A.prefilter_scores_torch(*leaves, x["lm"], x["mm"], T, L, C, 0.1, maps=True)
        loss = sum((o.reshape(u.shape) * u.to(dtype)).sum() for o, u in zip(out[3:], x["up"]))
        return [t.detach() for t in torch.autograd.grad(loss, leaves)]
    x["ref64"], x["ref32"] = autograd(torch.float64), autograd(torch.float32)
    _INPUTS[shape] = x
    return x


def forward_abi(dev, x):
    """the stored outputs (pm0, ps0, pe0) of smin_prefilter_scores in the current mode"""
    L_ = V()._lib
    Q, Vn, T, L, C, D = x["shape"]
    new = lambda *s: torch.empty(s, dtype=torch.float32, device=dev)
    outs = [new(Q, Vn), new(Q, Vn, 2), new(Q, Vn), new(Q * Vn, L, L), new(Q * Vn, L), new(Q * Vn, L)]
    nbytes = int(L_.load().smin_prefilter_ws_bytes(Q, Vn, T, D))
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    lm, mm = x["lm"].to(torch.uint8), x["mm"].to(torch.uint8)
    L_.call("smin_prefilter_scores", L_.stream(), *[L_.ptr(x[k]) for k in ("fv", "fs", "w", "b")], L_.ptr(lm), L_.ptr(mm), Q, Vn, T, L, C, D, 0.1,
            *[L_.ptr(o) for o in outs], L_.ptr(ws), nbytes)
    torch.cuda.synchronize()
    return outs[3:]


def bwd_abi(dev, x, maps, up=None, fill=float("nan"), ws_delta=0, **kw):
    """smin_prefilter_maps_bwd through the C ABI over banded outputs and a banded workspace of exactly the queried size (+ ws_delta); kw
    overrides arguments by name.  Returns (rc, outputs by name, their whole buffers)"""
    L_ = V()._lib
    Q, Vn, T, L, C, D = x["shape"]
    up = x["up"] if up is None else up
    shapes = dict(dfv=(Vn, T, D), dfs=(Q, D), dw=(3, D), db=(3,))
    bufs, outs = {}, {}
    for name, shape in shapes.items():
        bufs[name], outs[name] = banded(shape, dev, fill)
    a = dict(dpm0=up[0], dps0=up[1], dpe0=up[2], pm0=maps[0], ps0=maps[1], pe0=maps[2], fv=x["fv"], fs=x["fs"], w=x["w"],
             lmask=x["lm"].to(torch.uint8), mm=x["mm"].to(torch.uint8), Q=Q, V=Vn, T=T, L=L, C=C, D=D)
    a.update(outs)
    nbytes = int(L_.load().smin_prefilter_bwd_ws_bytes(Q, Vn, T, D)) + ws_delta
    ws_buf = torch.full((max(nbytes, 0) + 2 * BAND,), 77, dtype=torch.uint8, device=dev)
    a.update(ws=ws_buf[BAND:], ws_bytes=nbytes)
    a.update(kw)
    p = lambda key: L_.ptr(a[key])
    rc = L_.load().smin_prefilter_maps_bwd(L_.stream(), *[p(k) for k in ("dpm0", "dps0", "dpe0", "pm0", "ps0", "pe0", "fv", "fs", "w", "lmask", "mm")],
                                          a["Q"], a["V"], a["T"], a["L"], a["C"], a["D"], p("dfv"), p("dfs"), p("dw"), p("db"), p("ws"), a["ws_bytes"])
    torch.cuda.synchronize()
    assert bool(ws_buf[:BAND].eq(77).all()) and bool(ws_buf[BAND + max(nbytes, 0):].eq(77).all()), "the workspace's neighbours were written"
    return rc, outs, bufs


def gate(name, got, want, ref32):
    """e_kernel <= 32 * e_torch32 + 1e-6 with e = max|x - x64| / max|x64| (tests/test_prefilter.py's gate); prints the share used"""
    g, w, r = got.detach().cpu().double(), want.detach().cpu().double(), ref32.detach().cpu().double()
    assert g.shape == w.shape and torch.isfinite(g).all(), name
    scale = w.abs().max().item()
    if scale == 0.0:
        assert g.abs().max().item() == 0.0, name
        return
    e_k, e_t = (g - w).abs().max().item() / scale, (r - w).abs().max().item() / scale
    print(f"{name}: e_kernel {e_k:.2e}  e_torch32 {e_t:.2e}  share {e_k / (32 * e_t + 1e-6):.3f}")
    assert e_k <= 32 * e_t + 1e-6, (name, e_k, e_t)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["default", "f32e"])
@pytest.mark.parametrize("shape", SHAPES)
def test_maps_bwd_kernel(dev, shape, mode):
    """Measured on an MI355X: the table of INTEGRATION.md 3w."""
    A = V()
    Q, Vn, T, L, C, D = shape
    assert shape != SHAPES[1] or ((3 * Q) % 4 != 0 and D % 16 != 0)
    assert shape != SHAPES[2] or T % L != 0
    assert shape != SHAPES[3] or (3 * Q > 128 and Vn * T > 128)
    x = inputs(shape, dev)
    default = A._lib.DEFAULT_GEMM_MODE
    try:
        A.set_gemm_mode(default if mode == "default" else mode)
        maps = forward_abi(dev, x)
        rc, o, bufs = bwd_abi(dev, x, maps)                                          # a workspace of exactly the queried size
        rc2, o2, _ = bwd_abi(dev, x, maps, fill=0.0)
        # what a mask hides may hold anything: NaN upstream at every masked entry
        keep_m = x["mm"].repeat(Q, 1, 1)
        keep_l = x["lm"].repeat(Q, 1)
        nan = torch.full((), float("nan"), device=dev)
        hidden = [torch.where(keep_m, x["up"][0], nan), torch.where(keep_l, x["up"][1], nan), torch.where(keep_l, x["up"][2], nan)]
        rc3, o3, _ = bwd_abi(dev, x, maps, up=hidden)
    finally:
        A.set_gemm_mode(default)
    assert rc == 0 and rc2 == 0 and rc3 == 0 and A.get_gemm_mode() == default
    for name in GRADS:
        assert torch.isfinite(o[name]).all() and bands_intact(bufs[name]), name      # every element written over the NaN, none past the end
        assert torch.equal(bits(o[name]), bits(o2[name])), name                      # the same bits on a second run
        assert torch.equal(bits(o[name]), bits(o3[name])), name                      # dpm0 / dps0 / dpe0 under a zero mask: exactly nothing
    if Vn >= 2:
        assert o["dfv"][Vn // 2].abs().max().item() == 0.0                           # a pair without a valid cell contributes exactly 0
    if T % L != 0:
        assert o["dfv"][:, T // L * L:].abs().max().item() == 0.0                    # the frames no clip reaches
    for k, name in enumerate(GRADS):
        gate(f"{shape} {mode} {name}", o[name], x["ref64"][k], x["ref32"][k])


SAT_SHAPE = SHAPES[1]                                  # tests/test_prefilter.py's SAT_SHAPE: every window mean weighs whole frames


@pytest.mark.gpu
@pytest.mark.parametrize("level", ["hard", "frozen"])
def test_maps_bwd_saturated(dev, level):
    """smin_prefilter_maps_bwd on saturated_prefilter (tests/support/corpora.py; tests/test_prefilter.py shows on the host that the cases
    are in the regime they name), on the maps smin_prefilter_scores stored: everything finite and the project's gate for dfv, dfs, dw and
    db against fp64 autograd of the restatement; and with an upstream gradient that is nonzero only where the stored score p has
    p (1 - p) == 0 -- scores of exactly 0.0 and 1.0 -- every gradient is exactly 0.  Measured on an MI355X: INTEGRATION.md, "Saturated
    inputs"."""
    from tests.support.corpora import saturated_prefilter
    A = V()
    Q, Vn, T, L, C, D = SAT_SHAPE
    x, z = saturated_prefilter(inputs(SAT_SHAPE, dev), level)

    def autograd(dtype):
        leaves = [x[k].to(dtype).requires_grad_(True) for k in ("fv", "fs", "w", "b")]
        out = A.prefilter_scores_torch(*leaves, x["lm"], x["mm"], T, L, C, 0.1, maps=True)
        loss = sum((o.reshape(u.shape) * u.to(dtype)).sum() for o, u in zip(out[3:], x["up"]))
        return [t.detach() for t in torch.autograd.grad(loss, leaves)]
    want, ref32 = autograd(torch.float64), autograd(torch.float32)
    maps = forward_abi(dev, x)
    rc, o, bufs = bwd_abi(dev, x, maps)
    assert rc == 0 and all(torch.isfinite(o[name]).all() and bands_intact(bufs[name]) for name in GRADS)
    for k, name in enumerate(GRADS):
        gate(f"prefilter_maps_bwd {level} {name}", o[name], want[k], ref32[k])
    flat = [(m * (1 - m) == 0) for m in maps]
    assert all(bool(f.any()) for f in flat) and (level == "frozen" or not all(bool(f.all()) for f in flat))
    rc, o, _ = bwd_abi(dev, x, maps, up=[torch.where(f, u, torch.zeros_like(u)) for f, u in zip(flat, x["up"])])
    assert rc == 0 and all(bool((o[name] == 0).all()) for name in GRADS)


@pytest.mark.gpu
def test_zero_masks_give_exact_zeros(dev):
    """every lmask zero: dps0 and dpe0 contribute exactly 0 to dfv, dfs and dw (the map's heads alone remain), db[1] = db[2] = 0"""
    x = dict(inputs(SHAPES[0], dev))
    maps = forward_abi(dev, x)
    zero_up = [x["up"][0], torch.zeros_like(x["up"][1]), torch.zeros_like(x["up"][2])]
    rc0, want, _ = bwd_abi(dev, x, maps, up=zero_up)
    x["lm"] = torch.zeros_like(x["lm"])
    rc, got, _ = bwd_abi(dev, x, maps)
    assert rc == 0 and rc0 == 0
    assert got["db"][1:].abs().max().item() == 0.0
    for name in ("dfv", "dfs", "db"):
        assert torch.equal(bits(got[name]), bits(want[name])), name
    assert torch.equal(bits(got["dw"][0]), bits(want["dw"][0])) and got["dw"][1:].abs().max().item() == 0.0
    x["mm"] = torch.zeros_like(x["mm"])
    rc, got, _ = bwd_abi(dev, x, maps)
    assert rc == 0 and all(got[name].abs().max().item() == 0.0 for name in GRADS)


@pytest.mark.gpu
def test_workspace_and_rejections(dev):
    x = inputs(SHAPES[1], dev)
    Q, Vn, T, L, C, D = x["shape"]
    maps = forward_abi(dev, x)
    rc, o, bufs = bwd_abi(dev, x, maps, ws_delta=-1)                                  # one byte less than the queried size
    assert rc != 0 and untouched(o, bufs)
    cases = [dict(Q=0), dict(V=0), dict(T=L - 1), dict(T=2049), dict(L=0), dict(L=65), dict(C=0), dict(C=65537), dict(D=18), dict(D=0)]
    cases += [{name: None} for name in ("dpm0", "dps0", "dpe0", "pm0", "ps0", "pe0", "fv", "fs", "w", "lmask", "mm", "dfv", "dfs", "dw", "db", "ws")]
    for kw in cases:
        rc, o, bufs = bwd_abi(dev, x, maps, **kw)
        o = {k: v for k, v in o.items() if k not in kw}
        assert rc != 0 and untouched(o, {k: bufs[k] for k in o}), kw
    # an output that is one of the inputs, another output or the workspace
    spare = torch.full((Vn * T * D,), float("nan"), device=dev)
    for kw in (dict(dfv=x["fv"]), dict(dfs=x["fs"]), dict(dw=x["w"]), dict(dfv=maps[0]), dict(db=x["up"][1]), dict(dfs=spare, dw=spare), dict(ws=x["up"][0])):
        keep = {k: x[k].clone() for k in ("fv", "fs", "w")}
        rc, o, bufs = bwd_abi(dev, x, maps, **kw)
        o = {k: v for k, v in o.items() if k not in kw}
        assert rc != 0 and untouched(o, {k: bufs[k] for k in o}), list(kw)
        assert all(torch.equal(bits(x[k]), bits(keep[k])) for k in keep) and bool(torch.isnan(spare).all())
    rc, o, bufs = bwd_abi(dev, x, maps)
    assert rc == 0 and all(bool(torch.isfinite(o[name]).all()) for name in GRADS)


# ---------------------------------------------------------------- GPU, Python
@pytest.mark.gpu
@pytest.mark.parametrize("shape", SHAPES[:3])
def test_prefilter_maps_is_the_abi(dev, shape, monkeypatch):
    A = V()
    Q, Vn, T, L, C, D = shape
    x = inputs(shape, dev)
    leaves = [x[k].clone().requires_grad_(True) for k in ("fv", "fs", "w", "b")]
    got = A.prefilter_maps(*leaves, x["lm"], x["mm"], T, L, C, 0.1)
    want = A.prefilter_scores(x["fv"], x["fs"], x["w"], x["b"], x["lm"], x["mm"], T, L, C, 0.1, maps=True)
    assert len(got) == 4 and not got[3].requires_grad and all(t.requires_grad for t in got[:3])
    for name, g, r in zip(("pm0", "ps0", "pe0", "score"), got, (want[3], want[4], want[5], want[0])):
        assert g.shape == r.shape and torch.equal(bits(g), bits(r)), name
    up = [u.reshape(o.shape) for u, o in zip(x["up"], got[:3])]
    grads = torch.autograd.grad(list(got[:3]), leaves, up)
    rc, o, _ = bwd_abi(dev, x, [t.detach().reshape(u.shape) for t, u in zip(got[:3], x["up"])])
    assert rc == 0
    for name, g in zip(GRADS, grads):
        assert torch.equal(bits(g), bits(o[name])), name
    # one call, never tiled: past the cap it refuses
    monkeypatch.setattr(A.moments, "PREFILTER_WS_CAP", 1000)
    with pytest.raises(ValueError, match="workspace"):
        A.prefilter_maps(*leaves, x["lm"], x["mm"], T, L, C, 0.1)


def stacked_heads(m):
    D = TINY_SHAPE[3]
    heads = (m.localization.conv_layer_pm, m.localization.conv_layer_ps, m.localization.conv_layer_pe)
    return torch.stack([h.weight.reshape(D) for h in heads]), torch.cat([h.bias.reshape(1) for h in heads])


@pytest.mark.gpu
def test_prefilter_forward_on_the_tiny_model(dev, world):
    """with a video without rows (NO_ROWS): the maps are prefilter_scores' on the modules' own fv / fs, in pair order p = q V + v"""
    A, m = V(), world["m"]
    T, L, C = TINY_SHAPE[:3]
    vid, qry, _ = corpus_inputs(snips=NO_ROWS)
    vid, qry = on(dev, vid), on(dev, qry)
    pm0, ps0, pe0, score = m.prefilter_forward(*pair_args(vid, qry))
    assert tuple(pm0.shape) == (NQ * NV, L, L) and tuple(ps0.shape) == tuple(pe0.shape) == (NQ * NV, L) and tuple(score.shape) == (NQ, NV)
    assert pm0.requires_grad and ps0.requires_grad and pe0.requires_grad and not score.requires_grad
    with torch.no_grad():
        fv = m.backbone.videoencoder(vid["video_features"], vid["video_mask"])
        fs, _ = m.backbone.queryencoder(qry["query_features"], qry["query_mask"])
        w, b = stacked_heads(m)
        want = A.prefilter_scores(fv, fs, w, b, vid["length_mask"], vid["moment_mask"], T, L, C, 0.1, maps=True)
    for name, g, r in (("pm0", pm0, want[3]), ("ps0", ps0, want[4]), ("pe0", pe0, want[5]), ("score", score, want[0])):
        assert torch.equal(bits(g), bits(r.reshape(g.shape))), name
    assert score[:, 2].eq(0).all() and pm0.reshape(NQ, NV, L, L)[:, 2].eq(0).all()     # the video without rows


def rank_loss_restated(api, sd, vid, qry, dtype, encoders):
    """encoders -> prefilter_scores_torch -> pair_rank_loss_torch in ``dtype``; returns the loss (graph attached)"""
    T, L, C, D = TINY_SHAPE[:4]
    fv, fs = encoders(vid, qry)
    names = ("conv_layer_pm", "conv_layer_ps", "conv_layer_pe")
    w = torch.stack([sd[f"localization.{n}.weight"].reshape(D) for n in names])
    b = torch.stack([sd[f"localization.{n}.bias"].reshape(()) for n in names])
    out = api.prefilter_scores_torch(fv, fs, w, b, vid["length_mask"], vid["moment_mask"], T, L, C, 0.1, maps=True)
    plan = api.PairPlan(np.tile(np.arange(NV), NQ), np.repeat(np.arange(NQ), NV), NV, NQ, fv.device, gt_video=GT_VIDEO)
    mm = vid["moment_mask"].index_select(0, plan.video_index.long())
    return api.pair_rank_loss_torch(out[3].reshape(NQ * NV, L, L), out[4].reshape(NQ * NV, L), out[5].reshape(NQ * NV, L), mm, plan, 0.1, 0.1)


@pytest.mark.gpu
def test_rank_loss_gradients_against_fp64(dev, world):
    """prefilter_rank_loss and its gradients on every parameter of the encoders and the three heads against the fp64 restatement (the
    oracle's encoders -> prefilter_scores_torch -> pair_rank_loss_torch), under e_new <= 2 * e_ref32 + 1e-6 per parameter tensor
    (tests/test_pair_rank_loss.py's gate_model).

    What e_ref32 is, and why.  The heads' bias gradients are sums that cancel: in the fp64 restatement on the CPU, sum|terms| / |sum
    terms| is 339 (pm), 98 (ps) and 301 (pe) -- the softmax weights of a contrastive loss sum to zero over a query's videos.  Any two fp32
    forwards whose maps differ in the last bit therefore differ by some 1e-5 on these one-element tensors, whatever forms the gradient
    (the fp32 restatement on the CPU alone: 1.2e-5, 1.5e-6, 9.9e-6), and an independent fp32 route is a sample of that noise, not a
    yardstick (measured with it: pe.bias 8.72e-06 against 1.89e-06).  gate_model's two routes share their forward bits and differ in the
    part under test only; so do these: the comparator is the only route the parent commit has -- the modules' encoders,
    prefilter_scores_torch with autograd on the device, the existing pair_rank_loss --, with its maps' VALUES set to the kernel's bits
    (t + (h - t).detach(): exact, since h - t is), its pair order, mask gather and plan written out here.  The loss value is compared
    with the independent fp32 restatement's.  Measured on an MI355X, the worst tensor (conv_layer_pe.bias): e_new 1.34e-05 / e_ref32
    6.44e-06 (f32: 96 % of its gate), 1.43e-05 / 1.10e-05 (f32e); every tensor but the three biases: under 1.3e-06 on both sides."""
    from oracle import smin_oracle as O
    api, m = V(), world["m"]
    T, L, C, D = TINY_SHAPE[:4]
    sd64 = {k: v.double().requires_grad_(True) for k, v in world["sd"].items()}
    enc64 = lambda vid, qry: (O.video_encoder(sd64, vid["video_features"].double(), vid["video_mask"]),
                              O.query_encoder(sd64, qry["query_features"].double(), qry["query_mask"])[0])
    loss64 = rank_loss_restated(api, sd64, world["vid"], world["qry"], torch.float64, enc64)
    loss64.backward()
    g64 = {k: v.grad for k, v in sd64.items() if v.grad is not None}
    trained = {k for k in g64 if k.startswith("backbone.") or re.match(r"localization\.conv_layer_p[mse]\.", k)}
    assert trained == set(g64) and len(trained) == 19 + 6

    def model_grads(route):
        for p in m.parameters():
            p.grad = None
        loss = route()
        loss.backward()
        torch.cuda.synchronize()
        return loss.detach().item(), {k: (None if p.grad is None else p.grad.detach().clone()) for k, p in m.named_parameters()}
    vid, qry = world["vid_d"], world["qry_d"]
    g = dict(**vid, **qry, gt_video=GT_VIDEO)
    l_new, g_new = model_grads(lambda: api.prefilter_rank_loss(m, g))
    enc32 = lambda vid, qry: (m.backbone.videoencoder(vid["video_features"], vid["video_mask"]),
                              m.backbone.queryencoder(qry["query_features"], qry["query_mask"])[0])

    def parent_route():
        fv, fs = enc32(vid, qry)
        w, b = stacked_heads(m)
        t = api.prefilter_scores_torch(fv, fs, w, b, vid["length_mask"], vid["moment_mask"], T, L, C, 0.1, maps=True)[3:]
        h = api.prefilter_scores(fv.detach(), fs.detach(), w.detach(), b.detach(), vid["length_mask"], vid["moment_mask"], T, L, C, 0.1, maps=True)[3:]
        maps = [a + (c - a).detach() for a, c in zip(t, h)]
        assert all(torch.equal(bits(a), bits(c)) for a, c in zip(maps, h))
        plan = api.PairPlan(np.tile(np.arange(NV), NQ), np.repeat(np.arange(NQ), NV), NV, NQ, dev, gt_video=GT_VIDEO)
        mm = torch.stack([vid["moment_mask"][p % NV] for p in range(NQ * NV)])
        return api.pair_rank_loss(maps[0].reshape(NQ * NV, L, L), maps[1].reshape(NQ * NV, L), maps[2].reshape(NQ * NV, L), mm, plan, 0.1, 0.1)
    l_ref, g_ref = model_grads(parent_route)
    with torch.no_grad():
        l_32 = rank_loss_restated(api, dict(m.named_parameters()), vid, qry, torch.float32, enc32).item()
    print("prefilter_rank_loss", l_new, "parent route", l_ref, "fp32 restatement", l_32, "fp64", loss64.item())
    assert loss64.item() > 0 and abs(l_new - loss64.item()) <= 2 * abs(l_32 - loss64.item()) + 1e-6 * abs(loss64.item())
    for k, grad in g_new.items():                                                    # no SMI layer (and no pa head) is touched
        assert (grad is not None) == (k in trained), k
    assert any(k.startswith("smis.") for k in g_new)
    worst = [0.0, 0.0]
    for k in sorted(trained):
        r = g64[k]
        scale = r.abs().max().item()
        a, c = g_new[k].cpu().double(), g_ref[k].cpu().double()
        assert scale > 1e-9, k
        e_new, e_ref = (a - r).abs().max().item() / scale, (c - r).abs().max().item() / scale
        worst = [max(worst[0], e_new), max(worst[1], e_ref)]
        print(f"  {k}: e_new {e_new:.2e}  e_ref32 {e_ref:.2e}")
        assert e_new <= 2 * e_ref + 1e-6, (k, e_new, e_ref)
    print(api.get_gemm_mode(), f"prefilter_rank_loss, worst tensor: e_new {worst[0]:.2e}  e_ref32 {worst[1]:.2e}")


def fresh(api, world, dev):
    m, _ = tiny_model(dev)
    return m, api.FusedAdam(m.parameters(), lr=1e-3)


@pytest.mark.gpu
@pytest.mark.parametrize("loop", ["pairs", "mined"])
def test_loops_with_the_first_stage_term(dev, world, loop):
    api = V()
    Probe = probe(api)
    g = full_group(dev, lists=loop == "pairs")
    run = (lambda m, opt, groups, **kw: api.train_epoch_pairs(m, opt, groups, Probe(device=dev), **kw)) if loop == "pairs" else \
          (lambda m, opt, groups, **kw: api.train_epoch_mined(m, opt, groups, 2, meter=Probe(device=dev), **kw))
    # prefilter_weight 0.0 is the call without the argument, bit for bit, after two steps
    a, opt_a = fresh(api, world, dev)
    c, opt_c = fresh(api, world, dev)
    run(a, opt_a, [g, g])
    run(c, opt_c, [g, g], prefilter_weight=0.0)
    same_parameters(a, c)
    # prefilter_weight 0.5: the two terms computed separately, and no host read before the meter's
    twin, _ = tiny_model(dev)
    twin.train()
    if loop == "pairs":
        plan = api.PairPlan(g["video_index"], g["query_index"], NV, NQ, dev, gt_video=GT_VIDEO)
    else:
        with torch.no_grad():
            videos = twin.encode_videos(g["video_features"], g["video_mask"], g["length_mask"], g["moment_mask"], cell_counts=g["cell_counts"])
            queries = twin.encode_queries(g["query_features"], g["query_mask"])
            plan = twin.mine_pairs(videos, queries, GT_VIDEO, 2)
    base = hand_step(api, twin, g, plan, None).item()
    term = api.prefilter_rank_loss(twin, g).item()
    want = base + 0.5 * term
    assert term > 0
    m, opt = fresh(api, world, dev)
    run(m, opt, [g], prefilter_weight=0.5)                                           # (first use outside the checked region)
    m, opt = fresh(api, world, dev)
    Probe.reads = 0
    loss, metrics = checked(lambda: run(m, opt, [g], prefilter_weight=0.5))
    print(f"train_epoch_{loop} prefilter_weight 0.5: loss", loss, "by hand", want, "=", base, "+ 0.5 *", term)
    assert Probe.reads == 1 and m.known_cell_count is None
    assert abs(loss - want) <= 1e-6 * abs(want) and loss == metrics["loss"]
    assert int(api._lib.load_torch().layout_status(dev)[0]) == 0


@pytest.mark.gpu
def test_twenty_steps_lower_the_loss(dev, world):
    """one fixed tiny group (V = 5, Q = 4), FusedAdam at lr 1e-3 over all the parameters: the loss of the twentieth step is below the
    first's -- a condition on a deterministic run; the SMI layers do not move"""
    api = V()
    g = full_group(dev, lists=False)
    m, _ = tiny_model(dev)
    opt = api.FusedAdam(m.parameters(), lr=1e-3)
    losses, hits = [], []
    for _ in range(20):
        loss, hit = api.train_epoch_prefilter(m, opt, [g], tau=0.1, gamma=0.1)
        losses.append(loss)
        hits.append(hit)
    print("train_epoch_prefilter: losses", [round(x, 5) for x in losses], "hit rates", hits)
    assert all(np.isfinite(losses)) and losses[-1] < losses[0] and all(0.0 <= h <= 1.0 for h in hits)
    for k, p in m.named_parameters():
        if k.startswith("smis."):
            assert torch.equal(bits(p), bits(world["sd"][k].to(dev))), k
    two, hit = api.train_epoch_prefilter(m, opt, [g, g])                                 # the mean over two groups
    assert np.isfinite(two) and 0.0 <= hit <= 1.0


@pytest.mark.gpu
def test_nothing_else_moved(dev, world):
    """search(prefilter=M), prefilter_videos and pair_rank_loss (value and gradients) give the same bits before and after a first-stage
    backward"""
    api, m = V(), world["m"]
    vd, qd = world["vid_d"], world["qry_d"]
    g = dict(**vd, **qd, gt_video=GT_VIDEO)
    plan = api.training.all_pairs_plan(NV, NQ, GT_VIDEO, dev)
    gen = torch.Generator().manual_seed(5)
    L = TINY_SHAPE[1]
    maps = [torch.rand(NQ * NV, L, L, generator=gen).to(dev), torch.rand(NQ * NV, L, generator=gen).to(dev), torch.rand(NQ * NV, L, generator=gen).to(dev)]
    mm = vd["moment_mask"].index_select(0, plan.video_index)

    def everything():
        with torch.no_grad():
            vb = m.encode_videos(vd["video_features"], vd["video_mask"], vd["length_mask"], vd["moment_mask"])
            qb = m.encode_queries(qd["query_features"], qd["query_mask"])
        a = m.search(vb, qb, k=7, k_video=3, prefilter=2, gt_video=GT_VIDEO)
        b = m.prefilter_videos(vb, qb, 3, gt_video=GT_VIDEO)
        leaves = [t.clone().requires_grad_(True) for t in maps]
        loss = api.pair_rank_loss(*leaves, mm, plan)
        grads = torch.autograd.grad(loss, leaves)
        return [bits(v) for r in (a, b) for v in r.values()] + [bits(loss.reshape(1))] + [bits(t) for t in grads]

    before = everything()
    for p in m.parameters():
        p.grad = None
    api.prefilter_rank_loss(m, g).backward()
    torch.cuda.synchronize()
    after = everything()
    assert len(before) == len(after) and all(torch.equal(x, y) for x, y in zip(before, after))
