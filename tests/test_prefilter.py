"""First-stage pruning of corpus search from the banks alone: csrc/prefilter.hip smin_prefilter_scores /
smin_prefilter_select, moments.prefilter_scores / prefilter_select and their restatements, SMIN.prefilter_videos and search(prefilter=M).

Host: the C ABI surface; prefilter_scores_torch in fp64 against the oracle's own pieces (backbone -> proposal_generation -> localization
-> pair_pool_torch: the first stage is the reference model with its layers skipped) and against a dense content_matrix einsum;
prefilter_select_torch against a hand-written loop; the refusals.
GPU: smin_prefilter_scores through the C ABI -- its score / pool / cells are smin_pair_pool's bits on its own maps, the same bits with
NULL maps, on tiles of two videos and on a second run, NaN-prefilled outputs between sentinel bands, against the fp64 restatement under
e_kernel <= 32 * e_torch32 + 1e-6 (e = max|x - x64| / max|x64|, e_torch32 the fp32 restatement on the same device; the gate of
tests/test_video_rank.py) in the default mode and under f32e, the exact workspace and every rejection --; smin_prefilter_select against
its restatement bit for bit; prefilter_videos on a VideoBank and a WindowBank; search(prefilter=M) against search(pairs=...) on the
surviving pairs bit for bit, without a host read, and prefilter=None against search_torch."""
import os
import re

import numpy as np
import pytest
import torch

from tests.support import corpora as WS
from tests.support.device import dev  # noqa: F401  (the module's device fixture)
from tests.support.device import vml as V
from tests.support.compare import byte_bits as bits, gate, same
from tests.support.guards import banded, bands_intact, untouched, BAND
from tests.support.corpora import corpus_inputs, expand, host_pairs, inputs, tiny_model, GT_VIDEO, NO_ROWS, SEARCH_KEYS, SHAPES, TINY_SHAPE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TAUS = [1.0, 0.1, 0.01]


def heads64(sd, D):
    names = ("conv_layer_pm", "conv_layer_ps", "conv_layer_pe")
    w = torch.stack([sd[f"localization.{n}.weight"].double().reshape(D) for n in names])
    b = torch.stack([sd[f"localization.{n}.bias"].double().reshape(()) for n in names])
    return w, b


# ---------------------------------------------------------------- host: surface
def test_header_table_and_names():
    A = V()
    text = open(os.path.join(ROOT, "include", "smin_hip.h")).read()
    assert re.search(r"\bsize_t\s+smin_prefilter_ws_bytes\s*\(", text)
    assert re.search(r"\bint\s+smin_prefilter_scores\s*\(", text) and re.search(r"\bint\s+smin_prefilter_select\s*\(", text)
    lib = A._lib.load()
    for name in ("smin_prefilter_ws_bytes", "smin_prefilter_scores", "smin_prefilter_select"):
        assert name in A._lib.SIGNATURES and hasattr(lib, name), name
    assert len(A._lib.SIGNATURES["smin_prefilter_scores"]) == 22 and len(A._lib.SIGNATURES["smin_prefilter_select"]) == 7
    assert "#define SMIN_HIP_ABI_VERSION 2" in text and lib.smin_abi_version() == 2
    # the layout the entry point carves: the operand [3 Q rounded up to 4][D] and the transposed projections [.][V T rounded up to 4]
    assert lib.smin_prefilter_ws_bytes(5, 3, 20, 20) == 4 * (16 * 20 + 16 * 60)
    assert lib.smin_prefilter_ws_bytes(4, 5, 17, 32) == 4 * (12 * 32 + 12 * 88)
    assert lib.smin_prefilter_ws_bytes(0, 3, 20, 20) == 0 and lib.smin_prefilter_ws_bytes(5, 3, 20, 18) == 0
    for name in ("prefilter_scores", "prefilter_scores_torch", "prefilter_select", "prefilter_select_torch"):
        assert callable(getattr(A, name)) and callable(getattr(A.moments, name)), name
    import models
    assert callable(models.SMIN.prefilter_videos)
    import inspect
    assert inspect.signature(models.SMIN.search).parameters["prefilter"].default is None


# ---------------------------------------------------------------- host: the restatements
def test_first_stage_is_the_reference_model_without_its_layers():
    """prefilter_scores_torch on the oracle's banks against backbone -> proposal_generation -> localization -> pair_pool_torch on the
    expanded pairs, all fp64."""
    from oracle import smin_oracle as O
    A = V()
    T, L, C, D = TINY_SHAPE[:4]
    _, sd = tiny_model()
    sd = {k: v.double() for k, v in sd.items()}
    vid, qry, _ = corpus_inputs(snips=NO_ROWS)
    Vn, Q = 5, 4
    qi, vi = np.repeat(np.arange(Q), Vn), np.tile(np.arange(Vn), Q)
    x = expand(vid, qry, vi, qi)
    x[0], x[2] = x[0].double(), x[2].double()
    with torch.no_grad():
        f, _, _ = O.backbone(sd, x[0], x[1], x[2], x[3])
        _, fm, fb = O.proposal_generation(f, x[5], T, L, C)
        pm, ps, pe, _ = O.localization(sd, fm, fb, x[4], x[5])
        want = A.pair_pool_torch(pm, ps, pe, x[5], 0.1)
        fv = O.video_encoder(sd, vid["video_features"].double(), vid["video_mask"])
        fs, _ = O.query_encoder(sd, qry["query_features"].double(), qry["query_mask"])
        w, b = heads64(sd, D)
        got = A.prefilter_scores_torch(fv, fs, w, b, vid["length_mask"], vid["moment_mask"], T, L, C, 0.1, maps=True)
    assert got[0].dtype == torch.float64 and tuple(got[0].shape) == (Q, Vn) and tuple(got[3].shape) == (Q, Vn, L, L)
    for name, g, r in (("pm0", got[3].reshape(-1, L, L), pm), ("ps0", got[4].reshape(-1, L), ps), ("pe0", got[5].reshape(-1, L), pe),
                       ("score", got[0].reshape(-1), want[0]), ("pool", got[1].reshape(-1, 2), want[1]), ("cells", got[2].reshape(-1), want[2])):
        err = (g - r).abs().max().item()
        print(name, err)
        assert err <= 1e-12, (name, err)
    assert pm.abs().max().item() > 0.1 and got[2][:, 2].eq(0).all() and got[0][:, 2].eq(0).all() and got[1][:, 2].eq(0).all()
    assert got[2][0].tolist() == [36.0, 1.0, 0.0, 36.0, 6.0]


@pytest.mark.parametrize("T,L,C", [(8, 8, 4), (16, 8, 4), (20, 5, 3), (64, 16, 4)])
def test_restatement_against_a_dense_content_matrix(T, L, C):
    """n < C (r = 1, 2), cs > 1 with dropped trailing frames ((20, 5, 3): n = 4, 8, 16, 20), r in {1, 2, 4}"""
    from oracle import smin_oracle as O
    A = V()
    g = torch.Generator().manual_seed(T + L)
    Q, Vn, D = 3, 4, 8
    fv, fs = torch.randn(Vn, T, D, generator=g, dtype=torch.float64), torch.randn(Q, D, generator=g, dtype=torch.float64)
    w, b = torch.randn(3, D, generator=g, dtype=torch.float64) / 2, torch.randn(3, generator=g, dtype=torch.float64) / 2
    lens = torch.tensor([L, 1, 0, max(L // 2, 1)])
    lm = torch.arange(L).unsqueeze(0) < lens.unsqueeze(1)
    mm = torch.triu(lm.unsqueeze(2) & lm.unsqueeze(1))
    r = T // L
    start, size = O.content_windows(T, L, C)
    assert int(size.sum(-1).max()) <= T and (start + size).max() <= T
    drops = any(int(size[i, j].sum()) < (j - i + 1) * r for i in range(L) for j in range(i, L))
    assert drops == (r % C != 0)                                                     # a window drops trailing frames unless C divides every n
    assert int(size.max()) > 1 or r == 1                                                                # cs > 1 wherever r > 1
    Wc = O.content_matrix(T, L, C, torch.float64)                                    # (L, L, C, T)
    f = fv.unsqueeze(0) * fs.reshape(Q, 1, 1, D)                                     # (Q, V, T, D): Backbone's f = fv * fs
    fm = torch.einsum("lmct,qvtd->qvlmcd", Wc, f).mean(dim=4)
    pm = torch.sigmoid(fm @ w[0] + b[0]) * mm.unsqueeze(0)
    fb = f[:, :, :L * r].reshape(Q, Vn, L, r, D).mean(dim=3)
    ps, pe = torch.sigmoid(fb @ w[1] + b[1]) * lm.unsqueeze(0), torch.sigmoid(fb @ w[2] + b[2]) * lm.unsqueeze(0)
    want = A.pair_pool_torch(pm.reshape(-1, L, L), ps.reshape(-1, L), pe.reshape(-1, L), mm.repeat(Q, 1, 1), 0.1)
    got = A.prefilter_scores_torch(fv, fs, w, b, lm, mm, T, L, C, 0.1, maps=True)
    for name, x, y in (("pm0", got[3], pm), ("ps0", got[4], ps), ("pe0", got[5], pe), ("score", got[0].reshape(-1), want[0]),
                       ("pool", got[1].reshape(-1, 2), want[1]), ("cells", got[2].reshape(-1), want[2])):
        assert (x - y).abs().max().item() <= 1e-12, (name, (x - y).abs().max().item())
    short = A.prefilter_scores_torch(fv, fs, w, b, lm, mm, T, L, C, 0.1)
    assert len(short) == 3 and torch.equal(short[0], got[0])


def select_loop(rank, M):
    Q, Vn = len(rank), len(rank[0])
    Ms = min(M, Vn)
    out = []
    for q in range(Q):
        keep = [v for v in range(Vn) if 0 <= rank[q][v] < Ms]
        spare = [v for v in range(Vn) if rank[q][v] < 0]
        out.append(sorted(keep + spare[:Ms - len(keep)]))
    return out, [[q] * Ms for q in range(Q)]


def ranks_case(Vn, seed):
    """three queries over Vn videos: all candidates, none, and fewer than any M > 1 (one candidate where Vn > 1)"""
    g = torch.Generator().manual_seed(seed)
    full = torch.randperm(Vn, generator=g).to(torch.int32)
    none = torch.full((Vn,), -1, dtype=torch.int32)
    few = none.clone()
    few[int(torch.randint(Vn, (1,), generator=g))] = 0
    some = torch.where(torch.rand(Vn, generator=g) < 0.5, torch.ones(Vn), torch.zeros(Vn)).bool()
    part = none.clone()
    part[some] = torch.randperm(int(some.sum()), generator=g).to(torch.int32)
    return torch.stack([full, none, few, part])


@pytest.mark.parametrize("Vn", [1, 5])
def test_select_restatement_against_a_loop(Vn):
    A = V()
    rank = ranks_case(Vn, 7 + Vn)
    for M in (1, 3, Vn, Vn + 7):
        video, query = A.prefilter_select_torch(rank, M)
        want_v, want_q = select_loop(rank.tolist(), M)
        assert video.dtype == torch.int32 and query.dtype == torch.int32 and tuple(video.shape) == (4, min(M, Vn))
        assert video.tolist() == want_v and query.tolist() == want_q, (Vn, M)
    assert A.prefilter_select_torch(torch.tensor([[1, -1, 0, -1, 2]]), 4)[0].tolist() == [[0, 1, 2, 4]]


def test_refusals_on_the_host():
    import models
    A = V()
    T, L, C, D = TINY_SHAPE[:4]
    fv, fs, w, b = torch.zeros(2, T, D), torch.zeros(3, D), torch.zeros(3, D), torch.zeros(3)
    lm, mm = torch.ones(2, L, dtype=torch.bool), torch.ones(2, L, L, dtype=torch.bool)
    with pytest.raises(A._lib.SminHipError):
        A.prefilter_scores(fv, fs, w, b, lm, mm, T, L, C)
    with pytest.raises(A._lib.SminHipError):
        A.prefilter_select(torch.zeros(2, 3, dtype=torch.int32), 2)
    for bad_tau in (0.0, -1.0, float("inf"), float("nan"), None):
        with pytest.raises(ValueError):
            A.prefilter_scores_torch(fv, fs, w, b, lm, mm, T, L, C, tau=bad_tau)
    for bad_m in (0, -1, 2.0, None):
        with pytest.raises(ValueError):
            A.prefilter_select_torch(torch.zeros(2, 3, dtype=torch.int32), bad_m)
    with pytest.raises(ValueError):
        A.prefilter_scores_torch(fv[:, :, :30], fs[:, :30], w[:, :30], b, lm, mm, T, L, C)              # D % 4 != 0
    with pytest.raises(ValueError):
        A.prefilter_scores_torch(fv[:, :4], fs, w, b, lm, mm, 4, L, C)                                  # T < L
    m = models.SMIN(*TINY_SHAPE)
    vb = A.VideoBank(fv, torch.zeros(2, T, 24), torch.ones(2, T, 1, dtype=torch.uint8), lm, mm, (36, 36))
    qb = A.QueryBank(torch.zeros(3, 5, D), fs, torch.zeros(3, 5, 300), torch.ones(3, 5, dtype=torch.uint8))
    with pytest.raises(ValueError, match="prefilter"):
        m.search(vb, qb, pairs=[(0, 0)], prefilter=1)
    with pytest.raises(ValueError, match="prefilter"):
        m.search(vb, qb, carry=True, prefilter=1)
    for bad_m in (0, -3, 1.5):
        with pytest.raises(ValueError, match="M"):
            m.prefilter_videos(vb, qb, bad_m)
        with pytest.raises(ValueError, match="M"):
            m.search(vb, qb, prefilter=bad_m)
    with pytest.raises(ValueError, match="tau"):
        m.prefilter_videos(vb, qb, 1, tau=0.0)
    with pytest.raises(ValueError, match="gt_video"):
        m.prefilter_videos(vb, qb, 1, gt_video=[0])
    with pytest.raises(A._lib.SminHipError):
        m.prefilter_videos(vb, qb, 1)                                                                   # CPU banks
    with pytest.raises(A._lib.SminHipError):
        m.search(vb, qb, prefilter=1)


# ---------------------------------------------------------------- GPU
def references(x, tau):
    """(fp64 restatement, fp32 restatement) on the device, maps included: computed once per (shape, tau)"""
    A = V()
    if tau not in x["ref"]:
        _, _, T, L, C, _ = x["shape"]
        f64 = [x[k].double() for k in ("fv", "fs", "w", "b")]
        x["ref"][tau] = (A.prefilter_scores_torch(*f64, x["lm"], x["mm"], T, L, C, tau, maps=True),
                         A.prefilter_scores_torch(x["fv"], x["fs"], x["w"], x["b"], x["lm"], x["mm"], T, L, C, tau, maps=True))
    return x["ref"][tau]


def scores_abi(dev, x, tau, maps=True, v0=0, v1=None, fill=float("nan"), ws_delta=0, **kw):
    """smin_prefilter_scores through the C ABI on videos [v0, v1) over banded outputs; kw overrides arguments by name.
    Returns (rc, outputs by name, their whole buffers)"""
    L_ = V()._lib
    Q, Vn, T, L, C, D = x["shape"]
    v1 = Vn if v1 is None else v1
    n = v1 - v0
    shapes = dict(score=(Q, n), pool=(Q, n, 2), cells=(Q, n), pm0=(Q * n, L, L), ps0=(Q * n, L), pe0=(Q * n, L))
    bufs, outs = {}, {}
    for name, shape in shapes.items():
        bufs[name], outs[name] = banded(shape, dev, fill)
    a = dict(fv=x["fv"][v0:v1].contiguous(), fs=x["fs"], w=x["w"], b=x["b"], lmask=x["lm"][v0:v1].contiguous(), mm=x["mm"][v0:v1].contiguous(),
             Q=Q, V=n, T=T, L=L, C=C, D=D, tau=tau)
    a.update(outs)
    if not maps:
        a.update(pm0=None, ps0=None, pe0=None)
    a.update(kw)
    nbytes = int(L_.load().smin_prefilter_ws_bytes(Q, n, T, D)) + ws_delta
    ws_buf = torch.full((max(nbytes, 0) + 2 * BAND,), 77, dtype=torch.uint8, device=dev)
    a.setdefault("ws", ws_buf[BAND:])
    a.setdefault("ws_bytes", nbytes)
    p = lambda key: L_.ptr(a[key])
    rc = L_.load().smin_prefilter_scores(L_.stream(), p("fv"), p("fs"), p("w"), p("b"), p("lmask"), p("mm"), a["Q"], a["V"], a["T"], a["L"], a["C"],
                                         a["D"], a["tau"], p("score"), p("pool"), p("cells"), p("pm0"), p("ps0"), p("pe0"), p("ws"), a["ws_bytes"])
    torch.cuda.synchronize()
    assert bool(ws_buf[:BAND].eq(77).all()) and bool(ws_buf[BAND + max(nbytes, 0):].eq(77).all()), "the workspace's neighbours were written"
    return rc, outs, bufs


@pytest.mark.gpu
@pytest.mark.parametrize("tau", TAUS)
@pytest.mark.parametrize("shape", SHAPES)
def test_prefilter_scores_kernel(dev, shape, tau):
    """(5, 3, 20, 5, 3, 20): 3 Q = 15 is padded to 16 operand rows, D % 16 != 0 (the engine's partial K step), cs > 1 with dropped frames;
    (44, 9, 16, 8, 4, 32): 132 operand columns (two column tiles), V T = 144 rows (past one 128-row tile); (3, 2, 64, 16, 4, 64): r = 4.
    Measured on an MI355X: in the table of INTEGRATION.md 3v."""
    A = V()
    Q, Vn, T, L, C, D = shape
    assert shape != SHAPES[1] or ((3 * Q) % 4 != 0 and D % 16 != 0)
    assert shape != SHAPES[2] or (3 * Q > 128 and Vn * T > 128)
    x = inputs(shape, dev)
    names = ("score", "pool", "cells", "pm0", "ps0", "pe0")
    rc, o, bufs = scores_abi(dev, x, tau)
    assert rc == 0
    for name in names:
        assert torch.isfinite(o[name]).all(), name                                   # every element written over the NaN
        assert bands_intact(bufs[name]), name
    # score / pool / cells are smin_pair_pool's bits on the kernel's own maps and the gathered masks
    mm_pairs = x["mm"].repeat(Q, 1, 1)
    ps, pp, pc = A.pair_pool(o["pm0"], o["ps0"], o["pe0"], mm_pairs, tau)
    assert torch.equal(bits(o["score"].reshape(-1)), bits(ps)) and torch.equal(bits(o["pool"].reshape(-1, 2)), bits(pp))
    assert torch.equal(bits(o["cells"].reshape(-1)), bits(pc))
    assert o["cells"][0].tolist() == x["mm"].reshape(Vn, -1).sum(1).float().tolist()
    # the video without a valid cell
    z = Vn // 2
    assert bits(o["score"][:, z]).eq(0).all() and bits(o["pool"][:, z]).eq(0).all() and bits(o["cells"][:, z]).eq(0).all()
    assert o["pm0"].reshape(Q, Vn, L, L)[:, z].eq(0).all() and o["ps0"].reshape(Q, Vn, L)[:, z].eq(0).all()
    # NULL maps, a second run (over another fill), tiles of two videos: the same bits
    rc, o_null, bufs_null = scores_abi(dev, x, tau, maps=False)
    assert rc == 0 and all(bands_intact(b) for b in bufs_null.values())
    rc, o_again, _ = scores_abi(dev, x, tau, fill=-7.0)
    assert rc == 0
    for name in names:
        assert torch.equal(bits(o_again[name]), bits(o[name])), name
        if name in ("score", "pool", "cells"):
            assert torch.equal(bits(o_null[name]), bits(o[name])), name
        else:
            assert torch.isnan(o_null[name]).all(), name                              # (not passed: not written)
    for v0 in range(0, Vn, 2):
        v1 = min(v0 + 2, Vn)
        rc, o_t, bufs_t = scores_abi(dev, x, tau, v0=v0, v1=v1)
        assert rc == 0 and all(bands_intact(b) for b in bufs_t.values())
        for name in ("score", "pool", "cells"):
            assert torch.equal(bits(o_t[name]), bits(o[name][:, v0:v1])), (name, v0)
        for name, tail in (("pm0", (L, L)), ("ps0", (L,)), ("pe0", (L,))):
            assert torch.equal(bits(o_t[name].reshape(Q, v1 - v0, *tail)), bits(o[name].reshape(Q, Vn, *tail)[:, v0:v1])), (name, v0)
    # the Python entry point: the same bits, whole and with its tiles forced small
    got = A.prefilter_scores(x["fv"], x["fs"], x["w"], x["b"], x["lm"], x["mm"], T, L, C, tau, maps=True)
    cap = A.moments.PREFILTER_WS_CAP
    try:
        A.moments.PREFILTER_WS_CAP = int(A._lib.load().smin_prefilter_ws_bytes(Q, 2, T, D))
        tiled = A.prefilter_scores(x["fv"], x["fs"], x["w"], x["b"], x["lm"], x["mm"], T, L, C, tau)
    finally:
        A.moments.PREFILTER_WS_CAP = cap
    for k, name in enumerate(names):
        assert torch.equal(bits(got[k].reshape(o[name].shape)), bits(o[name])), name
        assert k >= 3 or torch.equal(bits(tiled[k]), bits(o[name])), name
    # against the fp64 restatement, gated by the fp32 restatement's error: the default mode and f32e
    want, ref32 = references(x, tau)
    assert torch.equal(o["cells"].double(), want[2])
    default = A._lib.DEFAULT_GEMM_MODE
    for mode in (default, "f32e"):
        try:
            A.set_gemm_mode(mode)
            rc, om, _ = scores_abi(dev, x, tau)
        finally:
            A.set_gemm_mode(default)
        assert rc == 0 and A.get_gemm_mode() == default
        tag = f"{shape} tau {tau} {mode}"
        gate(tag + " pm0", om["pm0"].reshape(Q, Vn, L, L), want[3], ref32[3])
        gate(tag + " ps0", om["ps0"].reshape(Q, Vn, L), want[4], ref32[4])
        gate(tag + " pe0", om["pe0"].reshape(Q, Vn, L), want[5], ref32[5])
        gate(tag + " score", om["score"], want[0], ref32[0])
        gate(tag + " pool.m", om["pool"][..., 0], want[1][..., 0], ref32[1][..., 0])
        gate(tag + " pool.sum", om["pool"][..., 1], want[1][..., 1], ref32[1][..., 1])


SAT_SHAPE = SHAPES[1]                                  # the smallest shape, and one whose every window mean weighs whole frames (T // L >= C)
LEVELS = ("hard", "frozen")


@pytest.mark.parametrize("level", LEVELS)
def test_saturated_first_stage_inputs_hold_what_they_claim(level):
    """On the fp64 restatement: the three heads' pre-activations of a pair are c_v k_q at every valid cell and clip -- frozen: all in
    +-{20, 95, 110}, each under both signs; hard: two fifths beyond +-17 and three fifths inside +-4 --, so the scores of a pair are all
    sigmoid(c_v k_q), exactly 1.0f from +20 on and 0.0f at -110."""
    A = V()
    Q, Vn, T, L, C, D = SAT_SHAPE
    x, z = WS.saturated_prefilter(WS.uncached_inputs(SAT_SHAPE, "cpu"), level)
    out = A.prefilter_scores_torch(x["fv"].double(), x["fs"].double(), x["w"].double(), x["b"].double(), x["lm"], x["mm"], T, L, C, 0.1, maps=True)
    p = torch.sigmoid(z.double())
    for m, valid in ((out[3], x["mm"]), (out[4], x["lm"]), (out[5], x["lm"])):
        assert bool(valid.any()) and not bool(valid.all())
        want = p.view(Q, Vn, *([1] * (m.dim() - 2))) * valid.unsqueeze(0)
        assert (m - want).abs().max().item() <= 1e-6 * 110                         # (sigmoid' <= 1/4; the inputs carry fp32's rounding)
    live = z[:, x["lm"].any(1)]
    if level == "frozen":
        assert {abs(v) for v in live.flatten().tolist()} == set(WS.PREFILTER_PRE) and bool((live > 0).any() and (live < 0).any())
        assert {v for v in live.flatten().tolist()} >= {s * m for m in WS.PREFILTER_PRE for s in (-1.0, 1.0)}
    else:
        assert (live.abs() > 17).double().mean().item() >= 0.25 and (live.abs() < 4).double().mean().item() >= 0.25
    assert bool((p[z >= 20].float() == 1.0).all()) and bool((p[z <= -110].float() == 0.0).all())


@pytest.mark.gpu
@pytest.mark.parametrize("level", LEVELS)
def test_prefilter_scores_saturated(dev, level):
    """smin_prefilter_scores on saturated_prefilter: the maps exactly 1.0 where the pair's pre-activation is +20 or more and exactly 0.0 at
    -110, +0.0 at every masked cell and snippet, everything finite, and the project's gate for the maps, the score and the pool against
    the fp64 restatement.  Measured on an MI355X: INTEGRATION.md, "Saturated inputs"."""
    Q, Vn, T, L, C, D = SAT_SHAPE
    x, z = WS.saturated_prefilter(inputs(SAT_SHAPE, dev), level)
    rc, o, bufs = scores_abi(dev, x, 0.1)
    assert rc == 0 and all(torch.isfinite(o[k]).all() and bands_intact(bufs[k]) for k in o)
    maps = (o["pm0"].reshape(Q, Vn, L, L).cpu(), o["ps0"].reshape(Q, Vn, L).cpu(), o["pe0"].reshape(Q, Vn, L).cpu())
    for m, valid in zip(maps, (x["mm"].cpu(), x["lm"].cpu(), x["lm"].cpu())):
        keep = valid.unsqueeze(0).expand_as(m)
        assert bool((m[~keep].view(torch.int32) == 0).all())
        zz = z.view(Q, Vn, *([1] * (m.dim() - 2))).expand_as(m)
        assert bool((m[keep & (zz >= 20)] == 1.0).all()) and bool((m[keep & (zz <= -110)] == 0.0).all())
    want, ref32 = references(x, 0.1)
    tag = f"prefilter_scores {level}"
    gate(tag + " pm0", maps[0], want[3], ref32[3])
    gate(tag + " ps0", maps[1], want[4], ref32[4])
    gate(tag + " pe0", maps[2], want[5], ref32[5])
    gate(tag + " score", o["score"], want[0], ref32[0])
    gate(tag + " pool.m", o["pool"][..., 0], want[1][..., 0], ref32[1][..., 0])
    gate(tag + " pool.sum", o["pool"][..., 1], want[1][..., 1], ref32[1][..., 1])


@pytest.mark.gpu
def test_prefilter_scores_workspace_and_rejections(dev):
    x = inputs(SHAPES[1], dev)
    Q, Vn, T, L, C, D = x["shape"]
    rc, o, bufs = scores_abi(dev, x, 0.1)                                            # a workspace of exactly smin_prefilter_ws_bytes
    assert rc == 0 and torch.isfinite(o["score"]).all()
    rc, o, bufs = scores_abi(dev, x, 0.1, ws_delta=-1)
    assert rc != 0 and untouched(o, bufs), "one byte less"
    bad = [dict(Q=0), dict(V=0), dict(Q=65536), dict(L=0), dict(L=65), dict(T=L - 1), dict(T=2049), dict(C=0), dict(D=0), dict(D=18), dict(D=-4),
           dict(tau=0.0), dict(tau=-1.0), dict(tau=float("nan")), dict(tau=float("inf")), dict(ws=None), dict(ws_bytes=0),
           dict(pm0=None), dict(ps0=None), dict(pe0=None), dict(pm0=None, ps0=None)]
    bad += [{name: None} for name in ("fv", "fs", "w", "b", "lmask", "mm", "score", "pool", "cells")]
    for kw in bad:
        rc, o, bufs = scores_abi(dev, x, kw.get("tau", 0.1), **{k: v for k, v in kw.items() if k != "tau"})
        assert rc != 0, kw
        assert untouched(o, bufs), kw


@pytest.mark.gpu
@pytest.mark.parametrize("Vn", [1, 5, 300, 2500])
def test_prefilter_select_kernel(dev, Vn):
    """ranks from smin_video_rank on scores with ties and non-candidates; 300 and 2500 lie past the scan's tile of 256 videos"""
    A = V()
    L_ = A._lib
    Q = 5
    g = torch.Generator().manual_seed(Vn)
    score = torch.randint(0, 6, (Q, Vn), generator=g).float() / 4                    # six values: ties everywhere
    cells = (torch.rand(Q, Vn, generator=g) < 0.8).float() * 3
    cells[1] = 0                                                                     # a query without a candidate
    cells[2] = 0
    cells[2, Vn // 2] = 1                                                            # ... and one with a single candidate
    video = torch.arange(Vn, dtype=torch.int32).repeat(Q).to(dev)
    ptr = (torch.arange(Q + 1, dtype=torch.int32) * Vn).to(dev)
    vr = A.rank_videos(score.reshape(-1).to(dev), cells.reshape(-1).to(dev), video, ptr, n=1)
    rank = vr["pair_rank"].reshape(Q, Vn)
    assert torch.equal(rank.cpu(), A.rank_videos_torch(score.reshape(-1), cells.reshape(-1), video.cpu(), ptr.cpu(), n=1)["pair_rank"].reshape(Q, Vn))
    assert rank[1].eq(-1).all() and int(rank[2].ge(0).sum()) == 1
    for M in (1, 3, Vn, Vn + 7):
        Ms = min(M, Vn)
        want_v, want_q = A.prefilter_select_torch(rank.cpu(), M)
        loop_v, loop_q = select_loop(rank.cpu().tolist(), M)
        assert want_v.tolist() == loop_v and want_q.tolist() == loop_q
        got_v, got_q = A.prefilter_select(rank, M)
        assert got_v.dtype == torch.int32 and tuple(got_v.shape) == (Q, Ms)
        assert torch.equal(got_v.cpu(), want_v) and torch.equal(got_q.cpu(), want_q), (Vn, M)
        # through the C ABI with sentinels behind the outputs, twice
        for fill in (-9, 123456):
            bv = torch.full((Q * Ms + BAND,), fill, dtype=torch.int32, device=dev)
            bq = torch.full((Q * Ms + BAND,), fill, dtype=torch.int32, device=dev)
            rc = L_.load().smin_prefilter_select(L_.stream(), L_.ptr(rank), Q, Vn, M, L_.ptr(bv), L_.ptr(bq))
            torch.cuda.synchronize()
            assert rc == 0
            assert torch.equal(bv[:Q * Ms].cpu().reshape(Q, Ms), want_v) and torch.equal(bq[:Q * Ms].cpu().reshape(Q, Ms), want_q)
            assert bv[Q * Ms:].eq(fill).all() and bq[Q * Ms:].eq(fill).all()
    out = torch.full((Q * Vn,), -9, dtype=torch.int32, device=dev)
    lib = L_.load()
    for args in ((None, Q, Vn, 1, L_.ptr(out), L_.ptr(out)), (L_.ptr(rank), 0, Vn, 1, L_.ptr(out), L_.ptr(out)), (L_.ptr(rank), Q, 0, 1, L_.ptr(out), L_.ptr(out)),
                 (L_.ptr(rank), Q, Vn, 0, L_.ptr(out), L_.ptr(out)), (L_.ptr(rank), Q, Vn, 1, None, L_.ptr(out)), (L_.ptr(rank), Q, Vn, 1, L_.ptr(out), None)):
        assert lib.smin_prefilter_select(L_.stream(), *args) != 0
    torch.cuda.synchronize()
    assert out.eq(-9).all()


@pytest.fixture(scope="module")
def world(dev):
    """the tiny model; the ragged corpus of test_pair_training with a video without rows (V = 5, Q = 4), a corpus of equal videos, and
    the small window corpus of test_window_search -- all as banks"""
    m, _ = tiny_model(dev)

    def banks(snips):
        vid, qry, _ = corpus_inputs(snips=snips)
        vid_d, qry_d = {k: v.to(dev) for k, v in vid.items()}, {k: v.to(dev) for k, v in qry.items()}
        return (m.encode_videos(vid_d["video_features"], vid_d["video_mask"], vid_d["length_mask"], vid_d["moment_mask"]),
                m.encode_queries(qry_d["query_features"], qry_d["query_mask"]))

    vb, qb = banks(NO_ROWS)
    evb, eqb = banks((8, 8, 8, 8, 8))
    raw, qf, qm = WS.corpus_rows(WS.SEED)
    wqb = m.encode_queries(qf.to(dev), qm.to(dev))
    wb = m.encode_windows(raw.to(dev), WS.LENGTHS, WS.WINDOW, WS.STRIDE)
    return dict(m=m, vb=vb, qb=qb, evb=evb, eqb=eqb, wb=wb, wqb=wqb)


def model_heads(m):
    lo, D = m.localization, TINY_SHAPE[3]
    hs = (lo.conv_layer_pm, lo.conv_layer_ps, lo.conv_layer_pe)
    return torch.stack([h.weight.detach().reshape(D) for h in hs]), torch.cat([h.bias.detach().reshape(1) for h in hs])


@pytest.mark.gpu
def test_prefilter_videos(dev, world):
    A = V()
    m, vb, qb = world["m"], world["vb"], world["qb"]
    T, L, C, D = TINY_SHAPE[:4]
    Q, Vn = len(qb), len(vb)
    assert vb.cell_counts == (36, 1, 0, 36, 6) and vb.fv is not None and qb.fs is not None
    w, b = model_heads(m)
    score, pool, cells = A.prefilter_scores(vb.fv, qb.fs, w, b, vb.length_mask, vb.moment_mask, T, L, C, 0.1)
    video_of = torch.arange(Vn, dtype=torch.int32).repeat(Q)
    ptr = torch.arange(Q + 1, dtype=torch.int32) * Vn
    gt = [g % Vn for g in GT_VIDEO]                                                  # [2, 0, 3, 1]: query 0's own video has no rows
    for M in (1, 2, 3, Vn, Vn + 4):
        Ms = min(M, Vn)
        r = m.prefilter_videos(vb, qb, M, gt_video=gt)
        assert set(r) == {"video", "score", "rank", "gt_rank", "video_index", "query_index"}
        assert torch.equal(bits(r["score"]), bits(score))
        want = A.rank_videos_torch(score.reshape(-1).cpu(), cells.reshape(-1).cpu(), video_of, ptr, n=1, gt_video=torch.tensor(gt))
        assert r["rank"].dtype == torch.int32 and torch.equal(r["rank"].cpu(), want["pair_rank"].reshape(Q, Vn))
        assert r["rank"][:, 2].eq(-1).all() and torch.equal(r["gt_rank"].cpu(), want["gt_rank"]) and r["gt_rank"][0].item() == -1
        sel_v, sel_q = A.prefilter_select_torch(r["rank"].cpu(), M)
        assert r["video"].dtype == torch.int64 and torch.equal(r["video"].cpu(), sel_v.long())
        assert (r["video"][:, 1:] > r["video"][:, :-1]).all()
        assert torch.equal(r["video_index"].cpu(), sel_v.reshape(-1)) and torch.equal(r["query_index"].cpu(), sel_q.reshape(-1))
        # VR@Ms is the share of queries whose own video survives (as a candidate: a filler has no rank)
        meter = A.VideoRankMeter(n=(Ms,), device=dev)
        meter.update(r["gt_rank"])
        inside = [gt[q] in r["video"][q].tolist() and cells[q, gt[q]].item() > 0 for q in range(Q)]
        assert meter.result()[f"VR@{Ms}"] == sum(inside) / Q
    assert m.prefilter_videos(vb, qb, 2)["gt_rank"].tolist() == [-1] * Q
    # a WindowBank: group_pool of the kernel's per-window pools
    wb, wqb = world["wb"], world["wqb"]
    Qw, W, Vw = len(wqb), len(wb), wb.n_videos
    assert W == 8 and Vw == 5
    _, wpool, wcells = A.prefilter_scores(wb.fv, wqb.fs, w, b, wb.length_mask, wb.moment_mask, T, L, C, 0.1)
    gp = torch.tensor([q * W + int(wb.video_ptr[v]) for q in range(Qw) for v in range(Vw)] + [Qw * W], dtype=torch.int32, device=dev)
    gs, gc = A.group_pool(wpool.reshape(-1, 2), wcells.reshape(-1), gp, 0.1)
    r = m.prefilter_videos(wb, wqb, 2, gt_video=[0] * Qw)
    assert set(r) == {"video", "score", "rank", "gt_rank"}
    assert torch.equal(bits(r["score"]), bits(gs.reshape(Qw, Vw))) and r["rank"][:, 3].eq(-1).all()       # video 3 has no rows
    wv = torch.arange(Vw, dtype=torch.int32).repeat(Qw)
    want = A.rank_videos_torch(gs.cpu(), gc.cpu(), wv, torch.arange(Qw + 1, dtype=torch.int32) * Vw, n=1)
    assert torch.equal(r["rank"].cpu(), want["pair_rank"].reshape(Qw, Vw))
    assert torch.equal(r["video"].cpu(), A.prefilter_select_torch(r["rank"].cpu(), 2)[0].long())
    with pytest.raises(ValueError, match="prefilter"):
        m.search(wb, wqb, prefilter=2)
    # a bank encoded off the one-node path: score_pairs' error
    off = A.VideoBank(None, vb.video_features, vb.video_mask, vb.length_mask, vb.moment_mask, vb.cell_counts)
    with pytest.raises(ValueError, match="off the one-node path"):
        m.prefilter_videos(off, qb, 2)


@pytest.mark.gpu
@pytest.mark.parametrize("M", [1, 2, 5])
def test_search_prefilter_is_search_on_the_surviving_pairs(dev, world, M):
    m, vb, qb = world["m"], world["vb"], world["qb"]
    Q, Vn = len(qb), len(vb)
    gt = [g % Vn for g in GT_VIDEO]
    duration = torch.tensor([10.0, 3.5, 60.0, 7.25, 100.0], device=dev)
    pf = m.prefilter_videos(vb, qb, M, gt_video=gt)
    for kw in (dict(), dict(video_weight=7.5, max_videos=2, gt_video=gt), dict(max_batch=3), dict(max_batch=3, video_weight=7.5, max_videos=2)):
        base = dict(k=5, k_video=3, duration=duration, **kw)
        got = m.search(vb, qb, prefilter=M, **base)
        assert torch.equal(got["prefilter_video"], pf["video"]) and torch.equal(bits(got["prefilter_score"]), bits(pf["score"]))
        assert got["prefilter_gt_rank"].tolist() == (pf["gt_rank"].tolist() if "gt_video" in kw else [-1] * Q)
        want = m.search(vb, qb, pairs=host_pairs(got["prefilter_video"]), **base)
        assert set(got) == set(want) | {"prefilter_video", "prefilter_score", "prefilter_gt_rank"}
        same(got, want, SEARCH_KEYS, (M, kw))
        assert torch.equal(torch.isnan(got["times"]), torch.isnan(want["times"]))
        assert torch.equal(bits(torch.nan_to_num(got["times"])), bits(torch.nan_to_num(want["times"])))
        if "video_weight" in kw:
            same(got, want, ("video_rank", "video_score", "video_count", "gt_rank"), (M, kw))
        for q in range(Q):
            assert set(got["video"][q, :int(got["count"][q])].tolist()) <= set(got["prefilter_video"][q].tolist())
        if M == 5:                                                                   # every video survives: today's search
            same(got, m.search(vb, qb, **base), SEARCH_KEYS + (("video_rank", "video_score", "video_count", "gt_rank") if "video_weight" in kw else ()),
                 "prefilter=V")
    assert m.known_cell_count is None


@pytest.mark.gpu
def test_search_prefilter_reads_nothing_back(dev, world):
    m, vb, qb = world["m"], world["evb"], world["eqb"]
    assert vb.cell_counts == (36,) * 5
    kw = dict(k=5, k_video=3, max_batch=3, prefilter=2, duration=torch.ones(5, device=dev))
    first = m.search(vb, qb, **kw)                                                   # first use outside the checked region
    weighted = m.search(vb, qb, video_weight=7.5, max_videos=1, gt_video=[0, 1, 2, 3], **kw)
    torch.cuda.synchronize()
    mode = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        second = m.search(vb, qb, **kw)
        second_w = m.search(vb, qb, video_weight=7.5, max_videos=1, gt_video=[0, 1, 2, 3], **kw)
        m.prefilter_videos(vb, qb, 2, gt_video=[0, 1, 2, 3])
    finally:
        torch.cuda.set_sync_debug_mode(mode)
    same(second, first, SEARCH_KEYS + ("prefilter_video", "prefilter_score"), "second run")
    same(second_w, weighted, SEARCH_KEYS + ("video_rank", "gt_rank", "prefilter_gt_rank"), "second weighted run")
    assert int(V()._lib.load_torch().layout_status(dev)[0]) == 0                     # the handed-over counts matched the masks
    want = m.search(vb, qb, pairs=host_pairs(first["prefilter_video"]), k=5, k_video=3, max_batch=3)
    same(first, want, SEARCH_KEYS, "equal videos")
    # unequal cell_counts: no count is handed over, the node reads it; the same bits
    rb = world["vb"]
    got = m.search(rb, world["qb"], k=5, k_video=3, max_batch=3, prefilter=2)
    same(got, m.search(rb, world["qb"], pairs=host_pairs(got["prefilter_video"]), k=5, k_video=3, max_batch=3), SEARCH_KEYS, "ragged videos")


@pytest.mark.gpu
def test_search_without_prefilter_is_unchanged(dev, world):
    """prefilter=None: the plain search against search_torch fed score_pairs, as tests/test_corpus_search.py compares it"""
    m, vb, qb = world["m"], world["vb"], world["qb"]
    scorer = lambda vi, qi: m.score_pairs(vb, qb, vi, qi)
    for kw in (dict(k=5, k_video=3, max_batch=7), dict(k=5, k_video=3, max_batch=64, pairs=np.array([(3, 4), (0, 2), (3, 0), (2, 1), (0, 0)]))):
        got = m.search(vb, qb, prefilter=None, **kw)
        want = m.search_torch(vb, qb, scorer=scorer, **kw)
        assert set(got) == set(want) == set(SEARCH_KEYS)
        same(got, {k: v.to(dev) for k, v in want.items()}, SEARCH_KEYS, kw)
        same(got, m.search(vb, qb, **kw), SEARCH_KEYS, "the default")
