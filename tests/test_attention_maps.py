"""Every SMI layer's word-attention maps (SMIN.keep_attention, SMIN.localize(attention=True)) against the reference's own
``attn_weights`` (tests/golden/ga_*.npz, tests/golden/make_golden_attn.py), the C ABI's probability store over the whole
attention dispatch against a float64 restatement, and the promise that recording the maps changes no bit of the step."""
import ctypes
import math

import pytest
import torch

from tests import helpers as H
from tests.support.device import dev  # noqa: F401  (the module's device fixture)
from tests.support.references import _attn_inputs, _layout_to, _ragged_mask, attn_form, ALL_FORMS

ATTN_FIXTURES = ["ga_ragged", "ga_r2", "ga_c3_q18"]
MAP_TOL = 1e-5


def probs_ref(chat, cells, C, Mq, uq, qmask):
    """ContentAttention's word weights (models.py:213-224) of every packed row, float64: chat [N*C, dl] with cells [N, 4] sorted by
    sample; S = (X Mq_b^T + uq_b) / sqrt(dl), S = S * qm, S[qm == 0] = -1e9, softmax over words.  [N*C, Nq]."""
    dl = chat.shape[1]
    b_row = cells[:, 0].long().repeat_interleave(C)
    S = (torch.einsum("rd,rwd->rw", chat, Mq[b_row]) + uq[b_row]) / math.sqrt(dl)
    qm = qmask[b_row]
    return torch.softmax((S * qm).masked_fill(qm == 0, -1e9), dim=-1)


def dense_ref(probs, cells, cellmap, C, uq, qmask, dl):
    """The dense (B, L, L, C, Nq) map: listed cells with m == 1 copy their rows, every other cell softmax(mask(uq_b / sqrt(dl)))."""
    B, L, _ = cellmap.shape
    Nq = uq.shape[1]
    s = (uq / math.sqrt(dl) * qmask).masked_fill(qmask == 0, -1e9)
    out = torch.softmax(s, dim=-1).view(B, 1, 1, 1, Nq).expand(B, L, L, C, Nq).clone()
    n = cellmap.long()
    listed = n >= 0
    listed[listed.clone()] = cells[n[listed], 3] != 0
    out[listed] = probs.view(-1, C, Nq)[n[listed]]
    return out


def _load(name):
    z = H.load_npz(name)
    cfg, sd, batch, out, _, _ = H.split_tiny(_TinyView(z))
    maps = {k[5:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("attn/")}
    return cfg, sd, batch, out, maps


class _TinyView(dict):
    """split_tiny's view of an attention fixture (it has no loss / gradients)."""

    def __init__(self, z):
        super().__init__({k: z[k] for k in z.files})
        self["loss"] = 0.0
        self.files = list(self.keys())


def _model(cfg, sd, dev, native):
    import models
    c = cfg
    m = models.SMIN(c["T"], c["L"], c["C"], c["D"], c["dl"], c["layers"], c["Din"], c["Nq"], c["H"], dev)
    m.load_state_dict(sd)
    m = m.to(dev)
    m.fused_core = native
    return m


# ---------------------------------------------------------------- CPU

def test_fixtures_hold_the_reference_maps():
    """The fixtures' maps have the reference's shapes, sum to 1 over words, and a sample's masked cells share one row."""
    for name in ATTN_FIXTURES:
        cfg, _, batch, _, maps = _load(name)
        B, L, C, Nq = cfg["B"], cfg["L"], cfg["C"], cfg["Nq"]
        for k in range(cfg["layers"]):
            cw, bw = maps[f"content{k}"], maps[f"boundary{k}"]
            assert cw.shape == (B, L, L, C, Nq) and bw.shape == (B, L, Nq)
            assert torch.allclose(cw.double().sum(-1), torch.ones(()).double(), atol=1e-5)
            mm = batch["moment_mask"]
            for b in range(B):
                rows = cw[b][~mm[b]].reshape(-1, Nq)
                assert rows.shape[0] > 0                          # every sample has masked cells (j < i at least)
                assert (rows - rows[:1]).abs().max().item() <= 1e-6


def test_forward_with_attention_operator_is_registered():
    import models
    ops = models.vml_amd._lib.load_torch()
    schema = str(ops.smin_forward.default._schema)
    assert schema.split("->")[1].count("Tensor[]") == 2, schema
    assert "str? attention" in schema, schema


def test_captured_step_refuses_keep_attention():
    import models
    from vml_amd.training import CapturedStep
    m = models.SMIN(32, 8, 4, 32, 16, 2, 24, 5, 16)
    m.keep_attention = True
    step = CapturedStep(m)
    with pytest.raises(RuntimeError, match="keep_attention"):
        step({k: torch.zeros(1) for k in ("moment_mask",)})


# ---------------------------------------------------------------- GPU: against the reference

@pytest.mark.gpu
@pytest.mark.parametrize("native", [True, False], ids=["one_node", "python_host"])
@pytest.mark.parametrize("name", ATTN_FIXTURES)
def test_maps_match_reference(dev, name, native):
    cfg, sd, batch, out, maps = _load(name)
    m = _model(cfg, sd, dev, native)
    for smi in m.smis:
        assert smi.content_unit.attn_layer.attn_weights is None and smi.boundary_unit.attn_layer.attn_weights is None
    m.keep_attention = True
    with torch.no_grad():
        pm, _, _, _ = m(*H.model_inputs(batch, dev))
    assert (pm.cpu() - out["pm"]).abs().max().item() < 1e-4
    qm = batch["query_mask"].reshape(cfg["B"], -1).bool()
    for k, smi in enumerate(m.smis):
        cw, bw = smi.content_unit.attn_layer.attn_weights, smi.boundary_unit.attn_layer.attn_weights
        assert cw is not None and bw is not None, f"layer {k}: attn_weights not set"
        assert not cw.requires_grad and not bw.requires_grad and cw.is_cuda
        ec = (cw.cpu() - maps[f"content{k}"]).abs().max().item()
        eb = (bw.cpu() - maps[f"boundary{k}"]).abs().max().item()
        print(name, "native" if native else "python", "layer", k, "content", ec, "boundary", eb)
        assert ec <= MAP_TOL and eb <= MAP_TOL, (k, ec, eb)
        c = cw.cpu()
        pad = ~qm.view(cfg["B"], 1, 1, 1, -1).expand_as(c)
        assert (c[pad] == 0).all(), "padded words must get exactly 0"
        assert (c.double().sum(-1) - 1).abs().max().item() < 1e-5


@pytest.mark.gpu
def test_hosts_agree(dev):
    cfg, sd, batch, _, _ = _load("ga_r2")
    got = []
    for native in (True, False):
        m = _model(cfg, sd, dev, native)
        m.keep_attention = True
        with torch.no_grad():
            m(*H.model_inputs(batch, dev))
        got.append([(s.content_unit.attn_layer.attn_weights, s.boundary_unit.attn_layer.attn_weights) for s in m.smis])
    for (c0, b0), (c1, b1) in zip(*got):
        assert (c0 - c1).abs().max().item() <= 1e-6 and (b0 - b1).abs().max().item() <= 1e-6


# ---------------------------------------------------------------- GPU: the C ABI over the whole dispatch

def _probs_cases():
    cases = [(4, dl, nq) for dl in (16, 32, 64) for nq in (13, 20)]
    cases += [(4, 128, nq) for nq in (13, 18, 24, 32)]
    cases += [(c, dl, nq) for c in (2, 3) for dl in (16, 32, 64, 128) for nq in (13, 20)]
    cases += [(4, 96, nq) for nq in (13, 20)]
    return cases


PROBS_CASES = _probs_cases()


def test_probs_cases_reach_every_form():
    assert {attn_form(*c) for c in PROBS_CASES} == set(ALL_FORMS)


@pytest.mark.gpu
@pytest.mark.parametrize("C,dl,Nq", PROBS_CASES, ids=[f"C{c}-dl{d}-Nq{q}" for c, d, q in PROBS_CASES])
def test_content_attn_fwd_probs(dev, C, dl, Nq):
    """smin_content_attn_fwd_probs: probs against probs_ref; cc / ccmean bit-identical to smin_content_attn_fwd (fp32 rows,
    no rows, rows only) and to smin_content_attn_fwd_cch (bf16 rows); the dense expansion against dense_ref."""
    from vml_amd._lib import call, ptr, stream
    from vml_amd.functional import content_attn_maps_dense
    g = torch.Generator().manual_seed(1000 * C + 10 * dl + Nq)
    lay, x = _attn_inputs(C, dl, Nq, _ragged_mask(5, 12, g), all_cells=False, seed=dl + Nq)
    ld = _layout_to(lay, dev)
    d = {k: v.float().to(dev).contiguous() for k, v in x.items()}
    N, B = lay.N, 5
    ref = probs_ref(x["chat"], lay.cells, C, x["Mq"], x["uq"], x["qmask"])
    args = lambda: (stream(), ptr(d["chat"]), ptr(ld.cells), ptr(ld.row_ptr), N, B, ld.L, C, dl, Nq, ptr(d["Mq"]), ptr(d["uq"]), ptr(d["what"]),
                    ptr(d["shat"]), ptr(d["qmask"]))
    for rows, mean in ((True, True), (False, True), (True, False)):
        cc0, m0 = torch.full((N * C, dl), 7.0, device=dev), torch.full((N, dl), 7.0, device=dev)
        cc1, m1 = cc0.clone(), m0.clone()
        probs = torch.full((N * C, Nq), float("nan"), device=dev)
        call("smin_content_attn_fwd", *args(), ptr(cc0) if rows else None, ptr(m0) if mean else None)
        call("smin_content_attn_fwd_probs", *args(), ptr(cc1) if rows else None, 0, ptr(m1) if mean else None, ptr(probs))
        assert torch.equal(cc0, cc1) and torch.equal(m0, m1), (rows, mean)
        err = (probs.double().cpu() - ref).abs().max().item()
        assert err <= 2e-6, (rows, mean, err)
        pad = (x["qmask"][lay.cells[:, 0].long().repeat_interleave(C)] == 0) & (x["qmask"][lay.cells[:, 0].long().repeat_interleave(C)].sum(1, keepdim=True) > 0)
        assert (probs.cpu()[pad] == 0).all()
    h0, h1 = torch.zeros((N * C, dl), dtype=torch.bfloat16, device=dev), torch.ones((N * C, dl), dtype=torch.bfloat16, device=dev)
    m0, m1 = torch.zeros((N, dl), device=dev), torch.ones((N, dl), device=dev)
    probs_h = torch.empty((N * C, Nq), device=dev)
    bf = lambda t: ctypes.c_void_p(t.data_ptr())                   # (bf16 rows: ptr() takes the fp32 / integer tensors only)
    call("smin_content_attn_fwd_cch", *args(), bf(h0), ptr(m0))
    call("smin_content_attn_fwd_probs", *args(), bf(h1), 1, ptr(m1), ptr(probs_h))
    assert torch.equal(h0, h1) and torch.equal(m0, m1) and torch.equal(probs_h, probs)
    dense = content_attn_maps_dense(probs, ld, d["uq"], d["qmask"], C, dl).cpu().double()
    dref = dense_ref(probs.cpu().double(), lay.cells, lay.cellmap, C, x["uq"], x["qmask"], dl)
    assert (dense - dref).abs().max().item() <= 1e-6


@pytest.mark.gpu
def test_content_attn_fwd_probs_refusals(dev):
    from vml_amd._lib import SminHipError, call, ptr, stream
    C, dl, Nq = 4, 32, 7
    g = torch.Generator().manual_seed(3)
    lay, x = _attn_inputs(C, dl, Nq, _ragged_mask(2, 6, g), all_cells=False, seed=3)
    ld = _layout_to(lay, dev)
    d = {k: v.float().to(dev).contiguous() for k, v in x.items()}
    m = torch.empty((lay.N, dl), device=dev)
    a = (stream(), ptr(d["chat"]), ptr(ld.cells), ptr(ld.row_ptr), lay.N, 2, ld.L, C, dl, Nq, ptr(d["Mq"]), ptr(d["uq"]), ptr(d["what"]),
         ptr(d["shat"]), ptr(d["qmask"]))
    with pytest.raises(SminHipError):
        call("smin_content_attn_fwd_probs", *a, None, 0, ptr(m), None)           # no probs
    with pytest.raises(SminHipError):
        call("smin_content_attn_fwd_probs", *a, None, 1, ptr(m), ptr(m))         # bf16 rows without rows


# ---------------------------------------------------------------- GPU: nothing perturbed, retrieval, refusals

def _step(m, b):
    from vml_amd import loss_fn
    m.zero_grad(set_to_none=True)
    out = m(*H.model_inputs(b))
    loss = loss_fn(out[0], b["ym"], b["sm"], b["moment_mask"], out[1], b["ys"], b["ss"], out[2], b["ye"], b["se"], out[3], b["ya"], b["length_mask"])
    loss.backward()
    torch.cuda.synchronize()
    return [t.detach().clone() for t in out] + [loss.detach().clone()], {k: p.grad.clone() for k, p in m.named_parameters()}


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["f32", "bf16"])
@pytest.mark.parametrize("native", [True, False], ids=["one_node", "python_host"])
def test_keep_attention_changes_no_bit(dev, mode, native):
    import models
    from oracle import smin_oracle as O
    cfg, sd, _, _, _ = _load("ga_ragged")
    c = cfg
    batch = O.synthetic_batch(c["B"], c["T"], c["L"], c["Nq"], c["Din"], seed=121)
    b = {k: v.to(dev) for k, v in batch.items()}
    m = _model(cfg, sd, dev, native)
    m.bf16_operand_storage = True
    models.vml_amd.set_gemm_mode(mode)
    try:
        runs = []
        for keep in (False, True, False):
            m.keep_attention = keep
            runs.append(_step(m, b))
    finally:
        models.vml_amd.set_gemm_mode(models.vml_amd._lib.DEFAULT_GEMM_MODE)
    assert m.smis[0].content_unit.attn_layer.attn_weights is not None
    for outs, grads in runs[1:]:
        for t0, t1 in zip(runs[0][0], outs):
            assert torch.equal(t0, t1)
        for k, g0 in runs[0][1].items():
            assert torch.equal(g0, grads[k]), k


@pytest.mark.gpu
@pytest.mark.parametrize("native", [True, False], ids=["one_node", "python_host"])
def test_localize_attention_gathers_the_dense_maps(dev, native):
    cfg, sd, batch, _, _ = _load("ga_ragged")
    m = _model(cfg, sd, dev, native)
    inputs = H.model_inputs(batch, dev)
    k = 40                                                        # more than any sample's valid cells: empty slots
    r = m.localize(*inputs, k=k, nms_thresh=0.7, attention=True)
    r0 = m.localize(*inputs, k=k, nms_thresh=0.7)
    assert torch.equal(r["idx"], r0["idx"]) and torch.equal(r["score"], r0["score"])
    m.keep_attention = True
    with torch.no_grad():
        m(*inputs)
    B, L, C, Nq, nl = cfg["B"], cfg["L"], cfg["C"], cfg["Nq"], cfg["layers"]
    ca, ba = r["content_attention"].cpu(), r["boundary_attention"].cpu()
    assert ca.shape == (B, k, nl, C, Nq) and ba.shape == (B, k, nl, 2, Nq)
    idx = r["idx"].cpu()
    for l, smi in enumerate(m.smis):
        cw, bw = smi.content_unit.attn_layer.attn_weights.cpu(), smi.boundary_unit.attn_layer.attn_weights.cpu()
        for b in range(B):
            for s in range(k):
                i, j = int(idx[b, s, 0]), int(idx[b, s, 1])
                if i < 0:
                    assert (ca[b, s, l] == 0).all() and (ba[b, s, l] == 0).all()
                    continue
                assert torch.equal(ca[b, s, l], cw[b, i, j]), (b, s, l)
                assert torch.equal(ba[b, s, l, 0], bw[b, i]) and torch.equal(ba[b, s, l, 1], bw[b, j])
    assert (idx[..., 0] < 0).any(), "the case should leave empty slots"


@pytest.mark.gpu
def test_paths_without_maps_refuse(dev):
    cfg, sd, batch, _, _ = _load("ga_ragged")
    m = _model(cfg, sd, dev, False)
    m.content_stream = False                                      # the units as written (ContentUnitFn)
    m.keep_attention = True
    with pytest.raises(RuntimeError, match="cannot deliver"):
        m(*H.model_inputs(batch, dev))
    with pytest.raises(RuntimeError, match="cannot deliver"):
        m.localize(*H.model_inputs(batch, dev), attention=True)


@pytest.mark.gpu
def test_standalone_attention_records_weights(dev):
    import models
    torch.manual_seed(0)
    at, ca = models.Attention(16).to(dev), models.ContentAttention(16).to(dev)
    q, kv = torch.randn(2, 5, 16, device=dev), torch.randn(2, 6, 16, device=dev)
    mask = torch.tensor([[1] * 6, [1] * 4 + [0] * 2], device=dev).view(2, 6, 1)
    at(q, kv, kv, mask)
    assert at.attn_weights is None                                # off by default
    at.keep_weights = ca.keep_weights = True
    at(q, kv, kv, mask)
    ca(torch.randn(2, 3, 3, 4, 16, device=dev), kv, kv, mask)
    assert at.attn_weights.shape == (2, 5, 6) and ca.attn_weights.shape == (2, 3, 3, 4, 6)
    assert (at.attn_weights[1, :, 4:] == 0).all() and (ca.attn_weights[1, ..., 4:] == 0).all()
    assert torch.allclose(at.attn_weights.sum(-1), torch.ones(2, 5, device=dev))
