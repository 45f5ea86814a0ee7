"""The gated moment feature (csrc/gate.hip: smin_gate_fwd, smin_gate_fwd_sum, smin_gate_bwd), the content unit as written
(csrc/content_unit.hip: smin_content_unit_fwd / _bwd with their own GEMM epilogues and virtual operands) and the training loss
(csrc/loss.hip: smin_loss_fwd / _bwd) against float64 restatements of the reference's formulas.

CPU: each restatement is pinned to the oracle (oracle/smin_oracle.py) at 1e-12, and Python mirrors of the launch arithmetic show that
the GPU case lists reach every form listed below (test_gate_cases_reach_every_form, test_content_unit_cases_reach_every_form,
test_loss_cases_plant_every_edge).
GPU: every case goes through the C ABI into NaN-prefilled outputs and a NaN-prefilled workspace of exactly the documented size,
every return code is checked, every output and gradient is compared with float64, and every backward runs twice, bit for bit.

Forms reached
  gate      one chunk, 2..7 chunks (fewer than the reducer's 8 phases), more than 8, the capped chunk count (L = 130: 498 chunks of 34
            cells where cdiv(L^2, 32) = 529), a sample with no cell between two that have cells, samples with fewer live chunks than
            max_chunks (the rest of their partial rows stays NaN), chunk tails of 1, 2, 3 and 0 cells modulo 4 (the clamped four-cell
            trip), D = 512 (one full trip of the d loop), D < 512, D = 1056 (three trips, the last partial), one and two reducer
            column blocks (D / 4 = 65), n_dhbar 1..4, n_dres 0 / 1 / 2 / 4, the boundary term on and off (on a triangular and on a
            non-triangular cell list), a forward grid whose last workgroup is partly idle, smin_gate_fwd_sum, and the refusals.
  content   C = 2, 3, 4 (the quad epilogues EpContentOut4 / EpAddDout4, and clip_mean_kernel / dout_sum_kernel for C != 4), last = 0
            with dfc_out, last = 0 with dfc_out = NULL (EpAddDout<false>, DoutEffMat<true, false>), last = 1 (EpLastMean, MaskedRowsMat,
            EpScale on N rows), from_mask and all_cells lists (masked cells listed), dl = 16 / 48 / 128 (and 32), D = 104 and 132
            (D % 64 != 0, the second column tile 4 wide), mini tiles and 128-row main tiles for EpBiasMask, EpContentOut,
            EpContentOut4, EpPlain over DoutEffMat, EpAddDout and EpAddDout4, one and several row splits of both weight-gradient
            contractions, and gemm mode 3 (fp32 emulated on the bf16 matrix cores) on a mini and a main case.
  loss      probabilities at exactly 0 and 1 (the -100 log clamp, the 1e-12 gradient floor), at 1e-9 and 1 - 2^-24, under both labels,
            scale targets at exactly 0 and 1, L = 300 (a second trip of the boundary loop), L * L < 256, B = 37, mask bytes 7 and 255,
            the part[B][6] partials, and the autograd wrapper vml_amd.loss_fn bit for bit against the direct calls.

Saturated inputs (the project's gate e_kernel <= 32 * e_torch32 + 1e-6 in place of the fixed bounds; INTEGRATION.md "Saturated inputs")
  gate      pre-activations fm * fs at +-{20, 90, 200, 1e4}, on every element and on half of them, at D = 48, D = 1056 and on the
            non-triangular all_cells list.
  loss      on the (5, 16) case, the mask bytes 7 / 255 and L = 300: p at 0, fp32's smallest denormal, 1e-30, 0.5, 1 - 2^-24 and 1 under both labels and the scale targets 0, 0.3, 1, in all four
            heads, the gradients gated per (head, p, label) group.

Left to other suites
  EpLastMean (and EpScale over MaskedRowsMat) on 128-row main tiles need more than 32 768 cells: the tile bodies are the engine
  tests' (tests/test_gemm_engine.py), the epilogue is covered here on mini tiles.  Gemm modes 1 and 2 stay with the whole-model tests
  (tests/test_hip_parity.py), the attention core's dispatch table with tests/test_attention_core.py, samples with no valid cell or
  snippet (0 / 0 in the loss) with test_degenerate_samples_and_empty_batch, the metric kernels with the meter tests.

Worst error per family: no device figure is recorded yet -- no MI355X run of this module had been possible when it was written;
every GPU test prints its worst ratios (run with -s) for the first run to fill in here.  What is known is the error of an fp32
restatement of the same formulas against float64 on the CPU, over the case lists below (max |got - ref| / max |ref|; the loss
relative per value, partial and gradient element): gate hbar 9.2e-8, dfm 2.1e-7, dfs 3.5e-6; content unit forward 4.9e-7,
gradients 2.4e-6; loss value 1.0e-7, partials 1.3e-7, gradients 2.6e-7 -- at least 28 times inside every bound."""
import ctypes
import functools
import math

import pytest
import torch

from tests import helpers as H
from tests.support.device import dev  # noqa: F401  (the module's device fixture)
from tests.support.device import gemm_mode  # noqa: F401  (fixture)
from tests.support.compare import _assert_spread, _spread
from tests.support.guards import _nan, _ws_nan
from tests.support.references import (
    _attn_inputs, _layout_to, _smi_params, attn_core_ref, lengths_mask, make_layout, moment_mask, nt_form, tn_forms, word_side_ref,
    WORD_PARAM_NAMES)

FWD_TOL = 1e-5          # max |got - ref| / max |ref|, per output and case (tests/test_proposal_map.py, tests/test_attention_core.py)
GRAD_TOL = 1e-4
LOSS_TOL = 1e-5         # the loss value and each partial, relative; every gradient element, relative
PIN_TOL = 1e-12

cdiv = H.cdiv


# ---------------------------------------------------------------- float64 restatements

def gate_ref(fm, fs, cells, dh_list, dres_list, A=None, dout=None):
    """hbar = sigmoid(fm * fs[b]) * fm per cell of cells [N, 4] (reference models.py:191, 272-274), and the gradients smin_gate_bwd
    forms: those of   sum_k <hbar, dh_k> + sum_k <fm, dres_k> + <hbar, A[b, i, j] * dout[b, i, :]>   (the last term is the boundary
    unit's gated row reduction, models.py:191-194) with respect to fm [N, D] and fs [B, D], by autograd in the inputs' dtype.
    Returns (hbar, dfm, dfs)."""
    fm, fs = fm.detach().clone().requires_grad_(True), fs.detach().clone().requires_grad_(True)
    c = cells.long()
    hbar = torch.sigmoid(fm * fs[c[:, 0]]) * fm
    tot = sum((hbar * g).sum() for g in dh_list) + sum((fm * g).sum() for g in dres_list)
    if A is not None:
        tot = tot + (hbar * (A[c[:, 0], c[:, 1], c[:, 2]].unsqueeze(-1) * dout[c[:, 0], c[:, 1]])).sum()
    dfm, dfs = torch.autograd.grad(tot, (fm, fs))
    return hbar.detach(), dfm, dfs


def content_unit_ref(fc, hbar, cells, C, Wch, bch, Mq, uq, what, shat, qmask, Wc, bc, last, fcmean_in):
    """ContentUnit (reference models.py:242-276) on packed cells, fc [N, C, D], hbar [N, D], m = cells[:, 3]:
        chat = m (fc Wch^T + bch);  cc = attn_core_ref(chat, ..)
        not last:  fc_out = m (cc Wc^T + bc) + fc + hbar;  fcmean = mean_c fc_out;  cchat = cc [N*C, dl]
        last:      fcmean = m (mean_c cc . Wc^T + bc) + fcmean_in + hbar;  cchat = mean_c cc [N, dl];  no fc_out
    (fcmean_in is mean_c fc by contract: hand it in as fc.mean(1) of the same leaf for the gradient of fc).
    Returns a dict of chat, cchat, fc_out (None when last), fcmean and the word logits S [N, C, Nq]; differentiable."""
    N, _, D = fc.shape
    m = cells[:, 3].to(fc.dtype)
    mrow = m.repeat_interleave(C).view(-1, 1)
    chat = (fc.reshape(N * C, D) @ Wch.t() + bch) * mrow
    cc, ccmean, S = attn_core_ref(chat, cells, C, Mq, uq, what, shat, qmask)
    if last:
        fcmean = m.view(-1, 1) * (ccmean @ Wc.t() + bc) + fcmean_in + hbar
        return dict(chat=chat, cchat=ccmean, fc_out=None, fcmean=fcmean, S=S)
    fc_out = (mrow * (cc @ Wc.t() + bc)).reshape(N, C, D) + fc + hbar.unsqueeze(1)
    return dict(chat=chat, cchat=cc, fc_out=fc_out, fcmean=fc_out.mean(1), S=S)


def clip_logits(chat, S, cells, C, what, shat, qmask):
    """The clip softmax's logits q q^T / sqrt(dl) [N, C, C] of attn_core_ref, re-formed from its word logits S (for the spread guard)."""
    N, dl = cells.shape[0], chat.shape[1]
    b_of = cells[:, 0].long()
    qm = qmask[b_of].unsqueeze(1)
    P = torch.softmax((S * qm).masked_fill(qm == 0, -1e9), dim=-1)
    a = cells[:, 3].to(chat.dtype).view(-1, 1, 1) * (P @ what[b_of])
    q = chat.reshape(N, C, dl) * (a + shat[b_of].unsqueeze(1))
    return q @ q.transpose(1, 2) / math.sqrt(dl)


LOSS_KEYS = ("pm", "ym", "sm", "mm", "ps", "ys", "ss", "pe", "ye", "se", "pa", "ya", "lm")


def _bce(p, y):
    return -(y * torch.log(p).clamp(min=-100) + (1 - y) * torch.log(1 - p).clamp(min=-100))


def _scaled_bce(p, y, s):
    return (s * y) * _bce(p, y) + ((1 - s) * (1 - y)) * _bce(1 - p, 1 - y)


def loss_ref(pm, ym, sm, mm, ps, ys, ss, pe, ye, se, pa, ya, lm):
    """csrc/loss.hip's header (reference main.py:89-116) in the dtype of pm: L = L_m + L_s + L_e + 0.5 L_a, each term the mean over
    samples of (sum of masked elements / number of valid ones), the logs clamped at -100.  Labels and masks: anything non-zero is 1.
    Returns (value, part [B, 6] = {sum_m, cnt_m, sum_s, sum_e, sum_a, cnt_l} per sample)."""
    dt = pm.dtype
    ym, ys, ye, ya, mm, lm = ((x != 0).to(dt) for x in (ym, ys, ye, ya, mm, lm))
    part = torch.stack([(_scaled_bce(pm, ym, sm) * mm).sum((1, 2)), mm.sum((1, 2)), (_scaled_bce(ps, ys, ss) * lm).sum(1),
                        (_scaled_bce(pe, ye, se) * lm).sum(1), (_bce(pa, ya) * lm).sum(1), lm.sum(1)], dim=1)
    value = (part[:, 0] / part[:, 1]).mean() + (part[:, 2] / part[:, 5]).mean() + (part[:, 3] / part[:, 5]).mean() \
        + 0.5 * (part[:, 4] / part[:, 5]).mean()
    return value, part


def loss_grad_ref(dloss, pm, ym, sm, mm, ps, ys, ss, pe, ye, se, pa, ya, lm):
    """The closed form csrc/loss.hip documents (torch's BCELoss gradient): d/dp = g_b w (p - y) / max(p (1 - p), 1e-12) at valid
    positions and 0 elsewhere, w = s y + (1 - s)(1 - y) for the three scaled terms, w = 1 and an extra factor 0.5 for pa,
    g_b = dloss / B / count_b.  Returns (dpm, dps, dpe, dpa)."""
    dt = pm.dtype
    B = pm.shape[0]
    ym, ys, ye, ya, mm, lm = ((x != 0).to(dt) for x in (ym, ys, ye, ya, mm, lm))

    def grad(p, y, w, mask, cnt):
        g = (dloss / B / cnt).view(-1, *([1] * (p.dim() - 1)))
        return g * w * (p - y) / (p * (1 - p)).clamp(min=1e-12) * mask
    w = lambda s, y: s * y + (1 - s) * (1 - y)
    cm, cl = mm.sum((1, 2)), lm.sum(1)
    return (grad(pm, ym, w(sm, ym), mm, cm), grad(ps, ys, w(ss, ys), lm, cl), grad(pe, ye, w(se, ye), lm, cl),
            0.5 * grad(pa, ya, torch.ones_like(pa), lm, cl))


# ---------------------------------------------------------------- GPU case lists and their inputs

# gate: (B, L, D, cells, lengths, n_dhbar, n_dres, boundary term)
GATE_CASES = [
    (1, 1, 4, "tri", (1,), 1, 0, False),
    (3, 5, 48, "tri", (5, 0, 3), 4, 2, True),
    (2, 12, 260, "tri", (12, 7), 2, 1, True),
    (2, 40, 512, "tri", (40, 33), 3, 4, False),
    (2, 24, 1056, "ragged", (24, 24), 4, 1, True),
    (2, 130, 8, "all_cells", (130, 130), 1, 1, True),          # every (b, i, j) of a random non-triangular mask
]


def _gate_id(c):
    B, L, D, kind, lens, ndh, ndr, bnd = c
    return f"B{B}_L{L}_D{D}_{kind}_dh{ndh}_dres{ndr}_{'boundary' if bnd else 'plain'}"


@functools.lru_cache(maxsize=None)
def _gate_layout(case):
    B, L, D, kind, lens, ndh, ndr, bnd = case
    g = torch.Generator().manual_seed(L * 131 + D)
    if kind == "all_cells":
        return make_layout(torch.rand(B, L, L, generator=g) < 0.5, "all_cells")
    return make_layout(moment_mask(B, L, kind, list(lens), g), "from_mask")


# content unit, small (mini tiles): (C, D, dl, B, L, lengths, Nq); each under both layouts and the three variants
CU_SMALL = [
    (4, 32, 16, 2, 6, (6, 4), 5),
    (3, 48, 48, 3, 7, (7, 3, 5), 9),
    (2, 104, 16, 3, 8, (8, 5, 6), 13),
    (4, 128, 128, 2, 8, (8, 6), 32),
]
# content unit, large (128-row main tiles): full triangle, L = 64, from_mask
CU_LARGE = [
    (4, 64, 32, 4, 64, (64,) * 4, 20),
    (3, 64, 32, 6, 64, (64,) * 6, 20),
    (4, 132, 32, 4, 64, (64,) * 4, 20),
]
VARIANTS = ("dfc", "nodfc", "last")        # last = 0 with dfc_out, last = 0 with dfc_out = NULL, last = 1
# (shape, layout, variant)
CU_CASES = ([(s, lay, v) for s in CU_SMALL for lay in ("from_mask", "all_cells") for v in VARIANTS]
            + [(s, "from_mask", "dfc") for s in CU_LARGE] + [(CU_LARGE[0], "from_mask", "last")])
CU_MODE3_CASES = [(CU_SMALL[0], "from_mask", "dfc"), (CU_LARGE[0], "from_mask", "dfc")]
CU_IN = ("fc", "hbar", "Wch", "bch", "Mq", "uq", "what", "shat", "Wc", "bc")


def _cu_id(case):
    (C, D, dl, B, L, lens, Nq), layout, variant = case
    return f"C{C}_D{D}_dl{dl}_B{B}_L{L}_Nq{Nq}_{layout}_{variant}"


def _cu_cell_count(case):
    (C, D, dl, B, L, lens, Nq), layout, variant = case
    return B * L * L if layout == "all_cells" else sum(n * (n + 1) // 2 for n in lens)


def _cu_launches(case):
    """(NT launches {name: (M, N, K)}, TN launches {name: (rows, I, J)}) of one case, as csrc/content_unit.hip issues them."""
    (C, D, dl, B, L, lens, Nq), layout, variant = case
    N = _cu_cell_count(case)
    M = N * C
    if variant == "last":
        nt = {"fwd chat": (M, dl, D), "fwd lastmean": (N, D, dl), "bwd dcchat last": (N, dl, D), "bwd dfc": (M, D, dl)}
        tn = {"dWc": (N, D, dl), "dWch": (M, dl, D)}
    else:
        nt = {"fwd chat": (M, dl, D), "fwd out": (M, D, dl), "bwd dcchat": (M, dl, D), "bwd dfc": (M, D, dl)}
        tn = {"dWc": (M, D, dl), "dWch": (M, dl, D)}
    return nt, tn


@functools.lru_cache(maxsize=4)
def _cu_reference(case):
    """Inputs (float64 copies of the fp32 values the kernels get), the layout, and the float64 outputs and gradients of one case."""
    (C, D, dl, B, L, lens, Nq), layout, variant = case
    label = _cu_id(case)
    last = variant == "last"
    g = torch.Generator().manual_seed(C * 1000 + D * 10 + dl + L)
    mask = moment_mask(B, L, "tri", list(lens), g)
    lay, x = _attn_inputs(C, dl, Nq, mask, layout == "all_cells", seed=C + D + dl + Nq)
    assert lay.N == _cu_cell_count(case)
    N = lay.N
    r = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    x = {k: v for k, v in x.items() if k != "chat"}
    x.update(fc=r(N, C, D), hbar=r(N, D), Wch=r(dl, D) / math.sqrt(D), bch=0.1 * r(dl), Wc=r(D, dl) / math.sqrt(dl), bc=0.1 * r(D))
    # the clip logits are quadratic in a + shat (both linear in what and shat): scale the two to a spread of about 1.2
    cell_live = (lay.cells[:, 3] != 0).view(-1, 1, 1)
    with torch.no_grad():
        o = content_unit_ref(x["fc"], x["hbar"], lay.cells, C, x["Wch"], x["bch"], x["Mq"], x["uq"], x["what"], x["shat"], x["qmask"], x["Wc"],
                             x["bc"], True, x["hbar"])
        sp = _spread(clip_logits(o["chat"], o["S"], lay.cells, C, x["what"], x["shat"], x["qmask"]), cell_live)
    x["what"], x["shat"] = x["what"] * math.sqrt(1.2 / sp), x["shat"] * math.sqrt(1.2 / sp)
    x = {k: v.float().double() for k, v in x.items()}                  # the kernels' fp32 inputs, exactly
    leaves = {k: v.clone().requires_grad_(k in CU_IN) for k, v in x.items()}
    fcmean_in = leaves["fc"].mean(1) if last else None
    out = content_unit_ref(leaves["fc"], leaves["hbar"], lay.cells, C, leaves["Wch"], leaves["bch"], leaves["Mq"], leaves["uq"], leaves["what"],
                           leaves["shat"], leaves["qmask"], leaves["Wc"], leaves["bc"], last, fcmean_in)
    # both softmaxes must be spread, or a dropped or doubled entry would hide behind a uniform or saturated one
    S = out.pop("S").detach()
    _assert_spread(S, cell_live & (x["qmask"][lay.cells[:, 0].long()] != 0).unsqueeze(1), label, "word")
    _assert_spread(clip_logits(out["chat"].detach(), S, lay.cells, C, x["what"], x["shat"], x["qmask"]), cell_live, label, "clip")
    G_out, G_mean = r(N, C, D).float().double(), r(N, D).float().double()
    tot = (out["fcmean"] * G_mean).sum() + ((out["fc_out"] * G_out).sum() if variant == "dfc" else 0)
    grads = dict(zip(CU_IN, torch.autograd.grad(tot, [leaves[k] for k in CU_IN])))
    outs = {k: (None if v is None else v.detach()) for k, v in out.items()}
    return lay, x, (None if fcmean_in is None else fcmean_in.detach()), outs, G_out, G_mean, grads


# loss: (B, L, mask bytes)
LOSS_CASES = [
    (1, 3, (1,)),
    (5, 16, (1,)),
    (3, 17, (7, 255)),
    (2, 300, (1,)),
    (37, 8, (1,)),
]
PLANTS = (0.0, 1.0, 1e-9, 1.0 - 2.0 ** -24)


def _loss_id(c):
    return f"B{c[0]}_L{c[1]}_mask{'_'.join(map(str, c[2]))}"


@functools.lru_cache(maxsize=None)
def _loss_inputs(case, plant=True):
    """The thirteen arguments of the loss on the CPU (fp32 scores and scale targets, uint8 labels and masks), ragged lengths, the
    first sample full; `planted`: {(tensor, value index, label)} of the edge probabilities written at valid positions."""
    B, L, mask_vals = case
    g = torch.Generator().manual_seed(B * 1000 + L)
    lens = [L] + [int(v) for v in torch.randint(max(1, L // 2), L + 1, (B - 1,), generator=g)]
    lmb = lengths_mask(B, L, lens)
    mmb = torch.triu(lmb.unsqueeze(2) & lmb.unsqueeze(1))
    x, planted = {}, set()
    for k, (p, y, s, valid) in enumerate((("pm", "ym", "sm", mmb), ("ps", "ys", "ss", lmb), ("pe", "ye", "se", lmb), ("pa", "ya", None, lmb))):
        shape = valid.shape
        prob = torch.sigmoid(4 * torch.randn(shape, generator=g)).clamp(max=1 - 2.0 ** -23)    # fp32 sigmoid saturates to 1.0 beyond 17
        lab = (torch.rand(shape, generator=g) < 0.5).to(torch.uint8)
        if plant:                                                      # value v under label yv at the valid positions, in turn
            pos = valid.reshape(-1).nonzero().flatten()
            pos = pos[torch.randperm(pos.numel(), generator=g)][:8]
            for n, o in enumerate(pos.tolist()):
                e = (n + 3 * k) % 8
                prob.view(-1)[o], lab.view(-1)[o] = PLANTS[e % 4], e // 4
                planted.add((p, e % 4, e // 4))
        x[p], x[y] = prob, lab
        if s is not None:
            u = torch.rand(shape, generator=g)
            x[s] = torch.where(u < 0.1, torch.zeros(()), torch.where(u > 0.9, torch.ones(()), torch.rand(shape, generator=g)))
    pick = lambda valid: torch.tensor(mask_vals, dtype=torch.uint8)[torch.randint(0, len(mask_vals), valid.shape, generator=g)] * valid
    x["mm"], x["lm"] = pick(mmb), pick(lmb)
    assert all(x[k].dtype == (torch.float32 if k[0] in "ps" else torch.uint8) for k in LOSS_KEYS)
    return x, planted


@functools.lru_cache(maxsize=None)
def _loss_reference(case):
    x, _ = _loss_inputs(case)
    xd = [x[k].double() if x[k].dtype == torch.float32 else x[k] for k in LOSS_KEYS]
    value, part = loss_ref(*xd)
    return value, part, loss_grad_ref(1.7, *xd)


# ---------------------------------------------------------------- CPU: the restatements against the oracle

@pytest.mark.parametrize("layout", ["from_mask", "all_cells"])
@pytest.mark.parametrize("mask_kind", ["dense", "ragged"])
def test_gate_and_content_unit_refs_match_oracle(mask_kind, layout):
    """gate_ref's hbar and content_unit_ref against oracle.content_unit (the content unit of oracle.smi_layer) in float64, the word-side
    operands from word_side_ref; then the last form against the clip mean of the full one (fcmean_in = mean_c fc)."""
    import models  # noqa: F401
    from oracle import smin_oracle as O
    B, L, C, D, dl, Nq = 3, 5, 4, 24, 16, 6
    p = "smis.0.content_unit."
    sd = _smi_params(D, dl, 1.5, 1)
    g = torch.Generator().manual_seed(2)
    if mask_kind == "dense":
        mm = torch.ones(B, L, L, dtype=torch.bool)
    else:
        mm = torch.rand(B, L, L, generator=g) < 0.6
        mm[2, 1:3] = False
    qmask = torch.ones(B, Nq)
    qmask[1, 4:] = 0
    qmask[2, 1] = 0
    f_c = torch.randn(B, L, L, C, D, generator=g, dtype=torch.float64)
    f_m = torch.randn(B, L, L, D, generator=g, dtype=torch.float64)
    f_w = torch.randn(B, Nq, D, generator=g, dtype=torch.float64) * qmask.double().unsqueeze(-1)
    f_s = torch.randn(B, D, generator=g, dtype=torch.float64)
    want = O.content_unit(sd, p, f_c, f_w, f_s, f_m, qmask.unsqueeze(-1), mm)
    lay = make_layout(mm, layout)
    assert mask_kind == "dense" or (lay.N < B * L * L if layout == "from_mask" else bool((lay.cells[:, 3] == 0).any()))
    fm = lay.pack(f_m)
    hbar, _, _ = gate_ref(fm, f_s, lay.cells, [torch.ones_like(fm)], [])
    torch.testing.assert_close(hbar, lay.pack(torch.sigmoid(f_m * f_s[:, None, None, :]) * f_m), rtol=PIN_TOL, atol=PIN_TOL)
    (what, shat, _, Mq, uq), = word_side_ref(f_w, f_s, qmask.double(), [sd[p + n] for n in WORD_PARAM_NAMES])
    W = (sd[p + "linear_c_hat.weight"], sd[p + "linear_c_hat.bias"], Mq, uq, what, shat, qmask.double(),
         sd[p + "linear_c.weight"], sd[p + "linear_c.bias"])
    fc = lay.pack(f_c)
    full = content_unit_ref(fc, hbar, lay.cells, C, *W, False, None)
    torch.testing.assert_close(full["fc_out"], lay.pack(want), rtol=PIN_TOL, atol=PIN_TOL)
    torch.testing.assert_close(full["fcmean"], lay.pack(want).mean(1), rtol=PIN_TOL, atol=PIN_TOL)
    last = content_unit_ref(fc, hbar, lay.cells, C, *W, True, fc.mean(1))
    assert last["fc_out"] is None
    torch.testing.assert_close(last["fcmean"], full["fcmean"], rtol=PIN_TOL, atol=PIN_TOL)
    torch.testing.assert_close(last["cchat"], full["cchat"].reshape(-1, C, dl).mean(1), rtol=PIN_TOL, atol=PIN_TOL)
    torch.testing.assert_close(last["chat"], full["chat"], rtol=0, atol=0)


@pytest.mark.parametrize("case", LOSS_CASES, ids=[_loss_id(c) for c in LOSS_CASES])
def test_loss_ref_matches_oracle(case):
    """loss_ref's value against oracle.loss_fn in float64, the planted 0 / 1 / 1e-9 / 1 - 2^-24 included (both clamp the logs at -100);
    the partials recombine to the value; every sample keeps a valid cell and a valid snippet."""
    from oracle import smin_oracle as O
    x, _ = _loss_inputs(case)
    assert bool((x["mm"] != 0).flatten(1).any(1).all()) and bool((x["lm"] != 0).any(1).all())
    xd = {k: x[k].double() if x[k].dtype == torch.float32 else x[k] != 0 for k in LOSS_KEYS}
    value, part = loss_ref(*[xd[k] for k in LOSS_KEYS])
    want = O.loss_fn(xd["pm"], xd["ym"], xd["sm"], xd["mm"], xd["ps"], xd["ys"], xd["ss"], xd["pe"], xd["ye"], xd["se"], xd["pa"], xd["ya"], xd["lm"])
    torch.testing.assert_close(value, want, rtol=PIN_TOL, atol=PIN_TOL)
    assert part.shape == (case[0], 6) and torch.equal(part[:, 1], (x["mm"] != 0).sum((1, 2)).double())
    assert torch.equal(part[:, 5], (x["lm"] != 0).sum(1).double())


@pytest.mark.parametrize("case", LOSS_CASES, ids=[_loss_id(c) for c in LOSS_CASES])
def test_loss_grad_ref_matches_oracle_autograd(case):
    """loss_grad_ref against autograd of oracle.loss_fn in float64, on interior probabilities only (the same inputs without the planted
    values): at a probability of exactly 0 or 1 autograd of a clamped log gives 0, where torch's BCELoss -- and the kernel -- give the
    floored quotient w (p - y) / 1e-12 that loss_grad_ref states."""
    from oracle import smin_oracle as O
    x, planted = _loss_inputs(case, plant=False)
    assert not planted
    xd = {k: x[k].double() if x[k].dtype == torch.float32 else x[k] != 0 for k in LOSS_KEYS}
    leaves = {k: xd[k].clone().requires_grad_(True) for k in ("pm", "ps", "pe", "pa")}
    assert all(bool(((v > 0) & (v < 1)).all()) for v in leaves.values())
    a = {**xd, **leaves}
    want = torch.autograd.grad(1.7 * O.loss_fn(a["pm"], a["ym"], a["sm"], a["mm"], a["ps"], a["ys"], a["ss"], a["pe"], a["ye"], a["se"], a["pa"],
                                               a["ya"], a["lm"]), list(leaves.values()))
    got = loss_grad_ref(1.7, *[xd[k] for k in LOSS_KEYS])
    for gg, ww in zip(got, want):
        torch.testing.assert_close(gg, ww, rtol=PIN_TOL, atol=PIN_TOL * ww.abs().max().item())


def test_loss_cases_plant_every_edge():
    """Every (score tensor, planted value, label) occurs at a valid position of some case, all of them in every case with eight valid
    positions; the mask bytes 7 and 255 occur; L = 300 takes a second trip of the boundary loop, L = 3 has L * L < 256."""
    every = {(p, v, y) for p in ("pm", "ps", "pe", "pa") for v in range(4) for y in (0, 1)}
    reached = set()
    for case in LOSS_CASES:
        x, planted = _loss_inputs(case)
        reached |= planted
        if case[1] >= 16:
            assert planted == every, case
        for (p, v, y) in planted:
            at = x[p] == torch.tensor(PLANTS[v], dtype=torch.float64).float()
            valid = x["mm" if p == "pm" else "lm"] != 0
            assert bool((at & valid & (x["y" + p[1]] == y)).any()), (case, p, v, y)
        for s in ("sm", "ss", "se"):
            assert bool((x[s] >= 0).all() and (x[s] <= 1).all())
            assert case[1] < 16 or (bool((x[s] == 0).any()) and bool((x[s] == 1).any()))
    assert reached == every
    assert {7, 255} <= set(_loss_inputs(LOSS_CASES[2])[0]["mm"].unique().tolist()) | set()
    assert {7, 255} <= set(_loss_inputs(LOSS_CASES[2])[0]["lm"].unique().tolist())
    assert any(L > 256 for _, L, _ in LOSS_CASES) and any(L * L < 256 for _, L, _ in LOSS_CASES)
    assert float(torch.tensor(PLANTS[3]).float()) < 1.0 and float(torch.tensor(PLANTS[2]).float()) > 0.0


# ---------------------------------------------------------------- mirrors of the launch arithmetic

SPR_PH = 8                        # sample_partial_reduce_kernel: phases over the chunks


def chunking_fine(L):
    """common.h chunking_fine: (cells per chunk, max_chunks) -- at most 512 chunks, at least 32 cells each."""
    cells = L * L
    mc = max(1, min(512, cdiv(cells, 32)))
    cpc = cdiv(cells, mc)
    return cpc, cdiv(cells, cpc)


def gate_forms(case):
    """The forms of gate_fwd_kernel, gate_bwd_kernel and sample_partial_reduce_kernel one case runs."""
    B, L, D, kind, lens, ndh, ndr, bnd = case
    lay = _gate_layout(case)
    counts = torch.bincount(lay.cells[:, 0].long(), minlength=B).tolist()
    cpc, mc = chunking_fine(L)
    f = {("n_dhbar", ndh), ("n_dres", ndr), ("boundary", bnd)}
    if cdiv(L * L, 32) > 512:
        assert mc < cdiv(L * L, 32) and mc <= 512
        f.add("chunks capped")
    for b, n in enumerate(counts):
        if n == 0:
            if 0 < b < B - 1 and counts[b - 1] and counts[b + 1]:
                f.add("empty sample between two")
            continue
        nch = cdiv(n, cpc)
        f.add("1 chunk" if nch == 1 else "2..7 chunks" if nch < SPR_PH else "more than 8 chunks" if nch > SPR_PH else "8 chunks")
        if nch < mc:
            f.add("fewer live chunks than max_chunks")
        f |= {("chunk cells % 4", min(cpc, n - k * cpc) % 4) for k in range(nch)}
    trips = cdiv(D, 512)                                   # for (d = threadIdx.x * 4; d < D; d += 512), 128 threads
    tail = D - 512 * (trips - 1)
    f.add(("d loop", trips, "full" if tail == 512 else "partial"))
    f.add(("reducer column blocks", cdiv(D // 4, 64)))
    if (lay.N * (D // 4)) % 256:
        f.add("forward: last workgroup partly idle")
    return f


GATE_REQUIRED = (
    {"1 chunk", "2..7 chunks", "more than 8 chunks", "chunks capped", "empty sample between two", "fewer live chunks than max_chunks",
     "forward: last workgroup partly idle"}
    | {("chunk cells % 4", k) for k in range(4)}
    | {("d loop", 1, "full"), ("d loop", 1, "partial"), ("d loop", 3, "partial")}
    | {("reducer column blocks", 1), ("reducer column blocks", 2)}
    | {("n_dhbar", k) for k in (1, 2, 3, 4)} | {("n_dres", k) for k in (0, 1, 2, 4)} | {("boundary", True), ("boundary", False)}
)


def test_gate_cases_reach_every_form():
    reached = set()
    for c in GATE_CASES:
        reached |= gate_forms(c)
    missing = GATE_REQUIRED - reached
    assert not missing, sorted(map(str, missing))
    assert chunking_fine(1) == (1, 1) and chunking_fine(5) == (25, 1) and chunking_fine(130) == (34, 498) and chunking_fine(40) == (32, 50)
    assert any(c[2] // 4 == 65 for c in GATE_CASES) and any(c[2] == 1056 for c in GATE_CASES)
    # the non-triangular list: cells with j < i, so the boundary term's A[b, i, j] is read off the triangle too
    c = _gate_layout(GATE_CASES[5]).cells
    assert bool((c[:, 2] < c[:, 1]).any())


def test_content_unit_cases_reach_every_form():
    """Mini and 128-row main tiles for every NT launch of csrc/content_unit.hip on N*C rows (the two launches of the last form that
    run on N rows are mini here: main tiles would need more than 32 768 cells), one and several row splits of both TN launches,
    every C, variant, layout, dl and the column edges."""
    nt_reached, tn_reached = set(), set()
    for case in CU_CASES:
        nt, tn = _cu_launches(case)
        nt_reached |= {(k, "mini" if nt_form(*v) == "mini" else "main") for k, v in nt.items() if nt_form(*v) in ("mini", "main", "main+idle-slots")}
        tn_reached |= {(k, "splits=1" if "splits=1" in tn_forms(*v) else "splits>1") for k, v in tn.items()}
        assert all(nt_form(*v) in ("mini", "main", "main+idle-slots") for v in nt.values()), case
    rows_MC = ("fwd chat", "fwd out", "bwd dcchat", "bwd dfc")
    assert {(k, f) for k in rows_MC for f in ("mini", "main")} <= nt_reached, sorted(nt_reached)
    assert {("fwd lastmean", "mini"), ("bwd dcchat last", "mini")} <= nt_reached
    assert 128 * H.GEMM_SLOTS // 3 == 32768 and nt_form(32768, 64, 32) == "mini" and nt_form(32769, 64, 32) != "mini"
    assert tn_reached == {(k, f) for k in ("dWc", "dWch") for f in ("splits=1", "splits>1")}, sorted(tn_reached)
    assert H.tn_splits(_cu_cell_count(CU_CASES[-1]), 64, 32) > 1                # the last form's dWc over N rows, several splits
    shapes = [c[0] for c in CU_CASES]
    assert {s[0] for s in shapes} == {2, 3, 4} and {16, 48, 128} <= {s[2] for s in shapes}
    assert {(s[0], v) for s, _, v in CU_CASES} == {(C, v) for C in (2, 3, 4) for v in VARIANTS}
    assert {(lay, v) for _, lay, v in CU_CASES} == {(lay, v) for lay in ("from_mask", "all_cells") for v in VARIANTS}
    assert any(s[1] % 64 and s[1] < 128 for s in shapes) and any(s[1] == 132 for s in CU_LARGE)
    # the quad epilogues (C = 4) and the general ones (C != 4) both on main tiles
    assert {s[0] for s in CU_LARGE} == {3, 4}
    assert all(c in CU_CASES for c in CU_MODE3_CASES)
    assert nt_form(*_cu_launches(CU_MODE3_CASES[0])[0]["fwd out"]) == "mini" and nt_form(*_cu_launches(CU_MODE3_CASES[1])[0]["fwd out"]) != "mini"


@pytest.mark.parametrize("case", [c for c in CU_CASES if c[0] in CU_SMALL], ids=_cu_id)
def test_content_unit_small_cases_have_spread_softmaxes(case):
    """The reference of every small case builds on the CPU: its own guards hold (cell count, both softmaxes spread); masked cells of the
    all_cells lists give chat = 0 and fc_out = fc + hbar."""
    lay, x, fcmean_in, outs, G_out, G_mean, grads = _cu_reference(case)
    (C, D, dl, B, L, lens, Nq), layout, variant = case
    dead = lay.cells[:, 3] == 0
    assert bool(dead.any()) == (layout == "all_cells") and bool((x["qmask"] == 0).any())
    assert bool((outs["chat"][dead.repeat_interleave(C)] == 0).all())
    if variant != "last":
        assert torch.equal(outs["fc_out"][dead], (x["fc"] + x["hbar"].unsqueeze(1))[dead])
    assert all(bool(torch.isfinite(v).all()) and bool(v.abs().max() > 0) for v in grads.values())


def test_bounds_separate_fp32_rounding_from_wrong_formulas():
    """On the CPU: an fp32 restatement of the same formulas sits far inside every bound, and a wrong one -- the gate's boundary term
    dropped, fcmean divided by C + 1 -- far outside the bound of the assertion that is meant to catch it."""
    rel = lambda got, ref: (got.double() - ref).abs().max().item() / ref.abs().max().item()
    case = GATE_CASES[2]
    B, L, D, kind, lens, ndh, ndr, bnd = case
    lay = _gate_layout(case)
    x = _gate_inputs(case, lay)
    ref = gate_ref(x["fm"], x["fs"], lay.cells, x["dh"], x["dres"], x["A"], x["dout"])
    f32 = lambda t: t.float()
    low = gate_ref(f32(x["fm"]), f32(x["fs"]), lay.cells, [f32(t) for t in x["dh"]], [f32(t) for t in x["dres"]], f32(x["A"]), f32(x["dout"]))
    for got, want, tol in zip(low, ref, (FWD_TOL, GRAD_TOL, GRAD_TOL)):
        assert rel(got, want) <= tol / 50
    wrong = gate_ref(x["fm"], x["fs"], lay.cells, x["dh"], x["dres"])
    assert rel(wrong[1], ref[1]) > 100 * GRAD_TOL and rel(wrong[2], ref[2]) > 100 * GRAD_TOL
    lay, xc, fcmean_in, outs, G_out, G_mean, grads = _cu_reference(CU_CASES[0])
    C = CU_CASES[0][0][0]
    low = content_unit_ref(f32(xc["fc"]), f32(xc["hbar"]), lay.cells, C, *[f32(xc[k]) for k in ("Wch", "bch", "Mq", "uq", "what", "shat", "qmask", "Wc", "bc")],
                           False, None)
    for k in ("chat", "cchat", "fc_out", "fcmean"):
        assert rel(low[k], outs[k]) <= FWD_TOL / 10, k
    assert rel(outs["fcmean"] * C / (C + 1), outs["fcmean"]) > 100 * FWD_TOL
    lcase = LOSS_CASES[1]
    xl, _ = _loss_inputs(lcase)
    value, part, grads = _loss_reference(lcase)
    lv, lp = loss_ref(*[xl[k] for k in LOSS_KEYS])
    assert abs(lv.item() - value.item()) <= LOSS_TOL / 10 * abs(value.item())
    lg = loss_grad_ref(1.7, *[xl[k] for k in LOSS_KEYS])
    for gg, ww in zip(lg, grads):
        assert bool(((gg.double() - ww).abs() <= LOSS_TOL / 10 * ww.abs()).all())
    # the planted values are what a max-norm would hide the rest behind
    assert grads[0].abs().max().item() > 1e8 * grads[0].abs()[grads[0] != 0].median().item()


# ---------------------------------------------------------------- GPU helpers
def _rel(got, ref):
    """max |got - ref| / max |ref| (inf for a NaN: an element the kernel never wrote)"""
    if not ref.numel():
        return 0.0
    got = got.detach().double().cpu()
    if not bool(torch.isfinite(got).all()):
        return float("inf")
    return (got - ref).abs().max().item() / max(ref.abs().max().item(), 1e-30)


def _vp(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _arr(ts):
    return (ctypes.c_void_p * max(1, len(ts)))(*[t.data_ptr() for t in ts])


def _check(label, what, got, ref, tol, worst, key):
    e = _rel(got, ref)
    worst[key] = max(worst.get(key, 0.0), e)
    assert e <= tol, (label, what, e)


def _report(family, label, worst):
    print(f"{family} {label}: worst " + " ".join(f"{k} {v:.2e}" for k, v in worst.items()))


# ---------------------------------------------------------------- GPU: gate

def _gate_inputs(case, lay):
    B, L, D, kind, lens, ndh, ndr, bnd = case
    g = torch.Generator().manual_seed(B * 7 + L * 3 + D)
    r = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64).float().double()      # the kernels' fp32 inputs, exactly
    N = lay.N
    return dict(fm=r(N, D), fs=r(B, D), dh=[r(N, D) for _ in range(ndh)], dres=[r(N, D) for _ in range(ndr)], hsum=r(N, D),
                A=r(B, L, L) if bnd else None, dout=r(B, L, D) if bnd else None)


@pytest.mark.gpu
@pytest.mark.parametrize("case", GATE_CASES, ids=[_gate_id(c) for c in GATE_CASES])
def test_gate_against_fp64(dev, case):
    """smin_gate_fwd, smin_gate_fwd_sum and smin_gate_bwd (gradient lists summed in-kernel, the boundary unit's A[b, i, j] * dout[b, i, :]
    formed in-kernel, the two-stage per-sample sum of dfs) on a workspace of exactly 4 B max_chunks D bytes."""
    from vml_amd._lib import call, ptr, stream
    B, L, D, kind, lens, ndh, ndr, bnd = case
    label = _gate_id(case)
    lay = _gate_layout(case)
    N = lay.N
    x = _gate_inputs(case, lay)
    hbar0, dfm0, dfs0 = gate_ref(x["fm"], x["fs"], lay.cells, x["dh"], x["dres"], x["A"], x["dout"])
    lay_d = _layout_to(lay, dev)
    f32 = lambda t: None if t is None else t.float().to(dev)
    fm, fs, hsum, A, dout = (f32(x[k]) for k in ("fm", "fs", "hsum", "A", "dout"))
    dh, dres = [f32(t) for t in x["dh"]], [f32(t) for t in x["dres"]]
    worst = {}
    hbar = _nan((N, D), dev)
    call("smin_gate_fwd", stream(), ptr(fm), ptr(fs), ptr(lay_d.cells), N, D, ptr(hbar))
    _check(label, "hbar", hbar, hbar0, FWD_TOL, worst, "hbar")
    hbar2, hsum_out = _nan((N, D), dev), _nan((N, D), dev)
    call("smin_gate_fwd_sum", stream(), ptr(fm), ptr(fs), ptr(lay_d.cells), N, D, ptr(hbar2), ptr(hsum), ptr(hsum_out))
    assert torch.equal(hbar2, hbar), (label, "smin_gate_fwd_sum's hbar differs from smin_gate_fwd's")
    assert torch.equal(hsum_out, hsum + hbar), (label, "hsum_out is not the fp32 sum hsum_in + hbar")
    cpc, mc = chunking_fine(L)
    dh_arr, dres_arr = _arr(dh), _arr(dres)

    def run():
        dfm, dfs = _nan((N, D), dev), _nan((B, D), dev)
        ws, wn = _ws_nan(4 * B * mc * D, dev)
        call("smin_gate_bwd", stream(), dh_arr, ndh, dres_arr if ndr else None, ndr, ptr(fm), ptr(fs), ptr(lay_d.row_ptr), N, B, L, D,
             ptr(dfm), ptr(dfs), ptr(ws), wn, ptr(lay_d.cells) if bnd else None, _vp(A), _vp(dout))
        return dfm, dfs
    dfm, dfs = run()
    _check(label, "dfm", dfm, dfm0, GRAD_TOL, worst, "dfm")
    _check(label, "dfs", dfs, dfs0, GRAD_TOL, worst, "dfs")
    counts = torch.bincount(lay.cells[:, 0].long(), minlength=B)
    for b in (counts == 0).nonzero().flatten().tolist():
        assert bool((dfs[b] == 0).all()), (label, "dfs of a sample with no cell must be exactly 0")
    again = run()
    assert torch.equal(dfm, again[0]) and torch.equal(dfs, again[1]), (label, "backward not deterministic")
    _report("gate", label, worst)


# ---------------------------------------------------------------- saturated inputs: gate

# the smallest case of each form the table names beyond the chunk counts: D < 512 with an empty sample and both gradient lists; D = 1056
# (three trips of the d loop, several reducer column blocks); the non-triangular all_cells list with the capped chunk count
GATE_SAT_CASES = [GATE_CASES[1], GATE_CASES[4], GATE_CASES[5]]
GATE_PRODUCTS = (20.0, 90.0, 200.0, 1e4)
LEVELS = ("hard", "frozen")


@functools.lru_cache(maxsize=None)
def _gate_saturated(case, level):
    """_gate_inputs of a case with fm chosen so that the gate's pre-activation fm * fs[b] takes given values: +-{20, 90, 200, 1e4}
    everywhere (frozen), or on half of the elements with N(0, 2) on the rest (hard).  |fs| lies in [1, 4], so |fm| <= 1e4."""
    lay = _gate_layout(case)
    x = dict(_gate_inputs(case, lay))
    g = torch.Generator().manual_seed(17 + len(level) + case[2])
    B, D, N = case[0], case[2], lay.N
    sign = lambda *s: torch.randint(0, 2, s, generator=g).double() * 2 - 1
    fs = ((1 + 3 * torch.rand(B, D, generator=g, dtype=torch.float64)) * sign(B, D)).float().double()
    t = torch.tensor(GATE_PRODUCTS, dtype=torch.float64)[torch.randint(0, 4, (N, D), generator=g)] * sign(N, D)
    if level == "hard":
        t = torch.where(torch.rand(N, D, generator=g) < 0.5, t, 2 * torch.randn(N, D, generator=g, dtype=torch.float64))
    x["fs"], x["fm"] = fs, (t / fs[lay.cells[:, 0].long()]).float().double()
    return lay, x, t


@pytest.mark.parametrize("level", LEVELS)
@pytest.mark.parametrize("case", GATE_SAT_CASES, ids=[_gate_id(c) for c in GATE_SAT_CASES])
def test_gate_saturated_inputs_hold_what_they_claim(case, level):
    """On the float64 reference: hard -- at least a quarter of the pre-activations beyond +-17 and a quarter inside +-4; frozen -- every
    one within 1e-6 of +-{20, 90, 200, 1e4}, each value under both signs; |fm| <= 1e4; everything finite, the gradients included."""
    lay, x, t = _gate_saturated(case, level)
    z = x["fm"] * x["fs"][lay.cells[:, 0].long()]
    assert x["fm"].abs().max().item() <= 1e4 and bool((z.float().double() - t).abs().le(1e-6 * t.abs() + 1e-6).all())
    if level == "hard":
        assert (z.abs() > 17).double().mean().item() >= 0.25 and (z.abs() < 4).double().mean().item() >= 0.25
    else:
        assert all(bool(((z - s * p).abs() <= 1e-6 * p).any()) for p in GATE_PRODUCTS for s in (-1, 1))
    ref = gate_ref(x["fm"], x["fs"], lay.cells, x["dh"], x["dres"], x["A"], x["dout"])
    assert all(bool(torch.isfinite(r).all()) for r in ref)
    hi = z >= 19.9999                                                            # 1 - sigmoid(20) = 2.1e-9 < 2^-25: fp32 holds fm itself there
    assert bool(((ref[0][hi] - x["fm"][hi]).abs() <= 2.2e-9 * x["fm"][hi].abs()).all())
    assert bool((ref[0][z <= -745].abs() == 0).all())                            # exp(-745) is 0 in float64


@pytest.mark.gpu
@pytest.mark.parametrize("level", LEVELS)
@pytest.mark.parametrize("case", GATE_SAT_CASES, ids=[_gate_id(c) for c in GATE_SAT_CASES])
def test_gate_saturated_against_fp64(dev, case, level):
    """smin_gate_fwd and smin_gate_bwd on _gate_saturated: expf overflows on one side and underflows on the other.  hbar is fm exactly
    where the pre-activation is >= 20 and +-0 where it is <= -110 (fp32's sigmoid is exactly 1 and 0 there), never NaN; dfm and dfs are
    finite; the empty sample's dfs is exactly 0; the project's gate against gate_ref in float64, e_torch32 from gate_ref in fp32.
    Measured on an MI355X: INTEGRATION.md, "Saturated inputs"."""
    from tests.support.compare import gate
    from vml_amd._lib import call, ptr, stream
    B, L, D, kind, lens, ndh, ndr, bnd = case
    lay, x, t = _gate_saturated(case, level)
    N = lay.N
    want = gate_ref(x["fm"], x["fs"], lay.cells, x["dh"], x["dres"], x["A"], x["dout"])
    h = lambda v: v.float()
    ref32 = gate_ref(h(x["fm"]), h(x["fs"]), lay.cells, [h(v) for v in x["dh"]], [h(v) for v in x["dres"]], h(x["A"]), h(x["dout"]))
    lay_d = _layout_to(lay, dev)
    f32 = lambda v: v.float().to(dev)
    fm, fs, A, dout = (f32(x[k]) for k in ("fm", "fs", "A", "dout"))
    dh, dres = [f32(v) for v in x["dh"]], [f32(v) for v in x["dres"]]
    hbar = _nan((N, D), dev)
    call("smin_gate_fwd", stream(), ptr(fm), ptr(fs), ptr(lay_d.cells), N, D, ptr(hbar))
    _, mc = chunking_fine(L)
    dfm, dfs = _nan((N, D), dev), _nan((B, D), dev)
    ws, wn = _ws_nan(4 * B * mc * D, dev)
    call("smin_gate_bwd", stream(), _arr(dh), ndh, _arr(dres), ndr, ptr(fm), ptr(fs), ptr(lay_d.row_ptr), N, B, L, D, ptr(dfm), ptr(dfs), ptr(ws), wn,
         ptr(lay_d.cells), _vp(A), _vp(dout))
    torch.cuda.synchronize()
    assert all(bool(torch.isfinite(v).all()) for v in (hbar, dfm, dfs))
    z = (fm * fs[lay_d.cells[:, 0].long()]).cpu()
    assert torch.equal(hbar.cpu()[z >= 19.9999], fm.cpu()[z >= 19.9999]) and bool((hbar.cpu()[z <= -110] == 0).all())
    for name, got, w, r in zip(("hbar", "dfm", "dfs"), (hbar, dfm, dfs), want, ref32):
        gate(f"gate {_gate_id(case)} {level} {name}", got, w, r)
    counts = torch.bincount(lay.cells[:, 0].long(), minlength=B)
    assert bool((counts == 0).any()) == (case == GATE_CASES[1]) and all(bool((dfs[b] == 0).all()) for b in (counts == 0).nonzero().flatten().tolist())


@pytest.mark.gpu
def test_gate_refusals(dev):
    """Arguments outside the documented ranges are refused with a negative code before anything is launched: the NaN-prefilled
    outputs stay untouched."""
    import models
    from vml_amd._lib import ptr, stream
    lib = models.vml_amd._lib.load()
    B, L, D, N = 2, 4, 8, 6
    cells = torch.zeros(N, 4, dtype=torch.int32, device=dev)
    row_ptr = torch.zeros(B * L + 1, dtype=torch.int32, device=dev)
    buf = torch.zeros(4, N, D, device=dev)
    A, dout = torch.zeros(B, L, L, device=dev), torch.zeros(B, L, D, device=dev)
    arr = _arr([buf[k] for k in range(4)] + [buf[0]])
    _, mc = chunking_fine(L)
    need = 4 * B * mc * D
    ws = torch.zeros(need // 4, device=dev)
    hbar, dfm, dfs = _nan((N, D), dev), _nan((N, D), dev), _nan((B, D), dev)

    def bwd(D=D, ndh=1, ndr=1, A=None, dout=None, wn=need):
        return lib.smin_gate_bwd(stream(), arr, ndh, arr, ndr, ptr(buf[0]), ptr(buf[1]), ptr(row_ptr), N, B, L, D, ptr(dfm), ptr(dfs),
                                 ptr(ws), wn, ptr(cells), _vp(A), _vp(dout))
    assert lib.smin_gate_fwd(stream(), ptr(buf[0]), ptr(buf[1]), ptr(cells), N, 6, ptr(hbar)) < 0
    assert lib.smin_gate_fwd_sum(stream(), ptr(buf[0]), ptr(buf[1]), ptr(cells), N, 6, ptr(hbar), ptr(buf[2]), ptr(hbar)) < 0
    assert bwd(D=6) < 0
    assert bwd(ndh=0) < 0 and bwd(ndh=5) < 0
    assert bwd(ndr=5) < 0
    assert bwd(A=A) < 0 and bwd(dout=dout) < 0
    assert bwd(wn=need - 4) < 0
    torch.cuda.synchronize()
    assert all(bool(torch.isnan(t).all()) for t in (hbar, dfm, dfs))


# ---------------------------------------------------------------- GPU: content unit

def _run_content_unit(dev, case, label):
    import models
    from vml_amd._lib import call, ptr, stream
    (C, D, dl, B, L, lens, Nq), layout, variant = case
    last = variant == "last"
    lay, x, fcmean_in, outs0, G_out, G_mean, grads0 = _cu_reference(case)
    N = lay.N
    lay_d = _layout_to(lay, dev)
    d = {k: v.float().to(dev) for k, v in x.items()}
    fcmean_in_d = None if fcmean_in is None else fcmean_in.float().to(dev)
    worst = {}
    fc_out = None if last else _nan((N, C, D), dev)
    fcmean, chat, cchat = _nan((N, D), dev), _nan((N * C, dl), dev), _nan((N if last else N * C, dl), dev)
    call("smin_content_unit_fwd", stream(), ptr(d["fc"]), ptr(d["hbar"]), ptr(lay_d.cells), ptr(lay_d.row_ptr), N, B, L, C, D, dl, Nq,
         ptr(d["Wch"]), ptr(d["bch"]), ptr(d["Mq"]), ptr(d["uq"]), ptr(d["what"]), ptr(d["shat"]), ptr(d["qmask"]), ptr(d["Wc"]), ptr(d["bc"]),
         _vp(fcmean_in_d), int(last), _vp(fc_out), ptr(fcmean), ptr(chat), ptr(cchat))
    _check(label, "chat", chat, outs0["chat"], FWD_TOL, worst, "f")
    _check(label, "cchat", cchat, outs0["cchat"], FWD_TOL, worst, "f")
    _check(label, "fcmean", fcmean, outs0["fcmean"], FWD_TOL, worst, "f")
    if not last:
        _check(label, "fc_out", fc_out, outs0["fc_out"], FWD_TOL, worst, "f")
    dead = (lay.cells[:, 3] == 0).to(dev)
    if layout == "all_cells":
        assert bool(dead.any())
        assert bool((chat[dead.repeat_interleave(C)] == 0).all()), (label, "chat rows of masked cells must be exactly 0")
        if not last:
            assert torch.equal(fc_out[dead], (d["fc"] + d["hbar"].unsqueeze(1))[dead]), (label, "fc_out of a masked cell is fc + hbar")

    nbytes = models.vml_amd._lib.load().smin_content_unit_bwd_ws_bytes(N, B, C, D, dl, int(last))
    WchT, WcT = d["Wch"].t().contiguous(), d["Wc"].t().contiguous()
    dfc_out = G_out.float().to(dev) if variant == "dfc" else None
    dfcmean = G_mean.float().to(dev)

    def run():
        o = {k: _nan(d[k].shape, dev) for k in CU_IN}
        ws, wn = _ws_nan(nbytes, dev)
        call("smin_content_unit_bwd", stream(), _vp(dfc_out), ptr(dfcmean), ptr(d["fc"]), ptr(lay_d.cells), ptr(lay_d.row_ptr),
             N, B, L, C, D, dl, Nq, ptr(WchT), ptr(d["Mq"]), ptr(d["uq"]), ptr(d["what"]), ptr(d["shat"]), ptr(d["qmask"]), ptr(WcT),
             ptr(chat), ptr(cchat), ptr(o["fc"]), ptr(o["hbar"]), ptr(o["Wch"]), ptr(o["bch"]), ptr(o["Mq"]), ptr(o["uq"]), ptr(o["what"]),
             ptr(o["shat"]), ptr(o["Wc"]), ptr(o["bc"]), ptr(ws), wn, int(last))
        return o
    got = run()
    for k in CU_IN:
        _check(label, "d" + k, got[k], grads0[k], GRAD_TOL, worst, "g")
    again = run()
    assert all(torch.equal(got[k], again[k]) for k in CU_IN), (label, "backward not deterministic")
    _report("content_unit", label, worst)


@pytest.mark.gpu
@pytest.mark.parametrize("case", CU_CASES, ids=[_cu_id(c) for c in CU_CASES])
def test_content_unit_against_fp64(dev, case):
    """smin_content_unit_fwd / _bwd: chat, cchat (the clip mean when last), fc_out, fcmean and all ten gradients, on a workspace of
    exactly its query (smin_content_unit_bwd_ws_bytes).  EpLastMean on 128-row main tiles would need more than 32 768 cells and is left to the engine
    tests (tests/test_gemm_engine.py): the last form of the first large case runs its final GEMM as a mini launch on N rows."""
    _run_content_unit(dev, case, _cu_id(case))


@pytest.mark.gpu
@pytest.mark.parametrize("case", CU_MODE3_CASES, ids=[_cu_id(c) for c in CU_MODE3_CASES])
def test_content_unit_against_fp64_gemm_mode_3(dev, gemm_mode, case):
    """The same under smin_set_gemm_mode(3) (fp32 emulated on the bf16 matrix cores), within the same bounds: the header promises
    agreement with mode 0 to fp32 rounding."""
    import models
    gemm_mode("f32e")
    assert models.vml_amd._lib.load().smin_get_gemm_mode() == 3
    _run_content_unit(dev, case, _cu_id(case) + "-mode3")


# ---------------------------------------------------------------- GPU: loss

def _loss_direct(dev, case):
    """smin_loss_fwd / smin_loss_bwd (twice) into NaN-prefilled outputs: (loss, part, (dpm, dps, dpe, dpa))"""
    from vml_amd._lib import call, ptr, stream
    B, L, _ = case
    x, _ = _loss_inputs(case)
    d = {k: v.to(dev) for k, v in x.items()}
    args = [ptr(d[k]) for k in LOSS_KEYS]
    loss, part = _nan((1,), dev), _nan((B, 6), dev)
    call("smin_loss_fwd", stream(), *args, B, L, ptr(loss), ptr(part))
    dloss = torch.tensor([1.7], device=dev)

    def run():
        o = [_nan((B, L, L), dev)] + [_nan((B, L), dev) for _ in range(3)]
        call("smin_loss_bwd", stream(), ptr(dloss), ptr(part), *args, B, L, *[ptr(t) for t in o])
        return o
    grads = run()
    again = run()
    assert all(torch.equal(a, b) for a, b in zip(grads, again)), (_loss_id(case), "backward not deterministic")
    return d, loss, part, grads


@pytest.mark.gpu
@pytest.mark.parametrize("case", LOSS_CASES, ids=[_loss_id(c) for c in LOSS_CASES])
def test_loss_against_fp64(dev, case):
    """The value and each of the 6 B partials relative to float64; the gradients element by element, |got - ref| <= tol |ref|, and
    exactly 0 at every masked position (a planted 0 or 1 gives a gradient near 1e11: a max-norm would accept anything elsewhere)."""
    label = _loss_id(case)
    x, _ = _loss_inputs(case)
    value0, part0, grads0 = _loss_reference(case)
    _, loss, part, grads = _loss_direct(dev, case)
    worst = {}
    worst["value"] = abs(loss.item() - value0.item()) / abs(value0.item())
    perr = (part.double().cpu() - part0).abs() / part0.abs().clamp(min=1e-300)
    assert bool(torch.isfinite(part).all()) and bool((part0 != 0).all())
    worst["part"] = perr.max().item()
    names = ("dpm", "dps", "dpe", "dpa")
    for name, got, ref in zip(names, grads, grads0):
        got = got.double().cpu()
        assert bool(torch.isfinite(got).all()), (label, name, "an element was not written")
        live = ref != 0
        worst[name] = ((got - ref).abs()[live] / ref.abs()[live]).max().item() if bool(live.any()) else 0.0
    print(f"loss {label}: value {value0.item():.6f} worst " + " ".join(f"{k} {v:.2e}" for k, v in worst.items()))
    assert worst["value"] <= LOSS_TOL, (label, "value", worst["value"])
    assert worst["part"] <= LOSS_TOL, (label, "partials", perr)
    for name, got, ref in zip(names, grads, grads0):
        got = got.double().cpu()
        valid = (x["mm" if name == "dpm" else "lm"] != 0)
        assert bool((got[~valid] == 0).all()), (label, name, "a masked position must get exactly 0")
        bad = (got - ref).abs() > LOSS_TOL * ref.abs()
        assert not bool(bad.any()), (label, name, int(bad.sum()), worst[name])
    assert max(g.abs().max().item() for g in grads0) > 1e9 or case[1] < 16


# ---------------------------------------------------------------- saturated inputs: loss

# the smallest case whose every head has room for all 36 combinations; the mask bytes 7 and 255; L = 300, the boundary loop's second trip
LOSS_SAT_CASES = [LOSS_CASES[1], LOSS_CASES[2], LOSS_CASES[3]]
SAT_P = (0.0, 1e-45, 1e-30, 0.5, 1.0 - 2.0 ** -24, 1.0)          # 1e-45 rounds to fp32's smallest denormal
SAT_P_NAMES = ("0", "1e-45", "1e-30", "0.5", "1-2^-24", "1")
SAT_S = (0.0, 0.3, 1.0)
HEADS = (("pm", "ym", "sm", "mm"), ("ps", "ys", "ss", "lm"), ("pe", "ye", "se", "lm"), ("pa", "ya", None, "lm"))


@functools.lru_cache(maxsize=None)
def _loss_saturated(case):
    """A case's masks with every valid position of every head holding another of the 36 combinations (p, label, scale target) of
    SAT_P x {0, 1} x SAT_S, in steps of 7 through their list (a head with fewer than 36 valid positions still meets every (p, label)).
    Returns (x, {head: (valid flat positions, p index, label, s index)})."""
    x = {k: v.clone() for k, v in _loss_inputs(case, plant=False)[0].items()}
    p32, s32 = torch.tensor(SAT_P, dtype=torch.float64).float(), torch.tensor(SAT_S, dtype=torch.float64).float()
    where = {}
    for k, (p, y, s, mask) in enumerate(HEADS):
        valid = (x[mask] != 0).reshape(-1).nonzero().flatten()
        c = (7 * torch.arange(valid.numel()) + 5 * k) % 36
        ip, lab, js = c // 6, (c // 3) % 2, c % 3
        x[p].view(-1)[valid], x[y].view(-1)[valid] = p32[ip], lab.to(torch.uint8)
        if s is not None:
            x[s].view(-1)[valid] = s32[js]
        where[p] = (valid, ip, lab, js)
    return x, where


def _loss_saturated_refs(case):
    """float64: the oracle's value, loss_ref's partials, loss_grad_ref's gradients at dloss = 1.7.  fp32: training.loss_fn_torch's value
    and autograd gradients (torch's BCELoss, with its -100 and 1e-12 clamps), loss_ref's partials."""
    import models  # noqa: F401
    from oracle import smin_oracle as O
    from vml_amd.training import loss_fn_torch
    x, _ = _loss_saturated(case)
    xd = {k: x[k].double() if x[k].dtype == torch.float32 else x[k] != 0 for k in LOSS_KEYS}
    value = O.loss_fn(xd["pm"], xd["ym"], xd["sm"], xd["mm"], xd["ps"], xd["ys"], xd["ss"], xd["pe"], xd["ye"], xd["se"], xd["pa"], xd["ya"], xd["lm"])
    _, part = loss_ref(*[xd[k] for k in LOSS_KEYS])
    grads = loss_grad_ref(1.7, *[xd[k] for k in LOSS_KEYS])
    xs = {k: (x[k].clone().requires_grad_(True) if k in ("pm", "ps", "pe", "pa") else x[k] if x[k].dtype == torch.float32 else x[k] != 0)
          for k in LOSS_KEYS}
    v32 = loss_fn_torch(xs["pm"], xs["ym"], xs["sm"], xs["mm"], xs["ps"], xs["ys"], xs["ss"], xs["pe"], xs["ye"], xs["se"], xs["pa"], xs["ya"], xs["lm"])
    g32 = torch.autograd.grad(1.7 * v32, [xs[k] for k in ("pm", "ps", "pe", "pa")])
    _, p32 = loss_ref(*[x[k] if x[k].dtype == torch.float32 else x[k] != 0 for k in LOSS_KEYS])
    return (value, part, grads), (v32.detach(), p32, g32)


@pytest.mark.parametrize("case", LOSS_SAT_CASES, ids=[_loss_id(c) for c in LOSS_SAT_CASES])
def test_loss_saturated_inputs_hold_what_they_claim(case):
    """Every head with 36 valid positions or more (every head but ps, pe, pa of the L = 17 case, which hold every (p, label)) holds every combination of p in SAT_P (as fp32: 0 < 1e-45, 1 - 2^-24 < 1), both labels and -- for the three scaled
    heads -- the scale targets 0, 0.3, 1 at valid positions; loss_ref in float64 is the oracle's loss_fn there; every reference value is
    finite; the gradient is identically 0 where p equals its label at 0 or 1 and where the weight is 0."""
    x, where = _loss_saturated(case)
    p32 = torch.tensor(SAT_P, dtype=torch.float64).float()
    assert 0.0 < p32[1].item() < 1e-44 and p32[4].item() < 1.0 and p32[2].item() > 0.0
    for p, y, s, mask in HEADS:
        valid, ip, lab, js = where[p]
        seen = set(zip(ip.tolist(), lab.tolist(), js.tolist() if s else [0] * len(ip)))
        assert valid.numel() >= 36 or (case == LOSS_CASES[2] and p != "pm")
        if valid.numel() >= 36:
            assert seen == {(a, b, c) for a in range(6) for b in (0, 1) for c in (range(3) if s else (0,))}, p
        assert {(a, b) for a, b, _ in seen} == {(a, b) for a in range(6) for b in (0, 1)}, p
        assert torch.equal(x[p].view(-1)[valid], p32[ip]) and bool((x[p] >= 0).all() and (x[p] <= 1).all())
    (value, part, grads), (v32, part32, g32) = _loss_saturated_refs(case)
    xd = [x[k].double() if x[k].dtype == torch.float32 else x[k] for k in LOSS_KEYS]
    torch.testing.assert_close(loss_ref(*xd)[0], value, rtol=PIN_TOL, atol=PIN_TOL)
    assert all(bool(torch.isfinite(t).all()) for t in (value, part, v32, part32, *grads, *g32))
    for (p, y, s, mask), g in zip(HEADS, grads):
        valid, ip, lab, js = where[p]
        gv = g.reshape(-1)[valid]
        assert bool((gv[((ip == 0) & (lab == 0)) | ((ip == 5) & (lab == 1))] == 0).all())
        if s:
            assert bool((gv[((js == 0) & (lab == 1)) | ((js == 2) & (lab == 0))] == 0).all())
        assert gv.abs().max().item() > 1e7                                       # the floored quotient 1 / 1e-12 over B * count


def _loss_run(dev, x, B, L):
    """smin_loss_fwd / smin_loss_bwd at dloss = 1.7 into NaN-prefilled outputs: (loss, part, (dpm, dps, dpe, dpa))"""
    from vml_amd._lib import call, ptr, stream
    d = {k: v.to(dev) for k, v in x.items()}
    args = [ptr(d[k]) for k in LOSS_KEYS]
    loss, part = _nan((1,), dev), _nan((B, 6), dev)
    call("smin_loss_fwd", stream(), *args, B, L, ptr(loss), ptr(part))
    dloss = torch.tensor([1.7], device=dev)
    o = [_nan((B, L, L), dev)] + [_nan((B, L), dev) for _ in range(3)]
    call("smin_loss_bwd", stream(), ptr(dloss), ptr(part), *args, B, L, *[ptr(t) for t in o])
    torch.cuda.synchronize()
    return loss, part, o


@pytest.mark.gpu
@pytest.mark.parametrize("case", LOSS_SAT_CASES, ids=[_loss_id(c) for c in LOSS_SAT_CASES])
def test_loss_saturated_against_fp64(dev, case):
    """smin_loss_fwd / smin_loss_bwd on _loss_saturated: p at 0, fp32's smallest denormal, 1e-30, 0.5, 1 - 2^-24 and 1 under both labels
    and the scale targets 0, 0.3, 1, in all four heads -- logf(p), logf(1 - p) and p (1 - p) on their clamps.  Everything finite, masked
    positions exactly +0.0, and the project's gate for the value, each column of the partials, and the gradients of every (head, p, label)
    group taken on its own (a planted 0 or 1 gives a gradient near 1e11 that a whole tensor's max-norm would hide the rest behind; a
    group whose float64 gradient is identically 0 must be exactly 0).  Measured on an MI355X: INTEGRATION.md, "Saturated inputs"."""
    from tests.support.compare import gate
    B, L, _ = case
    x, where = _loss_saturated(case)
    (value, part0, grads0), (v32, part32, g32) = _loss_saturated_refs(case)
    tag = f"loss {_loss_id(case)}"
    loss, part, grads = _loss_run(dev, x, B, L)
    assert all(bool(torch.isfinite(t).all()) for t in (loss, part, *grads))
    gate(f"{tag} value", loss.reshape(()), value, v32)
    for k, name in enumerate(("sum_m", "cnt_m", "sum_s", "sum_e", "sum_a", "cnt_l")):
        gate(f"{tag} part {name}", part[:, k], part0[:, k], part32[:, k])
    for (p, y, s, mask), got, w, r in zip(HEADS, grads, grads0, g32):
        valid, ip, lab, js = where[p]
        got = got.cpu()
        assert bool((got.reshape(-1)[(x[mask] == 0).reshape(-1)].view(torch.int32) == 0).all()), p
        for a in range(6):
            for b in (0, 1):
                at = valid[(ip == a) & (lab == b)]
                gate(f"{tag} d{p} p = {SAT_P_NAMES[a]} y = {b}", got.reshape(-1)[at], w.reshape(-1)[at], r.reshape(-1)[at])


@pytest.mark.gpu
@pytest.mark.parametrize("case", LOSS_CASES, ids=[_loss_id(c) for c in LOSS_CASES])
def test_loss_fn_wrapper_equals_direct_calls(dev, case):
    """vml_amd.loss_fn (the autograd wrapper) on the same inputs: value and gradients bit for bit those of the direct calls."""
    import models  # noqa: F401
    from vml_amd import loss_fn
    d, loss, part, grads = _loss_direct(dev, case)
    leaves = {k: d[k].clone().requires_grad_(True) for k in ("pm", "ps", "pe", "pa")}
    a = {**d, **leaves}
    out = loss_fn(a["pm"], a["ym"], a["sm"], a["mm"], a["ps"], a["ys"], a["ss"], a["pe"], a["ye"], a["se"], a["pa"], a["ya"], a["lm"])
    assert torch.equal(out.detach().reshape(1), loss)
    (out * 1.7).backward()
    for k, g in zip(("pm", "ps", "pe", "pa"), grads):
        assert torch.equal(leaves[k].grad, g), (_loss_id(case), k)
