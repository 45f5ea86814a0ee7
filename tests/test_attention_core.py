"""The content unit's attention core (csrc/content_attn.hip) and the word-side operand kernels (csrc/word_prep.hip) against a
float64 restatement of the reference's formulas.

CPU: the restatement itself is pinned to the oracle's dense content unit (oracle/smin_oracle.py content_unit, _lin).
GPU: ContentAttnFn over every template instantiation SMIN_ATTN_DISPATCH can pick, the bf16-rows forward, the C ABI's refusals,
and WordPrepFn over a grid of (layers, batch, words, widths) that covers each row-partition regime of wp_rows_per_part."""
import ctypes
import math

import pytest
import torch

from tests import helpers as H
from tests.support.device import dev  # noqa: F401  (the module's device fixture)
from tests.support.compare import _rel, gate
from tests.support.references import (
    _attn_inputs, _layout_to, _ragged_mask, _smi_params, attn_core_ref, attn_form, word_side_ref, ALL_FORMS, WORD_PARAM_NAMES)

FWD_TOL = 1e-5          # max |got - ref| / max |ref|, per output and case (as test_standalone_attention_classes_against_oracle)
GRAD_TOL = 1e-4


# ---------------------------------------------------------------- float64 restatements
def form_name(form):
    dl, ws, exact = form
    return f"<{dl},{ws},{'T' if exact else 'F'}>"


# ---------------------------------------------------------------- CPU: the restatements against the oracle
@pytest.mark.parametrize("mask_kind", ["dense", "ragged"])
def test_core_restatement_matches_oracle_content_unit(mask_kind):
    """linear_c(core) * m + f_c + gate == oracle.content_unit in float64, the core fed from linear_c_hat and word_side_ref."""
    import models
    from oracle import smin_oracle as O
    B, L, C, D, dl, Nq = 3, 5, 4, 24, 16, 6
    p = "smis.0.content_unit."
    sd = _smi_params(D, dl, 1.5, 1)
    g = torch.Generator().manual_seed(2)
    if mask_kind == "dense":
        mm = torch.ones(B, L, L, dtype=torch.bool)
    else:
        mm = torch.rand(B, L, L, generator=g) < 0.6          # not a triangle; sample 2 below also loses whole rows
        mm[2, 1:3] = False
    qmask = torch.ones(B, Nq)
    qmask[1, 4:] = 0
    qmask[2, 1] = 0
    f_c = torch.randn(B, L, L, C, D, generator=g, dtype=torch.float64)
    f_m = torch.randn(B, L, L, D, generator=g, dtype=torch.float64)
    f_w = torch.randn(B, Nq, D, generator=g, dtype=torch.float64) * qmask.double().unsqueeze(-1)
    f_s = torch.randn(B, D, generator=g, dtype=torch.float64)
    want = O.content_unit(sd, p, f_c, f_w, f_s, f_m, qmask.unsqueeze(-1), mm)

    lay = models.vml_amd.CellLayout.from_mask(mm)
    m = lay.cells[:, 3].double()
    chat = (O._lin(sd, p + "linear_c_hat", lay.pack(f_c)) * m.view(-1, 1, 1)).reshape(-1, dl)
    (what, shat, _, Mq, uq), = word_side_ref(f_w, f_s, qmask.double(), [sd[p + n] for n in WORD_PARAM_NAMES])
    cc, ccmean, _ = attn_core_ref(chat, lay.cells, C, Mq, uq, what, shat, qmask.double())
    out = f_c + (torch.sigmoid(f_m * f_s[:, None, None, :]) * f_m).unsqueeze(3)
    out[lay.bidx, lay.iidx, lay.jidx] += (O._lin(sd, p + "linear_c", cc) * m.repeat_interleave(C).view(-1, 1)).reshape(-1, C, D)
    assert lay.N < B * L * L or mask_kind == "dense"
    torch.testing.assert_close(out, want, rtol=1e-12, atol=1e-12)
    # the clip mean is the mean of the rows the unit's linear map sees
    torch.testing.assert_close(ccmean, cc.reshape(-1, C, dl).mean(1), rtol=0, atol=0)


def test_core_restatement_masked_cells_are_zero():
    """all_cells layout: a cell with m = 0 gives cc = 0 and no gradient to its rows, whatever its rows hold."""
    import models
    B, L, C, dl, Nq = 2, 4, 3, 16, 5
    g = torch.Generator().manual_seed(3)
    mm = torch.rand(B, L, L, generator=g) < 0.5
    lay = models.vml_amd.CellLayout.all_cells(mm)
    chat = torch.randn(lay.N * C, dl, generator=g, dtype=torch.float64, requires_grad=True)
    Mq, what = (torch.randn(B, Nq, dl, generator=g, dtype=torch.float64) for _ in range(2))
    uq, shat = torch.randn(B, Nq, generator=g, dtype=torch.float64), torch.randn(B, dl, generator=g, dtype=torch.float64)
    cc, ccmean, _ = attn_core_ref(chat, lay.cells, C, Mq, uq, what, shat, torch.ones(B, Nq, dtype=torch.float64))
    (cc.sum() + ccmean.sum()).backward()
    dead = (lay.cells[:, 3] == 0).repeat_interleave(C)
    assert dead.any() and (~dead).any()
    assert torch.all(cc[dead] == 0) and torch.all(chat.grad[dead] == 0) and torch.all(cc[~dead].abs().sum(1) > 0)


def test_word_side_restatement_matches_oracle_projections():
    """word_side_ref against the oracle's own _lin calls: what / shat are linear_w_hat / linear_s_hat, and the folded operands give
    the reference's word scores W_q(c) . W_k(what)^T = c Mq^T + uq for any clip rows c."""
    from oracle import smin_oracle as O
    B, Nq, D, dl = 3, 7, 40, 16
    p = "smis.0.content_unit."
    sd = _smi_params(D, dl, 1.0, 4)
    g = torch.Generator().manual_seed(5)
    qmask = (torch.rand(B, Nq, generator=g) < 0.7).double()
    qmask[0, 2] = 0.4
    f_w, f_s = torch.randn(B, Nq, D, generator=g, dtype=torch.float64), torch.randn(B, D, generator=g, dtype=torch.float64)
    (what, shat, kb, Mq, uq), = word_side_ref(f_w, f_s, qmask, [sd[p + n] for n in WORD_PARAM_NAMES])
    torch.testing.assert_close(what, O._lin(sd, p + "linear_w_hat", f_w) * qmask.unsqueeze(-1), rtol=1e-13, atol=1e-13)
    torch.testing.assert_close(shat, O._lin(sd, p + "linear_s_hat", f_s), rtol=1e-13, atol=1e-13)
    torch.testing.assert_close(kb, O._lin(sd, p + "attn_layer.W_k", what), rtol=1e-13, atol=1e-13)
    c = torch.randn(B, 11, dl, generator=g, dtype=torch.float64)
    scores = O._lin(sd, p + "attn_layer.W_q", c) @ kb.transpose(1, 2)
    torch.testing.assert_close(c @ Mq.transpose(1, 2) + uq.unsqueeze(1), scores, rtol=1e-12, atol=1e-12)


# ---------------------------------------------------------------- the dispatch table

def _attn_cases():
    cases = []
    for dl in (16, 32, 64):
        cases += [(4, dl, nq) for nq in (1, 16, 17, 32)]
    cases += [(4, 128, nq) for nq in (1, 4, 16, 17, 18, 19, 20, 21, 24, 25, 31, 32)]
    cases += [(c, dl, nq) for c in (2, 3) for dl in (16, 32, 64, 128) for nq in (1, 13, 32)]
    cases += [(4, dl, nq) for dl in (48, 80, 96, 112) for nq in (1, 13, 32)]
    return cases


ATTN_CASES = _attn_cases()


def _attn_id(case):
    C, dl, Nq = case
    return f"{form_name(attn_form(C, dl, Nq))}-C{C}-dl{dl}-Nq{Nq}"


def test_attention_cases_reach_every_form():
    reached = {attn_form(*c) for c in ATTN_CASES}
    assert reached == set(ALL_FORMS), sorted(set(ALL_FORMS) - reached)
    # partly used extra-word slots (16 < Nq < 20) and every general form below its template width
    assert {17, 18, 19} <= {nq for c, dl, nq in ATTN_CASES if attn_form(c, dl, nq) == (128, 5, True)}
    assert {48, 80, 96, 112} <= {dl for c, dl, nq in ATTN_CASES if not attn_form(c, dl, nq)[2]}


ATTN_IN = ("chat", "Mq", "uq", "what", "shat")


def _attn_refs(C, lay, x, Wcc, Wm, dtype):
    """attn_core_ref in ``dtype``: (cc, ccmean, S, {flavour: the five gradients})"""
    ref_in = {k: v.detach().to(dtype).clone().requires_grad_(k in ATTN_IN) for k, v in x.items()}
    cc0, cm0, S0 = attn_core_ref(ref_in["chat"], lay.cells, C, ref_in["Mq"], ref_in["uq"], ref_in["what"], ref_in["shat"], ref_in["qmask"])
    Wcc, Wm = Wcc.to(dtype), Wm.to(dtype)
    refs = {}
    for flav, loss in (("mean2", (cc0 * Wcc).sum() + (cm0 * Wm).sum()), ("percell", (cm0 * Wm).sum()), ("plain", (cc0 * Wcc).sum())):
        refs[flav] = torch.autograd.grad(loss, [ref_in[k] for k in ATTN_IN], retain_graph=True)
    return cc0.detach(), cm0.detach(), S0.detach(), refs


def _run_attn_case(dev, C, dl, Nq, lay, x, label, check_masked=True, saturated=False):
    """Every forward and backward flavour of one case against attn_core_ref; returns the worst (forward, gradient) ratio.
    saturated: the case is run without the spread precondition, and every comparison is the project's gate (tests/support/compare.py)
    with e_torch32 from attn_core_ref in fp32, in place of the fixed bounds."""
    import models
    F = models.vml_amd.functional
    from vml_amd._lib import call, ptr, stream
    lay_d = _layout_to(lay, dev)
    B = x["Mq"].shape[0]
    N = lay.N
    g = torch.Generator().manual_seed(N + 7 * Nq + dl)
    Wcc, Wm = torch.randn(N * C, dl, generator=g, dtype=torch.float64), torch.randn(N, dl, generator=g, dtype=torch.float64)

    cc0, cm0, S0, refs = _attn_refs(C, lay, x, Wcc, Wm, torch.float64)
    if saturated:
        cc32, cm32, _, refs32 = _attn_refs(C, lay, x, Wcc.float(), Wm.float(), torch.float32)
        ref32_of = {id(cc0): cc32, id(cm0): cm32}
    else:
        # the word scores must be spread (a saturated softmax hides a dropped or extra word)
        live = (lay.cells[:, 3] != 0).view(-1, 1, 1) & (x["qmask"][lay.cells[:, 0].long()] != 0).unsqueeze(1)
        sd = S0[live.expand_as(S0)].std().item()
        assert 0.5 <= sd <= 3.0, f"{label}: word-score spread {sd:.3f}"

    d = {k: v.float().to(dev) for k, v in x.items()}
    Wcc_d, Wm_d = Wcc.float().to(dev), Wm.float().to(dev)
    worst_f = worst_g = 0.0

    def check_fwd(what, got, ref):
        nonlocal worst_f
        if saturated:
            return gate(f"attn {label} {what}", got, ref, ref32_of[id(ref)])
        e = _rel(got, ref)
        worst_f = max(worst_f, e)
        assert e <= FWD_TOL, (label, what, e)

    def check_grads(flav, got):
        nonlocal worst_g
        for k, (name, gg, rr) in enumerate(zip(ATTN_IN, got, refs[flav])):
            if saturated:
                gate(f"attn {label} {flav} d{name}", gg, rr, refs32[flav][k])
                continue
            e = _rel(gg, rr)
            worst_g = max(worst_g, e)
            assert e <= GRAD_TOL, (label, flav, "d" + name, e)

    def fwd_bwd(want_rows):
        leaves = {k: d[k].clone().requires_grad_(True) for k in ATTN_IN}
        cc, cm = F.ContentAttnFn.apply(leaves["chat"], leaves["Mq"], leaves["uq"], leaves["what"], leaves["shat"], d["qmask"], lay_d, C, want_rows)
        loss = (cm * Wm_d).sum() + ((cc * Wcc_d).sum() if want_rows else 0)
        grads = torch.autograd.grad(loss, [leaves[k] for k in ATTN_IN])
        return cc.detach(), cm.detach(), grads

    # rows + mean; backward on both outputs (MEAN2)
    cc, cm, grads = fwd_bwd(True)
    for got, ref in ((cc, cc0), (cm, cm0)):
        check_fwd("fwd rows+mean", got, ref)
    check_grads("mean2", grads)
    _, _, again = fwd_bwd(True)                                   # fixed-order slab sums: bit for bit
    assert all(torch.equal(a, b) for a, b in zip(grads, again)), (label, "backward not deterministic")
    # mean only; backward on the mean alone (PERCELL)
    cc_e, cm2, grads = fwd_bwd(False)
    assert cc_e.numel() == 0
    check_fwd("fwd mean only", cm2, cm0)
    check_grads("percell", grads)
    # rows only (plain): ContentAttnFn always hands the kernel both gradients, so this flavour is called through the C ABI
    dchat, dMq, duq, dwhat, dshat = (torch.empty_like(d[k]) for k in ATTN_IN)
    nb = models.vml_amd._lib.load().smin_content_attn_bwd_workspace_bytes(N, B, C, dl)
    ws = torch.empty(nb, dtype=torch.uint8, device=dev)
    call("smin_content_attn_bwd", stream(), ptr(Wcc_d), None, ptr(d["chat"]), ptr(lay_d.cells), ptr(lay_d.row_ptr), N, B, lay.L, C, dl, Nq,
         ptr(d["Mq"]), ptr(d["uq"]), ptr(d["what"]), ptr(d["shat"]), ptr(d["qmask"]), ptr(dchat), ptr(dMq), ptr(duq), ptr(dwhat), ptr(dshat),
         ptr(ws), nb)
    check_grads("plain", (dchat, dMq, duq, dwhat, dshat))

    if check_masked:
        dead = (lay.cells[:, 3] == 0)
        if dead.any():                                            # "masked cells get dchat = 0" (smin_hip.h); cc = 0 too
            rows = dead.repeat_interleave(C).to(dev)
            assert torch.all(cc[rows] == 0) and torch.all(cm[dead.to(dev)] == 0), label
            assert torch.all(grads[0][rows] == 0) and torch.all(dchat[rows] == 0), label
            assert torch.all(d["chat"][rows] != 0)
    print(f"attn {label}: worst fwd {worst_f:.2e} grad {worst_g:.2e}")
    return worst_f, worst_g


@pytest.mark.gpu
@pytest.mark.parametrize("layout", ["from_mask", "all_cells"])
@pytest.mark.parametrize("C,dl,Nq", ATTN_CASES, ids=[_attn_id(c) for c in ATTN_CASES])
def test_content_attn_dispatch_table(dev, C, dl, Nq, layout):
    """ContentAttnFn at one shape per (form, word count): forward rows + mean and mean only, backward on both outputs (MEAN2), on the
    mean (PERCELL) and on the rows (plain), on a ragged non-triangular cell list (from_mask) and on every cell with masked ones
    (all_cells); query masks with a prefix, holes, fractional weights and no word at all."""
    g = torch.Generator().manual_seed(1000 * C + 10 * dl + Nq)
    mask = _ragged_mask(4, 6, g)
    lay, x = _attn_inputs(C, dl, Nq, mask, layout == "all_cells", seed=C + dl + Nq)
    assert layout == "from_mask" or bool((lay.cells[:, 3] == 0).any())
    _run_attn_case(dev, C, dl, Nq, lay, x, f"{_attn_id((C, dl, Nq))}-{layout}")


# ---------------------------------------------------------------- saturated word softmax

LEVELS = ("hard", "frozen")


def _saturated_attn_cases():
    """Per form of the dispatch table its smallest existing case with more than one word, a word count that is no multiple of 4 where
    the form has one (the -inf tail of the last word slot)"""
    picked = []
    for form in ALL_FORMS:
        cands = [c for c in ATTN_CASES if attn_form(*c) == form and c[2] > 1]
        if not form[2]:                                      # the general forms: C = 2 and C = 3 in turn
            cands = [c for c in cands if c[0] == (3 if form[0] in (32, 128) else 2)]
        odd = [c for c in cands if c[2] % 4]
        picked.append(min(odd or cands, key=lambda c: (c[0] * c[1] * c[2], c)))
    return picked


SAT_ATTN_CASES = _saturated_attn_cases()


def _word_probs(x, lay, C):
    """(the word softmax P [N, C, Nq] of attn_core_ref, its masked logits) in the dtype of x"""
    S = attn_core_ref(x["chat"], lay.cells, C, x["Mq"], x["uq"], x["what"], x["shat"], x["qmask"])[2]
    qm = x["qmask"][lay.cells[:, 0].long()].unsqueeze(1)
    S = (S * qm).masked_fill(qm == 0, -1e9)
    return torch.softmax(S, dim=-1), S


def _saturated_attn_inputs(C, dl, Nq, level):
    """test_content_attn_dispatch_table's all_cells inputs with Mq and uq -- the word logits are linear in them -- scaled by the factor
    the float64 reference asks for: frozen -- the live logits' standard deviation becomes 100; hard -- samples 0 and 2 by the smallest
    power of 2 at which a quarter of all live rows have a largest probability above 1 - 1e-6, sample 1 as it is (a quarter of all
    live rows below 0.9; one factor for all rows cannot give both: the gap between a row's two largest logits of 16 is too evenly
    spread)."""
    g = torch.Generator().manual_seed(1000 * C + 10 * dl + Nq)
    lay, x = _attn_inputs(C, dl, Nq, _ragged_mask(4, 6, g), True, seed=C + dl + Nq)
    live_rows = ((lay.cells[:, 3] != 0).view(-1, 1) & (x["qmask"][lay.cells[:, 0].long()] != 0).any(1, keepdim=True)).expand(-1, C)
    def scaled(k, samples=(0, 1, 2, 3)):
        f = torch.ones(x["Mq"].shape[0], dtype=torch.float64)
        f[list(samples)] = k
        return dict(x, Mq=(f.view(-1, 1, 1) * x["Mq"]).float().double(), uq=(f.view(-1, 1) * x["uq"]).float().double())
    if level == "frozen":
        S = _word_probs(x, lay, C)[1]
        live = live_rows.unsqueeze(-1) & (S > -1e8)
        return lay, scaled(100.0 / S[live].std().item()), live_rows
    for e in range(1, 12):                                  # samples 0 and 2 are driven into saturation, sample 1 keeps its spread
        y = scaled(2.0 ** e, (0, 2))
        top = _word_probs(y, lay, C)[0].max(-1).values[live_rows]
        if (top > 1 - 1e-6).double().mean().item() >= 0.25 and (top < 0.9).double().mean().item() >= 0.25:
            return lay, y, live_rows
    raise AssertionError(f"no scale puts C{C}-dl{dl}-Nq{Nq} into the hard regime")


def test_saturated_attention_cases_reach_every_form():
    assert {attn_form(*c) for c in SAT_ATTN_CASES} == set(ALL_FORMS) and len(SAT_ATTN_CASES) == len(ALL_FORMS)
    assert any(c[2] % 4 for c in SAT_ATTN_CASES) and {2, 3} <= {c[0] for c in SAT_ATTN_CASES}       # the -inf word tail; absent clips


@pytest.mark.parametrize("level", LEVELS)
@pytest.mark.parametrize("C,dl,Nq", SAT_ATTN_CASES, ids=[_attn_id(c) for c in SAT_ATTN_CASES])
def test_saturated_attention_inputs_hold_what_they_claim(C, dl, Nq, level):
    """On the float64 reference.  hard: at least a quarter of the live word-softmax rows have a largest probability above 1 - 1e-6 and
    at least a quarter below 0.9.  frozen: the live logits' standard deviation is 100 (to 1 %), at least 60 % of the rows are one-hot to
    1e-6 and 95 % have one word above 0.5 (two of 16 logits at that spread are sometimes within a few units of each other).
    Both: a sample whose query mask is all zero is there, every logit of it is -1e9 and its softmax uniform; masked cells are listed."""
    lay, x, live_rows = _saturated_attn_inputs(C, dl, Nq, level)
    P, S = _word_probs(x, lay, C)
    top = P.max(-1).values[live_rows]
    if level == "hard":
        assert (top > 1 - 1e-6).double().mean().item() >= 0.25 and (top < 0.9).double().mean().item() >= 0.25
    else:
        sd = S[live_rows.unsqueeze(-1) & (S > -1e8)].std().item()
        assert abs(sd - 100) <= 1.0 and (top > 1 - 1e-6).double().mean().item() >= 0.6 and (top > 0.5).double().mean().item() >= 0.95
    blank = (x["qmask"] == 0).all(1)
    of_blank = blank[lay.cells[:, 0].long()]
    assert bool(blank.any()) and bool(of_blank.any()) and bool((S[of_blank] == -1e9).all())
    assert (P[of_blank] - 1.0 / Nq).abs().max().item() <= 1e-15 and bool((lay.cells[:, 3] == 0).any())
    assert all(bool(torch.isfinite(v).all()) for v in x.values())


@pytest.mark.gpu
@pytest.mark.parametrize("level", LEVELS)
@pytest.mark.parametrize("C,dl,Nq", SAT_ATTN_CASES, ids=[_attn_id(c) for c in SAT_ATTN_CASES])
def test_content_attn_saturated_word_softmax(dev, C, dl, Nq, level):
    """smin_content_attn_fwd and _bwd (ContentAttnFn's three flavours and the C ABI's rows-only backward) and smin_content_attn_fwd_probs
    with the word softmax partly (hard) or wholly (frozen) one-hot, a sample without a word, word counts that leave the last slot's
    tail at -inf, and C < 4: everything finite, masked cells exactly 0, and the project's gate against attn_core_ref in float64 with
    e_torch32 from attn_core_ref in fp32.  Measured on an MI355X: INTEGRATION.md, "Saturated inputs"."""
    from vml_amd._lib import call, ptr, stream
    lay, x, live_rows = _saturated_attn_inputs(C, dl, Nq, level)
    label = f"{_attn_id((C, dl, Nq))} {level}"
    _run_attn_case(dev, C, dl, Nq, lay, x, label, saturated=True)
    ld = _layout_to(lay, dev)
    d = {k: v.float().to(dev).contiguous() for k, v in x.items()}
    N, B = lay.N, x["Mq"].shape[0]
    probs, cm = torch.full((N * C, Nq), float("nan"), device=dev), torch.full((N, dl), float("nan"), device=dev)
    call("smin_content_attn_fwd_probs", stream(), ptr(d["chat"]), ptr(ld.cells), ptr(ld.row_ptr), N, B, ld.L, C, dl, Nq, ptr(d["Mq"]), ptr(d["uq"]),
         ptr(d["what"]), ptr(d["shat"]), ptr(d["qmask"]), None, 0, ptr(cm), ptr(probs))
    torch.cuda.synchronize()
    rows = (lay.cells[:, 3] != 0).repeat_interleave(C)                            # (the rows of the sample without a word too: uniform)
    want = _word_probs(x, lay, C)[0].reshape(N * C, Nq)
    ref32 = _word_probs({k: v.float() for k, v in x.items()}, lay, C)[0].reshape(N * C, Nq)
    assert bool(torch.isfinite(probs.cpu()[rows]).all())
    gate(f"attn {label} probs", probs.cpu()[rows], want[rows], ref32[rows])
    off = (x["qmask"][lay.cells[:, 0].long()] == 0).unsqueeze(1).expand(-1, C, -1).reshape(N * C, Nq)
    assert bool((probs.cpu()[live_rows.reshape(-1, 1) & off] == 0).all())        # a masked word beside live ones: exactly 0


def _range_cells(N, slots):
    """Cells per range (csrc/content_attn.hip range_cells): whole tiles of 4 cells, at least 16."""
    per_slot = -(-N // slots)
    return max(-(-per_slot // 4) * 4, 16)


@pytest.mark.gpu
@pytest.mark.parametrize("C,dl,Nq", [(4, 64, 13), (3, 48, 9)], ids=["<64,4,T>", "<64,8,F>"])
def test_content_attn_ranges_cross_many_samples(dev, C, dl, Nq):
    """37 small samples with 0, 1, 5, 17, .. cells: the 16-cell ranges of both directions straddle samples, some samples are empty."""
    import models
    g = torch.Generator().manual_seed(37)
    B, L = 37, 8
    counts = [0, 1, 5, 17, 3, 0, 9, 1, 30, 2]
    mask = torch.zeros(B, L, L, dtype=torch.bool)
    for b in range(B):
        k = counts[b % len(counts)]
        mask[b].view(-1)[torch.randperm(L * L, generator=g)[:k]] = True
    lay, x = _attn_inputs(C, dl, Nq, mask, False, seed=99)
    sizes = torch.bincount(lay.cells[:, 0].long(), minlength=B)
    assert {0, 1, 5, 17} <= set(sizes.tolist()) and bool((sizes[1:-1] == 0).any())
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    assert _range_cells(lay.N, 3 * cus) == 16 and _range_cells(lay.N, 2 * cus) == 16 and lay.N > 2 * 16
    _run_attn_case(dev, C, dl, Nq, lay, x, f"ranges-B{B}-{form_name(attn_form(C, dl, Nq))}")


@pytest.mark.gpu
def test_content_attn_large_ranges(dev):
    """B = 8, L = 64, full triangle (16 640 cells), <128,5,T>: every range of either direction holds more than 16 cells."""
    B, L, C, dl, Nq = 8, 64, 4, 128, 20
    mask = torch.triu(torch.ones(L, L, dtype=torch.bool)).expand(B, L, L).contiguous()
    lay, x = _attn_inputs(C, dl, Nq, mask, False, seed=8)
    assert lay.N == 16640
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    assert _range_cells(lay.N, 3 * cus) > 16 and _range_cells(lay.N, 2 * cus) > 16, (lay.N, cus)
    _run_attn_case(dev, C, dl, Nq, lay, x, "large-B8-L64-<128,5,T>")


BF16_CASES = [(4, 128, 20), (4, 16, 32), (4, 48, 13), (4, 112, 32), (3, 64, 7), (2, 32, 32)]


@pytest.mark.gpu
@pytest.mark.parametrize("C,dl,Nq", BF16_CASES, ids=[_attn_id(c) for c in BF16_CASES])
def test_content_attn_bf16_rows_forward(dev, C, dl, Nq):
    """smin_content_attn_fwd_cch: the rows are the fp32 launch's rows rounded to nearest even, the clip mean is the fp32 launch's
    (both come from the unrounded rows)."""
    import models
    from vml_amd._lib import call, ptr, stream
    g = torch.Generator().manual_seed(5 + dl)
    lay, x = _attn_inputs(C, dl, Nq, _ragged_mask(4, 6, g), True, seed=dl + Nq)
    lay_d = _layout_to(lay, dev)
    d = {k: v.float().to(dev) for k, v in x.items()}
    N, B = lay.N, 4
    args = (ptr(d["Mq"]), ptr(d["uq"]), ptr(d["what"]), ptr(d["shat"]), ptr(d["qmask"]))
    cc, cm = torch.empty(N * C, dl, device=dev), torch.empty(N, dl, device=dev)
    call("smin_content_attn_fwd", stream(), ptr(d["chat"]), ptr(lay_d.cells), ptr(lay_d.row_ptr), N, B, lay.L, C, dl, Nq, *args, ptr(cc), ptr(cm))
    cch = torch.full((N * C, dl), float("nan"), dtype=torch.bfloat16, device=dev)
    cm_h = torch.full((N, dl), float("nan"), device=dev)
    call("smin_content_attn_fwd_cch", stream(), ptr(d["chat"]), ptr(lay_d.cells), ptr(lay_d.row_ptr), N, B, lay.L, C, dl, Nq, *args,
         ctypes.c_void_p(cch.data_ptr()), ptr(cm_h))
    assert torch.equal(cch.view(torch.int16), cc.to(torch.bfloat16).view(torch.int16))
    assert torch.equal(cm_h, cm)


@pytest.mark.gpu
def test_content_attn_c_abi_refusals(dev):
    """Sizes outside the kernels' table are refused with a negative code before anything runs; N = 0 is a no-op."""
    import models
    from vml_amd._lib import ptr, stream
    lib = models.vml_amd._lib.load()
    B, L, N = 2, 4, 6
    big = torch.zeros(1 << 16, device=dev)                       # generous for every size tried
    cells = torch.zeros(N, 4, dtype=torch.int32, device=dev)
    row_ptr = torch.zeros(B * L + 1, dtype=torch.int32, device=dev)
    ws = torch.zeros(1 << 20, dtype=torch.uint8, device=dev)
    P = ptr(big)

    def fwd(N, C, dl, Nq):
        return lib.smin_content_attn_fwd(stream(), P, ptr(cells), ptr(row_ptr), N, B, L, C, dl, Nq, P, P, P, P, P, P, P)

    def fwd_h(N, C, dl, Nq):
        return lib.smin_content_attn_fwd_cch(stream(), P, ptr(cells), ptr(row_ptr), N, B, L, C, dl, Nq, P, P, P, P, P, P, P)

    def bwd(N, C, dl, Nq):
        return lib.smin_content_attn_bwd(stream(), P, P, P, ptr(cells), ptr(row_ptr), N, B, L, C, dl, Nq, P, P, P, P, P, P, P, P, P, P,
                                         ptr(ws), ws.numel())
    for C, dl, Nq in ((4, 40, 8), (4, 144, 8), (5, 32, 8), (4, 32, 0), (4, 32, 33), (1, 32, 8), (4, 0, 8)):
        for f in (fwd, fwd_h, bwd):
            assert f(N, C, dl, Nq) < 0, (f.__name__, C, dl, Nq)
    for f in (fwd, fwd_h, bwd):
        assert f(0, 4, 32, 8) == 0, f.__name__
    torch.cuda.synchronize()


# ---------------------------------------------------------------- word-side operands

def wp_parts(nl, B, Nq, D, dl):
    """Row parts of one (sample, layer) in csrc/word_prep.hip (wp_rows_per_part), for the case list's coverage check."""
    fwd = lambda r: 4 * ((r + 1) * D + 2 * r * dl)
    bwd = lambda r: 4 * (r * D + 5 * r * dl + 32 + dl)
    parts = min(max(-(-384 // (nl * B)), 1), Nq)
    while parts < Nq and (fwd(-(-Nq // parts)) > 160 * 1024 or bwd(-(-Nq // parts)) > 160 * 1024):
        parts += 1
    rpp = -(-Nq // parts)
    return -(-Nq // rpp), rpp


# (nl, B, Nq, D, dl, layers whose Mq / uq / shat gradient is None)
WP_CASES = [
    (1, 1, 1, 32, 16, ()), (1, 1, 7, 40, 48, ()), (1, 1, 17, 520, 128, (0,)), (1, 1, 32, 40, 16, ()),
    (3, 1, 32, 520, 48, (2,)), (3, 1, 17, 32, 128, ()), (8, 1, 7, 40, 16, (7,)), (8, 1, 32, 32, 128, (3, 7)),
    (1, 5, 32, 32, 48, ()), (1, 5, 17, 520, 16, ()), (3, 5, 7, 40, 128, (2,)), (3, 5, 32, 520, 128, ()),
    (8, 5, 17, 32, 48, (7,)), (8, 5, 1, 40, 16, ()), (8, 5, 32, 40, 128, (0, 7)), (3, 5, 1, 520, 48, ()),
    (1, 64, 32, 40, 16, ()), (1, 64, 17, 520, 128, ()), (1, 64, 7, 32, 48, (0,)), (3, 64, 17, 32, 16, ()),
    (3, 64, 32, 40, 128, (2,)), (3, 64, 7, 520, 48, ()), (3, 64, 1, 32, 128, ()), (8, 64, 32, 520, 16, (7,)),
    (8, 64, 17, 40, 128, ()), (8, 64, 7, 32, 48, (1, 7)), (8, 64, 32, 32, 48, ()), (1, 64, 1, 520, 16, ()),
    (3, 128, 32, 520, 128, ()), (8, 5, 32, 520, 48, (4,)),
]


def _wp_id(case):
    nl, B, Nq, D, dl, none = case
    parts, rpp = wp_parts(nl, B, Nq, D, dl)
    tag = "1part" if parts == 1 else f"{parts}parts" + ("-ragged" if Nq % rpp else "")
    return f"nl{nl}-B{B}-Nq{Nq}-D{D}-dl{dl}-{tag}" + ("-none" + "".join(map(str, none)) if none else "")


def test_word_prep_cases_cover_grid_and_partitions():
    for i, vals in enumerate(((1, 3, 8), (1, 5, 64), (1, 7, 17, 32), (32, 40, 520), (16, 48, 128))):
        assert set(vals) <= {c[i] for c in WP_CASES}
    parts = [wp_parts(*c[:5]) for c in WP_CASES]
    assert any(p == 1 for p, _ in parts) and any(p >= 8 for p, _ in parts)
    assert any(p > 1 and nq % r for (p, r), nq in zip(parts, (c[2] for c in WP_CASES)))
    assert any(c[5] for c in WP_CASES)


def _wp_inputs(nl, B, Nq, D, dl, seed):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    fw, fs = r(B, Nq, D), r(B, D)
    qm = torch.ones(B, Nq, dtype=torch.float64)
    for b in range(B):
        qm[b, max(1, Nq - b % 5):] = 0
    qm[B // 2, 0] = 0.6
    fw = fw * (qm != 0).unsqueeze(-1)
    params = []
    for _ in range(nl):
        params += [r(dl, D) / math.sqrt(D), 0.1 * r(dl), r(dl, D) / math.sqrt(D), 0.1 * r(dl),
                   r(dl, dl) / math.sqrt(dl), 0.1 * r(dl), r(dl, dl) / math.sqrt(dl), 0.1 * r(dl)]
    fp32 = lambda t: t.float().double()                        # the kernels' fp32 inputs, exactly
    return fp32(fw), fp32(fs), fp32(qm), [fp32(p) for p in params]


def _run_word_prep(dev, nl, B, Nq, D, dl, none_layers, label):
    import models
    F = models.vml_amd.functional
    fw, fs, qm, params = _wp_inputs(nl, B, Nq, D, dl, seed=nl * 1000 + B * 10 + Nq + D + dl)
    g = torch.Generator().manual_seed(B + D)
    # gradient weights of (what, shat, Mq, uq) per layer; None for the listed layers' shat, Mq and uq
    W = []
    for k in range(nl):
        for j, shp in enumerate(((B, Nq, dl), (B, dl), (B, Nq, dl), (B, Nq))):
            W.append(None if (k in none_layers and j > 0) else torch.randn(*shp, generator=g, dtype=torch.float64))
    ref_in = [t.clone().requires_grad_(True) for t in [fw, fs] + params]
    outs = [o for lay in word_side_ref(ref_in[0], ref_in[1], qm, ref_in[2:]) for i, o in enumerate(lay) if i != 2]   # what, shat, Mq, uq
    loss = sum((o * w).sum() for o, w in zip(outs, W) if w is not None)
    ref_g = [torch.zeros_like(t) if gg is None else gg for t, gg in zip(ref_in, torch.autograd.grad(loss, ref_in, allow_unused=True))]

    d_in = [t.float().to(dev).requires_grad_(True) for t in [fw, fs] + params]
    got = F.WordPrepFn.apply(d_in[0], d_in[1], qm.float().to(dev), *d_in[2:])
    worst_f = worst_g = 0.0
    for i, (o, r) in enumerate(zip(got, outs)):
        e = _rel(o.detach(), r.detach())
        worst_f = max(worst_f, e)
        assert e <= FWD_TOL, (label, "fwd", i, e)
    # WordPrepFn's own backward with None for the absent gradients (autograd would hand it zeros): _ptr_array_opt's NULL entries
    grads = [None if w is None else w.float().to(dev) for w in W]
    dfw, dfs, _, *dparams = F.WordPrepFn.backward(got[0].grad_fn, *grads)
    for i, (o, r) in enumerate(zip([dfw, dfs] + dparams, ref_g)):
        e = _rel(o, r)
        worst_g = max(worst_g, e)
        assert e <= GRAD_TOL, (label, "grad", i, e)
    print(f"word_prep {label}: worst fwd {worst_f:.2e} grad {worst_g:.2e}")


@pytest.mark.gpu
@pytest.mark.parametrize("case", WP_CASES, ids=[_wp_id(c) for c in WP_CASES])
def test_word_prep_against_fp64(dev, case):
    nl, B, Nq, D, dl, none = case
    _run_word_prep(dev, nl, B, Nq, D, dl, none, _wp_id(case))


@pytest.mark.gpu
def test_word_prep_large_width_fits_lds(dev):
    """nl * B >= 384 used to give one part of the whole query: at D = 768, dl = 128 the backward's LDS image (180 KB) was refused."""
    _run_word_prep(dev, 3, 128, 32, 768, 128, (), "nl3-B128-Nq32-D768-dl128")


@pytest.mark.gpu
def test_python_host_step_at_h384(dev):
    """SMIN at H = 384 (torch LSTM, Python host, WordPrepFn at D = 768 with B = 128): forward and backward against the oracle."""
    import models
    from oracle import smin_oracle as O
    from vml_amd import loss_fn
    T, L, C, D, dl, layers, Din, Nq, Hh, B = 16, 4, 4, 768, 128, 3, 16, 32, 384, 128
    sd = O.formula_state_dict(H.smin_shapes(T, L, C, D, dl, layers, Din, Nq, Hh), gain=1.2)
    batch = O.synthetic_batch(B, T, L, Nq, Din, seed=384)
    sdg = {k: v.clone().requires_grad_(True) for k, v in sd.items()}
    ref = O.smin_forward(sdg, dict(T=T, L=L, C=C), *H.model_inputs(batch))
    O.loss_fn(ref[0], batch["ym"], batch["sm"], batch["moment_mask"], ref[1], batch["ys"], batch["ss"], ref[2], batch["ye"], batch["se"],
              ref[3], batch["ya"], batch["length_mask"]).backward()
    m = models.SMIN(T, L, C, D, dl, layers, Din, Nq, Hh, dev)
    m.load_state_dict(sd)
    m = m.to(dev)
    b = {k: v.to(dev) for k, v in batch.items()}
    xs = H.model_inputs(b)
    assert m._plan(xs[0], xs[2]) == "stream"
    out = m(*xs)
    for got, want in zip(out, ref):
        assert (got.detach().cpu() - want.detach()).abs().max().item() < 2e-5
    loss_fn(out[0], b["ym"], b["sm"], b["moment_mask"], out[1], b["ys"], b["ss"], out[2], b["ye"], b["se"], out[3], b["ya"], b["length_mask"]).backward()
    for k, p in m.named_parameters():
        want = sdg[k].grad
        assert (p.grad.cpu() - want).abs().max().item() <= 2e-3 * want.abs().max().item() + 1e-7, k
