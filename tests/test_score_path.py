"""The forward-only scoring path: csrc/score_tail.hip (the last layer's content-stream sum, moment unit and the map's score head
collapsed to row dots), smin_hip::smin_score and SMIN.score / SMIN.forward_only_scoring.

Host: the C ABI and operator surface, the collapsed formula (functional.score_tail_torch) on the oracle's seams against the golden pm,
and that the GPU case list reaches every form of the tail's launcher.
GPU: the kernel against the as-written formulas in fp64 -- gated by the error of the existing chain smin_linear_rows_fwd ->
smin_moment_unit_fwd -> smin_score_map_fwd on the same inputs --, SMIN.score against the golden outputs and the CPU oracle in every
contraction mode, that nothing else moved, the fall-backs, repeatability and the peak of allocated memory."""
import math
import os
import re

import numpy as np
import pytest
import torch

from tests import helpers as H
from tests.support.device import dev  # noqa: F401  (the module's device fixture)
from tests.support.device import vml as V
from tests.support.compare import layout_ok
from tests.support.corpora import build_model, NATIVE_ROWS, SCORE_TOL
from tests.support.references import collapsed_pm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------- host: surface
def test_header_and_table_declare_the_tail():
    text = open(os.path.join(ROOT, "include", "smin_hip.h")).read()
    for name in ("smin_score_tail_ws_bytes", "smin_score_tail_fwd"):
        assert re.search(r"\b(size_t|int)\s+" + name + r"\s*\(", text), name
        assert name in V()._lib.SIGNATURES, name
    assert "#define SMIN_HIP_ABI_VERSION 2" in text
    lib = V()._lib.load()
    assert lib.smin_score_tail_ws_bytes(2, 8, 64, 16) >= 4 * (2 * 64 + 16 + 1)


def test_score_operator_is_registered_and_refuses_cpu():
    import models
    ops = V()._lib.load_torch()
    schema = str(torch.ops.smin_hip.smin_score.default._schema)
    for name in ("video_features", "video_mask", "query_features", "query_mask", "length_mask", "moment_mask", "Tensor[] params", "int T", "int L",
                 "int C", "int num_smi_layers", "int max_query_length", "int lstm_hidden_size", "*, bool overlap_boundary", "bool overlap_prep",
                 "bool param_prep_kernel", "bool bf16_operand_storage", "int? known_cell_count", "-> (Tensor, Tensor, Tensor, Tensor)"):
        assert name in schema, schema
    for name in ("async_weights", "grad_sync", "tail_split", "input_grads", "attention"):
        assert name not in schema, schema
    m = models.SMIN(16, 8, 4, 32, 16, 2, 24, 5, 16)
    assert set(m._score_options()) == {"overlap_boundary", "overlap_prep", "param_prep_kernel", "bf16_operand_storage", "known_cell_count"}
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.smin_score(torch.zeros(2, 16, 24), torch.ones(2, 16, 1, dtype=torch.uint8), torch.zeros(2, 5, 300), torch.ones(2, 5, 1, dtype=torch.uint8),
                       torch.ones(2, 8, dtype=torch.bool), torch.ones(2, 8, 8, dtype=torch.bool), m._native_params(), 16, 8, 4, 2, 5, 16, **m._score_options())


def test_score_fails_loudly_on_cpu_and_switch_is_off():
    import models
    from oracle import smin_oracle as O
    assert models.SMIN.forward_only_scoring is False
    m = models.SMIN(16, 8, 4, 32, 16, 1, 24, 5, 16)
    with pytest.raises(V()._lib.SminHipError, match="no CPU fallback"):
        m.score(*H.model_inputs(O.synthetic_batch(2, 16, 8, 5, 24)))


# ---------------------------------------------------------------- host: the collapsed formula on the oracle's seams
@pytest.mark.parametrize("name", H.TINY)
def test_collapsed_formula_reproduces_golden_pm(name):
    from oracle import smin_oracle as O
    cfg, sd, batch, out, _, _ = H.split_tiny(H.load_npz(name))
    with torch.no_grad():
        _, seams = O.smin_forward(sd, cfg, *H.model_inputs(batch), return_seams=True)
        pm = collapsed_pm(sd, seams, batch, O.num_layers(sd))
    err = (pm - out["pm"]).abs().max().item()
    print(name, "collapsed fp32 vs golden pm", err)
    assert err < SCORE_TOL
    assert pm[~batch["moment_mask"].bool()].abs().max().item() == 0.0


# ---------------------------------------------------------------- the kernel's dispatch table
TAIL_CPW, TAIL_WAVES = 8, 4          # csrc/score_tail.hip: cells per wave, waves per workgroup of the streaming pass
# B, L, D, dl, hbar given, lengths (valid snippets per sample; None = L for all)
TAIL_CASES = [
    (1, 8, 64, 16, True, None),
    (1, 8, 64, 16, False, [5]),
    (17, 8, 104, 48, True, [1 + (3 * b) % 8 for b in range(17)]),
    (17, 8, 104, 48, False, None),
    (3, 64, 512, 128, True, [64, 37, 50]),
    (2, 64, 512, 128, False, [61, 64]),
    (2, 8, 256, 128, True, [7, 8]),
    (3, 8, 260, 16, False, [8, 3, 7]),
    (2, 8, 640, 32, True, [6, 8]),
    (2, 8, 640, 32, False, None),
    (2, 8, 64, 16, True, [0, 0]),          # N = 0
]


def tail_form(D, dl):
    """NV of score_tail_kernel as smin_score_tail_fwd picks it (0: vectors read per cell)."""
    return 0 if (dl > 256 or D > 512) else 2 if D > 256 else 1


def tail_count(case):
    B, L, D, dl, has_hbar, lens = case
    return sum(n * (n + 1) // 2 for n in (lens or [L] * B))


def test_tail_cases_reach_every_form():
    """Every (NV, hbar given / re-formed) instance of score_tail_kernel, D and dl that leave lanes idle, a ragged last workgroup and
    wave, both L, B = 1 and 17, and the empty list."""
    reached = {(tail_form(c[2], c[3]), c[4]) for c in TAIL_CASES if tail_count(c) > 0}
    assert reached == {(nv, hb) for nv in (0, 1, 2) for hb in (True, False)}
    assert {c[2] for c in TAIL_CASES} >= {64, 104, 512} and {c[3] for c in TAIL_CASES} >= {16, 48, 128}
    assert {c[1] for c in TAIL_CASES} >= {8, 64} and {c[0] for c in TAIL_CASES} >= {1, 17}
    counts = [tail_count(c) for c in TAIL_CASES]
    assert 0 in counts
    assert any(n % (TAIL_CPW * TAIL_WAVES) not in (0,) and n % TAIL_CPW != 0 for n in counts)
    assert any(n > TAIL_CPW * TAIL_WAVES for n in counts)
    assert any(c[2] % 256 != 0 and c[2] > 256 for c in TAIL_CASES)          # a second register slot that is partly idle
    lib = V()._lib.load()
    for B, L, D, dl, _, _ in TAIL_CASES:                                    # the workspace holds a, c, u and k0
        assert lib.smin_score_tail_ws_bytes(B, L, D, dl) >= 4 * (2 * D + dl + 1)


# ---------------------------------------------------------------- GPU
def tail_inputs(case, seed):
    B, L, D, dl, has_hbar, lens = case
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g)
    u_ = lambda fan, *s: (torch.rand(*s, generator=g) * 2 - 1) / math.sqrt(fan)
    lens = lens or [L] * B
    mask = torch.zeros(B, L, L, dtype=torch.bool)
    for b, n in enumerate(lens):
        mask[b, :n, :n] = torch.ones(n, n).triu().bool()
    b_idx, i_idx, j_idx = mask.nonzero(as_tuple=True)                        # sorted by (b, i, j), as the cell list
    N = b_idx.numel()
    t = dict(fm=r(N, D) * 0.5, cumean=r(N, D) * 0.5, ccmean=r(N, dl) * 0.5, fs=r(B, D), bu=r(B, L, D) * 0.5,
             Wc=u_(dl, D, dl), bc=u_(dl, D), Wfb=u_(D, D, D), Wfc=u_(D, D, D), bfb=u_(D, D), bfc=u_(D, D), wm=u_(D, D), bm=u_(D, 1),
             wb=u_(D, 3, D), bb=u_(D, 3))
    t["hbar"] = torch.sigmoid(t["fm"] * t["fs"][b_idx]) * t["fm"]
    t["lmask"] = (torch.arange(L).unsqueeze(0) < torch.tensor(lens).unsqueeze(1)).float()
    return t, mask, (b_idx, i_idx, j_idx)


def written_fp64(t, idx, has_hbar):
    """The as-written formulas in fp64 on the fp32 inputs: cum, [x1 | cum] Wcat^T + bcat + fm, the head.  Logits of the listed cells."""
    c = {k: v.double() for k, v in t.items()}
    b_idx, i_idx, j_idx = idx
    hbar = c["hbar"] if has_hbar else torch.sigmoid(c["fm"] * c["fs"][b_idx]) * c["fm"]
    cum = c["ccmean"] @ c["Wc"].t() + c["bc"] + c["cumean"] + hbar
    x1 = c["bu"][b_idx, i_idx] * c["bu"][b_idx, j_idx]
    mu = x1 @ c["Wfb"].t() + cum @ c["Wfc"].t() + (c["bfb"] + c["bfc"]) + c["fm"]
    return mu @ c["wm"] + c["bm"]


@pytest.mark.gpu
@pytest.mark.parametrize("case", TAIL_CASES, ids=lambda c: "B%d-L%d-D%d-dl%d-%s-N%d" % (c[0], c[1], c[2], c[3], "hbar" if c[4] else "gate", tail_count(c)))
def test_tail_kernel_against_fp64(dev, case):
    """err_new <= 2 * err_old + 2.4e-7 on pm against the as-written fp64 formulas, err_old the existing chain's error on the same inputs
    (both are fp32 sums of the same products in different orders: a factor of two plus two ulps at 1.0 separates a reordering from a
    mistake, which moves pm by 1e-2 on these inputs).  psea bit for bit, cells outside the list exactly 0."""
    F, (call, ptr, stream) = V().functional, (V()._lib.call, V()._lib.ptr, V()._lib.stream)
    B, L, D, dl, has_hbar, lens = case
    t, mask, idx = tail_inputs(case, seed=B * 1000 + L * 100 + D + dl + int(has_hbar))
    N = idx[0].numel()
    assert N == tail_count(case)
    d = {k: v.to(dev).contiguous() for k, v in t.items()}
    layout = V().CellLayout.from_mask(mask.to(dev))
    assert layout.cells.shape[0] == N
    Wcat = torch.cat([d["Wfb"], d["Wfc"]], dim=1).contiguous()
    bcat = d["bfb"] + d["bfc"]
    nan = lambda *s: torch.full(s, float("nan"), device=dev)
    # the existing chain
    pm_old, psea_old = nan(B, L, L), nan(3, B, L)
    if N:
        hbar_old = d["hbar"]
        if not has_hbar:
            hbar_old = nan(N, D)
            call("smin_gate_fwd", stream(), ptr(d["fm"]), ptr(d["fs"]), ptr(layout.cells), N, D, ptr(hbar_old))
        cum, x1, mu = nan(N, D), nan(N, D), nan(N, D)
        call("smin_linear_rows_fwd", stream(), F._ptr_array([d["ccmean"]]), 1, ptr(d["Wc"]), ptr(d["bc"]), ptr(d["cumean"]), ptr(hbar_old), 1, N, D, dl, ptr(cum))
        call("smin_pair_product", stream(), ptr(d["bu"]), ptr(layout.cells), N, L, D, ptr(x1))
        call("smin_moment_unit_fwd", stream(), ptr(cum), ptr(d["fm"]), ptr(d["bu"]), ptr(layout.cells), N, B, L, D, ptr(Wcat), ptr(bcat), ptr(mu), ptr(x1))
    else:
        mu = torch.zeros(1, D, device=dev)
    call("smin_score_map_fwd", stream(), ptr(mu), ptr(d["bu"]), ptr(layout.cells), N, B, L, D, ptr(d["wm"]), ptr(d["bm"]), ptr(d["wb"]), ptr(d["bb"]),
         ptr(d["lmask"]), ptr(pm_old), ptr(psea_old))
    # the tail (its workspace NaN-filled first)
    V()._lib.workspace(V()._lib.load().smin_score_tail_ws_bytes(B, L, D, dl), dev).fill_(0xFF)              # (all ones: NaN as fp32)
    pm_new, psea_new = F.score_tail(d["ccmean"], d["cumean"], d["hbar"] if has_hbar else None, d["fm"], d["fs"], d["bu"], layout.cells, d["Wc"], d["bc"],
                                    Wcat, bcat, d["wm"], d["bm"], d["wb"], d["bb"], d["lmask"])
    torch.cuda.synchronize()
    assert torch.equal(psea_new, psea_old) and not torch.isnan(psea_new).any()
    assert pm_new[~mask.to(dev)].abs().max().item() == 0.0 if (~mask).any() else True
    assert not torch.isnan(pm_new).any()
    if N == 0:
        assert torch.equal(pm_new, torch.zeros_like(pm_new)) and torch.equal(pm_old, pm_new)
        return
    z64 = written_fp64(t, idx, has_hbar)
    inside, std = (z64.abs() <= 4).double().mean().item(), z64.std().item()
    assert inside >= 0.9 and std >= 0.3, (inside, std)                       # the inputs keep the gate sensitive
    p64 = torch.sigmoid(z64)
    e_old = (pm_old.cpu()[mask].double() - p64).abs().max().item()
    e_new = (pm_new.cpu()[mask].double() - p64).abs().max().item()
    print("tail", case[:5], "N", N, "err_old %.3e err_new %.3e gate %.3e" % (e_old, e_new, 2 * e_old + 2.4e-7), "logits inside %.2f std %.2f" % (inside, std))
    assert e_new <= 2 * e_old + 2.4e-7, (e_new, e_old)
    # the torch restatement of the collapse agrees with the kernel to fp32 rounding as well
    z32 = F.score_tail_torch(t["ccmean"], t["cumean"], t["hbar"], t["fm"], t["bu"], *idx, t["Wc"], t["bc"], t["Wfb"], t["Wfc"], t["bfb"] + t["bfc"], t["wm"], t["bm"])
    assert (torch.sigmoid(z32) - pm_new.cpu()[mask]).abs().max().item() < 2e-6
    again, _ = F.score_tail(d["ccmean"], d["cumean"], d["hbar"] if has_hbar else None, d["fm"], d["fs"], d["bu"], layout.cells, d["Wc"], d["bc"],
                            Wcat, bcat, d["wm"], d["bm"], d["wb"], d["bb"], d["lmask"], split=True)
    assert torch.equal(again, pm_new)                                       # issued as its two stages: the same bits


TAIL_SAT_CASES = [TAIL_CASES[k] for k in (0, 1, 4, 7, 8, 9)]      # the smallest case of each (NV, hbar given / re-formed) instance
TAIL_PRE = (20.0, 95.0, 110.0)
LEVELS = ("hard", "frozen")


def written(t, idx, has_hbar, dtype):
    """written_fp64 in ``dtype``"""
    c = {k: v.to(dtype) for k, v in t.items()}
    b_idx, i_idx, j_idx = idx
    hbar = c["hbar"] if has_hbar else torch.sigmoid(c["fm"] * c["fs"][b_idx]) * c["fm"]
    cum = c["ccmean"] @ c["Wc"].t() + c["bc"] + c["cumean"] + hbar
    x1 = c["bu"][b_idx, i_idx] * c["bu"][b_idx, j_idx]
    mu = x1 @ c["Wfb"].t() + cum @ c["Wfc"].t() + (c["bfb"] + c["bfc"]) + c["fm"]
    return mu @ c["wm"] + c["bm"]


def tail_saturated(case, level):
    """tail_inputs with bu moved along the three row heads' weights so that their logits take given values, and then cumean -- which
    enters the map head's logit linearly, through Wfc^T wm -- moved along that direction so that each cell's logit does: +-{20, 95, 110}
    (frozen), or that on half of the cells and rows and N(0, 2) on the rest (hard).  Returns (t, mask, idx, the map head's targets [N],
    the row heads' targets [3, B, L])."""
    B, L, D, dl, has_hbar, lens = case
    t, mask, idx = tail_inputs(case, seed=B * 1000 + L * 100 + D + dl + int(has_hbar))
    g = torch.Generator().manual_seed(D + dl + len(level))
    N = idx[0].numel()

    def targets(*s):
        v = torch.tensor(TAIL_PRE, dtype=torch.float64)[torch.randint(0, 3, s, generator=g)] * (torch.randint(0, 2, s, generator=g).double() * 2 - 1)
        return v if level == "frozen" else torch.where(torch.rand(*s, generator=g) < 0.5, v, 2 * torch.randn(*s, generator=g, dtype=torch.float64))
    target, rows = targets(N), targets(3, B, L)
    wb, bb = t["wb"].double(), t["bb"].double().reshape(3, 1, 1)
    for _ in range(2):
        miss = rows - bb - torch.einsum("bld,kd->kbl", t["bu"].double(), wb)
        t["bu"] = (t["bu"].double() + torch.einsum("kbl,kd->bld", torch.linalg.solve(wb @ wb.t(), miss.reshape(3, -1)).reshape(3, B, L), wb)).float()
    v = t["Wfc"].double().t() @ t["wm"].double()
    for _ in range(2):                                      # (the second pass takes up the rounding of the first to fp32)
        z = written(t, idx, has_hbar, torch.float64)
        t["cumean"] = (t["cumean"].double() + ((target - z) / (v @ v)).unsqueeze(1) * v).float()
    return t, mask, idx, target, rows


@pytest.mark.parametrize("level", LEVELS)
@pytest.mark.parametrize("case", TAIL_SAT_CASES, ids=lambda c: "B%d-L%d-D%d-dl%d-%s" % (c[0], c[1], c[2], c[3], "hbar" if c[4] else "gate"))
def test_tail_saturated_inputs_hold_what_they_claim(case, level):
    """The cases cover every (NV, hbar given / re-formed) instance; on the as-written formulas in fp64 the fp32 inputs' logits are the
    targets to 1e-3: a quarter beyond +-17 and a quarter inside +-4 (hard), all at +-{20, 95, 110} with every value under both signs
    over the cases (frozen); the scores at +20 and above round to 1.0f, those at -110 to 0.0f."""
    assert {(tail_form(c[2], c[3]), c[4]) for c in TAIL_SAT_CASES} == {(nv, hb) for nv in (0, 1, 2) for hb in (True, False)}
    t, mask, idx, target, rows = tail_saturated(case, level)
    z = written(t, idx, case[4], torch.float64)
    zb = torch.einsum("bld,kd->kbl", t["bu"].double(), t["wb"].double()) + t["bb"].double().reshape(3, 1, 1)
    assert (z - target).abs().max().item() <= 1e-3 and (zb - rows).abs().max().item() <= 1e-3
    if level == "hard":
        assert (zb.abs() > 17).double().mean().item() >= 0.25 and (zb.abs() < 4).double().mean().item() >= 0.25
    else:
        assert zb.abs().min().item() > 19.99 and bool((zb > 0).any() and (zb < 0).any())
    if level == "hard":
        assert (z.abs() > 17).double().mean().item() >= 0.25 and (z.abs() < 4).double().mean().item() >= 0.25
    else:
        assert z.abs().min().item() > 19.99 and bool((z > 0).any() and (z < 0).any()) and len(set(target.abs().tolist())) == 3
    p = torch.sigmoid(z)
    assert bool((p[z > 19.99].float() == 1.0).all()) and bool((p[z < -109.99].float() == 0.0).all())


@pytest.mark.gpu
@pytest.mark.parametrize("level", LEVELS)
@pytest.mark.parametrize("case", TAIL_SAT_CASES, ids=lambda c: "B%d-L%d-D%d-dl%d-%s" % (c[0], c[1], c[2], c[3], "hbar" if c[4] else "gate"))
def test_tail_kernel_saturated_against_fp64(dev, case, level):
    """smin_score_tail_fwd on tail_saturated: pm and psea exactly 1.0 from a logit of +20 on and exactly 0.0 from -110 on, +0.0 outside
    the list and beyond the length, finite everywhere, and the project's gate against the as-written formulas in fp64, e_torch32 from
    the same formulas in fp32.
    Measured on an MI355X: INTEGRATION.md, "Saturated inputs"."""
    from tests.support.compare import gate
    F = V().functional
    B, L, D, dl, has_hbar, lens = case
    t, mask, idx, target, rows = tail_saturated(case, level)
    d = {k: v.to(dev).contiguous() for k, v in t.items()}
    layout = V().CellLayout.from_mask(mask.to(dev))
    Wcat = torch.cat([d["Wfb"], d["Wfc"]], dim=1).contiguous()
    pm, psea = F.score_tail(d["ccmean"], d["cumean"], d["hbar"] if has_hbar else None, d["fm"], d["fs"], d["bu"], layout.cells, d["Wc"], d["bc"],
                            Wcat, d["bfb"] + d["bfc"], d["wm"], d["bm"], d["wb"], d["bb"], d["lmask"])
    torch.cuda.synchronize()
    pm = pm.cpu()
    assert bool(torch.isfinite(pm).all()) and bool(torch.isfinite(psea).all())
    assert bool((pm[~mask].view(torch.int32) == 0).all())
    got = pm[mask]
    assert bool((got[target > 19.99] == 1.0).all()) and bool((got[target < -109.99] == 0.0).all())
    tag = "score_tail B%d-L%d-D%d-dl%d-%s %s" % (B, L, D, dl, "hbar" if has_hbar else "gate", level)
    gate(tag + " pm", got, torch.sigmoid(written(t, idx, has_hbar, torch.float64)), torch.sigmoid(written(t, idx, has_hbar, torch.float32)))
    heads = lambda dt: torch.sigmoid(torch.einsum("bld,kd->kbl", t["bu"].to(dt), t["wb"].to(dt)) + t["bb"].to(dt).reshape(3, 1, 1)) * t["lmask"].to(dt)
    psea = psea.cpu()
    on = (t["lmask"] != 0).expand(3, B, L)
    assert bool((psea[~on].view(torch.int32) == 0).all())
    assert bool((psea[on & (rows > 19.99)] == 1.0).all()) and bool((psea[on & (rows < -109.99)] == 0.0).all())
    gate(tag + " psea", psea, heads(torch.float64), heads(torch.float32))


@pytest.mark.gpu
def test_tail_refusals(dev):
    """D % 4, dl % 4, null pointers (beyond the two whole stages that may be skipped), a short or misaligned workspace: a negative
    code, nothing launched (the outputs stay NaN)."""
    ptr, stream = V()._lib.ptr, V()._lib.stream
    lib = V()._lib.load()
    case = (2, 8, 64, 16, True, None)
    t, mask, idx = tail_inputs(case, seed=3)
    d = {k: v.to(dev).contiguous() for k, v in t.items()}
    layout = V().CellLayout.from_mask(mask.to(dev))
    N, B, L, D, dl = idx[0].numel(), 2, 8, 64, 16
    Wcat, bcat = torch.cat([d["Wfb"], d["Wfc"]], dim=1).contiguous(), d["bfb"] + d["bfc"]
    pm, psea = torch.full((B, L, L), float("nan"), device=dev), torch.full((3, B, L), float("nan"), device=dev)
    nbytes = lib.smin_score_tail_ws_bytes(B, L, D, dl)
    ws = torch.empty(nbytes + 64, dtype=torch.uint8, device=dev)
    assert ws.data_ptr() % 16 == 0

    def run(D=D, dl=dl, ws_ptr=None, ws_n=nbytes, **null):
        a = dict(ccmean=d["ccmean"], cumean=d["cumean"], hbar=d["hbar"], fm=d["fm"], fs=d["fs"], bu=d["bu"], cells=layout.cells, Wc=d["Wc"], bc=d["bc"], Wcat=Wcat,
                 bcat=bcat, wm=d["wm"], bm=d["bm"], wb=d["wb"], bb=d["bb"], lmask=d["lmask"], pm=pm, psea=psea)
        a.update(null)
        p = {k: ptr(v) for k, v in a.items()}
        return lib.smin_score_tail_fwd(stream(), p["ccmean"], p["cumean"], p["hbar"], p["fm"], p["fs"], p["bu"], p["cells"], N, B, L, D, dl, p["Wc"], p["bc"], p["Wcat"],
                                       p["bcat"], p["wm"], p["bm"], p["wb"], p["bb"], p["lmask"], p["pm"], p["psea"], ptr(ws) if ws_ptr is None else ws_ptr, ws_n)

    assert run(D=62) < 0 and run(dl=18) < 0 and run(ws_n=nbytes - 4) < 0 and run(ws_n=0) < 0
    import ctypes
    assert run(ws_ptr=ctypes.c_void_p(ws.data_ptr() + 4)) < 0 and run(ws_ptr=ctypes.c_void_p(0)) < 0
    for name in ("ccmean", "cumean", "fm", "bu", "cells", "Wc", "bc", "Wcat", "bcat", "wm", "bm", "wb", "bb", "lmask", "pm", "psea"):
        assert run(**{name: None}) < 0, name
    assert run(hbar=None, fs=None) < 0
    assert run(Wc=None, bc=None, Wcat=None, bcat=None, pm=None, psea=None) < 0          # neither stage
    torch.cuda.synchronize()
    assert torch.isnan(pm).all() and torch.isnan(psea).all()
    assert run(pm=None, psea=None) == 0                                     # the vectors alone: no score is written
    torch.cuda.synchronize()
    assert torch.isnan(pm).all() and torch.isnan(psea).all()
    assert run(Wc=None, bc=None, Wcat=None, bcat=None, bm=None) == 0 and run() == 0 and run(hbar=None) == 0
    torch.cuda.synchronize()
    assert not torch.isnan(pm).any() and not torch.isnan(psea).any()


# ---------------------------------------------------------------- GPU: the model
def formula_model(shape, dev, gain=1.2):
    from oracle import smin_oracle as O
    T, L, C, D, dl, layers, Din, Nq, Hh = shape
    sd = O.formula_state_dict(H.smin_shapes(*shape), gain=gain)
    return build_model(dict(T=T, L=L, C=C, D=D, dl=dl, layers=layers, Din=Din, Nq=Nq, H=Hh), sd, dev), sd


def check_outputs(out, xs):
    pm, ps, pe, pa = out
    B, L = xs[4].shape
    assert pm.shape == (B, L, L) and ps.shape == pe.shape == pa.shape == (B, L)
    for t in out:
        assert t.dtype == torch.float32 and t.is_contiguous() and not t.requires_grad and t.grad_fn is None


@pytest.mark.gpu
@pytest.mark.parametrize("name", H.TINY)
def test_score_against_golden_tiny(dev, name):
    cfg, sd, batch, out, _, _ = H.split_tiny(H.load_npz(name))
    m = build_model(cfg, sd, dev)
    b = {k: v.to(dev) for k, v in batch.items()}
    xs = H.model_inputs(b)
    got = m.score(*xs)
    check_outputs(got, xs)
    for k, v in zip(("pm", "ps", "pe", "pa"), got):
        err = (v.cpu() - out[k]).abs().max().item()
        print(name, m._plan(xs[0], xs[2]), k, "max abs err", err)
        assert err < SCORE_TOL, (k, err)
    assert got[0][~b["moment_mask"]].abs().max().item() == 0.0


def full_size_errors(dev, name):
    from oracle import smin_oracle as O
    z = H.load_npz("g5_" + name)
    shape = H.FULL[name]
    B, seed = int(z["cfg"][-2]), int(z["cfg"][-1])
    m, _ = formula_model(shape, dev, gain=1.3)
    b = {k: v.to(dev) for k, v in O.synthetic_batch(B, shape[0], shape[1], shape[7], shape[6], seed=seed).items()}
    xs = H.model_inputs(b)
    assert m._plan(xs[0], xs[2]) == "node"
    got = m.score(*xs)
    check_outputs(got, xs)
    assert got[0][~b["moment_mask"]].abs().max().item() == 0.0
    errs = {k: (v.cpu() - torch.from_numpy(z["out/" + k])).abs().max().item() for k, v in zip(("pm", "ps", "pe", "pa"), got)}
    print("score", V().get_gemm_mode(), name, errs)
    return errs


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["tacos_yml", "tacos_d500", "charades", "anet_yml", "anet_t256"])
def test_score_full_size_against_golden(dev, name):
    for k, err in full_size_errors(dev, name).items():
        assert err < 1e-4, (k, err)


@pytest.fixture()
def f32e():
    V().set_gemm_mode("f32e")
    yield
    V().set_gemm_mode(V()._lib.DEFAULT_GEMM_MODE)


@pytest.fixture()
def bf16_mode():
    V().set_gemm_mode("bf16")
    yield
    V().set_gemm_mode(V()._lib.DEFAULT_GEMM_MODE)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["tacos_yml", "tacos_d500", "charades", "anet_yml", "anet_t256"])
def test_score_full_size_against_golden_f32e(dev, f32e, name):
    for k, err in full_size_errors(dev, name).items():
        assert err < 5e-6, (k, err)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["tacos_yml", "tacos_d500", "charades", "anet_yml", "anet_t256"])
def test_score_full_size_against_golden_bf16(dev, bf16_mode, name):
    for k, err in full_size_errors(dev, name).items():
        assert err < 2e-2, (k, err)


ORACLE_ROWS = [
    (64, 16, 4, 128, 64, 2, 40, 9, 64, 3),
    (32, 16, 4, 64, 32, 1, 24, 17, 32, 5),       # one layer: the clip mean entering the tail is the proposal map's f_m
    (32, 8, 4, 64, 16, 2, 24, 32, 32, 2),
    (64, 16, 4, 256, 128, 2, 40, 23, 128, 3),
    (32, 8, 4, 192, 128, 2, 24, 29, 96, 4),
    (64, 16, 4, 104, 48, 2, 24, 18, 52, 3),
    (48, 24, 4, 128, 64, 1, 32, 20, 64, 3),      # one layer, r = 2 < C
    (96, 32, 3, 128, 64, 3, 24, 32, 64, 1),      # B = 1, C = 3, Nq = 32
]


def test_oracle_rows_cover_the_native_rows():
    import models
    assert callable(models.SMIN.score)
    assert set(NATIVE_ROWS) <= set(ORACLE_ROWS)
    assert any(r[5] == 1 for r in ORACLE_ROWS) and any(r[9] == 1 for r in ORACLE_ROWS)


@pytest.mark.gpu
@pytest.mark.parametrize("T,L,C,D,dl,layers,Din,Nq,Hh,B", ORACLE_ROWS)
def test_score_against_oracle(dev, T, L, C, D, dl, layers, Din, Nq, Hh, B):
    from oracle import smin_oracle as O
    m, sd = formula_model((T, L, C, D, dl, layers, Din, Nq, Hh), dev)
    batch = O.synthetic_batch(B, T, L, Nq, Din, seed=T + L + D)
    with torch.no_grad():
        ref = O.smin_forward(sd, dict(T=T, L=L, C=C), *H.model_inputs(batch))
    b = {k: v.to(dev) for k, v in batch.items()}
    xs = H.model_inputs(b)
    assert m._plan(xs[0], xs[2]) == "node"
    got = m.score(*xs)
    check_outputs(got, xs)
    for k, v, r in zip(("pm", "ps", "pe", "pa"), got, ref):
        err = (v.cpu() - r).abs().max().item()
        print((T, L, C, D, dl, layers, B), k, "max abs err", err)
        assert err < SCORE_TOL, (k, err)
    assert got[0][~b["moment_mask"]].abs().max().item() == 0.0


SMALL = (32, 16, 4, 64, 32, 2, 48, 7, 32)             # T, L, C, D, dl, layers, Din, Nq, H


def same_dict(a, b):
    assert a.keys() == b.keys()
    for k in a:
        x, y = a[k], b[k]
        assert x.dtype == y.dtype and x.shape == y.shape, k
        assert torch.equal(torch.nan_to_num(x.float(), nan=-7.0), torch.nan_to_num(y.float(), nan=-7.0)) if x.is_floating_point() else torch.equal(x, y), k


def window_inputs(dev, seed=4):
    T = SMALL[0]
    lengths = [5, T, T + 1, 3 * T + 7]
    g = torch.Generator().manual_seed(seed)
    raw = torch.randn(sum(lengths), SMALL[6], generator=g).to(dev)
    qf = torch.randn(4, SMALL[7], 300, generator=g).to(dev)
    qm = (torch.arange(SMALL[7]).unsqueeze(0) < torch.tensor([7, 3, 5, 6]).unsqueeze(1)).to(torch.uint8).to(dev)
    return raw, lengths, qf, qm


@pytest.mark.gpu
def test_nothing_else_moved(dev):
    """forward_only_scoring off: localize and localize_windows return the same bits before and after a score call, and the forward
    under no_grad too."""
    from oracle import smin_oracle as O
    m, _ = formula_model(SMALL, dev)
    assert m.forward_only_scoring is False
    b = {k: v.to(dev) for k, v in O.synthetic_batch(4, SMALL[0], SMALL[1], SMALL[7], SMALL[6], seed=11).items()}
    xs = H.model_inputs(b)
    raw, lengths, qf, qm = window_inputs(dev)
    with torch.no_grad():
        f0 = [t.clone() for t in m(*xs)]
    r0 = m.localize(*xs, k=5)
    w0 = m.localize_windows(raw, lengths, qf, qm, k=5, max_batch=3)
    s = m.score(*xs)
    r1 = m.localize(*xs, k=5)
    w1 = m.localize_windows(raw, lengths, qf, qm, k=5, max_batch=3)
    with torch.no_grad():
        f1 = m(*xs)
    same_dict(r0, r1)
    same_dict(w0, w1)
    for a, c in zip(f0, f1):
        assert torch.equal(a, c)
    for a, c in zip(f0[1:], s[1:]):
        assert torch.equal(a, c)                                            # the boundary heads: the same launch on the same bu
    assert (f0[0] - s[0]).abs().max().item() < 2e-6
    assert layout_ok(dev)


def ranking_is_separated(pm, ps, pe, mask, k, thr, gap):
    """Whether greedy NMS over these scores visits candidates whose consecutive scores differ by more than ``gap`` (so that any
    perturbation of the scores below gap / 2 visits them in the same order and keeps the same cells)."""
    L = pm.shape[1]
    r = V().top_moments_torch(pm, ps, pe, mask, k=k, nms_thresh=thr)
    score = (pm * ps.sqrt().unsqueeze(2) * pe.sqrt().unsqueeze(1)).reshape(pm.shape[0], -1)
    for b in range(pm.shape[0]):
        s, order = torch.sort(score[b][mask[b].reshape(-1)], descending=True)
        n = int(r["count"][b])
        if n == 0:
            continue
        last = float(r["score"][b, n - 1])
        visited = int((s >= last).sum()) if n == k else s.numel()            # fewer than k kept: every candidate was visited
        head = s[:min(visited + 1, s.numel())]
        if head.numel() > 1 and (head[:-1] - head[1:]).min().item() <= gap:
            return False
    return True


RANK_SEED = 11


@pytest.mark.gpu
def test_switch_on_ranks_the_same_moments(dev):
    """forward_only_scoring on: localize keeps the same cells on a batch whose visited candidates are separated by more than 1e-4 in
    score (asserted on the CPU oracle's scores); localize_windows hands the plan's cell counts on and the layout word stays 0."""
    from oracle import smin_oracle as O
    m, sd = formula_model(SMALL, dev)
    batch = O.synthetic_batch(4, SMALL[0], SMALL[1], SMALL[7], SMALL[6], seed=RANK_SEED)
    with torch.no_grad():
        pm, ps, pe, _ = O.smin_forward(sd, dict(T=SMALL[0], L=SMALL[1], C=SMALL[2]), *H.model_inputs(batch))
    assert ranking_is_separated(pm, ps, pe, batch["moment_mask"], 3, 0.5, 1e-4)
    xs = H.model_inputs({k: v.to(dev) for k, v in batch.items()})
    off = m.localize(*xs, k=3)
    m.forward_only_scoring = True
    on = m.localize(*xs, k=3)
    assert torch.equal(on["idx"], off["idx"]) and torch.equal(on["count"], off["count"])
    assert (on["score"] - off["score"]).abs().max().item() < 2e-6
    raw, lengths, qf, qm = window_inputs(dev)
    w_on = m.localize_windows(raw, lengths, qf, qm, k=5, max_batch=3)
    torch.cuda.synchronize()
    assert layout_ok(dev)
    assert m.known_cell_count is None
    m.forward_only_scoring = False
    w_off = m.localize_windows(raw, lengths, qf, qm, k=5, max_batch=3)
    assert torch.equal(w_on["n_windows"], w_off["n_windows"]) and torch.equal(w_on["count"], w_off["count"])
    assert (torch.nan_to_num(w_on["score"]) - torch.nan_to_num(w_off["score"])).abs().max().item() < 2e-6
    # attention=True keeps the existing path whatever the switch says
    m.forward_only_scoring = True
    a_on = m.localize(*xs, k=3, attention=True)
    m.forward_only_scoring = False
    same_dict(a_on, m.localize(*xs, k=3, attention=True))


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["units", "python_host", "keep_attention"])
def test_fallbacks_score_as_forward(dev, kind):
    from oracle import smin_oracle as O
    shape = (32, 8, 4, 64, 16, 9, 24, 6, 32) if kind == "units" else SMALL
    m, _ = formula_model(shape, dev)
    if kind == "python_host":
        m.fused_core = False
    if kind == "keep_attention":
        m.keep_attention = True
    b = {k: v.to(dev) for k, v in O.synthetic_batch(2, shape[0], shape[1], shape[7], shape[6], seed=3).items()}
    xs = H.model_inputs(b)
    assert m._plan(xs[0], xs[2]) == {"units": "units", "python_host": "stream", "keep_attention": "node"}[kind]
    with torch.no_grad():
        want = [t.clone() for t in m(*xs)]
    got = m.score(*xs)
    check_outputs(got, xs)
    for a, c in zip(got, want):
        assert torch.equal(a, c)


@pytest.mark.gpu
def test_score_is_repeatable(dev):
    from oracle import smin_oracle as O
    shape = (64, 16, 4, 256, 128, 3, 40, 23, 128)
    m, _ = formula_model(shape, dev)
    b = {k: v.to(dev) for k, v in O.synthetic_batch(6, shape[0], shape[1], shape[7], shape[6], seed=2).items()}
    xs = H.model_inputs(b)
    first = [t.clone() for t in m.score(*xs)]
    for _ in range(9):
        for a, c in zip(first, m.score(*xs)):
            assert torch.equal(a, c)
    # a caller that knows the cell count: no host wait, the same bits, the layout word stays 0
    m.known_cell_count = int(b["moment_mask"].sum())
    for a, c in zip(first, m.score(*xs)):
        assert torch.equal(a, c)
    torch.cuda.synchronize()
    assert layout_ok(dev)


@pytest.mark.gpu
def test_score_allocates_less(dev):
    """anet_yml, B = 2: the peak of allocated memory over one score call is below that of one forward under no_grad by at least
    2 N D 4 bytes -- the last layer's x1, cum and mu (3 N x D) are never allocated, the tail's workspace is a few vectors; one N x D of
    slack for the allocator's rounding."""
    from oracle import smin_oracle as O
    shape = H.FULL["anet_yml"]
    m, _ = formula_model(shape, dev, gain=1.3)
    b = {k: v.to(dev) for k, v in O.synthetic_batch(2, shape[0], shape[1], shape[7], shape[6], seed=1).items()}
    xs = H.model_inputs(b)
    N, D = int(b["moment_mask"].sum()), shape[3]
    peaks = {}
    for name, fn in (("forward", lambda: m(*xs)), ("score", lambda: m.score(*xs))):
        with torch.no_grad():
            fn()                                                            # scratch, tables and streams exist from here on
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats(dev)
            out = fn()
            torch.cuda.synchronize()
            peaks[name] = torch.cuda.max_memory_allocated(dev)
            del out
    print("peak bytes over one call", peaks, "N", N, "2 N D 4 =", 2 * N * D * 4)
    assert peaks["forward"] - peaks["score"] >= 2 * N * D * 4, peaks
