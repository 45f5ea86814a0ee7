"""The 2D proposal map and the kernels built on it -- csrc/proposal_map.hip (ProposalGeneration, the content stream's clip-window
means, the clip-event table), csrc/boundary_unit.hip (the L x L boundary self-attention with its word attention and the map-sized row
reduction), csrc/moment_unit.hip and csrc/score_map.hip -- against float64 restatements of the reference's formulas.

CPU: each restatement is pinned to the oracle (oracle/smin_oracle.py) at 1e-12, and Python mirrors of the launch arithmetic show that
the GPU case lists together reach every instantiation and code path the C ABI can pick (test_map_cases_reach_every_form).
GPU: every case writes into NaN-prefilled outputs (and workspace), compares every output and gradient with float64, and runs its
backward twice, bit for bit."""
import ctypes
import math

import numpy as np
import pytest
import torch

from tests import helpers as H
from tests.support.device import dev  # noqa: F401  (the module's device fixture)
from tests.support.compare import _assert_spread, _spread
from tests.support.guards import _vp
from tests.support.references import _layout_to, lengths_mask, make_layout, moment_mask

FWD_TOL = 1e-5          # max |got - ref| / max |ref|, per output and case
GRAD_TOL = 1e-4
PIN_TOL = 1e-12


def cdiv(a, b):
    return (a + b - 1) // b


# ---------------------------------------------------------------- float64 restatements (packed cells: no dense L x L x C x T)

def clip_windows(cells, T, L, C):
    """Per cell of cells [N, 4] (b, i, j, m): first frame of every clip [N, C], clip size [N], which clips exist [N, C] (masked
    cells and cells with j < i have none), and 1/cs as the reference stores it (compute_content_matrix: a float32 reciprocal)."""
    r = T // L
    c = cells.long()
    i, j, m = c[:, 1], c[:, 2], c[:, 3]
    w = j - i + 1
    nf = w * r
    cs = torch.clamp(torch.div(nf, C, rounding_mode="floor"), min=1)
    nclip = torch.where((m != 0) & (w >= 1), torch.clamp(nf, max=C), torch.zeros_like(nf))
    k = torch.arange(C).view(1, C)
    live = k < nclip.view(-1, 1)
    start = torch.where(live, (i * r).view(-1, 1) + k * cs.view(-1, 1), torch.zeros(1, dtype=torch.long))
    inv = (1.0 / cs.to(torch.float32)).double()
    return start, cs, live, inv


def proposal_map_ref(f, cells, T, L, C):
    """ProposalGeneration (reference models.py:115-126) on packed cells from float64 prefix sums over time:
    fc [N, C, D] clip means (0 for absent clips and masked cells), fm [N, D] = mean over the C clips, fb [B, L, D] = AvgPool1d(r, r)."""
    B, _, D = f.shape
    P = torch.cat([f.new_zeros(B, 1, D), f.cumsum(1)], 1)
    start, cs, live, inv = clip_windows(cells, T, L, C)
    b = cells[:, 0].long().view(-1, 1)
    end = torch.where(live, start + cs.view(-1, 1), start)
    fc = (P[b, end] - P[b, start]) * (inv.view(-1, 1, 1) * live.unsqueeze(-1).to(f.dtype))
    r = T // L
    return fc, fc.mean(1), f.reshape(B, L, r, D).mean(2)


def clip_window_means_ref(g, bias, cells, T, L, C, nseg):
    """smin_clip_window_means_fwd: out[s][n*C + c] = m (clip mean of g's segment s + bias[segment s]); bias covers its first
    bias.numel() features (whole segments), empty clips of a present cell get the bias alone."""
    D = g.shape[2]
    W = D // nseg
    fc, _, _ = proposal_map_ref(g, cells, T, L, C)
    full = torch.cat([bias, g.new_zeros(D - bias.numel())]) if bias is not None else g.new_zeros(D)
    out = fc + cells[:, 3].to(g.dtype).view(-1, 1, 1) * full
    return [out[..., s * W:(s + 1) * W].reshape(-1, W) for s in range(nseg)]


def boundary_unit_ref(fb, fw, fs, hbar, cells, Wq, bq, Wk, bk, qmask, lmask):
    """BoundaryUnit (reference models.py:137-196) with f_bm summed over the listed cells only:
    returns out [B, L, D], the word weights P [B, L, Nq], the self-attention A [B, L, L], both logit tensors (masked) and Kb."""
    B, L, D = fb.shape
    Qb, Kb = fb @ Wq.t() + bq, fw @ Wk.t() + bk
    qm = qmask.unsqueeze(1)
    S = ((Qb @ Kb.transpose(1, 2)) / math.sqrt(D) * qm).masked_fill(qm == 0, -1e9)
    P = torch.softmax(S, -1)
    lcol, lrow = lmask.unsqueeze(-1), lmask.unsqueeze(1)
    baq = (P @ fw) * lcol
    bqv = fb * (baq + fs.unsqueeze(1))
    Z = ((bqv @ bqv.transpose(1, 2)) / math.sqrt(D) * lrow).masked_fill(lrow == 0, -1e9)
    A = torch.softmax(Z, -1) * lcol
    out = (A @ fb) * lcol + fb
    c = cells.long()
    a = A[c[:, 0], c[:, 1], c[:, 2]]
    out = out.reshape(B * L, D).index_add(0, c[:, 0] * L + c[:, 1], a.unsqueeze(-1) * hbar).reshape(B, L, D)
    return out, P, A, S, Z, Kb


def moment_unit_ref(fcmean, fm, fb, cells, Wcat, bcat, pair_used=None):
    """MomentUnit (reference models.py:288-303): mu = m ([fb_i * fb_j | fcmean] Wcat^T + bcat) + fm.  pair_used: the pair product the
    contraction reads instead (the bf16-stored operand); its gradient still flows to fb exactly, as moment_dfb_kernel forms it."""
    c = cells.long()
    pair = fb[c[:, 0], c[:, 1]] * fb[c[:, 0], c[:, 2]]
    if pair_used is not None:
        pair = pair + (pair_used - pair).detach()
    X = torch.cat([pair, fcmean], 1)
    return c[:, 3].to(fm.dtype).view(-1, 1) * (X @ Wcat.t() + bcat) + fm


def score_heads_ref(fm, fb, cells, wm, bm, wb, bb, lmask):
    """Localization (reference models.py:335-344): pm [B, L, L] (0 where no cell is listed), psea [3, B, L]."""
    B, L, _ = fb.shape
    c = cells.long()
    s = torch.sigmoid(fm @ wm + bm) * c[:, 3].to(fm.dtype)
    pm = fm.new_zeros(B * L * L).index_add(0, (c[:, 0] * L + c[:, 1]) * L + c[:, 2], s).reshape(B, L, L)
    psea = torch.sigmoid(torch.einsum("bld,kd->kbl", fb, wb) + bb.view(3, 1, 1)) * lmask
    return pm, psea


# ---------------------------------------------------------------- inputs
def default_lens(B, L):
    """Full length for even samples, ragged for odd ones (the synthetic batch's pattern)."""
    return [L if b % 2 == 0 else max(1, L - 1 - (b * 7) % max(1, L // 2)) for b in range(B)]


# ---------------------------------------------------------------- CPU: the restatements against the oracle

PIN_GEOMETRIES = [(8, 8, 4), (16, 8, 3), (24, 6, 4), (20, 5, 3), (12, 12, 5), (18, 9, 9)]


def test_pin_geometries_cover_the_windows():
    """r = T/L in {1, 2, 4}; some windows hold fewer frames than clips, some a frame count that is not a multiple of C."""
    rs, short, dropped = set(), False, False
    for T, L, C in PIN_GEOMETRIES:
        nf = np.arange(1, L + 1) * (T // L)
        rs.add(T // L)
        short |= bool((nf < C).any())
        dropped |= bool(((nf > C) & (nf % C != 0)).any())
    assert {1, 2, 4} <= rs and short and dropped


@pytest.mark.parametrize("T,L,C", PIN_GEOMETRIES)
@pytest.mark.parametrize("layout", ["from_mask", "all_cells"])
def test_proposal_map_ref_matches_oracle(T, L, C, layout):
    """r = T/L in {1, 2, 4}; windows of fewer frames than clips (empty clips) and of a frame count that is not a multiple of C
    (dropped frames); masked and lower-triangular cells in the all_cells layout.  Values and gradients."""
    import models
    from oracle import smin_oracle as O
    B, D = 2, 6
    g = torch.Generator().manual_seed(T * 31 + L + C)
    mm = moment_mask(B, L, "ragged", [L, L - 2], g)
    lay = make_layout(mm, layout)
    f = torch.randn(B, T, D, generator=g, dtype=torch.float64).requires_grad_(True)
    fc, fm, fb = proposal_map_ref(f, lay.cells, T, L, C)
    f2 = f.detach().clone().requires_grad_(True)
    ofc, ofm, ofb = O.proposal_generation(f2, mm.double(), T, L, C)
    for got, want in ((fc, lay.pack(ofc)), (fm, lay.pack(ofm)), (fb, ofb)):
        torch.testing.assert_close(got, want, rtol=PIN_TOL, atol=PIN_TOL)
    # the windows are compute_content_matrix's (the product's restatement, pinned to the reference by test_compute_content_matrix_matches_golden)
    Wc = models.compute_content_matrix(T, L, C).double()
    dense = torch.einsum("ijct,btd->bijcd", Wc, f.detach()) * mm.double()[..., None, None]
    torch.testing.assert_close(fc.detach(), lay.pack(dense), rtol=PIN_TOL, atol=PIN_TOL)
    G = [torch.randn(x.shape, generator=g, dtype=torch.float64) for x in (fc, fm, fb)]
    (sum((x * y).sum() for x, y in zip((fc, fm, fb), G))).backward()
    oG = [lay.unpack(G[0]), lay.unpack(G[1]), G[2]]
    (sum((x * y).sum() for x, y in zip((ofc, ofm, ofb), oG))).backward()
    torch.testing.assert_close(f.grad, f2.grad, rtol=PIN_TOL, atol=PIN_TOL)


def test_clip_window_means_ref_matches_oracle():
    """Three segments, the bias covering the first one only; masked cells of the all_cells layout give 0 rows."""
    from oracle import smin_oracle as O
    B, T, L, C, W, nseg = 2, 16, 8, 3, 4, 3
    g = torch.Generator().manual_seed(8)
    mm = moment_mask(B, L, "ragged", [8, 6], g)
    lay = make_layout(mm, "all_cells")
    gf = torch.randn(B, T, W * nseg, generator=g, dtype=torch.float64)
    bias = torch.randn(W, generator=g, dtype=torch.float64)
    outs = clip_window_means_ref(gf, bias, lay.cells, T, L, C, nseg)
    ofc, _, _ = O.proposal_generation(gf, mm.double(), T, L, C)
    want = lay.pack(ofc + torch.cat([bias, bias.new_zeros(W * (nseg - 1))]) * mm.double()[..., None, None])
    for s in range(nseg):
        torch.testing.assert_close(outs[s], want[..., s * W:(s + 1) * W].reshape(-1, W), rtol=PIN_TOL, atol=PIN_TOL)


def _bu_params(D, g, scale=1.0):
    std = scale / math.sqrt(D)
    return {n: torch.randn(s, generator=g, dtype=torch.float64) * (std if len(s) == 2 else 0.3)
            for n, s in (("W_q.weight", (D, D)), ("W_q.bias", (D,)), ("W_k.weight", (D, D)), ("W_k.bias", (D,)))}


@pytest.mark.parametrize("layout", ["from_mask", "all_cells"])
def test_boundary_unit_ref_matches_oracle(layout):
    """Fractional query masks, a query with every word masked, rows with lm = 0 and a sample of length 0; values and gradients."""
    from oracle import smin_oracle as O
    B, L, D, Nq = 4, 6, 8, 5
    g = torch.Generator().manual_seed(11)
    lens = [6, 4, 0, 5]
    lm = lengths_mask(B, L, lens).double()
    mm = moment_mask(B, L, "ragged", lens, g)
    lay = make_layout(mm, layout)
    qmask = torch.tensor([[1, 1, 0.5, 1, 0], [1, 0.25, 1, 0, 0], [1, 1, 1, 1, 1], [0, 0, 0, 0, 0]], dtype=torch.float64)
    p = _bu_params(D, g)
    sd = {"bu.attn_layer." + k: v for k, v in p.items()}
    fb = torch.randn(B, L, D, generator=g, dtype=torch.float64).requires_grad_(True)
    fw = torch.randn(B, Nq, D, generator=g, dtype=torch.float64).requires_grad_(True)
    fs = torch.randn(B, D, generator=g, dtype=torch.float64).requires_grad_(True)
    fm = (torch.randn(B, L, L, D, generator=g, dtype=torch.float64) * (mm.double().unsqueeze(-1) if layout == "from_mask" else 1)).requires_grad_(True)
    want = O.boundary_unit(sd, "bu.", fb, fw, fs, fm, qmask, lm)
    hbar = lay.pack(torch.sigmoid(fm * fs[:, None, None, :]) * fm)
    got = boundary_unit_ref(fb, fw, fs, hbar, lay.cells, p["W_q.weight"], p["W_q.bias"], p["W_k.weight"], p["W_k.bias"], qmask, lm)[0]
    torch.testing.assert_close(got, want, rtol=PIN_TOL, atol=PIN_TOL)
    G = torch.randn(B, L, D, generator=g, dtype=torch.float64)
    ga = list(torch.autograd.grad((got * G).sum(), (fb, fw, fs, fm)))
    gb = list(torch.autograd.grad((want * G).sum(), (fb, fw, fs, fm)))
    ga[3], gb[3] = lay.pack(ga[3]), lay.pack(gb[3])            # f_m enters through the listed cells' hbar only
    for a, b in zip(ga, gb):
        torch.testing.assert_close(a, b, rtol=PIN_TOL, atol=PIN_TOL)


@pytest.mark.parametrize("layout", ["from_mask", "all_cells"])
def test_moment_and_score_refs_match_oracle(layout):
    """moment_unit_ref and score_heads_ref against oracle.moment_unit / oracle.localization (masked cells: mu = fm, pm = 0)."""
    from oracle import smin_oracle as O
    B, L, C, D = 3, 5, 4, 8
    g = torch.Generator().manual_seed(12)
    lens = [5, 3, 4]
    lm = lengths_mask(B, L, lens).double()
    mm = moment_mask(B, L, "ragged", lens, g)
    lay = make_layout(mm, layout)
    r = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    sd = {"mu.conv_layer_fb.weight": r(D, D, 1, 1), "mu.conv_layer_fb.bias": r(D), "mu.conv_layer_fc.weight": r(D, D, 1, 1),
          "mu.conv_layer_fc.bias": r(D), "lo.conv_layer_pm.weight": r(1, D, 1, 1), "lo.conv_layer_pm.bias": r(1)}
    for n in ("ps", "pe", "pa"):
        sd[f"lo.conv_layer_{n}.weight"], sd[f"lo.conv_layer_{n}.bias"] = r(1, D, 1), r(1)
    f_c, f_m, f_b = r(B, L, L, C, D) * mm.double()[..., None, None], r(B, L, L, D), r(B, L, D)
    want = O.moment_unit(sd, "mu.", f_c, f_m, f_b, mm)
    Wcat = torch.cat([sd["mu.conv_layer_fb.weight"].reshape(D, D), sd["mu.conv_layer_fc.weight"].reshape(D, D)], 1)
    got = moment_unit_ref(lay.pack(f_c.mean(3)), lay.pack(f_m), f_b, lay.cells, Wcat, sd["mu.conv_layer_fb.bias"] + sd["mu.conv_layer_fc.bias"])
    torch.testing.assert_close(got, lay.pack(want), rtol=PIN_TOL, atol=PIN_TOL)
    opm, ops, ope, opa = O.localization(sd, f_m * mm.double().unsqueeze(-1), f_b, lm, mm, p="lo.")
    wb = torch.stack([sd[f"lo.conv_layer_{n}.weight"].reshape(D) for n in ("ps", "pe", "pa")])
    bb = torch.cat([sd[f"lo.conv_layer_{n}.bias"] for n in ("ps", "pe", "pa")])
    pm, psea = score_heads_ref(lay.pack(f_m * mm.double().unsqueeze(-1)), f_b, lay.cells, sd["lo.conv_layer_pm.weight"].reshape(D),
                               sd["lo.conv_layer_pm.bias"], wb, bb, lm)
    torch.testing.assert_close(pm, opm, rtol=PIN_TOL, atol=PIN_TOL)
    torch.testing.assert_close(psea, torch.stack([ops, ope, opa]), rtol=PIN_TOL, atol=PIN_TOL)


# ---------------------------------------------------------------- mirrors of the launch arithmetic

GEMM_SLOTS = H.GEMM_SLOTS
EV_ROUND = 2 * 512                # proposal_map_bwd_events2_kernel: 2 waves x EV_CAP table entries per round


def time_scan_small(T):
    """time_scan_kernel: a segment of ceil(T / 16) frames is held in registers when it is at most 16 long."""
    return cdiv(T, 16) <= 16


def events2_form(D, W, has_m):
    """launch_events2: (lanes, nslot, NS, UNR, HAS_M) of the proposal_map_bwd_events2_kernel instance (W = D for a dense gradient)."""
    lanes = min(128, W // 4)
    nslot = cdiv(D, 4 * lanes)
    NS = 1 if nslot == 1 else 4 if nslot <= 4 else 8
    UNR = {(1, True): 8, (4, True): 2, (8, True): 1, (1, False): 8, (4, False): 4, (8, False): 2}[(NS, has_m)]
    return lanes, nslot, NS, UNR, has_m


def events2_ok(L, C):
    """events2_ok (N < 2^27 always holds here) -- and smin_clip_event_table's own bounds, so a table exists at all."""
    return C <= 8 and L <= 4096


def event_counts(T, L, C):
    """clip_event_table_kernel's count per frame: every cell (i, w) with a clip boundary at t (start of clip q < nclip, end of
    clip q - 1 for 1 <= q <= nclip, base = t - i r = q cs)."""
    r = T // L
    i = np.arange(L).reshape(L, 1)
    w = np.arange(1, L + 1).reshape(1, L)
    ok = (i + w - 1) < L
    nf = w * r
    cs = np.maximum(1, nf // C)
    nclip = np.minimum(C, nf)
    out = np.zeros(T, dtype=np.int64)
    for t in range(T):
        base = t - i * r
        rows = (i <= min(L - 1, t // r)) & ok
        q = base // cs
        hit = rows & (q * cs == base)
        out[t] = int((hit & (q < nclip)).sum() + (hit & (q >= 1) & (q <= nclip)).sum())
    return out


def rows_reduce_slices(L):
    """smin_boundary_unit_bwd: dfs is reduced over the L rows in one pass for L <= 96, else in cdiv(L, 32) slices and a second pass."""
    return cdiv(L, 32) if L > 96 else 1


tn_splits = H.tn_splits            # gemm.h tn_splits (one mirror for every test file)


def parent_bu_ws_floats(B, L, Nq, D):
    """The boundary backward's workspace as the hosts reserved it before smin_boundary_unit_bwd_ws_bytes (2 x 64 TN slabs)."""
    return 2 * B * L * L + 3 * B * L * D + B * L * Nq + B * Nq * D + 2 * 64 * (D * D + D)


def bu_ws_floats(B, L, Nq, D):
    """What smin_boundary_unit_bwd carves (BuBwdWs), each piece padded to 4 floats."""
    p = lambda n: (n + 3) // 4 * 4
    sl = rows_reduce_slices(L)
    s1, s2 = tn_splits(B * L, D, D), tn_splits(B * Nq, D, D)
    return (2 * p(B * L * L) + 3 * p(B * L * D) + p(B * L * Nq) + p(B * Nq * D) + p(B * sl * D if sl > 1 else 0)
            + p(s1 * D * D) + p(s1 * D) + p(s2 * D * D) + p(s2 * D))


def test_event_count_mirror_busiest_frame():
    """At T = L = 256, C = 4 the busiest frame has 1443 clip boundaries: more than one 1024-entry round of the events2 kernel."""
    cnt = event_counts(256, 256, 4)
    assert cnt.max() == 1443 and cnt.max() > EV_ROUND


def test_boundary_workspace_arithmetic():
    """tn_splits allows up to 768 splits per contraction (capped at B L / 256): the 2 x 64 slabs the header documented fall short
    beyond ~32 K rows at D <= 256 (the hosts' workspaces grow with 25 % slack, which hid it), and the two-pass rows_reduce buffer [B][cdiv(L, 32)][D] outgrows draw [B][L][L] once D > L^2 / cdiv(L, 32)."""
    assert tn_splits(130 * 256, 128, 128) == 130 > 64
    assert bu_ws_floats(130, 256, 1, 128) > parent_bu_ws_floats(130, 256, 1, 128)
    assert tn_splits(64 * 512, 256, 256) == 128 and bu_ws_floats(64, 512, 20, 256) > parent_bu_ws_floats(64, 512, 20, 256)
    assert cdiv(97, 32) * 2400 > 97 * 97
    assert 4 * (2 * 8192 + 64) > 64 * 1024 >= 4 * (2 * 8160 + 64)


# ---------------------------------------------------------------- GPU case lists

# proposal map (ProposalGeneration through smin_proposal_map_fwd / _bwd): (B, T, L, C, D, layout, mask)
PM_CASES = [
    (3, 16, 8, 4, 24, "from_mask", "ragged"),       # D/4 = 6 lanes: 21 groups, 2 idle threads
    (2, 16, 16, 4, 64, "all_cells", "ragged"),      # masked cells listed
    (1, 6, 3, 2, 8, "from_mask", "tri"),            # T < 16
    (7, 40, 10, 3, 68, "from_mask", "ragged"),      # T % 16 != 0, D % 64 != 0
    (9, 32, 8, 4, 256, "all_cells", "tri"),
    (2, 16, 4, 4, 2048, "from_mask", "tri"),        # D = 2048: four column passes, NS = 4
    (2, 24, 6, 3, 516, "all_cells", "ragged"),      # D > 512, not a multiple of 512
    (2, 272, 16, 4, 68, "from_mask", "ragged"),     # T > 256: segments streamed from memory
    (1, 1024, 8, 8, 8, "from_mask", "tri"),
    (2, 256, 256, 4, 8, "from_mask", "ragged"),     # > 1024 events in a frame: several LDS rounds
    (1, 256, 256, 4, 8, "all_cells", "tri"),
    (37, 8, 4, 2, 8, "from_mask", "ragged"),        # per-sample XCD remap over five groups of eight
    (2, 27, 9, 9, 20, "all_cells", "ragged"),       # C > 8: no table, the in-kernel event search
    (2, 12, 6, 3, 16, "from_mask", "none"),         # N = 0
]

# clip-window means (the content stream's linear_c_hat): (B, T, L, C, W, nseg, bias segments, mask)
CWM_CASES = [
    (2, 16, 8, 4, 24, 1, 1, "tri"),
    (3, 32, 8, 3, 16, 2, 1, "ragged"),
    (2, 20, 10, 4, 64, 3, 2, "ragged"),
    (1, 16, 16, 4, 32, 4, 0, "tri"),
    (2, 24, 12, 2, 8, 5, 3, "ragged"),
    (9, 16, 8, 4, 12, 6, 6, "ragged"),
    (2, 16, 4, 4, 128, 7, 7, "tri"),
    (1, 32, 16, 3, 256, 8, 4, "ragged"),
    (2, 16, 8, 4, 520, 2, 1, "ragged"),             # W > 512: the in-kernel event search
    (2, 300, 10, 4, 12, 3, 1, "tri"),               # T > 256
]

# boundary unit: (B, L, Nq, D, layout, mask)
BU_CASES = [
    (3, 1, 3, 36, "all_cells", "tri"),
    (2, 2, 4, 4, "from_mask", "tri"),
    (4, 63, 5, 252, "from_mask", "ragged"),
    (2, 96, 16, 256, "all_cells", "ragged"),
    (3, 97, 17, 260, "from_mask", "ragged"),
    (2, 129, 32, 36, "all_cells", "band8"),
    (2, 512, 64, 4, "from_mask", "band6"),
    (2, 8, 1, 1024, "all_cells", "ragged"),
    (1, 16, 5, 2048, "from_mask", "tri"),
    (130, 256, 1, 128, "from_mask", "band2"),       # 130 TN splits per contraction: more workspace than 2 x 64 slabs
    (1, 97, 3, 2400, "from_mask", "ragged"),        # two-pass rows_reduce buffer larger than draw
    (1, 8192, 1, 4, "from_mask", "band2"),          # the forward's limit: 65.8 KB of LDS in the column backward
]

# moment unit: (B, L, D, layout, operand, mask)   operand: "pairmean" (generated in the contraction), "x1", "x1h" (bf16 stored)
MU_CASES = [
    (1, 7, 32, "from_mask", "pairmean", "tri"),
    (9, 6, 64, "all_cells", "pairmean", "ragged"),
    (2, 12, 132, "from_mask", "x1", "ragged"),
    (9, 5, 48, "all_cells", "x1", "tri"),
    (2, 9, 64, "from_mask", "x1h", "ragged"),
    (2, 6, 16, "from_mask", "pairmean", "none"),    # N = 0: the weight gradient is a memset
]

# score map: (B, L, D, layout, mask)
SC_CASES = [
    (3, 7, 36, "from_mask", "ragged"),
    (2, 11, 516, "all_cells", "ragged"),
    (9, 13, 1024, "from_mask", "tri"),
    (1, 64, 8, "from_mask", "tri"),
]


def _pm_forms(case):
    B, T, L, C, D, layout, mask = case
    forms = {("time_scan", "small" if time_scan_small(T) else "streamed"), ("pm_fwd", "fc+fm"), ("pm_fwd", "fm")}
    if T % 16:
        forms.add(("time_scan", "T%16"))
    if T < 16:
        forms.add(("time_scan", "T<16"))
    forms.add(("time_scan", "D=2048" if D == 2048 else "D%64" if D % 64 else "D64"))
    if D > 512:
        forms.add(("pm_fwd", "D>512"))
    if layout == "all_cells":
        forms.add(("pm_fwd", "masked cells"))
    forms.add(("B", B))
    if mask == "none":
        forms.add(("pm_fwd", "N=0"))
        return forms
    forms |= {("pm_bwd", "dfc=None"), ("pm_bwd", "dfb only"), ("bwd_events", "no table")}
    if events2_ok(L, C):
        for has_m in (True, False):
            _, _, NS, UNR, _ = events2_form(D, D, has_m)
            forms.add(("events2", NS, UNR, has_m))
        lanes = events2_form(D, D, True)[0]
        if 128 // lanes > 1:
            forms.add(("events2", "groups>1"))
        if 128 % lanes:
            forms.add(("events2", "idle threads"))
        if event_counts(T, L, C).max() > EV_ROUND:
            forms.add(("events2", "rounds>1"))
    else:
        forms.add(("bwd_events", "C>8" if C > 8 else "L>4096"))
    return forms


def _cwm_forms(case):
    B, T, L, C, W, nseg, nbs, mask = case
    forms = {("cwm", "nseg", nseg), ("time_scan", "small" if time_scan_small(T) else "streamed"), ("bwd_events", "no table")}
    if W > 512 or not events2_ok(L, C):
        forms.add(("bwd_events", "W>512" if W > 512 else "C>8"))
    else:
        _, _, NS, UNR, _ = events2_form(W * nseg, W, False)
        forms.add(("events2", NS, UNR, False))
    return forms


def _bu_forms(case):
    B, L, Nq, D, layout, mask = case
    return {("bu", "Nq", Nq), ("bu", "D", D), ("bu", "L", L), ("bu", "rows_reduce", "two-pass" if rows_reduce_slices(L) > 1 else "one-pass"),
            ("bu", layout), ("bu", "splits>64" if tn_splits(B * L, D, D) > 64 else "splits<=64")}


def _mu_forms(case):
    B, L, D, layout, operand, mask = case
    return {("mu", layout), ("mu", operand), ("mu", "B", B), ("mu", "N=0" if mask == "none" else "N>0")}


def _sc_forms(case, N):
    B, L, D, layout, mask = case
    return {("sc", "N%64" if N % 64 else "N%64=0"), ("sc", "BL%8" if (B * L) % 8 else "BL%8=0"), ("sc", "D<512" if D < 512 else "D>512"),
            ("sc", "absent cells" if N < B * L * L else "every cell")}


def _sc_count(case):
    B, L, D, layout, mask = case
    if layout == "all_cells":
        return B * L * L
    return int(moment_mask(B, L, mask, default_lens(B, L), torch.Generator().manual_seed(B * 1000 + L)).sum())


REQUIRED = (
    {("time_scan", f) for f in ("small", "streamed", "T%16", "T<16", "D%64", "D=2048")}
    | {("pm_fwd", f) for f in ("fc+fm", "fm", "D>512", "masked cells", "N=0")}
    | {("events2", NS, {(1, True): 8, (4, True): 2, (1, False): 8, (4, False): 4, (8, False): 2}[(NS, m)], m)
       for NS, m in ((1, True), (4, True), (1, False), (4, False), (8, False))}
    | {("events2", f) for f in ("groups>1", "idle threads", "rounds>1")}
    | {("B", b) for b in (1, 7, 9, 37)}
    | {("bwd_events", f) for f in ("no table", "C>8", "W>512")}
    | {("pm_bwd", "dfc=None"), ("pm_bwd", "dfb only")}
    | {("cwm", "nseg", k) for k in range(1, 9)}
    | {("bu", "Nq", n) for n in (1, 3, 4, 5, 16, 17, 32, 64)}
    | {("bu", "D", d) for d in (4, 36, 252, 256, 260, 1024, 2048)}
    | {("bu", "L", n) for n in (1, 2, 63, 96, 97, 129, 512)}
    | {("bu", "rows_reduce", "one-pass"), ("bu", "rows_reduce", "two-pass"), ("bu", "from_mask"), ("bu", "all_cells"), ("bu", "splits>64")}
    | {("mu", f) for f in ("from_mask", "all_cells", "pairmean", "x1", "x1h", "N=0")} | {("mu", "B", 1), ("mu", "B", 9)}
    | {("sc", f) for f in ("N%64", "BL%8", "D<512", "D>512", "absent cells")}
)


def test_map_cases_reach_every_form():
    """The GPU case lists together reach every form of the table: time_scan's register and streamed segments, the proposal map's
    forward forms, every proposal_map_bwd_events2_kernel instance a caller can pick, several LDS rounds, the per-sample XCD remap,
    the in-kernel event search for each of its three reasons, nseg 1..8, and the boundary / moment / score shapes."""
    reached = set()
    for c in PM_CASES:
        reached |= _pm_forms(c)
    for c in CWM_CASES:
        reached |= _cwm_forms(c)
    for c in BU_CASES:
        reached |= _bu_forms(c)
    for c in MU_CASES:
        reached |= _mu_forms(c)
    for c in SC_CASES:
        reached |= _sc_forms(c, _sc_count(c))
    missing = REQUIRED - reached
    assert not missing, sorted(map(str, missing))
    # (NS = 8, HAS_M) exists as a template but no caller picks it: dfm comes with a dense gradient only, whose D <= 2048 needs <= 4 slots
    assert all(events2_form(D, D, True)[2] <= 4 for D in range(4, 2049, 4))
    assert all(events2_form(W * n, W, False)[2] == (1 if n == 1 else 4 if n <= 4 else 8) for W in range(4, 513, 4) for n in range(1, 9) if W * n <= 2048)


# ---------------------------------------------------------------- GPU helpers
def _rel(got, ref, scale=0.0):
    """max |got - ref| / max(max |ref|, scale)"""
    if not ref.numel():
        return 0.0
    return (got.double().cpu() - ref.detach()).abs().max().item() / max(ref.detach().abs().max().item(), scale, 1e-30)


def _nan(shape, dev, dtype=torch.float32):
    return torch.full(shape, float("nan"), dtype=dtype, device=dev)


def _ws_nan(nbytes, dev):
    w = _nan((max(1, cdiv(int(nbytes), 4)),), dev)
    return w, w.numel() * 4


def _check(label, what, got, ref, tol, worst, key, scale=0.0):
    e = _rel(got, ref, scale)
    worst[key] = max(worst.get(key, 0.0), e)
    assert e <= tol, (label, what, e)


def _report(family, label, worst):
    print(f"{family} {label}: worst fwd {worst.get('f', 0.0):.2e} grad {worst.get('g', 0.0):.2e}")


# ---------------------------------------------------------------- GPU: proposal map

def _pm_id(c):
    return "B{}_T{}_L{}_C{}_D{}_{}_{}".format(*c)


@pytest.mark.gpu
@pytest.mark.parametrize("case", PM_CASES, ids=[_pm_id(c) for c in PM_CASES])
def test_proposal_map_against_fp64(dev, case):
    from vml_amd._lib import call, ptr, stream
    from vml_amd.functional import clip_event_table
    B, T, L, C, D, layout, mask = case
    label = _pm_id(case)
    g = torch.Generator().manual_seed(T * 7 + L * 3 + C + D + B)
    mm = moment_mask(B, L, mask, default_lens(B, L), g)
    lay = make_layout(mm, layout)
    N = lay.N
    f = torch.randn(B, T, D, generator=g, dtype=torch.float64).requires_grad_(True)
    fc0, fm0, fb0 = proposal_map_ref(f, lay.cells, T, L, C)
    G = {k: torch.randn(x.shape, generator=g, dtype=torch.float64) for k, x in (("c", fc0), ("m", fm0), ("b", fb0))}
    vjp = {k: (torch.autograd.grad((x * G[k]).sum(), f, retain_graph=True)[0] if x.numel() else torch.zeros_like(f))
           for k, x in (("c", fc0), ("m", fm0), ("b", fb0))}
    lay_d = _layout_to(lay, dev)
    fd = f.detach().float().to(dev)
    worst = {}
    for with_fc in (True, False):
        fc = _nan((N, C, D), dev) if with_fc else None
        fm, fb = _nan((N, D), dev), _nan((B, L, D), dev)
        ws, wn = _ws_nan(8 * B * (T + 1) * D, dev)
        call("smin_proposal_map_fwd", stream(), ptr(fd), ptr(lay_d.cells), N, B, T, L, C, D, _vp(fc), _vp(fm), ptr(fb), ptr(ws), wn)
        if with_fc:
            _check(label, "fc", fc, fc0, FWD_TOL, worst, "f")
        _check(label, "fm" + ("" if with_fc else " (means only)"), fm, fm0, FWD_TOL, worst, "f")
        _check(label, "fb", fb, fb0, FWD_TOL, worst, "f")
    Gd = {k: v.float().to(dev) for k, v in G.items()}
    tables = ([clip_event_table(dev, T, L, C)] if events2_ok(L, C) else []) + [(None, None)]
    if events2_ok(L, C):
        off = tables[0][0].cpu().numpy()
        assert np.array_equal(np.diff(off), event_counts(T, L, C)), label
    for eo, et in tables:
        for combo in ("cmb", "mb", "cb", "b", "cm"):
            def run():
                df = _nan((B, T, D), dev)
                ws, wn = _ws_nan(4 * B * T * D, dev)
                call("smin_proposal_map_bwd", stream(), _vp(Gd["c"]) if "c" in combo else None, _vp(Gd["m"]) if "m" in combo else None,
                     ptr(Gd["b"]) if "b" in combo else None, ptr(lay_d.cells), ptr(lay_d.row_ptr), ptr(lay_d.cellmap), N, B, T, L, C, D,
                     ptr(df), ptr(ws), wn, _vp(eo), _vp(et))
                return df
            df = run()
            _check(label, f"df[{combo}, table={eo is not None}]", df, sum(vjp[k] for k in combo), GRAD_TOL, worst, "g")
            assert torch.equal(df, run()), (label, combo, "backward not deterministic")
    _report("proposal_map", label, worst)


def _cwm_id(c):
    return "B{}_T{}_L{}_C{}_W{}_nseg{}_bias{}_{}".format(*c)


@pytest.mark.gpu
@pytest.mark.parametrize("case", CWM_CASES, ids=[_cwm_id(c) for c in CWM_CASES])
def test_clip_window_means_against_fp64(dev, case):
    from vml_amd._lib import call, ptr, stream
    from vml_amd.functional import clip_event_table
    B, T, L, C, W, nseg, nbs, mask = case
    label = _cwm_id(case)
    D = W * nseg
    g = torch.Generator().manual_seed(T + L + C + W + nseg)
    mm = moment_mask(B, L, mask, default_lens(B, L), g)
    lay = make_layout(mm, "from_mask")
    N = lay.N
    gf = torch.randn(B, T, D, generator=g, dtype=torch.float64).requires_grad_(True)
    bias = torch.randn(nbs * W, generator=g, dtype=torch.float64) if nbs else None
    refs = clip_window_means_ref(gf, bias, lay.cells, T, L, C, nseg)
    G = [torch.randn(r.shape, generator=g, dtype=torch.float64) for r in refs]
    dg0 = torch.autograd.grad(sum((r * x).sum() for r, x in zip(refs, G)), gf)[0]
    lay_d = _layout_to(lay, dev)
    worst = {}
    out = _nan((nseg, N * C, W), dev)
    ws, wn = _ws_nan(8 * B * (T + 1) * D, dev)
    bd = bias.float().to(dev) if nbs else None
    call("smin_clip_window_means_fwd", stream(), ptr(gf.detach().float().to(dev)), _vp(bd), nbs * W, ptr(lay_d.cells), N, B, T, L, C, W, nseg,
         ptr(out), ptr(ws), wn)
    for s in range(nseg):
        _check(label, f"out[{s}]", out[s], refs[s], FWD_TOL, worst, "f")
    Gd = [x.float().to(dev) for x in G]
    arr = (ctypes.c_void_p * nseg)(*[x.data_ptr() for x in Gd])
    tables = ([clip_event_table(dev, T, L, C)] if events2_ok(L, C) else []) + [(None, None)]
    for eo, et in tables:
        def run():
            dg = _nan((B, T, D), dev)
            ws, wn = _ws_nan(4 * B * T * D, dev)
            call("smin_clip_window_means_bwd", stream(), arr, ptr(lay_d.cells), ptr(lay_d.row_ptr), ptr(lay_d.cellmap), N, B, T, L, C, W, nseg,
                 ptr(dg), ptr(ws), wn, _vp(eo), _vp(et))
            return dg
        dg = run()
        _check(label, f"dg[table={eo is not None}]", dg, dg0, GRAD_TOL, worst, "g")
        assert torch.equal(dg, run()), (label, "backward not deterministic")
    _report("clip_window_means", label, worst)


# ---------------------------------------------------------------- GPU: boundary unit

def _bu_id(c):
    return "B{}_L{}_Nq{}_D{}_{}_{}".format(*c)


def _bu_inputs(B, L, Nq, D, mask, g, spread=1.5):
    """Inputs whose two softmaxes are spread: f_b rows are mostly a per-row multiple of one direction, so that the self-attention
    logits <bqv_i, bqv_j> / sqrt(D) vary along the row instead of being dominated by the diagonal.  spread: the standard deviation both
    logit tensors are scaled to."""
    lens = default_lens(B, L)
    if B >= 3:
        lens[2] = 0                                                   # a sample of length 0
    lm = lengths_mask(B, L, lens).double()
    mm = moment_mask(B, L, mask, lens, g)
    qmask = torch.ones(B, Nq, dtype=torch.float64)
    for b in range(B):
        if b % 2 == 1 and Nq > 1:
            qmask[b, Nq - Nq // 3:] = 0                                  # padded words
        if b % 3 == 1:
            qmask[b, 0] = 0.5                                            # fractional weights
            qmask[b, Nq // 2] *= 0.25
    if B >= 4:
        qmask[3] = 0                                                     # a query with every word masked
    e = torch.randn(D, generator=g, dtype=torch.float64)
    u = torch.randn(B, L, 1, generator=g, dtype=torch.float64)
    fb = u * e + 0.35 * torch.randn(B, L, D, generator=g, dtype=torch.float64)
    fw = torch.randn(B, Nq, D, generator=g, dtype=torch.float64)
    fs = torch.randn(B, D, generator=g, dtype=torch.float64)
    p = _bu_params(D, g)
    # scale f_b (self logits ~ f_b^2) and W_k, b_k (word logits, exactly linear) to a spread of about 1.5
    no_cells = torch.zeros(0, 4, dtype=torch.int32)
    wlive, slive = (qmask > 0).unsqueeze(1) & (lm > 0).unsqueeze(-1), (lm > 0).unsqueeze(1) & (lm > 0).unsqueeze(-1)
    for _ in range(3):
        _, _, _, S, Z, _ = boundary_unit_ref(fb, fw, fs, fb.new_zeros(0, D), no_cells, p["W_q.weight"], p["W_q.bias"], p["W_k.weight"],
                                             p["W_k.bias"], qmask, lm)
        sz = _spread(Z, slive)
        if sz:
            fb = fb * math.sqrt(spread / sz)
        _, _, _, S, Z, _ = boundary_unit_ref(fb, fw, fs, fb.new_zeros(0, D), no_cells, p["W_q.weight"], p["W_q.bias"], p["W_k.weight"],
                                             p["W_k.bias"], qmask, lm)
        sw = _spread(S, wlive)
        if sw:
            p["W_k.weight"], p["W_k.bias"] = p["W_k.weight"] * (spread / sw), p["W_k.bias"] * (spread / sw)
    return lm, mm, qmask, fb, fw, fs, p


@pytest.mark.gpu
@pytest.mark.parametrize("case", BU_CASES, ids=[_bu_id(c) for c in BU_CASES])
def test_boundary_unit_against_fp64(dev, case):
    import models
    from vml_amd._lib import call, ptr, stream
    F = models.vml_amd.functional
    B, L, Nq, D, layout, mask = case
    label = _bu_id(case)
    g = torch.Generator().manual_seed(B * 7 + L + Nq + D)
    lm, mm, qmask, fb, fw, fs, p = _bu_inputs(B, L, Nq, D, mask, g)
    lay = make_layout(mm, layout)
    N = lay.N
    hbar = torch.randn(N, D, generator=g, dtype=torch.float64)
    x = dict(fb=fb, fw=fw, fs=fs, hbar=hbar, Wq=p["W_q.weight"], bq=p["W_q.bias"], Wk=p["W_k.weight"], bk=p["W_k.bias"])
    names = list(x)
    leaves = {k: v.clone().requires_grad_(True) for k, v in x.items()}
    out0, P0, A0, S0, Z0, Kb0 = boundary_unit_ref(leaves["fb"], leaves["fw"], leaves["fs"], leaves["hbar"], lay.cells, leaves["Wq"], leaves["bq"],
                                                  leaves["Wk"], leaves["bk"], qmask, lm)
    _assert_spread(S0.detach(), (qmask > 0).unsqueeze(1) & (lm > 0).unsqueeze(-1), label, "word")
    _assert_spread(Z0.detach(), (lm > 0).unsqueeze(1) & (lm > 0).unsqueeze(-1), label, "self")
    G = torch.randn(B, L, D, generator=g, dtype=torch.float64)
    *gl, dKb0 = torch.autograd.grad((out0 * G).sum(), [leaves[k] for k in names] + [Kb0])
    grads0 = dict(zip(names, gl))
    # W_k's bias shifts every word logit of a row alike: the softmax cancels it but for fractional word weights, so dbk is often
    # (near) zero -- it is held to the magnitude of the word sum it is, sum_w |dKb[w]|, instead
    scale = {"bk": dKb0.abs().sum((0, 1)).max().item()}
    # a boundary row sums L fp32 terms in order (softmax denominator, A f_b, the column sums of the backward): beyond L = 512 the
    # bounds grow as sqrt(L / 512)
    ftol, gtol = (FWD_TOL * max(1.0, math.sqrt(L / 512)), GRAD_TOL * max(1.0, math.sqrt(L / 512)))
    del S0, Z0
    lay_d = _layout_to(lay, dev)
    d = {k: v.float().to(dev) for k, v in x.items()}
    qm_d, lm_d, G_d = qmask.float().to(dev), lm.float().to(dev), G.float().to(dev)
    worst = {}

    # the Python host's autograd.Function (its own workspace sizing)
    lv = {k: v.clone().requires_grad_(True) for k, v in d.items()}
    out = F.BoundaryUnitFn.apply(lv["fb"], lv["fw"], lv["fs"], lv["hbar"], lv["Wq"], lv["bq"], lv["Wk"], lv["bk"], qm_d, lm_d, lay_d)
    _check(label, "out (BoundaryUnitFn)", out.detach(), out0, ftol, worst, "f")
    gfn = dict(zip(names, torch.autograd.grad((out * G_d).sum(), [lv[k] for k in names])))
    for k in names:
        _check(label, "d" + k + " (BoundaryUnitFn)", gfn[k], grads0[k], gtol, worst, "g", scale.get(k, 0.0))

    # the C ABI into NaN-prefilled buffers
    outc, Qb, baq, bqv = (_nan((B, L, D), dev) for _ in range(4))
    Kb, P, A = _nan((B, Nq, D), dev), _nan((B, L, Nq), dev), _nan((B, L, L), dev)
    call("smin_boundary_unit_fwd", stream(), ptr(d["fb"]), ptr(d["fw"]), ptr(d["fs"]), _vp(d["hbar"]), ptr(lay_d.cells), ptr(lay_d.row_ptr),
         N, B, L, Nq, D, ptr(d["Wq"]), ptr(d["bq"]), ptr(d["Wk"]), ptr(d["bk"]), ptr(qm_d), ptr(lm_d),
         ptr(outc), ptr(Qb), ptr(Kb), ptr(P), ptr(baq), ptr(bqv), ptr(A))
    _check(label, "out", outc, out0, ftol, worst, "f")
    _check(label, "P", P, P0, ftol, worst, "f")
    _check(label, "A", A, A0, ftol, worst, "f")
    assert torch.equal(outc, out.detach()), label
    nbytes = models.vml_amd._lib.load().smin_boundary_unit_bwd_ws_bytes(B, L, Nq, D)
    assert nbytes > 0
    WqT, WkT = d["Wq"].t().contiguous(), d["Wk"].t().contiguous()

    def run(with_dhbar=True):
        o = {k: _nan(v.shape, dev) for k, v in d.items()}
        if not with_dhbar:
            o["hbar"] = None
        ws, wn = _ws_nan(nbytes, dev)
        call("smin_boundary_unit_bwd", stream(), ptr(G_d), ptr(d["fb"]), ptr(d["fw"]), ptr(d["fs"]), _vp(d["hbar"]), ptr(lay_d.cells),
             ptr(lay_d.row_ptr), N, B, L, Nq, D, ptr(WqT), ptr(WkT), ptr(qm_d), ptr(lm_d), ptr(Qb), ptr(Kb), ptr(P), ptr(baq), ptr(bqv), ptr(A),
             ptr(o["fb"]), ptr(o["fw"]), ptr(o["fs"]), _vp(o["hbar"]), ptr(o["Wq"]), ptr(o["bq"]), ptr(o["Wk"]), ptr(o["bk"]), ptr(ws), wn)
        return o
    gc = run()
    for k in names:
        _check(label, "d" + k, gc[k], grads0[k], gtol, worst, "g", scale.get(k, 0.0))
        assert torch.equal(gc[k], gfn[k]), (label, k, "C ABI and BoundaryUnitFn differ")
    again = run()
    assert all(torch.equal(gc[k], again[k]) for k in names), (label, "backward not deterministic")
    nod = run(with_dhbar=False)                                        # the native host forms dhbar in the gate backward
    assert all(torch.equal(gc[k], nod[k]) for k in names if k != "hbar"), (label, "dhbar == NULL changes the other gradients")
    _report("boundary_unit", label, worst)


@pytest.mark.gpu
def test_boundary_unit_workspace_refusals(dev):
    """The size function and the backward agree on what they accept: L beyond the forward's limit is refused by both."""
    import models
    lib = models.vml_amd._lib.load()
    assert lib.smin_boundary_unit_bwd_ws_bytes(1, 8192, 1, 4) > 0
    assert lib.smin_boundary_unit_bwd_ws_bytes(1, 8193, 1, 4) == 0
    assert lib.smin_boundary_unit_bwd_ws_bytes(1, 16, 65, 4) == 0
    assert lib.smin_boundary_unit_bwd_ws_bytes(1, 16, 4, 6) == 0
    for c in BU_CASES:
        B, L, Nq, D = c[:4]
        assert lib.smin_boundary_unit_bwd_ws_bytes(B, L, Nq, D) == 4 * bu_ws_floats(B, L, Nq, D), c


# ---------------------------------------------------------------- GPU: moment unit

def _mu_id(c):
    return "B{}_L{}_D{}_{}_{}_{}".format(*c)


@pytest.mark.gpu
@pytest.mark.parametrize("case", MU_CASES, ids=[_mu_id(c) for c in MU_CASES])
def test_moment_unit_against_fp64(dev, case):
    import models
    from vml_amd._lib import call, ptr, stream
    B, L, D, layout, operand, mask = case
    label = _mu_id(case)
    g = torch.Generator().manual_seed(B + L * 5 + D)
    mm = moment_mask(B, L, mask, default_lens(B, L), g)
    lay = make_layout(mm, layout)
    N = lay.N
    r = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    x = dict(fcmean=r(N, D), fm=r(N, D), fb=r(B, L, D), Wcat=r(D, 2 * D) / math.sqrt(2 * D), bcat=r(D))
    d = {k: v.float().to(dev) for k, v in x.items()}
    pair_h = None
    if operand == "x1h":
        c = lay.cells.long()
        fb32 = x["fb"].float()
        pair_h = (fb32[c[:, 0], c[:, 1]] * fb32[c[:, 0], c[:, 2]]).to(torch.bfloat16)
    names = ["fcmean", "fb", "Wcat", "bcat"]
    leaves = {k: v.clone().requires_grad_(k in names) for k, v in x.items()}
    mu0 = moment_unit_ref(leaves["fcmean"], leaves["fm"], leaves["fb"], lay.cells, leaves["Wcat"], leaves["bcat"],
                          None if pair_h is None else pair_h.double())
    G, acc_m, acc_b = r(N, D), r(N, D), r(B, L, D)
    grads0 = dict(zip(names, torch.autograd.grad((mu0 * G).sum(), [leaves[k] for k in names]))) if N else \
        {"fcmean": torch.zeros(0, D, dtype=torch.float64), "fb": torch.zeros(B, L, D, dtype=torch.float64),
         "Wcat": torch.zeros(D, 2 * D, dtype=torch.float64), "bcat": torch.zeros(D, dtype=torch.float64)}
    lay_d = _layout_to(lay, dev)
    worst = {}
    x1 = x1h = None
    if operand == "x1":
        x1 = _nan((N, D), dev)
        call("smin_pair_product", stream(), ptr(d["fb"]), ptr(lay_d.cells), N, L, D, _vp(x1))
        c = lay.cells.long()
        _check(label, "x1", x1, x["fb"][c[:, 0], c[:, 1]] * x["fb"][c[:, 0], c[:, 2]], FWD_TOL, worst, "f")
    elif operand == "x1h":
        x1h = torch.empty((N, D), dtype=torch.bfloat16, device=dev)
        call("smin_pair_product_bf16", stream(), ptr(d["fb"]), ptr(lay_d.cells), N, L, D, _vp(x1h))
        assert torch.equal(x1h.cpu(), pair_h), (label, "bf16 pair product is not the round-to-nearest-even of the fp32 product")
    mu = _nan((N, D), dev)
    fwd_args = (ptr(d["fcmean"]), ptr(d["fm"]), ptr(d["fb"]), ptr(lay_d.cells), N, B, L, D, ptr(d["Wcat"]), ptr(d["bcat"]), _vp(mu))
    if operand == "x1h":
        call("smin_moment_unit_fwd_x1h", stream(), *fwd_args, _vp(x1h))
    else:
        call("smin_moment_unit_fwd", stream(), *fwd_args, _vp(x1))
    _check(label, "mu", mu, mu0, FWD_TOL, worst, "f")

    WcatT = d["Wcat"].t().contiguous()
    nbytes = models.vml_amd._lib.load().smin_moment_unit_bwd_ws_bytes(N, B, L, D)
    G_d, am_d, ab_d = G.float().to(dev), acc_m.float().to(dev), acc_b.float().to(dev)
    fn = "smin_moment_unit_bwd_x1h" if operand == "x1h" else "smin_moment_unit_bwd"

    def run(want_in, want_w, accs):
        o = dict(fcmean=_nan((N, D), dev), fb=_nan((B, L, D), dev), Wcat=_nan((D, 2 * D), dev), bcat=_nan((D,), dev))
        ws, wn = _ws_nan(nbytes, dev)
        call(fn, stream(), _vp(G_d), ptr(d["fcmean"]), ptr(d["fb"]), ptr(lay_d.cells), ptr(lay_d.row_ptr), ptr(lay_d.cellmap), N, B, L, D, ptr(WcatT),
             _vp(o["fcmean"]) if want_in else None, ptr(o["fb"]) if want_in else None, ptr(o["Wcat"]) if want_w else None,
             ptr(o["bcat"]) if want_w else None, ptr(ws), wn, int(lay.all_valid), _vp(am_d) if accs else None,
             _vp(x1h if operand == "x1h" else x1), ptr(ab_d) if accs else None)
        return o
    for want_in, want_w, accs in ((True, True, True), (True, True, False), (True, False, False), (False, True, False)):
        o = run(want_in, want_w, accs)
        want = dict(grads0)
        if accs:
            want["fcmean"], want["fb"] = want["fcmean"] + acc_m, want["fb"] + acc_b
        keys = (["fcmean", "fb"] if want_in else []) + (["Wcat", "bcat"] if want_w else [])
        for k in keys:
            _check(label, f"d{k}[in={want_in}, w={want_w}, acc={accs}]", o[k], want[k], GRAD_TOL, worst, "g")
        for k in set(names) - set(keys):
            assert torch.isnan(o[k]).all(), (label, k, "a skipped half wrote its outputs")
        again = run(want_in, want_w, accs)
        assert all(torch.equal(o[k], again[k]) for k in keys), (label, "backward not deterministic")
    _report("moment_unit", label, worst)


# ---------------------------------------------------------------- GPU: score map

def _sc_id(c):
    return "B{}_L{}_D{}_{}_{}".format(*c)


@pytest.mark.gpu
@pytest.mark.parametrize("case", SC_CASES, ids=[_sc_id(c) for c in SC_CASES])
def test_score_map_against_fp64(dev, case):
    import models
    from vml_amd._lib import call, ptr, stream
    B, L, D, layout, mask = case
    label = _sc_id(case)
    lens = default_lens(B, L)
    mm = moment_mask(B, L, mask, lens, torch.Generator().manual_seed(B * 1000 + L))
    lay = make_layout(mm, layout)
    N = lay.N
    assert N == _sc_count(case)
    g = torch.Generator().manual_seed(B + L + D)
    r = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    lm = lengths_mask(B, L, lens).double()
    x = dict(fm=r(N, D), fb=r(B, L, D), wm=r(D) * 1.5 / math.sqrt(D), bm=r(1), wb=r(3, D) * 1.5 / math.sqrt(D), bb=r(3))
    names = list(x)
    leaves = {k: v.clone().requires_grad_(True) for k, v in x.items()}
    pm0, psea0 = score_heads_ref(leaves["fm"], leaves["fb"], lay.cells, leaves["wm"], leaves["bm"], leaves["wb"], leaves["bb"], lm)
    Gm, Gs = r(B, L, L), r(3, B, L)
    gm0 = dict(zip(["fm", "wm", "bm"], torch.autograd.grad((pm0 * Gm).sum(), [leaves[k] for k in ("fm", "wm", "bm")], retain_graph=True)))
    gs0 = dict(zip(["fb", "wb", "bb"], torch.autograd.grad((psea0 * Gs).sum(), [leaves[k] for k in ("fb", "wb", "bb")])))
    lay_d = _layout_to(lay, dev)
    d = {k: v.float().to(dev) for k, v in x.items()}
    lm_d = lm.float().to(dev)
    worst = {}
    pm, psea = _nan((B, L, L), dev), _nan((3, B, L), dev)
    call("smin_score_map_fwd", stream(), ptr(d["fm"]), ptr(d["fb"]), ptr(lay_d.cells), N, B, L, D, ptr(d["wm"]), ptr(d["bm"]), ptr(d["wb"]),
         ptr(d["bb"]), ptr(lm_d), ptr(pm), ptr(psea))
    _check(label, "pm", pm, pm0, FWD_TOL, worst, "f")
    _check(label, "psea", psea, psea0, FWD_TOL, worst, "f")
    assert torch.all(pm.cpu()[lay.cellmap < 0] == 0), (label, "a cell absent from the list must score 0")
    nbytes = models.vml_amd._lib.load().smin_score_map_bwd_ws_bytes(N, B, L, D)
    Gm_d, Gs_d = Gm.float().to(dev), Gs.float().to(dev)

    def run(with_pm, with_sea):
        o = {k: _nan(v.shape, dev) for k, v in d.items()}
        ws, wn = _ws_nan(nbytes, dev)
        call("smin_score_map_bwd", stream(), ptr(Gm_d) if with_pm else None, ptr(Gs_d) if with_sea else None, ptr(pm), ptr(psea), ptr(d["fm"]),
             ptr(d["fb"]), ptr(lay_d.cells), N, B, L, D, ptr(d["wm"]), ptr(d["wb"]), ptr(lm_d), ptr(o["fm"]), ptr(o["fb"]), ptr(o["wm"]),
             ptr(o["bm"]), ptr(o["wb"]), ptr(o["bb"]), ptr(ws), wn)
        return o
    for with_pm, with_sea in ((True, True), (True, False), (False, True)):
        o = run(with_pm, with_sea)
        keys = (["fm", "wm", "bm"] if with_pm else []) + (["fb", "wb", "bb"] if with_sea else [])
        for k in keys:
            _check(label, f"d{k}[pm={with_pm}, psea={with_sea}]", o[k], {**gm0, **gs0}[k], GRAD_TOL, worst, "g")
        for k in set(names) - set(keys):
            assert torch.isnan(o[k]).all(), (label, k, "a skipped half wrote its outputs")
        again = run(with_pm, with_sea)
        assert all(torch.equal(o[k], again[k]) for k in keys), (label, "backward not deterministic")
    _report("score_map", label, worst)


# ---------------------------------------------------------------- saturated inputs: boundary unit

BU_SAT_CASES = [BU_CASES[2], BU_CASES[3]]     # the smallest from_mask case with an empty sample and a query without words; all_cells
BU_NAMES = ("fb", "fw", "fs", "hbar", "Wq", "bq", "Wk", "bk")
LEVELS = ("hard", "frozen")


def _bu_saturated(case, level):
    """test_boundary_unit_against_fp64's inputs with both softmaxes driven by what the float64 reference measures.  frozen: _bu_inputs'
    own scaling aimed at a logit standard deviation of 100.  hard: the rows of the even samples -- the word logits are linear in f_b,
    the self logits quadratic -- scaled by the smallest power of 2^(1/2) at which a quarter of all live rows of either softmax have a
    largest probability above 1 - 1e-6; the odd samples keep their spread of 1.5.  Returns (lm, qmask, lay, x, G)."""
    B, L, Nq, D, layout, mask = case
    g = torch.Generator().manual_seed(B * 7 + L + Nq + D)
    lm, mm, qmask, fb, fw, fs, p = _bu_inputs(B, L, Nq, D, mask, g, spread=100.0 if level == "frozen" else 1.5)
    lay = make_layout(mm, layout)
    hbar, G = torch.randn(lay.N, D, generator=g, dtype=torch.float64), torch.randn(B, L, D, generator=g, dtype=torch.float64)
    x = dict(fb=fb, fw=fw, fs=fs, hbar=hbar, Wq=p["W_q.weight"], bq=p["W_q.bias"], Wk=p["W_k.weight"], bk=p["W_k.bias"])
    x = {k: v.float().double() for k, v in x.items()}
    if level == "hard":
        even = (torch.arange(B) % 2 == 0).double().view(B, 1, 1)
        for e in range(1, 24):
            y = dict(x, fb=(x["fb"] * (1 + even * (2.0 ** (e / 2) - 1))).float().double())
            tw, ts = _bu_tops(y, lay, qmask, lm)
            if (tw > 1 - 1e-6).double().mean().item() >= 0.25 and (ts > 1 - 1e-6).double().mean().item() >= 0.25:
                x = y
                break
        else:
            raise AssertionError(f"no scale puts {_bu_id(case)} into the hard regime")
    return lm, qmask, lay, x, G.float().double()


def _bu_tops(x, lay, qmask, lm):
    """the largest probability of every live row of the word softmax (rows of samples with a word) and of the self softmax"""
    with torch.no_grad():
        _, P, A, S, Z, _ = boundary_unit_ref(x["fb"], x["fw"], x["fs"], x["hbar"], lay.cells, x["Wq"], x["bq"], x["Wk"], x["bk"], qmask, lm)
    rows = lm > 0
    return P.max(-1).values[rows & (qmask > 0).any(1, keepdim=True)], torch.softmax(Z, -1).max(-1).values[rows]


def _bu_refs(x, lay, qmask, lm, G, dtype):
    leaves = {k: v.to(dtype).clone().requires_grad_(True) for k, v in x.items()}
    out, P, A, S, Z, _ = boundary_unit_ref(*[leaves[k] for k in ("fb", "fw", "fs", "hbar")], lay.cells, *[leaves[k] for k in ("Wq", "bq", "Wk", "bk")],
                                           qmask.to(dtype), lm.to(dtype))
    grads = torch.autograd.grad((out * G.to(dtype)).sum(), [leaves[k] for k in BU_NAMES])
    return out.detach(), P.detach(), A.detach(), S.detach(), Z.detach(), dict(zip(BU_NAMES, grads))


@pytest.mark.parametrize("level", LEVELS)
@pytest.mark.parametrize("case", BU_SAT_CASES, ids=[_bu_id(c) for c in BU_SAT_CASES])
def test_boundary_unit_saturated_inputs_hold_what_they_claim(case, level):
    """On the float64 reference, for the word softmax and for the self softmax.  hard: at least a quarter of the live rows with a largest
    probability above 1 - 1e-6 and a quarter below 0.9.  frozen: a logit standard deviation of 100 (to 5 %) and at least 60 % of the rows
    one-hot to 1e-6.  The first case holds a sample of length 0 (rows with length_mask == 0 everywhere) and a query whose every word is
    masked (every logit -1e9: a uniform softmax); both hold rows beyond their sample's length."""
    B, L, Nq, D, layout, mask = case
    lm, qmask, lay, x, G = _bu_saturated(case, level)
    out, P, A, S, Z, grads = _bu_refs(x, lay, qmask, lm, G, torch.float64)
    assert all(bool(torch.isfinite(v).all()) for v in (out, P, A, *grads.values()))
    tw, ts = _bu_tops(x, lay, qmask, lm)
    for top in (tw, ts):
        if level == "hard":
            assert (top > 1 - 1e-6).double().mean().item() >= 0.25 and (top < 0.9).double().mean().item() >= 0.25
        else:
            assert (top > 1 - 1e-6).double().mean().item() >= 0.6
    if level == "frozen":
        sw = _spread(S, (qmask > 0).unsqueeze(1) & (lm > 0).unsqueeze(-1))
        sz = _spread(Z, (lm > 0).unsqueeze(1) & (lm > 0).unsqueeze(-1))
        assert abs(sw - 100) <= 5 and abs(sz - 100) <= 5, (sw, sz)
    assert bool((lm == 0).any())
    if B >= 4:
        assert bool((lm[2] == 0).all()) and bool((qmask[3] == 0).all()) and bool((S[3] == -1e9).all())
        assert (P[3] - 1.0 / Nq).abs().max().item() <= 1e-15


@pytest.mark.gpu
@pytest.mark.parametrize("level", LEVELS)
@pytest.mark.parametrize("case", BU_SAT_CASES, ids=[_bu_id(c) for c in BU_SAT_CASES])
def test_boundary_unit_saturated_against_fp64(dev, case, level):
    """smin_boundary_unit_fwd / _bwd through the C ABI with both softmaxes partly (hard) or wholly (frozen) one-hot, rows beyond the
    length, an empty sample and a query without words: everything finite; out, P and A of the rows beyond the length as the reference
    has them (A exactly 0); the project's gate for out, P, A and the eight gradients against boundary_unit_ref in float64 with
    e_torch32 from the same in fp32.
    Measured on an MI355X: INTEGRATION.md, "Saturated inputs"."""
    import models
    from tests.support.compare import gate
    from vml_amd._lib import call, ptr, stream
    B, L, Nq, D, layout, mask = case
    lm, qmask, lay, x, G = _bu_saturated(case, level)
    N = lay.N
    out0, P0, A0, _, _, g0 = _bu_refs(x, lay, qmask, lm, G, torch.float64)
    out32, P32, A32, _, _, g32 = _bu_refs(x, lay, qmask, lm, G, torch.float32)
    lay_d = _layout_to(lay, dev)
    d = {k: v.float().to(dev) for k, v in x.items()}
    qm_d, lm_d, G_d = qmask.float().to(dev), lm.float().to(dev), G.float().to(dev)
    outc, Qb, baq, bqv = (_nan((B, L, D), dev) for _ in range(4))
    Kb_d, P, A = _nan((B, Nq, D), dev), _nan((B, L, Nq), dev), _nan((B, L, L), dev)
    call("smin_boundary_unit_fwd", stream(), ptr(d["fb"]), ptr(d["fw"]), ptr(d["fs"]), _vp(d["hbar"]), ptr(lay_d.cells), ptr(lay_d.row_ptr),
         N, B, L, Nq, D, ptr(d["Wq"]), ptr(d["bq"]), ptr(d["Wk"]), ptr(d["bk"]), ptr(qm_d), ptr(lm_d),
         ptr(outc), ptr(Qb), ptr(Kb_d), ptr(P), ptr(baq), ptr(bqv), ptr(A))
    nbytes = models.vml_amd._lib.load().smin_boundary_unit_bwd_ws_bytes(B, L, Nq, D)
    WqT, WkT = d["Wq"].t().contiguous(), d["Wk"].t().contiguous()
    o = {k: _nan(v.shape, dev) for k, v in d.items()}
    ws, wn = _ws_nan(nbytes, dev)
    call("smin_boundary_unit_bwd", stream(), ptr(G_d), ptr(d["fb"]), ptr(d["fw"]), ptr(d["fs"]), _vp(d["hbar"]), ptr(lay_d.cells),
         ptr(lay_d.row_ptr), N, B, L, Nq, D, ptr(WqT), ptr(WkT), ptr(qm_d), ptr(lm_d), ptr(Qb), ptr(Kb_d), ptr(P), ptr(baq), ptr(bqv), ptr(A),
         ptr(o["fb"]), ptr(o["fw"]), ptr(o["fs"]), _vp(o["hbar"]), ptr(o["Wq"]), ptr(o["bq"]), ptr(o["Wk"]), ptr(o["bk"]), ptr(ws), wn)
    torch.cuda.synchronize()
    assert all(bool(torch.isfinite(v).all()) for v in (outc, P, A, *o.values()))
    assert bool((A.cpu()[lm == 0] == 0).all())
    tag = f"boundary_unit {_bu_id(case)} {level}"
    gate(tag + " out", outc, out0, out32)
    gate(tag + " P", P, P0, P32)
    gate(tag + " A", A, A0, A32)
    for k in BU_NAMES:
        gate(tag + " d" + k, o[k], g0[k], g32[k])


# ---------------------------------------------------------------- saturated inputs: score map

SC_SAT_CASES = [SC_CASES[0], SC_CASES[1]]     # the smallest case with D < 512 (cells absent from the list) and the one with D > 512
SC_PRE = (20.0, 95.0, 110.0)


def _sc_saturated(case, level):
    """test_score_map_against_fp64's layout and weights with fm and fb moved along the heads' weight vectors so that the four heads'
    pre-activations take given values: +-{20, 95, 110} everywhere (frozen), or on half of the cells and rows with N(0, 2) on the rest
    (hard).  Returns (lay, lm, x, Gm, Gs, the targets of the map head [N] and of the three row heads [3, B, L])."""
    B, L, D, layout, mask = case
    lens = default_lens(B, L)
    lay = make_layout(moment_mask(B, L, mask, lens, torch.Generator().manual_seed(B * 1000 + L)), layout)
    N = lay.N
    g = torch.Generator().manual_seed(B + L + D + len(level))
    r = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    lm = lengths_mask(B, L, lens).double()
    x = dict(fm=r(N, D), fb=r(B, L, D), wm=r(D) * 1.5 / math.sqrt(D), bm=r(1), wb=r(3, D) * 1.5 / math.sqrt(D), bb=r(3))
    x = {k: v.float().double() for k, v in x.items()}

    def targets(*s):
        t = torch.tensor(SC_PRE, dtype=torch.float64)[torch.randint(0, 3, s, generator=g)] * (torch.randint(0, 2, s, generator=g).double() * 2 - 1)
        return t if level == "frozen" else torch.where(torch.rand(*s, generator=g) < 0.5, t, 2 * r(*s))
    tm, tb = targets(N), targets(3, B, L)
    wm, wb = x["wm"], x["wb"]
    x["fm"] = (x["fm"] + ((tm - x["bm"] - x["fm"] @ wm) / (wm @ wm)).unsqueeze(1) * wm).float().double()
    miss = tb - x["bb"].view(3, 1, 1) - torch.einsum("bld,kd->kbl", x["fb"], wb)
    x["fb"] = (x["fb"] + torch.einsum("kbl,kd->bld", torch.linalg.solve(wb @ wb.t(), miss.reshape(3, -1)).reshape(3, B, L), wb)).float().double()
    return lay, lm, x, r(B, L, L).float().double(), r(3, B, L).float().double(), tm, tb


def _sc_refs(lay, lm, x, Gm, Gs, dtype):
    """score_heads_ref and its gradients in ``dtype``: (pm, psea, {name: gradient})"""
    leaves = {k: v.to(dtype).requires_grad_(True) for k, v in x.items()}
    pm, psea = score_heads_ref(leaves["fm"], leaves["fb"], lay.cells, leaves["wm"], leaves["bm"], leaves["wb"], leaves["bb"], lm.to(dtype))
    names = ("fm", "wm", "bm", "fb", "wb", "bb")
    grads = torch.autograd.grad((pm * Gm.to(dtype)).sum() + (psea * Gs.to(dtype)).sum(), [leaves[k] for k in names])
    return pm.detach(), psea.detach(), dict(zip(names, grads))


@pytest.mark.parametrize("level", LEVELS)
@pytest.mark.parametrize("case", SC_SAT_CASES, ids=[_sc_id(c) for c in SC_SAT_CASES])
def test_score_map_saturated_inputs_hold_what_they_claim(case, level):
    """On the float64 reference: the fp32 inputs' pre-activations are the targets to 1e-4; hard -- a quarter of them beyond +-17 and a
    quarter inside +-4; frozen -- all of them at +-{20, 95, 110}, every value under both signs in the map head and in the row heads;
    scores at +20 and above round to 1.0f and those at -110 to 0.0f."""
    lay, lm, x, Gm, Gs, tm, tb = _sc_saturated(case, level)
    zm = x["fm"] @ x["wm"] + x["bm"]
    zb = torch.einsum("bld,kd->kbl", x["fb"], x["wb"]) + x["bb"].view(3, 1, 1)
    assert (zm - tm).abs().max().item() <= 1e-4 and (zb - tb).abs().max().item() <= 1e-4
    for z in (zm, zb):
        if level == "hard":
            assert (z.abs() > 17).double().mean().item() >= 0.25 and (z.abs() < 4).double().mean().item() >= 0.25
        else:
            assert all(bool(((z - s * p).abs() <= 1e-4).any()) for p in SC_PRE for s in (-1, 1)) and z.abs().min().item() > 19.99
    pm, psea, grads = _sc_refs(lay, lm, x, Gm, Gs, torch.float64)
    assert all(bool(torch.isfinite(v).all()) for v in (pm, psea, *grads.values()))
    live = lay.cells[:, 3] != 0
    s = torch.sigmoid(zm)[live]
    assert bool((s[zm[live] > 19.99].float() == 1.0).all()) and bool((s[zm[live] < -109.99].float() == 0.0).all())


@pytest.mark.gpu
@pytest.mark.parametrize("level", LEVELS)
@pytest.mark.parametrize("case", SC_SAT_CASES, ids=[_sc_id(c) for c in SC_SAT_CASES])
def test_score_map_saturated_against_fp64(dev, case, level):
    """smin_score_map_fwd / _bwd on _sc_saturated.  Scores are exactly 1.0 from a pre-activation of +20 on and exactly 0.0 from -110 on;
    cells absent from the list and rows beyond the length are +0.0; wherever the kernel's own score p has p (1 - p) == 0 the gradient
    row of fm (of fb: when all three heads are there) is exactly 0; everything finite; the project's gate against score_heads_ref in
    float64, e_torch32 from the same in fp32.  Measured on an MI355X: INTEGRATION.md, "Saturated inputs"."""
    import models
    from tests.support.compare import gate
    from vml_amd._lib import call, ptr, stream
    B, L, D, layout, mask = case
    lay, lm, x, Gm, Gs, tm, tb = _sc_saturated(case, level)
    N = lay.N
    pm0, psea0, g0 = _sc_refs(lay, lm, x, Gm, Gs, torch.float64)
    pm32, psea32, g32 = _sc_refs(lay, lm, x, Gm, Gs, torch.float32)
    lay_d = _layout_to(lay, dev)
    d = {k: v.float().to(dev) for k, v in x.items()}
    lm_d = lm.float().to(dev)
    pm, psea = _nan((B, L, L), dev), _nan((3, B, L), dev)
    call("smin_score_map_fwd", stream(), ptr(d["fm"]), ptr(d["fb"]), ptr(lay_d.cells), N, B, L, D, ptr(d["wm"]), ptr(d["bm"]), ptr(d["wb"]),
         ptr(d["bb"]), ptr(lm_d), ptr(pm), ptr(psea))
    nbytes = models.vml_amd._lib.load().smin_score_map_bwd_ws_bytes(N, B, L, D)
    o = {k: _nan(v.shape, dev) for k, v in d.items()}
    ws, wn = _ws_nan(nbytes, dev)
    Gm_d, Gs_d = Gm.float().to(dev), Gs.float().to(dev)
    call("smin_score_map_bwd", stream(), ptr(Gm_d), ptr(Gs_d), ptr(pm), ptr(psea), ptr(d["fm"]), ptr(d["fb"]),
         ptr(lay_d.cells), N, B, L, D, ptr(d["wm"]), ptr(d["wb"]), ptr(lm_d), ptr(o["fm"]), ptr(o["fb"]), ptr(o["wm"]), ptr(o["bm"]), ptr(o["wb"]),
         ptr(o["bb"]), ptr(ws), wn)
    torch.cuda.synchronize()
    pm_h, psea_h = pm.cpu(), psea.cpu()
    assert all(bool(torch.isfinite(v).all()) for v in (pm, psea, *o.values()))
    assert bool((pm_h[lay.cellmap < 0].view(torch.int32) == 0).all()) and bool((psea_h[:, lm == 0].view(torch.int32) == 0).all())
    c = lay.cells.long()
    live = c[:, 3] != 0
    at = pm_h[c[:, 0], c[:, 1], c[:, 2]]
    assert bool((at[live & (tm > 19.99)] == 1.0).all()) and bool((at[live & (tm < -109.99)] == 0.0).all())
    on = (lm != 0).expand(3, B, L)
    assert bool((psea_h[on & (tb > 19.99)] == 1.0).all()) and bool((psea_h[on & (tb < -109.99)] == 0.0).all())
    flat = (at * (1 - at) == 0) | ~live
    assert bool(flat.any()) and bool((o["fm"].cpu()[flat] == 0).all())
    flat_rows = ((psea_h * (1 - psea_h)) == 0).all(0)
    assert bool((o["fb"].cpu()[flat_rows] == 0).all())
    tag = f"score_map {_sc_id(case)} {level}"
    gate(tag + " pm", pm, pm0, pm32)
    gate(tag + " psea", psea, psea0, psea32)
    for k in ("fm", "wm", "bm", "fb", "wb", "bb"):
        gate(tag + " d" + k, o[k], g0[k], g32[k])
