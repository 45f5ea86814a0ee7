"""Restatements and hand computations used by more than one test module."""
import math

import numpy as np
import torch

from tests import helpers as H
from tests.helpers import GEMM_SLOTS, cdiv, tn_splits
from tests.support.device import vml


def abi_call(dev, x, plan, tau=0.1, gamma=0.1, fill=float("nan"), **kw):
    """smin_pair_rank_fwd and smin_pair_rank_bwd through the C ABI over outputs pre-filled with ``fill``; kw overrides arguments of the
    forward by name.  Returns (rc_fwd, forward outputs, rc_bwd, backward outputs)."""
    L_ = vml()._lib
    lib = L_.load()
    P, L = x[1].shape
    Q = plan.Q
    pm, ps, pe = (t.to(dev).contiguous() for t in x[:3])
    mm = x[3].to(dev).contiguous()
    full = lambda *shape: torch.full(shape, fill, dtype=torch.float32, device=dev)
    outs = dict(loss=full(1), stats=full(2), score=full(P), coef=full(P), pool=full(P, 2))
    nbytes = lib.smin_pair_rank_ws_bytes(P, Q, L)
    ws = torch.zeros(max(nbytes, 16), dtype=torch.uint8, device=dev)
    a = dict(pm=pm, ps=ps, pe=pe, mm=mm, q_ptr=plan.q_ptr, q_pairs=plan.q_pairs, positive=plan.positive, P=P, Q=Q, L=L, tau=tau, gamma=gamma,
             ws=ws, ws_bytes=nbytes, **outs)
    a.update(kw)
    p = lambda k: L_.ptr(a[k])
    rc = lib.smin_pair_rank_fwd(L_.stream(), p("pm"), p("ps"), p("pe"), p("mm"), p("q_ptr"), p("q_pairs"), p("positive"), a["P"], a["Q"], a["L"],
                                a["tau"], a["gamma"], p("loss"), p("stats"), p("score"), p("coef"), p("pool"), p("ws"), a["ws_bytes"])
    torch.cuda.synchronize()
    return rc, outs, a


def _sample_clips_ref(raw64, lengths, T, spos, mode):
    """sample_clips restated in torch (differentiable): clip_indices / mean_windows on the rows of each sample."""
    from vml_amd.sampling import clip_indices, mean_windows
    offs = np.concatenate([[0], np.cumsum(lengths)])
    rows = []
    for b, n in enumerate(lengths):
        x = raw64[offs[b]:offs[b + 1]]
        out = raw64.new_zeros((T, raw64.shape[1]))
        if mode == "pick" or n <= T:
            idx = clip_indices(n, T, spos[b])
            out = torch.cat([x[torch.from_numpy(idx)], out[idx.shape[0]:]])
        else:
            a = mean_windows(n, T)
            out = torch.stack([x[a[t]:a[t + 1]].sum(0) / float(a[t + 1] - a[t]) for t in range(T)])
        rows.append(out)
    return torch.stack(rows)


def attn_core_ref(chat, cells, C, Mq, uq, what, shat, qmask):
    """The packed attention core (reference models.py:207-226, 252-266) in the layout of ContentAttnFn: chat [N*C, dl], cells
    [N, 4] (b, i, j, m) sorted by sample, per-sample Mq / what [B, Nq, dl], uq / qmask [B, Nq], shat [B, dl].  For each cell of
    sample b with rows X [C, dl] and flag m:
        S = (X Mq_b^T + uq_b) / sqrt(dl);  S = S * qm;  S[qm == 0] = -1e9;  P = softmax over words
        a = m (P what_b);  q = X * (a + shat_b);  A = m softmax_c(q q^T / sqrt(dl));  cc = m (A X);  ccmean = mean_c cc
    Returns (cc [N*C, dl], ccmean [N, dl], S of every cell [N, C, Nq]); differentiable."""
    N, dl = cells.shape[0], chat.shape[1]
    X = chat.reshape(N, C, dl)
    b_of = cells[:, 0].long()
    m_of = cells[:, 3].to(chat.dtype)
    ccs, Ss = [], []
    for b in range(Mq.shape[0]):
        sel = (b_of == b).nonzero().flatten()
        if sel.numel() == 0:
            continue
        assert sel[-1] - sel[0] + 1 == sel.numel(), "cells must be sorted by sample"
        Xb = X[sel[0]:sel[-1] + 1]
        m = m_of[sel[0]:sel[-1] + 1].view(-1, 1, 1)
        qm = qmask[b].view(1, 1, -1)
        S = (Xb @ Mq[b].t() + uq[b]) / math.sqrt(dl)
        Ss.append(S)
        S = (S * qm).masked_fill(qm == 0, -1e9)
        P = torch.softmax(S, dim=-1)
        a = m * (P @ what[b])
        q = Xb * (a + shat[b])
        A = m * torch.softmax(q @ q.transpose(1, 2) / math.sqrt(dl), dim=-1)
        ccs.append(m * (A @ Xb))
    cc = torch.cat(ccs) if ccs else chat.new_zeros((0, C, dl))
    return cc.reshape(N * C, dl), cc.mean(dim=1), (torch.cat(Ss) if Ss else chat.new_zeros((0, C, Mq.shape[1])))


WORD_PARAM_NAMES = ("linear_w_hat.weight", "linear_w_hat.bias", "linear_s_hat.weight", "linear_s_hat.bias",
                    "attn_layer.W_k.weight", "attn_layer.W_k.bias", "attn_layer.W_q.weight", "attn_layer.W_q.bias")


def word_side_ref(fw, fs, qmask, params):
    """The five word-side operands of every layer (csrc/word_prep.hip header), 8 parameters per layer in WordPrepFn's order:
        what = (f_w WH^T + bWH) * qmask;  shat = f_s SH^T + bSH;  kb = what AK^T + bAK;  Mq = kb AQ;  uq = kb . bAQ
    Returns [(what, shat, kb, Mq, uq) per layer]."""
    out = []
    for k in range(len(params) // 8):
        WH, bWH, SH, bSH, AK, bAK, AQ, bAQ = params[8 * k:8 * k + 8]
        what = (fw @ WH.t() + bWH) * qmask.unsqueeze(-1)
        shat = fs @ SH.t() + bSH
        kb = what @ AK.t() + bAK
        out.append((what, shat, kb, kb @ AQ, kb @ bAQ))
    return out


def attn_form(C, dl, Nq):
    """(DL, WS, EXACT) of the instantiation SMIN_ATTN_DISPATCH (csrc/content_attn.hip) picks."""
    nws = (Nq + 3) // 4
    if not (C == 4 and dl in (16, 32, 64, 128)):
        return (16 if dl <= 16 else 32 if dl <= 32 else 64 if dl <= 64 else 128, 8, False)
    if dl < 128:
        return (dl, 4 if nws <= 4 else 8, True)
    return (128, 4 if nws <= 4 else nws if nws <= 6 else 8, True)


ALL_FORMS = ([(dl, ws, True) for dl in (16, 32, 64) for ws in (4, 8)] + [(128, ws, True) for ws in (4, 5, 6, 8)]
             + [(dl, 8, False) for dl in (16, 32, 64, 128)])


def _smi_params(D, dl, gain, seed):
    from oracle import smin_oracle as O
    shapes = {k: v for k, v in H.smin_shapes(32, 8, 4, D, dl, 1, 16, 4, D // 2).items() if k.startswith("smis.0.content_unit.")}
    sd = O.formula_state_dict(shapes, gain=gain)
    g = torch.Generator().manual_seed(seed)
    return {k: (v + 0.05 * gain * torch.randn(v.shape, generator=g)).double() for k, v in sd.items()}


def _query_mask(B, Nq, g):
    """Per sample, cycling: a prefix mask, a mask with holes, fractional weights, and a fully masked query."""
    qm = torch.ones(B, Nq, dtype=torch.float64)
    for b in range(B):
        kind = b % 4
        if kind == 0:
            qm[b, max(1, (2 * Nq + 2) // 3):] = 0
        elif kind == 1:
            qm[b, 1::3] = 0 if Nq > 1 else 1
        elif kind == 2:
            qm[b] = 0.25 + 0.75 * torch.rand(Nq, generator=g, dtype=torch.float64)
            if Nq > 2:
                qm[b, Nq // 2] = 0
        else:
            qm[b] = 0
    return qm


def _attn_inputs(C, dl, Nq, mask, all_cells, seed):
    """Float64 inputs on the CPU for a batch with the given moment mask.  Scales put the word scores' spread near 1 and keep the
    clip softmax off saturation; masked words carry garbage operands (their weight is exactly 0), a fully masked query has zero
    what rows (the pipeline's invariant: what = linear_w_hat(f_w) * qmask)."""
    import models
    g = torch.Generator().manual_seed(seed)
    B = mask.shape[0]
    lay = models.vml_amd.CellLayout.all_cells(mask) if all_cells else models.vml_amd.CellLayout.from_mask(mask)
    r = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    qm = _query_mask(B, Nq, g)
    chat = r(lay.N * C, dl)                                   # masked cells (all_cells) keep nonzero rows
    sw = 0.8 * dl ** -0.25
    Mq, uq, what, shat = 1.2 * r(B, Nq, dl), 0.5 * r(B, Nq), sw * r(B, Nq, dl), sw * r(B, dl)
    off = (qm == 0)
    Mq[off] = 50 * r(int(off.sum()), dl)
    uq[off] = 50 * r(int(off.sum()))
    what[off] = 50 * r(int(off.sum()), dl)
    what[(qm == 0).all(dim=1)] = 0
    x = dict(chat=chat, Mq=Mq, uq=uq, what=what, shat=shat, qmask=qm)
    return lay, {k: v.float().double() for k, v in x.items()}          # the kernels' fp32 inputs, exactly


def _ragged_mask(B, L, g):
    p = torch.tensor([0.55, 0.8, 0.35, 0.7])[torch.arange(B) % 4].view(B, 1, 1)
    return torch.rand(B, L, L, generator=g) < p


def _layout_to(lay, dev):
    import models
    CL = models.vml_amd.CellLayout
    return CL(lay.cells.to(dev), lay.row_ptr.to(dev), lay.cellmap.to(dev), lay.B, lay.L, None, lay.all_valid)


def nt_grid(M, N, K):
    """launch_gemm_nt: 128-row main tiles in XCD-aware order (main_blocks padded to whole groups of 8 row tiles), the rest of the rows
    in 32-row mini tiles; KFULL = K % 16 == 0."""
    tiles_m, tiles_n = cdiv(M, 128), cdiv(N, 128)
    main = tiles_m
    total = tiles_m * tiles_n
    full_rounds = total // GEMM_SLOTS
    if full_rounds >= 1 and total % GEMM_SLOTS != 0 and total % GEMM_SLOTS < 3 * GEMM_SLOTS // 4:
        main = full_rounds * GEMM_SLOTS // tiles_n
    elif total * 3 <= GEMM_SLOTS:
        main = 0
    rem_rows = M - main * 128
    return dict(tiles_m=tiles_m, tiles_n=tiles_n, total=total, main_tiles_m=main, kfull=K % 16 == 0,
                main_blocks=cdiv(main, 8) * 8 * tiles_n, mini_blocks=cdiv(rem_rows, 32) * tiles_n if rem_rows > 0 else 0)


def nt_form(M, N, K):
    g = nt_grid(M, N, K)
    if g["main_tiles_m"] == 0:
        return "mini"
    if g["main_tiles_m"] < g["tiles_m"]:
        return "rounds+mini"
    if g["total"] > GEMM_SLOTS:
        return "main-after-round"                      # a full round, then a remainder >= 3/4 of GEMM_SLOTS: main tiles only
    return "main+idle-slots" if g["main_tiles_m"] % 8 else "main"


def tn_grid(Mrows, I, J):
    """launch_gemm_tn: splits, rows per split (whole 32-row groups), grid (split count padded to a multiple of 8 per output tile)."""
    sp = tn_splits(Mrows, I, J)
    rps = cdiv(cdiv(Mrows, sp), 32) * 32
    tiles = cdiv(I, 128) * cdiv(J, 128)
    return dict(splits=sp, rows_per_split=rps, tiles=tiles, grid=cdiv(sp, 8) * 8 * tiles,
                empty=[z for z in range(sp) if z * rps >= Mrows])


def tn_forms(Mrows, I, J):
    g = tn_grid(Mrows, I, J)
    f = set()
    if g["splits"] == 1:
        f.add("splits=1")
    elif g["splits"] % 8:
        f.add("splits%8!=0")                           # padded XCD slots: workgroups with z >= splits return at once
    if g["empty"]:
        f.add("empty-trailing-split")
    if g["splits"] == GEMM_SLOTS:
        f.add("slots-capped")
    if Mrows < 32:
        f.add("Mrows<32")
    return f


def lengths_mask(B, L, lens):
    return torch.arange(L).view(1, L) < torch.tensor(lens).view(B, 1)


def moment_mask(B, L, kind, lens, g):
    """Upper-triangular mask within each sample's length: "tri" (all of it), "ragged" (a random part), "band<k>" (j - i < k),
    "none" (no cell)."""
    lm = lengths_mask(B, L, lens)
    tri = torch.triu(lm.unsqueeze(2) & lm.unsqueeze(1))
    if kind == "tri":
        return tri
    if kind == "none":
        return torch.zeros_like(tri)
    if kind == "ragged":
        return tri & (torch.rand(B, L, L, generator=g) < 0.6)
    k = int(kind[4:])
    ii, jj = torch.arange(L).view(L, 1), torch.arange(L).view(1, L)
    return tri & ((jj - ii) < k)


def make_layout(mm, layout):
    import models
    CL = models.vml_amd.CellLayout
    return CL.from_mask(mm) if layout == "from_mask" else CL.all_cells(mm)


def py_scores(pm, ps, pe):
    """fp32 score (pm * sqrt(ps_i)) * sqrt(pe_j), -0 -> +0 (numpy fp32 ops are correctly rounded)."""
    pm, ps, pe = (np.asarray(x, dtype=np.float32) for x in (pm, ps, pe))
    s = (pm * np.sqrt(ps)[:, None]) * np.sqrt(pe)[None, :]
    return np.where(s == 0, np.float32(0), s).astype(np.float32)


def py_iou(a, b):
    (i1, j1), (i2, j2) = a, b
    inter = max(0, min(j1, j2) + 1 - max(i1, i2))
    union = max(j1, j2) + 1 - min(i1, i2)
    return np.float32(inter) / np.float32(union)


def py_nms(pm, ps, pe, mm, k, thr):
    """One sample: [(i, j, score)] kept in order."""
    L = pm.shape[0]
    s = py_scores(pm, ps, pe)
    cand = [(-float(s[i, j]), i * L + j) for i in range(L) for j in range(L) if mm[i, j]]
    cand.sort()
    t = np.float32(thr)
    kept = []
    for _, c in cand:
        if len(kept) >= k:
            break
        cell = (c // L, c % L)
        if all(not (py_iou(cell, (a, b)) > t) for a, b, _ in kept):
            kept.append((cell[0], cell[1], s[cell]))
    return kept


def check_against_py(r, pm, ps, pe, mm, k, thr):
    B = pm.shape[0]
    for b in range(B):
        want = py_nms(pm[b].numpy(), ps[b].numpy(), pe[b].numpy(), mm[b].numpy(), k, thr)
        n = len(want)
        assert int(r["count"][b]) == n
        assert r["idx"][b, :n].tolist() == [[i, j] for i, j, _ in want], (b, k, thr)
        assert np.array_equal(r["score"][b, :n].numpy().view(np.int32), np.array([s for _, _, s in want], np.float32).view(np.int32))
        assert (r["idx"][b, n:] == -1).all() and (r["score"][b, n:] == 0).all()


def _api():
    import models
    return models.vml_amd


NAN = float("nan")


def py_span_iou(a, g):
    """include/smin_hip.h, span metric: every operation on np.float32 scalars (each rounded once)."""
    f = np.float32
    st, en, gs, ge = f(a[0]), f(a[1]), f(g[0]), f(g[1])
    inter = max(f(0), min(en, ge) - max(st, gs))
    uni = max(en, ge) - min(st, gs)
    return f(inter) / f(uni) if uni > 0 else f(0)


def py_span_ious(span, count, gt):
    span, count, gt = np.asarray(span, np.float32), np.asarray(count), np.asarray(gt, np.float32)
    B, k = span.shape[0], span.shape[1]
    out = np.zeros((B, k), np.float32)
    for b in range(B):
        for s in range(min(int(count[b]), k)):                                   # an empty slot is never read: IoU exactly 0
            out[b, s] = py_span_iou(span[b, s], gt[b])
    return out


def py_span_hits(ious, count, n, m):
    """{key: pairs with some slot s < min(n, count) whose iou > float32(m)}."""
    out = {}
    for n_ in n:
        for m_ in m:
            c = 0
            for b in range(ious.shape[0]):
                c += any(ious[b, s] > np.float32(m_) for s in range(min(n_, int(count[b]))))
            out[f"R@{n_}, IoU={m_}"] = float(c)
    return out


def edge_cases():
    """k = 5.  Pair by pair: a span equal to the ground truth then a disjoint one; count = 0 with NaN everywhere; empty slots holding
    NaN behind two filled ones; uni == 0 (a point span on a point ground truth); IoUs exactly 0.5 and exactly 0.75 (not hits at
    m = 0.5 / 0.75) next to one just above; a span containing the ground truth; negative coordinates."""
    span = [[[10.0, 20.0], [30.0, 40.0], [NAN, NAN], [NAN, NAN], [NAN, NAN]],
            [[NAN, NAN]] * 5,
            [[0.0, 4.0], [2.5, 7.25], [NAN, NAN], [NAN, NAN], [NAN, NAN]],
            [[3.0, 3.0], [3.0, 3.0], [1.0, 2.0], [NAN, NAN], [NAN, NAN]],
            [[0.0, 4.0], [0.0, 6.0], [0.0, 8.0], [0.0, 7.9999995], [100.0, 101.0]],
            [[-5.0, 50.0], [11.0, 12.5], [10.0, 12.0], [10.5, 12.0], [0.0, 100.0]],
            [[-7.5, -2.25], [-3.0, 1.0], [-10.0, -9.0], [NAN, NAN], [NAN, NAN]]]
    count = [2, 0, 2, 3, 5, 5, 3]
    gt = [[10.0, 20.0], [1.0, 2.0], [1.0, 6.5], [3.0, 3.0], [0.0, 8.0], [10.0, 12.0], [-6.0, -2.0]]
    return torch.tensor(span, dtype=torch.float32), torch.tensor(count, dtype=torch.int32), torch.tensor(gt, dtype=torch.float32)


def random_spans(B, k, seed, nan_valid=False):
    """Spans and ground truths on a 1/8-row grid inside [0, 600): overlaps, containments, equal spans and exact ties with thresholds
    all occur; count ragged (0 .. k), empty slots NaN."""
    g = torch.Generator().manual_seed(seed)
    a = torch.randint(0, 4800, (B, k, 2), generator=g).float() / 8
    span = torch.stack([a.min(dim=2).values, a.max(dim=2).values + 0.125 * torch.randint(0, 2, (B, k), generator=g)], 2)
    c = torch.randint(0, 4800, (B, 2), generator=g).float() / 8
    gt = torch.stack([c.min(dim=1).values, c.max(dim=1).values + 0.125], 1)
    near = torch.rand(B, k, generator=g) < 0.5                                   # half the slots sit near the ground truth
    jitter = torch.randint(-64, 65, (B, k, 2), generator=g).float() / 8
    cand = gt.unsqueeze(1) + jitter
    cand = torch.stack([cand.min(dim=2).values, cand.max(dim=2).values], 2)
    span = torch.where(near.unsqueeze(2), cand, span)
    count = torch.randint(0, k + 1, (B,), generator=g).to(torch.int32)
    count[0] = k
    empty = torch.arange(k).unsqueeze(0) >= count.unsqueeze(1)
    span[empty] = NAN
    return span, count, gt


def merge_frame_edges():
    """merge_window_moments inputs at the edges of the merge kernels' shared frame, with T = L = 8 and k = 3: G = 4 windows of
    k_window = 2 over B = 3 pairs.  pair_ptr starts below 0 and ends above G (both clamped), pair 1 owns no window, window 1 has count
    0 (its slots hold a score that must never be read into the order) and window 2 count 1; scores tie across windows (0.5 three
    times) and one is -0.0.  Returns (idx, score, count, start, lens, pair_ptr)."""
    idx = torch.tensor([[[0, 3], [2, 5]], [[1, 1], [0, 7]], [[4, 6], [3, 3]], [[0, 2], [5, 7]]], dtype=torch.int64)
    score = torch.tensor([[0.5, 0.5], [0.9, 0.1], [-0.0, 0.3], [0.5, 0.25]], dtype=torch.float32)
    count = torch.tensor([2, 0, 1, 2], dtype=torch.int32)
    start = torch.tensor([0, 4, 8, 12], dtype=torch.int64)
    lens = torch.tensor([8, 8, 8, 6], dtype=torch.int32)
    return idx, score, count, start, lens, torch.tensor([-1, 2, 2, 9], dtype=torch.int64)


def backward_rows(tok, table, dqf):
    """embed_tokens(sparse_grad=True) then backward of dqf: table.row_grad"""
    qf, _, _ = vml().embed_tokens(tok, table, differentiable=True, sparse_grad=True)
    qf.backward(dqf)
    assert table.grad is None
    return table.row_grad


def backward_dense(tok, table, dqf):
    table.grad = None
    qf, _, _ = vml().embed_tokens(tok, table, differentiable=True)
    qf.backward(dqf)
    return table.grad


def batches(B, Nq, V, E, steps, seed, cover=False):
    g = torch.Generator().manual_seed(seed)
    out = []
    for _ in range(steps):
        tok = torch.randint(-1, V + 1, (B, Nq), generator=g)             # -1 and V: out of range
        if cover:
            tok = torch.randint(0, V, (B, Nq), generator=g)
            tok.view(-1)[torch.randperm(B * Nq, generator=g)[:V]] = torch.arange(V)
        out.append((tok, torch.randn(B, Nq, E, generator=g) * 10.0 ** torch.randint(-4, 2, (B, Nq, 1), generator=g).float()))
    return out


def collapsed_pm(sd, seams, batch, nl):
    """pm of the collapsed last layer (fp32): ccmean re-formed from the last layer's inputs with the oracle's own pieces."""
    from oracle import smin_oracle as O
    score_tail_torch = vml().functional.score_tail_torch
    k = nl - 1
    p = f"smis.{k}."
    cp = p + "content_unit."
    f_m = seams["fm"] if k == 0 else seams[f"mu{k - 1}"]
    f_c = seams["fc"] if k == 0 else seams[f"cu{k - 1}"]
    bu, fs, fw = seams[f"bu{k}"], seams["fs"], seams["fw"]
    B, L, _, C, D = f_c.shape
    dl = sd[cp + "linear_c_hat.weight"].shape[0]
    m = batch["moment_mask"].float()[:, :, :, None, None]
    qm = batch["query_mask"].float()
    c_hat = O._lin(sd, cp + "linear_c_hat", f_c) * m
    w_hat = O._lin(sd, cp + "linear_w_hat", fw) * qm
    s_hat = O._lin(sd, cp + "linear_s_hat", fs)
    att = O._word_attention(sd, cp + "attn_layer.", c_hat.reshape(B, L * L * C, dl), w_hat, w_hat, qm.reshape(B, 1, -1), dl).reshape(B, L, L, C, dl) * m
    q = c_hat * (att + s_hat[:, None, None, None, :])
    A = torch.softmax(q @ q.transpose(3, 4) / math.sqrt(dl), dim=-1) * m
    ccmean = (A @ c_hat).mean(dim=3)
    hbar = torch.sigmoid(f_m * fs[:, None, None, :]) * f_m
    b_idx, i_idx, j_idx = (t.reshape(-1) for t in torch.meshgrid(torch.arange(B), torch.arange(L), torch.arange(L), indexing="ij"))
    logit = score_tail_torch(ccmean.reshape(-1, dl), f_c.mean(dim=3).reshape(-1, D), hbar.reshape(-1, D), f_m.reshape(-1, D), bu, b_idx, i_idx, j_idx,
                             sd[cp + "linear_c.weight"], sd[cp + "linear_c.bias"], sd[p + "moment_unit.conv_layer_fb.weight"].reshape(D, D),
                             sd[p + "moment_unit.conv_layer_fc.weight"].reshape(D, D),
                             sd[p + "moment_unit.conv_layer_fb.bias"] + sd[p + "moment_unit.conv_layer_fc.bias"],
                             sd["localization.conv_layer_pm.weight"].reshape(D), sd["localization.conv_layer_pm.bias"])
    return torch.sigmoid(logit).reshape(B, L, L) * batch["moment_mask"].float()
