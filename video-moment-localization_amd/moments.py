"""Top-k moment retrieval with greedy temporal NMS: which moments of a video match the query, as clip indices or seconds.

Semantics (csrc/moments.hip, include/smin_hip.h), for each sample b:
  * candidates: the cells (i, j) with ``moment_mask[b, i, j] != 0``; masked cells are never returned (the reference's plain
    ``topk`` can pick a masked cell with score 0 -- that is why the NMS path of ``compute_ious`` is opt-in);
  * score = ``(pm[b,i,j] * sqrtf(ps[b,i])) * sqrtf(pe[b,j])`` in fp32, in this order (the formula of ``compute_ious``);
  * order: higher score first, ties -> lower flat index ``i*L + j``; a score of -0 counts as +0;
  * temporal IoU of two cells in clip units (moment (i, j) spans [i, j+1), as dataset.get_iou defines it):
    ``inter = max(0, min(j1, j2) + 1 - max(i1, i2))``, ``union = max(j1, j2) + 1 - min(i1, i2)``,
    ``iou = (float)inter / (float)union`` (one correctly rounded fp32 division);
  * greedy NMS: walk the candidates in order; keep one unless its IoU with an already kept cell is > ``nms_thresh``
    (converted to fp32 once); stop after k kept or when the candidates run out.  ``nms_thresh >= 1``: no suppression,
    i.e. plain top-k over the valid cells;
  * empty slots: index -1 and score 0; ``count[b]`` = number kept;
  * limits: 1 <= k <= 64, 1 <= B <= 65535 (the band select puts the sample in the grid's second dimension; larger batches go
    through in chunks, as retrieval's ``max_batch`` does), L >= 1 with L*L < 2**31.

``top_moments`` is the product entry point (HIP kernels, HIP tensors only, no host synchronisation, capturable in a graph);
``top_moments_torch`` is the same function as plain torch + Python on any device, kept under its own name as the restatement
the tests compare against -- nothing routes to it silently.

``nms="linear"`` / ``"gaussian"`` replace the greedy walk by Soft-NMS (csrc/soft_nms.hip; ``soft_rule`` states the rules): a pick
decays the scores of the candidates it overlaps and the rest is ranked again.  ``top_moments_soft_torch`` is its restatement."""
import ctypes
import functools

import numpy as np
import torch

from ._host import _require_hip, byte_mask, host_array, require_ints
from ._lib import call, call_ws, load, ptr, stream

MAX_K = 64
MAX_B = 65535                       # csrc/moments.hip: the sample index is the band select's grid y coordinate
MAX_N, MAX_M = 64, 16               # compute_ious(..., nms_thresh=t): at most 64 values of n and 16 thresholds m


def _check(pm, ps, pe, moment_mask, k):
    if pm.dim() != 3 or pm.shape[1] != pm.shape[2]:
        raise ValueError(f"pm must be (B, L, L), got {tuple(pm.shape)}")
    B, L = pm.shape[0], pm.shape[1]
    if tuple(ps.shape) != (B, L) or tuple(pe.shape) != (B, L) or tuple(moment_mask.shape) != (B, L, L):
        raise ValueError(f"ps / pe must be (B, L) = {(B, L)} and moment_mask (B, L, L); got {tuple(ps.shape)}, {tuple(pe.shape)}, "
                         f"{tuple(moment_mask.shape)}")
    if not 1 <= B <= MAX_B or L < 1 or L * L >= 2 ** 31:
        raise ValueError(f"top_moments needs 1 <= B <= {MAX_B} and 1 <= L with L*L < 2**31 (B={B}, L={L})")
    if not (isinstance(k, int) and 1 <= k <= MAX_K):
        raise ValueError(f"top_moments needs an integer 1 <= k <= {MAX_K} (got {k!r})")
    return B, L


def _times(idx, duration, L):
    """(B, k, 2) seconds (i * duration / L, (j + 1) * duration / L) in fp32, NaN for empty slots (dataset.get_iou's clip units)."""
    d = duration.to(device=idx.device, dtype=torch.float32).reshape(-1, 1, 1)
    edge = idx.to(torch.float32) + torch.tensor([0.0, 1.0], device=idx.device)
    t = edge * d / L
    return torch.where(idx >= 0, t, torch.full_like(t, float("nan")))


def _result(idx, score, count, duration, L):
    out = {"idx": idx, "score": score, "count": count}
    if duration is not None:
        out["times"] = _times(idx, duration, L)
    return out


def _select_into(pm, ps, pe, moment_mask, k, nms_thresh, rule, idx, score, count, raw=None):
    """The selection of B checked samples on ``pm``'s device into the caller's contiguous ``idx (B, k, 2)`` int64, ``score (B, k)``
    float32 and ``count (B,)`` int32 (e.g. a chunk's rows of larger buffers): the workspace query, its allocation and the call.
    ``rule=None``: smin_top_moments at ``nms_thresh``; else ``soft_rule``'s tuple: smin_top_moments_soft, which also fills ``raw (B, k)``.
    Detached fp32 contiguous scores and a contiguous byte mask are passed as they are: no launch or copy beside the kernels'."""
    B, L = pm.shape[0], pm.shape[1]
    pm_, ps_, pe_ = (x.detach().float().contiguous() for x in (pm, ps, pe))
    mm_ = byte_mask(moment_mask)
    name, how, extra = ("smin_top_moments", (float(nms_thresh),), ()) if rule is None else ("smin_top_moments_soft", rule, (ptr(raw),))
    with torch.cuda.device(pm.device):
        call_ws(name, (B, L, k), stream(), ptr(pm_), ptr(ps_), ptr(pe_), ptr(mm_), B, L, k, *how, ptr(idx), ptr(score), *extra, ptr(count), fields="B, L, k")


def top_moments(pm, ps, pe, moment_mask, k=5, nms_thresh=0.5, duration=None, nms="hard", sigma=0.5, min_score=None):
    """The k best moments of each sample after greedy temporal NMS (module docstring), on the device: a band-parallel select
    and one NMS workgroup per sample (csrc/moments.hip).  HIP tensors only; no host synchronisation.

    Returns a dict: ``idx`` (B, k, 2) int64 start / end clip (-1 for empty slots), ``score`` (B, k) float32 (0 for empty
    slots), ``count`` (B,) int32; with ``duration`` (B,) seconds also ``times`` (B, k, 2) float32:
    ``(i * duration / L, (j + 1) * duration / L)``, NaN for empty slots.

    ``nms="linear"`` / ``"gaussian"`` select Soft-NMS (csrc/soft_nms.hip; the rules are stated at ``soft_rule``): a pick decays the
    score of the candidates it overlaps and the rest is ranked again.  ``score`` is then the decayed score at pick time and the dict
    gains ``raw_score (B, k)``, the picked cells' undecayed scores (0 for empty slots); ``min_score`` ends a sample's list at the first
    best decayed score below it (``None``: never).  ``nms="hard"`` (default) is the path above, unchanged; it reads neither ``sigma``
    nor ``min_score``."""
    _require_hip(pm, "top_moments")
    B, L = _check(pm, ps, pe, moment_mask, k)
    rule = soft_rule("top_moments", nms, nms_thresh, sigma, min_score)
    idx = torch.empty((B, k, 2), dtype=torch.int64, device=pm.device)
    score = torch.empty((B, k), dtype=torch.float32, device=pm.device)
    count = torch.empty((B,), dtype=torch.int32, device=pm.device)
    raw = None if rule is None else torch.empty((B, k), dtype=torch.float32, device=pm.device)
    _select_into(pm, ps, pe, moment_mask, k, nms_thresh, rule, idx, score, count, raw)
    out = _result(idx, score, count, duration, L)
    if rule is not None:
        out["raw_score"] = raw
    return out


# ---------------------------------------------------------------- Soft-NMS (csrc/soft_nms.hip)
NMS_METHODS = {"linear": 1, "gaussian": 2}          # include/smin_hip.h SMIN_NMS_LINEAR / SMIN_NMS_GAUSSIAN


def soft_rule(what, nms, nms_thresh, sigma, min_score):
    """``None`` for ``nms="hard"``, else the checked soft rule ``(method, nms_thresh, sigma, min_score)`` as the C ABI takes it.

    Per sample, with ``cur = score`` initially: pick the remaining candidate with the highest ``cur`` (ties -> lower index); stop
    after k picks, when none is left or when the best ``cur < min_score`` (fp32; ``None`` = -inf); record it; then for every remaining
    candidate ``cur = cur * w`` in fp32 with ``iou`` its IoU with the pick: ``"linear"``: ``w = 1 - iou if iou > nms_thresh else 1``;
    ``"gaussian"``: ``w = expf(-(iou * iou) / sigma)`` for every candidate (``sigma > 0``, ``inf`` allowed: ``w = 1``).  NaN and inf
    scores at valid cells are out of scope for the soft rules."""
    if nms == "hard":
        return None
    if nms not in NMS_METHODS:
        raise ValueError(f"{what}: nms must be 'hard', 'linear' or 'gaussian' (got {nms!r})")
    sigma = float(sigma)
    if nms == "gaussian" and not sigma > 0:
        raise ValueError(f"{what}: nms='gaussian' needs sigma > 0 (got {sigma!r})")
    floor = float("-inf") if min_score is None else float(min_score)
    if floor != floor:
        raise ValueError(f"{what}: min_score must not be NaN")
    return NMS_METHODS[nms], float(nms_thresh), sigma, floor


def _f32(x, dev):
    return torch.tensor(x, dtype=torch.float32, device=dev)


def _decay_torch(cur, iou, rule, dev):
    """One decay of fp32 ``cur`` by fp32 ``iou``.  linear: correctly rounded fp32 operations (bit for bit the kernel's); gaussian: the
    weight and the product in fp64, returned as fp64 (the kernel's expf is checked against it, not reproduced)."""
    method, thr, sigma, _ = rule
    if method == NMS_METHODS["linear"]:
        w = torch.where(iou > _f32(thr, dev), (1.0 - iou.double()).float(), torch.ones_like(iou))   # 1 - iou: one rounding
        return _mul32(cur, w)
    x = iou.double()
    return cur * torch.exp(-(x * x) / sigma)


def _soft_pick_loop(s0, valid, iou_with, k, rule, dev):
    """The soft rule over one sample's candidates: ``s0`` (n,) fp32 start scores, ``valid`` (n,) bool, ``iou_with(c)`` -> (n,) fp32
    IoUs with candidate c.  Returns the picks' candidate indices and their ``cur`` at pick time (fp32 for linear, fp64 for
    gaussian)."""
    gauss = rule[0] == NMS_METHODS["gaussian"]
    cur = s0.double() if gauss else s0.clone()
    alive = valid.clone()
    picks, vals = [], []
    floor = _f32(rule[3], dev)
    for _ in range(k):
        if not bool(alive.any()):
            break
        o = _order_word(cur.float())
        o = torch.where(alive, o, torch.zeros_like(o))
        c = int(torch.argmax((o == o.max()).to(torch.uint8)))                # the first index holding the maximum
        if bool(cur[c].float() < floor):
            break
        picks.append(c)
        vals.append(cur[c].clone())
        alive[c] = False
        cur = torch.where(alive, _decay_torch(cur, iou_with(c), rule, dev), cur)
    return picks, vals


def top_moments_soft_torch(pm, ps, pe, moment_mask, k=5, nms_thresh=0.5, duration=None, nms="linear", sigma=0.5, min_score=None):
    """Soft ``top_moments`` as plain torch + Python on any device.  ``nms="linear"`` gives the kernels' result bit for bit (every
    operation is a correctly rounded fp32 one); ``nms="gaussian"`` carries the decayed scores in fp64 (exact exp, unrounded
    products) and rounds the recorded ``score`` to fp32 once -- the reference the device's expf is measured against."""
    B, L = _check(pm, ps, pe, moment_mask, k)
    rule = soft_rule("top_moments_soft_torch", nms, nms_thresh, sigma, min_score)
    if rule is None:
        raise ValueError("top_moments_soft_torch restates the soft rules; nms='hard' is top_moments_torch")
    dev = pm.device
    score, valid = _score_map(pm, ps, pe, moment_mask)
    cells = torch.arange(L * L, device=dev)
    ci, cj = cells // L, cells % L
    idx = torch.full((B, k, 2), -1, dtype=torch.int64, device=dev)
    out_score = torch.zeros((B, k), dtype=torch.float32, device=dev)
    raw = torch.zeros((B, k), dtype=torch.float32, device=dev)
    count = torch.zeros((B,), dtype=torch.int32, device=dev)
    for b in range(B):
        picks, vals = _soft_pick_loop(score[b], valid[b], lambda c: _iou(ci, cj, ci[c], cj[c]), k, rule, dev)
        n = len(picks)
        if n:
            pc = torch.tensor(picks, dtype=torch.int64, device=dev)
            idx[b, :n, 0], idx[b, :n, 1] = pc // L, pc % L
            v = torch.stack(vals).float()
            out_score[b, :n] = torch.where(v == 0, torch.zeros_like(v), v)
            raw[b, :n] = score[b, pc]
        count[b] = n
    out = _result(idx, out_score, count, duration, L)
    out["raw_score"] = raw
    return out


# Correctly rounded fp32 sqrt / product / quotient on any device: computed in fp64 and rounded once to fp32 (fp64 carries more than
# 2 * 24 + 2 bits, so the double rounding is exact for these three operations).  torch's own fp32 sqrt is not correctly rounded
# on every CPU code path.
def _sqrt32(x):
    return torch.sqrt(x.float().double()).float()


def _mul32(a, b):
    return (a.float().double() * b.float().double()).float()


def _fused(pm, ps, pe):
    """(B, L, L) fp32 fused score of every cell: ``(pm * sqrtf(ps_i)) * sqrtf(pe_j)``, each operation rounded once."""
    return _mul32(_mul32(pm.detach(), _sqrt32(ps.detach()).unsqueeze(2)), _sqrt32(pe.detach()).unsqueeze(1))


def _score_map(pm, ps, pe, moment_mask):
    """``(score, valid)``, both (B, L*L): the fused score with -0 as +0 and 0 at the masked cells (their NaN / inf never enter), and the
    bool mask of the valid cells."""
    score = _fused(pm, ps, pe)
    score = torch.where(score == 0, torch.zeros_like(score), score).reshape(pm.shape[0], -1)     # -0 -> +0
    valid = byte_mask(moment_mask).reshape(pm.shape[0], -1) != 0
    return torch.where(valid, score, torch.zeros_like(score)), valid


def _order_word(score):
    """fp32 scores as int64 words in the kernels' order: a higher score has the higher word, -0 counts as +0, and no word is below 1
    (0 stands for "no candidate")."""
    score = torch.where(score == 0, torch.zeros_like(score), score)                             # -0 -> +0
    u = score.contiguous().view(torch.int32).to(torch.int64) & 0xFFFFFFFF                        # fp32 bits -> unsigned order word
    return torch.where(u >= 0x80000000, u ^ 0xFFFFFFFF, u | 0x80000000).clamp_min(1)


def _iou(i1, j1, i2, j2):
    inter = (torch.minimum(j1, j2) + 1 - torch.maximum(i1, i2)).clamp_min(0)
    union = torch.maximum(j1, j2) + 1 - torch.minimum(i1, i2)
    return (inter.to(torch.float32).double() / union.to(torch.float32).double()).float()


def top_moments_torch(pm, ps, pe, moment_mask, k=5, nms_thresh=0.5, duration=None, chunk=256):
    """``top_moments`` as plain torch + Python on any device (same result, bit for bit): the candidates sorted by (score, index),
    then greedy NMS, testing ``chunk`` candidates at a time against the kept set."""
    B, L = _check(pm, ps, pe, moment_mask, k)
    dev = pm.device
    score, valid = _score_map(pm, ps, pe, moment_mask)
    o = torch.where(valid, _order_word(score), torch.zeros_like(score, dtype=torch.int64))
    order = torch.sort(o, dim=1, descending=True, stable=True).indices                          # ties keep index order
    nvalid = valid.sum(dim=1).tolist()
    thr = torch.tensor(float(nms_thresh), dtype=torch.float32, device=dev)
    idx = torch.full((B, k, 2), -1, dtype=torch.int64, device=dev)
    out_score = torch.zeros((B, k), dtype=torch.float32, device=dev)
    count = torch.zeros((B,), dtype=torch.int32, device=dev)
    for b in range(B):
        cand = order[b, :nvalid[b]]
        ki = torch.empty(0, dtype=torch.int64, device=dev)
        kj = torch.empty(0, dtype=torch.int64, device=dev)
        kc = []
        for s in range(0, cand.numel(), chunk):
            if len(kc) >= k:
                break
            c = cand[s:s + chunk]
            ci, cj = c // L, c % L
            if len(kc):
                sup = (_iou(ci.unsqueeze(1), cj.unsqueeze(1), ki.unsqueeze(0), kj.unsqueeze(0)) > thr).any(dim=1)
            else:
                sup = torch.zeros_like(c, dtype=torch.bool)
            n0 = len(kc)
            for q in (~sup).nonzero().flatten().tolist():
                if len(kc) >= k:
                    break
                if len(kc) > n0 and bool((_iou(ci[q], cj[q], ki[n0:], kj[n0:]) > thr).any()):
                    continue                                                                     # suppressed inside the chunk
                ki, kj = torch.cat([ki, ci[q:q + 1]]), torch.cat([kj, cj[q:q + 1]])
                kc.append(int(c[q]))
        n = len(kc)
        if n:
            idx[b, :n, 0], idx[b, :n, 1] = ki, kj
            out_score[b, :n] = score[b, torch.tensor(kc, dtype=torch.int64, device=dev)]
        count[b] = n
    return _result(idx, out_score, count, duration, L)


def _nm_check(n, m):
    n, m = [int(x) for x in n], [float(x) for x in m]
    if not (1 <= len(n) <= MAX_N and 1 <= len(m) <= MAX_M and min(n) >= 1 and max(n) <= MAX_K):
        raise ValueError(f"compute_ious with nms_thresh: needs 1..{MAX_N} values 1 <= n <= {MAX_K} and 1..{MAX_M} thresholds m "
                         f"(got n={n}, m={m})")
    return n, m


def compute_ious_nms(pm, ps, pe, moment_mask, sm, n, m, nms_thresh, nms="hard", sigma=0.5):
    """R@n, IoU=m over the NMS-kept moments on the device (training.compute_ious(..., nms_thresh=t)): top-k with k = max(n), then
    sm gathered at the kept cells (empty slot = IoU 0) and the hits summed over the samples by the device.  One host read."""
    B, L = _check(pm, ps, pe, moment_mask, 1)
    keys = [f"R@{n_}, IoU={m_}" for n_ in n for m_ in m]
    n, m = _nm_check(n, m)
    k = max(n)
    pm_, ps_, pe_, sm_ = (x.detach().float().contiguous() for x in (pm, ps, pe, sm))
    mm_ = byte_mask(moment_mask)
    nl, ml = (ctypes.c_int * len(n))(*n), (ctypes.c_float * len(m))(*m)
    counts = torch.empty((len(n) * len(m),), dtype=torch.float32, device=pm.device)
    rule = soft_rule("compute_ious", nms, nms_thresh, sigma, None)
    # a soft rule puts its selection in front of the same hit flags and sums
    name, how = ("smin_compute_ious_nms", (float(nms_thresh),)) if rule is None else ("smin_compute_ious_soft", rule[:3])
    with torch.cuda.device(pm.device):
        call_ws(name, (B, L, k, len(n), len(m)), stream(), ptr(pm_), ptr(ps_), ptr(pe_), ptr(mm_), ptr(sm_), B, L, k, *how,
                ctypes.cast(nl, ctypes.c_void_p), len(n), ctypes.cast(ml, ctypes.c_void_p), len(m), ptr(counts), fields="B, L, k, nn, nm")
    return dict(zip(keys, counts.tolist()))


def compute_ious_nms_torch(pm, ps, pe, moment_mask, sm, n, m, nms_thresh, nms="hard", sigma=0.5):
    """``compute_ious_nms`` through ``top_moments_torch`` (any device)."""
    B, L = _check(pm, ps, pe, moment_mask, 1)
    keys = [f"R@{n_}, IoU={m_}" for n_ in n for m_ in m]
    n, m = _nm_check(n, m)
    if nms == "hard":
        r = top_moments_torch(pm, ps, pe, moment_mask, k=max(n), nms_thresh=nms_thresh)
    else:
        r = top_moments_soft_torch(pm, ps, pe, moment_mask, k=max(n), nms_thresh=nms_thresh, nms=nms, sigma=sigma)
    flat = r["idx"][..., 0] * L + r["idx"][..., 1]
    ious = torch.gather(sm.detach().float().reshape(B, -1), 1, flat.clamp_min(0))
    ious = torch.where(flat >= 0, ious, torch.zeros_like(ious))
    counts = torch.stack([((ious[:, :n_] > m_).sum(dim=1) > 0).sum() for n_ in n for m_ in m]).tolist()
    return {k_: float(v) for k_, v in zip(keys, counts)}


# ---------------------------------------------------------------- merge across the windows of long videos (SMIN.localize_windows)
def _merge_check(idx, score, count, start, lens, pair_ptr, T, L, k):
    if idx.dim() != 3 or idx.shape[2] != 2:
        raise ValueError(f"merge_window_moments: idx must be (G, k_window, 2), got {tuple(idx.shape)}")
    G, kw = idx.shape[0], idx.shape[1]
    if tuple(score.shape) != (G, kw) or tuple(count.shape) != (G,) or tuple(start.shape) != (G,) or tuple(lens.shape) != (G,):
        raise ValueError(f"merge_window_moments: score must be (G, k_window) = {(G, kw)}, count / start / lens (G,); got "
                         f"{tuple(score.shape)}, {tuple(count.shape)}, {tuple(start.shape)}, {tuple(lens.shape)}")
    if pair_ptr.dim() != 1 or pair_ptr.shape[0] < 1:
        raise ValueError("merge_window_moments: pair_ptr must be (B + 1,)")
    if not (isinstance(k, int) and 1 <= k <= MAX_K) or not 1 <= kw <= MAX_K:
        raise ValueError(f"merge_window_moments needs integers 1 <= k, k_window <= {MAX_K} (got k={k!r}, k_window={kw})")
    if int(T) < 1 or int(L) < 1 or G * kw >= 2 ** 31:
        raise ValueError(f"merge_window_moments needs T >= 1, L >= 1 and G * k_window < 2**31 (T={T}, L={L}, G={G}, k_window={kw})")
    return G, kw, pair_ptr.shape[0] - 1


def _merge_result(span, score, raw, window, cell, count):
    """merge_window_moments' dict; ``raw_score`` (soft rules only) sits behind ``score``."""
    out = {"span": span, "score": score}
    if raw is not None:
        out["raw_score"] = raw
    out.update(window=window, cell=cell, count=count)
    return out


def merge_window_moments(idx, score, count, start, lens, pair_ptr, T, L, k=5, nms_thresh=0.5, nms="hard", sigma=0.5, min_score=None):
    """Greedy temporal NMS, in raw-row time, of the per-window top moments of long videos (include/smin_hip.h,
    smin_merge_window_moments): one workgroup per (video, query) pair picks k times the best candidate that no kept span suppresses.

    ``idx (G, k_window, 2)`` int64, ``score (G, k_window)``, ``count (G,)``: top_moments' outputs for G windows; ``start (G,)`` each
    window's first row relative to its video, ``lens (G,)`` its row count; ``pair_ptr (B + 1,)``: pair b owns windows
    ``pair_ptr[b] .. pair_ptr[b + 1]``.  HIP tensors only; no host synchronisation.  Returns a dict: ``span (B, k, 2)`` float32 raw
    rows (NaN for empty slots), ``score (B, k)`` (0), ``window (B, k)`` int64 ordinal within the pair (-1), ``cell (B, k, 2)`` int64
    (-1), ``count (B,)`` int32.

    ``nms="linear"`` / ``"gaussian"``: the soft rule of ``soft_rule`` over the same candidates, spans and span IoU
    (smin_merge_window_moments_soft).  ``score`` must then hold the windows' UNDECAYED scores (soft ``top_moments``' ``raw_score``):
    the merge decays once, in raw-row time.  The result's ``score`` is the decayed score at pick time and ``raw_score (B, k)`` the
    candidate's input score."""
    _require_hip(idx, "merge_window_moments")
    G, kw, B = _merge_check(idx, score, count, start, lens, pair_ptr, T, L, k)
    rule = soft_rule("merge_window_moments", nms, nms_thresh, sigma, min_score)
    dev = idx.device
    args = [idx.to(torch.int64), score.detach().float(), count.to(torch.int32), start.to(torch.int64), lens.to(torch.int32),
            pair_ptr.to(torch.int64)]
    args = [a.contiguous() for a in args]
    span = torch.empty((B, k, 2), dtype=torch.float32, device=dev)
    out_score = torch.empty((B, k), dtype=torch.float32, device=dev)
    window = torch.empty((B, k), dtype=torch.int64, device=dev)
    cell = torch.empty((B, k, 2), dtype=torch.int64, device=dev)
    out_count = torch.empty((B,), dtype=torch.int32, device=dev)
    raw = None
    name, how, extra = "smin_merge_window_moments", (float(nms_thresh),), ()
    if rule is not None:
        raw = torch.empty((B, k), dtype=torch.float32, device=dev)
        name, how, extra = "smin_merge_window_moments_soft", rule, (ptr(raw),)
    with torch.cuda.device(dev):
        call(name, stream(), *[ptr(a) for a in args], G, B, int(T), int(L), kw, k, *how, ptr(span), ptr(out_score), *extra,
             ptr(window), ptr(cell), ptr(out_count))
    return _merge_result(span, out_score, raw, window, cell, out_count)


def _div32(a, b):
    return (a.float().double() / b.float().double()).float()


def _add32(a, b):
    return (a.float().double() + b.float().double()).float()


def window_spans(cell, start, lens, T, L):
    """Spans in raw rows of cells (i, j) (..., 2) of windows (start, lens) (...,), fp32 in the order of include/smin_hip.h."""
    s = start.to(torch.int64)
    n = lens.to(torch.int64)
    u = _div32(torch.clamp_min(n, int(T)).to(torch.float32), torch.full_like(n, int(L), dtype=torch.float32))
    sf = s.to(torch.float32)
    st = _add32(sf, _mul32(cell[..., 0].to(torch.float32), u))
    en = torch.minimum(_add32(sf, _mul32((cell[..., 1] + 1).to(torch.float32), u)), (s + n).to(torch.float32))
    return st, en


def _span_iou(st1, en1, st2, en2):
    inter = (torch.minimum(en1, en2) - torch.maximum(st1, st2)).clamp_min(0)
    uni = torch.maximum(en1, en2) - torch.minimum(st1, st2)
    return _div32(inter, uni)


def merge_window_moments_torch(idx, score, count, start, lens, pair_ptr, T, L, k=5, nms_thresh=0.5, nms="hard", sigma=0.5, min_score=None):
    """``merge_window_moments`` as plain torch + Python on any device (same result, bit for bit): each pair's candidates sorted by
    (score, window, slot), then the greedy walk.  With a soft ``nms``: the pick-and-decay loop of ``top_moments_soft_torch`` over the
    pair's candidates and their span IoUs (linear bit for bit, gaussian in fp64)."""
    G, kw, B = _merge_check(idx, score, count, start, lens, pair_ptr, T, L, k)
    rule = soft_rule("merge_window_moments_torch", nms, nms_thresh, sigma, min_score)
    dev = idx.device
    score = score.detach().float().reshape(-1)
    st_all, en_all = window_spans(idx, start.unsqueeze(1), lens.unsqueeze(1), T, L)              # (G, kw)
    st_all, en_all = st_all.reshape(-1), en_all.reshape(-1)
    slot_ok = (torch.arange(kw, device=dev).unsqueeze(0) < count.to(torch.int64).unsqueeze(1)).reshape(-1)
    thr = _f32(float(nms_thresh), dev)
    span = torch.full((B, k, 2), float("nan"), dtype=torch.float32, device=dev)
    out_score = torch.zeros((B, k), dtype=torch.float32, device=dev)
    raw = None if rule is None else torch.zeros((B, k), dtype=torch.float32, device=dev)
    window = torch.full((B, k), -1, dtype=torch.int64, device=dev)
    cell = torch.full((B, k, 2), -1, dtype=torch.int64, device=dev)
    out_count = torch.zeros((B,), dtype=torch.int32, device=dev)
    pp = pair_ptr.to(torch.int64).tolist()
    for b in range(B):
        g0 = min(max(pp[b], 0), G)
        g1 = min(max(pp[b + 1], g0), G)
        q = torch.arange(g0 * kw, g1 * kw, device=dev)                                             # candidates in (window, slot) order
        if rule is None:
            cand = q[slot_ok[q]]
            order = torch.sort(_order_word(score[cand]), descending=True, stable=True).indices     # ties keep (window, slot) order
            kept = []
            for c in cand[order].tolist():
                if len(kept) >= k:
                    break
                if kept:
                    ks = torch.tensor(kept, dtype=torch.int64, device=dev)
                    if bool((_span_iou(st_all[c], en_all[c], st_all[ks], en_all[ks]) > thr).any()):
                        continue
                kept.append(c)
            ks = torch.tensor(kept, dtype=torch.int64, device=dev)
            vals = list(score[ks])
        else:
            st, en = st_all[q], en_all[q]
            picks, vals = _soft_pick_loop(score[q], slot_ok[q], lambda c: _span_iou(st, en, st[c], en[c]), k, rule, dev)
            ks = q[torch.tensor(picks, dtype=torch.int64, device=dev)]
        n = len(vals)
        if n:
            span[b, :n, 0], span[b, :n, 1] = st_all[ks], en_all[ks]
            out_score[b, :n] = torch.stack(vals).float()
            if raw is not None:
                raw[b, :n] = score[ks]
            window[b, :n] = ks // kw - g0
            cell[b, :n] = idx.reshape(-1, 2)[ks].to(torch.int64)
        out_count[b] = n
    return _merge_result(span, out_score, raw, window, cell, out_count)


# ---------------------------------------------------------------- metric of merged spans against ground-truth spans
def _span_check(span, count, gt):
    if span.dim() != 3 or span.shape[2] != 2:
        raise ValueError(f"span must be (B, k, 2), got {tuple(span.shape)}")
    B, k = span.shape[0], span.shape[1]
    if tuple(count.shape) != (B,) or tuple(gt.shape) != (B, 2):
        raise ValueError(f"count must be (B,) = {(B,)} and gt (B, 2) = {(B, 2)}; got {tuple(count.shape)}, {tuple(gt.shape)}")
    if not 1 <= k <= MAX_K:
        raise ValueError(f"the span metric takes 1 <= k <= {MAX_K} slots per pair (got k = {k})")
    return B, k


def _span_nm_check(n, m, k):
    keys = [f"R@{n_}, IoU={m_}" for n_ in n for m_ in m]
    n, m = _nm_check(n, m)
    if max(n) > k:
        raise ValueError(f"R@{max(n)} needs at least {max(n)} slots per pair (span has k = {k})")
    return keys, n, m


def span_ious(span, count, gt):
    """IoU of every slot of ``span (B, k, 2)`` (``merge_window_moments`` / ``SMIN.localize_windows`` output, ``count (B,)`` filled
    slots) with the pair's ground truth ``gt (B, 2)`` in the same unit, on the device (include/smin_hip.h, smin_span_ious):
    ``(B, k)`` float32, exactly 0 for the empty slots (their NaN span does not propagate).  HIP tensors only; no host read."""
    _require_hip(span, "span_ious")
    B, k = _span_check(span, count, gt)
    span_, gt_, count_ = span.detach().float().contiguous(), gt.detach().float().contiguous(), count.to(torch.int32).contiguous()
    iou = torch.empty((B, k), dtype=torch.float32, device=span.device)
    with torch.cuda.device(span.device):
        call("smin_span_ious", stream(), ptr(span_), ptr(count_), ptr(gt_), B, k, ptr(iou))
    return iou


def _valid_slots(count, k):
    """(B, k) bool: slot s < count[b], the count clamped to [0, k] as the kernels read it."""
    return torch.arange(k, device=count.device).unsqueeze(0) < count.to(torch.int64).clamp(0, k).unsqueeze(1)


def span_ious_torch(span, count, gt):
    """``span_ious`` as plain torch on any device (same result, bit for bit): fminf / fmaxf as ``torch.fmin`` / ``torch.fmax``, the
    fp32 differences as torch forms them (IEEE), the division rounded once."""
    B, k = _span_check(span, count, gt)
    span, gt = span.detach().float(), gt.detach().float()
    st, en = span[..., 0], span[..., 1]
    gs, ge = gt[:, 0:1], gt[:, 1:2]
    inter = torch.fmax(torch.fmin(en, ge) - torch.fmax(st, gs), torch.zeros_like(st))
    uni = torch.fmax(en, ge) - torch.fmin(st, gs)
    pos = uni > 0
    iou = torch.where(pos, _div32(inter, torch.where(pos, uni, torch.ones_like(uni))), torch.zeros_like(uni))
    return torch.where(_valid_slots(count, k), iou, torch.zeros_like(iou))


def _span_meter_call(span, count, gt, n, m, acc):
    """smin_span_meter_update of B >= 1 checked pairs into ``acc`` (fp64, 4 + len(n) * len(m)) on the current stream."""
    B, k = span.shape[0], span.shape[1]
    span_, gt_, count_ = span.detach().float().contiguous(), gt.detach().float().contiguous(), count.to(torch.int32).contiguous()
    nl, ml = (ctypes.c_int * len(n))(*n), (ctypes.c_float * len(m))(*m)
    with torch.cuda.device(span.device):
        call_ws("smin_span_meter_update", (B, len(n), len(m)), stream(), ptr(span_), ptr(count_), ptr(gt_), B, k, ctypes.cast(nl, ctypes.c_void_p),
                len(n), ctypes.cast(ml, ctypes.c_void_p), len(m), ptr(acc), query="smin_span_meter_ws_bytes", fields="B, nn, nm")


def compute_span_ious(span, count, gt, n=(1, 5), m=(0.1, 0.3, 0.5, 0.7)):
    """R@n, IoU=m of merged spans on the device, mirroring ``compute_ious``: ``{"R@n, IoU=m": pairs with some slot
    s < min(n, count) whose IoU with gt is > m}`` (strict, as utils.py:29), summed over the pairs by the device
    (smin_span_meter_update into a fresh accumulator).  One host read.  HIP tensors only."""
    _require_hip(span, "compute_span_ious")
    B, k = _span_check(span, count, gt)
    keys, n, m = _span_nm_check(n, m, k)
    acc = torch.zeros((4 + len(keys),), dtype=torch.float64, device=span.device)
    if B:
        _span_meter_call(span, count, gt, n, m, acc)
    return dict(zip(keys, acc[4:].tolist()))


def _span_hits_torch(ious, count, n, m):
    """(len(n) * len(m),) int64: pairs with a hit for each (n, m), thresholds converted to fp32 once."""
    valid = _valid_slots(count, ious.shape[1])
    thr = torch.tensor(m, dtype=torch.float32, device=ious.device)
    return torch.stack([((ious[:, :n_] > thr[c]) & valid[:, :n_]).any(dim=1).sum() for n_ in n for c in range(len(m))])


def compute_span_ious_torch(span, count, gt, n=(1, 5), m=(0.1, 0.3, 0.5, 0.7)):
    """``compute_span_ious`` through ``span_ious_torch`` (any device)."""
    B, k = _span_check(span, count, gt)
    keys, n, m = _span_nm_check(n, m, k)
    counts = _span_hits_torch(span_ious_torch(span, count, gt), count, n, m).tolist()
    return {k_: float(v) for k_, v in zip(keys, counts)}


# ---------------------------------------------------------------- merge across the videos of a corpus (SMIN.search)
def _corpus_check(pair_score, pair_idx, pair_count, pair_video, pair_ptr, k):
    if pair_idx.dim() != 3 or pair_idx.shape[2] != 2:
        raise ValueError(f"corpus_topk: pair_idx must be (P, k_video, 2), got {tuple(pair_idx.shape)}")
    P, kv = pair_idx.shape[0], pair_idx.shape[1]
    if tuple(pair_score.shape) != (P, kv) or tuple(pair_count.shape) != (P,) or tuple(pair_video.shape) != (P,):
        raise ValueError(f"corpus_topk: pair_score must be (P, k_video) = {(P, kv)}, pair_count / pair_video (P,); got "
                         f"{tuple(pair_score.shape)}, {tuple(pair_count.shape)}, {tuple(pair_video.shape)}")
    if pair_ptr.dim() != 1 or pair_ptr.shape[0] < 1:
        raise ValueError("corpus_topk: pair_ptr must be (Q + 1,)")
    if not (isinstance(k, int) and 1 <= k <= MAX_K) or not 1 <= kv <= MAX_K:
        raise ValueError(f"corpus_topk needs integers 1 <= k, k_video <= {MAX_K} (got k={k!r}, k_video={kv})")
    if P >= 2 ** 31:
        raise ValueError(f"corpus_topk: {P} pairs exceed the int32 pair_ptr")
    return P, kv, pair_ptr.shape[0] - 1


def corpus_topk(pair_score, pair_idx, pair_count, pair_video, pair_ptr, k=5):
    """One ranked list per query over all of its videos (include/smin_hip.h, smin_corpus_topk): one workgroup per query picks k
    times the best remaining candidate of the query's pairs.

    ``pair_score (P, k_video)``, ``pair_idx (P, k_video, 2)`` int64, ``pair_count (P,)``: top_moments' outputs for P (video, query)
    pairs; ``pair_video (P,)`` each pair's video; ``pair_ptr (Q + 1,)``: query q owns pairs ``pair_ptr[q] .. pair_ptr[q + 1]``
    (ascending, within [0, P]).  Order: higher score first, ties -> lower video, then lower slot, then the earlier pair; -0 counts as
    +0.  HIP tensors only; no host synchronisation.  Returns a dict: ``video (Q, k)`` int64 (-1 for empty slots), ``idx (Q, k, 2)``
    int64 (-1), ``score (Q, k)`` float32 (0), ``count (Q,)`` int32."""
    _require_hip(pair_ptr, "corpus_topk")
    P, kv, Q = _corpus_check(pair_score, pair_idx, pair_count, pair_video, pair_ptr, k)
    dev = pair_ptr.device
    args = [pair_score.detach().float(), pair_idx.to(torch.int64), pair_count.to(torch.int32), pair_video.to(torch.int32), pair_ptr.to(torch.int32)]
    args = [a.contiguous() for a in args]
    video = torch.empty((Q, k), dtype=torch.int64, device=dev)
    idx = torch.empty((Q, k, 2), dtype=torch.int64, device=dev)
    score = torch.empty((Q, k), dtype=torch.float32, device=dev)
    count = torch.empty((Q,), dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        call("smin_corpus_topk", stream(), *[ptr(a) if a.numel() else None for a in args], Q, kv, k, ptr(video), ptr(idx), ptr(score), ptr(count))
    return {"video": video, "idx": idx, "score": score, "count": count}


def corpus_topk_torch(pair_score, pair_idx, pair_count, pair_video, pair_ptr, k=5):
    """``corpus_topk`` as plain torch + Python on any device (same result, bit for bit): each query's candidates sorted by
    (score, video, slot, pair)."""
    P, kv, Q = _corpus_check(pair_score, pair_idx, pair_count, pair_video, pair_ptr, k)
    dev = pair_ptr.device
    score = pair_score.detach().float()
    o = _order_word(score).reshape(-1).tolist()
    cnt = pair_count.to(torch.int64).clamp(max=kv).tolist()
    vid = pair_video.to(torch.int64).tolist()
    pp = pair_ptr.to(torch.int64).tolist()
    video = torch.full((Q, k), -1, dtype=torch.int64, device=dev)
    idx = torch.full((Q, k, 2), -1, dtype=torch.int64, device=dev)
    out_score = torch.zeros((Q, k), dtype=torch.float32, device=dev)
    count = torch.zeros((Q,), dtype=torch.int32, device=dev)
    for q in range(Q):
        g0 = max(pp[q], 0)
        g1 = max(pp[q + 1], g0)
        cand = [(-o[g * kv + s], vid[g], s, g) for g in range(g0, g1) for s in range(max(cnt[g], 0))]
        cand.sort()
        n = min(len(cand), k)
        if n:
            flat = torch.tensor([g * kv + s for _, _, s, g in cand[:n]], dtype=torch.int64, device=dev)
            video[q, :n] = torch.tensor([v for _, v, _, _ in cand[:n]], dtype=torch.int64, device=dev)
            idx[q, :n] = pair_idx.to(torch.int64).reshape(-1, 2)[flat]
            out_score[q, :n] = score.reshape(-1)[flat]
        count[q] = n
    return {"video": video, "idx": idx, "score": out_score, "count": count}


# ---------------------------------------------------------------- merge of span lists across videos (SMIN.search_windows)
def _corpus_span_check(what, span, score, window, cell, count, group_video, group_ptr, k):
    if span.dim() != 3 or span.shape[2] != 2:
        raise ValueError(f"{what}: span must be (G2, k_video, 2), got {tuple(span.shape)}")
    G2, kv = span.shape[0], span.shape[1]
    if tuple(score.shape) != (G2, kv) or tuple(window.shape) != (G2, kv) or tuple(cell.shape) != (G2, kv, 2) or tuple(count.shape) != (G2,) \
            or tuple(group_video.shape) != (G2,):
        raise ValueError(f"{what}: score and window must be (G2, k_video) = {(G2, kv)}, cell (G2, k_video, 2), count / group_video (G2,); got "
                         f"{tuple(score.shape)}, {tuple(window.shape)}, {tuple(cell.shape)}, {tuple(count.shape)}, {tuple(group_video.shape)}")
    if group_ptr.dim() != 1 or group_ptr.shape[0] < 1:
        raise ValueError(f"{what}: group_ptr must be (Q + 1,)")
    if not (isinstance(k, int) and 1 <= k <= MAX_K) or not 1 <= kv <= MAX_K:
        raise ValueError(f"{what} needs integers 1 <= k, k_video <= {MAX_K} (got k={k!r}, k_video={kv})")
    if G2 >= 2 ** 31:
        raise ValueError(f"{what}: {G2} groups exceed the int32 group_ptr")
    return G2, kv, group_ptr.shape[0] - 1


_SPAN_KEYS = ("video", "span", "score", "window", "cell", "count")


def corpus_span_topk(span, score, window, cell, count, group_video, group_ptr, k=5):
    """One ranked list of span-valued moments per query over all of its videos (include/smin_hip.h, smin_corpus_span_topk; the operator
    smin_hip::smin_corpus_span_topk): one workgroup per query picks k times the best remaining candidate of the query's groups.

    ``span (G2, k_video, 2)`` fp32, ``score (G2, k_video)``, ``window (G2, k_video)`` int64, ``cell (G2, k_video, 2)`` int64 and
    ``count (G2,)``: merge_window_moments' outputs for G2 (query, video) groups; ``group_video (G2,)`` each group's video;
    ``group_ptr (Q + 1,)``: query q owns groups ``group_ptr[q] .. group_ptr[q + 1]`` (ascending, within [0, G2]).  Order: corpus_topk's
    -- higher score first, ties -> lower video, then lower slot, then the earlier group; -0 counts as +0.  HIP tensors only; no host
    synchronisation.  Returns a dict: ``video (Q, k)`` int64 (-1 for empty slots), ``span (Q, k, 2)`` fp32 (NaN), ``score (Q, k)`` (0),
    ``window (Q, k)`` int64 (-1), ``cell (Q, k, 2)`` int64 (-1), ``count (Q,)`` int32; span, score, window and cell are copied bit
    for bit."""
    _require_hip(group_ptr, "corpus_span_topk")
    _corpus_span_check("corpus_span_topk", span, score, window, cell, count, group_video, group_ptr, k)
    from ._lib import load_torch
    out = load_torch().smin_corpus_span_topk(span.detach().float(), score.detach().float(), window.to(torch.int64), cell.to(torch.int64),
                                             count.to(torch.int32), group_video.to(torch.int32), group_ptr.to(torch.int32), k)
    return dict(zip(_SPAN_KEYS, out))


def corpus_span_topk_torch(span, score, window, cell, count, group_video, group_ptr, k=5):
    """``corpus_span_topk`` as plain torch + Python on any device (same result, bit for bit): each query's candidates sorted by
    (score, video, slot, group)."""
    G2, kv, Q = _corpus_span_check("corpus_span_topk_torch", span, score, window, cell, count, group_video, group_ptr, k)
    dev = group_ptr.device
    span, score = span.detach().float(), score.detach().float()
    o = _order_word(score).reshape(-1).tolist()
    cnt = count.to(torch.int64).clamp(0, kv).tolist()
    vid = group_video.to(torch.int64).tolist()
    gp = group_ptr.to(torch.int64).tolist()
    out = {"video": torch.full((Q, k), -1, dtype=torch.int64, device=dev),
           "span": torch.full((Q, k, 2), 0x7FC00000, dtype=torch.int32, device=dev).view(torch.float32),    # the kernel's NaN
           "score": torch.zeros((Q, k), dtype=torch.float32, device=dev),
           "window": torch.full((Q, k), -1, dtype=torch.int64, device=dev),
           "cell": torch.full((Q, k, 2), -1, dtype=torch.int64, device=dev),
           "count": torch.zeros((Q,), dtype=torch.int32, device=dev)}
    span_bits = span.contiguous().view(torch.int32).reshape(-1, 2)                               # moved as integers: a NaN keeps its payload
    for q in range(Q):
        g0 = max(gp[q], 0)
        g1 = max(gp[q + 1], g0)
        cand = [(-o[g * kv + s], vid[g], s, g) for g in range(g0, g1) for s in range(cnt[g])]
        cand.sort()
        n = min(len(cand), k)
        if n:
            flat = torch.tensor([g * kv + s for _, _, s, g in cand[:n]], dtype=torch.int64, device=dev)
            out["video"][q, :n] = torch.tensor([v for _, v, _, _ in cand[:n]], dtype=torch.int64, device=dev)
            out["span"].view(torch.int32)[q, :n] = span_bits[flat]
            out["score"].view(torch.int32)[q, :n] = score.contiguous().view(torch.int32).reshape(-1)[flat]
            out["window"][q, :n] = window.to(torch.int64).reshape(-1)[flat]
            out["cell"][q, :n] = cell.to(torch.int64).reshape(-1, 2)[flat]
        out["count"][q] = n
    return out


# ---------------------------------------------------------------- hard-negative mining (SMIN.mine_pairs)
def _mine_check(what, score, gt_video, negatives, skip):
    if score.dim() != 2:
        raise ValueError(f"{what}: score must be (Q, V), got {tuple(score.shape)}")
    Q, V = score.shape
    gt = host_array(gt_video)
    if gt.shape[0] != Q:
        raise ValueError(f"{what}: gt_video must name a video for each of the Q = {Q} queries of score (Q, V) = {tuple(score.shape)} (got {gt.shape[0]})")
    if Q < 1 or V < 2:
        raise ValueError(f"{what}: needs Q >= 1 queries and V >= 2 videos (score is {tuple(score.shape)})")
    if gt.min() < 0 or gt.max() >= V:
        raise ValueError(f"{what}: gt_video must lie in [0, {V})")
    require_ints(what, ("negatives", negatives, 1, MAX_K), ("skip", skip, 0, MAX_K))
    if skip + negatives > MAX_K or skip + negatives > V - 1:
        raise ValueError(f"{what}: skip + negatives = {skip + negatives} must not exceed {MAX_K} nor the V - 1 = {V - 1} wrong videos of a query")
    if Q * (1 + negatives) >= 2 ** 31:
        raise ValueError(f"{what}: {Q * (1 + negatives)} pairs exceed the int32 lists")
    return Q, V, gt


def mine_pairs(score, gt_video, negatives, skip=0):
    """The pair plan of hard-negative mining, built on the device (include/smin_hip.h, smin_mine_pairs): for each query its own
    video and its ``negatives`` highest-scoring wrong videos after the ``skip`` hardest (often unlabelled true matches).

    ``score (Q, V)`` fp32 HIP tensor: each (query, video) pair's score (SMIN.pair_scores); ``gt_video``: Q host ints in [0, V).
    Order among the videos v != gt_video[q]: higher score first, ties -> lower v, -0 counts as +0 (corpus_topk's order).  Limits:
    negatives >= 1, skip >= 0, skip + negatives <= min(64, V - 1).  Returns a retrieval.PairPlan of P = Q * (1 + negatives) pairs
    whose lists and groupings were formed by the kernels (``PairPlan.from_device``: its host lists ``vi`` / ``qi`` are None): pair
    q * (1 + negatives) is query q's positive, the next ``negatives`` its negatives in rank order.  gt_video and the positive flags
    (host arithmetic: the layout is fixed) travel in one pinned asynchronous copy; one call into the library; no host read."""
    _require_hip(score, "mine_pairs")
    Q, V, gt = _mine_check("mine_pairs", score, gt_video, negatives, skip)
    from .retrieval import PairPlan
    N, dev = int(negatives), score.device
    S, P = 1 + N, Q * (1 + N)
    rows = np.arange(Q, dtype=np.int64) * S
    host = torch.from_numpy(np.concatenate([gt, np.arange(P) % S == 0, rows]).astype(np.int32))
    sc = score.detach().float().contiguous()
    with torch.cuda.device(dev):
        buf = host.pin_memory().to(dev, non_blocking=True)
        out = torch.empty((4 * P + V + Q + 2,), dtype=torch.int32, device=dev)
        cut = np.cumsum([0, P, P, V + 1, P, Q + 1, P])
        lists = [out[cut[k]:cut[k + 1]] for k in range(6)]
        call_ws("smin_mine_pairs", (Q, V, N), stream(), ptr(sc), ptr(buf[:Q]), Q, V, N, int(skip), *[ptr(a) for a in lists], fields="Q, V, N")
        return PairPlan.from_device(*lists, V, Q, positive=buf[Q:Q + P], positive_rows=buf[Q + P:].to(torch.int64), num_positive=Q)


def mine_pairs_torch(score, gt_video, negatives, skip=0):
    """``mine_pairs`` as plain torch + Python on any device (same result, bit for bit): each query's wrong videos sorted by
    (score, video), then the pairs sorted by (video, pair).  Returns the six int32 arrays ``(video_index, query_index, v_ptr,
    v_pairs, q_ptr, q_pairs)`` on ``score``'s device."""
    Q, V, gt = _mine_check("mine_pairs_torch", score, gt_video, negatives, skip)
    N, S = int(negatives), 1 + int(negatives)
    o = _order_word(score.detach().float()).tolist()
    vi, qi = [], []
    for q in range(Q):
        g = int(gt[q])
        ranked = sorted((-o[q][v], v) for v in range(V) if v != g)
        vi += [g] + [v for _, v in ranked[skip:skip + N]]
        qi += [q] * S
    P = Q * S
    v_pairs = sorted(range(P), key=lambda p: (vi[p], p))
    v_ptr = [0] * (V + 1)
    for v in vi:
        v_ptr[v + 1] += 1
    for v in range(V):
        v_ptr[v + 1] += v_ptr[v]
    arrays = (vi, qi, v_ptr, v_pairs, [q * S for q in range(Q + 1)], list(range(P)))
    return tuple(torch.tensor(a, dtype=torch.int32, device=score.device) for a in arrays)


# ---------------------------------------------------------------- video ranking by the pooled pair score
MAX_POOL_L = 4096                   # smin_pair_pool counts a map's cells in fp32


def _temperature(what, tau):
    if not (isinstance(tau, (int, float)) and not isinstance(tau, bool) and 0.0 < float(tau) < float("inf")):
        raise ValueError(f"{what}: tau must be a finite positive number (got {tau!r})")
    return float(tau)


def _video_weight(what, alpha):
    if not (isinstance(alpha, (int, float)) and not isinstance(alpha, bool) and float("-inf") < float(alpha) < float("inf")):
        raise ValueError(f"{what}: the video weight must be a finite number (got {alpha!r})")
    return float(alpha)


def _pool_check(what, pm, ps, pe, moment_mask, tau):
    if pm.dim() != 3 or pm.shape[1] != pm.shape[2]:
        raise ValueError(f"{what}: pm must be (P, L, L), got {tuple(pm.shape)}")
    P, L = pm.shape[0], pm.shape[1]
    if tuple(ps.shape) != (P, L) or tuple(pe.shape) != (P, L) or tuple(moment_mask.shape) != (P, L, L):
        raise ValueError(f"{what}: ps / pe must be (P, L) = {(P, L)} and moment_mask (P, L, L); got {tuple(ps.shape)}, {tuple(pe.shape)}, "
                         f"{tuple(moment_mask.shape)}")
    if P < 1 or not 1 <= L <= MAX_POOL_L:
        raise ValueError(f"{what} needs P >= 1 and 1 <= L <= {MAX_POOL_L} (P={P}, L={L})")
    return P, L, _temperature(what, tau)


def _pair_pool_into(pm, ps, pe, moment_mask, tau, score, pool, cells):
    """smin_pair_pool of P checked maps on ``pm``'s device into the caller's contiguous fp32 ``score (P,)``, ``pool (P, 2)`` and ``cells
    (P,)`` (e.g. a chunk's rows of larger buffers): one launch, nothing else."""
    pm_, ps_, pe_ = (x.detach().float().contiguous() for x in (pm, ps, pe))
    mm_ = byte_mask(moment_mask)
    with torch.cuda.device(pm.device):
        call("smin_pair_pool", stream(), ptr(pm_), ptr(ps_), ptr(pe_), ptr(mm_), pm.shape[0], pm.shape[1], float(tau), ptr(score), ptr(pool), ptr(cells))


def pair_pool(pm, ps, pe, moment_mask, tau=0.1):
    """The pooled score of each of P (video, query) maps (include/smin_hip.h, smin_pair_pool): the log-mean-exp at temperature ``tau`` of
    the valid cells' fused scores ``pm * sqrt(ps_i) * sqrt(pe_j)`` -- the pair score training.pair_rank_loss contrasts, bit for bit.
    Returns ``(score (P,), pool (P, 2), cells (P,))`` fp32: ``pool = {the maximum m, sum exp((f - m) / tau)}``, ``cells`` the number of
    valid cells; a pair without one gives 0 throughout.  HIP tensors only; one launch; no host synchronisation."""
    _require_hip(pm, "pair_pool")
    P, _, tau = _pool_check("pair_pool", pm, ps, pe, moment_mask, tau)
    score = torch.empty((P,), dtype=torch.float32, device=pm.device)
    pool = torch.empty((P, 2), dtype=torch.float32, device=pm.device)
    cells = torch.empty((P,), dtype=torch.float32, device=pm.device)
    _pair_pool_into(pm, ps, pe, moment_mask, tau, score, pool, cells)
    return score, pool, cells


def pair_pool_torch(pm, ps, pe, moment_mask, tau=0.1):
    """``pair_pool`` as plain torch ops on any device, in the dtype of ``pm`` (fp64 inputs give the fp64 reference): the tests'
    restatement, nothing routes here."""
    P, _, tau = _pool_check("pair_pool_torch", pm, ps, pe, moment_mask, tau)
    valid = moment_mask != 0
    f = (pm * torch.sqrt(ps.clamp_min(1e-12)).unsqueeze(2)) * torch.sqrt(pe.clamp_min(1e-12)).unsqueeze(1)
    n = valid.reshape(P, -1).sum(dim=1)
    some = n > 0
    m = torch.where(valid, f, torch.full_like(f, float("-inf"))).reshape(P, -1).max(dim=1).values
    m = torch.where(some, m, torch.zeros_like(m))
    m3 = m.reshape(P, 1, 1)
    z = (torch.exp((torch.where(valid, f, m3) - m3) / tau) * valid.to(f.dtype)).reshape(P, -1).sum(dim=1)
    one = torch.ones_like(z)
    score = torch.where(some, m + tau * torch.log(torch.where(some, z, one) / torch.where(some, n.to(f.dtype), one)), torch.zeros_like(z))
    return score, torch.stack([m, z], dim=1), n.to(f.dtype)


def _group_check(what, pool, cells, group_ptr, tau):
    if pool.dim() != 2 or pool.shape[1] != 2 or tuple(cells.shape) != (pool.shape[0],):
        raise ValueError(f"{what}: pool must be (W, 2) and cells (W,), got {tuple(pool.shape)} and {tuple(cells.shape)}")
    if group_ptr.dim() != 1 or group_ptr.shape[0] < 1:
        raise ValueError(f"{what}: group_ptr must be (G2 + 1,)")
    if pool.shape[0] >= 2 ** 31 or group_ptr.shape[0] > 2 ** 31:
        raise ValueError(f"{what}: {pool.shape[0]} windows in {group_ptr.shape[0] - 1} groups exceed the int32 group_ptr")
    return pool.shape[0], group_ptr.shape[0] - 1, _temperature(what, tau)


def group_pool(pool, cells, group_ptr, tau=0.1):
    """The pooled score of each (query, video) group of a window search (include/smin_hip.h, smin_group_pool): the log-mean-exp over all
    valid cells of the group's windows, composed from ``pair_pool``'s ``pool (W, 2)`` and ``cells (W,)`` of the (query, window) maps;
    ``group_ptr (G2 + 1,)``: group g owns windows ``group_ptr[g] .. group_ptr[g + 1]``.  A cell in the overlap of two windows counts
    twice.  Returns ``(score (G2,), cells (G2,))`` fp32, 0 and 0 for a group without cells.  HIP tensors only; one launch; no host
    synchronisation."""
    _require_hip(group_ptr, "group_pool")
    W, G2, tau = _group_check("group_pool", pool, cells, group_ptr, tau)
    dev = group_ptr.device
    pool_, cells_, gp = pool.detach().float().contiguous(), cells.detach().float().contiguous(), group_ptr.to(torch.int32).contiguous()
    score = torch.empty((G2,), dtype=torch.float32, device=dev)
    out_cells = torch.empty((G2,), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        call("smin_group_pool", stream(), ptr(pool_) if W else None, ptr(cells_) if W else None, ptr(gp), G2, W, tau, ptr(score) if G2 else None,
             ptr(out_cells) if G2 else None)
    return score, out_cells


def group_pool_torch(pool, cells, group_ptr, tau=0.1):
    """``group_pool`` as plain torch + Python on any device, in the dtype of ``pool``: the tests' restatement (reads the host)."""
    W, G2, tau = _group_check("group_pool_torch", pool, cells, group_ptr, tau)
    gp = group_ptr.to(torch.int64).tolist()
    score, out_cells = pool.new_zeros((G2,)), pool.new_zeros((G2,))
    for g in range(G2):
        w0 = min(max(gp[g], 0), W)
        w1 = min(max(gp[g + 1], w0), W)
        keep = cells[w0:w1] > 0
        if not bool(keep.any()):
            continue
        m, s = pool[w0:w1, 0][keep], pool[w0:w1, 1][keep]
        big = m.max()
        total = cells[w0:w1][keep].sum()
        score[g] = big + tau * torch.log((s * torch.exp((m - big) / tau)).sum() / total)
        out_cells[g] = total
    return score, out_cells


_RANK_KEYS = ("video", "score", "count", "pair_rank", "weight", "gt_rank")


def _rank_check(what, pair_score, pair_cells, pair_video, pair_ptr, n, alpha, gt_video):
    if pair_score.dim() != 1 or tuple(pair_cells.shape) != tuple(pair_score.shape) or tuple(pair_video.shape) != tuple(pair_score.shape):
        raise ValueError(f"{what}: pair_score, pair_cells and pair_video must be (P,); got {tuple(pair_score.shape)}, {tuple(pair_cells.shape)}, "
                         f"{tuple(pair_video.shape)}")
    if pair_ptr.dim() != 1 or pair_ptr.shape[0] < 1:
        raise ValueError(f"{what}: pair_ptr must be (Q + 1,)")
    P, Q = pair_score.shape[0], pair_ptr.shape[0] - 1
    if not (isinstance(n, int) and not isinstance(n, bool) and 1 <= n <= MAX_K):
        raise ValueError(f"{what} needs an integer 1 <= n <= {MAX_K} (got {n!r})")
    if P > 0x7fff0000:
        raise ValueError(f"{what}: {P} pairs exceed the int32 pair_ptr")
    if gt_video is not None and tuple(gt_video.shape) != (Q,):
        raise ValueError(f"{what}: gt_video must be (Q,) = ({Q},) (got {tuple(gt_video.shape)})")
    return P, Q, _video_weight(what, alpha)


def rank_videos(pair_score, pair_cells, pair_video, pair_ptr, n=5, alpha=0.0, gt_video=None):
    """Each query's videos ranked by the pooled pair score (include/smin_hip.h, smin_video_rank): one workgroup per query ranks its pairs
    by counting, any number of pairs per query.

    ``pair_score (P,)`` / ``pair_cells (P,)``: ``pair_pool``'s (or ``group_pool``'s) score and cell count of P (query, video) pairs;
    ``pair_video (P,)`` each pair's video; ``pair_ptr (Q + 1,)``: query q owns pairs ``pair_ptr[q] .. pair_ptr[q + 1]``; ``gt_video (Q,)``
    int tensor or None: each query's own video.  Candidates: the pairs with cells > 0.  Order: higher score first, -0 counts as +0,
    ties -> lower video, then the earlier pair (corpus_topk's).  HIP tensors only; one launch; no host synchronisation.  Returns a
    dict: ``video (Q, n)`` int64 (-1 for empty slots), ``score (Q, n)`` (0), ``count (Q,)`` int32, ``pair_rank (P,)`` int32 the rank among
    the query's candidates (-1 for a non-candidate; not limited by n), ``weight (P,)`` = ``exp(alpha * (s_p - the query's best))`` (0
    for a non-candidate; exactly 1 at alpha = 0) and ``gt_rank (Q,)`` int32 the rank of gt_video's pair (-1: not listed, no candidate,
    or no gt_video)."""
    _require_hip(pair_ptr, "rank_videos")
    P, Q, alpha = _rank_check("rank_videos", pair_score, pair_cells, pair_video, pair_ptr, n, alpha, gt_video)
    dev = pair_ptr.device
    args = [pair_score.detach().float(), pair_cells.detach().float(), pair_video.to(torch.int32), pair_ptr.to(torch.int32)]
    args = [a.contiguous() for a in args]
    gt = None if gt_video is None or Q == 0 else gt_video.to(torch.int32).contiguous()
    video = torch.empty((Q, n), dtype=torch.int64, device=dev)
    score = torch.empty((Q, n), dtype=torch.float32, device=dev)
    count = torch.empty((Q,), dtype=torch.int32, device=dev)
    pair_rank = torch.empty((P,), dtype=torch.int32, device=dev)
    weight = torch.empty((P,), dtype=torch.float32, device=dev)
    gt_rank = torch.empty((Q,), dtype=torch.int32, device=dev)
    opt = lambda a: ptr(a) if a.numel() else None
    with torch.cuda.device(dev):
        call("smin_video_rank", stream(), *[opt(a) for a in args], ptr(gt), P, Q, n, alpha, opt(video), opt(score), opt(count), opt(pair_rank),
             opt(weight), opt(gt_rank))
    return dict(zip(_RANK_KEYS, (video, score, count, pair_rank, weight, gt_rank)))


def rank_videos_torch(pair_score, pair_cells, pair_video, pair_ptr, n=5, alpha=0.0, gt_video=None):
    """``rank_videos`` as plain torch + Python on any device: each query's candidates sorted by (score, video, pair), the same tie
    rules; ``score`` and ``weight`` in the dtype of ``pair_score`` (fp64 inputs give the fp64 reference).  Reads the host."""
    P, Q, alpha = _rank_check("rank_videos_torch", pair_score, pair_cells, pair_video, pair_ptr, n, alpha, gt_video)
    dev, dt = pair_ptr.device, pair_score.dtype
    s, c, vid, pp = pair_score.detach().tolist(), pair_cells.tolist(), pair_video.to(torch.int64).tolist(), pair_ptr.to(torch.int64).tolist()
    gt = None if gt_video is None else gt_video.to(torch.int64).tolist()
    video = torch.full((Q, n), -1, dtype=torch.int64, device=dev)
    score = torch.zeros((Q, n), dtype=dt, device=dev)
    count, gt_rank = [0] * Q, [-1] * Q
    pair_rank, best = [-1] * P, [0.0] * P
    for q in range(Q):
        g0 = min(max(pp[q], 0), P)
        g1 = min(max(pp[q + 1], g0), P)
        cand = sorted((-(s[e] + 0.0), vid[e], e) for e in range(g0, g1) if c[e] > 0)          # -0 + 0 = +0: -0 counts as +0
        for r, (_, v, e) in enumerate(cand):
            pair_rank[e] = r
            best[e] = s[cand[0][2]]
            if gt is not None and v == gt[q] and gt_rank[q] < 0:
                gt_rank[q] = r
        count[q] = min(len(cand), n)
        if count[q]:
            rows = torch.tensor([e for _, _, e in cand[:n]], dtype=torch.int64, device=dev)
            video[q, :count[q]] = torch.tensor([v for _, v, _ in cand[:n]], dtype=torch.int64, device=dev)
            score[q, :count[q]] = pair_score.detach()[rows]
    rank_t = torch.tensor(pair_rank, dtype=torch.int32, device=dev)
    listed = rank_t >= 0
    if alpha == 0.0:
        weight = listed.to(dt)
    else:
        top = torch.tensor(best, dtype=dt, device=dev)
        weight = torch.where(listed, torch.exp(alpha * (torch.where(listed, pair_score.detach(), top) - top)), torch.zeros_like(top))
    return dict(zip(_RANK_KEYS, (video, score, torch.tensor(count, dtype=torch.int32, device=dev), rank_t, weight,
                                 torch.tensor(gt_rank, dtype=torch.int32, device=dev))))


def _reweight_check(what, score, count, pair_rank, weight, max_videos):
    if score.dim() != 2 or not 1 <= score.shape[1] <= MAX_K:
        raise ValueError(f"{what}: score must be (P, k) with 1 <= k <= {MAX_K}, got {tuple(score.shape)}")
    P = score.shape[0]
    if tuple(count.shape) != (P,) or tuple(pair_rank.shape) != (P,) or tuple(weight.shape) != (P,):
        raise ValueError(f"{what}: count, pair_rank and weight must be (P,) = ({P},); got {tuple(count.shape)}, {tuple(pair_rank.shape)}, "
                         f"{tuple(weight.shape)}")
    if max_videos is None:
        return P, 0
    if not (isinstance(max_videos, int) and not isinstance(max_videos, bool) and 0 <= max_videos < 2 ** 31):
        raise ValueError(f"{what}: max_videos must be None or an integer >= 0, 0 for no cut (got {max_videos!r})")
    return P, max_videos


def reweight_moments(score, count, pair_rank, weight, max_videos=None):
    """The pairs' moment lists weighted by their video and cut to each query's best videos (include/smin_hip.h, smin_moment_reweight):
    ``(score * weight[p], count where 0 <= pair_rank[p] < max_videos else 0)`` for ``score (P, k)`` / ``count (P,)`` of top_moments or
    merge_window_moments and ``pair_rank`` / ``weight (P,)`` of ``rank_videos``; ``max_videos`` None or 0: no cut.  corpus_topk /
    corpus_span_topk then rank the lists as they are.  HIP tensors only; one launch; no host synchronisation."""
    _require_hip(score, "reweight_moments")
    P, cut = _reweight_check("reweight_moments", score, count, pair_rank, weight, max_videos)
    args = [score.detach().float(), count.to(torch.int32), pair_rank.to(torch.int32), weight.detach().float()]
    args = [a.contiguous() for a in args]
    out_score, out_count = torch.empty_like(args[0]), torch.empty_like(args[1])
    if P:
        with torch.cuda.device(score.device):
            call("smin_moment_reweight", stream(), *[ptr(a) for a in args], P, score.shape[1], cut, ptr(out_score), ptr(out_count))
    return out_score, out_count


def reweight_moments_torch(score, count, pair_rank, weight, max_videos=None):
    """``reweight_moments`` as plain torch ops on any device, in the dtype of ``score``."""
    _, cut = _reweight_check("reweight_moments_torch", score, count, pair_rank, weight, max_videos)
    keep = torch.ones_like(pair_rank, dtype=torch.bool) if cut <= 0 else (pair_rank >= 0) & (pair_rank < cut)
    return score * weight.to(score.dtype).unsqueeze(1), torch.where(keep, count, torch.zeros_like(count))


# ---------------------------------------------------------------- compact video banks
BANK_STORAGES = {"fp32": 0, "bf16": 1, "int8": 2}       # include/smin_hip.h SMIN_BANK_BF16 / SMIN_BANK_INT8 (0: the fp32 bank, no code)
_CODE_DTYPES = {torch.float32: "fp32", torch.bfloat16: "bf16", torch.int8: "int8"}


def require_storage(what, storage):
    if storage not in BANK_STORAGES:
        raise ValueError(f"{what}: storage must be one of {sorted(BANK_STORAGES)} (got {storage!r})")
    return storage


def bank_storage(what, codes, scale=None):
    """The storage a bank's ``fv`` is held in, from its dtype -- ``"fp32"`` (float32), ``"bf16"`` (bfloat16, no scale) or ``"int8"`` (int8
    with ``scale``, float32, one value per row of D codes); ValueError for anything else."""
    storage = _CODE_DTYPES.get(codes.dtype)
    if storage is None:
        raise ValueError(f"{what}: a bank holds float32 values, bfloat16 codes or int8 codes (got {codes.dtype})")
    if (storage == "int8") != (scale is not None):
        raise ValueError(f"{what}: int8 codes come with their rows' scales, {storage} with none")
    if scale is not None and (scale.dtype != torch.float32 or tuple(scale.shape) != tuple(codes.shape[:-1])):
        raise ValueError(f"{what}: scale must be float32 {tuple(codes.shape[:-1])}, one value per row of codes (got {scale.dtype} {tuple(scale.shape)})")
    return storage


def _encode_check(what, fv, storage):
    require_storage(what, storage)
    if storage == "fp32":
        raise ValueError(f"{what}: storage must be 'bf16' or 'int8' (an fp32 bank has no code)")
    if fv.dim() < 2 or fv.dtype != torch.float32 or fv.shape[-1] < 4 or fv.shape[-1] % 4 != 0 or fv.numel() < 1:
        raise ValueError(f"{what}: fv must be float32 (..., D) with D >= 4, D % 4 == 0 and at least one row (got {fv.dtype} {tuple(fv.shape)})")


def bank_encode_torch(fv, storage):
    """``bank_encode`` as plain torch ops on any device: the tests' restatement of the code (include/smin_hip.h, SMIN_BANK_*), nothing
    routes here.  ``"bf16"``: round to nearest even on the bit pattern, ``(u + 0x7fff + ((u >> 16) & 1)) >> 16``, a NaN -> 0x7fc0.
    ``"int8"``, per row of D values, in float32 ops: ``amax = max |x|``, ``scale = amax / 127`` and ``q = clamp(round_half_even(x /
    scale), -127, 127)``; a zero row gives scale 0 and a row with a NaN or an infinity scale NaN, codes 0 in both cases."""
    _encode_check("bank_encode_torch", fv, storage)
    x = fv.detach()
    if storage == "bf16":
        u = x.contiguous().view(torch.int32).to(torch.int64) & 0xffffffff
        r = (u + 0x7fff + ((u >> 16) & 1)) >> 16
        r = torch.where((u & 0x7fffffff) > 0x7f800000, torch.full_like(r, 0x7fc0), r)
        r = torch.where(r >= 0x8000, r - 0x10000, r).to(torch.int16)               # the 16 bits as a signed word
        return r.view(torch.bfloat16), None
    finite = torch.isfinite(x).all(dim=-1)
    amax = torch.where(torch.isfinite(x), x.abs(), torch.zeros_like(x)).amax(dim=-1)
    scale = torch.where(finite, amax / 127.0, torch.full_like(amax, float("nan")))
    live = (finite & (scale > 0)).unsqueeze(-1)
    q = torch.round(x / torch.where(live, scale.unsqueeze(-1), torch.ones_like(x))).clamp(-127.0, 127.0)
    return torch.where(live, q, torch.zeros_like(q)).to(torch.int8), scale


def bank_decode_torch(codes, scale=None):
    """``bank_decode`` as plain torch ops on any device: ``bits << 16`` for bfloat16 codes, ``float(q) * scale`` (one float32
    multiplication) for int8 codes.  The tests' restatement, nothing routes here."""
    if bank_storage("bank_decode_torch", codes, scale) == "int8":
        return codes.to(torch.float32) * scale.unsqueeze(-1)
    return codes.to(torch.float32)


def bank_encode(fv, storage):
    """``fv (..., D)`` float32 as a compact code (include/smin_hip.h, smin_bank_encode; csrc/bank_codec.hip): ``(codes, scale)`` with
    ``codes (..., D)`` torch.bfloat16 and ``scale`` None for ``storage="bf16"``, ``codes`` torch.int8 and ``scale (...)`` float32, one per
    row of D values, for ``"int8"``.  One launch, one wave per row; HIP tensors only; no host synchronisation."""
    _require_hip(fv, "bank_encode")
    _encode_check("bank_encode", fv, storage)
    x = fv.detach().contiguous()
    D, R = x.shape[-1], x.numel() // x.shape[-1]
    codes = torch.empty(x.shape, dtype=torch.bfloat16 if storage == "bf16" else torch.int8, device=x.device)
    scale = torch.empty(x.shape[:-1], dtype=torch.float32, device=x.device) if storage == "int8" else None
    with torch.cuda.device(x.device):
        call("smin_bank_encode", stream(), ptr(x), R, D, BANK_STORAGES[storage], ptr(codes), ptr(scale))
    return codes, scale


def bank_decode(codes, scale=None):
    """The decoded values of a compact code, float32 ``(..., D)`` (include/smin_hip.h, smin_bank_decode): what every kernel over a
    compact bank computes with.  HIP tensors only; one launch; no host synchronisation."""
    _require_hip(codes, "bank_decode")
    storage = bank_storage("bank_decode", codes, scale)
    if storage == "fp32":
        raise ValueError("bank_decode: float32 values are no code")
    if codes.dim() < 2 or codes.shape[-1] < 4 or codes.shape[-1] % 4 != 0 or codes.numel() < 1:
        raise ValueError(f"bank_decode: codes must be (..., D) with D >= 4, D % 4 == 0 and at least one row (got {tuple(codes.shape)})")
    c = codes.detach().contiguous()
    sc = None if scale is None else scale.detach().contiguous()
    out = torch.empty(c.shape, dtype=torch.float32, device=c.device)
    with torch.cuda.device(c.device):
        call("smin_bank_decode", stream(), ptr(c), ptr(sc), c.numel() // c.shape[-1], c.shape[-1], BANK_STORAGES[storage], ptr(out))
    return out


# ---------------------------------------------------------------- first-stage video score from the banks alone
PREFILTER_MAX_L, PREFILTER_MAX_T, PREFILTER_MAX_Q = 64, 2048, 65535        # csrc/prefilter.hip
PREFILTER_WS_CAP = 256 << 20        # bytes of workspace per call of smin_prefilter_scores: the videos are tiled to stay under it


def _prefilter_check(what, fv, fs, w, b, length_mask, moment_mask, T, L, C, tau):
    if fv.dim() != 3 or fs.dim() != 2 or fv.shape[2] != fs.shape[1] or fv.shape[0] < 1 or fs.shape[0] < 1:
        raise ValueError(f"{what}: fv must be (V, T, D) and fs (Q, D) with V, Q >= 1; got {tuple(fv.shape)} and {tuple(fs.shape)}")
    V, D, Q = fv.shape[0], fv.shape[2], fs.shape[0]
    require_ints(what, ("L", L, 1, PREFILTER_MAX_L), ("T", T, L, PREFILTER_MAX_T), ("C", C, 1, 65536))
    if fv.shape[1] != T or D % 4 != 0 or Q > PREFILTER_MAX_Q:
        raise ValueError(f"{what}: fv must hold T = {T} frames of D % 4 == 0 features for at most {PREFILTER_MAX_Q} queries; got "
                         f"{tuple(fv.shape)} and Q = {Q}")
    if tuple(w.shape) != (3, D) or tuple(b.shape) != (3,):
        raise ValueError(f"{what}: w must be (3, D) = (3, {D}) and b (3,), the heads in the order (pm, ps, pe); got {tuple(w.shape)} and "
                         f"{tuple(b.shape)}")
    if tuple(length_mask.shape) != (V, L) or tuple(moment_mask.shape) != (V, L, L):
        raise ValueError(f"{what}: length_mask must be (V, L) = {(V, L)} and moment_mask (V, L, L); got {tuple(length_mask.shape)} and "
                         f"{tuple(moment_mask.shape)}")
    return Q, V, D, _temperature(what, tau)


def prefilter_scores(fv, fs, w, b, length_mask, moment_mask, T, L, C, tau=0.1, maps=False, fv_scale=None):
    """The first-stage score of every (query, video) of a video bank's ``fv (V, T, D)`` and a query bank's ``fs (Q, D)``
    (include/smin_hip.h, smin_prefilter_scores): the model with zero SMI layers -- the heads ``w (3, D)`` / ``b (3,)``, in the order
    (pm, ps, pe), on ProposalGeneration's output --, pooled as ``pair_pool`` pools the full model's maps, at temperature ``tau``.  One
    contraction over D on the fp32 MFMA engine (in the mode of set_gemm_mode) and one workgroup per pair.

    Returns ``(score (Q, V), pool (Q, V, 2), cells (Q, V))`` fp32; with ``maps=True`` also ``pm0 (Q, V, L, L)``, ``ps0`` and ``pe0 (Q, V,
    L)``.  The videos are processed in tiles whose workspace stays under PREFILTER_WS_CAP; a tile changes no bits, every (q, v) is
    computed alone.  A compact bank passes its codes as ``fv`` (torch.bfloat16, or torch.int8 with ``fv_scale (V,
    T)``): smin_prefilter_scores_compact decodes inside the contraction's loader -- the bits of the decoded bank, which is never
    formed.  HIP tensors only; no host synchronisation."""
    _require_hip(fv, "prefilter_scores")
    Q, V, D, tau = _prefilter_check("prefilter_scores", fv, fs, w, b, length_mask, moment_mask, T, L, C, tau)
    dev = fv.device
    storage = bank_storage("prefilter_scores", fv, fv_scale) if fv.dtype in (torch.bfloat16, torch.int8) or fv_scale is not None else "fp32"
    fs_, w_, b_ = (x.detach().float().contiguous() for x in (fs, w, b))
    fv_ = fv.detach().contiguous() if storage != "fp32" else fv.detach().float().contiguous()
    sc_ = None if fv_scale is None else fv_scale.detach().contiguous()
    lm_, mm_ = byte_mask(length_mask), byte_mask(moment_mask)
    lib = load()
    per_video = max(int(lib.smin_prefilter_ws_bytes(Q, 2, T, D)) - int(lib.smin_prefilter_ws_bytes(Q, 1, T, D)), 1)
    step = max(1, min(V, 0x7fff0000 // T, PREFILTER_WS_CAP // per_video - 1))
    new = lambda *shape: torch.empty(shape, dtype=torch.float32, device=dev)
    outs = [new(Q, V), new(Q, V, 2), new(Q, V)] + ([new(Q, V, L, L), new(Q, V, L), new(Q, V, L)] if maps else [])
    with torch.cuda.device(dev):
        for v0 in range(0, V, step):
            v1 = min(v0 + step, V)
            tile = outs if (v0, v1) == (0, V) else [new(Q, v1 - v0, *o.shape[2:]) for o in outs]
            nbytes = int(lib.smin_prefilter_ws_bytes(Q, v1 - v0, T, D))
            ws = torch.empty((nbytes,), dtype=torch.uint8, device=dev)
            bank = [ptr(fv_[v0:v1])] if storage == "fp32" else [ptr(fv_[v0:v1]), None if sc_ is None else ptr(sc_[v0:v1]), BANK_STORAGES[storage]]
            call("smin_prefilter_scores" if storage == "fp32" else "smin_prefilter_scores_compact", stream(), *bank, ptr(fs_), ptr(w_), ptr(b_),
                 ptr(lm_[v0:v1]), ptr(mm_[v0:v1]), Q, v1 - v0, T, L, C, D, tau, *[ptr(o) for o in tile], *([] if maps else [None] * 3), ptr(ws), nbytes)
            if tile is not outs:
                for o, part in zip(outs, tile):
                    o[:, v0:v1] = part
    return tuple(outs)


def prefilter_maps(fv, fs, w, b, length_mask, moment_mask, T, L, C, tau=0.1):
    """``prefilter_scores(maps=True)`` with a backward (include/smin_hip.h, smin_prefilter_maps_bwd): the first-stage
    maps of every (query, video), differentiable with respect to ``fv``, ``fs``, ``w`` and ``b`` -- what training the first stage
    needs.  Returns ``(pm0 (Q, V, L, L), ps0 (Q, V, L), pe0 (Q, V, L), score (Q, V))``: the maps have prefilter_scores' bits, the score
    is detached.  The backward is HIP kernels and the library's two fp32 contractions (in the mode of set_gemm_mode), every sum in an
    order fixed by the shapes: the same bits every run.

    One call, never tiled -- a tile would change the summation order of the gradients of ``fs``, ``w`` and ``b`` --: where the
    forward's and the backward's workspaces together would pass PREFILTER_WS_CAP it raises ValueError.  HIP tensors only; no host
    synchronisation."""
    _require_hip(fv, "prefilter_maps")
    Q, V, D, tau = _prefilter_check("prefilter_maps", fv, fs, w, b, length_mask, moment_mask, T, L, C, tau)
    if any(x.dtype != torch.float32 for x in (fv, fs, w, b)):
        raise ValueError("prefilter_maps: fv, fs, w and b must be float32 (the gradients are formed in fp32)")
    lib = load()
    nbytes = int(lib.smin_prefilter_ws_bytes(Q, V, T, D)), int(lib.smin_prefilter_bwd_ws_bytes(Q, V, T, D))
    if min(nbytes) == 0 or sum(nbytes) > PREFILTER_WS_CAP:
        raise ValueError(f"prefilter_maps: {Q} queries over {V} videos of {T} frames need {nbytes[0]} + {nbytes[1]} bytes of workspace in "
                         f"one call (0: sizes out of range), the cap is {PREFILTER_WS_CAP}: train on smaller groups (the call is not tiled)")
    from .functional import PrefilterMapsFn
    with torch.cuda.device(fv.device):
        pm0, ps0, pe0, score, _, _ = PrefilterMapsFn.apply(fv, fs, w, b, byte_mask(length_mask), byte_mask(moment_mask), int(T), int(L), int(C), tau)
    return pm0, ps0, pe0, score


@functools.lru_cache(maxsize=8)
def _prefilter_window_weights(T, L, C):
    r = T // L
    weight = np.zeros((L, L, T))
    for i in range(L):
        for j in range(i, L):
            n = (j - i + 1) * r
            cs, c = max(1, n // C), min(C, n)
            weight[i, j, i * r:i * r + c * cs] = float(np.float32(1.0) / np.float32(cs))
    return weight


def _prefilter_windows(T, L, C, dtype, device):
    """``weight (L, L, T)`` of the content matrix's clips summed over C: cell (i, j) weighs the frames [i r, i r + c cs) by 1 / cs rounded
    to fp32, as the reference stores it, with r = T // L, n = (j - i + 1) r, cs = max(1, n // C), c = min(C, n) (oracle content_windows'
    arithmetic; an empty range under the diagonal).  Host arithmetic on T, L and C alone (kept per (T, L, C)), one copy to the device."""
    return torch.from_numpy(_prefilter_window_weights(int(T), int(L), int(C))).to(device=device, dtype=dtype)


def prefilter_scores_torch(fv, fs, w, b, length_mask, moment_mask, T, L, C, tau=0.1, maps=False):
    """``prefilter_scores`` as plain torch ops on any device, in the dtype of ``fv`` (fp64 inputs give the fp64 reference): the tests'
    restatement, nothing routes here.  Forms the (Q, V, L, L) maps at once."""
    Q, V, D, tau = _prefilter_check("prefilter_scores_torch", fv, fs, w, b, length_mask, moment_mask, T, L, C, tau)
    dt, r = fv.dtype, T // L
    fs, w, b = fs.to(dt), w.to(dt), b.to(dt)
    a = torch.einsum("vtd,hqd->hqvt", fv, fs.unsqueeze(0) * w.unsqueeze(1))                       # (3, Q, V, T)
    weight = _prefilter_windows(T, L, C, dt, fv.device)
    valid = (moment_mask != 0).unsqueeze(0)
    pm0 = torch.sigmoid(torch.einsum("qvt,ijt->qvij", a[0], weight) / C + b[0]) * valid.to(dt)
    clip = lambda x: x[..., :L * r].reshape(Q, V, L, r).sum(dim=-1) / r
    keep = (length_mask != 0).to(dt).unsqueeze(0)
    ps0, pe0 = torch.sigmoid(clip(a[1]) + b[1]) * keep, torch.sigmoid(clip(a[2]) + b[2]) * keep
    score, pool, cells = pair_pool_torch(pm0.reshape(Q * V, L, L), ps0.reshape(Q * V, L), pe0.reshape(Q * V, L),
                                         valid.expand(Q, V, L, L).reshape(Q * V, L, L), tau)
    out = (score.reshape(Q, V), pool.reshape(Q, V, 2), cells.reshape(Q, V))
    return out + (pm0, ps0, pe0) if maps else out


def _select_check(what, pair_rank, M):
    if pair_rank.dim() != 2 or pair_rank.shape[0] < 1 or pair_rank.shape[1] < 1:
        raise ValueError(f"{what}: pair_rank must be (Q, V) with Q, V >= 1, got {tuple(pair_rank.shape)}")
    require_ints(what, ("M", M, 1, 2 ** 31 - 1))
    return pair_rank.shape[0], pair_rank.shape[1], min(int(M), pair_rank.shape[1])


def prefilter_select(pair_rank, M):
    """Each query's best ``Ms = min(M, V)`` videos as the pair lists of a search (include/smin_hip.h, smin_prefilter_select).
    ``pair_rank (Q, V)``: rank_videos' ``pair_rank`` over the (Q, V) first-stage scores with ``pair_ptr[q] = q * V``.  Each query keeps
    the videos with ``0 <= rank < Ms``; with fewer candidates its lowest-indexed non-candidates fill the list.  Returns ``(video (Q,
    Ms), query (Q, Ms))`` int32, ``video[q]`` ascending, ``query[q] = q``.  HIP tensors only; one launch; no host synchronisation."""
    _require_hip(pair_rank, "prefilter_select")
    Q, V, Ms = _select_check("prefilter_select", pair_rank, M)
    rank = pair_rank.to(torch.int32).contiguous()
    video = torch.empty((Q, Ms), dtype=torch.int32, device=rank.device)
    query = torch.empty((Q, Ms), dtype=torch.int32, device=rank.device)
    with torch.cuda.device(rank.device):
        call("smin_prefilter_select", stream(), ptr(rank), Q, V, int(M), ptr(video), ptr(query))
    return video, query


def prefilter_select_torch(pair_rank, M):
    """``prefilter_select`` as plain torch ops on any device (for ranks that are rank_videos'): the tests' restatement."""
    Q, V, Ms = _select_check("prefilter_select_torch", pair_rank, M)
    kept = (pair_rank >= 0) & (pair_rank < Ms)
    non = pair_rank < 0
    need = Ms - kept.sum(dim=1, keepdim=True)
    keep = kept | (non & (non.cumsum(dim=1) <= need))
    video = torch.sort((~keep).to(torch.int8), dim=1, stable=True).indices[:, :Ms].to(torch.int32)
    query = torch.arange(Q, dtype=torch.int32, device=pair_rank.device).unsqueeze(1).expand(Q, Ms).contiguous()
    return video, query


# ---------------------------------------------------------------- the window plan of a pruned window search
def _expand_check(what, sel_video, video_ptr, W, cap):
    if sel_video.dim() != 2 or sel_video.shape[0] < 1 or sel_video.shape[1] < 1:
        raise ValueError(f"{what}: sel_video must be (Q, Ms) with Q, Ms >= 1, got {tuple(sel_video.shape)}")
    if video_ptr.dim() != 1 or video_ptr.shape[0] < 1:
        raise ValueError(f"{what}: video_ptr must be (V + 1,)")
    require_ints(what, ("W", W, 0, 2 ** 31 - 1), ("cap", cap, 0, 2 ** 31 - 1))
    Q, Ms = sel_video.shape
    if Q * Ms > 0x7f000000:
        raise ValueError(f"{what}: {Q} queries of {Ms} surviving videos exceed the {0x7f000000} groups of one call")
    return Q, Ms, video_ptr.shape[0] - 1


def expand_survivor_windows(sel_video, video_ptr, W, cap):
    """The (query, window) plan of a pruned window search (include/smin_hip.h, smin_window_expand): each query's surviving videos
    ``sel_video (Q, Ms)`` (prefilter_select's, ascending per query; an entry outside [0, V) is an empty group) expanded to their windows
    by ``video_ptr (V + 1,)`` int64, a WindowBank's ``video_ptr_d`` over its ``W`` windows, into lists of ``cap`` slots.  Returns
    ``(group_ptr (Q * Ms + 1,) int64, win_index (cap,) int32, win_query (cap,) int32, total (1,) int64)``: group ``q * Ms + j`` owns the
    slots of video ``sel_video[q, j]``'s windows in start order, slots ``>= total`` hold window 0 and query 0 (padding the model can
    score and no group owns), ``total`` is not clamped; with ``total > cap`` nothing lies past ``cap`` and every ``group_ptr`` entry is
    clamped to it.  HIP tensors only; three launches; no host synchronisation."""
    _require_hip(sel_video, "expand_survivor_windows")
    Q, Ms, V = _expand_check("expand_survivor_windows", sel_video, video_ptr, W, cap)
    dev = sel_video.device
    sel, vp = sel_video.to(torch.int32).contiguous(), video_ptr.to(torch.int64).contiguous()
    group_ptr = torch.empty((Q * Ms + 1,), dtype=torch.int64, device=dev)
    win_index = torch.empty((int(cap),), dtype=torch.int32, device=dev)
    win_query = torch.empty((int(cap),), dtype=torch.int32, device=dev)
    total = torch.empty((1,), dtype=torch.int64, device=dev)
    with torch.cuda.device(dev):
        call("smin_window_expand", stream(), ptr(sel), ptr(vp), Q, Ms, V, int(W), int(cap), ptr(group_ptr), ptr(win_index) if cap else None,
             ptr(win_query) if cap else None, ptr(total))
    return group_ptr, win_index, win_query, total


def expand_survivor_windows_torch(sel_video, video_ptr, W, cap):
    """``expand_survivor_windows`` as plain torch ops on any device: the tests' restatement (no host read)."""
    Q, Ms, V = _expand_check("expand_survivor_windows_torch", sel_video, video_ptr, W, cap)
    dev = sel_video.device
    sel, vp = sel_video.to(torch.int64).reshape(-1), video_ptr.to(torch.int64)
    inside = (sel >= 0) & (sel < V)
    v = sel.clamp(0, max(V - 1, 0))
    lo = vp[v].clamp(0, W)
    hi = torch.minimum(torch.maximum(vp[(v + 1).clamp(max=V)], lo), torch.full_like(lo, W))
    n = torch.where(inside, hi - lo, torch.zeros_like(lo))
    ptr_ = torch.cat([n.new_zeros(1), n.cumsum(0)])
    total = ptr_[-1:].clone()
    slot = torch.arange(int(cap), dtype=torch.int64, device=dev)
    g = torch.searchsorted(ptr_[1:].contiguous(), slot, right=True).clamp(max=Q * Ms - 1)         # the group whose slots hold s, for s < total
    real = slot < total
    win_index = torch.where(real, lo[g] + (slot - ptr_[g]), torch.zeros_like(slot)).to(torch.int32)
    win_query = torch.where(real, g // Ms, torch.zeros_like(slot)).to(torch.int32)
    return ptr_.clamp(max=int(cap)), win_index, win_query, total


def survivor_window_capacity(video_ptr, Ms, Q):
    """The slots ``expand_survivor_windows`` needs in the worst case, host arithmetic on a WindowBank's host ``video_ptr``: ``Q`` times the
    sum of the ``Ms`` largest per-video window counts -- no query's ``Ms`` survivors own more.  Exact where all videos have one count."""
    vp = host_array(video_ptr)
    require_ints("survivor_window_capacity", ("Ms", Ms, 0, 2 ** 31 - 1), ("Q", Q, 0, 2 ** 31 - 1))
    if vp.ndim != 1 or vp.shape[0] < 1:
        raise ValueError("survivor_window_capacity: video_ptr must be (V + 1,)")
    counts = np.sort(np.maximum(vp[1:] - vp[:-1], 0))[::-1]
    return int(Q) * int(counts[:int(Ms)].sum())


# ---------------------------------------------------------------- the corpus-wide first-stage cut over shards
PREFILTER_FOLD_MAX_M = 2048         # csrc/prefilter_fold.hip: a query's slots and their free list stay in LDS


def _fold_check(what, slot_score, slot_cells, slot_video, score, cells, seen):
    if slot_score.dim() != 2 or slot_score.shape[0] < 1 or tuple(slot_cells.shape) != tuple(slot_score.shape) or tuple(slot_video.shape) != tuple(slot_score.shape):
        raise ValueError(f"{what}: slot_score, slot_cells and slot_video must be (Q, M) with Q >= 1; got {tuple(slot_score.shape)}, "
                         f"{tuple(slot_cells.shape)}, {tuple(slot_video.shape)}")
    Q, M = slot_score.shape
    if score.dim() != 2 or score.shape[0] != Q or score.shape[1] < 1 or tuple(cells.shape) != tuple(score.shape):
        raise ValueError(f"{what}: score and cells must be (Q, Vs) = ({Q}, Vs >= 1); got {tuple(score.shape)} and {tuple(cells.shape)}")
    Vs = score.shape[1]
    if Vs > 0x7fff0000:
        raise ValueError(f"{what}: {Vs} videos in one shard exceed the int32 video ids")
    require_ints(what, ("M", M, 1, PREFILTER_FOLD_MAX_M), ("seen", seen, 0, 2 ** 31 - 1 - Vs))
    return Q, M, Vs, min(M, int(seen)), min(M, int(seen) + Vs)


def prefilter_fold(slot_score, slot_cells, slot_video, score, cells, seen, copy_src=None):
    """One shard folded into the running best-M of every query (include/smin_hip.h, smin_prefilter_fold): the state ``slot_score`` /
    ``slot_cells (Q, M)`` float32 and ``slot_video (Q, M)`` int32 (the global id, -1 for an empty slot; the filled slots are ``0 ..
    min(M, seen) - 1``) is UPDATED IN PLACE with the shard's ``score`` / ``cells (Q, Vs)`` of ``prefilter_scores``; ``seen`` (a host
    int) is the global id of the shard's video 0.  Afterwards the filled slots hold the first ``min(M, seen + Vs)`` of all the videos
    seen in the order of ``search(prefilter=M)``'s cut: candidates (cells > 0) by higher score, ties to the lower video, then the
    non-candidates by ascending video.  Incumbents that stay keep their slots; the evicted and the empty slots, ascending, receive the
    admitted shard videos in ascending local index.  Returns ``copy_src (Q, M)`` int32 (written into the tensor given, if any): the
    local index of the video a slot must receive (``survivors_admit`` copies it), -1 to leave the slot alone.  HIP tensors only; one
    launch; no host synchronisation."""
    _require_hip(slot_score, "prefilter_fold")
    Q, M, Vs, n_old, _ = _fold_check("prefilter_fold", slot_score, slot_cells, slot_video, score, cells, seen)
    state = (slot_score, slot_cells, slot_video) + (() if copy_src is None else (copy_src,))
    if any(not s.is_contiguous() for s in state) or slot_score.dtype != torch.float32 or slot_cells.dtype != torch.float32 \
            or slot_video.dtype != torch.int32 or (copy_src is not None and (copy_src.dtype != torch.int32 or tuple(copy_src.shape) != (Q, M))):
        raise ValueError("prefilter_fold: the state is updated in place: contiguous float32 slot_score / slot_cells and int32 slot_video / "
                         "copy_src (Q, M)")
    dev = slot_score.device
    if copy_src is None:
        copy_src = torch.empty((Q, M), dtype=torch.int32, device=dev)
    s_, c_ = score.detach().float().contiguous(), cells.detach().float().contiguous()
    with torch.cuda.device(dev):
        call("smin_prefilter_fold", stream(), ptr(s_), ptr(c_), Q, Vs, M, int(seen), n_old, ptr(slot_score), ptr(slot_cells), ptr(slot_video),
             ptr(copy_src))
    return copy_src


def prefilter_fold_torch(slot_score, slot_cells, slot_video, score, cells, seen):
    """``prefilter_fold`` as plain Python on any device, out of place: ``(slot_score, slot_cells, slot_video, copy_src)`` after the shard,
    the scores in the dtype of ``slot_score``.  The tests' restatement, nothing routes here.  Reads the host."""
    Q, M, Vs, n_old, n_new = _fold_check("prefilter_fold_torch", slot_score, slot_cells, slot_video, score, cells, seen)
    seen = int(seen)
    out_s, out_c, out_v = slot_score.clone(), slot_cells.clone(), slot_video.clone()
    copy_src = torch.full((Q, M), -1, dtype=torch.int32, device=slot_score.device)
    os_, oc, ov, s, c = slot_score.tolist(), slot_cells.tolist(), slot_video.tolist(), score.tolist(), cells.tolist()
    # the order: candidates first, higher score first (-0 + 0 = +0), then the lower video; non-candidates by ascending video
    key = lambda sc, ce, vid: (0, -(sc + 0.0), vid) if ce > 0 else (1, 0.0, vid)
    for q in range(Q):
        union = [(key(os_[q][j], oc[q][j], ov[q][j]), 0, j) for j in range(n_old)] + [(key(s[q][v], c[q][v], seen + v), 1, v) for v in range(Vs)]
        first = sorted(union)[:n_new]
        stay = {j for _, new, j in first if not new}
        admitted = sorted(v for _, new, v in first if new)
        free = [j for j in range(n_new) if j >= n_old or j not in stay]
        for j, v in zip(free, admitted):
            out_s[q, j], out_c[q, j], out_v[q, j], copy_src[q, j] = score[q, v].to(out_s.dtype), cells[q, v].to(out_c.dtype), seen + v, v
        if n_new < M:
            out_s[q, n_new:], out_c[q, n_new:], out_v[q, n_new:] = 0, 0, -1
    return out_s, out_c, out_v, copy_src


_ADMIT_NAMES = ("fv", "video_mask", "length_mask", "moment_mask")


def _admit_check(what, copy_src, shard, out):
    if len(shard) != 4 or len(out) != 4:
        raise ValueError(f"{what}: shard and out are (fv, video_mask, length_mask, moment_mask)")
    fv, lm = shard[0], shard[2]
    if fv.dim() != 3 or fv.shape[0] < 1 or fv.shape[2] % 4 != 0 or fv.shape[2] < 4 or lm.dim() != 2:
        raise ValueError(f"{what}: the shard's fv must be (Vs, T, D) with Vs >= 1 and D % 4 == 0 and its length_mask (Vs, L); got "
                         f"{tuple(fv.shape)} and {tuple(lm.shape)}")
    Vs, T, D = fv.shape
    L, R = lm.shape[1], copy_src.numel()
    if R < 1 or R >= 2 ** 31:
        raise ValueError(f"{what}: copy_src must hold between 1 and 2**31 - 1 rows (got {R})")
    for name, src, dst, tail in zip(_ADMIT_NAMES, shard, out, ((T, D), (T,), (L,), (L, L))):
        n = int(np.prod(tail))
        if src.shape[0] != Vs or src.numel() != Vs * n or dst.numel() != R * n or src.dtype != dst.dtype:
            raise ValueError(f"{what}: {name} must hold {tail} per video, {Vs} videos in the shard and {R} rows in the survivors, in one "
                             f"dtype; got {tuple(src.shape)} {src.dtype} and {tuple(dst.shape)} {dst.dtype}")
    return R, Vs, T, L, D


def survivors_admit(copy_src, shard, out, scale=None, out_scale=None):
    """The payload of a fold (include/smin_hip.h, smin_survivors_admit): for every row r of ``copy_src`` (any shape, R elements, row ``q *
    M + slot``) with ``copy_src[r] >= 0``, row r of ``out`` -- the survivors' ``(fv (R, T, D), video_mask (R, T[, 1]), length_mask (R,
    L), moment_mask (R, L, L))``, updated IN PLACE -- becomes video ``copy_src[r]`` of ``shard``, the same four tensors of the
    shard's bank (float32 fv, one byte per mask entry), bit for bit.  Rows with -1 are not touched.  A compact bank (INTEGRATION.md
    3y) passes its codes as ``fv`` and, for int8 codes, ``scale (Vs, T)`` and the survivors' ``out_scale (R, T)``, which is copied
    with the rows (smin_survivors_admit_compact).  HIP tensors only; one launch; no host synchronisation."""
    _require_hip(copy_src, "survivors_admit")
    R, Vs, T, L, D = _admit_check("survivors_admit", copy_src, shard, out)
    storage = bank_storage("survivors_admit", shard[0], scale)
    if any(m.dtype not in (torch.bool, torch.uint8) for m in shard[1:]):
        raise ValueError("survivors_admit: float32 fv (or a compact bank's codes) and bool / uint8 masks (the banks' own)")
    if (scale is None) != (out_scale is None) or (scale is not None and (tuple(scale.shape) != (Vs, T) or tuple(out_scale.shape) != (R, T) or
                                                                         out_scale.dtype != torch.float32 or not out_scale.is_contiguous())):
        raise ValueError(f"survivors_admit: int8 codes come with scale (Vs, T) = {(Vs, T)} and a contiguous float32 out_scale (R, T) = {(R, T)}")
    if any(not t.is_contiguous() for t in out) or copy_src.dtype != torch.int32 or not copy_src.is_contiguous():
        raise ValueError("survivors_admit: the survivors are updated in place: contiguous tensors, and a contiguous int32 copy_src")
    src = [t.detach().contiguous() for t in shard]
    with torch.cuda.device(copy_src.device):
        if storage == "fp32":
            call("smin_survivors_admit", stream(), ptr(copy_src), *[ptr(t) for t in src], R, Vs, T, L, D, *[ptr(t) for t in out])
        else:
            sc = None if scale is None else scale.detach().contiguous()
            call("smin_survivors_admit_compact", stream(), ptr(copy_src), ptr(src[0]), ptr(sc), BANK_STORAGES[storage], *[ptr(t) for t in src[1:]],
                 R, Vs, T, L, D, ptr(out[0]), ptr(out_scale), *[ptr(t) for t in out[1:]])
    return out


def survivors_admit_torch(copy_src, shard, out):
    """``survivors_admit`` as plain torch ops on any device, out of place: the four tensors of ``out`` after the copy, each in its own
    dtype.  The tests' restatement, nothing routes here."""
    _admit_check("survivors_admit_torch", copy_src, shard, out)
    src = copy_src.reshape(-1).to(torch.int64)
    take = src >= 0
    res = []
    for s, d in zip(shard, out):
        rows = s.reshape(s.shape[0], -1)[src.clamp_min(0)]
        res.append(torch.where(take.unsqueeze(1), rows, d.reshape(src.shape[0], -1)).reshape(d.shape))
    return tuple(res)


def _gt_rank_check(what, score, cand, gt_video):
    if score.dim() != 2 or score.shape[0] < 1 or score.shape[1] < 1 or tuple(cand.shape) != (score.shape[1],):
        raise ValueError(f"{what}: score must be (Q, V) with Q, V >= 1 and cand (V,); got {tuple(score.shape)} and {tuple(cand.shape)}")
    Q, V = score.shape
    if V > 0x7fff0000:
        raise ValueError(f"{what}: {V} videos exceed the int32 video ids")
    if gt_video is not None and tuple(gt_video.shape) != (Q,):
        raise ValueError(f"{what}: gt_video must be (Q,) = ({Q},) (got {tuple(gt_video.shape)})")
    return Q, V


def prefilter_gt_rank(score, cand, gt_video=None):
    """The first-stage rank of each query's own video over the whole corpus (include/smin_hip.h, smin_prefilter_gt_rank): ``score (Q, V)``
    the first-stage scores of all the videos, ``cand (V,)`` nonzero where a video has a valid cell, ``gt_video (Q,)`` int tensor or
    None.  Returns ``gt_rank (Q,)`` int32: the number of candidates ahead of the query's own video (higher score, or an equal score and
    a lower video) -- ``prefilter_videos(...)["gt_rank"]`` on one bank of all the videos, in O(V) per query --; -1 without gt_video,
    for one out of range or for a non-candidate.  HIP tensors only; one launch; no host synchronisation."""
    _require_hip(score, "prefilter_gt_rank")
    Q, V = _gt_rank_check("prefilter_gt_rank", score, cand, gt_video)
    s_, c_ = score.detach().float().contiguous(), byte_mask(cand)
    gt = None if gt_video is None else gt_video.to(torch.int32).contiguous()
    out = torch.empty((Q,), dtype=torch.int32, device=score.device)
    with torch.cuda.device(score.device):
        call("smin_prefilter_gt_rank", stream(), ptr(s_), ptr(c_), ptr(gt), Q, V, ptr(out))
    return out


def prefilter_gt_rank_torch(score, cand, gt_video=None):
    """``prefilter_gt_rank`` as plain torch ops on any device, comparing in the dtype of ``score``: the tests' restatement."""
    Q, V = _gt_rank_check("prefilter_gt_rank_torch", score, cand, gt_video)
    dev = score.device
    if gt_video is None:
        return torch.full((Q,), -1, dtype=torch.int32, device=dev)
    gt = gt_video.to(torch.int64)
    inside = (gt >= 0) & (gt < V)
    g = torch.where(inside, gt, torch.zeros_like(gt)).unsqueeze(1)
    c = (cand != 0).unsqueeze(0)
    own = score.detach().gather(1, g)
    video = torch.arange(V, device=dev).unsqueeze(0)
    ahead = c & ((score.detach() > own) | ((score.detach() == own) & (video < g)))
    ok = inside & c.expand(Q, V).gather(1, g).squeeze(1)
    return torch.where(ok, ahead.sum(dim=1), torch.full_like(gt, -1)).to(torch.int32)


def search_times(video, idx, duration, L):
    """``times (Q, k, 2)`` of a ranked corpus list: top_moments' formula on each moment's own video, ``(i * duration[video] / L,
    (j + 1) * duration[video] / L)`` in fp32, NaN for empty slots.  ``duration``: the (V,) seconds of the videos ``video`` indexes.
    Formed without a constant from the host: the call reads and writes no host memory."""
    Q, k = video.shape
    d = duration.to(device=video.device, dtype=torch.float32)[video.clamp_min(0)].reshape(Q, k, 1)
    edge = idx.to(torch.float32)
    edge[..., 1] += 1.0
    t = edge * d / L
    return torch.where(idx >= 0, t, torch.full_like(t, float("nan")))


def window_times(video, span, duration, n_rows):
    """``times (Q, k, 2)`` of a ranked list of spans: ``(span * duration[video]) / n_rows[video]`` in fp32 -- localize_windows' formula
    on each entry's own video; the NaN span of an empty slot carries through.  ``duration`` / ``n_rows``: the (V,) seconds and row
    counts of the videos ``video`` indexes."""
    v = video.clamp_min(0)
    d = duration.to(device=v.device, dtype=torch.float32)[v].unsqueeze(-1)
    return (span * d) / n_rows.to(device=v.device, dtype=torch.float32)[v].unsqueeze(-1)


# ---------------------------------------------------------------- merge of ranked lists of disjoint video shards
MAX_LISTS = 16

# What a ranked list holds, described once: field -> (dtype, the shape behind (Q, k_s)), and ``count (Q,)``.  The kernels leave -1 in an
# empty slot's integers, 0 in its floats and the NaN 0x7FC00000 in its span.
_ENTRY = dict(video=(torch.int64, ()), idx=(torch.int64, (2,)), span=(torch.float32, (2,)), score=(torch.float32, ()), raw=(torch.float32, ()),
              window=(torch.int64, ()), cell=(torch.int64, (2,)), count=(torch.int32, None))


def _fields(*names):
    """A kind of entry: its fields beside video, name -> the shape behind (Q, k_s)."""
    return {name: _ENTRY[name][1] for name in names}


_SEARCH_FIELDS, _SPAN_FIELDS = _fields("idx", "score"), _fields("span", "score", "window", "cell")
_WEIGHTED_SEARCH_FIELDS, _WEIGHTED_SPAN_FIELDS = dict(_SEARCH_FIELDS, raw=()), dict(_SPAN_FIELDS, raw=())          # 

# The merge kernels (include/smin_hip.h): (span entries, weighted) -> the symbol, its per-list tables and its outputs in argument order
_MERGE_KERNELS = {
    (False, False): ("smin_search_merge", ("video", "idx", "score", "count"), ("video", "idx", "score", "count")),
    (True, False): ("smin_span_search_merge", _SPAN_KEYS, _SPAN_KEYS),
    (False, True): ("smin_search_merge_weighted", ("video", "idx", "raw", "count"), ("video", "idx", "score", "raw", "count")),
    (True, True): ("smin_span_search_merge_weighted", ("video", "span", "raw", "window", "cell", "count"),
                   ("video", "span", "score", "raw", "window", "cell", "count"))}


def _ranked_lists_check(what, results, video_offset, k, fields):
    """What the merges of ranked lists check alike, whatever an entry holds: the lists, their offsets and Q."""
    results = list(results)
    S = len(results)
    if not 1 <= S <= MAX_LISTS:
        raise ValueError(f"{what}: takes 1..{MAX_LISTS} ranked lists at a time (got {S}); fold longer sequences")
    if not (isinstance(k, int) and 1 <= k <= MAX_K):
        raise ValueError(f"{what} needs an integer 1 <= k <= {MAX_K} (got {k!r})")
    Q = results[0]["video"].shape[0] if results[0]["video"].dim() == 2 else -1
    for s, r in enumerate(results):
        v = r["video"]
        if v.dim() != 2 or v.shape[0] != Q:
            raise ValueError(f"{what}: every list's video must be (Q, k_s) with one Q = {Q} (list {s}: {tuple(v.shape)})")
        ks = v.shape[1]
        if not 1 <= ks <= MAX_K:
            raise ValueError(f"{what}: a list holds 1..{MAX_K} slots per query (list {s}: k = {ks})")
        if any(tuple(r[key].shape) != (Q, ks) + tail for key, tail in fields.items()) or tuple(r["count"].shape) != (Q,):
            raise ValueError(f"{what}: list {s} must hold " + ", ".join(f"{key} {(Q, ks) + tail}" for key, tail in fields.items()) +
                             f" and count {(Q,)}; got " + ", ".join(str(tuple(r[key].shape)) for key in list(fields) + ["count"]))
        if r["video"].device != results[0]["video"].device:
            raise ValueError(f"{what}: the lists must be on one device")
    off = [0] * S if video_offset is None else [int(x) for x in video_offset]
    if len(off) != S or min(off) < 0 or max(off) >= 2 ** 31:
        raise ValueError(f"{what}: video_offset must hold one offset in [0, 2**31) per list (got {off})")
    return results, off, Q


def _times_check(what, fields, duration, scale):
    """``times`` of a merged list need ``duration`` and ``scale``: L for entries of ``idx``, n_rows for entries of ``span``."""
    if "span" in fields:
        if (duration is None) != (scale is None):
            raise ValueError(f"{what}: times need both duration and n_rows, the global (V,) seconds and row counts of the videos")
    elif duration is not None and scale is None:
        raise ValueError(f"{what}: times need L, the number of clips per video, beside duration")


def _with_times(out, duration, scale):
    if duration is not None and "span" in out:
        out["times"] = window_times(out["video"], out["span"], torch.as_tensor(duration), torch.as_tensor(scale))
    elif duration is not None:
        out["times"] = search_times(out["video"], out["idx"], duration, scale)
    return out


def _launch_merge(what, results, off, Q, k, fields, weighted=()):
    """One launch of the merge kernel for entries of ``fields`` over checked lists (_MERGE_KERNELS); ``weighted``: the weighted kernels'
    arguments between the offsets and Q.  Returns the kernel's outputs by name."""
    for r in results:
        for key in ["video"] + list(fields) + ["count"]:
            _require_hip(r[key], what)
    dev, S = results[0]["video"].device, len(results)
    symbol, ins, outs = _MERGE_KERNELS["span" in fields, bool(weighted)]
    cols = [[r[key].detach().to(_ENTRY[key][0]).contiguous() for r in results] for key in ins]
    tables = [(ctypes.c_void_p * S)(*[t.data_ptr() for t in col]) for col in cols]
    k_list = (ctypes.c_int32 * S)(*[t.shape[1] for t in cols[0]])
    offsets = (ctypes.c_int64 * S)(*off)
    out = {key: torch.empty((Q,) if key == "count" else (Q, k) + _ENTRY[key][1], dtype=_ENTRY[key][0], device=dev) for key in outs}
    with torch.cuda.device(dev):
        call(symbol, stream(), S, *[ctypes.cast(t, ctypes.c_void_p) for t in tables], ctypes.cast(k_list, ctypes.c_void_p),
             ctypes.cast(offsets, ctypes.c_void_p), *weighted, Q, k, *[ptr(out[key]) if out[key].numel() else None for key in outs])
    return out


def _merge_lists_torch(results, off, Q, k, fields, value=None, keep=None):
    """The merges of ranked lists as plain torch + Python on any device: each query's candidates -- the first ``count[q]`` entries of
    every list, of those the ones ``keep[s] (Q, k_s)`` bool admits -- sorted by (value, global video, list, position), and the best k
    moved bit for bit: floats travel as int32 views, so a NaN keeps its payload and -0 its sign.  ``value[s] (Q, k_s)`` fp32 stands in
    for list s's score, in the order and in the output.  Empty slots hold the kernels' patterns (_ENTRY)."""
    dev = results[0]["video"].device
    per, base, moved = [], [0], {key: [] for key in ["video"] + list(fields)}
    for s, r in enumerate(results):
        ks = r["video"].shape[1]
        g = r["video"].to(torch.int64) + off[s]
        score = r["score"].detach().float() if value is None else value[s]
        per.append((_order_word(score).tolist(), g.tolist(), r["count"].to(torch.int64).clamp(0, ks).tolist(),
                    None if keep is None else keep[s].tolist()))
        base.append(base[-1] + ks)
        for key in moved:                                                                      # list after list, (Q, sum k_s)
            t = g if key == "video" else score if key == "score" else r[key].detach().to(_ENTRY[key][0])
            moved[key].append(t.contiguous().view(torch.int32) if t.dtype == torch.float32 else t)
    moved = {key: torch.cat(ts, dim=1) for key, ts in moved.items()}
    out = {}
    for key in moved:
        dtype, tail = _ENTRY[key]
        if dtype == torch.float32:
            out[key] = torch.full((Q, k) + tail, 0x7FC00000 if key == "span" else 0, dtype=torch.int32, device=dev).view(torch.float32)
        else:
            out[key] = torch.full((Q, k) + tail, -1, dtype=dtype, device=dev)
    out["count"] = torch.zeros((Q,), dtype=torch.int32, device=dev)
    for q in range(Q):
        cand = [(-o[q][p], g[q][p], s, p) for s, (o, g, cnt, ok) in enumerate(per) for p in range(cnt[q]) if ok is None or ok[q][p]]
        cand.sort()
        n = min(len(cand), k)
        if n:
            flat = torch.tensor([base[s] + p for _, _, s, p in cand[:n]], dtype=torch.int64, device=dev)
            for key, src in moved.items():
                dst = out[key].view(torch.int32) if out[key].dtype == torch.float32 else out[key]
                dst[q, :n] = src[q, flat]
        out["count"][q] = n
    return out


def _merge(what, results, video_offset, k, fields, duration, scale, restated=False):
    """The body of the plain merges: the checks, the kernel or its restatement, ``times``."""
    results, off, Q = _ranked_lists_check(what, results, video_offset, k, fields)
    _times_check(what, fields, duration, scale)
    out = _merge_lists_torch(results, off, Q, k, fields) if restated else _launch_merge(what, results, off, Q, k, fields)
    return _with_times(out, duration, scale)


def merge_search(results, video_offset=None, k=5, duration=None, L=None):
    """One ranked list per query out of 1..16 ``SMIN.search``-style lists, each over its own shard of the videos (include/smin_hip.h,
    smin_search_merge): one launch, one workgroup per query picks k times the best remaining candidate of all lists.

    ``results``: dicts with ``video (Q, k_s)`` int64, ``idx (Q, k_s, 2)`` int64, ``score (Q, k_s)`` and ``count (Q,)`` on one HIP device
    with one Q; ``video_offset``: host ints, list s's first global video (default all 0).  Order: higher score first (-0 counts as
    +0), ties -> lower global video, then lower list, then lower position.  Each list is assumed ordered as ``search`` orders it; then
    the merge of the lists of disjoint shards in ascending offset is, bit for bit, the list ``search`` / ``corpus_topk`` give on the
    whole corpus at equal pair scores, all at once or folded (``merge_search([carry, next], [0, seen])``).  No host synchronisation.

    Returns ``search``'s dict with global ids in ``video``; with ``duration`` (the global (V,) seconds) and ``L`` also ``times``."""
    return _merge("merge_search", results, video_offset, k, _SEARCH_FIELDS, duration, L)


def merge_search_torch(results, video_offset=None, k=5, duration=None, L=None):
    """``merge_search`` as plain torch + Python on any device (same result, bit for bit): each query's candidates sorted by
    (score, global video, list, position)."""
    return _merge("merge_search_torch", results, video_offset, k, _SEARCH_FIELDS, duration, L, restated=True)


def fold_search(lists, offsets, k, merge):
    """``merge`` (merge_search or merge_search_torch) over any number of lists in ascending offset: the first 16 at once, then the carry
    -- which holds global ids already, so its offset is 0 -- with the next 15, and so on; the same list as one merge of all
    (INTEGRATION.md 3n)."""
    carry = merge(lists[:MAX_LISTS], offsets[:MAX_LISTS], k=k)
    for r0 in range(MAX_LISTS, len(lists), MAX_LISTS - 1):
        carry = merge([carry] + list(lists[r0:r0 + MAX_LISTS - 1]), [0] + list(offsets[r0:r0 + MAX_LISTS - 1]), k=k)
    return carry


# ---------------------------------------------------------------- merge of span lists of sharded window banks
def merge_search_windows(results, video_offset=None, k=5, duration=None, n_rows=None):
    """One ranked list of span-valued moments per query out of 1..16 ``SMIN.search_windows``-style lists, each over its own shard of a
    corpus of long videos (include/smin_hip.h, smin_span_search_merge): one launch, one workgroup per query; each candidate finds its
    rank in the merge by a binary search over every other list and moves its fields there -- one pass, not k rounds.

    ``results``: dicts with ``video (Q, k_s)`` int64, ``span (Q, k_s, 2)`` fp32, ``score (Q, k_s)``, ``window (Q, k_s)`` int64,
    ``cell (Q, k_s, 2)`` int64 and ``count (Q,)`` on one HIP device with one Q (their ``times``, if any, are not read);
    ``video_offset``: host ints, list s's first global video (default all 0).  Order: merge_search's -- higher score first (-0 counts
    as +0), ties -> lower global video, then lower list, then lower position.  Each list is assumed ordered as ``search_windows``
    orders it; then the merge of the lists of shards of whole, disjoint videos in ascending offset is, bit for bit, the list
    ``search_windows`` / ``corpus_span_topk`` give on the whole corpus at equal pair scores, all at once or folded
    (``merge_search_windows([carry, next], [0, seen])``; any number of lists: ``fold_search``).  No host synchronisation.

    Returns ``search_windows``' dict with global ids in ``video``; with ``duration`` and ``n_rows`` (the global (V,) seconds and row
    counts) also ``times``, by ``window_times``."""
    return _merge("merge_search_windows", results, video_offset, k, _SPAN_FIELDS, duration, n_rows)


def merge_search_windows_torch(results, video_offset=None, k=5, duration=None, n_rows=None):
    """``merge_search_windows`` as plain torch + Python on any device (same result, bit for bit): each query's candidates sorted by
    (score, global video, list, position)."""
    return _merge("merge_search_windows_torch", results, video_offset, k, _SPAN_FIELDS, duration, n_rows, restated=True)


# ---------------------------------------------------------------- weighted merge of shard lists that carry their video scores
_CARRY_KEYS = ("raw", "pair_score", "pair_cells")


def carry_slots(k, k_video, max_videos=None):
    """The entries per query a carry list must hold for the k best of the whole corpus to survive a merge under ``max_videos`` = M:
    ``min(64, k + (M - 1) * k_video)``, and k without a cut.  A shard (or a carry) cuts its list by the best M of ITS videos; up to
    M - 1 of those are not among the corpus' best M, the corpus-wide ranking drops their entries -- at most ``k_video`` each -- and
    until then they occupy slots in front of entries that stay.  With that many slots (or with every entry of the shard's best M
    videos listed, which 64 slots may already do) no entry of the final k is pushed out."""
    if not (isinstance(k, int) and 1 <= k <= MAX_K and isinstance(k_video, int) and 1 <= k_video <= MAX_K):
        raise ValueError(f"carry_slots needs integers 1 <= k, k_video <= {MAX_K} (got {k!r}, {k_video!r})")
    if not max_videos:
        return k
    return min(MAX_K, k + (int(max_videos) - 1) * k_video)


_LIST_KEYS = ("video", "idx", "span", "score", "raw", "window", "cell", "times")


def truncate_search(result, k):
    """The first ``k`` entries per query of a ranked list (a search result or a carry): slices of its per-entry tensors, the count
    limited to k, everything else as it is.  A list is sorted, so this is the list its search or merge gives at ``k``.  No host read."""
    out = dict(result)
    for key in _LIST_KEYS:
        if key in out:
            out[key] = out[key][:, :k].contiguous()
    out["count"] = out["count"].clamp(max=k)
    return out


def _weighted_check(what, results, video_offset, k, fields, max_videos, n_videos):
    """The carry lists of a weighted merge, checked: ``(results, offsets, Q, V, max_videos or 0, n_videos)``.  Beside what every merge of
    ranked lists checks, each list must carry ``raw`` and its ``pair_score`` / ``pair_cells (Q, V_s)``, and the lists must tile the V global
    videos in ascending offset: offset 0 first, each next one the sum of the widths before it."""
    results = list(results)
    for s, r in enumerate(results):
        missing = [key for key in _CARRY_KEYS if key not in r]
        if missing:
            raise ValueError(f"{what}: list {s} carries no {' / '.join(missing)} -- search the shard with carry=True (a plain list cannot be "
                             "re-weighted against the other shards' videos)")
    results, off, Q = _ranked_lists_check(what, results, video_offset, k, fields)
    seen = 0
    for s, r in enumerate(results):
        ps, pc = r["pair_score"], r["pair_cells"]
        if ps.dim() != 2 or ps.shape[0] != Q or tuple(pc.shape) != tuple(ps.shape):
            raise ValueError(f"{what}: list {s}'s pair_score and pair_cells must be (Q, V_s) with Q = {Q} (got {tuple(ps.shape)}, {tuple(pc.shape)})")
        if off[s] != seen:
            raise ValueError(f"{what}: the lists must tile the videos in ascending offset -- list {s} covers {ps.shape[1]} videos and must "
                             f"start at {seen} (got offsets {off})")
        seen += ps.shape[1]
    if Q * seen > 0x7fff0000:
        raise ValueError(f"{what}: {Q} queries x {seen} videos exceed the int32 pair list of the video ranking")
    if not (max_videos is None or (isinstance(max_videos, int) and not isinstance(max_videos, bool) and 0 <= max_videos < 2 ** 31)):
        raise ValueError(f"{what}: max_videos must be None or an integer >= 0, 0 for no cut (got {max_videos!r})")
    cut = 0 if max_videos is None else max_videos
    n_videos = min(k, MAX_K) if n_videos is None else n_videos
    if not (isinstance(n_videos, int) and not isinstance(n_videos, bool) and 1 <= n_videos <= MAX_K):
        raise ValueError(f"{what}: n_videos must be an integer in [1, {MAX_K}] (got {n_videos!r})")
    return results, off, Q, seen, cut, n_videos


def _video_tables(results, Q, V, n_videos, alpha, gt_video, rank):
    """The shards' pooled scores side by side and ``rank`` (rank_videos or rank_videos_torch) over them: ``(pair_score (Q, V), pair_cells
    (Q, V), rank's dict)`` -- every query against every global video, ``pair_ptr[q] = q * V`` and ``pair_video = v``, so ``pair_rank`` and
    ``weight`` reshape to the (Q, V) tables of the merge.  ``gt_video``: None, a (Q,) int tensor or Q host ints (which travel in one
    pinned asynchronous copy)."""
    dev = results[0]["video"].device
    ps = torch.cat([r["pair_score"].detach().float() for r in results], dim=1)
    pc = torch.cat([r["pair_cells"].detach().float() for r in results], dim=1)
    pair_ptr = torch.arange(Q + 1, dtype=torch.int32, device=dev) * V
    pair_video = torch.arange(V, dtype=torch.int32, device=dev).repeat(Q)
    if gt_video is not None and not isinstance(gt_video, torch.Tensor):
        gt = torch.from_numpy(host_array(gt_video).astype(np.int32))
        gt_video = gt.pin_memory().to(dev, non_blocking=True) if dev.type == "cuda" else gt
    return ps, pc, rank(ps.reshape(-1), pc.reshape(-1), pair_video, pair_ptr, n=n_videos, alpha=alpha, gt_video=gt_video)


def _merge_weighted(what, results, off, Q, k, fields, rank_table, weight_table, V, cut):
    """One launch of smin_search_merge_weighted (``fields`` with ``idx``) or smin_span_search_merge_weighted over checked lists:
    ``rank_table`` / ``weight_table (Q, V)`` int32 / fp32 on the lists' device, ``cut`` <= 0 for no cut.  Returns the carry's entry keys."""
    rank_table, weight_table = rank_table.to(torch.int32).contiguous(), weight_table.detach().float().contiguous()
    return _launch_merge(what, results, off, Q, k, fields, (ptr(rank_table) if rank_table.numel() else None,
                                                            ptr(weight_table) if weight_table.numel() else None, V, cut))


def _merge_weighted_torch(results, off, Q, k, fields, rank_table, weight_table, V, cut):
    """``_merge_weighted`` as plain torch + Python on any device (same result, bit for bit): each query's surviving candidates sorted by
    (value, global video, list, position), the value ``raw * weight`` rounded once to fp32.  A candidate survives with a global video in
    [0, V) whose rank is neither below 0 nor, under a cut, at or behind it."""
    value, keep = [], []
    for s, r in enumerate(results):
        g = r["video"].to(torch.int64) + off[s]
        inside = (g >= 0) & (g < V)
        at = torch.where(inside, g, torch.zeros_like(g))
        w = torch.gather(weight_table.detach().float(), 1, at) if V else torch.zeros(g.shape, device=g.device)
        rank = torch.gather(rank_table.to(torch.int64), 1, at) if V else torch.full_like(g, -1)
        value.append(_mul32(r["raw"].detach().float(), w))
        keep.append(inside & (rank >= 0) & ((rank < cut) if cut > 0 else inside))
    return _merge_lists_torch(results, off, Q, k, fields, value, keep)


def _search_merge_weighted(what, results, video_offset, k, video_weight, max_videos, n_videos, gt_video, duration, scale, fields,
                           restated=False, tables=None):
    """The body of the four weighted merges: the checks, the shards' pooled scores side by side and one video ranking over them, the
    kernel (or, ``restated``, the torch ranking -- replaced by ``tables`` where given -- and the sort), ``times`` and the carry's keys."""
    alpha = _video_weight(what, video_weight)
    results, off, Q, V, cut, n_videos = _weighted_check(what, results, video_offset, k, fields, max_videos, n_videos)
    _times_check(what, fields, duration, scale)
    if not restated:
        for r in results:
            for key in ("video", "pair_score", "pair_cells"):
                _require_hip(r[key], what)
    ps, pc, vr = _video_tables(results, Q, V, n_videos, alpha, gt_video, rank_videos_torch if restated else rank_videos)
    rank_table, weight_table = (vr["pair_rank"], vr["weight"]) if tables is None else tables
    merge = _merge_weighted_torch if restated else functools.partial(_merge_weighted, what)
    out = _with_times(merge(results, off, Q, k, fields, rank_table.reshape(Q, V), weight_table.reshape(Q, V), V, cut), duration, scale)
    out.update(pair_score=ps, pair_cells=pc, video_rank=vr["video"], video_score=vr["score"], video_count=vr["count"], gt_rank=vr["gt_rank"])
    return out


def merge_search_weighted(results, video_offset=None, k=5, video_weight=0.0, max_videos=None, n_videos=None, gt_video=None, duration=None, L=None):
    """One ranked list per query out of 1..16 ``SMIN.search(..., carry=True)`` lists of disjoint video shards, ranked as
    ``search(video_weight=..., max_videos=...)`` ranks one bank of all their videos.  In order: the lists'
    ``pair_score`` / ``pair_cells (Q, V_s)`` side by side (one torch.cat each, ascending offset), one ``rank_videos`` over the V videos they
    cover -- the corpus-wide video rank and weight ``exp(video_weight * (s - the query's best s))`` --, and one launch of
    smin_search_merge_weighted (include/smin_hip.h): each candidate's value is its ``raw`` score times its video's weight, the videos
    behind the query's best ``max_videos`` drop out, and each survivor finds its rank by counting -- the lists need not be sorted in the
    new order.  Order: higher value first (-0 counts as +0), ties -> lower global video, then lower list, then lower position.

    ``results``: dicts with ``video (Q, k_s)`` int64, ``idx (Q, k_s, 2)`` int64, ``score``, ``raw (Q, k_s)``, ``count (Q,)`` and ``pair_score`` /
    ``pair_cells (Q, V_s)`` on one HIP device with one Q; ``video_offset``: host ints, list s's first global video; the lists must tile
    [0, V) in ascending offset with their widths V_s (ValueError otherwise, or for a list without ``raw`` / ``pair_score`` /
    ``pair_cells``).  ``gt_video``: Q host ints or a (Q,) int tensor of global ids, or None.  No host synchronisation.

    Returns a list of the same form over global ids -- ``video``, ``idx``, ``score`` (weighted), ``raw`` (moved bit for bit), ``count``,
    ``pair_score`` / ``pair_cells (Q, V)`` -- so it merges again at offset 0 (``merge_search_weighted([carry, next], [0, V], ...)``;
    ``fold_search`` with the options bound), plus ``video_rank (Q, n_videos)``, ``video_score``, ``video_count`` and ``gt_rank (Q,)`` of that
    one ``rank_videos``; with ``duration`` (the global (V,) seconds) and ``L`` also ``times``.  With the same options in every shard
    search and every merge, ``k_s >= k`` and -- under a cut -- ``carry_slots(k, k_video, max_videos)`` entries in every list that is
    merged again (the shard lists, and the carries of a fold, cut to k by ``truncate_search`` at the end), the result is, at equal pair
    scores and away from fp32 near-ties between a query's candidate values, bit for bit the one-bank search's; the carry costs
    ``Q * V * 8`` bytes and every merge re-ranks all V videos seen."""
    return _search_merge_weighted("merge_search_weighted", results, video_offset, k, video_weight, max_videos, n_videos, gt_video, duration, L,
                                  _WEIGHTED_SEARCH_FIELDS)


def merge_search_weighted_torch(results, video_offset=None, k=5, video_weight=0.0, max_videos=None, n_videos=None, gt_video=None, duration=None,
                                L=None, tables=None):
    """``merge_search_weighted`` as plain torch + Python on any device: the video ranking by ``rank_videos_torch`` -- or, with ``tables``
    = ``(pair_rank, weight)`` of shape (Q, V), the rank and weight tables it is given (the tests feed it the kernel's, whose expf is
    not torch's exp) --, then a Python sort on (value, global video, list, position).  Nothing routes here."""
    return _search_merge_weighted("merge_search_weighted_torch", results, video_offset, k, video_weight, max_videos, n_videos, gt_video, duration, L,
                                  _WEIGHTED_SEARCH_FIELDS, restated=True, tables=tables)


def merge_search_windows_weighted(results, video_offset=None, k=5, video_weight=0.0, max_videos=None, n_videos=None, gt_video=None, duration=None,
                                  n_rows=None):
    """``merge_search_weighted`` for ``SMIN.search_windows(..., carry=True)`` lists of shards of whole videos: the same cat, the same one
    ``rank_videos`` (the lists' ``pair_score`` / ``pair_cells`` are the groups' ``group_pool`` outputs) and one launch of
    smin_span_search_merge_weighted -- the same kernel body over entries of ``span``, ``window`` and ``cell``.  Returns the carry form
    with those fields, plus ``video_rank``, ``video_score``, ``video_count`` and ``gt_rank``; with ``duration`` and ``n_rows`` (the global
    (V,) seconds and row counts) also ``times``, by ``window_times``."""
    return _search_merge_weighted("merge_search_windows_weighted", results, video_offset, k, video_weight, max_videos, n_videos, gt_video, duration,
                                  n_rows, _WEIGHTED_SPAN_FIELDS)


def merge_search_windows_weighted_torch(results, video_offset=None, k=5, video_weight=0.0, max_videos=None, n_videos=None, gt_video=None,
                                        duration=None, n_rows=None, tables=None):
    """``merge_search_windows_weighted`` as plain torch + Python on any device; ``tables`` as ``merge_search_weighted_torch`` takes them.
    Nothing routes here."""
    return _search_merge_weighted("merge_search_windows_weighted_torch", results, video_offset, k, video_weight, max_videos, n_videos, gt_video,
                                  duration, n_rows, _WEIGHTED_SPAN_FIELDS, restated=True, tables=tables)
