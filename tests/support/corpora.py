"""The inputs the tests share: the tiny model, the ragged corpus and its pair lists, the window corpus of long videos, the shard
splitters, the rank-loss plans and probes, and the first-stage score's inputs.  Seeds and the order of draws are part of what the
tests' tolerances were measured on."""
import math

import numpy as np
import pytest
import torch

from tests import helpers as H
from tests.support.device import vml
from tests.support.compare import bits

TINY_SHAPE = (16, 8, 4, 32, 16, 2, 24, 5, 16)          # T, L, C, D, dl, layers, Din, Nq, H
# P = 9 over V = 5, Q = 4: video 0 and query 0 have three pairs, video 3 and query 3 none, pair (0, 1) is listed twice
VI9, QI9 = [0, 2, 0, 1, 4, 0, 2, 4, 2], [1, 0, 1, 2, 0, 2, 0, 1, 1]
GT_VIDEO = [2, 0, 3, 1]                                # queries 0 and 1 have their own video among VI9 / QI9's pairs (p = 1, 6 and 0, 2)


def tiny_model(dev=None):
    import models
    from oracle import smin_oracle as O
    sd = O.formula_state_dict(H.smin_shapes(*TINY_SHAPE), gain=1.2)
    m = models.SMIN(*TINY_SHAPE) if dev is None else models.SMIN(*TINY_SHAPE, dev)
    m.load_state_dict(sd, strict=True)
    return (m if dev is None else m.to(dev)), sd


def corpus_inputs(snips=(8, 1, 5, 8, 3), words=(5, 1, 3, 4), seed=3):
    """V ragged videos and Q queries as host tensors, and the queries' loss targets
    against their own videos GT_VIDEO."""
    T, L, _, _, _, _, Din, Nq, _ = TINY_SHAPE
    g = torch.Generator().manual_seed(seed)
    nv, nq = len(snips), len(words)
    vf, qf = torch.randn(nv, T, Din, generator=g), torch.randn(nq, Nq, 300, generator=g)
    vmask, qmask = torch.zeros(nv, T, 1, dtype=torch.uint8), torch.zeros(nq, Nq, 1, dtype=torch.uint8)
    lmask = torch.zeros(nv, L, dtype=torch.bool)
    for v, s in enumerate(snips):
        nf = s * (T // L) - (v % 2)                    # odd videos end inside their last snippet
        vf[v, nf:] = 0
        vmask[v, :nf] = 1
        lmask[v, :s] = True
    for q, w in enumerate(words):
        qf[q, w:] = 0
        qmask[q, :w] = 1
    mmask = torch.triu(lmask.unsqueeze(2) & lmask.unsqueeze(1))
    gt = torch.as_tensor(GT_VIDEO[:nq]) % nv
    sm = torch.rand(nq, L, L, generator=g) * mmask[gt]
    ss, se = torch.rand(nq, L, generator=g), torch.rand(nq, L, generator=g)
    tg = dict(sm=sm, ym=sm > 0.5, ss=ss, ys=ss > 0.5, se=se, ye=se > 0.5, ya=torch.rand(nq, L, generator=g) > 0.5)
    return dict(video_features=vf, video_mask=vmask, length_mask=lmask, moment_mask=mmask), dict(query_features=qf, query_mask=qmask), tg


def expand(vid, qry, vi, qi):
    """the six forward inputs of the pairs (vi[p], qi[p])"""
    vi, qi = torch.as_tensor(vi, dtype=torch.int64), torch.as_tensor(qi, dtype=torch.int64)
    vi, qi = vi.to(vid["video_features"].device), qi.to(vid["video_features"].device)
    return [vid["video_features"][vi], vid["video_mask"][vi], qry["query_features"][qi], qry["query_mask"][qi], vid["length_mask"][vi],
            vid["moment_mask"][vi]]


def pair_args(vid, qry):
    return [vid["video_features"], vid["video_mask"], qry["query_features"], qry["query_mask"], vid["length_mask"], vid["moment_mask"]]


def loss_of(fn, out, t):
    return fn(out[0], t["ym"], t["sm"], t["moment_mask"], out[1], t["ys"], t["ss"], out[2], t["ye"], t["se"], out[3], t["ya"], t["length_mask"])


def p19_lists():
    rng = np.random.RandomState(19)
    vi, qi = rng.randint(0, 5, 19), rng.randint(0, 4, 19)
    clash = (qi >= 2) & (vi == np.array(GT_VIDEO)[qi])
    vi[clash] = (vi[clash] + 1) % 5                    # queries 2 and 3 never meet their own videos ...
    vi[:2], qi[:2] = [2, 0], [0, 1]                    # ... queries 0 and 1 do
    return vi.tolist(), qi.tolist()


SCORE_TOL = 2e-5                                       # test_score_path.SCORE_TOL


def host_banks():
    vid, qry, _ = corpus_inputs()
    A = vml()
    counts = vid["moment_mask"].reshape(5, -1).sum(1).tolist()
    vb = A.VideoBank(None, vid["video_features"], vid["video_mask"], vid["length_mask"], vid["moment_mask"], counts)
    qb = A.QueryBank(None, None, qry["query_features"], qry["query_mask"].reshape(4, -1))
    return vb, qb


def pair_lists(nv, Q, kv, seed, full_query=None, empty_query=None):
    """top_moments-shaped lists of all Q * nv (query, video) pairs, query-major: scores randint(0, 6) / 8 sorted per pair (ties
    everywhere), random counts in [0, kv]; ``full_query``: every count kv, ``empty_query``: every count 0."""
    g = torch.Generator().manual_seed(seed)
    P = Q * nv
    score = (torch.randint(0, 6, (P, kv), generator=g).float() / 8).sort(dim=1, descending=True).values
    idx = torch.randint(0, 64, (P, kv, 2), generator=g, dtype=torch.int64)
    count = torch.randint(0, kv + 1, (P,), generator=g, dtype=torch.int32)
    if full_query is not None:
        count[full_query * nv:(full_query + 1) * nv] = kv
    if empty_query is not None:
        count[empty_query * nv:(empty_query + 1) * nv] = 0
    return score, idx, count


def cell_topk_of(lists, nv, Q, v0, v1, K):
    """corpus_topk_torch(k=K) of the videos v0 .. v1 of ``lists`` (pair_lists), numbered from 0 within the shard"""
    score, idx, count = lists
    rows = torch.tensor([q * nv + v for q in range(Q) for v in range(v0, v1)], dtype=torch.int64)
    video = torch.arange(v1 - v0, dtype=torch.int32).repeat(Q)
    ptr = torch.arange(Q + 1, dtype=torch.int32) * (v1 - v0)
    return vml().corpus_topk_torch(score[rows], idx[rows], count[rows], video, ptr, k=K)


def shards_of(lists, nv, Q, split, K):
    edges = np.concatenate([[0], np.cumsum(split)]).tolist()
    assert edges[-1] == nv
    return [cell_topk_of(lists, nv, Q, a, b, K) for a, b in zip(edges[:-1], edges[1:])], edges[:-1]


MARGIN = 2 * SCORE_TOL
T, L, DIN, NWORDS = TINY_SHAPE[0], TINY_SHAPE[1], TINY_SHAPE[6], TINY_SHAPE[7]
LENGTHS = (40, 16, 9, 0, 23)                           # window 16, stride 8: sampling.window_plan gives 4, 1, 1, 0, 2 windows
WINDOW, STRIDE = 16, 8
STARTS = [0, 8, 16, 24, 0, 0, 0, 7]
LENS = [16, 16, 16, 16, 16, 9, 16, 16]
VPTR = [0, 4, 5, 6, 6, 8]
WORDS = (5, 1, 3, 4)
NAN_BITS = 0x7FC00000


def corpus_rows(seed):
    """the videos' rows back to back and the four ragged queries, host tensors"""
    g = torch.Generator().manual_seed(seed)
    raw = torch.randn(sum(LENGTHS), DIN, generator=g)
    qf = torch.randn(len(WORDS), NWORDS, 300, generator=g)
    qm = torch.zeros(len(WORDS), NWORDS, 1, dtype=torch.uint8)
    for q, w in enumerate(WORDS):
        qf[q, w:] = 0
        qm[q, :w] = 1
    return raw, qf, qm


def host_masks(lens):
    nf = np.minimum(np.asarray(lens), T)
    n_len = np.ceil(nf / (T / L)).astype(np.int64)
    vmask = (torch.arange(T).unsqueeze(0) < torch.from_numpy(nf).unsqueeze(1)).to(torch.uint8).unsqueeze(2)
    lmask = torch.arange(L).unsqueeze(0) < torch.from_numpy(n_len).unsqueeze(1)
    mmask = torch.triu(lmask.unsqueeze(2) & lmask.unsqueeze(1))
    return vmask, lmask, mmask, [int(x * (x + 1) // 2) for x in n_len]


def window_host_banks():
    """a WindowBank of LENGTHS' windows and a QueryBank of four queries on the CPU, formed by hand (no encoder ran: fv is None)"""
    A = vml()
    vmask, lmask, mmask, cells = host_masks(LENS)
    i64 = lambda x: torch.tensor(x, dtype=torch.int64)
    wb = A.WindowBank(None, None, vmask, lmask, mmask, cells, STARTS, LENS, VPTR, LENGTHS, i64(STARTS), torch.tensor(LENS, dtype=torch.int32), i64(VPTR),
                      WINDOW, STRIDE)
    _, qf, qm = corpus_rows(0)
    return wb, A.QueryBank(None, None, qf, qm.reshape(len(WORDS), -1))


def random_span_lists(per_query, kv, seed, garbage):
    """merge_window_moments-shaped lists of sum(per_query) groups: scores from six values (both zeros among them), so ties are everywhere;
    counts in [0, kv]; distinct videos within a query; behind each count a NaN span, -1 and `garbage` as the score"""
    g = torch.Generator().manual_seed(seed)
    G2 = sum(per_query)
    values = torch.tensor([0.9, 0.5, 0.25, 0.0, -0.0, 1e-3])
    score = values[torch.randint(0, 6, (G2, kv), generator=g)]
    span = torch.rand(G2, kv, 2, generator=g) * 100
    window = torch.randint(0, 9, (G2, kv), generator=g, dtype=torch.int64)
    cell = torch.randint(0, 64, (G2, kv, 2), generator=g, dtype=torch.int64)
    count = torch.randint(0, kv + 1, (G2,), generator=g, dtype=torch.int32)
    if G2:
        count[0] = kv
    if G2 > 1:
        count[-1] = 0
    video = torch.cat([torch.randperm(max(n, 1) + 5, generator=g)[:n] for n in per_query]).to(torch.int32) if G2 else torch.zeros(0, dtype=torch.int32)
    ptr = torch.tensor(np.concatenate([[0], np.cumsum(per_query)]), dtype=torch.int32)
    unused = torch.arange(kv).unsqueeze(0) >= count.unsqueeze(1)
    score = torch.where(unused, torch.full_like(score, garbage), score)
    span = torch.where(unused.unsqueeze(2), torch.full_like(span, float("nan")), span)
    window = torch.where(unused, torch.full_like(window, -1), window)
    cell = torch.where(unused.unsqueeze(2), torch.full_like(cell, -1), cell)
    return span, score, window, cell, count, video, ptr


KEYS = ("video", "span", "score", "window", "cell", "count")


def same_lists(got, want, what=""):
    for key in KEYS:
        assert got[key].dtype == want[key].dtype and got[key].shape == want[key].shape, (what, key)
        assert torch.equal(got[key].cpu().contiguous().view(torch.uint8), want[key].cpu().contiguous().view(torch.uint8)), (what, key)


SEED = 3
KW = dict(k=5, k_video=3, k_window=3)
DURATION_TENSOR = torch.tensor([10.0, 3.5, 60.0, 7.25, 100.0])


def separated(score, count):
    """(Q, k) bool: the listed entries whose score differs from both neighbours in the list by more than MARGIN"""
    Q, k = score.shape
    listed = torch.arange(k).unsqueeze(0) < count.to(torch.int64).unsqueeze(1)
    gap = (score[:, :-1] - score[:, 1:]).abs() > MARGIN
    apart = torch.ones(Q, k, dtype=torch.bool)
    apart[:, 1:] &= gap | ~listed[:, 1:]
    apart[:, :-1] &= gap | ~listed[:, 1:]
    return apart & listed


def same_search(got, want, keys=("video", "window", "cell", "span")):
    """the comparison of lists whose scores come from differently composed batches: equal counts, sorted scores within MARGIN, and
    wherever the restatement's neighbouring scores differ by more than MARGIN the same entry, the span bit for bit"""
    got = {key: v.cpu() for key, v in got.items()}
    assert torch.equal(got["count"], want["count"])
    diff = (got["score"] - want["score"]).abs().max().item() if want["score"].numel() else 0.0
    assert diff < MARGIN, diff
    sep = separated(want["score"], want["count"])
    for key in keys:
        g, w = got[key], want[key]
        if key == "span":
            g, w = bits(g), bits(w)
        assert g.shape == w.shape and torch.equal(g[sep], w[sep]), key
    return sep, diff


DURATION = np.array([10.0, 3.5, 60.0, 7.25, 100.0])
SHARD_SPLITS = ([2, 3], [1, 1, 3])


def shard_dicts(raw, split, lengths=LENGTHS, duration=DURATION):
    ve = np.concatenate([[0], np.cumsum(split)])
    re_ = np.concatenate([[0], np.cumsum(lengths)])
    return [dict(raw=raw[re_[a]:re_[b]], lengths=list(lengths[a:b]), duration=duration[a:b]) for a, b in zip(ve[:-1], ve[1:])]


GT_TIMES = np.stack([np.array([1.0, 0.5, 2.0, 0.0]), np.array([6.0, 3.0, 30.0, 5.0])], axis=1)


def video_shards(vid_d, split, cell_counts):
    e = np.concatenate([[0], np.cumsum(split)])
    return [dict({k: v[a:b] for k, v in vid_d.items()}, duration=DURATION[a:b], cell_counts=cell_counts[a:b]) for a, b in zip(e[:-1], e[1:])]


SEARCH_KEYS = ("video", "idx", "score", "count")
NO_ROWS = (8, 1, 0, 8, 3)                               # corpus_inputs' snippets with a video without rows at an even index
SHAPES = [(4, 5, 16, 8, 4, 32), (5, 3, 20, 5, 3, 20), (44, 9, 16, 8, 4, 32), (3, 2, 64, 16, 4, 64)]      # Q, V, T, L, C, D
_INPUTS = {}


def inputs(shape, dev):
    """random fp32 banks and heads and ragged masks of a shape; video V // 2 has no valid cell.  Made once per shape, with the fp64
    restatement (maps included) at each tau computed on demand and kept."""
    if shape not in _INPUTS:
        _INPUTS[shape] = uncached_inputs(shape, dev)
    return _INPUTS[shape]


def uncached_inputs(shape, dev):
    """what ``inputs`` makes and keeps, made anew (a host test must not leave host tensors where the device tests look)"""
    Q, Vn, T, L, C, D = shape
    g = torch.Generator().manual_seed(sum(shape))
    fv, fs = torch.randn(Vn, T, D, generator=g), torch.randn(Q, D, generator=g)
    w, b = torch.randn(3, D, generator=g) / D ** 0.5, torch.randn(3, generator=g) / 2
    lens = torch.randint(1, L + 1, (Vn,), generator=g)
    lens[0], lens[Vn // 2] = L, 0
    lm = torch.arange(L).unsqueeze(0) < lens.unsqueeze(1)
    mm = torch.triu(lm.unsqueeze(2) & lm.unsqueeze(1))
    return dict(fv=fv.to(dev), fs=fs.to(dev), w=w.to(dev), b=b.to(dev), lm=lm.to(dev), mm=mm.to(dev), shape=shape, ref={})


PREFILTER_PRE = (20.0, 95.0, 110.0)


def saturated_prefilter(x, level):
    """A first-stage inputs dict (this module's ``inputs`` or tests/test_prefilter_train.py's) with banks and heads of rank one: every
    frame of video v is c_v (1 + d_k) / D over the features k (d_k = +-1/2 in turn, so a contraction still adds D different
    products), every feature of query q is k_q, the heads are all ones and the biases 0.  The three heads' pre-activations of the pair
    (q, v) are then c_v k_q at every cell and clip whose window mean weighs whole frames (T // L >= C).  c_0 = +1, the others -1.
    frozen: k_q runs through +-{20, 95, 110}; hard: through +20, -95 and three values inside +-4.  Returns a new dict."""
    Q, Vn, T, L, C, D = x["shape"]
    assert T // L >= C and D % 2 == 0
    dev = x["fv"].device
    c = -torch.ones(Vn)
    c[0] = 1.0
    k = torch.tensor([20.0, -95.0, 110.0, -20.0, 95.0, -110.0] if level == "frozen" else [20.0, -95.0, 1.5, -0.75, 3.0]).repeat(Q)[:Q]
    d = 1 + torch.tensor([0.5, -0.5]).repeat(D // 2)
    y = dict(x, fv=(c.view(Vn, 1, 1) * d / D).expand(Vn, T, D).contiguous().to(dev), fs=k.view(Q, 1).expand(Q, D).contiguous().to(dev),
             w=torch.ones(3, D, device=dev), b=torch.zeros(3, device=dev), ref={})
    return y, torch.outer(k, c)


def host_pairs(video):
    """the host (query, video) rows of prefilter_video (Q, Ms)"""
    v = video.cpu().numpy()
    return np.stack([np.repeat(np.arange(v.shape[0]), v.shape[1]), v.reshape(-1)], axis=1)


NV, NQ = 5, 4
FULL = (8, 8, 8, 8, 8)


def mined_arrays(Q=3, Vn=5, N=2, seed=11):
    """a mined layout from mine_pairs_torch on the CPU: the six arrays, the positive flags and gt_video"""
    g = torch.Generator().manual_seed(seed)
    score = torch.randn(Q, Vn, generator=g)
    gt = torch.randint(0, Vn, (Q,), generator=g).tolist()
    arrays = vml().mine_pairs_torch(score, gt, N)
    P = Q * (1 + N)
    positive = torch.tensor([int(p % (1 + N) == 0) for p in range(P)], dtype=torch.int32)
    return arrays, positive, gt, Vn, Q


def mined_plan(dev="cpu", **kw):
    arrays, positive, _, Vn, Q = mined_arrays(**kw)
    rows = torch.nonzero(positive).reshape(-1)
    return vml().PairPlan.from_device(*[a.to(dev) for a in arrays], Vn, Q, positive=positive.to(dev), positive_rows=rows.to(dev), num_positive=Q)


def plan_of(P, Q, dev="cpu"):
    """the plan of a (P, Q) case: the VI9 lists (query 1 has two positives, query 2 pairs but no positive, query 3 no pair), the
    P = 19 lists of p19_lists, or small hand-made lists"""
    api = vml()
    if (P, Q) == (9, 4):
        return api.PairPlan(VI9, QI9, NV, NQ, dev, gt_video=GT_VIDEO)
    if (P, Q) == (19, 4):
        vi, qi = p19_lists()
        return api.PairPlan(vi, qi, NV, NQ, dev, gt_video=GT_VIDEO)
    if (P, Q) == (1, 1):
        return api.PairPlan([0], [0], 1, 1, dev, gt_video=[0])
    if (P, Q) == (6, 2):
        return api.PairPlan([0, 0, 1, 1, 2, 2], [0, 1, 0, 1, 0, 1], 3, 2, dev, gt_video=[1, 2])
    if (P, Q) == (2, 1):
        return api.PairPlan([0, 1], [0, 0], 2, 1, dev, gt_video=[0])
    raise KeyError((P, Q))


def synthetic(P, L, seed, dtype=torch.float32):
    """uniform pm, ps, pe in [0, 1] with exact 0 forced into ps and pe and exact 0 and 1 into pm, ragged upper-triangular masks and,
    for P > 2, one pair without a valid cell (at P = 2 it would be the query's only negative, with s = 0: at gamma = 0.05 its softmax
    weight exp(-18) is below fp32's unit roundoff beside 1, every fp32 route gives loss 0 and zero gradients, and the case checks nothing)"""
    g = torch.Generator().manual_seed(seed)
    pm, ps, pe = torch.rand(P, L, L, generator=g), torch.rand(P, L, generator=g), torch.rand(P, L, generator=g)
    n = torch.randint(1, L + 1, (P,), generator=g)
    n[0] = L
    lm = torch.arange(L).unsqueeze(0) < n.unsqueeze(1)
    mm = torch.triu(lm.unsqueeze(2) & lm.unsqueeze(1))
    if P > 2:
        mm[P // 2] = False
    if P > 1:
        for p in range(P):
            last = int(n[p]) - 1
            if p % 3 == 0:
                ps[p, 0] = 0.0
            if p % 4 == 1:
                pe[p, last] = 0.0
            if p % 2 == 0:
                pm[p, 0, last] = 1.0
            if p % 3 == 1:
                pm[p, 0, 0] = 0.0
    return pm.to(dtype), ps.to(dtype), pe.to(dtype), mm


# d = (the segment's best score - the positives' best score) / gamma of the hard query -> (gamma, that difference): all dyadic, so the
# scores, their differences and the quotients by gamma are exact in fp32 and d is what the kernel sees
RANK_DEPTHS = {50: (2.0 ** -7, 50 / 128), 95: (2.0 ** -8, 95 / 256), 120: (2.0 ** -8, 120 / 256), 800: (2.0 ** -11, 800 / 2048)}
RANK_BEST = 0.875


def saturated_pairs(d, dtype=torch.float32):
    """Constant maps with ps = pe = 1 over plan_of(6, 2) at L = 4 (segments [0, 2, 4] and [1, 3, 5], the positives p = 2 and p = 5): every
    valid cell of pair p holds c_p, so the pooled score s_p is c_p exactly at any tau.  Query 0's own video is its best pair (0.875 over
    0.5 and 0.25); query 1's own video lies d * gamma below its best negative (0.875), a second negative 0.125 below that.  Returns
    ((pm, ps, pe, mm), gamma, c)."""
    gamma, gap = RANK_DEPTHS[d]
    c = [0.5, RANK_BEST, RANK_BEST, RANK_BEST - 0.125, 0.25, RANK_BEST - gap]
    L = 4
    mm = torch.triu(torch.ones(L, L, dtype=torch.bool)).repeat(len(c), 1, 1)
    pm = torch.tensor(c, dtype=torch.float64).reshape(-1, 1, 1).expand(len(c), L, L).contiguous()
    assert torch.equal(pm.float().double(), pm)                                  # fp32 holds every constant
    return (pm.to(dtype), torch.ones(len(c), L, dtype=dtype), torch.ones(len(c), L, dtype=dtype), mm), gamma, c


def saturated_teacher(dtype=torch.float32):
    """a teacher over saturated_pairs' plan that puts each query's own video first: it agrees with the student on query 0 and, on
    query 1, prefers the pair the student ranks last"""
    return torch.tensor([0.5, 0.25, RANK_BEST, 0.625, 0.25, RANK_BEST], dtype=dtype)


def stable_rank_loss(c, segments, positives, gamma):
    """The contrastive loss' definition on given pair scores in Python floats (fp64), stable form: the mean over the queries of
    logsumexp(s / gamma) over the segment minus the same over its positives, and d(loss)/d(s_p).  Returns (loss, [coef_p])."""
    def lse(v):
        top = max(v)
        return top + math.log(sum(math.exp(x - top) for x in v))
    total, coef = 0.0, [0.0] * len(c)
    for seg, pos in zip(segments, positives):
        za, zp = lse([c[p] / gamma for p in seg]), lse([c[p] / gamma for p in pos])
        total += za - zp
        for p in seg:
            coef[p] += (math.exp(c[p] / gamma - za) - (math.exp(c[p] / gamma - zp) if p in pos else 0.0)) / gamma
    n = len(segments)
    return total / n, [v / n for v in coef]


def tied_maps(P, L, seed, dtype=torch.float32):
    """synthetic's masks under maps of eighths with ps = pe = 1, pair p capped at 1 - (p % 4) / 8: a pair's fused scores are multiples of
    1/8, several cells may share the maximum, neighbouring pairs have different maxima, and at tau <= 1e-3 every other cell lies at
    least 125 temperatures below its pair's maximum"""
    pm, ps, pe, mm = synthetic(P, L, seed, dtype=torch.float64)
    cap = 1.0 - (torch.arange(P, dtype=torch.float64) % 4) / 8
    pm = torch.minimum(torch.round(pm * 8) / 8, cap.reshape(P, 1, 1))
    return pm.to(dtype), torch.ones_like(ps).to(dtype), torch.ones_like(pe).to(dtype), mm


def tied_pool_by_hand(pm, mm, tau):
    """m + tau * log(k / n) per pair of tied_maps, k the number of valid cells at the maximum m of its n valid cells (0 without one), in
    Python floats; also the lists of m, k and n"""
    score, top, ties, cells = [], [], [], []
    for p in range(pm.shape[0]):
        vals = pm[p][mm[p]].tolist()
        m = max(vals) if vals else 0.0
        k = sum(v == m for v in vals)
        score.append(m + tau * math.log(k / len(vals)) if vals else 0.0)
        top.append(m), ties.append(k), cells.append(len(vals))
    return score, top, ties, cells


def on(dev, d):
    return {k: v.to(dev) for k, v in d.items()}


@pytest.fixture(scope="module")
def world(dev):
    m, sd = tiny_model(dev)
    vid, qry, tg = corpus_inputs()
    return dict(m=m, sd=sd, vid=vid, qry=qry, tg=tg, vid_d=on(dev, vid), qry_d=on(dev, qry), tg_d=on(dev, tg))


def full_group(dev, seed=3, lists=True):
    vid, qry, tg = corpus_inputs(snips=FULL, seed=seed)
    g = dict(**on(dev, vid), **on(dev, qry), **on(dev, tg), gt_video=GT_VIDEO, cell_counts=[36] * NV)
    if lists:
        g.update(video_index=VI9, query_index=QI9)
    return g


def probe(api):
    class Probe(api.EpochMeter):
        reads = 0

        def result(self, group=None):
            Probe.reads += 1
            torch.cuda.set_sync_debug_mode("default")
            return super().result(group)
    return Probe


def checked(fn):
    torch.cuda.synchronize()
    mode = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        return fn()
    finally:
        torch.cuda.set_sync_debug_mode(mode)


def hand_step(api, model, g, plan, weight, opt=None):
    """the parent's _pair_step by hand, plus weight * pair_rank_loss when weight is not None; returns the loss"""
    if opt is not None:
        opt.zero_grad()
    out = model.forward_pairs(*[g[k] for k in api.training.MODEL_INPUTS], None, None, cell_counts=g["cell_counts"], plan=plan)
    t = api.pair_targets(g, g, None, None, None, plan=plan)
    loss = loss_of(api.loss_fn, out, t)
    if weight is not None:
        loss = loss + weight * api.pair_rank_loss(out[0], out[1], out[2], t["moment_mask"], plan)
    if opt is not None:
        loss.backward()
        opt.step()
    return loss


def same_parameters(a, b):
    for (k, p), (_, r) in zip(a.named_parameters(), b.named_parameters()):
        assert torch.equal(bits(p), bits(r)), k


def build_model(cfg, sd, dev):
    import models
    m = models.SMIN(cfg["T"], cfg["L"], cfg["C"], cfg["D"], cfg["dl"], cfg["layers"], cfg["Din"], cfg["Nq"], cfg["H"], dev)
    missing = m.load_state_dict(sd, strict=True)
    assert not missing.missing_keys and not missing.unexpected_keys
    return m.to(dev)


# rows that send the one-node extension path into attention-core forms no other model-level case reaches
# (form <DL,WS,EXACT> as SMIN_ATTN_DISPATCH in csrc/content_attn.hip picks it)
NATIVE_ROWS = [
    (64, 16, 4, 128, 64, 2, 40, 9, 64, 3),       # <64,4,T>
    (32, 16, 4, 64, 32, 1, 24, 17, 32, 5),       # <32,8,T>, extra-word slots partly used
    (32, 8, 4, 64, 16, 2, 24, 32, 32, 2),        # <16,8,T>
    (64, 16, 4, 256, 128, 2, 40, 23, 128, 3),    # <128,6,T>
    (32, 8, 4, 192, 128, 2, 24, 29, 96, 4),      # <128,8,T>; parameter products in csrc/param_prep.hip
    (64, 16, 4, 104, 48, 2, 24, 18, 52, 3),      # <64,8,F> with dl < DL; torch parameter prep (D % 32 != 0)
]


def one_node_only(m):
    """Fail the step if it leaves the one-node path (the Python host's content stream would run)."""
    def python_host(*a):
        raise AssertionError("the step ran the Python host")
    m._forward_stream = python_host


def loss_of_batch(out, b, oracle=False):
    from oracle import smin_oracle as O
    from vml_amd import loss_fn
    return (O.loss_fn if oracle else loss_fn)(out[0], b["ym"], b["sm"], b["moment_mask"], out[1], b["ys"], b["ss"], out[2], b["ye"], b["se"], out[3], b["ya"],
                                             b["length_mask"])
