"""Retrieval on top of SMIN's scores, which the reference does not have: the best moments of a sample (``localize``), of videos of
any length over overlapping windows (``localize_windows``) and of a corpus encoded once (``encode_videos`` / ``encode_queries`` ->
``score_pairs`` / ``search``, pruned by a first-stage score from the banks alone with ``prefilter_videos`` / ``search(prefilter=M)`` and, for a corpus that comes in
shards, ``new_survivors`` / ``fold_survivors`` / ``search_survivors``; a corpus
of videos of any length: ``encode_windows`` -> ``search_windows``, pruned the same way with ``search_windows(prefilter=M)``), and the training counterpart
of ``score_pairs``, ``forward_pairs`` over (video, query) pairs that share their
encoders: host code around the library's kernels and the model's own ``score`` / ``forward``, which ``modules.SMIN`` inherits
through the stateless mixin ``_Retrieval``."""
import copy

import numpy as np
import torch

from . import _lib
from ._host import _AttnMaps, byte_mask, host_array, known_cells, query_mask_rows, require_hip_tensors, require_ints
from .feeder import build_masks_hip, cell_count
from .functional import attn_maps_gather
from .moments import (MAX_K, PREFILTER_FOLD_MAX_M, bank_decode, bank_encode, bank_storage, require_storage, prefilter_fold, prefilter_gt_rank, survivors_admit, _pair_pool_into, _temperature, _select_into, soft_rule, _video_weight, corpus_span_topk, corpus_span_topk_torch, corpus_topk,
                      corpus_topk_torch, group_pool, merge_window_moments, merge_window_moments_torch, mine_pairs, prefilter_maps, prefilter_scores, prefilter_select,
                      rank_videos, reweight_moments, expand_survivor_windows, survivor_window_capacity,
                      reweight_moments_torch, search_times, top_moments, top_moments_torch, window_times)
from .sampling import MAX_ROWS, MODES, sample_windows, window_plan


def _carry_raw(video, listed, lists, score, count, V):
    """``raw (Q, k)`` of a ranked list over every (query, video) of a bank of V videos: the unweighted score of each listed entry, taken
    from its pair's own list (pair q * V + video) at the slot whose integer fields match -- ``listed``: the entry's fields ``(Q, k, n)``,
    ``lists``: the pairs' ``(P, k_video, n)``, ``score (P, k_video)`` / ``count (P,)`` the pairs' lists before any weight.  A gather: the
    bits leave as they came; 0 for an empty slot.  A few torch ops, no host read."""
    Q, kv = video.shape[0], score.shape[1]
    pair = torch.arange(Q, device=video.device).unsqueeze(1) * V + video.clamp_min(0)                   # (Q, k)
    match = torch.arange(kv, device=video.device) < count.to(torch.int64).clamp(0, kv)[pair].unsqueeze(-1)
    for mine, theirs in zip(listed, lists):
        match = match & (theirs[pair] == mine.unsqueeze(2)).all(dim=-1)                                   # (Q, k, k_video)
    slot = match.to(torch.int8).argmax(dim=-1, keepdim=True)
    raw = score.detach().float()[pair].gather(-1, slot).squeeze(-1)
    return torch.where((video >= 0) & match.any(dim=-1), raw, torch.zeros_like(raw))


class VideoBank:
    """V videos encoded once (SMIN.encode_videos): ``fv (V, T, D)``, the video encoder's projection with position embedding and mask --
    everything of a video the model computes before the video meets a query (f = fv * fs, reference models.py:81) --, the videos'
    ``video_mask``, ``length_mask`` and ``moment_mask`` and ``cell_counts``, each video's number of valid cells as host ints (what
    lets SMIN.search hand every chunk's ``known_cell_count`` to the scorer without a device read).  ``video_features`` is the input
    itself (not a copy), kept for the configurations that score through SMIN.score.

    A bank is detached and is a snapshot of the parameters at the time of the call: a parameter update (an optimizer step,
    load_state_dict) makes it stale -- encode again.  ``fv`` is None when the call would not take the one-node path (SMIN._plan).

    Compact storage: ``storage`` is ``"fp32"`` (the default), ``"bf16"`` or ``"int8"``.  A compact bank's ``fv`` holds
    the codes themselves -- torch.bfloat16, or torch.int8 with ``fv_scale (V, T)`` float32, one scale per frame (None otherwise) --, so
    a path that was not told about codes fails on a dtype check instead of reading them as floats.  ``compact(storage)`` encodes an
    fp32 bank (moments.bank_encode), ``dequantized()`` gives the fp32 bank of the decoded values (moments.bank_decode); both keep
    every other field.  Scoring, search and the first stage read the codes directly and give the bits of ``dequantized()``.
    ``nbytes``: the bytes of ``fv`` and ``fv_scale``."""

    def __init__(self, fv, video_features, video_mask, length_mask, moment_mask, cell_counts, fv_scale=None):
        self.fv, self.video_features, self.video_mask, self.length_mask, self.moment_mask = fv, video_features, video_mask, length_mask, moment_mask
        self.cell_counts = tuple(int(c) for c in cell_counts)
        self.fv_scale = fv_scale
        if fv is not None:
            bank_storage("VideoBank", fv, fv_scale)

    @property
    def storage(self):
        return "fp32" if self.fv is None else bank_storage("VideoBank", self.fv, self.fv_scale)

    @property
    def nbytes(self):
        """The bytes the bank's ``fv`` (codes) and ``fv_scale`` hold; 0 without ``fv``."""
        return sum(t.numel() * t.element_size() for t in (self.fv, self.fv_scale) if t is not None)

    def _with_fv(self, fv, fv_scale):
        bank = copy.copy(self)                                    # every other field, a WindowBank's plan included
        bank.fv, bank.fv_scale = fv, fv_scale
        return bank

    def compact(self, storage):
        """The bank in ``storage``: the bank itself where it is held so already, else an fp32 bank encoded by moments.bank_encode (one
        launch).  ValueError for an unknown storage, a bank without ``fv`` (encoded off the one-node path) or a compact bank asked for
        another code (go through ``dequantized()``: a second rounding is a decision)."""
        require_storage("compact", storage)
        if self.fv is None:
            if storage == "fp32":
                return self
            raise ValueError("compact: a compact storage holds fv, which a bank encoded off the one-node path (SMIN._plan) does not have")
        if storage == self.storage:
            return self
        if self.storage != "fp32":
            raise ValueError(f"compact: the bank is held as {self.storage}; dequantized() gives the fp32 bank to encode again")
        return self._with_fv(*bank_encode(self.fv, storage))

    def dequantized(self):
        """An fp32 bank of the decoded values (moments.bank_decode); an fp32 bank is returned as it is."""
        if self.storage == "fp32":
            return self
        return self._with_fv(bank_decode(self.fv, self.fv_scale), None)

    def __len__(self):
        return (self.video_mask if self.video_features is None else self.video_features).shape[0]

    @property
    def device(self):
        return self.video_mask.device

    @property
    def plan_features(self):
        """What SMIN._plan reads of the bank's features (dtype, T, no gradient): the features themselves where the bank keeps them."""
        return self.video_features

    @property
    def cell_count(self):
        """Every video's valid-cell count where all ``cell_counts`` are one value, else None."""
        return self.cell_counts[0] if len(set(self.cell_counts)) == 1 else None


class WindowBank(VideoBank):
    """The W windows of V videos of any length, encoded once (SMIN.encode_windows): a VideoBank whose rows are the
    windows in global window order (video, then start) -- ``fv (W, T, D)``, the three masks and ``cell_counts`` per window --, and the
    plan they came from: ``start (W,)`` int64 and ``len (W,)`` int32 on the device (each window's first raw row relative to its video
    and its row count), ``video_ptr (V + 1,)`` on the host (numpy int64) and ``video_ptr_d`` on the device (int64) -- video v owns
    windows ``video_ptr[v] .. video_ptr[v + 1]`` --, ``n_rows (V,)`` the videos' row counts and ``starts`` / ``lens (W,)`` (host, numpy
    int64), ``window``, ``stride`` and ``mode``.  ``len(bank)`` is W; ``n_videos`` is V.

    ``video_features`` is None on the one-node path: the sampled ``(W, T, Din)`` features are several times ``fv``'s size (Din against
    D) and nothing reads them there; ``plan_features`` then is an empty ``(0, T, Din)`` tensor of their dtype and device.  They are kept
    only where pairs are scored through SMIN.score on expanded pairs (off the one-node path, keep_attention).  A snapshot of the
    parameters, as every bank."""

    def __init__(self, fv, video_features, video_mask, length_mask, moment_mask, cell_counts, starts, lens, video_ptr, n_rows, start, len,
                 video_ptr_d, window, stride, mode="pick", plan_features=None, fv_scale=None):
        super().__init__(fv, video_features, video_mask, length_mask, moment_mask, cell_counts, fv_scale)
        self.starts, self.lens, self.video_ptr, self.n_rows = (host_array(x) for x in (starts, lens, video_ptr, n_rows))     # host values
        self.start, self.len, self.video_ptr_d = start, len, video_ptr_d                                                    # their device copies
        self.window, self.stride, self.mode = int(window), int(stride), mode
        self.n_videos = self.n_rows.shape[0]
        self._plan_features = plan_features

    @property
    def plan_features(self):
        return self._plan_features if self.video_features is None else self.video_features


class SurvivorBank(VideoBank):
    """The running first-stage cut of a corpus that comes in shards (SMIN.new_survivors / fold_survivors / search_survivors;
    INTEGRATION.md 3x): for each of Q queries the best M videos seen so far by the first-stage score, WITH what the full model needs of
    them -- a VideoBank of ``Q * M`` rows, row ``q * M + slot``: ``fv (Q M, T, D)`` and the three masks, copied from each shard's bank
    before it is dropped.  A video kept by several queries is stored once per query.  The rows are allocated by the first fold (they
    take the shard bank's shapes and mask dtypes); before it ``fv`` and the masks are None.

    Beside the rows: the slot state of smin_prefilter_fold -- ``slot_score`` / ``slot_cells (Q, M)`` float32, ``slot_video (Q, M)``
    int32 (the global video id in shard order, -1 for an empty slot; the filled slots are ``0 .. min(M, seen) - 1``) and ``copy_src (Q,
    M)``, the last fold's --, ``tau``, ``seen`` (the videos folded so far, a host int), the kept first-stage scores ``score (Q, seen)``
    and the candidate flags ``candidate (seen,)`` (a video with a valid cell), both concatenated from the shards on demand.
    ``cell_count`` is every video's valid-cell count where all the shards' ``cell_counts`` were one value, else None.
    ``video_features`` is None and ``plan_features`` an empty ``(0, T, Din)`` tensor, as WindowBank gives on the one-node path.

    Memory: ``Q * M * (T * D * esize [+ 4 T] + T + L + L * L)`` bytes of rows (esize 4, 2 or 1 by the storage, which is the first
    shard's; the 4 T are an int8 bank's scales), fixed by (Q, M), plus ``4 * Q * V`` bytes of kept scores (and V flag
    bytes) -- the only part that grows with the corpus.  A snapshot of the parameters, as every bank."""

    def __init__(self, Q, M, tau, device, plan_features):
        super().__init__(None, None, None, None, None, ())
        self.Q, self.M, self.tau, self.seen = int(Q), int(M), tau, 0
        self._device, self._plan_features = torch.device(device), plan_features
        self.slot_score = torch.zeros((Q, M), dtype=torch.float32, device=device)
        self.slot_cells = torch.zeros((Q, M), dtype=torch.float32, device=device)
        self.slot_video = torch.full((Q, M), -1, dtype=torch.int32, device=device)
        self.copy_src = torch.full((Q, M), -1, dtype=torch.int32, device=device)
        self.shard_scores, self.shard_candidates, self.cell_values = [], [], set()

    def __len__(self):
        return self.Q * self.M

    @property
    def device(self):
        return self._device

    @property
    def plan_features(self):
        return self._plan_features

    @property
    def score(self):
        return torch.cat(self.shard_scores, dim=1)

    @property
    def candidate(self):
        return torch.cat(self.shard_candidates)

    @property
    def cell_count(self):
        return next(iter(self.cell_values)) if len(self.cell_values) == 1 else None


class QueryBank:
    """Q queries encoded once (SMIN.encode_queries): the query encoder's word features ``fw (Q, max_query_length, D)`` and sentence
    features ``fs (Q, D)``, and ``query_mask (Q, max_query_length)`` padded as the kernels read it.  ``query_features`` is the input
    itself, kept for the configurations that score through SMIN.score.  Detached; stale after a parameter update, as VideoBank."""

    def __init__(self, fw, fs, query_features, query_mask):
        self.fw, self.fs, self.query_features, self.query_mask = fw, fs, query_features, query_mask

    def __len__(self):
        return self.query_features.shape[0]


def _require_banks(what, videos, queries):
    if not isinstance(videos, VideoBank) or not isinstance(queries, QueryBank):
        raise TypeError(f"{what}: videos is a VideoBank (encode_videos) and queries a QueryBank (encode_queries)")


def _require_node_banks(videos, queries):
    """ValueError for a bank without the one-node path's encodings (encode_queries leaves ``fw`` and ``fs`` together)."""
    if videos.fv is None or queries.fw is None or queries.fs is None:
        raise ValueError("score_pairs: a bank was encoded while the module was off the one-node path (SMIN._plan); encode it again")


def _upload(parts, dtype, dev):
    """Host arrays as views of ONE buffer of ``dtype`` on ``dev``: a pinned asynchronous copy, so the call never waits for the device
    (a plain tensor on the CPU)."""
    host = torch.from_numpy(np.concatenate(parts).astype(dtype))
    buf = host.pin_memory().to(dev, non_blocking=True) if torch.device(dev).type == "cuda" else host
    return buf.split([a.shape[0] for a in parts])


class _Options:
    """The checked options of a search, as one value: ``k``, ``k_video`` and ``k_window`` with their defaults filled in; after
    ``video_level`` the options of INTEGRATION.md 3t -- ``ranked`` True, ``alpha``, ``max_videos`` (None: no cut), ``tau``, ``n_videos`` --;
    ``gt``, each query's own video as Q host ints (empty: none given).  Every check of these has its one source here; an entry point
    runs them in the order its errors have always come in.  ValueError for a bad value."""
    ranked, gt = False, np.zeros(0, np.int64)

    def __init__(self, what, k=1, k_video=None, max_batch=1, k_window=None, windows=False):
        k_video = k if k_video is None else k_video
        k_window = k_video if k_window is None else k_window
        require_ints(what, ("k", k, 1, MAX_K), ("k_video", k_video, 1, MAX_K), *([("k_window", k_window, 1, MAX_K)] if windows else []),
                     ("max_batch", max_batch, 1, 65535))
        self.what, self.k, self.k_video, self.k_window = what, int(k), int(k_video), int(k_window) if windows else None

    def duration(self, duration, V):
        if duration is not None and tuple(duration.shape) != (V,):
            raise ValueError(f"{self.what}: duration must be (V,) = ({V},) seconds (got {tuple(duration.shape)})")

    def gt_video(self, gt_video, Q):
        if gt_video is not None:
            self.gt = host_array(gt_video)
            if self.gt.shape[0] != Q:
                raise ValueError(f"{self.what}: gt_video must name a video for each of the Q = {Q} queries (got {self.gt.shape[0]})")
        return self

    def video_level(self, video_weight, max_videos, tau, n_videos, gt_video, Q):
        self.alpha = _video_weight(self.what, 0.0 if video_weight is None else video_weight)
        if max_videos is not None:
            require_ints(self.what, ("max_videos", max_videos, 1, 2 ** 31 - 1))
        n_videos = min(self.k, MAX_K) if n_videos is None else n_videos
        require_ints(self.what, ("n_videos", n_videos, 1, MAX_K))
        self.gt_video(gt_video, Q)
        self.max_videos, self.n_videos = None if max_videos is None else int(max_videos), int(n_videos)
        self.ranked, self.tau = True, _temperature(self.what, tau)
        return self


class PairPlan:
    """The index lists of P (video, query) pairs over V videos and Q queries as forward_pairs and training.pair_targets read them:
    the checked host lists ``vi`` / ``qi`` (int64 numpy) and, on ``device`` as int32, ``video_index`` / ``query_index (P,)`` and the
    same pairs grouped by video -- ``v_ptr (V + 1,)``, ``v_pairs (P,)`` -- and by query -- ``q_ptr (Q + 1,)``, ``q_pairs (P,)`` --,
    each segment in ascending p (smin_pair_assemble_bwd sums in that order).  With ``gt_video`` (Q host ints, each query's own video)
    also ``positive (P,)`` int32, 1 where ``video_index[p] == gt_video[query_index[p]]``, and ``positive_rows``, the ordinals of
    those pairs (int64).  Everything is formed on the host and travels in ONE pinned asynchronous copy (a plain copy on the CPU).

    ``PairPlan.from_device`` wraps the same arrays where the device formed them (moments.mine_pairs): there are no host lists then,
    ``vi`` and ``qi`` are None, and nothing that takes a plan may read them."""

    def __init__(self, video_index, query_index, V, Q, device, gt_video=None, what="pair_plan"):
        vi, qi = host_array(video_index), host_array(query_index)
        if vi.shape[0] != qi.shape[0]:
            raise ValueError(f"{what}: video_index and query_index must have one length (got {vi.shape[0]} and {qi.shape[0]})")
        P = vi.shape[0]
        if P < 1:
            raise ValueError(f"{what}: at least one pair")
        if vi.min() < 0 or vi.max() >= V or qi.min() < 0 or qi.max() >= Q:
            raise ValueError(f"{what}: video_index must lie in [0, {V}) and query_index in [0, {Q})")
        parts = [vi, qi]
        for idx, n in ((vi, V), (qi, Q)):
            parts += [np.concatenate([[0], np.cumsum(np.bincount(idx, minlength=n))]), np.argsort(idx, kind="stable")]
        rows = None
        if gt_video is not None:
            gv = host_array(gt_video)
            if gv.shape[0] != Q:
                raise ValueError(f"{what}: gt_video must name a video for each of the Q = {Q} queries (got {gv.shape[0]})")
            pos = vi == gv[qi]
            rows = np.flatnonzero(pos)
            parts += [pos, rows]
        device = torch.device(device)
        cuts = _upload(parts, np.int32, device)
        self.vi, self.qi, self.V, self.Q, self.P, self.device = vi, qi, V, Q, P, device
        self.video_index, self.query_index, self.v_ptr, self.v_pairs, self.q_ptr, self.q_pairs = cuts[:6]
        self.positive, self.positive_rows = (cuts[6], cuts[7].to(torch.int64)) if rows is not None else (None, None)
        self.num_positive = None if rows is None else int(rows.shape[0])

    @classmethod
    def from_device(cls, video_index, query_index, v_ptr, v_pairs, q_ptr, q_pairs, V, Q, positive=None, positive_rows=None, num_positive=None):
        """A plan over int32 arrays that are on their device already (smin_mine_pairs' outputs): nothing is copied, checked against
        the ranges or read back.  ``positive (P,)`` int32, ``positive_rows`` int64 and ``num_positive`` (a host int) as the
        constructor forms them from gt_video, where the caller knows them (pair_targets and train_epoch_pairs need them)."""
        P = video_index.shape[0]
        if P < 1 or any(tuple(a.shape) != (n,) for a, n in ((query_index, P), (v_pairs, P), (q_pairs, P), (v_ptr, V + 1), (q_ptr, Q + 1))):
            raise ValueError(f"PairPlan.from_device: four (P,) arrays with P >= 1, v_ptr (V + 1,) = ({V + 1},) and q_ptr (Q + 1,) = ({Q + 1},)")
        self = cls.__new__(cls)
        self.vi = self.qi = None
        self.V, self.Q, self.P, self.device = V, Q, P, video_index.device
        self.video_index, self.query_index, self.v_ptr, self.v_pairs, self.q_ptr, self.q_pairs = video_index, query_index, v_ptr, v_pairs, q_ptr, q_pairs
        self.positive, self.positive_rows, self.num_positive = positive, positive_rows, num_positive
        return self

    def fits(self, V, Q, device):
        return self.V == V and self.Q == Q and self.device == torch.device(device)


def _chunk_buffers(n, k, max_batch, dev):
    """Where the chunks of n windows / pairs leave their k best moments: top_moments' ``idx (n, k, 2)``, ``score (n, k)`` and
    ``count (n,)`` on ``dev``, and the chunks' bounds [(c0, c1), ...] of at most ``max_batch`` rows."""
    idx = torch.empty((n, k, 2), dtype=torch.int64, device=dev)
    score = torch.empty((n, k), dtype=torch.float32, device=dev)
    count = torch.empty((n,), dtype=torch.int32, device=dev)
    return idx, score, count, [(c0, min(c0 + max_batch, n)) for c0 in range(0, n, max_batch)]


def _pool_buffers(n, dev):
    """Where the chunks of n pairs leave pair_pool's ``score (n,)``, ``pool (n, 2)`` and ``cells (n,)`` on ``dev``."""
    return tuple(torch.empty(shape, dtype=torch.float32, device=dev) for shape in ((n,), (n, 2), (n,)))


def _rank_lists(o, lists, video_d, ptr_d, gt_d=None, pooled=None):
    """The ranking tail of every search: each query's ``o.k`` best moments across its videos out of ``lists``, its pairs' top_moments
    lists (``idx``: one smin_corpus_topk) or its groups' merge_window_moments lists (``span`` / ``window`` / ``cell``: one
    smin_corpus_span_topk) -- ``video_d``: each pair's or group's video, ``ptr_d (Q + 1,)``: query q owns ``ptr_d[q] .. ptr_d[q + 1]``, both
    int32.  With the video-level options (``o.ranked``), in front of it one smin_video_rank over ``pooled``, the pairs'
    or groups' pooled ``(score, cells)``, and one smin_moment_reweight of the lists by it; the result then gains ``video_rank``,
    ``video_score``, ``video_count`` and ``gt_rank`` (``gt_d``: ``o.gt`` on the device).  ``lists`` is left as it is.  No host read."""
    score, count = lists["score"], lists["count"]
    if o.ranked:
        vr = rank_videos(pooled[0], pooled[1], video_d, ptr_d, n=o.n_videos, alpha=o.alpha, gt_video=gt_d if o.gt.size else None)
        score, count = reweight_moments(score, count, vr["pair_rank"], vr["weight"], o.max_videos)
    if "idx" in lists:
        r = corpus_topk(score, lists["idx"], count, video_d, ptr_d, k=o.k)
    else:
        r = corpus_span_topk(lists["span"], score, lists["window"], lists["cell"], count, video_d, ptr_d, k=o.k)
    if o.ranked:
        r.update(video_rank=vr["video"], video_score=vr["score"], video_count=vr["count"], gt_rank=vr["gt_rank"])
    return r


class _Retrieval:
    """SMIN's retrieval methods, inherited by modules.SMIN: no constructor and no state of its own."""

    def _scores(self, *inputs):
        """The scores retrieval ranks (under no_grad): score() with forward_only_scoring, else the forward."""
        return self.score(*inputs) if self.forward_only_scoring else self(*inputs)

    def localize(self, video_features, video_mask, query_features, query_mask, length_mask, moment_mask, k=5, nms_thresh=0.5,
                 duration=None, attention=False, nms="hard", sigma=0.5, min_score=None):
        """The k best moments per sample: the forward under torch.no_grad() (score() with forward_only_scoring), then moments.top_moments of its (pm, ps, pe) -- greedy
        temporal NMS at ``nms_thresh`` over the valid cells of ``moment_mask``.  Returns top_moments' dict (``idx`` (B, k, 2) start
        / end clip, ``score``, ``count``; with ``duration`` (B,) seconds also ``times`` (B, k, 2) in seconds).
        ``nms="linear"`` / ``"gaussian"`` with ``sigma`` and ``min_score``: top_moments' Soft-NMS rules (the dict gains ``raw_score``).

        attention=True: also ``content_attention`` (B, k, layers, C, Nq), the content unit's word weights of each clip of each kept
        moment, and ``boundary_attention`` (B, k, layers, 2, Nq), the boundary unit's word weights of its start and end rows (empty
        slots 0): gathered on the device from the packed maps, no dense map is formed."""
        with torch.no_grad():
            if attention:
                maps = _AttnMaps("packed")
                pm, ps, pe, _ = self._forward(video_features, video_mask, query_features, query_mask, length_mask, moment_mask, maps)
            else:
                pm, ps, pe, _ = self._scores(video_features, video_mask, query_features, query_mask, length_mask, moment_mask)
            r = top_moments(pm, ps, pe, moment_mask, k=k, nms_thresh=nms_thresh, duration=duration, nms=nms, sigma=sigma, min_score=min_score)
            if attention:
                r["content_attention"], r["boundary_attention"] = attn_maps_gather([c for c, _ in maps], [b for _, b in maps], maps.cellmap,
                                                                                   r["idx"], self.C)
        return r

    def localize_windows(self, raw, lengths, query_features, query_mask, video_index=None, window=None, stride=None, k=5, k_window=None,
                         nms_thresh=0.5, mode="pick", duration=None, max_batch=64, nms="hard", sigma=0.5, min_score=None):
        """The k best moments of (video, query) pairs over videos of any length: overlapping windows of ``window`` raw rows (default
        T: one row per clip) every ``stride`` rows (default window // 2) are each resampled to T clips, scored by the model and cut to
        their ``k_window`` (default k) best moments, which are then merged per pair by greedy NMS in raw-row time.

        ``raw`` (R, Din) HIP float32 tensor of V videos' rows back to back, ``lengths`` their V row counts (host); ``query_features``
        (B, Nq, E) / ``query_mask`` the B pairs' queries, ``video_index`` (B,) host ints (default arange(V), B == V) maps a pair to
        its video (the rows are not copied per pair).  Windows are processed in chunks of ``max_batch``: sample_windows, the masks
        from nfeats, one forward under no_grad (score() with forward_only_scoring), top_moments; then one merge (moments.merge_window_moments).  The plan is host
        arithmetic, so each chunk's valid-cell count is handed to the forward (``known_cell_count``) and nothing is read back.

        Returns a dict: ``span`` (B, k, 2) float32 raw rows of the video (NaN for empty slots), ``score`` (B, k), ``window`` (B, k)
        int64 window ordinal within the pair (-1), ``cell`` (B, k, 2) int64 cell of that window (-1), ``count`` (B,) int32 and
        ``n_windows`` (B,) int64; with ``duration`` (B,) seconds also ``times`` = (span * duration) / n (fp32; n = the video's rows).

        ``nms="linear"`` / ``"gaussian"`` (moments.soft_rule): each window picks its ``k_window`` candidates by the soft rule and hands
        their UNDECAYED scores to the soft merge, which decays them once, in raw-row time, and applies ``min_score``; the result gains
        ``raw_score`` (B, k)."""
        T, L = self.T, self.L
        rule = soft_rule("localize_windows", nms, nms_thresh, sigma, min_score)
        k_window = k if k_window is None else k_window
        window = T if window is None else window
        stride = max(int(window) // 2, 1) if stride is None else stride
        require_ints("localize_windows", ("k", k, 1, MAX_K), ("k_window", k_window, 1, MAX_K), ("window", window, 1, MAX_ROWS),
                     ("stride", stride, 1, MAX_ROWS), ("max_batch", max_batch, 1, 65535))
        if mode not in MODES:
            raise ValueError(f"localize_windows: mode must be one of {sorted(MODES)} (got {mode!r})")
        require_hip_tensors("localize_windows", dict(raw=raw, query_features=query_features, query_mask=query_mask))
        if raw.dim() != 2 or raw.dtype != torch.float32 or raw.shape[1] % 4 != 0 or raw.shape[1] != self.input_video_dim:
            raise ValueError(f"localize_windows: raw must be float32 (R, Din = {self.input_video_dim}) with Din % 4 == 0 (got "
                             f"{tuple(raw.shape)} {raw.dtype})")
        n = host_array(lengths)
        if n.size and n.min() < 0 or int(n.sum()) != raw.shape[0]:
            raise ValueError(f"localize_windows: lengths must be >= 0 and sum to raw's {raw.shape[0]} rows (got {int(n.sum())})")
        V, B = n.shape[0], query_features.shape[0]
        if video_index is None:
            if B != V:
                raise ValueError(f"localize_windows: without video_index the B = {B} queries pair with the V = {V} videos one to one")
            vi = np.arange(V, dtype=np.int64)
        else:
            vi = host_array(video_index)
            if vi.shape[0] != B or (B and (vi.min() < 0 or vi.max() >= V)):
                raise ValueError(f"localize_windows: video_index must hold B = {B} indices in [0, {V}) (got {vi.tolist()[:8]})")
        if query_mask.shape[0] != B:
            raise ValueError(f"localize_windows: query_mask has {query_mask.shape[0]} rows for B = {B} queries")
        if duration is not None and tuple(duration.shape) != (B,):
            raise ValueError(f"localize_windows: duration must be (B,) = ({B},) seconds (got {tuple(duration.shape)})")
        starts, lens, vptr = (x.numpy() for x in window_plan(n, window, stride))
        dev = raw.device
        # per pair: its video's windows, in global window order (pair, then start)
        nw = (vptr[1:] - vptr[:-1])[vi] if B else np.zeros(0, np.int64)
        pair_ptr = np.concatenate([[0], np.cumsum(nw)]).astype(np.int64)
        G = int(pair_ptr[-1])
        if G * k_window >= 2 ** 31:
            raise ValueError(f"localize_windows: {G} windows of {k_window} moments exceed the merge's 2**31 candidates")
        wsel = np.concatenate([np.arange(vptr[v], vptr[v + 1]) for v in vi]).astype(np.int64) if G else np.zeros(0, np.int64)
        offs = np.concatenate([[0], np.cumsum(n)]).astype(np.int64)
        pair_of = np.repeat(np.arange(B, dtype=np.int64), nw)
        w_start, w_len = starts[wsel], lens[wsel].astype(np.int64)
        nf = np.minimum(w_len, T)
        cells = np.array([cell_count(x, T, L) for x in nf], dtype=np.int64)                      # per window, as csrc/labels.hip forms it
        # the whole plan in one pinned buffer, one asynchronous copy (the call never waits for the device)
        rb_d, st_d, ln_d, po_d, pp_d, nw_d, nr_d = _upload([offs[vi[pair_of]] + w_start if G else np.zeros(0, np.int64), w_start, w_len, pair_of,
                                                            pair_ptr, nw, n[vi]], np.int64, dev)
        ln_d = ln_d.to(torch.int32)
        idx, score, count, chunks = _chunk_buffers(G, k_window, max_batch, dev)
        # a soft rule's windows never stop early, and the merge is given their picks' RAW scores: `score` takes the selection's raw
        # output and the windows' own decayed scores go to `decayed`, which nothing reads
        wrule = None if rule is None else rule[:3] + (float("-inf"),)
        decayed = None if rule is None else torch.empty_like(score)
        with torch.no_grad(), torch.cuda.device(dev):
            for c0, c1 in chunks:
                vf, nfeats = sample_windows(raw, rb_d[c0:c1], ln_d[c0:c1], T, mode=mode)
                m = build_masks_hip(nfeats, T, L)
                rows = po_d[c0:c1]
                qf, qm = query_features.index_select(0, rows), query_mask.index_select(0, rows)
                with known_cells(self, int(cells[c0:c1].sum())):
                    pm, ps, pe, _ = self._scores(vf, m["video_mask"], qf, qm, m["length_mask"], m["moment_mask"])
                _select_into(pm, ps, pe, m["moment_mask"], k_window, nms_thresh, wrule, idx[c0:c1], (score if rule is None else decayed)[c0:c1],
                             count[c0:c1], raw=None if rule is None else score[c0:c1])
        r = merge_window_moments(idx, score, count, st_d, ln_d, pp_d, T, L, k=k, nms_thresh=nms_thresh, nms=nms, sigma=sigma, min_score=min_score)
        r["n_windows"] = nw_d
        if duration is not None:
            d = duration.to(device=dev, dtype=torch.float32).reshape(B, 1, 1)
            r["times"] = (r["span"] * d) / nr_d.to(torch.float32).reshape(B, 1, 1)
        return r

    # ---------------------------------------------------------------- corpus search
    def _bank_plan(self, video_features, query_features):
        """Whether pairs of these inputs score on the one-node path from banks (as score(): _plan == "node" and no keep_attention)."""
        return not self.keep_attention and self._plan(video_features, query_features) == "node"

    def encode_videos(self, video_features, video_mask, length_mask, moment_mask, cell_counts=None, storage="fp32", max_batch=None):
        """A VideoBank of V videos: the projection with position embedding and mask runs once per video (smin_hip::smin_encode_videos),
        not once per (video, query) pair.  ``video_features (V, T, Din)`` and the three masks as forward takes them.  One host read
        (the videos' valid-cell counts), none with ``cell_counts``, the V counts as host ints (feeder.cell_count); under
        torch.no_grad().  The bank is stale after a parameter update.

        ``storage``: ``"fp32"`` (default), ``"bf16"`` or ``"int8"`` -- the bank is held compact (VideoBank), with the
        codes of ``encode_videos(...).compact(storage)``.  ``max_batch``: the videos are encoded (and encoded to codes) at most that
        many at a time, so with a compact storage the fp32 ``fv`` of the whole corpus never exists.  Off the one-node path (``fv`` is
        None) a compact storage raises ValueError."""
        require_storage("encode_videos", storage)
        if max_batch is not None:
            require_ints("encode_videos", ("max_batch", max_batch, 1, 2 ** 31 - 1))
        require_hip_tensors("encode_videos", dict(video_features=video_features, video_mask=video_mask, length_mask=length_mask, moment_mask=moment_mask))
        V = video_features.shape[0]
        if video_features.dim() != 3 or V < 1 or video_mask.shape[0] != V or tuple(length_mask.shape) != (V, self.L) or tuple(moment_mask.shape) != (V, self.L, self.L):
            raise ValueError(f"encode_videos: video_features (V, T, Din) with V >= 1, video_mask (V, T[, 1]), length_mask (V, L) and moment_mask (V, L, L); got "
                             f"{tuple(video_features.shape)}, {tuple(video_mask.shape)}, {tuple(length_mask.shape)}, {tuple(moment_mask.shape)}")
        with torch.no_grad(), torch.cuda.device(video_features.device):
            vf = video_features.detach()
            masks = [byte_mask(t) for t in (video_mask, length_mask, moment_mask)]
            fv = fv_scale = None
            if self.fused_core and self.backbone.videoencoder.fused(vf) and vf.shape[1] == self.T:
                ops, prm, step = _lib.load_torch(), self._native_params()[:3], V if max_batch is None else int(max_batch)
                for c0 in range(0, V, step):
                    c1 = min(c0 + step, V)
                    part = ops.smin_encode_videos(vf[c0:c1], masks[0][c0:c1], prm)
                    part, part_scale = (part, None) if storage == "fp32" else bank_encode(part, storage)
                    if (c0, c1) == (0, V):
                        fv, fv_scale = part, part_scale
                        break
                    if fv is None:
                        fv = torch.empty((V,) + tuple(part.shape[1:]), dtype=part.dtype, device=part.device)
                        fv_scale = None if part_scale is None else torch.empty((V, part.shape[1]), dtype=torch.float32, device=part.device)
                    fv[c0:c1] = part
                    if part_scale is not None:
                        fv_scale[c0:c1] = part_scale
            elif storage != "fp32":
                raise ValueError("encode_videos: a compact storage holds fv, which this module or these inputs do not form (off the one-node path, "
                                 "SMIN._plan); encode with storage='fp32'")
            if cell_counts is None:
                counts = masks[2].reshape(V, -1).ne(0).sum(dim=1).tolist()         # the bank's only host read
            else:
                counts = host_array(cell_counts)
                if counts.shape[0] != V:
                    raise ValueError(f"encode_videos: cell_counts must hold the V = {V} videos' counts (got {counts.shape[0]})")
        return VideoBank(fv, vf, masks[0], masks[1], masks[2], counts, fv_scale)

    def encode_queries(self, query_features, query_mask):
        """A QueryBank of Q queries: the two BiLSTM layers and the sentence feature run once per query
        (smin_hip::smin_encode_queries).  ``query_features (Q, words, E)`` / ``query_mask`` as forward takes them.  No host read;
        under torch.no_grad().  The bank is stale after a parameter update."""
        require_hip_tensors("encode_queries", dict(query_features=query_features, query_mask=query_mask))
        if query_features.dim() != 3 or query_features.shape[0] < 1:
            raise ValueError(f"encode_queries: query_features (Q, words, E) with Q >= 1 (got {tuple(query_features.shape)})")
        qm = query_mask_rows(query_features, query_mask, self.max_query_length)
        with torch.no_grad(), torch.cuda.device(query_features.device):
            qf = query_features.detach()
            qm = byte_mask(qm)
            fw = fs = None
            if self.fused_core and self.backbone.queryencoder.fused() and qf.dtype == torch.float32:
                fw, fs = _lib.load_torch().smin_encode_queries(qf, qm, self._native_params()[:19], self.max_query_length, self.lstm_hidden_size)
            if qm.shape[1] < self.max_query_length:
                qm = torch.nn.functional.pad(qm, (0, self.max_query_length - qm.shape[1]))
        return QueryBank(fw, fs, qf, qm)

    @staticmethod
    def _pair_lists(what, videos, queries, video_index, query_index):
        _require_banks(what, videos, queries)
        vi, qi = host_array(video_index), host_array(query_index)
        if vi.shape[0] != qi.shape[0]:
            raise ValueError(f"{what}: video_index and query_index must have one length (got {vi.shape[0]} and {qi.shape[0]})")
        return _Retrieval._check_range(what, vi, qi, len(videos), len(queries))

    @staticmethod
    def _check_range(what, vi, qi, V, Q):
        if vi.size and (vi.min() < 0 or vi.max() >= V or qi.min() < 0 or qi.max() >= Q):
            raise ValueError(f"{what}: video_index must lie in [0, {V}) and query_index in [0, {Q})")
        return vi, qi

    def _score_pairs(self, videos, queries, vi, qi, vi_d, qi_d, cells=None):
        """score_pairs of checked host lists vi / qi (P >= 1) whose int32 device copies are vi_d / qi_d.  No host read.  ``vi`` None: the
        lists exist on the device only, and ``cells`` is the pairs' valid-cell count where the caller knows it (None: the node reads it)."""
        if vi is not None:
            cells = sum(videos.cell_counts[v] for v in vi)                        # host arithmetic: the scorer asks the device nothing
        with known_cells(self, cells), torch.no_grad(), torch.cuda.device(vi_d.device):
            if not self._bank_plan(videos.plan_features, queries.query_features):
                # as score(): configurations off the one-node path (and keep_attention) run the forward, here on expanded pairs
                if videos.video_features is None:
                    raise ValueError("score_pairs: the window bank was encoded on the one-node path and keeps no features to expand; encode it again")
                if videos.storage != "fp32":
                    raise ValueError(f"score_pairs: a bank held as {videos.storage} is scored on the one-node path only (SMIN._plan; the forward "
                                     "reads the videos' own features, not the codes)")
                qm = queries.query_mask[:, :queries.query_features.shape[1]]
                return self.score(videos.video_features.index_select(0, vi_d), videos.video_mask.index_select(0, vi_d),
                                  queries.query_features.index_select(0, qi_d), qm.index_select(0, qi_d),
                                  videos.length_mask.index_select(0, vi_d), videos.moment_mask.index_select(0, vi_d))
            _require_node_banks(videos, queries)
            if videos.storage != "fp32":
                return _lib.load_torch().smin_score_pairs_compact(
                    videos.fv, videos.fv_scale, queries.fw, queries.fs, videos.video_mask, queries.query_mask, videos.length_mask, videos.moment_mask,
                    vi_d, qi_d, *self._core_args(), **self._score_options())
            return _lib.load_torch().smin_score_pairs(
                videos.fv, queries.fw, queries.fs, videos.video_mask, queries.query_mask, videos.length_mask, videos.moment_mask, vi_d, qi_d,
                *self._core_args(), **self._score_options())

    def score_pairs(self, videos, queries, video_index, query_index):
        """(pm, ps, pe, pa) as score() returns them for the P pairs (videos[video_index[p]], queries[query_index[p]]) of a VideoBank
        and a QueryBank: neither encoder runs again, and no pair carries a copy of its video's features.  ``video_index`` /
        ``query_index``: host int sequences of one length P >= 1, any lists, repeats included; an index out of range raises
        ValueError.  On the one-node path this is smin_hip::smin_score_pairs: the pairs' masks gathered (bytes), smin_pair_assemble
        where smin_score has its backbone, then smin_score's own code -- the bits of score() on the expanded batch.  Where score()
        would run the forward instead (_plan != "node", keep_attention) the pairs are expanded and scored by score().  The valid-cell
        count comes from the bank, so nothing is read back."""
        vi, qi = self._pair_lists("score_pairs", videos, queries, video_index, query_index)
        if vi.shape[0] < 1:
            raise ValueError("score_pairs: at least one pair")
        require_hip_tensors("score_pairs", dict(videos=videos.video_mask, queries=queries.query_features), must="hold HIP tensors")
        return self._score_pairs(videos, queries, vi, qi, *_upload([vi, qi], np.int32, videos.device))

    # ---------------------------------------------------------------- training through shared banks
    def forward_pairs(self, video_features, video_mask, query_features, query_mask, length_mask, moment_mask, video_index, query_index,
                      cell_counts=None, plan=None):
        """(pm, ps, pe, pa) as forward returns them for the P pairs (video video_index[p], query query_index[p]) of V videos and Q
        queries, differentiable with respect to the parameters: the video encoder runs once per video and the query encoder once per
        query, in the forward and in the backward, and no pair carries a copy of its video's features.  ``video_features (V, T, Din)``,
        ``video_mask``, ``length_mask`` and ``moment_mask`` have a row per video, ``query_features (Q, words, E)`` and ``query_mask`` a
        row per query; ``video_index`` / ``query_index``: host int sequences of one length P >= 1, any lists, repeats included; an
        index out of range or an empty list raises ValueError.  ``cell_counts``: the V videos' valid-cell counts as host ints
        (feeder.cell_count); with them the pairs' count is host arithmetic and the step reads nothing back, without them the node
        reads the count once, as forward does.  ``plan``: a PairPlan already built from these lists (training.train_epoch_pairs
        shares one with pair_targets: one copy for both).  A device-built plan (SMIN.mine_pairs; ``plan.vi is None``) has no host list
        to sum the counts over: with ``cell_counts`` whose V entries are all one value c -- the common case, every longer video is
        resampled to T -- the pairs' count is P * c and the step reads nothing back; with unequal counts, or none, no
        count is handed over and the node reads it once.

        On the one-node path this is smin_hip::smin_forward_pairs, one autograd node: smin_pair_assemble where smin_forward has the
        product f = f_v * f_s, the layers at batch P, and in the backward smin_pair_assemble_bwd -- a sum over the pairs that share a
        video or a query, in list order, the same bits every run -- in front of the encoders' backward at batch V and Q.  Where
        forward would not take that path (_plan != "node", keep_attention) the pairs are expanded with index_select and go through
        forward: bit for bit that route.  Not with grad_sync (data-parallel training through this node is out of scope)."""
        V, Q = video_features.shape[0], query_features.shape[0]
        if plan is None:
            plan = PairPlan(video_index, query_index, V, Q, video_features.device, what="forward_pairs")
        elif not plan.fits(V, Q, video_features.device):
            raise ValueError(f"forward_pairs: the plan was built for {plan.V} videos and {plan.Q} queries on {plan.device}")
        require_hip_tensors("forward_pairs", dict(video_features=video_features, video_mask=video_mask, query_features=query_features, query_mask=query_mask,
                                                  length_mask=length_mask, moment_mask=moment_mask))
        if video_features.dim() != 3 or query_features.dim() != 3 or V < 1 or Q < 1 or video_mask.shape[0] != V or length_mask.shape[0] != V \
                or moment_mask.shape[0] != V or query_mask.shape[0] != Q:
            raise ValueError("forward_pairs: video_features (V, T, Din), video_mask, length_mask and moment_mask with a row per video; "
                             "query_features (Q, words, E) and query_mask with a row per query")
        if self.grad_sync:
            raise RuntimeError("forward_pairs: not combined with the in-node gradient exchange (SMIN.grad_sync)")
        cells = None
        if cell_counts is not None:
            cc = host_array(cell_counts)
            if cc.shape[0] != V:
                raise ValueError(f"forward_pairs: cell_counts must hold the V = {V} videos' counts (got {cc.shape[0]})")
            if plan.vi is not None:
                cells = int(cc[plan.vi].sum())
            elif (cc == cc[0]).all():
                cells = plan.P * int(cc[0])
        vi_d, qi_d = plan.video_index, plan.query_index
        with known_cells(self, cells), torch.cuda.device(video_features.device):
            if not self._bank_plan(video_features, query_features):
                # as score_pairs: configurations off the one-node path (and keep_attention) run the forward on expanded pairs
                return self.forward(video_features.index_select(0, vi_d), video_mask.index_select(0, vi_d), query_features.index_select(0, qi_d),
                                    query_mask.index_select(0, qi_d), length_mask.index_select(0, vi_d), moment_mask.index_select(0, vi_d))
            qm = query_mask_rows(query_features, query_mask, self.max_query_length)
            if qm.shape[1] < self.max_query_length:
                qm = torch.nn.functional.pad(qm, (0, self.max_query_length - qm.shape[1]))
            o = self._node_options()
            for refused in ("grad_sync", "input_grads", "attention"):
                o.pop(refused)
            return _lib.load_torch().smin_forward_pairs(
                video_features, video_mask, query_features, qm, length_mask, moment_mask, vi_d, qi_d, plan.v_ptr, plan.v_pairs, plan.q_ptr, plan.q_pairs,
                *self._core_args(), **o)

    def _search_plan(self, what, videos, queries, pairs, k, k_video, max_batch, duration):
        """search's checked arguments and its pair lists: ``(options, vi, qi, pair_ptr)`` (_Options, _listed_pairs)."""
        o = _Options(what, k, k_video, max_batch)
        _require_banks(what, videos, queries)
        V, Q = len(videos), len(queries)
        vi, qi, pair_ptr = self._listed_pairs(what, pairs, V, Q)
        o.duration(duration, V)
        require_hip_tensors(what, dict(videos=videos.video_mask, queries=queries.query_features), must="hold HIP tensors")
        return o, vi, qi, pair_ptr

    @staticmethod
    def _listed_pairs(what, pairs, V, Q):
        """The checked (query, video) pairs of a search over V videos and Q queries, sorted by (query, video): host lists ``vi``, ``qi``
        and ``pair_ptr (Q + 1,)``, query q owning pairs ``pair_ptr[q] .. pair_ptr[q + 1]``.  ``pairs`` None: every query against every
        video.  ValueError for a malformed list, an index out of range or a repeated pair."""
        if pairs is None:
            qi, vi = np.repeat(np.arange(Q, dtype=np.int64), V), np.tile(np.arange(V, dtype=np.int64), Q)
        else:
            pr = host_array(pairs, shape=None)
            if pr.size == 0:
                pr = pr.reshape(0, 2)
            if pr.ndim != 2 or pr.shape[1] != 2:
                raise ValueError(f"{what}: pairs must be (P, 2) rows of (query, video) (got {pr.shape})")
            order = np.lexsort((pr[:, 1], pr[:, 0]))                               # by (query, video)
            qi, vi = pr[order, 0], pr[order, 1]
        vi, qi = _Retrieval._check_range(what, host_array(vi), host_array(qi), V, Q)
        if vi.size > 1 and bool(((qi[1:] == qi[:-1]) & (vi[1:] == vi[:-1])).any()):
            raise ValueError(f"{what}: a (query, video) pair is listed more than once")
        pair_ptr = np.concatenate([[0], np.cumsum(np.bincount(qi, minlength=Q))]).astype(np.int64)
        return vi, qi, pair_ptr

    @staticmethod
    def _search_result(r, duration, L):
        if duration is not None:
            r["times"] = search_times(r["video"], r["idx"], duration, L)          # moments._times' formula on each moment's own video
        return r

    def search(self, videos, queries, pairs=None, k=5, k_video=None, nms_thresh=0.5, duration=None, max_batch=64, video_weight=None,
               max_videos=None, tau=0.1, n_videos=None, gt_video=None, prefilter=None, carry=False):
        """Which video, and where: the k best moments of each of the Q queries of a QueryBank over the videos of a VideoBank.

        ``pairs``: None -- every query against every video --, or a host (P, 2) array of (query, video) rows, in any order (sorted
        here by (query, video)); a repeated pair raises ValueError.  The pairs are scored in chunks of at most ``max_batch``
        (score_pairs: from the banks, no encoder runs again; each chunk's valid-cell count is the sum of the bank's cell_counts,
        nothing is read back), each chunk is cut to its ``k_video`` (default k) best moments per pair by top_moments' kernels
        (greedy NMS at ``nms_thresh``), and one smin_corpus_topk ranks each query's moments across its videos: higher score first,
        ties -> lower video, then lower slot.  Every listed pair is scored by the full model.

        Returns a dict: ``video (Q, k)`` int64 (-1 for empty slots), ``idx (Q, k, 2)`` int64 start / end clip (-1), ``score (Q, k)``
        (0), ``count (Q,)`` int32; with ``duration`` (V,) seconds also ``times (Q, k, 2)``: top_moments' formula on
        ``duration[video]``, NaN for empty slots.  Scores come from score_pairs (forward_only_scoring or not: a bank has no graph),
        in the contraction mode of set_gemm_mode.  No host synchronisation.

        ``video_weight`` / ``max_videos`` (both None: the search above, untouched) bring in the video-level score the contrastive
        loss trains: each chunk's scores are also pooled into their pair scores at temperature ``tau`` (one
        pair_pool launch; the model does not run again), one smin_video_rank ranks each query's videos by them, and one
        smin_moment_reweight multiplies every moment score by ``exp(video_weight * (s_video - the query's best s))`` and, with
        ``max_videos`` = M, empties the lists of the videos behind the query's best M, before the same smin_corpus_topk.  ``score`` is
        then the weighted score, and the result gains ``video_rank (Q, n_videos)`` int64 (-1), ``video_score`` (0), ``video_count
        (Q,)`` and ``gt_rank (Q,)`` int32: the rank of ``gt_video[q]`` (Q host ints) among the query's videos, -1 if it is not listed
        or no gt_video is given.  ``n_videos`` defaults to min(k, 64).

        ``carry=True`` (with the video-level options; alone it implies ``video_weight=0.0``) makes the result one that
        moments.merge_search_weighted can merge with other shards' (INTEGRATION.md 3u): ``pairs`` must be None (ValueError otherwise),
        and the result gains ``raw (Q, k)``, each listed entry's unweighted score -- the bits of its pair's own top_moments list, found
        by matching (video, idx) against that list with a few torch ops; 0 for empty slots --, and ``pair_score`` / ``pair_cells (Q, V)``,
        the pooled score and valid-cell count of every (query, video) of the bank, the arrays smin_video_rank was fed.  ``score`` stays
        the score weighted within this bank and the list stays cut by this bank's ranks.  No host read.

        ``prefilter=M`` (None: everything above, untouched) prunes the videos before the model runs:
        ``prefilter_videos`` scores every (query, video) from the banks alone and keeps each query's best ``Ms = min(M, V)`` videos, and
        the chunk loop and smin_corpus_topk above then run over those Q * Ms pairs, whose lists were built on the device
        (``pair_ptr[q] = q * Ms``): the full model scores Q * Ms pairs instead of Q * V.  No host list exists to sum the bank's
        cell_counts over, so the rule ``forward_pairs`` documents for a mined plan applies: when all the bank's ``cell_counts`` are one
        value c, each chunk's valid-cell count is ``pairs * c`` and the call reads nothing back; otherwise no count is handed over and
        the node reads it once per chunk.  ``video_weight`` / ``max_videos`` / ``gt_video`` / ``tau`` act as above on the surviving
        pairs (``tau`` is also the first stage's temperature).  With ``pairs`` or ``carry=True``: ValueError (a carried merge needs
        every video's pooled score).  The result gains ``prefilter_video (Q, Ms)`` int64 ascending, ``prefilter_score (Q, V)`` and
        ``prefilter_gt_rank (Q,)`` int32, the first stage's rank of ``gt_video[q]`` (-1 without gt_video or for a non-candidate).  What
        the pruning loses is not bounded: a video the first stage ranks behind M is never seen by the model."""
        if prefilter is not None:
            if pairs is not None or carry:
                raise ValueError("search: prefilter takes pairs=None and carry=False (it chooses the pairs itself, and a carried merge needs "
                                 "every video's pooled score)")
            return self._search_prefiltered(videos, queries, prefilter, k, k_video, nms_thresh, duration, max_batch, video_weight, max_videos, tau,
                                            n_videos, gt_video)
        if carry and pairs is not None:
            raise ValueError("search: carry=True takes pairs=None, every query against every video of the bank (a merge re-ranks all the shard's videos)")
        if carry and video_weight is None and max_videos is None:
            video_weight = 0.0
        o, vi, qi, pair_ptr = self._search_plan("search", videos, queries, pairs, k, k_video, max_batch, duration)
        if video_weight is not None or max_videos is not None:
            o.video_level(video_weight, max_videos, tau, n_videos, gt_video, len(queries))
        dev, Q, V = videos.device, len(queries), len(videos)
        # the whole plan in one pinned buffer, one asynchronous copy (the call never waits for the device)
        vi_d, qi_d, pp_d, gt_d = _upload([vi, qi, pair_ptr, o.gt], np.int32, dev)
        with torch.no_grad(), torch.cuda.device(dev):
            lists, pools = self._pair_chunks(videos, queries, vi_d, qi_d, max_batch, host=(vi, qi), cut=(o.k_video, nms_thresh),
                                             tau=o.tau if o.ranked else None)
            r = _rank_lists(o, lists, vi_d, pp_d, gt_d, pools and (pools[0], pools[2]))
            if carry:
                r["raw"] = _carry_raw(r["video"], (r["idx"],), (lists["idx"],), lists["score"], lists["count"], V)
                r["pair_score"], r["pair_cells"] = pools[0].reshape(Q, V), pools[2].reshape(Q, V)
        return self._search_result(r, duration, self.L)

    def _pair_chunks(self, videos, queries, vi_d, qi_d, max_batch, host=None, cell=None, cut=None, tau=None):
        """search's chunk loop, the only one: the P pairs of the int32 device lists ``vi_d`` / ``qi_d`` scored from the banks in chunks of
        at most ``max_batch`` (_score_pairs), each chunk's moment masks gathered, and of each chunk's scores what is asked for:
        ``cut = (k_video, nms_thresh)`` -- top_moments' ``idx (P, k_video, 2)``, ``score (P, k_video)`` and ``count (P,)``, returned as a
        dict --, ``tau`` -- pair_pool's ``(score (P,), pool (P, 2), cells (P,))`` at that temperature, one launch on the scores the chunk
        already holds.  Returns ``(lists, pools)``, None for what was not asked for.  A chunk's valid-cell count: with ``host``, the checked
        host lists ``(vi, qi)`` the device lists were copied from, the sum of the bank's cell_counts; without them the lists exist on the
        device only, and it is the chunk's pairs times ``cell`` -- every video's count where the bank's are all one value -- or, ``cell``
        None, not handed over: the node reads it once per chunk.  No host read otherwise."""
        P, dev = vi_d.shape[0], vi_d.device
        lists = dict(zip(("idx", "score", "count"), _chunk_buffers(P, cut[0], max_batch, dev))) if cut is not None else None
        pools = _pool_buffers(P, dev) if tau is not None else None
        for c0 in range(0, P, max_batch):
            c1 = min(c0 + max_batch, P)
            if host is not None:
                pm, ps, pe, _ = self._score_pairs(videos, queries, host[0][c0:c1], host[1][c0:c1], vi_d[c0:c1], qi_d[c0:c1])
            else:
                pm, ps, pe, _ = self._score_pairs(videos, queries, None, None, vi_d[c0:c1], qi_d[c0:c1], cells=None if cell is None else (c1 - c0) * cell)
            mm = videos.moment_mask.index_select(0, vi_d[c0:c1])
            if cut is not None:
                _select_into(pm, ps, pe, mm, cut[0], cut[1], None, lists["idx"][c0:c1], lists["score"][c0:c1], lists["count"][c0:c1])
            if tau is not None:
                _pair_pool_into(pm, ps, pe, mm, tau, pools[0][c0:c1], pools[1][c0:c1], pools[2][c0:c1])
        return lists, pools

    # ---------------------------------------------------------------- first-stage pruning from the banks alone
    def prefilter_videos(self, videos, queries, M, tau=0.1, gt_video=None):
        """Each query's best ``Ms = min(M, V)`` videos by the first-stage score: the model with zero SMI layers -- the score heads on
        ProposalGeneration's output, pooled as the contrastive loss pools the full model's maps at temperature ``tau`` --, computed from
        ``videos.fv`` and ``queries.fs`` alone (moments.prefilter_scores: one contraction over D for all Q * V pairs), ranked by the
        existing smin_video_rank and cut by moments.prefilter_select.  No new weights, no training, and no accuracy claim.

        ``videos``: a VideoBank, or a WindowBank of videos of any length -- the (query, window) pools are then composed by group_pool
        into per-video scores (a cell in the overlap of two windows counts twice).  ``gt_video``: Q host ints, each
        query's own video.  Returns a dict: ``video (Q, Ms)`` int64 ascending (a query with fewer than Ms candidates is filled with its
        lowest-indexed videos without a valid cell), ``score (Q, V)``, ``rank (Q, V)`` int32 the first-stage rank (-1 for a
        non-candidate), ``gt_rank (Q,)`` int32 as VideoRankMeter.update takes it (-1 without gt_video), and, for a VideoBank,
        ``video_index`` / ``query_index (Q * Ms,)`` int32, the device pair lists sorted by (query, video).  A bank encoded off the
        one-node path raises score_pairs' ValueError.  Under torch.no_grad(); the only copy is gt_video's (pinned, asynchronous); no
        host read."""
        what = "prefilter_videos"
        _require_banks(what, videos, queries)
        require_ints(what, ("M", M, 1, 2 ** 31 - 1))
        tau = _temperature(what, tau)
        windowed = isinstance(videos, WindowBank)
        Q, W, dev = len(queries), len(videos), videos.device
        V = videos.n_videos if windowed else W
        gt = _Options(what).gt_video(gt_video, Q).gt
        require_hip_tensors(what, dict(videos=videos.video_mask, queries=queries.query_features), must="hold HIP tensors")
        _require_node_banks(videos, queries)
        if Q * max(V, W) > 0x7fff0000:
            raise ValueError(f"{what}: {Q} queries over {max(V, W)} videos / windows exceed the int32 pair lists")
        with torch.no_grad(), torch.cuda.device(dev):
            w, b = self._first_stage_heads(videos.fv.shape[2])
            score, pool, cells = prefilter_scores(videos.fv, queries.fs, w, b, videos.length_mask, videos.moment_mask, self.T, self.L, self.C, tau,
                                                  fv_scale=videos.fv_scale)
            if windowed:
                first = torch.arange(Q, device=dev).unsqueeze(1) * W + videos.video_ptr_d[:-1].unsqueeze(0)           # group q * V + v begins here
                group_ptr = torch.cat([first.reshape(-1), first.new_full((1,), Q * W)])
                score, cells = (x.reshape(Q, V) for x in group_pool(pool.reshape(Q * W, 2), cells.reshape(Q * W), group_ptr, tau))
            gt_d = _upload([gt], np.int32, dev)[0] if gt.size else None
            video_of = torch.arange(V, dtype=torch.int32, device=dev).repeat(Q)
            pair_ptr = torch.arange(Q + 1, dtype=torch.int32, device=dev) * V
            vr = rank_videos(score.reshape(-1), cells.reshape(-1), video_of, pair_ptr, n=1, alpha=0.0, gt_video=gt_d)
            rank = vr["pair_rank"].reshape(Q, V)
            video, query = prefilter_select(rank, int(M))
        r = dict(video=video.to(torch.int64), score=score, rank=rank, gt_rank=vr["gt_rank"])
        if not windowed:
            r.update(video_index=video.reshape(-1), query_index=query.reshape(-1))
        return r

    def prefilter_fidelity(self, videos, queries, meter, tau=0.1, max_batch=64):
        """How much of the full model's video ranking a first-stage cut keeps, measured without labels: the teacher
        ranks are ``rank_videos`` on all pairs (``pair_rank`` as ``(Q, V)``), the student ranks ``prefilter_videos(...)["rank"]``, both
        pooled at ``tau``; ONE ``meter.update(teacher_rank, student_rank)`` (meter.CutFidelityMeter) and no host read.  ``videos``: a
        VideoBank; a WindowBank raises ValueError.  Returns ``(teacher score (Q, V), student score (Q, V))``."""
        what = "prefilter_fidelity"
        _require_banks(what, videos, queries)
        if isinstance(videos, WindowBank):
            raise ValueError(f"{what}: takes a VideoBank; window banks are not measured here")
        Q, V = len(queries), len(videos)
        full = self.rank_videos(videos, queries, n=1, tau=tau, max_batch=max_batch)
        first = self.prefilter_videos(videos, queries, 1, tau=tau)
        meter.update(full["pair_rank"].reshape(Q, V), first["rank"])
        return full["pair_score"].reshape(Q, V), first["score"]

    def prefilter_forward(self, video_features, video_mask, query_features, query_mask, length_mask, moment_mask, tau=0.1):
        """The first-stage maps of every (query, video) of V videos and Q queries, with grad: what prefilter_videos
        ranks by, differentiable with respect to the encoders and the three score heads; no SMI layer runs.  ``fv`` and ``fs`` come
        from the modules' own encoders (``backbone.videoencoder`` through LinearRowsFn, ``backbone.queryencoder`` through
        BiLstmLayerFn), the heads' ``w`` / ``b`` are stacked from ``localization.conv_layer_pm / ps / pe`` as prefilter_videos stacks
        them, and moments.prefilter_maps forms the maps and, in the backward, their gradients.

        Returns ``(pm0 (Q * V, L, L), ps0 (Q * V, L), pe0 (Q * V, L), score (Q, V))``: the maps in pair order ``p = q * V + v`` as
        training.pair_rank_loss takes them, the score detached (pooled at ``tau``).  Raises ValueError where the fused encoders are
        unavailable (``fused()`` false, inputs that are not float32, T differing from the model's).  No host read."""
        what = "prefilter_forward"
        if video_features.dim() != 3 or query_features.dim() != 3 or video_features.shape[0] < 1 or query_features.shape[0] < 1:
            raise ValueError(f"{what}: video_features (V, T, Din) and query_features (Q, words, E) with V, Q >= 1; got "
                             f"{tuple(video_features.shape)} and {tuple(query_features.shape)}")
        V, Q = video_features.shape[0], query_features.shape[0]
        if video_mask.shape[0] != V or tuple(length_mask.shape) != (V, self.L) or tuple(moment_mask.shape) != (V, self.L, self.L) or query_mask.shape[0] != Q:
            raise ValueError(f"{what}: video_mask (V, T[, 1]), length_mask (V, L) and moment_mask (V, L, L) with a row per video, query_mask with a "
                             f"row per query; got {tuple(video_mask.shape)}, {tuple(length_mask.shape)}, {tuple(moment_mask.shape)}, {tuple(query_mask.shape)}")
        tau = _temperature(what, tau)
        ve, qe = self.backbone.videoencoder, self.backbone.queryencoder
        if not (qe.fused() and query_features.dtype == torch.float32 and ve.fused(video_features) and video_features.shape[1] == self.T):
            raise ValueError(f"{what}: the first stage trains through the fused encoders (float32 inputs of T = {self.T} frames, "
                             "VideoEncoder.fused and QueryEncoder.fused); this module or these inputs are off that path")
        require_hip_tensors(what, dict(video_features=video_features, video_mask=video_mask, query_features=query_features, query_mask=query_mask,
                                       length_mask=length_mask, moment_mask=moment_mask))
        with torch.cuda.device(video_features.device):
            fv = ve(video_features, video_mask.reshape(V, -1, 1))
            fs, _ = qe(query_features, query_mask)
            w, b = self._first_stage_heads(self.D)
            pm0, ps0, pe0, score = prefilter_maps(fv, fs, w, b, length_mask, moment_mask, self.T, self.L, self.C, tau)
        L = self.L
        return pm0.reshape(Q * V, L, L), ps0.reshape(Q * V, L), pe0.reshape(Q * V, L), score

    def _search_prefiltered(self, videos, queries, M, k, k_video, nms_thresh, duration, max_batch, video_weight, max_videos, tau, n_videos, gt_video):
        """``search(prefilter=M)``: prefilter_videos, then search's chunk loop and ranking over the device-built Q * Ms pair lists."""
        o = _Options("search", k, k_video, max_batch)
        _require_banks("search", videos, queries)
        if isinstance(videos, WindowBank):
            raise ValueError("search: prefilter takes a VideoBank (a window search is pruned by search_windows(prefilter=M), which builds the "
                             "surviving windows' list on the device)")
        o.duration(duration, len(videos))
        if video_weight is not None or max_videos is not None:
            tau = o.video_level(video_weight, max_videos, tau, n_videos, gt_video, len(queries)).tau
        pf = self.prefilter_videos(videos, queries, M, tau, gt_video)
        gt_d = _upload([o.gt], np.int32, videos.device)[0] if o.gt.size else None
        r = self._search_survivor_pairs(o, videos, queries, pf["video_index"], pf["video_index"], pf["query_index"], pf["video"].shape[1],
                                        videos.cell_count, nms_thresh, max_batch, gt_d)
        r.update(prefilter_video=pf["video"], prefilter_score=pf["score"], prefilter_gt_rank=pf["gt_rank"])
        return self._search_result(r, duration, self.L)

    def _search_survivor_pairs(self, o, videos, queries, rows_d, video_d, qi_d, Ms, cell, nms_thresh, max_batch, gt_d):
        """The tail ``search(prefilter=M)`` and ``search_survivors`` share: the full model over the Q * Ms surviving pairs, sorted by (query,
        video), then the ranking.  ``rows_d (Q Ms,)`` int32: each pair's row of the bank ``videos``; ``video_d``: its video id as the
        ranking reads it (ties go to the lower video) and the result names it -- the same tensor for a VideoBank, the global ids for a
        SurvivorBank --; ``cell`` as ``_pair_chunks`` takes it; ``o``: the checked options, ``gt_d``: ``o.gt`` on the device where the
        video-level options read it.  No host read."""
        dev = videos.device
        with torch.no_grad(), torch.cuda.device(dev):
            pp_d = torch.arange(len(queries) + 1, dtype=torch.int32, device=dev) * Ms
            lists, pools = self._pair_chunks(videos, queries, rows_d, qi_d, max_batch, cell=cell, cut=(o.k_video, nms_thresh),
                                             tau=o.tau if o.ranked else None)
            return _rank_lists(o, lists, video_d, pp_d, gt_d, pools and (pools[0], pools[2]))

    # ---------------------------------------------------------------- the first-stage cut over a corpus in shards
    def _first_stage_heads(self, D):
        """The three score heads stacked as prefilter_scores reads them: ``w (3, D)``, ``b (3,)`` in the order (pm, ps, pe)."""
        lo = self.localization
        heads = (lo.conv_layer_pm, lo.conv_layer_ps, lo.conv_layer_pe)
        return torch.stack([h.weight.reshape(D) for h in heads]), torch.cat([h.bias.reshape(1) for h in heads])

    def new_survivors(self, queries, M, tau=0.1):
        """An empty SurvivorBank for the Q queries of a QueryBank: each query's best ``M`` videos by the first-stage score at
        temperature ``tau``, to be filled shard by shard with ``fold_survivors`` and searched with ``search_survivors``."""
        what = "new_survivors"
        if not isinstance(queries, QueryBank):
            raise TypeError(f"{what}: queries is a QueryBank (encode_queries)")
        require_ints(what, ("M", M, 1, PREFILTER_FOLD_MAX_M))
        tau = _temperature(what, tau)
        require_hip_tensors(what, dict(queries=queries.query_features), must="hold HIP tensors")
        dev = queries.query_features.device
        probe = torch.empty((0, self.T, self.input_video_dim), dtype=torch.float32, device=dev)
        return SurvivorBank(len(queries), int(M), tau, dev, probe)

    def fold_survivors(self, survivors, videos, queries):
        """One shard of the corpus folded into a SurvivorBank: on the shard's VideoBank ``videos``, ``prefilter_scores`` (tiled as
        prefilter_videos tiles it; every (query, video) is computed alone, so these are the bits one bank of all the videos gives),
        ``prefilter_fold`` -- the running cut: after the call each query's slots hold its best ``min(M, videos seen)`` of ALL the videos
        seen, in the order of search(prefilter=M)'s cut -- and ``survivors_admit``, which copies the admitted videos' fv rows and masks
        into the survivors' rows; the shard's bank may then be dropped.  The shard's videos get the global ids ``survivors.seen ..``.
        ValueError for a WindowBank (or a SurvivorBank), a bank encoded off the one-node path (score_pairs' message), another number of
        queries than the survivors were made for or a bank of other shapes or another storage than the earlier shards' (the survivors
        take the first shard's storage: compact shards are kept as codes).  Under torch.no_grad(); reads
        nothing back.  Returns ``survivors``."""
        what = "fold_survivors"
        if not isinstance(survivors, SurvivorBank):
            raise TypeError(f"{what}: survivors is a SurvivorBank (new_survivors)")
        _require_banks(what, videos, queries)
        if isinstance(videos, (WindowBank, SurvivorBank)):
            raise ValueError(f"{what}: a shard is a VideoBank of whole videos (pruning a window search is out of scope: the surviving windows' "
                             "list has a data-dependent length)")
        Q, V, M = len(queries), len(videos), survivors.M
        if Q != survivors.Q:
            raise ValueError(f"{what}: the survivors were made for Q = {survivors.Q} queries (got {Q})")
        _require_node_banks(videos, queries)
        shard = (videos.fv, videos.video_mask, videos.length_mask, videos.moment_mask)
        if survivors.fv is not None and any(a.shape[1:] != b.shape[1:] or a.dtype != b.dtype
                                             for a, b in zip(shard, (survivors.fv, survivors.video_mask, survivors.length_mask, survivors.moment_mask))):
            raise ValueError(f"{what}: the shard's bank differs from the earlier shards' in a shape, a mask's dtype or the storage "
                             f"({videos.storage} against {survivors.storage})")
        require_hip_tensors(what, dict(videos=videos.video_mask, queries=queries.query_features), must="hold HIP tensors")
        if survivors.seen + V > 0x7fff0000 // max(Q, 1):
            raise ValueError(f"{what}: {Q} queries over {survivors.seen + V} videos exceed the int32 pair lists")
        dev, D = videos.device, videos.fv.shape[2]
        with torch.no_grad(), torch.cuda.device(dev):
            if survivors.fv is None:
                survivors.fv, survivors.video_mask, survivors.length_mask, survivors.moment_mask = (
                    torch.zeros((Q * M,) + tuple(t.shape[1:]), dtype=t.dtype, device=dev) for t in shard)
                if videos.fv_scale is not None:                  # the survivors take the first shard's storage
                    survivors.fv_scale = torch.zeros((Q * M, videos.fv.shape[1]), dtype=torch.float32, device=dev)
            w, b = self._first_stage_heads(D)
            score, _, cells = prefilter_scores(videos.fv, queries.fs, w, b, videos.length_mask, videos.moment_mask, self.T, self.L, self.C, survivors.tau,
                                               fv_scale=videos.fv_scale)
            prefilter_fold(survivors.slot_score, survivors.slot_cells, survivors.slot_video, score, cells, survivors.seen, copy_src=survivors.copy_src)
            survivors_admit(survivors.copy_src, shard, (survivors.fv, survivors.video_mask, survivors.length_mask, survivors.moment_mask),
                            scale=videos.fv_scale, out_scale=survivors.fv_scale)
            survivors.shard_scores.append(score)
            survivors.shard_candidates.append(cells[0] > 0)          # (a video's valid cells do not depend on the query)
        survivors.seen += V
        survivors.cell_values.update(videos.cell_counts)
        return survivors

    def search_survivors(self, survivors, queries, k=5, k_video=None, nms_thresh=0.5, duration=None, max_batch=64, video_weight=None,
                         max_videos=None, n_videos=None, gt_video=None):
        """``search(prefilter=M)`` of a corpus that came in shards, once its last shard is folded: the full model runs once, over the ``Q *
        Ms`` pairs of the survivors' rows (``Ms = min(M, videos seen)``).  Each query's filled slots are put in ascending order of
        their global video (one torch.sort of (Q, Ms) ints), and the tail of search(prefilter=M) runs on them -- the chunk loop over
        the rows, the video-level options (their ``tau`` is the survivors') and smin_corpus_topk with the global video
        ids: bit for bit ``search(one bank of all the videos, prefilter=M)``, keys included -- ``prefilter_video (Q, Ms)`` int64
        ascending, ``prefilter_score (Q, V)`` and ``prefilter_gt_rank (Q,)`` (moments.prefilter_gt_rank over the kept scores: O(V) per
        query).  ``duration (V,)``, ``gt_video``: over the global ids.  Valid-cell count: when every shard's ``cell_counts`` were one
        value c, each chunk's count is ``pairs * c`` and nothing is read back; otherwise the node reads it once per chunk."""
        what = "search_survivors"
        o = _Options(what, k, k_video, max_batch)
        if not isinstance(survivors, SurvivorBank) or not isinstance(queries, QueryBank):
            raise TypeError(f"{what}: survivors is a SurvivorBank (new_survivors) and queries a QueryBank (encode_queries)")
        Q, V, M, dev = len(queries), survivors.seen, survivors.M, survivors.device
        if Q != survivors.Q:
            raise ValueError(f"{what}: the survivors were made for Q = {survivors.Q} queries (got {Q})")
        if V < 1:
            raise ValueError(f"{what}: no shard has been folded (fold_survivors)")
        o.duration(duration, V)
        if video_weight is not None or max_videos is not None:
            o.video_level(video_weight, max_videos, survivors.tau, n_videos, gt_video, Q)
        else:
            o.gt_video(gt_video, Q)
        Ms = min(M, V)
        with torch.no_grad(), torch.cuda.device(dev):
            video, order = torch.sort(survivors.slot_video[:, :Ms], dim=1)
            rows = (torch.arange(Q, dtype=torch.int32, device=dev) * M).unsqueeze(1) + order.to(torch.int32)
            qi_d = torch.arange(Q, dtype=torch.int32, device=dev).unsqueeze(1).expand(Q, Ms).reshape(-1)
            gt_d = _upload([o.gt], np.int32, dev)[0] if o.gt.size else None
            score = survivors.score
            gt_rank = prefilter_gt_rank(score, survivors.candidate, gt_d)
        r = self._search_survivor_pairs(o, survivors, queries, rows.reshape(-1), video.reshape(-1).contiguous(), qi_d, Ms, survivors.cell_count,
                                        nms_thresh, max_batch, gt_d)
        r.update(prefilter_video=video.to(torch.int64), prefilter_score=score, prefilter_gt_rank=gt_rank)
        return self._search_result(r, duration, self.L)

    # ---------------------------------------------------------------- video ranking by the pooled pair score
    def rank_videos(self, videos, queries, pairs=None, n=5, tau=0.1, gt_video=None, max_batch=64):
        """Which video: each of the Q queries' videos ranked by the pooled pair score, the score training.pair_rank_loss contrasts
         -- video retrieval only, no moment is cut.  ``videos``: a VideoBank, or a WindowBank of videos of any
        length; ``pairs`` as ``search`` takes them.  search's chunk loop with one pair_pool per chunk (log-mean-exp of the valid cells'
        fused scores at temperature ``tau``); for a WindowBank the (query, window) list is pooled and one group_pool composes each
        (query, video) group's windows (a cell in the overlap of two windows counts twice); then one smin_video_rank: higher score
        first, ties -> lower video.  A pair without a valid cell (a video without rows) is no candidate.

        Returns a dict: ``video (Q, n)`` int64 (-1 for empty slots), ``score (Q, n)`` (0), ``count (Q,)`` int32, ``pair_score (P,)`` and
        ``pair_rank (P,)`` int32 (-1 for a non-candidate) over the listed pairs sorted by (query, video), and ``gt_rank (Q,)`` int32, the
        rank of ``gt_video[q]`` (Q host ints; -1 if it is not listed or no gt_video is given).  The plan travels in one pinned
        asynchronous copy.  No host synchronisation."""
        what = "rank_videos"
        require_ints(what, ("n", n, 1, MAX_K))
        windowed = isinstance(videos, WindowBank)
        if windowed:
            o, p = self._window_search_plan(what, videos, queries, pairs, 1, 1, 1, max_batch, None)
            vi, pair_ptr, rest = p["vi"], p["query_ptr"], [p["wi"], p["wq"], p["group_ptr"]]
        else:
            o, vi, qi, pair_ptr = self._search_plan(what, videos, queries, pairs, 1, 1, max_batch, None)
            rest = [qi]
        require_hip_tensors(what, dict(videos=videos.video_mask, queries=queries.query_features), must="hold HIP tensors")
        o.video_level(None, None, tau, int(n), gt_video, len(queries))
        with torch.no_grad(), torch.cuda.device(videos.device):
            vi_d, pp_d, gt_d, *rest_d = _upload([vi, pair_ptr, o.gt] + rest, np.int32, videos.device)
            if windowed:
                _, (_, pool, cells) = self._pair_chunks(videos, queries, rest_d[0], rest_d[1], max_batch, host=(p["wi"], p["wq"]), tau=o.tau)
                score, cells = group_pool(pool, cells, rest_d[2], o.tau)
            else:
                _, (score, _, cells) = self._pair_chunks(videos, queries, vi_d, rest_d[0], max_batch, host=(vi, qi), tau=o.tau)
            vr = rank_videos(score, cells, vi_d, pp_d, n=o.n_videos, alpha=0.0, gt_video=gt_d if o.gt.size else None)
        return dict(video=vr["video"], score=vr["score"], count=vr["count"], pair_score=score, pair_rank=vr["pair_rank"], gt_rank=vr["gt_rank"])

    # ---------------------------------------------------------------- corpus search over long videos
    def encode_windows(self, raw, lengths, window=None, stride=None, mode="pick", max_batch=64, storage="fp32"):
        """A WindowBank of the W windows of V videos of any length: sampling.window_plan's overlapping windows of ``window`` raw rows
        (default T: one row per clip) every ``stride`` rows (default window // 2), each resampled to T clips and encoded once --
        chunk by chunk, at most ``max_batch`` windows each: sample_windows, build_masks_hip, encode_videos (smin_hip::smin_encode_videos).
        ``raw (R, Din)`` HIP float32 tensor of the videos' rows back to back and ``lengths`` their V row counts (host), as
        localize_windows takes them.  A video of 0 rows has no window.  The windows' valid-cell counts come from the host plan
        (feeder.cell_count of min(len, T)) and the plan travels in one pinned asynchronous copy: nothing is read back.  The sampled
        features are dropped chunk by chunk on the one-node path (WindowBank).  ``storage``: encode_videos' -- each chunk's windows are
        encoded to codes as they come, so the fp32 ``fv`` of all windows never exists.  Under torch.no_grad(); stale after a parameter
        update."""
        T, L = self.T, self.L
        require_storage("encode_windows", storage)
        window = T if window is None else window
        stride = max(int(window) // 2, 1) if stride is None else stride
        require_ints("encode_windows", ("window", window, 1, MAX_ROWS), ("stride", stride, 1, MAX_ROWS), ("max_batch", max_batch, 1, 65535))
        if mode not in MODES:
            raise ValueError(f"encode_windows: mode must be one of {sorted(MODES)} (got {mode!r})")
        require_hip_tensors("encode_windows", dict(raw=raw))
        if raw.dim() != 2 or raw.dtype != torch.float32 or raw.shape[1] % 4 != 0 or raw.shape[1] != self.input_video_dim:
            raise ValueError(f"encode_windows: raw must be float32 (R, Din = {self.input_video_dim}) with Din % 4 == 0 (got "
                             f"{tuple(raw.shape)} {raw.dtype})")
        n = host_array(lengths)
        if n.size and n.min() < 0 or int(n.sum()) != raw.shape[0]:
            raise ValueError(f"encode_windows: lengths must be >= 0 and sum to raw's {raw.shape[0]} rows (got {int(n.sum())})")
        starts, lens, vptr = (x.numpy() for x in window_plan(n, window, stride))
        V, W, dev, Din = n.shape[0], starts.shape[0], raw.device, raw.shape[1]
        offs = np.concatenate([[0], np.cumsum(n)]).astype(np.int64)
        row_begin = offs[np.repeat(np.arange(V), vptr[1:] - vptr[:-1])] + starts
        cells = [cell_count(x, T, L) for x in np.minimum(lens, T)]                              # per window, as csrc/labels.hip forms it
        probe = raw.new_empty((0, T, Din))                                                     # what SMIN._plan reads of the windows' features
        keep = not self._bank_plan(probe, probe)                                               # (the query side's dtype is checked when pairs are scored)
        with torch.no_grad(), torch.cuda.device(dev):
            # the whole plan in one pinned buffer, one asynchronous copy (the call never waits for the device)
            rb_d, st_d, ln_d, vp_d = _upload([row_begin, starts, lens, vptr], np.int64, dev)
            ln_d = ln_d.to(torch.int32)
            vmask = torch.empty((W, T, 1), dtype=torch.uint8, device=dev)
            lmask = torch.empty((W, L), dtype=torch.bool, device=dev)
            mmask = torch.empty((W, L, L), dtype=torch.bool, device=dev)
            feats = torch.empty((W, T, Din), dtype=torch.float32, device=dev) if keep else None
            fv = fv_scale = None
            for c0 in range(0, W, max_batch):
                c1 = min(c0 + max_batch, W)
                vf, nfeats = sample_windows(raw, rb_d[c0:c1], ln_d[c0:c1], T, mode=mode)
                m = build_masks_hip(nfeats, T, L)
                part = self.encode_videos(vf, m["video_mask"], m["length_mask"], m["moment_mask"], cell_counts=cells[c0:c1], storage=storage)
                vmask[c0:c1], lmask[c0:c1], mmask[c0:c1] = part.video_mask, part.length_mask, part.moment_mask
                if part.fv is not None:
                    fv = torch.empty((W,) + tuple(part.fv.shape[1:]), dtype=part.fv.dtype, device=dev) if fv is None else fv
                    fv[c0:c1] = part.fv
                    if part.fv_scale is not None:
                        fv_scale = torch.empty((W, part.fv.shape[1]), dtype=torch.float32, device=dev) if fv_scale is None else fv_scale
                        fv_scale[c0:c1] = part.fv_scale
                if keep:
                    feats[c0:c1] = vf
        return WindowBank(fv, feats, vmask, lmask, mmask, cells, starts, lens, vptr, n, st_d, ln_d, vp_d, window, stride, mode, plan_features=probe,
                          fv_scale=fv_scale)

    def _window_search_plan(self, what, windows, queries, pairs, k, k_video, k_window, max_batch, duration):
        """search_windows' checked arguments and its expansion, host arithmetic only: ``(options, plan)`` with ``options`` an _Options
        (``k``, ``k_video`` and ``k_window`` as ints, their defaults filled in) and ``plan`` a dict of numpy int64 arrays -- ``vi`` / ``qi
        (G2,)`` the (query, video) groups sorted by (query, video), ``wi`` / ``wq (G,)`` the (query, window) list (each group's windows in
        start order, ``wi`` a global window of the bank), ``group_ptr (G2 + 1,)`` over that list and ``query_ptr (Q + 1,)`` over the groups."""
        o = _Options(what, k, k_video, max_batch, k_window, windows=True)
        if not isinstance(windows, WindowBank) or not isinstance(queries, QueryBank):
            raise ValueError(f"{what}: windows is a WindowBank (encode_windows) and queries a QueryBank (encode_queries)")
        V, Q = windows.n_videos, len(queries)
        vi, qi, query_ptr = self._listed_pairs(what, pairs, V, Q)
        o.duration(duration, V)
        vptr = windows.video_ptr
        nw = (vptr[1:] - vptr[:-1])[vi]                                                        # windows per group; 0 for a video without rows
        group_ptr = np.concatenate([[0], np.cumsum(nw)]).astype(np.int64)
        G2, G = vi.shape[0], int(group_ptr[-1])
        if G * o.k_window >= 2 ** 31 or G2 >= 2 ** 31:
            raise ValueError(f"{what}: {G} (query, window) pairs of {o.k_window} moments in {G2} groups exceed the merges' 2**31 candidates / groups")
        wi = np.concatenate([np.arange(vptr[v], vptr[v + 1]) for v in vi]).astype(np.int64) if G else np.zeros(0, np.int64)
        return o, dict(vi=vi, qi=qi, wi=wi, wq=np.repeat(qi, nw), group_ptr=group_ptr, query_ptr=query_ptr)

    @staticmethod
    def _window_result(r, duration, n_rows):
        if duration is not None:
            r["times"] = window_times(r["video"], r["span"], duration, n_rows)       # moments' one formula, on each entry's own video
        return r

    def search_windows(self, windows, queries, pairs=None, k=5, k_video=None, k_window=None, nms_thresh=0.5, duration=None, max_batch=64,
                       video_weight=None, max_videos=None, tau=0.1, n_videos=None, gt_video=None, prefilter=None, trim=False, carry=False):
        """Which video, and where, over videos of any length: the k best moments of each of the Q queries of a QueryBank over the videos
        of a WindowBank, at the windows' native resolution.

        ``pairs``: None -- every query against every video --, or a host (P, 2) array of (query, video) rows, in any order (sorted here
        by (query, video)); a repeated pair raises ValueError.  Each pair expands to its video's windows in start order (a video
        without rows: none).  The (query, window) list is scored in chunks of at most ``max_batch`` -- score_pairs from the banks, no
        encoder runs again, each chunk's valid-cell count the sum of the bank's cell_counts -- and each chunk is cut to ``k_window``
        (default k_video) moments per window by top_moments' kernels.  One smin_merge_window_moments then merges each (query, video)
        group's windows by greedy NMS in raw-row time into ``k_video`` (default k) moments, and one smin_corpus_span_topk ranks each
        query's moments across its videos: higher score first, ties -> lower video, then lower slot.

        Returns a dict: ``video (Q, k)`` int64 (-1 for empty slots), ``span (Q, k, 2)`` float32 raw rows of that video (NaN),
        ``score (Q, k)`` (0), ``window (Q, k)`` int64 the window's ordinal within its video (-1), ``cell (Q, k, 2)`` int64 (-1),
        ``count (Q,)`` int32; with ``duration (V,)`` seconds also ``times (Q, k, 2) = (span * duration[video]) / n_rows[video]`` (fp32, NaN
        for empty slots).  The whole plan travels in one pinned asynchronous copy.  No host synchronisation.

        ``video_weight`` / ``max_videos`` / ``tau`` / ``n_videos`` / ``gt_video``: as ``search`` takes them (both of the first two None:
        the search above, untouched).  Each chunk's (query, window) scores are also pooled (pair_pool), one group_pool composes a (query,
        video) group's windows into the group's score, and smin_video_rank and smin_moment_reweight act on the groups' merged lists in
        front of the same smin_corpus_span_topk; the result gains ``video_rank``, ``video_score``, ``video_count`` and ``gt_rank``.

        ``carry=True``: as ``search`` takes it (``pairs`` must be None), for moments.merge_search_windows_weighted:
        ``raw (Q, k)`` holds the bits of the entry's score in its group's merge_window_moments list, matched by (video, window, cell), and
        ``pair_score`` / ``pair_cells (Q, V)`` are the group_pool outputs.

        ``prefilter=M`` (None: everything above, untouched) prunes the videos before the model runs, as ``search(prefilter=M)`` does
        (INTEGRATION.md 3za): ``prefilter_videos`` pools the first-stage scores of every (query, window) into per-video scores and keeps
        each query's best ``Ms = min(M, V)`` videos, moments.expand_survivor_windows turns them into the (query, window) list and its group
        pointers on the device, and the chunk loop, the merge and the ranking above run over that list: the model scores the windows of
        Q * Ms videos instead of Q * V.  The list's length depends on which videos survive, so it is built at a capacity the host can
        bound without a read -- ``cap`` = moments.survivor_window_capacity: Q times the sum of the Ms largest per-video window counts --
        and the slots behind the real ones hold window 0 and query 0.  ``trim=False``: no host read and no synchronisation; the chunk
        loop runs over all ``cap`` slots, so THE MODEL ALSO SCORES THE PADDING (no group owns it; it costs time, not results): nothing
        where every video has one window count, up to most of the work where a few videos are much longer than the rest.
        ``trim=True`` reads the real length once (ONE small host read, a synchronisation) and runs the loop over the real slots only:
        for corpora whose window counts are very unequal.  Each chunk's valid-cell count follows ``search(prefilter=M)``'s rule on the
        windows' ``cell_counts``.  ``video_weight`` / ``max_videos`` / ``gt_video`` / ``tau`` act on the surviving pairs (``tau`` is also
        the first stage's temperature).  With ``pairs`` or ``carry=True``: ValueError.  The result gains ``prefilter_video (Q, Ms)``
        int64 ascending, ``prefilter_score (Q, V)``, ``prefilter_gt_rank (Q,)`` int32 and ``window_pairs (1,)`` int64, the real slots
        (with ``cap`` it tells how much padding was scored).  What the pruning loses is not bounded."""
        if prefilter is not None:
            if pairs is not None or carry:
                raise ValueError("search_windows: prefilter takes pairs=None and carry=False (it chooses the pairs itself, and a carried merge "
                                 "needs every video's pooled score)")
            return self._search_windows_prefiltered(windows, queries, prefilter, trim, k, k_video, k_window, nms_thresh, duration, max_batch,
                                                    video_weight, max_videos, tau, n_videos, gt_video)
        if carry and pairs is not None:
            raise ValueError("search_windows: carry=True takes pairs=None, every query against every video of the bank (a merge re-ranks all the "
                             "shard's videos)")
        if carry and video_weight is None and max_videos is None:
            video_weight = 0.0
        o, p = self._window_search_plan("search_windows", windows, queries, pairs, k, k_video, k_window, max_batch, duration)
        if video_weight is not None or max_videos is not None:
            o.video_level(video_weight, max_videos, tau, n_videos, gt_video, len(queries))
        require_hip_tensors("search_windows", dict(windows=windows.video_mask, queries=queries.query_features), must="hold HIP tensors")
        dev, Q, V = windows.device, len(queries), windows.n_videos
        with torch.no_grad(), torch.cuda.device(dev):
            # the whole plan in one pinned buffer, one asynchronous copy (the call never waits for the device)
            wi_d, wq_d, gp_d, vid_d, qp_d, nr_d, gt_d = _upload([p["wi"], p["wq"], p["group_ptr"], p["vi"], p["query_ptr"], windows.n_rows, o.gt],
                                                                np.int64, dev)
            wi32, wq32 = wi_d.to(torch.int32), wq_d.to(torch.int32)
            r, g, pooled = self._window_search_tail(o, windows, queries, wi_d, wi32, wq32, gp_d, lambda: (vid_d.to(torch.int32), qp_d.to(torch.int32)),
                                                    gt_d, nms_thresh, max_batch, host=(p["wi"], p["wq"]))
            if carry:
                r["raw"] = _carry_raw(r["video"], (r["window"].unsqueeze(-1), r["cell"]), (g["window"].unsqueeze(-1), g["cell"]), g["score"],
                                      g["count"], V)
                r["pair_score"], r["pair_cells"] = pooled[0].reshape(Q, V), pooled[1].reshape(Q, V)
        return self._window_result(r, duration, nr_d)

    def _window_search_tail(self, o, windows, queries, rows_d, wi32, wq32, gp_d, narrow, gt_d, nms_thresh, max_batch, host=None, cell=None):
        """What every window search runs behind its plan: the chunk loop over the (query, window) list ``wi32`` / ``wq32`` (int32, on the
        device; ``host`` / ``cell`` as ``_pair_chunks`` takes them), one merge_window_moments over the groups of ``gp_d`` (int64; slots no
        group owns are scored and dropped) with ``start`` / ``len`` gathered by ``rows_d`` (the list as an index), group_pool with the
        video-level options, and the ranking.  ``narrow() -> (video, query_ptr)``: the groups' lists as int32, formed where each mode has
        always formed them -- in front of the loop with the video-level options, behind the merge without --, so the device sees the same
        launches in the same order.  Returns ``(result, the groups' merged lists, the groups' pooled (score, cells) or None)``.  No host
        read."""
        groups = narrow() if o.ranked else None
        lists, pools = self._pair_chunks(windows, queries, wi32, wq32, max_batch, host=host, cell=cell, cut=(o.k_window, nms_thresh),
                                         tau=o.tau if o.ranked else None)
        g = merge_window_moments(lists["idx"], lists["score"], lists["count"], windows.start.index_select(0, rows_d),
                                 windows.len.index_select(0, rows_d), gp_d, self.T, self.L, k=o.k_video, nms_thresh=nms_thresh)
        pooled = group_pool(pools[1], pools[2], gp_d, o.tau) if o.ranked else None
        return _rank_lists(o, g, *(groups or narrow()), gt_d, pooled), g, pooled

    def _search_windows_prefiltered(self, windows, queries, M, trim, k, k_video, k_window, nms_thresh, duration, max_batch, video_weight,
                                    max_videos, tau, n_videos, gt_video):
        """``search_windows(prefilter=M)``: prefilter_videos, the device-built window plan (moments.expand_survivor_windows) at the host's
        capacity bound, then search_windows' own tail."""
        what = "search_windows"
        o = _Options(what, k, k_video, max_batch, k_window, windows=True)
        if not isinstance(windows, WindowBank) or not isinstance(queries, QueryBank):
            raise ValueError(f"{what}: windows is a WindowBank (encode_windows) and queries a QueryBank (encode_queries)")
        require_ints(what, ("prefilter", M, 1, 2 ** 31 - 1))
        Q, V, W, dev = len(queries), windows.n_videos, len(windows), windows.device
        o.duration(duration, V)
        if video_weight is not None or max_videos is not None:
            tau = o.video_level(video_weight, max_videos, tau, n_videos, gt_video, Q).tau
        Ms = min(int(M), V)
        cap = survivor_window_capacity(windows.video_ptr, Ms, Q)
        if cap * o.k_window >= 2 ** 31:
            raise ValueError(f"{what}: {cap} (query, window) slots of {o.k_window} moments exceed the merges' 2**31 candidates")
        pf = self.prefilter_videos(windows, queries, int(M), tau, gt_video)
        with torch.no_grad(), torch.cuda.device(dev):
            nr_d, gt_d = _upload([windows.n_rows, o.gt], np.int64, dev)
            sel = pf["video"].to(torch.int32)
            gp_d, wi32, wq32, total = expand_survivor_windows(sel, windows.video_ptr_d, W, cap)
            if trim:
                n = min(int(total.item()), cap)                                       # the one host read of trim=True
                wi32, wq32 = wi32[:n], wq32[:n]
            narrow = lambda: (sel.reshape(-1), torch.arange(Q + 1, dtype=torch.int32, device=dev) * Ms)
            r, _, _ = self._window_search_tail(o, windows, queries, wi32, wi32, wq32, gp_d, narrow, gt_d if o.gt.size else None, nms_thresh,
                                               max_batch, cell=windows.cell_count)
        r.update(prefilter_video=pf["video"], prefilter_score=pf["score"], prefilter_gt_rank=pf["gt_rank"], window_pairs=total)
        return self._window_result(r, duration, nr_d)

    def search_windows_torch(self, windows, queries, raw=None, pairs=None, k=5, k_video=None, k_window=None, nms_thresh=0.5, duration=None,
                             max_batch=64, scorer=None, pair_rank=None, weight=None, max_videos=None):
        """``search_windows`` restated: the same expansion and chunking, each chunk's windows sampled from ``raw`` (encode_windows'
        ``raw``) and scored with their queries by localize_windows' own route (sample_windows, build_masks_hip, score() / the forward),
        cut by top_moments, merged per group by moments.merge_window_moments_torch and ranked by moments.corpus_span_topk_torch.  Kept
        under its own name as what the tests compare against -- nothing routes here.  ``scorer(window_index, query_index) -> (pm, ps,
        pe, pa)`` replaces the sampling and the model on a chunk's (window, query) pairs (the tests feed it score_pairs, to compare the
        selection on equal scores; with it ``raw`` is not read, and on CPU banks the cut is top_moments_torch).  ``pair_rank`` / ``weight
        (G2,)`` with ``max_videos``: moments.reweight_moments_torch on the groups' merged lists in front of the ranking (the tests feed it
        the kernels' ranks and weights of ``search_windows(video_weight=..., max_videos=...)``)."""
        what = "search_windows_torch"
        windows = windows.dequantized() if isinstance(windows, VideoBank) else windows
        o, p = self._window_search_plan(what, windows, queries, pairs, k, k_video, k_window, max_batch, duration)
        k, k_video, k_window = o.k, o.k_video, o.k_window
        if scorer is None and raw is None:
            raise ValueError(f"{what}: needs raw, the rows the bank was encoded from, or a scorer")
        dev, T, L, G = windows.device, self.T, self.L, p["wi"].shape[0]
        cut_moments = top_moments if dev.type == "cuda" else top_moments_torch
        idx, score, count, chunks = _chunk_buffers(G, k_window, max_batch, dev)
        offs = np.concatenate([[0], np.cumsum(windows.n_rows)]).astype(np.int64)
        video_of = np.repeat(np.arange(windows.n_videos), windows.video_ptr[1:] - windows.video_ptr[:-1])
        qm = queries.query_mask[:, :queries.query_features.shape[1]]
        with torch.no_grad():
            for c0, c1 in chunks:
                wi, wq = p["wi"][c0:c1], p["wq"][c0:c1]
                if scorer is not None:
                    pm, ps, pe, _ = scorer(wi, wq)
                    mm = windows.moment_mask.index_select(0, torch.from_numpy(wi).to(dev))
                else:
                    vf, nfeats = sample_windows(raw, (offs[video_of[wi]] + windows.starts[wi]).tolist(), windows.lens[wi].tolist(), T, mode=windows.mode)
                    m = build_masks_hip(nfeats, T, L)
                    wq_d = torch.from_numpy(wq).to(dev)
                    mm = m["moment_mask"]
                    pm, ps, pe, _ = self._scores(vf, m["video_mask"], queries.query_features.index_select(0, wq_d), qm.index_select(0, wq_d),
                                                 m["length_mask"], mm)
                t = cut_moments(pm, ps, pe, mm, k=k_window, nms_thresh=nms_thresh)
                idx[c0:c1], score[c0:c1], count[c0:c1] = t["idx"], t["score"], t["count"]
            on = lambda a, dt=torch.int64: torch.from_numpy(np.ascontiguousarray(a)).to(device=dev, dtype=dt)
            g = merge_window_moments_torch(idx, score, count, on(windows.starts[p["wi"]]), on(windows.lens[p["wi"]], torch.int32), on(p["group_ptr"]),
                                           T, L, k=k_video, nms_thresh=nms_thresh)
            if weight is not None:
                g["score"], g["count"] = reweight_moments_torch(g["score"], g["count"], pair_rank, weight, max_videos)
            r = corpus_span_topk_torch(g["span"], g["score"], g["window"], g["cell"], g["count"], on(p["vi"], torch.int32),
                                       on(p["query_ptr"], torch.int32), k=k)
            return r if duration is None else self._window_result(r, duration, on(windows.n_rows))

    # ---------------------------------------------------------------- hard-negative mining
    def pair_scores(self, videos, queries, max_batch=64, pool=None, tau=0.1):
        """``(Q, V)`` float32: the best fused moment score of every (query, video) pair of a QueryBank and a VideoBank -- search's chunk
        loop over all pairs at one moment per pair, so the bits of ``top_moments(*score_pairs(all pairs)[:3], moment_mask, k=1)``'s
        slot 0; 0 for a pair without a valid cell.  ``pool="lme"``: the pooled pair score at temperature ``tau`` instead -- the bits of
        ``moments.pair_pool`` on the same scores, the score training.pair_rank_loss contrasts.  Under
        torch.no_grad(); no host read."""
        if pool not in (None, "lme"):
            raise ValueError(f"pair_scores: pool must be None (the best moment) or 'lme' (the pooled pair score), got {pool!r}")
        _, vi, qi, _ = self._search_plan("pair_scores", videos, queries, None, 1, 1, max_batch, None)
        dev = videos.device
        with torch.no_grad(), torch.cuda.device(dev):
            vi_d, qi_d = _upload([vi, qi], np.int32, dev)
            if pool == "lme":
                score = self._pair_chunks(videos, queries, vi_d, qi_d, max_batch, host=(vi, qi), tau=_temperature("pair_scores", tau))[1][0]
            else:
                score = self._pair_chunks(videos, queries, vi_d, qi_d, max_batch, host=(vi, qi), cut=(1, 1.0))[0]["score"]   # (an empty slot's score is 0)
        return score.reshape(len(queries), len(videos))

    def mine_pairs(self, videos, queries, gt_video, negatives, skip=0, max_batch=64, pool=None, tau=0.1):
        """The pairs to train on, chosen by the model: for each query of the QueryBank its own video ``gt_video[q]`` (Q host ints) and
        the ``negatives`` wrong videos of the VideoBank it scores highest after the ``skip`` hardest -- ``pair_scores``, then
        moments.mine_pairs.  Returns a device-built PairPlan of Q * (1 + negatives) pairs for ``forward_pairs(plan=...)`` and
        training.pair_targets.  The banks are a snapshot of the parameters, and so is the choice.  ``pool`` / ``tau``: pair_scores' --
        ``pool="lme"`` mines by the pooled pair score the contrastive term contrasts, None by the best moment.  No host read."""
        return mine_pairs(self.pair_scores(videos, queries, max_batch, pool=pool, tau=tau), gt_video, negatives, skip)

    def search_torch(self, videos, queries, pairs=None, k=5, k_video=None, nms_thresh=0.5, duration=None, max_batch=64, scorer=None,
                     pair_rank=None, weight=None, max_videos=None):
        """``search`` restated: the same plan and chunking, each chunk's pairs expanded and scored by score(), cut by top_moments and
        merged by moments.corpus_topk_torch.  Kept under its own name as what the tests compare against -- nothing routes here.
        ``scorer(video_index, query_index) -> (pm, ps, pe, pa)`` replaces score() on the expanded pairs (the tests feed it
        score_pairs, to compare the ranking on equal scores).  ``pair_rank`` / ``weight (P,)`` with ``max_videos``:
        moments.reweight_moments_torch on the pairs' lists in front of the ranking (the tests feed it the kernels' ranks and weights of
        ``search(video_weight=..., max_videos=...)``)."""
        videos = videos.dequantized() if isinstance(videos, VideoBank) else videos
        o, vi, qi, pair_ptr = self._search_plan("search_torch", videos, queries, pairs, k, k_video, max_batch, duration)
        k, k_video, dev, L, P = o.k, o.k_video, videos.device, self.L, vi.shape[0]
        idx, score, count, chunks = _chunk_buffers(P, k_video, max_batch, dev)
        with torch.no_grad():
            for c0, c1 in chunks:
                vi_d, qi_d = (torch.from_numpy(x[c0:c1].copy()).to(dev) for x in (vi, qi))
                mm = videos.moment_mask.index_select(0, vi_d)
                if scorer is not None:
                    pm, ps, pe, _ = scorer(vi[c0:c1], qi[c0:c1])
                else:
                    qm = queries.query_mask[:, :queries.query_features.shape[1]]
                    pm, ps, pe, _ = self.score(videos.video_features.index_select(0, vi_d), videos.video_mask.index_select(0, vi_d),
                                               queries.query_features.index_select(0, qi_d), qm.index_select(0, qi_d),
                                               videos.length_mask.index_select(0, vi_d), mm)
                t = top_moments(pm, ps, pe, mm, k=k_video, nms_thresh=nms_thresh)
                idx[c0:c1], score[c0:c1], count[c0:c1] = t["idx"], t["score"], t["count"]
        if weight is not None:
            score, count = reweight_moments_torch(score, count, pair_rank, weight, max_videos)
        r = corpus_topk_torch(score, idx, count, torch.from_numpy(vi).to(dev), torch.from_numpy(pair_ptr).to(dev), k=k)
        return self._search_result(r, duration, L)

