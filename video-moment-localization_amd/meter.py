"""An epoch's loss and retrieval metrics accumulated on the device: one host read per epoch instead of two per batch.

The reference's loops (main.py:135-211) read ``loss.item()`` and the counts of ``compute_ious`` back on every batch, so the host
cannot enqueue step n + 1 while step n runs.  ``EpochMeter.update`` enqueues the same per-sample metric stage as ``compute_ious``
(csrc/metrics.hip, csrc/moments.hip) followed by one closing wave that adds the batch's sums to an fp64 accumulator in device
memory; ``result()`` is the only read.

State ``acc`` (fp64, ``4 + len(n) * len(m)`` values; include/smin_hip.h, smin_epoch_meter_update):
  ``[0]`` samples seen; ``[1]`` sum of ``float64(loss) * B`` over the updates that carried a loss; ``[2]`` samples of those updates;
  ``[3]`` sum of the top-1 IoU (``sm`` at the sample's first kept cell, 0 if it keeps none);
  ``[4 + a * len(m) + c]`` samples with a hit for ``(n[a], m[c])``.
Every batch sum is ``s = 0.0; for b in range(B): s += float64(x[b])``, then ``acc[slot] += s``: a fixed order, so
``EpochMeterTorch`` -- the same class as plain torch ops on any device, the restatement the tests compare against; nothing routes
to it -- reproduces ``EpochMeter.state`` bit for bit.

``update_spans(span, count, gt)`` adds a batch of merged spans (``SMIN.localize_windows`` / ``merge_window_moments`` output) measured
against ground-truth spans instead (include/smin_hip.h, smin_span_meter_update): slot 0, the top-1 IoU sum and the hit slots, with the
meter's own n / m; the rule (``nms_thresh``) plays no part, and a meter may mix both kinds of update.

``CorpusMeter`` / ``CorpusMeterTorch`` keep the numbers of corpus search the same way (include/smin_hip.h,
smin_corpus_meter_update): ``update(result, gt_video, gt)`` takes a ranked list over a corpus (``SMIN.search`` /
``merge_search`` output) and one ground-truth moment of one ground-truth video per query.  State: ``4 + len(n) * len(m) + len(n)``
values -- ``[0]`` queries, ``[1]`` / ``[2]`` unused, ``[3]`` the top-1 IoU sum (an entry of another video has IoU 0),
``[4 + a * len(m) + c]`` VCMR hits (the moment of the right video among the top n[a] with IoU > m[c]), ``[4 + len(n) * len(m) + a]`` VR
hits (the right video among the first n[a] distinct videos of the list).

All updates of one meter must be issued on one stream (the accumulator is ordered by the stream alone, no atomics)."""
import ctypes

import torch

from ._host import byte_mask
from .moments import MAX_K, _check, _fused, _mul32, _nm_check, _span_check, _span_meter_call, _valid_slots, span_ious_torch

_REF_N, _REF_M = (1, 5), (0.1, 0.3, 0.5, 0.7)


def _status_word(device):
    """The device's ``layout_status`` word (set by a forward whose ``known_cell_count`` did not match its mask) as a (1,) int32
    tensor, or None where no forward of the one-node path can have run (CPU, or the extension was never loaded)."""
    from . import _lib
    if torch.device(device).type != "cuda" or _lib._torch_ops is None:
        return None
    return _lib._torch_ops.layout_status(torch.device(device))


def _lstm_cluster_error(device):
    """1 once a poll of the cluster LSTM has expired since the last call (smin_lstm_cluster_error; clears the word), else 0."""
    from . import _lib
    if torch.device(device).type != "cuda":
        return 0
    with torch.cuda.device(device):
        return int(_lib.load().smin_lstm_cluster_error())


class _Meter:
    def __init__(self, n=_REF_N, m=_REF_M, nms_thresh=None, device=None, nms="hard", sigma=0.5):
        self.n, self.m = tuple(n), tuple(m)
        from .moments import soft_rule
        self.nms, self.sigma = nms, float(sigma)
        self._soft = soft_rule(type(self).__name__, nms, 1.0 if nms_thresh is None else nms_thresh, sigma, None)   # ValueError: bad nms / sigma
        if self._soft is not None and nms_thresh is None:
            raise ValueError(f"{type(self).__name__}: nms={nms!r} ranks the valid cells like the nms_thresh rule; pass nms_thresh")
        self.keys = [f"R@{n_}, IoU={m_}" for n_ in self.n for m_ in self.m]
        if nms_thresh is None:
            if self.n != _REF_N or self.m != _REF_M:
                raise ValueError(f"the meter's reference rule (nms_thresh=None) takes n = {_REF_N} and m = {_REF_M} only (got n={self.n}, "
                                 f"m={self.m}); pass nms_thresh (>= 1 for plain top-k over the valid cells) for other lists")
            self.rule, self.nms_thresh = 0, None
            self._n, self._m, self.k = list(_REF_N), list(_REF_M), 5
        else:
            self.rule, self.nms_thresh = 1, float(nms_thresh)
            self._n, self._m = _nm_check(self.n, self.m)                 # ValueError: more than 64 n / 16 m, or an n outside 1..64
            self.k = max(self._n)
            assert self.k <= MAX_K
        self.device = torch.device(self._default_device() if device is None else device)
        self.state = torch.zeros(4 + len(self.keys), dtype=torch.float64, device=self.device)

    def reset(self):
        self.state.zero_()

    def _spans_check(self, span, count, gt):
        B, k = _span_check(span, count, gt)                                  # ValueError: shapes, or more than 64 slots
        if k < max(self._n):
            raise ValueError(f"update_spans: the meter's R@{max(self._n)} needs at least {max(self._n)} slots per pair (span has k = {k})")
        return B, k

    def result(self, group=None):
        """The one host read: ``{"R@n, IoU=m": hits / samples, ..., "mIoU": ..., "num_samples": ...}`` plus ``"loss"`` when an
        update carried one (the divisions of main.py:162-163, 188-189).  ``group``: a torch.distributed process group whose
        ranks' states are summed first (the meter's own state is left as it is).  Raises RuntimeError, naming the word, when the
        device's ``layout_status`` word (a batch's ``cell_count`` did not match its ``moment_mask``; cleared here) or the cluster
        LSTM's poll-expiry word is set: the epoch's numbers are then meaningless."""
        st = self.state
        if group is not None:
            st = st.clone()
            torch.distributed.all_reduce(st, op=torch.distributed.ReduceOp.SUM, group=group)
        status = _status_word(self.device)
        if status is None:
            acc, bad = st.tolist(), 0
        else:
            vals = torch.cat([st, status.to(device=st.device, dtype=torch.float64)]).tolist()
            acc, bad = vals[:-1], int(vals[-1])
        expired = _lstm_cluster_error(self.device)
        if bad:
            status.zero_()
        if bad or expired:
            what = ["layout_status (a batch ran with a cell count that did not match its moment_mask)"] * bool(bad) \
                + ["smin_lstm_cluster_error (a poll of the cluster LSTM expired)"] * bool(expired)
            raise RuntimeError("EpochMeter.result: " + " and ".join(what) + " was set during the epoch; its results are meaningless")
        num = acc[0]
        out = {k: acc[4 + q] / num for q, k in enumerate(self.keys)}
        out["mIoU"] = acc[3] / num
        out["num_samples"] = int(num)
        if acc[2] > 0:
            out["loss"] = acc[1] / acc[2]
        return out


class EpochMeter(_Meter):
    """``EpochMeter(n=(1, 5), m=(0.1, 0.3, 0.5, 0.7), nms_thresh=None, device=...)``: ``nms_thresh=None`` is the reference's rule
    (``compute_ious``'s kernel; only the reference's n / m -- ``compute_ious`` sends other lists to its torch form, which the meter
    does not offer); a number selects greedy temporal NMS over the valid cells (``compute_ious(..., nms_thresh=t)``, same limits).
    With a number, ``nms="linear"`` / ``"gaussian"`` (and ``sigma``) rank by Soft-NMS instead (``compute_ious(..., nms=...)``).

    ``update(pm, ps, pe, moment_mask, sm, loss=None)`` enqueues the kernels on the current stream and returns nothing; ``loss``
    is the device scalar ``loss_fn`` returned.  HIP tensors only.  ``result()`` reads, ``reset()`` zeroes, ``state`` is the fp64
    device tensor."""

    @staticmethod
    def _default_device():
        return "cuda"

    def update(self, pm, ps, pe, moment_mask, sm, loss=None):
        from ._lib import SminHipError, call_ws, ptr, stream
        for t in (pm, ps, pe, moment_mask, sm) + (() if loss is None else (loss,)):
            if not t.is_cuda:
                raise SminHipError("EpochMeter.update runs on a HIP device only (got a CPU tensor); there is no CPU fallback -- the plain-torch "
                                   "restatement is available under the explicit name EpochMeterTorch")
        if pm.device != self.state.device:
            raise ValueError(f"EpochMeter on {self.state.device} got tensors on {pm.device}")
        B, L = _check(pm, ps, pe, moment_mask, 1)
        if self.rule == 0 and L * L < 5:
            raise ValueError("the meter's reference rule takes the top five of L*L cells: L*L >= 5")
        if tuple(sm.shape) != (B, L, L) or (loss is not None and loss.numel() != 1):
            raise ValueError(f"sm must be (B, L, L) = {(B, L, L)} and loss a scalar (got {tuple(sm.shape)}, "
                             f"{None if loss is None else tuple(loss.shape)})")
        pm_, ps_, pe_, sm_ = (x.detach().float().contiguous() for x in (pm, ps, pe, sm))
        mm_ = byte_mask(moment_mask)
        loss_ = None if loss is None else loss.detach().float().reshape(1).contiguous()
        nl, ml = (ctypes.c_int * len(self._n))(*self._n), (ctypes.c_float * len(self._m))(*self._m)
        nn, nm = len(self._n), len(self._m)
        if self._soft is None:
            name, query = "smin_epoch_meter_update", "smin_epoch_meter_ws_bytes"
            shape, fields = (B, L, self.rule, self.k), "B, L, rule, k, nn, nm"
            how = (1.0 if self.nms_thresh is None else self.nms_thresh,)
        else:                                                    # rule 1 with the Soft-NMS selection
            name, query = "smin_epoch_meter_update_soft", "smin_epoch_meter_soft_ws_bytes"
            shape, fields = (B, L, self.k), "B, L, k, nn, nm"
            how = self._soft[:3]
        with torch.cuda.device(pm.device):
            call_ws(name, shape + (nn, nm), stream(), ptr(pm_), ptr(ps_), ptr(pe_), ptr(mm_), ptr(sm_), *shape, *how,
                    ctypes.cast(nl, ctypes.c_void_p), nn, ctypes.cast(ml, ctypes.c_void_p), nm, ptr(loss_), ptr(self.state),
                    query=query, fields=fields)

    def update_spans(self, span, count, gt):
        """Adds B pairs' merged spans ``span (B, k, 2)`` / ``count (B,)`` against ``gt (B, 2)`` (same unit) to the state: samples,
        top-1 IoU and the hits of the meter's n / m (module docstring).  Enqueues on the current stream, returns nothing."""
        from ._lib import SminHipError
        for t in (span, count, gt):
            if not t.is_cuda:
                raise SminHipError("EpochMeter.update_spans runs on a HIP device only (got a CPU tensor); there is no CPU fallback -- the "
                                   "plain-torch restatement is available under the explicit name EpochMeterTorch")
        if span.device != self.state.device:
            raise ValueError(f"EpochMeter on {self.state.device} got tensors on {span.device}")
        B, k = self._spans_check(span, count, gt)
        if B:
            _span_meter_call(span, count, gt, self._n, self._m, self.state)


class EpochMeterTorch(_Meter):
    """``EpochMeter`` as plain torch ops and Python float64 sums on any device (module docstring): built on
    ``compute_ious_torch`` and ``top_moments_torch``; reads the host on every update."""

    @staticmethod
    def _default_device():
        return "cpu"

    def _top1(self, pm, ps, pe, moment_mask, sm):
        """(B,) fp32: sm at each sample's first kept cell, 0 if it keeps none."""
        B, L = pm.shape[0], pm.shape[1]
        smf = sm.detach().float().reshape(B, -1)
        if self.rule == 1:
            from .moments import top_moments_soft_torch, top_moments_torch
            if self._soft is None:
                idx = top_moments_torch(pm, ps, pe, moment_mask, k=1, nms_thresh=self.nms_thresh)["idx"][:, 0]
            else:                                                # the first pick of a soft rule is the best valid cell
                idx = top_moments_soft_torch(pm, ps, pe, moment_mask, k=1, nms_thresh=self.nms_thresh, nms=self.nms, sigma=self.sigma)["idx"][:, 0]
            flat = idx[:, 0] * L + idx[:, 1]
            iou = torch.gather(smf, 1, flat.clamp_min(0).unsqueeze(1)).squeeze(1)
            return torch.where(flat >= 0, iou, torch.zeros_like(iou))
        # the reference's rule as csrc/metrics.hip forms it: ((pm * sqrtf(ps_i)) * sqrtf(pe_j)) * mask over all cells, ties -> lower index
        # (a product, not moments._score_map's selection: a masked NaN stays a NaN)
        score = _mul32(_fused(pm, ps, pe), (byte_mask(moment_mask) != 0).float()).reshape(B, -1)
        cell = torch.arange(L * L, device=score.device).unsqueeze(0)
        best = torch.where(score == score.max(dim=1, keepdim=True).values, cell, torch.full_like(cell, L * L)).min(dim=1).values
        return torch.gather(smf, 1, best.unsqueeze(1)).squeeze(1)

    def update(self, pm, ps, pe, moment_mask, sm, loss=None):
        from .training import compute_ious_torch
        B, L = _check(pm, ps, pe, moment_mask, 1)
        counts = compute_ious_torch(pm.detach(), ps.detach(), pe.detach(), moment_mask, sm, self.n, self.m, nms_thresh=self.nms_thresh,
                                    nms=self.nms, sigma=self.sigma)
        delta = [0.0] * self.state.numel()
        delta[0] = float(B)
        if loss is not None:
            delta[1] = float(loss.detach().float().reshape(1)[0]) * float(B)     # fp32 value, widened: the product is exact in fp64
            delta[2] = float(B)
        s = 0.0
        for v in self._top1(pm, ps, pe, moment_mask, sm).tolist():               # float64 sum over the samples in order
            s += v
        delta[3] = s
        for q, k in enumerate(self.keys):
            delta[4 + q] = float(counts[k])                                       # a sum of 0 / 1 flags: exact in any order
        self.state += torch.tensor(delta, dtype=torch.float64).to(self.state.device)

    def update_spans(self, span, count, gt):
        from .moments import _span_hits_torch, span_ious_torch
        B, k = self._spans_check(span, count, gt)
        ious = span_ious_torch(span, count, gt)
        delta = [0.0] * self.state.numel()
        delta[0] = float(B)
        s = 0.0
        for v in (ious[:, 0].tolist() if B else []):                             # slot 0's IoU (0 when empty), float64 sum in order
            s += v
        delta[3] = s
        if B:
            for q, v in enumerate(_span_hits_torch(ious, count, self._n, self._m).tolist()):
                delta[4 + q] = float(v)
        self.state += torch.tensor(delta, dtype=torch.float64).to(self.state.device)


class _CorpusMeter(_Meter):
    def __init__(self, n=_REF_N, m=_REF_M, device=None):
        self.n, self.m = tuple(n), tuple(m)
        self._n, self._m = _nm_check(self.n, self.m)                         # ValueError: more than 64 n / 16 m, or an n outside 1..64
        self.keys = [f"R@{n_}, IoU={m_}" for n_ in self.n for m_ in self.m] + [f"VR@{n_}" for n_ in self.n]
        self.device = torch.device(self._default_device() if device is None else device)
        self.state = torch.zeros(4 + len(self.keys), dtype=torch.float64, device=self.device)

    def _lists(self, result, gt_video, gt):
        """The checked update: ``video (Q, k)`` int64, ``span (Q, k, 2)`` fp32 -- ``result["times"]`` when present, else the clip edges
        ``(i, j + 1)`` of ``result["idx"]`` --, ``count (Q,)``, ``gt_video (Q,)`` int64 and ``gt (Q, 2)`` fp32."""
        video, count = result["video"], result["count"]
        if video.dim() != 2:
            raise ValueError(f"{type(self).__name__}.update: result['video'] must be (Q, k), got {tuple(video.shape)}")
        Q, k = video.shape
        if not 1 <= k <= MAX_K or k < max(self._n):
            raise ValueError(f"{type(self).__name__}.update: the meter's R@{max(self._n)} needs lists of {max(self._n)}..{MAX_K} entries "
                             f"per query (result has k = {k})")
        if "times" in result:
            span = result["times"].detach().float()
        else:
            span = result["idx"].to(torch.float32)                            # a copy: idx is int64
            span[..., 1] += 1.0
        if tuple(span.shape) != (Q, k, 2) or tuple(count.shape) != (Q,) or tuple(gt_video.shape) != (Q,) or tuple(gt.shape) != (Q, 2):
            raise ValueError(f"{type(self).__name__}.update: times / idx must be (Q, k, 2) = {(Q, k, 2)}, count and gt_video (Q,) and gt "
                             f"(Q, 2); got {tuple(span.shape)}, {tuple(count.shape)}, {tuple(gt_video.shape)}, {tuple(gt.shape)}")
        return video.to(torch.int64), span, count.to(torch.int32), gt_video.to(torch.int64), gt.detach().float(), Q, k


class CorpusMeter(_CorpusMeter):
    """``CorpusMeter(n=(1, 5), m=(0.1, 0.3, 0.5, 0.7), device=...)``: VCMR R@n, IoU=m, VR R@n and the mean top-1 IoU of corpus search,
    in fp64 on the device (module docstring).  ``update(result, gt_video, gt)`` enqueues two kernels on the current stream and returns
    nothing: ``result`` is ``SMIN.search`` / ``merge_search`` / ``SMIN.search_windows`` output (``video``, ``count`` and ``times``, or
    ``idx`` where there are no times) with at least max(n) entries per query, ``gt_video (Q,)`` the
    ground-truth video in ``result["video"]``'s numbering, ``gt (Q, 2)`` the ground-truth moment in the unit of ``result["times"]``
    (seconds) or, without times, in clip edges ``(i, j + 1)``.  HIP tensors only.  ``result()`` reads (keys ``"R@n, IoU=m"``, ``"VR@n"``,
    ``"mIoU"``, ``"num_samples"``), ``reset()`` zeroes, ``state`` is the fp64 device tensor."""

    @staticmethod
    def _default_device():
        return "cuda"

    def update(self, result, gt_video, gt):
        from ._lib import SminHipError, call_ws, ptr, stream
        video, span, count, gt_video, gt, Q, k = self._lists(result, gt_video, gt)
        for t in (video, span, count, gt_video, gt):
            if not t.is_cuda:
                raise SminHipError("CorpusMeter.update runs on a HIP device only (got a CPU tensor); there is no CPU fallback -- the plain-torch "
                                   "restatement is available under the explicit name CorpusMeterTorch")
        if video.device != self.state.device:
            raise ValueError(f"CorpusMeter on {self.state.device} got tensors on {video.device}")
        if Q == 0:
            return
        args = [t.contiguous() for t in (video, span, count, gt_video, gt)]
        nn, nm = len(self._n), len(self._m)
        nl, ml = (ctypes.c_int * nn)(*self._n), (ctypes.c_float * nm)(*self._m)
        with torch.cuda.device(video.device):
            call_ws("smin_corpus_meter_update", (Q, nn, nm), stream(), *[ptr(a) for a in args], Q, k, ctypes.cast(nl, ctypes.c_void_p), nn,
                    ctypes.cast(ml, ctypes.c_void_p), nm, ptr(self.state), query="smin_corpus_meter_ws_bytes", fields="Q, nn, nm")


class CorpusMeterTorch(_CorpusMeter):
    """``CorpusMeter`` as plain torch ops and Python float64 sums on any device: reads the host on every update."""

    @staticmethod
    def _default_device():
        return "cpu"

    def update(self, result, gt_video, gt):
        video, span, count, gt_video, gt, Q, k = self._lists(result, gt_video, gt)
        delta = [0.0] * self.state.numel()
        delta[0] = float(Q)
        if Q:
            valid = _valid_slots(count, k)
            same = (video == gt_video.unsqueeze(1)) & valid
            iou = span_ious_torch(span, count, gt)                            # fp32, each operation rounded once; 0 behind the counts
            iou = torch.where(same, iou, torch.zeros_like(iou))
            s = 0.0
            for v in iou[:, 0].tolist():                                      # float64 sum over the queries in order
                s += v
            delta[3] = s
            thr = torch.tensor(self._m, dtype=torch.float32, device=iou.device)
            hits = [((iou[:, :n_] > thr[c]) & valid[:, :n_]).any(dim=1).sum() for n_ in self._n for c in range(len(self._m))]
            # VR: the distinct videos ranked ahead of the first entry of the ground-truth video
            rank = torch.arange(k, device=video.device)
            first = torch.where(same, rank.unsqueeze(0), torch.full_like(video, k)).min(dim=1).values
            earlier = (video.unsqueeze(2) == video.unsqueeze(1)) & (rank.unsqueeze(0) < rank.unsqueeze(1)).unsqueeze(0)     # [q, r, u]: u < r, same video
            fresh = ~earlier.any(dim=2)
            distinct = (fresh & (rank.unsqueeze(0) < first.unsqueeze(1))).sum(dim=1)
            hits += [((first < k) & (distinct < n_)).sum() for n_ in self._n]
            for q, v in enumerate(torch.stack(hits).tolist()):
                delta[4 + q] = float(v)                                       # sums of 0 / 1 flags: exact in any order
        self.state += torch.tensor(delta, dtype=torch.float64).to(self.state.device)


class VideoRankMeter:
    """``VideoRankMeter(n=(1, 5, 10, 100), device=...)``: video retrieval measured on the video ranking itself --
    VR@n for any positive n, the mean reciprocal rank and the number of queries, as fp64 totals in a device tensor.  ``update(gt_rank)``
    takes ``gt_rank (Q,)`` of ``SMIN.rank_videos`` / ``SMIN.search(video_weight=...)``: the 0-based rank of each query's own video among
    its ranked videos, -1 where it is not among them.  A query counts for VR@n when ``0 <= gt_rank < n`` and adds ``1 / (gt_rank + 1)``
    to the MRR sum (0 for -1).  A few torch ops on the tensor's device per update, no host read; ``result()`` is the one read (keys
    ``"VR@n"``, ``"MRR"``, ``"num_samples"``), ``reset()`` zeroes, ``state`` is ``[queries, sum of reciprocal ranks, hits per n ...]``.
    ``CorpusMeter``'s VR@n, derived from the videos the best moments lie in, stays as it is."""

    def __init__(self, n=(1, 5, 10, 100), device=None):
        self.n = tuple(n)
        if not self.n or any(not isinstance(v, int) or isinstance(v, bool) or v < 1 for v in self.n):
            raise ValueError(f"VideoRankMeter: n must be positive integers (got {n!r})")
        self.keys = [f"VR@{v}" for v in self.n]
        self.device = torch.device("cuda" if device is None else device)
        self.state = torch.zeros(2 + len(self.n), dtype=torch.float64, device=self.device)
        self._n = torch.tensor(self.n, dtype=torch.int64).to(self.device, non_blocking=True)

    def reset(self):
        self.state.zero_()

    def update(self, gt_rank):
        if gt_rank.dim() != 1 or gt_rank.is_floating_point():
            raise ValueError(f"VideoRankMeter.update: gt_rank must be an integer (Q,) tensor, got {tuple(gt_rank.shape)} {gt_rank.dtype}")
        if gt_rank.device != self.state.device:
            raise ValueError(f"VideoRankMeter on {self.state.device} got a tensor on {gt_rank.device}")
        r = gt_rank.to(torch.int64)
        found = r >= 0
        rr = torch.where(found, 1.0 / (r.clamp_min(0) + 1).to(torch.float64), torch.zeros_like(r, dtype=torch.float64))
        hits = (found.unsqueeze(1) & (r.unsqueeze(1) < self._n.unsqueeze(0))).sum(dim=0).to(torch.float64)
        self.state += torch.cat([hits.new_full((1,), float(r.shape[0])), rr.sum().reshape(1), hits])

    def result(self):
        acc = self.state.tolist()                                              # the one host read
        num = acc[0]
        out = {k: (acc[2 + a] / num if num else 0.0) for a, k in enumerate(self.keys)}
        out["MRR"] = acc[1] / num if num else 0.0
        out["num_samples"] = int(num)
        return out


class CutFidelityMeter:
    """``CutFidelityMeter(n=(1, 5, 10), M=(8, 16, 32), device=...)``: what a first-stage cut to M videos loses of a teacher's best n,
    measured without labels.  ``update(teacher_rank, student_rank)`` takes two ``(Q, V)`` integer rank tables --
    ``rank_videos``' ``pair_rank`` over all pairs and ``prefilter_videos``' ``rank``; -1: no candidate -- and for every (n, M) adds
    ``sum_q |{v : 0 <= teacher_rank < n and 0 <= student_rank < M}|`` to one total and ``sum_q min(n, c_q)`` to the other, c_q the
    number of the query's teacher candidates: fp64 totals in a device tensor.  A few torch ops on the tensors' device per update, no
    host read; ``result()`` is the one read (keys ``"keep@n/M"``, the ratio of the totals, 0 when empty, and ``"num_samples"``, the
    queries), ``reset()`` zeroes, ``state`` is ``[queries, kept per (n, M) ..., possible per n ...]``."""

    def __init__(self, n=(1, 5, 10), M=(8, 16, 32), device=None):
        self.n, self.M = tuple(n), tuple(M)
        for name, vals in (("n", self.n), ("M", self.M)):
            if not vals or any(not isinstance(v, int) or isinstance(v, bool) or v < 1 for v in vals):
                raise ValueError(f"CutFidelityMeter: {name} must be positive integers (got {vals!r})")
        self.keys = [f"keep@{a}/{b}" for a in self.n for b in self.M]
        self.device = torch.device("cuda" if device is None else device)
        self.state = torch.zeros(1 + len(self.keys) + len(self.n), dtype=torch.float64, device=self.device)
        self._n = torch.tensor(self.n, dtype=torch.int64).to(self.device, non_blocking=True)
        self._M = torch.tensor(self.M, dtype=torch.int64).to(self.device, non_blocking=True)

    def reset(self):
        self.state.zero_()

    def update(self, teacher_rank, student_rank):
        for name, r in (("teacher_rank", teacher_rank), ("student_rank", student_rank)):
            if r.dim() != 2 or r.is_floating_point() or r.shape != teacher_rank.shape:
                raise ValueError(f"CutFidelityMeter.update: {name} must be an integer (Q, V) tensor, both of one shape; got {tuple(r.shape)} {r.dtype}")
            if r.device != self.state.device:
                raise ValueError(f"CutFidelityMeter on {self.state.device} got a tensor on {r.device}")
        rt, rs = teacher_rank.to(torch.int64).reshape(-1, 1), student_rank.to(torch.int64).reshape(-1, 1)
        best = ((rt >= 0) & (rt < self._n)).to(torch.float64)                      # (Q V, n): among the teacher's best n
        kept = ((rs >= 0) & (rs < self._M)).to(torch.float64)                      # (Q V, M): survives the cut to M
        cands = (teacher_rank >= 0).sum(dim=1, keepdim=True)
        possible = torch.minimum(cands, self._n).sum(dim=0).to(torch.float64)
        self.state += torch.cat([possible.new_full((1,), float(teacher_rank.shape[0])), (best.t() @ kept).reshape(-1), possible])

    def result(self):
        acc = self.state.tolist()                                              # the one host read
        k, nm = len(self.keys), len(self.M)
        out = {key: (acc[1 + a] / acc[1 + k + a // nm] if acc[1 + k + a // nm] else 0.0) for a, key in enumerate(self.keys)}
        out["num_samples"] = int(acc[0])
        return out
