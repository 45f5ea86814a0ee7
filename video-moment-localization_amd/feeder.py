"""Batch feeder for the data-parallel train step (reference dataset.py:129-187 + main.py:118-133).

The reference builds eleven mask / target tensors per sample on the host (Python loops over CPU tensors), collates them and
ships thirteen tensors per batch to the device with blocking ``.to(device)`` calls.  Here a rank stages only what cannot be
derived -- the sampled clip features, the query word vectors and five scalars per sample (sampled frames, query length, ground
truth start / end, duration) -- in pinned host buffers, copies them on a dedicated HIP stream while the previous step computes,
and one kernel (csrc/labels.hip) writes every mask and target on the device.  Two slots alternate; a slot is refilled only
after the step that consumed it has been queued, which an event orders without host synchronisation.

A loader may instead hand over each video's raw feature rows and the query's token ids (the raw batch form, ``BatchFeeder``
docstring): the clip resampling of dataset.py:40-74 and the word-vector lookup of dataset.py:32-38 then run on the copy stream
as well (csrc/sampling.hip), and the host only packs the ragged rows into a pinned buffer.
"""
import math

import numpy as np
import torch

from . import _lib
from ._host import host_array
from ._lib import call, ptr
from .labels import two_sigma_sq

_BATCH_KEYS = ("video_features", "video_mask", "query_features", "query_mask", "length_mask", "moment_mask",
               "sm", "ym", "ss", "ys", "se", "ye", "ya")


def cell_count(nfeats, T, L):
    """Number of valid cells of the moment masks of samples with ``nfeats`` sampled frames (an int or a sequence), by host arithmetic:
    the sum of ``n_len * (n_len + 1) / 2`` with ``n_len = ceil(nfeats / (T / L))`` (dataset.py:145-147, as csrc/labels.hip forms it).
    It equals ``int(moment_mask.sum())`` of the batch, so a forward can be handed the count (``SMIN.known_cell_count``) and read
    nothing back."""
    total = 0
    for x in np.asarray(nfeats).reshape(-1).tolist():
        n_len = min(max(math.ceil(int(x) / (T / L)), 0), L)
        total += n_len * (n_len + 1) // 2
    return total


class FedBatch(dict):
    """A fed batch: the dict of the thirteen device tensors main.py's loop reads, plus ``cell_count``, the number of valid cells of
    its ``moment_mask`` computed on the host (``cell_count`` above)."""
    cell_count = None


def _annotation_times(times):
    """A batch's ``times`` as a CPU tensor for staging: float64 where the loader still has the annotation's doubles (a float64 array
    or tensor, or Python floats), so that build_targets_hip forms the Gaussians' denominator from them; float32 otherwise."""
    t = times.detach().cpu() if isinstance(times, torch.Tensor) else torch.from_numpy(np.asarray(times))
    return t if t.dtype == torch.float64 else t.float()


def build_targets_hip(times, duration, nfeats, qlen, T, L, Nq, stream=None):
    """All masks and targets of a batch in one launch (device tensors in, dict of device tensors out; dtypes and shapes as
    main.py reads them: video_mask / query_mask uint8 (B, T, 1) / (B, Nq, 1), length_mask / moment_mask / y* bool)."""
    if not times.is_cuda:
        raise _lib.SminHipError("build_targets_hip runs on a HIP device only (got a CPU tensor); there is no CPU fallback")
    dev, B = times.device, times.shape[0]
    u8 = lambda *s: torch.empty(s, dtype=torch.uint8, device=dev)
    f32 = lambda *s: torch.empty(s, dtype=torch.float32, device=dev)
    out = dict(video_mask=u8(B, T, 1), query_mask=u8(B, Nq, 1) if qlen is not None else None, length_mask=u8(B, L), moment_mask=u8(B, L, L),
               sm=f32(B, L, L), ym=u8(B, L, L), ss=f32(B, L), ys=u8(B, L), se=f32(B, L), ye=u8(B, L), ya=u8(B, L))
    # annotation times that still carry their double precision: 2 sigma^2 in double, rounded once (dataset.py:116-119 does the same
    # arithmetic in Python floats); fp32 times: the kernel forms it in double from what it is given
    den = two_sigma_sq(times).contiguous() if times.dtype == torch.float64 else None
    times, duration = times.float().contiguous(), duration.float().contiguous()
    nfeats = nfeats.to(torch.int32).contiguous()
    qlen32 = qlen.to(torch.int32).contiguous() if qlen is not None else None
    with torch.cuda.device(dev):
        s = _lib.stream() if stream is None else stream
        call("smin_build_targets", s, ptr(times), ptr(duration), ptr(nfeats), ptr(qlen32), B, T, L, Nq, ptr(out["video_mask"]), ptr(out["query_mask"]),
             ptr(out["length_mask"]), ptr(out["moment_mask"]), ptr(out["sm"]), ptr(out["ym"]), ptr(out["ss"]), ptr(out["ys"]), ptr(out["se"]),
             ptr(out["ye"]), ptr(out["ya"]), ptr(den))
    for k in ("length_mask", "moment_mask", "ym", "ys", "ye", "ya"):
        out[k] = out[k].view(torch.bool)                      # same bytes; the reference's tensors are BoolTensors
    if qlen is None:
        del out["query_mask"]
    return out


def build_masks_hip(nfeats, T, L):
    """The masks of build_targets_hip alone (smin_build_targets with no targets): nfeats (B,) device int -> dict video_mask uint8
    (B, T, 1), length_mask bool (B, L), moment_mask bool (B, L, L).  No annotation is needed; no host read."""
    if not nfeats.is_cuda:
        raise _lib.SminHipError("build_masks_hip runs on a HIP device only (got a CPU tensor); there is no CPU fallback")
    dev, B = nfeats.device, nfeats.shape[0]
    out = dict(video_mask=torch.empty((B, T, 1), dtype=torch.uint8, device=dev), length_mask=torch.empty((B, L), dtype=torch.uint8, device=dev),
               moment_mask=torch.empty((B, L, L), dtype=torch.uint8, device=dev))
    nf = nfeats.to(torch.int32).contiguous()
    with torch.cuda.device(dev):
        call("smin_build_targets", _lib.stream(), None, None, ptr(nf), None, B, T, L, 1, ptr(out["video_mask"]), None, ptr(out["length_mask"]),
             ptr(out["moment_mask"]), *([None] * 8))
    out["length_mask"], out["moment_mask"] = out["length_mask"].view(torch.bool), out["moment_mask"].view(torch.bool)
    return out


def _raw_parts(hb):
    """A raw batch's ``raw_features`` as ``(parts, lengths (B,) int64)``: the list's arrays, or the one packed array with its
    ``raw_lengths`` checked against its rows (ValueError)."""
    raw = hb["raw_features"]
    if isinstance(raw, (list, tuple)):
        parts = [r if isinstance(r, torch.Tensor) else np.asarray(r) for r in raw]
        return parts, np.array([p.shape[0] for p in parts], dtype=np.int64)
    parts = [raw if isinstance(raw, torch.Tensor) else np.asarray(raw)]
    if "raw_lengths" not in hb:
        raise ValueError("a packed raw_features array needs raw_lengths (B,)")
    lengths = np.asarray(hb["raw_lengths"], dtype=np.int64).reshape(-1)
    if (lengths < 0).any() or int(lengths.sum()) != parts[0].shape[0]:
        raise ValueError(f"raw_lengths must be >= 0 and sum to the {parts[0].shape[0]} rows of raw_features")
    return parts, lengths


class BatchFeeder:
    """Double-buffered host -> device feeder.  ``feed(sample_batches)`` takes an iterable of host batches
    ``dict(video_features (B,T,Din) float32, query_features (B,Nq,300) float32, nfeats (B,), qlen (B,), times (B,2), duration (B,))``
    (numpy arrays or CPU tensors) and yields device batches with the thirteen entries main.py's loop reads, one batch ahead of
    the consumer.  ``times`` given as float64 (a float64 array or tensor, or Python floats -- what a loader has) stay float64 up to
    ``build_targets_hip``, which forms the Gaussians' denominator from them in double as dataset.py:116-119 does; this holds for the
    raw and the window form as well.  fp32 ``times`` are taken as they are.  Each yielded batch is a ``FedBatch``: its int attribute ``cell_count`` is the number of valid cells of its
    ``moment_mask``, from the host's ``nfeats`` (raw form: ``min(raw length, T)``) -- nothing is read back for it.

    Raw batch form (chosen by its keys): ``dict(raw_features, tokens (B,Nq) int, times (B,2), duration (B,), spos (B,) optional)``
    with ``raw_features`` a list of B arrays ``(n_b, Din)`` or one packed ``(sum n_b, Din)`` array plus ``raw_lengths (B,)``.  The
    device resamples the rows to T clips (``pool``: "pick", the reference's rule, with start offsets ``spos``, default 0; or "mean",
    sampling.py) and looks the ids up in ``embedding`` (a device ``(V, E)`` table, required for this form) with ``pad_id``
    (default ``V - 1``); nfeats and qlen come from those kernels' outputs and query_mask is ``tokens < pad_id`` (dataset.py:173).
    Token ids and ``spos`` are validated on the host (ValueError).  The yielded batch has the same thirteen entries.

    Window form (a raw batch that also carries ``win_start (B,)`` and ``win_len (B,)``, e.g. from ``sampling.draw_windows``):
    ``raw_features`` holds whole videos as above, ``times`` / ``duration`` the annotations in seconds; only rows
    ``win_start[b] .. win_start[b] + win_len[b]`` of each video are packed into the pinned buffer, and the batch is then exactly the
    raw form of those rows with ``sampling.window_annotations``' ``(times_w, duration_w)``: ``spos`` is validated against
    ``win_len``, ``cell_count`` comes from ``min(win_len, T)``.  A window outside its video raises ValueError before staging."""

    def __init__(self, T, L, Nq, device, depth=3, embedding=None, pad_id=None, pool="pick"):
        from .sampling import MODES
        self.T, self.L, self.Nq, self.device = T, L, Nq, torch.device(device)
        if self.device.type != "cuda":
            raise _lib.SminHipError("BatchFeeder feeds a HIP device; there is no CPU path")
        if pool not in MODES:
            raise ValueError(f"pool must be one of {sorted(MODES)} (got {pool!r})")
        if embedding is not None and not (embedding.is_cuda and embedding.dim() == 2):
            raise _lib.SminHipError("BatchFeeder(embedding=...) takes a (V, E) table on the HIP device")
        self.embedding = None if embedding is None else embedding.detach().float().contiguous()
        self.pad_id = None if embedding is None else (embedding.shape[0] - 1 if pad_id is None else int(pad_id))
        self.pool = pool
        self.copy_stream = torch.cuda.Stream(self.device)
        self.slots = [dict(host={}, ready=torch.cuda.Event(), consumed=None) for _ in range(depth)]

    def _pinned(self, slot, key, src):
        if src.is_pinned():                                                  # a loader with pin_memory=True: no staging copy
            return src
        buf = slot["host"].get(key)
        if buf is None or buf.shape != src.shape or buf.dtype != src.dtype:
            buf = slot["host"][key] = torch.empty(src.shape, dtype=src.dtype, pin_memory=True)
        buf.copy_(src)
        return buf

    def _stage(self, slot, hb):
        """Host side of one batch: into the slot's pinned buffers, then H2D + target construction on the copy stream."""
        if "batch" in slot:
            slot["ready"].synchronize()                                      # the slot's previous H2D copies have left its pinned buffers
        if "raw_features" in hb:
            return self._stage_raw(slot, hb)
        t = {k: torch.as_tensor(v) for k, v in hb.items()}
        t["times"] = _annotation_times(hb["times"])                          # float64 annotations stay float64 up to build_targets_hip
        host = {k: self._pinned(slot, k, t[k] if k == "times" else t[k].float() if k in ("video_features", "query_features", "duration") else t[k].to(torch.int32))
                for k in ("video_features", "query_features", "nfeats", "qlen", "times", "duration")}
        with torch.cuda.device(self.device), torch.cuda.stream(self.copy_stream):
            if slot["consumed"] is not None:
                self.copy_stream.wait_event(slot["consumed"])              # the step that read this slot's tensors is queued before we overwrite
            d = {k: v.to(self.device, non_blocking=True) for k, v in host.items()}
            B = d["video_features"].shape[0]
            # (rows past a sample's sampled frames / words arrive as zeros, as the reference's loader makes them: dataset.py:72-73, 172)
            tg = build_targets_hip(d["times"], d["duration"], d["nfeats"], d["qlen"], self.T, self.L, self.Nq)
            batch = dict(video_features=d["video_features"], query_features=d["query_features"], **tg)
            slot["ready"].record(self.copy_stream)
        slot["batch"] = FedBatch((k, batch[k]) for k in _BATCH_KEYS)
        slot["batch"].cell_count = cell_count(t["nfeats"].numpy(), self.T, self.L)
        return B

    def _stage_raw(self, slot, hb):
        """Raw batch form: pack the ragged rows into the slot's pinned buffer (grown on demand, then reused), stage offsets, ids,
        start offsets and annotations, and enqueue H2D + resampling + lookup + targets on the copy stream.  No host read."""
        from .sampling import embed_tokens, sample_clips, _check_spos
        if self.embedding is None:
            raise ValueError("a raw batch (tokens) needs BatchFeeder(embedding=<(V, E) device table>)")
        if "win_start" in hb:
            hb = self._cut_windows(hb)
        parts, lengths = _raw_parts(hb)
        B = lengths.shape[0]
        Din = parts[0].shape[1] if parts and parts[0].ndim == 2 else -1
        if B < 1 or Din < 4 or Din % 4 or any(p.ndim != 2 or p.shape[1] != Din for p in parts):
            raise ValueError("raw_features must be (n_b, Din) arrays with one Din, Din % 4 == 0, and at least one sample")
        tok = host_array(hb["tokens"], None, None)
        V = self.embedding.shape[0]
        if tok.dtype.kind not in "iu" or tok.shape != (B, self.Nq):
            raise ValueError(f"tokens must be an integer array of shape (B, Nq) = {(B, self.Nq)} (got {tok.dtype}, {tok.shape})")
        if tok.size and (int(tok.min()) < 0 or int(tok.max()) >= V):
            raise ValueError(f"token ids must lie in [0, {V}) (the embedding table's rows)")
        spos = hb.get("spos")
        spos = None if spos is None else _check_spos(spos, lengths, self.T, self.pool)
        if self.pool == "mean":
            spos = None                                                      # validated to be all 0
        N = int(lengths.sum())
        p0 = parts[0]
        if len(parts) == 1 and isinstance(p0, torch.Tensor) and p0.dtype == torch.float32 and p0.is_contiguous() and p0.is_pinned():
            packed = p0                                                      # a loader's pinned packed rows: no staging copy
        else:
            buf = slot["host"].get("raw")
            if buf is None or buf.numel() < N * Din:                         # grows on demand, then is reused
                buf = slot["host"]["raw"] = torch.empty(max(N * Din, 4), dtype=torch.float32, pin_memory=True)
            packed = buf[:N * Din].view(N, Din)
            # one plain memcpy per video through numpy: a single core and no GIL, where a torch copy_ of this size would start
            # the intra-op thread pool and take cores from the thread that launches the step
            dst = packed.numpy()
            o = 0
            for p in parts:
                np.copyto(dst[o:o + p.shape[0]], p.detach().cpu().numpy() if isinstance(p, torch.Tensor) else p, casting="same_kind")
                o += p.shape[0]
        small = dict(offsets=torch.from_numpy(np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)), tokens=torch.from_numpy(tok.astype(np.int32)),
                     times=_annotation_times(hb["times"]), duration=torch.as_tensor(hb["duration"]).float())
        if spos is not None:
            small["spos"] = torch.from_numpy(spos)
        host = {k: self._pinned(slot, "raw_" + k, v) for k, v in small.items()}
        with torch.cuda.device(self.device), torch.cuda.stream(self.copy_stream):
            if slot["consumed"] is not None:
                self.copy_stream.wait_event(slot["consumed"])
            d = {k: v.to(self.device, non_blocking=True) for k, v in host.items()}
            raw_d = packed.to(self.device, non_blocking=True)
            vf, nfeats = sample_clips(raw_d, d["offsets"], self.T, spos=d.get("spos"), mode=self.pool)
            qf, qm, qlen = embed_tokens(d["tokens"], self.embedding, self.pad_id)
            tg = build_targets_hip(d["times"], d["duration"], nfeats, None, self.T, self.L, self.Nq)
            batch = dict(video_features=vf, query_features=qf, query_mask=qm.view(B, self.Nq, 1), **tg)
            slot["ready"].record(self.copy_stream)
        slot["batch"] = FedBatch((k, batch[k]) for k in _BATCH_KEYS)
        slot["batch"].cell_count = cell_count(np.minimum(lengths, self.T), self.T, self.L)
        return B

    def _cut_windows(self, hb):
        """Window form -> the raw batch of the windows' rows: views of rows win_start .. win_start + win_len of each video (nothing is
        copied here; the raw path packs them) and the annotations in window time."""
        from .sampling import window_annotations
        parts, n = _raw_parts(hb)
        if isinstance(hb["raw_features"], (list, tuple)):
            videos = parts
        else:
            o = np.concatenate([[0], np.cumsum(n)])
            videos = [parts[0][o[b]:o[b + 1]] for b in range(n.shape[0])]
        ws, wl = host_array(hb["win_start"]), host_array(hb["win_len"])
        if ws.shape != n.shape or wl.shape != n.shape:
            raise ValueError(f"win_start and win_len must be (B,) = {n.shape} (got {ws.shape}, {wl.shape})")
        bad = np.nonzero((ws < 0) | (wl < 0) | (ws + wl > n))[0]
        if bad.size:
            b = int(bad[0])
            raise ValueError(f"window {b} (rows {int(ws[b])} .. {int(ws[b] + wl[b])}) lies outside its video of {int(n[b])} rows")
        times_w, duration_w = window_annotations(hb["times"], hb["duration"], n, ws, wl, self.T)
        out = dict(raw_features=[v[int(s):int(s + w)] for v, s, w in zip(videos, ws, wl)], tokens=hb["tokens"], times=times_w, duration=duration_w)
        if hb.get("spos") is not None:
            out["spos"] = hb["spos"]
        return out

    def feed(self, host_batches):
        """Generator of device batches.  A worker thread does the host side of every batch (pinned staging copy, enqueueing the
        H2D copies and the target kernel on the copy stream) up to ``depth`` batches ahead; the consumer's thread only makes its
        stream wait for the slot's event, so no step waits for a host memcpy."""
        import queue
        import threading
        free, ready = queue.Queue(), queue.Queue()
        for slot in self.slots:
            free.put(slot)
        stop = threading.Event()

        def worker():
            try:
                for hb in host_batches:
                    slot = free.get()
                    if stop.is_set():
                        return
                    self._stage(slot, hb)
                    ready.put(slot)
                ready.put(None)
            except BaseException as e:                                       # surfaces in the consumer
                ready.put(e)

        th = threading.Thread(target=worker, name="smin-batch-feeder", daemon=True)
        th.start()
        try:
            while True:
                slot = ready.get()
                if slot is None:
                    return
                if isinstance(slot, BaseException):
                    raise slot
                cur = torch.cuda.current_stream(self.device)
                cur.wait_event(slot["ready"])                                # device-side wait only
                for v in slot["batch"].values():
                    v.record_stream(cur)
                yield slot["batch"]
                slot["consumed"] = torch.cuda.Event()
                slot["consumed"].record(torch.cuda.current_stream(self.device))
                free.put(slot)
        finally:
            stop.set()
            free.put(self.slots[0])                                          # unblock a worker waiting for a slot
