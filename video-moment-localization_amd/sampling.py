"""Clip resampling of raw per-video features and word-vector lookup of token ids, on the device (csrc/sampling.hip).

The reference does both per sample on the host, in ``AbstractDataset.__getitem__``: ``get_fixed_length_features``
(dataset.py:40-74) picks ``min(n, T)`` of a video's ``n`` raw feature rows at a stride of ``n / T`` and zero-pads the rest, and
``get_query_features`` (dataset.py:32-38) turns token ids into GloVe vectors.  Here a loader hands over the raw rows and the ids.

Pick (``mode="pick"``, the reference), for a video of ``n`` rows and a start offset ``spos``, all in double:

* ``stride = 1.0`` if ``n <= T`` else ``n / T``; ``delta = (spos + stride) - spos`` (numpy ``arange``'s fill step);
* row ``t < min(n, T)`` is raw row ``rint(spos + t * delta)`` (round half to even, as ``np.round``); later rows are zero;
* ``spos`` is 0 in the eval split; the train split draws it from ``[0, int(r + 1))`` with ``r = stride - 0.5``, minus 1 when ``r``
  is integral (dataset.py:45-49).  ``draw_offsets`` draws from that range; the kernel clamps a value outside it.

Mean (``mode="mean"``, the 2D-TAN alternative the reference's comment at dataset.py:68-70 names; ``spos`` must be 0): for
``n <= T`` the same as pick; for ``n > T`` row ``t`` is the mean of raw rows ``[a_t, a_{t+1})`` with ``a_t = rint(t * n / T)`` in
double and ``a_T = n``, summed in fp32 in ascending row order and divided once in fp32 by the row count.

``sample_clips`` / ``embed_tokens`` are the product entry points (HIP tensors only, no host read, capturable in a graph);
``sample_clips_torch`` / ``clip_indices`` are the plain numpy / torch restatement the tests compare against -- nothing routes to
them silently.

With ``differentiable=True`` and grad mode on, a ``raw`` / ``table`` that requires grad receives its gradient through an autograd
node backed by deterministic HIP backward kernels (``smin_sample_clips_bwd`` / ``smin_embed_tokens_bwd``: fixed summation order, no
atomics); ``nfeats``, ``query_mask`` and ``qlen`` are never differentiable.  By default both functions detach their inputs.

``embed_tokens(..., differentiable=True, sparse_grad=True)`` leaves the table's gradient as its distinct rows instead (a
``RowSparseGrad`` on ``table.row_grad``, from ``smin_embed_tokens_bwd_rows``: no ``(V, E)`` tensor is formed), for
``optim.RowSparseAdam`` to consume.  ``merge_row_grads`` merges several such gradients of one table into one
(``smin_row_lists_merge``: data-parallel ranks through ``distributed.exchange_row_grad``, micro-batches through
``embed_tokens(..., accumulate=True)``); ``merge_row_grads_torch`` restates it."""
from torch.autograd import Function
import numpy as np
import torch

from ._host import host_array

MODES = {"pick": 0, "mean": 1}


def spos_high(n, T):
    """Exclusive upper end of the train split's start offset for videos of ``n`` rows: ``int(r + 1)`` with ``r = stride - 0.5``,
    minus 1 when integral (dataset.py:45-49; ``np.random.randint(0, r + 1)`` draws from ``[0, int(r + 1))``).  1 when n <= T."""
    n, T = np.asarray(n, dtype=np.int64), np.asarray(T, dtype=np.int64)
    stride = np.where(n <= T, 1.0, n / T.astype(np.float64))
    r = stride - 0.5
    r = np.where(r == np.floor(r), r - 1.0, r)
    return (r + 1.0).astype(np.int64)


def draw_offsets(n, T, rng):
    """Train-split start offsets for videos of ``n`` rows (array-like), drawn uniformly from ``[0, spos_high(n, T))`` with a
    ``numpy.random.Generator`` (the reference's distribution; drawn on the host so a run is reproducible from its seed)."""
    return rng.integers(0, spos_high(n, T)).astype(np.int32)


def clip_indices(n, T, spos=0):
    """The raw row indices the pick rule takes for a video of ``n`` rows (length ``min(n, T)``), from the definition above."""
    n, spos = int(n), int(spos)
    stride = 1.0 if n <= T else n / float(T)
    s = float(spos)
    delta = (s + stride) - s
    idx = np.rint(s + np.arange(min(n, T), dtype=np.float64) * delta).astype(np.int64)
    return np.clip(idx, 0, max(n - 1, 0))


def mean_windows(n, T):
    """Mean mode's window starts ``a_t`` (T + 1 entries, ``a_T = n``) for a video of ``n > T`` rows."""
    a = np.rint(np.arange(T + 1, dtype=np.float64) * float(n) / float(T)).astype(np.int64)
    a[T] = n
    return a


def _check_spos(spos, lengths, T, mode):
    """Host-side validation of start offsets against the reference's range (ValueError)."""
    s = host_array(spos)
    if s.shape[0] != lengths.shape[0]:
        raise ValueError(f"spos has {s.shape[0]} entries for {lengths.shape[0]} samples")
    if mode == "mean" and s.any():
        raise ValueError("mode='mean' takes no start offset (spos must be 0)")
    hi = spos_high(lengths, T)
    bad = np.nonzero((s < 0) | (s >= hi))[0]
    if bad.size:
        b = int(bad[0])
        raise ValueError(f"spos[{b}] = {int(s[b])} is outside [0, {int(hi[b])}) for a video of {int(lengths[b])} rows at T = {T} "
                         "(dataset.py:45-49)")
    return s.astype(np.int32)


def _pack(raw, offsets_or_lengths):
    """-> (raw (N, Din) tensor, host lengths (B,) or None, device offsets (B+1,) int64 or None)."""
    if isinstance(raw, (list, tuple)):
        if offsets_or_lengths is not None:
            raise ValueError("a list of per-video tensors carries its own lengths (offsets_or_lengths must be None)")
        lengths = np.array([int(r.shape[0]) for r in raw], dtype=np.int64)
        if len(raw) == 0:
            return None, lengths, None
        return torch.cat([r.reshape(-1, r.shape[-1]) for r in raw], 0), lengths, None
    if isinstance(offsets_or_lengths, torch.Tensor) and offsets_or_lengths.is_cuda:
        return raw, None, offsets_or_lengths
    return raw, host_array(offsets_or_lengths), None


class _SampleClipsFn(Function):
    """sample_clips' resampling as an autograd node: raw (rows, Din) -> video_features (B, T, Din); backward smin_sample_clips_bwd."""

    @staticmethod
    def forward(ctx, raw, offsets, sp, B, T, mode):
        from ._lib import call, ptr, stream
        Din = raw.shape[1]
        out = torch.empty((B, T, Din), dtype=torch.float32, device=raw.device)
        nfeats = torch.empty((B,), dtype=torch.int32, device=raw.device)
        call("smin_sample_clips", stream(), ptr(raw), ptr(offsets), ptr(sp), B, T, Din, mode, ptr(out), ptr(nfeats))
        ctx.mark_non_differentiable(nfeats)
        ctx.save_for_backward(offsets, sp)
        ctx.dims = (B, T, Din, mode, raw.shape[0])
        return out, nfeats

    @staticmethod
    def backward(ctx, dout, _dnfeats):
        from ._lib import call, ptr, stream
        offsets, sp = ctx.saved_tensors
        B, T, Din, mode, rows = ctx.dims
        dout = dout.float().contiguous()
        if dout.data_ptr() % 16:
            dout = dout.clone()
        draw = torch.empty((rows, Din), dtype=torch.float32, device=dout.device)
        call("smin_sample_clips_bwd", stream(), ptr(dout), ptr(offsets), ptr(sp), B, T, Din, mode, rows, ptr(draw))
        return draw, None, None, None, None, None


def sample_clips(raw, offsets_or_lengths, T, spos=None, mode="pick", differentiable=False):
    """Resample a batch of ragged raw feature sequences to ``(B, T, Din)`` on the device (module docstring).

    ``raw``: one packed HIP tensor ``(sum n_b, Din)`` with ``offsets_or_lengths`` either host lengths ``(B,)`` (list, numpy or CPU
    tensor: validated here) or device offsets ``(B + 1,)`` int64 (nothing is read back: graph-capturable; they must be non-decreasing
    and within ``raw``, which is not checked); or a list of ``B`` HIP tensors ``(n_b, Din)`` with ``offsets_or_lengths=None``.
    ``spos``: ``None`` (all 0, the eval split), host values (validated against the reference's range: ValueError) or a device int
    tensor ``(B,)``.  Returns ``(video_features (B, T, Din) float32, nfeats (B,) int32)`` with ``nfeats = min(n_b, T)``.
    ``differentiable=True``: when ``raw`` (or a tensor of the list) requires grad under grad mode, ``video_features`` carries an
    autograd node whose backward gives each raw row the sum of the output rows' gradients that read it (ascending ``t``; mean mode:
    its window's gradient over the window's row count); rows never sampled get 0.  Default: ``raw`` is detached."""
    from ._lib import SminHipError, call, ptr, stream
    if mode not in MODES:
        raise ValueError(f"mode must be one of {sorted(MODES)} (got {mode!r})")
    raw, lengths, offsets = _pack(raw, offsets_or_lengths)
    if raw is None:
        raise ValueError("sample_clips needs at least one video (or a packed tensor with B = 0 lengths)")
    if not raw.is_cuda:
        raise SminHipError("sample_clips runs on a HIP device only (got a CPU tensor); there is no CPU fallback -- "
                           "the plain restatement is available under the explicit name sample_clips_torch")
    if raw.dim() != 2 or raw.shape[1] % 4 != 0 or raw.shape[1] < 4:
        raise ValueError(f"raw must be (rows, Din) with Din % 4 == 0 (got {tuple(raw.shape)})")
    dev, Din, T = raw.device, raw.shape[1], int(T)
    if T < 1:
        raise ValueError(f"T must be >= 1 (got {T})")
    grad = differentiable and raw.requires_grad and torch.is_grad_enabled()
    raw = (raw if grad else raw.detach()).float().contiguous()
    if raw.data_ptr() % 16:
        raw = raw.clone()
    if lengths is not None:
        if (lengths < 0).any() or int(lengths.sum()) != raw.shape[0]:
            raise ValueError(f"lengths must be >= 0 and sum to raw's {raw.shape[0]} rows (got {lengths.sum()})")
        offsets = torch.from_numpy(np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)).to(dev, non_blocking=False)
        B = int(lengths.shape[0])
    else:
        if offsets.dtype != torch.int64 or offsets.dim() != 1 or offsets.shape[0] < 1:
            raise ValueError("device offsets must be a 1-D int64 tensor of B + 1 entries")
        B = offsets.shape[0] - 1
    sp = None
    if spos is not None:
        if isinstance(spos, torch.Tensor) and spos.is_cuda:
            if mode != "pick":
                raise ValueError("mode='mean' takes no start offset (spos must be None)")
            sp = spos.to(torch.int32).contiguous()
        elif lengths is not None:
            s = _check_spos(spos, lengths, T, mode)
            sp = torch.from_numpy(s).to(dev) if mode == "pick" else None
        else:
            raise ValueError("host spos needs host lengths to be checked against (pass lengths, or spos as a device tensor)")
    if grad:
        if B > 65535:
            raise ValueError(f"sample_clips: at most 65535 videos per call (got {B})")
        with torch.cuda.device(dev):
            return _SampleClipsFn.apply(raw, offsets.contiguous(), sp, B, T, MODES[mode])
    out = torch.empty((B, T, Din), dtype=torch.float32, device=dev)
    nfeats = torch.empty((B,), dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        call("smin_sample_clips", stream(), ptr(raw), ptr(offsets.contiguous()), ptr(sp), B, T, Din, MODES[mode], ptr(out), ptr(nfeats))
    return out, nfeats


def sample_clips_torch(raw, offsets_or_lengths, T, spos=None, mode="pick"):
    """``sample_clips`` as plain numpy on the host (same result, bit for bit): the restatement the device is checked against.
    Takes the same argument forms (host lengths or offsets; CPU or device tensors, copied to the host); returns CPU tensors."""
    if mode not in MODES:
        raise ValueError(f"mode must be one of {sorted(MODES)} (got {mode!r})")
    if isinstance(raw, (list, tuple)):
        rows = [np.asarray(r.detach().cpu() if isinstance(r, torch.Tensor) else r, dtype=np.float32).reshape(-1, r.shape[-1]) for r in raw]
        lengths = np.array([r.shape[0] for r in rows], dtype=np.int64)
        Din = rows[0].shape[1] if rows else 0
        packed = np.concatenate(rows, 0) if rows else np.zeros((0, Din), np.float32)
    else:
        packed = np.asarray(raw.detach().cpu() if isinstance(raw, torch.Tensor) else raw, dtype=np.float32)
        lengths = host_array(offsets_or_lengths)
        if isinstance(offsets_or_lengths, torch.Tensor) and offsets_or_lengths.is_cuda:
            lengths = np.diff(lengths)                                        # device offsets -> lengths
        Din = packed.shape[1]
    B = lengths.shape[0]
    s = np.zeros(B, np.int64) if spos is None else _check_spos(spos, lengths, T, mode)
    offs = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    out = np.zeros((B, T, Din), np.float32)
    for b in range(B):
        n, x = int(lengths[b]), packed[offs[b]:offs[b + 1]]
        if mode == "pick" or n <= T:
            idx = clip_indices(n, T, s[b])
            out[b, :idx.shape[0]] = x[idx]
        else:
            a = mean_windows(n, T)
            cnt = a[1:] - a[:-1]
            acc = x[a[:-1]].copy()
            for q in range(1, int(cnt.max())):                               # fp32 sum in ascending row order
                m = cnt > q
                acc[m] += x[a[:-1][m] + q]
            out[b] = acc / cnt.astype(np.float32)[:, None]
    return torch.from_numpy(out), torch.from_numpy(np.minimum(lengths, T).astype(np.int32))


class _EmbedTokensFn(Function):
    """embed_tokens' lookup as an autograd node: table (V, E) -> query_features (B, Nq, E); backward smin_embed_tokens_bwd."""

    @staticmethod
    def forward(ctx, tok, table, pad_id):
        from ._lib import call, ptr, stream
        (B, Nq), (V, E) = tok.shape, table.shape
        qf = torch.empty((B, Nq, E), dtype=torch.float32, device=tok.device)
        qm = torch.empty((B, Nq), dtype=torch.uint8, device=tok.device)
        ql = torch.empty((B,), dtype=torch.int32, device=tok.device)
        call("smin_embed_tokens", stream(), ptr(tok), ptr(table), B, Nq, V, E, pad_id, ptr(qf), ptr(qm), ptr(ql))
        ctx.mark_non_differentiable(qm, ql)
        ctx.save_for_backward(tok)
        ctx.V = V
        return qf, qm, ql

    @staticmethod
    def backward(ctx, dqf, _dqm, _dql):
        from ._lib import call, load, ptr, stream, workspace
        (tok,) = ctx.saved_tensors
        B, Nq = tok.shape
        E = dqf.shape[2]
        dqf = dqf.float().contiguous()
        if dqf.data_ptr() % 16:
            dqf = dqf.clone()
        dtable = torch.empty((ctx.V, E), dtype=torch.float32, device=dqf.device)
        ws = workspace(load().smin_embed_tokens_bwd_workspace_bytes(B, Nq), dqf.device)
        call("smin_embed_tokens_bwd", stream(), ptr(tok), ptr(dqf), B, Nq, ctx.V, E, ptr(dtable), ptr(ws), ws.numel())
        return None, dtable, None


class RowSparseGrad:
    """The gradient of a ``(V, E)`` table as the rows a batch touched, all on the device (``smin_embed_tokens_bwd_rows``):

    ``ids (n,) int32``: slots ``s < count`` hold the distinct ids in ``[0, V)``, strictly ascending; later slots hold -1.
    ``rows (n, E) float32``: ``rows[s]`` = row ``ids[s]`` of the dense gradient, bit for bit; rows of later slots are unspecified.
    ``count (1,) int32``; ``sq_norm (1,) float64`` = the sum of squares of the ``count`` rows (a fixed summation order).
    ``n = B * Nq`` of the batch (the sum of its inputs' ``n`` for a merged gradient); ``shape = (V, E)``.  ``pending`` (host side) is set
    by the backward or merge that made it and cleared by ``clear()``, which the optimizer's ``step()`` / ``zero_grad()`` call: a backward
    into a table whose gradient is still pending is refused unless ``embed_tokens`` was called with ``accumulate=True``, which merges
    the two (``merge_row_grads``)."""

    def __init__(self, ids, rows, count, sq_norm, shape):
        self.ids, self.rows, self.count, self.sq_norm, self.shape = ids, rows, count, sq_norm, tuple(shape)
        self.pending = True

    def clear(self):
        self.pending = False

    def to_dense(self):
        """The ``(V, E)`` gradient, formed on the device without a host read: slots with id -1 are ignored."""
        V, E = self.shape
        idx = self.ids.to(torch.int64)
        used = (idx >= 0) & (idx < V)
        # the rows of unused slots were never written: they are replaced by zeros and added to row 0, which adding zero leaves as it is;
        # every other row receives exactly one listed row, so the sum is that row whatever the order of the additions
        rows = torch.where(used.unsqueeze(1), self.rows, torch.zeros_like(self.rows))
        dense = torch.zeros((V, E), dtype=self.rows.dtype, device=self.rows.device)
        return dense.index_add_(0, torch.where(used, idx, torch.zeros_like(idx)), rows)

    def to_sparse_coo(self):
        """A coalesced ``torch.sparse_coo_tensor`` of shape ``(V, E)`` (reads ``count``: one host read)."""
        c = int(self.count.item())
        return torch.sparse_coo_tensor(self.ids[:c].to(torch.int64).unsqueeze(0), self.rows[:c], self.shape, is_coalesced=True)


MERGE_MAX_LISTS = 16                 # row lists per merge_row_grads call
MERGE_MAX_SLOTS = 65536              # the sum of their capacities (and the longest list RowSparseAdam.step() takes)


def _merge_args(grads, who):
    """-> (list of RowSparseGrad, (V, E), device, N = the sum of the capacities), or ValueError"""
    grads = list(grads)
    if not 1 <= len(grads) <= MERGE_MAX_LISTS:
        raise ValueError(f"{who}: 1 to {MERGE_MAX_LISTS} row gradients per call (got {len(grads)})")
    shape, dev = tuple(grads[0].shape), grads[0].rows.device
    for g in grads:
        if tuple(g.shape) != shape or g.rows.device != dev or g.ids.device != dev or g.count.device != dev:
            raise ValueError(f"{who}: every row gradient must be of the same (V, E) table on one device (got {tuple(g.shape)} on "
                             f"{g.rows.device} beside {shape} on {dev})")
        if g.ids.dim() != 1 or g.rows.shape != (g.ids.shape[0], shape[1]) or g.count.numel() != 1:
            raise ValueError(f"{who}: ids (n,), rows (n, E) and count (1,) expected (got {tuple(g.ids.shape)}, {tuple(g.rows.shape)}, "
                             f"{tuple(g.count.shape)})")
    N = sum(int(g.ids.shape[0]) for g in grads)
    if N > MERGE_MAX_SLOTS:
        raise ValueError(f"{who}: the capacities add up to {N} slots, at most {MERGE_MAX_SLOTS} per call")
    return grads, shape, dev, N


def merge_row_grads(grads, scale=None):
    """Merge 1 to 16 ``RowSparseGrad`` of the same ``(V, E)`` table on one HIP device into one, on the device and without a host read
    (``smin_row_lists_merge``, csrc/row_sparse.hip).  The result has capacity ``N`` = the sum of the inputs'
    capacities (at most 65536): ``ids[:count]`` is the strictly ascending union of the listed ids, ``ids[count:]`` is -1; ``rows[s]`` is
    ``((rows_a + rows_b) + ...)`` over the inputs that list ``ids[s]``, in the order of ``grads``, every fp32 addition rounded on its own,
    then -- when ``scale`` is given: a float, or one fp64 value on the device -- multiplied by the scale cast once to fp32; ``sq_norm``
    is the fp64 sum of squares of the result's rows in the order of ``smin_embed_tokens_bwd_rows``, so one gradient merged alone comes
    back bit for bit.  The same bits every run.  Returns a pending ``RowSparseGrad``; the inputs are left as they are.
    ValueError: mismatched ``(V, E)`` or devices, more than 16 gradients, more than 65536 slots; SminHipError: CPU tensors."""
    import ctypes
    from ._lib import SminHipError, call, load, ptr, stream, workspace
    grads, (V, E), dev, N = _merge_args(grads, "merge_row_grads")
    if dev.type != "cuda":
        raise SminHipError("merge_row_grads runs on a HIP device only (got CPU tensors); there is no CPU fallback -- the plain restatement "
                           "is available under the explicit name merge_row_grads_torch")
    for g in grads:
        if (g.ids.dtype != torch.int32 or g.count.dtype != torch.int32 or g.rows.dtype != torch.float32
                or not (g.ids.is_contiguous() and g.rows.is_contiguous()) or g.rows.data_ptr() % 16):
            raise ValueError("merge_row_grads: ids and count must be int32, rows fp32, contiguous and 16-byte aligned")
    if scale is not None:
        if not isinstance(scale, torch.Tensor):
            scale = torch.full((1,), float(scale), dtype=torch.float64).to(dev, non_blocking=True)
        if scale.dtype != torch.float64 or scale.numel() != 1 or scale.device != dev:
            raise ValueError("merge_row_grads: scale must be one fp64 value on the gradients' device (or a float)")
        scale = scale.detach().contiguous()
    R = len(grads)
    ids = torch.empty((N,), dtype=torch.int32, device=dev)
    rows = torch.empty((N, E), dtype=torch.float32, device=dev)
    count = torch.empty((1,), dtype=torch.int32, device=dev)
    sq_norm = torch.empty((1,), dtype=torch.float64, device=dev)
    pointers = lambda ts: (ctypes.c_void_p * R)(*[t.data_ptr() if t.numel() else None for t in ts])
    caps = (ctypes.c_int * R)(*[int(g.ids.shape[0]) for g in grads])
    with torch.cuda.device(dev):
        ws = workspace(load().smin_row_lists_merge_workspace_bytes(R, N), dev)
        call("smin_row_lists_merge", stream(), pointers([g.ids for g in grads]), pointers([g.rows for g in grads]),
             pointers([g.count for g in grads]), caps, R, V, E, ptr(scale), ptr(ids), ptr(rows), ptr(count), ptr(sq_norm), ptr(ws), ws.numel())
    return RowSparseGrad(ids, rows, count, sq_norm, (V, E))


def merge_row_grads_torch(grads, scale=None):
    """``merge_row_grads`` as plain torch ops on any device (the restatement; reads the counts on the host): the same order of
    additions, one fp32 operation at a time, the same -1 tail; rows of slots ``>= count`` are zero; ``sq_norm`` is the fp64 sum of
    squares of ``rows[:count]`` (``torch.sum``: the kernel's value to a few ulps, not to the bit).  Nothing routes to it."""
    grads, (V, E), dev, N = _merge_args(grads, "merge_row_grads_torch")
    lists = []
    for g in grads:
        c = min(max(int(g.count.reshape(-1)[0]), 0), int(g.ids.shape[0]))
        lists.append((g.ids[:c].to(torch.int64), g.rows[:c].to(torch.float32)))
    union = torch.unique(torch.cat([i for i, _ in lists]))           # sorted
    K = int(union.numel())
    acc = torch.zeros((K, E), dtype=torch.float32, device=dev)
    have = torch.zeros((K,), dtype=torch.bool, device=dev)
    for i, r in lists:                                                # a list's ids are distinct: every slot receives one row per list at most
        slot = torch.searchsorted(union, i)
        acc[slot] = torch.where(have[slot].unsqueeze(1), acc[slot] + r, r)
        have[slot] = True
    if scale is not None:
        c = scale.detach().reshape(-1)[0].to(torch.float64) if isinstance(scale, torch.Tensor) else torch.tensor(float(scale), dtype=torch.float64)
        acc = acc * c.to(device=dev, dtype=torch.float32)             # cast once to fp32, one rounding per element
    ids = torch.full((N,), -1, dtype=torch.int32, device=dev)
    ids[:K] = union.to(torch.int32)
    rows = torch.zeros((N, E), dtype=torch.float32, device=dev)
    rows[:K] = acc
    count = torch.tensor([K], dtype=torch.int32, device=dev)
    sq_norm = (acc.double() * acc.double()).sum().reshape(1)
    return RowSparseGrad(ids, rows, count, sq_norm, (V, E))


class _EmbedTokensRowsFn(Function):
    """embed_tokens' lookup with a row-sparse backward: smin_embed_tokens_bwd_rows deposits a RowSparseGrad on ``holder[0].row_grad`` (the
    caller's table); the node itself returns no gradient, so ``table.grad`` stays None."""

    @staticmethod
    def forward(ctx, tok, table, pad_id, holder, accumulate):
        out = _EmbedTokensFn.forward(ctx, tok, table, pad_id)
        ctx.E, ctx.holder, ctx.accumulate = table.shape[1], holder, accumulate
        return out

    @staticmethod
    def backward(ctx, dqf, _dqm, _dql):
        from ._lib import call, load, ptr, stream, workspace
        (tok,) = ctx.saved_tensors
        table = ctx.holder[0]
        old = getattr(table, "row_grad", None)
        old = old if old is not None and old.pending else None
        if old is not None and not ctx.accumulate:
            raise RuntimeError("embed_tokens(sparse_grad=True): the table's row_grad of an earlier backward is still pending; consume it "
                               "with RowSparseAdam.step(), drop it with zero_grad() / table.row_grad.clear(), or pass accumulate=True to "
                               "add this backward's rows to it")
        B, Nq = tok.shape
        n, E, dev = B * Nq, ctx.E, dqf.device
        dqf = dqf.float().contiguous()
        if dqf.data_ptr() % 16:
            dqf = dqf.clone()
        ids = torch.empty((n,), dtype=torch.int32, device=dev)
        rows = torch.empty((n, E), dtype=torch.float32, device=dev)
        count = torch.empty((1,), dtype=torch.int32, device=dev)
        sq_norm = torch.empty((1,), dtype=torch.float64, device=dev)
        ws = workspace(load().smin_embed_tokens_bwd_rows_workspace_bytes(B, Nq), dev)
        call("smin_embed_tokens_bwd_rows", stream(), ptr(tok), ptr(dqf), B, Nq, ctx.V, E, ptr(ids), ptr(rows), ptr(count), ptr(sq_norm),
             ptr(ws), ws.numel())
        new = RowSparseGrad(ids, rows, count, sq_norm, (ctx.V, E))
        table.row_grad = new if old is None else merge_row_grads([old, new])   # old + new, as the dense path's table.grad += new
        return None, None, None, None, None


EMBED_BWD_MAX = 4096                 # B * Nq of one differentiable embed_tokens call (the backward sorts the positions in one workgroup)


def embed_tokens(tokens, table, pad_id=None, differentiable=False, sparse_grad=False, accumulate=False):
    """Query word vectors from token ids on the device (dataset.py:32-38, 173).  ``tokens`` (B, Nq) integer HIP tensor, ``table``
    (V, E) float32 HIP tensor (E % 4 == 0), ``pad_id`` default ``V - 1`` (the reference's ``<pad>``, appended last).

    Returns ``(query_features (B, Nq, E) float32 = table[tokens], query_mask (B, Nq) uint8 = tokens < pad_id, qlen (B,) int32 = sum
    of the mask)``.  An id outside ``[0, V)`` gives a zero row and mask 0; it is never read.
    ``differentiable=True``: when ``table`` requires grad under grad mode, ``query_features`` carries an autograd node whose backward
    forms the dense ``table.grad`` (as ``nn.Embedding(sparse=False)``): row ``v`` = the sum of the gradient rows at the positions
    holding ``v``, in ascending ``(b, w)`` order, other rows 0; ``B * Nq <= 4096``.  Default: ``table`` is detached.
    ``sparse_grad=True`` (needs ``differentiable=True``: ValueError otherwise; ``table`` fp32, contiguous, 16-byte aligned): the same
    forward, but the backward deposits the gradient's distinct rows as a ``RowSparseGrad`` on ``table.row_grad`` -- the same sums, bit
    for bit, with no ``(V, E)`` tensor -- and ``table.grad`` stays None.  A second backward while that gradient is pending raises
    RuntimeError (``RowSparseAdam.step()`` / ``zero_grad()`` or ``table.row_grad.clear()`` release it), unless
    ``accumulate=True`` (needs ``sparse_grad=True``: ValueError otherwise): the backward then replaces a pending ``row_grad`` by
    ``merge_row_grads([pending, new])``, whose ``to_dense()`` is what the dense path's ``table.grad += ...`` gives, bit for bit; the
    capacities add up, at most 65536 slots in all."""
    from ._lib import SminHipError, call, ptr, stream
    if sparse_grad and not differentiable:
        raise ValueError("embed_tokens: sparse_grad=True needs differentiable=True")
    if accumulate and not sparse_grad:
        raise ValueError("embed_tokens: accumulate=True needs sparse_grad=True (the dense path accumulates into table.grad by itself)")
    if not (tokens.is_cuda and table.is_cuda):
        raise SminHipError("embed_tokens runs on a HIP device only (got a CPU tensor); there is no CPU fallback")
    if tokens.dim() != 2 or table.dim() != 2 or table.shape[1] % 4 != 0 or table.shape[1] < 4 or tokens.shape[1] < 1:
        raise ValueError(f"tokens must be (B, Nq >= 1) and table (V, E) with E % 4 == 0 (got {tuple(tokens.shape)}, {tuple(table.shape)})")
    (B, Nq), (V, E) = tokens.shape, table.shape
    pad_id = V - 1 if pad_id is None else int(pad_id)
    tok = tokens.to(torch.int32).contiguous()
    grad = differentiable and table.requires_grad and torch.is_grad_enabled()
    if sparse_grad and (table.dtype != torch.float32 or not table.is_contiguous() or table.data_ptr() % 16):
        raise ValueError(f"embed_tokens(sparse_grad=True): the table must be fp32, contiguous and 16-byte aligned, since its rows are updated "
                         f"in place (got {table.dtype}, contiguous = {table.is_contiguous()})")
    tab = (table if grad else table.detach()).float().contiguous()
    if tab.data_ptr() % 16:
        tab = tab.clone()
    dev = tokens.device
    if grad:
        if B * Nq > EMBED_BWD_MAX:
            raise ValueError(f"embed_tokens(differentiable=True): B * Nq = {B * Nq} positions, at most {EMBED_BWD_MAX} per call")
        if sparse_grad:
            with torch.cuda.device(dev):
                return _EmbedTokensRowsFn.apply(tok, tab, pad_id, [table], bool(accumulate))
        with torch.cuda.device(dev):
            return _EmbedTokensFn.apply(tok, tab, pad_id)
    qf = torch.empty((B, Nq, E), dtype=torch.float32, device=dev)
    qm = torch.empty((B, Nq), dtype=torch.uint8, device=dev)
    ql = torch.empty((B,), dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        call("smin_embed_tokens", stream(), ptr(tok), ptr(tab), B, Nq, V, E, pad_id, ptr(qf), ptr(qm), ptr(ql))
    return qf, qm, ql


def embed_tokens_torch(tokens, table, pad_id=None):
    """``embed_tokens`` as plain torch on any device (the restatement)."""
    V = table.shape[0]
    pad_id = V - 1 if pad_id is None else int(pad_id)
    t = tokens.to(torch.int64)
    ok = (t >= 0) & (t < V)
    qf = table.float()[t.clamp(0, V - 1)]
    qf = torch.where(ok.unsqueeze(-1), qf, torch.zeros_like(qf))
    qm = (ok & (t < pad_id)).to(torch.uint8)
    return qf, qm, qm.sum(1, dtype=torch.int32)


# ---------------------------------------------------------------- overlapping windows of long videos (SMIN.localize_windows)
MAX_ROWS = 1 << 24                   # rows per video: a window start is then exact in fp32 (the merge's spans, moments.py)


def window_plan(lengths, window, stride):
    """Overlapping windows over V videos of ``lengths`` raw rows (host sequence or CPU tensor), pure host arithmetic.

    A video of ``n`` rows gets no window for ``n == 0``; one window ``(start 0, len n)`` for ``n <= window``; otherwise windows of
    ``len = window`` at starts ``0, stride, 2 * stride, ...`` while ``start + window <= n``, plus one at ``n - window`` when the last of
    those ends before ``n``.  Windows are ordered by video, then by start.  Returns CPU tensors ``(starts (W,) int64`` relative to the
    video, ``lens (W,) int32, ptr (V + 1,) int64)``: video ``v`` owns windows ``ptr[v] .. ptr[v + 1]``.  Needs ``window >= 1``,
    ``stride >= 1`` and ``0 <= n < 2**24``."""
    n = host_array(lengths)
    window, stride = int(window), int(stride)
    if window < 1:
        raise ValueError(f"window_plan: window must be >= 1 (got {window})")
    if stride < 1:
        raise ValueError(f"window_plan: stride must be >= 1 (got {stride})")
    if n.size and (n.min() < 0 or n.max() >= MAX_ROWS):
        raise ValueError(f"window_plan: every length must be in [0, 2**24) so that a start is exact in fp32 (got {n.min()} .. {n.max()})")
    starts, lens, ptr = [], [], [0]
    for v in n.tolist():
        if v == 0:
            pass
        elif v <= window:
            starts.append(np.zeros(1, np.int64))
            lens.append(np.full(1, v, np.int32))
        else:
            s = np.arange(0, v - window + 1, stride, dtype=np.int64)
            if s[-1] + window < v:
                s = np.append(s, v - window)
            starts.append(s)
            lens.append(np.full(s.shape[0], window, np.int32))
        ptr.append(ptr[-1] + (starts[-1].shape[0] if v else 0))
    cat = lambda xs, dt: np.concatenate(xs).astype(dt) if xs else np.zeros(0, dt)
    return (torch.from_numpy(cat(starts, np.int64)), torch.from_numpy(cat(lens, np.int32)),
            torch.from_numpy(np.asarray(ptr, dtype=np.int64)))


def window_annotations(times, duration, lengths, win_start, win_len, T):
    """Annotations of B samples re-expressed in the time of one window each, for training on windows (host, float64; unit: raw rows).

    ``times (B, 2)`` / ``duration (B,)`` in seconds, ``lengths (B,)`` the videos' row counts, ``win_start`` / ``win_len (B,)`` the
    chosen window of each.  With ``g = times / duration * n`` (the ground truth in rows): ``times_w = g - win_start`` and
    ``duration_w = max(win_len, T)``.  This is the geometry of the merge (``moments.window_spans``): a cell of the window spans
    ``max(len, T) / L`` rows, which is what the target kernel forms from ``duration_w``.  The ground truth is not clipped to the
    window: a window holding part of a long moment gets IoUs below 1, one that misses it ``sm = 0`` everywhere, and sigma comes
    from the whole moment.  The targets are then those of dataset.py:95-126 for ``(times_w, duration_w, nfeats = min(win_len, T))``.
    Returns ``(times_w (B, 2), duration_w (B,))`` float64 numpy arrays."""
    t = host_array(times, np.float64, (-1, 2))
    d = host_array(duration, np.float64)
    n, s, w = host_array(lengths), host_array(win_start), host_array(win_len)
    B = t.shape[0]
    if not (d.shape[0] == n.shape[0] == s.shape[0] == w.shape[0] == B):
        raise ValueError(f"window_annotations: times (B, 2) with duration, lengths, win_start, win_len (B,) (got B = {B} and "
                         f"{d.shape[0]}, {n.shape[0]}, {s.shape[0]}, {w.shape[0]})")
    g = t / d[:, None] * n.astype(np.float64)[:, None]
    return g - s.astype(np.float64)[:, None], np.maximum(w, int(T)).astype(np.float64)


def draw_windows(lengths, gt_rows, window, stride, rng, p_overlap):
    """One training window per sample, drawn on the host from a ``numpy.random.Generator`` (reproducible from its seed).

    The candidates of sample b are ``window_plan([n_b], window, stride)``: the grid ``SMIN.localize_windows`` scores.  Per sample, in
    order: ``u = rng.random()``; the overlapping candidates are those with ``min(s + len, ge) - max(s, gs) > 0`` for the ground
    truth ``gt_rows[b] = (gs, ge)`` in rows; if ``u < p_overlap`` and there is one, the choice is among them, else among all
    candidates; one ``rng.integers(0, len(set))`` picks it.  ``p_overlap`` is the training policy (1: always a window that sees the
    moment where one exists; 0: uniform over the grid).  Returns ``(win_start (B,) int64, win_len (B,) int32)``; a video of 0 rows
    raises ValueError."""
    n = host_array(lengths)
    gt = host_array(gt_rows, np.float64, (-1, 2))
    if gt.shape[0] != n.shape[0]:
        raise ValueError(f"draw_windows: gt_rows must be (B, 2) for B = {n.shape[0]} videos (got {gt.shape})")
    win_start, win_len = np.zeros(n.shape[0], np.int64), np.zeros(n.shape[0], np.int32)
    for b, v in enumerate(n.tolist()):
        if v == 0:
            raise ValueError(f"draw_windows: video {b} has no rows")
        starts, lens, _ = (x.numpy() for x in window_plan([v], window, stride))
        u = rng.random()
        over = np.flatnonzero(np.minimum(starts + lens, gt[b, 1]) - np.maximum(starts, gt[b, 0]) > 0)
        cand = over if (u < p_overlap and over.size) else np.arange(starts.shape[0])
        c = cand[int(rng.integers(0, cand.shape[0]))]
        win_start[b], win_len[b] = starts[c], lens[c]
    return win_start, win_len


def sample_windows(raw, row_begin, lens, T, mode="pick"):
    """Resample W row ranges of ``raw`` to ``(W, T, Din)`` on the device: sample ``w`` is exactly ``sample_clips`` of a video made
    of rows ``row_begin[w] .. row_begin[w] + lens[w]`` (eval split, ``spos = 0``), in either mode; ranges may overlap and repeat,
    and no row is copied to form them (csrc/sampling.hip, smin_sample_windows).  ``raw``: HIP tensor ``(R, Din)``, Din % 4 == 0.
    ``row_begin`` / ``lens``: host sequences (checked to lie within ``raw``: ValueError) or device int tensors ``(W,)`` (not
    checked, nothing read back).  Returns ``(video_features (W, T, Din) float32, nfeats (W,) int32 = min(lens, T))``."""
    from ._lib import SminHipError, call, ptr, stream
    if mode not in MODES:
        raise ValueError(f"mode must be one of {sorted(MODES)} (got {mode!r})")
    if not (isinstance(raw, torch.Tensor) and raw.is_cuda):
        raise SminHipError("sample_windows runs on a HIP device only (got a CPU tensor); there is no CPU fallback -- "
                           "the plain restatement is available under the explicit name sample_windows_torch")
    if raw.dim() != 2 or raw.shape[1] % 4 != 0 or raw.shape[1] < 4:
        raise ValueError(f"raw must be (rows, Din) with Din % 4 == 0 (got {tuple(raw.shape)})")
    T, dev, Din = int(T), raw.device, raw.shape[1]
    if T < 1:
        raise ValueError(f"T must be >= 1 (got {T})")
    on_dev = [isinstance(x, torch.Tensor) and x.is_cuda for x in (row_begin, lens)]
    if all(on_dev):
        rb, ln = row_begin.to(torch.int64).contiguous(), lens.to(torch.int32).contiguous()
    elif any(on_dev):
        raise ValueError("row_begin and lens must both be device tensors or both host values")
    else:
        b, n = host_array(row_begin), host_array(lens)
        if b.shape != n.shape:
            raise ValueError(f"row_begin has {b.shape[0]} entries, lens {n.shape[0]}")
        if b.size and (b.min() < 0 or n.min() < 0 or n.max() >= 2 ** 31 or (b + n).max() > raw.shape[0]):
            raise ValueError(f"sample_windows: every range must lie within raw's {raw.shape[0]} rows")
        rb, ln = torch.from_numpy(b).to(dev), torch.from_numpy(n.astype(np.int32)).to(dev)
    W = rb.shape[0]
    if ln.shape[0] != W or W > 65535:
        raise ValueError(f"sample_windows: row_begin and lens must have the same length, at most 65535 (got {W}, {ln.shape[0]})")
    raw = raw.detach().float().contiguous()
    if raw.data_ptr() % 16:
        raw = raw.clone()
    out = torch.empty((W, T, Din), dtype=torch.float32, device=dev)
    nfeats = torch.empty((W,), dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        call("smin_sample_windows", stream(), ptr(raw), ptr(rb), ptr(ln), W, T, Din, MODES[mode], ptr(out), ptr(nfeats))
    return out, nfeats


def sample_windows_torch(raw, row_begin, lens, T, mode="pick"):
    """``sample_windows`` restated: ``sample_clips_torch`` of each row range on its own (CPU tensors out)."""
    packed = raw.detach().cpu() if isinstance(raw, torch.Tensor) else torch.as_tensor(np.asarray(raw, np.float32))
    b, n = host_array(row_begin), host_array(lens)
    Din = packed.shape[1]
    if b.shape[0] == 0:
        return torch.zeros((0, T, Din), dtype=torch.float32), torch.zeros((0,), dtype=torch.int32)
    parts = [sample_clips_torch(packed[s:s + m], [m], T, mode=mode) for s, m in zip(b.tolist(), n.tolist())]
    return torch.cat([p[0] for p in parts]), torch.cat([p[1] for p in parts])
