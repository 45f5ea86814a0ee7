"""Host-side helpers that the module surface (modules.py), retrieval (retrieval.py), the loops (training.py), the feeder and the
samplers share, one copy each.  None of them launches anything or reads the device, except ``host_array`` of a device tensor."""
import contextlib

import numpy as np
import torch

from ._lib import SminHipError


class _AttnMaps(list):
    """Per-layer (content map, boundary map) pairs a forward fills; mode "dense": content maps (B, L, L, C, Nq), "packed": rows
    [N*C, Nq] of the cell list, whose cellmap (B, L, L) is kept beside them."""

    def __init__(self, mode):
        super().__init__()
        self.mode, self.cellmap = mode, None


def host_array(x, dtype=np.int64, shape=(-1,)):
    """A host sequence, numpy array or tensor (copied to the host) as a numpy array of ``dtype`` (None: as it comes), reshaped to
    ``shape`` (None: as it comes)."""
    a = np.asarray(x.cpu() if isinstance(x, torch.Tensor) else x, dtype=dtype)
    return a if shape is None else a.reshape(shape)


def byte_mask(mask):
    """A mask as one byte per element (bool / uint8 as they are), contiguous: what the banks keep and the kernels gather."""
    return (mask if mask.dtype in (torch.bool, torch.uint8) else mask != 0).contiguous()


@contextlib.contextmanager
def known_cells(model, count):
    """For the ``with`` body: a host-computed valid-cell count (feeder.cell_count, FedBatch.cell_count, VideoBank.cell_counts) as
    ``model.known_cell_count``, so the forward sizes its per-cell tensors without asking the device; the previous value is restored
    on exit, exceptions included.  ``count`` None: the attribute is left alone.  A count that does not match the mask sets the
    device's layout_status word, which EpochMeter.result() reads."""
    if count is None:
        yield
        return
    known = model.known_cell_count
    model.known_cell_count = int(count)
    try:
        yield
    finally:
        model.known_cell_count = known


def _require_hip(t, what):
    if not t.is_cuda:
        raise SminHipError(f"{what} runs on a HIP device only (got a CPU tensor); there is no CPU fallback -- "
                           f"the plain-torch restatement is available under the explicit name {what}_torch")


def require_hip_tensors(what, tensors, must="be a HIP tensor"):
    """SminHipError, in ``what``'s name, for the first of the named ``tensors`` (a dict) that is not a tensor on a HIP device."""
    for name, t in tensors.items():
        if not (isinstance(t, torch.Tensor) and t.is_cuda):
            raise SminHipError(f"{what}: {name} must {must} (there is no CPU fallback)")


def require_ints(what, *ranges):
    """ValueError, in ``what``'s name, for the first (name, value, lo, hi) whose value is not an integer in [lo, hi]."""
    for name, v, lo, hi in ranges:
        if not (isinstance(v, (int, np.integer)) and lo <= v <= hi):
            raise ValueError(f"{what}: {name} must be an integer in [{lo}, {hi}] (got {v!r})")


def query_mask_rows(query_features, query_mask, max_query_length):
    """``query_mask`` as (B, words): ValueError unless it has a column per word of ``query_features``, at most max_query_length."""
    query_mask = query_mask.reshape(query_features.shape[0], -1)
    if query_mask.shape[1] != query_features.shape[1] or query_mask.shape[1] > max_query_length:
        raise ValueError(f"query_mask has {query_mask.shape[1]} columns for {query_features.shape[1]} words (max_query_length {max_query_length})")
    return query_mask
