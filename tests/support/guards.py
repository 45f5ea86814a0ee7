"""Guarded buffers: sentinel bands around kernel outputs (fp32 bands of -12345.5, 32 words wide; words of 0x5A5A5A5A), NaN-filled
workspaces and the ctypes pointer and array helpers of the C ABI tests."""
import ctypes

import numpy as np
import torch

from tests.helpers import cdiv

WORD_SENTINEL = 0x5A5A5A5A
SENTINEL = -12345.5
BAND = 32


def banded(shape, dev, fill=float("nan")):
    """a contiguous fp32 tensor of ``shape`` pre-filled with ``fill`` between two bands of SENTINEL: ``(the whole buffer, the view)``"""
    n = int(np.prod(shape))
    buf = torch.full((n + 2 * BAND,), SENTINEL, dtype=torch.float32, device=dev)
    buf[BAND:BAND + n] = fill
    return buf, buf[BAND:BAND + n].view(*shape)


def bands_intact(buf):
    return bool(buf[:BAND].eq(SENTINEL).all()) and bool(buf[-BAND:].eq(SENTINEL).all())


def untouched(outs, bufs):
    return all(bands_intact(b) for b in bufs.values()) and all(bool(torch.isnan(o).all()) for o in outs.values())


def _vp(t):
    return None if t is None or t.numel() == 0 else ctypes.c_void_p(t.data_ptr())


def _nan(shape, dev, dtype=torch.float32):
    return torch.full(tuple(shape), float("nan"), dtype=dtype, device=dev)


def _ws_nan(nbytes, dev):
    """A NaN-filled workspace of at least nbytes (whole floats) and the byte count to declare: exactly nbytes."""
    return _nan((max(1, cdiv(int(nbytes), 4)),), dev), int(nbytes)
