"""Comparisons the tests share: bit views, dict and list comparators, relative errors and spreads."""
import torch

from tests.support.device import vml


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def same_merge(got, want, what=""):
    for key in ("video", "idx", "count"):
        assert torch.equal(got[key].cpu(), want[key]), (what, key)
    assert torch.equal(bits(got["score"]), bits(want["score"])), (what, "score")
    assert got["video"].dtype == torch.int64 and got["idx"].dtype == torch.int64 and got["count"].dtype == torch.int32


def byte_bits(t):
    return t.detach().cpu().contiguous().view(torch.uint8)


def same(got, want, keys, what):
    for key in keys:
        assert got[key].dtype == want[key].dtype and got[key].shape == want[key].shape, (what, key)
        assert torch.equal(byte_bits(got[key]), byte_bits(want[key])), (what, key)


def gate(name, got, want, ref32):
    """e_kernel <= 32 * e_torch32 + 1e-6 with e = max|x - x64| / max|x64|; a quantity that is identically 0 must come out exactly 0"""
    g, w, r = got.detach().cpu().double(), want.detach().cpu().double(), ref32.detach().cpu().double()
    assert g.shape == w.shape and torch.isfinite(g).all(), name
    scale = w.abs().max().item() if w.numel() else 0.0
    if scale == 0.0:
        assert g.abs().max().item() == 0.0 if g.numel() else True, name
        return
    e_k, e_t = (g - w).abs().max().item() / scale, (r - w).abs().max().item() / scale
    print(f"{name}: e_kernel {e_k:.2e}  e_torch32 {e_t:.2e}")
    assert e_k <= 32 * e_t + 1e-6, (name, e_k, e_t)


def _rel(got, ref):
    return (got.double().cpu() - ref).abs().max().item() / max(ref.abs().max().item(), 1e-30)


def _spread(logits, live):
    """Mean over rows (with >= 2 live entries) of the standard deviation of the live logits (None: no such row)."""
    live = live.expand_as(logits)
    cnt = live.sum(-1)
    ok = cnt >= 2
    if not ok.any():
        return None
    x = torch.where(live, logits, 0.0)
    mean = x.sum(-1) / cnt.clamp(min=1)
    var = (torch.where(live, logits - mean.unsqueeze(-1), 0.0) ** 2).sum(-1) / (cnt - 1).clamp(min=1)
    return var.sqrt()[ok].mean().item()


def _assert_spread(logits, live, label, what):
    """The softmaxes must be neither uniform nor saturated, or a dropped or doubled entry would hide."""
    sd = _spread(logits, live)
    assert sd is None or 0.5 <= sd <= 3.0, f"{label}: {what} logit spread {sd:.3f}"


def bits64(t):
    return t.detach().cpu().contiguous().view(torch.int64)


def same_state(opt, ref, table, rtable):
    p = table
    assert torch.equal(p.detach().cpu(), rtable.detach()), "table"
    assert torch.equal(opt.state[p]["exp_avg"].cpu(), ref.state[rtable]["exp_avg"]), "exp_avg"
    assert torch.equal(opt.state[p]["exp_avg_sq"].cpu(), ref.state[rtable]["exp_avg_sq"]), "exp_avg_sq"
    assert torch.equal(opt._state[:3].cpu(), ref._state[:3]), (opt._state, ref._state)


def layout_ok(dev):
    return int(vml()._lib.load_torch().layout_status(dev)[0]) == 0


def float_bits(t):
    t = t.detach().cpu().contiguous()
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def same_tensor(a, b):
    return tuple(a.shape) == tuple(b.shape) and a.dtype == b.dtype and torch.equal(float_bits(a), float_bits(b))
