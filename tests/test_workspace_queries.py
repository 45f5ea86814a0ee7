"""Every entry point that takes a workspace and had no size query of its own now has one (include/smin_hip.h: smin_<entry>_ws_bytes),
read from the layout the entry point carves.  For each of the eight, through the C ABI:

  1. the query's size is enough, and nothing is written past it: a call on exactly `need` bytes gives bit for bit what a call on a
     roomy buffer gives, and 4096 guard bytes behind the `need` bytes (inside the allocation) keep their pattern;
  2. one byte less is refused before any launch (a code below -1000, pattern-filled outputs untouched) -- or, where the header says
     the workspace is neither read nor checked, the call does what it does with a full workspace;
  3. the query returns 0 exactly for the shape arguments the entry point's own checks name, and more than 0 at each limit.

Three cell lists reach every branch of the layouts: "small" (one split of every TN reduction, one sample ragged), "split" (680 cells:
tn_splits gives 3 and more, chunking_fine(16) 8 chunks) and "empty" (N = 0: the layouts' `N > 0 ? .. : 1` arms)."""
import ctypes

import pytest
import torch

from tests.support.device import dev  # noqa: F401  (the module's device fixture)
from tests.support.guards import _vp, _ws_nan

GUARD = 4096
FILL = 7.0                                     # what the refusal runs pre-fill the outputs with

# name: (B, T, L, C, D, dl, Nq)
LISTS = {"small": (2, 16, 8, 3, 64, 16, 5), "split": (5, 32, 16, 2, 64, 16, 5), "empty": (2, 16, 8, 3, 64, 16, 5)}


def _mask(name):
    B, _, L = LISTS[name][:3]
    mm = torch.triu(torch.ones(L, L, dtype=torch.bool)).unsqueeze(0).repeat(B, 1, 1)
    if name == "small":
        mm[1, :, L - 2:] = False               # ragged: one sample's last rows cut
    if name == "empty":
        mm[:] = False
    return mm


def test_lists_are_what_the_layouts_branch_on():
    assert int(_mask("small").sum()) < 256 and int(_mask("split").sum()) == 680 and int(_mask("empty").sum()) == 0


_SETUPS = {}


def _setup(dev, name):
    """The list's layout on the device and a generator for its inputs, built once per list."""
    if name not in _SETUPS:
        import models
        _SETUPS[name] = models.vml_amd.CellLayout.from_mask(_mask(name).to(dev))
    return _SETUPS[name], torch.Generator().manual_seed(sorted(LISTS).index(name) + 11)


def _arr(ts):
    return (ctypes.c_void_p * len(ts))(*[t.data_ptr() for t in ts])


class Case:
    """One call of one entry point: need (its query's answer), outs(fill) -> fresh output tensors, launch(outs, ws pointer, ws_bytes)
    -> the entry point's return code, checked (False where the header says the workspace is neither read nor checked)."""
    def __init__(self, need, outs, launch, checked=True):
        self.need, self.outs, self.launch, self.checked = need, outs, launch, checked


def _pm_fwd(dev, name, variant):
    import models
    from vml_amd._lib import stream
    lib = models.vml_amd._lib.load()
    B, T, L, C, D = LISTS[name][:5]
    lay, g = _setup(dev, name)
    N = lay.N
    f = torch.randn(B, T, D, generator=g).to(dev)
    outs = lambda fill: [torch.full(s, fill, device=dev) for s in ((N, C, D), (N, D), (B, L, D))]
    launch = lambda o, wp, wn: lib.smin_proposal_map_fwd(stream(), _vp(f), _vp(lay.cells), N, B, T, L, C, D, _vp(o[0]), _vp(o[1]), _vp(o[2]), wp, wn)
    return Case(lib.smin_proposal_map_fwd_ws_bytes(B, T, D), outs, launch)


def _pm_bwd(dev, name, variant):
    import models
    from vml_amd._lib import stream
    from vml_amd.functional import clip_event_table
    lib = models.vml_amd._lib.load()
    B, T, L, C, D = LISTS[name][:5]
    lay, g = _setup(dev, name)
    N = lay.N
    dfc, dfm, dfb = (torch.randn(*s, generator=g).to(dev) for s in ((N, C, D), (N, D), (B, L, D)))
    eo, et = clip_event_table(dev, T, L, C)
    outs = lambda fill: [torch.full((B, T, D), fill, device=dev)]
    launch = lambda o, wp, wn: lib.smin_proposal_map_bwd(stream(), _vp(dfc), _vp(dfm), _vp(dfb), _vp(lay.cells), _vp(lay.row_ptr), _vp(lay.cellmap),
                                                         N, B, T, L, C, D, _vp(o[0]), wp, wn, _vp(eo), _vp(et))
    return Case(lib.smin_proposal_map_bwd_ws_bytes(B, T, D), outs, launch, checked=N > 0)        # N == 0: no workspace (header)


def _cwm(dev, name, variant):
    import models
    from vml_amd._lib import stream
    from vml_amd.functional import clip_event_table
    lib = models.vml_amd._lib.load()
    B, T, L, C = LISTS[name][:4]
    W, nseg = 16, 3
    lay, g = _setup(dev, name)
    N = lay.N
    need = getattr(lib, f"smin_clip_window_means_{variant}_ws_bytes")(B, T, W, nseg)
    if variant == "fwd":
        gf, bias = torch.randn(B, T, W * nseg, generator=g).to(dev), torch.randn(W, generator=g).to(dev)
        outs = lambda fill: [torch.full((nseg, N * C, W), fill, device=dev)]
        launch = lambda o, wp, wn: lib.smin_clip_window_means_fwd(stream(), _vp(gf), _vp(bias), W, _vp(lay.cells), N, B, T, L, C, W, nseg, _vp(o[0]), wp, wn)
        return Case(need, outs, launch)
    douts = [torch.randn(max(N * C, 1), W, generator=g).to(dev) for _ in range(nseg)]
    arr = _arr(douts)
    eo, et = clip_event_table(dev, T, L, C)
    outs = lambda fill: [torch.full((B, T, W * nseg), fill, device=dev)]
    launch = lambda o, wp, wn: lib.smin_clip_window_means_bwd(stream(), arr, _vp(lay.cells), _vp(lay.row_ptr), _vp(lay.cellmap), N, B, T, L, C, W, nseg,
                                                              _vp(o[0]), wp, wn, _vp(eo), _vp(et))
    case = Case(need, outs, launch, checked=N > 0)                                                   # N == 0: no workspace (header)
    case.keep = douts
    return case


def _gate_bwd(dev, name, variant):
    import models
    from vml_amd._lib import stream
    lib = models.vml_amd._lib.load()
    B, _, L, _, D = LISTS[name][:5]
    lay, g = _setup(dev, name)
    N = lay.N
    r = lambda *s: torch.randn(*s, generator=g).to(dev)
    fm, fs, dh, dres, A, dout = r(N, D), r(B, D), [r(N, D), r(N, D)], [r(N, D)], r(B, L, L), r(B, L, D)
    dh_arr, dres_arr = _arr(dh), _arr(dres)
    outs = lambda fill: [torch.full((N, D), fill, device=dev), torch.full((B, D), fill, device=dev)]
    launch = lambda o, wp, wn: lib.smin_gate_bwd(stream(), dh_arr, 2, dres_arr, 1, _vp(fm), _vp(fs), _vp(lay.row_ptr), N, B, L, D, _vp(o[0]), _vp(o[1]),
                                                 wp, wn, _vp(lay.cells), _vp(A), _vp(dout))
    case = Case(lib.smin_gate_bwd_ws_bytes(B, L, D), outs, launch)
    case.keep = (dh, dres)
    return case


def _mu_bwd(dev, name, variant):
    """variant: whole | inputs | weights (the halves) | x1h (smin_moment_unit_bwd_x1h, whole)"""
    import models
    from vml_amd._lib import stream
    lib = models.vml_amd._lib.load()
    B, _, L, _, D = LISTS[name][:5]
    lay, g = _setup(dev, name)
    N = lay.N
    r = lambda *s: torch.randn(*s, generator=g).to(dev)
    dmu, fcmean, fb, WT, acc, x1 = r(N, D), r(N, D), r(B, L, D), r(2 * D, D) * 0.1, r(N, D), r(N, D)
    x1h = x1.to(torch.bfloat16)
    want_in, want_w = variant != "weights", variant != "inputs"
    fn = lib.smin_moment_unit_bwd_x1h if variant == "x1h" else lib.smin_moment_unit_bwd
    outs = lambda fill: [torch.full(s, fill, device=dev) for s in ((N, D), (B, L, D), (D, 2 * D), (D,))]
    launch = lambda o, wp, wn: fn(stream(), _vp(dmu), _vp(fcmean), _vp(fb), _vp(lay.cells), _vp(lay.row_ptr), _vp(lay.cellmap), N, B, L, D, _vp(WT),
                                  _vp(o[0]) if want_in else None, _vp(o[1]) if want_in else None, _vp(o[2]) if want_w else None,
                                  _vp(o[3]) if want_w else None, wp, wn, 1, _vp(acc) if want_in else None, _vp(x1h if variant == "x1h" else x1), None)
    return Case(lib.smin_moment_unit_bwd_ws_bytes(N, B, L, D), outs, launch)


def _sc_bwd(dev, name, variant):
    """variant: whole | map | heads (the halves)"""
    import models
    from vml_amd._lib import stream
    lib = models.vml_amd._lib.load()
    B, _, L, _, D = LISTS[name][:5]
    lay, g = _setup(dev, name)
    N = lay.N
    r = lambda *s: torch.randn(*s, generator=g).to(dev)
    pm, psea, dpm, dpsea = torch.sigmoid(r(B, L, L)), torch.sigmoid(r(3, B, L)), r(B, L, L), r(3, B, L)
    fm, fb, wm, wb, lm = r(N, D), r(B, L, D), r(D), r(3, D), (torch.rand(B, L, generator=g) > 0.2).float().to(dev)
    mp, hd = variant != "heads", variant != "map"
    outs = lambda fill: [torch.full(s, fill, device=dev) for s in ((N, D), (B, L, D), (D,), (1,), (3, D), (3,))]
    launch = lambda o, wp, wn: lib.smin_score_map_bwd(stream(), _vp(dpm) if mp else None, _vp(dpsea) if hd else None, _vp(pm), _vp(psea), _vp(fm), _vp(fb),
                                                      _vp(lay.cells), N, B, L, D, _vp(wm), _vp(wb), _vp(lm), _vp(o[0]) if mp else None,
                                                      _vp(o[1]) if hd else None, _vp(o[2]) if mp else None, _vp(o[3]) if mp else None,
                                                      _vp(o[4]) if hd else None, _vp(o[5]) if hd else None, wp, wn)
    return Case(lib.smin_score_map_bwd_ws_bytes(N, B, L, D), outs, launch)


def _cu_bwd(dev, name, variant):
    """variant: dfc (a middle layer, dfc_out given) | mean (dfc_out == NULL) | last (the last layer's N-row form)"""
    import models
    from vml_amd._lib import call, stream
    lib = models.vml_amd._lib.load()
    B, _, L, C, D, dl, Nq = LISTS[name]
    lay, g = _setup(dev, name)
    N = lay.N
    last = variant == "last"
    r = lambda *s: torch.randn(*s, generator=g).to(dev)
    fc, hbar, Wch, bch, Wc, bc = r(N, C, D), r(N, D), r(dl, D) * 0.1, r(dl), r(D, dl) * 0.1, r(D)
    Mq, uq, what, shat, qmask = r(B, Nq, dl) * 0.3, r(B, Nq), r(B, Nq, dl), r(B, dl), torch.ones(B, Nq, device=dev)
    fcmean_in = fc.mean(1).contiguous() if last else None
    fc_out, fcmean, chat, cchat = r(N, C, D), r(N, D), r(N * C, dl), r(N if last else N * C, dl)
    call("smin_content_unit_fwd", stream(), _vp(fc), _vp(hbar), _vp(lay.cells), _vp(lay.row_ptr), N, B, L, C, D, dl, Nq, _vp(Wch), _vp(bch), _vp(Mq),
         _vp(uq), _vp(what), _vp(shat), _vp(qmask), _vp(Wc), _vp(bc), _vp(fcmean_in), int(last), None if last else _vp(fc_out), _vp(fcmean), _vp(chat),
         _vp(cchat))
    WchT, WcT = Wch.t().contiguous(), Wc.t().contiguous()
    dfc_out, dfcmean = (r(N, C, D) if variant == "dfc" else None), r(N, D)
    shapes = ((N, C, D), (N, D), (dl, D), (dl,), (B, Nq, dl), (B, Nq), (B, Nq, dl), (B, dl), (D, dl), (D,))
    outs = lambda fill: [torch.full(s, fill, device=dev) for s in shapes]
    launch = lambda o, wp, wn: lib.smin_content_unit_bwd(stream(), _vp(dfc_out), _vp(dfcmean), _vp(fc), _vp(lay.cells), _vp(lay.row_ptr), N, B, L, C, D, dl, Nq,
                                                         _vp(WchT), _vp(Mq), _vp(uq), _vp(what), _vp(shat), _vp(qmask), _vp(WcT), _vp(chat), _vp(cchat),
                                                         *[_vp(t) for t in o], wp, wn, int(last))
    return Case(lib.smin_content_unit_bwd_ws_bytes(N, B, C, D, dl, int(last)), outs, launch, checked=N > 0)      # N == 0: a no-op (header)


ENTRIES = [("proposal_map_fwd", _pm_fwd, "-"), ("proposal_map_bwd", _pm_bwd, "-"), ("clip_window_means", _cwm, "fwd"), ("clip_window_means", _cwm, "bwd"),
           ("gate_bwd", _gate_bwd, "-")] + [("moment_unit_bwd", _mu_bwd, v) for v in ("whole", "inputs", "weights", "x1h")] + \
          [("score_map_bwd", _sc_bwd, v) for v in ("whole", "map", "heads")] + [("content_unit_bwd", _cu_bwd, v) for v in ("dfc", "mean", "last")]
CASES = [(e, make, v, name) for e, make, v in ENTRIES for name in LISTS]


def _bits(t):
    return t.contiguous().view(torch.int32)


@pytest.mark.gpu
@pytest.mark.parametrize("entry,make,variant,name", CASES, ids=[f"{e}-{v}-{n}" for e, _, v, n in CASES])
def test_exact_workspace_is_enough_and_one_byte_less_is_refused(dev, entry, make, variant, name):
    case = make(dev, name, variant)
    need = case.need
    assert need > 0 and need % 4 == 0, (entry, need)
    # a roomy NaN-filled buffer: the reference
    roomy, _ = _ws_nan(4 * need, dev)
    ref = case.outs(float("nan"))
    assert case.launch(ref, _vp(roomy), 4 * need) == 0
    # exactly `need` bytes, NaN-filled, with a guard behind them inside the allocation
    buf = torch.empty(need + GUARD, dtype=torch.uint8, device=dev)
    buf[:need] = 0xFF
    buf[need:] = 0xA5
    got = case.outs(float("nan"))
    assert case.launch(got, _vp(buf), need) == 0
    torch.cuda.synchronize()
    for k, (a, b) in enumerate(zip(got, ref)):
        assert torch.equal(_bits(a), _bits(b)), (entry, variant, name, f"output {k} differs on a workspace of exactly the query's size")
    assert bool((buf[need:] == 0xA5).all()), (entry, variant, name, "written past the query's size")
    # one byte less
    kept = case.outs(FILL)
    rc = case.launch(kept, _vp(buf), need - 1)
    torch.cuda.synchronize()
    if case.checked:
        assert rc < -1000, (entry, variant, name, rc)
        assert all(bool((t == FILL).all()) for t in kept), (entry, variant, name, "a refused call wrote an output")
    else:                                      # the header: the workspace is neither read nor checked for these arguments
        assert rc == 0, (entry, variant, name, rc)
        full = case.outs(FILL)
        assert case.launch(full, _vp(buf), need) == 0
        torch.cuda.synchronize()
        assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(kept, full)), (entry, variant, name)


def test_queries_reject_what_their_entry_points_reject():
    """0 for a width that is no multiple of 4 and past each limit the entry point's own check names; more than 0 at the limit itself.
    The queries are plain host functions: no device."""
    import models
    lib = models.vml_amd._lib.load()
    for q in (lib.smin_proposal_map_fwd_ws_bytes, lib.smin_proposal_map_bwd_ws_bytes):
        assert q(2, 16, 2048) > 0 and q(2, 16, 4) > 0
        assert q(2, 16, 6) == 0 and q(2, 16, 2052) == 0
    for q in (lib.smin_clip_window_means_fwd_ws_bytes, lib.smin_clip_window_means_bwd_ws_bytes):
        assert q(2, 16, 16, 1) > 0 and q(2, 16, 256, 8) > 0 and q(2, 16, 2048, 1) > 0
        assert q(2, 16, 6, 1) == 0 and q(2, 16, 16, 0) == 0 and q(2, 16, 16, 9) == 0 and q(2, 16, 260, 8) == 0 and q(2, 16, 2052, 1) == 0
    assert lib.smin_gate_bwd_ws_bytes(2, 8, 8) > 0 and lib.smin_gate_bwd_ws_bytes(2, 8, 6) == 0
    assert lib.smin_moment_unit_bwd_ws_bytes(10, 2, 8, 2048) > 0 and lib.smin_moment_unit_bwd_ws_bytes(0, 2, 8, 4) > 0
    assert lib.smin_moment_unit_bwd_ws_bytes(10, 2, 8, 6) == 0 and lib.smin_moment_unit_bwd_ws_bytes(10, 2, 8, 2052) == 0
    assert lib.smin_score_map_bwd_ws_bytes(10, 2, 8, 8) > 0 and lib.smin_score_map_bwd_ws_bytes(0, 2, 8, 8) > 0
    assert lib.smin_score_map_bwd_ws_bytes(10, 2, 8, 6) == 0
    cu = lib.smin_content_unit_bwd_ws_bytes
    for last in (0, 1):
        assert cu(10, 2, 2, 8, 16, last) > 0 and cu(10, 2, 4, 8, 128, last) > 0 and cu(0, 2, 3, 8, 16, last) > 0
        assert cu(10, 2, 3, 6, 16, last) == 0                                             # D % 4
        assert cu(10, 2, 3, 8, 8, last) == 0 and cu(10, 2, 3, 8, 24, last) == 0 and cu(10, 2, 3, 8, 144, last) == 0    # dl
        assert cu(10, 2, 1, 8, 16, last) == 0 and cu(10, 2, 5, 8, 16, last) == 0          # C


def test_layouts_are_the_documented_pieces():
    """The queries against the pieces the sources name, at the three lists: a second, independent statement of each layout."""
    import models
    lib = models.vml_amd._lib.load()
    cdiv = lambda a, b: -(-a // b)
    pad4 = lambda n: (n + 3) & ~3
    for name, (B, T, L, C, D, dl, Nq) in LISTS.items():
        N = int(_mask(name).sum())
        assert lib.smin_proposal_map_fwd_ws_bytes(B, T, D) == 8 * B * (T + 1) * D
        assert lib.smin_proposal_map_bwd_ws_bytes(B, T, D) == 4 * B * T * D
        assert lib.smin_clip_window_means_fwd_ws_bytes(B, T, 16, 3) == 8 * B * (T + 1) * 48
        assert lib.smin_clip_window_means_bwd_ws_bytes(B, T, 16, 3) == 4 * B * T * 48
        mc = min(512, max(1, cdiv(L * L, 32)))
        mc = cdiv(L * L, cdiv(L * L, mc))
        assert lib.smin_gate_bwd_ws_bytes(B, L, D) == 4 * B * mc * D
        sp = {"small": 1, "split": 3, "empty": 1}[name]                                   # tn_splits(N, D, 2D): cdiv(N, 256) caps it here
        assert lib.smin_moment_unit_bwd_ws_bytes(N, B, L, D) == 4 * (pad4(N * D) + sp * (2 * D * D + D))
        nch, hch = cdiv(max(N, 1), 64), cdiv(B * L, 8)
        assert lib.smin_score_map_bwd_ws_bytes(N, B, L, D) == 4 * (nch * D + pad4(nch) + hch * 3 * D + hch * 3)
