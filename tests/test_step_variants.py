"""The step's variants against each other: the packed layout under a caller-supplied cell count (csrc/layout.hip
smin_build_cells_n, SMIN.known_cell_count), replayed HIP graphs and the gradients they deliver (training.CapturedStep), and the
stream placement switches of the one-node step (overlap_boundary, overlap_prep, tail_split, async_weights).

Every assertion is exact: the layout's outputs are integers, and a variant of the step is held to the bits of its twin.

Host: ``layout_ref``, the layout written out from its specification in numpy, against a hand-written example and against
CellLayout's torch formulation on CPU tensors, for exact counts and for truncated masks.
GPU: the two layout entry points through the C ABI against ``layout_ref`` (guard rows behind every output); a step run with an
under-count against the step on the truncated mask; a replayed graph's ``p.grad`` against the eager step of the same batch;
each placement setting against the all-off run."""
import itertools

import numpy as np
import pytest
import torch

from tests import helpers as H
from tests.support.device import dev  # noqa: F401  (the module's device fixture)
from tests.support.device import vml as V

SMALL = (64, 16, 4, 128, 32, 3, 40, 9, 64, 4)             # T, L, C, D, dl, layers, Din, Nq, H, B
# (B, L): byte loop; one 16-byte load; exactly one ballot round; vector loads and two ballot rounds; exactly 1024 rows (one scan
# chunk); a partial second chunk; 1320 rows with odd L; three ballot rounds with a ragged last one
LAYOUT_SHAPES = [(3, 6), (2, 16), (5, 64), (2, 80), (64, 16), (65, 16), (40, 33), (2, 130)]
MASK_BYTES = (1, 2, 16, 128, 255)                         # "non-zero = valid" (include/smin_hip.h): every bit position, low and high nibble
GUARD, SENTINEL = H.LAYOUT_GUARD, H.LAYOUT_SENTINEL
PLACEMENT = ("overlap_boundary", "overlap_prep", "tail_split", "async_weights")
PLACEMENT_SHAPES = [
    SMALL,                                                # the parameter products in csrc/param_prep.hip
    (64, 16, 4, 104, 48, 2, 24, 18, 52, 3),               # D % 32 != 0: torch forms them, on the second stream
    (32, 16, 4, 512, 128, 3, 64, 32, 256, 4),             # the cluster LSTM (H = 256) and dl = 128
]


# ---------------------------------------------------------------- the layout's specification
def layout_ref(mask_u8, all_cells, n_cap):
    """(cells [n_cap][4], row_ptr [B*L + 1], cellmap [B][L][L], status) of include/smin_hip.h's packed layout under a count:
    the listed cells -- the non-zero ones, or with all_cells every (b, i, j) -- in (b, i, j) order, the first min(total, n_cap)
    kept; cells[n] = {b, i, j, mask != 0}, entries total .. n_cap - 1 = {0, 0, 0, 0}; row_ptr[r] = kept cells before row r = b*L + i;
    cellmap = the cell's id, -1 where none is kept; status = 1 iff total != n_cap."""
    valid = np.asarray(mask_u8) != 0
    B, L, _ = valid.shape
    listed = np.argwhere(np.ones_like(valid) if all_cells else valid)      # rows of (b, i, j), in that order
    total = listed.shape[0]
    kept = listed[:min(total, n_cap)]
    where = tuple(kept.T)
    cells = np.zeros((n_cap, 4), dtype=np.int32)
    cells[:len(kept), :3] = kept
    cells[:len(kept), 3] = valid[where]
    cellmap = np.full((B, L, L), -1, dtype=np.int32)
    cellmap[where] = np.arange(len(kept))
    row_ptr = np.zeros(B * L + 1, dtype=np.int32)
    row_ptr[1:] = np.cumsum(np.bincount(kept[:, 0] * L + kept[:, 1], minlength=B * L))
    return cells, row_ptr, cellmap, int(total != n_cap)


def make_mask(B, L, seed, empty=False):
    """uint8 (B, L, L): about 0.4 of the bytes non-zero, drawn from MASK_BYTES; row (0, 1) and sample 1 empty.  empty: all zero."""
    rng = np.random.default_rng(seed)
    mask = np.where(rng.random((B, L, L)) < 0.4, rng.choice(MASK_BYTES, (B, L, L)), 0).astype(np.uint8)
    mask[0, 1] = 0
    mask[1] = 0
    if empty:
        mask[:] = 0
    return mask


def listed_total(mask, all_cells):
    return mask.size if all_cells else int((mask != 0).sum())


def counts_for(mask, all_cells):
    """n_expected of the kernel test: exact, over by 7 and by 300 (more than one 256-stride of the inert fill), under by 1 and by 7,
    a cut on the first sample's boundary, 0."""
    total = listed_total(mask, all_cells)
    first = listed_total(mask[:1], all_cells)
    out = []
    for n in (total, total + 7, total + 300, total - 1, total - 7, first, 0):
        if n >= 0 and n not in out:
            out.append(n)
    return total, out


def truncated(mask, keep):
    """mask with its listed cells after the first ``keep`` cleared"""
    flat = mask.reshape(-1).copy()
    flat[np.flatnonzero(flat)[keep:]] = 0
    return flat.reshape(mask.shape)


def test_layout_ref_on_a_hand_written_mask():
    mask = np.array([[[0, 2, 0], [0, 0, 0], [255, 0, 16]],
                     [[0, 0, 0], [0, 0, 0], [0, 0, 0]],
                     [[1, 0, 0], [0, 128, 1], [0, 0, 0]]], dtype=np.uint8)
    cells, row_ptr, cellmap, status = layout_ref(mask, 0, 6)
    assert cells.tolist() == [[0, 0, 1, 1], [0, 2, 0, 1], [0, 2, 2, 1], [2, 0, 0, 1], [2, 1, 1, 1], [2, 1, 2, 1]] and status == 0
    assert row_ptr.tolist() == [0, 1, 1, 3, 3, 3, 3, 4, 6, 6]
    assert cellmap.reshape(-1).tolist() == [-1, 0, -1, -1, -1, -1, 1, -1, 2] + [-1] * 9 + [3, -1, -1, -1, 4, 5, -1, -1, -1]
    # two cells short: the cut falls behind row (2, 0), and row (2, 1) owns nothing
    cells, row_ptr, cellmap, status = layout_ref(mask, 0, 4)
    assert cells.tolist() == [[0, 0, 1, 1], [0, 2, 0, 1], [0, 2, 2, 1], [2, 0, 0, 1]] and status == 1
    assert row_ptr.tolist() == [0, 1, 1, 3, 3, 3, 3, 4, 4, 4] and int(cellmap.max()) == 3 and cellmap[2, 1].tolist() == [-1, -1, -1]
    # two cells over: inert entries that no row owns
    cells, row_ptr, cellmap, status = layout_ref(mask, 0, 8)
    assert cells[6:].tolist() == [[0, 0, 0, 0]] * 2 and row_ptr[-1] == 6 and status == 1
    # every cell listed, its flag in m; a cut inside row (0, 1)
    cells, row_ptr, cellmap, status = layout_ref(mask, 1, 5)
    assert cells.tolist() == [[0, 0, 0, 0], [0, 0, 1, 1], [0, 0, 2, 0], [0, 1, 0, 0], [0, 1, 1, 0]] and status == 1
    assert row_ptr.tolist() == [0, 3, 5, 5, 5, 5, 5, 5, 5, 5] and cellmap.reshape(-1)[:6].tolist() == [0, 1, 2, 3, 4, -1]
    assert layout_ref(mask, 1, 27)[3] == 0 and layout_ref(mask, 0, 0)[1].tolist() == [0] * 10


def assert_same_layout(layout, ref, what):
    cells, row_ptr, cellmap, _ = ref
    assert layout.N == cells.shape[0], what
    for name, want in (("cells", cells), ("row_ptr", row_ptr), ("cellmap", cellmap)):
        got = getattr(layout, name)
        assert got.dtype == torch.int32 and np.array_equal(got.numpy(), want), (what, name)


@pytest.mark.parametrize("B,L", LAYOUT_SHAPES[:4] + [(40, 33)])
def test_layout_ref_equals_cell_layout_on_the_cpu(B, L):
    """Exact count: CellLayout.from_mask / all_cells on CPU tensors.  Under-count: from_mask of the mask with the surplus cells cleared."""
    CellLayout = V().CellLayout
    for empty in (False, True):
        mask = make_mask(B, L, seed=100 * B + L, empty=empty)
        total = listed_total(mask, 0)
        assert empty or (not mask[0, 1].any() and not mask[1].any() and mask[0].any() and set(np.unique(mask)) == {0, *MASK_BYTES})
        ref = layout_ref(mask, 0, total)
        assert ref[3] == 0
        assert_same_layout(CellLayout.from_mask(torch.from_numpy(mask)), ref, (B, L, empty, "exact"))
        ref_all = layout_ref(mask, 1, mask.size)
        assert ref_all[3] == 0
        assert_same_layout(CellLayout.all_cells(torch.from_numpy(mask)), ref_all, (B, L, empty, "all cells"))
        for n in counts_for(mask, 0)[1]:
            ref_n = layout_ref(mask, 0, n)
            assert ref_n[3] == int(n != total)
            if n <= total:
                assert_same_layout(CellLayout.from_mask(torch.from_numpy(truncated(mask, n))), ref_n, (B, L, empty, n))
            else:                                         # the exact layout and n - total inert entries
                assert np.array_equal(ref_n[0][:total], ref[0]) and not ref_n[0][total:].any()
                assert np.array_equal(ref_n[1], ref[1]) and np.array_equal(ref_n[2], ref[2])


# ---------------------------------------------------------------- the layout kernels through the C ABI
def assert_kernel_layout(got, ref, what):
    (cells, row_ptr, cellmap), (rcells, rrow, rmap, _) = got, ref
    n, rows, nmap = rcells.shape[0], rrow.shape[0], rmap.size
    cells, row_ptr, cellmap = cells.cpu().numpy(), row_ptr.cpu().numpy(), cellmap.cpu().numpy()
    assert (cells[n:] == SENTINEL).all() and (row_ptr[rows:] == SENTINEL).all() and (cellmap[nmap:] == SENTINEL).all(), (what, "written past the end")
    assert int(row_ptr[:rows].max()) <= n, (what, "row_ptr past the cell list", int(row_ptr[:rows].max()), n)
    assert np.array_equal(row_ptr[:rows], rrow), (what, "row_ptr")
    assert np.array_equal(cells[:n], rcells), (what, "cells")
    assert np.array_equal(cellmap[:nmap].reshape(rmap.shape), rmap), (what, "cellmap")


@pytest.mark.gpu
@pytest.mark.parametrize("B,L", LAYOUT_SHAPES)
def test_layout_kernels_under_a_known_count(dev, B, L):
    """smin_build_cells and smin_build_cells_n against layout_ref: every output exactly, nothing written behind any of them, the
    status word set on a miscount and left as found (0 or 1) on an exact count."""
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    for empty, all_cells in itertools.product((False, True), (0, 1)):
        mask = make_mask(B, L, seed=100 * B + L, empty=empty)
        mask_d = torch.from_numpy(mask).to(dev)
        total, counts = counts_for(mask, all_cells)
        what = (B, L, "empty" if empty else "random", "all" if all_cells else "valid")
        assert_kernel_layout(H.build_cells(dev, mask_d, all_cells, total), layout_ref(mask, all_cells, total), what + ("smin_build_cells",))
        for n in counts:
            ref = layout_ref(mask, all_cells, n)
            for preset in ((0, 1) if n == total else (0,)):
                status.fill_(preset)
                got = H.build_cells(dev, mask_d, all_cells, n, n, status)
                assert int(status.item()) == max(preset, ref[3]), what + (n, total, "status", preset)
                assert_kernel_layout(got, ref, what + (n, total))


# ---------------------------------------------------------------- the step on the small shape
def build_model(shape, sd, dev):
    import models
    T, L, C, D, dl, layers, Din, Nq, Hh, _ = shape
    m = models.SMIN(T, L, C, D, dl, layers, Din, Nq, Hh, dev)
    missing = m.load_state_dict(sd, strict=True)
    assert not missing.missing_keys and not missing.unexpected_keys
    return m.to(dev)


def state_dict_of(shape):
    from oracle import smin_oracle as O                   # seeded inputs and weights only
    return O.formula_state_dict(H.smin_shapes(*shape[:9]), gain=1.2)


def batch_of(shape, dev, seed):
    from oracle import smin_oracle as O
    T, L, _, _, _, _, Din, Nq, _, B = shape
    return {k: v.to(dev) for k, v in O.synthetic_batch(B, T, L, Nq, Din, seed=seed).items()}


def loss_of(out, t):
    return V().loss_fn(out[0], t["ym"], t["sm"], t["moment_mask"], out[1], t["ys"], t["ss"], out[2], t["ye"], t["se"], out[3], t["ya"], t["length_mask"])


def eager_step(m, b, loss_mask=None):
    """forward, loss, backward: (loss, the four outputs, the gradients by parameter name), cloned"""
    for p in m.parameters():
        p.grad = None
    out = m(*H.model_inputs(b))
    loss = loss_of(out, b if loss_mask is None else dict(b, moment_mask=loss_mask))
    loss.backward()
    torch.cuda.synchronize()
    return loss.detach().clone(), [o.detach().clone() for o in out], {k: p.grad.clone() for k, p in m.named_parameters()}


def differing(got, want):
    """names of the tensors of two eager_step results that differ in any bit"""
    names = [] if torch.equal(got[0], want[0]) else ["loss"]
    names += [n for n, a, w in zip(("pm", "ps", "pe", "pa"), got[1], want[1]) if not torch.equal(a, w)]
    assert set(got[2]) == set(want[2])
    return names + [k for k, g in got[2].items() if not torch.equal(g, want[2][k])]


@pytest.fixture(scope="module")
def small(dev):
    sd = state_dict_of(SMALL)
    b1, b3 = batch_of(SMALL, dev, 11), batch_of(SMALL, dev, 12)
    assert int(b3["moment_mask"].sum()) != int(b1["moment_mask"].sum())
    return dict(sd=sd, b1=b1, b3=b3)


@pytest.mark.gpu
def test_undercounted_step_is_the_truncated_masks_step(dev, small):
    """known_cell_count = n - 7: the status word is raised, and the step -- outputs, loss and every gradient -- is bit for bit the
    step on the mask with its last 7 cells cleared (the core reads moment_mask through the layout only; the loss, which the caller
    feeds, gets the cleared mask in both runs).  A correct step afterwards equals the same step before."""
    b = small["b1"]
    n = int(b["moment_mask"].sum())
    assert H.fail_unless_row_ptr_is_clamped(dev, b["moment_mask"], n - 7) == 1
    cleared = torch.from_numpy(truncated(b["moment_mask"].cpu().numpy().astype(np.uint8), n - 7)).to(dev).bool()
    assert int(cleared.sum()) == n - 7 and int((cleared & ~b["moment_mask"]).sum()) == 0
    m = build_model(SMALL, small["sd"], dev)
    status = V()._lib.load_torch().layout_status(dev)
    status.zero_()
    try:
        before = eager_step(m, b)
        m.known_cell_count = n - 7
        want = eager_step(m, dict(b, moment_mask=cleared))
        assert int(status.item()) == 0                                 # the exact count of the cleared mask
        got = eager_step(m, b, loss_mask=cleared)
        assert int(status.item()) == 1
        assert not differing(got, want), differing(got, want)
        assert all(bool(torch.isfinite(t).all()) for t in [got[0]] + got[1] + list(got[2].values()))
        assert float(got[1][0][~cleared].abs().max()) == 0.0           # no score where no cell is kept
        m.known_cell_count = None
        status.zero_()
        after = eager_step(m, b)
        assert int(status.item()) == 0
        assert not differing(after, before), differing(after, before)
    finally:
        m.known_cell_count = None
        status.zero_()


# ---------------------------------------------------------------- replayed graphs deliver their own gradients
def assert_step_equals(m, loss, out, want, what):
    torch.cuda.synchronize()
    assert torch.equal(loss.detach(), want[0]), (what, "loss")
    for name, a, w in zip(("pm", "ps", "pe", "pa"), out, want[1]):
        assert torch.equal(a.detach(), w), (what, name)
    for k, p in m.named_parameters():
        assert p.grad is not None, (what, k, "p.grad is None")
        assert torch.equal(p.grad, want[2][k]), (what, k)


@pytest.mark.gpu
def test_replay_delivers_the_replayed_graphs_gradients(dev, small):
    """CapturedStep(model, optimizer=None) with two graphs alive: after a replay p.grad holds that batch's gradients, whether the
    caller set the grads to None in between or the other graph ran last."""
    b1, b3 = small["b1"], small["b3"]
    m = build_model(SMALL, small["sd"], dev)
    step = V().CapturedStep(m, None)                               # (no optimizer: the warm-up steps change no parameter)
    want1, want3 = eager_step(m, b1), eager_step(m, b3)
    assert differing(want1, want3)                                  # two batches the test can tell apart
    step(b1)
    step(b3)
    for p in m.parameters():
        p.grad = None
    loss, out = step(b1)
    assert_step_equals(m, loss, out, want1, "b1 after grads set to None")
    loss, out = step(b3)
    assert_step_equals(m, loss, out, want3, "b3")
    loss, out = step(b1)                                            # p.grad untouched since b3's replay
    assert_step_equals(m, loss, out, want1, "b1 after b3")
    assert len(step.entries) == 2


@pytest.mark.gpu
def test_evicted_graph_is_captured_again(dev, small):
    """max_graphs = 1: every change of the cell count evicts the one graph; each call still equals the eager step."""
    m = build_model(SMALL, small["sd"], dev)
    step = V().CapturedStep(m, None, max_graphs=1)
    for name in ("b1", "b3", "b1"):
        want = eager_step(m, small[name])
        for p in m.parameters():
            p.grad = None
        loss, out = step(small[name])
        assert len(step.entries) == 1
        assert_step_equals(m, loss, out, want, name)


# ---------------------------------------------------------------- placement changes no bit
def with_placement(m, names, setting):
    for name, on in zip(names, setting):
        setattr(m, name, on)
    return m


def settings_of(names):
    """all-off first (the run the others are compared with), each setting once"""
    return list(itertools.product((False, True), repeat=len(names)))


@pytest.mark.gpu
@pytest.mark.parametrize("shape", PLACEMENT_SHAPES, ids=lambda s: "D%d_dl%d_H%d" % (s[3], s[4], s[8]))
def test_placement_changes_no_bit_of_the_step(dev, shape):
    """forward, loss_fn and backward under the 16 settings of the four placement switches, a fresh model from one state dict each:
    the outputs and every parameter gradient equal the all-off run's."""
    sd, b = state_dict_of(shape), batch_of(shape, dev, 11)
    base, diffs = None, {}
    for setting in settings_of(PLACEMENT):
        m = with_placement(build_model(shape, sd, dev), PLACEMENT, setting)
        assert m._plan(b["video_features"], b["query_features"]) == "node"
        got = eager_step(m, b)
        if base is None:
            base = got
        elif differing(got, base):
            diffs[setting] = differing(got, base)
    assert not diffs, f"{PLACEMENT}: tensors that differ from the all-off run {diffs}"
    assert V()._lib.load().smin_lstm_cluster_error() == 0, "a bounded poll of the cluster recurrence expired"
    assert int(V()._lib.load_torch().layout_status(dev)[0]) == 0


@pytest.mark.gpu
def test_placement_changes_no_bit_of_score(dev, small):
    names = ("overlap_boundary", "overlap_prep")
    b = small["b1"]
    base, diffs = None, {}
    for setting in settings_of(names):
        m = with_placement(build_model(SMALL, small["sd"], dev), names, setting).eval()
        assert m._plan(b["video_features"], b["query_features"]) == "node"
        got = [o.clone() for o in m.score(*H.model_inputs(b))]
        torch.cuda.synchronize()
        if base is None:
            base = got
        else:
            bad = [n for n, a, w in zip(("pm", "ps", "pe", "pa"), got, base) if not torch.equal(a, w)]
            if bad:
                diffs[setting] = bad
    assert not diffs, f"{names}: scores that differ from the all-off run {diffs}"


@pytest.mark.gpu
def test_placement_changes_no_bit_of_forward_pairs(dev, small):
    """forward_pairs, loss_fn over the pairs and backward: 3 videos, 4 queries, 7 pairs, the eight settings of its three switches."""
    names = ("overlap_boundary", "async_weights", "tail_split")
    b = small["b1"]
    vid = {k: b[k][:3] for k in ("video_features", "video_mask", "length_mask", "moment_mask")}
    qry = {k: b[k] for k in ("query_features", "query_mask")}
    vi, qi, gt = [0, 1, 2, 0, 2, 1, 0], [0, 1, 2, 3, 0, 3, 1], [0, 1, 2, 0]
    targets = V().pair_targets(vid, {k: b[k] for k in ("ym", "sm", "ys", "ss", "ye", "se", "ya")}, vi, qi, gt)
    base, diffs = None, {}
    for setting in settings_of(names):
        m = with_placement(build_model(SMALL, small["sd"], dev), names, setting)
        assert m._bank_plan(vid["video_features"], qry["query_features"])
        out = m.forward_pairs(vid["video_features"], vid["video_mask"], qry["query_features"], qry["query_mask"], vid["length_mask"], vid["moment_mask"], vi, qi)
        loss = loss_of(out, targets)
        loss.backward()
        torch.cuda.synchronize()
        got = (loss.detach().clone(), [o.detach().clone() for o in out], {k: p.grad.clone() for k, p in m.named_parameters()})
        if base is None:
            base = got
        elif differing(got, base):
            diffs[setting] = differing(got, base)
    assert not diffs, f"{names}: tensors that differ from the all-off run {diffs}"
    assert int(V()._lib.load_torch().layout_status(dev)[0]) == 0
