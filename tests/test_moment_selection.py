"""Top-k moment selection (csrc/moments.hip, smin_top_moments) over band layouts, ties and signed scores, and the tie rule and
top-5 insertion of the rule-0 metric kernel (csrc/metrics.hip, ious_kernel).

tests/test_moments.py launches one band layout above L = 64 (P = 32, MB = 128), scores in [0, 1) only, and no continuation that
ends with fewer than k kept.  Here every device list is compared bit for bit with `py_nms` (tests/test_moments.py: plain Python +
numpy fp32, written from the definition) on score families that reach `score_ord`'s sign branch, -0 against +0, infinities,
subnormals, ties inside one radix digit bin and values that differ in the second or the third digit only; on the band layouts
P = 1, 3, 5, 7, 9 and 16; and on walks that use up the exact prefix and the continuation's re-selects.  A Python model of
`band_count` / `ws_layout` says, for each sample, which bands are full, how long the exact prefix is and how far the greedy walk
goes; the CPU tests assert on it that the device cases reach the paths they claim, and `smin_top_moments_ws_bytes` is pinned to the
model so that a change of `band_count` or CAND cannot leave those cases quietly off their paths.

Subnormal scores are part of the contract (the library is built without flush-to-zero; include/smin_hip.h says so): the `subnormal`
family must come back with its bits.  `zeros` puts -0 and +0 at the top of the order, where every (k, nms_thresh) reaches them.

Out of scope: NaN scores at valid cells.  Host and device sqrt need not agree on a NaN's payload and the order of NaNs is by their
bits; NaN (and +-inf) at masked cells is in scope (`nan_masked`): it must never be read into the order.

The rule-0 metric is compared with a numpy reference written from metrics.hip's header: fp32 score ((pm * sqrt(ps_i)) * sqrt(pe_j))
* mask over all L*L cells, higher first, ties to the lower flat index, top five, a hit when sm at a top-n cell is > float32(m)."""

import functools

import numpy as np
import pytest
import torch

from tests.helpers import cdiv
from tests.support.device import dev  # noqa: F401  (the module's device fixture)
from tests.support.references import _api, check_against_py, py_iou, py_nms, py_scores

CAND = 4096                       # csrc/moments.hip: candidate keys the NMS workgroup holds
MAX_BANDS, MIN_BAND = 32, 1024    # csrc/moments.hip band_count
MAX_B = 65535                     # the band select's grid y coordinate

KT = ((64, 0.0), (64, 0.5), (5, 0.3), (1, 1.0), (64, 1.0))         # the (k, nms_thresh) of every device call
L96_LAYOUTS = {512: (1, 4096), 171: (3, 1365), 103: (5, 819), 74: (7, 585), 2: (9, 455)}      # B -> (P, MB) at L = 96
# (B, L) of the layout matrix: the five of the table, B = 13 (P = 9 again, with every family in the batch), and L = 128 (P = 16)
MATRIX = [(512, 96), (171, 96), (103, 96), (74, 96), (2, 96), (13, 96), (7, 128)]


# ---------------------------------------------------------------- score families: one sample each, a function of (L, seed)
def _triu(L, length=None):
    ok = torch.arange(L) < (L if length is None else length)
    return torch.triu(ok.view(L, 1) & ok.view(1, L))


def _bits(u):
    return u.to(torch.int32).view(torch.float32)


def _uniform(L, g):
    return torch.rand(L, L, generator=g), torch.rand(L, generator=g), torch.rand(L, generator=g), _triu(L)


def _fixed(pm):
    """ps = pe = 1: sqrt(1) and the products are exact, so pm's bits are the score's."""
    L = pm.shape[0]
    return pm.contiguous(), torch.ones(L), torch.ones(L), _triu(L)


def fam_uniform(L, g):
    return _uniform(L, g)


def fam_signed(L, g):
    pm, ps, pe, mm = _uniform(L, g)
    return 2 * pm - 1, ps, pe, mm


def fam_levels(L, g):
    levels = torch.tensor([-0.5, -0.25, -0.0, 0.0, 0.25, 0.5])
    return _fixed(levels[torch.randint(0, 6, (L, L), generator=g)])


def fam_zeros(L, g):
    """-0, +0 and -0.5 in equal parts, cell (0, 0) a -0: the top two thirds of the order are one tie, decided by index alone, and its
    members interleave with cells outside it, so the select's rank base across waves and rounds, and -0 against +0, decide every list
    (in `levels` the zeros lie too deep in the order for most (k, nms_thresh) to reach them)."""
    pm = torch.tensor([-0.0, 0.0, -0.5])[torch.randint(0, 3, (L, L), generator=g)]
    pm[0, 0] = -0.0
    return _fixed(pm)


def fam_lowbits(L, g):
    return _fixed(_bits(0x3F000000 + torch.randint(0, 1024, (L, L), generator=g)))


def fam_midbits(L, g):
    return _fixed(_bits(0x3F000000 + (torch.randint(0, 2048, (L, L), generator=g) << 10)))


def fam_desc(L, g):
    n = L * L
    return _fixed((1 - torch.arange(n, dtype=torch.float32) / n).view(L, L))


def fam_asc(L, g):
    n = L * L
    return _fixed((torch.arange(1, n + 1, dtype=torch.float32) / n).view(L, L))


def fam_longfirst(L, g):
    i, j = torch.arange(L).view(L, 1), torch.arange(L).view(1, L)
    return _fixed((j - i + 1).clamp_min(0).float() / L)


def fam_inf(L, g):
    pm, ps, pe, mm = _uniform(L, g)
    cells = mm.flatten().nonzero().flatten()
    pick = cells[torch.randperm(cells.numel(), generator=g)[:6]]
    pm.view(-1)[pick[:3]] = float("inf")
    pm.view(-1)[pick[3:]] = float("-inf")
    return pm, ps, pe, mm


def fam_subnormal(L, g):
    return torch.rand(L, L, generator=g) * 1e-30, torch.full((L,), 1e-16), torch.ones(L), _triu(L)


def fam_short(L, g):
    """valid length 50 of 96 (in proportion at other L): trailing bands empty"""
    pm, ps, pe, _ = _uniform(L, g)
    return pm, ps, pe, _triu(L, max(1, L * 25 // 48))


def fam_nan_masked(L, g):
    pm, ps, pe, mm = _uniform(L, g)
    junk = torch.tensor([float("nan"), float("inf"), float("-inf")])
    off = (~mm).flatten().nonzero().flatten()
    pm.view(-1)[off] = junk[torch.arange(off.numel()) % 3]
    return pm, ps, pe, mm


FAMILIES = [fam_uniform, fam_signed, fam_levels, fam_zeros, fam_lowbits, fam_midbits, fam_desc, fam_asc, fam_longfirst, fam_inf,
            fam_subnormal, fam_short, fam_nan_masked]
NAMES = [f.__name__[4:] for f in FAMILIES]
F = len(FAMILIES)
FULL_LENGTH = [q for q, name in enumerate(NAMES) if name != "short"]
RANDOM_VALUED = [NAMES.index(name) for name in ("uniform", "signed", "levels", "zeros", "lowbits", "midbits", "inf")]
SEED = 3


@functools.lru_cache(maxsize=None)
def sample(L, q):
    """Family q's sample at L: (pm (L, L), ps (L,), pe (L,), mm (L, L) bool).  Shared, never written."""
    return FAMILIES[q](L, torch.Generator().manual_seed(1000 * SEED + 10 * q + L))


@functools.lru_cache(maxsize=None)
def reference(L, q, k, thr):
    """py_nms of family q's sample: [(i, j, score)]."""
    return py_nms(*(x.numpy() for x in sample(L, q)), k, thr)


def batch(B, L):
    """Row b is family sample b % F: a wrong per-sample offset shows as a row that matches another sample's reference."""
    rows = [sample(L, b % F) for b in range(B)]
    return tuple(torch.stack([r[x] for r in rows]) for x in range(4))


def assert_row(r, b, want, what):
    """check_against_py's assertions for row b against a py_nms list: order, score bits, the -1 / 0 tail, count."""
    n = len(want)
    assert int(r["count"][b]) == n, what
    assert r["idx"][b, :n].tolist() == [[i, j] for i, j, _ in want], what
    assert np.array_equal(r["score"][b, :n].numpy().view(np.int32), np.array([s for _, _, s in want], np.float32).view(np.int32)), what
    assert (r["idx"][b, n:] == -1).all() and (r["score"][b, n:] == 0).all(), what


# ---------------------------------------------------------------- the layout model (band_count / ws_layout of csrc/moments.hip)
def layout(B, L):
    """(P, MB, band): bands per sample, keys each band hands over, cells per band."""
    n = L * L
    P = max(1, min(cdiv(512, B), MAX_BANDS, cdiv(n, MIN_BAND)))
    return P, CAND // P, cdiv(n, P)


def ws_bytes(B, L):
    P, MB, _ = layout(B, L)
    a256 = lambda x: (x + 255) & ~255
    return a256(B * P * MB * 8) + a256(B * P * 8) + a256(B * P * 4)


@functools.lru_cache(maxsize=None)
def candidate_order(L, q):
    """The valid cells of family q's sample in py_nms's candidate order (its sort, restated)."""
    pm, ps, pe, mm = (x.numpy() for x in sample(L, q))
    s = py_scores(pm, ps, pe)
    cand = [(-float(s[i, j]), i * L + j) for i in range(L) for j in range(L) if mm[i, j]]
    cand.sort()
    return [c for _, c in cand]


@functools.lru_cache(maxsize=None)
def walk(L, q, k, thr):
    """(candidates the greedy walk visits, moments kept): py_nms's loop over `candidate_order`, counting."""
    t = np.float32(thr)
    kept, visits = [], 0
    for c in candidate_order(L, q):
        if len(kept) >= k:
            break
        visits += 1
        cell = (c // L, c % L)
        if all(not (py_iou(cell, o) > t) for o in kept):
            kept.append(cell)
    assert kept == [(i, j) for i, j, _ in reference(L, q, k, thr)]
    return visits, len(kept)


def model(B, L, q):
    """(full, prefix): which bands of family q's sample hold more than MB valid cells, and the size of the exact prefix -- the keys at
    or above the largest of the full bands' MB-th keys (every valid cell if no band is full)."""
    P, MB, band = layout(B, L)
    order = candidate_order(L, q)
    rank = {c: r for r, c in enumerate(order)}
    per_band = [[] for _ in range(P)]
    for c in order:                                                     # each band's cells, in candidate order
        per_band[c // band].append(c)
    full = [len(cells) > MB for cells in per_band]
    floors = [rank[cells[MB - 1]] for cells, f in zip(per_band, full) if f]
    return full, (min(floors) + 1 if floors else len(order))


# ---------------------------------------------------------------- CPU
def test_families_are_what_they_claim():
    L = 96
    for q, name in enumerate(NAMES):
        pm, ps, pe, mm = sample(L, q)
        assert pm.dtype == torch.float32 and mm.dtype == torch.bool and pm.is_contiguous() and mm.is_contiguous(), name
        s = py_scores(pm.numpy(), ps.numpy(), pe.numpy())
        assert not np.isnan(s[mm.numpy()]).any(), name                  # NaN at valid cells is out of scope
        assert int(mm.sum()) == (1275 if name == "short" else L * (L + 1) // 2), name
    valid = sample(L, 0)[3].numpy()
    score = lambda name: py_scores(*(x.numpy() for x in sample(L, NAMES.index(name))[:3]))
    bits = lambda name: score(name)[valid].view(np.uint32)
    assert (score("signed")[valid] < 0).sum() > 1000 and (score("signed")[valid] > 0).sum() > 1000
    lv = sample(L, NAMES.index("levels"))[0].numpy()[valid]
    assert (np.signbit(lv) & (lv == 0)).sum() > 100 and (~np.signbit(lv) & (lv == 0)).sum() > 100       # -0 and +0 both present
    assert len(set(lv.view(np.uint32).tolist())) == 6
    zs = sample(L, NAMES.index("zeros"))[0].numpy()
    assert zs[0, 0] == 0 and np.signbit(zs[0, 0])
    assert all((zs[valid].view(np.uint32) == u).sum() > 1000 for u in (0x80000000, 0, 0xBF000000))     # -0, +0, -0.5
    assert reference(L, NAMES.index("zeros"), 1, 1.0) == [(0, 0, np.float32(0))] and not np.signbit(reference(L, NAMES.index("zeros"), 1, 1.0)[0][2])
    low, mid = bits("lowbits") | 0x80000000, bits("midbits") | 0x80000000                               # score_ord of a positive score
    assert len(set((low >> 10).tolist())) == 1 and len(set((low & 0x3FF).tolist())) > 900               # the third digit decides, with ties
    assert len(set((mid >> 21).tolist())) == 1 and len(set(((mid >> 10) & 0x7FF).tolist())) > 1500 and not (mid & 0x3FF).any()
    inf = score("inf")[valid]
    assert (inf == np.inf).sum() == 3 and (inf == -np.inf).sum() == 3
    sub = score("subnormal")[valid]
    assert ((sub > 0) & (sub < np.finfo(np.float32).tiny)).sum() > 4000                                 # subnormal and not flushed
    assert len(set(sub.view(np.uint32).tolist())) > 4000
    junk = sample(L, NAMES.index("nan_masked"))[0].numpy()[~valid]
    assert np.isnan(junk).sum() > 1000 and np.isinf(junk).sum() > 2000
    for name in ("desc", "asc"):
        assert len(set(bits(name).tolist())) == valid.sum()                                             # tie-free: the order is the index's
    assert candidate_order(L, NAMES.index("desc")) == sorted(candidate_order(L, NAMES.index("desc")))
    assert candidate_order(L, NAMES.index("asc")) == sorted(candidate_order(L, NAMES.index("asc")), reverse=True)


@pytest.mark.parametrize("q", range(F), ids=NAMES)
def test_torch_restatement_equals_python_nms_on_every_family(q):
    """top_moments_torch builds its order word by the kernel's bit trick; py_nms compares floats.  A shared misreading of the order on
    signed or special values would show here."""
    api = _api()
    pm, ps, pe, mm = (x.unsqueeze(0) for x in sample(40, q))
    for k in (1, 5, 64):
        for thr in (0.0, 0.3, 0.5, 1.0):
            r = api.top_moments_torch(pm, ps, pe, mm, k=k, nms_thresh=thr)
            check_against_py(r, pm, ps, pe, mm, k, thr)


def test_layouts_at_l96_and_l128():
    for B, (P, MB) in L96_LAYOUTS.items():
        assert layout(B, 96)[:2] == (P, MB), B
        if P & (P - 1):
            assert P * MB < CAND                                        # MB = CAND / P truncates
    assert layout(13, 96)[:2] == (9, 455)
    assert layout(7, 128)[:2] == (16, 256)
    assert layout(7, 197)[:2] == (32, 128) and layout(2, 512)[:2] == (32, 128)     # tests/test_moments.py's only layout above L = 64
    assert [layout(B, 96)[2] % 96 for B in (103, 74, 2)] == [20, 69, 64]           # these bands' cuts fall in the middle of a row


@pytest.mark.parametrize("B", list(L96_LAYOUTS))
def test_model_says_the_l96_cases_reach_their_paths(B):
    L = 96
    P, MB, band = layout(B, L)
    for q in FULL_LENGTH:
        full, prefix = model(B, L, q)
        assert any(full), (B, NAMES[q])
        assert P == 1 or not all(full), (B, NAMES[q])
    # the walk passes the exact prefix and ends, after the continuation's re-selects, with fewer than k kept
    for q in RANDOM_VALUED:
        _, prefix = model(B, L, q)
        visits, kept = walk(L, q, 64, 0.0)
        assert visits == len(candidate_order(L, q)) > prefix and kept < 64, (B, NAMES[q], prefix, visits, kept)
    q = NAMES.index("longfirst")
    assert walk(L, q, 64, 0.0) == (L * (L + 1) // 2, 1) and model(B, L, q)[1] < L * (L + 1) // 2
    # desc: band 0 holds the whole top, so the floor is its MB-th key and the prefix is exactly its MB keys
    q = NAMES.index("desc")
    full, prefix = model(B, L, q)
    assert full[0] and prefix == MB, (B, prefix)
    if P > 1:
        assert walk(L, q, 64, 0.5)[0] > MB, B
    # asc: the top lies in the last bands, the full bands' floors below it
    full, prefix = model(B, L, NAMES.index("asc"))
    assert prefix > MB or P == 1, (B, prefix)
    # short: trailing bands empty, the first one not
    if P >= 3:
        cells = candidate_order(L, NAMES.index("short"))
        assert max(cells) // band < P - 1 and min(cells) // band == 0, B


def test_model_says_l128_takes_two_continuation_rounds():
    """L = 128, B = 7: P = 16.  The uniform walk at (64, 0.0) visits every valid cell from a prefix short enough that more than CAND
    remain after it: the first re-select leaves `more` set and a second one follows, both entered with kept moments in LDS."""
    B, L = 7, 128
    q = NAMES.index("uniform")
    full, prefix = model(B, L, q)
    visits, kept = walk(L, q, 64, 0.0)
    print("L=128 full bands", sum(full), "prefix", prefix, "visits", visits, "kept", kept)
    assert 1 < sum(full) < 16
    assert visits == 8256 and visits - prefix > CAND and 0 < kept < 64
    for q in range(B):                                                  # the rows of the device batch
        assert walk(L, q, 64, 0.0)[0] > model(B, L, q)[1], NAMES[q]


def test_workspace_size_is_the_layout_models():
    """smin_top_moments_ws_bytes against the Python model.  If this fails, band_count, CAND or the workspace changed: re-derive the
    layout cases of this file (L96_LAYOUTS, MATRIX) before touching the expected sizes."""
    lib = _api()._lib.load()
    for B, L in MATRIX + [(7, 197), (2, 512)]:
        assert lib.smin_top_moments_ws_bytes(B, L, 64) == ws_bytes(B, L), (B, L, layout(B, L))


def test_batches_beyond_the_grid_limit_are_refused_before_any_launch():
    api = _api()
    lib = api._lib.load()
    assert lib.smin_top_moments_ws_bytes(MAX_B, 8, 5) == ws_bytes(MAX_B, 8)
    assert lib.smin_top_moments_ws_bytes(MAX_B + 1, 8, 5) == 0
    assert lib.smin_compute_ious_nms_ws_bytes(MAX_B, 8, 5, 2, 4) > 0
    assert lib.smin_compute_ious_nms_ws_bytes(MAX_B + 1, 8, 5, 2, 4) == 0
    assert lib.smin_epoch_meter_ws_bytes(MAX_B + 1, 8, 1, 5, 2, 4) == 0
    B = MAX_B + 1
    pm, ps, pe, mm = torch.zeros(B, 1, 1), torch.ones(B, 1), torch.ones(B, 1), torch.ones(B, 1, 1, dtype=torch.bool)
    assert api.moments._check(pm[:MAX_B], ps[:MAX_B], pe[:MAX_B], mm[:MAX_B], 5) == (MAX_B, 1)
    with pytest.raises(ValueError, match="B <= 65535"):
        api.moments._check(pm, ps, pe, mm, 5)
    with pytest.raises(ValueError, match="B <= 65535"):
        api.top_moments_torch(pm, ps, pe, mm, k=1)
    with pytest.raises(ValueError, match="B <= 65535"):
        api.compute_ious_torch(pm, ps, pe, mm, pm, nms_thresh=0.5)


# ---------------------------------------------------------------- rule 0: numpy reference from csrc/metrics.hip's header
REF_N, REF_M = (1, 5), (0.1, 0.3, 0.5, 0.7)


def np_rule0(pm, ps, pe, mm, sm):
    """({"R@n, IoU=m": samples with a hit}, top-1 IoU per sample fp32) of a batch, by the header: fp32 score ((pm * sqrt(ps_i)) *
    sqrt(pe_j)) * mask over all L*L cells; higher first, ties -> lower flat index; sm at the top five; hit: sm > float32(m)."""
    pm, ps, pe, sm = (np.asarray(x, dtype=np.float32) for x in (pm, ps, pe, sm))
    B, L = ps.shape
    s = ((pm * np.sqrt(ps)[:, :, None]) * np.sqrt(pe)[:, None, :]) * np.asarray(mm != 0, dtype=np.float32)
    hits = {f"R@{n}, IoU={m}": 0.0 for n in REF_N for m in REF_M}
    top1 = np.zeros(B, np.float32)
    for b in range(B):
        flat = s[b].reshape(-1)
        top = sorted(range(L * L), key=lambda c: (-float(flat[c]), c))[:5]          # -0 == +0 as floats: the index decides
        iou = sm[b].reshape(-1)[top]
        top1[b] = iou[0]
        for n in REF_N:
            for m in REF_M:
                hits[f"R@{n}, IoU={m}"] += float((iou[:n] > np.float32(m)).any())
    return hits, top1, s


def _next_up(x):
    return np.nextafter(np.float32(x), np.float32(2))


def rule0_inputs(B, L):
    """[(name, pm, ps, pe, mm, sm)]: the inputs of section "rule-0 metric kernel", each (B, ...)."""
    g = torch.Generator().manual_seed(77 * L + B)
    stack = lambda q: tuple(torch.stack([FAMILIES[q](L, g)[x] for _ in range(B)]) for x in range(4))
    rand_sm = lambda: torch.rand(B, L, L, generator=g)                               # non-zero at masked cells too
    out = []
    # ties among the valid cells (and, below the diagonal, masked zeros tied with the valid +-0 cells)
    out.append(("levels",) + stack(NAMES.index("levels")) + (rand_sm(),))
    # masked zeros outrank the negative valid cells: sm at masked cells is read
    out.append(("signed",) + stack(NAMES.index("signed")) + (rand_sm(),))
    # the best cells share one thread: flat indices r, r + 256, ... (six of them where L*L allows), rising or falling by row
    n = L * L
    pm = torch.rand(B, n, generator=g)
    for b in range(B):
        cells = list(range((7 * b + 3) % min(n, 256), n, 256))[:6]
        for rank, c in enumerate(cells if b % 2 else cells[::-1]):
            pm[b, c] = 2.0 + rank
    ones = torch.ones(B, L)
    sm = rand_sm().view(B, n)
    for b in range(B):                                                  # rows 0, 3, ..: only the fifth best cell can hit; rows 1, 4, ..: only
        if b % 3 < 2:                                                   # the sixth, which must not (the score is pm: ps = pe = 1, full mask)
            order = sorted(range(n), key=lambda c: (-float(pm[b, c]), c))
            sm[b] = 0
            sm[b, order[4 + b % 3]] = 0.9
    out.append(("one_thread", pm.view(B, L, L), ones, ones, torch.ones(B, L, L, dtype=torch.bool), sm.view(B, L, L)))
    # all-masked samples (every other row; the only row at B = 1): every score is +-0 and cells 0..4 are the top five
    pm, ps, pe, mm = stack(NAMES.index("signed"))
    mm = mm.clone()
    mm[::2] = False
    out.append(("all_masked", pm, ps, pe, mm, rand_sm()))
    # sm exactly at a threshold, or one float above it, at the top cell and at the fifth: the comparison is strict
    pm, ps, pe, mm = stack(NAMES.index("uniform"))
    _, _, s = np_rule0(pm.numpy(), ps.numpy(), pe.numpy(), mm.numpy(), np.zeros((B, L, L), np.float32))
    edge = [v for m in REF_M for v in (np.float32(m), _next_up(m))]
    sm = torch.zeros(B, n)
    for b in range(B):
        flat = s[b].reshape(-1)
        top = sorted(range(n), key=lambda c: (-float(flat[c]), c))[:5]
        sm[b, top[0]] = float(edge[b % 8])
        sm[b, top[4]] = float(edge[(b + 3) % 8])
    out.append(("thresholds", pm, ps, pe, mm, sm.view(B, L, L)))
    return out


def test_rule0_reference_by_hand():
    """L = 3: cells 0..8, mask keeps 0, 1, 2, 4, 5, 8.  Scores: cell 4 = 0.5, cells 1 and 8 tied at 0.25, cell 2 = -1 (below the masked
    zeros at 3, 6, 7 and the valid zero at 0), cell 5 = -0 (tied with them)."""
    pm = np.array([[[0.0, 0.25, -1.0], [9.0, 0.5, -0.0], [9.0, -9.0, 0.25]]], np.float32)
    mm = np.triu(np.ones((1, 3, 3), bool))
    sm = (np.arange(9, dtype=np.float32).reshape(1, 3, 3) + 1) / 10            # 0.1 .. 0.9: cell c holds (c + 1) / 10
    hits, top1, _ = np_rule0(pm, np.ones((1, 3), np.float32), np.ones((1, 3), np.float32), mm, sm)
    # order: 4, 1, 8, then the zeros 0, 3 (5, 6, 7 follow; 2 is last): sm = 0.5, 0.2, 0.9, 0.1, 0.4
    assert top1.tolist() == [np.float32(0.5)]
    assert hits == {"R@1, IoU=0.1": 1.0, "R@1, IoU=0.3": 1.0, "R@1, IoU=0.5": 0.0, "R@1, IoU=0.7": 0.0,
                    "R@5, IoU=0.1": 1.0, "R@5, IoU=0.3": 1.0, "R@5, IoU=0.5": 1.0, "R@5, IoU=0.7": 1.0}
    api = _api()
    ref = api.EpochMeterTorch()
    ref.update(*(torch.from_numpy(x) for x in (pm, np.ones((1, 3), np.float32), np.ones((1, 3), np.float32), mm, sm)))
    assert ref.state[3].item() == float(np.float32(0.5))                       # the restatement's top-1 follows the same tie rule


# ---------------------------------------------------------------- GPU
@functools.lru_cache(maxsize=None)
def torch_lists(L, rows, k, thr):
    """top_moments_torch of the first `rows` family samples at L."""
    return _api().top_moments_torch(*batch(rows, L), k=k, nms_thresh=thr)


@pytest.mark.gpu
@pytest.mark.parametrize("B,L", MATRIX)
def test_layout_matrix_against_python_nms(dev, B, L):
    """Every band layout runs every family (row b is sample b % F) at the five (k, nms_thresh): each row bitwise equal to py_nms's
    list of its family, to the row of the first period, and to top_moments_torch."""
    api = _api()
    assert api._lib.load().smin_top_moments_ws_bytes(B, L, 64) == ws_bytes(B, L)
    host = batch(B, L)
    d = [x.to(dev) for x in host]
    first = torch.arange(B) % F
    rows = min(B, F)
    for k, thr in KT:
        got = {key: v.cpu() for key, v in api.top_moments(*d, k=k, nms_thresh=thr).items()}
        bad = []
        for b in range(rows):
            what = (B, L, layout(B, L)[:2], k, thr, b, NAMES[b])
            print(what, "count", int(got["count"][b]), "want", len(reference(L, b, k, thr)))
            try:
                assert_row(got, b, reference(L, b, k, thr), what)
            except AssertionError:
                bad.append(what)
        assert not bad, bad
        for key in ("idx", "count"):
            same = (got[key] == got[key][first]).reshape(B, -1).all(dim=1)
            assert same.all(), (key, k, thr, (~same).nonzero().flatten().tolist())
        sb = got["score"].view(torch.int32)
        same = (sb == sb[first]).all(dim=1)
        assert same.all(), ("score", k, thr, (~same).nonzero().flatten().tolist())
        want = torch_lists(L, rows, k, thr)
        assert torch.equal(got["count"][:rows], want["count"]) and torch.equal(got["idx"][:rows], want["idx"]), (k, thr)
        assert torch.equal(sb[:rows], want["score"].view(torch.int32)), (k, thr)


def _carry_batch(dev):
    B, L = 74, 96
    host = batch(B, L)
    sm = torch.rand(B, L, L, generator=torch.Generator().manual_seed(11))
    return B, L, host + (sm,), [x.to(dev) for x in host + (sm,)]


@pytest.mark.gpu
def test_compute_ious_carries_the_lists_through(dev):
    """compute_ious(nms_thresh=0.0) on the P = 7 batch: R@n counts formed from py_nms's lists (an empty slot is IoU 0)."""
    api = _api()
    B, L, host, d = _carry_batch(dev)
    n, m = (1, 3, 64), (0.1, 0.5)
    sm = host[4].numpy()
    want = {}
    for n_ in n:
        for m_ in m:
            want[f"R@{n_}, IoU={m_}"] = float(sum(any(sm[b, i, j] > np.float32(m_) for i, j, _ in reference(L, b % F, 64, 0.0)[:n_])
                                                  for b in range(B)))
    got = api.compute_ious(*d, n=n, m=m, nms_thresh=0.0)
    print(got, want)
    assert got == want
    assert len(set(want.values())) > 2                                  # the counts tell the (n, m) pairs apart


@pytest.mark.gpu
def test_epoch_meter_carries_the_lists_through(dev):
    api = _api()
    B, L, host, d = _carry_batch(dev)
    n, m = (1, 3, 64), (0.1, 0.5)
    hip, ref = api.EpochMeter(n=n, m=m, nms_thresh=0.0, device=dev), api.EpochMeterTorch(n=n, m=m, nms_thresh=0.0)
    hip.update(*d)
    ref.update(*host)
    assert torch.equal(hip.state.cpu().view(torch.int64), ref.state.view(torch.int64)), (hip.state.tolist(), ref.state.tolist())
    top1 = 0.0
    for b in range(B):                                                  # and the top-1 sum from py_nms's first kept cell
        i, j, _ = reference(L, b % F, 64, 0.0)[0]
        top1 += float(host[4][b, i, j])
    assert hip.state[0].item() == B and hip.state[3].item() == top1


@pytest.mark.gpu
@pytest.mark.parametrize("B", [1, 9])
@pytest.mark.parametrize("L", [3, 16, 17, 40])
def test_rule0_metric_kernel_against_numpy(dev, L, B):
    """ious_kernel through compute_ious (default n, m) and the epoch meter's reference rule: hits and top-1, on ties, masked zeros
    above negative scores, one thread's insertion with its dropped sixth, all-masked samples and sm exactly at the thresholds."""
    api = _api()
    for name, pm, ps, pe, mm, sm in rule0_inputs(B, L):
        hits, top1, _ = np_rule0(pm.numpy(), ps.numpy(), pe.numpy(), mm.numpy(), sm.numpy())
        d = [x.to(dev) for x in (pm, ps, pe, mm, sm)]
        got = api.compute_ious(*d)
        print(name, L, B, got, hits)
        assert got == hits, (name, L, B)
        meter = api.EpochMeter(device=dev)
        meter.update(*d)
        s = 0.0
        for v in top1.tolist():
            s += v
        want = torch.tensor([float(B), 0.0, 0.0, s] + [hits[key] for key in meter.keys], dtype=torch.float64)
        assert torch.equal(meter.state.cpu().view(torch.int64), want.view(torch.int64)), (name, L, B, meter.state.tolist(), want.tolist())
        ref = api.EpochMeterTorch()
        ref.update(pm, ps, pe, mm, sm)
        assert ref.state[3].item() == s, (name, L, B)                   # the restatement's top-1 stays pinned on these inputs too
