"""Soft-NMS moment retrieval (csrc/soft_nms.hip): smin_top_moments_soft, its span form smin_merge_window_moments_soft, and the metric
entries behind compute_ious(..., nms=) and EpochMeter(..., nms=).

The linear rule is made of correctly rounded fp32 operations, so every device list is compared bit for bit with
`top_moments_soft_torch` / `merge_window_moments_torch(nms="linear")`, which the CPU tests tie to the worked example of
include/smin_hip.h and to `top_moments_torch`.  The gaussian rule goes through the device library's expf, which no host reproduces
bit for bit; it is checked by replaying the device's own picks in fp64 (`replay`).

Dispatch of csrc/soft_nms.hip: a map of L*L <= 12288 cells (L <= 110) is one launch with `cur` in LDS; a larger one takes k + 1
launches over P = min(32, ceil(L*L / 4096)) bands.  L = 110 and L = 111 sit on the two sides of that boundary; the banded path has
P >= 4 everywhere (there is no P = 1 case), and P only saturates at 32 from L = 357 on without a change of code path.

Out of scope, as the header says: NaN and +-inf at valid cells.  NaN and inf at masked cells are in scope (`nan_masked`)."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from tests import helpers as H
from tests.support.compare import same_tensor as same
from tests.support.device import dev  # noqa: F401  (the module's device fixture)
from tests.support.device import vml as V
from tests.support.guards import BAND, WORD_SENTINEL, bands_intact, banded
from tests.support.references import merge_frame_edges

LDS_CELLS, BAND_CELLS, MAX_BANDS = 12288, 4096, 32      # csrc/soft_nms.hip
U = 2.0 ** -24                                           # half an ulp of fp32, relative: one correctly rounded operation
ULP_EXPF = 1                                             # HIP's math API documents expf with a maximum error of 1 ulp
TINY = 2.0 ** -149                                       # the smallest fp32 subnormal: a product that lands there rounds absolutely

# (B, L, k); the per-sample valid lengths of a shape come from `lengths`
SHAPES = [(3, 1, 4), (3, 8, 8), (2, 33, 8), (2, 64, 16), (1, 96, 64), (2, 110, 4), (2, 111, 4)]
FIXED_LENGTHS = {(3, 1, 4): [1, 1, 0], (3, 8, 8): [8, 3, 0]}      # full; fewer valid cells than k (6 < 8); all masked
SEED = 11


def lengths(shape):
    """First sample full length, the others random (fixed for the two shapes that need a short and an all-masked sample)."""
    B, L, _ = shape
    if shape in FIXED_LENGTHS:
        return FIXED_LENGTHS[shape]
    g = torch.Generator().manual_seed(SEED + L)
    return [L] + [int(torch.randint(1, L + 1, (1,), generator=g)) for _ in range(B - 1)]


def mask_of(shape):
    B, L, _ = shape
    ok = torch.arange(L).unsqueeze(0) < torch.tensor(lengths(shape)).unsqueeze(1)          # (B, L)
    return torch.triu(torch.ones(L, L, dtype=torch.bool)).unsqueeze(0) & ok.unsqueeze(2) & ok.unsqueeze(1)


# ---------------------------------------------------------------- score families (the style of tests/test_moment_selection.py)
def fam_uniform(B, L, g, mm):
    return torch.rand(B, L, L, generator=g), torch.rand(B, L, generator=g), torch.rand(B, L, generator=g)


def fam_signed(B, L, g, mm):
    pm, ps, pe = fam_uniform(B, L, g, mm)
    return 2 * pm - 1, ps, pe


def fam_equal(B, L, g, mm):
    """every valid cell 0.5: the first pick goes by index, after it the decay alone decides, ties by index again"""
    return torch.full((B, L, L), 0.5), torch.ones(B, L), torch.ones(B, L)


def fam_subnormal(B, L, g, mm):
    return torch.rand(B, L, L, generator=g) * 1e-30, torch.full((B, L), 1e-16), torch.ones(B, L)


def fam_nan_masked(B, L, g, mm):
    pm, ps, pe = fam_uniform(B, L, g, mm)
    junk = torch.tensor([float("nan"), float("inf"), float("-inf")])
    off = (~mm).flatten().nonzero().flatten()
    pm.view(-1)[off] = junk[torch.arange(off.numel()) % 3]
    return pm, ps, pe


FAMILIES = [fam_uniform, fam_signed, fam_equal, fam_subnormal, fam_nan_masked]
NAMES = [f.__name__[4:] for f in FAMILIES]


@functools.lru_cache(maxsize=None)
def inputs(shape, q):
    """(pm, ps, pe, mm) of family q at `shape`, on the CPU.  Shared, never written."""
    B, L, _ = shape
    mm = mask_of(shape)
    pm, ps, pe = FAMILIES[q](B, L, torch.Generator().manual_seed(1000 * SEED + 10 * q + L), mm)
    return pm.contiguous(), ps.contiguous(), pe.contiguous(), mm.contiguous()


@functools.lru_cache(maxsize=None)
def linear_reference(shape, q, thr):
    return V().top_moments_soft_torch(*inputs(shape, q), k=shape[2], nms_thresh=thr, nms="linear")


def on(dev, xs):
    return [x.to(dev) for x in xs]


def same_lists(got, want, keys=("idx", "score", "raw_score", "count"), what=""):
    for key in keys:
        assert same(got[key].cpu(), want[key].cpu()), (what, key)


def worked_example():
    L = 4
    pm = torch.zeros(1, L, L)
    pm[0, 0, 3], pm[0, 0, 2], pm[0, 3, 3] = 1.0, 0.9, 0.5
    return pm, torch.ones(1, L), torch.ones(1, L), torch.triu(torch.ones(L, L, dtype=torch.bool)).unsqueeze(0)


# ---------------------------------------------------------------- the fp64 replay of the gaussian rule
def replay(s0, valid, iou64, picks, scores, sigma, iou_err):
    """Replays one sample's device picks in fp64 and checks each of them; returns (steps, steps with a runner-up inside the band).

    `s0` (n,) the fp32 start scores, `valid` (n,) bool, `iou64(c)` the (n,) IoUs with candidate c in fp64, `picks` / `scores` the
    device's list.  At step r the device's earlier picks p_0 .. p_{r-1} are taken as given, so every remaining candidate has had r
    decays:  cur64(c) = s0(c) * prod_t exp(-iou64(c, p_t)^2 / sigma), unrounded.

    Tolerance, derived and not tuned.  With u = 2^-24 (one correctly rounded fp32 operation), one decay factor on the device carries
      * the IoU: `iou_err` roundings (cells: the one division, 1; spans: the two fp32 subtractions and the division, 3) -> iou_err * u;
      * its square: twice that, plus the product's rounding                                            -> (2 * iou_err + 1) * u;
      * the division by sigma: one more rounding of the argument x = iou^2 / sigma                     -> (2 * iou_err + 2) * u;
        a relative error d of x moves exp(-x) by x * d <= d / sigma (iou <= 1)                          -> (2 * iou_err + 2) / sigma * u;
      * expf itself: ULP_EXPF ulp = 2 * ULP_EXPF * u relative;
      * the product cur * w: u, or, where it lands among the subnormals, TINY absolute.
    The per-factor errors add up over the r decays applied (first order):
      tol_r = r * ((2 * iou_err + 2) / sigma + 2 * ULP_EXPF + 1) * 2^-24,  band_r = tol_r * |max| + r * TINY.
    Checks at every step: the pick is a valid, unpicked candidate; its cur64 >= max cur64 - band_r; the returned score is within band_r
    of its cur64.  Outside the band the pick therefore IS the fp64 argmax; the caller asserts that the band is almost never populated."""
    cur = s0.double().clone()
    alive = valid.clone()
    steps = close = 0
    per_factor = ((2 * iou_err + 2) / sigma + 2 * ULP_EXPF + 1) * U
    for r, (c, sc) in enumerate(zip(picks, scores)):
        assert 0 <= c < cur.numel() and bool(alive[c]), (r, c)
        mx = float(cur[alive].max())
        band = r * per_factor * abs(mx) + r * TINY
        assert float(cur[c]) >= mx - band, (r, c, float(cur[c]), mx, band)
        assert abs(float(sc) - float(cur[c])) <= band, (r, c, float(sc), float(cur[c]), band)
        alive[c] = False
        steps += 1
        close += int(bool(alive.any()) and float(cur[alive].max()) >= mx - band)
        x = iou64(c)
        cur = torch.where(alive, cur * torch.exp(-(x * x) / sigma), cur)
    return steps, close


def cell_iou64(L):
    cells = torch.arange(L * L)
    ci, cj = cells // L, cells % L

    def f(c):
        inter = (torch.minimum(cj, cj[c]) + 1 - torch.maximum(ci, ci[c])).clamp_min(0)
        return inter.double() / (torch.maximum(cj, cj[c]) + 1 - torch.minimum(ci, ci[c])).double()
    return f


def start_scores(pm, ps, pe):
    M = V().moments
    s = M._mul32(M._mul32(pm, M._sqrt32(ps).unsqueeze(2)), M._sqrt32(pe).unsqueeze(1))
    return torch.where(s == 0, torch.zeros_like(s), s)


def replay_top(r, pm, ps, pe, mm, k, sigma):
    """`replay` over every sample of a soft top_moments result (CPU tensors); also the list's shape: count, the empty tail, raw_score."""
    B, L = pm.shape[0], pm.shape[1]
    s0 = start_scores(pm, ps, pe).reshape(B, -1)
    valid = mm.reshape(B, -1)
    s0 = torch.where(valid, s0, torch.zeros_like(s0))
    steps = close = 0
    for b in range(B):
        n = int(r["count"][b])
        assert n == min(k, int(valid[b].sum())), b
        flat = (r["idx"][b, :n, 0] * L + r["idx"][b, :n, 1]).tolist()
        assert (r["idx"][b, n:] == -1).all() and (r["score"][b, n:] == 0).all() and (r["raw_score"][b, n:] == 0).all(), b
        assert same(r["raw_score"][b, :n], s0[b, flat]), b
        a, c = replay(s0[b], valid[b], cell_iou64(L), flat, r["score"][b, :n].tolist(), sigma, iou_err=1)
        steps, close = steps + a, close + c
    return steps, close


# ---------------------------------------------------------------- CPU
def test_restatement_reproduces_the_worked_example():
    api = V()
    pm, ps, pe, mm = worked_example()
    r = api.top_moments_soft_torch(pm, ps, pe, mm, k=3, nms_thresh=0.5, nms="linear")
    f = np.float32
    assert r["idx"][0].tolist() == [[0, 3], [3, 3], [0, 2]] and int(r["count"][0]) == 3
    assert r["score"][0].numpy().tobytes() == np.array([f(1.0), f(0.5), f(0.9) * f(0.25)], np.float32).tobytes()
    assert r["raw_score"][0].numpy().tobytes() == np.array([1.0, 0.5, 0.9], np.float32).tobytes()
    assert api.top_moments_torch(pm, ps, pe, mm, k=3, nms_thresh=1.0)["idx"][0].tolist() == [[0, 3], [0, 2], [3, 3]]     # plain top-k
    assert api.top_moments_torch(pm, ps, pe, mm, k=3, nms_thresh=0.5)["idx"][0].tolist() == [[0, 3], [3, 3], [0, 0]]     # hard NMS


@pytest.mark.parametrize("q", range(len(FAMILIES)), ids=NAMES)
def test_restatement_without_decay_is_plain_topk(q):
    api = V()
    for shape in ((3, 8, 8), (2, 33, 8)):
        pm, ps, pe, mm = inputs(shape, q)
        want = api.top_moments_torch(pm, ps, pe, mm, k=shape[2], nms_thresh=1.0)
        for kw in (dict(nms="linear", nms_thresh=1.0), dict(nms="linear", nms_thresh=2.5), dict(nms="gaussian", sigma=float("inf"))):
            r = api.top_moments_soft_torch(pm, ps, pe, mm, k=shape[2], **kw)
            same_lists(r, want, keys=("idx", "score", "count"), what=(shape, kw))
            assert same(r["raw_score"], r["score"])


def test_all_equal_scores_go_by_decay_then_index():
    """every valid cell 0.5 at L = 8, linear at 0.0: (0, 0) first by index; every cell overlapping it is decayed, so the next pick is the
    first cell with no overlap, (1, 1), and so on down the diagonal"""
    pm, ps, pe, mm = inputs((3, 8, 8), NAMES.index("equal"))
    r = linear_reference((3, 8, 8), NAMES.index("equal"), 0.0)
    assert r["idx"][0].tolist() == [[d, d] for d in range(8)] and (r["score"][0] == 0.5).all()


def test_min_score_truncates_the_restated_list():
    api = V()
    pm, ps, pe, mm = worked_example()
    r = api.top_moments_soft_torch(pm, ps, pe, mm, k=3, nms_thresh=0.5, nms="linear", min_score=0.3)
    assert int(r["count"][0]) == 2 and r["idx"][0, 2].tolist() == [-1, -1] and float(r["score"][0, 2]) == 0 and float(r["raw_score"][0, 2]) == 0


def test_argument_refusals_on_the_host():
    api = V()
    pm, ps, pe, mm = worked_example()
    for kw in (dict(nms="soft"), dict(nms="gaussian", sigma=0.0), dict(nms="gaussian", sigma=-1.0), dict(nms="gaussian", sigma=float("nan")),
               dict(nms="linear", min_score=float("nan"))):
        with pytest.raises(ValueError):
            api.top_moments_soft_torch(pm, ps, pe, mm, k=3, **kw)
        with pytest.raises(ValueError):                                                  # the check the device entry points run first
            api.moments.soft_rule("top_moments", kw["nms"], 0.5, kw.get("sigma", 0.5), kw.get("min_score"))
    assert api.moments.soft_rule("top_moments", "hard", 0.5, -1.0, None) is None          # the hard rule reads neither
    assert api.moments.soft_rule("top_moments", "gaussian", 0.5, float("inf"), None) == (2, 0.5, float("inf"), float("-inf"))
    with pytest.raises(ValueError):
        api.top_moments_soft_torch(pm, ps, pe, mm, k=3, nms="hard")
    cand = [torch.zeros(1, 2, 2, dtype=torch.int64), torch.ones(1, 2), torch.tensor([2], dtype=torch.int32), torch.zeros(1, dtype=torch.int64),
            torch.tensor([8], dtype=torch.int32), torch.tensor([0, 1])]
    with pytest.raises(ValueError):
        api.merge_window_moments_torch(*cand, 8, 4, k=2, nms="gaussian", sigma=0.0)
    with pytest.raises(ValueError):
        api.merge_window_moments_torch(*cand, 8, 4, k=2, nms="median")
    sm = torch.rand(1, 4, 4)
    with pytest.raises(ValueError):
        api.compute_ious_torch(pm, ps, pe, mm, sm, nms="linear")                         # the soft rules rank like the nms_thresh rule
    with pytest.raises(ValueError):
        api.compute_ious_torch(pm, ps, pe, mm, sm, nms_thresh=0.5, nms="gaussian", sigma=0.0)
    with pytest.raises(ValueError):
        api.EpochMeterTorch(nms="linear")
    with pytest.raises(ValueError):
        api.EpochMeterTorch(nms_thresh=0.5, nms="gaussian", sigma=-2.0)
    with pytest.raises(ValueError):
        api.EpochMeterTorch(nms_thresh=0.5, nms="other")


def ws_model(B, L):
    """csrc/soft_nms.hip ws_layout"""
    n = L * L
    if n <= LDS_CELLS:
        return 256
    P = min(MAX_BANDS, H.cdiv(n, BAND_CELLS))
    a256 = lambda x: (x + 255) & ~255
    return a256(B * n * 4) + 2 * a256(B * P * 8)


def test_workspace_query_is_the_layout_model_and_new_symbols_are_exported():
    api = V()
    lib = api._lib.load()
    for name, nargs in (("smin_top_moments_soft_ws_bytes", 3), ("smin_top_moments_soft", 18), ("smin_merge_window_moments_soft", 23),
                        ("smin_compute_ious_soft_ws_bytes", 5), ("smin_compute_ious_soft", 19), ("smin_epoch_meter_soft_ws_bytes", 5),
                        ("smin_epoch_meter_update_soft", 20)):
        assert len(api._lib.SIGNATURES[name]) == nargs and hasattr(lib, name), name
    assert lib.smin_abi_version() == 2
    for B, L in ((1, 1), (3, 8), (2, 110), (2, 111), (1, 356), (16, 357), (16, 512), (65535, 8)):
        assert lib.smin_top_moments_soft_ws_bytes(B, L, 5) == ws_model(B, L), (B, L)
    for B, L, k in ((0, 8, 5), (65536, 8, 5), (2, 0, 5), (2, 46341, 5), (2, 8, 0), (2, 8, 65)):
        assert lib.smin_top_moments_soft_ws_bytes(B, L, k) == 0, (B, L, k)
    assert lib.smin_compute_ious_soft_ws_bytes(5, 16, 5, 2, 4) > ws_model(5, 16) and lib.smin_compute_ious_soft_ws_bytes(5, 16, 5, 0, 4) == 0
    assert lib.smin_epoch_meter_soft_ws_bytes(5, 16, 5, 2, 4) > lib.smin_compute_ious_soft_ws_bytes(5, 16, 5, 2, 4)
    assert lib.smin_epoch_meter_soft_ws_bytes(5, 16, 65, 2, 4) == 0


def test_uniform_replay_band_is_empty_on_the_restatement():
    """The band of `replay` must not be what makes the gaussian check pass: on the restatement's own (fp64) lists at most 5 % of a uniform
    case's steps have a runner-up inside it (the device test's criterion; here 1 step of the 64 at L = 96, none elsewhere)."""
    api = V()
    for shape in SHAPES[:5]:
        pm, ps, pe, mm = inputs(shape, 0)
        for sigma in (0.25, 0.5):
            r = api.top_moments_soft_torch(pm, ps, pe, mm, k=shape[2], nms="gaussian", sigma=sigma)
            steps, close = replay_top(r, pm, ps, pe, mm, shape[2], sigma)
            assert steps >= 2 and close <= 0.05 * steps, (shape, sigma, steps, close)


# ---------------------------------------------------------------- GPU
@pytest.mark.gpu
@pytest.mark.parametrize("q", range(len(FAMILIES)), ids=NAMES)
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_linear_equals_the_restatement_bit_for_bit(dev, shape, q):
    api = V()
    args = on(dev, inputs(shape, q))
    for thr in (0.0, 0.5):
        got = api.top_moments(*args, k=shape[2], nms_thresh=thr, nms="linear")
        same_lists(got, linear_reference(shape, q, thr), what=(shape, NAMES[q], thr))
        assert got["idx"].dtype == torch.int64 and got["count"].dtype == torch.int32


@pytest.mark.gpu
@pytest.mark.parametrize("sigma", (0.25, 0.5))
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_gaussian_picks_replay_in_fp64(dev, shape, sigma):
    """Every family through `replay` (its docstring derives the tolerance).  On the uniform family the band must be all but empty -- at
    most 5 % of the (sample, step) pairs may have a runner-up inside it -- so that the check pins the pick to the fp64 argmax; and the
    picked scores of non-negative inputs never increase (every weight is <= 1 and the fp32 product is monotone)."""
    api = V()
    for q, name in enumerate(NAMES):
        pm, ps, pe, mm = inputs(shape, q)
        got = {key: v.cpu() for key, v in api.top_moments(*on(dev, (pm, ps, pe, mm)), k=shape[2], nms="gaussian", sigma=sigma).items()}
        steps, close = replay_top(got, pm, ps, pe, mm, shape[2], sigma)
        print(f"{shape} {name} sigma={sigma}: {steps} steps, {close} with a runner-up inside the band")
        if name == "uniform":
            assert steps >= 2 and close <= 0.05 * steps, (shape, steps, close)
        if name != "signed":
            for b in range(shape[0]):
                s = got["score"][b, :int(got["count"][b])]
                assert bool((s[1:] <= s[:-1]).all()), (shape, name, b)


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(3, 8, 8), (2, 33, 8), (2, 111, 4)], ids=str)
def test_identities_on_the_device(dev, shape):
    api = V()
    for q in range(len(FAMILIES)):
        args = on(dev, inputs(shape, q))
        plain = api.top_moments(*args, k=shape[2], nms_thresh=1.0)
        for kw in (dict(nms="linear", nms_thresh=1.0), dict(nms="gaussian", sigma=float("inf"))):
            r = api.top_moments(*args, k=shape[2], **kw)
            same_lists(r, plain, keys=("idx", "score", "count"), what=(shape, NAMES[q], kw))
            assert same(r["raw_score"], r["score"])
        a, b = api.top_moments(*args, k=shape[2], nms_thresh=0.5), api.top_moments(*args, k=shape[2], nms_thresh=0.5, nms="hard")
        assert sorted(a) == sorted(b) == ["count", "idx", "score"]
        same_lists(a, b, keys=("idx", "score", "count"))


@pytest.mark.gpu
def test_worked_example_on_the_device(dev):
    api = V()
    args = worked_example()
    same_lists(api.top_moments(*on(dev, args), k=3, nms_thresh=0.5, nms="linear"),
               api.top_moments_soft_torch(*args, k=3, nms_thresh=0.5, nms="linear"))


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(2, 33, 8), (2, 111, 4)], ids=str)
def test_min_score_truncates_the_list(dev, shape):
    """a floor between the second and the third picked score: two picks, empty slots behind, on both dispatch paths"""
    api = V()
    full = linear_reference(shape, 0, 0.5)
    for b in range(shape[0]):                                                            # one floor per sample: a call per sample
        args = [x[b:b + 1] for x in inputs(shape, 0)]
        s1, s2 = float(full["score"][b, 1]), float(full["score"][b, 2])
        floor = 0.5 * (s1 + s2)
        assert s1 > floor > s2
        got = api.top_moments(*on(dev, args), k=shape[2], nms_thresh=0.5, nms="linear", min_score=floor)
        same_lists(got, api.top_moments_soft_torch(*args, k=shape[2], nms_thresh=0.5, nms="linear", min_score=floor))
        assert got["count"].tolist() == [2]
        assert (got["idx"][:, 2:] == -1).all() and (got["score"][:, 2:] == 0).all() and (got["raw_score"][:, 2:] == 0).all()
        assert same(got["score"][:, :2].cpu(), full["score"][b:b + 1, :2])


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(2, 64, 16), (2, 111, 4)], ids=str)
def test_two_calls_give_identical_bytes(dev, shape):
    api = V()
    args = on(dev, inputs(shape, 1))
    for kw in (dict(nms="linear", nms_thresh=0.0), dict(nms="gaussian", sigma=0.25)):
        same_lists(api.top_moments(*args, k=shape[2], **kw), api.top_moments(*args, k=shape[2], **kw), what=kw)


@pytest.mark.gpu
def test_graph_capture_follows_new_inputs(dev):
    api = V()
    shape = (2, 33, 8)
    pm, ps, pe, mm = (x.clone() for x in on(dev, inputs(shape, 0)))
    api.top_moments(pm, ps, pe, mm, k=8, nms_thresh=0.5, nms="linear")                   # library loaded, allocator warm
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = api.top_moments(pm, ps, pe, mm, k=8, nms_thresh=0.5, nms="linear")
    for x in out.values():
        x.zero_()
    g.replay()
    torch.cuda.synchronize()
    same_lists(out, linear_reference(shape, 0, 0.5))
    new = inputs(shape, 1)                                                               # the signed family into the captured buffers
    assert bool((new[3] == inputs(shape, 0)[3]).all())
    for dst, src in zip((pm, ps, pe, mm), new):
        dst.copy_(src.to(dev))
    g.replay()
    torch.cuda.synchronize()
    same_lists(out, api.top_moments(*on(dev, new), k=8, nms_thresh=0.5, nms="linear"))
    same_lists(out, linear_reference(shape, 1, 0.5))


# ---------------------------------------------------------------- metric entries
def metric_batch(seed=2):
    g = torch.Generator().manual_seed(seed)
    B, L = 5, 16
    mm = torch.triu(torch.ones(L, L, dtype=torch.bool)).expand(B, L, L).clone()
    mm[1, :, 9:] = False
    mm[3] = False                                                                        # a sample that keeps nothing
    return torch.rand(B, L, L, generator=g), torch.rand(B, L, generator=g), torch.rand(B, L, generator=g), mm, torch.rand(B, L, L, generator=g)


@pytest.mark.gpu
def test_compute_ious_and_meter_with_the_linear_rule(dev):
    api = V()
    n, m = (1, 5), (0.1, 0.3, 0.5, 0.7)
    a, b = metric_batch(2), metric_batch(3)
    for kw in (dict(nms="linear"), dict(nms="hard")):
        assert api.compute_ious(*on(dev, a), n=n, m=m, nms_thresh=0.5, **kw) == api.compute_ious_torch(*a, n=n, m=m, nms_thresh=0.5, **kw), kw
    soft = api.compute_ious_torch(*a, n=(5,), m=m, nms_thresh=0.0, nms="linear")
    hard = api.compute_ious_torch(*a, n=(5,), m=m, nms_thresh=0.0)
    assert soft != hard                                                                  # the rule is what is being measured
    hip = api.EpochMeter(n=n, m=m, nms_thresh=0.5, nms="linear", device=dev)
    ref = api.EpochMeterTorch(n=n, m=m, nms_thresh=0.5, nms="linear")
    for batch in (a, b):                                                                 # the second update accumulates
        hip.update(*on(dev, batch))
        ref.update(*batch)
        assert torch.equal(hip.state.cpu(), ref.state), (hip.state, ref.state)
    assert hip.result() == ref.result() and hip.result()["num_samples"] == 10


# ---------------------------------------------------------------- C ABI
def _vp(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def int_banded(shape, dev, dtype):
    n = int(np.prod(shape))
    sent = WORD_SENTINEL if dtype == torch.int32 else (WORD_SENTINEL << 32) | WORD_SENTINEL
    buf = torch.full((n + 2 * BAND,), sent, dtype=dtype, device=dev)
    buf[BAND:BAND + n] = -7
    return buf, buf[BAND:BAND + n].view(*shape), sent


def int_bands_intact(buf, sent):
    return bool(buf[:BAND].eq(sent).all()) and bool(buf[-BAND:].eq(sent).all())


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(3, 8, 8), (2, 111, 4)], ids=str)
def test_c_abi_workspace_guards_and_refusals(dev, shape):
    """The exact workspace is accepted, one byte less refused; every refusal is a nonzero code from a host-side check -- the outputs keep
    their fill, so nothing was launched --; an accepted call writes inside its outputs only."""
    api = V()
    lib = api._lib.load()
    B, L, k = shape
    pm, ps, pe, mm = on(dev, inputs(shape, 0))
    mm = mm.to(torch.uint8)
    need = lib.smin_top_moments_soft_ws_bytes(B, L, k)
    assert need == ws_model(B, L)
    ws = torch.zeros(need, dtype=torch.uint8, device=dev)
    ibuf, idx, isent = int_banded((B, k, 2), dev, torch.int64)
    cbuf, count, csent = int_banded((B,), dev, torch.int32)
    sbuf, score = banded((B, k), dev)
    rbuf, raw = banded((B, k), dev)
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def call(method=1, sigma=0.5, ws_bytes=need, **null):
        p = dict(pm=pm, ps=ps, pe=pe, mm=mm, idx=idx, score=score, raw=raw, count=count, ws=ws)
        p.update(null)
        return lib.smin_top_moments_soft(st, _vp(p["pm"]), _vp(p["ps"]), _vp(p["pe"]), _vp(p["mm"]), B, L, k, method, 0.5, sigma, float("-inf"),
                                         _vp(p["idx"]), _vp(p["score"]), _vp(p["raw"]), _vp(p["count"]), _vp(p["ws"]), ws_bytes)

    bad = [dict(method=0), dict(method=3), dict(method=-1), dict(method=2, sigma=0.0), dict(method=2, sigma=-0.5), dict(method=2, sigma=float("nan")),
           dict(ws_bytes=need - 1), dict(ws_bytes=0)]
    bad += [{name: None} for name in ("pm", "ps", "pe", "mm", "idx", "score", "raw", "count", "ws")]
    for kw in bad:
        assert call(**kw) != 0, kw
    torch.cuda.synchronize()
    assert bool(torch.isnan(score).all()) and bool(torch.isnan(raw).all()) and bool((idx == -7).all()) and bool((count == -7).all())
    for method, sigma in ((1, 0.5), (1, float("nan")), (2, 0.5), (2, float("inf"))):          # linear does not read sigma
        assert call(method=method, sigma=sigma) == 0, (method, sigma)
    torch.cuda.synchronize()
    assert bands_intact(sbuf) and bands_intact(rbuf) and int_bands_intact(ibuf, isent) and int_bands_intact(cbuf, csent)
    assert call(method=1) == 0
    torch.cuda.synchronize()
    same_lists(dict(idx=idx, score=score, raw_score=raw, count=count), linear_reference(shape, 0, 0.5))


@pytest.mark.gpu
def test_c_abi_metric_and_merge_refusals(dev):
    api = V()
    lib = api._lib.load()
    B, L, k = 5, 16, 5
    pm, ps, pe, mm, sm = on(dev, metric_batch())
    mm = mm.to(torch.uint8)
    nl, ml = (ctypes.c_int * 2)(1, 5), (ctypes.c_float * 4)(0.1, 0.3, 0.5, 0.7)
    nlp, mlp = ctypes.cast(nl, ctypes.c_void_p), ctypes.cast(ml, ctypes.c_void_p)
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    need = lib.smin_compute_ious_soft_ws_bytes(B, L, k, 2, 4)
    ws = torch.zeros(need + 4096, dtype=torch.uint8, device=dev)
    cbuf, counts = banded((8,), dev)

    def ious(method=1, sigma=0.5, ws_bytes=need, **null):
        p = dict(pm=pm, sm=sm, counts=counts, ws=ws)
        p.update(null)
        return lib.smin_compute_ious_soft(st, _vp(p["pm"]), _vp(ps), _vp(pe), _vp(mm), _vp(p["sm"]), B, L, k, method, 0.5, sigma, nlp, 2, mlp, 4,
                                          _vp(p["counts"]), _vp(p["ws"]), ws_bytes)
    for kw in (dict(method=0), dict(method=3), dict(method=2, sigma=0.0), dict(method=2, sigma=float("nan")), dict(ws_bytes=need - 1),
               dict(pm=None), dict(sm=None), dict(counts=None), dict(ws=None)):
        assert ious(**kw) != 0, kw
    torch.cuda.synchronize()
    assert bool(torch.isnan(counts).all())
    assert ious() == 0
    torch.cuda.synchronize()
    assert bands_intact(cbuf) and not bool(torch.isnan(counts).any())

    mneed = lib.smin_epoch_meter_soft_ws_bytes(B, L, k, 2, 4)
    acc = torch.zeros(4 + 8, dtype=torch.float64, device=dev)

    def meter(method=1, sigma=0.5, ws_bytes=mneed, **null):
        p = dict(pm=pm, acc=acc, ws=ws)
        p.update(null)
        return lib.smin_epoch_meter_update_soft(st, _vp(p["pm"]), _vp(ps), _vp(pe), _vp(mm), _vp(sm), B, L, k, method, 0.5, sigma, nlp, 2, mlp, 4, None,
                                                _vp(p["acc"]), _vp(p["ws"]), ws_bytes)
    assert mneed <= need + 4096
    for kw in (dict(method=0), dict(method=2, sigma=-1.0), dict(ws_bytes=mneed - 1), dict(pm=None), dict(acc=None), dict(ws=None)):
        assert meter(**kw) != 0, kw
    torch.cuda.synchronize()
    assert bool((acc == 0).all())
    assert meter() == 0
    torch.cuda.synchronize()
    assert float(acc[0]) == B


# ---------------------------------------------------------------- span form: the merge across the windows of long videos
WT, WL = 16, 8                                           # T, L of the window tests


@functools.lru_cache(maxsize=None)
def window_candidates(seed=5):
    """Three pairs with 0, 1 and 7 windows (k_window = 4): windows of 16 rows every 8 rows, so neighbours overlap by half; distinct cells
    inside a window, uniform scores, and count < k_window in some windows."""
    g = torch.Generator().manual_seed(seed)
    G, kw = 8, 4
    cells = torch.triu(torch.ones(WL, WL)).flatten().nonzero().flatten()
    flat = torch.stack([cells[torch.randperm(cells.numel(), generator=g)[:kw]] for _ in range(G)])
    idx = torch.stack([flat // WL, flat % WL], -1)
    score = torch.rand(G, kw, generator=g)
    count = torch.tensor([4, 4, 2, 4, 1, 3, 4, 4], dtype=torch.int32)
    slot = torch.arange(kw).unsqueeze(0) >= count.unsqueeze(1)
    idx[slot] = -1
    score[slot] = 0
    start = torch.tensor([0, 0, 8, 16, 24, 32, 40, 44], dtype=torch.int64)
    lens = torch.tensor([11, 16, 16, 16, 16, 16, 16, 12], dtype=torch.int32)
    return idx, score, count, start, lens, torch.tensor([0, 0, 1, 8], dtype=torch.int64)


MERGE_KEYS = ("span", "score", "raw_score", "window", "cell", "count")


def test_soft_merge_restatement_without_decay_is_the_hard_merge_without_suppression():
    api = V()
    cand = window_candidates()
    want = api.merge_window_moments_torch(*cand, WT, WL, k=6, nms_thresh=1.0)
    for kw in (dict(nms="linear", nms_thresh=1.0), dict(nms="gaussian", sigma=float("inf"))):
        r = api.merge_window_moments_torch(*cand, WT, WL, k=6, **kw)
        for key in ("span", "score", "window", "cell", "count"):
            assert same(r[key], want[key]), (kw, key)
        assert same(r["raw_score"], r["score"])
    assert want["count"].tolist() == [0, 4, 6]
    soft = api.merge_window_moments_torch(*cand, WT, WL, k=6, nms_thresh=0.0, nms="linear")
    assert not same(soft["window"], want["window"]) or not same(soft["cell"], want["cell"])       # the decay reorders these candidates


@pytest.mark.gpu
def test_span_form_equals_its_restatement(dev):
    api = V()
    cand = window_candidates()
    for thr in (0.0, 0.5):
        got = api.merge_window_moments(*on(dev, cand), WT, WL, k=6, nms_thresh=thr, nms="linear")
        want = api.merge_window_moments_torch(*cand, WT, WL, k=6, nms_thresh=thr, nms="linear")
        for key in MERGE_KEYS:
            assert same(got[key].cpu(), want[key]), (thr, key)
    floor = 0.5 * float(want["score"][2, 1] + want["score"][2, 2])
    got = api.merge_window_moments(*on(dev, cand), WT, WL, k=6, nms_thresh=0.5, nms="linear", min_score=floor)
    want = api.merge_window_moments_torch(*cand, WT, WL, k=6, nms_thresh=0.5, nms="linear", min_score=floor)
    for key in MERGE_KEYS:
        assert same(got[key].cpu(), want[key]), key
    assert int(got["count"][2]) == 2 and int(got["count"][0]) == 0
    hard = api.merge_window_moments(*on(dev, cand), WT, WL, k=6, nms_thresh=0.5)
    assert sorted(hard) == ["cell", "count", "score", "span", "window"]
    for key in hard:
        assert same(hard[key], api.merge_window_moments(*on(dev, cand), WT, WL, k=6, nms_thresh=0.5, nms="hard")[key]), key


@pytest.mark.gpu
def test_span_form_at_the_frame_edges(dev):
    """The hard merge's frame-edge case (test_window_localize) under the linear rule: pair_ptr outside [0, G], a pair without a window,
    a window without a moment, tied scores and a -0.0.  Every field bit for bit, the NaN of the empty spans included."""
    api = V()
    cand = merge_frame_edges()
    got = api.merge_window_moments(*on(dev, cand), 8, 8, k=3, nms_thresh=0.5, nms="linear")
    want = api.merge_window_moments_torch(*cand, 8, 8, k=3, nms_thresh=0.5, nms="linear")
    for key in MERGE_KEYS:
        assert same(got[key].cpu(), want[key]), key
    assert want["count"].tolist() == [2, 0, 3] and torch.equal(want["span"][1].view(torch.int32), torch.full((3, 2), 0x7FC00000, dtype=torch.int32))


@pytest.mark.gpu
@pytest.mark.parametrize("sigma", (0.25, 0.5))
def test_span_form_gaussian_replays_in_fp64(dev, sigma):
    """`replay` with the span IoU: the spans are the restated fp32 ones (bit for bit the kernel's), their IoU in fp64 from those; the
    device forms it with two fp32 subtractions and a division, hence iou_err = 3."""
    api = V()
    idx, score, count, start, lens, pair_ptr = window_candidates()
    got = {key: v.cpu() for key, v in api.merge_window_moments(*on(dev, window_candidates()), WT, WL, k=6, nms="gaussian", sigma=sigma).items()}
    G, kw = score.shape
    st, en = api.moments.window_spans(idx, start.unsqueeze(1), lens.unsqueeze(1), WT, WL)
    valid = torch.arange(kw).unsqueeze(0) < count.unsqueeze(1)
    pp = pair_ptr.tolist()
    steps = close = 0
    for b in range(3):
        q = slice(pp[b] * kw, pp[b + 1] * kw)
        s, e, ok = st.reshape(-1)[q].double(), en.reshape(-1)[q].double(), valid.reshape(-1)[q]
        n = int(got["count"][b])
        assert n == min(6, int(ok.sum())), b
        picks = (got["window"][b, :n] * kw).tolist()
        for r in range(n):                                                               # the slot of a pick: by its cell within its window
            w = int(got["window"][b, r]) + pp[b]
            slot = [x for x in range(int(count[w])) if idx[w, x].tolist() == got["cell"][b, r].tolist()]
            assert len(slot) == 1, (b, r)
            picks[r] += slot[0]
            assert same(got["raw_score"][b, r], score[w, slot[0]]) and same(got["span"][b, r], torch.stack([st[w, slot[0]], en[w, slot[0]]]))
        assert torch.isnan(got["span"][b, n:]).all() and (got["window"][b, n:] == -1).all() and (got["score"][b, n:] == 0).all()

        def iou64(c):
            inter = (torch.minimum(e, e[c]) - torch.maximum(s, s[c])).clamp_min(0)
            return inter / (torch.maximum(e, e[c]) - torch.minimum(s, s[c]))
        a, c = replay(score.reshape(-1)[q], ok, iou64, picks, got["score"][b, :n].tolist(), sigma, iou_err=3)
        steps, close = steps + a, close + c
    assert steps == 10 and close <= 0.05 * steps, (steps, close)


# ---------------------------------------------------------------- SMIN.localize / localize_windows
TINY_MODEL = (16, 8, 4, 64, 32, 2, 48, 7, 32)            # T, L, C, D, dl, layers, Din, Nq, H


def _model(shape, dev, gain=1.2):
    from oracle import smin_oracle as O                  # test infrastructure: the formula weights only
    import models
    T, L, C, D, dl, layers, Din, Nq, Hh = shape
    m = models.SMIN(T, L, C, D, dl, layers, Din, Nq, Hh, dev)
    m.load_state_dict(O.formula_state_dict(H.smin_shapes(T, L, C, D, dl, layers, Din, Nq, Hh), gain=gain))
    return m.to(dev)


@pytest.mark.gpu
def test_localize_windows_linear_is_the_composition_on_raw_scores(dev):
    """Two videos of 16 and 40 rows (one window, and four that overlap by half): localize_windows(nms="linear") equals _scores, soft
    top_moments per window and the soft merge of the windows' RAW scores, composed by hand.  nms_thresh = 0: every overlap decays, so
    the windows' own decayed scores differ from the raw ones that the merge must be given."""
    api = V()
    T, L = TINY_MODEL[0], TINY_MODEL[1]
    m = _model(TINY_MODEL, dev)
    g = torch.Generator().manual_seed(9)
    lens_v = [16, 40]
    raw = torch.randn(sum(lens_v), TINY_MODEL[6], generator=g).to(dev)
    qf = torch.randn(2, TINY_MODEL[7], 300, generator=g).to(dev)
    qm = (torch.arange(TINY_MODEL[7]).unsqueeze(0) < torch.tensor([7, 4]).unsqueeze(1)).to(torch.uint8).to(dev)
    kw = dict(k=5, k_window=4, nms_thresh=0.0, nms="linear")
    got = m.localize_windows(raw, lens_v, qf, qm, **kw)
    starts, wl, vptr = (x.tolist() for x in api.window_plan(lens_v, T, T // 2))
    assert vptr == [0, 1, 5] and starts == [0, 0, 8, 16, 24]
    pair = [0, 1, 1, 1, 1]
    begin = torch.tensor([s + (16 if p else 0) for s, p in zip(starts, pair)], dtype=torch.int64, device=dev)
    ln = torch.tensor(wl, dtype=torch.int32, device=dev)
    rows = torch.tensor(pair, device=dev)
    with torch.no_grad():
        vf, nfeats = api.sample_windows(raw, begin, ln, T, mode="pick")
        masks = api.build_masks_hip(nfeats, T, L)
        pm, ps, pe, _ = m._scores(vf, masks["video_mask"], qf[rows], qm[rows], masks["length_mask"], masks["moment_mask"])
    t = api.top_moments(pm, ps, pe, masks["moment_mask"], k=4, nms_thresh=0.0, nms="linear")
    want = api.merge_window_moments(t["idx"], t["raw_score"], t["count"], torch.tensor(starts, device=dev), ln,
                                    torch.tensor([0, 1, 5], device=dev), T, L, k=5, nms_thresh=0.0, nms="linear")
    for key in MERGE_KEYS:
        assert same(got[key], want[key]), key
    assert got["n_windows"].tolist() == [1, 4] and got["count"].tolist() == [4, 5]
    assert not same(t["raw_score"], t["score"])                                          # the windows' own decays did something
    loc = m.localize(vf, masks["video_mask"], qf[rows], qm[rows], masks["length_mask"], masks["moment_mask"], k=4, nms_thresh=0.0, nms="linear")
    same_lists(loc, t)


@pytest.mark.gpu
def test_c_abi_soft_merge_refusals(dev):
    api = V()
    lib = api._lib.load()
    idx, score, count, start, lens, pair_ptr = on(dev, window_candidates())
    G, kw, B, k = 8, 4, 3, 6
    sbuf, span = banded((B, k, 2), dev)
    obuf, out_score = banded((B, k), dev)
    rbuf, raw = banded((B, k), dev)
    wbuf, window, wsent = int_banded((B, k), dev, torch.int64)
    cbuf, cell, csent = int_banded((B, k, 2), dev, torch.int64)
    nbuf, out_count, nsent = int_banded((B,), dev, torch.int32)
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def call(method=1, sigma=0.5, k=k, **null):
        p = dict(idx=idx, score=score, pair_ptr=pair_ptr, span=span, out_score=out_score, raw=raw, window=window, cell=cell, out_count=out_count)
        p.update(null)
        return lib.smin_merge_window_moments_soft(st, _vp(p["idx"]), _vp(p["score"]), _vp(count), _vp(start), _vp(lens), _vp(p["pair_ptr"]), G, B, WT, WL,
                                                  kw, k, method, 0.5, sigma, float("-inf"), _vp(p["span"]), _vp(p["out_score"]), _vp(p["raw"]),
                                                  _vp(p["window"]), _vp(p["cell"]), _vp(p["out_count"]))
    bad = [dict(method=0), dict(method=3), dict(method=2, sigma=0.0), dict(method=2, sigma=float("nan")), dict(k=0), dict(k=65)]
    bad += [{name: None} for name in ("idx", "score", "pair_ptr", "span", "out_score", "raw", "window", "cell", "out_count")]
    for kw_ in bad:
        assert call(**kw_) != 0, kw_
    torch.cuda.synchronize()
    assert bool(torch.isnan(span).all()) and bool(torch.isnan(out_score).all()) and bool(torch.isnan(raw).all()) and bool((out_count == -7).all())
    assert call() == 0
    torch.cuda.synchronize()
    assert bands_intact(sbuf) and bands_intact(obuf) and bands_intact(rbuf)
    assert int_bands_intact(wbuf, wsent) and int_bands_intact(cbuf, csent) and int_bands_intact(nbuf, nsent)
    want = api.merge_window_moments_torch(*window_candidates(), WT, WL, k=k, nms_thresh=0.5, nms="linear")
    got = dict(span=span, score=out_score, raw_score=raw, window=window, cell=cell, count=out_count)
    for key in MERGE_KEYS:
        assert same(got[key].cpu(), want[key]), key
