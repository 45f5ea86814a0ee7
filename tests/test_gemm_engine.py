"""The contraction engines of csrc/gemm.h -- gemm_nt (exact fp32 MFMA), gemm_nt_x3 (bf16 matrix cores, NPROD 1 / 3 / 6), gemm_tn,
gemm_tn_bf16 and the slab reductions -- and the entry points built on them: the linear rows (csrc/linear_rows.hip) and the video
encoder (csrc/video_encoder.hip), against float64.

Mode-exact references: split_bf16x4 is reproducible on the host (hi = x.bfloat16(), the fp32 residual is exact, the next piece is the
residual's bfloat16()), so every reference is formed in float64 from exactly the bf16 products that mode's NPROD keeps.  What is left
between a kernel and its reference is fp32 accumulation (and the epilogue's few fp32 roundings), in every mode, and each element is
bounded on its own: |got - ref| <= TOL * (|A| |B|^T)_ij (plus the magnitudes of the epilogue's addends).

CPU: Python mirrors of launch_gemm_nt's grid and of the TN row splits (tn_splits, rows_per_split, padded XCD slots, empty splits);
the case lists below together reach every (engine kernel x mode x form x KFULL / dbias) combination, and the headline shapes are
put through the same mirrors.
GPU: every output is NaN-prefilled and checked element by element, sits between sentinel bands that must stay untouched, and every
case runs twice, bit for bit."""
import ctypes
import functools
import zlib

import pytest
import torch

from tests.helpers import GEMM_SLOTS, cdiv, tn_splits
from tests.support.device import dev  # noqa: F401  (the module's device fixture)
from tests.support.device import gemm_mode  # noqa: F401  (fixture)
from tests.support.references import nt_form, nt_grid, tn_forms, tn_grid

MODES = ("f32", "bf16x3", "bf16", "f32e")
KERNEL = {"f32": "gemm_nt", "bf16x3": "gemm_nt_x3<3>", "bf16": "gemm_nt_x3<1>", "f32e": "gemm_nt_x3<6>"}
TN_KERNEL = {"f32": "gemm_tn", "bf16x3": "gemm_tn_bf16<3>", "bf16": "gemm_tn_bf16<1>", "f32e": "gemm_tn_bf16<6>"}
TOL = 1e-6              # componentwise, every mode (test_gemm_engines_f32e: 1e-6 at K <= 2052)
TINY = 1e-30
GUARD = 1024            # sentinel floats before and after every output
SENTINEL = -7.375e33


# ---------------------------------------------------------------- mirrors of the launch arithmetic
def nt_block_tiles(M, N, K):
    """The (row0, rows, col0) output tile of every workgroup gemm_nt_kernel / gemm_nt_x3_kernel runs (idle slots omitted)."""
    g = nt_grid(M, N, K)
    out = []
    for bid in range(g["main_blocks"]):
        xcd, slot = bid & 7, bid >> 3
        tn, tm = slot % g["tiles_n"], (slot // g["tiles_n"]) * 8 + xcd
        if tm < g["main_tiles_m"]:
            out.append((tm * 128, 128, tn * 128))
    for i in range(g["mini_blocks"]):
        out.append((g["main_tiles_m"] * 128 + (i // g["tiles_n"]) * 32, 32, (i % g["tiles_n"]) * 128))
    return out


def tn_block_splits(Mrows, I, J):
    """(z, tile) of every workgroup gemm_tn_kernel / gemm_tn_bf16_kernel runs (padded slots omitted)."""
    g = tn_grid(Mrows, I, J)
    out = []
    for bid in range(g["grid"]):
        xcd, slot = bid & 7, bid >> 3
        z, tile = (slot // g["tiles"]) * 8 + xcd, slot % g["tiles"]
        if z < g["splits"]:
            out.append((z, tile))
    return out


# ---------------------------------------------------------------- GPU case lists

# gemm_nt / gemm_nt_acc: (M, N, K).  Large-M forms keep K at 16..36 so that the float64 references stay cheap; the long contractions
# (K = 1024 / 2052) run on mini-tile shapes.
NT_CASES = [
    (37, 20, 16), (300, 64, 2052), (1000, 128, 1024), (515, 132, 36),             # mini
    (8192, 600, 32), (8192, 600, 20),                                             # main (64 row tiles x 5 column tiles)
    (9000, 512, 32), (9000, 512, 36),                                             # main + idle slots (71 row tiles)
    (25000, 512, 32), (25000, 600, 36), (99999, 128, 20),                         # one round of main tiles + mini remainder
    (21800, 1024, 32), (172100, 128, 20),                                         # a round, then a remainder >= 3/4 of the slots
]
# linear-rows backward (dx through gemm_nt, dW / dbias through gemm_tn): (R, O, K, nseg)
TN_CASES = [
    (200, 128, 64, 1),              # splits = 1
    (20, 64, 36, 2),                # Mrows < 32
    (3000, 256, 100, 2),            # 12 splits; a 128-column tile of dx straddles the two segments
    (5121, 2560, 36, 4),            # 20 splits (padded XCD slots), the last two empty; CatMat with four segments
    (196700, 64, 32, 1),            # a single output tile: 768 splits (P >= 64: the wide slab reduction), 85 empty
]
# linear-rows forward: (R, O, K, nseg, C, bias, add_rows, add_cells)
LR_FWD_CASES = [
    (999, 128, 36, 3, 3, True, True, True),         # K % 16 != 0: K-steps straddle segments
    (1000, 64, 20, 2, 4, True, False, False),
    (515, 132, 64, 1, 1, False, False, False),
    (301, 100, 36, 4, 3, False, True, False),       # R % C != 0
    (4000, 96, 12, 2, 4, False, False, True),
    (64, 24, 16, 4, 1, True, True, False),
    (1027, 256, 100, 2, 4, True, False, True),
    (777, 68, 44, 3, 1, False, True, True),
    (9000, 512, 12, 3, 4, True, True, True),        # main tiles with idle slots
]
# video encoder: (B, T, Din, D)
VE_CASES = [
    (3, 50, 24, 64),
    (5, 100, 500, 512),             # mini tiles, Din % 16 != 0
    (33, 250, 500, 512),            # main tiles with K % 16 != 0 (the headline's form); 33 weight-gradient splits
    (60, 410, 132, 512),            # rounds + mini forward; 96 weight-gradient splits, the last ten empty
]

NT_FORMS = ("mini", "main", "main+idle-slots", "rounds+mini", "main-after-round")
TN_FORMS = ("splits=1", "splits%8!=0", "empty-trailing-split", "slots-capped", "Mrows<32")

# the headline workload (T=256, L=64, B=64, D=512, Din=500, dl=128; ~80 k moment cells assumed)
HEADLINE = {
    "video encoder forward": ("nt", 64 * 256, 512, 500),
    "moment unit forward": ("nt", 80000, 512, 1024),
    "moment unit input gradient": ("nt", 80000, 1024, 512),
    "content unit chat projection": ("nt", 80000 * 4, 128, 512),
    "video encoder weight gradient": ("tn", 64 * 256, 512, 500),
}


def test_headline_shapes_forms():
    """The forms the benchmark runs: main tiles with K % 16 != 0 for the video encoder, rounds + mini for the moment unit and the
    chat projection, and an empty trailing split (48 splits of 352 rows over 16 384) in the video encoder's weight gradient."""
    forms = {k: (nt_form(*v[1:]), nt_grid(*v[1:])["kfull"]) if v[0] == "nt" else tn_forms(*v[1:]) for k, v in HEADLINE.items()}
    assert forms["video encoder forward"] == ("main", False)
    assert forms["moment unit forward"] == ("rounds+mini", True)
    assert forms["moment unit input gradient"] == ("rounds+mini", True)
    assert forms["content unit chat projection"] == ("rounds+mini", True)
    assert forms["video encoder weight gradient"] == {"empty-trailing-split"}
    g = tn_grid(64 * 256, 512, 500)
    assert (g["splits"], g["rows_per_split"], g["empty"]) == (48, 352, [47])


def test_dispatch_mirrors_cover_every_tile_once():
    """The mirrored grids write every output tile exactly once: main tiles through the XCD swizzle (idle slots return), mini tiles
    after them; every (split, output tile) of a weight gradient once, padded slots returning."""
    shapes = [c for c in NT_CASES] + [(c[0], c[1], c[2] * c[3]) for c in TN_CASES] + [(M, N, K) for _, M, N, K in HEADLINE.values()]
    for M, N, K in shapes:
        g = nt_grid(M, N, K)
        tiles = nt_block_tiles(M, N, K)
        assert len(tiles) == len(set(tiles))
        rows = sorted({(r0, n) for r0, n, _ in tiles})
        covered = 0
        for r0, n in rows:
            assert r0 == covered, (M, N, K)
            covered += n
            assert sorted(c for r, _, c in tiles if r == r0) == [128 * t for t in range(g["tiles_n"])]
        assert covered >= M and covered - M < (32 if g["mini_blocks"] else 128), (M, N, K)
    for R, I, J in [(c[0], c[1], c[2] * c[3]) for c in TN_CASES] + [(B * T, D, Din) for B, T, Din, D in VE_CASES] + [(16384, 512, 500)]:
        g = tn_grid(R, I, J)
        blocks = tn_block_splits(R, I, J)
        assert sorted(blocks) == [(z, t) for z in range(g["splits"]) for t in range(g["tiles"])]
        assert g["rows_per_split"] % 32 == 0 and g["rows_per_split"] * g["splits"] >= R
    # gemm.h's `s > GEMM_SLOTS` cap never binds: cdiv(GEMM_SLOTS, tiles) <= GEMM_SLOTS already; a single-tile output over
    # > 196 352 rows is what reaches GEMM_SLOTS splits
    assert all(tn_splits(R, 128, 128) <= GEMM_SLOTS for R in (1, 10 ** 5, 10 ** 6, 10 ** 8))
    assert tn_splits(196352, 128, 128) == 767 and tn_splits(196353, 128, 128) == GEMM_SLOTS


def _nt_reached():
    return {(KERNEL[m], nt_form(*c), nt_grid(*c)["kfull"]) for c in NT_CASES for m in MODES}


def _tn_reached():
    return {(TN_KERNEL[m], f, bias) for c in TN_CASES for f in tn_forms(c[0], c[1], c[2] * c[3]) for m in MODES for bias in (False, True)}


def test_engine_cases_reach_every_form():
    """The GPU case lists reach every (engine kernel x mode x form x KFULL) of the NT engine and every (engine kernel x mode x split
    form x dbias requested) of the TN engine.  (The BIAS = false instances of the TN kernels are not reachable through the
    linear-rows or video-encoder ABI, which always pass a bias slab; without dbias the slab is not reduced.  They serve the BiLSTM
    recurrent weight gradient, tests/test_query_encoder.py.)"""
    nt_required = {(KERNEL[m], f, k) for m in MODES for f in NT_FORMS for k in (True, False)}
    missing = nt_required - _nt_reached()
    assert not missing, sorted(map(str, missing))
    tn_required = {(TN_KERNEL[m], f, b) for m in MODES for f in TN_FORMS for b in (False, True)}
    missing = tn_required - _tn_reached()
    assert not missing, sorted(map(str, missing))
    # the linear rows and the video encoder reach the forms that matter for them
    fwd = {(nt_form(c[0], c[1], c[2] * c[3]), c[2] % 16 == 0, c[3] > 1) for c in LR_FWD_CASES}
    assert ("main+idle-slots", False, True) in fwd and ("mini", False, True) in fwd
    assert {(b, r, c) for *_, b, r, c in LR_FWD_CASES} == {(b, r, c) for b in (False, True) for r in (False, True) for c in (False, True)}
    assert {c[4] for c in LR_FWD_CASES} == {1, 3, 4} and {c[3] for c in LR_FWD_CASES} == {1, 2, 3, 4}
    assert any(c[3] > 1 and c[2] % 16 for c in LR_FWD_CASES)                    # a K-step straddles two CatMat segments
    assert any(c[3] > 1 and c[2] % 128 and c[2] * c[3] > 128 for c in TN_CASES)  # a dx column tile straddles segments (EpSplitCols)
    ve_fwd = {(nt_form(B * T, D, Din), Din % 16 == 0) for B, T, Din, D in VE_CASES}
    assert ("main+idle-slots", False) in ve_fwd and ("rounds+mini", False) in ve_fwd
    assert any("empty-trailing-split" in tn_forms(B * T, D, Din) for B, T, Din, D in VE_CASES)
    assert all(T % 32 for _, T, _, _ in VE_CASES)


# ---------------------------------------------------------------- float64 references

# (piece of A, piece of B) of every product mfma_split_tiles forms (PA / PB, the last NPROD of the list); pieces: 0 = hi, 1, 2
PRODUCTS = {"bf16x3": ((1, 0), (0, 1), (0, 0)), "bf16": ((0, 0),), "f32e": ((2, 0), (0, 2), (1, 1), (1, 0), (0, 1), (0, 0))}


def split_pieces(x, n):
    """split_bf16x4 on the host: n bf16 pieces of fp32 x, hi first (each residual is exact in fp32)."""
    out, r = [], x.float()
    for _ in range(n):
        b = r.bfloat16().float()
        out.append(b)
        r = r - b
    return out


def contract_ref(a, b, mode):
    """sum_k a[i, k] b[j, k] in float64 from exactly the products `mode` forms (f32: the fp32 operands themselves)."""
    if mode == "f32":
        return a.double() @ b.double().t()
    prods = PRODUCTS[mode]
    n = 1 + max(max(p) for p in prods)
    pa, pb = split_pieces(a, n), split_pieces(b, n)
    out = None
    for i in range(n):                                  # grouped by the piece of A: the B pieces sum exactly in float64
        js = [j for ii, j in prods if ii == i]
        if js:
            bs = sum(pb[j].double() for j in js)
            t = pa[i].double() @ bs.t()
            out = t if out is None else out + t
    return out


def abs_bound(a, b):
    return a.double().abs() @ b.double().abs().t()


def worst_ratio(got, ref, bound):
    """max_ij |got - ref| / bound_ij (inf for a NaN: an element the kernel never wrote)"""
    got = got.detach().to(ref.device, torch.float64)
    if not torch.isfinite(got).all():
        return float("inf")
    if not got.numel():
        return 0.0
    return ((got - ref).abs() / (bound + TINY)).max().item()


def _gen(*key):
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))


def _rows(g, R, K, spread=2.0):
    """R x K normal values whose rows differ in magnitude by a few orders (the bf16 split is per element)."""
    return torch.randn(R, K, generator=g) * torch.exp(torch.randn(R, 1, generator=g) * spread)


# ---------------------------------------------------------------- GPU helpers
def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _arr(ts):
    return (ctypes.c_void_p * len(ts))(*[None if t is None else t.data_ptr() for t in ts])


class Guarded:
    """A NaN-prefilled output between two sentinel bands."""

    def __init__(self, shape, dev, fill=None):
        n = 1
        for s in shape:
            n *= s
        self.n = n
        self.buf = torch.full((2 * GUARD + n,), float("nan"), device=dev)
        self.buf[:GUARD] = SENTINEL
        self.buf[GUARD + n:] = SENTINEL
        self.t = self.buf[GUARD:GUARD + n].view(*shape)
        if fill is not None:
            self.t.copy_(fill)

    def check(self, what):
        band = torch.cat([self.buf[:GUARD], self.buf[GUARD + self.n:]])
        assert bool((band == SENTINEL).all()), f"{what}: a store outside the output"
        return self.t


def _ws_nan(nbytes, dev):
    w = torch.full((max(1, cdiv(int(nbytes), 4)),), float("nan"), device=dev)
    return w, w.numel() * 4


def _report(kind, mode, form, r):
    print(f"{kind:24s} {mode:7s} {form:40s} worst |err| / bound = {r:.3e}")


# ---------------------------------------------------------------- NT engine (smin_gemm_nt / smin_gemm_nt_acc)

@functools.lru_cache(maxsize=1)
def _nt_data(case):
    M, N, K = case
    g = _gen("nt", *case)
    a, b = _rows(g, M, K), _rows(g, N, K, 1.0)
    return a, b, abs_bound(a, b), torch.randn(M, N, generator=g)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("case", NT_CASES, ids=lambda c: "x".join(map(str, c)))
def test_gemm_nt_forms(dev, gemm_mode, case, mode):
    from vml_amd._lib import call, stream
    M, N, K = case
    a, b, bound, c0 = _nt_data(case)
    form = f"{nt_form(M, N, K)} KFULL={K % 16 == 0} {case}"
    gemm_mode(mode)
    ad, bd = a.to(dev), b.to(dev)
    outs = []
    for _ in range(2):
        c = Guarded((M, N), dev)
        call("smin_gemm_nt", stream(), _p(ad), _p(bd), _p(c.t), M, N, K)
        outs.append(c.check("smin_gemm_nt"))
    assert torch.equal(outs[0], outs[1]), "two runs differ"
    ref = contract_ref(a, b, mode)
    r = worst_ratio(outs[0], ref, bound)
    _report("gemm_nt", mode, form, r)
    assert r <= TOL, (mode, form, r)
    # accumulate epilogue: C0 + A B^T
    c = Guarded((M, N), dev, fill=c0.to(dev))
    call("smin_gemm_nt_acc", stream(), _p(ad), _p(bd), _p(c.t), M, N, K)
    r = worst_ratio(c.check("smin_gemm_nt_acc"), ref + c0.double(), bound + c0.double().abs())
    _report("gemm_nt_acc", mode, form, r)
    assert r <= TOL, (mode, form, "acc", r)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
def test_gemm_nt_identity_main_tiles(dev, gemm_mode, mode):
    """A = I against an asymmetric B on a main-tile shape (16 x 17 tiles): C must be B^T exactly, in every mode (B holds
    bf16-representable values, so the lower pieces are zero)."""
    from vml_amd._lib import call, stream
    K, N = 2048, 2176
    assert nt_form(K, N, K) == "main"
    a = torch.eye(K)
    b = (torch.randn(N, K, generator=_gen("eye")) * torch.arange(1, N + 1).view(N, 1) ** 0.5).bfloat16().float()
    gemm_mode(mode)
    ad, bd = a.to(dev), b.to(dev)
    c = Guarded((K, N), dev)
    call("smin_gemm_nt", stream(), _p(ad), _p(bd), _p(c.t), K, N, K)
    assert torch.equal(c.check("smin_gemm_nt").cpu(), b.t().contiguous())


# ---------------------------------------------------------------- linear rows: backward (dx through NT, dW / dbias through TN)

@functools.lru_cache(maxsize=1)
def _tn_data(case):
    R, O, K, nseg = case
    g = _gen("tn", *case)
    xs = [_rows(g, R, K) for _ in range(nseg)]
    X = torch.cat(xs, 1)
    dy = torch.randn(R, O, generator=g)             # (x's rows carry the spread: one spread operand per contraction, as the NT cases)
    W = torch.randn(O, nseg * K, generator=g)
    WT = W.t().contiguous()
    return xs, X, dy, WT, abs_bound(dy, WT), abs_bound(dy.t(), X.t()), dy.double().abs().sum(0)


@functools.lru_cache(maxsize=1)
def _tn_refs(case, mode):
    xs, X, dy, WT, *_ = _tn_data(case)
    return contract_ref(dy, WT, mode), contract_ref(dy.t(), X.t(), mode)


def _lr_bwd(dev, case, dy, xs, WT, want_w, want_b):
    from vml_amd._lib import call, load, stream
    R, O, K, nseg = case
    Kt = nseg * K
    dxs = [Guarded((R, K), dev) for _ in range(nseg)]
    dW = Guarded((O, Kt), dev) if want_w else None
    db = Guarded((O,), dev) if want_b else None
    ws, nb = _ws_nan(load().smin_linear_rows_bwd_workspace_bytes(R, O, Kt), dev)
    call("smin_linear_rows_bwd", stream(), _p(dy), _arr(xs), nseg, _p(WT), R, O, K, _arr([d.t for d in dxs]),
         dW and _p(dW.t), db and _p(db.t), _p(ws), nb)
    return ([d.check("dx") for d in dxs], dW and dW.check("dW"), db and db.check("dbias"))


@pytest.mark.gpu
@pytest.mark.parametrize("bias", [False, True], ids=["dbias=NULL", "dbias"])
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("case", TN_CASES, ids=lambda c: "x".join(map(str, c)))
def test_linear_rows_bwd_forms(dev, gemm_mode, case, mode, bias):
    R, O, K, nseg = case
    xs, X, dy, WT, bdx, bdw, bdb = _tn_data(case)
    form = f"{sorted(tn_forms(R, O, K * nseg))} {case}"
    gemm_mode(mode)
    xsd, dyd, WTd = [x.to(dev) for x in xs], dy.to(dev), WT.to(dev)
    runs = [_lr_bwd(dev, case, dyd, xsd, WTd, True, bias) for _ in range(2)]
    for u, v in zip(runs[0][0] + [runs[0][1]], runs[1][0] + [runs[1][1]]):
        assert torch.equal(u, v), "two runs differ"
    if bias:
        assert torch.equal(runs[0][2], runs[1][2])
    dxs, dW, db = runs[0]
    ref_dx, ref_dw = _tn_refs(case, mode)
    r = worst_ratio(torch.cat(dxs, 1), ref_dx, bdx)
    _report("linear_rows dx (NT)", mode, form, r)
    assert r <= TOL, ("dx", mode, form, r)
    r = worst_ratio(dW, ref_dw, bdw)
    _report("linear_rows dW (TN)", mode, form, r)
    assert r <= TOL, ("dW", mode, form, r)
    if bias:
        # the bias slabs sum the fp32 operand values themselves (not the split pieces): exact fp32 sums in every mode
        r = worst_ratio(db, dy.double().sum(0), bdb)
        _report("linear_rows dbias", mode, form, r)
        assert r <= TOL, ("dbias", mode, form, r)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("case", [(3000, 256, 100, 2), (999, 128, 36, 3), (2048, 64, 16, 1)], ids=lambda c: "x".join(map(str, c)))
def test_linear_rows_bwd_input_half(dev, gemm_mode, case, mode):
    """dW == NULL (and dbias NULL): only the input gradients, written into their own tensors (EpSplitCols for nseg > 1)."""
    R, O, K, nseg = case
    g = _gen("lrin", *case)
    dy, WT = _rows(g, R, O), torch.randn(nseg * K, O, generator=g)
    gemm_mode(mode)
    dyd, WTd = dy.to(dev), WT.to(dev)
    dxs, dW, db = _lr_bwd(dev, case, dyd, [None] * nseg, WTd, False, False)
    assert dW is None and db is None
    r = worst_ratio(torch.cat(dxs, 1), contract_ref(dy, WT, mode), abs_bound(dy, WT))
    _report("linear_rows dx only", mode, str(case), r)
    assert r <= TOL, (mode, case, r)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("case", [(1000, 128, 64, 1), (999, 128, 36, 3), (9000, 512, 12, 2)], ids=lambda c: "x".join(map(str, c)))
def test_linear_rows_dx_acc(dev, gemm_mode, case, mode):
    """smin_linear_rows_dx_acc: dx_s already holding another consumer's gradient receives dx_s + dy W_s."""
    from vml_amd._lib import call, stream
    R, O, K, nseg = case
    g = _gen("dxacc", *case)
    dy, WT = _rows(g, R, O), torch.randn(nseg * K, O, generator=g)
    dx0 = [torch.randn(R, K, generator=g) * 3 for _ in range(nseg)]
    gemm_mode(mode)
    dxs = [Guarded((R, K), dev, fill=d.to(dev)) for d in dx0]
    dyd, WTd = dy.to(dev), WT.to(dev)
    call("smin_linear_rows_dx_acc", stream(), _p(dyd), nseg, _p(WTd), R, O, K, _arr([d.t for d in dxs]))
    got = torch.cat([d.check("dx_acc") for d in dxs], 1)
    D0 = torch.cat(dx0, 1).double()
    r = worst_ratio(got, contract_ref(dy, WT, mode) + D0, abs_bound(dy, WT) + D0.abs())
    _report("linear_rows dx_acc", mode, f"{nt_form(R, nseg * K, O)} {case}", r)
    assert r <= TOL, (mode, case, r)


# ---------------------------------------------------------------- linear rows: forward

def _lr_fwd_inputs(case):
    R, O, K, nseg, C, hb, hr, hc = case
    g = _gen("lrf", *case)
    xs = [_rows(g, R, K) for _ in range(nseg)]
    W = torch.randn(O, nseg * K, generator=g)
    bias = torch.randn(O, generator=g) if hb else None
    ar = torch.randn(R, O, generator=g) * 4 if hr else None
    ac = torch.randn(cdiv(R, C), O, generator=g) * 4 if hc else None
    return xs, W, bias, ar, ac


def _lr_fwd_ref(case, xs, W, bias, ar, ac, mode):
    R, O, K, nseg, C = case[:5]
    X = torch.cat(xs, 1)
    ref, bound = contract_ref(X, W, mode), abs_bound(X, W)
    for t in (bias, ar, None if ac is None else ac[torch.arange(R) // C]):
        if t is not None:
            ref, bound = ref + t.double(), bound + t.double().abs()
    return ref, bound


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("case", LR_FWD_CASES, ids=lambda c: "-".join(map(str, c)))
def test_linear_rows_fwd(dev, gemm_mode, case, mode):
    from vml_amd._lib import call, stream
    R, O, K, nseg, C = case[:5]
    xs, W, bias, ar, ac = _lr_fwd_inputs(case)
    gemm_mode(mode)
    d = lambda t: None if t is None else t.to(dev)
    xsd, Wd, bd, ard, acd = [d(x) for x in xs], d(W), d(bias), d(ar), d(ac)
    outs = []
    for _ in range(2):
        y = Guarded((R, O), dev)
        call("smin_linear_rows_fwd", stream(), _arr(xsd), nseg, _p(Wd), _p(bd), _p(ard), _p(acd), C, R, O, K, _p(y.t))
        outs.append(y.check("linear_rows_fwd"))
    assert torch.equal(outs[0], outs[1])
    ref, bound = _lr_fwd_ref(case, xs, W, bias, ar, ac, mode)
    r = worst_ratio(outs[0], ref, bound)
    _report("linear_rows fwd", mode, f"{nt_form(R, O, nseg * K)} {case}", r)
    assert r <= TOL, (mode, case, r)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("case", [(999, 128, 36, 3, 3, True, True, True), (777, 68, 44, 1, 1, False, True, True),
                                  (9000, 512, 12, 2, 4, True, True, True)], ids=lambda c: "-".join(map(str, c)))
def test_linear_rows_xh_equal_fp32_storage(dev, gemm_mode, case, mode):
    """_xh forward and backward on bf16-stored x equal the fp32-storage calls on the same (bf16-representable) values bit for bit, in
    every mode: loading a representable value is exact and its split has zero lower pieces."""
    from vml_amd._lib import call, load, stream
    R, O, K, nseg, C = case[:5]
    xs, W, bias, ar, ac = _lr_fwd_inputs(case)
    xs = [x.bfloat16().float() for x in xs]
    gemm_mode(mode)
    d = lambda t: None if t is None else t.to(dev)
    xsd, Wd, bd, ard, acd = [d(x) for x in xs], d(W), d(bias), d(ar), d(ac)
    xhd = [x.bfloat16().view(torch.int16).to(dev) for x in xs]
    y32, yh = Guarded((R, O), dev), Guarded((R, O), dev)
    call("smin_linear_rows_fwd", stream(), _arr(xsd), nseg, _p(Wd), _p(bd), _p(ard), _p(acd), C, R, O, K, _p(y32.t))
    call("smin_linear_rows_fwd_xh", stream(), _arr(xhd), nseg, _p(Wd), _p(bd), _p(ard), _p(acd), C, R, O, K, _p(yh.t))
    assert torch.equal(y32.check("fwd"), yh.check("fwd_xh"))
    ref, bound = _lr_fwd_ref(case, xs, W, bias, ar, ac, mode)
    assert worst_ratio(yh.t, ref, bound) <= TOL
    dy = torch.randn(R, O, generator=_gen("xhdy", *case)).to(dev)
    Kt = nseg * K
    nb = load().smin_linear_rows_bwd_workspace_bytes(R, O, Kt)
    w1, n1 = _ws_nan(nb, dev)
    w2, n2 = _ws_nan(nb, dev)
    dW32, db32, dWh, dbh = Guarded((O, Kt), dev), Guarded((O,), dev), Guarded((O, Kt), dev), Guarded((O,), dev)
    WTd = Wd.t().contiguous()
    call("smin_linear_rows_bwd", stream(), _p(dy), _arr(xsd), nseg, _p(WTd), R, O, K, None, _p(dW32.t), _p(db32.t), _p(w1), n1)
    call("smin_linear_rows_bwd_xh", stream(), _p(dy), _arr(xhd), nseg, R, O, K, _p(dWh.t), _p(dbh.t), _p(w2), n2)
    assert torch.equal(dW32.check("bwd dW"), dWh.check("bwd_xh dW")) and torch.equal(db32.check("bwd dbias"), dbh.check("bwd_xh dbias"))
    X = torch.cat(xs, 1)
    assert worst_ratio(dWh.t, contract_ref(dy.cpu().t(), X.t(), mode), abs_bound(dy.cpu().t(), X.t())) <= TOL


@pytest.mark.gpu
@pytest.mark.parametrize("groups,C,W", [(1, 1, 4), (333, 3, 132), (1000, 4, 512), (77, 7, 20)])
def test_group_sum(dev, groups, C, W):
    from vml_amd._lib import call, stream
    x = _rows(_gen("gs", groups, C, W), groups * C, W)
    xd, out = x.to(dev), Guarded((groups, W), dev)
    call("smin_group_sum", stream(), _p(xd), groups, C, W, _p(out.t))
    xv = x.double().view(groups, C, W)
    r = worst_ratio(out.check("group_sum"), xv.sum(1), xv.abs().sum(1))
    assert r <= TOL, r


# ---------------------------------------------------------------- video encoder

@functools.lru_cache(maxsize=1)
def _ve_data(case):
    B, T, Din, D = case
    g = _gen("ve", *case)
    x = _rows(g, B * T, Din)
    W, bias, pe = torch.randn(D, Din, generator=g) * 0.05, torch.randn(D, generator=g), torch.randn(T + 7, D, generator=g)
    u = torch.rand(B * T, generator=g)
    vm = torch.where(u < 0.15, torch.zeros(()), torch.where(u < 0.35, torch.rand(B * T, generator=g), torch.ones(())))   # 0, fractional, 1
    vm[T - 3:T] = 0.0                                                   # a padded tail on the first sample
    fs = torch.randn(B, D, generator=g)
    df = torch.randn(B * T, D, generator=g)         # (x's rows carry the spread of the weight-gradient contraction)
    fv = torch.randn(B * T, D, generator=g)
    return x, W, bias, pe, vm, fs, df, fv, abs_bound(x, W)


def _ve_dv(case, df, fs, vm):
    """dv = df * fs[b] * vmask as video_enc_bwd_rows_kernel forms it in fp32 (two rounded products, in that order)"""
    B, T, Din, D = case
    return (df.view(B, T, D) * fs.view(B, 1, D)).mul(vm.view(B, T, 1)).view(B * T, D)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("case", VE_CASES, ids=lambda c: "x".join(map(str, c)))
def test_video_encoder_fwd(dev, gemm_mode, case, mode):
    """fv = (x W^T + bias + pe[t]) * vmask, f = fv * fs: the fused call, the projection alone + smin_video_encoder_gate, against
    float64 -- T not a multiple of 32 (samples change inside tiles), pe longer than T, zero and fractional vmask."""
    from vml_amd._lib import call, stream
    B, T, Din, D = case
    x, W, bias, pe, vm, fs, _, _, bxw = _ve_data(case)
    gemm_mode(mode)
    xd, Wd, bd, ped, vmd, fsd = (t.to(dev) for t in (x, W, bias, pe, vm, fs))
    fv1, f1, fv2, f2 = (Guarded((B * T, D), dev) for _ in range(4))
    call("smin_video_encoder_fwd", stream(), _p(xd), _p(Wd), _p(bd), _p(ped), _p(vmd), _p(fsd), B, T, Din, D, _p(fv1.t), _p(f1.t))
    call("smin_video_encoder_fwd", stream(), _p(xd), _p(Wd), _p(bd), _p(ped), _p(vmd), None, B, T, Din, D, _p(fv2.t), None)
    call("smin_video_encoder_gate", stream(), _p(fv2.t), _p(fsd), B, T, D, _p(f2.t))
    assert torch.equal(fv1.check("fv"), fv2.check("fv alone")) and torch.equal(f1.check("f"), f2.check("gate f"))
    tt = torch.arange(B * T) % T
    m = vm.double().view(-1, 1)
    ref = (contract_ref(x, W, mode) + bias.double() + pe.double()[tt]) * m
    bound = (bxw + bias.double().abs() + pe.double().abs()[tt]) * m.abs()
    form = f"{nt_form(B * T, D, Din)} KFULL={Din % 16 == 0} {case}"
    r = worst_ratio(fv1.t, ref, bound)
    _report("video_encoder fv", mode, form, r)
    assert r <= TOL, ("fv", mode, case, r)
    fsr = fs.double()[torch.arange(B * T) // T]
    r = worst_ratio(f1.t, ref * fsr, bound * fsr.abs())
    assert r <= TOL, ("f", mode, case, r)
    assert bool((fv1.t[vm.to(dev) == 0] == 0).all())


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("case", VE_CASES, ids=lambda c: "x".join(map(str, c)))
def test_video_encoder_bwd(dev, gemm_mode, case, mode):
    """dW, dbias, dpe, dfs against float64 as one call and as the two halves on one workspace (bit for bit), then
    smin_video_encoder_bwd_input's dx = dv W with the masked frames' rows exactly zero."""
    from vml_amd._lib import call, load, stream
    B, T, Din, D = case
    x, W, bias, pe, vm, fs, df, fv, _ = _ve_data(case)
    gemm_mode(mode)
    xd, vmd, fsd, dfd, fvd = (t.to(dev) for t in (x, vm, fs, df, fv))
    nb = load().smin_video_encoder_bwd_workspace_bytes(B, T, Din, D)

    def bwd(split):
        ws, n = _ws_nan(nb, dev)
        dW, db, dpe, dfs = Guarded((D, Din), dev), Guarded((D,), dev), Guarded((T, D), dev), Guarded((B, D), dev)
        if split:
            call("smin_video_encoder_bwd", stream(), _p(dfd), _p(fvd), _p(fsd), _p(vmd), _p(xd), B, T, Din, D, None, None, None, _p(dfs.t), _p(ws), n)
            call("smin_video_encoder_bwd", stream(), None, _p(fvd), _p(fsd), _p(vmd), _p(xd), B, T, Din, D, _p(dW.t), _p(db.t), _p(dpe.t), None, _p(ws), n)
        else:
            call("smin_video_encoder_bwd", stream(), _p(dfd), _p(fvd), _p(fsd), _p(vmd), _p(xd), B, T, Din, D, _p(dW.t), _p(db.t), _p(dpe.t), _p(dfs.t), _p(ws), n)
        return [t.check(k) for t, k in ((dW, "dW"), (db, "dbias"), (dpe, "dpe"), (dfs, "dfs"))], ws

    one, ws = bwd(False)
    two, _ = bwd(True)
    for k, a, b in zip(("dW", "dbias", "dpe", "dfs"), one, two):
        assert torch.equal(a, b), k
    dv = _ve_dv(case, df, fs, vm)
    dvd, dva = dv.double().view(B, T, D), dv.double().abs().view(B, T, D)
    pf, pfa = (df.double() * fv.double()).view(B, T, D), (df.double() * fv.double()).abs().view(B, T, D)
    form = f"{sorted(tn_forms(B * T, D, Din))} {case}"
    checks = {"dW": (contract_ref(dv.t(), x.t(), mode), abs_bound(dv.t(), x.t())), "dbias": (dvd.sum((0, 1)), dva.sum((0, 1))),
              "dpe": (dvd.sum(0), dva.sum(0)), "dfs": (pf.sum(1), pfa.sum(1))}
    for (k, (ref, bound)), got in zip(checks.items(), one):
        r = worst_ratio(got, ref, bound)
        _report(f"video_encoder {k}", mode, form, r)
        assert r <= TOL, (k, mode, case, r)
    # input gradient from the same workspace
    WT = W.t().contiguous()
    WTd = WT.to(dev)
    dx = Guarded((B * T, Din), dev)
    call("smin_video_encoder_bwd_input", stream(), _p(WTd), _p(vmd), B, T, Din, D, _p(dx.t), _p(ws), nb)
    got = dx.check("dx")
    r = worst_ratio(got, contract_ref(dv, WT, mode), abs_bound(dv, WT))
    _report("video_encoder dx", mode, f"{nt_form(B * T, Din, D)} KFULL={D % 16 == 0} {case}", r)
    assert r <= TOL, ("dx", mode, case, r)
    zero_rows = got[vm.to(dev) == 0]
    assert zero_rows.numel() and bool((zero_rows == 0).all())
