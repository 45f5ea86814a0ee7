"""Target construction -- csrc/labels.hip (smin_build_targets), feeder.build_targets_hip, labels.build_targets, BatchFeeder and the
checker oracle/labels_oracle.py -- against data the reference's own code produced.

tests/golden/make_golden_targets.py runs ``get_iou``, ``get_boundary_penalties``, ``get_snippet_label``, ``__getitem__`` and
``collate_fn`` of the reference's dataset.py (extracted with ``ast``; the module itself cannot be imported) and stores
gb_targets.npz (function level: clipped annotations, times on and one fp32 step off a snippet boundary, IoU exactly and one fp32 step
off one half, 1 ms / one-snippet / whole-video moments, Gaussians in the subnormal range, durations 2 .. 760 s, two-decimal doubles
that fp32 cannot hold, window-form geometry, ts == te) and gc_feeder_batch.npz (collated batches of the stub dataset).  No test here
reads a reference checkout except the regeneration test, which skips without one.

What is demanded: ``sm`` bit for bit (NaN by position), every label and mask exactly, with no exclusions (the generator asserts that
no stored ss / se lies within 1e-6 of the 0.5 threshold).  The arithmetic is IEEE mul, div, min, max, sub in the reference's order.
``ss`` / ``se`` go through ``exp``, which differs between libraries, so they are bounded as follows (``penalty_ulps``): the yardstick is
``exp`` in fp64 of the fp32 argument ``-(a * a) / den`` recomputed in numpy fp32 from the fixture's inputs and the once-rounded
denominator; ``e_ref`` is the fixture's error against it in units of ``np.spacing`` of the yardstick rounded to fp32 (the
reference's own CPU ``exp``); a value under test may err by ``max(2 * e_ref_max, 1)`` of those units, ``e_ref_max`` over the batch: the
factor 2 allows a second, independent exp of the same quality, the floor of 1 covers a correctly rounded reference.  The oracle
runs the reference's torch ops, so it is held to one fp32 spacing of the fixture (another CPU may take another vector exp)."""
import functools
import importlib.util
import os

import numpy as np
import pytest
import torch

from oracle import labels_oracle as LO
from tests import helpers as H
from tests.support.device import dev  # noqa: F401  (the module's device fixture)
from tests.support.device import vml as V

f32 = np.float32
LS = (5, 16, 17, 32, 64)
T_OF = {5: 5, 16: 64, 17: 34, 32: 128, 64: 256}                # the T each fixture-(a) group is launched with
GROUPS = [(T, L, split) for T, L in ((64, 16), (128, 32)) for split in ("val", "train")]
MASKS, LABELS = ("video_mask", "length_mask", "moment_mask"), ("ym", "ys", "ye", "ya")
KEYS = ["video_features", "video_mask", "query_features", "query_mask", "length_mask", "moment_mask", "sm", "ym", "ss", "ys", "se", "ye", "ya"]
GUARD, SENTINEL = H.LAYOUT_GUARD, H.LAYOUT_SENTINEL


@functools.lru_cache(maxsize=None)
def fixture_a():
    """{L: dict(ts, te, dur, fam, sm, ss, se, ya)}, the family names, the window cases.  Shared, never written."""
    z = H.load_npz("gb_targets")
    groups = {L: {k: z[f"L{L}/{k}"] for k in ("ts", "te", "dur", "fam", "sm", "ss", "se", "ya")} for L in LS}
    return groups, [str(s) for s in z["families"]], {k[4:]: z[k] for k in z.files if k.startswith("win/")}


@functools.lru_cache(maxsize=None)
def fixture_b():
    z = H.load_npz("gc_feeder_batch")
    out = {}
    for T, L, split in GROUPS:
        pre = f"T{T}L{L}_{split}/"
        g = {k[len(pre):]: z[k] for k in z.files if k.startswith(pre)}
        g["out"] = {k[4:]: v for k, v in g.items() if k.startswith("out/")}
        out[T, L, split] = g
    return out, z["table"], int(z["pad"])


def nfeats_for(n, T):
    """Sampled-frame counts for fixture (a)'s cases: 0, 1, every snippet edge's neighbours, T and beyond, in turn."""
    return (np.arange(n) * 7) % (T + 3)


def same_bits(got, want):
    """fp32 arrays equal bit for bit, except that any NaN matches any NaN at the same position."""
    got, want = np.ascontiguousarray(got, np.float32), np.ascontiguousarray(want, np.float32)
    nan = np.isnan(want)
    return got.shape == want.shape and np.array_equal(np.isnan(got), nan) and np.array_equal(got.view(np.int32)[~nan], want.view(np.int32)[~nan])


def denominators(ts, te):
    """2 sigma^2 in double from the float64 annotation, rounded once (dataset.py:116-119)."""
    return (2.0 * ((np.asarray(te, np.float64) - np.asarray(ts, np.float64)) / 5.0) ** 2).astype(np.float32)


def penalty_ulps(ts, te, dur, L, ss, se):
    """Errors of ``ss`` / ``se`` (n, L) against the fp64 yardstick, in fp32 spacings of the yardstick (module docstring); (n, 2L).
    Rows with ts == te (no Gaussian: 0 / 0 or -x / 0) hold 0 and are compared exactly elsewhere."""
    ts, te, dur = (np.asarray(x, np.float64).reshape(-1) for x in (ts, te, dur))
    k = np.arange(L, dtype=np.float32)[None, :]
    durf, Lf = dur.astype(np.float32)[:, None], f32(L)
    s, e = k * durf / Lf, (k + f32(1)) * durf / Lf
    a = np.concatenate([s - ts.astype(np.float32)[:, None], e - te.astype(np.float32)[:, None]], 1)
    with np.errstate(all="ignore"):
        arg = -(a * a) / denominators(ts, te)[:, None]
        assert arg.dtype == np.float32
        yard = np.exp(arg.astype(np.float64))
        err = np.abs(np.concatenate([ss, se], 1).astype(np.float64) - yard) / np.spacing(yard.astype(np.float32)).astype(np.float64)
    return np.where((ts < te)[:, None], err, 0.0)


def check_penalties(what, ts, te, dur, L, got_ss, got_se, ref_ss, ref_se):
    """The bound of the module docstring for one batch; returns (e_ref_max, worst error of the values under test)."""
    e_ref = float(penalty_ulps(ts, te, dur, L, ref_ss, ref_se).max())
    err = penalty_ulps(ts, te, dur, L, got_ss, got_se)
    worst = float(np.nanmax(np.where(np.isnan(err), np.inf, err)))
    degenerate = ~(np.asarray(ts) < np.asarray(te))
    for got, ref in ((got_ss, ref_ss), (got_se, ref_se)):                  # ts == te: NaN by position, 0 exactly
        assert same_bits(np.asarray(got)[degenerate], np.asarray(ref)[degenerate]), (what, "ts == te rows")
    print(f"{what}: ss/se e_ref_max = {e_ref:.3f} spacings, under test {worst:.3f}, bound {max(2 * e_ref, 1):.3f}")
    assert worst <= max(2 * e_ref, 1), (f"{what}: ss / se err by {worst:.3f} fp32 spacings of the fp64 yardstick; the reference's own exp errs by "
                                        f"{e_ref:.3f}, which allows {max(2 * e_ref, 1):.3f}")
    return e_ref, worst


def check_group(what, g, L, got, ss_ref=None):
    """``got`` (dict of numpy arrays, a row per case of fixture-(a) group ``g``) against the reference: sm bit for bit, labels exactly,
    ss / se within the bound."""
    assert same_bits(got["sm"], g["sm"]), (what, "sm", np.nonzero(np.any(got["sm"].view(np.int32) != g["sm"].view(np.int32), axis=(1, 2)))[0][:8])
    want = dict(ym=g["sm"] > f32(0.5), ys=g["ss"] > f32(0.5), ye=g["se"] > f32(0.5), ya=g["ya"].astype(bool))
    for k, v in want.items():
        bad = np.nonzero(np.any((got[k].astype(bool) != v).reshape(v.shape[0], -1), axis=1))[0]
        assert bad.size == 0, (what, k, "cases", bad[:8], [(g["ts"][b], g["te"][b], g["dur"][b]) for b in bad[:3]])
    return check_penalties(what, g["ts"], g["te"], g["dur"], L, got["ss"], got["se"], g["ss"], g["se"])


def check_masks(what, got, nfeats, T, L):
    """The three masks against the oracle's (pinned to the reference's collated batches by the sample-level test)."""
    for b, nf in enumerate(np.asarray(nfeats).tolist()):
        ref = mask_reference(int(nf), T, L)
        for k in MASKS:
            assert np.array_equal(np.asarray(got[k][b]).astype(np.uint8).reshape(-1), ref[k]), (what, k, b, nf)


@functools.lru_cache(maxsize=None)
def mask_reference(nf, T, L):
    ref = LO.sample_targets(0.0, 1.0, 2.0, nf, T, L)
    return {k: ref[k].numpy().astype(np.uint8).reshape(-1) for k in MASKS}


# ---------------------------------------------------------------- CPU: the fixtures themselves
def test_fixture_families_are_present():
    groups, families, win = fixture_a()
    assert families == ["clipped", "boundary", "iou_half", "extreme", "subnormal", "durations", "double", "fp32", "window", "degenerate"]
    fam = np.concatenate([g["fam"] for g in groups.values()])
    assert (np.bincount(fam, minlength=len(families)) > 0).all()
    half = f32(0.5)
    sm = np.concatenate([g["sm"].ravel() for g in groups.values()])
    pen = np.concatenate([np.concatenate([g["ss"].ravel(), g["se"].ravel()]) for g in groups.values()])
    assert (sm == half).sum() >= 8 and (sm == np.nextafter(half, f32(1))).sum() >= 1 and (sm == np.nextafter(half, f32(0))).sum() >= 1
    assert ((pen > 0) & (pen < np.finfo(np.float32).tiny)).sum() >= 4 and (pen == 0).sum() >= 4 and np.isnan(pen).sum() >= 2 and np.isnan(sm).sum() >= 1
    assert np.nanmin(np.abs(pen.astype(np.float64) - 0.5)) > 1e-6             # ys / ye can be demanded exactly, no exclusions
    for L, g in groups.items():
        rep = lambda x: x.astype(np.float32).astype(np.float64) == x
        single, double = g["fam"] == families.index("fp32"), g["fam"] == families.index("double")
        assert single.any() and (rep(g["ts"]) & rep(g["te"]) & rep(g["dur"]))[single].all()
        assert double.any() and not (rep(g["ts"]) | rep(g["te"]))[double].any()
        assert g["ts"].dtype == np.float64 and g["sm"].shape == (len(g["ts"]), L, L) and g["ss"].shape == (len(g["ts"]), L)
        assert ((g["ts"] == 631.06) & (g["te"] == 631.41) & (g["dur"] == 673.65)).any()
    assert len(groups[64]["ts"]) <= 32                                         # the 64s are few
    every = lambda k: np.concatenate([g[k] for g in groups.values()])
    assert every("dur").min() == 2.0 and every("dur").max() == 760.0
    assert (every("ts") < 0).any() and (every("te") > every("dur")).any() and (every("te") < 0).any() and (every("ts") > every("dur")).any()
    assert (every("ts") == every("te")).sum() == 8 and win["case"].shape == (2,)
    size = sum(os.path.getsize(os.path.join(H.GOLDEN, n)) for n in ("gb_targets.npz", "gc_feeder_batch.npz"))
    assert size <= os.path.getsize(os.path.join(H.GOLDEN, "g3_c3.npz"))


def kernel_model(ts, te, dur, L, e_split=False, ym_ge=False, ya_gt=False):
    """csrc/labels.hip's fp32 arithmetic for sm, ym and ya in numpy, one case; the flags are the three slips the fixture must catch:
    e_j formed as j * dur / L + dur / L, ym = sm >= 0.5, ya with s_t > ts."""
    tsf, tef, durf, Lf = f32(ts), f32(te), f32(dur), f32(L)
    k = np.arange(L, dtype=np.float32)
    s = k * durf / Lf
    e = k * durf / Lf + durf / Lf if e_split else (k + f32(1)) * durf / Lf
    si, ej = s[:, None], e[None, :]
    with np.errstate(all="ignore"):
        sm = np.maximum(f32(0), np.minimum(ej, tef) - np.maximum(si, tsf)) / np.maximum(f32(0), np.maximum(ej, tef) - np.minimum(si, tsf))
        ym = sm >= f32(0.5) if ym_ge else sm > f32(0.5)
    return sm, ym, ((s > tsf) if ya_gt else (s >= tsf)) & (e <= tef)


def test_fixture_catches_the_three_slips():
    """A numpy model of the kernel's arithmetic reproduces the reference's sm, ym and ya on every case; with `>` turned into `>=` in
    ym, `>=` into `>` in ya, or (j + 1) * dur / L into j * dur / L + dur / L, it disagrees inside the families built for that
    (boundary, iou_half), so a kernel with such a slip fails the device test below."""
    groups, families, _ = fixture_a()
    hits = dict(e_split=set(), ym_ge=set(), ya_gt=set())
    for L, g in groups.items():
        for c in range(len(g["ts"])):
            args = (g["ts"][c], g["te"][c], g["dur"][c], L)
            sm, ym, ya = kernel_model(*args)
            assert same_bits(sm, g["sm"][c]) and np.array_equal(ym, g["sm"][c] > f32(0.5)) and np.array_equal(ya, g["ya"][c].astype(bool)), (L, c)
            for slip in hits:
                m = kernel_model(*args, **{slip: True})
                if not (same_bits(m[0], sm) and np.array_equal(m[1], ym) and np.array_equal(m[2], ya)):
                    hits[slip].add(families[g["fam"][c]])
    print({k: sorted(v) for k, v in hits.items()})
    assert "iou_half" in hits["ym_ge"] and "boundary" in hits["ya_gt"] and {"boundary", "iou_half"} & hits["e_split"]


def test_generator_reproduces_the_fixtures(tmp_path):
    """With a checkout of the reference beside this repository (or named by SMIN_REFERENCE_DIR) the generator writes the two
    fixtures again, array for array and bit for bit."""
    ref_dir = os.environ.get("SMIN_REFERENCE_DIR") or os.path.join(os.path.dirname(os.path.dirname(os.path.dirname(H.GOLDEN))), "reference")
    if not os.path.exists(os.path.join(ref_dir, "dataset.py")):
        pytest.skip("no checkout of the reference here")
    spec = importlib.util.spec_from_file_location("make_golden_targets", os.path.join(H.GOLDEN, "make_golden_targets.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    state = np.random.get_state()
    try:
        paths = gen.main(ref_dir, str(tmp_path))
    finally:
        np.random.set_state(state)
    for path in paths:
        new, old = np.load(path), np.load(os.path.join(H.GOLDEN, os.path.basename(path)))
        assert sorted(new.files) == sorted(old.files)
        for k in old.files:
            assert new[k].dtype == old[k].dtype and new[k].shape == old[k].shape and new[k].tobytes() == old[k].tobytes(), (path, k)


# ---------------------------------------------------------------- CPU: the oracle and the torch form
def within_one_spacing(got, want):
    got, want = np.asarray(got, np.float32), np.asarray(want, np.float32)
    nan = np.isnan(want)
    return np.array_equal(np.isnan(got), nan) and bool((np.abs(got[~nan].astype(np.float64) - want[~nan]) <= np.spacing(np.abs(want[~nan]))).all())


@pytest.mark.parametrize("L", LS)
def test_oracle_functions_match_reference(L):
    g = fixture_a()[0][L]
    for c in range(len(g["ts"])):
        ts, te, dur = float(g["ts"][c]), float(g["te"][c]), float(g["dur"][c])
        assert same_bits(LO.get_iou(ts, te, dur, L).numpy(), g["sm"][c]), (L, c)
        ss, se = LO.get_boundary_penalties(ts, te, dur, L)
        assert within_one_spacing(ss.numpy(), g["ss"][c]) and within_one_spacing(se.numpy(), g["se"][c]), (L, c)
        assert np.array_equal(LO.get_snippet_label(ts, te, dur, L).numpy(), g["ya"][c].astype(bool)), (L, c)


@pytest.mark.parametrize("T,L,split", GROUPS)
def test_oracle_samples_match_reference_batches(T, L, split):
    """labels_oracle.sample_targets against the reference's __getitem__ + collate_fn: every mask, sm and label of every sample."""
    g = fixture_b()[0][T, L, split]
    out = g["out"]
    assert sorted(out) == sorted(KEYS + ["start_pos", "end_pos"]) and out["sm"].shape == (len(g["n"]), L, L)
    for b, n in enumerate(g["n"].tolist()):
        ref = LO.sample_targets(float(g["times"][b, 0]), float(g["times"][b, 1]), float(g["duration"][b]), n, T, L)
        for k, v in ref.items():
            v, want = v.numpy(), out[k][b]
            if k in ("ss", "se"):
                assert within_one_spacing(v, want), (b, k)
            elif k == "sm":
                assert same_bits(v, want), (b, k)
            else:
                assert v.shape == want.shape and np.array_equal(v.astype(np.uint8), want), (b, k)
        assert (out["ym"][b] == (out["sm"][b] > f32(0.5))).all() and (out["ys"][b] == (out["ss"][b] > f32(0.5))).all()


@pytest.mark.parametrize("L", LS)
def test_torch_form_matches_reference(L):
    """labels.build_targets on float64 times (2 sigma^2 in double, rounded once): sm bit for bit, labels and masks exactly."""
    g, T = fixture_a()[0][L], T_OF[L]
    nf = nfeats_for(len(g["ts"]), T)
    got = {k: v.numpy() for k, v in V().build_targets(np.stack([g["ts"], g["te"]], 1), g["dur"], nf, T, L).items()}
    check_group(f"labels.build_targets L={L}", g, L, got)
    check_masks(f"labels.build_targets L={L}", got, nf, T, L)


def test_torch_form_fp32_times_behave_as_before():
    """fp32 times keep the fp32 chain for sigma; for fp32-representable times that only moves the denominator's last bit."""
    groups, families, _ = fixture_a()
    g = groups[16]
    pick = g["fam"] == families.index("fp32")
    sub = {k: v[pick] for k, v in g.items()}
    times = torch.from_numpy(np.stack([sub["ts"], sub["te"]], 1)).float()
    got = V().build_targets(times, torch.from_numpy(sub["dur"]).float(), np.full(pick.sum(), 64), 64, 16)
    sigma = (times[:, 1:2] - times[:, 0:1]) / 5.0
    s = torch.arange(16, dtype=torch.float32).unsqueeze(0) * torch.from_numpy(sub["dur"]).float().unsqueeze(1) / 16
    assert torch.equal(got["ss"], torch.exp(-(s - times[:, 0:1]) ** 2 / (2.0 * sigma ** 2)))
    assert same_bits(got["sm"].numpy(), sub["sm"]) and np.array_equal(got["ya"].numpy(), sub["ya"].astype(bool))


# ---------------------------------------------------------------- GPU
def to_numpy(d):
    return {k: v.cpu().numpy() for k, v in d.items()}


@pytest.mark.gpu
@pytest.mark.parametrize("L", LS)
def test_build_targets_hip_matches_reference(dev, L):
    """feeder.build_targets_hip on every case of fixture (a) at this L, one launch: float64 times in (the two_sigma_sq path); the
    fp32-representable block again as fp32 times (the kernel forms the same denominator in double from them)."""
    groups, families, _ = fixture_a()
    g, T = groups[L], T_OF[L]
    n = len(g["ts"])
    nf = nfeats_for(n, T)
    times = torch.from_numpy(np.stack([g["ts"], g["te"]], 1))
    assert times.dtype == torch.float64
    got = to_numpy(V().build_targets_hip(times.to(dev), torch.from_numpy(g["dur"]).to(dev), torch.from_numpy(nf).to(dev), None, T, L, 1))
    check_group(f"build_targets_hip float64 L={L}", g, L, got)
    check_masks(f"build_targets_hip L={L}", got, nf, T, L)
    pick = g["fam"] == families.index("fp32")
    sub = {k: v[pick] for k, v in g.items()}
    got = to_numpy(V().build_targets_hip(times[torch.from_numpy(pick)].float().to(dev), torch.from_numpy(sub["dur"]).float().to(dev),
                                         torch.full((int(pick.sum()),), T, device=dev), None, T, L, 1))
    check_group(f"build_targets_hip fp32 L={L}", sub, L, got)


class Guarded:
    """The outputs of one smin_build_targets call, each with GUARD sentinel elements behind it."""
    SHAPES = dict(video_mask=("T",), query_mask=("Nq",), length_mask=("L",), moment_mask=("L", "L"), sm=("L", "L"), ym=("L", "L"), ss=("L",),
                  ys=("L",), se=("L",), ye=("L",), ya=("L",))

    def __init__(self, dev, B, **dims):
        self.n = {k: B * int(np.prod([dims[d] for d in s])) for k, s in self.SHAPES.items()}
        self.shape = {k: (B,) + tuple(dims[d] for d in s) for k, s in self.SHAPES.items()}
        self.buf = {k: torch.full((n + GUARD,), SENTINEL % 256 if k not in ("sm", "ss", "se") else SENTINEL, device=dev,
                                  dtype=torch.float32 if k in ("sm", "ss", "se") else torch.uint8) for k, n in self.n.items()}

    def ptrs(self, keys):
        return [V()._lib.ptr(self.buf[k]) if k in keys else None for k in self.SHAPES]

    def value(self, k):
        return self.buf[k][:self.n[k]].cpu().numpy().reshape(self.shape[k])

    def untouched(self, k):
        return bool((self.buf[k][:self.n[k]] == (SENTINEL % 256 if self.buf[k].dtype == torch.uint8 else SENTINEL)).all())

    def guards_hold(self):
        return all(bool((b[self.n[k]:] == (SENTINEL % 256 if b.dtype == torch.uint8 else SENTINEL)).all()) for k, b in self.buf.items())


def abi_call(dev, times, dur, nf, ql, B, T, L, Nq, out, keys, den=None):
    p = V()._lib.ptr
    rc = V()._lib.load().smin_build_targets(V()._lib.stream(), p(times), p(dur), p(nf), p(ql), B, T, L, Nq, *out.ptrs(keys), p(den))
    torch.cuda.synchronize(dev)
    return rc


def abi_case(T, L):
    """Five samples (one at L = 512): two-decimal annotations that fp32 cannot hold, nfeats in {0, 1, T, T + 1, 5T}, qlen in
    {0, Nq, Nq + 3}."""
    B = 1 if L == 512 else 5
    ann = np.array([(631.06, 631.41, 673.65), (0.0, 7.83, 30.47), (21.37, 30.47, 30.47), (3.3, 11.9, 17.31), (402.17, 455.09, 760.0)])[:B]
    return B, ann, np.array([T, 0, 1, T + 1, 5 * T], np.int32)[:B]


@pytest.mark.gpu
@pytest.mark.parametrize("T,L,Nq", [(34, 17, 7), (1024, 16, 13), (5, 5, 300), (1024, 512, 20)])
def test_c_abi_with_guard_bands(dev, T, L, Nq):
    """smin_build_targets itself, sentinels behind every output, against the oracle: a ragged second workgroup (L = 17: 289 cells),
    the stride loops over T = 1024 frames and Nq = 300 words from 256 threads, one long-video sample (L = 512: 1024 workgroups).
    Then the masks-only call, B = 0, and the two refusals."""
    B, ann, nf = abi_case(T, L)
    ql = np.array([Nq, 0, Nq + 3, 1, Nq - 1], np.int32)[:B]
    every = set(Guarded.SHAPES)
    d = dict(times=torch.from_numpy(ann[:, :2].astype(np.float32)).contiguous().to(dev), dur=torch.from_numpy(ann[:, 2].astype(np.float32)).to(dev),
             nf=torch.from_numpy(nf).to(dev), ql=torch.from_numpy(ql).to(dev))
    den = torch.from_numpy(denominators(ann[:, 0], ann[:, 1])).to(dev)
    full = Guarded(dev, B, T=T, L=L, Nq=Nq)
    assert abi_call(dev, d["times"], d["dur"], d["nf"], d["ql"], B, T, L, Nq, full, every, den) == 0
    assert full.guards_hold()
    got = {k: full.value(k) for k in every}
    refs = [LO.sample_targets(float(a[0]), float(a[1]), float(a[2]), int(n), T, L) for a, n in zip(ann, nf)]
    for b, ref in enumerate(refs):
        for k, v in ref.items():
            v = v.numpy()
            if k == "sm":
                assert same_bits(got[k][b], v), (b, k)
            elif k not in ("ss", "se"):
                assert np.array_equal(got[k][b].reshape(-1), v.astype(np.uint8).reshape(-1)), (b, k)
    assert np.array_equal(got["query_mask"], (np.arange(Nq)[None, :] < ql[:, None]).astype(np.uint8))
    check_penalties(f"smin_build_targets T={T} L={L}", ann[:, 0], ann[:, 1], ann[:, 2], L, got["ss"], got["se"],
                    np.stack([r["ss"].numpy() for r in refs]), np.stack([r["se"].numpy() for r in refs]))
    # masks only: every target pointer, times and duration NULL
    masks = Guarded(dev, B, T=T, L=L, Nq=Nq)
    mask_keys = {"video_mask", "query_mask", "length_mask", "moment_mask"}
    assert abi_call(dev, None, None, d["nf"], d["ql"], B, T, L, Nq, masks, mask_keys) == 0
    assert masks.guards_hold()
    for k in every:
        assert np.array_equal(masks.value(k), got[k]) if k in mask_keys else masks.untouched(k), k
    # B = 0 writes nothing; T % L != 0 and targets without sm are refused before anything is launched
    idle = Guarded(dev, B, T=T, L=L, Nq=Nq)
    assert abi_call(dev, d["times"], d["dur"], d["nf"], d["ql"], 0, T, L, Nq, idle, every, den) == 0
    assert abi_call(dev, d["times"], d["dur"], d["nf"], d["ql"], B, T + 1, L, Nq, idle, every, den) != 0
    assert abi_call(dev, d["times"], d["dur"], d["nf"], d["ql"], B, T, L, Nq, idle, every - {"sm"}, den) != 0
    assert idle.guards_hold() and all(idle.untouched(k) for k in every)


def check_fed(what, fed, g, L, features=True):
    """A fed batch against the reference's collated batch ``g['out']``."""
    out = g["out"]
    assert list(fed.keys()) == KEYS
    got = to_numpy(fed)
    for k in ("video_features", "query_features") if features else ():
        assert got[k].dtype == np.float32 and same_bits(got[k], out[k]), (what, k)
    for k in ("video_mask", "query_mask", "length_mask", "moment_mask"):
        assert got[k].shape == out[k].shape and np.array_equal(got[k].astype(np.uint8), out[k]), (what, k)
    ref = dict(ts=g["times"][:, 0], te=g["times"][:, 1], dur=g["duration"], sm=out["sm"], ss=out["ss"], se=out["se"], ya=out["ya"])
    for k in ("ym", "ys", "ye"):
        assert np.array_equal(out[k], ref["s" + k[1]] > f32(0.5)), k
    return check_group(what, ref, L, got)


@pytest.mark.gpu
@pytest.mark.parametrize("T,L,split", GROUPS)
def test_feeder_yields_the_reference_batch(dev, T, L, split):
    """BatchFeeder on the inputs the reference's __getitem__ saw (raw rows, token ids, float64 annotations, the drawn start offsets):
    the thirteen entries equal the reference's collated batch; then the host-feature form fed the reference's features."""
    groups, table, pad = fixture_b()
    g = groups[T, L, split]
    Nq, n = g["tokens"].shape[1], g["n"]
    assert g["times"].dtype == np.float64 and not (g["times"].astype(np.float32).astype(np.float64) == g["times"]).all()
    assert (g["spos"] > 0).any() == (split == "train")
    raw = dict(raw_features=list(np.split(g["raw"], np.cumsum(n)[:-1])), tokens=g["tokens"], times=g["times"], duration=g["duration"], spos=g["spos"])
    fed = list(V().BatchFeeder(T, L, Nq, dev, embedding=torch.from_numpy(table).to(dev), pad_id=pad, pool="pick").feed([raw]))
    assert len(fed) == 1
    check_fed(f"BatchFeeder raw form T={T} L={L} {split}", fed[0], g, L)
    host = dict(video_features=g["out"]["video_features"], query_features=g["out"]["query_features"], nfeats=np.minimum(n, T),
                qlen=g["out"]["query_mask"].reshape(len(n), Nq).sum(1), times=g["times"], duration=g["duration"])
    fed = list(V().BatchFeeder(T, L, Nq, dev).feed([host]))
    check_fed(f"BatchFeeder host form T={T} L={L} {split}", fed[0], g, L)


@pytest.mark.gpu
def test_feeder_window_form_matches_reference(dev):
    """Two windows of long videos through BatchFeeder's window form: window_annotations gives exactly the (times_w, duration_w) the
    fixture holds the reference functions' outputs for, and the fed targets equal those outputs."""
    groups, _, win = fixture_a()
    T, L = (int(x) for x in win["TL"])
    tw, dw = V().window_annotations(win["times"], win["duration"], win["n"], win["start"], win["len"], T)
    g = {k: v[win["case"]] for k, v in groups[L].items()}
    assert tw.tobytes() == np.stack([g["ts"], g["te"]], 1).tobytes() and dw.tobytes() == g["dur"].tobytes()
    _, table, pad = fixture_b()
    rng = np.random.default_rng(5)
    videos = [(rng.integers(-512, 513, (int(n), 8)) / 64.0).astype(np.float32) for n in win["n"]]
    tokens = np.array([[1, 2, 3, pad, pad, pad], [4, 5, 6, 7, 8, 9]])
    hb = dict(raw_features=videos, tokens=tokens, times=win["times"], duration=win["duration"], win_start=win["start"], win_len=win["len"])
    fed = list(V().BatchFeeder(T, L, 6, dev, embedding=torch.from_numpy(table).to(dev), pad_id=pad).feed([hb]))[0]
    got = to_numpy(fed)
    check_group("BatchFeeder window form", g, L, got)
    check_masks("BatchFeeder window form", got, np.minimum(win["len"], T), T, L)
    for b in range(2):
        rows = videos[b][win["start"][b]:win["start"][b] + win["len"][b]][:T]
        assert same_bits(got["video_features"][b, :len(rows)], rows) and not got["video_features"][b, len(rows):].any()
