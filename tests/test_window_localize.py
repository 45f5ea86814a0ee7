"""Moment retrieval in videos longer than T over overlapping windows: sampling.window_plan, sample_windows (csrc/sampling.hip),
moments.merge_window_moments (csrc/moments.hip) and SMIN.localize_windows.

The independent references are plain Python: `py_plan` (the window rule as written) and `py_merge` (the spans, candidate order,
IoU and greedy walk of include/smin_hip.h in numpy fp32 scalars).  `merge_window_moments_torch` is checked against `py_merge` on
the CPU; the device kernels are checked against the torch restatements bit for bit."""
import ctypes

import numpy as np
import pytest
import torch

from tests import helpers as H
from tests.support.device import dev  # noqa: F401  (the module's device fixture)
from tests.support.device import vml as V
from tests.support.compare import layout_ok, same_tensor as same
from tests.support.references import merge_frame_edges


def same_merge(got, want):
    for key in ("span", "score", "window", "cell", "count"):
        assert same(got[key], want[key]), key


# ---------------------------------------------------------------- independent references (definition, plain Python)
def py_plan(n, window, stride):
    if n == 0:
        return []
    if n <= window:
        return [(0, n)]
    out, s = [], 0
    while s + window <= n:
        out.append((s, window))
        s += stride
    if out[-1][0] + window < n:
        out.append((n - window, window))
    return out


def py_span(s, n, i, j, T, L):
    f = np.float32
    u = f(max(n, T)) / f(L)
    return f(s) + f(i) * u, min(f(s) + f(j + 1) * u, f(s + n))


def py_iou(a, b):
    f = np.float32
    inter = max(f(0), min(a[1], b[1]) - max(a[0], b[0]))
    uni = max(a[1], b[1]) - min(a[0], b[0])
    with np.errstate(invalid="ignore", divide="ignore"):
        return f(inter) / f(uni)


def py_merge(idx, score, count, start, lens, pair_ptr, T, L, k, thr):
    """[(span, score, window ordinal, (i, j))] kept per pair, from the definition."""
    idx, score, count = idx.numpy(), score.numpy(), count.numpy()
    start, lens, pair_ptr = start.numpy(), lens.numpy(), pair_ptr.numpy()
    t = np.float32(thr)
    out = []
    for b in range(pair_ptr.shape[0] - 1):
        cand = []
        for w, g in enumerate(range(pair_ptr[b], pair_ptr[b + 1])):
            for s in range(int(count[g])):
                cand.append((-float(score[g, s]), w, s, g))           # -0.0 == 0.0: ties fall through to (window, slot)
        cand.sort(key=lambda c: c[:3])
        kept = []
        for _, w, s, g in cand:
            if len(kept) >= k:
                break
            i, j = int(idx[g, s, 0]), int(idx[g, s, 1])
            sp = py_span(int(start[g]), int(lens[g]), i, j, T, L)
            if all(not (py_iou(sp, q[0]) > t) for q in kept):
                kept.append((sp, score[g, s], w, (i, j)))
        out.append(kept)
    return out


def check_py(r, want, k):
    for b, kept in enumerate(want):
        n = len(kept)
        assert int(r["count"][b]) == n
        for q, (sp, sc, w, cell) in enumerate(kept):
            assert np.float32(r["span"][b, q, 0]).tobytes() == sp[0].tobytes() and np.float32(r["span"][b, q, 1]).tobytes() == sp[1].tobytes()
            assert np.float32(r["score"][b, q]).tobytes() == np.float32(sc).tobytes()
            assert int(r["window"][b, q]) == w and tuple(r["cell"][b, q].tolist()) == cell
        assert torch.isnan(r["span"][b, n:]).all() and (r["score"][b, n:] == 0).all()
        assert (r["window"][b, n:] == -1).all() and (r["cell"][b, n:] == -1).all()


def rand_candidates(G, kw, B, T, L, seed, levels=None):
    """Per-window top-k outputs of G windows split over B pairs (some empty), with score ties across windows, -0 / +0, empty
    windows and count < k_window."""
    rng = np.random.default_rng(seed)
    count = rng.integers(0, kw + 1, G).astype(np.int32)
    if G:
        count[rng.integers(0, G, max(G // 5, 1))] = 0
    i = rng.integers(0, L, (G, kw))
    j = np.minimum(i + rng.integers(0, L, (G, kw)), L - 1)
    idx = np.stack([i, j], -1).astype(np.int64)
    vals = np.array([0.75, 0.5, 0.25, 0.0, -0.0, 0.125, 0.9], np.float32) if levels is None else levels
    score = vals[rng.integers(0, vals.shape[0], (G, kw))].astype(np.float32)
    if levels is None:                                                     # half the slots from the tie levels, half distinct
        score = np.where(rng.random((G, kw)) < 0.5, score, rng.random((G, kw)).astype(np.float32)).astype(np.float32)
    slot = np.arange(kw)[None, :] >= count[:, None]
    idx[slot] = -1
    score[slot] = 0
    lens = rng.integers(1, 3 * T + 1, G).astype(np.int32)
    start = rng.integers(0, 4 * T, G).astype(np.int64)
    cuts = np.sort(rng.integers(0, G + 1, B - 1)) if B > 1 else np.zeros(0, np.int64)
    pair_ptr = np.concatenate([[0], cuts, [G]]).astype(np.int64)
    return [torch.from_numpy(x) for x in (idx, score, count, start, lens, pair_ptr)]


# ---------------------------------------------------------------- CPU: the window plan
def test_window_plan_edge_cases():
    S = V().sampling
    W = 64
    cases = {0: [], 5: [(0, 5)], W: [(0, W)], W + 1: [(0, W), (1, W)], 200: [(0, W), (48, W), (96, W), (136, W)]}
    starts, lens, ptr = S.window_plan(list(cases), W, 48)                 # 200 - 64 = 136: stride 48 does not divide it
    assert starts.dtype == torch.int64 and lens.dtype == torch.int32 and ptr.dtype == torch.int64
    assert ptr.tolist() == np.cumsum([0] + [len(v) for v in cases.values()]).tolist()
    for v, (n, want) in enumerate(cases.items()):
        got = list(zip(starts[ptr[v]:ptr[v + 1]].tolist(), lens[ptr[v]:ptr[v + 1]].tolist()))
        assert got == want, n
    # stride > window: gaps are allowed, the last window still ends at n
    s, ln, p = S.window_plan(torch.tensor([250]), 32, 100)
    assert list(zip(s.tolist(), ln.tolist())) == [(0, 32), (100, 32), (200, 32), (218, 32)]
    s, ln, p = S.window_plan(np.zeros(0, np.int64), 8, 4)
    assert s.numel() == 0 and ln.numel() == 0 and p.tolist() == [0]
    for bad in (dict(window=0, stride=1), dict(window=4, stride=0)):
        with pytest.raises(ValueError):
            S.window_plan([10], **bad)
    with pytest.raises(ValueError):
        S.window_plan([1 << 24], 8, 4)
    with pytest.raises(ValueError):
        S.window_plan([-1], 8, 4)


def test_window_plan_covers_every_row():
    S = V().sampling
    rng = np.random.default_rng(3)
    for window in (1, 7, 16, 64):
        for stride in sorted({1, max(window // 2, 1), window, window + 3}):
            n = rng.integers(0, 6 * window + 5, 12)
            n[:3] = [0, window, window + 1]
            starts, lens, ptr = S.window_plan(n, window, stride)
            for v in range(n.shape[0]):
                got = list(zip(starts[ptr[v]:ptr[v + 1]].tolist(), lens[ptr[v]:ptr[v + 1]].tolist()))
                assert got == py_plan(int(n[v]), window, stride)
                if n[v]:
                    assert got[-1][0] + got[-1][1] == n[v] and got[0][0] == 0          # the last window ends at n
                    assert all(a[0] < b[0] for a, b in zip(got, got[1:]))
                    if stride <= window:
                        cover = np.zeros(int(n[v]), bool)
                        for s, m in got:
                            cover[s:s + m] = True
                        assert cover.all()


# ---------------------------------------------------------------- CPU: the merge restatement against the definition
@pytest.mark.parametrize("G,kw,B,k,thr,seed", [(1, 1, 1, 1, 0.5, 0), (12, 5, 3, 5, 0.5, 1), (40, 8, 6, 10, 0.3, 2),
                                               (30, 10, 4, 64, 0.7, 3), (25, 6, 5, 7, 1.0, 4), (20, 4, 4, 3, 0.0, 5),
                                               (0, 5, 3, 5, 0.5, 6)])
def test_merge_torch_equals_python_greedy(G, kw, B, k, thr, seed):
    M = V().moments
    T, L = 32, 8
    args = rand_candidates(G, kw, B, T, L, seed)
    r = M.merge_window_moments_torch(*args, T, L, k=k, nms_thresh=thr)
    check_py(r, py_merge(*args, T, L, k, thr), k)
    if thr >= 1:                                                        # no suppression: the k best candidates
        for b in range(B):
            assert int(r["count"][b]) == min(k, int(args[2][args[5][b]:args[5][b + 1]].sum()))


def test_merge_ties_across_windows_and_signed_zero():
    M = V().moments
    T, L = 16, 4
    # two windows of one pair, every score equal (+0 in the first, -0 in the second): window 0's slots come first, then window 1's
    idx = torch.tensor([[[0, 0], [1, 1]], [[2, 3], [0, 1]]])
    score = torch.tensor([[0.0, 0.0], [-0.0, -0.0]])
    count = torch.tensor([2, 2], dtype=torch.int32)
    start, lens = torch.tensor([0, 100]), torch.tensor([16, 16], dtype=torch.int32)
    r = M.merge_window_moments_torch(idx, score, count, start, lens, torch.tensor([0, 2]), T, L, k=4, nms_thresh=0.5)
    assert r["window"][0].tolist() == [0, 0, 1, 1] and r["cell"][0].tolist() == [[0, 0], [1, 1], [2, 3], [0, 1]]
    # spans in raw rows: u = max(16, T) / L = 4, start 100 for window 1
    assert r["span"][0].tolist() == [[0.0, 4.0], [4.0, 8.0], [108.0, 116.0], [100.0, 108.0]]
    check_py(r, py_merge(idx, score, count, start, lens, torch.tensor([0, 2]), T, L, 4, 0.5), 4)


def test_merge_refusals_on_the_host_and_the_c_abi():
    import models
    M = V().moments
    args = rand_candidates(4, 3, 2, 16, 4, 0)
    for k in (0, 65):
        with pytest.raises(ValueError):
            M.merge_window_moments_torch(*args, 16, 4, k=k)
    with pytest.raises(models.vml_amd._lib.SminHipError):
        M.merge_window_moments(*args, 16, 4, k=5)                          # CPU tensors: no fallback
    lib = models.vml_amd._lib.load()
    buf = (ctypes.c_byte * 4096)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    f = lib.smin_merge_window_moments

    def run(G=2, B=1, T=16, L=4, kw=3, k=5, ptrs=None):                  # 6 input and 5 output pointers
        ptrs = ptrs or [p] * 11
        return f(None, *ptrs[:6], G, B, T, L, kw, k, 0.5, *ptrs[6:])
    # refused before anything is launched (host memory here: a launch would fault)
    assert run(k=0) < 0 and run(k=65) < 0 and run(kw=0) < 0 and run(kw=65) < 0 and run(T=0) < 0 and run(L=0) < 0
    assert run(G=-1) < 0 and run(B=-1) < 0
    for q in range(11):
        ptrs = [p] * 11
        ptrs[q] = None
        assert run(ptrs=ptrs) < 0, q                                     # a NULL pointer with B = 1, G = 2
    assert run(B=0, ptrs=[None] * 11) == 0                               # B = 0: a no-op


def test_localize_windows_refuses_bad_arguments_on_the_host():
    import models
    m = models.SMIN(32, 16, 4, 64, 32, 2, 48, 7, 32)
    raw, qf, qm = torch.zeros(40, 48), torch.zeros(1, 7, 300), torch.ones(1, 7, dtype=torch.uint8)
    for kw in (dict(k=0), dict(k=65), dict(k_window=0), dict(k_window=65), dict(window=0), dict(stride=0), dict(max_batch=0)):
        with pytest.raises(ValueError):
            m.localize_windows(raw, [40], qf, qm, **kw)
    with pytest.raises(models.vml_amd._lib.SminHipError, match="no CPU fallback"):
        m.localize_windows(raw, [40], qf, qm)


# ---------------------------------------------------------------- GPU
@pytest.mark.gpu
@pytest.mark.parametrize("Din,T", [(4, 16), (500, 64), (500, 7)])
@pytest.mark.parametrize("mode", ["pick", "mean"])
def test_sample_windows_bit_exact(dev, Din, T, mode):
    S = V().sampling
    rng = np.random.default_rng(Din + T)
    R = 5 * T + 11
    raw = torch.randn(R, Din, generator=torch.Generator().manual_seed(T))
    lens = [1, T // 2 + 1, T, T + 1, 2 * T + 3, 4 * T + 5, T, T]            # len < T, == T, > T
    begins = [0, 3, 0, R - T - 1, 5, 2, 0, 0]                              # overlapping and repeated ranges
    lens += rng.integers(1, 3 * T, 8).tolist()
    begins += [int(rng.integers(0, R - n + 1)) for n in lens[8:]]
    got, nf = S.sample_windows(raw.to(dev), begins, lens, T, mode=mode)
    want, nfw = S.sample_windows_torch(raw, begins, lens, T, mode=mode)
    assert same(got, want) and same(nf, nfw)
    # each window is sample_clips of its rows, and device-resident ranges give the same result
    for w in (0, 4, 5):
        one, _ = S.sample_clips_torch(raw[begins[w]:begins[w] + lens[w]], [lens[w]], T, mode=mode)
        assert same(got[w:w + 1], one)
    got_d, _ = S.sample_windows(raw.to(dev), torch.tensor(begins, device=dev), torch.tensor(lens, device=dev, dtype=torch.int32), T, mode=mode)
    assert same(got_d, want)
    with pytest.raises(ValueError):
        S.sample_windows(raw.to(dev), [R - 3], [4], T)                    # past the end of raw
    e, ne = S.sample_windows(raw.to(dev), [], [], T)
    assert e.shape == (0, T, Din) and ne.shape == (0,)


@pytest.mark.gpu
@pytest.mark.parametrize("G,kw,B,k,thr,seed", [(64, 5, 8, 1, 0.5, 0), (64, 5, 8, 64, 0.5, 1), (200, 16, 9, 10, 0.3, 2),
                                               (90, 8, 12, 5, 1.0, 3), (0, 4, 3, 5, 0.5, 4), (4, 2, 3, 3, 0.5, "frame edges")])
def test_merge_on_device_equals_torch(dev, G, kw, B, k, thr, seed):
    M = V().moments
    if seed == "frame edges":                                              # pair_ptr outside [0, G], a pair and a window with nothing
        T, L = 8, 8
        args = list(merge_frame_edges())
        assert tuple(args[0].shape) == (G, kw, 2) and args[5].shape[0] == B + 1
    else:
        T, L = 64, 16
        args = rand_candidates(G, kw, B, T, L, seed)
        args[5][1] = args[5][0]                                            # pair 0 has zero windows
    got = M.merge_window_moments(*[a.to(dev) for a in args], T, L, k=k, nms_thresh=thr)
    want = M.merge_window_moments_torch(*args, T, L, k=k, nms_thresh=thr)
    same_merge(got, want)                                                  # bit for bit, the NaN of the empty spans included
    if seed == "frame edges":
        assert want["count"].tolist() == [2, 0, 2] and torch.equal(want["span"][1].view(torch.int32), torch.full((3, 2), 0x7FC00000, dtype=torch.int32))


@pytest.mark.gpu
@pytest.mark.parametrize("k,thr", [(64, 0.5), (64, 0.95), (5, 0.3)])
def test_merge_on_device_many_candidates(dev, k, thr):
    """A pair with more than 5 000 candidates (100 windows of 64), ties included, beside a pair with few and one with none."""
    M = V().moments
    T, L = 256, 64
    levels = (np.arange(40, dtype=np.float32) / 40).astype(np.float32)
    idx, score, count, start, lens, _ = rand_candidates(130, 64, 1, T, L, 11, levels=levels)
    count[:100] = 64
    rng = np.random.default_rng(5)
    i = torch.from_numpy(rng.integers(0, L, (100, 64)))
    idx[:100] = torch.stack([i, torch.minimum(i + torch.from_numpy(rng.integers(0, 8, (100, 64))), torch.tensor(L - 1))], -1)
    score[:100] = torch.from_numpy(levels[rng.integers(0, 40, (100, 64))])
    start[:100] = torch.arange(100) * 128
    lens[:100] = 256
    pair_ptr = torch.tensor([0, 100, 100, 130])
    args = (idx, score, count, start, lens, pair_ptr)
    assert int(count[:100].sum()) > 5000
    got = M.merge_window_moments(*[a.to(dev) for a in args], T, L, k=k, nms_thresh=thr)
    same_merge(got, M.merge_window_moments_torch(*args, T, L, k=k, nms_thresh=thr))


SMALL = (32, 16, 4, 64, 32, 2, 48, 7, 32)             # T, L, C, D, dl, layers, Din, Nq, H


def _model(shape, dev, gain=1.2):
    from oracle import smin_oracle as O                # test infrastructure: the formula weights only
    import models
    T, L, C, D, dl, layers, Din, Nq, Hh = shape
    m = models.SMIN(T, L, C, D, dl, layers, Din, Nq, Hh, dev)
    m.load_state_dict(O.formula_state_dict(H.smin_shapes(T, L, C, D, dl, layers, Din, Nq, Hh), gain=gain))
    return m.to(dev)


def restate(m, raw, lengths, qf, qm, video_index, window, stride, k, k_window, thr, mode, max_batch):
    """localize_windows spelled out with the same chunking: sample_windows_torch -> masks -> the model's forward -> top_moments ->
    merge_window_moments_torch (all host-side bookkeeping in plain Python)."""
    api = V()
    T, L = m.T, m.L
    dev = qf.device
    starts, lens, vptr = (x.tolist() for x in api.window_plan(lengths, window, stride))
    offs = np.concatenate([[0], np.cumsum(lengths)]).tolist()
    wins = [(b, offs[v] + starts[g], starts[g], lens[g]) for b, v in enumerate(video_index) for g in range(vptr[v], vptr[v + 1])]
    idx, score, count = [], [], []
    for c0 in range(0, len(wins), max_batch):
        chunk = wins[c0:c0 + max_batch]
        vf, nf = api.sample_windows_torch(raw.cpu(), [w[1] for w in chunk], [w[3] for w in chunk], T, mode=mode)
        g = len(chunk)
        masks = api.build_targets(torch.zeros(g, 2), torch.ones(g), nf, T, L, device=dev)
        rows = torch.tensor([w[0] for w in chunk], device=dev)
        with torch.no_grad():
            pm, ps, pe, _ = m(vf.to(dev), masks["video_mask"], qf[rows], qm[rows], masks["length_mask"], masks["moment_mask"])
            r = api.top_moments(pm, ps, pe, masks["moment_mask"], k=k_window, nms_thresh=thr)
        idx.append(r["idx"].cpu()), score.append(r["score"].cpu()), count.append(r["count"].cpu())
    G = len(wins)
    cat = lambda xs, shape, dt: torch.cat(xs) if xs else torch.zeros(shape, dtype=dt)
    pair_ptr = np.searchsorted([w[0] for w in wins], np.arange(len(video_index) + 1), side="left")
    return api.merge_window_moments_torch(cat(idx, (0, k_window, 2), torch.int64), cat(score, (0, k_window), torch.float32),
                                          cat(count, (0,), torch.int32), torch.tensor([w[2] for w in wins], dtype=torch.int64).reshape(G),
                                          torch.tensor([w[3] for w in wins], dtype=torch.int32).reshape(G), torch.from_numpy(pair_ptr.astype(np.int64)),
                                          T, L, k=k, nms_thresh=thr)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["pick", "mean"])
def test_localize_windows_end_to_end(dev, mode):
    T = SMALL[0]
    m = _model(SMALL, dev)
    lengths = [0, 5, T, T + 1, 3 * T + 7]
    g = torch.Generator().manual_seed(4)
    raw = torch.randn(sum(lengths), SMALL[6], generator=g)
    video_index = [4, 1, 4, 3, 2, 0]                                       # 2 queries on the long video, one on the empty one
    qf = torch.randn(6, SMALL[7], 300, generator=g)
    qm = (torch.arange(SMALL[7]).unsqueeze(0) < torch.tensor([7, 3, 5, 1, 6, 2]).unsqueeze(1)).to(torch.uint8)
    dur = torch.tensor([60.0, 3.5, 40.0, 21.0, 9.0, 1.0])
    for window, stride, max_batch, k, kw, thr in ((None, None, 4, 5, None, 0.5), (20, 7, 3, 8, 3, 0.3), (T, T, 64, 1, 1, 0.5)):
        got = m.localize_windows(raw.to(dev), lengths, qf.to(dev), qm.to(dev), video_index=video_index, window=window, stride=stride,
                                 k=k, k_window=kw, nms_thresh=thr, mode=mode, duration=dur.to(dev), max_batch=max_batch)
        w = T if window is None else window
        want = restate(m, raw, lengths, qf.to(dev), qm.to(dev), video_index, w, max(w // 2, 1) if stride is None else stride, k,
                       k if kw is None else kw, thr, mode, max_batch)
        same_merge(got, want)
        n_rows = torch.tensor([lengths[v] for v in video_index], dtype=torch.float32)
        nw = torch.tensor([len(py_plan(lengths[v], w, max(w // 2, 1) if stride is None else stride)) for v in video_index])
        assert torch.equal(got["n_windows"].cpu(), nw)
        assert same(got["times"], (want["span"] * dur.view(-1, 1, 1)) / n_rows.view(-1, 1, 1))
        assert int(got["n_windows"][5]) == 0 and int(got["count"][5]) == 0                    # the empty video: no window, no moment
        assert torch.isnan(got["times"][5]).all() and (got["window"][5] == -1).all()
        assert layout_ok(dev)


@pytest.mark.gpu
def test_localize_windows_short_video_equals_localize(dev):
    """n <= window: one window of the whole video, so the result is SMIN.localize on sample_clips of it, bit for bit.  n is a
    multiple of T / L, so no cell's span is clipped at n and the span IoU equals top_moments' cell IoU."""
    T, L = SMALL[0], SMALL[1]
    m = _model(SMALL, dev)
    api = V()
    g = torch.Generator().manual_seed(9)
    for n in (T, T - 2 * (T // L), 6):
        raw = torch.randn(n, SMALL[6], generator=g).to(dev)
        qf = torch.randn(1, SMALL[7], 300, generator=g).to(dev)
        qm = torch.ones(1, SMALL[7], dtype=torch.uint8, device=dev)
        got = m.localize_windows(raw, [n], qf, qm, k=5, nms_thresh=0.5)
        vf, nf = api.sample_clips(raw, [n], T)
        masks = api.build_masks_hip(nf, T, L)
        want = m.localize(vf, masks["video_mask"], qf, qm, masks["length_mask"], masks["moment_mask"], k=5, nms_thresh=0.5)
        assert same(got["cell"], want["idx"]) and same(got["score"], want["score"]) and same(got["count"], want["count"])
        assert (got["window"][0, :int(want["count"][0])] == 0).all()
        assert layout_ok(dev)


@pytest.mark.gpu
def test_localize_windows_full_width(dev):
    """The charades width (T = 64, L = 16, D = 512, dl = 128, H = 256, 3 layers): a 2 000-row video at stride 16, two queries,
    244 windows in six chunks."""
    shape = (64, 16, 4, 512, 128, 3, 500, 13, 256)
    m = _model(shape, dev, gain=1.3)
    g = torch.Generator().manual_seed(21)
    raw = torch.randn(2000, shape[6], generator=g)
    qf = torch.randn(2, shape[7], 300, generator=g)
    qm = (torch.arange(shape[7]).unsqueeze(0) < torch.tensor([[13], [6]])).to(torch.uint8)
    got = m.localize_windows(raw.to(dev), [2000], qf.to(dev), qm.to(dev), video_index=[0, 0], stride=16, k=5, max_batch=48)
    assert got["n_windows"].tolist() == [122, 122]
    want = restate(m, raw, [2000], qf.to(dev), qm.to(dev), [0, 0], 64, 16, 5, 5, 0.5, "pick", 48)
    same_merge(got, want)
    assert got["count"].tolist() == [5, 5]
    assert layout_ok(dev)


@pytest.mark.gpu
def test_localize_windows_refusals_on_device_tensors(dev):
    m = _model(SMALL, dev)
    raw = torch.zeros(40, SMALL[6], device=dev)
    qf, qm = torch.zeros(2, SMALL[7], 300, device=dev), torch.ones(2, SMALL[7], dtype=torch.uint8, device=dev)
    with pytest.raises(ValueError, match="video_index"):
        m.localize_windows(raw, [10, 30], qf, qm, video_index=[0, 2])
    with pytest.raises(ValueError, match="one to one"):
        m.localize_windows(raw, [40], qf, qm)
    with pytest.raises(ValueError, match="Din"):
        m.localize_windows(torch.zeros(40, SMALL[6] - 2, device=dev), [40], qf[:1], qm[:1])
    with pytest.raises(ValueError, match="sum to"):
        m.localize_windows(raw, [10, 20], qf, qm)
    r = m.localize_windows(raw[:0], [], qf[:0], qm[:0])                   # no pair: empty results
    assert r["span"].shape == (0, 5, 2) and r["count"].shape == (0,)
