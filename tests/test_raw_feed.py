"""Clip resampling and word-vector lookup on the device (sampling.py, csrc/sampling.hip) and BatchFeeder's raw batch form.

The pick rule is pinned to the reference's own ``get_fixed_length_features`` through g8_clip_sampling.npz
(tests/golden/make_golden_sampling.py); ``clip_indices`` / ``sample_clips_torch`` are checked against it on the CPU and the
device kernels against ``sample_clips_torch``, bit for bit."""
import os

import numpy as np
import pytest
import torch

from tests import helpers as H
from tests.support.device import dev  # noqa: F401  (the module's device fixture)
from tests.support.device import vml as V
from tests.support.compare import same_tensor as same


def fixture():
    z = np.load(os.path.join(H.GOLDEN, "g8_clip_sampling.npz"))
    return {k: z[k] for k in z.files}


# ---------------------------------------------------------------- CPU: the rule against the reference's fixture
def test_clip_indices_match_reference_fixture():
    z, S = fixture(), V().sampling
    assert len(z["n"]) > 400 and z["train"].sum() > 0 and (z["spos"] > 0).sum() > 50
    for c in range(len(z["n"])):
        n, T, sp = int(z["n"][c]), int(z["T"][c]), int(z["spos"][c])
        want = z["idx"][z["ptr"][c]:z["ptr"][c + 1]]
        assert int(z["nfeats"][c]) == min(n, T) == want.shape[0]
        assert 0 <= sp < int(S.spos_high(n, T)), (n, T, sp)                 # the reference drew inside the documented range
        assert np.array_equal(S.clip_indices(n, T, sp), want), (n, T, sp, bool(z["train"][c]))


@pytest.mark.parametrize("T", [16, 64, 128, 256, 1024])
def test_sample_clips_torch_matches_reference_fixture(T):
    """Every (n, split) case of one T as one batch: features whose column 0 is the row number, so the output's column 0 is the
    picked rows; rows past nfeats are zero."""
    z, S = fixture(), V().sampling
    cases = np.nonzero(z["T"] == T)[0]
    n = z["n"][cases]
    raw = [np.stack([np.arange(k, dtype=np.float32), np.full(k, 7, np.float32), np.zeros(k, np.float32), -np.arange(k, dtype=np.float32)], 1)
           for k in n]
    vf, nf = S.sample_clips_torch(raw, None, T, spos=z["spos"][cases])
    assert vf.shape == (len(cases), T, 4) and nf.dtype == torch.int32
    for r, c in enumerate(cases):
        want = z["idx"][z["ptr"][c]:z["ptr"][c + 1]]
        k = want.shape[0]
        assert int(nf[r]) == k
        assert np.array_equal(vf[r, :k, 0].numpy(), want.astype(np.float32)) and np.array_equal(vf[r, :k, 3].numpy(), -want.astype(np.float32))
        assert (vf[r, :k, 1] == 7).all() and (vf[r, k:] == 0).all()


def test_draw_offsets_range():
    S = V().sampling
    rng = np.random.default_rng(3)
    for T in (16, 256):
        for n in (0, 1, T - 1, T, T + 1, 2 * T, 2 * T + 1, (3 * T) // 2, (5 * T) // 2, 3 * T, 7 * T + 5, 20 * T):
            hi = int(S.spos_high(n, T))
            # the reference's own range (dataset.py:45-49), restated in Python floats
            stride = 1.0 if n <= T else n * 1.0 / T
            r = -0.5 + stride
            r = r - 1.0 if r == np.floor(r) else r
            assert hi == int(r + 1) >= 1, (n, T)
            d = S.draw_offsets(np.full(4000, n), T, rng)
            assert d.dtype == np.int32 and set(d.tolist()) == set(range(hi)), (n, T, hi)
    z = fixture()                                                            # every offset the reference drew is in the range
    assert (z["spos"] < S.spos_high(z["n"], z["T"])).all()


def test_mean_mode_hand_cases():
    S = V().sampling
    # (n, T, window edges worked out by hand: a_t = rint(t * n / T), half to even)
    for n, T, edges in [(7, 3, [0, 2, 5, 7]), (5, 2, [0, 2, 5]), (3, 2, [0, 2, 3]), (10, 4, [0, 2, 5, 8, 10]), (9, 2, [0, 4, 9]),
                        (64, 16, list(range(0, 65, 4)))]:
        assert S.mean_windows(n, T).tolist() == edges
        x = np.random.default_rng(n * 100 + T).standard_normal((n, 8)).astype(np.float32)
        want = np.zeros((T, 8), np.float32)
        for t in range(T):
            acc = x[edges[t]].copy()
            for r in range(edges[t] + 1, edges[t + 1]):
                acc = (acc + x[r]).astype(np.float32)
            want[t] = acc / np.float32(edges[t + 1] - edges[t])
        vf, nf = S.sample_clips_torch([x], None, T, mode="mean")
        assert int(nf[0]) == T and np.array_equal(vf[0].numpy().view(np.int32), want.view(np.int32)), (n, T)
    x = np.arange(20, dtype=np.float32).reshape(5, 4)                         # n <= T: mean is pick
    vm, _ = S.sample_clips_torch([x], None, 8, mode="mean")
    vp, _ = S.sample_clips_torch([x], None, 8)
    assert same(vm, vp) and (vm[0, 5:] == 0).all()


def test_host_side_checks():
    S = V().sampling
    x = np.zeros((10, 4), np.float32)
    with pytest.raises(ValueError, match="outside"):
        S.sample_clips_torch([x], None, 4, spos=[3])                          # n = 10, T = 4: stride 2.5, r = 2 -> spos in {0, 1}
    with pytest.raises(ValueError, match="mean"):
        S.sample_clips_torch([x], None, 4, spos=[1], mode="mean")
    with pytest.raises(V()._lib.SminHipError):
        S.sample_clips(torch.zeros(10, 4), [10], 4)
    with pytest.raises(V()._lib.SminHipError):
        S.embed_tokens(torch.zeros(2, 3, dtype=torch.int32), torch.zeros(5, 8))
    tab = torch.randn(6, 8)
    qf, qm, ql = S.embed_tokens_torch(torch.tensor([[0, 4, 5, -1], [6, 1, 5, 5]]), tab)
    assert same(qf[0, :3], tab[[0, 4, 5]]) and (qf[0, 3] == 0).all() and (qf[1, 0] == 0).all()
    assert qm.tolist() == [[1, 1, 0, 0], [0, 1, 0, 0]] and ql.tolist() == [2, 1]


# ---------------------------------------------------------------- GPU
def mixed_lengths(B, T, rng):
    """n = 0, n >> T, n < T, n = T, n = T + 1, then draws from [0, 4T]."""
    base = [0, 13 * T + 7, max(T // 3, 1), T, T + 1, 2 * T, (5 * T) // 2]
    return np.array((base + rng.integers(0, 4 * T + 1, max(B - len(base), 0)).tolist())[:B], dtype=np.int64)


@pytest.mark.gpu
@pytest.mark.parametrize("Din,T,B", [(4, 1024, 64), (500, 256, 64), (1024, 64, 33), (4096, 16, 7), (4096, 256, 3), (500, 16, 1), (4, 64, 2)])
def test_sample_clips_pick_bit_exact(dev, Din, T, B):
    S = V().sampling
    rng = np.random.default_rng(Din + T + B)
    n = mixed_lengths(B, T, rng)
    raw = torch.randn(int(n.sum()), Din, generator=torch.Generator().manual_seed(B))
    spos = S.draw_offsets(n, T, rng)
    if B > 1:
        spos[1] = S.spos_high(n[1], T) - 1                                  # the largest offset the reference draws
    for sp in (None, spos):
        got, nf = S.sample_clips(raw.to(dev), n, T, spos=sp)
        want, nfw = S.sample_clips_torch(raw, n, T, spos=sp)
        assert same(got, want) and same(nf, nfw)
    # the list form and device-resident offsets and start offsets give the same result
    parts = list(torch.split(raw.to(dev), n.tolist()))
    got_l, _ = S.sample_clips(parts, None, T, spos=spos)
    offs = torch.from_numpy(np.concatenate([[0], np.cumsum(n)])).to(dev)
    got_d, _ = S.sample_clips(raw.to(dev), offs, T, spos=torch.from_numpy(spos).to(dev))
    assert same(got_l, want) and same(got_d, want)


@pytest.mark.gpu
@pytest.mark.parametrize("Din,T,B", [(4, 1024, 16), (500, 256, 64), (1024, 64, 9), (4096, 16, 8)])
def test_sample_clips_mean_bit_exact(dev, Din, T, B):
    S = V().sampling
    rng = np.random.default_rng(7 * Din + T)
    n = mixed_lengths(B, T, rng)
    raw = torch.randn(int(n.sum()), Din, generator=torch.Generator().manual_seed(T))
    got, nf = S.sample_clips(raw.to(dev), n, T, mode="mean")
    want, nfw = S.sample_clips_torch(raw, n, T, mode="mean")
    assert same(got, want) and same(nf, nfw)


@pytest.mark.gpu
def test_sample_clips_rejects_and_no_ops(dev):
    S = V().sampling
    raw = torch.randn(30, 8, device=dev)
    with pytest.raises(ValueError, match="outside"):
        S.sample_clips(raw, [10, 20], 4, spos=[0, 5])                        # n = 20, T = 4: stride 5, spos in [0, 4]
    with pytest.raises(ValueError):
        S.sample_clips(raw[:, :6], [10, 20], 4)                             # Din % 4 != 0
    vf, nf = S.sample_clips(torch.zeros(0, 8, device=dev), np.zeros(0, np.int64), 4)
    assert vf.shape == (0, 4, 8) and nf.shape == (0,)
    # an out-of-range device spos is clamped into the reference's range: it never reads past the sample
    offs = torch.tensor([0, 10, 30], device=dev)
    got, _ = S.sample_clips(raw, offs, 4, spos=torch.tensor([1000, -3], device=dev, dtype=torch.int32))
    want, _ = S.sample_clips_torch(raw.cpu(), [10, 20], 4, spos=[1, 0])
    assert same(got, want)


@pytest.mark.gpu
def test_embed_tokens_bit_exact(dev):
    S = V().sampling
    g = torch.Generator().manual_seed(11)
    Vn, E, B, Nq = 1002, 300, 37, 20
    table = torch.cat([torch.randn(Vn - 2, E, generator=g), torch.zeros(2, E)])     # GloVe + <unk> + <pad>, the reference's layout
    tok = torch.randint(0, Vn - 2, (B, Nq), generator=g)
    ql = torch.randint(0, Nq + 1, (B,), generator=g)
    tok[torch.arange(Nq).unsqueeze(0) >= ql.unsqueeze(1)] = Vn - 1             # <pad> after each query
    tok[3, 0], tok[4, 1] = Vn - 2, Vn - 2                                       # <unk>
    got = S.embed_tokens(tok.to(dev), table.to(dev))
    assert same(got[0], table[tok]) and same(got[1], (tok < Vn - 1).to(torch.uint8)) and same(got[2], (tok < Vn - 1).sum(1, dtype=torch.int32))
    bad = tok.clone()
    bad[0, 0], bad[1, 2], bad[2, 5] = -1, Vn, 2 ** 31 - 1                       # out of range: zero row, mask 0, never read
    got = S.embed_tokens(bad.to(dev), table.to(dev))
    want = S.embed_tokens_torch(bad, table)
    assert all(same(a, b) for a, b in zip(got, want))
    assert (got[0][0, 0] == 0).all() and int(got[1][0, 0]) == 0 and int(got[1][1, 2]) == 0
    got = S.embed_tokens(tok.to(dev), table.to(dev), pad_id=Vn - 2)          # an explicit pad id
    assert same(got[1], (tok < Vn - 2).to(torch.uint8))


@pytest.mark.gpu
def test_sample_clips_64bit_addressing(dev):
    """The last sample starts past 2^31 elements of raw (an ~8.7 GB buffer filled on the device); a few rows are checked."""
    S = V().sampling
    Din, T = 4096, 256
    n0 = (1 << 31) // Din + 1000
    n1 = 3001
    raw = torch.empty(n0 + n1, Din, device=dev)
    start = n0
    assert start * Din > 2 ** 31
    raw[:start].fill_(1.5)
    raw[start:].copy_(torch.arange(n1, device=dev, dtype=torch.float32).unsqueeze(1) + torch.arange(Din, device=dev) / Din)
    spos = np.array([0, int(S.spos_high(n1, T)) - 1], dtype=np.int32)
    got, nf = S.sample_clips(raw, np.array([n0, n1]), T, spos=spos)
    idx = torch.from_numpy(S.clip_indices(n1, T, spos[1])).to(dev)
    assert nf.tolist() == [T, T] and torch.equal(got[1], raw[start + idx]) and (got[0] == 1.5).all()
    assert int(idx[-1]) > n1 - 20 and int(got[1, -1, 0]) == int(idx[-1])
    del raw, got
    torch.cuda.empty_cache()


def make_samples(B, T, Nq, Din, Vn, rng, g):
    n = rng.integers(1, 4 * T + 1, B)
    if B >= 4:
        n[:4] = [T, T + 1, max(T // 2, 1), 9 * T + 3]
    raws = [torch.randn(int(k), Din, generator=g).numpy() for k in n]
    ql = rng.integers(1, Nq + 1, B)
    tok = rng.integers(0, Vn - 1, (B, Nq))
    tok[np.arange(Nq)[None, :] >= ql[:, None]] = Vn - 1
    dur = torch.rand(B, generator=g) * 100 + 5
    ts = torch.rand(B, generator=g) * dur * 0.5
    te = ts + 1.0 + torch.rand(B, generator=g) * (dur - ts - 1.0).clamp(min=0)
    return dict(raw_features=raws, tokens=tok, times=torch.stack([ts, te], 1), duration=dur, spos=None), n


@pytest.mark.gpu
@pytest.mark.parametrize("pool", ["pick", "mean"])
def test_feeder_raw_path_equals_host_path(dev, pool):
    """The same samples through the raw batch form and through today's form (host-side resampling and lookup by the
    restatements): all thirteen yielded tensors are bit-identical batch after batch, across slot reuse, and one SMIN forward
    on each gives bit-identical scores."""
    import models
    T, L, Nq, Din, B, Vn = 64, 16, 9, 40, 6, 53
    rng, g = np.random.default_rng(21), torch.Generator().manual_seed(21)
    table = torch.cat([torch.randn(Vn - 2, 300, generator=g), torch.zeros(2, 300)])
    raws, hosts = [], []
    for s in range(6):
        rb, n = make_samples(B, T, Nq, Din, Vn, rng, g)
        if pool == "pick":
            rb["spos"] = V().draw_offsets(n, T, rng)
        if s % 2:                                                           # the packed form
            rb["raw_lengths"], rb["raw_features"] = n, np.concatenate(rb["raw_features"], 0)
        vf, nf = V().sample_clips_torch(rb["raw_features"], n if s % 2 else None, T, spos=rb["spos"], mode=pool)
        tok = torch.from_numpy(rb["tokens"])
        hosts.append(dict(video_features=vf.numpy(), query_features=table[tok], nfeats=nf, qlen=(tok < Vn - 1).sum(1),
                          times=rb["times"], duration=rb["duration"]))
        if rb["spos"] is None:
            del rb["spos"]
        if s in (3, 5):                                                     # pinned packed rows: the feeder reads them in place
            rb["raw_features"] = torch.from_numpy(rb["raw_features"]).pin_memory()
        raws.append(rb)
    m = models.SMIN(T, L, 4, 64, 32, 2, Din, Nq, 32, dev).to(dev)
    outs = {}
    for name, feeder, batches in (("raw", V().BatchFeeder(T, L, Nq, dev, embedding=table.to(dev), pool=pool), raws),
                                  ("host", V().BatchFeeder(T, L, Nq, dev), hosts)):
        outs[name] = []
        for i, fed in enumerate(feeder.feed(batches)):
            assert list(fed.keys()) == ["video_features", "video_mask", "query_features", "query_mask", "length_mask", "moment_mask",
                                        "sm", "ym", "ss", "ys", "se", "ye", "ya"]
            got = {k: v.clone() for k, v in fed.items()}
            if i == 0:
                with torch.no_grad():
                    got["scores"] = [x.clone() for x in m(*H.model_inputs(fed))]
            outs[name].append(got)
    assert len(outs["raw"]) == len(outs["host"]) == 6
    for a, b in zip(outs["raw"], outs["host"]):
        for k in b:
            if k == "scores":
                assert all(same(x, y) for x, y in zip(a[k], b[k]))
            else:
                assert same(a[k], b[k]), k


@pytest.mark.gpu
def test_feeder_raw_form_checks(dev):
    T, L, Nq, Din, B, Vn = 16, 4, 5, 8, 3, 12
    rng, g = np.random.default_rng(2), torch.Generator().manual_seed(2)
    table = torch.randn(Vn, 300).to(dev)
    rb, n = make_samples(B, T, Nq, Din, Vn, rng, g)
    del rb["spos"]
    with pytest.raises(ValueError, match="embedding"):
        list(V().BatchFeeder(T, L, Nq, dev).feed([rb]))
    tok = rb["tokens"].copy()
    tok[1, 0] = Vn
    bad = dict(rb, tokens=tok)
    with pytest.raises(ValueError, match="token ids"):
        list(V().BatchFeeder(T, L, Nq, dev, embedding=table).feed([bad]))
    with pytest.raises(ValueError, match="outside"):
        list(V().BatchFeeder(T, L, Nq, dev, embedding=table).feed([dict(rb, spos=[0, 99, 0])]))


@pytest.mark.gpu
def test_raw_inputs_to_targets_in_one_graph(dev):
    """sample_clips -> embed_tokens -> build_targets_hip on device-resident inputs read nothing back, so they capture as one graph;
    the replay equals the eager result bit for bit."""
    S = V().sampling
    T, L, Nq, Din, B, Vn = 256, 64, 20, 500, 16, 1002
    rng, g = np.random.default_rng(5), torch.Generator().manual_seed(5)
    n = mixed_lengths(B, T, rng)
    raw = torch.randn(int(n.sum()), Din, generator=g).to(dev)
    offs = torch.from_numpy(np.concatenate([[0], np.cumsum(n)])).to(dev)
    spos = torch.from_numpy(S.draw_offsets(n, T, rng)).to(dev)
    table = torch.randn(Vn, 300, generator=g).to(dev)
    tok = torch.from_numpy(rng.integers(0, Vn, (B, Nq))).to(dev)
    dur = (torch.rand(B, generator=g) * 100 + 5).to(dev)
    times = torch.stack([dur * 0.1, dur * 0.6], 1)

    def run():
        vf, nf = S.sample_clips(raw, offs, T, spos=spos)
        qf, qm, ql = S.embed_tokens(tok, table)
        tg = V().build_targets_hip(times, dur, nf, ql, T, L, Nq)
        return [vf, nf, qf, qm, ql] + [tg[k] for k in sorted(tg)]

    eager = [x.clone() for x in run()]
    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        run()
    torch.cuda.current_stream(dev).wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        static = run()
    for x in static:
        x.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert len(static) == len(eager) and all(same(a, b) for a, b in zip(static, eager))
    want, _ = S.sample_clips_torch(raw.cpu(), n, T, spos=spos.cpu())
    assert same(static[0], want)
