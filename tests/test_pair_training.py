"""Training through shared video and query banks: csrc/corpus.hip smin_pair_assemble_bwd, the operator
smin_hip::smin_forward_pairs, SMIN.forward_pairs, training.pair_targets and training.train_epoch_pairs.

Host: the C ABI and operator surface, the refusals, pair_targets against a hand-written loop.
GPU: the kernel through the C ABI against an fp64 restatement under the fixed-order fp32 sum bound; forward_pairs on identity lists
against SMIN.forward (same bits for the outputs and the layers' gradients); on shared banks (P = 9 and P = 19) against the fp64 oracle
with autograd, gated by the error of the expanded route; no host read with cell_counts, repeatability, an unpaired video, the
expansion fall-back and train_epoch_pairs.

Figures measured on an MI355X in the exact fp32 mode, e = max|g - g64| / max|g64| per parameter tensor, the worst tensor of each group,
e_new / e_expanded (printed by the tests; the table is in INTEGRATION.md 3o):
    identity P = 4   backbone 1.08e-06 / 1.08e-06   layers 1.98e-06 / 1.98e-06   head 2.60e-06 / 2.60e-06
    shared   P = 9   backbone 8.70e-07 / 8.51e-07   layers 2.09e-06 / 2.09e-06   head 3.75e-07 / 3.75e-07
    shared   P = 19  backbone 1.57e-06 / 1.36e-06   layers 1.96e-06 / 1.96e-06   head 3.98e-07 / 3.98e-07
"""
import os
import re

import numpy as np
import pytest
import torch

from tests.support.device import dev  # noqa: F401  (the module's device fixture)
from tests.support.device import vml as V
from tests.support.compare import bits
from tests.support.corpora import corpus_inputs, expand, loss_of, p19_lists, pair_args, tiny_model, GT_VIDEO, QI9, SCORE_TOL, VI9


ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -24                                         # fp32 unit roundoff
MASKS = ("video_mask", "length_mask", "moment_mask")
TARGETS = ("ym", "sm", "ys", "ss", "ye", "se", "ya")


def csr(idx, n):
    idx = np.asarray(idx)
    return np.concatenate([[0], np.cumsum(np.bincount(idx, minlength=n))]), np.argsort(idx, kind="stable")


# ---------------------------------------------------------------- host: surface
def test_header_and_table_declare_the_backward():
    text = open(os.path.join(ROOT, "include", "smin_hip.h")).read()
    assert re.search(r"\bint\s+smin_pair_assemble_bwd\s*\(", text) and re.search(r"\bsize_t\s+smin_pair_assemble_bwd_workspace_bytes\s*\(", text)
    for name in ("smin_pair_assemble_bwd", "smin_pair_assemble_bwd_workspace_bytes"):
        assert name in V()._lib.SIGNATURES, name
        assert hasattr(V()._lib.load(), name)
    assert "#define SMIN_HIP_ABI_VERSION 2" in text and V()._lib.load().smin_abi_version() == 2
    lib = V()._lib.load()
    assert lib.smin_pair_assemble_bwd_workspace_bytes(9, 16, 32) == 9 * 4 * 32 * 4          # P * ceil(T / 4) * D floats
    assert lib.smin_pair_assemble_bwd_workspace_bytes(19, 3, 36) == 19 * 1 * 36 * 4


def test_operator_is_registered_and_refuses_cpu():
    ops = V()._lib.load_torch()
    assert hasattr(ops, "smin_forward_pairs")
    schema = str(torch.ops.smin_hip.smin_forward_pairs.default._schema)
    for name in ("Tensor video_index", "Tensor query_index", "Tensor v_ptr", "Tensor v_pairs", "Tensor q_ptr", "Tensor q_pairs", "Tensor[] params",
                 "*, bool overlap_boundary", "bool async_weights", "int? known_cell_count", "bool tail_split"):
        assert name in schema, schema
    for name in ("grad_sync", "input_grads", "attention"):
        assert name not in schema, schema
    m, _ = tiny_model()
    vid, qry, _ = corpus_inputs()
    i32 = lambda x: torch.as_tensor(np.asarray(x), dtype=torch.int32)
    (vp, vs), (qp, qs) = csr(VI9, 5), csr(QI9, 4)
    o = m._node_options()
    for k in ("grad_sync", "input_grads", "attention"):
        o.pop(k)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.smin_forward_pairs(*pair_args(vid, qry), i32(VI9), i32(QI9), i32(vp), i32(vs), i32(qp), i32(qs), m._native_params(), 16, 8, 4, 2, 5, 16, **o)


def test_method_refuses_cpu_and_bad_lists():
    m, _ = tiny_model()
    vid, qry, _ = corpus_inputs()
    with pytest.raises(V()._lib.SminHipError, match="no CPU fallback"):
        m.forward_pairs(*pair_args(vid, qry), VI9, QI9)
    for vi, qi in (([0, 5], [0, 0]), ([0, 1], [0, -1]), ([0, 1], [4, 0])):
        with pytest.raises(ValueError, match="video_index must lie"):
            m.forward_pairs(*pair_args(vid, qry), vi, qi)
    with pytest.raises(ValueError, match="at least one pair"):
        m.forward_pairs(*pair_args(vid, qry), [], [])
    with pytest.raises(ValueError, match="one length"):
        m.forward_pairs(*pair_args(vid, qry), [0, 1, 2], [0, 1])


def test_pair_targets_by_hand():
    vid, _, tg = corpus_inputs()
    got = V().pair_targets(vid, tg, VI9, QI9, GT_VIDEO)
    assert set(got) == set(MASKS) | set(TARGETS)
    positives = [p for p in range(9) if VI9[p] == GT_VIDEO[QI9[p]]]
    assert positives == [0, 1, 2, 6]
    for p in range(9):
        for k in MASKS:
            assert torch.equal(got[k][p], vid[k][VI9[p]]), (k, p)
        for k in TARGETS:
            want = tg[k][QI9[p]] if p in positives else torch.zeros_like(tg[k][0])
            assert got[k].dtype == tg[k].dtype and torch.equal(got[k][p], want), (k, p)
    plan = V().PairPlan(VI9, QI9, 5, 4, "cpu", gt_video=GT_VIDEO)
    assert plan.positive.tolist() == [int(p in positives) for p in range(9)] and plan.positive_rows.tolist() == positives
    assert plan.v_ptr.tolist() == [0, 3, 4, 7, 7, 9] and plan.v_pairs.tolist() == [0, 2, 5, 3, 1, 6, 8, 4, 7]
    assert plan.q_ptr.tolist() == [0, 3, 7, 9, 9] and plan.q_pairs.tolist() == [1, 4, 6, 0, 2, 7, 8, 3, 5]
    with pytest.raises(ValueError, match="gt_video must name"):
        V().pair_targets(vid, tg, VI9, QI9, [0, 1])


# ---------------------------------------------------------------- GPU
def kernel_lists(P, nv, nq, seed):
    if (P, nv, nq) == (9, 5, 4):
        return np.array(VI9), np.array(QI9)
    rng = np.random.RandomState(seed)
    return rng.randint(0, nv, P), rng.randint(0, nq, P)


@pytest.mark.gpu
@pytest.mark.parametrize("P,nv,nq,T,Nq,D", [(9, 5, 4, 16, 5, 32), (1, 1, 1, 1, 1, 4), (19, 5, 4, 3, 2, 36)])
def test_pair_assemble_bwd_against_fp64(dev, P, nv, nq, T, Nq, D):
    L_ = V()._lib
    lib = L_.load()
    g = torch.Generator().manual_seed(P * 10 + D)
    df, dfw, dfs = torch.randn(P, T, D, generator=g), torch.randn(P, Nq, D, generator=g), torch.randn(P, D, generator=g)
    fv, fsb = torch.randn(nv, T, D, generator=g), torch.randn(nq, D, generator=g)
    vi, qi = kernel_lists(P, nv, nq, P)
    (vp, vs), (qp, qs) = csr(vi, nv), csr(qi, nq)
    vt, qt = torch.as_tensor(vi), torch.as_tensor(qi)
    # the fp64 restatement, and per output element the sum of |term| and the number of terms n of the bound (n + 1) * 2^-24 * sum|term|
    d64 = lambda x: x.double()
    tv = d64(df) * d64(fsb)[qt].unsqueeze(1)
    ts = torch.cat([d64(dfs).unsqueeze(1), d64(df) * d64(fv)[vt]], 1)                 # [P][1 + T][D]: dfs[p], then the T products
    want = [torch.zeros(nv, T, D, dtype=torch.float64).index_add_(0, vt, tv), torch.zeros(nq, Nq, D, dtype=torch.float64).index_add_(0, qt, d64(dfw)),
            torch.zeros(nq, D, dtype=torch.float64).index_add_(0, qt, ts.sum(1))]
    mag = [torch.zeros(nv, T, D, dtype=torch.float64).index_add_(0, vt, tv.abs()), torch.zeros(nq, Nq, D, dtype=torch.float64).index_add_(0, qt, d64(dfw).abs()),
           torch.zeros(nq, D, dtype=torch.float64).index_add_(0, qt, ts.abs().sum(1))]
    seg_v, seg_q = torch.as_tensor(np.diff(vp)).double(), torch.as_tensor(np.diff(qp)).double()
    n = [seg_v.reshape(nv, 1, 1), seg_q.reshape(nq, 1, 1), (seg_q * (T + 1)).reshape(nq, 1)]
    i32 = lambda x: torch.as_tensor(np.asarray(x), dtype=torch.int32).to(dev)
    ins = [x.to(dev) for x in (df, dfw, dfs, fv, fsb)] + [i32(vi), i32(qi), i32(vp), i32(vs), i32(qp), i32(qs)]
    nbytes = lib.smin_pair_assemble_bwd_workspace_bytes(P, T, D)
    assert nbytes == P * ((T + 3) // 4) * D * 4
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)

    def run(args, ws_bytes=nbytes, sizes=(P, nv, nq, T, Nq, D), outs=None):
        outs = [torch.full(w.shape, float("nan"), dtype=torch.float32, device=dev) for w in want] if outs is None else outs
        rc = lib.smin_pair_assemble_bwd(L_.stream(), *[L_.ptr(x) for x in args], *sizes, *[L_.ptr(o) for o in outs], L_.ptr(ws), ws_bytes)
        torch.cuda.synchronize()
        return rc, outs

    rc, got = run(ins)
    assert rc == 0
    for name, o, w, s, k in zip(("dfv", "dfw_bank", "dfs_bank"), got, want, mag, n):
        err, bound = (o.cpu().double() - w).abs(), (k + 1) * U * s
        print(name, "max err", err.max().item(), "max bound", bound.max().item())
        assert not torch.isnan(o).any(), name
        assert (err <= bound).all(), (name, (err - bound).max().item())
    # a video or query without a pair: exact zeros over the NaN fill
    for v in np.flatnonzero(np.diff(vp) == 0):
        assert bits(got[0][v]).eq(0).all()
    for q in np.flatnonzero(np.diff(qp) == 0):
        assert bits(got[1][q]).eq(0).all() and bits(got[2][q]).eq(0).all()
    if P == 9:
        assert np.diff(vp)[3] == 0 and np.diff(qp)[3] == 0 and np.diff(vp)[0] == 3 and np.diff(qp)[0] == 3
    # the same bits every run
    _, again = run(ins)
    for a, b in zip(got, again):
        assert torch.equal(bits(a), bits(b))
    # NULL dfw / dfs are zeros, bit for bit
    zeros = [ins[0], torch.zeros_like(ins[1]), torch.zeros_like(ins[2])] + ins[3:]
    _, z = run(zeros)
    for null in ([ins[0], None, None] + ins[3:], [ins[0], None, zeros[2]] + ins[3:], [ins[0], zeros[1], None] + ins[3:]):
        _, o = run(null)
        for a, b in zip(z, o):
            assert torch.equal(bits(a), bits(b))
    # rejected before any launch: the NaN fill stays
    bad = [dict(sizes=(P, nv, nq, T, Nq, D + 2)), dict(sizes=(P, nv, nq, T, Nq, 2)), dict(sizes=(0, nv, nq, T, Nq, D)), dict(sizes=(P, 0, nq, T, Nq, D)),
           dict(sizes=(P, nv, nq, 0, Nq, D)), dict(sizes=(P, nv, nq, T, 0, D)), dict(ws_bytes=nbytes - 1), dict(args=[None] + ins[1:]),
           dict(args=ins[:3] + [None] + ins[4:]), dict(args=ins[:7] + [None] + ins[8:]), dict(args=ins[:10] + [None])]
    for kw in bad:
        rc, o = run(kw.pop("args", ins), **kw)
        assert rc != 0, kw
        for t in o:
            assert torch.isnan(t).all(), kw
    rc, _ = run(ins, outs=[got[0], None, got[2]])
    assert rc != 0


@pytest.fixture(scope="module")
def world(dev):
    """the tiny model on the device, the V = 5 / Q = 4 inputs on both sides, and a cache of per-list references"""
    m, sd = tiny_model(dev)
    vid, qry, tg = corpus_inputs()
    to = lambda d: {k: v.to(dev) for k, v in d.items()}
    return dict(m=m, sd=sd, vid=vid, qry=qry, tg=tg, vid_d=to(vid), qry_d=to(qry), tg_d=to(tg), refs={})


def grads_of(m, out, targets):
    """{name: gradient} of loss_fn(out, targets), and the loss"""
    for p in m.parameters():
        p.grad = None
    loss = loss_of(V().loss_fn, out, targets)
    loss.backward()
    torch.cuda.synchronize()
    return {k: p.grad.detach().clone() for k, p in m.named_parameters()}, loss.detach()


def oracle_grads(w, vi, qi, vid=None, qry=None, tg=None, gt=GT_VIDEO):
    """the fp64 oracle with autograd on the expanded pairs: outputs, {name: gradient}"""
    from oracle import smin_oracle as O
    vid, qry, tg = w["vid"] if vid is None else vid, w["qry"] if qry is None else qry, w["tg"] if tg is None else tg
    sd = {k: v.double().requires_grad_(True) for k, v in w["sd"].items()}
    xs = expand(vid, qry, vi, qi)
    xs[0], xs[2] = xs[0].double(), xs[2].double()
    out = O.smin_forward(sd, dict(T=16, L=8, C=4), *xs)
    t = V().pair_targets(vid, {k: (v.double() if v.is_floating_point() else v) for k, v in tg.items()}, vi, qi, gt)
    loss_of(O.loss_fn, out, t).backward()
    return [o.detach() for o in out], {k: v.grad for k, v in sd.items()}


def group_of(key):
    return "backbone" if key.startswith("backbone.") else "layers" if key.startswith("smis.") else "head"


def gate(w, dev, vi, qi, vid, qry, tg, vid_d, qry_d, tg_d, gt, tag):
    """forward_pairs against the fp64 oracle, gated by the expanded route's own error; returns the two gradient dicts"""
    m = w["m"]
    key = (tag, tuple(vi), tuple(qi))
    if key not in w["refs"]:
        w["refs"][key] = oracle_grads(w, vi, qi, vid, qry, tg, gt)
    ref_out, g64 = w["refs"][key]
    assert m._plan(vid_d["video_features"], qry_d["query_features"]) == "node" and not m.keep_attention
    targets = V().pair_targets(vid_d, tg_d, vi, qi, gt)
    out = m.forward_pairs(*pair_args(vid_d, qry_d), vi, qi)
    for name, o, r in zip(("pm", "ps", "pe", "pa"), out, ref_out):
        assert o.shape == r.shape and o.dtype == torch.float32 and o.requires_grad
        err = (o.detach().cpu().double() - r).abs().max().item()
        print(V().get_gemm_mode(), tag, name, "forward_pairs vs oracle", err)
        assert err < SCORE_TOL, (name, err)
    g_new, _ = grads_of(m, out, targets)
    g_exp, _ = grads_of(m, m(*expand(vid_d, qry_d, vi, qi)), targets)
    assert set(g_new) == set(g64) == set(g_exp)
    worst = {}
    for k, r in g64.items():
        scale = r.abs().max().item()
        a, b = g_new[k].cpu().double(), g_exp[k].cpu().double()
        if scale < 1e-9:                               # the key biases the softmax is invariant to
            assert k.endswith("W_k.bias"), k
            assert a.abs().max().item() <= 2 * b.abs().max().item() + 1e-9, k
            continue
        e_new, e_exp = (a - r).abs().max().item() / scale, (b - r).abs().max().item() / scale
        grp = worst.setdefault(group_of(k), [0.0, 0.0])
        grp[0], grp[1] = max(grp[0], e_new), max(grp[1], e_exp)
        assert e_new <= 2 * e_exp + 1e-6, (k, e_new, e_exp)
    for grp, (a, b) in sorted(worst.items()):
        print(V().get_gemm_mode(), tag, f"P = {len(vi)}", grp, f"e_new {a:.2e}  e_expanded {b:.2e}")
    return out, g_new, g_exp


@pytest.mark.gpu
def test_identity_lists_are_forward(dev, world):
    w = world
    m = w["m"]
    sub = lambda d: {k: v[:4] for k, v in d.items()}
    vid, vid_d = sub(w["vid"]), sub(w["vid_d"])
    ar = list(range(4))
    gt = [0, 1, 3, 3]                                  # three positive pairs
    base = m(*pair_args(vid_d, w["qry_d"]))
    out, g_new, g_exp = gate(w, dev, ar, ar, vid, w["qry"], w["tg"], vid_d, w["qry_d"], w["tg_d"], gt, "identity")
    for name, o, b in zip(("pm", "ps", "pe", "pa"), out, base):
        assert torch.equal(bits(o), bits(b)), name
    same = [k for k in g_new if not k.startswith("backbone.")]
    assert len(g_new) - len(same) == 19 and len(same) == 2 * 20 + 8
    for k in same:                                     # the same kernels on the same bits
        assert torch.equal(bits(g_new[k]), bits(g_exp[k])), k
    assert int(V()._lib.load_torch().layout_status(dev)[0]) == 0


@pytest.mark.gpu
@pytest.mark.parametrize("P", [9, 19])
def test_shared_banks_against_oracle(dev, world, P):
    w = world
    vi, qi = (VI9, QI9) if P == 9 else p19_lists()
    assert len(vi) == P and sum(v == GT_VIDEO[q] for v, q in zip(vi, qi)) >= 2 and len({q for v, q in zip(vi, qi) if v == GT_VIDEO[q]}) == 2
    out, _, _ = gate(w, dev, vi, qi, w["vid"], w["qry"], w["tg"], w["vid_d"], w["qry_d"], w["tg_d"], GT_VIDEO, "shared")
    mm = w["vid"]["moment_mask"][torch.as_tensor(vi)]
    assert out[0].detach().cpu()[~mm].abs().max().item() == 0.0
    assert w["m"].known_cell_count is None


def step(w, vi, qi, vid_d=None, cell_counts=None, gt=GT_VIDEO):
    m = w["m"]
    vid_d = w["vid_d"] if vid_d is None else vid_d
    for p in m.parameters():
        p.grad = None
    out = m.forward_pairs(*pair_args(vid_d, w["qry_d"]), vi, qi, cell_counts=cell_counts)
    loss_of(V().loss_fn, out, V().pair_targets(vid_d, w["tg_d"], vi, qi, gt)).backward()
    return {k: p.grad for k, p in m.named_parameters()}


@pytest.mark.gpu
def test_step_reads_nothing_back_and_repeats(dev, world):
    w = world
    counts = w["vid"]["moment_mask"].reshape(5, -1).sum(1).tolist()
    assert counts == [36, 1, 15, 36, 6]
    first = {k: g.clone() for k, g in step(w, VI9, QI9, cell_counts=counts).items()}     # first use outside the checked region
    torch.cuda.synchronize()
    mode = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        second = step(w, VI9, QI9, cell_counts=counts)
    finally:
        torch.cuda.set_sync_debug_mode(mode)
    torch.cuda.synchronize()
    for k, g in second.items():
        assert torch.equal(bits(g), bits(first[k])), k
    third = step(w, VI9, QI9)                                                             # the node reads the count itself: the same bits
    for k, g in third.items():
        assert torch.equal(bits(g), bits(first[k])), k
    assert int(V()._lib.load_torch().layout_status(dev)[0]) == 0 and w["m"].known_cell_count is None


@pytest.mark.gpu
def test_unpaired_videos_change_nothing(dev, world):
    """Videos 0 and 3 (the two of full length) have no pair: the video encoder's gradients equal those of the bank without them up to
    the order of an fp32 sum (exact zeros are added), and the position embedding's rows past the longest paired video stay zero."""
    w = world
    m = w["m"]
    T, Din, D = 16, 24, 32
    vi, qi = [1, 2, 4, 2, 4, 1, 2], [0, 1, 2, 3, 0, 1, 0]
    gt = [1, 2, 0, 2]
    keep = torch.tensor([1, 2, 4], device=dev)
    small = {k: v.index_select(0, keep) for k, v in w["vid_d"].items()}
    remap = {1: 0, 2: 1, 4: 2}
    ga = {k: g.clone() for k, g in step(w, vi, qi, gt=gt).items()}
    gb = {k: g.clone() for k, g in step(w, [remap[v] for v in vi], qi, vid_d=small, gt=[remap.get(v, -1) for v in gt]).items()}
    # sum|term| of the three sums, from the expansion route on the Python host: df of the pairs at the backbone's output
    seen = {}
    hook = m.backbone.register_forward_hook(lambda mod, args, out: (seen.update(fs=out[1].detach()), out[0].register_hook(lambda g: seen.update(df=g.detach())))[0])
    m.fused_core = False
    try:
        step(w, vi, qi, gt=gt)
    finally:
        m.fused_core = True
        hook.remove()
    torch.cuda.synchronize()
    dv = torch.zeros(5, T, D, dtype=torch.float64).index_add_(0, torch.as_tensor(vi), (seen["df"].double() * seen["fs"].double().unsqueeze(1)).cpu())
    dv = (dv * w["vid"]["video_mask"].double()).abs()                                     # |masked gradient| per (video, frame)
    x = w["vid"]["video_features"].double().abs()
    pre = "backbone.videoencoder."
    checks = [(pre + "ve.weight", dv.reshape(-1, D).t() @ x.reshape(-1, Din), 5 * T), (pre + "ve.bias", dv.sum((0, 1)), 5 * T), (pre + "pe.weight", dv.sum(0), 5)]
    for k, mag, n in checks:
        err, bound = (ga[k].cpu().double() - gb[k].cpu().double()).abs(), (n + 1) * U * mag
        print(k, "max |difference|", err.max().item(), "max bound", bound.max().item())
        assert (err <= bound).all(), (k, (err - bound).max().item())
    assert ga[pre + "pe.weight"][:10].abs().max().item() > 0                              # video 2 has 10 frames, the longest with a pair
    assert bits(ga[pre + "pe.weight"][10:]).eq(0).all() and bits(gb[pre + "pe.weight"][10:]).eq(0).all()


@pytest.mark.gpu
@pytest.mark.parametrize("switch", ["keep_attention", "fused_core"])
def test_off_the_node_path_it_is_the_expanded_forward(dev, world, switch):
    w = world
    m = w["m"]
    old = getattr(m, switch)
    setattr(m, switch, switch == "keep_attention")
    try:
        assert not m._bank_plan(w["vid_d"]["video_features"], w["qry_d"]["query_features"])
        got = m.forward_pairs(*pair_args(w["vid_d"], w["qry_d"]), VI9, QI9)
        want = m(*expand(w["vid_d"], w["qry_d"], VI9, QI9))
        targets = V().pair_targets(w["vid_d"], w["tg_d"], VI9, QI9, GT_VIDEO)
        ga, _ = grads_of(m, got, targets)
        gb, _ = grads_of(m, want, targets)
    finally:
        setattr(m, switch, old)
    for name, g, b in zip(("pm", "ps", "pe", "pa"), got, want):
        assert torch.equal(bits(g), bits(b)), name
    for k in ga:
        assert torch.equal(bits(ga[k]), bits(gb[k])), k


@pytest.mark.gpu
def test_train_epoch_pairs(dev, world):
    api, w = V(), world
    m, _ = tiny_model(dev)
    twin, _ = tiny_model(dev)
    vi19, qi19 = p19_lists()
    counts = w["vid"]["moment_mask"].reshape(5, -1).sum(1).tolist()
    groups = [dict(**w["vid_d"], **w["qry_d"], **w["tg_d"], video_index=vi, query_index=qi, gt_video=GT_VIDEO, cell_counts=counts)
              for vi, qi in ((VI9, QI9), (vi19, qi19))]
    positives = [sum(v == GT_VIDEO[q] for v, q in zip(g["video_index"], g["query_index"])) for g in groups]
    assert positives[0] == 4 and positives[1] >= 2

    class Probe(api.EpochMeter):
        reads = 0

        def result(self, group=None):
            Probe.reads += 1
            torch.cuda.set_sync_debug_mode("default")
            return super().result(group)

    # the same two steps by hand on the twin: the expanded batch through SMIN.forward
    opt_t = api.FusedAdam(twin.parameters(), lr=1e-3)
    twin.train()
    items = []
    for g, npos in zip(groups, positives):
        opt_t.zero_grad()
        t = api.pair_targets(w["vid_d"], w["tg_d"], g["video_index"], g["query_index"], GT_VIDEO)
        loss = loss_of(api.loss_fn, twin(*expand(w["vid_d"], w["qry_d"], g["video_index"], g["query_index"])), t)
        loss.backward()
        opt_t.step()
        items.append((loss.item(), npos))
    opt = api.FusedAdam(m.parameters(), lr=1e-3)
    first, _ = api.train_epoch_pairs(m, opt, groups[:1], Probe(device=dev))              # (first use outside the checked region)
    assert first == float(items[0][0])                                                   # the same forward bits, the same loss kernel
    m.load_state_dict(w["sd"])
    opt = api.FusedAdam(m.parameters(), lr=1e-3)
    Probe.reads = 0
    meter = Probe(device=dev)
    torch.cuda.synchronize()
    mode = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        loss, metrics = api.train_epoch_pairs(m, opt, groups, meter)
    finally:
        torch.cuda.set_sync_debug_mode(mode)
    assert Probe.reads == 1 and m.known_cell_count is None and m.training
    assert metrics["num_samples"] == sum(positives) and loss == metrics["loss"]
    # the meter's loss: the groups' losses weighted by their positive pairs; the step's loss is loss_fn over pair_targets of the
    # expanded batch, which the pairs' node matches to the outputs' rounding (first group: the same parameters on both sides)
    want = sum(np.float64(v) * n for v, n in items) / sum(n for _, n in items)
    print("train_epoch_pairs loss", loss, "by hand on the expanded batch", want)
    assert abs(loss - want) <= 1e-5 * abs(want)
    assert int(api._lib.load_torch().layout_status(dev)[0]) == 0
    with pytest.raises(ValueError, match="at least one query with its own video"):
        api.train_epoch_pairs(m, opt, [dict(groups[0], gt_video=[3, 3, 3, 3])], meter)
