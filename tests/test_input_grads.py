"""Gradients of the model's own inputs (SMIN.input_grads) and the differentiable device feeding path (sampling.py
differentiable=True): the one-node step against the reference's autograd (tests/golden/g9_input_grads.npz,
tests/golden/make_golden_input_grads.py) and the oracle's, the Python host against the one-node step, and the feeder's backward
kernels against torch autograd through the plain restatements."""
import numpy as np
import pytest
import torch

from tests import helpers as H
from tests.support.device import dev  # noqa: F401  (the module's device fixture)
from tests.support.corpora import build_model, loss_of_batch as loss_of, one_node_only
from tests.support.references import _sample_clips_ref

pytestmark = pytest.mark.gpu

KEYS = ["T", "L", "C", "D", "dl", "layers", "Din", "Nq", "H", "B"]


def cluster_error():
    import models
    return models.vml_amd._lib.load().smin_lstm_cluster_error()


def close(got, want, rel):
    got, want = got.detach().double().cpu(), want.detach().double().cpu()
    err = float((got - want).abs().max())
    return err <= rel * float(want.abs().max()) + 1e-7, err


@pytest.mark.parametrize("case", ["tiny", "ragged"])
def test_input_grads_match_the_reference(dev, case):
    """video_features.grad / query_features.grad of a fixed linear functional of (pm, ps, pe, pa), one-node step with input_grads,
    against the reference's own autograd; padded frames' rows are exactly 0."""
    from oracle import smin_oracle as O
    z = H.load_npz("g9_input_grads")
    cfg = dict(zip(KEYS, [int(v) for v in z[case + "/cfg"]]))
    sd = O.formula_state_dict(H.smin_shapes(*[cfg[k] for k in KEYS[:-1]]), gain=1.2)
    inp = [torch.from_numpy(z[case + "/in/" + k]).to(dev) for k in H.IN_KEYS]
    w = {k: torch.from_numpy(z[case + "/w/" + k]).to(dev) for k in ("wm", "ws", "we", "wa")}
    m = build_model(cfg, sd, dev)
    m.input_grads = True
    one_node_only(m)
    inp[0].requires_grad_(True)
    inp[2].requires_grad_(True)
    assert m._plan(inp[0], inp[2]) == "node"
    pm, ps, pe, pa = m(*inp)
    ((w["wm"] * pm).sum() + (w["ws"] * ps).sum() + (w["we"] * pe).sum() + (w["wa"] * pa).sum()).backward()
    assert cluster_error() == 0
    for name, got in (("video_features", inp[0].grad), ("query_features", inp[2].grad)):
        ok, err = close(got, torch.from_numpy(z[case + "/grad/" + name]), 2e-3)
        print(case, name, "max abs err", err)
        assert ok, (name, err)
    pad = inp[1].reshape(inp[0].shape[0], -1) == 0
    assert pad.any()
    assert bool((inp[0].grad[pad] == 0).all())


@pytest.mark.parametrize("Din,layers,Hh,dl", [(40, 2, 32, 32), (500, 3, 256, 128)])
def test_input_grads_against_the_oracle(dev, Din, layers, Hh, dl):
    """B = 17 ragged samples, queries cut below max_query_length, two shapes of the query encoder (H = 256 runs the cluster LSTM):
    the one-node step's input gradients against the oracle's autograd, with no expired poll of the cluster recurrence."""
    from oracle import smin_oracle as O
    T, L, C, Nq, B, short = 64, 16, 4, 12, 17, 9
    D = 2 * Hh
    sd = O.formula_state_dict(H.smin_shapes(T, L, C, D, dl, layers, Din, Nq, Hh), gain=1.2)
    batch = O.synthetic_batch(B, T, L, Nq, Din, seed=Din + layers)
    batch["query_features"][:, short:] = 0
    batch["query_mask"][:, short:] = 0
    vf = batch["video_features"].clone().requires_grad_(True)
    qf = batch["query_features"].clone().requires_grad_(True)
    ref = O.smin_forward({k: v.clone() for k, v in sd.items()}, dict(T=T, L=L, C=C), vf, batch["video_mask"], qf, batch["query_mask"],
                         batch["length_mask"], batch["moment_mask"])
    loss_of(ref, batch, oracle=True).backward()
    m = build_model(dict(T=T, L=L, C=C, D=D, dl=dl, layers=layers, Din=Din, Nq=Nq, H=Hh), sd, dev)
    m.input_grads = True
    one_node_only(m)
    b = {k: v.to(dev) for k, v in batch.items()}
    inp = H.model_inputs(b)
    inp[0] = inp[0].clone().requires_grad_(True)
    inp[2] = inp[2][:, :short].contiguous().requires_grad_(True)       # the batch cut to its longest query
    inp[3] = inp[3][:, :short].contiguous()
    for step in range(2):
        inp[0].grad = inp[2].grad = None
        loss_of(m(*inp), b).backward()
        assert cluster_error() == 0, step
    assert inp[2].grad.shape == (B, short, 300)
    for name, got, want in (("video_features", inp[0].grad, vf.grad), ("query_features", inp[2].grad, qf.grad[:, :short])):
        ok, err = close(got, want, 2e-3)
        print(Din, layers, Hh, name, "max abs err", err, "of", float(want.abs().max()))
        assert ok, (name, err)


def test_input_grads_move_nothing_else(dev):
    """With input_grads on: scores and every parameter gradient are bit-identical whether or not the inputs require grad, and two
    repetitions give bit-identical input gradients.  With it off, video_features.grad stays None (the Python host serves the step)."""
    from oracle import smin_oracle as O
    T, L, C, D, dl, layers, Din, Nq, Hh, B = 64, 16, 4, 512, 128, 3, 500, 13, 256, 6
    sd = O.formula_state_dict(H.smin_shapes(T, L, C, D, dl, layers, Din, Nq, Hh), gain=1.2)
    batch = O.synthetic_batch(B, T, L, Nq, Din, seed=3)
    b = {k: v.to(dev) for k, v in batch.items()}
    m = build_model(dict(T=T, L=L, C=C, D=D, dl=dl, layers=layers, Din=Din, Nq=Nq, H=Hh), sd, dev)
    m.input_grads = True
    one_node_only(m)

    def step(grad_inputs):
        inp = [x.clone() for x in H.model_inputs(b)]
        if grad_inputs:
            inp[0].requires_grad_(True)
            inp[2].requires_grad_(True)
        m.zero_grad(set_to_none=True)
        out = m(*inp)
        loss_of(out, b).backward()
        torch.cuda.synchronize()
        assert cluster_error() == 0
        return [o.detach().clone() for o in out], {k: p.grad.clone() for k, p in m.named_parameters()}, inp[0].grad, inp[2].grad

    o0, g0, dx0, dq0 = step(False)
    assert dx0 is None and dq0 is None
    o1, g1, dx1, dq1 = step(True)
    o2, g2, dx2, dq2 = step(True)
    for x, y in zip(o0, o1):
        assert torch.equal(x, y)
    for k in g0:
        assert torch.equal(g0[k], g1[k]), k
        assert torch.equal(g1[k], g2[k]), k
    assert torch.equal(dx1, dx2) and torch.equal(dq1, dq2)
    assert float(dx1.abs().max()) > 0 and float(dq1.abs().max()) > 0
    m.input_grads = False
    inp = [x.clone() for x in H.model_inputs(b)]
    inp[0].requires_grad_(True)
    assert m._plan(inp[0], inp[2]) == "stream"


def test_python_host_forms_the_video_gradient(dev):
    """input_grads with fused_core = False: the Python host's fused video encoder returns video_features.grad through
    smin_video_encoder_bwd_input, equal to the one-node step's within 1e-5 relative."""
    from oracle import smin_oracle as O
    T, L, C, D, dl, layers, Din, Nq, Hh, B = 64, 16, 4, 128, 32, 2, 40, 9, 64, 5
    sd = O.formula_state_dict(H.smin_shapes(T, L, C, D, dl, layers, Din, Nq, Hh), gain=1.2)
    batch = O.synthetic_batch(B, T, L, Nq, Din, seed=21)
    b = {k: v.to(dev) for k, v in batch.items()}
    grads = []
    for native in (True, False):
        m = build_model(dict(T=T, L=L, C=C, D=D, dl=dl, layers=layers, Din=Din, Nq=Nq, H=Hh), sd, dev)
        m.input_grads, m.fused_core = True, native
        inp = H.model_inputs(b)
        inp[0] = inp[0].clone().requires_grad_(True)
        inp[2] = inp[2].clone().requires_grad_(True)
        loss_of(m(*inp), b).backward()
        grads.append((inp[0].grad, inp[2].grad))
    for got, want in zip(grads[1], grads[0]):
        ok, err = close(got, want, 1e-5)
        assert ok, err


def test_embed_tokens_backward(dev):
    """embed_tokens(differentiable=True): table.grad against torch autograd through embed_tokens_torch in fp64 (duplicate ids,
    out-of-range ids, the pad id), bit-reproducible; the mask and lengths carry no gradient; default: the table is detached."""
    from vml_amd.sampling import embed_tokens, embed_tokens_torch
    g = torch.Generator().manual_seed(4)
    V, E, B, Nq = 37, 20, 6, 11
    tok = torch.randint(0, 8, (B, Nq), generator=g)                    # many duplicates
    tok[0, :3] = torch.tensor([-1, V, V + 5])
    tok[1, -2:] = V - 1                                                  # the pad id
    table = torch.randn(V, E, generator=g)
    wts = torch.randn(B, Nq, E, generator=g)
    t64 = table.double().requires_grad_(True)
    (embed_tokens_torch(tok, t64)[0].double() * wts.double()).sum().backward()
    runs = []
    for _ in range(2):
        t = table.to(dev).requires_grad_(True)
        qf, qm, ql = embed_tokens(tok.to(dev), t, differentiable=True)
        assert qf.requires_grad and not qm.requires_grad and not ql.requires_grad
        (qf * wts.to(dev)).sum().backward()
        runs.append(t.grad)
    assert torch.equal(runs[0], runs[1])
    ok, err = close(runs[0], t64.grad, 1e-6)
    assert ok, err
    assert bool((runs[0][8:V - 1] == 0).all())                          # rows no token touches
    qf, _, _ = embed_tokens(tok.to(dev), table.to(dev).requires_grad_(True))
    assert not qf.requires_grad


@pytest.mark.parametrize("mode", ["pick", "mean"])
def test_sample_clips_backward(dev, mode):
    """sample_clips(differentiable=True): raw.grad against torch autograd through the restatement in fp64, bit-reproducible.
    pick with spos > 0 (the top of the reference's draw range) and n <= T; mean with n > T and n <= T.  (Within the draw range the
    pick rule never reaches the clip at n - 1, so no raw row is read twice; the kernel sums any repeat in ascending t all the same.)"""
    from vml_amd.sampling import spos_high
    g = torch.Generator().manual_seed(9)
    T, Din = 16, 12
    lengths = np.array([5, 16, 40, 0, 23, 100, 17])
    spos = (spos_high(lengths, T) - 1) if mode == "pick" else np.zeros(len(lengths), np.int64)
    raw = torch.randn(int(lengths.sum()), Din, generator=g)
    wts = torch.randn(len(lengths), T, Din, generator=g)
    r64 = raw.double().requires_grad_(True)
    (_sample_clips_ref(r64, lengths, T, spos, mode) * wts.double()).sum().backward()
    from vml_amd.sampling import sample_clips
    runs = []
    for _ in range(2):
        r = raw.to(dev).requires_grad_(True)
        out, nf = sample_clips(r, lengths, T, spos=spos if mode == "pick" else None, mode=mode, differentiable=True)
        assert out.requires_grad and not nf.requires_grad
        (out * wts.to(dev)).sum().backward()
        runs.append(r.grad)
    assert torch.equal(runs[0], runs[1])
    ok, err = close(runs[0], r64.grad, 1e-6)
    assert ok, err
    if mode == "pick":                                                   # rows the stride skips get 0
        assert int((runs[0].abs().sum(1) == 0).sum()) == int((r64.grad.abs().sum(1) == 0).sum()) > 0


def test_table_gradient_end_to_end(dev):
    """A word-vector table that requires grad -> embed_tokens(differentiable=True) -> SMIN with input_grads -> loss_fn -> backward:
    table.grad against the fp64 restatement (oracle forward in fp64 on the looked-up rows) within 2e-3 relative."""
    from oracle import smin_oracle as O
    from vml_amd.sampling import embed_tokens, embed_tokens_torch
    T, L, C, D, dl, layers, Din, Nq, Hh, B, V = 64, 16, 4, 64, 32, 2, 40, 9, 32, 5, 60
    sd = O.formula_state_dict(H.smin_shapes(T, L, C, D, dl, layers, Din, Nq, Hh), gain=1.2)
    batch = O.synthetic_batch(B, T, L, Nq, Din, seed=17)
    g = torch.Generator().manual_seed(17)
    tok = torch.randint(0, V - 1, (B, Nq), generator=g)
    tok[batch["query_mask"].reshape(B, Nq) == 0] = V - 1                 # <pad>
    table = torch.randn(V, 300, generator=g) * 0.5
    t64 = table.double().requires_grad_(True)
    sd64 = {k: v.double() for k, v in sd.items()}
    b64 = {k: (v.double() if v.is_floating_point() else v) for k, v in batch.items()}
    qf64 = embed_tokens_torch(tok, t64)[0].double() * (tok != V - 1).unsqueeze(-1).double()
    ref = O.smin_forward(sd64, dict(T=T, L=L, C=C), b64["video_features"], batch["video_mask"], qf64, batch["query_mask"], batch["length_mask"],
                         batch["moment_mask"])
    loss_of(ref, b64, oracle=True).backward()
    m = build_model(dict(T=T, L=L, C=C, D=D, dl=dl, layers=layers, Din=Din, Nq=Nq, H=Hh), sd, dev)
    m.input_grads = True
    one_node_only(m)
    b = {k: v.to(dev) for k, v in batch.items()}
    t = table.to(dev).requires_grad_(True)
    qf, qm, _ = embed_tokens(tok.to(dev), t, differentiable=True)
    qf = qf * qm.unsqueeze(-1).float()                                  # the dataset's padded rows are zero
    inp = H.model_inputs(b)
    inp[2] = qf
    loss_of(m(*inp), b).backward()
    ok, err = close(t.grad, t64.grad, 2e-3)
    print("table.grad max abs err", err, "of", float(t64.grad.abs().max()))
    assert ok, err
