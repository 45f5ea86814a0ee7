"""The query encoder's BiLSTM layer kernels (csrc/bilstm.hip, csrc/bilstm_cluster.hip) against a float64 restatement of one
bidirectional layer over packed sequences.

CPU: the restatement itself is pinned to torch.nn.LSTM(bidirectional=True) on pack_padded_sequence in float64, and the case list
is checked against Python mirrors of the layer dispatch (bilstm_cluster_ok, cl_geometry, nt_splitk_splits, tn_splits).
GPU: smin_bilstm_layer_fwd / _bwd / _bwd_weights through the C ABI and BiLstmLayerFn over both recurrences -- the cluster path at
every P = H / 32, single- and multi-pass, and the streamed path at every padded width Hp -- then the sentence feature and the
two-layer QueryEncoder."""
import math

import pytest
import torch

from tests.helpers import tn_splits      # gemm.h tn_splits (one mirror for every test file)
from tests.helpers import cdiv
from tests.support.device import dev  # noqa: F401  (the module's device fixture)
from tests.support.compare import _rel

FWD_TOL = 1e-5          # max |got - ref| / max |ref|, per output and case (as test_query_encoder_matches_packed_lstm)
GRAD_TOL = 2e-4
CUS = 256               # MI355X; the GPU tests read the real count


# ---------------------------------------------------------------- float64 restatement

def lstm_layer_ref(x, length, w_ih, w_hh, b_ih, b_hh):
    """One bidirectional LSTM layer (reference models.py:46-58: nn.LSTM over pack_padded_sequence / pad_packed_sequence) as the
    layer kernels compute it.  x [B, Nq, In]; length [B] (clamped to Nq; 0 gives an all-zero sample); w_ih [2, 4H, In],
    w_hh [2, 4H, H], b_ih / b_hh [2, 4H] (direction 0 forward, 1 reverse; gate order i, f, g, o).  Per sample and direction the
    recurrence visits positions 0 .. L-1 (forward) or L-1 .. 0 (reverse) from zero state.
    Returns (Hout [B, Nq, 2H], zero at padded positions; gate activations G [B, Nq, 2, 4H]; cell states Cs [B, Nq, 2, H]; steps),
    G and Cs zero at padded positions; steps holds the pre-activations of every (direction, step) for pre_activation_grad."""
    B, Nq, _ = x.shape
    H = w_hh.shape[2]
    L = length.long().clamp(0, Nq)
    ar = torch.arange(B)
    outs, gates, cells, steps = [], [], [], []
    for d in range(2):
        h = x.new_zeros(B, H)
        c = x.new_zeros(B, H)
        Hd, Gd, Cd = x.new_zeros(B, Nq, H), x.new_zeros(B, Nq, 4 * H), x.new_zeros(B, Nq, H)
        for s in range(Nq):
            act = s < L
            pos = torch.full((B,), s) if d == 0 else (L - 1 - s).clamp(min=0)
            z = x[ar, pos] @ w_ih[d].t() + b_ih[d] + b_hh[d] + h @ w_hh[d].t()
            if z.requires_grad:
                z.retain_grad()
            steps.append((d, pos, act, z))
            i, f, g, o = torch.sigmoid(z[:, :H]), torch.sigmoid(z[:, H:2 * H]), torch.tanh(z[:, 2 * H:3 * H]), torch.sigmoid(z[:, 3 * H:])
            cn = f * c + i * g
            hn = o * torch.tanh(cn)
            a = act.view(B, 1)
            h, c = torch.where(a, hn, h), torch.where(a, cn, c)
            b_act, p_act = ar[act], pos[act]
            Hd = Hd.index_put((b_act, p_act), hn[act])
            Gd = Gd.index_put((b_act, p_act), torch.cat([i, f, g, o], 1)[act])
            Cd = Cd.index_put((b_act, p_act), cn[act])
        outs.append(Hd)
        gates.append(Gd)
        cells.append(Cd)
    return torch.cat(outs, 2), torch.stack(gates, 2), torch.stack(cells, 2), steps


def pre_activation_grad(steps, B, Nq, H):
    """dG [B, Nq, 2, 4H]: the gradient of the pre-activation gates after a backward through lstm_layer_ref, zero at padded positions."""
    dG = torch.zeros(B, Nq, 2, 4 * H, dtype=torch.float64)
    ar = torch.arange(B)
    for d, pos, act, z in steps:
        if z.grad is not None:
            dG[ar[act], pos[act], d] = z.grad[act].double()
    return dG


def _live(length, B, Nq):
    return torch.arange(Nq).view(1, Nq) < length.long().clamp(0, Nq).view(B, 1)


# ---------------------------------------------------------------- Python mirrors of the layer dispatch

CL_U, CL_BS, GEMM_SLOTS = 32, 4, 768


def cluster_ok(H, streamed_env=False):
    """bilstm_cluster_ok (csrc/bilstm_cluster.hip); streamed_env: SMIN_LSTM_STREAMED is set."""
    return H % CL_U == 0 and CL_U <= H <= 256 and not streamed_env


def cl_geometry(B, H, cus):
    """cl_geometry: (P, nclus, grid, passes of each cluster) -- ceil(B / 4) * 2 (sample group, direction) passes dealt round-robin
    over nclus clusters of P workgroups; the grid is padded to whole groups of 8 clusters."""
    P = H // CL_U
    ngroups = cdiv(B, CL_BS) * 2
    maxclus = max(cus // (8 * P) * 8, 1)
    nclus = min(ngroups, maxclus)
    grid = cdiv(nclus, 8) * 8 * P
    passes = [len(range(c, ngroups, nclus)) for c in range(nclus)]
    return P, nclus, grid, passes, maxclus


def nt_splitk_splits(M, N, K, gemm_mode=0):
    """gemm.h nt_splitk_splits: the split-K factor of the layer's input gradient dX [M, N] = dG [M, K] Wih_cat [K, N]."""
    blocks = cdiv(M, 32) * cdiv(N, 128)
    if gemm_mode != 0 or blocks * 2 > GEMM_SLOTS or K < 1024:
        return 1
    s = GEMM_SLOTS * 2 // blocks
    while s > 1 and (K % (16 * s) != 0 or K // s < 256):
        s -= 1
    return min(s, 16)


def regimes(case, cus=CUS, gemm_mode=0):
    """Every dispatch class one layer case reaches."""
    H, B, Nq, In, lens, streamed = case
    R = B * Nq
    out = {f"lens-{lens}", "In-300" if In == 300 else "In-2H" if In == 2 * H else f"In-{In}"}
    out.add("B-1" if B == 1 else f"B-4k+{B % 4}")
    out.add("dX-splitk" if nt_splitk_splits(R, In, 8 * H, gemm_mode) > 1 else "dX-plain")
    out.add("dWih-tn-split" if tn_splits(R, 8 * H, In) > 1 else "dWih-tn-1")
    out.add("dWhh-tn-split" if tn_splits(R, 4 * H, H) > 1 else "dWhh-tn-1")
    if cluster_ok(H, streamed):
        P, nclus, grid, passes, maxclus = cl_geometry(B, H, cus)
        out.add(f"cluster-P{P}")
        assert grid <= cus or maxclus == 1, (case, grid)
        if max(passes) == 1:
            out.add("single-pass-full" if nclus == maxclus else "single-pass")
        else:
            out.add("multi-pass")
            if min(passes) < max(passes):
                out.add("multi-pass-unequal")
            if Nq <= 2:
                out.add(f"multi-pass-Nq{Nq}")
        if nclus == maxclus and P in (5, 6, 7):
            out.add(f"max-nclus-P{P}")
    else:
        Hp = cdiv(H, 64) * 64
        out.add(f"streamed-Hp{Hp}")
        if H % 64:
            out.add("streamed-idle-threads")
        if H % 32 == 0:
            out.add(f"streamed-forced-H{H}")
    return out


# (H, B, Nq, In, lens, expected regimes).  lens: "full" every sample Nq long, "ones" every sample 1, "mixed" the first group of 4
# holds Nq, 1, Nq, 1 and the rest random in 1 .. Nq, plus one sample longer than Nq (clamped) and one of length 0 when B > 5.
LAYER_CASES = [
    # cluster path, one pass, every P
    (32, 1, 5, 300, "full", {"cluster-P1", "B-1", "single-pass", "In-300"}),
    (64, 5, 7, 128, "mixed", {"cluster-P2", "B-4k+1", "single-pass", "In-2H"}),
    (96, 6, 6, 300, "mixed", {"cluster-P3", "B-4k+2"}),
    (128, 7, 9, 256, "ones", {"cluster-P4", "B-4k+3", "dX-splitk", "lens-ones"}),
    (160, 9, 4, 300, "mixed", {"cluster-P5", "dX-splitk"}),
    (192, 3, 5, 384, "mixed", {"cluster-P6", "B-4k+3"}),
    (224, 10, 4, 300, "mixed", {"cluster-P7", "B-4k+2"}),
    (256, 2, 6, 512, "mixed", {"cluster-P8", "In-2H", "dX-splitk"}),
    (256, 64, 12, 300, "mixed", {"cluster-P8", "single-pass-full"}),
    # cluster path, several passes per cluster
    (256, 65, 8, 300, "mixed", {"multi-pass-unequal", "B-4k+1", "dX-splitk"}),
    (256, 97, 2, 512, "full", {"multi-pass-unequal", "multi-pass-Nq2"}),
    (256, 130, 1, 300, "mixed", {"multi-pass-unequal", "multi-pass-Nq1"}),
    (128, 260, 6, 256, "mixed", {"cluster-P4", "multi-pass-unequal", "dWih-tn-split", "dWhh-tn-split"}),
    (160, 130, 5, 300, "mixed", {"max-nclus-P5", "multi-pass-unequal"}),
    (192, 90, 4, 384, "mixed", {"max-nclus-P6", "multi-pass-unequal"}),
    (224, 70, 3, 300, "mixed", {"max-nclus-P7", "multi-pass-unequal"}),
    (32, 520, 3, 64, "mixed", {"cluster-P1", "multi-pass-unequal", "dX-plain", "dWih-tn-split"}),
    (64, 300, 2, 128, "ones", {"cluster-P2", "multi-pass-unequal", "multi-pass-Nq2"}),
    (96, 350, 1, 300, "full", {"cluster-P3", "multi-pass-unequal", "multi-pass-Nq1"}),
    # streamed path: every Hp, idle threads u >= H, ragged tails
    (4, 3, 5, 300, "mixed", {"streamed-Hp64", "streamed-idle-threads"}),
    (12, 5, 6, 24, "full", {"streamed-Hp64", "In-2H"}),
    (36, 6, 4, 300, "mixed", {"streamed-Hp64"}),
    (100, 7, 5, 200, "mixed", {"streamed-Hp128"}),
    (132, 4, 6, 300, "ones", {"streamed-Hp192", "dX-splitk"}),
    (200, 9, 4, 400, "mixed", {"streamed-Hp256", "dX-splitk"}),
    (252, 2, 5, 300, "mixed", {"streamed-Hp256", "streamed-idle-threads"}),
]

# the same inputs through both recurrences: SMIN_LSTM_STREAMED set vs unset
FORCED_CASES = [
    (32, 5, 7, 300, "mixed", {"streamed-forced-H32"}),
    (256, 66, 5, 512, "mixed", {"streamed-forced-H256", "dX-splitk"}),
]

REQUIRED = ({f"cluster-P{p}" for p in range(1, 9)} | {"B-1", "B-4k+1", "B-4k+2", "B-4k+3"}
            | {"single-pass", "single-pass-full", "multi-pass-unequal", "multi-pass-Nq1", "multi-pass-Nq2"}
            | {f"max-nclus-P{p}" for p in (5, 6, 7)}
            | {f"streamed-Hp{hp}" for hp in (64, 128, 192, 256)} | {"streamed-idle-threads"}
            | {"streamed-forced-H32", "streamed-forced-H256"}
            | {"In-300", "In-2H", "dX-splitk", "dX-plain", "dWih-tn-1", "dWih-tn-split", "dWhh-tn-1", "dWhh-tn-split"}
            | {"lens-full", "lens-ones", "lens-mixed"})


def _case(c, streamed=False):
    return c[:5] + (streamed,)


def _layer_id(c, streamed=False):
    H, B, Nq, In, lens = c[:5]
    return f"{'s' if streamed or not cluster_ok(H) else 'c'}H{H}-B{B}-Nq{Nq}-In{In}-{lens}"


def _lengths(B, Nq, kind, g):
    if kind == "full":
        return torch.full((B,), Nq, dtype=torch.int32)
    if kind == "ones":
        return torch.ones(B, dtype=torch.int32)
    lens = torch.randint(1, Nq + 1, (B,), generator=g, dtype=torch.int32)
    lens[:4] = torch.tensor([Nq, 1, Nq, 1], dtype=torch.int32)[:B]
    if B > 5:
        lens[4], lens[5] = Nq + 3, 0
    return lens


def _layer_inputs(H, B, Nq, In, kind, seed):
    """fp32-valued float64 inputs: weights ~ N(0, 1 / fan_in) and biases ~ N(0, 0.3^2), so the gates are mostly off saturation."""
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    x = dict(x=r(B, Nq, In), w_ih=r(2, 4 * H, In) / math.sqrt(In), w_hh=r(2, 4 * H, H) / math.sqrt(H), b_ih=0.3 * r(2, 4 * H),
             b_hh=0.3 * r(2, 4 * H), dH=r(B, Nq, 2 * H))
    return {k: v.float().double() for k, v in x.items()}, _lengths(B, Nq, kind, g)


def _reference(x, lens):
    p = {k: x[k].clone().requires_grad_(True) for k in ("x", "w_ih", "w_hh", "b_ih", "b_hh")}
    Hout, G, Cs, steps = lstm_layer_ref(p["x"], lens, p["w_ih"], p["w_hh"], p["b_ih"], p["b_hh"])
    (Hout * x["dH"]).sum().backward()
    B, Nq, _ = x["x"].shape
    H = x["w_hh"].shape[2]
    live = _live(lens, B, Nq)
    z = torch.stack([torch.stack([z for d, _, _, z in steps if d == dd], 1) for dd in range(2)], 2)   # [B, Nq steps, 2, 4H]
    zlive = z.detach()[live]                                                                      # step s is live iff s < len
    return dict(Hout=Hout.detach(), G=G.detach(), Cs=Cs.detach(), dG=pre_activation_grad(steps, B, Nq, H), dX=p["x"].grad,
                dWih=p["w_ih"].grad.reshape(8 * H, -1), dbias=p["b_ih"].grad.reshape(8 * H), dWhh=p["w_hh"].grad,
                dbhh=p["b_hh"].grad.reshape(8 * H), live=live, zstd=zlive.std().item() if zlive.numel() > 1 else 1.0)


# ---------------------------------------------------------------- CPU: the restatement against nn.LSTM

@pytest.mark.parametrize("B,Nq,lens", [(4, 6, [6, 1, 6, 3]), (2, 5, [5, 5]), (3, 4, [1, 1, 1]), (5, 7, [7, 2, 1, 7, 4])],
                         ids=["mixed-group", "all-Nq", "all-1", "mixed-5"])
def test_restatement_matches_packed_nn_lstm(B, Nq, lens):
    """lstm_layer_ref == nn.LSTM(bidirectional=True).double() on pack_padded_sequence: outputs, dX and every parameter gradient."""
    from torch.nn.utils.rnn import pack_padded_sequence, pad_packed_sequence
    In, H = 10, 6
    torch.manual_seed(B * 10 + Nq)
    lstm = torch.nn.LSTM(In, H, num_layers=1, bidirectional=True, batch_first=True).double()
    for p in lstm.parameters():
        p.data.normal_(0, 0.5)
    lens = torch.tensor(lens)
    x = torch.randn(B, Nq, In, dtype=torch.float64)
    dH = torch.randn(B, Nq, 2 * H, dtype=torch.float64)
    xr = x.clone().requires_grad_(True)
    out, _ = lstm(pack_padded_sequence(xr, lens, batch_first=True, enforce_sorted=False))
    want, _ = pad_packed_sequence(out, batch_first=True, total_length=Nq)
    (want * dH).sum().backward()
    names = ("weight_ih_l0", "weight_hh_l0", "bias_ih_l0", "bias_hh_l0")
    ref_grads = [torch.stack([getattr(lstm, n).grad, getattr(lstm, n + "_reverse").grad]) for n in names]
    p = [torch.stack([getattr(lstm, n), getattr(lstm, n + "_reverse")]).detach().clone().requires_grad_(True) for n in names]
    xg = x.clone().requires_grad_(True)
    got, G, Cs, steps = lstm_layer_ref(xg, lens, *p)
    (got * dH).sum().backward()
    torch.testing.assert_close(got, want, rtol=1e-12, atol=1e-12)
    torch.testing.assert_close(xg.grad, xr.grad, rtol=1e-12, atol=1e-12)
    for a, b in zip(p, ref_grads):
        torch.testing.assert_close(a.grad, b, rtol=1e-12, atol=1e-12)
    # internals: h = o tanh(c) at live positions, zero elsewhere; dG is the pre-activation gradient (dWih = dG^T x, dbias = sum dG)
    live = _live(lens, B, Nq)
    o = G[..., 3 * H:]
    torch.testing.assert_close(got.view(B, Nq, 2, H), (o * torch.tanh(Cs)) * live.view(B, Nq, 1, 1), rtol=1e-14, atol=1e-14)
    assert torch.all(G[~live] == 0) and torch.all(Cs[~live] == 0)
    dG = pre_activation_grad(steps, B, Nq, H)
    assert torch.all(dG[~live] == 0)
    for d in range(2):
        torch.testing.assert_close(dG[:, :, d].reshape(-1, 4 * H).t() @ x.reshape(-1, In), p[0].grad[d], rtol=1e-12, atol=1e-12)
        torch.testing.assert_close(dG[:, :, d].reshape(-1, 4 * H).sum(0), p[2].grad[d], rtol=1e-12, atol=1e-12)


def test_restatement_clamps_lengths_and_keeps_empty_samples_zero():
    """A length past Nq is the full sequence (the kernels clamp it); length 0 gives zero outputs and no gradient."""
    B, Nq, In, H = 3, 4, 5, 3
    g = torch.Generator().manual_seed(9)
    w = [torch.randn(2, 4 * H, In, generator=g, dtype=torch.float64), torch.randn(2, 4 * H, H, generator=g, dtype=torch.float64),
         torch.randn(2, 4 * H, generator=g, dtype=torch.float64), torch.randn(2, 4 * H, generator=g, dtype=torch.float64)]
    x = torch.randn(B, Nq, In, generator=g, dtype=torch.float64, requires_grad=True)
    a = lstm_layer_ref(x, torch.tensor([Nq + 5, 0, 2]), *w)
    b = lstm_layer_ref(x, torch.tensor([Nq, 0, 2]), *w)
    for u, v in zip(a[:3], b[:3]):
        assert torch.equal(u, v)
    assert torch.all(a[0][1] == 0)
    a[0].sum().backward()
    assert torch.all(x.grad[1] == 0) and torch.all(x.grad[2, 2:] == 0) and torch.all(x.grad[0] != 0)


def test_layer_cases_reach_every_regime():
    """At 256 CUs the case list reaches every dispatch class of the layer (REQUIRED), each case reaches the classes it was written
    for, and the P = 5 / 6 / 7 cases at the largest cluster count are shapes whose grid exceeded the CUs before the cap."""
    reached = set()
    for c in LAYER_CASES:
        got = regimes(_case(c))
        assert c[5] <= got, (c[:5], sorted(c[5] - got))
        reached |= got
    for c in FORCED_CASES:
        got = regimes(_case(c, True))
        assert c[5] <= got, (c[:5], sorted(c[5] - got))
        assert "cluster-P%d" % (c[0] // 32) in regimes(_case(c))          # and without the switch the same inputs take the cluster path
        reached |= got
    assert REQUIRED <= reached, sorted(REQUIRED - reached)
    for c in LAYER_CASES:
        H, B = c[0], c[1]
        if H in (160, 192, 224) and any(t.startswith("max-nclus") for t in c[5]):
            P = H // 32
            uncapped = min(cdiv(B, 4) * 2, CUS // P)
            assert cdiv(uncapped, 8) * 8 * P > CUS
    # the cap leaves P = 1, 2, 4, 8 (every bench shape) where the CU count put them, and never exceeds the CUs
    for H in range(32, 257, 32):
        P = H // 32
        for B in (1, 7, 64, 65, 130, 257, 600, 2049):
            for cus in (80, 104, 228, 256, 304):
                _, nclus, grid, passes, maxclus = cl_geometry(B, H, cus)
                assert grid <= cus and sum(passes) == cdiv(B, 4) * 2
                if P in (1, 2, 4, 8) and cus == 256:
                    assert maxclus == cus // P


# ---------------------------------------------------------------- GPU
def _gemm_mode():
    import models
    return models.vml_amd._lib.GEMM_MODES[models.vml_amd._lib.get_gemm_mode()]


def _check_regime(case, streamed, want=None):
    """The case reaches the classes it was written for (want, default its own list) on this device and in this GEMM mode."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    mode = _gemm_mode()
    want = case[5] if want is None else want
    want = want if mode == 0 else {t for t in want if not t.startswith("dX-")}      # only exact fp32 splits dX over K
    got = regimes(_case(case, streamed), cus, mode)
    assert want <= got, (case[:5], cus, sorted(want - got))


def _packed(x, dev):
    """The kernels' operands from the per-direction parameters, built as BiLstmLayerFn builds them."""
    f = lambda k: x[k].float().to(dev)
    w_ih, w_hh, b_ih, b_hh = f("w_ih"), f("w_hh"), f("b_ih"), f("b_hh")
    H = w_hh.shape[2]
    Wih = torch.cat([w_ih[0], w_ih[1]]).contiguous()
    bias = torch.cat([b_ih[0] + b_hh[0], b_ih[1] + b_hh[1]]).contiguous()
    Whh = torch.stack([w_hh[0], w_hh[1]]).contiguous()
    W4 = Whh.view(2, 4, H, H).permute(0, 3, 2, 1).contiguous()
    return Wih, bias, Whh, W4


def _abi_layer(dev, x, lens, mode="split"):
    """Forward, then the backward through the C ABI on NaN-filled outputs and workspace.  mode: "split" (inputs half, weights half),
    "combined" (one call) or "pieces" (inputs half, then the weights half as which = 4, 1, 2 with a second dbias copy)."""
    from vml_amd._lib import call, load, ptr, stream
    B, Nq, In = x["x"].shape
    H = x["w_hh"].shape[2]
    nan = float("nan")
    X, dH, length = x["x"].float().to(dev), x["dH"].float().to(dev), lens.to(dev)
    Wih, bias, Whh, W4 = _packed(x, dev)
    G, Hout, Cs = (torch.full(s, nan, device=dev) for s in ((B, Nq, 2, 4 * H), (B, Nq, 2 * H), (B, Nq, 2, H)))
    call("smin_bilstm_layer_fwd", stream(), ptr(X), ptr(Wih), ptr(bias), ptr(W4), ptr(length), B, Nq, In, H, ptr(G), ptr(Hout), ptr(Cs))
    nb = load().smin_bilstm_layer_bwd_workspace_bytes(B, Nq, In, H)
    ws = torch.full((cdiv(nb, 4) + 64,), nan, device=dev)
    dX, dWih, dbias, dbias2, dWhh = (torch.full(s, nan, device=dev) for s in ((B, Nq, In), (8 * H, In), (8 * H,), (8 * H,), (2, 4 * H, H)))
    args = (ptr(X), ptr(Hout), ptr(G), ptr(Cs), ptr(Wih.t().contiguous()), ptr(Whh), ptr(length), B, Nq, In, H)
    wsa = (ptr(ws), 4 * ws.numel())
    dG = None
    if mode == "combined":
        call("smin_bilstm_layer_bwd", stream(), ptr(dH), *args, ptr(dX), ptr(dWih), ptr(dbias), ptr(dWhh), *wsa)
    else:
        call("smin_bilstm_layer_bwd", stream(), ptr(dH), *args, ptr(dX), None, None, None, *wsa)
        dG = ws[:B * Nq * 8 * H].view(B, Nq, 2, 4 * H).clone()
        assert torch.isnan(dWih).all() and torch.isnan(dWhh).all()          # the inputs half writes no weight gradient
        if mode == "pieces":
            for which in (4, 1, 2):
                call("smin_bilstm_layer_bwd_weights", stream(), which, ptr(X), ptr(Hout), B, Nq, In, H, ptr(dWih), ptr(dbias), ptr(dbias2),
                     ptr(dWhh), *wsa)
            assert torch.equal(dbias, dbias2)
        else:
            call("smin_bilstm_layer_bwd", stream(), None, *args, None, ptr(dWih), ptr(dbias), ptr(dWhh), *wsa)
    torch.cuda.synchronize()
    return dict(Hout=Hout, G=G, Cs=Cs, dG=dG, dX=dX, dWih=dWih, dbias=dbias, dWhh=dWhh)


def _fn_layer(dev, x, lens):
    """BiLstmLayerFn (the module's path) on the same inputs: Hout, dX and the eight parameter gradients."""
    import models
    F = models.vml_amd.functional
    X = x["x"].float().to(dev).requires_grad_(True)
    ps = [x[k][d].float().to(dev).requires_grad_(True) for d in range(2) for k in ("w_ih", "w_hh", "b_ih", "b_hh")]
    Hout = F.BiLstmLayerFn.apply(X, lens.to(dev), *ps)
    (Hout * x["dH"].float().to(dev)).sum().backward()
    torch.cuda.synchronize()
    return Hout.detach(), X.grad, [p.grad for p in ps]


def _run_layer_case(dev, case, streamed, label):
    import models
    H, B, Nq, In, kind = case[:5]
    x, lens = _layer_inputs(H, B, Nq, In, kind, seed=H * 1000 + B * 10 + Nq)
    ref = _reference(x, lens)
    assert 0.5 <= ref["zstd"] <= 3.0, f"pre-activation std {ref['zstd']:.2f} outside [0.5, 3]"
    live = ref["live"]
    got = _abi_layer(dev, x, lens)
    # written everywhere, exact zeros at padded positions (Hout, dG); the NaN prefill of the padded Cs entries reaches no result
    for k in ("Hout", "G", "dG", "dX", "dWih", "dbias", "dWhh"):
        assert torch.isfinite(got[k]).all(), f"{label}: {k} has unwritten (NaN) entries"
    for k in ("Hout", "dG"):
        assert torch.all(got[k].cpu()[~live] == 0), f"{label}: {k} not zero at padded positions"
    ratios_f = {"Hout": _rel(got["Hout"], ref["Hout"]), "G": _rel(got["G"].cpu()[live], ref["G"][live]),
                "Cs": _rel(got["Cs"].cpu()[live], ref["Cs"][live])}
    ratios_g = {k: _rel(got[k], ref[k]) for k in ("dG", "dX", "dWih", "dbias", "dWhh")}
    for k, v in ratios_f.items():
        assert v <= FWD_TOL, f"{label}: {k} rel err {v:.2e}"
    for k, v in ratios_g.items():
        assert v <= GRAD_TOL, f"{label}: {k} rel err {v:.2e}"
    # forward and backward repeat bit for bit, and the module's Function computes the same bits
    again = _abi_layer(dev, x, lens)
    for k in ("Hout", "G", "dG", "dX", "dWih", "dbias", "dWhh"):
        assert torch.equal(got[k], again[k]), f"{label}: {k} differs between two runs"
    assert torch.equal(got["Cs"][live.to(dev)], again["Cs"][live.to(dev)])
    Hf, dXf, gf = _fn_layer(dev, x, lens)
    assert torch.equal(Hf, got["Hout"]) and torch.equal(dXf, got["dX"])
    H4 = 4 * H
    for d in range(2):
        w_ih, w_hh, b_ih, b_hh = gf[4 * d:4 * d + 4]
        assert torch.equal(w_ih, got["dWih"][d * H4:(d + 1) * H4]) and torch.equal(w_hh, got["dWhh"][d])
        assert torch.equal(b_ih, got["dbias"][d * H4:(d + 1) * H4]) and torch.equal(b_hh, b_ih)
    assert models.vml_amd._lib.load().smin_lstm_cluster_error() == 0, f"{label}: a bounded poll of the cluster recurrence expired"
    worst_f, worst_g = max(ratios_f.values()), max(ratios_g.values())
    print(f"bilstm {label}: zstd {ref['zstd']:.2f} worst fwd {worst_f:.2e} grad {worst_g:.2e}")
    return worst_f, worst_g


@pytest.mark.gpu
@pytest.mark.parametrize("case", LAYER_CASES, ids=[_layer_id(c) for c in LAYER_CASES])
def test_layer_against_fp64(dev, case):
    """Forward (Hout, G, Cs), backward inputs half (dG from the workspace, dX), weights half (dWih, dbias, dWhh) against
    lstm_layer_ref; NaN-prefilled outputs; two runs and BiLstmLayerFn give the same bits; the error word stays 0."""
    _check_regime(case, False)
    _run_layer_case(dev, case, False, _layer_id(case))


@pytest.mark.gpu
@pytest.mark.parametrize("case", FORCED_CASES, ids=[_layer_id(c) for c in FORCED_CASES])
def test_layer_both_recurrences_against_fp64(dev, case, monkeypatch):
    """The same inputs through the cluster recurrence and, with SMIN_LSTM_STREAMED set (read at every call), the streamed one:
    each against fp64 on its own."""
    _check_regime(case, False, {f"cluster-P{case[0] // 32}"})
    _run_layer_case(dev, case, False, "cluster-" + _layer_id(case))
    monkeypatch.setenv("SMIN_LSTM_STREAMED", "1")
    _check_regime(case, True)
    _run_layer_case(dev, case, True, "forced-" + _layer_id(case, True))


# ---------------------------------------------------------------- saturated gates

# H = 32 through both recurrences (FORCED_CASES' case) and H = 256 at the module's smallest B (the cluster's eight-workgroup exchange)
SAT_LAYER_CASES = [FORCED_CASES[0][:5], LAYER_CASES[7][:5]]
LEVELS = ("hard", "frozen")


def _saturated_inputs(case, level):
    """_layer_inputs with b_ih moved so that b_ih + b_hh, which dominates the pre-activations, is large: on 40 % of the 8H gate units
    +-[22, 30] (hard), or on all of them +-[120, 170] (frozen).  Frozen: in direction 0 the input and forget gates of the first half of
    the units are open (+), so their cell state is a running sum of tanh(g) = +-1."""
    H, B, Nq, In, kind = case
    x, lens = _layer_inputs(H, B, Nq, In, kind, seed=H * 1000 + B * 10 + Nq)
    g = torch.Generator().manual_seed(H + len(level))
    sign = torch.randint(0, 2, (2, 4 * H), generator=g).double() * 2 - 1
    if level == "frozen":
        sign[0, :H // 2] = sign[0, H:H + H // 2] = 1.0
        target = sign * (120 + 50 * torch.rand(2, 4 * H, generator=g, dtype=torch.float64))
        x["b_ih"] = (target - x["b_hh"]).float().double()
    else:
        big = torch.rand(2, 4 * H, generator=g) < 0.4
        target = sign * (22 + 8 * torch.rand(2, 4 * H, generator=g, dtype=torch.float64))
        x["b_ih"] = torch.where(big, target - x["b_hh"], x["b_ih"]).float().double()
    return x, lens


def _pre_activations(x, lens):
    """the live pre-activations [n, 4H] of both directions, detached, from lstm_layer_ref"""
    B, Nq, _ = x["x"].shape
    with torch.no_grad():
        steps = lstm_layer_ref(x["x"], lens, x["w_ih"], x["w_hh"], x["b_ih"], x["b_hh"])[3]
    return torch.cat([z[act] for _, _, act, z in steps])


@pytest.mark.parametrize("level", LEVELS)
@pytest.mark.parametrize("case", SAT_LAYER_CASES, ids=[_layer_id(c) for c in SAT_LAYER_CASES])
def test_saturated_layer_inputs_hold_what_they_claim(case, level):
    """On the float64 restatement.  hard: at least a quarter of the live pre-activations beyond +-17 and a quarter inside +-4.  frozen:
    every one in +-[90, 200]; with the input and forget gates frozen open the cell state of a unit is +-(t + 1) after step t.  The
    lengths are ragged and include 1; the H = 32 case runs either recurrence, the H = 256 case eight workgroups per cluster."""
    H, B, Nq, In, kind = case
    x, lens = _saturated_inputs(case, level)
    assert 1 in lens.tolist() and Nq in lens.tolist() and cluster_ok(H) and (H == 32 or H // CL_U == 8)
    z = _pre_activations(x, lens)
    if level == "hard":
        assert (z.abs() > 17).double().mean().item() >= 0.25 and (z.abs() < 4).double().mean().item() >= 0.25
        return
    assert 90 <= z.abs().min().item() and z.abs().max().item() <= 200
    Cs = lstm_layer_ref(x["x"], lens, x["w_ih"], x["w_hh"], x["b_ih"], x["b_hh"])[2]
    full = [b for b in range(B) if int(lens[b]) >= Nq][0]
    c = Cs[full, :, 0, :H // 2]                                                  # direction 0 visits position t at step t
    want = torch.arange(1, Nq + 1, dtype=torch.float64).unsqueeze(1)
    assert (c.abs() - want).abs().max().item() <= 1e-9 and bool((c.abs()[1:] > c.abs()[:-1]).all())


def _run_saturated_layer(dev, case, level, label):
    """Both halves through the C ABI on _saturated_inputs: everything finite, exact zeros at padded positions, the error word 0, and the
    project's gate against lstm_layer_ref in float64 with e_torch32 from lstm_layer_ref in fp32."""
    import models
    from tests.support.compare import gate
    H, B, Nq, In, kind = case
    x, lens = _saturated_inputs(case, level)
    ref, ref32 = _reference(x, lens), _reference({k: v.float() for k, v in x.items()}, lens)
    live = ref["live"]
    got = _abi_layer(dev, x, lens)
    for k in ("Hout", "G", "dG", "dX", "dWih", "dbias", "dWhh"):
        assert torch.isfinite(got[k]).all(), f"{label}: {k} is not finite"
    assert torch.isfinite(got["Cs"].cpu()[live]).all()
    for k in ("Hout", "dG"):
        assert torch.all(got[k].cpu()[~live] == 0), f"{label}: {k} not zero at padded positions"
    for k in ("Hout", "dG", "dX", "dWih", "dbias", "dWhh"):
        gate(f"bilstm {label} {k}", got[k], ref[k], ref32[k])
    for k in ("G", "Cs"):
        gate(f"bilstm {label} {k}", got[k].cpu()[live], ref[k][live], ref32[k][live])
    if level == "frozen":
        full = [b for b in range(B) if int(lens[b]) >= Nq][0]
        c = got["Cs"].cpu()[full, :, 0, :H // 2].abs()
        assert bool((c[1:] > c[:-1]).all()) and torch.equal(c[:, 0], torch.arange(1.0, Nq + 1))
    assert models.vml_amd._lib.load().smin_lstm_cluster_error() == 0, f"{label}: a bounded poll of the cluster recurrence expired"


@pytest.mark.gpu
@pytest.mark.parametrize("level", LEVELS)
@pytest.mark.parametrize("case", SAT_LAYER_CASES, ids=[_layer_id(c) for c in SAT_LAYER_CASES])
def test_saturated_layer_against_fp64(dev, case, level):
    """smin_bilstm_layer_fwd, _bwd and the weights half through the cluster recurrence with the gates partly (hard) or wholly (frozen)
    saturated: expf overflows in the sigmoids and the tanh on one side and underflows on the other.  Measured on an MI355X:
    INTEGRATION.md, "Saturated inputs"."""
    _check_regime(case + (set(),), False, {f"cluster-P{case[0] // 32}"})
    _run_saturated_layer(dev, case, level, f"cluster-{_layer_id(case)} {level}")


@pytest.mark.gpu
@pytest.mark.parametrize("level", LEVELS)
def test_saturated_layer_streamed_against_fp64(dev, level, monkeypatch):
    """The H = 32 case through the streamed recurrence (SMIN_LSTM_STREAMED set, read at every call)."""
    case = SAT_LAYER_CASES[0]
    monkeypatch.setenv("SMIN_LSTM_STREAMED", "1")
    _check_regime(case + (set(),), True, {"streamed-forced-H32"})
    _run_saturated_layer(dev, case, level, f"forced-{_layer_id(case, True)} {level}")


HALVES_CASES = [(64, 5, 7, 128, "mixed"), (64, 300, 2, 128, "mixed"), (256, 65, 4, 300, "mixed"), (256, 8, 5, 512, "mixed")]


@pytest.mark.gpu
@pytest.mark.parametrize("case", HALVES_CASES, ids=[_layer_id(c) for c in HALVES_CASES])
def test_backward_halves_and_pieces_bit_equal(dev, case):
    """Over the cluster path at P = 2 and 8, one pass and several, split-K dX and plain: the combined backward == inputs half +
    weights half == the weights half's pieces in another order (with dbias_cat2), bit for bit."""
    import models
    H, B, Nq, In, kind = case
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    P, nclus, grid, passes, _ = cl_geometry(B, H, cus)
    assert P in (2, 8) and (max(passes) > 1) == (B > 64)
    x, lens = _layer_inputs(H, B, Nq, In, kind, seed=7 * H + B)
    outs = [_abi_layer(dev, x, lens, m) for m in ("combined", "split", "pieces")]
    for k in ("Hout", "dX", "dWih", "dbias", "dWhh"):
        assert torch.isfinite(outs[0][k]).all()
        assert torch.equal(outs[0][k], outs[1][k]) and torch.equal(outs[0][k], outs[2][k]), k
    assert torch.equal(outs[1]["dG"], outs[2]["dG"])
    assert models.vml_amd._lib.load().smin_lstm_cluster_error() == 0


# ---------------------------------------------------------------- sentence feature and module level

@pytest.mark.gpu
def test_sentence_feature_against_gather(dev):
    """smin_sentence_feature_fwd / _bwd: f_s[b] = [f_w[b, max(min(len, Nq) - 1, 0), :H] | f_w[b, 0, H:]], and the backward adds
    d f_s into exactly those entries -- at len 0, 1, Nq and past Nq."""
    from vml_amd._lib import call, ptr, stream
    B, Nq, H = 6, 5, 48
    g = torch.Generator().manual_seed(11)
    lens = torch.tensor([0, 1, Nq, Nq + 4, 3, 1], dtype=torch.int32)
    fw = torch.randn(B, Nq, 2 * H, generator=g)
    dfs = torch.randn(B, 2 * H, generator=g)
    base = torch.randn(B, Nq, 2 * H, generator=g)
    last = (lens.long().clamp(max=Nq) - 1).clamp(min=0)
    want = torch.cat([fw[torch.arange(B), last, :H], fw[:, 0, H:]], 1)
    want_d = base.clone()
    want_d[torch.arange(B), last, :H] += dfs[:, :H]
    want_d[:, 0, H:] += dfs[:, H:]
    fw_d, dfs_d, len_d = fw.to(dev), dfs.to(dev), lens.to(dev)
    fs = torch.full((B, 2 * H), float("nan"), device=dev)
    dfw = base.to(dev)
    call("smin_sentence_feature_fwd", stream(), ptr(fw_d), ptr(len_d), B, Nq, H, ptr(fs))
    call("smin_sentence_feature_bwd", stream(), ptr(dfs_d), ptr(len_d), B, Nq, H, ptr(dfw))
    assert torch.equal(fs.cpu(), want)
    assert torch.equal(dfw.cpu(), want_d)


def _encoder(H, Nq, seed):
    import models
    g = torch.Generator().manual_seed(seed)
    qe = models.QueryEncoder(Nq, H)
    for name, p in qe.lstm.named_parameters():
        p.data = torch.randn(p.shape, generator=g) * (0.3 if "bias" in name else 1 / math.sqrt(p.shape[1]))
    return qe, g


@pytest.mark.gpu
@pytest.mark.parametrize("B,Nq,H", [(90, 6, 192), (97, 5, 256)], ids=["P6-max-nclus", "P8-multi-pass"])
def test_query_encoder_two_layers_against_packed_fp64(dev, B, Nq, H):
    """QueryEncoder (both layers and the sentence feature) against nn.LSTM over pack_padded_sequence in fp64: outputs and every
    parameter gradient, at a P = 6 shape with the largest cluster count and a multi-pass P = 8 shape."""
    import models
    from torch.nn.utils.rnn import pack_padded_sequence, pad_packed_sequence
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    P, nclus, grid, passes, maxclus = cl_geometry(B, H, cus)
    assert max(passes) > 1 and grid <= cus and (P != 6 or nclus == maxclus)
    qe, g = _encoder(H, Nq, B + H)
    x = torch.randn(B, Nq, 300, generator=g)
    lens = _lengths(B, Nq, "mixed", g).clamp(1, Nq).long()
    mask = (torch.arange(Nq).unsqueeze(0) < lens.unsqueeze(1)).to(torch.uint8).unsqueeze(-1)
    x = x * mask
    ref = torch.nn.LSTM(300, H, num_layers=2, bidirectional=True, batch_first=True).double()
    ref.load_state_dict({k: v.double() for k, v in qe.lstm.state_dict().items()})
    out, _ = ref(pack_padded_sequence(x.double(), lens, batch_first=True, enforce_sorted=False))
    fw_ref, _ = pad_packed_sequence(out, batch_first=True, total_length=Nq)
    fs_ref = torch.cat([fw_ref[torch.arange(B), lens - 1, :H], fw_ref[:, 0, H:]], dim=1)
    wf, wsn = torch.randn(B, Nq, 2 * H, generator=g).double(), torch.randn(B, 2 * H, generator=g).double()
    ((fw_ref * wf).sum() + (fs_ref * wsn).sum()).backward()
    qd = qe.to(dev)
    fs, fw = qd(x.to(dev), mask.to(dev))
    ratios_f = [_rel(fw.detach(), fw_ref.detach()), _rel(fs.detach(), fs_ref.detach())]
    ((fw * wf.float().to(dev)).sum() + (fs * wsn.float().to(dev)).sum()).backward()
    ratios_g = {k: _rel(p.grad, r.grad) for (k, p), (_, r) in zip(qd.lstm.named_parameters(), ref.named_parameters())}
    assert max(ratios_f) <= FWD_TOL, ratios_f
    for k, v in ratios_g.items():
        assert v <= GRAD_TOL, (k, v)
    assert models.vml_amd._lib.load().smin_lstm_cluster_error() == 0
    print(f"query encoder B{B}-Nq{Nq}-H{H}: worst fwd {max(ratios_f):.2e} grad {max(ratios_g.values()):.2e}")


@pytest.mark.gpu
def test_query_encoder_length_zero_sample_matches_torch_path(dev):
    """A sample with no word: the fused layers give zero outputs for it and, like every other sample, the module's own torch path
    (fused_lstm = False) -- outputs and parameter gradients."""
    import models
    B, Nq, H = 6, 7, 64
    qe, g = _encoder(H, Nq, 5)
    qe = qe.to(dev)
    lens = torch.tensor([7, 0, 3, 1, 0, 5])
    mask = (torch.arange(Nq).unsqueeze(0) < lens.unsqueeze(1)).to(torch.uint8).unsqueeze(-1).to(dev)
    x = (torch.randn(B, Nq, 300, generator=g)).to(dev) * mask
    wf, wsn = torch.randn(B, Nq, 2 * H, generator=g).to(dev), torch.randn(B, 2 * H, generator=g).to(dev)

    def run(fused):
        qe.fused_lstm = fused
        qe.zero_grad(set_to_none=True)
        fs, fw = qe(x, mask)
        ((fw * wf).sum() + (fs * wsn).sum()).backward()
        return fs.detach(), fw.detach(), {k: p.grad.clone() for k, p in qe.lstm.named_parameters()}
    try:
        fs, fw, gr = run(True)
        fs_t, fw_t, gr_t = run(False)
    finally:
        qe.fused_lstm = True
    for b in (1, 4):
        assert torch.all(fw[b] == 0) and torch.all(fs[b] == 0) and torch.all(fw_t[b] == 0) and torch.all(fs_t[b] == 0)
    assert _rel(fw, fw_t.double().cpu()) <= FWD_TOL and _rel(fs, fs_t.double().cpu()) <= FWD_TOL
    for k in gr:
        assert torch.isfinite(gr[k]).all() and _rel(gr[k], gr_t[k].double().cpu()) <= GRAD_TOL, k
    assert models.vml_amd._lib.load().smin_lstm_cluster_error() == 0
