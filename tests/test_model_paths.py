"""Model-level gradients on weights that keep every backward path visible.

The kernels have their own fp64 tests.  What composes them -- the one-node step of csrc/torch_binding.cpp, where the kernels'
gradients are summed into dfs / dfw / df and handed to the encoders, and the two Python hosts -- is judged only by model-level tests,
all on oracle.formula_state_dict and all by |got - ref| <= 2e-3 * max|ref| + 1e-7 per parameter.  With those weights the query
encoder's outputs have rms about 0.1: every attention logit is tiny, every gate sits at sigmoid(0), every softmax is nearly uniform,
and most of the backward graph carries no signal the bound could see.  This file

  1. scales named parameter groups of the same formula weights (alive_state_dict; RNG-free),
  2. restates the oracle's forward with a named detach at each of 14 paths (cut_forward; bit for bit smin_forward without a cut),
  3. asserts on the fp64 oracle alone, for every case the GPU tests use: (1) cutting any one path moves some gradient by >= 5x its
     tolerance; (2) no gradient but W_k.bias (true gradient 0) lies under the floor, 1e-7 <= 1e-3 * max|grad|; (3) every valid
     score lies in (0.02, 0.98); (4) the fp32 CPU oracle is within 0.25x tolerance of the fp64 one, so the comparison is about the
     kernels and not about fp32; (5) formula weights hide six paths or more on the same case,
  4. and then compares the node, the stream host and the unit host with the fp64 oracle at the project's bound.

Largest change of any parameter gradient when a path is cut, in units of that gradient's tolerance (fp64 oracle; "formula" is
formula_state_dict(gain=1.2) on the same case and batch; the in_* cuts count the two input gradients as well):

                    native2           ragged5           b9                deep3             deep5
  path              formula  alive    formula  alive    formula  alive    formula  alive    formula  alive
  cu_word_logits      0.10   481.1      0.14   460.5      0.28   589.0      0.63   495.9    144.07   774.7
  cu_word_value      63.68   489.2     82.80   484.4    218.53   512.4    253.36   496.8    495.68   531.7
  cu_s_hat           63.68   489.2     82.80   484.4    218.53   492.6    253.36   496.8    495.68   499.6
  cu_self_logits     63.68   491.2     82.80   488.5    218.53   494.5    253.36   516.2    495.68   612.9
  cu_gate_arg         1.69    28.9      2.22    14.8      1.82     6.8     11.42    26.5     54.83    33.4
  bu_word_logits      0.16   438.9      0.45   449.9      0.89   406.1      0.90   494.1    364.90   472.3
  bu_word_value       0.11    43.9      0.32    73.3      0.47    30.1      0.22   132.7      1.92    12.3
  bu_fs_in_bq         0.14    46.7      0.38    99.6      0.59    50.0      0.33   115.7      2.19    22.7
  bu_self_logits      0.51   438.9      1.38   449.9      2.10   406.1      0.95   494.1    364.90   472.3
  bu_gate_arg         9.03   140.1      9.07   138.6     12.53    58.4     16.21   105.1    167.00   203.4
  bu_A_in_bm          0.08  1295.7      0.53   224.3      0.77   216.8      0.27   136.6    694.56  1281.5
  f_hadamard_fs     500.84   526.3    502.85   535.2    504.14   538.0    505.79   523.1    539.41   554.8
  mu_mean_c         499.46   498.5    499.64   498.5    499.77   498.7    499.96   498.7    500.00   499.9
  mu_pair            40.32   367.0     65.89   282.1     93.00   320.5    131.96   300.0   1299.13  2305.1
  in_video                   495.9
  in_query                   497.9
  hidden (< 5x)       7        0        7        0        7        0        6        0        2        0

  alive weights     native2           ragged5           b9                deep3             deep5
  weakest path      cu_gate_arg 28.9  cu_gate_arg 14.8  cu_gate_arg 6.8   cu_gate_arg 26.5  bu_word_value 12.3
  min max|grad|     1.34e-4           1.01e-4           1.19e-4           1.54e-4           1.30e-4
  valid scores      0.142 .. 0.961    0.093 .. 0.951    0.176 .. 0.932    0.110 .. 0.877    0.057 .. 0.976
  fp32 noise        0.037x            0.106x            0.068x            0.057x            0.132x

(ragged5 under formula weights: the smallest max|grad| is 3.0e-9, a thirtieth of the floor.)

Depth.  With more than two layers the residual sums grow (each layer adds f_m to f_c and doubles f_b).  deep3 meets all five
conditions.  At 4 and 5 layers condition 5 cannot be met on any shape tried (six shapes; formula weights hide 2 or 3 paths): there
formula weights saturate the scores (deep5: 66 % of the valid scores outside (0.02, 0.98), loss 12.3, fp32 oracle 1287x tolerance from
fp64) and see most paths for that bad reason.  deep5 therefore holds conditions 1 to 4 under its damped constants, and in place of 5
asserts that formula weights fail 3 and 4 there.  It is kept beside deep3 because only five layers reach the second 4-wide partition
of the content stream's history.

Measured on the GPU (MI355X): the worst gradient of any case and host is 0.17x tolerance, scores within 4.6e-6; the one entry over
the bound is a W_k.bias whose true gradient is 0 (RAISED below).  Three mutations of the node's backward, each run once against this
file and test_hip_parity.test_against_oracle_random: the gate's term dropped from dfs -- all six node runs here fail, 9 of the 13
rows there; layer 0's boundary dW_q zeroed, and the boundary unit's dfw dropped -- all six node runs here fail, there only the
saturated 5-layer row.
"""
import functools
import math

import pytest
import torch

from oracle import smin_oracle as O
from tests import helpers as H
from tests.support.device import dev  # noqa: F401  (the module's device fixture)
from tests.support.corpora import SCORE_TOL

KEYS = ["T", "L", "C", "D", "dl", "layers", "Din", "Nq", "H", "B"]


def tol_of(ref):
    """The project's bound on a parameter gradient (test_against_oracle_random)."""
    return 2e-3 * float(ref.abs().max()) + 1e-7


@pytest.fixture(scope="module", autouse=True)
def few_threads():
    """The oracle's operations are small: beyond a few threads they only wait for each other (measured: 7x slower on 64)."""
    n = torch.get_num_threads()
    torch.set_num_threads(min(n, 8))
    yield
    torch.set_num_threads(n)


# ---------------------------------------------------------------- the weight family
GROUPS = {
    "lstm": lambda n: ".queryencoder.lstm." in n,
    "ve": lambda n: ".videoencoder.ve." in n,
    "attn": lambda n: ".attn_layer.W_q." in n or ".attn_layer.W_k." in n,
    "hat": lambda n: ".linear_c_hat." in n or ".linear_w_hat." in n or ".linear_s_hat." in n,
    "conv": lambda n: ".moment_unit.conv_layer_" in n or ".content_unit.linear_c." in n,
    "loc": lambda n: n.startswith("localization."),
}
START = dict(lstm=3.0, ve=2.0, attn=4.0, hat=2.0, conv=1.0, loc=0.3)


def alive_state_dict(shapes, scales):
    """formula_state_dict(shapes, gain=1.2) with the parameter groups of GROUPS multiplied by the constants in ``scales``: the query
    encoder's outputs, the attention logits and the gate arguments leave the origin, the score heads stay short of saturation.
    RNG-free: names, shapes and the constants regenerate it."""
    assert set(scales) <= set(GROUPS), scales
    sd = O.formula_state_dict(shapes, gain=1.2)
    for name in sd:
        hit = [g for g, member in GROUPS.items() if member(name)]
        assert len(hit) <= 1, (name, hit)
        if hit and hit[0] in scales:
            sd[name] = sd[name] * scales[hit[0]]
    return sd


# ---------------------------------------------------------------- the oracle's forward with a named detach at each path
PATHS = ["cu_word_logits", "cu_word_value", "cu_s_hat", "cu_self_logits", "cu_gate_arg",
         "bu_word_logits", "bu_word_value", "bu_fs_in_bq", "bu_self_logits", "bu_gate_arg", "bu_A_in_bm",
         "f_hadamard_fs", "mu_mean_c", "mu_pair"]
INPUT_PATHS = ["in_video", "in_query"]                # what video_features.grad / query_features.grad are made of, cut at the encoders


def _at(x, name, cut):
    return x.detach() if cut == name else x


def _word_attention(sd, prefix, query, key, value, qmask_row, scale_dim, cut, unit):
    q = O._lin(sd, prefix + "W_q", query)
    k = O._lin(sd, prefix + "W_k", key)
    s = q @ k.transpose(1, 2) / math.sqrt(scale_dim)
    s = s * qmask_row
    s = s.masked_fill(qmask_row == 0, -1e9)
    return torch.softmax(_at(s, unit + "_word_logits", cut), dim=-1) @ _at(value, unit + "_word_value", cut)


def _content_unit(sd, p, f_c, f_w, f_s, f_m, query_mask, moment_mask, cut):
    dt = f_c.dtype
    B, L, _, C, D = f_c.shape
    m = moment_mask.to(dt)[:, :, :, None, None]
    qm = query_mask.to(dt)
    dl = sd[p + "linear_c_hat.weight"].shape[0]
    c_hat = O._lin(sd, p + "linear_c_hat", f_c) * m
    w_hat = O._lin(sd, p + "linear_w_hat", f_w) * qm
    s_hat = _at(O._lin(sd, p + "linear_s_hat", f_s), "cu_s_hat", cut)
    qrow = qm.reshape(B, 1, -1)
    a = _word_attention(sd, p + "attn_layer.", c_hat.reshape(B, L * L * C, dl), w_hat, w_hat, qrow, dl, cut, "cu")
    a = a.reshape(B, L, L, C, dl) * m
    q = c_hat * (a + s_hat[:, None, None, None, :])
    A = torch.softmax(_at(q @ q.transpose(3, 4) / math.sqrt(dl), "cu_self_logits", cut), dim=-1) * m
    cc = O._lin(sd, p + "linear_c", A @ c_hat) * m
    gated = torch.sigmoid(_at(f_m * f_s[:, None, None, :], "cu_gate_arg", cut)) * f_m
    return cc + f_c + gated.unsqueeze(3)


def _boundary_unit(sd, p, f_b, f_w, f_s, f_m, query_mask, length_mask, cut):
    dt = f_b.dtype
    B, L, D = f_b.shape
    lm = length_mask.to(dt)
    lcol = lm.unsqueeze(-1)
    qrow = query_mask.to(dt).reshape(B, 1, -1)
    baq = _word_attention(sd, p + "attn_layer.", f_b, f_w, f_w, qrow, D, cut, "bu") * lcol
    bq = f_b * (baq + _at(f_s, "bu_fs_in_bq", cut).unsqueeze(1))
    z = bq @ bq.transpose(1, 2) / math.sqrt(D)
    lrow = lm.unsqueeze(1)
    z = (z * lrow).masked_fill(lrow == 0, -1e9)
    A = torch.softmax(_at(z, "bu_self_logits", cut), dim=-1) * lcol
    bb = (A @ f_b) * lcol
    h = torch.sigmoid(_at(f_m * f_s[:, None, None, :], "bu_gate_arg", cut)) * f_m
    bm = (_at(A, "bu_A_in_bm", cut).unsqueeze(3) * h).sum(dim=2)
    return bb + f_b + bm


def _moment_unit(sd, p, f_c, f_m, f_b, moment_mask, cut):
    dt = f_m.dtype
    D = f_m.shape[-1]
    m = moment_mask.to(dt).unsqueeze(-1)
    wfb = sd[p + "conv_layer_fb.weight"].to(dt).reshape(D, D)
    wfc = sd[p + "conv_layer_fc.weight"].to(dt).reshape(D, D)
    pair = _at(f_b.unsqueeze(2) * f_b.unsqueeze(1), "mu_pair", cut)
    y_fb = (pair @ wfb.t() + sd[p + "conv_layer_fb.bias"].to(dt)) * m
    y_fc = (_at(f_c.mean(dim=3), "mu_mean_c", cut) @ wfc.t() + sd[p + "conv_layer_fc.bias"].to(dt)) * m
    return y_fb + y_fc + f_m


def cut_forward(sd, cfg, video_features, video_mask, query_features, query_mask, length_mask, moment_mask, cut=None):
    """oracle.smin_oracle.smin_forward, operation for operation, with ``x.detach()`` at the path named by ``cut`` (in every layer).  A
    detach changes no forward value; with cut=None the graph is smin_forward's."""
    assert cut is None or cut in PATHS + INPUT_PATHS, cut
    fv = O.video_encoder(sd, _at(video_features, "in_video", cut), video_mask)
    fs, fw = O.query_encoder(sd, _at(query_features, "in_query", cut), query_mask)
    f = fv * _at(fs, "f_hadamard_fs", cut).unsqueeze(1)
    fc, fm, fb = O.proposal_generation(f, moment_mask, cfg["T"], cfg["L"], cfg["C"])
    for k in range(O.num_layers(sd)):
        p = f"smis.{k}."
        cu = _content_unit(sd, p + "content_unit.", fc, fw, fs, fm, query_mask, moment_mask, cut)
        bu = _boundary_unit(sd, p + "boundary_unit.", fb, fw, fs, fm, query_mask, length_mask, cut)
        fm = _moment_unit(sd, p + "moment_unit.", cu, fm, bu, moment_mask, cut)
        fc, fb = cu, bu
    return O.localization(sd, fm, fb, length_mask, moment_mask)


def oracle_loss(out, b):
    return O.loss_fn(out[0], b["ym"], b["sm"], b["moment_mask"], out[1], b["ys"], b["ss"], out[2], b["ye"], b["se"], out[3], b["ya"],
                     b["length_mask"])


def reference(sd, cfg, batch, dtype=torch.float64, cut=None, forward=cut_forward):
    """Scores, loss, parameter gradients and the two input gradients of one oracle run in ``dtype``."""
    sdg = {k: v.to(dtype).requires_grad_(True) for k, v in sd.items()}
    b = {k: (v.to(dtype) if v.dtype.is_floating_point else v) for k, v in batch.items()}
    vf, qf = b["video_features"].requires_grad_(True), b["query_features"].requires_grad_(True)
    args = (sdg, dict(T=cfg["T"], L=cfg["L"], C=cfg["C"]), vf, b["video_mask"], qf, b["query_mask"], b["length_mask"], b["moment_mask"])
    out = forward(*args) if forward is O.smin_forward else forward(*args, cut=cut)
    loss = oracle_loss(out, b)
    loss.backward()
    grads = {k: (v.grad if v.grad is not None else torch.zeros_like(v)).detach() for k, v in sdg.items()}
    for name, x in (("video_features", vf), ("query_features", qf)):
        grads["input:" + name] = (x.grad if x.grad is not None else torch.zeros_like(x)).detach()
    return [o.detach() for o in out], float(loss.detach()), grads


# ---------------------------------------------------------------- the cases
# name: (T, L, C, D, dl, layers, Din, Nq, H, B), the constants of alive_state_dict, the seed of synthetic_batch (odd samples are ragged:
# fewer frames and a shorter query).  Shapes are the smallest that reach each form; constants and seeds were chosen on the CPU, by the
# five conditions below, before anything ran on a GPU.
CASES = {
    # NATIVE_ROWS[0] of tests/support/corpora.py, attention form <64,4,T>: the node, the node with input gradients, and both Python hosts
    "native2": ((64, 16, 4, 128, 64, 2, 40, 9, 64, 3), dict(START, lstm=3.5, loc=0.2), 208),
    # test_against_oracle_random's first row: two ragged samples with short queries among five
    "ragged5": ((64, 16, 4, 64, 32, 2, 40, 9, 32, 5), dict(START, loc=0.2), 144),
    # B = 9 at L = 8: the second sample group of the moment unit's and the proposal map's sample dealing.  The loss is a mean over the
    # samples, so gradients are a ninth: the batch seed is the one of {T+L+D, 1, 2, 3} whose scores leave room for loc = 0.3
    "b9": ((32, 8, 4, 64, 16, 2, 24, 6, 32, 9), dict(START, hat=3.0, conv=0.5, loc=0.3), 3),
    # 3 layers, the deepest at which formula weights still hide six paths (condition 5): the layer count every BASELINE config uses
    "deep3": ((64, 16, 4, 64, 32, 3, 40, 9, 32, 3), dict(START, lstm=3.5, conv=0.5, loc=0.2), 144),
    # 5 layers: the content stream's history spills into a second 4-wide partition.  Every layer adds f_m to f_c and doubles f_b, so
    # what feeds the residual sums is damped (ve, lstm, conv) until scores and the fp32 oracle hold conditions 1 to 4.  Condition 5
    # cannot hold at this depth on any shape tried: formula weights saturate the scores there and so see most paths (they hide 2 or
    # 3 of the 14 at 4 and 5 layers); the case asserts that failure of theirs instead (SATURATED_UNDER_FORMULA)
    "deep5": ((32, 8, 4, 64, 16, 5, 24, 6, 32, 2), dict(lstm=2.0, ve=0.75, attn=4.0, hat=2.5, conv=0.4, loc=0.18), 104),
}
SATURATED_UNDER_FORMULA = ["deep5"]
INPUT_GRAD_CASE = "native2"


def case_cfg(case):
    return dict(zip(KEYS, CASES[case][0]))


def case_batch(case):
    c = case_cfg(case)
    return O.synthetic_batch(c["B"], c["T"], c["L"], c["Nq"], c["Din"], seed=CASES[case][2])


def case_weights(case, weights="alive"):
    shapes = H.smin_shapes(*CASES[case][0][:-1])
    return alive_state_dict(shapes, CASES[case][1]) if weights == "alive" else O.formula_state_dict(shapes, gain=1.2)


@functools.lru_cache(maxsize=None)
def ref_of(case, weights="alive", dtype=torch.float64, cut=None):
    """One oracle run of a case, computed once and shared (read-only) by every test that needs it."""
    return reference(case_weights(case, weights), case_cfg(case), case_batch(case), dtype, cut)


def names_of(case, grads, inputs=False):
    """The gradients a case is judged on: every parameter, and the two input gradients where the GPU test compares them."""
    return [k for k in grads if inputs or not k.startswith("input:")]


def visibility(case, path, weights="alive"):
    """Largest change of a gradient under the cut, in units of that gradient's tolerance; and its name."""
    full, cut = ref_of(case, weights)[2], ref_of(case, weights, cut=path)[2]
    inputs = path in INPUT_PATHS
    return max((float((cut[k] - full[k]).abs().max()) / tol_of(full[k]), k) for k in names_of(case, full, inputs))


def true_zero(name):
    return name.endswith("W_k.bias")                   # a shift of every logit of a softmax row: the true gradient is 0


def fp32_noise(case, inputs=False):
    """The fp32 CPU oracle's gradient error against fp64, in units of the tolerance, per gradient."""
    g64, g32 = ref_of(case)[2], ref_of(case, dtype=torch.float32)[2]
    return {k: float((g32[k].double() - g64[k]).abs().max()) / tol_of(g64[k]) for k in names_of(case, g64, inputs) if not true_zero(k)}


def valid_scores(case, weights="alive"):
    out, b = ref_of(case, weights)[0], case_batch(case)
    mm, lm = b["moment_mask"], b["length_mask"]
    return torch.cat([out[0][mm], out[1][lm], out[2][lm], out[3][lm]])


def paths_of(case):
    return PATHS + (INPUT_PATHS if case == INPUT_GRAD_CASE else [])


# ---------------------------------------------------------------- CPU: the conditions, on the reference alone
@pytest.mark.parametrize("case", list(CASES))
def test_restatement_equals_the_oracle(case):
    """cut_forward with no cut is smin_forward: scores, loss and every gradient bit for bit in fp64."""
    ours = ref_of(case)
    theirs = reference(case_weights(case), case_cfg(case), case_batch(case), forward=O.smin_forward)
    for a, b in zip(ours[0], theirs[0]):
        assert torch.equal(a, b)
    assert ours[1] == theirs[1]
    assert set(ours[2]) == set(theirs[2])
    for k in ours[2]:
        assert torch.equal(ours[2][k], theirs[2][k]), k


def test_alive_weights_are_formula_weights_scaled():
    shapes = H.smin_shapes(*CASES["native2"][0][:-1])
    base, alive = O.formula_state_dict(shapes, gain=1.2), alive_state_dict(shapes, START)
    hits = {g: 0 for g in GROUPS}
    for k in base:
        hit = [g for g, member in GROUPS.items() if member(k)]
        for g in hit:
            hits[g] += 1
        assert torch.equal(alive[k], base[k] * (START[hit[0]] if hit else 1.0)), k
    assert all(hits.values()), hits
    assert hits["lstm"] == 16 and hits["ve"] == 2 and hits["attn"] == 16 and hits["hat"] == 12 and hits["conv"] == 12 and hits["loc"] == 8
    assert torch.equal(alive["backbone.videoencoder.pe.weight"], base["backbone.videoencoder.pe.weight"])


@pytest.mark.parametrize("case,path", [(c, p) for c in CASES for p in paths_of(c)])
def test_cut_is_visible(case, path):
    """Condition 1: with the path cut, at least one gradient moves by 5x its tolerance or more."""
    worst, name = visibility(case, path)
    print(f"{case} {path}: {worst:.1f} x tolerance at {name}")
    assert worst >= 5.0, (case, path, worst, name)


@pytest.mark.parametrize("case", list(CASES))
def test_no_gradient_under_the_floor(case):
    """Condition 2: the absolute floor 1e-7 of the bound is at most 1e-3 of every gradient's maximum (W_k.bias apart)."""
    g = ref_of(case)[2]
    small = {k: float(g[k].abs().max()) for k in names_of(case, g, case == INPUT_GRAD_CASE) if not true_zero(k)}
    k = min(small, key=small.get)
    print(f"{case}: smallest max|grad| {small[k]:.3g} at {k}")
    assert 1e-7 <= 1e-3 * small[k], (case, k, small[k])


@pytest.mark.parametrize("case", list(CASES))
def test_scores_are_unsaturated(case):
    """Condition 3: every valid pm, ps, pe, pa lies in (0.02, 0.98)."""
    v = valid_scores(case)
    print(f"{case}: valid scores in {float(v.min()):.4f} .. {float(v.max()):.4f}")
    assert float(v.min()) > 0.02 and float(v.max()) < 0.98


@pytest.mark.parametrize("case", list(CASES))
def test_fp32_oracle_is_conditioned(case):
    """Condition 4: the fp32 CPU oracle's gradients lie within a quarter of the tolerance of the fp64 oracle's."""
    noise = fp32_noise(case, case == INPUT_GRAD_CASE)
    k = max(noise, key=noise.get)
    print(f"{case}: fp32 noise {noise[k]:.3f} x tolerance at {k}")
    assert noise[k] <= 0.25, (case, k, noise[k])


@pytest.mark.parametrize("case", list(CASES))
def test_formula_weights_fall_short(case):
    """Condition 5, the reason this file exists: under formula_state_dict the same case hides six paths or more.  (The 5-layer case
    falls short the other way: its scores saturate and its fp32 oracle leaves the fp64 one, conditions 3 and 4.)  Then the per-case
    table: every path under both weight families, weakest path, smallest gradient maximum, score range, fp32 noise."""
    old = {p: visibility(case, p, "formula") for p in PATHS}
    hidden = [p for p in PATHS if old[p][0] < 5.0]
    new = {p: visibility(case, p) for p in paths_of(case)}
    print(f"\n{case} {CASES[case][0]} {CASES[case][1]} seed {CASES[case][2]}")
    print(f"  {'path':<16}{'formula':>10}{'alive':>10}   (largest gradient change, x tolerance)")
    for p in paths_of(case):
        print(f"  {p:<16}{old[p][0] if p in old else float('nan'):>10.2f}{new[p][0]:>10.1f}")
    g, v, noise = ref_of(case)[2], valid_scores(case), fp32_noise(case)
    weakest = min(new, key=lambda p: new[p][0])
    print(f"  weakest path {weakest} {new[weakest][0]:.1f}x; smallest max|grad| {min(float(g[k].abs().max()) for k in names_of(case, g) if not true_zero(k)):.3g};"
          f" scores {float(v.min()):.3f}..{float(v.max()):.3f}; fp32 noise {max(noise.values()):.3f}x; loss {ref_of(case)[1]:.3f}; formula hides {len(hidden)}")
    if case in SATURATED_UNDER_FORMULA:
        g64, g32 = ref_of(case, "formula")[2], ref_of(case, "formula", torch.float32)[2]
        old_noise = max(float((g32[k].double() - g64[k]).abs().max()) / tol_of(g64[k]) for k in names_of(case, g64) if not true_zero(k))
        v = valid_scores(case, "formula")
        outside = float(((v <= 0.02) | (v >= 0.98)).double().mean())
        print(f"  formula weights: {outside:.0%} of the valid scores outside (0.02, 0.98); fp32 noise {old_noise:.0f}x; loss {ref_of(case, 'formula')[1]:.2f}")
        assert outside > 0.5 and old_noise > 100.0, (case, outside, old_noise)
    else:
        assert len(hidden) >= 6, (case, hidden)


def test_the_ragged_case_is_ragged():
    b = case_batch("ragged5")
    frames, words = b["video_mask"].sum((1, 2)), b["query_mask"].sum((1, 2))
    assert int((frames < 64).sum()) >= 2 and int((words < 9).sum()) >= 2 and int(b["length_mask"].sum(1).min()) < 16


# ---------------------------------------------------------------- GPU: the three hosts against the fp64 oracle on the alive weights
# A bound raised above 2e-3 * max|ref| + 1e-7: (case, gradient) -> (fp32 CPU oracle's error against fp64, bound), both in units of that
# tolerance.  A bound may be at most 8x the fp32 oracle's own error (its noise, with room for another summation order) and never above
# 1e-2 relative (5x the tolerance).  The bounds here are 2x the oracle's error: set from the reference, before and whatever the GPU gave.
#
#   case   gradient                                   max|ref| (fp64)   fp32 oracle   node      stream    bound
#   deep5  smis.4.content_unit.attn_layer.W_k.bias    2.8e-17           0.894x        1.118x    1.118x    1.8x
#
# W_k.bias shifts every logit of a softmax row alike, so its true gradient is 0 and the bound is the bare floor, 1e-7: what any fp32
# evaluation returns there is the rounding residue of a sum that cancels, eps * sum|dS| over 2 * 36 * 4 rows of the largest layer's dS.
# The fp32 CPU oracle leaves 0.89e-7 and both hosts 1.12e-7 (one kernel, the same value): no defect, the floor is simply that close.
RAISED = {
    ("deep5", "smis.4.content_unit.attn_layer.W_k.bias"): (0.894, 1.8),
}


def test_raised_bounds_stay_within_the_reference_noise():
    for (case, name), (noise, bound) in RAISED.items():
        g64, g32 = ref_of(case)[2], ref_of(case, dtype=torch.float32)[2]
        measured = float((g32[name].double() - g64[name]).abs().max()) / tol_of(g64[name])
        print(f"{case} {name}: fp32 oracle {measured:.3f} x tolerance, bound {bound} x")
        # (a rounding residue: it moves with the CPU's summation order, so the recorded figure is held to a factor of 2)
        assert 0.5 * noise <= measured <= 2.0 * noise, (case, name, measured, noise)
        assert 1.0 < bound <= min(8.0 * noise, 8.0 * measured, 5.0), (case, name, bound, measured)


def run_case(dev, case, plan, input_grads=False, **switches):
    """One forward and backward of a case on the GPU under the given switches of SMIN; scores against the fp64 oracle to SCORE_TOL, every
    parameter gradient (and with input_grads the two input gradients) to 2e-3 * max|ref| + 1e-7.  Prints every figure, then asserts."""
    import models
    from vml_amd import loss_fn
    cfg, batch = case_cfg(case), case_batch(case)
    m = models.SMIN(cfg["T"], cfg["L"], cfg["C"], cfg["D"], cfg["dl"], cfg["layers"], cfg["Din"], cfg["Nq"], cfg["H"], dev)
    loaded = m.load_state_dict(case_weights(case), strict=True)
    assert not loaded.missing_keys and not loaded.unexpected_keys
    m = m.to(dev)
    for k, v in dict(switches, input_grads=input_grads).items():
        assert hasattr(m, k), k
        setattr(m, k, v)
    b = {k: v.to(dev) for k, v in batch.items()}
    xs = list(H.model_inputs(b))
    if input_grads:
        xs[0], xs[2] = xs[0].clone().requires_grad_(True), xs[2].clone().requires_grad_(True)
    assert m._plan(xs[0], xs[2]) == plan
    out = m(*xs)
    ref_out, ref_loss, ref_g = ref_of(case)
    bad = []
    for name, got, ref in zip(("pm", "ps", "pe", "pa"), out, ref_out):
        err = float((got.detach().cpu().double() - ref).abs().max())
        print(f"{case} {plan} {name}: max abs err {err:.3g}")
        if not err < SCORE_TOL:
            bad.append((name, err))
    loss = loss_fn(out[0], b["ym"], b["sm"], b["moment_mask"], out[1], b["ys"], b["ss"], out[2], b["ye"], b["se"], out[3], b["ya"], b["length_mask"])
    loss.backward()
    print(f"{case} {plan} loss {float(loss.detach()):.6f} oracle {ref_loss:.6f}")
    got_g = {k: p.grad for k, p in m.named_parameters()}
    if input_grads:
        got_g["input:video_features"], got_g["input:query_features"] = xs[0].grad, xs[2].grad
    assert set(got_g) == set(names_of(case, ref_g, input_grads))
    worst = (0.0, None)
    for k, g in got_g.items():
        assert g is not None and g.shape == ref_g[k].shape, k
        ratio = float((g.detach().cpu().double() - ref_g[k]).abs().max()) / tol_of(ref_g[k])
        worst = max(worst, (ratio, k))
        bound = RAISED.get((case, k), (None, 1.0))[1]
        if ratio > 0.25 or ratio > bound:
            print(f"{case} {plan} {k}: {ratio:.3f} x tolerance (max|ref| {float(ref_g[k].abs().max()):.3g})")
        if not ratio <= bound:
            bad.append((k, ratio))
    print(f"{case} {plan}: worst gradient {worst[0]:.3f} x tolerance at {worst[1]}")
    assert not bad, (case, plan, bad)
    return m, xs


@pytest.mark.gpu
@pytest.mark.parametrize("plan,switches", [("node", {}), ("stream", dict(fused_core=False)), ("units", dict(content_stream=False))],
                         ids=["node", "stream", "units"])
def test_two_layers_on_each_plan(dev, plan, switches):
    """The one-node extension, the Python host with the content stream and the Python host with the content units as written."""
    run_case(dev, "native2", plan, **switches)


@pytest.mark.gpu
def test_node_with_input_gradients(dev):
    """The one-node step with input_grads: video_features.grad and query_features.grad too; padded frames' rows are exactly 0."""
    m, xs = run_case(dev, INPUT_GRAD_CASE, "node", input_grads=True)
    pad = xs[1].reshape(xs[0].shape[0], -1) == 0
    assert pad.any() and bool((xs[0].grad[pad] == 0).all())


@pytest.mark.gpu
@pytest.mark.parametrize("case,plan,switches", [
    ("ragged5", "node", {}),                            # ragged lengths and short queries
    ("b9", "node", {}),                                 # the second sample group of the sample dealing
    ("deep3", "node", {}),
    ("deep5", "node", {}),                              # the second partition of the content stream's history, in the node ...
    ("deep5", "stream", dict(fused_core=False)),        # ... and in the Python host
], ids=["ragged5", "b9", "deep3", "deep5", "deep5-stream"])
def test_cases_against_the_oracle(dev, case, plan, switches):
    run_case(dev, case, plan, **switches)
