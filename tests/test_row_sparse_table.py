"""Row-sparse training of the word table (csrc/row_sparse.hip, sampling.RowSparseGrad, optim.RowSparseAdam):
the compact gradient of embed_tokens against the dense kernel bit for bit, the lazy Adam step against RowSparseAdamTorch -- the same
arithmetic as plain torch ops, run on the CPU -- and against FusedAdam bit for bit, the non-finite guard, checkpoints in
torch.optim.Adam's format, one step through the model, the refusals; on the CPU, RowSparseAdamTorch against FusedAdamTorch and
against torch.optim.SparseAdam."""
import copy
import math

import pytest
import torch

from tests.support.device import dev  # noqa: F401  (the module's device fixture)
from tests.support.device import vml as A
from tests.support.compare import same_state
from tests.support.corpora import build_model, loss_of_batch as loss_of, one_node_only
from tests.support.references import backward_dense, backward_rows, batches

gpu = pytest.mark.gpu


def draw_tokens(case, g):
    B, Nq, V, E = case[:4]
    if len(case) > 4:                                                    # every id out of range
        return torch.where(torch.rand(B, Nq, generator=g) < 0.5, torch.tensor(-1), torch.tensor(V + 3)).to(torch.int64)
    tok = torch.randint(0, V, (B, Nq), generator=g)
    if (B, Nq, V) == (3, 5, 11):                                         # ids -1 and V mixed in, and repeats
        tok = torch.tensor([[4, -1, 4, 11, 0], [10, 4, 11, 7, 7], [-1, 0, 10, 4, 2]])
    return tok


ROWS_CASES = [(3, 5, 11, 4), (4, 8, 7, 300), (1, 1, 5, 8), (128, 32, 50, 12), (128, 32, 100000, 4), (3, 5, 11, 4, "none in range")]


@gpu
@pytest.mark.parametrize("case", ROWS_CASES, ids=lambda c: "-".join(str(x) for x in c).replace(" ", "_"))
def test_rows_equal_the_dense_gradient_bitwise(dev, case):
    """ids[:count] = the sorted distinct in-range ids, rows[:count] = those rows of the dense kernel's gradient (torch.equal),
    ids[count:] = -1, to_dense() = the dense gradient, sq_norm within 1e-9 relative of the fp64 sum of squares of the dense gradient
    (at most 4096 * 300 fp64 additions: below 1.4e-10)."""
    B, Nq, V, E = case[:4]
    g = torch.Generator().manual_seed(B * 1000 + Nq + V)
    tok = draw_tokens(case, g)
    dqf = (torch.randn(B, Nq, E, generator=g) * 10.0 ** torch.randint(-3, 3, (B, Nq, 1), generator=g).float()).to(dev)
    table = torch.randn(V, E, generator=g).to(dev).requires_grad_(True)
    dense = backward_dense(tok.to(dev), table, dqf).clone()
    table.grad = None
    rg = backward_rows(tok.to(dev), table, dqf)
    want = torch.unique(tok[(tok >= 0) & (tok < V)])                     # sorted
    count = int(rg.count.item())
    assert rg.ids.dtype == torch.int32 and rg.ids.shape == (B * Nq,) and rg.rows.shape == (B * Nq, E) and rg.shape == (V, E)
    assert count == want.numel()
    if len(case) > 4:
        assert count == 0
    assert torch.equal(rg.ids[:count].cpu().long(), want)
    assert bool((rg.ids[count:] == -1).all())
    assert torch.equal(rg.rows[:count], dense[rg.ids[:count].long()])
    assert torch.equal(rg.to_dense(), dense)
    sp = rg.to_sparse_coo()
    assert sp.is_coalesced() and sp._nnz() == count and torch.equal(sp.to_dense(), dense)
    ref = float((dense.double() * dense.double()).sum())
    got = float(rg.sq_norm.item())
    print(case, "count", count, "sq_norm", got, "fp64 of dense", ref, "rel", abs(got - ref) / max(ref, 1e-300))
    assert rg.sq_norm.dtype == torch.float64 and abs(got - ref) <= 1e-9 * ref


@gpu
@pytest.mark.parametrize("scaled", [False, True], ids=["unscaled", "scaled"])
@pytest.mark.parametrize("shape", [(3, 5, 11, 4), (4, 8, 40, 300)], ids=["11x4", "40x300"])
def test_step_equals_the_torch_restatement_bitwise(dev, shape, scaled):
    """6 steps, another batch each, the whole table, both moments and state[:3] against RowSparseAdamTorch on the CPU after every step
    (so rows the batch did not touch are shown untouched); a step with nothing pending is a no-op; a step whose batch has no id in
    range advances t and nothing else."""
    B, Nq, V, E = shape
    g = torch.Generator().manual_seed(3)
    init = torch.randn(V, E, generator=g)
    table = init.clone().to(dev).requires_grad_(True)
    rtable = init.clone().requires_grad_(True)
    opt = A().RowSparseAdam(table, lr=3e-3, betas=(0.8, 0.99), eps=1e-7)
    ref = A().RowSparseAdamTorch(rtable, lr=3e-3, betas=(0.8, 0.99), eps=1e-7)
    scale = torch.tensor([torch.tensor(0.37, dtype=torch.float32).item()], dtype=torch.float64, device=dev) if scaled else None
    for k, (tok, dqf) in enumerate(batches(B, Nq, V, E, 6, seed=V)):
        rg = backward_rows(tok.to(dev), table, dqf.to(dev))
        assert rg.pending
        opt.step(scale=scale)
        assert not rg.pending
        if k % 2:
            ref.step(rg, scale=scale)                                    # a RowSparseGrad ...
        else:
            ref.step((rg.ids.cpu(), rg.rows.cpu()), scale=scale)         # ... or (ids, rows); the unused slots hold -1
        same_state(opt, ref, table, rtable)
        assert opt._state[0].item() == k + 1
        if scaled:
            assert opt.clip_coef.item() == scale.item()
        assert abs(opt.grad_norm.item() - math.sqrt(rg.sq_norm.item())) <= 1e-15 * opt.grad_norm.item()
        if k == 2:                                                       # nothing pending: no-op, t unchanged
            before = opt._state.clone()
            opt.step(scale=scale)
            ref.step(scale=scale)
            assert torch.equal(opt._state, before)
            same_state(opt, ref, table, rtable)
    before = [x.clone() for x in (table.detach(), opt.state[table]["exp_avg"], opt.state[table]["exp_avg_sq"])]
    rg = backward_rows(torch.full((B, Nq), V, device=dev), table, torch.ones(B, Nq, E, device=dev))
    assert rg.count.item() == 0
    opt.step(scale=scale)
    ref.step(rg, scale=scale)
    assert opt._state[0].item() == 7
    for x, y in zip(before, (table.detach(), opt.state[table]["exp_avg"], opt.state[table]["exp_avg_sq"])):
        assert torch.equal(x, y)
    same_state(opt, ref, table, rtable)


@gpu
def test_trajectory_equals_fused_adam_when_every_row_is_touched(dev):
    """V = 7, (4, 8, 7, 300), every id present in each of 3 steps: the table's trajectory is FusedAdam([table])'s on the dense gradient."""
    B, Nq, V, E = 4, 8, 7, 300
    init = torch.randn(V, E, generator=torch.Generator().manual_seed(5))
    ta = init.clone().to(dev).requires_grad_(True)
    tb = init.clone().to(dev).requires_grad_(True)
    fused, rows = A().FusedAdam([ta], lr=1e-2), A().RowSparseAdam(tb, lr=1e-2)
    for tok, dqf in batches(B, Nq, V, E, 3, seed=11, cover=True):
        assert torch.unique(tok).numel() == V
        backward_dense(tok.to(dev), ta, dqf.to(dev))
        fused.step()
        backward_rows(tok.to(dev), tb, dqf.to(dev))
        rows.step()
        assert torch.equal(ta.detach(), tb.detach())
        assert torch.equal(fused.state[ta]["exp_avg"], rows.state[tb]["exp_avg"])
        assert torch.equal(fused.state[ta]["exp_avg_sq"], rows.state[tb]["exp_avg_sq"])
        assert torch.equal(fused._state[:4], rows._state[:4])


@gpu
@pytest.mark.parametrize("what", ["nan_gradient", "inf_scale"])
def test_nonfinite_guard(dev, what):
    """With skip_nonfinite a NaN in dqf, or scale = inf, leaves table, moments and t alone and counts one skipped step; without it the
    touched rows become non-finite and the others keep their bits."""
    B, Nq, V, E = 3, 5, 11, 4
    (tok0, dqf0), (tok, dqf) = batches(B, Nq, V, E, 2, seed=2)
    if what == "nan_gradient":
        b, w = [(b, w) for b in range(B) for w in range(Nq) if 0 <= tok[b, w] < V][0]
        dqf[b, w, 1] = math.nan
        bad_ids, scale = torch.tensor([int(tok[b, w])]), None
    else:
        bad_ids, scale = torch.unique(tok[(tok >= 0) & (tok < V)]), torch.tensor([math.inf], dtype=torch.float64, device=dev)
    init = torch.randn(V, E, generator=torch.Generator().manual_seed(1))
    for guard in (True, False):
        table = init.clone().to(dev).requires_grad_(True)
        opt = A().RowSparseAdam(table, skip_nonfinite=guard)
        backward_rows(tok0.to(dev), table, dqf0.to(dev))
        opt.step()                                                       # one good step: non-zero moments
        before = [x.clone() for x in (table.detach(), opt.state[table]["exp_avg"], opt.state[table]["exp_avg_sq"], opt._state[:3])]
        backward_rows(tok.to(dev), table, dqf.to(dev))
        opt.step(scale=scale)
        after = (table.detach(), opt.state[table]["exp_avg"], opt.state[table]["exp_avg_sq"], opt._state[:3])
        if guard:
            for x, y in zip(before, after):
                assert torch.equal(x, y)
            assert opt.skipped_steps.item() == 1 and opt._state[0].item() == 1 and opt._state[7].item() == 1
        else:
            assert opt.skipped_steps.item() == 0 and opt._state[0].item() == 2
            finite = torch.isfinite(after[0]).all(1).cpu()
            other = torch.ones(V, dtype=torch.bool)
            other[bad_ids] = False
            assert not finite[bad_ids].any() and finite[other].all()
            untouched = torch.ones(V, dtype=torch.bool)
            untouched[torch.unique(tok[(tok >= 0) & (tok < V)])] = False
            assert untouched.any() and torch.equal(after[0][untouched.to(dev)], before[0][untouched.to(dev)])


@gpu
def test_checkpoint_resumes_bit_for_bit(dev):
    """Saved after 2 steps and loaded into a fresh optimizer: 2 more steps equal 4 uninterrupted ones; a torch.optim.Adam state dict of
    the same shape loads."""
    B, Nq, V, E = 4, 8, 40, 300
    bs = batches(B, Nq, V, E, 4, seed=9)
    init = torch.randn(V, E, generator=torch.Generator().manual_seed(4))

    def run(table, opt, some):
        for tok, dqf in some:
            backward_rows(tok.to(dev), table, dqf.to(dev))
            opt.step()

    ta = init.clone().to(dev).requires_grad_(True)
    oa = A().RowSparseAdam(ta, lr=2e-3)
    run(ta, oa, bs)
    tb = init.clone().to(dev).requires_grad_(True)
    ob = A().RowSparseAdam(tb, lr=2e-3)
    run(tb, ob, bs[:2])
    sd = copy.deepcopy(ob.state_dict())
    assert float(sd["state"][0]["step"]) == 2 and sd["state"][0]["exp_avg"].shape == (V, E)
    tc = tb.detach().clone().requires_grad_(True)
    oc = A().RowSparseAdam(tc, lr=1.0)
    oc.load_state_dict(sd)
    assert oc.param_groups[0]["lr"] == 2e-3
    run(tc, oc, bs[2:])
    assert torch.equal(tc.detach(), ta.detach())
    assert torch.equal(oc.state[tc]["exp_avg"], oa.state[ta]["exp_avg"]) and torch.equal(oc.state[tc]["exp_avg_sq"], oa.state[ta]["exp_avg_sq"])
    assert torch.equal(oc._state[:4], oa._state[:4])
    # torch.optim.Adam's own dict
    pt = torch.nn.Parameter(init.clone())
    theirs = torch.optim.Adam([pt], lr=5e-4, betas=(0.7, 0.9))
    pt.grad = torch.randn(V, E, generator=torch.Generator().manual_seed(6))
    theirs.step()
    od = A().RowSparseAdam(init.clone().to(dev).requires_grad_(True))
    od.load_state_dict(theirs.state_dict())
    assert od._state[:4].tolist() == [1.0, 0.7, 0.9, 5e-4]
    assert torch.equal(od.state[od.table]["exp_avg"].cpu(), theirs.state[pt]["exp_avg"])
    assert torch.equal(od.state[od.table]["exp_avg_sq"].cpu(), theirs.state[pt]["exp_avg_sq"])


@gpu
def test_end_to_end_through_the_model(dev):
    """The configuration of tests/test_input_grads.py::test_table_gradient_end_to_end: after backward() the row gradient's to_dense()
    equals the dense path's table.grad bit for bit; one FusedAdam + RowSparseAdam step then leaves the rows of ids absent from the
    batch untouched and changes the rows of the ids the queries hold."""
    from oracle import smin_oracle as O
    from tests import helpers as H
    T, L, C, D, dl, layers, Din, Nq, Hh, B, V = 64, 16, 4, 64, 32, 2, 40, 9, 32, 5, 60
    sd = O.formula_state_dict(H.smin_shapes(T, L, C, D, dl, layers, Din, Nq, Hh), gain=1.2)
    batch = O.synthetic_batch(B, T, L, Nq, Din, seed=17)
    g = torch.Generator().manual_seed(17)
    tok = torch.randint(0, V - 1, (B, Nq), generator=g)
    tok[batch["query_mask"].reshape(B, Nq) == 0] = V - 1                 # <pad>
    init = torch.randn(V, 300, generator=g) * 0.5
    m = build_model(dict(T=T, L=L, C=C, D=D, dl=dl, layers=layers, Din=Din, Nq=Nq, H=Hh), sd, dev)
    m.input_grads = True
    one_node_only(m)
    b = {k: v.to(dev) for k, v in batch.items()}

    def backward(table, sparse):
        m.zero_grad(set_to_none=True)
        qf, qm, _ = A().embed_tokens(tok.to(dev), table, differentiable=True, sparse_grad=sparse)
        inp = H.model_inputs(b)
        inp[2] = qf * qm.unsqueeze(-1).float()
        loss_of(m(*inp), b).backward()

    td = init.clone().to(dev).requires_grad_(True)
    backward(td, False)
    ts = init.clone().to(dev).requires_grad_(True)
    backward(ts, True)
    assert ts.grad is None and td.grad.abs().max().item() > 0
    assert torch.equal(ts.row_grad.to_dense(), td.grad)
    opt = A().FusedAdam(list(m.parameters()), lr=1e-3, max_norm=1.0)
    topt = A().RowSparseAdam(ts, lr=1e-3)
    opt.step()
    topt.step(scale=opt.clip_coef)
    assert topt.clip_coef.item() == opt.clip_coef.item()
    present = torch.zeros(V, dtype=torch.bool)
    present[torch.unique(tok)] = True
    assert (~present).any()
    new = ts.detach().cpu()
    assert torch.equal(new[~present], init[~present])
    words = torch.unique(tok[tok != V - 1])                              # <pad> is present, but its rows' gradient is zero
    assert bool((new[words] != init[words]).any(1).all())


@gpu
def test_refusals(dev):
    Err = A()._lib.SminHipError
    table = torch.randn(11, 8, device=dev, requires_grad=True)
    tok = torch.randint(0, 11, (3, 5), device=dev)
    qf, _, _ = A().embed_tokens(tok, table, differentiable=True, sparse_grad=True)
    qf.backward(torch.ones_like(qf), retain_graph=True)
    with pytest.raises(RuntimeError, match="pending"):                   # a second backward while a gradient is pending
        qf.backward(torch.ones_like(qf), retain_graph=True)
    table.row_grad.clear()
    qf.backward(torch.ones_like(qf), retain_graph=True)
    opt = A().RowSparseAdam(table)
    opt.zero_grad()
    qf.backward(torch.ones_like(qf))
    opt.step()
    with pytest.raises(ValueError, match="differentiable"):
        A().embed_tokens(tok, table, sparse_grad=True)
    with pytest.raises(ValueError, match="4096"):
        A().embed_tokens(torch.zeros(4097, 1, dtype=torch.int64, device=dev), table, differentiable=True, sparse_grad=True)
    with pytest.raises(Err, match="no CPU fallback"):
        A().embed_tokens(tok.cpu(), table.detach().cpu().requires_grad_(True), differentiable=True, sparse_grad=True)
    with pytest.raises(Err, match="no CPU fallback"):
        A().RowSparseAdam(torch.randn(11, 8, requires_grad=True))
    wide = torch.randn(11, 16, device=dev)
    for bad, why in ((wide[:, :8].requires_grad_(True), "contiguous"), (torch.randn(11, 8, device=dev, dtype=torch.float64).requires_grad_(True), "fp32|float64")):
        with pytest.raises(ValueError, match=why):
            A().embed_tokens(tok, bad, differentiable=True, sparse_grad=True)
        with pytest.raises(ValueError, match="RowSparseAdam.*(" + why + ")"):
            A().RowSparseAdam(bad)
    with pytest.raises(ValueError, match="weight_decay"):
        A().RowSparseAdam(table, weight_decay=1e-2)
    for key in ("amsgrad", "maximize"):
        with pytest.raises(ValueError, match="RowSparseAdam: amsgrad and maximize"):
            A().RowSparseAdam(table, **{key: True})


# ---------------------------------------------------------------- CPU
def test_torch_restatement_equals_fused_adam_torch_when_every_row_is_listed():
    """RowSparseAdamTorch with every row listed against FusedAdamTorch on the dense gradient, bit for bit over 3 steps."""
    V, E = 13, 8
    g = torch.Generator().manual_seed(0)
    init = torch.randn(V, E, generator=g)
    pa, pb = torch.nn.Parameter(init.clone()), torch.nn.Parameter(init.clone())
    fused, rows = A().FusedAdamTorch([pa], lr=1e-2), A().RowSparseAdamTorch(pb, lr=1e-2)
    for _ in range(3):
        grad = torch.randn(V, E, generator=g) * 10.0 ** torch.randint(-4, 2, (V, 1), generator=g).float()
        pa.grad = grad.clone()
        fused.step()
        perm = torch.arange(V)
        rows.step((perm, grad[perm]))
        assert torch.equal(pa.detach(), pb.detach())
        assert torch.equal(fused.state[pa]["exp_avg"], rows.state[pb]["exp_avg"])
        assert torch.equal(fused.state[pa]["exp_avg_sq"], rows.state[pb]["exp_avg_sq"])
        assert torch.equal(fused._state[:4], rows._state[:4])


def test_torch_restatement_against_sparse_adam():
    """torch.optim.SparseAdam with eps = 1e-30 on both sides (it refuses 0; with the default eps the two rules differ by design: eps
    sits inside or outside the bias correction), V = 37, E = 8, 20 steps of random row sets and gradients with |g| >= 1e-3: the set of
    changed rows is the same every step, and each step's update p_new - p_old agrees within 32 * 2**-24 of the step's largest update
    (the two formulas place the bias correction differently and are each under 16 roundings).
    What the bound is taken against, and why: (1) both tables are set to zero before every step -- the update does not depend on p,
    and 0 - x is exact, so p_new - p_old is the update itself; with p of order 1 and updates of order lr the difference would carry
    p's own rounding, 2**-24 * |p| / lr, which says nothing about the formulas.  (2) The difference is taken relative to the step's
    largest update, not element by element: the first moments -- beta1 * m + (1 - beta1) * g here, m + (g - m) * (1 - beta1) there --
    are each accurate relative to their terms, not to a sum that cancels, while every update is m / sqrt(v) * lr, of the order of lr
    at most.  The moments themselves carry over from step to step untouched by the zeroing."""
    V, E, lr = 37, 8, 1e-2
    g = torch.Generator().manual_seed(8)
    init = torch.randn(V, E, generator=g)
    pa, pb = torch.nn.Parameter(init.clone()), torch.nn.Parameter(init.clone())
    ours, theirs = A().RowSparseAdamTorch(pa, lr=lr, eps=1e-30), torch.optim.SparseAdam([pb], lr=lr, eps=1e-30)
    worst = 0.0
    for _ in range(20):
        k = int(torch.randint(1, V, (1,), generator=g))
        ids = torch.sort(torch.randperm(V, generator=g)[:k]).values
        rows = torch.randn(k, E, generator=g)
        rows = torch.where(rows.abs() < 1e-3, torch.full_like(rows, 1e-3), rows)
        with torch.no_grad():
            pa.zero_(), pb.zero_()
        a0, b0 = pa.detach().clone(), pb.detach().clone()
        ours.step((ids, rows))
        pb.grad = torch.sparse_coo_tensor(ids.unsqueeze(0), rows, (V, E))
        theirs.step()
        da, db = pa.detach() - a0, pb.detach() - b0
        changed_a, changed_b = (da != 0).any(1), (db != 0).any(1)
        assert torch.equal(changed_a, changed_b) and torch.equal(torch.nonzero(changed_a).view(-1), ids)
        rel = float((da - db).abs().max() / db.abs().max())
        worst = max(worst, rel)
        assert rel <= 32 * 2.0 ** -24, rel
    print("largest difference of an update, relative to the step's largest:", worst)
