"""Merging row-sparse table gradients (smin_row_lists_merge in csrc/row_sparse.hip, sampling.merge_row_grads, embed_tokens(accumulate=True),
distributed.exchange_row_grad): the merged list against dense sums and against merge_row_grads_torch -- the same
additions as plain torch ops, run on the CPU -- bit for bit, one list merged alone against itself, two runs against each other, a merged
list of more than 4096 slots through RowSparseAdam, accumulation over micro-batches against the dense path, shards against the full
batch, the refusals; on the CPU, the gather between two gloo ranks and the restatement against fp64.

The lists come from embed_tokens(sparse_grad=True) on per-list tables; the rows of their slots >= count are overwritten with NaN before
any merge, so a merge that read one would show it."""
import os

import pytest
import torch
import torch.multiprocessing as mp

from tests.support.device import dev  # noqa: F401  (the module's device fixture)
from tests.support.device import free_port, vml as A
from tests.support.compare import same_state

gpu = pytest.mark.gpu


def backward_rows(tok, table, dqf, **kw):
    """embed_tokens(sparse_grad=True) then backward of dqf: table.row_grad"""
    qf, _, _ = A().embed_tokens(tok, table, differentiable=True, sparse_grad=True, **kw)
    qf.backward(dqf)
    assert table.grad is None
    return table.row_grad


def device_bits(x):
    return x.contiguous().view(torch.int32 if x.dtype == torch.float32 else torch.int64)


def draw_dqf(shape, E, g):
    return torch.randn(*shape, E, generator=g) * 10.0 ** torch.randint(-3, 3, (*shape, 1), generator=g).float()


EXPLICIT = [[4, -1, 4, 11, 0], [10, 4, 11, 7, 7], [-1, 0, 10, 4, 2]]     # (3, 5), V = 11: ids 0 and V - 1, -1 and V, repeats


def case_tokens(name, g):
    """-> (V, E, [tokens of list 0, ...])"""
    out_of_range = lambda shape, V: torch.where(torch.rand(*shape, generator=g) < 0.5, torch.tensor(-1), torch.tensor(V + 3))
    if name == "one":
        return 11, 4, [torch.tensor(EXPLICIT)]
    if name == "two":
        return 11, 4, [torch.tensor(EXPLICIT), torch.randint(-1, 12, (3, 5), generator=g)]
    if name == "disjoint":
        return 40, 300, [torch.randint(0, 20, (4, 8), generator=g), torch.randint(20, 40, (4, 8), generator=g)]
    if name == "identical":
        tok = torch.randint(0, 40, (4, 8), generator=g)
        return 40, 300, [tok, tok.clone()]
    if name == "every_id":
        return 13, 8, [torch.randint(0, 13, (2, 8), generator=g) for _ in range(4)]
    if name == "unequal":
        return 50, 12, [torch.randint(0, 50, s, generator=g) for s in ((4, 8), (1, 1), (16, 8))]
    if name == "one_empty":
        return 11, 4, [torch.randint(0, 11, (3, 5), generator=g), out_of_range((3, 5), 11), torch.randint(0, 11, (3, 5), generator=g)]
    if name == "all_empty":
        return 11, 4, [out_of_range((3, 5), 11) for _ in range(3)]
    if name == "chunks":                                                 # N = 6144 and M > 4096: the scan crosses a chunk
        return 100000, 4, [torch.randint(0, 100000, (64, 32), generator=g) for _ in range(3)]
    if name == "sixteen":
        return 7, 4, [torch.randint(0, 7, (1, 4), generator=g) for _ in range(16)]
    raise KeyError(name)


CASES = ["one", "two", "disjoint", "identical", "every_id", "unequal", "one_empty", "all_empty", "chunks", "sixteen"]
_built = {}


def lists_of(name, dev):
    """The case's row gradients (made once, never changed afterwards) and their tokens"""
    if name not in _built:
        g = torch.Generator().manual_seed(100 + CASES.index(name))
        V, E, toks = case_tokens(name, g)
        grads = []
        for tok in toks:
            table = torch.randn(V, E, generator=g).to(dev).requires_grad_(True)
            rg = backward_rows(tok.to(dev), table, draw_dqf(tuple(tok.shape), E, g).to(dev))
            rg.rows[int(rg.count.item()):] = float("nan")
            grads.append(rg)
        _built[name] = (grads, toks, V, E)
    return _built[name]


def union_of(toks, V):
    t = torch.cat([t.reshape(-1) for t in toks])
    return torch.unique(t[(t >= 0) & (t < V)])                           # sorted


def on_cpu(rg):
    return A().RowSparseGrad(rg.ids.cpu(), rg.rows.cpu(), rg.count.cpu(), rg.sq_norm.cpu(), rg.shape)


@gpu
@pytest.mark.parametrize("scale", [None, 0.25], ids=["unscaled", "quarter"])
@pytest.mark.parametrize("name", CASES)
def test_merge_equals_the_dense_sums(dev, name, scale):
    """merged.to_dense() = (((g0.to_dense() + g1.to_dense()) + ...) * scale), torch.equal; the ids are the sorted union, the tail is -1,
    the count is right and everything below the count is finite (the inputs' rows above their counts are NaN)."""
    grads, toks, V, E = lists_of(name, dev)
    merged = A().merge_row_grads(grads, scale=scale)
    want = grads[0].to_dense()
    for rg in grads[1:]:
        want = want + rg.to_dense()
    if scale is not None:
        want = want * scale
    N = sum(t.numel() for t in toks)
    union = union_of(toks, V)
    count = int(merged.count.item())
    assert merged.pending and all(rg.pending for rg in grads) and merged.shape == (V, E)
    assert merged.ids.dtype == torch.int32 and merged.ids.shape == (N,) and merged.rows.shape == (N, E)
    assert count == union.numel()
    assert torch.equal(merged.ids[:count].cpu().long(), union)
    assert bool((merged.ids[count:] == -1).all())
    assert bool(torch.isfinite(merged.rows[:count]).all())
    assert torch.equal(merged.to_dense(), want)
    if name == "chunks":
        M = sum(int(rg.count.item()) for rg in grads)
        assert N == 6144 and M > 4096, (N, M)
    if name == "all_empty":
        assert count == 0 and merged.sq_norm.item() == 0.0


@gpu
@pytest.mark.parametrize("scale", [None, 0.25, 1.0 / 3.0], ids=["unscaled", "quarter", "third"])
@pytest.mark.parametrize("name", CASES)
def test_merge_equals_the_torch_restatement_bitwise(dev, name, scale):
    """ids, count and rows[:count] have the bits of merge_row_grads_torch run on the CPU; sq_norm is within 1e-9 relative of the fp64 sum of
    squares of rows[:count] (at most 6144 * 300 fp64 additions: below 2.1e-10, the reasoning of
    test_row_sparse_table.test_rows_equal_the_dense_gradient_bitwise)."""
    grads, _, V, E = lists_of(name, dev)
    merged = A().merge_row_grads(grads, scale=scale)
    ref = A().merge_row_grads_torch([on_cpu(rg) for rg in grads], scale=scale)
    count = int(ref.count.item())
    assert torch.equal(merged.count.cpu(), ref.count) and ref.pending
    assert torch.equal(merged.ids.cpu(), ref.ids)
    assert torch.equal(device_bits(merged.rows[:count].cpu()), device_bits(ref.rows[:count]))
    sq = float((merged.rows[:count].double() * merged.rows[:count].double()).sum())
    got = float(merged.sq_norm.item())
    print(name, scale, "count", count, "sq_norm", got, "fp64 of rows", sq, "rel", abs(got - sq) / max(sq, 1e-300))
    assert merged.sq_norm.dtype == torch.float64 and abs(got - sq) <= 1e-9 * sq
    assert abs(float(ref.sq_norm) - sq) <= 1e-9 * sq


@gpu
@pytest.mark.parametrize("name", ["one", "chunks"])
def test_one_list_alone_comes_back_bit_for_bit(dev, name):
    """R = 1, no scale: ids, rows[:count], count and the bits of sq_norm are the input's."""
    rg = lists_of(name, dev)[0][0]
    merged = A().merge_row_grads([rg])
    count = int(rg.count.item())
    assert merged is not rg and merged.rows.data_ptr() != rg.rows.data_ptr()
    assert torch.equal(merged.count, rg.count) and torch.equal(merged.ids, rg.ids)
    assert torch.equal(device_bits(merged.rows[:count]), device_bits(rg.rows[:count]))
    assert torch.equal(device_bits(merged.sq_norm), device_bits(rg.sq_norm))


@gpu
def test_two_runs_give_the_same_bits(dev):
    grads = lists_of("chunks", dev)[0]
    a = A().merge_row_grads(grads, scale=1.0 / 3.0)
    b = A().merge_row_grads(grads, scale=1.0 / 3.0)
    count = int(a.count.item())
    assert torch.equal(a.ids, b.ids) and torch.equal(a.count, b.count) and torch.equal(device_bits(a.sq_norm), device_bits(b.sq_norm))
    assert torch.equal(device_bits(a.rows[:count]), device_bits(b.rows[:count]))


@gpu
def test_a_merged_list_of_6144_slots_steps_like_the_restatement(dev):
    """The N = 6144 merged list through RowSparseAdam.step(scale=...) three times: table, both moments and state[:3] equal
    RowSparseAdamTorch on the CPU bit for bit after every step."""
    grads, _, V, E = lists_of("chunks", dev)
    init = torch.randn(V, E, generator=torch.Generator().manual_seed(12))
    table, rtable = init.clone().to(dev).requires_grad_(True), init.clone().requires_grad_(True)
    opt = A().RowSparseAdam(table, lr=3e-3, betas=(0.8, 0.99), eps=1e-7)
    ref = A().RowSparseAdamTorch(rtable, lr=3e-3, betas=(0.8, 0.99), eps=1e-7)
    scale = torch.tensor([torch.tensor(0.37, dtype=torch.float32).item()], dtype=torch.float64, device=dev)
    for k in range(3):
        merged = A().merge_row_grads(grads[k:] + grads[:k], scale=0.5)  # another order of the additions each step
        assert merged.ids.shape[0] == 6144
        table.row_grad = merged
        opt.step(scale=scale)
        assert not merged.pending
        ref.step(merged, scale=scale)
        same_state(opt, ref, table, rtable)
        assert opt._state[0].item() == k + 1
    assert not torch.equal(table.detach().cpu(), init)


@gpu
@pytest.mark.parametrize("shape", [(3, 5, 11, 4), (4, 8, 40, 300)], ids=["11x4", "40x300"])
def test_micro_batches_accumulate_like_the_dense_path(dev, shape):
    """Two backwards with accumulate=True: row_grad.to_dense() = table.grad after the same two backwards on the dense path (torch.equal);
    accumulate=False still refuses a pending gradient; one RowSparseAdam.step() consumes the merged gradient."""
    B, Nq, V, E = shape
    g = torch.Generator().manual_seed(V)
    init = torch.randn(V, E, generator=g)
    batches = [(torch.randint(-1, V + 1, (B, Nq), generator=g).to(dev), draw_dqf((B, Nq), E, g).to(dev)) for _ in range(2)]
    td = init.clone().to(dev).requires_grad_(True)
    ts = init.clone().to(dev).requires_grad_(True)
    for tok, dqf in batches:
        qf, _, _ = A().embed_tokens(tok, td, differentiable=True)
        qf.backward(dqf)
        backward_rows(tok, ts, dqf, accumulate=True)
    rg = ts.row_grad
    assert rg.pending and rg.ids.shape[0] == 2 * B * Nq and ts.grad is None
    assert torch.equal(rg.to_dense(), td.grad)
    with pytest.raises(RuntimeError, match="pending"):
        backward_rows(batches[0][0], ts, batches[0][1])
    assert ts.row_grad is rg
    opt = A().RowSparseAdam(ts)
    opt.step()
    assert not ts.row_grad.pending
    touched = torch.unique(torch.cat([t.reshape(-1) for t, _ in batches]).cpu())
    touched = touched[(touched >= 0) & (touched < V)]
    assert bool((ts.detach().cpu()[touched] != init[touched]).any(1).all())


@gpu
def test_shards_merge_to_the_full_batch(dev):
    """A batch (8, 8) over V = 13, E = 8 split into 4 shards of (2, 8): the merged shard gradients list the ids of the full batch's
    gradient, and per element |merged - fp64 dense| <= k * 2**-24 * sum |addends| with k the id's number of positions (the standard
    bound of a sum of k terms in any order: k - 1 roundings of at most 2**-24 each, relative to the sum of the magnitudes)."""
    B, Nq, V, E, R = 8, 8, 13, 8, 4
    g = torch.Generator().manual_seed(21)
    tok = torch.randint(0, V, (B, Nq), generator=g)
    dqf = draw_dqf((B, Nq), E, g)
    full = backward_rows(tok.to(dev), torch.zeros(V, E, device=dev).requires_grad_(True), dqf.to(dev))
    per = B // R
    shards = [backward_rows(tok[r * per:(r + 1) * per].to(dev), torch.zeros(V, E, device=dev).requires_grad_(True),
                            dqf[r * per:(r + 1) * per].to(dev)) for r in range(R)]
    merged = A().merge_row_grads(shards)
    assert torch.equal(merged.count, full.count) and torch.equal(merged.ids, full.ids)
    flat = tok.reshape(-1)
    exact = torch.zeros(V, E, dtype=torch.float64).index_add_(0, flat, dqf.reshape(-1, E).double())
    mags = torch.zeros(V, E, dtype=torch.float64).index_add_(0, flat, dqf.reshape(-1, E).double().abs())
    k = torch.bincount(flat, minlength=V).double().unsqueeze(1)
    err = (merged.to_dense().cpu().double() - exact).abs()
    bound = k * 2.0 ** -24 * mags
    print("largest error over its bound:", float((err / bound.clamp(min=1e-300)).max()))
    assert bool((err <= bound).all())


def empty_list(n, V, E, dev):
    return A().RowSparseGrad(torch.full((n,), -1, dtype=torch.int32, device=dev), torch.empty((n, E), device=dev),
                             torch.zeros(1, dtype=torch.int32, device=dev), torch.zeros(1, dtype=torch.float64, device=dev), (V, E))


@gpu
def test_refusals(dev):
    Err = A()._lib.SminHipError
    grads, _, V, E = lists_of("sixteen", dev)
    with pytest.raises(ValueError, match="16"):
        A().merge_row_grads(grads + grads[:1])
    with pytest.raises(ValueError, match="16"):
        A().merge_row_grads([])
    with pytest.raises(ValueError, match="same"):
        A().merge_row_grads([grads[0], lists_of("one", dev)[0][0]])      # (7, 4) beside (11, 4)
    with pytest.raises(ValueError, match="same"):
        A().merge_row_grads([grads[0], on_cpu(grads[1])])
    full = empty_list(4096, V, E, dev)
    with pytest.raises(ValueError, match="65536"):
        A().merge_row_grads([full] * 15 + [empty_list(4097, V, E, dev)])
    most = A().merge_row_grads([full] * 16)                              # 65536 slots are taken
    assert most.ids.shape[0] == 65536 and most.count.item() == 0 and most.sq_norm.item() == 0.0 and bool((most.ids == -1).all())
    with pytest.raises(Err, match="no CPU fallback"):
        A().merge_row_grads([on_cpu(rg) for rg in grads[:2]])
    with pytest.raises(ValueError, match="scale"):
        A().merge_row_grads(grads[:2], scale=torch.ones(1, device=dev))
    table = torch.randn(11, 8, device=dev, requires_grad=True)
    tok = torch.randint(0, 11, (3, 5), device=dev)
    with pytest.raises(ValueError, match="sparse_grad"):
        A().embed_tokens(tok, table, differentiable=True, accumulate=True)
    rg = backward_rows(tok, table, torch.ones(3, 5, 8, device=dev))
    assert not torch.distributed.is_initialized()
    assert A().distributed.exchange_row_grad(table) is None and table.row_grad is rg and rg.pending


# ---------------------------------------------------------------- CPU
def rows_grad_torch(tok, dqf, V):
    """A RowSparseGrad from CPU tensors with plain torch: the rows added in position order, -1 tail, NaN rows above the count."""
    n, E = tok.numel(), dqf.shape[-1]
    flat, d = tok.reshape(-1), dqf.reshape(-1, E)
    union = torch.unique(flat[(flat >= 0) & (flat < V)])
    ids = torch.full((n,), -1, dtype=torch.int32)
    ids[:union.numel()] = union.to(torch.int32)
    rows = torch.full((n, E), float("nan"))
    for s, v in enumerate(union.tolist()):
        where = torch.nonzero(flat == v).reshape(-1).tolist()
        acc = d[where[0]].clone()
        for q in where[1:]:
            acc = acc + d[q]
        rows[s] = acc
    live = rows[:union.numel()].double()
    return A().RowSparseGrad(ids, rows, torch.tensor([union.numel()], dtype=torch.int32), (live * live).sum().reshape(1), (V, E))


GLOO_SHAPE = (3, 5, 11, 4)                                               # per-rank (B, Nq), V, E


def gloo_batch(step, rank):
    B, Nq, V, E = GLOO_SHAPE
    g = torch.Generator().manual_seed(1000 + 10 * step + rank)
    return torch.randint(-1, V + 1, (B, Nq), generator=g), draw_dqf((B, Nq), E, g)


def _worker(rank, world, port, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), WORLD_SIZE=str(world), RANK=str(rank), LOCAL_RANK=str(rank))
    torch.set_num_threads(2)
    V, E = GLOO_SHAPE[2:]
    D = A().distributed
    D.init(backend="gloo")
    init = torch.randn(V, E, generator=torch.Generator().manual_seed(3))
    table, alone = init.clone().requires_grad_(True), init.clone().requires_grad_(True)
    opt, ref = A().RowSparseAdamTorch(table, lr=1e-2), A().RowSparseAdamTorch(alone, lr=1e-2)
    same = True
    for step in range(3):
        table.row_grad = rows_grad_torch(*gloo_batch(step, rank), V)
        D.exchange_row_grad(table, merge=A().merge_row_grads_torch)
        assert table.row_grad.pending and table.row_grad.ids.shape[0] == world * GLOO_SHAPE[0] * GLOO_SHAPE[1]
        # one process alone: both shards merged in rank order with scale 0.5
        want = A().merge_row_grads_torch([rows_grad_torch(*gloo_batch(step, r), V) for r in range(world)], scale=0.5)
        got = table.row_grad
        c = int(want.count)
        same = same and torch.equal(got.ids, want.ids) and torch.equal(got.count, want.count) and \
            torch.equal(got.rows[:c].view(torch.int32), want.rows[:c].view(torch.int32))
        opt.step()
        ref.step(want)
        assert not table.row_grad.pending
    refused = False
    try:
        D.exchange_row_grad(table, merge=A().merge_row_grads_torch)     # consumed on both ranks: refused before any collective
    except RuntimeError as e:
        refused = "pending" in str(e)
    D.barrier()
    state = [table.detach(), opt.state[table]["exp_avg"], opt.state[table]["exp_avg_sq"], opt._state[:3]]
    alone_state = [alone.detach(), ref.state[alone]["exp_avg"], ref.state[alone]["exp_avg_sq"], ref._state[:3]]
    q.put((rank, same, refused, [x.clone().numpy() for x in state], [x.clone().numpy() for x in alone_state]))
    torch.distributed.destroy_process_group()


@pytest.mark.timeout(300)
def test_two_gloo_ranks_end_with_the_same_table():
    """Each of two ranks builds its shard's gradient with plain torch, calls exchange_row_grad(table, merge=merge_row_grads_torch) and steps
    RowSparseAdamTorch, three times: the gathered and merged list is the one a single process gets from both shards in rank order with
    scale 0.5, and table and moments are bitwise equal across the ranks and to that single process; without a pending gradient the
    call raises RuntimeError."""
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = free_port()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = sorted([q.get(timeout=240) for _ in procs], key=lambda x: x[0])
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    for rank, same, refused, state, alone in res:
        assert same and refused, (rank, same, refused)
        for x, y, z in zip(state, alone, res[0][3]):
            assert x.tobytes() == y.tobytes() == z.tobytes(), rank
    init = torch.randn(*GLOO_SHAPE[2:], generator=torch.Generator().manual_seed(3))
    assert not torch.equal(torch.from_numpy(res[0][3][0]), init) and res[0][3][3][0] == 3.0


def test_torch_restatement_against_fp64():
    """merge_row_grads_torch over random lists (R = 5, V = 23, E = 8) against the dense fp64 sum: the sorted union, the -1 tail, the count,
    and per element an error of at most k * 2**-24 * sum |addends| for an id held by k lists (the bound of
    test_shards_merge_to_the_full_batch; scaling by 0.25 is exact); the inputs keep their pending flag and their contents."""
    R, V, E, n = 5, 23, 8, 9
    g = torch.Generator().manual_seed(4)
    grads, exact, mags, held = [], torch.zeros(V, E, dtype=torch.float64), torch.zeros(V, E, dtype=torch.float64), torch.zeros(V)
    for r in range(R):
        c = int(torch.randint(0, n + 1, (1,), generator=g))
        ids = torch.full((n,), -1, dtype=torch.int32)
        ids[:c] = torch.sort(torch.randperm(V, generator=g)[:c]).values.to(torch.int32)
        rows = torch.full((n, E), float("nan"))
        rows[:c] = draw_dqf((c,), E, g)
        exact[ids[:c].long()] += rows[:c].double()
        mags[ids[:c].long()] += rows[:c].double().abs()
        held[ids[:c].long()] += 1
        grads.append(A().RowSparseGrad(ids, rows, torch.tensor([c], dtype=torch.int32), torch.zeros(1, dtype=torch.float64), (V, E)))
    kept = [(rg.ids.clone(), rg.rows.clone()) for rg in grads]
    for scale in (None, 0.25, torch.tensor([0.25], dtype=torch.float64)):
        m = A().merge_row_grads_torch(grads, scale=scale)
        union = torch.nonzero(held).reshape(-1)
        count = int(m.count)
        assert m.pending and m.shape == (V, E) and m.ids.shape == (R * n,) and m.rows.shape == (R * n, E)
        assert count == union.numel() and torch.equal(m.ids[:count].long(), union) and bool((m.ids[count:] == -1).all())
        f = 1.0 if scale is None else 0.25
        err = (m.to_dense().double() - exact * f).abs()
        assert bool((err <= held.double().unsqueeze(1) * 2.0 ** -24 * mags * f).all())
        sq = float((m.rows[:count].double() ** 2).sum())
        assert abs(float(m.sq_norm) - sq) <= 1e-12 * sq
    for rg, (i, r) in zip(grads, kept):
        assert rg.pending and torch.equal(rg.ids, i) and torch.equal(device_bits(rg.rows), device_bits(r))
    with pytest.raises(ValueError, match="16"):
        A().merge_row_grads_torch(grads * 4)


def test_c_abi_rejects_before_any_launch():
    """smin_row_lists_merge returns a nonzero status without launching anything (so it runs without a device, on addresses that are never
    dereferenced) for: R outside [1, 16], a negative n[r], N > 65536, bad E, a NULL pointer with N > 0, misaligned rows and a workspace
    that is too small; N = 0 without outputs is accepted and does nothing; smin_row_adam_step rejects more than 65536 slots."""
    import ctypes
    lib = A()._lib.load()
    fake = 0x10000                                                       # 16-byte aligned, never read

    def merge(R=2, n=(8, 8), E=4, V=11, ids=fake, rows=fake, count=fake, out=fake, ws=fake, ws_bytes=None, scale=None):
        ptrs = lambda a: (ctypes.c_void_p * 17)(*([a] * 17))
        N = sum(n[:max(min(R, len(n)), 0)])
        need = lib.smin_row_lists_merge_workspace_bytes(R, max(N, 0))
        return lib.smin_row_lists_merge(None, ptrs(ids), ptrs(rows), ptrs(count), (ctypes.c_int * len(n))(*n), R, V, E, scale, out, out, out,
                                        out, ws, need if ws_bytes is None else ws_bytes)

    assert lib.smin_row_lists_merge_workspace_bytes(2, 16) >= 16 * 16 + 4
    assert merge(R=0) != 0 and merge(R=17, n=(1,) * 17) != 0
    assert merge(n=(8, -1)) != 0
    assert merge(R=16, n=(4096,) * 15 + (4097,)) != 0
    assert merge(E=6) != 0 and merge(E=0) != 0
    for null in ("ids", "rows", "count", "out", "ws"):
        assert merge(**{null: None}) != 0, null
    assert merge(rows=fake + 4) != 0
    assert merge(scale=fake + 4) != 0
    assert merge(ws_bytes=lib.smin_row_lists_merge_workspace_bytes(2, 16) - 1) != 0
    assert merge(R=1, n=(0,), ids=None, rows=None, count=None, out=None, ws=None) == 0
    step = lambda n: lib.smin_row_adam_step(None, fake, fake, fake, fake, fake, fake, None, n, 11, 4, fake, None, 0.9, 0.999, 1e-8, 0)
    assert step(65537) != 0 and step(-1) != 0
