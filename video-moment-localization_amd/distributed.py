"""Data-parallel plumbing for the train step: one process per GPU, batch sharded across ranks,
gradients all-reduced by torch DistributedDataParallel over RCCL (backend "nccl" on ROCm; "gloo" in CPU tests).
The hot path itself has no exchange step -- samples are independent -- so this is the only collective."""
import logging
import os

import torch
import torch.distributed as dist

log = logging.getLogger("vml_amd.distributed")


def env_world():
    return int(os.environ.get("WORLD_SIZE", "1")), int(os.environ.get("RANK", "0")), int(os.environ.get("LOCAL_RANK", "0"))


def init(backend=None, device=None):
    """Initialise the default process group from the torchrun environment (MASTER_ADDR should be 127.0.0.1)."""
    world, rank, _ = env_world()
    if (world == 1 and not os.environ.get("SMIN_FORCE_DDP")) or dist.is_initialized():
        return
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ.setdefault("MASTER_PORT", "29541")
    os.environ.setdefault("RANK", "0")
    os.environ.setdefault("WORLD_SIZE", "1")
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    if backend is None:
        backend = "nccl" if torch.cuda.is_available() else "gloo"
    kwargs = {"device_id": device} if (backend == "nccl" and device is not None) else {}
    dist.init_process_group(backend, **kwargs)


def shard_batch(batch, rank, world):
    """Contiguous equal split of every tensor's leading (sample) dimension; B must divide by world."""
    out = {}
    for k, v in batch.items():
        B = v.shape[0]
        if B % world:
            raise ValueError(f"batch of {B} does not split over {world} ranks")
        per = B // world
        out[k] = v[rank * per:(rank + 1) * per]
    return out


class InNodeDataParallel(torch.nn.Module):
    """Data-parallel wrapper of a SMIN whose step is one autograd node (the default).  torch DDP would see every gradient only when
    that node returns, so its all-reduce could not overlap the backward pass; here the node itself hands its gradient buffers to
    the process group as they become final (csrc/torch_binding.cpp GradSync: RCCL grouped all-reduces on the producing stream,
    joined before the node returns) and `.grad` holds the average over ranks when backward() returns.  Parameters are broadcast
    from rank 0 at construction, like DDP does; `.module` is the wrapped model."""

    def __init__(self, model):
        super().__init__()
        self.module = model
        for p in model.parameters():
            dist.broadcast(p.data, 0)
        from . import _lib
        _lib.load_torch().set_grad_sync(dist.group.WORLD.group_name, dist.get_world_size(), dist.get_backend() == "nccl")
        model.grad_sync = True

    def forward(self, *args, **kwargs):
        return self.module(*args, **kwargs)


def wrap(model, device=None, bucket_cap_mb=8):
    """Data parallel over the default process group (28-36 MB of fp32 gradients per step: SURVEY 5).  The one-node step
    exchanges its gradients itself, overlapped with its backward pass (InNodeDataParallel); the Python host (a node per module)
    goes through DistributedDataParallel with small buckets."""
    if not dist.is_initialized() or (dist.get_world_size() == 1 and not os.environ.get("SMIN_FORCE_DDP")):
        return model
    changed = {}
    gloo_on_gpu = dist.get_backend() == "gloo" and device is not None and device.type == "cuda"
    if gloo_on_gpu and getattr(model, "overlap_boundary", False):
        # gloo stages every bucket through the host and synchronises the streams a gradient touched: with the two-stream
        # step that serialises the whole backward pass (8x slower, measured); RCCL is unaffected
        model.overlap_boundary = changed["overlap_boundary"] = False
    from .modules import SMIN
    one_node = isinstance(model, SMIN) and model.fused_core
    if getattr(model, "overlap_prep", False) and (gloo_on_gpu or not one_node or os.environ.get("SMIN_DDP_NO_PREP_OVERLAP")):
        # a node per module (the Python host): DDP creates every parameter's gradient accumulator on the stream it is constructed on;
        # parameters that the step touches only on the second stream then make the main stream wait at each accumulation (measured +0.7 ms
        # over keeping that work on the main stream; the boundary unit's overlap still pays).  The one-node step hands every
        # gradient over on the main stream and keeps its second-stream tail under RCCL.
        model.overlap_prep = changed["overlap_prep"] = False
    model.ddp_overrides = changed                      # what wrap() switched off, for the caller to report
    if changed:
        log.warning("distributed.wrap (%s, world %d): set %s on the model", dist.get_backend(), dist.get_world_size(),
                    ", ".join(f"{k}={v}" for k, v in changed.items()))
    # The bf16-core contraction modes keep torch DDP (its all-reduce starts after the node has joined its streams): RCCL's
    # reduction kernels are not built under this library's no-packed-fp32 rule (csrc/Makefile) and have not been
    # checked beside the bf16 contraction kernels on a multi-GPU node, so they do not run beside them.
    in_node = one_node and model._param_prep_kernel() and SMIN._torch_beside_contractions() and not os.environ.get("SMIN_TORCH_DDP")
    model.grad_exchange = "in_node" if in_node else "torch_ddp"
    if in_node:
        return InNodeDataParallel(model)
    from torch.nn.parallel import DistributedDataParallel as DDP
    ids = [device.index] if (device is not None and device.type == "cuda") else None
    return DDP(model, device_ids=ids, bucket_cap_mb=bucket_cap_mb, gradient_as_bucket_view=True)


def exchange_row_grad(table, group=None, average=True, merge=None):
    """Give every data-parallel rank the same row-sparse gradient of ``table``: each rank's pending
    ``table.row_grad`` (``embed_tokens(..., sparse_grad=True)``) is gathered -- ``ids``, ``count`` and ``rows``, n * (E + 1) + 1 words a
    rank instead of the V * E of a dense all-reduce -- and ``table.row_grad`` is replaced by ``merge(lists in rank order, scale)``
    with ``scale = 1 / world size`` if ``average`` (what the model's gradients get) else ``None``.  ``merge`` defaults to
    ``sampling.merge_row_grads`` (HIP); ``sampling.merge_row_grads_torch`` is the restatement for CPU groups.  Every rank ends with the
    same list, bit for bit, so the ``RowSparseAdam`` steps that follow keep the replicas of the table identical.
    Without an initialised process group, or at world size 1, nothing is touched.  Otherwise every rank must call it: a table without
    a pending ``row_grad`` raises RuntimeError (a rank must not skip a collective silently), and ranks whose gradients differ in
    capacity n or in ``(V, E)`` raise ValueError on every rank (checked through one small gather read on the host)."""
    if not dist.is_initialized():
        return
    world = dist.get_world_size(group)
    if world == 1:
        return
    from .sampling import RowSparseGrad, merge_row_grads
    rg = getattr(table, "row_grad", None)
    if rg is None or not rg.pending:
        raise RuntimeError("exchange_row_grad: the table has no pending row_grad (every rank of the group takes part in the gather: run "
                           "the backward of embed_tokens(..., sparse_grad=True) on each before calling it)")
    (V, E), n, dev = rg.shape, int(rg.ids.shape[0]), rg.rows.device
    mine = torch.tensor([n, V, E], dtype=torch.int64, device=dev)
    dims = torch.empty((world, 3), dtype=torch.int64, device=dev)
    dist.all_gather([dims[r] for r in range(world)], mine, group=group)
    if not bool((dims == mine).all()):
        raise ValueError(f"exchange_row_grad: every rank's row_grad must have the same capacity and table shape (n, V, E); got {dims.tolist()}")
    if n == 0:
        return
    ids = torch.empty((world, n), dtype=torch.int32, device=dev)
    count = torch.empty((world, 1), dtype=torch.int32, device=dev)
    rows = torch.empty((world, n, E), dtype=torch.float32, device=dev)
    for buf, own in ((ids, rg.ids), (count, rg.count), (rows, rg.rows)):
        dist.all_gather([buf[r] for r in range(world)], own.reshape(buf.shape[1:]).contiguous(), group=group)
    # the merge recomputes the squared norm, so the lists' own are not gathered
    lists = [RowSparseGrad(ids[r], rows[r], count[r], None, (V, E)) for r in range(world)]
    table.row_grad = (merge or merge_row_grads)(lists, scale=1.0 / world if average else None)


def gather_search(result, num_videos, group=None, k=None, merge=None):
    """One global ranked list on every rank out of each rank's ``SMIN.search`` over its own shard of the videos (the same queries on
    every rank): the ranks gather ``video``, ``idx``, ``score`` and ``count`` -- Q * k_s * 4 + Q words a rank -- and
    their ``num_videos``, and each merges the lists in rank order with ``video_offset`` the exclusive prefix sum of ``num_videos``, so
    rank r's video v becomes global video ``sum(num_videos[:r]) + v``.  ``k``: entries per query of the merged list (default: the
    lists' own).  ``merge`` defaults to ``moments.merge_search`` (HIP); ``moments.merge_search_torch`` is the restatement for CPU
    groups.  More than 16 ranks are folded in groups of 16, which gives the same list.  Every rank returns the same dict, bit for bit
    (``video``, ``idx``, ``score``, ``count``; times follow from ``moments.search_times`` and the global durations).
    Without an initialised process group, or at world size 1, the rank's own list is merged alone.  Ranks whose lists differ in Q or
    in entries per query, or that pass different ``k``, raise ValueError on every rank (one small gather read on the host)."""
    from .moments import merge_search
    return _gather_lists("gather_search", result, {"idx": (torch.int64, (2,)), "score": (torch.float32, ())}, num_videos, group, k, merge or merge_search)


def gather_search_windows(result, num_videos, group=None, k=None, merge=None):
    """``gather_search`` for ``SMIN.search_windows`` lists: each rank searched the window bank of its own shard of
    whole videos with the same queries; the ranks gather ``video``, ``span``, ``score``, ``window``, ``cell`` and ``count`` and their
    ``num_videos`` by the same protocol -- the one small dims gather with its ValueError on every rank, rank order, offsets the
    exclusive prefix sum, more than 16 ranks folded -- and each merges them with ``moments.merge_search_windows`` (HIP; ``merge``:
    ``moments.merge_search_windows_torch`` is the restatement for CPU groups).  Every rank returns the same dict, bit for bit, without
    ``times``: they follow from ``moments.window_times`` and the global durations and row counts."""
    from .moments import merge_search_windows
    fields = {"span": (torch.float32, (2,)), "score": (torch.float32, ()), "window": (torch.int64, ()), "cell": (torch.int64, (2,))}
    return _gather_lists("gather_search_windows", result, fields, num_videos, group, k, merge or merge_search_windows)


def gather_search_weighted(result, num_videos=None, group=None, k=None, video_weight=0.0, max_videos=None, n_videos=None, gt_video=None, merge=None):
    """``gather_search`` for ``SMIN.search(..., carry=True)`` lists, merged under the corpus-wide video weights and ranks (INTEGRATION.md
    3u): ``gather_search``'s protocol with ``raw`` and the two ``(Q, V_r)`` matrices ``pair_score`` / ``pair_cells`` added -- their widths
    differ from rank to rank, so they travel padded to the widest, the widths taken from the one small dims gather -- and each rank
    merges the lists in rank order with ``moments.merge_search_weighted`` (HIP; ``merge``: ``moments.merge_search_weighted_torch`` is the
    restatement for CPU groups).  ``num_videos`` defaults to the width of ``pair_score``, which it must equal.  ``video_weight``,
    ``max_videos`` and ``n_videos`` must be the same on every rank, and are checked with the dims; ``gt_video``: the queries' global
    videos, the same on every rank.  Every rank returns the same dict, bit for bit.  A mismatch raises ValueError on every rank."""
    from .moments import merge_search_weighted
    fields = {"idx": (torch.int64, (2,)), "score": (torch.float32, ()), "raw": (torch.float32, ())}
    return _gather_weighted("gather_search_weighted", result, fields, num_videos, group, k, merge or merge_search_weighted, video_weight,
                            max_videos, n_videos, gt_video)


def gather_search_windows_weighted(result, num_videos=None, group=None, k=None, video_weight=0.0, max_videos=None, n_videos=None, gt_video=None,
                                   merge=None):
    """``gather_search_weighted`` for ``SMIN.search_windows(..., carry=True)`` lists of shards of whole videos, merged by
    ``moments.merge_search_windows_weighted`` (``merge``: its ``_torch`` restatement for CPU groups)."""
    from .moments import merge_search_windows_weighted
    fields = {"span": (torch.float32, (2,)), "score": (torch.float32, ()), "raw": (torch.float32, ()), "window": (torch.int64, ()),
              "cell": (torch.int64, (2,))}
    return _gather_weighted("gather_search_windows_weighted", result, fields, num_videos, group, k, merge or merge_search_windows_weighted,
                            video_weight, max_videos, n_videos, gt_video)


def _gather_weighted(what, result, fields, num_videos, group, k, merge, video_weight, max_videos, n_videos, gt_video):
    import struct
    for key in ("raw", "pair_score", "pair_cells"):
        if key not in result:
            raise ValueError(f"{what}: the list carries no {key} -- search the shard with carry=True")
    bound = lambda lists, offsets, k: merge(lists, offsets, k=k, video_weight=video_weight, max_videos=max_videos, n_videos=n_videos, gt_video=gt_video)
    width = int(result["pair_score"].shape[1])
    # the options every rank must share, as integers of the dims gather: the weight by its fp64 bits
    options = [struct.unpack("<q", struct.pack("<d", float(video_weight)))[0], -1 if max_videos is None else int(max_videos),
               -1 if n_videos is None else int(n_videos)]
    return _gather_lists(what, result, fields, width if num_videos is None else num_videos, group, k, bound, wide=("pair_score", "pair_cells"),
                         options=[width] + options)


def _gather_lists(what, result, fields, num_videos, group, k, merge, wide=(), options=()):
    """The protocol of the gathers of ranked lists: ``fields`` names a list's tensors beside ``video (Q, k_s)`` int64 and ``count (Q,)``
    int32 -- name -> (dtype, the shape behind (Q, k_s)).  ``wide``: the list's fp32 ``(Q, num_videos)`` matrices, gathered padded to the
    widest rank's; ``options``: further integers of the dims gather -- the first the matrices' width, which must be the rank's
    num_videos, the others values every rank must share."""
    from .moments import fold_search
    video = result["video"]
    Q, ks = video.shape
    k = ks if k is None else int(k)
    if not dist.is_initialized() or dist.get_world_size(group) == 1:
        if options and options[0] != int(num_videos):
            raise ValueError(f"{what}: num_videos = {int(num_videos)} must be the width of the list's (Q, V) matrices ({options[0]})")
        return merge([result], [0], k=k)
    world, dev = dist.get_world_size(group), video.device
    mine = torch.tensor([Q, ks, k, int(num_videos)] + list(options), dtype=torch.int64, device=dev)
    dims = torch.empty((world, mine.shape[0]), dtype=torch.int64, device=dev)
    dist.all_gather([dims[r] for r in range(world)], mine, group=group)
    dims = dims.tolist()
    if any(d[:3] != dims[0][:3] for d in dims) or min(d[3] for d in dims) < 0:
        raise ValueError(f"{what}: every rank's list must have the same queries, entries per query and k, and num_videos >= 0; got "
                         f"(Q, k_list, k, num_videos) = {[d[:4] for d in dims]}")
    if options and (any(d[4] != d[3] for d in dims) or any(d[5:] != dims[0][5:] for d in dims)):
        raise ValueError(f"{what}: every rank's num_videos must be the width of its (Q, V) matrices and the video-level options the same on "
                         f"every rank; got (num_videos, width, options...) = {[d[3:] for d in dims]}")
    bufs = {"video": torch.empty((world, Q, ks), dtype=torch.int64, device=dev)}
    bufs.update({key: torch.empty((world, Q, ks) + tail, dtype=dt, device=dev) for key, (dt, tail) in fields.items()})
    bufs["count"] = torch.empty((world, Q), dtype=torch.int32, device=dev)
    for key, buf in bufs.items():
        dist.all_gather([buf[r] for r in range(world)], result[key].detach().to(buf.dtype).contiguous(), group=group)
    lists = [{key: buf[r] for key, buf in bufs.items()} for r in range(world)]
    widest = max(d[3] for d in dims)
    for key in wide:
        buf = torch.empty((world, Q, widest), dtype=torch.float32, device=dev)
        own = torch.zeros((Q, widest), dtype=torch.float32, device=dev)
        own[:, :dims[dist.get_rank(group)][3]] = result[key].detach().float()
        dist.all_gather([buf[r] for r in range(world)], own, group=group)
        for r in range(world):
            lists[r][key] = buf[r, :, :dims[r][3]]
    offsets = [sum(d[3] for d in dims[:r]) for r in range(world)]
    return fold_search(lists, offsets, k, merge)


def describe():
    """(backend, world size) of the default process group as the collective library reports them -- what a benchmark
    line may claim about its gradient exchange."""
    if not dist.is_initialized():
        return None, 1
    return dist.get_backend(), dist.get_world_size()


def max_over_ranks(value, device):
    if not dist.is_initialized():
        return float(value)
    t = torch.tensor([float(value)], dtype=torch.float64, device=device)
    dist.all_reduce(t, op=dist.ReduceOp.MAX)
    return float(t.item())


def sum_over_ranks(value, device):
    if not dist.is_initialized():
        return float(value)
    t = torch.tensor([float(value)], dtype=torch.float64, device=device)
    dist.all_reduce(t)
    return float(t.item())


def barrier():
    if dist.is_initialized():
        dist.barrier()
