"""SHA-256 of everything the torch extension's host code computes, over the options and paths of csrc/torch_binding.cpp and the headers it
is made of (core_forward.h, core_backward.h, loss_nodes.h ...): the one-node core, scoring over fp32 and compact banks, the two
pair-plan losses and a weighted corpus search.  A change of those files that is meant to move no bit is checked by running this tool on
a build from before and a build from after and comparing the listings.

    python tools/core_digest.py [--root CHECKOUT] > listing.txt

Only public calls of the package are used (models.SMIN and its methods, vml_amd.loss_fn, vml_amd.set_gemm_mode), so the same file runs
against an older checkout: --root names the checkout whose build is loaded (default: the one this file lies in).  One line per tensor:
case, name, dtype, shape, digest.  Needs a HIP device."""
import argparse
import hashlib
import math
import os
import sys

import torch

# (T, L, C, D, dl, layers, Din, Nq, H, B)
SHAPES = {
    "prep_kernel": (64, 16, 4, 128, 32, 3, 40, 9, 64, 5),       # the parameter-product kernel is eligible
    "six_layers": (64, 16, 2, 128, 32, 6, 40, 9, 64, 3),        # layer 5: two weight-product parts; layers 0-1: the summed later-gradient path
    "torch_prep": (64, 16, 4, 64, 16, 2, 40, 9, 32, 5),         # dl = 16: the parameter products run as torch calls
}


def ragged_batch(B, T, L, Nq, Din, seed, dev):
    g = torch.Generator().manual_seed(seed)
    b = dict(video_features=torch.randn(B, T, Din, generator=g), query_features=torch.randn(B, Nq, 300, generator=g),
             video_mask=torch.zeros(B, T, 1, dtype=torch.uint8), query_mask=torch.zeros(B, Nq, 1, dtype=torch.uint8),
             length_mask=torch.zeros(B, L, dtype=torch.bool))
    for i in range(B):
        nf = T if i % 2 == 0 else int(torch.randint(T // 2, T, (1,), generator=g))
        nq = Nq - 2 if i == 0 else int(torch.randint(2, Nq - 1, (1,), generator=g))          # the longest query: Nq - 2 words
        b["video_features"][i, nf:] = 0
        b["query_features"][i, nq:] = 0
        b["video_mask"][i, :nf] = 1
        b["query_mask"][i, :nq] = 1
        b["length_mask"][i, :math.ceil(nf / (T / L))] = True
    b["moment_mask"] = torch.triu(b["length_mask"].unsqueeze(2) & b["length_mask"].unsqueeze(1))
    b["sm"] = torch.rand(B, L, L, generator=g) * b["moment_mask"]
    b["ss"], b["se"] = torch.rand(B, L, generator=g), torch.rand(B, L, generator=g)
    b.update(ym=b["sm"] > 0.5, ys=b["ss"] > 0.5, ye=b["se"] > 0.5, ya=torch.rand(B, L, generator=g) > 0.5)
    return {k: v.to(dev) for k, v in b.items()}


def inputs(b):
    return [b[k] for k in ("video_features", "video_mask", "query_features", "query_mask", "length_mask", "moment_mask")]


def emit(case, name, t):
    t = t.detach().cpu().contiguous()
    raw = t.reshape(-1).view(torch.uint8).numpy().tobytes() if t.numel() else b""
    print(f"{case:28s} {name:60s} {str(t.dtype):14s} {str(tuple(t.shape)):22s} {hashlib.sha256(raw).hexdigest()}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    root = os.path.abspath(ap.parse_args().root)
    sys.path.insert(0, root)
    import models
    vml = models.vml_amd
    dev = torch.device("cuda:0")

    def model(shape, **attrs):
        torch.manual_seed(43)
        m = models.SMIN(*shape[:9]).to(dev)
        for k, v in attrs.items():
            setattr(m, k, v)
        return m

    def loss_of(out, b, rows=None):
        t = {k: (b[k] if rows is None else b[k].index_select(0, rows)) for k in ("ym", "sm", "moment_mask", "ys", "ss", "ye", "se", "ya", "length_mask")}
        return vml.loss_fn(out[0], t["ym"], t["sm"], t["moment_mask"], out[1], t["ys"], t["ss"], out[2], t["ye"], t["se"], out[3], t["ya"], t["length_mask"])

    def step(case, m, b, inp=None, rows=None, run=None):
        """forward + loss + backward: the outputs, every parameter gradient, and the input gradients where they are formed"""
        inp = inputs(b) if inp is None else inp
        out = m(*inp) if run is None else run(m)
        loss_of(out, b, rows).backward()
        for name, o in zip(("pm", "ps", "pe", "pa"), out):
            emit(case, name, o)
        for name, p in m.named_parameters():
            emit(case, "grad " + name, p.grad)
        for name, t in (("grad video_features", inp[0]), ("grad query_features", inp[2])):
            if t.grad is not None:
                emit(case, name, t.grad)
        torch.cuda.synchronize()

    def cut(b, words):                                         # the batch cut to its longest query, below max_query_length
        inp = inputs(b)
        inp[2], inp[3] = inp[2][:, :words].contiguous(), inp[3][:, :words].contiguous()
        return inp

    for name, shape in SHAPES.items():
        T, L, C, D, dl, layers, Din, Nq, Hh, B = shape
        b = ragged_batch(B, T, L, Nq, Din, 7 + layers, dev)
        step(name, model(shape), b, cut(b, Nq - 2) if name == "six_layers" else None)

    shape = SHAPES["prep_kernel"]
    T, L, C, D, dl, layers, Din, Nq, Hh, B = shape
    b = ragged_batch(B, T, L, Nq, Din, 3, dev)
    for off in ("overlap_boundary", "overlap_prep", "async_weights", "tail_split"):
        step("no " + off, model(shape, **{off: False}), b)
    step("known_cell_count", model(shape, known_cell_count=int(b["moment_mask"].sum())), b)
    inp = inputs(b)
    inp[0], inp[2] = inp[0].clone().requires_grad_(True), inp[2].clone().requires_grad_(True)
    step("input_grads", model(shape, input_grads=True), b, inp)
    m = model(shape, keep_attention=True)
    step("keep_attention", m, b)
    for k, smi in enumerate(m.smis):
        emit("keep_attention", f"content map {k}", smi.content_unit.attn_layer.attn_weights)
        emit("keep_attention", f"boundary map {k}", smi.boundary_unit.attn_layer.attn_weights)
    for k, v in sorted(model(shape).localize(*inputs(b), k=3, attention=True).items()):
        if torch.is_tensor(v):
            emit("localize attention", k, v)
    for storage in (True, False):
        vml.set_gemm_mode("bf16")
        try:
            step(f"bf16 storage {storage}", model(shape, bf16_operand_storage=storage), b)
        finally:
            vml.set_gemm_mode("f32")
    step("float masks", model(shape), b, [t.float() if i in (1, 3, 4, 5) else t for i, t in enumerate(inputs(b))])
    m = model(shape)
    for name, o in zip(("pm", "ps", "pe", "pa"), m.score(*inputs(b))):
        emit("score", name, o)
    for name, o in zip(("pm", "ps", "pe", "pa"), m.score(*cut(b, Nq - 2))):
        emit("score cut", name, o)
    # pairs with repeats: 3 videos, 4 queries
    vi, qi = [0, 2, 1, 2, 0, 2, 1], [3, 0, 1, 1, 2, 3, 1]
    vrows = torch.tensor([0, 1, 2], device=dev)
    vb = {k: b[k].index_select(0, vrows) for k in ("video_features", "video_mask", "length_mask", "moment_mask")}
    qf, qm = b["query_features"][:4].contiguous(), b["query_mask"][:4].contiguous()
    videos, queries = m.encode_videos(vb["video_features"], vb["video_mask"], vb["length_mask"], vb["moment_mask"]), m.encode_queries(qf, qm)
    for name, o in zip(("pm", "ps", "pe", "pa"), m.score_pairs(videos, queries, vi, qi)):
        emit("score_pairs", name, o)
    for storage in ("bf16", "int8"):                            # the same pairs over a compact bank: codes, and for int8 the frames' scales
        for name, o in zip(("pm", "ps", "pe", "pa"), m.score_pairs(videos.compact(storage), queries, vi, qi)):
            emit("score_pairs " + storage, name, o)
    pair_rows = torch.tensor(vi, device=dev)                    # a pair's targets: its video's
    for counts in (None, videos.cell_counts):
        step("forward_pairs" + ("" if counts is None else " counts"), model(shape), b, rows=pair_rows,
             run=lambda mm: mm.forward_pairs(vb["video_features"], vb["video_mask"], qf, qm, vb["length_mask"], vb["moment_mask"], vi, qi, cell_counts=counts))
    # the two losses over the pair plan, forward and backward, on forward_pairs' outputs (leaves here: the gradients are the losses' own)
    plan = vml.PairPlan(vi, qi, 3, 4, dev, gt_video=[2, 1, 0, 0])
    pair_mask = vb["moment_mask"].index_select(0, pair_rows)
    with torch.no_grad():
        scores = m.forward_pairs(vb["video_features"], vb["video_mask"], qf, qm, vb["length_mask"], vb["moment_mask"], vi, qi)[:3]
    teacher = torch.linspace(-1.0, 1.0, len(vi), device=dev)
    for case, term in (("pair_rank_loss", lambda *s: vml.pair_rank_loss(*s, pair_mask, plan, return_stats=True)),
                       ("pair_distill_loss", lambda *s: vml.pair_distill_loss(*s, pair_mask, plan, teacher, gamma_teacher=0.2, return_stats=True))):
        leaves = [s.detach().clone().requires_grad_(True) for s in scores]
        out = term(*leaves)
        out[0].backward()
        for name, t in zip(("loss", "stats", "pair_score", "grad pm", "grad ps", "grad pe"), list(out) + [s.grad for s in leaves]):
            emit(case, name, t)
    # which video, and where: the video-level score folded into the ranking (rank_videos' pooled pair score)
    for k, v in sorted(m.search(videos, queries, k=4, video_weight=7.5, max_videos=2, max_batch=5).items()):     # 12 pairs in three chunks
        if torch.is_tensor(v):
            emit("search video_weight", k, v)
    torch.cuda.synchronize()


if __name__ == "__main__":
    main()
