"""Costs of feeding raw per-video features and token ids (BatchFeeder's raw batch form, sampling.py) against host-side preparation.

1. host CPU time per batch, split by part: a per-sample numpy restatement of the reference's clip resampling into a float64 (T, Din)
   array with its start / end index search, the conversion of that array to an fp32 tensor (torch.FloatTensor, as the reference's
   loader does), and the per-query word-vector lookup; against the raw path's host work (one memcpy per video into a pinned buffer,
   nothing for rows a loader hands over pinned and packed);
2. device time of smin_sample_clips (pick, mean) and smin_embed_tokens: 20 calls captured in one graph and replayed, timed by device
   events (no Python in the timed window), with effective GB/s (bytes read + written) next to a torch device-to-device copy of the
   same output bytes timed the same way.  The "large" shape's working set exceeds the 256 MB Infinity Cache;
3. the headline train step (activitynet_t256) fed three ways, in rotating blocks of steps in one process: host-prepared pinned
   batches of the same samples (bench.py --feed host's form), raw rows handed over pinned and packed, raw rows as a list of numpy
   arrays.  For each
   the step time, the time the step thread waits for the next batch and the feeder worker's time per batch.

    python tools/raw_feed_bench.py [--steps 30] [--rounds 2] [--skip-step] [--kernels-only] [--out path.json]
Prints one JSON line per measurement.
"""
import argparse
import itertools
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import models  # noqa: E402

api = models.vml_amd
SHAPES = {"headline": dict(B=64, T=256, Din=500, Nq=20), "tacos": dict(B=2, T=128, Din=4096, Nq=14),
          "large": dict(B=64, T=1024, Din=1024, Nq=20)}
VOCAB = 400002                                          # glove.6B.300d + <unk> + <pad>


def raw_batch(B, T, Din, Nq, rng, g):
    n = rng.integers(T // 2, 4 * T + 1, B)
    ql = rng.integers(3, Nq + 1, B)
    tok = rng.integers(0, VOCAB - 1, (B, Nq))
    tok[np.arange(Nq)[None, :] >= ql[:, None]] = VOCAB - 1
    dur = rng.uniform(20, 120, B).astype(np.float32)
    ts = (rng.uniform(0, 0.5, B) * dur).astype(np.float32)
    te = (ts + 1.0 + rng.uniform(0, 1, B) * (dur - ts - 1.0)).astype(np.float32)
    return dict(raw_features=[torch.randn(int(k), Din, generator=g).numpy() for k in n], tokens=tok, times=np.stack([ts, te], 1),
                duration=dur, spos=api.draw_offsets(n, T, rng)), n


def host_resample(rb, T):
    """Per sample, the reference's resampling in numpy: float64 output, start / end search over the picked frames."""
    outs = []
    for b, feat in enumerate(rb["raw_features"]):
        n = feat.shape[0]
        stride = 1.0 if n <= T else n / T
        idx = np.round(np.arange(int(rb["spos"][b]), n - 0.5, stride)).astype(int)[:T]
        sp, ep = 0.25 * (n - 1.0), 0.75 * (n - 1.0)
        si, ei = 0, T - 1
        for i in range(len(idx) - 1):
            if idx[i] <= ep < idx[i + 1]:
                ei = i
            if idx[i] <= sp < idx[i + 1]:
                si = i
        out = np.zeros((T, feat.shape[1]))
        out[:len(idx)] = feat[idx, :]
        outs.append(out)
    return outs


def host_to_tensor(outs):
    return [torch.FloatTensor(o) for o in outs]


def host_lookup(rb, table):
    return [torch.nn.functional.embedding(torch.as_tensor(t, dtype=torch.long), table) for t in rb["tokens"]]


def raw_pack(rb, buf):
    """The raw path's host work for a list of arrays (BatchFeeder._stage_raw): one memcpy per video into a pinned buffer, the id check."""
    Din = rb["raw_features"][0].shape[1]
    dst = buf.numpy()
    o = 0
    for p in rb["raw_features"]:
        np.copyto(dst[o * Din:(o + p.shape[0]) * Din].reshape(-1, Din), p, casting="same_kind")
        o += p.shape[0]
    assert int(rb["tokens"].min()) >= 0 and int(rb["tokens"].max()) < VOCAB


def cpu_ms(fn, iters):
    fn()
    t0 = time.process_time()
    w0 = time.perf_counter()
    for _ in range(iters):
        fn()
    return 1e3 * (time.process_time() - t0) / iters, 1e3 * (time.perf_counter() - w0) / iters


def graph_ms(fn, calls=20, replays=10):
    """Device time per call: ``calls`` calls captured in one graph, replayed, timed by events around the replays."""
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            fn()
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(calls):
            fn()
    g.replay()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(replays):
        g.replay()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / (calls * replays)


def emit(rec, out):
    print(json.dumps(rec), flush=True)
    out.append(rec)


def host_cpu(out):
    table_cpu = torch.randn(VOCAB, 300)
    for name in ("headline", "tacos"):
        s = SHAPES[name]
        B, T, Din, Nq = s["B"], s["T"], s["Din"], s["Nq"]
        rng, g = np.random.default_rng(1), torch.Generator().manual_seed(1)
        rb, n = raw_batch(B, T, Din, Nq, rng, g)
        buf = torch.empty(int(n.sum()) * Din, dtype=torch.float32, pin_memory=True)
        iters = 10 if B > 8 else 100
        outs = host_resample(rb, T)
        rec = dict(kind="host_ms_per_batch", shape=name, **s, raw_rows=int(n.sum()))
        for part, fn in (("reference_resample", lambda: host_resample(rb, T)), ("reference_to_fp32_tensor", lambda: host_to_tensor(outs)),
                         ("reference_word_lookup", lambda: host_lookup(rb, table_cpu)), ("raw_pack_list", lambda: raw_pack(rb, buf))):
            c, w = cpu_ms(fn, iters)
            rec[part + "_wall"], rec[part + "_cpu"] = round(w, 3), round(c, 3)
        rec["raw_pack_pinned_packed_wall"] = 0.0
        rec["note"] = "_cpu = process CPU time over all threads; the reference's per-sample total is the sum of its three parts"
        emit(rec, out)


def device(dev, out):
    table = torch.randn(VOCAB, 300, device=dev)
    for name, s in SHAPES.items():
        B, T, Din, Nq = s["B"], s["T"], s["Din"], s["Nq"]
        rng, g = np.random.default_rng(1), torch.Generator().manual_seed(1)
        rb, n = raw_batch(B, T, Din, Nq, rng, g)
        raw = torch.from_numpy(np.concatenate(rb["raw_features"])).to(dev)
        del rb["raw_features"]
        offs = torch.from_numpy(np.concatenate([[0], np.cumsum(n)])).to(dev)
        spos = torch.from_numpy(rb["spos"]).to(dev)
        tok = torch.from_numpy(rb["tokens"]).to(torch.int32).to(dev)
        nf = np.minimum(n, T)
        out_bytes = B * T * Din * 4
        pick_bytes = out_bytes + int(nf.sum()) * Din * 4                    # write every output row, read the picked ones
        mean_bytes = out_bytes + int(n.sum()) * Din * 4                      # ... read every raw row
        src = torch.randn(B, T, Din, device=dev)
        dst = torch.empty_like(src)
        t_copy = graph_ms(lambda: dst.copy_(src))
        t_pick = graph_ms(lambda: api.sample_clips(raw, offs, T, spos=spos))
        t_mean = graph_ms(lambda: api.sample_clips(raw, offs, T, mode="mean"))
        t_emb = graph_ms(lambda: api.embed_tokens(tok, table))
        emb_bytes = 2 * B * Nq * 300 * 4
        gbs = lambda b, t: round(b / t / 1e6, 1)
        emit(dict(kind="device_ms", shape=name, **s, raw_mb=round(raw.numel() * 4 / 1e6, 1), out_mb=round(out_bytes / 1e6, 1),
                  torch_copy_ms=round(t_copy, 4), torch_copy_gbs=gbs(2 * out_bytes, t_copy), pick_ms=round(t_pick, 4),
                  pick_gbs=gbs(pick_bytes, t_pick), pick_over_copy=round(t_pick / t_copy, 2), mean_ms=round(t_mean, 4),
                  mean_gbs=gbs(mean_bytes, t_mean), embed_ms=round(t_emb, 4), embed_gbs=gbs(emb_bytes, t_emb),
                  note="graph replay, device events; GB/s = bytes read + written"), out)
        del raw, src, dst
        torch.cuda.empty_cache()


def step_compare(dev, steps, rounds, out):
    import bench
    T, L, C, D, dl, layers, Din, Nq, Hh, B = bench.WORKLOADS["activitynet_t256"]
    torch.manual_seed(43)
    model = models.SMIN(T, L, C, D, dl, layers, Din, Nq, Hh, dev).to(dev)
    opt = torch.optim.Adam(model.parameters(), lr=5e-4, fused=True)
    table = torch.randn(VOCAB, 300, device=dev)
    rng, g = np.random.default_rng(3), torch.Generator().manual_seed(3)
    raws = [raw_batch(B, T, Din, Nq, rng, g) for _ in range(2)]
    pinned = [dict(rb, raw_features=torch.from_numpy(np.concatenate(rb["raw_features"])).pin_memory(), raw_lengths=n) for rb, n in raws]
    raws = [rb for rb, _ in raws]
    # the host-fed form carries the same samples, prepared on the host (resampled by the restatement, words looked up), so all three
    # feeds hand the step bit-identical batches and only the feeding differs
    table_cpu = table.cpu()
    hosts = []
    for rb in raws:
        vf, nf = api.sample_clips_torch(rb["raw_features"], None, T, spos=rb["spos"])
        tok = torch.from_numpy(rb["tokens"])
        hosts.append(dict(video_features=vf.pin_memory(), query_features=table_cpu[tok].pin_memory(), nfeats=nf,
                          qlen=(tok < VOCAB - 1).sum(1), times=torch.from_numpy(rb["times"]), duration=torch.from_numpy(rb["duration"])))
    stage_ms = {"host": [], "raw_pinned": [], "raw_list": []}

    def timed(feeder, name):
        inner = feeder._stage

        def stage(slot, hb):
            t0 = time.perf_counter()
            r = inner(slot, hb)
            stage_ms[name].append(1e3 * (time.perf_counter() - t0))
            return r
        feeder._stage = stage
        return feeder

    feeds = {"host": timed(api.BatchFeeder(T, L, Nq, dev), "host").feed(itertools.cycle(hosts)),
             "raw_pinned": timed(api.BatchFeeder(T, L, Nq, dev, embedding=table), "raw_pinned").feed(itertools.cycle(pinned)),
             "raw_list": timed(api.BatchFeeder(T, L, Nq, dev, embedding=table), "raw_list").feed(itertools.cycle(raws))}
    wait_ms = {k: [] for k in feeds}

    def step(name):
        t0 = time.perf_counter()
        batch = next(feeds[name])
        wait_ms[name].append(1e3 * (time.perf_counter() - t0))
        batch["sm"] = torch.nan_to_num(batch["sm"])
        opt.zero_grad(set_to_none=True)
        pm, ps, pe, pa = model(batch["video_features"], batch["video_mask"], batch["query_features"], batch["query_mask"],
                               batch["length_mask"], batch["moment_mask"])
        loss = api.loss_fn(pm, batch["ym"], batch["sm"], batch["moment_mask"], ps, batch["ys"], batch["ss"], pe, batch["ye"], batch["se"],
                           pa, batch["ya"], batch["length_mask"])
        loss.backward()
        opt.step()

    times = {k: [] for k in feeds}
    for name in feeds:
        for _ in range(5):
            step(name)
    for k in feeds:
        stage_ms[k].clear()
        wait_ms[k].clear()
    order = list(feeds)
    for _ in range(rounds):
        for name in order + order[::-1]:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                step(name)
            torch.cuda.synchronize()
            times[name].append(1e3 * (time.perf_counter() - t0) / steps)
    med = lambda v: round(float(np.median(v)), 3)
    emit(dict(kind="step_ms", workload="activitynet_t256", B=B, steps_per_block=steps, **{k + "_ms": [round(x, 3) for x in v] for k, v in times.items()},
              **{k + "_median": med(v) for k, v in times.items()}, **{k + "_wait_median": med(v) for k, v in wait_ms.items()},
              **{k + "_worker_median": med(v) for k, v in stage_ms.items()},
              note="wait = step thread blocked on the next batch; worker = feeder worker's host time per batch"), out)
    for f in feeds.values():
        f.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--skip-step", action="store_true")
    ap.add_argument("--kernels-only", action="store_true", help="only the device timings (for a kernel-trace run)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "raw_feed_bench.py needs a HIP device"
    dev = torch.device("cuda:0")
    api._lib.load()
    out = []
    device(dev, out)
    if args.kernels_only:
        return
    host_cpu(out)
    if not args.skip_step:
        step_compare(dev, args.steps, args.rounds, out)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
