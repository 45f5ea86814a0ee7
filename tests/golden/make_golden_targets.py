"""Generate tests/golden/gb_targets.npz and gc_feeder_batch.npz from the REFERENCE's own target construction.

Run where a checkout of the reference exists (it is not needed anywhere else):
``python -B tests/golden/make_golden_targets.py <reference checkout>``

``dataset.py`` cannot be imported offline (torchtext and h5py at module level, GloVe fetched at class-definition time), but the
methods of ``AbstractDataset`` that build a sample need only ``np``, ``torch`` and ``math``: as make_golden_sampling.py does, the
file is parsed with ``ast`` and the definitions of ``get_iou``, ``get_boundary_penalties``, ``get_snippet_label``,
``get_fixed_length_features``, ``__getitem__`` and ``collate_fn`` are executed with those three names in scope.  Only data is stored.

gb_targets.npz -- function level.  For every L in LS one group ``L<L>/``: ``ts``, ``te``, ``dur`` (float64, the annotation as the
reference receives it), ``fam`` (index into ``families``), and the reference's ``sm`` (n, L, L), ``ss``, ``se`` (n, L) float32 and
``ya`` (n, L) uint8.  ``ym``/``ys``/``ye`` are the stored scores ``> 0.5`` (dataset.py:152-156).  ``win/`` holds two window-form
samples (annotation in seconds, row count, window) whose ``sampling.window_annotations`` geometry ``win/case`` points to in
group ``L16/``.  The case families are asserted present and their counts printed.

gc_feeder_batch.npz -- sample level.  ``__getitem__`` and ``collate_fn`` run on a stub ``self`` (a SimpleNamespace with T, L,
split, ``vocab.stoi['<pad>']``, annotations, ``_load_video_features`` and the four helpers bound to it).  For (T, L) in SHAPES and
split in (val, train) one group ``T<T>L<L>_<split>/``: the raw inputs (``raw`` packed rows, ``n``, ``tokens``, ``times``,
``duration``, ``spos`` = the first picked row, as g8 records it) and ``out/<key>`` for the fifteen tensor items of the collated
batch; ``table`` is the word table (its last two rows zero, as the reference's vocab), ``pad`` its pad id.
"""
import ast
import functools
import math
import os
import sys
from types import SimpleNamespace

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
METHODS = ("get_iou", "get_boundary_penalties", "get_snippet_label", "get_fixed_length_features", "__getitem__", "collate_fn")
LS = (5, 16, 17, 32, 64)
FAMILIES = ("clipped", "boundary", "iou_half", "extreme", "subnormal", "durations", "double", "fp32", "window", "degenerate")
# (two-decimal doubles, fp32-representable) random cases per L; the 64s are few (an sm map is 16 KiB)
BLOCKS = {5: (16, 10), 16: (48, 32), 17: (16, 10), 32: (20, 12), 64: (3, 2)}
NAMED_DOUBLE = (631.06, 631.41, 673.65)         # a short moment late in a long video: the worst case of an fp32 denominator
SHAPES = ((64, 16), (128, 32))
DIN, NQ, VOCAB, EMB = 8, 6, 12, 8
ITEMS = ("video_features", "video_mask", "query_features", "query_mask", "length_mask", "moment_mask", "start_pos", "end_pos",
         "sm", "ym", "ss", "ys", "se", "ye", "ya")
# the two window-form samples: (ts, te, duration) in seconds, rows of the video, window start and length, at T = 64, L = 16
WIN_T, WIN_L = 64, 16
WINDOWS = dict(times=[[631.06, 631.41], [12.37, 95.03]], duration=[673.65, 141.77], n=[1501, 263], start=[1390, 40], len=[64, 41])

f32 = np.float32


def load_reference_methods(ref_dir):
    tree = ast.parse(open(os.path.join(ref_dir, "dataset.py")).read())
    cls = next(n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == "AbstractDataset")
    fns = [n for n in cls.body if isinstance(n, ast.FunctionDef) and n.name in METHODS]
    assert sorted(f.name for f in fns) == sorted(METHODS)
    scope = {"np": np, "torch": torch, "math": math}
    exec(compile(ast.Module(body=fns, type_ignores=[]), "dataset.py", "exec"), scope)
    return {k: scope[k] for k in METHODS}


def bound(i, dur, L):
    """Snippet boundary i as the reference's fp32 tensor expression forms it: float32(i) * float32(dur) / float32(L)."""
    return f32(i) * f32(dur) / f32(L)


def steps(x):
    """One fp32 step below x, x, one step above (as doubles)."""
    x = f32(x)
    return [float(np.nextafter(x, f32(-np.inf))), float(x), float(np.nextafter(x, f32(np.inf)))]


def representable(x):
    return float(f32(x)) == x


def window_geometry():
    """sampling.window_annotations' arithmetic (float64): the ground truth in rows minus the window start; duration max(len, T)."""
    t, d = np.asarray(WINDOWS["times"], np.float64), np.asarray(WINDOWS["duration"], np.float64)
    n, s, w = (np.asarray(WINDOWS[k]) for k in ("n", "start", "len"))
    g = t / d[:, None] * n.astype(np.float64)[:, None]
    return g - s.astype(np.float64)[:, None], np.maximum(w, WIN_T).astype(np.float64)


def random_annotation(rng):
    dur = round(float(rng.uniform(5, 760)), 2)
    ts = round(float(rng.uniform(0, dur * 0.95)), 2)
    length = float(rng.choice([rng.uniform(0.3, 3), rng.uniform(3, 60), rng.uniform(0.3, dur)]))
    return ts, round(min(dur, ts + length), 2), dur


def function_cases(L, R, rng):
    """[(family, ts, te, dur)] for one L.  R: the reference's methods, used to find moments whose Gaussians reach the subnormals."""
    few = L == 64
    fam = {k: i for i, k in enumerate(FAMILIES)}
    c = []
    # annotations the loaders clipped: ts = 0, te = duration, both (dataset.py:217-218)
    for dur in ((30.47,) if few else (2.0, 30.47, 100.0, 673.65, 760.0)):
        c += [(fam["clipped"], 0.0, round(0.37 * dur, 2), dur), (fam["clipped"], round(0.61 * dur, 2), dur, dur), (fam["clipped"], 0.0, dur, dur)]
    # times on a snippet boundary as the fp32 expression forms it, and one fp32 step either side: ya's two comparisons at equality
    for dur in ((673.65,) if few or L == 32 else (30.47, 673.65)):
        for i in ((L // 2,) if few else sorted({1, L // 2, L - 1})):
            c += [(fam["boundary"], t, dur, dur) for t in steps(bound(i, dur, L))]
            c += [(fam["boundary"], 0.13, t, dur) for t in steps(bound(i + 1, dur, L))]
    # IoU exactly one half (ts = 0, te = dur / 2 against the windows [0, dur] and, for 4 | L, [0, dur / 4]) and, with dur a power of
    # two, te one fp32 step off dur / 2: IoU one fp32 step above and below one half at cell (0, L - 1)
    for dur in ((64.0,) if few or L in (5, 17) else (2.0, 64.0, 128.0, 512.0)):
        c += [(fam["iou_half"], 0.0, t, dur) for t in steps(dur / 2)]
    # moments of 1 ms, of one snippet, of the whole video
    for x, dur in (((631.06, 673.65),) if few else ((12.5, 30.47), (631.06, 673.65), (0.0, 2.0))):
        c.append((fam["extreme"], x, x + 0.001, dur))
    for dur in ((30.47,) if few else (30.47, 100.0)):
        c += [(fam["extreme"], i * dur / L, (i + 1) * dur / L, dur) for i in ((L // 2,) if few else (0, L // 2, L - 1))]
    c += [(fam["extreme"], 0.0, dur, dur) for dur in ((760.0,) if few else (2.0, 760.0))]
    # short moments whose Gaussians pass through the subnormal range on their way to 0
    self = SimpleNamespace(L=L)
    tiny = float(np.finfo(np.float32).tiny)
    for dur in ((100.0,) if few else (32.0, 100.0, 673.65)):
        found = 0
        for m in np.arange(0.2, 4.0, 0.01):
            ts, te = 0.25 * dur, 0.25 * dur + float(m) * dur / L
            v = torch.cat(R["get_boundary_penalties"](self, ts, te, dur))
            if int(((v > 0) & (v < tiny)).sum()) and int((v == 0).sum()):
                c.append((fam["subnormal"], ts, te, dur))
                found += 1
                if found == (1 if few else 2):
                    break
        assert found, (L, dur)
    # durations from 2 s to 760 s
    for dur in ((2.0, 760.0) if few else (2.0, 5.5, 17.31, 61.7, 180.04, 333.33, 555.5, 760.0)):
        c.append((fam["durations"], round(0.21 * dur, 2), round(0.58 * dur, 2), dur))
    # dataset-like two-decimal doubles that are not fp32-representable, and a block whose times are
    c.append((fam["double"],) + NAMED_DOUBLE)
    n_double, n_single = BLOCKS[L]
    while n_double:
        ts, te, dur = random_annotation(rng)
        if ts < te and not representable(ts) and not representable(te):
            c.append((fam["double"], ts, te, dur))
            n_double -= 1
    while n_single:
        ts, te, dur = (float(f32(x)) for x in random_annotation(rng))
        if ts < te <= dur:
            c.append((fam["fp32"], ts, te, dur))
            n_single -= 1
    # window-form geometry: the moment starts before the window, ends after it, covers it, lies outside it on either side
    for ts, te in ((-3.25, 7.5), (20.1, 41.9), (-5.0, 40.0), (-9.0, -1.0), (35.0, 42.0)) if not few else ((-3.25, 41.9), (-9.0, -1.0)):
        c.append((fam["window"], ts, te, 30.47))
    if L == WIN_L:
        tw, dw = window_geometry()
        c += [(fam["window"], float(tw[b, 0]), float(tw[b, 1]), float(dw[b])) for b in range(tw.shape[0])]
    # ts == te: on a boundary (0 / 0 in sm, ss and se) and off it
    if not few:
        c += [(fam["degenerate"], float(bound(L // 2, 100.0, L)), float(bound(L // 2, 100.0, L)), 100.0), (fam["degenerate"], 12.34, 12.34, 100.0)]
    return c


def function_fixture(R, path):
    rng = np.random.default_rng(11)
    arrays, counts = dict(families=np.asarray(FAMILIES)), np.zeros(len(FAMILIES), np.int64)
    stats = dict(half=0, above=0, below=0, subnormal=0, zero=0, nan=0, ya_eq_s=0, ya_eq_e=0, worst_half=np.inf)
    half = f32(0.5)
    for L in LS:
        cases = function_cases(L, R, rng)
        self = SimpleNamespace(L=L)
        sm, ss, se, ya = [], [], [], []
        for _, ts, te, dur in cases:
            sm.append(R["get_iou"](self, ts, te, dur).numpy())
            s, e = R["get_boundary_penalties"](self, ts, te, dur)
            ss.append(s.numpy()); se.append(e.numpy())
            ya.append(R["get_snippet_label"](self, ts, te, dur).numpy().astype(np.uint8))
            b = np.array([bound(i, dur, L) for i in range(L + 1)])
            stats["ya_eq_s"] += int((b[:L] == f32(ts)).sum()); stats["ya_eq_e"] += int((b[1:] == f32(te)).sum())
        g = dict(ts=np.array([x[1] for x in cases]), te=np.array([x[2] for x in cases]), dur=np.array([x[3] for x in cases]),
                 fam=np.array([x[0] for x in cases], np.int8), sm=np.stack(sm), ss=np.stack(ss), se=np.stack(se), ya=np.stack(ya))
        assert g["ts"].dtype == np.float64 and g["sm"].dtype == np.float32 and g["ss"].dtype == np.float32
        arrays.update({f"L{L}/{k}": v for k, v in g.items()})
        counts += np.bincount(g["fam"], minlength=len(FAMILIES))
        pen = np.concatenate([g["ss"].ravel(), g["se"].ravel()])
        stats["half"] += int((g["sm"] == half).sum())
        stats["above"] += int((g["sm"] == np.nextafter(half, f32(1))).sum()); stats["below"] += int((g["sm"] == np.nextafter(half, f32(0))).sum())
        stats["subnormal"] += int(((pen > 0) & (pen < np.finfo(np.float32).tiny)).sum()); stats["zero"] += int((pen == 0).sum())
        stats["nan"] += int(np.isnan(g["sm"]).sum() + np.isnan(pen).sum())
        stats["worst_half"] = min(stats["worst_half"], float(np.nanmin(np.abs(pen.astype(np.float64) - 0.5))))
        print(f"L = {L}: {len(cases)} cases, durations {g['dur'].min()} .. {g['dur'].max()}")
    tw, dw = window_geometry()
    g16 = {k: arrays[f"L{WIN_L}/{k}"] for k in ("ts", "te", "dur")}
    case = [int(np.nonzero((g16["ts"] == tw[b, 0]) & (g16["te"] == tw[b, 1]) & (g16["dur"] == dw[b]))[0][0]) for b in range(tw.shape[0])]
    arrays.update({"win/times": np.asarray(WINDOWS["times"], np.float64), "win/duration": np.asarray(WINDOWS["duration"], np.float64),
                   "win/n": np.asarray(WINDOWS["n"], np.int64), "win/start": np.asarray(WINDOWS["start"], np.int64),
                   "win/len": np.asarray(WINDOWS["len"], np.int64), "win/TL": np.asarray([WIN_T, WIN_L], np.int64), "win/case": np.asarray(case, np.int64)})
    print("families:", dict(zip(FAMILIES, counts.tolist())))
    print("cells:", stats)
    assert (counts > 0).all() and counts[FAMILIES.index("degenerate")] == 2 * (len(LS) - 1)
    assert stats["half"] >= 8 and stats["above"] >= 1 and stats["below"] >= 1, "IoU at one half and one fp32 step either side"
    assert stats["subnormal"] >= 4 and stats["zero"] >= 4 and stats["nan"] >= 3
    assert stats["ya_eq_s"] >= 4 and stats["ya_eq_e"] >= 4, "times that equal a boundary of the fp32 expression"
    assert stats["worst_half"] > 1e-6, "a stored ss / se value within 1e-6 of the 0.5 threshold"
    all_ts, all_te, all_dur = (np.concatenate([arrays[f"L{L}/{k}"] for L in LS]) for k in ("ts", "te", "dur"))
    assert all_dur.min() == 2.0 and all_dur.max() == 760.0
    assert (all_ts < 0).any() and (all_te > all_dur).any() and (all_te < 0).any() and (all_ts > all_dur).any()
    assert any((arrays[f"L{L}/ts"] == NAMED_DOUBLE[0]).any() for L in LS)
    np.savez_compressed(path, **arrays)
    return os.path.getsize(path)


def sample_fixture(R, path):
    rng = np.random.default_rng(12)
    table = np.concatenate([rng.integers(-64, 65, (VOCAB - 2, EMB)) / 32.0, np.zeros((2, EMB))]).astype(np.float32)
    pad = VOCAB - 1
    arrays = dict(table=table, pad=np.asarray(pad, np.int64))
    # two-decimal annotations (not fp32-representable where the decimals are not), clipped ones among them
    annotations = [(631.06, 631.41, 673.65), (0.0, 7.83, 30.47), (21.37, 30.47, 30.47), (0.0, 141.77, 141.77), (3.3, 11.9, 17.31),
                   (402.17, 455.09, 760.0), (0.61, 1.27, 2.0), (88.88, 91.13, 180.04)]
    for T, L in SHAPES:
        ns = [1, T // L - 1, T // L, T // L + 1, T - 1, T, T + 1, 3 * T + 1]
        for split in ("val", "train"):
            order = rng.permutation(len(annotations))
            raws, anns = [], []
            for k, n in enumerate(ns):
                feat = (rng.integers(-512, 513, (n, DIN)) / 64.0).astype(np.float32)
                feat[:, 0] = np.arange(n)                                    # column 0 is the row number: the picked rows can be read back
                raws.append(feat)
                tok = rng.integers(0, VOCAB - 1, NQ)                        # <unk> (VOCAB - 2) among the ids: a word, not padding
                tok[NQ - k % (NQ + 1):] = pad                               # 0 .. Nq pad ids
                tok = torch.from_numpy(tok)
                ts, te, dur = annotations[order[k]]
                anns.append(dict(video_id=k, times=[ts, te], duration=dur, token_idx=tok, query_features=torch.from_numpy(table)[tok]))
            self = SimpleNamespace(T=T, L=L, split=split, vocab=SimpleNamespace(stoi={"<pad>": pad}), annotations=anns,
                                   _load_video_features=lambda vid: raws[vid].astype(np.float64))
            for m in METHODS[:4]:
                setattr(self, m, functools.partial(R[m], self))
            np.random.seed(100 * T + (split == "train"))
            batch = R["collate_fn"](self, [R["__getitem__"](self, k) for k in range(len(ns))])
            vf = batch["video_features"].numpy()
            assert vf.dtype == np.float32 and vf.shape == (len(ns), T, DIN)
            spos = vf[:, 0, 0].astype(np.int64)
            assert (spos == 0).all() if split == "val" else (spos > 0).any()
            pre = f"T{T}L{L}_{split}/"
            arrays.update({pre + "raw": np.concatenate(raws), pre + "n": np.asarray(ns, np.int64), pre + "spos": spos,
                           pre + "tokens": torch.stack([a["token_idx"] for a in anns]).numpy(),
                           pre + "times": np.asarray([a["times"] for a in anns], np.float64),
                           pre + "duration": np.asarray([a["duration"] for a in anns], np.float64)})
            for k in ITEMS:
                v = batch[k].numpy()
                arrays[pre + "out/" + k] = v.astype(np.uint8) if v.dtype == np.bool_ else v
            assert arrays[pre + "tokens"].dtype == np.int64 and sorted(set((arrays[pre + "tokens"] == pad).sum(1).tolist())) == list(range(NQ + 1))
    np.savez_compressed(path, **arrays)
    return os.path.getsize(path)


def main(ref_dir, out_dir=HERE):
    R = load_reference_methods(ref_dir)
    paths = [os.path.join(out_dir, "gb_targets.npz"), os.path.join(out_dir, "gc_feeder_batch.npz")]
    sizes = [function_fixture(R, paths[0]), sample_fixture(R, paths[1])]
    for p, s in zip(paths, sizes):
        print(f"{p}: {s} bytes")
    limit = os.path.getsize(os.path.join(HERE, "g3_c3.npz"))
    assert sum(sizes) <= limit, f"the two fixtures hold {sum(sizes)} bytes; the largest committed fixture holds {limit}"
    return paths


if __name__ == "__main__":
    main(os.path.abspath(sys.argv[1]))
