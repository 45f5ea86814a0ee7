"""Generate tests/golden/g8_clip_sampling.npz from the REFERENCE's own clip resampling.

Run where a checkout of the reference exists (it is not needed anywhere else):
``python -B tests/golden/make_golden_sampling.py <reference checkout>``

``dataset.py`` cannot be imported offline (torchtext and h5py at module level), but
``AbstractDataset.get_fixed_length_features`` (dataset.py:40-74) needs only numpy: the file is parsed with ``ast`` and that
one function definition is executed with ``np`` in scope.  It is called with ``self = SimpleNamespace(T, split)`` and features
whose column 0 is the row number, so the picked rows -- and, in the train split, the drawn start offset (the first picked row)
-- are read back from its output.  ``np.random`` is seeded for the train split.  Only data is stored: for every case
(n, T, split) the picked row indices and ``nfeats``.

Arrays: ``n``, ``T``, ``train`` (0/1), ``spos``, ``nfeats`` (one entry per case), ``ptr`` (cases + 1: case c's indices are
``idx[ptr[c]:ptr[c+1]]``), ``idx`` (int32).
"""
import ast
import os
import sys
from types import SimpleNamespace

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
TS = (16, 64, 128, 256, 1024)
TRAIN_DRAWS = 3


def load_reference_function(ref_dir):
    tree = ast.parse(open(os.path.join(ref_dir, "dataset.py")).read())
    cls = next(n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == "AbstractDataset")
    fn = next(n for n in cls.body if isinstance(n, ast.FunctionDef) and n.name == "get_fixed_length_features")
    scope = {"np": np}
    exec(compile(ast.Module(body=[fn], type_ignores=[]), "dataset.py", "exec"), scope)
    return scope["get_fixed_length_features"]


def lengths(T, rng):
    """n < T, n = T, n = T + 1; integral strides 2 and 3 and strides just above them; strides k + 0.5 (r integral); random
    non-integral strides up to ~20 T."""
    ns = {1, 2, T // 2, T - 1, T, T + 1, T + 2, 2 * T - 1, 2 * T, 2 * T + 1, 3 * T, 3 * T + 1, (3 * T) // 2, (5 * T) // 2,
          (7 * T) // 2 + 1, 20 * T, 20 * T + 3, 0}
    ns.update(int(x) for x in rng.integers(T + 1, 20 * T, 8))
    return sorted(x for x in ns if x >= 0)


def main(ref_dir):
    f = load_reference_function(ref_dir)
    rng = np.random.default_rng(8)
    np.random.seed(8)
    rows = dict(n=[], T=[], train=[], spos=[], nfeats=[])
    idx, ptr = [], [0]
    for T in TS:
        for n in lengths(T, rng):
            feat = np.stack([np.arange(n, dtype=np.float64), np.ones(n)], 1) if n else np.zeros((0, 2))
            for train in [0] + [1] * TRAIN_DRAWS:
                out, nf, _, _ = f(SimpleNamespace(T=T, split="train" if train else "val"), feat, 0.25, 0.75)
                assert out.shape == (T, 2) and (out[nf:] == 0).all()
                picked = out[:nf, 0].astype(np.int64)
                assert (out[:nf, 0] == picked).all()
                rows["n"].append(n); rows["T"].append(T); rows["train"].append(train); rows["nfeats"].append(nf)
                rows["spos"].append(int(picked[0]) if nf else 0)
                idx.append(picked.astype(np.int32))
                ptr.append(ptr[-1] + nf)
    arrays = {k: np.asarray(v, dtype=np.int32 if k != "n" else np.int64) for k, v in rows.items()}
    path = os.path.join(HERE, "g8_clip_sampling.npz")
    np.savez_compressed(path, idx=np.concatenate(idx), ptr=np.asarray(ptr, np.int64), **arrays)
    print(f"{path}: {len(ptr) - 1} cases, {ptr[-1]} indices, {os.path.getsize(path)} bytes, "
          f"{sum(1 for s in rows['spos'] if s)} train draws with spos > 0")


if __name__ == "__main__":
    main(os.path.abspath(sys.argv[1]))
