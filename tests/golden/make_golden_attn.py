"""Generate the word-attention map fixtures (tests/golden/ga_*.npz) from the REFERENCE implementation.

Run where a checkout of the reference exists (it is not needed anywhere else):
``python -B tests/golden/make_golden_attn.py <reference checkout> [fixture ...]``
(every fixture by default).

As make_golden.py: the reference's ``models.py`` is imported as-is on CPU and nothing of it is copied -- only inputs, weights
and the maps its own modules store after a forward:
  smis[k].content_unit.attn_layer.attn_weights    (B, L, L, C, Nq)   ContentAttention, models.py:207-226
  smis[k].boundary_unit.attn_layer.attn_weights   (B, L, Nq)         Attention,        models.py:137-154
Masked cells and rows are included as the reference computes them.  B >= 2 (the reference breaks at B = 1, models.py:50).

Fixtures (synthetic_batch: odd samples have a shorter video and query, so cells, rows and words are masked):
  ga_ragged   T 32, L 8, C 4 (r = 4 >= C), dl 16, Nq 7      the exact attention kernels, short queries
  ga_r2       T 16, L 8, C 4 (r = 2 <  C), dl 16, Nq 6      one-snippet moments hold fewer frames than clips
  ga_c3_q18   T 32, L 8, C 3, dl 16, Nq 18                   the general kernel form (C < 4) with more than 16 words
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.dont_write_bytecode = True
sys.path.insert(0, os.path.abspath(sys.argv[1]))

import models as ref_models          # noqa: E402  (the reference)
from oracle import smin_oracle as O  # noqa: E402

torch.set_num_threads(8)


def attn_case(name, T, L, C, D, dl, layers, Din, Nq, H, B, seed, boost):
    torch.manual_seed(seed)
    model = ref_models.SMIN(T, L, C, D, dl, layers, Din, Nq, H)
    with torch.no_grad():                 # push activations away from the untrained plateau (as make_golden.tiny_case)
        for n_, p in model.named_parameters():
            if "lstm" not in n_:
                p.mul_(boost)
    batch = O.synthetic_batch(B, T, L, Nq, Din, seed=seed + 100, with_labels=False)
    with torch.no_grad():
        pm, ps, pe, pa = model(batch["video_features"], batch["video_mask"], batch["query_features"], batch["query_mask"],
                               batch["length_mask"], batch["moment_mask"])
    blob = {"cfg": np.array([T, L, C, D, dl, layers, Din, Nq, H, B], dtype=np.int64)}
    blob.update({"sd/" + k: v.detach().numpy() for k, v in model.state_dict().items()})
    blob.update({"in/" + k: v.numpy() for k, v in batch.items()})
    blob.update({"out/pm": pm.numpy(), "out/ps": ps.numpy(), "out/pe": pe.numpy(), "out/pa": pa.numpy()})
    for k, smi in enumerate(model.smis):
        cw = smi.content_unit.attn_layer.attn_weights
        bw = smi.boundary_unit.attn_layer.attn_weights
        assert cw.shape == (B, L, L, C, Nq) and bw.shape == (B, L, Nq), (cw.shape, bw.shape)
        blob[f"attn/content{k}"] = cw.detach().numpy()
        blob[f"attn/boundary{k}"] = bw.detach().numpy()
    np.savez_compressed(os.path.join(HERE, name + ".npz"), **blob)
    print(name, "masked cells", int((~batch["moment_mask"]).sum()), "query lengths", batch["query_mask"].reshape(B, -1).sum(1).tolist())


if __name__ == "__main__":
    #                name                  T   L  C  D   dl lay Din Nq  H   B seed boost
    cases = {"ga_ragged": lambda: attn_case("ga_ragged", 32, 8, 4, 32, 16, 2, 24, 7, 16, 3, 21, 2.0),
             "ga_r2": lambda: attn_case("ga_r2", 16, 8, 4, 32, 16, 2, 24, 6, 16, 4, 22, 2.0),
             "ga_c3_q18": lambda: attn_case("ga_c3_q18", 32, 8, 3, 32, 16, 2, 24, 18, 16, 2, 23, 1.6)}
    for name in sys.argv[2:] or cases:
        cases[name]()
