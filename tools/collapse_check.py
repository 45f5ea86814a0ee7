#!/usr/bin/env python3
"""CPU check of the forward-only tail's formula: the last SMI layer's moment unit and the pm head collapsed to row dots
(functional.score_tail_torch on the oracle's seams), in fp32, against the golden pm, the as-written fp32 oracle and the fp64 oracle.
    python tools/collapse_check.py [charades anet_yml tacos_d500 ...]       (the tiny fixtures always; g5_<name> on request)"""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import smin_oracle as O          # noqa: E402
from tests import helpers as H               # noqa: E402
from tests.support.references import collapsed_pm  # noqa: E402


def run(name, cfg, sd, batch, pm_gold):
    with torch.no_grad():
        (pm32, *_), seams = O.smin_forward(sd, cfg, *H.model_inputs(batch), return_seams=True)
        pmc = collapsed_pm(sd, seams, batch, O.num_layers(sd))
        sd64 = {k: v.double() for k, v in sd.items()}
        b64 = {k: (v.double() if v.dtype == torch.float32 else v) for k, v in batch.items()}
        pm64 = O.smin_forward(sd64, cfg, *H.model_inputs(b64))[0]
    e = lambda x, y: (x.double() - y.double()).abs().max().item()
    print(f"{name:14s} as-written fp32 vs golden {e(pm32, pm_gold):.2e}  collapsed fp32 vs golden {e(pmc, pm_gold):.2e}  "
          f"as-written vs fp64 {e(pm32, pm64):.2e}  collapsed vs fp64 {e(pmc, pm64):.2e}  collapsed vs as-written {e(pmc, pm32):.2e}")


def main():
    for name in H.TINY:
        cfg, sd, batch, out, _, _ = H.split_tiny(H.load_npz(name))
        run(name, cfg, sd, batch, out["pm"])
    for name in sys.argv[1:]:
        z = H.load_npz("g5_" + name)
        T, L, C, D, dl, layers, Din, Nq, Hh = H.FULL[name]
        B, seed = int(z["cfg"][-2]), int(z["cfg"][-1])
        sd = O.formula_state_dict(H.smin_shapes(T, L, C, D, dl, layers, Din, Nq, Hh), gain=1.3)
        run(name, dict(T=T, L=L, C=C), sd, O.synthetic_batch(B, T, L, Nq, Din, seed=seed), torch.from_numpy(z["out/pm"]))


if __name__ == "__main__":
    main()
