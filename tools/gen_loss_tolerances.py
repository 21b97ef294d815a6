#!/usr/bin/env python3
"""Writes tests/golden/loss_tolerances.json: per case of tests/loss_cases.py the tolerances the GPU tests of the loss kernels
(tests/test_gpu_loss_kernels.py) assert, and the measured distances they come from.  CPU only.

Per contrastive case two distances from the fp64 reference (tests/loss_cases.py: contrastive_ref) are measured:
  (a) a float32 mirror of the same computation, every sum in float32 and in descending order;
  (b) the reference with every inverse norm moved by one float32 ulp up and down (a few bf16 roundings of the rows flip).
tolerance = 4 x max(a, b), floored at 1e-6; relative to max |reference| for the gradients and the per-row loss shares, relative to
the reference for the loss.  The factor covers the summation orders neither mirror reproduces (MFMA accumulation, up to eight
column-split partials).  The fp32-path cases (f32_*) have (a) only, against the exact fp64 loss.  The cycle-consistency cases have
the float32 mirror only, with a factor of 8: the kernel's __expf is the dominant term and the mirror's exp is correctly rounded.

    python tools/gen_loss_tolerances.py            # rewrite the file
    python tools/gen_loss_tolerances.py --check    # recompute and compare with the file
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import loss_cases as LC  # noqa: E402

PATH = os.path.join(ROOT, "tests", "golden", "loss_tolerances.json")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--check", action="store_true")
    ap.add_argument("--only", nargs="*")
    a = ap.parse_args()
    tol = LC.all_tolerances(a.only, log=lambda k, v: print(f"{k:34s} loss {v['loss']:.2e} grad {v['grad']:.2e} rows {v['rows']:.2e}", flush=True))
    rnd = {k: {n: float(f"{x:.6e}") for n, x in v.items()} for k, v in tol.items()}
    if a.check:
        have = json.load(open(PATH))
        bad = [k for k, v in rnd.items() if any(abs(have[k][n] - x) > 1e-6 * abs(x) for n, x in v.items())]
        print("mismatch: " + ", ".join(bad) if bad else f"{len(rnd)} cases match {PATH}")
        return 1 if bad else 0
    if a.only:
        have = json.load(open(PATH))
        have.update(rnd)
        rnd = have
    with open(PATH, "w") as f:
        json.dump(rnd, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"wrote {len(rnd)} cases to {PATH}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
