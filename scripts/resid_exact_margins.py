#!/usr/bin/env python3
"""Run the float64-bound cases of tests/resid_exact.py once over the HIP kernels and write the worst share of each
bound (err / e per family) to profiles/resid/resid_exact_mi355x.json.  The bounds themselves are derived in
tests/resid_exact.py and asserted by tests/test_resid_exact_gpu.py; this file records how much room they leave.

    python scripts/resid_exact_margins.py [--out profiles/resid/resid_exact_mi355x.json]
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import resid_exact as rx  # noqa: E402
from llm_based_apache_spark_optimization_amd import ops  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "resid", "resid_exact_mi355x.json"))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    ops.ext()
    for D in rx.NORM_D:
        rx.norm_suite(dev, D)
    for form in rx.NORM_FORMS[1:]:
        rx.norm_forms_suite(dev, form)
    rx.norm_spike_suite(dev)
    with rx.forced_xf_kernel():
        for rows in (65, 71, 80):
            rx.norm_xf_suite(dev, rows)
    for D in rx.RES_D:
        rx.res_suite(dev, D)
    for HH in [(4, 2), (24, 8)]:
        for mode in ("real", "real8"):
            rx.rope_suite(dev, HH, mode)
    rx.silu_small_suite(dev, bf16_fn=rx.silu_bf16_fn)
    rx.silu_parts_check(ops.silu_parts, dev, 1, rx.SILU_PARTS_CAP + 4096, 1, key="silu_parts/cap")
    rx.silu_mul_check(ops.silu_mul, dev, rx.SILU_MUL_CAP + 2056, key="silu_mul/cap")
    rx.silu_bf16_check(rx.silu_bf16_fn, dev, 1, rx.SILU_BF16_CAP + 4096, key="silu_bf16/cap")
    rec = {"unit": "worst err / e per family: the distance from the float64 result to the reals that round to the "
                   "kernel's output, over the slack e of tests/resid_exact.py (fp8 rows and Q24 sums: error / bound)",
           "bound": 1.0, "device": torch.cuda.get_device_properties(0).gcnArchName.split(":")[0],
           "worst": {k: round(v, 4) for k, v in sorted(rx.RATIOS.items())}}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(json.dumps(rec["worst"]))


if __name__ == "__main__":
    main()
