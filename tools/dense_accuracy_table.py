#!/usr/bin/env python3
"""The table of profiles/dense_accuracy.md: the scaled error e (tests/numeric_ref.py) of every matrix-core dense kernel and of the
oracle against the higher-precision reference, on the runs of tests/test_gpu_a_dense_accuracy.py — needs an MI355X.

One row per kernel x precision x k x matrix form x input class, pooled over the state sizes and target placements of the case
table: rms(e) and max|e| of the oracle and of the kernel, their ratios, and the derived bound on max|e|.

    python tools/dense_accuracy_table.py > table.md
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import numpy as np  # noqa: E402

import numeric_ref as nr  # noqa: E402
import rustqip_amd as q  # noqa: E402
from oracle import qip_oracle as O  # noqa: E402

FORMS = {"k_gate_kq_mfma": "four products", "k_gate_tile_mfma_k4": "four products", "k_gate_tile_mfma_k5": "four products",
         "k_gate_big_mfma": "three products", "k_gate_huge_mfma": "three products"}


def main():
    rows = {}
    for kc in nr.kernel_cases():
        with nr.HipRunner(q, kc) as dev:
            for runs in nr.accuracy_parts(kc).values():
                for _, targets, controls, mk, ik in runs:
                    real = mk == "orth" and kc.kernel in ("k_gate_tile_mfma_k5", "k_gate_big_mfma", "k_gate_huge_mfma")
                    form = "two products" if real else FORMS[kc.kernel]
                    cls = ik if mk == kc.matrix else f"{ik}, matrix {mk}"
                    key = (kc.kernel, "f64" if kc.dtype == np.complex128 else "f32", kc.k, form, cls)
                    rows.setdefault(key, []).append(nr.measure(O, q, dev, kc, targets, controls, mk, ik))
            print(f"measured {kc.id}", file=sys.stderr, flush=True)
    print("| kernel | precision | k | form | input class | runs | oracle rms(e) | oracle max\\|e\\| | kernel rms(e) | kernel max\\|e\\| | rms ratio | max ratio | hard bound |")
    print("|---|---|---|---|---|---|---|---|---|---|---|---|---|")
    worst = 0.0
    for (kernel, prec, k, form, cls), res in rows.items():
        ek, eo = nr.pool([r[0] for r in res]), nr.pool([r[1] for r in res])
        worst = max(worst, ek[0] / eo[0])
        print(f"| {kernel} | {prec} | {k} | {form} | {cls} | {len(res)} | {eo[0]:.3f} | {eo[1]:.2f} | {ek[0]:.3f} | {ek[1]:.2f} | "
              f"{ek[0] / eo[0]:.2f} | {ek[1] / eo[1]:.2f} | {nr.hard_bound(k)} |")
    print(f"\nLargest rms ratio of a row: {worst:.2f}.")


if __name__ == "__main__":
    main()
