"""Per-sweep table of the headline's default-path tile sweeps from a rocprofv3 kernel trace of
`bench.py --headline-only --steps K --warmup W` (K + W steps of 15 sweeps each, after the product-state preparation).

    python tools/sweep_table.py <..._kernel_trace.csv> [steps] [parent]

Host-only: the gate list of each sweep comes from the mode-1 tile plan (qip_hip_debug_tile_plan), the times from the
last `steps` x (sweeps per step) k_tile_passes dispatches of the trace; prints a markdown table."""
import csv
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from rustqip_amd import circuits  # noqa: E402
from rustqip_amd.ops import debug_tile_plan  # noqa: E402

N, GATES = 30, 256
HBM = 8.0e12


def main(path, steps, parent=False):
    ops = circuits.c2_random_circuit(N, GATES, seed=28, single_only=True)
    # the lists the interpreter is handed: uncontrolled X gates absorbed (mode bit 4096); `parent`: a trace of a build from before
    # that rewrite, the plan's own lists
    plan = [s if parent else s["absorb"] for s in debug_tile_plan(N, ops, 1 | (0 if parent else 4096))["steps"] if len(s["ops"]) >= 2]
    rows = [r for r in csv.DictReader(open(path)) if "k_tile_passes" in r["Kernel_Name"]]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    per = len(plan)
    timed = rows[-steps * per:]
    sweep_bytes = 2.0 * 16 * (1 << N)
    print("| sweep | gates | H | X | Rz | passes | mean ms | min ms | max ms | % of 8 TB/s |")
    print("|---|---|---|---|---|---|---|---|---|---|")
    means = []
    for i, st in enumerate(plan):
        ms = [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) * 1e-6 for r in timed[i::per]]
        g = st["gates"]
        nx = sum(1 for x in g if x["kind"] == 0 and x["b1"] & 2)
        nh = sum(1 for x in g if x["kind"] == 0 and not x["b1"] & 2)
        nd = sum(1 for x in g if x["kind"] == 1)
        m = statistics.mean(ms)
        means.append(m)
        print(f"| {i} | {len(g)} | {nh} | {nx} | {nd} | {len(st['passes'])} | {m:.3f} | {min(ms):.3f} | {max(ms):.3f} | "
              f"{100 * sweep_bytes / (m * 1e-3) / HBM:.1f} |")
    mean = statistics.mean(means)
    print(f"\nmean sweep {mean:.3f} ms ({100 * sweep_bytes / (mean * 1e-3) / HBM:.1f} % of 8 TB/s), sum {sum(means):.1f} ms per step, "
          f"{steps} steps x {per} sweeps")


if __name__ == "__main__":
    main(sys.argv[1], int(sys.argv[2]) if len(sys.argv) > 2 else 4, parent=len(sys.argv) > 3 and sys.argv[3] == "parent")
