"""bench.py's contract line without a GPU (BENCH_r05.json had `parsed: null` — the one JSON line had grown to
24 KB).  The line is built by a pure function from a result dict: here from a canned result with everything at its worst case
(N = 8, every optional field present, non-finite numbers in the input)."""
import json
import math
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402

REQUIRED = ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline",
            "dtype", "data", "config", "roofline", "cpu_baseline", "parity_ok", "parity")


def canned(world=1, parity_ok=True):
    res = {
        "n_gpus": world, "steps": 20, "warmup": 5, "n_local": 30, "gates": 256, "n": 30 + int(math.log2(world)),
        "value": 6531.123456789 * world, "ms_per_step": 1346.7891234, "bytes_per_step": 256 * 32 * 2 ** (30 + int(math.log2(world))),
        "gates_per_s": 190.1234567, "norm_sqr": 0.9999999999999,
        "roofline": {"bound": "hbm", "kernel": "k_tile_passes", "achieved": 6513.77, "peak": 8000.0, "unit": "GB/s", "frac": 0.81422,
                     "traffic": 3.4381e10, "traffic_source": "static: profiles/r06_pmc_traffic.md (separate rocprofv3 --pmc passes of this command)",
                     "traffic_stale": False, "avg_launch_ms": 5.275, "launches": 2620, "algorithmic_bytes_per_launch": 34359738368.0},
        "cpu_baseline": {"value": 37.1, "unit": "GB/s", "cores": 16, "kind": "port", "gates_per_s": 4.3, "ms_per_gate": 231.5,
                         "sample": "first 8 gates of the headline circuit at n=28 (2 x 4 GiB), C restatement of qip-iterators 1.5.0 "
                                   "apply_op_overwrite, gcc -O3 -fopenmp, 16 threads, median of 3 (5.6 s CPU work)",
                         "detail": {"big": list(range(1000))}},
        "parity_ok": parity_ok,
        "parity": {"checker": "CPU oracle on closed sub-cubes + twin state over all 2^n amplitudes", "n": 30, "legs": 24, "legs_failed": [] if parity_ok else ["x" * 60] * 6,
                   "gates_checked": 2258, "rows_checked": 575275008, "max_abs_delta_IEEE_legs": 0.0, "max_abs_delta_1e-12_legs": float("nan"),
                   "whole_vector_compares": 141, "whole_vector_amplitudes_not_equal_IEEE_legs": 0, "seconds": 61.2},
        "extras_skipped": [{"section": "tolerance"}],
    }
    if world > 1:
        res.update({"rccl_ranks": world, "per_gpu_efficiency": 0.83123456, "per_gpu_efficiency_reference": {"value": 6531.0, "source": "profiles/n1_reference.json"},
                    "comm": {"remaps": 12, "pack_sweeps": 3, "bytes_sent": 1 << 40, "exchange_ms": float("inf"), "pack_ms": 61.0, "rccl_ranks": world, "rccl_rank": 0,
                             "pieces_sent": 84, "piece_bytes": 1 << 30, "packs_via_permute": 1, "packs_folded": 9, "remaps_overlapped": 0,
                             "remaps_overlapped_after": 0, "slices_overlapped": 0}})
    return res


def test_contract_line_is_compact_valid_json_with_the_required_keys():
    for world in (1, 2, 8):
        for ok in (True, False, None):
            text = bench.contract_line(dict(canned(world, ok), stage="final"))
            assert len(text) < bench.CONTRACT_MAX_BYTES and "\n" not in text, len(text)
            assert "NaN" not in text and "Infinity" not in text
            line = json.loads(text, parse_constant=lambda c: (_ for _ in ()).throw(ValueError(c)))
            for key in REQUIRED:
                assert key in line, key
            assert line["n_gpus"] == world and line["unit"] == "GB/s" and line["dtype"] == "f64" and line["config"]["workload"]
            assert set(("bound", "achieved", "peak", "unit", "frac", "traffic")) <= set(line["roofline"])
            assert set(("value", "unit", "cores", "kind", "sample")) <= set(line["cpu_baseline"]) and "detail" not in line["cpu_baseline"]
            if ok is False:  # a failed parity withholds the value
                assert line["value"] is None and line["value_withheld"] > 0 and line["parity_ok"] is False
            else:
                assert line["value"] > 0
            if world > 1:
                assert line["rccl_ranks"] == world and 0 < line["per_gpu_efficiency"] < 1 and line["comm"]["remaps"] == 12
                assert line["comm"]["exchange_ms"] is None  # (a non-finite number becomes null, never a bare token)


def test_bench_cli_contract_without_a_gpu():
    """the flags the driver passes parse; without a device the script fails loudly (no CPU fallback) instead of printing a line"""
    a = bench.parse_args(["--gpus", "1", "--steps", "20", "--warmup", "5"])
    assert (a.gpus, a.steps, a.warmup, a.n_local, a.gates) == (1, 20, 5, 30, 256) and a.budget_s > 0
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "1", "--warmup", "0"], capture_output=True, text=True, timeout=300,
                       env=dict(os.environ, QIP_BENCH_DETAIL=os.devnull))
    assert p.returncode != 0 and "needs a HIP device" in (p.stderr + p.stdout)
    assert not [l for l in p.stdout.splitlines() if l.startswith("{")]


def test_bench_dump_outputs_flag_and_files(tmp_path):
    """--dump-outputs DIR parses, --steps 0 is refused, and the writer puts float64 arrays of at most 64 MB under DIR: the whole
    vector of a small state, a fixed seeded sample (same rows every time) of a large one"""
    import numpy as np
    import pytest

    assert bench.parse_args(["--steps", "3", "--dump-outputs", str(tmp_path)]).dump_outputs == str(tmp_path)
    assert bench.parse_args([]).dump_outputs == ""
    for bad in (["--steps", "0"], ["--warmup", "-1"]):
        with pytest.raises(SystemExit):
            bench.parse_args(bad)

    class FakeState:  # HipState.download_indices over a host vector whose amplitude k is k + 0.5j
        def download_indices(self, idx):
            idx = np.asarray(idx, dtype=np.uint64)
            assert idx.size and int(idx.max()) < 1 << n
            return idx.astype(np.float64) + 0.5j

    for n, rows in ((4, 16), (30, None)):
        dumps = []
        for rep in range(2):
            d = tmp_path / f"{n}_{rep}"
            nbytes = bench.dump_outputs(str(d), FakeState(), n, 0.75, 0)
            files = {p.name: np.load(p) for p in d.iterdir()}
            assert set(files) == {"state.npy", "state_index.npy", "norm_sqr.npy"} and nbytes <= 64 << 20
            assert all(a.dtype == np.float64 for a in files.values()) and sum(a.nbytes for a in files.values()) == nbytes
            state, index = files["state.npy"], files["state_index.npy"]
            assert state.shape == (index.size, 2) and np.array_equal(state[:, 0], index) and np.all(state[:, 1] == 0.5)
            assert files["norm_sqr.npy"].tolist() == [0.75] and np.all(np.diff(index) > 0)
            assert index.size == rows if rows else bench.DUMP_SAMPLE // 2 < index.size <= bench.DUMP_SAMPLE
            dumps.append(index)
        assert np.array_equal(*dumps)
    assert bench.dump_outputs(str(tmp_path / "rank1"), FakeState(), 4, 1.0, 1) == 0 and not (tmp_path / "rank1").exists()


def test_bench_plain_run_times_the_headline_alone_and_full_adds_the_rest():
    """without --full a run skips the parity checks, the CPU baseline and the extras; --full runs them, and the --no-* flags and
    --headline-only trim it as before"""
    plain = bench.parse_args(["--gpus", "1", "--steps", "20", "--warmup", "5"])
    assert not plain.full and plain.no_parity and plain.no_cpu_baseline and plain.no_extras
    full = bench.parse_args(["--gpus", "1", "--steps", "20", "--warmup", "5", "--full"])
    assert full.full and not (full.no_parity or full.no_cpu_baseline or full.no_extras)
    trimmed = bench.parse_args(["--full", "--no-extras", "--no-cpu-baseline"])
    assert trimmed.no_extras and trimmed.no_cpu_baseline and not trimmed.no_parity
    assert bench.parse_args(["--full", "--headline-only"]).headline_only
