"""Times measurement on the device (qsim_postselect, qsim_measure) against what the bytes say and against the three-line collapse it
replaces, and writes ONE JSON file.

  python tools/measure_bench.py [--n 30] [--reps 7] [--out profiles/measure/measure_n30.json]

The state is a short random circuit (bench.py's seed, 200 gates) at n qubits; the times do not depend on the values.  Every row is timed
with HIP events on the state's stream around the call, warm, median of --reps (>= 5), with the fastest and the slowest repetition beside
it; `wall_ms` is the host's clock around the same calls (a call waits once for its weight, so the host sees it end).  Rows, per precision
(64, 32):
  norm2                         the unit: one read of the state (16 bytes per fp64 amplitude); every model below is a multiple of it
  postselect_<case>             k = 1 on qubit 0, on the middle qubit and on the top one, k = 2, 5, 10 and 20
  measure_<case>                the same qubits: the sampler's pyramid and one draw, then the same two sweeps
  three_line_<case>             k = 1 only: marginal_probabilities, apply_matrix with the projector, scale — and the flush that runs the scale
Beside every row: `model` = the sweeps' bytes as a multiple of one read of the state (postselect 2 r + 1 with r the share of the 16-byte
units the plan call reports for the weight sweep, measure one more, three lines 5), and `x_model` = ms / (model * norm2's ms); `lines_model` and `x_lines_model` are the same with r counted in whole
128-byte lines, which a measured qubit inside a line (qubits 0-2 in fp64, 0-3 in fp32) thins without sparing.  The three lines are timed on a state that is
spread out again before every repetition, outside the clock: on a collapsed state their scale would be the identity.
`measure_over_three_line` compares the two k = 1 rows of each qubit.  Each precision runs in a child process of its own under
`timeout -k 10`; the first failure ends the run."""
import argparse
import ctypes
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)


def cases(n):
    top, mid = n - 1, n // 2
    spread = lambda k: sorted({(j * (n - 1)) // (k - 1) for j in range(k)})
    out = {"k1_q0": [0], f"k1_q{mid}": [mid], f"k1_q{top}": [top], "k2": [min(3, n - 2), top - 2], "k5": spread(5), "k10": spread(10)}
    if n >= 22:
        out["k20"] = list(range(1, 21))
    return {name: qs for name, qs in out.items() if len(set(qs)) == len(qs) and len(qs) <= n}


def child(args):
    import numpy as np
    from gpu_quantum_simulator_amd import Circuit, Simulator, circuits, _lib, plans
    import torch
    n = args.n
    _lib.load()  # libqsim (and torch's HIP runtime, where there is one) before anything else opens the device
    hip = ctypes.CDLL("libamdhip64.so.7")  # the runtime libqsim.so itself is linked against
    ev = [ctypes.c_void_p(), ctypes.c_void_p()]
    for e in ev:
        assert hip.hipEventCreate(ctypes.byref(e)) == 0
    rows = {"device": torch.cuda.get_device_name(0)}
    reps = max(5, args.reps)
    c = Circuit.from_gates(n, circuits.random_gates(n, 200, 20240117 + n, "all"))
    with Simulator(n, precision=args.precision) as sim:
        sim.run(c)
        sim.sync()
        stream = ctypes.c_void_p(sim.stream)

        def timed(name, fn, prepare=None):
            if prepare:
                prepare()
            fn()  # warm: scratch is allocated, plans are cached
            sim.sync()
            ms, wall = [], []
            for _ in range(reps):
                if prepare:  # outside the clock
                    prepare()
                t0 = time.perf_counter()
                assert hip.hipEventRecord(ev[0], stream) == 0
                fn()
                assert hip.hipEventRecord(ev[1], stream) == 0
                assert hip.hipEventSynchronize(ev[1]) == 0
                wall.append((time.perf_counter() - t0) * 1e3)
                t = ctypes.c_float()
                assert hip.hipEventElapsedTime(ctypes.byref(t), ev[0], ev[1]) == 0
                ms.append(t.value)
            rows[name] = {"ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4),
                          "wall_ms": round(statistics.median(wall), 4)}
            return rows[name]

        unit = timed("norm2", sim.norm2)
        unit["gbytes_per_s"] = round((16 if args.precision == 64 else 8) * (1 << n) / (unit["ms"] * 1e-3) / 1e9, 1)

        line_bit = 3 if args.precision == 64 else 4  # amplitude bits inside a 128-byte line

        def modelled(row, reads, r, rest, qs):
            """reads: how many sweeps read the kept subspace, r: its share of the 16-byte units; rest: what else the row moves, in reads of the whole state"""
            r_lines = 0.5 ** sum(1 for q in qs if q >= line_bit)
            row["qubits"], row["model"], row["lines_model"] = qs, round(reads * r + rest, 6), round(reads * r_lines + rest, 6)
            row["x_model"] = round(row["ms"] / (row["model"] * unit["ms"]), 3)
            row["x_lines_model"] = round(row["ms"] / (row["lines_model"] * unit["ms"]), 3)
            return row

        def spread_out():  # the three lines are timed on a state that is not collapsed yet: on a collapsed one the scale is the identity
            sim.run(c)
            sim.sync()

        for name, qs in cases(n).items():
            k = len(qs)
            p = plans.ok(plans.collapse_plan(qs, 0, n, args.precision))
            r = p["weight_units"] / p["collapse_units"]
            outcome = sim.measure(qs, draw=0.5)  # an outcome that has a probability; the state is collapsed onto it from here on
            before = plans.sweeps_launched("collapse")
            modelled(timed(f"postselect_{name}", lambda: sim.postselect(qs, outcome)), 2, r, 1, qs)
            modelled(timed(f"measure_{name}", lambda: sim.measure(qs, draw=0.5)), 2, r, 2, qs)
            assert plans.sweeps_launched("collapse") - before == 4 * (reps + 1)
            if k == 1:
                proj = np.zeros((2, 2))
                proj[outcome, outcome] = 1.0

                def three_lines():
                    p = sim.marginal_probabilities(qs)
                    sim.apply_matrix(proj, qs)
                    sim.scale(1.0 / np.sqrt(p[outcome]))
                    sim.flush()

                row = modelled(timed(f"three_line_{name}", three_lines, spread_out), 0, 1.0, 5, qs)
                row["measure_over_three_line"] = round(rows[f"measure_{name}"]["ms"] / row["ms"], 3)
                row["postselect_over_three_line"] = round(rows[f"postselect_{name}"]["ms"] / row["ms"], 3)
            sim.run(c)  # spread the state out again for the next case
            sim.sync()
    print("ROWS " + json.dumps(rows), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=30)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--precision", type=int, default=64)
    args = ap.parse_args()
    if args.child:
        return child(args)
    result = {"n": args.n, "reps": max(5, args.reps), "fp64": {}, "fp32": {}}
    for precision in (64, 32):  # the parent never opens the GPU
        cmd = ["timeout", "-k", "10", "300", sys.executable, os.path.abspath(__file__), "--child", "--n", str(args.n), "--reps", str(args.reps),
               "--precision", str(precision)]
        p = subprocess.run(cmd, capture_output=True, text=True)
        lines = [ln for ln in p.stdout.splitlines() if ln.startswith("ROWS ")]
        if p.returncode != 0 or not lines:  # nothing more is started on the GPU after a failure
            sys.stderr.write(p.stdout[-2000:] + p.stderr[-2000:])
            sys.exit(p.returncode or 1)
        result[f"fp{precision}"] = json.loads(lines[-1][5:])
    out = args.out or os.path.join(ROOT, "profiles", "measure", f"measure_n{args.n}.json")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result)[:8000])


if __name__ == "__main__":
    main()
