"""Times permutations of basis states under controls (qsim_apply_permutation) against the sweeps a caller had before and writes ONE
JSON file.

  python tools/permutation_bench.py [--n 30] [--reps 7] [--out profiles/permutation/permutation_n30.json] [--quick]

The state is the bench's random circuit (bench.py's seed) at n qubits.  Every row is timed with HIP events on the state's stream
around the call (which does not wait), warm, median of --reps (>= 5), with the fastest and the slowest repetition beside it.  Rows,
per precision (64, 32), for k = 1, 5, 9, 10 targets — low (qubits 0..k-1; 1..k under a control on qubit 0), spread (evenly spaced
from qubit 1), top (the top k below the controls) — and controls: none, 1, 2 and 4 high ones (the top qubits), one on qubit 0:
  perm_k<k>_<targets>_<controls>_random   a random table through qsim_apply_permutation
  perm_k<k>_<targets>_<controls>_modmul   permutations.modular_multiply_table(a, N, k), N the largest prime below 2^k (k = 1: the identity)
  rot_k<k>_<targets>_<controls>           the yardstick: ONE Pauli rotation on the same qubits under the same controls, the sweep that
                                          reads and writes the same bytes once (X Z X ... on the targets; k = 1: Z).  x_rot of a perm
                                          row = its time / this row's time.
  matrix_k<k>_<targets>_<controls>        k <= 5: qsim_apply_matrix with the random table as a matrix.  x_matrix of the perm row likewise.
tile_rule: k = 10 on top targets (two padding bits in fp64: runs of 64 bytes) over k = 9 there (three: 128 bytes), without controls.
--quick: the permutation rows without controls only, no yardsticks (what a counter run under a profiler repeats).
Each precision runs in a child process of its own under `timeout -k 10`; the first failure ends the run."""
import argparse
import ctypes
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)

KS = (1, 5, 9, 10)
MODMUL = {1: (1, 2), 5: (7, 31), 9: (7, 509), 10: (7, 1021)}  # (a, N): N the largest prime below 2^k


def control_sets(n):
    return {"c0": [], "c1": [n - 1], "c2": [n - 1, n - 2], "c4": [n - 1, n - 2, n - 3, n - 4], "cq0": [0]}


def targets(n, k, top, low_from):
    """top: the first qubit above the targets (below the high controls); low_from: 1 when qubit 0 is a control"""
    return {"low": list(range(low_from, low_from + k)), "spread": [1 + (j * (top - 2)) // max(k - 1, 1) for j in range(k)] if k > 1 else [top // 2],
            "top": list(range(top - k, top))}


def child(args):
    import numpy as np
    from gpu_quantum_simulator_amd import Circuit, Simulator, circuits, permutations
    import torch
    n = args.n
    hip = ctypes.CDLL("libamdhip64.so.7")  # the runtime libqsim.so itself is linked against
    ev = [ctypes.c_void_p(), ctypes.c_void_p()]
    for e in ev:
        assert hip.hipEventCreate(ctypes.byref(e)) == 0
    rng = np.random.default_rng(7)
    rows = {"device": torch.cuda.get_device_name(0)}
    c = Circuit.from_gates(n, circuits.random_gates(n, 1000, 20240117 + n, "all"))
    with Simulator(n, precision=args.precision) as sim:
        sim.run(c)
        sim.sync()
        stream = ctypes.c_void_p(sim.stream)

        def timed(name, fn):
            fn()  # warm
            sim.sync()
            ms = []
            for _ in range(max(5, args.reps)):
                assert hip.hipEventRecord(ev[0], stream) == 0
                fn()
                assert hip.hipEventRecord(ev[1], stream) == 0
                assert hip.hipEventSynchronize(ev[1]) == 0
                t = ctypes.c_float()
                assert hip.hipEventElapsedTime(ctypes.byref(t), ev[0], ev[1]) == 0
                ms.append(t.value)
            rows[name] = {"ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4)}
            return rows[name]

        for cname, controls in control_sets(n).items():
            if args.quick and cname != "c0":
                continue
            top = n - len(controls) if cname != "cq0" else n
            for k in KS:
                for tname, qs in targets(n, k, top, 1 if cname == "cq0" else 0).items():
                    tables = {"random": rng.permutation(1 << k), "modmul": permutations.modular_multiply_table(*MODMUL[k], k)}
                    rot = mat = None
                    if not args.quick:
                        text = " ".join(("X" if j % 2 == 0 else "Z") + str(q) for j, q in enumerate(qs)) if k > 1 else f"Z{qs[0]}"
                        rot = timed(f"rot_k{k}_{tname}_{cname}", lambda: sim.apply_pauli_rotation(0.37, text, controls))
                        if k <= 5:
                            U = np.zeros((1 << k, 1 << k))
                            U[tables["random"], np.arange(1 << k)] = 1.0
                            mat = timed(f"matrix_k{k}_{tname}_{cname}", lambda: sim.apply_matrix(U, qs, controls))
                    for pname, table in tables.items():
                        row = timed(f"perm_k{k}_{tname}_{cname}_{pname}", lambda: sim.apply_permutation(table, qs, controls))
                        row["targets"], row["controls"] = qs, controls
                        if rot:
                            row["x_rot"] = round(row["ms"] / rot["ms"], 3)
                        if mat:
                            row["x_matrix"] = round(row["ms"] / mat["ms"], 3)
        rows["tile_rule_k10_over_k9_top"] = round(rows["perm_k10_top_c0_random"]["ms"] / rows["perm_k9_top_c0_random"]["ms"], 3)
        rows["norm2_after"] = sim.norm2()  # permutations and rotations throughout: the state's norm after all the sweeps
    print("ROWS " + json.dumps(rows), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=30)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--precision", type=int, default=64)
    args = ap.parse_args()
    if args.child:
        return child(args)
    result = {"n": args.n, "reps": max(5, args.reps), "quick": args.quick, "fp64": {}, "fp32": {}}
    for precision in (64, 32):  # the parent never opens the GPU
        cmd = ["timeout", "-k", "10", "420", sys.executable, os.path.abspath(__file__), "--child", "--n", str(args.n), "--reps", str(args.reps),
               "--precision", str(precision)] + (["--quick"] if args.quick else [])
        p = subprocess.run(cmd, capture_output=True, text=True)
        lines = [ln for ln in p.stdout.splitlines() if ln.startswith("ROWS ")]
        if p.returncode != 0 or not lines:  # nothing more is started on the GPU after a failure
            sys.stderr.write(p.stdout[-2000:] + p.stderr[-2000:])
            sys.exit(p.returncode or 1)
        result[f"fp{precision}"] = json.loads(lines[-1][5:])
    out = args.out or os.path.join(ROOT, "profiles", "permutation", f"permutation_n{args.n}.json")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result)[:3000])


if __name__ == "__main__":
    main()
