"""Times dense matrices on target qubits under controls (qsim_apply_matrix) against the sweeps a caller had before and writes ONE
JSON file.

  python tools/matrix_bench.py [--n 30] [--reps 7] [--out profiles/matrix/matrix_n30.json]

The state is the bench's random circuit (bench.py's seed) at n qubits.  Every row is timed with HIP events on the state's stream
around the call (which does not wait), warm, median of --reps (>= 5), with the fastest and the slowest repetition beside it.  Rows,
per precision (64, 32), for k = 1..5 targets — low (qubits 0..k-1; 1..k under a control on qubit 0), high (the top k below the
controls), spread (evenly spaced from qubit 1) — and controls: none, 1, 2 and 4 high ones (the top qubits), one on qubit 0:
  matrix_k<k>_<targets>_<controls>   a random unitary through qsim_apply_matrix
  rot_k<k>_<targets>_<controls>      the yardstick: ONE Pauli rotation on the same qubits under the same controls, the sweep that moves
                                     the same bytes (X Z X ... on the targets; k = 1: Z, a single X is a queued gate, not a sweep).
                                     x_rot of the matrix row = its time / this row's time.
  gate2_<targets>                    k = 2 without controls: apply_2q followed by flush.  x_gate2 of the matrix row likewise.
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


def control_sets(n):
    return {"c0": [], "c1": [n - 1], "c2": [n - 1, n - 2], "c4": [n - 1, n - 2, n - 3, n - 4], "cq0": [0]}


def targets(n, k, top, low_from):
    """top: the first qubit above the targets (below the high controls); low_from: 1 when qubit 0 is a control"""
    return {"low": list(range(low_from, low_from + k)), "high": list(range(top - k, top)),
            "spread": [1 + (j * (top - 2)) // max(k - 1, 1) for j in range(k)] if k > 1 else [top // 2]}


def child(args):
    import numpy as np
    from gpu_quantum_simulator_amd import Circuit, Simulator, circuits
    n = args.n
    hip = ctypes.CDLL("libamdhip64.so.7")  # the runtime libqsim.so itself is linked against
    ev = [ctypes.c_void_p(), ctypes.c_void_p()]
    for e in ev:
        assert hip.hipEventCreate(ctypes.byref(e)) == 0
    rng = np.random.default_rng(7)
    rows = {}
    c = Circuit.from_gates(n, circuits.random_gates(n, 1000, 20240117 + n, "all"))
    with Simulator(n, precision=args.precision) as sim:
        sim.run(c)
        sim.sync()
        stream = ctypes.c_void_p(sim.stream)

        def unitary(dim):
            q, r = np.linalg.qr(rng.standard_normal((dim, dim)) + 1j * rng.standard_normal((dim, dim)))
            return q * (np.diag(r) / np.abs(np.diag(r)))

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
            top = n - len(controls) if cname != "cq0" else n
            for k in range(1, 6):
                for tname, qs in targets(n, k, top, 1 if cname == "cq0" else 0).items():
                    U = unitary(1 << k)
                    text = " ".join(("X" if j % 2 == 0 else "Z") + str(q) for j, q in enumerate(qs)) if k > 1 else f"Z{qs[0]}"
                    rot = timed(f"rot_k{k}_{tname}_{cname}", lambda: sim.apply_pauli_rotation(0.37, text, controls))
                    row = timed(f"matrix_k{k}_{tname}_{cname}", lambda: sim.apply_matrix(U, qs, controls))
                    row["targets"], row["controls"], row["x_rot"] = qs, controls, round(row["ms"] / rot["ms"], 3)
                    if k == 2 and not controls:
                        def gate2():
                            sim.apply_2q(U, max(qs), min(qs))
                            sim.flush()
                        row["x_gate2"] = round(row["ms"] / timed(f"gate2_{tname}", gate2)["ms"], 3)
        rows["norm2_after"] = sim.norm2()  # unitaries throughout: the state's norm after some 1500 sweeps
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
        cmd = ["timeout", "-k", "10", "420", sys.executable, os.path.abspath(__file__), "--child", "--n", str(args.n), "--reps", str(args.reps),
               "--precision", str(precision)]
        p = subprocess.run(cmd, capture_output=True, text=True)
        lines = [ln for ln in p.stdout.splitlines() if ln.startswith("ROWS ")]
        if p.returncode != 0 or not lines:  # nothing more is started on the GPU after a failure
            sys.stderr.write(p.stdout[-2000:] + p.stderr[-2000:])
            sys.exit(p.returncode or 1)
        result[f"fp{precision}"] = json.loads(lines[-1][5:])
    out = args.out or os.path.join(ROOT, "profiles", "matrix", f"matrix_n{args.n}.json")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result)[:3000])


if __name__ == "__main__":
    main()
