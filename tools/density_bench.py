"""Times reduced density matrices (qsim_reduced_density) against two yardsticks on one state and writes ONE JSON file.

  python tools/density_bench.py [--n 30] [--reps 7] [--out profiles/density/density_n30.json]

The state is the bench's random circuit (bench.py's seed) at n qubits.  Every row is timed with HIP events on the state's stream,
warm, median of --reps (>= 5), with the fastest and the slowest repetition beside it.  Rows, per precision (64, 32):
  norm2                      the floor: one read of the state, nothing written
  rho_k<k>_<subset>          rho of k = 1..5 qubits, one sweep; subset: low (qubits 0..k-1), high (the top k), spread (evenly spaced, qubit
                             0 excluded).  The call allocates its scratch, waits for its result and assembles rho on the host: all inside the
                             events.  x_floor = time / norm2's time.
  pauli_k<k>_<subset>        the route a caller had before: the same rho assembled from qsim_expect_paulis over all 4^k strings on the
                             subset (2^k x_mask groups: 2^k sweeps).  x_rho = time / the rho row's time.
max_abs_diff_routes is the largest difference between the two routes' matrices over all shapes.
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


def subsets(n, k):
    return {"low": list(range(k)), "high": list(range(n - k, n)), "spread": [1 + (j * (n - 2)) // max(k - 1, 1) for j in range(k)] if k > 1 else [n // 2]}


def child(args):
    import numpy as np
    from gpu_quantum_simulator_amd import Circuit, Simulator, circuits
    n = args.n
    hip = ctypes.CDLL("libamdhip64.so.7")  # the runtime libqsim.so itself is linked against
    ev = [ctypes.c_void_p(), ctypes.c_void_p()]
    for e in ev:
        assert hip.hipEventCreate(ctypes.byref(e)) == 0
    sigma = {"I": np.eye(2), "X": np.array([[0, 1], [1, 0]]), "Y": np.array([[0, -1j], [1j, 0]]), "Z": np.diag([1.0, -1.0])}
    rows = {}
    c = Circuit.from_gates(n, circuits.random_gates(n, 1000, 20240117 + n, "all"))
    with Simulator(n, precision=args.precision) as sim:
        sim.run(c)
        sim.sync()
        stream = ctypes.c_void_p(sim.stream)

        def timed(name, fn):
            fn()  # warm
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

        def from_paulis(qs):
            letters = [""]
            for _ in qs:
                letters = [w + l for w in letters for l in "IXYZ"]  # letter j of a word is on qs[j]
            values = sim.expectation_terms([" ".join(f"{l}{q}" for l, q in zip(w, qs) if l != "I") for w in letters])
            rho = np.zeros((1 << len(qs), 1 << len(qs)), dtype=np.complex128)
            for v, w in zip(values, letters):
                p = np.eye(1)
                for l in w:
                    p = np.kron(sigma[l], p)                       # qs[0] is the low bit
                rho += v * p
            return rho / (1 << len(qs))

        floor = timed("norm2", sim.norm2)["ms"]
        worst = 0.0
        for k in range(1, 6):
            for name, qs in subsets(n, k).items():
                r = timed(f"rho_k{k}_{name}", lambda: sim.reduced_density_matrix(qs))
                r["qubits"], r["x_floor"] = qs, round(r["ms"] / floor, 3)
                p = timed(f"pauli_k{k}_{name}", lambda: from_paulis(qs))
                p["sweeps"], p["x_rho"] = 1 << k, round(p["ms"] / r["ms"], 2)
                worst = max(worst, float(np.max(np.abs(from_paulis(qs) - sim.reduced_density_matrix(qs)))))
        timed("norm2_again", sim.norm2)  # the yardstick's own drift over the run
        rows["max_abs_diff_routes"] = worst
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
    out = args.out or os.path.join(ROOT, "profiles", "density", f"density_n{args.n}.json")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
