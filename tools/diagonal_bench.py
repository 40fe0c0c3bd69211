"""Times whole-register diagonal operators from a table (Diagonal, apply_diagonal_phase, expectation_diagonal) against the sweeps a
caller had before and writes ONE JSON file.

  python tools/diagonal_bench.py [--n 30] [--reps 7] [--out profiles/diagonal/diagonal_n30.json]

The state is |+>^n, where a QAOA run starts.  Both precisions run one after the other in ONE child process under `timeout -k 10` (the
parent never opens the GPU).  Every row is the WHOLE call on the host clock — the call and, where it does not wait itself, the
synchronisation of the state's stream behind it — warm, median of --reps (>= 5), with the fastest and the slowest repetition.
Rows per precision (fp64, fp32), chain = the 29-term ZZ chain (n - 1 terms), pairs = ZZ on all pairs (435 terms at n = 30):
  add_terms_chain, add_terms_pairs   Diagonal.add_terms on an existing table
  phase                              apply_diagonal_phase with the table of `pairs`
  rot_z0                             (a) ONE diagonal rotation apply_pauli_rotation(theta, "Z0"): the sweep that reads and writes the state
  rot_pairs                          (b) apply_pauli_rotations over the terms of `pairs`: what the same separator cost before
  expect                             expectation_diagonal(moments=True)
  norm2                              the state's squared norm: the read-only sweep of the state alone
  expect_pairs                       expectation over the terms of `pairs`: what the same <C> cost before
  extrema                            Diagonal.extrema
and the ratios against the byte model: an fp64 amplitude of the phase sweep moves 40 B against 32 B of rot_z0 and one of
the expectation sweep 24 B against 16 B of norm2; fp32: 24 B against 16 B and 16 B against 8 B.  x_model = measured ratio / that
ratio; `met` = x_model <= 1.15."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)

MODEL = {64: {"phase": 40.0 / 32.0, "expect": 24.0 / 16.0}, 32: {"phase": 24.0 / 16.0, "expect": 16.0 / 8.0}}
ALLOWED = 1.15


def chain_terms(n):
    return [(1.0, f"Z{q} Z{q + 1}") for q in range(n - 1)]


def pair_terms(n):
    return [(1.0, f"Z{a} Z{b}") for a in range(n) for b in range(a + 1, n)]


def child(args):
    from gpu_quantum_simulator_amd import Circuit, Diagonal, Simulator
    n, gamma = args.n, 0.37
    chain, pairs = chain_terms(n), pair_terms(n)
    result = {}
    for precision in (64, 32):
        rows = {}
        with Simulator(n, precision=precision) as sim, Diagonal.from_terms(n, pairs) as diag, Diagonal(n) as scratch:
            sim.run(Circuit.from_gates(n, [("h", q) for q in range(n)]))
            sim.sync()

            def timed(name, fn):
                fn()  # warm
                sim.sync()
                ms = []
                for _ in range(max(5, args.reps)):
                    t0 = time.perf_counter()
                    fn()
                    sim.sync()
                    ms.append((time.perf_counter() - t0) * 1e3)
                rows[name] = {"ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4)}
                return rows[name]

            timed("add_terms_chain", lambda: scratch.add_terms(chain))["terms"] = len(chain)
            timed("add_terms_pairs", lambda: scratch.add_terms(pairs))["terms"] = len(pairs)
            rot = timed("rot_z0", lambda: sim.apply_pauli_rotation(gamma, "Z0"))
            phase = timed("phase", lambda: sim.apply_diagonal_phase(diag, gamma))
            rot_pairs = timed("rot_pairs", lambda: sim.apply_pauli_rotations([(2.0 * gamma * c, p) for c, p in pairs]))
            norm2 = timed("norm2", sim.norm2)
            expect = timed("expect", lambda: sim.expectation_diagonal(diag, moments=True))
            expect_pairs = timed("expect_pairs", lambda: sim.expectation(pairs))
            timed("extrema", diag.extrema)
            for row, base, old, key in ((phase, rot, rot_pairs, "phase"), (expect, norm2, expect_pairs, "expect")):
                row["x_base"] = round(row["ms"] / base["ms"], 3)
                row["x_model"] = round(row["ms"] / base["ms"] / MODEL[precision][key], 3)
                row["met"] = bool(row["ms"] / base["ms"] / MODEL[precision][key] <= ALLOWED)
                row["x_terms"] = round(row["ms"] / old["ms"], 4)  # against the sweeps over the 435 terms
            rows["values"] = {"expect": sim.expectation_diagonal(diag, moments=True), "expect_pairs": sim.expectation(pairs),
                              "extrema": diag.extrema(), "norm2_after": sim.norm2()}
        result[f"fp{precision}"] = rows
    print("ROWS " + json.dumps(result), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=30)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", action="store_true")
    args = ap.parse_args()
    if args.child:
        return child(args)
    cmd = ["timeout", "-k", "10", "540", sys.executable, os.path.abspath(__file__), "--child", "--n", str(args.n), "--reps", str(args.reps)]
    p = subprocess.run(cmd, capture_output=True, text=True)
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("ROWS ")]
    if p.returncode != 0 or not lines:
        sys.stderr.write(p.stdout[-2000:] + p.stderr[-2000:])
        sys.exit(p.returncode or 1)
    result = {"n": args.n, "reps": max(5, args.reps), "timing": "whole call on the host clock, state's stream synchronised", "allowed_x_model": ALLOWED}
    result.update(json.loads(lines[-1][5:]))
    out = args.out or os.path.join(ROOT, "profiles", "diagonal", f"diagonal_n{args.n}.json")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result)[:4000])


if __name__ == "__main__":
    main()
