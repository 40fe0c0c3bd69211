"""Times the backward sweep of an adjoint gradient through controlled Pauli rotations (qsim_controlled_pauli_gradient,
k_pauli_cadjoint) against the uncontrolled backward sweep of the same terms (k_pauli_adjoint) on the same state, in the same process,
and writes ONE JSON line (also to profiles/gradient/controlled_gradient_n<n>.json).

  python tools/controlled_gradient_bench.py [--n 30] [--reps 7]

The state is a layer of H and rz gates at n qubits (a sweep's time does not depend on the amplitudes).  Every figure is the median of
--reps (>= 5) warm repetitions of a call that ends in a stream synchronise, timed with the host clock.  G = 8 rotations of the one
string "X3 Z5 X9" (one x, one control set: ONE fused backward sweep) and a one-term H.  As in tools/gradient_bench.py the backward
sweep is a difference of whole calls — the C ABI has no entry that launches one alone:
  call_0                 the call without rotations: lambda = H psi and the energy sweep
  per row:  call         the whole call;  forward: the G rotations alone (apply_pauli_rotations + sync), one sweep
            backward     call - call_0 - forward
            units        what plans.controlled_gradient_plan reports for the backward sweep
            share        backward / backward of `uncontrolled`; the traffic model of DESIGN "Adjoint gradients under controls" says 2^-c
Rows, per precision (64, 32):
  uncontrolled           the yardstick (k_pauli_adjoint)
  high_<c>               c = 1, 2, 4 controls on the highest qubits
  low_0                  one control on qubit 0 (fp32: the odd slot of every unit; fp64: every other amplitude of a line)
Each precision runs in a child process of its own under its own `timeout -k 10`; the first failure ends the run."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
STRING_X = 1 << 3 | 1 << 9
TEXT = "X3 Z5 X9"
G = 8


def child(args):
    from gpu_quantum_simulator_amd import Circuit, Simulator, _lib, plans
    n = args.n
    assert n >= 16
    _lib.load()  # libqsim (and torch's HIP runtime, where there is one) before anything else opens the device
    reps = max(5, args.reps)
    rows = {}

    def units(controls):
        p = plans.ok(plans.controlled_gradient_plan([sum(1 << q for q in controls)] * G, [STRING_X] * G, [0], n, args.precision))
        assert (p["adjoint_sweeps"], p["sum_sweeps"]) == (1, 1)
        return p["units_visited"]

    with Simulator(n, precision=args.precision) as sim:
        sim.run(Circuit.from_gates(n, [("h", q) for q in range(n)] + [("rz", 0.1 + 0.05 * q, q) for q in range(n)]))
        sim.sync()
        ham = [(1.0, "Z0 Z1")]

        def timed(fn):
            fn()  # warm
            ms = []
            for _ in range(reps):
                t0 = time.perf_counter()
                fn()
                ms.append(1e3 * (time.perf_counter() - t0))
            return statistics.median(ms)

        call_0 = timed(lambda: sim.energy_and_gradient([], ham))
        rows["call_0"] = {"ms": round(call_0, 4)}

        def row(name, controls):
            rots = [(0.3 + 0.01 * k, TEXT, controls) for k in range(G)]
            before = plans.sweeps_launched("pauli_adjoint")
            sim.energy_and_gradient(rots, ham)
            assert plans.sweeps_launched("pauli_adjoint") - before == 1

            def forward():
                sim.apply_pauli_rotations(rots)
                sim.sync()

            call, fwd = timed(lambda: sim.energy_and_gradient(rots, ham)), timed(forward)
            rows[name] = {"controls": list(controls), "units": units(controls), "call_ms": round(call, 4), "forward_ms": round(fwd, 4),
                          "backward_ms": round(call - call_0 - fwd, 4), "model": 2.0 ** -len(controls)}
            rows[name]["share"] = round(rows[name]["backward_ms"] / rows["uncontrolled"]["backward_ms"], 4)

        row("uncontrolled", ())
        for c in (1, 2, 4):
            row(f"high_{c}", tuple(range(n - c, n)))
        row("low_0", (0,))
    print("ROWS " + json.dumps(rows), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=30)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--precision", type=int, default=64)
    args = ap.parse_args()
    if args.child:
        return child(args)
    result = {"n": args.n, "reps": max(5, args.reps), "string": TEXT, "rotations": G, "how": "backward = call - call_0 - forward, medians of host-clock times"}
    for precision in (64, 32):
        cmd = ["timeout", "-k", "10", "300", sys.executable, os.path.abspath(__file__), "--child", "--n", str(args.n), "--reps", str(args.reps),
               "--precision", str(precision)]
        p = subprocess.run(cmd, capture_output=True, text=True)
        lines = [ln for ln in p.stdout.splitlines() if ln.startswith("ROWS ")]
        if p.returncode != 0 or not lines:  # nothing more is started on the GPU after a failure
            sys.stderr.write(p.stdout[-2000:] + p.stderr[-2000:])
            sys.exit(p.returncode or 1)
        result[f"fp{precision}"] = json.loads(lines[-1][5:])
    line = json.dumps(result)
    out_dir = os.path.join(ROOT, "profiles", "gradient")
    os.makedirs(out_dir, exist_ok=True)
    with open(os.path.join(out_dir, f"controlled_gradient_n{args.n}.json"), "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
