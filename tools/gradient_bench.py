"""Times the adjoint-gradient sweeps (qsim_pauli_gradient, csrc/adjoint.hip) against the same work composed from the existing
kernels, in the same process, and writes ONE JSON line (also to profiles/gradient/gradient_n<n>.json).

  python tools/gradient_bench.py [--n 30] [--reps 7]

fp64.  The state is a layer of H and rz gates at n qubits (the sweeps' time does not depend on the amplitudes).  Every row is the
median of --reps (>= 5) warm repetitions of a call that ends in a stream synchronise, timed with the host clock.
  call_<G>      qsim_pauli_gradient for G rotations sharing one x (qubits 3 and n - 1) and a one-term H: forward sweep, lambda = H psi,
                energy sweep, ONE fused backward sweep of G terms
  call_0        the same call without rotations: lambda = H psi and the energy sweep alone
  rot_<G>       the forward sweep alone (apply_pauli_rotations + sync)
  fused_<G>     call_<G> - call_0 - rot_<G>: the fused backward sweep.  A difference of medians, not an event pair: the C ABI has no
                entry that launches a backward sweep alone
  composed_<G>  the yardstick, composed from the existing kernels on TWO states (psi and a stand-in for lambda): one paired
                expectation sweep of G terms on each (together: both buffers read once) and one rotation sweep of G terms on each
                (both read and written once) — 6 state volumes against the fused sweep's 4.  This composition lives here only
  ratio_<G>     fused_<G> / composed_<G>; the traffic model says 4/6
  ising_2_layers  the whole call for a 59-term transverse-field Ising ansatz (n - 1 ZZ rotations and n X rotations per layer, 2
                layers) with the Ising chain as H, and the sweeps it made
The measurement runs in a child process under its own `timeout -k 10`; a failure ends the run."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
GROUPS = (1, 8, 32)


def child(args):
    import numpy as np
    from gpu_quantum_simulator_amd import Circuit, Simulator, _lib, plans
    n = args.n
    _lib.load()  # libqsim (and torch's HIP runtime, where there is one) before anything else opens the device
    reps = max(5, args.reps)
    rows = {}
    prep = Circuit.from_gates(n, [("h", q) for q in range(n)] + [("rz", 0.1 + 0.05 * q, q) for q in range(n)])
    with Simulator(n) as sim, Simulator(n) as twin:
        for s in (sim, twin):
            s.run(prep)
            s.sync()

        def timed(name, fn, extra=None):
            fn()  # warm
            ms = []
            for _ in range(reps):
                t0 = time.perf_counter()
                fn()
                ms.append(1e3 * (time.perf_counter() - t0))
            rows[name] = dict({"ms": round(statistics.median(ms), 4)}, **(extra or {}))
            return rows[name]["ms"]

        rng = np.random.default_rng(5)
        zs = [int(z) for z in rng.integers(1, 1 << n, size=32)]
        x = 1 << (n - 1) | 1 << 3

        def text(xm, zm):
            return " ".join("IXZY"[(xm >> q & 1) | 2 * (zm >> q & 1)] + str(q) for q in range(n) if (xm | zm) >> q & 1)

        ham = [(1.0, "Z0 Z1")]
        timed("call_0", lambda: sim.energy_and_gradient([], ham))
        for G in GROUPS:
            rots = [(0.3 + 0.01 * k, text(x, zs[k])) for k in range(G)]
            strings = [p for _, p in rots]
            before = plans.sweeps_launched("pauli_adjoint")
            sim.energy_and_gradient(rots, ham)
            assert plans.sweeps_launched("pauli_adjoint") - before == 1

            def forward():
                sim.apply_pauli_rotations(rots)
                sim.sync()

            def composed():
                sim.expectation_terms(strings)
                twin.expectation_terms(strings)
                sim.apply_pauli_rotations(rots)
                twin.apply_pauli_rotations(rots)
                sim.sync()
                twin.sync()

            call = timed(f"call_{G}", lambda: sim.energy_and_gradient(rots, ham))
            rot = timed(f"rot_{G}", forward)
            comp = timed(f"composed_{G}", composed)
            fused = call - rows["call_0"]["ms"] - rot
            rows[f"fused_{G}"] = {"ms": round(fused, 4), "how": "call - call_0 - rot"}
            rows[f"ratio_{G}"] = round(fused / comp, 4)
        layers = 2
        ising = [(-1.0, f"Z{q} Z{q + 1}") for q in range(n - 1)] + [(-0.5, f"X{q}") for q in range(n)]
        ansatz = [(0.1 + 0.01 * k, p) for k, (_, p) in enumerate(ising * layers)]
        before = plans.sweeps_launched("pauli_adjoint")
        timed("ising_2_layers", lambda: sim.energy_and_gradient(ansatz, ising), {"parameters": len(ansatz), "hamiltonian_terms": len(ising)})
        rows["ising_2_layers"]["adjoint_sweeps_per_call"] = (plans.sweeps_launched("pauli_adjoint") - before) // (reps + 1)
    print("ROWS " + json.dumps(rows), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=30)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--child", action="store_true")
    args = ap.parse_args()
    if args.child:
        return child(args)
    cmd = ["timeout", "-k", "10", "420", sys.executable, os.path.abspath(__file__), "--child", "--n", str(args.n), "--reps", str(args.reps)]
    p = subprocess.run(cmd, capture_output=True, text=True)
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("ROWS ")]
    if p.returncode != 0 or not lines:  # nothing more is started on the GPU after a failure
        sys.stderr.write(p.stdout[-2000:] + p.stderr[-2000:])
        sys.exit(p.returncode or 1)
    result = {"n": args.n, "reps": max(5, args.reps), "precision": 64, "fp64": json.loads(lines[-1][5:])}
    line = json.dumps(result)
    out_dir = os.path.join(ROOT, "profiles", "gradient")
    os.makedirs(out_dir, exist_ok=True)
    with open(os.path.join(out_dir, f"gradient_n{args.n}.json"), "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
