"""Times controlled Pauli-rotation sweeps (qsim_apply_controlled_pauli_rotations, k_pauli_crot) against the uncontrolled sweep of
the same x on the same state, in the same process, and prints ONE JSON line.

  python tools/controlled_rot_bench.py [--n 30] [--reps 7]

The state is a layer of H and rz gates at n qubits (a sweep's time does not depend on the amplitudes).  Every row is timed with HIP
events on the state's stream, warm, median of --reps (>= 5): ms, the units the plan reports (plans.controlled_rotation_plan) and
`share` = ms / ms of the uncontrolled sweep — the traffic model of DESIGN "Controlled Pauli rotations" says 2^-c for c controls.
Rows, per precision (64, 32), all with the one string "X3 Z5 X9" (x = qubits 3 and 9, a paired sweep):
  uncontrolled           the yardstick: the sweep without controls (k_pauli_rot)
  high_<c>               c = 1, 2, 4 controls on the highest qubits
  low_0, low_7           one control on qubit 0 (fp32: the odd slot of every unit) and on qubit 7 (the top lane bit of a unit index)
  mcx_<c>                Simulator.apply_mcx with c = 2 and 4 controls on the highest qubits, target qubit 3: two sweeps
Each precision runs in a child process of its own under its own `timeout -k 10`; the first failure ends the run."""
import argparse
import ctypes
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
STRING_X, STRING_Z = 1 << 3 | 1 << 9, 1 << 5
TEXT = "X3 Z5 X9"


def child(args):
    from gpu_quantum_simulator_amd import Circuit, Simulator, _lib, plans
    n = args.n
    assert n >= 16
    _lib.load()  # libqsim (and torch's HIP runtime, where there is one) before anything else opens the device
    hip = ctypes.CDLL("libamdhip64.so.7")  # the runtime libqsim.so itself is linked against
    ev = [ctypes.c_void_p(), ctypes.c_void_p()]
    for e in ev:
        assert hip.hipEventCreate(ctypes.byref(e)) == 0
    rows = {}

    def units(controls):
        p = plans.ok(plans.controlled_rotation_plan([sum(1 << q for q in controls)], [STRING_X], [STRING_Z], n, args.precision))
        assert (p["sweeps"], p["queued_as_gates"]) == (1, 0)
        return p["units_visited"]

    with Simulator(n, precision=args.precision) as sim:
        sim.run(Circuit.from_gates(n, [("h", q) for q in range(n)] + [("rz", 0.1 + 0.05 * q, q) for q in range(n)]))
        sim.sync()
        stream = ctypes.c_void_p(sim.stream)

        def timed(name, fn, sweeps, extra):
            before = plans.sweeps_launched("pauli_rotation")
            fn()  # warm
            assert plans.sweeps_launched("pauli_rotation") - before == sweeps
            ms = []
            for _ in range(max(5, args.reps)):
                assert hip.hipEventRecord(ev[0], stream) == 0
                fn()
                assert hip.hipEventRecord(ev[1], stream) == 0
                assert hip.hipEventSynchronize(ev[1]) == 0
                t = ctypes.c_float()
                assert hip.hipEventElapsedTime(ctypes.byref(t), ev[0], ev[1]) == 0
                ms.append(t.value)
            rows[name] = dict({"ms": round(statistics.median(ms), 4)}, **extra)
            if "uncontrolled" in rows:
                rows[name]["share"] = round(rows[name]["ms"] / rows["uncontrolled"]["ms"], 4)

        def sweep(name, controls):
            timed(name, lambda: sim.apply_pauli_rotation(0.3, TEXT, controls), 1, {"controls": list(controls), "units": units(controls)})

        sweep("uncontrolled", ())
        for c in (1, 2, 4):
            sweep(f"high_{c}", tuple(range(n - c, n)))
        sweep("low_0", (0,))
        sweep("low_7", (7,))
        for c in (2, 4):
            controls = tuple(range(n - c, n))
            timed(f"mcx_{c}", lambda: sim.apply_mcx(controls, 3), 2, {"controls": list(controls)})
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
    result = {"n": args.n, "reps": max(5, args.reps), "string": TEXT}
    for precision in (64, 32):
        cmd = ["timeout", "-k", "10", "300", sys.executable, os.path.abspath(__file__), "--child", "--n", str(args.n), "--reps", str(args.reps),
               "--precision", str(precision)]
        p = subprocess.run(cmd, capture_output=True, text=True)
        lines = [ln for ln in p.stdout.splitlines() if ln.startswith("ROWS ")]
        if p.returncode != 0 or not lines:  # nothing more is started on the GPU after a failure
            sys.stderr.write(p.stdout[-2000:] + p.stderr[-2000:])
            sys.exit(p.returncode or 1)
        result[f"fp{precision}"] = json.loads(lines[-1][5:])
    print(json.dumps(result))


if __name__ == "__main__":
    main()
