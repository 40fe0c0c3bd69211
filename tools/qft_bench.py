"""Times the quantum Fourier transform (qsim_apply_qft) against what the bytes say and against the textbook circuit through the gate
queue, and writes ONE JSON file.

  python tools/qft_bench.py [--n 30] [--reps 7] [--out profiles/qft/qft_n30.json]

The state is the bench's random circuit (bench.py's seed) at n qubits.  Every row is timed with HIP events on the state's stream
around the call (which does not wait), warm, median of --reps (>= 5), with the fastest and the slowest repetition beside it.  Rows,
per precision (64, 32):
  qft_k10_low | _spread | _top     ten qubits: 0..9, evenly spaced from qubit 1, the top ten — one sweep
  qft_k20_low | _high              qubits 0..19 and 10..29 — three sweeps at the plan's own cap (7 + 7 + 6)
  qft_k<n>                         the whole register — four sweeps at n = 30 (8 + 8 + 7 + 7)
  qft_..._cap10 | _cap6            the same registers under a digit cap of 10 (a sweep fewer: 10 + 10, 10 + 10 + 10) and of 6 (a sweep more)
Two yardsticks beside every qft row, taken in the same process:
  rot      ONE Pauli rotation on the same qubits (X Z X ... ): the sweep that reads and writes the same bytes once; x_rot = the row's
           time / (passes * this)
  circuit  the textbook circuit (h, controlled phases as 2-qubit gates, swaps as three cx) through run() with its plan cached;
           circuit_launches = the kernel launches of one run; x_circuit = the row's time / this
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


def textbook_circuit(n, qubits):
    import numpy as np
    from gpu_quantum_simulator_amd import Circuit
    h = np.array([[1, 1], [1, -1]], dtype=np.complex128) / np.sqrt(2.0)
    c = Circuit.empty(n)
    k = len(qubits)
    for j in range(k - 1, -1, -1):
        c.append_1q(h, qubits[j])
        for m in range(j - 1, -1, -1):
            cp = np.diag([1, 1, 1, np.exp(1j * np.pi / (1 << (j - m)))]).astype(np.complex128)
            c.append_2q(cp, max(qubits[j], qubits[m]), min(qubits[j], qubits[m]))
    for j in range(k // 2):
        a, b = qubits[j], qubits[k - 1 - j]
        c.append_cx(a, b), c.append_cx(b, a), c.append_cx(a, b)
    return c


def registers(n):
    top = n - 10
    return {"k10_low": list(range(10)), "k10_spread": [1 + (j * (n - 2)) // 9 for j in range(10)], "k10_top": list(range(top, n)),
            "k20_low": list(range(20)), "k20_high": list(range(n - 20, n)), f"k{n}": list(range(n))}


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
    c = Circuit.from_gates(n, circuits.random_gates(n, 1000, 20240117 + n, "all"))
    with Simulator(n, precision=args.precision) as sim:
        sim.run(c)
        sim.sync()
        stream = ctypes.c_void_p(sim.stream)

        def timed(name, fn):
            fn()  # warm: the second buffer is allocated, the circuit's plan is cached
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

        def qft_row(name, qs, cap, rot, circ):
            before = plans.sweeps_launched("qft")
            row = timed(name, lambda: sim.apply_qft(qs, max_digit_bits=cap))
            row["qubits"], row["cap"] = qs, cap
            row["passes"] = int(plans.sweeps_launched("qft") - before) // (max(5, args.reps) + 1)
            row["x_rot"] = round(row["ms"] / (row["passes"] * rot["ms"]), 3)
            row["x_circuit"] = round(row["ms"] / circ["ms"], 3)
            return row

        for rname, qs in registers(n).items():
            if rname.startswith("k20") and n < 20:
                continue
            text = " ".join(("X" if j % 2 == 0 else "Z") + str(q) for j, q in enumerate(qs))
            rot = timed(f"rot_{rname}", lambda: sim.apply_pauli_rotation(0.37, text))
            circuit = textbook_circuit(n, qs)
            sim.run(circuit)
            sim.sync()
            launches = sim.stats()["launches"]
            circ = timed(f"circuit_{rname}", lambda: sim.run(circuit) or sim.flush())
            circ["gates"] = len(circuit)
            circ["launches"] = (sim.stats()["launches"] - launches) // (max(5, args.reps) + 1)
            circ["host_passes_dense"] = len(circuit.passes(initial_support=(1 << n) - 1))
            qft_row(f"qft_{rname}", qs, 0, rot, circ)
            if len(qs) >= 20:
                for cap in (10, 6):
                    qft_row(f"qft_{rname}_cap{cap}", qs, cap, rot, circ)
        rows["norm2_after"] = sim.norm2()  # unitary sweeps throughout: the state's norm after all of them
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
    out = args.out or os.path.join(ROOT, "profiles", "qft", f"qft_n{args.n}.json")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result)[:6000])


if __name__ == "__main__":
    main()
