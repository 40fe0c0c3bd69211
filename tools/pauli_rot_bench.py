"""Times the Pauli-rotation sweeps (qsim_apply_pauli_rotations) against one dense single-qubit pass on the same state, in the
same process, and prints ONE JSON line.

  python tools/pauli_rot_bench.py [--n 30] [--reps 7]

The state is a layer of H and rz gates at n qubits (the sweeps' time does not depend on the amplitudes).  Every row is timed with
HIP events on the state's stream, warm, median of --reps (>= 5): ms and TB/s = 2 * bytes of the state / time (one read and one
write).  Rows, per precision (64, 32); the sweep rows once per grid policy ("resident": as many workgroups as are resident at
once, the default; "blocks": one workgroup per block of units, QSIM_OPT_GRID_CAP = 2^30):
  gate1_hi               the yardstick: one dense 2x2 on the top qubit at fusion level 0 (k_gate1_hi), same bytes as a paired sweep
  diag_<G>               G all-Z terms in one sweep, G in 1, 8, 32
  pair_low_<G>           G terms sharing an x confined to low bits (qubits 1 and 3: the partner lines are permuted inside a wave)
  pair_high_<G>          G terms sharing an x that reaches the top qubit (qubits 3 and n - 1)
  rot_w6                 one weight-6 rotation "X1 Y4 Z9 X15 Y22 Z29" as a sweep
  cx_ladder_w6           the same rotation through the gate queue: basis changes, 2 * 5 cx and an rz (checked against the sweep at
                         n = 10 first, up to the global phase the gate table's rz drops), with the passes it became
  ratio_pair_1_vs_gate1  max(pair_low_1, pair_high_1) / gate1_hi: the figure DESIGN "Pauli rotations" holds against 1.15
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
GROUPS = (1, 8, 32)
POLICIES = {"resident": 0, "blocks": 1 << 30}
W6 = "X1 Y4 Z9 X15 Y22 Z29"


def ladder_gates(text, theta):
    """exp(-i theta/2 P) for the string `text` as the gate list a caller wrote by hand: basis changes, a cx ladder onto the last
    qubit, rz(theta) there, and back.  Equal to the rotation up to the global phase e^(-i theta/2) the table's rz drops."""
    factors = [(tok[0], int(tok[1:])) for tok in text.split()]
    pre, post = [], []
    for letter, q in factors:
        if letter == "X":
            pre.append(("h", q)), post.append(("h", q))
        elif letter == "Y":
            pre += [("sdg", q), ("h", q)]
            post += [("h", q), ("s", q)]
    qs = [q for _, q in factors]
    ladder = [("cx", a, b) for a, b in zip(qs, qs[1:])]
    return pre + ladder + [("rz", theta, qs[-1])] + ladder[::-1] + post


def check_ladder():
    import cmath
    import numpy as np
    from gpu_quantum_simulator_amd import Circuit, Simulator
    n, theta, text = 10, 0.77, "X1 Y4 Z5 X6 Y8 Z9"
    rng = np.random.default_rng(1)
    start = rng.standard_normal(1 << n) + 1j * rng.standard_normal(1 << n)
    start /= np.linalg.norm(start)
    with Simulator(n) as a, Simulator(n) as b:
        a.write(start), b.write(start)
        a.apply_pauli_rotation(theta, text)
        b.run(Circuit.from_gates(n, ladder_gates(text, theta)))
        diff = float(np.max(np.abs(a.read() - cmath.exp(-0.5j * theta) * b.read())))
    assert diff < 1e-10, diff
    return diff


def child(args):
    import numpy as np
    from gpu_quantum_simulator_amd import Circuit, Simulator, _lib, gate_matrix, plans
    n = args.n
    _lib.load()  # libqsim (and torch's HIP runtime, where there is one) before anything else opens the device
    hip = ctypes.CDLL("libamdhip64.so.7")  # the runtime libqsim.so itself is linked against
    ev = [ctypes.c_void_p(), ctypes.c_void_p()]
    for e in ev:
        assert hip.hipEventCreate(ctypes.byref(e)) == 0
    rows = {"ladder_check_max_abs_diff": check_ladder()}
    with Simulator(n, precision=args.precision) as sim:
        sim.run(Circuit.from_gates(n, [("h", q) for q in range(n)] + [("rz", 0.1 + 0.05 * q, q) for q in range(n)]))
        sim.sync()
        stream = ctypes.c_void_p(sim.stream)
        state_bytes = (16 if args.precision == 64 else 8) * (1 << n)

        def timed(name, fn, extra=None):
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
            med = statistics.median(ms)
            rows[name] = dict({"ms": round(med, 4), "TBps": round(2 * state_bytes / med / 1e9, 3)}, **(extra or {}))

        rng = np.random.default_rng(5)
        zs = [int(z) for z in rng.integers(1, 1 << n, size=32)]

        def text(x, z):
            return " ".join("IXZY"[(x >> q & 1) | 2 * (z >> q & 1)] + str(q) for q in range(n) if (x | z) >> q & 1)

        def sweep(x, G):
            rots = [(0.3 + 0.01 * k, text(x, zs[k])) for k in range(G)]
            before = plans.sweeps_launched("pauli_rotation")
            sim.apply_pauli_rotations(rots)
            assert plans.sweeps_launched("pauli_rotation") - before == 1
            return lambda: sim.apply_pauli_rotations(rots)

        # the yardstick: one launch per gate at fusion level 0, target bit >= 6
        sim.set_option(_lib.OPT_FUSE, 0)
        H = gate_matrix("h")

        def gate1():
            sim.apply_1q(H, n - 1)
            sim.flush()

        sim.reset_stats()
        timed("gate1_hi", gate1)
        st = sim.stats()["kernels"]
        assert st["gate1"]["launches"] == 1 + max(5, args.reps) and st["tile"]["launches"] == 0, st
        sim.set_option(_lib.OPT_FUSE, 3)
        ladder = Circuit.from_gates(n, ladder_gates(W6, 0.77))

        def run_ladder():
            sim.run(ladder)
            sim.flush()

        sim.reset_stats()
        run_ladder()
        launches = {k: v["launches"] for k, v in sim.stats()["kernels"].items() if v["launches"]}
        timed("cx_ladder_w6", run_ladder, {"gates": len(ladder), "launches": launches})
        common, out = rows, {}
        for policy, cap in POLICIES.items():
            sim.set_option(_lib.OPT_GRID_CAP, cap)
            rows = out[policy] = {}
            for G in GROUPS:
                timed(f"diag_{G}", sweep(0, G))
                timed(f"pair_low_{G}", sweep(0b1010, G))
                timed(f"pair_high_{G}", sweep(1 << (n - 1) | 1 << 3, G))
            timed("rot_w6", lambda: sim.apply_pauli_rotation(0.77, W6))
            rows["ratio_pair_1_vs_gate1"] = round(max(rows["pair_low_1"]["ms"], rows["pair_high_1"]["ms"]) / common["gate1_hi"]["ms"], 4)
            rows["ladder_over_sweep"] = round(common["cx_ladder_w6"]["ms"] / rows["rot_w6"]["ms"], 3)
        sim.set_option(_lib.OPT_GRID_CAP, 0)
        rows = dict(common, **out)
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
    result = {"n": args.n, "reps": max(5, args.reps)}
    for precision in (64, 32):
        cmd = ["timeout", "-k", "10", "400", sys.executable, os.path.abspath(__file__), "--child", "--n", str(args.n), "--reps", str(args.reps),
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
