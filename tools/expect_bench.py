"""Times the Pauli expectation sweeps (qsim_expect_paulis) against qsim_norm2 on one state and prints ONE JSON line.

  python tools/expect_bench.py [--n 30] [--reps 7] [--host-row]

The state is the bench's random circuit (bench.py's seed) at n qubits.  Every row is timed with HIP events on the state's stream,
warm, median of --reps (>= 5): ms and TB/s = bytes of the state / time.  Rows, per precision (64, 32):
  norm2                  the parent's yardstick: one read of the state, nothing written
  diag_1                 one diagonal term
  pair_high / pair_bit0 / pair_5bit   one paired term: x on the top qubit, on qubit 0, on five qubits across lane and high bits
  group_<G>_k<K>         G terms that share one x (a paired x) in a library whose terms-per-sweep is K, for G, K in 8, 16, 32
  diag_group_<G>_k<K>    the same for a diagonal group
  ising / heisenberg     1-D transverse-field Ising (n ZZ + n X) and a Heisenberg chain (3 (n - 1) terms), default K
  host_ising (--host-row, fp64) wall clock of what a caller did before: sim.read() and numpy over the amplitudes, once
K is fixed when the library loads (QSIM_PAULI_TERMS_PER_SWEEP), so every (precision, K) runs in a child process of its own,
each under its own `timeout -k 10`; the first failure ends the run."""
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
CANDIDATES = (8, 16, 32)


def ising_terms(n):
    return [f"Z{q} Z{(q + 1) % n}" for q in range(n)] + [f"X{q}" for q in range(n)]


def heisenberg_terms(n):
    return [f"{p}{q} {p}{q + 1}" for q in range(n - 1) for p in "XYZ"]


def host_ising(psi, n):
    """The Ising terms from the amplitudes on the host, by reshapes (no index arrays): what a caller did before."""
    import numpy as np
    p = psi.real ** 2 + psi.imag ** 2
    out = []
    for q in range(n):
        r = (q + 1) % n
        lo, hi = min(q, r), max(q, r)
        v = p.reshape(1 << (n - hi - 1), 2, 1 << (hi - lo - 1), 2, 1 << lo).sum(axis=(0, 2, 4))
        out.append(float(v[0, 0] + v[1, 1] - v[0, 1] - v[1, 0]))
    for q in range(n):
        v = psi.reshape(1 << (n - q - 1), 2, 1 << q)
        out.append(float(2.0 * np.vdot(v[:, 1, :], v[:, 0, :]).real))
    return out


def child(args):
    import numpy as np
    from gpu_quantum_simulator_amd import Circuit, Simulator, circuits, _lib, plans
    n, K = args.n, args.k
    _lib.load()  # libqsim (and torch's HIP runtime, where there is one) before anything else opens the device
    assert plans.pauli_terms_per_sweep() == K
    hip = ctypes.CDLL("libamdhip64.so.7")  # the runtime libqsim.so itself is linked against
    ev = [ctypes.c_void_p(), ctypes.c_void_p()]
    for e in ev:
        assert hip.hipEventCreate(ctypes.byref(e)) == 0
    rows = {}
    c = Circuit.from_gates(n, circuits.random_gates(n, 1000, 20240117 + n, "all"))
    with Simulator(n, precision=args.precision) as sim:
        sim.run(c)
        sim.sync()
        stream = ctypes.c_void_p(sim.stream)
        state_bytes = (16 if args.precision == 64 else 8) * (1 << n)

        def timed(name, fn, sweeps=1):
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
            rows[name] = {"ms": round(med, 4), "TBps": round(sweeps * state_bytes / med / 1e9, 3), "sweeps": sweeps}

        rng = np.random.default_rng(5)
        zs = [int(z) for z in rng.integers(1, 1 << n, size=32)]
        x_pair = (1 << (n - 1)) | (1 << 3)

        def text(x, z):
            return " ".join("IXZY"[(x >> q & 1) | 2 * (z >> q & 1)] + str(q) for q in range(n) if (x | z) >> q & 1)

        if K == args.default_k:
            timed("norm2", sim.norm2)
            timed("diag_1", lambda: sim.expectation_terms([text(0, zs[0])]))
            timed("pair_high", lambda: sim.expectation_terms([f"X{n - 1}"]))
            timed("pair_bit0", lambda: sim.expectation_terms(["X0"]))
            timed("pair_5bit", lambda: sim.expectation_terms([f"X1 Y4 X9 Y{n // 2} X{n - 2}"]))
            for name, terms in (("ising", ising_terms(n)), ("heisenberg", heisenberg_terms(n))):
                from gpu_quantum_simulator_amd import pauli_masks
                sweeps = plans.ok(plans.pauli_sweeps([pauli_masks(t, n)[0] for t in terms]))["sweeps"]
                timed(name, lambda terms=terms: sim.expectation_terms(terms), sweeps)
                rows[name]["terms"] = len(terms)
        for G in CANDIDATES:
            timed(f"group_{G}_k{K}", lambda: sim.expectation_terms([text(x_pair, z) for z in zs[:G]]), -(-G // K))
            timed(f"diag_group_{G}_k{K}", lambda: sim.expectation_terms([text(0, z) for z in zs[:G]]), -(-G // K))
        if args.host_row and args.precision == 64 and K == args.default_k:
            terms = ising_terms(n)
            device = sim.expectation_terms(terms)
            t0 = time.time()
            host = host_ising(sim.read(), n)
            rows["host_ising"] = {"seconds": round(time.time() - t0, 2), "terms": len(terms),
                                  "max_abs_diff_vs_device": float(np.max(np.abs(np.array(host) - device)))}
    print("ROWS " + json.dumps(rows), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=30)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--host-row", action="store_true")
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--k", type=int, default=0)
    ap.add_argument("--default-k", type=int, default=0)
    ap.add_argument("--precision", type=int, default=64)
    args = ap.parse_args()
    if args.child:
        return child(args)
    # the parent never opens the GPU: it reads the library's default K through a child too
    env = {k: v for k, v in os.environ.items() if k != "QSIM_PAULI_TERMS_PER_SWEEP"}
    probe = "import sys; sys.path.insert(0, %r); from gpu_quantum_simulator_amd import plans; print(plans.pauli_terms_per_sweep())" % ROOT
    default_k = int(subprocess.run([sys.executable, "-c", probe], env=env, check=True, capture_output=True, text=True).stdout.split()[-1])
    result = {"n": args.n, "reps": max(5, args.reps), "terms_per_sweep": default_k, "fp64": {}, "fp32": {}}
    for precision in (64, 32):
        for K in CANDIDATES:
            cmd = ["timeout", "-k", "10", "900" if args.host_row else "240", sys.executable, os.path.abspath(__file__), "--child", "--n", str(args.n),
                   "--reps", str(args.reps), "--k", str(K), "--default-k", str(default_k), "--precision", str(precision)]
            if args.host_row:
                cmd.append("--host-row")
            p = subprocess.run(cmd, env=dict(env, QSIM_PAULI_TERMS_PER_SWEEP=str(K)), capture_output=True, text=True)
            lines = [ln for ln in p.stdout.splitlines() if ln.startswith("ROWS ")]
            if p.returncode != 0 or not lines:  # nothing more is started on the GPU after a failure
                sys.stderr.write(p.stdout[-2000:] + p.stderr[-2000:])
                sys.exit(p.returncode or 1)
            result[f"fp{precision}"].update(json.loads(lines[-1][5:]))
    print(json.dumps(result))


if __name__ == "__main__":
    main()
