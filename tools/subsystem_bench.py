"""Times reduced density matrices of 6 to 10 qubits (qsim_subsystem_density) against their floors on one state and writes ONE JSON file.

  python tools/subsystem_bench.py [--n 30] [--reps 7] [--out profiles/density/subsystem_n30.json]

The state is the bench's random circuit (bench.py's seed) at n qubits.  Every row is timed with HIP events on the state's stream,
warm, median of --reps (>= 5), with the fastest and the slowest repetition beside it.  Rows, per precision (64, 32):
  norm2                      one read of the state, nothing written: the memory rate
  mfma_k<k>                  the arithmetic floor: as many v_mfma_f64_16x16x4_f64 per wave, in as many workgroups reserving as much
                             LDS, as the sweep's two kernels of k qubits issue (off the diagonal, then the diagonal blocks), on
                             registers alone (qsim_debug_mfma_f64_probe, undocumented); cycles_per_instruction_per_simd at 2.4 GHz
                             over 1024 SIMDs beside it
  rho_k<k>_<subset>          rho of k = 6..10 qubits, the whole call (scratch allocation, sweep, final sum, 4^k copy, host assembly);
                             subset: low (qubits 0..k-1), high (the top k), spread (evenly spaced, qubit 0 excluded).
                             traffic_ms = the plan's units_read at norm2's rate; x_floor = time / max(traffic_ms, mfma ms)
  pauli_k6_spread            the route a caller had before, k = 6 only: qsim_expect_paulis over all 4096 strings on the subset (64
                             x_mask groups), the expectation values alone, without assembling rho.  x_rho = time / the rho row's time
Each precision runs in a child process of its own under `timeout -k 10`; the first failure ends the run."""
import argparse
import ctypes
import json
import os
import statistics
import subprocess
import sys
from ctypes import byref, c_double, c_int, c_long

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
SWEEP_LDS_BYTES = 2 * 32 * 144 * 8  # the two panels of k_subsystem


def subsets(n, k):
    return {"low": list(range(k)), "high": list(range(n - k, n)), "spread": [1 + (j * (n - 2)) // (k - 1) for j in range(k)]}


def child(args):
    from gpu_quantum_simulator_amd import Circuit, Simulator, _lib, circuits, plans
    n = args.n
    lib = _lib.load()
    hip = ctypes.CDLL("libamdhip64.so.7")  # the runtime libqsim.so itself is linked against
    probe = lib.qsim_debug_mfma_f64_probe
    probe.restype, probe.argtypes = c_int, [c_long, c_int, c_int, ctypes.POINTER(c_double)]
    ev = [ctypes.c_void_p(), ctypes.c_void_p()]
    for e in ev:
        assert hip.hipEventCreate(byref(e)) == 0
    rows = {}

    def plan(qs):
        return plans.ok(plans.subsystem_density_plan(qs, n, args.precision))

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
                assert hip.hipEventElapsedTime(byref(t), ev[0], ev[1]) == 0
                ms.append(t.value)
            rows[name] = {"ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4)}
            return rows[name]

        floor = timed("norm2", sim.norm2)["ms"]
        state_units = (1 << n) >> (1 if args.precision == 32 else 0)
        for k in range(6, 11):
            p = plan(list(range(k)))
            blocks = 1 << (k - 6)
            # per chunk of 32 environments a wave issues 8 steps of 16 products off the diagonal, of 9 in a diagonal block
            launches = [(p["trips_per_workgroup"] * 8 * 16, (p["upper_blocks"] - blocks) * p["slices"], SWEEP_LDS_BYTES),
                        (p["trips_per_workgroup"] * 8 * 9, blocks * p["slices"], SWEEP_LDS_BYTES // 2)]
            ms = []
            for _ in range(3):
                total = 0.0
                for per_wave, groups, lds in launches:
                    if groups:
                        t = c_double()
                        assert probe(per_wave, groups, lds, byref(t)) == 0
                        total += t.value
                ms.append(total)
            mfma = statistics.median(ms)
            count = sum(per_wave * groups * 4 for per_wave, groups, _ in launches)
            rows[f"mfma_k{k}"] = {"ms": round(mfma, 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4), "instructions": count,
                                  "cycles_per_instruction_per_simd": round(mfma * 2.4e6 * 1024 / count, 2)}
            for name, qs in subsets(n, k).items():
                p = plan(qs)
                assert p["path"] == 1
                r = timed(f"rho_k{k}_{name}", lambda: sim.subsystem_density_matrix(qs))
                traffic = p["units_read"] / state_units * floor
                r.update(qubits=qs, plan=p, traffic_ms=round(traffic, 3), mfma_ms=round(mfma, 3), x_floor=round(r["ms"] / max(traffic, mfma), 3))
        qs = subsets(n, 6)["spread"]
        letters = [""]
        for _ in qs:
            letters = [w + l for w in letters for l in "IXYZ"]
        texts = [" ".join(f"{l}{q}" for l, q in zip(w, qs) if l != "I") for w in letters]
        pr = timed("pauli_k6_spread", lambda: sim.expectation_terms(texts))
        pr["strings"], pr["x_rho"] = len(texts), round(pr["ms"] / rows["rho_k6_spread"]["ms"], 2)
        timed("norm2_again", sim.norm2)  # the yardstick's own drift over the run
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
    out = args.out or os.path.join(ROOT, "profiles", "density", f"subsystem_n{args.n}.json")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
