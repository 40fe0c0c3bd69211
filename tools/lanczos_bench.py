"""Times the state-combination kernel (qsim_combine, csrc/combine.hip), the inner product and one Lanczos step
(qsim_lanczos_ground, csrc/lanczos.cpp) against the existing sweeps in the same process, and writes ONE JSON line (also to
profiles/lanczos/lanczos_n<n>.json).

  python tools/lanczos_bench.py [--n 30] [--reps 7]

fp64; at n = 30 the run needs 64 GiB (three states in the first half, one state and the call's three work buffers in the second).
The states are a layer of H and rz gates (a sweep's time does not depend on the amplitudes).  Every row is the median of --reps
(>= 5) warm repetitions of a call that ends in a stream synchronise, timed with the host clock; `volumes` is the state volumes the
row reads and writes, `gbps` = volumes * state bytes / ms.
  combine_three / _two / _d0_two / _d0_one   dst <- d dst + a p + b q with its norm: 4, 3, 3 (dst not read) and 2 (the scaled copy) volumes
  inner, norm2                               <p|q> (2 volumes) and qsim_norm2 (1)
  sum_store                                  qsim_pauli_sum_into for one term: the storing k_pauli_sum sweep (2)
  sum_store_zz_chain                         the same for the n - 1 terms of sum Z_q Z_(q+1): one storing sweep of n - 1 terms (2)
  sum_accumulate                             the same for two terms of different x minus sum_store: ONE accumulating sweep (3); a
                                             difference of medians, the C ABI launches no accumulating sweep alone
  step_ising, step_zz                        one Lanczos step for the transverse-field Ising chain (2n - 1 terms, G = n + 1 sweeps) and for
                                             H = sum Z_q Z_(q+1) alone (G = 1): (call of 4 steps - call of 2 steps) / 2, vector=False, tol = 0 —
                                             steps 2 and 3, which have all three vectors; allocation and the start norm cancel.  `volumes`
                                             is plans.lanczos_plan's; model_ms_sum / model_ms_norm2 = those volumes at the rate of
                                             sum_accumulate / norm2, ratio_* = ms / model
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


def child(args):
    from gpu_quantum_simulator_amd import Circuit, Simulator, pauli_masks, _lib, plans
    n = args.n
    _lib.load()  # libqsim (and torch's HIP runtime, where there is one) before anything else opens the device
    reps = max(5, args.reps)
    state_bytes = float(16 << n)
    rows = {}
    prep = Circuit.from_gates(n, [("h", q) for q in range(n)] + [("rz", 0.1 + 0.05 * q, q) for q in range(n)])

    def timed(name, fn, volumes):
        fn()  # warm
        ms = []
        for _ in range(reps):
            t0 = time.perf_counter()
            fn()
            ms.append(1e3 * (time.perf_counter() - t0))
        med = statistics.median(ms)
        rows[name] = {"ms": round(med, 4), "volumes": volumes, "gbps": round(volumes * state_bytes / med / 1e6, 1)}
        return med

    d, a, b = 0.6 - 0.3j, 0.5 + 0.2j, -0.4 + 0.1j
    with Simulator(n) as dst:
        with Simulator(n) as p, Simulator(n) as q:
            for s in (dst, p, q):
                s.run(prep)
                s.sync()
            timed("combine_three", lambda: dst.combine(d, (a, p), (b, q), norm=True), 4)
            timed("combine_two", lambda: dst.combine(d, (a, p), norm=True), 3)
            timed("combine_d0_two", lambda: dst.combine(0, (a, p), (b, q), norm=True), 3)
            timed("combine_d0_one", lambda: dst.combine(0, (a, p), norm=True), 2)
            timed("inner", lambda: p.inner(q), 2)
            timed("norm2", lambda: p.norm2(), 1)
            out = q.device_ptr
            q.sync()

            def sum_into(terms):
                p.pauli_sum_into(terms, out)
                p.sync()

            one = timed("sum_store", lambda: sum_into([(0.7, f"X3 Z{n - 1}")]), 2)
            two = timed("sum_two_groups", lambda: sum_into([(0.7, f"X3 Z{n - 1}"), (-0.4, f"X{n - 2} Y5")]), 5)
            timed("sum_store_zz_chain", lambda: sum_into([(-1.0, f"Z{k} Z{k + 1}") for k in range(n - 1)]), 2)
            acc = two - one
            rows["sum_accumulate"] = {"ms": round(acc, 4), "volumes": 3, "gbps": round(3 * state_bytes / acc / 1e6, 1), "how": "sum_two_groups - sum_store"}
        # p and q are gone: the state and the call's three work buffers
        dst.run(prep)
        dst.sync()
        for name, terms in (("step_ising", [(-1.0, f"Z{k} Z{k + 1}") for k in range(n - 1)] + [(-0.5, f"X{k}") for k in range(n)]),
                            ("step_zz", [(-1.0, f"Z{k} Z{k + 1}") for k in range(n - 1)])):
            short = timed(name + "_2_steps", lambda: dst.ground_state(terms, 0.0, max_steps=2, vector=False), 0)
            long = timed(name + "_4_steps", lambda: dst.ground_state(terms, 0.0, max_steps=4, vector=False), 0)
            for k in (name + "_2_steps", name + "_4_steps"):
                del rows[k]["volumes"], rows[k]["gbps"]
            plan = plans.ok(plans.lanczos_plan([pauli_masks(text, n)[0] for _, text in terms], 4, 0))
            sums, others, volumes = plan["sum_sweeps_per_step"], plan["other_sweeps_per_step"], plan["volumes_per_step"]
            step = 0.5 * (long - short)
            model_sum = volumes * state_bytes / (rows["sum_accumulate"]["gbps"] * 1e6)
            model_norm = volumes * state_bytes / (rows["norm2"]["gbps"] * 1e6)
            rows[name] = {"ms": round(step, 4), "how": "(4 steps - 2 steps) / 2", "terms": len(terms), "sum_sweeps": sums, "other_sweeps": others,
                          "volumes": volumes, "gbps": round(volumes * state_bytes / step / 1e6, 1), "model_ms_sum": round(model_sum, 4),
                          "model_ms_norm2": round(model_norm, 4), "ratio_sum": round(step / model_sum, 4), "ratio_norm2": round(step / model_norm, 4)}
    for name in ("combine_three", "combine_two", "combine_d0_two", "combine_d0_one", "inner"):
        rows[name]["rate_vs_sum_accumulate"] = round(rows[name]["gbps"] / rows["sum_accumulate"]["gbps"], 4)
        rows[name]["rate_vs_norm2"] = round(rows[name]["gbps"] / rows["norm2"]["gbps"], 4)
    print("ROWS " + json.dumps(rows), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=30)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--child", action="store_true")
    args = ap.parse_args()
    if args.child:
        return child(args)
    cmd = ["timeout", "-k", "10", "540", sys.executable, os.path.abspath(__file__), "--child", "--n", str(args.n), "--reps", str(args.reps)]
    p = subprocess.run(cmd, capture_output=True, text=True)
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("ROWS ")]
    if p.returncode != 0 or not lines:  # nothing more is started on the GPU after a failure
        sys.stderr.write(p.stdout[-2000:] + p.stderr[-2000:])
        sys.exit(p.returncode or 1)
    result = {"n": args.n, "reps": max(5, args.reps), "precision": 64, "fp64": json.loads(lines[-1][5:])}
    line = json.dumps(result)
    out_dir = os.path.join(ROOT, "profiles", "lanczos")
    os.makedirs(out_dir, exist_ok=True)
    with open(os.path.join(out_dir, f"lanczos_n{args.n}.json"), "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
