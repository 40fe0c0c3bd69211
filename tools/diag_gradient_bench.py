"""Times adjoint gradients through diagonal phases (qsim_diagonal_gradient; csrc/diagonal.hip's k_diag_adjoint and k_diag_apply) on
the all-pairs MaxCut table and writes ONE JSON file.

  python tools/diag_gradient_bench.py [--n 30] [--reps 7] [--out profiles/diagonal/diag_gradient_n30.json]

The state is |+>^n, where a QAOA run starts; cost = ZZ on all pairs (435 terms at n = 30) as a Diagonal.  Both precisions run one after
the other in ONE child process under `timeout -k 10` (the parent never opens the GPU).  Every row is the WHOLE call on the host clock
— the call and, where it does not wait itself, the synchronisation of the state's stream behind it — warm, median of --reps (>= 5),
with the fastest and the slowest repetition.  Rows per precision (fp64, fp32):
  qaoa_p1, qaoa_p2, qaoa_p4   energy_and_gradient(layers, cost) for p layers of (gamma, cost) and an X mixer on every qubit
  phase                       apply_diagonal_phase(cost, gamma): the forward sweep, in the same process; timed last, so that every
                              gradient row starts from |+>^n
  diag_1, diag_2              energy_and_gradient([(gamma, cost)] * k, cost) for k = 1, 2: diag_2 - diag_1 is one forward phase and
                              one backward diagonal sweep more
  diag_adjoint                diag_2 - diag_1 - phase: ONE backward diagonal sweep.  A difference of medians, not an event pair: the C
                              ABI has no entry that launches a backward sweep alone
  strings_p1                  the gradient of qaoa_p1 with the separator spelled as 435 Z rotations and the cost as 435 strings, through
                              the same call without any Diagonal: what a caller had before
and the ratio against the byte model: an fp64 amplitude of the backward sweep moves 72 B against 40 B of the phase sweep,
an fp32 one 40 B against 24 B.  x_phase = diag_adjoint / phase, x_model = x_phase / that ratio, `met` = x_model <= 1.15."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)

MODEL = {64: 72.0 / 40.0, 32: 40.0 / 24.0}
ALLOWED = 1.15
LAYERS = (1, 2, 4)


def pair_terms(n):
    return [(1.0, f"Z{a} Z{b}") for a in range(n) for b in range(a + 1, n)]


def child(args):
    from gpu_quantum_simulator_amd import Circuit, Diagonal, Simulator, _lib, plans
    n, gamma, beta = args.n, 0.37, 0.52
    _lib.load()  # libqsim (and torch's HIP runtime, where there is one) before anything else opens the device
    pairs = pair_terms(n)
    mixer = [(2.0 * beta, f"X{q}") for q in range(n)]
    result = {}
    for precision in (64, 32):
        rows = {}
        with Simulator(n, precision=precision) as sim, Diagonal.from_terms(n, pairs) as cost:
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

            one = timed("diag_1", lambda: sim.energy_and_gradient([(gamma, cost)], cost))
            two = timed("diag_2", lambda: sim.energy_and_gradient([(gamma, cost)] * 2, cost))
            for p in LAYERS:
                layers = ([(gamma, cost)] + mixer) * p
                before = (plans.sweeps_launched("diagonal_adjoint"), plans.sweeps_launched("pauli_adjoint"))
                energy, grad = sim.energy_and_gradient(layers, cost)
                taken = (plans.sweeps_launched("diagonal_adjoint") - before[0], plans.sweeps_launched("pauli_adjoint") - before[1])
                row = timed(f"qaoa_p{p}", lambda: sim.energy_and_gradient(layers, cost))
                row.update(parameters=len(layers), diag_adjoint_sweeps=taken[0], pauli_adjoint_sweeps=taken[1], energy=energy, dE_dgamma_0=float(grad[0]))
            spelled = [(2.0 * gamma * c, text) for c, text in pairs] + mixer
            energy, grad = sim.energy_and_gradient(spelled, pairs)
            row = timed("strings_p1", lambda: sim.energy_and_gradient(spelled, pairs))
            # the chain rule: dE/dgamma = sum_k 2 c_k dE/dtheta_k over the separator's rotations
            row.update(parameters=len(spelled), energy=energy, dE_dgamma_0=float(sum(2.0 * c * g for (c, _), g in zip(pairs, grad))))
            row["x_qaoa_p1"] = round(row["ms"] / rows["qaoa_p1"]["ms"], 3)
            # last: every row above starts from |+>^n, which a gradient call leaves as it found it; the phases move the state
            phase = timed("phase", lambda: sim.apply_diagonal_phase(cost, gamma))
            back = two["ms"] - one["ms"] - phase["ms"]
            rows["diag_adjoint"] = {"ms": round(back, 4), "how": "diag_2 - diag_1 - phase", "x_phase": round(back / phase["ms"], 3),
                                    "model": round(MODEL[precision], 3), "x_model": round(back / phase["ms"] / MODEL[precision], 3),
                                    "met": bool(back / phase["ms"] / MODEL[precision] <= ALLOWED)}
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
    if p.returncode != 0 or not lines:  # nothing more is started on the GPU after a failure
        sys.stderr.write(p.stdout[-2000:] + p.stderr[-2000:])
        sys.exit(p.returncode or 1)
    result = {"n": args.n, "reps": max(5, args.reps), "timing": "whole call on the host clock, state's stream synchronised", "allowed_x_model": ALLOWED}
    result.update(json.loads(lines[-1][5:]))
    out = args.out or os.path.join(ROOT, "profiles", "diagonal", f"diag_gradient_n{args.n}.json")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result)[:6000])


if __name__ == "__main__":
    main()
