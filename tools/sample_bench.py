"""Times drawing shots on the device (Simulator.sample_shots, qsim_sample_shots) and writes ONE JSON file.

  python tools/sample_bench.py [--n 30] [--reps 7] [--out profiles/sample/sample_n30.json]

The state is the dense state the bench circuit leaves (1000 seeded random gates, as bench.py runs it).  Both precisions run one after
the other in ONE child process under `timeout -k 10` (the parent never opens the GPU).  Warm, median of --reps (>= 5) with the fastest
and the slowest repetition.  Rows per precision (fp64, fp32):
  norm2                    the state's squared norm, the whole call on the host clock: the read-only sweep of the state alone
  chunk_sums, prefix       the two preparing stages between device events (qsim_sample_stage_times): the sweep that forms the chunk
                           totals, and the two launches that turn them into running sums
  shots_1                  the whole call for ONE draw on the host clock: allocation, upload, both stages, one wave, download, free
  shots_2^10, 2^16, 2^20   the whole call for that many seeded draws on the host clock, and the time per draw beyond shots_1
  sample_2^10, 2^12        qsim_sample (Simulator.sample), the reference-parity path, on the FIRST 2^10 and 2^12 of the same draws:
                           one repetition each after a warm call of 16 draws; `agree` = the share of these draws on which both return
                           the same index
x_norm2 of chunk_sums is its time over norm2's: the model is one read of the state, 1.0."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)

SHOTS = (10, 16, 20)
OLD_SHOTS = (10, 12)


def _row(ms):
    return {"ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4)}


def child(args):
    from ctypes import byref, c_double

    import numpy as np

    from gpu_quantum_simulator_amd import Circuit, Simulator, _lib, circuits
    n, reps = args.n, max(5, args.reps)
    lib = _lib.load()
    draws = np.random.default_rng(20240117).random(1 << max(SHOTS))
    result = {}
    for precision in (64, 32):
        rows = {}
        with Simulator(n, precision=precision) as sim:
            sim.run(Circuit.from_gates(n, circuits.random_gates(n, 1000, 20240117 + n, "all")))
            sim.sync()

            def timed(name, fn):
                fn()  # warm
                ms = []
                for _ in range(reps):
                    t0 = time.perf_counter()
                    fn()
                    ms.append((time.perf_counter() - t0) * 1e3)
                rows[name] = _row(ms)
                return rows[name]

            norm2 = timed("norm2", sim.norm2)
            a, b = c_double(), c_double()
            stages = []
            for _ in range(reps + 1):
                _lib.check(lib.qsim_sample_stage_times(sim._h, byref(a), byref(b)))
                stages.append((a.value, b.value))
            rows["chunk_sums"] = _row([s[0] for s in stages[1:]])
            rows["prefix"] = _row([s[1] for s in stages[1:]])
            rows["chunk_sums"]["x_norm2"] = round(rows["chunk_sums"]["ms"] / norm2["ms"], 3)
            one = timed("shots_1", lambda: sim.sample_shots(draws=draws[:1]))
            got = {}
            for e in SHOTS:
                row = timed(f"shots_2^{e}", lambda: got.__setitem__(e, sim.sample_shots(draws=draws[:1 << e])))
                row["us_per_draw_beyond_one"] = round((row["ms"] - one["ms"]) * 1e3 / (1 << e), 4)
            rows["norm2_end"] = timed("norm2_end", sim.norm2)
            sim.sample(draws[:16])  # warm
            for e in OLD_SHOTS:
                t0 = time.perf_counter()
                old = sim.sample(draws[:1 << e])
                ms = (time.perf_counter() - t0) * 1e3
                new = got[max(SHOTS)][:1 << e]
                rows[f"sample_2^{e}"] = {"ms": round(ms, 3), "us_per_draw": round(ms * 1e3 / (1 << e), 3), "agree": float(np.mean(old == new))}
            rows["shots_2^10"]["x_sample"] = round(rows["shots_2^10"]["ms"] / rows["sample_2^10"]["ms"], 5)
            rows["values"] = {"norm2": sim.norm2(), "distinct_of_2^20": int(np.unique(got[max(SHOTS)]).size)}
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
    result = {"n": args.n, "reps": max(5, args.reps),
              "timing": "host clock around whole calls that wait; chunk_sums and prefix between device events"}
    result.update(json.loads(lines[-1][5:]))
    out = args.out or os.path.join(ROOT, "profiles", "sample", f"sample_n{args.n}.json")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result)[:6000])


if __name__ == "__main__":
    main()
