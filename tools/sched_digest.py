"""Digests of the host scheduler's output over a grid of circuits and settings: the instrument of a change that must leave every
schedule as it is.  Host only: no device is opened (torch is not loaded), nothing outside the package and numpy is imported.

  sched_digest.py OUT.txt            one run under the environment as it is (QSIM_LIB picks another build of the library)
  sched_digest.py --all DIR [JOBS]   DIR/sched_digests_default.txt with no QSIM_SCHED_* variable set, then one file per variable,
                                     each set alone to a value other than its default (KNOBS), each run in a child process of its
                                     own; fails unless the files differ from one another (every knob was live)
  sched_digest.py --shard-plans OUT.txt   the shard planner's plans (it schedules every segment with gates tracked per pass and a partial
                                     initial support), in the configurations of profiles/dist_split: run it with QSIM_SHARD_TAIL unset, 0 and 24
  sched_digest.py --tile-records OUT.txt [ORDER_SEED ...]   what the digests above do not cover: Circuit.tile_records() — every field of
                                     every record, under order seeds 0, 1 and 7 unless others are named (files of different seeds must
                                     differ) — and the schedule with deferred X gates, Circuit.schedule(flips=[]), with its flip mask

A configuration is random_gates(n, 1000, seed, vocabulary) x fuse x tile geometry; its digest is the sha256 over
  * every entry of Circuit.schedule() for tile_max_ops 1, 8 and 32: pass, kernel class, kind, qubits, gates folded, matrix as raw bytes;
  * every field of Circuit.passes() for initial_support 0, the lower half of the qubits and all ones;
  * Circuit.plan() for the same three.
To keep the files small a line holds n, the number of configurations behind it (vocabularies x seeds x fuse x geometries) and the sha256
over their digests; --shard-plans likewise writes one line per n.  Two builds schedule alike exactly when their files are
equal byte for byte; a line that differs names the group to look into (digest() and lines_for() give the single configurations)."""
import hashlib
import os
import subprocess
import sys

os.environ.setdefault("QSIM_NO_TORCH_PRELOAD", "1")
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

NS = (3, 6, 9, 12, 16, 20, 24, 28, 30, 33)
VOCABULARIES = ("all", "clifford_t")
SEEDS = (11, 12, 13)
FUSE = (0, 1, 2, 3)
GEOMETRIES = ((12, 3), (11, 3), (13, 3), (12, 5), (8, 2))
TILE_MAX_OPS = (1, 8, 32)
# every QSIM_SCHED_* variable with a value that is not its default (scheduler.h SchedConfig, fusion.cpp engine_sched_config)
KNOBS = (("LOOKAHEAD", "2"), ("ROLLOUT", "2"), ("WINDOW", "48"), ("LOCAL", "2"), ("OBJ", "1"), ("MERGE", "0"), ("MERGEQ", "4"),
         ("CAP", "12"), ("CHEAP", "0.25"), ("NOCOMMUTE", "1"), ("SEED", "7"), ("SUPW", "5"))


def digest(circuit, n, fuse, tile_bits, low_bits):
    h = hashlib.sha256()
    for cap in TILE_MAX_OPS:
        for pass_i, kclass, kind, qubits, matrix, folded in circuit.schedule(fuse, tile_bits, low_bits, cap):
            h.update(repr((cap, pass_i, kclass, kind, qubits, folded)).encode())
            if matrix is not None:
                h.update(matrix.tobytes())
    for support in (0, (1 << (n // 2)) - 1, (1 << 64) - 1):
        for p in circuit.passes(fuse, tile_bits, low_bits, support):
            h.update(repr((p["kernel"], p["blocks"], p["tile_mask"], p["visited"].hex(), p["bytes"].hex(), p["cost_bytes"].hex())).encode())
        h.update(repr(sorted(circuit.plan(fuse, tile_bits, low_bits, support).items())).encode())
    return h.hexdigest()


def lines_for(n):
    from gpu_quantum_simulator_amd import Circuit, circuits
    group = []
    for vocabulary in VOCABULARIES:
        for seed in SEEDS:
            c = Circuit.from_gates(n, circuits.random_gates(n, 1000, seed, vocabulary))
            for fuse in FUSE:
                for tile_bits, low_bits in GEOMETRIES:
                    group.append(f"{vocabulary} {seed} {fuse} {tile_bits} {low_bits} {digest(c, n, fuse, tile_bits, low_bits)}")
    return [f"n={n} configurations={len(group)} {hashlib.sha256(' '.join(group).encode()).hexdigest()}\n"]


def shard_plans(path):
    """Every step, every shard's local ops with their matrices as raw bytes, step_support, exchange_roles of every rank, final_pos and
    predict, hashed per configuration."""
    import numpy as np
    from gpu_quantum_simulator_amd import Circuit, ShardPlanHandle, circuits
    with open(path, "w") as out:
        for n in (8, 12, 15, 16, 18):
            group, steps, exchanged = [], 0, 0
            for shards in (1, 2, 4, 8, 16, 32):
                for vocabulary in VOCABULARIES:
                    for seed in SEEDS:
                        plan = ShardPlanHandle(Circuit.from_gates(n, circuits.random_gates(n, 400, seed + 100 * n, vocabulary)), shards)
                        h = hashlib.sha256()
                        exchanges = 0
                        for i in range(plan.num_steps):
                            step = plan.step(i)
                            h.update(repr(step).encode())
                            if step[0] == "local":
                                for rank in range(shards):
                                    for op in plan.local_ops(i, rank):
                                        h.update(repr(op[:2] if op[0] == "u1" else op[:1] if op[0] == "scale" else op).encode())
                                        if op[0] != "cx":
                                            h.update(np.asarray(op[-1], dtype=np.complex128).tobytes())
                            else:
                                exchanges += 1
                                h.update(repr(plan.step_support(i)).encode())
                                for rank in range(shards):
                                    h.update(repr(sorted(plan.exchange_roles(i, rank).items())).encode())
                        h.update(repr(plan.final_pos()).encode())
                        h.update(repr([x.hex() for x in plan.predict()]).encode())
                        group.append(f"{shards} {vocabulary} {seed} {plan.num_steps} {exchanges} {h.hexdigest()}")
                        steps += plan.num_steps
                        exchanged += exchanges
            out.write(f"n={n} configurations={len(group)} steps={steps} exchanges={exchanged} {hashlib.sha256(' '.join(group).encode()).hexdigest()}\n")


def tile_records(path, order_seeds=(0, 1, 7)):
    """One line per n: random_gates(n, 400, seed, vocabulary) x geometry, each with its records for fp64 and fp32 under every order
    seed (matrices and record bytes raw) and its deferred schedule with the flip mask."""
    from gpu_quantum_simulator_amd import Circuit, circuits
    with open(path, "w") as out:
        for n in (3, 6, 9, 12, 16):
            h, records = hashlib.sha256(), 0
            for vocabulary in VOCABULARIES:
                for seed in (11, 12):
                    c = Circuit.from_gates(n, circuits.random_gates(n, 400, seed, vocabulary))
                    for tile_bits, low_bits in ((12, 3), (13, 4), (8, 2)):
                        for f32 in (0, 1):
                            for order_seed in order_seeds:
                                for r in c.tile_records(3, tile_bits, low_bits, 32, bool(f32), order_seed):
                                    h.update(repr((vocabulary, seed, tile_bits, low_bits, f32, order_seed, r["pass"], r["tile_bits"], r["low_bits"],
                                                   r["high"], r["selectors"], r["qubits"])).encode())
                                    h.update(r["matrix"].tobytes())
                                    h.update(r["record"])
                                    records += 1
                        flips = []
                        for pass_i, kclass, kind, qubits, matrix, folded in c.schedule(3, tile_bits, low_bits, 32, flips):
                            h.update(repr((pass_i, kclass, kind, qubits, folded)).encode())
                            if matrix is not None:
                                h.update(matrix.tobytes())
                        h.update(repr(flips).encode())
            out.write(f"n={n} order_seeds={','.join(map(str, order_seeds))} records={records} {h.hexdigest()}\n")


def run(path, jobs):
    from multiprocessing import Pool
    with Pool(jobs) as pool: # the workers are forked before the library is loaded
        chunks = pool.map(lines_for, sorted(NS, reverse=True), chunksize=1)
    with open(path, "w") as f:
        for chunk in reversed(chunks):
            f.writelines(chunk)


def run_all(outdir, jobs):
    os.makedirs(outdir, exist_ok=True)
    base = {k: v for k, v in os.environ.items() if not k.startswith("QSIM_SCHED_")}
    sums = {}
    for name, value in (("default", None),) + KNOBS:
        path = os.path.join(outdir, f"sched_digests_{name.lower()}.txt")
        env = dict(base)
        if value is not None:
            env["QSIM_SCHED_" + name] = value
        subprocess.check_call([sys.executable, os.path.abspath(__file__), path, str(jobs)], env=env)
        with open(path, "rb") as f:
            sums[name] = hashlib.sha256(f.read()).hexdigest()
        print(f"{sums[name]}  {os.path.basename(path)}", flush=True)
    if len(set(sums.values())) != len(sums):
        sys.exit("two settings gave the same digests: a knob was not live")


if __name__ == "__main__":
    if len(sys.argv) >= 3 and sys.argv[1] == "--all":
        run_all(sys.argv[2], int(sys.argv[3]) if len(sys.argv) > 3 else 4)
    elif len(sys.argv) >= 3 and sys.argv[1] == "--shard-plans":
        shard_plans(sys.argv[2])
    elif len(sys.argv) >= 3 and sys.argv[1] == "--tile-records":
        tile_records(sys.argv[2], tuple(int(x) for x in sys.argv[3:]) or (0, 1, 7))
    elif len(sys.argv) >= 2:
        run(sys.argv[1], int(sys.argv[2]) if len(sys.argv) > 2 else 4)
    else:
        sys.exit(__doc__)
