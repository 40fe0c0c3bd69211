"""Digests of what the Pauli sweeps compute on the device: the instrument of a change that must leave every result bit as it is.
Both kernels promise equal bits for equal calls (no atomics, a fixed-order reduction), so two builds compute alike exactly when
their files are equal byte for byte.

  pauli_digest.py OUT.txt      one line per case: its name and the sha256 over the float64 expectation values, or over the state
                               read back after the rotations (QSIM_LIB picks another build of the library)

Cases come from the generators of tests/pauli_ref.py and tests/pauli_rot_ref.py: for n in NS and both precisions on one state,
expectation values of random strings of every weight and of a single X, Y or Z at every position, and the states after
single_bit_rotations, every_weight_rotations and long_run_rotations (its x cut to the register); the same, in fp64, on clusters of
2 and 4 shards on one device, where the strings with X or Y on a shard-selecting qubit sweep a shard against its partner's buffer."""
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import pauli_ref  # noqa: E402
import pauli_rot_ref as ref  # noqa: E402

NS = (1, 2, 5, 7, 9, 13)
CLUSTER_NS, CLUSTER_SHARDS = (5, 9), (2, 4)


def expectation_strings(n):
    rng = np.random.default_rng(500 + n)
    masks = [pauli_ref.random_masks(rng, n, 1 + i % n) for i in range(80)] + [(x, z) for _, x, z in ref.single_bit_rotations(n)]
    return [pauli_ref.masks_to_text(x, z, n) for x, z in masks]


def rotation_cases(n, K):
    mask = (1 << n) - 1
    diag, paired = ref.long_run_rotations(K, n)
    yield "single_bit", ref.single_bit_rotations(n)
    yield "every_weight", ref.every_weight_rotations(n)
    yield "long_runs", diag + [(theta, x & mask, z) for theta, x, z in paired]


def cases():
    """(name, bytes) of every case, in a fixed order."""
    from gpu_quantum_simulator_amd import Circuit, Cluster, Simulator, _lib, circuits
    K = _lib.load().qsim_pauli_rotations_per_sweep()
    for n in NS:
        for precision in (64, 32):
            with Simulator(n, precision=precision) as sim:
                sim.write(ref.rand_state(n, 300 + n))
                yield f"state n={n} p{precision} expectation", sim.expectation_terms(expectation_strings(n)).tobytes()
                for name, rotations in rotation_cases(n, K):
                    sim.write(ref.rand_state(n, 300 + n))
                    sim.apply_pauli_rotations(ref.texts(rotations, n))
                    yield f"state n={n} p{precision} {name}", sim.read().tobytes()
    for n in CLUSTER_NS:
        for shards in CLUSTER_SHARDS:
            circuit = Circuit.from_gates(n, circuits.random_gates(n, 60, 7 + n, "all"))
            with Cluster(n, shards, devices=[0] * shards) as cl:
                cl.run(circuit)
                yield f"cluster n={n} shards={shards} expectation", cl.expectation_terms(expectation_strings(n)).tobytes()
                for name, rotations in rotation_cases(n, K):
                    cl.apply_pauli_rotations(ref.texts(rotations, n))  # on top of what the case before left
                    yield f"cluster n={n} shards={shards} {name}", cl.read().tobytes()
                yield f"cluster n={n} shards={shards} expectation afterwards", cl.expectation_terms(expectation_strings(n)).tobytes()


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    with open(sys.argv[1], "w") as out:
        for name, data in cases():
            out.write(f"{name}: {hashlib.sha256(data).hexdigest()}\n")
