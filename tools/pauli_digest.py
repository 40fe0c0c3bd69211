"""Digests of what the Pauli sweeps compute on the device: the instrument of a change that must leave every result bit as it is.
Both kernels promise equal bits for equal calls (no atomics, a fixed-order reduction), so two builds compute alike exactly when
their files are equal byte for byte.

  pauli_digest.py OUT.txt      one line per case: its name and the sha256 over the float64 expectation values, over the state read
                               back after the rotations, over (energy, gradient) of a gradient call and over the state read back
                               after it, or over the destination of pauli_sum_into (QSIM_LIB picks another build of the library)

Cases come from the generators of tests/pauli_ref.py and tests/pauli_rot_ref.py: for n in NS and both precisions on one state,
expectation values of random strings of every weight and of a single X, Y or Z at every position, and the states after
single_bit_rotations, every_weight_rotations and long_run_rotations (its x cut to the register); the same, in fp64, on clusters of
2 and 4 shards on one device, where the strings with X or Y on a shard-selecting qubit sweep a shard against its partner's buffer.
Gradient cases come from tests/adjoint_ref.py, both precisions on one state: geometry_strings(n) for n in (1, 2, 9), one call per
string; order_case() in both orders; the runs longer than K of long_run_rotations; and sum_cases(9) through pauli_sum_into, into a
buffer that torch allocates and reads back.  The adjoint sweep's grid does not depend on the grid cap, so these bits are the build's."""
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import adjoint_ref  # noqa: E402
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


def gradient_cases(K):
    """(name, n, [rotations of one call, ...], terms): the calls of a case follow one another on one state."""
    for n in (1, 2, 9):
        yield f"geometry n={n}", n, [[(0.7, x, z)] for x, z in adjoint_ref.geometry_strings(n)], adjoint_ref.random_hamiltonian(n, 6, 300 + n, 2)
    ab, ba, terms = adjoint_ref.order_case()
    yield "order ab", 6, [ab], terms
    yield "order ba", 6, [ba], terms
    diag, paired = ref.long_run_rotations(K)
    yield "long_runs", 12, [diag, paired, diag + paired], adjoint_ref.random_hamiltonian(12, 10, 1200, 2)


def cases():
    """(name, bytes) of every case, in a fixed order."""
    import torch
    from gpu_quantum_simulator_amd import Circuit, Cluster, Simulator, circuits, plans
    K = plans.pauli_rotations_per_sweep()
    for n in NS:
        for precision in (64, 32):
            with Simulator(n, precision=precision) as sim:
                sim.write(ref.rand_state(n, 300 + n))
                yield f"state n={n} p{precision} expectation", sim.expectation_terms(expectation_strings(n)).tobytes()
                for name, rotations in rotation_cases(n, K):
                    sim.write(ref.rand_state(n, 300 + n))
                    sim.apply_pauli_rotations(ref.texts(rotations, n))
                    yield f"state n={n} p{precision} {name}", sim.read().tobytes()
    for name, n, calls, terms in gradient_cases(K):
        for precision in (64, 32):
            with Simulator(n, precision=precision) as sim:
                sim.write(ref.rand_state(n, 300 + n))
                results = [sim.energy_and_gradient(ref.texts(rotations, n), adjoint_ref.term_texts(terms, n)) for rotations in calls]
                yield f"gradient {name} p{precision} energy and gradient", b"".join(np.float64(e).tobytes() + g.tobytes() for e, g in results)
                yield f"gradient {name} p{precision} state afterwards", sim.read().tobytes()
    for precision in (64, 32):
        n = 9
        with Simulator(n, precision=precision) as sim:
            sim.write(ref.rand_state(n, 300 + n))
            for name, terms in adjoint_ref.sum_cases(n).items():
                dst = torch.full((2 << n,), 3.0, dtype=torch.float64 if precision == 64 else torch.float32, device="cuda")  # overwritten
                torch.cuda.synchronize()
                sim.pauli_sum_into(adjoint_ref.term_texts(terms, n), dst.data_ptr())
                sim.sync()
                yield f"pauli_sum_into {name} p{precision}", dst.cpu().numpy().tobytes()
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
