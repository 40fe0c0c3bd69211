"""The tests' own checker for Pauli-string rotations exp(-i theta/2 P): a numpy restatement of the pair formula the device sweeps
implement, in complex128 or in complex64 (tests/test_pauli_rot_cpu.py pins it against dense operators), and the rotation
sequences of the GPU tests as data, so that the CPU test can hold every fp32 sequence to fp32_ref.REF_CAP.

A string is two masks (tests/pauli_ref.py).  With s(j) = (-1)^popcount(j & z), ny = popcount(x & z), c = cos(theta/2) and
w = -i sin(theta/2) i^ny, every index j gets   psi_j' = c psi_j + w (-1)^ny s(j) psi_(j^x)   (for the other member of a pair,
j = k ^ x, this is the second line of the pair rule, since s(k ^ x) = (-1)^ny s(k))."""
import math

import numpy as np

import pauli_ref


def _sign(n_amps, z, real):
    j = np.arange(n_amps, dtype=np.uint64)
    return (1 - 2 * pauli_ref._parity(j & np.uint64(z))).astype(real)


def apply_rotation(psi, x, z, theta, dtype=np.complex128):
    """exp(-i theta/2 P) psi as a new array of `dtype`: c and w are formed in fp64, rounded once to `dtype`, and applied with
    `dtype` arithmetic."""
    psi = np.asarray(psi, dtype=dtype)
    real = np.float64 if dtype == np.complex128 else np.float32
    c, sn = math.cos(0.5 * theta), math.sin(0.5 * theta)
    ny = bin(x & z).count("1")
    w = (-1j * sn, sn, 1j * sn, -sn)[ny % 4] * (-1) ** ny  # w (-1)^ny, exactly (no product is rounded)
    s = _sign(psi.size, z, real)
    partner = psi[np.arange(psi.size, dtype=np.uint64) ^ np.uint64(x)]
    return (real(c) * psi + dtype(w) * (s * partner)).astype(dtype)


def replay(psi, rotations, dtype=np.complex128):
    """`rotations` = [(theta, x, z), ...] applied in order, the first one first."""
    out = np.asarray(psi, dtype=dtype)
    for theta, x, z in rotations:
        out = apply_rotation(out, x, z, theta, dtype)
    return out


def dense_rotation(x, z, n, theta):
    return math.cos(0.5 * theta) * np.eye(1 << n) - 1j * math.sin(0.5 * theta) * pauli_ref.dense_pauli(x, z, n)


def texts(rotations, n):
    """[(theta, x, z)] -> [(theta, "X0 Z3 ...")] as Simulator.apply_pauli_rotations takes them."""
    return [(theta, pauli_ref.masks_to_text(x, z, n)) for theta, x, z in rotations]


def rand_state(n, seed):
    rng = np.random.default_rng(seed)
    s = rng.standard_normal(1 << n) + 1j * rng.standard_normal(1 << n)
    return (s / np.linalg.norm(s)).astype(np.complex128)


# ---- the sequences of tests/test_gpu_pauli_rot.py, as data ------------------------------------------------------------------
SPECIAL_ANGLES = (0.0, math.pi, 2.0 * math.pi, -math.pi, -0.75, 4.5 * math.pi)
EVERY_WEIGHT_SIZES = (1, 2, 5, 6, 7, 13, 18)
LONG_RUN_X = 0b100000100101  # lane bits, bit 0 and a high bit of a 12-qubit register


def single_bit_rotations(n=13):
    """"X_q Z_r", "Y_q Z_r" (r = q + 1 mod n) and "Z_q" for every q: x lands in every lane, wave and uniform region."""
    rng = np.random.default_rng(130)
    out = []
    for q in range(n):
        r = (q + 1) % n
        out += [(float(rng.uniform(-3, 3)), 1 << q, 1 << r), (float(rng.uniform(-3, 3)), 1 << q, 1 << q | 1 << r), (float(rng.uniform(-3, 3)), 0, 1 << q)]
    return out


def every_weight_rotations(n):
    """About 200 random strings of every weight 1..n with random angles."""
    rng = np.random.default_rng(2000 + n)
    out = [(float(rng.uniform(-math.pi, math.pi)),) + pauli_ref.random_masks(rng, n, 1 + i % n) for i in range(max(200, 12 * n))]
    assert {bin(x | z).count("1") for _, x, z in out} == set(range(1, n + 1))
    return out


def long_run_rotations(K, n=12):
    """3K + 5 all-Z terms, then 3K + 5 terms sharing LONG_RUN_X — among them non-commuting neighbours and the identity; the angles
    include 0, pi, 2 pi and negative ones.  Returns (diagonal run, paired run)."""
    rng = np.random.default_rng(12)
    big = 3 * K + 5

    def angle(i):
        return SPECIAL_ANGLES[i % 7] if i % 7 < len(SPECIAL_ANGLES) else float(rng.uniform(-math.pi, math.pi))

    diag = [(angle(i), 0, int(z)) for i, z in enumerate(rng.integers(1, 1 << n, size=big))]
    diag[5] = (0.9, 0, 0)  # the identity joins the diagonal run
    paired = [(angle(i + 3), LONG_RUN_X, int(z)) for i, z in enumerate(rng.integers(0, 1 << n, size=big))]
    paired[10] = (1.1, LONG_RUN_X, 0)
    paired[11] = (0.7, LONG_RUN_X, 1)  # X0 ... then Y0 ...: anticommuting neighbours with one x
    return diag, paired


ORDER_PAIR = [(0.8, 0b11, 0b00), (1.3, 0b11, 0b01)]  # "X0 X1" and "Y0 X1": one x, they anticommute
AFTER_FEW = [(0.6, 1 << 17 | 1, 0), (-1.2, 1 << 17 | 1, 1 << 9), (0.4, 0, 1 << 12 | 1 << 3), (2.2, 1 << 10 | 1 << 5, 1 << 10), (0.3, 1 << 2, 0)]
AFTER_FEW_GATES = [("h", 15), ("cx", 15, 2), ("rz", 0.37, 17), ("sx", 0)]


RZ_CASE = (9, 6, 0.83)  # n, qubit, theta of the rz-convention test
FRESH_SIZES = [1, 4, 13, 20]
FRESH_THETA = 0.9


def fresh_rotation(n):
    """The one rotation a never-touched register gets: "Y0" at n = 1, "X0 X{n-1}" above."""
    return (FRESH_THETA, 1, 1) if n == 1 else (FRESH_THETA, 1 | 1 << (n - 1), 0)


def queued_rotations(n=13):
    rng = np.random.default_rng(104)
    return [(float(rng.uniform(-2, 2)),) + pauli_ref.random_masks(rng, n, 1 + i % n) for i in range(40)] + [(0.5, 1, 0), (0.25, 1 << 12, 1 << 12)]


def reproducible_rotations(n=16):
    rng = np.random.default_rng(16)
    return [(float(rng.uniform(-2, 2)),) + pauli_ref.random_masks(rng, n, 1 + i % n) for i in range(64)]


DRIFT_TIME, DRIFT_STEPS = 0.4, 20  # the energy-drift run of test_gpu_pauli_rot.test_evolve_ising (its docstring has the bound)


def ising_terms(n=8, j=1.0, h=0.7):
    """A transverse-field Ising chain as (coefficient, string) pairs: the ZZ layer, then the X layer."""
    return [(-j, f"Z{q} Z{q + 1}") for q in range(n - 1)] + [(-h, f"X{q}") for q in range(n)]


def diagonal_hamiltonian(n=10, terms=30):
    rng = np.random.default_rng(30)
    out = []
    for i in range(terms):
        z = int(rng.integers(1, 1 << n))
        out.append((float(rng.uniform(-1, 1)), pauli_ref.masks_to_text(0, z, n)))
    return out


def masks_of(rotation_texts, n):
    from gpu_quantum_simulator_amd import pauli_masks
    return [(theta,) + pauli_masks(text, n) for theta, text in rotation_texts]


def fp32_sequences(K):
    """(label, n, start state, [(theta, x, z)]) of every rotation sequence the GPU tests run on an fp32 state
    from a state the test knows beforehand (the others start from whatever the engine holds and are checked call by call)."""
    from gpu_quantum_simulator_amd import trotter_rotations
    yield "single_bit", 13, rand_state(13, 13), single_bit_rotations()
    for n in EVERY_WEIGHT_SIZES:
        yield f"every_weight_n{n}", n, rand_state(n, 40 + n), every_weight_rotations(n)
    diag, paired = long_run_rotations(K)
    yield "long_runs", 12, rand_state(12, 12), diag + paired
    yield "order_ab", 6, rand_state(6, 6), ORDER_PAIR
    yield "order_ba", 6, rand_state(6, 6), ORDER_PAIR[::-1]
    yield "rz_convention", RZ_CASE[0], rand_state(RZ_CASE[0], 9), [(RZ_CASE[2], 0, 1 << RZ_CASE[1])]
    for n in FRESH_SIZES:
        zero = np.zeros(1 << n, dtype=np.complex128)
        zero[0] = 1.0
        yield f"fresh_n{n}", n, zero, [fresh_rotation(n)]
    yield "reproducible", 16, rand_state(16, 160), reproducible_rotations() + reproducible_rotations()[::-1]
    yield "after_few", 18, rand_state(18, 18), AFTER_FEW  # the rotations themselves, on a dense stand-in for the circuit's state
    yield "queued", 13, rand_state(13, 104), queued_rotations()
    for order in (1, 2):
        yield f"ising_order{order}", 8, rand_state(8, 8), masks_of(trotter_rotations(ising_terms(), 0.9, 3, order), 8)
    yield "ising_20_steps", 8, rand_state(8, 8), masks_of(trotter_rotations(ising_terms(), DRIFT_TIME, DRIFT_STEPS, 2), 8)
    yield "diagonal_h", 10, rand_state(10, 10), masks_of(trotter_rotations(diagonal_hamiltonian(), 0.8, 1, 1), 10)
