"""The tests' own checker for adjoint-mode gradients (qsim_pauli_gradient, csrc/adjoint.hip): a numpy restatement of the adjoint
algorithm on top of pauli_rot_ref.apply_rotation (tests/test_adjoint_cpu.py pins it against the shift rule and dense operators),
and the cases of tests/test_gpu_adjoint.py as data.

Circuit |psi_k> = U_k ... U_1 |psi_0>, U_k = exp(-i theta_k/2 P_k); H = sum_t c_t Q_t with real c_t; E = <psi_K|H|psi_K>.
|lambda_K> = H |psi_K>, |lambda_(k-1)> = U_k^+ |lambda_k>, and dE/dtheta_k = Im <lambda_k|P_k|psi_k>."""
import math

import numpy as np

import pauli_ref
import pauli_rot_ref


def apply_pauli(psi, x, z):
    """P psi in psi's dtype: (P psi)_i = i^ny s(i ^ x) psi_(i ^ x).  Exact: a permutation and a factor of +-1 or +-i."""
    psi = np.asarray(psi)
    i = np.arange(psi.size, dtype=np.uint64) ^ np.uint64(x)
    s = 1 - 2 * pauli_ref._parity(i & np.uint64(z))
    return (1j ** (bin(x & z).count("1") % 4) * s * psi[i]).astype(psi.dtype)


def apply_sum(psi, terms, dtype=np.complex128):
    """sum_t c_t Q_t psi for terms [(c, x, z)], in `dtype`: coefficients rounded once, sums in `dtype`."""
    psi = np.asarray(psi, dtype=dtype)
    real = np.float64 if dtype == np.complex128 else np.float32
    out = np.zeros(psi.size, dtype=dtype)
    for c, x, z in terms:
        out = (out + real(c) * apply_pauli(psi, x, z)).astype(dtype)
    return out


def gradient(psi0, rotations, terms, dtype=np.complex128):
    """(E, grad, psi_K) by the adjoint algorithm: states and rotations in `dtype`, every inner product in fp64."""
    psi = pauli_rot_ref.replay(psi0, rotations, dtype)
    final = psi
    lam = apply_sum(psi, terms, dtype)
    wide = np.complex128
    energy = float(np.vdot(lam.astype(wide), psi.astype(wide)).real)
    grad = np.zeros(len(rotations))
    for k in range(len(rotations) - 1, -1, -1):
        theta, x, z = rotations[k]
        grad[k] = float(np.vdot(lam.astype(wide), apply_pauli(psi, x, z).astype(wide)).imag)
        psi = pauli_rot_ref.apply_rotation(psi, x, z, -theta, dtype)
        lam = pauli_rot_ref.apply_rotation(lam, x, z, -theta, dtype)
    return energy, grad, final


def energy(psi0, rotations, terms):
    """E in fp64 from the replayed state and pauli_ref.pauli_expectation: independent of the adjoint algorithm."""
    psi = pauli_rot_ref.replay(psi0, rotations)
    return sum(c * pauli_ref.pauli_expectation(psi, x, z) for c, x, z in terms)


def shift_gradient(psi0, rotations, terms, which=None):
    """The exact shift rule [E(theta_k + pi/2) - E(theta_k - pi/2)] / 2 for the components `which` (default: all)."""
    out = {}
    for k in (range(len(rotations)) if which is None else which):
        theta, x, z = rotations[k]
        plus = rotations[:k] + [(theta + 0.5 * math.pi, x, z)] + rotations[k + 1:]
        minus = rotations[:k] + [(theta - 0.5 * math.pi, x, z)] + rotations[k + 1:]
        out[k] = 0.5 * (energy(psi0, plus, terms) - energy(psi0, minus, terms))
    return out


def dense_hamiltonian(terms, n):
    return sum(c * pauli_ref.dense_pauli(x, z, n) for c, x, z in terms)


def term_texts(terms, n):
    """[(c, x, z)] -> [(c, "X0 Z3 ...")] as Simulator.expectation and energy_and_gradient take them."""
    return [(c, pauli_ref.masks_to_text(x, z, n)) for c, x, z in terms]


def weight(terms):
    return sum(abs(c) for c, _, _ in terms)


# ---- the cases of tests/test_gpu_adjoint.py, as data ---------------------------------------------------------------------------
def geometry_strings(n):
    """(x, z) with the highest x bit at 0, at 1, on either side of the sweeps' thread boundary (7 and 8) and at n - 1, as far as the
    register has these bits, X, Y and Z factors mixed, and one diagonal string (test_gpu_pauli_rot._geometry_strings' rule)."""
    out = []
    for h in sorted({0, 1, 7, 8, n - 1} & set(range(n))):
        x = 1 << h | (1 << (h - 2) if h >= 2 else 0)
        z = (1 << h if h % 2 else 0) | 1 << (h + 1) % n
        out.append((x, z))
    return out + [(0, 0b101101101 & ((1 << n) - 1))]


def random_hamiltonian(n, count, seed, duplicates_of_one_x=0):
    """`count` random strings of every weight with coefficients in [-1, 1], then `duplicates_of_one_x` more that share the first
    string's x (so that one x group of H has several terms, of both parities of ny)."""
    rng = np.random.default_rng(seed)
    terms = [(float(rng.uniform(-1, 1)),) + pauli_ref.random_masks(rng, n, 1 + i % n) for i in range(count)]
    x0 = terms[0][1]
    for _ in range(duplicates_of_one_x):
        terms.append((float(rng.uniform(-1, 1)), x0, int(rng.integers(0, 1 << n))))
    return terms


def every_weight_case(n=13):
    """40 rotations of weights 1..13 plus single-qubit X, Y, Z and the identity; H of 20 random strings plus 6 sharing one x."""
    rng = np.random.default_rng(1300)
    rotations = [(float(rng.uniform(-math.pi, math.pi)),) + pauli_ref.random_masks(rng, n, 1 + i % n) for i in range(40)]
    rotations[7:7] = [(0.9, 1 << 3, 0)]              # X3: through the gate queue forwards, through a sweep backwards
    rotations[19:19] = [(-0.4, 1 << 8, 1 << 8)]      # Y8
    rotations[23:23] = [(1.7, 0, 1 << 12)]           # Z12
    rotations[30:30] = [(0.6, 0, 0)]                 # the identity: a global phase
    return rotations, random_hamiltonian(n, 20, 1301, 6)


def order_case():
    """pauli_rot_ref.ORDER_PAIR (one x, anticommuting) between two other terms, and H on the same qubits."""
    a, b = pauli_rot_ref.ORDER_PAIR
    before, after = (0.5, 0b100, 0b010), (-0.9, 0b1000, 0b0001)
    terms = [(0.7, 0b01, 0b10), (-0.4, 0, 0b11), (0.9, 0b11, 0b01), (0.3, 0b1010, 0b0100), (-0.6, 0b01, 0)]
    return [before, a, b, after], [before, b, a, after], terms


def ansatz_case(n=13, layers=2):
    """A hardware-efficient ansatz from |0...0>: layers of Y rotations on every qubit and ZZ rotations on neighbours; a
    transverse-field Ising chain as H."""
    rng = np.random.default_rng(77)
    rotations = []
    for _ in range(layers):
        rotations += [(float(rng.uniform(-1.5, 1.5)), 1 << q, 1 << q) for q in range(n)]
        rotations += [(float(rng.uniform(-1.5, 1.5)), 0, 0b11 << q) for q in range(n - 1)]
    terms = [(-1.0, 0, 0b11 << q) for q in range(n - 1)] + [(-0.7, 1 << q, 0) for q in range(n)]
    return rotations, terms


def shift_case(n=9):
    rng = np.random.default_rng(900)
    rotations = [(float(rng.uniform(-2, 2)),) + pauli_ref.random_masks(rng, n, 1 + i % n) for i in range(12)]
    return rotations, random_hamiltonian(n, 8, 901, 2), (0, 5, 11)


def sum_cases(n=9):
    """label -> terms of the pauli_sum_into test: one group, several groups, more than 32 terms of one x, none."""
    rng = np.random.default_rng(99)
    x = 0b100100101
    one = [(float(rng.uniform(-1, 1)), x, int(rng.integers(0, 1 << n))) for _ in range(5)]
    many = [(float(rng.uniform(-1, 1)), x, int(rng.integers(0, 1 << n))) for _ in range(70)]
    return {"one_group": one, "several_groups": random_hamiltonian(n, 12, 98, 3) + [(0.5, 0, 0), (0.25, 1, 1)], "long_group": many, "empty": []}
