"""The tests' own checker for adjoint-mode gradients through CONTROLLED Pauli rotations (qsim_controlled_pauli_gradient,
csrc/cadjoint.hip): adjoint_ref's algorithm with controlled_rot_ref's rotations (tests/test_controlled_adjoint_cpu.py pins it against
dense operators and the four-term shift rule), and the cases of tests/test_gpu_controlled_adjoint.py as data.

A rotation is (theta, c, x, z) as in controlled_rot_ref: U = (1 - Pi) + Pi exp(-i theta/2 P), Pi = "every qubit of c is 1",
c & (x | z) == 0.  dU/dtheta = -(i/2) Pi P U, so with |lambda_K> = H |psi_K> and |lambda_(k-1)> = U_k^+ |lambda_k>
    dE/dtheta_k = Im <lambda_k| Pi_k P_k |psi_k>:
the inner product of lambda and P psi restricted to the indices with (j & c) == c.  The generator Pi P / 2 has the eigenvalues
{0, +-1/2}, so the two-term shift rule is WRONG for c != 0; the exact rule takes four energies (shift4_gradient).

The energy bound (a copy of tests/test_gpu_adjoint.py's docstring).  fp64: 1e-10 sum|c_t|.  fp32: the energy is <lambda|psi> in
fp64 of a lambda that was accumulated in fp32: each of the T + 1 roundings of an amplitude of lambda is at most 2^-24 of a partial
sum bounded by sum|c_t| |psi_partner|, so by Cauchy-Schwarz on a unit state |E - E_exact(forward state)| <= (T + 1) 2^-24 sum|c_t|;
the tests assert (T + 2) 2^-24 sum|c_t|.  Against the fp64 checker, which replays the rotations in fp64, the fp32 forward state's
own error comes on top: the rotation tests hold it to f = C max(rel_err(complex64 replay), FLOOR), and it moves <H> by at most
2 f sum|c_t|."""
import functools
import math

import numpy as np

import adjoint_ref
import controlled_rot_ref as crot
import fp32_ref
import pauli_ref
from adjoint_ref import apply_pauli, apply_sum, dense_hamiltonian, random_hamiltonian, term_texts, weight  # noqa: F401
from controlled_rot_ref import (EXHAUSTIVE_SIZES, GATE_N, GATE_TERMS, ORDER_N, ORDER_PAIR, RUN_CONTROLS, RUN_N, SEVERAL_N, SLOT_N, SLOT_TERMS,  # noqa: F401
                                dense_controlled, entries, every_position_terms, exhaustive_terms, mask_of, rand_state, run_terms, several_controls_terms)

TOL = 1e-10


def _inside(size, c):
    j = np.arange(size, dtype=np.uint64)
    return (j & np.uint64(c)) == np.uint64(c)


def gradient(psi0, rotations, terms, dtype=np.complex128, large=False):
    """(E, grad, psi_K) by the adjoint algorithm: states and rotations in `dtype`, every inner product in fp64.  `large`: the same
    arithmetic through the primitives for large registers below."""
    rotate, pauli, mask = (large_rotation, large_pauli, large_inside) if large else (crot.apply_rotation, apply_pauli, _inside)
    psi = np.asarray(psi0, dtype=dtype)
    for theta, c, x, z in rotations:
        psi = rotate(psi, c, x, z, theta, dtype)
    final = psi
    lam = large_sum(psi, terms, dtype) if large else apply_sum(psi, terms, dtype)
    wide = np.complex128
    energy = float(np.vdot(lam.astype(wide), psi.astype(wide)).real)
    grad = np.zeros(len(rotations))
    for k in range(len(rotations) - 1, -1, -1):
        theta, c, x, z = rotations[k]
        inside = mask(psi.size, c)
        if large:  # a product with the 0 / 1 vector instead of a selection: the same terms of the sum
            grad[k] = float(np.vdot(lam.astype(wide), inside * pauli(psi, x, z).astype(wide)).imag)
        else:
            grad[k] = float(np.vdot(lam.astype(wide)[inside], pauli(psi, x, z).astype(wide)[inside]).imag)
        psi = rotate(psi, c, x, z, -theta, dtype)
        lam = rotate(lam, c, x, z, -theta, dtype)
    return energy, grad, final


# ---- the same primitives for large registers (n = 22): sign and subspace vectors as Kronecker products, the partner through a flip of
# ---- axes, no index arrays; tests/test_controlled_adjoint_cpu.py holds them to the BITS of the ones above
@functools.lru_cache(maxsize=16)
def _kron_vector(size, mask, set_value, clear_value):
    """v[j] = product over the set bits q of `mask` of (set_value if bit q of j else clear_value)."""
    out = np.ones(1)
    for q in range(size.bit_length() - 2, -1, -1):
        out = np.kron(out, np.array([clear_value, set_value]) if mask >> q & 1 else np.ones(2))
    return out


@functools.lru_cache(maxsize=4)
def large_inside(size, c):
    return _kron_vector(size, c, 1.0, 0.0) != 0.0


def _partner(psi, x):
    n = psi.size.bit_length() - 1
    axes = [n - 1 - q for q in range(n) if x >> q & 1]
    return np.flip(psi.reshape((2,) * n), axis=axes).reshape(-1) if axes else psi


def large_pauli(psi, x, z):
    s = _kron_vector(psi.size, z, -1.0, 1.0)  # s(i ^ x) = (-1)^ny s(i)
    ny = bin(x & z).count("1")
    return (1j ** (ny % 4) * (-1) ** ny * s * _partner(psi, x)).astype(psi.dtype)


def large_sum(psi, terms, dtype=np.complex128):
    psi = np.asarray(psi, dtype=dtype)
    real = np.float64 if dtype == np.complex128 else np.float32
    out = np.zeros(psi.size, dtype=dtype)
    for c, x, z in terms:
        out = (out + real(c) * large_pauli(psi, x, z)).astype(dtype)
    return out


def large_rotation(psi, c, x, z, theta, dtype=np.complex128):
    """controlled_rot_ref.apply_rotation, operation for operation."""
    psi = np.asarray(psi, dtype=dtype)
    real = np.float64 if dtype == np.complex128 else np.float32
    cs, sn = math.cos(0.5 * theta), math.sin(0.5 * theta)
    ny = bin(x & z).count("1")
    w = (-1j * sn, sn, 1j * sn, -sn)[ny % 4] * (-1) ** ny
    s = _kron_vector(psi.size, z, -1.0, 1.0).astype(real)
    rotated = (real(cs) * psi + dtype(w) * (s * _partner(psi, x))).astype(dtype)
    return np.where(large_inside(psi.size, c), rotated, psi).astype(dtype)


def large_replay(psi, rotations, dtype=np.complex128):
    out = np.asarray(psi, dtype=dtype)
    for theta, c, x, z in rotations:
        out = large_rotation(out, c, x, z, theta, dtype)
    return out


def energy(psi0, rotations, terms):
    """E in fp64 from the replayed state and pauli_ref.pauli_expectation: independent of the adjoint algorithm."""
    psi = crot.replay(psi0, rotations)
    return sum(c * pauli_ref.pauli_expectation(psi, x, z) for c, x, z in terms)


def _shifted(rotations, k, shift):
    theta, c, x, z = rotations[k]
    return rotations[:k] + [(theta + shift, c, x, z)] + rotations[k + 1:]


C_PLUS, C_MINUS = (math.sqrt(2.0) + 1.0) / (4.0 * math.sqrt(2.0)), (math.sqrt(2.0) - 1.0) / (4.0 * math.sqrt(2.0))


def shift4(energy_of_shift):
    """The four-term rule for a generator with eigenvalues {0, +-1/2} from E(theta + shift): exact for every frequency 1/2 and 1."""
    e = energy_of_shift
    return C_PLUS * (e(0.5 * math.pi) - e(-0.5 * math.pi)) - C_MINUS * (e(1.5 * math.pi) - e(-1.5 * math.pi))


def shift4_gradient(psi0, rotations, terms, which=None):
    return {k: shift4(lambda s, k=k: energy(psi0, _shifted(rotations, k, s), terms)) for k in (range(len(rotations)) if which is None else which)}


def shift2_gradient(psi0, rotations, terms, which=None):
    """The two-term rule [E(theta + pi/2) - E(theta - pi/2)] / 2: right without controls, wrong with them."""
    return {k: 0.5 * (energy(psi0, _shifted(rotations, k, 0.5 * math.pi), terms) - energy(psi0, _shifted(rotations, k, -0.5 * math.pi), terms))
            for k in (range(len(rotations)) if which is None else which)}


def dense_gradient(psi0, rotations, terms, n):
    """(E, grad) from dense operators: dE/dtheta_k = 2 Re <psi_K| H U_K ... U_(k+1) [-(i/2) Pi_k P_k U_k] U_(k-1) ... U_1 |psi_0>."""
    H = dense_hamiltonian(terms, n) if terms else np.zeros((1 << n, 1 << n))
    us = [dense_controlled(c, x, z, n, theta) for theta, c, x, z in rotations]
    psi = psi0
    for u in us:
        psi = u @ psi
    grad = np.zeros(len(rotations))
    for k, (theta, c, x, z) in enumerate(rotations):
        v = psi0
        for u in us[:k + 1]:
            v = u @ v
        v = -0.5j * (np.diag(_inside(1 << n, c).astype(np.float64)) @ (pauli_ref.dense_pauli(x, z, n) @ v))
        for u in us[k + 1:]:
            v = u @ v
        grad[k] = 2.0 * np.vdot(psi, H @ v).real
    return float(np.vdot(psi, H @ psi).real), grad


def energy_tol(precision, terms, finals=None):
    """The module docstring's bound; `finals` = (complex64 replay, fp64 replay) of the rotations from the state before the call, as
    gradient returns them, when the energy is compared with the fp64 checker."""
    if precision == 64:
        return TOL * weight(terms)
    forward = fp32_ref.C * max(fp32_ref.rel_err(*finals), fp32_ref.FLOOR) if finals is not None else 0.0
    return ((len(terms) + 2) * 2.0 ** -24 + 2.0 * forward) * weight(terms)


def plan(rotations, terms, n, precision=64, null_controls=False):
    """(adjoint sweeps, sum sweeps, units visited) of [(theta, c, x, z)] and H on n qubits: plans.controlled_gradient_plan."""
    from gpu_quantum_simulator_amd import plans
    p = plans.ok(plans.controlled_gradient_plan(None if null_controls else [r[1] for r in rotations], [r[2] for r in rotations],
                                                [x for _, x, _ in terms], n, precision))
    return p["adjoint_sweeps"], p["sum_sweeps"], p["units_visited"]


def weighted_state(n, seed, c, outside=0.1):
    """A random state whose amplitudes outside the subspace of c are scaled by `outside`, renormalised: deep controls keep gradients
    well above rounding."""
    psi = rand_state(n, seed)
    psi = np.where(_inside(psi.size, c), psi, outside * psi)
    return (psi / np.linalg.norm(psi)).astype(np.complex128)


# ---- the cases of tests/test_gpu_controlled_adjoint.py, as data: (n, start state, [(theta, c, x, z)], [(coefficient, x, z)]) --------
def exhaustive_case(n):
    return n, rand_state(n, 50 + n), exhaustive_terms(n), random_hamiltonian(n, 6, 300 + n, 2)


POSITION_N = 13


def position_rotations(n=POSITION_N):
    """For every q: control {q} on "Y(q+1) Z(q+3) X(q+5)" and on "Z(q+2) Z(q+7)" (qubit numbers mod n): the control below the lane
    bits, on either side of the thread boundary (unit bits 7 / 8), in the trip bits and at n - 1; the highest x bit above and below it."""
    out = []
    for q in range(n):
        a, b, d = (q + 1) % n, (q + 3) % n, (q + 5) % n
        out.append((0.7, 1 << q, 1 << a | 1 << d, 1 << a | 1 << b))
        out.append((-1.1, 1 << q, 0, 1 << (q + 2) % n | 1 << (q + 7) % n))
    return out


def position_case(n=POSITION_N):
    return n, rand_state(n, 131), position_rotations(n), random_hamiltonian(n, 8, 1310, 2)


def one_call_position_case():
    """controlled_rot_ref.every_position_terms as ONE rotation list: the highest x bit below and above every control position."""
    return 13, rand_state(13, 132), every_position_terms(13), random_hamiltonian(13, 8, 1320, 2)


def gate_case():
    """One control on a single X or Y: the 4x4 of the gate queue forwards, a controlled sweep backwards."""
    return GATE_N, rand_state(GATE_N, 7), GATE_TERMS, random_hamiltonian(GATE_N, 6, 701, 2)


def slot_case():
    return SLOT_N, rand_state(SLOT_N, 10), SLOT_TERMS, random_hamiltonian(SLOT_N, 8, 1000, 2)


def several_case():
    return SEVERAL_N, rand_state(SEVERAL_N, 1300), several_controls_terms(), random_hamiltonian(SEVERAL_N, 10, 1302, 3)


def run_cases(K):
    """label -> (rotations, sweeps): one control mask, cut into pieces of K; alternating masks, every term a sweep of its own."""
    out = {f"run_{c:#x}": (run_terms(K, (c,)), -(-(3 * K + 5) // K)) for c in RUN_CONTROLS}
    out["run_alternating"] = (run_terms(K, RUN_CONTROLS), 3 * K + 5)
    return out


def run_hamiltonian():
    return random_hamiltonian(RUN_N, 10, 1200, 2)


def order_case():
    """controlled_rot_ref.ORDER_PAIR ("X0 X1" and "Y0 X1" under qubit 3) between two other terms; H as in adjoint_ref.order_case."""
    a, b = ORDER_PAIR
    before, after = (0.5, 1 << 5, 0b100, 0b010), (-0.9, 0, 0b1000, 0b0001)
    terms = adjoint_ref.order_case()[2]
    return [before, a, b, after], [before, b, a, after], terms


ANSATZ_N = 13
ANSATZ_PHASE = (0.6, (2, 7, 11))  # phi and the qubits of the multi-controlled phase


def ansatz_case(n=ANSATZ_N, layers=2):
    """From |0...0>: layers of Y rotations on every qubit and CRY(q -> q + 1), and one multi-controlled phase; the transverse-field
    Ising chain of adjoint_ref.ansatz_case as H."""
    rng = np.random.default_rng(78)
    rotations = []
    for layer in range(layers):
        rotations += [(float(rng.uniform(0.4, 1.5)), 0, 1 << q, 1 << q) for q in range(n)]
        rotations += [(float(rng.uniform(-1.5, 1.5)), 1 << q, 1 << (q + 1), 1 << (q + 1)) for q in range(n - 1)]
        if layer == 0:
            rotations.append((-2.0 * ANSATZ_PHASE[0], mask_of(ANSATZ_PHASE[1]), 0, 0))
    return n, rotations, adjoint_ref.ansatz_case(n)[1]


SHIFT_N = 9


def shift_case(n=SHIFT_N):
    """Twelve rotations, every third one uncontrolled, and the three controlled components the device's four-term rule checks."""
    rng = np.random.default_rng(910)
    rotations = []
    for i in range(12):
        c = mask_of(int(q) for q in rng.choice(n, size=i % 3, replace=False))
        rotations.append((float(rng.uniform(-2, 2)), c) + crot.random_string(rng, n, c, 1 + i % 4))
    which = (1, 5, 10)
    assert all(rotations[k][1] for k in which)
    return rotations, random_hamiltonian(n, 8, 911, 2), which


BITS_N = 13


def uncontrolled_case(n=BITS_N):
    rotations, terms = adjoint_ref.every_weight_case(n)
    return [(theta, 0, x, z) for theta, x, z in rotations], terms


def under_qubit_11_case(n=BITS_N):
    """Every rotation controlled on qubit 11, some on further qubits: amplitudes with bit 11 clear are never written."""
    rng = np.random.default_rng(1311)
    rotations = []
    for i in range(16):
        c = 1 << 11 | mask_of(int(q) for q in rng.choice(11, size=i % 3, replace=False))
        rotations.append((float(rng.uniform(-2, 2)), c) + crot.random_string(rng, n, c, 1 + i % 5))
    rotations += [(0.9, 1 << 11, 1 << 3, 0), (0.4, 1 << 11, 0, 0)]  # a 4x4 of the gate queue forwards; the controlled identity
    return rotations, random_hamiltonian(n, 8, 1312, 2)


LOOP_N = 22


def loop_case(n=LOOP_N):
    """A paired and a diagonal rotation under control {n - 1} and then under control {2}, and a 3-term H, on a register whose
    controlled sweeps loop."""
    a, b, d = 3, 9, n - 2
    rotations = []
    for control in (n - 1, 2):
        rotations += [(0.7 if control == 2 else -0.5, 1 << control, 1 << a | 1 << d, 1 << a | 1 << b), (1.1 if control == 2 else 0.3, 1 << control, 0, 1 << b | 1 << d)]
    terms = [(0.8, 1 << a, 1 << b), (-0.6, 0, 1 << d | 1 << (n - 1)), (0.5, 1 << b | 1 << 2, 1 << b)]
    return n, rotations, terms


@functools.lru_cache(maxsize=None)
def loop_state(n=LOOP_N):
    """A product of random one-qubit states plus a random vector of a third of its norm: on a random state of 2^22 amplitudes every
    gradient would be of the order 2^-11, and a product state alone is too regular."""
    rng = np.random.default_rng(221)
    psi = np.ones(1, dtype=np.complex128)
    for _ in range(n):
        one = rng.standard_normal(2) + 1j * rng.standard_normal(2)
        psi = np.kron(one / np.linalg.norm(one), psi)
    psi = psi + rand_state(n, 220) / 3.0
    return (psi / np.linalg.norm(psi)).astype(np.complex128)


def fp32_cases(K):
    """(label, start state, rotations, terms) of every gradient the GPU tests hold an fp32 state to, from a state known beforehand."""
    for n in EXHAUSTIVE_SIZES:
        _, start, rotations, terms = exhaustive_case(n)
        yield f"exhaustive_n{n}", start, rotations, terms
    _, start, rotations, terms = position_case()
    for k, rot in enumerate(rotations):
        yield f"position_{k}", start, [rot], terms
    yield ("slots",) + slot_case()[1:]
    yield ("every_position",) + one_call_position_case()[1:]
    yield ("gates",) + gate_case()[1:]
    yield ("several",) + several_case()[1:]
    for label, (rotations, _) in run_cases(K).items():
        yield label, rand_state(RUN_N, 12), rotations, run_hamiltonian()
    ab, ba, terms = order_case()
    yield "order_ab", rand_state(ORDER_N, 6), ab, terms
    yield "order_ba", rand_state(ORDER_N, 6), ba, terms
    n, rotations, terms = ansatz_case()
    ket0 = np.zeros(1 << n, dtype=np.complex128)
    ket0[0] = 1.0
    yield "ansatz", ket0, rotations, terms
    rotations, terms, _ = shift_case()
    yield "shift4", rand_state(SHIFT_N, 99), rotations, terms
    rotations, terms = under_qubit_11_case()
    yield "under_qubit_11", weighted_state(BITS_N, 13, 1 << 11), rotations, terms
