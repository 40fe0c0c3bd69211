"""Pins tests/adjoint_ref.py, the checker of the GPU gradient tests, on the CPU: against the exact shift rule built from
pauli_rot_ref.replay and pauli_ref.pauli_expectation, and against dense operators; and checks the host-only sweep plan of
qsim_pauli_gradient (plans.pauli_gradient_plan)."""
import ctypes
import math

import numpy as np
import pytest

import adjoint_ref as ref
import fp32_ref
import pauli_ref
import pauli_rot_ref
from gpu_quantum_simulator_amd import _lib, plans

UP = ctypes.POINTER(ctypes.c_uint64)


def _small_case(n, seed, rotations=9, terms=6):
    rng = np.random.default_rng(seed)
    rots = [(float(rng.uniform(-3, 3)),) + pauli_ref.random_masks(rng, n, 1 + i % n) for i in range(rotations)]
    rots += [(0.8, 0, 0), (0.3, rots[0][1], rots[0][2] ^ 1)]  # the identity, and a second term on the first one's x
    return pauli_rot_ref.rand_state(n, seed), rots, ref.random_hamiltonian(n, terms, seed + 1, 2)


@pytest.mark.parametrize("n", [1, 2, 3, 5])
def test_adjoint_matches_the_shift_rule(n):
    psi0, rotations, terms = _small_case(n, 50 + n)
    energy, grad, final = ref.gradient(psi0, rotations, terms)
    assert abs(energy - ref.energy(psi0, rotations, terms)) < 1e-12
    assert np.max(np.abs(final - pauli_rot_ref.replay(psi0, rotations))) == 0
    shift = ref.shift_gradient(psi0, rotations, terms)
    worst = max(abs(grad[k] - shift[k]) for k in shift)
    print(f"n={n}: adjoint vs shift rule, worst {worst:.3e}")
    assert worst < 1e-12
    assert np.max(np.abs(grad)) > 1e-3 and abs(grad[len(rotations) - 2]) < 1e-12  # the identity's derivative is zero


@pytest.mark.parametrize("n", [1, 2, 4])
def test_adjoint_matches_dense_operators(n):
    psi0, rotations, terms = _small_case(n, 70 + n)
    H = ref.dense_hamiltonian(terms, n)
    assert np.max(np.abs(ref.apply_sum(psi0, terms) - H @ psi0)) < 1e-13
    for _, x, z in rotations:
        assert np.max(np.abs(ref.apply_pauli(psi0, x, z) - pauli_ref.dense_pauli(x, z, n) @ psi0)) < 1e-15
    us = [pauli_rot_ref.dense_rotation(x, z, n, theta) for theta, x, z in rotations]
    psi = psi0
    for u in us:
        psi = u @ psi
    energy, grad, _ = ref.gradient(psi0, rotations, terms)
    assert abs(energy - np.vdot(psi, H @ psi).real) < 1e-12
    for k, (theta, x, z) in enumerate(rotations):  # dE/dtheta_k = 2 Re <psi_K| H U_K ... U_(k+1) (-i/2 P_k) U_k ... U_1 |psi_0>
        v = psi0
        for u in us[:k + 1]:
            v = u @ v
        v = -0.5j * (pauli_ref.dense_pauli(x, z, n) @ v)
        for u in us[k + 1:]:
            v = u @ v
        assert abs(grad[k] - 2.0 * np.vdot(psi, H @ v).real) < 1e-12


def test_fp32_checker_stays_under_the_reference_cap():
    """The complex64 run of the checker, which the fp32 GPU tests use as ref32, is itself within fp32_ref.REF_CAP of the fp64 one."""
    psi0, rotations, terms = _small_case(5, 90)
    psi0 = psi0.astype(np.complex64).astype(np.complex128)
    e64, g64, _ = ref.gradient(psi0, rotations, terms)
    e32, g32, _ = ref.gradient(psi0.astype(np.complex64), rotations, terms, np.complex64)
    assert 0 < fp32_ref.rel_err(g32, g64) < fp32_ref.REF_CAP and abs(e32 - e64) < 1e-5 * ref.weight(terms)


def _plan(rot_x, ham_x):
    p = plans.ok(plans.pauli_gradient_plan(rot_x, ham_x))
    return p["adjoint_sweeps"], p["sum_sweeps"]


def test_gradient_plan():
    lib = _lib.load()
    K, KH = plans.pauli_rotations_per_sweep(), plans.pauli_terms_per_sweep()
    assert _plan([], []) == (0, 0)
    # maximal runs of consecutive equal x: single X / Y terms are sweeps too; equal x apart from each other do not share
    assert _plan([1, 1, 2, 1, 0, 0, 0], []) == (4, 0)
    # a run is cut into pieces of K
    assert _plan([5] * (3 * K + 5) + [0] * K + [7] * (K + 1), []) == (4 + 1 + 2, 0)
    # H is grouped by x wherever the terms stand, every group cut into pieces of the expectation sweeps' K
    assert _plan([], [3, 0, 3, 9, 0, 3]) == (0, 3)
    assert _plan([4], [6] * (2 * KH + 1) + [1]) == (1, 4)
    diag, paired = pauli_rot_ref.long_run_rotations(K)
    assert _plan([x for _, x, _ in diag + paired], [0]) == (2 * math.ceil((3 * K + 5) / K), 1)
    a, s = ctypes.c_long(), ctypes.c_long()
    ok = np.array([1, 2], dtype=np.uint64).ctypes.data_as(UP)
    for rot_x, ham_x, counts in (([1, 2], [1, 2], dict(num_rot=-1)), ([1, 2], [1, 2], dict(num_ham=-1)), (None, [1, 2], dict(num_rot=2)),
                                 ([1, 2], None, dict(num_ham=2))):
        assert plans.pauli_gradient_plan(rot_x, ham_x, **counts)[0] == _lib.ERR_ARG
    for args in ((ok, 2, ok, 2, None, ctypes.byref(s)), (ok, 2, ok, 2, ctypes.byref(a), None)):
        assert lib.qsim_pauli_gradient_plan(*args) == _lib.ERR_ARG  # raw: NULL for an out-parameter
