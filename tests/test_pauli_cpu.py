"""Pauli-string expectation values, the parts that need no GPU: the string parser, the host-side sweep count of
plans.pauli_sweeps, and the numpy checker (tests/pauli_ref.py) the GPU tests lean on, pinned against dense operators."""
import ctypes

import numpy as np
import pytest

import pauli_ref
from gpu_quantum_simulator_amd import pauli_masks, plans


def test_pauli_masks_examples():
    assert pauli_masks("X0", 4) == (1, 0)
    assert pauli_masks("Z3", 4) == (0, 8)
    assert pauli_masks("Y2", 4) == (4, 4)  # Y sets both masks
    assert pauli_masks("X0 Z3 Y17", 18) == (1 | 1 << 17, 8 | 1 << 17)
    assert pauli_masks("x0\tz3  y17\n", 18) == pauli_masks("X0 Z3 Y17", 18)  # case and any whitespace
    assert pauli_masks("", 5) == (0, 0) and pauli_masks("   ", 5) == (0, 0)  # identity
    assert pauli_masks("I2 X1 i0", 3) == (2, 0)  # I is allowed and ignored
    assert pauli_masks("Z39", 40) == (0, 1 << 39)


@pytest.mark.parametrize("text, n", [("X4", 4), ("X0 Z0", 3), ("I1 Y1", 3), ("Q0", 2), ("X", 2), ("X-1", 2), ("X0Z1", 3), ("0X", 2),
                                     ("X1.0", 3)])
def test_pauli_masks_rejects(text, n):
    with pytest.raises(ValueError):
        pauli_masks(text, n)


def test_pauli_masks_round_trip():
    rng = np.random.default_rng(5)
    for n in (1, 2, 7, 30):
        for _ in range(50):
            x, z = pauli_ref.random_masks(rng, n, int(rng.integers(0, n + 1)))
            assert pauli_masks(pauli_ref.masks_to_text(x, z, n), n) == (x, z)


def test_sweep_count_matches_grouping():
    from gpu_quantum_simulator_amd import _lib
    lib = _lib.load()
    K = plans.pauli_terms_per_sweep()
    assert K in (8, 16, 32)
    up = ctypes.POINTER(ctypes.c_uint64)
    rng = np.random.default_rng(11)
    assert plans.ok(plans.pauli_sweeps(None))["sweeps"] == 0
    for trial in range(60):
        distinct = int(rng.integers(1, 9))
        pool = rng.integers(0, 1 << 40, size=distinct, dtype=np.uint64)
        if trial % 3 == 0:
            pool[0] = 0  # a diagonal group
        xs = np.ascontiguousarray(rng.choice(pool, size=int(rng.integers(1, 6 * K))))
        want = sum(-(-int(np.sum(xs == v)) // K) for v in np.unique(xs))
        assert plans.ok(plans.pauli_sweeps(xs.tolist()))["sweeps"] == want, (trial, xs.size, distinct)
    one = np.zeros(3 * K + 1, dtype=np.uint64)
    assert plans.ok(plans.pauli_sweeps(one.tolist()))["sweeps"] == 4
    assert plans.pauli_sweeps(one.tolist(), num_terms=-1) == (_lib.ERR_ARG, {"sweeps": -1})
    assert plans.pauli_sweeps(None, num_terms=3) == (_lib.ERR_ARG, {"sweeps": -1})
    assert lib.qsim_pauli_sweeps(one.ctypes.data_as(up), 3, None) == _lib.ERR_ARG  # raw: NULL for an out-parameter


@pytest.mark.parametrize("n", [1, 2, 3, 5, 8])
def test_checker_equals_dense_operators(n):
    rng = np.random.default_rng(100 + n)
    psi = rng.standard_normal(1 << n) + 1j * rng.standard_normal(1 << n)
    psi /= np.linalg.norm(psi)
    cases = [(0, 0)] + [(1 << q if k != 2 else 0, 1 << q if k else 0) for q in range(n) for k in range(3)]  # I; X, Y, Z on each qubit
    cases += [pauli_ref.random_masks(rng, n, int(rng.integers(1, n + 1))) for _ in range(40 if n < 8 else 12)]
    for x, z in cases:
        dense = np.vdot(psi, pauli_ref.dense_pauli(x, z, n) @ psi)
        assert abs(dense.imag) < 1e-12
        assert abs(pauli_ref.pauli_expectation(psi, x, z) - dense.real) < 1e-12, (n, x, z)
