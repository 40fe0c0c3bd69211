"""Pauli-string rotations, the parts that need no GPU: the numpy checker (tests/pauli_rot_ref.py) pinned against dense
operators, the routing plan of plans.pauli_rotation_plan, the fp32 legality of every sequence the GPU tests run, and the list
Simulator.evolve hands to the C call."""
import ctypes
import math

import numpy as np
import pytest

import fp32_ref
import pauli_ref
import pauli_rot_ref
from gpu_quantum_simulator_amd import _lib, pauli_masks, trotter_rotations, plans

UP = ctypes.POINTER(ctypes.c_uint64)


def test_checker_matches_dense_operators():
    rng = np.random.default_rng(3)
    worst = 0.0
    for n in range(1, 7):
        psi = pauli_rot_ref.rand_state(n, n)
        for weight in range(0, n + 1):
            for _ in range(6):
                x, z = pauli_ref.random_masks(rng, n, weight)
                theta = float(rng.uniform(-2 * math.pi, 2 * math.pi))
                want = pauli_rot_ref.dense_rotation(x, z, n, theta) @ psi
                worst = max(worst, float(np.max(np.abs(pauli_rot_ref.apply_rotation(psi, x, z, theta) - want))))
                got32 = pauli_rot_ref.apply_rotation(psi.astype(np.complex64), x, z, theta, np.complex64)
                assert got32.dtype == np.complex64 and np.max(np.abs(got32 - want)) < 1e-6
    assert worst < 1e-13, worst


def test_checker_replay_is_a_product_in_order():
    n = 4
    psi = pauli_rot_ref.rand_state(n, 44)
    a, b = pauli_rot_ref.ORDER_PAIR
    ab = pauli_rot_ref.replay(psi, [a, b])
    want = pauli_rot_ref.dense_rotation(b[1], b[2], n, b[0]) @ (pauli_rot_ref.dense_rotation(a[1], a[2], n, a[0]) @ psi)
    assert np.max(np.abs(ab - want)) < 1e-13
    assert np.max(np.abs(ab - pauli_rot_ref.replay(psi, [b, a]))) > 1e-2  # they anticommute: the order shows


def _plan(rotations):
    p = plans.ok(plans.pauli_rotation_plan([x for _, x, _ in rotations], [z for _, _, z in rotations]))
    return p["sweeps"], p["queued_as_gates"]


def test_routing_plan():
    lib = _lib.load()
    K = plans.pauli_rotations_per_sweep()
    assert K == 32
    rng = np.random.default_rng(70)
    all_z = [(0.1, 0, int(z)) for z in rng.integers(1, 1 << 20, size=70)]
    assert _plan(all_z) == (-(-70 // K), 0)
    assert _plan([]) == (0, 0)
    alternating = [(0.1, 0b110 if i % 2 else 0b011, int(rng.integers(0, 8))) for i in range(12)]
    assert _plan(alternating) == (12, 0)  # no reordering: one sweep per term
    singles = [(0.1, 1 << 3, 0), (0.1, 1 << 5, 1 << 5), (0.1, 1, 0)]  # X3, Y5, X0
    assert _plan(singles) == (0, 3)
    assert _plan([(0.1, 0, 1 << 4)]) == (1, 0)  # a single Z is a sweep term
    assert _plan([(0.1, 1 << 3, 1 << 4)]) == (1, 0)  # X3 Z4 is not a single-qubit term
    with_identity = all_z[:10] + [(0.3, 0, 0)] + all_z[10:20]
    assert _plan(with_identity) == (1, 0)  # the identity joins the diagonal run
    assert _plan([(0.3, 0, 0)]) == (1, 0)
    # a queued gate between two sweep terms with one x cuts the run: the order is the caller's
    assert _plan([(0.1, 0b11, 0), (0.1, 0b100, 0), (0.1, 0b11, 1)]) == (2, 1)
    assert _plan([(0.1, 0b11, 0), (0.1, 0b11, 1)]) == (1, 0)
    diag, paired = pauli_rot_ref.long_run_rotations(K)
    assert _plan(diag + paired) == (2 * -(-(3 * K + 5) // K), 0)
    # errors
    ok = np.array([1, 2], dtype=np.uint64).ctypes.data_as(UP)
    s, g = ctypes.c_long(), ctypes.c_long()
    assert plans.pauli_rotation_plan([1, 2], [1, 2], num_terms=-1)[0] == _lib.ERR_ARG
    assert b"negative" in lib.qsim_last_error()
    for masks in ((None, [1, 2]), ([1, 2], None)):
        assert plans.pauli_rotation_plan(*masks, num_terms=2)[0] == _lib.ERR_ARG
        assert b"NULL" in lib.qsim_last_error()
    for args in ((ok, ok, 2, None, ctypes.byref(g)), (ok, ok, 2, ctypes.byref(s), None)):
        assert lib.qsim_pauli_rotation_plan(*args) == _lib.ERR_ARG  # raw: NULL for an out-parameter
        assert b"NULL" in lib.qsim_last_error()


def test_fp32_sequences_are_legal():
    K = plans.pauli_rotations_per_sweep()
    labels = []
    for label, n, start, rotations in pauli_rot_ref.fp32_sequences(K):
        start32 = start.astype(np.complex64)
        want = pauli_rot_ref.replay(start32.astype(np.complex128), rotations)
        ref32 = pauli_rot_ref.replay(start32, rotations, np.complex64)
        assert ref32.dtype == np.complex64
        err = fp32_ref.rel_err(ref32, want)
        print(f"{label}: {len(rotations)} rotations, rel_err(ref32) = {err:.3e}")
        assert err <= fp32_ref.REF_CAP, (label, err)
        labels.append(label)
    assert len(labels) == len(set(labels)) >= 18


def test_trotter_rotation_lists():
    terms = [(0.5, "Z0 Z1"), (-1.25, "X0"), (2, "Y1 Z2")]
    one = trotter_rotations(terms, 0.6, steps=1, order=1)
    assert one == [(2 * 0.5 * 0.6, "Z0 Z1"), (2 * -1.25 * 0.6, "X0"), (2 * 2.0 * 0.6, "Y1 Z2")]
    three = trotter_rotations(terms, 0.6, steps=3, order=1)
    assert len(three) == 9 and three[:3] == three[3:6] == three[6:]
    assert [t for _, t in three[:3]] == ["Z0 Z1", "X0", "Y1 Z2"]
    assert all(abs(th - 2 * c * 0.2) < 1e-15 for (th, _), (c, _) in zip(three, terms))
    sym = trotter_rotations(terms, 0.6, steps=2, order=2)
    assert len(sym) == 12 and sym[:6] == sym[6:]
    assert [t for _, t in sym[:6]] == ["Z0 Z1", "X0", "Y1 Z2", "Y1 Z2", "X0", "Z0 Z1"]
    assert all(abs(th - c * 0.3) < 1e-15 for (th, _), (c, _) in zip(sym[:3], terms))  # half a step each: theta = 2 c dt / 2
    assert trotter_rotations(iter(terms), 1.0) == trotter_rotations(terms, 1.0, 1, 1)
    assert trotter_rotations([(np.float64(0.5), "Z0")], 1.0) == [(1.0, "Z0")]
    assert trotter_rotations([], 1.0, 4, 2) == []
    for bad in ({"order": 3}, {"order": 0}, {"steps": 0}, {"steps": 1.5}):
        with pytest.raises(ValueError):
            trotter_rotations(terms, 0.6, **bad)
    for coeff in (1j, 1 + 0j, np.complex128(2)):
        with pytest.raises(ValueError, match="complex"):
            trotter_rotations([(coeff, "Z0")], 0.6)


def test_product_formula_orders_on_the_checker():
    """Order 2 beats order 1 on the Ising chain, and both approach exp(-iHt): the lists mean what they say."""
    n = 4
    terms = pauli_rot_ref.ising_terms(n)
    H = sum(c * pauli_ref.dense_pauli(*pauli_masks(t, n), n) for c, t in terms)
    evals, evecs = np.linalg.eigh(H)
    psi = pauli_rot_ref.rand_state(n, 9)
    exact = evecs @ (np.exp(-1j * evals * 0.5) * (evecs.conj().T @ psi))
    err = {}
    for order in (1, 2):
        rots = pauli_rot_ref.masks_of(trotter_rotations(terms, 0.5, 8, order), n)
        err[order] = float(np.linalg.norm(pauli_rot_ref.replay(psi, rots) - exact))
    assert err[2] < err[1] / 5 and err[1] < 0.05, err
