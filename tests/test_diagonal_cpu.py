"""Whole-register diagonal operators from a table, checked on the CPU: the checker of tests/test_gpu_diagonal.py (diagonal_ref) against
dense operators built with np.kron and against pauli_rot_ref's Z rotations, the host-only plan call (plans.diagonal_plan) against its
rules, the argument refusals that need no device, and Diagonal.from_terms refusing X and Y before anything touches a device."""
from ctypes import byref, c_double, c_int, c_long, c_uint64, c_void_p

import numpy as np
import pytest

import diagonal_ref
import pauli_ref
import pauli_rot_ref
from gpu_quantum_simulator_amd import _lib, plans
from pauli_rot_ref import rand_state

NEW_NAMES = ("qsim_diagonal_create", "qsim_diagonal_create_external", "qsim_diagonal_destroy", "qsim_diagonal_num_qubits",
             "qsim_diagonal_device_ptr", "qsim_diagonal_add_terms", "qsim_diagonal_write", "qsim_diagonal_read", "qsim_diagonal_extrema",
             "qsim_apply_diagonal_phase", "qsim_expect_diagonal", "qsim_diagonal_sweeps_launched", "qsim_diagonal_plan")  # census of the signature table


def _terms(n, count, seed):
    rng = np.random.default_rng(seed)
    return [(float(rng.uniform(-1, 1)), int(rng.integers(0, 1 << n))) for _ in range(count)]


def test_signatures_and_exports_have_the_new_names():
    import gpu_quantum_simulator_amd as pkg
    lib = _lib.load()
    for name in NEW_NAMES:
        assert name in _lib.SIGNATURES and hasattr(lib, name)
    assert "Diagonal" in pkg.__all__ and pkg.Diagonal.__name__ == "Diagonal"
    assert not hasattr(pkg.Cluster, "apply_diagonal_phase") and not hasattr(pkg.Cluster, "expectation_diagonal")


# ---- the checker ----------------------------------------------------------------------------------------------------------------------
def test_signs_are_the_parity_of_the_masked_index():
    rng = np.random.default_rng(49)
    for n in (0, 1, 5, 11):
        i = np.arange(1 << n, dtype=np.uint64)
        for z in [0, (1 << n) - 1] + [int(rng.integers(0, 1 << n)) for _ in range(6)]:
            assert np.array_equal(diagonal_ref.signs(n, z), 1.0 - 2.0 * pauli_ref._parity(i & np.uint64(z)))


def test_table_is_the_diagonal_of_the_dense_operator():
    for n in range(0, 7):
        terms = _terms(n, 9, 50 + n) + [(0.25, 0)]   # z == 0: a constant
        dense = sum(c * pauli_ref.dense_pauli(0, z, n) for c, z in terms)
        assert np.count_nonzero(dense - np.diag(np.diag(dense))) == 0
        got = diagonal_ref.table_from_terms(n, terms)
        assert np.max(np.abs(got - np.diag(dense).real)) < 1e-14
        # on top of a start table, and the order of the terms is the order of the additions
        start = np.random.default_rng(n).standard_normal(1 << n)
        assert np.array_equal(diagonal_ref.table_from_terms(n, terms, start), diagonal_ref.table_from_terms(n, terms[5:], diagonal_ref.table_from_terms(n, terms[:5], start)))


def test_phase_is_the_product_of_z_rotations():
    """exp(-i gamma D) for D = sum c_k P_k equals the rotations exp(-i theta_k/2 P_k) with theta_k = 2 gamma c_k."""
    gamma = 0.73
    for n in range(0, 7):
        terms = _terms(n, 7, 60 + n)
        psi = rand_state(n, 70 + n)
        want = pauli_rot_ref.replay(psi, [(2.0 * gamma * c, 0, z) for c, z in terms])
        got = diagonal_ref.apply_phase(psi, diagonal_ref.table_from_terms(n, terms), gamma)
        assert np.max(np.abs(got - want)) < 1e-12
        got32 = diagonal_ref.apply_phase(psi, diagonal_ref.table_from_terms(n, terms), gamma, dtype=np.complex64)
        assert got32.dtype == np.complex64 and np.max(np.abs(got32 - want)) < 1e-6


def test_moments_and_extrema_of_the_checker():
    n = 5
    terms = _terms(n, 6, 80)
    d = diagonal_ref.table_from_terms(n, terms)
    psi = rand_state(n, 81)
    dense = sum(c * pauli_ref.dense_pauli(0, z, n) for c, z in terms)
    mean, second = diagonal_ref.moments(psi, d)
    assert abs(mean - np.vdot(psi, dense @ psi).real) < 1e-13 and abs(second - np.vdot(psi, dense @ dense @ psi).real) < 1e-13
    assert abs(mean - sum(c * pauli_ref.pauli_expectation(psi, 0, z) for c, z in terms)) < 1e-13
    ties = np.array([3.0, -2.0, 5.0, -2.0, 5.0, 0.0, -2.0, 5.0])
    assert diagonal_ref.extrema(ties) == {"min": -2.0, "argmin": 1, "max": 5.0, "argmax": 2}


# ---- the plan -------------------------------------------------------------------------------------------------------------------------
def _model(n, precision):
    """The plan's rules, restated: an item is two amplitudes; 3 items per thread and trip in fp64 and 4 in fp32; workgroups of 256
    threads, at most 2048 for the phase sweep and 1024 for the expectation sweep; fewer than 64 items: the plain path, one trip."""
    items = max(1, (1 << n) >> 1)
    per = 3 if precision == 64 else 4
    blocks = -(-items // 256)
    plain = items < 64
    return dict(items=items, items_per_trip_phase=per, items_per_trip_expect=per, trips_at_cap_phase=1 if plain else -(-blocks // (per * 2048)),
                trips_at_cap_expect=1 if plain else -(-blocks // (per * 1024)))


@pytest.mark.parametrize("precision", [64, 32])
def test_plan(precision):
    loop = diagonal_ref.loop_n(precision)
    for n in (0, 1, 2, 9, loop - 1, loop, 30, 40):
        assert diagonal_ref.plan(n, precision) == _model(n, precision), n
    assert diagonal_ref.plan(0, precision)["items"] == 1 and diagonal_ref.plan(1, precision)["items"] == 1 and diagonal_ref.plan(2, precision)["items"] == 2
    assert diagonal_ref.plan(9, precision)["trips_at_cap_phase"] == 1 and diagonal_ref.plan(9, precision)["trips_at_cap_expect"] == 1
    at = diagonal_ref.plan(loop, precision)
    assert at["trips_at_cap_phase"] > 1 and at["trips_at_cap_expect"] > 1 and 20 <= loop <= 24
    assert diagonal_ref.plan(loop - 1, precision)["trips_at_cap_phase"] == 1   # the smallest such size


def test_plan_refusals():
    lib = _lib.load()
    items, a, b, c, d = c_uint64(), c_int(), c_int(), c_long(), c_long()
    ok = (byref(items), byref(a), byref(b), byref(c), byref(d))
    assert plans.diagonal_plan(9, 64)[0] == _lib.QSIM_OK
    for n, bits in ((-1, 64), (41, 64), (9, 16), (9, 0)):
        assert plans.diagonal_plan(n, bits)[0] == _lib.ERR_ARG
    for missing in range(5):
        args = [None if i == missing else p for i, p in enumerate(ok)]
        assert lib.qsim_diagonal_plan(9, 64, *args) == _lib.ERR_ARG  # raw: NULL for an out-parameter
        assert b"NULL" in lib.qsim_last_error()


# ---- refusals that need no device -------------------------------------------------------------------------------------------------------
def test_refusals_without_a_device():
    lib = _lib.load()
    h = c_void_p()
    assert lib.qsim_diagonal_create(None, 3, 0) == _lib.ERR_ARG
    for n in (-1, 41):
        assert lib.qsim_diagonal_create(byref(h), n, 0) == _lib.ERR_ARG and not h
    assert lib.qsim_diagonal_create_external(byref(h), 3, 0, None) == _lib.ERR_ARG and not h
    assert lib.qsim_diagonal_create_external(byref(h), 3, 0, c_void_p(4096 + 8)) == _lib.ERR_ARG and not h   # not aligned to 16 bytes
    z, co, x = c_uint64(0), c_double(0.0), c_double(0.0)
    assert lib.qsim_diagonal_add_terms(None, byref(z), byref(co), 1) == _lib.ERR_ARG
    assert lib.qsim_diagonal_write(None, 0, 1, byref(x)) == _lib.ERR_ARG
    assert lib.qsim_diagonal_read(None, 0, 1, byref(x)) == _lib.ERR_ARG
    idx = c_uint64()
    assert lib.qsim_diagonal_extrema(None, byref(x), byref(idx), byref(x), byref(idx)) == _lib.ERR_ARG
    assert lib.qsim_apply_diagonal_phase(None, None, 0.5) == _lib.ERR_ARG
    out = (c_double * 2)()
    assert lib.qsim_expect_diagonal(None, None, out) == _lib.ERR_ARG
    assert lib.qsim_diagonal_num_qubits(None) == -1 and not lib.qsim_diagonal_device_ptr(None)
    lib.qsim_diagonal_destroy(None)
    assert isinstance(plans.sweeps_launched("diagonal"), int)


def test_from_terms_refuses_x_and_y_before_touching_a_device(monkeypatch):
    from gpu_quantum_simulator_amd import Diagonal, simulator

    def no_library():
        raise AssertionError("the library was loaded")

    monkeypatch.setattr(simulator._lib, "load", no_library)
    for bad in ("X0", "Z1 Y2", "z0 x3"):
        with pytest.raises(ValueError, match="X or Y"):
            Diagonal.from_terms(4, [(1.0, "Z0 Z1"), (0.5, bad)])
    with pytest.raises(ValueError, match="complex"):
        Diagonal.from_terms(4, [(1.0 + 1j, "Z0")])
    with pytest.raises(ValueError, match="outside"):
        Diagonal.from_terms(4, [(1.0, "Z4")])
