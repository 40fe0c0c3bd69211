"""Reduced density matrices of 6 to 10 qubits, checked on the CPU: the numpy restatement of the blocked R R^T (tests/subsystem_ref.py)
against the checker density_ref.reduced_density, and the host-only plan call (plans.subsystem_density_plan) against the restatement's
geometry."""
import ctypes
from ctypes import byref, c_int, c_long, c_uint64

import numpy as np
import pytest

import density_ref
import subsystem_ref
from gpu_quantum_simulator_amd import _lib, plans
from pauli_rot_ref import rand_state

NEW_NAMES = ("qsim_subsystem_density", "qsim_subsystem_density_max_qubits", "qsim_subsystem_density_plan", "qsim_subsystem_sweeps_launched")  # census of the signature table
MODEL_KEYS = {"trips_per_workgroup": "trips"}  # header name -> subsystem_ref.plan's key


def subsets(n, k):
    """low, high, and one spread subset (an even spacing over the register, which holds qubit 0 or not as it falls)"""
    spread = sorted({(j * (n - 1)) // max(k - 1, 1) for j in range(k)})
    free = [q for q in range(n) if q not in spread]
    spread = sorted(spread + free[:k - len(spread)])
    return [list(range(k)), list(range(n - k, n)), spread]


def orders(qs, seed):
    return [qs[::-1], [int(q) for q in np.random.default_rng(seed).permutation(qs)]]


def test_signatures_have_the_new_names():
    for name in NEW_NAMES:
        assert name in _lib.SIGNATURES
    assert plans.subsystem_density_max_qubits() == 10
    assert plans.reduced_density_max_qubits() == 5            # the one-wave call keeps its own


@pytest.mark.parametrize("f32", [False, True])
@pytest.mark.parametrize("n", [8, 9, 10, 11, 12])
def test_restatement_matches_the_checker(n, f32):
    psi = rand_state(n, 470 + n)
    for k in range(6, min(n, 10) + 1):
        for qs in subsets(n, k):
            for order in orders(qs, 16 * n + k):
                got, units = subsystem_ref.emulate(psi, order, f32)
                want = density_ref.reduced_density(psi, order)
                assert np.max(np.abs(got - want)) < 1e-13, (n, order)
                assert np.array_equal(got, got.conj().T) and not np.any(np.imag(np.diagonal(got)))
                assert units == subsystem_ref.plan(order, n, f32)["units_read"], (n, order)


@pytest.mark.parametrize("bits", [64, 32])
def test_plan_call_matches_the_restatement(bits):
    for n in list(range(0, 15)) + [18, 22, 23, 30, 34, 40]:
        for k in range(0, min(n, 10) + 1):
            for qs in subsets(n, k):
                rc, got = plans.subsystem_density_plan(qs[::-1], n, bits)
                want = subsystem_ref.plan(qs[::-1], n, bits == 32)
                assert rc == _lib.QSIM_OK, (n, qs)
                assert got == {key: want[MODEL_KEYS.get(key, key)] for key in got}, (n, qs, got, want)
                assert got["path"] == (2 if k < 6 else 1 if n - k >= 2 else 0)
                if got["path"] == 1:
                    assert got["block_rows"] == 128 and got["upper_blocks"] == (1 << (k - 6)) * ((1 << (k - 6)) + 1) // 2
                    assert got["slices"] * got["trips_per_workgroup"] * min(32, 1 << (n - k)) == 1 << (n - k)  # every environment in one slice


def test_plan_is_a_function_of_the_shape_alone():
    """The slices and blocks do not look at a device: the plan call opens none, and the sweep runs what it says."""
    assert plans.subsystem_density_plan(list(range(6)), 30, 64)[1] == dict(path=1, block_rows=128, upper_blocks=1, slices=1024, units_read=1 << 30,
                                                      scratch_bytes=1025 * 128 * 128 * 8, trips_per_workgroup=512)
    assert plans.subsystem_density_plan(list(range(10)), 30, 32)[1] == dict(path=1, block_rows=128, upper_blocks=136, slices=16, units_read=16 << 29,
                                                       scratch_bytes=17 * 136 * 128 * 128 * 8, trips_per_workgroup=2048)


@pytest.mark.parametrize("bits", [64, 32])
def test_scratch_stays_within_a_gibibyte(bits):
    for n in range(0, 35):
        for k in range(0, min(n, 10) + 1):
            rc, got = plans.subsystem_density_plan(list(range(k)), n, bits)
            assert rc == _lib.QSIM_OK and got["scratch_bytes"] <= 1 << 30, (n, k, got)


def test_plan_call_refusals():
    ok = lambda *a: plans.subsystem_density_plan(*a)[0]
    assert ok([0, 1], 6, 64) == _lib.QSIM_OK
    assert ok(list(range(10)), 12, 64) == _lib.QSIM_OK
    assert ok([0, 0], 6, 64) == _lib.ERR_ARG                     # a repeated qubit
    assert ok([0, 1, 2, 3, 4, 5, 5], 8, 64) == _lib.ERR_ARG
    assert ok([0, 6], 6, 64) == _lib.ERR_ARG                     # outside [0, n)
    assert ok([-1], 6, 64) == _lib.ERR_ARG
    assert ok(list(range(11)), 12, 64) == _lib.ERR_ARG           # k > 10
    assert ok([0, 1, 2], 2, 64) == _lib.ERR_ARG                  # k > n
    assert ok([0], -1, 64) == _lib.ERR_ARG and ok([0], 41, 64) == _lib.ERR_ARG and ok([], 41, 64) == _lib.ERR_ARG
    assert ok([0], 40, 64) == _lib.QSIM_OK and ok([], 0, 32) == _lib.QSIM_OK
    assert ok([0], 6, 16) == _lib.ERR_ARG                        # precision_bits
    lib = _lib.load()
    o = [c_int(), c_int(), c_long(), c_long(), c_uint64(), c_uint64(), c_long()]
    refs = [byref(x) for x in o]
    assert plans.subsystem_density_plan(None, 6, 64, k=1)[0] == _lib.ERR_ARG
    assert plans.subsystem_density_plan(None, 6, 64, k=-1)[0] == _lib.ERR_ARG
    assert plans.subsystem_density_plan(None, 6, 64, k=0)[0] == _lib.QSIM_OK
    arr = (c_int * 1)(0)
    for missing in range(len(refs)):
        args = list(refs)
        args[missing] = None
        assert lib.qsim_subsystem_density_plan(arr, 1, 6, 64, *args) == _lib.ERR_ARG  # raw: NULL for an out-parameter
    # the call itself refuses a NULL state before it looks at anything else
    out = (ctypes.c_double * 8)()
    assert lib.qsim_subsystem_density(None, arr, 1, out) == _lib.ERR_ARG
