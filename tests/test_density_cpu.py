"""Reduced density matrices, checked on the CPU: the checker of tests/test_gpu_density.py against dense constructions, the numpy
emulation of the kernel's decomposition (tests/density_ref.py) against the checker, and the host-only plan call
(plans.reduced_density_plan) against the emulation's geometry."""
import ctypes
import itertools
from ctypes import byref, c_int, c_long, c_uint64

import numpy as np
import pytest

import density_ref
from gpu_quantum_simulator_amd import _lib, plans
from pauli_rot_ref import rand_state

NEW_NAMES = ("qsim_reduced_density", "qsim_reduced_density_max_qubits", "qsim_reduced_density_plan", "qsim_density_sweeps_launched")  # census of the signature table
MODEL_KEYS = {"kernel_mask": "mask", "units_visited": "units", "trips_per_workgroup_at_grid_cap": "trips"}  # header name -> density_ref.plan's key


def _partial_trace_dense(psi, qubits):
    """rho of the whole register by an outer product, then the trace over every other qubit, one qubit at a time."""
    n = int(psi.size).bit_length() - 1
    rho = np.outer(psi, psi.conj()).reshape((2,) * (2 * n))      # axes: row bits top first, then column bits top first
    kept = list(range(n))                                        # qubit of row axis j is kept[::-1][j]
    for q in sorted((q for q in range(n) if q not in qubits), reverse=True):
        m = len(kept)
        ax = m - 1 - kept.index(q)
        rho = np.trace(rho, axis1=ax, axis2=m + ax)
        kept.remove(q)
    # kept is ascending; bring the row and the column axes into the caller's order (qubits[k-1] on top)
    k = len(qubits)
    order = [k - 1 - kept.index(q) for q in reversed(qubits)]
    rho = np.transpose(rho, order + [k + a for a in order]) if k else rho
    return rho.reshape(1 << k, 1 << k)


def test_signatures_have_the_new_names():
    for name in NEW_NAMES:
        assert name in _lib.SIGNATURES
    assert plans.reduced_density_max_qubits() == 5


def test_checker_on_product_states():
    """A product state's rho_A is the kron of its factors' projectors, top qubit first."""
    rng = np.random.default_rng(5)
    for n in range(1, 7):
        f = [rng.standard_normal(2) + 1j * rng.standard_normal(2) for _ in range(n)]
        psi = np.array([1.0 + 0j])
        for q in range(n):                                       # qubit q = index bit q: later factors are higher bits
            psi = np.kron(f[q], psi)
        for k in range(0, min(n, 5) + 1):
            for qs in itertools.permutations(range(n), k) if n <= 4 else density_ref.subsets(n, k):
                want = np.array([[np.vdot(psi, psi) / np.prod([np.vdot(f[q], f[q]) for q in qs])]])
                for q in qs:
                    want = np.kron(np.outer(f[q], f[q].conj()), want)
                assert np.allclose(density_ref.reduced_density(psi, list(qs)), want, atol=1e-12)


def test_checker_against_dense_partial_trace():
    for n in range(0, 7):
        psi = rand_state(n, 70 + n)
        for k in range(0, min(n, 5) + 1):
            for qs in density_ref.subsets(n, k):
                for order in (qs, qs[::-1], list(np.random.default_rng(n * 8 + k).permutation(qs))):
                    order = [int(q) for q in order]
                    assert np.allclose(density_ref.reduced_density(psi, order), _partial_trace_dense(psi, order), atol=1e-13)


@pytest.mark.parametrize("f32", [False, True])
def test_emulation_matches_the_checker(f32):
    """R R^T by 16 x 16 tiles in the instruction's lane layout, rho from G, the padding traced out, the caller's order — for both unit
    sizes, qubit 0 inside and outside the subset, both paths."""
    for n in range(0, 9):
        psi = rand_state(n, 170 + n)
        for k in range(0, min(n, 5) + 1):
            sets = density_ref.subsets(n, k)
            if n >= 7:                                           # the lowest, the highest and one in between, with and without qubit 0
                sets = [sets[0], sets[-1], sets[len(sets) // 2], sets[len(sets) // 3]]
            for qs in sets:
                for order in (qs, qs[::-1]) if k > 1 else (qs,):
                    got, units = density_ref.emulate(psi, order, f32)
                    assert np.max(np.abs(got - density_ref.reduced_density(psi, order))) < 1e-13, (n, order)
                    assert units == density_ref.plan(order, n, f32)["units"], (n, order)


@pytest.mark.parametrize("bits", [64, 32])
def test_plan_call_matches_the_emulation(bits):
    for n in range(0, 9):
        for k in range(0, min(n, 5) + 1):
            for qs in density_ref.subsets(n, k):
                for order in (qs, qs[::-1]) if k > 1 else (qs,):
                    rc, got = plans.reduced_density_plan(order, n, bits)
                    want = density_ref.plan(order, n, bits == 32)
                    assert rc == _lib.QSIM_OK, (n, order)
                    assert got == {key: want[MODEL_KEYS.get(key, key)] for key in got}, (n, order, got, want)
                    # the padding qubits are the lowest bits that are free
                    free = [q for q in range(n) if q not in order]
                    pad = [q for q in range(n) if got["kernel_mask"] >> q & 1 and q not in order]
                    assert pad == free[:len(pad)] and len(pad) == got["padded_k"] - k
                    assert got["path"] == (1 if n >= 3 and n - max(k, 3) >= 2 else 0)


def test_plan_call_trips_at_the_looping_sizes():
    """Where tests/test_gpu_density.py expects every workgroup to walk its loop more than once."""
    for bits, n in ((64, 22), (32, 23)):
        for qs in ([0, 1, 2], [n - 3, n - 2, n - 1], [0, 1, 2, 3, 4], [n - 5, n - 4, n - 3, n - 2, n - 1]):
            rc, got = plans.reduced_density_plan(qs, n, bits)
            assert rc == _lib.QSIM_OK and got["path"] == 1 and got["trips_per_workgroup_at_grid_cap"] >= 2, (bits, qs, got)
            assert got["trips_per_workgroup_at_grid_cap"] == density_ref.plan(qs, n, bits == 32)["trips"]
    assert plans.reduced_density_plan([0, 1, 2], 12, 64)[1]["trips_per_workgroup_at_grid_cap"] == 1


def test_plan_call_refusals():
    ok = lambda *a: plans.reduced_density_plan(*a)[0]
    assert ok([0, 1], 6, 64) == _lib.QSIM_OK
    assert ok([0, 0], 6, 64) == _lib.ERR_ARG                     # a repeated qubit
    assert ok([0, 6], 6, 64) == _lib.ERR_ARG                     # outside [0, n)
    assert ok([-1], 6, 64) == _lib.ERR_ARG
    assert ok([0, 1, 2, 3, 4, 5], 8, 64) == _lib.ERR_ARG         # k > 5
    assert ok([0, 1, 2], 2, 64) == _lib.ERR_ARG                  # k > n
    assert ok([0], -1, 64) == _lib.ERR_ARG and ok([0], 41, 64) == _lib.ERR_ARG and ok([], 41, 64) == _lib.ERR_ARG
    assert ok([0], 40, 64) == _lib.QSIM_OK and ok([], 0, 32) == _lib.QSIM_OK
    assert ok([0], 6, 16) == _lib.ERR_ARG                        # precision_bits
    lib = _lib.load()
    padded, mask, units, trips = c_int(), c_uint64(), c_uint64(), c_long()
    assert plans.reduced_density_plan(None, 6, 64, k=1)[0] == _lib.ERR_ARG
    assert plans.reduced_density_plan(None, 6, 64, k=-1)[0] == _lib.ERR_ARG
    assert plans.reduced_density_plan(None, 6, 64, k=0)[0] == _lib.QSIM_OK
    arr = (c_int * 1)(0)
    assert lib.qsim_reduced_density_plan(arr, 1, 6, 64, None, byref(padded), byref(mask), byref(units), byref(trips)) == _lib.ERR_ARG  # raw: NULL for an out-parameter
    # the call itself refuses a NULL state before it looks at anything else
    out = (ctypes.c_double * 8)()
    assert lib.qsim_reduced_density(None, arr, 1, out) == _lib.ERR_ARG
