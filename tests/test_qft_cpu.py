"""The quantum Fourier transform, checked on the CPU: the checker of tests/test_gpu_qft.py (qft_ref.apply_qft) against the dense DFT
through matrix_ref.apply_matrix, the pass rule (qft_ref.walk_plan) against the checker for the digit lists the host-only plan call
(plans.apply_qft_plan) reports, the plan itself against a restatement of its rule, its refusals, the complex64 replay's error on every
shape the GPU test uses, the textbook circuit the GPU test cross-checks against, and a census of include/qsim_qft.h against
_lib.QFT_SIGNATURES.  Needs the built library for the plan call, no device."""
import itertools
import os
import re
from ctypes import byref, c_int, c_long, c_uint64

import numpy as np
import pytest

import fp32_ref
import matrix_ref
import qft_ref
from gpu_quantum_simulator_amd import Cluster, Simulator, _lib, plans
from gpu_quantum_simulator_amd._marshal import ints as _ints
from pauli_rot_ref import rand_state

GRID_CAP = 512
MAX_DIGIT = 10
OWN_LONG_CAP = 9   # the plan's own cap for a register of more than ten qubits: three padding bits in an fp64 tile


def _pad_subset(subset, size, n):
    """`subset` and the lowest index bits outside it until it has `size` bits."""
    for q in range(n):
        if bin(subset).count("1") >= size:
            break
        subset |= 1 << q
    return subset


def test_signatures_and_header_census():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "include", "qsim_qft.h")).read()
    declared = set(re.findall(r"\b(qsim_[a-z0-9_]+)\s*\(", text))
    assert declared == set(_lib.QFT_SIGNATURES), declared ^ set(_lib.QFT_SIGNATURES)
    assert not set(_lib.QFT_SIGNATURES) & set(_lib.SIGNATURES)
    main = open(os.path.join(root, "include", "qsim.h")).read()
    assert main.count('#include "qsim_qft.h"') == 1 and "qsim_apply_qft" not in main
    lib = _lib.load()
    for name in _lib.QFT_SIGNATURES:
        assert getattr(lib, name).restype is _lib.QFT_SIGNATURES[name][0]   # load() has applied the table
    assert plans.apply_qft_max_digit_bits() == MAX_DIGIT
    assert hasattr(Simulator, "apply_qft") and not hasattr(Cluster, "apply_qft")


# ---- the checker ----------------------------------------------------------------------------------------------------------------------
def test_checker_equals_the_dense_dft():
    for n in range(0, 7):
        psi = rand_state(n, 900 + n)
        for k in range(0, min(n, 5) + 1):
            for qubits in list(itertools.permutations(range(n), k))[:: max(1, n)]:
                for inverse in (False, True):
                    got = qft_ref.apply_qft(psi, qubits, inverse)
                    want = matrix_ref.apply_matrix(psi, qft_ref.dft_matrix(k, inverse), qubits)
                    assert np.max(np.abs(got - want)) < 1e-14, (n, qubits, inverse)
    # the definition, by hand: |1> on one qubit goes to (|0> - |1>) / sqrt 2, and |01> on (q0, q1) to the phases 1, i, -1, -i over 2
    assert np.allclose(qft_ref.apply_qft(np.array([0, 1.0]), [0]), np.array([1, -1]) / np.sqrt(2))
    assert np.allclose(qft_ref.apply_qft(np.array([0, 1.0, 0, 0]), [0, 1]), np.array([1, 1j, -1, -1j]) / 2)
    assert np.allclose(qft_ref.apply_qft(np.array([0, 1.0, 0, 0]), [0, 1], inverse=True), np.array([1, -1j, -1, 1j]) / 2)
    assert np.allclose(qft_ref.apply_qft(np.array([0, 1.0, 0, 0]), [1, 0]), np.array([1, 1, -1, -1]) / 2)    # qubit 0 is the register's top bit: x = 2, (-1)^y, and y = 1 is index 2
    psi = rand_state(9, 99)
    back = qft_ref.apply_qft(qft_ref.apply_qft(psi, [8, 0, 3, 5]), [8, 0, 3, 5], inverse=True)
    assert np.max(np.abs(back - psi)) < 1e-14


def test_textbook_circuit_equals_the_checker():
    for n, qubits in ((5, [3, 0, 4]), (6, [5, 4, 3, 2, 1, 0]), (7, [1, 6, 2, 0, 5]), (4, [2]), (9, [8, 0, 3, 5, 1, 7, 2, 6])):
        psi = rand_state(n, 910 + n)
        got = fp32_ref.replay(n, qft_ref.textbook_gates(qubits), start=psi, dtype=np.complex128)
        assert np.max(np.abs(got - qft_ref.apply_qft(psi, qubits))) < 1e-13, qubits


# ---- the plan and the pass rule ---------------------------------------------------------------------------------------------------------
def _register_choices(n, k, rng):
    out = [list(range(k)), list(range(n - k, n))[::-1]]
    if 0 < k < n:
        out.append([int(q) for q in rng.permutation(n)[:k]])
    return out


@pytest.mark.parametrize("bits", [64, 32])
def test_plan_against_its_rule_and_walk_plan_against_the_checker(bits):
    full = 13 if bits == 32 else 12
    rng = np.random.default_rng(920)
    for n in range(0, 17):
        psi = rand_state(n, 930 + n)
        for k in sorted({max(0, min(k, n)) for k in (0, 1, 2, 5, 10, n - 1, n)}):
            for qubits in _register_choices(n, k, rng):
                for cap in (0, 1, 3, 4, 10):
                    rc, plan = plans.apply_qft_plan(qubits, n, bits, cap)
                    assert rc == _lib.QSIM_OK, (n, qubits, cap)
                    limit = cap or (MAX_DIGIT if k <= MAX_DIGIT else OWN_LONG_CAP)
                    digits = plan["digit_bits"]
                    assert sum(digits) == k and all(1 <= d <= limit for d in digits) and plan["passes"] == -(-k // limit)
                    assert sum(plan["out_of_place"]) % 2 == 0 and all(plan["out_of_place"][:-1]) and (k > limit or plan["out_of_place"] == [0] * plan["passes"])
                    B = min(full, n)
                    first = 0
                    for d, mask in zip(digits, plan["tile_mask"]):
                        top = qubits[k - d:]                     # the sub-register's top d bits: the rest has moved up behind the digits done
                        assert mask == _pad_subset(sum(1 << q for q in top), B, n), (n, qubits, cap, first)
                        first += d
                    assert plan["tiles"] == 1 << (n - B) and plan["units"] == max(1, (1 << n) >> (1 if bits == 32 else 0))
                    assert plan["trips_per_workgroup"] == -(-plan["tiles"] // GRID_CAP)
                    if n <= 12 or cap in (0, 4):
                        for inverse in (False, True):
                            got = qft_ref.walk_plan(psi, qubits, digits, inverse)
                            assert np.max(np.abs(got - qft_ref.apply_qft(psi, qubits, inverse))) < 1e-13, (n, qubits, cap, inverse)


def test_plan_named_cases():
    assert plans.apply_qft_plan(list(range(10)), 30, 64, 0)[1]["digit_bits"] == [10] and plans.apply_qft_plan(list(range(10)), 30, 64, 0)[1]["out_of_place"] == [0]
    p = plans.apply_qft_plan(list(range(20)), 30, 64, 10)[1]
    assert p["digit_bits"] == [10, 10] and p["out_of_place"] == [1, 1] and p["tile_mask"] == [0b11 | sum(1 << q for q in range(10, 20))] * 2
    p = plans.apply_qft_plan(list(range(20)), 30, 64, 0)[1]                                        # the plan's own cap beyond ten qubits is nine bits
    assert p["digit_bits"] == [7, 7, 6] and p["out_of_place"] == [1, 1, 0] and p["tile_mask"][0] == 0b11111 | sum(1 << q for q in range(13, 20))
    assert plans.apply_qft_plan(list(range(18)), 30, 64, 0)[1]["digit_bits"] == [9, 9]
    p = plans.apply_qft_plan(list(range(30)), 30, 64, 10)[1]
    assert p["digit_bits"] == [10, 10, 10] and p["out_of_place"] == [1, 1, 0] and p["tiles"] == 1 << 18 and p["trips_per_workgroup"] == 512
    assert plans.apply_qft_plan(list(range(30)), 30, 64, 0)[1]["digit_bits"] == [8, 8, 7, 7] and plans.apply_qft_plan(list(range(30)), 30, 64, 0)[1]["out_of_place"] == [1, 1, 1, 1]
    assert plans.apply_qft_plan(list(range(11)), 13, 64, 0)[1]["digit_bits"] == [6, 5]                 # as even as the cap allows
    assert plans.apply_qft_plan(list(range(12)), 13, 64, 4)[1]["out_of_place"] == [1, 1, 0] and plans.apply_qft_plan(list(range(13)), 13, 64, 4)[1]["out_of_place"] == [1, 1, 1, 1]
    assert plans.apply_qft_plan(list(range(13)), 13, 64, 1)[1]["passes"] == 13 and sum(plans.apply_qft_plan(list(range(13)), 13, 64, 1)[1]["out_of_place"]) == 12
    assert plans.apply_qft_plan([], 0, 32, 0)[1] == dict(passes=0, digit_bits=[], out_of_place=[], tile_mask=[], tiles=1, units=1, trips_per_workgroup=1)
    for precision in (64, 32):                                                       # the looping sizes of the GPU test
        n = 22 if precision == 64 else 23
        assert plans.apply_qft_plan(list(range(n)), n, precision, 0)[1]["trips_per_workgroup"] >= 2


def test_plan_refusals():
    ok = lambda qubits, n, bits, cap=0, **kw: plans.apply_qft_plan(qubits, n, bits, cap, **kw)[0]
    assert ok([0, 1], 6, 64) == _lib.QSIM_OK and ok(None, 6, 64) == _lib.QSIM_OK
    assert ok(None, 6, 64, k=1) == _lib.ERR_ARG                                 # a NULL list with k > 0
    assert ok([0], 6, 64, k=-1) == _lib.ERR_ARG and ok(list(range(7)), 6, 64) == _lib.ERR_ARG   # k outside [0, n]
    assert ok([0, 0], 6, 64) == _lib.ERR_ARG and ok([2, 5, 2], 6, 64) == _lib.ERR_ARG           # a repeated qubit
    assert ok([6], 6, 64) == _lib.ERR_ARG and ok([-1], 6, 64) == _lib.ERR_ARG                   # out of range
    assert ok([0], 6, 64, cap=11) == _lib.ERR_ARG and ok([0], 6, 64, cap=-1) == _lib.ERR_ARG    # max_digit_bits outside [0, 10]
    assert ok([0], 6, 64, cap=10) == _lib.QSIM_OK and ok([0], 6, 64, cap=1) == _lib.QSIM_OK
    assert ok([0], 6, 16) == _lib.ERR_ARG and ok([0], -1, 64) == _lib.ERR_ARG and ok([0], 41, 64) == _lib.ERR_ARG
    assert ok(list(range(40)), 40, 64) == _lib.QSIM_OK
    passes, tiles, units, trips = c_int(), c_uint64(), c_uint64(), c_long()
    digits, oop, masks = (c_int * 40)(), (c_int * 40)(), (c_uint64 * 40)()
    assert _lib.load().qsim_apply_qft_plan(_ints([0]), 1, 6, 64, 0, None, digits, oop, masks, byref(tiles), byref(units), byref(trips)) == _lib.ERR_ARG  # raw: NULL for an out-parameter
    assert _lib.load().qsim_apply_qft_plan(_ints([0]), 1, 6, 64, 0, byref(passes), digits, oop, None, byref(tiles), byref(units), byref(trips)) == _lib.ERR_ARG  # raw: NULL for an out-parameter
    assert _lib.load().qsim_apply_qft(None, _ints([0]), 1, 0, 0) == _lib.ERR_ARG     # the call refuses a NULL state before anything else


# ---- the fp32 replay --------------------------------------------------------------------------------------------------------------------
def test_replay_error_is_inside_the_reference_cap_on_every_gpu_shape():
    worst = 0.0
    for n, k in qft_ref.fp32_shapes():
        psi = rand_state(n, 940 + n).astype(np.complex64)
        qubits = [int(q) for q in np.random.default_rng(n * 41 + k).permutation(n)[:k]]
        for inverse in (False, True):
            want = qft_ref.apply_qft(psi.astype(np.complex128), qubits, inverse)
            ref32 = qft_ref.apply_qft(psi, qubits, inverse, dtype=np.complex64)
            assert ref32.dtype == np.complex64
            err = fp32_ref.rel_err(ref32, want)
            worst = max(worst, err)
            assert err <= fp32_ref.REF_CAP, (n, k, inverse, err)
    print(f"fp32 replay: worst rel_err {worst:.3e}")
    assert worst < 1e-6                                          # a radix-2 transform of at most 23 stages in complex64
