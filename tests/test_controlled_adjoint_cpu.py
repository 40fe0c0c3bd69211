"""Adjoint gradients through controlled Pauli rotations, the parts that need no GPU: the numpy checker
(tests/controlled_adjoint_ref.py) pinned against dense operators and the four-term shift rule, the two-term rule shown wrong (the
reason the feature exists), the host-only plan plans.controlled_gradient_plan, and the fp32 legality of every case the GPU tests run."""
import ctypes
import itertools
import math

import numpy as np
import pytest

import controlled_adjoint_ref as ref
import controlled_rot_ref as crot
import fp32_ref
import pauli_rot_ref
from gpu_quantum_simulator_amd import _lib, plans

UP = ctypes.POINTER(ctypes.c_uint64)


def _against_dense(n, psi0, rotations, terms):
    energy, grad, final = ref.gradient(psi0, rotations, terms)
    e_dense, g_dense = ref.dense_gradient(psi0, rotations, terms, n)
    assert np.max(np.abs(final - crot.replay(psi0, rotations))) == 0
    return max(abs(energy - e_dense), float(np.max(np.abs(grad - g_dense))))


def test_checker_matches_the_dense_derivative_exhaustively_up_to_three_qubits():
    """Every assignment of {control, I, X, Y, Z} to the qubits, the uncontrolled ones too, each between two other rotations."""
    worst, largest = 0.0, 0.0
    for n in (1, 2, 3):
        psi0 = ref.rand_state(n, 30 + n)
        terms = ref.random_hamiltonian(n, 5, 40 + n, 2)
        rng = np.random.default_rng(n)
        for letters in itertools.product("CIXYZ", repeat=n):
            c, x, z = (ref.mask_of(q for q in range(n) if letters[q] in sel) for sel in ("C", "XY", "ZY"))
            rotations = [(0.6, 0, 1, 1), (float(rng.uniform(-3, 3)), c, x, z), (-0.8, 0, 1 << (n - 1), 0)]
            worst = max(worst, _against_dense(n, psi0, rotations, terms))
            largest = max(largest, abs(ref.gradient(psi0, rotations, terms)[1][1]))
    assert worst < 1e-12 and largest > 1e-2, (worst, largest)


def _random_case(n, seed, count=10):
    rng = np.random.default_rng(seed)
    rotations = []
    for i in range(count):
        c = ref.mask_of(int(q) for q in rng.choice(n, size=i % min(n, 4), replace=False))
        rotations.append((float(rng.uniform(-3, 3)), c) + crot.random_string(rng, n, c))
    return ref.rand_state(n, seed), rotations, ref.random_hamiltonian(n, 6, seed + 1, 2)


def test_checker_matches_the_dense_derivative_on_random_cases():
    worst = max(_against_dense(4, *_random_case(4, seed)) for seed in range(70, 76))
    assert worst < 1e-12, worst


def test_checker_matches_the_four_term_rule_and_the_two_term_rule_does_not():
    n = 6
    psi0, rotations, terms = _random_case(n, 60, 12)
    energy, grad, _ = ref.gradient(psi0, rotations, terms)
    assert abs(energy - ref.energy(psi0, rotations, terms)) < 1e-12
    four, two = ref.shift4_gradient(psi0, rotations, terms), ref.shift2_gradient(psi0, rotations, terms)
    worst = max(abs(grad[k] - four[k]) for k in four)
    controlled = [k for k, r in enumerate(rotations) if r[1]]
    off = max(abs(grad[k] - two[k]) for k in controlled)
    print(f"adjoint vs four-term rule: worst {worst:.3e}; the two-term rule is off by up to {off:.3e} on a controlled component")
    assert worst < 1e-12
    assert off > 1e-3  # the generator Pi P / 2 has the eigenvalue 0 too
    assert all(abs(grad[k] - two[k]) < 1e-12 for k, r in enumerate(rotations) if not r[1])  # without controls it is exact
    assert np.max(np.abs(grad)) > 1e-3


def test_plan_sweeps():
    K = plans.pauli_rotations_per_sweep()
    KH = plans.pauli_terms_per_sweep()
    n = ref.RUN_N
    a, b = ref.RUN_CONTROLS
    x = pauli_rot_ref.LONG_RUN_X
    H = [(1.0, 3, 0), (1.0, 0, 1), (1.0, 3, 1)]
    assert ref.plan([], [], n) == (0, 0, 0)
    for label, (rotations, sweeps) in ref.run_cases(K).items():
        assert ref.plan(rotations, H, n)[:2] == (sweeps, 2), label
    # a change of control mask ends a run as a change of x does; equal (c, x) apart from each other do not share
    mixed = [(0.1, a, x, 0)] * 3 + [(0.1, b, x, 0)] * 2 + [(0.1, 0, x, 0)] * 2 + [(0.1, a, x, 0)] + [(0.1, a, x ^ 1, 0)] + [(0.1, a, x, 0)] * (K + 1)
    assert ref.plan(mixed, [], n)[:2] == (4 + 1 + 2, 0)
    # every term is a sweep backwards: one control on a single X or Y too, which takes the gate queue forwards
    assert ref.plan([(0.1, 1 << 5, 1 << 2, 0), (0.1, 1, 1 << 9, 1 << 9)], [], n)[:2] == (2, 0)
    assert ref.plan([(0.1, a, 0, 0), (0.1, a, 0, 4), (0.1, a, 0, 0)], [], n)[:2] == (1, 0)  # the controlled identity joins a diagonal run
    assert ref.plan([(0.1, a, x, 0)], [(1.0, 6, 0)] * (2 * KH + 1) + [(1.0, 1, 0)], n)[:2] == (1, 4)


def test_plan_without_controls_is_the_uncontrolled_plan():
    K = plans.pauli_rotations_per_sweep()
    diag, paired = pauli_rot_ref.long_run_rotations(K)
    rotations, terms = ref.uncontrolled_case()
    for old, n in ((diag + paired, 13), ([(t, x, z) for t, _, x, z in rotations], ref.BITS_N), (pauli_rot_ref.single_bit_rotations(13), 13)):
        plain = plans.ok(plans.pauli_gradient_plan([x for _, x, _ in old], [x for _, x, _ in terms]))
        zero = [(t, 0, x, z) for t, x, z in old]
        for precision in (64, 32):
            got = ref.plan(zero, terms, n, precision)
            assert got[:2] == (plain["adjoint_sweeps"], plain["sum_sweeps"])
            assert got == ref.plan(zero, terms, n, precision, null_controls=True)


def test_large_register_primitives_have_the_bits_of_the_small_ones():
    """What the n = 22 GPU case is checked with (Kronecker sign vectors, partners through a flip of axes) against the index-array
    checker: the loop case's shape at n = 10 and random cases, in both dtypes — equal bits of the states, the sums to rounding."""
    cases = [(ref.rand_state(10, 3),) + ref.loop_case(10)[1:]] + [_random_case(n, 80 + n, 8) for n in (1, 2, 5, 7)]
    for psi0, rotations, terms in cases:
        for dtype in (np.complex128, np.complex64):
            small = ref.gradient(psi0.astype(dtype), rotations, terms, dtype)
            large = ref.gradient(psi0.astype(dtype), rotations, terms, dtype, large=True)
            assert large[2].dtype == dtype and np.array_equal(small[2], large[2])
            assert abs(small[0] - large[0]) < 1e-14 and np.max(np.abs(small[1] - large[1])) < 1e-14
            back = [(-theta, c, x, z) for theta, c, x, z in rotations[::-1]]
            assert np.array_equal(ref.large_replay(small[2], back, dtype), crot.replay(small[2], back, dtype))
    assert np.max(np.abs(ref.gradient(ref.rand_state(10, 3), *ref.loop_case(10)[1:])[1])) > 1e-3


def _units_by_enumeration(n, precision, c, x):
    """Distinct 16-byte units that hold a visited index: every control bit 1 and, for x != 0, the highest bit of x clear."""
    j = np.arange(1 << n, dtype=np.uint64)
    visited = (j & np.uint64(c)) == np.uint64(c)
    if x:
        visited &= (j >> np.uint64(x.bit_length() - 1)) & np.uint64(1) == 0
    return int(np.unique(j[visited] >> np.uint64(0 if precision == 64 else 1)).size)


@pytest.mark.parametrize("precision", [64, 32])
def test_plan_units_against_an_enumeration(precision):
    n = 10
    checked = 0
    for x in (0, 1, 2, 1 << (n - 1) | 0b100):
        uncontrolled = ref.plan([(0.3, 0, x, 0)], [], n, precision)
        assert uncontrolled == (1, 0, _units_by_enumeration(n, precision, 0, x)), (x, uncontrolled)
        for qubits in [(q,) for q in range(n)] + list(itertools.combinations(range(n), 2)):
            c = ref.mask_of(qubits)
            if c & x:
                continue
            got = ref.plan([(0.3, c, x, 0)], [], n, precision)
            want = _units_by_enumeration(n, precision, c, x)
            assert got == (1, 0, want), (x, qubits, got, want)
            if precision == 64 or (not c & 1 and x != 1):
                assert got[2] == uncontrolled[2] >> len(qubits)  # 2^-c of the uncontrolled sweep; psi and lambda share the unit index
            checked += 1
    assert checked > 150
    # units add up over the sweeps of a call, pieces of a long run and uncontrolled sweeps included
    K = plans.pauli_rotations_per_sweep()
    run = ref.run_terms(K)
    sweeps, _, units = ref.plan(run + [(0.2, 0, 0, 1)], [], ref.RUN_N, precision)
    assert sweeps == -(-len(run) // K) + 1
    assert units == (sweeps - 1) * _units_by_enumeration(ref.RUN_N, precision, run[0][1], run[0][2]) + _units_by_enumeration(ref.RUN_N, precision, 0, 0)
    assert ref.plan([(0.3, (1 << n) - 1, 0, 0)], [], n, precision) == (1, 0, 1)  # every qubit a control: one amplitude, one unit
    assert ref.plan([(0.3, 1, 0, 0)], [], 1, precision) == (1, 0, 1)


def test_plan_argument_errors():
    lib = _lib.load()
    ok, cs = [1, 2], [4, 8]
    probe = plans.controlled_gradient_plan

    def refused(word, *args, **counts):
        assert probe(*args, **counts)[0] == _lib.ERR_ARG
        assert word in lib.qsim_last_error(), lib.qsim_last_error()

    rc, got = probe(cs, ok, ok, 5, 64)
    assert rc == 0 and (got["adjoint_sweeps"], got["sum_sweeps"]) == (2, 2)
    refused(b"negative", cs, ok, ok, 5, 64, num_rot=-1)
    refused(b"negative", cs, ok, ok, 5, 64, num_ham=-1)
    refused(b"NULL", cs, None, ok, 5, 64, num_rot=2)
    refused(b"NULL", cs, ok, None, 5, 64, num_ham=2)
    okp, csp = (np.array(v, dtype=np.uint64).ctypes.data_as(UP) for v in (ok, cs))
    out = (ctypes.byref(ctypes.c_long()), ctypes.byref(ctypes.c_long()), ctypes.byref(ctypes.c_uint64()))
    for i in range(3):
        missing = (None if k == i else p for k, p in enumerate(out))
        assert lib.qsim_controlled_gradient_plan(csp, okp, 2, okp, 2, 5, 64, *missing) == _lib.ERR_ARG  # raw: NULL for an out-parameter
        assert b"NULL" in lib.qsim_last_error(), lib.qsim_last_error()
    refused(b"precision", cs, ok, ok, 5, 16)
    refused(b"qubits", cs, ok, ok, -1, 64)
    refused(b"qubits", cs, ok, ok, 41, 64)
    refused(b"outside", cs, ok, ok, 1, 64)  # a string's qubit outside the register
    refused(b"control qubit outside", cs, ok, ok, 3, 64)  # control 3 on three qubits
    refused(b"term 1: a control qubit carries a Pauli factor", [4, 2], ok, ok, 5, 64)
    assert probe(None, None, None, 5, 64) == (0, dict(adjoint_sweeps=0, sum_sweeps=0, units_visited=0))


def test_fp32_cases_stay_under_the_reference_cap():
    """The complex64 run of the checker, which the fp32 GPU tests use as ref32, is within fp32_ref.REF_CAP of the fp64 one on every
    case; every case is legal and has a gradient that is no comparison of zeros."""
    K = plans.pauli_rotations_per_sweep()
    labels = []
    for label, start, rotations, terms in ref.fp32_cases(K):
        n = start.size.bit_length() - 1
        assert all(c & (x | z) == 0 and (c | x | z) < 1 << n for _, c, x, z in rotations), label
        start32 = start.astype(np.complex64)
        _, g64, _ = ref.gradient(start32.astype(np.complex128), rotations, terms)
        _, g32, final32 = ref.gradient(start32, rotations, terms, np.complex64)
        assert final32.dtype == np.complex64
        err = fp32_ref.rel_err(g32, g64)
        print(f"{label}: {len(rotations)} rotations, max |grad| {np.max(np.abs(g64)):.3e}, rel_err(ref32) = {err:.3e}")
        assert err <= fp32_ref.REF_CAP, (label, err)
        assert np.max(np.abs(g64)) > 1e-3, label
        labels.append(label)
    assert len(labels) == len(set(labels)) >= 40
