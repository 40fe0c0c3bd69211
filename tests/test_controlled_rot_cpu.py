"""Controlled Pauli rotations, the parts that need no GPU: the numpy checker (tests/controlled_rot_ref.py) pinned against dense
operators, the fp32 legality of every sequence the GPU tests run, the routing and the units visited as
plans.controlled_rotation_plan reports them, and the Python front end's argument checks."""
import ctypes
import itertools
import math

import numpy as np
import pytest

import controlled_rot_ref as ref
import fp32_ref
import pauli_ref
import pauli_rot_ref
from gpu_quantum_simulator_amd import _lib, plans
from gpu_quantum_simulator_amd.pauli import control_mask

UP = ctypes.POINTER(ctypes.c_uint64)


def _against_dense(n, psi, theta, c, x, z):
    want = ref.dense_controlled(c, x, z, n, theta) @ psi
    got = ref.apply_rotation(psi, c, x, z, theta)
    got32 = ref.apply_rotation(psi.astype(np.complex64), c, x, z, theta, np.complex64)
    assert got32.dtype == np.complex64 and np.max(np.abs(got32 - want)) < 1e-6
    return float(np.max(np.abs(got - want)))


def test_checker_matches_dense_operators_exhaustively_up_to_three_qubits():
    worst = 0.0
    for n in (1, 2, 3):
        psi = ref.rand_state(n, 30 + n)
        for letters in itertools.product("CIXYZ", repeat=n):  # every assignment, the uncontrolled ones too
            c, x, z = (ref.mask_of(q for q in range(n) if letters[q] in sel) for sel in ("C", "XY", "ZY"))
            for theta in (0.0, math.pi, -0.75, 2.9):
                worst = max(worst, _against_dense(n, psi, theta, c, x, z))
    assert worst < 1e-12, worst


def test_checker_matches_dense_operators_on_random_cases():
    rng = np.random.default_rng(4)
    worst = 0.0
    for n in range(2, 7):
        psi = ref.rand_state(n, n)
        for size in range(1, n + 1):
            for _ in range(4):
                c = ref.mask_of(int(q) for q in rng.choice(n, size=size, replace=False))
                x, z = ref.random_string(rng, n, c)
                worst = max(worst, _against_dense(n, psi, float(rng.uniform(-2 * math.pi, 2 * math.pi)), c, x, z))
    assert worst < 1e-12, worst


def test_mcx_and_mcz_constructions_on_the_checker():
    """What Simulator.apply_mcx and apply_mcz hand to the C call is the permutation and the diagonal they promise."""
    n = 5
    psi = ref.rand_state(n, 55)
    j = np.arange(1 << n)
    for controls, target in (((0, 3), 1), ((4, 2, 1), 0), ((0, 1, 2, 3), 4)):
        c = ref.mask_of(controls)
        got = ref.replay(psi, ref.mcx_terms(controls, target))
        assert np.max(np.abs(got - psi[np.where((j & c) == c, j ^ (1 << target), j)])) < 1e-15
    for qubits in ((0, 1), (1, 2, 4), (0, 1, 2, 3, 4)):
        c = ref.mask_of(qubits)
        got = ref.replay(psi, [(-2.0 * math.pi, c, 0, 0)])
        assert np.max(np.abs(got - np.where((j & c) == c, -psi, psi))) < 1e-15


def test_fp32_sequences_are_legal():
    K = plans.pauli_rotations_per_sweep()
    labels = []
    for label, n, start, rotations in ref.fp32_sequences(K):
        assert all(c & (x | z) == 0 and (c | x | z) < 1 << n for _, c, x, z in rotations), label
        start32 = start.astype(np.complex64)
        want = ref.replay(start32.astype(np.complex128), rotations)
        ref32 = ref.replay(start32, rotations, np.complex64)
        assert ref32.dtype == np.complex64
        err = fp32_ref.rel_err(ref32, want)
        print(f"{label}: {len(rotations)} rotations, rel_err(ref32) = {err:.3e}")
        assert err <= fp32_ref.REF_CAP, (label, err)
        labels.append(label)
    assert len(labels) == len(set(labels)) >= 20


_plan = ref.plan


def _old_plan(rotations):
    p = plans.ok(plans.pauli_rotation_plan([r[2] for r in rotations], [r[3] for r in rotations]))
    return p["sweeps"], p["queued_as_gates"]


def test_routing_plan():
    K = plans.pauli_rotations_per_sweep()
    n = ref.RUN_N
    run = ref.run_terms(K)
    assert len(run) == 3 * K + 5 and len({(c, x) for _, c, x, _ in run}) == 1
    assert _plan(run, n)[:2] == (-(-(3 * K + 5) // K), 0)  # one (control mask, x): pieces of K
    alternating = ref.run_terms(K, ref.RUN_CONTROLS)
    assert _plan(alternating, n)[:2] == (len(alternating), 0)  # a change of control mask ends a run
    a, b = ref.RUN_CONTROLS
    x = pauli_rot_ref.LONG_RUN_X
    assert _plan([(0.1, a, x, 0)] * 3 + [(0.1, b, x, 0)] * 2 + [(0.1, 0, x, 0)] * 2 + [(0.1, a, x, 0)], n)[:2] == (4, 0)
    assert _plan([(0.1, a, x, 0), (0.1, a, x ^ 1, 0), (0.1, a, x, 0)], n)[:2] == (3, 0)  # and so does a change of x
    assert _plan([(0.1, a, 0, 0), (0.1, a, 0, 4), (0.1, a, 0, 0)], n)[:2] == (1, 0)  # the controlled identity joins a diagonal run
    # one control on a single X or Y: the gate queue; anything else under controls: a sweep
    assert _plan([(0.1, 1 << 5, 1 << 2, 0), (0.1, 1, 1 << 9, 1 << 9)], n)[:2] == (0, 2)
    assert _plan([(0.1, 1 << 5 | 1, 1 << 2, 0)], n)[:2] == (1, 0)  # two controls
    assert _plan([(0.1, 1 << 5, 0, 1 << 2)], n)[:2] == (1, 0)  # a controlled Z
    assert _plan([(0.1, 1 << 5, 0, 0)], n)[:2] == (1, 0)  # the controlled identity
    assert _plan([(0.1, 1 << 5, 1 << 2, 1 << 3)], n)[:2] == (1, 0)  # X2 Z3
    assert _plan([(0.1, 1 << 5, 0b11, 0), (0.1, 1 << 5, 1, 0), (0.1, 1 << 5, 0b11, 0)], n)[:2] == (2, 1)  # a queued 4x4 cuts a run
    assert _plan([], n) == (0, 0, 0)
    # no controls anywhere: plans.pauli_rotation_plan, with c_masks all zero and with c_masks NULL
    diag, paired = pauli_rot_ref.long_run_rotations(K)
    rng = np.random.default_rng(71)
    mixed = [(0.1,) + pauli_ref.random_masks(rng, n, 1 + i % 3) for i in range(60)]
    for old in (diag + paired, mixed, pauli_rot_ref.single_bit_rotations(n)):
        rotations = [(t, 0, x, z) for t, x, z in old]
        for precision in (64, 32):
            got = _plan(rotations, n, precision)
            assert got[:2] == _old_plan(rotations)
        assert tuple(plans.ok(plans.controlled_rotation_plan(None, [r[2] for r in rotations], [r[3] for r in rotations], n, 32)).values()) == got


def _units_by_enumeration(n, precision, c, x):
    """Distinct 16-byte units that hold a visited index: every control bit 1 and, for x != 0, the highest bit of x clear."""
    j = np.arange(1 << n, dtype=np.uint64)
    visited = (j & np.uint64(c)) == np.uint64(c)
    if x:
        visited &= (j >> np.uint64(x.bit_length() - 1)) & np.uint64(1) == 0
    return int(np.unique(j[visited] >> np.uint64(0 if precision == 64 else 1)).size)


@pytest.mark.parametrize("precision", [64, 32])
def test_units_visited_against_an_enumeration(precision):
    n = 10
    checked = 0
    for x in (0, 1, 2, 1 << (n - 1) | 0b100):
        uncontrolled = _plan([(0.3, 0, x, 1 << 5 if x != 1 << 5 else 0b11)], n, precision)
        assert uncontrolled == (1, 0, _units_by_enumeration(n, precision, 0, x)), (x, uncontrolled)
        sets = [(q,) for q in range(n)] + list(itertools.combinations(range(n), 2))
        for qubits in sets:
            c = ref.mask_of(qubits)
            if c & x:
                continue
            z = next(1 << q for q in range(n) if not (c | x) >> q & 1)  # a Z elsewhere: every case is a sweep
            sweeps, gates, units = _plan([(0.3, c, x, z)], n, precision)
            want = _units_by_enumeration(n, precision, c, x)
            assert (sweeps, gates, units) == (1, 0, want), (x, qubits, units, want)
            if precision == 64 or (not c & 1 and x != 1):
                assert units == uncontrolled[2] >> len(qubits)  # 2^-c of the uncontrolled sweep
            checked += 1
    assert checked > 150
    # units add up over the sweeps of a call, pieces of a long run included
    K = plans.pauli_rotations_per_sweep()
    run = ref.run_terms(K)
    sweeps, _, units = _plan(run, ref.RUN_N, precision)
    assert units == sweeps * _units_by_enumeration(ref.RUN_N, precision, run[0][1], run[0][2])
    # every qubit a control: one amplitude, one unit
    assert _plan([(0.3, (1 << n) - 1, 0, 0)], n, precision) == (1, 0, 1)
    assert _plan([(0.3, 1, 0, 0)], 1, precision) == (1, 0, 1)


def test_plan_argument_errors():
    lib = _lib.load()
    ok, cs = [1, 2], [4, 8]
    probe = plans.controlled_rotation_plan

    def refused(word, *args, **counts):
        assert probe(*args, **counts)[0] == _lib.ERR_ARG
        assert word in lib.qsim_last_error(), lib.qsim_last_error()

    assert probe(cs, ok, ok, 5, 64)[0] == 0
    refused(b"negative", cs, ok, ok, 5, 64, num_terms=-1)
    refused(b"NULL", cs, None, ok, 5, 64, num_terms=2)
    refused(b"NULL", cs, ok, None, 5, 64)
    okp, csp = (np.array(v, dtype=np.uint64).ctypes.data_as(UP) for v in (ok, cs))
    out = (ctypes.byref(ctypes.c_long()), ctypes.byref(ctypes.c_long()), ctypes.byref(ctypes.c_uint64()))
    for i in range(3):
        missing = (None if k == i else p for k, p in enumerate(out))
        assert lib.qsim_controlled_rotation_plan(csp, okp, okp, 2, 5, 64, *missing) == _lib.ERR_ARG  # raw: NULL for an out-parameter
        assert b"NULL" in lib.qsim_last_error(), lib.qsim_last_error()
    refused(b"precision", cs, ok, ok, 5, 16)
    refused(b"qubits", cs, ok, ok, -1, 64)
    refused(b"qubits", cs, ok, ok, 41, 64)
    refused(b"outside", cs, ok, ok, 1, 64)  # a string's qubit outside the register
    refused(b"control qubit outside", cs, ok, ok, 3, 64)  # control 3 on three qubits
    refused(b"term 1: a control qubit carries a Pauli factor", [4, 2], ok, ok, 5, 64)
    refused(b"term 0: a control qubit carries a Pauli factor", [1, 8], [2, 2], ok, 5, 64)
    assert probe(None, None, None, 5, 64) == (0, dict(sweeps=0, queued_as_gates=0, units_visited=0))


def test_control_mask_checks():
    assert control_mask((), 5) == 0 and control_mask([4, 0], 5, "X1 Z2") == 0b10001
    for bad, word in (((4, 4), "twice"), ((5,), "outside"), ((-1,), "outside"), ((0.5,), "outside"), ((2,), "Pauli factor"), ((1,), "Pauli factor")):
        with pytest.raises(ValueError, match=word):
            control_mask(bad, 5, "X1 Z2")
