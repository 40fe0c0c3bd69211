"""Measurement, checked on the CPU: the checker of tests/test_gpu_measure.py (measure_ref) against brute force on n <= 4, the host-only
plan call (qsim_collapse_plan) against a restatement of its rule and its refusals, a census of include/qsim_measure.h against
_lib.MEASURE_SIGNATURES, the Kraus lists of channels.py, and the complex64 replay's error on the shapes the GPU test uses.  Needs the built
library for the plan call, no device."""
import math
import os
import re
from ctypes import byref, c_double, c_long, c_uint64
from fractions import Fraction

import numpy as np
import pytest

import fp32_ref
import matrix_ref
import measure_ref
import sample_ref
from gpu_quantum_simulator_amd import Cluster, Simulator, _lib, channels, plans
from gpu_quantum_simulator_amd._marshal import ints as _ints
from pauli_rot_ref import rand_state

GRID_CAP = 1024      # workgroups of either sweep at most
PER_TRIP = 256 * 8   # units a workgroup takes per trip


def test_signatures_and_header_census():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "include", "qsim_measure.h")).read()
    declared = set(re.findall(r"\b(qsim_[a-z0-9_]+)\s*\(", text))
    assert declared == set(_lib.MEASURE_SIGNATURES), declared ^ set(_lib.MEASURE_SIGNATURES)
    assert not set(_lib.MEASURE_SIGNATURES) & (set(_lib.SIGNATURES) | set(_lib.QFT_SIGNATURES))
    main = open(os.path.join(root, "include", "qsim.h")).read()
    assert main.count('#include "qsim_measure.h"') == 1
    assert not set(re.findall(r"\b(qsim_[a-z0-9_]+)\s*\(", main)) & set(_lib.MEASURE_SIGNATURES)
    lib = _lib.load()
    for name in _lib.MEASURE_SIGNATURES:
        assert getattr(lib, name).restype is _lib.MEASURE_SIGNATURES[name][0]   # load() has applied the table
    for method in ("postselect", "measure", "reset_qubits", "apply_channel"):
        assert hasattr(Simulator, method) and not hasattr(Cluster, method)


# ---- the checker ----------------------------------------------------------------------------------------------------------------------
def test_postselect_checker_equals_brute_force():
    for n in range(1, 5):
        psi = rand_state(n, 1100 + n) * 1.7                      # not normalised: the result is, whatever the start
        for qubits, outcome in measure_ref.small_cases(n):
            exact = Fraction(0)
            want = np.zeros(1 << n, dtype=np.complex128)
            for i in range(1 << n):
                if all(((i >> q) & 1) == ((outcome >> j) & 1) for j, q in enumerate(qubits)):
                    exact += Fraction(float(psi[i].real)) ** 2 + Fraction(float(psi[i].imag)) ** 2
                    want[i] = psi[i]
            W, got = measure_ref.postselect(psi, qubits, outcome)
            assert abs(Fraction(W) - exact) <= Fraction(2.0 ** -51) * exact, (n, qubits, outcome)
            assert np.max(np.abs(got - want / math.sqrt(float(exact)))) < 1e-15
            assert abs(np.vdot(got, got).real - 1.0) < 1e-14
            discarded = ~measure_ref.kept_indices(n, qubits, outcome)
            assert not np.ascontiguousarray(got[discarded]).view(np.uint64).any()           # +0.0, bit for bit
            back = measure_ref.cleared(got, qubits, outcome)
            measured, _ = measure_ref.masks(qubits, outcome)
            assert not back[(np.arange(1 << n) & measured) != 0].any() and abs(np.vdot(back, back).real - 1.0) < 1e-14
    # by hand: (|00> + |11>) / sqrt 2, qubit 1 read as 1, leaves |11> with weight one half
    W, got = measure_ref.postselect(np.array([1, 0, 0, 1]) / math.sqrt(2), [1], 1)
    assert abs(W - 0.5) < 1e-15 and np.allclose(got, [0, 0, 0, 1])
    W, got = measure_ref.postselect(np.array([0.6, 0.8j, 0, 0]), [1, 0], 2)                 # outcome bit 0 is qubit 1, bit 1 is qubit 0
    assert abs(W - 0.64) < 1e-15 and np.allclose(got, [0, 1j, 0, 0])


def test_admissible_outcomes_hold_the_brute_force_sampler():
    for n, qubits in ((3, [2, 0]), (4, [1]), (4, [3, 0, 2, 1])):
        psi = rand_state(n, 1110 + n)
        draws = [(i + 0.5) / 16 for i in range(16)] + [0.0, 1.0]
        hits = sample_ref.outcome_bits(sample_ref.brute_force(psi, draws), qubits)
        for u, hit in zip(draws, hits):
            assert int(hit) in measure_ref.admissible_outcomes(n, psi, u, qubits), (n, qubits, u)
        assert all(len(measure_ref.admissible_outcomes(n, psi, u, qubits)) == 1 for u in draws[:16])   # away from the edges: determined


def test_kraus_step_equals_the_dense_operators():
    n = 4
    psi = rand_state(n, 1120) * 0.8
    for kraus, targets in ((channels.two_qubit_depolarizing(0.3), (1, 3)), (channels.amplitude_damping(0.4), (0,)), (channels.bit_flip(0.0), (2,))):
        images = [matrix_ref.dense_operator(n, K, targets) @ psi for K in kraus]
        p = [float(np.vdot(v, v).real) / float(np.vdot(psi, psi).real) for v in images]
        assert abs(sum(p) - 1.0) < 1e-14
        for i, u in enumerate(measure_ref.midpoints(p)):
            if u is None:                                        # bit_flip(0): X has probability zero and is never picked
                assert p[i] == 0.0
                continue
            got_i, got_p, got_state, got_all = measure_ref.kraus_step(psi, kraus, targets, u)
            assert got_i == i and abs(got_p - p[i]) < 1e-14 and np.allclose(got_all, p, atol=1e-14)
            assert np.max(np.abs(got_state - images[i] / np.linalg.norm(images[i]))) < 1e-14
        for u in (0.0, 1.0):                                     # the ends pick the first and the last index that has a probability
            got_i = measure_ref.kraus_step(psi, kraus, targets, u)[0]
            assert p[got_i] > 0.0 and got_i == [i for i in range(len(p)) if p[i] > 0.0][0 if u == 0.0 else -1]
            assert channels.pick(p, u) == got_i
        rho = np.zeros((1 << len(targets),) * 2, dtype=np.complex128)   # the library's route, through rho of the targets, gives the same numbers
        for e in range(1 << n):
            if all(not (e >> q) & 1 for q in targets):
                col = np.array([psi[e | matrix_ref.deposit(a, targets)] for a in range(1 << len(targets))])
                rho += np.outer(col, col.conj())
        assert np.allclose(channels.probabilities(kraus, rho), p, atol=1e-14)


# ---- the plan -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bits", [64, 32])
def test_plan_against_its_rule(bits):
    rng = np.random.default_rng(1130)
    for n in range(0, 25):
        for k in sorted({min(k, n) for k in (0, 1, 2, 5, 10, 13, n)}):
            choices = [list(range(k)), list(range(n - k, n))[::-1], [int(q) for q in rng.permutation(n)[:k]]]
            for qubits in choices:
                for outcome in {0, (1 << k) - 1, int(rng.integers(0, 1 << k))}:
                    rc, plan = plans.collapse_plan(qubits, outcome, n, bits)
                    assert rc == _lib.QSIM_OK, (n, qubits, outcome)
                    per_unit = 2 if bits == 32 else 1
                    whole = max(1, (1 << n) // per_unit)
                    slot_measured = bits == 32 and 0 in qubits       # one slot of every visited unit counts: a unit more per pair
                    kept_units = max(1, ((1 << (n - k)) * (2 if slot_measured else 1)) // per_unit)
                    assert plan["collapse_units"] == whole and plan["weight_units"] == kept_units, (n, qubits, plan)
                    assert plan["collapse_trips"] == max(1, -(-whole // (PER_TRIP * GRID_CAP)))
                    assert plan["weight_trips"] == max(1, -(-kept_units // (PER_TRIP * GRID_CAP)))
    for precision in (64, 32):                                   # the looping sizes of the GPU test
        for n, qubits, outcome in measure_ref.looping_cases(precision):
            assert plans.collapse_plan(qubits, outcome, n, precision)[1]["collapse_trips"] >= 2


def test_plan_refusals():
    ok = lambda *a, **kw: plans.collapse_plan(*a, **kw)[0]
    assert ok([0, 1], 3, 6, 64) == _lib.QSIM_OK and ok(None, 0, 6, 64) == _lib.QSIM_OK
    assert ok(None, 0, 6, 64, k=1) == _lib.ERR_ARG                                      # a NULL list with k > 0
    assert ok([0], 0, 6, 64, k=-1) == _lib.ERR_ARG and ok(list(range(7)), 0, 6, 64) == _lib.ERR_ARG   # k outside [0, n]
    assert ok([0, 0], 0, 6, 64) == _lib.ERR_ARG and ok([2, 5, 2], 0, 6, 64) == _lib.ERR_ARG           # a repeated qubit
    assert ok([6], 0, 6, 64) == _lib.ERR_ARG and ok([-1], 0, 6, 64) == _lib.ERR_ARG                   # out of range
    assert ok([0, 1], 4, 6, 64) == _lib.ERR_ARG and ok([], 1, 6, 64) == _lib.ERR_ARG and ok([3], 2, 6, 32) == _lib.ERR_ARG   # outcome >= 2^k
    assert ok([0], 1, 6, 16) == _lib.ERR_ARG and ok([0], 1, -1, 64) == _lib.ERR_ARG and ok([0], 1, 41, 64) == _lib.ERR_ARG
    assert ok(list(range(40)), (1 << 40) - 1, 40, 64) == _lib.QSIM_OK and ok(list(range(40)), 1 << 40, 40, 64) == _lib.ERR_ARG
    wu, cu, wt, ct = c_uint64(), c_uint64(), c_long(), c_long()
    assert _lib.load().qsim_collapse_plan(_ints([0]), 1, 0, 6, 64, None, byref(cu), byref(wt), byref(ct)) == _lib.ERR_ARG  # raw: NULL for an out-parameter
    assert _lib.load().qsim_collapse_plan(_ints([0]), 1, 0, 6, 64, byref(wu), byref(cu), byref(wt), None) == _lib.ERR_ARG  # raw: NULL for an out-parameter
    w, d = (c_uint64 * 1)(), c_double()
    assert _lib.load().qsim_postselect(None, _ints([0]), 1, 0, byref(d)) == _lib.ERR_ARG    # the calls refuse a NULL state before anything else
    assert _lib.load().qsim_measure(None, _ints([0]), 1, 0.5, w, byref(d)) == _lib.ERR_ARG


# ---- the channels ---------------------------------------------------------------------------------------------------------------------
def test_channels_are_trace_preserving_and_known_values():
    for p in (0.0, 0.05, 0.3, 0.75, 1.0):
        for name, kraus, dim in (("bit_flip", channels.bit_flip(p), 2), ("phase_flip", channels.phase_flip(p), 2), ("depolarizing", channels.depolarizing(p), 2),
                                 ("amplitude_damping", channels.amplitude_damping(p), 2), ("phase_damping", channels.phase_damping(p), 2),
                                 ("two_qubit_depolarizing", channels.two_qubit_depolarizing(p), 4)):
            assert all(K.shape == (dim, dim) and K.dtype == np.complex128 for K in kraus), name
            gap = np.max(np.abs(sum(K.conj().T @ K for K in kraus) - np.eye(dim)))
            assert gap < 1e-12, (name, p, gap)
            assert len(channels.as_kraus_list(kraus, 1 if dim == 2 else 2)) == len(kraus)
    assert [len(f(0.1)) for f in (channels.bit_flip, channels.phase_flip, channels.depolarizing, channels.amplitude_damping, channels.phase_damping,
                                  channels.two_qubit_depolarizing)] == [2, 2, 4, 2, 2, 16]
    # depolarizing(3/4) sends every state to the fully mixed one
    rho = np.array([[0.7, 0.2 - 0.3j], [0.2 + 0.3j, 0.3]])
    out = sum(K @ rho @ K.conj().T for K in channels.depolarizing(0.75))
    assert np.max(np.abs(out - np.eye(2) / 2)) < 1e-15
    assert np.allclose(channels.depolarizing(0.3)[2], math.sqrt(0.1) * np.array([[0, -1j], [1j, 0]]))
    # amplitude_damping(gamma) moves gamma of |1>'s population to |0> and shrinks the coherence by sqrt(1 - gamma)
    out = sum(K @ rho @ K.conj().T for K in channels.amplitude_damping(0.36))
    assert np.allclose(out, [[0.7 + 0.36 * 0.3, 0.8 * (0.2 - 0.3j)], [0.8 * (0.2 + 0.3j), 0.64 * 0.3]], atol=1e-15)
    assert np.allclose(channels.amplitude_damping(0.36)[1], [[0, 0.6], [0, 0]])
    out = sum(K @ rho @ K.conj().T for K in channels.phase_damping(0.36))
    assert np.allclose(out, [[0.7, 0.8 * (0.2 - 0.3j)], [0.8 * (0.2 + 0.3j), 0.3]], atol=1e-15)
    # the two-qubit list: index 4 a + b is P_a on targets[1] and P_b on targets[0]
    ks = channels.two_qubit_depolarizing(0.3)
    assert np.allclose(ks[0], math.sqrt(0.7) * np.eye(4)) and np.allclose(ks[4 * 3 + 1], math.sqrt(0.02) * np.kron(channels.Z, channels.X))
    for bad in (lambda: channels.bit_flip(-0.1), lambda: channels.depolarizing(1.5), lambda: channels.amplitude_damping(float("nan")),
                lambda: channels.as_kraus_list([np.eye(2), 0.1 * channels.X], 1), lambda: channels.as_kraus_list([], 1),
                lambda: channels.as_kraus_list(channels.bit_flip(0.1), 2), lambda: channels.as_kraus_list([(1 + 2e-9) * np.eye(2)], 1)):
        with pytest.raises(ValueError):
            bad()
    assert len(channels.as_kraus_list([(1 + 1e-10) * np.eye(2)], 1)) == 1      # inside the tolerance of 1e-9
    assert channels.pick([0.0, 0.25, 0.0, 0.75], 0.0) == 1 and channels.pick([0.0, 0.25, 0.0, 0.75], 0.25) == 1
    assert channels.pick([0.0, 0.25, 0.0, 0.75], 0.2500001) == 3 and channels.pick([0.5, 0.5, 0.0], 1.0) == 1


# ---- the fp32 replay --------------------------------------------------------------------------------------------------------------------
def test_replay_error_is_inside_the_reference_cap_on_every_gpu_shape():
    worst = 0.0
    states = {}
    shapes = measure_ref.fp32_shapes() + [measure_ref.looping_cases(32)[0]]
    for n, qubits, outcome in shapes:
        if n not in states:
            states[n] = rand_state(n, 1140 + n).astype(np.complex64)
        held = states[n].astype(np.complex128)
        _, want = measure_ref.postselect(held, qubits, outcome)
        _, ref32 = measure_ref.postselect(held, qubits, outcome, dtype=np.complex64)
        assert ref32.dtype == np.complex64
        err = fp32_ref.rel_err(ref32, want)
        worst = max(worst, err)
        assert err <= fp32_ref.REF_CAP, (n, qubits, outcome, err)
    print(f"fp32 replay: worst rel_err {worst:.3e}")
    assert worst < 2.0 ** -22                                   # one rounding of the factor and one of each product
    for kraus, targets in ((channels.two_qubit_depolarizing(0.3), (1, 4)), (channels.amplitude_damping(0.4), (0,))):
        held = rand_state(6, 1150).astype(np.complex64).astype(np.complex128)
        for i, u in enumerate(measure_ref.midpoints(measure_ref.kraus_step(held, kraus, targets, 0.5)[3])):
            _, _, want, _ = measure_ref.kraus_step(held, kraus, targets, u)
            _, _, ref32, _ = measure_ref.kraus_step(held, kraus, targets, u, dtype=np.complex64)
            assert fp32_ref.rel_err(ref32, want) <= fp32_ref.REF_CAP, (targets, i)
