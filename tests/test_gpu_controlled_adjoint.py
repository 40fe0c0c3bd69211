"""Adjoint-mode gradients through controlled Pauli rotations on the device (qsim_controlled_pauli_gradient, csrc/cadjoint.hip;
Simulator.energy_and_gradient with (theta, string, controls) entries).

The checker is tests/controlled_adjoint_ref.py (numpy, pinned against dense operators and the four-term shift rule by
tests/test_controlled_adjoint_cpu.py) applied to the amplitudes READ BACK before the call.  The tolerances are those of
tests/test_gpu_adjoint.py.  fp64: |got - ref| < 1e-10 * sum|c_t| per gradient component and for the energy, and the state afterwards
within 1e-10 of the state before.  fp32: fp32_ref.check_fp32(got_grad, want64, ref32_grad) with ref32 the checker run in complex64,
C = 8 and FLOOR unchanged; the energy bound is the one copied into controlled_adjoint_ref's docstring; the state afterwards by the
two-sided rule of the rotation tests.  Every asserted gradient vector has a reference component above 1e-3."""
import ctypes
import functools

import numpy as np
import pytest

import controlled_adjoint_ref as ref
import controlled_rot_ref as crot
import fp32_ref
from fp32_ref import check_fp32, report
from gpu_quantum_simulator_amd import Simulator, _lib, plans

pytestmark = pytest.mark.gpu
TOL = ref.TOL
PRECISIONS = [64, 32]
UP = ctypes.POINTER(ctypes.c_uint64)
DP = ctypes.POINTER(ctypes.c_double)


def _bits(sim):
    return sim.read().view(np.uint64).copy()


def _run(sim, n, rotations, terms):
    return sim.energy_and_gradient(ref.entries(rotations, n), ref.term_texts(terms, n))


def _check(precision, energy, grad, before, rotations, terms, label, large=False, fp32_criterion=True):
    """`energy`, `grad` against the checker run from `before` (a state as read back); returns the fp64 gradient and, for fp32, the
    checker's complex64 gradient.  fp32_criterion=False: the caller gathers the components of several calls into one vector first."""
    e64, g64, final64 = ref.gradient(before, rotations, terms, large=large)
    g32 = finals = None
    if precision == 32:
        _, g32, final32 = ref.gradient(before.astype(np.complex64), rotations, terms, np.complex64, large=large)
        finals = (final32, final64) if len(rotations) else None
    worst = float(np.max(np.abs(grad - g64))) if len(rotations) else 0.0
    tol = ref.energy_tol(precision, terms, finals)
    print(f"{label} p{precision}: energy err {abs(energy - e64):.3e} (tol {tol:.3e}), gradient max abs err {worst:.3e}, max |grad| {np.max(np.abs(g64)):.3e}, "
          f"sum|c| {ref.weight(terms):.3f}")
    assert abs(energy - e64) < tol
    assert np.max(np.abs(g64)) > 1e-3  # not a comparison of zeros
    if precision == 64:
        assert worst < TOL * ref.weight(terms)
    elif fp32_criterion:
        report(label, check_fp32(grad, g64, g32))
    return g64, g32


def _state_back(precision, after, before, rotations, label, large=False):
    """The state after the call against the state before it: fp64 < TOL; fp32 by the two-sided rule of the rotation tests with the
    complex64 replay of the rotations and of their inverses as ref32."""
    if precision == 64:
        worst = float(np.max(np.abs(after - before)))
        print(f"{label}: state after vs before, max abs {worst:.3e}")
        assert worst < TOL
    else:
        there_and_back = list(rotations) + [(-theta, c, x, z) for theta, c, x, z in rotations[::-1]]
        ref32 = (ref.large_replay if large else crot.replay)(before.astype(np.complex64), there_and_back, np.complex64)
        bound = 2 * fp32_ref.C * max(fp32_ref.rel_err(ref32, before), fp32_ref.FLOOR)
        print(f"{label}: state after vs before, rel err {fp32_ref.rel_err(after, before):.3e} (bound {bound:.3e})")
        assert fp32_ref.rel_err(after, before) <= bound


def _one_call(precision, n, start, rotations, terms, label, sweeps=None):
    """One call from `start` (None: a fresh |0...0>), everything checked; returns the gradient."""
    with Simulator(n, precision=precision) as sim:
        if start is None:
            before = np.zeros(1 << n, dtype=np.complex128)
            before[0] = 1.0
        else:
            sim.write(start)
            before = sim.read()
        count = plans.sweeps_launched("pauli_adjoint")
        energy, grad = _run(sim, n, rotations, terms)
        taken = plans.sweeps_launched("pauli_adjoint") - count
        after = sim.read()
    assert taken == ref.plan(rotations, terms, n, precision)[0], (label, taken)
    if sweeps is not None:
        assert taken == sweeps, (label, taken, sweeps)
    _check(precision, energy, grad, before, rotations, terms, label)
    _state_back(precision, after, before, rotations, label)
    return grad


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("n", ref.EXHAUSTIVE_SIZES)
def test_exhaustive_small_registers(n, precision):
    """Every assignment of {control, I, X, Y, Z} with a control, as one rotation list: n = 1 with its one control and the identity
    string, the one-unit fp32 register, every x / control adjacency."""
    _, start, rotations, terms = ref.exhaustive_case(n)
    assert len(rotations) == 5 ** n - 4 ** n
    _one_call(precision, n, start, rotations, terms, f"exhaustive n={n}")


@pytest.mark.parametrize("precision", PRECISIONS)
def test_every_control_position(precision):
    """One rotation per call: control {q} for every q on a paired and on a diagonal string — below the lane bits, on either side of
    the thread boundary, in the trip bits, at n - 1, and fp32 slot 0.  fp64 holds every component to its bound.  fp32 holds the
    components to the criterion together, as one vector, as test_gpu_adjoint.test_geometry_strings does: the criterion compares
    rel_err(got) with rel_err(ref32), and for ONE number rel_err(ref32) is a single draw of a rounding error around zero, not a
    measure of its scale — the quotient of two such draws exceeds 8 in about one case in twelve whatever the kernel does (on the
    device the 26 single components gave bound_ratio 0.15 to 9.04; control {11}, diagonal: 1.11e-6 against 1.23e-7, on a gradient
    of 1.6e-3 whose absolute error is 1.8e-9; together, as one vector: 1.14).  Each component's quotient is printed."""
    n, start, rotations, terms = ref.position_case()
    assert {c for _, c, _, _ in rotations} == {1 << q for q in range(n)}
    got, want, ref32 = [], [], []
    with Simulator(n, precision=precision) as sim:
        for k, rot in enumerate(rotations):
            sim.write(start)
            before = sim.read()
            count = plans.sweeps_launched("pauli_adjoint")
            energy, grad = _run(sim, n, [rot], terms)
            assert plans.sweeps_launched("pauli_adjoint") - count == 1
            after = sim.read()
            label = f"control {{{k // 2}}} {'diagonal' if k % 2 else 'paired'}"
            g64, g32 = _check(precision, energy, grad, before, [rot], terms, label, fp32_criterion=False)
            if precision == 32:
                report(label + " (one component, not asserted)", (fp32_ref.rel_err(grad, g64), fp32_ref.rel_err(g32, g64)))
            _state_back(precision, after, before, [rot], f"control {{{k // 2}}}")
            got.append(grad[0]), want.append(g64[0]), ref32.append(g32[0] if precision == 32 else 0.0)
    if precision == 32:
        report("controlled adjoint, every control position", check_fp32(np.array(got), np.array(want), np.array(ref32)))


@pytest.mark.parametrize("precision", PRECISIONS)
def test_every_position_in_one_call(precision):
    n, start, rotations, terms = ref.one_call_position_case()
    _one_call(precision, n, start, rotations, terms, "every position, one call")


@pytest.mark.parametrize("precision", PRECISIONS)
def test_gate_queue_forwards_sweep_backwards(precision):
    n, start, rotations, terms = ref.gate_case()
    assert all(crot.takes_the_gate_queue(c, x, z) and c for _, c, x, z in rotations)
    assert crot.plan(rotations, n, precision)[:2] == (0, len(rotations))  # forwards: no sweep
    _one_call(precision, n, start, rotations, terms, "gates", len(rotations))  # backwards: every term, no two share (c, x)


@pytest.mark.parametrize("precision", PRECISIONS)
def test_slots(precision):
    """A control on qubit 0 (fp32: only the odd slot of a unit enters the sums and is rotated) and x = 1 beside a control on qubit 1."""
    n, start, rotations, terms = ref.slot_case()
    assert any(c & 1 for _, c, _, _ in rotations) and any(x == 1 and c & 2 for _, c, x, _ in rotations)
    _one_call(precision, n, start, rotations, terms, "slots")


@pytest.mark.parametrize("precision", PRECISIONS)
def test_several_controls_and_every_weight(precision):
    n, start, rotations, terms = ref.several_case()
    assert {bin(c).count("1") for _, c, _, _ in rotations} == set(range(2, n + 1))
    _one_call(precision, n, start, rotations, terms, "several controls")


@pytest.mark.parametrize("precision", PRECISIONS)
def test_runs(precision):
    """Runs longer than K are cut into ceil(len / K) sweeps; a change of control mask ends a run, as the plan says."""
    K = plans.pauli_rotations_per_sweep()
    for label, (rotations, sweeps) in ref.run_cases(K).items():
        _one_call(precision, ref.RUN_N, ref.rand_state(ref.RUN_N, 12), rotations, ref.run_hamiltonian(), label, sweeps)


@pytest.mark.parametrize("precision", PRECISIONS)
def test_order_inside_a_fused_run_matters(precision):
    n = ref.ORDER_N
    ab, ba, terms = ref.order_case()
    assert ab[1][1:3] == ab[2][1:3] and ab[1][1] != 0
    results = [_one_call(precision, n, ref.rand_state(n, 6), order, terms, "order", 3) for order in (ab, ba)]  # the pair shares its sweep
    swapped_back = results[1][[0, 2, 1, 3]]  # component k of both belongs to the same string
    assert np.max(np.abs(results[0] - swapped_back)) > 1e-2


@pytest.mark.parametrize("precision", PRECISIONS)
def test_fresh_zero_ket_ansatz(precision):
    """Y layers, CRY(q -> q + 1) — through the 4x4 of the gate queue forwards and a controlled sweep backwards — and a
    multi-controlled phase, from a never-touched register; the state is back at |0...0>."""
    n, rotations, terms = ref.ansatz_case()
    assert sum(1 for _, c, x, z in rotations if crot.takes_the_gate_queue(c, x, z) and c) >= n - 1
    assert any(x == 0 and z == 0 and bin(c).count("1") == 3 for _, c, x, z in rotations)
    _one_call(precision, n, None, rotations, terms, "ansatz from |0...0>")


@pytest.mark.parametrize("precision", PRECISIONS)
def test_against_the_four_term_rule_on_the_device(precision):
    """Independent of numpy: the four-term rule from apply_pauli_rotations + expectation.  The tolerance is
    test_gpu_adjoint.test_against_the_shift_rule_on_the_device's; the rule's weights add up to 1 as the two-term rule's do."""
    n = ref.SHIFT_N
    rotations, terms, which = ref.shift_case(n)
    start = ref.rand_state(n, 99)
    texts = ref.term_texts(terms, n)
    tol = (TOL if precision == 64 else fp32_ref.C * len(rotations) * 2.0 ** -24) * ref.weight(terms)
    with Simulator(n, precision=precision) as sim:
        sim.write(start)
        _, grad = _run(sim, n, rotations, terms)

        def energy_of(shift, k):
            theta, c, x, z = rotations[k]
            sim.write(start)
            sim.apply_pauli_rotations(ref.entries(rotations[:k] + [(theta + shift, c, x, z)] + rotations[k + 1:], n))
            return sim.expectation(texts)

        for k in which:
            assert rotations[k][1] != 0
            four = ref.shift4(lambda s: energy_of(s, k))
            print(f"p{precision} component {k}: adjoint {grad[k]:+.9e}, four-term rule on the device {four:+.9e}")
            assert abs(grad[k] - four) < tol
    assert max(abs(grad[k]) for k in which) > 1e-3


@functools.lru_cache(maxsize=None)
def _uncontrolled():
    return ref.uncontrolled_case()


def _c_call(lib, fn, h, cs, rotations, terms, energy=True, grad=True):
    """The C entry points with mask arrays: fn = "controlled" (cs: an array, or None for a NULL rot_c) or "plain"."""
    xs, zs = (np.array([r[i] for r in rotations], dtype=np.uint64) for i in (2, 3))
    th = np.array([r[0] for r in rotations], dtype=np.float64)
    hx, hz = (np.array([t[i] for t in terms], dtype=np.uint64) for i in (1, 2))
    co = np.array([t[0] for t in terms], dtype=np.float64)
    e, g = ctypes.c_double(7.0), np.full(len(rotations), 7.0)
    tail = (xs.ctypes.data_as(UP), zs.ctypes.data_as(UP), th.ctypes.data_as(DP), xs.size, hx.ctypes.data_as(UP), hz.ctypes.data_as(UP), co.ctypes.data_as(DP), hx.size,
            ctypes.byref(e) if energy else None, g.ctypes.data_as(DP) if grad else None)
    if fn == "plain":
        rc = lib.qsim_pauli_gradient(h, *tail)
    else:
        rc = lib.qsim_controlled_pauli_gradient(h, None if cs is None else cs.ctypes.data_as(UP), *tail)
    return rc, e.value, g


@pytest.mark.parametrize("precision", PRECISIONS)
def test_without_controls_the_bits_of_the_uncontrolled_call(precision):
    n = ref.BITS_N
    rotations, terms = _uncontrolled()
    start = ref.rand_state(n, 13)
    lib = _lib.load()
    out = []
    for fn, cs in (("plain", None), ("controlled", None), ("controlled", np.zeros(len(rotations), dtype=np.uint64))):
        with Simulator(n, precision=precision) as sim:
            sim.write(start)
            rc, energy, grad = _c_call(lib, fn, sim._h, cs, rotations, terms)
            _lib.check(rc)
            out.append((np.float64(energy).view(np.uint64), grad.view(np.uint64).copy(), _bits(sim)))
    assert np.max(np.abs(out[0][1].view(np.float64))) > 1e-3
    for other in out[1:]:
        assert out[0][0] == other[0] and np.array_equal(out[0][1], other[1]) and np.array_equal(out[0][2], other[2])


@pytest.mark.parametrize("precision", PRECISIONS)
def test_equal_calls_equal_bits_and_the_rest_of_the_state_keeps_its_bits(precision):
    """Equal bits under grid_cap 0, 3 and 1 << 30 and with lambda in a lent spare buffer; every rotation is controlled on qubit 11 (among
    others), so the amplitudes with bit 11 clear keep their exact bits through the call."""
    n = ref.BITS_N
    rotations, terms = ref.under_qubit_11_case()
    assert all(c >> 11 & 1 for _, c, _, _ in rotations)
    start = ref.weighted_state(n, 13, 1 << 11)
    out = []
    for cap, lend in ((0, False), (0, False), (3, False), (1 << 30, False), (0, True)):
        with Simulator(n, precision=precision, grid_cap=cap) as sim, Simulator(n, precision=precision) as lender:
            sim.write(start)
            before_bits, before = _bits(sim), sim.read()
            if lend:  # lambda in a lent spare buffer instead of the state's own: the same arithmetic
                ptr = lender.device_ptr
                lender.sync()
                sim.set_spare_buffer(ptr)
            energy, grad = _run(sim, n, rotations, terms)
            out.append((np.float64(energy).view(np.uint64), grad.view(np.uint64).copy(), _bits(sim)))
            if lend:
                sim.set_spare_buffer(None)
            if len(out) == 1:
                _check(precision, energy, grad, before, rotations, terms, "under qubit 11")
    for other in out[1:]:
        assert out[0][0] == other[0] and np.array_equal(out[0][1], other[1]) and np.array_equal(out[0][2], other[2])
    outside = (np.arange(1 << n) >> 11 & 1) == 0
    assert np.array_equal(out[0][2].reshape(-1, 2)[outside], before_bits.reshape(-1, 2)[outside])
    assert not np.array_equal(out[0][2].reshape(-1, 2)[~outside], before_bits.reshape(-1, 2)[~outside])  # inside: rounding moved it


@pytest.mark.parametrize("precision", PRECISIONS)
def test_where_the_sweep_loops(precision):
    """n = 22: the reducing grid holds at most 1024 workgroups of 256 threads, a paired trip takes 2 units per thread (2^19 units per
    round of the grid against the 2^20 of a paired sweep under one control) and a diagonal trip 4 (2^20 against 2^21): every
    workgroup walks its grid-stride loop at least twice, under a control above every other bit and under one below the lane bits."""
    n, rotations, terms = ref.loop_case()
    assert n == 22 and [c for _, c, _, _ in rotations] == [1 << 21, 1 << 21, 1 << 2, 1 << 2]
    assert ref.plan(rotations, terms, n, precision) == (4, 3, 2 * ((1 << 20) + (1 << 21)) >> (precision == 32))
    with Simulator(n, precision=precision) as sim:
        sim.write(ref.loop_state())
        before = sim.read()
        count = plans.sweeps_launched("pauli_adjoint")
        energy, grad = _run(sim, n, rotations, terms)
        assert plans.sweeps_launched("pauli_adjoint") - count == 4
        after = sim.read()
    _check(precision, energy, grad, before, rotations, terms, "n=22", large=True)
    _state_back(precision, after, before, rotations, "n=22", large=True)


@pytest.mark.parametrize("precision", PRECISIONS)
def test_errors_and_edge_cases(precision):
    lib = _lib.load()
    n = 5
    rotations = [(0.3, 1 << 3, 1, 0b10), (0.4, 0, 0b10, 0b10)]
    terms = [(0.3, 1, 1), (0.4, 2, 2)]
    assert _c_call(lib, "controlled", None, np.array([8, 0], dtype=np.uint64), rotations, terms)[0] == _lib.ERR_ARG and b"NULL" in lib.qsim_last_error()
    with Simulator(n, precision=precision) as sim:
        sim.write(ref.rand_state(n, 5))
        before = _bits(sim)
        h = sim._h
        # a control that names a qubit of the string (x, then z), a control at or above n: refused, nothing applied
        for cs, word in (([1, 0], "Pauli factor"), ([2, 0], "Pauli factor"), ([8, 2], "Pauli factor"), ([1 << n, 0], "control qubit outside"), ([8, 1 << 63], "control qubit outside")):
            with pytest.raises(_lib.QsimError, match=word):
                _lib.check(_c_call(lib, "controlled", h, np.array(cs, dtype=np.uint64), rotations, terms)[0])
        # what qsim_pauli_gradient refuses
        with pytest.raises(_lib.QsimError, match="outside"):
            _lib.check(_c_call(lib, "controlled", h, np.array([8, 0], dtype=np.uint64), [(0.3, 0, 1 << n, 0), rotations[1]], terms)[0])
        with pytest.raises(_lib.QsimError, match="non-finite"):
            _lib.check(_c_call(lib, "controlled", h, np.array([8, 0], dtype=np.uint64), [(float("nan"), 8, 1, 0), rotations[1]], terms)[0])
        with pytest.raises(_lib.QsimError, match="negative"):
            _lib.check(lib.qsim_controlled_pauli_gradient(h, None, None, None, None, -1, None, None, None, 0, None, None))
        for bad in ([(0.1, "X0 Z1", (1,))], [(0.1, "X0", (0,))], [(0.1, "X0", (n,))], [(0.1, "X0", (2, 2))], [(0.1, "X0", (1,), 4)]):
            with pytest.raises(ValueError):
                sim.energy_and_gradient(bad, [(1.0, "Z0")])
        assert np.array_equal(_bits(sim), before)
        # NULL rot_c: no controls anywhere; energy or grad may be NULL; no rotation: the energy alone
        plain = [(t, 0, x, z) for t, _, x, z in rotations]
        rc, energy, grad = _c_call(lib, "controlled", h, None, plain, terms)
        _lib.check(rc)
        tol = TOL if precision == 64 else 2e-5  # each call leaves the state moved by the rounding of its rotations (test_gpu_adjoint)
        want_e, want_g, _ = ref.gradient(sim.read(), plain, terms)
        assert abs(energy - want_e) < tol and np.max(np.abs(grad - want_g)) < tol
        want_e, want_g, _ = ref.gradient(sim.read(), rotations, terms)
        cs = np.array([r[1] for r in rotations], dtype=np.uint64)
        rc, energy, grad = _c_call(lib, "controlled", h, cs, rotations, terms, energy=False)
        _lib.check(rc)
        assert energy == 7.0 and np.max(np.abs(grad - want_g)) < tol and np.max(np.abs(want_g)) > 1e-3
        rc, energy, grad = _c_call(lib, "controlled", h, cs, rotations, terms, grad=False)
        _lib.check(rc)
        assert abs(energy - want_e) < tol and np.all(grad == 7.0)
        count = plans.sweeps_launched("pauli_adjoint")
        rc, energy, grad = _c_call(lib, "controlled", h, cs[:0], [], terms)
        _lib.check(rc)
        assert abs(energy - sim.expectation(ref.term_texts(terms, n))) < tol and plans.sweeps_launched("pauli_adjoint") == count
        energy, grad = sim.energy_and_gradient([], [])
        assert energy == 0.0 and grad.size == 0
        # a shard that holds nothing: energy 0, gradient zeros, no sweep, the state untouched
        sim.reset(holds_index0=False)
        count = plans.sweeps_launched("pauli_adjoint")
        energy, grad = sim.energy_and_gradient(ref.entries(rotations, n), ref.term_texts(terms, n))
        assert energy == 0.0 and grad.size == 2 and not grad.any() and plans.sweeps_launched("pauli_adjoint") == count and sim.get_support()[1:] == (1, 0.0)
