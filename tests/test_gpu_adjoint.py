"""Adjoint-mode gradients of <H> for circuits of Pauli rotations on the device (qsim_pauli_gradient, qsim_pauli_sum_into,
csrc/adjoint.hip).

The checker is tests/adjoint_ref.py (numpy, pinned against the shift rule and dense operators by tests/test_adjoint_cpu.py) applied to
the amplitudes READ BACK before the call — for an fp32 state `read()` is the exact widened contents, so state rounding cancels.
fp64: |got - ref| < 1e-10 * sum|c_t| per gradient component and for the energy: the project's parity tolerance scaled by the
operator's weight, as test_evolve_ising scales its bound (rounding stays near 1e-13, a sign or pairing mistake shows at 1e-2).
fp32: fp32_ref.check_fp32(got_grad, want64, ref32_grad) with ref32 the checker run in complex64 (inner products in fp64, as on the
device); C = 8 and FLOOR carry over: one backward term rounds each amplitude of psi and of lambda about as often as one term of the
replay does.  The fp32 ENERGY is <lambda|psi> in fp64 of a lambda that was accumulated in fp32: each of the T + 1 roundings of an
amplitude of lambda is at most 2^-24 of a partial sum bounded by sum|c_t| |psi_partner|, so by Cauchy-Schwarz on a unit state
|E - E_exact(forward state)| <= (T + 1) 2^-24 sum|c_t|; the tests assert (T + 2) 2^-24 sum|c_t| against the expectation sweep on
the same forward state.  Against the fp64 checker, which replays the rotations in fp64, the fp32 forward state's own error comes on
top: the rotation tests hold it to f = C max(rel_err(complex64 replay), FLOOR), and it moves <H> by at most 2 f sum|c_t|.
"""
import ctypes
import functools
import math

import numpy as np
import pytest

import adjoint_ref as ref
import fp32_ref
import pauli_ref
import pauli_rot_ref
from fp32_ref import check_fp32, report
from gpu_quantum_simulator_amd import Simulator, _lib, plans

pytestmark = pytest.mark.gpu
TOL = 1e-10
PRECISIONS = [64, 32]
UP = ctypes.POINTER(ctypes.c_uint64)
DP = ctypes.POINTER(ctypes.c_double)


def _plan(rotations, terms):
    p = plans.ok(plans.pauli_gradient_plan([x for _, x, _ in rotations], [x for _, x, _ in terms]))
    return p["adjoint_sweeps"], p["sum_sweeps"]


def _bits(sim):
    return sim.read().view(np.uint64).copy()


def _energy_tol(precision, terms, before=None, rotations=()):
    """The module docstring's bound; `before`, `rotations`: the energy is compared with the fp64 replay from `before`."""
    if precision == 64:
        return TOL * ref.weight(terms)
    forward = 0.0
    if len(rotations):
        want = pauli_rot_ref.replay(before, list(rotations))
        forward = fp32_ref.C * max(fp32_ref.rel_err(pauli_rot_ref.replay(before.astype(np.complex64), list(rotations), np.complex64), want), fp32_ref.FLOOR)
    return ((len(terms) + 2) * 2.0 ** -24 + 2.0 * forward) * ref.weight(terms)


def _run(sim, n, rotations, terms):
    return sim.energy_and_gradient(pauli_rot_ref.texts(rotations, n), ref.term_texts(terms, n))


def _check(precision, energy, grad, before, rotations, terms, label):
    """`energy`, `grad` against the checker run from `before` (a state as read back); returns the fp64 gradient and the largest
    error the criterion allows one component (fp32: the whole vector's bound)."""
    e64, g64, _ = ref.gradient(before, rotations, terms)
    worst = float(np.max(np.abs(grad - g64))) if len(rotations) else 0.0
    tol = _energy_tol(precision, terms, before, rotations)
    print(f"{label} p{precision}: energy err {abs(energy - e64):.3e} (tol {tol:.3e}), gradient max abs err {worst:.3e}, sum|c| {ref.weight(terms):.3f}")
    assert abs(energy - e64) < tol
    if precision == 64:
        assert worst < TOL * ref.weight(terms)
        return g64, TOL * ref.weight(terms)
    _, g32, _ = ref.gradient(before.astype(np.complex64), rotations, terms, np.complex64)
    report(label, check_fp32(grad, g64, g32))
    return g64, fp32_ref.C * max(fp32_ref.rel_err(g32, g64), fp32_ref.FLOOR) * float(np.linalg.norm(g64))


def _state_back(precision, after, before, rotations, label):
    """The state after the call against the state before it: fp64 < TOL; fp32 by the two-sided rule of the rotation tests
    (test_gpu_pauli_rot._close) with the complex64 replay of the rotations and of their inverses as ref32."""
    if precision == 64:
        worst = float(np.max(np.abs(after - before)))
        print(f"{label}: state after vs before, max abs {worst:.3e}")
        assert worst < TOL
    else:
        there_and_back = rotations + [(-theta, x, z) for theta, x, z in rotations[::-1]]
        ref32 = pauli_rot_ref.replay(before.astype(np.complex64), there_and_back, np.complex64)
        bound = 2 * fp32_ref.C * max(fp32_ref.rel_err(ref32, before), fp32_ref.FLOOR)
        print(f"{label}: state after vs before, rel err {fp32_ref.rel_err(after, before):.3e} (bound {bound:.3e})")
        assert fp32_ref.rel_err(after, before) <= bound


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("n", [1, 2, 9])
def test_geometry_strings(n, precision):
    """One parameter per call; the components of one register size are held to the fp32 criterion together, as one vector."""
    terms = ref.random_hamiltonian(n, 6, 300 + n, 2)
    got, want, ref32 = [], [], []
    with Simulator(n, precision=precision) as sim:
        sim.write(pauli_rot_ref.rand_state(n, 70 + n))
        for x, z in ref.geometry_strings(n):
            rot = [(0.7, x, z)]
            before = sim.read()
            count = plans.sweeps_launched("pauli_adjoint")
            energy, grad = _run(sim, n, rot, terms)
            assert plans.sweeps_launched("pauli_adjoint") - count == 1
            e64, g64, _ = ref.gradient(before, rot, terms)
            _, g32, _ = ref.gradient(before.astype(np.complex64), rot, terms, np.complex64)
            print(f"n={n} p{precision} {pauli_ref.masks_to_text(x, z, n)!r}: grad {grad[0]:+.9e} want {g64[0]:+.9e}, energy err {abs(energy - e64):.3e}")
            assert abs(energy - e64) < _energy_tol(precision, terms, before, rot)
            if precision == 64:
                assert abs(grad[0] - g64[0]) < TOL * ref.weight(terms)
            _state_back(precision, sim.read(), before, rot, f"geometry n={n}")
            got.append(grad[0]), want.append(g64[0]), ref32.append(g32[0])
    assert max(abs(g) for g in want) > 1e-3  # not a comparison of zeros
    if precision == 32:
        report(f"adjoint geometry n={n}", check_fp32(np.array(got), np.array(want), np.array(ref32)))


@functools.lru_cache(maxsize=None)
def _every_weight():
    return ref.every_weight_case(13)


@pytest.mark.parametrize("precision", PRECISIONS)
def test_every_weight(precision):
    n = 13
    rotations, terms = _every_weight()
    assert {bin(x | z).count("1") for _, x, z in rotations} == set(range(0, n + 1))
    assert max(np.bincount([sorted({x for _, x, _ in terms}).index(x) for _, x, _ in terms])) >= 7  # one x group of H has several terms
    with Simulator(n, precision=precision) as sim:
        sim.write(pauli_rot_ref.rand_state(n, 13))
        before = sim.read()
        count = plans.sweeps_launched("pauli_adjoint")
        energy, grad = _run(sim, n, rotations, terms)
        assert plans.sweeps_launched("pauli_adjoint") - count == _plan(rotations, terms)[0]
        after = sim.read()
    g64, component_tol = _check(precision, energy, grad, before, rotations, terms, "every weight n=13")
    identity = [k for k, (_, x, z) in enumerate(rotations) if x == 0 and z == 0]
    assert len(identity) == 1 and abs(g64[identity[0]]) < 1e-14 and abs(grad[identity[0]]) < component_tol  # a global phase
    assert np.max(np.abs(g64)) > 1e-3
    _state_back(precision, after, before, rotations, "every weight n=13")


@pytest.mark.parametrize("precision", PRECISIONS)
def test_order_inside_a_run_matters(precision):
    n = 6
    ab, ba, terms = ref.order_case()
    assert ab[1][1] == ab[2][1] and _plan(ab, terms)[0] == 3
    results = []
    for order in (ab, ba):
        with Simulator(n, precision=precision) as sim:
            sim.write(pauli_rot_ref.rand_state(n, 6))
            before = sim.read()
            count = plans.sweeps_launched("pauli_adjoint")
            energy, grad = _run(sim, n, order, terms)
            assert plans.sweeps_launched("pauli_adjoint") - count == 3  # the pair shares its sweep
            _check(precision, energy, grad, before, order, terms, "order")
            results.append(grad)
    swapped_back = results[1][[0, 2, 1, 3]]  # component k of both belongs to the same string
    assert np.max(np.abs(results[0] - swapped_back)) > 1e-2


@pytest.mark.parametrize("precision", PRECISIONS)
def test_runs_longer_than_k(precision):
    n = 12
    K = plans.pauli_rotations_per_sweep()
    diag, paired = pauli_rot_ref.long_run_rotations(K)
    terms = ref.random_hamiltonian(n, 10, 1200, 2)
    with Simulator(n, precision=precision) as sim:
        sim.write(pauli_rot_ref.rand_state(n, 12))
        for label, run in (("diagonal", diag), ("paired", paired), ("both", diag + paired)):
            before = sim.read()
            count = plans.sweeps_launched("pauli_adjoint")
            energy, grad = _run(sim, n, run, terms)
            taken = plans.sweeps_launched("pauli_adjoint") - count
            assert taken == _plan(run, terms)[0] == -(-len(diag) // K) * (len(run) // len(diag)), (label, taken)
            _check(precision, energy, grad, before, run, terms, f"run of {len(run)} {label}")
            _state_back(precision, sim.read(), before, run, f"run of {len(run)} {label}")


@pytest.mark.parametrize("precision", PRECISIONS)
def test_energy_is_the_expectation_on_the_forward_state(precision):
    n = 9
    rotations, terms, _ = ref.shift_case(n)
    start = pauli_rot_ref.rand_state(n, 9)
    with Simulator(n, precision=precision) as sim, Simulator(n, precision=precision) as twin:
        sim.write(start), twin.write(start)
        twin.apply_pauli_rotations(pauli_rot_ref.texts(rotations, n))
        want = twin.expectation(ref.term_texts(terms, n))
        energy, _ = _run(sim, n, rotations, terms)
        only_energy, none = _run(sim, n, [], terms)  # no rotation: the energy of the state as it is
        here = sim.expectation(ref.term_texts(terms, n))
    print(f"p{precision}: energy {energy:.12f} vs expectation on the forward state {want:.12f}")
    assert abs(energy - want) < _energy_tol(precision, terms)
    assert none.size == 0 and abs(only_energy - here) < _energy_tol(precision, terms)


@pytest.mark.parametrize("precision", PRECISIONS)
def test_fresh_zero_ket_ansatz(precision):
    n = 13
    rotations, terms = ref.ansatz_case(n)
    ket0 = np.zeros(1 << n, dtype=np.complex128)
    ket0[0] = 1.0
    with Simulator(n, precision=precision) as sim:  # never touched: |0...0> is still held lazily
        energy, grad = _run(sim, n, rotations, terms)
        after = sim.read()
    g64, _ = _check(precision, energy, grad, ket0, rotations, terms, "ansatz from |0...0>")
    assert np.max(np.abs(g64)) > 1e-3
    _state_back(precision, after, ket0, rotations, "ansatz from |0...0>")


@pytest.mark.parametrize("precision", PRECISIONS)
def test_against_the_shift_rule_on_the_device(precision):
    """Independent of numpy: [E(theta_k + pi/2) - E(theta_k - pi/2)] / 2 from apply_pauli_rotations + expectation.  Each fp32 energy
    carries the rounding of the rotations, about len(rotations) * 2^-24 of sum|c_t|; fp32_ref.C of that is allowed for the difference."""
    n = 9
    rotations, terms, which = ref.shift_case(n)
    start = pauli_rot_ref.rand_state(n, 99)
    texts = ref.term_texts(terms, n)
    tol = (TOL if precision == 64 else fp32_ref.C * len(rotations) * 2.0 ** -24) * ref.weight(terms)
    with Simulator(n, precision=precision) as sim:
        sim.write(start)
        _, grad = _run(sim, n, rotations, terms)
        for k in which:
            theta, x, z = rotations[k]
            e = []
            for shift in (0.5 * math.pi, -0.5 * math.pi):
                sim.write(start)
                sim.apply_pauli_rotations(pauli_rot_ref.texts(rotations[:k] + [(theta + shift, x, z)] + rotations[k + 1:], n))
                e.append(sim.expectation(texts))
            print(f"p{precision} component {k}: adjoint {grad[k]:+.9e}, shift rule on the device {0.5 * (e[0] - e[1]):+.9e}")
            assert abs(grad[k] - 0.5 * (e[0] - e[1])) < tol


@pytest.mark.parametrize("precision", PRECISIONS)
def test_equal_calls_equal_bits_whatever_the_grid_cap(precision):
    n = 13
    rotations, terms = _every_weight()
    start = pauli_rot_ref.rand_state(n, 13)
    out = []
    for cap, lend in ((0, False), (0, False), (3, False), (1 << 30, False), (0, True)):
        with Simulator(n, precision=precision, grid_cap=cap) as sim, Simulator(n, precision=precision) as lender:
            sim.write(start)
            if lend:  # lambda in a lent spare buffer instead of the state's own: the same arithmetic
                ptr = lender.device_ptr
                lender.sync()
                sim.set_spare_buffer(ptr)
            energy, grad = _run(sim, n, rotations, terms)
            out.append((np.float64(energy).view(np.uint64), grad.view(np.uint64).copy(), _bits(sim)))
            if lend:
                sim.set_spare_buffer(None)
    for other in out[1:]:
        assert out[0][0] == other[0] and np.array_equal(out[0][1], other[1]) and np.array_equal(out[0][2], other[2])


@pytest.mark.parametrize("precision", PRECISIONS)
def test_pauli_sum_into(precision):
    n = 9
    dtype = np.complex128 if precision == 64 else np.complex64
    with Simulator(n, precision=precision) as sim, Simulator(n, precision=precision) as dst:
        sim.write(pauli_rot_ref.rand_state(n, 19))
        psi = sim.read()
        for label, terms in ref.sum_cases(n).items():
            dst.write(np.full(1 << n, 3.0 - 2.0j))  # whatever was there is overwritten
            ptr = dst.device_ptr
            dst.sync()
            sim.pauli_sum_into(ref.term_texts(terms, n), ptr)
            sim.sync()
            got = dst.read()
            want = ref.apply_sum(psi, terms)
            if not terms:
                assert not got.any()
            elif precision == 64:
                worst = float(np.max(np.abs(got - want)))
                print(f"pauli_sum_into {label}: {len(terms)} terms, max abs err {worst:.3e}")
                assert worst < TOL * ref.weight(terms)
            else:
                report(f"pauli_sum_into {label}", check_fp32(got, want, ref.apply_sum(psi.astype(dtype), terms, dtype)))
        assert np.array_equal(sim.read(), psi)


@pytest.mark.parametrize("precision", PRECISIONS)
def test_errors_and_edge_cases(precision):
    lib = _lib.load()
    n = 5
    ok = np.array([1, 2], dtype=np.uint64)
    okp = ok.ctypes.data_as(UP)
    th = np.array([0.3, 0.4])
    thp = th.ctypes.data_as(DP)
    e, g = ctypes.c_double(), np.zeros(2)
    ep, gp = ctypes.byref(e), g.ctypes.data_as(DP)
    assert lib.qsim_pauli_gradient(None, okp, okp, thp, 2, okp, okp, thp, 2, ep, gp) == _lib.ERR_ARG and b"NULL" in lib.qsim_last_error()
    assert lib.qsim_pauli_sum_into(None, okp, okp, thp, 2, ctypes.c_void_p(64)) == _lib.ERR_ARG
    with Simulator(n, precision=precision) as sim, Simulator(n, precision=precision) as other:
        sim.write(pauli_rot_ref.rand_state(n, 5))
        before = _bits(sim)
        h = sim._h
        other_ptr = other.device_ptr
        other.sync()

        def grad_call(rx=okp, rz=okp, t=thp, nr=2, hx=okp, hz=okp, c=thp, nh=2):
            return lib.qsim_pauli_gradient(h, rx, rz, t, nr, hx, hz, c, nh, ep, gp)

        for bad_x, bad_z in (([1, 1 << n], [0, 0]), ([1, 2], [0, 1 << 63])):  # a mask bit at or above n, in either list
            bx, bz = np.array(bad_x, dtype=np.uint64).ctypes.data_as(UP), np.array(bad_z, dtype=np.uint64).ctypes.data_as(UP)
            for rc in (grad_call(rx=bx, rz=bz), grad_call(hx=bx, hz=bz), lib.qsim_pauli_sum_into(h, bx, bz, thp, 2, ctypes.c_void_p(other_ptr))):
                with pytest.raises(_lib.QsimError, match="outside"):
                    _lib.check(rc)
        for kw in ({"rx": None}, {"rz": None}, {"t": None}, {"hx": None}, {"hz": None}, {"c": None}):
            with pytest.raises(_lib.QsimError, match="NULL"):
                _lib.check(grad_call(**kw))
        for args in ((None, okp, thp), (okp, None, thp), (okp, okp, None)):
            with pytest.raises(_lib.QsimError, match="NULL"):
                _lib.check(lib.qsim_pauli_sum_into(h, *args, 2, ctypes.c_void_p(other_ptr)))
        for rc in (grad_call(nr=-1), grad_call(nh=-1), lib.qsim_pauli_sum_into(h, okp, okp, thp, -1, ctypes.c_void_p(other_ptr))):
            with pytest.raises(_lib.QsimError, match="negative"):
                _lib.check(rc)
        for bad in (float("nan"), float("inf"), -float("inf")):
            bt = np.array([0.3, bad]).ctypes.data_as(DP)
            for rc in (grad_call(t=bt), grad_call(c=bt), lib.qsim_pauli_sum_into(h, okp, okp, bt, 2, ctypes.c_void_p(other_ptr))):
                with pytest.raises(_lib.QsimError, match="non-finite"):
                    _lib.check(rc)
        # the destination of a sum: not NULL, not the state's buffer, not its spare buffer
        for dst in (None, sim.device_ptr):
            with pytest.raises(_lib.QsimError, match="destination"):
                _lib.check(lib.qsim_pauli_sum_into(h, okp, okp, thp, 2, ctypes.c_void_p(dst)))
        sim.set_spare_buffer(other_ptr)
        with pytest.raises(_lib.QsimError, match="destination"):
            _lib.check(lib.qsim_pauli_sum_into(h, okp, okp, thp, 2, ctypes.c_void_p(other_ptr)))
        sim.set_spare_buffer(None)
        with pytest.raises(ValueError):
            sim.energy_and_gradient([(0.1, "X0")], [(1j, "Z0")])
        with pytest.raises(ValueError):
            sim.pauli_sum_into([(1j, "Z0")], other_ptr)
        with pytest.raises(ValueError):
            sim.energy_and_gradient([(0.1, f"X{n}")], [(1.0, "Z0")])
        assert np.array_equal(_bits(sim), before)  # nothing of a refused call was applied
        # energy or grad may be NULL; no terms at all is fine
        _lib.check(lib.qsim_pauli_gradient(h, okp, okp, thp, 2, okp, okp, thp, 2, None, gp))
        _lib.check(lib.qsim_pauli_gradient(h, okp, okp, thp, 2, okp, okp, thp, 2, ep, None))
        # (each call leaves the state moved by the rounding of its rotations: 2e-5 is test_gpu_pauli_rot.TOL32, a few hundred fp32 roundings)
        energy, grad = sim.energy_and_gradient([(0.3, "Y0"), (0.4, "Y1")], [(0.3, "Y0"), (0.4, "Y1")])  # the masks of `ok`: x = z
        assert abs(energy - e.value) < (TOL if precision == 64 else 2e-5) and np.max(np.abs(grad - g)) < (TOL if precision == 64 else 2e-5)
        energy, grad = sim.energy_and_gradient([(0.3, "Z0 Z1")], [])  # H = 0
        assert energy == 0.0 and grad[0] == 0.0
        energy, grad = sim.energy_and_gradient([], [])
        assert energy == 0.0 and grad.size == 0
        # a shard that holds nothing: energy 0, gradient zeros, no sweep, the state untouched
        sim.reset(holds_index0=False)
        count = plans.sweeps_launched("pauli_adjoint")
        energy, grad = sim.energy_and_gradient([(0.3, "Z0 Z1"), (0.2, "X0 X1")], [(1.0, "Z0"), (0.5, "X1")])
        assert energy == 0.0 and not grad.any() and plans.sweeps_launched("pauli_adjoint") == count and sim.get_support()[1:] == (1, 0.0)
