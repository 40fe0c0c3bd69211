"""Measurement on the device (Simulator.postselect, measure, reset_qubits, apply_channel; qsim_postselect, qsim_measure; csrc/measure.hip,
csrc/measure.cpp).

The checker is measure_ref (pinned on the CPU by tests/test_measure_cpu.py) on the amplitudes READ BACK from the same state before the
call — for an fp32 state `read()` is the exact widened contents.  fp64: max abs error < 1e-10 on a unit-norm result, the project's
tolerance.  fp32: fp32_ref.check_fp32(got, want64, ref32) with the complex64 replay of measure_ref.  W: within (kept + 8) 2^-52 W of
math.fsum over the widened squares (measure_ref.weight_tolerance has the derivation).  The discarded amplitudes: the +0.0 bit pattern.
Every accepted call raises the sweep counter by exactly 2, every refused one by 0 and leaves the state's bits alone.
Sizes: n <= 4 exhaustively, n = 13 for k = 1, 2, 5, 10, 13, and n = 22 (fp64) / 23 (fp32), where the plan call reports two trips per
workgroup of the collapse sweep at the default grid."""
import functools
import math
from ctypes import byref, c_double, c_uint64

import numpy as np
import pytest

import fp32_ref
import lazy_cases
import matrix_ref
import measure_ref
from gpu_quantum_simulator_amd import Circuit, Cluster, Simulator, _lib, channels, gate_matrix, plans
from gpu_quantum_simulator_amd._marshal import ints as _ints
from gpu_quantum_simulator_amd._lib import QsimError
from pauli_rot_ref import rand_state
from test_gpu_lazy_states import Side, _dense

pytestmark = pytest.mark.gpu
TOL = 1e-10
PRECISIONS = [64, 32]


def _bits(state):
    return np.ascontiguousarray(state).view(np.uint64)


def _check_state(got, before, qubits, outcome, precision, label):
    """The state after a collapse onto `outcome` against the checker on `before`; returns the checker's W."""
    W, want = measure_ref.postselect(before, qubits, outcome)
    n = int(got.size).bit_length() - 1
    discarded = ~measure_ref.kept_indices(n, qubits, outcome)
    assert not _bits(got[discarded]).any(), f"{label}: a discarded amplitude is not +0.0"
    if precision == 64:
        worst = float(np.max(np.abs(got - want)))
        print(f"measure {label}: max abs err {worst:.3e}")
        assert worst < TOL, label
    else:
        _, ref32 = measure_ref.postselect(before, qubits, outcome, dtype=np.complex64)
        fp32_ref.report(f"measure {label}", fp32_ref.check_fp32(got, want, ref32))
    return W


def _check_weight(got_w, want_w, kept, label):
    err, bound = abs(got_w - want_w), measure_ref.weight_tolerance(kept, want_w)
    print(f"measure {label}: W {got_w:.17g} against {want_w:.17g}, off by {err:.3e}, bound {bound:.3e}")
    assert err <= bound, label


def _postselect_and_check(sim, before, qubits, outcome, label=""):
    count = plans.sweeps_launched("collapse")
    W = sim.postselect(qubits, outcome)
    assert plans.sweeps_launched("collapse") == count + 2
    got = sim.read()
    label = f"n={sim.num_qubits} p{sim.precision} q={qubits} o={outcome} {label}"
    want_w = _check_state(got, before, qubits, outcome, sim.precision, label)
    _check_weight(W, want_w, 1 << (sim.num_qubits - len(qubits)), label)
    return W, got


def _sim_with(n, precision, seed, scale=1.0, **options):
    sim = Simulator(n, precision=precision, **options)
    sim.write(rand_state(n, seed) * scale)
    return sim, sim.read()


# ---- post-selection ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("n", [1, 2, 3, 4])
def test_postselect_exhaustively_on_small_registers(n, precision):
    sim, psi = _sim_with(n, precision, 1200 + n)
    with sim:
        for qubits, outcome in measure_ref.small_cases(n):
            sim.write(psi)
            _postselect_and_check(sim, psi, qubits, outcome)


@pytest.mark.parametrize("precision", PRECISIONS)
def test_postselect_n13(precision):
    sim, psi = _sim_with(measure_ref.N13, precision, 1210, scale=1.3)        # not normalised: the result is
    assert any(0 in q for q, _ in measure_ref.N13_CASES) and any(0 not in q for q, _ in measure_ref.N13_CASES)
    with sim:
        for qubits, outcome in measure_ref.N13_CASES:
            sim.write(psi)
            _postselect_and_check(sim, psi, qubits, outcome)
            assert sim.norm2() == pytest.approx(1.0, abs=1e-12 if precision == 64 else 1e-6)
        sim.write(psi)                                                     # no qubit: the state is normalised and nothing else
        _postselect_and_check(sim, psi, [], 0)


@functools.lru_cache(maxsize=None)
def _large_state(n):
    return rand_state(n, 1220)


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("which", [0, 1])
def test_looping_at_the_default_grid(which, precision):
    n, qubits, outcome = measure_ref.looping_cases(precision)[which]
    assert plans.ok(plans.collapse_plan(qubits, outcome, n, precision))["collapse_trips"] >= 2
    with Simulator(n, precision=precision) as sim:
        sim.write(_large_state(n))
        _postselect_and_check(sim, sim.read(), qubits, outcome)


@pytest.mark.parametrize("precision", PRECISIONS)
def test_equal_bits_whatever_the_grid(precision):
    n = measure_ref.N13
    start = rand_state(n, 1230)
    with Simulator(n, precision=precision) as sim:
        for qubits, outcome in measure_ref.GRID_CASES:
            results = []
            for grid_cap in measure_ref.GRID_CAPS:
                sim.set_option(_lib.OPT_GRID_CAP, grid_cap)
                sim.write(start)
                W = sim.postselect(qubits, outcome)
                results.append((W, _bits(sim.read()).copy()))
            assert all(np.float64(W).view(np.uint64) == np.float64(results[0][0]).view(np.uint64) for W, _ in results), (qubits, [W for W, _ in results])
            assert all(np.array_equal(state, results[0][1]) for _, state in results), qubits


@pytest.mark.parametrize("precision", PRECISIONS)
def test_the_discarded_part_is_never_read(precision):
    n = measure_ref.N13
    clean = rand_state(n, 1240)
    poison = np.array([complex(float("nan"), float("inf")), complex(float("-inf"), float("nan")), complex(float("inf"), 1.0)])
    with Simulator(n, precision=precision) as sim:
        for qubits, outcome in measure_ref.N13_CASES:
            keep = measure_ref.kept_indices(n, qubits, outcome)
            dirty = np.where(keep, clean, poison[np.arange(1 << n) % 3])
            sim.write(dirty)                                               # a plain copy: the buffer holds NaN and Inf outside the kept subspace
            held = np.where(keep, sim.read(), 0.0)                           # what the kept part holds, zeros elsewhere for the checker
            count = plans.sweeps_launched("collapse")
            W = sim.postselect(qubits, outcome)
            assert plans.sweeps_launched("collapse") == count + 2 and math.isfinite(W)
            got = sim.read()
            assert np.isfinite(got.real).all() and np.isfinite(got.imag).all(), (qubits, outcome)
            label = f"poisoned p{precision} q={qubits} o={outcome}"
            _check_weight(W, _check_state(got, held, qubits, outcome, precision, label), 1 << (n - len(qubits)), label)


# ---- measurement ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("qubits", measure_ref.MEASURE_CASES, ids=["k3", "k10"])
def test_measure_agrees_with_the_sampler(qubits, precision):
    n = measure_ref.MEASURE_N
    sim, psi = _sim_with(n, precision, 1250, scale=math.sqrt(3.0))           # norm^2 = 3
    total = math.fsum(np.concatenate((psi.real ** 2, psi.imag ** 2)))
    assert abs(total - 3.0) < 1e-5
    with sim:
        for i in range(64):
            u = (i + 0.5) / 64
            sim.write(psi)
            drawn = int(sim.sample_shots(draws=[u], qubits=qubits)[0])
            count = plans.sweeps_launched("collapse")
            outcome, p = sim.measure(qubits, draw=u, return_probability=True)
            assert plans.sweeps_launched("collapse") == count + 2
            assert outcome == drawn, (u, outcome, drawn)
            assert outcome in measure_ref.admissible_outcomes(n, psi, u, qubits), (u, outcome)
            got = sim.read()
            label = f"n={n} p{precision} k={len(qubits)} u={u}"
            W = _check_state(got, psi, qubits, outcome, precision, label)
            err, bound = abs(p - W / total), measure_ref.weight_tolerance(1 << (n - len(qubits)), W / total)
            print(f"measure {label}: p {p:.17g} against {W / total:.17g}, off by {err:.3e}, bound {bound:.3e}")
            assert err <= bound, label
            assert abs(sim.norm2() - 1.0) <= (1e-12 if precision == 64 else 1e-6), label
        sim.write(psi)                                                     # the draw comes from the seed the way sample_shots draws
        drawn = int(sim.sample_shots(1, qubits, seed=77)[0])
        assert sim.measure(qubits, seed=77) == drawn
        assert sim.measure(qubits, draw=0.3) == drawn                      # measured again, the collapsed state reads the same whatever the draw


# ---- refusals -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", PRECISIONS)
def test_refusals(precision):
    lib = _lib.load()
    for method in ("postselect", "measure", "reset_qubits", "apply_channel"):
        assert hasattr(Simulator, method) and not hasattr(Cluster, method)
    n = 12
    with Simulator(n, precision=precision) as sim:
        psi = rand_state(n, 1260)
        psi[(np.arange(1 << n) & 0b100000100) == 0b100000000] = 0.0          # qubit 8 one and qubit 2 zero never happens
        sim.write(psi)
        state = _bits(sim.read()).copy()
        before = plans.sweeps_launched("collapse")
        with pytest.raises(QsimError) as err:                              # an outcome of probability zero
            sim.postselect([2, 8], 0b10)
        assert err.value.code == _lib.ERR_ARG and "probability zero" in str(err.value)
        assert plans.sweeps_launched("collapse") == before and np.array_equal(_bits(sim.read()), state)
        for bad in (lambda: sim.postselect([0, 0], 0), lambda: sim.postselect([2, 5, 2], 1), lambda: sim.postselect([n], 0), lambda: sim.postselect([-1], 0),
                    lambda: sim.postselect(list(range(n)) + [3], 0), lambda: sim.postselect([0, 1], 4), lambda: sim.postselect([], 1),
                    lambda: sim.measure([0, 0], draw=0.5), lambda: sim.measure([n], draw=0.5), lambda: sim.measure([0], draw=1.5),
                    lambda: sim.measure([0], draw=-0.1), lambda: sim.measure([0], draw=float("nan")), lambda: sim.reset_qubits([3, 3], draw=0.5)):
            with pytest.raises(QsimError) as err:
                bad()
            assert err.value.code == _lib.ERR_ARG
        with pytest.raises(ValueError):
            sim.measure([0], seed=1, draw=0.5)
        out, w = c_uint64(), c_double()
        assert lib.qsim_postselect(sim._h, None, 1, 0, byref(w)) == _lib.ERR_ARG and lib.qsim_postselect(sim._h, _ints([0]), -1, 0, byref(w)) == _lib.ERR_ARG
        assert lib.qsim_postselect(sim._h, _ints([0]), 1, 0, None) == _lib.ERR_ARG and lib.qsim_postselect(None, _ints([0]), 1, 0, byref(w)) == _lib.ERR_ARG
        assert lib.qsim_measure(sim._h, _ints([0]), 1, 0.5, None, byref(w)) == _lib.ERR_ARG and lib.qsim_measure(sim._h, _ints([0]), 1, 0.5, byref(out), None) == _lib.ERR_ARG
        assert lib.qsim_measure(sim._h, _ints(list(range(n + 1))), n + 1, 0.5, byref(out), byref(w)) == _lib.ERR_ARG
        assert plans.sweeps_launched("collapse") == before
        assert np.array_equal(_bits(sim.read()), state)
        sim.reset(holds_index0=False)                                      # a state that holds nothing: every outcome has probability zero
        for bad in (lambda: sim.postselect([0], 0), lambda: sim.measure([0], draw=0.5), lambda: sim.postselect([], 0)):
            with pytest.raises(QsimError) as err:
                bad()
            assert err.value.code == _lib.ERR_ARG
        assert plans.sweeps_launched("collapse") == before and lib.qsim_holds_nothing(sim._h) == 1
    with Simulator(3, precision=precision) as sim:                         # the zero vector, written out: its total is zero
        sim.write(np.zeros(8))
        for bad in (lambda: sim.postselect([1], 0), lambda: sim.measure([1], draw=0.5)):
            with pytest.raises(QsimError) as err:
                bad()
            assert err.value.code == _lib.ERR_ARG
        assert plans.sweeps_launched("collapse") == before and not sim.read().any()


# ---- order with the gate queue ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", PRECISIONS)
def test_queued_gates_land_first(precision):
    n, qubits, u = 13, [0, 8, 3, 12], 0.4
    gates = [("h", q) for q in (0, 4, 12, 7)] + [("cx", 0, 8), ("x", 3), ("cx", 12, 1)]
    circuit = Circuit.from_gates(n, gates)
    with Simulator(n, precision=precision) as twin:                        # what the gates alone leave, as a state of this precision holds it
        twin.run(circuit)
        before = twin.read()
        want_outcome = int(twin.sample_shots(draws=[u], qubits=qubits)[0])
    assert np.count_nonzero(before) == 16
    with Simulator(n, precision=precision) as sim:
        sim.run(circuit)                                                   # queued, not flushed
        count = plans.sweeps_launched("collapse")
        outcome, p = sim.measure(qubits, draw=u, return_probability=True)
        assert plans.sweeps_launched("collapse") == count + 2 and outcome == want_outcome
        assert (outcome >> 2) & 1 == 1 and (outcome & 1) == ((outcome >> 1) & 1)   # qubit 3 was flipped, qubit 8 copies qubit 0
        assert p == pytest.approx(0.25, abs=1e-12 if precision == 64 else 1e-6)
        _check_state(sim.read(), before, qubits, outcome, precision, f"queued gates p{precision}")


# ---- reset ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", PRECISIONS)
def test_reset_qubits(precision):
    n = measure_ref.RESET_N
    sim, psi = _sim_with(n, precision, 1270)
    with sim:
        for qubits, u in measure_ref.RESET_CASES:
            sim.write(psi)
            want_outcome = int(sim.sample_shots(draws=[u], qubits=qubits)[0])
            outcome = sim.reset_qubits(qubits, draw=u)
            assert outcome == want_outcome
            marginal = sim.marginal_probabilities(qubits)
            assert abs(marginal[0] - 1.0) <= (1e-12 if precision == 64 else 1e-6) and not marginal[1:].any()
            got = sim.read()
            _, want = measure_ref.postselect(psi, qubits, outcome)
            want = measure_ref.cleared(want, qubits, outcome)
            label = f"reset p{precision} q={qubits} o={outcome}"
            if precision == 64:
                worst = float(np.max(np.abs(got - want)))
                print(f"measure {label}: max abs err {worst:.3e}")
                assert worst < TOL
            else:
                _, ref32 = measure_ref.postselect(psi, qubits, outcome, dtype=np.complex64)
                fp32_ref.report(f"measure {label}", fp32_ref.check_fp32(got, want, measure_ref.cleared(ref32, qubits, outcome)))
        sim.write(psi)                                                     # the draw made from a seed
        assert sim.reset_qubits([2, 8], seed=5) in range(4) and abs(sim.marginal_probabilities([2, 8])[0] - 1.0) < 1e-6


# ---- lazily held states -----------------------------------------------------------------------------------------------------------------------
# One qubit set inside SUPPORT_LOW.  No qubit lies outside BOTH partial supports (together they cover the register), so the other set has
# a qubit outside each of them: 4 is outside SUPPORT_LOW, 0 outside SUPPORT_HIGH, and both are outside what the `pending` start holds.
LAZY_INSIDE_LOW = (9, 0, 5)
LAZY_OUTSIDE = (4, 14, 0)
assert set(LAZY_INSIDE_LOW) <= set(lazy_cases.SUPPORT_LOW)
assert set(LAZY_OUTSIDE) - set(lazy_cases.SUPPORT_LOW) and set(LAZY_OUTSIDE) - set(lazy_cases.SUPPORT_HIGH)


def _likely_outcome(start, precision, qubits):
    """The most probable outcome of `qubits` on the state a start stands for: non-zero probability, and bits of 0 on every qubit
    outside a sparse start's support, where a 1 never happens."""
    p = np.abs(_dense(start, precision)) ** 2
    idx = np.arange(p.size)
    outcome_of = sum(((idx >> q) & 1) << j for j, q in enumerate(qubits))
    return int(np.argmax(np.bincount(outcome_of, weights=p, minlength=1 << len(qubits))))


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("start", lazy_cases.STARTS)
@pytest.mark.parametrize("qubits", [LAZY_INSIDE_LOW, LAZY_OUTSIDE], ids=["inside_low", "outside"])
@pytest.mark.parametrize("call", ["postselect", "measure"])
def test_lazy_starts_over_poisoned_memory(call, qubits, start, precision):
    qubits = list(qubits)
    outcome = _likely_outcome(start, precision, qubits)
    if start in lazy_cases.SUPPORTS:
        assert not any((outcome >> j) & 1 for j, q in enumerate(qubits) if q not in lazy_cases.SUPPORTS[start])
    results = []
    for lazy in (True, False):
        with Side(precision, lazy) as side:
            sim = side.state(start)
            count = plans.sweeps_launched("collapse")
            returned = sim.postselect(qubits, outcome) if call == "postselect" else sim.measure(qubits, draw=0.37, return_probability=True)
            assert plans.sweeps_launched("collapse") == count + 2
            results.append((returned, sim.read()))
    (lazy_ret, lazy_got), (twin_ret, twin_got) = results
    assert not np.isnan(lazy_got).any()
    assert np.array_equal(_bits(lazy_got), _bits(twin_got))
    assert np.array_equal(np.asarray(lazy_ret, dtype=np.float64).view(np.uint64), np.asarray(twin_ret, dtype=np.float64).view(np.uint64))
    assert float(np.linalg.norm(twin_got)) == pytest.approx(1.0, abs=1e-5)


# ---- teleportation ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", PRECISIONS)
def test_teleportation_end_to_end(precision):
    """fp64: the issue's 1e-10 on rho and 1e-12 on the probabilities.  fp32: 1e-6 for both — six gates on amplitudes below 1, each rounding
    its products to 2^-24 relative, and one collapse."""
    tol_rho, tol_p = (1e-10, 1e-12) if precision == 64 else (1e-6, 1e-6)
    rng = np.random.default_rng(1280)
    phi = rng.standard_normal(2) + 1j * rng.standard_normal(2)
    phi /= np.linalg.norm(phi)
    U = np.linalg.qr(np.column_stack([phi, rng.standard_normal(2) + 1j * rng.standard_normal(2)]))[0]
    U = U * (phi[0] / U[0, 0])                                              # the first column is phi itself
    assert np.allclose(U[:, 0], phi) and np.allclose(U.conj().T @ U, np.eye(2))

    def prepared(sim):
        sim.reset()
        sim.apply_1q(U, 0)
        sim.apply_1q(gate_matrix("h"), 1)
        sim.apply_cx(1, 2)
        sim.apply_cx(0, 1)
        sim.apply_1q(gate_matrix("h"), 0)

    with Simulator(3, precision=precision) as sim:
        prepared(sim)
        draws = [(i + 0.5) / 16 for i in range(16)]
        read = sim.sample_shots(draws=draws, qubits=[0, 1])
        forcing = {int(o): u for u, o in zip(draws, read)}
        assert sorted(forcing) == [0, 1, 2, 3]
        for want_outcome, u in sorted(forcing.items()):
            prepared(sim)
            outcome, p = sim.measure([0, 1], draw=u, return_probability=True)
            assert outcome == want_outcome and abs(p - 0.25) <= tol_p, (outcome, p)
            if outcome & 2:
                sim.apply_1q(gate_matrix("x"), 2)
            if outcome & 1:
                sim.apply_1q(gate_matrix("z"), 2)
            rho = sim.reduced_density_matrix([2])
            worst = float(np.max(np.abs(rho - np.outer(phi, phi.conj()))))
            print(f"teleportation p{precision} outcome {outcome}: p off by {abs(p - 0.25):.3e}, rho off by {worst:.3e}")
            assert worst <= tol_rho, outcome
            assert sim.marginal_probabilities([0, 1])[outcome] == pytest.approx(1.0, abs=tol_p)


# ---- Kraus channels ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("which", ["two_qubit_depolarizing", "amplitude_damping"])
def test_apply_channel(which, precision):
    n = 6
    kraus, targets = (channels.two_qubit_depolarizing(0.3), (1, 4)) if which == "two_qubit_depolarizing" else (channels.amplitude_damping(0.4), (0,))
    sim, psi = _sim_with(n, precision, 1290)
    with sim:
        p_all = measure_ref.kraus_step(psi, kraus, targets, 0.5)[3]
        mixture = np.zeros((1 << n, 1 << n), dtype=np.complex128)
        for i, u in enumerate(measure_ref.midpoints(p_all)):
            assert u is not None
            want_i, want_p, want, _ = measure_ref.kraus_step(psi, kraus, targets, u)
            assert want_i == i
            sim.write(psi)
            got_i, got_p = sim.apply_channel(kraus, targets, draw=u, return_probability=True)
            got = sim.read()
            assert got_i == i and abs(got_p - want_p) <= 1e-12, (i, got_i, got_p, want_p)
            label = f"channel {which} p{precision} i={i}"
            if precision == 64:
                worst = float(np.max(np.abs(got - want)))
                print(f"measure {label}: max abs err {worst:.3e}")
                assert worst < TOL, label
            else:
                ref32 = measure_ref.kraus_step(psi, kraus, targets, u, dtype=np.complex64)[2]
                fp32_ref.report(f"measure {label}", fp32_ref.check_fp32(got, want, ref32))
            mixture += got_p * np.outer(got, got.conj())
        if precision == 64:                                                # the trajectories average to the channel
            total = float(np.vdot(psi, psi).real)
            images = [matrix_ref.apply_matrix(psi, K, targets) for K in kraus]
            channel = sum(np.outer(v, v.conj()) for v in images) / total
            worst = float(np.max(np.abs(mixture - channel)))
            print(f"measure channel {which}: mixture off by {worst:.3e}")
            assert worst < TOL
        sim.write(psi)
        state = _bits(sim.read()).copy()
        for bad in ([np.eye(1 << len(targets)), 0.1 * np.eye(1 << len(targets))], [0.5 * K for K in kraus], []):
            with pytest.raises(ValueError):
                sim.apply_channel(bad, targets, draw=0.5)
        with pytest.raises(ValueError):
            sim.apply_channel(kraus, targets, draw=1.5)
        assert np.array_equal(_bits(sim.read()), state)
        assert sim.apply_channel(kraus, targets, seed=3) in range(len(kraus))
        assert abs(sim.norm2() - 1.0) <= (1e-12 if precision == 64 else 1e-6)
