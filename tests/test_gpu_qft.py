"""The quantum Fourier transform on the device (Simulator.apply_qft, qsim_apply_qft; csrc/qft.hip, csrc/qft.cpp).

The checker is qft_ref.apply_qft (numpy.fft on the gathered register axis; pinned on the CPU by tests/test_qft_cpu.py) on the
amplitudes READ BACK from the same state before the call — for an fp32 state `read()` is the exact widened contents.  fp64: max abs
error < 1e-10 on a unit-norm state, the project's tolerance.  fp32: fp32_ref.check_fp32(got, want64, ref32) with the complex64 radix-2
replay of qft_ref.  Every accepted call must raise the sweep counter by exactly the plan's `passes`; every refused call raises it by
zero and leaves the state's bits alone.
Sizes: n <= 4 (the guarded instantiation), both sides of the tile boundary (n = 11 | 12 | 13 in fp64, 12 | 13 | 14 in fp32), n = 13
for single passes and for two, three, four and thirteen passes, n = 16 with twelve scattered targets, n = 15 and 16 under grid caps,
and n = 22 (fp64) / 23 (fp32), where the plan call reports two trips per workgroup at the default grid."""
import functools
import itertools

import numpy as np
import pytest

import fp32_ref
import lazy_cases
import qft_ref
from gpu_quantum_simulator_amd import Circuit, Cluster, Simulator, _lib, plans
from gpu_quantum_simulator_amd._marshal import ints as _ints
from gpu_quantum_simulator_amd._lib import QsimError
from pauli_rot_ref import rand_state
from test_gpu_lazy_states import Side

pytestmark = pytest.mark.gpu
TOL = 1e-10
PRECISIONS = [64, 32]


def _bits(state):
    return np.ascontiguousarray(state).view(np.uint64)


def _compare(got, before, qubits, inverse, precision, label):
    want = qft_ref.apply_qft(before, qubits, inverse)
    if precision == 64:
        worst = float(np.max(np.abs(got - want))) if got.size else 0.0
        print(f"qft {label}: max abs err {worst:.3e}")
        assert worst < TOL, label
    else:
        ref32 = qft_ref.apply_qft(before.astype(np.complex64), qubits, inverse, dtype=np.complex64)
        fp32_ref.report(f"qft {label}", fp32_ref.check_fp32(got, want, ref32))


def _apply_and_check(sim, before, qubits, inverse=False, cap=0):
    """One call on the device against the checker on `before` (the state as read back); returns the state after it."""
    passes = plans.ok(plans.apply_qft_plan(qubits, sim.num_qubits, sim.precision, cap))["passes"]
    count = plans.sweeps_launched("qft")
    sim.apply_qft(qubits, inverse=inverse, max_digit_bits=cap)
    assert plans.sweeps_launched("qft") == count + passes
    got = sim.read()
    _compare(got, before, qubits, inverse, sim.precision, f"n={sim.num_qubits} p{sim.precision} k={len(qubits)} cap={cap} inv={int(inverse)} passes={passes}")
    return got


def _sim_with(n, precision, seed, **options):
    sim = Simulator(n, precision=precision, **options)
    sim.write(rand_state(n, seed))
    return sim, sim.read()


# ---- registers smaller than a workgroup's tile ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("n", [0, 1, 2, 3, 4])
def test_small_registers_every_subset_in_both_orders(n, precision):
    sim, psi = _sim_with(n, precision, 1000 + n)
    with sim:
        for k in range(0, n + 1):
            for subset in itertools.combinations(range(n), k):
                for qubits in {subset, subset[::-1]}:
                    for inverse in (False, True):
                        psi = _apply_and_check(sim, psi, list(qubits), inverse)


# ---- both sides of the tile boundary ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("offset", [-1, 0, 1])
def test_tile_boundaries(offset, precision):
    n = qft_ref.tile_bits(precision) + offset
    sim, psi = _sim_with(n, precision, 1010 + n)
    with sim:
        for case_n, qubits, cap in qft_ref.boundary_cases(precision):
            if case_n == n:
                assert plans.ok(plans.apply_qft_plan(qubits, n, precision, 0))["tiles"] == (2 if offset > 0 else 1)
                psi = _apply_and_check(sim, psi, qubits, inverse=bool(len(qubits) & 1), cap=cap)


# ---- n = 13: one pass -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", PRECISIONS)
def test_single_pass_places_and_the_way_back(precision):
    sim, start = _sim_with(13, precision, 1020)
    with sim:
        for n, qubits, cap in qft_ref.single_pass_cases():
            plan = plans.ok(plans.apply_qft_plan(qubits, n, precision, cap))
            assert plan["passes"] == 1 and plan["out_of_place"] == [0]
            there = _apply_and_check(sim, start, qubits)
            back = _apply_and_check(sim, there, qubits, inverse=True)
            if precision == 64:
                assert float(np.max(np.abs(back - start))) < TOL
            else:                                                # the same criterion for the two calls as one circuit: the replay of both
                ref32 = qft_ref.apply_qft(qft_ref.apply_qft(start.astype(np.complex64), qubits, dtype=np.complex64), qubits, True, dtype=np.complex64)
                fp32_ref.check_fp32(back, start, ref32)
            start = back


# ---- several passes -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", PRECISIONS)
def test_several_passes(precision):
    sims = {}
    try:
        for n, qubits, cap, passes in qft_ref.multi_pass_cases():
            if n not in sims:
                sims[n] = _sim_with(n, precision, 1030 + n)
            sim, psi = sims[n]
            plan = plans.ok(plans.apply_qft_plan(qubits, n, precision, cap))
            assert plan["passes"] == passes and sum(plan["out_of_place"]) % 2 == 0 and sum(plan["out_of_place"]) >= passes - 1
            for inverse in (False, True):
                psi = _apply_and_check(sim, psi, qubits, inverse, cap)
            sims[n] = (sim, psi)
    finally:
        for sim, _ in sims.values():
            sim.close()


# ---- the grid ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", PRECISIONS)
def test_equal_bits_whatever_the_grid(precision):
    for n, qubits, cap in qft_ref.grid_cases():
        start = rand_state(n, 1040 + n)
        assert plans.ok(plans.apply_qft_plan(qubits, n, precision, cap))["passes"] == (1 if cap == 0 else 3)
        with Simulator(n, precision=precision) as sim:
            sim.write(start)
            first = _bits(_apply_and_check(sim, sim.read(), qubits, cap=cap)).copy()
            for grid_cap in (1, 2, 7):
                sim.set_option(_lib.OPT_GRID_CAP, grid_cap)
                sim.write(start)
                sim.apply_qft(qubits, max_digit_bits=cap)
                assert np.array_equal(_bits(sim.read()), first), (n, qubits, grid_cap)
            sim.set_option(_lib.OPT_GRID_CAP, 0)


@functools.lru_cache(maxsize=None)
def _large_state(n):
    return rand_state(n, 1050)


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("which", [0, 1])
def test_looping_at_the_default_grid(which, precision):
    n, qubits, cap = qft_ref.looping_cases(precision)[which]
    assert plans.ok(plans.apply_qft_plan(qubits, n, precision, cap))["trips_per_workgroup"] >= 2
    with Simulator(n, precision=precision) as sim:
        sim.write(_large_state(n))
        _apply_and_check(sim, sim.read(), qubits, inverse=bool(which), cap=cap)


# ---- buffers ----------------------------------------------------------------------------------------------------------------------------------
MOVING = (13, [12, 3, 7, 0, 9, 5, 11, 1, 8, 4, 10, 6], 4)        # three passes, two of them out of place


@pytest.mark.parametrize("precision", PRECISIONS)
def test_the_state_stays_in_its_buffer(precision):
    import torch
    n, qubits, cap = MOVING
    real = torch.float32 if precision == 32 else torch.float64
    view = np.complex64 if precision == 32 else np.complex128
    assert plans.ok(plans.apply_qft_plan(qubits, n, precision, cap))["out_of_place"] == [1, 1, 0]
    sim, psi = _sim_with(n, precision, 1060)
    with sim:
        at = sim.device_ptr
        want = _bits(_apply_and_check(sim, psi, qubits, cap=cap)).copy()
        assert sim.device_ptr == at
        # a caller's tensor as the state's buffer holds the result
        mine = torch.zeros((1 << n, 2), dtype=real, device="cuda")
        torch.cuda.synchronize()
        was = sim.swap_buffer(mine.data_ptr())
        try:
            sim.write(psi)
            sim.apply_qft(qubits, max_digit_bits=cap)
            sim.sync()
            assert sim.device_ptr == mine.data_ptr()
            held = mine.cpu().numpy().reshape(-1).view(view).astype(np.complex128)
            assert np.array_equal(_bits(held), want)
        finally:
            sim.swap_buffer(was)
        # a lent spare buffer full of NaN, and none at all, give the same bits
        lent = torch.full((1 << n, 2), float("nan"), dtype=real, device="cuda")
        torch.cuda.synchronize()
        sim.set_spare_buffer(lent.data_ptr())
        try:
            sim.write(psi)
            sim.apply_qft(qubits, max_digit_bits=cap)
            assert np.array_equal(_bits(sim.read()), want)
        finally:
            sim.set_spare_buffer(None)
        sim.write(psi)
        sim.apply_qft(qubits, max_digit_bits=cap)
        assert np.array_equal(_bits(sim.read()), want) and sim.device_ptr == at


# ---- lazily held states -----------------------------------------------------------------------------------------------------------------------
LAZY_SINGLE = ([14, 0, 3, 7, 9, 1, 12, 5, 13, 10], 0)
LAZY_MOVING = ([14, 0, 3, 7, 9, 1, 12, 5, 13, 10, 4, 8], 4)


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("start", lazy_cases.STARTS)
@pytest.mark.parametrize("case", [LAZY_SINGLE, LAZY_MOVING], ids=["single", "moving"])
def test_lazy_starts_over_poisoned_memory(case, start, precision):
    qubits, cap = case
    results = []
    for lazy in (True, False):
        with Side(precision, lazy) as side:
            sim = side.state(start)
            count = plans.sweeps_launched("qft")
            sim.apply_qft(qubits, max_digit_bits=cap)
            assert plans.sweeps_launched("qft") == count + plans.ok(plans.apply_qft_plan(qubits, lazy_cases.N, precision, cap))["passes"]
            results.append(sim.read())
    lazy_got, twin_got = results
    assert not np.isnan(lazy_got).any()
    assert np.array_equal(_bits(lazy_got), _bits(twin_got))
    assert float(np.linalg.norm(twin_got)) == pytest.approx(1.0, abs=1e-5)


# ---- order with the gate queue ----------------------------------------------------------------------------------------------------------------
def _feed(sim, gates):
    for g in gates:
        if g[0] == "u1":
            sim.apply_1q(g[2], g[1])
        elif g[0] == "cx":
            sim.apply_cx(g[1], g[2])
        else:
            sim.apply_2q(g[3], g[1], g[2])


@pytest.mark.parametrize("precision", PRECISIONS)
def test_queued_gates_land_first(precision):
    n, qubits = 13, [12, 0, 5, 9, 1, 7, 3, 11, 2, 6, 10]
    gates = [("h", q) for q in (0, 4, 12, 7)] + [("cx", 0, 8), ("x", 3), ("cx", 12, 1)]
    circuit = Circuit.from_gates(n, gates)
    with Simulator(n, precision=precision) as twin:              # what the gates alone leave, as a state of this precision holds it
        twin.run(circuit)
        before = twin.read()
    assert np.count_nonzero(before) == 16
    with Simulator(n, precision=precision) as sim:
        sim.run(circuit)                                         # queued, not flushed
        count = plans.sweeps_launched("qft")
        sim.apply_qft(qubits)
        assert plans.sweeps_launched("qft") == count + 2
        _compare(sim.read(), before, qubits, False, precision, f"queued gates p{precision}")


def test_agrees_with_the_textbook_circuit_through_the_gate_queue():
    n, qubits = 14, [13, 2, 7, 0, 9, 4, 11, 6]
    psi = rand_state(n, 1070)
    with Simulator(n) as sim, Simulator(n) as other:
        sim.write(psi)
        sim.apply_qft(qubits)
        got = sim.read()
        other.write(psi)
        _feed(other, qft_ref.textbook_gates(qubits))
        want = other.read()
    worst = float(np.max(np.abs(got - want)))
    print(f"qft against the gate queue: max abs err {worst:.3e}")
    assert worst < TOL


@pytest.mark.parametrize("precision", PRECISIONS)
def test_order_finding_end_to_end(precision):
    """n = 12, N = 15, a = 7, whose order is 4: the counting register reads a multiple of 256 / 4."""
    n, counting, work = 12, list(range(8)), [8, 9, 10, 11]
    with Simulator(n, precision=precision) as sim:
        sim.run(Circuit.from_gates(n, [("h", q) for q in counting] + [("x", work[0])]))
        for j in counting:
            sim.apply_modular_multiply(pow(7, 1 << j, 15), 15, work, controls=[j])
        sim.apply_qft(counting, inverse=True)
        p = sim.marginal_probabilities(counting)
    want = np.zeros(256)
    want[[0, 64, 128, 192]] = 0.25
    worst = float(np.max(np.abs(p - want)))
    print(f"order finding p{precision}: max abs err {worst:.3e}")
    assert worst < (TOL if precision == 64 else 1e-5)            # fp64: the issue's 1e-10; fp32: amplitudes of 1/2 held to a few 2^-24


# ---- refusals -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", PRECISIONS)
def test_refusals(precision):
    lib = _lib.load()
    assert hasattr(Simulator, "apply_qft") and not hasattr(Cluster, "apply_qft")
    with Simulator(12, precision=precision) as sim:
        sim.write(rand_state(12, 3))
        state = _bits(sim.read()).copy()
        before = plans.sweeps_launched("qft")
        sim.apply_qft([])                                        # k = 0 is accepted and does nothing
        assert lib.qsim_apply_qft(sim._h, None, 0, 0, 0) == _lib.QSIM_OK
        assert plans.sweeps_launched("qft") == before and np.array_equal(_bits(sim.read()), state)
        for bad in (lambda: sim.apply_qft([0, 0]), lambda: sim.apply_qft([2, 5, 2]), lambda: sim.apply_qft([12]), lambda: sim.apply_qft([-1]),
                    lambda: sim.apply_qft(list(range(12)) + [3]), lambda: sim.apply_qft([0, 1], max_digit_bits=11),
                    lambda: sim.apply_qft([0, 1], max_digit_bits=-1), lambda: sim.apply_qft([0, 1], inverse=True, max_digit_bits=12)):
            with pytest.raises(QsimError) as err:
                bad()
            assert err.value.code == _lib.ERR_ARG
        assert lib.qsim_apply_qft(sim._h, None, 1, 0, 0) == _lib.ERR_ARG and lib.qsim_apply_qft(sim._h, _ints([0]), -1, 0, 0) == _lib.ERR_ARG
        assert lib.qsim_apply_qft(sim._h, _ints(list(range(13))), 13, 0, 0) == _lib.ERR_ARG and lib.qsim_apply_qft(None, _ints([0]), 1, 0, 0) == _lib.ERR_ARG
        assert plans.sweeps_launched("qft") == before
        assert np.array_equal(_bits(sim.read()), state)
        sim.reset(holds_index0=False)                            # a state that holds nothing: accepted, no sweep
        sim.apply_qft(list(range(12)))
        assert plans.sweeps_launched("qft") == before and lib.qsim_holds_nothing(sim._h) == 1
