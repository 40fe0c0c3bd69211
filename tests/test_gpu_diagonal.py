"""Whole-register diagonal operators from a table, on the device: Diagonal (qsim_diagonal_*), Simulator.apply_diagonal_phase and
Simulator.expectation_diagonal (csrc/diagonal.hip, csrc/diagonal.cpp).

The checker is numpy (tests/diagonal_ref.py, pinned by tests/test_diagonal_cpu.py) on the amplitudes READ BACK before the call — for
an fp32 state `read()` is the exact widened contents, so the rounding of a write cancels.
Table build: np.array_equal with the sequential sum — c s is an exact sign flip and the device adds in the caller's order.
Phase, fp64: max abs error < 1e-10, the project's parity tolerance (one complex multiply rounds near 1e-16; the angle gamma d_i
carries two roundings of relative 1.1e-16, 1e-14 at |gamma d_i| = 50 and 2e-12 at 1e4, where a sine with a poor argument reduction
misses by orders of magnitude).  fp32: fp32_ref.check_fp32(got, want64, ref32), ref32 the factor formed in fp64, rounded once and
multiplied in complex64.
Moments: |mean - numpy| <= 1e-10 max|d| and the second moment likewise with max d^2: sums of 2^n products of weights that add up to
one, in fp64 — only the order of the additions differs.
Sizes: n = 0 (no 16-byte unit of the table), 1, 2, 3, 6 (the largest register on the plain path), 7 (the smallest on the main one:
one wave), 9, and per precision the smallest n at which plans.diagonal_plan reports more than one trip per workgroup for both sweeps
with the grid at its cap."""
import numpy as np
import pytest

import diagonal_ref
import fp32_ref
import pauli_rot_ref
from fp32_ref import check_fp32, report
from gpu_quantum_simulator_amd import Circuit, Cluster, Diagonal, Simulator, _lib, circuits, plans
from pauli_rot_ref import rand_state

pytestmark = pytest.mark.gpu
TOL = 1e-10
PRECISIONS = [64, 32]
SMALL = [0, 1, 2, 3, 6, 7, 9]
GAMMA = 0.37
ANGLE = 50.0  # |gamma d_i| at most


def _bits(sim):
    return sim.read().view(np.uint64).copy()


def _table(n, seed, angle=ANGLE):
    return np.random.default_rng(seed).uniform(-angle / GAMMA, angle / GAMMA, size=1 << n)


def _dtype(precision):
    return np.complex128 if precision == 64 else np.complex64


def _check_state(precision, got, before, d, gamma, label):
    """`d`: the table, or a list of tables applied one after the other."""
    want, ref32 = before, before.astype(np.complex64)
    for table in d if isinstance(d, list) else [d]:
        want = diagonal_ref.apply_phase(want, table, gamma)
        ref32 = diagonal_ref.apply_phase(ref32, table, gamma, dtype=np.complex64)
    print(f"{label} p{precision}: max abs err {np.max(np.abs(got - want)):.3e}")
    if precision == 64:
        assert np.max(np.abs(got - want)) < TOL
    else:
        report(label, check_fp32(got, want, ref32))


def _check_moments(got, before, d, label):
    mean, second = diagonal_ref.moments(before, d)
    scale = float(np.max(np.abs(d)))
    print(f"{label}: mean err {abs(got[0] - mean):.3e} (max|d| {scale:.3e}), second moment err {abs(got[1] - second):.3e}")
    assert abs(got[0] - mean) <= TOL * scale
    assert abs(got[1] - second) <= TOL * scale * scale


def _random_terms(n, count, seed):
    """[(c, z)]: masks on the thread's bits only (below 8), on bits from 8 up only, bit n - 1 alone, z == 0, and any."""
    rng = np.random.default_rng(seed)
    full = (1 << n) - 1
    out = []
    for k in range(count):
        z = int(rng.integers(0, 1 << n)) if n else 0
        kind = k % 5
        z = (z & 0xFF, z & ~0xFF & full, (1 << (n - 1)) if n else 0, 0, z)[kind]
        out.append((float(rng.uniform(-1, 1)), z))
    return out


@pytest.fixture(scope="module")
def loop_data():
    """At the looping sizes, computed once: precision -> (n, random unit state, random table)."""
    out = {}
    for precision in PRECISIONS:
        n = diagonal_ref.loop_n(precision)
        out[precision] = (n, rand_state(n, 700 + precision), _table(n, 800 + precision))
    return out


# ---- 1. the table ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,count", [(0, 33), (1, 33), (2, 33), (3, 33), (9, 33), (13, 1), (13, 31), (13, 32), (13, 33), (13, 70)])
def test_table_build_is_the_sequential_sum(n, count):
    terms = _random_terms(n, count, 100 * n + count)
    with Diagonal.from_terms(n, diagonal_ref.texts(terms, n)) as diag:
        assert np.array_equal(diag.read(), diagonal_ref.table_from_terms(n, terms))
        start = np.random.default_rng(n).standard_normal(1 << n)
        diag.write(start)
        assert np.array_equal(diag.read(), start)
        diag.add_terms(diagonal_ref.texts(terms[::-1], n))           # a second add_terms on top of a write, another order
        assert np.array_equal(diag.read(), diagonal_ref.table_from_terms(n, terms[::-1], start))
        assert np.array_equal(diag.read(first=(1 << n) // 2), diag.read()[(1 << n) // 2:])


def test_table_build_where_every_workgroup_loops():
    n = max(diagonal_ref.loop_n(p) for p in PRECISIONS)
    terms = _random_terms(n, 33, 23)
    with Diagonal(n) as diag:
        assert diag.num_qubits == n and not diag.read().any()      # created as zeros
        diag.add_terms(diagonal_ref.texts(terms, n))
        assert np.array_equal(diag.read(), diagonal_ref.table_from_terms(n, terms))


# ---- 2. the phase ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("n", SMALL)
def test_phase(n, precision):
    d = _table(n, 200 + n)
    with Simulator(n, precision=precision) as sim, Diagonal(n) as diag:
        sim.write(rand_state(n, 210 + n))
        before = sim.read()
        diag.write(d)
        sim.apply_diagonal_phase(diag, GAMMA)
        _check_state(precision, sim.read(), before, d, GAMMA, f"phase n={n}")
        assert np.array_equal(diag.read().view(np.uint64), d.view(np.uint64))   # the table's bits are untouched


@pytest.mark.parametrize("precision", PRECISIONS)
def test_phase_where_every_workgroup_loops(precision, loop_data):
    n, psi, d = loop_data[precision]
    with Simulator(n, precision=precision) as sim, Diagonal(n) as diag:
        sim.write(psi)
        before = sim.read()
        diag.write(d)
        sim.apply_diagonal_phase(diag, GAMMA)
        _check_state(precision, sim.read(), before, d, GAMMA, f"looping phase n={n}")
        assert np.array_equal(diag.read().view(np.uint64), d.view(np.uint64))


def test_phase_with_large_angles():
    """|gamma d_i| up to 1e4 in fp64 still meets 1e-10: the argument reduction is exact, only the angle's own rounding is left."""
    n = 9
    d = _table(n, 220, angle=1e4)
    assert np.max(np.abs(GAMMA * d)) > 9e3
    with Simulator(n) as sim, Diagonal(n) as diag:
        sim.write(rand_state(n, 221))
        before = sim.read()
        diag.write(d)
        sim.apply_diagonal_phase(diag, GAMMA)
        _check_state(64, sim.read(), before, d, GAMMA, "large angles")


# ---- 3. against the rotations ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", PRECISIONS)
def test_phase_equals_the_z_rotations(precision):
    n, gamma = 12, 0.61
    rng = np.random.default_rng(12)
    terms = [(float(rng.uniform(-1, 1)), int(rng.integers(1, 1 << n))) for _ in range(40)]
    texts = diagonal_ref.texts(terms, n)
    with Simulator(n, precision=precision) as sim, Simulator(n, precision=precision) as twin, Diagonal.from_terms(n, texts) as diag:
        for s in (sim, twin):
            s.write(rand_state(n, 120))
        before = sim.read()
        sweeps = plans.sweeps_launched("diagonal")
        sim.apply_diagonal_phase(diag, gamma)
        assert plans.sweeps_launched("diagonal") == sweeps + 1
        twin.apply_pauli_rotations([(2.0 * gamma * c, text) for c, text in texts])
        got, rotated = sim.read(), twin.read()
        rotations = [(2.0 * gamma * c, 0, z) for c, z in terms]
        want = pauli_rot_ref.replay(before, rotations)
        print(f"phase against rotations p{precision}: max abs difference {np.max(np.abs(got - rotated)):.3e}")
        if precision == 64:
            assert np.max(np.abs(got - rotated)) < TOL and np.max(np.abs(got - want)) < TOL
        else:
            ref32 = pauli_rot_ref.replay(before, rotations, dtype=np.complex64)
            report("phase against rotations: the table", check_fp32(got, want, ref32))
            report("phase against rotations: the rotations", check_fp32(rotated, want, ref32))


# ---- 4. the expectation value ---------------------------------------------------------------------------------------------------------
def _expectation_case(sim, diag, d, precision, label):
    before, bits = sim.read(), _bits(sim)
    got = sim.expectation_diagonal(diag, moments=True)
    _check_moments(got, before, d, f"{label} p{precision}")
    assert sim.expectation_diagonal(diag, moments=True) == got     # equal calls, equal bits
    assert sim.expectation_diagonal(diag) == got[0]
    assert np.array_equal(_bits(sim), bits)                        # read-only
    return before, got


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("n", SMALL)
def test_expectation(n, precision):
    terms = _random_terms(n, 12, 300 + n)
    texts = diagonal_ref.texts(terms, n)
    d = _table(n, 310 + n)
    with Simulator(n, precision=precision) as sim, Diagonal(n) as diag, Diagonal.from_terms(n, texts) as from_terms:
        sim.write(rand_state(n, 320 + n))
        diag.write(d)
        _expectation_case(sim, diag, d, precision, f"expectation n={n}")
        _, got = _expectation_case(sim, from_terms, diagonal_ref.table_from_terms(n, terms), precision, f"expectation of terms n={n}")
        by_strings = sim.expectation(texts)
        assert abs(got[0] - by_strings) <= TOL * sum(abs(c) for c, _ in terms)


@pytest.mark.parametrize("precision", PRECISIONS)
def test_expectation_where_every_workgroup_loops(precision, loop_data):
    n, psi, d = loop_data[precision]
    terms = _random_terms(n, 12, 330)
    texts = diagonal_ref.texts(terms, n)
    with Simulator(n, precision=precision) as sim, Diagonal(n) as diag:
        sim.write(psi)
        diag.write(d)
        _expectation_case(sim, diag, d, precision, f"looping expectation n={n}")
        diag.write(np.zeros(1 << n))
        diag.add_terms(texts)
        got = sim.expectation_diagonal(diag)
        assert abs(got - sim.expectation(texts)) <= TOL * sum(abs(c) for c, _ in terms)


# ---- 5. the state's bookkeeping -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("n", [0, 3, 9, 14])
def test_fresh_state(n, precision):
    """|0...0> was never written: amplitude 0 becomes the factor of d_0 and the rest stays exactly zero."""
    d = _table(n, 400 + n)
    with Simulator(n, precision=precision) as sim, Diagonal(n) as diag:
        diag.write(d)
        assert sim.get_support()[1]                                # |0...0> is held lazily
        assert sim.expectation_diagonal(diag, moments=True) == (d[0], d[0] * d[0])
    with Simulator(n, precision=precision) as sim, Diagonal(n) as diag:
        diag.write(d)
        sim.apply_diagonal_phase(diag, GAMMA)
        got = sim.read()
        assert sim.get_support()[0] == (1 << n) - 1                # dense afterwards
        want = np.exp(-1j * GAMMA * d[0]).astype(_dtype(precision))
        assert abs(got[0] - want) < (TOL if precision == 64 else 2e-7) and not got[1:].any()


@pytest.mark.parametrize("precision", PRECISIONS)
def test_partial_support(precision):
    """Gates on the low 7 qubits of an 18-qubit register leave most of the buffer unwritten: the sweeps write the zeros out first, and
    a later run on the state agrees with numpy."""
    n = 18
    few = Circuit.from_gates(n, circuits.random_gates(*fp32_ref.FEW_CIRCUIT))
    gates = fp32_ref.gate_list(*fp32_ref.FEW_CIRCUIT)
    d = _table(n, 418)
    with Simulator(n, precision=precision) as probe, Simulator(n, precision=precision) as sim, Diagonal(n) as diag:
        diag.write(d)
        probe.run(few)
        before = probe.read()                                      # the read writes the zeros out: the state is read from a twin
        sim.run(few)
        assert sim.get_support()[0] != (1 << n) - 1                # partial
        got = sim.expectation_diagonal(diag, moments=True)
        _check_moments(got, before, d, f"partial support p{precision}")
        sim.reset()
        sim.run(few)
        assert sim.get_support()[0] != (1 << n) - 1
        sim.apply_diagonal_phase(diag, GAMMA)
        after = sim.read()
        assert sim.get_support()[0] == (1 << n) - 1
        _check_state(precision, after, before, d, GAMMA, "partial support")
        sim.run(few)
        later = sim.read()
        want = fp32_ref.replay(n, gates, start=after, dtype=np.complex128)
        if precision == 64:
            assert np.max(np.abs(later - want)) < TOL
        else:
            report("a run after the phase", check_fp32(later, want, fp32_ref.replay(n, gates, start=after, dtype=np.complex64)))


@pytest.mark.parametrize("precision", PRECISIONS)
def test_queued_gates_are_applied_first(precision):
    n = 9
    c = Circuit.from_gates(n, circuits.random_gates(n, 60, 59, "all"))
    d = _table(n, 509)
    with Simulator(n, precision=precision) as sim, Simulator(n, precision=precision) as twin, Diagonal(n) as diag:
        diag.write(d)
        for s in (sim, twin):
            s.write(rand_state(n, 510))
            s.run(c)                                               # no sync, no flush
        before = twin.read()
        _check_moments(sim.expectation_diagonal(diag, moments=True), before, d, f"queued gates p{precision}")
        sim.reset()
        sim.write(rand_state(n, 510))
        sim.run(c)
        sim.apply_diagonal_phase(diag, GAMMA)
        _check_state(precision, sim.read(), before, d, GAMMA, "queued gates")


@pytest.mark.parametrize("precision", PRECISIONS)
def test_a_shard_that_holds_nothing_stays_untouched(precision):
    n = 9
    with Simulator(n, precision=precision) as sim, Diagonal(n) as diag:
        diag.write(_table(n, 520))
        sim.reset(holds_index0=False)
        sweeps = plans.sweeps_launched("diagonal")
        sim.apply_diagonal_phase(diag, GAMMA)
        assert sim.expectation_diagonal(diag, moments=True) == (0.0, 0.0)
        assert plans.sweeps_launched("diagonal") == sweeps
        assert _lib.load().qsim_holds_nothing(sim._h) == 1 and not sim.read().any()


# ---- 6. ordering ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("first", ["phase", "expectation"])
@pytest.mark.parametrize("precision", PRECISIONS)
def test_calls_take_effect_in_the_order_issued(precision, first, loop_data):
    """A sweep, then a change of the table, then a sweep, nothing synchronised in between: the first sweep saw the old table, the
    second the new one."""
    n, psi, d = loop_data[precision]
    extra = [(11.0, 1 << (n - 1)), (-7.0, 0b101), (3.0, 0)]
    d2 = diagonal_ref.table_from_terms(n, extra, d)
    with Simulator(n, precision=precision) as sim, Diagonal(n) as diag:
        sim.write(psi)
        before = sim.read()
        diag.write(d)
        sim.sync()
        if first == "phase":
            sim.apply_diagonal_phase(diag, GAMMA)
        else:
            moments = sim.expectation_diagonal(diag, moments=True)
        diag.add_terms(diagonal_ref.texts(extra, n))
        sim.apply_diagonal_phase(diag, GAMMA)
        got = sim.read()
        if first == "phase":
            _check_state(precision, got, before, [d, d2], GAMMA, f"ordering n={n}")
        else:
            _check_moments(moments, before, d, f"ordering n={n}")
            _check_state(precision, got, before, d2, GAMMA, f"ordering n={n}")
        assert np.array_equal(diag.read(), d2)


# ---- 7. a table of the caller's -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("n", [0, 9])
def test_external_table(n, precision):
    import torch
    d = _table(n, 600 + n)
    tensor = torch.tensor(d, dtype=torch.float64, device="cuda:0")
    torch.cuda.synchronize()
    with Simulator(n, precision=precision) as sim, Simulator(n, precision=precision) as twin, Diagonal(n) as owned:
        owned.write(d)
        adopted = Diagonal(n, ptr=tensor.data_ptr())
        assert adopted.device_ptr() == tensor.data_ptr() and np.array_equal(adopted.read(), d)
        for s in (sim, twin):
            s.write(rand_state(n, 610 + n))
        assert sim.expectation_diagonal(adopted, moments=True) == twin.expectation_diagonal(owned, moments=True)
        assert adopted.extrema() == owned.extrema() == diagonal_ref.extrema(d)
        sim.apply_diagonal_phase(adopted, GAMMA)
        twin.apply_diagonal_phase(owned, GAMMA)
        assert np.array_equal(_bits(sim), _bits(twin))
        adopted.add_terms([(0.5, "")])                             # the caller's buffer is written through the object
        adopted.close()
        assert np.array_equal(tensor.cpu().numpy(), d + 0.5)       # and is still the caller's after close()


# ---- 8. extrema -----------------------------------------------------------------------------------------------------------------------
def test_extrema_ties_go_to_the_lowest_index():
    with Diagonal(0) as diag:
        diag.write(np.array([1.5]))
        assert diag.extrema() == {"min": 1.5, "argmin": 0, "max": 1.5, "argmax": 0}
    for n in (1, 3, 9, max(diagonal_ref.loop_n(p) for p in PRECISIONS)):
        N = 1 << n
        d = np.random.default_rng(n).uniform(-1, 1, size=N)
        lows = sorted({min(5, N - 1), N // 2, N - 1 - min(2, N // 4)})   # in the first workgroup's range, the middle, the last one's
        highs = sorted({min(700, N - 1) if n > 3 else 0, N // 2 - 1 if n > 1 else 0, N - 1} - set(lows))
        d[lows], d[highs] = -2.0, 3.0
        with Diagonal(n) as diag:
            diag.write(d)
            got = diag.extrema()
            assert got == diagonal_ref.extrema(d) and got["argmin"] == lows[0] and got["argmax"] == highs[0]
            assert diag.extrema() == got
            assert np.array_equal(diag.read(), d)


# ---- 9. refusals ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", PRECISIONS)
def test_refusals_leave_the_state_alone(precision):
    n = 6
    with Simulator(n, precision=precision) as sim, Diagonal(n) as diag, Diagonal(n + 1) as wide, Diagonal(n) as closed:
        closed.close()
        sim.write(rand_state(n, 900))
        before = _bits(sim)
        calls = [lambda: sim.apply_diagonal_phase(wide, GAMMA),
                 lambda: sim.expectation_diagonal(wide),
                 lambda: sim.apply_diagonal_phase(closed, GAMMA),
                 lambda: sim.expectation_diagonal(closed),
                 lambda: sim.apply_diagonal_phase(diag, float("nan")),
                 lambda: sim.apply_diagonal_phase(diag, float("inf")),
                 lambda: diag.write(np.zeros(3), first=(1 << n) - 2),
                 lambda: closed.read()]
        for call in calls:
            with pytest.raises(_lib.QsimError) as err:
                call()
            assert err.value.code == _lib.ERR_ARG
            assert np.array_equal(_bits(sim), before)
        with pytest.raises(ValueError):
            diag.add_terms([(1.0, "X0")])
        with pytest.raises(ValueError):
            diag.add_terms([(1.0, f"Z{n}")])
    assert not hasattr(Cluster, "apply_diagonal_phase") and not hasattr(Cluster, "expectation_diagonal")


def test_a_table_outlives_the_states_that_swept_it():
    """The event behind a sweep that read a table is recorded on the STATE's stream, and the table's set-up calls wait for it.  A state
    that goes takes its stream along, so it tells the tables first (qsim_destroy): add_terms after the state is gone waits for nothing
    that is gone, and the table is the exact sequential sum — every coefficient is a dyadic fraction."""
    n = 10
    j = np.arange(1 << n)
    sign = lambda *qs: 1.0 - 2.0 * (sum((j >> q) & 1 for q in qs) & 1)
    with Diagonal.from_terms(n, [(0.5, "Z0 Z3"), (-0.25, "Z9")]) as diag:
        rounds = 0
        for precision in PRECISIONS:
            for _ in range(20):
                with Simulator(n, precision=precision) as sim:
                    sim.apply_diagonal_phase(diag, GAMMA)
                    sim.expectation_diagonal(diag)
                diag.add_terms([(0.125, "Z1")])  # waits for every sweep that still reads the table
                rounds += 1
        assert np.array_equal(diag.read(), 0.5 * sign(0, 3) - 0.25 * sign(9) + 0.125 * rounds * sign(1))
