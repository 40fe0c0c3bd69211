"""Dense matrices on up to five target qubits under controls on the device (Simulator.apply_matrix, qsim_apply_matrix;
csrc/matrix.hip, csrc/matrix.cpp).

The checker is matrix_ref.apply_matrix (gather, matmul, scatter; pinned on the CPU by tests/test_matrix_cpu.py) on the amplitudes READ
BACK from the same state before the call — for an fp32 state `read()` is the exact widened contents.  fp64: 1e-10 max abs, the
project's parity tolerance, on a unit-norm state and a matrix of spectral norm <= 1.  fp32: fp32_ref.check_fp32(got, want64, ref32)
with ref32 the checker run in complex64 (on n = 13, k = 5 that replay is 1.1e-7 off the truth, inside REF_CAP).  Every accepted call
must raise the sweep counter by exactly one.  Sizes: the plain path (n <= 4), both sides of the switch to the matrix path for each
subset size (from the plan call), n = 13 for the matrix path's subsets and controls, and n = 22 (fp64) / 23 (fp32), where the plan
call reports at least two trips per workgroup."""
import functools
import itertools
from ctypes import POINTER, c_double

import numpy as np
import pytest

import fp32_ref
import matrix_ref
from gpu_quantum_simulator_amd import Simulator, _lib, plans
from gpu_quantum_simulator_amd._marshal import ints as _ints
from gpu_quantum_simulator_amd._lib import QsimError
from helpers import np_apply_1q, np_apply_2q, np_apply_cx, random_unitary
from pauli_rot_ref import rand_state
from test_gpu_density import N13_SUBSETS

pytestmark = pytest.mark.gpu
TOL = 1e-10
PRECISIONS = [64, 32]
H = np.array([[1, 1], [1, -1]]) / np.sqrt(2.0)
X = np.array([[0, 1], [1, 0]], dtype=np.complex128)
Z = np.diag([1.0, -1.0]).astype(np.complex128)


def _compare(sim, got, before, U, targets, controls, label):
    want = matrix_ref.apply_matrix(before, U, targets, controls)
    if sim.precision == 64:
        worst = float(np.max(np.abs(got - want)))
        print(f"{label} n={sim.num_qubits} p64 targets={list(targets)} controls={list(controls)}: max abs err {worst:.3e}")
        assert worst < TOL
    else:
        ref32 = matrix_ref.apply_matrix(before, U, targets, controls, dtype=np.complex64)
        fp32_ref.report(f"{label} n={sim.num_qubits} targets={list(targets)} controls={list(controls)}", fp32_ref.check_fp32(got, want, ref32))
    # outside the control subspace nothing may change, bit for bit
    if controls:
        ones = sum(1 << q for q in controls)
        outside = (np.arange(before.size, dtype=np.uint32) & np.uint32(ones)) != ones
        assert np.array_equal(got[outside].view(np.uint64), before[outside].view(np.uint64))


def _apply_and_check(sim, before, U, targets, controls=(), label=""):
    """One call on the device against the checker on `before` (the state as read back); returns the state after it."""
    count = plans.sweeps_launched("matrix")
    sim.apply_matrix(U, targets, controls)
    assert plans.sweeps_launched("matrix") == count + 1
    got = sim.read()
    _compare(sim, got, before, U, targets, controls, label)
    return got


def _sim_with(n, precision, seed):
    sim = Simulator(n, precision=precision)
    sim.write(rand_state(n, seed))
    return sim, sim.read()


def _contraction(dim, rng):
    """A random complex matrix of spectral norm 1: not unitary, not normal."""
    a = rng.standard_normal((dim, dim)) + 1j * rng.standard_normal((dim, dim))
    return a / np.linalg.norm(a, 2)


# ---- the plain path ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("n", [0, 1, 2, 3, 4])
def test_plain_path_every_subset(n, precision):
    rng = np.random.default_rng(500 + n)
    sim, psi = _sim_with(n, precision, 500 + n)
    with sim:
        for k in range(0, n + 1):
            for ts in itertools.combinations(range(n), k):
                for targets in ({ts, ts[::-1]}):
                    assert plans.ok(plans.apply_matrix_plan(targets, [], n, precision))["path"] == 0
                    psi = _apply_and_check(sim, psi, random_unitary(1 << k, rng), targets, (), "plain")
                rest = [q for q in range(n) if q not in ts]
                if rest:
                    psi = _apply_and_check(sim, psi, random_unitary(1 << k, rng), ts, rest[:1], "plain")
                    psi = _apply_and_check(sim, psi, random_unitary(1 << k, rng), ts[::-1], rest, "plain")


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("k", [3, 4, 5])
def test_path_switch(k, precision):
    """The smallest register the matrix path takes for this subset size, and the one below it: both from the plan call."""
    rng = np.random.default_rng(520 + k)
    for low in (0, 1):                                           # fp32: with qubit 0 in the subset and without (one qubit later)
        first = next(n for n in range(k + low, 16) if plans.ok(plans.apply_matrix_plan(list(range(low, low + k)), [], n, precision))["path"] == 1)
        assert plans.ok(plans.apply_matrix_plan(list(range(low, low + k)), [], first - 1, precision))["path"] == 0
        for n in (first - 1, first):
            sim, psi = _sim_with(n, precision, 520 + n)
            with sim:
                for targets in {tuple(range(low, low + k)), tuple(range(n - k, n)), tuple(range(n - 1, n - 1 - k, -1))}:
                    if precision == 64 or (0 in targets) == (low == 0):  # fp32: the switch depends on whether qubit 0 is in the subset
                        assert plans.ok(plans.apply_matrix_plan(targets, [], n, precision))["path"] == (1 if n == first else 0)
                    psi = _apply_and_check(sim, psi, random_unitary(1 << k, rng), targets, (), "switch")
                # one control on the larger register is the smaller one's count of environments
                free = [q for q in range(n) if q >= low + k]
                assert plans.ok(plans.apply_matrix_plan(list(range(low, low + k)), free[-1:], n, precision))["path"] == 0
                psi = _apply_and_check(sim, psi, random_unitary(1 << k, rng), list(range(low, low + k)), free[-1:], "switch")


# ---- the matrix path, n = 13 ----------------------------------------------------------------------------------------------------------------
def _n13_controls(targets):
    """No control; one: qubit 0, qubit 12 and the lowest qubit between two targets, each where it is no target; three: the first
    three of those and of 6, 9, 3, 10, 1 that are no targets."""
    between = [q for q in range(13) if targets and min(targets) < q < max(targets) and q not in targets][:1]
    singles = [q for q in [0, 12] + between if q not in targets]
    pool = [q for q in dict.fromkeys(singles + [6, 9, 3, 10, 1]) if q not in targets]
    return [[]] + [[q] for q in singles] + [pool[:3]]


@pytest.mark.parametrize("precision", PRECISIONS)
def test_matrix_path_subsets_and_controls(precision):
    """n = 13, every k: low, high, spread and shuffled targets, with qubit 0 and without; no control, one (qubit 0, qubit 12, one
    between two targets) and three.  Controls that are targets of a subset are left out for it."""
    n = 13
    rng = np.random.default_rng(513)
    sim, psi = _sim_with(n, precision, 513)
    seen = {"q0": 0, "q12": 0, "between": 0}
    with sim:
        for targets in N13_SUBSETS:
            sets = _n13_controls(targets)
            assert [len(c) for c in sets].count(1) >= 1 and len(sets[-1]) == 3
            for controls in sets:
                assert not set(controls) & set(targets)
                assert plans.ok(plans.apply_matrix_plan(targets, controls, n, precision))["path"] == 1
                psi = _apply_and_check(sim, psi, random_unitary(1 << len(targets), rng), targets, controls, "matrix")
                if len(controls) == 1:
                    seen["q0" if controls[0] == 0 else "q12" if controls[0] == 12 else "between"] += 1
    assert min(seen.values()) >= 8, seen


@pytest.mark.parametrize("precision", PRECISIONS)
def test_enough_controls_for_the_small_path(precision):
    """n = 13: control after control halves the environments until the plan leaves the matrix path; both sides of that are run."""
    n = 13
    rng = np.random.default_rng(514)
    sim, psi = _sim_with(n, precision, 514)
    with sim:
        for targets in ([1, 3, 6, 9, 12], [0, 7, 11], [4, 2]):
            pool = [q for q in (0, 5, 10, 8, 2, 11, 7, 4, 12, 1) if q not in targets]
            paths = []
            for c in range(1, len(pool) + 1):
                controls = pool[:c]
                paths.append(plans.ok(plans.apply_matrix_plan(targets, controls, n, precision))["path"])
                if len(paths) >= 2 and paths[-2:] == [0, 0]:
                    break
                psi = _apply_and_check(sim, psi, random_unitary(1 << len(targets), rng), targets, controls, "controls")
            assert 1 in paths and 0 in paths


# ---- exact cases ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", PRECISIONS)
def test_exact_cases(precision):
    """The identity and permutation matrices move values and round nothing: np.array_equal on the values (-0 == +0)."""
    n = 13
    rng = np.random.default_rng(530)
    sim, psi = _sim_with(n, precision, 530)
    swap = np.eye(4)[[0, 2, 1, 3]]
    toffoli = np.eye(8)[[0, 1, 2, 7, 4, 5, 6, 3]]                # on [control, control, target]
    cx = np.eye(4)[[0, 3, 2, 1]]                                 # on [control, target]
    perm32 = np.eye(32)[rng.permutation(32)]
    with sim:
        for U, targets, controls in ((np.eye(8), [2, 7, 11], []), (np.eye(2), [0], [5]), (np.eye(32), [0, 1, 2, 3, 4], [12]),
                                     (X, [0], []), (X, [12], []), (X, [6], [0]), (X, [0], [3, 9]),
                                     (swap, [0, 12], []), (swap, [5, 4], [0]), (toffoli, [3, 8, 0], []), (toffoli, [12, 1, 6], [0]),
                                     (perm32, [1, 3, 6, 9, 12], []), (perm32, [4, 0, 3, 2, 1], [8]), (perm32, [8, 9, 10, 11, 12], [0, 1])):
            count = plans.sweeps_launched("matrix")
            sim.apply_matrix(U, targets, controls)
            assert plans.sweeps_launched("matrix") == count + 1
            got = sim.read()
            want = matrix_ref.apply_matrix(psi, U, targets, controls)
            assert np.array_equal(got, want), (targets, controls)
            ones = sum(1 << q for q in controls)
            outside = (np.arange(1 << n) & ones) != ones
            assert np.array_equal(got[outside].view(np.uint64), psi[outside].view(np.uint64))
            psi = got
        # cx as a 4x4 against apply_cx, bit for bit in the values
        for control, target in ((0, 12), (12, 0), (3, 4), (7, 2)):
            with Simulator(n, precision=precision) as other:
                other.write(psi)
                other.apply_cx(control, target)
                want = other.read()
            sim.apply_matrix(cx, [control, target])
            psi = sim.read()
            assert np.array_equal(psi, want)


# ---- agreement with the existing routes -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", PRECISIONS)
def test_agreement_with_the_existing_routes(precision):
    n = 13
    rng = np.random.default_rng(540)
    start = rand_state(n, 540)
    # fp32: both routes round every amplitude they touch a few times (two sweeps for mcx, a fused block for the gates) to 2^-24 of
    # its size, and no amplitude exceeds the largest of the start state by more than the factor 8 of a 3-qubit gate
    tol = TOL if precision == 64 else 32 * 2.0 ** -24 * 8 * float(np.max(np.abs(start)))

    def both(via_matrix, via_route):
        out = []
        for run in (via_matrix, via_route):
            with Simulator(n, precision=precision) as sim:
                sim.write(start)
                run(sim)
                out.append(sim.read())
        worst = float(np.max(np.abs(out[0] - out[1])))
        print(f"routes p{precision}: max abs difference {worst:.3e}")
        assert worst < tol
        assert np.max(np.abs(out[0] - start)) > 1e-3             # something happened

    for q in (0, 6, 12):
        u = random_unitary(2, rng)
        both(lambda s: s.apply_matrix(u, [q]), lambda s: s.apply_1q(u, q))
    for q_hi, q_lo in ((1, 0), (12, 0), (9, 4)):
        u = random_unitary(4, rng)
        both(lambda s: s.apply_matrix(u, [q_lo, q_hi]), lambda s: s.apply_2q(u, q_hi, q_lo))
    theta = 0.83
    P = np.kron(X, np.kron(Z, X))                                # "X3 Z5 X9" on targets [3, 5, 9]: qubit 9 is the top bit
    R = np.cos(theta / 2) * np.eye(8) - 1j * np.sin(theta / 2) * P
    for controls in ((), (0,), (12, 7), (0, 1, 11)):
        both(lambda s: s.apply_matrix(R, [3, 5, 9], controls), lambda s: s.apply_pauli_rotation(theta, "X3 Z5 X9", controls))
    for controls, target in (((3, 8), 0), ((0, 12, 5), 7), ((1, 2, 3, 4), 12)):
        both(lambda s: s.apply_matrix(X, [target], controls), lambda s: s.apply_mcx(controls, target))


# ---- not unitary ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", PRECISIONS)
def test_projector_and_scale_are_a_collapse(precision):
    n = 13
    sim, psi = _sim_with(n, precision, 550)
    with sim:
        for qubits, outcome in (([4, 0, 12], 5), ([7], 1), ([1, 2, 3, 9, 10], 19)):
            p = sim.marginal_probabilities(qubits)[outcome]
            assert 0.0 < p < 1.0
            proj = np.zeros((1 << len(qubits), 1 << len(qubits)))
            proj[outcome, outcome] = 1.0
            psi = _apply_and_check(sim, psi, proj, qubits, (), "projector")
            assert abs(sim.norm2() - p) < (TOL if precision == 64 else 1e-6)
            sim.scale(1.0 / np.sqrt(p))
            got = sim.read()
            assert abs(sim.norm2() - 1.0) < (TOL if precision == 64 else 1e-6)
            want = psi / np.sqrt(p)
            assert np.max(np.abs(got - want)) < (TOL if precision == 64 else 1e-6)
            after = sim.marginal_probabilities(qubits)
            assert abs(after[outcome] - 1.0) < (TOL if precision == 64 else 1e-6) and np.count_nonzero(after) == 1
            psi = got


@pytest.mark.parametrize("precision", PRECISIONS)
def test_random_matrices_of_norm_one(precision):
    n = 13
    rng = np.random.default_rng(560)
    sim, psi = _sim_with(n, precision, 560)
    with sim:
        for targets, controls in (([], []), ([], [0, 4]), ([6], []), ([0, 12], [5]), ([2, 7, 11], []), ([0, 5, 6, 9], [12]), ([1, 3, 6, 9, 12], []),
                                  ([0, 1, 2, 3, 4], [7, 8])):
            sim.write(rand_state(n, 561))                        # a contraction shrinks the state: start from unit norm each time
            psi = _apply_and_check(sim, sim.read(), _contraction(1 << len(targets), rng), targets, controls, "contraction")


# ---- looping ------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _large_state(n):
    return rand_state(n, 570)                                    # once for all the cases of a size


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("controlled", [False, True])
@pytest.mark.parametrize("k", [3, 5])
def test_looping(k, controlled, precision):
    """Every workgroup walks its loop at least twice, whatever the device holds at once: low, high and mixed targets, without a
    control and under the top qubit."""
    n = 22 if precision == 64 else 23
    rng = np.random.default_rng(570 + k)
    controls = [n - 1] if controlled else []
    with Simulator(n, precision=precision) as sim:
        sim.write(_large_state(n))
        psi = sim.read()
        for targets in (list(range(k)), list(range(n - 1 - k, n - 1)), [n - 2, 3, 9, 7, 1][:k]):
            p = plans.ok(plans.apply_matrix_plan(targets, controls, n, precision))
            assert p["path"] == 1 and p["trips_per_workgroup"] >= 2
            psi = _apply_and_check(sim, psi, random_unitary(1 << k, rng), targets, controls, "looping")


# ---- stream and bits ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", PRECISIONS)
def test_equal_bits_whatever_the_grid(precision):
    n = 16
    rng = np.random.default_rng(580)
    start = rand_state(n, 580)
    with Simulator(n, precision=precision) as sim:
        for targets, controls in (([2, 9, 15], []), ([0, 5, 6, 11, 14], [3]), ([1], [0, 15]), ([4, 7, 8, 13], [])):
            U = random_unitary(1 << len(targets), rng)
            results = []
            for cap in (0, 0, 1, 7):                             # twice as it comes, then one workgroup, then seven
                sim.set_option(_lib.OPT_GRID_CAP, cap)
                sim.write(start)
                sim.apply_matrix(U, targets, controls)
                results.append(sim.read().view(np.uint64).copy())
            sim.set_option(_lib.OPT_GRID_CAP, 0)
            for other in results[1:]:
                assert np.array_equal(results[0], other)
            assert not np.array_equal(results[0], sim_bits(start, precision))


def sim_bits(state, precision):
    s = state.astype(np.complex64).astype(np.complex128) if precision == 32 else state
    return np.ascontiguousarray(s).view(np.uint64)


@pytest.mark.parametrize("precision", PRECISIONS)
def test_queued_gates_before_and_after(precision):
    n = 13
    tol = TOL if precision == 64 else 2e-6
    rng = np.random.default_rng(590)
    sim, psi = _sim_with(n, precision, 590)
    with sim:
        us = {q: random_unitary(2, rng) for q in (0, 4, 12)}
        for q, u in us.items():
            sim.apply_1q(u, q)                                   # queued: nothing has been flushed or waited for
            psi = np_apply_1q(psi, n, u, q)
        sim.apply_cx(12, 3)
        psi = np_apply_cx(psi, n, 12, 3)
        U = random_unitary(8, rng)
        count = plans.sweeps_launched("matrix")
        sim.apply_matrix(U, [12, 3, 0], [7])
        assert plans.sweeps_launched("matrix") == count + 1
        psi = matrix_ref.apply_matrix(psi, U, [12, 3, 0], [7])
        v = random_unitary(4, rng)
        sim.apply_2q(v, 9, 0)                                    # queued behind the sweep: it sees the sweep's result
        sim.apply_cx(0, 12)
        psi = np_apply_cx(np_apply_2q(psi, n, v, 9, 0), n, 0, 12)
        assert np.max(np.abs(sim.read() - psi)) < tol


@pytest.mark.parametrize("precision", PRECISIONS)
def test_fresh_state_and_partial_support(precision):
    n = 13
    tol = TOL if precision == 64 else 2e-6
    rng = np.random.default_rng(600)
    U = random_unitary(8, rng)
    with Simulator(n, precision=precision) as sim:               # never touched: |0...0> is still held lazily
        sim.apply_matrix(U, [12, 0, 5])
        want = np.zeros(1 << n, dtype=np.complex128)
        want[0] = 1.0
        want = matrix_ref.apply_matrix(want, U, [12, 0, 5])
        assert np.max(np.abs(sim.read() - want)) < tol
    with Simulator(n, precision=precision) as sim:               # a fresh state under a control: nothing moves
        sim.apply_matrix(U, [12, 0, 5], [3])
        got = sim.read()
        assert got[0] == 1.0 and np.count_nonzero(got) == 1
    with Simulator(n, precision=precision) as sim:               # three h on low qubits: the support is partial when the call settles it
        for q in (0, 1, 2):
            sim.apply_1q(H, q)
        sim.flush()
        sim.apply_matrix(U, [9, 12, 1], [0])
        want = np.zeros(1 << n, dtype=np.complex128)
        want[0] = 1.0
        for q in (0, 1, 2):
            want = np_apply_1q(want, n, H, q)
        want = matrix_ref.apply_matrix(want, U, [9, 12, 1], [0])
        got = sim.read()
        assert np.max(np.abs(got - want)) < tol
        assert np.count_nonzero(np.abs(got) > 1e-3) > 8          # the high targets are populated now


@pytest.mark.parametrize("precision", PRECISIONS)
def test_a_shard_that_holds_nothing(precision):
    rng = np.random.default_rng(610)
    with Simulator(13, precision=precision) as sim:
        sim.reset(holds_index0=False)
        before = plans.sweeps_launched("matrix")
        for targets, controls in (([], []), ([0], []), ([12, 3, 4], [0]), ([0, 1, 2, 3, 4], [])):
            sim.apply_matrix(random_unitary(1 << len(targets), rng), targets, controls)
        assert plans.sweeps_launched("matrix") == before
        assert _lib.load().qsim_holds_nothing(sim._h) == 1
        assert np.array_equal(sim.read(), np.zeros(1 << 13))
        sim.reset()
        sim.apply_matrix(random_unitary(8, rng), [12, 3, 4])
        assert plans.sweeps_launched("matrix") == before + 1


# ---- refusals -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", PRECISIONS)
def test_refusals(precision):
    lib = _lib.load()
    DP = POINTER(c_double)
    eyes = [np.ascontiguousarray(np.eye(1 << k, dtype=np.complex128).reshape(-1)).view(np.float64).copy() for k in range(6)]
    u = eyes[2]
    up = u.ctypes.data_as(DP)
    with Simulator(6, precision=precision) as sim:
        sim.write(rand_state(6, 1))
        state = sim.read().view(np.uint64).copy()
        before = plans.sweeps_launched("matrix")
        # the identity of the targets' size (of five qubits where the count itself is what is refused)
        call = lambda ts, cs=(), k=None, c=None: lib.qsim_apply_matrix(sim._h, eyes[min(len(ts), 5)].ctypes.data_as(DP), _ints(ts),
                                                                     len(ts) if k is None else k, _ints(cs), len(cs) if c is None else c)
        assert call([0, 1]) == _lib.QSIM_OK and call([0, 1], [5]) == _lib.QSIM_OK and call([], [2]) == _lib.QSIM_OK
        assert plans.sweeps_launched("matrix") == before + 3
        assert np.array_equal(sim.read().view(np.uint64), state)  # the identity, three times
        for ts, cs in (([0, 0], []), ([6], []), ([-1], []), ([2, 5, 2], []), ([0, 1, 2, 3, 4, 5], []), ([0], [0]), ([0, 1], [3, 1]), ([0], [6]),
                       ([0], [-1]), ([0], [2, 2])):
            assert call(ts, cs) == _lib.ERR_ARG, (ts, cs)
        assert call([0], (), k=-1) == _lib.ERR_ARG and call([0], [1], c=-1) == _lib.ERR_ARG
        assert lib.qsim_apply_matrix(sim._h, up, None, 1, None, 0) == _lib.ERR_ARG
        assert lib.qsim_apply_matrix(sim._h, up, _ints([0]), 1, None, 1) == _lib.ERR_ARG
        assert lib.qsim_apply_matrix(sim._h, None, _ints([0]), 1, None, 0) == _lib.ERR_ARG
        assert lib.qsim_apply_matrix(None, up, _ints([0]), 1, None, 0) == _lib.ERR_ARG
        for bad in (np.nan, np.inf, -np.inf):
            v = u.copy()
            v[5] = bad
            assert lib.qsim_apply_matrix(sim._h, v.ctypes.data_as(DP), _ints([0, 3]), 2, None, 0) == _lib.ERR_ARG
        assert lib.qsim_apply_matrix(sim._h, up, None, 0, None, 0) == _lib.QSIM_OK   # k = 0 needs no list: the scalar 1
        assert plans.sweeps_launched("matrix") == before + 4                           # nothing was launched for a refused call
        assert np.array_equal(sim.read().view(np.uint64), state)
        with pytest.raises(QsimError):
            sim.apply_matrix(np.eye(2), [0], [0])
        with pytest.raises(QsimError):
            sim.apply_matrix(np.eye(2), [6])
        with pytest.raises(ValueError):
            sim.apply_matrix(np.eye(4), [0])                     # the shape does not fit the targets
        with pytest.raises(ValueError):
            sim.apply_matrix(np.eye(64), [0, 1, 2, 3, 4, 5])
        assert plans.sweeps_launched("matrix") == before + 4
    with Simulator(2, precision=precision) as sim:
        assert lib.qsim_apply_matrix(sim._h, up, _ints([0, 1, 1]), 3, None, 0) == _lib.ERR_ARG  # k > n


@pytest.mark.parametrize("precision", PRECISIONS)
def test_the_operand_ring_outlives_the_states_it_served(precision):
    """The operand travels through a ring of pinned slots that belongs to the device, not to a state; a slot's event is recorded on the
    state's stream.  Forty states come and go, more than twice around the ring: a slot that a state used is free when the state has
    gone, and is not waited for on the stream that went with it (qsim_destroy tells the ring)."""
    n, targets, controls = 9, (7, 0, 4), (2,)
    rng = np.random.default_rng(90)
    first = None
    for i in range(40):
        U = _contraction(8, rng)
        sim, before = _sim_with(n, precision, 90)
        with sim:
            got = _apply_and_check(sim, before, U, targets, controls, f"ring, state {i}")
            first = first or (U, got)
    sim, before = _sim_with(n, precision, 90)  # the first state's call again, on the forty-first: the same bits
    with sim:
        sim.apply_matrix(first[0], targets, controls)
        assert np.array_equal(sim.read().view(np.uint64), first[1].view(np.uint64))
