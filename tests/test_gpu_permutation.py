"""Permutations of the basis states of up to ten target qubits under controls on the device (Simulator.apply_permutation,
qsim_apply_permutation; csrc/permutation.hip, csrc/permutation.cpp).

The checker is permutation_ref.apply_permutation (gather, index, scatter; pinned on the CPU by tests/test_permutation_cpu.py) on the
amplitudes READ BACK from the same state before the call — for an fp32 state `read()` is the exact widened contents.  Every comparison
is bit for bit: np.array_equal on .view(np.uint64), no tolerance, in both precisions.  The one exception is the composite test with
queued gates, which uses the project's 1e-10.  Every accepted call must raise the sweep counter by exactly one (the identity table is
swept like any other); every refused call raises it by zero and leaves the state's bits alone.
Sizes: n <= 4 (the tile is smaller than a workgroup), both sides of the path switch from the plan call (n - c = 11 | 12 | 13 in fp64,
12 | 13 | 14 in fp32), n = 13 for tables, target places and controls, n = 15 and 16 with two workgroups (several tiles each), and
n = 22 (fp64) / 23 (fp32), where the plan call reports two trips per workgroup at the default grid."""
import functools
import itertools
from ctypes import POINTER, c_uint32

import numpy as np
import pytest

import permutation_ref
from gpu_quantum_simulator_amd import Circuit, Cluster, Simulator, _lib, permutations, plans
from gpu_quantum_simulator_amd._marshal import ints as _ints
from helpers import np_apply_1q
from pauli_rot_ref import rand_state

pytestmark = pytest.mark.gpu
TOL = 1e-10
PRECISIONS = [64, 32]
H = np.array([[1, 1], [1, -1]]) / np.sqrt(2.0)
X = np.array([[0, 1], [1, 0]], dtype=np.complex128)


def _bits(state):
    return np.ascontiguousarray(state).view(np.uint64)


def _apply_and_check(sim, before, perm, targets, controls=(), inverse=False):
    """One call on the device against the checker on `before` (the state as read back), bit for bit; returns the state after it."""
    count = plans.sweeps_launched("permutation")
    sim.apply_permutation(perm, targets, controls, inverse=inverse)
    assert plans.sweeps_launched("permutation") == count + 1
    got = sim.read()
    want = permutation_ref.apply_permutation(before, permutations.inverse_table(perm) if inverse else perm, targets, controls)
    assert np.array_equal(_bits(got), _bits(want)), (sim.num_qubits, sim.precision, list(targets), list(controls))
    return got


def _sim_with(n, precision, seed, **options):
    sim = Simulator(n, precision=precision, **options)
    sim.write(rand_state(n, seed))
    return sim, sim.read()


def _tables(k, rng):
    """A random table, a single transposition and the cyclic shift j -> j + 1."""
    dim = 1 << k
    swap = np.arange(dim)
    if dim > 1:
        a, b = rng.choice(dim, 2, replace=False)
        swap[[a, b]] = swap[[b, a]]
    return [rng.permutation(dim), swap, (np.arange(dim) + 1) % dim]


# ---- registers smaller than a workgroup's tile ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("n", [0, 1, 2, 3, 4])
def test_small_registers_every_subset_and_control_choice(n, precision):
    rng = np.random.default_rng(800 + n)
    sim, psi = _sim_with(n, precision, 800 + n)
    with sim:
        for k in range(0, n + 1):
            for ts in itertools.combinations(range(n), k):
                rest = [q for q in range(n) if q not in ts]
                for c in range(0, len(rest) + 1):
                    for controls in itertools.combinations(rest, c):
                        for targets in {ts, ts[::-1]}:
                            p = plans.ok(plans.apply_permutation_plan(targets, controls, n, precision))
                            assert p["path"] == 0 and p["tiles"] == 1 and p["tile_bits"] == n - c
                            psi = _apply_and_check(sim, psi, rng.permutation(1 << k), targets, controls)


# ---- both sides of every boundary the plan reports --------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("offset", [-1, 0, 1])
def test_tile_boundaries(offset, precision):
    """n - c = B_max - 1 (one partial tile, the guarded instantiation), B_max (one whole tile) and B_max + 1 (two tiles), reached
    without a control and with one and two controls on a larger register."""
    full = 12 if precision == 64 else 13
    rng = np.random.default_rng(810 + offset)
    for c in (0, 1, 2):
        n = full + offset + c
        sim, psi = _sim_with(n, precision, 810 + n)
        with sim:
            for targets in ([0], [n - 1, 0, 5], list(range(n - 5 - c, n - c)), [7, 2, 9, 4]):
                pool = [q for q in (n - 1, 0, 3) if q not in targets] + [q for q in range(n) if q not in targets and q not in (n - 1, 0, 3)]
                controls = pool[:c]
                p = plans.ok(plans.apply_permutation_plan(targets, controls, n, precision))
                assert p["path"] == (0 if offset < 0 else 1) and p["tiles"] == (2 if offset > 0 else 1) and p["tile_bits"] == full + min(offset, 0)
                for perm in _tables(len(targets), rng)[:2]:
                    psi = _apply_and_check(sim, psi, perm, targets, controls)


# ---- n = 13: tables, target places, controls ----------------------------------------------------------------------------------------------
def _n13_targets(k, rng):
    n = 13
    low, top = list(range(k)), list(range(n - k, n))
    spread = sorted({(j * (n - 1)) // max(k - 1, 1) for j in range(k)}) if k > 1 else [6]
    if len(spread) != k:                                         # k = 9, 10: all but the qubits 4, 8 (and 6)
        spread = [q for q in range(n) if q not in (4, 8, 6, 2)[:n - k]]
    scrambled = [int(q) for q in rng.permutation(n)[:k]]
    return [low, top, spread, scrambled, top[::-1]]


def _n13_controls(targets):
    """No control; one: qubit 0 and qubit 12, each where it is no target, else the lowest free qubit; three (fewer where the
    register has no more): qubit 0, qubit 12 and others that are no targets."""
    n = 13
    free = [q for q in range(n) if q not in targets]
    singles = [q for q in (0, n - 1) if q in free] or free[:1]
    pool = list(dict.fromkeys(singles + [q for q in (6, 9, 3, 10, 1) if q in free] + free))
    return [[]] + [[q] for q in singles] + [pool[:3]]


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("k", [1, 2, 5, 9, 10])
def test_n13_tables_places_and_controls(k, precision):
    n = 13
    rng = np.random.default_rng(820 + k)
    sim, psi = _sim_with(n, precision, 820 + k)
    seen = set()
    with sim:
        for targets in _n13_targets(k, rng):
            assert len(set(targets)) == k
            for controls in _n13_controls(targets):
                assert not set(controls) & set(targets)
                seen |= {("q0" if q == 0 else "top" if q == n - 1 else "mid") for q in controls} | {len(controls)}
                p = plans.ok(plans.apply_permutation_plan(targets, controls, n, precision))
                assert p["tile_bits"] == min(12 if precision == 64 else 13, n - len(controls)) and p["tiles"] == 1 << (n - len(controls) - p["tile_bits"])
                for perm in _tables(k, rng):
                    psi = _apply_and_check(sim, psi, perm, targets, controls)
    assert {"q0", "top", 0, 1, 3} <= seen, seen


# ---- several tiles per workgroup ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", PRECISIONS)
def test_two_workgroups_walk_several_tiles(precision):
    """grid_cap = 2: two workgroups, a static assignment of the tiles.  n = 15 is 8 tiles in fp64 and 4 in fp32, n = 16 twice as many,
    so each workgroup walks at least four tiles in either precision; the bits equal those of the default grid, of one workgroup and of
    seven."""
    rng = np.random.default_rng(830)
    for n in (15, 16):
        start = rand_state(n, 830 + n)
        cases = [([n - 1, 3, 0, 8, 12, 5, 10, 2, 13, 7], []), (list(range(n - 10, n)), []), ([4, 11], [0, n - 1]), (list(range(9)), [9])]
        with Simulator(n, precision=precision, grid_cap=2) as sim:
            walked = 0
            for targets, controls in cases:
                perm = rng.permutation(1 << len(targets))
                walked = max(walked, plans.ok(plans.apply_permutation_plan(targets, controls, n, precision))["tiles"] // 2)
                sim.set_option(_lib.OPT_GRID_CAP, 2)
                sim.write(start)
                first = _bits(_apply_and_check(sim, sim.read(), perm, targets, controls)).copy()
                for cap in (0, 1, 7):
                    sim.set_option(_lib.OPT_GRID_CAP, cap)
                    sim.write(start)
                    sim.apply_permutation(perm, targets, controls)
                    assert np.array_equal(_bits(sim.read()), first), (n, targets, cap)
            assert walked >= (4 if n == 16 or precision == 64 else 2)


@functools.lru_cache(maxsize=None)
def _large_state(n):
    return rand_state(n, 840)


@pytest.mark.parametrize("precision", PRECISIONS)
def test_looping_at_the_default_grid(precision):
    """The size at which every workgroup of the default grid walks at least two tiles: one call, k = 10 spread over the register."""
    n = 22 if precision == 64 else 23
    targets = [n - 1, 3, 17, 8, 12, 5, 20, 10, 15, 0]
    assert plans.ok(plans.apply_permutation_plan(targets, [], n, precision))["trips_per_workgroup"] >= 2
    rng = np.random.default_rng(840)
    with Simulator(n, precision=precision) as sim:
        sim.write(_large_state(n))
        _apply_and_check(sim, sim.read(), rng.permutation(1 << 10), targets, [])


# ---- exact relations ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", PRECISIONS)
def test_inverse_restores_the_state(precision):
    n = 13
    rng = np.random.default_rng(850)
    sim, start = _sim_with(n, precision, 850)
    with sim:
        for targets, controls in (([12, 0, 5, 9, 1, 7, 3, 11, 2, 6], []), ([3, 8], [0]), (list(range(4, 13)), [0, 2]), ([], [4]), ([0], [])):
            perm = rng.permutation(1 << len(targets))
            moved = _apply_and_check(sim, start, perm, targets, controls)
            assert len(targets) < 2 or not np.array_equal(_bits(moved), _bits(start))
            back = _apply_and_check(sim, moved, perm, targets, controls, inverse=True)
            assert np.array_equal(_bits(back), _bits(start))


@pytest.mark.parametrize("precision", PRECISIONS)
def test_cx_table_equals_apply_cx(precision):
    n = 13
    sim, psi = _sim_with(n, precision, 860)
    with sim:
        for control, target in ((0, 12), (12, 0), (3, 4), (7, 2), (1, 0)):
            with Simulator(n, precision=precision) as other:
                other.write(psi)
                other.apply_cx(control, target)
                want = other.read()
            sim.apply_permutation([0, 1, 3, 2], [target, control])
            psi = sim.read()
            assert np.array_equal(_bits(psi), _bits(want)), (control, target)


# ---- order with the gate queue ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", PRECISIONS)
def test_queued_gates_land_first(precision):
    """Order finding's modular exponentiation at n = 12: h on 8 counting qubits and x on the work register's lowest qubit through run
    (queued, not flushed), then x -> 7^(2^j) x mod 15 on the work register under counting qubit j, for every j.  The replay is numpy
    at 1e-10.  fp32: the replay starts from the gates' state as a twin state holds it (the same circuit, read back), because an fp32
    h is 6e-8 from numpy's; from there on the permutations move bits and the comparison is as tight as in fp64."""
    n, counting, work = 12, list(range(8)), [8, 9, 10, 11]
    gates = [("h", q) for q in counting] + [("x", work[0])]
    circuit = Circuit.from_gates(n, gates)
    if precision == 64:
        want = np.zeros(1 << n, dtype=np.complex128)
        want[0] = 1.0
        for q in counting:
            want = np_apply_1q(want, n, H, q)
        want = np_apply_1q(want, n, X, work[0])
    else:
        with Simulator(n, precision=precision) as twin:
            twin.run(circuit)
            want = twin.read()
    with Simulator(n, precision=precision) as sim:
        sim.run(circuit)
        before = plans.sweeps_launched("permutation")
        for j in counting:
            a = pow(7, 1 << j, 15)
            sim.apply_modular_multiply(a, 15, work, controls=[j])
            want = permutation_ref.apply_permutation(want, permutations.modular_multiply_table(a, 15, 4), work, [j])
        assert plans.sweeps_launched("permutation") == before + len(counting)
        got = sim.read()
    worst = float(np.max(np.abs(got - want)))
    print(f"queued gates p{precision}: max abs err {worst:.3e}")
    assert worst < TOL
    # the work register holds 7^x mod 15 for the counting value x: 1, 7, 4, 13 in turn, each 64 times with weight 1/16
    x = np.arange(256)
    powers = np.array([pow(7, int(v), 15) for v in x])
    assert np.allclose(np.abs(got[x | (powers << 8)]), 1.0 / 16.0, atol=1e-6) and np.count_nonzero(np.abs(got) > 1e-6) == 256


@pytest.mark.parametrize("precision", PRECISIONS)
def test_fresh_state_moves_index_zero(precision):
    n = 13
    rng = np.random.default_rng(870)
    with Simulator(n, precision=precision) as sim:
        for targets in ([12, 0, 5, 9], [3], list(range(10)), [11, 12]):
            perm = rng.permutation(1 << len(targets))
            if perm[0] == 0:
                perm = np.roll(perm, 1)
            sim.reset()                                          # |0...0>, held lazily: nothing has run
            count = plans.sweeps_launched("permutation")
            sim.apply_permutation(perm, targets)
            assert plans.sweeps_launched("permutation") == count + 1
            got = sim.read()
            at = permutation_ref.deposit(int(perm[0]), targets)
            assert at != 0 and got[at] == 1.0 and np.count_nonzero(got) == 1, (targets, at)
        sim.reset()                                              # under a control nothing moves
        sim.apply_permutation([1, 0], [4], [7])
        got = sim.read()
        assert got[0] == 1.0 and np.count_nonzero(got) == 1


@pytest.mark.parametrize("precision", PRECISIONS)
def test_a_state_that_holds_nothing(precision):
    with Simulator(13, precision=precision) as sim:
        sim.reset(holds_index0=False)
        before = plans.sweeps_launched("permutation")
        sim.apply_permutation([1, 0], [5])
        sim.apply_permutation(np.arange(1024)[::-1], list(range(10)), [12])
        assert plans.sweeps_launched("permutation") == before and _lib.load().qsim_holds_nothing(sim._h) == 1
        assert np.array_equal(sim.read(), np.zeros(1 << 13))


def test_helpers_on_the_device():
    """apply_function_xor and apply_modular_add go through the same call: against the checker with the builders' tables."""
    n = 13
    sim, psi = _sim_with(n, 64, 880)
    rng = np.random.default_rng(880)
    with sim:
        values = rng.integers(0, 8, 32)
        count = plans.sweeps_launched("permutation")
        sim.apply_function_xor(values, [12, 0, 3, 7, 5], [1, 9, 4], controls=[2])
        want = permutation_ref.apply_permutation(psi, permutations.xor_function_table(values, 5, 3), [12, 0, 3, 7, 5, 1, 9, 4], [2])
        psi = sim.read()
        assert np.array_equal(_bits(psi), _bits(want))
        sim.apply_modular_add(77, 1000, list(range(3, 13)))
        want = permutation_ref.apply_permutation(psi, permutations.modular_add_table(77, 1000, 10), list(range(3, 13)))
        assert np.array_equal(_bits(sim.read()), _bits(want)) and plans.sweeps_launched("permutation") == count + 2


def test_cluster_has_no_permutation_methods():
    for name in ("apply_permutation", "apply_function_xor", "apply_modular_add", "apply_modular_multiply"):
        assert hasattr(Simulator, name) and not hasattr(Cluster, name)


# ---- refusals -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", PRECISIONS)
def test_refusals(precision):
    lib = _lib.load()
    UP = POINTER(c_uint32)
    table = lambda values: np.ascontiguousarray(values, dtype=np.uint32)
    ident = [table(np.arange(1 << k)) for k in range(12)]
    with Simulator(12, precision=precision) as sim:
        sim.write(rand_state(12, 2))
        state = _bits(sim.read()).copy()
        before = plans.sweeps_launched("permutation")
        call = lambda ts, cs=(), k=None, c=None, perm=None: lib.qsim_apply_permutation(
            sim._h, (ident[min(len(ts), 11)] if perm is None else perm).ctypes.data_as(UP), _ints(ts), len(ts) if k is None else k, _ints(cs),
            len(cs) if c is None else c)
        assert call([0, 1]) == _lib.QSIM_OK and call([0, 1], [5]) == _lib.QSIM_OK and call([], [2]) == _lib.QSIM_OK
        assert lib.qsim_apply_permutation(sim._h, ident[0].ctypes.data_as(UP), None, 0, None, 0) == _lib.QSIM_OK   # k = 0 needs no list
        assert plans.sweeps_launched("permutation") == before + 4                           # the identity is swept like any other table
        assert np.array_equal(_bits(sim.read()), state)
        before = plans.sweeps_launched("permutation")
        for ts, cs in (([0, 0], []), ([12], []), ([-1], []), ([2, 5, 2], []), (list(range(11)), []), ([0], [0]), ([0, 1], [3, 1]), ([0], [12]),
                       ([0], [-1]), ([0], [2, 2])):
            assert call(ts, cs) == _lib.ERR_ARG, (ts, cs)
        assert call([0], (), k=-1) == _lib.ERR_ARG and call([0], [1], c=-1) == _lib.ERR_ARG
        assert lib.qsim_apply_permutation(sim._h, ident[1].ctypes.data_as(UP), None, 1, None, 0) == _lib.ERR_ARG
        assert lib.qsim_apply_permutation(sim._h, ident[1].ctypes.data_as(UP), _ints([0]), 1, None, 1) == _lib.ERR_ARG
        assert lib.qsim_apply_permutation(sim._h, None, _ints([0]), 1, None, 0) == _lib.ERR_ARG
        assert lib.qsim_apply_permutation(None, ident[1].ctypes.data_as(UP), _ints([0]), 1, None, 0) == _lib.ERR_ARG
        assert call([0, 3], perm=table([0, 1, 2, 4])) == _lib.ERR_ARG        # an entry >= 2^k
        assert call([0, 3], perm=table([0, 1, 1, 3])) == _lib.ERR_ARG        # two equal entries
        assert call([], perm=table([1])) == _lib.ERR_ARG
        with Simulator(3, precision=precision) as small:
            assert lib.qsim_apply_permutation(small._h, ident[4].ctypes.data_as(UP), _ints([0, 1, 2, 3]), 4, None, 0) == _lib.ERR_ARG   # k > n
        for bad in (lambda: sim.apply_permutation([0, 1, 2], [0, 1]), lambda: sim.apply_permutation([0, 2, 2, 3], [0, 1]),
                    lambda: sim.apply_permutation([0, 1.5], [0])):
            with pytest.raises(ValueError):
                bad()
        assert plans.sweeps_launched("permutation") == before
        assert np.array_equal(_bits(sim.read()), state)
