"""Reduced density matrices of 6 to 10 qubits on the device (Simulator.subsystem_density_matrix, qsim_subsystem_density;
csrc/subsystem.hip, csrc/subsystem.cpp).

The checker is density_ref.reduced_density (a tensordot, pinned on the CPU) on the amplitudes READ BACK from the same state — for an
fp32 state `read()` is the exact widened contents.  Tolerance 1e-10 absolute, the project's parity tolerance, in both precisions, by
the argument at the top of tests/test_gpu_density.py: a unit-norm state, products exact (fp32 amplitudes, widened) or once rounded
(fp64), only the order of the fp64 additions differs from numpy's; the worst case for 2^16 environments is 7e-12, and any index or
pairing mistake shows at 1e-2.  Every comparison also asks for exact Hermiticity, an imaginary diagonal of +0 and the trace of
norm2().  Sizes are the smallest at which each mechanism exists, taken from the plan call: both sides of the switch from the plain
kernel to blocks, one block against several (n = 13), and the smallest registers with two slices and two trips per workgroup."""
import ctypes
from ctypes import c_int

import numpy as np
import pytest

import density_ref
from gpu_quantum_simulator_amd import Simulator, _lib, plans
from gpu_quantum_simulator_amd._marshal import ints as _ints
from gpu_quantum_simulator_amd._lib import QsimError
from helpers import random_unitary
from pauli_rot_ref import rand_state

pytestmark = pytest.mark.gpu
TOL = 1e-10
PRECISIONS = [64, 32]
H = np.array([[1, 1], [1, -1]]) / np.sqrt(2.0)


def _check(sim, psi, qubits, label=""):
    """rho of `qubits` against the checker on psi (the state as read back), and what every result owes."""
    got = sim.subsystem_density_matrix(qubits)
    want = density_ref.reduced_density(psi, qubits)
    k = len(qubits)
    assert got.shape == (1 << k, 1 << k) and got.dtype == np.complex128
    worst = float(np.max(np.abs(got - want)))
    print(f"{label} n={sim.num_qubits} p{sim.precision} qubits={list(qubits)}: max abs err {worst:.3e}")
    assert worst < TOL
    assert np.array_equal(got, got.conj().T) and np.array_equal(np.imag(np.diagonal(got)), np.zeros(1 << k))
    assert not np.any(np.signbit(np.imag(np.diagonal(got))))
    assert abs(float(np.real(np.trace(got))) - sim.norm2()) < TOL
    return got


def _sim_with(n, precision, seed):
    sim = Simulator(n, precision=precision)
    sim.write(rand_state(n, seed))
    return sim, sim.read()


def _shuffled(qs, seed):
    return [int(q) for q in np.random.default_rng(seed).permutation(qs)]


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("k", [6, 10])
def test_path_switch(k, precision):
    """n = k and k + 1 take the plain kernel; the next register is the smallest for blocks: four environments, one matrix step."""
    first = next(n for n in range(k, k + 8) if plans.ok(plans.subsystem_density_plan(list(range(k)), n, precision))["path"] == 1)
    assert first - k == 2
    for n in range(k, first + 1):
        sim, psi = _sim_with(n, precision, 520 + n)
        with sim:
            for qs in {tuple(range(k)), tuple(range(n - k, n)), tuple(range(n - 1, n - 1 - k, -1))}:
                assert plans.ok(plans.subsystem_density_plan(list(qs), n, precision))["path"] == (1 if n == first else 0)
                _check(sim, psi, list(qs), "switch")


@pytest.mark.parametrize("precision", PRECISIONS)
def test_one_block_against_several(precision):
    """n = 13: the largest subset whose G is one block and the smallest with off-diagonal blocks, on the lowest and the highest
    qubits and on spread subsets with qubit 0 (fp32: the slot is a row bit) and without (an environment bit); k = 10 too."""
    n = 13
    upper = {k: plans.ok(plans.subsystem_density_plan(list(range(k)), n, precision))["upper_blocks"] for k in range(6, 11)}
    one, several = max(k for k in upper if upper[k] == 1), min(k for k in upper if upper[k] > 1)
    assert several == one + 1
    sim, psi = _sim_with(n, precision, 513)
    with sim:
        for k in (one, several):
            spread0 = [(j * (n - 1)) // (k - 1) for j in range(k)]   # 0 ... 12
            spread1 = [1 + (j * (n - 2)) // (k - 1) for j in range(k)]  # 1 ... 12
            for qs in (list(range(k)), list(range(n - k, n)), spread0, spread1):
                assert len(set(qs)) == k
                for order in (qs, _shuffled(qs, 7 * k + qs[1])):
                    p = plans.ok(plans.subsystem_density_plan(order, n, precision))
                    assert p["path"] == 1 and p["upper_blocks"] == upper[k]
                    _check(sim, psi, order, "blocks")
        _check(sim, psi, [12, 0, 3, 4, 5, 11, 7, 8, 9, 1], "blocks")
    sim, psi = _sim_with(14, precision, 514)
    with sim:
        _check(sim, psi, [2, 3, 4, 5, 6, 7, 8, 10, 12, 13], "blocks")


def _looping_size(k, precision, high):
    """The smallest register at which the plan reports two slices or more and two trips or more per workgroup."""
    for n in range(k + 2, 24):
        qs = list(range(n - k, n)) if high else list(range(k))
        p = plans.ok(plans.subsystem_density_plan(qs, n, precision))
        if p["slices"] >= 2 and p["trips_per_workgroup"] >= 2:
            return n, qs
    raise AssertionError("no register up to 23 qubits loops")


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("k", [6, 10])
def test_several_slices_and_a_loop_that_trips(k, precision):
    for high in (False, True):
        n, qs = _looping_size(k, precision, high)
        assert n <= (22 if precision == 64 else 23)
        sim, psi = _sim_with(n, precision, 530 + n)
        with sim:
            _check(sim, psi, qs, "looping")


@pytest.mark.parametrize("precision", PRECISIONS)
def test_agreement_at_the_seam(precision):
    n = 13
    sim, psi = _sim_with(n, precision, 541)
    with sim:
        for qs in ([0, 1, 2, 3, 4], [12, 3, 7, 0, 9], [5], []):
            assert np.array_equal(sim.subsystem_density_matrix(qs).view(np.uint64), sim.reduced_density_matrix(qs).view(np.uint64))
        for six, drop in (([12, 3, 7, 0, 9, 5], 5), ([1, 2, 3, 4, 5, 6], 0), ([12, 11, 10, 9, 8, 7], 3)):
            rho6 = _check(sim, psi, six, "seam").reshape((2,) * 12)  # axes: row bits top first, then column bits top first
            traced = np.trace(rho6, axis1=5 - drop, axis2=11 - drop).reshape(32, 32)
            five = sim.reduced_density_matrix(six[:drop] + six[drop + 1:])
            assert np.max(np.abs(traced - five)) < TOL


@pytest.mark.parametrize("precision", PRECISIONS)
def test_equal_bits_and_state_untouched(precision):
    for k in (6, 10):
        n, qs = _looping_size(k, precision, False)
        sim, _ = _sim_with(n, precision, 550 + n)
        with sim:
            before = sim.read().view(np.uint64).copy()
            first = sim.subsystem_density_matrix(qs)
            assert np.array_equal(sim.subsystem_density_matrix(qs).view(np.uint64), first.view(np.uint64))
            for cap in (1, 7):                                   # the option does not apply: the sums keep their order
                sim.set_option(_lib.OPT_GRID_CAP, cap)
                assert np.array_equal(sim.subsystem_density_matrix(qs).view(np.uint64), first.view(np.uint64))
            sim.set_option(_lib.OPT_GRID_CAP, 0)
            assert np.max(np.abs(first)) > 1e-4
            assert np.array_equal(sim.read().view(np.uint64), before)


@pytest.mark.parametrize("precision", PRECISIONS)
def test_bell_pairs(precision):
    """n = 14, qubits q and q + 7 in a Bell state: seven halves are maximally mixed."""
    n = 14
    with Simulator(n, precision=precision) as sim:
        for q in range(7):
            sim.apply_1q(H, q)
            sim.apply_cx(q, q + 7)
        for qs in (list(range(7)), [7, 1, 9, 3, 11, 5, 13], list(range(13, 6, -1))):
            assert abs(sim.entanglement_entropy(qs) - 7.0) < 1e-6 and abs(sim.purity(qs) - 2.0 ** -7) < 1e-6
            w = sim.entanglement_spectrum(qs)
            assert w.shape == (128,) and w.dtype == np.float64 and np.all(np.diff(w) <= 0.0)
            assert np.max(np.abs(w - 2.0 ** -7)) < 1e-6
        # both halves of three pairs and one half of four more: four bits
        assert abs(sim.entanglement_entropy([0, 7, 1, 8, 2, 9, 3, 4, 5, 6]) - 4.0) < 1e-6


@pytest.mark.parametrize("precision", PRECISIONS)
def test_product_state_and_the_complement_route(precision):
    n = 13
    rng = np.random.default_rng(22)
    with Simulator(n, precision=precision) as sim:
        for q in range(n):
            sim.apply_1q(random_unitary(2, rng), q)
        for qs in ([0, 1, 2, 3, 4, 5], [12, 5, 3, 4, 9, 0, 7, 11], list(range(3, 13))):
            assert abs(sim.purity(qs) - 1.0) < 1e-5 and abs(sim.entanglement_entropy(qs)) < 1e-3
            assert abs(sim.entanglement_spectrum(qs)[0] - 1.0) < 1e-5
    sim, _ = _sim_with(n, precision, 561)
    with sim:
        eleven, two = [q for q in range(n) if q not in (4, 9)], [4, 9]
        assert abs(sim.entanglement_entropy(eleven) - sim.entanglement_entropy(two)) < 1e-9
        assert abs(sim.purity(eleven[::-1]) - sim.purity(two)) < 1e-9
        assert sim.entanglement_spectrum(eleven).shape == (4,)
        with pytest.raises(QsimError):
            sim.subsystem_density_matrix(eleven)                 # rho itself of 11 qubits is refused


@pytest.mark.parametrize("precision", PRECISIONS)
def test_a_shard_that_holds_nothing(precision):
    with Simulator(13, precision=precision) as sim:
        sim.reset(holds_index0=False)
        before = plans.sweeps_launched("subsystem")
        for qs in ([0, 1, 2, 3, 4, 5], list(range(3, 13))):
            assert np.array_equal(sim.subsystem_density_matrix(qs), np.zeros((1 << len(qs), 1 << len(qs))))
        assert plans.sweeps_launched("subsystem") == before
        sim.reset()
        got = sim.subsystem_density_matrix([12, 3, 4, 0, 1, 2])   # never touched: |0...0> is still held lazily
        assert got[0, 0] == 1.0 and np.count_nonzero(got) == 1
        assert plans.sweeps_launched("subsystem") == before + 1


@pytest.mark.parametrize("precision", PRECISIONS)
def test_errors(precision):
    lib = _lib.load()
    out = (ctypes.c_double * (2 << 12))()
    with Simulator(7, precision=precision) as sim:
        sim.write(rand_state(7, 1))
        state = sim.read().view(np.uint64).copy()
        before, density_before = plans.sweeps_launched("subsystem"), plans.sweeps_launched("density")
        call = lambda qs, k=None: lib.qsim_subsystem_density(sim._h, _ints(qs), len(qs) if k is None else k, out)
        assert call([0, 1, 2, 3, 4, 5]) == _lib.QSIM_OK
        assert plans.sweeps_launched("subsystem") == before + 1
        assert call([0, 1]) == _lib.QSIM_OK                      # forwarded: the one-wave call's sweep
        assert plans.sweeps_launched("subsystem") == before + 1 and plans.sweeps_launched("density") == density_before + 1
        for qs in ([0, 0], [7], [-1], [2, 5, 2], [0, 1, 2, 3, 4, 5, 5], [0, 1, 2, 3, 4, 5, 6, 7]):
            assert call(qs) == _lib.ERR_ARG
        assert call([0], -1) == _lib.ERR_ARG
        assert lib.qsim_subsystem_density(sim._h, None, 1, out) == _lib.ERR_ARG
        assert lib.qsim_subsystem_density(sim._h, None, 0, out) == _lib.QSIM_OK
        assert lib.qsim_subsystem_density(sim._h, (c_int * 1)(0), 1, None) == _lib.ERR_ARG
        assert lib.qsim_subsystem_density(None, (c_int * 1)(0), 1, out) == _lib.ERR_ARG
        assert plans.sweeps_launched("subsystem") == before + 1  # nothing was launched for a refused call
        assert np.array_equal(sim.read().view(np.uint64), state)   # nor did a successful one touch the state
    with Simulator(12, precision=precision) as sim:
        before = plans.sweeps_launched("subsystem")
        assert lib.qsim_subsystem_density(sim._h, (c_int * 11)(*range(11)), 11, out) == _lib.ERR_ARG
        with pytest.raises(QsimError):
            sim.subsystem_density_matrix(list(range(11)))
        with pytest.raises(QsimError):
            sim.entanglement_entropy(list(range(11)) + [3])       # a repeated qubit takes no complement
        assert plans.sweeps_launched("subsystem") == before
        with pytest.raises(QsimError):
            sim.reduced_density_matrix([0, 1, 2, 3, 4, 5])        # the one-wave entry keeps its limit
