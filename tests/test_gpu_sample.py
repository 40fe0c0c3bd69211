"""Shots drawn on the device: Simulator.sample_shots / sample_counts (qsim_sample_shots; csrc/sample.hip, csrc/sample.cpp).

The checker is numpy (tests/sample_ref.py, pinned by tests/test_sample_cpu.py) on the amplitudes READ BACK — for an fp32 state `read()`
is the exact widened contents, so the rounding of a write cancels.  It does not know the device's order of summation: a returned index
must be ADMISSIBLE (p_i > 0 and E_(i-1) - gamma < r <= E_i + gamma, gamma = 2^(n-52) E_last, the any-order bound), a DETERMINED draw
(farther than gamma from both edges of its interval) must return exactly searchsorted(E, r), and at least 99 % of the draws of every
test must be determined.  One test has no tolerance at all: 64 amplitudes of exactly 1/8, every partial sum exact in any order.
Sizes come from plans.sample_geometry (cb: bits of a chunk, gb: bits of a group): registers below, at and above one chunk (the plain
path, exactly one chunk, several chunks of one group), several groups with empty ones among them, and shot counts around the four
waves of a workgroup."""

import numpy as np
import pytest

import sample_ref
from gpu_quantum_simulator_amd import Circuit, Simulator, _lib, circuits, plans
from pauli_rot_ref import rand_state

pytestmark = pytest.mark.gpu
PRECISIONS = [64, 32]
EDGES = [0.0, 1e-300, 1.0]


def _geometry(n):
    g = plans.ok(plans.sample_geometry(n))
    return g["chunk_bits"], g["group_bits"]


CB, GB = _geometry(30)
DENSE_SIZES = sorted({1, 3, CB - 1, CB, CB + 1, 12, 13})


def _draws(count, seed, edges=True):
    u = np.random.default_rng(seed).random(count)
    return np.concatenate((u, EDGES)) if edges else u


def _loaded(n, precision, psi, **options):
    sim = Simulator(n, precision=precision, **options)
    sim.write(psi)
    return sim


# ---- dense states: the plain path, one chunk, several chunks of one group --------------------------------------------------------------
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("n", DENSE_SIZES)
def test_dense_random_states(n, precision):
    assert _geometry(n) == (min(CB, n), min(GB, n))
    draws = _draws(1000, 40 + n)
    with _loaded(n, precision, rand_state(n, 20 + n)) as sim:
        got = sim.sample_shots(draws=draws)
        assert got.dtype == np.uint64
        sample_ref.check(n, sim.read(), draws, got, f"dense p{precision}")


# ---- several groups, empty ones among them ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", PRECISIONS)
def test_several_groups_with_empty_ones(precision):
    n = GB + 2
    N, G = 1 << n, 1 << GB
    rng = np.random.default_rng(77)
    # groups 0 and 2 wholly empty; 4095 amplitudes in groups 1 and 3, and the last index
    where = np.concatenate((G + rng.choice(G, 2048, replace=False), 3 * G + rng.choice(G - 1, 2047, replace=False), [N - 1]))
    assert np.unique(where).size == 4096
    psi = np.zeros(N, dtype=np.complex128)
    psi[where] = rng.standard_normal(4096) + 1j * rng.standard_normal(4096)
    psi /= np.linalg.norm(psi)
    draws = _draws(4096, 78)
    with _loaded(n, precision, psi) as sim:
        got = sim.sample_shots(draws=draws)
        amps = sim.read()
        assert np.count_nonzero(amps[:G]) == 0 and np.count_nonzero(amps[2 * G:3 * G]) == 0 and amps[-1] != 0
        sample_ref.check(n, amps, draws, got, f"groups p{precision}")


# ---- exact arithmetic: no tolerance ----------------------------------------------------------------------------------------------------
def _exact_indices(n):
    """64 indices: 0 and 2^n - 1, both ends of the trips of a wave, of chunks and of groups, and others in between."""
    N, C, G = 1 << n, 1 << CB, 1 << GB
    idx = {0, 1, 63, 64, 127, 128, C - 1, C, C + 1, 2 * C - 1, 2 * C, 7 * C + 65, G - C, G - 1, G, G + 1, G + C - 1, G + C, N - C, N - C + 63, N - 2, N - 1}
    k = 1
    while len(idx) < 64:  # one index in each of a spread of chunks, walking through the trips and lanes
        idx.add((37 * k * C + 29 * k) % N)
        k += 1
    assert len(idx) == 64
    return sorted(idx)


@pytest.mark.parametrize("precision", PRECISIONS)
def test_exact_eighths_pin_the_rule(precision):
    n = GB + 1
    idx = _exact_indices(n)
    psi = np.zeros(1 << n, dtype=np.complex128)
    psi[idx[0::2]] = 0.125
    psi[idx[1::2]] = 0.125j
    eps = 2.0 ** -30
    draws, want = [0.0, 1.0], [idx[0], idx[63]]
    for j in range(65):  # E at the j-th of the indices (from 1) is j / 64 exactly: r = j / 64 is reached there (>=), r just above only by the next
        if j >= 1:
            draws += [j / 64, j / 64 - eps]
            want += [idx[j - 1], idx[j - 1]]
        if j <= 63:
            draws += [j / 64 + eps]
            want += [idx[j]]
    draws = np.array(draws)
    with _loaded(n, precision, psi) as sim:
        assert np.array_equal(sim.read(), psi)
        got = sim.sample_shots(draws=draws)
    assert np.array_equal(got, np.array(want, dtype=np.uint64)), np.flatnonzero(got != np.array(want, dtype=np.uint64))


# ---- the grid: equal bits whatever QSIM_OPT_GRID_CAP is ----------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", PRECISIONS)
def test_results_do_not_depend_on_the_grid(precision):
    n = 13
    psi, draws = rand_state(n, 91), _draws(1000, 92)
    runs = {}
    for cap in (0, 1, 3):
        with _loaded(n, precision, psi, grid_cap=cap) as sim:
            runs[cap] = sim.sample_shots(draws=draws)
            if cap == 0:
                sample_ref.check(n, sim.read(), draws, runs[cap], f"grid p{precision}")
    assert runs[1].tobytes() == runs[0].tobytes() and runs[3].tobytes() == runs[0].tobytes()


# ---- shot counts around a workgroup of four waves ---------------------------------------------------------------------------------------
def test_shot_counts_around_a_workgroup():
    n = 11
    draws = _draws(257, 93, edges=False)
    with _loaded(n, 64, rand_state(n, 94)) as sim:
        amps = sim.read()
        whole = sim.sample_shots(draws=draws)
        sample_ref.check(n, amps, draws, whole, "257 shots")
        for shots in (0, 1, 3, 4, 5):
            got = sim.sample_shots(draws=draws[:shots])
            assert got.shape == (shots,) and np.array_equal(got, whole[:shots])
        assert sim.sample_shots(0).shape == (0,) and sim.sample_counts(0) == {}


# ---- qubit lists -----------------------------------------------------------------------------------------------------------------------
def test_qubit_lists_extract_the_bits_of_the_index():
    n = 10
    draws = _draws(500, 95)
    rng = np.random.default_rng(96)
    with _loaded(n, 64, rand_state(n, 97)) as sim:
        full = sim.sample_shots(draws=draws)
        sample_ref.check(n, sim.read(), draws, full, "qubit lists")
        for qubits in ([0], [n - 1], [4], list(rng.permutation(n)), list(rng.permutation(n)[:4]), list(range(n)), range(3)):
            got = sim.sample_shots(draws=draws, qubits=qubits)
            assert np.array_equal(got, sample_ref.outcome_bits(full, list(qubits))), list(qubits)
        assert np.array_equal(sim.sample_shots(draws=draws, qubits=list(range(n))), full)


def test_refusals():
    n = 6
    good = np.array([0.25, 0.5])
    with _loaded(n, 64, rand_state(n, 98)) as sim:
        before = sim.read().tobytes()
        for kwargs in ({"draws": good, "qubits": [1, 1]}, {"draws": good, "qubits": [n]}, {"draws": good, "qubits": [-1]},
                       {"draws": good, "qubits": list(range(n)) * 11}, {"draws": [0.25, float("nan")]}, {"draws": [1.5]}, {"draws": [-1e-9]}):
            with pytest.raises(_lib.QsimError) as err:
                sim.sample_shots(**kwargs)
            assert err.value.code == _lib.ERR_ARG and "qsim_sample_shots" in str(err.value), kwargs
        with pytest.raises(ValueError):
            sim.sample_shots()
        with pytest.raises(ValueError):
            sim.sample_shots(3, draws=good)
        assert sim.read().tobytes() == before
        sim.write(np.zeros(1 << n, dtype=np.complex128))
        with pytest.raises(_lib.QsimError) as err:
            sim.sample_shots(draws=good)
        assert err.value.code == _lib.ERR_ARG and "total" in str(err.value)


# ---- settling: queued gates and deferred X flips are materialised first; the state is untouched -------------------------------------------
def test_sampling_settles_a_queued_circuit_and_leaves_the_state_alone():
    n = 14
    gates = [g for g in circuits.random_gates(n, 480, 99, "all") if g[0] != "x"][:160] + [("x", q) for q in (0, 5, 9, 13)]
    draws = _draws(1000, 100)
    with Simulator(n, fuse=3, pingpong=2, defer_flips=2) as sim:
        sim.run(Circuit.from_gates(n, gates))  # queued, not flushed
        got = sim.sample_shots(draws=draws)
        amps = sim.read().copy()
        print("deferred flips:", sim.deferred_flip_stats())
        sample_ref.check(n, amps, draws, got, "settled")
        assert np.array_equal(sim.sample_shots(draws=draws), got)
        assert sim.read().tobytes() == amps.tobytes()
    with Simulator(n, fuse=3, pingpong=2, defer_flips=2) as sim:  # the same circuit, flushed and read without a sample in between
        sim.run(Circuit.from_gates(n, gates))
        assert sim.read().tobytes() == amps.tobytes()


# ---- an unnormalised state samples |a|^2 / norm2 -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", PRECISIONS)
def test_unnormalised_state_is_scaled_by_its_total(precision):
    n = 11
    psi, draws = rand_state(n, 101), _draws(1000, 102)
    with _loaded(n, precision, psi) as sim:
        unit = sim.sample_shots(draws=draws)
    with _loaded(n, precision, 0.5 * psi) as sim:
        amps = sim.read()
        got = sim.sample_shots(draws=draws)
        sample_ref.check(n, amps, draws, got, f"half p{precision}")
    assert abs(np.sum(sample_ref.probabilities(amps)) - 0.25) < 1e-6
    assert np.mean(got == unit) > 0.99 and np.count_nonzero(got == (1 << n) - 1) < 10  # halving is exact: the same outcomes, no pile-up on the last index


# ---- against the reference-parity path -----------------------------------------------------------------------------------------------------
def test_agrees_with_sample_on_determined_draws():
    n = 12
    draws = _draws(1000, 103, edges=False)
    with _loaded(n, 64, rand_state(n, 104)) as sim:
        new, old = sim.sample_shots(draws=draws), sim.sample(draws)
        _, want, determined, *_ = sample_ref.classify(n, sim.read(), draws)
    assert np.mean(determined) >= sample_ref.MIN_DETERMINED
    assert np.array_equal(new[determined], old[determined]) and np.array_equal(new[determined], want[determined])


# ---- counts ----------------------------------------------------------------------------------------------------------------------------------
def test_counts_of_a_ghz_state():
    n, shots = 10, 10_000
    psi = np.zeros(1 << n, dtype=np.complex128)
    psi[0] = psi[-1] = 1 / np.sqrt(2)
    with _loaded(n, 64, psi) as sim:
        got = sim.sample_counts(shots, seed=5)
        again = sim.sample_counts(shots, seed=5)
        draws = np.random.default_rng(5).random(shots)
        _, want, determined, *_ = sample_ref.classify(n, sim.read(), draws)
        low = sim.sample_counts(shots, qubits=[0, n - 1], seed=5)
    assert np.all(determined)
    assert got == sample_ref.counts(want) and got == again
    assert list(got) == sorted(got) == [0, (1 << n) - 1] and sum(got.values()) == shots
    assert low == {0: got[0], 3: got[(1 << n) - 1]}
