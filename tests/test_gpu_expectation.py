"""Pauli-string expectation values computed on the device (qsim_expect_paulis, csrc/expect.hip).

The checker is tests/pauli_ref.py (numpy, pinned against dense operators by tests/test_pauli_cpu.py) on the amplitudes READ BACK
from the same state — for an fp32 state `read()` is the exact widened contents — so state rounding cancels and only the
reduction is compared.  Tolerance 1e-10 absolute, the project's parity tolerance: the device adds at most 2^n exactly formed
(fp32) or once-rounded (fp64) products in fp64 by a tree whose error bound is about (n + a few hundred sequential adds) * 2^-53 *
sum|c| <= 1e-13, and any index, sign or pairing mistake shows at 1e-2 or above.
"""
import ctypes
import os

import numpy as np
import pytest

import pauli_ref
from gpu_quantum_simulator_amd import Circuit, Cluster, ShardPlanHandle, Simulator, _lib, circuits, plans
from helpers import random_unitary

pytestmark = pytest.mark.gpu
TOL = 1e-10
TOL32 = 2e-5  # tests/test_gpu_fp32.py derives it: a few hundred gates of fp32 rounding on a unit-norm state
PRECISIONS = [64, 32]


def _rand_state(n, seed):
    rng = np.random.default_rng(seed)
    s = rng.standard_normal(1 << n) + 1j * rng.standard_normal(1 << n)
    return (s / np.linalg.norm(s)).astype(np.complex128)


def _text(x, z, n):
    return pauli_ref.masks_to_text(x, z, n)


def _check_against_readback(sim, n, masks, tol=TOL):
    psi = sim.read()
    got = sim.expectation_terms([_text(x, z, n) for x, z in masks])
    assert got.dtype == np.float64 and got.shape == (len(masks),)
    want = np.array([pauli_ref.pauli_expectation(psi, x, z) for x, z in masks])
    worst = float(np.max(np.abs(got - want))) if len(masks) else 0.0
    print(f"n={n} precision={sim.precision} strings={len(masks)} max abs err {worst:.3e}")
    assert worst < tol, [(m, g, w) for m, g, w in zip(masks, got, want) if abs(g - w) >= tol][:5]
    return got


@pytest.mark.parametrize("precision", PRECISIONS)
def test_every_pauli_on_every_qubit(precision):
    n = 13
    with Simulator(n, precision=precision) as sim:
        sim.write(_rand_state(n, 21))
        masks = [(1 << q if k != 2 else 0, 1 << q if k else 0) for q in range(n) for k in range(3)]  # X, Y, Z
        assert len(set(masks)) == 3 * n
        _check_against_readback(sim, n, masks)


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("n", [1, 2, 5, 6, 7, 13, 18])
def test_random_strings_of_every_weight(n, precision):
    rng = np.random.default_rng(1000 + n)
    masks = [pauli_ref.random_masks(rng, n, 1 + i % n) for i in range(max(200, 12 * n))]
    assert {bin(x | z).count("1") for x, z in masks} == set(range(1, n + 1)) and len(masks) >= 200
    with Simulator(n, precision=precision) as sim:
        sim.write(_rand_state(n, 31 + n))
        _check_against_readback(sim, n, masks)


@pytest.mark.parametrize("precision", PRECISIONS)
def test_large_groups_duplicates_identity_and_order(precision):
    n = 12
    K = plans.pauli_terms_per_sweep()
    rng = np.random.default_rng(7)
    big = 3 * K + 5
    diag = [(0, int(z)) for z in rng.choice(np.arange(1, 1 << n), size=big, replace=False)]
    x0 = 0b100000100101  # lane bits, bit 0 and a high bit
    paired = [(x0, int(z)) for z in rng.choice(1 << n, size=big, replace=False)]
    others = [pauli_ref.random_masks(rng, n, int(rng.integers(1, n + 1))) for _ in range(40)]
    masks = diag + paired + others + [(0, 0)] + diag[:7] + paired[-9:] + [(0, 0)]
    order = rng.permutation(len(masks))
    masks = [masks[i] for i in order]
    assert sum(1 for x, _ in masks if x == 0) > 3 * K and sum(1 for x, _ in masks if x == x0) > 3 * K
    with Simulator(n, precision=precision) as sim:
        sim.write(_rand_state(n, 8) * 1.25)  # norm^2 = 1.5625: the identity must not just return 1
        got = _check_against_readback(sim, n, masks)
        norm2 = sim.norm2()
        ident = [g for g, m in zip(got, masks) if m == (0, 0)]
        assert len(ident) == 2 and all(abs(g - norm2) < 1e-12 for g in ident) and abs(norm2 - 1.5625) < 1e-6


@pytest.mark.parametrize("precision", PRECISIONS)
def test_queued_gates_are_launched_first(precision, golden_dir, oracle):
    path = os.path.join(golden_dir, "live_n13_seed104.qasm")
    n, want, _, _ = oracle.run_qasm(path)
    assert n == 13
    rng = np.random.default_rng(13)
    masks = [pauli_ref.random_masks(rng, n, 1 + i % n) for i in range(60)] + [(0, 1), (1, 0), (1 << 12, 1 << 12)]
    c = Circuit.from_file(path)
    with Simulator(n, precision=precision) as sim:
        sim.run(c)  # queued: nothing has been flushed or waited for
        got = sim.expectation_terms([_text(x, z, n) for x, z in masks])
    ref = np.array([pauli_ref.pauli_expectation(want, x, z) for x, z in masks])
    worst = float(np.max(np.abs(got - ref)))
    print(f"precision={precision} vs the oracle's state: max abs err {worst:.3e}")
    assert np.max(np.abs(ref)) > 1e-3
    assert worst < (TOL if precision == 64 else TOL32)


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("n", [1, 4, 13, 20])
def test_fresh_state(n, precision):
    with Simulator(n, precision=precision) as sim:  # never touched: |0...0> is still held lazily
        got = sim.expectation_terms([f"Z{q}" for q in range(n)] + [f"X{q}" for q in range(n)] + [f"Y{q}" for q in range(n)] + [""])
    assert np.array_equal(got[:n], np.ones(n)) and np.array_equal(got[n:3 * n], np.zeros(2 * n)) and got[-1] == 1.0


@pytest.mark.parametrize("precision", PRECISIONS)
def test_state_unchanged_and_results_reproducible(precision):
    n = 16
    rng = np.random.default_rng(3)
    paulis = [_text(*pauli_ref.random_masks(rng, n, 1 + i % n), n) for i in range(100)]
    with Simulator(n, precision=precision) as sim:
        sim.write(_rand_state(n, 4))
        before = sim.read()
        first = sim.expectation_terms(paulis)
        second = sim.expectation_terms(paulis)
        after = sim.read()
    assert np.array_equal(before.view(np.uint64), after.view(np.uint64))
    assert np.array_equal(first.view(np.uint64), second.view(np.uint64))
    assert np.max(np.abs(first)) > 1e-4


def _product_state_case(n, seed, strings):
    """One random 1-qubit unitary per qubit on |0...0>; <P> = prod_q <0|U_q^+ sigma_q U_q|0> on the host."""
    rng = np.random.default_rng(seed)
    sigma = {"I": np.eye(2), "X": np.array([[0, 1], [1, 0]]), "Y": np.array([[0, -1j], [1j, 0]]), "Z": np.diag([1.0, -1.0])}
    us = [random_unitary(2, rng) for _ in range(n)]
    masks = [pauli_ref.random_masks(rng, n, int(rng.integers(1, 7))) for _ in range(strings)]
    want = []
    for x, z in masks:
        v = 1.0
        for q, letter in enumerate(pauli_ref.masks_to_letters(x, z, n)):
            if letter != "I":
                v *= np.vdot(us[q][:, 0], sigma[letter] @ us[q][:, 0]).real
        want.append(v)
    with Simulator(n) as sim:
        for q in range(n):
            sim.apply_1q(us[q], q)
        got = sim.expectation_terms([_text(x, z, n) for x, z in masks])
        norm2 = sim.norm2()
    worst = float(np.max(np.abs(got - np.array(want))))
    print(f"n={n} product state, {strings} strings: max abs err {worst:.3e}, norm2 - 1 = {norm2 - 1:.3e}")
    assert np.max(np.abs(want)) > 1e-3
    assert worst < TOL
    return n


def test_large_registers_against_product_state():
    import torch
    ran = [_product_state_case(28, 2800, 64)]
    free_b, _total = torch.cuda.mem_get_info()
    room = free_b > (40 << 30)  # the 16 GiB state, a second buffer of that size for out-of-place passes, and slack
    if room:
        ran.append(_product_state_case(30, 3000, 64))
    assert ran == ([28, 30] if room else [28])


def test_expectation_weighted_sum():
    n = 10
    with Simulator(n) as sim:
        sim.write(_rand_state(n, 18))
        paulis = ["Z0 Z1", "X3", "Y2 Z9", "", "Z0 Z1"]
        vals = sim.expectation_terms(paulis)
        assert vals[0] == vals[4]
        real = [0.5, -1.25, 2, np.float64(0.75), 1]
        e = sim.expectation(zip(real, paulis))
        assert type(e) is float and abs(e - float(np.dot(real, vals))) < 1e-12
        cplx = [0.5, -1.25j, 2, 0.75, 1 + 0j]
        e = sim.expectation(list(zip(cplx, paulis)))
        assert type(e) is complex and abs(e - complex(np.dot(np.array(cplx), vals))) < 1e-12
        assert abs(e.imag) > 1e-6 or abs(vals[1]) < 1e-6
        assert sim.expectation([]) == 0.0 and type(sim.expectation([])) is float


@pytest.mark.parametrize("shards", [2, 4, 8])
def test_cluster_matches_single_state(shards):
    n = 14
    c = Circuit.from_gates(n, circuits.random_gates(n, 400, 77 + shards, "all"))
    plan = ShardPlanHandle(c, shards)
    pos = plan.final_pos()
    plan.close()
    assert pos != list(range(n))  # the exchanges left a permuted qubit map behind
    m = n - shards.bit_length() + 1
    rank_qubits = [q for q in range(n) if pos[q] >= m]
    local_qubits = [q for q in range(n) if pos[q] < m]
    assert len(rank_qubits) == shards.bit_length() - 1
    rng = np.random.default_rng(shards)

    def string_on(x_qubits, other_qubits):
        x = z = 0
        for q in x_qubits:
            x |= 1 << q
            z |= int(rng.integers(2)) << q  # X or Y
        for q in other_qubits:
            if q not in x_qubits and rng.integers(2):
                z |= 1 << q
        return x, z

    masks = []
    for i in range(50):  # x on rank qubits only
        xq = [q for q in rank_qubits if rng.integers(2)] or [rank_qubits[i % len(rank_qubits)]]
        masks.append(string_on(xq, range(n)))
    for i in range(50):  # x on local qubits only
        xq = list(rng.choice(local_qubits, size=1 + i % 5, replace=False))
        masks.append(string_on([int(q) for q in xq], range(n)))
    for i in range(50):  # both
        xq = [rank_qubits[i % len(rank_qubits)]] + [int(q) for q in rng.choice(local_qubits, size=1 + i % 4, replace=False)]
        masks.append(string_on(xq, range(n)))
    masks += [pauli_ref.random_masks(rng, n, 1 + i % n) for i in range(50)]
    assert len(masks) == 200
    rank_mask = sum(1 << q for q in rank_qubits)
    assert any(x and not x & ~rank_mask for x, _ in masks) and any(x and not x & rank_mask for x, _ in masks)
    assert any(x & rank_mask and x & ~rank_mask for x, _ in masks)
    paulis = [_text(x, z, n) for x, z in masks]
    with Simulator(n) as sim:
        sim.run(c)
        single = sim.expectation_terms(paulis)
    with Cluster(n, shards, devices=[0] * shards) as cl:
        cl.run(c)
        got = cl.expectation_terms(paulis)
        psi = cl.read()
        e = cl.expectation([(0.5, paulis[0]), (2.0, paulis[60])])
        assert type(e) is float and abs(e - (0.5 * got[0] + 2.0 * got[60])) < 1e-12
    want = np.array([pauli_ref.pauli_expectation(psi, x, z) for x, z in masks])
    print(f"P={shards}: vs single {np.max(np.abs(got - single)):.3e}, vs checker on cluster.read() {np.max(np.abs(got - want)):.3e}")
    assert np.max(np.abs(want)) > 1e-3
    assert np.max(np.abs(got - single)) < TOL
    assert np.max(np.abs(got - want)) < TOL


def test_cluster_fresh_state():
    n = 8
    with Cluster(n, 4, devices=[0] * 4) as cl:
        cl._check(_lib.load().qsim_cluster_reset(cl._h))  # three shards hold nothing, one holds |0...0>, none of it written yet
        got = cl.expectation_terms([f"Z{q}" for q in range(n)] + [f"X{q}" for q in range(n)] + [""])
    assert np.array_equal(got, np.array([1.0] * n + [0.0] * n + [1.0]))


@pytest.mark.parametrize("precision", PRECISIONS)
def test_errors(precision):
    lib = _lib.load()
    up = ctypes.POINTER(ctypes.c_uint64)
    n = 5
    with Simulator(n, precision=precision) as sim:
        out = np.full(2, 7.0)
        dp = out.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
        ok = np.array([1, 2], dtype=np.uint64)
        for bad_x, bad_z in (([1, 1 << n], [0, 0]), ([1, 2], [0, 1 << 63])):  # a mask bit at or above n
            bx, bz = np.array(bad_x, dtype=np.uint64), np.array(bad_z, dtype=np.uint64)
            with pytest.raises(_lib.QsimError, match="outside"):
                _lib.check(lib.qsim_expect_paulis(sim._h, bx.ctypes.data_as(up), bz.ctypes.data_as(up), 2, dp))
        for args in ((None, ok.ctypes.data_as(up), 2, dp), (ok.ctypes.data_as(up), None, 2, dp), (ok.ctypes.data_as(up), ok.ctypes.data_as(up), 2, None)):
            with pytest.raises(_lib.QsimError, match="NULL"):
                _lib.check(lib.qsim_expect_paulis(sim._h, *args))
        with pytest.raises(_lib.QsimError, match="negative"):
            _lib.check(lib.qsim_expect_paulis(sim._h, ok.ctypes.data_as(up), ok.ctypes.data_as(up), -1, dp))
        assert np.array_equal(out, [7.0, 7.0])
        _lib.check(lib.qsim_expect_paulis(sim._h, None, None, 0, None))  # zero terms: fine, writes nothing
        empty = sim.expectation_terms([])
        assert empty.shape == (0,) and empty.dtype == np.float64
        with pytest.raises(ValueError):
            sim.expectation_terms([f"X{n}"])
    if precision == 64:
        with Cluster(n, 2, devices=[0, 0]) as cl:
            bx = np.array([1 << n], dtype=np.uint64)
            with pytest.raises(_lib.QsimError, match="outside"):
                cl._check(lib.qsim_cluster_expect_paulis(cl._h, bx.ctypes.data_as(up), bx.ctypes.data_as(up), 1, dp))
            with pytest.raises(_lib.QsimError, match="negative"):
                cl._check(lib.qsim_cluster_expect_paulis(cl._h, bx.ctypes.data_as(up), bx.ctypes.data_as(up), -2, dp))
            assert cl.expectation_terms([]).shape == (0,)
