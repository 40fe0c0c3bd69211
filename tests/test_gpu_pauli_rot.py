"""Pauli-string rotations exp(-i theta/2 P) applied on the device (qsim_apply_pauli_rotations, csrc/evolve.hip).

The checker is tests/pauli_rot_ref.py (numpy, pinned against dense operators by tests/test_pauli_rot_cpu.py) applied to the
amplitudes READ BACK before the call — for an fp32 state `read()` is the exact widened contents, so state rounding cancels.
fp64: 1e-10 max abs, the project's parity tolerance (a run rounds a few times per term and amplitude: 200 terms stay below
1e-13, any index, sign or pairing mistake shows at 1e-2).  fp32: fp32_ref.check_fp32(got, want64, ref32) with ref32 the
complex64 replay of the same terms; C = 8 carries over, one term of a run rounds about as often per amplitude as one term of the
replay.  Where two fp32 results are compared with each other, each is within C * max(rel_err(ref32), FLOOR) of the truth, so
they are within twice that of each other (triangle inequality).

Convention found in the gate table: rz(theta) = diag(1, e^(i theta)) (read through gate_matrix), so the rotation
exp(-i theta/2 Z_q) = diag(e^(-i theta/2), e^(i theta/2)) is e^(-i theta/2) times it: the table drops the global phase.
"""
import cmath
import ctypes
import functools
import math
import os

import numpy as np
import pytest

import fp32_ref
import pauli_ref
import pauli_rot_ref as ref
from fp32_ref import check_fp32, report
from gpu_quantum_simulator_amd import Circuit, Cluster, ShardPlanHandle, Simulator, _lib, circuits, gate_matrix, pauli_masks, trotter_rotations, plans

pytestmark = pytest.mark.gpu
TOL = 1e-10
TOL32 = 2e-5  # tests/test_gpu_fp32.py derives it for a few hundred fp32 roundings per amplitude
PRECISIONS = [64, 32]
UP = ctypes.POINTER(ctypes.c_uint64)
DP = ctypes.POINTER(ctypes.c_double)


def _check(precision, got, before, rotations, label):
    """`got` against the checker's replay of `rotations` from `before` (a state as read back)."""
    want = ref.replay(before, rotations)
    if precision == 64:
        worst = float(np.max(np.abs(got - want)))
        print(f"{label}: fp64 max abs err {worst:.3e} over {len(rotations)} rotations")
        assert worst < TOL
    else:
        report(label, check_fp32(got, want, ref.replay(before.astype(np.complex64), rotations, np.complex64)))
    return want


def _close(precision, a, b, want, ref32):
    if precision == 64:
        assert np.max(np.abs(a - b)) < TOL
    else:
        assert fp32_ref.rel_err(a, b) <= 2 * fp32_ref.C * max(fp32_ref.rel_err(ref32, want), fp32_ref.FLOOR)


def _plan(rotations):
    p = plans.ok(plans.pauli_rotation_plan([x for _, x, _ in rotations], [z for _, _, z in rotations]))
    return p["sweeps"], p["queued_as_gates"]


@pytest.mark.parametrize("precision", PRECISIONS)
def test_single_bit_x_at_every_position(precision):
    n = 13
    rotations = ref.single_bit_rotations(n)
    assert {x for _, x, _ in rotations} == {0} | {1 << q for q in range(n)}
    with Simulator(n, precision=precision) as sim:
        sim.write(ref.rand_state(n, 13))
        before = sim.read()
        for i, rot in enumerate(rotations):
            sim.apply_pauli_rotation(*ref.texts([rot], n)[0])
            got = sim.read()
            _check(precision, got, before, [rot], f"single-bit {ref.texts([rot], n)[0][1]} p{precision}")
            before = got


@functools.lru_cache(maxsize=None)
def _every_weight_truth(n, precision):
    start = ref.rand_state(n, 40 + n)
    if precision == 32:
        start = start.astype(np.complex64).astype(np.complex128)
    rotations = ref.every_weight_rotations(n)
    return start, rotations, ref.replay(start, rotations), ref.replay(start.astype(np.complex64), rotations, np.complex64)


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("n", ref.EVERY_WEIGHT_SIZES)
def test_every_weight_one_call_each_and_fused(n, precision):
    start, rotations, want, ref32 = _every_weight_truth(n, precision)
    texts = ref.texts(rotations, n)
    with Simulator(n, precision=precision) as one_each, Simulator(n, precision=precision) as fused:
        one_each.write(start)
        fused.write(start)
        assert np.array_equal(one_each.read(), start)  # the rounded start state is what the device holds
        for theta, text in texts:
            one_each.apply_pauli_rotation(theta, text)
        fused.apply_pauli_rotations(texts)
        a, b = one_each.read(), fused.read()
    for label, got in (("one call each", a), ("one call", b)):
        if precision == 64:
            worst = float(np.max(np.abs(got - want)))
            print(f"n={n} {label}: fp64 max abs err {worst:.3e}")
            assert worst < TOL
        else:
            report(f"every weight n={n} {label}", check_fp32(got, want, ref32))
    _close(precision, a, b, want, ref32)


@pytest.mark.parametrize("precision", PRECISIONS)
def test_runs_longer_than_k(precision):
    n = 12
    K = plans.pauli_rotations_per_sweep()
    diag, paired = ref.long_run_rotations(K)
    assert len(diag) == len(paired) == 3 * K + 5 and (0.9, 0, 0) in diag
    thetas = {t for t, _, _ in diag + paired}
    assert {0.0, math.pi, 2 * math.pi} <= thetas and min(thetas) < 0
    with Simulator(n, precision=precision) as sim:
        sim.write(ref.rand_state(n, 12))
        for label, run in (("diagonal", diag), ("paired", paired), ("both", diag + paired)):
            before = sim.read()
            count = plans.sweeps_launched("pauli_rotation")
            sim.apply_pauli_rotations(ref.texts(run, n))
            taken = plans.sweeps_launched("pauli_rotation") - count
            assert (taken, 0) == _plan(run) and taken == -(-len(diag) // K) * (len(run) // len(diag)), (label, taken)
            _check(precision, sim.read(), before, run, f"run of {len(run)} {label} p{precision}")


@pytest.mark.parametrize("precision", PRECISIONS)
def test_order_matters(precision):
    n = 6
    a, b = ref.ORDER_PAIR
    assert ref.texts([a, b], n) == [(0.8, "X0 X1"), (1.3, "Y0 X1")]
    results = []
    for order in ([a, b], [b, a]):
        with Simulator(n, precision=precision) as sim:
            sim.write(ref.rand_state(n, 6))
            before = sim.read()
            count = plans.sweeps_launched("pauli_rotation")
            sim.apply_pauli_rotations(ref.texts(order, n))
            assert plans.sweeps_launched("pauli_rotation") - count == 1  # one x: one sweep, the order kept inside it
            results.append(sim.read())
            _check(precision, results[-1], before, order, f"order p{precision}")
    assert np.max(np.abs(results[0] - results[1])) > 1e-2


@pytest.mark.parametrize("precision", PRECISIONS)
def test_z_rotation_is_the_gate_table_rz_up_to_its_phase(precision):
    n, q, theta = ref.RZ_CASE
    U = gate_matrix(f"rz({theta!r})")
    rot = np.array([cmath.exp(-0.5j * theta), cmath.exp(0.5j * theta)])
    phase = rot[0] / U[0, 0]
    assert abs(U[0, 1]) == abs(U[1, 0]) == 0 and np.max(np.abs(np.diag(U) * phase - rot)) < 1e-15 and abs(phase - cmath.exp(-0.5j * theta)) < 1e-15
    with Simulator(n, precision=precision) as a, Simulator(n, precision=precision) as b:
        for sim in (a, b):
            sim.write(ref.rand_state(n, 9))
        before = a.read()
        a.apply_pauli_rotation(theta, f"Z{q}")
        b.apply_1q(U, q)
        got, gate = a.read(), b.read() * phase
    want = _check(precision, got, before, [(theta, 0, 1 << q)], f"rz convention p{precision}")
    if precision == 64:
        assert np.max(np.abs(got - gate)) < TOL
    else:
        check_fp32(gate, want, ref.replay(before.astype(np.complex64), [(theta, 0, 1 << q)], np.complex64))


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("n", ref.FRESH_SIZES)
def test_fresh_state(n, precision):
    theta, x, z = ref.fresh_rotation(n)
    c, s = math.cos(0.5 * theta), math.sin(0.5 * theta)
    eps = 1e-15 if precision == 64 else 2.0 ** -24
    with Simulator(n, precision=precision) as sim:  # never touched: |0...0> is still held lazily
        sim.apply_pauli_rotation(theta, pauli_ref.masks_to_text(x, z, n))
        got = sim.read()
        assert sim.get_support()[0] == (1 << n) - 1
    other = 1 if n == 1 else 1 | 1 << (n - 1)
    want_other = s if n == 1 else -1j * s  # exp(-i theta/2 Y)|0> = c|0> + s|1>;  exp(-i theta/2 XX)|00> = c|00> - i s|11>
    assert list(np.flatnonzero(got)) == [0, other]
    assert abs(got[0] - c) <= eps and abs(got[other] - want_other) <= eps


@pytest.mark.parametrize("precision", PRECISIONS)
def test_partial_state_then_rotations_then_gates(precision):
    n = 18
    spec = fp32_ref.FEW_CIRCUIT
    gates = fp32_ref.gate_list(*spec)
    tail = Circuit.from_gates(n, ref.AFTER_FEW_GATES)
    tail_gates = [tail.gate(i) for i in range(len(tail))]
    few = Circuit.from_gates(n, circuits.random_gates(*spec))
    with Simulator(n, precision=precision) as probe, Simulator(n, precision=precision) as sim:
        probe.run(few)
        before = probe.read()  # the read writes the zeros out: the state the rotations must see is read from a twin
        assert not before[128:].any()
        sim.run(few)
        assert sim.get_support()[0] != (1 << n) - 1  # partial: most of the buffer has never been written
        sim.apply_pauli_rotations(ref.texts(ref.AFTER_FEW, n))
        assert sim.get_support()[0] == (1 << n) - 1  # dense after the sweep
        sim.run(tail)
        got = sim.read()
    want = fp32_ref.replay(n, tail_gates, ref.replay(before, ref.AFTER_FEW), np.complex128)
    if precision == 64:
        truth = fp32_ref.replay(n, gates, dtype=np.complex128)
        assert np.max(np.abs(before - truth)) < TOL
        worst = float(np.max(np.abs(got - want)))
        print(f"partial then rotations then gates: fp64 max abs err {worst:.3e}")
        assert worst < TOL
        assert np.count_nonzero(np.abs(got[1 << 17:]) > 1e-6) > 10  # the rotations reached the untouched qubits
    else:
        ref32 = fp32_ref.replay(n, tail_gates, ref.replay(before.astype(np.complex64), ref.AFTER_FEW, np.complex64), np.complex64)
        report("partial then rotations then gates", check_fp32(got, want, ref32))


@pytest.mark.parametrize("precision", PRECISIONS)
def test_queued_gates_go_first_and_the_call_does_not_wait(precision, golden_dir, oracle):
    path = os.path.join(golden_dir, "live_n13_seed104.qasm")
    n, truth, _, _ = oracle.run_qasm(path)
    assert n == 13
    rotations = ref.queued_rotations(n)
    singles = sum(1 for _, x, z in rotations if bin(x).count("1") == 1 and not z & ~x)
    assert _plan(rotations)[1] == singles >= 2  # single X / Y terms travel through the gate queue
    c = Circuit.from_file(path)
    with Simulator(n, precision=precision) as sim:
        sim.run(c)  # queued: nothing has been flushed or waited for
        sim.apply_pauli_rotations(ref.texts(rotations, n))
        got = sim.read()
    want = ref.replay(truth, rotations)
    if precision == 64:
        worst = float(np.max(np.abs(got - want)))
        print(f"circuit then rotations vs the oracle's state: max abs err {worst:.3e}")
        assert worst < TOL
    else:
        c2 = Circuit.from_file(path)
        ref32 = ref.replay(fp32_ref.replay(n, [c2.gate(i) for i in range(len(c2))]), rotations, np.complex64)
        report("circuit then rotations", check_fp32(got, want, ref32))


@pytest.mark.parametrize("precision", PRECISIONS)
def test_reproducible(precision):
    n = 16
    texts = ref.texts(ref.reproducible_rotations(n), n)
    out = []
    for _ in range(2):
        with Simulator(n, precision=precision) as sim:
            sim.write(ref.rand_state(n, 160))
            before = sim.read()
            sim.apply_pauli_rotations(texts)
            sim.apply_pauli_rotations(texts[::-1])
            out.append(sim.read())
    assert np.array_equal(out[0].view(np.uint64), out[1].view(np.uint64))
    _check(precision, out[0], before, ref.reproducible_rotations(n) + ref.reproducible_rotations(n)[::-1], f"reproducible p{precision}")


@pytest.mark.parametrize("precision", PRECISIONS)
def test_grid_cap_changes_no_bit(precision):
    """QSIM_OPT_GRID_CAP caps a sweep's grid (0: the resident grid).  Which workgroup takes a block of units changes no amplitude's
    arithmetic: 3 workgroups walking many trips each, and one workgroup per block, give the bits of the default."""
    n = 16
    texts = ref.texts(ref.reproducible_rotations(n), n)
    out = []
    for cap in (0, 3, 1 << 30):
        with Simulator(n, precision=precision, grid_cap=cap) as sim:
            sim.write(ref.rand_state(n, 160))
            sim.apply_pauli_rotations(texts)
            out.append(sim.read().view(np.uint64).copy())
    assert np.array_equal(out[0], out[1]) and np.array_equal(out[0], out[2])


@pytest.mark.parametrize("precision", PRECISIONS)
def test_evolve_diagonal_hamiltonian_is_exact(precision):
    n, t = 10, 0.8
    terms = ref.diagonal_hamiltonian(n, 30)
    j = np.arange(1 << n, dtype=np.uint64)
    energy = sum(c * (1.0 - 2.0 * pauli_ref._parity(j & np.uint64(pauli_masks(text, n)[1]))) for c, text in terms)
    with Simulator(n, precision=precision) as sim:
        sim.write(ref.rand_state(n, 10))
        before = sim.read()
        count = plans.sweeps_launched("pauli_rotation")
        sim.evolve(terms, t, steps=1)
        assert plans.sweeps_launched("pauli_rotation") - count == 1  # 30 all-Z terms: one sweep
        got = sim.read()
    exact = np.exp(-1j * energy * t) * before
    rotations = ref.masks_of(trotter_rotations(terms, t), n)
    if precision == 64:
        worst = float(np.max(np.abs(got - exact)))
        print(f"diagonal H, 30 terms: max abs err vs exp(-iHt) {worst:.3e}")
        assert worst < TOL
    else:
        report("diagonal H vs exp(-iHt)", check_fp32(got, exact, ref.replay(before.astype(np.complex64), rotations, np.complex64)))


@pytest.mark.parametrize("precision", PRECISIONS)
def test_evolve_ising(precision):
    """Orders 1 and 2 against the checker's replay of the same product formula, and the energy drift of an order-2 run.

    The drift bound.  H = A + B with A the ZZ layer (||A|| <= 7) and B the X layer (||B|| <= 5.6); the terms of a layer commute,
    so the order-2 list is exactly the Strang splitting e^(-iA dt/2) e^(-iB dt) e^(-iA dt/2) = exp(-i dt (H + dt^2 E + ...)) with
    ||E|| <= ||[B,[B,A]]|| / 12 + ||[A,[A,B]]|| / 24 <= (4 * 7 * 5.6^2) / 12 + (4 * 7^2 * 5.6) / 24 = 119.  The effective
    Hamiltonian is conserved, so |<H>(t) - <H>(0)| <= 2 dt^2 ||E||: at dt = 0.4 / 20 that is 0.095, below the 1e-2 * sum|c_k| =
    0.126 asserted (fp32 adds the state's rounding, some 1e-5)."""
    n = 8
    terms = ref.ising_terms(n)
    weight = sum(abs(c) for c, _ in terms)
    assert abs(weight - 12.6) < 1e-12
    with Simulator(n, precision=precision) as sim:
        for order in (1, 2):
            sim.write(ref.rand_state(n, 8))
            before = sim.read()
            sim.evolve(terms, 0.9, steps=3, order=order)
            _check(precision, sim.read(), before, ref.masks_of(trotter_rotations(terms, 0.9, 3, order), n), f"ising order {order} p{precision}")
        sim.write(ref.rand_state(n, 8))
        e0 = sim.expectation(terms)
        sim.evolve(terms, ref.DRIFT_TIME, steps=ref.DRIFT_STEPS, order=2)
        e1 = sim.expectation(terms)
    print(f"ising n={n} p{precision}: <H> {e0:.6f} -> {e1:.6f}, drift {abs(e1 - e0):.3e} ({abs(e1 - e0) / weight:.3e} of sum|c|)")
    assert abs(e1 - e0) < 1e-2 * weight


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
    rng = np.random.default_rng(100 + shards)

    def string_on(x_qubits):
        x = z = 0
        for q in x_qubits:
            x |= 1 << q
            z |= int(rng.integers(2)) << q  # X or Y
        for q in range(n):
            if q not in x_qubits and rng.integers(2):
                z |= 1 << q  # Z anywhere
        return float(rng.uniform(-math.pi, math.pi)), x, z

    rotations = []
    for i in range(50):  # x on shard-id qubits only
        rotations.append(string_on([q for q in rank_qubits if rng.integers(2)] or [rank_qubits[i % len(rank_qubits)]]))
    for i in range(50):  # x on local qubits only
        rotations.append(string_on([int(q) for q in rng.choice(local_qubits, size=1 + i % 5, replace=False)]))
    for i in range(50):  # both
        rotations.append(string_on([rank_qubits[i % len(rank_qubits)]] + [int(q) for q in rng.choice(local_qubits, size=1 + i % 4, replace=False)]))
    rotations += [(float(rng.uniform(-2, 2)),) + pauli_ref.random_masks(rng, n, 1 + i % n) for i in range(50)]
    rotations += [(0.4, 1 << local_qubits[0], 0), (0.7, 1 << rank_qubits[0], 1 << rank_qubits[0]), (0.2, 0, 0), (0.3, 0, 1 << rank_qubits[-1])]
    rank_mask = sum(1 << q for q in rank_qubits)
    assert any(x and not x & ~rank_mask for _, x, _ in rotations) and any(x and not x & rank_mask for _, x, _ in rotations)
    assert any(x & rank_mask and x & ~rank_mask for _, x, _ in rotations)
    order = rng.permutation(len(rotations))
    rotations = [rotations[i] for i in order]
    texts = ref.texts(rotations, n)
    with Simulator(n) as sim:
        sim.run(c)
        circuit_state = sim.read()
        sim.apply_pauli_rotations(texts)
        single = sim.read()
    with Cluster(n, shards, devices=[0] * shards) as cl:
        cl.run(c)
        before = cl.read()
        cl.apply_pauli_rotations(texts[:100])
        for theta, text in texts[100:110]:
            cl.apply_pauli_rotation(theta, text)
        cl.apply_pauli_rotations(texts[110:])
        got = cl.read()
        assert abs(cl.norm2() - 1.0) < 1e-10
        cl.run(c)  # resets, and works as before
        again = cl.read()
        # straight after rotations on a reset cluster a circuit is still refused: the state is no longer |0...0>
        lib = _lib.load()
        cl._check(lib.qsim_cluster_reset(cl._h))
        cl.apply_pauli_rotation(0.5, f"X{n - 1} Z0")
        fresh_then_rotated = cl.read()
        assert lib.qsim_cluster_run_circuit(cl._h, c._h) == _lib.ERR_ARG
        assert b"reset" in lib.qsim_cluster_error()
        cl.evolve([(0.5, "Z0 Z1"), (-0.3, f"X{n - 1}")], 0.4, steps=2, order=2)
        evolved = cl.read()
    want = ref.replay(before, rotations)
    print(f"P={shards}: vs single {np.max(np.abs(got - single)):.3e}, vs checker on cluster.read() {np.max(np.abs(got - want)):.3e}")
    assert np.max(np.abs(before - circuit_state)) < TOL
    assert np.max(np.abs(got - single)) < TOL and np.max(np.abs(got - want)) < TOL
    assert np.max(np.abs(got - before)) > 1e-3
    assert np.max(np.abs(again - circuit_state)) < TOL
    # identity qubit map after the reset: qubit n - 1 selects the shard, and all but one shard held nothing
    ket0 = np.zeros(1 << n, dtype=np.complex128)
    ket0[0] = 1
    one = [(0.5,) + pauli_masks(f"X{n - 1} Z0", n)]
    assert np.max(np.abs(fresh_then_rotated - ref.replay(ket0, one))) < TOL
    rest = ref.masks_of(trotter_rotations([(0.5, "Z0 Z1"), (-0.3, f"X{n - 1}")], 0.4, 2, 2), n)
    assert np.max(np.abs(evolved - ref.replay(ket0, one + rest))) < TOL


def _bits(sim_or_cluster):
    return sim_or_cluster.read().view(np.uint64).copy()


@pytest.mark.parametrize("precision", PRECISIONS)
def test_errors(precision):
    """Every QSIM_ERR_ARG case of the state's call and the cluster's, with the state bit-identical afterwards.  One case is NOT
    here: a term with X or Y on a shard-id qubit while the shards sit on different devices.  It needs two devices, and this
    suite's GPU tests run on one; the refusal is the same test of `same_device`, with the same wording, as in
    qsim_cluster_expect_paulis."""
    lib = _lib.load()
    n = 5
    ok = np.array([1, 2], dtype=np.uint64)
    okp = ok.ctypes.data_as(UP)
    th = np.array([0.3, 0.4])
    thp = th.ctypes.data_as(DP)
    assert lib.qsim_apply_pauli_rotations(None, okp, okp, thp, 2) == _lib.ERR_ARG and b"NULL" in lib.qsim_last_error()
    with Simulator(n, precision=precision) as sim:
        sim.write(ref.rand_state(n, 5))
        before = _bits(sim)
        for bad_x, bad_z in (([1, 1 << n], [0, 0]), ([1, 2], [0, 1 << 63])):  # a mask bit at or above n
            bx, bz = np.array(bad_x, dtype=np.uint64), np.array(bad_z, dtype=np.uint64)
            with pytest.raises(_lib.QsimError, match="outside"):
                _lib.check(lib.qsim_apply_pauli_rotations(sim._h, bx.ctypes.data_as(UP), bz.ctypes.data_as(UP), thp, 2))
        for args in ((None, okp, thp, 2), (okp, None, thp, 2), (okp, okp, None, 2)):
            with pytest.raises(_lib.QsimError, match="NULL"):
                _lib.check(lib.qsim_apply_pauli_rotations(sim._h, *args))
        with pytest.raises(_lib.QsimError, match="negative"):
            _lib.check(lib.qsim_apply_pauli_rotations(sim._h, okp, okp, thp, -1))
        for bad in (float("nan"), float("inf"), -float("inf")):
            bt = np.array([0.3, bad])
            with pytest.raises(_lib.QsimError, match="non-finite"):
                _lib.check(lib.qsim_apply_pauli_rotations(sim._h, okp, okp, bt.ctypes.data_as(DP), 2))
        assert np.array_equal(_bits(sim), before)  # the valid first term of a refused call was not applied either
        _lib.check(lib.qsim_apply_pauli_rotations(sim._h, None, None, None, 0))  # zero terms: fine, does nothing
        sim.apply_pauli_rotations([])
        sim.evolve([], 1.0)
        assert np.array_equal(_bits(sim), before)
        with pytest.raises(ValueError):
            sim.apply_pauli_rotation(0.1, f"X{n}")
        with pytest.raises(ValueError):
            sim.evolve([(1j, "Z0")], 1.0)
        with pytest.raises(ValueError):
            sim.evolve([(1.0, "Z0")], 1.0, order=3)
        assert np.array_equal(_bits(sim), before)
        sim.reset(holds_index0=False)  # a shard that holds nothing stays untouched
        count = plans.sweeps_launched("pauli_rotation")
        sim.apply_pauli_rotations([(0.3, "Z0 Z1"), (0.2, "X0 X1")])
        assert plans.sweeps_launched("pauli_rotation") == count and sim.get_support()[1:] == (1, 0.0)
    if precision == 64:
        with Cluster(n, 2, devices=[0, 0]) as cl:
            assert lib.qsim_cluster_apply_pauli_rotations(None, okp, okp, thp, 2) == _lib.ERR_ARG
            cl.run(Circuit.from_gates(n, circuits.random_gates(n, 60, 5, "all")))
            before = _bits(cl)
            for bad_x, bad_z in (([1, 1 << n], [1, 2]), ([1, 2], [0, 1 << 63])):  # a mask bit at or above n, in x and in z
                bx, bz = np.array(bad_x, dtype=np.uint64), np.array(bad_z, dtype=np.uint64)
                with pytest.raises(_lib.QsimError, match="outside"):
                    cl._check(lib.qsim_cluster_apply_pauli_rotations(cl._h, bx.ctypes.data_as(UP), bz.ctypes.data_as(UP), thp, 2))
            with pytest.raises(_lib.QsimError, match="negative"):
                cl._check(lib.qsim_cluster_apply_pauli_rotations(cl._h, okp, okp, thp, -2))
            for args in ((None, okp, thp, 2), (okp, None, thp, 2), (okp, okp, None, 2)):
                with pytest.raises(_lib.QsimError, match="NULL"):
                    cl._check(lib.qsim_cluster_apply_pauli_rotations(cl._h, *args))
            bt = np.array([0.3, float("nan")])
            with pytest.raises(_lib.QsimError, match="non-finite"):
                cl._check(lib.qsim_cluster_apply_pauli_rotations(cl._h, okp, okp, bt.ctypes.data_as(DP), 2))
            cl._check(lib.qsim_cluster_apply_pauli_rotations(cl._h, None, None, None, 0))
            cl.apply_pauli_rotations([])
            assert np.array_equal(_bits(cl), before)


GEOMETRY_THETA = 0.7


def _geometry_strings(n):
    """(x, z) with the highest x bit at 0, at 1, on either side of the unit / thread boundary of the sweeps (7 and 8) and at n - 1,
    as far as the register has these bits, and one diagonal string."""
    out = []
    for h in sorted({0, 1, 7, 8, n - 1} & set(range(n))):
        x = 1 << h | (1 << (h - 2) if h >= 2 else 0)        # a second X two bits below, where there is room
        z = (1 << h if h % 2 else 0) | 1 << (h + 1) % n     # Y at an odd h, and a Z next to it (n = 1: Y0)
        out.append((x, z))
    return out + [(0, 0b101101101 & ((1 << n) - 1))]


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("n", [1, 2, 9])
def test_expectation_of_p_survives_its_own_rotation(n, precision):
    """exp(-i theta/2 P) commutes with P, so <P> read by k_expect before and after k_pauli_rot applied the rotation is one number:
    the two kernels walk the state by one geometry (csrc/pauli_sweep.h), and a string that one of them paired or signed differently
    from the other would move it.  fp64: TOL.  fp32: the rotation rounds every amplitude a few times, once per fused multiply-add;
    TOL32 is the bound for a few hundred such roundings."""
    largest = 0.0
    with Simulator(n, precision=precision) as sim:
        for x, z in _geometry_strings(n):
            text = pauli_ref.masks_to_text(x, z, n)
            sim.write(ref.rand_state(n, 70 + n))
            before = float(sim.expectation_terms([text])[0])
            sim.apply_pauli_rotation(GEOMETRY_THETA, text)
            after = float(sim.expectation_terms([text])[0])
            print(f"n={n} p{precision} {text}: <P> {before:+.6e} -> {after:+.6e}, moved by {abs(after - before):.3e}")
            assert abs(after - before) < (TOL if precision == 64 else TOL32)
            largest = max(largest, abs(before))
    assert largest > 1e-3  # not a comparison of zeros
