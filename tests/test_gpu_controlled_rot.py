"""Controlled Pauli rotations (1 - Pi) + Pi exp(-i theta/2 P) on the device (qsim_apply_controlled_pauli_rotations, csrc/crot.hip).

The checker is tests/controlled_rot_ref.py (pauli_rot_ref's pair formula kept where every control bit is 1; pinned against dense
operators by tests/test_controlled_rot_cpu.py) applied to the amplitudes READ BACK before the call.  Tolerances are those of
tests/test_gpu_pauli_rot.py: fp64 1e-10 max abs; fp32 fp32_ref.check_fp32(got, want64, ref32) with ref32 the complex64 replay of
the same terms — a controlled term rounds the amplitudes it touches as often as the uncontrolled one and the others not at all.
"""
import ctypes
import math
import os

import numpy as np
import pytest

import controlled_rot_ref as ref
import fp32_ref
import pauli_rot_ref
from fp32_ref import check_fp32, report
from gpu_quantum_simulator_amd import Circuit, Cluster, Simulator, _lib, circuits, plans

pytestmark = pytest.mark.gpu
TOL = 1e-10
PRECISIONS = [64, 32]
UP = ctypes.POINTER(ctypes.c_uint64)
DP = ctypes.POINTER(ctypes.c_double)


def _check(precision, got, before, rotations, label, quiet=False):
    """`got` against the checker's replay of `rotations` from `before` (a state as read back)."""
    want = ref.replay(before, rotations)
    if precision == 64:
        worst = float(np.max(np.abs(got - want)))
        if not quiet:
            print(f"{label}: fp64 max abs err {worst:.3e} over {len(rotations)} rotations")
        assert worst < TOL, (label, worst)
    else:
        errs = check_fp32(got, want, ref.replay(before.astype(np.complex64), rotations, np.complex64))
        if not quiet:
            report(label, errs)
    return want


def _bits(sim):
    """The state's bits, one row (re, im) per amplitude."""
    return sim.read().view(np.uint64).reshape(-1, 2).copy()


def _one_by_one(precision, n, start, rotations, label):
    """Every term as a call of its own on one state, each checked against the replay from the state read before it."""
    worst_moved = 0.0
    with Simulator(n, precision=precision) as sim:
        sim.write(start)
        before = sim.read()
        for i, rot in enumerate(rotations):
            theta, text, controls = ref.entries([rot], n)[0]
            sim.apply_pauli_rotation(theta, text, controls)
            got = sim.read()
            _check(precision, got, before, [rot], f"{label} #{i} {text or 'I'} | {controls} p{precision}", quiet=True)
            worst_moved = max(worst_moved, float(np.max(np.abs(got - before))))
            before = got
    print(f"{label} p{precision}: {len(rotations)} terms, each within tolerance of the replay")
    assert worst_moved > 1e-3  # not a comparison of untouched states


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("n", ref.EXHAUSTIVE_SIZES)
def test_exhaustive_small_registers(n, precision):
    terms = ref.exhaustive_terms(n)
    assert len(terms) == {1: 1, 2: 9, 3: 61, 4: 369}[n]
    _one_by_one(precision, n, ref.rand_state(n, 50 + n), terms, f"exhaustive n={n}")


@pytest.mark.parametrize("precision", PRECISIONS)
def test_one_control_at_every_position(precision):
    n = 13
    terms = ref.every_position_terms(n)
    assert {c for _, c, _, _ in terms} == {1 << q for q in range(n)}
    for q in range(n):
        mine = [(x, z) for _, c, x, z in terms if c == 1 << q]
        assert any(x == 0 and z for x, z in mine)
        assert q == 0 or any(x and x < 1 << q for x, _ in mine)
        assert q == n - 1 or any(x > 1 << q for x, _ in mine)
    assert ref.plan(terms, n, precision)[:2] == (len(terms), 0)
    _one_by_one(precision, n, ref.rand_state(n, 131), terms, "every position")


@pytest.mark.parametrize("precision", PRECISIONS)
def test_fp32_slot_cases(precision):
    """A control on qubit 0 leaves one slot of an fp32 unit active; x = 1 keeps a pair inside one unit.  fp64 runs the same terms."""
    n = ref.SLOT_N
    assert {(c & 1, x) for _, c, x, _ in ref.SLOT_TERMS} >= {(1, 0b10), (1, 0b110), (1, 0), (0, 1)}
    assert ref.plan(ref.SLOT_TERMS, n, precision)[1] == 0
    _one_by_one(precision, n, ref.rand_state(n, 10), ref.SLOT_TERMS, "slots")


@pytest.mark.parametrize("precision", PRECISIONS)
def test_several_controls(precision):
    n = ref.SEVERAL_N
    terms = ref.several_controls_terms(n)
    sizes = {bin(c).count("1") for _, c, _, _ in terms}
    assert sizes >= set(range(2, n + 1))
    assert any(c == (1 << n) - 1 for _, c, _, _ in terms) and any(c & 0b110000000 == 0b110000000 for _, c, _, _ in terms)
    _one_by_one(precision, n, ref.rand_state(n, 1300), terms, "several controls")


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("c", ref.BITEXACT_CONTROLS)
def test_bit_exact_relation_to_the_uncontrolled_sweep(c, precision):
    """Inside the control subspace k_pauli_crot runs rotate_pair / rotate_diag with the c and v k_pauli_rot gets, on the same pairs:
    the same bits.  Outside it nothing is written: the old bits."""
    n = ref.BITEXACT_N
    terms = ref.bitexact_terms(c, n)
    assert all(x == 0 or bin(x).count("1") >= 2 for _, _, x, _ in terms)
    assert ref.plan(terms, n, precision)[1] == 0 and ref.plan([(t, 0, x, z) for t, _, x, z in terms], n, precision)[1] == 0
    with Simulator(n, precision=precision) as with_c, Simulator(n, precision=precision) as without:
        for sim in (with_c, without):
            sim.write(ref.rand_state(n, 12))
        start = _bits(with_c)
        before = with_c.read()
        with_c.apply_pauli_rotations(ref.entries(terms, n))
        without.apply_pauli_rotations(pauli_rot_ref.texts(ref.uncontrolled(terms), n))
        got, free = _bits(with_c), _bits(without)
        _check(precision, with_c.read(), before, terms, f"bit-exact c={c:#x} p{precision}")
    inside = (np.arange(1 << n) & c) == c
    assert np.array_equal(got[inside], free[inside])
    assert np.array_equal(got[~inside], start[~inside])
    assert not np.array_equal(got[inside], start[inside])


@pytest.mark.parametrize("precision", PRECISIONS)
def test_runs(precision):
    n = ref.RUN_N
    K = plans.pauli_rotations_per_sweep()
    run, alternating = ref.run_terms(K), ref.run_terms(K, ref.RUN_CONTROLS)
    assert len(run) == 3 * K + 5 and {t for t, _, _, _ in run} >= set(pauli_rot_ref.SPECIAL_ANGLES)
    assert (run[10][2:], run[11][2:]) == ((pauli_rot_ref.LONG_RUN_X, 0), (pauli_rot_ref.LONG_RUN_X, 1))  # anticommuting neighbours
    with Simulator(n, precision=precision) as sim:
        sim.write(ref.rand_state(n, 12))
        for label, terms, want_sweeps in (("one control mask", run, -(-(3 * K + 5) // K)), ("alternating control masks", alternating, len(alternating))):
            before = sim.read()
            count = plans.sweeps_launched("pauli_rotation")
            sim.apply_pauli_rotations(ref.entries(terms, n))
            taken = plans.sweeps_launched("pauli_rotation") - count
            assert taken == ref.plan(terms, n, precision)[0] == want_sweeps, (label, taken)
            _check(precision, sim.read(), before, terms, f"run of {len(terms)}, {label} p{precision}")
    results = []
    a, b = ref.ORDER_PAIR
    for order in ([a, b], [b, a]):
        with Simulator(ref.ORDER_N, precision=precision) as sim:
            sim.write(ref.rand_state(ref.ORDER_N, 6))
            before = sim.read()
            count = plans.sweeps_launched("pauli_rotation")
            sim.apply_pauli_rotations(ref.entries(order, ref.ORDER_N))
            assert plans.sweeps_launched("pauli_rotation") - count == 1
            results.append(sim.read())
            _check(precision, results[-1], before, order, f"order p{precision}")
    assert np.max(np.abs(results[0] - results[1])) > 1e-2


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("c", ref.GRID_CONTROLS)
def test_multi_trip_grids(c, precision):
    """QSIM_OPT_GRID_CAP 0 (the resident grid), 3 (several trips per workgroup) and 1 << 30 (one workgroup per block of units):
    which workgroup takes a block changes no amplitude's arithmetic."""
    n = ref.GRID_N
    terms = ref.grid_terms(c, n)
    out = []
    for cap in (0, 3, 1 << 30):
        with Simulator(n, precision=precision, grid_cap=cap) as sim:
            sim.write(ref.rand_state(n, 160))
            before = sim.read()
            sim.apply_pauli_rotations(ref.entries(terms, n))
            out.append(_bits(sim))
    assert np.array_equal(out[0], out[1]) and np.array_equal(out[0], out[2])
    _check(precision, out[0].view(np.complex128).reshape(-1), before, terms, f"grid caps c={c:#x} p{precision}")


@pytest.mark.parametrize("precision", PRECISIONS)
def test_gate_route(precision):
    n = ref.GATE_N
    assert ref.plan(ref.GATE_TERMS, n, precision) == (0, len(ref.GATE_TERMS), 0)
    dtype = np.complex128 if precision == 64 else np.complex64
    with Simulator(n, precision=precision) as sim:
        sim.write(ref.rand_state(n, 7))
        before = sim.read()
        count = plans.sweeps_launched("pauli_rotation")
        sim.apply_pauli_rotations(ref.entries(ref.GATE_TERMS, n))
        got = sim.read()
        assert plans.sweeps_launched("pauli_rotation") == count  # 4x4s through the gate queue: no sweep
        _check(precision, got, before, ref.GATE_TERMS, f"gate route p{precision}")
    # queued between the two halves of a circuit
    circuit = Circuit.from_gates(n, circuits.random_gates(*ref.GATE_CIRCUIT))
    gates = [circuit.gate(i) for i in range(len(circuit))]
    half = len(gates) // 2
    with Simulator(n, precision=precision) as sim:
        count = plans.sweeps_launched("pauli_rotation")
        sim.run(circuit, 0, half)
        sim.apply_pauli_rotations(ref.entries(ref.GATE_TERMS, n))
        sim.run(circuit, half, -1)
        got = sim.read()
        assert plans.sweeps_launched("pauli_rotation") == count

    def truth(dt):
        return fp32_ref.replay(n, gates[half:], ref.replay(fp32_ref.replay(n, gates[:half], dtype=dt), ref.GATE_TERMS, dt), dt)

    want = truth(np.complex128)
    if precision == 64:
        worst = float(np.max(np.abs(got - want)))
        print(f"gates, 4x4s, gates: fp64 max abs err {worst:.3e}")
        assert worst < TOL
    else:
        report("gates, 4x4s, gates", check_fp32(got, want, truth(dtype)))


@pytest.mark.parametrize("precision", PRECISIONS)
def test_queued_gates_go_first(precision, golden_dir, oracle):
    path = os.path.join(golden_dir, "live_n13_seed104.qasm")
    n, truth, _, _ = oracle.run_qasm(path)
    assert n == 13
    terms = ref.queued_terms(n)
    sweeps, gates, _ = ref.plan(terms, n, precision)
    assert gates >= 2 and sweeps >= 10 and any(c == 0 for _, c, _, _ in terms) and any(c for _, c, _, _ in terms)
    circuit = Circuit.from_file(path)
    with Simulator(n, precision=precision) as sim:
        sim.run(circuit)  # queued: nothing has been flushed or waited for
        sim.apply_pauli_rotations(ref.entries(terms, n))
        got = sim.read()
    want = ref.replay(truth, terms)
    if precision == 64:
        worst = float(np.max(np.abs(got - want)))
        print(f"circuit then mixed terms vs the oracle's state: max abs err {worst:.3e}")
        assert worst < TOL
    else:
        ref32 = ref.replay(fp32_ref.replay(n, [circuit.gate(i) for i in range(len(circuit))]), terms, np.complex64)
        report("circuit then mixed terms", check_fp32(got, want, ref32))


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("n", ref.FRESH_SIZES)
def test_fresh_state(n, precision):
    term = ref.fresh_term(n)
    assert ref.plan([term], n, precision)[:2] == (1, 0)
    with Simulator(n, precision=precision) as sim:  # never touched: |0...0> is still held lazily
        count = plans.sweeps_launched("pauli_rotation")
        sim.apply_pauli_rotations(ref.entries([term], n))
        assert plans.sweeps_launched("pauli_rotation") - count == 1
        assert sim.get_support()[0] == (1 << n) - 1
        got = sim.read()
    want = np.zeros(1 << n, dtype=np.complex128)
    want[0] = 1.0
    assert np.array_equal(got, want)


@pytest.mark.parametrize("precision", PRECISIONS)
def test_partial_state(precision):
    n = ref.AFTER_FEW_N
    spec = fp32_ref.FEW_CIRCUIT
    few = Circuit.from_gates(n, circuits.random_gates(*spec))
    assert ref.plan(ref.AFTER_FEW_REACH, n, precision)[:2] == (2, 1) and ref.plan(ref.AFTER_FEW_NOTHING, n, precision)[:2] == (3, 0)
    with Simulator(n, precision=precision) as probe, Simulator(n, precision=precision) as reach, Simulator(n, precision=precision) as nothing:
        probe.run(few)
        before = probe.read()  # the read writes the zeros out: the state the terms must see is read from a twin
        assert not before[128:].any()
        for sim, terms in ((reach, ref.AFTER_FEW_REACH), (nothing, ref.AFTER_FEW_NOTHING)):
            sim.run(few)
            assert sim.get_support()[0] != (1 << n) - 1  # partial: most of the buffer has never been written
            sim.apply_pauli_rotations(ref.entries(terms, n))
        assert nothing.get_support()[0] == (1 << n) - 1  # dense after a sweep
        got, same = reach.read(), nothing.read()
    _check(precision, got, before, ref.AFTER_FEW_REACH, f"partial state, controls among the touched qubits p{precision}")
    assert np.count_nonzero(np.abs(got[1 << 17:]) > 1e-6) > 10  # X17 reached the untouched part
    assert np.array_equal(same, before)  # a control on an untouched qubit: nothing to rotate


@pytest.mark.parametrize("precision", PRECISIONS)
def test_helpers(precision):
    n = ref.HELPER_N
    j = np.arange(1 << n)
    start = ref.rand_state(n, 9)

    def close(got, want, terms, before, label):
        if precision == 64:
            assert np.max(np.abs(got - want)) < TOL, label
        else:
            report(label, check_fp32(got, want, ref.replay(before.astype(np.complex64), terms, np.complex64)))

    with Simulator(n, precision=precision) as sim:
        sim.write(start)
        for controls, target in ref.MCX_CASES:
            before = sim.read()
            count = plans.sweeps_launched("pauli_rotation")
            sim.apply_mcx(controls, target)
            got = sim.read()
            c = ref.mask_of(controls)
            want = before[np.where((j & c) == c, j ^ (1 << target), j)]
            assert plans.sweeps_launched("pauli_rotation") - count == (2 if len(controls) >= 2 else 0)
            close(got, want, ref.mcx_terms(controls, target) if len(controls) >= 2 else [(math.pi, c, 1 << target, 0), (-math.pi, c, 0, 0)], before,
                  f"mcx {controls} -> {target}")
            assert np.max(np.abs(got - before)) > 1e-3
        for qubits in ref.MCZ_CASES:
            before = sim.read()
            sim.apply_mcz(qubits)
            c = ref.mask_of(qubits)
            close(sim.read(), np.where((j & c) == c, -before, before), [(-2.0 * math.pi, c, 0, 0)], before, f"mcz {qubits}")
        for phi, qubits in ref.MCPHASE_CASES:
            before = sim.read()
            sim.apply_mcphase(phi, qubits)
            c = ref.mask_of(qubits)
            close(sim.read(), np.where((j & c) == c, np.exp(1j * phi) * before, before), [(-2.0 * phi, c, 0, 0)], before, f"mcphase {phi} {qubits}")
        with pytest.raises(ValueError):
            sim.apply_mcx((1, 2), 2)
        with pytest.raises(ValueError):
            sim.apply_mcz((3, 3))


@pytest.mark.parametrize("precision", PRECISIONS)
def test_zero_controls_take_the_uncontrolled_path(precision):
    n = 13
    lib = _lib.load()
    rotations = pauli_rot_ref.queued_rotations(n)
    texts = pauli_rot_ref.texts(rotations, n)
    xs, zs = (np.array([r[i] for r in rotations], dtype=np.uint64) for i in (1, 2))
    thetas = np.array([r[0] for r in rotations])
    zeros = np.zeros(len(rotations), dtype=np.uint64)
    out = []
    for how in ("plain", "empty controls", "NULL", "zeros"):
        with Simulator(n, precision=precision) as sim:
            sim.write(ref.rand_state(n, 104))
            count = plans.sweeps_launched("pauli_rotation")
            if how == "plain":
                sim.apply_pauli_rotations(texts)
            elif how == "empty controls":
                sim.apply_pauli_rotations([(theta, text, ()) for theta, text in texts])
            else:
                cp = None if how == "NULL" else zeros.ctypes.data_as(UP)
                _lib.check(lib.qsim_apply_controlled_pauli_rotations(sim._h, cp, xs.ctypes.data_as(UP), zs.ctypes.data_as(UP), thetas.ctypes.data_as(DP), xs.size))
            out.append((plans.sweeps_launched("pauli_rotation") - count, _bits(sim)))
    for taken, bits in out[1:]:
        assert taken == out[0][0] and np.array_equal(bits, out[0][1])


@pytest.mark.parametrize("precision", PRECISIONS)
def test_errors(precision):
    lib = _lib.load()
    n = 5
    fn = lib.qsim_apply_controlled_pauli_rotations

    def arr(values):
        a = np.array(values, dtype=np.uint64)
        return a, a.ctypes.data_as(UP)

    _ok, okp = arr([1, 2])
    _cs, csp = arr([4, 8])
    th = np.array([0.3, 0.4])
    thp = th.ctypes.data_as(DP)
    assert fn(None, csp, okp, okp, thp, 2) == _lib.ERR_ARG and b"NULL" in lib.qsim_last_error()
    with Simulator(n, precision=precision) as sim:
        sim.write(ref.rand_state(n, 5))
        before = _bits(sim)
        count = plans.sweeps_launched("pauli_rotation")
        keep = []
        for word, c, x, z in (("outside", [4, 8], [1, 1 << n], [0, 0]), ("outside", [4, 8], [1, 2], [0, 1 << 63]),
                              ("control qubit outside", [4, 1 << n], [1, 2], [1, 2]), ("control qubit outside", [1 << 63, 8], [1, 2], [1, 2]),
                              ("term 1: a control qubit carries a Pauli factor", [4, 8 | 2], [1, 2], [0, 0]),
                              ("term 1: a control qubit carries a Pauli factor", [4, 8], [1, 2], [0, 8]),
                              ("term 0: a control qubit carries a Pauli factor", [16 | 1, 8], [1, 2], [0, 0])):
            (ca, cp), (xa, xp), (za, zp) = arr(c), arr(x), arr(z)
            keep += [ca, xa, za]
            with pytest.raises(_lib.QsimError, match=word):
                _lib.check(fn(sim._h, cp, xp, zp, thp, 2))
        for args in ((csp, None, okp, thp, 2), (csp, okp, None, thp, 2), (csp, okp, okp, None, 2)):
            with pytest.raises(_lib.QsimError, match="NULL"):
                _lib.check(fn(sim._h, *args))
        with pytest.raises(_lib.QsimError, match="negative"):
            _lib.check(fn(sim._h, csp, okp, okp, thp, -1))
        for bad in (float("nan"), float("inf")):
            bt = np.array([0.3, bad])
            with pytest.raises(_lib.QsimError, match="non-finite"):
                _lib.check(fn(sim._h, csp, okp, okp, bt.ctypes.data_as(DP), 2))
        _lib.check(fn(sim._h, None, None, None, None, 0))  # zero terms: fine, does nothing
        for bad in ((0.1, "X0", (0,)), (0.1, "Z1 X0", (1,)), (0.1, "X0", (2, 2)), (0.1, "X0", (n,)), (0.1, "X0", (-1,)), (0.1, "X0", (1,), 3)):
            with pytest.raises(ValueError):
                sim.apply_pauli_rotations([(0.2, "X1 X2", (3,)), bad])  # the valid first term is not applied either
        with pytest.raises(ValueError):
            sim.apply_pauli_rotation(0.1, "X0", controls=(0,))
        assert np.array_equal(_bits(sim), before) and plans.sweeps_launched("pauli_rotation") == count
        sim.reset(holds_index0=False)  # a shard that holds nothing stays untouched
        sim.apply_pauli_rotations([(0.3, "Z0 Z1", (2, 3)), (0.2, "X0 X1", (4,)), (0.1, "", (0, 1))])
        assert plans.sweeps_launched("pauli_rotation") == count and sim.get_support()[1:] == (1, 0.0)
    with Cluster(n, 2, devices=[0, 0]) as cl:
        cl.run(Circuit.from_gates(n, circuits.random_gates(n, 40, 5, "all")))
        before = cl.read()
        with pytest.raises(ValueError, match="sharded states have no controlled rotations yet"):
            cl.apply_pauli_rotation(0.3, "X0 X1", controls=(2,))
        with pytest.raises(ValueError, match="sharded"):
            cl.apply_pauli_rotations([(0.3, "Z0"), (0.3, "X0 X1", (2, 3))])
        cl.apply_pauli_rotations([(0.0, "Z0", ())])  # no control anywhere: the cluster's own call
        assert np.array_equal(cl.read(), before)
