"""Deferred X gates in the scheduler's feed (SchedConfig::defer_flips), host only.

With the option on, an X produces no cluster: it toggles a flip bit on its qubit, every later gate on that qubit is fed
conjugated by the flip (rows and columns permuted, nothing multiplied), an anti-diagonal 2x2 is fed as the diagonal X·A, and
what is left at the end is one index mask m: the circuit's state is the replayed one with amplitude i moved to i ^ m.
qsim_schedule_circuit_deferred hands out such a schedule and its mask; here it is replayed with numpy and held to the oracle
running the unfused circuit at 1e-10, and the conjugation is checked byte for byte.

The oracle applies 1-qubit gates and cx only, so the case with arbitrary 2-qubit gates takes the oracle's kernels for those two
and tests/helpers.np_apply_2q for the 4x4s (the reference of test_scheduler_cpu.test_generic_two_qubit_gates_and_blocking)."""
import numpy as np
import pytest

from gpu_quantum_simulator_amd import Circuit, circuits, gate_matrix
from helpers import np_apply_2q, random_unitary, replay_schedule

TOL = 1e-10
SMALL_TILES = dict(fuse=3, tile_bits=8, tile_low_bits=4, tile_max_ops=6)  # grouping, high-bit choice and blocking at n <= 11
X = np.array([[0, 1], [1, 0]], dtype=np.complex128)


def _deferred(c, **kw):
    flips = []
    sched = c.schedule(flips=flips, **kw)
    return sched, flips[0]


def _replay_with_flips(n, sched, mask):
    psi = replay_schedule(n, sched)
    return psi[np.arange(1 << n) ^ mask]  # final[i] = replayed[i ^ mask]


def _every_third_is_x(n, depth, seed):
    rng = np.random.default_rng(seed)
    base = circuits.random_gates(n, depth, seed, "all")
    return [("x", int(rng.integers(n))) if i % 3 == 2 else g for i, g in enumerate(base)]


CASES = [(n, depth, seed, vocab) for vocab in ("all", "clifford_t") for n, depth, seed in ((3, 80, 1), (6, 300, 2), (9, 400, 3), (11, 600, 4))]


@pytest.mark.parametrize("n,depth,seed,vocab", CASES + [(9, 300, 5, "thirds"), (11, 450, 6, "thirds")])
def test_deferred_schedule_replays_to_the_oracle(oracle, tmp_path, n, depth, seed, vocab):
    gates = _every_third_is_x(n, depth, seed) if vocab == "thirds" else circuits.random_gates(n, depth, seed, vocab)
    path = circuits.write_qasm(str(tmp_path / "c.qasm"), n, gates)
    _, want, _, _ = oracle.run_qasm(path)
    c = Circuit.from_file(path)
    sched, mask = _deferred(c, **SMALL_TILES)
    assert 0 <= mask < (1 << n)
    got = _replay_with_flips(n, sched, mask)
    assert np.max(np.abs(got - want)) < TOL
    # no X survives as a scheduled gate, and nothing is counted twice
    assert sum(s[5] for s in sched) <= depth
    plain = c.schedule(**SMALL_TILES)
    assert np.max(np.abs(replay_schedule(n, plain) - want)) < TOL  # the same circuit with the option off, for the record of the pair


def test_generic_gates_with_flips_in_between(oracle):
    """Arbitrary u1, u2 and cx with X gates and anti-diagonal u1s in between, n = 10, 120 gates.  The scheduler drops a cluster
    that is exactly the identity, with its count; among random unitaries only a cx repeated on the same operands with nothing in
    between makes one, so that statement is not generated twice in a row.  Every statement is then counted exactly once: the folded
    counts sum to the input length."""
    rng = np.random.default_rng(11)
    n = 10
    c = Circuit.empty(n)
    ref = oracle.zero_state(n)
    last = [None] * n  # per qubit: the cx statement that touched it last, if nothing else has since (an X in between does not count: it is deferred)
    for _ in range(120):
        r = int(rng.integers(5))
        if r == 1:
            a, b = (int(x) for x in rng.choice(n, 2, replace=False))
            if last[a] == last[b] == (a, b):
                r = 0
            else:
                c.append_cx(a, b); oracle.apply_cx(ref, n, a, b)
                last[a] = last[b] = (a, b)
                continue
        if r == 0:
            q = int(rng.integers(n)); U = random_unitary(2, rng)
            c.append_1q(U, q); oracle.apply_1q(ref, n, U.T, q)  # the oracle applies the transpose of its argument
            last[q] = None
        elif r == 2:
            lo, hi = sorted(int(x) for x in rng.choice(n, 2, replace=False))
            U = random_unitary(4, rng)
            c.append_2q(U, hi, lo); ref = np.ascontiguousarray(np_apply_2q(ref, n, U, hi, lo))
            last[lo] = last[hi] = None
        elif r == 3:
            q = int(rng.integers(n))
            c.append_1q(X, q); oracle.apply_1q(ref, n, X.T, q)
        else:
            q = int(rng.integers(n))
            a, b = np.exp(1j * rng.uniform(0, 2 * np.pi, 2))
            A = np.array([[0, a], [b, 0]])
            c.append_1q(A, q); oracle.apply_1q(ref, n, A.T, q)
            last[q] = None
    sched, mask = _deferred(c, fuse=3, tile_bits=8, tile_low_bits=5, tile_max_ops=4)
    assert mask != 0
    assert np.max(np.abs(_replay_with_flips(n, sched, mask) - ref)) < TOL
    assert sum(s[5] for s in sched) == 120


def _one(c, **kw):
    sched, mask = _deferred(c, fuse=3, **kw)
    assert len(sched) == 1, sched
    return sched[0], mask


def test_conjugation_moves_entries_and_multiplies_nothing():
    rng = np.random.default_rng(3)
    # x q; U q; x q: the scheduled matrix is X U X byte for byte and no flip is left
    U = random_unitary(2, rng)
    c = Circuit.empty(8)
    c.append_1q(X, 7); c.append_1q(U, 7); c.append_1q(X, 7)
    (_, _, kind, qs, m, folded), mask = _one(c)
    assert (kind, qs, mask, folded) == ("u1", (7,), 0, 3)
    assert m.tobytes() == np.ascontiguousarray(U[::-1, ::-1]).tobytes()
    # a 2-qubit U with the X on either operand: index bits of the 4x4 are (q_hi, q_lo)
    U4 = random_unitary(4, rng)
    for q, bit in ((7, 2), (6, 1)):
        c = Circuit.empty(8)
        c.append_1q(X, q); c.append_2q(U4, 7, 6); c.append_1q(X, q)
        (_, _, kind, qs, m, folded), mask = _one(c)
        idx = np.arange(4) ^ bit
        assert (kind, qs, mask, folded) == ("u2", (7, 6), 0, 3)
        assert m.tobytes() == np.ascontiguousarray(U4[np.ix_(idx, idx)]).tobytes()


def test_a_diagonal_gate_stays_diagonal():
    """... exactly, so that it still asks for no tile qubit: alone it runs as the phase kernel, which only a diagonal 2x2 gets."""
    d0, d1 = np.exp(0.3j), np.exp(-1.1j)
    c = Circuit.empty(8)
    c.append_1q(X, 7); c.append_1q(np.diag([d0, d1]), 7); c.append_1q(X, 7)
    (_, kclass, kind, qs, m, _), mask = _one(c)
    assert (kclass, kind, qs, mask) == ("phase", "u1", (7,), 0)
    assert m.tobytes() == np.diag([d1, d0]).astype(np.complex128).tobytes()
    # an anti-diagonal gate is fed as the diagonal X A and leaves the X owed
    A = np.array([[0, d0], [d1, 0]])
    c = Circuit.empty(8)
    c.append_1q(A, 7)
    (_, kclass, _, _, m, _), mask = _one(c)
    assert (kclass, mask) == ("phase", 1 << 7)
    assert m.tobytes() == np.diag([d1, d0]).astype(np.complex128).tobytes()


def test_cx_under_flips():
    c = Circuit.empty(8)
    c.append_1q(X, 0); c.append_cx(7, 0); c.append_1q(X, 0)  # a flipped target changes nothing
    (_, kclass, kind, qs, _, folded), mask = _one(c)
    assert (kclass, kind, qs, mask, folded) == ("cx", "cx", (7, 0), 0, 3)
    c = Circuit.empty(8)
    c.append_1q(X, 7); c.append_cx(7, 6)  # a flipped control: the 4x4 that acts where the control is 0
    (_, _, kind, qs, m, _), mask = _one(c)
    want = np.zeros((4, 4), dtype=np.complex128)
    for i, j in ((0, 1), (1, 0), (2, 2), (3, 3)):
        want[i, j] = 1
    assert (kind, qs, mask) == ("u2", (7, 6), 1 << 7) and m.tobytes() == want.tobytes()


def test_gate_names_that_defer():
    """Of the parser's gate table only x is anti-diagonal: h, sx and the diagonal gates are scheduled as before."""
    for tok in ("x", "sx", "z", "s", "sdg", "t", "tdg", "h", "rz(0.25)"):
        c = Circuit.empty(4)
        c.append_1q(gate_matrix(tok), 2)
        sched, mask = _deferred(c, fuse=3)
        assert (mask, len(sched)) == ((1 << 2, 0) if tok == "x" else (0, 1)), tok


def test_levels_below_three_ignore_the_option():
    gates = circuits.random_gates(6, 120, 8, "all")
    c = Circuit.from_gates(6, gates)
    for fuse in (0, 1, 2):
        flips = []
        sched = c.schedule(fuse=fuse, flips=flips)
        assert flips == [0]
        plain = c.schedule(fuse=fuse)
        assert len(sched) == len(plain) and all(a[:4] == b[:4] and a[5] == b[5] for a, b in zip(sched, plain))
