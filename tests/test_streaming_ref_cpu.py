"""Pins what tests/test_gpu_streaming_kernels.py relies on, on the CPU: its numpy references against the oracle at every position
of small registers, the guard-size and trip-count tables of tests/streaming_ref.py against the figures read off csrc/launch.inc,
and the gaps of the n = 29 sampling state."""
import numpy as np
import pytest

import streaming_ref as sr
from fp32_ref import replay
from helpers import np_apply_1q, np_apply_2q, np_apply_cx, random_unitary


# ---- reference functions -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", range(1, 9))
def test_numpy_references_equal_the_oracle_at_every_position(oracle, n):
    """np_apply_1q / np_apply_cx / np_apply_2q and the complex128 replay against oracle.apply_1q (which applies the TRANSPOSE of
    its argument) and oracle.apply_cx.  The oracle has no 4x4: a 4x4 that is a product of 1q gates and cx is composed there."""
    rng = np.random.default_rng(800 + n)
    s = sr.rand_state(n, 810 + n)
    for q in range(n):
        for U in (sr.dense_2x2(q), np.diag([1.0, sr.LAMBDA]), np.diag([sr.D0, sr.D1]), random_unitary(2, rng)):
            want = s.copy()
            oracle.apply_1q(want, n, U.T, q)
            assert np.max(np.abs(np_apply_1q(s, n, U, q) - want)) < 1e-14, q
            assert np.max(np.abs(replay(n, [("u1", q, U)], start=s, dtype=np.complex128) - want)) < 1e-14, q
    for c in range(n):
        for t in range(n):
            want = s.copy()
            oracle.apply_cx(want, n, c, t)
            assert np.array_equal(np_apply_cx(s, n, c, t), want), (c, t)
            assert np.array_equal(replay(n, [("cx", c, t)], start=s, dtype=np.complex128), want), (c, t)
    for hi in range(1, n):
        for lo in range(hi):
            A, B, C, D = (random_unitary(2, rng) for _ in range(4))
            # (C on hi, D on lo) . cx(hi -> lo) . (A on hi, B on lo), as the oracle applies it gate by gate
            want = s.copy()
            oracle.apply_1q(want, n, A.T, hi)
            oracle.apply_1q(want, n, B.T, lo)
            oracle.apply_cx(want, n, hi, lo)
            oracle.apply_1q(want, n, C.T, hi)
            oracle.apply_1q(want, n, D.T, lo)
            cx = np.eye(4)[[0, 1, 3, 2]]  # row / column index = (bit hi, bit lo)
            M = np.kron(C, D) @ cx @ np.kron(A, B)
            assert np.max(np.abs(np_apply_2q(s, n, M, hi, lo) - want)) < 1e-14, (hi, lo)
            assert np.max(np.abs(replay(n, [("u2", hi, lo, M)], start=s, dtype=np.complex128) - want)) < 1e-14, (hi, lo)


def test_case_matrices_are_what_the_cases_need():
    for seed in range(40):
        U = sr.dense_2x2(seed)
        assert np.allclose(U.conj().T @ U, np.eye(2), atol=1e-14)
        assert abs(U[0, 1] - U[1, 0]) > 0.1 and np.min(np.abs(U)) > 0.3  # not symmetric, no entry near zero
    for z in (sr.LAMBDA, sr.D0, sr.D1):
        assert abs(abs(z) - 1.0) < 1e-15 and abs(z - 1.0) > 1.5
    for U, p0 in zip(sr.sparse_matrices(), sr.SPARSE_P0):
        assert np.allclose(U.conj().T @ U, np.eye(2), atol=1e-14) and abs(U[0, 1] - U[1, 0]) > 0.1
        assert abs(abs(U[0, 0]) ** 2 - p0) < 1e-15 and 0.3 <= p0 <= 0.7 and 0.3 <= 1.0 - p0 <= 0.7


# ---- guard sizes ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kernel,guarded,first_unguarded", [
    ("k_gate1_hi", range(7, 11), 11), ("k_gate1_lo", range(1, 10), 10), ("k_diag1_full", range(1, 10), 10),
    ("k_phase", range(3, 11), 11), ("k_cx", range(2, 12), 12), ("k_gate2_hh", range(8, 11), 11)])
def test_guard_size_table(kernel, guarded, first_unguarded):
    """Read off QSIM_DISPATCH_GUARD: guarded while items < TPB * IPT (items is a power of two, so `%` and `<` agree)."""
    assert sr.guarded_sizes(kernel) == list(guarded)
    assert not sr.launch(kernel, first_unguarded).guarded and sr.launch(kernel, first_unguarded).tiles == 1
    assert first_unguarded in sr.EVERY_POSITION_SIZES
    for n in guarded:
        la = sr.launch(kernel, n)
        assert la.grid == 1 and la.tiles == 1  # one partly filled work tile
        assert sr.positions(kernel, n), (kernel, n)
    assert sr.launch("k_pack", 9).guarded and not sr.launch("k_pack", 10).guarded


def test_positions_cover_what_the_engine_dispatches():
    n = 12
    assert len(sr.positions("k_gate1_hi", n)) + len(sr.positions("k_gate1_lo", n)) == n
    assert len(sr.positions("k_cx", n)) == n * (n - 1) and len(sr.positions("k_gate2_hh", n)) == 15
    assert sr.positions("k_gate1_lo", 3) == [(0,), (1,), (2,)] and sr.positions("k_gate1_hi", 6) == []
    assert sr.positions("k_phase", 2) == [] and sr.positions("k_gate2_hh", 7) == []


# ---- trip counts ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kernel", sorted(sr.GATE_KERNELS))
def test_grid_caps_make_the_gate_kernels_loop(kernel):
    """n = 14 under grid_cap 1, 3 and 5: the busiest workgroup takes at least two trips and, under 3 and 5, the workgroups do not
    all take as many.  k_cx has four work tiles there (2^12 items in tiles of 2^10), so a cap of 5 does not bind: its multi-trip
    caps are 1 and 3."""
    n = sr.LOOP_N
    assert sr.launch(kernel, n, 0).max_trips == 1 and sr.launch(kernel, n, 1 << 30).max_trips == 1
    assert not sr.launch(kernel, n).guarded
    for cap in (1, 3, 5):
        la = sr.launch(kernel, n, cap)
        if kernel == "k_cx" and cap == 5:
            assert (la.tiles, la.grid, la.max_trips) == (4, 4, 1)
            continue
        assert la.grid == cap and la.max_trips >= 2, (kernel, cap, la)
        assert la.uneven == (cap != 1), (kernel, cap, la)
    la = sr.launch("k_pack", n, 3)
    assert la.grid == 3 and la.max_trips == 6 and la.uneven and sr.launch("k_pack", n).max_trips == 1


def test_capped_grids_loop_at_the_sizes_the_tests_use():
    for kernel in ("k_init", "k_zero_outside"):
        assert sr.launch(kernel, sr.INIT_LOOP_N - 1).max_trips == 1
        la = sr.launch(kernel, sr.INIT_LOOP_N)
        assert la.grid == 16384 and la.max_trips == 2 and not la.uneven
    assert sr.launch("k_block_prob", sr.SAMPLE_LOOP_N - 1).max_trips == 1
    la = sr.launch("k_block_prob", sr.SAMPLE_LOOP_N)
    assert la.grid == 65536 and la.max_trips == 2
    assert sr.launch("k_block_prob", sr.SAMPLE_DENSE_N).grid == 256
    for n in sr.SAMPLE_SMALL_SIZES:
        assert sr.launch("k_block_prob", n).tiles == 1  # the block is the whole register
    assert sr.capped_grid(0, 1, 8) == 1 and sr.grid_for(0, 1 << 23) == sr.MAX_GRID and sr.grid_for(sr.MAX_GRID, 5) == 5


def test_bands_cover_what_a_wrong_index_can_reach():
    for n in sr.EVERY_POSITION_SIZES:
        assert sr.band(n) >= 4096 and sr.band(n) >= 4 << n
    # the largest index the last item of a FULL work tile reaches at a guarded size: two zero bits inserted, both bits set
    def ins(t, q):
        return ((t >> q) << (q + 1)) | (t & ((1 << q) - 1))

    for n in range(2, 12):
        worst = max(ins(ins(sr.TPB * 4 - 1, lo), hi) | 1 << lo | 1 << hi for hi in range(1, n) for lo in range(hi))
        assert worst < 4096 <= sr.band(n), n


# ---- the n = 29 sampling state ---------------------------------------------------------------------------------------------------
def test_sparse_sampling_state_has_wide_gaps():
    idx, amps, p = sr.sparse_state()
    draws, want, run = sr.sparse_draws()
    assert len(idx) == 16 and np.all(np.diff(idx) > 0) and idx[-1] < 1 << sr.SAMPLE_LOOP_N
    assert np.max(np.abs(np.abs(amps) ** 2 - p)) < 1e-15 and abs(run[-1] - 1.0) < 1e-15
    assert p.min() >= 0.3 ** 4
    gap = float(np.min(np.diff(np.concatenate([[0.0], run]))))
    assert gap >= 0.3 ** 4
    assert len(draws) == 17 and draws[0] == 0.0
    for r, w in zip(draws, want):
        assert np.min(np.abs(run - r)) >= 0.5 * gap * (1 - 1e-12), r     # no draw near a boundary (a midpoint is half its own gap away) ...
        assert w == idx[np.searchsorted(run, r, side="left")] or r == 0.0  # ... and each answered by the first index that reaches it
    assert want[0] == idx[0] == 0
    # half the mass (the 1 outcome of qubit 28) lies in blocks only the second trip of k_block_prob's loop sums
    far = idx >> sr.SAMPLE_BLOCK_BITS >= 65536
    assert far.sum() == 8 and abs(p[far].sum() - (1.0 - sr.SPARSE_P0[0])) < 1e-15 and 0.3 <= p[far].sum() <= 0.7
    # two of the sixteen share a block (they differ in qubit 3 only): the search inside a block is exercised too
    assert len(set(idx >> sr.SAMPLE_BLOCK_BITS)) == 8


def test_zero_block_state_sums_exactly(oracle):
    """What lets the GPU test demand the reference's sample for every draw, boundary draws included."""
    n = sr.SAMPLE_DENSE_N
    s = sr.zero_block_state(n)
    assert np.array_equal(s.astype(np.complex64).astype(np.complex128), s)
    blocks = np.flatnonzero(np.abs(s.reshape(-1, 1 << sr.SAMPLE_BLOCK_BITS)).sum(axis=1))
    assert list(blocks) == [3, 200, 201] and s[3 << sr.SAMPLE_BLOCK_BITS] == 0 and s[(202 << sr.SAMPLE_BLOCK_BITS) - 1] != 0
    cumul = oracle.cumulative(s, n)
    units = cumul * 2.0 ** 14
    assert np.array_equal(units, np.round(units)) and cumul[-1] == 1.0
    p = s.real * s.real + s.imag * s.imag
    assert np.array_equal(np.cumsum(p[::-1])[::-1][0:1], [1.0]) and np.array_equal(np.cumsum(p), cumul)  # any order, same sums


def test_pack_cases_fit_their_registers():
    for n in sr.PACK_SMALL_SIZES:
        for bits in sr.pack_bit_sets(n):
            assert all(0 <= b < n for b in bits) and list(bits) == sorted(set(bits)) and len(bits) <= 3
            src = sr.pack_src_index(n, bits)
            assert sorted(src) == list(range(1 << n))
    assert sr.pack_bit_sets(2) == [(0,), (0, 1), (1,)] and (1, 3, 4) in sr.pack_bit_sets(5)
