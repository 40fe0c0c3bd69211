"""The one-gate streaming kernels (csrc/gate_kernels.inc), the readout kernels (csrc/readout_kernels.inc) and k_pack where they
guard, loop and end: every position at every register size that takes a bounds-checked instantiation, grid caps that make the
grid-stride loops take several and unequal numbers of trips, and the register sizes from which k_init, k_zero_outside and
k_block_prob loop under their own caps.  What a case is meant to reach is asserted against tests/streaming_ref.py (the launch
arithmetic restated), which kernel class ran against sim.stats().

fp64: a complex128 oracle / numpy result, 1e-10 abs per amplitude; kernels that only move amplitudes or write constants (cx,
k_init, k_zero_outside, pack) are compared with np.array_equal.  fp32: the criterion of tests/fp32_ref.py, truth and complex64
replay both started from the state as stored after the write, with 2e-5 abs as the weaker second check; cx is bit-exact.

Guard bands exist for fp64 states only: an external buffer (Simulator(external_ptr=...)) is fp64 by definition, so the fp32 cases
of the every-position test run on a state that owns its buffer and check values alone.  k_pack writes to the caller's buffer in
either precision and is banded in both."""
import numpy as np
import pytest

import streaming_ref as sr
from fp32_ref import check_fp32, replay, report
from gpu_quantum_simulator_amd import Circuit, Simulator, _lib, circuits
from helpers import np_apply_2q, random_unitary

pytestmark = pytest.mark.gpu
TOL = 1e-10
TOL32 = 2e-5
PRECISIONS = [64, 32]


# ---- gates, references, the check of one gate ------------------------------------------------------------------------------------
def _gate(kernel, pos, seed):
    """The gate, as fp32_ref.replay takes it, that the engine hands to `kernel` at fuse 0."""
    if kernel in ("k_gate1_hi", "k_gate1_lo"):
        return ("u1", pos[0], sr.dense_2x2(seed))
    if kernel == "k_phase":
        return ("u1", pos[0], np.diag([1.0, sr.LAMBDA]))
    if kernel == "k_diag1_full":
        return ("u1", pos[0], np.diag([sr.D0, sr.D1]))
    if kernel == "k_cx":
        return ("cx", pos[0], pos[1])
    return ("u2", pos[0], pos[1], random_unitary(4, np.random.default_rng(seed)))


def _apply(sim, g):
    if g[0] == "u1":
        sim.apply_1q(g[2], g[1])
    elif g[0] == "cx":
        sim.apply_cx(g[1], g[2])
    else:
        sim.apply_2q(g[3], g[1], g[2])


def _truth(oracle, s, n, g):
    """The gate applied to a copy of `s` in complex128: the oracle for what it has (it applies the transpose of its argument)."""
    want = np.array(s, dtype=np.complex128)
    if g[0] == "u1":
        oracle.apply_1q(want, n, np.asarray(g[2]).T, g[1])
    elif g[0] == "cx":
        oracle.apply_cx(want, n, g[1], g[2])
    else:
        want = np_apply_2q(want, n, g[3], g[1], g[2])
    return want


def _check_gate(oracle, precision, n, s, g, got, label):
    if precision == 64:
        want = _truth(oracle, s, n, g)
        if g[0] == "cx":
            assert np.array_equal(got, want), label
        else:
            assert np.max(np.abs(got - want)) < TOL, label
        return
    s32 = s.astype(np.complex64)
    want32 = _truth(oracle, s32, n, g)
    if g[0] == "cx":
        assert np.array_equal(got, want32), label
        return
    report(label, check_fp32(got, want32, replay(n, [g], start=s32)))
    assert np.max(np.abs(got - _truth(oracle, s, n, g))) < TOL32, label


def _launches(sim):
    return {k: v["launches"] for k, v in sim.stats()["kernels"].items()}


def _hadamards(n):
    return Circuit.from_gates(n, [("h", q) for q in range(n)])


def _dirty(sim, n):
    """Leaves a dense state (every amplitude 2^(-n/2)) in the buffer behind a reset: whatever k_init or k_zero_outside then fails
    to write shows as a non-zero amplitude.  (Fresh device memory is often zero already and would hide it.)"""
    sim.set_option(_lib.OPT_FUSE, 3)
    sim.run(_hadamards(n))
    sim.sync()
    sim.reset()


# ---- a. every position at every guarded size, with guard bands ---------------------------------------------------------------
def _batches(n):
    """(kernel, gates) per kernel's batch on n qubits: a dense 2x2 and diag(1, lambda) and diag(d0, d1) on every target, cx on every
    ordered pair, a dense 4x4 on every pair with q_lo >= 6.  diag(1, lambda) takes k_phase from q = 2 and k_diag1_full below."""
    lam = np.diag([1.0, sr.LAMBDA])
    out = [(k, [_gate(k, p, 100 * n + i) for i, p in enumerate(sr.positions(k, n))])
           for k in ("k_gate1_lo", "k_gate1_hi", "k_phase", "k_diag1_full", "k_cx", "k_gate2_hh")]
    out.insert(3, ("k_diag1_full", [("u1", q, lam) for q in range(min(n, 2))]))
    return [(k, gates) for k, gates in out if gates]


@pytest.mark.parametrize("n", sr.EVERY_POSITION_SIZES)
@pytest.mark.parametrize("precision", PRECISIONS)
def test_every_position_at_every_guarded_size(oracle, precision, n):
    """n = 1 .. 12 covers every size at which a gate kernel's launch is guarded and the first at which it is not.  The state is
    random and rewritten before each gate.  The fp64 state is an external one in the middle of a torch buffer whose bands of
    streaming_ref.band(n) amplitudes on each side hold a fixed pattern and must be bit-identical after every kernel's batch; fp32
    states cannot be external, so the fp32 cases check values only."""
    import torch
    N, band = 1 << n, sr.band(n)
    opts = {}
    if precision == 64:
        host = (np.arange(2 * (2 * band + N), dtype=np.float64) % 251.0 + 1.0) * 0.5  # finite, non-zero, no two neighbours equal
        buf = torch.from_numpy(host.copy()).reshape(-1, 2).to("cuda")
        torch.cuda.synchronize()  # the fill runs on torch's stream, the kernels on the engine's: order them
        opts["external_ptr"] = buf.data_ptr() + 16 * band
    forms = {kernel: sr.launch(kernel, n).guarded for kernel, _ in _batches(n)}
    # what this size is here for: some kernel's guarded form, or the first size at which one stops being guarded
    assert any(forms.values()) or any(n == sr.guarded_sizes(k)[-1] + 1 for k in forms), forms
    with Simulator(n, fuse=0, precision=precision, **opts) as sim:
        s = sr.rand_state(n, 900 + n)
        for kernel, gates in _batches(n):
            sim.write(s)  # (the first write has the engine write |0...0> first: k_init runs inside the bands too)
            sim.reset_stats()
            for g in gates:
                sim.write(s)
                _apply(sim, g)
                _check_gate(oracle, precision, n, s, g, sim.read(), f"{kernel} n={n} guarded={forms[kernel]} {g[:3] if g[0] != 'u1' else g[:2]}")
            ran = _launches(sim)
            assert ran[sr.STATS_CLASS[kernel]] == len(gates) == sum(ran.values()), (kernel, ran)
            if precision == 64:
                sim.sync()
                after = buf.cpu().numpy().reshape(-1)
                for lo, hi in ((0, 2 * band), (2 * (band + N), 2 * (2 * band + N))):
                    assert np.array_equal(after[lo:hi].view(np.uint64), host[lo:hi].view(np.uint64)), (kernel, n, lo)


# ---- b. where the loop takes more than one trip ---------------------------------------------------------------------------------
@pytest.mark.parametrize("kernel", sorted(sr.GATE_KERNELS))
@pytest.mark.parametrize("precision", PRECISIONS)
def test_grid_stride_loop_takes_several_trips(oracle, precision, kernel):
    """n = 14, every position of the kernel, under grid_cap 0, 1, 3, 5 and 2^30: one workgroup walking every work tile, three and
    five workgroups taking unequal numbers of trips, and a cap that does not bind.  The uncapped result is held to the
    reference; every other cap's is bit-identical to it, since each amplitude is written by one thread with the same instruction
    sequence whatever the trip."""
    n = sr.LOOP_N
    trips = {cap: sr.launch(kernel, n, cap) for cap in sr.LOOP_CAPS}
    assert trips[0].max_trips == 1 and not trips[0].guarded
    assert trips[1].max_trips >= 2 and trips[3].max_trips >= 2 and trips[3].uneven, trips
    assert trips[5].max_trips >= 2 or kernel == "k_cx", trips  # (four work tiles: a cap of 5 leaves k_cx one trip each)
    s = sr.rand_state(n, 1400)
    gates = [_gate(kernel, p, 1400 + i) for i, p in enumerate(sr.positions(kernel, n))]
    with Simulator(n, fuse=0, precision=precision) as sim:
        sim.write(s)
        sim.reset_stats()
        for g in gates:
            label = f"{kernel} n={n} {g[:3] if g[0] != 'u1' else g[:2]}"
            ref = None
            for cap in sr.LOOP_CAPS:
                sim.set_option(_lib.OPT_GRID_CAP, cap)
                sim.write(s)
                _apply(sim, g)
                got = sim.read()
                if cap == 0:
                    _check_gate(oracle, precision, n, s, g, got, label)
                    ref = got
                else:
                    assert np.array_equal(got, ref), (label, cap)
        ran = _launches(sim)
        assert ran[sr.STATS_CLASS[kernel]] == len(gates) * len(sr.LOOP_CAPS) == sum(ran.values()), ran


# ---- c. k_init and k_zero_outside past their grid cap ----------------------------------------------------------------------------
@pytest.mark.parametrize("precision", PRECISIONS)
def test_init_past_its_grid_cap(precision):
    """n = 23: k_init's 16384 workgroups take two trips.  A reset state over a stale dense one, a dense 2x2 on qubit 22 and one on
    qubit 0 at fuse 0, the whole state read: four amplitudes are products of matrix entries, every other one is exactly 0.0."""
    n = sr.INIT_LOOP_N
    assert sr.launch("k_init", n).max_trips >= 2
    A, B = sr.dense_2x2(231), sr.dense_2x2(232)
    with Simulator(n, precision=precision) as sim:
        _dirty(sim, n)
        sim.set_option(_lib.OPT_FUSE, 0)
        sim.reset_stats()
        sim.apply_1q(A, n - 1)
        sim.apply_1q(B, 0)
        got = sim.read()
        ran = _launches(sim)
    assert (ran["init"], ran["gate1"], ran["gate1_lo"], sum(ran.values())) == (1, 1, 1, 3), ran
    places = [0, 1, 1 << (n - 1), 1 << (n - 1) | 1]
    want = np.array([A[0, 0] * B[0, 0], A[0, 0] * B[1, 0], A[1, 0] * B[0, 0], A[1, 0] * B[1, 0]])
    if precision == 64:
        assert np.max(np.abs(got[places] - want)) < TOL
    else:
        report(f"init n={n}", check_fp32(got[places], want, replay(2, [("u1", 1, A), ("u1", 0, B)])))
        assert np.max(np.abs(got[places] - want)) < TOL32
    assert np.count_nonzero(got) == 4  # (the four are non-zero: they passed the tolerance)


FEW_QUBITS = (0, 4, 11, 17, 22)


def _few_qubit_circuit(n):
    """A random circuit on the five qubits FEW_QUBITS of an n-qubit register: (circuit, its gates on a 5-qubit register)."""
    small = circuits.random_gates(5, 80, 13, "all")
    wide = [g[:-1] + (FEW_QUBITS[g[-1]],) if g[0] != "cx" else ("cx", FEW_QUBITS[g[1]], FEW_QUBITS[g[2]]) for g in small]
    c5 = Circuit.from_gates(5, small)
    return Circuit.from_gates(n, wide), [c5.gate(i) for i in range(len(c5))]


@pytest.mark.parametrize("precision", PRECISIONS)
def test_zero_outside_past_its_grid_cap(precision):
    """n = 23: k_zero_outside's 16384 workgroups take two trips.  Over a stale dense state, a reset and a fuse-3 circuit on five
    qubits, qubit 22 among them, leave the support partial; norm2 materialises the state.  Read back, it matches the replay
    inside the support and is exactly zero outside it, and norm2 is the fp64 sum over it."""
    n = sr.INIT_LOOP_N
    assert sr.launch("k_zero_outside", n).max_trips >= 2 and FEW_QUBITS[-1] == n - 1
    circuit, gates5 = _few_qubit_circuit(n)
    with Simulator(n, precision=precision) as sim:
        _dirty(sim, n)
        sim.reset_stats()
        sim.run(circuit)
        support, pending, _ = sim.get_support()
        assert not pending and support != (1 << n) - 1 and all(support >> q & 1 for q in FEW_QUBITS)
        ran = _launches(sim)
        assert ran["tile"] >= 1 and ran["tile"] == sum(ran.values()), ran
        nv = sim.norm2()
        ran = _launches(sim)
        assert ran["init"] == 1 and ran["tile"] + 1 == sum(ran.values()), ran
        got = sim.read()
    idx = np.arange(1 << n, dtype=np.int64)
    outside = (idx & ~support) != 0
    assert outside.sum() == (1 << n) - (1 << bin(support).count("1"))
    assert not got[outside].any(), f"{np.count_nonzero(got[outside])} non-zero amplitudes outside the support"
    assert abs(nv - float(np.sum(got.real * got.real + got.imag * got.imag))) < 1e-12
    at = np.zeros(32, dtype=np.int64)  # where index i of the 5-qubit register lies in the wide one
    for j, q in enumerate(FEW_QUBITS):
        at |= ((np.arange(32) >> j) & 1) << q
    want = np.zeros(1 << n, dtype=np.complex128)
    want[at] = replay(5, gates5, dtype=np.complex128)
    inside = ~outside
    if precision == 64:
        assert np.max(np.abs(got[inside] - want[inside])) < TOL
    else:
        ref32 = np.zeros(1 << n, dtype=np.complex64)
        ref32[at] = replay(5, gates5)
        report(f"zero_outside n={n}", check_fp32(got[inside], want[inside], ref32[inside]))
        assert np.max(np.abs(got[inside] - want[inside])) < TOL32


# ---- d. sampling over many blocks and few ------------------------------------------------------------------------------------------
def _draws(cumul, n):
    """300 uniform draws, the edge values, and for the first, second, a middle and the last two blocks the cumulative value at the
    block's end with both neighbours."""
    rng = np.random.default_rng(2000 + n)
    out = list(rng.uniform(0, 1, 300)) + [0.0, 1e-300, 1.0, 1.5]
    for b in (0, 1, 127, 254, 255):
        c = cumul[((b + 1) << sr.SAMPLE_BLOCK_BITS) - 1]
        out += [c, np.nextafter(c, -np.inf), np.nextafter(c, np.inf)]
    return np.array(out)


def _check_samples(oracle, cumul, n, draws, got, exact):
    """Each draw against oracle.measure.  exact: no difference at all.  Otherwise the rule of test_measurement_post_path, per
    draw: one index apart, and only when the draw is within 1e-13 of the cumulative value at one of the two indices."""
    for r, g in zip(draws, got):
        w = oracle.measure(cumul, n, float(r))
        if int(g) != w:
            assert not exact, (r, int(g), w)
            assert abs(int(g) - w) == 1 and min(abs(cumul[w] - r), abs(cumul[int(g)] - r)) < 1e-13, (r, int(g), w)


def _stored(sim, s, precision):
    """The state as the device holds it after write(s): s itself in fp64, its rounding widened again in fp32."""
    sim.write(s)
    stored = sim.read()
    assert np.array_equal(stored, s if precision == 64 else s.astype(np.complex64).astype(np.complex128))
    return stored


@pytest.mark.parametrize("precision", PRECISIONS)
def test_sampling_a_dense_state_over_many_blocks(oracle, precision):
    """n = 20, 256 blocks of k_block_prob: draws at, just below and just above block ends.  The reference cumulative is the
    oracle's over the stored state (in fp32: built in fp64 from the widened read())."""
    n = sr.SAMPLE_DENSE_N
    assert sr.launch("k_block_prob", n).tiles == 256
    with Simulator(n, precision=precision) as sim:
        stored = _stored(sim, sr.rand_state(n, 2001), precision)
        cumul = oracle.cumulative(stored, n)
        draws = _draws(cumul, n)
        _check_samples(oracle, cumul, n, draws, sim.sample(draws), exact=False)
        assert abs(sim.norm2() - float(np.sum(stored.real * stored.real + stored.imag * stored.imag))) < 1e-12


@pytest.mark.parametrize("precision", PRECISIONS)
def test_sampling_across_runs_of_zero_mass_blocks(oracle, precision):
    """n = 20, non-zero only in blocks 3, 200 and 201 (streaming_ref.zero_block_state): every probability is a multiple of
    2^-14, every partial sum exact in any order and in either precision, so every draw — those on block ends, r = 0 and r > 1
    included — owes the reference's answer exactly."""
    n = sr.SAMPLE_DENSE_N
    s = sr.zero_block_state(n)
    with Simulator(n, precision=precision) as sim:
        stored = _stored(sim, s, precision)
        assert np.array_equal(stored, s)  # exact in fp32 too
        cumul = oracle.cumulative(stored, n)
        assert cumul[-1] == 1.0
        draws = _draws(cumul, n)
        _check_samples(oracle, cumul, n, draws, sim.sample(draws), exact=True)
        assert abs(sim.norm2() - 1.0) < 1e-12


@pytest.mark.parametrize("n", sr.SAMPLE_SMALL_SIZES)
@pytest.mark.parametrize("precision", PRECISIONS)
def test_sampling_small_registers(oracle, precision, n):
    """Registers below one block of 2^12 amplitudes: the block is the whole register (k_block_prob's hi > N clamp)."""
    assert sr.launch("k_block_prob", n).tiles == 1
    with Simulator(n, precision=precision) as sim:
        stored = _stored(sim, sr.rand_state(n, 2100 + n), precision)
        cumul = oracle.cumulative(stored, n)
        draws = np.random.default_rng(2200 + n).uniform(0, 1, 20)
        _check_samples(oracle, cumul, n, draws, sim.sample(draws), exact=False)
        assert abs(sim.norm2() - float(np.sum(stored.real * stored.real + stored.imag * stored.imag))) < 1e-12


# ---- e. k_block_prob past its grid cap ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fuse", [0, 3])
@pytest.mark.parametrize("precision", PRECISIONS)
def test_sampling_past_the_block_grid_cap(precision, fuse):
    """n = 29: 2^17 blocks, k_block_prob's 65536 workgroups take two trips and half the mass lies in blocks only the second trip
    sums.  The state is |0...0> (over a stale dense state) with one 2x2 on each of qubits 28, 17, 12 and 3: sixteen non-zero
    amplitudes, known analytically.  Built at fuse 0, k_init loops over 2^29 amplitudes; at fuse 3 one tile pass generates the
    state inside its support and k_zero_outside loops over 2^29.  Draws are the midpoints between consecutive running
    probabilities (gaps >= 0.3^4, pinned on the CPU) and r = 0, each owed its analytic index exactly.
    r = 1 lies ON the last running value, which equals 1 only up to rounding: the sampler then answers either the last of the
    sixteen (the sum reached 1) or 2^n - 1 (it did not), as measurement() of the reference does; both are accepted for that one
    draw and nothing else is.  Nothing larger than one block is copied to the host."""
    n = sr.SAMPLE_LOOP_N
    N = 1 << n
    assert sr.launch("k_block_prob", n).max_trips >= 2
    assert sr.launch("k_init" if fuse == 0 else "k_zero_outside", n).max_trips >= 2
    idx, amps, _ = sr.sparse_state()
    draws, want, _ = sr.sparse_draws()
    gates = [("u1", q, U) for q, U in zip(sr.SPARSE_QUBITS, sr.sparse_matrices())]
    with Simulator(n, precision=precision) as sim:
        _dirty(sim, n)
        sim.set_option(_lib.OPT_FUSE, fuse)
        sim.reset_stats()
        for g in gates:
            _apply(sim, g)
        if fuse == 0:
            sim.flush()
            ran = _launches(sim)
            assert (ran["init"], ran["gate1"], ran["gate1_lo"], sum(ran.values())) == (1, 3, 1, 5), ran
        else:
            support, pending, _ = sim.get_support()
            assert not pending and support != N - 1
            ran = _launches(sim)
            assert ran["tile"] >= 1 and ran["tile"] == sum(ran.values()), ran
        got = sim.sample(np.concatenate([draws, [1.0]]))
        if fuse == 3:
            ran = _launches(sim)
            assert ran["init"] == 1 and ran["tile"] + 1 == sum(ran.values()), ran
        assert np.array_equal(got[:-1].astype(np.int64), want), (got, want)
        assert int(got[-1]) in (int(idx[-1]), N - 1), got[-1]
        assert abs(sim.norm2() - 1.0) < (1e-12 if precision == 64 else 1e-6)
        found = np.array([sim.read(int(i), 1)[0] for i in idx])
        for first, count in ((1, 7), (int(idx[1]) + 1, 64), (int(idx[8]) - 64, 64), (N - 64, 64), ((N >> 1) + (1 << 20), 4096)):
            assert not set(range(first, first + count)) & set(int(i) for i in idx)
            assert not sim.read(first, count).any(), first
    if precision == 64:
        assert np.max(np.abs(found - amps)) < TOL
    else:
        small = [("u1", 3 - j, U) for j, U in enumerate(sr.sparse_matrices())]  # qubits 28, 17, 12, 3 as 3, 2, 1, 0: same order
        report(f"sparse n={n} fuse={fuse}", check_fp32(found, amps, replay(4, small)))
        assert np.max(np.abs(found - amps)) < TOL32


# ---- f. k_pack below one work tile -------------------------------------------------------------------------------------------------
def _pattern(count, real):
    return ((np.arange(2 * count, dtype=np.float64) % 241.0 + 1.0) * 0.25).astype(real)


def _complex(flat, precision):
    return flat.view(np.complex128 if precision == 64 else np.complex64).astype(np.complex128)


@pytest.mark.parametrize("n", sr.PACK_SMALL_SIZES)
@pytest.mark.parametrize("precision", PRECISIONS)
def test_pack_below_one_work_tile(precision, n):
    """qsim_pack_bits and qsim_pack_bits_to at n = 2, 5, 9 (k_pack's sidx < N guard decides), 10 (exactly one work tile) and 11.
    Every destination lies inside a torch buffer between bands of 4096 amplitudes holding a fixed pattern; the layout is the
    index formula of test_pack_bits_layout and everything outside the destinations stays bit-identical."""
    import torch
    assert sr.launch("k_pack", n).guarded == (n <= 9)
    N, band = 1 << n, 4096
    real, amp_bytes = (np.float64, 16) if precision == 64 else (np.float32, 8)
    bits_view = np.uint64 if precision == 64 else np.uint32
    with Simulator(n, precision=precision) as sim:
        state = _stored(sim, sr.rand_state(n, 2300 + n), precision)
        sim.reset_stats()
        packs = 0
        for bits in sr.pack_bit_sets(n):
            want = state[sr.pack_src_index(n, bits)]
            nblk, blk = 1 << len(bits), N >> len(bits)
            # one buffer: band | packed state | band
            host = _pattern(2 * band + N, real)
            buf = torch.from_numpy(host.copy()).to("cuda")
            torch.cuda.synchronize()  # the fill runs on torch's stream, the pack on the engine's: order them
            sim.pack_bits(bits, buf.data_ptr() + amp_bytes * band)
            sim.sync()
            after = buf.cpu().numpy()
            assert np.array_equal(_complex(after[2 * band:2 * (band + N)], precision), want), bits
            for lo, hi in ((0, 2 * band), (2 * (band + N), after.size)):
                assert np.array_equal(after[lo:hi].view(bits_view), host[lo:hi].view(bits_view)), (bits, lo)
            # one destination per block, in reverse order, a band in front of each and one at the end
            starts = [band + (nblk - 1 - b) * (blk + band) for b in range(nblk)]
            total = nblk * (blk + band) + band
            host = _pattern(total, real)
            buf = torch.from_numpy(host.copy()).to("cuda")
            torch.cuda.synchronize()
            sim.pack_bits_to(bits, [buf.data_ptr() + amp_bytes * st for st in starts])
            sim.sync()
            after = buf.cpu().numpy()
            untouched = np.ones(2 * total, dtype=bool)
            for b, st in enumerate(starts):
                assert np.array_equal(_complex(after[2 * st:2 * (st + blk)], precision), want[b * blk:(b + 1) * blk]), (bits, b)
                untouched[2 * st:2 * (st + blk)] = False
            assert np.array_equal(after[untouched].view(bits_view), host[untouched].view(bits_view)), bits
            packs += 2
        ran = _launches(sim)
        assert ran["pack"] == packs == sum(ran.values()), ran


@pytest.mark.parametrize("precision", PRECISIONS)
def test_pack_tile_loop_takes_several_trips(precision):
    """n = 14 under grid_cap 3: three workgroups walk k_pack's sixteen work tiles in 6, 5 and 5 trips; bit-equal to the uncapped
    launch (one trip each) and to the index formula."""
    import torch
    n, bits = sr.LOOP_N, (1, 3, 4)
    assert sr.launch("k_pack", n, 0).max_trips == 1
    assert sr.launch("k_pack", n, 3).max_trips >= 2 and sr.launch("k_pack", n, 3).uneven
    tdt = torch.float64 if precision == 64 else torch.float32
    out = {}
    with Simulator(n, precision=precision) as sim:
        state = _stored(sim, sr.rand_state(n, 2400), precision)
        sim.reset_stats()
        for cap in (0, 3):
            sim.set_option(_lib.OPT_GRID_CAP, cap)
            dst = torch.full((1 << n, 2), float("nan"), dtype=tdt, device="cuda")
            torch.cuda.synchronize()
            sim.pack_bits(bits, dst.data_ptr())
            sim.sync()
            out[cap] = _complex(dst.cpu().numpy().reshape(-1), precision)
        assert _launches(sim)["pack"] == 2
    assert np.array_equal(out[0], state[sr.pack_src_index(n, bits)])
    assert np.array_equal(out[3], out[0]), f"{np.count_nonzero(out[3] != out[0])} amplitudes differ under grid_cap 3"
