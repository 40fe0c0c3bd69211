"""Every state call on a register past 2^32 amplitudes: n = 33 (64 GiB in fp32, 128 GiB in fp64), the smallest size at which an
amplitude index, a unit index, a byte offset, a qubit number and a mask all need the upper half of a 64-bit word.

The reference is tests/large_ref.py (restriction to 14 active qubits, the rest spectators in product states; pinned without a device by
tests/test_large_ref_cpu.py, which also shows that an index or mask that lost its upper half moves every case by 100 tolerances or more).
The state is prepared by apply_1q on every qubit — the gate path, oracle-checked and with an n = 33 test of its own — and the first test
checks the prepared state itself, so that a later failure points at the call under test.

Sizes.  fp32 always runs at n = 33.  fp64 runs at n = 33 where the free-memory rule of test_largest_sharded_config_on_virtual_shards
allows what the case allocates (free > allocation + total / 32), else at n = 32 with the active set's top qubits at 29 ... 31; the size
that ran is printed.  States are created with pingpong=0: the tile passes of the preparation stay in place and the memory a case takes
is what its calls need.

Bounds.  fp64 amplitudes: per sampled window ||got - want|| / ||want|| <= 1e-10 (the project's parity figure, relative: the amplitudes
of a unit state of 2^33 are about 1e-5).  fp64 scalars: 1e-10 times the scale of the quantity, as the features' own tests have it.  fp32:
error relative to the fp64 truth <= 8 max(the complex64 replay's own error, 2^-24), the replay capped at 1e-5 (tests/fp32_ref.py).
Sampling and measurement outcomes on dyadic states, zeros after a collapse and data movement are compared exactly."""
import time

import numpy as np
import pytest

import diagonal_ref
import fp32_ref
import large_ref as lr
from gpu_quantum_simulator_amd import Diagonal, Simulator, _lib, plans
from gpu_quantum_simulator_amd._lib import QsimError

pytestmark = pytest.mark.gpu
PRECISIONS = [32, 64]
N = 33


def _size(precision, state_buffers, other_bytes=0):
    """33, or for an fp64 case that the card cannot hold next to everything else, 32."""
    if precision == 32:
        return N
    import torch
    free_b, total_b = torch.cuda.mem_get_info()
    need = state_buffers * (16 << N) + other_bytes
    n = N if free_b > need + total_b // 32 else N - 1
    return n


def _prepared(n, precision, seed=1, **options):
    emb = lr.Embedding(n, seed)
    sim = Simulator(n, precision=precision, fuse=3, pingpong=0, **options)
    for q in range(n):
        sim.apply_1q(emb.prep_matrix(q), q)
    return emb, sim


def _starts(emb):
    return emb.small_start(), emb.small_start(np.complex64)


def _report(label, precision, n, what, value, t0=None):
    took = f", {time.perf_counter() - t0:.2f} s" if t0 is not None else ""
    print(f"large-registers {label} p{precision} n={n}: {what} {value:.3e}{took}")


def _check_values(got, want, ref32, precision, scale=1.0, fp32_scale=None):
    """A vector of scalars against the fp64 truth: fp64 max abs error <= 1e-10 scale; fp32 the relative rule with the replay's values.
    fp32_scale: what both fp32 errors are taken relative to in place of ||want|| — for an inner product the two states' norms, the
    scale Cauchy-Schwarz gives it (the overlap of two product states of 33 qubits is small and says nothing about its own error).
    Returns the error as a fraction of its bound."""
    got, want = np.asarray(got, dtype=np.complex128).reshape(-1), np.asarray(want, dtype=np.complex128).reshape(-1)
    assert got.shape == want.shape
    if precision == 64:
        err = float(np.max(np.abs(got - want)))
        assert err <= lr.TOL64 * scale, (err, lr.TOL64 * scale)
        return err / (lr.TOL64 * scale)
    ref32 = np.asarray(ref32, dtype=np.complex128).reshape(-1)
    if fp32_scale is None:
        e_ref, e_got = lr.rel_err(ref32, want), lr.rel_err(got, want)
    else:
        e_ref, e_got = float(np.linalg.norm(ref32 - want)) / fp32_scale, float(np.linalg.norm(got - want)) / fp32_scale
    assert e_ref <= fp32_ref.REF_CAP, e_ref
    bound = fp32_ref.C * max(e_ref, fp32_ref.FLOOR)
    assert e_got <= bound, (e_got, e_ref, bound)
    return e_got / bound


def _check_amps(sim, plan, want_of, ref32_of):
    """Every window of `plan` against want_of(indices) (complex128) and, for an fp32 state, ref32_of(indices) (the complex64 replay).
    Where the truth is exactly zero the state must hold the +0.0 bit pattern.  Returns the worst error as a fraction of its bound."""
    worst = 0.0
    for first, count in plan:
        idx = lr.window_indices(first, count)
        got, want = sim.read(first, count), want_of(idx)
        zero = want == 0
        assert not np.ascontiguousarray(got[zero]).view(np.uint64).any(), (first, "an amplitude that is zero by definition is not +0.0")
        if zero.all():
            continue
        if sim.precision == 64:
            e = lr.rel_err(got, want)
            assert e <= lr.TOL64, (first, e)
            worst = max(worst, e / lr.TOL64)
        else:
            e_ref = lr.rel_err(ref32_of(idx), want)
            assert e_ref <= fp32_ref.REF_CAP, (first, e_ref)
            bound = fp32_ref.C * max(e_ref, fp32_ref.FLOOR)
            e = lr.rel_err(got, want)
            assert e <= bound, (first, e, e_ref, bound)
            worst = max(worst, e / bound)
    return worst


def _check_state(sim, emb, plan, small64, small32):
    return _check_amps(sim, plan, lambda idx: emb.amps(small64, idx), lambda idx: emb.amps(small32, idx, np.complex64))


def _check_norm(sim, want, ref32):
    return _check_values([sim.norm2()], [want], [ref32], sim.precision)


def _norms(emb, small64, small32):
    return float(np.vdot(small64, small64).real), float(np.vdot(small32.astype(np.complex128), small32.astype(np.complex128)).real) * emb.spectator_norm2(np.complex64)


def _run_case(name, precision, buffers=1):
    """One case of large_ref.CASES: prepare, the steps before the checks, then every mutating step followed by the sampled amplitudes and
    the norm, then the queries.  Returns (simulator still open, embedding, plan, final small states) for what a test adds."""
    t0 = time.perf_counter()
    n = _size(precision, buffers)
    emb, sim = _prepared(n, precision)
    try:
        before, steps, queries = lr.CASES[name]
        plan = lr.case_plan(emb, name)
        s64, s32 = _starts(emb)
        for step in before:
            lr.gpu_apply(sim, step, emb.lab)
            s64, s32 = lr.ref_apply(s64, step), lr.ref_apply(s32, step, dtype=np.complex64)
        worst = _check_state(sim, emb, plan, s64, s32) if not steps else 0.0
        for k, step in enumerate(steps):
            if step[0] == "channel":
                want_pick, ref_pick = lr.channel_pick(s64, step), lr.channel_pick(s32.astype(np.complex128), step)
            elif step[0] == "postselect":
                want_w = lr.ref_scalars(s64, ("weight", step[1], step[2]))
                ref_w = lr.ref_scalars(s32.astype(np.complex128), ("weight", step[1], step[2])) * emb.spectator_norm2(np.complex64)
            out = lr.gpu_apply(sim, step, emb.lab)
            if step[0] == "channel":
                assert out[0] == want_pick[0], (name, k, out, want_pick)
                _check_values([out[1]], [want_pick[1]], [ref_pick[1]], precision)
            elif step[0] == "postselect":
                _check_values([out], want_w, ref_w, precision)
            s64, s32 = lr.ref_apply(s64, step), lr.ref_apply(s32, step, dtype=np.complex64)
            worst = max(worst, _check_state(sim, emb, plan, s64, s32))
            worst = max(worst, _check_norm(sim, *_norms(emb, s64, s32)))
        _report(name, precision, n, "amplitudes, worst error / bound", worst)
        wide32 = s32.astype(np.complex128)
        for query in queries:
            want = lr.ref_scalars(s64, query)
            ref32 = lr.ref_scalars(wide32, query) * (1.0 if query[0] == "purity" else emb.spectator_norm2(np.complex64))
            frac = _check_values(lr.gpu_scalars(sim, query, emb.lab), want, ref32, precision)
            worst = max(worst, frac)
        _report(name, precision, n, "with scalars, worst error / bound", worst, t0)
    except BaseException:
        sim.close()                                          # a failed case gives its memory back before the next one
        raise
    return sim, emb, plan, s64, s32


# ---- the prepared state, and the calls whose cases are lists of steps -----------------------------------------------------------------
@pytest.mark.parametrize("precision", PRECISIONS)
def test_prepared_state(precision):
    sim, emb, plan, s64, s32 = _run_case("prepared", precision)
    with sim:
        assert len(plan) >= 60 and sum(c for _, c in plan) >= 19000
        assert any(f < 1 << 32 < f + c for f, c in plan) and any(f < 1 << 31 < f + c for f, c in plan)
        assert {f >> (emb.n - 3) for f, _ in plan} == set(range(8))       # every value of the top three qubits


@pytest.mark.parametrize("precision", PRECISIONS)
def test_expectation(precision):
    strings = lr.expectation_strings(precision)
    xs = [lr.masks(t, lr.M)[0] for t in strings]
    assert xs.count(xs[0]) == 32 and xs[0] >> lr.T == 1 and 0 in xs and any(x >> (lr.T - 1) == 1 for x in xs)
    assert precision == 64 or (1 in xs and any(x & 1 and x != 1 for x in xs))
    sim, *_ = _run_case(f"expectation{precision}", precision)
    sim.close()


@pytest.mark.parametrize("precision", PRECISIONS)
def test_rotations(precision):
    sim, *_ = _run_case("rotations", precision)
    sim.close()


@pytest.mark.parametrize("precision", PRECISIONS)
def test_matrix(precision):
    sim, *_ = _run_case("matrix", precision)
    sim.close()


@pytest.mark.parametrize("precision", PRECISIONS)
def test_channel_and_scale(precision):
    sim, *_ = _run_case("channel", precision)
    sim.close()


@pytest.mark.parametrize("precision", PRECISIONS)
def test_qft_inside_the_active_set(precision):
    sim, *_ = _run_case("qft", precision, buffers=2)     # two digits: moving passes between the state and a second buffer
    sim.close()


@pytest.mark.parametrize("name", ["postselect", "postselect10"])
@pytest.mark.parametrize("precision", PRECISIONS)
def test_postselect(precision, name):
    sim, emb, plan, s64, s32 = _run_case(name, precision)
    with sim:
        before = [sim.read(f, c) for f, c in plan[-4:]]
        qubits, outcome = lr.CASES[name][1][-1][1:3]
        with pytest.raises(QsimError):                   # the outcome the last call ruled out has probability zero now
            sim.postselect(emb.qubits(qubits), outcome ^ 1)
        assert all(np.array_equal(np.ascontiguousarray(a).view(np.uint64), np.ascontiguousarray(sim.read(f, c)).view(np.uint64))
                   for a, (f, c) in zip(before, plan[-4:]))                # nothing was written


@pytest.mark.parametrize("precision", PRECISIONS)
def test_density_matrices(precision):
    sim, emb, plan, s64, s32 = _run_case("density", precision)
    with sim:
        for query in lr.CASES["density"][2]:                                # k = 10 runs in several slices (and blocks) at this size
            if query[0] == "sdm" and len(query[1]) == 10:
                qs = emb.qubits(query[1])
                p = plans.ok(plans.subsystem_density_plan(qs, emb.n, precision, k=10))
                assert p["path"] == 1 and p["slices"] > 1 and p["upper_blocks"] > 1, (qs, p["slices"], p["upper_blocks"])
        bits = [np.ascontiguousarray(sim.read(f, c)).view(np.uint64) for f, c in plan[:12]]
        wide32, worst = s32.astype(np.complex128), 0.0
        spectator = emb.spectators[-1]                                     # the highest spectator: 31 > q > 21
        for qubits in ([spectator, emb.n - 1], [0, spectator, emb.n - 1, emb.n - 2], [emb.n - 1, 0, 1, 3, 5, 9, spectator, emb.n - 2]):
            call = sim.reduced_density_matrix if len(qubits) <= 5 else sim.subsystem_density_matrix
            worst = max(worst, _check_values(call(qubits), emb.rdm(s64, qubits), emb.rdm(wide32, qubits) * emb.spectator_norm2(np.complex64), precision))
        _report("density with a spectator", precision, emb.n, "worst error / bound", worst)
        again = [np.ascontiguousarray(sim.read(f, c)).view(np.uint64) for f, c in plan[:12]]
        assert all(np.array_equal(a, b) for a, b in zip(bits, again))      # read-only sweeps: the state's bits are where they were


@pytest.mark.parametrize("precision", PRECISIONS)
def test_permutations_move_bits(precision):
    """The case's sampled checks, and bit for bit: four windows of the final state against the prepared state's amplitudes at the indices
    the composed permutations take them from, read before the first call."""
    n = _size(precision, 1)
    emb = lr.Embedding(n, 1)
    steps = lr.CASES["permutation"][1]
    plan = lr.sample_plan(n)
    windows = [plan[0], plan[1], plan[3] if n == N else plan[2], plan[20]]
    sources = []
    for first, count in windows:
        src = lr.window_indices(first, count)
        for step in reversed(steps):
            src = lr.perm_source(step, src, emb.lab)
        sources.append(src)
    sim, emb, plan, s64, s32 = _run_case("prepared", precision)
    with sim:
        t0 = time.perf_counter()
        held = [np.array([sim.read(int(j), 1)[0] for j in src]) for src in sources]
        worst = 0.0
        for step in steps:
            lr.gpu_apply(sim, step, emb.lab)
            s64, s32 = lr.ref_apply(s64, step), lr.ref_apply(s32, step, dtype=np.complex64)
            worst = max(worst, _check_state(sim, emb, plan, s64, s32), _check_norm(sim, *_norms(emb, s64, s32)))
        for (first, count), want in zip(windows, held):
            got = sim.read(first, count)
            assert np.array_equal(np.ascontiguousarray(got).view(np.uint64), np.ascontiguousarray(want).view(np.uint64)), first
        _report("permutation", precision, n, "amplitudes, worst error / bound; four windows bit for bit", worst, t0)


# ---- the whole register: the QFT of a basis state ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", PRECISIONS)
def test_qft_of_the_whole_register(precision):
    t0 = time.perf_counter()
    n = _size(precision, 2)
    j = (1 << (n - 1)) | (1 << (n - 2)) | 1
    plan = lr.sample_plan(n)
    with Simulator(n, precision=precision, fuse=3, pingpong=0) as sim:
        for q in (0, n - 2, n - 1):
            sim.apply_1q(lr.EXACT["x"], q)
        sim.apply_qft(list(range(n)))
        worst = _check_amps(sim, plan, lambda idx: lr.qft_basis_amps(n, j, idx), lambda idx: lr.qft_basis_amps32(n, j, idx))
        # the norm: fp64 1e-10; fp32 stated directly — each of the n butterfly stages of the transform rounds an amplitude once, by at
        # most 2^-24 of itself, so the squared norm moves by at most 2 n 2^-24 (the worst case, every rounding the same way)
        assert abs(sim.norm2() - 1.0) <= (lr.TOL64 if precision == 64 else 2 * n * fp32_ref.FLOOR)
        sim.apply_qft(list(range(n)), inverse=True)
        back = sim.read(j, 1)[0]
        bound = lr.TOL64 if precision == 64 else fp32_ref.C * fp32_ref.REF_CAP
        assert abs(back - 1.0) <= bound and abs(sim.norm2() - 1.0) <= bound, (back, bound)
        for first, count in plan[:8]:
            got = sim.read(first, count)
            got[lr.window_indices(first, count) == np.uint64(j)] = 0
            assert np.max(np.abs(got)) <= bound
        _report("qft of the whole register", precision, n, "worst error / bound", worst, t0)


# ---- dyadic states: exact sampling and measurement ----------------------------------------------------------------------------------------
def _dyadic(dy, precision, **options):
    sim = Simulator(dy.n, precision=precision, fuse=3, pingpong=0, **options)
    for g in dy.gates():
        if g[0] == "hh":
            sim.apply_2q(lr.HH, g[1], g[2])
        else:
            sim.apply_1q(lr.EXACT[g[0]], g[1])
    return sim


def _outcomes(indices, qubits):
    out = np.zeros(indices.shape, dtype=np.uint64)
    for j, q in enumerate(qubits):
        out |= ((indices >> np.uint64(q)) & np.uint64(1)) << np.uint64(j)
    return out


@pytest.mark.parametrize("variant", ["bit 7 fixed at 0", "top qubit fixed at 1"])
@pytest.mark.parametrize("precision", PRECISIONS)
def test_sampling_is_exact_on_dyadic_states(precision, variant):
    t0 = time.perf_counter()
    n = N                                     # one state buffer and 0.2 % of scratch: both precisions at full size
    dy = lr.Dyadic(n, 7, 0, phases=[("z", 3), ("s", n - 1), ("z", n - 2), ("s", 0)]) if variant.startswith("bit") else lr.Dyadic(n, n - 1, 1, phases=[("s", 5), ("z", n - 2)])
    numer2 = lr.sampling_numerators(n)
    draws, want = dy.draws(numer2), dy.index_for(numer2)
    assert np.count_nonzero(want >> np.uint64(n - 1)) > 100 and np.count_nonzero(want >> np.uint64(18) >= np.uint64(1024)) > 100   # groups >= 1024
    with _dyadic(dy, precision) as sim:
        for first, count in lr.sample_plan(n)[:6]:
            idx = lr.window_indices(first, count)
            assert np.array_equal(sim.read(first, count), dy.amp(idx)), first          # the state itself, exactly
        assert sim.norm2() == 1.0
        got = sim.sample_shots(draws=draws)
        assert np.array_equal(got, want), np.flatnonzero(got != want)[:8]
        qubits = [0, n - 2, n - 1, 9]
        assert np.array_equal(sim.sample_shots(draws=draws, qubits=qubits), _outcomes(want, qubits))
        for cap in (3, 1 << 30, 0):
            sim.set_option(_lib.OPT_GRID_CAP, cap)
            assert np.array_equal(sim.sample_shots(draws=draws), want), cap
        seeded = np.random.default_rng(5).random(2000)
        ks = np.maximum(np.ceil(seeded * 2.0 ** (n - 1)).astype(np.int64) - 1, 0)                     # exact: a double times a power of two
        values, counts = np.unique(_outcomes(dy.support_index(ks), [n - 2, n - 1, 1]), return_counts=True)
        assert sim.sample_counts(2000, [n - 2, n - 1, 1], seed=5) == {int(v): int(c) for v, c in zip(values, counts)}
    _report(f"sampling, {variant}", precision, n, "draws compared exactly:", float(draws.size), t0)


@pytest.mark.parametrize("precision", PRECISIONS)
def test_measurement_is_exact_on_dyadic_states(precision):
    t0 = time.perf_counter()
    n = N
    dy = lr.Dyadic(n, 7, 0, phases=[("z", 3), ("s", n - 1)])
    plan = lr.sample_plan(n)
    tol = lr.TOL64 if precision == 64 else fp32_ref.C * fp32_ref.FLOOR
    with _dyadic(dy, precision) as sim:
        # measure {top}: the draw 0.75 lies in the upper half of the running sum, where the top qubit reads 1
        outcome, p = sim.measure([n - 1], draw=0.75, return_probability=True)
        assert outcome == 1 and p == 0.5
        mask, bits, scale = 1 << (n - 1), 1 << (n - 1), 2.0 ** 0.5

        def want_of(idx):
            kept = (idx & np.uint64(mask)) == np.uint64(bits)
            return np.where(kept, dy.amp(idx) * scale, 0.0)

        def windows():
            rng = np.random.default_rng(13)
            inside = [(int(rng.integers(0, 1 << n)) & ~mask) | bits for _ in range(8)]           # windows that begin inside what was kept
            return plan[:16] + [(min(f, (1 << n) - lr.WINDOW), lr.WINDOW) for f in inside]

        def check():
            worst = 0.0
            for first, count in windows():
                idx = lr.window_indices(first, count)
                got, want = sim.read(first, count), want_of(idx)
                zero = want == 0
                assert not np.ascontiguousarray(got[zero]).view(np.uint64).any(), first     # the ruled-out part: +0.0, on both sides of 2^32
                if not zero.all():
                    worst = max(worst, lr.rel_err(got, want))
            assert worst <= tol, worst
            assert abs(sim.norm2() - 1.0) <= tol
            return worst

        worst = check()
        # post-select {0, top}, {top-2, top-1, top} and ten qubits with the top one: W is the outcome's probability given what was kept
        for qubits, outcome in (([0, n - 1], 0b10), ([n - 3, n - 2, n - 1], 0b101), ([1, 2, 4, 6, 8, 10, 12, n - 3, n - 2, n - 1], 0b1010110010)):
            fresh = [q for q in qubits if not (mask >> q) & 1]
            W = sim.postselect(qubits, outcome)
            assert abs(W - 2.0 ** -len(fresh)) <= tol * 2.0 ** -len(fresh), (qubits, W)
            for j, q in enumerate(qubits):
                mask |= 1 << q
                bits = (bits & ~(1 << q)) | (((outcome >> j) & 1) << q)
            scale *= 2.0 ** (0.5 * len(fresh))
            worst = max(worst, check())
        held = [np.ascontiguousarray(sim.read(f, c)).view(np.uint64) for f, c in plan[:8]]
        with pytest.raises(QsimError):
            sim.postselect([n - 1], 0)                                                     # probability zero: refused
        assert all(np.array_equal(a, np.ascontiguousarray(sim.read(f, c)).view(np.uint64)) for a, (f, c) in zip(held, plan[:8]))
        # reset {top, 0}: both were measured as 1 and 0; the x on the top qubit moves the state to the lower half
        assert sim.reset_qubits([n - 1, 0], draw=0.3) == 0b01
        upper = lambda idx: idx | np.uint64(1 << (n - 1))
        keep_mask, keep_bits = mask, bits & ~(1 << (n - 1))
        mask, bits = keep_mask, keep_bits
        for first, count in windows():
            idx = lr.window_indices(first, count)
            kept = (idx & np.uint64(keep_mask)) == np.uint64(keep_bits)
            want = np.where(kept, dy.amp(upper(idx)) * scale, 0.0)
            got = sim.read(first, count)
            assert not np.ascontiguousarray(got[want == 0]).view(np.uint64).any() and (not kept.any() or lr.rel_err(got, want) <= tol), first
    _report("measurement on a dyadic state", precision, n, "worst relative error", worst, t0)


# ---- gradients ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["plain", "controlled", "diagonal"])
@pytest.mark.parametrize("precision", PRECISIONS)
def test_energy_and_gradient(precision, name):
    t0 = time.perf_counter()
    table_bytes = (8 << N) if name == "diagonal" else 0
    n = _size(precision, 2, table_bytes)                         # the state and lambda, and the table
    steps, terms, obs = lr.GRADIENTS[name]
    emb, sim = _prepared(n, precision)
    s64, s32 = _starts(emb)
    diag = None
    with sim:
        try:
            if name == "diagonal":
                diag = Diagonal.from_terms(n, [(c, emb.text(t)) for c, t in lr.DIAG_TERMS])
            entries = [(s[1], diag) if s[0] == "diag" else (s[0], emb.text(s[1]), emb.qubits(s[2])) for s in steps]
            ham = [(c, emb.text(t)) for c, t in terms] + ([(obs[0], diag)] if obs else [])
            energy, grad = sim.energy_and_gradient(entries, ham)
            e64, g64, f64 = lr.gradient_ref(s64, name)
            e32, g32, _ = lr.gradient_ref(s32, name, dtype=np.complex64)
            k32 = emb.spectator_norm2(np.complex64)
            frac = _check_values(np.concatenate([[energy], grad]), np.concatenate([[e64], g64]), np.concatenate([[e32], g32]) * k32, precision,
                                 scale=lr.gradient_weight(name))
            # the state is left as the call found it, to rounding: there and back
            back32 = s32
            for sign in (1.0, -1.0):
                for s in (steps if sign > 0 else reversed(steps)):
                    step = ("diag_phase", sign * s[1], s[2]) if s[0] == "diag" else ("rotations", [(sign * s[0], s[1], s[2])])
                    back32 = lr.ref_apply(back32, step, dtype=np.complex64)
            worst = _check_state(sim, emb, lr.sample_plan(n), s64, back32)
            worst = max(worst, _check_norm(sim, *_norms(emb, s64, back32)))
            _report(f"gradient {name}", precision, n, "energy and gradient, error / bound", frac)
            _report(f"gradient {name}", precision, n, "the state afterwards, worst error / bound", worst, t0)
        finally:
            if diag is not None:
                diag.close()


# ---- diagonal tables -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", PRECISIONS)
def test_diagonal_tables(precision):
    t0 = time.perf_counter()
    n = _size(precision, 1, 8 << N)
    emb, sim = _prepared(n, precision)
    s64, s32 = _starts(emb)
    small = lr.diag_table(lr.M, lr.DIAG_TERMS)
    big_terms = [(c, emb.text(t)) for c, t in lr.DIAG_TERMS]
    assert any(lr.masks(t, n)[1] >> (n - 1) for _, t in big_terms)
    with sim, Diagonal.from_terms(n, big_terms[:3]) as diag:
        diag.add_terms(big_terms[3:])
        plan = lr.sample_plan(n)
        for first, count in plan:
            assert np.array_equal(diag.read(first, count), small[emb.small_index(lr.window_indices(first, count))]), first   # the sequential sum, bit for bit
        ex, want = diag.extrema(), diagonal_ref.extrema(small)
        assert ex["min"] == want["min"] and ex["max"] == want["max"]
        assert ex["argmin"] == min(lr.deposit_on_active(emb, p) for p in np.flatnonzero(small == want["min"]))
        assert ex["argmax"] == min(lr.deposit_on_active(emb, p) for p in np.flatnonzero(small == want["max"]))
        first = (1 << (n - 1)) + 12345                                    # a window above entry 2^32: write, read, put back
        kept = diag.read(first, 1000)
        values = np.random.default_rng(3).standard_normal(1000)
        diag.write(values, first)
        assert np.array_equal(diag.read(first, 1000), values) and np.array_equal(diag.read(first - 8, 8), small[emb.small_index(lr.window_indices(first - 8, 8))])
        assert np.array_equal(diag.read(12345, 4), small[emb.small_index(lr.window_indices(12345, 4))])   # and nothing 2^32 entries below it
        diag.write(kept, first)
        m64, m32 = diagonal_ref.moments(s64, small), np.array(diagonal_ref.moments(s32.astype(np.complex128), small)) * emb.spectator_norm2(np.complex64)
        scale = float(np.max(np.abs(small))) ** 2
        frac = _check_values(sim.expectation_diagonal(diag, moments=True), m64, m32, precision, scale=scale)
        step = ("diag_phase", 0.37, lr.DIAG_TERMS)
        sim.apply_diagonal_phase(diag, 0.37)
        s64, s32 = lr.ref_apply(s64, step), lr.ref_apply(s32, step, dtype=np.complex64)
        worst = _check_state(sim, emb, plan, s64, s32)
        worst = max(worst, _check_norm(sim, *_norms(emb, s64, s32)))
        _report("diagonal", precision, n, "<D> and <D^2>, error / bound", frac)
        _report("diagonal", precision, n, "the phase, worst error / bound", worst, t0)


@pytest.mark.parametrize("precision", PRECISIONS)
def test_diagonal_into(precision):
    t0 = time.perf_counter()
    n = _size(precision, 2, 8 << N)
    emb, sim = _prepared(n, precision)
    s64, s32 = _starts(emb)
    small = lr.diag_table(lr.M, lr.DIAG_TERMS)
    real = np.float64 if precision == 64 else np.float32
    with sim, Simulator(n, precision=precision, pingpong=0) as dst, Diagonal.from_terms(n, [(c, emb.text(t)) for c, t in lr.DIAG_TERMS]) as diag:
        plan = lr.sample_plan(n)
        sim.diagonal_into(diag, dst.device_ptr, 0.8)
        sim.sync()
        w64, w32 = (0.8 * small) * s64, ((np.float64(0.8) * small).astype(real) * s32).astype(np.complex64)
        worst = max(_check_state(dst, emb, plan, w64, w32), _check_norm(dst, *_norms(emb, w64, w32)))
        sim.diagonal_into(diag, dst.device_ptr, -0.5, accumulate=True)
        sim.sync()
        w64, w32 = w64 + (-0.5 * small) * s64, (w32 + ((np.float64(-0.5) * small).astype(real) * s32).astype(np.complex64)).astype(np.complex64)
        worst = max(worst, _check_state(dst, emb, plan, w64, w32), _check_norm(dst, *_norms(emb, w64, w32)))
        worst = max(worst, _check_state(sim, emb, plan[:8], s64, s32), _check_norm(sim, *_norms(emb, s64, s32)))   # the source is only read
        _report("diagonal_into", precision, n, "worst error / bound", worst, t0)


# ---- state algebra -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", PRECISIONS)
def test_state_algebra(precision):
    t0 = time.perf_counter()
    n = _size(precision, 3)
    emb1, sim1 = _prepared(n, precision, seed=1)
    emb2, sim2 = _prepared(n, precision, seed=2)
    plan = lr.sample_plan(n)
    psi1, psi2 = lr.Mix.of(emb1), lr.Mix.of(emb2)
    seq, g = lr.algebra_sequence(psi1, psi2), lr.ALGEBRA
    inner = lambda x, y, mx, my: _check_values([x.inner(y)], [mx.inner(my)], [mx.inner(my, wide32=True)], precision,
                                               fp32_scale=float(np.sqrt(mx.inner(mx).real * my.inner(my).real)))

    def check(sim, mix):      # the sampled amplitudes and the norm
        norm = _check_values([sim.norm2()], [mix.inner(mix).real], [mix.inner(mix, wide32=True).real], precision, scale=mix.inner(mix).real)
        return max(_check_amps(sim, plan, mix.amps, mix.amps32), norm)

    with sim1, sim2, Simulator(n, precision=precision, pingpong=0) as sim3:
        worst = max(check(sim1, psi1), check(sim2, psi2), inner(sim1, sim2, psi1, psi2), inner(sim2, sim2, psi2, psi2))
        sim3.copy_from(sim1)                                                           # data movement: bit for bit
        for first, count in plan:
            assert np.array_equal(np.ascontiguousarray(sim3.read(first, count)).view(np.uint64), np.ascontiguousarray(sim1.read(first, count)).view(np.uint64))
        sim3.scale(g["s"])
        worst = max(worst, check(sim3, seq["scaled copy"]))
        norm2 = sim1.combine(g["d"], (g["a"], sim2), (g["b"], sim3), norm=True)         # three streams and the norm from the same sweep
        psi1 = seq["combined"]
        worst = max(worst, check(sim1, psi1))
        worst = max(worst, _check_values([norm2], [psi1.inner(psi1).real], [psi1.inner(psi1, wide32=True).real], precision, scale=psi1.inner(psi1).real))
        assert sim2.combine(0.0, (g["c"], sim1)) is None                               # d == 0: overwritten without being read; two streams
        psi2 = seq["overwritten"]
        worst = max(worst, check(sim2, psi2), inner(sim1, sim2, psi1, psi2), inner(sim3, sim2, seq["scaled copy"], psi2))
        sim2.pauli_sum_into([(co, emb1.text(t)) for co, t in lr.HAMILTONIAN], sim3.device_ptr)
        sim2.sync()
        worst = max(worst, check(sim3, seq["pauli sum"]), check(sim2, psi2))
        _report("state algebra", precision, n, "worst error / bound", worst, t0)


@pytest.mark.parametrize("precision", PRECISIONS)
def test_ground_state_for_a_few_steps(precision):
    """Four Lanczos steps from the prepared state for H inside the active set: every Krylov vector stays a product with the spectators, so
    alphas, betas, the Ritz value and the Ritz vector are those of the 14-qubit problem (lanczos_ref).  The solver takes three work
    buffers of the state's size beside the state."""
    t0 = time.perf_counter()
    n = _size(precision, 4)
    emb, sim = _prepared(n, precision)
    s64, s32 = _starts(emb)
    with sim:
        got = sim.ground_state([(c, emb.text(t)) for c, t in lr.HAMILTONIAN], 1e-12, max_steps=lr.LANCZOS_STEPS, vector=True)
        want, ref32 = lr.ground_state_ref(s64), lr.ground_state_ref(s32, np.complex64)
        assert got["steps"] == want["steps"] == lr.LANCZOS_STEPS
        pack = lambda r: np.concatenate([[r["energy"], r["residual"]], r["alphas"], r["betas"]])
        weight = sum(abs(c) for c, _ in lr.HAMILTONIAN)
        frac = _check_values(pack(got), pack(want), pack(ref32), precision, scale=weight)
        # a Ritz vector is defined up to its sign (the eigenvector of the tridiagonal is): both references take the device's
        y64, y32 = want["y"], ref32["y"]
        head = lr.window_indices(0, lr.WINDOW)
        y64 = y64 * np.sign(np.vdot(emb.amps(y64, head), sim.read(0, lr.WINDOW)).real)
        y32 = (y32 * np.float32(np.sign(np.vdot(y64, y32.astype(np.complex128)).real))).astype(np.complex64)
        worst = _check_state(sim, emb, lr.sample_plan(n), y64, y32)
        worst = max(worst, _check_norm(sim, *_norms(emb, y64, y32)))
        _report("ground_state", precision, n, "energy, residual, alphas, betas: error / bound", frac)
        _report("ground_state", precision, n, "the Ritz vector, worst error / bound", worst, t0)


def _matrix_path(targets, controls, n, precision):
    return plans.ok(plans.apply_matrix_plan(targets, controls, n, precision))["path"]


@pytest.mark.parametrize("precision", PRECISIONS)
def test_matrix_off_the_matrix_path(precision):
    """apply_matrix under 29 controls — every spectator and ten active qubits: 16 amplitudes are written, fewer environments than a step
    of the matrix path takes, so the plain kernel runs (the plan probe says which; the steps of test_matrix all take the matrix path).
    Where every spectator bit is 1 the state is the spectators' factor times the small state after the small step, elsewhere unchanged."""
    t0 = time.perf_counter()
    n = _size(precision, 1)
    emb, sim = _prepared(n, precision)
    s64, s32 = _starts(emb)
    (U, targets, controls), small = lr.plain_matrix_step(emb)
    assert _matrix_path(targets, controls, n, precision) == 0
    assert all(_matrix_path(emb.qubits(st[2]), emb.qubits(st[3]), n, precision) == 1 for st in lr.CASES["matrix"][1])
    with sim:
        sim.apply_matrix(U, targets, controls)
        on64, on32 = lr.ref_apply(s64, small), lr.ref_apply(s32, small, dtype=np.complex64)
        want_of = lambda idx: lr.plain_matrix_amps(emb, s64, on64, idx)
        ref_of = lambda idx: lr.plain_matrix_amps(emb, s32, on32, idx, np.complex64)
        written = lr.plain_matrix_indices(emb)
        got = np.array([sim.read(int(j), 1)[0] for j in written])
        frac = _check_values(got, want_of(written), ref_of(written), precision, scale=float(np.max(np.abs(want_of(written)))))
        assert lr.rel_err(want_of(written), emb.amps(s64, written)) > 0.1          # the step moved what it wrote
        worst = _check_amps(sim, lr.sample_plan(n), want_of, ref_of)               # and nothing else
        worst = max(worst, _check_norm(sim, *_norms(emb, s64, s32)))
        _report("matrix, plain kernel", precision, n, "the 16 amplitudes written, error / bound", frac)
        _report("matrix, plain kernel", precision, n, "everything else, worst error / bound", worst, t0)
