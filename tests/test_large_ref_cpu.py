"""Pins tests/large_ref.py, the reference of tests/test_gpu_large_registers.py, without a device.

1. The restriction: at n = 16, where numpy holds the state, every case runs densely through the features' checkers on the whole register
   and restricted to the active set; the scalars and `Embedding.amps` must agree to 1e-13.
2. The reach: for every GPU case at n = 33 the reference is evaluated under the fault models of large_ref (an index truncated to 32
   bits or sign-extended from bit 31, a mask without bit 32, a shift count mod 32, a partner index with x truncated, a truncated unit
   index); at least one checked quantity must move by 100 tolerances — of the fp64 bound 1e-10 AND of the largest bound an fp32 run
   can be given, 8 * 1e-5 (fp32_ref.C * REF_CAP).  For the exact sampling cases the returned index must differ.
3. The host geometry of the calls at n = 33 ... 40 from the plan probes: nothing wrapped."""

import numpy as np
import pytest

import fp32_ref
import large_ref as lr
import qft_ref
import sample_ref
from gpu_quantum_simulator_amd import plans
from helpers import np_apply_1q, np_apply_2q

N_PIN = 16
TOL_PIN = 1e-13
FP32_WORST_BOUND = fp32_ref.C * fp32_ref.REF_CAP


def _dense_start(emb):
    s = np.ones(1, dtype=np.complex128)
    for q in reversed(range(emb.n)):
        s = np.kron(s, np.array([emb.alpha[q], emb.beta[q]]))
    return s


@pytest.fixture(scope="module")
def pin():
    emb = lr.Embedding(N_PIN, 5)
    return emb, _dense_start(emb), emb.small_start()


def test_active_sets_hold_the_ends_of_the_register():
    for n in (16, 32, 33):
        a = lr.active_set(n)
        assert len(a) == lr.M == 14 and {0, 1, n - 3, n - 2, n - 1} <= set(a) and len(set(a)) == 14
    emb = lr.Embedding(33, 1)
    r = np.abs(emb.beta / emb.alpha)
    assert np.all((r >= lr.RATIO[0]) & (r <= lr.RATIO[1])) and np.allclose(np.abs(emb.alpha) ** 2 + np.abs(emb.beta) ** 2, 1.0)
    u = emb.prep_matrix(32)
    assert np.allclose(u.conj().T @ u, np.eye(2)) and u[0, 0] == emb.alpha[32] and u[1, 0] == emb.beta[32]
    assert len(set(np.round(np.angle(emb.beta / emb.alpha), 6))) == 33  # distinct phases


@pytest.mark.parametrize("name", sorted(lr.CASES))
def test_restriction_holds_where_numpy_holds_the_state(pin, name):
    emb, dense0, small0 = pin
    every = np.arange(1 << N_PIN, dtype=np.uint64)
    assert np.max(np.abs(emb.amps(small0, every) - dense0)) < TOL_PIN
    dense_states, dense_scalars = lr.run_case(name, dense0, emb.lab)
    small_states, small_scalars = lr.run_case(name, small0)
    for d, s in zip(dense_states, small_states):
        assert np.max(np.abs(emb.amps(s, every) - d)) < TOL_PIN, name
    for d, s in zip(dense_scalars, small_scalars):
        assert d.shape == s.shape and np.max(np.abs(d - s)) < TOL_PIN, name
    for k, step in enumerate(lr.CASES[name][1]):
        if step[0] == "channel":
            i_d, p_d = lr.channel_pick(dense_states[k], step, emb.lab)
            i_s, p_s = lr.channel_pick(small_states[k], step)
            assert i_d == i_s and abs(p_d - p_s) < TOL_PIN


def test_density_matrices_with_a_spectator(pin):
    import density_ref
    emb, dense0, small0 = pin
    dense = lr.ref_apply(dense0, lr.ENTANGLE, emb.lab)
    small = lr.ref_apply(small0, lr.ENTANGLE)
    for qubits in ([2], [15, 2, 0], [7, 13, 14, 15], [0, 1, 2, 3, 4, 5, 6, 15], [15, 14, 7, 12, 11, 10, 9, 8, 6, 5]):
        assert sum(q in emb.spectators for q in qubits) == 1
        assert np.max(np.abs(emb.rdm(small, qubits) - density_ref.reduced_density(dense, qubits))) < TOL_PIN


@pytest.mark.parametrize("name", sorted(lr.GRADIENTS))
def test_gradients_restrict(pin, name):
    emb, dense0, small0 = pin
    e_d, g_d, f_d = lr.gradient_ref(dense0, name, emb.lab)
    e_s, g_s, f_s = lr.gradient_ref(small0, name)
    assert abs(e_d - e_s) < TOL_PIN and np.max(np.abs(g_d - g_s)) < TOL_PIN
    small33 = lr.Embedding(33, 1).small_start()
    assert np.min(np.abs(lr.gradient_ref(small33, name)[1])) > 1e-3   # the GPU test's own start state: no component is zero by accident
    assert np.max(np.abs(emb.amps(f_s, np.arange(1 << N_PIN, dtype=np.uint64)) - f_d)) < TOL_PIN


def test_diagonal_tables_and_inner_products_restrict(pin):
    import diagonal_ref
    emb, dense0, small0 = pin
    other = lr.Embedding(N_PIN, 6)
    dense1, small1 = _dense_start(other), other.small_start()
    assert abs(np.vdot(dense0, dense1) - np.vdot(small0, small1) * emb.spectator_inner(other)) < TOL_PIN
    big, small = lr.diag_table(N_PIN, lr.DIAG_TERMS, emb.lab), lr.diag_table(lr.M, lr.DIAG_TERMS)
    every = np.arange(1 << N_PIN, dtype=np.uint64)
    assert np.array_equal(big, small[emb.small_index(every)])
    assert np.allclose(diagonal_ref.moments(dense0, big), diagonal_ref.moments(small0, small), rtol=0, atol=TOL_PIN)
    assert diagonal_ref.extrema(big)["min"] == diagonal_ref.extrema(small)["min"]
    step = ("diag_phase", 0.37, lr.DIAG_TERMS)
    assert np.max(np.abs(emb.amps(lr.ref_apply(small0, step), every) - lr.ref_apply(dense0, step, emb.lab))) < TOL_PIN


def test_complex64_replay_stays_under_the_reference_cap():
    emb = lr.Embedding(33, 1)
    for name in sorted(lr.CASES):
        windows = [lr.window_indices(*w) for w in lr.case_plan(emb, name)]
        s64, _ = lr.run_case(name, emb.small_start())
        s32, _ = lr.run_case(name, emb.small_start(np.complex64), dtype=np.complex64)
        for a, b in zip(s64, s32):
            assert b.dtype == np.complex64
            worst = max(lr.rel_err(emb.amps(b, idx, np.complex64), emb.amps(a, idx)) for idx in windows)   # window by window, as the GPU test checks
            assert 0 < worst <= fp32_ref.REF_CAP / 4, (name, worst)


# ---- closed forms ---------------------------------------------------------------------------------------------------------------------
def test_qft_of_a_basis_state_closed_form():
    n, j = 10, 0b1000010011
    s = np.zeros(1 << n, dtype=np.complex128)
    s[j] = 1
    idx = np.arange(1 << n, dtype=np.uint64)
    for inverse in (False, True):
        assert np.max(np.abs(lr.qft_basis_amps(n, j, idx, inverse) - qft_ref.apply_qft(s, list(range(n)), inverse=inverse))) < TOL_PIN
    big = lr.qft_basis_amps(33, (1 << 32) | (1 << 31) | 1, np.array([0, 1, (1 << 32) + 5, (1 << 33) - 1], dtype=np.uint64))
    assert np.allclose(np.abs(big), 2.0 ** -16.5, rtol=1e-15) and abs(big[1] - 2.0 ** -16.5 * np.exp(2j * np.pi * (0.75 + 2.0 ** -33))) < 1e-19


@pytest.mark.parametrize("fixed,value", [(7, 0), (3, 1), (14, 1)])
def test_dyadic_states_by_brute_force(fixed, value):
    n = 15
    dy = lr.Dyadic(n, fixed, value, phases=[("z", 2), ("s", n - 1 if fixed != n - 1 else 0), ("z", 9)])
    s = np.zeros(1 << n, dtype=np.complex128)
    s[0] = 1
    for g in dy.gates():
        s = np_apply_2q(s, n, lr.HH, g[1], g[2]) if g[0] == "hh" else np_apply_1q(s, n, lr.EXACT[g[0]], g[1])
    assert np.array_equal(dy.amp(np.arange(1 << n, dtype=np.uint64)), s)    # exact: every factor is a power of two, +-1 or +-i
    half = 1 << (n - 1)
    numer2 = np.array([0, 1, 2, 3, 4, 2 * half - 1, 2 * half, half - 1, half, half + 1, 2 * 777 + 1, 2 * 778], dtype=np.int64)
    draws = dy.draws(numer2)
    exact = dy.amp(np.arange(1 << n, dtype=np.uint64))
    assert np.array_equal(dy.index_for(numer2), sample_ref.brute_force(exact, draws))


# ---- the reach of the GPU cases -----------------------------------------------------------------------------------------------------------
def _reach(n, amps_of, plan):
    """fault -> the largest per-window relative move of amps_of(indices) when the indices go through the fault."""
    moved = {}
    for name, fault in lr.index_faults(n).items():
        moved[name] = max(lr.rel_err(amps_of(fault(lr.window_indices(f, c))), amps_of(lr.window_indices(f, c))) for f, c in plan)
    return moved


def _amplitude_reach(emb, states, plan):
    out = {}
    for small in states:
        for k, v in _reach(emb.n, lambda idx: emb.amps(small, idx), plan).items():
            out[k] = max(out.get(k, 0.0), v)
    return out


def _scalar_reach(small, queries):
    moved = {}
    for name, fault in lr.label_faults().items():
        best = 0.0
        for q in queries:
            want = lr.ref_scalars(small, q)
            best = max(best, float(np.linalg.norm(lr.faulty_scalars(small, q, fault) - want) / np.linalg.norm(want)))
        moved[name] = best
    return moved


def _reach_table():
    """(case of the GPU file, {fault or quantity: relative move}) for EVERY test of tests/test_gpu_large_registers.py but the two exact
    sampling ones, which test_reach_of_the_exact_sampling_cases covers."""
    n = 33
    emb, emb2 = lr.Embedding(n, 1), lr.Embedding(n, 2)
    plan = lr.sample_plan(n)
    start = emb.small_start()
    drop_top = lambda m: m & ~(1 << lr.T)   # every mask of a call without bit 32
    for name in sorted(lr.CASES):
        states, _ = lr.run_case(name, start)
        queries = [q for q in lr.CASES[name][2] if q[0] != "norm2"]
        moved = _amplitude_reach(emb, states[1:] if len(states) > 1 else states, lr.case_plan(emb, name))   # (a scalar case checks its state too)
        if queries:
            moved.update({f"scalars: {k}": v for k, v in _scalar_reach(states[-1], queries).items()})
        yield name, moved
    for name in sorted(lr.GRADIENTS):
        e, g, final = lr.gradient_ref(start, name)
        e2, g2, _ = lr.gradient_ref(start, name, fix=drop_top)
        want = np.concatenate([[e], g])
        moved = _amplitude_reach(emb, [start, final], plan)      # the state afterwards (the start again) and on the way
        moved["energy and gradient: mask bit 32 dropped"] = float(np.linalg.norm(np.concatenate([[e2], g2]) - want) / np.linalg.norm(want))
        yield f"gradient {name}", moved
    psi1, psi2 = lr.Mix.of(emb), lr.Mix.of(emb2)
    for label, mix in [("start 1", psi1), ("start 2", psi2)] + list(lr.algebra_sequence(psi1, psi2).items()):
        yield f"state algebra, {label}", _reach(n, mix.amps, plan)
    table = lr.diag_table(lr.M, lr.DIAG_TERMS)
    yield "diagonal tables, the table", _reach(n, lambda idx: table[emb.small_index(idx)], plan)
    yield "diagonal tables, the phase", _amplitude_reach(emb, [lr.ref_apply(start, ("diag_phase", 0.37, lr.DIAG_TERMS))], plan)
    yield "diagonal_into", _amplitude_reach(emb, [(0.8 * table) * start, (0.3 * table) * start], plan)
    j = (1 << 32) | (1 << 31) | 1
    yield "qft of the whole register", _reach(n, lambda idx: lr.qft_basis_amps(n, j, idx), plan[:12])
    dy = lr.Dyadic(n, 7, 0, phases=[("z", 3), ("s", n - 1)])
    top = np.uint64(1 << (n - 1))
    yield "measurement on a dyadic state", _reach(n, lambda idx: np.where(idx & top, dy.amp(idx) * 2.0 ** 0.5, 0.0), plan)
    yield "ground_state", _amplitude_reach(emb, [lr.ground_state_ref(start)["y"]], plan)
    _, small_step = lr.plain_matrix_step(emb)
    on = lr.ref_apply(start, small_step)
    written = lr.plain_matrix_indices(emb)
    yield "matrix, plain kernel", _reach(n, lambda idx: lr.plain_matrix_amps(emb, start, on, idx), [(int(w), 1) for w in written] + plan[:8])


def test_reach_of_every_case():
    need = lr.REACH * max(lr.TOL64, FP32_WORST_BOUND)
    smallest, seen = float("inf"), []
    for name, moved in _reach_table():
        best = max(moved.values())
        smallest = min(smallest, best / need)
        seen.append(name)
        print(f"reach {name}: " + ", ".join(f"{k} {v:.3g}" for k, v in moved.items()) + f"; margin {best / need:.3g} x the need")
        assert best >= need, (name, moved)
        assert all(v >= need for k, v in moved.items() if k.startswith("index") or k.startswith("unit")), (name, moved)
    assert len(seen) == len(lr.CASES) + len(lr.GRADIENTS) + 6 + 7   # six states of the algebra test, seven more tests
    print(f"reach: {len(seen)} cases, the smallest margin is {smallest:.3g} x (100 tolerances)")


def test_reach_of_the_exact_sampling_cases():
    n = 33
    for dy in (lr.Dyadic(n, 7, 0), lr.Dyadic(n, n - 1, 1)):
        numer2 = lr.sampling_numerators(n)
        want = dy.index_for(numer2)
        assert np.count_nonzero(want >= np.uint64(1 << 32)) > 100 and (dy.fixed == n - 1 or np.count_nonzero(want < np.uint64(1 << 32)) > 100)
        for name, fault in lr.index_faults(n).items():
            if name == "partner with x truncated" and dy.fixed == n - 1:
                continue  # (that variant's indices all have the top bit)
            assert np.count_nonzero(fault(want) != want) > 0, name


# ---- host geometry at n = 33 ... 40: every plan probe, no device ----------------------------------------------------------------------
SIZES = range(33, 41)
PRECISIONS = [64, 32]


def _state_units(n, precision):
    """16-byte units of a state: one fp64 amplitude, two fp32 amplitudes."""
    return (1 << n) if precision == 64 else (1 << (n - 1))


def _ceil_div(a, b):
    return -(-a // b)


def _doubles(values, what):
    """A count over n = 33 ... 40 that is proportional to the register doubles from one size to the next: a field that wrapped does not."""
    for a, b in zip(values, values[1:]):
        assert a > 0 and 2 * a - 1 <= b <= 2 * a, (what, values)   # (a count rounded up may double to one less)


def _subsets(n):
    return [[n - 1], [0, n - 1], [n - 3, n - 2, n - 1], [1, 13, n - 2, n - 1], [0, 5, 21, n - 2, n - 1]]


def test_pauli_plans_take_masks_above_bit_31():
    for n in SIZES:
        top, below = 1 << (n - 1), 1 << (n - 2)
        xs = [top | 1, top | 1, top | 1, below | 2, 0, top]
        zs = [0, top, below, top, top | 1, top]
        p = plans.ok(plans.pauli_rotation_plan(xs, zs))
        # three strings share x (one sweep), the fourth has another, x = 0 is a sweep of its own kind, the last is a single-qubit Y: a gate
        assert p["sweeps"] == 3 and p["queued_as_gates"] == 1, (n, p)
        # x strings that differ ONLY above bit 31 do not share a sweep: the plan compares 64-bit masks
        assert plans.ok(plans.pauli_rotation_plan([top | 1, (top >> 1) | 1, top | 1], [2, 2, 2])) == dict(sweeps=3, queued_as_gates=0)
        g = plans.ok(plans.pauli_gradient_plan(xs, xs[:4]))
        assert g["adjoint_sweeps"] > 0 and g["sum_sweeps"] == 2   # H's strings: two distinct x


@pytest.mark.parametrize("precision", PRECISIONS)
def test_controlled_plans_visit_the_control_subspace(precision):
    seen = []
    for n in SIZES:
        top = 1 << (n - 1)
        for cs, xs, zs, share in (([top], [1 | 4], [2], 2), ([top | (top >> 1)], [8], [0], 4), ([2], [top | 4], [top >> 1], 2)):
            p = plans.ok(plans.controlled_rotation_plan(cs, xs, zs, n, precision))
            assert p["sweeps"] + p["queued_as_gates"] == 1
            # every control bit 1 and the highest bit of x clear (tests/test_controlled_rot_cpu.py enumerates it at n = 10)
            assert p["sweeps"] == 1 and p["units_visited"] == _state_units(n, precision) // (2 * share), (n, cs, p["units_visited"])
            g = plans.ok(plans.controlled_gradient_plan(cs, xs, [top | 1], n, precision))
            assert g["adjoint_sweeps"] == 1 and g["sum_sweeps"] == 1 and g["units_visited"] == _state_units(n, precision) // (2 * share)
        seen.append(p["units_visited"])
    _doubles(seen, "controlled rotation units")


@pytest.mark.parametrize("precision", PRECISIONS)
def test_density_plans_read_the_whole_state(precision):
    trips, reads = [], []
    for n in SIZES:
        for qubits in _subsets(n):
            p = plans.ok(plans.reduced_density_plan(qubits, n, precision))
            assert p["units_visited"] == _state_units(n, precision) and p["trips_per_workgroup_at_grid_cap"] > 0
            want, mask = sum(1 << q for q in qubits), p["kernel_mask"]
            assert mask & want == want and mask >> n == 0 and bin(mask).count("1") == p["padded_k"]
        trips.append(p["trips_per_workgroup_at_grid_cap"])
        for qubits in ([0, 1, 2, 3, n - 2, n - 1], [1, 2, 3, 4, 5, 6, 7, 8, 9, n - 1], list(range(n - 10, n))):
            p = plans.ok(plans.subsystem_density_plan(qubits, n, precision))
            assert p["path"] == 1 and p["block_rows"] == 128 and p["upper_blocks"] > 0 and p["slices"] > 0 and p["trips_per_workgroup"] > 0 and p["scratch_bytes"] > 0
            assert len(qubits) < 10 or (p["slices"] > 1 and p["upper_blocks"] > 1)                                    # k = 10: several slices
            read = p["units_read"]
            assert read % _state_units(n, precision) == 0 and read // _state_units(n, precision) >= 1               # whole state volumes
        reads.append(read)
    _doubles(trips, "reduced density trips")
    _doubles(reads, "subsystem density units read")


@pytest.mark.parametrize("precision", PRECISIONS)
def test_matrix_and_permutation_plans_cover_the_control_subspace(precision):
    m_trips, p_trips, p_tiles = [], [], []
    for n in SIZES:
        for targets in _subsets(n):
            for controls in ([], [n - 4], [2, n - 4]):
                m = plans.ok(plans.apply_matrix_plan(targets, controls, n, precision))
                assert m["units"] == _state_units(n, precision) >> len(controls), (n, targets, controls)
                want, mask = sum(1 << q for q in targets), m["kernel_mask"]
                assert mask & want == want and mask >> n == 0 and not mask & sum(1 << q for q in controls)
                # the matrix path (16 environments a step and more are left); a workgroup's trips at the grid's cap: 1024 workgroups, 512 for
                # five qubits, each taking a whole number of units per trip — so the units are a multiple of trips x cap and no field wrapped
                cap = 512 if len(targets) == 5 else 1024
                t = m["trips_per_workgroup"]
                assert m["path"] == 1 and t > 0 and m["units"] % (t * cap) == 0, (n, targets, controls, t)
                if not controls and len(targets) == 3:
                    m_trips.append(t)
                p = plans.ok(plans.apply_permutation_plan(targets, controls, n, precision))
                b, tmask = 12 if precision == 64 else 13, p["tile_mask"]
                assert p["path"] == 1 and p["tile_bits"] == b and bin(tmask).count("1") == b and tmask & want == want and tmask >> n == 0
                assert p["tiles"] == 1 << (n - len(controls) - b) and p["units"] == _state_units(n, precision) >> len(controls)
                assert p["trips_per_workgroup"] == _ceil_div(p["tiles"], 512)
        p_trips.append(p["trips_per_workgroup"])
        p_tiles.append(p["tiles"])
        emb = lr.Embedding(33, 1) if n == 33 else None
        if emb is not None:   # the plain kernel: the step of test_matrix_off_the_matrix_path leaves fewer than 16 environments
            (_, tg, cs), _small = lr.plain_matrix_step(emb)
            m = plans.ok(plans.apply_matrix_plan(tg, cs, n, precision, k=2))
            assert m["path"] == 0 and m["units"] == _state_units(n, precision) >> len(cs) and m["trips_per_workgroup"] == 1
            for st in lr.CASES["matrix"][1]:
                assert plans.ok(plans.apply_matrix_plan(emb.qubits(st[2]), emb.qubits(st[3]), n, precision, k=len(st[2]), num_controls=len(st[3])))["path"] == 1, st[2:]
        if precision == 32:   # a control on qubit 0: the odd amplitude of twice as many units
            assert plans.ok(plans.apply_matrix_plan([n - 1], [0], n, 32))["units"] == _state_units(n, 32)
    _doubles(m_trips, "matrix trips")
    _doubles(p_trips, "permutation trips")
    _doubles(p_tiles, "permutation tiles")


@pytest.mark.parametrize("precision", PRECISIONS)
def test_diagonal_plans_count_the_table(precision):
    import diagonal_ref
    trips_p, trips_e, trips_a = [], [], []
    for n in SIZES:
        p = diagonal_ref.plan(n, precision)
        assert p["items"] == 1 << (n - 1) and p["items_per_trip_phase"] > 0 and p["items_per_trip_expect"] > 0   # 16 bytes of the table: two entries
        trips_p.append(p["trips_at_cap_phase"])
        trips_e.append(p["trips_at_cap_expect"])
        top = 1 << (n - 1)
        g = plans.ok(plans.diagonal_gradient_plan([0, 1, 0], [0, 0, top], [top | 1, 0, 2], [top, 1], 1, n, precision))
        assert g["pauli_adjoint_sweeps"] == 2 and g["diag_adjoint_sweeps"] == 1 and g["sum_sweeps"] == 3
        assert g["diag_adjoint_items_per_trip"] > 0 and g["diag_adjoint_trips_at_cap"] > 0
        trips_a.append(g["diag_adjoint_trips_at_cap"])
    _doubles(trips_p, "diagonal phase trips")
    _doubles(trips_e, "diagonal expectation trips")
    _doubles(trips_a, "diagonal adjoint trips")


def test_sample_geometry_is_the_documented_pyramid():
    for n in SIZES:
        assert plans.ok(plans.sample_geometry(n)) == dict(chunk_bits=8, group_bits=18, scratch_bytes=8 * ((1 << (n - 8)) + (1 << (n - 18))))


@pytest.mark.parametrize("precision", PRECISIONS)
def test_qft_plans_partition_the_register(precision):
    all_trips = []
    for n in SIZES:
        regs = [[n - 1, 0, n - 2, 5], [1, 3, 6, n - 3, n - 2, n - 1, 9, 0, 4, 7], list(range(11)) + [n - 2, n - 1], list(range(n))]
        for reg in regs:
            plan = plans.ok(plans.apply_qft_plan(reg, n, precision, 0))
            p, digits, oop, tmask = plan["passes"], plan["digit_bits"], plan["out_of_place"], plan["tile_mask"]
            b = min(12 if precision == 64 else 13, n)
            assert 1 <= p <= 40 and len(digits) == len(oop) == len(tmask) == p and sum(digits) == len(reg) and all(1 <= d <= 10 for d in digits)
            assert sum(oop) % 2 == 0 and (len(reg) > 10 or p == 1)
            assert plan["units"] == _state_units(n, precision) and plan["tiles"] == 1 << (n - b) and plan["trips_per_workgroup"] == _ceil_div(plan["tiles"], 512)
            for i in range(p):   # every sweep works on the register's top digits[i] qubits (the rest has moved up behind the digits done)
                digit = sum(1 << q for q in reg[len(reg) - digits[i]:])
                assert bin(tmask[i]).count("1") == b and tmask[i] >> n == 0 and tmask[i] & digit == digit, (n, reg, i, hex(tmask[i]))
        all_trips.append(plan["trips_per_workgroup"])
    _doubles(all_trips, "qft trips")


@pytest.mark.parametrize("precision", PRECISIONS)
def test_collapse_plans_count_the_kept_part_and_the_whole_state(precision):
    for n in SIZES:
        for qubits, outcome in (([n - 1], 1), ([0, n - 1], 2), ([n - 3, n - 2, n - 1], 5), ([1, 2, 4, 6, 8, 10, 12, n - 3, n - 2, n - 1], 0b1011001101)):
            p = plans.ok(plans.collapse_plan(qubits, outcome, n, precision))
            kept = 1 << (n - len(qubits))
            assert p["collapse_units"] == _state_units(n, precision)
            assert p["weight_units"] == (kept if precision == 64 or 0 in qubits else kept // 2), (n, qubits, p["weight_units"])
            per_trip = 1024 * 256 * 8
            assert p["weight_trips"] == _ceil_div(p["weight_units"], per_trip) and p["collapse_trips"] == _ceil_div(p["collapse_units"], per_trip)


def test_helpers_of_the_gpu_test(pin):
    emb, dense0, small0 = pin
    every = np.arange(1 << N_PIN, dtype=np.uint64)
    for step in lr.CASES["permutation"][1]:
        moved = lr.ref_apply(dense0, step, emb.lab)
        assert np.array_equal(moved, dense0[lr.perm_source(step, every, emb.lab).astype(np.int64)])   # data movement: bit for bit
    n, j = 12, 0b100000100011
    idx = np.arange(1 << n, dtype=np.uint64)
    for inverse in (False, True):
        e = lr.rel_err(lr.qft_basis_amps32(n, j, idx, inverse), lr.qft_basis_amps(n, j, idx, inverse))
        assert 0 < e < 1e-6
    assert lr.deposit_on_active(emb, 0b10000000000011) == (1 << 15) | 3
