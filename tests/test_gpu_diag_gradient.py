"""Adjoint gradients through diagonal phases on the device (qsim_diagonal_gradient, csrc/diagonal.hip's k_diag_adjoint and k_diag_apply;
Simulator.energy_and_gradient with (gamma, Diagonal) entries and a Diagonal in the observable; Simulator.diagonal_into).

The checker is tests/diag_adjoint_ref.py (numpy, pinned against the chain rule and dense operators by tests/test_diag_gradient_cpu.py)
applied to the amplitudes READ BACK before the call.
fp64, with W = sum|c_t| + |w| max|d_obs|: |E - ref| < 1e-10 W (the project's parity tolerance, scaled as tests/test_gpu_adjoint.py scales
it); a rotation's component < 1e-10 W; a diagonal step's component < 1e-10 * 2 max|d_step| * W (dE/dgamma = 2 <lambda|(-i) D|psi> is
bounded by 2 max|d| |lambda| and |lambda| by W).  The state afterwards within 1e-10 of the state before.
fp32: fp32_ref.check_fp32(got_grad, want64, ref32_grad), ref32 the checker run in complex64, C = 8 and FLOOR unchanged, for every call on its own; only
the calls on a register of ONE qubit are held to it together (test_energy_and_gradient says why), and a call whose every operator is
diagonal, whose gradient is zero, has a bound from the format's precision instead.  The energy by controlled_adjoint_ref.energy_tol with w D_obs counted as one more term of weight |w| max|d|.  The
state afterwards by the two-sided rule of the rotation tests.
Sizes: n = 1 and 6 (the plain path), 7 (exactly one wave block of 64 items), 10 (several workgroups) and the smallest n at which
plans.diagonal_gradient_plan reports more than one trip per workgroup with the grid at its cap."""
import contextlib
import ctypes
import math

import numpy as np
import pytest

import adjoint_ref
import controlled_adjoint_ref
import diag_adjoint_ref as ref
import diagonal_ref
import fp32_ref
from diag_adjoint_ref import Diag
from fp32_ref import check_fp32, report
from gpu_quantum_simulator_amd import Circuit, Cluster, Diagonal, Simulator, _lib, circuits, plans
from pauli_rot_ref import rand_state

pytestmark = pytest.mark.gpu
TOL = ref.TOL
PRECISIONS = [64, 32]
SMALL = [1, 6, 7, 10]
ANGLE = 50.0  # |gamma d_i| at most for the random tables
UP = ctypes.POINTER(ctypes.c_uint64)
DP = ctypes.POINTER(ctypes.c_double)


def _counters():
    return np.array([plans.sweeps_launched("diagonal_adjoint"), plans.sweeps_launched("pauli_adjoint"), plans.sweeps_launched("diagonal")], dtype=np.int64)


def _bits(sim):
    return sim.read().view(np.uint64).copy()


def _z_terms(n, count, seed):
    """[(c, z)]: ZZ pairs where the register has two qubits, single Z below that — a MaxCut-like cost."""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(count):
        a = int(rng.integers(0, n))
        b = int(rng.integers(0, n))
        out.append((float(rng.uniform(-1, 1)), 1 << a | 1 << b if a != b else 1 << a))
    return out


def _random_table(n, seed, gamma):
    return np.random.default_rng(seed).uniform(-ANGLE / abs(gamma), ANGLE / abs(gamma), size=1 << n)


@contextlib.contextmanager
def _diagonals(n, arrays):
    """id(array) -> a Diagonal that holds it, for ref.entries and ref.observable."""
    with contextlib.ExitStack() as stack:
        tables = {}
        for a in arrays:
            if id(a) not in tables:
                diag = stack.enter_context(Diagonal(n))
                diag.write(a)
                tables[id(a)] = diag
        yield tables


def _arrays(steps, obs):
    return [s.d for s in steps if ref.is_diag(s)] + ([obs[1]] if obs is not None else [])


def _energy_terms(terms, obs):
    """w D_obs as one more term of weight |w| max|d| for controlled_adjoint_ref.energy_tol."""
    return terms + ([(obs[0] * float(np.max(np.abs(obs[1]))), 0, 0)] if obs is not None else [])


def _check(precision, energy, grad, before, steps, terms, obs, label, nonzero=True, fp32_criterion=True):
    """`energy`, `grad` against the checker run from `before`; returns (want64, ref32 or None) of the gradient.  fp32_criterion=False:
    the caller gathers the components of several calls into one vector first."""
    e64, g64, final64 = ref.gradient(before, steps, terms, obs)
    W = ref.observable_weight(terms, obs)
    g32 = finals = None
    if precision == 32:
        _, g32, final32 = ref.gradient(before.astype(np.complex64), steps, terms, obs, np.complex64)
        finals = (final32, final64) if len(steps) else None
    tol_e = controlled_adjoint_ref.energy_tol(precision, _energy_terms(terms, obs), finals)
    scale = np.array([2.0 * float(np.max(np.abs(s.d))) if ref.is_diag(s) else 1.0 for s in steps])
    worst = float(np.max(np.abs(grad - g64) / scale)) if len(steps) else 0.0
    print(f"{label} p{precision}: energy err {abs(energy - e64):.3e} (tol {tol_e:.3e}), gradient max scaled err {worst:.3e} (W {W:.3f}), "
          f"max |grad| {np.max(np.abs(g64)) if len(steps) else 0.0:.3e}")
    assert abs(energy - e64) < tol_e
    if nonzero:
        assert np.max(np.abs(g64)) > 1e-3  # not a comparison of zeros
    if precision == 64:
        assert np.all(np.abs(grad - g64) < TOL * scale * W)
    elif fp32_criterion:
        report(label, check_fp32(grad, g64, g32))
    elif np.any(g64):
        report(label + " (one call, not asserted)", (fp32_ref.rel_err(grad, g64), fp32_ref.rel_err(g32, g64)))
    return g64, g32


def _state_back(precision, after, before, steps, label):
    if precision == 64:
        worst = float(np.max(np.abs(after - before)))
        print(f"{label}: state after vs before, max abs {worst:.3e}")
        assert worst < TOL
    else:
        ref32 = ref.replay(before.astype(np.complex64), ref.there_and_back(steps), np.complex64)
        bound = 2 * fp32_ref.C * max(fp32_ref.rel_err(ref32, before), fp32_ref.FLOOR)
        print(f"{label}: state after vs before, rel err {fp32_ref.rel_err(after, before):.3e} (bound {bound:.3e})")
        assert fp32_ref.rel_err(after, before) <= bound


def _one_call(precision, n, start, steps, terms, obs, label, nonzero=True, fp32_criterion=False):
    """One call from `start`, everything checked: counters against the plan, energy, gradient, the state afterwards.  Returns
    (got, want64, ref32) of the gradient."""
    with Simulator(n, precision=precision) as sim, _diagonals(n, _arrays(steps, obs)) as tables:
        sim.write(start)
        before = sim.read()
        count = _counters()
        energy, grad = sim.energy_and_gradient(ref.entries(steps, n, tables), ref.observable(terms, obs, n, tables))
        taken = _counters() - count
        after = sim.read()
    plan = ref.plan(steps, terms, obs, n, precision)
    num_diag = sum(1 for s in steps if ref.is_diag(s))
    assert taken[0] == plan["diag_adjoint_sweeps"] == num_diag, (label, taken, plan)       # one backward diagonal sweep per diagonal step
    assert taken[1] == plan["pauli_adjoint_sweeps"], (label, taken, plan)                   # none of them in the Pauli counter
    assert taken[2] == num_diag + (1 if obs is not None else 0), (label, taken)      # the forward phases and the k_diag_apply sweep
    g64, g32 = _check(precision, energy, grad, before, steps, terms, obs, label, nonzero, fp32_criterion)
    _state_back(precision, after, before, steps, label)
    return grad, g64, g32


def _circuits(n, d_terms, d_random):
    """label -> steps: diagonal steps only; a 2-layer QAOA (phase, then X mixers); diagonal steps between Y rotations and a controlled
    rotation.  gamma times the random table stays within ANGLE."""
    top = n - 1
    controlled = (0.9, 1, 0, 0) if n == 1 else (0.9, 1 << top, 1, 1 | (1 << (n // 2) if n > 2 else 0))
    return {
        "diagonal only": [Diag(0.37, d_terms), Diag(-0.37, d_random), Diag(0.81, d_terms)],
        "qaoa": [Diag(0.43, d_terms)] + [(0.7, 0, 1 << q, 0) for q in range(n)] + [Diag(-0.29, d_terms)] + [(-1.1, 0, 1 << q, 0) for q in range(n)],
        "mixed": [(0.6, 0, 1, 1), Diag(0.37, d_random), (-0.8, 0, 1 << top, 1 << top), controlled, Diag(-0.52, d_terms), (1.3, 0, 1 << (n // 2), 1 << (n // 2))],
    }


# ---- 1. accuracy of the energy and the gradient, and the state restored ----------------------------------------------------------------
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("n", SMALL)
def test_energy_and_gradient(n, precision):
    """Three circuits times three observables (Pauli only, D only, both), tables from Z terms and from a random write with
    |gamma d_i| up to 50.  fp32: every call's gradient is held to the criterion on its own, but for two kinds of call.  Where every
    operator is diagonal the reference is zero and the call has a bound of its own (below).  At n = 1 the eight other calls are held to
    it together, one vector per kind of table: a state of two amplitudes makes the complex64 restatement's error the sum of a handful
    of roundings, which among these calls falls anywhere from 7e-8 to 1.9e-6 on the device's state (the device: 7e-9 to 2.4e-6), so the
    quotient of one call divides two such draws; every n = 1 call's own quotient is printed."""
    z_terms = _z_terms(n, 12, 100 + n)
    d_terms = diagonal_ref.table_from_terms(n, z_terms)
    d_random = _random_table(n, 110 + n, 0.37)
    d_obs = _random_table(n, 120 + n, 25.0)   # |d| up to 2
    assert 40.0 < np.max(np.abs(0.37 * d_random)) <= ANGLE or n == 1
    terms = adjoint_ref.random_hamiltonian(n, 6, 130 + n, 2)
    plus = np.full(1 << n, 2.0 ** (-0.5 * n), dtype=np.complex128)
    gathered = {"terms": ([], [], []), "random": ([], [], [])}
    for name, steps in _circuits(n, d_terms, d_random).items():
        start = plus if name == "qaoa" else rand_state(n, 140 + n)
        for kind, t, o in (("pauli", terms, None), ("diagonal", [], (0.7, d_obs)), ("both", terms, (-0.6, d_terms))):
            commute = name == "diagonal only" and kind == "diagonal"   # every operator is diagonal: the gradient is zero
            got, want, ref32 = _one_call(precision, n, start, steps, t, o, f"{name}, H {kind}, n={n}", nonzero=not commute,
                                         fp32_criterion=n > 1 and not commute)
            if commute:
                # zero but for rounding.  fp32: lambda = fl(f psi) carries 2^-24 per component, so Im(conj(lambda_i) psi_i) is at most
                # 2^-23 |f| |psi_i|^2 and a component at most 2 max|d_step| 2^-23 W; each of the 3 steps back rounds both once more: C = 8
                assert np.max(np.abs(want)) < 1e-12 * np.max(np.abs(d_random))
                if precision == 32:
                    bound = fp32_ref.C * 2.0 ** -23 * 2.0 * np.array([np.max(np.abs(s.d)) for s in steps]) * ref.observable_weight(t, o)
                    assert np.all(np.abs(got) < bound)
            elif precision == 32 and n == 1:
                which = gathered["random" if any(ref.is_diag(s) and s.d is d_random for s in steps) else "terms"]
                which[0].extend(got), which[1].extend(want), which[2].extend(ref32)
    if precision == 32 and n == 1:
        for key, (got, want, ref32) in gathered.items():
            report(f"diagonal gradient n={n}, tables: {key}", check_fp32(np.array(got), np.array(want), np.array(ref32)))


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("n", SMALL)
def test_diagonal_steps_leave_the_bits_of_the_public_phases(n, precision):
    """A list of diagonal steps only: psi is stepped forwards by k_diag_phase and back by k_diag_adjoint with the factor of
    apply_diagonal_phase(diag, -gamma), so the state's bits equal those of the public calls gamma_1 .. gamma_K, -gamma_K .. -gamma_1."""
    d1, d2 = _random_table(n, 200 + n, 0.37), diagonal_ref.table_from_terms(n, _z_terms(n, 9, 210 + n))
    steps = [Diag(0.37, d1), Diag(-1.21, d2), Diag(0.05, d1)]
    terms = adjoint_ref.random_hamiltonian(n, 5, 220 + n, 1)
    with Simulator(n, precision=precision) as sim, Simulator(n, precision=precision) as twin, _diagonals(n, [d1, d2]) as tables:
        for s in (sim, twin):
            s.write(rand_state(n, 230 + n))
        assert np.array_equal(_bits(sim), _bits(twin))
        sim.energy_and_gradient(ref.entries(steps, n, tables), ref.observable(terms, (0.4, d2), n, tables))
        for s in ref.there_and_back(steps):
            twin.apply_diagonal_phase(tables[id(s.d)], s.gamma)
        assert np.array_equal(_bits(sim), _bits(twin))


# ---- 2. where every workgroup loops ----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def loop_data():
    """At the looping size, computed once: n, the start state, the step's table (top-bit-sensitive: 2 bit(n-1) - 1, plus a low-bit
    term) and the observable's."""
    sizes = {ref.loop_n(p) for p in PRECISIONS}
    assert len(sizes) == 1
    n = sizes.pop()
    step_terms = [(-1.0, 1 << (n - 1)), (0.25, 1)]          # -Z_(n-1) = 2 bit(n-1) - 1
    obs_terms = [(0.5, 1 << (n - 1) | 1 << 3), (-0.75, 1 << 8), (0.3, 1 << 1)]
    return n, controlled_adjoint_ref.loop_state(n), diagonal_ref.table_from_terms(n, step_terms), diagonal_ref.table_from_terms(n, obs_terms)


@pytest.mark.parametrize("precision", PRECISIONS)
def test_where_the_sweep_loops(precision, loop_data):
    """One diagonal step with a diagonal observable of another table: a trip skipped or done twice changes the energy and the state.
    Every operator of that call is diagonal, so its gradient is zero; a second call puts a rotation between two such steps and adds a
    Pauli term to H, so that its gradient is not."""
    n, start, d_step, d_obs = loop_data
    assert ref.plan([Diag(0.0, None)], [], None, n, precision)["diag_adjoint_trips_at_cap"] > 1 and ref.plan([Diag(0.0, None)], [], None, n - 1, precision)["diag_adjoint_trips_at_cap"] == 1
    steps = [Diag(0.61, d_step)]
    _, want, _ = _one_call(precision, n, start, steps, [], (1.0, d_obs), f"looping, H diagonal, n={n}", nonzero=False)
    assert np.max(np.abs(want)) < 1e-12
    steps = [Diag(0.61, d_step), (0.7, 0, 1 << (n - 1) | 1 << 2, 1 << 5), Diag(-0.4, d_step)]
    _one_call(precision, n, start, steps, [(0.8, 1 << (n - 2) | 1 << 2, 1 << 5)], (1.0, d_obs), f"looping, H mixed, n={n}", fp32_criterion=True)


# ---- 3. diagonal_into ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("n", [1, 7, 10])
def test_diagonal_into(n, precision):
    import torch
    real = torch.float64 if precision == 64 else torch.float32
    cdtype = np.complex128 if precision == 64 else np.complex64
    d = _random_table(n, 300 + n, 1.0)
    w = -0.83
    with Simulator(n, precision=precision) as sim, Diagonal(n) as diag:
        diag.write(d)
        sim.write(rand_state(n, 310 + n))
        psi, bits = sim.read().astype(cdtype), _bits(sim)
        dst = torch.full((2 << n,), float("nan"), dtype=real, device="cuda:0")
        torch.cuda.synchronize()
        count = _counters()
        sim.diagonal_into(diag, dst.data_ptr(), w)           # storing: the NaNs are not read
        sim.sync()
        stored = dst.cpu().numpy().view(cdtype).copy()
        factor = (np.float64(w) * d).astype(np.float64 if precision == 64 else np.float32)
        want = (factor * psi).astype(cdtype)
        eps = 2.0 ** -52 if precision == 64 else 2.0 ** -23
        assert not np.isnan(stored).any() and np.max(np.abs(stored - want)) <= 2 * eps * np.max(np.abs(want))
        sim.diagonal_into(diag, dst.data_ptr(), 0.5, accumulate=True)
        sim.sync()
        summed = dst.cpu().numpy().view(cdtype).copy()
        want2 = stored.astype(np.complex128) + 0.5 * d * psi.astype(np.complex128)
        assert np.max(np.abs(summed - want2)) <= 4 * eps * np.max(np.abs(want))
        assert np.array_equal(_counters() - count, [0, 0, 2]) and np.array_equal(_bits(sim), bits)
        sim.diagonal_into(diag, dst.data_ptr())              # weight 1
        sim.sync()
        assert np.max(np.abs(dst.cpu().numpy().view(cdtype) - (d.astype(factor.dtype) * psi).astype(cdtype))) <= 2 * eps * np.max(np.abs(d))


@pytest.mark.parametrize("precision", PRECISIONS)
def test_diagonal_into_refusals(precision):
    import torch
    n = 6
    with Simulator(n, precision=precision) as sim, Simulator(n, precision=precision) as lender, Diagonal(n) as diag, Diagonal(n + 1) as wide, \
            Diagonal(n) as closed:
        closed.close()
        sim.write(rand_state(n, 320))
        spare = lender.device_ptr
        lender.sync()
        sim.set_spare_buffer(spare)
        dst = torch.zeros(2 << n, dtype=torch.float64, device="cuda:0")
        torch.cuda.synchronize()
        before = _bits(sim)
        calls = [lambda: sim.diagonal_into(wide, dst.data_ptr()),
                 lambda: sim.diagonal_into(closed, dst.data_ptr()),
                 lambda: sim.diagonal_into(diag, dst.data_ptr(), float("nan")),
                 lambda: sim.diagonal_into(diag, dst.data_ptr(), float("inf")),
                 lambda: sim.diagonal_into(diag, 0),
                 lambda: sim.diagonal_into(diag, sim.device_ptr),
                 lambda: sim.diagonal_into(diag, spare)]           # the state's spare buffer
        for call in calls:
            with pytest.raises(_lib.QsimError) as err:
                call()
            assert err.value.code == _lib.ERR_ARG
            assert np.array_equal(_bits(sim), before)
        sim.set_spare_buffer(None)
        assert not dst.cpu().numpy().any()
    assert not hasattr(Cluster, "diagonal_into")


@pytest.mark.parametrize("precision", PRECISIONS)
def test_a_write_behind_diagonal_into_waits_for_the_sweep(precision, loop_data):
    """diagonal_into returns without waiting, so a diag.write issued right behind it has to wait for the sweep that still reads the table
    (mark_read behind the launch): dst holds w D psi of the OLD table, storing and accumulating, at the size where the sweep loops."""
    import torch
    n, start, d_old, d_obs = loop_data
    cdtype = np.complex128 if precision == 64 else np.complex64
    eps = 2.0 ** -52 if precision == 64 else 2.0 ** -23
    with Simulator(n, precision=precision) as sim, Diagonal(n) as diag:
        sim.write(start)
        psi = sim.read()
        dst = torch.zeros(2 << n, dtype=torch.float64 if precision == 64 else torch.float32, device="cuda:0")
        torch.cuda.synchronize()
        want = np.zeros(1 << n, dtype=np.complex128)
        for accumulate, old, new in ((False, d_old, d_obs), (True, d_obs, np.full(1 << n, 1e6))):
            if not accumulate:
                diag.write(old)
            sim.sync()
            sim.diagonal_into(diag, dst.data_ptr(), 0.75, accumulate=accumulate)
            diag.write(new)                                        # nothing synchronised in between
            sim.sync()
            want = want + 0.75 * old * psi
            got = dst.cpu().numpy().view(cdtype)
            assert np.max(np.abs(got - want)) <= 4 * eps * np.max(np.abs(want))
            assert np.array_equal(diag.read(), new)


# ---- 4. routing ------------------------------------------------------------------------------------------------------------------------
def _c_arrays(rotations, terms):
    cs, xs, zs = (np.array([r[i] for r in rotations], dtype=np.uint64) for i in (1, 2, 3))
    th = np.array([r[0] for r in rotations], dtype=np.float64)
    hx, hz = (np.array([t[i] for t in terms], dtype=np.uint64) for i in (1, 2))
    co = np.array([t[0] for t in terms], dtype=np.float64)
    return cs, xs, zs, th, hx, hz, co


@pytest.mark.parametrize("precision", PRECISIONS)
def test_without_a_diagonal_the_bits_of_the_pauli_gradient(precision):
    """A list without any Diagonal takes the old path in Python and, through qsim_diagonal_gradient with no table anywhere, launches
    what qsim_pauli_gradient launches: the same bits for energy, gradient and state, and no diagonal counter moves."""
    n = controlled_adjoint_ref.BITS_N
    rotations, terms = controlled_adjoint_ref.uncontrolled_case()
    cs, xs, zs, th, hx, hz, co = _c_arrays(rotations, terms)
    start = rand_state(n, 13)
    lib = _lib.load()
    out = []
    for how in ("qsim_pauli_gradient", "python", "qsim_diagonal_gradient", "qsim_diagonal_gradient, NULL entries"):
        with Simulator(n, precision=precision) as sim:
            sim.write(start)
            count = _counters()
            e, g = ctypes.c_double(7.0), np.full(len(rotations), 7.0)
            ham = (hx.ctypes.data_as(UP), hz.ctypes.data_as(UP), co.ctypes.data_as(DP), hx.size)
            if how == "qsim_pauli_gradient":
                _lib.check(lib.qsim_pauli_gradient(sim._h, xs.ctypes.data_as(UP), zs.ctypes.data_as(UP), th.ctypes.data_as(DP), xs.size, *ham, ctypes.byref(e), g.ctypes.data_as(DP)))
                energy = e.value
            elif how == "python":
                energy, g = sim.energy_and_gradient(controlled_adjoint_ref.entries(rotations, n), controlled_adjoint_ref.term_texts(terms, n))
            else:
                none = (ctypes.c_void_p * len(rotations))() if "NULL entries" in how else None
                _lib.check(lib.qsim_diagonal_gradient(sim._h, xs.size, none, None, xs.ctypes.data_as(UP), zs.ctypes.data_as(UP), th.ctypes.data_as(DP), *ham, None, 0.0,
                                                      ctypes.byref(e), g.ctypes.data_as(DP)))
                energy = e.value
            taken = _counters() - count
            assert taken[0] == 0 and taken[2] == 0 and taken[1] == ref.plan(rotations, terms, None, n, precision)["pauli_adjoint_sweeps"]
            out.append((np.float64(energy).view(np.uint64), g.view(np.uint64).copy(), _bits(sim)))
    assert np.max(np.abs(out[0][1].view(np.float64))) > 1e-3
    for other in out[1:]:
        assert out[0][0] == other[0] and np.array_equal(out[0][1], other[1]) and np.array_equal(out[0][2], other[2])


# ---- 5. ordering and equal bits --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", PRECISIONS)
def test_equal_calls_equal_bits_and_a_write_behind_the_call_changes_nothing(precision):
    """Equal bits for energy, gradient and state under grid_cap 0, 3 and 1 << 30 (the backward sweep reduces: the cap does not apply to
    it; the forward phase and k_diag_apply write each amplitude from one thread); a diag.write issued right behind the call waits for
    the call's sweeps and leaves its result and the state it restored alone."""
    n = 12
    d1, d2 = _random_table(n, 400, 0.37), diagonal_ref.table_from_terms(n, _z_terms(n, 20, 401))
    steps = [(0.6, 0, 1 << 3, 1 << 3), Diag(0.37, d1), (-0.8, 1 << 11, 0b110, 1), Diag(-0.52, d2), (1.3, 0, 1 << 7, 0)]
    terms = adjoint_ref.random_hamiltonian(n, 6, 402, 2)
    obs = (0.7, d2)
    start = rand_state(n, 403)
    out = []
    for cap in (0, 0, 3, 1 << 30):
        with Simulator(n, precision=precision, grid_cap=cap) as sim, _diagonals(n, [d1, d2]) as tables:
            sim.write(start)
            before = sim.read()
            energy, grad = sim.energy_and_gradient(ref.entries(steps, n, tables), ref.observable(terms, obs, n, tables))
            for diag in tables.values():      # nothing synchronised in between
                diag.write(np.full(1 << n, 1e6))
            out.append((np.float64(energy).view(np.uint64), grad.view(np.uint64).copy(), _bits(sim)))
            if len(out) == 1:
                _check(precision, energy, grad, before, steps, terms, obs, "ordering")
                _state_back(precision, sim.read(), before, steps, "ordering")
    for other in out[1:]:
        assert out[0][0] == other[0] and np.array_equal(out[0][1], other[1]) and np.array_equal(out[0][2], other[2])


# ---- 6. other conditions of the state --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", PRECISIONS)
def test_fresh_zero_ket(precision):
    """A QAOA layer pair from a never-touched register: Y rotations make the superposition through the gate queue."""
    n = 9
    d = diagonal_ref.table_from_terms(n, _z_terms(n, 15, 500))
    steps = [(0.5 * math.pi, 0, 1 << q, 1 << q) for q in range(n)] + [Diag(0.43, d)] + [(0.7, 0, 1 << q, 0) for q in range(n)] + [Diag(-0.3, d)] + [(0.4, 0, 1 << q, 0) for q in range(n)]
    ket0 = np.zeros(1 << n, dtype=np.complex128)
    ket0[0] = 1.0
    with Simulator(n, precision=precision) as sim, _diagonals(n, [d]) as tables:
        assert sim.get_support()[1]                                    # |0...0> is held lazily
        energy, grad = sim.energy_and_gradient(ref.entries(steps, n, tables), tables[id(d)])   # H = D
        after = sim.read()
    _check(precision, energy, grad, ket0, steps, [], (1.0, d), "fresh |0...0>")
    _state_back(precision, after, ket0, steps, "fresh |0...0>")


@pytest.mark.parametrize("precision", PRECISIONS)
def test_partial_support(precision):
    """Gates on the low 7 qubits of an 18-qubit register leave most of the buffer unwritten, as tests/test_gpu_diagonal.py builds it:
    the call writes the zeros out first."""
    n = 18
    few = Circuit.from_gates(n, circuits.random_gates(*fp32_ref.FEW_CIRCUIT))
    d = diagonal_ref.table_from_terms(n, _z_terms(n, 15, 510))
    steps = [Diag(0.43, d), (0.7, 0, 1 << 17 | 1 << 2, 1 << 2), (0.9, 0, 1 << 5, 0), Diag(-0.3, d)]
    terms = [(0.8, 1 << 17 | 1, 1 << 3), (-0.5, 1 << 4, 1 << 4)]
    with Simulator(n, precision=precision) as probe, Simulator(n, precision=precision) as sim, _diagonals(n, [d]) as tables:
        probe.run(few)
        before = probe.read()                                          # the read writes the zeros out: the state is read from a twin
        sim.run(few)
        assert sim.get_support()[0] != (1 << n) - 1                    # partial
        energy, grad = sim.energy_and_gradient(ref.entries(steps, n, tables), ref.observable(terms, (0.6, d), n, tables))
        after = sim.read()
    _check(precision, energy, grad, before, steps, terms, (0.6, d), "partial support")
    _state_back(precision, after, before, steps, "partial support")


@pytest.mark.parametrize("precision", PRECISIONS)
def test_a_state_that_holds_nothing_and_refused_calls(precision):
    n = 6
    lib = _lib.load()
    d = _random_table(n, 600, 1.0)
    with Simulator(n, precision=precision) as sim, Diagonal(n) as diag, Diagonal(n + 1) as wide:
        diag.write(d)
        sim.write(rand_state(n, 601))
        before = _bits(sim)
        nan, inf = float("nan"), float("inf")
        refused = [lambda: sim.energy_and_gradient([(0.3, wide)], [(1.0, "Z0")]),          # a table of another qubit count
                   lambda: sim.energy_and_gradient([(0.3, "X0")], wide),
                   lambda: sim.energy_and_gradient([(0.3, "X0"), (nan, diag)], diag),     # a non-finite gamma
                   lambda: sim.energy_and_gradient([(inf, "X0"), (0.1, diag)], diag),
                   lambda: sim.energy_and_gradient([(0.3, diag)], [(nan, diag)]),         # a non-finite weight
                   lambda: sim.energy_and_gradient([(0.3, diag)], [(inf, "Z0")]),
                   lambda: sim.energy_and_gradient([(0.3, "X0", (1,)), (0.1, "Z2", (7,)), (0.1, diag)], diag)]   # a control outside the register
        for call in refused:
            with pytest.raises((_lib.QsimError, ValueError)) as err:
                call()
            assert not isinstance(err.value, _lib.QsimError) or err.value.code == _lib.ERR_ARG
            assert np.array_equal(_bits(sim), before)
        # the C call: a control mask on a diagonal step, NULL arguments, negative counts
        one = (ctypes.c_void_p * 1)(diag._h.value)
        c, x, z, th = (np.array([v], dtype=t) for v, t in ((1 << 2, np.uint64), (0, np.uint64), (0, np.uint64), (0.3, np.float64)))
        e, g = ctypes.c_double(), np.zeros(1)
        tail = (None, None, None, 0, diag._h, 1.0, ctypes.byref(e), g.ctypes.data_as(DP))
        assert lib.qsim_diagonal_gradient(sim._h, 1, one, c.ctypes.data_as(UP), x.ctypes.data_as(UP), z.ctypes.data_as(UP), th.ctypes.data_as(DP), *tail) == _lib.ERR_ARG
        assert b"control mask" in lib.qsim_last_error()
        assert lib.qsim_diagonal_gradient(sim._h, 1, one, None, None, None, None, *tail) == _lib.ERR_ARG
        assert lib.qsim_diagonal_gradient(sim._h, -1, None, None, None, None, None, *tail) == _lib.ERR_ARG
        assert lib.qsim_diagonal_gradient(sim._h, 1, None, None, None, None, th.ctypes.data_as(DP), *tail) == _lib.ERR_ARG   # a rotation step without masks
        assert lib.qsim_diagonal_gradient(sim._h, 0, None, None, None, None, None, None, None, None, -1, None, 0.0, ctypes.byref(e), None) == _lib.ERR_ARG
        assert np.array_equal(_bits(sim), before)
        # x, z of a diagonal step are not looked at and may be NULL when every step is diagonal; energy or grad may be NULL
        _lib.check(lib.qsim_diagonal_gradient(sim._h, 1, one, None, None, None, th.ctypes.data_as(DP), None, None, None, 0, diag._h, 1.0, None, None))
        # a shard that holds nothing: zeros, no sweep, the state untouched
        sim.reset(holds_index0=False)
        count = _counters()
        energy, grad = sim.energy_and_gradient([(0.3, diag), (0.2, "X0"), (0.1, diag)], [(0.5, "Z1"), (2.0, diag)])
        assert energy == 0.0 and grad.size == 3 and not grad.any() and not (_counters() - count).any()
        assert lib.qsim_holds_nothing(sim._h) == 1 and not sim.read().any()
