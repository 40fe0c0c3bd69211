"""Adjoint gradients through diagonal phases, checked on the CPU: the checker of tests/test_gpu_diag_gradient.py (diag_adjoint_ref)
against the exact chain rule through the Z rotations that a table of terms stands for and against dense operators, the host-only plan
call (plans.diagonal_gradient_plan) against its rules, the refusals that need no device, and the ValueErrors that
Simulator.energy_and_gradient raises in pure Python.

The tolerance of the checker-against-checker comparisons is 1e-12, DESIGN §7d's figure for these checkers: sums of at most 2^6
products of numbers of order one in fp64."""
from ctypes import byref, c_double, c_int, c_long, c_void_p

import numpy as np
import pytest

import adjoint_ref
import controlled_adjoint_ref
import diag_adjoint_ref as ref
import diagonal_ref
from diag_adjoint_ref import Diag
from gpu_quantum_simulator_amd import Diagonal, Simulator, _lib, plans
from pauli_rot_ref import rand_state

CHECKER_TOL = 1e-12
NEW_NAMES = ("qsim_diagonal_gradient", "qsim_diagonal_gradient_plan", "qsim_diagonal_adjoint_sweeps_launched", "qsim_diagonal_apply_into")  # census of the signature table


def test_signatures_and_exports_have_the_new_names():
    import gpu_quantum_simulator_amd as pkg
    lib = _lib.load()
    for name in NEW_NAMES:
        assert name in _lib.SIGNATURES and hasattr(lib, name)
    assert hasattr(pkg.Simulator, "diagonal_into")
    assert not hasattr(pkg.Cluster, "diagonal_into") and not hasattr(pkg.Cluster, "energy_and_gradient")


# ---- the checker ----------------------------------------------------------------------------------------------------------------------
def _mixed_case(n=6):
    """Two diagonal steps of tables from Z terms between X / Y rotations and controlled rotations; H mixes Pauli terms and w D."""
    rng = np.random.default_rng(60)
    cost = [(float(rng.uniform(-1, 1)), int(rng.integers(1, 1 << n))) for _ in range(7)]
    other = [(float(rng.uniform(-1, 1)), int(rng.integers(0, 1 << n))) for _ in range(4)]
    d_cost, d_other = diagonal_ref.table_from_terms(n, cost), diagonal_ref.table_from_terms(n, other)
    steps = [(0.7, 0, 1 << 2, 0),                       # X2
             Diag(0.43, d_cost),
             (-1.1, 0, 1 << 4, 1 << 4),                 # Y4
             (0.9, 1 << 1, 1 << 3 | 1, 1 << 3 | 1 << 5),  # a controlled rotation
             Diag(-0.81, d_other),
             (0.35, 1 << 5, 0, 1 | 1 << 2),             # a controlled Z string
             Diag(1.3, d_cost),
             (1.9, 0, 1, 1 << 3)]
    table_terms = {1: cost, 4: other, 6: cost}
    terms = adjoint_ref.random_hamiltonian(n, 5, 61, 2)
    return n, steps, table_terms, terms, (0.6, d_other)


def test_gradient_obeys_the_chain_rule_through_the_z_rotations():
    """exp(-i gamma D) = prod_k exp(-i (2 gamma c_k)/2 Z_k) for D = sum_k c_k Z_k, so dE/dgamma = sum_k 2 c_k dE/dtheta_k of the
    expanded list: exact, no finite difference.  The diagonal part of H is expanded the same way, into Pauli terms."""
    n, steps, table_terms, terms, obs = _mixed_case()
    psi0 = rand_state(n, 62)
    other = table_terms[4]
    expanded, owner = ref.expand(steps, table_terms)
    all_terms = terms + [(obs[0] * c, 0, z) for c, z in other]
    e_want, g_expanded, final_want = controlled_adjoint_ref.gradient(psi0, expanded, all_terms)
    want = ref.chain_rule(g_expanded, owner, len(steps))
    energy, grad, final = ref.gradient(psi0, steps, terms, obs)
    assert np.max(np.abs(want)) > 1e-2 and all(abs(want[k]) > 1e-3 for k in (1, 4, 6))
    assert abs(energy - e_want) < CHECKER_TOL and np.max(np.abs(grad - want)) < CHECKER_TOL
    assert np.max(np.abs(final - final_want)) < CHECKER_TOL
    # each part of the observable alone, and no observable
    for t, o, tt in ((terms, None, terms), ([], obs, [(obs[0] * c, 0, z) for c, z in other])):
        e_want, g_expanded, _ = controlled_adjoint_ref.gradient(psi0, expanded, tt)
        energy, grad, _ = ref.gradient(psi0, steps, t, o)
        assert abs(energy - e_want) < CHECKER_TOL and np.max(np.abs(grad - ref.chain_rule(g_expanded, owner, len(steps)))) < CHECKER_TOL
    energy, grad, _ = ref.gradient(psi0, steps, [], None)
    assert energy == 0.0 and not grad.any()


def test_gradient_against_dense_operators_for_a_table_that_is_no_pauli_sum():
    n = 4
    rng = np.random.default_rng(40)
    d1, d2, d_obs = (rng.uniform(-3, 3, size=1 << n) for _ in range(3))
    steps = [Diag(0.37, d1), (0.8, 0, 0b0110, 0b0010), Diag(-1.4, d2), (1.2, 1 << 3, 1, 1), Diag(0.9, d1)]
    terms = adjoint_ref.random_hamiltonian(n, 4, 41, 1)
    psi0 = rand_state(n, 42)
    for t, o in ((terms, (0.7, d_obs)), (terms, None), ([], (-1.3, d_obs))):
        e_want, g_want = ref.dense_gradient(psi0, steps, t, o, n)
        energy, grad, _ = ref.gradient(psi0, steps, t, o)
        assert np.max(np.abs(g_want)) > 1e-2
        assert abs(energy - e_want) < CHECKER_TOL * ref.observable_weight(t, o)
        assert np.max(np.abs(grad - g_want)) < CHECKER_TOL * 2 * 3 * ref.observable_weight(t, o)


def test_complex64_restatement_rounds_the_factor_once_and_steps_the_state_back():
    n, steps, _, terms, obs = _mixed_case()
    psi0 = rand_state(n, 63).astype(np.complex64)
    e64, g64, final64 = ref.gradient(psi0, steps, terms, obs)
    e32, g32, final32 = ref.gradient(psi0, steps, terms, obs, np.complex64)
    assert final32.dtype == np.complex64
    assert 0 < np.max(np.abs(g32 - g64)) < 1e-4 and abs(e32 - e64) < 1e-5
    only = [s for s in steps if ref.is_diag(s)]
    psi = ref.replay(psi0, only, np.complex64)
    for s in only:  # the same factor as diagonal_ref.apply_phase
        assert np.array_equal(ref.apply_step(psi, s, np.complex64), diagonal_ref.apply_phase(psi, s.d, s.gamma, np.complex64))
    back = ref.replay(psi0, ref.there_and_back(only), np.complex64)
    assert np.max(np.abs(back.astype(np.complex128) - psi0)) < 1e-5


# ---- the plan -------------------------------------------------------------------------------------------------------------------------
def _per_trip(precision):
    """diagonal.h's rule: about eight 16-byte loads in flight; an fp64 item is 5 loads (2 of psi, 2 of lambda, 1 of the table), an fp32
    item 3."""
    loads = 5 if precision == 64 else 3
    return min(range(1, 9), key=lambda items: (abs(items * loads - 8), -items))


@pytest.mark.parametrize("precision", [64, 32])
def test_plan_counts_sweeps(precision):
    K = plans.pauli_rotations_per_sweep()
    T = plans.pauli_terms_per_sweep()
    n = 9
    d = None
    x = 0b101
    assert _per_trip(64) == 2 and _per_trip(32) == 3
    cases = [
        ([], [], None, (0, 0, 0)),
        ([Diag(0.1, d), Diag(0.2, d), Diag(0.3, d)], [], (1.0, d), (0, 3, 1)),
        # runs of equal x split by a diagonal step: a run may not fuse across it
        ([(0.1, 0, x, 0), (0.2, 0, x, 1), Diag(0.3, d), (0.4, 0, x, 2), (0.5, 0, x, 0)], [(1.0, 1, 0), (0.5, 1, 1), (0.2, 2, 0)], None, (2, 1, 2)),
        ([(0.1, 0, x, 0)] * (K + 1), [(1.0, 0, 1)], (2.0, d), (2, 0, 2)),
        ([(0.1, 0, x, 0)] * K + [Diag(0.3, d)] + [(0.1, 0, x, 0)], [(1.0, 3, 1)] * (T + 1), None, (2, 1, 2)),
        # controls: a change of control mask ends a run
        ([(0.1, 1 << 4, x, 0), (0.2, 1 << 4, x, 0), (0.3, 1 << 5, x, 0), Diag(0.1, d), (0.3, 1 << 5, x, 0)], [], None, (3, 1, 0)),
    ]
    for steps, terms, obs, (pauli, diag, sums) in cases:
        got = ref.plan(steps, terms, obs, n, precision)
        assert (got["pauli_adjoint_sweeps"], got["diag_adjoint_sweeps"], got["sum_sweeps"]) == (pauli, diag, sums), (steps, got)
        assert got["diag_adjoint_sweeps"] == sum(1 for s in steps if ref.is_diag(s))
        assert got["diag_adjoint_items_per_trip"] == _per_trip(precision)
    # without diagonal steps and without D_obs: plans.controlled_gradient_plan's counts
    rotations, terms = controlled_adjoint_ref.uncontrolled_case()
    got = ref.plan(rotations, terms, None, controlled_adjoint_ref.BITS_N, precision)
    assert (got["pauli_adjoint_sweeps"], got["sum_sweeps"]) == controlled_adjoint_ref.plan(rotations, terms, controlled_adjoint_ref.BITS_N, precision)[:2]
    # NULL is_diag and NULL step_c: no diagonal step, no control
    rc, got = ref.plan_call([0, 0], [0, 0], [x, x], [], False, n, precision, null_flags=True, null_controls=True)
    assert rc == 0 and (got["pauli_adjoint_sweeps"], got["diag_adjoint_sweeps"]) == (1, 0)


@pytest.mark.parametrize("precision", [64, 32])
def test_plan_trips(precision):
    grid, threads = 1024, 256
    for n in range(0, 31):
        got = ref.plan([Diag(0.0, None)], [], None, n, precision)
        items = max(1, (1 << n) >> 1)
        if n <= 6:
            assert got["diag_adjoint_trips_at_cap"] == 1  # the plain path
        else:
            assert got["diag_adjoint_trips_at_cap"] == -(-(-(-items // threads)) // (_per_trip(precision) * grid))
    assert ref.loop_n(precision) == 21


def test_plan_refusals():
    lib = _lib.load()
    n, x = 9, 0b101

    def rc(flags, cs, xs, ham_x=(), n=n, bits=64, **kw):
        return ref.plan_call(flags, cs, xs, list(ham_x), False, n, bits, **kw)[0]

    assert rc([0], [0], [x]) == 0
    assert rc([1], [1 << 3], [0]) == _lib.ERR_ARG and b"control mask" in lib.qsim_last_error()  # a control mask on a diagonal step
    assert rc([1], [1 << 3], [0], null_controls=True) == 0
    assert rc([0], [0], [1 << n]) == _lib.ERR_ARG          # a qubit outside the register
    assert rc([1], [0], [1 << n]) == 0                     # x of a diagonal step is not looked at
    assert rc([0], [1], [x]) == _lib.ERR_ARG               # a control that carries a Pauli factor
    assert rc([0], [1 << n], [x]) == _lib.ERR_ARG          # a control outside the register
    assert rc([0], [0], [x], ham_x=[1 << n]) == _lib.ERR_ARG
    assert rc([0], [0], [x], n=41) == _lib.ERR_ARG and rc([0], [0], [x], n=-1) == _lib.ERR_ARG and rc([0], [0], [x], bits=16) == _lib.ERR_ARG
    out = [byref(c_long()), byref(c_long()), byref(c_long()), byref(c_int()), byref(c_long())]
    nothing = lambda **counts: plans.diagonal_gradient_plan(None, None, None, None, 0, n, 64, **counts)[0]
    assert nothing(num_steps=-1) == _lib.ERR_ARG and b"negative" in lib.qsim_last_error()
    assert nothing(num_ham=-1) == _lib.ERR_ARG
    assert nothing(num_steps=1) == _lib.ERR_ARG   # a rotation step without masks
    for k in range(5):
        args = list(out)
        args[k] = None
        assert lib.qsim_diagonal_gradient_plan(None, None, None, 0, None, 0, 0, n, 64, *args) == _lib.ERR_ARG  # raw: NULL for an out-parameter


def test_refusals_without_a_device():
    lib = _lib.load()
    e, g = c_double(), c_double()
    assert lib.qsim_diagonal_gradient(None, 0, None, None, None, None, None, None, None, None, 0, None, 0.0, byref(e), byref(g)) == _lib.ERR_ARG
    assert lib.qsim_diagonal_apply_into(None, None, 1.0, c_void_p(4096), 0) == _lib.ERR_ARG
    assert isinstance(plans.sweeps_launched("diagonal_adjoint"), int)   # a counter, no device


# ---- pure Python ----------------------------------------------------------------------------------------------------------------------
class _NoLibrary:
    def __getattr__(self, name):
        raise AssertionError(f"the library was asked for {name}")


def _stand_ins():
    """A Simulator and a Diagonal that never touched a device: only the type dispatch of energy_and_gradient is tested."""
    sim = object.__new__(Simulator)
    sim._h, sim.num_qubits, sim.precision = c_void_p(), 4, 64
    diag = object.__new__(Diagonal)
    diag._h, diag.num_qubits = c_void_p(1), 4   # never dereferenced: every call below raises first
    return sim, diag


def test_value_errors_before_any_launch(monkeypatch):
    sim, diag = _stand_ins()
    closed = object.__new__(Diagonal)
    closed._h, closed.num_qubits = c_void_p(), 4
    monkeypatch.setattr(_lib, "load", lambda: _NoLibrary())
    try:
        bad = [
            ([(0.3, diag, (1,))], [(1.0, "Z0")]),                       # controls on a diagonal entry
            ([(0.3, diag, (0, 2))], diag),
            ([(0.3, diag, (), 4)], diag),                               # not (gamma, diag)
            ([(0.3, diag)], [(1.0, diag), (0.5, "Z1"), (2.0, diag)]),   # two diagonal parts
            ([(0.3, diag)], [(1.0 + 0.5j, diag)]),                      # a complex weight
            ([(0.3, "X0")], [(np.complex128(2.0), diag)]),
            ([(0.3 + 0.1j, diag)], diag),                               # a complex gamma
            ([(0.3, diag)], [(1.0j, "Z0")]),                            # what the call refuses without a Diagonal
            ([(0.3, "X0", (0,)), (0.1, diag)], diag),
            ([(0.3, "X9"), (0.1, diag)], diag),
        ]
        for rotations, terms in bad:
            with pytest.raises(ValueError):
                sim.energy_and_gradient(rotations, terms)
        for rotations, terms in (([(0.3, closed)], [(1.0, "Z0")]), ([(0.3, "X0")], closed)):
            with pytest.raises(ValueError, match="closed"):
                sim.energy_and_gradient(rotations, terms)
    finally:
        diag._h = c_void_p()   # nothing to destroy
