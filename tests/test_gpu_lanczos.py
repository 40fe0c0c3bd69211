"""The Lanczos ground-state solver on the device (Simulator.ground_state, qsim_lanczos_ground; csrc/lanczos.cpp, csrc/combine.hip).

The checker is tests/lanczos_ref.py (numpy, the device's order of operations; tests/test_lanczos_cpu.py pins it against dense
operators) and dense diagonalisation of the small Hamiltonians used here.  W = sum|c_t| throughout.
What is derived, not tuned: for any vector y with Rayleigh quotient rq, |rq - E_0'| <= |H y - rq y| / |y| for SOME eigenvalue E_0';
together with rq < E_0 + gap / 2 that eigenvalue is the lowest.  The Ritz vector read back is held to exactly that, computed in
numpy fp64.
fp64: the returned energy against rq and the returned residual against the one measured in numpy, both within 1e-10 W, the
project's parity tolerance scaled by the operator's weight.
fp32: the project's rule for fp32 results, |theta - E_0| <= C max(|theta_ref32 - E_0|, FLOOR W), with theta_ref32 from the checker
run in complex64 and C, FLOOR of tests/fp32_ref.py; the returned residual against the numpy one within the same bound.  On the
CPU the checker's own error was 1e-8 against a floor term FLOOR W = 1.4e-6: the reference is inside by a wide margin."""
import functools

import numpy as np
import pytest

import adjoint_ref
import fp32_ref
import lanczos_ref as ref
from gpu_quantum_simulator_amd import Simulator, _lib
from pauli_rot_ref import rand_state

pytestmark = pytest.mark.gpu
TOL = 1e-10
PRECISIONS = [64, 32]


def _ctype(precision):
    return np.complex128 if precision == 64 else np.complex64


def _tol(precision, terms):
    return (1e-9 if precision == 64 else 1e-5) * adjoint_ref.weight(terms)


def _bits(sim):
    return sim.read().view(np.uint64).copy()


@functools.lru_cache(maxsize=None)
def _levels(case):
    """The two lowest eigenvalues of a case's Hamiltonian, computed once."""
    terms, n = {"ising": (ref.ising(ref.ISING_N), ref.ISING_N), "random": (ref.random_case()[1], 9)}[case]
    w = np.linalg.eigvalsh(adjoint_ref.dense_hamiltonian(terms, n))
    return float(w[0]), float(w[1])


@functools.lru_cache(maxsize=None)
def _checker(case, precision, max_steps=200):
    state, terms = ref.ising_case() if case == "ising" else ref.random_case()
    return ref.lanczos(state.astype(_ctype(precision)), terms, _tol(precision, terms), max_steps, _ctype(precision))


def _energy_bound(precision, e_ref, e0, terms):
    weight = adjoint_ref.weight(terms)
    return TOL * weight if precision == 64 else fp32_ref.C * max(abs(e_ref - e0), fp32_ref.FLOOR * weight)


def _run(sim, n, terms, tol, **kw):
    return sim.ground_state(adjoint_ref.term_texts(terms, n), tol, **kw)


def _check_vector(precision, out, y, terms, e0, label, gap=None, checker=None):
    """The state read back after ground_state(vector=True) and the call's numbers, by the module docstring's criteria."""
    weight = adjoint_ref.weight(terms)
    rq, r = ref.rayleigh(y, terms)
    norm2 = float(np.vdot(y, y).real)
    e_ref = checker["energy"] if checker else e0
    bound = _energy_bound(precision, e_ref, e0, terms)
    quotient = abs(out["energy"] - e0) / max(abs(e_ref - e0), fp32_ref.FLOOR * weight)
    print(f"{label} p{precision}: steps {out['steps']} (checker {checker['steps'] if checker else '-'}), E - E0 = {out['energy'] - e0:.3e}, rq - E0 = {rq - e0:.3e}, "
          f"residual returned {out['residual']:.6e} numpy {r:.6e}, |y|^2 - 1 = {norm2 - 1:.3e}, fp32 quotient {quotient:.3f}, W = {weight:.3f}")
    assert abs(norm2 - 1.0) < (1e-10 if precision == 64 else 1e-6)
    assert abs(rq - e0) <= r
    if gap is not None:
        assert rq < e0 + 0.5 * gap
    assert abs(out["residual"] - r) <= bound
    if precision == 64:
        assert abs(out["energy"] - rq) < TOL * weight
    else:
        assert abs(out["energy"] - e0) <= bound


@pytest.mark.parametrize("precision", PRECISIONS)
def test_ising_chain(precision):
    """Transverse-field Ising, n = 10, J = 1, h = 1.5, from rand_state(10, 5): converged before 200 steps, the Ritz vector is the
    ground state; vector=False leaves the state's bits alone and returns the same energy, steps, alphas and betas, bit for bit;
    equal calls return equal bits."""
    state, terms = ref.ising_case()
    n, tol = ref.ISING_N, _tol(precision, terms)
    e0, e1 = _levels("ising")
    checker = _checker("ising", precision)
    with Simulator(n, precision=precision) as sim:
        sim.write(state)
        before = _bits(sim)
        plain = _run(sim, n, terms, tol, vector=False)
        assert np.array_equal(_bits(sim), before)
        out = _run(sim, n, terms, tol)
        y = sim.read()
        assert out["converged"] and out["steps"] < 200 and plain["converged"]
        assert (plain["energy"], plain["steps"]) == (out["energy"], out["steps"])
        assert np.array_equal(plain["alphas"], out["alphas"]) and np.array_equal(plain["betas"], out["betas"])
        assert plain["residual"] <= tol
        _check_vector(precision, out, y, terms, e0, "ising n=10", gap=e1 - e0, checker=checker)
        assert abs((e1 - e0) - ref.ISING_GAP) < 1e-3
        # equal calls, equal bits
        sim.write(state)
        again = _run(sim, n, terms, tol)
        assert again["energy"] == out["energy"] and again["residual"] == out["residual"] and again["steps"] == out["steps"]
        assert np.array_equal(again["alphas"], out["alphas"]) and np.array_equal(again["betas"], out["betas"])
        assert np.array_equal(sim.read().view(np.uint64), y.view(np.uint64))


@pytest.mark.parametrize("precision", PRECISIONS)
def test_three_steps(precision):
    state, terms = ref.ising_case()
    n, weight = ref.ISING_N, adjoint_ref.weight(ref.ising(ref.ISING_N))
    e0, _ = _levels("ising")
    checker = _checker("ising", precision, 3)
    with Simulator(n, precision=precision) as sim:
        sim.write(state)
        out = _run(sim, n, terms, _tol(precision, terms), max_steps=3)
        y = sim.read()
    assert out["steps"] == 3 and not out["converged"] and checker["steps"] == 3
    assert out["alphas"].size == 3 and out["betas"].size == 3
    print(f"three steps p{precision}: alphas err {np.max(np.abs(out['alphas'] - checker['alphas'])):.3e}, betas err {np.max(np.abs(out['betas'] - checker['betas'])):.3e}, "
          f"E - E0 = {out['energy'] - e0:.3e}")
    if precision == 64:
        assert np.max(np.abs(out["alphas"] - checker["alphas"])) < TOL * weight
        assert np.max(np.abs(out["betas"] - checker["betas"])) < TOL * weight
        assert abs(out["energy"] - checker["energy"]) < TOL * weight
    else:
        assert abs(out["energy"] - e0) <= fp32_ref.C * max(abs(checker["energy"] - e0), fp32_ref.FLOOR * weight)
    rq, r = ref.rayleigh(y, terms)
    assert abs(rq - out["energy"]) < (TOL if precision == 64 else 1e-5) * weight  # the Ritz vector of three steps carries the Ritz value


@pytest.mark.parametrize("precision", PRECISIONS)
def test_random_hamiltonian_with_a_degenerate_ground_level(precision):
    """Strings of every weight; the two lowest levels are degenerate, so the vector is held only to |rq - E_0| <= r."""
    state, terms = ref.random_case()
    e0, _ = _levels("random")
    checker = _checker("random", precision)
    with Simulator(9, precision=precision) as sim:
        sim.write(state)
        out = _run(sim, 9, terms, _tol(precision, terms))
        y = sim.read()
    assert out["converged"] and out["steps"] < 200
    _check_vector(precision, out, y, terms, e0, "random n=9", checker=checker)


@pytest.mark.parametrize("precision", PRECISIONS)
def test_exhausted_krylov_spaces(precision):
    eps_tol = 1e-10 if precision == 64 else 1e-6
    # |0...0> is an eigenvector of the ZZ chain: one step, no division by beta = 0
    n, terms = 9, ref.zz_chain(9)
    with Simulator(n, precision=precision) as sim:
        out = _run(sim, n, terms, 1e-9 * adjoint_ref.weight(terms))
        y = sim.read()
    assert out["steps"] == 1 and out["converged"] and abs(out["energy"] + 8.0) < TOL * adjoint_ref.weight(terms)
    assert np.isfinite(y).all() and abs(abs(y[0]) - 1.0) < eps_tol and not y[1:].any() and out["residual"] < eps_tol * 8
    # one qubit: the Krylov space has two dimensions
    terms = [(1.0, 1, 0), (0.5, 0, 1)]
    with Simulator(1, precision=precision) as sim:
        sim.write(rand_state(1, 3))
        out = _run(sim, 1, terms, 0.0 if precision == 64 else 1e-6)
        y = sim.read()
    rq, r = ref.rayleigh(y, terms)
    print(f"one qubit p{precision}: steps {out['steps']}, E + sqrt(1.25) = {out['energy'] + np.sqrt(1.25):.3e}, residual {r:.3e}")
    assert out["steps"] <= 2 and out["converged"]
    assert abs(out["energy"] + np.sqrt(1.25)) < (TOL if precision == 64 else fp32_ref.C * fp32_ref.FLOOR) * 1.5
    assert abs(rq + np.sqrt(1.25)) <= max(r, 1e-15)
    # no qubit: H = 0.7 times the identity string
    with Simulator(0, precision=precision) as sim:
        out = _run(sim, 0, [(0.7, 0, 0)], 1e-9)
        assert out["steps"] == 1 and abs(out["energy"] - 0.7) < (TOL if precision == 64 else fp32_ref.C * fp32_ref.FLOOR) * 0.7
        assert abs(abs(sim.read()[0]) - 1.0) < eps_tol
    # H = 0: one step, energy 0
    with Simulator(5, precision=precision) as sim:
        sim.write(rand_state(5, 4))
        out = _run(sim, 5, [], 1e-9, vector=False)
        assert (out["steps"], out["energy"]) == (1, 0.0)


@pytest.mark.parametrize("precision", PRECISIONS)
def test_refusals_leave_the_state_alone(precision):
    n = 6
    terms = adjoint_ref.term_texts(ref.ising(n), n)
    with Simulator(n, precision=precision) as sim:
        sim.write(rand_state(n, 6))
        before = _bits(sim)
        calls = [lambda: sim.ground_state(terms, 1e-9, max_steps=0),
                 lambda: sim.ground_state(terms, -1.0),
                 lambda: sim.ground_state(terms, float("nan")),
                 lambda: sim.ground_state([(float("inf"), "Z0")], 1e-9)]
        for call in calls:
            with pytest.raises(_lib.QsimError) as err:
                call()
            assert err.value.code == _lib.ERR_ARG
            assert np.array_equal(_bits(sim), before)
        # a mask bit outside the register, through the C ABI
        import ctypes
        up, dp = ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_double)
        x, z, c = np.array([1 << n], dtype=np.uint64), np.zeros(1, dtype=np.uint64), np.ones(1)
        e, r, m = ctypes.c_double(), ctypes.c_double(), ctypes.c_int()
        rc = _lib.load().qsim_lanczos_ground(sim._h, x.ctypes.data_as(up), z.ctypes.data_as(up), c.ctypes.data_as(dp), 1, 10, 1e-9, 1, ctypes.byref(e),
                                             ctypes.byref(r), ctypes.byref(m), None, None)
        assert rc == _lib.ERR_ARG and np.array_equal(_bits(sim), before)
        with pytest.raises(ValueError):
            sim.ground_state([(1j, "Z0")], 1e-9)
        # a zero state: a shard that holds nothing, and a written vector of zeros
        sim.reset(holds_index0=False)
        with pytest.raises(_lib.QsimError) as err:
            sim.ground_state(terms, 1e-9)
        assert err.value.code == _lib.ERR_ARG and sim.get_support()[1:] == (True, 0.0)
        sim.write(np.zeros(1 << n, dtype=np.complex128))
        with pytest.raises(_lib.QsimError) as err:
            sim.ground_state(terms, 1e-9)
        assert err.value.code == _lib.ERR_ARG and not sim.read().any()


@pytest.mark.parametrize("precision", PRECISIONS)
def test_a_lent_spare_buffer_serves_as_a_work_buffer(precision):
    """A state with a lent spare buffer gives the result of one without, bit for bit."""
    state, terms = ref.ising_case()
    n, tol = ref.ISING_N, _tol(precision, terms)
    results = []
    for lend in (False, True):
        with Simulator(n, precision=precision) as sim, Simulator(n, precision=precision) as lender:
            if lend:
                ptr = lender.device_ptr
                lender.sync()
                sim.set_spare_buffer(ptr)
            sim.write(state)
            out = _run(sim, n, terms, tol, max_steps=12)
            results.append((out, _bits(sim)))
            if lend:
                sim.set_spare_buffer(None)
    (a, ya), (b, yb) = results
    assert a["energy"] == b["energy"] and a["residual"] == b["residual"] and a["steps"] == b["steps"] == 12
    assert np.array_equal(a["alphas"], b["alphas"]) and np.array_equal(a["betas"], b["betas"]) and np.array_equal(ya, yb)
