"""Host side of the Lanczos ground-state solver, no GPU: the tridiagonal eigensolver qsim_tridiag_lowest against numpy.linalg.eigh,
the host-only plan plans.lanczos_plan against sweep counts worked out by hand, and the numpy checker tests/lanczos_ref.py pinned
against dense operators.

Bounds.  With |T| := max|alpha| + 2 max|beta| (a Gershgorin bound on the spectrum) LAPACK's own accuracy is a few eps |T|; the
solver is held to 1e-12 |T| for the eigenvalue and for the residual |T t - theta t| of its unit vector.  The vector itself is not
compared: it is ambiguous when the lowest pair is nearly degenerate.  The checker is held to the Hermitian residual bound
|rq(y) - E_0| <= |H y - rq y|, which is derived, not tuned."""
import ctypes

import numpy as np
import pytest

import adjoint_ref
import lanczos_ref as ref
from gpu_quantum_simulator_amd import _lib, plans

DP = ctypes.POINTER(ctypes.c_double)
UP = ctypes.POINTER(ctypes.c_uint64)


def _lowest(alphas, betas, want_vec=True):
    al = np.ascontiguousarray(alphas, dtype=np.float64)
    be = np.ascontiguousarray(betas, dtype=np.float64)
    theta, vec = ctypes.c_double(), np.zeros(al.size)
    _lib.check(_lib.load().qsim_tridiag_lowest(al.ctypes.data_as(DP), be.ctypes.data_as(DP) if be.size else None, al.size, ctypes.byref(theta),
                                               vec.ctypes.data_as(DP) if want_vec else None))
    return theta.value, vec


def _check_tridiag(alphas, betas, label):
    theta, t = _lowest(alphas, betas)
    T = ref.tridiag(alphas, betas)
    want = float(np.linalg.eigvalsh(T)[0])
    norm = float(np.max(np.abs(alphas))) + 2.0 * (float(np.max(np.abs(betas))) if len(betas) else 0.0)
    res = float(np.linalg.norm(T @ t - theta * t))
    print(f"{label}: m={len(alphas)} |theta - numpy| = {abs(theta - want):.3e}, residual {res:.3e}, |t| - 1 = {np.linalg.norm(t) - 1:.3e}, |T| = {norm:.3f}")
    assert abs(theta - want) <= 1e-12 * norm
    assert abs(float(np.linalg.norm(t)) - 1.0) <= 1e-12
    assert res <= 1e-12 * norm
    assert _lowest(alphas, betas, want_vec=False)[0] == theta


@pytest.mark.parametrize("m", [1, 2, 3, 50, 300])
def test_tridiag_lowest_random(m):
    rng = np.random.default_rng(4000 + m)
    _check_tridiag(rng.uniform(-2, 2, m), rng.uniform(0.05, 1.5, m - 1), "random")


def test_tridiag_lowest_zero_beta_in_the_middle():
    rng = np.random.default_rng(4100)
    betas = rng.uniform(0.1, 1.0, 39)
    betas[17] = 0.0
    _check_tridiag(rng.uniform(-1, 1, 40), betas, "zero beta")


def test_tridiag_lowest_nearly_degenerate_pair():
    alphas, betas = ref.wilkinson_negated(21)
    w = np.linalg.eigvalsh(ref.tridiag(alphas, betas))
    assert w[1] - w[0] < 1e-12 * abs(w[0])  # the case is what it says
    _check_tridiag(alphas, betas, "negated Wilkinson W21+")


def test_tridiag_lowest_refuses_bad_arguments():
    lib = _lib.load()
    one, th = np.ones(3), ctypes.c_double()
    assert lib.qsim_tridiag_lowest(one.ctypes.data_as(DP), one.ctypes.data_as(DP), 0, ctypes.byref(th), None) == _lib.ERR_ARG
    assert lib.qsim_tridiag_lowest(None, one.ctypes.data_as(DP), 3, ctypes.byref(th), None) == _lib.ERR_ARG
    assert lib.qsim_tridiag_lowest(one.ctypes.data_as(DP), None, 3, ctypes.byref(th), None) == _lib.ERR_ARG
    assert lib.qsim_tridiag_lowest(one.ctypes.data_as(DP), one.ctypes.data_as(DP), 3, None, None) == _lib.ERR_ARG
    bad = np.array([0.0, np.nan, 1.0])
    assert lib.qsim_tridiag_lowest(bad.ctypes.data_as(DP), one.ctypes.data_as(DP), 3, ctypes.byref(th), None) == _lib.ERR_ARG


def _plan(terms, max_steps=10, vector=1):
    rc, p = plans.lanczos_plan([x for _, x, _ in terms] or None, max_steps, vector)
    return rc, p["sum_sweeps_per_step"], p["other_sweeps_per_step"], p["volumes_per_step"]


@pytest.mark.parametrize("n", [2, 10, 30])
def test_plan_ising_chain(n):
    """2n - 1 terms: the ZZ terms share x = 0 (one sweep), every X_q is an x group of its own: G = 1 + n sweeps; the first stores (2
    volumes), the others accumulate (3), alpha reads two vectors, the update reads three and writes one."""
    assert plans.pauli_terms_per_sweep() >= 29  # the ZZ group of n = 30 fits one sweep
    rc, sums, others, volumes = _plan(ref.ising(n))
    assert (rc, sums, others) == (0, 1 + n, 2)
    assert volumes == 3 * (1 + n) - 1 + 2 + 4


def test_plan_all_z_and_empty():
    assert _plan(ref.zz_chain(30)) == (0, 1, 2, 2.0 + 2.0 + 4.0)
    assert _plan([]) == (0, 0, 2, 1.0 + 2.0 + 4.0)  # H = 0: one fill of w
    assert _plan(ref.zz_chain(5), vector=0) == _plan(ref.zz_chain(5), vector=1)
    assert _plan(ref.zz_chain(5), max_steps=0)[0] == _lib.ERR_ARG
    lib = _lib.load()
    hx = np.zeros(2, dtype=np.uint64)
    assert lib.qsim_lanczos_plan(hx.ctypes.data_as(UP), 2, 5, 0, None, None, None) == _lib.ERR_ARG  # raw: NULL for the out-parameters


def test_checker_against_dense_operators():
    """Transverse-field Ising, n = 10, J = 1, h = 1.5, from rand_state(10, 5): measured here 46 steps, E - E_0 = 5e-14, estimated and
    true residual equal to 9 digits."""
    state, terms = ref.ising_case()
    weight = adjoint_ref.weight(terms)
    tol = 1e-9 * weight
    levels = np.linalg.eigvalsh(adjoint_ref.dense_hamiltonian(terms, ref.ISING_N))
    e0 = float(levels[0])
    assert abs((levels[1] - levels[0]) - ref.ISING_GAP) < 1e-3
    out = ref.lanczos(state, terms, tol, 200)
    rq, r = ref.rayleigh(out["y"], terms)
    print(f"ising n=10: steps {out['steps']}, E - E0 = {out['energy'] - e0:.3e}, estimate {out['estimate']:.6e}, measured {out['residual']:.6e}, "
          f"true {r:.6e}, rq - E0 = {rq - e0:.3e}")
    assert out["steps"] < 200 and out["estimate"] <= tol
    assert out["energy"] >= e0 - 1e-10 * weight
    assert abs(rq - e0) <= r
    assert abs(float(np.vdot(out["y"], out["y"]).real) - 1.0) < 1e-12
    # the complex64 run of the same case converges at the fp32 tolerance of the GPU test, and its energy sits inside the fp32 rule
    import fp32_ref
    out32 = ref.lanczos(state.astype(np.complex64), terms, 1e-5 * weight, 200, np.complex64)
    print(f"ising n=10 complex64: steps {out32['steps']}, |E - E0| = {abs(out32['energy'] - e0):.3e}, floor term {fp32_ref.FLOOR * weight * fp32_ref.C:.3e}")
    assert out32["steps"] < 200
    assert abs(out32["energy"] - e0) <= fp32_ref.C * fp32_ref.FLOOR * weight


def test_checker_on_a_degenerate_ground_level():
    state, terms = ref.random_case()
    weight = adjoint_ref.weight(terms)
    levels = np.linalg.eigvalsh(adjoint_ref.dense_hamiltonian(terms, 9))
    assert levels[1] - levels[0] < 1e-9 * weight  # the case is what it says
    out = ref.lanczos(state, terms, 1e-9 * weight, 200)
    rq, r = ref.rayleigh(out["y"], terms)
    print(f"random n=9: steps {out['steps']}, E - E0 = {out['energy'] - levels[0]:.3e}, residual {r:.3e}")
    assert out["steps"] < 200
    assert abs(rq - float(levels[0])) <= r
