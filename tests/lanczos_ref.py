"""The tests' own checker for the Lanczos ground-state solver (qsim_lanczos_ground, csrc/lanczos.cpp): a numpy restatement of the
recurrence in the device's order on top of adjoint_ref.apply_sum (tests/test_lanczos_cpu.py pins it against dense operators), the
two-pass Ritz vector, and the cases of tests/test_gpu_lanczos.py as data.

Recurrence: v_0 = state / |state|; step j: w = H v_j, alpha_j = Re <v_j|w>, w <- w - alpha_j v_j - beta_(j-1) v_(j-1), beta_j = |w|,
v_(j+1) = w / beta_j; no reorthogonalisation.  As on the device the buffers hold the UNNORMALISED w with norms nu_j known in fp64
(nu_0 = |state|, nu_(j+1) = beta_j), 1 / nu is folded into the coefficients, coefficients are rounded once to the vectors' dtype,
multiply-adds run in that dtype, inner products and norms in fp64.  After every step the tridiagonal is solved (numpy.linalg.eigh
here; the device's own solver is pinned against it) and beta_j |t_last| estimates the residual."""
import numpy as np

import adjoint_ref
from pauli_rot_ref import rand_state

WIDE = np.complex128


def _real(dtype):
    return np.float64 if dtype == np.complex128 else np.float32


def _eps(dtype):
    return 2.0 ** -53 if dtype == np.complex128 else 2.0 ** -24


def tridiag(alphas, betas):
    m = len(alphas)
    T = np.diag(np.asarray(alphas, dtype=np.float64))
    for i in range(m - 1):
        T[i, i + 1] = T[i + 1, i] = betas[i]
    return T


def lowest(alphas, betas):
    """(theta, t): the lowest eigenpair of the tridiagonal of alphas[0..m), betas[0..m-1)."""
    w, v = np.linalg.eigh(tridiag(alphas, betas))
    return float(w[0]), v[:, 0]


def _apply_h(vec, nu, terms, dtype):
    return adjoint_ref.apply_sum(vec, [(c / nu, x, z) for c, x, z in terms], dtype)


def _update(w, alpha, cur, nu_cur, prev, beta_prev, nu_prev, dtype):
    real = _real(dtype)
    out = (w + real(-alpha / nu_cur) * cur).astype(dtype)
    if prev is not None:
        out = (out + real(-beta_prev / nu_prev) * prev).astype(dtype)
    return out


def _norm(v):
    return float(np.sqrt(np.vdot(v.astype(WIDE), v.astype(WIDE)).real))


def lanczos(state, terms, tol, max_steps=200, dtype=np.complex128, vector=True):
    """dict(energy, residual, steps, alphas, betas, estimate, y): the recurrence from `state` in `dtype`.  residual: the estimate
    beta |t_last|, or with `vector` the measured |H y - theta y| of the unit Ritz vector y (second pass with the recorded alphas and
    betas), all inner products in fp64."""
    v0 = np.asarray(state).astype(dtype)
    floor_beta = 64.0 * _eps(dtype) * adjoint_ref.weight(terms)
    nu = [_norm(v0)]
    al, be = [], []
    cur, prev = v0, None
    theta, t, estimate = 0.0, None, 0.0
    for j in range(max_steps):
        w = _apply_h(cur, nu[j], terms, dtype)
        alpha = float(np.vdot(cur.astype(WIDE), w.astype(WIDE)).real) / nu[j]
        w = _update(w, alpha, cur, nu[j], prev, be[j - 1] if j else 0.0, nu[j - 1] if j else 1.0, dtype)
        beta = _norm(w)
        al.append(alpha)
        be.append(beta)
        nu.append(beta)
        theta, t = lowest(al, be[:-1])
        estimate = beta * abs(t[-1])
        if estimate <= tol or beta <= floor_beta:
            break
        prev, cur = cur, w
    m = len(al)
    out = {"energy": theta, "steps": m, "alphas": np.array(al), "betas": np.array(be), "estimate": estimate, "residual": estimate, "y": None}
    if not vector:
        return out
    real = _real(dtype)
    y = (real(t[0] / nu[0]) * v0).astype(dtype)
    cur, prev = v0, None
    for j in range(m - 1):
        w = _apply_h(cur, nu[j], terms, dtype)
        w = _update(w, al[j], cur, nu[j], prev, be[j - 1] if j else 0.0, nu[j - 1] if j else 1.0, dtype)
        y = (y + real(t[j + 1] / nu[j + 1]) * w).astype(dtype)
        prev, cur = cur, w
    ny = _norm(y)
    r = (_apply_h(y, ny, terms, dtype) + real(-theta / ny) * y).astype(dtype)
    out["residual"] = _norm(r)
    out["y"] = (real(1.0 / ny) * y).astype(dtype)
    return out


def rayleigh(y, terms):
    """(rq, |H y - rq y| / |y|) in fp64."""
    y = np.asarray(y, dtype=WIDE)
    hy = adjoint_ref.apply_sum(y, terms)
    n2 = float(np.vdot(y, y).real)
    rq = float(np.vdot(y, hy).real) / n2
    return rq, float(np.linalg.norm(hy - rq * y) / np.sqrt(n2))


# ---- the cases, as data ---------------------------------------------------------------------------------------------------------------
def ising(n, J=1.0, h=1.5):
    """Transverse-field Ising chain, open ends: -J sum Z_q Z_(q+1) - h sum X_q as [(c, x, z)]."""
    return [(-J, 0, 0b11 << q) for q in range(n - 1)] + [(-h, 1 << q, 0) for q in range(n)]


ISING_N, ISING_SEED = 10, 5
ISING_GAP = 1.167  # E_1 - E_0 of ising(10), to the digits given


def ising_case():
    return rand_state(ISING_N, ISING_SEED), ising(ISING_N)


def random_case():
    """Strings of every weight on 9 qubits; the two lowest levels are degenerate."""
    return rand_state(9, 12), adjoint_ref.random_hamiltonian(9, 12, 309, 2)


def zz_chain(n):
    return [(-1.0, 0, 0b11 << q) for q in range(n - 1)]


def wilkinson_negated(m=21):
    """-W_m^+: diagonal -|i - (m-1)/2|, off-diagonal -1; its two lowest eigenvalues agree to about 1e-14 relative."""
    half = (m - 1) // 2
    return np.array([-abs(i - half) for i in range(m)], dtype=np.float64), -np.ones(m - 1)
