"""The tests' own checker for adjoint-mode gradients through diagonal phases (qsim_diagonal_gradient, csrc/diagonal.hip's
k_diag_adjoint and k_diag_apply): controlled_adjoint_ref's algorithm for a circuit whose steps are (controlled) Pauli
rotations OR diagonal phases exp(-i gamma D) of a real table, and an observable with a diagonal part (tests/test_diag_gradient_cpu.py
pins it against the chain rule through Z rotations and against dense operators), and the plan probe the GPU tests take their sizes from.

A step is (theta, c, x, z) as in controlled_rot_ref, or Diag(gamma, d) with d a float64 table of 2^n entries.  The observable is
H = sum_t c_t Q_t + w D_obs: `terms` = [(c, x, z)] and `obs` = (w, d_obs) or None.
U = exp(-i gamma D), dU/dgamma = -i D U, so with |lambda_K> = H |psi_K> and |lambda_(k-1)> = U_k^+ |lambda_k>
    dE/dgamma_k = 2 Re <lambda_k| (-i) D |psi_k> = 2 sum_i d_i Im(conj(lambda_i) psi_i),
taken from psi_k and lambda_k BEFORE the step back (D commutes with U: the product conj(lambda_i) psi_i is the same after it).
complex64: the factor of a phase is formed in fp64 and rounded once (diagonal_ref.apply_phase), w d_i likewise; every inner product in
fp64."""
from collections import namedtuple

import numpy as np

import controlled_rot_ref as crot
import diagonal_ref
import pauli_ref
from adjoint_ref import apply_pauli, apply_sum, dense_hamiltonian, weight  # noqa: F401

Diag = namedtuple("Diag", "gamma d")
TOL = 1e-10


def is_diag(step):
    return isinstance(step, Diag)


def apply_step(psi, step, dtype=np.complex128, inverse=False):
    sign = -1.0 if inverse else 1.0
    if is_diag(step):
        return diagonal_ref.apply_phase(psi, step.d, sign * step.gamma, dtype)
    theta, c, x, z = step
    return crot.apply_rotation(psi, c, x, z, sign * theta, dtype)


def replay(psi, steps, dtype=np.complex128):
    out = np.asarray(psi, dtype=dtype)
    for step in steps:
        out = apply_step(out, step, dtype)
    return out


def apply_observable(psi, terms, obs, dtype=np.complex128):
    """lambda = sum_t c_t Q_t psi + w D_obs psi in `dtype`; w d_i is formed in fp64 and rounded once."""
    lam = apply_sum(psi, terms, dtype)
    if obs is not None:
        w, d = obs
        real = np.float64 if dtype == np.complex128 else np.float32
        lam = (lam + (np.float64(w) * np.asarray(d, dtype=np.float64)).astype(real) * np.asarray(psi, dtype=dtype)).astype(dtype)
    return lam


def gradient(psi0, steps, terms, obs=None, dtype=np.complex128):
    """(E, grad, psi_K) by the adjoint algorithm: states, rotations and phases in `dtype`, every inner product in fp64."""
    psi = replay(psi0, steps, dtype)
    final = psi
    lam = apply_observable(psi, terms, obs, dtype)
    wide = np.complex128
    energy = float(np.vdot(lam.astype(wide), psi.astype(wide)).real)
    grad = np.zeros(len(steps))
    for k in range(len(steps) - 1, -1, -1):
        step = steps[k]
        if is_diag(step):
            grad[k] = 2.0 * float(np.sum(np.asarray(step.d, dtype=np.float64) * (np.conj(lam.astype(wide)) * psi.astype(wide)).imag))
        else:
            _, c, x, z = step
            j = np.arange(psi.size, dtype=np.uint64)
            inside = (j & np.uint64(c)) == np.uint64(c)
            grad[k] = float(np.vdot(lam.astype(wide)[inside], apply_pauli(psi, x, z).astype(wide)[inside]).imag)
        psi = apply_step(psi, step, dtype, inverse=True)
        lam = apply_step(lam, step, dtype, inverse=True)
    return energy, grad, final


def there_and_back(steps):
    """The steps, then their inverses, last first: what a gradient call does to the state."""
    back = [Diag(-s.gamma, s.d) if is_diag(s) else (-s[0],) + tuple(s[1:]) for s in steps[::-1]]
    return list(steps) + back


def expand(steps, table_terms):
    """Every Diag step whose table is table_from_terms(n, table_terms[k]) for its position k, spelled as the Z rotations
    exp(-i (2 gamma c_j)/2 Z-string_j): (rotations [(theta, c, x, z)], owner) with owner[i] = (k, 2 c_j) for a rotation that came from
    step k's term j and (k, None) for a rotation that is step k itself."""
    rotations, owner = [], []
    for k, step in enumerate(steps):
        if is_diag(step):
            for c, z in table_terms[k]:
                rotations.append((2.0 * step.gamma * c, 0, 0, z))
                owner.append((k, 2.0 * c))
        else:
            rotations.append(step)
            owner.append((k, None))
    return rotations, owner


def chain_rule(grad_expanded, owner, num_steps):
    """dE/dgamma_k = sum_j 2 c_j dE/dtheta_j over the rotations of step k; a rotation step keeps its own component."""
    out = np.zeros(num_steps)
    for g, (k, factor) in zip(grad_expanded, owner):
        out[k] += g if factor is None else factor * g
    return out


def dense_step(step, n):
    if is_diag(step):
        return np.diag(np.exp(-1j * step.gamma * np.asarray(step.d, dtype=np.float64)))
    theta, c, x, z = step
    return crot.dense_controlled(c, x, z, n, theta)


def dense_gradient(psi0, steps, terms, obs, n):
    """(E, grad) from dense operators: dE/dangle_k = 2 Re <psi_K| H U_K ... U_(k+1) G_k U_k ... U_1 |psi_0> with G_k = -i D_k for a
    diagonal step and -(i/2) Pi_k P_k for a rotation."""
    N = 1 << n
    H = dense_hamiltonian(terms, n) if terms else np.zeros((N, N), dtype=np.complex128)
    if obs is not None:
        H = H + obs[0] * np.diag(np.asarray(obs[1], dtype=np.float64))
    us = [dense_step(s, n) for s in steps]
    psi = np.asarray(psi0, dtype=np.complex128)
    for u in us:
        psi = u @ psi
    grad = np.zeros(len(steps))
    for k, step in enumerate(steps):
        v = np.asarray(psi0, dtype=np.complex128)
        for u in us[:k + 1]:
            v = u @ v
        if is_diag(step):
            v = -1j * np.asarray(step.d, dtype=np.float64) * v
        else:
            _, c, x, z = step
            j = np.arange(N)
            v = -0.5j * (((j & c) == c) * (pauli_ref.dense_pauli(x, z, n) @ v))
        for u in us[k + 1:]:
            v = u @ v
        grad[k] = 2.0 * np.vdot(psi, H @ v).real
    return float(np.vdot(psi, H @ psi).real), grad


def observable_weight(terms, obs):
    """W = sum|c_t| + |w| max|d|: the scale of E and of lambda."""
    return weight(terms) + (abs(obs[0]) * float(np.max(np.abs(obs[1]))) if obs is not None else 0.0)


# ---- the plan probe (host only) -------------------------------------------------------------------------------------------------------
def plan_call(is_diag_flags, cs, xs, ham_x, has_obs, n, precision, null_flags=False, null_controls=False):
    """plans.diagonal_gradient_plan with arrays: (return code, dict)."""
    from gpu_quantum_simulator_amd import plans
    return plans.diagonal_gradient_plan(None if null_flags else is_diag_flags, None if null_controls else cs, xs, ham_x, 1 if has_obs else 0, n, precision)


def plan(steps, terms, obs, n, precision=64):
    """The plan of a step list and an observable as gradient() takes them."""
    from gpu_quantum_simulator_amd import _lib
    flags = [1 if is_diag(s) else 0 for s in steps]
    cs = [0 if is_diag(s) else s[1] for s in steps]
    xs = [0 if is_diag(s) else s[2] for s in steps]
    rc, out = plan_call(flags, cs, xs, [x for _, x, _ in terms], obs is not None, n, precision)
    _lib.check(rc)
    return out


def loop_n(precision):
    """The smallest n at which the backward diagonal sweep makes more than one trip per workgroup with the grid at its cap."""
    for n in range(41):
        if plan([Diag(0.0, None)], [], None, n, precision)["diag_adjoint_trips_at_cap"] > 1:
            return n
    raise AssertionError("no register size makes the sweep loop")


# ---- how the GPU tests hand steps and observables to Simulator.energy_and_gradient -------------------------------------------------------
def entries(steps, n, tables):
    """steps -> the entries energy_and_gradient takes; tables[id(step.d)] is the Diagonal that holds a Diag step's table."""
    out = []
    for s in steps:
        if is_diag(s):
            out.append((s.gamma, tables[id(s.d)]))
        else:
            theta, c, x, z = s
            out.append((theta, pauli_ref.masks_to_text(x, z, n), crot.controls_of(c, n)))
    return out


def observable(terms, obs, n, tables):
    texts = [(c, pauli_ref.masks_to_text(x, z, n)) for c, x, z in terms]
    return texts if obs is None else texts + [(obs[0], tables[id(obs[1])])]
