"""The tests' own checker for whole-register diagonal operators from a table (Diagonal, Simulator.apply_diagonal_phase,
Simulator.expectation_diagonal): a numpy restatement of what the device kernels compute (tests/test_diagonal_cpu.py pins it against
dense operators and against pauli_rot_ref's Z rotations), and the probe the GPU tests take their sizes from.

The table of D = sum_k c_k P_k (strings of I and Z): d_i = (...((0 + c_0 s_0(i)) + c_1 s_1(i)) + ...), s_k(i) = (-1)^popcount(i & z_k),
added in the caller's order — c s is an exact sign flip, so a device that adds in that order returns these bits exactly.
The phase: a_i <- exp(-i gamma d_i) a_i; for an fp32 state the factor is formed in fp64, rounded once to complex64, and multiplied
in complex64."""

import numpy as np

import pauli_ref


def signs(n, z):
    """s(i) = (-1)^popcount(i & z) for i < 2^n as +-1.0, built qubit by qubit: the upper half of each doubling is the lower half,
    negated where z has the bit (test_diagonal_cpu.py holds it to pauli_ref._parity)."""
    s = np.ones(1, dtype=np.float64)
    for q in range(n):
        s = np.concatenate([s, -s if z >> q & 1 else s])
    return s


def table_from_terms(n, terms, start=None):
    """terms = [(c, z)]: the sequential sum on top of `start` (default zeros), float64."""
    d = np.zeros(1 << n, dtype=np.float64) if start is None else np.array(start, dtype=np.float64, copy=True)
    for c, z in terms:
        d += np.float64(c) * signs(n, z)
    return d


def texts(terms, n):
    """[(c, z)] -> [(c, "Z0 Z7")] as Diagonal.from_terms takes them."""
    return [(c, pauli_ref.masks_to_text(0, z, n)) for c, z in terms]


def apply_phase(psi, d, gamma, dtype=np.complex128):
    factor = np.exp(-1j * (np.float64(gamma) * np.asarray(d, dtype=np.float64)))
    return (np.asarray(psi, dtype=dtype) * factor.astype(dtype)).astype(dtype)


def moments(psi, d):
    """(sum_i d_i |a_i|^2, sum_i d_i^2 |a_i|^2) in float64."""
    psi = np.asarray(psi, dtype=np.complex128)
    w = psi.real ** 2 + psi.imag ** 2
    d = np.asarray(d, dtype=np.float64)
    return float(np.sum(d * w)), float(np.sum(d * d * w))


def extrema(d):
    """min, argmin, max, argmax with the lowest index among equal values (numpy's argmin and argmax return the first)."""
    d = np.asarray(d, dtype=np.float64)
    lo, hi = int(np.argmin(d)), int(np.argmax(d))
    return {"min": float(d[lo]), "argmin": lo, "max": float(d[hi]), "argmax": hi}


def plan(n, precision):
    """plans.diagonal_plan as a dict (host only)."""
    from gpu_quantum_simulator_amd import plans
    return plans.ok(plans.diagonal_plan(n, precision))


def loop_n(precision):
    """The smallest n at which both sweeps make more than one trip per workgroup with the grid at its cap."""
    for n in range(41):
        p = plan(n, precision)
        if p["trips_at_cap_phase"] > 1 and p["trips_at_cap_expect"] > 1:
            return n
    raise AssertionError("no register size makes the sweeps loop")
