"""Kraus lists for Simulator.apply_channel: the standard one- and two-qubit noise channels as lists of complex128 matrices K_i with
sum_i K_i^dagger K_i = 1.  Pure numpy, no native code: usable and testable without a device or the library.

Bit j of a row or column index of a matrix is qubit targets[j] of the call that applies it (the convention of Simulator.apply_matrix).
Every builder raises ValueError for a parameter outside [0, 1]; an operator of weight zero stays in the list as the zero matrix, so that
an index means the same whatever the parameter (apply_channel never picks an index of probability zero)."""
from __future__ import annotations

import math

import numpy as np

I2 = np.eye(2, dtype=np.complex128)
X = np.array([[0, 1], [1, 0]], dtype=np.complex128)
Y = np.array([[0, -1j], [1j, 0]], dtype=np.complex128)
Z = np.array([[1, 0], [0, -1]], dtype=np.complex128)
PAULIS = (I2, X, Y, Z)
TRACE_TOLERANCE = 1e-9  # apply_channel refuses a list whose sum K^dagger K is farther from the identity than this, in max abs


def _unit(value, what: str) -> float:
    v = float(value)
    if not 0.0 <= v <= 1.0:
        raise ValueError(f"{what}: a number in [0, 1] is wanted, got {value!r}")
    return v


def bit_flip(p) -> list:
    """X with probability p: [sqrt(1 - p) I, sqrt(p) X]."""
    p = _unit(p, "bit_flip")
    return [math.sqrt(1.0 - p) * I2, math.sqrt(p) * X]


def phase_flip(p) -> list:
    """Z with probability p: [sqrt(1 - p) I, sqrt(p) Z]."""
    p = _unit(p, "phase_flip")
    return [math.sqrt(1.0 - p) * I2, math.sqrt(p) * Z]


def depolarizing(p) -> list:
    """rho -> (1 - p) rho + p/3 (X rho X + Y rho Y + Z rho Z): [sqrt(1 - p) I, sqrt(p/3) X, sqrt(p/3) Y, sqrt(p/3) Z]."""
    p = _unit(p, "depolarizing")
    return [math.sqrt(1.0 - p) * I2] + [math.sqrt(p / 3.0) * P for P in (X, Y, Z)]


def amplitude_damping(gamma) -> list:
    """|1> decays to |0> with probability gamma: [[1, 0], [0, sqrt(1 - gamma)]] and [[0, sqrt(gamma)], [0, 0]]."""
    g = _unit(gamma, "amplitude_damping")
    return [np.array([[1, 0], [0, math.sqrt(1.0 - g)]], dtype=np.complex128), np.array([[0, math.sqrt(g)], [0, 0]], dtype=np.complex128)]


def phase_damping(gamma) -> list:
    """The off-diagonal of rho shrinks by sqrt(1 - gamma), no population moves: [[1, 0], [0, sqrt(1 - gamma)]] and [[0, 0], [0, sqrt(gamma)]]."""
    g = _unit(gamma, "phase_damping")
    return [np.array([[1, 0], [0, math.sqrt(1.0 - g)]], dtype=np.complex128), np.array([[0, 0], [0, math.sqrt(g)]], dtype=np.complex128)]


def two_qubit_depolarizing(p) -> list:
    """rho -> (1 - p) rho + p/15 sum over the 15 non-identity two-qubit Paulis P rho P: 16 operators, index 4 a + b being
    P_a on targets[1] (x) P_b on targets[0] with (I, X, Y, Z) numbered 0 to 3; index 0 is sqrt(1 - p) times the identity."""
    p = _unit(p, "two_qubit_depolarizing")
    out = []
    for a in range(4):
        for b in range(4):
            w = math.sqrt(1.0 - p) if a == b == 0 else math.sqrt(p / 15.0)
            out.append(w * np.kron(PAULIS[a], PAULIS[b]))
    return out


def as_kraus_list(kraus, num_targets: int) -> list:
    """`kraus` as a list of (2^k, 2^k) complex128 arrays after the checks of Simulator.apply_channel: at least one operator, every one
    of that shape, and sum K^dagger K within TRACE_TOLERANCE of the identity."""
    dim = 1 << num_targets
    ks = [np.asarray(K, dtype=np.complex128) for K in kraus]
    if not ks or any(K.shape != (dim, dim) for K in ks):
        raise ValueError(f"apply_channel: {num_targets} targets take a non-empty list of matrices of shape ({dim}, {dim})")
    gap = float(np.max(np.abs(sum(K.conj().T @ K for K in ks) - np.eye(dim))))
    if not gap <= TRACE_TOLERANCE:
        raise ValueError(f"apply_channel: the list is not trace-preserving: sum K^dagger K differs from the identity by {gap:.3g} "
                         f"(more than {TRACE_TOLERANCE:g}); the one trajectory step there is keeps the norm")
    return ks


def probabilities(kraus, rho) -> np.ndarray:
    """p_i = Re Tr(K_i rho K_i^dagger) / Tr rho for the (unnormalised) reduced density matrix `rho` of the targets; rounding below zero
    is cut off at zero."""
    total = float(np.real(np.trace(rho)))
    return np.array([max(float(np.real(np.trace(K @ rho @ K.conj().T))), 0.0) for K in kraus], dtype=np.float64) / total


def pick(p, draw: float) -> int:
    """The index a draw in [0, 1] picks: the first i with p_i > 0 whose running sum p_0 + ... + p_i reaches draw * sum(p) — the draw is
    scaled by the list's own total, so rounding in it cannot leave a draw of 1 without an index — else the last i with p_i > 0."""
    p = np.asarray(p, dtype=np.float64)
    positive = np.flatnonzero(p > 0.0)
    if positive.size == 0:
        raise ValueError("apply_channel: every operator has probability zero")
    running = np.cumsum(p)
    r = float(draw) * running[-1]
    for i in positive:
        if running[i] >= r:
            return int(i)
    return int(positive[-1])
