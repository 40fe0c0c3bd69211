"""Pauli-list arguments as the C ABI takes them, and `_PauliStrings`: what Simulator and Cluster share."""
from __future__ import annotations

import numpy as np

from . import _lib, _marshal
from ._marshal import dp as _dp
from .pauli import control_mask, pauli_masks, trotter_rotations


def _mask_arrays(masks):
    """[(x, z)] as two uint64 arrays and their pointers: xs, zs, xp, zp."""
    (xs, xp), (zs, zp) = _marshal.masks(m[0] for m in masks), _marshal.masks(m[1] for m in masks)
    return xs, zs, xp, zp


def _pauli_term_masks(paulis, num_q: int):
    """Distinct strings of `paulis` as mask arrays, and for every entry the position of its string among them."""
    index, where = {}, []
    for text in paulis:
        where.append(index.setdefault(pauli_masks(text, num_q), len(index)))
    return _mask_arrays(index) + (np.array(where, dtype=np.intp),)


def _rotation_arrays(rotations, num_q: int):
    """(theta, string) pairs as the arrays qsim_apply_pauli_rotations takes, in order: xs, zs, thetas and their pointers."""
    rotations = list(rotations)
    xs, zs, xp, zp = _mask_arrays([pauli_masks(text, num_q) for _, text in rotations])
    thetas = np.array([float(theta) for theta, _ in rotations], dtype=np.float64)
    return xs, zs, thetas, xp, zp, _dp(thetas)


def _split_controls(rotations):
    """(theta, string) and (theta, string, controls) entries, mixed, as ([(theta, string)], [controls]); controls () where none."""
    pairs, controls = [], []
    for entry in rotations:
        entry = tuple(entry)
        if len(entry) not in (2, 3):
            raise ValueError(f"a rotation is (theta, string) or (theta, string, controls), not {entry!r}")
        pairs.append(entry[:2])
        controls.append(tuple(entry[2]) if len(entry) == 3 else ())
    return pairs, controls


def _control_masks(pairs, controls, num_q: int):
    """The control sets of _split_controls as the uint64 array the controlled calls take, and its pointer; (None, None) where no
    entry has controls.  ValueError (pauli.control_mask) for a control named twice, outside the register or named by its string."""
    if not any(controls):
        return None, None
    return _marshal.masks(control_mask(c, num_q, text) for (_, text), c in zip(pairs, controls))


def _hamiltonian_arrays(terms, num_q: int):
    """(real coefficient, string) pairs as the arrays qsim_pauli_gradient and qsim_pauli_sum_into take: xs, zs, coeffs and their
    pointers.  ValueError for a complex coefficient."""
    terms = list(terms)
    for coeff, text in terms:
        if _marshal.is_complex(coeff):
            raise ValueError(f"coefficient {coeff!r} of {text!r} is complex: a Hamiltonian's coefficients are real")
    return _rotation_arrays(terms, num_q)  # the same layout: masks, float64 weights, their pointers


def _weighted_sum(terms, evaluate):
    """sum_t c_t <P_t> for (coefficient, string) pairs: a float when every coefficient is real, else a complex."""
    terms = list(terms)
    coeffs = [c for c, _ in terms]
    values = evaluate([p for _, p in terms])
    if all(isinstance(c, (int, float, np.integer, np.floating)) for c in coeffs):
        return float(np.dot(np.asarray(coeffs, dtype=np.float64), values))
    return complex(np.dot(np.asarray(coeffs, dtype=np.complex128), values))


class _PauliStrings:
    """Pauli strings on a state: what Simulator and Cluster share.  A class names its two C functions (_expect_fn, _rotate_fn) and
    has _check(rc); the strings of a Cluster name LOGICAL qubits."""

    def expectation_terms(self, paulis) -> np.ndarray:
        """<psi|P|psi> for every Pauli string of `paulis` ("X0 Z3 Y17", see pauli_masks), computed on the device
        (qsim_expect_paulis, qsim_cluster_expect_paulis): one float64 per string, in the caller's order.  Equal strings are
        evaluated once.  On a Cluster the strings name LOGICAL qubits."""
        xs, zs, xp, zp, where = _pauli_term_masks(paulis, self.num_qubits)
        out = np.empty(xs.size, dtype=np.float64)
        self._check(getattr(_lib.load(), self._expect_fn)(self._h, xp, zp, xs.size, _dp(out)))
        return out[where]

    def expectation(self, terms):
        """sum_t c_t <P_t> for an iterable of (coefficient, Pauli string): <psi|H|psi> of H = sum_t c_t P_t.  A float when
        every coefficient is real, else a complex."""
        return _weighted_sum(terms, self.expectation_terms)

    def apply_pauli_rotation(self, theta: float, pauli: str, controls=()) -> None:
        """state <- exp(-i theta/2 P) state for the Pauli string P ("X0 Y3 Z17", see pauli_masks); on a Cluster the string
        names LOGICAL qubits.  `controls` (a Simulator only): qubit numbers; the rotation then acts where all of them are 1."""
        self.apply_pauli_rotations([(theta, pauli, controls)])

    def apply_pauli_rotations(self, rotations) -> None:
        """exp(-i theta/2 P) for every (theta, string) of `rotations`, the first one first, as ONE call of
        qsim_apply_pauli_rotations (qsim_cluster_apply_pauli_rotations): consecutive strings with X/Y on the same qubits share
        a sweep of the state.  Returns without waiting.
        An entry may be (theta, string, controls) instead, controls being qubit numbers: that rotation acts only where every
        control qubit is 1 (qsim_apply_controlled_pauli_rotations: a sweep of 2^-c of the state for c controls; consecutive
        terms share it under one control set).  ValueError for a control named twice, outside the register, or named by the
        string too — and for any control on a Cluster: sharded states have no controlled rotations yet."""
        pairs, controls = _split_controls(rotations)
        xs, zs, thetas, xp, zp, tp = _rotation_arrays(pairs, self.num_qubits)
        if any(controls):
            self._apply_controlled(pairs, controls, xp, zp, tp)
        else:
            self._check(getattr(_lib.load(), self._rotate_fn)(self._h, xp, zp, tp, xs.size))

    def _apply_controlled(self, pairs, controls, xp, zp, tp) -> None:
        raise ValueError("sharded states have no controlled rotations yet")

    def evolve(self, terms, time: float, steps: int = 1, order: int = 1) -> None:
        """A product formula for exp(-i H time) with H = sum_k c_k P_k given as (c_k, string) pairs, real c_k
        (pauli.trotter_rotations builds the list: order 1 or 2, `steps` steps), applied as one call."""
        self.apply_pauli_rotations(trotter_rotations(terms, time, steps, order))

