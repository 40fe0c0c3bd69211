"""`Diagonal` = qsim_diagonal, a real table on the device, and the parsers of energy_and_gradient's diagonal steps and observable."""
from __future__ import annotations

from ctypes import byref, c_double, c_uint64, c_void_p
from typing import Optional

import numpy as np

from . import _lib, _marshal
from ._lib import check
from ._marshal import dp as _dp, is_complex as _is_complex
from .pauli import pauli_masks


def _diagonal_term_arrays(terms, num_q: int):
    """(real coefficient, string of I and Z) pairs as the arrays qsim_diagonal_add_terms takes: zs, coeffs and their pointers.
    ValueError for an X or Y factor or a complex coefficient — pure Python, before anything touches the library."""
    terms = list(terms)
    masks = []
    for coeff, text in terms:
        if _is_complex(coeff):
            raise ValueError(f"coefficient {coeff!r} of {text!r} is complex: a diagonal table is real")
        x, z = pauli_masks(text, num_q)
        if x:
            raise ValueError(f"{text!r} has an X or Y factor: a diagonal operator is a sum of strings of I and Z")
        masks.append(z)
    zs, zp = _marshal.masks(masks)
    coeffs = np.array([float(c) for c, _ in terms], dtype=np.float64)
    return zs, coeffs, zp, _dp(coeffs)


class Diagonal(_lib.Handle):
    """A real table d[0..2^n) of float64 on one GPU: the operator D = sum_i d_i |i><i| on a register of n qubits (qsim_diagonal).
    Simulator.apply_diagonal_phase applies exp(-i gamma D) and Simulator.expectation_diagonal returns <D>, each in one sweep
    whatever the number of terms D has.  `ptr` adopts 2^n float64 values already on the device (tensor.data_ptr() of a torch
    tensor, say); the caller keeps them alive and nothing is freed.  Calls take effect in the order issued."""
    _free = "qsim_diagonal_destroy"

    def __init__(self, num_q: int, device: int = 0, ptr: Optional[int] = None):
        self._h = c_void_p()
        lib = _lib.load()
        if ptr is None:
            check(lib.qsim_diagonal_create(byref(self._h), num_q, device))
        else:
            check(lib.qsim_diagonal_create_external(byref(self._h), num_q, device, c_void_p(ptr)))
        self.num_qubits = num_q

    @classmethod
    def from_terms(cls, num_q: int, terms, device: int = 0) -> "Diagonal":
        """The diagonal of sum_k c_k P_k for (c_k, string) pairs, strings of I and Z only ("Z0 Z7"): ValueError for X or Y,
        before any launch."""
        arrays = _diagonal_term_arrays(terms, num_q)
        diag = cls(num_q, device)
        diag._add(arrays)
        return diag

    def _add(self, arrays) -> None:
        zs, coeffs, zp, cp = arrays
        check(_lib.load().qsim_diagonal_add_terms(self._h, zp, cp, zs.size))

    def add_terms(self, terms) -> None:
        """d_i += c_k (-1)^popcount(i & z_k), term after term in the order given: bit for bit the sequential sum."""
        self._add(_diagonal_term_arrays(terms, self.num_qubits))

    def write(self, values, first: int = 0) -> None:
        v = np.ascontiguousarray(values, dtype=np.float64)
        check(_lib.load().qsim_diagonal_write(self._h, first, v.size, _dp(v)))

    def read(self, first: int = 0, count: Optional[int] = None) -> np.ndarray:
        if count is None:
            count = (1 << self.num_qubits) - first
        out = np.empty(count, dtype=np.float64)
        check(_lib.load().qsim_diagonal_read(self._h, first, count, _dp(out)))
        return out

    def extrema(self) -> dict:
        """{"min", "argmin", "max", "argmax"} of the table, one reduction on the device; among equal values the lowest index."""
        lo, hi, ilo, ihi = c_double(), c_double(), c_uint64(), c_uint64()
        check(_lib.load().qsim_diagonal_extrema(self._h, byref(lo), byref(ilo), byref(hi), byref(ihi)))
        return {"min": float(lo.value), "argmin": int(ilo.value), "max": float(hi.value), "argmax": int(ihi.value)}

    def device_ptr(self) -> int:
        return int(_lib.load().qsim_diagonal_device_ptr(self._h) or 0)


def _split_diagonal_steps(rotations):
    """The entries of energy_and_gradient's `rotations`, (gamma, Diagonal) steps among them, as (entries, tables): an entry that is
    a diagonal phase has its table in `tables` (None elsewhere) and (gamma, "") — the identity string, which the library does not
    look at — in its place.  ValueError for controls on a diagonal entry, a complex gamma, a closed table.  Pure Python."""
    entries, tables = [], []
    for entry in rotations:
        entry = tuple(entry)
        if len(entry) >= 2 and isinstance(entry[1], Diagonal):
            if len(entry) > 3 or (len(entry) == 3 and tuple(entry[2])):
                raise ValueError(f"a diagonal step is (gamma, diag): it takes no controls, got {entry[2:]!r}")
            if _is_complex(entry[0]):
                raise ValueError(f"gamma {entry[0]!r} of a diagonal step is complex")
            if not entry[1]._h:
                raise ValueError("a diagonal step names a closed Diagonal")
            tables.append(entry[1])
            entries.append((entry[0], ""))
        else:
            tables.append(None)
            entries.append(entry)
    return entries, tables


def _split_diagonal_observable(terms):
    """energy_and_gradient's `terms` as (Pauli terms, table or None, weight): a Diagonal alone is the whole observable with weight 1,
    and a list may hold one (w, Diagonal) among its (coefficient, string) pairs.  ValueError for two diagonal parts, a complex
    weight, a closed table.  Pure Python."""
    if isinstance(terms, Diagonal):
        terms = [(1.0, terms)]
    paulis, table, weight = [], None, 0.0
    for term in terms:
        if len(term) == 2 and isinstance(term[1], Diagonal):
            if table is not None:
                raise ValueError("the observable has two diagonal parts: add the tables up into one Diagonal")
            if _is_complex(term[0]):
                raise ValueError(f"weight {term[0]!r} of the diagonal part is complex: a Hamiltonian's coefficients are real")
            if not term[1]._h:
                raise ValueError("the observable names a closed Diagonal")
            table, weight = term[1], float(term[0])
        else:
            paulis.append(term)
    return paulis, table, weight
