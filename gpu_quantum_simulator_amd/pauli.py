"""Pauli strings as the two masks qsim_expect_paulis takes.  Pure Python: usable without the library.

A string is written sparsely in the project's qubit numbering (qubit q = bit q of the amplitude index): "X0 Z3 Y17" —
whitespace-separated, letters XYZ in either case, "I5" allowed and ignored, "" = the identity."""
from __future__ import annotations

from typing import Tuple


def pauli_masks(text: str, num_q: int) -> Tuple[int, int]:
    """(x, z): bit q of x set where the string has X or Y on qubit q, bit q of z where it has Z or Y (both: Y).
    ValueError for a malformed factor, a qubit outside [0, num_q) or a qubit named twice."""
    x = z = seen = 0
    for tok in text.split():
        letter, digits = tok[0].upper(), tok[1:]
        if letter not in "IXYZ" or not digits.isascii() or not digits.isdigit():
            raise ValueError(f"bad Pauli factor {tok!r} in {text!r}: expected one of I, X, Y, Z and a qubit number, like X0 or z17")
        q = int(digits)
        if q >= num_q:
            raise ValueError(f"qubit {q} in {text!r} is outside the {num_q}-qubit register")
        if seen >> q & 1:
            raise ValueError(f"qubit {q} is named twice in {text!r}")
        seen |= 1 << q
        if letter in "XY":
            x |= 1 << q
        if letter in "ZY":
            z |= 1 << q
    return x, z
