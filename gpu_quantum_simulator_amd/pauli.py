"""Pauli strings as the two masks qsim_expect_paulis and qsim_apply_pauli_rotations take, the control mask of a controlled
rotation, and the rotation list of a product formula.  Pure Python: usable without the library.

A string is written sparsely in the project's qubit numbering (qubit q = bit q of the amplitude index): "X0 Z3 Y17" —
whitespace-separated, letters XYZ in either case, "I5" allowed and ignored, "" = the identity."""
from __future__ import annotations

from typing import Iterable, List, Tuple


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


def control_mask(controls: Iterable[int], num_q: int, pauli: str = "") -> int:
    """The control mask of a controlled rotation: bit q set for every qubit number q of `controls`.  ValueError for a qubit named
    twice, a qubit outside [0, num_q) and a control that the string `pauli` also names with X, Y or Z."""
    x, z = pauli_masks(pauli, num_q)
    mask = 0
    for q in controls:
        if int(q) != q or not 0 <= q < num_q:
            raise ValueError(f"control qubit {q!r} is outside the {num_q}-qubit register")
        if mask >> int(q) & 1:
            raise ValueError(f"control qubit {q} is named twice")
        if (x | z) >> int(q) & 1:
            raise ValueError(f"control qubit {q} carries a Pauli factor in {pauli!r}")
        mask |= 1 << int(q)
    return mask


def trotter_rotations(terms: Iterable, time: float, steps: int = 1, order: int = 1) -> List[Tuple[float, str]]:
    """The rotations [(theta, string), ...] of a product formula for exp(-i H time), H = sum_k c_k P_k given as (c_k, string)
    pairs with real c_k, first rotation first; exp(-i c dt P) is the rotation by theta = 2 c dt.
    order 1: `steps` times the terms in order with dt = time / steps.  order 2: `steps` times the symmetric formula, the terms
    forward and then in reverse, each by dt / 2.  ValueError for a complex coefficient, an order other than 1 or 2, steps < 1."""
    if order not in (1, 2):
        raise ValueError(f"product formula of order {order!r}: only 1 and 2 are built")
    if int(steps) != steps or steps < 1:
        raise ValueError(f"steps must be a positive integer, not {steps!r}")
    pairs = []
    for coeff, text in terms:
        if isinstance(coeff, complex) or (hasattr(coeff, "dtype") and coeff.dtype.kind == "c"):
            raise ValueError(f"coefficient {coeff!r} of {text!r} is complex: a Hamiltonian's coefficients are real")
        pairs.append((float(coeff), text))
    dt = float(time) / int(steps)
    if order == 1:
        one_step = [(2.0 * c * dt, text) for c, text in pairs]
    else:
        half = [(c * dt, text) for c, text in pairs]
        one_step = half + half[::-1]
    return one_step * int(steps)
