"""Tables for Simulator.apply_permutation: classical reversible functions on a register of k <= 10 qubits as bijections of
range(2**k).  Pure numpy, no native code: usable and testable without a device or the library.

A table `perm` sends basis state j of the register to basis state perm[j]; bit i of j and of perm[j] is qubit targets[i] of the call
that applies it.  Every builder returns a numpy array of uint32 and raises ValueError for arguments that give no bijection."""
from __future__ import annotations

import math
import operator

import numpy as np

MAX_QUBITS = 10  # plans.apply_permutation_max_qubits()


def _int(value, what: str) -> int:
    try:
        return operator.index(value)
    except TypeError:
        raise ValueError(f"{what}: an integer is wanted, got {value!r}") from None


def _width(k, what: str) -> int:
    k = _int(k, what)
    if not 0 <= k <= MAX_QUBITS:
        raise ValueError(f"{what}: 0 to {MAX_QUBITS} qubits, got {k}")
    return k


def as_table(perm, k: int) -> np.ndarray:
    """`perm` as a uint32 array after the checks of Simulator.apply_permutation: 2**k entries, integers, each of range(2**k) once."""
    k = _width(k, "apply_permutation")
    table = np.asarray(perm)
    if table.dtype.kind not in "iu":                             # anything but an integer array: entry by entry, to name the culprit
        try:
            entries = [_int(v, "apply_permutation") for v in perm]
        except TypeError:
            raise ValueError("apply_permutation: the table is a sequence of integers") from None
        table = np.array(entries, dtype=object if any(abs(v) >= 1 << 62 for v in entries) else np.int64)
    if table.ndim != 1 or table.size != 1 << k:
        raise ValueError(f"apply_permutation: {k} targets take a table of {1 << k} entries, got shape {table.shape}")
    if table.min() < 0 or table.max() >= 1 << k or np.bincount(table.astype(np.int64), minlength=1 << k).min() != 1:
        raise ValueError(f"apply_permutation: the table is not a bijection of range({1 << k})")
    return table.astype(np.uint32)


def inverse_table(perm) -> np.ndarray:
    """inv with inv[perm[j]] = j."""
    entries = [_int(v, "inverse_table") for v in perm]
    if sorted(entries) != list(range(len(entries))):
        raise ValueError(f"inverse_table: the table is not a bijection of range({len(entries)})")
    inv = np.zeros(len(entries), dtype=np.uint32)
    inv[np.array(entries, dtype=np.int64)] = np.arange(len(entries), dtype=np.uint32)
    return inv


def xor_function_table(values, num_in: int, num_out: int) -> np.ndarray:
    """|x>|y> -> |x>|y ^ values[x]>: x is the low num_in index bits, y the num_out bits above them.  values: 2**num_in integers
    below 2**num_out; num_in + num_out <= 10.  An involution for any function, invertible or not."""
    num_in, num_out = _int(num_in, "xor_function_table"), _int(num_out, "xor_function_table")
    if num_in < 0 or num_out < 0 or num_in + num_out > MAX_QUBITS:
        raise ValueError(f"xor_function_table: num_in + num_out <= {MAX_QUBITS}, both >= 0; got {num_in} and {num_out}")
    vals = [_int(v, "xor_function_table") for v in values]
    if len(vals) != 1 << num_in:
        raise ValueError(f"xor_function_table: {num_in} input qubits take {1 << num_in} values, got {len(vals)}")
    if any(not 0 <= v < 1 << num_out for v in vals):
        raise ValueError(f"xor_function_table: every value lies in range({1 << num_out})")
    j = np.arange(1 << (num_in + num_out), dtype=np.uint32)
    f = np.array(vals, dtype=np.uint32)
    return j ^ (f[j & np.uint32((1 << num_in) - 1)] << np.uint32(num_in))


def _modulus(modulus, k, what: str):
    k, modulus = _width(k, what), _int(modulus, what)
    if not 1 <= modulus <= 1 << k:
        raise ValueError(f"{what}: 1 <= modulus <= 2**k = {1 << k}, got {modulus}")
    return modulus, k


def modular_add_table(a: int, modulus: int, k: int) -> np.ndarray:
    """x -> (x + a) mod N for x < N = modulus, the identity for N <= x < 2**k.  Any integer a."""
    a = _int(a, "modular_add_table")
    modulus, k = _modulus(modulus, k, "modular_add_table")
    out = np.arange(1 << k, dtype=np.uint32)
    out[:modulus] = [(x + a) % modulus for x in range(modulus)]
    return out


def modular_multiply_table(a: int, modulus: int, k: int) -> np.ndarray:
    """x -> a x mod N for x < N = modulus, the identity for N <= x < 2**k.  gcd(a, N) = 1, or the map is no bijection."""
    a = _int(a, "modular_multiply_table")
    modulus, k = _modulus(modulus, k, "modular_multiply_table")
    if math.gcd(a, modulus) != 1:
        raise ValueError(f"modular_multiply_table: gcd({a}, {modulus}) = {math.gcd(a, modulus)}, multiplication by {a} mod {modulus} is not invertible")
    out = np.arange(1 << k, dtype=np.uint32)
    out[:modulus] = [(a * x) % modulus for x in range(modulus)]
    return out
