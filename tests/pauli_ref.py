"""The tests' own checker for Pauli-string expectation values: a numpy restatement of the two formulas the device sweeps
implement (tests/test_pauli_cpu.py pins it against dense operators), plus the dense operator itself for small registers.

A string is two masks in the project's qubit numbering (qubit q = bit q of the amplitude index): bit q of x set where it has
X or Y, bit q of z set where it has Z or Y."""
import numpy as np

_PAULI = {"I": np.eye(2), "X": np.array([[0, 1], [1, 0]]), "Y": np.array([[0, -1j], [1j, 0]]), "Z": np.diag([1.0, -1.0])}


def _parity(v):
    v = v.copy()
    for s in (32, 16, 8, 4, 2, 1):
        v ^= v >> np.uint64(s)
    return (v & np.uint64(1)).astype(np.int64)


def pauli_expectation(psi, x, z):
    """<psi|P|psi> from the amplitudes: x == 0 sums s(j)|psi_j|^2; otherwise the pairs (j, j ^ x) with the highest bit of x clear in j."""
    psi = np.asarray(psi, dtype=np.complex128)
    j = np.arange(psi.size, dtype=np.uint64)
    sign = 1.0 - 2.0 * _parity(j & np.uint64(z))
    if x == 0:
        return float(np.sum(sign * (psi.real ** 2 + psi.imag ** 2)))
    keep = (j >> np.uint64(x.bit_length() - 1)) & np.uint64(1) == 0
    jj = j[keep]
    c = np.conj(psi[jj ^ np.uint64(x)]) * psi[jj]
    ny = bin(x & z).count("1")
    if ny % 2 == 0:
        return float((1 if ny % 4 == 0 else -1) * np.sum(sign[keep] * 2.0 * c.real))
    return float((-1 if ny % 4 == 1 else 1) * np.sum(sign[keep] * 2.0 * c.imag))


def masks_to_letters(x, z, n):
    return ["IXZY"[(x >> q & 1) | 2 * (z >> q & 1)] for q in range(n)]


def dense_pauli(x, z, n):
    """The 2^n x 2^n operator, qubit 0 = least significant index bit (the last kron factor)."""
    op = np.ones((1, 1), dtype=np.complex128)
    for letter in reversed(masks_to_letters(x, z, n)):
        op = np.kron(op, _PAULI[letter])
    return op


def masks_to_text(x, z, n):
    return " ".join(f"{letter}{q}" for q, letter in enumerate(masks_to_letters(x, z, n)) if letter != "I")


def random_masks(rng, n, weight):
    """A random string acting on exactly `weight` qubits."""
    x = z = 0
    for q in rng.choice(n, size=weight, replace=False):
        letter = "XYZ"[rng.integers(3)]
        x |= (letter in "XY") << int(q)
        z |= (letter in "ZY") << int(q)
    return x, z
