"""The tests' own reference for the quantum Fourier transform (Simulator.apply_qft, qsim_apply_qft): the checker through numpy.fft,
a complex64 radix-2 replay for the fp32 criterion of fp32_ref, the pass rule of csrc/qft.h in numpy (walk_plan), the textbook
circuit as a gate list, and the shapes tests/test_gpu_qft.py runs (tests/test_qft_cpu.py pins all of it on the CPU).

Convention: bit j of the register value is qubits[j]; forwards is  new[y] = 2^(-k/2) sum_x exp(+2 pi i x y / 2^k) old[x]  for every
setting of the other qubits — numpy's ifft times sqrt(2^k) along the register axis; inverse=True is the conjugate sign.
Plain numpy: nothing here imports the library or touches a device."""
import numpy as np


def _num_qubits(state):
    n = int(state.size).bit_length() - 1
    assert state.size == 1 << n
    return n


def _axes(n, qubits):
    """The transposition that brings the register to the front: axis 0 of the result is the register value after a reshape."""
    front = [n - 1 - q for q in reversed(list(qubits))]          # the axis of qubit q in shape (2,) * n is n - 1 - q; MSB first
    rest = [a for a in range(n) if a not in front]
    return front + rest


def gather(state, qubits):
    """(2^k, 2^(n-k)): row x holds the amplitudes whose register value is x, one column per setting of the other qubits."""
    n, k = _num_qubits(state), len(qubits)
    return state.reshape((2,) * n).transpose(_axes(n, qubits)).reshape(1 << k, -1)


def scatter(rows, qubits, n):
    """The inverse of gather."""
    order = _axes(n, qubits)
    return rows.reshape((2,) * n).transpose(np.argsort(order)).reshape(-1)


def _replay32(rows, inverse):
    """Radix-2, decimation in frequency, k stages over axis 0 in complex64: each stage's twiddles are formed in fp64 and rounded to
    complex64 once, the butterflies are complex64 arithmetic, the bit reversal is an index permutation and the scaling comes last."""
    x = rows.astype(np.complex64)
    size = x.shape[0]
    k = size.bit_length() - 1
    sign = -1.0 if inverse else 1.0
    for b in range(k - 1, -1, -1):                                # pairs (t, t + 2^b), twiddle exp(+-2 pi i (t mod 2^b) / 2^(b+1))
        half = 1 << b
        tw = np.exp(sign * 2j * np.pi * np.arange(half) / (2 * half)).astype(np.complex64)
        v = x.reshape(size // (2 * half), 2, half, -1)
        lo, hi = v[:, 0].copy(), v[:, 1].copy()
        v[:, 0] = lo + hi
        v[:, 1] = (lo - hi) * tw[None, :, None]
    rev = np.array([int(format(t, f"0{k}b")[::-1], 2) if k else 0 for t in range(size)])
    return x[rev] * np.float32(2.0 ** (-0.5 * k))


def apply_qft(state, qubits, inverse=False, dtype=np.complex128):
    """A new array of `dtype`: the transform of `state` on `qubits`.  complex128: numpy.fft; complex64: the radix-2 replay."""
    state = np.asarray(state).reshape(-1)
    n, k = _num_qubits(state), len(qubits)
    assert len(set(qubits)) == k and all(0 <= q < n for q in qubits)
    if dtype == np.complex64:
        return scatter(_replay32(gather(state.astype(np.complex64), qubits), inverse), qubits, n)
    rows = gather(state.astype(np.complex128), qubits)
    size = 1 << k
    out = np.fft.fft(rows, axis=0) / np.sqrt(size) if inverse else np.fft.ifft(rows, axis=0) * np.sqrt(size)
    return scatter(out, qubits, n)


def dft_matrix(k, inverse=False):
    x = np.arange(1 << k)
    return np.exp((-2j if inverse else 2j) * np.pi * np.outer(x, x) / (1 << k)) / np.sqrt(1 << k)


def walk_plan(state, qubits, digits, inverse=False):
    """The pass rule of csrc/qft.h: pass p works on the sub-register qubits[s_p:], whose value is (t, r) with t the top d_p bits;
    it replaces t by its unitary DFT u, multiplies by w^(+-r u), w = exp(2 pi i / 2^k_p), and stores the sub-register as r 2^d_p + u."""
    state = np.asarray(state, dtype=np.complex128).reshape(-1)
    n, k = _num_qubits(state), len(qubits)
    assert sum(digits) == k
    first = 0
    for d in digits:
        sub = list(qubits[first:])
        kp = len(sub)
        rows = gather(state, sub).reshape(1 << d, 1 << (kp - d), -1)          # (t, r, environment)
        rows = np.tensordot(dft_matrix(d, inverse), rows, axes=(1, 0))        # (u, r, environment)
        u, r = np.arange(1 << d)[:, None], np.arange(1 << (kp - d))[None, :]
        rows = rows * np.exp((-2j if inverse else 2j) * np.pi * ((u * r) % (1 << kp)) / (1 << kp))[:, :, None]
        state = scatter(rows.transpose(1, 0, 2).reshape(1 << kp, -1), sub, n)  # value r 2^d + u
        first += d
    return state


def textbook_gates(qubits):
    """The textbook circuit as the tuples of Circuit.gate / fp32_ref.replay: h on the top qubit of the register first, the controlled
    phases pi / 2^(j - m) of every lower qubit m onto it, and so down the register; then the swaps that undo the bit reversal, three cx
    each.  k (k - 1) / 2 two-qubit gates, k h and 3 floor(k / 2) cx."""
    h = np.array([[1, 1], [1, -1]], dtype=np.complex128) / np.sqrt(2.0)
    gates = []
    k = len(qubits)
    for j in range(k - 1, -1, -1):
        gates.append(("u1", qubits[j], h))
        for m in range(j - 1, -1, -1):
            cp = np.diag([1, 1, 1, np.exp(1j * np.pi / (1 << (j - m)))]).astype(np.complex128)
            gates.append(("u2", max(qubits[j], qubits[m]), min(qubits[j], qubits[m]), cp))
    for j in range(k // 2):
        a, b = qubits[j], qubits[k - 1 - j]
        gates += [("cx", a, b), ("cx", b, a), ("cx", a, b)]
    return gates


# ---- the shapes of tests/test_gpu_qft.py, as data: (n, qubits, max_digit_bits) ----------------------------------------------------------
def tile_bits(precision):
    return 12 if precision == 64 else 13


def _scrambled(n, k, seed):
    return [int(q) for q in np.random.default_rng(seed).permutation(n)[:k]]


def boundary_cases(precision):
    """n = B - 1, B, B + 1 with k = 1, 5, 10 in low, top and scrambled places."""
    out = []
    for n in (tile_bits(precision) - 1, tile_bits(precision), tile_bits(precision) + 1):
        for k in (1, 5, 10):
            out += [(n, list(range(k)), 0), (n, list(range(n - k, n)), 0), (n, _scrambled(n, k, 100 * n + k), 0)]
    return out


def single_pass_cases():
    """n = 13: k = 1, 2, 5, 9, 10 in low, top, spread and scrambled places."""
    n, out = 13, []
    for k in (1, 2, 5, 9, 10):
        spread = sorted({(j * (n - 1)) // max(k - 1, 1) for j in range(k)}) if k > 1 else [6]
        if len(spread) != k:
            spread = [q for q in range(n) if q not in (4, 8, 6, 2)[:n - k]]
        out += [(n, list(range(k)), 0), (n, list(range(n - k, n)), 0), (n, spread, 0), (n, _scrambled(n, k, 1300 + k), 0)]
    return out


SCATTERED_12_OF_16 = [14, 3, 9, 0, 12, 6, 15, 2, 10, 5, 8, 13]   # the environment bits 1, 4, 7, 11 lie below, between and above


def multi_pass_cases():
    """(n, qubits, cap, passes): k = 11, 12, 13 at the default cap; three, four and thirteen passes at n = 13; n = 16 with twelve
    scattered targets at caps 0 and 5."""
    n = 13
    return [(n, list(range(11)), 0, 2), (n, _scrambled(n, 11, 1311), 0, 2), (n, list(range(1, 13)), 0, 2), (n, _scrambled(n, 12, 1312), 0, 2),
            (n, list(range(13)), 0, 2), (n, _scrambled(n, 13, 1313), 0, 2),
            (n, _scrambled(n, 12, 1322), 4, 3), (n, _scrambled(n, 13, 1323), 4, 4), (n, list(range(13))[::-1], 4, 4), (n, _scrambled(n, 13, 1324), 1, 13),
            (16, SCATTERED_12_OF_16, 0, 2), (16, SCATTERED_12_OF_16, 5, 3)]


def grid_cases():
    """(n, qubits, cap): one single-pass and one three-pass case for n = 15 and 16."""
    return [(n, qs, cap) for n in (15, 16) for qs, cap in ((_scrambled(n, 10, 1500 + n), 0), (_scrambled(n, 12, 1600 + n), 4))]


def looping_cases(precision):
    """n = 22 (fp64) / 23 (fp32): at least two tiles per workgroup at the default grid; one k = 10 case and the whole register."""
    n = 22 if precision == 64 else 23
    return [(n, [n - 1, 3, 17, 8, 12, 5, 20, 10, 15, 0], 0), (n, list(range(n)), 0)]


def fp32_shapes():
    """(n, k) of every shape the fp32 GPU tests hold to the replay."""
    shapes = {(n, len(qs)) for n, qs, _ in boundary_cases(32) + single_pass_cases() + grid_cases() + looping_cases(32)}
    shapes |= {(n, len(qs)) for n, qs, _, _ in multi_pass_cases()}
    shapes |= {(n, k) for n in range(5) for k in range(n + 1)} | {(14, 8), (12, 8), (15, 10), (15, 12)}
    return sorted(shapes)
