"""The tests' own checker for measurement on the device (qsim_postselect, qsim_measure, Simulator.reset_qubits, Simulator.apply_channel;
csrc/measure.hip, csrc/measure.cpp), in numpy and independent of the order in which the device adds.  tests/test_measure_cpu.py pins it
against brute force; tests/test_gpu_measure.py applies it to the amplitudes READ BACK from the state before a call.

postselect(amps, qubits, outcome, dtype)   W = math.fsum of |a_i|^2 over the kept indices (bit j of the outcome is qubits[j]) and the
    collapsed vector: +0.0 outside the kept subspace, a_i / sqrt(W) inside.  dtype=np.complex64 is the fp32 replay: the amplitudes as
    complex64, every product formed in float32 with the factor rounded to float32.
weight_tolerance(kept, W)   (kept + 8) 2^-52 W: the a-priori bound on a sum of `kept` non-negative fp64 terms added in ANY order against
    the exact sum ((kept - 1) 2^-53 W), doubled for the rounding of the terms themselves, plus a few units for the checker's own.
admissible_outcomes(n, amps, draw, qubits)   which outcomes a measurement by `draw` may read: the outcomes of the indices
    sample_ref.admissible admits, so the sampler's tolerance is the measurement's.
kraus_step(amps, kraus, targets, draw, dtype)   one trajectory step of a Kraus channel by the definition, without a density matrix:
    psi_i = K_i psi through matrix_ref.apply_matrix, p_i = |psi_i|^2 / |psi|^2, the index picked by the draw against the running sum
    (lowest first, never one of probability zero), and psi_i / |psi_i|.
The shapes of the GPU test are data here, so that the CPU test can hold the fp32 replay to fp32_ref.REF_CAP on each of them."""
import math

import numpy as np

import matrix_ref
import sample_ref


def masks(qubits, outcome):
    """(the measured qubits as a mask, the outcome deposited on them)"""
    return sum(1 << q for q in qubits), sum(((outcome >> j) & 1) << q for j, q in enumerate(qubits))


def kept_indices(n, qubits, outcome):
    measured, bits = masks(qubits, outcome)
    idx = np.arange(1 << n, dtype=np.int64)
    return (idx & measured) == bits


def weight(amps, qubits, outcome):
    a = np.asarray(amps, dtype=np.complex128).reshape(-1)
    n = int(a.size).bit_length() - 1
    kept = a[kept_indices(n, qubits, outcome)]
    return math.fsum(np.concatenate((kept.real * kept.real, kept.imag * kept.imag)))


def postselect(amps, qubits, outcome, dtype=np.complex128):
    """(W, the collapsed vector as `dtype`)"""
    a = np.asarray(amps, dtype=np.complex128).reshape(-1)
    n = int(a.size).bit_length() - 1
    W = weight(a, qubits, outcome)
    keep = kept_indices(n, qubits, outcome)
    out = np.zeros(a.size, dtype=dtype)
    if dtype == np.complex64:
        out[keep] = a[keep].astype(np.complex64) * np.float32(1.0 / math.sqrt(W))
    else:
        out[keep] = a[keep] * (1.0 / math.sqrt(W))
    return W, out


def weight_tolerance(kept, W):
    return (kept + 8) * 2.0 ** -52 * W


def cleared(collapsed, qubits, outcome):
    """The collapsed vector with the measured qubits returned to 0: amplitude i moves to i with the outcome's bits cleared."""
    a = np.asarray(collapsed).reshape(-1)
    _, bits = masks(qubits, outcome)
    return a[np.arange(a.size, dtype=np.int64) ^ bits]


def admissible_outcomes(n, amps, draw, qubits):
    p, _, _, before, E, r, gamma = sample_ref.classify(n, amps, [draw])
    ok = (p > 0) & (before - gamma < r[0]) & (r[0] <= E + gamma)
    return set(int(v) for v in sample_ref.outcome_bits(np.flatnonzero(ok), qubits))


def kraus_step(amps, kraus, targets, draw, dtype=np.complex128):
    """(i, p_i, psi_i / |psi_i| as `dtype`, [p_0, p_1, ...]) for the draw in [0, 1]."""
    a = np.asarray(amps, dtype=np.complex128).reshape(-1)
    total = float(np.vdot(a, a).real)
    images = [matrix_ref.apply_matrix(a, K, targets) for K in kraus]
    p = [float(np.vdot(v, v).real) / total for v in images]
    running, pick = 0.0, None
    for i, pi in enumerate(p):
        running += pi
        if pi > 0.0 and running >= draw * sum(p):
            pick = i
            break
    if pick is None:
        pick = max(i for i, pi in enumerate(p) if pi > 0.0)
    scaled = np.asarray(kraus[pick], dtype=np.complex128) / math.sqrt(p[pick] * total)
    return pick, p[pick], matrix_ref.apply_matrix(a.astype(dtype), scaled, targets, dtype=dtype), p


def midpoints(p):
    """A draw in the middle of every index's interval of the running sum (None for an index of probability zero)."""
    total, running, out = sum(p), 0.0, []
    for pi in p:
        out.append((running + pi / 2.0) / total if pi > 0.0 else None)
        running += pi
    return out


# ---- the shapes of tests/test_gpu_measure.py ----------------------------------------------------------------------------------------
# n = 13: k = 1 on qubit 0 and on the top qubit, 2, 5, 10 and the whole register; mixed orders; outcomes 0, all ones and others.  Qubit 0
# (the slot of an fp32 unit) is measured in some cases and not in others.
N13 = 13
N13_CASES = [
    ([0], 0), ([0], 1), ([12], 0), ([12], 1),
    ([7, 3], 2), ([0, 12], 3), ([12, 0], 0),
    ([12, 0, 5, 9, 3], 0b10110), ([4, 11, 2, 8, 6], 0b11111), ([1, 10, 7, 2, 5], 0),
    ([9, 1, 12, 3, 7, 5, 11, 2, 8, 4], 0), ([0, 12, 6, 1, 11, 3, 9, 5, 7, 10], (1 << 10) - 1), ([10, 0, 2, 4, 6, 8, 1, 3, 5, 7], 0b0110100101),
    ([12, 0, 11, 1, 10, 2, 9, 3, 8, 4, 7, 5, 6], (1 << 13) - 1), (list(range(13)), 0), (list(range(13))[::-1], 0x0A5B),
]
GRID_CASES = [([0], 1), ([12, 0, 5, 9, 3], 0b10110), ([4, 11, 2, 8, 6], 0b11111), ([12], 0)]
GRID_CAPS = (1, 2, 7, 0)


MEASURE_N = 10                                                   # measure against the sampler: 64 stratified draws each
MEASURE_CASES = [[7, 0, 4], [9, 0, 3, 7, 1, 8, 5, 2, 6, 4]]
RESET_N = 11
RESET_CASES = [([0], 0.9), ([10, 0, 4], 0.35), ([3, 7, 1, 9, 5], 0.71), ([6], 0.05)]   # (qubits, draw)


def looping_n(precision):
    return 23 if precision == 32 else 22


def looping_cases(precision):
    n = looping_n(precision)
    return [(n, [0], 1), (n, [n - 1], 0)]


def small_cases(n):
    """Every non-empty subset of range(n) in two orders with every outcome."""
    import itertools
    out = []
    for k in range(1, n + 1):
        for subset in itertools.combinations(range(n), k):
            for qubits in sorted({subset, subset[::-1]}):
                for outcome in range(1 << k):
                    out.append((list(qubits), outcome))
    return out


def fp32_shapes():
    """(n, qubits, outcome) of the fp32 collapses the GPU test checks with fp32_ref.check_fp32: every post-selection but the looping
    sizes (the CPU test takes one of those), and for the measurements and resets, whose outcome the draw decides, outcome 0, all ones
    and one in between."""
    out = [(n, q, o) for n in range(1, 5) for q, o in small_cases(n)]
    out += [(N13, q, o) for q, o in N13_CASES]
    for n, lists in ((MEASURE_N, MEASURE_CASES), (RESET_N, [q for q, _ in RESET_CASES])):
        out += [(n, q, o) for q in lists for o in sorted({0, (1 << len(q)) - 1, 0x155 & ((1 << len(q)) - 1)})]
    return out
