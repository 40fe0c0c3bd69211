"""The checker of tests/test_gpu_sample.py (pinned by tests/test_sample_cpu.py): which basis index a draw u in [0, 1] may return for a
state, in numpy and independent of the order in which the device adds.

From the amplitudes read back it forms p_i = re^2 + im^2 in float64, the cumulative E in np.longdouble (sequential; its own error,
N 2^-64, is 2^-11 of the tolerance below) and r = u E_last.  With gamma = 2^(n - 52) E_last:
  * index i is ADMISSIBLE for the draw iff p_i > 0 and E_(i-1) - gamma < r <= E_i + gamma;
  * a draw farther than gamma from both edges of its interval (E_(i-1), E_i], i = searchsorted(E, r), is DETERMINED: it must return
    exactly i.
gamma is the bound (N - 1) 2^-53 E_last on the error of a sum of N non-negative fp64 terms added in ANY order, doubled for the rounding of
the p_i themselves: derived, not tuned.  Every test also asserts that at least 99 % of its draws are determined, so the tolerance
cannot hide a failure."""
from fractions import Fraction

import numpy as np

MIN_DETERMINED = 0.99


def probabilities(amps):
    a = np.asarray(amps, dtype=np.complex128)
    return a.real * a.real + a.imag * a.imag


def cumulative(p):
    return np.cumsum(np.asarray(p, dtype=np.float64).astype(np.longdouble))


def classify(n, amps, draws):
    """(p, want, determined, lower, upper, r, gamma): per draw the index searchsorted gives, whether the draw is determined, and the
    edges of that index's interval; all in longdouble."""
    p = probabilities(amps)
    assert p.size == 1 << n
    E = cumulative(p)
    total = E[-1]
    assert total > 0
    gamma = np.longdouble(2.0) ** (n - 52) * total
    r = np.asarray(draws, dtype=np.float64).astype(np.longdouble) * total
    want = np.minimum(np.searchsorted(E, r, side="left"), p.size - 1)
    before = np.concatenate(([np.longdouble(0)], E[:-1]))
    lower, upper = before[want], E[want]
    determined = (r - lower > gamma) & (upper - r > gamma)
    return p, want.astype(np.uint64), determined, before, E, r, gamma


def admissible(n, amps, draws, got):
    """Per draw: whether the returned index may be returned."""
    p, _, _, before, E, r, gamma = classify(n, amps, draws)
    i = np.asarray(got, dtype=np.uint64).astype(np.int64)
    inside = (i >= 0) & (i < p.size)
    i = np.where(inside, i, 0)
    return inside & (p[i] > 0) & (before[i] - gamma < r) & (r <= E[i] + gamma)


def check(n, amps, draws, got, label=""):
    """Asserts the three properties of a result; returns the share of determined draws."""
    _, want, determined, *_ = classify(n, amps, draws)
    got = np.asarray(got, dtype=np.uint64)
    assert got.shape == want.shape
    ok = admissible(n, amps, draws, got)
    share = float(np.mean(determined)) if determined.size else 1.0
    exact = got[determined] == want[determined]
    print(f"{label}: n={n} draws={got.size} determined={share:.4f} inadmissible={int(np.sum(~ok))} wrong among determined={int(np.sum(~exact))}")
    assert np.all(ok), (label, np.flatnonzero(~ok)[:8], got[~ok][:8], want[~ok][:8])
    assert np.all(exact), (label, np.flatnonzero(determined)[~exact][:8])
    assert share >= MIN_DETERMINED, (label, share)
    return share


def outcome_bits(indices, qubits):
    """bit j of an outcome = bit qubits[j] of the index"""
    idx = np.asarray(indices, dtype=np.uint64)
    out = np.zeros(idx.shape, dtype=np.uint64)
    for j, q in enumerate(qubits):
        out |= ((idx >> np.uint64(q)) & np.uint64(1)) << np.uint64(j)
    return out


def counts(values):
    v, c = np.unique(np.asarray(values, dtype=np.uint64), return_counts=True)
    return {int(a): int(b) for a, b in zip(v, c)}


def brute_force(amps, draws):
    """The definition, one amplitude after the other in exact rational arithmetic: the first index with p > 0 whose cumulative
    probability reaches r = u E_last."""
    p = [Fraction(float(x)) for x in probabilities(amps)]
    total = sum(p)
    out = []
    for u in draws:
        r = Fraction(float(u)) * total
        c, hit = Fraction(0), None
        for i, pi in enumerate(p):
            c += pi
            if pi > 0 and c >= r:
                hit = i
                break
        out.append(hit)
    return np.array(out, dtype=np.uint64)
