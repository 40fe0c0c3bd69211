"""Shots drawn on the device, what can be checked without one: the checker of tests/test_gpu_sample.py (sample_ref) against a brute-force
loop in exact rational arithmetic at n <= 6, the host-only geometry call (plans.sample_geometry) against the rule in include/qsim.h, and
the new names in the binding."""
from ctypes import byref, c_int, c_uint64

import numpy as np
import pytest

import sample_ref
from gpu_quantum_simulator_amd import Simulator, _lib, plans
from pauli_rot_ref import rand_state

NEW_NAMES = ("qsim_sample_geometry", "qsim_sample_shots", "qsim_sample_stage_times")  # census of the signature table
EDGES = [0.0, 1e-300, 1.0]


def test_signatures_and_exports_have_the_new_names():
    lib = _lib.load()
    for name in NEW_NAMES:
        assert name in _lib.SIGNATURES and hasattr(lib, name)
    assert hasattr(Simulator, "sample_shots") and hasattr(Simulator, "sample_counts")


@pytest.mark.parametrize("n", [1, 7, 8, 9, 18, 19, 30])
def test_geometry_clips_the_bits_by_n(n):
    got = plans.ok(plans.sample_geometry(n))
    cb, gb, sb = got["chunk_bits"], got["group_bits"], got["scratch_bytes"]
    assert (cb, gb) == (min(8, n), min(18, n))
    assert sb == 8 * ((1 << (n - cb)) + (1 << (n - gb)))
    if n == 30:
        assert sb == (32 << 20) + (32 << 10)  # 32 MiB of chunk entries, 32 KiB of group entries: 0.2 % of the 16 GiB state


def test_geometry_refusals():
    lib = _lib.load()
    cb, gb, sb = c_int(), c_int(), c_uint64()
    for n in (-1, 41):
        assert plans.sample_geometry(n) == (_lib.ERR_ARG, dict(chunk_bits=-1, group_bits=-1, scratch_bytes=0))
        assert b"qsim_sample_geometry" in lib.qsim_last_error()  # the library's message names the call
    assert lib.qsim_sample_geometry(8, None, byref(gb), byref(sb)) == _lib.ERR_ARG  # raw: NULL for an out-parameter
    assert lib.qsim_sample_geometry(8, byref(cb), None, byref(sb)) == _lib.ERR_ARG  # raw: NULL for an out-parameter
    assert lib.qsim_sample_geometry(8, byref(cb), byref(gb), None) == _lib.ERR_ARG  # raw: NULL for an out-parameter
    geometry = lambda n: (plans.sample_geometry(n)[0],) + tuple(plans.sample_geometry(n)[1][key] for key in ("chunk_bits", "group_bits"))
    assert geometry(0) == (_lib.QSIM_OK, 0, 0) and geometry(40) == (_lib.QSIM_OK, 8, 18)


# ---- the checker --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 4, 6])
def test_reference_agrees_with_the_brute_force_loop(n):
    rng = np.random.default_rng(300 + n)
    psi = rand_state(n, 310 + n)
    psi[rng.random(psi.size) < 0.3] = 0.0          # holes: indices of probability zero
    if not np.any(psi):
        psi[-1] = 1.0
    psi *= 0.7                                     # unnormalised: the draws are scaled by the total
    draws = np.concatenate((rng.random(200), EDGES))
    brute = sample_ref.brute_force(psi, draws)
    _, want, determined, *_ = sample_ref.classify(n, psi, draws)
    assert np.mean(determined) >= sample_ref.MIN_DETERMINED - 3 / draws.size  # the three edge draws sit on an edge by construction
    assert np.array_equal(brute[determined], want[determined])
    assert np.all(sample_ref.admissible(n, psi, draws, brute))
    assert np.all(sample_ref.probabilities(psi)[brute.astype(np.int64)] > 0)


def test_reference_refuses_what_it_should():
    n = 4
    psi = np.zeros(1 << n, dtype=np.complex128)
    psi[[3, 9]] = [0.6, 0.8j]                      # E: 0.36 from index 3 on, 1.0 from index 9 on
    draws = np.array([0.1, 0.36 + 1e-9, 0.9, 1.0, 0.0])
    right = np.array([3, 9, 9, 9, 3], dtype=np.uint64)
    assert np.all(sample_ref.admissible(n, psi, draws, right))
    _, want, determined, *_ = sample_ref.classify(n, psi, draws)
    assert list(determined) == [True, True, True, False, False] and np.array_equal(want[:3], right[:3])
    for wrong in ([9, 9, 9, 9, 3], [3, 3, 9, 9, 3], [3, 9, 9, 15, 3], [3, 9, 9, 9, 0], [3, 9, 8, 9, 3]):
        assert not np.all(sample_ref.admissible(n, psi, draws, np.array(wrong, dtype=np.uint64))), wrong
    with pytest.raises(AssertionError):
        sample_ref.check(n, psi, draws, right)     # only 60 % of these draws are determined: the cap speaks


def test_outcome_bits_and_counts():
    idx = np.array([0b1011, 0b0100, 0b1111], dtype=np.uint64)
    assert list(sample_ref.outcome_bits(idx, [0])) == [1, 0, 1]
    assert list(sample_ref.outcome_bits(idx, [3, 0])) == [0b11, 0b00, 0b11]
    assert list(sample_ref.outcome_bits(idx, [2, 1, 3])) == [0b110, 0b001, 0b111]
    assert sample_ref.counts([5, 1, 5, 5, 0]) == {0: 1, 1: 1, 5: 3} and list(sample_ref.counts([5, 1, 0])) == [0, 1, 5]
