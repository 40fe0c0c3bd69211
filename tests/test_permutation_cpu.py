"""Permutations of basis states under controls, checked on the CPU: the checker of tests/test_gpu_permutation.py
(permutation_ref.apply_permutation) against matrix_ref.apply_matrix with the permutation matrix, the host-only plan call
(plans.apply_permutation_plan) against a restatement of the tile rule, the operand the kernel is handed
(plans.apply_permutation_operand) pushed through a numpy walk of the tiles, and the table builders of
gpu_quantum_simulator_amd.permutations.  Every comparison of amplitudes is exact."""
import itertools
from ctypes import POINTER, byref, c_int, c_long, c_uint32, c_uint64

import numpy as np
import pytest

import matrix_ref
import permutation_ref
from gpu_quantum_simulator_amd import _lib, permutations, plans
from gpu_quantum_simulator_amd._marshal import ints as _ints

NEW_NAMES = ("qsim_apply_permutation", "qsim_apply_permutation_max_qubits", "qsim_apply_permutation_plan", "qsim_apply_permutation_operand",  # census
             "qsim_permutation_sweeps_launched")  # both lines: census of the signature table
GRID_CAP = 512


def _table(perm):
    return np.ascontiguousarray(perm, dtype=np.uint32).ctypes.data_as(POINTER(c_uint32))


def _model(targets, controls, n, f32):
    """The tile rule, restated: the targets and the lowest bits that are neither targets nor controls, B = min(12 | 13, n - c) in all."""
    c = len(controls)
    full = 13 if f32 else 12
    B = min(full, n - c)
    free = [q for q in range(n) if q not in targets and q not in controls]
    tile = sorted(list(targets) + free[:B - len(targets)])
    tiles = 1 << (n - c - B)
    return dict(path=1 if B == full else 0, tile_bits=B, tile_mask=sum(1 << q for q in tile), tiles=tiles, units=max(1, (1 << (n - c)) >> (1 if f32 else 0)),
                trips_per_workgroup=-(-tiles // GRID_CAP))


def _int_state(n, seed, dtype=np.complex128):
    """small integers: every product with 0 or 1 and every sum of one non-zero term is exact"""
    rng = np.random.default_rng(seed)
    return (rng.integers(-99, 100, 1 << n) + 1j * rng.integers(-99, 100, 1 << n)).astype(dtype)


def test_signatures_have_the_new_names():
    for name in NEW_NAMES:
        assert name in _lib.SIGNATURES
    assert plans.apply_permutation_max_qubits() == 10 == permutations.MAX_QUBITS


# ---- the checker ----------------------------------------------------------------------------------------------------------------------
def test_checker_equals_apply_matrix_with_the_permutation_matrix():
    rng = np.random.default_rng(71)
    for n in range(0, 6):
        psi = _int_state(n, 700 + n)
        for k in range(0, n + 1):
            for targets in itertools.permutations(range(n), k):
                perm = rng.permutation(1 << k)
                rest = [q for q in range(n) if q not in targets]
                for controls in ([], rest[:1], rest[-2:]):
                    got = permutation_ref.apply_permutation(psi, perm, targets, controls)
                    for checker in (matrix_ref.apply_matrix, matrix_ref.apply_matrix_gather):
                        want = checker(psi, permutation_ref.permutation_matrix(perm), targets, controls)
                        assert np.array_equal(got, want), (n, targets, controls, perm)
    # the definition, by hand: [0, 1, 3, 2] on (t, c) exchanges |c=1,t=0> and |c=1,t=1>
    psi = np.arange(4, dtype=np.complex128)
    assert np.array_equal(permutation_ref.apply_permutation(psi, [0, 1, 3, 2], [1, 0]), [0, 3, 2, 1])    # t = qubit 1, c = qubit 0
    assert np.array_equal(permutation_ref.apply_permutation(psi, [1, 2, 3, 0], [0, 1]), [3, 0, 1, 2])    # j -> j + 1: new[j + 1] = old[j]
    psi32 = _int_state(5, 77, np.complex64)
    got = permutation_ref.apply_permutation(psi32, [1, 0], [3], [0])
    assert got.dtype == np.complex64 and np.array_equal(got[0::2], psi32[0::2]) and not np.array_equal(got, psi32)


# ---- the plan call --------------------------------------------------------------------------------------------------------------------
def _target_sets(n, k):
    low, high = list(range(k)), list(range(n - k, n))
    spread = sorted({(j * (n - 1)) // max(k - 1, 1) for j in range(k)}) if k > 1 else [n // 2][:k]
    sets = [low, high] + ([spread] if len(spread) == k else [])
    return [s for s in sets] + [s[::-1] for s in sets]


@pytest.mark.parametrize("bits", [64, 32])
def test_plan_call_against_the_tile_rule(bits):
    f32 = bits == 32
    for n in range(0, 17):
        for k in range(0, min(n, 10) + 1):
            for targets in _target_sets(n, k):
                rest = [q for q in range(n) if q not in targets]
                choices = [[], rest[:1], rest[-1:], rest[len(rest) // 2:len(rest) // 2 + 1], sorted(set(rest[:1] + rest[-1:])), rest[1:4]]
                for controls in choices:
                    rc, got = plans.apply_permutation_plan(targets, controls, n, bits)
                    assert rc == _lib.QSIM_OK, (n, targets, controls)
                    assert got == _model(targets, controls, n, f32), (n, targets, controls)
                    assert got["tile_mask"] & sum(1 << q for q in controls) == 0 and all(got["tile_mask"] >> q & 1 for q in targets)


def test_plan_call_named_cases():
    # k = 10 with all targets high: two padding bits in fp64 (64-byte runs), three in fp32
    rc, got = plans.apply_permutation_plan(list(range(6, 16)), [], 16, 64)
    assert rc == _lib.QSIM_OK and got["tile_mask"] == 0b11 | sum(1 << q for q in range(6, 16)) and got["tile_bits"] == 12 and got["tiles"] == 16
    rc, got = plans.apply_permutation_plan(list(range(6, 16)), [], 16, 32)
    assert got["tile_mask"] == 0b111 | sum(1 << q for q in range(6, 16)) and got["tile_bits"] == 13
    # k = 9 high keeps three in fp64; a control on qubit 0 is stepped over
    assert plans.apply_permutation_plan(list(range(7, 16)), [], 16, 64)[1]["tile_mask"] & 0x7F == 0b111
    assert plans.apply_permutation_plan(list(range(7, 16)), [0], 16, 64)[1]["tile_mask"] & 0x7F == 0b1110
    # controls on qubit 0, in between and on top take one factor of two of tiles each and leave the tile's size alone
    assert plans.apply_permutation_plan([3, 9], [0, 5, 15], 16, 64)[1] == dict(path=1, tile_bits=12, tile_mask=0b11_1111_1101_1110, tiles=2, units=1 << 13, trips_per_workgroup=1)
    # both sides of the path switch: n - c = 11 | 12 (fp64), 12 | 13 (fp32)
    for bits, full in ((64, 12), (32, 13)):
        assert plans.apply_permutation_plan([0], [], full - 1, bits)[1]["path"] == 0 and plans.apply_permutation_plan([0], [], full, bits)[1]["path"] == 1
        assert plans.apply_permutation_plan([0], [full], full + 1, bits)[1]["path"] == 1 and plans.apply_permutation_plan([0], [full - 1], full, bits)[1]["path"] == 0
    # the looping sizes of tests/test_gpu_permutation.py: two tiles per workgroup at the default cap
    assert plans.apply_permutation_plan(list(range(2, 22, 2)), [], 22, 64)[1]["trips_per_workgroup"] == 2 and plans.apply_permutation_plan(list(range(2, 22, 2)), [], 21, 64)[1]["trips_per_workgroup"] == 1
    assert plans.apply_permutation_plan(list(range(2, 22, 2)), [], 23, 32)[1]["trips_per_workgroup"] == 2 and plans.apply_permutation_plan(list(range(2, 22, 2)), [], 22, 32)[1]["trips_per_workgroup"] == 1
    assert plans.apply_permutation_plan([0], [], 30, 64)[1]["units"] == 1 << 30 and plans.apply_permutation_plan([0], [29], 30, 32)[1]["units"] == 1 << 28
    assert plans.apply_permutation_plan([], [], 0, 32)[1] == dict(path=0, tile_bits=0, tile_mask=0, tiles=1, units=1, trips_per_workgroup=1)


def test_plan_call_and_operand_refusals():
    ok = lambda *a, **kw: plans.apply_permutation_plan(*a, **kw)[0]
    assert ok([0, 1], [2], 6, 64) == _lib.QSIM_OK
    assert ok([0, 0], [], 6, 64) == _lib.ERR_ARG                 # a repeated target
    assert ok([0], [2, 2], 6, 64) == _lib.ERR_ARG                # a repeated control
    assert ok([0, 1], [1], 6, 64) == _lib.ERR_ARG                # a control among the targets
    assert ok([0, 6], [], 6, 64) == _lib.ERR_ARG and ok([-1], [], 6, 64) == _lib.ERR_ARG
    assert ok([0], [6], 6, 64) == _lib.ERR_ARG and ok([0], [-1], 6, 64) == _lib.ERR_ARG
    assert ok(list(range(11)), [], 16, 64) == _lib.ERR_ARG       # k > 10
    assert ok(list(range(10)), [], 16, 64) == _lib.QSIM_OK
    assert ok([0, 1, 2], [], 2, 64) == _lib.ERR_ARG              # k > n
    assert ok([0], [], 6, 64, k=-1) == _lib.ERR_ARG and ok([0], [1], 6, 64, num_controls=-1) == _lib.ERR_ARG
    assert ok(None, [], 6, 64, k=1) == _lib.ERR_ARG and ok([0], None, 6, 64, num_controls=1) == _lib.ERR_ARG
    assert ok(None, None, 6, 64) == _lib.QSIM_OK
    assert ok([0], [], -1, 64) == _lib.ERR_ARG and ok([0], [], 41, 64) == _lib.ERR_ARG
    assert ok([0], [], 40, 64) == _lib.QSIM_OK and ok([], [], 0, 32) == _lib.QSIM_OK
    assert ok([0], [], 6, 16) == _lib.ERR_ARG                    # precision_bits
    lib = _lib.load()
    tile_bits, mask, tiles, units, trips = c_int(), c_uint64(), c_uint64(), c_uint64(), c_long()
    assert lib.qsim_apply_permutation_plan(_ints([0]), 1, None, 0, 6, 64, None, byref(tile_bits), byref(mask), byref(tiles), byref(units),  # raw, as below
                                           byref(trips)) == _lib.ERR_ARG  # raw: NULL for an out-parameter
    # the table: an entry >= 2^k, two equal entries
    assert plans.apply_permutation_operand([0, 1, 2, 3], [0, 1], [], 6, 64)[0] == _lib.QSIM_OK
    assert plans.apply_permutation_operand([0, 1, 2, 4], [0, 1], [], 6, 64)[0] == _lib.ERR_ARG
    assert plans.apply_permutation_operand([0, 1, 2, 2], [0, 1], [], 6, 64)[0] == _lib.ERR_ARG
    assert plans.apply_permutation_operand([1], [], [], 6, 64)[0] == _lib.ERR_ARG and plans.apply_permutation_operand([0], [], [], 6, 64)[0] == _lib.QSIM_OK
    assert plans.apply_permutation_operand([0, 1], [0], [0], 6, 64)[0] == _lib.ERR_ARG
    assert plans.apply_permutation_operand(None, [0], None, 6, 64)[0] == _lib.ERR_ARG
    # the call itself refuses a NULL state before it looks at anything else
    assert lib.qsim_apply_permutation(None, _table([0, 1]), _ints([0]), 1, None, 0) == _lib.ERR_ARG


# ---- the operand ------------------------------------------------------------------------------------------------------------------------
def _random_case(n, rng):
    k = int(rng.integers(0, min(n, 10) + 1))
    qubits = [int(q) for q in rng.permutation(n)]
    targets = qubits[:k]
    c = int(rng.integers(0, min(n - k, 3) + 1))
    controls = qubits[k:k + c]
    return [int(v) for v in rng.permutation(1 << k)], targets, controls


@pytest.mark.parametrize("bits", [64, 32])
@pytest.mark.parametrize("n", [6, 9, 13])
def test_tile_walk_with_plan_and_operand_reproduces_the_checker(n, bits):
    rng = np.random.default_rng(720 + n)
    psi = _int_state(n, 730 + n)
    cases = [_random_case(n, rng) for _ in range(24)]
    top = list(range(n - min(n, 10), n))
    cases += [([int(v) for v in rng.permutation(1 << len(top))], top, []), ([int(v) for v in rng.permutation(1 << len(top))], top[::-1], []),
              ([1, 0], [0], [n - 1]), ([1, 0], [n - 1], [0]), ([0], [], [0, n - 1]), ([0], [], [])]
    for perm, targets, controls in cases:
        rc, plan = plans.apply_permutation_plan(targets, controls, n, bits)
        assert rc == _lib.QSIM_OK
        rc, operand = plans.apply_permutation_operand(perm, targets, controls, n, bits)
        local_map = operand["local_map"]
        assert rc == _lib.QSIM_OK and local_map.size == 1 << plan["tile_bits"]
        assert np.array_equal(np.sort(local_map), np.arange(local_map.size))                       # a bijection of range(2^B)
        tile_bits = [q for q in range(n) if plan["tile_mask"] >> q & 1]
        pad = sum(1 << i for i, q in enumerate(tile_bits) if q not in targets)
        assert np.array_equal(local_map & pad, np.arange(local_map.size) & pad)                    # the padding bits are kept
        got = permutation_ref.walk_tiles(psi, plan["tile_mask"], controls, local_map)
        assert np.array_equal(got, permutation_ref.apply_permutation(psi, perm, targets, controls)), (perm[:8], targets, controls)


# ---- the builders -----------------------------------------------------------------------------------------------------------------------
def _is_bijection(t):
    return t.dtype == np.uint32 and np.array_equal(np.sort(t), np.arange(t.size))


def test_builders():
    rng = np.random.default_rng(74)
    for k in range(0, 11):
        perm = rng.permutation(1 << k)
        inv = permutations.inverse_table(perm)
        assert _is_bijection(inv) and np.array_equal(inv[perm], np.arange(1 << k)) and np.array_equal(perm[inv], np.arange(1 << k))
    for N, k in ((1, 0), (1, 3), (15, 4), (16, 4), (21, 5), (1000, 10), (1023, 10), (1024, 10)):
        x = np.arange(1 << k)
        for a in [a for a in (1, 2, 7, 13, N - 1, N + 2) if np.gcd(a, N) == 1]:
            t = permutations.modular_multiply_table(a, N, k)
            assert _is_bijection(t) and np.array_equal(t[:N], (a * x[:N]) % N) and np.array_equal(t[N:], x[N:])   # the identity above N
            back = permutations.modular_multiply_table(pow(a, -1, N), N, k)
            assert np.array_equal(back[t], x)
        for a in (0, 1, 5, N - 1, N, -3):
            t = permutations.modular_add_table(a, N, k)
            assert _is_bijection(t) and np.array_equal(t[:N], (x[:N] + a) % N) and np.array_equal(t[N:], x[N:])
            assert np.array_equal(permutations.modular_add_table(N - a, N, k)[t], x)
    for num_in, num_out in ((0, 0), (0, 3), (3, 0), (1, 1), (4, 3), (7, 3), (5, 5), (9, 1)):
        values = rng.integers(0, 1 << num_out, 1 << num_in)
        t = permutations.xor_function_table(values, num_in, num_out)
        j = np.arange(1 << (num_in + num_out))
        low = (1 << num_in) - 1
        assert _is_bijection(t) and np.array_equal(t[t], j)                                        # an involution
        assert np.array_equal(t & low, j & low) and np.array_equal(t >> num_in, (j >> num_in) ^ values[j & low])


def test_value_errors_without_the_library(monkeypatch):
    """Every documented ValueError comes from pure Python: loading the library would fail the test."""
    def no_library():
        raise AssertionError("the library was loaded")
    monkeypatch.setattr(_lib, "load", no_library)
    P = permutations
    bad_calls = [
        lambda: P.inverse_table([0, 0]), lambda: P.inverse_table([0, 2]), lambda: P.inverse_table([0.5, 1]),
        lambda: P.xor_function_table([0] * 64, 6, 5), lambda: P.xor_function_table([0, 4], 1, 2), lambda: P.xor_function_table([0, -1], 1, 2),
        lambda: P.xor_function_table([0, 1, 2], 1, 2), lambda: P.xor_function_table([0, 1.5], 1, 2),
        lambda: P.modular_add_table(1, 17, 4), lambda: P.modular_add_table(1, 0, 4), lambda: P.modular_add_table(1, 5, 11), lambda: P.modular_add_table(1.0, 5, 4),
        lambda: P.modular_multiply_table(6, 15, 4), lambda: P.modular_multiply_table(0, 15, 4), lambda: P.modular_multiply_table(7, 17, 4),
        lambda: P.modular_multiply_table(7, 15, 11),
    ]
    from gpu_quantum_simulator_amd.simulator import Simulator
    sim = Simulator.__new__(Simulator)                           # no state behind it: a call that reached the library would fail
    sim._h = None
    bad_calls += [
        lambda: sim.apply_permutation([0, 1, 2], [0, 1]), lambda: sim.apply_permutation([0, 1, 2, 3, 4], [0, 1]),      # a wrong length
        lambda: sim.apply_permutation([0, 1, 2.5, 3], [0, 1]), lambda: sim.apply_permutation([0, 1, "2", 3], [0, 1]),  # a non-integer
        lambda: sim.apply_permutation([0, 1, 2, 2], [0, 1]), lambda: sim.apply_permutation([0, 1, 2, 4], [0, 1]),      # not a bijection
        lambda: sim.apply_permutation([0, 1, 1, 0], [0, 1], inverse=True), lambda: sim.apply_permutation(list(range(2048)), list(range(11))),
        lambda: sim.apply_modular_multiply(5, 15, [0, 1, 2, 3]), lambda: sim.apply_modular_add(1, 17, [0, 1, 2, 3]),
        lambda: sim.apply_function_xor([0, 2], [0], [1]),
    ]
    for call in bad_calls:
        with pytest.raises(ValueError):
            call()
    # and an accepted table does reach the library
    with pytest.raises(AssertionError, match="the library was loaded"):
        sim.apply_permutation([1, 0], [0])
