"""Pins tests/fp32_ref.py on the CPU: the complex128 replay is the fp64 truth, and the fp32 criterion accepts a faithful fp32
evaluation of every circuit the fp32 GPU tests use while rejecting the errors it exists to catch (coefficients rounded to
half precision, one rz angle off by 1e-4)."""
import os

import numpy as np
import pytest

import fp32_ref
from fp32_ref import check_fp32, gate_list, rel_err, replay
from gpu_quantum_simulator_amd import Circuit, circuits

GOLDEN32 = ["entanglement", "grover_3_18", "rand_n10_all", "rand_n12_all", "rand_n12_clifford_t_physical"]  # test_golden_fixtures_fp32


def _fp16_coefficients(gates):
    """The same gates with every coefficient rounded to float16 (real and imaginary parts), cx untouched."""
    def r16(m):
        m = np.asarray(m)
        return m.real.astype(np.float16).astype(np.float64) + 1j * m.imag.astype(np.float16).astype(np.float64)
    return [(g[0], g[1], r16(g[2])) if g[0] == "u1" else (g[0], g[1], g[2], r16(g[3])) if g[0] == "u2" else g for g in gates]


def _truth(oracle, tmp_path, spec):
    n, depth, seed, vocab = spec
    path = circuits.random_circuit_file(str(tmp_path / "c.qasm"), n, depth, seed, vocab)
    _, want, _, _ = oracle.run_qasm(path)
    return want


@pytest.mark.parametrize("name", GOLDEN32 + ["rand_n9_clifford_t", "live_n13_seed104"])
def test_fp64_replay_equals_the_oracle(oracle, golden_dir, name):
    path = os.path.join(golden_dir, name + ".qasm")
    c = Circuit.from_file(path)
    n, want, _, _ = oracle.run_qasm(path)
    got = replay(n, [c.gate(i) for i in range(len(c))], dtype=np.complex128)
    assert got.dtype == np.complex128
    assert np.max(np.abs(got - want)) < 1e-12


def test_rz_convention_and_written_start():
    """rz(theta) arrives as diag(1, e^{i theta}); a written start is replayed from exactly the values given."""
    g = gate_list(3, 40, 5, "all")
    raw = circuits.random_gates(3, 40, 5, "all")
    rz = [(a, b) for a, b in zip(raw, g) if a[0] == "rz"]
    assert rz
    for a, b in rz:
        assert b[0] == "u1" and b[1] == a[2]
        assert np.allclose(b[2], np.diag([1.0, np.exp(1j * a[1])]), rtol=0, atol=1e-15)
    rng = np.random.default_rng(1)
    s = (rng.standard_normal(8) + 1j * rng.standard_normal(8)).astype(np.complex64)
    assert np.array_equal(replay(3, [], start=s), s)
    H = np.array([[1, 1], [1, -1]]) / np.sqrt(2)
    want = np.kron(np.eye(4), H) @ s.astype(np.complex128)  # H on qubit 0 (least significant index bit)
    assert np.max(np.abs(replay(3, [("u1", 0, H)], start=s, dtype=np.complex128) - want)) < 1e-15
    assert np.array_equal(replay(3, [("cx", 0, 2)], start=s), s[[0, 5, 2, 7, 4, 1, 6, 3]])  # control 0 flips bit 2


def test_2q_replay_matches_the_dense_operator():
    from helpers import np_apply_2q, random_unitary
    rng = np.random.default_rng(4)
    n = 6
    s = rng.standard_normal(1 << n) + 1j * rng.standard_normal(1 << n)
    for hi, lo in [(5, 0), (3, 2), (4, 1)]:
        U = random_unitary(4, rng)
        got = replay(n, [("u2", hi, lo, U)], start=s, dtype=np.complex128)
        assert np.max(np.abs(got - np_apply_2q(s.copy(), n, U, hi, lo))) < 1e-13


def test_the_circuit_list_is_what_the_gpu_tests_use():
    specs = fp32_ref.all_circuits()
    assert len(specs) >= 50
    for n, depth, seed, vocab in specs:
        assert 2 <= n <= 22 and depth >= 3 and vocab in ("all", "clifford_t")
    cases = fp32_ref.geometry_sweep_cases()
    assert len(cases) == 30 and any("tile_threads" in o for *_, o in cases) and any("grid_cap" in o for *_, o in cases)


def _check_one(want, gates, n):
    ref32 = replay(n, gates)
    e_ref = rel_err(ref32, want)
    assert e_ref <= fp32_ref.REF_CAP, e_ref                        # the reference cap
    e_self, _ = check_fp32(ref32, want, ref32)                      # the fp32 replay itself passes
    assert e_self == e_ref
    half = replay(n, _fp16_coefficients(gates))
    with pytest.raises(AssertionError, match="rel_err\\(got\\)"):   # ... and half-precision coefficients do not
        check_fp32(half, want, ref32)
    return e_ref, rel_err(half, want)


@pytest.mark.parametrize("spec", fp32_ref.all_circuits(), ids=lambda s: "n%d_d%d_s%d_%s" % s)
def test_checker_accepts_fp32_and_rejects_fp16_coefficients(oracle, tmp_path, spec):
    want = _truth(oracle, tmp_path, spec)
    e_ref, e_half = _check_one(want, gate_list(*spec), spec[0])
    print(f"{spec}: ref32 {e_ref:.3e}, fp16 coefficients {e_half:.3e} ({e_half / max(e_ref, fp32_ref.FLOOR):.0f}x)")


@pytest.mark.parametrize("name", GOLDEN32)
def test_checker_on_the_golden_fixtures(golden_dir, name):
    want = np.load(os.path.join(golden_dir, name + ".npy"), allow_pickle=False).view(np.complex128).reshape(-1)
    c = Circuit.from_file(os.path.join(golden_dir, name + ".qasm"))
    _check_one(want, [c.gate(i) for i in range(len(c))], c.num_qubits)


@pytest.mark.parametrize("spec", [c for c, _ in fp32_ref.RANDOM_CIRCUITS if c[3] == "all" and c[0] <= 19] + [fp32_ref.TILE_ORDER_CIRCUIT],
                         ids=lambda s: "n%d_s%d" % (s[0], s[2]))
def test_checker_rejects_one_rz_angle_off_by_1e_4(oracle, tmp_path, spec):
    """Shifting rz(theta) on qubit q by 1e-4 moves the state by 1e-4 * sqrt(P(q = 1)) at that point (relative), so the test
    picks an rz where the fp64 replay shows P(q = 1) >= 0.25: at least 5e-5 against bounds of at most ~1e-5."""
    n = spec[0]
    want = _truth(oracle, tmp_path, spec)
    gates = gate_list(*spec)
    raw = circuits.random_gates(*spec)
    s, done, pick = None, 0, None
    for i in range(len(gates) // 2, len(gates)):
        if raw[i][0] != "rz":
            continue
        s = replay(n, gates[done:i], start=s, dtype=np.complex128)
        done = i
        q = raw[i][2]
        p1 = float(np.sum(np.abs(s.reshape(-1, 2, 1 << q)[:, 1, :]) ** 2))
        if p1 >= 0.25:
            pick = i
            break
    assert pick is not None
    assert np.allclose(gates[pick][2], np.diag([1.0, np.exp(1j * raw[pick][1])]), rtol=0, atol=1e-15)
    shifted = list(gates)
    shifted[pick] = ("u1", gates[pick][1], np.diag([1.0, np.exp(1j * (raw[pick][1] + 1e-4))]))
    ref32 = replay(n, gates)
    off = replay(n, shifted)
    assert rel_err(off, want) >= 4e-5
    with pytest.raises(AssertionError, match="rel_err\\(got\\)"):
        check_fp32(off, want, ref32)
