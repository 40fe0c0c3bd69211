"""fp32 state (qsim_create_f32): the precision of the reference's CUDA variants (cuFloatComplex, naive.cu:38).

NOT the parity configuration (that is fp64 within 1e-10, tests/test_gpu_parity.py).  The same kernels are instantiated for
float amplitudes; these tests hold them to the fp64 truth with the criterion of tests/fp32_ref.py: the relative 2-norm error
may be at most C = 8 times that of a gate-by-gate complex64 replay of the same gates (floor 2^-24).  That tells fp32
arithmetic from anything coarser: coefficients rounded to half precision sit thousands of times above it.

TOL32 = 2e-5 abs is kept as a second, much weaker check.  It catches indexing errors (1e-2..1) but NOT precision loss: at
n = 20..22 the RMS amplitude is 5e-4..1e-3, so 2e-5 abs admits 2-4 % error per amplitude, and an engine with half-precision
coefficients would pass it at those sizes.  Run with -s to see each case's rel_err(got), rel_err(ref32) and their ratio.
"""
import os

import numpy as np
import pytest

import fp32_ref
from fp32_ref import check_fp32, gate_list, replay, report
from gpu_quantum_simulator_amd import Circuit, Simulator, circuits, run_qasm
from helpers import random_unitary

pytestmark = pytest.mark.gpu
TOL32 = 2e-5


def _rand_state(n, seed):
    rng = np.random.default_rng(seed)
    s = rng.standard_normal(1 << n) + 1j * rng.standard_normal(1 << n)
    return (s / np.linalg.norm(s)).astype(np.complex128)


def test_precision_flag_and_io_round_trip():
    n = 12
    s = _rand_state(n, 3)
    with Simulator(n, precision=32) as sim:
        assert sim.precision == 32
        from gpu_quantum_simulator_amd import _lib
        assert _lib.load().qsim_precision_bits(sim._h) == 32
        zero = sim.read()
        assert zero[0] == 1.0 and not zero[1:].any()
        sim.write(s)
        got = sim.read()
        assert np.array_equal(got, s.astype(np.complex64).astype(np.complex128))  # one rounding, nothing else
        part = sim.read(100, 37)
        assert np.array_equal(part, got[100:137])
        assert abs(sim.norm2() - 1.0) < 1e-6
    with Simulator(n) as sim:
        from gpu_quantum_simulator_amd import _lib
        assert _lib.load().qsim_precision_bits(sim._h) == 64
    with pytest.raises(ValueError):
        Simulator(4, precision=16)


@pytest.mark.parametrize("precision", [32, 64])
def test_tile_bits_14_and_retired_options_rejected(precision):
    from gpu_quantum_simulator_amd import _lib
    with Simulator(10, precision=precision) as sim:
        sim.set_option(_lib.OPT_TILE_BITS, 13)
        with pytest.raises(_lib.QsimError, match="not in 8..13"):
            sim.set_option(_lib.OPT_TILE_BITS, 14)
        assert _lib.load().qsim_get_option(sim._h, _lib.OPT_TILE_BITS) == 13
        for opt in (10, 11):  # retired measurement aids: rejected like any unknown option
            with pytest.raises(_lib.QsimError, match="unknown option"):
                sim.set_option(opt, 1)


@pytest.mark.parametrize("fuse", [0, 1, 2, 3])
@pytest.mark.parametrize("name", ["entanglement", "grover_3_18", "rand_n10_all", "rand_n12_all",
                                  "rand_n12_clifford_t_physical"])
def test_golden_fixtures_fp32(golden_dir, name, fuse):
    want = np.load(os.path.join(golden_dir, name + ".npy"), allow_pickle=False).view(np.complex128).reshape(-1)
    path = os.path.join(golden_dir, name + ".qasm")
    got = run_qasm(path, fuse=fuse, precision=32)
    c = Circuit.from_file(path)
    report(f"golden {name} fuse={fuse}", check_fp32(got, want, replay(c.num_qubits, [c.gate(i) for i in range(len(c))])))
    assert np.max(np.abs(got - want)) < TOL32


def test_every_target_bit_and_pair_fp32(oracle):
    """Per-gate kernels (fuse=0): dense/diagonal 1q on every bit, cx on every ordered pair, against the oracle.  Compared from
    the start the state holds after the write (rounded to fp32); cx only moves data and is bit-exact."""
    n = 13
    rng = np.random.default_rng(5)
    with Simulator(n, fuse=0, precision=32) as sim:
        for q in range(n):
            for kind, U in (("dense", random_unitary(2, rng)), ("diag", np.diag(np.exp(1j * rng.uniform(0, 6.28, 2))))):
                s = _rand_state(n, 300 + q)
                s32 = s.astype(np.complex64)
                sim.write(s)
                sim.apply_1q(U, q)
                got = sim.read()
                want = s.copy()
                oracle.apply_1q(want, n, U.T, q)
                assert np.max(np.abs(got - want)) < TOL32, q
                want32 = s32.astype(np.complex128)
                oracle.apply_1q(want32, n, U.T, q)
                report(f"1q {kind} q={q}", check_fp32(got, want32, replay(n, [("u1", q, U)], start=s32)))
        for c in range(n):
            for t in range(n):
                if c == t:
                    continue
                s = _rand_state(n, 400 + c * n + t)
                sim.write(s)
                sim.apply_cx(c, t)
                got = sim.read()
                want = s.copy()
                oracle.apply_cx(want, n, c, t)
                assert np.max(np.abs(got - want)) < TOL32, (c, t)
                want32 = s.astype(np.complex64).astype(np.complex128)
                oracle.apply_cx(want32, n, c, t)
                assert np.array_equal(got, want32), (c, t)


@pytest.mark.parametrize("n,depth,seed,vocab,opts", [(*spec, opts) for spec, opts in fp32_ref.RANDOM_CIRCUITS])
def test_random_circuits_fp32(oracle, tmp_path, n, depth, seed, vocab, opts):
    spec = (n, depth, seed, vocab)
    path = circuits.random_circuit_file(str(tmp_path / "c.qasm"), n, depth, seed, vocab)
    _, want, _, _ = oracle.run_qasm(path)
    got = run_qasm(path, fuse=3, precision=32, **opts)
    report(f"random {spec} {opts}", check_fp32(got, want, replay(n, gate_list(*spec))))
    assert np.max(np.abs(got - want)) < TOL32


@pytest.mark.parametrize("order_seed", [1, 2])
def test_tile_bit_order_fp32(oracle, tmp_path, order_seed):
    """Shuffled tile-bit orders (QSIM_OPT_DEBUG_TILE_ORDER) through the fp32 instantiation of the tile kernel."""
    spec = fp32_ref.TILE_ORDER_CIRCUIT
    path = circuits.random_circuit_file(str(tmp_path / "c.qasm"), *spec)
    _, want, _, _ = oracle.run_qasm(path)
    got = run_qasm(path, fuse=3, precision=32, debug_tile_order=order_seed)
    report(f"tile order {order_seed} {spec}", check_fp32(got, want, replay(spec[0], gate_list(*spec))))
    assert np.max(np.abs(got - want)) < TOL32


def test_randomised_geometry_sweep_fp32(oracle, tmp_path):
    """Seeded sweep over register sizes and every engine option (fp32_ref.geometry_sweep_cases: tile size, low bits, ops per
    pass, padding start, threads, grid cap), each case against the oracle."""
    for case, spec, fuse, opts in fp32_ref.geometry_sweep_cases():
        n, depth, seed, vocab = spec
        path = circuits.random_circuit_file(str(tmp_path / f"g{case}.qasm"), n, depth, seed, vocab)
        _, want, _, _ = oracle.run_qasm(path)
        got = run_qasm(path, fuse=fuse, precision=32, **opts)
        err = float(np.max(np.abs(got - want)))
        assert err < TOL32, (case, n, depth, fuse, opts, err)
        try:
            report(f"sweep {case} {spec} fuse={fuse} {opts}", check_fp32(got, want, replay(n, gate_list(*spec))))
        except AssertionError as e:
            raise AssertionError(f"case {case}: {spec} fuse={fuse} {opts}: {e}") from None


def test_dense_2q_and_sparse_blocks_fp32():
    from helpers import np_apply_2q
    n = 14
    rng = np.random.default_rng(9)
    with Simulator(n, precision=32) as sim:
        for hi, lo in [(13, 0), (5, 2), (12, 7), (1, 0), (9, 3)]:
            U = random_unitary(4, rng)
            s = _rand_state(n, 500 + hi)
            s32 = s.astype(np.complex64)
            sim.write(s)
            sim.apply_2q(U, hi, lo)
            got = sim.read()
            want = np_apply_2q(s.copy(), n, U, hi, lo)
            assert np.max(np.abs(got - want)) < TOL32, (hi, lo)
            want32 = np_apply_2q(s32.astype(np.complex128), n, U, hi, lo)
            report(f"2q ({hi}, {lo})", check_fp32(got, want32, replay(n, [("u2", hi, lo, U)], start=s32)))


def test_sampling_and_pack_fp32():
    import torch
    n = 14
    s = _rand_state(n, 60)
    with Simulator(n, precision=32) as sim:
        sim.write(s)
        s32 = s.astype(np.complex64)
        r = np.array([0.0, 0.1, 0.5, 0.999, 0.25, 1.0])
        idx = sim.sample(r)
        # sums run in fp64 over the widened amplitudes: identical to an fp64 state holding the rounded values
        with Simulator(n) as wide:
            wide.write(s32.astype(np.complex128))
            assert np.array_equal(idx, wide.sample(r))
        dst = torch.zeros((1 << n, 2), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()  # the fill runs on torch's stream, the pack on the engine's: order them
        sim.pack_bits((3, 11), dst.data_ptr())
        sim.sync()
        got = dst.cpu().numpy().reshape(-1).view(np.complex64)
    d = np.arange(1 << n, dtype=np.int64)
    rest, blk = d & ((1 << (n - 2)) - 1), d >> (n - 2)
    keep = [b for b in range(n) if b not in (3, 11)]
    src = np.zeros_like(d)
    for i, b in enumerate(keep):
        src |= ((rest >> i) & 1) << b
    for i, b in enumerate((3, 11)):
        src |= ((blk >> i) & 1) << b
    assert np.array_equal(got, s32[src])


def test_round_trip_at_n31_fp32():
    """2^31 fp32 amplitudes (16 GiB, as many bytes as the n=30 fp64 headline): circuit then its inverse returns |0...0>."""
    from gpu_quantum_simulator_amd import Circuit
    from test_gpu_parity import _inverse
    n = 31
    gates = circuits.random_gates(n, 150, 4242, "all")
    fwd = Circuit.from_gates(n, gates)
    bwd = Circuit.from_gates(n, _inverse(gates))
    with Simulator(n, precision=32) as sim:
        sim.run(fwd)
        assert abs(sim.norm2() - 1.0) < 1e-4
        assert abs(sim.read(0, 4)[0]) < 0.999
        sim.run(bwd)
        head = sim.read(0, 1 << 12)
        tail = sim.read((1 << n) - 4096, 4096)
        assert abs(sim.norm2() - 1.0) < 1e-4
    assert abs(head[0] - 1.0) < 1e-4 and np.max(np.abs(head[1:])) < 1e-4 and np.max(np.abs(tail)) < 1e-4
