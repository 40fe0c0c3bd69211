"""SchedConfig::support_weight on the device: schedules packed with the weight (QSIM_SCHED_SUPW = 5 and 10) run from a reset, so
that their first passes go over a partial support, and give the amplitudes of the oracle: 1e-10 for fp64 states, the fp32 bound of
fp32_ref for fp32 ones.  n = 14 with 2^8 tiles (64 tiles, five free slots: several partial passes) and n = 16 with the default tile;
a plain flush, the cached plan's replay, the planning step's choice, and a choice that went through the wisdom file."""
import numpy as np
import pytest

from gpu_quantum_simulator_amd import Circuit, Simulator, _lib, circuits

from fp32_ref import check_fp32, replay

pytestmark = pytest.mark.gpu
TOL = 1e-10
SHAPES = [(14, {"tile_bits": 8}, 300, 21), (16, {}, 300, 33)]  # n, engine options, gates, circuit seed

_want = {}


def _reference(oracle, tmp_path, n, depth, seed):
    """The oracle's amplitudes and the two numpy replays the fp32 bound needs, computed once per circuit."""
    if (n, seed) not in _want:
        gates = circuits.random_gates(n, depth, seed, "all")
        path = circuits.write_qasm(str(tmp_path / "c.qasm"), n, gates)
        c = Circuit.from_gates(n, gates)
        gl = [c.gate(i) for i in range(len(c))]
        _want[(n, seed)] = (gates, oracle.run_qasm(path)[1], replay(n, gl, dtype=np.complex128), replay(n, gl))
    return _want[(n, seed)]


def _check(got, ref, precision):
    _, want, ref64, ref32 = ref
    if precision == 64:
        err = float(np.max(np.abs(got - want)))
        assert err < TOL, err
    else:
        check_fp32(got, ref64, ref32)


@pytest.mark.parametrize("precision", [64, 32])
@pytest.mark.parametrize("weight", [5, 10])
@pytest.mark.parametrize("n,opts,depth,seed", SHAPES)
def test_weighted_schedules_from_a_reset(oracle, tmp_path, monkeypatch, n, opts, depth, seed, weight, precision):
    ref = _reference(oracle, tmp_path, n, depth, seed)
    c = Circuit.from_gates(n, ref[0])
    monkeypatch.setenv("QSIM_SCHED_SUPW", str(weight))
    try:
        with Simulator(n, fuse=3, precision=precision, **opts) as sim:
            sim.run(c)                      # a plain flush
            first = sim.read().copy()
            _check(first, ref, precision)
            sim.reset()
            sim.run(c)                      # the cached plan
            assert sim.read().tobytes() == first.tobytes()
            assert sim.plan_cache_stats()["replays"] == 1
            sim.choose_schedule(c)          # the planning step's choice (the variable still applies on top of it)
            sim.reset()
            sim.run(c)
            _check(sim.read(), ref, precision)
    finally:
        _lib.load().qsim_tune_table_clear()


def test_a_planned_choice_through_the_wisdom_file(oracle, tmp_path):
    """The planning step with timing (the best of every family is run, the weighted one included), its choice saved, the tables
    cleared, the file loaded: the circuit runs under the loaded choice and the file saves to the same lines again."""
    n, opts, depth, seed = SHAPES[0]
    ref = _reference(oracle, tmp_path, n, depth, seed)
    c = Circuit.from_gates(n, ref[0])
    lib = _lib.load()
    lib.qsim_tune_table_clear()
    path, again = str(tmp_path / "wisdom.txt").encode(), str(tmp_path / "again.txt").encode()
    try:
        with Simulator(n, fuse=3, **opts) as sim:
            sim.tune(c, 2, 50.0)
            sim.run(c)
            _check(sim.read(), ref, 64)
            assert lib.qsim_tune_table_save(path) == 0
            lines = open(path).read().splitlines()
            assert sum(line.startswith("sched ") for line in lines) == 1
            lib.qsim_tune_table_clear()
            assert lib.qsim_tune_table_load(path) == len(lines)
            sim.reset()
            sim.run(c)
            _check(sim.read(), ref, 64)
            assert lib.qsim_tune_table_save(again) == 0
            assert sorted(open(again).read().splitlines()) == sorted(lines)
    finally:
        lib.qsim_tune_table_clear()
