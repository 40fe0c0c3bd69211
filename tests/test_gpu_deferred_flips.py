"""Deferred X gates on the device (QSIM_OPT_DEFER_FLIPS = 2): the X gates of a queue never reach a tile; the last tile pass of
the flush stores amplitude i at i ^ mask through the PACK store path of the tile kernel.  n = 14 and 15 (four and eight tiles of
2^12), out-of-place passes forced on, against the oracle at 1e-10.

The mask splits by which part of the store address owns each bit: the three low bits, the bits walked by the lanes of a wave
(tile-local high bits 0..2 with 512 threads), by the waves (3..5), by a lane's registers (6..8), and the bits outside the tile.
Every qubit is flipped alone, under the ascending order and under two shuffled ones (QSIM_OPT_DEBUG_TILE_ORDER), and the role it
had in the flipping pass is read back from the launch log, so that each of the five is known to have been hit; then all at once.

Where the last pass cannot take the flip, the X gates run in a pass of their own and the flush counts a fallback
(qsim_deferred_flip_stats); where a flush may not defer at all (fp32, in-place passes, other tile shapes, shards) nothing is
deferred and nothing counted.  Which kernel variant a launch ran is not in the launch log; the counters stand in for it."""
import numpy as np
import pytest

from gpu_quantum_simulator_amd import Circuit, Simulator, _lib, circuits

from fp32_ref import check_fp32, replay

pytestmark = pytest.mark.gpu
TOL = 1e-10
ROLES = ("low", "lane", "wave", "register", "outer")


def _base(n, seed, depth=160):
    """A dense-making circuit without any x: the residual mask of a circuit built on it is exactly the X gates put in."""
    return [g for g in circuits.random_gates(n, 3 * depth, seed, "all") if g[0] != "x"][:depth]


def _with_x(base, qubits, at=40):
    return base[:at] + [("x", q) for q in qubits] + base[at:]  # early: the flips are carried through most of the circuit


def _oracle(oracle, tmp_path, n, gates):
    path = circuits.write_qasm(str(tmp_path / "c.qasm"), n, gates)
    return oracle.run_qasm(path)[1]


def _role(order, q):
    if q < 3:
        return "low"
    return ROLES[1 + order.index(q) // 3] if q in order else "outer"


@pytest.mark.parametrize("n,tile_order", [(14, 0), (14, 1), (15, 2)])
def test_every_flip_position_alone_and_all_together(oracle, tmp_path, n, tile_order):
    base = _base(n, 100 + n)
    seen = set()
    with Simulator(n, fuse=3, profile=True, pingpong=2, defer_flips=2, debug_tile_order=tile_order) as sim:
        for k, qubits in enumerate([[q] for q in range(n)] + [list(range(n))]):
            gates = _with_x(base, qubits)
            want = _oracle(oracle, tmp_path, n, gates)
            sim.reset(); sim.reset_stats()
            sim.run(Circuit.from_gates(n, gates))
            got = sim.read()
            assert np.max(np.abs(got - want)) < TOL, qubits
            assert sim.deferred_flip_stats() == {"applied": k + 1, "fallbacks": 0}
            log, orders = sim.launch_log(), sim.launch_log_orders()
            assert len(log) >= 2 and all(rec[0] == "tile" for rec in log)
            seen |= {_role(orders[-1], q) for q in qubits}
    assert seen == set(ROLES)


def test_a_cached_plan_replays_the_flip(oracle, tmp_path):
    n = 14
    gates = _with_x(_base(n, 7), [0, 4, 8, 11, 13])
    want = _oracle(oracle, tmp_path, n, gates)
    c = Circuit.from_gates(n, gates)
    with Simulator(n, fuse=3, pingpong=2, defer_flips=2) as sim:
        runs = []
        for _ in range(2):
            sim.reset()
            sim.run(c)
            runs.append(sim.read().copy())
        assert np.max(np.abs(runs[0] - want)) < TOL
        assert runs[0].tobytes() == runs[1].tobytes()
        assert sim.plan_cache_stats()["replays"] == 1
        assert sim.deferred_flip_stats() == {"applied": 2, "fallbacks": 0}


def test_x_on_a_qubit_outside_the_support_falls_back():
    n = 14
    with Simulator(n, fuse=3, pingpong=2, defer_flips=2, sparse_start=1) as sim:
        sim.run(Circuit.from_gates(n, [("x", 13)]))
        got = sim.read()
        want = np.zeros(1 << n, dtype=np.complex128)
        want[1 << 13] = 1
        assert np.array_equal(got, want)
        assert sim.deferred_flip_stats() == {"applied": 0, "fallbacks": 1}


def test_a_support_that_misses_a_flipped_qubit_falls_back(oracle, tmp_path):
    """Two tile passes on qubits 0..11 only, then the flip of qubit 13: the last pass is a tile pass with one before it, but it does
    not visit the tiles the flipped amplitudes belong in."""
    n = 14
    inner = [g for g in circuits.random_gates(12, 400, 3, "all") if g[0] != "x"][:200]
    gates = _with_x(inner, [13, 2])
    want = _oracle(oracle, tmp_path, n, gates)
    with Simulator(n, fuse=3, pingpong=2, defer_flips=2, sparse_start=1) as sim:
        sim.run(Circuit.from_gates(n, gates))
        assert np.max(np.abs(sim.read() - want)) < TOL
        assert sim.deferred_flip_stats() == {"applied": 0, "fallbacks": 1}


def test_a_queue_that_ends_in_a_single_gate_kernel_falls_back(oracle, tmp_path):
    n = 14
    gates = [("x", 0), ("x", 9), ("h", 13)]  # one cluster: the gate1 kernel, no tile pass to carry the flip
    want = _oracle(oracle, tmp_path, n, gates)
    with Simulator(n, fuse=3, profile=True, pingpong=2, defer_flips=2) as sim:
        sim.run(Circuit.from_gates(n, gates))
        assert np.max(np.abs(sim.read() - want)) < TOL
        assert [rec[0] for rec in sim.launch_log()][:2] == ["init", "gate1"]  # |0...0> written out, the h alone; the X gates follow
        assert sim.deferred_flip_stats() == {"applied": 0, "fallbacks": 1}


def test_a_single_tile_pass_falls_back(oracle, tmp_path):
    """The flipping pass is out of place and must end in the state's own buffer: it needs a tile pass before it to lead away."""
    n = 14
    gates = [("h", 3), ("cx", 3, 5), ("x", 5), ("t", 5), ("h", 7), ("x", 12)]
    want = _oracle(oracle, tmp_path, n, gates)
    with Simulator(n, fuse=3, pingpong=2, defer_flips=2, sparse_start=0) as sim:
        sim.run(Circuit.from_gates(n, gates))
        assert np.max(np.abs(sim.read() - want)) < TOL
        assert sim.deferred_flip_stats() == {"applied": 0, "fallbacks": 1}


@pytest.mark.parametrize("opts", [{"pingpong": 0}, {"pingpong": 2, "tile_bits": 11}, {"pingpong": 2, "tile_threads": 256},
                                  {"pingpong": 2, "defer_flips": 0}, {"pingpong": 2, "defer_flips": 1}])
def test_flushes_that_may_not_defer_schedule_the_x_gates(oracle, tmp_path, opts):
    """In-place passes, a 2^11 tile, 256 threads (shapes without the PACK variant); the option off; and the default, which defers
    only where the planning step chose a schedule that does — none was chosen here."""
    n = 14
    gates = _with_x(_base(n, 21), [1, 5, 13])
    want = _oracle(oracle, tmp_path, n, gates)
    with Simulator(n, fuse=3, **{"defer_flips": 2, **opts}) as sim:
        sim.run(Circuit.from_gates(n, gates))
        assert np.max(np.abs(sim.read() - want)) < TOL
        assert sim.deferred_flip_stats() == {"applied": 0, "fallbacks": 0}


def test_fp32_states_do_not_defer():
    n = 14
    gates = _with_x(_base(n, 22), [1, 5, 13])
    c = Circuit.from_gates(n, gates)
    with Simulator(n, fuse=3, pingpong=2, defer_flips=2, precision=32) as sim:
        sim.run(c)
        got = sim.read()
        assert sim.deferred_flip_stats() == {"applied": 0, "fallbacks": 0}
    gl = [c.gate(i) for i in range(len(c))]
    check_fp32(got, replay(n, gl, dtype=np.complex128), replay(n, gl))


def test_a_circuit_without_x_defers_nothing(oracle, tmp_path):
    n = 14
    gates = _base(n, 23)
    want = _oracle(oracle, tmp_path, n, gates)
    with Simulator(n, fuse=3, profile=True, pingpong=2, defer_flips=2) as sim:
        sim.run(Circuit.from_gates(n, gates))
        assert np.max(np.abs(sim.read() - want)) < TOL
        assert all(rec[0] == "tile" for rec in sim.launch_log())
        assert sim.deferred_flip_stats() == {"applied": 0, "fallbacks": 0}  # no launch took the PACK variant


def test_planned_schedules_may_defer(oracle, tmp_path):
    """The default setting: deferral is one more variant for the planning step, and whichever it picks, the result stands."""
    n = 14
    gates = _with_x(_base(n, 24), [2, 6, 10, 13])
    want = _oracle(oracle, tmp_path, n, gates)
    c = Circuit.from_gates(n, gates)
    try:
        with Simulator(n, fuse=3, pingpong=2) as sim:
            sim.choose_schedule(c)
            sim.run(c)
            assert np.max(np.abs(sim.read() - want)) < TOL
            st = sim.deferred_flip_stats()
            assert st["applied"] + st["fallbacks"] <= 1
    finally:
        _lib.load().qsim_tune_table_clear()  # the choice is kept process-wide


def test_shards_keep_it_off(oracle, tmp_path):
    from gpu_quantum_simulator_amd import Cluster
    n = 14
    gates = _with_x(_base(n, 25, depth=240), [0, 5, 12, 13])
    want = _oracle(oracle, tmp_path, n, gates)
    with Cluster(n, 2, devices=[0, 0], pingpong=2) as cl:
        cl.run(Circuit.from_gates(n, gates))
        assert np.max(np.abs(cl.read() - want)) < TOL
