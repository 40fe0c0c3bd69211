"""Affine support on the device (QSIM_OPT_AFFINE_SUPPORT): inside one flush the tile passes over a partially written state visit
only the tiles of the affine subspace the support lies in, walked by generators, and stage every slot that fails a parity check of
the region the previous pass wrote as zero; the last tile pass in front of anything else writes the whole coordinate cube.

Both buffers are poisoned with the dense state of an unrelated circuit first.  Every case is held to the oracle at 1e-10 (fp32: the
bound of tests/fp32_ref.py) and to the same run with the option off, equal as numbers (a zero that is never computed is +0 where
the other run computed -0).  And every case reads the launch log: the shares of the register the passes visited must be the
refined ones, else the case would pass with the feature silently inactive.

Shapes: n = 14 .. 16 in the production shape (2^12 slots, 512 threads: two to four index bits outside the tile) with few clusters
per pass, so that the support grows over many passes; n = 12 with 2^8 slots on 64 threads, where generators and checks span four
outer bits.  A check mask lies on bits outside the PREVIOUS pass's tile, so it never holds one of the low bits (they are inside
every tile); in the pass that tests it, its bits play the lane, wave and register roles or stay outside the tile, and three
tile-bit orders reach all four."""
import ctypes

import numpy as np
import pytest

from gpu_quantum_simulator_amd import Circuit, Simulator, _lib, circuits

from fp32_ref import check_fp32, replay

pytestmark = pytest.mark.gpu
TOL = 1e-10
SMALL = {"tile_bits": 8, "tile_low_bits": 3}


def _ladder(n):
    gates = [("h", 0)]
    for q in range(n - 1):
        gates += [("cx", q, q + 1), ("t", q + 1)]
    return gates


def _oracle(oracle, tmp_path, n, gates):
    return oracle.run_qasm(circuits.write_qasm(str(tmp_path / "c.qasm"), n, gates))[1]


_STALE = {}


def _stale(n):
    if n not in _STALE:
        _STALE[n] = Circuit.from_gates(n, circuits.random_gates(n, 200, 5, "all"))
    return _STALE[n]


def _log(sim, n, low_bits, support=0):
    """[(kernel, high mask, tile-bit order, visited, coordinate visited)] per launch of the log; support: where the run started."""
    lib = _lib.load()
    full = (1 << n) - 1
    out = []
    for i, (rec, order) in enumerate(zip(sim.launch_log(), sim.launch_log_orders())):
        k, hm = rec[0], rec[2]
        v = ctypes.c_double()
        lib.qsim_launch_log_visited(sim._h, i, ctypes.byref(v))
        if k != "tile":
            support = full
            out.append((k, hm, order, v.value, 1.0))
            continue
        support |= (hm | ((1 << low_bits) - 1)) & full
        out.append((k, hm, order, v.value, 2.0 ** -(n - bin(support).count("1"))))
    return out


def _run(n, c, affine, poison=True, precision=64, **opts):
    opts = {"pingpong": 2, **opts}
    with Simulator(n, fuse=3, profile=True, precision=precision, affine_support=affine, **opts) as sim:
        if poison:
            sim.run(_stale(n)); sim.sync()
            sim.run(_stale(n)); sim.sync()
        sim.reset(); sim.reset_stats()
        sim.run(c)
        got = np.asarray(sim.read()).copy()
        return got, _log(sim, n, opts.get("tile_low_bits", 4 if precision == 32 else 3))  # (an fp32 state: 2^13 slots, four low bits)


def _walks(c, **shape):
    """Per pass of the plain schedule: the share it visits when the option is on (closing passes: the coordinate cube)."""
    regions = c.regions(fuse=3, **shape)
    out = []
    for i, r in enumerate(regions):
        walk = r["on"] and r["refined"] and i + 1 < len(regions) and regions[i + 1]["on"]
        out.append(r["visited"] if walk else None)
    return out


def _check_pair(oracle, tmp_path, n, gates, min_refined, exact=True, **opts):
    want = _oracle(oracle, tmp_path, n, gates)
    c = Circuit.from_gates(n, gates)
    got, log = _run(n, c, 1, **opts)
    ref, log_off = _run(n, c, 0, **opts)
    assert np.max(np.abs(got - want)) < TOL
    assert np.array_equal(got, ref)  # as numbers: -0 == +0
    assert [rec[:2] for rec in log] == [rec[:2] for rec in log_off]  # the same schedule
    assert all(v == coord for _, _, _, v, coord in log_off)
    refined = [v < coord for _, _, _, v, coord in log]
    assert sum(refined) >= min_refined, [(v, coord) for _, _, _, v, coord in log]
    assert all(v <= coord for _, _, _, v, coord in log)
    if exact:  # exactly the passes the host says, by exactly its shares
        shape = {k: opts[k] for k in ("tile_bits", "tile_low_bits", "tile_max_ops") if k in opts}
        walks = _walks(c, **shape)
        assert len(walks) == len(log)
        for w, (_, _, _, v, coord) in zip(walks, log):
            assert v == (w if w is not None else coord)
    return log


@pytest.mark.parametrize("n", [15, 16])
def test_cx_ladder(oracle, tmp_path, n):
    _check_pair(oracle, tmp_path, n, _ladder(n), 1, tile_max_ops=3)


@pytest.mark.parametrize("n,seed,opts,min_refined", [(14, 46, {"tile_max_ops": 4}, 3), (15, 1, {"tile_max_ops": 3}, 3), (16, 4, {"tile_max_ops": 4}, 3),
                                                     (12, 3, {**SMALL, "tile_max_ops": 4}, 3)])
def test_seeded_circuits_stay_below_the_cube_for_three_passes(oracle, tmp_path, n, seed, opts, min_refined):
    _check_pair(oracle, tmp_path, n, circuits.random_gates(n, 120, seed, "all"), min_refined, **opts)


def test_check_bits_in_every_role(oracle, tmp_path):
    """The bits of the check masks as the testing pass sees them: walked by the lanes of a wave (tile-local high bits 0..2 with 512
    threads and three low bits), by the waves (3..5), by a lane's registers (6..8), or outside its tile."""
    n, seed = 16, 4
    gates = circuits.random_gates(n, 120, seed, "all")
    c = Circuit.from_gates(n, gates)
    regions = c.regions(fuse=3, tile_max_ops=4)
    seen = set()
    for tile_order in (0, 1, 2):
        log = _check_pair(oracle, tmp_path, n, gates, 3, tile_max_ops=4, debug_tile_order=tile_order)
        assert len(log) == len(regions)
        for i, (r, (_, _, order, _, _)) in enumerate(zip(regions, log)):
            walked_before = i > 0 and log[i - 1][3] < log[i - 1][4]
            if not (walked_before and r["checks"]):
                continue
            bits = 0
            for mask, _ in r["checks"]:
                bits |= mask
            for b in range(n):
                if bits >> b & 1:
                    assert b >= 3
                    seen.add(("lane", "wave", "register")[order.index(b) // 3] if b in order else "outer")
    assert seen == {"lane", "wave", "register", "outer"}, seen


@pytest.mark.parametrize("defer", [0, 2])
def test_deferred_flips_on_and_off(oracle, tmp_path, defer):
    n = 15
    gates = circuits.random_gates(n, 120, 1, "all")
    want = _oracle(oracle, tmp_path, n, gates)
    c = Circuit.from_gates(n, gates)
    with Simulator(n, fuse=3, profile=True, pingpong=2, tile_max_ops=3, defer_flips=defer) as sim:
        sim.run(_stale(n)); sim.sync(); sim.run(_stale(n)); sim.sync()
        sim.reset(); sim.reset_stats()
        before = sim.deferred_flip_stats()  # (the poisoning runs defer their X gates as well)
        sim.run(c)
        got = np.asarray(sim.read()).copy()
        log = _log(sim, n, 3)
        flips = {k: v - before[k] for k, v in sim.deferred_flip_stats().items()}
    ref, log_off = _run(n, c, 0, tile_max_ops=3, defer_flips=defer)
    assert np.max(np.abs(got - want)) < TOL
    assert np.array_equal(got, ref)  # as numbers: -0 == +0
    assert [rec[:2] for rec in log] == [rec[:2] for rec in log_off]  # the same schedule
    assert all(v == coord for _, _, _, v, coord in log_off)
    assert all(v <= coord for _, _, _, v, coord in log)
    assert sum(v < coord for _, _, _, v, coord in log) >= 2
    assert flips["applied"] + flips["fallbacks"] == (1 if defer else 0)
    assert log[-1][3] == log[-1][4]  # the last pass closes
    if flips["applied"]:
        assert log[-2][3] == log[-2][4]  # ... and so does the one in front of the flipping pass


def test_a_cached_plan_replays_the_regions(oracle, tmp_path):
    n = 15
    gates = circuits.random_gates(n, 120, 1, "all")
    want = _oracle(oracle, tmp_path, n, gates)
    c = Circuit.from_gates(n, gates)
    with Simulator(n, fuse=3, profile=True, pingpong=2, tile_max_ops=3) as sim:
        runs, logs = [], []
        for _ in range(2):
            sim.run(_stale(n)); sim.sync(); sim.run(_stale(n)); sim.sync()
            sim.reset(); sim.reset_stats()
            sim.run(c)
            runs.append(np.asarray(sim.read()).copy())
            logs.append(_log(sim, n, 3))
        replays = sim.plan_cache_stats()["replays"]
    ref, log_off = _run(n, c, 0, tile_max_ops=3)
    assert np.max(np.abs(runs[0] - want)) < TOL
    assert runs[0].tobytes() == runs[1].tobytes()
    assert np.array_equal(runs[0], ref)  # as numbers: -0 == +0
    assert [rec[:2] + rec[3:] for rec in logs[0]] == [rec[:2] + rec[3:] for rec in logs[1]] and replays >= 1
    assert all(v == coord for _, _, _, v, coord in log_off)
    walks = _walks(c, tile_max_ops=3)
    assert sum(w is not None for w in walks) >= 3
    for log in logs:  # the first run and the replay: exactly the passes the host says, by exactly its shares
        assert [rec[:2] for rec in log] == [rec[:2] for rec in log_off]
        assert len(log) == len(walks)
        for w, (_, _, _, v, coord) in zip(walks, log):
            assert v == (w if w is not None else coord)
        assert sum(v < coord for _, _, _, v, coord in log) >= 3


@pytest.mark.parametrize("n,seed,opts", [(15, 1, {"tile_max_ops": 3}), (12, 3, {**SMALL, "tile_max_ops": 4})])
def test_in_place_passes(oracle, tmp_path, n, seed, opts):
    _check_pair(oracle, tmp_path, n, circuits.random_gates(n, 120, seed, "all"), 3, pingpong=0, **opts)


@pytest.mark.parametrize("n,seed,opts", [(15, 1, {"tile_bits": 12, "tile_max_ops": 3}), (16, 4, {"tile_max_ops": 3})])
def test_fp32_states(n, seed, opts):
    """The second case runs the shape an fp32 state gets by default: 2^13 slots on 512 threads, three index bits outside the tile."""
    c = Circuit.from_gates(n, circuits.random_gates(n, 120, seed, "all"))
    got, log = _run(n, c, 1, precision=32, **opts)
    ref, log_off = _run(n, c, 0, precision=32, **opts)
    assert np.array_equal(got, ref)
    assert [rec[:2] for rec in log] == [rec[:2] for rec in log_off]
    assert all(v == coord for _, _, _, v, coord in log_off)
    if "tile_bits" not in opts:
        assert all(len(order) == 9 for k, _, order, _, _ in log if k == "tile")  # 13 tile bits, four of them low
    assert all(v <= coord for _, _, _, v, coord in log)
    assert sum(v < coord for _, _, _, v, coord in log) >= 1  # (an fp32 state schedules with other search settings: fewer passes)
    gl = [c.gate(i) for i in range(len(c))]
    check_fp32(got, replay(n, gl, dtype=np.complex128), replay(n, gl))


def test_a_closing_pass_in_front_of_a_one_gate_kernel(oracle, tmp_path):
    """Two clusters per pass at most: eleven tile passes, refined ones among them, then a CX kernel.  The tile pass in front of it
    writes the whole cube, the engine writes the zeros outside it, and the read finds the oracle's state."""
    n = 12
    gates = circuits.random_gates(n, 60, 7, "all")
    log = _check_pair(oracle, tmp_path, n, gates, 2, exact=False, **SMALL, tile_max_ops=2)  # (the log also holds the launch that writes the zeros)
    kinds = [rec[0] for rec in log]
    first_other = next(i for i, k in enumerate(kinds) if k != "tile")
    assert kinds[first_other:first_other + 2] == ["init", "cx"] and first_other >= 3
    assert log[first_other - 1][3] == log[first_other - 1][4]  # the cube
    walks = _walks(Circuit.from_gates(n, gates), **SMALL, tile_max_ops=2)
    for w, (_, _, _, v, coord) in zip(walks[:first_other], log[:first_other]):
        assert v == (w if w is not None else coord)


def test_a_run_that_starts_on_a_given_support():
    """qsim_set_support as the start: V begins as the cube over the caller's support (bits 0, 1, 2, 3, 9), random amplitudes inside
    it and NaNs outside, as the receiving side of a sparse exchange leaves them; fp64 reference: the gate-by-gate replay."""
    n, bits = 15, (0, 1, 2, 3, 9)
    rng = np.random.default_rng(8)
    c = Circuit.from_gates(n, circuits.random_gates(n, 120, 1, "all"))
    gl = [c.gate(i) for i in range(len(c))]
    support = sum(1 << b for b in bits)
    inside = (np.arange(1 << n) & ~support) == 0
    init = np.where(inside, rng.standard_normal(1 << n) + 1j * rng.standard_normal(1 << n), 0)
    init /= np.linalg.norm(init)
    want = replay(n, gl, start=init, dtype=np.complex128)
    walks = [r["visited"] if r["on"] and r["refined"] and i + 1 < len(rs) and rs[i + 1]["on"] else None
             for rs in [c.regions(fuse=3, tile_max_ops=3, initial_support=support)] for i, r in enumerate(rs)]
    assert sum(w is not None for w in walks) >= 3
    for pingpong in (2, 0):
        with Simulator(n, fuse=3, profile=True, pingpong=pingpong, tile_max_ops=3) as sim:
            sim.write(np.where(inside, init, np.nan + 1j * np.nan))
            sim.set_support(support)
            sim.reset_stats()
            sim.run(c)
            got = sim.read()
            log = _log(sim, n, 3, support)
        assert not np.isnan(got).any()
        assert np.max(np.abs(got - want)) < TOL
        assert len(log) == len(walks)
        for w, (_, _, _, v, coord) in zip(walks, log):
            assert v == (w if w is not None else coord)


def _run_shards(n, c, affine, **opts):
    """(state, per shard [(kernel, high mask, visited)]) of two virtual shards, their buffers poisoned first."""
    from gpu_quantum_simulator_amd import Cluster
    lib = _lib.load()
    with Cluster(n, 2, devices=[0, 0], pingpong=2, profile=1, affine_support=affine, **opts) as cl:
        cl.run(_stale(n))
        cl.run(_stale(n))
        shards = [ctypes.c_void_p(lib.qsim_cluster_shard(cl._h, r)) for r in range(2)]
        for s in shards:
            lib.qsim_reset_stats(s)
        cl.run(c)
        got = np.asarray(cl.read()).copy()
        logs = []
        for s in shards:
            log = []
            for i in range(lib.qsim_launch_log(s, -1, None, None, None, None)):
                k, o, hm, ms, v = ctypes.c_int(), ctypes.c_int(), ctypes.c_uint64(), ctypes.c_double(), ctypes.c_double()
                lib.qsim_launch_log(s, i, ctypes.byref(k), ctypes.byref(o), ctypes.byref(hm), ctypes.byref(ms))
                lib.qsim_launch_log_visited(s, i, ctypes.byref(v))
                log.append((_lib.K_NAMES[k.value], hm.value, v.value))
            logs.append(log)
        return got, logs


def test_two_virtual_shards(oracle, tmp_path):
    """Every shard flushes its local steps through qsim_flush / qsim_flush_pack with the option on.  With it off a pass logs the
    coordinate count; with it on the same launches, never a larger share, and on some shard passes that went by their region."""
    n = 14
    gates = circuits.random_gates(n, 160, 46, "all")
    want = _oracle(oracle, tmp_path, n, gates)
    c = Circuit.from_gates(n, gates)
    got, logs = _run_shards(n, c, 1, **SMALL, tile_max_ops=4)
    ref, logs_off = _run_shards(n, c, 0, **SMALL, tile_max_ops=4)
    assert np.max(np.abs(got - want)) < TOL
    assert np.array_equal(got, ref)  # as numbers: -0 == +0
    walked = 0
    for log, log_off in zip(logs, logs_off):
        assert [rec[:2] for rec in log] == [rec[:2] for rec in log_off]  # the same launches
        assert all(v <= v_off for (_, _, v), (_, _, v_off) in zip(log, log_off))
        walked += sum(v < v_off for (_, _, v), (_, _, v_off) in zip(log, log_off))
    assert walked >= 1, (logs, logs_off)
