"""Affine support (QSIM_OPT_AFFINE_SUPPORT, SchedConfig::affine_support), host only.

After a reset the state's support stays inside an affine subspace V = o + span(g_1..g_d) of GF(2)^n: X translates it, CX maps it
linearly, diagonal gates leave it alone, only a mixing gate adds a direction.  The scheduler carries V through the schedule and
gives every tile pass over a partial support a region (Circuit.regions()): the tiles to visit, origin ^ span(gen), and the parity
checks of the region the previous pass wrote.  Here the schedule is replayed with numpy:

  * soundness — after every pass the exact non-zero set of the replayed state lies inside that pass's region, and the next
    pass's checks accept every such index;
  * the contract over stale memory — two buffers of garbage, every pass writes only the tiles of its region and stages slots
    that fail the incoming checks (or the coordinate zero mask) as zero, closing passes write the whole coordinate cube; the
    final state is the oracle's within 1e-10, so no garbage survives inside the cube of the support.

A pass is closing when the next thing to run is not a tile pass of the same schedule that carries a region (engine.cpp PassRouter
rule 7): the last pass, the pass in front of a one-gate kernel, and with deferred X gates the pass in front of the flipping one."""
import numpy as np
import pytest

from gpu_quantum_simulator_amd import Circuit, circuits
from helpers import np_apply_cx, np_apply_kq

TOL = 1e-10
GARBAGE = 7.0 - 3.0j
SHAPES = [dict(tile_bits=8, tile_low_bits=4, tile_max_ops=6), dict(tile_bits=8, tile_low_bits=2, tile_max_ops=32),
          dict(tile_bits=10, tile_low_bits=3, tile_max_ops=8), dict(tile_bits=11, tile_low_bits=3, tile_max_ops=32)]


def _by_pass(sched):
    out = []
    for entry in sched:
        while len(out) <= entry[0]:
            out.append([])
        out[entry[0]].append(entry)
    return out


def _schedule(c, defer, **shape):
    """(passes as lists of schedule entries, regions, flip mask)."""
    flips = [] if defer else None
    sched = c.schedule(fuse=3, flips=flips, **shape)
    regions = c.regions(fuse=3, defer=defer, **shape)
    passes = _by_pass(sched)
    assert len(passes) == len(regions)
    for entries, r in zip(passes, regions):
        assert entries[0][1] == r["kernel"]
    return passes, regions, (flips[0] if defer else 0)


def _apply(state, n, entries):
    for _p, _k, kind, qs, m, _f in entries:
        state = np_apply_cx(state, n, qs[0], qs[1]) if kind == "cx" else np_apply_kq(state, n, m, qs)
    return state


def _span(origin, gen):
    pts = np.array([origin], dtype=np.int64)
    for g in gen:
        pts = np.concatenate([pts, pts ^ g])
    return pts


def _tiles(n, r, walk):
    """Outer parts of the tile bases a pass visits: its region, or (closing) the coordinate cube."""
    full = (1 << n) - 1
    outer = full & ~r["tile_mask"]
    if walk:
        return _span(r["origin"], r["gen"])
    return _span(0, [1 << b for b in range(n) if (outer & r["support_before"]) >> b & 1])


def _accepts(idx, checks):
    ok = np.ones(idx.shape, dtype=bool)
    for mask, parity in checks:
        x = idx & mask
        par = np.zeros(idx.shape, dtype=np.int64)
        while np.any(x):
            par ^= x & 1
            x = x >> 1
        ok &= par == parity
    return ok


def _check_soundness(n, passes, regions, start=None):
    """start: the state the schedule finds (None: |0...0>)."""
    idx = np.arange(1 << n, dtype=np.int64)
    full = (1 << n) - 1
    state = np.zeros(1 << n, dtype=np.complex128)
    state[0] = 1
    if start is not None:
        state = start.copy()
    refined = 0
    for i, (entries, r) in enumerate(zip(passes, regions)):
        if r["on"]:  # what the pass believes of its input
            nz = idx[state != 0]
            assert np.all(nz & ~r["support_before"] & full == 0), i
            assert np.all(_accepts(nz, r["checks"])), i
            assert np.all(np.isin(nz & full & ~r["tile_mask"], _tiles(n, r, True))), i
            assert len(r["gen"]) <= 18 and len(r["checks"]) <= 18
        state = _apply(state, n, entries)
        if r["on"]:  # ... and what it leaves
            nz = idx[state != 0]
            assert np.all(np.isin(nz & full & ~r["tile_mask"], _tiles(n, r, True))), i
            assert len(_span(r["origin"], r["gen"])) == len(set(_span(r["origin"], r["gen"]).tolist()))  # independent generators
            cube = bin(full & ~r["tile_mask"] & r["support_before"]).count("1")
            assert r["refined"] == (len(r["gen"]) < cube)
            assert r["visited"] == 2.0 ** (len(r["gen"]) - bin(full & ~r["tile_mask"]).count("1"))
            refined += r["refined"]
            if i + 1 < len(regions) and regions[i + 1]["on"]:
                assert np.all(_accepts(nz, regions[i + 1]["checks"])), i
                assert bool(regions[i + 1]["checks"]) == r["refined"]
    return state, refined


def _run_over_garbage(n, passes, regions, flip, pingpong, start=None, support0=0):
    """The engine's contract, restated: which tiles a pass writes, which slots it may believe.  start, support0: the run finds
    a state that was written inside the cube of support0 only (qsim_set_support) instead of a reset."""
    idx = np.arange(1 << n, dtype=np.int64)
    full = (1 << n) - 1
    bufs = [np.full(1 << n, GARBAGE, dtype=np.complex128), np.full(1 << n, GARBAGE * 1j, dtype=np.complex128)]
    cur, support, pending, region_pending = 0, 0, True, False
    if start is not None:
        inside = idx & ~support0 & full == 0
        bufs[0][inside] = start[inside]
        support, pending = support0, False
    walked = 0
    for i, (entries, r) in enumerate(zip(passes, regions)):
        if r["kernel"] != "tile":
            assert not region_pending
            buf = bufs[cur]
            if pending:
                buf[:] = 0; buf[0] = 1
            else:
                buf[idx & ~support & full != 0] = 0  # materialize_zero_ket
            bufs[cur] = _apply(buf, n, entries)
            support, pending = full, False
            continue
        last = i + 1 == len(passes)
        before_flip = flip != 0 and i + 2 == len(passes)
        closing = last or before_flip or not (regions[i + 1]["kernel"] == "tile" and regions[i + 1]["on"])
        by_region = r["on"] and not pending and support != full and r["support_before"] == support
        assert not region_pending or (by_region and r["checks"])
        walk = by_region and not closing and r["refined"]
        after = (support | r["tile_mask"]) & full
        if pending:
            visited = idx & ~r["tile_mask"] & full == 0
            x = np.zeros(1 << n, dtype=np.complex128)
            x[0] = 1
        else:
            if support == full:
                visited = np.ones(1 << n, dtype=bool)
            elif walk:
                visited = np.isin(idx & full & ~r["tile_mask"], _tiles(n, r, True))
            else:
                visited = idx & ~after & full == 0
            valid = visited & (idx & ~support & full == 0)
            if region_pending:
                valid &= _accepts(idx, r["checks"])
            x = np.where(valid, bufs[cur], 0)
        y = _apply(x, n, entries)
        out = 1 - cur if pingpong else cur
        bufs[out][visited] = y[visited]
        assert np.all(y[~visited] == 0)  # blocks never carry an amplitude out of its tile
        cur, support, pending, region_pending = out, after, False, walk
        walked += walk
    assert not region_pending
    final = bufs[cur].copy()
    final[idx & ~support & full != 0] = 0
    return final[idx ^ flip], walked


def _oracle_state(oracle, tmp_path, n, gates):
    return oracle.run_qasm(circuits.write_qasm(str(tmp_path / "c.qasm"), n, gates))[1]


CASES = [(8, 200, 1, 0), (9, 300, 2, 1), (10, 300, 3, 1), (11, 300, 4, 0), (12, 300, 5, 2), (13, 300, 6, 2), (14, 300, 7, 3), (16, 400, 8, 3),
         (12, 300, 9, 0), (14, 400, 10, 1)]


@pytest.mark.parametrize("defer", [False, True])
@pytest.mark.parametrize("n,depth,seed,shape", CASES)
def test_regions_are_sound_and_survive_stale_memory(oracle, tmp_path, n, depth, seed, shape, defer):
    gates = circuits.random_gates(n, depth, seed, "all")
    want = _oracle_state(oracle, tmp_path, n, gates)
    passes, regions, flip = _schedule(Circuit.from_gates(n, gates), defer, **SHAPES[shape])
    state, _ = _check_soundness(n, passes, regions)
    assert np.max(np.abs(state[np.arange(1 << n) ^ flip] - want)) < TOL
    for pingpong in (True, False):
        got, _ = _run_over_garbage(n, passes, regions, flip, pingpong)
        assert np.max(np.abs(got - want)) < TOL, pingpong


def _directed(oracle, tmp_path, n, gates, shape=None, defer=False):
    shape = shape or dict(tile_bits=8, tile_low_bits=3, tile_max_ops=4)
    want = _oracle_state(oracle, tmp_path, n, gates)
    passes, regions, flip = _schedule(Circuit.from_gates(n, gates), defer, **shape)
    _check_soundness(n, passes, regions)
    walked = 0
    for pingpong in (True, False):
        got, walked = _run_over_garbage(n, passes, regions, flip, pingpong)
        assert np.max(np.abs(got - want)) < TOL
    return passes, regions, walked


def _filler(qubits):
    """Diagonal gates that keep a pass from being a single cluster without moving the support."""
    return [("t", q) for q in qubits]


def test_a_cx_ladder_keeps_one_direction(oracle, tmp_path):
    n = 16
    gates = [("h", 0)]
    for q in range(n - 1):
        gates += [("cx", q, q + 1), ("t", q + 1)]
    passes, regions, walked = _directed(oracle, tmp_path, n, gates)
    tile = [r for r in regions if r["on"]]
    assert len(tile) >= 3 and walked >= 2
    for i, r in enumerate(regions):
        closing = i + 1 == len(regions) or not regions[i + 1]["on"]
        if r["on"] and not closing:
            assert len(r["gen"]) <= 1  # at most two tiles, whatever the qubits touched so far


def test_cx_onto_a_fresh_target_then_h_on_the_control(oracle, tmp_path):
    n = 12
    gates = [("h", 9), ("cx", 9, 10), ("t", 10), ("cx", 10, 11), ("s", 11)] + _filler(range(3)) * 3 + [("h", 9), ("h", 0), ("cx", 0, 8), ("t", 8), ("h", 11)]
    _directed(oracle, tmp_path, n, gates)


@pytest.mark.parametrize("seed", [15, 26, 28])
def test_an_x_on_a_tied_qubit_gives_parity_one(oracle, tmp_path, seed):
    """X gates that are not deferred translate V: a qubit tied to another one by a CX and flipped is t = c ^ 1.  Where the scheduler
    puts which gate is its own business, so the circuits are seeded ones in which it happens: a region with a non-zero origin,
    and behind it a check that wants parity 1."""
    n = 12
    gates = circuits.random_gates(n, 300, seed, "all")
    _, regions, walked = _directed(oracle, tmp_path, n, gates, SHAPES[0])
    assert walked >= 1
    assert any(parity == 1 for r in regions for _, parity in r["checks"])
    assert any(r["origin"] != 0 for r in regions if r["refined"])


def test_two_h_on_one_qubit(oracle, tmp_path):
    n = 11
    gates = [("h", 9), ("t", 9), ("h", 9), ("cx", 9, 10), ("t", 10)] + _filler(range(4)) + [("h", 0), ("cx", 0, 8), ("t", 8), ("h", 9), ("sx", 10)]
    _directed(oracle, tmp_path, n, gates)


def test_a_dense_two_qubit_gate(oracle):
    """apply_2q with a dense 4x4: both qubits become directions at once.  (The oracle applies 1-qubit gates and cx only: the
    reference is the unfused numpy replay.)"""
    from helpers import np_apply_1q, np_apply_2q, random_unitary
    rng = np.random.default_rng(4)
    n = 12
    c = Circuit.empty(n)
    ref = np.zeros(1 << n, dtype=np.complex128)
    ref[0] = 1
    H = np.array([[1, 1], [1, -1]]) / np.sqrt(2)
    T = np.diag([1, np.exp(0.25j * np.pi)])
    def one(U, q):
        nonlocal ref
        c.append_1q(U, q); ref = np_apply_1q(ref, n, U, q)
    def cx(a, b):
        nonlocal ref
        c.append_cx(a, b); ref = np_apply_cx(ref, n, a, b)
    one(H, 8); cx(8, 9); one(T, 9)
    U4 = random_unitary(4, rng)
    c.append_2q(U4, 11, 10); ref = np.ascontiguousarray(np_apply_2q(ref, n, U4, 11, 10))
    for q in range(4):
        one(T, q)
    cx(9, 3); one(T, 3); one(H, 0); cx(0, 7); one(T, 7); one(H, 10)
    passes, regions, _ = _schedule(c, False, tile_bits=8, tile_low_bits=3, tile_max_ops=4)
    state, _ = _check_soundness(n, passes, regions)
    assert np.max(np.abs(state - ref)) < TOL
    for pingpong in (True, False):
        got, _ = _run_over_garbage(n, passes, regions, 0, pingpong)
        assert np.max(np.abs(got - ref)) < TOL


def test_the_pass_before_a_one_gate_kernel_closes(oracle, tmp_path):
    """fuse = 3 runs a cluster that no pass could take with others as a one-gate kernel; the engine writes the zeros out in front
    of it, so the tile pass before it must have written the whole cube, and the passes behind it carry no region.  Two clusters
    per pass at most: the queue reaches a CX kernel behind eleven tile passes, refined ones among them."""
    n = 12
    gates = circuits.random_gates(n, 60, 7, "all")
    c = Circuit.from_gates(n, gates)
    shape = dict(tile_bits=8, tile_low_bits=3, tile_max_ops=2)
    passes, regions, flip = _schedule(c, False, **shape)
    kinds = [r["kernel"] for r in regions]
    first_other = next(i for i, k in enumerate(kinds) if k != "tile")
    assert first_other >= 2 and regions[first_other - 1]["refined"] and any(r["refined"] for r in regions[:first_other - 1])
    assert not any(r["on"] for r in regions[first_other:])
    want = _oracle_state(oracle, tmp_path, n, gates)
    for pingpong in (True, False):
        got, _ = _run_over_garbage(n, passes, regions, flip, pingpong)
        assert np.max(np.abs(got - want)) < TOL


@pytest.mark.parametrize("defer,cube,affine", [(False, 9.57, 8.82), (True, 8.56, 8.14)])
def test_the_bench_circuit_loses_the_tiles_counted_on_the_host(defer, cube, affine):
    """n = 30, the bench circuit, default schedule: the tiles visited, in sweeps of the register, with the coordinate cube and
    with the regions (closing passes write the cube)."""
    n = 30
    c = Circuit.from_gates(n, circuits.random_gates(n, 1000, 20240117 + n, "all"))
    regions = c.regions(defer=defer)
    full = (1 << n) - 1
    total_cube = total_affine = 0.0
    support = 0
    for i, r in enumerate(regions):
        if r["kernel"] != "tile":
            total_cube += 1.0; total_affine += 1.0  # (a one-gate kernel: counted as a sweep either way)
            support = full
            continue
        outer = full & ~r["tile_mask"]
        after = (support | r["tile_mask"]) & full
        v = 2.0 ** -(n - bin(after).count("1"))
        rd = 0.0 if support == 0 else v * 2.0 ** -bin(r["tile_mask"] & ~support & full).count("1")
        total_cube += v
        last = i + 1 == len(regions) or (defer and i + 2 == len(regions))
        walk = r["on"] and r["refined"] and not last and regions[i + 1]["on"]
        total_affine += r["visited"] if walk else v
        assert r["read_share"] <= max(rd, r["visited"]) * (1 + 1e-12)
        assert r["visited"] <= v * (1 + 1e-12)
        support = after
        assert outer | r["tile_mask"] == full
    assert total_cube == pytest.approx(cube, abs=0.006)
    assert total_affine == pytest.approx(affine, abs=0.006)


def test_the_option_leaves_every_schedule_alone():
    """The same passes, blocks and matrices with and without the tracking (the plan probes schedule without it)."""
    for n, seed in ((10, 3), (14, 5)):
        c = Circuit.from_gates(n, circuits.random_gates(n, 300, seed, "all"))
        shape = dict(tile_bits=8, tile_low_bits=3)
        plain = c.passes(fuse=3, **shape)
        regions = c.regions(fuse=3, tile_max_ops=32, **shape)
        assert [p["kernel"] for p in plain] == [r["kernel"] for r in regions]
        assert [p["tile_mask"] for p in plain if p["kernel"] == "tile"] == [r["tile_mask"] for r in regions if r["kernel"] == "tile"]


def _replay_gates(n, gates, start=None):
    """The unfused circuit gate by gate with numpy, from |0...0> or from start."""
    from gpu_quantum_simulator_amd import gate_matrix
    from helpers import np_apply_1q
    state = np.zeros(1 << n, dtype=np.complex128)
    state[0] = 1
    if start is not None:
        state = start.copy()
    for g in gates:
        if g[0] == "cx":
            state = np_apply_cx(state, n, g[1], g[2])
        elif g[0] == "rz":
            state = np_apply_1q(state, n, gate_matrix(f"rz({g[1]!r})"), g[2])
        else:
            state = np_apply_1q(state, n, gate_matrix(g[0]), g[1])
    return state


@pytest.mark.parametrize("bits", [(0, 1, 2, 3, 9), (0, 1, 2, 10, 11)])
def test_a_run_that_starts_on_a_given_support(bits):
    """qsim_set_support as the start: V begins as the coordinate cube of the caller's support, a dense random state inside it
    and garbage outside (what the receiving side of a sparse exchange leaves).  Reference: the gate-by-gate numpy replay."""
    n = 12
    shape = dict(tile_bits=8, tile_low_bits=3, tile_max_ops=4)
    rng = np.random.default_rng(8)
    gates = circuits.random_gates(n, 200, 11, "all")
    c = Circuit.from_gates(n, gates)
    support = sum(1 << b for b in bits)
    inside = (np.arange(1 << n) & ~support) == 0
    start = np.where(inside, rng.standard_normal(1 << n) + 1j * rng.standard_normal(1 << n), 0)
    start /= np.linalg.norm(start)
    want = _replay_gates(n, gates, start)
    passes = _by_pass(c.schedule(fuse=3, initial_support=support, **shape))
    regions = c.regions(fuse=3, initial_support=support, **shape)
    assert len(passes) == len(regions) and regions[0]["on"] and regions[0]["support_before"] == support
    assert len(regions[0]["gen"]) >= bin(support & ~regions[0]["tile_mask"]).count("1")  # the cube's bits outside the tile are directions
    state, refined = _check_soundness(n, passes, regions, start)
    assert np.max(np.abs(state - want)) < TOL
    assert refined >= 2
    for pingpong in (True, False):
        got, walked = _run_over_garbage(n, passes, regions, 0, pingpong, start, support)
        assert walked >= 1
        assert np.max(np.abs(got - want)) < TOL, pingpong


# The soundness and stale-memory checks again under every QSIM_SCHED_* variable of tests/test_scheduler_cpu.py, each set alone to
# the non-default value that test draws: they change how the packer groups clusters, and so which V every pass sees.  The library
# reads the environment per Scheduler, so every setting runs in a child process of its own; the reference there is the
# gate-by-gate numpy replay.
KNOB_CASES = [(10, 300, 3, 1), (12, 300, 5, 2), (13, 300, 6, 0)]  # (circuits whose regions get refined under every setting)
_KNOB_CHILD = """
import json, sys
import numpy as np
sys.path.insert(0, sys.argv[1])
import test_affine_support_cpu as t
from gpu_quantum_simulator_amd import Circuit, circuits
out = []
for n, depth, seed, shape in json.loads(sys.argv[2]):
    gates = circuits.random_gates(n, depth, seed, "all")
    want = t._replay_gates(n, gates)
    for defer in (False, True):
        passes, regions, flip = t._schedule(Circuit.from_gates(n, gates), defer, **t.SHAPES[shape])
        state, refined = t._check_soundness(n, passes, regions)
        err = float(np.max(np.abs(state[np.arange(1 << n) ^ flip] - want)))
        walked = 0
        for pingpong in (True, False):
            got, walked = t._run_over_garbage(n, passes, regions, flip, pingpong)
            err = max(err, float(np.max(np.abs(got - want))))
        out.append({"err": err, "refined": int(refined), "walked": int(walked), "passes": len(passes)})
print(json.dumps(out))
"""


def test_regions_are_sound_under_every_sched_variable():
    import json
    import os
    import subprocess
    import sys
    from test_scheduler_cpu import KNOBS_LIVE, KNOBS_WITHOUT_EFFECT_HERE
    here = os.path.dirname(os.path.abspath(__file__))
    base = {k: v for k, v in os.environ.items() if not k.startswith("QSIM_SCHED_")}
    base["PYTHONPATH"] = os.pathsep.join([os.path.dirname(here), here, base.get("PYTHONPATH", "")])
    base["QSIM_NO_TORCH_PRELOAD"] = "1"  # host only
    settings = {"default": None, **KNOBS_LIVE, **KNOBS_WITHOUT_EFFECT_HERE}
    assert len(settings) == 12
    procs = {}
    for name, value in settings.items():
        env = dict(base)
        if value is not None:
            env["QSIM_SCHED_" + name] = value
        procs[name] = subprocess.Popen([sys.executable, "-c", _KNOB_CHILD, here, json.dumps(KNOB_CASES)], env=env,
                                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    for name, p in procs.items():
        out, err = p.communicate()
        assert p.returncode == 0, (name, err[-2000:])  # (an assertion of the soundness replay fails the child)
        got = json.loads(out.strip().splitlines()[-1])
        assert len(got) == 2 * len(KNOB_CASES)
        for rec in got:
            assert rec["err"] < TOL, (name, rec)
        assert sum(rec["walked"] for rec in got) >= 1 and sum(rec["refined"] for rec in got) >= 1, (name, got)
