"""Tile passes over a partially written state do not LOAD the slots outside the support (k_tile SPARSE): both buffers are
pre-filled with the dense amplitudes of an unrelated circuit, then the state is reset and the circuit run.  Whatever role
the qubits new to the support play in a pass (register, lane, wave; more than three of them; tiles with tail guards), the
amplitudes equal those of the same run with QSIM_OPT_SPARSE_START off bit for bit, and the oracle's within 1e-10 (fp32:
the project's fp32 bound).  Further down: which role the new bits really play in these cases, new LOW bits (qsim_set_support), a
qsim_flush_pack ending on a partial state, and measured orders with the wisdom file's round trip.

Which circuits can be compared bit for bit.  With sparse start off the scheduler does not know the support, and it then
builds OTHER passes out of the same gates (pass_builder.cpp): (1) build_passes tries a pass that stays inside the support
first (cheap_margin), and (2) tile_pass takes qubits a block is merely block-diagonal in into the tile only when they are
inside the support, which changes what merge_blocks multiplies together on the host.  Other products of the same
matrices round differently, so two such runs of a general circuit agree to ~1e-17 and not in the last bit — with or
without the kernel under test (the parent commit shows the same: five of these cases at 4.6e-18 .. 7.3e-18;
tests/test_gpu_parity.py::test_sparse_start_visits_only_the_support compares the same pair to 1e-13 for that reason).
The bit-for-bit comparison therefore runs on circuits for which both runs provably multiply the same matrices
(`_shared_schedule_gates`): every diagonal gate and every cx control sits on one of the three lowest qubits, which are
inside every tile, so (2) has nothing to decide, and QSIM_SCHED_CHEAP=0 switches (1) off for BOTH runs.  Their support
still grows a few qubits per pass, the cx gates entangle every qubit with the low ones, and the state is dense inside its
support.  General circuits (all gates anywhere) are held to the oracle, and to the same sparse run on buffers that never
held stale data, bit for bit — which is the statement "stale memory outside the support is never seen" itself."""
import ctypes

import numpy as np
import pytest

from gpu_quantum_simulator_amd import Circuit, Simulator, _lib, circuits

from fp32_ref import check_fp32, replay

pytestmark = pytest.mark.gpu
TOL = 1e-10

# (n, options): ascending orders put the new bits into the register role (1, 2, 3 of them, by the circuit's own support growth);
# debug_tile_order shuffles them into the lane and wave roles (also with tile_low_bits 4); tile_bits 9 runs
# 128 threads (tiles with tail guards exist only for registers below 2^8: test_new_low_bits); tile_bits 13 admits more than three new bits in one pass.
GEOMETRIES = [
    (16, {"tile_bits": 10}),
    (17, {"tile_bits": 12}),
    (18, {"tile_bits": 12, "debug_tile_order": 1}),
    (18, {"tile_bits": 12, "debug_tile_order": 2}),
    (16, {"tile_bits": 10, "tile_low_bits": 4, "debug_tile_order": 3}),
    (15, {"tile_bits": 9}),
    (17, {"tile_bits": 13}),
    (17, {"tile_bits": 11, "tile_threads": 512}),
]


def _windowed_gates(n, seed, depth=200):
    full = circuits.random_gates(n, 8 * depth, seed, "all")
    rng = np.random.default_rng(seed)
    order = [int(q) for q in rng.permutation(n)]
    out = []
    for g in full:
        width = min(n, 2 + len(out) * n // depth)
        allowed = set(order[:width])
        qs = [x for x in g[1:] if isinstance(x, int)]
        if all(q in allowed for q in qs):
            out.append(g)
        if len(out) == depth:
            break
    return out


def _shared_schedule_gates(n, seed, depth=200):
    """Gates whose passes do not depend on whether the scheduler knows the support (module docstring): h / sx / x anywhere,
    cx with the control on qubits 0..2, diagonal gates on qubits 0..2; the high qubits in use widen as the circuit goes on."""
    rng = np.random.default_rng(seed)
    order = [int(q) for q in rng.permutation(np.arange(3, n))]
    out = []
    while len(out) < depth:
        hi = order[:min(n - 3, 1 + len(out) * (n - 3) // depth)]
        r = int(rng.integers(0, 10))
        q = int(hi[rng.integers(len(hi))])
        lo = int(rng.integers(3))
        if r < 4:
            out.append((["h", "sx", "x", "h"][r], q))
        elif r < 7:
            out.append(("cx", lo, q))
        elif r < 8:
            out.append(("rz", float(rng.uniform(0, 6.28)), lo))
        elif r < 9:
            out.append((["t", "s", "z", "tdg", "sdg"][int(rng.integers(5))], lo))
        else:
            out.append((["h", "sx"][int(rng.integers(2))], lo))
    return out


def _run(n, c, stale, sparse, precision=64, **opts):
    with Simulator(n, fuse=3, profile=True, pingpong=2, precision=precision, sparse_start=sparse, **opts) as sim:
        if stale is not None:
            sim.run(stale); sim.sync()   # dense garbage in the state buffer ...
            sim.run(stale); sim.sync()   # ... and, the passes going out of place, in the other one
        sim.reset(); sim.reset_stats()
        sim.run(c)
        got = sim.read()
        return got, sim.stats()


@pytest.mark.parametrize("n,opts", GEOMETRIES)
def test_stale_memory_outside_the_support_is_never_seen(oracle, tmp_path, monkeypatch, n, opts):
    stale = Circuit.from_gates(n, circuits.random_gates(n, 300, 5, "all"))
    # a general circuit: the oracle, and the same run on buffers without stale data
    gates = _windowed_gates(n, 900 + n)
    path = circuits.write_qasm(str(tmp_path / "c.qasm"), n, gates)
    _, want, _, _ = oracle.run_qasm(path)
    c = Circuit.from_file(path)
    got, st = _run(n, c, stale, 1, **opts)
    clean, _ = _run(n, c, None, 1, **opts)
    assert np.max(np.abs(got - want)) < TOL
    assert np.array_equal(got.view(np.float64), clean.view(np.float64))
    tile = st["kernels"]["tile"]
    assert tile["bytes"] < tile["launches"] * 32.0 * (1 << n)  # partial passes were charged less than full ones
    # a circuit both schedulers cut the same way: sparse start off, bit for bit
    monkeypatch.setenv("QSIM_SCHED_CHEAP", "0")
    gates = _shared_schedule_gates(n, 900 + n)
    path = circuits.write_qasm(str(tmp_path / "s.qasm"), n, gates)
    _, want, _, _ = oracle.run_qasm(path)
    c = Circuit.from_file(path)
    got, _ = _run(n, c, stale, 1, **opts)
    ref, _ = _run(n, c, stale, 0, **opts)
    assert np.max(np.abs(got - want)) < TOL
    assert np.array_equal(got.view(np.float64), ref.view(np.float64))


@pytest.mark.parametrize("n,opts", [(16, {"tile_bits": 10}), (18, {"tile_bits": 13, "debug_tile_order": 1})])
def test_fp32_states(monkeypatch, n, opts):
    stale = Circuit.from_gates(n, circuits.random_gates(n, 300, 6, "all"))
    c = Circuit.from_gates(n, _windowed_gates(n, 700 + n))
    got, _ = _run(n, c, stale, 1, precision=32, **opts)
    clean, _ = _run(n, c, None, 1, precision=32, **opts)
    assert np.array_equal(np.asarray(got).view(np.float32), np.asarray(clean).view(np.float32))
    gl = [c.gate(i) for i in range(len(c))]
    check_fp32(got, replay(n, gl, dtype=np.complex128), replay(n, gl))
    monkeypatch.setenv("QSIM_SCHED_CHEAP", "0")
    c = Circuit.from_gates(n, _shared_schedule_gates(n, 700 + n))
    got, _ = _run(n, c, stale, 1, precision=32, **opts)
    ref, _ = _run(n, c, stale, 0, precision=32, **opts)
    assert np.array_equal(np.asarray(got).view(np.float32), np.asarray(ref).view(np.float32))
    gl = [c.gate(i) for i in range(len(c))]
    check_fp32(got, replay(n, gl, dtype=np.complex128), replay(n, gl))


def _threads(opts, precision=64):
    """Threads per workgroup launch_tile picks for a geometry (launch.inc tile_threads)."""
    b = opts.get("tile_bits", 12)
    if opts.get("tile_threads"):
        return opts["tile_threads"]
    return {9: 128, 10: 256, 11: 256, 12: 512, 13: 512 if precision == 32 else 1024}.get(b, 64)  # up to 2^8: 64


def _new_bit_roles(sim, n, low_bits, threads, support=0):
    """Per sparse launch of the log: {(role, how many new bits play it)} — new = tile bits outside the running support."""
    out = []
    lib = _lib.load()
    lanes, tbits = 6, threads.bit_length() - 1
    for i, ((k, _, hm, _), order) in enumerate(zip(sim.launch_log(), sim.launch_log_orders())):
        if k != "tile":
            support = (1 << n) - 1
            continue
        v, r = ctypes.c_double(), ctypes.c_double()
        lib.qsim_launch_log_visited(sim._h, i, ctypes.byref(v))
        lib.qsim_launch_log_read_share(sim._h, i, ctypes.byref(r))
        roles = {}
        for j, b in enumerate(order):
            if not (support >> b) & 1:
                slot = j + low_bits
                role = "lane" if slot < lanes else "wave" if slot < tbits else "register"
                roles[role] = roles.get(role, 0) + 1
        for b in range(low_bits):
            if not (support >> b) & 1:
                roles["low"] = roles.get("low", 0) + 1
        z = sum(roles.values())
        if support != 0:  # (the generating pass reads nothing)
            assert r.value == pytest.approx(v.value / (1 << z), rel=1e-12), (i, roles)
            if z:
                out.append(roles)
        support |= hm | ((1 << low_bits) - 1)
    return out


def test_every_role_of_the_new_bits_occurs(capsys):
    """The cases above are only worth their names while their circuits really put new bits into each role: register (1, 2
    and 3 of them, alone), more than the register role holds, lane and wave."""
    seen = set()
    for n, opts in GEOMETRIES:
        for gates in (_windowed_gates(n, 900 + n), _shared_schedule_gates(n, 900 + n)):
            with Simulator(n, fuse=3, profile=True, pingpong=2, **opts) as sim:
                sim.run(Circuit.from_gates(n, gates)); sim.sync()
                threads = _threads(opts)
                regs = (opts["tile_bits"] - (threads.bit_length() - 1))
                for roles in _new_bit_roles(sim, n, opts.get("tile_low_bits", 3), threads):
                    if set(roles) == {"register"}:
                        seen.add(("register", min(roles["register"], regs + 1)))
                    for role in roles:
                        if role != "register":
                            seen.add((role,))
                    if roles.get("register", 0) == regs and len(roles) > 1:
                        seen.add(("more than the registers hold",))
    with capsys.disabled():
        print("roles seen:", sorted(seen))
    for want in [("register", 1), ("register", 2), ("register", 3), ("lane",), ("wave",), ("more than the registers hold",)]:
        assert want in seen, (want, sorted(seen))


def test_new_low_bits(tmp_path):
    """qsim_set_support with a LOW tile bit outside the support (after a reset the low bits are always inside): lanes whose own
    index has that bit are masked off for the whole batch.  NaNs outside the support, as the receiving side of a sparse exchange
    leaves them; fp64 reference: the gate-by-gate replay in complex128."""
    rng = np.random.default_rng(5)
    # (n = 6: the whole register is one 2^6 tile on 64 threads, the only shape with tail guards: it loads every slot and zeroes)
    for n, tile_bits, bits in ((15, 12, (0, 2, 3, 5, 6, 9, 10, 12)), (15, 10, (2, 3, 4, 5, 6, 7, 8, 11)), (15, 9, (0, 1, 4, 5, 6, 13)), (6, 12, (0, 2, 3))):
        c = Circuit.from_gates(n, circuits.random_gates(n, 300, 91, "all"))
        gl = [c.gate(i) for i in range(len(c))]
        support = sum(1 << b for b in bits)
        inside = (np.arange(1 << n) & ~support) == 0
        init = np.where(inside, rng.standard_normal(1 << n) + 1j * rng.standard_normal(1 << n), 0)
        init /= np.linalg.norm(init)
        want = replay(n, gl, start=init, dtype=np.complex128)
        for order in (0, 2):
            with Simulator(n, fuse=3, profile=True, pingpong=2, tile_bits=tile_bits, debug_tile_order=order) as sim:
                sim.write(np.where(inside, init, np.nan + 1j * np.nan))
                sim.set_support(support)
                sim.reset_stats()
                sim.run(c)
                got = sim.read()
                roles = _new_bit_roles(sim, n, 3, _threads({"tile_bits": min(tile_bits, n)}), support)
            assert not np.isnan(got).any()
            assert np.max(np.abs(got - want)) < TOL
            assert roles and "low" in roles[0], roles


def test_flush_pack_ending_on_a_partial_state(oracle, tmp_path):
    """k_tile<12, 512, PACK, SPARSE>: the queue ends in a pass over a partial support that also does the re-layout of an exchange.
    Stale dense data in both buffers; the packed amplitudes equal the oracle's where the receivers look, and the same run
    without stale data bit for bit."""
    import torch
    n = 16
    low = circuits.random_gates(10, 260, 11, "all")                     # qubits 0..9: at least one pass, support stays partial
    m = {0: 0, 1: 1, 2: 2, 3: 13, 4: 14}
    late = [tuple(m[x] if isinstance(x, int) else x for x in g) for g in circuits.random_gates(5, 60, 12, "all")]
    gates = low + late                                                  # ... then qubits 13 and 14 join: new to the support
    path = circuits.write_qasm(str(tmp_path / "p.qasm"), n, gates)
    _, want, _, _ = oracle.run_qasm(path)
    c = Circuit.from_file(path)
    stale = Circuit.from_gates(n, circuits.random_gates(n, 300, 5, "all"))
    bits = (3, 14)
    src = _pack_src_index(n, bits)
    outs = []
    for with_stale in (True, False):
        with Simulator(n, fuse=3, profile=True, pingpong=2, tile_bits=12) as sim:
            out = torch.full((1 << n, 2), float("nan"), dtype=torch.float64, device="cuda")
            torch.cuda.synchronize()
            if with_stale:
                sim.run(stale); sim.sync(); sim.run(stale); sim.sync()
            sim.reset(); sim.reset_stats()
            needed = sim.support_after(c)
            assert needed != (1 << n) - 1                               # still partial at the end
            sim.run(c)
            at, fused = sim.flush_pack(bits, out.data_ptr(), needed=needed)
            sim.sync()
            assert fused and at == out.data_ptr()
            roles = _new_bit_roles(sim, n, 3, 512)
            assert roles and roles[-1], roles                           # the last (packing) pass admitted new qubits
            got = out.cpu().numpy().reshape(-1).view(np.complex128)
            inside = (src & ~needed) == 0
            assert not np.isnan(got[inside]).any()
            assert np.max(np.abs(got[inside] - want[src][inside])) < TOL
            outs.append(got[inside].copy())
    assert np.array_equal(outs[0].view(np.float64), outs[1].view(np.float64))


def _pack_src_index(n, bits):
    """Source index of every position of the packed layout of qsim_pack_bits."""
    k = len(bits)
    d = np.arange(1 << n, dtype=np.int64)
    rest, blk = d & ((1 << (n - k)) - 1), d >> (n - k)
    keep = [b for b in range(n) if b not in bits]
    src = np.zeros_like(d)
    for i, b in enumerate(keep):
        src |= ((rest >> i) & 1) << b
    for i, b in enumerate(bits):
        src |= ((blk >> i) & 1) << b
    return src


def test_measured_orders_on_partial_passes(oracle, tmp_path):
    """qsim_tune_circuit times a pass over a partial support on that support, its new bits topmost in every candidate, and
    enters it under a key of its own ("part <new bits>" in the file).  Orders never change amplitudes: the run after planning,
    the run after a save / clear / load round trip equals the planned run bit for bit, and the run under a parent-format line
    for the same bit set (an order of the FULL pass, which must not be applied to the partial one) the unplanned run."""
    lib = _lib.load()
    n = 18
    gates = _windowed_gates(n, 918)
    path = circuits.write_qasm(str(tmp_path / "c.qasm"), n, gates)
    _, want, _, _ = oracle.run_qasm(path)
    c = Circuit.from_file(path)
    stale = Circuit.from_gates(n, circuits.random_gates(n, 300, 5, "all"))
    wisdom = str(tmp_path / "wisdom.txt").encode()

    def run(sim):
        sim.reset(); sim.run(stale); sim.sync(); sim.run(stale); sim.sync()
        sim.reset(); sim.reset_stats(); sim.run(c)
        got = sim.read()
        log = [(hm, order) for (k, _, hm, _), order in zip(sim.launch_log(), sim.launch_log_orders()) if k == "tile"]
        return got, log, _new_bit_roles(sim, n, 3, 512)

    lib.qsim_tune_table_clear()
    try:
        with Simulator(n, fuse=3, profile=True, pingpong=2, tile_bits=12) as sim:
            base, log0, roles0 = run(sim)
            assert np.max(np.abs(base - want)) < TOL and roles0
            rep = sim.tune(c, max_candidates=6, budget_ms=0)
            assert rep["passes_tuned"] >= 2
            tuned, log1, roles1 = run(sim)
            assert np.max(np.abs(tuned - want)) < TOL       # (planning may also pick another schedule: other roundings than `base`)
            assert all(set(r) == {"register"} for r in roles1 if sum(r.values()) <= 3), roles1   # new bits where the loads are dropped
            assert lib.qsim_tune_table_save(wisdom) == 0
            lines = open(wisdom.decode()).read().splitlines()
            parts = [l for l in lines if l.startswith("part ")]
            assert parts, lines
            size = lib.qsim_tune_table_size()
            lib.qsim_tune_table_clear()
            assert lib.qsim_tune_table_load(wisdom) >= size and lib.qsim_tune_table_size() == size
            again, log2, _ = run(sim)
            assert np.array_equal(again, tuned) and log2 == log1
            # a line in the parent's format for the bit set of a partial pass, highest bit first: an order of the full pass
            lib.qsim_tune_table_clear()
            sup = 0
            target = None
            for hm, order in log0:
                if sup and (hm & ~sup):
                    target = (hm, [b for b in order if (sup >> b) & 1] + [b for b in order if not (sup >> b) & 1])
                    break
                sup |= hm | 7
            assert target
            hm, placed = target
            desc = sorted(placed, reverse=True)
            with open(wisdom.decode(), "w") as f:
                f.write(f"{n} 0 12 3 {hm:x} 1.0000 2.0000 " + " ".join(str(b) for b in desc) + "\n")
            assert lib.qsim_tune_table_load(wisdom) == 1
            last, log3, _ = run(sim)
            assert np.array_equal(last, base)
            got_order = [order for h, order in log3 if h == hm][0]
            assert got_order == sorted(b for b in placed if (sup >> b) & 1) + sorted(b for b in placed if not (sup >> b) & 1)
    finally:
        lib.qsim_tune_table_clear()


def test_run_bytes_equal_the_plan():
    n = 18
    c = Circuit.from_gates(n, _windowed_gates(n, 31))
    with Simulator(n, fuse=3, profile=True, tile_bits=10) as sim:
        sim.run(c); sim.sync()
        moved = sim.stats()["kernels"]["tile"]["bytes"]  # (the zeros written behind a state that ends partial are not in a plan)
        shares = []
        for i, rec in enumerate(sim.launch_log()):
            v, r = ctypes.c_double(), ctypes.c_double()
            _lib.load().qsim_launch_log_visited(sim._h, i, ctypes.byref(v))
            _lib.load().qsim_launch_log_read_share(sim._h, i, ctypes.byref(r))
            shares.append((v.value, r.value))
    passes = c.passes(fuse=3, tile_bits=10, tile_low_bits=3)
    assert all(p["kernel"] == "tile" for p in passes)
    assert moved == pytest.approx(sum(p["bytes"] for p in passes), rel=1e-12)
    assert shares[0][1] == 0.0 and any(0.0 < r < v for v, r in shares)  # reads dropped in some pass


def test_cached_plan_replay_on_a_partial_state(oracle, tmp_path):
    n = 17
    gates = _windowed_gates(n, 77)
    path = circuits.write_qasm(str(tmp_path / "c.qasm"), n, gates)
    _, want, _, _ = oracle.run_qasm(path)
    c = Circuit.from_file(path)
    stale = Circuit.from_gates(n, circuits.random_gates(n, 300, 9, "all"))
    with Simulator(n, fuse=3, pingpong=2, tile_bits=12) as sim:
        outs = []
        for _ in range(3):  # the second and third run replay the cached plan
            sim.reset(); sim.run(stale); sim.sync(); sim.run(stale); sim.sync()
            sim.reset(); sim.run(c)
            outs.append(sim.read())
    assert np.max(np.abs(outs[0] - want)) < TOL
    assert np.array_equal(outs[0], outs[1]) and np.array_equal(outs[0], outs[2])
