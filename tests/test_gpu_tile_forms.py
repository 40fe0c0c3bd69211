"""Every block form of k_tile on the device, by name: the directed circuits of tile_forms_ref.py at each tile shape of
fp32_ref.TILE_SHAPES, in both precisions, under the default tile order and a shuffled one, with a census of what was launched.

Shapes: n = B + 2 qubits, four tiles — two selector bits can lie outside the tile, and a block whose bank 0 is the identity is
skipped on some tiles and run on others.  The shapes cover k_tile's two items per thread (12/256, 13/512), one full round
(11/256, 12/512, 13/1024) and the guarded tails (8/64 ... 10/512, 11/512, 12/1024).  The largest state is 2^15 amplitudes; a case
is a write, at most a dozen gates and a read.

Checks: fp64 against helpers.np_apply_kq under the suite's 1e-10; fp32 by the fp32_ref criterion (C, FLOOR, REF_CAP), as
test_gpu_fp32.py applies it.  The census comes from qsim_launch_log_block_flags (profile = 2), i.e. from the headers of the
records the kernel was given: each case must have launched the form it is named after, and over the module every cell of the
coverage table of test_tile_records_cpu.py must have been launched at every shape where it can exist.  A missing cell fails.

What this module does NOT prove: a record that drops a needed barrier between the reads and the writes races on the device and
mostly gives the right answer anyway.  That property is pinned deterministically on the host
(test_tile_records_cpu.py, the hazard-freedom runs of its record check); nothing here tries to provoke the race.
"""
import functools
import time

import numpy as np
import pytest

from gpu_quantum_simulator_amd import Simulator
import fp32_ref
import tile_forms_ref as F

pytestmark = pytest.mark.gpu
TOL = 1e-10
LOW_BITS = F.DEVICE_LOW_BITS
ORDER_SEED = 5


def _apply(sim, gates):
    for g in gates:
        if g[0] == "cx":
            sim.apply_cx(g[1], g[2])
        elif g[0] == "u1":
            sim.apply_1q(g[2], g[1])
        else:
            sim.apply_2q(g[3], g[1], g[2])


@functools.lru_cache(maxsize=None)
def _run_shape(B, threads, precision):
    """Runs every directed case of tile size B at this shape and precision under both tile orders; asserts accuracy and the
    case's own form; returns (forms launched, worst error, seconds)."""
    t0 = time.perf_counter()
    opts = {"tile_bits": B, "tile_low_bits": LOW_BITS}
    if threads:
        opts["tile_threads"] = threads
    launched, worst = set(), 0.0
    for order in (0, ORDER_SEED):
        if order:
            opts["debug_tile_order"] = order
        n = B + 2
        with Simulator(n, fuse=3, profile=2, precision=precision, **opts) as sim:
            for name, (n_, gates, form, s0, want64, want32, ref32) in F.references(B).items():
                sim.write(s0)
                sim.reset_stats()
                _apply(sim, gates)
                got = sim.read()
                forms = {F.form_of(b) for blocks in sim.launch_log_block_flags() for b in blocks}
                if precision == 64:
                    err = float(np.max(np.abs(got - want64)))
                    assert err < TOL, (name, B, threads, order, err)
                else:
                    err, _ = fp32_ref.check_fp32(got, want32, ref32)
                worst = max(worst, err)
                assert form in forms, f"{name} at {B}/{threads} order {order}: launched {sorted(forms)}, not {form}"
                launched |= forms
    return launched, worst, time.perf_counter() - t0


@pytest.mark.parametrize("precision", [64, 32])
@pytest.mark.parametrize("B,threads", fp32_ref.TILE_SHAPES)
def test_directed_forms(B, threads, precision):
    launched, worst, seconds = _run_shape(B, threads, precision)
    kind = "max abs err" if precision == 64 else "rel err"
    print(f"\ntile forms {B}/{threads or 'default'} fp{precision}: {len(F.references(B))} cases x 2 orders, {len(launched)} forms launched, "
          f"worst {kind} {worst:.3e}, {seconds:.2f} s")


def test_census_covers_the_table_at_every_shape():
    """Every cell of the coverage table (tile_forms_ref.required_cells) was launched at every shape and precision where
    it exists; prints the table as reached and the worst error per precision."""
    worst = {64: 0.0, 32: 0.0}
    for B, threads in fp32_ref.TILE_SHAPES:
        cells, nsels = F.required_cells(B)
        for precision in (64, 32):
            launched, w, _ = _run_shape(B, threads, precision)
            worst[precision] = max(worst[precision], w)
            missing = [c for c in cells if not F.covers(launched, c)] + [("nsel", ns) for ns in nsels if not any(f[4] == ns for f in launched)]
            assert not missing, (B, threads, precision, missing, sorted(launched))
            assert not any(f[0] == 3 and f[3] for f in launched), "barrier bit at K = 3: one part per group has no other part to wait for"
            if precision == 64:
                print(f"\ncensus {B}/{threads or 'default'}: (K, T, skips, barrier, nsel) launched: {sorted(launched)}")
    print(f"\ntile forms worst error: fp64 max abs {worst[64]:.3e}, fp32 rel {worst[32]:.3e}")


def test_block_flags_of_a_replayed_plan():
    """qsim_launch_log_block_flags reads the records the kernel was given — also when the pass is replayed from the plan cache,
    whose records live on the device only."""
    B = 12
    n, gates, form, s0, want64, _, _ = F.references(B)["sel2_k3_t2"]
    assert len(gates) >= 8  # shorter queues are not cached
    with Simulator(n, fuse=3, profile=2, tile_bits=B, tile_low_bits=LOW_BITS) as sim:
        seen = []
        for _ in range(2):
            sim.write(s0)
            sim.reset_stats()
            _apply(sim, gates)
            got = sim.read()
            assert np.max(np.abs(got - want64)) < TOL
            seen.append(sim.launch_log_block_flags())
        assert sim.plan_cache_stats()["replays"] >= 1
    assert seen[0] == seen[1] and form in {F.form_of(b) for blocks in seen[1] for b in blocks}
    with Simulator(n, fuse=3, profile=1, tile_bits=B, tile_low_bits=LOW_BITS) as sim:  # recorded under profile = 2 only
        sim.write(s0)
        _apply(sim, gates)
        sim.read()
        assert all(blocks == [] for blocks in sim.launch_log_block_flags())
