"""qsim_support_after predicts what a flush leaves.  The engine has ONE statement of how a flush schedules a queue (engine.cpp
flush_rule): the flush runs by it, and qsim_support_after — from which a cluster's planner derives what the receivers of an
exchange look at — asks it.  This file pins the contract between the two on the smallest shapes at which a run stays partial
over several tile passes and an X gate can meet a qubit outside the support: for every way the rule can decide (X gates
deferred never / where planned / always, passes in place / out of place, both precisions, no planning / the model's schedule
choice / a measured one, a run from a reset / on a written state declared partial), the support the engine reports after
run + flush is the predicted one, the amplitudes are the reference's, and a second run of the same circuit replays the cached
plan to the same bits.

References.  From a reset: the oracle's run of the circuit.  On a written state: the state is the oracle's result of a prefix
circuit on the qubits of the declared support (so it is zero outside it by construction), and the reference is the oracle's
run of prefix + circuit.  fp32 states are held to the criterion of tests/fp32_ref.py (a written start is rounded by the write,
so truth and fp32 replay both start from the rounded state, as fp32_ref says)."""
import numpy as np
import pytest

from gpu_quantum_simulator_amd import Circuit, Simulator, _lib, circuits

from fp32_ref import check_fp32, replay

pytestmark = pytest.mark.gpu
TOL = 1e-10  # the file-local bound of test_gpu_sparse_reads.py

# n, engine options, qubits of the opening gates, the two high qubits that join late, the high qubit of the written start's support
SHAPES = {
    14: ({"tile_bits": 8, "tile_low_bits": 3}, 6, (11, 12), 13),
    16: ({"tile_bits": 12}, 10, (13, 14), 15),
}


def _on(gates, qubit_of):
    return [tuple(qubit_of[x] if isinstance(x, int) else x for x in g) for g in gates]


def _gates(n):
    """The pattern of test_flush_pack_ending_on_a_partial_state: gates on the low qubits (the support stays partial over the
    passes they make), then 40 that bring in two high qubits; the vocabulary has x, so there are flips."""
    _, low, late, _ = SHAPES[n]
    return circuits.random_gates(low, 260, 11 + n, "all") + _on(circuits.random_gates(5, 40, 12 + n, "all"), {0: 0, 1: 1, 2: 2, 3: late[0], 4: late[1]})


def _start_mask(n):
    _, low, _, top = SHAPES[n]
    return ((1 << low) - 1) | (1 << top)


_refs = {}


def _reference(oracle, tmp_path_factory, n, start):
    """(circuit, start state or None, its support, fp64 truth, {precision: (want, ref32)}), computed once per (n, start)."""
    if (n, start) in _refs:
        return _refs[n, start]
    d = tmp_path_factory.mktemp(f"flush_rule_{n}_{start}")
    gates = _gates(n)
    c = Circuit.from_text(circuits.qasm_text(n, gates))
    listed = [c.gate(i) for i in range(len(c))]
    if start == "reset":
        state, mask = None, 0
        _, want, _, _ = oracle.run_qasm(circuits.write_qasm(str(d / "c.qasm"), n, gates))
        want32, ref32 = want, replay(n, listed)
    else:
        _, low, _, top = SHAPES[n]
        prefix = _on(circuits.random_gates(low + 1, 80, 13 + n, "all"), {**{q: q for q in range(low)}, low: top})
        mask = _start_mask(n)
        _, state, _, _ = oracle.run_qasm(circuits.write_qasm(str(d / "p.qasm"), n, prefix))
        assert not np.any(state[(np.arange(1 << n) & ~mask) != 0])  # zero outside the declared support
        assert np.any(state[1 << top:]) and np.any(state[:1 << top])  # ... and using the high qubit inside it
        _, want, _, _ = oracle.run_qasm(circuits.write_qasm(str(d / "pc.qasm"), n, prefix + gates))
        rounded = state.astype(np.complex64)
        want32, ref32 = replay(n, listed, start=rounded, dtype=np.complex128), replay(n, listed, start=rounded)
    _refs[n, start] = (c, state, mask, want, want32, ref32)
    return _refs[n, start]


def _run(sim, c, state, mask):
    """One run from the start under test; returns (support reported after the flush, amplitudes)."""
    if state is None:
        sim.reset()
    else:
        sim.write(state)
        sim.set_support(mask)
    sim.run(c)
    sim.flush()
    support = sim.get_support()[0]
    return support, sim.read()


@pytest.fixture
def clean_tables():
    clear = _lib.load().qsim_tune_table_clear
    clear()
    yield
    clear()


@pytest.mark.parametrize("start", ["reset", "written"])
@pytest.mark.parametrize("planning", ["none", "choose", "tune"])
@pytest.mark.parametrize("precision", [64, 32])
@pytest.mark.parametrize("pingpong", [0, 2])
@pytest.mark.parametrize("defer_flips", [0, 1, 2])
@pytest.mark.parametrize("n", sorted(SHAPES))
def test_support_after_predicts_the_flush(oracle, tmp_path_factory, clean_tables, n, defer_flips, pingpong, precision, planning, start):
    c, state, mask, want, want32, ref32 = _reference(oracle, tmp_path_factory, n, start)
    with Simulator(n, fuse=3, precision=precision, pingpong=pingpong, defer_flips=defer_flips, **SHAPES[n][0]) as sim:
        if planning == "choose":
            sim.choose_schedule(c)
        elif planning == "tune":
            sim.tune(c, 3, 0)
        predicted = sim.support_after(c, mask)
        support, got = _run(sim, c, state, mask)
        print(f"flush-rule n={n} defer={defer_flips} pingpong={pingpong} fp{precision} {planning} {start}: predicted={predicted:#x} "
              f"reported={support:#x} flips={sim.deferred_flip_stats()}")
        assert support == predicted, f"predicted {predicted:#x}, the flush left {support:#x}"
        if precision == 64:
            assert np.max(np.abs(got - want)) < TOL
        else:
            check_fp32(got, want32, ref32)
        replays = sim.plan_cache_stats()["replays"]
        support2, again = _run(sim, c, state, mask)
        assert sim.plan_cache_stats()["replays"] == replays + 1
        assert support2 == predicted
        assert np.array_equal(np.ascontiguousarray(again).view(got.real.dtype), np.ascontiguousarray(got).view(got.real.dtype))
