"""Byte accounting of tile passes over a partially written state (host only).

A run that starts from a reset knows where the state is zero (its support).  A tile pass then visits only the tiles inside
support | tile qubits, WRITES all of those, and READS of each only the slots inside the support it finds: with z tile qubits
new to the support that is 2^-z of what it writes, and nothing at all for the pass that generates the basis state.  The
plan's per-pass bytes are restated here from `Circuit.passes()` (tile_mask per pass) and the running support alone.
"""
import pytest

from gpu_quantum_simulator_amd import Circuit, circuits


def _restated(n, passes, support):
    """[(visited, read_share)] per pass from the tile masks and the running support."""
    full = (1 << n) - 1
    out = []
    for p in passes:
        tmask = p["tile_mask"] & full
        if p["kernel"] != "tile" or support & full == full:
            out.append((1.0, 1.0))
            support = full
            continue
        after = (support | tmask) & full
        visited = 2.0 ** -(n - bin(after).count("1"))
        z = bin(tmask & ~support & full).count("1")
        read = 0.0 if support & full == 0 else visited * 2.0 ** -z
        out.append((visited, read))
        support = after
    return out


@pytest.mark.parametrize("n,tile_bits,seed", [(14, 10, 3), (16, 10, 5), (18, 12, 7), (20, 12, 11), (24, 12, 13), (30, 12, 20240147)])
def test_plan_bytes_follow_the_support(n, tile_bits, seed):
    c = Circuit.from_gates(n, circuits.random_gates(n, 400, seed, "all"))
    S = 16.0 * (1 << n)
    passes = c.passes(fuse=3, tile_bits=tile_bits, tile_low_bits=3)
    want = _restated(n, passes, 0)
    partial = 0
    for p, (visited, read) in zip(passes, want):
        scale = 1.0 if p["kernel"] == "tile" else p["bytes"] / (2 * S)  # single-gate kernels: whatever the scheduler charges
        assert p["bytes"] == pytest.approx(S * (visited + read) * scale, rel=1e-12), (p, visited, read)
        if p["kernel"] == "tile":
            assert p["visited"] == pytest.approx(visited, rel=1e-12)
            partial += read < visited
    assert partial >= 2  # the generating pass and at least one pass that admits qubits to a support
    assert passes[0]["bytes"] == pytest.approx(S * want[0][0], rel=1e-12)  # the generating pass only writes
    total = c.plan(fuse=3, tile_bits=tile_bits, tile_low_bits=3)["algorithmic_bytes"]
    assert total == pytest.approx(sum(p["bytes"] for p in passes), rel=1e-12)
    # strictly less than with reads charged like writes
    assert total < sum(2 * S * v if p["kernel"] == "tile" else p["bytes"] for p, (v, _) in zip(passes, want))


@pytest.mark.parametrize("n,tile_bits", [(16, 10), (20, 12)])
def test_a_full_support_sweeps_everything(n, tile_bits):
    c = Circuit.from_gates(n, circuits.random_gates(n, 300, 17, "all"))
    S = 16.0 * (1 << n)
    full = (1 << n) - 1
    passes = c.passes(fuse=3, tile_bits=tile_bits, tile_low_bits=3, initial_support=full)
    assert passes
    for p in passes:
        if p["kernel"] == "tile":
            assert p["bytes"] == 2 * S and p["visited"] == 1.0
    assert c.plan(fuse=3, tile_bits=tile_bits, tile_low_bits=3, initial_support=full)["algorithmic_bytes"] == sum(p["bytes"] for p in passes)


def test_a_given_partial_support():
    """A support that is neither empty nor full (qsim_set_support): the first pass reads the slots inside it."""
    n = 18
    c = Circuit.from_gates(n, circuits.random_gates(n, 300, 23, "all"))
    S = 16.0 * (1 << n)
    support = 0b111111  # qubits 0..5 may be 1
    passes = c.passes(fuse=3, tile_bits=10, tile_low_bits=3, initial_support=support)
    want = _restated(n, passes, support)
    assert want[0][1] > 0.0
    for p, (visited, read) in zip(passes, want):
        if p["kernel"] == "tile":
            assert p["bytes"] == pytest.approx(S * (visited + read), rel=1e-12)
