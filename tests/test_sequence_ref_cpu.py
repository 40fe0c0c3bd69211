"""tests/sequence_ref.py on the CPU: the model of every in-place kind against dense 2^n x 2^n operators built here (Kronecker products,
explicit permutation matrices — none of the *_ref modules' index arithmetic), the census of the pair table, the conditions of the
module's docstring on every program tests/test_gpu_sequences.py runs (same sizes, same seeds), the reach of the checker — what an
ordering mistake, a stale operand slot or a lost step does to the modelled result — and the two ring sizes against the engine's text."""
import functools
import math
import os
import re

import numpy as np
import pytest

import adjoint_ref
import diagonal_ref
import fp32_ref
import measure_ref
import sequence_ref as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 14                       # test_gpu_sequences.N
WALK_SEEDS = list(range(8))  # test_gpu_sequences.WALK_SEEDS
SMALL = [(n, seed) for n in (1, 2, 3) for seed in range(4)]
PRECISIONS = [64, 32]
REACH = 1e-2
REACH_SHARE = 0.95


# ---- dense operators, built here --------------------------------------------------------------------------------------------------------
_I2 = np.eye(2, dtype=np.complex128)
_LETTER = {"I": _I2, "X": np.array([[0, 1], [1, 0]], dtype=np.complex128), "Y": np.array([[0, -1j], [1j, 0]]), "Z": np.diag([1.0 + 0j, -1.0])}


def _kron(factors):
    """factors[q] acts on qubit q; qubit 0 is the least significant index bit, so it is the LAST Kronecker factor."""
    op = np.ones((1, 1), dtype=np.complex128)
    for f in reversed(factors):
        op = np.kron(op, f)
    return op


def _pauli(x, z, n):
    return _kron([_LETTER["IXZY"[(x >> q & 1) + 2 * (z >> q & 1)]] for q in range(n)])


def _projector(mask, n):
    """Onto the basis states whose bits under `mask` are all 1: a Kronecker product of |1><1| and identities."""
    one = np.diag([0.0 + 0j, 1.0])
    return _kron([one if mask >> q & 1 else _I2 for q in range(n)])


def _swap(a, b, n):
    """The permutation matrix that exchanges qubits a and b."""
    op = np.zeros((1 << n, 1 << n), dtype=np.complex128)
    for i in range(1 << n):
        ba, bb = i >> a & 1, i >> b & 1
        op[(i & ~(1 << a) & ~(1 << b)) | bb << a | ba << b, i] = 1
    return op


def _on_qubits(U, qubits, n):
    """U (bit j of its index is qubits[j]) on the register: U on the low k qubits by a Kronecker product, moved into place by swaps."""
    k = len(qubits)
    op = np.kron(np.eye(1 << (n - k)), np.asarray(U, dtype=np.complex128).reshape(1 << k, 1 << k))
    # a permutation matrix R with R |bits of low position j> = |bit at qubits[j]>: compose swaps that carry position j to qubits[j]
    where = list(range(n))  # where[p] = the position that currently holds what started at position p
    R = np.eye(1 << n, dtype=np.complex128)
    for j, q in enumerate(qubits):
        p = where[j]
        if p != q:
            R = _swap(p, q, n) @ R
            other = where.index(q)
            where[j], where[other] = q, p
    return R @ op @ R.T


def _controlled(op, controls, n):
    P = _projector(S._mask(controls), n)
    return (np.eye(1 << n) - P) + P @ op


def _dense(step, n, psi):
    """The step as a matrix on n qubits (`psi`: the state before it, for the steps that normalise)."""
    kind, op = step
    eye = np.eye(1 << n, dtype=np.complex128)
    if kind == "gates":
        out = eye
        for g in op["gates"]:
            if g[0] == "cx":
                m = _controlled(_kron([_LETTER["X"] if q == g[2] else _I2 for q in range(n)]), [g[1]], n)
            else:
                m = _kron([g[2] if q == g[1] else _I2 for q in range(n)])
            out = m @ out
        return out
    if kind in ("rotations", "rotations_mixed", "rotations_controlled"):
        out = eye
        for r in op["rotations"]:
            theta, c, x, z = (r[0], 0, r[1], r[2]) if len(r) == 3 else r
            rot = math.cos(theta / 2) * eye - 1j * math.sin(theta / 2) * _pauli(x, z, n)
            out = _controlled(rot, [q for q in range(n) if c >> q & 1], n) @ out
        return out
    if kind in ("matrix_main", "matrix_small"):
        return _controlled(_on_qubits(op["U"], op["targets"], n), op["controls"], n)
    if kind in ("permutation_main", "permutation_small"):
        k = len(op["targets"])
        U = np.zeros((1 << k, 1 << k))
        for j, to in enumerate(op["table"]):
            U[to, j] = 1
        return _controlled(_on_qubits(U, op["targets"], n), op["controls"], n)
    if kind in ("qft_single", "qft_moving"):
        k = len(op["qubits"])
        v = np.arange(1 << k)
        F = np.exp((-2j if op["inverse"] else 2j) * np.pi * np.outer(v, v) / (1 << k)) / math.sqrt(1 << k)
        return _on_qubits(F, op["qubits"], n)
    if kind == "diagonal_phase":
        d = sum(c * np.real(np.diagonal(_pauli(0, z, n))) for c, z in op["terms"])
        return np.diag(np.exp(-1j * op["gamma"] * d))
    if kind == "scale":
        return complex(*op["z"]) * eye
    if kind in ("postselect", "measure"):
        keep = eye
        for j, q in enumerate(op["qubits"]):
            bit = np.diag([0.0 + 0j, 1.0]) if op["outcome"] >> j & 1 else np.diag([1.0 + 0j, 0.0])
            keep = _kron([bit if p == q else _I2 for p in range(n)]) @ keep
        return keep / np.linalg.norm(keep @ psi)
    raise AssertionError(kind)


@pytest.mark.parametrize("n", [3, 5])
@pytest.mark.parametrize("kind", [k for k in S.IN_PLACE if k != "write_subrange"])
def test_the_model_of_an_in_place_kind_is_the_dense_operator(kind, n):
    for seed in range(4):
        bld = S.Builder(n, 64).add("write", 40 + seed)
        psi = bld.model.want.copy()
        bld.add(kind, 50 + seed)
        want = _dense(bld.program[-1], n, psi) @ psi
        assert np.max(np.abs(bld.model.want - want)) < 1e-12, (kind, n, seed)
        assert fp32_ref.rel_err(bld.model.ref32, want) < 1e-5, (kind, n, seed)


def test_the_swap_construction_places_a_matrix_where_the_definition_does():
    """_on_qubits against the definition, entry by entry, on scrambled targets."""
    rng = np.random.default_rng(3)
    n, qubits = 4, [2, 0, 3]
    U = rng.standard_normal((8, 8)) + 1j * rng.standard_normal((8, 8))
    op = _on_qubits(U, qubits, n)
    for col in range(1 << n):
        b = sum((col >> q & 1) << j for j, q in enumerate(qubits))
        for a in range(8):
            row = col
            for j, q in enumerate(qubits):
                row = (row & ~(1 << q)) | (a >> j & 1) << q
            assert op[row, col] == U[a, b]
    assert np.count_nonzero(op) == 64 * 2


def test_the_other_kinds_of_the_model():
    """write_subrange, the two-state kinds and housekeeping, which are no operators: against their definitions."""
    n = 4
    for precision in PRECISIONS:
        bld = S.Builder(n, precision).add("write", 9)
        psi = bld.model.want.copy()
        bld.add("write_subrange", 3)
        op = bld.program[-1][1]
        want = psi.copy()
        want[op["first"]:op["first"] + op["count"]] = S.subrange_values(op, n, precision)
        assert np.array_equal(bld.model.want, want) and np.array_equal(bld.model.ref32, want.astype(np.complex64))
        assert 1 <= op["count"] and op["first"] + op["count"] <= 1 << n
        bld.add("gradient", 4).add("inner", 5).add("copy_into", 6).add("lend_spare", 0).add("grid_cap", 1).add("withdraw_spare", 0)
        assert np.max(np.abs(bld.model.want - want)) < 1e-13  # none of them changes the state (a gradient: to rounding)
        assert np.array_equal(bld.model.partners[1][0], S._apply("permutation_main", bld.program[-4][1]["partner"]["after"], bld.model.want, np.complex128, n, precision))
        bld.add("combine_into", 7)
        op = bld.program[-1][1]
        partner = S.partner_states(op, n, precision)[0]
        assert abs(abs(complex(*op["d"])) ** 2 + abs(complex(*op["a"])) ** 2 - 1) < 1e-12
        assert np.max(np.abs(bld.model.want - (complex(*op["d"]) * want + complex(*op["a"]) * partner))) < 1e-13
        assert abs(np.linalg.norm(partner) - 1) < 1e-6
        bld.add("partial_write", 8)
        values, inside = S.partial_values(bld.program[-1][1], n, precision)
        assert np.array_equal(bld.model.want, values) and not values[~inside].any() and abs(np.linalg.norm(values) - 1) < 1e-6
        bld.add("reset", 0)
        assert bld.model.want[0] == 1 and not bld.model.want[1:].any()


# ---- every program the GPU file runs ----------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _programs(family, precision):
    """[(label, n, program, builder)]"""
    if family == "pair":
        return [(f"{a} -> {b}", N, p, bld) for a, b, p, bld in S.pair_programs(N, precision)]
    if family == "ring":
        return [(name, N, p, bld) for name, (p, bld) in S.ring_programs(N, precision).items()]
    if family == "tenants":
        return [(f"tenants {lent}", N) + S.tenant_program(N, precision, lent) for lent in S.TENANTS] + [("partners", N) + S.partner_program(N, precision)]
    if family == "walk":
        return [(f"walk {seed}", N) + S.random_program(N, 60, seed, precision) for seed in WALK_SEEDS]
    return [(f"walk {seed} on {n}", n) + S.random_program(n, 60, seed, precision) for n, seed in SMALL]


FAMILIES = ("pair", "ring", "tenants", "walk", "small")


def test_every_ordered_pair_appears_exactly_once():
    for precision in PRECISIONS:
        pairs = [tuple(label.split(" -> ")) for label, *_ in _programs("pair", precision)]
        assert len(pairs) == len(set(pairs)) == len(S.KINDS) ** 2
        assert set(pairs) == {(a, b) for a in S.KINDS for b in S.KINDS}
        for (a, b), (_, _, program, _) in zip(pairs, _programs("pair", precision)):
            assert [kind for kind, _ in program] == ["write", "gates", a, b, "gates"]
        assert [a for a, *_ in S.pair_programs(3, precision, first="norm2")] == ["norm2"] * len(S.KINDS)
    assert len(S.KINDS) == len(set(S.KINDS)) == 27 and not set(S.KINDS) & set(S.HOUSEKEEPING)
    assert set(S.STAGING) | set(S.COLLAPSES) | set(S.PARTNERED) | set(S.DRAWN) <= set(S.KINDS)


def _matrices(program):
    for kind, op in program:
        if "U" in op:
            yield op["U"]
        if "partner" in op:
            yield op["partner"]["matrix"]["U"]
        if kind == "gates":
            for g in op["gates"]:
                if g[0] == "u1":
                    yield g[2]


def _verify(label, n, precision, program):
    """The conditions of sequence_ref's docstring on one program, by a run of the model of this test's own."""
    model = S.Model(n, precision)
    collapses = 0
    for kind, op in program:
        if kind == "gates":
            assert 6 <= len(op["gates"]) <= 10, label
            assert any(g[0] == "u1" and np.array_equal(g[2], S.GATE_MATRICES["x"]) for g in op["gates"]), label
        if kind == "scale":
            assert 0.5 <= abs(complex(*op["z"])) <= 2.0, label
        if kind in S.COLLAPSES:
            collapses += 1
        if kind == "gradient":
            _, grad, _ = adjoint_ref.gradient(model.want, op["rotations"], op["terms"])
            assert np.linalg.norm(grad) >= S.GRADIENT_FLOOR * adjoint_ref.weight(op["terms"]) * float(np.vdot(model.want, model.want).real), label
        if kind == "postselect":
            assert 1 <= len(op["qubits"]) <= min(3, max(n - 1, 1)), label
            norm2 = float(np.vdot(model.want, model.want).real)
            weights = [measure_ref.weight(model.want, op["qubits"], o) for o in range(1 << len(op["qubits"]))]
            assert op["outcome"] == int(np.argmax(weights)) and weights[op["outcome"]] >= norm2 / 8, label
        if kind in S.DRAWN:
            assert sorted(op["qubits"]) == list(range(n - len(op["qubits"]), n)) and len(op["qubits"]) <= min(3, max(n - 1, 1)), label
            for u in op["draws"] if kind == "sample_shots" else [op["draw"]]:
                outcome, margin, agree = model.outcome_of(op, u)
                assert margin >= S.MARGIN and agree, (label, kind, u, margin)
                if kind == "measure":
                    assert outcome == op["outcome"], label
        model.apply((kind, op))
    for U in _matrices(program):
        U = np.asarray(U)
        assert np.max(np.abs(U.conj().T @ U - np.eye(U.shape[0]))) < 1e-12, label
    assert collapses <= S.MAX_COLLAPSES, label
    e_ref = fp32_ref.rel_err(model.ref32, model.want)
    assert e_ref <= fp32_ref.REF_CAP, (label, e_ref)
    assert np.isfinite(model.want).all() and np.linalg.norm(model.want) > 0, label
    return e_ref


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("family", FAMILIES)
def test_the_conditions_hold_for_every_program(family, precision):
    programs = _programs(family, precision)
    worst = max(_verify(label, n, precision, program) for label, n, program, _ in programs)
    drawn, redrawn = sum(b.drawn for *_, b in programs), sum(b.redrawn for *_, b in programs)
    idle = sum(b.idle for *_, b in programs)
    print(f"{family}, fp{precision}: {len(programs)} programs, {redrawn} of {drawn} steps redrawn for a condition ({redrawn / drawn:.2%}), {idle} for moving "
          f"the model by less than {S.EFFECT:g}, worst rel_err(ref32) {worst:.3e}")
    assert redrawn <= S.MAX_REDRAWN_SHARE * drawn
    if family in ("walk", "small"):
        for label, n, program, _ in programs:
            kinds = [kind for kind, _ in program]
            assert len(program) == 61 and kinds[0] == "write" and kinds[-1] == "gates", label
            assert all(kind not in S.DEFINERS and not (n == 1 and kind in S.COLLAPSES + ("write_subrange",)) for kind in kinds[S.EARLY + 1:]), label
            assert kinds.count("measure") <= 1, label
        seen = {kind for _, _, program, _ in programs for kind, _ in program}
        assert set(S.KINDS) | set(S.HOUSEKEEPING) <= seen, sorted((set(S.KINDS) | set(S.HOUSEKEEPING)) - seen)


def test_the_operands_take_the_path_their_kind_is_named_for():
    """Host only: at n = 14 the main kinds take the main kernels and the small kinds the plain ones, a moving transform has at least
    three sweeps, two of them out of place, a single one is one sweep in place."""
    from gpu_quantum_simulator_amd import plans
    seen = set()
    for precision in PRECISIONS:
        for family in ("pair", "ring", "tenants", "walk"):
            for label, n, program, _ in _programs(family, precision):
                steps = list(program) + [("matrix_main", op["partner"]["matrix"]) for _, op in program if "partner" in op]
                steps += [("permutation_main", op["partner"]["after"]) for _, op in program if "partner" in op]
                steps += [("qft_moving", op["partner"]["qft"]) for _, op in program if "partner" in op]
                for kind, op in steps:
                    if kind in ("matrix_main", "matrix_small"):
                        t, c = op["targets"], op["controls"]
                        path = plans.ok(plans.apply_matrix_plan(t, c, n, precision))["path"]
                        assert (path, len(t), len(c)) == ((1, 5, 1) if kind == "matrix_main" else (0, 2, 9)), (label, kind)
                    elif kind in ("permutation_main", "permutation_small"):
                        t, c = op["targets"], op["controls"]
                        path = plans.ok(plans.apply_permutation_plan(t, c, n, precision))["path"]
                        assert (path, len(t)) == ((1, 10) if kind == "permutation_main" else (0, 3)), (label, kind)
                    elif kind in ("qft_single", "qft_moving"):
                        plan = plans.ok(plans.apply_qft_plan(op["qubits"], n, precision, op["max_digit_bits"]))
                        passes, moving = plan["passes"], sum(plan["out_of_place"])
                        assert (passes, moving) == ((1, 0) if kind == "qft_single" else (3, 2)), (label, kind, passes, moving)
                    else:
                        continue
                    seen.add(kind)
    assert seen == {"matrix_main", "matrix_small", "permutation_main", "permutation_small", "qft_single", "qft_moving"}


# ---- the reach of the checker -------------------------------------------------------------------------------------------------------------
CHANGES = S.IN_PLACE + ("combine_into",)                      # the kinds that change the state


def _commute(a, b, n, precision):
    """Whether two steps commute as maps: applied in both orders to a random vector that has nothing to do with the program (so that
    a subspace the program's state has left empty does not hide an operator)."""
    probe = S.start_state(n, 4242, precision)
    ab = S._apply(b[0], b[1], S._apply(a[0], a[1], probe, np.complex128, n, precision), np.complex128, n, precision)
    ba = S._apply(a[0], a[1], S._apply(b[0], b[1], probe, np.complex128, n, precision), np.complex128, n, precision)
    return fp32_ref.rel_err(ab, ba) < 1e-9


def _tail(n, precision, states, program, at, mutated_tail):
    """The final complex128 state of program[:at] + mutated_tail, from the model's state before step `at`."""
    psi = states[at]
    for kind, op in mutated_tail:
        psi = S._apply(kind, op, psi, np.complex128, n, precision)
    return psi


def _reach(label, n, precision, program, stale=False):
    """(trials, hits): every mutation of the docstring at every position where it applies; a hit changes the modelled final state by
    at least REACH relative (a state that is no longer finite counts: nothing passes with it)."""
    states = [S.Model(n, precision).want]
    model = S.Model(n, precision)
    for step in program:
        model.apply(step)
        states.append(model.want)
    final = states[-1]
    last_definer = max(i for i, (kind, _) in enumerate(program) if kind in S.DEFINERS or (n == 1 and kind in S.COLLAPSES + ("write_subrange",)))
    trials = hits = 0

    def tried(at, tail):
        nonlocal trials, hits
        try:
            got = _tail(n, precision, states, program, at, tail)
            err = fp32_ref.rel_err(got, final) if np.isfinite(got).all() else float("inf")
        except ZeroDivisionError:  # the outcome a later postselect takes has probability zero now: the device refuses the call
            err = float("inf")
        trials += 1
        hits += err >= REACH
        return err

    for i in range(last_definer + 1, len(program)):
        kind, op = program[i]
        if kind not in CHANGES:
            continue
        tried(i, program[i + 1:])                                                        # the step is lost
        if i + 1 < len(program) and program[i + 1][0] in CHANGES:                        # two adjacent steps change places
            a, b = program[i], program[i + 1]
            if not _commute(a, b, n, precision):
                tried(i, [b, a] + program[i + 2:])
        if stale and i - S.STAGING_SLOTS > last_definer and program[i - S.STAGING_SLOTS][0] == kind:  # the slot still holds the operand of 16 calls ago
            tried(i, [(kind, program[i - S.STAGING_SLOTS][1])] + program[i + 1:])
    return trials, hits


def test_a_mistake_in_the_order_or_a_stale_operand_shows_in_the_model():
    precision = 64  # (what a mutation does to the model does not depend on the rounding of the start state)
    rows = []
    for name, _, program, _ in _programs("ring", precision):
        if not name.startswith("tile_ops"):
            rows.append((f"ring {name}",) + _reach(name, N, precision, program, stale=True))
    for family in ("walk", "small"):
        for label, n, program, _ in _programs(family, precision):
            rows.append((label,) + _reach(label, n, precision, program))
    for label, trials, hits in rows:
        print(f"reach of {label}: {hits} of {trials} mutations change the final state by >= {REACH:g}")
        assert trials >= 5 and hits >= REACH_SHARE * trials, (label, hits, trials)


def test_the_mutations_are_what_they_say():
    """Dropping a step that is the identity changes nothing; a swap of two steps on disjoint qubits is not tried."""
    n = 4
    bld = S.Builder(n, 64).add("write", 1).add("qft_single", 2).add("permutation_main", 3)
    program = bld.program + [("scale", dict(z=(1.0, 0.0)))]
    trials, hits = _reach("identity", n, 64, program)
    assert (trials, hits) == (4, 3)  # three drops, one of them the identity, and one swap (scale commutes with everything: not tried)


# ---- the two ring sizes -------------------------------------------------------------------------------------------------------------------
def test_the_ring_constants_are_the_engine_s():
    csrc = os.path.join(ROOT, "gpu_quantum_simulator_amd", "csrc")
    with open(os.path.join(csrc, "matrix.cpp")) as f:
        slots = re.findall(r"constexpr\s+int\s+kSlots\s*=\s*(\d+)\s*;", f.read())
    with open(os.path.join(csrc, "engine.cpp")) as f:
        cap = re.findall(r"constexpr\s+size_t\s+kOpsCap\s*=\s*(\d+)\s*;", f.read())
    assert slots == [str(S.STAGING_SLOTS)] == ["16"]
    assert cap == [str(S.OPS_CAP)] == ["512"]
    assert S.RING_CALLS == 3 * S.STAGING_SLOTS + 5 and S.TWO_STATES_FIRST_HALF > S.STAGING_SLOTS
