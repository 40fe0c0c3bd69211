"""The TileOp record contract, checked on the CPU: every record csrc/tile_op.cpp encodes for the suite's random circuits and for
the directed circuits of tile_forms_ref.py is decoded and run by the independent model in tile_record_ref.py.

What this pins that no amplitude comparison on the device can: the barrier bit.  A record with K > 3 and no barrier bit lets
the waves of different parts read and write in any order; test 5 runs its parts in place in five orders (and with all reads
first) and demands bit-identical results — a record that needs the barrier and does not ask for it fails here, every time,
where on the device it would mostly pass.

Bound: the model multiplies the record's own coefficients in fp64; a row has at most four terms, amplitudes and coefficients
of magnitude <= 1, so 1e-13 absolute per amplitude (four products and three sums at 2^-53 relative each stay below 1e-15).
fp32 records are compared with the dense matrix of the float32-rounded coefficients under the same bound.

Cost: every distinct record is run on eight groups of a tile (the first, the last and six seeded ones: the coefficients and
offsets are the same for every group), and the first record of every distinct (K, lane nibbles) — which alone
decide how the groups are enumerated — on the whole tile.
"""
import hashlib

import numpy as np
import pytest

from gpu_quantum_simulator_amd import Circuit, circuits
import fp32_ref
import tile_forms_ref as F
import tile_record_ref as R

BOUND = 1e-13
SEEDS = (0, 3, 11)
TILE_BITS = range(8, 14)


def _low_bits(B):
    """Two values of tile_low_bits per tile size, the ends of the range the geometry sweeps draw from."""
    return (max(2, B - 10), min(6, B - 2))


def _random_specs():
    return [c[:4] for c in F.CACHE_BLOCKED_CIRCUITS] + [c for c, _ in fp32_ref.RANDOM_CIRCUITS]


class Collected:
    def __init__(self):
        self.unique = {}     # key -> (record dict, f32)
        self.total = 0
        self.directed = {}   # (B, f32) -> set of forms, from the directed circuits only

    def add(self, c, B, L, directed):
        for f32 in (False, True):
            for seed in SEEDS:
                for r in c.tile_records(tile_bits=B, tile_low_bits=L, f32=f32, order_seed=seed):
                    self.total += 1
                    geom = (r["tile_bits"], r["low_bits"], r["high"])
                    bits = tuple(R.local_bit(geom, q) for q in r["qubits"])
                    key = (geom[0], f32, bits, hashlib.sha1(r["record"]).digest(), hashlib.sha1(r["matrix"].tobytes()).digest())
                    self.unique.setdefault(key, (r, f32))
                    if directed:
                        h = R.header(r["record"])
                        if h["kind"] == R.TOP_PART:
                            self.directed.setdefault((r["tile_bits"], f32), set()).add(F.form_of(h))


@pytest.fixture(scope="module")
def collected():
    col = Collected()
    for spec in _random_specs():
        c = Circuit.from_text(circuits.qasm_text(spec[0], circuits.random_gates(*spec)))
        for B in TILE_BITS:
            for L in _low_bits(B):
                col.add(c, B, L, False)
    for B in TILE_BITS:
        for L in _low_bits(B):
            for _name, n, gates, _form in F.directed_cases(B, L):
                col.add(F.circuit_of(n, gates), B, L, True)
    return col


_TILES = {}


def _tile(B):
    if B not in _TILES:
        rng = np.random.default_rng(4000 + B)
        t = rng.uniform(-1, 1, 1 << B) + 1j * rng.uniform(-1, 1, 1 << B)
        _TILES[B] = t / np.sqrt(2)  # |amplitude| <= 1
    return _TILES[B]


def _unswizzle(byte, f32):
    """Logical slot of an LDS byte offset (the swizzle only touches the unit bits, so it is its own inverse)."""
    v = np.asarray(byte, dtype=np.int64) >> R.slot_shift(f32)
    return v ^ R.lds_sw_fold(v >> R.sw_low(f32), f32)


def _row_index(slot, bits):
    """Row / column index of the block's matrix for a logical slot: bits = tile-local bit of each qubit, most significant first."""
    idx = np.zeros_like(slot)
    for b in bits:
        idx = (idx << 1) | ((slot >> b) & 1)
    return idx


def _check_part(r, f32, full_tile):
    rec, M = r["record"], r["matrix"]
    h = R.header(rec)
    B, K, T, nsel = r["tile_bits"], h["nq"], h["terms"], h["nsel"]
    geom = (B, r["low_bits"], r["high"])
    k = len(r["qubits"])
    bits = [R.local_bit(geom, q) for q in r["qubits"]]
    S = R.slot_shift(f32)
    banks = 1 << nsel
    nparts = 1 << (K - 3)
    OFF, ROWOFF, CF = R.tables(rec, f32)
    dec = (h, (OFF, ROWOFF, CF))
    assert nsel == len(r["selectors"]) and h["selbit"][:nsel] == r["selectors"]
    assert 3 <= K <= 6 and K >= k and T in (1, 2, 4)
    # 2. lane nibbles: the first B - K a permutation of the tile bits the block does not use, every later one 15
    free = h["nibbles"][:B - K]
    assert len(set(free)) == B - K and all(0 <= b < B for b in free), free
    assert all(x == R.LANE_NONE for x in h["nibbles"][B - K:])
    used = sorted(set(range(B)) - set(free))
    assert len(used) == K and set(bits) <= set(used), (used, bits)
    used_mask = sum(1 << b for b in used)
    # 3. offsets: slot-aligned, inside the tile, on the block's own bits; written slots distinct; unwritten = identity rows
    live = OFF[:banks, :nparts] != R.SKIP_CLASS   # [bank, part, 8]; a skipped class has the marker at its first operand
    skipped_class = ~live[:, :, ::T]              # [bank, part, classes]
    skipped_pos = np.repeat(skipped_class, T, axis=2)
    assert np.array_equal(ROWOFF[:banks, :nparts] == R.SKIP_CLASS, skipped_pos), "rowoff markers go with the class's off marker"
    any_skips = bool(skipped_class.any())
    WS = _unswizzle(np.where(skipped_pos, 0, ROWOFF[:banks, :nparts]), f32)  # logical slots written / read; 0 at skipped positions
    RS = _unswizzle(np.where(np.repeat(skipped_class, T, axis=2), 0, OFF[:banks, :nparts]), f32)
    qmask = sum(1 << b for b in bits)
    codes = np.zeros(1 << K, dtype=np.int64)
    for i, b in enumerate(used):
        codes |= ((np.arange(1 << K) >> i) & 1) << b
    keep = ~skipped_pos                                                       # [bank, part, 8]
    for x in (ROWOFF[:banks, :nparts][keep], OFF[:banks, :nparts][keep]):
        assert np.all(x % (1 << S) == 0) and np.all(x < (1 << (B + S))), "slot-aligned and inside the tile"
    assert np.all(WS & ~used_mask == 0) and np.all(RS & ~used_mask == 0), "offsets stay on the block's bits"
    # closed <=> every part of every bank writes exactly the slots it reads (a skipped class reads and writes nothing)
    sw, sr = np.sort(np.where(keep, WS, -1), axis=2), np.sort(np.where(keep, RS, -1), axis=2)
    closed = bool(np.array_equal(sw, sr))
    # the coefficient of position pos, entry j is the matrix entry (row written, column read) — exactly
    P = np.arange(R.PART_ROWS)[:, None]
    J = (P // T) * T + np.arange(T)[None, :]
    U_all = np.stack([R.dense_bank(M, k, v) for v in range(banks)])
    Uc = R.round32(U_all) if f32 else U_all
    ri, ci = _row_index(WS, bits), _row_index(RS, bits)                      # [bank, part, 8]
    V = np.arange(banks)[:, None, None, None]
    want = np.where((WS & ~qmask)[:, :, P] == (RS & ~qmask)[:, :, J], Uc[V, ri[:, :, P], ci[:, :, J]], 0.0)  # a padding copy reads its own copy only
    got = CF[:banks, :nparts, :R.PART_ROWS * T].reshape(banks, nparts, R.PART_ROWS, T)
    assert np.array_equal(got[keep], want[keep]), "coefficients are the matrix entries at (row written, column read)"
    eye = np.eye(1 << k)
    code_row = _row_index(codes, bits)
    for v in range(banks):
        U = U_all[v]
        written = WS[v][keep[v]]
        assert len(np.unique(written)) == written.size, "two positions write one slot"
        ident_row = np.all(U == eye, axis=1)
        unwritten = ~np.isin(codes, written)
        assert not np.any(unwritten & ~ident_row[code_row]), "a row that is not an identity row is not written"
        # ... and exactly the identity rows are left out, class by class (a class is skipped when ALL its T rows are identity rows;
        # an identity row that fills up a class of other rows is written like them, with coefficient 1)
        class_ident = ident_row[ri[v]].reshape(nparts, R.PART_ROWS // T, T).all(axis=2)
        assert not np.any(class_ident & ~skipped_class[v]), "a class of identity rows only is written"
        # 1. ident bit v <=> bank v of the reported matrix is exactly the identity
        assert bool(h["ident"] >> v & 1) == bool(ident_row.all()), v
    assert h["ident"] >> banks == 0
    # 4. / 5. semantics
    tile = _tile(B)
    gcount = 1 << (B - K)
    groups = None
    if not full_tile:
        rng = np.random.default_rng(B * 64 + K)
        groups = np.unique(np.concatenate([[0, gcount - 1], rng.integers(0, gcount, 6)]))
        gslots = np.zeros_like(groups)
        for a in range(B - K):
            gslots |= ((groups >> a) & 1) << free[a]
        mark = np.zeros(1 << B, dtype=bool)
        mark[gslots] = True
        touched = mark[np.arange(1 << B) & ~used_mask]
    for v in range(banks):
        U = R.dense_bank(M, k, v)
        want = R.apply_dense(R.round32(U) if f32 else U, geom, r["qubits"], tile)
        if groups is not None:
            want = np.where(touched, want, tile)
        if h["info_barrier"] or K == 3:
            got = R.apply(rec, geom, tile, v, "barrier", f32, groups, dec)
            assert np.max(np.abs(got - want)) <= BOUND, (v, np.max(np.abs(got - want)))
        else:  # hazard freedom: the parts in place, one after the other, in any order — and with every read first
            rng = np.random.default_rng(nparts)
            orders = [list(range(nparts)), list(range(nparts))[::-1]] + [list(rng.permutation(nparts)) for _ in range(3)]
            results = [R.apply(rec, geom, tile, v, o, f32, groups, dec) for o in orders] + [R.apply(rec, geom, tile, v, "barrier", f32, groups, dec)]
            for o, res in zip(orders + ["reads first"], results):
                assert np.array_equal(res, results[0]), f"part order {o} changes the result: the record needs the barrier it does not ask for"
            assert np.max(np.abs(results[0] - want)) <= BOUND, (v, np.max(np.abs(results[0] - want)))
    # 1. header consistency (after the runs: a record that claims to be closed and is not fails the hazard runs above first)
    assert h["info_log2T"] == {1: 0, 2: 1, 4: 2}[T]
    assert h["info_skips"] == bool(h["flags"] & R.FLAG_SKIPS) == any_skips
    assert bool(h["flags"] & R.FLAG_CLOSED) == closed, "closed <=> every part of every bank writes exactly the slots it reads"
    assert h["info_barrier"] == (K > 3 and not closed)
    assert h["info"] & ~(6 | R.INFO_SKIPS | R.INFO_BARRIER) == 0
    # 6. fp32 records: the pairs (ur, ui), (-ui, ur), exactly
    if f32:
        body = np.frombuffer(rec, dtype=np.uint8)[128:].reshape(R.MAX_BANKS, R.MAX_PARTS, R.REC_BYTES)
        f = np.ascontiguousarray(body[:banks, :nparts, 64:]).view("<f4").reshape(banks, nparts, 32, 4)[:, :, :8 * T]
        assert np.array_equal(f[..., 2], -f[..., 1]) and np.array_equal(f[..., 3], f[..., 0]), "fp32 second pair is (-ui, ur)"
    return h


def _check_scale(r, f32):
    h = R.header(r["record"])
    assert h["nq"] == 0 and r["qubits"] == () and h["nsel"] == len(r["selectors"]) >= 1
    for v in range(1 << h["nsel"]):
        z = r["matrix"][v, v]
        want = complex(np.complex64(z)) if f32 else complex(z)
        assert R.scale(r["record"], v, f32) == want  # fp32: exactly the two floats
        assert bool(h["ident"] >> v & 1) == (z == 1.0)


def test_every_record_of_the_suite_and_directed_circuits(collected):
    """Assertions 1-6 on every distinct record (module docstring); the counts are printed for the record."""
    kinds, patterns, forms = {}, set(), {}
    for (B, f32, bits, _d, _m), (r, _) in collected.unique.items():
        h = R.header(r["record"])
        kinds[h["kind"]] = kinds.get(h["kind"], 0) + 1
        if h["kind"] == R.TOP_SCALE:
            _check_scale(r, f32)
            continue
        assert h["kind"] == R.TOP_PART, "tiles of 2^3 amplitudes and more know the part form only"
        pattern = (B, f32, r["record"][1], r["record"][8:13])  # the group enumeration hangs on K and the lane nibbles alone
        _check_part(r, f32, full_tile=pattern not in patterns)
        patterns.add(pattern)
        forms[F.form_of(h)[:4]] = forms.get(F.form_of(h)[:4], 0) + 1
    print(f"\ntile records: {collected.total} encoded, {len(collected.unique)} distinct, {len(patterns)} patterns run on a whole tile; kinds {kinds}")
    for form in sorted(forms):
        print("  (K, T, skips, barrier) =", form, forms[form])
    assert kinds.get(R.TOP_SCALE, 0) > 0, "no tile-uniform factor among the records"


def test_directed_circuits_yield_their_forms():
    """Each directed case contains the form it is named after, at every tile size and both low-bit choices."""
    for B in TILE_BITS:
        for L in _low_bits(B):
            for name, n, gates, form in F.directed_cases(B, L):
                assert len(gates) <= 12, (name, len(gates))
                got = [F.form_of(R.header(r["record"])) for r in F.circuit_of(n, gates).tile_records(tile_bits=B, tile_low_bits=L)
                       if R.header(r["record"])["kind"] == R.TOP_PART]
                assert form in got, (B, L, name, form, got)


def test_coverage_of_the_directed_circuits(collected):
    """The union of the directed circuits' records holds every cell of the table (tile_forms_ref.required_cells), per precision
    and tile size.  No cell of it is unreachable: every (T, skips, barrier) at K > 3 takes three gates.  The one form that cannot
    exist, the barrier bit at K = 3 (one part per group: no other part's writes to wait for), is asserted absent."""
    for B in TILE_BITS:
        cells, nsels = F.required_cells(B)
        for f32 in (False, True):
            forms = collected.directed[B, f32]
            for cell in cells:
                assert F.covers(forms, cell), (B, f32, cell, sorted(forms))
            for ns in nsels:
                assert any(f[4] == ns for f in forms), (B, f32, "nsel", ns)
            assert not any(f[0] == 3 and f[3] for f in forms), "barrier bit at K = 3"


def test_tiny_tiles():
    """Registers of fewer than three qubits (B < 3) keep the pair / quad forms: TOP_G1, TOP_DIAG1 and TOP_G2, interpreted as the
    header comment describes them.  n = 1 is always ONE fused 2x2, which runs as a single-gate kernel: no tile pass, no record.
    At n = 2 a lone gate is a single-gate kernel too; blocks on both qubits merge into one TOP_G2; and two clusters on the SAME
    qubit that a cancelled pair of CXs kept apart merge inside the tile pass into a block on that one qubit — TOP_G1 when
    the product is dense, TOP_DIAG1 when it is diagonal, with off[0] = 1 exactly when d0 of the reported matrix is exactly 1
    (decided from the double: an fp32 record of d0 = 1 - 2^-53 holds 1.0f and off[0] = 0).  Every form under both precisions,
    on both qubits and under tile orders that swap the two bits."""
    rng = np.random.default_rng(52)
    X, Z = np.array([[0, 1], [1, 0]], dtype=np.complex128), np.diag([1, -1]).astype(np.complex128)
    T_GATE, RZ = np.diag([1, np.exp(0.25j * np.pi)]), np.diag(np.exp([-0.3j, 0.3j]))
    for gates in ([("u1", 0, F.random_unitary(2, rng))], [("u1", 0, T_GATE)], [("u1", 0, RZ), ("u1", 0, F.random_unitary(2, rng))]):
        assert F.circuit_of(1, gates).tile_records() == []
    assert F.circuit_of(2, [("u1", 1, T_GATE)]).tile_records() == []  # a lone gate: a single-gate kernel
    cases = []  # (gates, kind expected, qubits expected)
    for gates in ([("u2", 1, 0, F.random_unitary(4, rng))], [("u1", 0, T_GATE), ("u1", 1, RZ)], [("u1", 1, F.random_unitary(2, rng)), ("u1", 0, T_GATE)],
                  [("cx", 1, 0), ("u1", 0, F.random_unitary(2, rng))], [("cx", 0, 1), ("u1", 1, RZ)]):
        cases.append((gates, R.TOP_G2, (1, 0)))
    for q in (0, 1):
        def split(first, second, q=q):  # two clusters on q: the CX pair between them cancels and is dropped
            return [("u1", q, first), ("cx", q, 1 - q), ("cx", q, 1 - q), ("u1", q, second)]
        cases.append((split(X, F.random_unitary(2, rng)), R.TOP_G1, (q,)))
        cases.append((split(F._H, F.random_unitary(2, rng)), R.TOP_G1, (q,)))
        cases.append((split(X, np.diag([1, np.exp(0.7j)]) @ X), R.TOP_DIAG1, (q,)))           # d0 == 1 exactly: off[0] = 1
        cases.append((split(F._H, Z @ F._H), R.TOP_DIAG1, (q,)))                                # d0 = 1 - 2^-53: off[0] = 0
        cases.append((split(X, np.diag(np.exp([0.4j, 1.1j])) @ X), R.TOP_DIAG1, (q,)))          # no one: off[0] = 0
    tile = _tile(2)
    seen, swapped = set(), set()
    for gates, kind, qubits in cases:
        c = F.circuit_of(2, gates)
        for L in (0, 1, 2):
            for f32 in (False, True):
                for seed in SEEDS + (1, 2):
                    recs = c.tile_records(tile_bits=12, tile_low_bits=L, f32=f32, order_seed=seed)
                    assert len(recs) == 1
                    r = recs[0]
                    h = R.header(r["record"])
                    geom = (r["tile_bits"], r["low_bits"], r["high"])
                    assert geom[0] == 2 and h["kind"] == kind and h["nsel"] == 0 and h["nq"] == len(qubits) and r["qubits"] == qubits
                    bits = [R.local_bit(geom, q) for q in r["qubits"]]
                    assert list(h["b"][:len(bits)]) == sorted(bits)  # the block's tile-local bits, ascending
                    if bits != list(r["qubits"]):
                        swapped.add(kind)                            # the tile order moved the block's qubits
                    M = r["matrix"]
                    U = R.round32(M) if f32 else M
                    got = R.apply_small(r["record"], tile, f32)
                    assert np.max(np.abs(got - R.apply_dense(U, geom, r["qubits"], tile))) <= BOUND
                    cells = {R.TOP_G1: 4, R.TOP_DIAG1: 2, R.TOP_G2: 16}[kind]
                    if kind == R.TOP_G1:
                        want = U.reshape(4)                          # row-major
                    elif kind == R.TOP_DIAG1:
                        want = np.array([U[0, 0], U[1, 1]])
                        off, _ = R.offsets(r["record"], 0, 0)
                        assert off[0] == (1 if M[0, 0] == 1.0 else 0), "off[0] = 1 exactly when d0 of the (double) matrix is 1"
                        assert M[0, 1] == 0 and M[1, 0] == 0
                        seen.add(("d0 == 1", bool(M[0, 0] == 1.0), bool(np.complex64(M[0, 0]) == 1.0)))
                    else:  # index bit 0 is b[0], bit 1 is b[1]: the qubits' roles swap with the tile order
                        want = (U if bits == [1, 0] else U.reshape(2, 2, 2, 2).transpose(1, 0, 3, 2)).reshape(16)
                    assert np.array_equal(R.coefs(r["record"], 0, 0, f32)[:cells], want)
                    if f32:
                        raw = R.coef_raw(r["record"], 0, 0, True)[:cells]
                        assert np.array_equal(raw[:, 2], -raw[:, 1]) and np.array_equal(raw[:, 3], raw[:, 0])
                    seen.add((kind, f32))
    assert {(k, f) for k in (R.TOP_G1, R.TOP_DIAG1, R.TOP_G2) for f in (False, True)} <= seen
    # d0 exactly 1; d0 that only rounds to 1 in fp32 (off[0] stays 0); d0 nowhere near
    assert {("d0 == 1", True, True), ("d0 == 1", False, True), ("d0 == 1", False, False)} <= seen, seen
    assert swapped == {R.TOP_G1, R.TOP_DIAG1, R.TOP_G2}, f"forms never seen under a tile order that moves their bits: {swapped}"
    spec = (2, 60, 42, "all")  # ... and whatever a random circuit yields
    for r in Circuit.from_text(circuits.qasm_text(2, circuits.random_gates(*spec))).tile_records():
        assert np.max(np.abs(R.apply_small(r["record"], tile, False) - R.apply_dense(r["matrix"], (2, r["low_bits"], r["high"]), r["qubits"], tile))) <= BOUND


def test_swizzle_is_linear_and_a_bijection():
    """What lets the host pre-swizzle offsets: sw(a ^ b) = sw(a) ^ sw(b), and every slot has its own address, both slot sizes."""
    rng = np.random.default_rng(9)
    for f32 in (False, True):
        every = np.arange(1 << 13, dtype=np.int64)
        addr = R.slot_byte(every, f32)
        assert len(np.unique(addr)) == every.size and addr.max() < (1 << 13) << R.slot_shift(f32)
        a, b = rng.integers(0, 1 << 13, 4096), rng.integers(0, 1 << 13, 4096)
        assert np.array_equal(R.slot_byte(a ^ b, f32), R.slot_byte(a, f32) ^ R.slot_byte(b, f32))


def test_directed_circuits_stay_under_the_fp32_reference_cap():
    """The fp32 criterion the device half holds them to (fp32_ref.check_fp32) asks that a circuit's own complex64 replay stays
    under REF_CAP: checked here, on the start states the device half writes."""
    worst = 0.0
    for B in TILE_BITS:
        for name, (_n, _gates, _form, _s0, _want64, want32, ref32) in F.references(B).items():
            worst = max(worst, fp32_ref.rel_err(ref32, want32))
            assert fp32_ref.rel_err(ref32, want32) <= fp32_ref.REF_CAP, (B, name)
    print(f"\ndirected circuits: worst rel_err(ref32) = {worst:.3e} (cap {fp32_ref.REF_CAP:g})")
