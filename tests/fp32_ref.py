"""The tests' own reference and checker for fp32 states: a numpy replay of a gate list in a chosen precision, and the error
criterion the fp32 GPU tests hold the engine to (tests/test_fp32_ref_cpu.py pins both on the CPU).

Criterion.  `want` is the fp64 truth (oracle run, golden file, or replay(..., dtype=np.complex128)), `ref32` the replay of the
same gates in complex64.  The engine passes when
    rel_err(got, want) <= C * max(rel_err(ref32, want), FLOOR),      rel_err(x, w) = ||x - w||_2 / ||w||_2.
C = 8: both sides round once per multiply-add.  A fused block of a tile pass keeps at most 4 entries per row and a per-gate
kernel 2 (1q) or 4 (2q), so one block application rounds at most about twice as often per amplitude as one 1q
gate of the replay; the engine applies no more blocks than the replay applies gates (as many at fusion level 0, fewer above
it; a cx folded into a block adds no rounding, its entries are 0 and 1); and it rounds each fused coefficient to fp32 once,
where the replay rounds every gate's matrix.  A correct kernel lands within about 2x of ref32; C = 8 leaves 4x for
random-walk scatter.  An engine that rounded its coefficients to half precision sits 2000-8000x above ref32.
FLOOR = 2^-24 is a condition, not a measurement: it keeps the bound above zero for circuits whose coefficients are exact in
fp32.  REF_CAP is a condition on the circuits themselves: a pathological circuit may not inflate its own bound.

A start state the caller writes is rounded to fp32 by the write; `want` and `ref32` then both start from that rounded
state (s.astype(np.complex64)), so the write's own rounding is not charged to the kernels.
"""
import numpy as np

C = 8.0
FLOOR = 2.0 ** -24
REF_CAP = 1e-5

# ---- the circuits of the fp32 GPU tests, as data: (n, depth, seed, vocab) of circuits.random_gates ---------------------
RANDOM_CIRCUITS = [  # test_random_circuits_fp32, with the engine options of each case
    ((14, 400, 31, "all"), {}),
    ((16, 500, 32, "clifford_t"), {}),
    ((18, 400, 33, "all"), {"tile_bits": 13, "tile_low_bits": 6}),
    ((20, 300, 34, "all"), {"tile_bits": 11, "tile_low_bits": 5, "tile_max_ops": 3}),
    ((19, 300, 35, "all"), {"tile_bits": 9, "tile_low_bits": 2}),
    ((20, 300, 36, "all"), {"grid_cap": 64}),
    ((22, 400, 37, "all"), {}),
]
TILE_ORDER_CIRCUIT = (17, 500, 91, "all")                        # test_tile_bit_order_fp32
TILE_SHAPES = [(8, 0), (9, 0), (10, 256), (10, 512), (11, 256), (11, 512), (12, 256), (12, 512), (12, 1024), (13, 512), (13, 1024)]
TILE_MANY = (18, 300, 1801, "all")                               # test_gpu_fp32_paths: many tiles ...


def tile_single(b):
    """... and a register of exactly one tile of 2^b amplitudes."""
    return (b, 150, 1800 + b, "all")


# (the three gates of seed 703, the fp64 test's, are exact in half precision: no check could see a rounding error there)
OOP_CIRCUITS = [(16, 3, 704, "all")] + [(16, d, 700 + d, "all") for d in (40, 90, 200, 400)] + [(16, 300, 77, "clifford_t")]
SPARE_CIRCUIT = (15, 350, 31, "all")
SPARSE_CIRCUIT = (18, 500, 21, "all")
FEW_CIRCUIT = (7, 120, 9, "all")    # run on an 18-qubit register: qubits 0..6 only, the rest stays exactly zero


def geometry_sweep_cases():
    """test_randomised_geometry_sweep_fp32: (case, (n, depth, seed, vocab), fuse, engine options), the options drawn the
    way test_gpu_parity.test_randomised_geometry_sweep draws them."""
    rng = np.random.default_rng(77)
    out = []
    for case in range(30):
        n = int(rng.integers(2, 20))
        depth = int(rng.integers(20, 300))
        tile_bits = int(rng.integers(8, 14))
        tile_low = int(rng.integers(max(2, tile_bits - 10), min(6, tile_bits - 2) + 1))
        opts = {"tile_bits": tile_bits, "tile_low_bits": tile_low, "tile_max_ops": int(rng.integers(1, 40)),
                "tile_pad_from": int(rng.integers(-1, 20))}
        if tile_bits >= 12 and rng.random() < 0.5:
            opts["tile_threads"] = int(rng.choice([256, 512, 1024] if tile_bits == 12 else [512, 1024]))
        if rng.random() < 0.3:
            opts["grid_cap"] = int(rng.integers(1, 64))
        fuse = int(rng.choice([0, 1, 2, 3, 3, 3]))
        out.append((case, (n, depth, 7000 + case, "all"), fuse, opts))
    return out


def all_circuits():
    """Every (n, depth, seed, vocab) above: the CPU test checks the reference cap and the checker's reach on each."""
    cs = [c for c, _ in RANDOM_CIRCUITS] + [TILE_ORDER_CIRCUIT, TILE_MANY] + [tile_single(b) for b, _ in TILE_SHAPES]
    cs += OOP_CIRCUITS + [SPARE_CIRCUIT, SPARSE_CIRCUIT, FEW_CIRCUIT] + [c for _, c, _, _ in geometry_sweep_cases()]
    return sorted(set(cs))


def gate_list(n, depth, seed, vocab):
    """The gate list the engine receives for circuits.random_gates(n, depth, seed, vocab): Circuit.gate(i) of every gate."""
    from gpu_quantum_simulator_amd import Circuit, circuits
    c = Circuit.from_text(circuits.qasm_text(n, circuits.random_gates(n, depth, seed, vocab)))
    return [c.gate(i) for i in range(len(c))]


# ---- the replay ------------------------------------------------------------------------------------------------------
def _apply_1q(s, U, q):
    v = s.reshape(-1, 2, 1 << q)
    a0, a1 = v[:, 0, :].copy(), v[:, 1, :].copy()
    v[:, 0, :] = U[0, 0] * a0 + U[0, 1] * a1
    v[:, 1, :] = U[1, 0] * a0 + U[1, 1] * a1


def _pair_view(s, n, a, b):
    hi, lo = max(a, b), min(a, b)
    return s.reshape(1 << (n - hi - 1), 2, 1 << (hi - lo - 1), 2, 1 << lo)  # axes 1 / 3: bit hi / bit lo


def _apply_cx(s, n, control, target):
    if control == target:
        return
    v = _pair_view(s, n, control, target)
    if control > target:
        x, y = v[:, 1, :, 0, :], v[:, 1, :, 1, :]
    else:
        x, y = v[:, 0, :, 1, :], v[:, 1, :, 1, :]
    t = x.copy()
    x[...] = y
    y[...] = t


def _apply_2q(s, n, M, q_hi, q_lo):
    v = _pair_view(s, n, q_hi, q_lo)
    a = {(h, l): v[:, h, :, l, :].copy() for h in (0, 1) for l in (0, 1)}
    for h in (0, 1):
        for l in (0, 1):
            r = 2 * h + l
            v[:, h, :, l, :] = M[r, 0] * a[0, 0] + M[r, 1] * a[0, 1] + M[r, 2] * a[1, 0] + M[r, 3] * a[1, 1]


def replay(n, gates, start=None, dtype=np.complex64):
    """Applies `gates` (the tuples Circuit.gate returns: ("u1", q, U), ("cx", c, t), ("u2", q_hi, q_lo, M)) one at a time
    in `dtype`, starting from `start` (default |0...0>).  Every matrix is rounded to `dtype` once and applied with `dtype`
    arithmetic; cx is an index permutation.  dtype=np.complex128 is the fp64 reference for cases without an oracle run."""
    if start is None:
        s = np.zeros(1 << n, dtype=dtype)
        s[0] = 1
    else:
        s = np.array(start, dtype=dtype, copy=True).reshape(-1)
        assert s.size == 1 << n
    for g in gates:
        if g[0] == "u1":
            _apply_1q(s, np.asarray(g[2]).astype(dtype), g[1])
        elif g[0] == "cx":
            _apply_cx(s, n, g[1], g[2])
        elif g[0] == "u2":
            _apply_2q(s, n, np.asarray(g[3]).astype(dtype), g[1], g[2])
        else:
            raise ValueError(f"unknown gate {g[0]!r}")
    return s


# ---- the checker -----------------------------------------------------------------------------------------------------
def rel_err(x, want):
    want = np.asarray(want, dtype=np.complex128)
    return float(np.linalg.norm(np.asarray(x, dtype=np.complex128) - want) / np.linalg.norm(want))


def check_fp32(got, want, ref32):
    """Asserts the fp32 criterion (module docstring); returns (rel_err(got, want), rel_err(ref32, want))."""
    e_got, e_ref = rel_err(got, want), rel_err(ref32, want)
    assert e_ref <= REF_CAP, f"the circuit breaks the reference cap: rel_err(ref32) = {e_ref:.3g} > {REF_CAP}"
    bound = C * max(e_ref, FLOOR)
    assert e_got <= bound, f"rel_err(got) = {e_got:.3g} > {C:g} * max(rel_err(ref32) = {e_ref:.3g}, 2^-24) = {bound:.3g}"
    return e_got, e_ref


def report(label, errs):
    """One line per checked case, for the -s output the accuracy records keep."""
    e_got, e_ref = errs
    ratio = e_got / e_ref if e_ref > 0 else float("inf") if e_got > 0 else 0.0
    print(f"fp32-accuracy {label}: rel_err(got)={e_got:.3e} rel_err(ref32)={e_ref:.3e} ratio={ratio:.3f} "
          f"bound_ratio={e_got / max(e_ref, FLOOR):.3f}")
