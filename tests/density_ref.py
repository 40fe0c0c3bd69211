"""The tests' own checker for reduced density matrices (qsim_reduced_density, csrc/density.hip, csrc/density.cpp).

`reduced_density(psi, qubits)` is the definition, rho[a][a'] = sum_b psi(a, b) conj(psi(a', b)) with bit j of a row or column index
being qubit qubits[j], as one tensordot; tests/test_density_cpu.py pins it against dense kron and partial-trace constructions.

The rest restates, in plain numpy and lane by lane, what the kernel's matrix path does (csrc/density.h): the plan (padding with the
lowest free bits, which path), the 16-byte units a lane loads, the operand tiles of the real matrix R = [Re Psi; Im Psi], G = R R^T
by 16 x 16 x 4 products in the operand layout of the fp64 matrix instruction (A[l & 15][l >> 4], B[l >> 4][l & 15]; C/D col =
lane & 15, row = (lane >> 4) + 4 reg), rho from G (Re rho = G_RR + G_II, Im rho = G_IR - G_RI), the trace over the padding and the
permutation into the caller's order.  It is pinned against `reduced_density`, and the C plan call against its geometry."""
import itertools

import numpy as np

MAX_QUBITS = 5
GRID_CAP = 1024   # kExpectGrid
WAVES = 4         # of a workgroup; each walks environment blocks of its own


def reduced_density(psi, qubits):
    """(2^k, 2^k) complex128; psi: 2^n amplitudes, index bit q = qubit q."""
    psi = np.asarray(psi, dtype=np.complex128)
    n = int(psi.size).bit_length() - 1
    qubits = list(qubits)
    k = len(qubits)
    t = psi.reshape((2,) * n) if n else psi.reshape(())
    axis = lambda q: n - 1 - q                                   # qubit q's axis: axis 0 is the top index bit
    rest = [axis(q) for q in range(n) if q not in qubits]
    rows = [axis(q) for q in reversed(qubits)]                   # qubits[k-1] is the top bit of a row index
    m = np.transpose(t, rows + rest).reshape(1 << k, -1)
    return m @ m.conj().T


def marginal(psi, qubits):
    return np.real(np.diagonal(reduced_density(psi, qubits))).copy()


def deposit(v, bits):
    """bit j of v -> index bit bits[j]"""
    return sum(((v >> j) & 1) << b for j, b in enumerate(bits))


# ---- the plan -------------------------------------------------------------------------------------------------------------------------
def shape(f32, kk, q0_in):
    """Constants of a kernel shape: row units, components that are rows of R, environments per unit, loads per lane and step, steps
    per trip, operand tiles."""
    ru = 1 << (kk - 1) if f32 and q0_in else 1 << kk
    cr = 4 if f32 and q0_in else 2
    es = 2 if f32 and not q0_in else 1
    nl = ru // 16 if ru >= 16 else 1
    return dict(ru=ru, cr=cr, es=es, nl=nl, u=8 // nl, nt=(2 << kk) // 16)


def plan(qubits, n, f32):
    """What plans.reduced_density_plan reports, or None where it refuses."""
    qubits = list(qubits)
    k = len(qubits)
    if not 0 <= n <= 40 or k > MAX_QUBITS or k > n or len(set(qubits)) != k or any(q < 0 or q >= n for q in qubits):
        return None
    kk = max(k, 3)
    path = 1 if n >= 3 and n - kk >= 2 else 0
    subset = sorted(qubits)
    if path:
        free = [q for q in range(n) if q not in subset]
        subset = sorted(subset + free[:kk - k])                  # the lowest free bits
    p = dict(path=path, padded_k=len(subset), subset=subset, mask=sum(1 << q for q in subset), units=max(1, (1 << n) >> (1 if f32 else 0)),
             trips=1, q0_in=0 in subset)
    if path:
        sh = shape(f32, kk, p["q0_in"])
        env_units = (1 << (n - kk)) // sh["es"]
        steps = (env_units + 3) // 4
        per_round = WAVES * sh["u"] * GRID_CAP
        p.update(env_units=env_units, trips=(steps + per_round - 1) // per_round)
    return p


def row_of(f32, kk, q0_in, tile, i):
    """(part, a): the row of R = [Re Psi; Im Psi] behind lane row i of operand tile `tile` (density_row)."""
    sh = shape(f32, kk, q0_in)
    if sh["ru"] >= 16:
        c, m = tile // sh["nl"], 16 * (tile % sh["nl"]) + i
    else:
        c, m = tile * (16 // sh["ru"]) + i // sh["ru"], i % sh["ru"]
    if f32 and q0_in:
        return c & 1, 2 * m + (c >> 1)
    return c, m


# ---- the kernel, lane by lane -------------------------------------------------------------------------------------------------------
def emulate(psi, qubits, f32):
    """(rho in the caller's order, 16-byte units read) by the kernel's decomposition; psi is used as it is (fp64 arithmetic)."""
    psi = np.asarray(psi, dtype=np.complex128)
    n = int(psi.size).bit_length() - 1
    qubits = list(qubits)
    p = plan(qubits, n, f32)
    subset, kk = p["subset"], p["padded_k"]
    dim = 1 << kk
    read = set()
    shift = 1 if f32 else 0
    if not p["path"]:
        env = [q for q in range(n) if q not in subset]
        rho = np.zeros((dim, dim), dtype=np.complex128)
        for a in range(dim):
            for b in range(dim):
                for e in range(1 << len(env)):
                    ja, jb = deposit(a, subset) | deposit(e, env), deposit(b, subset) | deposit(e, env)
                    read.update((ja >> shift, jb >> shift))
                    rho[a, b] += psi[ja] * np.conj(psi[jb])
    else:
        sh = shape(f32, kk, p["q0_in"])
        ru, es_n, nl, nt = sh["ru"], sh["es"], sh["nl"], sh["nt"]
        row_bits = [q for q in subset if not (f32 and q == 0)]   # fp32: index bit 0 is the slot inside a unit
        env_bits = [q for q in range(shift, n) if q not in subset]
        flat = np.stack([psi.real, psi.imag], axis=1).reshape(-1)  # (re, im) pairs: component c of unit u is flat[(4 or 2) u + c]
        per_unit = 4 if f32 else 2
        tiles = {}
        for step in range((p["env_units"] + 3) // 4):
            ops = np.zeros((es_n, nt, 64))
            for lane in range(64):
                i, eu = lane & 15, 4 * step + (lane >> 4)
                if eu >= p["env_units"]:
                    continue
                base = deposit(eu, env_bits)
                units = []
                for t in range(nl):
                    amp = base | deposit((16 * t + i) & (ru - 1), row_bits)
                    assert amp % (1 << shift) == 0
                    read.add(amp >> shift)
                    units.append(flat[per_unit * (amp >> shift):per_unit * (amp >> shift) + per_unit])
                for es in range(es_n):
                    for t in range(nt):
                        if ru >= 16:
                            ops[es, t, lane] = units[t % nl][2 * es + t // nl]
                        else:
                            ops[es, t, lane] = units[0][2 * es + t * (16 // ru) + i // ru]
            for es in range(es_n):
                for s in range(nt):
                    for t in range(s, nt):
                        a_op = ops[es, s].reshape(4, 16).T      # A[i][k] sits in lane (k << 4) | i
                        b_op = ops[es, t].reshape(4, 16)        # B[k][j] in lane (k << 4) | j
                        tiles[s, t] = tiles.get((s, t), np.zeros((16, 16))) + a_op @ b_op
        where = {row_of(f32, kk, p["q0_in"], t, i): (t, i) for t in range(nt) for i in range(16)}
        assert len(where) == 2 * dim                            # every row of R is one lane row of one tile

        def g(r, c):
            (s, i), (t, j) = where[r], where[c]
            return tiles[s, t][i, j] if s <= t else tiles[t, s][j, i]

        rho = np.zeros((dim, dim), dtype=np.complex128)
        for a in range(dim):
            for b in range(a, dim):
                rho[a, b] = complex(g((0, a), (0, b)) + g((1, a), (1, b)), g((1, a), (0, b)) - g((0, a), (1, b)))
                rho[b, a] = np.conj(rho[a, b])
    # the trace over the padding and the caller's order
    k = len(qubits)
    pos = [subset.index(q) for q in qubits]
    pad = [j for j in range(kk) if j not in pos]
    out = np.zeros((1 << k, 1 << k), dtype=np.complex128)
    for a in range(1 << k):
        for b in range(1 << k):
            for t in range(1 << len(pad)):
                out[a, b] += rho[deposit(a, pos) | deposit(t, pad), deposit(b, pos) | deposit(t, pad)]
    return out, len(read)


def subsets(n, k):
    return [list(c) for c in itertools.combinations(range(n), k)]
