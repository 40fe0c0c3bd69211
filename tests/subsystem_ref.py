"""A numpy restatement of the blocked R R^T behind qsim_subsystem_density (csrc/subsystem.h, csrc/subsystem.hip, csrc/subsystem.cpp;
DESIGN §7m), for reduced density matrices of 6 to 10 qubits.

The checker stays density_ref.reduced_density.  This file restates what the kernels and the host do: the plan (which path, the blocks
of 128 rows of R, the chunks of 32 environments, the slices and trips, the units read, the scratch), which 16-byte units a workgroup's
threads load for a (block, chunk) and where each component lands in a panel, the rows of R in block b (row 2a = Re Psi[a], row 2a + 1 =
Im Psi[a], a >> 6 == b over the SORTED subset), the environments of slice s, the partial blocks accumulated four environments at a
time (of a diagonal block only the tiles on and above the diagonal) and added in ascending slice order, rho from G, and the
caller's order.  tests/test_subsystem_cpu.py pins it against the checker and the C plan call against its geometry."""
import numpy as np

MAX_QUBITS = 10
MIN_QUBITS = 6            # fewer: qsim_reduced_density (density_ref)
BLOCK_ROWS = 128
BLOCK_AMP_BITS = 6
CHUNK_ENV_BITS = 5
MAX_PARTIAL_BLOCKS = 4096
MAX_SLICES = 1024
MIN_TRIPS = 4
TPB = 256
LOWER_TILES = np.kron(np.tril(np.ones((8, 8)), -1), np.ones((16, 16))).astype(bool)  # of a block's 8 x 8 tiles of 16 x 16


def deposit(v, bits):
    """bit j of v (an int or an integer array) -> index bit bits[j]"""
    out = v * 0
    for j, b in enumerate(bits):
        out = out | (((v >> j) & 1) << b)
    return out


def extract(idx, bits):
    """the inverse: index bit bits[j] -> bit j"""
    out = idx * 0
    for j, b in enumerate(bits):
        out = out | (((idx >> b) & 1) << j)
    return out


def plan(qubits, n, f32):
    """What plans.subsystem_density_plan reports, or None where it refuses."""
    qubits = list(qubits)
    k = len(qubits)
    if not 0 <= n <= 40 or k > MAX_QUBITS or k > n or len(set(qubits)) != k or any(q < 0 or q >= n for q in qubits):
        return None
    shift = 1 if f32 else 0
    p = dict(path=2, block_rows=0, upper_blocks=0, slices=0, units_read=max(1, (1 << n) >> shift), scratch_bytes=0, trips=1,
             subset=sorted(qubits))
    if k < MIN_QUBITS:
        return p
    if n - k < 2:
        p.update(path=0, units_read=(2 << (2 * k + n - k)) >> shift, scratch_bytes=16 << (2 * k))
        return p
    blocks = (2 << k) // BLOCK_ROWS
    upper = blocks * (blocks + 1) // 2
    env_bits = min(CHUNK_ENV_BITS, n - k)
    chunks = 1 << (n - k - env_bits)
    target = 1
    while 2 * target * upper <= MAX_PARTIAL_BLOCKS and 2 * target <= MAX_SLICES:
        target *= 2
    slices = min(target, max(1, chunks // MIN_TRIPS))
    p.update(path=1, block_rows=BLOCK_ROWS, blocks=blocks, upper_blocks=upper, env_bits=env_bits, chunks=chunks, slices=slices,
             trips=chunks // slices, units_read=((1 << n) >> shift) * blocks, scratch_bytes=(slices + 1) * upper * BLOCK_ROWS * BLOCK_ROWS * 8)
    return p


def stage_panel(flat, p, n, f32, block, chunk):
    """The panel of block row `block` and chunk `chunk` as the workgroup's threads stage it: (environments of a chunk, 128 rows of R)
    and the number of 16-byte units loaded.  flat: the state as (re, im) doubles.  Every cell is written exactly once."""
    subset = p["subset"]
    env = [q for q in range(n) if q not in subset]
    row_low, env_low = subset[:BLOCK_AMP_BITS], env[:p["env_bits"]]
    free = sorted(q for q in row_low + env_low if not (f32 and q == 0))  # fp32: index bit 0 is the slot inside a unit
    units = (1 << (BLOCK_AMP_BITS + p["env_bits"])) >> (1 if f32 else 0)
    t = np.arange(units, dtype=np.int64)                         # thread tid takes t = tid, tid + 256, ...
    own = deposit(t, free)
    base = deposit(chunk << p["env_bits"], env) | deposit(block << BLOCK_AMP_BITS, subset)
    a_low, e_low = extract(own, row_low), extract(own, env_low)
    panel = np.full((1 << p["env_bits"], BLOCK_ROWS), np.nan)
    written = np.zeros(panel.shape, dtype=np.int64)
    amp = base | own
    slots = [(0, 0, 0)]
    if f32:
        assert np.all(amp % 2 == 0)
        slots.append((1, 1, 0) if 0 in subset else (1, 0, 1))    # the second amplitude: the next row of Psi, or the next environment
    for d_amp, d_a, d_e in slots:
        for part in (0, 1):
            panel[e_low + d_e, 2 * (a_low + d_a) + part] = flat[2 * (amp + d_amp) + part]
            np.add.at(written, (e_low + d_e, 2 * (a_low + d_a) + part), 1)
    assert np.all(written == 1)
    # consecutive threads take consecutive units: whole 128-byte lines wherever the subset lies
    unit_index = np.sort(amp >> (1 if f32 else 0))
    assert np.all(unit_index[0::8] % 8 == 0) and np.all(np.diff(unit_index.reshape(-1, 8), axis=1) == 1)
    return panel, units


def block_of(blocks, index):
    bi = 0
    while index >= blocks - bi:
        index -= blocks - bi
        bi += 1
    return bi, bi + index


def emulate(psi, qubits, f32):
    """(rho in the caller's order, 16-byte units read by all workgroups) by the kernels' decomposition; psi is used as it is."""
    psi = np.asarray(psi, dtype=np.complex128)
    n = int(psi.size).bit_length() - 1
    qubits = list(qubits)
    p = plan(qubits, n, f32)
    subset, k = p["subset"], len(qubits)
    dim = 1 << k
    env = [q for q in range(n) if q not in subset]
    flat = np.stack([psi.real, psi.imag], axis=1).reshape(-1)
    if p["path"] == 0:                                           # a thread per element, the environments in ascending order
        rows = deposit(np.arange(dim, dtype=np.int64), subset)
        full = np.zeros((dim, dim), dtype=np.complex128)
        for b in range(1 << len(env)):
            col = psi[rows | deposit(b, env)]
            full += np.outer(col, col.conj())
        rho = np.triu(full)
        units = (2 * dim * dim << len(env)) >> (1 if f32 else 0)
    else:
        assert p["path"] == 1
        blocks, upper, trips = p["blocks"], p["upper_blocks"], p["trips"]
        units = 0
        result = None
        for s in range(p["slices"]):                             # ascending slice order
            partial = np.zeros((upper, BLOCK_ROWS, BLOCK_ROWS))
            for blk in range(upper):
                bi, bj = block_of(blocks, blk)
                for chunk in range(s * trips, (s + 1) * trips):  # the environments of slice s
                    pa, u = stage_panel(flat, p, n, f32, bi, chunk)
                    units += u
                    pb = pa
                    if bj != bi:
                        pb, u = stage_panel(flat, p, n, f32, bj, chunk)
                        units += u
                    for e0 in range(0, 1 << p["env_bits"], 4):   # one matrix instruction: four environments
                        partial[blk] += pa[e0:e0 + 4].T @ pb[e0:e0 + 4]
                if bi == bj:                                     # symmetric: only the 36 tiles with row <= column are multiplied,
                    partial[blk][LOWER_TILES] = 0.0              # the others are written as zeros
            result = partial if result is None else result + partial
        g = np.zeros((2 * dim, 2 * dim))                         # the upper blocks of G; rows and columns 2a: Re Psi[a], 2a + 1: Im Psi[a]
        for blk in range(upper):
            bi, bj = block_of(blocks, blk)
            g[bi * BLOCK_ROWS:(bi + 1) * BLOCK_ROWS, bj * BLOCK_ROWS:(bj + 1) * BLOCK_ROWS] = result[blk]
        rho = np.triu((g[0::2, 0::2] + g[1::2, 1::2]) + 1j * (g[1::2, 0::2] - g[0::2, 1::2]))  # a <= b: Re = G_RR + G_II, Im = G_IR - G_RI
    rho = np.triu(rho, 1) + np.triu(rho, 1).conj().T + np.diag(np.real(np.diagonal(rho)))
    at = deposit(np.arange(dim, dtype=np.int64), [subset.index(q) for q in qubits])  # caller's index -> index over the sorted subset
    return rho[np.ix_(at, at)], units
