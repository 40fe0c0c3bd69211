"""The tests' own model of how the one-gate streaming kernels (csrc/gate_kernels.inc), the readout kernels
(csrc/readout_kernels.inc) and k_pack are launched: a restatement of the launch arithmetic of csrc/launch.inc, and the cases of
tests/test_gpu_streaming_kernels.py as data, so that the GPU tests state what they mean ("this launch is guarded", "its busiest
workgroup takes two trips") instead of hard-coding register sizes (tests/test_streaming_ref_cpu.py pins the tables on the CPU).

A gate kernel works on `items` work items in work tiles of TPB * IPT of them; workgroup w takes tiles w, w + grid, w + 2 grid, ...
The launch takes the GUARD = true instantiation when the items do not fill whole work tiles (QSIM_DISPATCH_GUARD).  k_init,
k_zero_outside, k_norm2 and k_gather_masked stride over amplitudes, k_block_prob over blocks of 2^12 amplitudes (qsim_sample),
each with a fixed cap on its grid; k_pack walks work tiles of 2^10 amplitudes under grid_cap and 8192 workgroups."""
import numpy as np

TPB = 256
MAX_GRID = 1 << 22      # kMaxGrid: beyond this the gate kernels loop without being asked to
SAMPLE_BLOCK_BITS = 12  # qsim_sample's kBlockBits


def ceil_div(a, b):
    return (a + b - 1) // b


def capped_grid(items, per_wg, cap):
    g = ceil_div(items, per_wg)
    return cap if g > cap else g if g else 1


def grid_for(grid_cap, ntiles):
    return capped_grid(ntiles, 1, grid_cap if 0 < grid_cap < MAX_GRID else MAX_GRID)


# kernel -> (work items of an n-qubit register, items per thread, smallest register the engine launches it on).  k_gate1_hi needs
# a target q >= 6, k_phase q >= 2 (below that diag(1, lambda) takes k_diag1_full), k_cx two qubits, k_gate2_hh 7 > 6 >= q_lo.
GATE_KERNELS = {
    "k_gate1_hi": (lambda n: (1 << n) >> 1, 4, 7),
    "k_gate1_lo": (lambda n: 1 << n, 4, 1),
    "k_phase": (lambda n: (1 << n) >> 1, 4, 3),
    "k_diag1_full": (lambda n: 1 << n, 4, 1),
    "k_cx": (lambda n: (1 << n) >> 2, 4, 2),
    "k_gate2_hh": (lambda n: (1 << n) >> 2, 2, 8),
}
# kernel -> (work items, items per workgroup, grid cap) of the kernels that cap their own grid
STRIDED_KERNELS = {
    "k_init": (lambda n: 1 << n, TPB, 16384),
    "k_zero_outside": (lambda n: 1 << n, TPB, 16384),
    "k_norm2": (lambda n: 1 << n, TPB * 8, 4096),
    "k_block_prob": (lambda n: (1 << n) >> min(n, SAMPLE_BLOCK_BITS), 1, 65536),
}
# the class sim.stats()["kernels"] counts a launch under (k_phase and k_diag1_full share one; the readout kernels have none)
STATS_CLASS = {"k_gate1_hi": "gate1", "k_gate1_lo": "gate1_lo", "k_phase": "phase", "k_diag1_full": "phase", "k_cx": "cx",
               "k_gate2_hh": "gate2", "k_init": "init", "k_zero_outside": "init", "k_pack": "pack"}


class Launch:
    """guarded: the bounds-checked form runs; grid: workgroups; tiles: work tiles (or strides' worth of items) in all."""

    def __init__(self, guarded, grid, tiles):
        self.guarded, self.grid, self.tiles = guarded, grid, tiles

    @property
    def max_trips(self):  # of the busiest workgroup (workgroup 0)
        return ceil_div(self.tiles, self.grid)

    @property
    def uneven(self):  # some workgroups take a trip fewer than others
        return self.tiles % self.grid != 0

    def __repr__(self):
        return f"Launch(guarded={self.guarded}, grid={self.grid}, tiles={self.tiles}, max_trips={self.max_trips})"


def launch(kernel, n, grid_cap=0):
    """What launch.inc does for `kernel` on an n-qubit register under QSIM_OPT_GRID_CAP = grid_cap (0: none)."""
    if kernel in GATE_KERNELS:
        items_of, ipt, n_min = GATE_KERNELS[kernel]
        assert n >= n_min, f"{kernel} never runs on {n} qubits"
        items, per_tile = items_of(n), TPB * ipt
        ntiles = ceil_div(items, per_tile)
        return Launch(items % per_tile != 0, grid_for(grid_cap, ntiles), ntiles)
    if kernel == "k_pack":
        ntiles = ceil_div(1 << n, TPB * 4)
        return Launch((1 << n) % (TPB * 4) != 0, capped_grid(grid_for(grid_cap, ntiles), 1, 8192), ntiles)
    items_of, per_wg, cap = STRIDED_KERNELS[kernel]  # every thread checks its index: always guarded
    items = items_of(n)
    return Launch(True, capped_grid(items, per_wg, cap), max(1, ceil_div(items, per_wg)))


def guarded_sizes(kernel, up_to=16):
    """The register sizes, from the smallest the kernel runs on, at which its launch is guarded."""
    return [n for n in range(GATE_KERNELS[kernel][2], up_to + 1) if launch(kernel, n).guarded]


# ---- the cases ---------------------------------------------------------------------------------------------------------------
EVERY_POSITION_SIZES = tuple(range(1, 13))  # a: every guarded size of every gate kernel and the first unguarded one
LOOP_N = 14                                 # b
LOOP_CAPS = (0, 1, 3, 5, 1 << 30)
INIT_LOOP_N = 23                            # c: 2^23 / 256 = 2 * 16384 workgroups' worth
SAMPLE_LOOP_N = 29                          # e: 2^29 / 2^12 = 2 * 65536 blocks
SAMPLE_DENSE_N = 20                         # d
SAMPLE_SMALL_SIZES = (1, 2, 5, 11)
PACK_SMALL_SIZES = (2, 5, 9, 10, 11)        # f

LAMBDA = np.exp(2.1j)                       # diag(1, LAMBDA): |LAMBDA - 1| = 1.73, a skipped item is off by its own size
D0, D1 = np.exp(-2.6j), np.exp(1.9j)        # diag(D0, D1), both further than 1.8 from 1


def band(n):
    """Guard band, in amplitudes, on each side of an n-qubit state.  A full work tile of a guarded launch holds at most TPB * 4 =
    1024 items; two bit insertions (k_cx, k_gate2_hh) at most quadruple an item number, so an overrun of such a tile reaches
    below 4096 amplitudes; an index with a spurious bit n or n + 1 set reaches below 4 * 2^n."""
    return max(4 << n, 4096)


def positions(kernel, n):
    """Every argument tuple the engine can hand `kernel` on n qubits: (q,) targets, (control, target) or (q_hi, q_lo) pairs."""
    if kernel == "k_gate1_hi":
        return [(q,) for q in range(6, n)]
    if kernel == "k_gate1_lo":
        return [(q,) for q in range(min(n, 6))]
    if kernel == "k_phase":
        return [(q,) for q in range(2, n)]
    if kernel == "k_diag1_full":
        return [(q,) for q in range(n)]
    if kernel == "k_cx":
        return [(c, t) for c in range(n) for t in range(n) if c != t]
    if kernel == "k_gate2_hh":
        return [(hi, lo) for hi in range(7, n) for lo in range(6, hi)]
    raise ValueError(kernel)


def dense_2x2(seed):
    """A unitary that is neither symmetric nor diagonal, every entry well away from 0 and 1."""
    rng = np.random.default_rng(seed)
    t, a, b, d = rng.uniform(0.6, 1.0), *rng.uniform(0.5, 2.5, 3)
    c = 2.0 * b + d  # U[0, 1] = -sin t e^(i (b + d)) against U[1, 0] = sin t e^(i b): |difference| = 2 sin t |cos(d / 2)| > 0.3
    return np.array([[np.cos(t) * np.exp(1j * a), -np.sin(t) * np.exp(1j * (c - b))],
                     [np.sin(t) * np.exp(1j * b), np.cos(t) * np.exp(1j * (c - a))]])


def rand_state(n, seed):
    rng = np.random.default_rng(seed)
    s = rng.standard_normal(1 << n) + 1j * rng.standard_normal(1 << n)
    return (s / np.linalg.norm(s)).astype(np.complex128)


def pack_src_index(n, bits):
    """qsim_pack_bits layout: packed index (block << (n-k)) | rest reads source index src[packed]."""
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


def pack_bit_sets(n):
    """The bit sets of the small pack cases that fit n qubits (qsim_pack_bits_to takes up to three bits)."""
    sets = [(0,), (n - 1,), (0, n - 1)] + ([(1, 3, 4)] if n >= 5 else [])
    return sorted(set(s for s in sets if len(set(s)) == len(s)))


def zero_block_state(n=SAMPLE_DENSE_N):
    """Non-zero only in blocks 3, 200 and 201 of 2^12 amplitudes, with a run of zeros at the start of block 3.  Every amplitude is
    +-2^-7 or +-2^-6, real or imaginary, so every probability is 1 or 4 units of 2^-14 (exact in fp32 as well), the units add
    up to 2^14 and every partial sum is exact whatever the order of summation."""
    rng = np.random.default_rng(2002)
    s = np.zeros(1 << n, dtype=np.complex128)
    blk = 1 << SAMPLE_BLOCK_BITS
    phase = lambda m: np.array([1, 1j, -1, -1j])[rng.integers(0, 4, m)]
    s[3 * blk + 512:4 * blk] = 2.0 ** -7 * phase(blk - 512)    # 3584 units
    s[200 * blk:201 * blk] = 2.0 ** -7 * phase(blk)            # 4096
    s[201 * blk:201 * blk + 1536] = 2.0 ** -6 * phase(1536)    # 6144
    s[201 * blk + 1536:202 * blk] = 2.0 ** -7 * phase(blk - 1536)  # 2560
    return s


# ---- the n = 29 sampling state: one 2x2 on each of four qubits of |0...0> -----------------------------------------------------
SPARSE_QUBITS = (28, 17, 12, 3)
SPARSE_P0 = (0.36, 0.55, 0.42, 0.67)  # probability of 0 on each of them; both outcomes within [0.3, 0.7]


def sparse_matrices():
    """One non-symmetric unitary per qubit of SPARSE_QUBITS whose first column has |.|^2 = (p0, 1 - p0)."""
    out = []
    for j, p0 in enumerate(SPARSE_P0):
        a, b = np.sqrt(p0) * np.exp(0.4j + 0.9j * j), np.sqrt(1.0 - p0) * np.exp(-1.1j + 0.5j * j)
        ph = np.exp(0.7j * (j + 1))
        out.append(np.array([[a, -np.conj(b) * ph], [b, np.conj(a) * ph]]))
    return out


def sparse_state(qubits=SPARSE_QUBITS):
    """(indices ascending, amplitudes, probabilities) of the sixteen non-zero amplitudes, as products of matrix entries."""
    mats = sparse_matrices()
    rows = []
    for k in range(16):
        idx, amp, p = 0, 1.0 + 0.0j, 1.0
        for j, q in enumerate(qubits):
            bit = (k >> j) & 1
            idx |= bit << q
            amp *= mats[j][bit, 0]
            p *= SPARSE_P0[j] if bit == 0 else 1.0 - SPARSE_P0[j]
        rows.append((idx, amp, p))
    rows.sort()
    return (np.array([r[0] for r in rows], dtype=np.int64), np.array([r[1] for r in rows]), np.array([r[2] for r in rows]))


def sparse_draws():
    """(draws, expected index of each): the midpoints between consecutive running probabilities, answered by the first of the
    sixteen indices whose running probability reaches the draw, and r = 0, answered by the first index.  The GPU test adds
    r = 1 itself: that draw sits ON the last running value, which is 1 only up to rounding.  Also the running values."""
    idx, _, p = sparse_state()
    run = np.cumsum(p)
    mids = np.concatenate([[0.5 * run[0]], 0.5 * (run[:-1] + run[1:])])
    draws = np.concatenate([[0.0], mids])
    want = np.concatenate([[idx[0]], idx])
    return draws, want, run
