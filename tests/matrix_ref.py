"""The tests' own checker for dense matrices on target qubits under controls (qsim_apply_matrix, csrc/matrix.hip, csrc/matrix.cpp).

`apply_matrix_gather(psi, U, targets, controls, dtype)` is the definition: inside the subspace where every control bit is 1, gather
the 2^k amplitudes of every environment (bit j of a row or column index of U is qubit targets[j]), multiply, scatter; everything
else keeps its bits.  `apply_matrix` is the same through reshaped views and one tensordot, several times faster on large registers.
tests/test_matrix_cpu.py pins both against dense Kronecker operators and the helpers of the 1q / 2q / cx tests, and each other.

`emulate_operand` restates, lane by lane, what the kernel's matrix path does with the operand the library hands it
(plans.apply_matrix_operand): R' = M R in 16 x 16 tiles by 16 x 16 x 4 products in the layout of the fp64 matrix instruction
(A[l & 15][l >> 4], B[l >> 4][l & 15]; C/D col = l & 15, row = (l >> 4) + 4 reg), every lane feeding components of units it loaded
and storing what the D map gives it."""
import numpy as np


def deposit(v, bits):
    """bit j of v -> index bit bits[j]"""
    return sum(((v >> j) & 1) << b for j, b in enumerate(bits))


def apply_matrix(psi, U, targets, controls=(), dtype=np.complex128):
    """A new array of `dtype`: psi with U applied on `targets` where all `controls` are 1.  U is rounded to `dtype` once and the
    products and sums are `dtype` arithmetic (complex64: the fp32 replay).  The same gather, matmul and scatter as apply_matrix_gather,
    through views: the register is reshaped so that every target and control is an axis of its own, the control axes are fixed at 1
    and one tensordot contracts the target axes — what the tests of 2^22 amplitudes and more can afford."""
    out = np.array(psi, dtype=dtype, copy=True).reshape(-1)
    n = int(out.size).bit_length() - 1
    targets, controls = list(targets), list(controls)
    k = len(targets)
    m = np.asarray(U, dtype=np.complex128).reshape(1 << k, 1 << k).astype(dtype)
    shape, axis_of, above = [], {}, n
    for q in sorted(targets + controls, reverse=True):           # ..., 2^(bits between), 2 (qubit q), 2^(bits below)
        shape.append(1 << (above - q - 1))
        axis_of[q] = len(shape)
        shape.append(2)
        above = q
    shape.append(1 << above)
    index = [slice(None)] * len(shape)
    for q in controls:
        index[axis_of[q]] = 1
    sub = out.reshape(shape)[tuple(index)]                       # a view of the control subspace; its control axes are gone
    kept = [a for a in range(len(shape)) if a not in [axis_of[q] for q in controls]]
    if k == 0:
        sub[...] = (m[0, 0] * sub).astype(dtype)
        return out
    axes = [kept.index(axis_of[targets[j]]) for j in reversed(range(k))]   # the top bit of a matrix index is targets[k-1]
    res = np.tensordot(m.reshape((2,) * (2 * k)), sub, axes=(list(range(k, 2 * k)), axes))
    sub[...] = np.moveaxis(res, list(range(k)), axes)
    return out


def apply_matrix_gather(psi, U, targets, controls=(), dtype=np.complex128):
    """The definition, literally: gather the 2^k amplitudes of every environment inside the control subspace, matmul, scatter."""
    out = np.array(psi, dtype=dtype, copy=True).reshape(-1)
    n = int(out.size).bit_length() - 1
    targets, controls = list(targets), list(controls)
    k = len(targets)
    m = np.asarray(U, dtype=np.complex128).reshape(1 << k, 1 << k).astype(dtype)
    env = [q for q in range(n) if q not in targets and q not in controls]
    ones = sum(1 << q for q in controls)
    rows = np.array([deposit(a, targets) for a in range(1 << k)], dtype=np.int64)
    cols = np.array([deposit(b, env) | ones for b in range(1 << len(env))], dtype=np.int64)
    idx = rows[:, None] | cols[None, :]                          # (2^k, environments)
    out[idx] = (m @ out[idx]).astype(dtype)
    return out


def dense_operator(n, U, targets, controls=()):
    """The 2^n x 2^n matrix of the same map, built entry by entry."""
    k = len(targets)
    m = np.asarray(U, dtype=np.complex128).reshape(1 << k, 1 << k)
    ones = sum(1 << q for q in controls)
    tmask = sum(1 << q for q in targets)
    op = np.zeros((1 << n, 1 << n), dtype=np.complex128)
    for col in range(1 << n):
        if col & ones != ones:
            op[col, col] = 1.0
            continue
        b = sum(((col >> q) & 1) << j for j, q in enumerate(targets))
        for a in range(1 << k):
            op[(col & ~tmask) | deposit(a, targets), col] = m[a, b]
    return op


def emulate_operand(M, row_amp, row_part, columns, f32, q0_in):
    """`columns`: (2^K, 16) complex — the amplitudes of 16 environments over the SORTED kernel subset.  Returns the (2^K, 16) result
    assembled from what every lane receives, and checks on the way that a lane supplies and receives the same rows and that these
    are whole 16-byte units."""
    rows = M.shape[0]
    kdim = rows // 2
    assert M.shape == (rows, rows) and columns.shape == (kdim, 16) and rows % 16 == 0
    R = np.zeros((rows, 16))
    for r in range(rows):
        R[r] = columns[row_amp[r]].imag if row_part[r] else columns[row_amp[r]].real
    assert sorted(zip(row_amp, row_part)) == [(a, p) for a in range(kdim) for p in (0, 1)]   # every row of [Re; Im] once
    out = np.zeros((rows, 16))
    received = {lane: [] for lane in range(64)}
    supplied = {lane: [] for lane in range(64)}
    for t in range(rows // 16):
        acc = np.zeros((64, 4))                                  # the lanes' accumulator registers
        for s in range(rows // 4):
            a_op = np.array([M[16 * t + (lane & 15), 4 * s + (lane >> 4)] for lane in range(64)])
            b_op = np.zeros(64)
            for lane in range(64):
                r = 4 * s + (lane >> 4)                          # B[k = lane >> 4][col = lane & 15]: the lane's own row of slice s
                b_op[lane] = R[r, lane & 15]
                if t == 0:
                    supplied[lane].append(r)
            A = a_op.reshape(4, 16).T                            # A[i][k] sits in lane (k << 4) | i
            B = b_op.reshape(4, 16)                              # B[k][j] in lane (k << 4) | j
            D = A @ B
            for lane in range(64):
                for reg in range(4):
                    acc[lane, reg] += D[(lane >> 4) + 4 * reg, lane & 15]
        for lane in range(64):
            for reg in range(4):
                r = 16 * t + (lane >> 4) + 4 * reg
                out[r, lane & 15] = acc[lane, reg]
                received[lane].append(r)
    for lane in range(64):
        assert sorted(received[lane]) == sorted(supplied[lane]), lane
        mine = {(row_amp[r], row_part[r]) for r in received[lane]}
        amps = {a for a, _ in mine}
        assert mine == {(a, p) for a in amps for p in (0, 1)}    # Re and Im of an amplitude go together
        if f32 and q0_in:                                        # a unit is the even and the odd row of the subset's lowest bit
            assert amps == {a ^ 1 for a in amps}
    res = np.zeros((kdim, 16), dtype=np.complex128)
    for r in range(rows):
        if row_part[r]:
            res[row_amp[r]] += 1j * out[r]
        else:
            res[row_amp[r]] += out[r]
    return res
