"""An independent interpreter of the TileOp record k_tile reads (csrc/qsim_internal.h), in plain numpy.

Written from the layout comments of qsim_internal.h, not from the kernel: the LDS swizzle is restated from its prose (which
column of GF(2)^4 / GF(2)^5 each higher slot bit gets), the header and the part records are decoded byte by byte, and apply()
runs a record on a tile the way the comments say a workgroup does — items, parts, group bases from the lane nibbles, one read
of T operands per class, T rows written.  tests/test_tile_records_cpu.py holds every record the encoder (csrc/tile_op.cpp)
produces for the suite's circuits to this model; tests/test_gpu_tile_forms.py runs the same block forms on the device.

Layout (bytes).  TileOp: 0 kind, 1 nq, 2 terms, 3 nsel, 4-5 selbit, 6 ident, 7 flags, 8-15 b[8], 32 scale[4][2] (doubles; fp32:
two floats in the first 8 bytes of each), 128 rec[4][8].  PartRec (576): 0 off[8] (u32), 32 rowoff[8] (u32), 64 coef: entry j of
position p in the 16 bytes at 64 + (p*T + j) * 16 — fp64 (re, im), fp32 the float pairs (ur, ui), (-ui, ur).
"""
import numpy as np

TOP_G1, TOP_G2, TOP_DIAG1, TOP_PART, TOP_SCALE = 1, 2, 3, 4, 5
MAX_BANKS, MAX_PARTS, PART_ROWS = 4, 8, 8
SKIP_CLASS = 0xFFFFFFFF
FLAG_SKIPS, FLAG_CLOSED = 1, 2
LANE_NIBBLES, LANE_NONE = 10, 15
INFO_LOG2T_SHIFT, INFO_SKIPS, INFO_BARRIER = 1, 8, 16
REC_BYTES, OP_BYTES = 576, 128 + 4 * 8 * 576


# ---- the LDS layout swizzle ------------------------------------------------------------------------------------------------
def slot_shift(f32):
    """log2 of the LDS slot size: 16-byte slots for fp64 amplitudes, 8-byte slots for fp32."""
    return 3 if f32 else 4


def sw_low(f32):
    """Slot bits below this are the unit inside a 256-byte bank row."""
    return 5 if f32 else 4


_COL64 = (0b1111, 0b0001, 0b0010, 0b0100, 0b1000)  # slot bit 4 + j gets column j mod 5


def _col32(i):
    """fp32: slot bit 5 + i (i < 5) gets e_i ^ e_(i+1 mod 5), slot bit 10 + i the three ones 00111 << i."""
    return (1 << i) ^ (1 << ((i + 1) % 5)) if i < 5 else (0b00111 << (i - 5)) & 31


def _fold_table(f32):
    """The XOR of the columns of the set bits of hi, for every hi of 10 bits (a linear map into the unit bits)."""
    hi = np.arange(1 << 10, dtype=np.int64)
    out = np.zeros_like(hi)
    for j in range(10):
        col = _col32(j) if f32 else _COL64[j % 5]
        out ^= ((hi >> j) & 1) * col
    return out


_FOLD = {False: _fold_table(False), True: _fold_table(True)}


def lds_sw_fold(hi, f32):
    """fold(hi), hi = slot >> sw_low (at most 10 bits)."""
    return _FOLD[bool(f32)][np.asarray(hi, dtype=np.int64)]


def slot_byte(slot, f32):
    """LDS byte address of logical tile slot `slot`: (s ^ fold(s >> low)) << S."""
    slot = np.asarray(slot, dtype=np.int64)
    return (slot ^ lds_sw_fold(slot >> sw_low(f32), f32)) << slot_shift(f32)


# ---- decoding --------------------------------------------------------------------------------------------------------------
def header(record):
    r = np.frombuffer(record, dtype=np.uint8)
    assert r.size == OP_BYTES, r.size
    nib = int.from_bytes(bytes(r[8:13]), "little")
    info = int(r[15])
    return {"kind": int(r[0]), "nq": int(r[1]), "terms": int(r[2]), "nsel": int(r[3]), "selbit": (int(r[4]), int(r[5])),
            "ident": int(r[6]), "flags": int(r[7]), "b": tuple(int(x) for x in r[8:16]),
            "nibbles": tuple((nib >> (4 * a)) & 15 for a in range(LANE_NIBBLES)),
            "info": info, "info_log2T": (info >> INFO_LOG2T_SHIFT) & 3, "info_skips": bool(info & INFO_SKIPS),
            "info_barrier": bool(info & INFO_BARRIER)}


def _rec(record, bank, part):
    at = 128 + (bank * MAX_PARTS + part) * REC_BYTES
    return record[at:at + REC_BYTES]


def offsets(record, bank, part):
    """(off[8], rowoff[8]) of one part record, as int64."""
    w = np.frombuffer(_rec(record, bank, part)[:64], dtype="<u4").astype(np.int64)
    return w[:8], w[8:]


def coef_raw(record, bank, part, f32):
    """The 32 coefficient cells of one part record as stored: fp64 -> (32,) complex128; fp32 -> (32, 4) float32."""
    raw = _rec(record, bank, part)[64:]
    if f32:
        return np.frombuffer(raw, dtype="<f4").reshape(32, 4)
    return np.frombuffer(raw, dtype="<f8").reshape(32, 2).view(np.complex128).reshape(32)


def coefs(record, bank, part, f32):
    """... and as the numbers they stand for: (32,) complex128 (fp32: the first float pair)."""
    c = coef_raw(record, bank, part, f32)
    if f32:
        return c[:, 0].astype(np.float64) + 1j * c[:, 1].astype(np.float64)
    return c


def scale(record, bank, f32):
    raw = record[32 + 16 * bank: 48 + 16 * bank]
    if f32:
        re, im = np.frombuffer(raw[:8], dtype="<f4")
        return complex(float(re), float(im))
    re, im = np.frombuffer(raw, dtype="<f8")
    return complex(re, im)


# ---- geometry --------------------------------------------------------------------------------------------------------------
def local_bit(geom, q):
    """Tile-local bit of global qubit q under geom = (tile_bits, low_bits, high): low bits are themselves, high[j] is bit L + j."""
    B, L, high = geom
    if q < L:
        return q
    return L + list(high).index(q)


# ---- running a record --------------------------------------------------------------------------------------------------------
_ADDR = {}


def _slot_index(B, f32):
    """LDS slot position (byte address >> S) of every logical tile slot, cached per tile size and precision."""
    if (B, f32) not in _ADDR:
        _ADDR[B, f32] = slot_byte(np.arange(1 << B, dtype=np.int64), f32) >> slot_shift(f32)
    return _ADDR[B, f32]


def tables(record, f32):
    """Every part record of every bank at once: off, rowoff as int64 [bank, part, 8]; coefficients as complex128 [bank, part, 32]."""
    body = np.frombuffer(record, dtype=np.uint8)[128:].reshape(MAX_BANKS, MAX_PARTS, REC_BYTES)
    words = np.ascontiguousarray(body[:, :, :64]).view("<u4").astype(np.int64)
    raw = np.ascontiguousarray(body[:, :, 64:])
    if f32:
        f = raw.view("<f4").reshape(MAX_BANKS, MAX_PARTS, 32, 4).astype(np.float64)
        cf = f[..., 0] + 1j * f[..., 1]
    else:
        cf = raw.view("<f8").reshape(MAX_BANKS, MAX_PARTS, 32, 2).copy().view(np.complex128).reshape(MAX_BANKS, MAX_PARTS, 32)
    return words[:, :, :8], words[:, :, 8:], cf


def apply(record, geom, tile, bank, order, f32, groups=None, decoded=None):
    """Runs a TOP_PART record on `tile` (2^B complex128, logical slot order) for a tile whose selector bits pick `bank`.
    An item is (part, group): the part is the top K - 3 bits of the item index, the group its low B - K bits; bit a of the item
    index walks the tile bit nibble a names, and position 15 falls off (the part bits).  Per class of the item's part record the T
    operands at base ^ off are read once and the T rows written at base ^ rowoff.
    order: "barrier" — every read of every item happens before any write (the barrier bit, or K = 3: one part); otherwise a
    sequence of part indices — each part reads all its operands and writes all its rows in place, one part after the other,
    which is what the kernel may do when no barrier separates the waves of different parts.
    groups: run these groups only (default: all 2^(B-K)); the slots of the others stay as they were.
    decoded: (header(record), tables(record, f32)) of a caller that has them already."""
    B = geom[0]
    h = header(record) if decoded is None else decoded[0]
    assert h["kind"] == TOP_PART
    K, T, S = h["nq"], h["terms"], slot_shift(f32)
    gbits = B - K
    nparts = 1 << (K - 3)
    grp = np.arange(1 << gbits, dtype=np.int64) if groups is None else np.asarray(groups, dtype=np.int64)
    where = _slot_index(B, f32)
    lds = np.empty(1 << B, dtype=np.complex128)
    lds[where] = tile
    OFF, ROWOFF, CF = tables(record, f32) if decoded is None else decoded[1]
    # where each item's group starts: bit a of the item index walks the tile bit nibble a names
    item = (np.arange(nparts, dtype=np.int64)[:, None] << gbits) | grp[None, :]
    x = np.zeros_like(item)
    for a in range(min(LANE_NIBBLES, B - 3)):
        x |= ((item >> a) & 1) << h["nibbles"][a]
    base = slot_byte(x & ((1 << B) - 1), f32)  # [part, group]; position 15 has fallen off

    def reads(p):
        off, b = OFF[bank, p], base[p]
        return {c: lds[(b[None, :] ^ off[c * T:(c + 1) * T, None]) >> S] for c in range(PART_ROWS // T) if off[c * T] != SKIP_CLASS}

    def writes(p, got):
        rowoff, cf, b = ROWOFF[bank, p], CF[bank, p], base[p]
        for c, xs in got.items():
            m = cf[c * T * T:(c + 1) * T * T].reshape(T, T)  # entry j of position c*T + i at (c*T + i) * T + j
            lds[(b[None, :] ^ rowoff[c * T:(c + 1) * T, None]) >> S] = m @ xs

    if isinstance(order, str):
        assert order == "barrier"
        held = [reads(p) for p in range(nparts)]
        for p in range(nparts):
            writes(p, held[p])
    else:
        assert sorted(order) == list(range(nparts))
        for p in order:
            writes(p, reads(p))
    return lds[where]


def apply_small(record, tile, f32):
    """The pair / quad forms of tiles of fewer than 2^3 amplitudes (TOP_G1, TOP_DIAG1, TOP_G2), bank 0: coefficients row-major in
    rec[0][0].coef; b[0], b[1] = the block's tile-local bits, ascending = bits 0, 1 of the row / column index."""
    h = header(record)
    cf = coefs(record, 0, 0, f32)
    out = np.array(tile, dtype=np.complex128)
    idx = np.arange(out.size)
    b0 = h["b"][0]
    if h["kind"] == TOP_G1:
        U = cf[:4].reshape(2, 2)
        lo, hi = tile[idx & ~(1 << b0)], tile[idx | (1 << b0)]
        r = (idx >> b0) & 1
        return U[r, 0] * lo + U[r, 1] * hi
    if h["kind"] == TOP_DIAG1:
        # (d0, d1) in the first two cells.  off[0] = 1 says d0 == 1, so only the bit = 1 half moves: the half the kernel may then
        # leave alone is multiplied by exactly 1 here, whatever the cell holds
        off, _ = offsets(record, 0, 0)
        d = np.array([1.0 if off[0] == 1 else cf[0], cf[1]])
        return d[(idx >> b0) & 1] * out
    assert h["kind"] == TOP_G2
    b1 = h["b"][1]
    U = cf[:16].reshape(4, 4)
    clear = idx & ~((1 << b0) | (1 << b1))
    r = ((idx >> b0) & 1) | (((idx >> b1) & 1) << 1)
    res = np.zeros_like(out)
    for c in range(4):
        res += U[r, c] * tile[clear | ((c & 1) << b0) | ((c >> 1) << b1)]
    return res


def dense_bank(matrix, nq, bank):
    """Bank `bank` of the block's full matrix on (selectors..., tile qubits...): the 2^nq x 2^nq diagonal block."""
    d = 1 << nq
    return matrix[bank * d:(bank + 1) * d, bank * d:(bank + 1) * d]


def apply_dense(U, geom, qubits, tile):
    """U (on `qubits`, global, most significant first) applied to the tile under the record's geometry."""
    B = geom[0]
    k = len(qubits)
    t = np.asarray(tile, dtype=np.complex128).reshape([2] * B)
    axes = [B - 1 - local_bit(geom, q) for q in qubits]
    M = np.asarray(U, dtype=np.complex128).reshape([2] * (2 * k))
    out = np.tensordot(M, t, axes=(list(range(k, 2 * k)), axes))
    out = np.moveaxis(out, list(range(k)), axes)
    return np.ascontiguousarray(out).reshape(-1)


def round32(U):
    return np.asarray(U, dtype=np.complex128).astype(np.complex64).astype(np.complex128)
