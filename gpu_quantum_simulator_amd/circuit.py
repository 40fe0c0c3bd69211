"""`Circuit` = qsim_circuit (the tokenizer of quantum_simulator.c:115-254 and the gate table :184-211), with the host-only probes of
its schedule: plan, passes, regions, plan_choice, schedule, tile_records."""
from __future__ import annotations

import ctypes
from ctypes import byref, c_double, c_int, c_uint64, c_void_p
from typing import Iterable, Optional, Sequence

import numpy as np

from . import _lib
from ._lib import QsimStats, check
from ._marshal import dp as _dp, mat as _mat


def gate_matrix(token: str) -> Optional[np.ndarray]:
    """2x2 for a gate token of the reference's vocabulary (None for cx / unknown)."""
    u = np.zeros(8)
    kind = _lib.load().qsim_gate_matrix(token.encode(), _dp(u))
    return u.view(np.complex128).reshape(2, 2).copy() if kind == _lib.GATE_U1 else None


class Circuit(_lib.Handle):
    _free = "qsim_circuit_free"

    def __init__(self, handle: c_void_p):
        self._h = handle

    @classmethod
    def empty(cls, num_q: int) -> "Circuit":
        h = c_void_p()
        check(_lib.load().qsim_circuit_create(num_q, byref(h)))
        return cls(h)

    @classmethod
    def from_file(cls, path: str) -> "Circuit":
        h = c_void_p()
        rc = _lib.load().qsim_circuit_parse_file(path.encode(), byref(h))
        if rc:
            raise _lib.QsimError(rc, (_lib.load().qsim_circuit_error() or b"").decode())
        return cls(h)

    @classmethod
    def from_text(cls, text: str) -> "Circuit":
        h = c_void_p()
        raw = text.encode()
        rc = _lib.load().qsim_circuit_parse_text(raw, len(raw), byref(h))
        if rc:
            raise _lib.QsimError(rc, (_lib.load().qsim_circuit_error() or b"").decode())
        return cls(h)

    @classmethod
    def from_gates(cls, num_q: int, gates: Iterable[Sequence]) -> "Circuit":
        """gates in the tuple form of circuits.random_gates."""
        c = cls.empty(num_q)
        cache = {}
        for g in gates:
            if g[0] == "cx":
                c.append_cx(g[1], g[2])
            elif g[0] == "rz":
                c.append_1q(gate_matrix(f"rz({g[1]!r})"), g[2])
            else:
                if g[0] not in cache:
                    cache[g[0]] = gate_matrix(g[0])
                c.append_1q(cache[g[0]], g[1])
        return c

    def append_1q(self, U, target: int) -> None:
        check(_lib.load().qsim_circuit_append_1q(self._h, _dp(_mat(U, 2)), target))

    def append_cx(self, control: int, target: int) -> None:
        check(_lib.load().qsim_circuit_append_cx(self._h, control, target))

    def append_2q(self, U, q_hi: int, q_lo: int) -> None:
        check(_lib.load().qsim_circuit_append_2q(self._h, _dp(_mat(U, 4)), q_hi, q_lo))

    @property
    def num_qubits(self) -> int:
        return _lib.load().qsim_circuit_num_qubits(self._h)

    def __len__(self) -> int:
        return int(_lib.load().qsim_circuit_num_gates(self._h))

    def gate(self, i: int):
        kind, q0, q1 = c_int(), c_int(), c_int()
        u = np.zeros(32)
        check(_lib.load().qsim_circuit_gate(self._h, i, byref(kind), byref(q0), byref(q1), _dp(u)))
        if kind.value == _lib.GATE_U1:
            return ("u1", q0.value, u[:8].view(np.complex128).reshape(2, 2).copy())
        if kind.value == _lib.GATE_CX:
            return ("cx", q0.value, q1.value)
        return ("u2", q0.value, q1.value, u.view(np.complex128).reshape(4, 4).copy())

    def plan(self, fuse: int = 3, tile_bits: int = 12, tile_low_bits: int = 3, initial_support: int = 0) -> dict:
        """Launches and algorithmic bytes of the schedule (host only).  initial_support: index bits that may be 1 in the state
        the circuit finds (0: fresh from a reset; all ones: dense)."""
        st = QsimStats()
        check(_lib.load().qsim_plan_circuit_from(self._h, fuse, tile_bits, tile_low_bits, initial_support, byref(st)))
        return st.as_dict()

    def passes(self, fuse: int = 3, tile_bits: int = 12, tile_low_bits: int = 3, initial_support: int = 0) -> list:
        """qsim_plan_passes: the schedule pass by pass (host only) — kernel class, blocks, the index bits inside the tile, the
        fraction of the register visited, algorithmic bytes and the bytes-equivalent of the pass-time model."""
        cap = 4096
        buf = (_lib.QsimPassInfo * cap)()
        n = c_int()
        check(_lib.load().qsim_plan_passes(self._h, fuse, tile_bits, tile_low_bits, initial_support, buf, cap, byref(n)))
        return [{"kernel": _lib.K_NAMES[buf[i].kernel_class], "blocks": int(buf[i].blocks), "tile_mask": int(buf[i].tile_mask),
                 "visited": float(buf[i].visited), "bytes": float(buf[i].bytes), "cost_bytes": float(buf[i].cost_bytes)}
                for i in range(min(n.value, cap))]

    def regions(self, fuse: int = 3, tile_bits: int = 12, tile_low_bits: int = 3, tile_max_ops: int = 32, initial_support: int = 0,
                defer: bool = False, setting: dict = None) -> list:
        """qsim_plan_regions: per pass of schedule() with the same arguments (defer: of schedule(flips=[])) what
        QSIM_OPT_AFFINE_SUPPORT adds — the tiles to visit (origin, gen), the parity checks of the region the previous pass wrote
        as (mask, parity) pairs, and the shares of the register written and read.  setting: of schedule(setting=...)."""
        cap = 4096
        buf = (_lib.QsimPassRegion * cap)()
        n = c_int()
        if setting is not None:
            if fuse != 3 or defer:
                raise ValueError("regions: a setting goes with fuse=3 and states its own defer")
            check(_lib.load().qsim_plan_regions_with(self._h, tile_bits, tile_low_bits, tile_max_ops, initial_support,
                                                     byref(_lib.QsimSchedSetting.of(setting)), buf, cap, byref(n)))
        else:
            check(_lib.load().qsim_plan_regions(self._h, fuse, tile_bits, tile_low_bits, tile_max_ops, initial_support, int(bool(defer)), buf, cap, byref(n)))
        return [{"kernel": _lib.K_NAMES[r.kernel_class], "on": bool(r.on), "refined": bool(r.refined), "tile_mask": int(r.tile_mask),
                 "support_before": int(r.support_before), "origin": int(r.origin), "gen": [int(r.gen[j]) for j in range(r.n_gen)],
                 "checks": [(int(r.check_mask[j]), int(r.check_parity >> j & 1)) for j in range(r.n_checks)],
                 "visited": float(r.visited), "read_share": float(r.read_share)}
                for r in (buf[i] for i in range(min(n.value, cap)))]

    def plan_choice(self, tile_bits: int = 12, tile_low_bits: int = 3, tile_max_ops: int = 32, initial_support: int = 0, f32: bool = False,
                    with_defer: bool = True) -> dict:
        """qsim_plan_choice: what the planning step's model would choose for this circuit (host only) — every candidate setting in
        candidate order with its price ("candidates"), the index of the choice ("chosen") and the host seconds of the ranking."""
        cap = 4096
        buf = (_lib.QsimSchedSetting * cap)()
        n, chosen, seconds = c_int(), c_int(), c_double()
        check(_lib.load().qsim_plan_choice(self._h, tile_bits, tile_low_bits, tile_max_ops, initial_support, int(bool(f32)), int(bool(with_defer)),
                                           buf, cap, byref(n), byref(chosen), byref(seconds)))
        return {"candidates": [buf[i].as_dict() for i in range(min(n.value, cap))], "chosen": chosen.value, "seconds": seconds.value}

    def schedule(self, fuse: int = 3, tile_bits: int = 12, tile_low_bits: int = 3, tile_max_ops: int = 32, flips: list = None,
                 initial_support: int = 0, setting: dict = None) -> list:
        """Fused blocks in launch order: (pass, kernel_class, kind, qubits, matrix|None, gates_folded); kind is
        "u1" / "cx" / "u2" ... "u8", qubits most significant first (cx: control, target).  flips: a list — the schedule with
        the X gates deferred (qsim_schedule_circuit_deferred); the residual index mask is appended to it.  initial_support
        (without flips): the index bits that may be 1 in the state the circuit finds (qsim_schedule_circuit_from).  setting: a
        candidate of the planning step as a dict (fields of qsim_sched_setting; those left out are the options' own) — the level-3
        schedule under it (qsim_schedule_circuit_with); where it defers, pass flips=[] to receive the mask."""
        out = []

        def cb(_user, pass_i, kclass, kind, qubits, nq, U, folded):
            qs = tuple(qubits[i] for i in range(nq))
            m = None
            if kind != _lib.GATE_CX:
                d = 1 << nq
                m = np.ctypeslib.as_array(U, shape=(2 * d * d,)).copy().view(np.complex128).reshape(d, d)
            out.append((pass_i, _lib.K_NAMES[kclass], {1: "u1", 2: "cx", 3: "u2", 4: "u3", 5: "u4", 6: "u5", 7: "u6", 8: "u7", 9: "u8"}[kind], qs, m, folded))

        if setting is not None:
            if fuse != 3 or (flips is None) != (not setting.get("defer")):
                raise ValueError("schedule: a setting goes with fuse=3, and with flips=[] exactly when it defers")
            mask = c_uint64()
            check(_lib.load().qsim_schedule_circuit_with(self._h, tile_bits, tile_low_bits, tile_max_ops, initial_support,
                                                         byref(_lib.QsimSchedSetting.of(setting)), _lib.SCHED_CB(cb), None, byref(mask)))
            if flips is not None:
                flips.append(int(mask.value))
            return out
        if flips is None:
            check(_lib.load().qsim_schedule_circuit_from(self._h, fuse, tile_bits, tile_low_bits, tile_max_ops, initial_support, _lib.SCHED_CB(cb), None))
            return out
        if initial_support:
            raise ValueError("schedule: initial_support goes with flips=None")
        mask = c_uint64()
        check(_lib.load().qsim_schedule_circuit_deferred(self._h, fuse, tile_bits, tile_low_bits, tile_max_ops, _lib.SCHED_CB(cb), None,
                                                         byref(mask)))
        flips.append(int(mask.value))
        return out

    def tile_records(self, fuse: int = 3, tile_bits: int = 12, tile_low_bits: int = 3, tile_max_ops: int = 32, f32: bool = False,
                     order_seed: int = 0) -> list:
        """qsim_tile_records: every block of every tile pass of the schedule() with the same arguments, as a dict: pass,
        tile_bits, low_bits, high (global bit of each high tile-local bit, in order), selectors and qubits (most significant
        first), matrix (on selectors + qubits) and record, the encoded TileOp as bytes.  order_seed != 0 shuffles each pass's
        high bits before encoding.  Host only."""
        out = []

        def cb(_user, pass_i, geom, high, sel, nsel, tq, nq, U, record, nbytes):
            d = 1 << (nsel + nq)
            out.append({"pass": pass_i, "tile_bits": geom[0], "low_bits": geom[1], "high": tuple(high[j] for j in range(geom[2])),
                        "selectors": tuple(sel[a] for a in range(nsel)), "qubits": tuple(tq[a] for a in range(nq)),
                        "matrix": np.ctypeslib.as_array(U, shape=(2 * d * d,)).copy().view(np.complex128).reshape(d, d),
                        "record": ctypes.string_at(record, nbytes)})

        check(_lib.load().qsim_tile_records(self._h, fuse, tile_bits, tile_low_bits, tile_max_ops, int(bool(f32)), order_seed,
                                            _lib.TILE_RECORD_CB(cb), None))
        return out
