"""The sharding handles over the C ABI: `Cluster` (P shards driven by one process), `ShardPlanHandle` (the C++ planner's output) and
`RankComm` (one rank's end of the exchanges in a one-process-per-GPU job)."""
from __future__ import annotations

import ctypes
from ctypes import byref, c_double, c_int, c_uint64, c_void_p
from typing import Optional, Sequence

import numpy as np

from . import _lib, _marshal
from ._lib import check, check_cluster
from ._marshal import dp as _dp
from .circuit import Circuit
from .pauli_args import _PauliStrings


class Cluster(_PauliStrings, _lib.Handle):
    """qsim_cluster: P shards driven by this one process (the C host's multi-GPU path; repeat a device for virtual shards)."""
    _expect_fn, _rotate_fn, _check = "qsim_cluster_expect_paulis", "qsim_cluster_apply_pauli_rotations", staticmethod(check_cluster)
    _free = "qsim_cluster_destroy"

    def __init__(self, num_q: int, num_shards: int, devices: Optional[Sequence[int]] = None, **options):
        self._h = c_void_p()
        lib = _lib.load()
        arr = (c_int * num_shards)(*devices) if devices is not None else None
        check_cluster(lib.qsim_cluster_create(byref(self._h), num_q, num_shards, arr))
        self.num_qubits, self.num_shards = num_q, num_shards
        names = {"fuse": _lib.OPT_FUSE, "tile_bits": _lib.OPT_TILE_BITS, "tile_low_bits": _lib.OPT_TILE_LOW_BITS,
                 "tile_max_ops": _lib.OPT_TILE_MAX_OPS, "profile": _lib.OPT_PROFILE, "pingpong": _lib.OPT_PINGPONG,
                 "affine_support": _lib.OPT_AFFINE_SUPPORT}
        for key in sorted(options, key=lambda k: k != "tile_low_bits"):
            self._check(lib.qsim_cluster_set_option(self._h, names[key], int(options[key])))

    def run(self, circuit: Circuit) -> None:
        lib = _lib.load()
        self._check(lib.qsim_cluster_reset(self._h))
        self._check(lib.qsim_cluster_run_circuit(self._h, circuit._h))
        self._check(lib.qsim_cluster_sync(self._h))

    def plan(self, circuit: Circuit, max_candidates: int = 1, budget_ms: float = 0.0) -> None:
        """qsim_cluster_plan: schedule choice (and, with max_candidates > 1, measured tile-bit orders) for every shard's local steps."""
        self._check(_lib.load().qsim_cluster_plan(self._h, circuit._h, max_candidates, budget_ms))

    def read(self, first: int = 0, count: Optional[int] = None) -> np.ndarray:
        if count is None:
            count = (1 << self.num_qubits) - first
        out = np.empty(2 * count, dtype=np.float64)
        self._check(_lib.load().qsim_cluster_read(self._h, first, count, _dp(out)))
        return out.view(np.complex128)

    def norm2(self) -> float:
        v = c_double()
        self._check(_lib.load().qsim_cluster_norm2(self._h, byref(v)))
        return v.value

    def sample(self, randoms) -> np.ndarray:
        """measurement() (quantum_simulator.c:270-283) on the sharded state, indices in logical order."""
        r = np.ascontiguousarray(randoms, dtype=np.float64)
        out = np.zeros(r.size, dtype=np.uint64)
        self._check(_lib.load().qsim_cluster_sample(self._h, _dp(r), r.size, _marshal.u64p(out)))
        return out

    def exchange_stats(self):
        n, b = c_uint64(), c_double()
        _lib.load().qsim_cluster_exchange_stats(self._h, byref(n), byref(b))
        return int(n.value), float(b.value)

    def pack_counts(self):
        """(re-layouts done by the last tile pass in front of an exchange, by the separate pack kernel) per shard and exchange."""
        a, b = c_uint64(), c_uint64()
        _lib.load().qsim_cluster_pack_counts(self._h, byref(a), byref(b))
        return int(a.value), int(b.value)

    def exchange_bytes_moved(self) -> float:
        """Bytes all shards together really sent (blocks of / for shards that hold nothing stay home)."""
        b = c_double()
        _lib.load().qsim_cluster_exchange_bytes_moved(self._h, byref(b))
        return float(b.value)

    @property
    def exchange_mode(self) -> str:
        """"rccl" | "direct" | "copies" | "none" (qsim_cluster_exchange_mode)."""
        return (_lib.load().qsim_cluster_exchange_mode(self._h) or b"").decode()


class ShardPlanHandle(_lib.Handle):
    """qsim_shard_plan: the C++ planner's output for one circuit and shard count (host only)."""
    _free = "qsim_shard_plan_free"

    def __init__(self, circuit: Circuit, num_shards: int):
        self._h = c_void_p()
        lib = _lib.load()
        check_cluster(lib.qsim_shard_plan_create(byref(self._h), circuit._h, num_shards))
        self.num_shards = num_shards
        self.num_qubits = circuit.num_qubits
        self.num_steps = lib.qsim_shard_plan_num_steps(self._h)

    def step(self, i: int):
        """("local",) or ("exchange", shard_bits, local_positions)."""
        kind, k = c_int(), c_int()
        J, L = (c_int * 16)(), (c_int * 16)()
        check(_lib.load().qsim_shard_plan_step(self._h, i, byref(kind), byref(k), J, L))
        if kind.value == 0:
            return ("local",)
        return ("exchange", tuple(J[: k.value]), tuple(L[: k.value]))

    def local_ops(self, i: int, shard: int) -> list:
        """[("u1", pos, U) | ("cx", a, b) | ("scale", z)] for one shard."""
        out = []

        def cb(_u, kind, a, b, m):
            if kind == 1:
                out.append(("u1", a, np.ctypeslib.as_array(m, shape=(8,)).copy().view(np.complex128).reshape(2, 2)))
            elif kind == 2:
                out.append(("cx", a, b))
            else:
                out.append(("scale", complex(m[0], m[1])))

        check(_lib.load().qsim_shard_plan_local_ops(self._h, i, shard, _lib.LOCAL_OP_CB(cb), None))
        return out

    def apply_local(self, i: int, shard: int, sim: "Simulator") -> None:
        check_cluster(_lib.load().qsim_shard_plan_apply_local(self._h, i, shard, sim._h))

    def step_support(self, i: int):
        """(mixed_local, mixed_rank) of an exchange step: where the register can be non-zero just before it."""
        a, b = c_uint64(), c_uint64()
        check(_lib.load().qsim_shard_plan_step_support(self._h, i, byref(a), byref(b)))
        return int(a.value), int(b.value)

    def exchange_roles(self, i: int, shard: int) -> dict:
        """qsim_shard_plan_exchange_roles: what one shard sends, receives and holds afterwards in the exchange of step i."""
        r = _lib.QsimExchangeRoles()
        check(_lib.load().qsim_shard_plan_exchange_roles(self._h, i, shard, byref(r)))
        return r.as_dict()

    def final_pos(self) -> list:
        pos = (c_int * self.num_qubits)()
        check(_lib.load().qsim_shard_plan_final_pos(self._h, pos))
        return list(pos)

    def tune(self, shard: int, sim: "Simulator", max_candidates: int = 32, budget_ms: float = 6000.0) -> dict:
        """qsim_shard_plan_tune: geometry planning for one shard's local steps (leaves `sim` reset)."""
        rep = _lib.QsimTuneReport()
        check_cluster(_lib.load().qsim_shard_plan_tune(self._h, shard, sim._h, max_candidates, budget_ms, byref(rep)))
        return rep.as_dict()

    def predict(self, link_gbps: float = 50.0, pack_gbps: float = 5000.0):
        """(bytes each rank sends, seconds spent in exchanges) under the planner's cost model (qsim_shard_plan_predict)."""
        b, t = c_double(), c_double()
        check(_lib.load().qsim_shard_plan_predict(self._h, link_gbps, pack_gbps, byref(b), byref(t)))
        return b.value, t.value


class RankComm(_lib.Handle):
    """qsim_rank_comm: this rank's end of the exchanges in a one-process-per-GPU job — RCCL send/recv issued by libqsim
    on the shard's own stream.  `unique_id()` (rank 0) produces the bytes every rank passes to the constructor."""
    _free = "qsim_rank_comm_destroy"

    @staticmethod
    def unique_id() -> bytes:
        buf = ctypes.create_string_buffer(128)
        check_cluster(_lib.load().qsim_rccl_unique_id(buf))
        return buf.raw

    def __init__(self, sim: "Simulator", device: int, world: int, rank: int, uid: bytes, scratch_ptr: Optional[int] = None):
        self._h = c_void_p()
        lib = _lib.load()
        buf = ctypes.create_string_buffer(bytes(uid), 128)
        check_cluster(lib.qsim_rank_comm_create(byref(self._h), sim._h, device, world, rank, buf,
                                       c_void_p(scratch_ptr) if scratch_ptr else None))

    def exchange(self, shard_bits: Sequence[int], local_bits: Sequence[int]) -> None:
        k = len(shard_bits)
        check_cluster(_lib.load().qsim_rank_comm_exchange(self._h, _marshal.ints(shard_bits), _marshal.ints(local_bits), k))

    def exchange_step(self, plan: "ShardPlanHandle", step: int) -> None:
        """qsim_rank_comm_exchange_step: the exchange of one plan step, leaving out what the plan knows to be zero."""
        check_cluster(_lib.load().qsim_rank_comm_exchange_step(self._h, plan._h, step))

    def loopback(self, count: int) -> None:
        """`count` doubles of the shard through ncclSend -> ncclRecv to this same rank (qsim_rank_comm_loopback)."""
        check_cluster(_lib.load().qsim_rank_comm_loopback(self._h, count))

    def pack_counts(self):
        """(re-layouts done by the last tile pass in front of an exchange, by the separate pack kernel)."""
        a, b = c_uint64(), c_uint64()
        _lib.load().qsim_rank_comm_pack_counts(self._h, byref(a), byref(b))
        return int(a.value), int(b.value)

    def stats(self, reset: bool = False):
        """(exchanges, bytes sent by this rank, seconds its stream spent in exchanges)."""
        n, b, t = c_uint64(), c_double(), c_double()
        check_cluster(_lib.load().qsim_rank_comm_stats(self._h, byref(n), byref(b), byref(t), 1 if reset else 0))
        return int(n.value), float(b.value), float(t.value)
