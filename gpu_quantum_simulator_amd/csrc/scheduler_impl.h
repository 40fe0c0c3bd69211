// scheduler_impl.h — the few helpers fusion.cpp, tile_block.cpp and pass_builder.cpp share.  Nothing else includes it, and the
// namespace has hidden visibility: libqsim.so exports none of it.
#ifndef QSIM_SCHEDULER_IMPL_H
#define QSIM_SCHEDULER_IMPL_H

#include "scheduler.h"

namespace qsim {
namespace sched __attribute__((visibility("hidden"))) {

inline bool is_zero(const cd &z) { return z.real() == 0.0 && z.imag() == 0.0; }
inline bool is_one(const cd &z) { return z.real() == 1.0 && z.imag() == 0.0; }

// fusion.cpp: a fused op of `kind` on (q_hi[, q_lo]) with the 2x2 / 4x4 matrix m (nullptr: left zero, as for a CX)
FusedOp make_op(int kind, int q_hi, int q_lo, const cd *m, uint32_t gates = 1);

// tile_block.cpp: a fused op (1 or 2 qubits at level 3) split by the tile: qubits in `inside` stay matrix indices, the others
// become bank selectors.  The op must be block-diagonal in every qubit left outside.
TileBlock to_block(const FusedOp &op, uint64_t inside);

} // namespace sched
} // namespace qsim
#endif
