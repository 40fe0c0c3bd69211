"""The tests' own checker for permutations of basis states under controls (qsim_apply_permutation, csrc/permutation.hip,
csrc/permutation.cpp).

`apply_permutation(psi, perm, targets, controls)` is the definition, literally: inside the subspace where every control bit is 1,
gather the 2^k amplitudes of every environment (bit j of a table index is qubit targets[j]), index, scatter:
new[e | dep(perm[j])] = old[e | dep(j)].  Everything else keeps its bits; nothing is computed, so the dtype's bits move as they are.

`walk_tiles` restates what the kernel does with the plan and the operand the library reports (plans.apply_permutation_plan,
plans.apply_permutation_operand): tile by tile, amplitudes move inside the tile by the tile-local map."""
import numpy as np


def deposit(v, bits):
    """bit j of v -> index bit bits[j]"""
    return sum(((v >> j) & 1) << b for j, b in enumerate(bits))


def deposit_all(count_bits, bits):
    """deposit(v, bits) for every v in range(2**count_bits), as an int64 array"""
    v = np.arange(1 << count_bits, dtype=np.int64)
    out = np.zeros_like(v)
    for j, b in enumerate(bits):
        out |= ((v >> j) & 1) << b
    return out


def apply_permutation(psi, perm, targets, controls=()):
    """A new array of psi's dtype: basis state j of `targets` moved to perm[j] where all `controls` are 1."""
    out = np.array(psi, copy=True).reshape(-1)
    n = int(out.size).bit_length() - 1
    targets, controls = list(targets), list(controls)
    k = len(targets)
    perm = np.asarray(perm, dtype=np.int64).reshape(1 << k)
    env = [q for q in range(n) if q not in targets and q not in controls]
    ones = sum(1 << q for q in controls)
    rows = deposit_all(k, targets)
    cols = deposit_all(len(env), env) | ones
    idx = rows[:, None] | cols[None, :]                          # (2^k, environments)
    old = out[idx]                                               # gather
    out[idx[perm]] = old                                         # row j lands in row perm[j]: index, scatter
    return out


def permutation_matrix(perm):
    """U with U[perm[j], j] = 1: what apply_matrix takes for the same map."""
    perm = np.asarray(perm, dtype=np.int64)
    U = np.zeros((perm.size, perm.size), dtype=np.complex128)
    U[perm, np.arange(perm.size)] = 1.0
    return U


def walk_tiles(psi, tile_mask, controls, local_map):
    """The kernel's walk: for every tile base (the bits outside `tile_mask` and outside the controls, the controls all 1) the element
    at tile-local index u (bit i of u is the i-th lowest bit of tile_mask) moves to tile-local index local_map[u]."""
    out = np.array(psi, copy=True).reshape(-1)
    n = int(out.size).bit_length() - 1
    tile_bits = [q for q in range(n) if tile_mask >> q & 1]
    controls = list(controls)
    rest = [q for q in range(n) if q not in tile_bits and q not in controls]
    ones = sum(1 << q for q in controls)
    local_map = np.asarray(local_map, dtype=np.int64)
    assert local_map.size == 1 << len(tile_bits)
    inside = deposit_all(len(tile_bits), tile_bits)
    bases = deposit_all(len(rest), rest) | ones
    src = bases[:, None] | inside[None, :]                       # (tiles, 2^B)
    dst = bases[:, None] | inside[local_map][None, :]
    out[dst] = np.asarray(psi).reshape(-1)[src]
    return out
