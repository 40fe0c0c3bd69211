"""The measured-order table as a file (host only).  A pass over a partial support is keyed by the tile bits new to the support as
well and written as "part <new bits, hex> <the full pass's fields>"; it runs with the new bits topmost, so a line that places
them elsewhere is rejected.  Lines without the prefix — every line of a file written before partial passes were told apart — load
as orders of full passes."""
from gpu_quantum_simulator_amd import _lib


def _table(lib, path):
    assert lib.qsim_tune_table_save(path.encode()) == 0
    return sorted(l for l in open(path).read().splitlines() if l and not l.startswith("sched "))


def test_part_lines_round_trip_and_bad_ones_are_rejected(tmp_path):
    lib = _lib.load()
    src, dst = str(tmp_path / "in.txt"), str(tmp_path / "out.txt")
    hm = sum(1 << b for b in (3, 5, 7, 9, 11, 13, 15, 17, 19))
    asc = [3, 5, 7, 9, 11, 13, 15, 17, 19]
    good_full = f"20 0 12 3 {hm:x} 6.5000 7.0000 19 3 5 7 9 11 13 15 17"
    new = (1 << 9) | (1 << 17)
    placed = [b for b in asc if not (new >> b) & 1] + [9, 17]
    good_part = f"part {new:x} 20 0 12 3 {hm:x} 3.2500 3.5000 " + " ".join(map(str, placed))
    lines = [
        good_full,
        good_part,
        f"part {new:x} 20 0 12 3 {hm:x} 3.0000 3.5000 " + " ".join(map(str, asc)),           # new bits not topmost
        f"part {1 << 4:x} 20 0 12 3 {hm:x} 3.0000 3.5000 " + " ".join(map(str, asc)),          # new bit outside the set
        f"part 0 20 0 12 3 {hm:x} 3.0000 3.5000 " + " ".join(map(str, asc)),                   # no new bits: not a partial pass
        f"part {new:x} 20 0 12 3 {hm:x} 3.0000 3.5000 3 5 7 9 11 13 15 17",                    # not a permutation of the set
        "part zz",
    ]
    open(src, "w").write("\n".join(lines) + "\n")
    lib.qsim_tune_table_clear()
    try:
        assert lib.qsim_tune_table_load(src.encode()) == 2
        assert lib.qsim_tune_table_size() == 2                                                 # same bit set, two keys
        saved = _table(lib, dst)
        assert saved == sorted([good_full, good_part])
        lib.qsim_tune_table_clear()
        assert lib.qsim_tune_table_load(dst.encode()) == 2 and _table(lib, src) == saved       # what was saved loads unchanged
    finally:
        lib.qsim_tune_table_clear()


def test_a_file_without_part_lines_fills_only_full_pass_keys(tmp_path):
    lib = _lib.load()
    path = str(tmp_path / "old.txt")
    hm = sum(1 << b for b in (4, 6, 8, 10, 12, 14, 16, 18, 20))
    old = f"22 0 12 3 {hm:x} 6.5000 7.0000 20 18 16 14 12 10 8 6 4"
    open(path, "w").write(old + "\n")
    lib.qsim_tune_table_clear()
    try:
        assert lib.qsim_tune_table_load(path.encode()) == 1 and lib.qsim_tune_table_size() == 1
        assert _table(lib, path) == [old]                                                       # saved without a prefix: a full pass's order
    finally:
        lib.qsim_tune_table_clear()
