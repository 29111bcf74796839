"""The batch sizes and `alive` masks of tests/test_path_advance_scale_gpu.py, numpy alone: tests/test_path_advance_scale_host.py
checks on any machine that the family reaches every level of the compaction (csrc/advance_pack.hip), so that the GPU tests
cannot pass vacuously.  A path advance counts survivors per workgroup of 256 rows; one workgroup of 1024 threads scans those
counts 1024 a trip, each of its sixteen waves 64 of them.  Sizes are named by their workgroup count B = ceil(rows / 256)."""
import zlib

import numpy as np

ROWS = 256     # rows per workgroup of the step and of the gather
WAVE = 64      # counts per wave of the scan workgroup
TRIP = 1024    # counts per trip of the scan's loop

# one per level of the scan and each side of it: a second wave (more than 64 counts), a second trip (more than 1024), a third
# (more than 2048), and a fourth trip that ends in its second wave
SIZES = {
    "64": 64 * ROWS,
    "65": 64 * ROWS + 1,                        # one row in the last workgroup
    "1023": 1022 * ROWS + 100,                  # a partial last workgroup
    "1024": 1024 * ROWS,
    "1025": 1025 * ROWS,
    "2049": 2048 * ROWS + 255,                  # all but one row in the last workgroup
    "3137": (3 * 1024 + 64) * ROWS + 1,         # 3 * 1024 + 65 workgroups, one row in the last: 802 817 rows
}
LARGEST = max(SIZES.values())


def workgroups(rows):
    return (rows + ROWS - 1) // ROWS


def _generator(name, rows):
    return np.random.default_rng([zlib.crc32(name.encode()), rows])


def _none(rows):
    return np.zeros(rows, dtype=np.uint8)


def _at(rows, where):
    alive = _none(rows)
    where = np.asarray(where, dtype=np.int64)
    alive[where[where < rows]] = 1
    return alive


def _bernoulli(name, rows, one_in):
    return (_generator(name, rows).integers(0, one_in, size=rows) == 0).astype(np.uint8)


def _whole_waves(rows):
    """Workgroup b holds 256 survivors where b // 64 is even and none where it is odd: whole waves of the scan hold zeros between
    whole waves of 256s, and (wave 15 is odd, wave 16 even) a trip ends in zeros where the next one starts with 256s."""
    b = np.arange(rows) // ROWS
    return ((b // WAVE) % 2 == 0).astype(np.uint8)


def _one_a_workgroup(rows):
    """Workgroup b's survivor is its lane b % 256 (the last row of a partial last workgroup that has no such lane)."""
    b = np.arange(workgroups(rows))
    return _at(rows, np.minimum(b * ROWS + b % ROWS, rows - 1))


MASKS = {
    "all": lambda rows: np.ones(rows, dtype=np.uint8),
    "none": _none,
    "half": lambda rows: _bernoulli("half", rows, 2),
    "one in 64": lambda rows: _bernoulli("one in 64", rows, 64),                   # four a workgroup, a few workgroups count 0
    "one in 1024": lambda rows: _bernoulli("one in 1024", rows, 1024),             # most workgroups count 0
    "the last row": lambda rows: _at(rows, [rows - 1]),
    "the first row of the last workgroup": lambda rows: _at(rows, [(workgroups(rows) - 1) * ROWS]),
    "the first row of every trip after the first": lambda rows: _at(rows, np.arange(1, (workgroups(rows) - 1) // TRIP + 1) * TRIP * ROWS),
    "one a workgroup": _one_a_workgroup,
    "whole waves": _whole_waves,
}


def alive_of(mask, rows):
    """The `alive` array of a mask at a size: (rows,) uint8 of zeros and ones, the same at every call."""
    return MASKS[mask](rows)


def workgroup_counts(alive):
    """What the step kernel leaves the scan when every alive ray scatters: the alive rows of each workgroup of 256."""
    padded = np.zeros(workgroups(len(alive)) * ROWS, dtype=np.int64)
    padded[:len(alive)] = alive != 0
    return padded.reshape(-1, ROWS).sum(axis=1)
