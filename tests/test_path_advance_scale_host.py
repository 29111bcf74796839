"""The sizes and masks of tests/test_path_advance_scale_gpu.py reach every level of the compaction's scan (csrc/advance_pack.hip):
checked in numpy on the workgroup counts the masks give where every alive ray scatters.  No GPU and no library is needed."""
import numpy as np

from advance_scale_masks import MASKS, ROWS, SIZES, TRIP, WAVE, alive_of, workgroup_counts, workgroups


def test_the_sizes_are_the_workgroup_counts_their_names_say():
    assert {name: workgroups(rows) for name, rows in SIZES.items()} == {name: int(name) for name in SIZES}
    assert sorted(int(name) for name in SIZES) == [64, 65, 1023, 1024, 1025, 2049, 3 * 1024 + 65]
    assert SIZES["1023"] % ROWS not in (0, 1) and SIZES["3137"] == 802817 and SIZES["3137"] % ROWS == 1


def test_the_masks_reach_every_level():
    seen = set()
    for size, rows in SIZES.items():
        for mask in MASKS:
            alive = alive_of(mask, rows)
            assert alive.shape == (rows,) and alive.dtype == np.uint8 and alive.max(initial=0) <= 1, (size, mask)
            assert np.array_equal(alive, alive_of(mask, rows)), "the same mask at every call"
            counts = workgroup_counts(alive)
            n = len(counts)
            assert n == workgroups(rows) and counts.sum() == alive.sum()
            b = np.flatnonzero(counts)
            if ((b % TRIP) // WAVE != 0).any():
                seen.add("a non-zero count in a scan wave other than wave 0")
            if (b >= TRIP).any():
                seen.add("a non-zero count in a trip other than trip 0")
            if n % WAVE and counts[n - n % WAVE:].any():
                seen.add("a trip whose last wave is partial")
            trips = [counts[t:t + TRIP] for t in range(0, n, TRIP)]
            if any(not trips[t].any() and trips[t + 1].any() for t in range(len(trips) - 1)):
                seen.add("a trip of all zeros followed by a non-zero trip")
            for boundary in (WAVE, TRIP):
                for at in range(boundary, n, boundary):
                    if boundary == WAVE and at % TRIP == 0:
                        continue   # (a wave boundary inside a trip)
                    if {int(counts[at - 1]), int(counts[at])} == {0, ROWS}:
                        seen.add(f"a workgroup count of 256 and one of 0 adjacent across a {boundary} boundary")
            if counts.sum() == 0:
                seen.add("a total of 0")
            if counts.sum() == rows:
                seen.add("a total equal to the capacity")
    assert seen == {
        "a non-zero count in a scan wave other than wave 0", "a non-zero count in a trip other than trip 0",
        "a trip whose last wave is partial", "a trip of all zeros followed by a non-zero trip",
        "a workgroup count of 256 and one of 0 adjacent across a 64 boundary",
        "a workgroup count of 256 and one of 0 adjacent across a 1024 boundary", "a total of 0", "a total equal to the capacity"}


def test_every_size_meets_every_mask_it_can():
    """Per size, so that trimming the list of sizes is noticed too: every size has both totals, the single survivors where their names
    say, and the whole waves of zeros before a trip that starts with survivors."""
    for size, rows in SIZES.items():
        counts = {mask: workgroup_counts(alive_of(mask, rows)) for mask in MASKS}
        n = workgroups(rows)
        assert counts["all"].sum() == rows and counts["none"].sum() == 0
        assert counts["one a workgroup"].tolist() == [1] * n, size
        assert counts["the last row"].tolist() == [0] * (n - 1) + [1] and counts["the first row of the last workgroup"].tolist() == [0] * (n - 1) + [1]
        assert counts["one in 64"].sum() > 0 and 2 * (counts["one in 1024"] == 0).sum() > n and counts["one in 1024"].sum() > 0
        assert counts["the first row of every trip after the first"].sum() == (n - 1) // TRIP
        if n > 2 * WAVE:
            assert counts["half"][WAVE:].any() and counts["one in 64"][WAVE:].any()
        if n > TRIP:
            assert set(counts["whole waves"][TRIP - WAVE:TRIP]) == {0} and counts["whole waves"][TRIP] in (ROWS, rows - TRIP * ROWS)
