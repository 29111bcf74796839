"""The LDS table of the grouped scan's packed fp32 rows (``scan_pairs``, sphere-list kernel kind 16), as rt_plan_launch shows it.

16 bytes a padded sphere row behind the survivor queues and the fp64 planes: staged exactly when the planes are staged and the
workgroup's block stays within the 52 KB at which three workgroups share a compute unit's 160 KB (so always within 64 KB);
16-byte aligned, disjoint from queues and planes (it starts at ``lds_front_bytes`` or later) and inside ``lds_bytes``; absent for
a list whose planes do not fit and for every other kernel.  No device is needed.
"""
import numpy as np
import pytest

import raytracinginoneweekendincuda_amd as rt
from frame_helpers import render_params

QUEUES = 4 * 16 * 64 * 2          # four waves' survivor queues
SHARED, MOST, PLANES_MOST = 52 * 1024, 64 * 1024, 48 * 1024


def _list_world(n):
    s = rt.Scene()
    rnd = np.random.default_rng(n)
    items = [s.Sphere((float(rnd.uniform(-3, 3)), float(rnd.uniform(-0.4, 1.2)), float(rnd.uniform(-9, -3))), 0.2,
                      s.Lambertian((0.5, 0.5, 0.5))) for _ in range(n)]
    s.SetWorld(s.HittableList(items))
    s.Camera((0.0, 0.8, 1.0), (0.0, 0.3, -5.0), (0, 1, 0), 45, 1.5, 0.0, 10.0)
    s.Commit()
    return s


def _plan(scene, adaptive=False):
    return scene.plan_launch(render_params(96, 64, 4, pixels_per_wave=64), num_cus=256, adaptive=adaptive)


def _expected(n):
    padded = (n + 63) // 64 * 64
    planes, pairs = padded * 5 * 8, padded * 16
    staged = planes <= PLANES_MOST
    front = QUEUES + (planes if staged else 0)
    with_pairs = staged and front + pairs <= SHARED
    return staged, front, pairs, with_pairs


# 485: C2's list; 768 / 769: the last length whose block stays within the budget with the rows, and the first whose does not;
# 1216 / 1217: the planes' own cap -- the planes alone, then nothing but the queues
@pytest.mark.parametrize("n", [1, 64, 65, 485, 768, 769, 1216, 1217])
def test_scan_pairs_table_follows_the_rule(n):
    staged, front, pairs, with_pairs = _expected(n)
    for adaptive in (False, True):
        pl = _plan(_list_world(n), adaptive)
        assert pl["kernel_kind"] & 127 == 16, "the sphere-list kernel, plain or adaptive"
        offset, size = pl["lds_tables"]["scan_pairs"]
        print(f"n {n} adaptive {adaptive}: lds_bytes {pl['lds_bytes']}, front {pl['lds_front_bytes']}, scan_pairs {offset} + {size}")
        assert pl["lds_spheres"] == int(staged) and pl["lds_front_bytes"] == front
        if with_pairs:
            assert (offset, size) == (front, pairs) and offset % 16 == 0
            assert pl["lds_front_bytes"] <= offset and offset + size == pl["lds_bytes"] <= MOST
        else:
            assert offset is None and size == 0 and pl["lds_bytes"] == front


def test_the_rule_takes_both_sides_at_the_lengths_tested():
    assert {n: _expected(n)[3] for n in (485, 768, 769, 1216, 1217)} == {485: True, 768: True, 769: False, 1216: False, 1217: False}
    assert [_expected(n)[0] for n in (1216, 1217)] == [True, False]
    assert _expected(485)[1] + _expected(485)[2] == 36864 and _expected(768)[1] + _expected(768)[2] <= SHARED < MOST


def test_no_other_kernel_has_the_table():
    for scene_id, world in ((0, 0), (7, 0)):
        pl = _plan(rt.builtin_scene(scene_id, world, 96, 64))
        assert pl["kernel_kind"] & 127 != 16 and pl["lds_tables"]["scan_pairs"] == (None, 0)
