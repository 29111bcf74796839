"""Every LDS-staged table rendered from both sides of its cap.

launch_plan.cpp lds_layout decides per launch and per table whether a BVH kernel reads its rows from LDS or from global
memory, and every accessor of render.hip has both sides as a run-time branch.  The cases (test_lds_layout.staging_cases, which
test_lds_layout proves to reach both sides of every table in every kernel that has the choice) are pairs of scenes that
differ in the rows of one table only, one at the cap and one past it, through kinds 2, 6, 7, 39 and the 768-thread kernels;
node rows at 853 nodes (61 416 B: more dynamic LDS than a launch gets without asking) and past them; and the crowded layouts
of 727 nodes in which placement stops partway.  96 x 64, 4 samples, depth 50, both builds, plain and through the Adaptive<>
instantiation.  References: the CPU oracle on the same scene (conftest.build_both) and, for the fast build of media-free
scenes, the same items as a HittableList world, whose kernels read every table from global memory."""
import numpy as np
import pytest
import torch

import raytracinginoneweekendincuda_amd as rt
import test_lds_layout as L
from conftest import build_both
from frame_helpers import compare
from query_helpers import bits

pytestmark = pytest.mark.gpu

W, H, SPP = L.W, L.H, L.SPP


@pytest.mark.parametrize("case", L.staging_cases(), ids=L.CASE_IDS)
def test_frames_do_not_depend_on_which_side_a_table_lies(case):
    """Per case, both builds, plain and adaptive (min_samples = the cap = 4, an interval of 1: the only check point is the cap, so
    the Adaptive<> instantiation must give the plain frame bit for bit):
      * what ran is what was planned (kernel kind, LDS bytes, pixels per wave), and the planned side of the case's table is
        the one the case claims;
      * strict build: frame and ray count equal the oracle's bit for bit; the scenes of the Perlin pair evaluate device sin,
        which differs from glibc's by an ulp in a few pixels: the bar of test_deep_kernel_falls_back_when_its_tables_do_not_fit;
      * fast build: the bar of test_custom_scenes_gpu.check against the oracle, and for media-free scenes bit-identity with
        the list world of the same items in the same build (the invariant of ..._bvh_world_equals_list_world_bitwise)."""
    name, table, n, mode, fillers, flags, side = case
    num_cus = torch.cuda.get_device_properties(0).multi_processor_count
    prod, orc = build_both(L.case_build(case))
    want, stats = orc.render(W, H, SPP, want_stats=True)
    perlin, media = stats["noise_calls"] > 0, stats["medium_calls"] > 0
    assert perlin == (table == "perlin")
    for variant in (0, 1):
        frames = []
        for adaptive in (False, True):
            film = rt.Film(W, H)
            if adaptive:
                film.set_adaptive(SPP, 1, 0.05)
            params = film.params(SPP, variant=variant, flags=flags)
            pl = prod.plan_launch(params, num_cus=num_cus, adaptive=adaptive)
            film.launch(prod, params)
            st = film.finish(prod)
            got = film.download()
            exact, within, worst = compare(got, want)
            print(f"{name} variant {variant} adaptive {adaptive}: kind {st.kernel_kind}, {st.lds_bytes} B LDS ({pl['lds_front_bytes']} in front), "
                  f"{st.kernel_vgprs} VGPRs, rays {st.rays} / {stats['rays']}, bit-exact {exact:.4f}, within {within:.4f}, max |d| {worst:.3g}; "
                  f"global: {sorted(t for t, s in L.sides(pl).items() if not s)}")
            assert (st.kernel_kind, st.lds_bytes, st.pixels_per_wave) == (pl["kernel_kind"], pl["lds_bytes"], pl["pixels_per_wave"])
            assert st.kernel_kind == (pl["kernel_kind"] & ~L.ADAPTIVE) + (L.ADAPTIVE if adaptive else 0)
            assert L.label(pl) == {"deep": "deep7" if flags else 263}.get(mode, mode)
            assert L.staged(pl, table) == side
            assert np.isfinite(got).all()
            frames.append((got, st))
        (plain, st), (adapt, st_adapt) = frames
        assert st.rays == st_adapt.rays and np.array_equal(bits(plain), bits(adapt)), (name, variant, "adaptive frame differs")
        exact, within, worst = compare(plain, want)
        if variant == 0:
            assert st.rays == stats["rays"], "ray counter differs from the oracle's RayColor iterations"
            if perlin:
                assert within >= 0.999 and exact >= 0.95
            else:
                assert np.array_equal(bits(plain), bits(want)), (name, exact, within, worst)
        else:
            assert within >= 0.995
            if not media:
                twin = L.product(L.case_build(case, world="list"))
                lst, st_lst = twin.render(W, H, SPP, variant=variant, flags=flags)
                print(f"{name} variant {variant}: list world kind {st_lst.kernel_kind}, rays {st_lst.rays}, "
                      f"pixels equal {np.mean(np.all(bits(lst) == bits(plain), axis=-1)):.4f}")
                assert st_lst.kernel_kind & 8 or st_lst.kernel_kind & 16, st_lst.kernel_kind   # a list kernel: every table from global memory
                assert st_lst.rays == st.rays
                assert np.array_equal(bits(lst), bits(plain)), (name, "BVH world and list world differ in the fast build")
