"""What ran is what was planned: rt_render_stats of a launch against rt_plan_launch for the same params and the GPU's own
number of compute units -- the three scenes of smoke(), a sphere list and a library-tree world at a frame size that takes the
rehearsal, the classes and the serving waves.  tests/test_launch_plan.py checks the plan itself, without a GPU."""
import os

import numpy as np
import pytest
import torch

import raytracinginoneweekendincuda_amd as rt

pytestmark = pytest.mark.gpu

CASES = [  # scene, world, W, H, spp, render keywords
    (0, 0, 48, 24, 2, {}), (7, 0, 48, 24, 2, {}), (9, 0, 48, 24, 2, {}),
    (11, 1, 512, 256, 64, {}), (0, 0, 512, 256, 64, {}),
    (7, 1, 48, 24, 2, dict(pixels_per_wave=12)), (11, 1, 48, 24, 2, dict(pixels_per_wave=12, flags=rt.FLAG_ACCELERATE_LISTS)),
]


@pytest.mark.parametrize("scene_id,world,w,h,spp,kw", CASES)
def test_stats_equal_the_plan(scene_id, world, w, h, spp, kw):
    earth = np.load(os.path.join(os.path.dirname(__file__), "golden", "earthmap_stb.npz"))["bytes"] if scene_id == 9 else None
    num_cus = torch.cuda.get_device_properties(0).multi_processor_count
    scene = rt.builtin_scene(scene_id, world, w, h, earth=earth)
    for variant in (0, 1):
        for adaptive in (False, True):
            film = rt.Film(w, h)
            if adaptive:
                film.set_adaptive(8, 8, 0.05)
            params = film.params(spp, variant=variant, **kw)
            plan = scene.plan_launch(params, num_cus=num_cus, adaptive=adaptive)
            film.launch(scene, params)
            st = film.finish(scene)
            print(f"scene {scene_id} world {world} variant {variant} adaptive {adaptive}: kind {st.kernel_kind}, {st.lds_bytes} B LDS, "
                  f"{st.pixels_per_wave} pixels per wave, {st.kernel_vgprs} VGPRs; plan: classes {plan['pixel_classes']}, ranked {plan['rank_tiles']}")
            assert (st.kernel_kind, st.lds_bytes, st.pixels_per_wave) == (plan["kernel_kind"], plan["lds_bytes"], plan["pixels_per_wave"])
            assert st.kernel_vgprs > 0 and st.rays > 0
