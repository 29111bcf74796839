"""The environment without a device: what rt_scene_set_environment refuses, the PFM reader, the importance sampler's tables
against the numpy restatement (tests/environment_restated.py) bit for bit, and the kernel a launch of such a scene chooses."""
import struct

import numpy as np
import pytest

import environment_restated as E
import raytracinginoneweekendincuda_amd as rt
from frame_helpers import render_params
from query_helpers import bits


def base_scene(world="list"):
    """A small world, a camera with a black background; not committed."""
    s = rt.Scene()
    red = s.Lambertian((0.6, 0.2, 0.2))
    if world == "list":      # a sphere list
        s.SetWorld(s.HittableList([s.Sphere((0, 0, -3), 1.0, red), s.Sphere((2, 0, -3), 0.5, red)]))
    elif world == "bvh":     # a primitive BVH
        s.SetWorld(s.BvhNode([s.Sphere((k, 0, -3), 0.4, red) for k in range(-2, 3)]))
    else:                    # an instanced list
        s.SetWorld(s.HittableList([s.Translate(s.MakeBox((0, 0, 0), (1, 1, 1), red), (0, 0, -3)), s.Sphere((2, 0, -3), 0.5, red)]))
    s.Camera((0, 0, 0), (0, 0, -1), (0, 1, 0), 60.0, 1.0, 0.0, 1.0, background=(0, 0, 0))
    return s


def random_map(w, h, seed):
    return np.random.default_rng(seed).uniform(0.05, 2.0, size=(h, w, 3)).astype(np.float32)


# ---- refusals ----
def test_both_or_neither_of_texture_and_image_is_refused():
    s = base_scene()
    t = s.SolidColor((1, 1, 1))
    with pytest.raises(rt.RtowError, match="not both"):
        s.Environment(texture=t, image=random_map(2, 2, 0))
    env = rt._lib.Environment()   # neither: only the C call can say it (Environment() with both None removes the environment)
    env.intensity[:] = [1.0, 1.0, 1.0]
    env.rotation[:] = list(np.eye(3).reshape(9))
    assert rt.lib().rt_scene_set_environment(s._p, env) != 0 and b"not both" in rt.lib().rt_last_error()


@pytest.mark.parametrize("intensity", [-1.0, float("nan"), float("inf"), (1.0, 1.0, -0.5)])
def test_bad_intensity_is_refused(intensity):
    s = base_scene()
    with pytest.raises(rt.RtowError, match="intensity"):
        s.Environment(image=random_map(2, 2, 0), intensity=intensity)


def test_bad_rotation_is_refused():
    s = base_scene()
    bad = np.eye(3)
    bad[0, 0] = float("nan")
    with pytest.raises(rt.RtowError, match="not finite"):
        s.Environment(image=random_map(2, 2, 0), rotation=bad)
    with pytest.raises(rt.RtowError, match="orthonormal"):
        s.Environment(image=random_map(2, 2, 0), rotation=2.0 * np.eye(3))
    skew = np.eye(3)
    skew[0, 1] = 1e-8   # rows no longer orthogonal to 1e-9
    with pytest.raises(rt.RtowError, match="orthonormal"):
        s.Environment(image=random_map(2, 2, 0), rotation=skew)
    s.Environment(image=random_map(2, 2, 0), rotation=E.rotation((1, 2, 3), 40.0))   # a rotation that is not axis-aligned passes


def test_bad_sizes_and_texels_are_refused():
    s = base_scene()
    env = rt._lib.Environment()
    env.intensity[:] = [1.0, 1.0, 1.0]
    env.rotation[:] = list(np.eye(3).reshape(9))
    img = random_map(2, 2, 0)
    env.rgb = img.ctypes.data
    for w, h in ((0, 2), (2, 0), (-1, 2)):
        env.width, env.height = w, h
        assert rt.lib().rt_scene_set_environment(s._p, env) != 0 and b"at least 1" in rt.lib().rt_last_error()
    for bad in (-0.5, float("nan"), float("inf")):
        img = random_map(3, 2, 1)
        img[1, 2, 1] = bad
        with pytest.raises(rt.RtowError, match="texel"):
            s.Environment(image=img)
    with pytest.raises(rt.RtowError, match="texture handle"):
        s.Environment(texture=999)


def test_a_call_after_commit_uncommits_like_the_other_construction_calls():
    """No construction call refuses after commit: each makes the scene count as not committed (rt_scene_set_world)."""
    s = base_scene()
    s.Commit()
    assert s.flags() & rt.SCENE_FLAG_ENVIRONMENT == 0
    s.Environment(image=random_map(2, 2, 0))
    with pytest.raises(rt.RtowError, match="not committed"):
        s.info()
    s.Commit()
    assert s.flags() & rt.SCENE_FLAG_ENVIRONMENT
    s.Environment()   # back to the camera's background
    s.Commit()
    assert s.flags() & rt.SCENE_FLAG_ENVIRONMENT == 0 and s.environment() is None


# ---- the PFM reader ----
def test_pfm_round_trip_to_the_float(tmp_path):
    frame = np.random.default_rng(3).uniform(0.0, 50.0, size=(5, 7, 3))
    path = tmp_path / "frame.pfm"
    rt.write_pfm(path, frame)
    got = rt.load_pfm(path)
    assert got.dtype == np.float32 and got.shape == (5, 7, 3)
    assert np.array_equal(bits(got), bits(frame[::-1].astype(np.float32)))   # the file's rows are bottom first, the array's top first


@pytest.mark.parametrize("order,scale", [("<", -1.0), (">", 1.0), ("<", -2.5), (">", 0.5)])
def test_pfm_both_byte_orders_and_the_scale(tmp_path, order, scale):
    rows = np.random.default_rng(4).uniform(0.0, 9.0, size=(3, 4, 3)).astype(np.float32)   # as the file holds them: bottom first
    path = tmp_path / "map.pfm"
    with open(path, "wb") as f:
        f.write(b"PF\n4 3\n%r\n" % scale)
        f.write(struct.pack(order + "36f", *rows.reshape(-1)))
    want = rows[::-1] if abs(scale) == 1.0 else np.float32(abs(scale)) * rows[::-1]
    assert np.array_equal(bits(rt.load_pfm(path)), bits(want))


def test_pfm_refuses_what_is_no_colour_pfm(tmp_path):
    for name, data in (("grey.pfm", b"Pf\n1 1\n-1.0\n" + bytes(4)), ("short.pfm", b"PF\n2 2\n-1.0\n" + bytes(40)), ("zero.pfm", b"PF\n2 2\n0.0\n" + bytes(48))):
        path = tmp_path / name
        path.write_bytes(data)
        with pytest.raises(rt.RtowError, match="rt_pfm_load"):
            rt.load_pfm(path)
    with pytest.raises(rt.RtowError, match="cannot open"):
        rt.load_pfm(tmp_path / "none.pfm")


# ---- the distribution ----
def test_get_environment_round_trips():
    s = base_scene()
    assert s.environment() is None
    img, R = random_map(3, 2, 5), E.rotation((0.3, 1.0, -0.2), 77.0)
    s.Environment(image=img, intensity=(1.0, 0.5, 2.0), rotation=R)
    got = s.environment()
    assert got["texture"] is None and np.array_equal(bits(got["image"]), bits(img)) and not got["has_distribution"]   # not committed yet
    assert np.array_equal(got["intensity"], [1.0, 0.5, 2.0]) and np.array_equal(bits(got["rotation"]), bits(R))
    s.Commit()
    assert s.environment()["has_distribution"]
    t = s.SolidColor((0.2, 0.3, 0.4))
    s.Environment(texture=t)
    got = s.environment()
    assert got["texture"] == t and got["image"] is None and np.array_equal(got["rotation"], np.eye(3))


@pytest.mark.parametrize("w,h", [(1, 1), (3, 2), (8, 4)])
@pytest.mark.parametrize("intensity", [(1.0, 1.0, 1.0), (0.25, 3.0, 1.5)])
def test_cdf_equals_the_restatement_bit_for_bit(w, h, intensity):
    img = random_map(w, h, 10 * w + h)
    s = base_scene()
    s.Environment(image=img, intensity=intensity)
    s.Commit()
    marginal, conditional = s.environment_cdf()
    want_m, want_c = E.build_cdf(img, intensity)
    assert marginal.shape == (h,) and conditional.shape == (h, w)
    assert np.array_equal(bits(marginal), bits(want_m)) and np.array_equal(bits(conditional), bits(want_c))
    assert marginal[-1] == 1.0 and np.all(conditional[:, -1] == 1.0) and np.all(np.diff(marginal) >= 0.0) and np.all(np.diff(conditional, axis=1) >= 0.0)


def test_cdf_of_an_8_bit_image_texture():
    img8 = np.random.default_rng(6).integers(0, 256, size=(4, 8, 3), dtype=np.uint8)
    s = base_scene()
    s.Environment(texture=s.ImageTexture(img8), intensity=(2.0, 1.0, 0.5))
    s.Commit()
    marginal, conditional = s.environment_cdf()
    want_m, want_c = E.build_cdf(img8, (2.0, 1.0, 0.5))
    assert np.array_equal(bits(marginal), bits(want_m)) and np.array_equal(bits(conditional), bits(want_c))


def test_cdf_with_zero_rows_and_zero_texels():
    img = random_map(4, 5, 8)
    img[0] = 0.0          # the first row
    img[2] = 0.0          # a row in the middle
    img[4] = 0.0          # the last row
    img[1, 0] = 0.0       # texels at both ends of a row, and one inside
    img[1, 3] = 0.0
    img[3, 2] = 0.0
    s = base_scene()
    s.Environment(image=img)
    s.Commit()
    marginal, conditional = s.environment_cdf()
    want_m, want_c = E.build_cdf(img, (1.0, 1.0, 1.0))
    assert np.array_equal(bits(marginal), bits(want_m)) and np.array_equal(bits(conditional), bits(want_c))
    # a zero row or texel has chance 0: its entry repeats the one before it (0 for the first), so no draw in (0, 1] finds it
    assert marginal[0] == 0.0 and marginal[2] == marginal[1] and marginal[3] == 1.0 and marginal[4] == 1.0
    assert conditional[1, 0] == 0.0 and conditional[1, 2] == 1.0 and conditional[3, 2] == conditional[3, 1]
    assert np.all(conditional[[0, 2, 4]] == 1.0)   # never consulted


def test_no_distribution_for_an_all_zero_map_or_zero_intensity():
    for img, k in ((np.zeros((2, 3, 3), dtype=np.float32), 1.0), (random_map(3, 2, 9), 0.0)):
        s = base_scene()
        s.Environment(image=img, intensity=k)
        s.Commit()
        assert s.environment_cdf() is None and not s.environment()["has_distribution"] and E.build_cdf(img, (k, k, k)) is None


def test_no_distribution_for_a_texture_that_is_no_image():
    for make in (lambda s: s.SolidColor((1, 2, 3)), lambda s: s.CheckerTexture(0.5, s.SolidColor((1, 1, 1)), s.SolidColor((0, 0, 0))),
                 lambda s: s.NoiseTexture(4.0, rt.Rng(1984, 0)),
                 lambda s: s.CheckerTexture(0.5, s.ImageTexture(np.full((2, 2, 3), 200, dtype=np.uint8)), s.SolidColor((0, 0, 0)))):
        s = base_scene()
        s.Environment(texture=make(s))
        s.Commit()
        assert s.environment_cdf() is None and not s.environment()["has_distribution"]
        assert s.flags() & rt.SCENE_FLAG_ENVIRONMENT


# ---- launch plans ----
@pytest.mark.parametrize("world", ["list", "bvh", "instanced"])
@pytest.mark.parametrize("adaptive", [False, True])
def test_an_environment_scene_takes_a_rich_instantiation_and_no_other_scene_changes(world, adaptive):
    p = render_params(16, 16, 4)
    s = base_scene(world)
    s.Commit()
    before, flags = s.plan_launch(p, adaptive=adaptive), s.flags()
    assert before["kernel_kind"] & 1 == 0 and flags & rt.SCENE_FLAG_ENVIRONMENT == 0   # specialised: no texture code
    s.Environment(texture=s.SolidColor((0.5, 0.7, 1.0)))
    s.Commit()
    with_env = s.plan_launch(p, adaptive=adaptive)
    assert with_env["kernel_kind"] & 1 == 1 and with_env["kernel_kind"] & 2 == 2, with_env["kernel_kind"]   # rich, general
    assert s.flags() == flags | rt.SCENE_FLAG_ENVIRONMENT
    s.Environment()
    s.Commit()
    assert s.plan_launch(p, adaptive=adaptive) == before and s.flags() == flags   # without it: the flags and the plan it had


def test_abi_sizes_and_the_cap():
    assert rt._lib.env_lds_rows() == 2048
