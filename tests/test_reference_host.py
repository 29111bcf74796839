"""The reference's own classes, compiled for the host (oracle/ref_world.cpp -> oracle/_ref/libref_world.so, built only where the
reference checkout is present), against the oracle and the library's host side: the generator behind every stream, the frames of
three worlds off the beaten scenes, every constructed bounding box, and the currency of tests/golden/reference_hits.npz.  No GPU.
What needs the built library skips where it is absent; the rest reads the committed fixture."""
import importlib.util
import os

import numpy as np
import pytest

import raytracinginoneweekendincuda_amd as rt
import reference_scene
import reference_worlds as RW
from conftest import ROOT, OracleRng, OracleScene
from query_helpers import bits

needs_reference = pytest.mark.skipif(not reference_scene.available(), reason="oracle/_ref/libref_world.so is built only beside the reference checkout")
CASES = [(name, kind) for name in RW.WORLDS for kind in RW.KINDS]
IDS = [f"{name}-{('bvh', 'list')[kind]}" for name, kind in CASES]


@pytest.fixture(scope="module")
def fixture():
    with np.load(os.path.join(ROOT, "tests", "golden", "reference_hits.npz")) as g:
        return RW.Fixture({k: g[k] for k in g.files})


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


# ---- the generator ----
@needs_reference
@pytest.mark.parametrize("seed, sequence", [(1984, 0), (1984, 1), (1984, 1 << 20), (7, 0), (0x1234567890ABCDEF, 3)])
def test_the_shim_is_the_oracles_xorwow(oracle, seed, sequence):
    """curand_init and curand_uniform of oracle/ref_shim/curand_kernel.h against oracle_rng_state / oracle_rng_stream: the six words
    after seeding and the first 64 uniforms, bit for bit (tests/test_rng.py pins the oracle's to rocRAND's engine)."""
    r = reference_scene.RefRng(seed, sequence)
    assert np.array_equal(np.array(r.state(), dtype=np.uint32), oracle.rng_state(seed, sequence))
    _, want = oracle.rng_stream(seed, sequence, 64)
    got = np.array([r.uniform() for _ in range(64)], dtype=np.float32)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    # the words after 64 draws are the seeded words advanced 64 steps: the layout is Rng.state()'s
    assert np.array_equal(np.array(r.state(), dtype=np.uint32), RW.xorwow_advance(oracle.rng_state(seed, sequence), [64])[0])
    assert rt.Rng(seed, sequence).state() == [int(x) for x in oracle.rng_state(seed, sequence)]


# ---- the oracle is the reference ----
@pytest.mark.parametrize("name, kind", CASES, ids=IDS)
def test_the_oracles_frame_is_the_references_frame(fixture, name, kind):
    """OracleScene.render against the frame ref_render made of the same world: the reference's Hit, Scatter, Emitted, textures,
    Perlin, GetRay and BVH under the restated pixel loop, the same compiler flags and libm on both sides, so no tolerance."""
    scene = RW.build(name, OracleScene(), OracleRng, kind)
    got = scene.render(RW.W, RW.H, RW.SPP, seed=RW.SEED)
    want = fixture.of(name, "frame", kind)
    differ = np.flatnonzero(np.any(bits(got) != bits(want), axis=-1).reshape(-1))
    print(f"{name} kind {kind}: {len(differ)} of {RW.W * RW.H} pixels differ" + (f", the first at {differ[0] % RW.W},{differ[0] // RW.W}" if len(differ) else ""))
    assert len(differ) == 0


@needs_reference
@pytest.mark.parametrize("name, kind", CASES, ids=IDS)
def test_the_committed_frame_is_current(fixture, name, kind):
    scene = RW.build(name, reference_scene.RefScene(), reference_scene.RefRng, kind)
    assert same(scene.render(RW.W, RW.H, RW.SPP, RW.SEED), fixture.of(name, "frame", kind))


# ---- constructed bounding boxes ----
@pytest.mark.parametrize("name, kind", CASES, ids=IDS)
def test_every_constructed_box_is_the_references(fixture, name, kind):
    """BoundingBox() of every Hittable in the order of construction -- every leaf, wrapper, list and BvhNode root: the oracle's and the
    library's against the reference's (the committed ones; where the reference is built, its own as well), bit for bit.  And every
    leaf box of dump_leaves is the box of one of them."""
    want = fixture.of(name, "boxes", kind)
    sides = {"oracle": (OracleScene(), OracleRng), "library": (rt.Scene(), rt.Rng)}
    if reference_scene.available():
        sides["reference"] = (reference_scene.RefScene(), reference_scene.RefRng)
    for label, (scene, Rng) in sides.items():
        rec = RW.Recorder(scene)
        RW.build(name, rec, Rng, kind)
        got = np.array([scene.BoundingBox(h) for h in rec.hittables])
        assert got.shape == want.shape, label
        wrong = np.flatnonzero(np.any(bits(got) != bits(want), axis=-1))
        assert len(wrong) == 0, f"{label}: hittable {wrong[0]} of {len(want)} in the order of construction: {got[wrong[0]]} != {want[wrong[0]]}"
        if label == "library":
            known = {row.tobytes() for row in want}
            kinds, leaves = scene.dump_leaves()
            assert len(leaves) > 0 and all(row.tobytes() in known for row in np.ascontiguousarray(leaves)), "a leaf box that no constructor made"


# ---- the fixture ----
@needs_reference
def test_the_committed_rays_and_answers_are_current(fixture):
    """ref_hit, ref_step, the folded paths and everything else the generator writes, made again and compared bit for bit."""
    spec = importlib.util.spec_from_file_location("make_reference_golden", os.path.join(ROOT, "tests", "golden", "make_reference_golden.py"))
    module = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(module)
    fresh = module.generate()
    assert sorted(fresh) == sorted(fixture.g)
    stale = [k for k in fresh if not same(fresh[k], fixture.g[k])]
    assert not stale, stale


def test_the_fixture_holds_what_the_sets_are_for(fixture):
    """Without the reference: the committed sets still have their sizes, their zeros and their shares of hits."""
    for name in RW.WORLDS:
        for set_name in RW.SETS:
            o, d, time, tmin, tmax = fixture.rays(name, set_name)
            assert o.shape == d.shape == (512, 3) and time.shape == tmin.shape == tmax.shape == (512,)
            for kind in RW.KINDS:
                share = float(np.mean(fixture.hits(name, kind, set_name)["hit"] != 0))
                assert 0.2 <= share <= 0.8, (name, set_name, kind, share)
        d = fixture.rays(name, "axis")[1]
        zeros = np.sum(d == 0, axis=-1)
        assert np.sum(zeros >= 1) >= 384 and np.any(np.signbit(d) & (d == 0))
        assert fixture.steps(name, 0)["rng_state"].shape == (1024, 6)
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "reference_hits.npz")) <= os.path.getsize(os.path.join(ROOT, "tests", "golden", "earthmap_stb.npz"))
