"""The LDS layout of a launch (csrc/launch_plan.cpp lds_layout) through rt_plan_launch, table by table, without a GPU.

Every accessor of the BVH kernels (render.hip get_object, get_xform, get_medium, get_group_box, get_quad_aa, get_box, MatView,
perlin_noise_lds / perlin_noise, NodeView) reads its table from LDS or from global memory as lds_layout decided for the launch,
and the frames must not depend on that decision.  rt_launch_plan lists the decision per table (``plan["lds_tables"]``); this file

  (a) pins the row count at which every table changes sides, derived from the sizes of the rows,
  (b) holds every layout of every scene the suite builds to alignment, disjointness and the budgets of a compute unit,
  (c) proves that the cases tests/test_lds_staging_gpu.py renders reach both sides of every table in every kernel that has
      the choice, and the crowded layouts in which placement stops partway,

and shows that the row with the highest index of each table is in view in those scenes.  The scenes (staging_world) are
written once and built on both sides (conftest.build_both) like those of test_shading_gpu."""
import functools
import os

import numpy as np
import pytest

import raytracinginoneweekendincuda_amd as rt
from conftest import build_both
from frame_helpers import render_params

W, H, SPP = 96, 64, 4

# sizes of the rows as csrc/flat_scene.h declares them (doubles and 32-bit words, no padding)
SIZEOF = {"objects": 8 * 4, "xforms": 3 * 8 + 2 * 4, "media": 8 + 2 * 4 + 4 * 8, "group_boxes": 6 * 8,
          "materials": 4 * 8 + 4 * 4 + 7 * 8 + 8, "perlin": 256 * 3 * 8 + 3 * 256 * 4, "quad_aa": 7 * 8 + 2 * 4,
          "boxes": 18 * 8 + 2 * 4, "nodes": 72}
# lds_layout's caps in bytes: a table larger than this stays in global memory
CAP_BYTES = {"objects": 4096, "xforms": 4096, "media": 2048, "group_boxes": 4096, "materials": 4096, "perlin": 2 * SIZEOF["perlin"],
             "boxes": 16 * 1024, "nodes": 60 * 1024}
MAKEBOX_BYTES = 6 * SIZEOF["quad_aa"] + SIZEOF["boxes"]   # a MakeBox is six quad rows and one box row; the two tables go together
# ... and in rows: the last count that is staged
CAP_ROWS = {t: CAP_BYTES[t] // (MAKEBOX_BYTES if t == "boxes" else SIZEOF[t]) for t in CAP_BYTES}
assert CAP_ROWS == {"objects": 128, "xforms": 128, "media": 42, "group_boxes": 85, "materials": 36, "perlin": 2, "boxes": 30, "nodes": 853}

DEFAULT_DYNAMIC_LDS, SHARED_CU_BUDGET, NODE_ROWS_MOST = 48 * 1024, 52 * 1024, 60 * 1024
FLAG_FORCE_GENERAL, FLAG_ALWAYS_WALK, FLAG_REFERENCE_TREE = rt.FLAG_FORCE_GENERAL, rt.FLAG_ALWAYS_WALK, rt.FLAG_REFERENCE_TREE
ADAPTIVE = 512


# ----------------------------------------------------------------------------------------------------------------------
# the scenes
# ----------------------------------------------------------------------------------------------------------------------
COLS = 15                       # the grid of cells faces the camera in the plane z = 0, one unit apart
TABLES = ("objects", "xforms", "media", "group_boxes", "materials", "boxes")   # tables whose rows are grid cells
MODES = (2, 6, 7, 39)           # the composite BVH kernels with a run-time choice per table: instances, media, general, nested


def cell_centre(k):
    return -7.0 + 1.0 * (k % COLS), 3.5 - 1.0 * (k // COLS)


def filler_centre(k):
    return -8.75 + 0.5 * (k % 36), -5.25 + 0.5 * (k // 36), -3.0


def staging_world(table, amount, mode, world="bvh", fillers=20, tweak=None, log=None):
    """One table's rows as a grid of cells facing the camera, in front of a field of small spheres (`fillers` leaves: the node
    rows), beside one of everything so that every accessor is used whatever the table: two instanced boxes, a plain box, an
    instanced group of 20 spheres.

    table, amount   'objects'      amount lists of two spheres (an object row each, no transform)
                    'xforms'       amount transforms, in chains of eight around boxes (the last chain takes the rest)
                    'media'        amount ConstantMedium leaves (every seventh in a box); each brings a phase material
                    'group_boxes'  amount sixteens of static spheres in two instanced BvhNode groups (43 x 16 in the first; the
                                   last sixteen holds a single sphere)
                    'materials'    amount spheres with a material each
                    'boxes'        amount plain MakeBox leaves
                    'perlin'       amount Perlin tables, each on a sphere in view
                    'nodes'        nothing in the grid: the table is the field, `fillers` decides
    mode            2 nothing more; 6 a ConstantMedium; 7 an image texture in view and three NoiseTextures nothing refers
                    to (the scene is rich and the three Perlin tables are over their cap, so the deep kernels do not fit and
                    no noise is evaluated); 'deep' the same with two NoiseTextures and a medium (the deep kernels fit);
                    39 an instance of a list of composites; 0 spheres only, nothing composite
    tweak           the world item of that number (in order of creation) is made of a dark material instead of its own (a medium
                    gets a dark colour); for 'group_boxes' a pair (group, set of sphere numbers)
    log             a list: gets (bounding box, tables the item has rows in) per world item, in order of creation"""
    def build(s, Rng):
        pal = [s.Lambertian((0.8, 0.25, 0.2)), s.Lambertian((0.2, 0.7, 0.3)), s.Lambertian((0.25, 0.3, 0.8)),
               s.Metal((0.8, 0.8, 0.6), 0.1), s.Dielectric(1.5)]
        dark = (0.03, 0.03, 0.03)
        dark_mat = s.Lambertian(dark) if tweak is not None else None
        items = []

        def put(make, default, *tables):
            """make(material) -> the item; `default` is the item's own material"""
            hit = tweak == len(items)
            h = make((dark if isinstance(default, tuple) else dark_mat) if hit else default)
            if log is not None:
                log.append((tuple(s.BoundingBox(h)), tables))
            items.append(h)

        for k in range(fillers):
            put(lambda m: s.Sphere(filler_centre(k), 0.2, m), pal[(k * 7) % 4])
        if mode != 0:
            # one of everything, in the bottom row of the grid
            x, y = cell_centre(8 * COLS + 1)
            put(lambda m: s.Translate(s.RotateY(s.MakeBox((-0.4, -0.4, -0.4), (0.4, 0.4, 0.4), m), 20.0), (x, y, 0.0)), pal[0],
                "objects", "xforms", "boxes")
            put(lambda m: s.Translate(s.RotateY(s.MakeBox((-0.3, -0.4, -0.3), (0.3, 0.4, 0.3), m), -35.0), (x + 1.0, y, 0.0)), pal[3],
                "objects", "xforms", "boxes")
            put(lambda m: s.MakeBox((x + 1.7, y - 0.4, -0.3), (x + 2.3, y + 0.4, 0.3), m), pal[1], "boxes")
            put(lambda m: s.Translate(s.BvhNode([s.Sphere((0.18 * (j % 5), 0.18 * (j // 5), 0.05 * (j % 3)), 0.08, m if j % 2 else pal[j % 4])
                                                 for j in range(20)]), (x + 2.7, y - 0.3, 0.0)), pal[2], "objects", "xforms", "group_boxes")
        if mode in (6, "deep"):
            x, y = cell_centre(8 * COLS + 6)
            put(lambda m: s.ConstantMedium(s.Sphere((x, y, 0.0), 0.45, pal[4]), 2.0, m), (0.9, 0.9, 0.9), "objects", "media", "materials")
        if mode in (7, "deep"):
            x, y = cell_centre(8 * COLS + 7)
            texels = np.random.default_rng(3).integers(0, 256, (3, 2, 3), dtype=np.uint8)
            put(lambda m: s.Sphere((x, y, 0.0), 0.45, m), s.Lambertian(s.ImageTexture(texels)), "materials")
        if mode == 39:
            x, y = cell_centre(8 * COLS + 8)
            put(lambda m: s.Translate(s.RotateY(s.HittableList([s.RotateY(s.Sphere((0, 0, 0), 0.35, m), 30.0),
                                                                s.Translate(s.Sphere((0, 0, 0), 0.3, pal[3]), (0.9, 0.0, 0.0))]), 10.0), (x, y, 0.0)),
                pal[2], "xforms")
        # the table's own rows
        if table == "objects":
            for k in range(amount):
                x, y = cell_centre(k)
                put(lambda m: s.HittableList([s.Sphere((x, y, 0.0), 0.42, m), s.Sphere((x + 0.3, y + 0.3, 0.3), 0.2, pal[(k + 2) % 5])]),
                    pal[k % 5], "objects")
        elif table == "xforms":
            k, left = 0, amount
            while left > 0:
                links = 8 if left >= 16 or left == 8 else left    # chains of eight; the last one takes what is left
                left -= links

                def chain(m):
                    obj = s.MakeBox((-0.4, -0.4, -0.4), (0.4, 0.4, 0.4), m)
                    for j in range(links - 1):
                        obj = s.RotateY(obj, 4.0 + j) if j % 2 == 0 else s.Translate(obj, (0.02, 0.01 * j, -0.01))
                    return s.Translate(obj, (x, y, 0.0))
                x, y = cell_centre(2 * k)
                put(chain, pal[k % 5], "objects", "xforms", "boxes")
                k += 1
        elif table == "media":
            for k in range(amount):
                x, y = cell_centre(k)
                edge = s.MakeBox((x - 0.4, y - 0.4, -0.4), (x + 0.4, y + 0.4, 0.4), pal[4]) if k % 7 == 3 else s.Sphere((x, y, 0.0), 0.45, pal[4])
                put(lambda m: s.ConstantMedium(edge, 3.0, m), (0.2 + 0.1 * (k % 7), 0.9 - 0.1 * (k % 5), 0.3 + 0.2 * (k % 3)),
                    "objects", "media", "materials")
        elif table == "group_boxes" and amount > 0:
            first = 43 * 16
            for g, count in enumerate((first, amount * 16 - first - 15)):
                y0 = 0.4 if g == 0 else -3.2
                swap = tweak[1] if isinstance(tweak, tuple) and tweak[0] == g else ()
                put(lambda m: s.Translate(s.BvhNode([s.Sphere(group_centre(j, y0), 0.07, dark_mat if j in swap else pal[j % 4])
                                                     for j in range(count)]), (0.05, 0.0, 0.0)), pal[0], "objects", "xforms", "group_boxes")
        elif table == "materials":
            for k in range(amount):
                x, y = cell_centre(k)
                shade = (0.15 + 0.1 * (k % 8), 0.85 - 0.1 * (k % 6), 0.2 + 0.15 * (k % 5))
                put(lambda m: s.Sphere((x, y, 0.0), 0.42, m), s.Lambertian(shade) if k % 4 else s.Metal(shade, 0.05), "materials")
        elif table == "boxes":
            for k in range(amount):
                x, y = cell_centre(k)
                put(lambda m: s.MakeBox((x - 0.4, y - 0.4, -0.4), (x + 0.4, y + 0.4, 0.4), m), pal[k % 5], "boxes")
        elif table == "perlin":
            for k in range(amount):
                x, y = cell_centre(k)
                put(lambda m: s.Sphere((x, y, 0.0), 0.45, m), s.Lambertian(s.NoiseTexture(3.0 + k, Rng(1984, k))), "perlin", "materials")
        else:
            assert table in ("nodes", "group_boxes")
        if mode in (7, "deep") and table != "perlin":
            for k in range(3 if mode == 7 else 2):
                s.NoiseTexture(5.0, Rng(1984, 7 + k))
        s.SetWorld(s.BvhNode(items) if world == "bvh" else s.HittableList(items))
        s.Camera((0.0, -0.5, 15.0), (0.0, -0.5, 0.0), (0, 1, 0), 42.0, W / H, 0.0, 15.0, 0.0, 1.0, (0.6, 0.7, 0.9))
        s.Commit()
    return build


def group_centre(j, y0):
    return -3.7 + 0.17 * (j % 43), y0 + 0.17 * (j // 43), 0.0


# ----------------------------------------------------------------------------------------------------------------------
# plans
# ----------------------------------------------------------------------------------------------------------------------
def product(build):
    s = rt.Scene()
    build(s, rt.Rng)
    return s


def plan(scene, w=W, h=H, spp=SPP, variant=0, flags=0, num_cus=256, adaptive=False, pixels_per_wave=64):
    p = render_params(w, h, spp, variant=variant, flags=flags, pixels_per_wave=pixels_per_wave)
    return scene.plan_launch(p, num_cus=num_cus, adaptive=adaptive)


def rows(pl, table):
    """Rows of a table as the plan's layout lists it; 'boxes' are MakeBox boxes (six quad rows and a box row each), 'nodes'
    the node rows at the front (0 where they are read from global memory)."""
    t = pl["lds_tables"]
    if table == "nodes":
        assert pl["lds_front_bytes"] % SIZEOF["nodes"] == 0
        return pl["lds_front_bytes"] // SIZEOF["nodes"]
    if table == "boxes":
        n = t["boxes"][1] // SIZEOF["boxes"]
        assert t["boxes"][1] == n * SIZEOF["boxes"] and t["quad_aa"][1] == 6 * n * SIZEOF["quad_aa"], "quads that are no MakeBox face"
        return n
    assert t[table][1] % SIZEOF[table] == 0
    return t[table][1] // SIZEOF[table]


def staged(pl, table):
    t = pl["lds_tables"]
    if table == "nodes":
        return pl["lds_nodes"] == 1
    if table == "boxes":   # the kernels whose workgroups share a compute unit stage quads and boxes together or not at all
        assert (t["boxes"][0] is None) == (t["quad_aa"][0] is None)
    return t[table][0] is not None


def sides(pl):
    """{table: staged?} for every table with a run-time choice that is not empty in this launch."""
    out = {"nodes": staged(pl, "nodes")}
    for table, (offset, size) in pl["lds_tables"].items():
        if size and table not in ("fast_order", "seg_media", "seg_cand", "park"):
            out[table] = offset is not None
    return out


def bvh_nodes(leaves):
    """Nodes of the reference's tree over that many leaves (R/BvhNode.h: spans of one or two leaves are bottom nodes, a larger
    span is cut in the middle)."""
    return 1 if leaves <= 2 else 1 + bvh_nodes(leaves // 2) + bvh_nodes(leaves - leaves // 2)


@functools.lru_cache(maxsize=None)
def base_rows(table, mode):
    """Rows of `table` and world leaves that a scene of this mode has before its grid is filled."""
    scene = product(staging_world(table, 0, mode, fillers=20))
    return rows(plan(scene, flags=FLAG_ALWAYS_WALK), table) if table != "nodes" else 0, scene.info()["n_leaves"] - 20


def world_with(table, n, mode, fillers=20, **kw):
    """The scene of this mode in which `table` has exactly n rows ('nodes': whose tree has n nodes; `fillers` is ignored)."""
    if table == "nodes":
        leaves = [k for k in range(3, 1200) if bvh_nodes(k) == n]
        assert leaves, f"no leaf count gives {n} nodes"
        return staging_world("nodes", 0, mode, fillers=leaves[0] - base_rows("nodes", mode)[1], **kw)
    return staging_world(table, n - base_rows(table, mode)[0], mode, fillers=fillers, **kw)


# node counts nearest either side of the cap that some leaf count gives
NODES_UNDER = max(bvh_nodes(k) for k in range(3, 1200) if bvh_nodes(k) <= CAP_ROWS["nodes"])
NODES_OVER = min(bvh_nodes(k) for k in range(3, 1200) if bvh_nodes(k) > CAP_ROWS["nodes"])
NODES_CROWDED = 727   # 620 leaves, 52 344 B of rows: what is left of the 52 KB that three workgroups share holds some tables only

# the kernel a mode's scenes run, as test_staging_gpu's cases name it
KIND_OF_MODE = {0: 0, 2: 2, 6: 6, 7: 7, 39: 39}


def label(pl):
    """The instantiation of a plan as the coverage table names it: its kind, 'deep7' for the 768-thread form of kind 7."""
    kind = pl["kernel_kind"] & ~ADAPTIVE
    return "deep7" if kind == 7 and pl["waves_per_simd"] == 3 else kind


# ----------------------------------------------------------------------------------------------------------------------
# the cases tests/test_lds_staging_gpu.py renders: (name, table, rows, mode, fillers, flags, the side it claims for its table)
# ----------------------------------------------------------------------------------------------------------------------
def staging_cases():
    cases = []
    for mode in MODES:
        for table in TABLES + ("perlin",):
            if table == "media" and mode == 2 or table == "perlin" and mode not in (7, 39):
                continue
            for n in (CAP_ROWS[table], CAP_ROWS[table] + 1):   # (the pairs of CAP_PAIRS)
                cases.append((f"{table}-{n}-kind{mode}", table, n, mode, 20, 0, n <= CAP_ROWS[table]))
    for mode in (0,) + MODES:
        flags = FLAG_REFERENCE_TREE if mode == 0 else 0
        cases.append((f"nodes-{NODES_UNDER}-kind{mode}", "nodes", NODES_UNDER, mode, 0, flags, True))
        cases.append((f"nodes-{NODES_OVER}-kind{mode}", "nodes", NODES_OVER, mode, 0, flags, False))
        if mode:
            cases.append((f"nodes-{NODES_CROWDED}-kind{mode}", "nodes", NODES_CROWDED, mode, 0, flags, True))
    # the 768-thread kernels stage the quad rows where they fit behind everything else and read them from global memory otherwise
    for n, side in ((30, True), (50, False)):
        for flags, name in ((0, "kind263"), (FLAG_REFERENCE_TREE, "deep7")):
            cases.append((f"quads-{n}-{name}", "quad_aa", n, "deep", 60, flags, side))
    return cases


def case_build(case, **kw):
    name, table, n, mode, fillers, flags, side = case
    if table == "quad_aa":
        return world_with("boxes", n, mode, fillers=fillers, **kw)
    return world_with(table, n, mode, fillers=fillers, **kw)


CASE_IDS = [c[0] for c in staging_cases()]


# ----------------------------------------------------------------------------------------------------------------------
# (a) the boundary of every cap
# ----------------------------------------------------------------------------------------------------------------------
def flipped(a, b):
    """Tables that are on different sides in two plans of one kernel ('boxes' stands for quads and boxes together)."""
    sa, sb = sides(a), sides(b)
    assert sa.keys() == sb.keys()
    out = {t for t in sa if sa[t] != sb[t]}
    if "quad_aa" in out or "boxes" in out:
        assert {"quad_aa", "boxes"} <= out
        out.discard("quad_aa")
    return out


# (a world with a medium runs kind 6, not 2, and the non-rich kernels read no Perlin table: no such kernel-table pairs)
CAP_PAIRS = [(t, m) for m in MODES for t in TABLES + ("perlin",) if not (t == "media" and m == 2) and not (t == "perlin" and m in (2, 6))]


@pytest.mark.parametrize("table,mode", CAP_PAIRS)
def test_a_table_changes_sides_at_its_cap_and_takes_no_other_with_it(table, mode):
    """objects 128 | 129, xforms 128 | 129, media 42 | 43, group boxes 85 | 86, materials 36 | 37, Perlin tables 2 | 3, MakeBox
    boxes 30 | 31 (six quad rows and a box row each, 16 KB for both tables, all or nothing): CAP_ROWS, from the sizes of the
    rows.  Synthetic worlds with exactly that many rows in all four composite BVH kernels; one row more moves that table to
    global memory and no other.  Every ConstantMedium brings a phase material, so the worlds of the media pair have more than
    36 materials: `materials` is global on both sides of that pair."""
    cap = CAP_ROWS[table]
    under, over = (plan(product(world_with(table, n, mode))) for n in (cap, cap + 1))
    assert label(under) == label(over) == mode
    assert (rows(under, table), rows(over, table)) == (cap, cap + 1)
    assert staged(under, table) and not staged(over, table)
    assert flipped(under, over) == {table}
    if table == "media":
        assert rows(under, "materials") > CAP_ROWS["materials"] and not staged(under, "materials") and not staged(over, "materials")
    # the cap is in bytes: the largest staged table is within it, the smallest global one beyond
    size = lambda pl: sum(pl["lds_tables"][t][1] for t in (("quad_aa", "boxes") if table == "boxes" else (table,)))
    assert size(under) <= CAP_BYTES[table] < size(over)


def test_node_rows_change_sides_at_their_cap():
    """kNodeRowsMost = 60 KB of 72-byte rows: 853 nodes are staged, 854 would not be.  No leaf count gives the reference's tree
    854 nodes (a span of one or two leaves is one node): the nearest trees either side have 853 and 855.  In the primitive
    kernel on the reference's tree (kind 0) the node rows are all there is.  In the composite kernels 853 rows leave no room in
    the 52 KB that three workgroups share, so nothing else is staged beside them, and with the rows in global memory every table
    is: those flips follow from the budget, not from a cap of their own."""
    assert (NODES_UNDER, NODES_OVER) == (CAP_ROWS["nodes"], CAP_ROWS["nodes"] + 2) and CAP_ROWS["nodes"] * SIZEOF["nodes"] <= NODE_ROWS_MOST
    assert (CAP_ROWS["nodes"] + 1) * SIZEOF["nodes"] > NODE_ROWS_MOST
    for mode in (0,) + MODES:
        flags = FLAG_REFERENCE_TREE if mode == 0 else 0
        under, over = (plan(product(world_with("nodes", n, mode)), flags=flags) for n in (NODES_UNDER, NODES_OVER))
        assert label(under) == label(over) == mode
        assert under["lds_nodes"] == 1 and rows(under, "nodes") == NODES_UNDER and under["lds_front_bytes"] > DEFAULT_DYNAMIC_LDS
        assert over["lds_nodes"] == 0 and over["lds_front_bytes"] == 0
        if mode == 0:
            assert under["lds_bytes"] == NODES_UNDER * SIZEOF["nodes"] and over["lds_bytes"] == 0
            assert flipped(under, over) == {"nodes"}
        else:
            s_under, s_over = sides(under), sides(over)
            assert [t for t in s_under if s_under[t]] == ["nodes"]
            assert [t for t in s_over if not s_over[t]] == ["nodes"] + (["perlin"] if mode == 7 else [])


# ----------------------------------------------------------------------------------------------------------------------
# (b) every layout of every scene the suite builds
# ----------------------------------------------------------------------------------------------------------------------
LIBRARY_TREE_READS = ("mspheres", "msphere_aux", "spheres_tab", "sphere_aux", "materials")
DEEP_READS = ("objects", "xforms", "media", "group_boxes", "materials", "perlin", "boxes", "spheres_tab")


def check_layout(pl, name):
    """The layout of one plan: staged tables 16-byte aligned, pairwise disjoint, behind the node rows / planes / queues at the
    front and inside lds_bytes; a compute unit's 160 KB hold one 768-thread workgroup or, at 64 KB each, two of 256 threads;
    a kernel that reads a table from LDS only has it staged."""
    kind = pl["kernel_kind"] & ~ADAPTIVE
    big = bool(kind & 64) or bool(kind & 256) or label(pl) == "deep7"
    assert 0 <= pl["lds_front_bytes"] <= pl["lds_bytes"] <= (160 if big else 64) * 1024, (name, pl["lds_bytes"], big)
    assert (pl["lds_front_bytes"] > 0) == bool(pl["lds_nodes"] or pl["lds_spheres"] or (kind & ~128) == 16), name
    spans = []
    for table, (offset, size) in pl["lds_tables"].items():
        if offset is None or size == 0:
            continue
        assert offset % 16 == 0, (name, table, offset)
        assert pl["lds_front_bytes"] <= offset and offset + size <= pl["lds_bytes"], (name, table, offset, size)
        spans.append((offset, offset + size, table))
    spans.sort()
    for (a0, a1, ta), (b0, b1, tb) in zip(spans, spans[1:]):
        assert a1 <= b0, (name, ta, tb)
    need = ()
    if kind & 64:
        need = LIBRARY_TREE_READS
    elif kind & 256:
        need = DEEP_READS + ("fast_order", "seg_media", "seg_cand")
    elif label(pl) == "deep7":
        need = DEEP_READS
    if need:
        assert pl["lds_nodes"] == 1, name
        for table in need:
            offset, size = pl["lds_tables"][table]
            assert size == 0 or offset is not None, (name, table, "is read from LDS only and is not staged")
    return label(pl), big


def suite_scenes():
    """(name, scene) of every world the suite builds: the built-in scenes in both worlds, the carrier, inline, edge and deep
    worlds of test_shading_gpu, the deep media worlds of test_custom_scenes_gpu, the motion fields, and the cases of this file."""
    import test_motion_time_gpu as M
    import test_shading_gpu as G
    from test_custom_scenes_gpu import _deep_media_world
    from test_motion_time import field
    earth = np.load(os.path.join(os.path.dirname(__file__), "golden", "earthmap_stb.npz"))["bytes"]
    for scene_id in range(12):
        for world in (0, 1):
            yield f"builtin {scene_id} world {world}", rt.builtin_scene(scene_id, world, 96, 64, earth=earth if scene_id == 9 else None)
    for texture in G.TEXTURES:
        for world in ("list", "bvh"):
            for media in (True, False):
                yield f"carrier {texture} {world} media {media}", product(G.carrier_world(texture, world, media=media))
    for texture in sorted(G.NESTED_FLOOR):
        for world in ("list", "bvh"):
            for tree in ("bvh_object", "instance_of_list"):
                yield f"nested {texture} {world} {tree}", product(G.carrier_world(texture, world, tree=tree))
    for shape in ("spheres", "prims", "instances", "media"):
        for world in ("list", "bvh"):
            yield f"inline {shape} {world}", product(G.inline_world(shape, world))
    for scene in ("static", "moving", "inside", "mixed"):
        for world in ("list", "bvh"):
            yield f"edges {scene} {world}", product(G.edges_world(scene, world))
    for kw in (dict(n_noise=1), dict(n_noise=2), dict(n_noise=2, unused_noise=1), dict(n_noise=2, filler_boxes=200)):
        yield f"deep rich {kw}", product(G.deep_rich_world(**kw))
    for media in (("mist",), ("mist", "ball", "crate"), ("lone", "ball"), (), ("mist", "ball", "crate", "far", "more", "more")):
        yield f"deep media {media}", product(_deep_media_world(media))
    for case in M.IDS:
        motion, shutter, rise, inside = M.CASES[case]
        for world in ("bvh", "list"):
            yield f"motion {case} {world}", product(field(world, motion, shutter, rise=rise, moving_every=3, quads=True))
        yield f"motion {case} small", product(field("bvh", motion, shutter, rise=rise, n=11))
    for case in staging_cases():
        yield f"staging {case[0]}", product(case_build(case))
        if case[6] is False or case[1] == "nodes":
            yield f"staging {case[0]} list", product(case_build(case, world="list"))


def test_every_layout_of_every_scene_of_the_suite_is_sound():
    """check_layout over suite_scenes(), both builds, plain and adaptive, one lane per ray and eight pixels per wave, and every
    flag that changes the kernel: RT_FLAG_FORCE_GENERAL, _REFERENCE_TREE, both, _ALWAYS_WALK, _ACCELERATE_LISTS."""
    flag_sets = (0, FLAG_FORCE_GENERAL, FLAG_REFERENCE_TREE, FLAG_FORCE_GENERAL | FLAG_REFERENCE_TREE, FLAG_ALWAYS_WALK, rt.FLAG_ACCELERATE_LISTS)
    seen, plans = set(), 0
    for name, scene in suite_scenes():
        for flags in flag_sets:
            for adaptive in (False, True):
                for ppw in (64, 8):
                    for variant in (0, 1):
                        pl = plan(scene, flags=flags, adaptive=adaptive, pixels_per_wave=ppw, variant=variant)
                        seen.add(check_layout(pl, (name, flags, adaptive, ppw, variant)))
                        plans += 1
    print(f"{plans} plans; instantiations (kind, 768 threads): {sorted(seen, key=str)}")
    # nothing above passes for want of layouts: both block sizes, each LDS-only kernel, the list and sphere-list kernels were there
    assert {(64, True), ("deep7", True), (263, True), (0, False), (2, False), (6, False), (7, False), (39, False), (16, False), (10, False)} <= seen


# ----------------------------------------------------------------------------------------------------------------------
# (c) what the GPU cases reach
# ----------------------------------------------------------------------------------------------------------------------
def choices():
    """Every (instantiation, table, staged?) with a run-time choice in a BVH kernel."""
    out = set()
    for side in (True, False):
        out |= {(k, "nodes", side) for k in (0, 2, 6, 7, 39)}
        out |= {(k, t, side) for k in (2, 6, 7, 39) for t in ("objects", "xforms", "group_boxes", "materials", "boxes")}
        out |= {(k, "media", side) for k in (6, 7, 39)}
        out |= {(k, "perlin", side) for k in (7, 39)}
        out |= {(k, "quad_aa", side) for k in ("deep7", 263)}
    return out


def case_plans(case, num_cus=256):
    """The scene of a case and its plans, plain and adaptive, strict and fast: {(variant, adaptive): plan}."""
    scene = product(case_build(case))
    return scene, {(v, a): plan(scene, flags=case[5], variant=v, adaptive=a, num_cus=num_cus) for v in (0, 1) for a in (False, True)}


def test_the_gpu_cases_reach_both_sides_of_every_table_in_every_kernel():
    """The plan proves on the CPU what tests/test_lds_staging_gpu.py renders: every (instantiation, table, side) of choices(), and
    per 256-thread composite instantiation a crowded layout -- more than 48 KB of node rows, some tables staged behind them
    and some under their caps refused for want of room -- and one of more than 48 KB that holds node rows and nothing else."""
    reached, crowded, rows_only = set(), set(), set()
    for case in staging_cases():
        name, table, n, mode, fillers, flags, side = case
        _, plans = case_plans(case)
        pl = plans[0, False]
        for other in plans.values():   # the same layout in both builds, adaptive or not
            assert (label(other), other["lds_bytes"], other["lds_tables"]) == (label(pl), pl["lds_bytes"], pl["lds_tables"]), name
            assert other["kernel_kind"] & ~ADAPTIVE == pl["kernel_kind"]
        kind = label(pl)
        assert kind == {"deep": "deep7" if flags else 263}.get(mode, mode), (name, kind)
        assert staged(pl, "boxes" if table in ("boxes",) else table) == side, name
        if table not in ("nodes", "quad_aa"):
            assert rows(pl, table) == n, name
        for t, s in sides(pl).items():
            if kind in ("deep7", 263):
                if t == "quad_aa":
                    reached.add((kind, t, s))
            elif t == "boxes":
                reached.add((kind, "boxes", staged(pl, "boxes")))
            elif t != "quad_aa":
                reached.add((kind, t, s))
        if kind in (2, 6, 7, 39) and pl["lds_front_bytes"] > DEFAULT_DYNAMIC_LDS:
            s = {t: v for t, v in sides(pl).items() if t != "nodes"}
            under_cap = lambda t: pl["lds_tables"][t][1] <= CAP_BYTES.get(t, 16 * 1024)
            if any(s.values()) and any(not v and under_cap(t) for t, v in s.items()):
                crowded.add(kind)
                assert pl["lds_bytes"] <= SHARED_CU_BUDGET
            if not any(s.values()):
                rows_only.add(kind)
                assert DEFAULT_DYNAMIC_LDS < pl["lds_bytes"] <= NODE_ROWS_MOST
    assert reached >= choices(), sorted(choices() - reached, key=str)
    assert crowded == {2, 6, 7, 39} and rows_only == {2, 6, 7, 39}


# ----------------------------------------------------------------------------------------------------------------------
# the row with the highest index is in view
# ----------------------------------------------------------------------------------------------------------------------
def top_item(table, n, mode):
    """The world item (in order of creation) that holds the row of `table` with the highest index.  Object, transform, medium,
    box and node rows are written leaf by leaf in the order of the world's leaves (rt_scene_dump_leaves); material rows and
    Perlin tables in order of creation.  'group_boxes': (group, spheres) of the last sixteen of the group lowered last."""
    log = []
    scene = product(world_with(table, n, mode, log=log))
    _, leaf_boxes = scene.dump_leaves()
    created = {box: k for k, (box, _) in enumerate(log)}
    assert len(created) == len(log) == len(leaf_boxes)
    order = [created[tuple(b)] for b in leaf_boxes]
    if table in ("materials", "perlin"):
        return max(k for k, (_, tables) in enumerate(log) if table in tables)
    if table == "nodes":
        return order[-1]
    if table != "group_boxes":
        return [k for k in order if table in log[k][1]][-1]
    # the sub-BVHs of the groups follow the world's nodes, in the order the groups were lowered; their sphere rows likewise
    node_boxes, abe = scene.dump_nodes()
    world_nodes = rows(plan(scene), "nodes")
    best = (-1, None)
    for k in range(world_nodes, len(abe)):
        for ref in abe[k][:2]:
            if int(ref) >> 28 == 0:
                best = max(best, (int(ref) & ((1 << 28) - 1), k))
    lo, hi = node_boxes[best[1]][0::2], node_boxes[best[1]][1::2]   # xlo, xhi, ylo, yhi, zlo, zhi
    amount = n - base_rows("group_boxes", mode)[0]
    for g, count in enumerate((43 * 16, amount * 16 - 43 * 16 - 15)):
        inside = {j for j in range(count) if all(lo[a] <= group_centre(j, 0.4 if g == 0 else -3.2)[a] <= hi[a] for a in range(3))}
        if inside:
            assert len(inside) <= 2
            return g, frozenset(inside)
    raise AssertionError("the last sixteen belongs to none of the two groups of the grid")


@pytest.mark.parametrize("table,mode", [(t, 2) for t in ("objects", "xforms", "group_boxes", "materials", "boxes")] +
                         [("media", 6), ("perlin", 7), ("nodes", 0), ("nodes", 2)])
def test_the_row_with_the_highest_index_is_in_view(table, mode, oracle):
    """On the global side of its pair, the item that holds the table's last row (top_item) made of another material (a
    medium: of another colour) changes the oracle's frame: a kernel that mis-reads the rows past the
    cap index cannot render these scenes right."""
    from conftest import OracleRng, OracleScene
    n = NODES_OVER if table == "nodes" else CAP_ROWS[table] + 1
    top = top_item(table, n, mode)
    frames = []
    for tweak in (None, top):
        orc = OracleScene()
        world_with(table, n, mode, tweak=tweak)(orc, OracleRng)
        frames.append(orc.render(W, H, SPP))
    changed = np.any(frames[0] != frames[1], axis=-1)
    print(f"{table}: item {top} holds the last row; {int(changed.sum())} pixels change with it")
    assert changed.sum() >= 2
