// scene_builder.cpp -- host side of the construction API (include/rtow.h) and the flattener.
//
// The reference builds its world on the device with `new` inside a <<<1,1>>> kernel
// (R/kernel.cu:176-543).  Here the same constructors run on the host, keep a handle-addressed object
// graph, and rt_scene_commit() lowers that graph to the SoA tables of flat_scene.h.  All arithmetic
// that decides geometry (bounding boxes, quad planes, rotation constants, BVH split order) follows
// the reference expression by expression, in fp64 without contraction, so the tables are bit-identical
// to what the reference's constructors compute.
#include <algorithm>
#include <cfloat>
#include <charconv>
#include <cmath>
#include <limits>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <unordered_map>

#include "../../include/rtow.h"
#include "launch_plan.h"
#include "primary_cull_rule.h"
#include "scan_window_rule.h"
#include "scene_host.h"

namespace rtow {

// ------------------------------------------------------------------------------------------------
// errors
// ------------------------------------------------------------------------------------------------
static thread_local std::string g_error;
void set_error(const std::string &msg) { g_error = msg; }
int fail(int status, const std::string &msg)
{
    g_error = msg;
    return status;
}

// ------------------------------------------------------------------------------------------------
// small vector helpers (R/Vec3.h semantics: v / t is (1 / t) * v)
// ------------------------------------------------------------------------------------------------
static inline D3 mk(double x, double y, double z) { return D3{x, y, z}; }
static inline D3 add(D3 a, D3 b) { return mk(a.x + b.x, a.y + b.y, a.z + b.z); }
static inline D3 sub(D3 a, D3 b) { return mk(a.x - b.x, a.y - b.y, a.z - b.z); }
static inline D3 neg(D3 a) { return mk(-a.x, -a.y, -a.z); }
static inline D3 scale(double t, D3 a) { return mk(t * a.x, t * a.y, t * a.z); }
static inline double dot(D3 a, D3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
static inline D3 cross(D3 u, D3 v) { return mk(u.y * v.z - u.z * v.y, u.z * v.x - u.x * v.z, u.x * v.y - u.y * v.x); }
static inline double length(D3 a) { return std::sqrt(a.x * a.x + a.y * a.y + a.z * a.z); }
static inline D3 over(D3 a, double t) { return scale(1 / t, a); }
static inline D3 normalize(D3 a) { return over(a, length(a)); }
static inline double comp(D3 a, int k) { return k == 0 ? a.x : (k == 1 ? a.y : a.z); }
// A general affine instance's arithmetic as include/rtow.h rt_transform states it (and render.hip affine_rows computes it): one
// rounding per operation, this file is built with contraction off.  m: a row-major 3x3.
static inline D3 mat_rows(const double *m, D3 p)
{
    return mk(((m[0] * p.x) + (m[1] * p.y)) + (m[2] * p.z), ((m[3] * p.x) + (m[4] * p.y)) + (m[5] * p.z), ((m[6] * p.x) + (m[7] * p.y)) + (m[8] * p.z));
}
static inline D3 affine_point(const HostAffine &a, D3 p) { return add(mat_rows(a.L, p), mk(a.t[0], a.t[1], a.t[2])); }  // (L p) + t
static inline D3 affine_normal(const HostAffine &a, D3 n)  // Li^T n, renormalised
{
    const double *i = a.Li;
    const D3 m = mk(((i[0] * n.x) + (i[3] * n.y)) + (i[6] * n.z), ((i[1] * n.x) + (i[4] * n.y)) + (i[7] * n.z), ((i[2] * n.x) + (i[5] * n.y)) + (i[8] * n.z));
    return scale(1.0 / std::sqrt(m.x * m.x + m.y * m.y + m.z * m.z), m);
}
static inline bool is_instance(HKind k) { return k == HKind::Translate || k == HKind::RotateY || k == HKind::Transform || k == HKind::MovingTransform; }

// ------------------------------------------------------------------------------------------------
// boxes (R/AABB.h, R/Interval.h)
// ------------------------------------------------------------------------------------------------
static Box empty_box()
{
    Box b;
    for (int k = 0; k < 3; k++) {
        b.lo[k] = +DBL_MAX;
        b.hi[k] = -DBL_MAX;
    }
    return b;
}
static void pad_thin_axes(Box &b)  // AABB.h:114-120
{
    const double delta = 0.0001;
    for (int k = 0; k < 3; k++)
        if (b.hi[k] - b.lo[k] < delta) {
            double half = delta / 2.0;
            b.lo[k] = b.lo[k] - half;
            b.hi[k] = b.hi[k] + half;
        }
}
static Box box_from_corners(D3 a, D3 b)  // AABB.h:34-40
{
    Box r;
    for (int k = 0; k < 3; k++) {
        double p = comp(a, k), q = comp(b, k);
        if (p <= q) {
            r.lo[k] = p;
            r.hi[k] = q;
        } else {
            r.lo[k] = q;
            r.hi[k] = p;
        }
    }
    pad_thin_axes(r);
    return r;
}
static Box box_merge(const Box &a, const Box &b)  // AABB.h:43-48 (no padding)
{
    Box r;
    for (int k = 0; k < 3; k++) {
        r.lo[k] = a.lo[k] <= b.lo[k] ? a.lo[k] : b.lo[k];
        r.hi[k] = a.hi[k] >= b.hi[k] ? a.hi[k] : b.hi[k];
    }
    return r;
}
static Box box_moved(const Box &b, D3 off)  // AABB.h:127-130 (interval ctor pads again)
{
    Box r;
    for (int k = 0; k < 3; k++) {
        r.lo[k] = b.lo[k] + comp(off, k);
        r.hi[k] = b.hi[k] + comp(off, k);
    }
    pad_thin_axes(r);
    return r;
}
static int longest_axis(const Box &b)  // AABB.h:101-107
{
    double sx = b.hi[0] - b.lo[0], sy = b.hi[1] - b.lo[1], sz = b.hi[2] - b.lo[2];
    if (sx > sy) return sx > sz ? 0 : 2;
    return sy > sz ? 1 : 2;
}

// ------------------------------------------------------------------------------------------------
// host RNG jump table: T^(2^67 * g * 16^k) for g = 1..15, k = 0..15
// ------------------------------------------------------------------------------------------------
namespace {
struct Gf2 {
    uint32_t row[160][5];
};
void gf2_mul_vec(const Gf2 &m, const uint32_t in[5], uint32_t out[5])
{
    uint32_t acc[5] = {0, 0, 0, 0, 0};
    for (int i = 0; i < 160; i++)
        if ((in[i >> 5] >> (i & 31)) & 1u)
            for (int k = 0; k < 5; k++) acc[k] ^= m.row[i][k];
    std::memcpy(out, acc, sizeof acc);
}
// r = a after b (apply b first, then a): row_i(r) = a(row_i(b))
void gf2_compose(const Gf2 &a, const Gf2 &b, Gf2 &r)
{
    for (int i = 0; i < 160; i++) gf2_mul_vec(a, b.row[i], r.row[i]);
}
std::vector<uint32_t> build_jump_table()
{
    std::vector<uint32_t> table(kJumpTableWords);
    Gf2 *cur = new Gf2, *tmp = new Gf2, *pw = new Gf2;
    for (int i = 0; i < 160; i++) {
        Xorwow s{0, 0, 0, 0, 0, 0};
        uint32_t *w = &s.v0;
        w[i >> 5] = 1u << (i & 31);
        xorwow_next(s);
        cur->row[i][0] = s.v0; cur->row[i][1] = s.v1; cur->row[i][2] = s.v2; cur->row[i][3] = s.v3; cur->row[i][4] = s.v4;
    }
    for (int k = 0; k < 67; k++) {  // T^(2^67)
        gf2_compose(*cur, *cur, *tmp);
        std::swap(cur, tmp);
    }
    for (int k = 0; k < kJumpDigits; k++) {
        // cur = J^(16^k); fill g = 1..15 by repeated composition
        *pw = *cur;
        for (int g = 1; g <= 15; g++) {
            std::memcpy(&table[((size_t)k * 15 + (g - 1)) * kJumpMatrixWords], pw->row, sizeof pw->row);
            if (g < 15) {
                gf2_compose(*cur, *pw, *tmp);
                *pw = *tmp;
            }
        }
        gf2_compose(*cur, *pw, *tmp);  // J^(16^k * 16)
        *cur = *tmp;
    }
    delete cur;
    delete tmp;
    delete pw;
    return table;
}
} // namespace

const uint32_t *host_jump_table()
{
    static std::once_flag once;
    static std::vector<uint32_t> table;
    std::call_once(once, [] { table = build_jump_table(); });
    return table.data();
}

// ------------------------------------------------------------------------------------------------
// graph access helpers
// ------------------------------------------------------------------------------------------------
static HostHittable *get_h(SceneImpl *s, rt_handle h)
{
    if (!s || h == 0 || h > s->hittables.size()) return nullptr;
    return &s->hittables[h - 1];
}
static bool valid_mat(SceneImpl *s, rt_handle m) { return s && m >= 1 && m <= s->materials.size(); }
static bool valid_tex(SceneImpl *s, rt_handle t) { return s && t >= 1 && t <= s->textures.size(); }
static rt_handle push_h(SceneImpl *s, HostHittable &&h)
{
    s->committed = false;
    s->hittables.push_back(std::move(h));
    return (rt_handle)s->hittables.size();
}
static rt_handle push_tex(SceneImpl *s, const HostTexture &t)
{
    s->committed = false;
    s->textures.push_back(t);
    return (rt_handle)s->textures.size();
}
static rt_handle push_mat(SceneImpl *s, const HostMaterial &m)
{
    s->committed = false;
    s->materials.push_back(m);
    return (rt_handle)s->materials.size();
}

// ------------------------------------------------------------------------------------------------
// BVH construction: R/BvhNode.h:50-90 (recursive median split) + :170-193 (stable insertion sort)
// ------------------------------------------------------------------------------------------------
static int build_tree(SceneImpl *s, HostHittable &bvh, std::vector<uint32_t> &objs, int start, int end)
{
    int me = (int)bvh.tree.size();
    bvh.tree.push_back({});
    Box box = empty_box();
    for (int i = start; i < end; i++) box = box_merge(box, s->hittables[objs[i] - 1].box);
    int axis = longest_axis(box);
    int span = end - start;
    HostHittable::TreeNode node{};
    node.box = box;
    node.left = node.right = -1;
    if (span == 1) {
        node.leaf_a = node.leaf_b = objs[start];
    } else if (span == 2) {
        node.leaf_a = objs[start];
        node.leaf_b = objs[start + 1];
    } else {
        for (int i = start + 1; i < end; i++) {
            uint32_t key = objs[i];
            double key_min = s->hittables[key - 1].box.lo[axis];
            int j = i - 1;
            while (j >= start && key_min < s->hittables[objs[j] - 1].box.lo[axis]) {
                objs[j + 1] = objs[j];
                j--;
            }
            objs[j + 1] = key;
        }
        int mid = start + span / 2;
        node.left = build_tree(s, bvh, objs, start, mid);
        node.right = build_tree(s, bvh, objs, mid, end);
    }
    bvh.tree[me] = node;
    return me;
}

// ------------------------------------------------------------------------------------------------
// flattening
// ------------------------------------------------------------------------------------------------
namespace {
// Coincident surfaces: two identical spheres, or two quads in one plane whose rectangles overlap.  A ray that hits both
// gets the same t twice, and then the ORDER of the tests decides which material it sees: the reference's list keeps the
// first sphere it meets (strict `<`, R/Sphere.h:38,50) and the last quad (inclusive interval, R/Quad.h:59-64).  The
// library's own accelerators (the near-child-first tree of a primitive world, the segmented walk of a composite world and
// its media's candidate lists, the sub-BVH / cooperative scan of a large group) meet the leaves in another order, so they are
// not built over such a set: it keeps the reference's tree or its linear list.
//
// What is compared, per leaf handed in (ties inside one leaf are that leaf's own scan's business, which runs in list order):
//   spheres   Sphere and MovingSphere leaves.  A moving sphere that rests (center0 == center1, time0 != time1) is at c0 + frac * 0
//             = c0 exactly at every time and is keyed as the static sphere it is; one with time0 == time1 has a centre of inf /
//             NaN and is never hit.  Exact comparison.
//   faces     every quad: a Quad leaf, the quads of a list leaf (MakeBox: six), and both behind a Translate / RotateY / Transform chain,
//             in world space.  Two faces that were not transformed are compared bit for bit (surfaces that differ in the last bit
//             do not tie); a transformed face is compared with a tolerance far above its rounding, since finding a tie too
//             many costs only speed.  Rectangles overlap when their (padded) bounding boxes meet.
// One kind of overlap is left alone, or a field of boxes that stand side by side (the ground of the Book-2 final scene) would
// lose its tree: two faces of closed, untransformed MakeBox boxes
//   - that share no area (the boxes touch along an edge or a corner at most: the rays that meet both are a set of measure
//     zero in any pixel), or
//   - whose boxes lie on opposite sides of the shared plane (one's +x face is the other's -x face), both of a material that
//     sends no ray inwards (Lambertian, Metal -- R/Metal.h:29 absorbs what its fuzz turns inwards --, DiffuseLight): every
//     point of the shared area has a solid on either side, and no ray reaches it.  This assumes what the reference's scenes
//     assume: no camera inside a solid box.
// A pair with a triangle in it is decided on the polygons themselves (share_area): a triangle's bounding box is no padded
// rectangle of it, and a tessellated floor, a flat region of a mesh or a height field on a lattice is nothing but coplanar
// faces whose boxes meet.  Two convex polygons of one plane tie only where they share area; meeting in an edge or a vertex is
// the boxes' case above, a set of rays of measure zero.  Quad-quad pairs keep the rule of the boxes that meet.
struct TieFace {
    double n[3], d;        // plane, the normal's sign fixed by its largest component
    double lo[3], hi[3];   // padded bounding box of the rectangle
    bool exact;            // not transformed: n, d, lo, hi are the quad's own
    uint32_t leaf;         // position in `handles`
    int box;               // index into the closed untransformed boxes, or -1
    int axis, end;         // of such a box: the face lies in coordinate `axis` = (end ? mx : mn)[axis]
    int nv;                // 4: a quad Q, Q+u, Q+u+v, Q+v; 3: a triangle Q, Q+u, Q+v
    double p[4][3];        // the corners as computed (fl(Q + u), ...), in world space
};

// Do two convex polygons of one plane (unit normal n) share area?  Separating axes over the in-plane edge normals of both.  An
// exact pair (neither face transformed) that penetrates by at most 2^-40 of the pair's coordinate reach only touches: the
// projections' own rounding is a few 2^-53 of that reach.  A pair with a transformed face errs towards a tie instead: only a gap
// of more than the 1e-4 per transformed face that the rectangles' rule allows separates it.
static bool share_area(const TieFace &x, const TieFace &y)
{
    double pair_reach = 0.0;
    for (const TieFace *f : {&x, &y})
        for (int i = 0; i < f->nv; i++)
            for (int k = 0; k < 3; k++) pair_reach = std::max(pair_reach, std::fabs(f->p[i][k]));
    const bool exact = x.exact && y.exact;
    const double limit = exact ? 0x1p-40 * pair_reach : -((x.exact ? 0.0 : 1e-4) + (y.exact ? 0.0 : 1e-4));
    const D3 n = mk(x.n[0], x.n[1], x.n[2]);
    for (const TieFace *f : {&x, &y})
        for (int i = 0; i < f->nv; i++) {
            const double *a = f->p[i], *b = f->p[(i + 1) % f->nv];
            D3 axis = cross(mk(b[0] - a[0], b[1] - a[1], b[2] - a[2]), n);
            const double len = length(axis);
            if (!(len > 0.0) || !std::isfinite(len)) continue;  // an edge of no length separates nothing
            axis = over(axis, len);
            double lo[2] = {DBL_MAX, DBL_MAX}, hi[2] = {-DBL_MAX, -DBL_MAX};
            int side = 0;
            for (const TieFace *g : {&x, &y}) {
                for (int j = 0; j < g->nv; j++) {
                    const double t = dot(axis, mk(g->p[j][0], g->p[j][1], g->p[j][2]));
                    lo[side] = std::min(lo[side], t);
                    hi[side] = std::max(hi[side], t);
                }
                side++;
            }
            const double depth = std::min(hi[0], hi[1]) - std::max(lo[0], lo[1]);
            if (exact ? depth <= limit : depth < limit) return false;
        }
    return true;
}
struct TieBox {
    double mn[3], mx[3];
    bool opaque;
};

static bool only_primitives(const SceneImpl &s, uint32_t handle)  // a primitive, or a (nested) list / BVH whose members are all primitives
{
    const HostHittable &h = s.hittables[handle - 1];
    if (h.kind == HKind::Sphere || h.kind == HKind::MovingSphere || h.kind == HKind::Quad || h.kind == HKind::Triangle) return true;
    if (h.kind != HKind::List && h.kind != HKind::Bvh) return false;
    for (uint32_t c : h.items)
        if (!only_primitives(s, c)) return false;
    return true;
}

// A list of six quads that bound a box mn < mx as MakeBox builds it (R/Instance.h:166-184), in any order: one quad in each of the
// six face planes, its edges along the two other axes, each starting at a corner coordinate and spanning the rounded extent
// fl(mx - mn) towards the other one (Flattener::box_of_six has the same notion for the lowered quads).
static bool closed_box(const SceneImpl &s, const HostHittable &list, TieBox &b, int axis_of[6], int end_of[6])
{
    if (list.kind != HKind::List || list.items.size() != 6) return false;
    int edge_axis[6][2], seen[3] = {0, 0, 0};
    double edge[6][2];
    for (int f = 0; f < 6; f++) {
        const HostHittable &q = s.hittables[list.items[f] - 1];
        if (q.kind != HKind::Quad || q.material != s.hittables[list.items[0] - 1].material) return false;
        const double o[3] = {q.q.x, q.q.y, q.q.z}, u[3] = {q.u.x, q.u.y, q.u.z}, v[3] = {q.v.x, q.v.y, q.v.z};
        int p = -1, qa = -1;
        for (int k = 0; k < 3; k++) {
            if (!std::isfinite(o[k]) || !std::isfinite(u[k]) || !std::isfinite(v[k])) return false;
            if (u[k] != 0.0) p = p == -1 ? k : -2;
            if (v[k] != 0.0) qa = qa == -1 ? k : -2;
        }
        if (p < 0 || qa < 0 || p == qa) return false;
        const int a = 3 - p - qa;
        axis_of[f] = a;
        edge_axis[f][0] = p;
        edge_axis[f][1] = qa;
        edge[f][0] = u[p];
        edge[f][1] = v[qa];
        if (seen[a] == 0) b.mn[a] = b.mx[a] = o[a];
        else if (seen[a] == 1) {
            b.mn[a] = std::min(b.mn[a], o[a]);
            b.mx[a] = std::max(b.mx[a], o[a]);
        } else return false;
        seen[a]++;
    }
    for (int k = 0; k < 3; k++)
        if (seen[k] != 2 || !(b.mn[k] < b.mx[k])) return false;
    for (int f = 0; f < 6; f++) {
        const HostHittable &q = s.hittables[list.items[f] - 1];
        const double o[3] = {q.q.x, q.q.y, q.q.z};
        end_of[f] = o[axis_of[f]] == b.mx[axis_of[f]] ? 1 : 0;
        for (int e = 0; e < 2; e++) {
            const int k = edge_axis[f][e];
            const double ext = b.mx[k] - b.mn[k];
            if (!(o[k] == b.mn[k] && edge[f][e] == ext) && !(o[k] == b.mx[k] && edge[f][e] == -ext)) return false;
        }
    }
    const uint32_t kind = s.materials[s.hittables[list.items[0] - 1].material - 1].kind;
    b.opaque = kind == MAT_LAMBERTIAN || kind == MAT_METAL || kind == MAT_DIFFUSE_LIGHT;
    return true;
}

static bool has_coincident_primitives(const SceneImpl &s, const std::vector<uint32_t> &handles)
{
    struct Key {
        double v[10];
        uint32_t leaf;
    };
    auto less = [](const Key &a, const Key &b) { return std::lexicographical_compare(a.v, a.v + 10, b.v, b.v + 10); };
    auto same = [](const Key &a, const Key &b) { return std::equal(a.v, a.v + 10, b.v); };
    std::vector<Key> spheres;
    std::vector<TieFace> faces;
    std::vector<TieBox> boxes;
    double reach = 0.0;  // the largest coordinate of a face: scales the tolerance of transformed planes

    auto add_face = [&](const HostHittable &q, const std::vector<const HostHittable *> &chain, uint32_t leaf, int box, int axis, int end) {
        TieFace f{};
        f.exact = chain.empty();
        f.leaf = leaf;
        f.box = box;
        f.axis = axis;
        f.end = end;
        double n[3], d;
        const bool tri = q.kind == HKind::Triangle;
        f.nv = tri ? 3 : 4;
        D3 c[4] = {q.q, add(q.q, q.u), tri ? add(q.q, q.v) : add(add(q.q, q.u), q.v), add(q.q, q.v)};
        if (f.exact) {
            n[0] = q.normal.x; n[1] = q.normal.y; n[2] = q.normal.z;
            d = q.plane_d;
            for (int k = 0; k < 3; k++) {
                f.lo[k] = q.box.lo[k];
                f.hi[k] = q.box.hi[k];
            }
        } else {
            for (D3 &p : c)
                for (size_t k = chain.size(); k-- > 0;) {  // innermost transform first (R/Instance.h:49-50, :142-147)
                    const HostHittable &x = *chain[k];
                    if (x.kind == HKind::Translate) p = add(p, x.offset);
                    else if (x.kind == HKind::RotateY) p = mk(x.cos_t * p.x + x.sin_t * p.z, p.y, -x.sin_t * p.x + x.cos_t * p.z);
                    else p = affine_point(s.transforms[x.xf - 1], p);
                }
            const D3 nn = normalize(cross(sub(c[1], c[0]), sub(c[3], c[0])));
            n[0] = nn.x; n[1] = nn.y; n[2] = nn.z;
            d = dot(nn, c[0]);
            for (int k = 0; k < 3; k++) {
                f.lo[k] = DBL_MAX;
                f.hi[k] = -DBL_MAX;
                for (const D3 &p : c) {  // (a triangle's fourth entry repeats its third corner)
                    f.lo[k] = std::min(f.lo[k], comp(p, k));
                    f.hi[k] = std::max(f.hi[k], comp(p, k));
                }
            }
        }
        if (!std::isfinite(n[0]) || !std::isfinite(n[1]) || !std::isfinite(n[2]) || !std::isfinite(d)) return;  // never hit
        for (int k = 0; k < 3; k++) {
            if (!std::isfinite(f.lo[k]) || !std::isfinite(f.hi[k])) return;
            reach = std::max(reach, std::max(std::fabs(f.lo[k]), std::fabs(f.hi[k])));
        }
        int lead = 0;
        for (int k = 1; k < 3; k++)
            if (std::fabs(n[k]) > std::fabs(n[lead])) lead = k;
        const double sign = n[lead] < 0.0 ? -1.0 : 1.0;
        for (int k = 0; k < 3; k++) f.n[k] = sign * n[k] + 0.0;  // + 0.0: -0.0 -> +0.0
        f.d = sign * d + 0.0;
        for (int i = 0; i < f.nv; i++)
            for (int k = 0; k < 3; k++) f.p[i][k] = comp(c[i], k);
        faces.push_back(f);
    };
    auto add_prims = [&](auto &&self, uint32_t hnd, const std::vector<const HostHittable *> &chain, uint32_t leaf, int box, const int *axis_of,
                         const int *end_of) -> void {
        const HostHittable &h = s.hittables[hnd - 1];
        if (h.kind == HKind::Quad || h.kind == HKind::Triangle) {
            add_face(h, chain, leaf, -1, 0, 0);
        } else if (h.kind == HKind::Sphere || h.kind == HKind::MovingSphere) {
            if (!chain.empty()) return;  // (an instanced sphere is not compared)
            const bool moving = h.kind == HKind::MovingSphere && !(h.c0.x == h.c1.x && h.c0.y == h.c1.y && h.c0.z == h.c1.z && h.t0 != h.t1);
            spheres.push_back({{h.c0.x, h.c0.y, h.c0.z, moving ? h.c1.x : h.c0.x, moving ? h.c1.y : h.c0.y, moving ? h.c1.z : h.c0.z,
                                moving ? h.t0 : 0.0, moving ? h.t1 : 0.0, h.radius, moving ? 1.0 : 0.0}, leaf});
        } else {
            for (size_t k = 0; k < h.items.size(); k++) {
                const HostHittable &c = s.hittables[h.items[k] - 1];
                if (box >= 0 && c.kind == HKind::Quad) add_face(c, chain, leaf, box, axis_of[k], end_of[k]);
                else self(self, h.items[k], chain, leaf, -1, nullptr, nullptr);
            }
        }
    };
    // A face or sphere under a MovingTransform (rt_moving_transform) stands at no one position, and the guard knows no time: such a
    // leaf counts as coincident with every other compared leaf whose box meets its own, which is the swept box of the step with the
    // static steps above it applied.  Too many ties only keep the reference's order.
    std::vector<uint32_t> moving_leaves, compared_leaves;
    for (uint32_t leaf = 0; leaf < handles.size(); leaf++) {
        const HostHittable *h = &s.hittables[handles[leaf] - 1];
        std::vector<const HostHittable *> chain;  // outermost first
        bool moves = false;
        while (is_instance(h->kind)) {
            chain.push_back(h);
            moves |= h->kind == HKind::MovingTransform;
            h = &s.hittables[h->child - 1];
        }
        // a medium's hit is drawn, not found: it ties with nothing.  General nesting gets no library tree in the first place.
        const uint32_t inner = (uint32_t)(h - s.hittables.data()) + 1;
        if (h->kind == HKind::Medium || !only_primitives(s, inner)) continue;
        compared_leaves.push_back(leaf);
        if (moves) {
            moving_leaves.push_back(leaf);
            continue;
        }
        TieBox b;
        int axis_of[6], end_of[6], box = -1;
        if (chain.empty() && closed_box(s, *h, b, axis_of, end_of)) {
            box = (int)boxes.size();
            boxes.push_back(b);
        }
        add_prims(add_prims, inner, chain, leaf, box, axis_of, end_of);
    }

    for (uint32_t m : moving_leaves) {
        const Box &mb = s.hittables[handles[m] - 1].box;
        for (uint32_t o : compared_leaves) {
            if (o == m) continue;
            const Box &ob = s.hittables[handles[o] - 1].box;
            bool meet = true;
            for (int k = 0; k < 3; k++) meet &= mb.lo[k] <= ob.hi[k] && ob.lo[k] <= mb.hi[k];
            if (meet) return true;
        }
    }

    std::sort(spheres.begin(), spheres.end(), less);
    for (size_t a = 0; a < spheres.size(); a++)
        for (size_t b = a + 1; b < spheres.size() && same(spheres[a], spheres[b]); b++)
            if (spheres[a].leaf != spheres[b].leaf) return true;

    // Candidate pairs are faces whose plane offsets d differ by at most tol_d; what such a pair needs besides -- one plane, and
    // rectangles, boxes or polygons that overlap -- fails for certain where the faces' extents along any one axis do not meet.  So
    // the faces sorted by d are cut where two neighbours differ by more than tol_d (no pair crosses such a cut), and each piece is
    // swept along the axis it extends farthest in: a flat mesh of n faces costs its neighbours' pairs, not n^2 / 2.
    std::sort(faces.begin(), faces.end(), [](const TieFace &a, const TieFace &b) { return a.d < b.d; });
    const double tol_n = 1e-9, tol_d = 1e-9 * (1.0 + reach), sweep_pad = 2e-4;  // sweep_pad: the most two transformed faces allow
    auto tie = [&](const TieFace &x, const TieFace &y) {
        if (x.leaf == y.leaf || std::fabs(x.d - y.d) > tol_d) return false;
        bool same_plane = true;
        if (x.exact && y.exact) {
            same_plane = x.d == y.d && x.n[0] == y.n[0] && x.n[1] == y.n[1] && x.n[2] == y.n[2];
        } else {
            for (int k = 0; k < 3; k++) same_plane &= std::fabs(x.n[k] - y.n[k]) <= tol_n;
        }
        if (!same_plane) return false;
        if (x.box >= 0 && y.box >= 0) {
            const TieBox &p = boxes[(size_t)x.box], &q = boxes[(size_t)y.box];
            bool area = true;
            for (int k = 0; k < 3; k++)
                if (k != x.axis) area &= p.mn[k] < q.mx[k] && q.mn[k] < p.mx[k];
            if (!area) return false;                                        // an edge or a corner at most
            if (x.end != y.end && p.opaque && q.opaque) return false;      // a solid on either side
            return true;
        }
        bool overlap = true;
        for (int k = 0; k < 3; k++) overlap &= x.lo[k] - (x.exact ? 0.0 : 1e-4) <= y.hi[k] + (y.exact ? 0.0 : 1e-4) &&
                                               y.lo[k] - (y.exact ? 0.0 : 1e-4) <= x.hi[k] + (x.exact ? 0.0 : 1e-4);
        if (!overlap) return false;
        return (x.nv == 4 && y.nv == 4) || share_area(x, y);  // two quads: the rectangles' boxes; a triangle: the polygons
    };
    for (size_t first = 0; first < faces.size();) {
        size_t last = first + 1;
        while (last < faces.size() && faces[last].d - faces[last - 1].d <= tol_d) last++;
        double lo[3] = {DBL_MAX, DBL_MAX, DBL_MAX}, hi[3] = {-DBL_MAX, -DBL_MAX, -DBL_MAX};
        for (size_t k = first; k < last; k++)
            for (int a = 0; a < 3; a++) {
                lo[a] = std::min(lo[a], faces[k].lo[a]);
                hi[a] = std::max(hi[a], faces[k].hi[a]);
            }
        int ax = 0;
        for (int a = 1; a < 3; a++)
            if (hi[a] - lo[a] > hi[ax] - lo[ax]) ax = a;
        std::sort(faces.begin() + (ptrdiff_t)first, faces.begin() + (ptrdiff_t)last,
                  [ax](const TieFace &a, const TieFace &b) { return a.lo[ax] < b.lo[ax]; });
        for (size_t a = first; a < last; a++)
            for (size_t b = a + 1; b < last && faces[b].lo[ax] <= faces[a].hi[ax] + sweep_pad; b++)
                if (tie(faces[a], faces[b])) return true;
        first = last;
    }
    return false;
}

// A moving sphere whose centre moves lies outside its bounding box (c0 .. c1, R/MovingSphere.h) at ray times outside its own
// [time0, time1]: R/MovingSphere.h:51 does not clamp frac.  Which of such hits a tree culls then depends on the tree, so no
// tree of the library's own may stand in for a list that holds one -- commit does not know the shutter.
static bool has_moving_centre(const SceneImpl &s, const std::vector<uint32_t> &handles)
{
    for (uint32_t hnd : handles) {
        const HostHittable &h = s.hittables[hnd - 1];
        if (h.kind != HKind::MovingSphere) continue;
        const D3 dc = sub(h.c1, h.c0);
        if (dc.x != 0.0 || dc.y != 0.0 || dc.z != 0.0) return true;  // (NaN too)
    }
    return false;
}

struct Flattener {
    SceneImpl &s;
    FlatScene &f;
    std::string err;
    // sub-BVHs are emitted after the world's nodes (the kernel stages nodes [0, n_world_nodes) in LDS)
    struct PendingSubBvh {
        uint32_t object;
        HostHittable tree;
        std::vector<uint32_t> ref_of;
    };
    std::vector<PendingSubBvh> pending;

    // When a BVH world mixes Sphere and MovingSphere leaves, static spheres are stored as moving-sphere rows with a
    // zero displacement (centre(t) = c0 + frac * 0 = c0 exactly), so that a wave's leaf tests run one code path
    // instead of two.  Not done if a centre component is -0.0 (c0 + 0.0 would flip it to +0.0).
    bool unify_spheres = false;
    const bool plain_quads = (s.options & RT_SCENE_PLAIN_QUADS) != 0;

    uint32_t add_primitive(const HostHittable &h, bool world_leaf = false)
    {
        if (h.kind == HKind::Sphere && unify_spheres && world_leaf) {
            f.mspheres.push_back({h.c0.x, h.c0.y, h.c0.z, 0.0, 0.0, 0.0, 0.0, 1.0, h.radius * h.radius});
            f.msphere_aux.push_back({1 / h.radius, h.material - 1, 0});
            return make_ref(REF_MSPHERE, (uint32_t)f.mspheres.size() - 1);
        }
        if (h.kind == HKind::Sphere) {
            f.spheres.push_back({h.c0.x, h.c0.y, h.c0.z, h.radius * h.radius});
            f.sphere_aux.push_back({1 / h.radius, h.material - 1, 0});
            return make_ref(REF_SPHERE, (uint32_t)f.spheres.size() - 1);
        }
        if (h.kind == HKind::MovingSphere) {
            D3 dc = sub(h.c1, h.c0);
            f.mspheres.push_back({h.c0.x, h.c0.y, h.c0.z, dc.x, dc.y, dc.z, h.t0, h.t1 - h.t0, h.radius * h.radius});
            f.msphere_aux.push_back({1 / h.radius, h.material - 1, 0});
            return make_ref(REF_MSPHERE, (uint32_t)f.mspheres.size() - 1);
        }
        f.quads.push_back({h.q.x, h.q.y, h.q.z, h.u.x, h.u.y, h.u.z, h.v.x, h.v.y, h.v.z, h.w.x, h.w.y, h.w.z,
                           h.normal.x, h.normal.y, h.normal.z, h.plane_d});
        // RT_SCENE_PLAIN_QUADS (tests): every quad takes the general test, boxes stay lists of six quads
        // A triangle is the quad's row with the mark that selects its interior rule (flat_scene.h kQuadTriangle).
        AAQuad aa{};
        if (h.kind == HKind::Triangle) {
            aa.code = kQuadTriangle;
            if (h.attr) {  // 1 + the attribute row for now; flatten_scene adds the final number of quad rows (flat_scene.h TriAttrRow)
                f.tri_attr.push_back(s.tri_attr[h.attr - 1]);
                aa.pad = (uint32_t)f.tri_attr.size();
            }
        } else if (!plain_quads) aa = axis_aligned(f.quads.back());
        f.quad_aa.push_back(aa);
        f.quad_mat.push_back(h.material - 1);
        return make_ref(REF_QUAD, (uint32_t)f.quads.size() - 1);
    }

    // Six consecutive quads that are exactly what MakeBox builds for some corners mn < mx (R/Instance.h:166-184: front,
    // right, back, left, top, bottom): every face lies in the plane of one corner coordinate, starts at a corner and
    // spans the rounded extent fl(mx - mn) towards the other one.  Anything else stays a plain list of quads.
    bool box_of_six(uint32_t first, BoxRec &b) const
    {
        static const uint32_t codes[6] = {1 + 3 * 2 + 0, 1 + 3 * 0 + 2, 1 + 3 * 2 + 0, 1 + 3 * 0 + 2, 1 + 3 * 1 + 0, 1 + 3 * 1 + 0};
        for (int k = 0; k < 6; k++)
            if (f.quad_aa[first + k].code != codes[k]) return false;
        const QuadGeom &front = f.quads[first + 0], &back = f.quads[first + 2], &top = f.quads[first + 4];
        const double mn[3] = {front.qx, front.qy, back.qz}, mx[3] = {back.qx, top.qy, front.qz};
        for (int k = 0; k < 3; k++)
            if (!(mn[k] < mx[k]) || !std::isfinite(mn[k]) || !std::isfinite(mx[k])) return false;
        for (int k = 0; k < 6; k++) {
            const QuadGeom &g = f.quads[first + k];
            const double q[3] = {g.qx, g.qy, g.qz}, u[3] = {g.ux, g.uy, g.uz}, v[3] = {g.vx, g.vy, g.vz};
            const int a = (int)(codes[k] - 1) / 3, p = (int)(codes[k] - 1) % 3, qa = 3 - a - p;
            if (q[a] != mn[a] && q[a] != mx[a]) return false;
            const int ax[2] = {p, qa};
            const double ev[2] = {u[p], v[qa]};
            for (int e = 0; e < 2; e++) {
                const double ext = mx[ax[e]] - mn[ax[e]];
                const bool from_min = q[ax[e]] == mn[ax[e]] && ev[e] == ext;
                const bool from_max = q[ax[e]] == mx[ax[e]] && ev[e] == -ext;
                if (!from_min && !from_max) return false;
            }
            b.na[k] = f.quad_aa[first + k].na;
            b.d[k] = f.quad_aa[first + k].d;
        }
        for (int k = 0; k < 3; k++) {
            b.mn[k] = mn[k];
            b.mx[k] = mx[k];
        }
        b.quad_first = first;
        return true;
    }

    // AAQuad of a quad whose edge vectors each lie along one coordinate axis (code 0 otherwise); see flat_scene.h.
    static AAQuad axis_aligned(const QuadGeom &g)
    {
        AAQuad out{};
        const double u[3] = {g.ux, g.uy, g.uz}, v[3] = {g.vx, g.vy, g.vz}, w[3] = {g.wx, g.wy, g.wz}, n[3] = {g.nx, g.ny, g.nz};
        const double q[3] = {g.qx, g.qy, g.qz};
        int p = -1, qa = -1;
        for (int k = 0; k < 3; k++) {
            if (u[k] != 0.0) p = p == -1 ? k : -2;
            if (v[k] != 0.0) qa = qa == -1 ? k : -2;
        }
        if (p < 0 || qa < 0 || p == qa) return out;
        const int a = 3 - p - qa;
        // everything the shortcut drops must be an exact zero, everything it keeps finite
        if (n[p] != 0.0 || n[qa] != 0.0 || w[p] != 0.0 || w[qa] != 0.0) return out;
        if (!std::isfinite(n[a]) || !std::isfinite(w[a]) || !std::isfinite(g.d) || n[a] == 0.0) return out;
        for (int k = 0; k < 3; k++)
            if (!std::isfinite(u[k]) || !std::isfinite(v[k]) || !std::isfinite(q[k])) return out;
        out.na = n[a];
        out.d = g.d;
        out.wa = w[a];
        out.qp = q[p];
        out.qq = q[qa];
        // component a of cross(ph, v) is ph[a+1]*v[a+2] - ph[a+2]*v[a+1]; of cross(u, ph): u[a+1]*ph[a+2] - u[a+2]*ph[a+1]
        const bool p_first = p == (a + 1) % 3;  // (p, q) = (a+1, a+2)
        out.kv = p_first ? v[qa] : -v[qa];
        out.ku = p_first ? u[p] : -u[p];
        out.code = 1u + 3u * (uint32_t)a + (uint32_t)p;
        return out;
    }

    static bool is_primitive(HKind k) { return k == HKind::Sphere || k == HKind::MovingSphere || k == HKind::Quad || k == HKind::Triangle; }

    // Collect the primitives of a (possibly nested) list in visiting order.  A closest-hit scan over a
    // nested list equals the scan over its flattened sequence (R/HittableList.h:39-57 keeps one running
    // closestSoFar), provided the members draw no random numbers -- i.e. are primitives.
    bool collect_list(uint32_t handle, std::vector<uint32_t> &prims)
    {
        const HostHittable &h = s.hittables[handle - 1];
        if (is_primitive(h.kind)) {
            prims.push_back(handle);
            return true;
        }
        if (h.kind == HKind::List || h.kind == HKind::Bvh) {
            // A nested BvhNode over primitives returns the same closest hit as a scan of its leaves.
            for (uint32_t c : h.items)
                if (!collect_list(c, prims)) return false;
            return true;
        }
        err = "unsupported nesting: a list/BVH inside an instance or medium may only contain primitives and lists";
        return false;
    }

    // ---- general nesting: what ObjectRec cannot express stays a tree (flat_scene.h TreeNodeRec) ----
    // [ConstantMedium] -> Translate / RotateY chain -> a primitive or a list / BVH of primitives: the ObjectRec form
    bool fits_flat(uint32_t handle) const
    {
        const HostHittable *h = &s.hittables[handle - 1];
        if (h->kind == HKind::Medium) h = &s.hittables[h->child - 1];
        while (is_instance(h->kind)) h = &s.hittables[h->child - 1];
        if (h->kind == HKind::Medium) return false;
        return only_primitives(s, (uint32_t)(h - s.hittables.data()) + 1);
    }
    // One instance as rows of xforms[] (flat_scene.h Xform; a Transform is kAffineRows of them, a MovingTransform kMovingRows and sets SCENE_MOVING besides SCENE_AFFINE).
    void push_step(std::vector<Xform> &to, const HostHittable &h)
    {
        if (h.kind == HKind::Translate) {
            to.push_back({h.offset.x, h.offset.y, h.offset.z, XF_TRANSLATE, 0});
        } else if (h.kind == HKind::RotateY) {
            to.push_back({h.sin_t, h.cos_t, 0.0, XF_ROTATE_Y, 0});
        } else if (h.kind == HKind::MovingTransform) {  // flat_scene.h kMovingRows has the rows
            const HostMovingAffine &a = s.moving_transforms[h.xf - 1];
            to.push_back({a.t0[0], a.t0[1], a.t0[2], XF_MOVING, 0});
            for (uint32_t r = 0; r < 3; r++) to.push_back({a.L0[3 * r], a.L0[3 * r + 1], a.L0[3 * r + 2], XF_AFFINE_ROW, 1 + r});
            to.push_back({a.dt[0], a.dt[1], a.dt[2], XF_AFFINE_ROW, 4});
            for (uint32_t r = 0; r < 3; r++) to.push_back({a.dL[3 * r], a.dL[3 * r + 1], a.dL[3 * r + 2], XF_AFFINE_ROW, 5 + r});
            to.push_back({a.time0, a.dtime, 0.0, XF_AFFINE_ROW, kMovingRows - 1});
            f.flags |= SCENE_AFFINE | SCENE_MOVING;
        } else {
            const HostAffine &a = s.transforms[h.xf - 1];
            to.push_back({a.t[0], a.t[1], a.t[2], XF_AFFINE, 0});
            for (uint32_t r = 0; r < 3; r++) to.push_back({a.L[3 * r], a.L[3 * r + 1], a.L[3 * r + 2], XF_AFFINE_ROW, 1 + r});
            for (uint32_t r = 0; r < 3; r++) to.push_back({a.Li[3 * r], a.Li[3 * r + 1], a.Li[3 * r + 2], XF_AFFINE_ROW, 4 + r});
            f.flags |= SCENE_AFFINE;
        }
    }
    uint32_t tree_depth_seen = 0;
    // One node of the tree for `handle`, whose Hit is called with the ray transformed by `chain` (outermost first).
    uint32_t lower_tree(uint32_t handle, const std::vector<Xform> &chain, uint32_t depth)
    {
        if (depth > tree_depth_seen) tree_depth_seen = depth;
        const HostHittable &h = s.hittables[handle - 1];
        TreeNodeRec rec{};
        rec.chain_first = (uint32_t)f.xforms.size();
        rec.chain_count = (uint32_t)chain.size();
        f.xforms.insert(f.xforms.end(), chain.begin(), chain.end());
        const uint32_t me = (uint32_t)f.tree_nodes.size();
        f.tree_nodes.push_back(rec);
        if (is_primitive(h.kind)) {
            rec.kind = TN_PRIM;
            rec.a = add_primitive(h);
        } else if (is_instance(h.kind)) {
            std::vector<Xform> inner = chain;
            push_step(inner, h);
            rec.kind = h.kind == HKind::Translate ? TN_TRANSLATE : (h.kind == HKind::RotateY ? TN_ROTATE_Y : TN_TRANSFORM);
            rec.a = lower_tree(h.child, inner, depth + 1);
        } else if (h.kind == HKind::Medium) {
            f.media.push_back({h.neg_inv_density, h.material - 1, kNone, 0.0, 0.0, 0.0, 0.0});
            f.flags |= SCENE_HAS_MEDIA;
            rec.kind = TN_MEDIUM;
            rec.b = (uint32_t)f.media.size() - 1;
            rec.a = lower_tree(h.child, chain, depth + 1);
        } else if (h.kind == HKind::List) {
            rec.kind = TN_LIST;
            std::vector<uint32_t> kids;
            for (uint32_t c : h.items) kids.push_back(lower_tree(c, chain, depth + 1));
            rec.a = (uint32_t)f.tree_items.size();
            rec.b = (uint32_t)kids.size();
            f.tree_items.insert(f.tree_items.end(), kids.begin(), kids.end());
        } else {  // HKind::Bvh
            rec.kind = TN_BVH;
            std::vector<uint32_t> node_of(s.hittables.size() + 1, kNone);
            lower_bvh_leaves(h, chain, depth + 1, node_of);
            rec.a = thread_tree_general(h, 0, kNone, node_of);
        }
        f.tree_nodes[me] = rec;
        return me;
    }
    // Threaded nodes of a BvhNode inside a tree.  Unlike the world's (thread_tree), a child may be a BvhNode OBJECT: the
    // reference's loop cannot tell it from one of its own inner nodes (Hittable::IsBvhNode, R/BvhNode.h:124-143), so it is
    // spliced in as an inner child -- a node may then hold one leaf and one inner child, and a span-1 node over a BvhNode
    // object walks that object's tree twice.  a / b = REF_TREE | tree node for a leaf, the REF_INNER marker for an inner
    // child; the inner children follow the node in order, the first one at n + 1.
    // Leaves are lowered first (lower_bvh_leaves): a leaf may hold BvhNodes of its own, whose nodes must not land between a
    // node and its first inner child.
    void lower_bvh_leaves(const HostHittable &bvh, const std::vector<Xform> &chain, uint32_t depth, std::vector<uint32_t> &node_of)
    {
        for (const auto &tn : bvh.tree) {
            if (tn.left >= 0) continue;
            for (uint32_t hnd : {tn.leaf_a, tn.leaf_b}) {
                const HostHittable &obj = s.hittables[hnd - 1];
                if (obj.kind == HKind::Bvh) lower_bvh_leaves(obj, chain, depth, node_of);
                else if (node_of[hnd] == kNone) node_of[hnd] = lower_tree(hnd, chain, depth);
            }
        }
    }
    uint32_t thread_tree_general(const HostHittable &bvh, int ti, uint32_t escape, const std::vector<uint32_t> &node_of)
    {
        const auto &tn = bvh.tree[ti];
        const uint32_t me = (uint32_t)f.tree_bvh.size();
        f.tree_bvh.push_back({});
        BvhNodeRec rec{};
        rec.xlo = tn.box.lo[0]; rec.xhi = tn.box.hi[0];
        rec.ylo = tn.box.lo[1]; rec.yhi = tn.box.hi[1];
        rec.zlo = tn.box.lo[2]; rec.zhi = tn.box.hi[2];
        rec.escape = escape;
        // the two children, each an inner subtree (own tree node, or a BvhNode object) or a leaf
        struct Kid { bool inner; const HostHittable *owner; int index; uint32_t leaf; } kid[2];
        for (int c = 0; c < 2; c++) {
            if (tn.left >= 0) {
                kid[c] = {true, &bvh, c == 0 ? tn.left : tn.right, 0};
            } else {
                const uint32_t hnd = c == 0 ? tn.leaf_a : tn.leaf_b;
                const HostHittable &obj = s.hittables[hnd - 1];
                if (obj.kind == HKind::Bvh) kid[c] = {true, &obj, 0, 0};
                else kid[c] = {false, nullptr, 0, hnd};
            }
        }
        uint32_t refs[2];
        for (int c = 0; c < 2; c++)
            refs[c] = kid[c].inner ? make_ref(REF_INNER, 0) : make_ref(REF_TREE, node_of[kid[c].leaf]);
        rec.a = refs[0];
        rec.b = refs[1];
        f.tree_bvh[me] = rec;
        // inner children in order; the first one's walk escapes to the second one, the last one's to this node's escape
        const int n_inner = (kid[0].inner ? 1 : 0) + (kid[1].inner ? 1 : 0);
        int seen = 0;
        size_t first_begin = 0, first_end = 0;
        for (int c = 0; c < 2; c++) {
            if (!kid[c].inner) continue;
            seen++;
            if (seen == 1 && n_inner == 2) {
                first_begin = f.tree_bvh.size();
                thread_tree_general(*kid[c].owner, kid[c].index, kNone - 1 /* placeholder */, node_of);
                first_end = f.tree_bvh.size();
            } else {
                if (n_inner == 2)
                    for (size_t k = first_begin; k < first_end; k++)
                        if (f.tree_bvh[k].escape == kNone - 1) f.tree_bvh[k].escape = (uint32_t)f.tree_bvh.size();
                thread_tree_general(*kid[c].owner, kid[c].index, escape, node_of);
            }
        }
        return me;
    }

    // Lower one world leaf to a ref.
    uint32_t lower_leaf(uint32_t handle)
    {
        const HostHittable *h = &s.hittables[handle - 1];
        if (is_primitive(h->kind)) return add_primitive(*h, true);
        if (!fits_flat(handle)) {
            f.flags |= SCENE_HAS_TREES;
            return make_ref(REF_TREE, lower_tree(handle, {}, 1));
        }

        ObjectRec obj{};
        obj.medium = kNone;
        obj.coop_first = kNone;
        obj.coop_boxes = kNone;
        if (h->kind == HKind::Medium) {
            f.media.push_back({h->neg_inv_density, h->material - 1, kNone, 0.0, 0.0, 0.0, 0.0});
            obj.medium = (uint32_t)f.media.size() - 1;
            f.flags |= SCENE_HAS_MEDIA;
            h = &s.hittables[h->child - 1];
            if (h->kind == HKind::Medium) {
                err = "unsupported nesting: ConstantMedium directly inside ConstantMedium";
                return kNone;
            }
        }
        obj.xf_first = (uint32_t)f.xforms.size();
        while (is_instance(h->kind)) {
            push_step(f.xforms, *h);
            h = &s.hittables[h->child - 1];
        }
        obj.xf_count = (uint32_t)f.xforms.size() - obj.xf_first;
        if (h->kind == HKind::Medium) {
            err = "unsupported nesting: ConstantMedium inside an instance transform";
            return kNone;
        }
        if (is_primitive(h->kind)) {
            obj.geom_kind = GEOM_SINGLE;
            obj.first = add_primitive(*h);
            obj.count = 1;
        } else {
            std::vector<uint32_t> prims;
            uint32_t self = (uint32_t)(h - s.hittables.data()) + 1;
            if (!collect_list(self, prims)) return kNone;
            bool all_s = true, all_m = true, all_q = true;
            for (uint32_t p : prims) {
                HKind k = s.hittables[p - 1].kind;
                all_s &= k == HKind::Sphere;
                all_m &= k == HKind::MovingSphere;
                all_q &= k == HKind::Quad || k == HKind::Triangle;  // one table, one loop (GEOM_QUADS); never a box: box_of_six reads the codes
            }
            obj.count = (uint32_t)prims.size();
            if (prims.size() >= kSubBvhMinPrims && !has_coincident_primitives(s, prims) && !has_moving_centre(s, prims)) {
                // A closest-hit scan and a BVH over the same primitives return the same hit (the reference's own
                // invariant, Docs 2-3 BVH :733,:772) when two things hold: primitives draw no random numbers, and every hit
                // lies inside its primitive's box.  A moving sphere breaks the second at ray times outside its interval
                // (has_moving_centre): such a group stays a list scanned in order, as the reference's HittableList does.
                HostHittable sub{};
                sub.kind = HKind::Bvh;
                std::vector<uint32_t> objs = prims;
                build_tree(&s, sub, objs, 0, (int)objs.size());
                std::vector<uint32_t> ref_of(s.hittables.size() + 1, kNone);
                const size_t spheres_before = f.spheres.size();
                for (uint32_t hnd : objs)
                    if (ref_of[hnd] == kNone) ref_of[hnd] = add_primitive(s.hittables[hnd - 1]);
                // all static spheres, each listed once: the rows just added are this group's, contiguously
                if (all_s && f.spheres.size() - spheres_before == prims.size()) {
                    obj.coop_first = (uint32_t)spheres_before;
                    obj.coop_boxes = (uint32_t)f.group_boxes.size();
                    for (size_t g0 = 0; g0 < prims.size(); g0 += kCoopGroup) {
                        GroupBox gb;
                        for (int k = 0; k < 3; k++) {
                            gb.lo[k] = DBL_MAX;
                            gb.hi[k] = -DBL_MAX;
                        }
                        for (size_t k = g0; k < g0 + kCoopGroup && k < prims.size(); k++) {
                            const SphereGeom &sg = f.spheres[spheres_before + k];
                            const double r = std::sqrt(sg.r2), c[3] = {sg.cx, sg.cy, sg.cz};
                            for (int a2 = 0; a2 < 3; a2++) {
                                // outwards by a part in 2^20 of the magnitudes involved: far beyond any rounding of the slab
                                // test or of the sphere's own arithmetic, far below anything that would cost culling power
                                const double pad = 9.5367431640625e-07 * (std::fabs(c[a2]) + r) + 1e-300;
                                gb.lo[a2] = std::fmin(gb.lo[a2], c[a2] - r - pad);
                                gb.hi[a2] = std::fmax(gb.hi[a2], c[a2] + r + pad);
                            }
                        }
                        f.group_boxes.push_back(gb);
                    }
                }
                obj.geom_kind = GEOM_BVH;
                obj.first = kNone;  // patched by emit_pending()
                pending.push_back({(uint32_t)f.objects.size(), std::move(sub), std::move(ref_of)});
            } else if (prims.empty()) {
                obj.geom_kind = GEOM_MIXED;
                obj.first = (uint32_t)f.items.size();
            } else if (all_s || all_m || all_q) {
                obj.geom_kind = all_s ? GEOM_SPHERES : (all_m ? GEOM_MSPHERES : GEOM_QUADS);
                uint32_t first_ref = add_primitive(s.hittables[prims[0] - 1]);
                obj.first = first_ref & kRefIndexMask;
                for (size_t k = 1; k < prims.size(); k++) add_primitive(s.hittables[prims[k] - 1]);
                if (all_q && prims.size() == 6) {
                    BoxRec b{};
                    if (box_of_six(obj.first, b)) {
                        obj.geom_kind = GEOM_BOX;
                        obj.first = (uint32_t)f.boxes.size();
                        f.boxes.push_back(b);
                    }
                }
            } else {
                obj.geom_kind = GEOM_MIXED;
                std::vector<uint32_t> refs;
                for (uint32_t p : prims) refs.push_back(add_primitive(s.hittables[p - 1]));
                obj.first = (uint32_t)f.items.size();
                f.items.insert(f.items.end(), refs.begin(), refs.end());
            }
        }
        // a plain box needs nothing from the object record: the leaf points at the box itself
        if (obj.geom_kind == GEOM_BOX && obj.xf_count == 0 && obj.medium == kNone) return make_ref(REF_BOX, obj.first);
        if (obj.medium != kNone && obj.geom_kind == GEOM_SINGLE && obj.xf_count == 0 && (obj.first >> kRefShift) == REF_SPHERE) {
            const SphereGeom &g = f.spheres[obj.first & kRefIndexMask];
            MediumRec &m = f.media[obj.medium];
            m.sphere = obj.first & kRefIndexMask;
            m.cx = g.cx; m.cy = g.cy; m.cz = g.cz; m.r2 = g.r2;
        }
        f.objects.push_back(obj);
        return make_ref(obj.medium != kNone ? REF_MOBJECT : REF_OBJECT, (uint32_t)f.objects.size() - 1);
    }

    void emit_pending()
    {
        for (auto &job : pending) f.objects[job.object].first = thread_tree(job.tree, 0, kNone, job.ref_of);
        pending.clear();
    }

    // Thread the reference's traversal (R/BvhNode.h:101-158) into escape links.  The reference visits
    // a node, tests leaf children on the spot, descends into the first inner child and stacks the
    // second; the stack therefore always holds the right siblings of the current root path, so "pop"
    // is a static successor: the escape link.
    uint32_t thread_tree(const HostHittable &bvh, int ti, uint32_t escape, const std::vector<uint32_t> &leaf_ref_of_handle)
    {
        const auto &tn = bvh.tree[ti];
        uint32_t me = (uint32_t)f.nodes.size();
        f.nodes.push_back({});
        BvhNodeRec rec{};
        rec.xlo = tn.box.lo[0]; rec.xhi = tn.box.hi[0];
        rec.ylo = tn.box.lo[1]; rec.yhi = tn.box.hi[1];
        rec.zlo = tn.box.lo[2]; rec.zhi = tn.box.hi[2];
        rec.escape = escape;
        if (tn.left < 0) {
            rec.a = leaf_ref_of_handle[tn.leaf_a];
            rec.b = leaf_ref_of_handle[tn.leaf_b];
            f.nodes[me] = rec;
            return me;
        }
        rec.a = rec.b = make_ref(REF_INNER, 0);
        f.nodes[me] = rec;
        // left subtree occupies [me+1, right_index); its escape is the right child
        // we do not know right_index until the left subtree is emitted: patch afterwards
        size_t left_begin = f.nodes.size();
        thread_tree(bvh, tn.left, kNone - 1 /* placeholder */, leaf_ref_of_handle);
        uint32_t right_index = (uint32_t)f.nodes.size();
        for (size_t k = left_begin; k < right_index; k++)
            if (f.nodes[k].escape == kNone - 1) f.nodes[k].escape = right_index;
        thread_tree(bvh, tn.right, escape, leaf_ref_of_handle);
        return me;
    }
};
} // namespace

static void lower_materials(SceneImpl &s, FlatScene &f)
{
    f.materials.clear();
    f.textures.clear();
    for (const HostTexture &t : s.textures) {
        TextureRec r{};
        r.kind = t.kind;
        r.r = t.color.x; r.g = t.color.y; r.b = t.color.z;
        r.s = t.s;
        if (t.kind == TEX_IMAGE || t.kind == TEX_NOISE) f.flags |= SCENE_RICH_TEXTURES;
        if (t.kind == TEX_CHECKER) {
            r.a = t.a - 1;
            r.b_ = t.b - 1;
        } else {
            r.a = t.a;
        }
        f.textures.push_back(r);
    }
    for (const HostMaterial &m : s.materials) {
        MaterialRec r{};
        r.kind = m.kind;
        r.tex = m.texture ? m.texture - 1 : kNone;
        r.r = m.albedo.x; r.g = m.albedo.y; r.b = m.albedo.z;
        r.p = m.p;
        if (m.texture) {
            const HostTexture &t = s.textures[m.texture - 1];
            auto put = [](double *dst, D3 c) { dst[0] = c.x; dst[1] = c.y; dst[2] = c.z; };
            if (t.kind == TEX_SOLID) {
                r.tex_inline = 1;
                put(r.even, t.color);
            } else if (t.kind == TEX_CHECKER && s.textures[t.a - 1].kind == TEX_SOLID && s.textures[t.b - 1].kind == TEX_SOLID) {
                r.tex_inline = 2;
                put(r.even, s.textures[t.a - 1].color);
                put(r.odd, s.textures[t.b - 1].color);
                r.inv_scale = t.s;
            } else if (t.kind == TEX_CHECKER) {
                f.flags |= SCENE_RICH_TEXTURES;  // nested checker: general kernel walks the table
            }
        }
        // U/V are only ever read by ImageTexture::Value; find out whether this material can reach one
        std::vector<uint32_t> todo;
        if (m.texture) todo.push_back(m.texture);
        while (!todo.empty()) {
            const HostTexture &t = s.textures[todo.back() - 1];
            todo.pop_back();
            if (t.kind == TEX_IMAGE) r.needs_uv = 1;
            if (t.kind == TEX_CHECKER) {
                todo.push_back(t.a);
                todo.push_back(t.b);
            }
        }
        f.materials.push_back(r);
    }
    f.images = s.images;
    f.image_bytes = s.image_bytes;
    f.perlin = s.perlin;
}

// ------------------------------------------------------------------------------------------------
// The library's own tree for primitive-only BVH worlds (flat_scene.h FastNodeRec): surface-area heuristic, full sweep
// over the three axes, bottom nodes of one or two primitives; then the eight octant threadings.
// ------------------------------------------------------------------------------------------------
namespace {
struct FastBuilder {
    const std::vector<Box> &boxes;       // the primitives' own boxes (the reference's, padded where thin)
    const std::vector<uint32_t> &refs;   // their leaf refs
    struct Node {
        Box box;
        int left = -1, right = -1;       // children, or -1
        uint32_t a = kNone, b = kNone;   // bottom node: one or two leaf refs
        int axis = 0;
    };
    std::vector<Node> nodes;

    static double area(const Box &b)
    {
        const double dx = b.hi[0] - b.lo[0], dy = b.hi[1] - b.lo[1], dz = b.hi[2] - b.lo[2];
        return 2.0 * (dx * dy + dy * dz + dz * dx);
    }
    int build(std::vector<uint32_t> &idx, size_t lo, size_t hi)
    {
        const int me = (int)nodes.size();
        nodes.push_back({});
        Node node;
        node.box = empty_box();
        for (size_t k = lo; k < hi; k++) node.box = box_merge(node.box, boxes[idx[k]]);
        const size_t n = hi - lo;
        if (n <= 2) {
            node.a = refs[idx[lo]];
            if (n == 2) node.b = refs[idx[lo + 1]];
            nodes[me] = node;
            return me;
        }
        // best split over the three axes: sort by box centre, sweep prefix / suffix areas
        double best_cost = DBL_MAX;
        int best_axis = 0;
        size_t best_at = lo + n / 2;
        std::vector<uint32_t> order(idx.begin() + lo, idx.begin() + hi), best_order;
        std::vector<double> suffix(n + 1);
        for (int axis = 0; axis < 3; axis++) {
            std::stable_sort(order.begin(), order.end(), [&](uint32_t p, uint32_t q) {
                return boxes[p].lo[axis] + boxes[p].hi[axis] < boxes[q].lo[axis] + boxes[q].hi[axis];
            });
            Box acc = empty_box();
            suffix[n] = 0.0;
            for (size_t k = n; k-- > 0;) {
                acc = box_merge(acc, boxes[order[k]]);
                suffix[k] = area(acc);
            }
            acc = empty_box();
            for (size_t k = 1; k < n; k++) {
                acc = box_merge(acc, boxes[order[k - 1]]);
                const double cost = area(acc) * (double)k + suffix[k] * (double)(n - k);
                if (cost < best_cost) {
                    best_cost = cost;
                    best_axis = axis;
                    best_at = lo + k;
                    best_order = order;
                }
            }
        }
        std::copy(best_order.begin(), best_order.end(), idx.begin() + lo);
        node.axis = best_axis;
        node.left = build(idx, lo, best_at);
        node.right = build(idx, best_at, hi);
        nodes[me] = node;
        return me;
    }
    // visiting order for direction octant `oct` (bit k set: direction component k is negative): the child on the side
    // the ray comes from first.  hit[n] = where to go when n's box is hit (inner nodes), esc[n] = where to go otherwise.
    void thread(int n, uint32_t escape, int oct, std::vector<uint16_t> &hit, std::vector<uint16_t> &esc) const
    {
        const Node &nd = nodes[n];
        esc[n] = (uint16_t)escape;
        if (nd.left < 0) {
            // a bottom node parks the lane (its leaves done, the walk goes to esc): the "hit" link says so -- bit 15, and in bits
            // 12-13 the kind of leaf a as the kind-batched kernels sort by it (render.hip leaf_kind) -- so that a node visit needs
            // no look at the leaf refs (kFastMaxNodes keeps node indices below bit 15)
            const uint32_t tag = nd.a >> kRefShift;
            const uint32_t kind = tag == REF_BOX ? 0u : (tag == REF_MOBJECT ? 1u : (tag == REF_OBJECT ? 2u : 3u));
            hit[n] = (uint16_t)(kFastBottom | (kind << 12));
            return;
        }
        const bool negative = (oct >> nd.axis) & 1;
        const int first = negative ? nd.right : nd.left, second = negative ? nd.left : nd.right;
        hit[n] = (uint16_t)first;
        thread(first, (uint32_t)second, oct, hit, esc);
        thread(second, escape, oct, hit, esc);
    }
};
} // namespace

static void build_fast_tree(FlatScene &f, bool reference_tree_only)
{
    f.fast_nodes.clear();
    if (reference_tree_only) return;  // RT_SCENE_REFERENCE_TREE_ONLY, or leaves that coincide (has_coincident_primitives)
    const size_t n = f.world_items.size();
    // (built for list worlds of primitives as well: RT_FLAG_ACCELERATE_LISTS renders them through it)
    if (n < 3 || n > 40000 || !f.objects.empty() || !f.boxes.empty() || !f.tree_nodes.empty()) return;
    for (uint32_t ref : f.world_items) {
        const uint32_t tag = ref >> kRefShift;
        if (tag != REF_SPHERE && tag != REF_MSPHERE && tag != REF_QUAD) return;
    }
    FastBuilder fb{f.leaf_boxes, f.world_items, {}};
    std::vector<uint32_t> idx(n);
    for (size_t k = 0; k < n; k++) idx[k] = (uint32_t)k;
    fb.build(idx, 0, n);
    if (fb.nodes.size() >= kFastMaxNodes) return;
    f.fast_nodes.resize(fb.nodes.size());
    for (size_t k = 0; k < fb.nodes.size(); k++) {
        const FastBuilder::Node &nd = fb.nodes[k];
        FastNodeRec &r = f.fast_nodes[k];
        r.xlo = nd.box.lo[0]; r.xhi = nd.box.hi[0];
        r.ylo = nd.box.lo[1]; r.yhi = nd.box.hi[1];
        r.zlo = nd.box.lo[2]; r.zhi = nd.box.hi[2];
        r.a = nd.left < 0 ? nd.a : make_ref(REF_INNER, 0);
        r.b = nd.left < 0 ? nd.b : make_ref(REF_INNER, 0);
    }
    std::vector<uint16_t> hit(fb.nodes.size()), esc(fb.nodes.size());
    for (int oct = 0; oct < 8; oct++) {
        fb.thread(0, kFastEnd, oct, hit, esc);
        for (size_t k = 0; k < fb.nodes.size(); k++) {
            f.fast_nodes[k].link[oct][0] = hit[k];
            f.fast_nodes[k].link[oct][1] = esc[k];
        }
    }
}

// Cut the trips of sphere_scan32 into segments in list order (flat_scene.h ScanSegment) and store the rows of every run with
// their varying coordinates in the cx and cz slots.  A run is a maximal range of whole trips whose decided rows (finite k) share
// one fp32 centre coordinate bit for bit; undecided rows and padding fit any run.  From each trip on, the axis that reaches
// farthest wins (x before y before z on a tie); a reach below kScanRunMinTrips leaves the trip to a general segment, and no
// later run could have begun at that trip either, since it would have reached at least as far from there.
static void cut_scan_segments(FlatScene &f)
{
    f.scan_segments.clear();
    const size_t trips = (f.sphere_scan.size() + 2 * kScanTripPairs - 1) / (2 * kScanTripPairs);
    struct Shared { bool any, conflict; uint32_t bits; };  // one trip, one axis: the coordinate of its decided rows
    std::vector<Shared> shared(3 * trips, Shared{false, false, 0u});
    for (size_t t = 0; t < trips; t++)
        for (size_t k = 2 * kScanTripPairs * t; k < 2 * kScanTripPairs * (t + 1); k++) {
            const SphereScanPair &pr = f.sphere_scan32[k / 2];
            const int h = (int)(k & 1);
            if (!std::isfinite(pr.k[h])) continue;
            const float c[3] = {pr.cx[h], pr.cy[h], pr.cz[h]};
            for (int a = 0; a < 3; a++) {
                Shared &sh = shared[3 * t + a];
                uint32_t bits;
                std::memcpy(&bits, &c[a], sizeof bits);
                if (sh.any && sh.bits != bits) sh.conflict = true;
                sh.any = true;
                sh.bits = bits;
            }
        }
    size_t t = 0;
    while (t < trips) {
        size_t best_len = 0;
        uint32_t best_axis = kScanAxisNone, best_bits = 0u;
        for (uint32_t a = 0; a < 3; a++) {
            size_t len = 0;
            bool have = false;
            uint32_t bits = 0u;  // a run without a decided row shares +0
            for (size_t u = t; u < trips; u++, len++) {
                const Shared &sh = shared[3 * u + a];
                if (sh.conflict || (sh.any && have && sh.bits != bits)) break;
                if (sh.any) {
                    have = true;
                    bits = sh.bits;
                }
            }
            if (len > best_len) {
                best_len = len;
                best_axis = a;
                best_bits = bits;
            }
        }
        if (best_len >= kScanRunMinTrips) {
            ScanSegment sg{(uint32_t)t, (uint32_t)best_len, best_axis, 0.0f};
            std::memcpy(&sg.c, &best_bits, sizeof sg.c);
            f.scan_segments.push_back(sg);
            for (size_t p = kScanTripPairs * t; p < kScanTripPairs * (t + best_len); p++) {
                SphereScanPair &pr = f.sphere_scan32[p];
                for (int h = 0; h < 2; h++) {
                    if (best_axis == 0) std::swap(pr.cx[h], pr.cy[h]);
                    if (best_axis == 2) std::swap(pr.cz[h], pr.cy[h]);
                }
            }
            t += best_len;
        } else {
            if (!f.scan_segments.empty() && f.scan_segments.back().axis == kScanAxisNone) f.scan_segments.back().n_trips++;
            else f.scan_segments.push_back(ScanSegment{(uint32_t)t, 1u, kScanAxisNone, 0.0f});
            t++;
        }
    }
}

// The window tables of the runs (scan_window_rule.h; flat_scene.h ScanWindowSeg, ScanTripSpan).  Slab and spans come from the
// fp64 centres and radii the reference's test reads (FlatScene::spheres), not from the filter's fp32 rows, and are stored as fp32
// numbers rounded outwards; a row counts as decided exactly where the filter's row does (finite k).  A run gets a table where its
// trips are selective on one of its varying axes (kScanWindowMaxMeanSpan), on the axis where they are most so.
static void build_scan_windows(FlatScene &f)
{
    f.scan_windows.clear();
    f.scan_trip_spans.clear();
    const size_t trips = (f.sphere_scan.size() + 2 * kScanTripPairs - 1) / (2 * kScanTripPairs);
    const float inf = std::numeric_limits<float>::infinity();
    auto down = [](double v) { float x = (float)v; return (double)x > v ? std::nextafterf(x, -INFINITY) : x; };
    auto up = [](double v) { float x = (float)v; return (double)x < v ? std::nextafterf(x, INFINITY) : x; };
    std::vector<ScanWindowSeg> segs(f.scan_segments.size(), ScanWindowSeg{kScanAxisNone, 0.0f, 0.0f, 0u});
    std::vector<ScanTripSpan> spans(trips, ScanTripSpan{-inf, inf});
    bool any = false;
    for (size_t k = 0; k < f.scan_segments.size(); k++) {
        const ScanSegment &sg = f.scan_segments[k];
        if (sg.axis == kScanAxisNone) continue;
        // per trip and axis: the extent of the decided rows; whether the trip holds an undecided row
        struct Extent { double lo, hi; };
        std::vector<Extent> ext(3 * (size_t)sg.n_trips, Extent{INFINITY, -INFINITY});
        std::vector<char> undecided(sg.n_trips, 0);
        for (uint32_t t = 0; t < sg.n_trips; t++)
            for (size_t row = 2 * kScanTripPairs * (size_t)(sg.first_trip + t); row < 2 * kScanTripPairs * (size_t)(sg.first_trip + t + 1); row++) {
                const float fk = f.sphere_scan32[row / 2].k[row & 1];
                if (fk == inf) continue;  // padding
                if (fk == -inf) {
                    undecided[t] = 1;
                    continue;
                }
                const SphereGeom &g = f.spheres[row];
                const double r = std::sqrt(std::fabs(g.r2)) * (1.0 + 0x1p-40), c[3] = {g.cx, g.cy, g.cz};
                for (int a = 0; a < 3; a++) {
                    Extent &e = ext[3 * (size_t)t + a];
                    e.lo = std::fmin(e.lo, c[a] - r);
                    e.hi = std::fmax(e.hi, c[a] + r);
                }
            }
        uint32_t best_axis = kScanAxisNone;
        double best_mean = INFINITY;
        for (uint32_t a = 0; a < 3; a++) {
            if (a == sg.axis) continue;
            double lo = INFINITY, hi = -INFINITY, sum = 0.0;
            size_t counted = 0;
            for (uint32_t t = 0; t < sg.n_trips; t++) {
                const Extent &e = ext[3 * (size_t)t + a];
                if (!(e.lo <= e.hi)) continue;  // no decided row
                lo = std::fmin(lo, e.lo);
                hi = std::fmax(hi, e.hi);
                sum += e.hi - e.lo;
                counted++;
            }
            if (!counted || !(hi - lo > 0.0) || !std::isfinite(hi - lo)) continue;
            const double mean = sum / (double)counted / (hi - lo);
            if (mean <= kScanWindowMaxMeanSpan && mean < best_mean) {
                best_mean = mean;
                best_axis = a;
            }
        }
        if (best_axis == kScanAxisNone) continue;
        double slab_lo = INFINITY, slab_hi = -INFINITY;
        for (uint32_t t = 0; t < sg.n_trips; t++) {
            const Extent &own = ext[3 * (size_t)t + sg.axis], &e = ext[3 * (size_t)t + best_axis];
            slab_lo = std::fmin(slab_lo, own.lo);
            slab_hi = std::fmax(slab_hi, own.hi);
            ScanTripSpan &sp = spans[sg.first_trip + t];
            if (undecided[t]) sp = ScanTripSpan{-inf, inf};
            else if (!(e.lo <= e.hi)) sp = ScanTripSpan{inf, -inf};
            else sp = ScanTripSpan{down(e.lo), up(e.hi)};
        }
        segs[k] = ScanWindowSeg{best_axis, down(slab_lo), up(slab_hi), 0u};
        any = true;
    }
    if (!any) return;
    f.scan_windows = std::move(segs);
    f.scan_trip_spans = std::move(spans);
}

// The segmented walk of a BVH world with composite leaves (flat_scene.h FastOrder / SegMedium): the library's tree over the
// world's surface leaves, every node with the range of leaf positions below it, and the medium leaves in visiting order.
static void build_segment_tree(FlatScene &f, bool reference_tree_only)
{
    f.fast_order.clear();
    f.seg_media.clear();
    f.seg_cand.clear();
    if (reference_tree_only || f.world_kind != WORLD_BVH || !f.fast_nodes.empty()) return;
    const size_t n = f.world_items.size();
    if (n < 4 || n >= kSegEnd || (f.objects.empty() && f.boxes.empty())) return;
    std::vector<Box> boxes;
    std::vector<uint32_t> refs, order_of;
    std::vector<uint32_t> media;
    for (size_t k = 0; k < n; k++) {
        const uint32_t tag = f.world_items[k] >> kRefShift;
        if (tag == REF_TREE) return;  // general nesting: the interpreter's kernels
        if (tag == REF_MOBJECT) {
            media.push_back((uint32_t)k);
            continue;
        }
        boxes.push_back(f.leaf_boxes[k]);
        refs.push_back(f.world_items[k]);
        order_of.push_back((uint32_t)k);
    }
    if (media.size() > kSegMaxMedia || refs.size() < 3) return;
    FastBuilder fb{boxes, refs, {}};
    std::vector<uint32_t> idx(refs.size());
    for (size_t k = 0; k < idx.size(); k++) idx[k] = (uint32_t)k;
    fb.build(idx, 0, idx.size());
    if (fb.nodes.size() >= kFastMaxNodes) return;
    // position of a leaf ref in the world's list (refs are unique: every leaf was lowered once)
    std::unordered_map<uint32_t, uint32_t> position_of;
    for (size_t k = 0; k < refs.size(); k++) position_of[refs[k]] = order_of[k];
    auto position = [&](uint32_t ref) -> uint32_t { return position_of.at(ref); };
    f.fast_nodes.resize(fb.nodes.size());
    f.fast_order.resize(fb.nodes.size());
    for (size_t k = fb.nodes.size(); k-- > 0;) {  // children follow their parent in the array: bottom-up by going backwards
        const FastBuilder::Node &nd = fb.nodes[k];
        FastNodeRec &r = f.fast_nodes[k];
        r.xlo = nd.box.lo[0]; r.xhi = nd.box.hi[0];
        r.ylo = nd.box.lo[1]; r.yhi = nd.box.hi[1];
        r.zlo = nd.box.lo[2]; r.zhi = nd.box.hi[2];
        r.a = nd.left < 0 ? nd.a : make_ref(REF_INNER, 0);
        r.b = nd.left < 0 ? nd.b : make_ref(REF_INNER, 0);
        FastOrder &o = f.fast_order[k];
        if (nd.left < 0) {
            o.oa = (uint16_t)position(nd.a);
            o.ob = nd.b == kNone ? o.oa : (uint16_t)position(nd.b);
            o.omin = std::min(o.oa, o.ob);
            o.omax = std::max(o.oa, o.ob);
        } else {
            const FastOrder &l = f.fast_order[(size_t)nd.left], &rr = f.fast_order[(size_t)nd.right];
            o.oa = o.ob = 0;
            o.omin = std::min(l.omin, rr.omin);
            o.omax = std::max(l.omax, rr.omax);
        }
    }
    std::vector<uint16_t> hit(fb.nodes.size()), esc(fb.nodes.size());
    for (int oct = 0; oct < 8; oct++) {
        fb.thread(0, kFastEnd, oct, hit, esc);
        for (size_t k = 0; k < fb.nodes.size(); k++) {
            f.fast_nodes[k].link[oct][0] = hit[k];
            f.fast_nodes[k].link[oct][1] = esc[k];
        }
    }
    for (uint32_t k : media) {
        SegMedium m{};
        const Box &b = f.leaf_boxes[k];
        for (int a = 0; a < 3; a++) {
            // outwards by a part in 2^20 of the magnitudes involved (and at least the reference's own thin-box padding): far
            // beyond any rounding of the slab test or of the boundary's own arithmetic
            const double pad = 9.5367431640625e-07 * (std::fabs(b.lo[a]) + std::fabs(b.hi[a])) + 1e-4;
            m.lo[a] = b.lo[a] - pad;
            m.hi[a] = b.hi[a] + pad;
        }
        m.order = k;
        m.object = f.world_items[k] & kRefIndexMask;
        m.twice = 0;
        for (uint32_t nd = 0; nd < f.n_world_nodes; nd++)  // the reference's own tree: a span-1 node holds the leaf twice
            if (f.nodes[nd].a == f.world_items[k] && f.nodes[nd].b == f.world_items[k]) m.twice = 1;
        // the surface leaves that reach into the padded box (flat_scene.h SegMedium)
        m.cand_first = (uint32_t)f.seg_cand.size();
        m.cand_count = 0;
        for (size_t j = 0; j < refs.size() && m.cand_count != kNone; j++) {
            const Box &lb = boxes[j];
            bool meets = true;
            for (int a = 0; a < 3; a++) meets &= lb.lo[a] <= m.hi[a] && m.lo[a] <= lb.hi[a];
            if (!meets) continue;
            const uint32_t tag = refs[j] >> kRefShift;
            const bool simple = tag == REF_BOX || tag == REF_SPHERE || tag == REF_MSPHERE || tag == REF_QUAD;
            if (!simple || m.cand_count >= kSegMaxCandidates) {
                m.cand_count = kNone;
                f.seg_cand.resize(m.cand_first);
                break;
            }
            f.seg_cand.push_back({refs[j], order_of[j]});
            m.cand_count++;
        }
        f.seg_media.push_back(m);
    }
    f.flags |= SCENE_SEGMENTED;
}

// ------------------------------------------------------------------------------------------------
// The light table (flat_scene.h LightRow): every primitive with a DiffuseLight material below world leaf `leaf`, found through
// lists, BvhNodes (in their sorted order) and Translate / RotateY, never through a ConstantMedium (its boundary is no surface).
// `chain` = the instances above the primitive, outermost first; their forward transforms -- what the hit record goes through on
// its way back to the world, R/Instance.h:53,137-147 -- are applied innermost first, in fp64, nothing fused (this file is built
// with contraction off).  A RotateY turns points and vectors alike, a Translate moves points only, a Transform (rt_transform) takes
// points through (L p) + t, vectors through L and the normal through Li^T, renormalised; under one, s is the transformed area.
// ------------------------------------------------------------------------------------------------
namespace {
struct LightCollector {
    const SceneImpl &s;
    FlatScene &f;
    std::vector<const HostHittable *> chain;
    std::vector<double> weight;  // strategy 1, parallel to f.lights
    bool too_deep = false;       // an object graph deeper than kLightMaxDepth levels: the commit is refused
    static constexpr int kLightMaxDepth = 64;  // (recursion bound; far beyond kTreeMaxDepth, which the flattener enforces for trees)

    D3 forward(D3 p, bool point) const
    {
        for (size_t k = chain.size(); k-- > 0;) {
            const HostHittable &x = *chain[k];
            if (x.kind == HKind::Translate) {
                if (point) p = add(p, x.offset);
            } else if (x.kind == HKind::RotateY) {
                p = mk((x.cos_t * p.x) + (x.sin_t * p.z), p.y, (-x.sin_t * p.x) + (x.cos_t * p.z));
            } else {
                const HostAffine &a = s.transforms[x.xf - 1];
                p = point ? affine_point(a, p) : mat_rows(a.L, p);
            }
        }
        return p;
    }
    // a unit normal: a RotateY turns it, a Transform takes it through Li^T and renormalises it (include/rtow.h rt_transform)
    D3 forward_normal(D3 n) const
    {
        for (size_t k = chain.size(); k-- > 0;) {
            const HostHittable &x = *chain[k];
            if (x.kind == HKind::RotateY) n = mk((x.cos_t * n.x) + (x.sin_t * n.z), n.y, (-x.sin_t * n.x) + (x.cos_t * n.z));
            else if (x.kind == HKind::Transform) n = affine_normal(s.transforms[x.xf - 1], n);
        }
        return n;
    }
    bool chain_has_transform() const
    {
        for (const HostHittable *x : chain)
            if (x->kind == HKind::Transform) return true;
        return false;
    }
    static void put(double *dst, D3 v) { dst[0] = v.x; dst[1] = v.y; dst[2] = v.z; }

    void walk(uint32_t handle, uint32_t leaf, int depth)
    {
        if (depth > kLightMaxDepth) {
            too_deep = true;
            return;
        }
        const HostHittable &h = s.hittables[handle - 1];
        switch (h.kind) {
        case HKind::Medium: return;
        case HKind::Translate:
        case HKind::RotateY:
        case HKind::Transform:
        case HKind::MovingTransform:  // (holds no light: rt_moving_transform refused an emissive child, so forward() never meets one)
            chain.push_back(&h);
            walk(h.child, leaf, depth + 1);
            chain.pop_back();
            return;
        case HKind::List:
        case HKind::Bvh:
            for (uint32_t c : h.items) walk(c, leaf, depth + 1);
            return;
        default: break;
        }
        const HostMaterial &m = s.materials[h.material - 1];
        if (m.kind != MAT_DIFFUSE_LIGHT) return;
        LightRow r{};
        r.mat = h.material - 1;
        r.leaf = leaf;
        double area;
        if (h.kind == HKind::Sphere || h.kind == HKind::MovingSphere) {
            const double pi = 3.1415926535897932385;
            put(r.a, forward(h.c0, true));
            r.s = h.radius;
            area = 4.0 * pi * (h.radius * h.radius);
            r.kind = LIGHT_SPHERE;
            if (h.kind == HKind::MovingSphere) {
                r.kind = LIGHT_MSPHERE;
                put(r.b, forward(sub(h.c1, h.c0), false));  // MSphereGeom's dc, turned
                r.c[0] = h.t0;
                r.c[1] = h.t1 - h.t0;
            }
        } else {
            put(r.a, forward(h.q, true));
            put(r.b, forward(h.u, false));
            put(r.c, forward(h.v, false));
            put(r.n, forward_normal(h.normal));
            area = length(cross(h.u, h.v));  // of the primitive as constructed: Translate and RotateY are rigid
            if (chain_has_transform()) area = length(cross(mk(r.b[0], r.b[1], r.b[2]), mk(r.c[0], r.c[1], r.c[2])));  // of the world-space row
            r.kind = LIGHT_QUAD;
            if (h.kind == HKind::Triangle) {
                r.kind = LIGHT_TRIANGLE;
                area = 0.5 * area;
            }
            r.s = area;
        }
        double brightest = 1.0;  // any texture but a solid colour
        if (m.texture && s.textures[m.texture - 1].kind == TEX_SOLID) {
            const D3 c = s.textures[m.texture - 1].color;
            brightest = std::fmax(c.x, std::fmax(c.y, c.z));
        }
        f.lights.push_back(r);
        weight.push_back(area * brightest);
    }

    // cumulative tables: entry k = (w_0 + ... + w_k) / total, summed in order; the last entry exactly 1.0
    void finish()
    {
        const size_t n = f.lights.size(), padded = (n + 1) & ~(size_t)1;
        double total = 0.0;
        bool usable = n > 0;
        for (double w : weight) {
            usable = usable && std::isfinite(w) && w >= 0.0;
            total += w;
        }
        usable = usable && std::isfinite(total) && total > 0.0;  // otherwise strategy 1 is strategy 0
        for (int st = 0; st < 2; st++) {
            std::vector<double> &cdf = f.light_cdf[st];
            cdf.assign(padded, 1.0);
            double run = 0.0;
            for (size_t k = 0; k + 1 < n; k++) {
                if (st == 1 && usable) {
                    run += weight[k];
                    cdf[k] = std::fmin(run / total, 1.0);
                } else {
                    cdf[k] = (double)(k + 1) / (double)n;
                }
            }
        }
    }
};
}  // namespace

// The environment's record and, for an image, the importance sampler's tables (include/rtow.h rt_scene_dump_environment_cdf states
// the rule; tests/environment_restated.py restates it to the bit).
static void build_environment(const SceneImpl &s, FlatScene &f)
{
    const HostEnvironment &h = s.environment;
    f.flags |= SCENE_ENVIRONMENT;
    EnvRec &r = f.env;
    // the environment as a light of the direct estimators: the shares of a light sample, fixed here (f.lights is complete)
    r.light_share = 0.0;
    r.table_share = 1.0;
    if (s.environment_light > 0.0) {
        f.flags |= SCENE_ENVIRONMENT_LIGHT;
        r.light_share = f.lights.empty() ? 1.0 : s.environment_light;
        r.table_share = f.lights.empty() ? 0.0 : 1.0 - s.environment_light;
    }
    std::memcpy(r.intensity, h.intensity, sizeof r.intensity);
    std::memcpy(r.rot, h.rotation, sizeof r.rot);
    r.texture = h.texture ? h.texture - 1 : kNone;
    r.width = h.width;
    r.height = h.height;
    f.env_rgb = h.rgb;
    const unsigned char *bytes = nullptr;
    if (h.texture) {
        const HostTexture &t = s.textures[h.texture - 1];
        r.width = r.height = 0;
        if (t.kind != TEX_IMAGE || s.images[t.a].height <= 0 || s.images[t.a].width <= 0) return;  // no image: no distribution
        r.width = s.images[t.a].width;
        r.height = s.images[t.a].height;
        bytes = s.image_bytes.data() + s.images[t.a].offset;
    }
    const size_t W = (size_t)r.width, H = (size_t)r.height;
    const double pi = 3.1415926535897932385, cs = 1.0 / 255.0;
    std::vector<double> weight(W * H), row_sum(H);
    double total = 0.0;
    for (size_t j = 0; j < H; j++) {
        const double sn = std::sin(pi * ((double)j + 0.5) / (double)H);
        double sum = 0.0;
        for (size_t i = 0; i < W; i++) {
            double brightest = 0.0;
            for (int c = 0; c < 3; c++) {
                const size_t at = (j * W + i) * 3 + (size_t)c;
                const double value = bytes ? cs * bytes[at] : (double)h.rgb[at];
                const double x = h.intensity[c] * value;
                brightest = c == 0 || x > brightest ? x : brightest;
            }
            weight[j * W + i] = brightest * sn;
            sum += weight[j * W + i];
        }
        row_sum[j] = sum;
        total += sum;
    }
    if (!(std::isfinite(total) && total > 0.0)) return;
    f.env_mcdf.assign(H, 1.0);
    f.env_ccdf.assign(W * H, 1.0);
    double run = 0.0;
    for (size_t j = 0; j + 1 < H; j++) {
        run += row_sum[j];
        f.env_mcdf[j] = run / total;
    }
    for (size_t j = 0; j < H; j++) {
        if (!(row_sum[j] > 0.0)) continue;  // never consulted
        double part = 0.0;
        for (size_t i = 0; i + 1 < W; i++) {
            part += weight[j * W + i];
            f.env_ccdf[j * W + i] = part / row_sum[j];
        }
    }
    r.has_distribution = 1;
}

int flatten_scene(SceneImpl &s)
{
    if (s.world == 0) return fail(RT_ERR_STATE, "rt_scene_commit: no world set (rt_scene_set_world)");
    if (!s.has_camera) return fail(RT_ERR_STATE, "rt_scene_commit: no camera set (rt_scene_set_camera)");
    if (s.launches_in_flight > 0)
        return fail(RT_ERR_STATE, "rt_scene_commit: a render of this scene is in flight (rt_render_finish it first)");
    s.committed = false;
    s.generation++;  // device copies made from the previous tables are stale from here on
    s.flat = FlatScene{};
    FlatScene &f = s.flat;
    lower_materials(s, f);
    Flattener fl{s, f, {}, {}};

    const HostHittable &world = s.hittables[s.world - 1];
    std::vector<uint32_t> leaves;  // hittable handles, final order
    if (world.kind == HKind::Bvh) {
        f.world_kind = WORLD_BVH;
        leaves = world.items;
    } else if (world.kind == HKind::List) {
        f.world_kind = WORLD_LIST;
        leaves = world.items;
    } else {
        f.world_kind = WORLD_LIST;  // a lone hittable as world behaves as a list of one
        leaves.push_back(s.world);
    }
    // A BvhNode OBJECT among a BvhNode world's leaves is walked by the reference as part of the world's own tree
    // (Hittable::IsBvhNode, R/BvhNode.h:124-143), not called as a leaf.  Over primitives only that makes no difference
    // (it becomes a group leaf); over composites the order of the leaf calls -- hence of the media's random draws -- does,
    // and the whole world is then kept as one tree (flat_scene.h TreeNodeRec, thread_tree_general).
    if (world.kind == HKind::Bvh) {
        bool nested_bvh = false;
        for (uint32_t h : leaves) nested_bvh |= s.hittables[h - 1].kind == HKind::Bvh && !fl.fits_flat(h);
        if (nested_bvh) {
            f.world_kind = WORLD_LIST;
            leaves.assign(1, s.world);
        }
    }
    if (f.world_kind == WORLD_BVH) {
        bool any_static = false, any_moving = false, negative_zero = false;
        for (uint32_t h : leaves) {
            const HostHittable &hh = s.hittables[h - 1];
            any_moving |= hh.kind == HKind::MovingSphere;
            if (hh.kind == HKind::Sphere) {
                any_static = true;
                negative_zero |= std::signbit(hh.c0.x) && hh.c0.x == 0.0;
                negative_zero |= std::signbit(hh.c0.y) && hh.c0.y == 0.0;
                negative_zero |= std::signbit(hh.c0.z) && hh.c0.z == 0.0;
            }
        }
        fl.unify_spheres = any_static && any_moving && !negative_zero;
    }
    std::vector<uint32_t> ref_of_handle(s.hittables.size() + 1, kNone);
    for (uint32_t h : leaves) {
        uint32_t ref = fl.lower_leaf(h);
        if (ref == kNone) return fail(RT_ERR_UNSUPPORTED, fl.err);
        ref_of_handle[h] = ref;
        f.world_items.push_back(ref);
        f.leaf_boxes.push_back(s.hittables[h - 1].box);
        const HKind hk = s.hittables[h - 1].kind;
        f.leaf_kinds.push_back(hk == HKind::Sphere ? 0 : (hk == HKind::MovingSphere ? 1 : (hk == HKind::Quad ? 2 : (hk == HKind::Triangle ? 4 : 3))));
    }
    if (f.world_kind == WORLD_BVH) {
        if (world.tree.empty()) return fail(RT_ERR_INVALID, "BvhNode world has no nodes");
        fl.thread_tree(world, 0, kNone, ref_of_handle);
        f.n_world_nodes = (uint32_t)f.nodes.size();
        // Ray queries report which world leaf was hit: per node of the world's tree, the positions among the leaves of a bottom
        // node's two.  build_tree halves [start, end) of the sorted leaves and thread_tree numbers the nodes in the same
        // preorder, so the ranges are recomputed rather than looked up by handle (a handle may be listed twice).
        f.node_leaf_pos.assign(2 * (size_t)f.n_world_nodes, kNone);
        uint32_t next_node = 0;
        auto number = [&](auto &&self, int ti, uint32_t start, uint32_t end) -> void {
            const auto &tn = world.tree[(size_t)ti];
            const uint32_t me = next_node++;
            if (tn.left < 0) {
                f.node_leaf_pos[2 * (size_t)me] = start;
                f.node_leaf_pos[2 * (size_t)me + 1] = end - 1;  // span 1: the same leaf twice
                return;
            }
            const uint32_t mid = start + (end - start) / 2;
            self(self, tn.left, start, mid);
            self(self, tn.right, mid, end);
        };
        number(number, 0, 0u, (uint32_t)leaves.size());
    } else {
        bool all_spheres = !f.world_items.empty();
        for (size_t k = 0; k < f.world_items.size(); k++) all_spheres &= f.world_items[k] == make_ref(REF_SPHERE, (uint32_t)k);
        if (all_spheres && f.spheres.size() == f.world_items.size()) f.flags |= SCENE_LIST_ALL_SPHERES;
    }
    {
        LightCollector lc{s, f, {}, {}};
        for (size_t k = 0; k < leaves.size(); k++) lc.walk(leaves[k], (uint32_t)k, 0);
        if (lc.too_deep)
            return fail(RT_ERR_UNSUPPORTED, "object nesting deeper than " + std::to_string(LightCollector::kLightMaxDepth) +
                                                " levels (the walk that collects the lights is bounded)");
        lc.finish();
    }
    fl.emit_pending();
    if (fl.tree_depth_seen > kTreeMaxDepth)
        return fail(RT_ERR_UNSUPPORTED, "object nesting deeper than " + std::to_string(kTreeMaxDepth) +
                                            " levels (the interpreter's stack; the reference's recursion is bounded by its 32 KiB stack)");
    {
        // What testing every leaf once costs, in half sphere tests (sphere 2, quad 3, box 12, a transform chain +4): the
        // launcher scans a small BVH world instead of walking it when this stays under a budget.  Measured: 16 spheres
        // scan 1.3x faster than they walk, 24 spheres and 8 free-standing boxes slower; the Cornell box (6 quads, 2
        // instanced boxes, rays that cross every node's box) 1.4x faster.
        uint64_t cost = 0;
        for (uint32_t ref : f.world_items) {
            const uint32_t tag = ref >> kRefShift, idx = ref & kRefIndexMask;
            if (tag == REF_SPHERE || tag == REF_MSPHERE) cost += 2;
            else if (tag == REF_QUAD) cost += 3;
            else if (tag == REF_BOX) cost += 12;
            else if (tag == REF_TREE) cost += 1000;
            else {
                const ObjectRec &o = f.objects[idx];
                cost += o.xf_count ? 4 : 0;
                if (o.geom_kind == GEOM_BOX) cost += 12;
                else if (o.geom_kind == GEOM_BVH) cost += 1000;
                else cost += 3ull * o.count;
            }
        }
        f.scan_cost = cost > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)cost;
    }
    {
        const bool reference_only = (s.options & RT_SCENE_REFERENCE_TREE_ONLY) != 0 || has_coincident_primitives(s, leaves);
        build_fast_tree(f, reference_only);
        build_segment_tree(f, reference_only);
    }
    {
        // Rows of the list scan's conservative filter (render.hip filter_four): centre and |c|^2 - r^2, and the
        // scene's reach max(|c| + r) that bounds the filter's rounding error.  A non-finite row becomes (0, 0, 0, -inf):
        // such a sphere passes the filter for every ray and the exact test decides.
        f.sphere_scan.clear();
        f.scan_reach = 0.0;
        for (const SphereGeom &g : f.spheres) {
            const long double cc = (long double)g.cx * g.cx + (long double)g.cy * g.cy + (long double)g.cz * g.cz;
            double k = (double)(cc - (long double)g.r2);
            double reach = std::sqrt((double)cc) + std::sqrt(std::fabs(g.r2));
            if (!std::isfinite(k) || !std::isfinite(reach)) {
                f.sphere_scan.push_back(SphereScanRow{0.0, 0.0, 0.0, -std::numeric_limits<double>::infinity()});
                continue;
            }
            f.sphere_scan.push_back(SphereScanRow{g.cx, g.cy, g.cz, k});
            f.scan_reach = std::max(f.scan_reach, reach);
        }
        f.scan_reach *= 1.0 + 0x1p-40;  // the two square roots above were rounded
        // The packed fp32 form (flat_scene.h SphereScanPair).  Its margin grows with the square of the reach it has to cover, so
        // the few spheres that lie far outside the bulk -- the Book-1 ground sphere: |c| + r = 2000 in a scene of 15 -- are not
        // decided by it at all (k = -inf: always on to the exact test); the bulk is what stays within four times the median reach.
        {
            std::vector<double> reach(f.sphere_scan.size(), 0.0);
            for (size_t k = 0; k < f.sphere_scan.size(); k++) {
                const SphereScanRow &r = f.sphere_scan[k];
                const SphereGeom &g = f.spheres[k];
                reach[k] = std::isfinite(r.k) ? std::sqrt(r.cx * r.cx + r.cy * r.cy + r.cz * r.cz) + std::sqrt(std::fabs(g.r2)) : 0.0;
            }
            std::vector<double> sorted = reach;
            std::sort(sorted.begin(), sorted.end());
            const double bulk = sorted.empty() ? 0.0 : 4.0 * sorted[sorted.size() / 2];
            f.scan_reach32 = 0.0;
            f.sphere_scan32.assign(scan32_padded_pairs(f.sphere_scan.size()), SphereScanPair{});
            const float inf = std::numeric_limits<float>::infinity();
            for (size_t k = 0; k < 2 * f.sphere_scan32.size(); k++) {
                SphereScanPair &pr = f.sphere_scan32[k / 2];
                const int h = (int)(k & 1);
                if (k >= f.sphere_scan.size()) {  // padding: never passes
                    pr.cx[h] = pr.cy[h] = pr.cz[h] = 0.0f;
                    pr.k[h] = inf;
                    continue;
                }
                const SphereScanRow &r = f.sphere_scan[k];
                const bool decided = std::isfinite(r.k) && reach[k] <= bulk && reach[k] < 1e15;
                pr.cx[h] = decided ? (float)r.cx : 0.0f;
                pr.cy[h] = decided ? (float)r.cy : 0.0f;
                pr.cz[h] = decided ? (float)r.cz : 0.0f;
                pr.k[h] = decided ? (float)r.k : -inf;
                if (decided) f.scan_reach32 = std::max(f.scan_reach32, reach[k]);
            }
            f.scan_reach32 *= 1.0 + 0x1p-20;
            cut_scan_segments(f);
            build_scan_windows(f);
        }
    }
    {
        bool unit_time = !f.mspheres.empty();
        for (const MSphereGeom &m : f.mspheres) unit_time &= (m.t0 == 0.0 && m.dt == 1.0);
        if (unit_time) f.flags |= SCENE_MS_UNIT_TIME;
        // The rows whose hits may leave their boxes, for the launcher's test of the shutter (FlatScene::ms_intervals).  A row
        // with dc == 0 is where its box is at every time; one with dt == 0 has a centre of inf / NaN and is never hit.
        for (const MSphereGeom &m : f.mspheres) {
            if ((m.dcx == 0.0 && m.dcy == 0.0 && m.dcz == 0.0) || m.dt == 0.0) continue;
            const double v[8] = {m.c0x, m.c0y, m.c0z, m.dcx, m.dcy, m.dcz, m.t0, m.dt};
            bool finite = true;
            for (double x : v) finite &= std::isfinite(x);
            if (finite) f.ms_intervals.push_back({m.t0, m.dt});
            else f.ms_nonfinite = true;
        }
        auto before = [](const MsInterval &a, const MsInterval &b) { return a.t0 < b.t0 || (a.t0 == b.t0 && a.dt < b.dt); };
        auto same = [](const MsInterval &a, const MsInterval &b) { return a.t0 == b.t0 && a.dt == b.dt; };
        std::sort(f.ms_intervals.begin(), f.ms_intervals.end(), before);
        f.ms_intervals.erase(std::unique(f.ms_intervals.begin(), f.ms_intervals.end(), same), f.ms_intervals.end());
        // A BVH world of nothing but spheres and unit-time moving spheres: thin waves scan all of them together instead of
        // walking (order-independent: no leaf draws random numbers).  The planes hold the leaves in leaf order, a static
        // sphere as a moving one that does not move (c0 + t * 0 = c0 exactly; not done when a centre component is -0.0).
        bool all_ms = f.world_kind == WORLD_BVH && !f.world_items.empty() && (f.mspheres.empty() || unit_time) && f.quads.empty() &&
                      f.objects.empty() && f.boxes.empty();
        for (size_t k = 0; all_ms && k < f.world_items.size(); k++) {
            const uint32_t tag = f.world_items[k] >> kRefShift, idx = f.world_items[k] & kRefIndexMask;
            all_ms = tag == REF_MSPHERE || tag == REF_SPHERE;
            if (tag == REF_SPHERE) {
                const SphereGeom &g = f.spheres[idx];
                all_ms = !(g.cx == 0.0 && std::signbit(g.cx)) && !(g.cy == 0.0 && std::signbit(g.cy)) && !(g.cz == 0.0 && std::signbit(g.cz));
            }
        }
        if (all_ms) {
            const size_t n = f.world_items.size(), np = (n + 63) & ~(size_t)63;
            f.ms_padded = (uint32_t)np;
            f.ms_planes.assign(7 * np, 0.0);
            for (size_t k = 0; k < np; k++) {
                const uint32_t ref = f.world_items[k < n ? k : 0];  // padding repeats leaf 0; the scan guards by index
                double row[7];
                if ((ref >> kRefShift) == REF_MSPHERE) {
                    const MSphereGeom &g = f.mspheres[ref & kRefIndexMask];
                    const double r7[7] = {g.c0x, g.c0y, g.c0z, g.dcx, g.dcy, g.dcz, g.r2};
                    std::memcpy(row, r7, sizeof row);
                } else {
                    const SphereGeom &g = f.spheres[ref & kRefIndexMask];
                    const double r7[7] = {g.cx, g.cy, g.cz, 0.0, 0.0, 0.0, g.r2};
                    std::memcpy(row, r7, sizeof row);
                }
                for (int p2 = 0; p2 < 7; p2++) f.ms_planes[(size_t)p2 * np + k] = row[p2];
            }
            f.flags |= SCENE_WORLD_MSPHERES;
        }
    }
    if (!f.tri_attr.empty()) {  // the attribute rows stand behind the quad rows on the device: AAQuad::pad = the row's index there
        for (AAQuad &a : f.quad_aa)
            if (a.code == kQuadTriangle && a.pad) a.pad += (uint32_t)f.quads.size() - 1u;
        f.flags |= SCENE_VERTEX_ATTR;
    }
    if (s.has_environment) build_environment(s, f);
    s.committed = true;
    return RT_OK;
}

SceneImpl::~SceneImpl()
{
    if (launches_in_flight > 0 || !films_in_flight.empty()) wait_for_films_in_flight(*this);  // kernels still read the tables
    for (DeviceTables *t : device)
        if (t) release_device_tables(t);
}

} // namespace rtow

// ================================================================================================
// C-ABI: construction
// ================================================================================================
using namespace rtow;

static inline SceneImpl *S(rt_scene *s) { return reinterpret_cast<SceneImpl *>(s); }

extern "C" {

const char *rt_last_error(void) { return g_error.c_str(); }
const char *rt_version(void) { return "rtow-hip 0.1 (gfx950)"; }

rt_rng *rt_rng_create_salted(uint64_t seed, uint64_t sequence, int salt_kind)
{
    RngImpl *r = new RngImpl;
    r->state = xorwow_seed(seed, salt_kind ? kSaltRocrand : kSaltCurandDevice);
    if (sequence) xorwow_skip_sequences(host_jump_table(), sequence, r->state);
    return reinterpret_cast<rt_rng *>(r);
}
rt_rng *rt_rng_create(uint64_t seed, uint64_t sequence) { return rt_rng_create_salted(seed, sequence, 0); }
rt_rng *rt_rng_create_from_state(const uint32_t in6[6])
{
    if (!in6) {
        fail(RT_ERR_INVALID, "rt_rng_create_from_state: null state");
        return nullptr;
    }
    RngImpl *r = new RngImpl;
    r->state.d = in6[0]; r->state.v0 = in6[1]; r->state.v1 = in6[2]; r->state.v2 = in6[3]; r->state.v3 = in6[4]; r->state.v4 = in6[5];
    return reinterpret_cast<rt_rng *>(r);
}
void rt_rng_destroy(rt_rng *rng) { delete reinterpret_cast<RngImpl *>(rng); }
float rt_rng_uniform(rt_rng *rng) { return xorwow_uniform(reinterpret_cast<RngImpl *>(rng)->state); }
uint32_t rt_rng_next_u32(rt_rng *rng) { return xorwow_next(reinterpret_cast<RngImpl *>(rng)->state); }
void rt_rng_state(const rt_rng *rng, uint32_t out6[6])
{
    const Xorwow &s = reinterpret_cast<const RngImpl *>(rng)->state;
    out6[0] = s.d; out6[1] = s.v0; out6[2] = s.v1; out6[3] = s.v2; out6[4] = s.v3; out6[5] = s.v4;
}

rt_scene *rt_scene_create(void) { return reinterpret_cast<rt_scene *>(new SceneImpl); }
int rt_scene_set_options(rt_scene *scene, uint32_t options)
{
    if (!scene) return fail(RT_ERR_INVALID, "rt_scene_set_options: null scene");
    if (options & ~(uint32_t)(RT_SCENE_PLAIN_QUADS | RT_SCENE_REFERENCE_TREE_ONLY)) return fail(RT_ERR_INVALID, "rt_scene_set_options: unknown option bit");
    S(scene)->options = options;
    S(scene)->committed = false;  // takes effect with the next rt_scene_commit
    return RT_OK;
}
void rt_scene_destroy(rt_scene *scene) { delete S(scene); }

// ---- textures ----
rt_handle rt_solid_color(rt_scene *s, double r, double g, double b)
{
    if (!s) return 0;
    HostTexture t{};
    t.kind = TEX_SOLID;
    t.color = mk(r, g, b);
    return push_tex(S(s), t);
}
rt_handle rt_checker_texture(rt_scene *s, double scale, rt_handle even, rt_handle odd)
{
    if (!valid_tex(S(s), even) || !valid_tex(S(s), odd)) {
        set_error("rt_checker_texture: invalid texture handle");
        return 0;
    }
    HostTexture t{};
    t.kind = TEX_CHECKER;
    t.s = 1.0 / scale;  // Texture.h:64
    t.a = even;
    t.b = odd;
    return push_tex(S(s), t);
}
rt_handle rt_image_texture(rt_scene *s, const unsigned char *rgb, int width, int height)
{
    if (!s) return 0;
    SceneImpl *sc = S(s);
    ImageRec im{};
    im.offset = sc->image_bytes.size();
    if (rgb && width > 0 && height > 0) {
        im.width = width;
        im.height = height;
        sc->image_bytes.insert(sc->image_bytes.end(), rgb, rgb + (size_t)width * height * 3);
    } else {
        im.width = 0;
        im.height = 0;  // Texture.h:113-114: no data => cyan
    }
    sc->images.push_back(im);
    HostTexture t{};
    t.kind = TEX_IMAGE;
    t.a = (uint32_t)sc->images.size() - 1;
    return push_tex(sc, t);
}
void rt_rtwimage_bytes(const unsigned char *in, size_t count, unsigned char *out)
{
    // stbi__ldr_to_hdr: (float)(pow(byte / 255.0f, l2h_gamma = 2.2f) * l2h_scale = 1.0f)   [stb_image.h:1869]
    // RtwImage::FloatToByte: <= 0 -> 0, >= 1 -> 255, else (unsigned char)(256.0f * v)     [R/RtwImage.h:100-105]
    unsigned char lut[256];
    for (int b = 0; b < 256; b++) {
        float v = (float)(std::pow((double)((float)b / 255.0f), (double)2.2f) * (double)1.0f);
        lut[b] = v <= 0.0f ? 0 : (1.0f <= v ? 255 : (unsigned char)(256.0f * v));
    }
    for (size_t k = 0; k < count; k++) out[k] = lut[in[k]];
}

rt_handle rt_noise_texture(rt_scene *s, double scale, rt_rng *rng)
{
    if (!s || !rng) {
        set_error("rt_noise_texture: scene and rng are required");
        return 0;
    }
    SceneImpl *sc = S(s);
    Xorwow &st = reinterpret_cast<RngImpl *>(rng)->state;
    PerlinRec p{};
    // Perlin.h:27-35: 256 unit vectors from RandomVector(-1, 1) (arguments drawn left to right), then
    // three Fisher-Yates permutations (Perlin.h:105-116: int(uniform * (i + 1)) in fp32, clamped to i).
    for (int i = 0; i < 256; i++) {
        double range = 1.0 - (-1.0);
        double a = -1.0 + range * (double)xorwow_uniform(st);
        double b = -1.0 + range * (double)xorwow_uniform(st);
        double c = -1.0 + range * (double)xorwow_uniform(st);
        D3 u = normalize(mk(a, b, c));
        p.vec[i][0] = u.x; p.vec[i][1] = u.y; p.vec[i][2] = u.z;
    }
    int32_t *perms[3] = {p.perm_x, p.perm_y, p.perm_z};
    for (int t = 0; t < 3; t++) {
        int32_t *q = perms[t];
        for (int i = 0; i < 256; i++) q[i] = i;
        for (int i = 255; i > 0; i--) {
            int target = (int)(xorwow_uniform(st) * (float)(i + 1));
            if (target > i) target = i;
            int32_t tmp = q[i];
            q[i] = q[target];
            q[target] = tmp;
        }
    }
    sc->perlin.push_back(p);
    HostTexture t{};
    t.kind = TEX_NOISE;
    t.s = scale;
    t.a = (uint32_t)sc->perlin.size() - 1;
    return push_tex(sc, t);
}

// ---- materials ----
static rt_handle textured_material(rt_scene *s, uint32_t kind, rt_handle tex, const char *who)
{
    if (!valid_tex(S(s), tex)) {
        set_error(std::string(who) + ": invalid texture handle");
        return 0;
    }
    HostMaterial m{};
    m.kind = kind;
    m.texture = tex;
    return push_mat(S(s), m);
}
rt_handle rt_lambertian_tex(rt_scene *s, rt_handle texture) { return textured_material(s, MAT_LAMBERTIAN, texture, "rt_lambertian_tex"); }
rt_handle rt_lambertian(rt_scene *s, double r, double g, double b) { return s ? rt_lambertian_tex(s, rt_solid_color(s, r, g, b)) : 0; }
rt_handle rt_diffuse_light_tex(rt_scene *s, rt_handle texture) { return textured_material(s, MAT_DIFFUSE_LIGHT, texture, "rt_diffuse_light_tex"); }
rt_handle rt_diffuse_light(rt_scene *s, double r, double g, double b) { return s ? rt_diffuse_light_tex(s, rt_solid_color(s, r, g, b)) : 0; }
rt_handle rt_isotropic_tex(rt_scene *s, rt_handle texture) { return textured_material(s, MAT_ISOTROPIC, texture, "rt_isotropic_tex"); }
rt_handle rt_isotropic(rt_scene *s, double r, double g, double b) { return s ? rt_isotropic_tex(s, rt_solid_color(s, r, g, b)) : 0; }
rt_handle rt_metal(rt_scene *s, double r, double g, double b, double fuzz)
{
    if (!s) return 0;
    HostMaterial m{};
    m.kind = MAT_METAL;
    m.albedo = mk(r, g, b);
    m.p = fuzz < 1.0 ? fuzz : 1.0;  // Metal.h:14
    return push_mat(S(s), m);
}
rt_handle rt_dielectric(rt_scene *s, double refraction_index)
{
    if (!s) return 0;
    HostMaterial m{};
    m.kind = MAT_DIELECTRIC;
    m.p = refraction_index;
    return push_mat(S(s), m);
}

// ---- hittables ----
rt_handle rt_sphere(rt_scene *s, double cx, double cy, double cz, double radius, rt_handle material)
{
    if (!valid_mat(S(s), material)) {
        set_error("rt_sphere: invalid material handle");
        return 0;
    }
    HostHittable h{};
    h.kind = HKind::Sphere;
    h.c0 = mk(cx, cy, cz);
    h.radius = radius;
    h.material = material;
    D3 rv = mk(radius, radius, radius);
    h.box = box_from_corners(sub(h.c0, rv), add(h.c0, rv));  // Sphere.h:18-19
    return push_h(S(s), std::move(h));
}
rt_handle rt_moving_sphere(rt_scene *s, double c0x, double c0y, double c0z, double c1x, double c1y, double c1z,
                           double time0, double time1, double radius, rt_handle material)
{
    if (!valid_mat(S(s), material)) {
        set_error("rt_moving_sphere: invalid material handle");
        return 0;
    }
    HostHittable h{};
    h.kind = HKind::MovingSphere;
    h.c0 = mk(c0x, c0y, c0z);
    h.c1 = mk(c1x, c1y, c1z);
    h.t0 = time0;
    h.t1 = time1;
    h.radius = radius;
    h.material = material;
    D3 rv = mk(radius, radius, radius);
    Box b0 = box_from_corners(sub(h.c0, rv), add(h.c0, rv));
    Box b1 = box_from_corners(sub(h.c1, rv), add(h.c1, rv));
    h.box = box_merge(b0, b1);  // MovingSphere.h:32-35
    return push_h(S(s), std::move(h));
}
rt_handle rt_quad(rt_scene *s, const double q[3], const double u[3], const double v[3], rt_handle material)
{
    if (!valid_mat(S(s), material) || !q || !u || !v) {
        set_error("rt_quad: invalid material handle or null vector");
        return 0;
    }
    HostHittable h{};
    h.kind = HKind::Quad;
    h.q = mk(q[0], q[1], q[2]);
    h.u = mk(u[0], u[1], u[2]);
    h.v = mk(v[0], v[1], v[2]);
    h.material = material;
    D3 n = cross(h.u, h.v);  // Quad.h:33-37
    h.normal = normalize(n);
    h.plane_d = dot(h.normal, h.q);
    h.w = over(n, dot(n, n));
    Box d1 = box_from_corners(h.q, add(add(h.q, h.u), h.v));  // Quad.h:44-49
    Box d2 = box_from_corners(add(h.q, h.u), add(h.q, h.v));
    h.box = box_merge(d1, d2);
    return push_h(S(s), std::move(h));
}
// R/Quad.h's primitive with the interior rule its own comment (:86-88) names.  Everything but the box is the quad's.
rt_handle rt_triangle(rt_scene *s, const double q[3], const double u[3], const double v[3], rt_handle material)
{
    if (!valid_mat(S(s), material) || !q || !u || !v) {
        set_error("rt_triangle: invalid material handle or null vector");
        return 0;
    }
    HostHittable h{};
    h.kind = HKind::Triangle;
    h.q = mk(q[0], q[1], q[2]);
    h.u = mk(u[0], u[1], u[2]);
    h.v = mk(v[0], v[1], v[2]);
    h.material = material;
    D3 n = cross(h.u, h.v);  // Quad.h:33-37
    h.normal = normalize(n);
    h.plane_d = dot(h.normal, h.q);
    h.w = over(n, dot(n, n));
    // per axis the min and max of the three corners as computed, through the quad's corner-box helper (thin axes padded)
    const D3 b = add(h.q, h.u), c = add(h.q, h.v);
    h.box = box_from_corners(mk(std::fmin(h.q.x, std::fmin(b.x, c.x)), std::fmin(h.q.y, std::fmin(b.y, c.y)), std::fmin(h.q.z, std::fmin(b.z, c.z))),
                             mk(std::fmax(h.q.x, std::fmax(b.x, c.x)), std::fmax(h.q.y, std::fmax(b.y, c.y)), std::fmax(h.q.z, std::fmax(b.z, c.z))));
    return push_h(S(s), std::move(h));
}
rt_handle rt_triangle_mesh(rt_scene *s, const double *vertices, int n_vertices, const int32_t *indices, int n_triangles, rt_handle material,
                           rt_handle *triangles_out)
{
    if (!valid_mat(S(s), material) || !vertices || !indices || n_vertices < 3 || n_triangles < 1) {
        set_error("rt_triangle_mesh: invalid material handle, null array, fewer than 3 vertices or no triangle");
        return 0;
    }
    for (size_t k = 0; k < 3 * (size_t)n_triangles; k++)
        if (indices[k] < 0 || indices[k] >= n_vertices) {
            set_error("rt_triangle_mesh: index " + std::to_string(indices[k]) + " outside [0, " + std::to_string(n_vertices) + ")");
            return 0;
        }
    std::vector<rt_handle> tris((size_t)n_triangles);
    for (size_t k = 0; k < tris.size(); k++) {
        const double *a = vertices + 3 * (size_t)indices[3 * k], *b = vertices + 3 * (size_t)indices[3 * k + 1],
                     *c = vertices + 3 * (size_t)indices[3 * k + 2];
        const double u[3] = {b[0] - a[0], b[1] - a[1], b[2] - a[2]}, v[3] = {c[0] - a[0], c[1] - a[1], c[2] - a[2]};
        tris[k] = rt_triangle(s, a, u, v, material);
        if (!tris[k]) return 0;
    }
    if (triangles_out) std::memcpy(triangles_out, tris.data(), sizeof(rt_handle) * tris.size());  // input order: rt_bvh_node permutes its own copy
    return rt_bvh_node(s, tris.data(), n_triangles);
}

// Corner attributes (include/rtow.h rt_triangle_attr): what a triangle may be given, checked before anything is added.
static bool attr_acceptable(SceneImpl *sc, const double *normals, const double *texcoords, rt_handle material, const char *who)
{
    if (normals)
        for (int c = 0; c < 3; c++) {
            const double *n = normals + 3 * c;
            if (!std::isfinite(n[0]) || !std::isfinite(n[1]) || !std::isfinite(n[2]) || (n[0] == 0.0 && n[1] == 0.0 && n[2] == 0.0)) {
                set_error(std::string(who) + ": a corner normal is not finite or is all zero");
                return false;
            }
        }
    if (texcoords) {
        for (int c = 0; c < 6; c++)
            if (!std::isfinite(texcoords[c])) {
                set_error(std::string(who) + ": a texture coordinate is not finite");
                return false;
            }
        if (sc->materials[material - 1].kind == MAT_DIFFUSE_LIGHT) {
            set_error(std::string(who) + ": an emissive triangle takes no texture coordinates (the light table evaluates emission at the barycentric U, V)");
            return false;
        }
    }
    return true;
}
rt_handle rt_triangle_attr(rt_scene *s, const double q[3], const double u[3], const double v[3], const double *normals,
                           const double *texcoords, rt_handle material)
{
    if (!normals && !texcoords) return rt_triangle(s, q, u, v, material);
    if (!valid_mat(S(s), material) || !q || !u || !v) {
        set_error("rt_triangle_attr: invalid material handle or null vector");
        return 0;
    }
    if (!attr_acceptable(S(s), normals, texcoords, material, "rt_triangle_attr")) return 0;
    const rt_handle t = rt_triangle(s, q, u, v, material);
    if (!t) return 0;
    TriAttrRow row{};
    if (normals) std::memcpy(row.n, normals, sizeof row.n);
    if (texcoords) std::memcpy(row.t, texcoords, sizeof row.t);
    row.kinds = (normals ? ATTR_NORMALS : 0u) | (texcoords ? ATTR_TEXCOORDS : 0u);
    S(s)->tri_attr.push_back(row);
    S(s)->hittables[t - 1].attr = (uint32_t)S(s)->tri_attr.size();
    return t;
}
rt_handle rt_triangle_mesh_attr(rt_scene *s, const double *vertices, int n_vertices, const int32_t *indices, int n_triangles,
                                const double *normals, int n_normals, const int32_t *normal_indices, const double *texcoords,
                                int n_texcoords, const int32_t *texcoord_indices, rt_handle material, rt_handle *triangles_out)
{
    if (!normals && !texcoords) return rt_triangle_mesh(s, vertices, n_vertices, indices, n_triangles, material, triangles_out);
    if (!valid_mat(S(s), material) || !vertices || !indices || n_vertices < 3 || n_triangles < 1) {
        set_error("rt_triangle_mesh_attr: invalid material handle, null array, fewer than 3 vertices or no triangle");
        return 0;
    }
    if ((normals && n_normals < 1) || (texcoords && n_texcoords < 1)) {
        set_error("rt_triangle_mesh_attr: an attribute array without entries");
        return 0;
    }
    const int32_t *ni = normal_indices ? normal_indices : indices, *ti = texcoord_indices ? texcoord_indices : indices;
    const size_t corners = 3 * (size_t)n_triangles;
    auto in_range = [&](const int32_t *idx, int n, const char *what) {
        for (size_t k = 0; k < corners; k++)
            if (idx[k] < 0 || idx[k] >= n) {
                set_error(std::string("rt_triangle_mesh_attr: ") + what + " " + std::to_string(idx[k]) + " outside [0, " + std::to_string(n) + ")");
                return false;
            }
        return true;
    };
    if (!in_range(indices, n_vertices, "index") || (normals && !in_range(ni, n_normals, "normal index")) ||
        (texcoords && !in_range(ti, n_texcoords, "texture coordinate index")))
        return 0;
    std::vector<double> nrm(normals ? 3 * corners : 0), tex(texcoords ? 2 * corners : 0);  // per corner, gathered
    for (size_t k = 0; k < corners; k++) {
        if (normals) std::memcpy(&nrm[3 * k], normals + 3 * (size_t)ni[k], 3 * sizeof(double));
        if (texcoords) std::memcpy(&tex[2 * k], texcoords + 2 * (size_t)ti[k], 2 * sizeof(double));
    }
    for (size_t k = 0; k < (size_t)n_triangles; k++)  // every triangle's attributes before the first one is added
        if (!attr_acceptable(S(s), normals ? &nrm[9 * k] : nullptr, texcoords ? &tex[6 * k] : nullptr, material, "rt_triangle_mesh_attr")) return 0;
    std::vector<rt_handle> tris((size_t)n_triangles);
    for (size_t k = 0; k < tris.size(); k++) {
        const double *a = vertices + 3 * (size_t)indices[3 * k], *b = vertices + 3 * (size_t)indices[3 * k + 1],
                     *c = vertices + 3 * (size_t)indices[3 * k + 2];
        const double u[3] = {b[0] - a[0], b[1] - a[1], b[2] - a[2]}, v[3] = {c[0] - a[0], c[1] - a[1], c[2] - a[2]};
        tris[k] = rt_triangle_attr(s, a, u, v, normals ? &nrm[9 * k] : nullptr, texcoords ? &tex[6 * k] : nullptr, material);
        if (!tris[k]) return 0;
    }
    if (triangles_out) std::memcpy(triangles_out, tris.data(), sizeof(rt_handle) * tris.size());
    return rt_bvh_node(s, tris.data(), n_triangles);
}

// Wavefront OBJ: positions and faces, and for rt_obj_load_attr (`attr`) the vn / vt statements and the j, k of a face corner.
// fs, fn, ft: three corner indices a triangle, 0-based; a positive one may name an entry that follows (checked at the end).
// fn / ft come back empty unless every corner of every face named a normal / a texture coordinate.
namespace {
struct ObjText {
    std::vector<double> vs, vn, vt;
    std::vector<long long> fs, fn, ft;
};
int obj_parse(const char *who, const char *path, bool attr, ObjText &o)
{
    FILE *fp = std::fopen(path, "rb");
    if (!fp) return fail(RT_ERR_INVALID, std::string(who) + ": cannot open " + path);
    std::string text;
    char buf[1 << 16];
    for (size_t got; (got = std::fread(buf, 1, sizeof buf, fp)) > 0;) text.append(buf, got);
    const bool read_error = std::ferror(fp) != 0;
    std::fclose(fp);
    if (read_error) return fail(RT_ERR_INVALID, std::string(who) + ": cannot read " + path);

    std::vector<double> &vs = o.vs;
    std::vector<long long> &fs = o.fs;
    bool all_n = attr, all_t = attr;  // so far every corner named a normal / a texture coordinate
    size_t line_no = 0;
    auto bad = [&](const char *what) { return fail(RT_ERR_INVALID, std::string(who) + ": " + path + ":" + std::to_string(line_no) + ": " + what); };
    for (size_t pos = 0; pos < text.size();) {
        size_t eol = text.find('\n', pos);
        if (eol == std::string::npos) eol = text.size();
        std::string line = text.substr(pos, eol - pos);
        pos = eol + 1;
        line_no++;
        const size_t hash = line.find('#');
        if (hash != std::string::npos) line.resize(hash);
        const char *c = line.c_str();
        while (*c == ' ' || *c == '\t') c++;
        const bool is_v = c[0] == 'v' && (c[1] == ' ' || c[1] == '\t'), is_f = c[0] == 'f' && (c[1] == ' ' || c[1] == '\t');
        const bool is_vn = attr && c[0] == 'v' && c[1] == 'n' && (c[2] == ' ' || c[2] == '\t');
        const bool is_vt = attr && c[0] == 'v' && c[1] == 't' && (c[2] == ' ' || c[2] == '\t');
        if (!is_v && !is_f && !is_vn && !is_vt) continue;  // g, o, s, usemtl, mtllib, ... (and vn, vt for rt_obj_load): skipped
        c += is_v || is_f ? 2 : 3;
        if (!is_f) {
            const char *line_end = line.c_str() + line.size();
            std::vector<double> &into = is_v ? vs : (is_vn ? o.vn : o.vt);
            for (int k = 0; k < (is_vt ? 2 : 3); k++) {  // std::from_chars: the "C" number format whatever locale the host program has set
                while (*c == ' ' || *c == '\t') c++;
                if (*c == '+') c++;
                double x = 0.0;
                const auto parsed = std::from_chars(c, line_end, x);
                if (parsed.ec != std::errc() || parsed.ptr == c)
                    return bad(is_v ? "a vertex needs three numbers" : (is_vn ? "a vn needs three numbers" : "a vt needs two numbers"));
                into.push_back(x);
                c = parsed.ptr;
            }
            continue;  // (a vt's third number, a vertex's w or colour: not read)
        }
        std::vector<long long> corner, corner_n, corner_t;
        for (;;) {
            while (*c == ' ' || *c == '\t' || *c == '\r') c++;
            if (!*c) break;
            char *end = nullptr;
            const long long i = std::strtoll(c, &end, 10);
            if (end == c || i == 0) return bad("a face corner needs a non-zero vertex index");
            const long long n_so_far = (long long)(vs.size() / 3);
            if (i < -n_so_far) return bad("relative vertex index out of range");
            corner.push_back(i > 0 ? i - 1 : n_so_far + i);
            c = end;
            if (attr) {  // "/j", "/j/k", "//k": each relative to the count of its own kind so far
                bool has_t = false, has_n = false;
                if (*c == '/') {
                    c++;
                    if (*c != '/' && *c && *c != ' ' && *c != '\t' && *c != '\r') {
                        const long long j = std::strtoll(c, &end, 10);
                        const long long nt = (long long)(o.vt.size() / 2);
                        if (end == c || j == 0) return bad("a face corner's texture coordinate index must be a non-zero number");
                        if (j < -nt) return bad("relative texture coordinate index out of range");
                        corner_t.push_back(j > 0 ? j - 1 : nt + j);
                        has_t = true;
                        c = end;
                    }
                    if (*c == '/') {
                        c++;
                        if (*c && *c != ' ' && *c != '\t' && *c != '\r') {
                            const long long k = std::strtoll(c, &end, 10);
                            const long long nn = (long long)(o.vn.size() / 3);
                            if (end == c || k == 0) return bad("a face corner's normal index must be a non-zero number");
                            if (k < -nn) return bad("relative normal index out of range");
                            corner_n.push_back(k > 0 ? k - 1 : nn + k);
                            has_n = true;
                            c = end;
                        }
                    }
                }
                all_t = all_t && has_t;
                all_n = all_n && has_n;
            }
            while (*c && *c != ' ' && *c != '\t' && *c != '\r') c++;  // rt_obj_load: "/j", "/j/k", "//k" are not read
        }
        if (corner.size() < 3) return bad("a face needs three corners");
        for (size_t k = 1; k + 1 < corner.size(); k++) {  // a polygon is fanned from its first corner
            fs.push_back(corner[0]);
            fs.push_back(corner[k]);
            fs.push_back(corner[k + 1]);
            if (all_n) o.fn.insert(o.fn.end(), {corner_n[0], corner_n[k], corner_n[k + 1]});
            if (all_t) o.ft.insert(o.ft.end(), {corner_t[0], corner_t[k], corner_t[k + 1]});
        }
    }
    if (fs.empty()) return fail(RT_ERR_INVALID, std::string(who) + ": " + path + " has no face");
    const long long nv = (long long)(vs.size() / 3);
    for (long long i : fs)
        if (i < 0 || i >= nv) return fail(RT_ERR_INVALID, std::string(who) + ": " + path + ": vertex index out of range");
    if (!all_n) o.fn.clear();
    if (!all_t) o.ft.clear();
    for (long long i : o.fn)
        if (i < 0 || i >= (long long)(o.vn.size() / 3)) return fail(RT_ERR_INVALID, std::string(who) + ": " + path + ": normal index out of range");
    for (long long i : o.ft)
        if (i < 0 || i >= (long long)(o.vt.size() / 2)) return fail(RT_ERR_INVALID, std::string(who) + ": " + path + ": texture coordinate index out of range");
    if (fs.size() / 3 > (size_t)INT32_MAX || nv > (long long)INT32_MAX || o.vn.size() / 3 > (size_t)INT32_MAX || o.vt.size() / 2 > (size_t)INT32_MAX)
        return fail(RT_ERR_INVALID, std::string(who) + ": mesh too large");
    return RT_OK;
}
// malloc'ed copies for the caller (rt_mesh_free, rt_obj_mesh_free); false: out of memory
bool obj_copy_numbers(const std::vector<double> &from, double *&to)
{
    to = (double *)std::malloc(std::max<size_t>(from.size(), 1) * sizeof(double));
    if (to) std::memcpy(to, from.data(), from.size() * sizeof(double));
    return to != nullptr;
}
bool obj_copy_indices(const std::vector<long long> &from, int32_t *&to)
{
    to = (int32_t *)std::malloc(std::max<size_t>(from.size(), 1) * sizeof(int32_t));
    for (size_t k = 0; to && k < from.size(); k++) to[k] = (int32_t)from[k];
    return to != nullptr;
}
}  // namespace

int rt_obj_load(const char *path, double **vertices, int *n_vertices, int32_t **indices, int *n_triangles)
{
    if (!path || !vertices || !n_vertices || !indices || !n_triangles) return fail(RT_ERR_INVALID, "rt_obj_load: null argument");
    *vertices = nullptr;
    *indices = nullptr;
    *n_vertices = *n_triangles = 0;
    ObjText o;
    if (int rc = obj_parse("rt_obj_load", path, false, o)) return rc;
    double *vout = nullptr;
    int32_t *iout = nullptr;
    if (!obj_copy_numbers(o.vs, vout) || !obj_copy_indices(o.fs, iout)) {
        std::free(vout);
        std::free(iout);
        return fail(RT_ERR_INVALID, "rt_obj_load: out of memory");
    }
    *vertices = vout;
    *indices = iout;
    *n_vertices = (int)(o.vs.size() / 3);
    *n_triangles = (int)(o.fs.size() / 3);
    return RT_OK;
}
int rt_obj_load_attr(const char *path, rt_obj_mesh *out)
{
    if (!path || !out) return fail(RT_ERR_INVALID, "rt_obj_load_attr: null argument");
    std::memset(out, 0, sizeof *out);
    ObjText o;
    if (int rc = obj_parse("rt_obj_load_attr", path, true, o)) return rc;
    bool ok = obj_copy_numbers(o.vs, out->vertices) && obj_copy_indices(o.fs, out->indices);
    if (ok && !o.fn.empty()) ok = obj_copy_numbers(o.vn, out->normals) && obj_copy_indices(o.fn, out->normal_indices);
    if (ok && !o.ft.empty()) ok = obj_copy_numbers(o.vt, out->texcoords) && obj_copy_indices(o.ft, out->texcoord_indices);
    if (!ok) {
        rt_obj_mesh_free(out);
        return fail(RT_ERR_INVALID, "rt_obj_load_attr: out of memory");
    }
    out->n_vertices = (int)(o.vs.size() / 3);
    out->n_triangles = (int)(o.fs.size() / 3);
    out->n_normals = o.fn.empty() ? 0 : (int)(o.vn.size() / 3);
    out->n_texcoords = o.ft.empty() ? 0 : (int)(o.vt.size() / 2);
    return RT_OK;
}
void rt_obj_mesh_free(rt_obj_mesh *m)
{
    if (!m) return;
    std::free(m->vertices);
    std::free(m->normals);
    std::free(m->texcoords);
    std::free(m->indices);
    std::free(m->normal_indices);
    std::free(m->texcoord_indices);
    std::memset(m, 0, sizeof *m);
}
void rt_mesh_free(double *vertices, int32_t *indices)
{
    std::free(vertices);
    std::free(indices);
}
rt_handle rt_translate(rt_scene *s, rt_handle object, double ox, double oy, double oz)
{
    HostHittable *c = get_h(S(s), object);
    if (!c) {
        set_error("rt_translate: invalid object handle");
        return 0;
    }
    HostHittable h{};
    h.kind = HKind::Translate;
    h.child = object;
    h.offset = mk(ox, oy, oz);
    h.box = box_moved(c->box, h.offset);  // Instance.h:36
    return push_h(S(s), std::move(h));
}
rt_handle rt_rotate_y(rt_scene *s, rt_handle object, double angle_degrees)
{
    HostHittable *c = get_h(S(s), object);
    if (!c) {
        set_error("rt_rotate_y: invalid object handle");
        return 0;
    }
    HostHittable h{};
    h.kind = HKind::RotateY;
    h.child = object;
    double radians = angle_degrees * 3.1415926535897932385 / 180.0;  // Instance.h:78-80
    h.sin_t = std::sin(radians);
    h.cos_t = std::cos(radians);
    const Box cb = c->box;
    double mn[3] = {DBL_MAX, DBL_MAX, DBL_MAX}, mx[3] = {-DBL_MAX, -DBL_MAX, -DBL_MAX};
    for (int i = 0; i < 2; i++)  // Instance.h:87-109: rotate the 8 corners
        for (int j = 0; j < 2; j++)
            for (int k = 0; k < 2; k++) {
                double x = i * cb.hi[0] + (1 - i) * cb.lo[0];
                double y = j * cb.hi[1] + (1 - j) * cb.lo[1];
                double z = k * cb.hi[2] + (1 - k) * cb.lo[2];
                double nx = h.cos_t * x + h.sin_t * z;
                double nz = -h.sin_t * x + h.cos_t * z;
                double t[3] = {nx, y, nz};
                for (int c2 = 0; c2 < 3; c2++) {
                    mn[c2] = std::fmin(mn[c2], t[c2]);
                    mx[c2] = std::fmax(mx[c2], t[c2]);
                }
            }
    h.box = box_from_corners(mk(mn[0], mn[1], mn[2]), mk(mx[0], mx[1], mx[2]));
    return push_h(S(s), std::move(h));
}
// An emissive primitive below `handle`, found as the light collector finds lights: never through a ConstantMedium.  spheres_only: a
// Sphere or MovingSphere (what rt_transform cannot hold); otherwise a quad or triangle too (what rt_moving_transform cannot hold).
static bool holds_lamp(const SceneImpl &s, uint32_t handle, bool spheres_only, int depth)
{
    if (depth > 64) return false;  // (deeper than the light collector goes: the commit refuses such a graph)
    const HostHittable &h = s.hittables[handle - 1];
    switch (h.kind) {
    case HKind::Medium: return false;
    case HKind::Translate:
    case HKind::RotateY:
    case HKind::Transform:
    case HKind::MovingTransform: return holds_lamp(s, h.child, spheres_only, depth + 1);
    case HKind::List:
    case HKind::Bvh:
        for (uint32_t c : h.items)
            if (holds_lamp(s, c, spheres_only, depth + 1)) return true;
        return false;
    case HKind::Quad:
    case HKind::Triangle: return !spheres_only && s.materials[h.material - 1].kind == MAT_DIFFUSE_LIGHT;
    case HKind::Sphere:
    case HKind::MovingSphere: return s.materials[h.material - 1].kind == MAT_DIFFUSE_LIGHT;
    default: return false;
    }
}
// The nine cofactors and the determinant of a row-major 3x3, in the order include/rtow.h rt_transform states (this file: contraction off).
static double cofactors(const double *L, double cf[9])
{
    const double c[9] = {(L[4] * L[8]) - (L[5] * L[7]), (L[5] * L[6]) - (L[3] * L[8]), (L[3] * L[7]) - (L[4] * L[6]),
                         (L[2] * L[7]) - (L[1] * L[8]), (L[0] * L[8]) - (L[2] * L[6]), (L[1] * L[6]) - (L[0] * L[7]),
                         (L[1] * L[5]) - (L[2] * L[4]), (L[2] * L[3]) - (L[0] * L[5]), (L[0] * L[4]) - (L[1] * L[3])};
    std::memcpy(cf, c, sizeof c);
    return ((L[0] * c[0]) + (L[1] * c[1])) + (L[2] * c[2]);
}
// L, t and Li of the row-major 3x4 m as rt_transform stores them; why such a matrix is refused, or nullptr.
static const char *affine_from_matrix(const double m[12], HostAffine &a)
{
    for (int r = 0; r < 3; r++) {
        for (int k = 0; k < 3; k++) a.L[3 * r + k] = m[4 * r + k];
        a.t[r] = m[4 * r + 3];
    }
    for (int k = 0; k < 12; k++)
        if (!std::isfinite(m[k])) return "a matrix entry is not finite";
    double cf[9];
    const double det = cofactors(a.L, cf);
    if (!std::isfinite(det) || det == 0.0) return "the determinant is zero or not finite";
    for (int r = 0; r < 3; r++)
        for (int k = 0; k < 3; k++) {
            a.Li[3 * r + k] = cf[3 * k + r] / det;
            if (!std::isfinite(a.Li[3 * r + k])) return "an entry of the inverse is not finite";
        }
    return nullptr;
}
// fmin / fmax per axis over the eight corners of `cb` taken forward by (L p) + t, as rt_rotate_y takes them: x outermost, lo before hi
static void corners_forward(const Box &cb, const HostAffine &a, double mn[3], double mx[3])
{
    for (int i = 0; i < 2; i++)
        for (int j = 0; j < 2; j++)
            for (int k = 0; k < 2; k++) {
                const D3 p = affine_point(a, mk(i ? cb.hi[0] : cb.lo[0], j ? cb.hi[1] : cb.lo[1], k ? cb.hi[2] : cb.lo[2]));
                for (int c2 = 0; c2 < 3; c2++) {
                    mn[c2] = std::fmin(mn[c2], comp(p, c2));
                    mx[c2] = std::fmax(mx[c2], comp(p, c2));
                }
            }
}
rt_handle rt_transform(rt_scene *s, rt_handle object, const double m[12])
{
    HostHittable *c = get_h(S(s), object);
    if (!c || !m) {
        set_error("rt_transform: invalid object handle or null matrix");
        return 0;
    }
    HostAffine a{};
    if (const char *why = affine_from_matrix(m, a)) {
        set_error(std::string("rt_transform: ") + why);
        return 0;
    }
    if (holds_lamp(*S(s), object, true, 0)) {
        set_error("rt_transform: the child holds an emissive Sphere or MovingSphere (an ellipsoid lamp; the light table cannot hold it)");
        return 0;
    }
    HostHittable h{};
    h.kind = HKind::Transform;
    h.child = object;
    double mn[3] = {DBL_MAX, DBL_MAX, DBL_MAX}, mx[3] = {-DBL_MAX, -DBL_MAX, -DBL_MAX};
    corners_forward(c->box, a, mn, mx);
    h.box = box_from_corners(mk(mn[0], mn[1], mn[2]), mk(mx[0], mx[1], mx[2]));
    S(s)->transforms.push_back(a);
    h.xf = (uint32_t)S(s)->transforms.size();
    return push_h(S(s), std::move(h));
}
// Is det(L(s)), L(s) = L0 + s dL, of one strict sign over [0, 1]?  It is a cubic in s; with rows a_i of L0 and b_i of L0 + dL its Bernstein
// coefficients are det(a0,a1,a2), a third of the three determinants with one b row, a third of the three with two, det(b0,b1,b2), and
// a polynomial lies in the hull of its coefficients.  Where the four do not agree the interval is halved (de Casteljau), to depth 8.
// A coefficient has a sign only beyond `margin`, 2^-30 of the largest of the first four: the halving rounds, and a double root (a half
// turn about an axis: det = (1 - 2s)^2) would otherwise be passed by a midpoint that comes out as a few 1e-17 instead of zero.
static bool det_keeps_sign(const double c[4], double margin, int depth)
{
    if ((c[0] > margin && c[1] > margin && c[2] > margin && c[3] > margin) || (c[0] < -margin && c[1] < -margin && c[2] < -margin && c[3] < -margin))
        return true;
    const bool ends_agree = (c[0] > margin && c[3] > margin) || (c[0] < -margin && c[3] < -margin);
    if (depth >= 8 || !ends_agree) return false;  // the ends are values of det: a zero or a change of sign there is final
    const double p01 = 0.5 * (c[0] + c[1]), p12 = 0.5 * (c[1] + c[2]), p23 = 0.5 * (c[2] + c[3]);
    const double p012 = 0.5 * (p01 + p12), p123 = 0.5 * (p12 + p23), mid = 0.5 * (p012 + p123);
    const double left[4] = {c[0], p01, p012, mid}, right[4] = {mid, p123, p23, c[3]};
    return det_keeps_sign(left, margin, depth + 1) && det_keeps_sign(right, margin, depth + 1);
}
rt_handle rt_moving_transform(rt_scene *s, rt_handle object, const double m0[12], const double m1[12], double time0, double time1)
{
    HostHittable *c = get_h(S(s), object);
    if (!c || !m0 || !m1) {
        set_error("rt_moving_transform: invalid object handle or null matrix");
        return 0;
    }
    HostAffine key0{}, key1{};
    const char *why = affine_from_matrix(m0, key0);
    if (!why) why = affine_from_matrix(m1, key1);
    if (why) {
        set_error(std::string("rt_moving_transform: ") + why);
        return 0;
    }
    if (!std::isfinite(time0) || !std::isfinite(time1) || !(time1 > time0)) {
        set_error("rt_moving_transform: time0 and time1 must be finite with time0 < time1");
        return 0;
    }
    HostMovingAffine a{};
    HostAffine end{};  // the matrices of s = 1 as the device forms them: L0 + (1.0 * dL), t0 + (1.0 * dt)
    for (int k = 0; k < 9; k++) {
        a.L0[k] = key0.L[k];
        a.dL[k] = key1.L[k] - key0.L[k];
        end.L[k] = a.L0[k] + (1.0 * a.dL[k]);
    }
    for (int k = 0; k < 3; k++) {
        a.t0[k] = key0.t[k];
        a.dt[k] = key1.t[k] - key0.t[k];
        end.t[k] = a.t0[k] + (1.0 * a.dt[k]);
    }
    a.time0 = time0;
    a.dtime = time1 - time0;
    bool finite = std::isfinite(a.dtime);
    for (int k = 0; k < 9; k++) finite &= std::isfinite(a.dL[k]) && std::isfinite(end.L[k]);
    for (int k = 0; k < 3; k++) finite &= std::isfinite(a.dt[k]) && std::isfinite(end.t[k]);
    if (!finite) {
        set_error("rt_moving_transform: the difference of the keys is not finite");
        return 0;
    }
    auto det3 = [](const double *r0, const double *r1, const double *r2) {
        const double L[9] = {r0[0], r0[1], r0[2], r1[0], r1[1], r1[2], r2[0], r2[1], r2[2]};
        double cf[9];
        return cofactors(L, cf);
    };
    const double *a0 = a.L0, *a1 = a.L0 + 3, *a2 = a.L0 + 6, *b0 = end.L, *b1 = end.L + 3, *b2 = end.L + 6;
    const double bern[4] = {det3(a0, a1, a2), ((det3(b0, a1, a2) + det3(a0, b1, a2)) + det3(a0, a1, b2)) / 3.0,
                            ((det3(b0, b1, a2) + det3(b0, a1, b2)) + det3(a0, b1, b2)) / 3.0, det3(b0, b1, b2)};
    double largest = 0.0;
    for (double b : bern) largest = std::fmax(largest, std::fabs(b));
    if (!std::isfinite(largest) || !det_keeps_sign(bern, 0x1p-30 * largest, 0)) {
        set_error("rt_moving_transform: the interpolated matrix L0 + s (L1 - L0) is singular, or cannot be shown regular, for some s in "
                  "[0, 1]; split the motion into smaller steps");
        return 0;
    }
    if (holds_lamp(*S(s), object, false, 0)) {
        set_error("rt_moving_transform: the child holds an emissive primitive (the light table is static; a moving lamp is out of scope)");
        return 0;
    }
    HostHittable h{};
    h.kind = HKind::MovingTransform;
    h.child = object;
    double mn[3] = {DBL_MAX, DBL_MAX, DBL_MAX}, mx[3] = {-DBL_MAX, -DBL_MAX, -DBL_MAX};
    corners_forward(c->box, key0, mn, mx);
    corners_forward(c->box, end, mn, mx);
    // a point at an intermediate s is a convex combination of its two key positions only up to the roundings of (L p) + t
    double reach = 0.0;
    for (int k = 0; k < 3; k++) reach = std::fmax(reach, std::fmax(std::fabs(mn[k]), std::fabs(mx[k])));
    const double widen = 16.0 * DBL_EPSILON * reach;
    for (int k = 0; k < 3; k++) {
        mn[k] -= widen;
        mx[k] += widen;
    }
    h.box = box_from_corners(mk(mn[0], mn[1], mn[2]), mk(mx[0], mx[1], mx[2]));
    S(s)->moving_transforms.push_back(a);
    h.xf = (uint32_t)S(s)->moving_transforms.size();
    return push_h(S(s), std::move(h));
}
rt_handle rt_moving_translate(rt_scene *s, rt_handle object, const double offset0[3], const double offset1[3], double time0, double time1)
{
    if (!offset0 || !offset1) {
        set_error("rt_moving_translate: null offset");
        return 0;
    }
    const double m0[12] = {1.0, 0.0, 0.0, offset0[0], 0.0, 1.0, 0.0, offset0[1], 0.0, 0.0, 1.0, offset0[2]};
    const double m1[12] = {1.0, 0.0, 0.0, offset1[0], 0.0, 1.0, 0.0, offset1[1], 0.0, 0.0, 1.0, offset1[2]};
    return rt_moving_transform(s, object, m0, m1, time0, time1);
}
int rt_moving_transform_get(rt_scene *s, rt_handle h, double out26[26])
{
    HostHittable *x = get_h(S(s), h);
    if (!x || !out26 || x->kind != HKind::MovingTransform)
        return fail(RT_ERR_INVALID, "rt_moving_transform_get: not a MovingTransform handle, or null output");
    const HostMovingAffine &a = S(s)->moving_transforms[x->xf - 1];
    std::memcpy(out26, a.L0, 9 * sizeof(double));
    std::memcpy(out26 + 9, a.t0, 3 * sizeof(double));
    std::memcpy(out26 + 12, a.dL, 9 * sizeof(double));
    std::memcpy(out26 + 21, a.dt, 3 * sizeof(double));
    out26[24] = a.time0;
    out26[25] = a.dtime;
    return RT_OK;
}
rt_handle rt_rotate_x(rt_scene *s, rt_handle object, double angle_degrees)
{
    const double radians = angle_degrees * 3.1415926535897932385 / 180.0;  // as rt_rotate_y
    const double sn = std::sin(radians), cs = std::cos(radians);
    const double m[12] = {1.0, 0.0, 0.0, 0.0, 0.0, cs, -sn, 0.0, 0.0, sn, cs, 0.0};
    return rt_transform(s, object, m);
}
rt_handle rt_rotate_z(rt_scene *s, rt_handle object, double angle_degrees)
{
    const double radians = angle_degrees * 3.1415926535897932385 / 180.0;
    const double sn = std::sin(radians), cs = std::cos(radians);
    const double m[12] = {cs, -sn, 0.0, 0.0, sn, cs, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0};
    return rt_transform(s, object, m);
}
rt_handle rt_scale(rt_scene *s, rt_handle object, double sx, double sy, double sz)
{
    const double m[12] = {sx, 0.0, 0.0, 0.0, 0.0, sy, 0.0, 0.0, 0.0, 0.0, sz, 0.0};
    return rt_transform(s, object, m);
}
int rt_transform_get(rt_scene *s, rt_handle transform, double out21[21])
{
    HostHittable *h = get_h(S(s), transform);
    if (!h || !out21 || h->kind != HKind::Transform) return fail(RT_ERR_INVALID, "rt_transform_get: not a Transform handle, or null output");
    const HostAffine &a = S(s)->transforms[h->xf - 1];
    std::memcpy(out21, a.L, 9 * sizeof(double));
    std::memcpy(out21 + 9, a.t, 3 * sizeof(double));
    std::memcpy(out21 + 12, a.Li, 9 * sizeof(double));
    return RT_OK;
}
rt_handle rt_hittable_list(rt_scene *s, const rt_handle *objects, int count)
{
    if (!s || count < 0 || (count > 0 && !objects)) {
        set_error("rt_hittable_list: bad arguments");
        return 0;
    }
    HostHittable h{};
    h.kind = HKind::List;
    h.box = empty_box();
    for (int i = 0; i < count; i++) {
        HostHittable *c = get_h(S(s), objects[i]);
        if (!c) {
            set_error("rt_hittable_list: invalid child handle");
            return 0;
        }
        h.box = box_merge(h.box, c->box);  // HittableList.h:25-26
        h.items.push_back(objects[i]);
    }
    return push_h(S(s), std::move(h));
}
rt_handle rt_make_box(rt_scene *s, const double a[3], const double b[3], rt_handle material)
{
    if (!valid_mat(S(s), material) || !a || !b) {
        set_error("rt_make_box: invalid material handle or null corner");
        return 0;
    }
    // Instance.h:166-184: six quads, in the reference's order and with its (negated) edge vectors.
    double mn[3], mx[3];
    for (int k = 0; k < 3; k++) {
        mn[k] = std::fmin(a[k], b[k]);
        mx[k] = std::fmax(a[k], b[k]);
    }
    D3 dx = mk(mx[0] - mn[0], 0, 0), dy = mk(0, mx[1] - mn[1], 0), dz = mk(0, 0, mx[2] - mn[2]);
    D3 ndx = neg(dx), ndz = neg(dz);
    struct Side { double q[3]; D3 u, v; } sides[6] = {
        {{mn[0], mn[1], mx[2]}, dx, dy},    // front
        {{mx[0], mn[1], mx[2]}, ndz, dy},   // right
        {{mx[0], mn[1], mn[2]}, ndx, dy},   // back
        {{mn[0], mn[1], mn[2]}, dz, dy},    // left
        {{mn[0], mx[1], mx[2]}, dx, ndz},   // top
        {{mn[0], mn[1], mn[2]}, dx, dz},    // bottom
    };
    rt_handle quads[6];
    for (int k = 0; k < 6; k++) {
        double u[3] = {sides[k].u.x, sides[k].u.y, sides[k].u.z}, v[3] = {sides[k].v.x, sides[k].v.y, sides[k].v.z};
        quads[k] = rt_quad(s, sides[k].q, u, v, material);
        if (!quads[k]) return 0;
    }
    return rt_hittable_list(s, quads, 6);
}
static rt_handle medium_common(rt_scene *s, rt_handle boundary, double density, rt_handle phase)
{
    HostHittable *c = get_h(S(s), boundary);
    if (!c || !phase) {
        set_error("rt_constant_medium: invalid boundary or texture handle");
        return 0;
    }
    HostHittable h{};
    h.kind = HKind::Medium;
    h.child = boundary;
    h.neg_inv_density = -1.0 / density;  // ConstantMedium.h:41
    h.material = phase;
    h.box = c->box;  // ConstantMedium.h:96
    return push_h(S(s), std::move(h));
}
rt_handle rt_constant_medium(rt_scene *s, rt_handle boundary, double density, double r, double g, double b)
{
    if (!s) return 0;
    return medium_common(s, boundary, density, rt_isotropic(s, r, g, b));
}
rt_handle rt_constant_medium_tex(rt_scene *s, rt_handle boundary, double density, rt_handle texture)
{
    if (!s) return 0;
    return medium_common(s, boundary, density, rt_isotropic_tex(s, texture));
}
rt_handle rt_bvh_node(rt_scene *s, rt_handle *objects, int count)
{
    if (!s || !objects || count <= 0) {
        set_error("rt_bvh_node: needs at least one object (the reference's constructor does not terminate on an empty span)");
        return 0;
    }
    SceneImpl *sc = S(s);
    for (int i = 0; i < count; i++)
        if (!get_h(sc, objects[i])) {
            set_error("rt_bvh_node: invalid object handle");
            return 0;
        }
    HostHittable h{};
    h.kind = HKind::Bvh;
    std::vector<uint32_t> objs(objects, objects + count);
    build_tree(sc, h, objs, 0, count);
    h.box = h.tree[0].box;
    h.items = objs;
    std::memcpy(objects, objs.data(), sizeof(rt_handle) * (size_t)count);  // the reference sorts list[] in place
    return push_h(sc, std::move(h));
}
int rt_hittable_bounding_box(rt_scene *s, rt_handle object, double out[6])
{
    HostHittable *h = get_h(S(s), object);
    if (!h || !out) return fail(RT_ERR_INVALID, "rt_hittable_bounding_box: invalid handle");
    for (int k = 0; k < 3; k++) {
        out[2 * k] = h->box.lo[k];
        out[2 * k + 1] = h->box.hi[k];
    }
    return RT_OK;
}

int rt_scene_set_world(rt_scene *s, rt_handle world)
{
    if (!get_h(S(s), world)) return fail(RT_ERR_INVALID, "rt_scene_set_world: invalid handle");
    S(s)->world = world;
    S(s)->committed = false;
    return RT_OK;
}

int rt_scene_set_camera(rt_scene *s, const double lookfrom[3], const double lookat[3], const double vup[3],
                        double vfov_degrees, double aspect, double aperture, double focus_dist, double time0,
                        double time1, const double background[3])
{
    if (!s || !lookfrom || !lookat || !vup || !background) return fail(RT_ERR_INVALID, "rt_scene_set_camera: null argument");
    if (S(s)->launches_in_flight > 0)
        return fail(RT_ERR_STATE, "rt_scene_set_camera: a render of this scene is in flight (rt_render_finish it first)");
    // Camera.h:47-72
    CameraRec c{};
    D3 from = mk(lookfrom[0], lookfrom[1], lookfrom[2]), at = mk(lookat[0], lookat[1], lookat[2]);
    D3 up = mk(vup[0], vup[1], vup[2]);
    double theta = vfov_degrees * 3.14159265358979323846 / 180.0;
    double half_h = std::tan(theta / 2.0);
    double half_w = aspect * half_h;
    D3 w = normalize(sub(from, at));
    D3 u = normalize(cross(up, w));
    D3 v = cross(w, u);
    D3 llc = sub(sub(sub(from, scale(half_w * focus_dist, u)), scale(half_h * focus_dist, v)), scale(focus_dist, w));
    D3 horiz = scale(2.0 * half_w * focus_dist, u);
    D3 vert = scale(2.0 * half_h * focus_dist, v);
    auto put = [](double *dst, D3 a) { dst[0] = a.x; dst[1] = a.y; dst[2] = a.z; };
    put(c.bg, mk(background[0], background[1], background[2]));
    put(c.origin, from);
    put(c.llc, llc);
    put(c.horizontal, horiz);
    put(c.vertical, vert);
    put(c.u, u);
    put(c.v, v);
    put(c.w, w);
    c.lens_radius = aperture / 2.0;
    c.time0 = time0;
    c.time1 = time1;
    S(s)->camera = c;
    S(s)->has_camera = true;
    S(s)->generation++;  // the uploaded CameraRec is stale; the flat tables do not depend on the camera
    return RT_OK;
}

static_assert(RT_SCENE_FLAG_ENVIRONMENT == SCENE_ENVIRONMENT, "the bit the header names");
uint32_t rt_scene_flags(rt_scene *s) { return s && S(s)->committed ? S(s)->flat.flags : 0u; }

int rt_scene_set_environment(rt_scene *s, const rt_environment *env)
{
    if (!s) return fail(RT_ERR_INVALID, "rt_scene_set_environment: null scene");
    SceneImpl &sc = *S(s);
    if (sc.launches_in_flight > 0)
        return fail(RT_ERR_STATE, "rt_scene_set_environment: a render of this scene is in flight (rt_render_finish it first)");
    if (!env) {
        sc.has_environment = false;
        sc.environment = HostEnvironment{};
        sc.committed = false;
        return RT_OK;
    }
    if ((env->texture != 0) == (env->rgb != nullptr)) return fail(RT_ERR_INVALID, "rt_scene_set_environment: give a texture or a float image, not both, not neither");
    if (env->texture && !valid_tex(&sc, env->texture)) return fail(RT_ERR_INVALID, "rt_scene_set_environment: invalid texture handle");
    for (int c = 0; c < 3; c++)
        if (!(std::isfinite(env->intensity[c]) && env->intensity[c] >= 0.0))
            return fail(RT_ERR_INVALID, "rt_scene_set_environment: intensity must be finite and not negative");
    for (int k = 0; k < 9; k++)
        if (!std::isfinite(env->rotation[k])) return fail(RT_ERR_INVALID, "rt_scene_set_environment: rotation is not finite");
    for (int a = 0; a < 3; a++)
        for (int b = 0; b < 3; b++) {
            const double *ra = env->rotation + 3 * a, *rb = env->rotation + 3 * b;
            const double d = (ra[0] * rb[0] + ra[1] * rb[1]) + ra[2] * rb[2];
            if (!(std::fabs(d - (a == b ? 1.0 : 0.0)) <= 1e-9)) return fail(RT_ERR_INVALID, "rt_scene_set_environment: rotation is not orthonormal to 1e-9");
        }
    HostEnvironment h;
    h.texture = env->texture;
    if (env->rgb) {
        if (env->width < 1 || env->height < 1) return fail(RT_ERR_INVALID, "rt_scene_set_environment: width and height must be at least 1");
        const size_t n = (size_t)env->width * (size_t)env->height * 3;
        for (size_t k = 0; k < n; k++)
            if (!(std::isfinite(env->rgb[k]) && env->rgb[k] >= 0.0f))
                return fail(RT_ERR_INVALID, "rt_scene_set_environment: a texel of the float image is negative or not finite");
        h.rgb.assign(env->rgb, env->rgb + n);
        h.width = env->width;
        h.height = env->height;
    }
    std::memcpy(h.intensity, env->intensity, sizeof h.intensity);
    std::memcpy(h.rotation, env->rotation, sizeof h.rotation);
    sc.environment = std::move(h);
    sc.has_environment = true;
    sc.committed = false;
    return RT_OK;
}

static_assert(RT_SCENE_FLAG_ENVIRONMENT_LIGHT == SCENE_ENVIRONMENT_LIGHT, "the bit the header names");
int rt_scene_set_environment_light(rt_scene *s, double chance)
{
    if (!s) return fail(RT_ERR_INVALID, "rt_scene_set_environment_light: null scene");
    SceneImpl &sc = *S(s);
    if (sc.launches_in_flight > 0)
        return fail(RT_ERR_STATE, "rt_scene_set_environment_light: a render of this scene is in flight (rt_render_finish it first)");
    if (!(chance >= 0.0 && chance <= 1.0)) return fail(RT_ERR_INVALID, "rt_scene_set_environment_light: chance must lie in [0, 1]");
    sc.environment_light = chance;
    sc.committed = false;
    return RT_OK;
}

int rt_scene_get_environment_light(rt_scene *s, double *chance_out, double *effective_out)
{
    if (!s) return fail(RT_ERR_INVALID, "rt_scene_get_environment_light: null scene");
    const SceneImpl &sc = *S(s);
    if (chance_out) *chance_out = sc.environment_light;
    if (effective_out) *effective_out = sc.committed && (sc.flat.flags & SCENE_ENVIRONMENT_LIGHT) ? sc.flat.env.light_share : 0.0;
    return RT_OK;
}

int rt_scene_get_environment(rt_scene *s, rt_environment *out, int *has_distribution)
{
    if (!s || !out) return fail(RT_ERR_INVALID, "rt_scene_get_environment: null argument");
    const SceneImpl &sc = *S(s);
    std::memset(out, 0, sizeof *out);
    if (has_distribution) *has_distribution = 0;
    if (!sc.has_environment) return RT_OK;
    const HostEnvironment &h = sc.environment;
    out->texture = h.texture;
    out->rgb = h.rgb.empty() ? nullptr : h.rgb.data();
    out->width = h.width;
    out->height = h.height;
    std::memcpy(out->intensity, h.intensity, sizeof h.intensity);
    std::memcpy(out->rotation, h.rotation, sizeof h.rotation);
    if (has_distribution) *has_distribution = sc.committed && sc.flat.env.has_distribution ? 1 : 0;
    return RT_OK;
}

int rt_scene_dump_environment_cdf(rt_scene *s, int *width_out, int max_entries, double *marginal_out, double *conditional_out)
{
    if (!s || !S(s)->committed) return -fail(RT_ERR_STATE, "rt_scene_dump_environment_cdf: scene not committed");
    const FlatScene &f = S(s)->flat;
    if (width_out) *width_out = 0;
    if (!(f.flags & SCENE_ENVIRONMENT) || !f.env.has_distribution) return 0;
    if (width_out) *width_out = f.env.width;
    if ((int64_t)max_entries >= (int64_t)f.env.width * f.env.height) {
        if (marginal_out) std::memcpy(marginal_out, f.env_mcdf.data(), f.env_mcdf.size() * sizeof(double));
        if (conditional_out) std::memcpy(conditional_out, f.env_ccdf.data(), f.env_ccdf.size() * sizeof(double));
    }
    return f.env.height;
}

int rt_pfm_load(const char *path, float **rgb_out, int *width, int *height)
{
    if (!path || !rgb_out || !width || !height) return fail(RT_ERR_INVALID, "rt_pfm_load: null argument");
    *rgb_out = nullptr;
    FILE *fp = std::fopen(path, "rb");
    if (!fp) return fail(RT_ERR_INVALID, std::string("rt_pfm_load: cannot open ") + path);
    char magic[3] = {0, 0, 0};
    int w = 0, h = 0;
    double scale = 0.0;
    // "PF", the two sizes and the scale, separated by white space; exactly one white-space byte before the data
    const bool head = std::fscanf(fp, "%2s %d %d %lf", magic, &w, &h, &scale) == 4 && std::strcmp(magic, "PF") == 0 && std::isspace(std::fgetc(fp));
    if (!head || w < 1 || h < 1 || (int64_t)w * h > ((int64_t)1 << 28) || !std::isfinite(scale) || scale == 0.0) {
        std::fclose(fp);
        return fail(RT_ERR_INVALID, std::string("rt_pfm_load: not a colour PFM file: ") + path);
    }
    const size_t row = (size_t)w * 3;
    float *rgb = static_cast<float *>(std::malloc(row * (size_t)h * sizeof(float)));
    if (!rgb) {
        std::fclose(fp);
        return fail(RT_ERR_INVALID, "rt_pfm_load: out of memory");
    }
    const bool little = scale < 0.0;
    const float magnitude = (float)std::fabs(scale);
    bool ok = true;
    for (int j = h - 1; j >= 0 && ok; j--) {  // the file's first row is the bottom one
        float *dst = rgb + (size_t)j * row;
        ok = std::fread(dst, sizeof(float), row, fp) == row;
        for (size_t k = 0; k < row && ok; k++) {
            unsigned char b[4];
            std::memcpy(b, &dst[k], 4);
            const uint32_t bits = little ? (uint32_t)b[0] | (uint32_t)b[1] << 8 | (uint32_t)b[2] << 16 | (uint32_t)b[3] << 24
                                         : (uint32_t)b[3] | (uint32_t)b[2] << 8 | (uint32_t)b[1] << 16 | (uint32_t)b[0] << 24;
            float x;
            std::memcpy(&x, &bits, 4);
            dst[k] = magnitude == 1.0f ? x : magnitude * x;
        }
    }
    std::fclose(fp);
    if (!ok) {
        std::free(rgb);
        return fail(RT_ERR_INVALID, std::string("rt_pfm_load: file ends before its last row: ") + path);
    }
    *rgb_out = rgb;
    *width = w;
    *height = h;
    return RT_OK;
}
void rt_pfm_free(float *rgb) { std::free(rgb); }

int rt_scene_commit(rt_scene *s)
{
    if (!s) return fail(RT_ERR_INVALID, "rt_scene_commit: null scene");
    return flatten_scene(*S(s));
}

int rt_scene_get_info(rt_scene *s, rt_scene_info *out)
{
    if (!s || !out) return fail(RT_ERR_INVALID, "rt_scene_get_info: null argument");
    if (!S(s)->committed) return fail(RT_ERR_STATE, "rt_scene_get_info: scene not committed");
    const FlatScene &f = S(s)->flat;
    std::memset(out, 0, sizeof *out);
    out->world_kind = f.world_kind;
    out->n_leaves = (uint32_t)f.world_items.size();
    out->n_nodes = (uint32_t)f.nodes.size();
    out->n_spheres = (uint32_t)f.spheres.size();
    out->n_moving_spheres = (uint32_t)f.mspheres.size();
    out->n_quads = (uint32_t)f.quads.size();
    out->n_objects = (uint32_t)f.objects.size();
    out->n_xforms = 0;  // steps: a Transform's kAffineRows rows are one
    for (const Xform &x : f.xforms) out->n_xforms += x.kind != XF_AFFINE_ROW;
    out->n_media = (uint32_t)f.media.size();
    out->n_materials = (uint32_t)f.materials.size();
    out->n_textures = (uint32_t)f.textures.size();
    out->n_perlin = (uint32_t)f.perlin.size();
    out->n_images = (uint32_t)f.images.size();
    out->table_bytes = (uint32_t)(f.nodes.size() * sizeof(BvhNodeRec) + f.spheres.size() * sizeof(SphereGeom) +
                                  f.mspheres.size() * sizeof(MSphereGeom) + f.quads.size() * sizeof(QuadGeom) +
                                  f.objects.size() * sizeof(ObjectRec) + f.xforms.size() * sizeof(Xform) +
                                  f.materials.size() * sizeof(MaterialRec));
    out->image_bytes = (uint32_t)f.image_bytes.size();
    for (const AAQuad &a : f.quad_aa) out->reserved[0] += a.code == kQuadTriangle;  // n_triangles (counted in n_quads too)
    out->reserved[1] = (uint32_t)f.lights.size();  // n_lights
    out->reserved[2] = (uint32_t)f.tri_attr.size();  // triangle rows with corner attributes
    return RT_OK;
}

static_assert(sizeof(rt_light_row) == sizeof(LightRow) && offsetof(rt_light_row, s) == offsetof(LightRow, s) &&
                  offsetof(rt_light_row, kind) == offsetof(LightRow, kind) && offsetof(rt_light_row, leaf) == offsetof(LightRow, leaf),
              "rt_light_row is LightRow");
int rt_scene_dump_lights(rt_scene *s, int max_lights, int *kind_out, int *leaf_out, rt_light_row *rows_out, double *cdf_out)
{
    if (!s || !S(s)->committed) return -fail(RT_ERR_STATE, "rt_scene_dump_lights: scene not committed");
    const FlatScene &f = S(s)->flat;
    const int n = (int)f.lights.size();
    for (int k = 0; k < n && k < max_lights; k++) {
        if (kind_out) kind_out[k] = (int)f.lights[k].kind;
        if (leaf_out) leaf_out[k] = (int)f.lights[k].leaf;
        if (rows_out) std::memcpy(&rows_out[k], &f.lights[k], sizeof(LightRow));
        if (cdf_out) {
            cdf_out[2 * k] = f.light_cdf[0][k];
            cdf_out[2 * k + 1] = f.light_cdf[1][k];
        }
    }
    return n;
}

int rt_scene_dump_leaves(rt_scene *s, int max_leaves, int *kind_out, double *box_out)
{
    if (!s || !S(s)->committed) return -fail(RT_ERR_STATE, "rt_scene_dump_leaves: scene not committed");
    const FlatScene &f = S(s)->flat;
    int n = (int)f.world_items.size();
    for (int k = 0; k < n && k < max_leaves; k++) {
        if (kind_out) kind_out[k] = f.leaf_kinds[k];
        if (box_out)
            for (int a = 0; a < 3; a++) {
                box_out[6 * k + 2 * a] = f.leaf_boxes[k].lo[a];
                box_out[6 * k + 2 * a + 1] = f.leaf_boxes[k].hi[a];
            }
    }
    return n;
}
int rt_scene_dump_nodes(rt_scene *s, int max_nodes, double *box_out, uint32_t *abe_out)
{
    if (!s || !S(s)->committed) return -fail(RT_ERR_STATE, "rt_scene_dump_nodes: scene not committed");
    const FlatScene &f = S(s)->flat;
    int n = (int)f.nodes.size();
    for (int k = 0; k < n && k < max_nodes; k++) {
        const BvhNodeRec &r = f.nodes[k];
        if (box_out) {
            double *b = box_out + 6 * k;
            b[0] = r.xlo; b[1] = r.xhi; b[2] = r.ylo; b[3] = r.yhi; b[4] = r.zlo; b[5] = r.zhi;
        }
        if (abe_out) {
            abe_out[3 * k] = r.a;
            abe_out[3 * k + 1] = r.b;
            abe_out[3 * k + 2] = r.escape;
        }
    }
    return n;
}
int rt_scene_dump_fast_nodes(rt_scene *s, int max_nodes, double *box_out, uint32_t *ab_out, uint16_t *link_out)
{
    if (!s || !S(s)->committed) return -fail(RT_ERR_STATE, "rt_scene_dump_fast_nodes: scene not committed");
    const FlatScene &f = S(s)->flat;
    int n = (int)f.fast_nodes.size();
    for (int k = 0; k < n && k < max_nodes; k++) {
        const FastNodeRec &r = f.fast_nodes[k];
        if (box_out) {
            double *b = box_out + 6 * k;
            b[0] = r.xlo; b[1] = r.xhi; b[2] = r.ylo; b[3] = r.yhi; b[4] = r.zlo; b[5] = r.zhi;
        }
        if (ab_out) {
            ab_out[2 * k] = r.a;
            ab_out[2 * k + 1] = r.b;
        }
        if (link_out) std::memcpy(link_out + 16 * k, r.link, sizeof r.link);
    }
    return n;
}
int rt_scene_dump_camera(rt_scene *s, double out27[27])
{
    if (!s || !S(s)->has_camera || !out27) return fail(RT_ERR_STATE, "rt_scene_dump_camera: no camera");
    const CameraRec &c = S(s)->camera;
    const double *vs[8] = {c.bg, c.origin, c.llc, c.horizontal, c.vertical, c.u, c.v, c.w};
    for (int k = 0; k < 8; k++) std::memcpy(out27 + 3 * k, vs[k], 3 * sizeof(double));
    out27[24] = c.lens_radius;
    out27[25] = c.time0;
    out27[26] = c.time1;
    return RT_OK;
}

int rt_scene_dump_scan_segments(rt_scene *s, int max_segments, uint32_t *rows_axis_out, float *shared_out)
{
    if (!s || !S(s)->committed) return -fail(RT_ERR_STATE, "rt_scene_dump_scan_segments: scene not committed");
    const FlatScene &f = S(s)->flat;
    const int n = (int)f.scan_segments.size();
    for (int k = 0; k < n && k < max_segments; k++) {
        const ScanSegment &sg = f.scan_segments[k];
        if (rows_axis_out) {
            rows_axis_out[3 * k] = sg.first_trip * 2u * kScanTripPairs;
            rows_axis_out[3 * k + 1] = sg.n_trips * 2u * kScanTripPairs;
            rows_axis_out[3 * k + 2] = sg.axis;
        }
        if (shared_out) shared_out[k] = sg.c;
    }
    return n;
}

int rt_scene_dump_scan_windows(rt_scene *s, int max_segments, uint32_t *axis_out, float *slab_out, int max_trips, float *spans_out)
{
    if (!s || !S(s)->committed) return -fail(RT_ERR_STATE, "rt_scene_dump_scan_windows: scene not committed");
    const FlatScene &f = S(s)->flat;
    const float inf = std::numeric_limits<float>::infinity();
    const int n = (int)f.scan_segments.size();
    for (int k = 0; k < n && k < max_segments; k++) {
        const ScanWindowSeg w = f.scan_windows.empty() ? ScanWindowSeg{kScanAxisNone, 0.0f, 0.0f, 0u} : f.scan_windows[k];
        if (axis_out) axis_out[k] = w.axis;
        if (slab_out) {
            slab_out[2 * k] = w.slab_lo;
            slab_out[2 * k + 1] = w.slab_hi;
        }
    }
    const int trips = (int)((f.sphere_scan.size() + 2 * kScanTripPairs - 1) / (2 * kScanTripPairs));
    for (int t = 0; t < trips && t < max_trips && spans_out; t++) {
        spans_out[2 * t] = f.scan_trip_spans.empty() ? -inf : f.scan_trip_spans[t].lo;
        spans_out[2 * t + 1] = f.scan_trip_spans.empty() ? inf : f.scan_trip_spans[t].hi;
    }
    return n;
}

int rt_scene_scan_window_trips(rt_scene *s, int n_rays, const double *origin, const double *direction, int max_trips, uint8_t *needed_out)
{
    if (!s || !S(s)->committed) return -fail(RT_ERR_STATE, "rt_scene_scan_window_trips: scene not committed");
    if (n_rays < 0 || (n_rays > 0 && (!origin || !direction))) return -fail(RT_ERR_INVALID, "rt_scene_scan_window_trips: no rays");
    const FlatScene &f = S(s)->flat;
    const int trips = (int)((f.sphere_scan.size() + 2 * kScanTripPairs - 1) / (2 * kScanTripPairs));
    if (!needed_out) return trips;
    if (max_trips < trips) return -fail(RT_ERR_INVALID, "rt_scene_scan_window_trips: max_trips is below the table's trips");
    for (int k = 0; k < n_rays; k++) {
        const double *o = origin + 3 * (size_t)k, *d = direction + 3 * (size_t)k;
        uint8_t *out = needed_out + (size_t)k * (size_t)max_trips;
        for (int t = 0; t < max_trips; t++) out[t] = t < trips ? 1 : 0;
        for (size_t g = 0; g < f.scan_windows.size(); g++) {
            const ScanSegment &sg = f.scan_segments[g];
            const ScanWindowSeg &w = f.scan_windows[g];
            if (w.axis == kScanAxisNone) continue;
            // the kernel's own steps (render.hip scan_filtered32): the extent in fp64, the union's ends in fp32, the test per trip
            const ScanExtent ex = scan_window_extent(o[sg.axis], d[sg.axis], o[w.axis], d[w.axis], std::fabs(o[0]) + std::fabs(o[1]) + std::fabs(o[2]),
                                                     d[0] * d[0] + d[1] * d[1] + d[2] * d[2], f.scan_reach32, (double)w.slab_lo, (double)w.slab_hi);
            const float x0 = (float)ex.lo, x1 = -(-(float)ex.hi);
            for (uint32_t t = 0; t < sg.n_trips; t++) {
                const ScanTripSpan &sp = f.scan_trip_spans[sg.first_trip + t];
                out[sg.first_trip + t] = scan_window_needs(sp.lo, sp.hi, x0, x1) ? 1 : 0;
            }
        }
    }
    return trips;
}

int rt_scene_dump_primary_lists(rt_scene *s, int width, int height, int stripe_rows, int rank, int world_size, int max_tiles, uint16_t *lists_out)
{
    if (!s || !S(s)->committed || !S(s)->has_camera) return -fail(RT_ERR_STATE, "rt_scene_dump_primary_lists: scene not committed, or no camera");
    if (width <= 0 || height <= 0 || stripe_rows <= 0 || world_size <= 0 || rank < 0 || rank >= world_size)
        return -fail(RT_ERR_INVALID, "rt_scene_dump_primary_lists: bad geometry");
    const FlatScene &f = S(s)->flat;
    if (f.spheres.size() > 0xFFFFu) return -fail(RT_ERR_INVALID, "rt_scene_dump_primary_lists: more spheres than a list entry can name");
    const FilmGeometry g = film_geometry(width, height, stripe_rows, rank, world_size);
    for (uint32_t tile = 0; tile < g.n_tiles && (int)tile < max_tiles; tile++) {
        if (!lists_out) break;
        const TileCone cone = primary_tile_cone(S(s)->camera, width, height, primary_tile_pixels(tile, width, g.rows_owned, stripe_rows, rank, world_size));
        primary_list_for_tile(cone, f.spheres.data(), (uint32_t)f.spheres.size(), lists_out + (size_t)tile * kPrimaryListWords);
    }
    return (int)g.n_tiles;
}

int rt_stripe_rows(int height, int stripe_rows, int rank, int world_size, int *rows_out, int max_rows)
{
    if (height < 0 || stripe_rows <= 0 || world_size <= 0 || rank < 0 || rank >= world_size) return -1;
    int n = 0;
    for (int j = 0; j < height; j++)
        if ((j / stripe_rows) % world_size == rank) {
            if (rows_out && n < max_rows) rows_out[n] = j;
            n++;
        }
    return n;
}

int rt_deinterleave(const double *gathered, int width, int height, int stripe_rows, int world_size,
                    size_t rank_stride_doubles, double *frame_full)
{
    if (!gathered || !frame_full || width <= 0 || height <= 0 || stripe_rows <= 0 || world_size <= 0)
        return fail(RT_ERR_INVALID, "rt_deinterleave: bad arguments");
    std::vector<size_t> next(world_size, 0);
    for (int j = 0; j < height; j++) {
        int r = (j / stripe_rows) % world_size;
        const double *src = gathered + (size_t)r * rank_stride_doubles + next[r] * (size_t)width * 3;
        std::memcpy(frame_full + (size_t)j * width * 3, src, sizeof(double) * (size_t)width * 3);
        next[r]++;
    }
    return RT_OK;
}

int rt_write_ppm_binary(const char *path, const double *frame, int width, int height)
{
    if (!path || !frame || width <= 0 || height <= 0) return fail(RT_ERR_INVALID, "rt_write_ppm_binary: bad arguments");
    FILE *fp = std::fopen(path, "wb");
    if (!fp) return fail(RT_ERR_INVALID, std::string("rt_write_ppm_binary: cannot open ") + path);
    std::fprintf(fp, "P6\n%d %d\n255\n", width, height);
    std::vector<unsigned char> row((size_t)width * 3);
    for (int j = height - 1; j >= 0; j--) {  // same clamp and int(256 * c) as R/kernel.cu:710-718
        for (int i = 0; i < width * 3; i++) {
            double c = frame[(size_t)j * width * 3 + i];
            double x = c < 0.0 ? 0.0 : (c > 0.999 ? 0.999 : c);
            row[i] = (unsigned char)(int)(256.0 * x);
        }
        std::fwrite(row.data(), 1, row.size(), fp);
    }
    std::fclose(fp);
    return RT_OK;
}

int rt_write_pfm(const char *path, const double *frame, int width, int height)
{
    if (!path || !frame || width <= 0 || height <= 0) return fail(RT_ERR_INVALID, "rt_write_pfm: bad arguments");
    FILE *fp = std::fopen(path, "wb");
    if (!fp) return fail(RT_ERR_INVALID, std::string("rt_write_pfm: cannot open ") + path);
    std::fprintf(fp, "PF\n%d %d\n-1.0\n", width, height);
    std::vector<float> row((size_t)width * 3);
    for (int j = 0; j < height; j++) {  // PFM stores the bottom row first: the frame's own order (j = 0 bottom)
        for (int i = 0; i < width * 3; i++) row[i] = (float)frame[(size_t)j * width * 3 + i];
        std::fwrite(row.data(), sizeof(float), row.size(), fp);
    }
    std::fclose(fp);
    return RT_OK;
}

int rt_write_ppm(const char *path, const double *frame, int width, int height)
{
    if (!path || !frame || width <= 0 || height <= 0) return fail(RT_ERR_INVALID, "rt_write_ppm: bad arguments");
    FILE *fp = std::fopen(path, "w");
    if (!fp) return fail(RT_ERR_INVALID, std::string("rt_write_ppm: cannot open ") + path);
    // R/kernel.cu:696-721: text P3, top row (j = H-1) first, clamp to [0, 0.999], int(256 * c)
    std::string buf;
    buf.reserve((size_t)width * 12 * 64);
    std::fprintf(fp, "P3\n%d %d\n255\n", width, height);
    char line[64];
    for (int j = height - 1; j >= 0; j--) {
        buf.clear();
        for (int i = 0; i < width; i++) {
            const double *c = frame + ((size_t)j * width + i) * 3;
            int q[3];
            for (int k = 0; k < 3; k++) {
                double x = c[k] < 0.0 ? 0.0 : (c[k] > 0.999 ? 0.999 : c[k]);
                q[k] = (int)(256.0 * x);
            }
            int n = std::snprintf(line, sizeof line, "%d %d %d\n", q[0], q[1], q[2]);
            buf.append(line, (size_t)n);
        }
        std::fwrite(buf.data(), 1, buf.size(), fp);
    }
    std::fclose(fp);
    return RT_OK;
}

} // extern "C"
