// scene_host.h -- host-side object graph behind the construction API, and its flattened form.
// Internal to librtow_hip.so.
#pragma once
#include <cstdint>
#include <string>
#include <vector>

#include "flat_scene.h"
#include "rng.h"

namespace rtow {

struct D3 {
    double x, y, z;
};

struct Box {  // R/AABB.h:16-22: three closed intervals
    double lo[3], hi[3];
};

enum class HKind : uint8_t { Sphere, MovingSphere, Quad, Translate, RotateY, List, Bvh, Medium,
                             Triangle,    // the quad's fields and plane constants; corners Q, Q + u, Q + v
                             Transform,   // a general affine instance (rt_transform): HostHittable::xf
                             MovingTransform };  // an affine instance keyed at two times (rt_moving_transform): HostHittable::xf
// The numbers of a Transform exactly as rt_transform stored them and as they are uploaded: x_world = L x_obj + t, Li = inverse of L.
struct HostAffine {
    double L[9], t[3], Li[9];  // L, Li row-major
};
// The numbers of a MovingTransform exactly as rt_moving_transform stored them and as they are uploaded (rt_moving_transform_get).
struct HostMovingAffine {
    double L0[9], t0[3], dL[9], dt[3], time0, dtime;  // L0, dL row-major
};

struct HostHittable {
    HKind kind;
    Box box;
    uint32_t material = 0;             // handle (1-based) for primitives; phase function for media
    D3 c0{}, c1{};                     // sphere centre(s)
    double t0 = 0, t1 = 0, radius = 0;
    D3 q{}, u{}, v{}, w{}, normal{};   // quad, triangle
    double plane_d = 0;
    uint32_t attr = 0;                 // triangle with corner normals / texture coordinates: 1 + its row of SceneImpl::tri_attr
    uint32_t child = 0;                // instance / medium: wrapped hittable handle
    D3 offset{};
    double sin_t = 0, cos_t = 0;
    uint32_t xf = 0;                   // Transform: 1 + its row of SceneImpl::transforms; MovingTransform: of SceneImpl::moving_transforms
    std::vector<uint32_t> items;       // list children / bvh leaves (in sorted order, after build)
    double neg_inv_density = 0;
    // bvh topology (built at construction): nodes in preorder
    struct TreeNode {
        Box box;
        int left, right;               // child tree-node indices, or -1
        uint32_t leaf_a, leaf_b;       // hittable handles when bottom node, else 0
    };
    std::vector<TreeNode> tree;
};

struct HostMaterial {
    uint32_t kind;
    uint32_t texture = 0;  // handle (1-based) or 0
    D3 albedo{};
    double p = 0;
};

struct HostTexture {
    uint32_t kind;
    D3 color{};
    double s = 0;
    uint32_t a = 0, b = 0;  // checker: even/odd handles; image: image index; noise: perlin index
};

struct MsInterval {
    double t0, dt;
};

struct FlatScene {
    std::vector<SphereGeom> spheres;
    std::vector<SphereScanRow> sphere_scan;  // parallel to spheres
    double scan_reach = 0.0;
    std::vector<SphereScanPair> sphere_scan32;  // pairs of sphere_scan rows in fp32
    double scan_reach32 = 0.0;
    std::vector<ScanSegment> scan_segments;  // tile the trips of sphere_scan32 in order (flat_scene.h ScanSegment)
    // the windows of the runs (flat_scene.h ScanWindowSeg, ScanTripSpan): one record per segment, one span per trip; both empty
    // where no run has a table
    std::vector<ScanWindowSeg> scan_windows;
    std::vector<ScanTripSpan> scan_trip_spans;
    std::vector<SphereAux> sphere_aux;
    std::vector<MSphereGeom> mspheres;
    std::vector<double> ms_planes;       // SCENE_WORLD_MSPHERES: seven planes of ms_padded doubles (see DeviceScene)
    uint32_t ms_padded = 0;
    std::vector<SphereAux> msphere_aux;
    std::vector<QuadGeom> quads;
    std::vector<AAQuad> quad_aa;
    std::vector<TriAttrRow> tri_attr;    // SCENE_VERTEX_ATTR: row k is quads[quads.size() + k] on the device (flat_scene.h TriAttrRow)
    std::vector<BoxRec> boxes;
    std::vector<uint32_t> quad_mat;
    std::vector<ObjectRec> objects;
    std::vector<uint32_t> items;
    std::vector<Xform> xforms;
    std::vector<MediumRec> media;
    std::vector<GroupBox> group_boxes;
    std::vector<TreeNodeRec> tree_nodes;
    std::vector<uint32_t> tree_items;
    std::vector<BvhNodeRec> tree_bvh;
    std::vector<BvhNodeRec> nodes;
    std::vector<FastNodeRec> fast_nodes;
    std::vector<FastOrder> fast_order;   // SCENE_SEGMENTED
    std::vector<SegMedium> seg_media;    // SCENE_SEGMENTED
    std::vector<SegCandidate> seg_cand;  // SCENE_SEGMENTED
    std::vector<uint32_t> world_items;   // leaf refs in final order (both world kinds)
    std::vector<uint32_t> node_leaf_pos; // WORLD_BVH: per world node, the positions in world_items of a bottom node's leaves a and b (ray queries)
    std::vector<Box> leaf_boxes;         // introspection
    std::vector<int> leaf_kinds;         // introspection: the leaf's kind as constructed (0 sphere, 1 moving sphere, 2 quad, 3 composite, 4 triangle)
    std::vector<MaterialRec> materials;
    std::vector<TextureRec> textures;
    std::vector<ImageRec> images;
    std::vector<unsigned char> image_bytes;
    std::vector<PerlinRec> perlin;
    uint32_t world_kind = WORLD_BVH;
    uint32_t flags = 0;
    uint32_t n_world_nodes = 0;
    uint32_t scan_cost = 0;  // cost of testing every world leaf once (scene_builder.cpp), for the scan-or-walk choice
    // Moving-sphere rows whose centre moves (dc != 0) over an interval of non-zero length (dt != 0): their distinct (t0, dt).
    // The launcher checks them against the camera's shutter (launch_plan.cpp hits_stay_in_boxes); ms_nonfinite: such a
    // row has a non-finite centre, motion or interval, and no shutter keeps it inside its box.
    std::vector<MsInterval> ms_intervals;
    bool ms_nonfinite = false;
    // The emissive world primitives in world space, in the depth-first construction order of the world (scene_builder.cpp
    // collect_lights), and their cumulative selection tables: [0] uniform over lights, [1] by area x the brightest channel.  Each
    // table's entry lights.size() - 1 is exactly 1.0; both are padded with 1.0 to an even length (the kernels stage them in LDS
    // with 16-byte loads).
    std::vector<LightRow> lights;
    std::vector<double> light_cdf[2];
    // SCENE_ENVIRONMENT: the record as it is uploaded behind the camera's, its three pointers null (device_scene.cpp sets them), the
    // float image, and the importance sampler's tables (scene_builder.cpp build_environment; empty: no distribution)
    EnvRec env{};
    std::vector<float> env_rgb;
    std::vector<double> env_mcdf, env_ccdf;
};

// The environment exactly as rt_scene_set_environment took it (rt_scene_get_environment hands it back).
struct HostEnvironment {
    uint32_t texture = 0;  // handle (1-based), or 0: the float image
    std::vector<float> rgb;
    int32_t width = 0, height = 0;
    double intensity[3] = {1.0, 1.0, 1.0};
    double rotation[9] = {1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0};
};

struct DeviceTables;  // device_scene.cpp

struct SceneImpl {
    std::vector<HostHittable> hittables;  // handle = index + 1
    std::vector<HostMaterial> materials;
    std::vector<HostTexture> textures;
    std::vector<TriAttrRow> tri_attr;     // HostHittable::attr
    std::vector<HostAffine> transforms;   // HostHittable::xf
    std::vector<HostMovingAffine> moving_transforms;  // HostHittable::xf of a MovingTransform
    std::vector<ImageRec> images;
    std::vector<unsigned char> image_bytes;
    std::vector<PerlinRec> perlin;
    uint32_t world = 0;
    bool has_camera = false;
    CameraRec camera{};
    bool has_environment = false;
    HostEnvironment environment;
    double environment_light = 0.0;  // rt_scene_set_environment_light's chance, read by the next rt_scene_commit; it outlives a change of environment
    bool committed = false;
    FlatScene flat;
    std::vector<DeviceTables *> device;  // one per device ordinal, lazily
    // Every change the device copies depend on (a commit, a new camera) bumps `generation`; rt_scene_upload replaces a
    // device's tables when they are older.  `launches_in_flight` counts rt_render_launch calls not yet finished: the
    // scene may not be changed while a kernel may still be reading its tables.
    uint64_t generation = 0;
    int launches_in_flight = 0;
    std::vector<void *> films_in_flight;  // the FilmImpl of every launch counted above (device_scene.cpp)
    uint32_t options = 0;                 // RT_SCENE_* (rt_scene_set_options), read by the next rt_scene_commit

    ~SceneImpl();
};

struct RngImpl {
    Xorwow state;
};

// error plumbing (thread-local message)
void set_error(const std::string &msg);
int fail(int status, const std::string &msg);

// host jump table for curand_init's sequence skip (built once, on first use)
const uint32_t *host_jump_table();

// flattening (scene_builder.cpp)
int flatten_scene(SceneImpl &s);

// device side (device_scene.cpp)
void release_device_tables(DeviceTables *t);
// A scene that goes away while launches are in flight: wait for each of them and make their films forget the scene
// (rt_scene_destroy; the films stay valid, their rt_render_finish then only reports).
void wait_for_films_in_flight(SceneImpl &s);

} // namespace rtow
