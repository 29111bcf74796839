// rtow.hpp -- header-only C++17 veneer over the C-ABI (rtow.h).
//
// Keeps scene code shaped like the reference's CreateWorld (R/kernel.cu:199-517): the same
// constructor names and parameter lists (Sphere(center, radius, material), Lambertian(color),
// CheckerTexture(scale, even, odd), MakeBox(a, b, material), Translate(object, offset), ...),
// returning small value handles instead of device pointers.  Ownership is the scene's: nothing
// to delete, sharing a child between two parents is fine (the reference double-frees there,
// Docs 2-10 :202-213).
#pragma once
#include <limits>
#include <stdexcept>
#include <string>
#include <vector>

#include "rtow.h"

namespace rtow_api {

struct Vector3 {
    double x = 0, y = 0, z = 0;
    Vector3() = default;
    Vector3(double a, double b, double c) : x(a), y(b), z(c) {}
};
using Point3 = Vector3;
using Color = Vector3;

struct Texture { rt_handle h = 0; };
struct Material { rt_handle h = 0; };
struct Hittable { rt_handle h = 0; };

class Error : public std::runtime_error {
public:
    using std::runtime_error::runtime_error;
};

// curandState stand-in for scene generation: Rng rng(1984, 0); float u = rng();   (RND macro, R/kernel.cu:157)
class Rng {
public:
    Rng(unsigned long long seed, unsigned long long sequence) : r_(rt_rng_create(seed, sequence)) {}
    ~Rng() { rt_rng_destroy(r_); }
    Rng(const Rng &) = delete;
    Rng &operator=(const Rng &) = delete;
    float operator()() { return rt_rng_uniform(r_); }
    rt_rng *raw() { return r_; }

private:
    rt_rng *r_;
};

class Scene {
public:
    Scene() : s_(rt_scene_create()) {}
    ~Scene() { if (own_) rt_scene_destroy(s_); }
    explicit Scene(rt_scene *borrowed) : s_(borrowed), own_(false) {}
    Scene(const Scene &) = delete;
    Scene &operator=(const Scene &) = delete;
    rt_scene *raw() { return s_; }

    // textures (R/Texture.h)
    Texture SolidColor(const Color &c) { return {ok(rt_solid_color(s_, c.x, c.y, c.z))}; }
    Texture SolidColor(double r, double g, double b) { return {ok(rt_solid_color(s_, r, g, b))}; }
    Texture CheckerTexture(double scale, Texture even, Texture odd) { return {ok(rt_checker_texture(s_, scale, even.h, odd.h))}; }
    Texture ImageTexture(const unsigned char *rgb, int w, int h) { return {ok(rt_image_texture(s_, rgb, w, h))}; }
    Texture NoiseTexture(double scale, Rng &rng) { return {ok(rt_noise_texture(s_, scale, rng.raw()))}; }

    // materials (R/Material.h, R/Metal.h, R/Dielectric.h)
    Material Lambertian(const Color &c) { return {ok(rt_lambertian(s_, c.x, c.y, c.z))}; }
    Material Lambertian(Texture t) { return {ok(rt_lambertian_tex(s_, t.h))}; }
    Material Metal(const Color &c, double fuzz) { return {ok(rt_metal(s_, c.x, c.y, c.z, fuzz))}; }
    Material Dielectric(double ior) { return {ok(rt_dielectric(s_, ior))}; }
    Material DiffuseLight(const Color &c) { return {ok(rt_diffuse_light(s_, c.x, c.y, c.z))}; }
    Material DiffuseLight(Texture t) { return {ok(rt_diffuse_light_tex(s_, t.h))}; }
    Material Isotropic(const Color &c) { return {ok(rt_isotropic(s_, c.x, c.y, c.z))}; }
    Material Isotropic(Texture t) { return {ok(rt_isotropic_tex(s_, t.h))}; }

    // hittables
    Hittable Sphere(const Point3 &c, double r, Material m) { return {ok(rt_sphere(s_, c.x, c.y, c.z, r, m.h))}; }
    Hittable MovingSphere(const Point3 &c0, const Point3 &c1, double t0, double t1, double r, Material m)
    {
        return {ok(rt_moving_sphere(s_, c0.x, c0.y, c0.z, c1.x, c1.y, c1.z, t0, t1, r, m.h))};
    }
    Hittable Quad(const Point3 &q, const Vector3 &u, const Vector3 &v, Material m)
    {
        const double qq[3] = {q.x, q.y, q.z}, uu[3] = {u.x, u.y, u.z}, vv[3] = {v.x, v.y, v.z};
        return {ok(rt_quad(s_, qq, uu, vv, m.h))};
    }
    Hittable Triangle(const Point3 &q, const Vector3 &u, const Vector3 &v, Material m)
    {
        const double qq[3] = {q.x, q.y, q.z}, uu[3] = {u.x, u.y, u.z}, vv[3] = {v.x, v.y, v.z};
        return {ok(rt_triangle(s_, qq, uu, vv, m.h))};
    }
    // rt_triangle_mesh: a BvhNode over the triangles; `triangles`, if given, receives them in input order
    Hittable TriangleMesh(const std::vector<Point3> &vertices, const std::vector<int32_t> &indices, Material m, std::vector<Hittable> *triangles = nullptr)
    {
        std::vector<double> xyz;
        for (const Point3 &p : vertices) xyz.insert(xyz.end(), {p.x, p.y, p.z});
        std::vector<rt_handle> hs(indices.size() / 3);
        const rt_handle root = ok(rt_triangle_mesh(s_, xyz.data(), (int)vertices.size(), indices.data(), (int)(indices.size() / 3), m.h, hs.data()));
        if (triangles) {
            triangles->clear();
            for (rt_handle h : hs) triangles->push_back({h});
        }
        return {root};
    }
    // rt_triangle_attr: corner normals (three) and / or corner texture coordinates (three (u, v) pairs); nullptr = none
    Hittable Triangle(const Point3 &q, const Vector3 &u, const Vector3 &v, Material m, const Vector3 *normals, const double *texcoords = nullptr)
    {
        const double qq[3] = {q.x, q.y, q.z}, uu[3] = {u.x, u.y, u.z}, vv[3] = {v.x, v.y, v.z};
        double nn[9] = {};
        for (int c = 0; normals && c < 3; c++) nn[3 * c] = normals[c].x, nn[3 * c + 1] = normals[c].y, nn[3 * c + 2] = normals[c].z;
        return {ok(rt_triangle_attr(s_, qq, uu, vv, normals ? nn : nullptr, texcoords, m.h))};
    }
    // rt_triangle_mesh_attr: `normals` indexed by `normal_indices`, `texcoords` (u, v pairs) by `texcoord_indices`; an empty attribute
    // array = none of that kind, an empty index array = `indices`
    Hittable TriangleMesh(const std::vector<Point3> &vertices, const std::vector<int32_t> &indices, Material m, const std::vector<Vector3> &normals,
                          const std::vector<int32_t> &normal_indices = {}, const std::vector<double> &texcoords = {},
                          const std::vector<int32_t> &texcoord_indices = {}, std::vector<Hittable> *triangles = nullptr)
    {
        if ((!normal_indices.empty() && normal_indices.size() != indices.size()) || (!texcoord_indices.empty() && texcoord_indices.size() != indices.size()))
            throw Error("TriangleMesh: an attribute index array must be as long as indices");
        std::vector<double> xyz, nrm;
        for (const Point3 &p : vertices) xyz.insert(xyz.end(), {p.x, p.y, p.z});
        for (const Vector3 &n : normals) nrm.insert(nrm.end(), {n.x, n.y, n.z});
        std::vector<rt_handle> hs(indices.size() / 3);
        const rt_handle root = ok(rt_triangle_mesh_attr(
            s_, xyz.data(), (int)vertices.size(), indices.data(), (int)(indices.size() / 3), normals.empty() ? nullptr : nrm.data(), (int)normals.size(),
            normal_indices.empty() ? nullptr : normal_indices.data(), texcoords.empty() ? nullptr : texcoords.data(), (int)(texcoords.size() / 2),
            texcoord_indices.empty() ? nullptr : texcoord_indices.data(), m.h, hs.data()));
        if (triangles) {
            triangles->clear();
            for (rt_handle h : hs) triangles->push_back({h});
        }
        return {root};
    }
    Hittable Translate(Hittable o, const Vector3 &off) { return {ok(rt_translate(s_, o.h, off.x, off.y, off.z))}; }
    Hittable RotateY(Hittable o, double degrees) { return {ok(rt_rotate_y(s_, o.h, degrees))}; }
    // general affine instances (rt_transform): m = row-major 3x4, x_world = L x_obj + t
    Hittable Transform(Hittable o, const double m[12]) { return {ok(rt_transform(s_, o.h, m))}; }
    Hittable RotateX(Hittable o, double degrees) { return {ok(rt_rotate_x(s_, o.h, degrees))}; }
    Hittable RotateZ(Hittable o, double degrees) { return {ok(rt_rotate_z(s_, o.h, degrees))}; }
    Hittable Scale(Hittable o, double sx, double sy, double sz) { return {ok(rt_scale(s_, o.h, sx, sy, sz))}; }
    // moving instances (rt_moving_transform): m0 holds at time0, m1 at time1, interpolated entry by entry per ray
    Hittable MovingTransform(Hittable o, const double m0[12], const double m1[12], double time0 = 0.0, double time1 = 1.0)
    {
        return {ok(rt_moving_transform(s_, o.h, m0, m1, time0, time1))};
    }
    Hittable MovingTranslate(Hittable o, const Vector3 &off0, const Vector3 &off1, double time0 = 0.0, double time1 = 1.0)
    {
        const double a[3] = {off0.x, off0.y, off0.z}, b[3] = {off1.x, off1.y, off1.z};
        return {ok(rt_moving_translate(s_, o.h, a, b, time0, time1))};
    }
    // L0 (9), t0 (3), dL (9), dt (3), time0, time1 - time0 of a moving instance as stored and uploaded (rt_moving_transform_get)
    void MovingTransformKeys(Hittable moving, double out26[26]) { check(rt_moving_transform_get(s_, moving.h, out26)); }
    Hittable MakeBox(const Point3 &a, const Point3 &b, Material m)
    {
        const double aa[3] = {a.x, a.y, a.z}, bb[3] = {b.x, b.y, b.z};
        return {ok(rt_make_box(s_, aa, bb, m.h))};
    }
    Hittable HittableList(const std::vector<Hittable> &items)
    {
        std::vector<rt_handle> hs;
        for (const auto &i : items) hs.push_back(i.h);
        return {ok(rt_hittable_list(s_, hs.data(), (int)hs.size()))};
    }
    Hittable ConstantMedium(Hittable boundary, double density, const Color &c)
    {
        return {ok(rt_constant_medium(s_, boundary.h, density, c.x, c.y, c.z))};
    }
    Hittable ConstantMedium(Hittable boundary, double density, Texture t)
    {
        return {ok(rt_constant_medium_tex(s_, boundary.h, density, t.h))};
    }
    // BvhNode(list, 0, n, ...): sorts `items` in place like the reference does with list[]
    Hittable BvhNode(std::vector<Hittable> &items)
    {
        std::vector<rt_handle> hs;
        for (const auto &i : items) hs.push_back(i.h);
        rt_handle root = ok(rt_bvh_node(s_, hs.data(), (int)hs.size()));
        for (size_t k = 0; k < hs.size(); k++) items[k].h = hs[k];
        return {root};
    }

    void SetWorld(Hittable world) { check(rt_scene_set_world(s_, world.h)); }
    void Camera(const Point3 &lookfrom, const Point3 &lookat, const Vector3 &vup, double vfov, double aspect,
                double aperture, double focusDist, double time0 = 0.0, double time1 = 0.0,
                const Color &background = Color(0.70, 0.80, 1.00))
    {
        const double f[3] = {lookfrom.x, lookfrom.y, lookfrom.z}, a[3] = {lookat.x, lookat.y, lookat.z};
        const double u[3] = {vup.x, vup.y, vup.z}, bg[3] = {background.x, background.y, background.z};
        check(rt_scene_set_camera(s_, f, a, u, vfov, aspect, aperture, focusDist, time0, time1, bg));
    }
    // What a ray that leaves the world sees in place of the camera's background (rtow.h "the environment"): a texture of this
    // scene, or a linear float image of width x height x 3 values, top row first (copied).  rotation: row-major 3 x 3, world ->
    // environment, nullptr = identity.  Takes effect with the next Commit.
    void Environment(Texture texture, const Color &intensity = Color(1.0, 1.0, 1.0), const double *rotation = nullptr)
    {
        set_environment(texture.h, nullptr, 0, 0, intensity, rotation);
    }
    void Environment(const float *rgb, int width, int height, const Color &intensity = Color(1.0, 1.0, 1.0), const double *rotation = nullptr)
    {
        set_environment(0, rgb, width, height, intensity, rotation);
    }
    void NoEnvironment() { check(rt_scene_set_environment(s_, nullptr)); }
    // The environment as a light of the direct estimators (rtow.h rt_scene_set_environment_light): the share of the light samples
    // that go to it where the scene also has lamps.  Takes effect with the next Commit.
    void EnvironmentLight(double chance = 0.5) { check(rt_scene_set_environment_light(s_, chance)); }
    // c_e of the committed scene (0 before Commit, without an environment and at chance 0); *chance: as set
    double EnvironmentLightShare(double *chance = nullptr)
    {
        double effective = 0.0;
        check(rt_scene_get_environment_light(s_, chance, &effective));
        return effective;
    }
    void Commit() { check(rt_scene_commit(s_)); }

    // Ray queries on host arrays (rtow.h "ray queries"): origins and directions hold 3 doubles per ray; an output vector is
    // filled only where `want` names it ("t normal uv albedo leaf front_face material", any subset, space separated).
    struct Hits {
        std::vector<double> t, normal, uv, albedo;
        std::vector<int32_t> leaf;
        std::vector<uint8_t> front_face, material;
    };
    Hits Intersect(const std::vector<double> &origins, const std::vector<double> &directions, rt_query_params params = DefaultQuery(),
                   const std::string &want = "t normal uv albedo leaf front_face material", const double *times = nullptr)
    {
        if (origins.size() != directions.size() || origins.size() % 3 != 0) throw Error("Intersect: origins and directions must hold 3 doubles per ray");
        const size_t n = origins.size() / 3;
        Hits out;
        auto wanted = [&](const char *name) { return (" " + want + " ").find(std::string(" ") + name + " ") != std::string::npos; };
        if (wanted("t")) out.t.resize(n);
        if (wanted("normal")) out.normal.resize(3 * n);
        if (wanted("uv")) out.uv.resize(2 * n);
        if (wanted("albedo")) out.albedo.resize(3 * n);
        if (wanted("leaf")) out.leaf.resize(n);
        if (wanted("front_face")) out.front_face.resize(n);
        if (wanted("material")) out.material.resize(n);
        params.count = (int64_t)n;
        params.mode = 0;
        auto ptr = [](auto &v) { return v.empty() ? nullptr : v.data(); };
        const rt_query_rays rays{origins.data(), directions.data(), times, nullptr, nullptr};
        const rt_query_hits hits{ptr(out.t), ptr(out.normal), ptr(out.uv), ptr(out.albedo), ptr(out.leaf), ptr(out.front_face), ptr(out.material), nullptr};
        check(rt_scene_intersect(s_, &params, &rays, &hits, nullptr));
        return out;
    }
    std::vector<uint8_t> Occluded(const std::vector<double> &origins, const std::vector<double> &directions, rt_query_params params = DefaultQuery(),
                                  const double *times = nullptr)
    {
        if (origins.size() != directions.size() || origins.size() % 3 != 0) throw Error("Occluded: origins and directions must hold 3 doubles per ray");
        std::vector<uint8_t> out(origins.size() / 3);
        params.count = (int64_t)out.size();
        params.mode = 1;
        const rt_query_rays rays{origins.data(), directions.data(), times, nullptr, nullptr};
        const rt_query_hits hits{nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, out.data()};
        check(rt_scene_intersect(s_, &params, &rays, &hits, nullptr));
        return out;
    }
    // what a render passes: [0.001, inf), time 0, seed 1984, the strict build, device 0
    static rt_query_params DefaultQuery()
    {
        rt_query_params p{};
        p.tmin = 0.001;
        p.tmax = std::numeric_limits<double>::infinity();
        p.seed = 1984;
        return p;
    }

    // One bounce for a batch of paths, the ended ones folded and the live rays kept packed (rtow.h "path advances"): the structs
    // pass through as they are.  Device pointers and no statistics: the call is enqueued on params.stream and returns.
    void PathAdvance(const rt_path_advance_params &params, const rt_path_advance_rays &rays, const rt_path_advance_out &out,
                     rt_path_advance_stats *stats = nullptr, bool device_pointers = true)
    {
        check(device_pointers ? rt_scene_path_advance_device(s_, &params, &rays, &out, stats) : rt_scene_path_advance(s_, &params, &rays, &out, stats));
    }

    // The same with a light sample, its shadow ray and the MIS weights at every diffuse hit (rtow.h "path advances with light
    // samples"): params.sample = 1 in every call of a path but its last.
    void PathAdvanceDirect(const rt_path_advance_direct_params &params, const rt_path_advance_direct_rays &rays,
                           const rt_path_advance_direct_out &out, rt_path_advance_direct_stats *stats = nullptr, bool device_pointers = true)
    {
        check(device_pointers ? rt_scene_path_advance_direct_device(s_, &params, &rays, &out, stats)
                              : rt_scene_path_advance_direct(s_, &params, &rays, &out, stats));
    }

    // Whole paths with those light samples, any number of samples a ray, in one launch (rtow.h "radiance queries with light
    // samples"): rays and outputs are the plain radiance query's structs.  The call returns when the results are there.
    void RadianceDirect(const rt_radiance_direct_params &params, const rt_radiance_rays &rays, const rt_radiance_out &out,
                        rt_radiance_direct_stats *stats = nullptr, bool device_pointers = true)
    {
        check(device_pointers ? rt_scene_radiance_direct_device(s_, &params, &rays, &out, stats) : rt_scene_radiance_direct(s_, &params, &rays, &out, stats));
    }

private:
    rt_handle ok(rt_handle h)
    {
        if (!h) throw Error(rt_last_error());
        return h;
    }
    void check(int status)
    {
        if (status != RT_OK) throw Error(rt_last_error());
    }
    void set_environment(rt_handle texture, const float *rgb, int width, int height, const Color &intensity, const double *rotation)
    {
        rt_environment env{};
        env.texture = texture;
        env.rgb = rgb;
        env.width = width;
        env.height = height;
        env.intensity[0] = intensity.x;
        env.intensity[1] = intensity.y;
        env.intensity[2] = intensity.z;
        for (int k = 0; k < 9; k++) env.rotation[k] = rotation ? rotation[k] : (k % 4 == 0 ? 1.0 : 0.0);
        check(rt_scene_set_environment(s_, &env));
    }
    rt_scene *s_;
    bool own_ = true;
};

// A film on one GPU with the feature pass and the a-trous filter (rtow.h "first-hit feature buffers"): render, then
//   film.RenderFeatures(scene); film.Denoise(); auto clean = film.Denoised();
class Film {
public:
    struct Features {
        std::vector<double> albedo, normal, depth;  // W*H*3, W*H*3, W*H; pixel (i, j) at j*W+i, j = 0 bottom
    };
    Film(int device, int width, int height, int stripe_rows = 8, int rank = 0, int world_size = 1)
        : f_(rt_film_create(device, width, height, stripe_rows, rank, world_size)), w_(width), h_(height)
    {
        if (!f_) throw Error(rt_last_error());
    }
    ~Film() { rt_film_destroy(f_); }
    Film(const Film &) = delete;
    Film &operator=(const Film &) = delete;
    rt_film *raw() { return f_; }

    rt_render_stats Render(Scene &scene, const rt_render_params &params)
    {
        rt_render_stats st{};
        check(rt_render_launch(scene.raw(), f_, &params));
        check(rt_render_finish(scene.raw(), f_, &st));
        return st;
    }
    // the same frame with light samples (rtow.h "frames with light samples"): strategy 0 uniform over lights, 1 by area x brightest
    // channel; the shadow statistics of the launch come back through `direct` where given
    rt_render_stats RenderDirect(Scene &scene, const rt_render_params &params, int strategy = 1, rt_film_direct_stats *direct = nullptr)
    {
        rt_render_stats st{};
        rt_film_direct_params dp{};
        dp.strategy = strategy;
        check(rt_render_launch_direct(scene.raw(), f_, &params, &dp));
        check(rt_render_finish(scene.raw(), f_, &st));
        if (direct) check(rt_film_last_direct_stats(f_, direct));
        return st;
    }
    std::vector<double> Download()
    {
        std::vector<double> frame((size_t)w_ * h_ * 3);
        check(rt_film_download(f_, frame.data(), w_, h_));
        return frame;
    }
    void RenderFeatures(Scene &scene, int samples = 0, unsigned long long seed = 1984, int variant = 0, void *stream = nullptr)
    {
        rt_feature_params p{};
        p.width = w_;
        p.height = h_;
        p.samples = samples;
        p.seed = seed;
        p.variant = variant;
        p.stream = stream;
        check(rt_film_render_features(scene.raw(), f_, &p));
    }
    Features DownloadFeatures()
    {
        Features out;
        out.albedo.resize((size_t)w_ * h_ * 3);
        out.normal.resize((size_t)w_ * h_ * 3);
        out.depth.resize((size_t)w_ * h_);
        check(rt_film_download_features(f_, out.albedo.data(), out.normal.data(), out.depth.data(), w_, h_));
        return out;
    }
    void *DeviceFeatures(int which) { return rt_film_device_features(f_, which); }
    void Denoise(const rt_denoise_params &params = rt_denoise_params{5, 0.6, 0.1, 0.3, 0.1}) { check(rt_film_denoise(f_, &params)); }
    std::vector<double> Denoised()
    {
        std::vector<double> frame((size_t)w_ * h_ * 3);
        check(rt_film_download_denoised(f_, frame.data(), w_, h_));
        return frame;
    }

private:
    void check(int status)
    {
        if (status != RT_OK) throw Error(rt_last_error());
    }
    rt_film *f_;
    int w_, h_;
};

// rt_denoise_frame on host frames (gathered from several ranks): albedo, normal, depth may each be null
inline std::vector<double> DenoiseFrame(int device, const double *color, const double *albedo, const double *normal, const double *depth, int width,
                                        int height, const rt_denoise_params &params = rt_denoise_params{5, 0.6, 0.1, 0.3, 0.1})
{
    std::vector<double> out((size_t)width * height * 3);
    if (rt_denoise_frame(device, color, albedo, normal, depth, width, height, &params, out.data()) != RT_OK) throw Error(rt_last_error());
    return out;
}

} // namespace rtow_api
