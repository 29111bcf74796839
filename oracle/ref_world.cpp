/*
 * ref_world.cpp -- the reference's own classes, compiled for the host (test infrastructure, built only where the reference
 * checkout is present: `make -C oracle ref` -> oracle/_ref/libref_world.so, git-ignored).
 *
 * Everything numerical below is the reference's code, included from $(REF) (R/ = RayTracinginOneWeekend/) at build time:
 * Hittable::Hit of every class, Material::Scatter and Emitted, the textures and Perlin, Camera::GetRay, BvhNode's construction
 * and walk.  This file copies none of their lines; it only constructs their objects, one exported call per reference
 * constructor (the calls mirror oracle_c_* of rtow_oracle.c, handles 1-based per table, 0 = refused), and runs batches of
 * rays through world->Hit.  oracle/ref_shim/ stands in for the two CUDA headers: the qualifiers as empty macros, and XORWOW
 * with cuRAND's seeding (tests/test_rng.py pins that generator to rocRAND's engine).
 *
 * Build with clang++, -O2 -ffp-contract=off -fno-fast-math: R/Material.h:19-21, R/Camera.h:15 and R/Perlin.h draw their
 * random numbers as constructor arguments, whose order of evaluation the language leaves open; clang takes them left to
 * right, as the device compilers do, g++ right to left.
 *
 * Objects live until the process ends: the reference's destructors delete their children (R/Instance.h:39,114,
 * R/ConstantMedium.h:46-50), handles may share children, and a test process is short.
 */
#include <cfloat>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

#include "Vec3.h"
#include "Ray.h"
#include "Interval.h"
#include "AABB.h"
#include "Hittable.h"
#include "Perlin.h"
#include "Texture.h"
#include "Material.h"
#include "Metal.h"
#include "Dielectric.h"
#include "Sphere.h"
#include "MovingSphere.h"
#include "Quad.h"
#include "HittableList.h"
#include "Instance.h"
#include "BvhNode.h"
#include "ConstantMedium.h"
#include "Camera.h"

#define REF_API extern "C" __attribute__((visibility("default")))

namespace {

enum { KIND_LAMBERTIAN = 0, KIND_METAL = 1, KIND_DIELECTRIC = 2, KIND_LIGHT = 3, KIND_ISOTROPIC = 4 };   /* rt_query_hits.material */

struct RefScene {
    std::vector<Texture*> tex;
    std::vector<bool> texNoise;          /* the texture reaches a NoiseTexture */
    std::vector<Material*> mat;
    std::vector<bool> matNoise;
    std::vector<Hittable*> hit;
    bool mediumNoise = false;            /* some ConstantMedium's phase function reaches a NoiseTexture */
    Hittable* world = nullptr;
    Camera* camera = nullptr;
};

Texture* Tex(RefScene* c, int h) { return (h >= 1 && h <= (int)c->tex.size()) ? c->tex[h - 1] : nullptr; }
Material* Mat(RefScene* c, int h) { return (h >= 1 && h <= (int)c->mat.size()) ? c->mat[h - 1] : nullptr; }
Hittable* Hit(RefScene* c, int h) { return (h >= 1 && h <= (int)c->hit.size()) ? c->hit[h - 1] : nullptr; }

int PushTex(RefScene* c, Texture* t, bool noise)
{
    c->tex.push_back(t);
    c->texNoise.push_back(noise);
    return (int)c->tex.size();
}
int PushMat(RefScene* c, Material* m, bool noise)
{
    c->mat.push_back(m);
    c->matNoise.push_back(noise);
    return (int)c->mat.size();
}
int PushHit(RefScene* c, Hittable* h)
{
    c->hit.push_back(h);
    return (int)c->hit.size();
}

Vector3 V3(const double* p) { return Vector3(p[0], p[1], p[2]); }
void Put3(double* out, const Vector3& v)
{
    out[0] = v.X();
    out[1] = v.Y();
    out[2] = v.Z();
}

/* The handle of a material of this scene; 0 for one made out of our sight (a ConstantMedium's own Isotropic). */
int MatHandle(const RefScene* c, const Material* m)
{
    for (size_t k = 0; k < c->mat.size(); k++)
        if (c->mat[k] == m) return (int)k + 1;
    return 0;
}
int MatKind(const Material* m)
{
    if (dynamic_cast<const Lambertian*>(m)) return KIND_LAMBERTIAN;
    if (dynamic_cast<const Metal*>(m)) return KIND_METAL;
    if (dynamic_cast<const Dielectric*>(m)) return KIND_DIELECTRIC;
    if (dynamic_cast<const DiffuseLight*>(m)) return KIND_LIGHT;
    if (dynamic_cast<const Isotropic*>(m)) return KIND_ISOTROPIC;
    return 255;
}
bool MatNoise(const RefScene* c, const Material* m)
{
    int h = MatHandle(c, m);
    return h ? c->matNoise[h - 1] : c->mediumNoise;
}

curandState LoadStream(const uint32_t* w)
{
    curandState s;
    s.d = w[0];
    std::memcpy(s.v, w + 1, sizeof s.v);
    return s;
}
void StoreStream(uint32_t* w, const curandState& s)
{
    w[0] = s.d;
    std::memcpy(w + 1, s.v, sizeof s.v);
}
bool SameStream(const curandState& a, const curandState& b) { return a.d == b.d && std::memcmp(a.v, b.v, sizeof a.v) == 0; }

}  // namespace

REF_API RefScene* ref_new(void) { return new RefScene(); }
REF_API void ref_free(RefScene* c) { delete c; }   /* the handle tables only; see the note on lifetimes above */

/* ---- curand_init + curand_uniform of the shim, for scene generation and for the tests of the shim itself ---- */
REF_API curandState* ref_rng_new(uint64_t seed, uint64_t sequence)
{
    curandState* s = new curandState;
    curand_init(seed, sequence, 0, s);
    return s;
}
REF_API void ref_rng_free(curandState* s) { delete s; }
REF_API float ref_rng_uniform(curandState* s) { return curand_uniform(s); }
REF_API void ref_rng_state(const curandState* s, uint32_t out[6]) { StoreStream(out, *s); }

/* ---- textures (R/Texture.h) ---- */
REF_API int ref_c_solid(RefScene* c, double r, double g, double b) { return PushTex(c, new SolidColor(Color(r, g, b)), false); }
REF_API int ref_c_checker(RefScene* c, double scale, int even, int odd)
{
    if (!Tex(c, even) || !Tex(c, odd)) return 0;
    return PushTex(c, new CheckerTexture(scale, Tex(c, even), Tex(c, odd)), c->texNoise[even - 1] || c->texNoise[odd - 1]);
}
REF_API int ref_c_image(RefScene* c, const unsigned char* rgb, int w, int h)
{
    unsigned char* copy = nullptr;
    if (rgb && w > 0 && h > 0) {
        copy = new unsigned char[(size_t)w * h * 3];
        std::memcpy(copy, rgb, (size_t)w * h * 3);
    }
    return PushTex(c, new ImageTexture(copy, copy ? w : 0, copy ? h : 0), false);
}
REF_API int ref_c_noise(RefScene* c, double scale, curandState* rng) { return PushTex(c, new NoiseTexture(scale, rng), true); }

/* ---- materials (R/Material.h, R/Metal.h, R/Dielectric.h) ---- */
REF_API int ref_c_lambertian_tex(RefScene* c, int t) { return Tex(c, t) ? PushMat(c, new Lambertian(Tex(c, t)), c->texNoise[t - 1]) : 0; }
REF_API int ref_c_lambertian(RefScene* c, double r, double g, double b) { return PushMat(c, new Lambertian(Color(r, g, b)), false); }
REF_API int ref_c_metal(RefScene* c, double r, double g, double b, double fuzz) { return PushMat(c, new Metal(Color(r, g, b), fuzz), false); }
REF_API int ref_c_dielectric(RefScene* c, double ior) { return PushMat(c, new Dielectric(ior), false); }
REF_API int ref_c_light_tex(RefScene* c, int t) { return Tex(c, t) ? PushMat(c, new DiffuseLight(Tex(c, t)), c->texNoise[t - 1]) : 0; }
REF_API int ref_c_light(RefScene* c, double r, double g, double b) { return PushMat(c, new DiffuseLight(Color(r, g, b)), false); }
REF_API int ref_c_isotropic_tex(RefScene* c, int t) { return Tex(c, t) ? PushMat(c, new Isotropic(Tex(c, t)), c->texNoise[t - 1]) : 0; }
REF_API int ref_c_isotropic(RefScene* c, double r, double g, double b) { return PushMat(c, new Isotropic(Color(r, g, b)), false); }

/* ---- hittables ---- */
REF_API int ref_c_sphere(RefScene* c, double x, double y, double z, double r, int m)
{
    return Mat(c, m) ? PushHit(c, new Sphere(Point3(x, y, z), r, Mat(c, m))) : 0;
}
REF_API int ref_c_moving_sphere(RefScene* c, double x0, double y0, double z0, double x1, double y1, double z1, double t0, double t1,
                                double r, int m)
{
    return Mat(c, m) ? PushHit(c, new MovingSphere(Point3(x0, y0, z0), Point3(x1, y1, z1), t0, t1, r, Mat(c, m))) : 0;
}
REF_API int ref_c_quad(RefScene* c, const double q[3], const double u[3], const double v[3], int m)
{
    return Mat(c, m) ? PushHit(c, new Quad(V3(q), V3(u), V3(v), Mat(c, m))) : 0;
}
REF_API int ref_c_translate(RefScene* c, int h, double x, double y, double z)
{
    return Hit(c, h) ? PushHit(c, new Translate(Hit(c, h), Vector3(x, y, z))) : 0;
}
REF_API int ref_c_rotate_y(RefScene* c, int h, double degrees) { return Hit(c, h) ? PushHit(c, new RotateY(Hit(c, h), degrees)) : 0; }
REF_API int ref_c_make_box(RefScene* c, const double a[3], const double b[3], int m)
{
    return Mat(c, m) ? PushHit(c, MakeBox(V3(a), V3(b), Mat(c, m))) : 0;
}
REF_API int ref_c_list(RefScene* c, const int* items, int n)
{
    Hittable** list = new Hittable*[n > 0 ? n : 1];
    for (int k = 0; k < n; k++)
        if (!(list[k] = Hit(c, items[k]))) return 0;
    return PushHit(c, new HittableList(list, n));
}
/* BvhNode(list, 0, n, storage, &count): sorts list[] in place (R/BvhNode.h:180-193); items[] comes back in that order */
REF_API int ref_c_bvh(RefScene* c, int* items, int n)
{
    if (n <= 0) return 0;
    Hittable** list = new Hittable*[n];
    for (int k = 0; k < n; k++)
        if (!(list[k] = Hit(c, items[k]))) return 0;
    Hittable** storage = new Hittable*[2 * (size_t)n + 2];
    int count = 0;
    BvhNode* root = new BvhNode(list, 0, n, storage, &count);
    for (int k = 0; k < n; k++)
        for (size_t h = 0; h < c->hit.size(); h++)
            if (c->hit[h] == list[k]) {
                items[k] = (int)h + 1;
                break;
            }
    return PushHit(c, root);
}
REF_API int ref_c_medium(RefScene* c, int boundary, double density, double r, double g, double b)
{
    return Hit(c, boundary) ? PushHit(c, new ConstantMedium(Hit(c, boundary), density, Color(r, g, b))) : 0;
}
REF_API int ref_c_medium_tex(RefScene* c, int boundary, double density, int t)
{
    if (!Hit(c, boundary) || !Tex(c, t)) return 0;
    c->mediumNoise = c->mediumNoise || c->texNoise[t - 1];
    return PushHit(c, new ConstantMedium(Hit(c, boundary), density, Tex(c, t)));
}
REF_API int ref_c_bounding_box(RefScene* c, int h, double out[6])
{
    if (!Hit(c, h)) return -1;
    Aabb box = Hit(c, h)->BoundingBox();
    out[0] = box.X.Min, out[1] = box.X.Max, out[2] = box.Y.Min, out[3] = box.Y.Max, out[4] = box.Z.Min, out[5] = box.Z.Max;
    return 0;
}
REF_API int ref_c_set_world(RefScene* c, int h)
{
    if (!Hit(c, h)) return -1;
    c->world = Hit(c, h);
    return 0;
}
REF_API int ref_c_set_camera(RefScene* c, const double from[3], const double at[3], const double vup[3], double vfov, double aspect,
                             double aperture, double focus, double t0, double t1, const double bg[3])
{
    c->camera = new Camera(V3(from), V3(at), V3(vup), vfov, aspect, aperture, focus, t0, t1, V3(bg));
    return 0;
}

/* ---- batches ---- */

/* world->Hit(Ray(origin, direction, time), tmin, tmax, rec, &stream) for n rays.  streams: n x 6 words, read and written back.
 * Outputs (any may be NULL): hit n, t n, p n x 3, normal n x 3, uv n x 2, front n, material n (handle, 0 = a medium's own
 * phase function), kind n (0..4 as rt_query_hits.material, 255 for a miss).  A miss leaves zeros. */
REF_API int ref_hit(RefScene* c, int n, const double* origin, const double* direction, const double* time, const double* tmin,
                    const double* tmax, uint32_t* streams, uint8_t* hit, double* t, double* p, double* normal, double* uv,
                    uint8_t* front, int32_t* material, uint8_t* kind)
{
    if (!c->world) return -1;
    for (int k = 0; k < n; k++) {
        curandState s = LoadStream(streams + 6 * k);
        Ray ray(V3(origin + 3 * k), V3(direction + 3 * k), time[k]);
        HitRecord rec = HitRecord();
        bool found = c->world->Hit(ray, tmin[k], tmax[k], rec, &s);
        if (!found) rec = HitRecord();   /* a test that fails late may have written part of it */
        /* ConstantMedium::Hit sets no U, V (R/ConstantMedium.h:86-91): what the record holds there is whatever a caller's
         * uninitialised HitRecord held (R/HittableList.h:42), so it is reported as the (0, 0) rt_query_hits documents */
        if (found && MatHandle(c, rec.MaterialPtr) == 0) rec.U = rec.V = 0.0;
        StoreStream(streams + 6 * k, s);
        if (hit) hit[k] = found;
        if (t) t[k] = rec.T;
        if (p) Put3(p + 3 * k, rec.P);
        if (normal) Put3(normal + 3 * k, rec.Normal);
        if (uv) uv[2 * k] = rec.U, uv[2 * k + 1] = rec.V;
        if (front) front[k] = rec.bFrontFace;
        if (material) material[k] = found ? MatHandle(c, rec.MaterialPtr) : 0;
        if (kind) kind[k] = found ? (uint8_t)MatKind(rec.MaterialPtr) : 255;
    }
    return 0;
}

/* One iteration of RayColor's loop per ray, every call of it the reference's: world->Hit over RayColor's window
 * (0.001, DBL_MAX), then Emitted and Scatter on the record.  The arrangement of the outputs is rt_scene_path_step's
 * (include/rtow.h): status 0 miss, 1 the path ends here, 2 scattered; emitted is the background for a miss; attenuation is
 * zero and the ray that goes out is the ray that came in where status is not 2.  flags: bit 0 the search drew from the stream
 * or ended inside a medium, bit 1 the material at the hit reaches a NoiseTexture. */
REF_API int ref_step(RefScene* c, int n, const double* origin, const double* direction, const double* time, uint32_t* streams,
                     uint8_t* status, double* emitted, double* attenuation, double* out_origin, double* out_direction,
                     double* out_time, double* t, uint8_t* front, uint8_t* kind, uint8_t* flags)
{
    if (!c->world || !c->camera) return -1;
    for (int k = 0; k < n; k++) {
        curandState s = LoadStream(streams + 6 * k);
        const curandState before = s;
        Ray ray(V3(origin + 3 * k), V3(direction + 3 * k), time[k]);
        HitRecord rec;
        Color emit(0.0, 0.0, 0.0), atten(0.0, 0.0, 0.0);
        Ray next = ray;
        int st = 0, f = 0, hitKind = 255;
        double hitT = INFINITY;
        bool face = false;
        if (!c->world->Hit(ray, 0.001, DBL_MAX, rec, &s)) {
            emit = c->camera->Background();
            if (!SameStream(before, s)) f |= 1;
        } else {
            hitKind = MatKind(rec.MaterialPtr);
            if (!SameStream(before, s) || MatHandle(c, rec.MaterialPtr) == 0) f |= 1;
            if (MatNoise(c, rec.MaterialPtr)) f |= 2;
            hitT = rec.T;
            face = rec.bFrontFace;
            emit = rec.MaterialPtr->Emitted(rec.U, rec.V, rec.P);
            Ray scattered;
            Color a;
            if (rec.MaterialPtr->Scatter(ray, rec, a, scattered, &s)) {
                st = 2;
                atten = a;
                next = scattered;
            } else {
                st = 1;
            }
        }
        StoreStream(streams + 6 * k, s);
        if (status) status[k] = (uint8_t)st;
        if (emitted) Put3(emitted + 3 * k, emit);
        if (attenuation) Put3(attenuation + 3 * k, atten);
        if (out_origin) Put3(out_origin + 3 * k, next.Origin());
        if (out_direction) Put3(out_direction + 3 * k, next.Direction());
        if (out_time) out_time[k] = next.Time();
        if (t) t[k] = hitT;
        if (front) front[k] = face;
        if (kind) kind[k] = (uint8_t)hitKind;
        if (flags) flags[k] = (uint8_t)f;
    }
    return 0;
}

/* RESTATED, not included: the reference's RayColor (R/kernel.cu:65-98) and the pixel loop of its Render kernel
 * (R/kernel.cu:122-160) sit in a translation unit that cannot be compiled here (kernel launches, cudaMalloc, device new of
 * the whole world), so these two functions say again in our words what those lines do; every call inside them -- Hit, Emitted,
 * Scatter, GetRay, curand_init, curand_uniform, the Vector3 operators -- is the reference's own code or the shim's. */
static Color RestatedRayColor(const Ray& first, const Color& background, Hittable* world, curandState* s)
{
    Ray current = first;
    Color throughput(1.0, 1.0, 1.0), accumulated(0.0, 0.0, 0.0);
    for (int bounce = 0; bounce < 50; bounce++) {
        HitRecord rec;
        if (!world->Hit(current, 0.001, DBL_MAX, rec, s)) {
            accumulated += throughput * background;
            return accumulated;
        }
        accumulated += throughput * rec.MaterialPtr->Emitted(rec.U, rec.V, rec.P);
        Ray scattered;
        Color attenuation;
        if (!rec.MaterialPtr->Scatter(current, rec, attenuation, scattered, s)) return accumulated;
        throughput = throughput * attenuation;
        current = scattered;
    }
    return accumulated;
}

/* frame: height x width x 3, row j = 0 first, as the kernel's frameBuffer[j * maxX + i] */
REF_API int ref_render(RefScene* c, int width, int height, int samples, uint64_t seed, double* frame)
{
    if (!c->world || !c->camera) return -1;
    for (int j = 0; j < height; j++)
        for (int i = 0; i < width; i++) {
            int pixel = j * width + i;
            curandState s;
            curand_init(seed, pixel, 0, &s);
            Color col(0.0, 0.0, 0.0);
            Color background = c->camera->Background();
            for (int k = 0; k < samples; k++) {
                double u = double(i + curand_uniform(&s)) / double(width);    /* int + float: a float sum, as there */
                double v = double(j + curand_uniform(&s)) / double(height);
                Ray r = c->camera->GetRay(u, v, &s);
                col += RestatedRayColor(r, background, c->world, &s);
            }
            col = col / double(samples);
            frame[3 * pixel + 0] = sqrt(col[0]);
            frame[3 * pixel + 1] = sqrt(col[1]);
            frame[3 * pixel + 2] = sqrt(col[2]);
        }
    return 0;
}
