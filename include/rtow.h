/*
 * rtow.h -- C-ABI of the MI355X-native path tracer (librtow_hip.so).
 *
 * The reference (eazuooz/RayTracinginOneWeekendinCUDA) has no FFI layer; its hot path sits behind two
 * internal C++ interfaces.  This header is the drop-in boundary for both:
 *
 *   1. the CONSTRUCTION API that CreateWorld calls (R/kernel.cu:176-543): one extern "C" function per
 *      reference constructor, same parameter order and meaning, returning a handle instead of a
 *      device pointer;
 *   2. the RENDER API that main() calls (R/kernel.cu:570-742): RenderInit + Render launches, the
 *      framebuffer hand-back and the PPM writer.
 *
 * R/ = /root/reference/RayTracinginOneWeekend/.  Plain pointers and sizes only; no C++ or torch types.
 * Every function returning int returns 0 on success and a non-zero rt_status otherwise; functions
 * returning rt_handle return 0 on error.  rt_last_error() gives the message of the calling thread's
 * last failure.  A scene is thread-compatible (one thread at a time), not thread-safe.
 */
#ifndef RTOW_H
#define RTOW_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RTOW_API __attribute__((visibility("default")))

typedef uint32_t rt_handle;             /* 0 = invalid */
typedef struct rt_scene rt_scene;       /* owns every object built through it (host arena + device tables) */
typedef struct rt_rng rt_rng;           /* host-side curandState replacement for scene generation */
typedef struct rt_film rt_film;         /* framebuffer + per-pixel RNG state on one GPU */

enum rt_status {
    RT_OK = 0,
    RT_ERR_INVALID = 1,        /* bad argument / handle */
    RT_ERR_UNSUPPORTED = 2,    /* object nesting the flattener cannot normalise */
    RT_ERR_HIP = 3,            /* a HIP call failed (message carries the hipError_t) */
    RT_ERR_NO_DEVICE = 4,      /* no usable gfx950 device */
    RT_ERR_STATE = 5           /* call order violated (e.g. render before commit) */
};

RTOW_API const char *rt_last_error(void);
RTOW_API const char *rt_version(void);

/* ---- RNG: curand_init(seed, sequence, 0) / curand_uniform (R/kernel.cu:101-107, RND macro :157) ---- */
RTOW_API rt_rng *rt_rng_create(uint64_t seed, uint64_t sequence);
RTOW_API void rt_rng_destroy(rt_rng *rng);
RTOW_API float rt_rng_uniform(rt_rng *rng);                       /* float in (0,1] */
RTOW_API uint32_t rt_rng_next_u32(rt_rng *rng);
RTOW_API void rt_rng_state(const rt_rng *rng, uint32_t out6[6]);   /* {d, v0..v4} */
/* salt_kind 0 = cuRAND device-API seed salts (the product's RNG); 1 = rocRAND's salts (test cross-check only) */
RTOW_API rt_rng *rt_rng_create_salted(uint64_t seed, uint64_t sequence, int salt_kind);
/* a host stream that continues where a stream stood: {d, v0..v4} as rt_rng_state writes them, and as the films and the queries
 * save and return the device streams (NULL for a NULL argument) */
RTOW_API rt_rng *rt_rng_create_from_state(const uint32_t in6[6]);

/* ---- scene lifetime ---- */
RTOW_API rt_scene *rt_scene_create(void);
RTOW_API void rt_scene_destroy(rt_scene *scene);                   /* replaces FreeWorld, R/kernel.cu:548-568 */
/* Destroying a scene while launches of it are in flight is allowed: the call first waits for every such launch (the
 * kernels read the scene's tables); the films stay valid and their rt_render_finish reports as usual. */
/* Options read by the next rt_scene_commit (tests and timing; none changes an image). */
#define RT_SCENE_PLAIN_QUADS 1u          /* every quad takes the general test of R/Quad.h:52-99 (default: quads along the coordinate
                                            axes drop the terms that are exact zeros; MakeBox boxes are tested as boxes) */
#define RT_SCENE_REFERENCE_TREE_ONLY 2u  /* do not build the library's own tree for primitive worlds: only the reference's */
RTOW_API int rt_scene_set_options(rt_scene *scene, uint32_t options);

/* ---- textures (R/Texture.h) ---- */
RTOW_API rt_handle rt_solid_color(rt_scene *s, double r, double g, double b);                 /* :38,:43 */
RTOW_API rt_handle rt_checker_texture(rt_scene *s, double scale, rt_handle even, rt_handle odd); /* :63 */
/* bytes are copied; w*h*3 RGB, row 0 = top (what RtwImage hands to ImageTexture, R/RtwImage.h:51-92). NULL data => cyan. */
RTOW_API rt_handle rt_image_texture(rt_scene *s, const unsigned char *rgb, int width, int height); /* :103 */
RTOW_API rt_handle rt_noise_texture(rt_scene *s, double scale, rt_rng *rng);                  /* :153; draws from rng */
/* What RtwImage::Load does to decoded 8-bit pixels before ImageTexture sees them (R/RtwImage.h:54,66-67,100-105 on top
 * of stbi_loadf's LDR->HDR step, R/external/stb_image.h:1869): out = FloatToByte((float)pow(in / 255.0f, 2.2f)).
 * For decoded pixels that come from elsewhere (another decoder's output differs from stb's by up to 3 in ~0.6 % of the bytes of
 * the reference's earthmap.jpg); rt_rtwimage_load below does the whole of RtwImage::Load.  in/out may alias. */
RTOW_API void rt_rtwimage_bytes(const unsigned char *decoded_srgb, size_t count, unsigned char *out);
/* RtwImage::Load itself (R/RtwImage.h:51-87 over stbi_loadf, R/StbImageImpl.cpp): read a JPEG file and return the width * height * 3
 * bytes the reference hands to ImageTexture (row 0 = top), bit for bit what the reference's stb_image build produces for a
 * sequential Huffman JPEG of 8-bit samples, grey or YCbCr / RGB, any sampling factors, with or without restart intervals
 * (csrc/jpeg_decode.cpp restates that decoder's inverse DCT, upsampling and colour conversion).  Progressive / arithmetic-coded /
 * 12-bit / CMYK files return RT_ERR_UNSUPPORTED -- ImageTexture(NULL) then renders the reference's cyan fallback.
 * rt_jpeg_decode: the 8-bit sRGB pixels only (stbi_load), without RtwImage's linearisation.  Free the result with rt_image_free. */
RTOW_API int rt_rtwimage_load(const char *path, unsigned char **rgb_out, int *width, int *height);
RTOW_API int rt_jpeg_decode(const unsigned char *data, size_t size, unsigned char **rgb_out, int *width, int *height);
RTOW_API void rt_image_free(unsigned char *rgb);

/* ---- materials (R/Material.h, R/Metal.h, R/Dielectric.h) ---- */
RTOW_API rt_handle rt_lambertian(rt_scene *s, double r, double g, double b);                  /* Material.h:57 */
RTOW_API rt_handle rt_lambertian_tex(rt_scene *s, rt_handle texture);                         /* Material.h:63 */
RTOW_API rt_handle rt_metal(rt_scene *s, double r, double g, double b, double fuzz);          /* Metal.h:12 */
RTOW_API rt_handle rt_dielectric(rt_scene *s, double refraction_index);                       /* Dielectric.h:13 */
RTOW_API rt_handle rt_diffuse_light(rt_scene *s, double r, double g, double b);               /* Material.h:109 */
RTOW_API rt_handle rt_diffuse_light_tex(rt_scene *s, rt_handle texture);                      /* Material.h:103 */
RTOW_API rt_handle rt_isotropic(rt_scene *s, double r, double g, double b);                   /* Material.h:142 */
RTOW_API rt_handle rt_isotropic_tex(rt_scene *s, rt_handle texture);                          /* Material.h:147 */

/* ---- hittables ---- */
RTOW_API rt_handle rt_sphere(rt_scene *s, double cx, double cy, double cz, double radius, rt_handle material); /* Sphere.h:12 */
RTOW_API rt_handle rt_moving_sphere(rt_scene *s, double c0x, double c0y, double c0z, double c1x, double c1y,
                                    double c1z, double time0, double time1, double radius,
                                    rt_handle material);                                       /* MovingSphere.h:19 */
RTOW_API rt_handle rt_quad(rt_scene *s, const double q[3], const double u[3], const double v[3],
                           rt_handle material);                                                /* Quad.h:25 */
/* R/Quad.h's planar primitive with the interior rule its own comment (:86-88) names: corners Q, Q+u, Q+v.
 *   constants   the quad's (Quad.h:33-36): n = u x v, normal = unit(n), D = normal . Q, w = n / (n . n)
 *   Hit         Quad.h:56-71 unchanged: denom = normal . dir, |denom| < 1e-8 rejects; t = (D - normal . origin) / denom,
 *               tmin <= t <= tmax (inclusive); alpha = w . (p x v), beta = w . (u x p) with p = ray(t) - Q
 *   interior    accept <=> 0 <= alpha && 0 <= beta && fl(alpha + beta) <= 1: inclusive like the quad's rule, one IEEE add of the
 *               two values the quad forms, a NaN rejects.  So a triangle is hit exactly where the quad (Q, u, v) is hit with such
 *               alpha, beta, with the same t bit for bit.  Neighbouring triangles of a mesh are decided each by its own rounded
 *               alpha, beta: the arithmetic promises no watertightness along shared edges (DESIGN.md section 5 has the count).
 *   HitRecord   U = alpha, V = beta (the barycentric coordinates of Q+u and Q+v); the normal is the flat geometric one, set
 *               against the ray (SetFaceNormal); corner normals and texture coordinates: rt_triangle_attr below
 *   degenerate  u x v = 0: normal and w are not finite and no ray is accepted, like a degenerate quad
 *   box         per axis the min and max of Q, fl(Q+u), fl(Q+v), through the corner constructor the quad uses (AABB.h:34-40) with
 *               its padding of axes thinner than 0.0001 (AABB.h:114-120)
 * Everywhere a quad may stand a triangle may: in lists and BvhNodes, under Translate / RotateY, as a ConstantMedium boundary.  It
 * is no box face: a list with a triangle in it is a list.  Returns 0 on an invalid material or a NULL vector. */
RTOW_API rt_handle rt_triangle(rt_scene *s, const double q[3], const double u[3], const double v[3],
                               rt_handle material);
/* Triangle k has corners A = vertices[indices[3k]], B = vertices[indices[3k+1]], C = vertices[indices[3k+2]] (vertices: 3 doubles
 * each) and is rt_triangle(A, fl(B - A), fl(C - A), material).  Returns rt_bvh_node over the n_triangles handles (the reference's
 * rule and permutation); triangles_out, if not NULL, receives the n_triangles handles in input order (for a list, or a BvhNode
 * shared with other objects).  Returns 0 where n_triangles < 1, n_vertices < 3, an array is NULL, the material is invalid or an
 * index lies outside [0, n_vertices); nothing is added to the scene then. */
RTOW_API rt_handle rt_triangle_mesh(rt_scene *s, const double *vertices, int n_vertices, const int32_t *indices,
                                    int n_triangles, rt_handle material, rt_handle *triangles_out);
/* Wavefront OBJ, positions and faces only: `v x y z`, `f` with i, i/j, i/j/k and i//k forms, negative (relative) indices,
 * polygons fanned from their first corner (0 1 2, 0 2 3, ...), comments and every other statement skipped.  Indices come back
 * 0-based.  The arrays are the library's: release them with rt_mesh_free.  RT_ERR_INVALID for an unreadable file, a file without
 * a face, an index out of range (0 included), a vertex with fewer than three numbers or a face with fewer than three corners. */
RTOW_API int rt_obj_load(const char *path, double **vertices, int *n_vertices, int32_t **indices, int *n_triangles);
RTOW_API void rt_mesh_free(double *vertices, int32_t *indices);
/* Corner attributes: a triangle may carry three corner normals n0, n1, n2 (normals: 9 doubles, or NULL) and / or three corner
 * texture coordinates t0, t1, t2 (texcoords: 6 doubles u0 v0 u1 v1 u2 v2, or NULL).  Corner 0 is Q, corner 1 is Q+u, corner 2 is Q+v.
 * With both NULL the call is rt_triangle exactly.
 *   Hit         unchanged: t, the interior rule, the box, the leaf, the ties and front_face = dot(dir, ng) < 0 are rt_triangle's,
 *               where ng is the row's geometric unit normal (`normal` above).  Only the hit record differs.
 *   HitRecord   in the space the hit was found in (below any Translate / RotateY), each line one IEEE double operation per
 *               arithmetic sign, nothing contracted in the strict build:
 *                 p = ray(t), ph = p - Q
 *                 alpha = dot(w, cross(ph, v)), beta = dot(w, cross(u, ph))     (the U, V of rt_triangle)
 *                 gamma = (1.0 - alpha) - beta
 *               with normals, per component:
 *                 m  = (gamma * n0 + alpha * n1) + beta * n2
 *                 ns = unit(m) = (1 / sqrt(length_sq(m))) * m,  length_sq(m) = m.x*m.x + m.y*m.y + m.z*m.z
 *                 ns = ng  where length_sq(m) is not a finite positive number or dot(ns, ng) <= 0: a shading normal never points
 *                          under the geometric surface
 *                 Normal = front_face ? ns : -ns, then back through the instance chain as the flat normal goes
 *               with texture coordinates:
 *                 U = (gamma * t0.u + alpha * t1.u) + beta * t2.u,  V = (gamma * t0.v + alpha * t1.v) + beta * t2.v
 *               without them U = alpha, V = beta.  Render and shading kernels compute U, V only for materials that read them
 *               (an ImageTexture in the texture tree), ray queries whenever they are asked for.
 *   scatter     materials see only Normal: a direction scattered about ns may point below the geometric surface and is accepted
 *               as it is (a Lambertian's ns + unit vector, a metal's reflection about ns near a silhouette).
 *   refused     (returns 0, nothing added, rt_last_error says why) a corner normal with a non-finite component or all zero -- they
 *               are otherwise taken as given, not normalised; a non-finite texture coordinate; texture coordinates on an emissive
 *               (DiffuseLight) material: the light table evaluates emission at the barycentric U, V.  An emissive triangle with
 *               normals only is accepted (Emitted reads U, V and P, never the normal); its light row is the flat triangle's. */
RTOW_API rt_handle rt_triangle_attr(rt_scene *s, const double q[3], const double u[3], const double v[3], const double *normals,
                                    const double *texcoords, rt_handle material);
/* rt_triangle_mesh with attribute arrays: normals (3 doubles each, n_normals of them) indexed by normal_indices, texcoords
 * (2 doubles each, n_texcoords of them) indexed by texcoord_indices, three indices a triangle like `indices`.  An index array that
 * is NULL means "use indices"; an attribute array that is NULL means the mesh has none of that kind, and with both NULL the call is
 * rt_triangle_mesh exactly.  Triangle k is rt_triangle_attr of its corners' entries.  Every index and every triangle's attributes
 * are checked before the first triangle is added: on a refusal (rt_triangle_mesh's, rt_triangle_attr's, an attribute index outside
 * its array) nothing is added. */
RTOW_API rt_handle rt_triangle_mesh_attr(rt_scene *s, const double *vertices, int n_vertices, const int32_t *indices,
                                         int n_triangles, const double *normals, int n_normals, const int32_t *normal_indices,
                                         const double *texcoords, int n_texcoords, const int32_t *texcoord_indices,
                                         rt_handle material, rt_handle *triangles_out);
/* rt_obj_load that also reads `vn x y z`, `vt u v [w]` and the j (vt) and k (vn) of the face forms i/j, i/j/k, i//k.  A negative
 * index is relative to the count of its own kind so far; polygons are fanned as by rt_obj_load.  normals / normal_indices come
 * back only if every corner of every face names a normal, else NULL with n_normals = 0; the same, separately, for texcoords.
 * The index arrays hold 3 * n_triangles 0-based entries.  RT_ERR_INVALID as for rt_obj_load (file and line in the message), and
 * for a vn with fewer than three numbers, a vt with fewer than two, and a j or k that is 0 or out of range.  The arrays are the
 * library's: release them with rt_obj_mesh_free, which also clears the struct. */
typedef struct rt_obj_mesh {
    double *vertices, *normals, *texcoords;
    int32_t *indices, *normal_indices, *texcoord_indices;
    int n_vertices, n_normals, n_texcoords, n_triangles;
} rt_obj_mesh;
RTOW_API int rt_obj_load_attr(const char *path, rt_obj_mesh *out);
RTOW_API void rt_obj_mesh_free(rt_obj_mesh *mesh);
RTOW_API rt_handle rt_translate(rt_scene *s, rt_handle object, double ox, double oy, double oz); /* Instance.h:31 */
RTOW_API rt_handle rt_rotate_y(rt_scene *s, rt_handle object, double angle_degrees);          /* Instance.h:74 */
/* A general affine instance: the child placed by x_world = L x_obj + t.  m is row-major 3x4: L[r][c] = m[4 r + c], t[r] = m[4 r + 3].
 * The reference has no such class; it stands wherever Translate / RotateY may stand -- in chains of any length and order, above
 * lists, BvhNodes, meshes, boxes, media, and in the general object tree -- and is stated here operation by operation, each operation
 * one IEEE double operation, nothing contracted in the strict build:
 *   creation    Li, the inverse of L, is computed once, in fp64, from cofactors over the determinant:
 *                 c00 = (L11*L22) - (L12*L21)   c01 = (L12*L20) - (L10*L22)   c02 = (L10*L21) - (L11*L20)
 *                 c10 = (L02*L21) - (L01*L22)   c11 = (L00*L22) - (L02*L20)   c12 = (L01*L20) - (L00*L21)
 *                 c20 = (L01*L12) - (L02*L11)   c21 = (L02*L10) - (L00*L12)   c22 = (L00*L11) - (L01*L10)
 *                 det = ((L00*c00) + (L01*c01)) + (L02*c02)
 *                 Li[r][c] = c[c][r] / det      (the transposed cofactor over det, one division an entry)
 *               L, t and Li are stored, uploaded and used exactly as rt_transform_get returns them.
 *   refused     (returns 0, nothing added, rt_last_error says why) an invalid handle or NULL m; a non-finite entry of m; a det that
 *               is zero or non-finite; a non-finite entry of Li; a child subtree that holds an emissive (DiffuseLight) Sphere or
 *               MovingSphere outside any ConstantMedium boundary -- under a general map such a lamp is an ellipsoid, which the light
 *               table cannot hold.  Mirrors (det < 0) are accepted.
 *   Hit         the local ray: p = o - t, then per row r
 *                 o'[r] = ((Li[r][0]*p.x) + (Li[r][1]*p.y)) + (Li[r][2]*p.z)      d'[r] the same from d
 *               The time is unchanged and d' is NOT normalised: the child's Hit is called with the caller's interval and its t is
 *               the world's t, as under RotateY.
 *   HitRecord   P[r] = (((L[r][0]*P'.x) + (L[r][1]*P'.y)) + (L[r][2]*P'.z)) + t[r]
 *               n[c] = ((Li[0][c]*n'.x) + (Li[1][c]*n'.y)) + (Li[2][c]*n'.z)
 *               Normal = (1 / sqrt(length_sq(n))) * n,  length_sq(n) = n.x*n.x + n.y*n.y + n.z*n.z
 *               renormalised at every Transform step of a chain; Translate and RotateY steps stay exactly as they are.  front_face,
 *               U, V, the material and the leaf are the child's.  A shading normal from corner attributes (rt_triangle_attr) goes
 *               the same way as the flat normal.
 *   box         the eight corners of the child's box (x outermost, then y, then z; lo before hi) go forward as P does; per axis
 *               their fmin / fmax, then the corner constructor with its padding (AABB.h:34-40), as rt_rotate_y does.
 *   media       a ConstantMedium UNDER a Transform measures its path in object space (length(d') of the local ray): a fog scaled by
 *               2 is as opaque across its width as before.  A ConstantMedium whose BOUNDARY is a Transform measures in the space the
 *               medium itself is called in.
 *   lights      an emissive quad or triangle under a Transform is listed in the light table: see rt_scene_dump_lights. */
RTOW_API rt_handle rt_transform(rt_scene *s, rt_handle object, const double m[12]);
/* The three convenience constructors fill the twelve numbers and call rt_transform.  Angles are converted as rt_rotate_y converts
 * them: radians = angle_degrees * 3.1415926535897932385 / 180.0, s = std::sin(radians), c = std::cos(radians); every t is 0.
 *   rt_rotate_x   L = 1 0 0 / 0 c -s / 0 s c     (+sin in L[2][1], -sin in L[1][2])
 *   rt_rotate_z   L = c -s 0 / s c 0 / 0 0 1     (+sin in L[1][0], -sin in L[0][1])
 *   rt_scale      L = sx 0 0 / 0 sy 0 / 0 0 sz   (a zero factor is refused as a zero determinant) */
RTOW_API rt_handle rt_rotate_x(rt_scene *s, rt_handle object, double angle_degrees);
RTOW_API rt_handle rt_rotate_z(rt_scene *s, rt_handle object, double angle_degrees);
RTOW_API rt_handle rt_scale(rt_scene *s, rt_handle object, double sx, double sy, double sz);
/* L (9, row-major), t (3), Li (9, row-major) of a Transform exactly as stored and uploaded.  RT_ERR_INVALID: not a Transform. */
RTOW_API int rt_transform_get(rt_scene *s, rt_handle transform, double out21[21]);
/* A moving instance: rt_transform's matrix keyed at two times and interpolated ENTRY BY ENTRY per ray on the device, so that any
 * hittable -- a mesh, a box, a fog, a whole BvhNode -- moves during the shutter.  m0 = [L0 | t0] holds at time0, m1 = [L1 | t1] at
 * time1 (both row-major 3x4 as rt_transform's m).  It stands wherever an rt_transform may stand.  The reference has no such class;
 * each line below is one IEEE double operation, nothing contracted in the strict build:
 *   creation    dL[r][c] = L1[r][c] - L0[r][c]      dt[r] = t1[r] - t0[r]      dtime = time1 - time0
 *               L0, t0, dL, dt, time0, dtime are stored, uploaded and used exactly as rt_moving_transform_get returns them.
 *   per ray     of time tm:
 *                 s = (tm - time0) / dtime,  then  s = fmin(fmax(s, 0.0), 1.0)
 *                 L[r][c] = L0[r][c] + (s * dL[r][c])      t[r] = t0[r] + (s * dt[r])
 *                 Li from L by rt_transform's cofactor formula: the same nine cofactors, the same det, one division an entry,
 *                 computed on the device in that order.
 *               A time outside [time0, time1] sees the nearer key and a NaN time sees key 0 (fmax drops the NaN).  MovingSphere's
 *               unclamped rule is the reference's and stays; this class is the library's, and the clamp is what makes its box valid
 *               for every ray a query can send.
 *   Hit, HitRecord, media
 *               exactly rt_transform's lines with this ray's L, t, Li: the local ray is recomputed from the world ray, d' is not
 *               normalised, t is the world's, P = (L P') + t, the normal goes through Li^T and is renormalised.  A ConstantMedium
 *               under the step measures in object space, one whose boundary is the step measures where it is called.  The way back
 *               of the hit record forms L and Li again from the same tm, so it uses the same bits.
 *   box         the eight corners of the child's box (rt_transform's order) go forward with (L0, t0) and with the matrices of s = 1
 *               as the device forms them, L0 + (1.0 * dL) and t0 + (1.0 * dt); per axis fmin / fmax over the sixteen points; every
 *               bound is then widened outward by 16 * DBL_EPSILON * (the largest absolute coordinate among the sixteen) -- a point
 *               at an intermediate s is a convex combination of its two key positions only up to the seven roundings of (L p) + t,
 *               each at most half an ulp of a sum of three products bounded by that coordinate --; then the corner constructor with
 *               its padding, as rt_rotate_y.
 *   refused     (returns 0, nothing added, rt_last_error says why) whatever rt_transform refuses, for either key; time0 or time1
 *               non-finite, or time1 <= time0; a non-finite dL, dt or dtime; a matrix L(s) that is singular, or cannot be shown
 *               regular, somewhere in [0, 1] (below); a child subtree that holds ANY emissive primitive outside a ConstantMedium
 *               boundary: the light table is in world space and static, a moving lamp is out of scope.
 *   singular in between
 *               det(L(s)) is a cubic in s.  With rows a_i of L0 and b_i of L0 + (1.0 * dL) its Bernstein coefficients over [0, 1]
 *               are det(a0,a1,a2); a third of det(b0,a1,a2) + det(a0,b1,a2) + det(a0,a1,b2); a third of det(b0,b1,a2) +
 *               det(b0,a1,b2) + det(a0,b1,b2); det(b0,b1,b2).  The step is accepted if all four have one strict sign; otherwise
 *               the interval is halved (de Casteljau) up to depth 8 and accepted only if every piece is proven so.  A coefficient
 *               counts as positive (negative) only beyond 2^-30 of the largest of the first four in absolute value, which covers
 *               the roundings of the halving.  Equal signs of the two key determinants are not enough: a half turn about Z,
 *               L1 = diag(-1, -1, 1), has det = (1 - 2s)^2.
 * Entry-wise interpolation is no rotation: keys that differ by a rotation through an angle theta shrink the object by cos(theta / 2)
 * at mid-shutter.  Key rotations in small angles, and split a long motion into several steps of consecutive time intervals. */
RTOW_API rt_handle rt_moving_transform(rt_scene *s, rt_handle object, const double m0[12], const double m1[12], double time0, double time1);
/* L = the identity at both keys, t = offset0 at time0 and offset1 at time1; calls rt_moving_transform. */
RTOW_API rt_handle rt_moving_translate(rt_scene *s, rt_handle object, const double offset0[3], const double offset1[3], double time0, double time1);
/* L0 (9, row-major), t0 (3), dL (9, row-major), dt (3), time0, dtime = time1 - time0 of a moving instance exactly as stored and
 * uploaded.  RT_ERR_INVALID: not such a handle. */
RTOW_API int rt_moving_transform_get(rt_scene *s, rt_handle h, double out26[26]);
RTOW_API rt_handle rt_make_box(rt_scene *s, const double a[3], const double b[3], rt_handle material); /* Instance.h:166 */
RTOW_API rt_handle rt_hittable_list(rt_scene *s, const rt_handle *objects, int count);        /* HittableList.h:21 */
RTOW_API rt_handle rt_constant_medium(rt_scene *s, rt_handle boundary, double density, double r, double g,
                                      double b);                                               /* ConstantMedium.h:39 */
RTOW_API rt_handle rt_constant_medium_tex(rt_scene *s, rt_handle boundary, double density,
                                          rt_handle texture);                                  /* ConstantMedium.h:32 */
/* BvhNode(objects, 0, count, ...): builds the tree with the reference's rule and PERMUTES objects[] in
 * place exactly as the reference's DeviceSort does (R/BvhNode.h:50-90,180-193). */
RTOW_API rt_handle rt_bvh_node(rt_scene *s, rt_handle *objects, int count);                   /* BvhNode.h:50 */
RTOW_API int rt_hittable_bounding_box(rt_scene *s, rt_handle object, double out_xyz_minmax[6]); /* Hittable.h:60 */

/* ---- world + camera (the two outputs of CreateWorld, R/kernel.cu:523-541) ---- */
RTOW_API int rt_scene_set_world(rt_scene *s, rt_handle world);      /* a BvhNode, a HittableList or any hittable */
RTOW_API int rt_scene_set_camera(rt_scene *s, const double lookfrom[3], const double lookat[3],
                                 const double vup[3], double vfov_degrees, double aspect, double aperture,
                                 double focus_dist, double time0, double time1,
                                 const double background[3]);                                  /* Camera.h:36-72 */

/* Built-in scenes: ids 0..9 = the reference's sceneId (R/kernel.cu:199-517); 10 = three-spheres (config C1);
 * 11 = scene 0 with every MovingSphere made static (config C2); 12 = scene 7's Cornell walls, light and camera with two triangle
 * meshes in place of the boxes (a 320-triangle Lambertian icosphere under Translate, a 20-triangle metal icosahedron under
 * RotateY + Translate; both rt_triangle_mesh); 13 = scene 12 with both meshes given corner normals unit(vertex position) in mesh
 * space (rt_triangle_mesh_attr) and nothing else changed; 14 = scene 7's walls, light and camera with four general affine
 * instances: scene 13's icosphere under one rt_transform (scale 1.1, 1.6, 0.8, then 25 degrees about Z, then a translation), a metal
 * MakeBox under rt_rotate_x + rt_translate, a glass unit Sphere under rt_scale + rt_translate (an ellipsoid), and a ConstantMedium
 * whose boundary is a unit MakeBox under rt_scale + rt_translate.  world_kind 0 = BvhNode world (the
 * reference's), 1 = HittableList world ("no BVH").  earth_rgb may be NULL (scenes 2 and 9 then show cyan). */
RTOW_API int rt_scene_build_builtin(rt_scene *s, int scene_id, int world_kind, int image_width,
                                    int image_height, uint64_t seed, const unsigned char *earth_rgb,
                                    int earth_w, int earth_h);
/* The environment's demonstration scene, `rtow --scene 15` (not an id of rt_scene_build_builtin, whose ids stay 0..14): the static
 * random spheres of scene 11 on their ground under a sky computed here -- a 256 x 128 linear float image with a vertical gradient
 * and a small, very bright sun disc (rt_scene_set_environment) -- with a black camera background, so that a miss that does not
 * reach the environment shows.  Builds, sets world, camera and environment, and commits, like rt_scene_build_builtin. */
RTOW_API int rt_scene_build_sky_demo(rt_scene *s, int world_kind, int image_width, int image_height, uint64_t seed);

/* Flatten the object graph into the SoA tables the kernel reads (host only; no GPU needed). */
RTOW_API int rt_scene_commit(rt_scene *s);

typedef struct rt_scene_info {
    uint32_t world_kind;          /* 0 bvh, 1 list */
    uint32_t n_leaves;            /* top-level leaves of the world */
    uint32_t n_nodes;             /* threaded BVH nodes */
    uint32_t n_spheres, n_moving_spheres, n_quads;
    uint32_t n_objects;           /* composite leaves (instances, boxes, media) */
    uint32_t n_xforms, n_media, n_materials, n_textures, n_perlin, n_images;
    uint32_t table_bytes;         /* bytes of the geometry tables staged on chip */
    uint32_t image_bytes;
    uint32_t reserved[3];         /* [0] = n_triangles: the rows of n_quads that are triangles; [1] = n_lights: the rows of the
                                     light table (rt_scene_dump_lights); [2] = n_attributed_triangles: the triangle rows that
                                     carry corner normals or texture coordinates (rt_triangle_attr) */
} rt_scene_info;
RTOW_API int rt_scene_get_info(rt_scene *s, rt_scene_info *out);
/* The committed scene's flags word as the kernels receive it (csrc/flat_scene.h SCENE_*), 0 before commit.  Introspection for
 * tests: a scene without an environment has the word it always had, one with an environment additionally this bit. */
#define RT_SCENE_FLAG_ENVIRONMENT 1024u
RTOW_API uint32_t rt_scene_flags(rt_scene *s);

/* Introspection for tests (valid after commit): world leaves in final order. kind: 0 sphere, 1 moving
 * sphere, 2 quad, 3 composite object, 4 triangle; box = {xmin,xmax,ymin,ymax,zmin,zmax}. Returns the leaf count. */
RTOW_API int rt_scene_dump_leaves(rt_scene *s, int max_leaves, int *kind_out, double *box_out);
/* Threaded-BVH nodes in preorder: box[6], a, b, escape per node (a,b = leaf refs or 0xE0000000 for inner). */
RTOW_API int rt_scene_dump_nodes(rt_scene *s, int max_nodes, double *box_out, uint32_t *abe_out);
/* The library's own tree for primitive-only BVH worlds (0 nodes if the world has none): box[6], a, b, and per direction
 * octant the {hit, escape} links (16 x uint16 per node, 0xFFFF = end). */
RTOW_API int rt_scene_dump_fast_nodes(rt_scene *s, int max_nodes, double *box_out, uint32_t *ab_out, uint16_t *link_out);
RTOW_API int rt_scene_dump_camera(rt_scene *s, double out27[27]);
/* The segments of the sphere-list scan over the scene's static spheres (0 segments without any), in list order: first row, row
 * count (whole trips of eight rows; the last may end in padding) and axis per segment -- 0 x, 1 y, 2 z: every row of the segment
 * that the fp32 filter decides has shared_out[k] as that centre coordinate, bit for bit, and the scan forms its terms once per ray;
 * 3: a general segment (shared_out[k] = 0).  The segments tile the rows exactly.  Host only.  Returns the segment count. */
RTOW_API int rt_scene_dump_scan_segments(rt_scene *s, int max_segments, uint32_t *rows_axis_out, float *shared_out);
/* The windows of those segments (csrc/scan_window_rule.h), tables beside them: per segment the window axis -- 0 x, 1 y, 2 z; 3: the
 * segment has no table and is scanned whole, as every general segment and every run whose trips are not selective is -- and the
 * slab {lo, hi} of the run's decided rows on the run's own axis; per trip of eight rows of the whole table the span {lo, hi} of its
 * decided rows on the window axis: (-inf, +inf) for a trip with a row the fp32 filter does not decide and outside the windowed runs,
 * (+inf, -inf) for a trip of padding alone.  A pixel-parallel pass runs, of a windowed run, the trips whose span meets the union of
 * its rays' extents inside the slab (gaps of one or two trips filled).  Host only.  Returns the segment count (negative: error);
 * writes min(segments, max_segments) records and min(trips, max_trips) spans where the arrays are given. */
RTOW_API int rt_scene_dump_scan_windows(rt_scene *s, int max_segments, uint32_t *axis_out, float *slab_out, int max_trips, float *spans_out);
/* The same rule for caller-supplied rays, one at a time, as the device evaluates it: needed_out[k * max_trips + t] = 1 where trip t
 * must run for ray k (origin and direction: n_rays x 3), 0 where the rule proves that the reference's Sphere::Hit accepts no decided
 * row of the trip over (0.001, inf).  Trips outside the windowed runs are always 1, entries from the table's trips on 0.  Host only.
 * Returns the table's trips (negative: error; max_trips must not be below them where needed_out is given). */
RTOW_API int rt_scene_scan_window_trips(rt_scene *s, int n_rays, const double *origin, const double *direction, int max_trips, uint8_t *needed_out);
/* The camera rays' candidate lists of a sphere-list world, as a launch on a film of this geometry builds them on the device (same
 * rule, csrc/primary_cull_rule.h): per 8x8 tile of the rank's rows, row-major over its compact rows, 16 uint16 -- [0] the number
 * of listed spheres, 0..14, or 15: too many, the tile has no list; [1..count] their positions in the sphere list, ascending.  A
 * list holds every sphere the reference's Sphere::Hit could accept over (0.001, inf) for any camera ray of any pixel of the tile.
 * Host only.  Returns the tile count (negative: error); writes min(tiles, max_tiles) lists where lists_out is given. */
RTOW_API int rt_scene_dump_primary_lists(rt_scene *s, int width, int height, int stripe_rows, int rank, int world_size, int max_tiles,
                                         uint16_t *lists_out);

/* The light table (valid after commit): one row per world primitive whose material is a DiffuseLight -- spheres, moving spheres,
 * quads, triangles (those of meshes included), the six faces of a MakeBox -- wherever it sits in the world: in lists, in BvhNodes,
 * under any chain of Translate / RotateY, in the general object tree.  Nothing that is, or lies inside, the boundary of a
 * ConstantMedium is listed.  The order is the depth-first order of the world as constructed: the world's leaves in
 * rt_scene_dump_leaves order, and below a leaf a list's members in list order, a BvhNode's in its sorted order.  Every row is in
 * WORLD space: the forward transforms of the chain above the primitive (innermost first; a RotateY turns points and vectors, x' =
 * (cos * x) + (sin * z), z' = (-sin * x) + (cos * z), a Translate adds its offset to points) are applied on the host, in fp64,
 * one IEEE operation at a time.  A Transform (rt_transform) takes points through (L p) + t, the vectors u, v and a moving sphere's
 * dc through L, and n through its normal rule (Li^T, renormalised), each in the row form stated there.  Where the chain above a quad
 * or triangle holds a Transform, s is the area of the TRANSFORMED primitive: |b x c| of the world-space row (half of it for a
 * triangle); without a Transform s is bit for bit what it always was.  (No sphere lamp stands under a Transform: rt_transform
 * refuses it.)
 *   kind 0 quad, 1 triangle   a = Q, b = u, c = v (corners Q, Q + u, Q + v [, Q + u + v]), n = the unit normal the primitive was
 *                             constructed with, turned through the chain; s = the area |u x v| (half of it for a triangle) of the
 *                             primitive as constructed
 *   kind 2 sphere             a = the centre, s = the radius
 *   kind 3 moving sphere      a = c0, b = dc = c1 - c0 (turned), c = (time0, time1 - time0, 0), s = the radius; the centre at time t
 *                             is a + ((t - c[0]) / c[1]) * b
 * mat = the row of the material table, leaf = the position of the world leaf the light belongs to (rt_query_hits.leaf).
 * cdf_out[2k + st] = the cumulative selection table of strategy st at light k: entry k = fl(fl(w_0 + ... + w_k) / fl(w_0 + ... +
 * w_{n-1})), summed in order, the last entry exactly 1.0.  Strategy 0: uniform, entry k = fl((k + 1) / n).  Strategy 1: w = the area
 * (4 pi r^2 for a sphere) x max(r, g, b) of a SolidColor emission texture, x 1 for any other texture; where those weights do not
 * sum to a finite positive number it is strategy 0's table.  Returns the number of lights (rt_scene_info.reserved[1]); writes
 * min(lights, max_lights) entries of each array given. */
typedef struct rt_light_row {
    double a[3], b[3], c[3], n[3], s;
    uint32_t kind, mat, leaf, pad0;
    double pad1;
} rt_light_row;                           /* 128 bytes, exactly as uploaded */
RTOW_API int rt_scene_dump_lights(rt_scene *s, int max_lights, int *kind_out, int *leaf_out, rt_light_row *rows_out, double *cdf_out);

/* ---- the environment: a textured sky at every miss ----
 * A scene without one gives a ray that leaves the world the camera's `background`, whatever its direction.  With one, such a ray
 * gets the environment's value along its direction, in every frame and every call on caller-supplied rays (renders, adaptive and
 * direct films, radiance queries, path steps, advances, and the albedo of a miss in the feature pass and in rt_scene_intersect);
 * the camera's background is then not read.  A construction call: it takes effect with the next rt_scene_commit (the scene counts
 * as not committed behind it, as behind rt_scene_set_world).  A scene without an environment commits to the flags, tables and
 * launch plans it always had; one with an environment is rendered by the instantiations that carry the texture code (the
 * general, deep, segmented and nested kernels: rt_plan_launch says which).
 *
 * The value for a ray of direction d (not necessarily unit), one IEEE fp64 operation at a time in the strict build:
 *   n = (1 / sqrt((d.x * d.x + d.y * d.y) + d.z * d.z)) * d
 *   e = R n, each row (r0 * n.x + r1 * n.y) + r2 * n.z                        (rotation: world -> environment)
 *   theta = acos(-e.y), phi = atan2(-e.z, e.x) + pi, u = phi / (2 pi), v = theta / pi          (the reference's GetSphereUV: the
 *       earth map used as a sky has its north pole at +y, exactly as it lies on the reference's globe)
 *   texture != 0:  value = intensity * texture_value(texture, u, v, e)   -- a checker or marble sky is a function of the direction
 *   rgb != NULL:   ImageTexture::Value's index rule (R/Texture.h:110-133): u and v clamped to [0, 1], v = 1 - v, i = int(u * width),
 *                  j = int(v * height), each clamped to the table; value = intensity * the three floats of texel (i, j) of row j
 *                  (top row first) widened to double
 * The float image is copied at the call; it is a table of its own, not a texture: no material can name it.
 *
 * Refused with RT_ERR_INVALID: a NULL scene; both or neither of texture and rgb; a texture handle that is none of this scene's;
 * with rgb, a width or height below 1 or a texel that is negative or not finite; an intensity that is negative or not finite; a
 * rotation with an entry that is not finite or with |R R^T - I| above 1e-9 in some entry.  RT_ERR_STATE while a render of the
 * scene is in flight.  env == NULL removes the environment: back to the camera's background. */
typedef struct rt_environment {
    rt_handle    texture;        /* a texture of this scene (solid, checker, noise, 8-bit image), or 0 */
    const float *rgb;            /* or: a linear float image, width x height x 3, top row first, copied; NULL with `texture` */
    int32_t      width, height;  /* of rgb */
    double       intensity[3];   /* multiplies the value per channel */
    double       rotation[9];    /* row-major R, world -> environment; must be orthonormal to 1e-9 */
    int32_t      reserved[4];
} rt_environment;
RTOW_API int rt_scene_set_environment(rt_scene *s, const rt_environment *env);
/* What was set: *out as given (rgb points at the scene's own copy, valid until the next rt_scene_set_environment or the scene's
 * end); without an environment *out is all zeros and the call returns RT_OK.  *has_distribution (may be NULL): 1 where the
 * committed scene holds the importance sampler's tables (below), else 0 -- before commit always 0. */
RTOW_API int rt_scene_get_environment(rt_scene *s, rt_environment *out, int *has_distribution);
/* The environment as a light of the direct estimators (rt_scene_path_advance_direct states what changes; nothing else does: plain
 * renders, launch plans, rt_scene_dump_lights and rt_scene_get_info of such a scene are what they were).  `chance` is the share of
 * the light samples that go to the environment where the scene also has lamps.  A construction call like
 * rt_scene_set_environment: it takes effect with the next rt_scene_commit, and the scene counts as not committed behind it.  The
 * default is 0.  It is independent of rt_scene_set_environment: it survives a change of environment, and it has no effect while
 * the committed scene has no environment.  At commit the effective shares c_e (environment) and c_l (light table) are fixed:
 *   no environment, or chance == 0:            c_e = 0,       c_l = 1,                 flag bit 2048 clear
 *   environment, chance > 0, no lights:        c_e = 1,       c_l = 0,                 flag bit 2048 set
 *   environment, chance > 0, lights:           c_e = chance,  c_l = fl(1 - chance),    flag bit 2048 set
 * Refusals, in this order: RT_ERR_INVALID for a NULL scene; RT_ERR_STATE while a render of the scene is in flight;
 * RT_ERR_INVALID for a chance that is NaN, below 0 or above 1. */
#define RT_SCENE_FLAG_ENVIRONMENT_LIGHT 2048u
RTOW_API int rt_scene_set_environment_light(rt_scene *s, double chance);
/* *chance_out: as set; *effective_out: c_e of the committed scene, 0 before commit.  Either may be NULL. */
RTOW_API int rt_scene_get_environment_light(rt_scene *s, double *chance_out, double *effective_out);
/* The importance sampler's tables, built by rt_scene_commit on the host in fp64, for an environment that is an image -- the float
 * image, or a texture that is itself an 8-bit image (W x H its own size; a checker of images is not one).  Texel (i, j), j counted
 * from the top row, has the weight w = max over the channels c of (intensity_c * value_c) times sin(pi * (j + 0.5) / H), value_c
 * the float widened to double or (1.0 / 255.0) * byte; pi = 3.1415926535897932385, sin the host's libm.  Row sums are taken in
 * order, i = 0 .. W - 1, and the total over the row sums in order, j = 0 .. H - 1.  marginal[j] = fl(fl(s_0 + ... + s_j) /
 * fl(total)), conditional[j * W + i] = fl(fl(w_0 + ... + w_i) / fl(s_j)), the last entry of each table exactly 1.0 -- the rule of
 * rt_scene_dump_lights.  A row of sum 0 holds 1.0 throughout and is never consulted.  A total that is not a positive finite
 * number, or an environment that is no image (solid, checker, noise), gives no tables.  Returns height (0: no tables; negative:
 * error, e.g. before commit) and *width_out; fills the arrays given where max_entries >= width * height. */
RTOW_API int rt_scene_dump_environment_cdf(rt_scene *s, int *width_out, int max_entries, double *marginal_out, double *conditional_out);
/* Reads what rt_write_pfm writes: "PF", width and height, a scale whose sign gives the byte order (negative: little endian) and
 * whose magnitude multiplies every value, then the rows bottom first.  Hands back width x height x 3 floats with the TOP row
 * first (what rt_environment::rgb takes), to be released with rt_pfm_free. */
RTOW_API int rt_pfm_load(const char *path, float **rgb_out, int *width, int *height);
RTOW_API void rt_pfm_free(float *rgb);

/* ---- render (RenderInit + Render, R/kernel.cu:110-154,675-691) ---- */
typedef struct rt_render_params {
    int32_t width, height;        /* full frame (maxX, maxY) */
    int32_t samples_per_pixel;    /* numSamples */
    int32_t max_depth;            /* literal 50 at R/kernel.cu:71 */
    uint64_t seed;                /* literal 1984 at R/kernel.cu:118 */
    int32_t stripe_rows;          /* multi-GPU: rows are dealt in stripes of this many rows ... */
    int32_t rank, world_size;     /* ... stripe k belongs to rank k % world_size.  1 GPU: rank 0 of 1 */
    int32_t variant;              /* 0 = strict: no FMA contraction, the reference's arithmetic operation by operation; frames equal the CPU
                                     oracle's bit for bit -- the build to use where the north star's 1e-5 tolerance matters.
                                     1 = fast: FMA contraction, 0-3 % faster.  A contracted comparison that falls the other way re-draws
                                     the rest of that pixel's random stream: rare at a few hundred samples on surface scenes (C2-C4:
                                     >= 0.9998 of the pixels within 1e-5), but on media scenes at thousands of samples per pixel most
                                     pixels leave the tolerance (C5 at 5000 spp: 0.24-0.75 within 1e-5; still a correct image) */
    int32_t device;               /* HIP device ordinal */
    int32_t flags;                /* RT_FLAG_* */
    void *stream;                 /* hipStream_t to launch on (NULL = the film's own stream) */
    int32_t coop_threshold;       /* tuning: sphere-list waves with fewer live lanes scan cooperatively (0 = default) */
    int32_t overdue_rays_per_sample; /* tuning: a pixel past this many rays/sample advances in extra cooperative passes (0 or <0 = never, the default) */
    int32_t shade_batch;          /* tuning: BVH kernels shade once this many lanes finished traversal (0 = default 16) */
    int32_t max_blocks_per_cu;    /* tuning: cap on resident 256-thread workgroups per CU (0 = as many as fit) */
    int32_t pixels_per_wave;      /* list worlds (HittableList worlds and small BVH worlds rendered as lists; no media): pixels a wave works
                                     on at a time, a power of two 1..64; the wave's other lanes share each ray's leaf tests (64 / pixels
                                     lanes per ray), the same frame bit for bit.  0 or 64 = one lane per ray, which is also the fastest
                                     setting for every frame size measured (a mixed list's leaves are different
                                     code, which a group of lanes runs one after the other like a single lane does); smaller values are
                                     for lists of one kind of leaf and for experiments */
    int32_t reserved0;
} rt_render_params;

#define RT_FLAG_KEEP_RNG_STATE 1u  /* do not re-seed: continue from the film's saved per-pixel state (progressive) */
#define RT_FLAG_OVERDUE_PRIORITY 4u /* tuning/diagnostics: overdue pixels raise their wave's priority instead of going cooperative */
#define RT_FLAG_ACCUMULATE 8u      /* progressive: with KEEP_RNG_STATE, add this launch's samples to the film's running sums;
                                      the pixels then hold sqrt(sum / all samples so far), bit-identical to one launch of that many spp */
#define RT_FLAG_FORCE_GENERAL 2u   /* tests: run the general kernel even where a specialised instantiation applies */
#define RT_FLAG_ALWAYS_WALK 32u     /* small BVH worlds without media (up to 16 cheap leaves) are rendered by scanning all leaves in the tree's
                                      leaf order (same closest hit, no node visits); this flag walks the tree anyway */
#define RT_FLAG_NO_PIXEL_CLASSES 64u /* hand every pixel out through the one tile queue (default: a rehearsal of the first samples lists the
                                      pixels with long ray chains, and some waves of every workgroup serve those first, a few pixels per
                                      wave, before they join the tile queue, which skips them -- sphere lists in two tiers of 4 and 8
                                      pixels per wave with the lanes sharing each ray's scan, primitive BVH worlds on the library's tree
                                      with the very longest chains one to a wave, deep composite worlds only where the frame is a few
                                      generations of pixels on the GPU's lanes, e.g. one rank's stripes; the image is the same either way) */
#define RT_FLAG_REFERENCE_TREE 128u  /* BVH worlds of primitives only are walked through the library's own tree (surface-area heuristic, near
                                      child first) -- no leaf draws random numbers there, so the closest hit is the one the reference's tree
                                      gives; this flag walks the reference's own tree in its own order instead (tests, timing).  A world in
                                      which two leaves coincide -- identical spheres (a moving sphere that rests counts as the static
                                      sphere it is), or two quads in one plane whose rectangles overlap, be they Quad leaves, faces of
                                      MakeBox boxes, or either behind Translate / RotateY -- has no library tree at all, nor the segmented
                                      walk of a composite world: there the order of the tests decides which of the two a ray sees.  (Not
                                      counted: faces of untransformed opaque boxes that abut, which no ray reaches.) */
#define RT_FLAG_EXACT_SCAN 256u      /* sphere-list worlds: every ray runs the reference's discriminant against every sphere (default: a cheaper
                                      conservative filter rejects the spheres a ray's line misses and only the survivors go through the
                                      reference's arithmetic; the image is the same bit for bit either way) */
#define RT_FLAG_FILTER_FP64 2048u     /* sphere-list worlds: the conservative filter in fp64, one sphere per 8 instructions (default: its packed
                                      fp32 form, two spheres per 9 instructions, a little coarser; the survivors always go through the
                                      reference's fp64 test, so the image is the same bit for bit) -- tests, timing */
#define RT_FLAG_NO_PRIMARY_LISTS 4096u /* sphere-list worlds: every camera ray goes through the scan of the whole list (default: where a wave
                                      scans one ray per lane, camera rays are tested against the short list of spheres that a ray through
                                      their 8x8 tile can reach, in list order, with the reference's test; the image is the same bit for
                                      bit either way) -- tests, timing */
#define RT_FLAG_NO_SCAN_WINDOWS 8192u /* sphere-list worlds: a pixel-parallel pass scans every trip of every run of the list (default: of a
                                      run whose trips are selective along an axis, only the trips that the pass's rays can reach while
                                      they are inside the run's slab, csrc/scan_window_rule.h; the image is the same bit for bit
                                      either way).  With the flag a launch runs the scan as it was before the windows, entered by the
                                      lanes that hold a ray; without it, where the scene has a window table, all 64 lanes of a wave
                                      enter the scan, idle lanes with a filter term that passes no sphere -- tests, timing */
#define RT_FLAG_ACCELERATE_LISTS 512u /* HittableList worlds of primitives only (no leaf draws random numbers): render through the library's
                                      own tree as a BvhNode world would be -- the reference's "BVH image == list image" invariant the other
                                      way round; off by default so that a list world is scanned as the reference scans it.  Ignored for
                                      a list with coincident leaves (see RT_FLAG_REFERENCE_TREE) */
#define RT_FLAG_COOP_SINGLE 1024u    /* tests: sphere-list worlds, thin waves scan one ray at a time with all 64 lanes (the older scheme)
                                      instead of several rays in groups of lanes */
#define RT_FLAG_ROW_MAJOR_TILES 16u /* BVH worlds: keep the pixel queue in row-major tile order (default: a short rehearsal ranks
                                      the 8x8 tiles by rays traced and the heaviest start first; the image is the same either way) */

typedef struct rt_render_stats {
    uint64_t samples;             /* samples this launch took: pixels rendered by this rank x spp, fewer with adaptive sampling */
    uint64_t rays;                /* RayColor loop iterations (one world Hit each) */
    double seconds_seed;          /* RNG seeding kernel, HIP events */
    double seconds_render;        /* render kernel, HIP events */
    uint32_t pixels;              /* pixels owned by this rank */
    uint32_t rows;                /* rows owned by this rank */
    uint32_t kernel_vgprs;
    uint32_t lds_bytes;
    uint32_t kernel_kind;         /* which instantiation ran: world*8 + media*4 + composite*2 + rich (world 0 bvh, 1 list, 2 sphere
                                     list) + nested*32 + library-tree*64 + grouped*128 + segmented*256 + adaptive*512 (KIND_*,
                                     csrc/launch_plan.h) */
    uint32_t pixels_per_wave;     /* what rt_render_params.pixels_per_wave came to for this launch (64 = one lane per ray) */
} rt_render_stats;

/* Rows owned by (rank, world_size) for a height: returns count, fills rows_out (ascending j) if non-NULL. */
RTOW_API int rt_stripe_rows(int height, int stripe_rows, int rank, int world_size, int *rows_out, int max_rows);

RTOW_API rt_film *rt_film_create(int device, int width, int height, int stripe_rows, int rank, int world_size);
RTOW_API void rt_film_destroy(rt_film *film);
/* Device pointer of this rank's compact framebuffer: rows_owned x width x 3 doubles (sqrt-gamma applied, like
 * frameBuffer[] at R/kernel.cu:150-153), rows in ascending j. */
RTOW_API void *rt_film_device_pixels(rt_film *film);
/* Render into caller-owned device memory instead (e.g. a torch tensor that RCCL will gather from); must hold
 * rt_film_pixel_bytes() bytes on the film's device.  NULL restores the film's own buffer. */
RTOW_API int rt_film_bind_pixels(rt_film *film, void *device_pixels);
RTOW_API size_t rt_film_pixel_bytes(rt_film *film);

/* ---- adaptive sampling: "render until the noise is below a threshold, at most samples_per_pixel samples" ----
 * Per pixel the film keeps, next to the colour sum (r, g, b): n = samples taken so far in this frame, and q = the sum over those
 * samples of y^2, y = (r_s + g_s) + b_s the plain sum of the three channels of sample s's radiance.  The rule is looked at
 * exactly when n >= min_samples and (n - min_samples) % check_interval == 0, and a pixel stops at the first such n where, with
 * N = (double)n and s = (r + g) + b:
 *     lhs = q*N - s*s;   m = max(s, luminance_floor*N);   rhs = ((tau*tau)*(N - 1))*(m*m);   stops <=> lhs <= rhs
 * (a NaN anywhere: it goes on) -- "standard error of the mean of y <= tau * max(mean of y, luminance_floor)" without divisions
 * or roots, every operation an IEEE-754 double operation in this order, never fused (the strict and the fast build alike).  A pixel that never stops ends at the
 * launch's samples_per_pixel, which is the cap.  Its value is sqrt(sum / n) with its OWN n: pixel for pixel the frame a plain
 * render of n samples gives.  The rule stops too early where light is found rarely (a pixel whose first min_samples samples
 * all miss a small lamp has q = s = 0): min_samples is the guard.  noise_threshold = 0 is accepted but decides pixels of equal
 * samples by rounding noise; use >= 1e-3, and NULL for "never stop early".
 * Accumulated frames (RT_FLAG_KEEP_RNG_STATE | RT_FLAG_ACCUMULATE): n, q and the stopped mark persist like the sums;
 * samples_per_pixel is then the most ADDITIONAL samples a pixel takes, check points count on the pixel's total n (k launches of S
 * are one launch of k*S), a stopped pixel is never touched again.  Changing the setting between two launches of one accumulated
 * frame makes the second rt_render_launch return RT_ERR_STATE; a re-seeding launch begins a new frame.  A launch without
 * RT_FLAG_ACCUMULATE, adaptive or not, ends an accumulated adaptive frame the film held (it overwrites the stopped pixels, which
 * nothing would write again).  A stopped pixel lives only in the buffer that was bound when it stopped: after
 * rt_film_bind_pixels to another buffer in the middle of such a frame the new buffer lacks the pixels that had stopped before. */
typedef struct rt_adaptive_params {
    int32_t min_samples, check_interval;      /* >= 2, >= 1 */
    double noise_threshold, luminance_floor;  /* tau >= 0, floor > 0 (0.01 is a good one) */
} rt_adaptive_params;
/* NULL = off (default).  Takes effect at the next launch.  RT_ERR_INVALID for parameters out of range,
 * RT_ERR_STATE while a launch on the film is in flight. */
RTOW_API int rt_film_set_adaptive(rt_film *film, const rt_adaptive_params *params);
/* Samples each pixel has had so far in this frame, full W x H, pixel (i,j) at j*W+i like rt_film_download;
 * pixels this rank does not own are 0.  Without adaptive: the frame's spp everywhere (0 before the first launch). */
RTOW_API int rt_film_download_sample_counts(rt_film *film, uint32_t *counts_full, int width, int height);
/* The rule above on the host, the same source the kernel compiles: 1 = a pixel with these sums stops at n,
 * 0 = it goes on (n below min_samples or not a check point included); -RT_ERR_INVALID for parameters out of range. */
RTOW_API int rt_adaptive_converged(const rt_adaptive_params *p, uint32_t n, double sum_r, double sum_g,
                                   double sum_b, double sum_y2);
/* Introspection for tests: the rule as the adaptive render kernels of one build compile it (variant 0 strict, 1 fast), run on
 * the device over `count` entries: q_out[k] = sums_rgbq[4k+3] + y^2 with y = the plain sum of sample_rgb[3k..3k+2], and
 * stops_out[k] = the rule on (n[k], sums_rgbq[4k], [4k+1], [4k+2], q_out[k]).  Host arrays in and out. */
RTOW_API int rt_adaptive_rule_on_device(int device, int variant, const rt_adaptive_params *p, uint32_t count, const uint32_t *n,
                                        const double *sums_rgbq, const double *sample_rgb, double *q_out, uint8_t *stops_out);

/* Introspection for tests: what rt_render_launch would decide for a committed scene and these params on a GPU of num_cus
 * compute units (film geometry from params: width, height, stripe_rows, rank, world_size; adaptive: as after
 * rt_film_set_adaptive).  Needs no device: the launch reaches its decisions through the same function (csrc/launch_plan.h)
 * and takes none anywhere else.  The frames do not depend on any of these fields, only the time they take. */
typedef struct rt_launch_plan {
    int32_t kernel_kind, lds_bytes, pixels_per_wave; /* as rt_render_stats reports them after the launch */
    int32_t kernel, probe_kernel;  /* the instantiation of the launch and of its rehearsal (csrc/launch_plan.h KernelId; not ABI) */
    int32_t waves_per_simd;        /* the occupancy that instantiation is compiled for */
    int32_t lds_nodes, lds_spheres; /* node rows / sphere planes are staged in LDS */
    int32_t reference_tree, always_walk, accelerate_lists; /* the flags of that name as the kernel choice saw them: a shutter
                                      that lets a moving sphere leave its box forces the reference's tree, walked, no accelerated list */
    int32_t coop_threshold, max_blocks_per_cu, probe_max_blocks_per_cu;
    int32_t node_burst, park_ratio, leaf_batch, object_batch, rounds, shade_batch;
    uint32_t ray_budget;
    int32_t rank_tiles, pixel_classes; /* rehearsal: 8x8 tiles ranked by cost / heavy pixels listed and served by waves of their own */
    int32_t probe_spp;             /* samples per pixel of the rehearsal (0: none) */
    int32_t tile_flatness_x8;      /* tiles stay row-major where the heaviest is below this / 8 of the mean */
    int32_t heavy_threshold, super_threshold; /* probed rays from which a pixel is listed / listed among the longest (0: no such list) */
    int32_t near_percent, near_neighbours; /* ... or at this share of the threshold with that many of its 8 neighbours over it */
    int32_t heavy_waves, heavy_ppw, super_ppw, heavy_priority, adaptive_ppw; /* serving waves per workgroup, pixels each takes, ... */
    /* The LDS layout of the launch, table by table (csrc/launch_plan.h LdsLayout, the very result the launch applies).  At the front
     * of the dynamic LDS block lie lds_front_bytes of node rows (BVH worlds) or survivor queues and sphere planes (sphere lists);
     * behind them the tables, in the order of RT_LDS_TABLE_NAMES.  lds_table_offset[k] = byte offset of table k in the block,
     * 0xFFFFFFFF = the kernel reads it from global memory; lds_table_bytes[k] = the table's unpadded size, 0 for an empty table and
     * for one this instantiation never considers. */
    int32_t lds_front_bytes;
    uint32_t lds_table_offset[18], lds_table_bytes[18];
    /* The rehearsal's samples: probe_keeps = 1 where the frame launch resumes from them (it renders samples_per_pixel - probe_spp
     * more of every pixel), 0 where it renders every sample again (adaptive films) and where there is no rehearsal.  probe_ray_cap:
     * rays at which a rehearsed pixel stops at once, its place on the longest-chain list being decided (super_threshold; 0: no
     * cap) -- such a pixel keeps nothing and the frame launch renders all of its samples. */
    int32_t probe_keeps, probe_ray_cap;
} rt_launch_plan;
#define RT_LDS_TABLES 18
#define RT_LDS_TABLE_NAMES "quad_aa boxes objects xforms media materials perlin spheres_tab group_boxes mspheres msphere_aux " \
                           "sphere_aux fast_order seg_media seg_cand park scan_pairs scan_spans"
RTOW_API int rt_plan_launch(rt_scene *s, const rt_render_params *params, int num_cus, int adaptive, rt_launch_plan *out);
/* Introspection for tests: the rays the rehearsal of the film's last launch booked for every pixel, full W x H like
 * rt_film_download_sample_counts -- at least rt_launch_plan.probe_ray_cap for a pixel the cap stopped.  RT_ERR_STATE where that
 * launch classified no pixels (rt_launch_plan.pixel_classes). */
RTOW_API int rt_film_download_probe_costs(rt_film *film, uint32_t *costs_full, int width, int height);

/* Upload the committed scene to a device (idempotent per device). */
RTOW_API int rt_scene_upload(rt_scene *s, int device);

/* Asynchronous on params->stream: seeds (unless KEEP_RNG_STATE) and renders this rank's rows into the film. */
RTOW_API int rt_render_launch(rt_scene *s, rt_film *film, const rt_render_params *params);
/* Waits for the launch, fills stats (HIP-event kernel durations, ray counter). */
RTOW_API int rt_render_finish(rt_scene *s, rt_film *film, rt_render_stats *stats);
/* Copies this rank's compact rows into a full W x H x 3 host frame (pixel (i,j) at (j*W+i)*3, j = 0 bottom). */
RTOW_API int rt_film_download(rt_film *film, double *frame_full, int width, int height);
/* Scatter compact rank buffers (as gathered over RCCL, rank-major) into a full frame; pure host code. */
RTOW_API int rt_deinterleave(const double *gathered, int width, int height, int stripe_rows, int world_size,
                             size_t rank_stride_doubles, double *frame_full);

/* ---- first-hit feature buffers (AOVs) and the edge-avoiding a-trous filter that uses them as edge stops ----
 * rt_film_render_features fills three film-owned device planes for the rows the film owns, compact like the pixels: albedo
 * (3 doubles per pixel), shading normal (3) and depth (1) of the closest hit over [0.001, inf) of the pixel's primary rays, found
 * by the traversal, leaf tests and hit record of the render kernels (the reference's tree or list in the reference's order).
 *   samples >= 1: the pixel's stream is seeded as a render seeds it, curand_init(seed, pixelIndex, 0); every feature sample's
 *     primary ray takes the camera's draws of a render sample, in the same order, and nothing else is drawn except by the
 *     world's hit test itself (media).  The pixel's value is (1 / N) * (sum over its samples in order), as a render averages.
 *   samples == 0: one ray through the pixel centre, u = (i + 0.5) / W, v = (j + 0.5) / H, no lens offset, time = time0; the
 *     camera draws nothing (media still draw from the pixel's stream); the one sample is stored as it is.
 * What a sample records:          surface hit                                          medium hit                  miss
 *   albedo   Lambertian / isotropic: the material's texture at (u, v, p); metal:       the phase material's        the camera's
 *            its albedo; dielectric: (1, 1, 1); diffuse light: its emitted colour      texture value               background
 *   normal   the unit shading normal, faced against the ray, in world space            (0, 0, 0)                   (0, 0, 0)
 *   depth    t * |ray direction|                                                       the same                    0
 * With an environment (rt_scene_set_environment) the albedo of a miss is the environment's value along the sample's ray, not the
 * camera's background; normal and depth stay 0.
 * The film's saved RNG state, its pixels, sums and statistics are neither read nor written: a feature pass between two
 * progressive launches changes nothing of the frame.  The call returns when the planes are filled (it waits on params->stream,
 * NULL = the film's own).  RT_ERR_STATE while a render of the film is in flight. */
typedef struct rt_feature_params {
    int32_t width, height;
    int32_t samples;     /* 0: one ray through the pixel centre; N >= 1: N jittered primary rays, averaged */
    uint64_t seed;       /* the per-pixel stream, as in rt_render_params */
    int32_t variant;     /* 0 strict, 1 fast, as for renders */
    void *stream;
    int32_t reserved[4];
} rt_feature_params;
RTOW_API int rt_film_render_features(rt_scene *s, rt_film *film, const rt_feature_params *params);
/* The full frame, pixel (i, j) at j*W+i like rt_film_download (albedo and normal W*H*3 doubles, depth W*H); pixels this rank
 * does not own are 0.  Any pointer may be NULL.  RT_ERR_STATE before the film's first feature pass. */
RTOW_API int rt_film_download_features(rt_film *film, double *albedo_full, double *normal_full, double *depth_full, int width,
                                       int height);
/* Device pointer of one compact plane (which: 0 albedo, 1 normal, 2 depth), for callers that gather over RCCL as they do with
 * the pixels; NULL before the first feature pass. */
RTOW_API void *rt_film_device_features(rt_film *film, int which);

/* The edge-avoiding a-trous wavelet filter of Dammertz et al. 2010.  Level k = 0 .. iterations-1 reads level k-1's output (the
 * guides never change) and, for pixel p and the 25 taps q = p + 2^k * (dx, dy), dx, dy in {-2..2}, dy outer, dx inner, both
 * ascending, taps outside the frame skipped:
 *     h = {1/16, 1/4, 3/8, 1/4, 1/16}
 *     e = |c_p - c_q|^2 / (sigma_color * 2^-k)^2 + |a_p - a_q|^2 / sigma_albedo^2 + |n_p - n_q|^2 / sigma_normal^2
 *         + ((z_p - z_q) / max(z_p, z_q, 1e-30))^2 / sigma_depth^2
 *     w = h[dx+2] * h[dy+2] * exp(-e);     out_p = (sum w * c_q) / (sum w)
 * c = the colour as the film stores it (the reference's sqrt-gamma values, unclamped), a, n, z = albedo, normal, depth.  fp64,
 * no contraction, one exp per tap; |.|^2 is the plain three-term sum; a sigma of +inf switches its term off (it contributes an
 * exact 0).  A tap whose colour is not finite (NaN, +-inf) has weight 0; a centre whose colour is not finite passes through. */
typedef struct rt_denoise_params {
    int32_t iterations;                 /* 1..8 levels; level k uses step 2^k, k = 0.. */
    double sigma_color, sigma_albedo, sigma_normal, sigma_depth;   /* > 0; +inf switches a term off */
} rt_denoise_params;
/* Filters the film's pixels with the film's feature planes into a second film-owned buffer (read it with
 * rt_film_download_denoised): never in place, the raw pixels, sums and RNG state stay as they are and accumulated or adaptive
 * frames continue afterwards.  RT_ERR_INVALID for parameters out of range; RT_ERR_UNSUPPORTED for a film that owns only part of
 * the frame (world_size > 1: its neighbours live on other ranks -- gather and use rt_denoise_frame); RT_ERR_STATE before a
 * feature pass on this film and while a render is in flight.  Returns when the result is there. */
RTOW_API int rt_film_denoise(rt_film *film, const rt_denoise_params *params);
RTOW_API int rt_film_download_denoised(rt_film *film, double *frame_full, int width, int height);
/* The same kernel on uploaded copies of host arrays (frames gathered from several ranks; synthetic inputs): color and out W*H*3,
 * albedo and normal W*H*3, depth W*H; albedo, normal and depth may each be NULL, that term is then off.  Parameters are checked
 * before the device is touched. */
RTOW_API int rt_denoise_frame(int device, const double *color, const double *albedo, const double *normal, const double *depth,
                              int width, int height, const rt_denoise_params *params, double *out);

/* ---- ray queries: closest hit and occlusion for caller-supplied rays ----
 * Ray k is origin[3k..3k+2] + t * direction[3k..3k+2] (the direction need not be a unit vector: t is the ray parameter) at time
 * time[k], searched over the reference's interval of Hittable::Hit: tmin < t < tmax for spheres, tmin <= t <= tmax for quads
 * (R/Sphere.h:38,50, R/Quad.h:59-64).  A per-ray array that is NULL takes the scalar of rt_query_params for every ray.
 *   mode 0, closest hit: the reference's world->Hit(ray, tmin, tmax, rec, &stream).  The reference's own tree or list is visited in
 *     the reference's order, through the leaf tests and the hit record of the render kernels -- what the general kernels do under
 *     RT_FLAG_REFERENCE_TREE | RT_FLAG_FORCE_GENERAL -- so the reference's tie rules hold (RT_FLAG_REFERENCE_TREE) and a
 *     ConstantMedium draws from the ray's stream, curand_init(seed, k + first_sequence, 0); nothing else draws.  The library's own
 *     tree is never used: it is valid only while every hit stays inside its leaf's box, which depends on the shutter (flat_scene.h
 *     FastNodeRec), and a caller's times are arbitrary.
 *   mode 1, occlusion: occluded[k] = 1 exactly where the closest-hit query of ray k with the same parameters reports a hit.  In a
 *     world without ConstantMedium leaves the search stops at the first accepted hit; with media it is the full search (what a
 *     medium answers depends on what was found before it).  Only `occluded` is written.
 * What a closest-hit query writes, each output only where its pointer is not NULL (an output left NULL costs no texture or
 * material work):
 *   t           the ray parameter of the hit, +inf for a miss
 *   normal      the unit shading normal, faced against the ray, in world space; (0, 0, 0) for a medium hit and for a miss
 *   uv          HitRecord U, V of the primitive that was hit; (0, 0) for a medium hit and for a miss
 *   albedo      the table of rt_film_render_features above, the camera's background for a miss included
 *   leaf        the position, in rt_scene_dump_leaves order, of the world leaf whose test produced the winning record; -1: miss
 *   front_face  HitRecord FrontFace (1 for a medium hit, 0 for a miss)
 *   material    0 Lambertian, 1 metal, 2 dielectric, 3 diffuse light, 4 isotropic; 255 for a miss
 *   occluded    1 for a hit, 0 for a miss
 * Both calls return when the results are there (they wait on the stream), so no query outlives a destroy or a re-commit of the
 * scene; a query reads and writes no film.  Parameters are checked before the device is touched: RT_ERR_STATE before commit;
 * RT_ERR_INVALID for a count below 0 or above 2^30, a NULL origin or direction with count > 0, a mode or variant other than 0 / 1,
 * a tmin that is NaN, tmax < tmin (or NaN).  count == 0 returns RT_OK without a launch.  A ray with a zero or non-finite direction
 * terminates (every walk is a bounded loop); its result is unspecified. */
typedef struct rt_query_params {
    int64_t  count;            /* rays; 0 is allowed (no launch), > 2^30 is RT_ERR_INVALID */
    double   tmin, tmax;       /* used where the per-ray arrays are NULL; tmax = +inf means DBL_MAX, what a render passes */
    double   time;             /* used where times is NULL */
    uint64_t seed;             /* ray k draws from curand_init(seed, k + first_sequence, 0): only media draw */
    uint64_t first_sequence;
    int32_t  mode;             /* 0 closest hit, 1 occlusion */
    int32_t  variant;          /* 0 strict, 1 fast, as for renders */
    int32_t  device;
    void    *stream;           /* NULL = the default stream */
    int32_t  reserved[4];
} rt_query_params;
typedef struct rt_query_rays {
    const double *origin, *direction;   /* count x 3 each */
    const double *time, *tmin, *tmax;   /* count each, any may be NULL */
} rt_query_rays;
typedef struct rt_query_hits {
    double *t;             /* count */
    double *normal;        /* count x 3 */
    double *uv;            /* count x 2 */
    double *albedo;        /* count x 3 */
    int32_t *leaf;         /* count */
    uint8_t *front_face;   /* count */
    uint8_t *material;     /* count */
    uint8_t *occluded;     /* count; any pointer may be NULL */
} rt_query_hits;
typedef struct rt_query_stats {
    uint64_t rays, hits;
    double seconds;               /* the query kernel, HIP events */
    uint32_t kernel_vgprs, scratch_bytes;   /* of the instantiation that ran: registers, private memory per lane */
} rt_query_stats;
/* rays and hits hold device pointers (on params->device).  stats may be NULL: the call is then the launch and the wait alone (no
 * events, no count of the rays that hit).  A scene is thread-compatible, as everywhere in this header: one call at a time. */
RTOW_API int rt_scene_intersect_device(rt_scene *s, const rt_query_params *params, const rt_query_rays *rays, const rt_query_hits *hits,
                                       rt_query_stats *stats);
/* the same on host arrays (uploaded, queried, copied back) */
RTOW_API int rt_scene_intersect(rt_scene *s, const rt_query_params *params, const rt_query_rays *rays, const rt_query_hits *hits,
                                rt_query_stats *stats);
/* sizeof of rt_query_params, rt_query_rays, rt_query_hits, rt_query_stats as this library was compiled (bindings check theirs) */
RTOW_API void rt_query_abi_sizes(uint32_t out4[4]);

/* ---- radiance queries: path-trace caller-supplied rays ----
 * Ray k is origin[3k..3k+2] + t * direction[3k..3k+2] at time time[k] (params->time where `time` is NULL), as in the ray queries.
 * `samples` paths are traced from it, one after the other, all drawing from the ray's one stream.  Sample s is what the
 * reference's RayColor(ray, world, max_depth, &stream) returns (R/kernel.cu:66-98), as the render kernels compute it: throughput
 * (1, 1, 1), accumulated (0, 0, 0), depth 0; the world is searched over (0.001, DBL_MAX); a miss adds throughput * background and
 * ends the path; a hit adds what the material emits and scatters, and the path ends where the material does not scatter or
 * where ++depth >= max_depth.  The world is searched as the ray queries search it -- the reference's own tree or list in the
 * reference's order, every table from global memory, never the library's own tree -- so media draw what they draw in a render.
 * Here every ray draws (scatter directions, Fresnel choices, media): the stream of ray k is rng_state[6k..6k+5] = {d, v0..v4} as
 * rt_rng_state writes them, or, where rays->rng_state is NULL, curand_init(seed, k + first_sequence, 0) -- always seeded.
 * Outputs, each only where its pointer is not NULL (not all three may be NULL):
 *   radiance   (1 / samples) * (((0 + L_1) + L_2) + ...), linear: no gamma, no clamp -- the square root of it is the pixel a
 *              render of `samples` samples writes for the same rays and streams
 *   path_rays  world searches (iterations of RayColor's loop) over all samples of the ray, modulo 2^32
 *   rng_state  the ray's stream after its last draw, to continue it in a later call; may be the array rays->rng_state points to
 * max_depth == 0: every radiance is 0, nothing is searched, nothing is drawn (the state that goes out is the state that came in).
 * Both calls return when the results are there (they wait on the stream) and read and write no film.  Parameters are checked
 * before the device is touched: RT_ERR_STATE before commit; RT_ERR_INVALID for a count below 0 or above 2^30, samples outside
 * 1 .. 2^20, max_depth < 0, a variant other than 0 / 1, a NULL origin or direction with count > 0, all three outputs NULL.
 * count == 0 returns RT_OK without a launch.  A ray with a zero or non-finite direction terminates (at most samples * max_depth
 * bounded searches); its result is unspecified. */
typedef struct rt_radiance_params {
    int64_t  count;            /* rays; 0 is allowed (no launch), > 2^30 is RT_ERR_INVALID */
    int32_t  samples;          /* 1 .. 2^20: paths traced per ray, all from the ray's one stream, one after the other */
    int32_t  max_depth;        /* >= 0, as rt_render_params.max_depth; 0: black, nothing searched, nothing drawn */
    double   time;             /* used where rays->time is NULL */
    uint64_t seed;             /* ray k: curand_init(seed, k + first_sequence, 0), unless rays->rng_state is given */
    uint64_t first_sequence;
    int32_t  variant;          /* 0 strict, 1 fast, as for renders */
    int32_t  device;
    void    *stream;           /* NULL = the default stream */
    int32_t  reserved[4];
} rt_radiance_params;
typedef struct rt_radiance_rays {
    const double   *origin, *direction;   /* count x 3 each */
    const double   *time;                 /* count, or NULL */
    const uint32_t *rng_state;            /* count x 6 {d, v0..v4} as rt_rng_state writes them, or NULL: seeded as above */
} rt_radiance_rays;
typedef struct rt_radiance_out {
    double   *radiance;        /* count x 3 */
    uint32_t *path_rays;       /* count */
    uint32_t *rng_state;       /* count x 6; any pointer may be NULL, not all three */
} rt_radiance_out;
typedef struct rt_radiance_stats {
    uint64_t rays;                          /* the sum of path_rays (counted whether or not path_rays is asked for) */
    double seconds;                         /* the radiance kernel, HIP events */
    uint32_t kernel_vgprs, scratch_bytes;   /* of the instantiation that ran: registers, private memory per lane */
} rt_radiance_stats;
/* rays and out hold device pointers (on params->device).  stats may be NULL: the call is then the launch and the wait alone. */
RTOW_API int rt_scene_radiance_device(rt_scene *s, const rt_radiance_params *params, const rt_radiance_rays *rays,
                                      const rt_radiance_out *out, rt_radiance_stats *stats);
/* the same on host arrays (uploaded, traced, copied back) */
RTOW_API int rt_scene_radiance(rt_scene *s, const rt_radiance_params *params, const rt_radiance_rays *rays, const rt_radiance_out *out,
                               rt_radiance_stats *stats);
/* sizeof of rt_radiance_params, rt_radiance_rays, rt_radiance_out, rt_radiance_stats as this library was compiled */
RTOW_API void rt_radiance_abi_sizes(uint32_t out4[4]);

/* ---- path steps: one bounce of RayColor for caller-supplied rays ----
 * What happens at the hit: Material::Scatter and Emitted for a caller that continues the path itself (its own termination rule,
 * light sampling beside rt_scene_intersect's occlusion mode, per-bounce outputs).  Ray k is origin[3k..3k+2] + t *
 * direction[3k..3k+2] at time time[k] (params->time where `time` is NULL), as in the radiance queries, and the step is one
 * iteration of RayColor's loop (R/kernel.cu:74-94) exactly as a radiance query runs it: the world is searched over
 * (0.001, DBL_MAX) -- the reference's own tree or list in the reference's order, every table from global memory, never the
 * library's own tree -- then the hit record is made and the material emits and scatters.  The stream of ray k is
 * rng_state[6k..6k+5] = {d, v0..v4} as rt_rng_state writes them, or, where rays->rng_state is NULL, curand_init(seed,
 * k + first_sequence, 0) -- always seeded.  Media draw inside the search, materials after it, in the order of a render.
 * Outputs, each only where its pointer is not NULL (not all may be NULL):
 *   status       0 = miss; 1 = the path ends at this hit (a diffuse light; a metal whose scattered direction falls below the
 *                surface); 2 = scattered
 *   emitted      count x 3.  A miss: the camera's background.  A diffuse light: its texture's value.  Otherwise (0, 0, 0).
 *   attenuation  count x 3.  Scatter's attenuation where status is 2; otherwise (0, 0, 0).
 *   origin, direction, time   the scattered ray where status is 2; elsewhere the input ray, unchanged bit for bit
 *   t            the ray parameter of the hit, +inf for a miss
 *   normal, front_face, material   as in rt_query_hits
 *   rng_state    count x 6: the ray's stream after the step's last draw
 * The values are those of the radiance query's arithmetic: the step runs it from throughput (1, 1, 1) and accumulated (0, 0, 0),
 * so emitted is 0 + 1 * x and attenuation is 1 * a -- x and a bit for bit, except that a negative zero comes out as a positive
 * one, which no later sum can tell apart.  A caller that folds, one operation at a time and nothing fused,
 *   acc = acc + thr * emitted   where status is 0 or 1        thr = thr * attenuation   where status is 2
 * from acc (0, 0, 0), thr (1, 1, 1), over at most max_depth steps of the rays of status 2, has what rt_scene_radiance sums for one
 * sample, bit for bit in the strict build (the fast build may fuse acc + thr * x, which the fold cannot restate).
 * Every output may be the input array of the same meaning (origin, direction, time, rng_state): each ray is read, its six words
 * included, before anything of it is written.
 * Both calls return when the results are there (they wait on the stream) and read and write no film.  Parameters are checked
 * before the device is touched: RT_ERR_STATE before commit; RT_ERR_INVALID for a count below 0 or above 2^30, a variant other
 * than 0 / 1, a NULL origin or direction with count > 0, every output NULL.  count == 0 returns RT_OK without a launch.  A ray
 * with a zero or non-finite direction terminates (one bounded search, straight-line shading; the rejection loops depend on the
 * stream alone); its result is unspecified. */
typedef struct rt_path_step_params {
    int64_t  count;            /* rays; 0 is allowed (no launch), > 2^30 is RT_ERR_INVALID */
    double   time;             /* used where rays->time is NULL */
    uint64_t seed;             /* ray k: curand_init(seed, k + first_sequence, 0), unless rays->rng_state is given */
    uint64_t first_sequence;
    int32_t  variant;          /* 0 strict, 1 fast, as for renders */
    int32_t  device;
    void    *stream;           /* NULL = the default stream */
    int32_t  reserved[4];
} rt_path_step_params;
typedef struct rt_path_step_rays {
    const double   *origin, *direction;   /* count x 3 each */
    const double   *time;                 /* count, or NULL */
    const uint32_t *rng_state;            /* count x 6 {d, v0..v4} as rt_rng_state writes them, or NULL: seeded as above */
} rt_path_step_rays;
typedef struct rt_path_step_out {
    uint8_t  *status;          /* count */
    double   *emitted;         /* count x 3 */
    double   *attenuation;     /* count x 3 */
    double   *origin;          /* count x 3 */
    double   *direction;       /* count x 3 */
    double   *time;            /* count */
    double   *t;               /* count */
    double   *normal;          /* count x 3 */
    uint8_t  *front_face;      /* count */
    uint8_t  *material;        /* count */
    uint32_t *rng_state;       /* count x 6; any pointer may be NULL, not all */
} rt_path_step_out;
typedef struct rt_path_step_stats {
    uint64_t rays, scattered;               /* rays stepped; those of status 2 (counted whether or not status is asked for) */
    double seconds;                         /* the step kernel, HIP events */
    uint32_t kernel_vgprs, scratch_bytes;   /* of the instantiation that ran: registers, private memory per lane */
} rt_path_step_stats;
/* rays and out hold device pointers (on params->device).  stats may be NULL: the call is then the launch and the wait alone. */
RTOW_API int rt_scene_path_step_device(rt_scene *s, const rt_path_step_params *params, const rt_path_step_rays *rays,
                                       const rt_path_step_out *out, rt_path_step_stats *stats);
/* the same on host arrays (uploaded, stepped, copied back) */
RTOW_API int rt_scene_path_step(rt_scene *s, const rt_path_step_params *params, const rt_path_step_rays *rays, const rt_path_step_out *out,
                                rt_path_step_stats *stats);
/* sizeof of rt_path_step_params, rt_path_step_rays, rt_path_step_out, rt_path_step_stats as this library was compiled */
RTOW_API void rt_path_step_abi_sizes(uint32_t out4[4]);

/* ---- path advances: step a batch of paths by one bounce, fold what ended, keep the live rays packed, on the device ----
 * What a caller's loop around rt_scene_path_step does between two steps, done by the library: one call steps the live rays, adds
 * the light of the paths that ended to a radiance array, writes the scattered rays packed, in their input order, into a second
 * set of arrays and leaves their number in device memory, so that the next call can be enqueued without the host learning it.
 * Let n = min(*rays->count, params->count), or params->count where rays->count is NULL.  Rows at and beyond n are never read.  A
 * word larger than the capacity params->count is clamped: it is no error, and nothing beyond params->count rows is read or
 * written.  Operation by operation, for each k < n with alive[k] != 0 (every k < n where `alive` is NULL):
 *   ray k is stepped exactly as rt_scene_path_step steps it: the same search, hit record, shading and stream rules, the stream
 *   rng_state[6k..6k+5] or, where that is NULL, curand_init(seed, k + first_sequence, 0).
 *   id = ray_id[k] (k where ray_id is NULL), thr = throughput[3k..3k+2] ((1, 1, 1) where throughput is NULL).
 *   status 0 or 1 (the path ends): where out->radiance is given and 0 <= id < sources,
 *       radiance[id] = radiance[id] + thr * emitted
 *     the product rounded, then the sum -- one operation at a time in the strict build, the fold stated above for the path steps;
 *     the fast build may fuse the two (0 + thr * e is exact either way).  An id outside the range adds nothing.  THE IDS OF LIVE
 *     RAYS MUST BE DISTINCT: each ended ray is one plain load, add and store, no atomics.
 *   status 2 (scattered): the ray is survivor j, where j counts the survivors before it in input order -- the compaction is
 *     stable.  Row j of each output given holds the scattered ray (origin, direction), its time, the stream after the step
 *     (rng_state), thr * attenuation (throughput; one multiply in either build), the id (ray_id), and t, normal, front_face,
 *     material of the hit it scattered from, as rt_query_hits.
 * A ray with alive[k] == 0 is dropped untraced: nothing is added for it and it is no survivor.  *out->count = the number of
 * survivors.  Output rows from the survivors' count up to params->count are unspecified.  Inputs are only read.
 * Folding sources = count fresh rays over max_depth calls -- a zeroed radiance array, the two array sets swapped each time, whoever
 * is still alive after the last call dropped -- is rt_scene_radiance with samples = 1, bit for bit in the strict build.
 * Aliasing: an output array may NOT be the input array of the same meaning (origin, direction, time, rng_state, throughput,
 * ray_id; RT_ERR_INVALID, decided by pointer equality): a compaction across workgroups cannot be done in place.  out->count may
 * be the word rays->count points to: it is read by the first kernel of the call and written by the last.
 * Waiting: with stats == NULL, rt_scene_path_advance_device ENQUEUES ON params->stream AND RETURNS WITHOUT WAITING -- the point of
 * the call, and the one difference from its siblings above.  With stats it waits and fills them.  rt_scene_destroy, a re-commit
 * followed by an upload, and whatever else frees the scene's device tables first wait for the last advance enqueued on that
 * scene.  As everywhere, one call at a time per scene; advances that share a workspace must be on one stream or ordered by the
 * caller, and the caller's arrays must stay allocated until the stream has run the call.
 * The host-array form rt_scene_path_advance uploads, runs, waits and copies back the count word and the first *out->count rows of
 * each output; `workspace` is ignored, rays->count and out->count are host words, radiance (sources x 3) is copied both ways.
 * Refusals, all before the device is touched, in this order: RT_ERR_STATE before commit; RT_ERR_INVALID for count or sources
 * outside 0 .. 2^30, a variant other than 0 / 1, a NULL origin or direction input with count > 0, a NULL out->origin,
 * out->direction or out->count, out->radiance given with sources == 0, an aliased pair, and in the device call a workspace that
 * is NULL or smaller than rt_path_advance_workspace_bytes(count) (a count of 0 needs none).  count == 0 is RT_OK with nothing
 * launched and nothing written; the other parameters are still checked.  A zero or non-finite direction terminates with an
 * unspecified result, as in the path steps. */
typedef struct rt_path_advance_params {
    int64_t  count;            /* capacity: rows readable in every input and writable in every output; 0 .. 2^30 */
    int64_t  sources;          /* rows of out->radiance; 0 .. 2^30 */
    double   time;             /* used where rays->time is NULL */
    uint64_t seed;             /* ray k: curand_init(seed, k + first_sequence, 0), unless rays->rng_state is given */
    uint64_t first_sequence;
    int32_t  variant;          /* 0 strict, 1 fast */
    int32_t  device;
    void    *stream;           /* NULL = the default stream */
    void    *workspace;        /* device call only: device memory, >= rt_path_advance_workspace_bytes(count); its layout is private */
    uint64_t workspace_bytes;
    int32_t  reserved[4];
} rt_path_advance_params;
typedef struct rt_path_advance_rays {
    const double   *origin, *direction;   /* count x 3 each */
    const double   *time;                 /* count, or NULL */
    const uint32_t *rng_state;            /* count x 6, or NULL: seeded */
    const double   *throughput;           /* count x 3, or NULL: (1, 1, 1) */
    const int32_t  *ray_id;               /* count, or NULL: k */
    const uint8_t  *alive;                /* count, or NULL: all; a ray with alive[k] == 0 is dropped untraced */
    const uint32_t *count;                /* one word, or NULL: params->count.  Rays stepped = min(*count, params->count) */
} rt_path_advance_rays;
typedef struct rt_path_advance_out {
    double   *radiance;        /* sources x 3, read-modify-write; or NULL: nothing is folded */
    double   *origin;          /* count x 3; required */
    double   *direction;       /* count x 3; required */
    double   *time;            /* count; this and the following are optional */
    uint32_t *rng_state;       /* count x 6 */
    double   *throughput;      /* count x 3 */
    int32_t  *ray_id;          /* count */
    double   *t;               /* count: the hit the survivor scattered from, as rt_query_hits */
    double   *normal;          /* count x 3 */
    uint8_t  *front_face;      /* count */
    uint8_t  *material;        /* count */
    uint32_t *count;           /* one word: the survivors; required */
} rt_path_advance_out;
typedef struct rt_path_advance_stats {
    uint64_t rays, scattered;               /* rays stepped (below n and alive); the survivors */
    double seconds;                         /* the call's three kernels, HIP events */
    uint32_t kernel_vgprs, scratch_bytes;   /* of the step kernel that ran: registers, private memory per lane */
} rt_path_advance_stats;
/* rays and out hold device pointers (on params->device), the two count words included.  stats == NULL: enqueue and return. */
RTOW_API int rt_scene_path_advance_device(rt_scene *s, const rt_path_advance_params *params, const rt_path_advance_rays *rays,
                                          const rt_path_advance_out *out, rt_path_advance_stats *stats);
/* the same on host arrays (uploaded, advanced, waited for, copied back) */
RTOW_API int rt_scene_path_advance(rt_scene *s, const rt_path_advance_params *params, const rt_path_advance_rays *rays,
                                   const rt_path_advance_out *out, rt_path_advance_stats *stats);
/* bytes of workspace a device call of capacity `count` needs: 0 for 0, non-decreasing in count */
RTOW_API uint64_t rt_path_advance_workspace_bytes(int64_t count);
/* sizeof of rt_path_advance_params, rt_path_advance_rays, rt_path_advance_out, rt_path_advance_stats as this library was compiled */
RTOW_API void rt_path_advance_abi_sizes(uint32_t out4[4]);

/* ---- light sampling queries: sample the emitters of the light table, and the density of doing so ----
 * For next-event estimation and multiple importance sampling beside rt_scene_path_step and the occlusion mode of
 * rt_scene_intersect.  Two calls over the rows of rt_scene_dump_lights; neither searches the world (visibility is the caller's
 * shadow ray).  Every operation below is one IEEE-754 double operation in the order written, a * b + c two of them; the strict
 * build fuses nothing, so its outputs can be restated to the bit (tests/light_restated.py does); the fast build may fuse.
 * P(k) = cdf[k] - cdf[k - 1] (cdf[0] for k = 0) under params->strategy; pi = 3.1415926535897932385.
 *
 * rt_scene_sample_lights: for point k, P = point[3k..3k+2] at time[k] (params->time where `time` is NULL), from the stream
 * rng_state[6k..6k+5] = {d, v0..v4} or, where that is NULL, curand_init(seed, k + first_sequence, 0).  Draws, all (double)
 * curand_uniform, in this order:
 *   1. xi: the light is the first k with cdf[k] >= xi (a binary search; the draw happens with one light too)
 *   2. quad:      a, b.                                      S = (Q + a * u) + b * v, per component
 *      triangle:  a, b; where a + b > 1: a = 1 - a, b = 1 - b.    S as for the quad
 *      sphere (centre C, moving spheres at the point's time; radius r): pairs a, b, p = (2 * a - 1, 2 * b - 1), s = p.x * p.x + p.y * p.y,
 *      until s < 1 and s > 0 (the lens loop of the camera).  Then, whatever P is -- the draws depend on the stream alone:
 *        oc = C - P, d2 = (oc.x * oc.x + oc.y * oc.y) + oc.z * oc.z, r2 = r * r;  d2 <= r2 (P inside, or a NaN): invalid sample
 *        w = (1 / sqrt(d2)) * oc;  cosmax = sqrt(1 - r2 / d2);  omc = 1 - cosmax;  omc == 0: invalid sample
 *        z = 1 - s * omc;  rho = sqrt(1 - z * z);  q = sqrt(s);  ex = (rho * p.x) / q;  ey = (rho * p.y) / q
 *        e1: with ax = |w.x|, ay = |w.y|, az = |w.z|:  ax >= ay and ax >= az: t = (w.z, 0, -w.x), e1 = (1 / sqrt(w.z * w.z + w.x * w.x)) * t
 *                                                     else ay >= az:         t = (-w.y, w.x, 0), e1 = (1 / sqrt(w.y * w.y + w.x * w.x)) * t
 *                                                     else:                  t = (0, -w.z, w.y), e1 = (1 / sqrt(w.z * w.z + w.y * w.y)) * t
 *        e2 = w x e1 (the full cross product, its zero terms included)
 *        g = (z * w + ex * e1) + ey * e2;  direction = (1 / sqrt((g.x * g.x + g.y * g.y) + g.z * g.z)) * g
 *        the near intersection, as the renderer's own sphere test finds it for the ray (P, direction) (R/Sphere.h:28-50), so that a shadow
 *        ray along `direction` meets the lamp at this very parameter: po = P - C, qa = direction . direction, qb = po . direction,
 *        qc = po . po - r2 (every dot product (x + y) + z), disc = qb * qb - qa * qc, distance = (-qb - sqrt(disc)) / qa;  disc <= 0
 *        (the rounded direction grazes past the sphere: a sample within a few ulps of the cone's rim) or distance <= 0: invalid
 *        sample;  S = P + distance * direction
 *   planar lights: D = S - P, d2 = (D.x * D.x + D.y * D.y) + D.z * D.z, distance = sqrt(d2), direction = (1 / distance) * D;
 *     d2 == 0 (or a NaN): invalid sample
 *   either kind: a density (below) that is not a positive finite number -- a light of area 0, a chance of 0 -- is an invalid sample
 * Outputs, each only where its pointer is not NULL (not all may be NULL):
 *   direction    count x 3: the unit direction from P to the sample; (0, 0, 0) for an invalid sample and without lights
 *   distance     count: P + distance * direction is the sample; 0 for an invalid sample
 *   light        count: the light's row, also for an invalid sample; -1 in a scene without lights
 *   pdf          count: the solid-angle density of the direction under the picked light TIMES P(light); 0 for an invalid sample.
 *                planar: c = |(n.x * dir.x + n.y * dir.y) + n.z * dir.z|; c == 0: invalid; else (d2 / (c * area)) * P(k)
 *                sphere: P(k) / ((2 * pi) * omc), uniform over the cone the sphere subtends
 *   emitted      count x 3: the light's texture at the sample (both sides emit, as Material::Emitted does), through the render
 *                kernels' texture code with the point S and the primitive's own U, V: a and b for a quad or triangle; for a sphere
 *                the reference's (R/Sphere.h:74-81) of (1 / r) * (S - C), computed only where the material has an image texture,
 *                else 0 -- of the sphere in WORLD space: an image on a sphere under RotateY is not turned.  0 for an invalid sample
 *   scatter_pdf  count: the density with which the renderer's own Material::Scatter sends a ray from a surface of normal[3k..] and
 *                material[k] (as rt_query_hits.material) into `direction`: Lambertian (0), c = n . direction: c > 0: (2 * ((c * c) *
 *                c)) / pi, else 0 -- the exact density of unit-normal + uniform point of the unit ball (R/Material.h:67-82), which is
 *                NOT a cosine lobe; isotropic (4): 1 / (4 * pi); metal, dielectric, diffuse light, 255: 0 (they are treated as
 *                specular: all their light arrives through Scatter).  0 for an invalid sample
 *   contribution count x 3: (scatter_pdf / pdf) * emitted, (0, 0, 0) where either density is 0
 *   rng_state    count x 6: the stream after the last draw; may be the array points->rng_state points to
 * A scene without lights: RT_OK, light = -1, every other output 0, the stream that goes out is the stream that came in (or was seeded).
 *
 * rt_scene_light_pdf: for ray k (origin, direction -- not necessarily unit -- and time as above) pdf[k] = the sum over ALL lights
 * whose surface the ray meets at a parameter t > 0 of that light's density above under params->strategy: the density with which
 * rt_scene_sample_lights from `origin` produces this direction -- what multiple importance sampling needs when a scattered ray
 * finds a lamp.  Planar lights: the plane at t = (n . (Q - o)) / (n . d), n . d != 0, the interior rule of the primitive (quad: 0 <=
 * alpha, beta <= 1; triangle: 0 <= alpha, 0 <= beta, alpha + beta <= 1, with alpha, beta from m = u x v as m . (ph x v) / (m . m),
 * m . (u x ph) / (m . m)); density ((t * t) * (d . d)) / ((|n . d| / sqrt(d . d)) * area) * P(k).  Spheres: origin outside (d2 > r2),
 * b = oc . d > 0 and b * b - (d . d) * (d2 - r2) >= 0; the density is the expression of the sampling call, which depends on the origin
 * alone -- bit for bit the sampled pdf wherever the hit test agrees.  light[k] = the row of the nearest light met, -1 for none.
 * Nothing is drawn.
 *
 * Both calls return when the results are there (they wait on the stream), like the path steps.  Refusals, before the device is
 * touched, in this order: RT_ERR_INVALID for a NULL argument; RT_ERR_STATE before commit; RT_ERR_INVALID for a count below 0 or
 * above 2^30, a strategy other than 0 / 1, a variant other than 0 / 1, a NULL point (origin or direction) with count > 0, every
 * output NULL, and scatter_pdf or contribution asked for without both normal and material.  count == 0 returns RT_OK without a
 * launch. */
typedef struct rt_light_params {
    int64_t  count;            /* points or rays; 0 is allowed (no launch), > 2^30 is RT_ERR_INVALID */
    double   time;             /* used where the per-point array is NULL (moving spheres) */
    uint64_t seed;             /* point k: curand_init(seed, k + first_sequence, 0), unless points->rng_state is given */
    uint64_t first_sequence;
    int32_t  strategy;         /* 0 uniform over lights, 1 by area x brightest channel (rt_scene_dump_lights) */
    int32_t  variant;          /* 0 strict, 1 fast */
    int32_t  device;
    void    *stream;           /* NULL = the default stream */
    int32_t  reserved[4];
} rt_light_params;
typedef struct rt_light_points {
    const double   *point;         /* count x 3; required */
    const double   *normal;        /* count x 3, or NULL */
    const uint8_t  *material;      /* count, as rt_query_hits.material, or NULL */
    const double   *time;          /* count, or NULL */
    const uint32_t *rng_state;     /* count x 6, or NULL: seeded */
} rt_light_points;
typedef struct rt_light_samples {
    double   *direction;       /* count x 3 */
    double   *distance;        /* count */
    int32_t  *light;           /* count */
    double   *pdf;             /* count */
    double   *emitted;         /* count x 3 */
    double   *scatter_pdf;     /* count */
    double   *contribution;    /* count x 3 */
    uint32_t *rng_state;       /* count x 6; any pointer may be NULL, not all */
} rt_light_samples;
typedef struct rt_light_rays {
    const double *origin, *direction;   /* count x 3 each */
    const double *time;                 /* count, or NULL */
} rt_light_rays;
typedef struct rt_light_pdf_out {
    double  *pdf;              /* count */
    int32_t *light;            /* count; either may be NULL, not both */
} rt_light_pdf_out;
typedef struct rt_light_stats {
    uint64_t points, valid;                 /* points sampled / rays looked up; valid samples / rays that meet a light */
    double seconds;                         /* the kernel, HIP events */
    uint32_t kernel_vgprs, scratch_bytes;   /* of the kernel that ran: registers, private memory per lane */
} rt_light_stats;
/* points and out hold device pointers (on params->device).  stats may be NULL: the call is then the launch and the wait alone. */
RTOW_API int rt_scene_sample_lights_device(rt_scene *s, const rt_light_params *params, const rt_light_points *points,
                                           const rt_light_samples *out, rt_light_stats *stats);
/* the same on host arrays (uploaded, sampled, copied back) */
RTOW_API int rt_scene_sample_lights(rt_scene *s, const rt_light_params *params, const rt_light_points *points, const rt_light_samples *out,
                                    rt_light_stats *stats);
RTOW_API int rt_scene_light_pdf_device(rt_scene *s, const rt_light_params *params, const rt_light_rays *rays, const rt_light_pdf_out *out,
                                       rt_light_stats *stats);
RTOW_API int rt_scene_light_pdf(rt_scene *s, const rt_light_params *params, const rt_light_rays *rays, const rt_light_pdf_out *out,
                                rt_light_stats *stats);
/* sizeof of rt_light_params, rt_light_points, rt_light_samples, rt_light_rays, rt_light_pdf_out, rt_light_stats, rt_light_row as
 * this library was compiled, and kLightLdsRows: the rows of the light table the kernels stage on chip */
RTOW_API void rt_light_abi_sizes(uint32_t out8[8]);

/* ---- environment sampling: draw directions by the brightness of the map, and the density of doing so ----
 * The environment (rt_scene_set_environment) is no row of the light table, and direct = "mis" samples it only where the scene
 * says so (rt_scene_set_environment_light; rt_scene_path_advance_direct states the estimator): otherwise a path that misses adds
 * it with weight 1, as it adds the background.  These two calls are what that estimator is made of, for a caller's own: one lane a
 * point, the light calls' structs where the fields mean the same.  points->point is required as there (a shadow ray starts at
 * it; the sample itself does not depend on it), ->time is not read.  RT_ERR_STATE for a scene without an environment; the other
 * refusals are the light calls', without the strategy.
 *
 * rt_scene_sample_environment.  Four draws from the point's stream, each (double) curand_uniform, in this order: a, b, c, d.
 * With tables (rt_scene_dump_environment_cdf):
 *   j = the first row with marginal[j] >= a, by bisection (lo = 0, hi = H - 1; mid = (lo + hi) / 2; table[mid] >= x ? hi = mid :
 *       lo = mid + 1); i = the first column with conditional[j * W + i] >= b, likewise          -- light[k] = j * W + i
 *   u = (i + c) / W, v = 1 - (j + d) / H            -- the position inside the texel: c along the row, d down from its top edge
 *   theta = pi * v, phi = (2 pi) * u - pi, e = (sin(theta) * cos(phi), -cos(theta), -(sin(theta) * sin(phi)))
 * Without tables the sphere uniformly: y = 1 - 2 c, s = sqrt(1 - y * y), phi = (2 pi) * d - pi, e = (s * cos(phi), y,
 * -(s * sin(phi))); light[k] = -1.
 *   direction = R^T e, each row (r0 * e.x + r3 * e.y) + r6 * e.z
 * pdf and emitted are then computed FROM direction: pdf = the density below, emitted = the environment's value along it, the very
 * lookup a miss makes -- so rt_scene_environment_pdf of the direction is the sampled pdf, and a path step along it returns the
 * sampled emitted, bit for bit in the strict build.  A pdf that is not positive and finite (a pole; a texel of chance 0 reached
 * through rounding) makes the sample invalid: direction (0, 0, 0), distance 0, pdf 0, emitted, scatter_pdf, contribution 0, the
 * same four draws taken.  distance of a valid sample is +inf.  scatter_pdf and contribution = (scatter_pdf / pdf) * emitted are
 * the light calls' own.
 *
 * The density of a direction (both calls): with n, e, (u, v) and the texel (i, j) exactly as the value's lookup forms them,
 *   P(j) = marginal[j] - marginal[j - 1], P(i | j) = conditional[j * W + i] - conditional[j * W + i - 1]    (entry -1 = 0)
 *   pdf = ((P(j) * P(i | j)) * ((double)W * (double)H)) / (((2 pi) * pi) * sqrt(1 - e.y * e.y))
 * a density that is constant over a texel in (u, v), over the Jacobian of the map; without tables 1 / (4 pi).
 * rt_scene_environment_pdf: pdf[k] of rays->direction[k] (0 where it is not positive and finite), light[k] = j * W + i of its
 * texel (-1 without tables); rays->origin is required and not read.
 *
 * The kernel stages the first kEnvLdsRows entries of the marginal table in LDS; beyond the cap it reads the table from global
 * memory, with the same results. */
typedef struct rt_environment_params {
    int64_t  count;            /* points or rays; 0 is allowed (no launch), > 2^30 is RT_ERR_INVALID */
    uint64_t seed;             /* point k: curand_init(seed, k + first_sequence, 0), unless points->rng_state is given */
    uint64_t first_sequence;
    int32_t  variant;          /* 0 strict, 1 fast */
    int32_t  device;
    void    *stream;           /* NULL = the default stream */
    int32_t  reserved[4];
} rt_environment_params;
RTOW_API int rt_scene_sample_environment_device(rt_scene *s, const rt_environment_params *params, const rt_light_points *points,
                                                const rt_light_samples *out, rt_light_stats *stats);
RTOW_API int rt_scene_sample_environment(rt_scene *s, const rt_environment_params *params, const rt_light_points *points,
                                         const rt_light_samples *out, rt_light_stats *stats);
RTOW_API int rt_scene_environment_pdf_device(rt_scene *s, const rt_environment_params *params, const rt_light_rays *rays,
                                             const rt_light_pdf_out *out, rt_light_stats *stats);
RTOW_API int rt_scene_environment_pdf(rt_scene *s, const rt_environment_params *params, const rt_light_rays *rays,
                                      const rt_light_pdf_out *out, rt_light_stats *stats);
/* sizeof of rt_environment and rt_environment_params as this library was compiled, kEnvLdsRows (the entries of the marginal
 * table the sample kernel stages on chip), and 0 */
RTOW_API void rt_environment_abi_sizes(uint32_t out4[4]);

/* ---- path advances with light samples: next-event estimation and its MIS weights inside the advance ----
 * rt_scene_path_advance with the light sample, the mixture density, the shadow ray and the balance-heuristic weights of a
 * caller's loop around rt_scene_sample_lights, rt_scene_light_pdf and rt_scene_intersect done by the library, in the same call.
 * Everything rt_scene_path_advance states holds -- n, the rows read, the ids, the stable compaction, the count words, the
 * waiting (stats == NULL: enqueue and return; whatever frees the scene's device tables waits for the last call enqueued) -- with
 * these additions.  Every operation below is one IEEE-754 double operation in the order written in the strict build; the fast
 * build may fuse.
 * Row k is stepped exactly as rt_scene_path_advance steps it.  The step gives a status, emitted E, attenuation A, the scattered
 * ray (o', d', tm), the normal n, the material kind m (both as rt_query_hits) and the stream R1 after its last draw; the row
 * carries thr = throughput[3k..3k+2], its id and q = scatter_pdf[k] (0 where rays->scatter_pdf is NULL): the density with which
 * the bounce before sent the ray this way, 0 meaning "no light sample was taken there: count a lamp in full".
 *   status 0 or 1 (the path ends): w = 1, unless status is 1, m is a diffuse light (3) and q > 0: then p = the pdf of
 *     rt_scene_light_pdf for the incoming ray as given (origin, direction -- not normalised --, time, params->strategy) and
 *     w = q / (q + p).  radiance[id] = radiance[id] + (thr * E) * w; with w = 1 this is rt_scene_path_advance to the bit.
 *   status 2 (scattered): thr' = thr * A and the survivor's row as in rt_scene_path_advance.  Where m is Lambertian (0) or
 *     isotropic (4), the scene has lights and params->sample is 1:
 *       the sample of rt_scene_sample_lights for the point o', normal n, material m, time tm, from the stream R1 under
 *       params->strategy: dir, distance, contribution C, scatter_pdf s, and the stream R2 (the draws happen whether or not the
 *       sample is valid, as there).  Where C is not all zero:
 *         p = the pdf of rt_scene_light_pdf at (o', dir, tm);  w = p / (p + s), 0 where p + s == 0;  L = (thr' * C) * w
 *         the shadow ray (o', dir, tm) over (0.001, distance * (1 - 2^-20)) is searched as rt_scene_intersect mode 1 searches; a
 *         ConstantMedium draws from the path's own stream, which continues at R2.  Not occluded: radiance[id] = radiance[id] + L
 *         (where out->radiance is given and 0 <= id < sources; the search happens either way)
 *       the survivor's stream is the one after the last draw, and its density
 *         q' = scatter_pdf(m, n, u), u = (1 / sqrt((d'.x * d'.x + d'.y * d'.y) + d'.z * d'.z)) * d'
 *       with the closed form stated for rt_scene_sample_lights' scatter_pdf.
 *     In every other case (metal, glass, a scene without lights -- and without flag bit 2048, below --, sample == 0) nothing is drawn and q' = 0.
 * A row either ends or scatters: a call makes at most one addition per id, so distinct live ids still need no atomics.
 * out->scatter_pdf, row j: q' of survivor j.
 * The estimator: fresh rays start with q = 0 (rays->scatter_pdf NULL); sample = 1 in every call but the last of max_depth calls;
 * whoever is alive after the last call is dropped.  The radiance so folded has the expectation of rt_scene_radiance with samples
 * = 1 and the same max_depth: a light sample at bounce b stands for the lamp that scattering would find at bounce b + 1, which is
 * why the last call takes none.
 * A scene without lights and without flag bit 2048: rt_scene_path_advance to the bit.
 *
 * A scene whose environment is a light (RT_SCENE_FLAG_ENVIRONMENT_LIGHT, shares c_e and c_l: rt_scene_set_environment_light).
 * Everything above holds; a scene without the bit is the call above to the bit; with the bit only this differs:
 *   who samples: a row that scatters from a Lambertian or isotropic hit with sample == 1 takes a sample where the scene has
 *     lights OR the bit; q' is the closed form wherever a sample was drawn, valid or not.
 *   the pick: where c_e < 1 (so lights exist), x = (double) curand_uniform(R1), and the environment is picked where x <= c_e;
 *     where c_e == 1 nothing is drawn for the pick.
 *   the light table picked: the sample of rt_scene_sample_lights exactly as above, from the stream behind the pick's draw;
 *     C = (s / (c_l * pdf)) * emitted, all 0 where s == 0.  Where C is not all zero: p = c_l * light_pdf(o', dir, tm),
 *     w = p / (p + s), 0 where p + s == 0, L = (thr' * C) * w; the shadow ray as above.
 *   the environment picked: the sample of rt_scene_sample_environment for the point o', normal n, material m, from the stream
 *     behind the pick's draw -- four draws, valid or not --: dir, pdf, emitted, s.  C = (s / (c_e * pdf)) * emitted, all 0 for an
 *     invalid sample or s == 0.  Where C is not all zero: p = c_e * pdf, w = p / (p + s), L = (thr' * C) * w; the shadow ray is
 *     (o', dir, tm) over (0.001, fmin(inf * (1 - 2^-20), DBL_MAX)), the expression above with distance = +inf, searched as above
 *     (a medium draws from the path's stream as above); L is added where nothing is met.  No loop over the light table runs.
 *   status 0 (a miss) with q > 0: p = c_e * environment_pdf(d) for the incoming direction as given (rt_scene_environment_pdf's
 *     value: 0 where it is not positive and finite), w = q / (q + p), radiance[id] = radiance[id] + (thr * E) * w.  With q == 0,
 *     w = 1 as above.
 *   status 1 on a lamp with q > 0: p = c_l * light_pdf(...), w = q / (q + p); with c_l == 0, p = 0 and w = q / q = 1 (the table is
 *     then not consulted).
 * The weights are per emitter, not one mixture c_e p_e + c_l p_l everywhere: an environment sample along a direction that meets
 * a lamp is always occluded, so environment sampling is no technique for the lamp's light, and table sampling is none for the
 * sky's.  Under the one mixture the weights of the techniques that can produce a contribution would not sum to 1 -- at chance 1 in
 * a scene with lamps a visible bias.  So the sky's light is weighted between scattering and environment sampling, a lamp's
 * between scattering and table sampling, each technique's density scaled by the share of the samples it gets.
 * With the bit, max_depth == 1 (one call, sample = 0) is still rt_scene_radiance to the bit; the expectation is
 * rt_scene_radiance's for every max_depth.  stats->shadow_rays / shadow_reached count both kinds of shadow ray.
 *
 * Aliasing as for rt_scene_path_advance, and out->scatter_pdf may not be rays->scatter_pdf.
 * Refusals, all before the device is touched, in this order: those of rt_scene_path_advance up to the variant; a strategy other
 * than 0 / 1; a sample other than 0 / 1; the rest of rt_scene_path_advance's (the aliased pairs now include scatter_pdf; the
 * workspace is measured by rt_path_advance_direct_workspace_bytes).  count == 0 is RT_OK with nothing launched and nothing
 * written; the other parameters are still checked. */
typedef struct rt_path_advance_direct_params {
    int64_t  count;            /* as rt_path_advance_params, field for field ... */
    int64_t  sources;
    double   time;
    uint64_t seed;
    uint64_t first_sequence;
    int32_t  variant;
    int32_t  device;
    void    *stream;
    void    *workspace;        /* device call only: >= rt_path_advance_direct_workspace_bytes(count) */
    uint64_t workspace_bytes;
    int32_t  reserved[4];
    int32_t  strategy;         /* ... and: 0 uniform over lights, 1 by area x brightest channel, as rt_light_params */
    int32_t  sample;           /* 1: a light sample at every diffuse or isotropic hit of this call; 0: none (the last bounce) */
} rt_path_advance_direct_params;
typedef struct rt_path_advance_direct_rays {
    const double   *origin, *direction;   /* as rt_path_advance_rays, field for field ... */
    const double   *time;
    const uint32_t *rng_state;
    const double   *throughput;
    const int32_t  *ray_id;
    const uint8_t  *alive;
    const uint32_t *count;
    const double   *scatter_pdf;          /* ... and: count, or NULL: all 0 */
} rt_path_advance_direct_rays;
typedef struct rt_path_advance_direct_out {
    double   *radiance;        /* as rt_path_advance_out, field for field ... */
    double   *origin;
    double   *direction;
    double   *time;
    uint32_t *rng_state;
    double   *throughput;
    int32_t  *ray_id;
    double   *t;
    double   *normal;
    uint8_t  *front_face;
    uint8_t  *material;
    uint32_t *count;
    double   *scatter_pdf;     /* ... and: count; optional */
} rt_path_advance_direct_out;
typedef struct rt_path_advance_direct_stats {
    uint64_t rays, scattered;                 /* rays stepped (below n and alive); the survivors */
    uint64_t shadow_rays, shadow_reached;     /* shadow rays cast; those that reached their lamp */
    double seconds;                           /* the call's four kernels, HIP events */
    uint32_t kernel_vgprs, scratch_bytes;     /* of the step-and-sample kernel that ran: registers, private memory per lane */
    uint32_t shadow_vgprs, shadow_scratch_bytes;  /* of the shadow-ray kernel */
} rt_path_advance_direct_stats;
/* rays and out hold device pointers (on params->device), the two count words included.  stats == NULL: enqueue and return. */
RTOW_API int rt_scene_path_advance_direct_device(rt_scene *s, const rt_path_advance_direct_params *params,
                                                 const rt_path_advance_direct_rays *rays, const rt_path_advance_direct_out *out,
                                                 rt_path_advance_direct_stats *stats);
/* the same on host arrays (uploaded, advanced, waited for, copied back) */
RTOW_API int rt_scene_path_advance_direct(rt_scene *s, const rt_path_advance_direct_params *params, const rt_path_advance_direct_rays *rays,
                                          const rt_path_advance_direct_out *out, rt_path_advance_direct_stats *stats);
/* bytes of workspace a device call of capacity `count` needs: 0 for 0, non-decreasing in count, at least the plain call's */
RTOW_API uint64_t rt_path_advance_direct_workspace_bytes(int64_t count);
/* sizeof of rt_path_advance_direct_params, _rays, _out, _stats as this library was compiled */
RTOW_API void rt_path_advance_direct_abi_sizes(uint32_t out4[4]);

/* ---- radiance queries with light samples: the MIS estimator of the advances above in one call ----
 * rt_scene_radiance with every sample replaced by the estimator rt_scene_path_advance_direct states: one launch, any number of
 * samples, no workspace.  Rays, streams and outputs are rt_scene_radiance's (rt_radiance_rays and rt_radiance_out as they are).
 * Every operation below is one IEEE-754 double operation in the order written in the strict build; the fast build may fuse.
 * Sample s of ray k is the fold of rt_scene_path_advance_direct over one path: thr = (1, 1, 1), acc = (0, 0, 0), q = 0, the
 * ray as given, the stream R where the sample before left it (sample 0: the ray's stream).  At most max_depth bounces; bounce
 * b = 0, 1, ... is one row of that call with throughput thr, scatter_pdf q, params->strategy, and sample = 1 where
 * b + 1 < max_depth, sample = 0 at the last -- in this order:
 *   1. the step's draws.  A path that ends (status 0 or 1) does acc = acc + (thr * E) * w, w = q / (q + p) only where status is 1,
 *      the material is a diffuse light and q > 0 (p as stated there, along the incoming ray as given); in every other case w = 1
 *      and the term is thr * E.  The sample is over.
 *   2. status 2: thr' = thr * A.  Where the hit is Lambertian or isotropic, the scene has lights and sample is 1: the light
 *      sample's draws, and, where its contribution C is not all zero, L = (thr' * C) * w with w = p / (p + s), 0 where p + s == 0.
 *   3. the shadow ray (o', dir, tm) over (0.001, distance * (1 - 2^-20)), searched as rt_scene_intersect mode 1 searches; a
 *      ConstantMedium draws from the path's own stream.  Where the lamp is reached, acc = acc + L.
 *   4. the survivor goes on with thr', (o', d', tm), the stream after the last draw and q' as stated there (0 where no sample
 *      was drawn).  A path still alive after bounce max_depth - 1 is dropped.
 * Then sum = sum + acc (sum starts at (0, 0, 0)) and the next sample starts from the same ray with the stream where it stands.
 * Outputs as rt_scene_radiance: radiance = the mean as that call forms it; path_rays counts the path searches only (the shadow
 * searches are in the statistics); rng_state is the stream after the last draw, and may alias the input.
 * With samples == 1 the radiance is what max_depth calls of rt_scene_path_advance_direct fold for the ray, to the bit in the strict
 * build.  max_depth == 0: black, nothing searched, nothing drawn.  max_depth == 1, or a scene without lights and without flag bit 2048: rt_scene_radiance to
 * the bit in the strict build.  The expectation is rt_scene_radiance's for every max_depth.
 * Both calls return when the results are there.  Refusals, all before the device is touched: rt_scene_radiance's, in its order,
 * then a strategy other than 0 / 1.  count == 0 returns RT_OK without a launch.  Termination as for rt_scene_radiance, with at
 * most as many shadow searches as path searches. */
typedef struct rt_radiance_direct_params {
    int64_t  count;            /* as rt_radiance_params, field for field ... */
    int32_t  samples;
    int32_t  max_depth;
    double   time;
    uint64_t seed;
    uint64_t first_sequence;
    int32_t  variant;
    int32_t  device;
    void    *stream;
    int32_t  reserved[4];
    int32_t  strategy;         /* ... and: 0 uniform over lights, 1 by area x brightest channel, as rt_light_params */
    int32_t  reserved2[3];
} rt_radiance_direct_params;
typedef struct rt_radiance_direct_stats {
    uint64_t rays;                            /* the sum of path_rays: path searches */
    uint64_t shadow_rays, shadow_reached;     /* shadow rays cast; those that reached their lamp */
    double seconds;                           /* the kernel, HIP events */
    uint32_t kernel_vgprs, scratch_bytes;     /* of the instantiation that ran: registers, private memory per lane */
} rt_radiance_direct_stats;
/* rays and out hold device pointers (on params->device).  stats may be NULL: the call is then the launch and the wait alone. */
RTOW_API int rt_scene_radiance_direct_device(rt_scene *s, const rt_radiance_direct_params *params, const rt_radiance_rays *rays,
                                             const rt_radiance_out *out, rt_radiance_direct_stats *stats);
/* the same on host arrays (uploaded, traced, copied back) */
RTOW_API int rt_scene_radiance_direct(rt_scene *s, const rt_radiance_direct_params *params, const rt_radiance_rays *rays,
                                      const rt_radiance_out *out, rt_radiance_direct_stats *stats);
/* sizeof of rt_radiance_direct_params, rt_radiance_rays, rt_radiance_out, rt_radiance_direct_stats as this library was compiled */
RTOW_API void rt_radiance_direct_abi_sizes(uint32_t out4[4]);

/* ---- frames with light samples: a film rendered by the estimator of rt_scene_radiance_direct ----
 * rt_render_launch with every sample of every pixel replaced by one sample of rt_scene_radiance_direct.  Take the film of W x H,
 * params with seed, S = samples_per_pixel and max_depth, and direct->strategy.  Pixel (i, j), owned by the film's rank through the
 * usual stripes, has the film's saved stream under RT_FLAG_KEEP_RNG_STATE and curand_init(seed, j * W + i, 0) otherwise, as for
 * rt_render_launch.  For s = 0 .. S - 1, in this order:
 *   1. the camera ray of the render kernels for (i, j) (their own draws and operations);
 *   2. one sample of rt_scene_radiance_direct for that ray -- samples = 1, this max_depth and strategy, steps 1-4 of the comment
 *      above rt_radiance_direct_params -- drawn from the stream where step 1 left it; the stream moves on as that call moves it;
 *   3. col = col + acc, where col starts at (0, 0, 0), or at the film's running sum under RT_FLAG_ACCUMULATE on a continued frame.
 * The pixel is then finished as rt_render_launch finishes it: the six stream words go to the film's state, col to the running sum
 * where the frame accumulates, pixels = sqrt(col / (double)N) with N all samples of the frame so far.  With adaptive sampling set
 * on the film (rt_film_set_adaptive) the pixel is finished by that rule instead, exactly as rt_render_launch applies it: q takes
 * the sample's y^2 after each sample, the rule is looked at with the pixel's total n, a pixel that stops keeps its own n and is
 * marked, and a marked pixel is never touched by a later launch of the frame.  In the strict build every operation is one IEEE-754
 * double operation in that order; the fast build may fuse (never inside the rule).
 * Consequences: without lights and without flag bit 2048, or at max_depth == 1, the frame is rt_render_launch's bit for bit in the strict build;
 * max_depth == 0 gives a black frame with only the camera's draws taken; k launches of S with KEEP_RNG_STATE | ACCUMULATE are one
 * launch of kS; a frame may mix plain and direct launches (the sums and streams are the same objects, both estimators have the
 * same expectation; the changed-adaptive-setting rule applies as it does to rt_render_launch).  No frame depends on which lane
 * rendered which pixel.
 * S == 0 is accepted and finishes no pixel: the launch does what every launch does before its kernel (it seeds the streams where
 * it does not keep them, and begins a frame where it does not continue one) and runs no kernel, so no pixel and no running sum is
 * written (rt_render_launch would write every pixel again from a sum of no samples), and rt_render_finish reports no samples, no
 * rays and no shadow rays.
 * rt_render_finish ends the launch and fills rt_render_stats as for any launch: rays counts the path searches only (the shadow
 * searches are in rt_film_last_direct_stats), pixels_per_wave is 64, kernel_kind carries the bit 1024 beside the bits of the
 * nested kernel whose search runs.  variant, device, stream, stripe_rows / rank / world_size, RT_FLAG_KEEP_RNG_STATE and
 * RT_FLAG_ACCUMULATE mean what they mean for rt_render_launch; max_blocks_per_cu caps the resident workgroups; every other
 * RT_FLAG_* scheduling or tuning bit and every other tuning field is accepted and ignored (none changes a picture).
 * Refusals, all before the device is touched: rt_render_launch's own, in its order; then a NULL direct, a strategy other than
 * 0 / 1, a non-zero reserved word (RT_ERR_INVALID, the message names the field). */
typedef struct rt_film_direct_params {
    int32_t strategy;        /* 0 uniform over lights, 1 by area x brightest channel, as rt_light_params */
    int32_t reserved[7];     /* must be 0 */
} rt_film_direct_params;
typedef struct rt_film_direct_stats {
    uint64_t shadow_rays, shadow_reached;   /* of the last direct launch that was finished: shadow rays cast; those that reached their lamp */
    uint32_t scratch_bytes, reserved;       /* private memory per lane of the kernel that ran */
} rt_film_direct_stats;
RTOW_API int rt_render_launch_direct(rt_scene *s, rt_film *film, const rt_render_params *params, const rt_film_direct_params *direct);
/* RT_ERR_STATE before a direct launch of this film was finished */
RTOW_API int rt_film_last_direct_stats(rt_film *film, rt_film_direct_stats *out);
/* sizeof of rt_film_direct_params, rt_film_direct_stats as this library was compiled */
RTOW_API void rt_film_direct_abi_sizes(uint32_t out2[2]);

/* Convenience: create film, upload, render 1 GPU, download.  frame = W*H*3 doubles. */
RTOW_API int rt_render(rt_scene *s, const rt_render_params *params, double *frame, rt_render_stats *stats);

/* Extra outputs: binary PPM (P6, same quantisation as the P3 writer) and PFM (little-endian float32, the
 * gamma-corrected values unclamped, bottom row first as PFM prescribes). */
RTOW_API int rt_write_ppm_binary(const char *path, const double *frame, int width, int height);
RTOW_API int rt_write_pfm(const char *path, const double *frame, int width, int height);

/* PPM writer, byte-for-byte the reference's (R/kernel.cu:696-721): P3, rows from j=H-1 down, clamp [0,0.999], int(256*c). */
RTOW_API int rt_write_ppm(const char *path, const double *frame, int width, int height);

#ifdef __cplusplus
}
#endif
#endif /* RTOW_H */
