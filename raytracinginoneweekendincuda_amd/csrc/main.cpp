// rtow -- thin host executable over the C-ABI; the MI355X counterpart of the reference's main()
// (R/kernel.cu:570-742): same defaults (1440x720, sceneId 9, spp rule, seed 1984, depth 50), same
// stderr lines, same output.ppm, exit code 99 on a device error.
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include <hip/hip_runtime_api.h>
#include <rccl/rccl.h>

#include "../../include/rtow.h"

// Multi-GPU frame: rows dealt to the N GPUs of the node in 8-row stripes (rank = stripe % N), every GPU renders its
// stripes into a compact buffer, ONE ncclGather over xGMI brings them to GPU 0, the host de-interleaves.
// Single process, one HIP stream and one RCCL communicator per device.
// --denoise / --aov-prefix with --gpus: every rank runs the feature pass on its stripes and the three planes are gathered like
// the pixels (same staging buffers, same communicators), then scattered into full frames on the host.
struct FeatureRequest {
    int samples;
    std::vector<double> albedo, normal, depth;  // full frames: W*H*3, W*H*3, W*H
};

static int render_multi_gpu(rt_scene *scene, rt_render_params base, int n_gpus, double *frame, rt_render_stats *total,
                            double *gather_seconds, FeatureRequest *features = nullptr)
{
    const int W = base.width, H = base.height, stripe = 8;
    int rows_max = 0;
    for (int r = 0; r < n_gpus; r++) {
        int n = rt_stripe_rows(H, stripe, r, n_gpus, nullptr, 0);
        if (n > rows_max) rows_max = n;
    }
    const size_t count = (size_t)rows_max * W * 3;  // doubles per rank
    std::vector<rt_film *> films(n_gpus, nullptr);
    std::vector<double *> send(n_gpus, nullptr);
    std::vector<hipStream_t> streams(n_gpus, nullptr);
    std::vector<ncclComm_t> comms(n_gpus);
    std::vector<int> devs(n_gpus);
    double *recv = nullptr;
    auto hip_ok = [](hipError_t e, const char *what) {
        if (e != hipSuccess) {
            std::fprintf(stderr, "HIP error = %u at '%s'\n", (unsigned)e, what);
            std::exit(99);
        }
    };
    auto nccl_ok = [](ncclResult_t r, const char *what) {
        if (r != ncclSuccess) {
            std::fprintf(stderr, "RCCL error = %d (%s) at '%s'\n", (int)r, ncclGetErrorString(r), what);
            std::exit(99);
        }
    };
    for (int r = 0; r < n_gpus; r++) {
        devs[r] = r;
        hip_ok(hipSetDevice(r), "hipSetDevice");
        hip_ok(hipStreamCreateWithFlags(&streams[r], hipStreamNonBlocking), "hipStreamCreate");
        hip_ok(hipMalloc((void **)&send[r], count * sizeof(double)), "hipMalloc(send)");
        hip_ok(hipMemsetAsync(send[r], 0, count * sizeof(double), streams[r]), "hipMemsetAsync");
        films[r] = rt_film_create(r, W, H, stripe, r, n_gpus);
        if (!films[r] || rt_film_bind_pixels(films[r], send[r]) != RT_OK) return 1;
        if (rt_scene_upload(scene, r) != RT_OK) return 1;
    }
    hip_ok(hipSetDevice(0), "hipSetDevice(0)");
    hip_ok(hipMalloc((void **)&recv, count * n_gpus * sizeof(double)), "hipMalloc(recv)");
    nccl_ok(ncclCommInitAll(comms.data(), n_gpus, devs.data()), "ncclCommInitAll");

    for (int r = 0; r < n_gpus; r++) {  // all GPUs render concurrently
        rt_render_params p = base;
        p.device = r;
        p.rank = r;
        p.world_size = n_gpus;
        p.stripe_rows = stripe;
        p.stream = streams[r];
        if (rt_render_launch(scene, films[r], &p) != RT_OK) return 1;
    }
    auto t0 = std::chrono::steady_clock::now();
    nccl_ok(ncclGroupStart(), "ncclGroupStart");
    for (int r = 0; r < n_gpus; r++)
        nccl_ok(ncclGather(send[r], r == 0 ? recv : nullptr, count, ncclDouble, 0, comms[r], streams[r]), "ncclGather");
    nccl_ok(ncclGroupEnd(), "ncclGroupEnd");
    std::memset(total, 0, sizeof *total);
    for (int r = 0; r < n_gpus; r++) {
        rt_render_stats st{};
        if (rt_render_finish(scene, films[r], &st) != RT_OK) return 1;
        hip_ok(hipSetDevice(r), "hipSetDevice");
        hip_ok(hipStreamSynchronize(streams[r]), "hipStreamSynchronize");
        total->samples += st.samples;
        total->rays += st.rays;
        if (st.seconds_render + st.seconds_seed > total->seconds_render) total->seconds_render = st.seconds_render + st.seconds_seed;
        total->kernel_vgprs = st.kernel_vgprs;
        total->lds_bytes = st.lds_bytes;
        total->kernel_kind = st.kernel_kind;
    }
    *gather_seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    std::vector<double> gathered(count * n_gpus);
    hip_ok(hipSetDevice(0), "hipSetDevice(0)");
    hip_ok(hipMemcpy(gathered.data(), recv, gathered.size() * sizeof(double), hipMemcpyDeviceToHost), "hipMemcpy(D2H)");
    int rc = rt_deinterleave(gathered.data(), W, H, stripe, n_gpus, count, frame);
    if (rc == RT_OK && features) {
        rt_feature_params fp{};
        fp.width = W;
        fp.height = H;
        fp.samples = features->samples;
        fp.seed = base.seed;
        fp.variant = base.variant;
        for (int r = 0; r < n_gpus; r++) {
            fp.stream = streams[r];
            if (rt_film_render_features(scene, films[r], &fp) != RT_OK) return 1;
        }
        std::vector<double> *planes[3] = {&features->albedo, &features->normal, &features->depth};
        for (int which = 0; which < 3; which++) {
            const int channels = which == 2 ? 1 : 3;
            const size_t plane_count = (size_t)rows_max * W * channels;  // doubles per rank (the pixels' staging buffers hold 3 per pixel)
            for (int r = 0; r < n_gpus; r++) {
                const size_t owned = (size_t)rt_stripe_rows(H, stripe, r, n_gpus, nullptr, 0) * W * channels;
                hip_ok(hipSetDevice(r), "hipSetDevice");
                hip_ok(hipMemcpyAsync(send[r], rt_film_device_features(films[r], which), owned * sizeof(double), hipMemcpyDeviceToDevice, streams[r]),
                       "hipMemcpyAsync(feature plane)");
            }
            nccl_ok(ncclGroupStart(), "ncclGroupStart");
            for (int r = 0; r < n_gpus; r++)
                nccl_ok(ncclGather(send[r], r == 0 ? recv : nullptr, plane_count, ncclDouble, 0, comms[r], streams[r]), "ncclGather(features)");
            nccl_ok(ncclGroupEnd(), "ncclGroupEnd");
            for (int r = 0; r < n_gpus; r++) {
                hip_ok(hipSetDevice(r), "hipSetDevice");
                hip_ok(hipStreamSynchronize(streams[r]), "hipStreamSynchronize");
            }
            hip_ok(hipSetDevice(0), "hipSetDevice(0)");
            hip_ok(hipMemcpy(gathered.data(), recv, plane_count * n_gpus * sizeof(double), hipMemcpyDeviceToHost), "hipMemcpy(D2H)");
            planes[which]->assign((size_t)W * H * channels, 0.0);
            std::vector<int> rows((size_t)rows_max);
            for (int r = 0; r < n_gpus; r++) {
                const int n = rt_stripe_rows(H, stripe, r, n_gpus, rows.data(), rows_max);
                for (int lr = 0; lr < n; lr++)
                    std::memcpy(planes[which]->data() + (size_t)rows[lr] * W * channels, gathered.data() + (size_t)r * plane_count + (size_t)lr * W * channels,
                                sizeof(double) * (size_t)W * channels);
            }
        }
    }
    for (int r = 0; r < n_gpus; r++) {
        hipSetDevice(r);
        ncclCommDestroy(comms[r]);
        rt_film_destroy(films[r]);
        hipFree(send[r]);
        hipStreamDestroy(streams[r]);
    }
    hipSetDevice(0);
    hipFree(recv);
    return rc;
}

// Binary PPM (P6, maxval 255) -> RGB bytes, row 0 = top: the layout RtwImage hands to ImageTexture (R/RtwImage.h:51-92).
static bool read_p6(const std::string &path, std::vector<unsigned char> &rgb, int &w, int &h)
{
    FILE *fp = std::fopen(path.c_str(), "rb");
    if (!fp) return false;
    auto token = [&](char *buf, size_t cap) {  // header tokens, '#' comments skipped
        size_t n = 0;
        int c = std::fgetc(fp);
        while (c != EOF) {
            if (c == '#') {
                while (c != EOF && c != '\n') c = std::fgetc(fp);
            } else if (c == ' ' || c == '\t' || c == '\n' || c == '\r') {
                c = std::fgetc(fp);
            } else {
                break;
            }
        }
        while (c != EOF && !(c == ' ' || c == '\t' || c == '\n' || c == '\r') && n + 1 < cap) {
            buf[n++] = (char)c;
            c = std::fgetc(fp);
        }
        buf[n] = 0;
        return n > 0;
    };
    char magic[8], sw[16], sh[16], smax[16];
    bool ok = token(magic, sizeof magic) && std::strcmp(magic, "P6") == 0 && token(sw, sizeof sw) && token(sh, sizeof sh) &&
              token(smax, sizeof smax) && std::atoi(smax) == 255;
    if (ok) {
        w = std::atoi(sw);
        h = std::atoi(sh);
        ok = w > 0 && h > 0 && (long long)w * h < (1ll << 28);
    }
    if (ok) {
        rgb.resize((size_t)w * h * 3);
        ok = std::fread(rgb.data(), 1, rgb.size(), fp) == rgb.size();
    }
    std::fclose(fp);
    return ok;
}

static int die(const char *what)
{
    std::fprintf(stderr, "%s: %s\n", what, rt_last_error());
    return 99;  // R/kernel.cu:29-40: checkCudaErrors -> exit(99)
}

int main(int argc, char **argv)
{
    int width = 1440, height = 720, scene_id = 9, spp = -1, depth = 50, world_kind = 0, variant = 1, device = 0, gpus = 0;
    unsigned long long seed = 1984;
    unsigned flags = 0;          // RT_FLAG_* bits (schedulers and the opt-in list acceleration; none changes the picture)
    std::string out = "output.ppm";
    std::string environment_path;  // --environment: a .pfm float image or a JPEG, the sky of any scene
    double environment_intensity = 1.0, environment_rotate_y = 0.0;
    double environment_light = 0.0;  // --environment-light C: --direct mis samples the sky as a light with chance C (rt_scene_set_environment_light)
    bool environment_light_given = false;
    std::string earth_path;      // decoded 8-bit sRGB pixels of the earth texture (P6): converted like RtwImage::Load does
    bool earth_is_bytes = false; // --earth-bytes: the file already holds what RtwImage::Load hands to ImageTexture
    // adaptive sampling (--noise): a pixel stops once its noise is below the threshold, --spp is then the most it takes
    double noise = -1.0;
    int min_spp = 16, check_every = 16;
    std::string samples_map;     // --samples-map: the samples every pixel took, as a 16-bit PGM
    bool noise_given = false, adaptive_option = false;  // --noise seen; an option that only means something with it seen
    // first-hit feature buffers and the a-trous filter (--denoise, --aov-prefix)
    bool denoise = false, denoise_option = false;  // --denoise seen; an option that only means something with it seen
    rt_denoise_params dp{5, 0.6, 0.1, 0.3, 0.1};   // the library's defaults
    int feature_samples = 0;
    bool feature_samples_given = false;
    std::string raw_output, aov_prefix;
    bool pick = false;           // --pick i,j: what the centre ray of that pixel hits, one line, no render
    int pick_i = 0, pick_j = 0;
    bool radiance_at = false;    // --radiance-at i,j: the light that comes back along the centre ray of that pixel, one line, no render
    bool trace_at = false;       // --trace-at i,j: that path vertex by vertex (rt_scene_path_step), then --radiance-at's line
    bool direct_mis = false;     // --direct mis: the MIS estimator with light samples, for --radiance-at's samples (rt_scene_radiance_direct) or, without it, for the frame (rt_render_launch_direct)
    bool list_lights = false;    // --lights: the scene's light table (rt_scene_dump_lights), a line per light, no render
    for (int k = 1; k < argc; k++) {
        std::string a = argv[k];
        auto val = [&](const char *name) -> const char * {
            if (a == name && k + 1 < argc) return argv[++k];
            return nullptr;
        };
        if (const char *v = val("--width")) width = std::atoi(v);
        else if (const char *v = val("--height")) height = std::atoi(v);
        else if (const char *v = val("--scene")) scene_id = std::atoi(v);
        else if (const char *v = val("--spp")) spp = std::atoi(v);
        else if (const char *v = val("--depth")) depth = std::atoi(v);
        else if (const char *v = val("--seed")) seed = std::strtoull(v, nullptr, 10);
        else if (const char *v = val("--world")) world_kind = std::strcmp(v, "list") == 0 ? 1 : 0;
        else if (const char *v = val("--variant")) variant = std::strcmp(v, "strict") == 0 ? 0 : 1;
        else if (const char *v = val("--device")) device = std::atoi(v);
        else if (const char *v = val("--gpus")) gpus = std::atoi(v);  // >= 1: stripe the frame over that many GPUs + one RCCL gather
        else if (const char *v = val("--flags")) flags = (unsigned)std::strtoul(v, nullptr, 0);
        else if (a == "--accelerate-lists") flags |= RT_FLAG_ACCELERATE_LISTS;
        else if (const char *v = val("--output")) out = v;
        else if (const char *v = val("--noise")) {
            char *end = nullptr;
            noise = std::strtod(v, &end);
            noise_given = true;
            if (end == v || *end != 0 || !std::isfinite(noise) || noise < 0.0) {
                std::fprintf(stderr, "--noise needs a finite number >= 0, not '%s'\n", v);
                return 2;
            }
        } else if (const char *v = val("--min-spp")) {
            min_spp = std::atoi(v);
            adaptive_option = true;
        } else if (const char *v = val("--check-every")) {
            check_every = std::atoi(v);
            adaptive_option = true;
        } else if (const char *v = val("--samples-map")) {
            samples_map = v;
            adaptive_option = true;
        }
        else if (a == "--denoise") denoise = true;
        else if (a == "--lights") list_lights = true;
        else if (const char *v = val("--denoise-iterations")) {
            dp.iterations = std::atoi(v);
            denoise_option = true;
        } else if (const char *v = val("--denoise-sigmas")) {
            if (std::sscanf(v, "%lf,%lf,%lf,%lf", &dp.sigma_color, &dp.sigma_albedo, &dp.sigma_normal, &dp.sigma_depth) != 4) {
                std::fprintf(stderr, "--denoise-sigmas needs four numbers c,a,n,z (inf switches a term off), not '%s'\n", v);
                return 2;
            }
            denoise_option = true;
        } else if (const char *v = val("--raw-output")) {
            raw_output = v;
            denoise_option = true;
        } else if (const char *v = val("--feature-samples")) {
            feature_samples = std::atoi(v);
            feature_samples_given = true;
        } else if (const char *v = val("--aov-prefix")) aov_prefix = v;
        else if (const char *v = val("--pick")) {
            if (std::sscanf(v, "%d,%d", &pick_i, &pick_j) != 2) {
                std::fprintf(stderr, "--pick needs a pixel i,j, not '%s'\n", v);
                return 2;
            }
            pick = true;
        } else if (const char *v = val("--radiance-at")) {
            if (std::sscanf(v, "%d,%d", &pick_i, &pick_j) != 2) {
                std::fprintf(stderr, "--radiance-at needs a pixel i,j, not '%s'\n", v);
                return 2;
            }
            pick = radiance_at = true;
        } else if (const char *v = val("--trace-at")) {
            if (std::sscanf(v, "%d,%d", &pick_i, &pick_j) != 2) {
                std::fprintf(stderr, "--trace-at needs a pixel i,j, not '%s'\n", v);
                return 2;
            }
            pick = radiance_at = trace_at = true;
        }
        else if (const char *v = val("--direct")) {
            if (std::strcmp(v, "mis") != 0) {
                std::fprintf(stderr, "--direct needs 'mis', not '%s'\n", v);
                return 2;
            }
            direct_mis = true;
        }
        else if (const char *v = val("--environment-light")) {  // (before the prefix match of --environment)
            char *end = nullptr;
            environment_light = std::strtod(v, &end);
            if (end == v || *end != '\0') {
                std::fprintf(stderr, "--environment-light needs a number in [0, 1], not '%s'\n", v);
                return 2;
            }
            environment_light_given = true;
        }
        else if (const char *v = val("--environment-intensity")) environment_intensity = std::atof(v);
        else if (const char *v = val("--environment-rotate-y")) environment_rotate_y = std::atof(v);
        else if (const char *v = val("--environment")) environment_path = v;
        else if (const char *v = val("--earth")) earth_path = v;
        else if (const char *v = val("--earth-bytes")) {
            earth_path = v;
            earth_is_bytes = true;
        } else {
            std::fprintf(stderr,
                         "usage: rtow [--scene 0..15] [--width W] [--height H] [--spp N] [--depth D] [--seed S]\n"
                         "            [--world bvh|list] [--variant strict|fast] [--device N] [--gpus N] [--output file.ppm]\n"
                         "            [--earth earthmap.jpg|decoded.ppm | --earth-bytes texture.ppm] [--accelerate-lists] [--flags N]\n"
                         "            [--noise T [--min-spp N] [--check-every K] [--samples-map file.pgm]]\n"
                         "            [--denoise [--denoise-iterations N] [--denoise-sigmas c,a,n,z] [--raw-output file.ppm]]\n"
                         "            [--aov-prefix P] [--feature-samples N] [--pick i,j] [--radiance-at i,j] [--trace-at i,j] [--lights] [--direct mis]\n"
                         "            [--environment sky.pfm|sky.jpg] [--environment-intensity X] [--environment-rotate-y DEG] [--environment-light C]\n"
                         "  --environment  what a ray that leaves the scene sees, in place of the scene's background colour: a .pfm file is a linear\n"
                         "                 float image (an HDR panorama, top row = up), any other file is read as --earth reads a JPEG, as an 8-bit\n"
                         "                 image texture; --environment-intensity multiplies it, --environment-rotate-y turns it about the vertical.\n"
                         "                 Scene 15 brings a computed sky along (the two options adjust that one too)\n"
                         "  --lights       render nothing: print the light table (rt_scene_dump_lights), a line per emissive primitive in world space --\n"
                         "                 kind, world leaf, material row, geometry, and its entries of the two cumulative selection tables\n"
                         "  --pick         render nothing: print what the ray through the centre of pixel (i, j) hits (j = 0 is the bottom row) --\n"
                         "                 leaf, material kind, t, point, normal, albedo -- at the shutter's opening, over [0.001, inf)\n"
                         "  --radiance-at  render nothing: path-trace the same ray, --spp samples (default 1) of --depth bounces from the pixel's stream,\n"
                         "                 and print the linear radiance, the rays traced and the kernel's time\n"
                         "  --environment-light C  with --direct mis: the environment is a light too -- a light sample goes to it with chance C, to the\n"
                         "                 lamps otherwise (to it alone in a scene without lamps); C in [0, 1], 0 = off (rt_scene_set_environment_light)\n"
                         "  --direct mis   every sample takes a light sample at each diffuse hit and weights it against the lamps scattering finds.\n"
                         "                 With --radiance-at (rt_scene_radiance_direct): the line then ends with the shadow rays cast and those that\n"
                         "                 reached their lamp.  Without it the frame is rendered that way (rt_render_launch_direct, lights picked by area\n"
                         "                 and brightness), with --noise, --denoise, --aov-prefix, --samples-map and --output as for any frame.  One GPU\n"
                         "                 (no --gpus)\n"
                         "  --trace-at     render nothing: the same paths one bounce at a time (rt_scene_path_step), a line per vertex -- sample, depth,\n"
                         "                 status (0 miss, 1 the path ends, 2 scattered), t, material, emitted, attenuation -- folded here, on the host;\n"
                         "                 the last line is --radiance-at's (to the last bit with --variant strict; its time is the steps' kernels')\n"
                         "  --denoise      --output gets the frame after the edge-avoiding a-trous filter (1..8 levels, default 5; sigmas of the colour,\n"
                         "                 albedo, normal and depth edge stops, inf = off), guided by the first hits' albedo, normal and depth;\n"
                         "                 --raw-output: the unfiltered frame beside it\n"
                         "  --aov-prefix   write those three buffers as P_albedo.pfm, P_normal.pfm and P_depth.pfm (depth in all three channels)\n"
                         "  --feature-samples  primary rays per pixel for the buffers, drawn as the render draws them (default 0: one ray through\n"
                         "                 the pixel centre)\n"
                         "  --noise        adaptive sampling: a pixel stops at the first check (after --min-spp samples, default 16, then every\n"
                         "                 --check-every, default 16) where the standard error of its mean is at most T x max(mean, 0.01);\n"
                         "                 --spp is then the most samples a pixel takes.  Use T >= 0.001.  One GPU (no --gpus)\n"
                         "  --samples-map  with --noise: the samples every pixel took as a binary PGM (P5, 16 bit, clamped to 65535; rows top\n"
                         "                 first like the PPM)\n"
                         "  --earth        the texture of scenes 2 and 9: a JPEG file (default: ./earthmap.jpg, like the reference) is read as\n"
                         "                 RtwImage::Load reads it -- decoded as the reference's stb_image decodes it, bit for bit; a binary PPM\n"
                         "                 (P6) is taken as pixels some other decoder produced (libjpeg's differ from stb's in ~0.6 %% of the\n"
                         "                 bytes: near-identical texture, parity unpinned) and is linearised and re-quantised the same way\n"
                         "  --earth-bytes  binary PPM (P6) that already holds the bytes RtwImage::Load hands to ImageTexture; with the\n"
                         "                 bytes the reference's own stb_image build decodes (tests/golden/earthmap_stb.npz, written out\n"
                         "                 by tests/golden/make_earth_golden.py) this is the only input that reproduces the reference's\n"
                         "                 texture bit for bit\n"
                         "  --accelerate-lists  render a list world of primitives through the library's tree (same picture, faster)\n"
                         "  --flags        RT_FLAG_* bits of include/rtow.h (none of them changes the picture)\n");
            return 2;
        }
    }
    const bool adaptive = noise_given;
    if (!adaptive && adaptive_option) {
        std::fprintf(stderr, "--min-spp, --check-every and --samples-map need --noise\n");
        return 2;
    }
    if (adaptive && gpus >= 1) {
        std::fprintf(stderr, "--noise renders on one GPU (no --gpus)\n");
        return 2;
    }
    const bool wants_features = denoise || !aov_prefix.empty();
    if (!denoise && denoise_option) {
        std::fprintf(stderr, "--denoise-iterations, --denoise-sigmas and --raw-output need --denoise\n");
        return 2;
    }
    if (!wants_features && feature_samples_given) {
        std::fprintf(stderr, "--feature-samples needs --denoise or --aov-prefix\n");
        return 2;
    }
    if (feature_samples < 0 || dp.iterations < 1 || dp.iterations > 8 || !(dp.sigma_color > 0) || !(dp.sigma_albedo > 0) || !(dp.sigma_normal > 0) ||
        !(dp.sigma_depth > 0)) {
        std::fprintf(stderr, "--feature-samples needs N >= 0, --denoise-iterations 1..8, --denoise-sigmas four numbers > 0\n");
        return 2;
    }
    if (radiance_at && spp < 0) spp = 1;
    if (direct_mis && (trace_at || list_lights || (pick && !radiance_at))) {
        std::fprintf(stderr, "--direct goes with --radiance-at, or with a frame: not with --pick, --trace-at or --lights\n");
        return 2;
    }
    if (environment_light_given && !direct_mis) {
        std::fprintf(stderr, "--environment-light goes with --direct mis: no other estimator samples the sky\n");
        return 2;
    }
    if (environment_light_given && !(environment_light >= 0.0 && environment_light <= 1.0)) {
        std::fprintf(stderr, "--environment-light needs a chance in [0, 1]\n");
        return 2;
    }
    const bool direct_frame = direct_mis && !pick;  // the frame itself by the MIS estimator (rt_render_launch_direct)
    if (direct_frame && gpus >= 1) {
        std::fprintf(stderr, "--direct renders its frame on one GPU (no --gpus)\n");
        return 2;
    }
    if (trace_at && (spp < 1 || depth < 0)) {  // (what rt_scene_radiance refuses for --radiance-at)
        std::fprintf(stderr, "--trace-at needs --spp >= 1 and --depth >= 0\n");
        return 2;
    }
    if (spp < 0) spp = (scene_id == 9) ? 100 : (((scene_id >= 5 && scene_id <= 8) || (scene_id >= 12 && scene_id <= 14)) ? 200 : (scene_id == 15 ? 100 : 10));  // R/kernel.cu:593 (12 .. 14: lit like 7; 15: lit by its sun)

    if (pick && (pick_i < 0 || pick_i >= width || pick_j < 0 || pick_j >= height)) {
        std::fprintf(stderr, "%s: pixel (%d, %d) is outside the %dx%d frame\n", trace_at ? "--trace-at" : radiance_at ? "--radiance-at" : "--pick", pick_i, pick_j, width, height);
        return 2;
    }
    if (!pick && !list_lights) std::fprintf(stderr, "Rendering a %dx%d image with %d samples per pixel in 8x8 blocks.\n", width, height, spp);
    rt_scene *scene = rt_scene_create();
    // R/kernel.cu:656-665: scenes 2 and 9 load earthmap.jpg through stb_image.  This executable carries no JPEG decoder:
    // the decoded pixels come in as a PPM (--earth / --earth-bytes; ./earthmap.ppm is picked up like the reference picks
    // up ./earthmap.jpg).  Without one the sphere shows the reference's own fallback for a missing file, cyan
    // (R/Texture.h:113-114) -- and the picture then differs from the reference's, which ships the file.
    std::vector<unsigned char> earth;
    int earth_w = 0, earth_h = 0;
    if (scene_id == 2 || scene_id == 9) {
        if (earth_path.empty()) {  // R/kernel.cu:661: RtwImage::Load("earthmap.jpg") from the working directory
            for (const char *name : {"earthmap.jpg", "earthmap.ppm"})
                if (FILE *probe = std::fopen(name, "rb")) {
                    std::fclose(probe);
                    earth_path = name;
                    break;
                }
        }
        const bool is_jpeg = earth_path.size() > 4 && (earth_path.rfind(".jpg") == earth_path.size() - 4 || earth_path.rfind(".jpeg") == earth_path.size() - 5 ||
                                                       earth_path.rfind(".JPG") == earth_path.size() - 4);
        if (earth_path.empty()) {
            std::fprintf(stderr, "ERROR: Could not load image file 'earthmap.jpg'.\n");  // R/RtwImage.h:57; the texture renders cyan (R/Texture.h:113-114)
        } else if (is_jpeg) {
            // the whole of RtwImage::Load (JPEG decode as the reference's stb_image does it, linearisation, FloatToByte)
            unsigned char *bytes = nullptr;
            if (rt_rtwimage_load(earth_path.c_str(), &bytes, &earth_w, &earth_h) != RT_OK) {
                std::fprintf(stderr, "ERROR: Could not load image file '%s' (%s).\n", earth_path.c_str(), rt_last_error());
                earth_w = earth_h = 0;
            } else {
                earth.assign(bytes, bytes + (size_t)earth_w * earth_h * 3);
                rt_image_free(bytes);
                std::fprintf(stderr, "Loaded image '%s' (%dx%d) and uploaded to device.\n", earth_path.c_str(), earth_w, earth_h);
            }
        } else if (!read_p6(earth_path, earth, earth_w, earth_h)) {
            std::fprintf(stderr, "ERROR: Could not load image file '%s'.\n", earth_path.c_str());
            earth.clear();
            earth_w = earth_h = 0;
        } else {
            if (!earth_is_bytes) rt_rtwimage_bytes(earth.data(), earth.size(), earth.data());
            std::fprintf(stderr, "Loaded image '%s' (%dx%d) and uploaded to device.\n", earth_path.c_str(), earth_w, earth_h);
        }
    }
    if (scene_id == 15) {  // the environment's demonstration: a scene of its own call, not a builtin id
        if (rt_scene_build_sky_demo(scene, world_kind, width, height, seed) != RT_OK) return die("scene");
    } else if (rt_scene_build_builtin(scene, scene_id, world_kind, width, height, seed, earth.empty() ? nullptr : earth.data(), earth_w,
                                      earth_h) != RT_OK)
        return die("scene");

    // --environment FILE: a sky for any scene (.pfm: a linear float image; anything else goes through RtwImage::Load as an 8-bit image
    // texture); --environment-intensity and --environment-rotate-y also adjust the sky a scene brings along (scene 15)
    if (!environment_path.empty() || environment_intensity != 1.0 || environment_rotate_y != 0.0) {
        rt_environment env{};
        float *pfm = nullptr;
        if (environment_path.empty()) {
            if (rt_scene_get_environment(scene, &env, nullptr) != RT_OK) return die("environment");
            if (!env.texture && !env.rgb) {
                std::fprintf(stderr, "--environment-intensity / --environment-rotate-y: the scene has no environment (--environment FILE, or --scene 15)\n");
                return 1;
            }
        } else if (environment_path.size() > 4 && environment_path.rfind(".pfm") == environment_path.size() - 4) {
            if (rt_pfm_load(environment_path.c_str(), &pfm, &env.width, &env.height) != RT_OK) return die("environment");
            env.rgb = pfm;
        } else {
            unsigned char *bytes = nullptr;
            int w = 0, h = 0;
            if (rt_rtwimage_load(environment_path.c_str(), &bytes, &w, &h) != RT_OK) return die("environment");
            env.texture = rt_image_texture(scene, bytes, w, h);
            rt_image_free(bytes);
            if (!env.texture) return die("environment");
        }
        const double radians = environment_rotate_y * 3.1415926535897932385 / 180.0, cs = std::cos(radians), sn = std::sin(radians);
        const double about_y[9] = {cs, 0.0, -sn, 0.0, 1.0, 0.0, sn, 0.0, cs};
        for (int k = 0; k < 3; k++) env.intensity[k] = environment_intensity;
        for (int k = 0; k < 9; k++) env.rotation[k] = about_y[k];
        const int rc = rt_scene_set_environment(scene, &env);  // (copies the image)
        rt_pfm_free(pfm);
        if (rc != RT_OK || rt_scene_commit(scene) != RT_OK) return die("environment");
    }

    if (environment_light_given) {  // --environment-light C: the sky as a light of --direct mis
        if (!(rt_scene_flags(scene) & RT_SCENE_FLAG_ENVIRONMENT)) {
            std::fprintf(stderr, "--environment-light: the scene has no environment (--environment FILE, or --scene 15)\n");
            return 1;
        }
        if (rt_scene_set_environment_light(scene, environment_light) != RT_OK || rt_scene_commit(scene) != RT_OK) return die("environment light");
    }

    if (list_lights) {  // host only: the table as rt_scene_upload would copy it
        const int n = rt_scene_dump_lights(scene, 0, nullptr, nullptr, nullptr, nullptr);
        if (n < 0) return die("lights");
        std::vector<rt_light_row> rows((size_t)n + 1);
        std::vector<double> cdf(2 * (size_t)n + 2);
        rt_scene_dump_lights(scene, n, nullptr, nullptr, rows.data(), cdf.data());
        static const char *const names[] = {"quad", "triangle", "sphere", "moving_sphere"};
        std::printf("%d lights\n", n);
        for (int k = 0; k < n; k++) {
            const rt_light_row &r = rows[(size_t)k];
            std::printf("%d %s leaf %u material %u", k, names[r.kind & 3u], r.leaf, r.mat);
            if (r.kind <= 1)
                std::printf(" Q %.17g %.17g %.17g u %.17g %.17g %.17g v %.17g %.17g %.17g n %.17g %.17g %.17g area %.17g", r.a[0], r.a[1], r.a[2],
                            r.b[0], r.b[1], r.b[2], r.c[0], r.c[1], r.c[2], r.n[0], r.n[1], r.n[2], r.s);
            else if (r.kind == 2) std::printf(" centre %.17g %.17g %.17g radius %.17g", r.a[0], r.a[1], r.a[2], r.s);
            else
                std::printf(" c0 %.17g %.17g %.17g dc %.17g %.17g %.17g t0 %.17g dt %.17g radius %.17g", r.a[0], r.a[1], r.a[2], r.b[0], r.b[1],
                            r.b[2], r.c[0], r.c[1], r.s);
            std::printf(" cdf %.17g %.17g\n", cdf[2 * (size_t)k], cdf[2 * (size_t)k + 1]);
        }
        rt_scene_destroy(scene);
        return 0;
    }

    if (pick) {  // one closest-hit query (rt_scene_intersect) for the pixel's centre ray as the feature pass builds it
        double cam[27];  // bg, origin, lower-left corner, horizontal, vertical, u, v, w, lens radius, time0, time1
        if (rt_scene_dump_camera(scene, cam) != RT_OK) return die("camera");
        const double u = ((double)pick_i + 0.5) / (double)width, v = ((double)pick_j + 0.5) / (double)height;
        double o[3], d[3];
        for (int a = 0; a < 3; a++) {
            o[a] = cam[3 + a];
            d[a] = ((cam[6 + a] + u * cam[9 + a]) + v * cam[12 + a]) - o[a];
        }
        if (trace_at) {  // the radiance query below as a caller's own integrator: one path step a vertex, the fold of include/rtow.h
#pragma clang fp contract(off)
            static const char *const kinds[] = {"lambertian", "metal", "dielectric", "diffuse_light", "isotropic"};
            rt_path_step_params sp{};
            sp.count = 1;
            sp.time = cam[25];
            sp.seed = seed;
            sp.first_sequence = (unsigned long long)pick_j * (unsigned long long)width + (unsigned long long)pick_i;
            sp.variant = variant;
            sp.device = device;
            uint32_t state[6];
            bool seeded = false;  // the first step seeds the pixel's stream in the library; every later one continues it
            double sum[3] = {0.0, 0.0, 0.0}, seconds = 0.0;
            unsigned rays_traced = 0;
            for (int sample = 0; sample < spp && depth > 0; sample++) {
                double ro[3] = {o[0], o[1], o[2]}, rd[3] = {d[0], d[1], d[2]}, tm = cam[25];
                double thr[3] = {1.0, 1.0, 1.0}, acc[3] = {0.0, 0.0, 0.0};
                for (int bounce = 0; bounce < depth; bounce++) {
                    const rt_path_step_rays sr{ro, rd, &tm, seeded ? state : nullptr};
                    uint8_t status = 0, kind = 255;
                    double emitted[3], atten[3], t = 0.0;
                    const rt_path_step_out so{&status, emitted, atten, ro, rd, &tm, &t, nullptr, nullptr, &kind, state};
                    rt_path_step_stats ss{};
                    if (rt_scene_path_step(scene, &sp, &sr, &so, &ss) != RT_OK) return die("trace-at");
                    seeded = true;
                    seconds += ss.seconds;
                    rays_traced++;
                    std::printf("vertex: sample %d depth %d status %u t %.17g material %s emitted %.17g %.17g %.17g attenuation %.17g %.17g %.17g\n", sample,
                                bounce, (unsigned)status, t, kind < 5 ? kinds[kind] : "none", emitted[0], emitted[1], emitted[2], atten[0], atten[1],
                                atten[2]);
                    if (status != 2) {
                        for (int a = 0; a < 3; a++) {
                            const double product = thr[a] * emitted[a];
                            acc[a] = acc[a] + product;
                        }
                        break;
                    }
                    for (int a = 0; a < 3; a++) thr[a] = thr[a] * atten[a];
                }
                for (int a = 0; a < 3; a++) sum[a] = sum[a] + acc[a];
            }
            const double inv = 1 / (double)spp;
            std::printf("radiance %d,%d: samples %d radiance %.17g %.17g %.17g rays %u seconds %.9g\n", pick_i, pick_j, spp, inv * sum[0], inv * sum[1],
                        inv * sum[2], rays_traced, seconds);
            rt_scene_destroy(scene);
            return 0;
        }
        if (radiance_at && direct_mis) {  // the same query with light samples (rt_scene_radiance_direct), strategy 1
            rt_radiance_direct_params rp{};
            rp.count = 1;
            rp.samples = spp;
            rp.max_depth = depth;
            rp.time = cam[25];
            rp.seed = seed;
            rp.first_sequence = (unsigned long long)pick_j * (unsigned long long)width + (unsigned long long)pick_i;
            rp.variant = variant;
            rp.device = device;
            rp.strategy = 1;
            const rt_radiance_rays rr{o, d, nullptr, nullptr};
            double radiance[3];
            uint32_t path_rays = 0;
            const rt_radiance_out ro{radiance, &path_rays, nullptr};
            rt_radiance_direct_stats rs{};
            if (rt_scene_radiance_direct(scene, &rp, &rr, &ro, &rs) != RT_OK) return die("radiance-at");
            std::printf("radiance %d,%d: samples %d radiance %.17g %.17g %.17g rays %u seconds %.9g shadow_rays %llu reached %llu\n", pick_i, pick_j, spp,
                        radiance[0], radiance[1], radiance[2], (unsigned)path_rays, rs.seconds, (unsigned long long)rs.shadow_rays,
                        (unsigned long long)rs.shadow_reached);
            rt_scene_destroy(scene);
            return 0;
        }
        if (radiance_at) {  // one radiance query (rt_scene_radiance) for the same ray, from the pixel's stream
            rt_radiance_params rp{};
            rp.count = 1;
            rp.samples = spp;
            rp.max_depth = depth;
            rp.time = cam[25];
            rp.seed = seed;
            rp.first_sequence = (unsigned long long)pick_j * (unsigned long long)width + (unsigned long long)pick_i;
            rp.variant = variant;
            rp.device = device;
            const rt_radiance_rays rr{o, d, nullptr, nullptr};
            double radiance[3];
            uint32_t path_rays = 0;
            const rt_radiance_out ro{radiance, &path_rays, nullptr};
            rt_radiance_stats rs{};
            if (rt_scene_radiance(scene, &rp, &rr, &ro, &rs) != RT_OK) return die("radiance-at");
            std::printf("radiance %d,%d: samples %d radiance %.17g %.17g %.17g rays %u seconds %.9g\n", pick_i, pick_j, spp, radiance[0], radiance[1],
                        radiance[2], (unsigned)path_rays, rs.seconds);
            rt_scene_destroy(scene);
            return 0;
        }
        rt_query_params qp{};
        qp.count = 1;
        qp.tmin = 0.001;
        qp.tmax = INFINITY;
        qp.time = cam[25];
        qp.seed = seed;
        qp.first_sequence = (unsigned long long)pick_j * (unsigned long long)width + (unsigned long long)pick_i;  // the pixel's stream
        qp.variant = variant;
        qp.device = device;
        const rt_query_rays rays{o, d, nullptr, nullptr, nullptr};
        double t = 0.0, n[3], albedo[3];
        int32_t leaf = -1;
        uint8_t kind = 255;
        const rt_query_hits hits{&t, n, nullptr, albedo, &leaf, nullptr, &kind, nullptr};
        if (rt_scene_intersect(scene, &qp, &rays, &hits, nullptr) != RT_OK) return die("pick");
        static const char *const kinds[] = {"lambertian", "metal", "dielectric", "diffuse_light", "isotropic"};
        std::printf("pick %d,%d: leaf %d material %s t %.17g point %.17g %.17g %.17g normal %.17g %.17g %.17g albedo %.17g %.17g %.17g\n", pick_i,
                    pick_j, (int)leaf, kind < 5 ? kinds[kind] : "none", t, o[0] + t * d[0], o[1] + t * d[1], o[2] + t * d[2], n[0], n[1], n[2],
                    albedo[0], albedo[1], albedo[2]);
        rt_scene_destroy(scene);
        return 0;
    }

    rt_render_params p{};
    p.width = width;
    p.height = height;
    p.samples_per_pixel = spp;
    p.max_depth = depth;
    p.seed = seed;
    p.stripe_rows = 8;
    p.rank = 0;
    p.world_size = 1;
    p.variant = variant;
    p.device = device;
    p.flags = flags;
    std::vector<double> frame((size_t)width * height * 3);
    rt_render_stats st{};
    auto t0 = std::chrono::steady_clock::now();
    double gather_s = 0.0;
    FeatureRequest features{feature_samples, {}, {}, {}};
    std::vector<double> clean;  // --denoise: the filtered frame
    // one GPU: the feature pass on the film that holds the frame, the planes to the host, the filter on the film
    auto film_features = [&](rt_film *film) {
        rt_feature_params fp{};
        fp.width = width;
        fp.height = height;
        fp.samples = feature_samples;
        fp.seed = seed;
        fp.variant = variant;
        features.albedo.resize(frame.size());
        features.normal.resize(frame.size());
        features.depth.resize((size_t)width * height);
        if (rt_film_render_features(scene, film, &fp) != RT_OK ||
            rt_film_download_features(film, features.albedo.data(), features.normal.data(), features.depth.data(), width, height) != RT_OK)
            return false;
        if (!denoise) return true;
        clean.resize(frame.size());
        return rt_film_denoise(film, &dp) == RT_OK && rt_film_download_denoised(film, clean.data(), width, height) == RT_OK;
    };
    const rt_film_direct_params direct_params{1, {0, 0, 0, 0, 0, 0, 0}};  // lights picked by area x brightest channel
    auto launch = [&](rt_film *film) { return direct_frame ? rt_render_launch_direct(scene, film, &p, &direct_params) : rt_render_launch(scene, film, &p); };
    if (gpus >= 1) {
        if (render_multi_gpu(scene, p, gpus, frame.data(), &st, &gather_s, wants_features ? &features : nullptr) != 0) return die("render (multi-GPU)");
        if (denoise) {  // the planes are gathered: the same kernel on the whole frame, on GPU 0
            clean.resize(frame.size());
            if (rt_denoise_frame(0, frame.data(), features.albedo.data(), features.normal.data(), features.depth.data(), width, height, &dp,
                                 clean.data()) != RT_OK)
                return die("denoise");
        }
    } else if ((wants_features || direct_frame) && !adaptive) {
        rt_film *film = rt_film_create(device, width, height, p.stripe_rows, 0, 1);
        if (!film) return die("film");
        if (launch(film) != RT_OK || rt_render_finish(scene, film, &st) != RT_OK) return die("render");
        if (rt_film_download(film, frame.data(), width, height) != RT_OK) return die("download");
        if (wants_features && !film_features(film)) return die("features / denoise");
        rt_film_destroy(film);
    } else if (adaptive) {
        rt_film *film = rt_film_create(device, width, height, p.stripe_rows, 0, 1);
        if (!film) return die("film");
        const rt_adaptive_params ap{min_spp, check_every, noise, 0.01};
        if (rt_film_set_adaptive(film, &ap) != RT_OK) return die("adaptive");
        if (launch(film) != RT_OK || rt_render_finish(scene, film, &st) != RT_OK) return die("render");
        if (rt_film_download(film, frame.data(), width, height) != RT_OK) return die("download");
        std::vector<uint32_t> counts((size_t)width * height);
        if (rt_film_download_sample_counts(film, counts.data(), width, height) != RT_OK) return die("sample counts");
        // an adaptive frame is filtered like any other: the film's pixels, whatever sample count each has
        if (wants_features && !film_features(film)) return die("features / denoise");
        rt_film_destroy(film);
        std::fprintf(stderr, "adaptive: %.2f samples per pixel on average (noise %g, at least %d, at most %d).\n",
                     (double)st.samples / ((double)width * height), noise, min_spp, spp);
        if (!samples_map.empty()) {
            FILE *fp = std::fopen(samples_map.c_str(), "wb");
            if (!fp) {
                std::fprintf(stderr, "cannot write %s\n", samples_map.c_str());
                return 99;
            }
            std::fprintf(fp, "P5\n%d %d\n65535\n", width, height);
            std::vector<unsigned char> row((size_t)width * 2);
            for (int j = height - 1; j >= 0; j--) {  // top row first; big-endian samples as PGM prescribes
                for (int i = 0; i < width; i++) {
                    const uint32_t c = counts[(size_t)j * width + i] > 65535u ? 65535u : counts[(size_t)j * width + i];
                    row[2 * i] = (unsigned char)(c >> 8);
                    row[2 * i + 1] = (unsigned char)(c & 255u);
                }
                std::fwrite(row.data(), 1, row.size(), fp);
            }
            std::fclose(fp);
        }
    } else if (rt_render(scene, &p, frame.data(), &st) != RT_OK) {
        return die("render");
    }
    double wall = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    double kern = st.seconds_seed + st.seconds_render;
    if (gpus >= 1) std::fprintf(stderr, "%d GPU(s): slowest rank %.4f s of kernels; launch-to-gathered %.4f s\n", gpus, kern, gather_s);
    std::fprintf(stderr, "took %g seconds.\n", kern);
    std::fprintf(stderr, "%.1f Msamples/s, %.1f Mray/s (kernels); %.3f s wall incl. upload/download\n",
                 st.samples / kern * 1e-6, st.rays / kern * 1e-6, wall);
    if (rt_write_ppm(out.c_str(), denoise ? clean.data() : frame.data(), width, height) != RT_OK) return die("ppm");
    if (!raw_output.empty() && rt_write_ppm(raw_output.c_str(), frame.data(), width, height) != RT_OK) return die("ppm (raw)");
    if (!aov_prefix.empty()) {
        std::vector<double> depth3(frame.size());  // depth in all three channels: one PFM writer for all
        for (size_t k = 0; k < features.depth.size(); k++) depth3[3 * k] = depth3[3 * k + 1] = depth3[3 * k + 2] = features.depth[k];
        if (rt_write_pfm((aov_prefix + "_albedo.pfm").c_str(), features.albedo.data(), width, height) != RT_OK ||
            rt_write_pfm((aov_prefix + "_normal.pfm").c_str(), features.normal.data(), width, height) != RT_OK ||
            rt_write_pfm((aov_prefix + "_depth.pfm").c_str(), depth3.data(), width, height) != RT_OK)
            return die("pfm");
    }
    std::fprintf(stderr, "\nDone. Saved to %s\n", out.c_str());
    rt_scene_destroy(scene);
    return 0;
}
