"""The environment as a light of direct="mis" (Scene.EnvironmentLight): its first numbers, on one MI355X.

  timeout -k 10 540 python profiles/environment_light_measure.py [OUT]

writes OUT (profiles/r35_environment_light.txt by default) and prints it.  Scene 15 (the static random spheres under the computed
256 x 128 sky with a sun of 4000; no lamps, so the environment's effective share is 1 at any chance above 0), 400 x 400, strict
build throughout:
  1. seconds a sample of Scene.radiance(direct="mis") on the frame's centre rays and of a direct film, bit off and on (chance 0.5 and
     1.0), with the registers and the scratch of the kernels that ran;
  2. RMSE and median error per pixel of the linear luminance against a plain frame of REFERENCE_SPP samples -- and against a frame
     of REFERENCE_MIS_SPP samples by the estimator with the bit on --, at the wall time of 64 plain samples: plain, MIS with the bit
     off, MIS with the bit on;
  3. the share of the pixels of an adaptive direct film (min_samples 32) that stop at their first check, bit off against on;
  4. the standard errors on the sun ground of tests/test_environment_light_gpu.py (test E).
One process, one GPU; every timed launch follows a warm-up launch of the same kind, and the times are the kernels' own."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import raytracinginoneweekendincuda_amd as rt  # noqa: E402

W = H = 400
DEPTH = 50
REFERENCE_SPP, PLAIN_SPP, PROBE_SPP = 2048, 64, 16
REFERENCE_MIS_SPP = 1024    # a second reference by the estimator with the bit on: a plain frame of 2048 samples has itself found the sun in few pixels
ADAPTIVE = (32, 16, 0.05)   # min_samples, check_interval, noise_threshold
ADAPTIVE_CAP = 256
lines = []


def say(text=""):
    print(text, flush=True)
    lines.append(text)


def scene_with(chance):
    scene = rt.sky_demo_scene(1, W, H)
    if chance is not None:
        scene.EnvironmentLight(chance)
        scene.Commit()
    return scene


def luminance(frame):
    linear = frame * frame            # the film stores sqrt(colour)
    return linear.sum(axis=-1)


def centre_rays(scene):
    cam = scene.dump_camera()
    origin, llc, hor, ver = (cam[3 * k:3 * k + 3] for k in range(1, 5))
    u = ((np.arange(W) + 0.5) / W)[None, :, None]
    v = ((np.arange(H) + 0.5) / H)[:, None, None]
    d = np.ascontiguousarray((((llc + u * hor) + v * ver) - origin).reshape(-1, 3))
    return np.ascontiguousarray(np.broadcast_to(origin, d.shape)), d, float(cam[25])


def frame_of(scene, spp, direct, seed=1984):
    film = rt.Film(W, H)
    film.render(scene, 1, direct=direct, max_depth=DEPTH, seed=seed, variant=0)   # the warm-up
    film = rt.Film(W, H)
    st = film.render(scene, spp, direct=direct, max_depth=DEPTH, seed=seed, variant=0)
    return film.download(), st, film.direct_stats() if direct else None


def main(out_path):
    cases = (("bit off", None), ("chance 0.5", 0.5), ("chance 1.0", 1.0))
    scenes = {name: scene_with(chance) for name, chance in cases}
    say("The environment as a light of direct=\"mis\": scene 15, 400 x 400, max_depth 50, strict build, one MI355X (profiles/environment_light_measure.py).")
    for name, scene in scenes.items():
        told = scene.environment_light()
        say(f"  {name}: flags {scene.flags():#x}, lights {scene.info()['n_lights']}, chance {told['chance']}, effective share {told['effective']}")
    say()
    say("1. Seconds a sample (the kernel's own time over rays x samples), registers, scratch")
    o, d, tm = centre_rays(scenes["bit off"])
    for name, scene in scenes.items():
        scene.radiance(o, d, time=tm, samples=1, max_depth=DEPTH, direct="mis", stats=True)
        _, st = scene.radiance(o, d, time=tm, samples=PROBE_SPP, max_depth=DEPTH, direct="mis", stats=True)
        say(f"  Scene.radiance(direct='mis'), {len(o)} rays x {PROBE_SPP} samples, {name:10s}: {st.seconds * 1e3:8.2f} ms, {st.seconds / (len(o) * PROBE_SPP) * 1e9:7.2f} ns a sample, "
            f"{st.rays} path rays, {st.shadow_rays} shadow rays ({st.shadow_reached} reached), {st.kernel_vgprs} VGPRs, {st.scratch_bytes} B scratch")
    per_sample = {}
    for name, scene in scenes.items():
        _, st, ds = frame_of(scene, PROBE_SPP, "mis")
        per_sample[name] = st.seconds_render / PROBE_SPP
        say(f"  direct film, {PROBE_SPP} spp, {name:10s}: {st.seconds_render * 1e3:8.2f} ms, {per_sample[name] / (W * H) * 1e9:7.2f} ns a sample, {st.rays} path rays, "
            f"{ds.shadow_rays} shadow rays ({ds.shadow_reached} reached), {st.kernel_vgprs} VGPRs, {ds.scratch_bytes} B scratch, {st.lds_bytes} B LDS")
    say()
    say(f"2. Error against a plain frame of {REFERENCE_SPP} spp (seed 7), at the wall time of {PLAIN_SPP} plain samples: linear luminance r + g + b per pixel")
    reference, _, _ = frame_of(scenes["bit off"], REFERENCE_SPP, None, seed=7)
    ref = luminance(reference)
    reference_mis, _, _ = frame_of(scenes["chance 1.0"], REFERENCE_MIS_SPP, "mis", seed=7)
    ref_mis = luminance(reference_mis)
    both = np.abs(ref - ref_mis)
    say(f"  the two references: plain {REFERENCE_SPP} spp mean luminance {ref.mean():.5f}, MIS with the bit on {REFERENCE_MIS_SPP} spp {ref_mis.mean():.5f}; "
        f"between them RMSE {np.sqrt(np.mean(both * both)):.5f}, median difference {np.median(both):.5f}")
    plain, st, _ = frame_of(scenes["bit off"], PLAIN_SPP, None)
    budget = st.seconds_render
    rows = [("plain", plain, PLAIN_SPP, st.seconds_render)]
    for name in ("bit off", "chance 1.0"):
        spp = max(1, int(round(budget / per_sample[name])))
        frame, st, _ = frame_of(scenes[name], spp, "mis")
        rows.append((f"MIS, {name}", frame, spp, st.seconds_render))
    for name, frame, spp, seconds in rows:
        err, err_mis = np.abs(luminance(frame) - ref), np.abs(luminance(frame) - ref_mis)
        say(f"  {name:16s}: {spp:4d} spp in {seconds * 1e3:8.2f} ms, mean luminance {luminance(frame).mean():.5f}; against the plain reference RMSE "
            f"{np.sqrt(np.mean(err * err)):.5f}, median error {np.median(err):.5f}; against the MIS reference RMSE {np.sqrt(np.mean(err_mis * err_mis)):.5f}, "
            f"median error {np.median(err_mis):.5f}")
    say()
    say(f"3. Adaptive direct film, set_adaptive{ADAPTIVE}, at most {ADAPTIVE_CAP} samples: pixels that stop at their first check")
    for name in ("bit off", "chance 1.0"):
        film = rt.Film(W, H)
        film.set_adaptive(*ADAPTIVE)
        st = film.render(scenes[name], ADAPTIVE_CAP, direct="mis", max_depth=DEPTH, seed=1984, variant=0)
        counts = film.sample_counts()
        err, err_mis = np.abs(luminance(film.download()) - ref), np.abs(luminance(film.download()) - ref_mis)
        say(f"  {name:10s}: {np.mean(counts == ADAPTIVE[0]):.4f} of the pixels stop at {ADAPTIVE[0]} samples, mean samples {counts.mean():.1f}, at the cap {np.mean(counts == ADAPTIVE_CAP):.4f}, "
            f"{st.seconds_render * 1e3:.1f} ms; against the plain reference RMSE {np.sqrt(np.mean(err * err)):.5f}, median error {np.median(err):.5f}; against the MIS "
            f"reference RMSE {np.sqrt(np.mean(err_mis * err_mis)):.5f}, median error {np.median(err_mis):.5f}")
    say()
    say("4. The sun ground of tests/test_environment_light_gpu.py (a Lambertian ground and a box under scene 15's sky reduced to 64 x 32, 512 points, 64 batches,")
    say("   the mean over the points of r + g + b, two bounces)")
    from test_environment_light_gpu import sun_ground_estimates
    (ma, ea), (mf, ef), (mb, eb) = sun_ground_estimates()
    say(f"  A  Scene.radiance(samples=1, max_depth=2)                      {ma:.5f} +- {ea:.5f}")
    say(f"  B  path_step, sample_environment, occluded(shadow_rays(...))   {mb:.5f} +- {eb:.5f}    e_A / e_B = {ea / eb:.1f}  (r33: 36.9)")
    say(f"  F  Scene.radiance(direct='mis'), EnvironmentLight(1.0)         {mf:.5f} +- {ef:.5f}    e_A / e_F = {ea / ef:.1f}")
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "r35_environment_light.txt"))
