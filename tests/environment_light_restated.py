"""One call of rt_scene_path_advance_direct for a scene whose environment is a light (Scene.EnvironmentLight; include/rtow.h states
the estimator under rt_scene_path_advance_direct), restated from public calls only: ``path_step``, ``Rng.from_state(...).uniform()``
for the pick, ``sample_lights``, ``sample_environment``, ``light_pdf``, ``environment_pdf``, ``shadow_rays`` + ``occluded`` and
``rt.scatter_pdf``.  C, p, w and L are formed in numpy with exactly the operations of the header, one IEEE double operation each,
so the strict build equals it bit for bit.  It mirrors ``restated`` of tests/test_path_advance_direct_gpu.py, which stays the
restatement of a scene without the bit; for such a scene (shares 0 and 1) the two agree.

One thing no public call can do: carry a stream through an occlusion search.  Where a shadow ray meets a ConstantMedium the
medium draws from the path's stream; ``shadows`` lets the caller answer for those rays (test A's fog world does, from the
device's own streams, under the constraints stated there).  Without it the shadow rays draw nothing."""
import numpy as np

import raytracinginoneweekendincuda_amd as rt
from raytracinginoneweekendincuda_amd import _lib

SAMPLE_WANT = ("direction", "distance", "pdf", "emitted", "scatter_pdf", "rng_state")


def shares(scene):
    """(c_e, c_l) of the committed scene, by the table of rt_scene_set_environment_light."""
    told = scene.environment_light()
    c_e = told["effective"]
    if c_e == 0.0:
        return 0.0, 1.0
    return c_e, (1.0 - told["chance"]) if len(scene.lights()["kind"]) else 0.0


def pick(states, c_e):
    """The pick of every row: x = (double) curand_uniform from the row's stream, the environment where x <= c_e; nothing is drawn
    where c_e == 1.  Returns (environment picked, the streams behind the draw)."""
    if not c_e < 1.0:
        return np.ones(len(states), dtype=bool), states.copy()
    sky, after = np.zeros(len(states), dtype=bool), states.copy()
    for k in range(len(states)):
        rng = rt.Rng.from_state(states[k])
        sky[k] = np.float64(rng.uniform()) <= c_e
        after[k] = rng.state()
    return sky, after


def restated(scene, live, radiance, strategy, sample, alive=None, shadows=None):
    """(the survivors' rows by output name, the radiance array afterwards, the bookkeeping).  ``shadows(P, direction, distance, time,
    rows, streams)``: None, or a function that answers (visible, streams afterwards or None) for the shadow rays cast -- ``rows`` are
    their positions among the survivors, ``streams`` the paths' streams behind the sample."""
    c_e, c_l = shares(scene)
    assert c_e > 0.0, "the scene's environment is a light"
    o, d, tm, states = live["origin"], live["direction"], live["time"], live["rng_state"]
    T, ids, q = live["throughput"], live["ray_id"], live["scatter_pdf"]
    n = len(ids)
    alive = np.ones(n, dtype=bool) if alive is None else alive != 0
    step = scene.path_step(o, d, times=tm, rng_state=states, want=tuple(_lib.STEP_OUTPUTS))
    status, m, nrm = step["status"], step["material"], step["normal"]
    after = radiance.copy()
    inside = (ids >= 0) & (ids < len(after))
    told = dict(cast=0, reached=0, sky_picks=0, table_picks=0, sky_ends=0, lamp_ends=0, dark_samples=0, lamp_weights=[], sky_rows=[],
                isotropic=0)
    with np.errstate(all="ignore"):
        # the path ended: a lamp against the table's share, a miss against the environment's
        ends = alive & (status != 2)
        lamp = ends & (status == 1) & (m == 3) & (q > 0)
        sky = ends & (status == 0) & (q > 0)
        p_lamp = c_l * scene.light_pdf(o, d, times=tm, strategy=strategy)["pdf"] if len(scene.lights()["kind"]) else np.zeros(n)
        p_sky = c_e * scene.environment_pdf(o, d)["pdf"]
        w = np.where(lamp, q / (q + p_lamp), np.where(sky, q / (q + p_sky), 1.0))
        sel = ends & inside
        after[ids[sel]] = after[ids[sel]] + (T[sel] * step["emitted"][sel]) * w[sel][:, None]
        told.update(sky_ends=int((sky & inside).sum()), lamp_ends=int((lamp & inside).sum()), lamp_weights=w[lamp & inside])
        # the path scattered
        goes = alive & (status == 2)
        Tn = T * step["attenuation"]
        q_next = np.zeros(n)
        states_next = step["rng_state"].copy()
        idx = np.flatnonzero(goes & ((m == 0) | (m == 4))) if sample else np.zeros(0, dtype=np.int64)
        if len(idx):
            P, nn, tt, mm = (np.ascontiguousarray(step[k][idx]) for k in ("origin", "normal", "time", "material"))
            picked_sky, behind = pick(np.ascontiguousarray(step["rng_state"][idx]), c_e)
            C, p, s = np.zeros((len(idx), 3)), np.zeros(len(idx)), np.zeros(len(idx))
            direction, distance = np.zeros((len(idx), 3)), np.zeros(len(idx))
            e, t = np.flatnonzero(picked_sky), np.flatnonzero(~picked_sky)
            if len(e):
                smp = scene.sample_environment(np.ascontiguousarray(P[e]), normals=np.ascontiguousarray(nn[e]), materials=np.ascontiguousarray(mm[e]),
                                               rng_state=np.ascontiguousarray(behind[e]), want=SAMPLE_WANT + ("light",))
                valid = smp["pdf"] > 0.0
                s[e] = smp["scatter_pdf"]
                C[e] = np.where((valid & (s[e] != 0))[:, None], (s[e] / (c_e * smp["pdf"]))[:, None] * smp["emitted"], 0.0)
                p[e] = c_e * smp["pdf"]
                direction[e], distance[e], behind[e] = smp["direction"], smp["distance"], smp["rng_state"]
                told["sky_rows"] = smp["light"]
            if len(t):
                smp = scene.sample_lights(np.ascontiguousarray(P[t]), np.ascontiguousarray(nn[t]), np.ascontiguousarray(mm[t]), np.ascontiguousarray(tt[t]),
                                          np.ascontiguousarray(behind[t]), strategy=strategy, want=SAMPLE_WANT)
                s[t] = smp["scatter_pdf"]
                C[t] = np.where((s[t] != 0)[:, None], (s[t] / (c_l * smp["pdf"]))[:, None] * smp["emitted"], 0.0)
                direction[t], distance[t], behind[t] = smp["direction"], smp["distance"], smp["rng_state"]
                p[t] = c_l * scene.light_pdf(np.ascontiguousarray(P[t]), np.ascontiguousarray(direction[t]), times=np.ascontiguousarray(tt[t]),
                                             strategy=strategy)["pdf"]
            wl = np.where(p + s == 0, 0.0, p / (p + s))
            L = (Tn[idx] * C) * wl[:, None]
            cast = (C != 0).any(axis=1)
            visible = np.zeros(len(idx), dtype=bool)
            if cast.any():
                rows = np.flatnonzero(cast)
                args = (np.ascontiguousarray(P[cast]), np.ascontiguousarray(direction[cast]), np.ascontiguousarray(distance[cast]),
                        np.ascontiguousarray(tt[cast]))
                if shadows is None:
                    visible[cast] = ~scene.occluded(*scene.shadow_rays(*args))
                else:
                    visible[cast], drawn = shadows(*args, np.searchsorted(np.flatnonzero(goes), idx[rows]), behind[rows])
                    if drawn is not None:
                        behind[rows] = drawn
            states_next[idx] = behind
            add = visible & inside[idx]
            after[ids[idx][add]] = after[ids[idx][add]] + L[add]
            dn = step["direction"][idx]
            u = (1.0 / np.sqrt((dn[:, 0] * dn[:, 0] + dn[:, 1] * dn[:, 1]) + dn[:, 2] * dn[:, 2]))[:, None] * dn
            q_next[idx] = rt.scatter_pdf(mm, nn, u)
            told.update(cast=int(cast.sum()), reached=int(visible.sum()), sky_picks=len(e), table_picks=len(t),
                        dark_samples=int((~cast).sum()), isotropic=int((mm == 4).sum()))
    out = {k: step[k][goes] for k in ("origin", "direction", "time", "t", "normal", "front_face", "material")}
    out.update(rng_state=states_next[goes], throughput=Tn[goes], ray_id=ids[goes], scatter_pdf=q_next[goes])
    return out, after, told
