"""Frames against frames, and rt_render_params by keyword (tests only)."""
import numpy as np

import raytracinginoneweekendincuda_amd as rt


def compare(got, want, tol=1e-5):
    """Two (..., 3) float64 frames: (share of bit-identical pixels, share of pixels within ``tol`` in every channel, max |d|).
    1e-5 is BASELINE.json's north_star: absolute, on the gamma-corrected [0, 1] colour the kernel stores."""
    diff = np.abs(got - want)
    exact = float(np.mean(np.all(got.view(np.uint64) == want.view(np.uint64), axis=-1)))
    within = float(np.mean(np.all(diff <= tol, axis=-1)))
    return exact, within, float(diff.max())


def render_params(width, height, spp, **kw):
    """rt.RenderParams by field name (raytracinginoneweekendincuda_amd/_lib.py): max_depth 50, seed 1984, stripes of 8 rows, rank 0
    of 1 as in Scene.render; every other field 0 / None."""
    unknown = set(kw) - {name for name, _ in rt.RenderParams._fields_}
    assert not unknown, unknown   # a ctypes Structure takes a misspelt keyword without a word
    fields = dict(max_depth=50, seed=1984, stripe_rows=8, rank=0, world_size=1)
    fields.update(kw)
    return rt.RenderParams(width=width, height=height, samples_per_pixel=spp, **fields)
