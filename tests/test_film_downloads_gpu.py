"""Every film download puts a rank's compact rows where they belong in the full frame (csrc/film_rows.h behind
csrc/device_scene.cpp download_rows).  The Cornell box at 24 x 22, 4 samples, strict build, rendered whole and once per rank of
three with 4-row stripes -- rank 2 ends on a stripe of 2 rows: each rank's rows are the whole frame's bit for bit, in the pixels,
the sample counts of an adaptive film and the three feature planes; the rows of the other ranks come back 0, except from
rt_film_download, which leaves them as the caller had them."""
import numpy as np
import pytest

import raytracinginoneweekendincuda_amd as rt
from raytracinginoneweekendincuda_amd import _lib
from query_helpers import bits

pytestmark = pytest.mark.gpu

W, H, SPP, STRIPE, WORLD = 24, 22, 4, 4, 3
# adaptive sampling: checks after 2 and 3 samples; a pixel whose two first samples are equal (black twice: most of the box at
# this sample count) stops at 2, one with a single path to the light has a relative error of 1 and goes on
ADAPTIVE = dict(min_samples=2, check_interval=1, noise_threshold=0.5)
SENTINEL = -123.25


class Rendered:
    """One share of the frame: a plain film with its feature pass, and an adaptive film."""

    def __init__(self, scene, **share):
        self.film = rt.Film(W, H, **share)
        self.film.render(scene, SPP, variant=0)
        self.film.render_features(scene, samples=0, variant=0)
        self.frame = self.film.download()
        self.features = self.film.features()
        adaptive = rt.Film(W, H, **share)
        adaptive.set_adaptive(**ADAPTIVE)
        adaptive.render(scene, SPP, variant=0)
        self.counts = adaptive.sample_counts()


@pytest.fixture(scope="module")
def scene():
    return rt.builtin_scene(7, 0, W, H)


@pytest.fixture(scope="module")
def whole(scene):
    return Rendered(scene)


@pytest.fixture(scope="module", params=range(WORLD))
def share(request, scene):
    rank = request.param
    rows = rt.stripe_rows(H, STRIPE, rank, WORLD)
    others = np.setdiff1d(np.arange(H), rows)
    assert len(rows) == (8, 8, 6)[rank] and len(others) == H - len(rows)
    return Rendered(scene, stripe_rows=STRIPE, rank=rank, world_size=WORLD), rows, others


def test_whole_frame_is_worth_comparing(whole):
    assert whole.frame.any()
    assert len(np.unique(whole.counts)) > 1 and whole.counts.min() >= 2 and whole.counts.max() <= SPP
    albedo, normal, depth = whole.features
    assert albedo.any() and normal.any() and depth.any()


def test_pixels(whole, share):
    mine, rows, others = share
    assert np.array_equal(bits(mine.frame[rows]), bits(whole.frame[rows]))


def test_sample_counts(whole, share):
    mine, rows, others = share
    assert np.array_equal(mine.counts[rows], whole.counts[rows])
    assert not mine.counts[others].any()


def test_features(whole, share):
    mine, rows, others = share
    for got, want in zip(mine.features, whole.features):
        assert np.array_equal(bits(got[rows]), bits(want[rows]))
        assert not bits(got[others]).any()


def test_download_leaves_other_rows_alone(whole, share):
    mine, rows, others = share
    frame = np.full((H, W, 3), SENTINEL)
    assert rt.lib().rt_film_download(mine.film._p, frame.ctypes.data_as(_lib.D3), W, H) == 0
    assert np.array_equal(bits(frame[rows]), bits(whole.frame[rows]))
    assert (frame[others] == SENTINEL).all()
