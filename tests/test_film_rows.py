"""csrc/film_rows.h scatter_owned_rows: a rank's compact rows to their places in the full frame, the one routine behind every
film download.  A stand-alone program (its own main, the header and the library's rt_stripe_rows, nothing of HIP in it) built with
the address and undefined-behaviour sanitizers scatters buffers of distinct values, exactly as large as the geometry says, into
sentinel-filled frames and prints them; the frames are compared with a restatement of the ownership rule in numpy."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import raytracinginoneweekendincuda_amd as rt

PACKAGE = os.path.dirname(os.path.abspath(rt.__file__))

# (width, height, stripe_rows, rank, world_size)
GEOMETRIES = [(5, 22, 4, 2, 3),    # a partial last stripe of 2 rows, 6 rows owned
              (5, 22, 4, 0, 1),    # owns everything
              (3, 3, 8, 1, 2),     # owns nothing
              (4, 16, 1, 3, 4)]    # one-row stripes
TYPES = {"u32": (1, 0xDEADBEEF), "f64": (3, -7.5)}   # name -> (channels, sentinel)

SOURCE = r"""
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "film_rows.h"

template <class T>
static void run(const char *name, int channels, T sentinel, const int *g, bool clear)
{
    const int w = g[0], h = g[1], owned = rt_stripe_rows(h, g[2], g[3], g[4], nullptr, 0);
    std::vector<T> compact((size_t)owned * w * channels);   // exactly the rows owned: a row too many read is out of bounds
    for (size_t k = 0; k < compact.size(); k++) compact[k] = (T)(k + 1);
    std::vector<T> full((size_t)h * w * channels, sentinel);
    rtow::scatter_owned_rows(compact.data(), channels, w, h, g[2], g[3], g[4], clear, full.data());
    std::printf("%s %d", name, (int)clear);
    for (T v : full) std::printf(" %.17g", (double)v);
    std::printf("\n");
}

int main(int argc, char **argv)
{
    if (argc != 6) return 2;
    int g[5];
    for (int k = 0; k < 5; k++) g[k] = std::atoi(argv[k + 1]);
    for (int clear = 0; clear < 2; clear++) {
        run<uint32_t>("u32", 1, 0xDEADBEEFu, g, clear != 0);
        run<double>("f64", 3, -7.5, g, clear != 0);
    }
    return 0;
}
"""


@pytest.fixture(scope="module")
def scatter_program(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("g++ not present")
    work = tmp_path_factory.mktemp("film_rows")
    src, exe = work / "film_rows_main.cpp", work / "film_rows_main"
    src.write_text(SOURCE)
    # (the sanitizers' runtimes linked into the program: it runs as it is wherever the suite runs)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-static-libasan", "-static-libubsan",
                           "-I", os.path.join(PACKAGE, "csrc"), str(src), "-o", str(exe),
                           "-L", PACKAGE, "-lrtow_hip", "-Wl,-rpath," + PACKAGE])
    return str(exe)


@pytest.mark.parametrize("geometry", GEOMETRIES)
def test_scatter_owned_rows(scatter_program, geometry):
    w, h, stripe, rank, world = geometry
    done = subprocess.run([scatter_program] + [str(v) for v in geometry], capture_output=True, text=True)
    assert done.returncode == 0, done.stderr   # every sanitizer report ends the program with an error status
    lines = [line.split() for line in done.stdout.splitlines()]
    assert sorted((l[0], l[1]) for l in lines) == [("f64", "0"), ("f64", "1"), ("u32", "0"), ("u32", "1")]
    rows = [j for j in range(h) if (j // stripe) % world == rank]
    assert rows == list(rt.stripe_rows(h, stripe, rank, world))
    for name, clear, *values in lines:
        channels, sentinel = TYPES[name]
        got = np.array([float(v) for v in values]).reshape(h, w * channels)
        want = np.full((h, w * channels), 0.0 if clear == "1" else float(sentinel))
        want[rows] = 1.0 + np.arange(len(rows) * w * channels).reshape(len(rows), w * channels)   # owned rows, in order
        assert np.array_equal(got, want), (name, clear)
