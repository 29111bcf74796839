// film_rows.h -- a rank's compact rows to their places in the full frame.  Host only, nothing of HIP: device_scene.cpp puts the
// device-to-host copy in front of it, tests/test_film_rows.py compiles it alone.
#pragma once
#include <cstddef>
#include <cstring>
#include <vector>

#include "../../include/rtow.h"

namespace rtow {

// `compact` holds the rows this rank owns, one after the other, `channels` values of T per pixel; which rows those are is
// rt_stripe_rows' to say (the one statement of the ownership rule).  The rows of other ranks are zeroed (clear_other_rows) or
// stay as the caller had them.
template <class T>
void scatter_owned_rows(const T *compact, int channels, int width, int height, int stripe_rows, int rank, int world_size,
                        bool clear_other_rows, T *full)
{
    const size_t row = (size_t)width * (size_t)channels;
    if (clear_other_rows) std::memset(full, 0, row * (size_t)height * sizeof(T));
    std::vector<int> rows((size_t)height);
    const int owned = rt_stripe_rows(height, stripe_rows, rank, world_size, rows.data(), height);
    for (int k = 0; k < owned; k++) std::memcpy(full + (size_t)rows[k] * row, compact + (size_t)k * row, row * sizeof(T));
}

}  // namespace rtow
