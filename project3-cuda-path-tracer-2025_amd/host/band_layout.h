// band_layout.h — which bytes of a W x H float3 image belong to one shard of a multi-device context.
//
// The image is cut into bands of `rows` rows; shard `rank` of `count` owns bands rank, rank + count,
// ... (ShardDev, (y / rows) % count == rank).  Its full bands are one strided 2-D region: `height`
// bands of `width` bytes, `pitch` bytes apart, the first at byte `first`.  The image's last band is
// shorter when rows does not divide H; the shard that owns it gets it as `tail_bytes` at `tail_off`.
// Pure arithmetic (csrc/rt_multi.h band_prepare; host/runtime_host_check.cpp paints every case).
#pragma once

#include <algorithm>
#include <cstddef>

namespace pth {

struct BandGeom {
    size_t first = 0, pitch = 0, width = 0, height = 0;   // `height` bands of `width` bytes, `pitch` apart
    size_t tail_off = 0, tail_bytes = 0;                 // a shorter last band (0 bytes: none)
};

inline BandGeom band_geometry(int W, int H, int rows, int count, int rank) {
    const size_t R = (size_t)std::max(1, rows), N = (size_t)std::max(1, count), k = (size_t)rank;
    const size_t h = (size_t)H, row = 3 * sizeof(float) * (size_t)W;
    const size_t nb = (h + R - 1) / R;                   // bands of the image; shard k has k, k + N, ..
    size_t mine = k < nb ? (nb - 1 - k) / N + 1 : 0;
    BandGeom b;
    b.width = R * row;
    b.pitch = N * R * row;
    b.first = k * R * row;
    if (mine > 0 && (nb - 1) % N == k && h % R != 0) {   // the image's last band is shorter and ours
        --mine;
        b.tail_off = (nb - 1) * R * row;
        b.tail_bytes = (h - (nb - 1) * R) * row;
    }
    b.height = mine;
    return b;
}

}  // namespace pth
