// meshbvh_layout.h -- the buffer lara_meshbvh_build writes, as the units that walk it see it (meshbvh.hip, meshray.hip, meshsign.hip,
// meshwind.hip): the layout as a function of T, the header's slot, and the load of a 24-byte box; the 48-byte record (TriRec,
// tri_load) is trimesh.h's, the walk itself bvhwalk.h's, which includes this file.  Format and sizes in include/lara_meshbvh.h.
// Include after common.h and unigrid.h.
#pragma once

#include "trimesh.h"
#include "../../include/lara_meshbvh.h"

namespace {

constexpr int MB_LEVELS = LARA_MESHBVH_MAX_LEVELS;

// byte offsets into the caller's buffer and slot counts: functions of T alone
struct MbLayout {
    int64_t keys, rec, part, total, steps;      // steps: all stored slots, the walk's cap
    int64_t box[MB_LEVELS];
    int n[MB_LEVELS];
    int levels;
};

struct MbHeader {
    int count[LARA_MESHBVH_HEADER_INTS];      // LARA_MESHBVH_HDR_*
    float lo[3], inv[3];                      // the cell rule
    MbLayout L;
};
static_assert(sizeof(MbHeader) <= 256, "the header's slot");

MbLayout mb_layout(const int64_t T) {
    MbLayout w = {};
    int64_t o = 256;
    w.keys = o;  o = align_up(o + T * 8, 256);
    w.rec = o;   o = align_up(o + T * 48, 256);
    w.part = o;  o = align_up(o + MM_BOUNDS_BLOCKS * 6 * 4, 256);
    int64_t n = (T + 7) / 8;
    for (int k = 0; k < MB_LEVELS; k++) {
        const int64_t padded = (n + 7) / 8 * 8;
        w.box[k] = o;  o = align_up(o + padded * 24, 256);
        w.n[k] = (int)n;
        w.steps += padded;
        w.levels = k + 1;
        if (n == 1) break;
        n = (n + 7) / 8;
    }
    w.total = o;
    return w;
}

__device__ __forceinline__ void mb_load_box(const float2 *__restrict__ box, const size_t j, float lo[3], float hi[3]) {
    const float2 a = box[3 * j], b = box[3 * j + 1], c = box[3 * j + 2];
    lo[0] = a.x; lo[1] = a.y; lo[2] = b.x;
    hi[0] = b.y; hi[1] = c.x; hi[2] = c.y;
}

}  // namespace
