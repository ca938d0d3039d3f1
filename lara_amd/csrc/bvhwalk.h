// bvhwalk.h -- the one stackless walk over the implicit complete 8-ary tree of meshbvh_layout.h, and what every unit that walks it
// needs around it: whether a buffer can be walked, the walk, and the eight records of a leaf.  meshbvh.hip, meshray.hip,
// meshsign.hip and meshwind.hip differ in what they ask of a slot (`enter`) and do with a leaf (`leaf`); the skeleton is here alone.
// `level` counts from the leaves (0) to the root (`top`); `pos` is the counter within the level, its upper bits the parent's slot.
// Behind the last of eight siblings the walk goes on behind their parent, level by level; back on `top` it is over.  `mask`: of
// eight siblings the one at counter c is slot c ^ mask below the root (meshray.hip's front-to-back order); 0 is the stored order.
// The walk is __host__ __device__ and reads three fields of the layout (levels, steps, n[]): tools/bvhwalk_hostcheck.cpp runs it
// on the host over mb_layout(T).
#pragma once

#include "meshbvh_layout.h"

#define LARA_BVHWALK_HD __host__ __device__ __forceinline__
// on every lambda handed to the walk or to mb_leaf_records: inlined with the functions around it, its captures stay in registers
#define LARA_BVHWALK_INLINE __attribute__((always_inline))

// the slot the counter `pos` of `level` stands for
LARA_BVHWALK_HD int lara_bvhwalk_slot(const int level, const int pos, const int top, const int mask) {
    return level < top ? pos ^ mask : pos;
}

// on to the next counter; true: the walk is over (back on the root's level)
LARA_BVHWALK_HD bool lara_bvhwalk_advance(int &level, int &pos, const int top, const int mask) {
    pos++;
    while (level < top && (pos & 7) == 0) {      // behind the last of eight siblings: on behind their parent
        const int parent = (pos >> 3) - 1;
        level++;
        pos = lara_bvhwalk_slot(level, parent, top, mask) + 1;
    }
    return level == top;
}

// The walk over a layout with 0 < L.levels <= MB_LEVELS, from the root: enter(level, slot) -> the slot is to be descended into (on
// level 0: its records are wanted), leaf(slot) -> true ends the walk.  True: a leaf ended it.  At most L.steps slots are asked.
template <class Enter, class Leaf>
LARA_BVHWALK_HD bool lara_bvhwalk(const MbLayout &L, const int mask, Enter &&enter, Leaf &&leaf) {
    const int top = L.levels - 1;
    const long long steps = L.steps;
    int level = top, pos = 0;
    for (long long step = 0; step < steps; step++) {
        const int slot = lara_bvhwalk_slot(level, pos, top, mask);
        if (slot >= ((L.n[level] + 7) & ~7)) break;      // (never, on a buffer lara_meshbvh_build wrote)
        if (enter(level, slot)) {
            if (level > 0) { level--; pos = slot << 3; continue; }
            if (leaf(slot)) return true;
        }
        if (lara_bvhwalk_advance(level, pos, top, mask)) break;
    }
    return false;
}

namespace {

// what a walker reads of the buffer before it starts; ok: the levels are in range, the buffer can be walked
struct MbWalk { const MbHeader *hdr; const float4 *rec; int T, n_valid, top; bool ok; };

__device__ __forceinline__ MbWalk mb_walk_open(const char *__restrict__ bvh) {
    MbWalk w;
    w.hdr = (const MbHeader *)bvh;
    w.T = w.hdr->count[LARA_MESHBVH_HDR_TRIANGLES];
    w.n_valid = min(w.hdr->count[LARA_MESHBVH_HDR_VALID], w.T);
    w.top = w.hdr->L.levels - 1;
    w.ok = w.top >= 0 && w.top < MB_LEVELS;
    w.rec = (const float4 *)(bvh + w.hdr->L.rec);
    return w;
}

// the valid records of leaf `leaf`, in stored order: f(record, its position) -> true ends the loop.  True: f ended it
template <class F>
__device__ __forceinline__ bool mb_leaf_records(const float4 *__restrict__ rec, const int T, const int leaf, F &&f) {
#pragma unroll 1
    for (int k = 0; k < 8; k++) {
        const long long r = 8ll * leaf + k;
        if (r >= T) break;
        const TriRec m = tri_load(rec, (int)r);
        if (m.id < 0) continue;
        if (f(m, (int)r)) return true;
    }
    return false;
}

}  // namespace
