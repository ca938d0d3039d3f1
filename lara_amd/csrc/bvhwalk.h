// bvhwalk.h -- the step of the stackless walks over the implicit complete 8-ary tree of meshbvh_layout.h: from a slot that was
// stepped over, or a leaf that is done, to the next slot in order.  `level` counts from the leaves (0) to the root (`top`); `pos`
// is the counter within the level, its upper bits the parent's slot.  Behind the last of eight siblings the walk goes on behind
// their parent, level by level; back on `top` it is over.  `mask`: of eight siblings the one at counter c is slot c ^ mask below
// the root (meshray.hip's front-to-back order); 0 is the stored order.  meshsign.hip's walk uses this; lara_meshbvh_query and
// mr_walk carry the same arithmetic inline.
#pragma once

#if defined(__HIPCC__)
#define LARA_BVHWALK_HD __host__ __device__ __forceinline__
#else
#define LARA_BVHWALK_HD inline
#endif

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
