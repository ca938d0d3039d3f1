// bvhwalk_hostcheck.cpp -- the walk of csrc/bvhwalk.h on the host, over the layouts mb_layout(T) gives, for a build with
// -fsanitize=address,undefined (tools/bvhwalk_hostcheck.py compiles this file for the host alone and runs it; nothing here touches a
// device or is loaded into python).  The callables are trivial: every slot below n[level] is entered, every leaf visit is recorded.
// Against a recursive enumeration of the same tree, for every T of the list and each of the eight sibling masks:
//   * the leaves visited are those of the enumeration, in its order (mask 0: 0 .. ceil(T/8) - 1 ascending, each once), so no
//     padding slot reaches `leaf`;
//   * `enter` is asked exactly as often as the enumeration meets a slot, which is below L.steps: the walk ended back on the root's
//     level, neither by the bound nor by the padding guard; it is never asked for a level or a slot outside the stored ones;
//   * a `leaf` that returns true at its k-th visit ends the walk there, and the walk returns true then and only then.
// T: 1 (the root is the leaf level), 8^k - 1 .. 8^k + 2 for every k (8^k + 1 is where the number of levels changes), and 75, whose
// last sibling group is partly padding on two levels at once.  Prints one line per T and the violations; exit 1 on any.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../lara_amd/csrc/common.h"
#include "../lara_amd/csrc/unigrid.h"
#include "../lara_amd/csrc/bvhwalk.h"

namespace {

struct Visits { std::vector<int> leaves; long long asked = 0; };

void enumerate(const MbLayout &L, const int mask, const int level, const int slot, Visits &v) {
    v.asked++;
    if (slot >= L.n[level]) return;
    if (level == 0) { v.leaves.push_back(slot); return; }
    for (int c = 0; c < 8; c++) enumerate(L, mask, level - 1, slot * 8 + (c ^ mask), v);
}

// the walk that ends at the `stop`-th leaf visit (0: never); bad: questions outside the stored slots
bool walk(const MbLayout &L, const int mask, const long long stop, Visits &v, long long &bad) {
    return lara_bvhwalk(
        L, mask,
        [&](const int level, const int slot) {
            v.asked++;
            if (level < 0 || level >= L.levels || slot < 0 || slot >= (L.n[level] + 7) / 8 * 8) { bad++; return false; }
            return slot < L.n[level];
        },
        [&](const int leaf) {
            v.leaves.push_back(leaf);
            return (long long)v.leaves.size() == stop;
        });
}

long long check(const int64_t T) {
    const MbLayout L = mb_layout(T);
    const int n0 = (int)((T + 7) / 8);
    long long bad = 0, asked0 = 0;
    if (L.levels < 1 || L.levels > MB_LEVELS || L.n[0] != n0 || L.n[L.levels - 1] != 1) bad++;
    for (int mask = 0; mask < 8; mask++) {
        Visits want, got;
        enumerate(L, mask, L.levels - 1, 0, want);
        if (walk(L, mask, 0, got, bad)) bad++;
        if (got.leaves != want.leaves || got.asked != want.asked || !(got.asked < L.steps)) bad++;
        if ((int)got.leaves.size() != n0) bad++;
        if (mask == 0) {
            asked0 = got.asked;
            for (int i = 0; i < (int)got.leaves.size(); i++) bad += got.leaves[i] != i;
        } else {      // the same set: every leaf once
            std::vector<char> seen((size_t)n0, 0);
            for (const int s : got.leaves) {
                if (s < 0 || s >= n0 || seen[(size_t)s]) { bad++; break; }
                seen[(size_t)s] = 1;
            }
        }
        for (const long long k : {1ll, (long long)(n0 + 1) / 2, (long long)n0}) {
            Visits part;
            if (!walk(L, mask, k, part, bad) || (long long)part.leaves.size() != k) { bad++; continue; }
            for (long long i = 0; i < k; i++) bad += part.leaves[(size_t)i] != want.leaves[(size_t)i];
        }
    }
    std::printf("T %9lld: levels %d, leaves %8d, steps bound %9lld, slots asked %9lld, violations %lld\n", (long long)T, L.levels, n0,
                (long long)L.steps, asked0, bad);
    return bad;
}

}  // namespace

int main() {
    long long bad = 0;
    int sizes = 0, changes = 0;
    bad += check(1);
    sizes++;
    for (int64_t p = 8; p + 2 < (1ll << 26); p *= 8) {
        if (mb_layout(p).levels + 1 == mb_layout(p + 1).levels) changes++; else bad++;
        for (int64_t T = p - 1; T <= p + 2; T++, sizes++) bad += check(T);
    }
    const MbLayout two = mb_layout(75);
    if (!(two.levels >= 3 && two.n[0] % 8 != 0 && two.n[1] % 8 != 0)) bad++;
    bad += check(75);
    sizes++;
    std::printf("sizes %d, changes of the level count covered %d, masks 8, violations %lld\n", sizes, changes, bad);
    return bad ? 1 : 0;
}
