// split_noise_check.cpp -- the leaf lookup of a split noise draw (split_leaf_of, split_covers, split_shifted, make_split of
// csrc/vrg_common.hpp) as a stand-alone host program, also for the address and undefined-behaviour sanitizers
// (tests/test_split_noise_host.py).  The oracle is a bisect over the leaves' starts (std::upper_bound): random tables of 1 .. 8 leaves
// that follow one another exactly, looked up at every boundary element and the elements on either side of it, at the launch's first and
// last element, and at random elements in between; then tables that are NOT tables (overlap, gap, grid not a multiple of 256, a count
// outside 1 .. 8, leaves that do not reach the launch's ends) against split_covers.
//
//   g++ -std=c++17 -fsanitize=address,undefined -I comfyui-vrgamedevgirl_amd/csrc tests/host_math/split_noise_check.cpp -o split_noise_check
#include <math.h>
#include <stdint.h>
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <random>
// libm stand-ins for the hardware transcendentals that csrc/vrg_pixel_math.hpp names (never called here)
#define VRG_HW_LOG2(x) log2f(x)
#define VRG_HW_SIN_REV(x) sinf((x) * 6.28318530717958647692f)
#define VRG_HW_COS_REV(x) cosf((x) * 6.28318530717958647692f)
#define VRG_HW_EXP2(x) exp2f(x)
#define VRG_HW_RCP(x) (1.0f / (x))
#include "vrg_common.hpp"

using namespace vrg;

static long checked = 0;

static void fail(const char* what, long long a = 0, long long b = 0) {
    std::fprintf(stderr, "split_noise_check: %s (%lld, %lld)\n", what, a, b);
    std::exit(1);
}

// the leaf of element e by bisect: the last leaf whose start is at or before e (the first leaf for an element before the table)
static int oracle(const vrg_noise_split& t, int64_t e) {
    int64_t starts[VRG_NOISE_LEAVES_MAX];
    for (int i = 0; i < t.count; ++i) starts[i] = t.leaves[i].start;
    const int64_t* at = std::upper_bound(starts, starts + t.count, e);
    return at == starts ? 0 : (int)(at - starts) - 1;
}

static void look_up(const vrg_noise_split& t, const NoiseSplitK& k, int64_t e) {
    const int got = split_leaf_of(k, e), want = oracle(t, e);
    if (got != want) fail("split_leaf_of differs from the bisect at element", e, got * 100 + want);
    const int64_t end = t.leaves[t.count - 1].start + (int64_t)t.leaves[t.count - 1].size;
    if (e >= t.leaves[0].start && e < end) {                     // inside the table: the element lies inside the leaf it was given
        const NoiseLeafK& l = k.leaf[got];
        if (e < l.start || e - l.start >= (int64_t)l.size) fail("the element is not inside its leaf", e, got);
    }
    ++checked;
}

int main() {
    std::mt19937_64 rnd(20240607);
    auto below = [&](uint64_t n) { return (int64_t)(rnd() % n); };
    for (int round = 0; round < 4000; ++round) {
        vrg_noise_split t{};
        t.seed = rnd();
        t.count = 1 + (int)below(VRG_NOISE_LEAVES_MAX);
        const bool large = round & 1;                            // sizes near 2^28 .. 2^29 (the real leaves) or a few elements
        int64_t at = -below(large ? ((int64_t)1 << 29) : 40);
        const int64_t first_start = at;
        for (int i = 0; i < t.count; ++i) {
            const uint32_t size = large ? (uint32_t)(((int64_t)1 << 28) + below((int64_t)1 << 28)) : (uint32_t)(1 + below(60));
            t.leaves[i] = vrg_noise_leaf{at, size, 256u * (uint32_t)(1 + below(2048)), (uint64_t)below((int64_t)1 << 40) * 4u};
            at += size;
        }
        const int64_t end = at;
        if (end <= 0) continue;                                  // (a table that ends before the launch begins covers nothing)
        const NoiseSplitK k = make_split(&t);
        if (k.count != t.count || k.seed != t.seed) fail("make_split lost the header");
        const int64_t total = 1 + below((uint64_t)end);
        if (!split_covers(k, total)) fail("a table that covers the launch is refused", round, total);
        if (!split_covers(k, end) || split_covers(k, end + 1)) fail("the table's end is not where the leaves end", round, end);
        for (int i = 0; i < t.count; ++i)
            for (int64_t d = -1; d <= 1; ++d) {
                look_up(t, k, t.leaves[i].start + d);
                look_up(t, k, t.leaves[i].start + (int64_t)t.leaves[i].size + d);
            }
        look_up(t, k, 0);
        look_up(t, k, total - 1);
        for (int j = 0; j < 16; ++j) look_up(t, k, first_start + below((uint64_t)(end - first_start)));
        // the same table for a launch that starts `shift` elements further on: every element keeps its leaf and its place in it
        const int64_t shift = below((uint64_t)end);
        const NoiseSplitK s = split_shifted(k, shift);
        for (int j = 0; j < 8; ++j) {
            const int64_t e = shift + below((uint64_t)(end - shift));
            const int a = split_leaf_of(k, e), b = split_leaf_of(s, e - shift);
            if (a != b || e - k.leaf[a].start != (e - shift) - s.leaf[b].start) fail("split_shifted moved an element", e, shift);
            ++checked;
        }
        // what is not a table
        if (t.count > 1) {
            NoiseSplitK bad = k;
            bad.leaf[1].start += 1;
            if (split_covers(bad, total)) fail("a gap between two leaves is accepted", round);
            bad.leaf[1].start -= 2;
            if (split_covers(bad, total)) fail("two overlapping leaves are accepted", round);
        }
        {
            NoiseSplitK bad = k;
            bad.leaf[t.count - 1].G += 128;
            if (split_covers(bad, total)) fail("a grid that is no multiple of 256 is accepted", round);
            bad = k; bad.leaf[0].G = 0;
            if (split_covers(bad, total)) fail("an empty grid is accepted", round);
            bad = k; bad.leaf[0].off += 2;
            if (split_covers(bad, total)) fail("an offset that is no multiple of 4 is accepted", round);
            bad = k; bad.count = 0;
            if (split_covers(bad, total)) fail("a table of no leaves is accepted", round);
            bad = k; bad.count = VRG_NOISE_LEAVES_MAX + 1;
            if (split_covers(bad, total)) fail("a table of nine leaves is accepted", round);
            bad = k; bad.count = -3;
            if (split_covers(bad, total)) fail("a negative count is accepted", round);
            bad = split_shifted(k, first_start - 1);             // the first leaf starts at element 1
            if (split_covers(bad, 1)) fail("a table that begins behind the launch's first element is accepted", round);
            if (split_covers(k, 0)) fail("a launch of no elements is accepted", round);
            checked += 9;
        }
    }
    // records from outside: counts that are not counts must not make make_split read or write past the eight leaves
    vrg_noise_split wild{};
    wild.count = 1000;
    if (split_covers(make_split(&wild), 1)) fail("count 1000 is accepted");
    wild.count = INT32_MIN;
    if (split_covers(make_split(&wild), 1)) fail("count INT32_MIN is accepted");
    std::printf("split_noise_check: %ld lookups and tables agree with the bisect\n", checked);
    return 0;
}
