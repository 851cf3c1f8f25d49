// overlap_check.cpp -- vrg_ranges_overlap and vrg_operand_bytes of csrc/vrg_common.hpp, the one overlap rule of the entry points, as a
// stand-alone program for the address and undefined-behaviour sanitizers (tests/test_overlap_host.py).  The oracle is the plain interval
// test on 128-bit integers, where no sum can wrap: [a, a + na) and [b, b + nb) share a byte iff both hold a byte, both operands are there
// (not null) and a < b + nb and b < a + na.  The addresses are made from integers and never dereferenced.
//
//   g++ -std=c++17 -fsanitize=address,undefined -I comfyui-vrgamedevgirl_amd/csrc tests/host_math/overlap_check.cpp -o overlap_check
#include <math.h>
#include <stdint.h>
#include <cstdio>
#include <cstdlib>
// libm stand-ins for the hardware transcendentals that csrc/vrg_pixel_math.hpp names (never called here)
#define VRG_HW_LOG2(x) log2f(x)
#define VRG_HW_SIN_REV(x) sinf((x) * 6.28318530717958647692f)
#define VRG_HW_COS_REV(x) cosf((x) * 6.28318530717958647692f)
#define VRG_HW_EXP2(x) exp2f(x)
#define VRG_HW_RCP(x) (1.0f / (x))
#include "vrg_common.hpp"

typedef unsigned __int128 u128;

static long checked = 0;

static const void* at(uintptr_t address) { return reinterpret_cast<const void*>(address); }

static bool oracle(uintptr_t a, int64_t na, uintptr_t b, int64_t nb) {
    if (!a || !b || na <= 0 || nb <= 0) return false;
    const u128 a0 = a, a1 = a0 + (u128)(uint64_t)na, b0 = b, b1 = b0 + (u128)(uint64_t)nb;
    return a0 < b1 && b0 < a1;
}

static void fail(const char* what, uintptr_t a, int64_t na, uintptr_t b, int64_t nb, bool got) {
    std::fprintf(stderr, "overlap_check: %s: [%#llx, +%lld) against [%#llx, +%lld) gave %d\n", what, (unsigned long long)a, (long long)na,
                 (unsigned long long)b, (long long)nb, (int)got);
    std::exit(1);
}

// the helper against the oracle, and against itself with the two ranges swapped
static bool check(uintptr_t a, int64_t na, uintptr_t b, int64_t nb) {
    const bool got = vrg_ranges_overlap(at(a), na, at(b), nb), swapped = vrg_ranges_overlap(at(b), nb, at(a), na);
    if (got != oracle(a, na, b, nb)) fail("differs from the 128-bit interval test", a, na, b, nb, got);
    if (got != swapped) fail("changes with the order of its arguments", a, na, b, nb, got);
    ++checked;
    return got;
}

static void expect(bool want, uintptr_t a, int64_t na, uintptr_t b, int64_t nb, const char* arrangement) {
    if (check(a, na, b, nb) != want) fail(arrangement, a, na, b, nb, !want);
}

// the arrangements of tests/overlap_support.py for a written range of `wn` elements and a read range of `rn` elements of `e` bytes whose
// read range starts at `r`: (a) .. (e) refused, (f) .. (h) accepted
static void arrangements(uintptr_t r, int64_t rn, int64_t wn, int64_t e) {
    const int64_t rb = rn * e, wb = wn * e;
    expect(true, r, wb, r, rb, "(a) same start");
    if (rn > 1) expect(true, r + (uintptr_t)e, wb, r, rb, "(b) the write starts one element after the read's start");
    expect(true, r - (uintptr_t)(wb - e), wb, r, rb, "(c) the write's last element is the read's first");
    if (wn + 2 <= rn) expect(true, r + (uintptr_t)e, wb, r, rb, "(d) the write lies strictly inside the read");
    if (rn + 2 <= wn) expect(true, r - (uintptr_t)e, wb, r, rb, "(e) the read lies strictly inside the write");
    expect(false, r - (uintptr_t)wb, wb, r, rb, "(f) the write ends exactly where the read starts");
    if ((u128)r + (u128)rb <= (u128)UINTPTR_MAX) expect(false, r + (uintptr_t)rb, wb, r, rb, "(g) the write starts exactly where the read ends");
    for (int64_t shift = -e; shift <= rb + e; shift += e)                               // (h): nothing is written, wherever `out` points
        if ((u128)r + (u128)(shift < 0 ? 0 : shift) <= (u128)UINTPTR_MAX) expect(false, r + (uintptr_t)shift, 0, r, rb, "(h) an empty operand");
}

int main() {
    const int64_t elements[] = {1, 2, 3, 7, 64, 1000};
    const int64_t sizes[] = {1, 3, 4, 12};
    for (int64_t e : sizes)
        for (int64_t rn : elements)
            for (int64_t wn : elements) {
                const int64_t rb = rn * e, wb = wn * e;
                arrangements(1u << 20, rn, wn, e);
                arrangements((uintptr_t)1 << 47, rn, wn, e);                              // a device address
                arrangements(UINTPTR_MAX - (uintptr_t)rb, rn, wn, e);                   // the read ends at UINTPTR_MAX
                arrangements(UINTPTR_MAX - (uintptr_t)rb + 1, rn, wn, e);               // ... and with the last byte of the address space
                (void)wb;
            }
    // every pair of short ranges near the bottom and at the very top of the address space, lengths 0 .. 8 and a negative one
    const uintptr_t bases[] = {1, 4096, UINTPTR_MAX - 40};
    for (uintptr_t base : bases)
        for (uintptr_t a = 0; a < 24; ++a)
            for (uintptr_t b = 0; b < 24; ++b)
                for (int64_t na = -1; na <= 8; ++na)
                    for (int64_t nb = -1; nb <= 8; ++nb) {
                        if ((u128)base + a + (u128)(na < 0 ? 0 : na) > (u128)UINTPTR_MAX + 1) continue;      // no operand leaves the address space
                        if ((u128)base + b + (u128)(nb < 0 ? 0 : nb) > (u128)UINTPTR_MAX + 1) continue;
                        check(base + a, na, base + b, nb);
                    }
    // the longest ranges there are
    expect(true, 1, INT64_MAX, 2, 1, "a range of INT64_MAX bytes from 1 holds 2");
    expect(true, 16, INT64_MAX, (uintptr_t)INT64_MAX + 15, 1, "... and its last byte");
    expect(false, 16, INT64_MAX, (uintptr_t)INT64_MAX + 16, 1, "... and not the byte after it");
    expect(true, (uintptr_t)INT64_MAX + 2, INT64_MAX, UINTPTR_MAX, 1, "a range that ends with the address space holds its last byte");
    expect(false, (uintptr_t)INT64_MAX + 2, INT64_MAX, 1, INT64_MAX, "two halves of the address space");
    expect(false, (uintptr_t)INT64_MAX + 2, INT64_MAX, 2, INT64_MAX, "... that touch");
    expect(true, (uintptr_t)INT64_MAX + 2, INT64_MAX, 3, INT64_MAX, "... moved by one more byte");
    // a null pointer is an operand that is not there
    expect(false, 0, 100, 50, 100, "a null operand");
    expect(false, 0, 100, 0, 100, "two null operands");

    // vrg_operand_bytes: count * each, 0 for nothing, INT64_MAX where the product does not fit
    const int64_t counts[] = {-1, 0, 1, 2, 3, 32768, (int64_t)1 << 31, (int64_t)1 << 40, INT64_MAX / 12, INT64_MAX / 12 + 1, INT64_MAX};
    for (int64_t count : counts)
        for (int64_t each : counts) {
            const u128 exact = count > 0 && each > 0 ? (u128)count * (u128)each : 0;
            const int64_t want = exact > (u128)INT64_MAX ? INT64_MAX : (int64_t)exact;
            if (vrg_operand_bytes(count, each) != want) {
                std::fprintf(stderr, "overlap_check: vrg_operand_bytes(%lld, %lld) = %lld\n", (long long)count, (long long)each,
                             (long long)vrg_operand_bytes(count, each));
                return 1;
            }
            ++checked;
        }
    std::printf("overlap_check: %ld cases agree with the 128-bit interval test\n", checked);
    return 0;
}
