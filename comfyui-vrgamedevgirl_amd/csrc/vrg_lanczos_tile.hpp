// vrg_lanczos_tile.hpp -- the byte tile filter of cv2.resize(..., INTER_LANCZOS4), device only: k_lanczos4_tile (csrc/vrg_lanczos.hip) and
// k_msr_tile (csrc/vrg_msr.hip) are built on it.  Arithmetic: csrc/vrg_lanczos_math.hpp (integer, exact).
//
// A workgroup of 256 threads filters a tile of output pixels through LDS:
//   stage       lz_stage_records: the tile's column and row records (s, eight int16 as four dwords) from the table into LDS;
//   horizontal  one thread = one (source row, column).  The eight source pixels are 24 consecutive bytes = six unaligned dword loads
//               (lz_window; a column whose taps are clamped at a frame edge gathers byte by byte), the byte pairs of taps 2k, 2k + 1 are
//               lined up with v_perm_b32 and multiplied with the int16 weight pair by v_dot2_i32_i16 (lz_hsum3): 4 + 4 instructions per
//               channel instead of 8 extracts + 8 multiply-adds.  The caller keeps the sums (|h| < 2^20) in LDS as int32, channel-planar:
//               consecutive lanes hit consecutive banks;
//   vertical    one thread = one output pixel: lz_unpack_weights, then per channel eight LDS rows through v_mad_i32_i24 (|h| < 2^23,
//               |w| < 2^12: exact, and full rate where v_mul_lo_i32 is not) and FixedPtCast (lz_vsum).
// Which source rows a tile holds and where the row of tap k lies -- consecutive rows, or the slots of a strip plan -- is the caller's:
// lz_vsum asks a callable for the sum of tap k.
#pragma once
#include "vrg_common.hpp"
#include "vrg_lanczos_math.hpp"

namespace vrg {

VRG_D int32_t lz_dot2(uint32_t pair, uint32_t w, int32_t acc) {
    typedef short lz_s2 __attribute__((ext_vector_type(2)));
    lz_s2 a, b;
    __builtin_memcpy(&a, &pair, 4);
    __builtin_memcpy(&b, &w, 4);
    return __builtin_amdgcn_sdot2(a, b, acc, false);
}

// bytes j0 and j1 of the 24-byte window d[6] as (byte j0) | (byte j1) << 16
template <int J0, int J1>
VRG_D uint32_t lz_pair(const uint32_t (&d)[6]) {
    constexpr uint32_t sel = 0x0c000c00u | (uint32_t)(J0 & 3) | ((uint32_t)(4 + (J1 & 3)) << 16);
    return __builtin_amdgcn_perm(d[J1 >> 2], d[J0 >> 2], sel);
}

template <int C>
VRG_D int32_t lz_hsum_window(const uint32_t (&d)[6], const uint32_t (&w)[4]) {
    int32_t acc = 0;
    acc = lz_dot2(lz_pair<C, C + 3>(d), w[0], acc);
    acc = lz_dot2(lz_pair<C + 6, C + 9>(d), w[1], acc);
    acc = lz_dot2(lz_pair<C + 12, C + 15>(d), w[2], acc);
    acc = lz_dot2(lz_pair<C + 18, C + 21>(d), w[3], acc);
    return acc;
}

// The records of columns x0 .. x0 + CW - 1 and rows y0 .. y0 + CH - 1 (clamped to the picture) of the table at `taps`: out_w column records,
// then out_h row records.  All 256 threads call it; the caller's barrier follows.
template <int CW, int CH>
VRG_D void lz_stage_records(const uint32_t* __restrict__ taps, int32_t x0, int32_t y0, int32_t out_w, int32_t out_h, int tid, int32_t (&cs)[CW],
                            uint32_t (&cw)[CW][4], int32_t (&rs)[CH], uint32_t (&rw)[CH][4]) {
    for (int i = tid; i < CW + CH; i += 256) {
        const bool col = i < CW;
        const int l = col ? i : i - CW;
        const int32_t gi = col ? lz_clampi(x0 + l, out_w - 1) : out_w + lz_clampi(y0 + l, out_h - 1);
        const uint32_t* e = taps + (int64_t)gi * 5;
        if (col) {
            cs[l] = (int32_t)e[0];
#pragma unroll
            for (int k = 0; k < 4; ++k) cw[l][k] = e[1 + k];
        } else {
            rs[l] = (int32_t)e[0];
#pragma unroll
            for (int k = 0; k < 4; ++k) rw[l][k] = e[1 + k];
        }
    }
}

// pixels s - 3 .. s + 4 (clamped to the row) of the source row at `src` as 24 bytes
VRG_D void lz_window(const uint8_t* __restrict__ src, int32_t s, int32_t in_w, uint32_t (&d)[6]) {
    if (s >= 3 && s <= in_w - 5) {
        __builtin_memcpy(d, src + (int64_t)(s - 3) * 3, 24);
    } else {
#pragma unroll
        for (int q = 0; q < 6; ++q) d[q] = 0u;
#pragma unroll
        for (int k = 0; k < LZ_TAPS; ++k) {
            const uint8_t* px = src + (int64_t)lz_clampi(s - 3 + k, in_w - 1) * 3;
#pragma unroll
            for (int c = 0; c < 3; ++c) d[(3 * k + c) >> 2] |= (uint32_t)px[c] << (8 * ((3 * k + c) & 3));
        }
    }
}

// the three channel sums of a window under the four weight dwords of its column's record
VRG_D void lz_hsum3(const uint32_t (&d)[6], const uint32_t (&cw)[4], int32_t (&h)[3]) {
    const uint32_t w[4] = {cw[0], cw[1], cw[2], cw[3]};
    h[0] = lz_hsum_window<0>(d, w);
    h[1] = lz_hsum_window<1>(d, w);
    h[2] = lz_hsum_window<2>(d, w);
}

VRG_D void lz_unpack_weights(const uint32_t (&rw)[4], int32_t (&wk)[LZ_TAPS]) {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        wk[2 * k] = (int32_t)(int16_t)(rw[k] & 0xffffu);
        wk[2 * k + 1] = (int32_t)rw[k] >> 16;
    }
}

// one channel of one output pixel: h(k) = the horizontal sum of tap k in the pixel's column
template <class H>
VRG_D uint8_t lz_vsum(const int32_t (&wk)[LZ_TAPS], H h) {
    uint32_t v = 0;
#pragma unroll
    for (int k = 0; k < LZ_TAPS; ++k) v += (uint32_t)__mul24(h(k), wk[k]);
    return lz_cast((int32_t)v);
}

}  // namespace vrg
