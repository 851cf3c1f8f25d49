// vrg_lanczos.hip -- the stand-alone enhancer's upscale (VRGDG_StandaloneVideoEnhancerNodes.py:213-230: cv2.resize(..., INTER_LANCZOS4) on
// decoded B,G,R bytes) and the same upscale fused into the loop body that follows it (/ 255 -> unsharp -> per-frame-seeded grain -> * 255
// clip truncate, :311-324 and :278-294).  gfx950 only.  Arithmetic: csrc/vrg_lanczos_math.hpp (integer, exact) and the shared byte pipeline
// of csrc/vrg_pixel_math.hpp (sharpen_grain_byte: what k_sharpen_grain_u8 evaluates).
//
// k_lanczos4_tile: one workgroup = one 64 x 32 tile of output pixels (HALO = 1: plus a one-pixel ring) of one frame, on the tile filter of
// csrc/vrg_lanczos_tile.hpp, whose comment describes the staging and the two filter passes.  What is this kernel's own:
//   pass 1  the source rows are the consecutive rows s(first) - 3 .. s(last) + 4 that the tile's output rows touch, clamped on use;
//   pass 2  HALO = 0 stores the bytes; HALO = 1 keeps them in LDS, the ring outside the frame being the replicated edge pixel (the clamped
//           coordinate) or zero bytes;
//   pass 3  (HALO = 1) one thread = one pixel: 3 x 3 window per channel from the LDS bytes, sharpen_grain_byte, three normals of
//           torch.randn's stream per pixel by the general per-element form (torch_randn_element: one Philox call per element -- the
//           sibling elements of a call lie G elements apart, outside any tile).
// LDS: 44 rows x 3 x 66 x 4 B = 34.8 KB of sums + 6.7 KB of bytes + 2.5 KB of records.
// A tile whose rows span more than LZ_MAXROWS source rows (vertical ratios below about 0.9) is not tiled: vrg_lanczos4_u8 runs the plain
// per-pixel kernel, vrg_upscale_sharpen_grain_u8 reports VRG_ERR_UNSUPPORTED and the caller runs the two entry points.
#include "vrg_common.hpp"
#include "vrg_lanczos_tile.hpp"

namespace vrg {

constexpr int LZ_TW = 64, LZ_TH = 32, LZ_MAXROWS = 44;

struct LzGeom {
    int32_t in_h, in_w, out_h, out_w, tiles_x, tiles_y;
};

template <int HALO>
struct LzShared {
    static constexpr int CW = LZ_TW + 2 * HALO, CH = LZ_TH + 2 * HALO;
    int32_t h[LZ_MAXROWS][3][CW];
    int32_t cs[CW], rs[CH];
    uint32_t cw[CW][4], rw[CH][4];
    uint8_t ub[HALO ? CH : 1][HALO ? CW * 3 + 2 : 4];
};

template <int HALO, bool ZERO, bool SHARP, bool GRAIN>
__global__ __launch_bounds__(256) void k_lanczos4_tile(const uint8_t* __restrict__ in, uint8_t* __restrict__ out, const uint32_t* __restrict__ taps,
                                                        LzGeom g, NoiseK nk, float strength, float I, float S, float T) {
    typedef LzShared<HALO> Sh;
    constexpr int CW = Sh::CW, CH = Sh::CH;
    __shared__ Sh sh;
    const uint32_t tid = threadIdx.x;
    const uint32_t tpf = (uint32_t)g.tiles_x * (uint32_t)g.tiles_y;
    const uint32_t frame = blockIdx.x / tpf;
    const uint32_t rem = blockIdx.x - frame * tpf;
    const uint32_t ty = rem / (uint32_t)g.tiles_x, tx = rem - ty * (uint32_t)g.tiles_x;
    const int32_t x0 = (int32_t)tx * LZ_TW, y0 = (int32_t)ty * LZ_TH;
    const int32_t in_pitch = g.in_w * 3;
    const uint8_t* fin = in + (int64_t)frame * g.in_h * in_pitch;
    uint8_t* fout = out + (int64_t)frame * g.out_h * g.out_w * 3;

    lz_stage_records(taps, x0 - HALO, y0 - HALO, g.out_w, g.out_h, (int)tid, sh.cs, sh.cw, sh.rs, sh.rw);
    __syncthreads();
    const int32_t r0 = sh.rs[0] - 3;
    int32_t nrows = sh.rs[CH - 1] + 4 - r0 + 1;
    nrows = nrows < LZ_MAXROWS ? nrows : LZ_MAXROWS;                   // the entry point has checked it: never taken

    // pass 1: horizontal
    for (int it = (int)tid; it < nrows * CW; it += 256) {
        const int row = it / CW, col = it - row * CW;
        const uint8_t* src = fin + (int64_t)lz_clampi(r0 + row, g.in_h - 1) * in_pitch;
        uint32_t d[6];
        int32_t h[3];
        lz_window(src, sh.cs[col], g.in_w, d);
        lz_hsum3(d, sh.cw[col], h);
#pragma unroll
        for (int c = 0; c < 3; ++c) sh.h[row][c][col] = h[c];
    }
    __syncthreads();

    // pass 2: vertical
    for (int it = (int)tid; it < CH * CW; it += 256) {
        const int ly = it / CW, lx = it - ly * CW;
        const int32_t gy = y0 + ly - HALO, gx = x0 + lx - HALO;
        const bool inside = gx >= 0 && gx < g.out_w && gy >= 0 && gy < g.out_h;
        if (HALO == 0 && !inside) continue;
        int32_t base = sh.rs[ly] - 3 - r0;
        base = base < 0 ? 0 : (base > LZ_MAXROWS - LZ_TAPS ? LZ_MAXROWS - LZ_TAPS : base);     // never taken (see nrows)
        int32_t wk[LZ_TAPS];
        lz_unpack_weights(sh.rw[ly], wk);
        uint8_t o[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) o[c] = lz_vsum(wk, [&](int k) { return sh.h[base + k][c][lx]; });
        if (HALO == 0) {
            uint8_t* dst = fout + ((int64_t)gy * g.out_w + gx) * 3;
            dst[0] = o[0]; dst[1] = o[1]; dst[2] = o[2];
        } else {
#pragma unroll
            for (int c = 0; c < 3; ++c) sh.ub[ly][lx * 3 + c] = (ZERO && !inside) ? (uint8_t)0 : o[c];
        }
    }
    if (HALO == 0) return;
    __syncthreads();

    // pass 3: / 255 -> unsharp -> grain -> bytes
    const uint64_t seed = GRAIN ? chunk_seed(nk, frame) : 0, off = GRAIN ? chunk_offset(nk, frame) : 0;
    for (int it = (int)tid; it < LZ_TH * LZ_TW; it += 256) {
        const int ly = it / LZ_TW, lx = it - ly * LZ_TW;
        const int32_t gy = y0 + ly, gx = x0 + lx;
        if (gx >= g.out_w || gy >= g.out_h) continue;
        const uint64_t li = ((uint64_t)gy * (uint64_t)g.out_w + (uint64_t)gx) * 3u;
        float n[3] = {0.0f, 0.0f, 0.0f};
        if (GRAIN) {
#pragma unroll
            for (int c = 0; c < 3; ++c) n[c] = torch_randn_element(seed, off, nk.G, li + (uint64_t)c);
        }
        uint8_t* dst = fout + li;
#pragma unroll
        for (int j = 0; j < 3; ++j) {                                  // byte j of the B,G,R pixel = element 2 - j of the R,G,B tensor
            float p[3][3];
#pragma unroll
            for (int r = 0; r < 3; ++r)
#pragma unroll
                for (int k = 0; k < 3; ++k) p[r][k] = unit_from_u8(sh.ub[ly + r][(lx + k) * 3 + j]);
            dst[j] = sharpen_grain_byte<SHARP, GRAIN>(p, strength, ZERO ? 1 : 0, n[2 - j], n[1], 2 - j, I, S, T);
        }
    }
}

// Any ratio, any size: one thread = one output pixel, straight from the definition (64 taps x 3 channels from L1 / L2).
__global__ __launch_bounds__(256) void k_lanczos4_pixel(const uint8_t* __restrict__ in, uint8_t* __restrict__ out, const LzTap* __restrict__ taps,
                                                         LzGeom g, int64_t total_px) {
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= total_px) return;
    const int64_t per = (int64_t)g.out_h * g.out_w;
    const int64_t frame = p / per;
    const int32_t r = (int32_t)(p - frame * per);
    const int32_t y = r / g.out_w, x = r - y * g.out_w;
    const uint8_t* fin = in + frame * (int64_t)g.in_h * g.in_w * 3;
    const LzTap cx = taps[x], ry = taps[g.out_w + y];
    uint8_t o[3];
    lz_pixel(cx, ry, g.in_w, g.in_h, [&](int32_t sy, int32_t sx, int c) { return fin[((int64_t)sy * g.in_w + sx) * 3 + c]; }, o);
    uint8_t* dst = out + p * 3;
    dst[0] = o[0]; dst[1] = o[1]; dst[2] = o[2];
}

// does every tile's row span fit the LDS rows?  (s is monotonic in the output row)
static bool lz_tileable(int32_t in_h, int32_t out_h, int halo) {
    for (int32_t y0 = 0; y0 < out_h; y0 += LZ_TH) {
        int32_t s_first, s_last;
        float t;
        lz_source(lz_clampi(y0 - halo, out_h - 1), in_h, out_h, s_first, t);
        lz_source(lz_clampi(y0 + LZ_TH - 1 + halo, out_h - 1), in_h, out_h, s_last, t);
        if (s_last - s_first + LZ_TAPS > LZ_MAXROWS) return false;
    }
    return true;
}

static bool lz_bad_geometry(const void* in, const void* out, const void* taps, int64_t frames, int32_t in_h, int32_t in_w, int32_t out_h, int32_t out_w) {
    if (!in || !out || in == out || !taps || (reinterpret_cast<uintptr_t>(taps) & 3u) != 0 || frames < 0 || in_h < 1 || in_w < 1 || out_h < 1 || out_w < 1)
        return true;
    return vrg_ranges_overlap(in, vrg_operand_bytes(frames, (int64_t)in_h * in_w * 3), out, vrg_operand_bytes(frames, (int64_t)out_h * out_w * 3));
}

}  // namespace vrg

using namespace vrg;

extern "C" {

int vrg_lanczos4_taps(int32_t in_h, int32_t in_w, int32_t out_h, int32_t out_w, void* taps_host) {
    if (!taps_host || in_h < 1 || in_w < 1 || out_h < 1 || out_w < 1) return VRG_ERR_BAD_ARG;
    lz_fill_taps(in_w, in_h, out_w, out_h, reinterpret_cast<LzTap*>(taps_host));
    return VRG_OK;
}

int vrg_lanczos4_u8(const uint8_t* in, uint8_t* out, int64_t frames, int32_t in_h, int32_t in_w, int32_t out_h, int32_t out_w, const void* taps,
                    void* stream) {
    if (lz_bad_geometry(in, out, taps, frames, in_h, in_w, out_h, out_w)) return VRG_ERR_BAD_ARG;
    if (frames == 0) return VRG_OK;
    if ((int64_t)out_h * out_w * 3 > 0x7fffffffll || (int64_t)in_h * in_w * 3 > 0x7fffffffll) return VRG_ERR_UNSUPPORTED;
    LzGeom g{in_h, in_w, out_h, out_w, (out_w + LZ_TW - 1) / LZ_TW, (out_h + LZ_TH - 1) / LZ_TH};
    const int64_t in_fe = (int64_t)in_h * in_w * 3, out_fe = (int64_t)out_h * out_w * 3;
    if (!lz_tileable(in_h, out_h, 0)) {
        const int64_t per = (int64_t)out_h * out_w;
        const int64_t step = (0x7fffffffll * 256 - 255) / per;             // frames per launch
        if (step < 1) return VRG_ERR_UNSUPPORTED;
        for (int64_t f0 = 0; f0 < frames; f0 += step) {
            const int64_t nf = frames - f0 < step ? frames - f0 : step;
            const int64_t total = nf * per;
            hipLaunchKernelGGL(k_lanczos4_pixel, dim3((uint32_t)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, in + f0 * in_fe,
                               out + f0 * out_fe, reinterpret_cast<const LzTap*>(taps), g, total);
            VRG_CHECK_LAUNCH();
        }
        return VRG_OK;
    }
    const int64_t tpf = (int64_t)g.tiles_x * g.tiles_y;
    const int64_t step = 0x7fffffffll / tpf;
    if (step < 1) return VRG_ERR_UNSUPPORTED;
    const NoiseK nk{};
    for (int64_t f0 = 0; f0 < frames; f0 += step) {
        const int64_t nf = frames - f0 < step ? frames - f0 : step;
        hipLaunchKernelGGL((k_lanczos4_tile<0, false, false, false>), dim3((uint32_t)(nf * tpf)), dim3(256), 0, (hipStream_t)stream, in + f0 * in_fe,
                           out + f0 * out_fe, reinterpret_cast<const uint32_t*>(taps), g, nk, 0.0f, 0.0f, 0.0f, 0.0f);
        VRG_CHECK_LAUNCH();
    }
    return VRG_OK;
}

int vrg_upscale_sharpen_grain_u8(const uint8_t* in, uint8_t* out, int64_t frames, int32_t in_h, int32_t in_w, int32_t out_h, int32_t out_w,
                                 const void* taps, float strength, int32_t border, float intensity, float sat, float one_minus_sat,
                                 const vrg_noise_desc* nd, void* stream) {
    const bool grain = intensity > 0.0f, sharp = strength > 0.0f;
    if (lz_bad_geometry(in, out, taps, frames, in_h, in_w, out_h, out_w) || border < 0 || border > 1) return VRG_ERR_BAD_ARG;
    if (grain && (!nd || nd->chunk_frames < 1 || nd->grid_threads == 0 || (nd->grid_threads % 256u) != 0)) return VRG_ERR_BAD_ARG;
    if (frames == 0) return VRG_OK;
    const int64_t in_fe = (int64_t)in_h * in_w * 3, out_fe = (int64_t)out_h * out_w * 3;
    if (out_fe > 0x7fffffffll || in_fe > 0x7fffffffll || (grain && nd->chunk_frames != 1) || !lz_tileable(in_h, out_h, 1)) return VRG_ERR_UNSUPPORTED;
    LzGeom g{in_h, in_w, out_h, out_w, (out_w + LZ_TW - 1) / LZ_TW, (out_h + LZ_TH - 1) / LZ_TH};
    const int64_t tpf = (int64_t)g.tiles_x * g.tiles_y;
    const int64_t step = 0x7fffffffll / tpf;
    if (step < 1) return VRG_ERR_UNSUPPORTED;
    NoiseK nk{};
    if (grain) nk = make_noise(nd, out_fe);
    const bool zero = border == VRG_BORDER_ZERO;
    for (int64_t f0 = 0; f0 < frames; f0 += step) {
        const int64_t nf = frames - f0 < step ? frames - f0 : step;
        NoiseK nkk = nk;
        nkk.chunk0 += f0;
#define VRG_LZ_LAUNCH(Z, S_, G_)                                                                                                              \
    hipLaunchKernelGGL((k_lanczos4_tile<1, Z, S_, G_>), dim3((uint32_t)(nf * tpf)), dim3(256), 0, (hipStream_t)stream, in + f0 * in_fe,        \
                       out + f0 * out_fe, reinterpret_cast<const uint32_t*>(taps), g, nkk, strength, intensity, sat, one_minus_sat)
        if (zero) {
            if (sharp && grain) VRG_LZ_LAUNCH(true, true, true);
            else if (sharp) VRG_LZ_LAUNCH(true, true, false);
            else if (grain) VRG_LZ_LAUNCH(true, false, true);
            else VRG_LZ_LAUNCH(true, false, false);
        } else {
            if (sharp && grain) VRG_LZ_LAUNCH(false, true, true);
            else if (sharp) VRG_LZ_LAUNCH(false, true, false);
            else if (grain) VRG_LZ_LAUNCH(false, false, true);
            else VRG_LZ_LAUNCH(false, false, false);
        }
#undef VRG_LZ_LAUNCH
        VRG_CHECK_LAUNCH();
    }
    return VRG_OK;
}

}  // extern "C"
