// vrg_thumbs.hip -- the input of the landmark estimator (VRGDGFaceFixCompositeLandmarkAligned._landmarks, VRGDG_StandaloneFaceFixNodes.py:
// 955-979 of the reference): the 320 x 320 B,G,R thumbnails cv2.cvtColor(cv2.resize(rgb, (320, 320), INTER_AREA), COLOR_RGB2BGR) makes of
// the packed face images of vrg_face_bytes_u8, for a list of descriptors in one launch.  gfx950 only.  Arithmetic: csrc/vrg_grid_math.hpp
// (nothing of its own: csrc/vrg_thumbs_math.hpp holds the descriptor's rules and the host loop).
//
// k_face_thumbs: one workgroup (four waves) = 64 columns of one row of one thumbnail, 5 x 320 workgroups per descriptor, on the source walk
// of csrc/vrg_area_walk.hpp with the rule of the descriptor: byte sources with three channels, read swapped (output channel c reads channel
// 2 - c), every lane owns a column; the image starts at any byte, so the row buffer keeps the phase of the address mod 16.  The
// workgroup's 192 bytes are put together in LDS and leave as twelve 16-byte stores, always aligned: 192, 960 and 307,200 are multiples of
// 16 and `out` is 16-byte aligned.  Every byte of a thumbnail is written once.  When both axes shrink a source byte is read once, twice for
// the rows two output rows share; when an axis enlarges (a box below 320: at most 307 KB) the one or two source rows of an output row are
// read again by its neighbours, out of the cache.
#include "vrg_common.hpp"
#include "vrg_area_walk.hpp"
#include "vrg_thumbs_math.hpp"

namespace vrg {

constexpr int TH_OUT_BYTES = 256;                                              // the bytes of the workgroup (192 used)
constexpr int TH_HEAD_BYTES = WALK_PART_BYTES + WALK_CELL_BYTES + TH_OUT_BYTES;
constexpr int TH_ROWBUF = GRID_ROW_VALUES + 16;                                // a staged byte lies at the byte phase of its source
constexpr int TH_LDS_BYTES = TH_HEAD_BYTES + WALK_WAVES * TH_ROWBUF;
static_assert(TH_HEAD_BYTES % 16 == 0 && TH_ROWBUF % 16 == 0 && (WALK_PART_BYTES + WALK_CELL_BYTES) % 16 == 0,
              "the row buffers and the output bytes start on a 16-byte boundary");

__global__ __launch_bounds__(WALK_THREADS) void k_face_thumbs(const uint8_t* __restrict__ generated, const uint8_t* __restrict__ source,
                                                            int64_t n_bytes, const vrg_thumb_desc* __restrict__ descs,
                                                            uint8_t* __restrict__ out) {
    __shared__ __attribute__((aligned(16))) uint8_t lds[TH_LDS_BYTES];
    uint32_t* part = reinterpret_cast<uint32_t*>(lds);                        // [2][WALK_WAVES][WALK_VALUES]
    AreaCell* xc = reinterpret_cast<AreaCell*>(lds + WALK_PART_BYTES);        // [64]
    uint8_t* ob = lds + WALK_PART_BYTES + WALK_CELL_BYTES;
    const int tid = (int)threadIdx.x, wave = tid >> 6, lane = tid & 63;
    uint8_t* rb = lds + TH_HEAD_BYTES + wave * TH_ROWBUF;

    const vrg_thumb_desc d = descs[blockIdx.y];
    const int seg = (int)(blockIdx.x % (uint32_t)THUMB_SEGMENTS), ty = (int)(blockIdx.x / (uint32_t)THUMB_SEGMENTS);
    const int tx0 = seg * GRID_LANES;
    // a descriptor the host check refuses writes nothing (workgroup-uniform)
    const uint8_t* image = d.which == 0 ? generated : (d.which == 1 ? source : nullptr);
    if (!image || !d.xtab || !d.ytab || d.mode < GRID_COPY || d.mode > GRID_LINEAR || !thumb_image_fits(d.offset, d.box_w, d.box_h, n_bytes)) return;
    image += d.offset;
    const int mode = d.mode, W = d.box_w;

    xc[lane] = walk_clamped(reinterpret_cast<const AreaCell*>(d.xtab)[tx0 + lane], W);      // the four waves write the same 64 records
    const AreaCell yc = walk_clamped(reinterpret_cast<const AreaCell*>(d.ytab)[ty], d.box_h);
    __syncthreads();
    const AreaCell m = xc[lane];
    const int cps = d.cps < 1 ? 1 : (d.cps > GRID_LANES ? GRID_LANES : d.cps);

    WalkSums s{0, 0, 0};
    const int batches = (yc.count + WALK_WAVES - 1) / WALK_WAVES;
    for (int b = 0; b < batches; ++b) {
        const int r = b * WALK_WAVES + wave;
        if (r < yc.count)                                                      // wave-uniform
            walk_row<grid_quant, true>(image + (int64_t)(yc.first + r) * W * 3, 3, mode, xc, GRID_LANES, lane, m, cps, rb, GRID_ROW_VALUES, lane,
                                       walk_words(part, b, wave, lane));
        walk_fold(part, b, tid, mode, yc, s);
    }

    // the 192 bytes of this workgroup: value tid = column tx0 + tid / 3, channel tid % 3 (B, G, R)
    if (tid < WALK_VALUES) ob[tid] = walk_byte(s, mode, yc, d.inv);
    __syncthreads();
    if (tid < WALK_VALUES / 16) {
        uint8_t* dst = out + (int64_t)blockIdx.y * THUMB_BYTES + (int64_t)ty * THUMB_ROW_BYTES + tx0 * 3;
        reinterpret_cast<walk_u4*>(dst)[tid] = reinterpret_cast<const walk_u4*>(ob)[tid];
    }
}

}  // namespace vrg

using namespace vrg;

extern "C" {

int vrg_face_thumbs_check(const vrg_thumb_desc* desc_host, int64_t n_desc, int64_t n_bytes, int has_source) {
    if (n_desc < 0 || n_bytes < 0 || (n_desc > 0 && !desc_host)) return VRG_ERR_BAD_ARG;
    for (int64_t i = 0; i < n_desc; ++i)
        if (!thumb_desc_ok(desc_host[i], n_bytes, has_source != 0)) return VRG_ERR_BAD_ARG;
    return VRG_OK;
}

int vrg_face_thumbs_u8(const uint8_t* generated, const uint8_t* source, int64_t n_bytes, const vrg_thumb_desc* desc, int64_t n_desc,
                       uint8_t* out, void* stream) {
    if (n_desc < 0 || n_bytes < 0) return VRG_ERR_BAD_ARG;
    if (n_desc == 0) return VRG_OK;
    if (!generated || !desc || !out || (reinterpret_cast<uintptr_t>(desc) & 7u) != 0 || (reinterpret_cast<uintptr_t>(out) & 15u) != 0) return VRG_ERR_BAD_ARG;
    if (n_desc > INT64_MAX / THUMB_BYTES) return VRG_ERR_BAD_ARG;
    if (vrg_ranges_overlap(out, n_desc * THUMB_BYTES, generated, n_bytes) || vrg_ranges_overlap(out, n_desc * THUMB_BYTES, source, n_bytes)) return VRG_ERR_BAD_ARG;
    return launch_chunks(n_desc, [&](int64_t first, int64_t count) -> int {
        hipLaunchKernelGGL(k_face_thumbs, dim3((uint32_t)(THUMB_SEGMENTS * THUMB_SIDE), (uint32_t)count), dim3(WALK_THREADS), 0, (hipStream_t)stream,
                           generated, source, n_bytes, desc + first, out + first * THUMB_BYTES);
        VRG_CHECK_LAUNCH();
        return VRG_OK;
    });
}

}  // extern "C"
