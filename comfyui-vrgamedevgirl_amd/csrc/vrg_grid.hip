// vrg_grid.hip -- the Video Folder Grid Plot (VRGDG_VideoFolderGridPlot, LTXLoraTrain.py:7926-8314 of the reference): every tile of every
// output frame quantised, resized as cv2.resize(..., INTER_AREA) does on bytes and written as fp32 / 255 straight into its place in the grid
// frame, with the letterbox bars, the label band and the empty cells, in one launch.  gfx950 only.  Arithmetic: csrc/vrg_grid_math.hpp.
//
// k_grid_tiles: one workgroup (four waves) = 64 tile columns of one tile row of one descriptor (one tile of one output frame), so a row of
// any width is a row of workgroups.  A row of the band takes the overlay's bytes, a row of the picture is computed, everything else is 0;
// the workgroup leaves its <= 192 bytes in LDS and stores (float)byte / 255 for all of them: every float of the grid is written once.
//   The picture rows go through the source walk of csrc/vrg_area_walk.hpp with the rule of the descriptor: fp32 sources are quantised by
//   grid_quant (truncation) as they are staged, decoded byte frames are B,G,R and read swapped; the lanes of the picture columns [d_lo,
//   d_hi) of this workgroup own a column each.
//   The store goes in 16-byte pieces from the first 16-byte boundary of the destination on, the floats in front of and behind them one by
//   one: a tile may start anywhere on the 4-byte grid.
// There is no row buffer for the output.  The row buffer of a wave holds GRID_ROW_VALUES source values: when the 64 columns of a workgroup
// need more, they go through it desc.cps columns at a time; the taps of ONE column must fit it (vrg_grid_plan refuses the rest), the
// width of a source as such is not bounded: a row wider than the buffer is split across workgroups and, inside one, into these
// segments.  The source is read once (rows that two output rows share are read by both); 12 B per source pixel with C = 3.
#include "vrg_common.hpp"
#include "vrg_area_walk.hpp"

namespace vrg {

constexpr int GRID_UNIT_BYTES = 256 * 4;                                       // k / 255
constexpr int GRID_OUT_BYTES = 256;                                            // the bytes of the workgroup (192 used)
constexpr int GRID_HEAD_BYTES = WALK_PART_BYTES + WALK_CELL_BYTES + GRID_UNIT_BYTES + GRID_OUT_BYTES;
constexpr int GRID_ROWBUF = GRID_ROW_VALUES + 16;                              // a staged value lies at the byte phase of its source
constexpr int GRID_LDS_BYTES = GRID_HEAD_BYTES + WALK_WAVES * GRID_ROWBUF;
static_assert(GRID_HEAD_BYTES % 16 == 0 && GRID_ROWBUF % 16 == 0, "the row buffers start on a 16-byte boundary");

struct GridGeom {
    int64_t frames;
    int32_t cell_w, cell_h, grid_w, grid_h, segments;
};

template <typename T>
__global__ __launch_bounds__(WALK_THREADS) void k_grid_tiles(const vrg_grid_desc* __restrict__ descs, float* __restrict__ out, GridGeom g) {
    constexpr bool SWAP = sizeof(T) == 1;                                      // decoded frames are B,G,R
    __shared__ __attribute__((aligned(16))) uint8_t lds[GRID_LDS_BYTES];
    uint32_t* part = reinterpret_cast<uint32_t*>(lds);                        // [2][WALK_WAVES][WALK_VALUES]
    AreaCell* xc = reinterpret_cast<AreaCell*>(lds + WALK_PART_BYTES);        // [64]
    float* unit = reinterpret_cast<float*>(lds + WALK_PART_BYTES + WALK_CELL_BYTES);
    uint8_t* ob = lds + WALK_PART_BYTES + WALK_CELL_BYTES + GRID_UNIT_BYTES;
    const int tid = (int)threadIdx.x, wave = tid >> 6, lane = tid & 63;
    uint8_t* rb = lds + GRID_HEAD_BYTES + wave * GRID_ROWBUF;

    const vrg_grid_desc d = descs[blockIdx.y];
    const int seg = (int)(blockIdx.x % (uint32_t)g.segments), ty = (int)(blockIdx.x / (uint32_t)g.segments);
    const int tx0 = seg * GRID_LANES;
    const int ncol = g.cell_w - tx0 < GRID_LANES ? g.cell_w - tx0 : GRID_LANES;
    // a tile outside the grid writes nothing (vrg_grid_check refuses it on the host)
    if (d.frame < 0 || (int64_t)d.frame >= g.frames || d.dst_x < 0 || d.dst_y < 0 || d.dst_x > g.grid_w - g.cell_w || d.dst_y > g.grid_h - g.cell_h) return;

    unit[tid] = grid_unit(tid);
    const int C = d.channels, mode = d.mode;
    // picture: the geometry must lie inside the tile, else the tile has none
    const bool geometry = d.src && d.new_w >= 1 && d.new_h >= 1 && d.x_off >= 0 && d.y_off >= 0 && d.x_off <= g.cell_w - d.new_w &&
                          d.y_off <= g.cell_h - d.new_h && d.xtab && d.ytab && d.height >= 1 && d.width >= 1 && (C == 3 || (C == 4 && !SWAP)) &&
                          mode >= GRID_COPY && mode <= GRID_LINEAR;
    int d_lo = tx0 - d.x_off, d_hi = tx0 + ncol - d.x_off;                     // the picture columns [d_lo, d_hi) of this workgroup
    d_lo = d_lo < 0 ? 0 : d_lo;
    d_hi = d_hi > d.new_w ? d.new_w : d_hi;
    const bool picture = geometry && ty >= d.y_off && ty < d.y_off + d.new_h && d_lo < d_hi;       // workgroup-uniform
    const int lane0 = d_lo + d.x_off - tx0;                                    // the lane of picture column d_lo

    WalkSums s{0, 0, 0};
    AreaCell yc{0, 0, 0.0f, 0.0f, 0.0f};
    if (picture) {
        const AreaCell* xt = reinterpret_cast<const AreaCell*>(d.xtab);
        const int nc = d_hi - d_lo;
        if (tid < nc) xc[tid] = walk_clamped(xt[d_lo + tid], d.width);
        yc = walk_clamped(reinterpret_cast<const AreaCell*>(d.ytab)[ty - d.y_off], d.height);
        __syncthreads();
        const int cl = lane - lane0;                                           // this lane's column of xc, if 0 <= cl < nc
        const AreaCell m = cl >= 0 && cl < nc ? xc[cl] : AreaCell{0, 0, 0.0f, 0.0f, 0.0f};
        const int cps = d.cps < 1 ? 1 : (d.cps > GRID_LANES ? GRID_LANES : d.cps);
        const T* fin = reinterpret_cast<const T*>(d.src);
        const int batches = (yc.count + WALK_WAVES - 1) / WALK_WAVES;
        for (int b = 0; b < batches; ++b) {
            const int r = b * WALK_WAVES + wave;
            if (r < yc.count)                                                  // wave-uniform
                walk_row<grid_quant, SWAP>(fin + (int64_t)(yc.first + r) * d.width * C, C, mode, xc, nc, cl, m, cps, rb, GRID_ROW_VALUES, lane,
                                           walk_words(part, b, wave, lane));
            walk_fold(part, b, tid, mode, yc, s);
        }
    }

    // the bytes of this workgroup's values: picture, overlay or nothing
    if (tid < WALK_VALUES) {
        const int col = tid / 3;                                               // tile column tx0 + col, channel tid - 3 * col
        uint8_t o = 0;
        if (col < ncol) {
            const int dcol = tx0 + col - d.x_off;
            if (picture && dcol >= 0 && dcol < d.new_w) {
                o = walk_byte(s, mode, yc, d.inv);
            } else if (d.overlay && ty < d.band) {
                o = d.overlay[((int64_t)ty * g.cell_w + tx0) * 3 + tid];
            }
        }
        ob[tid] = o;
    }
    __syncthreads();

    // (float)byte / 255 for the ncol * 3 values, 16-byte stores from the first 16-byte boundary on
    const int n = ncol * 3;
    float* dst = out + (((int64_t)d.frame * g.grid_h + d.dst_y + ty) * g.grid_w + d.dst_x + tx0) * 3;
    const int ph = (int)((reinterpret_cast<uintptr_t>(dst) >> 2) & 3u);
    int head = (4 - ph) & 3;
    head = head < n ? head : n;
    const int nq = (n - head) >> 2;
    if (wave == 0) {
        if (lane < head) dst[lane] = unit[ob[lane]];
        const int t = head + 4 * nq + lane;
        if (lane < 3 && t < n) dst[t] = unit[ob[t]];
    } else if (tid - 64 < nq) {
        const int i = head + 4 * (tid - 64);
        walk_f4 v;
        v.x = unit[ob[i]]; v.y = unit[ob[i + 1]]; v.z = unit[ob[i + 2]]; v.w = unit[ob[i + 3]];
        *reinterpret_cast<walk_f4*>(dst + i) = v;
    }
}

// is this descriptor one the kernel follows as the caller means it (host)
static bool grid_desc_ok(const vrg_grid_desc& d, bool bytes, int64_t frames, int32_t cell_w, int32_t cell_h, int32_t grid_w, int32_t grid_h) {
    if (d.frame < 0 || (int64_t)d.frame >= frames || d.dst_x < 0 || d.dst_y < 0 || d.dst_x > grid_w - cell_w || d.dst_y > grid_h - cell_h) return false;
    if (d.band < 0 || d.band > cell_h) return false;
    if (!d.src) return true;
    if (!d.xtab || !d.ytab || d.height < 1 || d.width < 1 || !(d.channels == 3 || (d.channels == 4 && !bytes))) return false;
    if ((reinterpret_cast<uintptr_t>(d.xtab) & 3u) || (reinterpret_cast<uintptr_t>(d.ytab) & 3u) || (!bytes && (reinterpret_cast<uintptr_t>(d.src) & 3u))) return false;
    if ((int64_t)d.height * d.width * d.channels > 0x7fffffffll) return false;
    if (d.new_w < 1 || d.new_h < 1 || d.x_off < 0 || d.y_off < d.band || d.x_off > cell_w - d.new_w || d.y_off > cell_h - d.new_h) return false;
    if (d.mode != grid_mode(d.height, d.width, d.new_h, d.new_w) || d.cps < 1 || d.cps > GRID_LANES) return false;
    return true;
}

template <typename T>
static int grid_launch(const vrg_grid_desc* desc, int64_t n_desc, float* out, int64_t frames, int32_t cell_w, int32_t cell_h, int32_t grid_w,
                       int32_t grid_h, void* stream) {
    if (n_desc < 0 || frames < 0 || cell_w < 1 || cell_h < 1 || grid_w < cell_w || grid_h < cell_h) return VRG_ERR_BAD_ARG;
    if (n_desc == 0 || frames == 0) return VRG_OK;
    if (!desc || !out || (reinterpret_cast<uintptr_t>(desc) & 7u) != 0 || (reinterpret_cast<uintptr_t>(out) & 3u) != 0) return VRG_ERR_BAD_ARG;
    GridGeom g{frames, cell_w, cell_h, grid_w, grid_h, (cell_w + GRID_LANES - 1) / GRID_LANES};
    if ((int64_t)g.segments * cell_h > 0x7fffffffll) return VRG_ERR_UNSUPPORTED;
    return launch_chunks(n_desc, [&](int64_t first, int64_t count) -> int {
        hipLaunchKernelGGL((k_grid_tiles<T>), dim3((uint32_t)(g.segments * cell_h), (uint32_t)count), dim3(WALK_THREADS), 0, (hipStream_t)stream,
                           desc + first, out, g);
        VRG_CHECK_LAUNCH();
        return VRG_OK;
    });
}

}  // namespace vrg

using namespace vrg;

extern "C" {

int vrg_grid_plan(int32_t in_h, int32_t in_w, int32_t channels, int32_t out_h, int32_t out_w, int32_t* mode, int32_t* cps, float* inv) {
    if (!mode || !cps || !inv || in_h < 1 || in_w < 1 || out_h < 1 || out_w < 1 || channels < 3 || channels > 4) return VRG_ERR_BAD_ARG;
    *mode = grid_mode(in_h, in_w, out_h, out_w);
    *inv = *mode == GRID_FAST || *mode == GRID_FAST_2X2 ? grid_fast_inv(in_h, in_w, out_h, out_w) : 1.0f;
    AreaCell* cells = new AreaCell[out_w];
    grid_fill_taps(in_w, out_w, *mode, cells);
    *cps = grid_cells_per_segment(cells, out_w, channels);
    delete[] cells;
    return *cps ? VRG_OK : VRG_ERR_UNSUPPORTED;
}

int vrg_grid_taps(int32_t n_in, int32_t n_out, int32_t mode, void* taps_host) {
    if (!taps_host || n_in < 1 || n_out < 1 || mode < GRID_COPY || mode > GRID_LINEAR) return VRG_ERR_BAD_ARG;
    if (mode == GRID_COPY && n_in != n_out) return VRG_ERR_BAD_ARG;
    int32_t step;
    if ((mode == GRID_FAST || mode == GRID_FAST_2X2) && (n_out > n_in || !grid_integer_scale(grid_scale(n_in, n_out), step))) return VRG_ERR_BAD_ARG;
    if (mode == GRID_GENERAL && n_out > n_in) return VRG_ERR_BAD_ARG;
    grid_fill_taps(n_in, n_out, mode, reinterpret_cast<AreaCell*>(taps_host));
    return VRG_OK;
}

int vrg_grid_check(const vrg_grid_desc* desc_host, int64_t n_desc, int32_t bytes, int64_t frames, int32_t cell_w, int32_t cell_h, int32_t grid_w,
                   int32_t grid_h) {
    if (n_desc < 0 || frames < 0 || cell_w < 1 || cell_h < 1 || grid_w < cell_w || grid_h < cell_h || (n_desc > 0 && !desc_host)) return VRG_ERR_BAD_ARG;
    for (int64_t i = 0; i < n_desc; ++i)
        if (!grid_desc_ok(desc_host[i], bytes != 0, frames, cell_w, cell_h, grid_w, grid_h)) return VRG_ERR_BAD_ARG;
    return VRG_OK;
}

int vrg_grid_tiles_f32(const vrg_grid_desc* desc, int64_t n_desc, float* out, int64_t frames, int32_t cell_w, int32_t cell_h, int32_t grid_w,
                       int32_t grid_h, void* stream) {
    return grid_launch<float>(desc, n_desc, out, frames, cell_w, cell_h, grid_w, grid_h, stream);
}

int vrg_grid_tiles_u8(const vrg_grid_desc* desc, int64_t n_desc, float* out, int64_t frames, int32_t cell_w, int32_t cell_h, int32_t grid_w,
                      int32_t grid_h, void* stream) {
    return grid_launch<uint8_t>(desc, n_desc, out, frames, cell_w, cell_h, grid_w, grid_h, stream);
}

}  // extern "C"
