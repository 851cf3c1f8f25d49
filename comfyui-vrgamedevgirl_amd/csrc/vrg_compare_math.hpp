// vrg_compare_math.hpp -- the Video Compare Slider's IMAGE batch as rgb24 bytes (csrc/vrg_compare.hip), host and device: the per-value
// rule.  Pinned against live numpy by tests/test_compare_host.py.
//   _write_image_batch_video (VRGDG_VideoCompareNode.py:63-107 of the reference): np.clip(frame[..., :3] * 255.0, 0, 255).astype(np.uint8)
//   frame by frame -- the product of an fp32 array and a Python float is ONE fp32 product, the clip works on that product, and the
//   conversion truncates.  Truncation is what sets this rule apart from anchor_store_byte (csrc/vrg_anchor_math.hpp), which rounds: a
//   product in [k + 0.5, k + 1) is k here and k + 1 there, and the float just under a byte level k / 255.0f is k - 1 here and k there.
//   The levels themselves are k under both rules: 1 / 255 = 0.(00000001) in binary, so the 24 significant bits of k / 255 end on a whole
//   period, the first bit dropped is the leading 1 of k again, the quotient rounds UP, and (k / 255.0f) * 255.0f is never below k
//   (tests/test_compare_host.py holds that for all 256).  The product is formed first and alone (the library is built with
//   -ffp-contract=off; no pre-scaled compare stands in for it), so a value just under 1 whose product rounds up to 255.0f gives 255 as
//   numpy does.  np.clip keeps a NaN and numpy's conversion of NaN to uint8 is platform-defined: x86
//   numpy yields 0, the pack's convention for byte outputs: RGB24_NAN_BYTE.
#pragma once
#include "vrg_common.hpp"

namespace vrg {

constexpr uint8_t RGB24_NAN_BYTE = 0;

VRG_HD uint8_t rgb24_byte(float x) {
    const float v = x * 255.0f;
    if (v != v) return RGB24_NAN_BYTE;
    const float c = v < 0.0f ? 0.0f : (v > 255.0f ? 255.0f : v);          // -0.0f passes and truncates to 0
    return (uint8_t)(int32_t)c;
}

// HOST.  vrg_rgb24_frames_u8 in plain loops: src = [pixels][channels] fp32, dst = [pixels][3] bytes
inline void rgb24_frames_host(const float* src, int64_t pixels, int32_t channels, uint8_t* dst) {
    for (int64_t p = 0; p < pixels; ++p)
        for (int32_t c = 0; c < 3; ++c) dst[p * 3 + c] = rgb24_byte(src[p * channels + c]);
}

}  // namespace vrg
