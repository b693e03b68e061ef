// overview_kernels.h -- launch interface of the overview pyramid sweep (overview_kernels.hip): levels s + 1 .. s + depth
// of the aligned 2 x 2 cascade from level s of an interleaved u8 / u16 raster, one pass over level s.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

namespace sarpro {

constexpr uint32_t kOvrThreads = 256;  // one workgroup per source tile
constexpr uint32_t kOvrTile = 64;      // source pixels per tile side: a tile yields its 32^2, 16^2, ... 1^2 pieces of the next six levels
constexpr uint32_t kOvrMaxDepth = 6;   // levels one launch can write (log2 of the tile side)
constexpr uint32_t kOvrDefaultDepth = 2; // levels per launch when the context's OVR_DEPTH is unset (overview_path.cpp)
constexpr size_t kOvrMaxDim = (size_t)1 << 30;

// One pixel component of the next level from the n source samples that take part, summed in `sum`: round half up of
// the mean in integer arithmetic; n = 0 (SKIP_ZERO with no valid source pixel): 0.  The kernel and the host restatement share it.
__host__ __device__ inline uint32_t ovr_round(uint32_t sum, uint32_t n) {
    switch (n) {
    case 4: return (sum + 2u) >> 2;
    case 3: return (sum + 1u) / 3u;
    case 2: return (sum + 1u) >> 1;
    default: return n ? sum : 0u;
    }
}

struct OvrArgs {
    const uint8_t *src;              // level s: interleaved samples, `components` per pixel
    size_t src_pitch;                // bytes per row
    uint32_t cols, rows;             // of level s, 1..2^30
    uint32_t depth;                  // levels to write, 1..kOvrMaxDepth
    uint32_t skip_zero;              // SARPRO_HIP_OVR_SKIP_ZERO: a source pixel with all components 0 takes no part
    uint8_t *dst[kOvrMaxDepth];      // level s + 1 + k
    size_t dst_pitch[kOvrMaxDepth];  // bytes per row of it (>= its row bytes; bytes past the row are never written)
};

// bits 8 or 16, components 1..3.  vec: 16-byte loads of the source (src 16-byte aligned and src_pitch % 16 == 0); otherwise element
// loads with the same results.  Destinations may have any alignment (of the sample size): stores are as wide as each address allows.
hipError_t launch_overviews(const OvrArgs &a, int bits, int components, bool vec, unsigned max_grid, hipStream_t s);

} // namespace sarpro
