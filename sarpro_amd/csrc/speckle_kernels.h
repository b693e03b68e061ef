// speckle_kernels.h -- launch interface of the speckle filters (speckle_kernels.hip): Lee and Kuan over u16 and f32 bands, windows of
// 3, 5 and 7 samples, f32 out.  The definition is this project's own (include/sarpro_hip.h): the reference's roadmap
// names the filters and ships none.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

namespace sarpro {

constexpr uint32_t kSpeckleThreads = 256;  // one lane per output column of a strip
constexpr uint32_t kSpeckleHaloCols = 8;   // halo columns a side that a stage row holds (>= 3, a whole 16-byte vector of u16)
constexpr uint32_t kSpeckleRowLen = kSpeckleThreads + 2 * kSpeckleHaloCols; // samples of one stage row
constexpr uint32_t kSpeckleMaxBandRows = 128; // output rows of a u16 tile (the host may choose fewer)
constexpr uint32_t kSpeckleF32BandRows = 16;  // output rows of an f32 tile
constexpr size_t kSpeckleMaxDim = (size_t)1 << 30;

struct SpeckleArgs {
    const void *src[2]; // nbands rasters of the same shape and pitch (u16 or f32)
    float *dst[2];
    uint32_t nbands;
    uint32_t rows, cols;
    uint32_t band_rows;         // output rows per tile (u16: 1..kSpeckleMaxBandRows; f32: kSpeckleF32BandRows)
    size_t in_pitch, out_pitch; // elements
    double cu2;                 // 1 / looks
    double g;                   // Kuan: 1 / (1 + cu2); Lee: exactly 1.0 (w * 1.0 == w)
    float thr;                  // f32: the smallest valid sample
};

// window: 3, 5 or 7.  vec: 16-byte loads (in_pitch % 8 == 0 and every base 16-byte aligned); otherwise element loads, the same results
hipError_t launch_speckle_u16(const SpeckleArgs &a, int window, bool vec, hipStream_t s);
hipError_t launch_speckle_f32(const SpeckleArgs &a, int window, hipStream_t s);

} // namespace sarpro
