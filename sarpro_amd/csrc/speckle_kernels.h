// speckle_kernels.h -- launch interface of the speckle filters (speckle_kernels.hip): Lee and Kuan over u16 and f32 bands, windows of
// 3, 5 and 7 samples, and Frost (windows 3, 5, 7) and Refined Lee (window 7) over u16 bands; f32 out.  The definitions are this
// project's own (include/sarpro_hip.h): the reference's roadmap names the filters and ships none.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstddef>
#include <cstdint>

#include "band_walk.h"

namespace sarpro {

constexpr uint32_t kSpeckleThreads = 256;  // one lane per output column of a strip
constexpr uint32_t kSpeckleHaloCols = 8;   // halo columns a side that a stage row holds (>= 3, a whole 16-byte vector of u16)
constexpr uint32_t kSpeckleRowLen = kSpeckleThreads + 2 * kSpeckleHaloCols; // samples of one stage row
constexpr uint32_t kSpeckleMaxBandRows = 128; // output rows of a u16 tile (the host may choose fewer)
constexpr uint32_t kSpeckleF32BandRows = 16;  // output rows of an f32 tile
constexpr size_t kSpeckleMaxDim = (size_t)1 << 30;
constexpr uint32_t kFrostMaxClasses = 10;     // distinct dy^2 + dx^2 of a 7 x 7 window: 0 1 2 4 5 8 9 10 13 18 (k = 5: the first 6; k = 3: the first 3)

struct SpeckleArgs {
    BandRasters io; // u16 or f32 in
    uint32_t rows, cols;
    uint32_t band_rows;         // output rows per tile (u16: 1..kSpeckleMaxBandRows; f32: kSpeckleF32BandRows)
    double cu2;                 // 1 / looks
    double g;                   // Kuan: 1 / (1 + cu2); Lee: exactly 1.0 (w * 1.0 == w)
    float thr;                  // f32: the smallest valid sample
};

// Frost and Refined Lee (u16 only): the same rasters and tiling; Frost reads damping and dist[], Refined Lee reads base.cu2
struct SpeckleExtArgs {
    SpeckleArgs base;
    double damping;
    double dist[kFrostMaxClasses]; // sqrt((double)r2) of the classes in ascending r2, IEEE-correct, computed on the host
};

// EXP(x) of DESIGN.md 9e for x <= 0: the library's own exponential, one fixed sequence of f64 operations (nothing contracted), so that
// the device, the host and the numpy restatement agree bit for bit and no libm is trusted.  rint and ldexp are exact operations.
__host__ __device__ inline double speckle_exp(double x) {
    constexpr double kLog2e = 0x1.71547652b82fep+0, kLn2Hi = 0x1.62e42fee00000p-1, kLn2Lo = 0x1.a39ef35793c76p-33; // fdlibm's split of ln 2
    if (x < -708.0) return 0.0;
    const double kf = rint(x * kLog2e); // ties to even
    const double r = (x - kf * kLn2Hi) - kf * kLn2Lo;
    double p = 1.0 / 6227020800.0;      // c_i = 1 / i!, each one correctly rounded division (every i! is exact in f64)
    p = p * r + 1.0 / 479001600.0;
    p = p * r + 1.0 / 39916800.0;
    p = p * r + 1.0 / 3628800.0;
    p = p * r + 1.0 / 362880.0;
    p = p * r + 1.0 / 40320.0;
    p = p * r + 1.0 / 5040.0;
    p = p * r + 1.0 / 720.0;
    p = p * r + 1.0 / 120.0;
    p = p * r + 1.0 / 24.0;
    p = p * r + 1.0 / 6.0;
    p = p * r + 1.0 / 2.0;
    p = p * r + 1.0;
    p = p * r + 1.0;
    return ldexp(p, (int)kf); // exact: kf >= -1022
}

// window: 3, 5 or 7.  vec: 16-byte loads (in_pitch % 8 == 0 and every base 16-byte aligned); otherwise element loads, the same results
hipError_t launch_speckle_u16(const SpeckleArgs &a, int window, bool vec, hipStream_t s);
hipError_t launch_speckle_f32(const SpeckleArgs &a, int window, hipStream_t s);
// refined: false = Frost (window 3, 5 or 7), true = Refined Lee (window 7)
hipError_t launch_speckle_ext_u16(const SpeckleExtArgs &a, bool refined, int window, bool vec, hipStream_t s);

} // namespace sarpro
