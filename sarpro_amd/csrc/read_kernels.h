// read_kernels.h -- launch interface of the downsample-on-read passes (read_kernels.hip): the Lanczos filter (below) and the area average of u16 bands to f32 that
// SafeReader::open_with_options(.., target_size) asks of GDAL (io/sentinel1.rs:1074-1108 -> io/gdal.rs:145-177, ResampleAlg::Average).
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "band_walk.h"

namespace sarpro {

// One destination sample of one axis: its window [first, first + count) of source samples and the weights of the window's two edge
// samples (interior samples weigh exactly 1; a one-sample window has the single weight w_first and w_last = 0).  Built on the host
// (read_path.cpp: read_average_axis), 32 bytes.
struct ReadAxis {
    uint32_t first, count;
    double w_first, w_last, w_sum;
};

constexpr uint32_t kReadThreads = 256;    // one lane per destination column of a strip
constexpr uint32_t kReadChunk = 3072;     // source samples of one row that one LDS slab holds
constexpr uint32_t kReadUnits = 4;        // slabs per stage (two stages in LDS: 48 KiB)
constexpr uint32_t kReadMaxBandRows = 32; // destination rows of a workgroup's tile

struct ReadArgs {
    BandRasters io; // u16 in
    uint32_t rows, cols, out_rows, out_cols;
    const ReadAxis *col_tab;    // [out_cols], device
    const ReadAxis *row_tab;    // [out_rows]
    uint32_t strip_cols;        // destination columns per tile, 1..kReadThreads
    uint32_t band_rows;         // destination rows per tile, 1..kReadMaxBandRows
    uint32_t max_span;          // the widest strip's span of source columns, from its first window's vector boundary to its last window's end
};

// vec: 16-byte loads (in_pitch % 8 == 0 and both bases 16-byte aligned); otherwise element loads with the same results
hipError_t launch_read_average_u16(const ReadArgs &a, bool vec, hipStream_t s);

// ---- the Lanczos filter (a = 3) of the same step, DESIGN.md 9d: k_read_lanczos_u16.  One axis' table: per destination sample its
// window [first, first + count) of source samples, count <= kLanczosTaps, and kLanczosTaps normalised f64 weights (unused slots 0.0).
// Built on the host (read_path.cpp: read_lanczos_axis).
constexpr uint32_t kLanczosTaps = 32;        // weight slots per destination sample (a ratio of 5 needs 30)
constexpr uint32_t kLanczosChunk = 1536;     // source samples of one row that one LDS slab holds: 256 columns x 5 + 30 taps + alignment, and kLanczosTaps of slack
constexpr uint32_t kLanczosUnits = 4;        // source rows per stage (two stages in LDS: 24 KiB)
constexpr uint32_t kLanczosMaxBandRows = 64; // destination rows of a workgroup's tile (their row weights sit in LDS: 16 KiB)
constexpr uint32_t kLanczosRing = 8;         // open destination rows per source row: window i is complete before window i + 8 opens

struct LanczosArgs {
    BandRasters io; // u16 in
    uint32_t rows, cols, out_rows, out_cols;
    const uint32_t *col_first, *col_count; // [out_cols], device
    const uint32_t *row_first, *row_count; // [out_rows]
    const double *col_w, *row_w;           // [out_cols][kLanczosTaps], [out_rows][kLanczosTaps]
    uint32_t band_rows;                    // destination rows per tile, 1..kLanczosMaxBandRows
    uint32_t col_taps;                     // the widest column window, 1..kLanczosTaps (picks the kernel's tap class: 8 / 16 / 24 / 32)
};

// vec as above.  The caller guarantees (read_path.cpp checks the tables): every strip of kReadThreads destination columns spans at
// most kLanczosChunk - kLanczosTaps source columns from its first window's vector boundary, and first[i] + count[i] <= first[i + 8].
hipError_t launch_read_lanczos_u16(const LanczosArgs &a, bool vec, hipStream_t s);

} // namespace sarpro
