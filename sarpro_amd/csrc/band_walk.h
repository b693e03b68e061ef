// band_walk.h -- what the u16-in, f32-out window passes share (read_kernels.hip: Average and Lanczos on read; speckle_kernels.hip: Lee /
// Kuan, Frost, Refined Lee), defined once: the rasters of a launch, the 8-sample fetch and the tiling.  A workgroup owns a tile: a strip
// of destination columns (one lane each) x a band of destination rows of one raster of the launch; blockIdx.x counts strips fastest
// (neighbouring workgroups read neighbouring spans of the same source rows), then row bands, then the band of the raster pair.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

namespace sarpro {

struct BandRasters {
    const void *src[2]; // nbands rasters of the same shape and pitch
    float *dst[2];
    uint32_t nbands;
    size_t in_pitch, out_pitch; // elements
};

// host: the rasters of a launch.  true: 16-byte loads apply (in_pitch % 8 == 0 and every base 16-byte aligned)
template <typename T>
inline bool band_rasters(BandRasters &r, const T *const d_in[], int nb, size_t in_pitch, float *const d_out[], size_t out_pitch) {
    bool vec = in_pitch % 8 == 0;
    for (int b = 0; b < nb; ++b) {
        r.src[b] = d_in[b]; r.dst[b] = d_out[b];
        vec = vec && (reinterpret_cast<uintptr_t>(d_in[b]) & 15) == 0;
    }
    r.nbands = (uint32_t)nb;
    r.in_pitch = in_pitch; r.out_pitch = out_pitch;
    return vec;
}

// host: the grid of a launch whose tiles hold strip_cols x band_rows destination samples; 0: no tile, or more than a grid's 2^31 - 1
inline unsigned band_grid(uint32_t out_cols, uint32_t strip_cols, uint32_t out_rows, uint32_t band_rows, uint32_t nbands) {
    if (!strip_cols || !band_rows) return 0;
    const uint64_t nstrips = ((uint64_t)out_cols + strip_cols - 1) / strip_cols, nrb = ((uint64_t)out_rows + band_rows - 1) / band_rows;
    const uint64_t grid = nstrips * nrb * nbands;
    return grid > 0x7fffffffull ? 0u : (unsigned)grid;
}

// device: the workgroup's tile of that grid
struct BandTile {
    const void *src;
    float *dst;
    uint32_t strip, rb;
};

__device__ __forceinline__ BandTile band_tile(const BandRasters &r, uint32_t out_cols, uint32_t strip_cols, uint32_t out_rows, uint32_t band_rows) {
    const uint32_t nstrips = (out_cols + strip_cols - 1) / strip_cols;
    const uint32_t nrb = (out_rows + band_rows - 1) / band_rows;
    uint32_t t = blockIdx.x;
    BandTile o;
    o.strip = t % nstrips;
    t /= nstrips;
    o.rb = t % nrb;
    const uint32_t band = t / nrb;
    o.src = band ? r.src[1] : r.src[0];
    o.dst = band ? r.dst[1] : r.dst[0];
    return o;
}

// 8 samples from column c (a multiple of 8, c < cols) of a row; samples at and beyond `cols` are never used.  The vector form reads
// them from the row's padding (c + 8 <= in_pitch, a multiple of 8: rasters are rows x in_pitch elements), with no branch between
// the loads of a stage; the element form reads them as 0.
template <bool VEC>
__device__ __forceinline__ uint4 fetch8_u16(const uint16_t *row, uint32_t c, uint32_t cols) {
    if (VEC) return *reinterpret_cast<const uint4 *>(row + c);
    uint32_t w[4];
#pragma unroll
    for (uint32_t p = 0; p < 4; ++p) {
        const uint32_t lo = c + 2 * p < cols ? row[c + 2 * p] : 0u;
        const uint32_t hi = c + 2 * p + 1 < cols ? row[c + 2 * p + 1] : 0u;
        w[p] = lo | (hi << 16);
    }
    return make_uint4(w[0], w[1], w[2], w[3]);
}

} // namespace sarpro
