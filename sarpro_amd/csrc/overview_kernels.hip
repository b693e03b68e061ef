// overview_kernels.hip -- the overview pyramid of an interleaved u8 / u16 raster in ONE sweep over it (restated in
// tests/overviewref.py).  Level k is the aligned 2 x 2 cascade of the ROUNDED level k - 1 with edges clipped, so a pixel of level k
// depends on the source block [i * 2^k, (i + 1) * 2^k) alone: a workgroup owns one 64 x 64-pixel source tile (clipped at the raster's
// edge; tiles walked grid-stride), brings it into LDS with 16-byte loads, reduces it level by level in LDS (each level a buffer of its
// own: 33 KB for u16 x 3) and stores its 32^2, 16^2, ... 1^2 pieces of the next `depth` levels.  Tiles never exchange data: no
// cooperative launch, no grid barrier, no atomics.  All arithmetic is integer: the result is a function of the definition alone,
// whatever the depth per launch, the pitch or the alignment.
//
// Stores: a piece's row is pw * C * B bytes at tile_x * (64 >> k) * C * B bytes into the level's row.  The work items of a piece are
// the 16-byte-aligned slots its rows touch: a slot that lies inside the row goes out as one 16-byte store, the ragged ends as dword
// stores where the address allows and sample stores otherwise -- at levels 1 and 2 of an aligned buffer every store of an interior
// tile is 16 bytes, deeper pieces narrow with their rows (8 * C * B, 4 * C * B, ... bytes).  Bytes outside [row start, row end) are
// never written.
#include "overview_kernels.h"

namespace sarpro {
namespace {

// LDS image of a tile: level l (0 = the source tile) holds (64 >> l)^2 pixels in rows of (64 >> l) * C samples; every level starts on
// a 16-byte boundary
template <typename T, int C> struct OvrLds {
    static constexpr uint32_t bytes(uint32_t l) { return (kOvrTile >> l) * (kOvrTile >> l) * C * (uint32_t)sizeof(T); }
    static constexpr uint32_t off(uint32_t l) {
        uint32_t o = 0;
        for (uint32_t m = 0; m < l; ++m) o += (bytes(m) + 15u) & ~15u;
        return o;
    }
    static constexpr uint32_t total = off(kOvrMaxDepth + 1);
};

// four bytes of a level's LDS buffer at byte offset o (a multiple of the sample size)
template <typename T> __device__ inline uint32_t lds_u32(const uint8_t *base, uint32_t o) {
    if ((o & 3u) == 0) return *reinterpret_cast<const uint32_t *>(base + o);
    if (sizeof(T) == 2) {
        const uint16_t *p = reinterpret_cast<const uint16_t *>(base + o);
        return (uint32_t)p[0] | ((uint32_t)p[1] << 16);
    }
    const uint8_t *p = base + o;
    return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
}

template <typename T, int C, bool VEC>
__global__ __launch_bounds__(kOvrThreads) void k_overviews(const OvrArgs a) {
    using L = OvrLds<T, C>;
    constexpr uint32_t PX = C * (uint32_t)sizeof(T); // bytes per pixel
    constexpr uint32_t ROW0 = kOvrTile * PX;          // bytes per row of the source tile's LDS image (a multiple of 16)
    __shared__ __attribute__((aligned(16))) uint8_t lds[L::total];
    const uint32_t tid = threadIdx.x;
    const uint32_t tiles_x = (a.cols + kOvrTile - 1) / kOvrTile, tiles_y = (a.rows + kOvrTile - 1) / kOvrTile;
    const uint64_t ntiles = (uint64_t)tiles_x * tiles_y;
    for (uint64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
        const uint32_t ty = (uint32_t)(t / tiles_x), tx = (uint32_t)(t - (uint64_t)ty * tiles_x);
        const uint32_t x0 = tx * kOvrTile, y0 = ty * kOvrTile;
        const uint32_t tw = min(kOvrTile, a.cols - x0), th = min(kOvrTile, a.rows - y0); // the tile's valid pixels
        const uint8_t *g = a.src + (size_t)y0 * a.src_pitch + (size_t)x0 * PX;
        // ---- the source tile into LDS.  (The previous tile's stores read levels >= 1 only, and every lane passes the barrier below
        // after them: level 0 is free.)
#ifndef SARPRO_OVR_ABLATE_LOAD // (timing variant, wrong results: no source loads -- the LDS image is whatever it was)
        if (VEC) {
            constexpr uint32_t CPR = ROW0 / 16; // 16-byte slots per tile row; 64 * CPR slots = PX per lane
            const uint32_t rowb = tw * PX;
            uint4 v[PX];
            bool full[PX];
#pragma unroll
            for (int k = 0; k < (int)PX; ++k) {
                const uint32_t c = tid + k * kOvrThreads, r = c / CPR, q = (c % CPR) * 16u;
                full[k] = r < th && q + 16u <= rowb;
                v[k] = full[k] ? *reinterpret_cast<const uint4 *>(g + (size_t)r * a.src_pitch + q) : uint4{0u, 0u, 0u, 0u};
            }
#pragma unroll
            for (int k = 0; k < (int)PX; ++k) {
                const uint32_t c = tid + k * kOvrThreads, r = c / CPR, q = (c % CPR) * 16u;
                if (full[k]) {
                    *reinterpret_cast<uint4 *>(lds + r * ROW0 + q) = v[k];
                } else if (r < th) { // the slot that holds the row's end: sample by sample, never past the row
                    for (uint32_t b = q; b < rowb; b += (uint32_t)sizeof(T))
                        *reinterpret_cast<T *>(lds + r * ROW0 + b) = *reinterpret_cast<const T *>(g + (size_t)r * a.src_pitch + b);
                }
            }
        } else {
            constexpr uint32_t EPR = kOvrTile * C; // samples per tile row
            for (uint32_t e = tid; e < kOvrTile * EPR; e += kOvrThreads) {
                const uint32_t r = e / EPR, x = e % EPR;
                if (r < th && x < tw * C)
                    reinterpret_cast<T *>(lds)[e] = *reinterpret_cast<const T *>(g + (size_t)r * a.src_pitch + (size_t)x * sizeof(T));
            }
        }
#endif
        __syncthreads();
        uint32_t pw = tw, ph = th; // valid pixels of the level being read
#pragma unroll
        for (uint32_t l = 1; l <= kOvrMaxDepth; ++l) {
            if (l > a.depth) break; // (the same in every lane)
            const uint32_t side = kOvrTile >> l, nw = (pw + 1u) >> 1, nh = (ph + 1u) >> 1;
            const T *in = reinterpret_cast<const T *>(lds + L::off(l - 1));
            uint8_t *lev = lds + L::off(l);
            T *out = reinterpret_cast<T *>(lev);
            // ---- level l of the tile from its level l - 1.  A work item makes TWO neighbouring pixels of a row: their 4 x 2 source
            // pixels are PX dwords of each of two LDS rows (4 * PX bytes at a multiple of 4 * PX; a row that does not exist, or pixels
            // past the valid width, are read inside the buffer and masked out).  The 1 x 1 piece of level 6 takes the plain loop.
            if (side >= 2u) {
                const uint32_t half = side >> 1;
                for (uint32_t p = tid; p < side * half; p += kOvrThreads) {
                    const uint32_t i = p / half, jj = p % half;
                    if (i >= nh || 2u * jj >= nw) continue;
                    const uint8_t *r0 = reinterpret_cast<const uint8_t *>(in) + ((size_t)(2u * i) * (2u * side) + 4u * jj) * PX;
                    uint32_t w[2][PX];
#pragma unroll
                    for (uint32_t k = 0; k < PX; ++k) {
                        w[0][k] = *reinterpret_cast<const uint32_t *>(r0 + 4u * k);
                        w[1][k] = *reinterpret_cast<const uint32_t *>(r0 + 2u * side * PX + 4u * k);
                    }
#ifdef SARPRO_OVR_ABLATE_REDUCE // (timing variant, wrong results: a level is the top-left sample of each block -- no sums)
                    for (int c = 0; c < C; ++c) { out[(i * side + 2u * jj) * C + c] = (T)w[0][c % PX]; if (2u * jj + 1u < nw) out[(i * side + 2u * jj + 1u) * C + c] = (T)w[1][c % PX]; }
                    continue;
#endif
                    const bool row1 = 2u * i + 1u < ph;
                    uint32_t sum[2][C], n[2] = {0u, 0u};
#pragma unroll
                    for (int c = 0; c < C; ++c) sum[0][c] = sum[1][c] = 0;
#pragma unroll
                    for (uint32_t r = 0; r < 2; ++r) {
#pragma unroll
                        for (uint32_t k = 0; k < 4; ++k) { // source pixel 4 * jj + k of the row feeds output pixel 2 * jj + (k >> 1)
                            uint32_t v[C], any = 0;
#pragma unroll
                            for (uint32_t c = 0; c < (uint32_t)C; ++c) {
                                const uint32_t sidx = k * C + c; // the sample's index among the 4 * C of the row piece
                                v[c] = sizeof(T) == 1 ? (w[r][sidx >> 2] >> ((sidx & 3u) * 8u)) & 0xFFu : (w[r][sidx >> 1] >> ((sidx & 1u) * 16u)) & 0xFFFFu;
                                any |= v[c];
                            }
                            const bool take = 4u * jj + k < pw && (r == 0 || row1) && (!a.skip_zero || any); // exists, and is no no-data
                            const uint32_t m = take ? 1u : 0u;
#pragma unroll
                            for (int c = 0; c < C; ++c) sum[k >> 1][c] += v[c] * m;
                            n[k >> 1] += m;
                        }
                    }
#pragma unroll
                    for (int c = 0; c < C; ++c) out[(i * side + 2u * jj) * C + c] = (T)ovr_round(sum[0][c], n[0]);
                    if (2u * jj + 1u < nw) {
#pragma unroll
                        for (int c = 0; c < C; ++c) out[(i * side + 2u * jj + 1u) * C + c] = (T)ovr_round(sum[1][c], n[1]);
                    }
                }
            } else {
                for (uint32_t p = tid; p < side * side; p += kOvrThreads) {
                    const uint32_t i = p / side, j = p % side;
                    if (i >= nh || j >= nw) continue;
#ifdef SARPRO_OVR_ABLATE_REDUCE // (timing variant, wrong results: a level is the top-left sample of each block -- one LDS read, no sums)
                    for (int c = 0; c < C; ++c) out[(i * side + j) * C + c] = in[((size_t)(2u * i) * (2u * side) + 2u * j) * C + c];
                    continue;
#endif
                    uint32_t sum[C], n = 0;
#pragma unroll
                    for (int c = 0; c < C; ++c) sum[c] = 0;
#pragma unroll
                    for (uint32_t dy = 0; dy < 2; ++dy) {
#pragma unroll
                        for (uint32_t dx = 0; dx < 2; ++dx) {
                            const uint32_t y = 2u * i + dy, x = 2u * j + dx;
                            if (y >= ph || x >= pw) continue; // the samples that exist
                            const T *s = in + ((size_t)y * (2u * side) + x) * C;
                            uint32_t v[C], any = 0;
#pragma unroll
                            for (int c = 0; c < C; ++c) { v[c] = s[c]; any |= v[c]; }
                            if (a.skip_zero && !any) continue; // no-data: takes no part
#pragma unroll
                            for (int c = 0; c < C; ++c) sum[c] += v[c];
                            ++n;
                        }
                    }
#pragma unroll
                    for (int c = 0; c < C; ++c) out[(i * side + j) * C + c] = (T)ovr_round(sum[c], n);
                }
            }
            __syncthreads();
            // ---- the piece leaves: one work item per 16-byte-aligned slot a row of it touches
            const size_t pitch = a.dst_pitch[l - 1];
            uint8_t *d = a.dst[l - 1] + (size_t)(ty * side) * pitch + (size_t)(tx * side) * PX;
            const uint32_t rb = nw * PX, maxc = (side * PX + 15u) / 16u + 1u;
#ifdef SARPRO_OVR_ABLATE_STORE // (timing variant, wrong results: one slot per piece leaves)
            for (uint32_t it = tid; it < 1u; it += kOvrThreads) {
#else
            for (uint32_t it = tid; it < nh * maxc; it += kOvrThreads) {
#endif
                const uint32_t i = it / maxc, q = it % maxc;
                const uintptr_t g0 = reinterpret_cast<uintptr_t>(d + (size_t)i * pitch), slot = (g0 & ~(uintptr_t)15) + 16u * q;
                const uintptr_t lo = slot > g0 ? slot : g0, hi = slot + 16u < g0 + rb ? slot + 16u : g0 + rb;
                if (lo >= hi) continue;
                const uint32_t o = i * side * PX; // the row in the level's LDS buffer
                if (hi - lo == 16u) {
                    const uint32_t b = o + (uint32_t)(lo - g0);
                    uint4 v;
                    v.x = lds_u32<T>(lev, b); v.y = lds_u32<T>(lev, b + 4u); v.z = lds_u32<T>(lev, b + 8u); v.w = lds_u32<T>(lev, b + 12u);
                    *reinterpret_cast<uint4 *>(lo) = v;
                } else {
                    for (uintptr_t p = lo; p < hi;) {
                        const uint32_t b = o + (uint32_t)(p - g0);
                        if ((p & 3u) == 0 && p + 4u <= hi) {
                            *reinterpret_cast<uint32_t *>(p) = lds_u32<T>(lev, b);
                            p += 4u;
                        } else {
                            *reinterpret_cast<T *>(p) = *reinterpret_cast<const T *>(lev + b);
                            p += sizeof(T);
                        }
                    }
                }
            }
            pw = nw; ph = nh;
        }
    }
}

template <typename T, int C> void launch_tc(const OvrArgs &a, bool vec, unsigned grid, hipStream_t s) {
    if (vec) hipLaunchKernelGGL((k_overviews<T, C, true>), dim3(grid), dim3(kOvrThreads), 0, s, a);
    else hipLaunchKernelGGL((k_overviews<T, C, false>), dim3(grid), dim3(kOvrThreads), 0, s, a);
}

template <typename T> void launch_t(const OvrArgs &a, int components, bool vec, unsigned grid, hipStream_t s) {
    if (components == 1) launch_tc<T, 1>(a, vec, grid, s);
    else if (components == 2) launch_tc<T, 2>(a, vec, grid, s);
    else launch_tc<T, 3>(a, vec, grid, s);
}

} // namespace

hipError_t launch_overviews(const OvrArgs &a, int bits, int components, bool vec, unsigned max_grid, hipStream_t s) {
    if (!a.src || !a.cols || !a.rows || a.cols > kOvrMaxDim || a.rows > kOvrMaxDim || !a.depth || a.depth > kOvrMaxDepth || !max_grid) return hipErrorInvalidValue;
    if ((bits != 8 && bits != 16) || components < 1 || components > 3) return hipErrorInvalidValue;
    for (uint32_t k = 0; k < a.depth; ++k)
        if (!a.dst[k]) return hipErrorInvalidValue;
    const uint64_t ntiles = (uint64_t)((a.cols + kOvrTile - 1) / kOvrTile) * ((a.rows + kOvrTile - 1) / kOvrTile);
    const unsigned grid = (unsigned)(ntiles < max_grid ? ntiles : max_grid);
    if (bits == 8) launch_t<uint8_t>(a, components, vec, grid, s);
    else launch_t<uint16_t>(a, components, vec, grid, s);
    return hipGetLastError();
}

} // namespace sarpro
