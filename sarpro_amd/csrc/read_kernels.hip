// read_kernels.hip -- downsample on read: the Lanczos filter of u16 bands to f32 (the second half of this file) and the
// area average of u16 bands to f32 (io/sentinel1.rs:1074-1108 -> io/gdal.rs:145-177 with
// ResampleAlg::Average), DESIGN.md 9b.  A destination pixel is the separable weighted box over its source window: per source row the
// EXACT integer sum of the window's interior columns plus the two edge samples times their f64 weights, the rows of the window
// accumulated top to bottom in f64 with the row weights, one correctly rounded division by the window's weight, one rounding to f32.
// Only the integer sum is order-free, and it is exact: every f64 operation happens in the order of the definition, so the result
// does not depend on the tiling.  (-ffp-contract=off: no product is fused into a sum.)
//
// A workgroup owns a tile (band_walk.h): a strip of <= 256 destination columns (one lane each) x a band of <= 32 destination rows.  It
// walks the source rows of the band top to bottom; every row's span of source columns is cut into slabs of kReadChunk samples (one slab
// for every reduction up to ~12 at full strips; the host narrows the strip for larger reductions; windows wider than a slab -- a
// reduction beyond 3072, a single destination sample -- simply take several slabs per row: the lane's sums run across them).  kReadUnits
// slabs make a stage; two stages live in LDS (SlabStager, which both filters of this file use): while the lanes sum stage s out of LDS,
// the loads of stage s + 1 are in flight into registers and are written to the other half behind the compiler's counted wait, one
// barrier per stage.  The row tables of the tile sit in LDS so that no global load inside the loop sits behind the prefetch in the
// memory counter's order.
#include "read_kernels.h"

namespace sarpro {

namespace {

static_assert((uint64_t)kReadChunk * 65535u < (1ull << 32), "a slab's interior sum fits 32 bits");

// The staging of a tile's source rectangle -- columns [cs, ce) (cs on a vector boundary), rows [ys, ye) -- through two LDS stages of
// UNITS slabs of CHUNK samples: unit u = slab (u % nchunks) of source row ys + u / nchunks.  Which vectors of a stage a lane loads,
// where the next stage's lie, the loads, the LDS writes.  nchunks == 1 (a literal at the call: Lanczos, Average's ONE): qk stays 0.
template <uint32_t UNITS, uint32_t CHUNK>
struct SlabStager {
    static constexpr uint32_t VPU = CHUNK / 8;                        // 16-byte vectors of a slab
    static constexpr uint32_t LOADS = UNITS * VPU / kReadThreads;     // Average: 6, Lanczos: 3
    static_assert(UNITS * VPU % kReadThreads == 0, "a stage is a whole number of vectors per lane");
    uint32_t cs, ce, ye, nchunks;
    uint32_t qy[LOADS], qk[LOADS];
    uint4 regs[LOADS];
    // vector v = tid + q * 256 is vector v % VPU of the stage's unit v / VPU
    __device__ __forceinline__ void init(uint32_t tid, uint32_t cs_, uint32_t ce_, uint32_t ys, uint32_t ye_, uint32_t nchunks_) {
        cs = cs_; ce = ce_; ye = ye_; nchunks = nchunks_;
#pragma unroll
        for (uint32_t q = 0; q < LOADS; ++q) {
            const uint32_t ul = (tid + q * kReadThreads) / VPU;
            qy[q] = ys + ul / nchunks;
            qk[q] = ul % nchunks;
        }
    }
    // the next stage into registers (units past the rectangle: zeros)
    template <bool VEC>
    __device__ __forceinline__ void load(uint32_t tid, const uint16_t *src, size_t in_pitch, uint32_t cols) {
        const uint32_t step_y = UNITS / nchunks, step_k = UNITS % nchunks;
#pragma unroll
        for (uint32_t q = 0; q < LOADS; ++q) {
            const uint32_t iv = (tid + q * kReadThreads) % VPU;
            const uint32_t col = cs + qk[q] * CHUNK + iv * 8;
            regs[q] = make_uint4(0u, 0u, 0u, 0u);
            if (qy[q] < ye && col < ce) regs[q] = fetch8_u16<VEC>(src + (size_t)qy[q] * in_pitch, col, cols);
            qk[q] += step_k; qy[q] += step_y;
            if (qk[q] >= nchunks) { qk[q] -= nchunks; ++qy[q]; }
        }
    }
    __device__ __forceinline__ void write(uint32_t tid, uint4 *half) const {
#pragma unroll
        for (uint32_t q = 0; q < LOADS; ++q) half[tid + q * kReadThreads] = regs[q];
    }
};

} // namespace

// ONE: every strip's span of source columns fits one slab (the host checks the widest): the slab index, the chunk bounds and the
// lane's range inside the slab are then constants of the tile, and a row's interior sum fits 32 bits.
template <bool VEC, bool ONE>
__global__ __launch_bounds__(kReadThreads) void k_read_average_u16(ReadArgs a) {
    using Stager = SlabStager<kReadUnits, kReadChunk>;
    __shared__ uint4 s_slab[2][kReadUnits * Stager::VPU];
    __shared__ ReadAxis s_rows[kReadMaxBandRows];
    const uint32_t tid = threadIdx.x;
    const BandTile tl = band_tile(a.io, a.out_cols, a.strip_cols, a.out_rows, a.band_rows);
    const uint16_t *src = static_cast<const uint16_t *>(tl.src);
    float *dst = tl.dst;
    const uint32_t j0 = tl.strip * a.strip_cols, j1 = min(j0 + a.strip_cols, a.out_cols);
    const uint32_t i0 = tl.rb * a.band_rows, i1 = min(i0 + a.band_rows, a.out_rows);
    if (tid < i1 - i0) s_rows[tid] = a.row_tab[i0 + tid];
    // the tile's source rectangle: columns [cs, ce) (cs on a vector boundary), rows [ys, ye)
    const ReadAxis cfirst = a.col_tab[j0], clast = a.col_tab[j1 - 1], rfirst = a.row_tab[i0], rlast = a.row_tab[i1 - 1];
    const uint32_t cs = cfirst.first & ~7u, ce = clast.first + clast.count;
    const uint32_t ys = rfirst.first, ye = rlast.first + rlast.count;
    const uint32_t nchunks = ONE ? 1u : (ce - cs + kReadChunk - 1) / kReadChunk;
    const uint32_t nunits = (ye - ys) * nchunks;
    const uint32_t nstages = (nunits + kReadUnits - 1) / kReadUnits;
    // the lane's destination column (idle lanes: an empty window beyond every slab)
    const bool active = tid < j1 - j0;
    uint32_t c0 = 0x7fffffffu, c1 = 0x7fffffffu;
    double cwf = 0.0, cwl = 0.0, cws = 1.0;
    if (active) {
        const ReadAxis e = a.col_tab[j0 + tid];
        c0 = e.first; c1 = e.first + e.count;
        cwf = e.w_first; cwl = e.w_last; cws = e.w_sum;
    }
    const bool wide = c1 - c0 > 1;
    Stager st;
    st.init(tid, cs, ce, ys, ye, nchunks);
    st.template load<VEC>(tid, src, a.io.in_pitch, a.cols);
    st.write(tid, s_slab[0]);
    __syncthreads();
    // running state: the source row y and its slab k (uniform); the destination row i with its window [r0, r1) (uniform); per lane the
    // row's interior sum and edge samples, and the window's weighted sum T
    uint32_t y = ys, k = 0, i = i0;
    ReadAxis re = s_rows[0];
    uint32_t r0 = re.first, r1 = re.first + re.count;
    uint64_t isum = 0;
    uint32_t vf = 0, vl = 0;
    double T = 0.0;
    for (uint32_t s = 0; s < nstages; ++s) {
        const bool more = s + 1 < nstages;
        if (more) st.template load<VEC>(tid, src, a.io.in_pitch, a.cols);
        const uint32_t nu = min(kReadUnits, nunits - s * kReadUnits);
        for (uint32_t ul = 0; ul < nu; ++ul) {
            const uint16_t *slab = reinterpret_cast<const uint16_t *>(&s_slab[s & 1][ul * Stager::VPU]);
            const uint32_t cb = cs + k * kReadChunk, cend = min(cb + kReadChunk, ce);
            const uint32_t lo = max(c0 + 1, cb), hi = min(c1 - 1, cend);
            uint32_t part = 0;
#ifndef SARPRO_READ_ABLATE_SUM // (timing variant, tools/build_variant.sh: the pass without the lanes' LDS reads -- loads, staging, row logic, stores)
            uint32_t c = lo; // (blocks of independent LDS reads: a one-sample loop waits out the LDS latency per sample)
            for (; c + 8 <= hi; c += 8) {
                const uint16_t *p = slab + (c - cb);
                part += ((uint32_t)p[0] + p[1]) + ((uint32_t)p[2] + p[3]) + (((uint32_t)p[4] + p[5]) + ((uint32_t)p[6] + p[7]));
            }
            if (c + 4 <= hi) {
                const uint16_t *p = slab + (c - cb);
                part += ((uint32_t)p[0] + p[1]) + ((uint32_t)p[2] + p[3]);
                c += 4;
            }
            for (; c < hi; ++c) part += slab[c - cb];
            isum += part;
            if (c0 >= cb && c0 < cend) vf = slab[c0 - cb];
            if (c1 - 1 >= cb && c1 - 1 < cend) vl = slab[c1 - 1 - cb];
#endif
            if (k + 1 < nchunks) { ++k; continue; }
            // the row is complete: its weighted line sum, then the destination row(s) it belongs to
            double L = (double)isum + cwf * (double)vf;
            if (wide) L = L + cwl * (double)vl;
            while (i < i1 && y >= r0) {
                const double wy = y == r0 ? re.w_first : (y == r1 - 1 ? re.w_last : 1.0);
                T = T + wy * L;
                if (y != r1 - 1) break;
                if (active) dst[(size_t)i * a.io.out_pitch + j0 + tid] = (float)(T / (cws * re.w_sum));
                T = 0.0;
                if (++i < i1) { re = s_rows[i - i0]; r0 = re.first; r1 = re.first + re.count; } // (a fractional boundary: this row opens the next window too)
            }
            isum = 0;
            k = 0; ++y;
        }
        if (more) st.write(tid, s_slab[(s + 1) & 1]);
        __syncthreads();
    }
}

hipError_t launch_read_average_u16(const ReadArgs &a, bool vec, hipStream_t s) {
    const unsigned grid = band_grid(a.out_cols, a.strip_cols, a.out_rows, a.band_rows, a.io.nbands);
    if (!grid || a.strip_cols > kReadThreads || a.band_rows > kReadMaxBandRows) return hipErrorInvalidValue;
#ifdef SARPRO_READ_ABLATE_GENERIC // (timing variant: the several-slabs form at every shape)
    const bool one = false;
#else
    const bool one = a.max_span <= kReadChunk;
#endif
    if (vec && one) hipLaunchKernelGGL((k_read_average_u16<true, true>), dim3(grid), dim3(kReadThreads), 0, s, a);
    else if (vec) hipLaunchKernelGGL((k_read_average_u16<true, false>), dim3(grid), dim3(kReadThreads), 0, s, a);
    else if (one) hipLaunchKernelGGL((k_read_average_u16<false, true>), dim3(grid), dim3(kReadThreads), 0, s, a);
    else hipLaunchKernelGGL((k_read_average_u16<false, false>), dim3(grid), dim3(kReadThreads), 0, s, a);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------------------------------------------
// The Lanczos filter (a = 3) of the same step, DESIGN.md 9d.  out[i][j] = (float) sum_y w_y[i][y] * H[y][j] with H[y][j] = sum_c
// w_x[j][c] * (double)v[y][c]: both sums in ascending order from 0.0, every product and sum rounded on its own, one rounding to f32.
// H depends on (y, j) alone, so the result does not depend on the tiling.  ONE pass, H never leaves the registers: a workgroup owns a
// strip of <= 256 destination columns (one lane each) x a band of <= 64 destination rows and walks the band's source rows top to
// bottom through the double-buffered LDS slabs of the Average pass (one slab per row: a strip spans <= 1318 source columns at the
// largest ratio, 5).  Per source row a lane forms H from LDS with its own NT column weights (registers; slots past the window weigh 0.0
// and add +0.0: bit-neutral) and adds w_y * H into the open accumulators: destination row i accumulates in ring entry (i - i0) % 8
// (window i is complete before window i + 8 opens: the host checks the tables), the ring and its bookkeeping statically indexed --
// the loop over the entries is unrolled and every branch in it is workgroup-uniform.  The row weights of the band sit in LDS.
static_assert(kLanczosChunk % 8 == 0 && kLanczosChunk >= kReadThreads * 5 + 30 + 7 + kLanczosTaps, "a strip's span at a ratio of 5, plus the slack of the unused tap slots");

template <bool VEC, uint32_t NT>
__global__ __launch_bounds__(kReadThreads) void k_read_lanczos_u16(LanczosArgs a) {
    using Stager = SlabStager<kLanczosUnits, kLanczosChunk>;
    __shared__ uint4 s_slab[2][kLanczosUnits * Stager::VPU];
    __shared__ double s_wrow[kLanczosMaxBandRows * kLanczosTaps];
    __shared__ uint32_t s_rfirst[kLanczosMaxBandRows], s_rend[kLanczosMaxBandRows];
    const uint32_t tid = threadIdx.x;
    const BandTile tl = band_tile(a.io, a.out_cols, kReadThreads, a.out_rows, a.band_rows);
    const uint16_t *src = static_cast<const uint16_t *>(tl.src);
    float *dst = tl.dst;
    const uint32_t j0 = tl.strip * kReadThreads, j1 = min(j0 + kReadThreads, a.out_cols);
    const uint32_t i0 = tl.rb * a.band_rows, i1 = min(i0 + a.band_rows, a.out_rows), nb = i1 - i0;
    for (uint32_t e = tid; e < nb * kLanczosTaps; e += kReadThreads) s_wrow[e] = a.row_w[(size_t)i0 * kLanczosTaps + e];
    if (tid < nb) {
        const uint32_t f = a.row_first[i0 + tid];
        s_rfirst[tid] = f; s_rend[tid] = f + a.row_count[i0 + tid];
    }
    // the tile's source rectangle: columns [cs, ce) (cs on a vector boundary), rows [ys, ye)
    const uint32_t cs = a.col_first[j0] & ~7u, ce = a.col_first[j1 - 1] + a.col_count[j1 - 1];
    const uint32_t ys = a.row_first[i0], ye = a.row_first[i1 - 1] + a.row_count[i1 - 1];
    const uint32_t nunits = ye - ys; // unit u = the slab of source row ys + u
    const uint32_t nstages = (nunits + kLanczosUnits - 1) / kLanczosUnits;
    // the lane's destination column: where its window starts in the slab, its weights (idle lanes: weights 0.0 at the slab's start)
    const bool active = tid < j1 - j0;
    uint32_t off = 0;
    double w[NT];
#pragma unroll
    for (uint32_t k = 0; k < NT; ++k) w[k] = 0.0;
    if (active) {
        off = a.col_first[j0 + tid] - cs;
        const double *p = a.col_w + (size_t)(j0 + tid) * kLanczosTaps;
#pragma unroll
        for (uint32_t k = 0; k < NT; ++k) w[k] = p[k];
    }
    Stager st;
    st.init(tid, cs, ce, ys, ye, 1u);
    st.template load<VEC>(tid, src, a.io.in_pitch, a.cols);
    st.write(tid, s_slab[0]);
    __syncthreads();
    // the ring: entry e holds destination row i0 + li[e] (li[e] % 8 == e) with its window [rf[e], re[e]) of source rows (uniform; no
    // row left: an empty window past every row) and, per lane, the running sum
    double acc[kLanczosRing];
    uint32_t li[kLanczosRing], rf[kLanczosRing], re[kLanczosRing];
#pragma unroll
    for (uint32_t e = 0; e < kLanczosRing; ++e) {
        acc[e] = 0.0; li[e] = e; rf[e] = 0xffffffffu; re[e] = 0xffffffffu;
        if (e < nb) { rf[e] = __builtin_amdgcn_readfirstlane(s_rfirst[e]); re[e] = __builtin_amdgcn_readfirstlane(s_rend[e]); }
    }
    uint32_t y = ys;
    for (uint32_t s = 0; s < nstages; ++s) {
        const bool more = s + 1 < nstages;
        if (more) st.template load<VEC>(tid, src, a.io.in_pitch, a.cols);
        const uint32_t nu = min(kLanczosUnits, nunits - s * kLanczosUnits);
        for (uint32_t ul = 0; ul < nu; ++ul, ++y) {
            const uint16_t *slab = reinterpret_cast<const uint16_t *>(&s_slab[s & 1][ul * Stager::VPU]) + off;
#ifndef SARPRO_LANCZOS_ABLATE_TAPS // (timing variant, tools/build_variant.sh: the pass without the lanes' tap reads and f64 products -- wrong results)
            double H = 0.0;
#pragma unroll
            for (uint32_t k = 0; k < NT; ++k) H = H + w[k] * (double)slab[k];
#else
            const double H = w[0] * (double)slab[0];
#endif
#pragma unroll
            for (uint32_t e = 0; e < kLanczosRing; ++e) {
                if (y >= rf[e] && y < re[e]) {
                    acc[e] = acc[e] + s_wrow[li[e] * kLanczosTaps + (y - rf[e])] * H;
                    if (y + 1 == re[e]) { // the window is complete: the one rounding to f32; the entry takes its next destination row
                        if (active) dst[(size_t)(i0 + li[e]) * a.io.out_pitch + j0 + tid] = (float)acc[e];
                        acc[e] = 0.0;
                        li[e] += kLanczosRing;
                        rf[e] = 0xffffffffu; re[e] = 0xffffffffu;
                        if (li[e] < nb) { rf[e] = __builtin_amdgcn_readfirstlane(s_rfirst[li[e]]); re[e] = __builtin_amdgcn_readfirstlane(s_rend[li[e]]); }
                    }
                }
            }
        }
        if (more) st.write(tid, s_slab[(s + 1) & 1]);
        __syncthreads();
    }
}

template <bool VEC>
static void launch_lanczos_class(const LanczosArgs &a, unsigned grid, hipStream_t s) {
    if (a.col_taps <= 8) hipLaunchKernelGGL((k_read_lanczos_u16<VEC, 8>), dim3(grid), dim3(kReadThreads), 0, s, a);
    else if (a.col_taps <= 16) hipLaunchKernelGGL((k_read_lanczos_u16<VEC, 16>), dim3(grid), dim3(kReadThreads), 0, s, a);
    else if (a.col_taps <= 24) hipLaunchKernelGGL((k_read_lanczos_u16<VEC, 24>), dim3(grid), dim3(kReadThreads), 0, s, a);
    else hipLaunchKernelGGL((k_read_lanczos_u16<VEC, 32>), dim3(grid), dim3(kReadThreads), 0, s, a);
}

hipError_t launch_read_lanczos_u16(const LanczosArgs &a, bool vec, hipStream_t s) {
    const unsigned grid = band_grid(a.out_cols, kReadThreads, a.out_rows, a.band_rows, a.io.nbands);
    if (!grid || a.band_rows > kLanczosMaxBandRows || !a.col_taps || a.col_taps > kLanczosTaps) return hipErrorInvalidValue;
    if (vec) launch_lanczos_class<true>(a, grid, s);
    else launch_lanczos_class<false>(a, grid, s);
    return hipGetLastError();
}

} // namespace sarpro
