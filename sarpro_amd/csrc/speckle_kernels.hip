// speckle_kernels.hip -- adaptive speckle filters over u16 and f32 bands, f32 out: Lee and Kuan, and over u16 bands Frost and
// Refined Lee (defined in include/sarpro_hip.h, their kernels are further below).  Lee and Kuan: the definition is this
// project's own -- the reference's roadmap names the filters (ROADMAP Phase 4) and ships none -- and is fixed operation by operation:
//   window   k x k around the pixel, clipped to the raster, only VALID samples count (u16: v >= 1; f32: thr <= v < +inf)
//   centre invalid: the output is (float)v (u16) / the input's bit pattern (f32)
//   otherwise, n valid samples:  S1 = sum v, S2 = sum v^2;  A = S1 * S1;  D = n * S2 - A;  m = S1 / n;
//            !(D > 0): out = (float)m;   else q = (cu2 * A) / D;  w = 1 - q (Lee) | (1 - q) * g (Kuan);  !(w > 0): w = 0;
//            out = (float)(m + w * (v - m))
//   u16: S1, S2, A, D are EXACT integers (any order; all below 2^45, so their f64 forms are exact).  f32: per window row, top to bottom,
//   the row's partial sums left to right in f64 from 0.0, the row partials added top to bottom from 0.0; B = (double)n * S2; D = B - A.
//   f64 throughout, nothing contracted (-ffp-contract=off), correctly rounded divisions, one rounding to f32.  Lee is computed as
//   (1 - q) * 1.0, which is 1 - q bit for bit.
// So the result is a function of the definition alone, whatever the tiling, the pitch or the load width.
//
// k_speckle_u16 (the hot path: 400 MP bands, 2 B/px in, 4 B/px out) = speckle_band_walk with LeeFilter; Frost is a second filter of the
// same walk.  A workgroup owns a tile (band_walk.h): a strip of <= 256 output columns (one lane each) x a band of output rows; it walks
// the band's source rows (h halo rows above and below; rows and columns outside the raster read as 0 = invalid) top to bottom through
// two LDS stages of 28 / 30 rows x (256 + 2 * 8) samples: while the lanes work through stage s, the four 16-byte loads per lane of
// stage s + 1 are in flight into registers and are written to the other half behind the compiler's counted wait, one barrier per stage.
// Per source row a lane forms the row's horizontal (n, S1, S2) over its k columns from LDS, pushes it into a ring of k row entries in
// registers (statically indexed: the row loop is unrolled by k, and a stage holds a multiple of k rows), keeps the vertical totals by
// adding the new row and subtracting the oldest -- exact, these are integers -- and emits the pixel of row y - h.  A ring entry is 3
// words: S1 | n << 19, and S2 (< 2^35) with the row's centre sample in bits 40..55.
#include <type_traits>

#include "speckle_kernels.h"

namespace sarpro {

namespace {

// the f64 tail both flavours share; nd >= 1
__device__ __forceinline__ float speckle_tail(double nd, double S1, double A, double D, double vd, double cu2, double g) {
    const double m = S1 / nd;
    const double q = (cu2 * A) / D;
    double w = (1.0 - q) * g;
    w = w > 0.0 ? w : 0.0;
    const double o = m + w * (vd - m);
    return D > 0.0 ? (float)o : (float)m;
}

// word p of a vector of which the first nv samples (0..8) lie inside the raster (fetch8_u16's vector form may have read the row's
// padding beyond `cols`)
__device__ __forceinline__ uint32_t speckle_keep(uint32_t w, uint32_t nv, uint32_t p) {
    return nv >= 2 * p + 2 ? w : (nv == 2 * p + 1 ? (w & 0xffffu) : 0u);
}

// the part of the u16 kernels' staging that does not depend on the filter: which vectors of a stage a lane loads, the loads, the LDS writes
template <uint32_t ROWS, bool VEC>
struct SpeckleStager {
    static constexpr uint32_t VPR = kSpeckleRowLen / 8;  // 16-byte vectors of a stage row (34)
    static constexpr uint32_t NVEC = ROWS * VPR;
    static constexpr uint32_t LOADS = (NVEC + kSpeckleThreads - 1) / kSpeckleThreads; // 4
    uint32_t lrow[LOADS], lcol[LOADS], lnv[LOADS];
    uint4 regs[LOADS];
    // vector v = tid + q * 256 is vector v % VPR of stage row v / VPR (the same for every stage)
    __device__ __forceinline__ void init(uint32_t tid, uint32_t x0, uint32_t cols) {
#pragma unroll
        for (uint32_t q = 0; q < LOADS; ++q) {
            const uint32_t v = tid + q * kSpeckleThreads;
            lrow[q] = v / VPR;
            const int32_t c = (int32_t)x0 - (int32_t)kSpeckleHaloCols + (int32_t)(v % VPR) * 8;
            const bool ok = v < NVEC && c >= 0 && (uint32_t)c < cols;
            lcol[q] = ok ? (uint32_t)c : 0u;
            lnv[q] = ok ? min(8u, cols - (uint32_t)c) : 0u;
        }
    }
    // source rows [ys, ye) of the band; rows and columns outside the raster read as 0 = invalid
    __device__ __forceinline__ void load(const uint16_t *src, const SpeckleArgs &a, int32_t ys, int32_t ye, uint32_t s) {
#pragma unroll
        for (uint32_t q = 0; q < LOADS; ++q) {
            const int32_t y = ys + (int32_t)(s * ROWS + lrow[q]);
            regs[q] = make_uint4(0u, 0u, 0u, 0u);
            if (lnv[q] && y >= 0 && y < ye && (uint32_t)y < a.rows) regs[q] = fetch8_u16<VEC>(src + (size_t)y * a.io.in_pitch, lcol[q], a.cols);
        }
    }
    __device__ __forceinline__ void write(uint4 *half, uint32_t tid) const {
#pragma unroll
        for (uint32_t q = 0; q < LOADS; ++q) {
            const uint32_t v = tid + q * kSpeckleThreads;
            const uint4 r = regs[q];
            if (v < NVEC)
                half[v] = make_uint4(speckle_keep(r.x, lnv[q], 0), speckle_keep(r.y, lnv[q], 1), speckle_keep(r.z, lnv[q], 2), speckle_keep(r.w, lnv[q], 3));
        }
    }
};

// The band walk of the three u16 kernels, which differ only in the Filter: the tile (band_walk.h), the two LDS stages and their
// prologue, the band's source rows [ys, ye) top to bottom -- stage s, group g of K rows, row r of the group, unrolled, so that r is
// static and a stage starts at ring entry 0 -- the write-behind and the barrier.  Per source row the walk calls
//   f.take(r, p)   row r's K samples, p[0 .. K - 1] in LDS (p[H]: the lane's own column), into ring entry r
//   f.pixel(r)     the pixel whose window row r completes (rows r - K + 1 .. r of the ring, centre row (r + K - H) % K): for output rows >= i0
// and stores the pixel of the lanes inside the raster.  Every exit of the loops is workgroup-uniform.
template <uint32_t K, bool VEC, typename Filter>
__device__ __forceinline__ void speckle_band_walk(const SpeckleArgs &a, Filter &f) {
    constexpr uint32_t H = K / 2;
    constexpr uint32_t ROWS = K == 7 ? 28u : 30u; // source rows of a stage: a multiple of K
    using Stager = SpeckleStager<ROWS, VEC>;
    static_assert(ROWS % K == 0, "a stage starts at ring entry 0");
    static_assert(H <= kSpeckleHaloCols && kSpeckleRowLen % 8 == 0, "the halo is a whole vector");
    __shared__ uint4 s_stage[2][Stager::NVEC];
    const uint32_t tid = threadIdx.x;
    const BandTile tl = band_tile(a.io, a.cols, kSpeckleThreads, a.rows, a.band_rows);
    const uint16_t *src = static_cast<const uint16_t *>(tl.src);
    const uint32_t x0 = tl.strip * kSpeckleThreads, i0 = tl.rb * a.band_rows, i1 = min(i0 + a.band_rows, a.rows);
    // source rows [ys, ye) of the band, halo included; rows outside the raster are all invalid
    const int32_t ys = (int32_t)i0 - (int32_t)H, ye = (int32_t)i1 + (int32_t)H;
    const uint32_t nstages = ((uint32_t)(ye - ys) + ROWS - 1) / ROWS;
    const bool active = x0 + tid < a.cols;
    Stager st;
    st.init(tid, x0, a.cols);
    st.load(src, a, ys, ye, 0);
    st.write(s_stage[0], tid);
    __syncthreads();
    for (uint32_t s = 0; s < nstages; ++s) {
        const bool more = s + 1 < nstages;
        if (more) st.load(src, a, ys, ye, s + 1);
        const uint16_t *lds = reinterpret_cast<const uint16_t *>(&s_stage[s & 1][0]) + tid + kSpeckleHaloCols - H;
        int32_t y = ys + (int32_t)(s * ROWS);
        for (uint32_t g = 0; g < ROWS / K && y < ye; ++g) {
#pragma unroll
            for (uint32_t r = 0; r < K; ++r, ++y) {
                if (y >= ye) break; // (uniform)
                f.take(r, lds + (g * K + r) * kSpeckleRowLen);
                const int32_t yo = y - (int32_t)H; // the output row whose window this row completes
                if (yo < (int32_t)i0) continue;    // (uniform)
                const float out = f.pixel(r);
                if (active) tl.dst[(size_t)yo * a.io.out_pitch + x0 + tid] = out;
            }
        }
        if (more) st.write(s_stage[(s + 1) & 1], tid);
        __syncthreads();
    }
}

// Lee and Kuan: the ring of the last K rows' (n, S1, S2) and the window's totals
template <uint32_t K>
struct LeeFilter {
    static constexpr uint32_t H = K / 2;
    static constexpr uint64_t kS2Mask = (1ull << 40) - 1;
    const SpeckleArgs &a;
    uint32_t e1[K];
    uint64_t e2[K];
    uint32_t tn = 0, ts1 = 0;
    uint64_t ts2 = 0;
    __device__ __forceinline__ explicit LeeFilter(const SpeckleArgs &args) : a(args) {
#pragma unroll
        for (uint32_t r = 0; r < K; ++r) { e1[r] = 0u; e2[r] = 0ull; }
    }
    __device__ __forceinline__ void take(uint32_t r, const uint16_t *p) {
        const uint32_t c = p[H];
        uint32_t n = c != 0u, s1 = c;
        uint64_t s2 = c * c; // (c < 2^16: the 32-bit product is the whole one)
#ifndef SARPRO_SPECKLE_ABLATE_SUM // (timing variant: the pass without the window's LDS reads and row sums -- a window of k rows x 1 column)
#pragma unroll
        for (uint32_t j = 0; j < K; ++j) {
            if (j == H) continue;
            const uint32_t v = p[j];
            n += v != 0u;
            s1 += v;
            s2 += v * v;
        }
#endif
        tn = tn + n - (e1[r] >> 19);
        ts1 = ts1 + s1 - (e1[r] & 0x7ffffu);
        ts2 = ts2 + s2 - (e2[r] & kS2Mask);
        e1[r] = s1 | (n << 19);
        e2[r] = s2 | ((uint64_t)c << 40);
    }
    __device__ __forceinline__ float pixel(uint32_t r) const {
        const uint32_t v = (uint32_t)(e2[(r + K - H) % K] >> 40);
        float out;
#ifndef SARPRO_SPECKLE_ABLATE_TAIL // (timing variant: the pass without its f64 tail)
        const uint64_t A = (uint64_t)ts1 * ts1;
        const uint64_t D = (uint64_t)tn * ts2 - A;
        out = speckle_tail((double)max(tn, 1u), (double)ts1, (double)A, (double)D, (double)v, a.cu2, a.g);
#else
        out = (float)(ts1 + tn + (uint32_t)ts2);
#endif
        return v ? out : 0.0f;
    }
};

} // namespace

template <uint32_t K, bool VEC>
__global__ __launch_bounds__(kSpeckleThreads) void k_speckle_u16(SpeckleArgs a) {
    LeeFilter<K> f(a);
    speckle_band_walk<K, VEC>(a, f);
}

// The f32 flavour: the same strips and row bands, one tile of (16 + 2h) x (256 + 2h) samples in LDS (outside the raster: NaN = invalid);
// a lane sums its window's rows from LDS in the order of the definition.  The f32 scenes this library sees are a few MP.
template <uint32_t K>
__global__ __launch_bounds__(kSpeckleThreads) void k_speckle_f32(SpeckleArgs a) {
    constexpr uint32_t H = K / 2, TR = kSpeckleF32BandRows, LR = TR + 2 * H, LC = kSpeckleThreads + 2 * H;
    __shared__ uint32_t s_tile[LR][LC];
    const uint32_t tid = threadIdx.x;
    const BandTile tl = band_tile(a.io, a.cols, kSpeckleThreads, a.rows, TR);
    const uint32_t *src = static_cast<const uint32_t *>(tl.src); // (bit patterns: an invalid centre goes out as it came in)
    uint32_t *dst = reinterpret_cast<uint32_t *>(tl.dst);
    const uint32_t x0 = tl.strip * kSpeckleThreads;
    const uint32_t i0 = tl.rb * TR, i1 = min(i0 + TR, a.rows);
    for (uint32_t idx = tid; idx < LR * LC; idx += kSpeckleThreads) {
        const uint32_t r = idx / LC, c = idx % LC;
        const int32_t y = (int32_t)i0 - (int32_t)H + (int32_t)r, x = (int32_t)x0 - (int32_t)H + (int32_t)c;
        uint32_t bits = 0x7fc00000u;
        if (y >= 0 && (uint32_t)y < a.rows && x >= 0 && (uint32_t)x < a.cols) bits = src[(size_t)y * a.io.in_pitch + (uint32_t)x];
        s_tile[r][c] = bits;
    }
    __syncthreads();
    const bool active = x0 + tid < a.cols;
    const float thr = a.thr, inf = __builtin_inff();
    for (uint32_t i = i0; i < i1; ++i) {
        double S1 = 0.0, S2 = 0.0;
        uint32_t n = 0;
#pragma unroll
        for (uint32_t dy = 0; dy < K; ++dy) {
            double r1 = 0.0, r2 = 0.0;
#pragma unroll
            for (uint32_t dx = 0; dx < K; ++dx) {
                const float v = __uint_as_float(s_tile[i - i0 + dy][tid + dx]);
                const bool ok = v >= thr && v < inf;
                const double d = ok ? (double)v : 0.0; // (adding 0.0 to these non-negative sums changes nothing)
                r1 = r1 + d;
                r2 = r2 + d * d;
                n += ok;
            }
            S1 = S1 + r1;
            S2 = S2 + r2;
        }
        const uint32_t cbits = s_tile[i - i0 + H][tid + H];
        const float cv = __uint_as_float(cbits);
        const bool cok = cv >= thr && cv < inf;
        const double A = S1 * S1;
        const double B = (double)n * S2;
        const double D = B - A;
        const float out = speckle_tail((double)max(n, 1u), S1, A, D, cok ? (double)cv : 0.0, a.cu2, a.g);
        const uint32_t obits = cok ? __float_as_uint(out) : cbits;
        if (active) dst[(size_t)i * a.io.out_pitch + x0 + tid] = obits;
    }
}

// ---------------------------------------------------------------------------- Frost and Refined Lee over u16 bands
// Both are filters of speckle_band_walk, as Lee is: per source row a lane reads its k samples from LDS once, pushes what the filter
// needs of them into a ring of k row entries in registers (statically indexed) and emits the pixel of row y - h.
namespace {

// index of r2 = dy^2 + dx^2 in the ascending list 0 1 2 4 5 8 9 10 13 18 (windows 3 and 5 use its first 3 and 6 entries)
__host__ __device__ constexpr uint32_t frost_class(uint32_t r2) { return r2 <= 2 ? r2 : r2 <= 5 ? r2 - 1 : r2 <= 10 ? r2 - 3 : r2 == 13 ? 8u : 9u; }

// Frost.  The weight of a sample depends on its distance from the centre alone, so a pixel needs, per distance class, the sum T_c and
// the count N_c of the class's valid samples.  A row at vertical offset dy gives its pair sums v[x - j] + v[x + j] (j = 1..h) and its
// centre sample to the classes dy^2 + j^2, so a ring entry holds the row's h pair words -- sum in bits 0..19, count of valid samples in
// bits 20.. -- and, as in k_speckle_u16, the row's S2 with its centre sample in bits 40..55.  Per pixel the k ring rows' words are added
// class by class in packed form (a class has at most 8 samples: T_c <= 8 * 65535 < 2^20), S1 and n are the classes' totals, S2 is kept
// as a running total; then the f64 tail: a, up to 9 EXPs, the two accumulations in ascending r2, one division.
template <uint32_t K>
struct FrostFilter {
    static constexpr uint32_t H = K / 2;
    static constexpr uint32_t NC = frost_class(2 * H * H) + 1;
    static constexpr uint64_t kS2Mask = (1ull << 40) - 1;
    static_assert(NC <= kFrostMaxClasses, "dist[] holds every class");
    const SpeckleExtArgs &xa;
    uint32_t pr[K][H];
    uint64_t e2[K];
    uint64_t ts2 = 0;
    __device__ __forceinline__ explicit FrostFilter(const SpeckleExtArgs &args) : xa(args) {
#pragma unroll
        for (uint32_t r = 0; r < K; ++r) {
            e2[r] = 0ull;
#pragma unroll
            for (uint32_t j = 0; j < H; ++j) pr[r][j] = 0u;
        }
    }
    __device__ __forceinline__ void take(uint32_t r, const uint16_t *p) {
        const uint32_t c = p[H];
        uint64_t s2 = c * c; // (c < 2^16: the 32-bit product is the whole one)
#pragma unroll
        for (uint32_t j = 1; j <= H; ++j) {
            const uint32_t lo = p[H - j], hi = p[H + j];
            pr[r][j - 1] = (lo + hi) | (((lo != 0u) + (hi != 0u)) << 20);
            s2 += lo * lo;
            s2 += hi * hi;
        }
        ts2 = ts2 + s2 - (e2[r] & kS2Mask);
        e2[r] = s2 | ((uint64_t)c << 40);
    }
    __device__ __forceinline__ float pixel(uint32_t r) const {
        uint32_t cls[NC];
#pragma unroll
        for (uint32_t k = 0; k < NC; ++k) cls[k] = 0u;
#pragma unroll
        for (uint32_t dyi = 0; dyi < K; ++dyi) { // the window's rows, top to bottom: ring entry (r + 1 + dyi) % K
            const uint32_t slot = (r + 1 + dyi) % K, dy = dyi > H ? dyi - H : H - dyi;
            const uint32_t cc = (uint32_t)(e2[slot] >> 40);
            cls[frost_class(dy * dy)] += cc | ((uint32_t)(cc != 0u) << 20);
#pragma unroll
            for (uint32_t j = 1; j <= H; ++j) cls[frost_class(dy * dy + j * j)] += pr[slot][j - 1];
        }
        const uint32_t v = (uint32_t)(e2[(r + K - H) % K] >> 40);
        uint32_t n = 0, s1 = 0;
#pragma unroll
        for (uint32_t k = 0; k < NC; ++k) { n += cls[k] >> 20; s1 += cls[k] & 0xfffffu; }
        const uint64_t A = (uint64_t)s1 * s1;
        const uint64_t D = (uint64_t)n * ts2 - A;
        const double aa = xa.damping * ((double)D / (double)max(A, (uint64_t)1)); // (A >= 1 wherever the centre is valid)
        double num = (double)(cls[0] & 0xfffffu), den = (double)(cls[0] >> 20);    // 0.0 + 1.0 * T_0 and 0.0 + 1.0 * N_0, bit for bit
#pragma unroll
        for (uint32_t k = 1; k < NC; ++k) {
            const double w = speckle_exp(-(aa * xa.dist[k]));
            num = num + w * (double)(cls[k] & 0xfffffu);
            den = den + w * (double)(cls[k] >> 20);
        }
        return v ? (float)(num / den) : 0.0f;
    }
};

// what the u16 launchers check, and their grid; 0: refused
unsigned speckle_u16_grid(const SpeckleArgs &a) {
    if (a.band_rows > kSpeckleMaxBandRows || !a.rows || !a.cols || a.rows > kSpeckleMaxDim || a.cols > kSpeckleMaxDim) return 0;
    return band_grid(a.cols, kSpeckleThreads, a.rows, a.band_rows, a.io.nbands);
}

// their one window x load-width dispatch: launch(K, VEC) with both as integral constants; false: no such window
template <typename Launch>
bool by_window_vec(int window, bool vec, Launch launch) {
    using std::integral_constant;
    switch (window * 2 + (vec ? 1 : 0)) {
    case 6: launch(integral_constant<uint32_t, 3>{}, integral_constant<bool, false>{}); break;
    case 7: launch(integral_constant<uint32_t, 3>{}, integral_constant<bool, true>{}); break;
    case 10: launch(integral_constant<uint32_t, 5>{}, integral_constant<bool, false>{}); break;
    case 11: launch(integral_constant<uint32_t, 5>{}, integral_constant<bool, true>{}); break;
    case 14: launch(integral_constant<uint32_t, 7>{}, integral_constant<bool, false>{}); break;
    case 15: launch(integral_constant<uint32_t, 7>{}, integral_constant<bool, true>{}); break;
    default: return false;
    }
    return true;
}

} // namespace

template <uint32_t K, bool VEC>
__global__ __launch_bounds__(kSpeckleThreads) void k_speckle_frost_u16(SpeckleExtArgs xa) {
    FrostFilter<K> f(xa);
    speckle_band_walk<K, VEC>(xa.base, f);
}

// Refined Lee, window 7.  Beside k_speckle_u16's ring and running totals at k = 7 -- which give the fallback, Lee 7 through the same
// speckle_tail, and tell a directed pixel: 49 valid samples -- a ring entry keeps the row's 7 samples themselves in 4 words, so a pixel
// has its whole window in registers.  From them, for every pixel: the row sums of three columns -> the nine block sums -> the four
// gradients -> the direction and the side -> S1 and S2 of the chosen half, each of the 49 samples counted or not by the sign of
// ax * dx + ay * dy (E: (1, 0), NE: (1, -1), N: (0, -1), NW: (-1, -1); W, SW, S, SE: the negatives).  One tail, fed with the half's
// (28, S1, A, D) or with the window's.
// This kernel keeps its own copy of the band walk: as a filter of speckle_band_walk the same instructions come out scheduled so that
// they need 271 registers instead of 161 (occupancy 1 instead of 3).
template <bool VEC>
__global__ __launch_bounds__(kSpeckleThreads) void k_speckle_rlee_u16(SpeckleExtArgs xa) {
    const SpeckleArgs &a = xa.base;
    constexpr uint32_t K = 7, H = 3, ROWS = 28;
    using Stager = SpeckleStager<ROWS, VEC>;
    __shared__ uint4 s_stage[2][Stager::NVEC];
    const uint32_t tid = threadIdx.x;
    const BandTile tl = band_tile(a.io, a.cols, kSpeckleThreads, a.rows, a.band_rows);
    const uint16_t *src = static_cast<const uint16_t *>(tl.src);
    const uint32_t x0 = tl.strip * kSpeckleThreads, i0 = tl.rb * a.band_rows, i1 = min(i0 + a.band_rows, a.rows);
    const int32_t ys = (int32_t)i0 - (int32_t)H, ye = (int32_t)i1 + (int32_t)H;
    const uint32_t nstages = ((uint32_t)(ye - ys) + ROWS - 1) / ROWS;
    const bool active = x0 + tid < a.cols;
    Stager st;
    st.init(tid, x0, a.cols);
    st.load(src, a, ys, ye, 0);
    st.write(s_stage[0], tid);
    __syncthreads();
    uint32_t e1[K], raw[K][4];
    uint64_t e2[K];
#pragma unroll
    for (uint32_t r = 0; r < K; ++r) {
        e1[r] = 0u; e2[r] = 0ull;
#pragma unroll
        for (uint32_t q = 0; q < 4; ++q) raw[r][q] = 0u;
    }
    uint32_t tn = 0, ts1 = 0;
    uint64_t ts2 = 0;
    for (uint32_t s = 0; s < nstages; ++s) {
        const bool more = s + 1 < nstages;
        if (more) st.load(src, a, ys, ye, s + 1);
        const uint16_t *lds = reinterpret_cast<const uint16_t *>(&s_stage[s & 1][0]) + tid + kSpeckleHaloCols - H;
        int32_t y = ys + (int32_t)(s * ROWS);
        for (uint32_t g = 0; g < ROWS / K && y < ye; ++g) {
#pragma unroll
            for (uint32_t r = 0; r < K; ++r, ++y) {
                if (y >= ye) break; // (uniform)
                const uint16_t *p = lds + (g * K + r) * kSpeckleRowLen;
                uint32_t smp[K];
                uint32_t n = 0, s1 = 0;
                uint64_t s2 = 0;
#pragma unroll
                for (uint32_t j = 0; j < K; ++j) {
                    smp[j] = p[j];
                    n += smp[j] != 0u;
                    s1 += smp[j];
                    s2 += smp[j] * smp[j]; // (< 2^32: the 32-bit product is the whole one)
                }
                tn = tn + n - (e1[r] >> 19);
                ts1 = ts1 + s1 - (e1[r] & 0x7ffffu);
                ts2 = ts2 + s2 - e2[r];
                e1[r] = s1 | (n << 19);
                e2[r] = s2;
                raw[r][0] = smp[0] | (smp[1] << 16);
                raw[r][1] = smp[2] | (smp[3] << 16);
                raw[r][2] = smp[4] | (smp[5] << 16);
                raw[r][3] = smp[6];
                const int32_t yo = y - (int32_t)H; // the output row whose window this row completes
                if (yo < (int32_t)i0) continue; // (uniform)
                // sample (dyi, dxi) of the window, 0..6 each: ring entry (r + 1 + dyi) % K
                auto at = [&](uint32_t dyi, uint32_t dxi) -> uint32_t {
                    const uint32_t w = raw[(r + 1 + dyi) % K][dxi / 2];
                    return dxi & 1 ? w >> 16 : w & 0xffffu;
                };
                const uint32_t v = at(H, H);
                // block (i, j): rows 2i..2i+2, columns 2j..2j+2 of the window (named scalars: nothing here may be indexed by a lane's value)
                auto block = [&](uint32_t i, uint32_t j) -> int32_t {
                    uint32_t b = 0;
#pragma unroll
                    for (uint32_t dy = 0; dy < 3; ++dy)
#pragma unroll
                        for (uint32_t dx = 0; dx < 3; ++dx) b += at(2 * i + dy, 2 * j + dx);
                    return (int32_t)b;
                };
                const int32_t b00 = block(0, 0), b01 = block(0, 1), b02 = block(0, 2), b10 = block(1, 0), b11 = block(1, 1), b12 = block(1, 2),
                              b20 = block(2, 0), b21 = block(2, 1), b22 = block(2, 2);
                const int32_t g0 = abs((b02 + b12 + b22) - (b00 + b10 + b20));
                const int32_t g1 = abs((b01 + b02 + b12) - (b10 + b20 + b21));
                const int32_t g2 = abs((b00 + b01 + b02) - (b20 + b21 + b22));
                const int32_t g3 = abs((b00 + b01 + b10) - (b12 + b21 + b22));
                // the largest gradient, the lowest index on a tie; P and Q and P's half-plane (ax, ay)
                int32_t gm = g0, P = b12, Q = b10, ax = 1, ay = 0;
                const bool t1 = g1 > gm;
                gm = t1 ? g1 : gm; P = t1 ? b02 : P; Q = t1 ? b20 : Q; ay = t1 ? -1 : ay;
                const bool t2 = g2 > gm;
                gm = t2 ? g2 : gm; P = t2 ? b01 : P; Q = t2 ? b21 : Q; ax = t2 ? 0 : ax; ay = t2 ? -1 : ay;
                const bool t3 = g3 > gm;
                P = t3 ? b00 : P; Q = t3 ? b22 : Q; ax = t3 ? -1 : ax; ay = t3 ? -1 : ay;
                const bool useP = abs(P - b11) <= abs(Q - b11);
                ax = useP ? ax : -ax;
                ay = useP ? ay : -ay;
                uint32_t hs1 = 0;
                uint64_t hs2 = 0;
#pragma unroll
                for (uint32_t dyi = 0; dyi < K; ++dyi) {
                    const int32_t base = ay * ((int32_t)dyi - (int32_t)H);
#pragma unroll
                    for (uint32_t dxi = 0; dxi < K; ++dxi) {
                        const uint32_t sv = base + ax * ((int32_t)dxi - (int32_t)H) >= 0 ? at(dyi, dxi) : 0u;
                        hs1 += sv;
                        hs2 += sv * sv;
                    }
                }
                const bool directed = tn == K * K; // the window lies inside the raster and all its 49 samples are valid
                const uint32_t fn = directed ? 28u : max(tn, 1u), fs1 = directed ? hs1 : ts1;
                const uint64_t fs2 = directed ? hs2 : ts2;
                const uint64_t A = (uint64_t)fs1 * fs1;
                const uint64_t D = (uint64_t)fn * fs2 - A;
                float out = speckle_tail((double)fn, (double)fs1, (double)A, (double)D, (double)v, a.cu2, 1.0);
                out = v ? out : 0.0f;
                if (active) tl.dst[(size_t)yo * a.io.out_pitch + x0 + tid] = out;
            }
        }
        if (more) st.write(s_stage[(s + 1) & 1], tid);
        __syncthreads();
    }
}

hipError_t launch_speckle_u16(const SpeckleArgs &a, int window, bool vec, hipStream_t s) {
    const dim3 g(speckle_u16_grid(a)), b(kSpeckleThreads);
    if (!g.x) return hipErrorInvalidValue;
    if (!by_window_vec(window, vec, [&](auto k, auto v) { hipLaunchKernelGGL((k_speckle_u16<decltype(k)::value, decltype(v)::value>), g, b, 0, s, a); }))
        return hipErrorInvalidValue;
    return hipGetLastError();
}

hipError_t launch_speckle_ext_u16(const SpeckleExtArgs &xa, bool refined, int window, bool vec, hipStream_t s) {
    const dim3 g(speckle_u16_grid(xa.base)), b(kSpeckleThreads);
    if (!g.x) return hipErrorInvalidValue;
    if (refined) {
        if (window != 7) return hipErrorInvalidValue;
        if (vec) hipLaunchKernelGGL((k_speckle_rlee_u16<true>), g, b, 0, s, xa);
        else hipLaunchKernelGGL((k_speckle_rlee_u16<false>), g, b, 0, s, xa);
    } else if (!by_window_vec(window, vec, [&](auto k, auto v) { hipLaunchKernelGGL((k_speckle_frost_u16<decltype(k)::value, decltype(v)::value>), g, b, 0, s, xa); })) {
        return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

hipError_t launch_speckle_f32(const SpeckleArgs &a, int window, hipStream_t s) {
    if (!a.rows || !a.cols || a.rows > kSpeckleMaxDim || a.cols > kSpeckleMaxDim) return hipErrorInvalidValue;
    const dim3 g(band_grid(a.cols, kSpeckleThreads, a.rows, kSpeckleF32BandRows, a.io.nbands)), b(kSpeckleThreads);
    if (!g.x) return hipErrorInvalidValue;
    switch (window) {
    case 3: hipLaunchKernelGGL((k_speckle_f32<3>), g, b, 0, s, a); break;
    case 5: hipLaunchKernelGGL((k_speckle_f32<5>), g, b, 0, s, a); break;
    case 7: hipLaunchKernelGGL((k_speckle_f32<7>), g, b, 0, s, a); break;
    default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

} // namespace sarpro
