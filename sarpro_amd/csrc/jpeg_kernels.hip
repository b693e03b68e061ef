// jpeg_kernels.hip -- baseline JPEG on the device: what write_rgb_jpeg / write_gray_jpeg (io/writers/jpeg.rs:14,27) hand to
// jpeg_encoder::Encoder::new(w, 100): quality 100 (every quantisation entry 1), 4:4:4, the Annex K Huffman tables, plus restart
// intervals, which make the entropy-coded scan a set of independent segments.
//
//   1. k_jpeg_transform   8 lanes per 8 x 8 block (one row each): libjpeg's jccolor arithmetic, edge replication, level shift, the
//                         row pass of jfdctint, a transposition through LDS, the column pass, quantisation by 8, zigzag.  The quantised
//                         coefficients are materialised (2 B per sample): both entropy passes read them.
//   2. k_jpeg_entropy     one wave per restart segment, one lane per coefficient of the block in hand: a ballot of the non-zero
//                         lanes gives every lane its zero run, a wave prefix sum of the code lengths its bit offset; the block's
//                         bits are assembled in LDS and leave as bytes, 0xFF followed by its stuffed 0x00 (a second ballot gives the
//                         byte offsets).  <false> only counts (the segment's exact length), <true> writes at the final offset.
//   3. k_jpeg_scan_*      exclusive scan of the segment lengths between the two.
// Parity with the jpeg-encoder crate itself is unpinned (its source is absent); the arithmetic is libjpeg's (jccolor, jfdctint,
// jchuff), which the crate is documented to port, and the scan is checked byte for byte against libjpeg-turbo.
#include "jpeg_kernels.h"

namespace sarpro {
namespace {

#define FIX_0_298631336 2446
#define FIX_0_390180644 3196
#define FIX_0_541196100 4433
#define FIX_0_765366865 6270
#define FIX_0_899976223 7373
#define FIX_1_175875602 9633
#define FIX_1_501321110 12299
#define FIX_1_847759065 15137
#define FIX_1_961570560 16069
#define FIX_2_053119869 16819
#define FIX_2_562915447 20995
#define FIX_3_072711026 25172

__device__ __forceinline__ int descale(int x, int n) { return (x + (1 << (n - 1))) >> n; }

// one pass of jfdctint over 8 values, in place.  PASS = 1: rows (outputs 0 and 4 scaled up by PASS1_BITS = 2, the others descaled by
// CONST_BITS - PASS1_BITS = 11); PASS = 2: columns (descaled by 2 and by CONST_BITS + PASS1_BITS = 15)
template <int PASS>
__device__ __forceinline__ void fdct8(int (&d)[8]) {
    const int tmp0 = d[0] + d[7], tmp7 = d[0] - d[7], tmp1 = d[1] + d[6], tmp6 = d[1] - d[6];
    const int tmp2 = d[2] + d[5], tmp5 = d[2] - d[5], tmp3 = d[3] + d[4], tmp4 = d[3] - d[4];
    const int tmp10 = tmp0 + tmp3, tmp13 = tmp0 - tmp3, tmp11 = tmp1 + tmp2, tmp12 = tmp1 - tmp2;
    constexpr int kOdd = PASS == 1 ? 11 : 15;
    if (PASS == 1) { d[0] = (tmp10 + tmp11) << 2; d[4] = (tmp10 - tmp11) << 2; }
    else { d[0] = descale(tmp10 + tmp11, 2); d[4] = descale(tmp10 - tmp11, 2); }
    int z1 = (tmp12 + tmp13) * FIX_0_541196100;
    d[2] = descale(z1 + tmp13 * FIX_0_765366865, kOdd);
    d[6] = descale(z1 + tmp12 * (-FIX_1_847759065), kOdd);
    z1 = tmp4 + tmp7;
    int z2 = tmp5 + tmp6, z3 = tmp4 + tmp6, z4 = tmp5 + tmp7;
    const int z5 = (z3 + z4) * FIX_1_175875602;
    const int t4 = tmp4 * FIX_0_298631336, t5 = tmp5 * FIX_2_053119869, t6 = tmp6 * FIX_3_072711026, t7 = tmp7 * FIX_1_501321110;
    z1 *= -FIX_0_899976223; z2 *= -FIX_2_562915447; z3 *= -FIX_1_961570560; z4 *= -FIX_0_390180644;
    z3 += z5; z4 += z5;
    d[7] = descale(t4 + z1 + z3, kOdd);
    d[5] = descale(t5 + z2 + z4, kOdd);
    d[3] = descale(t6 + z2 + z3, kOdd);
    d[1] = descale(t7 + z1 + z4, kOdd);
}

constexpr int kXformBlocks = 32; // 8 x 8 blocks (MCUs) per workgroup of 256 threads

__global__ __launch_bounds__(256) void k_jpeg_transform(JpegArgs a) {
    __shared__ int s_t[3][kXformBlocks][8][9]; // row-pass results; 9: the column reads of the 4 blocks of a half-wave fall on distinct banks
    __shared__ uint8_t s_zz[64];
    const int tid = threadIdx.x, blk = tid >> 3, r = tid & 7;
    if (tid < 64) s_zz[tid] = a.tables->zz_pos[tid];
    const uint64_t m = (uint64_t)blockIdx.x * kXformBlocks + blk;
    const bool active = m < a.n_mcus;
    const int nc = (int)a.components;
    if (active) {
        const uint32_t bx = (uint32_t)(m % a.mcus_x), by = (uint32_t)(m / a.mcus_x);
        const uint32_t y = min(by * 8 + r, a.rows - 1);                  // edge blocks replicate the last row ...
        const uint8_t *row = a.pixels + (size_t)y * a.pitch_bytes;
        int d[3][8];
#pragma unroll
        for (int c = 0; c < 8; ++c) {
            const uint32_t x = min(bx * 8 + c, a.cols - 1);              // ... and the last column (of the converted samples: the conversion is per pixel)
            if (nc == 3) {
                const int R = row[(size_t)x * 3], G = row[(size_t)x * 3 + 1], B = row[(size_t)x * 3 + 2];
                // jccolor: 16 fractional bits, FIX(x) = int(x * 65536 + 0.5)
                d[0][c] = ((19595 * R + 38470 * G + 7471 * B + 32768) >> 16) - 128;
                d[1][c] = ((-11059 * R - 21709 * G + 32768 * B + (128 << 16) + 32767) >> 16) - 128;
                d[2][c] = ((32768 * R - 27439 * G - 5329 * B + (128 << 16) + 32767) >> 16) - 128;
            } else {
                d[0][c] = (int)row[x] - 128;
            }
        }
        for (int k = 0; k < nc; ++k) {
            fdct8<1>(d[k]);
#pragma unroll
            for (int c = 0; c < 8; ++c) s_t[k][blk][r][c] = d[k][c];
        }
    }
    __syncthreads();
    if (!active) return;
    for (int k = 0; k < nc; ++k) {
        int d[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) d[i] = s_t[k][blk][i][r]; // this lane: column r of the block
        fdct8<2>(d);
        int16_t *dst = a.coef + (m * nc + k) * 64;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int c = d[i];
            const int q = c < 0 ? -((-c + 4) >> 3) : (c + 4) >> 3; // table entry 1 x the transform's scale 8
            dst[s_zz[i * 8 + r]] = (int16_t)q;
        }
    }
}

constexpr int kBitWords = 128; // 64 lanes x at most 59 bits (three ZRL + the longest code + 10 value bits) + 7 carried bits = 3783 bits < 4096

template <bool WRITE>
__global__ __launch_bounds__(64) void k_jpeg_entropy(JpegArgs a) {
    __shared__ uint32_t s_dc[2][16];
    __shared__ uint32_t s_ac[2][256];
    __shared__ uint32_t s_bits[kBitWords]; // the block's bit stream, first bit in the top bit of word 0
    const int lane = threadIdx.x;
    const uint64_t seg = blockIdx.x;
    if (lane < 32) s_dc[lane >> 4][lane & 15] = a.tables->dc[lane >> 4][lane & 15];
    for (int i = lane; i < 512; i += 64) s_ac[i >> 8][i & 255] = a.tables->ac[i >> 8][i & 255];
    s_bits[lane] = 0; s_bits[lane + 64] = 0;
    __syncthreads();
    const int nc = (int)a.components;
    const uint64_t m0 = seg * a.restart_mcus, m1 = min(m0 + (uint64_t)a.restart_mcus, a.n_mcus);
    const uint64_t cap = a.out_capacity;
    uint64_t pos = WRITE ? a.header_bytes + a.seg_off[seg] : 0;
    const uint64_t pos0 = pos;
    uint32_t carry_bits = 0, carry_byte = 0;
    const uint64_t below = lane ? (1ull << lane) - 1 : 0ull;
    const int16_t *base = a.coef + m0 * (uint64_t)nc * 64;
    const uint32_t nblk = (uint32_t)(m1 - m0) * (uint32_t)nc; // the segment's blocks: MCU after MCU, component after component
    int vnext = base[lane];
    int pd0 = 0, pd1 = 0, pd2 = 0; // lane 0: the previous DC of each component (a restart resets the predictors)
    int c = 0;
    for (uint32_t b = 0; b < nblk; ++b, c = c + 1 == nc ? 0 : c + 1) {
        const int tb = c ? 1 : 0;
        int v = vnext;
        if (b + 1 < nblk) vnext = base[(size_t)(b + 1) * 64 + lane]; // the next block's load is in flight while this one is coded
        if (lane == 0) { // DC: the difference to the segment's previous block of this component
            const int raw = v;
            if (c == 0) { v -= pd0; pd0 = raw; } else if (c == 1) { v -= pd1; pd1 = raw; } else { v -= pd2; pd2 = raw; }
        }
        const uint64_t nzmask = __ballot(v != 0);
        uint64_t acc = 0;
        uint32_t len = 0;
        const uint32_t mag = (uint32_t)(v < 0 ? -v : v);
        const uint32_t size = mag ? 32u - (uint32_t)__clz(mag) : 0u;
        const uint32_t extra = (uint32_t)(v < 0 ? v - 1 : v) & ((1u << size) - 1u);
        if (lane == 0) {
            const uint32_t e = s_dc[tb][size & 15u];
            acc = e & 0xFFFFu; len = e >> 16;
            acc = (acc << size) | extra; len += size;
        } else if (v != 0) {
            const uint64_t prev_set = (nzmask | 1ull) & below;       // position 0 anchors the first run
            const int prev = 63 - __clzll((long long)prev_set);
            const uint32_t run = (uint32_t)(lane - prev - 1);
            const uint32_t zrl = s_ac[tb][0xF0];
            for (uint32_t i = 0; i < (run >> 4); ++i) { acc = (acc << (zrl >> 16)) | (zrl & 0xFFFFu); len += zrl >> 16; }
            const uint32_t e = s_ac[tb][(((run & 15u) << 4) | size) & 255u];
            acc = (acc << (e >> 16)) | (e & 0xFFFFu); len += e >> 16;
            acc = (acc << size) | extra; len += size;
        } else if (lane == 63) { // the block ends in zeros: EOB
            const uint32_t e = s_ac[tb][0];
            acc = e & 0xFFFFu; len = e >> 16;
        }
        uint32_t inc = len;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const uint32_t t = __shfl_up(inc, d);
            if (lane >= d) inc += t;
        }
        const uint32_t tot = carry_bits + __shfl(inc, 63);
        if (len) {
            const uint64_t al = acc << (64 - len); // left-aligned
            const uint32_t o = carry_bits + inc - len, w = o >> 5, s = o & 31u;
            const uint32_t hi = (uint32_t)(al >> (32 + s)), mid = (uint32_t)(al >> s), lo = s ? (uint32_t)(al << (32 - s)) : 0u;
            if (hi) atomicOr(&s_bits[w], hi);
            if (mid) atomicOr(&s_bits[w + 1], mid);
            if (lo) atomicOr(&s_bits[w + 2], lo);
        }
        __syncthreads();
        const uint32_t nb = tot >> 3; // complete bytes
        for (uint32_t j0 = 0; j0 < nb; j0 += 64) {
            const uint32_t j = j0 + lane;
            const bool valid = j < nb;
            const uint32_t b = valid ? (s_bits[j >> 2] >> (24 - 8 * (j & 3))) & 0xFFu : 0u;
            const bool ff = valid && b == 0xFFu;
            const uint64_t ffmask = __ballot(ff);
            if (WRITE && valid) {
                const uint64_t p = pos + lane + (uint64_t)__popcll(ffmask & below);
                if (p < cap) a.out[p] = (uint8_t)b;
                if (ff && p + 1 < cap) a.out[p + 1] = 0;
            }
            pos += min(64u, nb - j0) + (uint32_t)__popcll(ffmask);
        }
        carry_byte = (s_bits[nb >> 2] >> (24 - 8 * (nb & 3))) & 0xFFu;
        carry_bits = tot & 7u;
        __syncthreads();
        s_bits[lane] = 0; s_bits[lane + 64] = 0;
        __syncthreads();
        if (lane == 0) s_bits[0] = carry_byte << 24;
        __syncthreads();
    }
    if (carry_bits) { // the last partial byte is padded with 1-bits (and stuffed like any other)
        const uint32_t b = carry_byte | (0xFFu >> carry_bits);
        if (WRITE && lane == 0) {
            if (pos < cap) a.out[pos] = (uint8_t)b;
            if (b == 0xFFu && pos + 1 < cap) a.out[pos + 1] = 0;
        }
        pos += b == 0xFFu ? 2 : 1;
    }
    if (WRITE && lane == 0) { // RSTn behind every segment but the last; EOI behind that one
        if (pos < cap) a.out[pos] = 0xFF;
        if (pos + 1 < cap) a.out[pos + 1] = seg + 1 < a.n_segments ? (uint8_t)(0xD0 + (seg & 7)) : (uint8_t)0xD9;
    }
    pos += 2;
    if (!WRITE && lane == 0) a.seg_len[seg] = (uint32_t)(pos - pos0);
}

// ---- exclusive scan of the segment lengths: per-chunk sums, their scan in one workgroup, the chunks' own scans on top
constexpr int kScanPerThread = kJpegScanChunk / 256;

__device__ __forceinline__ uint64_t block_exclusive_scan_256(uint64_t v, uint64_t *s, uint64_t *total) {
    const int t = threadIdx.x;
    s[t] = v;
    __syncthreads();
    for (int d = 1; d < 256; d <<= 1) {
        const uint64_t x = t >= d ? s[t - d] : 0;
        __syncthreads();
        s[t] += x;
        __syncthreads();
    }
    const uint64_t inc = s[t];
    *total = s[255];
    __syncthreads();
    return inc - v;
}

__global__ __launch_bounds__(256) void k_jpeg_scan_sums(JpegArgs a) {
    __shared__ uint64_t s[256];
    const uint64_t base = (uint64_t)blockIdx.x * kJpegScanChunk;
    uint64_t v = 0;
    for (int i = 0; i < kScanPerThread; ++i) {
        const uint64_t k = base + (uint64_t)i * 256 + threadIdx.x;
        if (k < a.n_segments) v += a.seg_len[k];
    }
    uint64_t total;
    (void)block_exclusive_scan_256(v, s, &total);
    if (threadIdx.x == 0) a.scan_sums[blockIdx.x] = total;
}

__global__ __launch_bounds__(256) void k_jpeg_scan_chunks(JpegArgs a, uint64_t n_chunks) {
    __shared__ uint64_t s[256];
    uint64_t carry = 0;
    for (uint64_t c0 = 0; c0 < n_chunks; c0 += 256) {
        const uint64_t k = c0 + threadIdx.x;
        const uint64_t v = k < n_chunks ? a.scan_sums[k] : 0;
        uint64_t total;
        const uint64_t ex = block_exclusive_scan_256(v, s, &total);
        if (k < n_chunks) a.scan_sums[k] = carry + ex;
        carry += total;
    }
    if (threadIdx.x == 0) a.seg_off[a.n_segments] = carry;
}

__global__ __launch_bounds__(256) void k_jpeg_scan_final(JpegArgs a) {
    __shared__ uint64_t s[256];
    const uint64_t first = (uint64_t)blockIdx.x * kJpegScanChunk + (uint64_t)threadIdx.x * kScanPerThread;
    uint32_t l[kScanPerThread];
    uint64_t v = 0;
    for (int i = 0; i < kScanPerThread; ++i) {
        l[i] = first + i < a.n_segments ? a.seg_len[first + i] : 0u;
        v += l[i];
    }
    uint64_t total;
    uint64_t off = a.scan_sums[blockIdx.x] + block_exclusive_scan_256(v, s, &total);
    for (int i = 0; i < kScanPerThread; ++i) {
        if (first + i < a.n_segments) a.seg_off[first + i] = off;
        off += l[i];
    }
}

} // namespace

hipError_t launch_jpeg_transform(const JpegArgs &a, hipStream_t s) {
    const uint64_t grid = (a.n_mcus + kXformBlocks - 1) / kXformBlocks;
    hipLaunchKernelGGL(k_jpeg_transform, dim3((unsigned)grid), dim3(256), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_jpeg_entropy_size(const JpegArgs &a, hipStream_t s) {
    hipLaunchKernelGGL(k_jpeg_entropy<false>, dim3((unsigned)a.n_segments), dim3(64), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_jpeg_scan(const JpegArgs &a, hipStream_t s) {
    const uint64_t n_chunks = (a.n_segments + kJpegScanChunk - 1) / kJpegScanChunk;
    hipLaunchKernelGGL(k_jpeg_scan_sums, dim3((unsigned)n_chunks), dim3(256), 0, s, a);
    hipLaunchKernelGGL(k_jpeg_scan_chunks, dim3(1), dim3(256), 0, s, a, n_chunks);
    hipLaunchKernelGGL(k_jpeg_scan_final, dim3((unsigned)n_chunks), dim3(256), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_jpeg_entropy_write(const JpegArgs &a, hipStream_t s) {
    hipLaunchKernelGGL(k_jpeg_entropy<true>, dim3((unsigned)a.n_segments), dim3(64), 0, s, a);
    return hipGetLastError();
}

} // namespace sarpro
