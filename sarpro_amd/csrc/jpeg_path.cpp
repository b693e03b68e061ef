// jpeg_path.cpp -- write_rgb_jpeg / write_gray_jpeg (io/writers/jpeg.rs:14,27; called from save.rs:317-403 and api/mod.rs:404-437) on the
// device: the raster is encoded where it lies and only the file crosses PCIe.  Both writers call jpeg_encoder::Encoder::new(w, 100):
// baseline, quality 100 (every quantisation entry 1), 4:4:4 (the crate's choice for quality >= 90), the Annex K Huffman tables.  Restart
// intervals (a DRI segment any decoder reads) cut the scan into independent segments, which is what the kernels parallelise over.
// Parity with the jpeg-encoder crate itself is unpinned (its source is absent); it is documented as a port of libjpeg's jfdctint and
// colour arithmetic, which jpeg_kernels.hip restates and the tests check byte for byte against libjpeg-turbo.
#include <algorithm>
#include <cstring>

#include "internal.h"
#include "jpeg_kernels.h"

using namespace sarpro;

#define HIPCHK(ctx, expr)                                                                         \
    do {                                                                                          \
        hipError_t e__ = (expr);                                                                  \
        if (e__ != hipSuccess) {                                                                  \
            (ctx)->err = std::string(#expr) + ": " + hipGetErrorString(e__);                      \
            return e__ == hipErrorOutOfMemory ? SARPRO_HIP_ERR_OOM : SARPRO_HIP_ERR_HIP;          \
        }                                                                                         \
    } while (0)
#define RETCHK(expr)                                   \
    do {                                               \
        int rc__ = (expr);                             \
        if (rc__ != SARPRO_HIP_OK) return rc__;        \
    } while (0)

static int fail(sarpro_hip_ctx *ctx, int code, const char *msg) {
    if (ctx) ctx->err = msg;
    return code;
}

namespace {

// The library's restart interval in MCUs (restart_mcus = 0): DESIGN.md, "JPEG encoding", has the measurements behind it.
constexpr uint32_t kJpegDefaultRestartMcus = 8;

// ITU-T T.81 Annex K.3-K.6: code counts per length 1..16, then the symbols in code order
struct HuffSpec { uint8_t bits[16]; const uint8_t *vals; int nvals; };
const uint8_t kDcVals[12] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11};
const uint8_t kAcLumaVals[162] = {
    0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81, 0x91, 0xa1,
    0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a, 0x25, 0x26,
    0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56,
    0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85,
    0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa,
    0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6,
    0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9,
    0xfa};
const uint8_t kAcChromaVals[162] = {
    0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08, 0x14, 0x42,
    0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17, 0x18, 0x19,
    0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55,
    0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83,
    0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8,
    0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4,
    0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9,
    0xfa};
// index: class * 2 + table (DC luminance, DC chrominance, AC luminance, AC chrominance)
const HuffSpec kHuff[4] = {
    {{0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0}, kDcVals, 12},
    {{0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0}, kDcVals, 12},
    {{0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d}, kAcLumaVals, 162},
    {{0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77}, kAcChromaVals, 162},
};

// T.81 Annex C: canonical codes from the counts.  out[symbol] = (length << 16) | code; returns the longest length
int huff_codes(const HuffSpec &h, uint32_t *out, int nout) {
    for (int i = 0; i < nout; ++i) out[i] = 0;
    uint32_t code = 0;
    int k = 0, longest = 0;
    for (int len = 1; len <= 16; ++len) {
        for (int i = 0; i < h.bits[len - 1]; ++i, ++k) {
            if (h.vals[k] < nout) out[h.vals[k]] = ((uint32_t)len << 16) | code;
            ++code;
            longest = len;
        }
        code <<= 1;
    }
    return longest;
}

void zigzag_positions(uint8_t pos[64]) { // walk the anti-diagonals, alternating direction
    int k = 0;
    for (int s = 0; s < 15; ++s)
        for (int i = 0; i <= s; ++i) {
            const int r = (s & 1) ? i : s - i, c = s - r;
            if (r < 8 && c < 8) pos[r * 8 + c] = (uint8_t)k++;
        }
}

void build_tables(JpegCodeTables *t) {
    huff_codes(kHuff[0], t->dc[0], 16); huff_codes(kHuff[1], t->dc[1], 16);
    huff_codes(kHuff[2], t->ac[0], 256); huff_codes(kHuff[3], t->ac[1], 256);
    zigzag_positions(t->zz_pos);
}

bool args_ok(size_t cols, size_t rows, int components, unsigned restart_mcus) {
    return cols >= 1 && cols <= 65535 && rows >= 1 && rows <= 65535 && (components == 1 || components == 3) && restart_mcus <= 65535;
}

struct Put {
    uint8_t *p; size_t cap, n = 0;
    void b(unsigned v) { if (n < cap) p[n] = (uint8_t)v; ++n; }
    void w(unsigned v) { b(v >> 8); b(v & 0xFF); }
};

// SOI .. SOS header: returns the length; writes at most cap bytes
size_t write_header(size_t cols, size_t rows, int nc, unsigned R, uint8_t *out, size_t cap) {
    Put o{out, cap};
    o.w(0xFFD8);
    o.w(0xFFE0); o.w(16); for (char ch : {'J', 'F', 'I', 'F', '\0'}) o.b((unsigned char)ch);
    o.b(1); o.b(1); o.b(0); o.w(1); o.w(1); o.b(0); o.b(0);                       // JFIF 1.01, no units, 1 x 1, no thumbnail
    for (int t = 0; t < (nc == 3 ? 2 : 1); ++t) { o.w(0xFFDB); o.w(67); o.b(t); for (int i = 0; i < 64; ++i) o.b(1); } // quality 100
    o.w(0xFFC0); o.w(8 + 3 * nc); o.b(8); o.w((unsigned)rows); o.w((unsigned)cols); o.b(nc);
    for (int c = 0; c < nc; ++c) { o.b(c + 1); o.b(0x11); o.b(c ? 1 : 0); }
    for (int t = 0; t < (nc == 3 ? 2 : 1); ++t)
        for (int cls = 0; cls < 2; ++cls) {
            const HuffSpec &h = kHuff[cls * 2 + t];
            o.w(0xFFC4); o.w(2 + 1 + 16 + h.nvals); o.b((cls << 4) | t);
            for (int i = 0; i < 16; ++i) o.b(h.bits[i]);
            for (int i = 0; i < h.nvals; ++i) o.b(h.vals[i]);
        }
    o.w(0xFFDD); o.w(4); o.w(R);
    o.w(0xFFDA); o.w(6 + 2 * nc); o.b(nc);
    for (int c = 0; c < nc; ++c) { o.b(c + 1); o.b(c ? 0x11 : 0x00); }
    o.b(0); o.b(63); o.b(0);
    return o.n;
}

// A capacity no file can exceed.  One block: its DC symbol is at most the longest DC code of its table plus 11 value bits (8-bit samples
// after the level shift give quantised DC values in [-1024, 1016], differences within +-2040: category 11); each of the 63 AC coefficients
// at most the longest AC code plus 10 value bits (category 10 is the limit for 8-bit input).  A coefficient that is zero costs less than
// one that is not: a ZRL or EOB symbol stands for 16 (or all remaining) positions at no more than the longest code.  A segment's bits are
// rounded up to a byte (the padding), every byte may be 0xFF and stuffed (factor 2), and the segment ends in a two-byte marker (RSTn, or
// EOI after the last).
size_t file_bound(size_t cols, size_t rows, int nc, unsigned R) {
    uint32_t tmp[256];
    const size_t dc_bits[2] = {(size_t)huff_codes(kHuff[0], tmp, 16) + 11, (size_t)huff_codes(kHuff[1], tmp, 16) + 11};
    const size_t ac_bits[2] = {(size_t)huff_codes(kHuff[2], tmp, 256) + 10, (size_t)huff_codes(kHuff[3], tmp, 256) + 10};
    size_t mcu_bits = dc_bits[0] + 63 * ac_bits[0];
    if (nc == 3) mcu_bits += 2 * (dc_bits[1] + 63 * ac_bits[1]);
    const size_t n_mcus = ((cols + 7) / 8) * ((rows + 7) / 8), full = n_mcus / R, rest = n_mcus % R;
    size_t bytes = write_header(cols, rows, nc, R, nullptr, 0);
    bytes += full * (2 * ((R * mcu_bits + 7) / 8) + 2);
    if (rest) bytes += 2 * ((rest * mcu_bits + 7) / 8) + 2;
    return bytes;
}

// Everything of one image enqueued on the context's stream: header, transform, sizing, offsets, writing, and the scan's length on its
// way to pinned memory (ctx->jpeg_host, first 8 bytes).  The caller synchronises once and adds *header_bytes.
int encode_enqueue(sarpro_hip_ctx *ctx, const uint8_t *d_pixels, size_t cols, size_t rows, size_t pitch_bytes, int nc, unsigned R,
                   uint8_t *d_out, size_t cap, size_t *header_bytes) {
    HIPCHK(ctx, hipSetDevice(ctx->device));
    HIPCHK(ctx, ctx->jpeg_host.reserve(4096));
    if (!ctx->jpeg_tables.p) {
        HIPCHK(ctx, ctx->jpeg_tables.reserve(sizeof(JpegCodeTables)));
        JpegCodeTables *t = reinterpret_cast<JpegCodeTables *>(ctx->jpeg_host.as<uint8_t>() + 64);
        build_tables(t);
        HIPCHK(ctx, hipMemcpyAsync(ctx->jpeg_tables.p, t, sizeof(JpegCodeTables), hipMemcpyHostToDevice, ctx->stream));
        HIPCHK(ctx, hipStreamSynchronize(ctx->stream)); // once per context: the pinned stage holds the header from here on
    }
    JpegArgs a{};
    a.pixels = d_pixels; a.pitch_bytes = pitch_bytes; a.cols = (uint32_t)cols; a.rows = (uint32_t)rows; a.components = (uint32_t)nc;
    a.mcus_x = (uint32_t)((cols + 7) / 8); a.mcus_y = (uint32_t)((rows + 7) / 8); a.restart_mcus = R;
    a.n_mcus = (uint64_t)a.mcus_x * a.mcus_y; a.n_segments = (a.n_mcus + R - 1) / R;
    const uint64_t n_chunks = (a.n_segments + kJpegScanChunk - 1) / kJpegScanChunk;
    HIPCHK(ctx, ctx->jpeg_coef.reserve(a.n_mcus * (size_t)nc * 64 * sizeof(int16_t)));
    HIPCHK(ctx, ctx->jpeg_seg.reserve((a.n_segments + 1 + n_chunks) * sizeof(uint64_t) + a.n_segments * sizeof(uint32_t)));
    a.coef = ctx->jpeg_coef.as<int16_t>();
    a.tables = ctx->jpeg_tables.as<JpegCodeTables>();
    a.seg_off = ctx->jpeg_seg.as<uint64_t>();
    a.scan_sums = a.seg_off + a.n_segments + 1;
    a.seg_len = reinterpret_cast<uint32_t *>(a.scan_sums + n_chunks);
    a.out = d_out; a.out_capacity = cap;
    uint8_t *h = ctx->jpeg_host.as<uint8_t>() + 64;
    const size_t hb = write_header(cols, rows, nc, R, h, 4096 - 64);
    a.header_bytes = hb;
    *header_bytes = hb;
    if (std::min(hb, cap)) HIPCHK(ctx, hipMemcpyAsync(d_out, h, std::min(hb, cap), hipMemcpyHostToDevice, ctx->stream));
    {
        KernelTimer t(ctx, "jpeg_transform");
        HIPCHK(ctx, launch_jpeg_transform(a, ctx->stream));
    }
    {
        KernelTimer t(ctx, "jpeg_entropy_size");
        HIPCHK(ctx, launch_jpeg_entropy_size(a, ctx->stream));
    }
    {
        KernelTimer t(ctx, "jpeg_scan");
        HIPCHK(ctx, launch_jpeg_scan(a, ctx->stream));
    }
    {
        KernelTimer t(ctx, "jpeg_entropy_write");
        HIPCHK(ctx, launch_jpeg_entropy_write(a, ctx->stream));
    }
    HIPCHK(ctx, hipMemcpyAsync(ctx->jpeg_host.p, a.seg_off + a.n_segments, sizeof(uint64_t), hipMemcpyDeviceToHost, ctx->stream));
    return SARPRO_HIP_OK;
}

// the file of a raster in device memory into the caller's host buffer: only the file crosses PCIe
int encode_to_host(sarpro_hip_ctx *ctx, const uint8_t *d_pixels, size_t cols, size_t rows, size_t pitch_bytes, int nc, unsigned R, uint8_t *out,
                   size_t cap, size_t *bytes_out) {
    const size_t dcap = std::min(cap, file_bound(cols, rows, nc, R));
    HIPCHK(ctx, hipSetDevice(ctx->device));
    HIPCHK(ctx, ctx->jpeg_file.reserve(std::max<size_t>(dcap, 1)));
    size_t hb = 0;
    RETCHK(encode_enqueue(ctx, d_pixels, cols, rows, pitch_bytes, nc, R, ctx->jpeg_file.as<uint8_t>(), dcap, &hb));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    const size_t total = hb + (size_t)*ctx->jpeg_host.as<uint64_t>();
    *bytes_out = total;
    if (std::min(total, dcap)) {
        HIPCHK(ctx, hipMemcpyAsync(out, ctx->jpeg_file.p, std::min(total, dcap), hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    }
    return total > cap ? fail(ctx, SARPRO_HIP_ERR_BUFFER_TOO_SMALL, "jpeg: the file does not fit the buffer (bytes_out has the size it needs)") : SARPRO_HIP_OK;
}

} // namespace

namespace sarpro {
int jpeg_encode_to_host(sarpro_hip_ctx *ctx, const uint8_t *d_pixels, size_t cols, size_t rows, size_t pitch_bytes, int components, unsigned restart_mcus,
                        uint8_t *out, size_t out_capacity, size_t *bytes_out) {
    if (!args_ok(cols, rows, components, restart_mcus)) return fail(ctx, SARPRO_HIP_ERR_INVALID_ARG, "jpeg: cols and rows 1..65535, components 1 or 3, restart interval 0..65535");
    return encode_to_host(ctx, d_pixels, cols, rows, pitch_bytes, components, restart_mcus ? restart_mcus : kJpegDefaultRestartMcus, out, out_capacity, bytes_out);
}
} // namespace sarpro

extern "C" int sarpro_hip_host_jpeg_header(size_t cols, size_t rows, int components, unsigned restart_mcus, uint8_t *out, size_t cap, size_t *bytes) {
    if (!args_ok(cols, rows, components, restart_mcus) || !bytes || (!out && cap)) return SARPRO_HIP_ERR_INVALID_ARG;
    const unsigned R = restart_mcus ? restart_mcus : kJpegDefaultRestartMcus;
    *bytes = write_header(cols, rows, components, R, out, cap);
    return *bytes > cap ? SARPRO_HIP_ERR_BUFFER_TOO_SMALL : SARPRO_HIP_OK;
}

extern "C" int sarpro_hip_jpeg_bound(size_t cols, size_t rows, int components, unsigned restart_mcus, size_t *bytes) {
    if (!args_ok(cols, rows, components, restart_mcus) || !bytes) return SARPRO_HIP_ERR_INVALID_ARG;
    *bytes = file_bound(cols, rows, components, restart_mcus ? restart_mcus : kJpegDefaultRestartMcus);
    return SARPRO_HIP_OK;
}

extern "C" int sarpro_hip_jpeg_encode_dev(sarpro_hip_ctx *ctx, const uint8_t *d_pixels, size_t cols, size_t rows, size_t pitch_bytes, int components,
                                          unsigned restart_mcus, uint8_t *d_out, size_t out_capacity, size_t *bytes_out) {
    if (!ctx) return SARPRO_HIP_ERR_INVALID_ARG;
    if (!args_ok(cols, rows, components, restart_mcus)) return fail(ctx, SARPRO_HIP_ERR_INVALID_ARG, "jpeg: cols and rows 1..65535, components 1 or 3, restart interval 0..65535");
    if (!d_pixels || !bytes_out || (!d_out && out_capacity)) return fail(ctx, SARPRO_HIP_ERR_INVALID_ARG, "null raster");
    if (pitch_bytes < cols * (size_t)components) return fail(ctx, SARPRO_HIP_ERR_INVALID_ARG, "pitch < row bytes");
    timing_reset(ctx);
    size_t hb = 0;
    RETCHK(encode_enqueue(ctx, d_pixels, cols, rows, pitch_bytes, components, restart_mcus ? restart_mcus : kJpegDefaultRestartMcus, d_out, out_capacity, &hb));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream)); // the one synchronisation of an image: it returns the byte count
    *bytes_out = hb + (size_t)*ctx->jpeg_host.as<uint64_t>();
    return *bytes_out > out_capacity ? fail(ctx, SARPRO_HIP_ERR_BUFFER_TOO_SMALL, "jpeg: the file does not fit the buffer (bytes_out has the size it needs)") : SARPRO_HIP_OK;
}

extern "C" int sarpro_hip_jpeg_encode(sarpro_hip_ctx *ctx, const uint8_t *pixels, size_t cols, size_t rows, size_t pitch_bytes, int components,
                                      unsigned restart_mcus, uint8_t *out, size_t out_capacity, size_t *bytes_out) {
    if (!ctx) return SARPRO_HIP_ERR_INVALID_ARG;
    if (!args_ok(cols, rows, components, restart_mcus)) return fail(ctx, SARPRO_HIP_ERR_INVALID_ARG, "jpeg: cols and rows 1..65535, components 1 or 3, restart interval 0..65535");
    if (!pixels || !bytes_out || (!out && out_capacity)) return fail(ctx, SARPRO_HIP_ERR_INVALID_ARG, "null raster");
    const size_t row_bytes = cols * (size_t)components;
    if (pitch_bytes < row_bytes) return fail(ctx, SARPRO_HIP_ERR_INVALID_ARG, "pitch < row bytes");
    timing_reset(ctx);
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const size_t dpitch = round_up(row_bytes, 64);
    HIPCHK(ctx, ctx->jpeg_rgb.reserve(rows * dpitch));
    HIPCHK(ctx, hipMemcpy2DAsync(ctx->jpeg_rgb.p, dpitch, pixels, pitch_bytes, row_bytes, rows, hipMemcpyHostToDevice, ctx->stream));
    return encode_to_host(ctx, ctx->jpeg_rgb.as<uint8_t>(), cols, rows, dpitch, components, restart_mcus ? restart_mcus : kJpegDefaultRestartMcus, out,
                          out_capacity, bytes_out);
}

// ---- save.rs:317-367 / api/mod.rs:404-437 up to the file: the bands are staged in device memory, the existing device-resident flow
// composes the RGB raster into a raster of the context, the encoder reads it there: the raster never leaves the device.
namespace {

int flow_dims(sarpro_hip_ctx *ctx, size_t rows, size_t cols, size_t target_size, int pad, unsigned restart_mcus, size_t *fc, size_t *fr) {
    RETCHK(sarpro_hip_resize_output_dims(cols, rows, target_size, pad, fc, fr));
    if (!args_ok(*fc, *fr, 3, restart_mcus)) return fail(ctx, SARPRO_HIP_ERR_INVALID_ARG, "jpeg: final cols and rows 1..65535, restart interval 0..65535");
    return SARPRO_HIP_OK;
}

int stage_band(sarpro_hip_ctx *ctx, int b, const void *host, size_t rows, size_t cols, size_t esz, size_t pitch) {
    HIPCHK(ctx, ctx->jpeg_band[b].reserve(rows * pitch * esz));
    HIPCHK(ctx, hipMemcpy2DAsync(ctx->jpeg_band[b].p, pitch * esz, host, cols * esz, cols * esz, rows, hipMemcpyHostToDevice, ctx->stream));
    return SARPRO_HIP_OK;
}

} // namespace

extern "C" int sarpro_hip_dualpol_synrgb_resized_u16_jpeg(sarpro_hip_ctx *ctx, const uint16_t *band1, const uint16_t *band2, size_t rows, size_t cols,
                                                          int strategy, int mode, size_t target_size, int pad, uint8_t *jpeg_out, size_t jpeg_capacity,
                                                          size_t *jpeg_bytes_out, unsigned restart_mcus, sarpro_hip_resize_meta *meta) {
    if (!ctx) return SARPRO_HIP_ERR_INVALID_ARG;
    if (!band1 || !band2 || !jpeg_bytes_out || (!jpeg_out && jpeg_capacity)) return fail(ctx, SARPRO_HIP_ERR_INVALID_ARG, "null raster");
    size_t fc = 0, fr = 0;
    RETCHK(flow_dims(ctx, rows, cols, target_size, pad, restart_mcus, &fc, &fr));
    TimingHold hold(ctx); // last_kernel_times: the flow's kernels and the encoder's
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const size_t pitch = round_up(cols, 64);
    RETCHK(stage_band(ctx, 0, band1, rows, cols, 2, pitch));
    RETCHK(stage_band(ctx, 1, band2, rows, cols, 2, pitch));
    HIPCHK(ctx, ctx->jpeg_rgb.reserve(fc * fr * 3));
    RETCHK(sarpro_hip_dualpol_synrgb_resized_u16_dev(ctx, ctx->jpeg_band[0].as<uint16_t>(), ctx->jpeg_band[1].as<uint16_t>(), rows, cols, pitch, strategy, mode,
                                                     target_size, pad, ctx->jpeg_rgb.as<uint8_t>(), meta));
    return encode_to_host(ctx, ctx->jpeg_rgb.as<uint8_t>(), fc, fr, fc * 3, 3, restart_mcus ? restart_mcus : kJpegDefaultRestartMcus, jpeg_out, jpeg_capacity,
                          jpeg_bytes_out);
}

extern "C" int sarpro_hip_dualpol_synrgb_resized_f32_jpeg(sarpro_hip_ctx *ctx, const float *band1, const float *band2, size_t rows, size_t cols, int strategy,
                                                          int mode, unsigned flags, size_t target_size, int pad, uint8_t *jpeg_out, size_t jpeg_capacity,
                                                          size_t *jpeg_bytes_out, unsigned restart_mcus, sarpro_hip_resize_meta *meta) {
    if (!ctx) return SARPRO_HIP_ERR_INVALID_ARG;
    if (!band1 || !band2 || !jpeg_bytes_out || (!jpeg_out && jpeg_capacity)) return fail(ctx, SARPRO_HIP_ERR_INVALID_ARG, "null raster");
    size_t fc = 0, fr = 0;
    RETCHK(flow_dims(ctx, rows, cols, target_size, pad, restart_mcus, &fc, &fr));
    TimingHold hold(ctx);
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const size_t pitch = round_up(cols, 64);
    RETCHK(stage_band(ctx, 0, band1, rows, cols, 4, pitch));
    RETCHK(stage_band(ctx, 1, band2, rows, cols, 4, pitch));
    HIPCHK(ctx, ctx->jpeg_rgb.reserve(fc * fr * 3));
    RETCHK(sarpro_hip_dualpol_synrgb_resized_f32_dev(ctx, ctx->jpeg_band[0].as<float>(), ctx->jpeg_band[1].as<float>(), rows, cols, pitch, strategy, mode, flags,
                                                     target_size, pad, ctx->jpeg_rgb.as<uint8_t>(), meta));
    return encode_to_host(ctx, ctx->jpeg_rgb.as<uint8_t>(), fc, fr, fc * 3, 3, restart_mcus ? restart_mcus : kJpegDefaultRestartMcus, jpeg_out, jpeg_capacity,
                          jpeg_bytes_out);
}
