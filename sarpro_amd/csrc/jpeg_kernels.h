// jpeg_kernels.h -- launch interface of the baseline JPEG encoder (jpeg_kernels.hip): quality 100, 4:4:4, Annex K tables,
// restart intervals (io/writers/jpeg.rs:14,27 -> jpeg_encoder::Encoder::new(w, 100)).
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

namespace sarpro {

// Huffman codes as the entropy kernel reads them: (length << 16) | code.  [0] luminance, [1] chrominance.
struct JpegCodeTables {
    uint32_t dc[2][16];
    uint32_t ac[2][256];
    uint8_t zz_pos[64]; // position in zigzag order of the coefficient at natural index (row * 8 + column)
};

struct JpegArgs {
    const uint8_t *pixels;   // interleaved RGB (components = 3) or a gray plane (1)
    size_t pitch_bytes;
    uint32_t cols, rows, components;
    uint32_t mcus_x, mcus_y; // 8 x 8 blocks per row / column (4:4:4: an MCU is one block of every component)
    uint32_t restart_mcus;   // R
    uint64_t n_mcus, n_segments;
    int16_t *coef;                // [n_mcus][components][64], zigzag order, quantised
    const JpegCodeTables *tables; // device
    uint32_t *seg_len;            // [n_segments] bytes of each restart segment: stuffing, padding and its RST marker (the last: EOI) included
    uint64_t *seg_off;            // [n_segments + 1] exclusive scan of seg_len; [n_segments] = the scan's length
    uint64_t *scan_sums;          // one partial sum per kJpegScanChunk segments
    uint8_t *out;                 // the file
    uint64_t out_capacity;        // nothing is written at or past this offset
    uint64_t header_bytes;        // the scan starts here
};
constexpr uint32_t kJpegScanChunk = 2048; // segment lengths one workgroup of the offset scan covers

// colour conversion -> edge replication -> level shift -> jfdctint rows, columns -> quantisation (divisor 8) -> zigzag
hipError_t launch_jpeg_transform(const JpegArgs &a, hipStream_t s);
// exact byte length of every restart segment
hipError_t launch_jpeg_entropy_size(const JpegArgs &a, hipStream_t s);
// seg_off = exclusive scan of seg_len (three launches)
hipError_t launch_jpeg_scan(const JpegArgs &a, hipStream_t s);
// every segment at its final offset, then EOI
hipError_t launch_jpeg_entropy_write(const JpegArgs &a, hipStream_t s);

} // namespace sarpro
