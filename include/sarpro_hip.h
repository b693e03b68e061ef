/*
 * sarpro_hip.h -- C ABI of libsarpro_hip.so: the MI355X (gfx950) replacement for
 * sarpro's per-pixel raster core (reference: bogwi/sarpro v0.3.0, src/core/processing).
 *
 * The reference has no FFI layer: its seam is ordinary Rust calls from save.rs /
 * api/mod.rs / io/sentinel1.rs into core::processing::{pipeline,autoscale,ops,
 * synthetic_rgb}.  Each entry point below names the Rust function it replaces
 * (file:line in the reference tree) -- a Rust `extern "C"` crate binding these
 * (rust/sarpro-hip-sys) gives save.rs the same call surface.
 *
 * Conventions
 *   - every call returns a status (0 = ok, <0 = error); message via sarpro_hip_last_error
 *   - rasters are row-major (rows, cols), the layout of ndarray::Array2 / GDAL read_as
 *     (io/gdal.rs:123-131); all sizes in ELEMENTS; outputs are caller-allocated
 *   - enum integers are the declaration order of src/types.rs
 *   - host entry points take HOST pointers (pageable or pinned) and are synchronous;
 *     `_dev` entry points take DEVICE pointers (+ pitch in elements) and run on the
 *     context's stream; they return after the result is complete on the device
 *   - STREAM ORDERING of `_dev` entry points: they run on the context's own hipStreamNonBlocking stream
 *     (sarpro_hip_ctx_stream), which is NOT ordered against any other stream, the NULL stream included.  The caller
 *     must order that stream behind the producers of its input rasters and behind earlier users of its output
 *     rasters -- hipStreamWaitEvent(sarpro_hip_ctx_stream(ctx), event recorded on the producer's stream), or a
 *     device / stream synchronisation before the call -- and order consumers behind the context's stream the same
 *     way unless the call was synchronous (every call is, except on a SARPRO_HIP_CTX_ASYNC_DEV context)
 *   - one context per host thread; contexts are independent (no global state)
 *   - nothing here falls back to a CPU implementation: without a usable HIP device
 *     ctx_create fails with SARPRO_HIP_ERR_NO_DEVICE
 *   - `sarpro_hip_host_*` functions are the host half of the path (statistics, LUT and
 *     CDF construction from device-produced histograms); they need no GPU and are
 *     exported so the multi-GPU driver and the tests can call them directly
 */
#ifndef SARPRO_HIP_H
#define SARPRO_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- status codes (reference: infallible fns; callers wrap panics/errors as
 *      Error::External / Error::Processing, src/error.rs:39-46) ---- */
#define SARPRO_HIP_OK 0
#define SARPRO_HIP_ERR_INVALID_ARG (-1)
#define SARPRO_HIP_ERR_SHAPE_MISMATCH (-2)
#define SARPRO_HIP_ERR_UNSUPPORTED_SHAPE (-3) /* CLAHE tile underflow sizes where the reference panics (autoscale.rs:250,254) */
#define SARPRO_HIP_ERR_HIP (-4)
#define SARPRO_HIP_ERR_RCCL (-5)
#define SARPRO_HIP_ERR_OOM (-6)
#define SARPRO_HIP_ERR_NO_DEVICE (-7)
#define SARPRO_HIP_ERR_IO (-8) /* a row reader / sink / TIFF file failed */
#define SARPRO_HIP_ERR_BUFFER_TOO_SMALL (-9) /* an output buffer's capacity: the call reports the size it needs */

/* ---- src/types.rs discriminants ---- */
typedef enum { /* types.rs:115-123 */
    SARPRO_STRATEGY_STANDARD = 0,
    SARPRO_STRATEGY_ROBUST = 1,
    SARPRO_STRATEGY_ADAPTIVE = 2,
    SARPRO_STRATEGY_EQUALIZED = 3,
    SARPRO_STRATEGY_CLAHE = 4,
    SARPRO_STRATEGY_TAMED = 5,
    SARPRO_STRATEGY_DEFAULT = 6
} sarpro_strategy;
typedef enum { SARPRO_BITDEPTH_U8 = 0, SARPRO_BITDEPTH_U16 = 1 } sarpro_bitdepth; /* types.rs:170-173 */
typedef enum { /* types.rs:8-14 */
    SARPRO_OP_SUM = 0,
    SARPRO_OP_DIFF = 1,
    SARPRO_OP_RATIO = 2,
    SARPRO_OP_NDIFF = 3,
    SARPRO_OP_LOGRATIO = 4
} sarpro_polop;
typedef enum { /* types.rs:177-182 */
    SARPRO_SYNRGB_DEFAULT = 0,
    SARPRO_SYNRGB_RGB_RATIO = 1,
    SARPRO_SYNRGB_SAR_URBAN = 2,
    SARPRO_SYNRGB_ENHANCED = 3
} sarpro_synrgb_mode;

/* HistogramStats (autoscale.rs:7-24) + the window the reference only logs
 * (autoscale.rs:398-401,431-434,485-488,566-569). */
typedef struct {
    uint64_t valid_count;
    double min_db, max_db, mean_db, std_db, median_db;
    double p01, p02, p05, p10, p25, p75, p90, p95, p98, p99;
    double low_clip, high_clip, gamma;
    double skew_factor, tail_heaviness; /* Adaptive only (autoscale.rs:503-504) */
} sarpro_hip_stats;

typedef struct sarpro_hip_ctx sarpro_hip_ctx;

/* ---- context ---- */
#define SARPRO_HIP_CTX_TIMING 1u    /* HIP-event pairs around the kernels (sarpro_hip_last_kernel_times) */
/* Stream-ordered device entry points: sarpro_hip_dualpol_synrgb_u16_dev called with u8 outputs, stats_out == NULL
 * and a scene the device-resident chain takes (16-byte aligned rasters, pitch % 8 == 0) returns once the chain is
 * ENQUEUED on the context's stream: the rasters are complete after sarpro_hip_ctx_synchronize (or after work the
 * caller orders behind sarpro_hip_ctx_stream).  Scenes enqueued back to back run back to back: the GPU does not
 * idle for the ~30 us a host round trip per scene costs.  Every other call stays synchronous.  The reference's
 * functions are synchronous: this is an opt-in for callers that keep rasters in HBM. */
#define SARPRO_HIP_CTX_ASYNC_DEV 2u
int sarpro_hip_ctx_create(int device, unsigned flags, sarpro_hip_ctx **ctx_out);
void sarpro_hip_ctx_destroy(sarpro_hip_ctx *ctx);
const char *sarpro_hip_last_error(const sarpro_hip_ctx *ctx); /* ctx may be NULL: last ctx_create error */
const char *sarpro_hip_version(void);
/* raw hipStream_t of the context (for callers that enqueue their own work / events) */
void *sarpro_hip_ctx_stream(sarpro_hip_ctx *ctx);
int sarpro_hip_ctx_synchronize(sarpro_hip_ctx *ctx);

/* ================= host-pointer entry points (the drop-in seam) ================= */

/* process_scalar_data_pipeline (pipeline.rs:42-67) for an f32 band as GDAL hands it over
 * (io/gdal.rs:123-131).  U8: fills out_u8 (out_u16 may be NULL); U16: fills out_u16.
 * The dB buffer / mask the reference also returns are not materialised (callers only
 * use their dims, save.rs:331; see sarpro_hip_db_mask_f32 for the buffers themselves).
 * stats_out may be NULL (the f32 flavour then skips the per-sample dB moments, which only the statistics and the
 * Adaptive strategy read). */
int sarpro_hip_autoscale_band_f32(sarpro_hip_ctx *ctx, const float *in, size_t rows, size_t cols,
                                  int strategy, int bit_depth, uint8_t *out_u8, uint16_t *out_u16,
                                  sarpro_hip_stats *stats_out);
/* Same function for the u16 DN samples of a full-resolution GRD read (io/gdal.rs:107-141
 * reads u16 as f32; values are integral), the fast flavour. */
int sarpro_hip_autoscale_band_u16(sarpro_hip_ctx *ctx, const uint16_t *in, size_t rows, size_t cols,
                                  int strategy, int bit_depth, uint8_t *out_u8, uint16_t *out_u16,
                                  sarpro_hip_stats *stats_out);

/* process_scalar_data_inplace (pipeline.rs:8-40): db = 10*log10(max(v,1e-10)) as f64,
 * mask = db > -50 (exact).  Either output may be NULL.  db is within 2 ulp(f64) of glibc's
 * value (so within 1 ulp when held as f32). */
int sarpro_hip_db_mask_f32(sarpro_hip_ctx *ctx, const float *in, size_t rows, size_t cols,
                           double *db_out, uint8_t *mask_out);

/* autoscale_db_image_tamed_synrgb_u8 (autoscale.rs:710-742); takes the band itself
 * (the dB buffer is recomputed on the device, never shipped). */
int sarpro_hip_tamed_synrgb_u8_f32(sarpro_hip_ctx *ctx, const float *in, size_t rows, size_t cols,
                                   int is_copol, uint8_t *out_u8);
int sarpro_hip_tamed_synrgb_u8_u16(sarpro_hip_ctx *ctx, const uint16_t *in, size_t rows, size_t cols,
                                   int is_copol, uint8_t *out_u8);

/* sum_arrays / difference_arrays / ratio_arrays / normalized_diff_arrays /
 * log_ratio_arrays (ops.rs:4-44). */
int sarpro_hip_polop_f32(sarpro_hip_ctx *ctx, int op, const float *a, const float *b, size_t n,
                         float *out);

/* Pol-op band straight to its autoscaled raster: sum / difference / ratio / normalized_diff / log_ratio_arrays
 * (ops.rs:4-44) followed by process_scalar_data_pipeline (pipeline.rs:42-67) on the result -- what
 * io/sentinel1.rs:1501-1578 + save.rs do for a `PolarOp` product -- with the operation computed in registers inside
 * every pass: the f32 pol-op raster is never written or read (12 B/px of traffic less than polop_f32 + autoscale_band_f32,
 * same raster bit for bit).  a, b: the two co-registered bands, as f32 or as the u16 DN of a full-resolution GRD read. */
int sarpro_hip_polop_autoscale_band_f32(sarpro_hip_ctx *ctx, int op, const float *a, const float *b, size_t rows, size_t cols,
                                        int strategy, int bit_depth, uint8_t *out_u8, uint16_t *out_u16,
                                        sarpro_hip_stats *stats_out);
int sarpro_hip_polop_autoscale_band_u16(sarpro_hip_ctx *ctx, int op, const uint16_t *a, const uint16_t *b, size_t rows, size_t cols,
                                        int strategy, int bit_depth, uint8_t *out_u8, uint16_t *out_u16,
                                        sarpro_hip_stats *stats_out);

/* create_synthetic_rgb_by_mode_and_strategy (synthetic_rgb.rs:182-197): interleaved RGB,
 * rgb_out holds 3*n bytes. */
int sarpro_hip_synrgb_u8(sarpro_hip_ctx *ctx, int mode, int strategy, const uint8_t *band1,
                         const uint8_t *band2, size_t n, uint8_t *rgb_out);

/* The JPEG/multiband branch of save_processed_multiband_image_sequential at native
 * resolution (save.rs:317-367): pipeline(band1,U8) -> [Tamed: tamed_synrgb(copol)] ->
 * pipeline(band2,U8) -> [Tamed: tamed_synrgb(cross-pol)] -> synRGB by strategy, fused on the
 * device.  rgb_out holds 3*rows*cols bytes; u8_band1/u8_band2 (optional) receive the
 * per-band u8 rasters that feed the composition; stats_out (optional) is [2]. */
int sarpro_hip_dualpol_synrgb_u16(sarpro_hip_ctx *ctx, const uint16_t *band1, const uint16_t *band2,
                                  size_t rows, size_t cols, int strategy, int mode,
                                  uint8_t *rgb_out, uint8_t *u8_band1, uint8_t *u8_band2,
                                  sarpro_hip_stats *stats_out);
int sarpro_hip_dualpol_synrgb_f32(sarpro_hip_ctx *ctx, const float *band1, const float *band2,
                                  size_t rows, size_t cols, int strategy, int mode,
                                  uint8_t *rgb_out, uint8_t *u8_band1, uint8_t *u8_band2,
                                  sarpro_hip_stats *stats_out);
/* f32 bands are what the reference's DEFAULT flow hands the raster core: `--size N` resamples on read (sentinel1.rs:1074-1108), so
 * the bands arrive as non-integer f32.  flags for the f32 dual-pol entry points below:
 *   SARPRO_HIP_DUALPOL_PLAIN_PIPELINE  api/mod.rs:404-437 (process_safe_to_buffer_with_mode): both bands go through
 *                                      process_scalar_data_pipeline with the caller's strategy; without it save.rs:324-351 applies:
 *                                      under Tamed the bands are re-autoscaled band-specifically (autoscale.rs:710-742). */
#define SARPRO_HIP_DUALPOL_PLAIN_PIPELINE 1u
/* save.rs:317-367 / api/mod.rs:404-437 with resize -> pad between the per-band autoscale and the composition, host f32 bands in,
 * final_rows * final_cols * 3 bytes out (sarpro_hip_resize_output_dims); the reference's order, so the suppressed floor sees the
 * padding.  The resize happens on the u8 level rasters, as in the reference. */
/* (declared with the resize entry points below: sarpro_hip_dualpol_synrgb_resized_f32 / _f32_dev) */

/* ================= resize + pad (first "next" row) ================= */
/* Bookkeeping the reference returns next to the raster (resize.rs:98-108). */
typedef struct {
    size_t final_cols, final_rows;
    double scale_x, scale_y;
    size_t pad_left, pad_top;
} sarpro_hip_resize_meta;
/* Output shape of resize_image_data_with_meta for (cols, rows, target_size (0 = None), pad):
 * calculate_resize_dimensions (resize.rs:6-30) + add_padding_to_square (padding.rs:12). */
int sarpro_hip_resize_output_dims(size_t cols, size_t rows, size_t target_size, int pad, size_t *final_cols,
                                  size_t *final_rows);
/* resize_image_data_with_meta (resize.rs:91-236): Lanczos3 resample to target_size on the long side
 * (skipped when already there), then optional centre zero-pad to a square.  bit_depth selects u8 / u16
 * elements.  `out` holds final_rows * final_cols elements.  Dimension and padding rules are exact; the
 * Lanczos3 arithmetic restates the fast_image_resize crate's convolution and its parity with the crate
 * is unpinned (crate source absent, version not locked). */
int sarpro_hip_resize_image_data(sarpro_hip_ctx *ctx, const void *data, size_t cols, size_t rows, size_t target_size,
                                 int bit_depth, int pad, void *out, sarpro_hip_resize_meta *meta);
int sarpro_hip_resize_image_data_dev(sarpro_hip_ctx *ctx, const void *d_data, size_t cols, size_t rows, size_t pitch,
                                     size_t target_size, int bit_depth, int pad, void *d_out, size_t out_pitch,
                                     sarpro_hip_resize_meta *meta);
/* The JPEG/multiband branch with its resize and pad steps (save.rs:317-367): per-band u8 autoscale at
 * native resolution -> resize -> pad -> synRGB, all on the device; only the final RGB
 * (final_rows * final_cols * 3 bytes, see sarpro_hip_resize_output_dims) crosses PCIe. */
int sarpro_hip_dualpol_synrgb_resized_u16(sarpro_hip_ctx *ctx, const uint16_t *band1, const uint16_t *band2, size_t rows,
                                          size_t cols, int strategy, int mode, size_t target_size, int pad,
                                          uint8_t *rgb_out, sarpro_hip_resize_meta *meta);
int sarpro_hip_dualpol_synrgb_resized_f32(sarpro_hip_ctx *ctx, const float *band1, const float *band2, size_t rows, size_t cols,
                                          int strategy, int mode, unsigned flags, size_t target_size, int pad, uint8_t *rgb_out,
                                          sarpro_hip_resize_meta *meta);
int sarpro_hip_dualpol_synrgb_resized_f32_dev(sarpro_hip_ctx *ctx, const float *d_band1, const float *d_band2, size_t rows, size_t cols,
                                              size_t in_pitch, int strategy, int mode, unsigned flags, size_t target_size, int pad,
                                              uint8_t *d_rgb_out, sarpro_hip_resize_meta *meta);
/* The same product with both bands and the RGB raster (final_rows * final_cols * 3 bytes, compact) resident in device memory:
 * nothing crosses PCIe.  in_pitch in elements.  Synchronous. */
int sarpro_hip_dualpol_synrgb_resized_u16_dev(sarpro_hip_ctx *ctx, const uint16_t *d_band1, const uint16_t *d_band2, size_t rows,
                                              size_t cols, size_t in_pitch, int strategy, int mode, size_t target_size, int pad,
                                              uint8_t *d_rgb_out, sarpro_hip_resize_meta *meta);

/* ================= JPEG encoding (io/writers/jpeg.rs:14,27 write_rgb_jpeg / write_gray_jpeg) =================
 * What the reference's JPEG branches end in (save.rs:317-403, api/mod.rs:404-437): jpeg_encoder::Encoder::new(w, 100).  Baseline
 * sequential JPEG, quality 100 (not a parameter: every quantisation entry is 1), all sampling factors 1x1 (the crate's choice for
 * quality >= 90), the Annex K Huffman tables (not optimised), components = 1 (gray) or 3 (RGB -> YCbCr).  The arithmetic is libjpeg's:
 * jccolor with 16 fractional bits, edge blocks replicating the last column and row, jfdctint ("islow"), divisor 8, jchuff's coding.
 * The scan carries restart intervals (a DRI segment with the interval, RST0..7 markers): the segments are independent, which is what
 * the device parallelises over; any decoder reads such a file.  restart_mcus = 0 picks the library's interval (DESIGN.md "JPEG
 * encoding"), 1..65535 are taken as given.  cols and rows must be 1..65535 (the reference's `as u16` cast truncates silently: refused
 * here), components 1 or 3: SARPRO_HIP_ERR_INVALID_ARG otherwise.  File layout: SOI, APP0 JFIF 1.01, DQT, SOF0, DHT, DRI, SOS, scan,
 * EOI.  The scan is checked byte for byte against libjpeg-turbo; parity with the jpeg-encoder crate itself is unpinned (crate source
 * absent, version not locked): it is documented as a port of the same libjpeg jfdctint and colour arithmetic. */
/* Everything up to and including the SOS header (no GPU): *bytes = its length; SARPRO_HIP_ERR_BUFFER_TOO_SMALL when cap is less. */
int sarpro_hip_host_jpeg_header(size_t cols, size_t rows, int components, unsigned restart_mcus, uint8_t *out, size_t cap, size_t *bytes);
/* A capacity no file of this shape can exceed (no GPU): the longest codes of the four tables, the category limits of 8-bit input,
 * every byte stuffed.  Far above real files (about 6.5 bytes per sample): a caller may offer less and retry with the size the
 * encoder reports. */
int sarpro_hip_jpeg_bound(size_t cols, size_t rows, int components, unsigned restart_mcus, size_t *bytes);
/* The raster (pitch_bytes per row: interleaved RGB or a gray plane) and the file both in device memory.  Synchronous: one
 * synchronisation, the one that returns *bytes_out.  When the file does not fit, nothing at or past out_capacity is written, *bytes_out
 * is the size it needs and the status is SARPRO_HIP_ERR_BUFFER_TOO_SMALL.  Kernel times: jpeg_transform, jpeg_entropy_size, jpeg_scan,
 * jpeg_entropy_write. */
int sarpro_hip_jpeg_encode_dev(sarpro_hip_ctx *ctx, const uint8_t *d_pixels, size_t cols, size_t rows, size_t pitch_bytes, int components,
                               unsigned restart_mcus, uint8_t *d_out, size_t out_capacity, size_t *bytes_out);
/* The raster and the file both in host memory: the raster goes up, only the file comes back. */
int sarpro_hip_jpeg_encode(sarpro_hip_ctx *ctx, const uint8_t *pixels, size_t cols, size_t rows, size_t pitch_bytes, int components,
                           unsigned restart_mcus, uint8_t *out, size_t out_capacity, size_t *bytes_out);
/* sarpro_hip_dualpol_synrgb_resized_u16 / _f32 up to the FILE the reference writes: the device-resident flow composes the RGB raster
 * into a raster of the context and the encoder reads it there; the raster never leaves the device, only the file crosses PCIe. */
int sarpro_hip_dualpol_synrgb_resized_u16_jpeg(sarpro_hip_ctx *ctx, const uint16_t *band1, const uint16_t *band2, size_t rows, size_t cols,
                                               int strategy, int mode, size_t target_size, int pad, uint8_t *jpeg_out, size_t jpeg_capacity,
                                               size_t *jpeg_bytes_out, unsigned restart_mcus, sarpro_hip_resize_meta *meta);
int sarpro_hip_dualpol_synrgb_resized_f32_jpeg(sarpro_hip_ctx *ctx, const float *band1, const float *band2, size_t rows, size_t cols, int strategy,
                                               int mode, unsigned flags, size_t target_size, int pad, uint8_t *jpeg_out, size_t jpeg_capacity,
                                               size_t *jpeg_bytes_out, unsigned restart_mcus, sarpro_hip_resize_meta *meta);

/* save_processed_image (save.rs:23-170) up to the raster its writer receives: pipeline at native
 * resolution -> resize -> pad, on the device.  `out` holds final_rows * final_cols u8 / u16 elements.
 * The multiband TIFF branch (save.rs:200-316) is this call once per band. */
int sarpro_hip_process_band_resized_u16(sarpro_hip_ctx *ctx, const uint16_t *in, size_t rows, size_t cols, int strategy,
                                        int bit_depth, size_t target_size, int pad, void *out,
                                        sarpro_hip_resize_meta *meta);
int sarpro_hip_process_band_resized_f32(sarpro_hip_ctx *ctx, const float *in, size_t rows, size_t cols, int strategy,
                                        int bit_depth, size_t target_size, int pad, void *out,
                                        sarpro_hip_resize_meta *meta);

/* Batch mode (api/mod.rs:474-536 process_directory_to_path; BatchReport :453-458) for scenes already
 * decoded into host memory: workers_per_device worker threads (each with a context of its own) per listed
 * device, scenes dealt dynamically, no collective.  workers_per_device = 0 picks the default, 2: a scene's
 * call is upload -> chain -> download, one PCIe direction at a time; with two workers on a device scene i's
 * D2H crosses the full-duplex link beside scene i + 1's H2D (50.2 -> 31.8 ms per 400 MP scene, bench.py
 * `secondary.e2e_two_in_flight`).  continue_on_error = 0 stops handing out scenes after the first failure
 * (the rest count as skipped) and returns that failure's status. */
/* row-chunk callbacks of the streaming entry points (described with sarpro_hip_dualpol_synrgb_stream_u16 below) */
typedef int (*sarpro_hip_row_reader)(void *user, int band, size_t row0, size_t nrows, uint16_t *dst, size_t dst_pitch);
typedef int (*sarpro_hip_row_sink)(void *user, size_t row0, size_t nrows, const uint8_t *src, size_t src_pitch_bytes);
typedef struct {
    const uint16_t *band1, *band2; /* rows x cols each; ignored when `reader` is set */
    size_t rows, cols;
    uint8_t *rgb_out;              /* final_rows * final_cols * 3 (sarpro_hip_resize_output_dims) */
    int *status_out;               /* optional per-scene status */
    sarpro_hip_row_reader reader;  /* optional: the scene's bands come through this row reader (a batch of SAFE scenes
                                      does not fit host memory as arrays: api/mod.rs:484-533 opens them one by one) */
    void *reader_user;
} sarpro_hip_batch_scene;
typedef struct { size_t processed, skipped, errors; } sarpro_hip_batch_report;
int sarpro_hip_batch_dualpol_synrgb_resized_u16(const int *devices, int ndevices, int workers_per_device, const sarpro_hip_batch_scene *scenes,
                                                size_t nscenes, int strategy, int mode, size_t target_size, int pad,
                                                int continue_on_error, sarpro_hip_batch_report *report);

/* f32 bands (the reference's default, resampled-on-read flow); flags: SARPRO_HIP_DUALPOL_* */
typedef struct {
    const float *band1, *band2; /* rows x cols each */
    size_t rows, cols;
    uint8_t *rgb_out;           /* final_rows * final_cols * 3 */
    int *status_out;            /* optional per-scene status */
} sarpro_hip_batch_scene_f32;
int sarpro_hip_batch_dualpol_synrgb_resized_f32(const int *devices, int ndevices, int workers_per_device, const sarpro_hip_batch_scene_f32 *scenes,
                                                size_t nscenes, int strategy, int mode, unsigned flags, size_t target_size, int pad,
                                                int continue_on_error, sarpro_hip_batch_report *report);

/* Resident batch: the batch loop of api/mod.rs:484-533 for scenes whose bands are ALREADY in device memory (decoded and uploaded by
 * the caller, or produced on the device), all of one shape -- the save.rs:317-367 product at native resolution per scene:
 * d_band1, d_band2 -> per-band autoscale -> synRGB -> d_rgb (rgb_pitch_px pixels per row).  One context, `lanes` internal lanes (each
 * its own stream and workspace set, created on first use; 0 = the library's default): scene i runs on lane i mod lanes, so scene
 * i + 1's histogram sweep and its short dependent kernels (statistics, CLAHE bins, CDFs, sample, prediction) are enqueued beside
 * scene i's CLAHE -> RGB pass instead of behind it.  Every scene takes the route it would take alone (speculative, refuted or
 * unproven -> exact kernels): the rasters are those of sarpro_hip_dualpol_synrgb_u16_dev, bit for bit.  The call returns when every
 * raster is complete.  status / route are written per scene (route: SARPRO_HIP_ROUTE_*; -1 when no speculative chain ran for it);
 * continue_on_error = 0 stops enqueuing after the first failure (the rest count as skipped), as the other batch entry points.
 * Stream ordering: the lanes' streams are ordered against nothing of the caller's -- inputs must be complete before the call. */
#define SARPRO_HIP_ROUTE_NONE (-1)      /* no speculative CLAHE chain ran (another strategy, a small or unaligned scene) */
#define SARPRO_HIP_ROUTE_ACCEPTED 0     /* the fused CLAHE -> RGB pass's raster stood */
#define SARPRO_HIP_ROUTE_REFUTED 1      /* the predicted floor / rescale range was refuted in the pass: exact kernels produced the raster */
#define SARPRO_HIP_ROUTE_UNPROVEN 2     /* the speculation never started */
#define SARPRO_HIP_ROUTE_POOL_OVERFLOW 3 /* DN windows beyond the fused pass's LDS pool: exact kernels */
#define SARPRO_HIP_ROUTE_RETRIED 4      /* the first floor was refuted, a second fused pass with the floor its counts point to stood */
typedef struct {
    const uint16_t *d_band1, *d_band2; /* device, rows x in_pitch */
    uint8_t *d_rgb;                    /* device, rows x rgb_pitch_px x 3 */
    int status;                        /* out */
    int route;                         /* out */
} sarpro_hip_resident_scene;
int sarpro_hip_batch_dualpol_synrgb_u16_dev(sarpro_hip_ctx *ctx, sarpro_hip_resident_scene *scenes, size_t nscenes, size_t rows,
                                            size_t cols, size_t in_pitch, int strategy, int mode, size_t rgb_pitch_px, int lanes,
                                            int continue_on_error, sarpro_hip_batch_report *report);

/* The resident batch for f32 bands -- the reference's default flow (api/mod.rs:374-449: bands resampled on read, a few megapixels) looped
 * over the scenes of a directory (api/mod.rs:474-536), for bands that are already in device memory: per scene
 * sarpro_hip_dualpol_synrgb_resized_f32_dev (flags: SARPRO_HIP_DUALPOL_*; d_rgb: final_rows * final_cols * 3 bytes, compact), on one of
 * `lanes` internal lanes of the context (0 = the default), each driven by a host thread of its own for the duration of the call: at this
 * size the chain is bound by its host turns, which now overlap.  The rasters are the single call's, bit for bit.  BatchReport semantics
 * as the other batch entry points; the call returns when every raster is complete. */
typedef struct {
    const float *d_band1, *d_band2;    /* device, rows x in_pitch */
    uint8_t *d_rgb;                    /* device, final_rows x final_cols x 3 */
    int status;                        /* out */
} sarpro_hip_resident_scene_f32;
int sarpro_hip_batch_dualpol_synrgb_resized_f32_dev(sarpro_hip_ctx *ctx, sarpro_hip_resident_scene_f32 *scenes, size_t nscenes, size_t rows, size_t cols,
                                                    size_t in_pitch, int strategy, int mode, unsigned flags, size_t target_size, int pad, int lanes,
                                                    int continue_on_error, sarpro_hip_batch_report *report);

/* ================= device-pointer entry points ================= */
/* Same operations on rasters already resident in HBM.  pitch = row stride in elements
 * (>= cols).  The vectorised kernels need base pointers aligned to 16 bytes and
 * pitch % 8 == 0; other layouts take the scalar kernels (same results). */
int sarpro_hip_autoscale_band_u16_dev(sarpro_hip_ctx *ctx, const uint16_t *d_in, size_t rows,
                                      size_t cols, size_t in_pitch, int strategy, int bit_depth,
                                      void *d_out, size_t out_pitch, sarpro_hip_stats *stats_out);
int sarpro_hip_autoscale_band_f32_dev(sarpro_hip_ctx *ctx, const float *d_in, size_t rows,
                                      size_t cols, size_t in_pitch, int strategy, int bit_depth,
                                      void *d_out, size_t out_pitch, sarpro_hip_stats *stats_out);
/* f32 bands resident in device memory (pitches in elements / pixels); flags: SARPRO_HIP_DUALPOL_*.  Synchronous. */
int sarpro_hip_dualpol_synrgb_f32_dev(sarpro_hip_ctx *ctx, const float *d_band1, const float *d_band2, size_t rows, size_t cols,
                                      size_t in_pitch, int strategy, int mode, unsigned flags, uint8_t *d_rgb, size_t rgb_pitch_px,
                                      uint8_t *d_u8_band1, uint8_t *d_u8_band2, size_t u8_pitch, sarpro_hip_stats *stats_out);
int sarpro_hip_dualpol_synrgb_u16_dev(sarpro_hip_ctx *ctx, const uint16_t *d_band1,
                                      const uint16_t *d_band2, size_t rows, size_t cols,
                                      size_t in_pitch, int strategy, int mode, uint8_t *d_rgb,
                                      size_t rgb_pitch_px, uint8_t *d_u8_band1, uint8_t *d_u8_band2,
                                      size_t u8_pitch, sarpro_hip_stats *stats_out);
/* device-pointer forms of sarpro_hip_polop_autoscale_band_*: in_pitch (elements) is shared by d_a and d_b; d_out is u8 or
 * u16 by bit_depth, out_pitch in elements */
int sarpro_hip_polop_autoscale_band_f32_dev(sarpro_hip_ctx *ctx, int op, const float *d_a, const float *d_b, size_t rows, size_t cols,
                                            size_t in_pitch, int strategy, int bit_depth, void *d_out, size_t out_pitch,
                                            sarpro_hip_stats *stats_out);
int sarpro_hip_polop_autoscale_band_u16_dev(sarpro_hip_ctx *ctx, int op, const uint16_t *d_a, const uint16_t *d_b, size_t rows, size_t cols,
                                            size_t in_pitch, int strategy, int bit_depth, void *d_out, size_t out_pitch,
                                            sarpro_hip_stats *stats_out);
int sarpro_hip_polop_f32_dev(sarpro_hip_ctx *ctx, int op, const float *d_a, const float *d_b,
                             size_t n, float *d_out);
int sarpro_hip_synrgb_u8_dev(sarpro_hip_ctx *ctx, int mode, int strategy, const uint8_t *d_band1,
                             const uint8_t *d_band2, size_t n, uint8_t *d_rgb);

/* ---- per-kernel timing of the last *_dev / host call on this context (HIP events on the
 * context's stream).  names_out receives up to max_entries pointers to static strings. */
int sarpro_hip_last_kernel_times(sarpro_hip_ctx *ctx, const char **names_out, float *ms_out,
                                 int max_entries);
/* Restrict the event pairs to the kernel of this name (as reported by sarpro_hip_last_kernel_times); NULL or ""
 * = every kernel.  An event pair costs the stream about 10 us of idle time between two kernels: a chain of a
 * dozen kernels timed one by one runs ~6 % slower than untimed, timed on its dominant kernel only ~0.5 %. */
int sarpro_hip_ctx_time_only(sarpro_hip_ctx *ctx, const char *kernel_name);

/* ---- context attributes: the route switches.  Every fast route of the library has a slower twin that must give the same raster
 * ("Cross-check switches"), plus a few test hooks and planner tuning values.  They live on the CONTEXT: each
 * attribute NAME (e.g. "NO_SPEC", "SAMPLE_STRIDE"; an optional "SARPRO_HIP_" prefix is accepted) is either unset (the default
 * behaviour) or set to an integer; a switch is on when set and non-zero.  The environment variable SARPRO_HIP_<NAME> is read ONCE,
 * when the context is created, as the attribute's initial value (a non-numeric word counts as 1; SPEC_FORCE takes
 * "mispredict" = 1 and / or "nospec" = 2, F32_ZONES takes "tiny" = 2); no call path reads the environment afterwards.  A context's
 * twin (the second band of a dual-pol f32 product) follows its parent.  Planner attributes (STRIP_ALIGN, CHUNK_ROWS, ...) act when a
 * shape's plan is first built.  sarpro_hip_attr_name(i) enumerates the names (NULL past the last). */
int sarpro_hip_ctx_set_attr(sarpro_hip_ctx *ctx, const char *name, int64_t value);
int sarpro_hip_ctx_reset_attr(sarpro_hip_ctx *ctx, const char *name); /* back to "unset" */
int sarpro_hip_ctx_get_attr(const sarpro_hip_ctx *ctx, const char *name, int64_t *value, int *is_set);
const char *sarpro_hip_attr_name(int index);

/* Diagnostics of the last speculative CLAHE chain of this context.  A whole dual-pol u8 scene (>= 32 MP) counts its level
 * histogram on sampled rows only; from the sample the chain PROVES that the u8 rescale of autoscale.rs:348-364 is the
 * identity (levels 0 and 255 occur) and PREDICTS the suppressed-synRGB floor (synthetic_rgb.rs:99-113), composes with the
 * prediction, and verifies it exactly inside the compose pass (csrc/chain_kernels.hip, k_chain_predict).  Synchronises the
 * context's stream.  spec_ok: 1 = the proof held and the speculative composition ran; 2 = a band holds no level 0 (a crop
 * without invalid pixels), its lowest level min_pred is a PREDICTION too, the rescale (min_pred, 255) is folded into the tables and
 * the fused pass counts the level bytes below min_pred (n_below_min: any refutes); 0 = no speculation.  verdict 0: the speculative
 * RGB stood, 1: refuted (or never ran) and the exact recount + composition ran; the raster is the reference's either way.
 * A refuted FLOOR gets one second fused pass first (retried = 1): the pass's counts say on which side of the prediction the floor lies. */
typedef struct {
    uint32_t spec_ok, verdict;
    int32_t floor_pred;       /* predicted floor before the +3 cushion; 37 stands for "37 or more" (the cushion caps at 40) */
    uint32_t pool_overflow;   /* 1: spec_ok, but the fused CLAHE -> RGB pass stepped aside (the bands' DN windows exceed its LDS pool): verdict 1 */
    uint64_t n_lt[2];         /* band-pixels with level < floor_pred, < floor_pred + 1 (exact, counted by the compose pass) */
    uint64_t target;          /* synthetic_rgb.rs:99-100 */
    double est_lt[2];         /* the sample's estimate of n_lt */
    uint64_t sample_valid[2]; /* per band: valid pixels on the sampled rows, each work item weighted by rows / sampled rows, 4096 = 1.0 */
    uint64_t n_below_min;     /* spec_ok 2: band-pixels whose level lies below their band's min_pred (exact; 0 or refuted) */
    uint32_t min_pred[2];     /* spec_ok 2: predicted lowest level per band (0: proven) */
    uint32_t retried;         /* 1: the first floor was refuted and a second fused pass ran with the floor the counts pointed to (floor_pred is that floor, verdict its verdict) */
    int32_t floor_first;      /* the floor the first pass tried */
} sarpro_hip_spec_report;
int sarpro_hip_ctx_spec_report(sarpro_hip_ctx *ctx, sarpro_hip_spec_report *out);

/* Diagnostics of the last device-resident CLAHE chain of this context (u16 flavour): what stood between the CLAHE levels and the
 * composition.  rescale[b]: the u8 rescale of band b's levels (autoscale.rs:348-364) as a table; floor_with_cushion: synthetic_rgb.rs:
 * 110-113 (-1: none, no synRGB was composed); level_hist[b]: the exact level histogram the exact kernels built them from (bin 0 implied:
 * pixels - sum of the others) -- all zero when the speculative composition stood (nothing was recounted).  Synchronises the stream. */
typedef struct {
    int32_t floor_with_cushion;
    uint8_t identity[2];      /* 1: band b's rescale is the identity on the levels that occur */
    uint8_t reserved[2];
    uint8_t rescale[512];     /* [band][256] */
    uint64_t level_hist[512]; /* [band][256] */
} sarpro_hip_chain_report;
int sarpro_hip_ctx_chain_report(sarpro_hip_ctx *ctx, sarpro_hip_chain_report *out);

/* ================= row-stripe (multi-GPU) protocol ================= */
/* One scene split into row stripes, one per rank.  Each phase
 * ends in a small integer reduction that the caller merges across ranks (RCCL
 * all-reduce(sum) on the returned DEVICE buffers, or sarpro_hip_comm_* below), so the
 * N-rank result is bit-identical to the 1-rank result.  A phase returns with its buffer
 * complete; the caller's reduction must be complete before it calls the next phase. */
typedef struct sarpro_hip_stripe sarpro_hip_stripe;
/* rows_total x cols scene; this rank owns rows [row0, row0+rows_local).  d_band1/2 are the
 * local stripe (rows_local x cols, pitch in elements). */
int sarpro_hip_stripe_begin_u16(sarpro_hip_ctx *ctx, const uint16_t *d_band1, const uint16_t *d_band2,
                                size_t rows_total, size_t cols, size_t row0, size_t rows_local,
                                size_t in_pitch, int strategy, int mode, sarpro_hip_stripe **out);
/* phase 1: local DN histograms.  *d_buf: device u64 buffer to all-reduce(sum), *count its length. */
int sarpro_hip_stripe_phase1(sarpro_hip_stripe *s, uint64_t **d_buf, size_t *count);
/* phase 2 (CLAHE only; no-op otherwise): local per-tile bin histograms -> all-reduce(sum). */
int sarpro_hip_stripe_phase2(sarpro_hip_stripe *s, uint64_t **d_buf, size_t *count);
/* phase 3: apply; local histogram of the pre-rescale u8 levels -> all-reduce(sum). */
int sarpro_hip_stripe_phase3(sarpro_hip_stripe *s, uint64_t **d_buf, size_t *count);
/* phase 4: compose the local stripe of the RGB raster (rows_local x cols x 3). */
int sarpro_hip_stripe_phase4(sarpro_hip_stripe *s, uint8_t *d_rgb, size_t rgb_pitch_px,
                             sarpro_hip_stats *stats_out);
void sarpro_hip_stripe_end(sarpro_hip_stripe *s);

/* ================= streaming ingest / egress (north-star: "staged to device via pinned
 * hipMemcpyAsync overlapped on a side stream") =================
 * The caller keeps its decoder (GDAL RasterIO, the strip-TIFF reader below, a socket ...): `reader` fills `nrows`
 * rows of band 0 or 1 starting at `row0` into a PINNED buffer of the library (`dst_pitch` elements per row);
 * `sink` receives finished interleaved RGB rows (`src_pitch_bytes` per row, cols * 3 valid).  Both return 0 or an
 * error code of their own, which aborts the call with SARPRO_HIP_ERR_IO.  While the reader produces chunk k + 1,
 * chunk k crosses PCIe on a side stream and the DN-histogram work items of the rows that have arrived run on the
 * compute stream; the RGB leaves chunk by chunk the same way.  Replaces the read loop + processing + write of
 * save_processed_multiband_image_sequential's JPEG branch at native resolution (save.rs:317-367, io/gdal.rs:107-141).
 * chunk_rows = 0 picks ~32 MiB chunks. */
int sarpro_hip_dualpol_synrgb_stream_u16(sarpro_hip_ctx *ctx, sarpro_hip_row_reader reader, void *reader_user, size_t rows,
                                         size_t cols, int strategy, int mode, size_t chunk_rows, sarpro_hip_row_sink sink,
                                         void *sink_user, sarpro_hip_stats *stats_out);

/* save.rs:317-367 with its resize / pad (sarpro_hip_dualpol_synrgb_resized_u16) fed by the row reader: the product is
 * small (target_size^2 x 3 bytes), so it is returned in one piece. */
int sarpro_hip_dualpol_synrgb_resized_stream_u16(sarpro_hip_ctx *ctx, sarpro_hip_row_reader reader, void *reader_user, size_t rows,
                                                 size_t cols, int strategy, int mode, size_t target_size, int pad, uint8_t *rgb_out,
                                                 sarpro_hip_resize_meta *meta);

/* ================= downsample on read (io/sentinel1.rs:1074-1108 -> io/gdal.rs:145-177) =================
 * The reference's default flow does not process full-resolution bands: SafeReader::open_with_options(.., target_size) has GDAL
 * resample each band while reading it (read_band_resampled), the long side going to target_size, and the raster core sees the
 * resulting few-MP non-integer f32 bands.  The filter is ResampleAlg::Average when the reduction is >= 4 (every GRD quicklook) and
 * Lanczos below (sentinel1.rs:1093-1102).  This section is that step for u16 bands, on the device: the Average filter, and the
 * Lanczos filter for per-axis ratios up to 5 (further down).
 *   shape   scale = min(ts / max(cols, rows), 1) in f64; out = max(round(n * scale), 1) per axis, round half away from zero.
 *   filter  the separable weighted box: per axis, destination sample j of m covers [j * r, min((j + 1) * r, n)) with r = n / m;
 *           a source sample weighs its overlap with that interval (1 for every interior sample).  Per destination pixel, for each
 *           source row of the window top to bottom: the EXACT integer sum of the interior columns plus the two edge samples times
 *           their weights (f64), times the row's weight, added to the running f64 sum; one correctly rounded division by
 *           w_sum_x * w_sum_y; one rounding to f32.  DESIGN.md 9b states it operation by operation; tests/readref.py is its
 *           restatement.  The results are a function of the definition alone (bit for bit, whatever the tiling or pitch).
 * Parity with GDAL's own Average is UNPINNED: GDAL is absent here and the reference does not lock its version; this is the weighted
 * box GDAL's average resampler documents, in its working precision for a Float32 buffer.  Lanczos on read (reductions below 4) is
 * the section's second filter, below; the flows take it only on a context whose READ_LANCZOS attribute is on and return
 * SARPRO_HIP_ERR_UNSUPPORTED otherwise. */
#define SARPRO_HIP_ERR_UNSUPPORTED (-10) /* a documented combination that is not built or not switched on (Lanczos on read) */
typedef enum {
    SARPRO_READ_DEFAULT = -1, /* the rule of sentinel1.rs:1093-1102 */
    SARPRO_READ_AVERAGE = 0,
    SARPRO_READ_LANCZOS = 1
} sarpro_hip_read_alg;
/* sentinel1.rs:1084-1102 (no GPU): the shape a band of cols x rows is read at, and the filter the rule picks for it (*alg =
 * SARPRO_READ_AVERAGE iff max(cols, rows) / target_size >= 4).  cols, rows or target_size = 0, a null pointer: INVALID_ARG. */
int sarpro_hip_read_output_dims(size_t cols, size_t rows, size_t target_size, size_t *out_cols, size_t *out_rows, int *alg);
/* One axis of the Average filter (no GPU): for each of the n_dst destination samples its window [first, first + count) of the n_src
 * source samples, the weights of the window's first and last sample (a one-sample window: w_first alone, w_last = 0) and the window's
 * total weight.  1 <= n_dst <= n_src <= 2^30; arrays of n_dst entries. */
int sarpro_hip_host_read_average_axis(size_t n_src, size_t n_dst, uint32_t first[], uint32_t count[], double w_first[], double w_last[],
                                      double w_sum[]);
/* The Average filter: rows x cols u16 (in_pitch elements per row) -> out_rows x out_cols f32 (out_pitch elements per row), both in
 * device memory; 1 <= out_rows <= rows, 1 <= out_cols <= cols (a ratio of 1 is the plain u16 -> f32 cast).  Stream-ordered on the
 * context's stream and synchronous like the other _dev calls (on a SARPRO_HIP_CTX_ASYNC_DEV context it returns once enqueued).
 * 16-byte loads when in_pitch % 8 == 0 and d_in is 16-byte aligned (the raster is rows x in_pitch elements, as everywhere in this
 * header: the last vector of a row may reach into the row's padding, whose values are never used), element loads otherwise: the same
 * results.  Kernel time: read_average. */
int sarpro_hip_read_average_u16_dev(sarpro_hip_ctx *ctx, const uint16_t *d_in, size_t rows, size_t cols, size_t in_pitch, size_t out_rows,
                                    size_t out_cols, float *d_out_f32, size_t out_pitch);
/* The same with host pointers (compact rasters): the band goes up, the averaged raster comes back. */
int sarpro_hip_read_average_u16(sarpro_hip_ctx *ctx, const uint16_t *in, size_t rows, size_t cols, size_t out_rows, size_t out_cols,
                                float *out_f32);
/* "Two measurement bands in, quicklook RGB out, as --size N does it": the shape of sarpro_hip_read_output_dims, both bands averaged
 * (one launch) into f32 rasters of the context, then sarpro_hip_dualpol_synrgb_resized_f32_dev on them with the caller's flags
 * (SARPRO_HIP_DUALPOL_PLAIN_PIPELINE or 0).  The bands arrive at target_size already, so the resize step takes its early-out and
 * only the pad remains, as in the reference.  d_rgb_out: final_rows * final_cols * 3 bytes, where (final_cols, final_rows) =
 * sarpro_hip_resize_output_dims(out_cols, out_rows, target_size, pad).  alg: SARPRO_READ_DEFAULT follows the rule; an explicit
 * SARPRO_READ_AVERAGE is honoured at any reduction >= 1; Lanczos, chosen by the rule or requested, returns
 * SARPRO_HIP_ERR_UNSUPPORTED with a message naming the reduction (nothing is written) -- UNLESS the context attribute READ_LANCZOS
 * is on (sarpro_hip_ctx_set_attr(ctx, "READ_LANCZOS", 1), or SARPRO_HIP_READ_LANCZOS in the environment when the context is created).
 * Then, in all four flows of this section: SARPRO_READ_DEFAULT follows the rule to either filter (every shape the rule sends to
 * Lanczos has per-axis ratios <= 5); an explicit SARPRO_READ_LANCZOS is honoured wherever both per-axis ratios are <= 5 and returns
 * SARPRO_HIP_ERR_UNSUPPORTED with a message naming the ratios beyond; SARPRO_READ_AVERAGE is unchanged.  The filtered f32 bands go to
 * sarpro_hip_dualpol_synrgb_resized_f32_dev either way (kernel time: read_lanczos in place of read_average).  The switch exists only
 * because the suite pins the refusal on a default context; making the rule's choice the default is a one-line follow-up. */
int sarpro_hip_dualpol_synrgb_read_u16_dev(sarpro_hip_ctx *ctx, const uint16_t *d_band1, const uint16_t *d_band2, size_t rows, size_t cols,
                                           size_t in_pitch, int alg, int strategy, int mode, unsigned flags, size_t target_size, int pad,
                                           uint8_t *d_rgb_out, sarpro_hip_resize_meta *meta);
/* Host u16 bands in (compact), host RGB out: only the raw DNs and the product cross PCIe. */
int sarpro_hip_dualpol_synrgb_read_u16(sarpro_hip_ctx *ctx, const uint16_t *band1, const uint16_t *band2, size_t rows, size_t cols, int alg,
                                       int strategy, int mode, unsigned flags, size_t target_size, int pad, uint8_t *rgb_out,
                                       sarpro_hip_resize_meta *meta);
/* The bands through a row reader and the pinned ring (as sarpro_hip_dualpol_synrgb_resized_stream_u16), then the device steps above. */
int sarpro_hip_dualpol_synrgb_read_stream_u16(sarpro_hip_ctx *ctx, sarpro_hip_row_reader reader, void *reader_user, size_t rows, size_t cols,
                                              int alg, int strategy, int mode, unsigned flags, size_t target_size, int pad, uint8_t *rgb_out,
                                              sarpro_hip_resize_meta *meta);
/* The same up to the FILE: the RGB raster stays on the device and is encoded there (the contract of the other _jpeg flows: when the
 * file does not fit, *jpeg_bytes_out is the size it needs and the status is SARPRO_HIP_ERR_BUFFER_TOO_SMALL). */
int sarpro_hip_dualpol_synrgb_read_stream_u16_jpeg(sarpro_hip_ctx *ctx, sarpro_hip_row_reader reader, void *reader_user, size_t rows,
                                                   size_t cols, int alg, int strategy, int mode, unsigned flags, size_t target_size, int pad,
                                                   uint8_t *jpeg_out, size_t jpeg_capacity, size_t *jpeg_bytes_out, unsigned restart_mcus,
                                                   sarpro_hip_resize_meta *meta);

/* ---- the Lanczos filter on read (restated in tests/readlanczosref.py).  Parity with GDAL's own Lanczos is UNPINNED:
 * GDAL is absent here and the reference does not lock its version; this is the a = 3 Lanczos kernel with its support scaled by the
 * reduction, as GDAL's resampler documents it, in f64 with one rounding to f32.
 *   per axis   n source samples -> m destination samples, 1 <= m <= n, n / m <= 5.  m == n: the identity (one tap, weight 1.0).
 *              m < n, all in f64: r = n / m; s = 3.0 * r; x = (j + 0.5) * r; first = max(0, (int)floor(x - s + 0.5));
 *              end = min(n, (int)floor(x + s + 0.5)); taps c = first .. end - 1 (at most 30); t = ((c + 0.5) - x) / r;
 *              raw = 1.0 if t == 0, 0.0 if |t| >= 3, else with pt = M_PI * t: (3.0 * sin(pt) * sin(pt / 3.0)) / (pt * pt) (glibc sin);
 *              tot = the raw weights added in ascending c from 0.0; w[c] = raw[c] / tot.  Taps clipped at the raster's edge are dropped
 *              before normalising.
 *   per pixel  H[y][j] = sum_c w_x[j][c] * (double)v[y][c] in ascending c from 0.0; out[i][j] = (float) sum_y w_y[i][y] * H[y][j] in
 *              ascending y from 0.0; every product and every sum rounded on its own (nothing fused), one round-to-nearest-even to
 *              f32.  NO CLAMP: a result may be negative or above 65535 (the kernel's lobes are signed); downstream such pixels count
 *              as invalid exactly as negative input of the f32 chain does.  H depends on (y, j) alone: the results are a function of
 *              the definition (bit for bit, whatever the tiling, pitch or load width).
 * One axis' tables (no GPU): first[n_dst], count[n_dst] and weights[n_dst * 32] -- 32 slots per destination sample, unused slots 0.0.
 * INVALID_ARG outside 1 <= n_dst <= n_src <= 2^30, when n_src / n_dst > 5, on a null pointer. */
int sarpro_hip_host_read_lanczos_axis(size_t n_src, size_t n_dst, uint32_t first[], uint32_t count[], double weights[]);
/* The Lanczos filter with the rules of sarpro_hip_read_average_u16_dev (shapes, pitches, load paths, stream order).  A per-axis ratio
 * above 5: SARPRO_HIP_ERR_UNSUPPORTED with a message naming the ratios; nothing is written.  Kernel time: read_lanczos. */
int sarpro_hip_read_lanczos_u16_dev(sarpro_hip_ctx *ctx, const uint16_t *d_in, size_t rows, size_t cols, size_t in_pitch, size_t out_rows,
                                    size_t out_cols, float *d_out_f32, size_t out_pitch);
/* The same with host pointers (compact rasters). */
int sarpro_hip_read_lanczos_u16(sarpro_hip_ctx *ctx, const uint16_t *in, size_t rows, size_t cols, size_t out_rows, size_t out_cols,
                                float *out_f32);

/* ================= speckle filtering: Lee and Kuan over u16 and f32 bands =================
 * The next per-pixel step SAR users expect, Phase 4 of the reference's roadmap (Lee, Kuan, Frost, Refined Lee; windows of 3-7 px;
 * placed before autoscale).  The reference's roadmap NAMES these filters and SHIPS NONE, so THE DEFINITION IS THIS PROJECT'S OWN: it is
 * fixed here operation by operation, the result is a function of it alone (bit for bit, whatever the tiling or pitch), and it is
 * tested by bit pattern against the numpy restatement tests/speckleref.py.  There is no parity target beyond that.
 *   parameters  filter = SARPRO_SPECKLE_LEE | SARPRO_SPECKLE_KUAN; window k in {3, 5, 7}, h = k / 2; looks: a finite f64 > 0.
 *               Once per call, in f64: cu2 = 1.0 / looks; g = 1.0 / (1.0 + cu2).  cu2 is the squared coefficient of variation of the
 *               speckle OF THE VALUES AS GIVEN: `looks` is L for L-look intensity; a caller filtering amplitude DNs passes the
 *               equivalent number of looks for amplitude, L / 0.2732.
 *   validity    u16: a sample is valid iff v >= 1 (DN 0 is the GRD black fill; the pipeline's mask gives the same answer).
 *               f32: valid iff thr <= v < +inf, thr = sarpro_hip_host_f32_valid_threshold(): NaN, +-inf and everything below thr
 *               are invalid.
 *   window      the k x k window around (y, x), clipped to the raster: no reflection, no padding.  Only valid samples count.
 *   per pixel   centre invalid: the output is (float)v for u16 and the input's bit pattern for f32 (the band's valid mask is
 *               unchanged by the filter).  Otherwise, with n >= 1 valid samples in the window (the centre included):
 *                 u16   S1 = sum v and S2 = sum v^2 as EXACT integers (any order); A = S1 * S1, D = n * S2 - A, exact integers in 64
 *                       bits; all stay below 2^45, so (double) of each is exact.
 *                 f32   for each window row, top to bottom, the row's partial sums left to right over its valid samples, in f64 from
 *                       0.0: r1 = sum (double)v, r2 = sum (double)v * (double)v; S1 and S2 are the row partials added top to bottom
 *                       from 0.0 (a row without a valid sample adds 0.0); A = S1 * S1, B = (double)n * S2, D = B - A.
 *                 m = S1 / (double)n, one correctly rounded division.
 *                 !(D > 0):  out = (float)m (for u16 this is exactly the centre value).
 *                 else       q = (cu2 * A) / D;  w = 1.0 - q (Lee) or (1.0 - q) * g (Kuan);  if !(w > 0) then w = 0;
 *                            out = (float)(m + w * ((double)v - m)).
 *               f64 throughout, nothing contracted, one round-to-nearest-even conversion to f32.
 *   properties  a constant raster comes back unchanged (65535 gives exactly 65535.0); out lies between m and v; a valid centre stays
 *               valid; with very few looks w is 0 everywhere and the result is the boxcar mean of the valid samples; with very many
 *               looks the result approaches the input.
 * Frost and Refined Lee over u16 bands: the _ext entry points further below; the calls of this section keep refusing them.
 * Not built: windows above 7, a u16 -> u16 form, f32 forms of Frost and Refined Lee, filtering inside the batch / stream / _jpeg /
 * stripe flows. */
typedef enum { SARPRO_SPECKLE_LEE = 0, SARPRO_SPECKLE_KUAN = 1, SARPRO_SPECKLE_FROST = 2, SARPRO_SPECKLE_REFINED_LEE = 3 } sarpro_hip_speckle_filter;
/* rows x cols samples (in_pitch elements per row) -> rows x cols f32 (out_pitch elements per row; the padding is not written), both in
 * device memory; any shape >= 1 x 1, rasters smaller than the window included.  Stream-ordered on the context's stream and synchronous
 * like the other _dev calls (on a SARPRO_HIP_CTX_ASYNC_DEV context it returns once enqueued).  u16: 16-byte loads when in_pitch % 8 ==
 * 0 and d_in is 16-byte aligned (the raster is rows x in_pitch elements: the last vector of a row may reach into the row's padding,
 * whose values are never used), element loads otherwise: the same results.  SARPRO_HIP_ERR_INVALID_ARG with a message, nothing
 * written: a bad filter, a window not in {3, 5, 7}, looks not finite or <= 0, a pitch below cols, an empty raster, a null pointer,
 * and for f32 an output raster that overlaps the input.  Kernel times: speckle_u16, speckle_f32. */
int sarpro_hip_speckle_u16_dev(sarpro_hip_ctx *ctx, const uint16_t *d_in, size_t rows, size_t cols, size_t in_pitch, int filter, int window,
                               double looks, float *d_out_f32, size_t out_pitch);
int sarpro_hip_speckle_f32_dev(sarpro_hip_ctx *ctx, const float *d_in, size_t rows, size_t cols, size_t in_pitch, int filter, int window,
                               double looks, float *d_out_f32, size_t out_pitch);
/* The same with host pointers (compact rasters): the band goes up, the filtered raster comes back. */
int sarpro_hip_speckle_u16(sarpro_hip_ctx *ctx, const uint16_t *in, size_t rows, size_t cols, int filter, int window, double looks,
                           float *out_f32);
int sarpro_hip_speckle_f32(sarpro_hip_ctx *ctx, const float *in, size_t rows, size_t cols, int filter, int window, double looks,
                           float *out_f32);
/* "Two measurement bands in, filtered at native resolution, RGB out": both bands filtered (one launch) into f32 rasters of the
 * context, then sarpro_hip_dualpol_synrgb_resized_f32_dev on them, unchanged, with the caller's strategy, mode, flags
 * (SARPRO_HIP_DUALPOL_PLAIN_PIPELINE or 0), target_size (0 = native size) and pad.  d_rgb_out: final_rows * final_cols * 3 bytes,
 * (final_cols, final_rows) = sarpro_hip_resize_output_dims(cols, rows, target_size, pad).  Synchronous.  No other entry point filters. */
int sarpro_hip_dualpol_synrgb_speckle_u16_dev(sarpro_hip_ctx *ctx, const uint16_t *d_band1, const uint16_t *d_band2, size_t rows, size_t cols,
                                              size_t in_pitch, int filter, int window, double looks, int strategy, int mode, unsigned flags,
                                              size_t target_size, int pad, uint8_t *d_rgb_out, sarpro_hip_resize_meta *meta);
/* Host u16 bands in (compact), host RGB out. */
int sarpro_hip_dualpol_synrgb_speckle_u16(sarpro_hip_ctx *ctx, const uint16_t *band1, const uint16_t *band2, size_t rows, size_t cols,
                                          int filter, int window, double looks, int strategy, int mode, unsigned flags, size_t target_size,
                                          int pad, uint8_t *rgb_out, sarpro_hip_resize_meta *meta);

/* ================= speckle filtering: Frost and Refined Lee over u16 bands =================
 * The other two filters of the roadmap's Phase 4.  As above THE DEFINITIONS ARE THIS PROJECT'S OWN, fixed here operation by operation;
 * the result is a function of them alone, bit for bit, whatever the tiling, the pitch or the load width; the kernels are tested by f32
 * bit pattern against the numpy restatement tests/speckleextref.py.  u16 bands only.
 *   common      as above: a sample is valid iff v >= 1; the window is clipped to the raster, no reflection; only valid samples count;
 *               an invalid centre gives 0.0f; f64 throughout, nothing contracted, one round-to-nearest-even conversion to f32.
 *   EXP(x)      for x <= 0, the library's own exponential (no libm is trusted).  LOG2E = 0x1.71547652b82fep+0, LN2_HI =
 *               0x1.62e42fee00000p-1, LN2_LO = 0x1.a39ef35793c76p-33 (fdlibm's split of ln 2), c_i = 1.0 / (double)(i!) for i = 0..13,
 *               each one correctly rounded division (every i! is exact in f64).
 *                 1. x < -708.0 (-inf included): +0.0.
 *                 2. kf = rint(x * LOG2E), ties to even.
 *                 3. r = (x - kf * LN2_HI) - kf * LN2_LO.
 *                 4. p = c_13; for i = 12 down to 0: p = p * r + c_i, one multiplication then one addition.
 *                 5. ldexp(p, (int)kf), exact since kf >= -1022.
 *               EXP(0) = 1.0, results lie in (0, 1], within 1 ulp of a correctly rounded exp where measured.
 *   Frost       window k in {3, 5, 7}, h = k / 2, damping: a finite f64 > 0; looks is ignored.  Valid centre v, n >= 1 valid samples:
 *                 S1, S2, A = S1 * S1, D = n * S2 - A exact integers as above (A >= 1);  a = damping * ((double)D / (double)A).
 *                 The window's offsets fall into classes by r2 = dy^2 + dx^2: {0,1,2}, {0,1,2,4,5,8}, {0,1,2,4,5,8,9,10,13,18} for
 *                 k = 3, 5, 7.  T_c = the exact integer sum of the class's valid samples, N_c their number;
 *                 dist_c = sqrt((double)r2), IEEE-correct;  w_0 = 1.0, w_c = EXP(-(a * dist_c)) for c > 0.
 *                 From num = den = 0.0, over the classes in ascending r2: num = num + w_c * (double)T_c; den = den + w_c * (double)N_c
 *                 (an empty class adds +0.0).  out = (float)(num / den).
 *               D / A is the squared coefficient of variation of the window, so the weight is the classical exp(-K * Ci^2 * |t|).
 *               Every output is finite (a may overflow to +inf: EXP gives 0) and lies between the smallest and the largest valid
 *               sample of the window; a constant raster comes back unchanged; damping >= 1e6 returns the input.
 *   Refined Lee window 7, looks: a finite f64 > 0, cu2 = 1.0 / looks; damping is ignored.
 *               Fallback: if the 7 x 7 window is not wholly inside the raster, or any of its 49 samples is invalid, the output is
 *               exactly that of Lee with window 7 above, bit for bit.
 *               Directed (all 49 samples present and valid): B_ij, i, j in {0,1,2}, = the integer sum of the 3 x 3 block whose
 *               top-left offset is (dy, dx) = (-3 + 2i, -3 + 2j).  Integer gradients
 *                 g0 = |(B02+B12+B22) - (B00+B10+B20)|   g1 = |(B01+B02+B12) - (B10+B20+B21)|
 *                 g2 = |(B00+B01+B02) - (B20+B21+B22)|   g3 = |(B00+B01+B10) - (B12+B21+B22)|
 *               d = the index of the largest, the lowest index on a tie.  Each d has a pair (P, Q) and the half-window each selects:
 *                 d0: P = B12 -> E (dx >= 0),   Q = B10 -> W (dx <= 0)      d1: P = B02 -> NE (dx >= dy),     Q = B20 -> SW (dx <= dy)
 *                 d2: P = B01 -> N (dy <= 0),   Q = B21 -> S (dy >= 0)      d3: P = B00 -> NW (dx + dy <= 0), Q = B22 -> SE (dx + dy >= 0)
 *               P's half-window if |P - B11| <= |Q - B11|, else Q's: 28 samples, the centre among them.  Over it, with n = 28: S1, S2,
 *               A = S1 * S1, D = 28 * S2 - A exact integers, m = S1 / 28.0;  !(D > 0): out = (float)m;  else q = (cu2 * A) / D,
 *               w = 1.0 - q, w = 0 if !(w > 0), out = (float)(m + w * ((double)v - m)).
 * The _ext calls accept all four filters.  With SARPRO_SPECKLE_LEE or SARPRO_SPECKLE_KUAN they give exactly what the calls above give
 * (the same kernel, the same bits; damping is ignored).  Stream order, synchrony, SARPRO_HIP_CTX_ASYNC_DEV, pitches, alignment and the
 * choice between 16-byte and element loads are those of sarpro_hip_speckle_u16_dev; the output's padding is not written; any shape
 * >= 1 x 1.  SARPRO_HIP_ERR_INVALID_ARG with a message, nothing written: everything the calls above reject, a filter outside 0..3,
 * Frost with a window not in {3, 5, 7} or a damping that is not finite or <= 0, Refined Lee with a window other than 7 or looks not
 * finite or <= 0.  Kernel times: speckle_frost_u16, speckle_rlee_u16 (Lee, Kuan: speckle_u16). */
int sarpro_hip_speckle_ext_u16_dev(sarpro_hip_ctx *ctx, const uint16_t *d_in, size_t rows, size_t cols, size_t in_pitch, int filter, int window,
                                   double looks, double damping, float *d_out_f32, size_t out_pitch);
int sarpro_hip_speckle_ext_u16(sarpro_hip_ctx *ctx, const uint16_t *in, size_t rows, size_t cols, int filter, int window, double looks,
                               double damping, float *out_f32);
/* The flows of sarpro_hip_dualpol_synrgb_speckle_u16(_dev) with any of the four filters: they differ in the filter step alone. */
int sarpro_hip_dualpol_synrgb_speckle_ext_u16_dev(sarpro_hip_ctx *ctx, const uint16_t *d_band1, const uint16_t *d_band2, size_t rows, size_t cols,
                                                  size_t in_pitch, int filter, int window, double looks, double damping, int strategy, int mode,
                                                  unsigned flags, size_t target_size, int pad, uint8_t *d_rgb_out, sarpro_hip_resize_meta *meta);
int sarpro_hip_dualpol_synrgb_speckle_ext_u16(sarpro_hip_ctx *ctx, const uint16_t *band1, const uint16_t *band2, size_t rows, size_t cols,
                                              int filter, int window, double looks, double damping, int strategy, int mode, unsigned flags,
                                              size_t target_size, int pad, uint8_t *rgb_out, sarpro_hip_resize_meta *meta);
/* EXP of the definition above on the host (no GPU): the same source sequence as the kernels'.  NaN for a NaN or x > 0. */
double sarpro_hip_host_speckle_exp(double x);

/* ---- file shims for the two callbacks: uncompressed strip TIFF / BigTIFF (what Sentinel-1 GRD measurement rasters
 * are; io/gdal.rs:107-141 and io/writers/tiff.rs:6-78 go through GDAL).  Baseline TIFF 6.0 + BigTIFF, II or MM,
 * Compression = 1, strips, 8- / 16-bit unsigned samples, chunky or planar; anything else fails with
 * SARPRO_HIP_ERR_IO and a message (sarpro_hip_tiff_last_error, per thread).  No GPU involved. ---- */
typedef struct sarpro_hip_tiff sarpro_hip_tiff;
typedef struct sarpro_hip_tiff_writer sarpro_hip_tiff_writer;
typedef struct {
    uint64_t width, height, rows_per_strip;
    uint32_t bits_per_sample, samples_per_pixel, sample_format, planar, compression, big_endian, bigtiff, tiled;
    uint32_t has_geo;        /* bit 0: pixel_scale, bit 1: tiepoint, bit 2: GeoKey directory */
    uint32_t tiepoint_count; /* GRD products carry a GCP grid: only the first tiepoint is returned here */
    double pixel_scale[3], tiepoint[6];
} sarpro_hip_tiff_info;
int sarpro_hip_tiff_open(const char *path, sarpro_hip_tiff **out, sarpro_hip_tiff_info *info_out);
int sarpro_hip_tiff_read_rows_u16(sarpro_hip_tiff *t, int sample, size_t row0, size_t nrows, uint16_t *dst, size_t dst_pitch);
void sarpro_hip_tiff_close(sarpro_hip_tiff *t);
/* a sarpro_hip_row_reader over two single-band files: user = sarpro_hip_tiff *[2] (band 0, band 1) */
int sarpro_hip_tiff_pair_reader(void *user, int band, size_t row0, size_t nrows, uint16_t *dst, size_t dst_pitch);
/* geotransform6 (GDAL order, north-up) and geo_keys_from (GeoKey directory carried over verbatim) may be NULL */
int sarpro_hip_tiff_create(const char *path, uint64_t width, uint64_t height, uint32_t samples, uint32_t bits,
                           const double *geotransform6, const sarpro_hip_tiff *geo_keys_from, sarpro_hip_tiff_writer **out);
int sarpro_hip_tiff_write_rows(sarpro_hip_tiff_writer *w, size_t row0, size_t nrows, const void *src, size_t src_pitch_bytes);
/* a sarpro_hip_row_sink: user = sarpro_hip_tiff_writer * */
int sarpro_hip_tiff_row_sink(void *user, size_t row0, size_t nrows, const uint8_t *src, size_t src_pitch_bytes);
int sarpro_hip_tiff_finish(sarpro_hip_tiff_writer *w); /* writes the directory, closes and frees the writer */
const char *sarpro_hip_tiff_last_error(void);
/* A TILED file with overviews, uncompressed, in cloud-optimised order: the header; then every directory with its
 * TileOffsets / TileByteCounts arrays -- the full resolution first, then overviews 1..levels with NewSubfileType = 1, level k of
 * ceil(w_{k-1} / 2) x ceil(h_{k-1} / 2) pixels --; then the tile data, the SMALLEST level first and the full resolution last, each
 * level's tiles row-major, edge tiles zero-padded.  Nothing is compressed, so every offset is fixed at creation and the directories
 * are written then; tile is a multiple of 16 (0: 512); levels 0..16.  Photometric / ExtraSamples / SampleFormat as
 * sarpro_hip_tiff_create writes them for the same sample count; the geo tags go on directory 0 only.  BigTIFF by the strip writer's
 * rule applied to the whole file (sarpro_hip_tiff_pyramid_is_bigtiff), or whatever the size when SARPRO_HIP_TIFF_BIGTIFF=YES (or 1)
 * is in the environment at creation (GDAL's BIGTIFF=YES creation option).  GDAL's ghost "structural metadata" block is NOT written.
 * Rows of level `level` (0 = the full resolution) may arrive in any order and any chunking: the writer scatters them into their
 * tiles at the tiles' final offsets; tiles never written read as zeros.  sarpro_hip_tiff_finish completes and closes the file.
 * sarpro_hip_tiff_write_rows / _row_sink on such a writer write level 0.  The reader of this shim stays strip-only. */
int sarpro_hip_tiff_create_pyramid(const char *path, uint64_t width, uint64_t height, uint32_t samples, uint32_t bits, uint32_t tile, int levels,
                                   const double *geotransform6, const sarpro_hip_tiff *geo_keys_from, sarpro_hip_tiff_writer **out);
int sarpro_hip_tiff_write_level_rows(sarpro_hip_tiff_writer *w, int level, size_t row0, size_t nrows, const void *src, size_t src_pitch_bytes);
/* The size rule, a pure function: 1 when a pyramid file of this shape is written as BigTIFF (header, directories without geo tags and
 * tile data, plus 1 MiB, reach 2^32 - 1 bytes: the strip writer's rule), 0 for a classic file, < 0 for bad arguments.
 * *file_bytes_out (may be NULL): the size of that file without geo tags. */
int sarpro_hip_tiff_pyramid_is_bigtiff(uint64_t width, uint64_t height, uint32_t samples, uint32_t bits, uint32_t tile, int levels,
                                       uint64_t *file_bytes_out);
/* sysfs cpulist syntax ("0-31,64-95") -> CPU numbers, at most max of them; returns the count, -1 on a syntax error.  The batch
 * driver binds each worker thread to the CPUs of its GPU's NUMA node with it (csrc/batch.cpp). */
int sarpro_hip_host_parse_cpulist(const char *s, int *cpus, int max);
/* the geotransform of a resized / padded product, save.rs:71-81 (pixel size by cols / final_cols, origin by the padding) */
void sarpro_hip_host_update_geotransform(double gt[6], size_t cols, size_t rows, const sarpro_hip_resize_meta *m);

/* ================= overview pyramids and the tiled GeoTIFF with overviews =================
 * The reference's roadmap puts "COG + overviews" (TILED=YES, 512 or 256 blocks, BuildOverviews with AVERAGE) right behind the
 * plumbing this library mirrors and ships none of it: the definition is this library's own, restated in tests/overviewref.py.
 * Parity with GDAL's AVERAGE overviews is UNPINNED (GDAL is absent, and it takes fractional source windows at odd sizes); this is
 * the aligned cascade a COG reader assumes geometrically.
 *   rasters   u8 or u16 samples (bits 8 / 16), 1..3 components interleaved, row pitch in BYTES
 *   shapes    level 0 is the raster; level k has w_k = ceil(w_{k-1} / 2), h_k = ceil(h_{k-1} / 2)
 *   levels    the smallest L >= 0 with max(w_L, h_L) <= min_size (min_size 0: 512), at most 16
 *   a pixel   of level k, per component: (sum + n / 2) / n in integer arithmetic over the n in {1, 2, 4} samples of the ROUNDED
 *             level k - 1 at rows 2i, 2i + 1 and columns 2j, 2j + 1 that exist (round half up of the mean)
 *   SKIP_ZERO 0 is this library's no-data level: a source pixel takes part only if one of its components is non-zero; n = 0
 *             gives 0 in every component.  ((1,0,0), (0,1,0), (0,0,1) average to (0,0,0): no-data one level up, by definition.)
 * The result is a function of this definition alone, whatever the levels per launch (context attribute OVR_DEPTH, 1..6: at 6 ONE sweep
 * over the source writes six levels, at 1 every level is a launch of its own; unset: 2, as fast as 1 and 1.75 x faster than 6 where
 * measured), pitch or alignment.  A plan places levels 1..L in ONE packed buffer: entry k of its arrays is level k + 1, pitch_bytes =
 * row bytes rounded up to 16, offset_bytes multiples of 256.  The bytes between a row's end and its pitch and between levels are
 * never written. */
#define SARPRO_HIP_OVR_MAX_LEVELS 16
#define SARPRO_HIP_OVR_SKIP_ZERO 1u
typedef struct {
    int levels, components, bits, reserved;
    size_t cols[16], rows[16], pitch_bytes[16], offset_bytes[16];
    size_t total_bytes;
} sarpro_hip_ovr_plan;
/* No GPU.  Returns the level count (>= 0) and fills *out; SARPRO_HIP_ERR_INVALID_ARG for a zero size, components outside 1..3,
 * bits other than 8 / 16 or a NULL plan. */
int sarpro_hip_overview_plan(size_t cols, size_t rows, int components, int bits, size_t min_size, sarpro_hip_ovr_plan *out);
/* Levels 1..L of the raster at d_src into d_out (plan->total_bytes), both in device memory; kernel-time name "overviews" (one
 * entry per launch: ceil(L / OVR_DEPTH), OVR_DEPTH unset = 2).  Stream-ordered on the context's stream; synchronous, enqueue-only on a
 * SARPRO_HIP_CTX_ASYNC_DEV context.  The plan must be one of this raster (a caller may widen pitches and offsets).  A source that
 * is 16-byte aligned with pitch_bytes % 16 == 0 takes 16-byte loads, any other (aligned to its sample size) element loads with the
 * same results.  A plan of 0 levels is a successful no-op. */
int sarpro_hip_overviews_dev(sarpro_hip_ctx *ctx, const void *d_src, size_t cols, size_t rows, size_t pitch_bytes, int components, int bits,
                             unsigned flags, const sarpro_hip_ovr_plan *plan, void *d_out);
/* host pointers: a compact source in, the packed buffer out (its padding bytes keep the caller's values) */
int sarpro_hip_overviews(sarpro_hip_ctx *ctx, const void *src, size_t cols, size_t rows, int components, int bits, unsigned flags,
                         const sarpro_hip_ovr_plan *plan, void *out);
/* the same definition on the host: no GPU, one thread, the same packed layout */
int sarpro_hip_host_overviews(const void *src, size_t cols, size_t rows, size_t pitch_bytes, int components, int bits, unsigned flags,
                              const sarpro_hip_ovr_plan *plan, void *out);
/* sarpro_hip_dualpol_synrgb_u16_dev without the per-band u8 outputs, then the pyramid of its RGB raster (components 3, bits 8, pitch
 * rgb_pitch_px * 3 bytes) into d_ovr_out on the same stream: the RGB is that call's bit for bit, the levels are
 * sarpro_hip_overviews_dev's of that RGB, stats_out (may be NULL) that call's.  Where the chain is device-resident (every scene that
 * call runs without host round trips) there is NO host synchronisation between the chain and the sweep: the chain's final read-back
 * is left enqueued, the sweep goes behind it, and one synchronisation ends the call.  A scene that call orchestrates from the host
 * (the NO_CHAIN attribute, shapes the chain does not take) synchronises inside the chain as it always does.  Synchronous; on a
 * SARPRO_HIP_CTX_ASYNC_DEV context with stats_out == NULL the whole call is enqueue-only wherever that call is. */
int sarpro_hip_dualpol_synrgb_pyramid_u16_dev(sarpro_hip_ctx *ctx, const uint16_t *d_band1, const uint16_t *d_band2, size_t rows, size_t cols,
                                              size_t in_pitch, int strategy, int mode, uint8_t *d_rgb, size_t rgb_pitch_px,
                                              sarpro_hip_stats *stats_out, unsigned ovr_flags, const sarpro_hip_ovr_plan *plan, void *d_ovr_out);
/* Files in, one file out: the two bands through a row reader (sarpro_hip_tiff_pair_reader, a GDAL RasterIO loop, ...) into device
 * memory, the call above, and the product as a tiled GeoTIFF with overviews at `path` (sarpro_hip_tiff_create_pyramid: tile 0 = 512,
 * min_size 0 = 512; geotransform6 / geo_keys_from may be NULL).  The levels come down through pinned buffers in row chunks, the
 * smallest first, so the file is written front to back.  stats_out (may be NULL): sarpro_hip_stats[2]. */
int sarpro_hip_dualpol_synrgb_stream_u16_cog(sarpro_hip_ctx *ctx, sarpro_hip_row_reader reader, void *reader_user, size_t rows, size_t cols,
                                             int strategy, int mode, unsigned ovr_flags, uint32_t tile, size_t min_size, const char *path,
                                             const double *geotransform6, const sarpro_hip_tiff *geo_keys_from, sarpro_hip_stats *stats_out);

/* The same stripe in ONE call per rank, reductions over the library's communicator (sarpro_hip_comm_init
 * must have been called): the device-resident chains with their small all-reduces enqueued on the stream,
 * no host synchronisation until the stripe's RGB (rows_local x cols x 3) is complete.  Every rank of the
 * communicator must make the call (a rank may hold an empty stripe). */
int sarpro_hip_stripe_run_u16(sarpro_hip_ctx *ctx, const uint16_t *d_band1, const uint16_t *d_band2, size_t rows_total,
                              size_t cols, size_t row0, size_t rows_local, size_t in_pitch, int strategy, int mode,
                              uint8_t *d_rgb, size_t rgb_pitch_px, sarpro_hip_stats *stats_out);

/* Row stripes of one scene -> the RESIZED, padded product (save.rs:317-367: per-band u8 autoscale at native resolution -> Lanczos3
 * resize -> pad -> synRGB; SURVEY.md 8e's halo item).  Each rank holds rows [row0, row0 + rows_local) of both DN rasters -- 1 / N of
 * the scene crossed its PCIe link -- and produces a contiguous range of the FINAL raster's rows: output row j of the vertical pass
 * belongs to the rank holding the centre row of j's window, the rows its window needs from the neighbours travel in ONE small
 * all-reduce (sarpro_amd/csrc/resize_path.cpp); the rank owning the first / last resized row also owns the padding above / below.
 * d_rgb_slice receives out_rows x final_cols x 3 bytes, compact; the caller places them at row *out_row0 of the product.  Size the
 * slice with sarpro_hip_stripe_resized_rows (pure host arithmetic, the same answer on every rank).  The stripes must tile the scene in
 * rank order; every rank of the communicator makes the call (a rank may hold an empty stripe).  The assembled raster is that of
 * sarpro_hip_dualpol_synrgb_resized_u16_dev on the one-piece scene, bit for bit. */
int sarpro_hip_stripe_resized_rows(size_t rows_total, size_t cols, size_t row0, size_t rows_local, size_t target_size, int pad,
                                   size_t *out_row0, size_t *out_rows, size_t *final_cols, size_t *final_rows);
int sarpro_hip_stripe_run_resized_u16(sarpro_hip_ctx *ctx, const uint16_t *d_band1, const uint16_t *d_band2, size_t rows_total, size_t cols,
                                      size_t row0, size_t rows_local, size_t in_pitch, int strategy, int mode, size_t target_size, int pad,
                                      uint8_t *d_rgb_slice, size_t *out_row0, size_t *out_rows, sarpro_hip_resize_meta *meta);
/* the same for f32 bands (the reference's default, resampled-on-read flow; flags: SARPRO_HIP_DUALPOL_*): the levels come from the
 * striped f32 chain (process_scalar_data_pipeline at U8); under Tamed without SARPRO_HIP_DUALPOL_PLAIN_PIPELINE from the band-specific
 * re-autoscale of save.rs:324-351 (autoscale_db_image_tamed_synrgb_u8 over stripes: the same collectives, the Tamed windows from the
 * same all-reduced bins), with the flag as api/mod.rs:404-437 has it (both bands through the pipeline's Tamed arm). */
int sarpro_hip_stripe_run_resized_f32(sarpro_hip_ctx *ctx, const float *d_band1, const float *d_band2, size_t rows_total, size_t cols, size_t row0,
                                      size_t rows_local, size_t in_pitch, int strategy, int mode, unsigned flags, size_t target_size, int pad,
                                      uint8_t *d_rgb_slice, size_t *out_row0, size_t *out_rows, sarpro_hip_resize_meta *meta);

/* Self-test: the division the u16 pol-op kernels use (the Newton core of the IEEE division without its rescaling frame) against
 * the compiler's IEEE division over ALL 2^32 pairs of u16 values, ratio and normalised difference.  *mismatches_out must be 0. */
int sarpro_hip_selftest_polop_division(sarpro_hip_ctx *ctx, uint64_t *mismatches_out);

/* ---- row stripes of the f32 flavour (a calibrated f32 band, or a polarisation operation of two bands computed on the
 * fly): autoscale.rs:35-117 needs the scene's count / min / max before it can bin, and the scene's 4096 bins before it can
 * select the window, so the protocol has one more reduction than the u16 one.  One open f32 stripe per context. ---- */
typedef struct {
    uint64_t count;           /* valid samples                      merge: sum */
    double sum_db, sumsq_db;  /* of dB over the valid samples       merge: sum (in rank order: sarpro_hip_host_f32_merge_partials) */
    float min_v, max_v;       /* of the valid samples (+inf / -inf when there is none)   merge: min / max */
} sarpro_hip_f32_partial;
typedef struct sarpro_hip_stripe_f32 sarpro_hip_stripe_f32;
/* this rank owns rows [row0, row0 + rows_local) of the rows_total x cols scene; d_in / d_out are the local stripe */
int sarpro_hip_stripe_begin_f32(sarpro_hip_ctx *ctx, const float *d_in, size_t rows_total, size_t cols, size_t row0,
                                size_t rows_local, size_t in_pitch, int strategy, int bit_depth, void *d_out, size_t out_pitch,
                                sarpro_hip_stripe_f32 **out);
/* the samples are op(a, b) (ops.rs:4-44) of two f32 (elem_u16 = 0) or u16 DN (elem_u16 = 1) stripes */
int sarpro_hip_stripe_begin_polop(sarpro_hip_ctx *ctx, int op, const void *d_a, const void *d_b, int elem_u16, size_t rows_total,
                                  size_t cols, size_t row0, size_t rows_local, size_t in_pitch, int strategy, int bit_depth,
                                  void *d_out, size_t out_pitch, sarpro_hip_stripe_f32 **out);
/* phase 1: the stripe's count / min / max / dB moments, on the HOST (32 bytes); the caller gathers and merges them */
int sarpro_hip_stripe_f32_phase1(sarpro_hip_stripe_f32 *s, sarpro_hip_f32_partial *local_out);
int sarpro_hip_host_f32_merge_partials(const sarpro_hip_f32_partial *parts, size_t n, sarpro_hip_f32_partial *out);
/* phase 2: the stripe's 4096-bin histogram over the scene's [min, max] (autoscale.rs:102-117) -> all-reduce(sum) */
int sarpro_hip_stripe_f32_phase2(sarpro_hip_stripe_f32 *s, const sarpro_hip_f32_partial *global, uint64_t **d_buf, size_t *count);
/* phase 3: statistics and window from the merged bins; CLAHE: the stripe's tile histograms -> all-reduce(sum) (else count 0) */
int sarpro_hip_stripe_f32_phase3(sarpro_hip_stripe_f32 *s, uint64_t **d_buf, size_t *count);
/* phase 4: the stripe's levels; u8: histogram of the pre-rescale levels -> all-reduce(sum) (u16: count 0) */
int sarpro_hip_stripe_f32_phase4(sarpro_hip_stripe_f32 *s, uint64_t **d_buf, size_t *count);
/* phase 5: u8 rescale in place (autoscale.rs:348-364); the stripe of the output raster is complete on return */
int sarpro_hip_stripe_f32_phase5(sarpro_hip_stripe_f32 *s, sarpro_hip_stats *stats_out);
void sarpro_hip_stripe_f32_end(sarpro_hip_stripe_f32 *s);
/* the same in one call per rank over the library's communicator (every rank must make the call) */
int sarpro_hip_stripe_run_f32(sarpro_hip_ctx *ctx, const float *d_in, size_t rows_total, size_t cols, size_t row0, size_t rows_local,
                              size_t in_pitch, int strategy, int bit_depth, void *d_out, size_t out_pitch, sarpro_hip_stats *stats_out);
int sarpro_hip_stripe_run_polop(sarpro_hip_ctx *ctx, int op, const void *d_a, const void *d_b, int elem_u16, size_t rows_total,
                                size_t cols, size_t row0, size_t rows_local, size_t in_pitch, int strategy, int bit_depth,
                                void *d_out, size_t out_pitch, sarpro_hip_stats *stats_out);

/* RCCL communicator owned by the library (optional: callers may reduce the phase buffers
 * with their own communicator, e.g. torch.distributed's).  uid is the 128-byte
 * ncclUniqueId produced by sarpro_hip_comm_unique_id on rank 0 and shipped to all ranks. */
int sarpro_hip_comm_unique_id(uint8_t uid_out[128]);
int sarpro_hip_comm_init(sarpro_hip_ctx *ctx, int nranks, int rank, const uint8_t uid[128]);
int sarpro_hip_comm_allreduce_sum_u64(sarpro_hip_ctx *ctx, uint64_t *d_buf, size_t count);
/* The same communicator for the contexts of ONE process (one context and one host thread per rank -- several GPUs of a node driven by
 * threads as sarpro_hip_batch_* does, or several contexts on one GPU): no RCCL, no rendezvous.  An all-reduce is a barrier, a sum kernel
 * over the ranks' device buffers (they must be mutually accessible: one device, or peer access enabled by the caller) and a second
 * barrier; every rank's thread must be inside the collective for it to complete.  Create the group once, join it from every context,
 * destroy it after the contexts.  The stripe entry points (sarpro_hip_stripe_run_*) use whichever communicator the context has. */
typedef struct sarpro_hip_local_group sarpro_hip_local_group;
int sarpro_hip_local_group_create(int nranks, sarpro_hip_local_group **out);
void sarpro_hip_local_group_destroy(sarpro_hip_local_group *group);
int sarpro_hip_comm_init_local(sarpro_hip_ctx *ctx, sarpro_hip_local_group *group, int rank);
void sarpro_hip_comm_destroy(sarpro_hip_ctx *ctx);

/* ================= host half of the path (no GPU needed) ================= */
/* compute_histogram_stats (autoscale.rs:35-160) from the exact 65536-bin DN histogram of a
 * u16 band (valid <=> DN >= 1, pipeline.rs:19-22). */
int sarpro_hip_host_stats_from_dn_hist(const uint64_t dn_hist[65536], sarpro_hip_stats *out);
/* Strategy window (autoscale.rs:404-429 Standard; :491-564 advanced; :721-729 tamed-synrgb
 * when tamed_synrgb = 1 copol / 2 crosspol) -> fills low_clip/high_clip/gamma in *stats. */
int sarpro_hip_host_window(sarpro_hip_stats *stats, int strategy, int tamed_synrgb);
/* Level of every DN under the window: the u16 the reference's map loop yields
 * (autoscale.rs:437-447 / :647-655; tamed :731-741), max_val 255 or 65535.  lut[0] = 0. */
int sarpro_hip_host_level_lut_u16(const sarpro_hip_stats *stats, int bit_depth, int tamed_synrgb,
                                  uint16_t lut_out[65536]);
/* CLAHE bin of every DN (autoscale.rs:583-591 then :262-265): 0..255. */
int sarpro_hip_host_clahe_bin_lut_u16(const sarpro_hip_stats *stats, uint8_t lut_out[65536]);
/* Clip / redistribute / CDF for all tiles (autoscale.rs:271-302).  tile_hists is
 * [8*8][256] counts in tile order ty*8+tx; cdfs_out is [64][256] f64. */
int sarpro_hip_host_clahe_cdfs(const uint64_t *tile_hists, size_t rows, size_t cols,
                               double *cdfs_out);
/* scale_u16_to_u8 (autoscale.rs:348-364) as a 256-entry map for levels 0..255 given the
 * global min / max of the level raster. */
int sarpro_hip_host_u8_rescale_lut(unsigned min_level, unsigned max_level, uint8_t lut_out[256]);
/* LUTs of create_synthetic_rgb (synthetic_rgb.rs:20-51) / _suppressed (:92-155, from the
 * combined 256-bin histogram of both u8 bands).  luts_out = lut_r[256] | lut_g[256] |
 * lut_b[65536]; floor_out = floor_with_cushion (suppressed) or -1. */
int sarpro_hip_host_synrgb_luts(int strategy, const uint64_t combined_hist[256], uint64_t n_per_band,
                                uint8_t *luts_out, int *floor_out);
/* CLAHE shape check: 0 when the reference's tile arithmetic underflows (autoscale.rs:250,254). */
int sarpro_hip_host_clahe_shape_ok(size_t rows, size_t cols);
/* autoscale.rs:327-329 for a bin whose four tile CDFs are all 1.0 (every sample from p99 up): level 255 or -- in the first half tile
 * row / column, where a blend weight is negative and (1 - d) + d can round below 1.0 -- 254, by the pixel's row and column alone.
 * col_class[cols] in {0, 1, 2}; bit k of row_bits[rows]: a saturated pixel of that row in a column of class k gets 255 (else 254).
 * What the fused CLAHE -> RGB pass uses instead of the f64 blend for such samples.  SARPRO_HIP_ERR_UNSUPPORTED_SHAPE: no table. */
int sarpro_hip_host_clahe_saturated_levels(size_t rows, size_t cols, uint8_t *col_class, uint8_t *row_bits);
/* Row-stripe plan: stripes aligned to CLAHE tile rows (tile_h = ceil(rows/8)).
 * row0_out / nrows_out hold nranks entries. */
int sarpro_hip_host_stripe_plan(size_t rows, int nranks, size_t *row0_out, size_t *nrows_out);

/* f32-input flavour: the per-pixel decisions as sorted f32 threshold tables (exact w.r.t. the
 * reference's f64/libm evaluation; the device only compares).  thr[0] is unused;
 * thr[k] = smallest valid f32 sample whose index/level is >= k (+inf if unreachable). */
/* percentiles of compute_histogram_stats (autoscale.rs:81-159) from its 4096-bin histogram */
int sarpro_hip_host_stats_from_bins4096(uint64_t valid_count, double min_db, double max_db, double mean_db,
                                        double std_db, const uint64_t hist4096[4096], sarpro_hip_stats *out);
float sarpro_hip_host_f32_valid_threshold(void); /* smallest f32 with 10*log10(v) > -50 (pipeline.rs:22) */
int sarpro_hip_host_f32_bin4096_thresholds(double min_db, double max_db, float thr_out[4096]); /* autoscale.rs:113-115 */
/* levels (autoscale.rs:440-442) under stats->low_clip/high_clip/gamma: 256 (U8) or 65536 (U16) entries */
int sarpro_hip_host_f32_level_thresholds(const sarpro_hip_stats *stats, int bit_depth, float *thr_out);
int sarpro_hip_host_f32_clahe_bin_thresholds(const sarpro_hip_stats *stats, float thr_out[256]); /* autoscale.rs:585-586,262-265 */

/* ================= synthetic scene generator (bench / tests) ================= */
/* counter-based (splitmix64) dual-pol GRD-like scene written
 * straight into HBM.  q_tables: 2 bands x 4 classes x 65536 u16 inverse-CDF tables
 * (host pointer).  band in {0,1}. */
int sarpro_hip_synth_scene_u16_dev(sarpro_hip_ctx *ctx, uint64_t seed, int band,
                                   const uint16_t *q_tables_host, size_t rows_total, size_t cols,
                                   size_t row0, size_t rows_local, uint16_t *d_out, size_t pitch);
/* The same generator with the scene's structure selectable (bench.py cycles its timed steps over scenes that differ in
 * distribution, not only in seed).  flags: bit 0 no no-data wedges (no invalid pixel anywhere), bit 1 no bright targets, bit 2 an all-invalid second band,
 * bits 4-7 class map (0: (r/b + 3 c/b) mod 4, the generator above; 1: (r/b xor c/b) mod 4; 2: diagonal bands ((r + c) / b) mod 4;
 * 3: one class -- table 1 -- everywhere), bits 8-15 class blocks per side (0 = 16: b = ceil(rows / 16)). */
#define SARPRO_HIP_SYNTH_NO_WEDGE 1u
#define SARPRO_HIP_SYNTH_NO_BRIGHT 2u
#define SARPRO_HIP_SYNTH_NO_BAND2 4u   /* band 1 (the second) is no-data everywhere */
#define SARPRO_HIP_SYNTH_MAP(m) (((unsigned)(m) & 15u) << 4)
#define SARPRO_HIP_SYNTH_BLOCKS(n) (((unsigned)(n) & 255u) << 8)
int sarpro_hip_synth_scene_u16_dev_ex(sarpro_hip_ctx *ctx, uint64_t seed, int band,
                                      const uint16_t *q_tables_host, size_t rows_total, size_t cols,
                                      size_t row0, size_t rows_local, uint16_t *d_out, size_t pitch, uint32_t flags);

#ifdef __cplusplus
}
#endif
#endif /* SARPRO_HIP_H */
