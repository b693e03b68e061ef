// read_path.cpp -- downsample on read (io/sentinel1.rs:1074-1108 -> io/gdal.rs:145-177): SafeReader::open_with_options(.., target_size)
// has GDAL resample each band while reading it, the long side going to target_size, with ResampleAlg::Average when the reduction is
// >= 4 (every GRD quicklook) and Lanczos below; the few-MP f32 bands that result are what the raster core processes.  Here: the
// output shape and the filter rule, the Average filter's per-axis window tables (host, f64, every operation in the order DESIGN.md
// 9b fixes), the device pass over u16 bands (read_kernels.hip) and the flows "two u16 bands in, quicklook RGB / JPEG out".
// Parity with GDAL's own Average is unpinned (GDAL is absent, the reference does not lock its version): the definition is the
// weighted box its average resampler documents, restated in tests/readref.py.  The Lanczos filter (a = 3, the support
// scaled by the reduction, restated in tests/readlanczosref.py; parity with GDAL's own Lanczos is unpinned in the same way) is built
// for per-axis ratios up to 5 and enters the flows on a context whose READ_LANCZOS attribute is on.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "api_common.h"
#include "internal.h"
#include "read_kernels.h"

using namespace sarpro;

// ---- the steps every "two u16 bands in, quicklook RGB out" flow takes (internal.h; speckle_path.cpp's host flow takes them too)
int sarpro::check_flow(sarpro_hip_ctx *ctx, int strategy, int mode, unsigned flags) { // (before anything is enqueued or crosses PCIe)
    if (strategy < 0 || strategy > SARPRO_STRATEGY_DEFAULT) return fail(ctx, SARPRO_HIP_ERR_INVALID_ARG, "bad strategy");
    if (mode < 0 || mode > SARPRO_SYNRGB_ENHANCED) return fail(ctx, SARPRO_HIP_ERR_INVALID_ARG, "bad synrgb mode");
    if (flags & ~SARPRO_HIP_DUALPOL_PLAIN_PIPELINE) return fail(ctx, SARPRO_HIP_ERR_INVALID_ARG, "unknown dual-pol flag");
    return SARPRO_HIP_OK;
}

int sarpro::stage_bands(sarpro_hip_ctx *ctx, const uint16_t *const host[2], sarpro_hip_row_reader reader, void *reader_user, size_t rows, size_t cols,
                        size_t pitch) {
    HIPCHK(ctx, hipSetDevice(ctx->device));
    for (int b = 0; b < 2; ++b) {
        HIPCHK(ctx, ctx->read_src[b].reserve(rows * pitch * sizeof(uint16_t)));
        if (reader) {
            HIPCHK(ctx, hipStreamSynchronize(ctx->stream)); // the ring's slots are free: the previous band has landed
            RETCHK(stream_upload_band(ctx, reader, reader_user, b, rows, cols, ctx->read_src[b].as<uint16_t>(), pitch, 0));
        } else {
            HIPCHK(ctx, hipMemcpy2DAsync(ctx->read_src[b].p, pitch * 2, host[b], cols * 2, cols * 2, rows, hipMemcpyHostToDevice, ctx->stream));
        }
    }
    return SARPRO_HIP_OK;
}

int sarpro::rgb_to_host(sarpro_hip_ctx *ctx, uint8_t *rgb_out, size_t bytes) {
    if (!bytes) return SARPRO_HIP_OK;
    HIPCHK(ctx, hipMemcpyAsync(rgb_out, ctx->jpeg_rgb.p, bytes, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return SARPRO_HIP_OK;
}

namespace {

constexpr size_t kReadMaxDim = (size_t)1 << 30;

// sentinel1.rs:1084-1102.  f64::round is half away from zero: std::round.
void read_dims(size_t cols, size_t rows, size_t ts, size_t *oc, size_t *orows, int *alg) {
    const size_t long_side = std::max(cols, rows);
    const double scale = std::min((double)ts / (double)long_side, 1.0);
    *oc = (size_t)std::max(std::round((double)cols * scale), 1.0);
    *orows = (size_t)std::max(std::round((double)rows * scale), 1.0);
    const double reduction = std::max((double)long_side / (double)ts, 1.0);
    *alg = reduction >= 4.0 ? SARPRO_READ_AVERAGE : SARPRO_READ_LANCZOS;
}

// One axis: destination sample j covers [j * r, min((j + 1) * r, n)), r = n / m.  Plain f64 + - * / in exactly this order.
void read_average_axis(size_t n, size_t m, ReadAxis *out) {
    const double r = (double)n / (double)m, nd = (double)n;
    for (size_t j = 0; j < m; ++j) {
        const double x0 = (double)j * r;
        const double x1 = std::min(((double)j + 1.0) * r, nd);
        const size_t c0 = (size_t)std::min(std::floor(x0), (double)(n - 1));
        const size_t c1 = std::max((size_t)std::min(std::ceil(x1), nd), c0 + 1);
        const size_t count = c1 - c0;
        ReadAxis e;
        e.first = (uint32_t)c0; e.count = (uint32_t)count;
        if (count == 1) { e.w_first = x1 - x0; e.w_last = 0.0; }
        else { e.w_first = (double)(c0 + 1) - x0; e.w_last = x1 - (double)(c1 - 1); }
        e.w_sum = (e.w_first + (double)(count > 2 ? count - 2 : 0)) + e.w_last;
        out[j] = e;
    }
}

// One axis of the Lanczos filter: n source samples -> m destination samples, 1 <= m <= n.  Destination sample j is
// centred at x = (j + 0.5) * r in source coordinates, r = n / m; its window holds the source samples whose centres lie within 3 * r
// of x, clipped to the axis; a sample weighs lanczos3(distance / r), the weights of the window normalised by their sum in ascending
// order.  Plain f64 + - * / and glibc's sin in exactly this order.  m == n: the identity, one tap of weight 1.0.  Every window's
// kLanczosTaps weight slots are written (unused: 0.0).  false: a window needs more slots (never at n / m <= 5).
bool read_lanczos_axis(size_t n, size_t m, uint32_t *first, uint32_t *count, double *w) {
    std::memset(w, 0, m * kLanczosTaps * sizeof(double));
    if (m == n) {
        for (size_t j = 0; j < m; ++j) { first[j] = (uint32_t)j; count[j] = 1; w[j * kLanczosTaps] = 1.0; }
        return true;
    }
    const double r = (double)n / (double)m, s = 3.0 * r;
    for (size_t j = 0; j < m; ++j) {
        const double x = ((double)j + 0.5) * r;
        const long long lo = std::max<long long>(0, (long long)std::floor(x - s + 0.5));
        const long long hi = std::min<long long>((long long)n, (long long)std::floor(x + s + 0.5));
        if (hi <= lo || hi - lo > (long long)kLanczosTaps) return false;
        double *wj = w + j * kLanczosTaps, tot = 0.0;
        for (long long c = lo; c < hi; ++c) {
            const double t = (((double)c + 0.5) - x) / r;
            double raw = 1.0;
            if (std::fabs(t) >= 3.0) raw = 0.0;
            else if (t != 0.0) {
                const double pt = M_PI * t;
                raw = (3.0 * std::sin(pt) * std::sin(pt / 3.0)) / (pt * pt);
            }
            wj[c - lo] = raw;
            tot = tot + raw;
        }
        for (long long k = 0; k < hi - lo; ++k) wj[k] = wj[k] / tot;
        first[j] = (uint32_t)lo; count[j] = (uint32_t)(hi - lo);
    }
    return true;
}

constexpr double kLanczosMaxRatio = 5.0;
double axis_ratio(size_t n, size_t m) { return (double)n / (double)m; }

bool shape_ok(size_t rows, size_t cols, size_t out_rows, size_t out_cols) {
    return out_rows >= 1 && out_cols >= 1 && out_rows <= rows && out_cols <= cols && rows <= kReadMaxDim && cols <= kReadMaxDim;
}

// The tables of a shape (key: rows, cols, out_rows, out_cols) in their cache: when the shape changes they are rebuilt in the pinned
// stage by build(stage) -> a status, timed as the host segment `timer`, and uploaded on the context's stream.  A failing build leaves
// the cache without a shape.
template <typename Build>
int cached_tables(sarpro_hip_ctx *ctx, TableCache &c, const size_t key[4], size_t bytes, const char *timer, Build build) {
    if (c.tab.p && std::memcmp(key, c.key, sizeof(c.key)) == 0) return SARPRO_HIP_OK;
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream)); // (an earlier upload may still read the pinned stage on a stream-ordered context)
    c.key[0] = 0;
    HIPCHK(ctx, c.host.reserve(bytes));
    HIPCHK(ctx, c.tab.reserve(bytes));
    int rc;
    {
        HostTimer t(ctx, timer);
        rc = build(c.host.p);
    }
    RETCHK(rc);
    HIPCHK(ctx, hipMemcpyAsync(c.tab.p, c.host.p, bytes, hipMemcpyHostToDevice, ctx->stream));
    std::memcpy(c.key, key, sizeof(c.key));
    return SARPRO_HIP_OK;
}

// The Average pass over nb bands of one shape, enqueued on the context's stream.
int average_enqueue(sarpro_hip_ctx *ctx, const uint16_t *const d_in[], int nb, size_t rows, size_t cols, size_t in_pitch, size_t out_rows, size_t out_cols,
                    float *const d_out[], size_t out_pitch) {
    const size_t key[4] = {rows, cols, out_rows, out_cols};
    TableCache &tc = ctx->read_tables;
    RETCHK(cached_tables(ctx, tc, key, (out_cols + out_rows) * sizeof(ReadAxis), "host:read_tables", [&](void *stage) {
        ReadAxis *h = static_cast<ReadAxis *>(stage);
        read_average_axis(cols, out_cols, h);
        read_average_axis(rows, out_rows, h + out_cols);
        return SARPRO_HIP_OK;
    }));
    ReadArgs a{};
    const bool vec = band_rasters(a.io, d_in, nb, in_pitch, d_out, out_pitch);
    a.rows = (uint32_t)rows; a.cols = (uint32_t)cols; a.out_rows = (uint32_t)out_rows; a.out_cols = (uint32_t)out_cols;
    a.col_tab = tc.tab.as<ReadAxis>(); a.row_tab = a.col_tab + out_cols;
    // a strip's span of source columns fits one LDS slab where the reduction allows it (wider windows take several slabs per row)
    const double r = (double)cols / (double)out_cols;
    a.strip_cols = (uint32_t)std::min<double>(kReadThreads, std::max(1.0, std::floor((double)(kReadChunk - 16) / r)));
    // about 2048 tiles (8 per compute unit), a tile no taller than the row table the kernel keeps in LDS
    const size_t nstrips = (out_cols + a.strip_cols - 1) / a.strip_cols;
    a.band_rows = (uint32_t)std::min<size_t>(kReadMaxBandRows, std::max<size_t>(1, out_rows * nstrips * (size_t)nb / 2048));
    const ReadAxis *hc = tc.host.as<ReadAxis>(); // (the pinned stage keeps the tables of the cached shape)
    a.max_span = 0;
    for (size_t j0 = 0; j0 < out_cols; j0 += a.strip_cols) {
        const ReadAxis &l = hc[std::min<size_t>(j0 + a.strip_cols, out_cols) - 1];
        a.max_span = std::max(a.max_span, l.first + l.count - (hc[j0].first & ~7u));
    }
    KernelTimer t(ctx, "read_average");
    HIPCHK(ctx, launch_read_average_u16(a, vec, ctx->stream));
    return SARPRO_HIP_OK;
}

// The Lanczos pass over nb bands of one shape, enqueued on the context's stream.  Both per-axis ratios are <= 5 (the callers check).
int lanczos_enqueue(sarpro_hip_ctx *ctx, const uint16_t *const d_in[], int nb, size_t rows, size_t cols, size_t in_pitch, size_t out_rows, size_t out_cols,
                    float *const d_out[], size_t out_pitch) {
    const size_t key[4] = {rows, cols, out_rows, out_cols};
    const size_t nw = (out_cols + out_rows) * kLanczosTaps; // the weights of both axes, then first | count of the columns and of the rows
    TableCache &tc = ctx->lanczos_tables;
    RETCHK(cached_tables(ctx, tc, key, nw * sizeof(double) + 2 * (out_cols + out_rows) * sizeof(uint32_t), "host:read_lanczos_tables", [&](void *stage) {
        double *hw = static_cast<double *>(stage);
        uint32_t *hcf = reinterpret_cast<uint32_t *>(hw + nw), *hcc = hcf + out_cols, *hrf = hcc + out_cols, *hrc = hrf + out_rows;
        bool ok = read_lanczos_axis(cols, out_cols, hcf, hcc, hw) && read_lanczos_axis(rows, out_rows, hrf, hrc, hw + out_cols * kLanczosTaps);
        // what the kernel relies on: a strip's span of source columns (from its first window's vector boundary) and the slack of the
        // unused tap slots fit one LDS slab; window i of the rows is complete before window i + kLanczosRing opens
        uint32_t taps = 0;
        for (size_t j0 = 0; ok && j0 < out_cols; j0 += kReadThreads) {
            const size_t jl = std::min<size_t>(j0 + kReadThreads, out_cols) - 1;
            ok = hcf[jl] + hcc[jl] - (hcf[j0] & ~7u) + kLanczosTaps <= kLanczosChunk;
        }
        for (size_t j = 0; ok && j < out_cols; ++j) taps = std::max(taps, hcc[j]);
        for (size_t i = 0; ok && i + kLanczosRing < out_rows; ++i) ok = hrf[i] + hrc[i] <= hrf[i + kLanczosRing];
        ctx->lanczos_col_taps = taps;
        return ok ? SARPRO_HIP_OK : fail(ctx, SARPRO_HIP_ERR_UNSUPPORTED, "read: the Lanczos windows of this shape do not fit the kernel's tiles");
    }));
    LanczosArgs a{};
    const bool vec = band_rasters(a.io, d_in, nb, in_pitch, d_out, out_pitch);
    a.rows = (uint32_t)rows; a.cols = (uint32_t)cols; a.out_rows = (uint32_t)out_rows; a.out_cols = (uint32_t)out_cols;
    a.col_w = tc.tab.as<double>(); a.row_w = a.col_w + out_cols * kLanczosTaps;
    a.col_first = reinterpret_cast<const uint32_t *>(a.col_w + nw); a.col_count = a.col_first + out_cols;
    a.row_first = a.col_count + out_cols; a.row_count = a.row_first + out_rows;
    a.col_taps = ctx->lanczos_col_taps;
    // a tile re-reads the ~6 * ratio source rows of its windows' overhang: bands of at least 16 destination rows where the raster has
    // them, taller ones (up to the LDS row table) once that still leaves about 1024 tiles (4 per compute unit)
    const size_t nstrips = (out_cols + kReadThreads - 1) / kReadThreads;
    a.band_rows = (uint32_t)std::min<size_t>(out_rows, std::min<size_t>(kLanczosMaxBandRows, std::max<size_t>(16, out_rows * nstrips * (size_t)nb / 1024)));
    KernelTimer t(ctx, "read_lanczos");
    HIPCHK(ctx, launch_read_lanczos_u16(a, vec, ctx->stream));
    return SARPRO_HIP_OK;
}

// the pass of `filter` (SARPRO_READ_AVERAGE or SARPRO_READ_LANCZOS)
int read_enqueue(sarpro_hip_ctx *ctx, int filter, const uint16_t *const d_in[], int nb, size_t rows, size_t cols, size_t in_pitch, size_t out_rows,
                 size_t out_cols, float *const d_out[], size_t out_pitch) {
    HIPCHK(ctx, hipSetDevice(ctx->device));
    return (filter == SARPRO_READ_LANCZOS ? lanczos_enqueue : average_enqueue)(ctx, d_in, nb, rows, cols, in_pitch, out_rows, out_cols, d_out, out_pitch);
}

// the argument rules of the two sarpro_hip_read_lanczos_u16 forms beyond shape_ok: nothing is enqueued or written on a refusal
int lanczos_ratio_check(sarpro_hip_ctx *ctx, size_t rows, size_t cols, size_t out_rows, size_t out_cols) {
    const double rx = axis_ratio(cols, out_cols), ry = axis_ratio(rows, out_rows);
    if (rx <= kLanczosMaxRatio && ry <= kLanczosMaxRatio) return SARPRO_HIP_OK;
    char msg[200];
    std::snprintf(msg, sizeof(msg), "read: Lanczos on read is built for per-axis ratios up to 5 (columns %.4f, rows %.4f)", rx, ry);
    return fail(ctx, SARPRO_HIP_ERR_UNSUPPORTED, msg);
}

// the shape of the flow and its filter (*filter: SARPRO_READ_AVERAGE or SARPRO_READ_LANCZOS): DEFAULT follows the rule, AVERAGE is honoured
// at any reduction; Lanczos is refused unless the context's READ_LANCZOS attribute is on, and then taken up to a per-axis ratio of 5
int flow_shape(sarpro_hip_ctx *ctx, size_t rows, size_t cols, int alg, size_t target_size, int pad, size_t *oc, size_t *orows, size_t *fc, size_t *fr,
               int *filter) {
    if (alg != SARPRO_READ_DEFAULT && alg != SARPRO_READ_AVERAGE && alg != SARPRO_READ_LANCZOS) return fail(ctx, SARPRO_HIP_ERR_INVALID_ARG, "bad read filter");
    if (!rows || !cols || !target_size) return fail(ctx, SARPRO_HIP_ERR_INVALID_ARG, "read: rows, cols and target_size must be positive");
    if (rows > kReadMaxDim || cols > kReadMaxDim) return fail(ctx, SARPRO_HIP_ERR_INVALID_ARG, "read: rows and cols up to 2^30");
    int rule = 0;
    read_dims(cols, rows, target_size, oc, orows, &rule);
    *filter = alg == SARPRO_READ_DEFAULT ? rule : alg;
    if (*filter != SARPRO_READ_AVERAGE && ctx->attrs.on(A_READ_LANCZOS)) {
        RETCHK(lanczos_ratio_check(ctx, rows, cols, *orows, *oc));
    } else if (*filter != SARPRO_READ_AVERAGE) {
        char msg[200];
        std::snprintf(msg, sizeof(msg), "read: Lanczos on read is not built (reduction %.4f: the rule picks Average from 4.0; request SARPRO_READ_AVERAGE)",
                      std::max((double)std::max(cols, rows) / (double)target_size, 1.0));
        return fail(ctx, SARPRO_HIP_ERR_UNSUPPORTED, msg);
    }
    return sarpro_hip_resize_output_dims(*oc, *orows, target_size, pad, fc, fr);
}

// device u16 bands -> the RGB raster in device memory (d_rgb: fc * fr * 3 bytes); synchronous (the resized f32 flow is)
int flow_dev(sarpro_hip_ctx *ctx, const uint16_t *const d_bands[2], size_t rows, size_t cols, size_t in_pitch, size_t oc, size_t orows, int filter,
             int strategy, int mode, unsigned flags, size_t target_size, int pad, uint8_t *d_rgb, sarpro_hip_resize_meta *meta) {
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const size_t opitch = round_up(oc, 64);
    float *d_f32[2];
    for (int b = 0; b < 2; ++b) {
        HIPCHK(ctx, ctx->read_band[b].reserve(orows * opitch * sizeof(float)));
        d_f32[b] = ctx->read_band[b].as<float>();
    }
    RETCHK(read_enqueue(ctx, filter, d_bands, 2, rows, cols, in_pitch, orows, oc, d_f32, opitch));
    return sarpro_hip_dualpol_synrgb_resized_f32_dev(ctx, d_f32[0], d_f32[1], orows, oc, opitch, strategy, mode, flags, target_size, pad, d_rgb, meta);
}

// host bands or a reader -> the RGB raster in jpeg_rgb (the raster of the context the encoder reads)
int flow_staged(sarpro_hip_ctx *ctx, const uint16_t *const host[2], sarpro_hip_row_reader reader, void *reader_user, size_t rows, size_t cols, int alg,
                int strategy, int mode, unsigned flags, size_t target_size, int pad, size_t *fc, size_t *fr, sarpro_hip_resize_meta *meta) {
    size_t oc = 0, orows = 0;
    int filter = 0;
    RETCHK(flow_shape(ctx, rows, cols, alg, target_size, pad, &oc, &orows, fc, fr, &filter));
    RETCHK(check_flow(ctx, strategy, mode, flags));
    const size_t pitch = round_up(cols, 64);
    RETCHK(stage_bands(ctx, host, reader, reader_user, rows, cols, pitch));
    HIPCHK(ctx, ctx->jpeg_rgb.reserve(std::max<size_t>(*fc * *fr * 3, 1)));
    const uint16_t *d_bands[2] = {ctx->read_src[0].as<uint16_t>(), ctx->read_src[1].as<uint16_t>()};
    return flow_dev(ctx, d_bands, rows, cols, pitch, oc, orows, filter, strategy, mode, flags, target_size, pad, ctx->jpeg_rgb.as<uint8_t>(), meta);
}

// one band through `filter`: the bodies of sarpro_hip_read_{average,lanczos}_u16_dev ...
int read_dev(sarpro_hip_ctx *ctx, int filter, const uint16_t *d_in, size_t rows, size_t cols, size_t in_pitch, size_t out_rows, size_t out_cols,
             float *d_out_f32, size_t out_pitch) {
    if (!ctx) return SARPRO_HIP_ERR_INVALID_ARG;
    if (!shape_ok(rows, cols, out_rows, out_cols)) return fail(ctx, SARPRO_HIP_ERR_INVALID_ARG, "read: 1 <= out_rows <= rows, 1 <= out_cols <= cols, both up to 2^30");
    if (!d_in || !d_out_f32) return fail(ctx, SARPRO_HIP_ERR_INVALID_ARG, "null raster");
    if (in_pitch < cols || out_pitch < out_cols) return fail(ctx, SARPRO_HIP_ERR_INVALID_ARG, "pitch < cols");
    if (filter == SARPRO_READ_LANCZOS) RETCHK(lanczos_ratio_check(ctx, rows, cols, out_rows, out_cols));
    timing_reset(ctx);
    const uint16_t *in[1] = {d_in};
    float *out[1] = {d_out_f32};
    RETCHK(read_enqueue(ctx, filter, in, 1, rows, cols, in_pitch, out_rows, out_cols, out, out_pitch));
    if (ctx->async_dev) { ctx->async_pending = ctx->timing; return SARPRO_HIP_OK; } // stream-ordered: nothing is read back
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return SARPRO_HIP_OK;
}

// ... and of sarpro_hip_read_{average,lanczos}_u16
int read_host(sarpro_hip_ctx *ctx, int filter, const uint16_t *in, size_t rows, size_t cols, size_t out_rows, size_t out_cols, float *out_f32) {
    if (!ctx) return SARPRO_HIP_ERR_INVALID_ARG;
    if (!shape_ok(rows, cols, out_rows, out_cols)) return fail(ctx, SARPRO_HIP_ERR_INVALID_ARG, "read: 1 <= out_rows <= rows, 1 <= out_cols <= cols, both up to 2^30");
    if (!in || !out_f32) return fail(ctx, SARPRO_HIP_ERR_INVALID_ARG, "null raster");
    if (filter == SARPRO_READ_LANCZOS) RETCHK(lanczos_ratio_check(ctx, rows, cols, out_rows, out_cols));
    timing_reset(ctx);
    size_t pitch = 0;
    RETCHK(stage_in_2d(ctx, ctx->read_src[0], in, rows, cols, 2, &pitch));
    const size_t opitch = round_up(out_cols, 64);
    HIPCHK(ctx, ctx->read_band[0].reserve(out_rows * opitch * sizeof(float)));
    const uint16_t *d_in[1] = {ctx->read_src[0].as<uint16_t>()};
    float *d_out[1] = {ctx->read_band[0].as<float>()};
    RETCHK(read_enqueue(ctx, filter, d_in, 1, rows, cols, pitch, out_rows, out_cols, d_out, opitch));
    return fetch_out_2d(ctx, out_f32, d_out[0], opitch * sizeof(float), out_cols * sizeof(float), out_rows);
}

} // namespace

extern "C" int sarpro_hip_read_output_dims(size_t cols, size_t rows, size_t target_size, size_t *out_cols, size_t *out_rows, int *alg) {
    if (!cols || !rows || !target_size || !out_cols || !out_rows || !alg) return SARPRO_HIP_ERR_INVALID_ARG;
    read_dims(cols, rows, target_size, out_cols, out_rows, alg);
    return SARPRO_HIP_OK;
}

extern "C" int sarpro_hip_host_read_average_axis(size_t n_src, size_t n_dst, uint32_t first[], uint32_t count[], double w_first[], double w_last[],
                                                 double w_sum[]) {
    if (!n_dst || n_dst > n_src || n_src > kReadMaxDim || !first || !count || !w_first || !w_last || !w_sum) return SARPRO_HIP_ERR_INVALID_ARG;
    std::vector<ReadAxis> tab;
    try {
        tab.resize(n_dst);
    } catch (...) { // nothing may unwind across the C ABI
        return SARPRO_HIP_ERR_OOM;
    }
    read_average_axis(n_src, n_dst, tab.data()); // the builder of the device tables itself
    for (size_t j = 0; j < n_dst; ++j) {
        first[j] = tab[j].first; count[j] = tab[j].count;
        w_first[j] = tab[j].w_first; w_last[j] = tab[j].w_last; w_sum[j] = tab[j].w_sum;
    }
    return SARPRO_HIP_OK;
}

extern "C" int sarpro_hip_read_average_u16_dev(sarpro_hip_ctx *ctx, const uint16_t *d_in, size_t rows, size_t cols, size_t in_pitch, size_t out_rows,
                                               size_t out_cols, float *d_out_f32, size_t out_pitch) {
    return read_dev(ctx, SARPRO_READ_AVERAGE, d_in, rows, cols, in_pitch, out_rows, out_cols, d_out_f32, out_pitch);
}

extern "C" int sarpro_hip_read_average_u16(sarpro_hip_ctx *ctx, const uint16_t *in, size_t rows, size_t cols, size_t out_rows, size_t out_cols,
                                           float *out_f32) {
    return read_host(ctx, SARPRO_READ_AVERAGE, in, rows, cols, out_rows, out_cols, out_f32);
}

extern "C" int sarpro_hip_host_read_lanczos_axis(size_t n_src, size_t n_dst, uint32_t first[], uint32_t count[], double weights[]) {
    if (!n_dst || n_dst > n_src || n_src > kReadMaxDim || !first || !count || !weights) return SARPRO_HIP_ERR_INVALID_ARG;
    if (axis_ratio(n_src, n_dst) > kLanczosMaxRatio) return SARPRO_HIP_ERR_INVALID_ARG;
    return read_lanczos_axis(n_src, n_dst, first, count, weights) ? SARPRO_HIP_OK : SARPRO_HIP_ERR_INVALID_ARG; // the builder of the device tables itself
}

extern "C" int sarpro_hip_read_lanczos_u16_dev(sarpro_hip_ctx *ctx, const uint16_t *d_in, size_t rows, size_t cols, size_t in_pitch, size_t out_rows,
                                               size_t out_cols, float *d_out_f32, size_t out_pitch) {
    return read_dev(ctx, SARPRO_READ_LANCZOS, d_in, rows, cols, in_pitch, out_rows, out_cols, d_out_f32, out_pitch);
}

extern "C" int sarpro_hip_read_lanczos_u16(sarpro_hip_ctx *ctx, const uint16_t *in, size_t rows, size_t cols, size_t out_rows, size_t out_cols,
                                           float *out_f32) {
    return read_host(ctx, SARPRO_READ_LANCZOS, in, rows, cols, out_rows, out_cols, out_f32);
}

extern "C" int sarpro_hip_dualpol_synrgb_read_u16_dev(sarpro_hip_ctx *ctx, const uint16_t *d_band1, const uint16_t *d_band2, size_t rows, size_t cols,
                                                      size_t in_pitch, int alg, int strategy, int mode, unsigned flags, size_t target_size, int pad,
                                                      uint8_t *d_rgb_out, sarpro_hip_resize_meta *meta) {
    if (!ctx) return SARPRO_HIP_ERR_INVALID_ARG;
    if (!d_band1 || !d_band2 || !d_rgb_out) return fail(ctx, SARPRO_HIP_ERR_INVALID_ARG, "null raster");
    if (in_pitch < cols) return fail(ctx, SARPRO_HIP_ERR_INVALID_ARG, "pitch < cols");
    size_t oc = 0, orows = 0, fc = 0, fr = 0;
    int filter = 0;
    RETCHK(flow_shape(ctx, rows, cols, alg, target_size, pad, &oc, &orows, &fc, &fr, &filter));
    TimingHold hold(ctx); // last_kernel_times: read_average / read_lanczos and the kernels of the resized f32 flow
    const uint16_t *d_bands[2] = {d_band1, d_band2};
    return flow_dev(ctx, d_bands, rows, cols, in_pitch, oc, orows, filter, strategy, mode, flags, target_size, pad, d_rgb_out, meta);
}

extern "C" int sarpro_hip_dualpol_synrgb_read_u16(sarpro_hip_ctx *ctx, const uint16_t *band1, const uint16_t *band2, size_t rows, size_t cols, int alg,
                                                  int strategy, int mode, unsigned flags, size_t target_size, int pad, uint8_t *rgb_out,
                                                  sarpro_hip_resize_meta *meta) {
    if (!ctx) return SARPRO_HIP_ERR_INVALID_ARG;
    if (!band1 || !band2 || !rgb_out) return fail(ctx, SARPRO_HIP_ERR_INVALID_ARG, "null raster");
    TimingHold hold(ctx);
    const uint16_t *host[2] = {band1, band2};
    size_t fc = 0, fr = 0;
    RETCHK(flow_staged(ctx, host, nullptr, nullptr, rows, cols, alg, strategy, mode, flags, target_size, pad, &fc, &fr, meta));
    return rgb_to_host(ctx, rgb_out, fc * fr * 3);
}

extern "C" int sarpro_hip_dualpol_synrgb_read_stream_u16(sarpro_hip_ctx *ctx, sarpro_hip_row_reader reader, void *reader_user, size_t rows, size_t cols,
                                                         int alg, int strategy, int mode, unsigned flags, size_t target_size, int pad, uint8_t *rgb_out,
                                                         sarpro_hip_resize_meta *meta) {
    if (!ctx) return SARPRO_HIP_ERR_INVALID_ARG;
    if (!reader || !rgb_out) return fail(ctx, SARPRO_HIP_ERR_INVALID_ARG, "null reader / raster");
    TimingHold hold(ctx);
    const uint16_t *none[2] = {nullptr, nullptr};
    size_t fc = 0, fr = 0;
    RETCHK(flow_staged(ctx, none, reader, reader_user, rows, cols, alg, strategy, mode, flags, target_size, pad, &fc, &fr, meta));
    return rgb_to_host(ctx, rgb_out, fc * fr * 3);
}

extern "C" int sarpro_hip_dualpol_synrgb_read_stream_u16_jpeg(sarpro_hip_ctx *ctx, sarpro_hip_row_reader reader, void *reader_user, size_t rows,
                                                              size_t cols, int alg, int strategy, int mode, unsigned flags, size_t target_size, int pad,
                                                              uint8_t *jpeg_out, size_t jpeg_capacity, size_t *jpeg_bytes_out, unsigned restart_mcus,
                                                              sarpro_hip_resize_meta *meta) {
    if (!ctx) return SARPRO_HIP_ERR_INVALID_ARG;
    if (!reader || !jpeg_bytes_out || (!jpeg_out && jpeg_capacity)) return fail(ctx, SARPRO_HIP_ERR_INVALID_ARG, "null reader / buffer");
    size_t oc = 0, orows = 0, fc = 0, fr = 0;
    int filter = 0;
    RETCHK(flow_shape(ctx, rows, cols, alg, target_size, pad, &oc, &orows, &fc, &fr, &filter)); // (before the scene crosses PCIe)
    if (!fc || !fr || fc > 65535 || fr > 65535 || restart_mcus > 65535) return fail(ctx, SARPRO_HIP_ERR_INVALID_ARG, "jpeg: final cols and rows 1..65535, restart interval 0..65535");
    TimingHold hold(ctx); // last_kernel_times: the read filter, the flow's kernels and the encoder's
    const uint16_t *none[2] = {nullptr, nullptr};
    RETCHK(flow_staged(ctx, none, reader, reader_user, rows, cols, alg, strategy, mode, flags, target_size, pad, &fc, &fr, meta));
    return jpeg_encode_to_host(ctx, ctx->jpeg_rgb.as<uint8_t>(), fc, fr, fc * 3, 3, restart_mcus, jpeg_out, jpeg_capacity, jpeg_bytes_out);
}
