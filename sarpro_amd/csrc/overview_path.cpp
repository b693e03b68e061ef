// overview_path.cpp -- overview pyramids of interleaved u8 / u16 rasters (overview_kernels.hip) and the product as a tiled GeoTIFF
// with overviews.  The reference's roadmap names the step (Phase 2, "COG + overviews": TILED=YES, 512 or 256 blocks, BuildOverviews
// with AVERAGE) and ships none of it, so the definition is this project's own (include/sarpro_hip.h), restated in
// tests/overviewref.py: the aligned 2 x 2 cascade over the rounded previous level, edges clipped, round half up in integer
// arithmetic.  Parity with GDAL's AVERAGE overviews is unpinned (GDAL is absent and takes fractional source windows at odd sizes).
// Here: the plan of the packed buffer, the same definition on the host, the device pass (ceil(levels / OVR_DEPTH) launches of one
// kernel; OVR_DEPTH 1..6, 2 unless set), the flow "two u16 bands in, RGB and its pyramid out" and the file flow that ends in sarpro_hip_tiff_create_pyramid.
#include <algorithm>
#include <cstdint>
#include <cstring>

#include "api_common.h"
#include "internal.h"
#include "overview_kernels.h"

using namespace sarpro;

namespace {

bool raster_ok(size_t cols, size_t rows, int components, int bits) {
    return cols && rows && cols <= kOvrMaxDim && rows <= kOvrMaxDim && components >= 1 && components <= 3 && (bits == 8 || bits == 16);
}

// the plan is one of this raster: the cascade's shapes, rows that fit their pitch, levels in ascending order that do not overlap
bool plan_ok(const sarpro_hip_ovr_plan *p, size_t cols, size_t rows, int components, int bits) {
    if (!p || p->levels < 0 || p->levels > SARPRO_HIP_OVR_MAX_LEVELS || p->components != components || p->bits != bits) return false;
    const size_t bps = (size_t)bits / 8;
    size_t w = cols, h = rows, end = 0;
    for (int k = 0; k < p->levels; ++k) {
        w = (w + 1) / 2; h = (h + 1) / 2;
        if (p->cols[k] != w || p->rows[k] != h || p->pitch_bytes[k] < w * (size_t)components * bps) return false;
        if (p->pitch_bytes[k] % bps || p->offset_bytes[k] % bps || p->offset_bytes[k] < end) return false;
        end = p->offset_bytes[k] + h * p->pitch_bytes[k];
    }
    return end <= p->total_bytes;
}

template <typename T>
void host_level(const T *in, size_t in_pitch_bytes, size_t pw, size_t ph, int C, bool skip, T *out, size_t out_pitch_bytes) {
    const size_t nw = (pw + 1) / 2, nh = (ph + 1) / 2;
    for (size_t i = 0; i < nh; ++i) {
        T *o = reinterpret_cast<T *>(reinterpret_cast<uint8_t *>(out) + i * out_pitch_bytes);
        for (size_t j = 0; j < nw; ++j) {
            uint32_t sum[3] = {0, 0, 0}, n = 0;
            for (size_t y = 2 * i; y < std::min(2 * i + 2, ph); ++y) {
                const T *s = reinterpret_cast<const T *>(reinterpret_cast<const uint8_t *>(in) + y * in_pitch_bytes);
                for (size_t x = 2 * j; x < std::min(2 * j + 2, pw); ++x) {
                    uint32_t any = 0;
                    for (int c = 0; c < C; ++c) any |= s[x * C + c];
                    if (skip && !any) continue;
                    for (int c = 0; c < C; ++c) sum[c] += s[x * C + c];
                    ++n;
                }
            }
            for (int c = 0; c < C; ++c) o[j * C + c] = (T)ovr_round(sum[c], n);
        }
    }
}

// The launches of a pyramid, enqueued on the context's stream: levels 1..depth from the source, then further launches of the same
// kernel on the deepest level written so far.
int overviews_enqueue(sarpro_hip_ctx *ctx, const void *d_src, size_t cols, size_t rows, size_t pitch_bytes, int components, int bits, unsigned flags,
                      const sarpro_hip_ovr_plan *plan, void *d_out) {
    HIPCHK(ctx, hipSetDevice(ctx->device));
    // 2 levels per launch unless OVR_DEPTH says otherwise: measured on the 20000^2 RGB raster, 1 and 2 tie at 0.58 ms, 3
    // takes 0.69 and 6 takes 1.01 -- a tile's deep levels occupy 16, 4 and 1 of its 256 lanes between barriers -- and 2 halves the launches
    const long long depth_attr = ctx->attrs.val(A_OVR_DEPTH, kOvrDefaultDepth);
    const int depth = (int)std::min<long long>(kOvrMaxDepth, std::max<long long>(1, depth_attr));
    const uint8_t *src = static_cast<const uint8_t *>(d_src);
    uint8_t *out = static_cast<uint8_t *>(d_out);
    size_t w = cols, h = rows, sp = pitch_bytes;
    for (int done = 0; done < plan->levels;) {
        OvrArgs a{};
        a.src = src; a.src_pitch = sp; a.cols = (uint32_t)w; a.rows = (uint32_t)h;
        a.depth = (uint32_t)std::min(depth, plan->levels - done);
        a.skip_zero = (flags & SARPRO_HIP_OVR_SKIP_ZERO) ? 1u : 0u;
        for (uint32_t k = 0; k < a.depth; ++k) {
            a.dst[k] = out + plan->offset_bytes[done + k];
            a.dst_pitch[k] = plan->pitch_bytes[done + k];
        }
        const bool vec = reinterpret_cast<uintptr_t>(src) % 16 == 0 && sp % 16 == 0;
        {
            KernelTimer t(ctx, "overviews");
            // up to 8 workgroups per compute unit walk the tiles (33 KB of LDS at most: 4 resident for u16 x 3, 8 for the narrower types)
            HIPCHK(ctx, launch_overviews(a, bits, components, vec, (unsigned)std::max(1, ctx->cu_count) * 8u, ctx->stream));
        }
        done += (int)a.depth;
        src = out + plan->offset_bytes[done - 1]; sp = plan->pitch_bytes[done - 1];
        w = plan->cols[done - 1]; h = plan->rows[done - 1];
    }
    return SARPRO_HIP_OK;
}

int check_call(sarpro_hip_ctx *ctx, const void *src, size_t cols, size_t rows, size_t pitch_bytes, int components, int bits, unsigned flags,
               const sarpro_hip_ovr_plan *plan, const void *out) {
    if (!raster_ok(cols, rows, components, bits)) return fail(ctx, SARPRO_HIP_ERR_INVALID_ARG, "overviews: cols and rows 1..2^30, components 1..3, bits 8 or 16");
    if (flags & ~SARPRO_HIP_OVR_SKIP_ZERO) return fail(ctx, SARPRO_HIP_ERR_INVALID_ARG, "overviews: unknown flag");
    if (!plan_ok(plan, cols, rows, components, bits)) return fail(ctx, SARPRO_HIP_ERR_INVALID_ARG, "overviews: the plan is not one of this raster");
    const size_t bps = (size_t)bits / 8;
    if (pitch_bytes < cols * (size_t)components * bps || pitch_bytes % bps) return fail(ctx, SARPRO_HIP_ERR_INVALID_ARG, "overviews: pitch_bytes < row bytes, or no multiple of the sample size");
    if (!src || (!out && plan->levels)) return fail(ctx, SARPRO_HIP_ERR_INVALID_ARG, "null raster");
    if (reinterpret_cast<uintptr_t>(src) % bps || reinterpret_cast<uintptr_t>(out) % bps) return fail(ctx, SARPRO_HIP_ERR_INVALID_ARG, "overviews: rasters must be aligned to their sample size");
    return SARPRO_HIP_OK;
}

} // namespace

extern "C" int sarpro_hip_overview_plan(size_t cols, size_t rows, int components, int bits, size_t min_size, sarpro_hip_ovr_plan *out) {
    if (!out || !raster_ok(cols, rows, components, bits)) return SARPRO_HIP_ERR_INVALID_ARG;
    if (!min_size) min_size = 512;
    std::memset(out, 0, sizeof(*out));
    out->components = components; out->bits = bits;
    const size_t px = (size_t)components * ((size_t)bits / 8);
    size_t w = cols, h = rows, off = 0;
    int L = 0;
    while (std::max(w, h) > min_size && L < SARPRO_HIP_OVR_MAX_LEVELS) {
        w = (w + 1) / 2; h = (h + 1) / 2;
        out->cols[L] = w; out->rows[L] = h;
        out->pitch_bytes[L] = (w * px + 15) / 16 * 16;
        out->offset_bytes[L] = off;
        off = (off + h * out->pitch_bytes[L] + 255) / 256 * 256;
        ++L;
    }
    out->levels = L;
    out->total_bytes = L ? out->offset_bytes[L - 1] + out->rows[L - 1] * out->pitch_bytes[L - 1] : 0;
    return L;
}

extern "C" int sarpro_hip_host_overviews(const void *src, size_t cols, size_t rows, size_t pitch_bytes, int components, int bits, unsigned flags,
                                         const sarpro_hip_ovr_plan *plan, void *out) {
    if (check_call(nullptr, src, cols, rows, pitch_bytes, components, bits, flags, plan, out) != SARPRO_HIP_OK) return SARPRO_HIP_ERR_INVALID_ARG;
    const bool skip = (flags & SARPRO_HIP_OVR_SKIP_ZERO) != 0;
    const uint8_t *in = static_cast<const uint8_t *>(src);
    size_t w = cols, h = rows, ip = pitch_bytes;
    for (int k = 0; k < plan->levels; ++k) {
        uint8_t *o = static_cast<uint8_t *>(out) + plan->offset_bytes[k];
        if (bits == 8) host_level<uint8_t>(in, ip, w, h, components, skip, o, plan->pitch_bytes[k]);
        else host_level<uint16_t>(reinterpret_cast<const uint16_t *>(in), ip, w, h, components, skip, reinterpret_cast<uint16_t *>(o), plan->pitch_bytes[k]);
        in = o; ip = plan->pitch_bytes[k]; w = plan->cols[k]; h = plan->rows[k];
    }
    return SARPRO_HIP_OK;
}

extern "C" int sarpro_hip_overviews_dev(sarpro_hip_ctx *ctx, const void *d_src, size_t cols, size_t rows, size_t pitch_bytes, int components, int bits,
                                        unsigned flags, const sarpro_hip_ovr_plan *plan, void *d_out) {
    if (!ctx) return SARPRO_HIP_ERR_INVALID_ARG;
    RETCHK(check_call(ctx, d_src, cols, rows, pitch_bytes, components, bits, flags, plan, d_out));
    timing_reset(ctx);
    if (!plan->levels) return SARPRO_HIP_OK;
    RETCHK(overviews_enqueue(ctx, d_src, cols, rows, pitch_bytes, components, bits, flags, plan, d_out));
    if (ctx->async_dev) { ctx->async_pending = ctx->timing; return SARPRO_HIP_OK; } // stream-ordered: nothing is read back
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return SARPRO_HIP_OK;
}

extern "C" int sarpro_hip_overviews(sarpro_hip_ctx *ctx, const void *src, size_t cols, size_t rows, int components, int bits, unsigned flags,
                                    const sarpro_hip_ovr_plan *plan, void *out) {
    if (!ctx) return SARPRO_HIP_ERR_INVALID_ARG;
    const size_t row_bytes = cols * (size_t)(components > 0 ? components : 1) * (size_t)(bits == 16 ? 2 : 1);
    RETCHK(check_call(ctx, src, cols, rows, row_bytes, components, bits, flags, plan, out));
    timing_reset(ctx);
    if (!plan->levels) return SARPRO_HIP_OK;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const size_t pitch = round_up(row_bytes, 16);
    HIPCHK(ctx, ctx->ovr_src.reserve(rows * pitch));
    HIPCHK(ctx, ctx->ovr_out.reserve(plan->total_bytes));
    HIPCHK(ctx, hipMemcpy2DAsync(ctx->ovr_src.p, pitch, src, row_bytes, row_bytes, rows, hipMemcpyHostToDevice, ctx->stream));
    RETCHK(overviews_enqueue(ctx, ctx->ovr_src.p, cols, rows, pitch, components, bits, flags, plan, ctx->ovr_out.p));
    const size_t bps = (size_t)bits / 8;
    for (int k = 0; k < plan->levels; ++k) { // the rows alone: the caller's padding keeps its bytes
        const size_t rb = plan->cols[k] * (size_t)components * bps;
        HIPCHK(ctx, hipMemcpy2DAsync(static_cast<uint8_t *>(out) + plan->offset_bytes[k], plan->pitch_bytes[k], ctx->ovr_out.as<uint8_t>() + plan->offset_bytes[k],
                                     plan->pitch_bytes[k], rb, plan->rows[k], hipMemcpyDeviceToHost, ctx->stream));
    }
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return SARPRO_HIP_OK;
}

extern "C" int sarpro_hip_dualpol_synrgb_pyramid_u16_dev(sarpro_hip_ctx *ctx, const uint16_t *d_band1, const uint16_t *d_band2, size_t rows, size_t cols,
                                                         size_t in_pitch, int strategy, int mode, uint8_t *d_rgb, size_t rgb_pitch_px,
                                                         sarpro_hip_stats *stats_out, unsigned ovr_flags, const sarpro_hip_ovr_plan *plan, void *d_ovr_out) {
    if (!ctx) return SARPRO_HIP_ERR_INVALID_ARG;
    if (rgb_pitch_px < cols) return fail(ctx, SARPRO_HIP_ERR_INVALID_ARG, "rgb_pitch_px < cols");
    RETCHK(check_call(ctx, d_rgb, cols, rows, rgb_pitch_px * 3, 3, 8, ovr_flags, plan, d_ovr_out)); // (before anything is enqueued)
    TimingHold hold(ctx); // last_kernel_times: the chain's kernels, then "overviews"
    // The device-resident chain leaves its final read-back enqueued (context.h: defer_chain_tail), the sweep goes behind it on the same
    // stream, and ONE synchronisation ends the call: no host synchronisation between the two.  (A route that is orchestrated from the
    // host -- NO_CHAIN, a shape the chain does not take -- synchronises inside itself as it always does.)
    ctx->deferred_tail = sarpro_hip_ctx::DeferredTail();
    ctx->defer_chain_tail = true;
    int rc = sarpro_hip_dualpol_synrgb_u16_dev(ctx, d_band1, d_band2, rows, cols, in_pitch, strategy, mode, d_rgb, rgb_pitch_px, nullptr, nullptr, 0, stats_out);
    ctx->defer_chain_tail = false;
    if (rc == SARPRO_HIP_OK && plan->levels) rc = overviews_enqueue(ctx, d_rgb, cols, rows, rgb_pitch_px * 3, 3, 8, ovr_flags, plan, d_ovr_out);
    if (ctx->deferred_tail.kind) { // (also behind a failed enqueue: the tail's copy is in flight)
        const int frc = chain_deferred_tail_finish(ctx);
        return rc != SARPRO_HIP_OK ? rc : frc;
    }
    RETCHK(rc);
    if (!plan->levels) return SARPRO_HIP_OK;
    if (ctx->async_dev) { ctx->async_pending = ctx->timing; return SARPRO_HIP_OK; }
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return SARPRO_HIP_OK;
}

namespace {

// A level (pitched, in device memory) into the file through two pinned slots in row chunks: the copy of chunk k + 1 crosses PCIe while
// chunk k is scattered into its tiles.
int level_to_file(sarpro_hip_ctx *ctx, sarpro_hip_tiff_writer *w, int level, const uint8_t *d, size_t pitch, size_t row_bytes, size_t rows,
                  hipEvent_t evt[2]) {
    const size_t chunk_rows = std::max<size_t>(1, std::min<size_t>(rows, (16u << 20) / row_bytes));
    HIPCHK(ctx, ctx->ovr_host.reserve(2 * chunk_rows * row_bytes));
    uint8_t *slot[2] = {ctx->ovr_host.as<uint8_t>(), ctx->ovr_host.as<uint8_t>() + chunk_rows * row_bytes};
    const size_t nchunks = (rows + chunk_rows - 1) / chunk_rows;
    auto enqueue = [&](size_t k) -> int {
        const size_t r0 = k * chunk_rows, n = std::min(chunk_rows, rows - r0);
        HIPCHK(ctx, hipMemcpy2DAsync(slot[k & 1], row_bytes, d + r0 * pitch, pitch, row_bytes, n, hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(ctx, hipEventRecord(evt[k & 1], ctx->stream));
        return SARPRO_HIP_OK;
    };
    RETCHK(enqueue(0));
    for (size_t k = 0; k < nchunks; ++k) {
        HIPCHK(ctx, hipEventSynchronize(evt[k & 1]));
        if (k + 1 < nchunks) RETCHK(enqueue(k + 1));
        const size_t r0 = k * chunk_rows, n = std::min(chunk_rows, rows - r0);
        HostTimer t(ctx, "host:sink");
        if (int rc = sarpro_hip_tiff_write_level_rows(w, level, r0, n, slot[k & 1], row_bytes)) {
            (void)hipStreamSynchronize(ctx->stream);
            ctx->err = std::string("tiled TIFF writer failed: ") + sarpro_hip_tiff_last_error();
            return rc;
        }
    }
    return SARPRO_HIP_OK;
}

} // namespace

extern "C" int sarpro_hip_dualpol_synrgb_stream_u16_cog(sarpro_hip_ctx *ctx, sarpro_hip_row_reader reader, void *reader_user, size_t rows, size_t cols,
                                                        int strategy, int mode, unsigned ovr_flags, uint32_t tile, size_t min_size, const char *path,
                                                        const double *geotransform6, const sarpro_hip_tiff *geo_keys_from, sarpro_hip_stats *stats_out) {
    if (!ctx) return SARPRO_HIP_ERR_INVALID_ARG;
    if (!reader || !path) return fail(ctx, SARPRO_HIP_ERR_INVALID_ARG, "null reader / path");
    if (strategy < 0 || strategy > SARPRO_STRATEGY_DEFAULT) return fail(ctx, SARPRO_HIP_ERR_INVALID_ARG, "bad strategy");
    if (mode < 0 || mode > SARPRO_SYNRGB_ENHANCED) return fail(ctx, SARPRO_HIP_ERR_INVALID_ARG, "bad synrgb mode");
    if (ovr_flags & ~SARPRO_HIP_OVR_SKIP_ZERO) return fail(ctx, SARPRO_HIP_ERR_INVALID_ARG, "overviews: unknown flag");
    if (tile % 16) return fail(ctx, SARPRO_HIP_ERR_INVALID_ARG, "tile must be a multiple of 16 (0: 512)");
    sarpro_hip_ovr_plan plan;
    if (sarpro_hip_overview_plan(cols, rows, 3, 8, min_size, &plan) < 0) return fail(ctx, SARPRO_HIP_ERR_INVALID_ARG, "cols and rows 1..2^30");
    TimingHold hold(ctx); // last_kernel_times: the chain's kernels, "overviews" and the host segments of the reader and the writer
    const size_t pitch = round_up(cols, 64);
    const uint16_t *none[2] = {nullptr, nullptr};
    RETCHK(stage_bands(ctx, none, reader, reader_user, rows, cols, pitch));
    HIPCHK(ctx, ctx->jpeg_rgb.reserve(rows * pitch * 3));
    HIPCHK(ctx, ctx->ovr_out.reserve(std::max<size_t>(plan.total_bytes, 1)));
    uint8_t *d_rgb = ctx->jpeg_rgb.as<uint8_t>();
    RETCHK(sarpro_hip_dualpol_synrgb_pyramid_u16_dev(ctx, ctx->read_src[0].as<uint16_t>(), ctx->read_src[1].as<uint16_t>(), rows, cols, pitch, strategy, mode,
                                                     d_rgb, pitch, stats_out, ovr_flags, &plan, ctx->ovr_out.p));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream)); // (a stream-ordered context returns from the call above once it is enqueued)
    sarpro_hip_tiff_writer *w = nullptr;
    if (int rc = sarpro_hip_tiff_create_pyramid(path, cols, rows, 3, 8, tile, plan.levels, geotransform6, geo_keys_from, &w)) {
        ctx->err = std::string("tiled TIFF writer failed: ") + sarpro_hip_tiff_last_error();
        return rc;
    }
    hipEvent_t evt[2] = {nullptr, nullptr};
    int rc = SARPRO_HIP_OK;
    for (hipEvent_t &e : evt)
        if (rc == SARPRO_HIP_OK && hipEventCreateWithFlags(&e, hipEventDisableTiming) != hipSuccess) rc = fail(ctx, SARPRO_HIP_ERR_HIP, "hipEventCreateWithFlags failed");
    for (int k = plan.levels; k >= 1 && rc == SARPRO_HIP_OK; --k) // the file's order: the smallest level first
        rc = level_to_file(ctx, w, k, ctx->ovr_out.as<uint8_t>() + plan.offset_bytes[k - 1], plan.pitch_bytes[k - 1], plan.cols[k - 1] * 3, plan.rows[k - 1], evt);
    if (rc == SARPRO_HIP_OK) rc = level_to_file(ctx, w, 0, d_rgb, pitch * 3, cols * 3, rows, evt);
    for (hipEvent_t e : evt)
        if (e) (void)hipEventDestroy(e);
    const int frc = sarpro_hip_tiff_finish(w); // (closes the file and frees the writer on every path)
    if (rc == SARPRO_HIP_OK && frc != SARPRO_HIP_OK) {
        ctx->err = std::string("tiled TIFF writer failed: ") + sarpro_hip_tiff_last_error();
        rc = frc;
    }
    return rc;
}
