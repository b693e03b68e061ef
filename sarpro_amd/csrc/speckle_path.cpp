// speckle_path.cpp -- speckle filtering of u16 and f32 bands into f32 rasters on the device (speckle_kernels.hip): Lee and Kuan
// (windows 3, 5, 7), and through the _ext entry points also Frost (windows 3, 5, 7) and Refined Lee (window 7) over u16 bands; and the
// flows "two u16 bands in, filtered, quicklook RGB out".  The definitions are this project's own (DESIGN.md 9c and 9e,
// include/sarpro_hip.h): the reference's roadmap names the filters (Phase 4: Lee, Kuan, Frost, Refined Lee, before autoscale) and ships
// none, so there is no parity target beyond the numpy restatements in tests/speckleref.py and tests/speckleextref.py.  A caller of the
// reference would place the call between the band read and process_scalar_data_pipeline.
#include <algorithm>
#include <cmath>
#include <cstdint>

#include "api_common.h"
#include "internal.h"
#include "speckle_kernels.h"

using namespace sarpro;

namespace {

// the filter and its parameters.  ext: a call through an _ext entry point, which knows all four filters; the others know Lee and Kuan
struct Filter {
    int filter, window;
    double looks, damping;
    bool ext;
};

// everything but the rasters; nothing is written when it fails
int check_params(sarpro_hip_ctx *ctx, size_t rows, size_t cols, const Filter &f) {
    const bool frost = f.ext && f.filter == SARPRO_SPECKLE_FROST, refined = f.ext && f.filter == SARPRO_SPECKLE_REFINED_LEE;
    if (f.filter != SARPRO_SPECKLE_LEE && f.filter != SARPRO_SPECKLE_KUAN && !frost && !refined) return fail(ctx, SARPRO_HIP_ERR_INVALID_ARG, "speckle: bad filter");
    if (refined && f.window != 7) return fail(ctx, SARPRO_HIP_ERR_INVALID_ARG, "speckle: Refined Lee has a window of 7");
    if (f.window != 3 && f.window != 5 && f.window != 7) return fail(ctx, SARPRO_HIP_ERR_INVALID_ARG, "speckle: window must be 3, 5 or 7");
    if (frost) { // looks is ignored
        if (!std::isfinite(f.damping) || !(f.damping > 0.0)) return fail(ctx, SARPRO_HIP_ERR_INVALID_ARG, "speckle: damping must be finite and positive");
    } else if (!std::isfinite(f.looks) || !(f.looks > 0.0)) { // damping is ignored
        return fail(ctx, SARPRO_HIP_ERR_INVALID_ARG, "speckle: looks must be finite and positive");
    }
    if (!rows || !cols) return fail(ctx, SARPRO_HIP_ERR_INVALID_ARG, "speckle: empty raster");
    if (rows > kSpeckleMaxDim || cols > kSpeckleMaxDim) return fail(ctx, SARPRO_HIP_ERR_INVALID_ARG, "speckle: rows and cols up to 2^30");
    return SARPRO_HIP_OK;
}

// The pass over nb bands of one shape, enqueued on the context's stream.
int speckle_enqueue(sarpro_hip_ctx *ctx, bool f32, const void *const d_in[], int nb, size_t rows, size_t cols, size_t in_pitch, const Filter &f,
                    float *const d_out[], size_t out_pitch) {
    HIPCHK(ctx, hipSetDevice(ctx->device));
    SpeckleArgs a{};
    const bool vec = band_rasters(a.io, d_in, nb, in_pitch, d_out, out_pitch);
    a.rows = (uint32_t)rows; a.cols = (uint32_t)cols;
    const bool frost = f.filter == SARPRO_SPECKLE_FROST, refined = f.filter == SARPRO_SPECKLE_REFINED_LEE;
    a.cu2 = frost ? 0.0 : 1.0 / f.looks;
    a.g = f.filter == SARPRO_SPECKLE_KUAN ? 1.0 / (1.0 + a.cu2) : 1.0;
    a.thr = sarpro_hip_host_f32_valid_threshold();
    // u16: about 1024 tiles for a small raster (4 per compute unit) with bands of at least 16 rows; bands of 128 rows (k - 1 halo rows
    // each: 5 % more rows read at k = 7) for a large one
    const size_t nstrips = (cols + kSpeckleThreads - 1) / kSpeckleThreads;
    a.band_rows = f32 ? kSpeckleF32BandRows : (uint32_t)std::min<size_t>(kSpeckleMaxBandRows, std::max<size_t>(16, rows * nstrips * (size_t)nb / 1024));
    if (frost || refined) { // (u16 only: check_params admits these filters through the _ext entry points alone, and those take u16 bands)
        SpeckleExtArgs xa{};
        xa.base = a;
        xa.damping = frost ? f.damping : 0.0;
        static const int kR2[kFrostMaxClasses] = {0, 1, 2, 4, 5, 8, 9, 10, 13, 18};
        for (uint32_t c = 0; c < kFrostMaxClasses; ++c) xa.dist[c] = std::sqrt((double)kR2[c]);
        KernelTimer t(ctx, frost ? "speckle_frost_u16" : "speckle_rlee_u16");
        HIPCHK(ctx, launch_speckle_ext_u16(xa, refined, f.window, vec, ctx->stream));
        return SARPRO_HIP_OK;
    }
    {
        KernelTimer t(ctx, f32 ? "speckle_f32" : "speckle_u16");
        HIPCHK(ctx, f32 ? launch_speckle_f32(a, f.window, ctx->stream) : launch_speckle_u16(a, f.window, vec, ctx->stream));
    }
    return SARPRO_HIP_OK;
}

int speckle_dev(sarpro_hip_ctx *ctx, bool f32, const void *d_in, size_t rows, size_t cols, size_t in_pitch, const Filter &f, float *d_out,
                size_t out_pitch) {
    if (!ctx) return SARPRO_HIP_ERR_INVALID_ARG;
    RETCHK(check_params(ctx, rows, cols, f));
    if (!d_in || !d_out) return fail(ctx, SARPRO_HIP_ERR_INVALID_ARG, "null raster");
    if (in_pitch < cols || out_pitch < cols) return fail(ctx, SARPRO_HIP_ERR_INVALID_ARG, "pitch < cols");
    if (f32) { // a window reads its neighbours' inputs: the rasters may not overlap
        const uintptr_t i0 = reinterpret_cast<uintptr_t>(d_in), i1 = i0 + ((rows - 1) * in_pitch + cols) * sizeof(float);
        const uintptr_t o0 = reinterpret_cast<uintptr_t>(d_out), o1 = o0 + ((rows - 1) * out_pitch + cols) * sizeof(float);
        if (i0 < o1 && o0 < i1) return fail(ctx, SARPRO_HIP_ERR_INVALID_ARG, "speckle: the output raster may not alias the input");
    }
    timing_reset(ctx);
    const void *in[1] = {d_in};
    float *out[1] = {d_out};
    RETCHK(speckle_enqueue(ctx, f32, in, 1, rows, cols, in_pitch, f, out, out_pitch));
    if (ctx->async_dev) { ctx->async_pending = ctx->timing; return SARPRO_HIP_OK; } // stream-ordered: nothing is read back
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return SARPRO_HIP_OK;
}

int speckle_host(sarpro_hip_ctx *ctx, bool f32, const void *in, size_t rows, size_t cols, const Filter &f, float *out) {
    if (!ctx) return SARPRO_HIP_ERR_INVALID_ARG;
    RETCHK(check_params(ctx, rows, cols, f));
    if (!in || !out) return fail(ctx, SARPRO_HIP_ERR_INVALID_ARG, "null raster");
    timing_reset(ctx);
    size_t pitch = 0;
    RETCHK(stage_in_2d(ctx, ctx->read_src[0], in, rows, cols, f32 ? 4 : 2, &pitch));
    const size_t opitch = round_up(cols, 64);
    HIPCHK(ctx, ctx->speckle_band[0].reserve(rows * opitch * sizeof(float)));
    const void *d_in[1] = {ctx->read_src[0].p};
    float *d_out[1] = {ctx->speckle_band[0].as<float>()};
    RETCHK(speckle_enqueue(ctx, f32, d_in, 1, rows, cols, pitch, f, d_out, opitch));
    return fetch_out_2d(ctx, out, d_out[0], opitch * sizeof(float), cols * sizeof(float), rows);
}

// device u16 bands -> both filtered in one launch into f32 rasters of the context -> the resized f32 flow, unchanged (target_size 0:
// that flow's native size); synchronous, as that flow is
int flow_dev(sarpro_hip_ctx *ctx, const uint16_t *const d_bands[2], size_t rows, size_t cols, size_t in_pitch, const Filter &f, int strategy,
             int mode, unsigned flags, size_t target_size, int pad, uint8_t *d_rgb, sarpro_hip_resize_meta *meta) {
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const size_t opitch = round_up(cols, 64);
    float *d_f32[2];
    for (int b = 0; b < 2; ++b) {
        HIPCHK(ctx, ctx->speckle_band[b].reserve(rows * opitch * sizeof(float)));
        d_f32[b] = ctx->speckle_band[b].as<float>();
    }
    const void *in[2] = {d_bands[0], d_bands[1]};
    RETCHK(speckle_enqueue(ctx, false, in, 2, rows, cols, in_pitch, f, d_f32, opitch));
    return sarpro_hip_dualpol_synrgb_resized_f32_dev(ctx, d_f32[0], d_f32[1], rows, cols, opitch, strategy, mode, flags, target_size, pad, d_rgb, meta);
}

int flow_entry_dev(sarpro_hip_ctx *ctx, const uint16_t *d_band1, const uint16_t *d_band2, size_t rows, size_t cols, size_t in_pitch, const Filter &f,
                   int strategy, int mode, unsigned flags, size_t target_size, int pad, uint8_t *d_rgb_out, sarpro_hip_resize_meta *meta) {
    if (!ctx) return SARPRO_HIP_ERR_INVALID_ARG;
    RETCHK(check_params(ctx, rows, cols, f));
    RETCHK(check_flow(ctx, strategy, mode, flags));
    if (!d_band1 || !d_band2 || !d_rgb_out) return fail(ctx, SARPRO_HIP_ERR_INVALID_ARG, "null raster");
    if (in_pitch < cols) return fail(ctx, SARPRO_HIP_ERR_INVALID_ARG, "pitch < cols");
    TimingHold hold(ctx); // last_kernel_times: the filter's kernel and the kernels of the resized f32 flow
    const uint16_t *d_bands[2] = {d_band1, d_band2};
    return flow_dev(ctx, d_bands, rows, cols, in_pitch, f, strategy, mode, flags, target_size, pad, d_rgb_out, meta);
}

int flow_entry_host(sarpro_hip_ctx *ctx, const uint16_t *band1, const uint16_t *band2, size_t rows, size_t cols, const Filter &f, int strategy, int mode,
                    unsigned flags, size_t target_size, int pad, uint8_t *rgb_out, sarpro_hip_resize_meta *meta) {
    if (!ctx) return SARPRO_HIP_ERR_INVALID_ARG;
    RETCHK(check_params(ctx, rows, cols, f));
    RETCHK(check_flow(ctx, strategy, mode, flags));
    if (!band1 || !band2 || !rgb_out) return fail(ctx, SARPRO_HIP_ERR_INVALID_ARG, "null raster");
    size_t fc = 0, fr = 0;
    RETCHK(sarpro_hip_resize_output_dims(cols, rows, target_size, pad, &fc, &fr));
    TimingHold hold(ctx);
    const size_t pitch = round_up(cols, 64);
    const uint16_t *host[2] = {band1, band2};
    RETCHK(stage_bands(ctx, host, nullptr, nullptr, rows, cols, pitch));
    HIPCHK(ctx, ctx->jpeg_rgb.reserve(std::max<size_t>(fc * fr * 3, 1)));
    const uint16_t *d_bands[2] = {ctx->read_src[0].as<uint16_t>(), ctx->read_src[1].as<uint16_t>()};
    RETCHK(flow_dev(ctx, d_bands, rows, cols, pitch, f, strategy, mode, flags, target_size, pad, ctx->jpeg_rgb.as<uint8_t>(), meta));
    return rgb_to_host(ctx, rgb_out, fc * fr * 3);
}

} // namespace

extern "C" int sarpro_hip_speckle_u16_dev(sarpro_hip_ctx *ctx, const uint16_t *d_in, size_t rows, size_t cols, size_t in_pitch, int filter, int window,
                                          double looks, float *d_out_f32, size_t out_pitch) {
    return speckle_dev(ctx, false, d_in, rows, cols, in_pitch, Filter{filter, window, looks, 0.0, false}, d_out_f32, out_pitch);
}

extern "C" int sarpro_hip_speckle_f32_dev(sarpro_hip_ctx *ctx, const float *d_in, size_t rows, size_t cols, size_t in_pitch, int filter, int window,
                                          double looks, float *d_out_f32, size_t out_pitch) {
    return speckle_dev(ctx, true, d_in, rows, cols, in_pitch, Filter{filter, window, looks, 0.0, false}, d_out_f32, out_pitch);
}

extern "C" int sarpro_hip_speckle_u16(sarpro_hip_ctx *ctx, const uint16_t *in, size_t rows, size_t cols, int filter, int window, double looks,
                                      float *out_f32) {
    return speckle_host(ctx, false, in, rows, cols, Filter{filter, window, looks, 0.0, false}, out_f32);
}

extern "C" int sarpro_hip_speckle_f32(sarpro_hip_ctx *ctx, const float *in, size_t rows, size_t cols, int filter, int window, double looks,
                                      float *out_f32) {
    return speckle_host(ctx, true, in, rows, cols, Filter{filter, window, looks, 0.0, false}, out_f32);
}

extern "C" int sarpro_hip_dualpol_synrgb_speckle_u16_dev(sarpro_hip_ctx *ctx, const uint16_t *d_band1, const uint16_t *d_band2, size_t rows, size_t cols,
                                                         size_t in_pitch, int filter, int window, double looks, int strategy, int mode, unsigned flags,
                                                         size_t target_size, int pad, uint8_t *d_rgb_out, sarpro_hip_resize_meta *meta) {
    return flow_entry_dev(ctx, d_band1, d_band2, rows, cols, in_pitch, Filter{filter, window, looks, 0.0, false}, strategy, mode, flags, target_size, pad,
                          d_rgb_out, meta);
}

extern "C" int sarpro_hip_dualpol_synrgb_speckle_u16(sarpro_hip_ctx *ctx, const uint16_t *band1, const uint16_t *band2, size_t rows, size_t cols,
                                                     int filter, int window, double looks, int strategy, int mode, unsigned flags, size_t target_size,
                                                     int pad, uint8_t *rgb_out, sarpro_hip_resize_meta *meta) {
    return flow_entry_host(ctx, band1, band2, rows, cols, Filter{filter, window, looks, 0.0, false}, strategy, mode, flags, target_size, pad, rgb_out, meta);
}

// ---- the _ext entry points: all four filters.  Lee and Kuan take the path above -- the same kernel, the same bits.
extern "C" int sarpro_hip_speckle_ext_u16_dev(sarpro_hip_ctx *ctx, const uint16_t *d_in, size_t rows, size_t cols, size_t in_pitch, int filter, int window,
                                              double looks, double damping, float *d_out_f32, size_t out_pitch) {
    return speckle_dev(ctx, false, d_in, rows, cols, in_pitch, Filter{filter, window, looks, damping, true}, d_out_f32, out_pitch);
}

extern "C" int sarpro_hip_speckle_ext_u16(sarpro_hip_ctx *ctx, const uint16_t *in, size_t rows, size_t cols, int filter, int window, double looks,
                                          double damping, float *out_f32) {
    return speckle_host(ctx, false, in, rows, cols, Filter{filter, window, looks, damping, true}, out_f32);
}

extern "C" int sarpro_hip_dualpol_synrgb_speckle_ext_u16_dev(sarpro_hip_ctx *ctx, const uint16_t *d_band1, const uint16_t *d_band2, size_t rows,
                                                             size_t cols, size_t in_pitch, int filter, int window, double looks, double damping,
                                                             int strategy, int mode, unsigned flags, size_t target_size, int pad, uint8_t *d_rgb_out,
                                                             sarpro_hip_resize_meta *meta) {
    return flow_entry_dev(ctx, d_band1, d_band2, rows, cols, in_pitch, Filter{filter, window, looks, damping, true}, strategy, mode, flags, target_size, pad,
                          d_rgb_out, meta);
}

extern "C" int sarpro_hip_dualpol_synrgb_speckle_ext_u16(sarpro_hip_ctx *ctx, const uint16_t *band1, const uint16_t *band2, size_t rows, size_t cols,
                                                         int filter, int window, double looks, double damping, int strategy, int mode, unsigned flags,
                                                         size_t target_size, int pad, uint8_t *rgb_out, sarpro_hip_resize_meta *meta) {
    return flow_entry_host(ctx, band1, band2, rows, cols, Filter{filter, window, looks, damping, true}, strategy, mode, flags, target_size, pad, rgb_out,
                           meta);
}

// EXP of DESIGN.md 9e on the host: the same source sequence as the kernel's (speckle_kernels.h).  Defined for x <= 0; NaN for a NaN or x > 0.
extern "C" double sarpro_hip_host_speckle_exp(double x) {
    if (!(x <= 0.0)) return std::nan("");
    return speckle_exp(x);
}

