// workspace_layout.h -- what lives where in the context's work buffers of the u16 flavour (and the parts the f32 flavour shares): every
// size and offset once, the proof that the regions fit, and the one place each buffer is reserved.  Host only.
#pragma once
#include "chain_kernels.h"
#include "context.h"

namespace sarpro {
namespace layout {

// ---- device buffers, per band
constexpr size_t kLutBandStride = 131072;            // ctx->luts: one band's DN table, 65536 entries of up to 2 bytes (u8 bins / final values, u16 levels)
constexpr size_t kLutsBytes = kMaxBands * kLutBandStride;
constexpr size_t kTileBinCount = 64 * 256;           // ctx->tile_bins (u64) and ctx->cdfs (f64): kTiles x kTiles tiles of kClaheBins bins per band
constexpr size_t kTileBinsBytes = sizeof(uint64_t) * kTileBinCount * kMaxBands;
constexpr size_t kCdfsBytes = sizeof(double) * kTileBinCount * kMaxBands;
constexpr size_t kLevelHistCount = 256;              // ctx->level_hist (u64): one count per u8 level per band
constexpr size_t kLevelHistBytes = sizeof(uint64_t) * kLevelHistCount * kMaxBands;
// the CLAHE chain's form: [kSampleReplicas][2][256] the apply / sampling pass's histogram (replica 0 alone unless it is sampled), then [2][256] the gated recount
constexpr size_t kLevelHistExactAt = kLevelHistCount * kMaxBands * kSampleReplicas; // (in counts)
constexpr size_t kLevelHistSampledBytes = kLevelHistBytes * (kSampleReplicas + 1);

// ---- ctx->tables
constexpr size_t kComposeBytes = 66048;                      // R[256] | G[256] | blue by pair [65536] (host_logic.h fold_compose_tables)
constexpr size_t kTablesOffMaps = kComposeBytes;             // the two per-band u8 rescale maps [2][256] of the host route's optional band outputs
constexpr size_t kTablesOffPQ = kTablesOffMaps + 512;        // Pv[256] f32 | Qv[256] f32: the blue factors by LEVEL, kept by the device chain
constexpr size_t kTablesHostBytes = kTablesOffPQ;            // what the host routes reserve
constexpr size_t kTablesChainBytes = kTablesOffPQ + 2 * 256 * 4; // what the device chain reserves

// ---- ctx->chain_consts: uploaded once (chain_prepare)
constexpr size_t kChainOffDb = 0;                            // dB of every DN, f64 [65536]
constexpr size_t kChainOffSupp = 65536 * 8;                  // suppressed lut_r | lut_g per floor [42][512] (41 used)
constexpr size_t kChainOffBlue = kChainOffSupp + 21504;      // blue of the suppressed variant by pair [65536]
constexpr size_t kChainOffBlueDef = kChainOffBlue + 65536;   // blue of the default variant by pair [65536]
constexpr size_t kChainOffDefRg = kChainOffBlueDef + 65536;  // default lut_r | lut_g [512]
constexpr size_t kChainOffGamma = kChainOffDefRg + 512;      // gamma level thresholds f64 [3][256]
constexpr size_t kChainOffBluePQ = kChainOffGamma + 3 * 256 * 8; // the suppressed blue's factors P[256] | Q[256] f32
constexpr size_t kChainConstBytes = kChainOffBluePQ + 512 * 4;

// ---- ctx->chain_state
constexpr size_t kStateOffResc = 2 * sizeof(ChainBandState); // behind ChainBandState[2]: the u8 rescale maps [2][256]
constexpr size_t kStateOffIdent = kStateOffResc + 512;       // identity flag per band
constexpr size_t kStateOffFloor = kStateOffIdent + 16;       // the synRGB floor with its cushion (int)
constexpr size_t kStateBytes = kStateOffFloor + 16;

// ---- ctx->h_upload (pinned): what the host routes stage before an upload
constexpr size_t kUploadOffLuts = 0;                         // the bands' DN tables, kLutBandStride apart (u8 tables of the CLAHE bins: 65536 apart)
constexpr size_t kUploadOffCdfs = kLutsBytes;                // the host-built CDFs f64 [2][64][256]
constexpr size_t kUploadOffTables = kUploadOffCdfs + kCdfsBytes; // the composition tables with the per-band maps behind them (as ctx->tables)
constexpr size_t kUploadBytes = kUploadOffTables + kComposeBytes + 1024;
// aliases by design (never live together with what they overlay):
constexpr size_t kUploadOffLevelHist = kUploadOffCdfs;       // percentile strategies: the host's level histogram on its way to the device
constexpr size_t kUploadOffFlatTables = 0;                   // the composition tables of a flat product and of the f32 flow; the single band's rescale map
static_assert(kUploadOffTables + kTablesHostBytes <= kUploadBytes, "h_upload: the tables and their maps fit");
static_assert(kUploadOffLevelHist + kLevelHistBytes <= kUploadOffTables, "h_upload: the level histogram stays inside the CDF region");
static_assert(kUploadOffFlatTables + kComposeBytes <= kUploadOffCdfs, "h_upload: the flat tables stay inside the DN-table region");

// ---- ctx->h_small (pinned): what comes back from the device
constexpr size_t kSmallOffTileBins = 0;                      // the host route's tile-bin histograms u64 [2][64][256]
constexpr size_t kSmallOffLevelHist = kTileBinsBytes;        // ... and its level histograms u64 [2][256]
constexpr size_t kSmallBytes = kSmallOffLevelHist + kLevelHistBytes; // the u16 flavour's size
// aliases at offset 0 by design (one call has one of them in flight): ChainBandState[2] of a device chain's tail; the f32 flavour's
// partials (at most kSmallF32MaxPartials), counts, histograms and, in a stripe, the ranks' gathered partials
constexpr size_t kSmallF32MaxPartials = 2048, kSmallF32PartialBytes = 32;
constexpr size_t kSmallOffF32Direct = 64 * 1024;             // f32 direct route: 4096 bins u64 | queue count (+ kSmallF32DirectCount) | queue (+ kSmallF32DirectQueue)
constexpr size_t kSmallF32DirectCount = 32768, kSmallF32DirectQueue = kSmallF32DirectCount + 64;
constexpr size_t kSmallF32QueueBytes = 65536 * 16;           // a whole sample queue (f32 direct route, f32 level queue behind a 16-byte count): 65536 entries of 16 bytes
constexpr size_t kSmallF32TailBytes = 64 * 1024 + kSmallF32QueueBytes; // what the f32 flavour reserves beyond the u16 size
constexpr size_t kSmallF32Bytes = kSmallBytes + kSmallF32TailBytes;
constexpr size_t kSmallF32MaxRanks = 1024;                   // f32 stripe: 32 bytes per rank and one status word
static_assert(2 * sizeof(ChainBandState) <= kSmallBytes, "h_small: the chain's state read-back fits");
static_assert(kSmallF32PartialBytes * kSmallF32MaxRanks + 8 <= kSmallBytes, "h_small: the gathered partials of 1024 ranks fit the u16 size (the stripe reserves no more)");
static_assert(kSmallF32PartialBytes * kSmallF32MaxPartials <= kSmallOffF32Direct, "h_small: the f32 partials end where the direct route's bins begin");
static_assert(sizeof(uint64_t) * 4096 <= kSmallF32DirectCount, "h_small: the 4096 bins end where the queue count begins");
static_assert(kSmallOffF32Direct + kSmallF32DirectQueue + kSmallF32QueueBytes <= kSmallF32Bytes, "h_small: the direct route's whole queue fits");
static_assert(16 + kSmallF32QueueBytes + sizeof(uint64_t) * kLevelHistCount <= kSmallF32Bytes, "h_small: the f32 level queue and the histogram behind it fit");

// ---- one reserve per buffer
inline hipError_t reserve_luts(sarpro_hip_ctx *ctx) { return ctx->luts.reserve(kLutsBytes); }
inline hipError_t reserve_tile_bins(sarpro_hip_ctx *ctx) { return ctx->tile_bins.reserve(kTileBinsBytes); }
inline hipError_t reserve_cdfs(sarpro_hip_ctx *ctx) { return ctx->cdfs.reserve(kCdfsBytes); }
inline hipError_t reserve_level_hist(sarpro_hip_ctx *ctx, bool sampled_form = false) { return ctx->level_hist.reserve(sampled_form ? kLevelHistSampledBytes : kLevelHistBytes); }
inline hipError_t reserve_tables(sarpro_hip_ctx *ctx, bool chain = false) { return ctx->tables.reserve(chain ? kTablesChainBytes : kTablesHostBytes); }
inline hipError_t reserve_h_upload(sarpro_hip_ctx *ctx, size_t at_least = 0) { return ctx->h_upload.reserve(at_least > kUploadBytes ? at_least : kUploadBytes); }
inline hipError_t reserve_h_small(sarpro_hip_ctx *ctx, bool f32 = false) { return ctx->h_small.reserve(f32 ? kSmallF32Bytes : kSmallBytes); }

// ---- the per-band pieces
inline uint8_t *lut_of(sarpro_hip_ctx *ctx, int b) { return ctx->luts.as<uint8_t>() + (size_t)b * kLutBandStride; }
inline unsigned long long *tile_bins_of(sarpro_hip_ctx *ctx, int b) { return ctx->tile_bins.as<unsigned long long>() + (size_t)b * kTileBinCount; }
inline double *cdfs_of(sarpro_hip_ctx *ctx, int b) { return ctx->cdfs.as<double>() + (size_t)b * kTileBinCount; }
inline unsigned long long *level_hist_of(sarpro_hip_ctx *ctx, int b) { return ctx->level_hist.as<unsigned long long>() + (size_t)b * kLevelHistCount; }

} // namespace layout
} // namespace sarpro
