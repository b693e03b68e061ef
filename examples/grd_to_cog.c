/* grd_to_cog.c -- the C ABI end to end, no Python, no GDAL: two single-band u16 strip TIFFs (VV, VH as in a
 * Sentinel-1 GRD product's measurement/ folder) -> calibrate + autoscale + synthetic RGB on the GPU, its overview
 * pyramid in one more sweep over the raster in HBM -> ONE tiled GeoTIFF with overviews in cloud-optimised order
 * (directories first, smallest level first), which a viewer opens without reading the full resolution.
 *
 *   gcc -std=c99 -O2 -Iinclude examples/grd_to_cog.c -Lsarpro_amd -lsarpro_hip -Wl,-rpath,$PWD/sarpro_amd -o grd_to_cog
 *   ./grd_to_cog vv.tiff vh.tiff out.tiff [strategy 0..6, default 4 = CLAHE] [tile, default 512] [min_size, default 512]
 */
#include <stdio.h>
#include <stdlib.h>

#include "sarpro_hip.h"

int main(int argc, char **argv) {
    if (argc < 4) {
        fprintf(stderr, "usage: %s vv.tiff vh.tiff out.tiff [strategy] [tile] [min_size]\n", argv[0]);
        return 2;
    }
    const int strategy = argc > 4 ? atoi(argv[4]) : SARPRO_STRATEGY_CLAHE;
    const uint32_t tile = argc > 5 ? (uint32_t)atoi(argv[5]) : 0;
    const size_t min_size = argc > 6 ? (size_t)atoi(argv[6]) : 0;
    sarpro_hip_tiff *bands[2] = {NULL, NULL};
    sarpro_hip_tiff_info info[2];
    for (int b = 0; b < 2; ++b)
        if (sarpro_hip_tiff_open(argv[1 + b], &bands[b], &info[b]) != SARPRO_HIP_OK) {
            fprintf(stderr, "%s\n", sarpro_hip_tiff_last_error());
            return 1;
        }
    if (info[0].width != info[1].width || info[0].height != info[1].height) {
        fprintf(stderr, "the two bands differ in size\n");
        return 1;
    }
    sarpro_hip_ovr_plan plan;
    const int levels = sarpro_hip_overview_plan((size_t)info[0].width, (size_t)info[0].height, 3, 8, min_size, &plan);
    sarpro_hip_ctx *ctx = NULL;
    int rc = sarpro_hip_ctx_create(0, 0, &ctx);
    if (rc != SARPRO_HIP_OK) {
        fprintf(stderr, "no GPU context: %s\n", sarpro_hip_last_error(NULL));
        return 1;
    }
    sarpro_hip_stats stats[2];
    /* 0 is the no-data level of the product: it stays out of the averages */
    rc = sarpro_hip_dualpol_synrgb_stream_u16_cog(ctx, sarpro_hip_tiff_pair_reader, bands, (size_t)info[0].height, (size_t)info[0].width, strategy,
                                                  SARPRO_SYNRGB_DEFAULT, SARPRO_HIP_OVR_SKIP_ZERO, tile, min_size, argv[3], NULL, bands[0], stats);
    if (rc != SARPRO_HIP_OK) fprintf(stderr, "processing failed (%d): %s\n", rc, sarpro_hip_last_error(ctx));
    else
        printf("%llu x %llu + %d overviews down to %llu x %llu: band 1 %.2f..%.2f dB (median %.2f), band 2 %.2f..%.2f dB (median %.2f)\n",
               (unsigned long long)info[0].width, (unsigned long long)info[0].height, levels,
               (unsigned long long)(levels > 0 ? plan.cols[levels - 1] : info[0].width), (unsigned long long)(levels > 0 ? plan.rows[levels - 1] : info[0].height),
               stats[0].low_clip, stats[0].high_clip, stats[0].median_db, stats[1].low_clip, stats[1].high_clip, stats[1].median_db);
    sarpro_hip_ctx_destroy(ctx);
    sarpro_hip_tiff_close(bands[0]);
    sarpro_hip_tiff_close(bands[1]);
    return rc == SARPRO_HIP_OK ? 0 : 1;
}
