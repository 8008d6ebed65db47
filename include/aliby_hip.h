/*
 * aliby_hip.h — C ABI of libaliby_hip.so (MI355X / gfx950).
 *
 * The reference (afermg/aliby) has no FFI: its seam is the Python step-callable
 * protocol chosen by step-name prefix (src/aliby/pipe.py:47-72).
 * This header is the boundary the Python step callables in `aliby_amd/` sit on;
 * every entry point cites the reference interface whose arithmetic it replaces.
 *
 * Conventions
 *   - every function returns an int status (ALIBY_OK == 0); on failure
 *     aliby_last_error() returns a thread-local message.  The ctypes shim maps
 *     codes to the Python exception types the reference raises
 *     (ValueError / OverflowError / Exception, SURVEY.md §8b "Errors").
 *   - `stream` is a hipStream_t passed as void* (NULL = the null stream).
 *   - pointers marked [dev] are device pointers (hipMalloc / torch), [host] host.
 *   - images are row-major; a "tile" is one [Y,X] label image plus C planes.
 *   - pixel planes are ALIBY_U16 (uint16) or ALIBY_F32 (float).
 *   - feature outputs are float64, written at out[row*ld + col].
 *   - nothing here allocates inside a launch path: workspaces are explicit.
 */
#ifndef ALIBY_HIP_H
#define ALIBY_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ALIBY_ABI_VERSION 1

enum {
  ALIBY_OK = 0,
  ALIBY_ERR_INVALID = 1,      /* bad argument             -> ValueError    */
  ALIBY_ERR_OVERFLOW = 2,     /* labels >= 65535          -> OverflowError */
  ALIBY_ERR_HIP = 3,          /* HIP runtime failure      -> RuntimeError  */
  ALIBY_ERR_TOO_LARGE = 4,    /* object exceeds workspace -> RuntimeError  */
  ALIBY_ERR_UNSUPPORTED = 5   /* e.g. non-ufunc reducer   -> Exception     */
};

enum { ALIBY_U16 = 0, ALIBY_F32 = 1,
       ALIBY_U64 = 2, ALIBY_F64 = 3 /* output dtypes of aliby_reduce_z only: NumPy's own result types */,
       ALIBY_U8W = 4 /* uint16 storage holding uint8 / bool pixels: aliby_features_texture only (their grey level is the value
                        itself, skimage.util.img_as_ubyte leaves uint8 alone); every other entry takes such planes as ALIBY_U16 */ };

/* reduce_z operators — extraction/core/functions/loaders.py:110-127 ("max","add","div";
 * "mean"/"median" are not ufuncs and raise in distributors.py:20-24). */
enum { ALIBY_RED_MAX = 0, ALIBY_RED_ADD = 1, ALIBY_RED_DIV = 2 };

typedef struct aliby_ctx aliby_ctx;

/* One row per object, in (tile, label) order — the row order of
 * process_tree_masks' ind_masks (extraction/extract.py:276-281). */
typedef struct aliby_object {
  int32_t tile;   /* index into the F tiles                               */
  int32_t label;  /* 1..max(labels[tile])                                 */
  int32_t y0, x0; /* bbox, inclusive; y0>y1 when the label is absent      */
  int32_t y1, x1; /* bbox, exclusive                                      */
  int32_t area;   /* pixel count (0 when absent)                          */
  int32_t pad_;
} aliby_object;

/* ---- context / errors ------------------------------------------------- */
int aliby_abi_version(void);
const char* aliby_last_error(void);
int aliby_ctx_create(int device, aliby_ctx** out);
int aliby_ctx_destroy(aliby_ctx* ctx);
int aliby_device_info(aliby_ctx* ctx, int* cu_count, int* lds_bytes, size_t* hbm_bytes,
                      char* name, int name_len);

/* plain memory helpers for callers without torch */
int aliby_malloc(aliby_ctx* ctx, size_t bytes, void** dptr);
int aliby_free(aliby_ctx* ctx, void* dptr);
int aliby_memcpy_h2d(aliby_ctx* ctx, void* dst_dev, const void* src_host, size_t bytes, void* stream);
int aliby_memcpy_d2h(aliby_ctx* ctx, void* dst_host, const void* src_dev, size_t bytes, void* stream);
int aliby_memset(aliby_ctx* ctx, void* dst_dev, int value, size_t bytes, void* stream);
int aliby_stream_sync(aliby_ctx* ctx, void* stream);

/* ---- a4: tile stager --------------------------------------------------- */
/* Tiler.get_fczyx / get_tp_channel / if_out_of_bounds_pad
 * (src/aliby/tile/tiler.py:309-366,601-650; Tile.as_range tiles.py:151-166).
 * stack [dev] is one time point [C,Z,Y,X]; rects [host] is F x (y0,x0,h,w) in
 * image coordinates and may leave the image.  out [dev] is [F,C,Z,h,w].
 * Partly outside -> np.pad(mode="median") semantics (per-line medians, rounded
 * for integers); more than 25% outside along an axis -> the tile is NaN and
 * flags[f] = 1 (out_f32 only).  All tiles share (h,w).  A window that misses the
 * image altogether and still escapes that rule (the reference pairs before-pads with h
 * and after-pads with w: wholly left with h >= 4w, wholly below with w >= 4h) has no
 * tile in the reference either (np.pad raises on the empty axis): ALIBY_ERR_INVALID,
 * nothing launched. */
int aliby_crop_pad_u16(aliby_ctx* ctx, const uint16_t* stack, int C, int Z, int Y, int X,
                       const int32_t* rects, int F, int h, int w, uint16_t* out,
                       int32_t* nan_flags_host, void* stream);

/* ---- a5: reduce_z ------------------------------------------------------- */
/* reduce_z(pixels, ufunc, axis) (extraction/core/functions/distributors.py:6-24):
 * in [dev] is [outer, Z, inner]; out [dev] is [outer, inner]; ufunc.reduce order
 * (left fold over Z).  max keeps the input dtype.  For u16 input NumPy's results are
 * uint64 for add.reduce (small unsigned ints are promoted, no wrap) and float64 for
 * divide.reduce: out_dtype ALIBY_U64 / ALIBY_F64 give exactly those; out_dtype
 * ALIBY_F32 gives the same values narrowed to f32, which is what the feature kernels
 * consume (sums exact while < 2^24, i.e. Z <= 256).  f32 input: f32 left fold; its max
 * gives NaN wherever a plane holds one, as np.maximum does. */
int aliby_reduce_z(aliby_ctx* ctx, const void* in, int dtype, size_t outer, int Z, size_t inner,
                   int op, void* out, int out_dtype, void* stream);

/* ---- crop tiler ------------------------------------------------------------ */
/* CropTiler.get_fczyx (src/aliby/tile/tiler.py:75-189): per-channel whole-frame normalisation, then a grid of
 * non-overlapping tile_size x tile_size tiles, n_th = (Y - ts) / ts + 1 by n_tw = (X - ts) / ts + 1 (remainder rows and
 * columns dropped; a tile larger than the frame: no tile, nothing written).  Stages, in this order, each optional: */
enum { ALIBY_CROP_CLIP = 1 /* clip_outliers: (v - pmin) / (pmax - pmin) clipped to [0, 1] */,
       ALIBY_CROP_8BIT = 2 /* convert_8bit: trunc(x * 255) as uint8; on raw integers (v * 255) mod 256, as NumPy wraps */,
       ALIBY_CROP_STD = 4 /* standard_scale: (x - mean) / std, population std */ };
/* stack [dev] is uint16 [C,Z,Y,X], out [dev] is [n_th * n_tw, C, Z, ts, ts] of out_dtype: ALIBY_U16 while no float stage is
 * on (raw crop; 8-bit results as 8-bit-in-uint16), else ALIBY_F64 (the reference's values) or ALIBY_F32 (those rounded once).
 * pmin / pmax are NumPy's percentile(method="linear") at clip and 100 - clip per channel (clip <= 0: min / max), mean and std
 * those of the values after the earlier stages; a constant channel gives NaN (0 / 0) in float outputs and 0 after the 8-bit
 * cast.  stats_out [dev, C x 4 float64, may be NULL] receives (pmin, pmax, mean, std), NaN where a stage is off.  Everything
 * runs on the device in stream order; histogram and statistics use ctx scratch.  Z*Y*X < 2^32. */
int aliby_crop_tiles_u16(aliby_ctx* ctx, const uint16_t* stack, int C, int Z, int Y, int X, int tile_size, int flags,
                         double clip, void* out, int out_dtype, double* stats_out, void* stream);
/* Its three parts.  hist [dev] is [C,65536] uint32 counts of stack [C, n] (zeroed here; integer atomics: independent of the
 * launch geometry); stats [dev] [C,4] from such a histogram; the tile pass with given statistics (NULL when flags has neither
 * ALIBY_CROP_CLIP nor ALIBY_CROP_STD). */
int aliby_crop_hist_u16(aliby_ctx* ctx, const uint16_t* stack, int C, size_t n, uint32_t* hist, void* stream);
int aliby_crop_stats(aliby_ctx* ctx, const uint32_t* hist, int C, size_t n, int flags, double clip, double* stats, void* stream);
int aliby_crop_cut_u16(aliby_ctx* ctx, const uint16_t* stack, int C, int Z, int Y, int X, int tile_size, int flags,
                       const double* stats, void* out, int out_dtype, void* stream);

/* ---- a7/a8: object table (replaces transform_2d_to_3d) ------------------ */
/* process_tree_masks enumerates labels 1..mask.max() per tile
 * (extract.py:276-281); transform_2d_to_3d (agora/utils/masks.py:35-37) explodes
 * them to (N,Y,X) bool.  Here the label image stays as is and a compact table of
 * per-object bboxes/areas is built instead.
 * Step 1: per-tile maximum label -> max_host[F] (synchronises `stream`). */
int aliby_label_max(aliby_ctx* ctx, const uint16_t* labels, int F, int Y, int X,
                    int32_t* max_host, void* stream);
/* Step 2: fill table [dev] (n_obj rows = sum(max_host)), offsets_host[F+1] is the
 * exclusive prefix sum of max_host.  Also copies the table to table_host if non-NULL
 * (synchronises). */
int aliby_object_table(aliby_ctx* ctx, const uint16_t* labels, int F, int Y, int X,
                       const int32_t* offsets_host, aliby_object* table_dev,
                       aliby_object* table_host, void* stream);

/* relabel_sequential (skimage, used at segment/dispatch.py:223 and extract.py:496):
 * labels [dev, in place] renumbered 1..n in increasing original-label order,
 * n_host[F] receives the per-tile count.  Raises ALIBY_ERR_OVERFLOW if n >= 65535
 * (dispatch.py:230-233). */
int aliby_relabel_sequential(aliby_ctx* ctx, uint16_t* labels, int F, int Y, int X,
                             int32_t* n_host, void* stream);

/* ---- a6: segment closure pre-processing ----------------------------------- */
/* pixels[:, channel_to_segment] then max over Z (segment/dispatch.py:192,199-206):
 * pixels [dev] [F,C,Z,Y,X] uint16 -> out [dev] [F,Y,X]. */
int aliby_select_project_u16(aliby_ctx* ctx, const uint16_t* pixels, int F, int C, int Z, int Y, int X,
                             int channel, uint16_t* out, void* stream);
/* cellpose.transforms.normalize99 (normalize=True at dispatch.py:203,212): per image
 * (x - p_lower) / (p_upper - p_lower) as float32, zeros when the range is < 1e-3; percentiles are exact
 * order statistics with linear interpolation (numpy.percentile).  percentiles_dev [F,2] receives them. */
int aliby_normalize99_u16(aliby_ctx* ctx, const uint16_t* img, int F, int Y, int X, double lower,
                          double upper, float* out, double* percentiles_dev, void* stream);
/* cellpose.transforms.make_tiles on the zero-padded image: tiles [dev] [F*ny*nx, nchan, by, bx]; channel 0
 * is the image, the others are zero (grayscale input of the 2-channel U-Net). */
int aliby_make_tiles(aliby_ctx* ctx, const float* img, int F, int Y, int X, int ypad1, int xpad1, int Ly,
                     int Lx, int by, int bx, int ny, int nx, const int32_t* ystart_dev,
                     const int32_t* xstart_dev, int nchan, float* tiles, void* stream);
/* cellpose.transforms.average_tiles + un-padding: network output tiles [F*ny*nx, 3, by, bx] -> dP [F,2,Y,X],
 * cellprob [F,Y,X], weighted by taper_dev [by,bx] and accumulated in tile order in float32. */
int aliby_average_tiles(aliby_ctx* ctx, const float* ytiles, int F, int Y, int X, int ypad1, int xpad1,
                        int Ly, int Lx, int by, int bx, int ny, int nx, const int32_t* ystart_dev,
                        const int32_t* xstart_dev, const float* taper_dev, float* dP, float* cellprob,
                        void* stream);
/* The same two steps over N slices of a batch of volumes, read and written in place (cellpose's do_3D passes): image n starts
 * at (n / S) * vol_stride + (n % S) * slice_stride elements and its pixel (y, x) lies row_stride * y + col_stride * x further.
 * aliby_average_tiles_strided writes output channel 0 / 1 into components comp0 / comp1 of dP (comp_stride elements apart,
 * dP_vol_stride per volume) and channel 2 into cellprob (prob_vol_stride per volume), at the same slice / row / column
 * offsets; bit k of add_mask adds channel k to the value already there (float32) instead of writing it. */
int aliby_make_tiles_strided(aliby_ctx* ctx, const float* vol, int N, int S, long long vol_stride, long long slice_stride,
                             long long row_stride, long long col_stride, int Y, int X, int ypad1, int xpad1, int Ly, int Lx,
                             int by, int bx, int ny, int nx, const int32_t* ystart_dev, const int32_t* xstart_dev, int nchan,
                             float* tiles, void* stream);
int aliby_average_tiles_strided(aliby_ctx* ctx, const float* ytiles, int N, int S, long long dP_vol_stride,
                                long long prob_vol_stride, long long slice_stride, long long row_stride, long long col_stride,
                                long long comp_stride, int comp0, int comp1, int add_mask, int Y, int X, int ypad1, int xpad1,
                                int Ly, int Lx, int by, int bx, int ny, int nx, const int32_t* ystart_dev,
                                const int32_t* xstart_dev, const float* taper_dev, float* dP, float* cellprob, void* stream);

/* Fused pointwise stage between two convolutions of the U-Net (bf16, NHWC): sum = A (+ B) (+ bias[c]), A/B
 * optionally read through a 2x nearest upsample; act = relu?(scale[c]*sum + shift[n,c] or shift[c]).
 * shift_per_sample: 0 = one shift row for all samples, 1 = contiguous [N, C], >1 = row stride in floats.  SUM
 * and/or ACT are written.  Replaces the eager conv-bias / BatchNorm / ReLU / add / style-add / upsample
 * passes of the network that `model.eval` (segment/dispatch.py:208-215) runs.  Only the A/B fallback path
 * (`FusedUNet(mfma_levels=())`, kept for the tests) uses it: the product forward runs the aliby_nn_conv* units
 * below, which carry these stages in their prologue / epilogue. */
int aliby_nn_fused_act_bf16(aliby_ctx* ctx, const void* A, const void* B, void* SUM, void* ACT,
                            const float* bias, const float* scale, const float* shift, int N, int H, int W,
                            int C, int upA, int upB, int relu, int shift_per_sample, void* stream);
/* One convolution unit of the U-Net on the matrix cores (bf16 NHWC, fp32 accumulate), hand-written MFMA
 * implicit GEMM with the pointwise stages fused around it:
 *   OUT[n,y,x,:] = conv3x3( relu(scale[c]*IN[n, y>>in_up, x>>in_up, c] + shift[n or 0, c]), zero padded )
 *                  + bias[:] + RES[n, y>>res_up, x>>res_up, :]
 * (bias, RES may be NULL; shift_per_sample as for the fused pointwise stage).  This is cellpose's `batchconv` / `batchconvstyle` (BatchNorm -> ReLU -> Conv2d)
 * plus the residual / skip / style adds of `resdown` / `resup`, i.e. the network `model.eval`
 * (segment/dispatch.py:208-215) runs.  wpk comes from the packing call below.  IN may be a channel slice
 * [in_channel0, in_channel0 + CIN) of a tensor with in_channels channels (0 = exactly CIN): a convolution
 * over more input channels than one launch holds is split along K, each launch adding to the previous one
 * through RES.  OUT / RES / pool_out may likewise be the channel slice [out_channel0, out_channel0 + COUT) of
 * tensors with out_channels channels (0 = exactly COUT): wide outputs are produced slice by slice.  pool_out, when not NULL, also receives max_pool2d(OUT, 2, 2) as bf16 NHWC [N,H/2,W/2,COUT]
 * (cellpose's `downsample` maxpool, fused into the epilogue of the block's last convolution).
 * Supported (CIN, COUT, in_up): (32,32,0) (32,64,0) (64,64,0) (64,32,1) (64,64,1) (64,128,0) (64,128,1);
 * anything else returns ALIBY_ERR_UNSUPPORTED (wider layers: K/N slices, see above). */
int aliby_nn_conv3x3_bf16(aliby_ctx* ctx, const void* in, const void* wpk, void* out, const float* scale,
                          const float* shift, int shift_per_sample, const float* bias, const void* res,
                          int res_up, int N, int H, int W, int CIN, int COUT, int in_up, int in_channels,
                          int in_channel0, int out_channels, int out_channel0, void* pool_out, void* stream);
/* Frame-to-frame IoU stitching of label images, batched over tiles: the working stand-in for the reference's `stitch`
 * tracker (src/aliby/track/trackers.py:14-90 = update_labels + cellpose.utils.stitch3D on a (previous, current) pair
 * per tile; not importable as shipped).  prev / cur are uint16 [F,Y,X]; the tables and their host offsets come from
 * aliby_object_table (rows in (tile, label) order); prev_tracked_dev[row] is the tracked label the previous frame's
 * object already carries (NULL = its own label); max_label_in_host[tile] the running maximum (NULL = 0).
 * cur_tracked_dev[row] receives the tracked label of every current object (0 for labels absent from the frame):
 * the previous tracked label of the best IoU >= threshold partner that is also that partner's best, else
 * max_label + 1, + 2, ... in current label order; max_label_out_host[tile] the new running maximum.
 * threshold in [0.01, 1] (cellpose's default is 0.25; the reference's 3-D branch passes 0.01, dispatch.py:195); more than 16
 * previous objects above the threshold under one current mask is an error. */
int aliby_track_stitch(aliby_ctx* ctx, const uint16_t* prev, const uint16_t* cur, int F, int Y, int X,
                       const aliby_object* cur_table_dev, const int32_t* cur_offsets_host,
                       const aliby_object* prev_table_dev, const int32_t* prev_offsets_host,
                       const int32_t* prev_tracked_dev, const int32_t* max_label_in_host, double threshold,
                       int32_t* cur_tracked_dev, int32_t* max_label_out_host, void* stream);

/* The same unit for the deep levels of the network (128 / 256 channels at 56 x 56 and 28 x 28) as ONE launch: the whole
 * K = 9 * CIN reduction is accumulated in fp32 registers (K loop over 64-channel slices inside the kernel, weights streamed
 * from the packed array), instead of K/N-slice launches of aliby_nn_conv3x3_bf16 adding bf16 partial sums through HBM.
 * Arguments as aliby_nn_conv3x3_bf16 (full tensors, no channel slices); wpk = aliby_nn_pack_conv3x3_bf16 over the full CIN.
 * Supported: CIN in {64, 128, 256}, COUT a multiple of 128, W <= 56, (H + 1) * (W + 2) >= 226 + 2 * (W + 2) when the shift
 * is per sample; anything else returns ALIBY_ERR_UNSUPPORTED (the caller then uses the slice launches).
 * Replaces: cellpose `batchconv` / `batchconvstyle` at the deep levels of the network `model.eval` runs
 * (segment/dispatch.py:208-215). */
int aliby_nn_conv3x3_deep_bf16(aliby_ctx* ctx, const void* in, const void* wpk, void* out, const float* scale,
                               const float* shift, int shift_per_sample, const float* bias, const void* res, int res_up,
                               int N, int H, int W, int CIN, int COUT, int in_up, void* stream);

/* The same K-loop unit for the up path's 128 -> 64 convolution (input read through the 2x upsample, skip tensor as RES): ONE
 * launch with fp32 accumulation over the whole 9 * 128 reduction (K loop over 32-channel slices, a workgroup = 2 channel
 * groups x 2 position groups), instead of two K-slice launches of aliby_nn_conv3x3_bf16 with a bf16 partial sum in HBM.
 * Arguments as aliby_nn_conv3x3_deep_bf16.  Supported: CIN = 128, COUT = 64, in_up = 1, even H and W, W <= 128,
 * (H + 1) * (W + 2) >= 450 + 2 * (W + 2) when the shift is per sample; anything else returns ALIBY_ERR_UNSUPPORTED and
 * launches nothing.  Replaces: cellpose `batchconv` of `resup.conv0` at the second-finest level (segment/dispatch.py:208-215). */
int aliby_nn_conv3x3_kloop64_bf16(aliby_ctx* ctx, const void* in, const void* wpk, void* out, const float* scale,
                                  const float* shift, int shift_per_sample, const float* bias, const void* res, int res_up,
                                  int N, int H, int W, int CIN, int COUT, int in_up, void* stream);

/* The limits of the two K-loop units above, for a caller that routes by them: limits[0] = output positions per tile of
 * aliby_nn_conv3x3_deep_bf16 (its minimum image with a per-sample shift is (H + 1) * (W + 2) >= limits[0] + 2 * (W + 2) + 2),
 * limits[1] = its widest map, limits[2] and limits[3] = the same two figures of aliby_nn_conv3x3_kloop64_bf16.  Needs no
 * device and no context. */
int aliby_nn_conv3x3_kloop_limits(int limits[4]);

/* The same unit on v_mfma_f32_16x16x32_bf16 (the shape the chip holds a higher clock on: nn_conv_deep.hip).  Same arguments and
 * meaning; `wpk16` is packed by aliby_nn_pack_conv3x3_deep16_bf16 (w_oihw float32 [COUT, CIN, 3, 3], COUT a multiple of 32, CIN
 * of 64 -> COUT * CIN * 9 bf16).  Accumulates 32 input channels per instruction: agrees with aliby_nn_conv3x3_deep_bf16 to fp32
 * rounding, not bit for bit. */
int aliby_nn_conv3x3_deep16_bf16(aliby_ctx* ctx, const void* in, const void* wpk16, void* out, const float* scale,
                               const float* shift, int shift_per_sample, const float* bias, const void* res, int res_up,
                               int N, int H, int W, int CIN, int COUT, int in_up, void* stream);
int aliby_nn_pack_conv3x3_deep16_bf16(aliby_ctx* ctx, const float* w_oihw, int COUT, int CIN, void* wpk16, void* stream);
/* Diagnostics for the deep kernel: stamps_dev [8 tiles][32] uint64 shader-clock stamps of wave 0 of workgroup 0 (0 tile start,
 * 1 set-up done, then per K slice s: 2+4s after the first barrier, 3+4s prologue written, 4+4s after the second barrier,
 * 5+4s MFMA loop done; 2+4S epilogue done).  NULL switches it off (the default). */
int aliby_debug_conv_deep_trace(aliby_ctx* ctx, void* stamps_dev);
/* max_pool2d(IN, 2, 2) on bf16 NHWC [N,H,W,C] -> [N,H/2,W/2,C] (cellpose `downsample.maxpool` between the levels whose
 * last convolution runs on the deep kernel; elsewhere the pooled tensor is an epilogue of aliby_nn_conv3x3_bf16). */
int aliby_nn_maxpool2_bf16(aliby_ctx* ctx, const void* in, void* out, int N, int H, int W, int C, void* stream);

/* Diagnostics: when stamps_dev != NULL, wave 0 of workgroup 0 of every following conv3x3 launch (register-staged
 * variant) writes its shader-clock stamps at the phase boundaries of its first 16 tiles into stamps_dev[16][8]
 * (uint64: 0 tile start, 1 loads issued, 2 after barrier, 3 prologue done, 4 after barrier, 5 MFMA done,
 * 6 stores issued).  NULL switches it off (the default). */
int aliby_debug_conv_trace(aliby_ctx* ctx, void* stamps_dev);
/* Tile order of the persistent convolution launches (every aliby_nn_conv3x3* / _pair / aliby_nn_first_pair entry) on `ctx`.  Each
 * XCD walks its eighth of a launch's tiles upwards (ALIBY_CONV_ASCENDING), from its end downwards (ALIBY_CONV_DESCENDING), or
 * (ALIBY_CONV_ALTERNATE, a new context's mode) in the direction opposite to the context's previous launch, so that a launch
 * starts on what its producer wrote last and the Infinity Cache still holds.  Setting a mode restarts the alternation at
 * ascending.  The order changes when a tile is computed, never its bits; launches with phase stamps on walk upwards. */
enum { ALIBY_CONV_ALTERNATE = 0, ALIBY_CONV_ASCENDING = 1, ALIBY_CONV_DESCENDING = 2 };
int aliby_nn_conv_order(aliby_ctx* ctx, int mode);
/* The same unit (segment/dispatch.py:208-215) with the residual block's 1x1 projection fused in (cellpose `resdown`: x = proj(x_in) + conv1(conv0(x_in))):
 *   OUT = conv3x3( relu(scale*IN + shift) ) + bias + proj_w . PROJ_IN[n,y,x,:]
 * PROJ_IN is the block's RAW input [N,H,W,proj_channels] bf16 (no activation; the projection's BatchNorm is folded into
 * proj_w, its bias into `bias`), so the projected tensor never exists in HBM.  proj_wpk comes from
 * aliby_nn_pack_conv1x1_bf16 with CIN = 16 (for (CIN,COUT) = (32,32), proj_channels <= 16) or 32 ((64,64), <= 32). */
int aliby_nn_conv3x3_proj_bf16(aliby_ctx* ctx, const void* in, const void* wpk, void* out, const float* scale,
                               const float* shift, int shift_per_sample, const float* bias, int N, int H, int W,
                               int CIN, int COUT, const void* proj_in, const void* proj_wpk, int proj_channels,
                               void* stream);
/* The network's LAST unit with the output head in its epilogue (cellpose CPnet.output: BatchNorm + ReLU + 1x1 convolution
 * to `head_channels` <= 3 maps, segment/unet.py): head_out [N, head_channels, H, W] float32 =
 * head_bias[o] + sum_c head_w[o, c] * bf16(relu(head_scale[c] * OUT[c] + head_shift[c])) — bit-identical to running
 * aliby_nn_out_head_bf16 on the unit's bf16 output.  out_or_null = NULL skips writing that output (nothing else reads
 * it).  Built for the 32 -> 32 unit. */
int aliby_nn_conv3x3_head_bf16(aliby_ctx* ctx, const void* in, const void* wpk, void* out_or_null, const float* scale,
                               const float* shift, int shift_per_sample, const float* bias, const void* res, int res_up,
                               int N, int H, int W, int CIN, int COUT, const float* head_scale,
                               const float* head_shift, const float* head_w, const float* head_bias, int head_channels,
                               float* head_out, void* stream);
/* The network's first two units in ONE launch (round 3): x1 = conv3x3(act1(conv3x3(act0(tiles)))) + proj(tiles) + bias1 — what
 * aliby_nn_first_conv_bf16 followed by aliby_nn_conv3x3_proj_bf16 compute, without the first layer's output (c0, 32 channels)
 * and the raw bf16 copy of the tiles ever reaching HBM: same bits as the two launches.  tiles float32 [N, Cin <= 2, H, W];
 * scale0 / shift0 [Cin] and w_oihw [32][Cin][9] as in aliby_nn_first_conv_bf16; wpk1 the second unit's packed weights
 * (32 -> 32), scale1 / shift1 [32] its prologue (shift1 already carries the first layer's bias), bias1 [32] its bias plus the
 * projection's; proj_wpk the projection packed with aliby_nn_pack_conv1x1_bf16(..., CIN = 16).  out [N, H, W, 32] bf16. */
int aliby_nn_first_pair_bf16(aliby_ctx* ctx, const float* tiles, int N, int Cin, int H, int W, const float* scale0,
                             const float* shift0, const float* w_oihw, const void* wpk1, const float* scale1,
                             const float* shift1, const float* bias1, const void* proj_wpk, void* out, void* stream);
/* Two consecutive 32 -> 32 units of a residual block in ONE launch (cellpose resdown / resup: x + conv3(conv2(x)),
 * segment/unet.py): out = conv_b(act_b(conv_a(act_a(in)) + bias_a)) + bias_b + res, the tensor in between kept in LDS
 * (rounded to bf16 where the two-launch path stores it: same bits as two aliby_nn_conv3x3_bf16 launches).  An 8-wave
 * workgroup per CU: four waves hold unit A's weights and produce a tile's intermediate block while the other four hold
 * unit B's and consume the previous tile's.  pool_out as in aliby_nn_conv3x3_bf16; head_* as in
 * aliby_nn_conv3x3_head_bf16 (head_out != NULL: out_or_null may be NULL). */
int aliby_nn_conv3x3_pair_bf16(aliby_ctx* ctx, const void* in, const void* wpk_a, const void* wpk_b, void* out_or_null,
                               const float* scale_a, const float* shift_a, int shift_a_per_sample, const float* bias_a,
                               const float* scale_b, const float* shift_b, int shift_b_per_sample, const float* bias_b,
                               const void* res, int N, int H, int W, void* pool_out, const float* head_scale,
                               const float* head_shift, const float* head_w, const float* head_bias, int head_channels,
                               float* head_out, void* stream);
/* float32 OIHW [COUT, CIN_src, 3, 3] device weights -> the MFMA fragment order the kernel above reads
 * ([COUT/32][9 taps][CIN/16][64 lanes][8] bf16, COUT*CIN*9*2 bytes; input channels >= CIN_src are zero). */
int aliby_nn_pack_conv3x3_bf16(aliby_ctx* ctx, const float* w_oihw, int COUT, int CIN_src, int CIN, void* wpk,
                               void* stream);
/* Weight preparation for the two entries above (what the reference leaves to torch's module loading,
 * segment/dispatch.py:161-175): float32 [COUT, CIN_src] device weights of a 1x1 convolution -> [COUT/32][CIN/16][64 lanes][8] bf16 (same row order). */
int aliby_nn_pack_conv1x1_bf16(aliby_ctx* ctx, const float* w_oi, int COUT, int CIN_src, int CIN, void* wpk,
                               void* stream);
/* network output bf16 NHWC [N,H,W,Cpad] (+ bias[Cout]) -> float32 NCHW [N,Cout,H,W]. */
int aliby_nn_nhwc_to_nchw_f32(aliby_ctx* ctx, const void* y, int N, int H, int W, int Cpad, int Cout,
                              const float* bias, float* out, void* stream);
/* 1x1 convolution of the network that `model.eval` runs (segment/dispatch.py:208-215; cellpose `resdown.proj` /
 * `resup.proj`: BatchNorm -> Conv2d(1x1), BatchNorm folded into the weights by the caller): OUT[n,y,x,:] = W . IN[n,y,x,:] + bias, bf16 NHWC, hand-written MFMA GEMM over the N*H*W
 * pixels.  wpk from aliby_nn_pack_conv1x1_bf16(COUT, CIN, CIN).  CIN in {32, 64, 128, 256}; COUT 32, 64 or a multiple of
 * 128; bias may be NULL. */
int aliby_nn_conv1x1_bf16(aliby_ctx* ctx, const void* in, const void* wpk, const float* bias, void* out, int N, int H, int W,
                          int CIN, int COUT, void* stream);
/* First layer of the network that `model.eval` runs (segment/dispatch.py:208-215) on float32 NCHW tiles with Cin <= 2
 * channels (the 2-channel input cellpose builds from the selected plane, dispatch.py:192-206):
 * c0 = conv3x3(bf16(relu(scale[c]*x + shift[c])), zero padded) as bf16 NHWC[32] WITHOUT the convolution's bias, and the raw
 * input as bf16 NHWC[8] (channels >= Cin zero) for the block's projection.  w_oihw: float32 [32, Cin, 3, 3] (pass bf16-
 * representable values to reproduce a bf16 convolution). */
int aliby_nn_first_conv_bf16(aliby_ctx* ctx, const float* tiles, int N, int Cin, int H, int W, const float* scale,
                             const float* shift, const float* w_oihw, void* raw8, void* c0, void* stream);
/* Style vector of the network that `model.eval` runs (segment/dispatch.py:208-215; cellpose `make_style`: global average pool of the deepest feature map, L2-normalised) and
 * the per-sample shifts of every styled unit derived from it in one batched product: x bf16 NHWC [N,H,W,C] ->
 * style float32 [N,C]; shifts[n,:] = b + style[n,:] . wt, wt float32 [C,J] (`batchconvstyle.full` of all units, folded with
 * their BatchNorm by the caller), shifts float32 [N,J]. */
int aliby_nn_style_bf16(aliby_ctx* ctx, const void* x, int N, int H, int W, int C, const float* wt, const float* b, int J,
                        float* style, float* shifts, void* stream);
/* Output head of the network (cellpose CPnet.output = BatchNorm -> ReLU -> 1x1 Conv2d, the flows + cellprob
 * that `model.eval` (segment/dispatch.py:208-215) returns): x bf16 NHWC [N,H,W,32] -> float32 NCHW [N,O,H,W],
 * y = bias[o] + sum_c bf16(w[o,c]) * bf16(relu(scale[c]*x + shift[c])); w is float32 [O,32], rounded to bf16 as the bf16
 * convolution it replaces holds it.  Round 3: two k-steps of the 32x32x16 MFMA per 32 pixels (csrc/nn_conv.hip, head_apply)
 * — the same function the fused forms (aliby_nn_conv3x3_head_bf16, aliby_nn_conv3x3_pair_bf16) call: same bits. */
int aliby_nn_out_head_bf16(aliby_ctx* ctx, const void* x, const float* scale, const float* shift, const float* w,
                           const float* bias, int N, int H, int W, int C, int O, float* out, void* stream);
/* float32 NCHW network tiles (Cin <= 8) -> bf16 NHWC padded to 8 channels: raw copy and relu(bn(x)). */
int aliby_nn_tiles_to_nhwc8_bf16(aliby_ctx* ctx, const float* tiles, int N, int Cin, int H, int W,
                                 const float* scale, const float* shift, void* raw, void* act, void* stream);

/* ---- a6': Cellpose post-network dynamics ---------------------------------- */
/* What `model.eval` (segment/dispatch.py:208-215; cellpose.dynamics.compute_masks) does after the
 * network for 2-D images: dP [dev] is [F,2,Y,X] float32 (dY,dX at network scale), cellprob [dev] is
 * [F,Y,X]; labels_out [dev] receives uint16 labels 1..n per tile, n_labels_host[F] the counts.
 * Defaults of the reference's call: niter=200, cellprob_threshold=0, flow_threshold=0.4,
 * min_size=15, max_size_fraction=0.4.  workspace [dev] >= aliby_masks_workspace_bytes(F,Y,X).
 * p_final_out [dev, optional] receives the flow-following end points [F,2,Y,X] (debug/tests).
 * Raises ALIBY_ERR_OVERFLOW when a tile would need >= 65535 labels (dispatch.py:230-233). */
size_t aliby_masks_workspace_bytes(int F, int Y, int X);
int aliby_masks_from_flows(aliby_ctx* ctx, const float* dP, const float* cellprob, int F, int Y, int X,
                           int niter, float cellprob_threshold, float flow_threshold, int min_size,
                           float max_size_fraction, void* workspace, size_t workspace_bytes,
                           uint16_t* labels_out, int32_t* n_labels_host, float* p_final_out, void* stream);
/* The same for volumes (cellpose's do_3D): dP [dev] [F,3,Z,Y,X] float32 (dZ,dY,dX at network scale), cellprob [dev]
 * [F,Z,Y,X] -> labels_out [dev] uint16 [F,Z,Y,X], 1..n per volume, n_labels_host[F].  Trilinear flow following (grid_sample,
 * align_corners=False, zero padding), 5x5x5 seeds, growth in 11x11x11 windows, masks above max_size_fraction of the volume and
 * below min_size voxels dropped, 3-D holes (6-connected background) filled.  There is no flow-error QC in 3-D (cellpose: "not
 * used for 3D").  workspace [dev] >= aliby_masks3d_workspace_bytes(F,Z,Y,X); p_final_out [dev, optional] [F,3,Z,Y,X] receives
 * the end points of the foreground voxels.  ALIBY_ERR_OVERFLOW when a volume would need >= 65535 labels. */
size_t aliby_masks3d_workspace_bytes(int F, int Z, int Y, int X);
int aliby_masks_from_flows_3d(aliby_ctx* ctx, const float* dP, const float* cellprob, int F, int Z, int Y, int X, int niter,
                              float cellprob_threshold, int min_size, float max_size_fraction, void* workspace,
                              size_t workspace_bytes, uint16_t* labels_out, int32_t* n_labels_host, float* p_final_out,
                              void* stream);

/* ---- a13: cp_measure single-image features ------------------------------ */
/* Call site wrap_cp_measure_features (loaders.py:135-150): fun(mask.astype(uint16), pixels).
 * planes [dev] is [F, C, Y, X] (already z-reduced); channel selects the plane.
 * Rows of `out` follow the object table; columns start at col0 in the order listed in
 * aliby_amd/extraction/features.py (intensity: 21 columns, 16 without the edge block). */
int aliby_features_intensity(aliby_ctx* ctx, const uint16_t* labels, const void* planes, int dtype,
                             int F, int C, int Y, int X, int channel,
                             const aliby_object* table_dev, int n_obj, int max_area,
                             int edge_measurements, double* out, int ld, int col0, void* stream);

int aliby_features_sizeshape(aliby_ctx* ctx, const uint16_t* labels, int F, int Y, int X,
                             const aliby_object* table_dev, int n_obj, int max_h, int max_w,
                             int max_area, double* out, int ld, int col0, void* stream);

/* cp_measure "feret" (get_core_measurements()["feret"], default feature list pipe_builder.py:49-56):
 * out[:, col0] = MinFeretDiameter, out[:, col0+1] = MaxFeretDiameter. */
int aliby_features_feret(aliby_ctx* ctx, const uint16_t* labels, int F, int Y, int X,
                         const aliby_object* table_dev, int n_obj, int max_h, double* out, int ld,
                         int col0, void* stream);

/* Minimum enclosing circle of each object's pixel centres (centrosome.cpmorphology.
 * minimum_enclosing_circle, used by the Zernike families): mec_dev[n_obj][4] = (centre_i, centre_j,
 * radius, n_hull_vertices) in tile coordinates. */
int aliby_object_mec(aliby_ctx* ctx, const uint16_t* labels, int F, int Y, int X,
                     const aliby_object* table_dev, int n_obj, int max_h, double* mec_dev, void* stream);

/* cp_measure "zernike" (weighted=0: 30 columns, |sum Z_nm|/(pi r^2)) and "radial_zernikes"
 * (weighted=1: 30 magnitudes |sum I Z_nm|/n_pixels then 30 phases atan2(Re,Im)); n<=9. */
int aliby_features_zernike(aliby_ctx* ctx, const uint16_t* labels, const void* planes, int dtype,
                           int F, int C, int Y, int X, int channel, const aliby_object* table_dev,
                           int n_obj, const double* mec_dev, int weighted, double* out, int ld, int col0,
                           void* stream);
/* radial_zernikes (the weighted form above) of 2..5 channels of the same planes in ONE launch: the unit-disc coordinates, the
 * powers (y + ix)^m and the radial polynomials of a pixel are evaluated once and applied to every channel's weight.
 * channels[i] -> out[:, col0s[i] .. col0s[i] + 60); same numbers as n_channels calls of aliby_features_zernike(weighted = 1). */
int aliby_features_radial_zernikes_multi(aliby_ctx* ctx, const uint16_t* labels, const void* planes, int dtype, int F, int C, int Y,
                                         int X, const int* channels, const int* col0s, int n_channels, const aliby_object* table_dev,
                                         int n_obj, const double* mec_dev, double* out, int ld, void* stream);

/* cp_measure "texture": 13 Haralick statistics x 4 directions (direction-major, 52 columns) of the
 * object's bbox crop quantised to 8-bit grey levels (uint16 >> 8; ALIBY_U8W: the value; [0,1] floats -> rint(255 f)),
 * co-occurrence distance `scale` (3), zero grey level ignored (mahotas ignore_zeros=True). */
int aliby_features_texture(aliby_ctx* ctx, const uint16_t* labels, const void* planes, int dtype,
                           int F, int C, int Y, int X, int channel, const aliby_object* table_dev,
                           int n_obj, int max_h, int max_w, int max_area, int scale, int gray_levels,
                           double* out, int ld, int col0, void* stream);

/* cp_measure "radial_distribution" (scaled rings, centre = the object itself), two steps:
 *  1. aliby_radial_geometry: channel-independent ring/wedge code of every object pixel, written into
 *     binmap_dev [F,Y,X] (0x80 | wedge<<4 | ring; 0 = not reached from the centre).  Paths are followed however far
 *     they wind; an object of more than 65536 pixels with a path of more than 65535 edge or 65534 diagonal steps gets
 *     0 on every pixel, and step 2 then writes NaN in all its columns;
 *  2. aliby_features_radial_distribution: per channel, 3*bin_count columns
 *     FracAtD_1..n, MeanFrac_1..n, RadialCV_1..n. */
int aliby_radial_geometry(aliby_ctx* ctx, const uint16_t* labels, int F, int Y, int X,
                          const aliby_object* table_dev, int n_obj, int max_h, int max_w, int bin_count,
                          uint8_t* binmap_dev, void* stream);
int aliby_features_radial_distribution(aliby_ctx* ctx, const uint16_t* labels, const uint8_t* binmap_dev,
                                       const void* planes, int dtype, int F, int C, int Y, int X,
                                       int channel, const aliby_object* table_dev, int n_obj,
                                       int bin_count, double* out, int ld, int col0, void* stream);
/* The same with `scaled=False` (CellProfiler's unscaled bins): rings of maximum_radius / bin_count pixels of centre distance,
 * everything beyond maximum_radius in an overflow ring.  aliby_radial_geometry_unscaled writes ring `bin_count` for those
 * pixels; aliby_features_radial_distribution_rings with rings_out = bin_count + 1 reports it as a last column of each of
 * FracAtD / MeanFrac / RadialCV (3 * rings_out columns; rings_out = bin_count is the scaled call above). */
int aliby_radial_geometry_unscaled(aliby_ctx* ctx, const uint16_t* labels, int F, int Y, int X,
                                   const aliby_object* table_dev, int n_obj, int max_h, int max_w, int bin_count,
                                   double maximum_radius, uint8_t* binmap_dev, void* stream);
int aliby_features_radial_distribution_rings(aliby_ctx* ctx, const uint16_t* labels, const uint8_t* binmap_dev,
                                             const void* planes, int dtype, int F, int C, int Y, int X,
                                             int channel, const aliby_object* table_dev, int n_obj,
                                             int bin_count, int rings_out, double* out, int ld, int col0, void* stream);

/* ---- a15: the reference's in-repo per-cell metrics ------------------------ */
/* extraction/core/functions/cell.py:18-303.  17 columns: area, centroid_x, centroid_y, conical_volume,
 * eccentricity, spherical_volume, volume, min_ax, maj_ax (min_maj_approximation), mean, median, std, total,
 * total_squared, max2p5pc, max5px_median, moment_of_inertia.  planes may be NULL (mask-only metrics). */
int aliby_features_cell(aliby_ctx* ctx, const uint16_t* labels, const void* planes, int dtype, int F, int C,
                        int Y, int X, int channel, const aliby_object* table_dev, int n_obj, int max_h,
                        int max_w, int max_area, double* out, int ld, int col0, void* stream);

/* cell.ratio (src/extraction/core/functions/cell.py:268-279): out[n_obj] = median over the object of channel0 / channel1 (true
 * division), NaN when any channel1 pixel of the object is 0 or the object is empty. */
int aliby_features_cell_ratio(aliby_ctx* ctx, const uint16_t* labels, const void* planes, int dtype, int F, int C, int Y,
                              int X, int channel0, int channel1, const aliby_object* table_dev, int n_obj, int max_area,
                              double* out, void* stream);
/* custom/localisation.py:75-120, nuc_est_conv: out[row * ld + col0] = the maximum over the tile of the object's median-subtracted
 * pixels (0 outside the object) convolved ("same") with a Gaussian sized to the expected nucleus, divided by
 * sum(h^2) alpha pi chi sigma^2, where N = the object's non-zero pixels, r = sqrt(object_radius_estimation N / pi), the filter
 * half-width ceil(2 r), chi = -2 ln(1 - alpha) and sigma = gaussian_sigma, or r / sqrt(chi) when gaussian_sigma <= 0.
 * median_dev [dev] holds one float64 per object: its np.median (column 10 of aliby_features_cell).  NaN for an absent label and,
 * with a derived sigma, for an object without a non-zero pixel.  alpha outside (0, 1), object_radius_estimation <= 0 or a
 * non-finite gaussian_sigma is ALIBY_ERR_INVALID.  Working set and launch forms: csrc/feat_localisation.hip. */
int aliby_features_nuc_est_conv(aliby_ctx* ctx, const uint16_t* labels, const void* planes, int dtype, int F, int C, int Y,
                                int X, int channel, const aliby_object* table_dev, int n_obj, int max_h, int max_w,
                                int max_area, const double* median_dev, double alpha, double object_radius_estimation,
                                double gaussian_sigma, double* out, int ld, int col0, void* stream);
/* custom/localisation.py:123-140, nuc_conv_3d: the Z-stack sibling of nuc_est_conv.  stack is [F,C,Z,Y,X] (ALIBY_U16 or ALIBY_F32);
 * the object's 2-D mask is repeated on every plane.  out[row * ld + col0] = the maximum over the [Z,Y,X] stack of the object's
 * median-subtracted voxels (0 off the mask) convolved ("same") with the reference's gauss3D of half-width ceil(2 r) on all three
 * axes, divided by sum(h^2) 0.95 pi chi sd^2, where N = the object's non-zero voxels, r = sqrt(0.085 N / pi),
 * chi = -2 ln(0.05), sd = r / sqrt(chi); the filter's exponents are x^2 / (2 sd), y^2 / (2 sd), z^2 / (2 sd z_spacing / pixel_size),
 * as the reference writes them.  N and the median are found in the kernel.  NaN for an absent label and for an object without a
 * non-zero voxel.  Z < 1, or a pixel_size or z_spacing that is not positive and finite, is ALIBY_ERR_INVALID.  Working set and
 * launch forms: csrc/feat_localisation.hip. */
int aliby_features_nuc_conv_3d(aliby_ctx* ctx, const uint16_t* labels, const void* stack, int dtype, int F, int C, int Z, int Y,
                               int X, int channel, const aliby_object* table_dev, int n_obj, int max_h, int max_w, int max_area,
                               double pixel_size, double z_spacing, double* out, int ld, int col0, void* stream);
/* "neighbors": CellProfiler's MeasureObjectNeighbors with the objects as their own neighbours (among cp_measure's multi-mask
 * measurements; not bound by the reference's loader).  PARITY UNPINNED: recalled from CellProfiler 4's measureobjectneighbors.py and
 * centrosome's outline / strel_disk, neither of which can be run beside this library (tests/neighbors_ref.py restates it).
 * Per tile [Y,X] (labels 1..n, 0 = background), object L, integer distance d in 1..64: S = the offsets with
 * dy^2 + dx^2 <= d^2 (strel_disk(d)), T = those with dy^2 + dx^2 <= d^2 + d (strel_disk(d + 0.5)); offsets that leave the frame are
 * dropped; the outline of L = its pixels on the frame's first / last row or column or with an 8-neighbour of another value.
 * out[row * ld + col0 + k], k = 0..6:
 *   0 NumberOfNeighbors: distinct labels not in {0, L} at q + o, q a pixel of L, o in S
 *   1 PercentTouching: double(t) / double(p) * 100; p = outline pixels, t = those with a label not in {0, L} at q + o, o in T
 *   2, 3 FirstClosestObjectNumber, FirstClosestDistance; 4, 5 SecondClosest...: centres (sum y / area, sum x / area) from exact
 *     64-bit sums and one float64 division each; candidates = the other present labels of the tile, ranked by dy dy + dx dx in
 *     float64, ties to the lower label; distance = sqrt(key).  No first candidate: 2-3 are 0; no second: 4-6 are 0.
 *   6 AngleBetweenNeighbors: atan2(|v1 x v2|, v1 . v2) 180 / pi for the vectors from L's centre to the two centres, NaN when one
 *     is zero (CellProfiler: arccos of the normalised dot product — the same angle, ill-conditioned near 0 and 180 degrees; the
 *     departure is deliberate).
 * A label of 1..n without pixels: NaN in all seven, never a neighbour or a candidate.  A label above its tile's table count (a
 * wrong max_labels hint) is not counted.  Not built: "Expand until adjacent", neighbours from a second object set.
 * offsets_dev [dev, F + 1]: the table's row offsets (row offsets[tile] + l - 1 is label l); max_count: the largest tile's rows;
 * centres_dev [dev, n_obj x 2 float64]: workspace, holds the centres (y, x) afterwards.  Two launches on `stream`; ctx scratch is
 * not used, so the call may run beside other launches of the context.  n_obj == 0 launches nothing.  distance outside 1..64 is
 * ALIBY_ERR_INVALID (the cap bounds the per-pixel scan).  Kernels: csrc/feat_neighbors.hip. */
int aliby_features_neighbors(aliby_ctx* ctx, const uint16_t* labels, int F, int Y, int X, const aliby_object* table_dev, int n_obj,
                             int max_h, int max_w, const int32_t* offsets_dev, int max_count, int distance, double* centres_dev,
                             double* out, int ld, int col0, void* stream);
/* "relate": two object sets of one tile read together — CellProfiler's RelateObjects and IdentifyTertiaryObjects.  PARITY UNPINNED:
 * recalled from CellProfiler 4's relateobjects.py and identifytertiaryobjects.py and centrosome's outline, none of which can be run
 * beside this library (tests/relate_ref.py restates it).
 * Per tile, A and B are two label images of one shape [Y,X]: uint16, 0 = background, labels 1..n_A and 1..n_B, a label may be absent
 * (area 0).  Row L of A relative to B, out[row * ld + col0 + k], k = 0..4:
 *   0 Parent: the label p >= 1 of B that covers the most pixels of L, ties to the smallest p; 0 when no pixel of L has a non-zero B
 *     label, or when L is absent
 *   1 ParentOverlap: that pixel count, an exact integer; 0 without a parent (an extension: the number Parent is the argmax of)
 *   2 Children count: the B objects whose Parent in A, under the same rule with the roles swapped, is L
 *   3 Distance_Centroid: centres (sum y / area, sum x / area) from exact 64-bit sums and one float64 division each, as the
 *     `neighbors` family's; dy = py - cy, dx = px - cx (parent minus L), sqrt(dy dy + dx dx); NaN without a parent
 *   4 Distance_Minimum: the smallest sqrt(dy dy + dx dx) from the centre of L to the centre (y, x) of an outline pixel of its parent,
 *     dy = y - cy, dx = x - cx: the minimum over the squares first, then one sqrt (order-free).  The outline is the `neighbors`
 *     family's: pixels of the parent on the first or last row or column of the tile, or with an 8-neighbour of another value.  NaN
 *     without a parent.
 * Every float64 operation is rounded on its own (-ffp-contract=off); columns 0-2 are integers.
 * The tertiary image T(outer, inner, shrink_inner): T[q] = outer[q] where inner[q] == 0, or where shrink_inner is set and q is an
 * outline pixel of its inner object; 0 elsewhere.  It keeps outer's labels (a row of the new compartment joins its outer object on the
 * label), removes the interior of ANY inner object, not only the outer object's own child (as CellProfiler does), and a label that
 * loses all its pixels is simply absent.
 * Worked example, a 6 x 8 tile.  B = cells: 1 on columns 0..3, 2 on columns 4..7, all rows.  A = nuclei: 1 on rows 1..2 x columns 1..2,
 * 2 on rows 3..4 x columns 3..4, 3 on row 0 x columns 6..7.
 *   nucleus  Parent  ParentOverlap  Children  Distance_Centroid  Distance_Minimum
 *   1        1       4              1         1                  sqrt(2.5)
 *   2        1       2              1         sqrt(5)            sqrt(0.5)     (a tie, 2 pixels in either cell: the smaller label)
 *   3        2       2              0         sqrt(7.25)         0.5
 *   cell     Parent  ParentOverlap  Children
 *   1        1       4              2
 *   2        2       2              1                                          (nuclei 2 and 3 tie at 2 pixels)
 * Tertiary areas of cells 1 and 2: 18 and 20 with shrink_inner = 0; 24 and 24 with shrink_inner = 1 (every pixel of these small
 * nuclei is an outline pixel).  A 3 x 3 nucleus loses exactly its one interior pixel.
 * Not built: per-parent means of child measurements, "Expand until adjacent" and `neighbors` against a second object set.  (Volume
 * labels: aliby_features_relate3d below.)
 *
 * The relate entry fills both directions in one call: rows of A relative to B into out_a, rows of B relative to A into out_b; either
 * may be NULL (both directions are still computed: column 2 of one needs the parents of the other).  table_*: device tables of the
 * two label blocks [F,Y,X] with n_* rows and largest boxes max_h_* x max_w_*; offsets_*_dev [dev, F + 1]: their row offsets (row
 * offsets[tile] + l - 1 is label l); max_count_*: the largest tile's rows, which sizes the per-workgroup counters — one int per
 * label of the other set's tile, in LDS up to 32 KiB and in ctx scratch above (same bits): no cap on how many objects one object may
 * meet.  work_dev [dev]: the bytes the workspace function below returns for (n_a, n_b), 8-byte aligned.  A label above its tile's
 * table count (a wrong max_labels hint) is not counted.  n_a == n_b == 0 launches nothing.  Kernels: csrc/feat_relate.hip. */
size_t aliby_relate_workspace_bytes(int n_a, int n_b);
int aliby_features_relate(aliby_ctx* ctx, const uint16_t* labels_a, const uint16_t* labels_b, int F, int Y, int X,
                          const aliby_object* table_a, int n_a, int max_h_a, int max_w_a, const aliby_object* table_b, int n_b,
                          int max_h_b, int max_w_b, const int32_t* offsets_a_dev, int max_count_a, const int32_t* offsets_b_dev,
                          int max_count_b, void* work_dev, double* out_a, int ld_a, int col0_a, double* out_b, int ld_b, int col0_b,
                          void* stream);
/* The tertiary image of outer and inner [dev, F x Y x X uint16] into out (same shape; must not alias an input).  One pass, 6 bytes of
 * algorithmic traffic per pixel; 16-byte accesses where X is a multiple of 8 and the three pointers are 16-byte aligned. */
int aliby_tertiary_labels(aliby_ctx* ctx, const uint16_t* outer, const uint16_t* inner, int F, int Y, int X, int shrink_inner,
                          uint16_t* out, void* stream);
/* "secondary": CellProfiler's IdentifySecondaryObjects, method "Distance - N" — every primary object grows by up to N pixels into the
 * background, and the grown pixels carry its label, so a secondary row joins its primary on the label.  CellProfiler computes it as
 * scipy.ndimage.distance_transform_edt(labels == 0, return_indices=True) and labels_out[dist <= N] = labels_in[i, j]
 * (skimage.segmentation.expand_labels).  This is that function, except that where several labelled pixels are equally near SciPy's
 * index depends on its sweep order and this library takes the smaller label (tests/secondary_ref.py restates the definition;
 * tests/test_cpu_secondary_ref.py holds it against SciPy on every pixel that is not such a tie).
 * Every tile f of primary [dev, F x Y x X uint16, 0 = background] is handled on its own.  For a pixel p:
 *   primary[p] != 0: out[p] = primary[p]
 *   else let m be the smallest integer |p - q|^2 over the pixels q of the same tile with primary[q] != 0:
 *     no such q, or m > N^2: out[p] = 0      (sqrt(m) <= N and m <= N^2 are one test for an integer N)
 *     else: out[p] = min{ primary[q] : |p - q|^2 = m }      (ties go to the smaller label: order-free)
 * Labels keep the primary numbering and 65535 is a label like any other; nothing crosses a tile edge; everything is integer
 * arithmetic, so a tile's output carries the same bits whatever the batch, the launch form and the stream.
 * Worked examples, one row of 9 pixels and one tile of 6 x 6:
 *   [7 0 0 0 3 0 0 0 0] with N = 2 -> [7 7 3 3 3 3 3 0 0]   (pixel 2 is 2 from either object: m = 4 for both, the smaller label 3)
 *   a lone pixel of label 9 at (0, 0), N = 5: (3, 4) is 9 (m = 25 <= 25), (4, 4) is 0 (m = 32), (5, 0) is 9, (5, 1) is 0 (m = 26).
 * distance = N in 1..64, else ALIBY_ERR_INVALID (the cap bounds the per-pixel scan; it is not a structural limit).  workspace [dev,
 * 4-byte aligned]: the caller's, at least aliby_secondary_workspace_bytes(F, Y, X) = 4 F Y X bytes (one packed word per pixel: the
 * vertical distance to the column's nearest labelled pixel and its label); a smaller one, and out == primary, are ALIBY_ERR_INVALID.
 * F * Y * X == 0 is a successful no-op.  Uses no context scratch and does not wait for `stream`.  Two launches; 2 B read, 4 B + 4 B
 * through the workspace and 2 B written per pixel; per-pixel work linear in N.  Not built: "Watershed", discarding objects on the
 * border.  ("Propagation" and "Distance - B": aliby_propagate_labels.  Volume labels: aliby_secondary_volume.)  Kernels:
 * csrc/feat_secondary.hip. */
size_t aliby_secondary_workspace_bytes(int F, int Y, int X);
int aliby_secondary_labels(aliby_ctx* ctx, const uint16_t* primary, int F, int Y, int X, int distance, void* workspace,
                           size_t workspace_bytes, uint16_t* out, void* stream);
/* "secondary" on volume labels: the same function one dimension up, on an integer lattice.  It is
 * scipy.ndimage.distance_transform_edt(vol == 0, sampling=(sz, sy, sx), return_indices=True) and out[dist <= N] = vol[idx]
 * (skimage.segmentation.expand_labels(..., spacing=)), with the same tie rule as above: the smaller label (tests/secondary3d_ref.py
 * restates the definition; tests/test_cpu_secondary3d_ref.py holds it against SciPy on every voxel that is not a tie).
 * Every stack f of primary [dev, F x Z x Y x X uint16, 0 = background] is handled on its own.  With the integer spacing (sz, sy, sx)
 * and d2(p, q) = (sz dz)^2 + (sy dy)^2 + (sx dx)^2, an integer, for a voxel p:
 *   primary[p] != 0: out[p] = primary[p]
 *   else let m be the smallest d2(p, q) over the voxels q of the same stack with primary[q] != 0:
 *     no such q, or m > N^2: out[p] = 0
 *     else: out[p] = min{ primary[q] : d2(p, q) = m }
 * Labels keep the primary numbering, so no object can vanish and a grown row joins its primary on the label; 65535 is a label like any
 * other; nothing crosses a stack edge; everything is integer arithmetic, so a stack's output carries the same bits whatever the batch,
 * the launch form and the stream.  With Z == 1, spacing (1, 1, 1) and N <= 64 it is aliby_secondary_labels on the one plane, bit for
 * bit.  Worked examples ((z, y, x) coordinates):
 *   labels 9 at (1, 2, 2) and 4 at (3, 0, 0), unit spacing, N = 3: (0, 0, 0) is 4 (m = 9 for both: 1 + 4 + 4 = 9 + 0 + 0, the smaller
 *     label); with N = 2 it is 0.
 *   spacing (3, 1, 1), N = 3, labels 7 at (0, 5, 5) and 2 at (1, 5, 8): (1, 5, 5) is 2 (one plane = 3 = three pixels); (0, 5, 8) is 2
 *     (the same tie seen from the other side); (1, 5, 4) is 0 (9 + 1 = 10 > 9 through the plane, 16 > 9 along the row: neither
 *     reaches); (0, 5, 2) is 7 (m = 9), (2, 5, 8) is 2 (m = 9), (3, 5, 8) is 0 (m = 36).
 *   spacing (13, 5, 5), N = 25: a voxel grows 5 pixels in its plane (m = 625) and one plane up or down (m = 169), and from the
 *     neighbouring plane 4 pixels (169 + 400 = 569) but not 5 (169 + 625 = 794 > 625).
 * distance = N in 1..255 and every spacing component in 1..255 (N^2 <= 65025 fits the 16-bit field of the packed key
 * (d2 << 16) | label below the 0xffffffff sentinel), and the reach N / s_a at most 64 voxels on every axis (it bounds the scans; not a
 * structural limit); else ALIBY_ERR_INVALID.  A float spacing is not offered: real stacks are anisotropic in small ratios (0.6 um per
 * plane over 0.23 um per pixel is about 13 : 5 : 5), and with integer steps every distance is an exact integer.  workspace [dev,
 * 4-byte aligned]: the caller's, at least aliby_secondary_volume_workspace_bytes(F, Z, Y, X) = 8 F Z Y X bytes (two packed words per
 * voxel: the z pass's and the y pass's); a smaller one, and out == primary, are ALIBY_ERR_INVALID, and no refused call writes
 * anything.  F * Z * Y * X == 0 is a successful no-op that needs no buffers.  Uses no context scratch and does not wait for `stream`.
 * Three launches (a z walk, a y scan, an x scan); 2 B read, 4 B + 4 B and 4 B + 4 B through the workspace and 2 B written per voxel
 * (20 B); per-voxel work linear in the reach.  Not built: "Propagation" and "Distance - B" on volumes (2-D: aliby_propagate_labels),
 * "Watershed", a float spacing, "Expand until adjacent", discarding objects on the border.  Kernels: csrc/feat_secondary3d.hip. */
size_t aliby_secondary_volume_workspace_bytes(int F, int Z, int Y, int X);
int aliby_secondary_volume(aliby_ctx* ctx, const uint16_t* primary, int F, int Z, int Y, int X, int distance, int sz, int sy, int sx,
                           void* workspace, size_t workspace_bytes, uint16_t* out, void* stream);
/* "propagate": CellProfiler's IdentifySecondaryObjects, method "Propagation" (its default) — the primary labels grow along a stain:
 * a pixel takes the label of the seed it reaches most cheaply over a metric that charges for grey-level differences, and a threshold
 * on the stain says where the cells end.  centrosome's `propagate` works in float64 with a priority queue: its result on ties follows
 * the queue order, and float sums follow the order of relaxation.  Here the metric is an exact integer, so every relaxation order
 * reaches the same unique fixed point and a tile carries the same bits whatever the batch, the launch form and the stream
 * (tests/propagate_ref.py restates the definition as a heap Dijkstra in Python integers and as a Jacobi iteration).  PARITY UNPINNED:
 * the 1/16-grey-level quantisation, ties to the smaller label and >= for the threshold are this library's.
 * Every tile f of primary [dev, F x Y x X uint16, 0 = background] and image [dev, F x Y x X uint16] is handled on its own.
 *   lambda2 = L = llrint((regularization * image_max)^2), computed by the caller in float64 (features.propagate_args); at most 2^40.
 *   A pixel p is passable iff primary[p] != 0, or image[p] >= threshold and (distance == 0, or some labelled pixel of the tile lies
 *     within `distance` of p: aliby_secondary_labels(primary, distance)[p] != 0).
 *   Passable pixels are joined to their passable 8-neighbours of the same tile.  For neighbours p, q:
 *     P(p,q) = sum over o in {-1,0,1}^2 of |image[clamp(p+o)] - image[clamp(q+o)]|, each coordinate clamped to the tile on its own
 *       (centrosome's clamped_fetch); an integer <= 9 * 65535.
 *     m = |dy| + |dx|, 1 or 2.
 *     W(p,q) = isqrt(256 (P^2 + m L)), the floor of the exact root: CellProfiler's sqrt(P^2 + m lambda^2) in sixteenths of a grey
 *       level.  W is symmetric.
 *   D[p] = the minimum over paths from any labelled pixel to p of the sum of W; 0 on labelled pixels.
 *   out[p] = the smallest label among the seeds that reach p at exactly D[p].  Labelled pixels keep their label: they are sources
 *     only (it matters where L = 0 on a flat stain lets another seed arrive at distance 0).
 *   A pixel that is not passable, or has no path, gets out = 0 and D = 2^64 - 1.
 * Y * X <= 2^23, else ALIBY_ERR_INVALID: with that bound D < 2^48 and (D << 16) | label fits one 64-bit word, the key the kernels
 * minimise.  Nothing crosses a tile edge; 65535 is a label like any other.  "Distance - B" is threshold = 0 with distance = N: the
 * reachable set is that of "Distance - N" (the digital segment to the nearest seed stays within N) and the stain only divides it.
 * Worked examples:
 *   regularization 0.05, image_max 65535: L = llrint(3276.75^2) = 10 737 091.  On a flat image P = 0: a straight step costs
 *     isqrt(256 L) = 52 428, a diagonal one isqrt(512 L) = 74 144 (two straight steps cost more: paths cut corners).
 *   the row [7 0 0 0 0 0 0 0 3] on a flat image: D = [0 52428 104856 157284 209712 157284 104856 52428 0], out = [7 7 7 7 3 3 3 3 3]
 *     (the middle pixel is 4 steps from either seed: the smaller label).
 *   P at the corner (0, 0) of a tile towards (0, 1): the offsets o = (., -1) of p read column 0 (clamped), those of q columns 0, 1, 2,
 *     and the offsets o = (-1, .) read row 0 again: P = 2 (|I00 - I00| + |I00 - I01| + |I01 - I02|) + (|I10 - I10| + |I10 - I11| +
 *     |I11 - I12|).
 * threshold in 0..65535, distance 0 (none) or in 1..64, else ALIBY_ERR_INVALID.  workspace [dev, 8-byte aligned]: the caller's, at
 * least aliby_propagate_workspace_bytes(F, Y, X) = 32 F Y X + 256 bytes (two key buffers, four weight planes, the flags; with a
 * distance the reach pass's words lie over the weight planes); a smaller one, and out_labels == primary, are ALIBY_ERR_INVALID, and no
 * refused call writes anything.  F * Y * X == 0 is a successful no-op that needs no buffers.  out_dist [dev, F x Y x X uint64] may be
 * NULL.  stats_host [host, int32 x 2] may be NULL: the rounds that changed a key, and the reads of the change flags.  A round runs
 * every 32 x 32 region of every tile to its fixed point inside LDS against a halo from the buffer no region writes; the call reads the
 * flags of eight rounds at a time and so waits on `stream`.  More than Y * X + 1 changing rounds is ALIBY_ERR_TOO_LARGE, never a
 * result (found at the read of the flags that passes the bound, up to seven rounds later; stats_host then holds the counts so far;
 * every other refusal leaves it zero).  Uses no context scratch.  (A threshold per tile: aliby_propagate_labels_per_tile, below.)  Not built: filling holes, discarding border objects, float32 images, a
 * volume form.  Kernels: csrc/feat_propagate.hip. */
size_t aliby_propagate_workspace_bytes(int F, int Y, int X);
int aliby_propagate_labels(aliby_ctx* ctx, const uint16_t* primary, const uint16_t* image, int F, int Y, int X, int threshold,
                           uint64_t lambda2, int distance, void* workspace, size_t workspace_bytes, uint16_t* out_labels,
                           uint64_t* out_dist, int32_t* stats_host, void* stream);
/* aliby_propagate_labels with one threshold per tile: thresholds [dev, F int32] stands where `threshold` stood, and k_propagate_weights
 * reads thresholds[f] for tile f on the device — the output of aliby_auto_threshold on the same stream, never read back.  The values
 * are not range-checked: one above 65535 means that no unlabelled pixel of that tile is passable, a negative one that all are.
 * thresholds == NULL is ALIBY_ERR_INVALID (unless F * Y * X == 0); everything else is aliby_propagate_labels', the workspace included. */
int aliby_propagate_labels_per_tile(aliby_ctx* ctx, const uint16_t* primary, const uint16_t* image, int F, int Y, int X,
                                    const int32_t* thresholds, uint64_t lambda2, int distance, void* workspace, size_t workspace_bytes,
                                    uint16_t* out_labels, uint64_t* out_dist, int32_t* stats_host, void* stream);
/* "auto threshold": the threshold a `propagate` call takes, computed per tile on the device — CellProfiler's automatic threshold,
 * method Otsu with two or three classes, its correction factor and its bounds.  PARITY UNPINNED: CellProfiler, scikit-image and
 * centrosome bin 0..1 floats into 256 classes after a log transform; here the two-class search is over all 65 536 grey levels, the
 * three-class search over 256 bins of the occupied range, and the criterion's order of operations is this library's.
 * Every tile f of image [dev, F x Y x X uint16] is handled on its own.  h[v] = the number of pixels of grey level v among all Y * X
 * pixels (labelled ones included); lo, hi = the smallest and largest v with h[v] > 0.  Counts and sums of v h[v] are exact integers
 * below 2^48 (Y * X < 2^32), so each converts to float64 exactly; every float64 operation below is IEEE round-to-nearest, in the
 * order written, without contraction.
 *   Two classes.  For t in lo + 1 .. hi: class 0 = {v < t}, class 1 = {v >= t}, n_i and s_i their counts and sums of v,
 *     J(t) = (double)s0 * (double)s0 / (double)n0 + (double)s1 * (double)s1 / (double)n1   (maximal where the between-class variance is).
 *     raw = the SMALLEST t that attains the maximum: where empty levels lie between two occupied ones, the level just above the
 *     dark class.  lo == hi (a constant tile): raw = lo.
 *   Three classes.  256 bins over the occupied range: W = hi - lo + 1, bin(v) = ((v - lo) * 256) / W (integer division), per-bin
 *     counts and sums of v from h.  For 0 <= k1 < k2 <= 254: class 0 = bins <= k1, class 1 = bins in (k1, k2], class 2 = bins > k2,
 *     all three non-empty; J = s0^2 / n0 + s1^2 / n1 + s2^2 / n2, each term as above, summed from the left.  The maximum, ties to the
 *     smallest k1, then the smallest k2.  t_i = lo + ceil((k_i + 1) * W / 256), the first grey level of the next bin.  No valid pair
 *     (fewer than three occupied bins): t1 = t2 = the two-class raw threshold.  middle = ALIBY_THRESHOLD_MIDDLE_FOREGROUND takes
 *     raw = t1 (the middle class counts as foreground), ALIBY_THRESHOLD_MIDDLE_BACKGROUND raw = t2.  With two classes t1 = t2 = raw
 *     and `middle` is not used.
 *   thresholds[f] = min(max(llrint(min(raw * correction, 65535.0)), bound_lo), bound_hi): the product in float64, the rounding half
 *     to even.  details [dev, F x 4 int32], may be NULL: (lo, hi, t1, t2), raw.
 * Worked examples (pixels -> raw):
 *   10 x 100 and 10 x 200: every t in 101..200 has the same J; raw = 101.
 *   10 each of 100, 200, 300: the splits after 100 and after 200 tie at J = 1 350 000; raw = 101.  Three classes: W = 201, the bins
 *     of 100, 200, 300 are 0, 127, 254; (k1, k2) = (0, 127): (t1, t2) = (101, 201).
 *   [10, 20, 30]: raw = 11; three classes: W = 21, bins 0, 121, 243: (11, 21).
 *   [0, 65535]: raw = 1; three classes fall back: (1, 1).
 *   [32767, 32768, 32768]: raw = 32768.
 *   raw 101 with correction 0.5: 50.5 rounds to even, 50.
 * classes 2 or 3, middle one of the two constants, correction in (0, 16], 0 <= bound_lo <= bound_hi <= 65535, F <= 65535 and
 * Y * X < 2^32 (the limits of aliby_crop_hist_u16, whose histogram this is), else ALIBY_ERR_INVALID.  workspace [dev, 16-byte
 * aligned]: the caller's, at least aliby_auto_threshold_workspace_bytes(F) = 262144 F bytes (the [F, 65536] uint32 histogram); a
 * smaller one is ALIBY_ERR_INVALID, and no refused call writes anything.  F * Y * X == 0 is a successful no-op that needs no buffers.
 * Stream-ordered: no context scratch, no wait on `stream`.  Not built: minimum cross-entropy (its criterion needs log, which is
 * not bit-reproducible between the device and NumPy: it needs a tolerance of its own), the log transform and smoothing before
 * thresholding, adaptive (windowed) thresholds, one threshold over the whole batch, masks, float32 images.
 * Kernels: csrc/feat_threshold.hip (the search), csrc/tile_crop.hip (the histogram). */
#define ALIBY_THRESHOLD_MIDDLE_FOREGROUND 0
#define ALIBY_THRESHOLD_MIDDLE_BACKGROUND 1
size_t aliby_auto_threshold_workspace_bytes(int F);
int aliby_auto_threshold(aliby_ctx* ctx, const uint16_t* image, int F, int Y, int X, int classes, int middle, double correction,
                         int bound_lo, int bound_hi, void* workspace, size_t workspace_bytes, int32_t* thresholds, int32_t* details,
                         void* stream);
/* trap.imBackground / trap.background_max5 (src/extraction/core/functions/trap.py:6-43): per tile, over the pixels of
 * `channel` under NO mask (labels == 0): out[f*2] = their median (numpy.median), out[f*2+1] = the mean of the five largest
 * (of all of them when fewer); NaN for a tile without background. */
int aliby_features_trap_background(aliby_ctx* ctx, const uint16_t* labels, const void* planes, int dtype, int F, int C,
                                   int Y, int X, int channel, double* out, void* stream);

/* ---- a13 (widening): cp_measure "granularity" ------------------------------ */
/* Bound like every core measurement at src/extraction/core/functions/loaders.py:71-73 (fun(mask, pixels) -> dict of
 * Granularity_1..L); not in the builder's default list (pipe_builder.py:49-56).  CellProfiler's MeasureGranularity: frame
 * subsampled by subsample_size (bilinear), background (erode + dilate with disk(element_size) on a further
 * image_sample_size subsample) removed, then spectrum_length rounds of erode-by-disk(1) + reconstruction-by-dilation;
 * out[obj, col0 + i - 1] = (mean_{i-1} - mean_i) * 100 / max(mean_0, eps) over the object's pixels, mean_0 on the
 * original pixels.  image_mask_objects = 0: the image mask is the frame (CellProfiler's default); 1: labels > 0, sampled
 * bilinearly.  The image-level part runs once per (tile, channel), float64.  `workspace` is device memory of at least
 * aliby_granularity_workspace_bytes(); the call synchronises `stream` while it iterates the reconstruction to its fixed
 * point.  PARITY UNPINNED (oracle/granularity_restated.py; cp_measure is not available offline).  Kernels:
 * csrc/granularity_pass.h (shared with granularity3d), csrc/feat_granularity.hip. */
size_t aliby_granularity_workspace_bytes(int F, int Y, int X, int n_obj, double subsample_size, double image_sample_size);
int aliby_features_granularity(aliby_ctx* ctx, const uint16_t* labels, const void* planes, int dtype, int F, int C, int Y,
                               int X, int channel, const aliby_object* table_dev, int n_obj, double subsample_size,
                               double image_sample_size, int element_size, int spectrum_length, int image_mask_objects,
                               void* workspace, size_t workspace_bytes, double* out, int ld, int col0, void* stream);

/* ---- a14: cp_measure colocalisation -------------------------------------- */
/* Call site wrap_cp_corr_features (loaders.py:153-167): fun(pixels1, pixels2, mask); metric list
 * pipe_builder.py:37.  One launch evaluates any subset of {pearson, manders_fold, rwc, costes} for the
 * channel pair (ch0, ch1); col_* is the first of the metric's two columns or -1 to skip it.
 * thr_percent = 15 and costes_scale_max = 255 are CellProfiler's defaults.  rwc needs ranks_dev / rmax_dev
 * (aliby_object_ranks) for both channels; they may be NULL otherwise. */
int aliby_features_coloc(aliby_ctx* ctx, const uint16_t* labels, const void* planes, int dtype,
                         int F, int C, int Y, int X, int ch0, int ch1,
                         const aliby_object* table_dev, int n_obj, int max_area,
                         double* out, int ld, int col_pearson, int col_manders, int col_rwc,
                         int col_costes, double thr_percent, double costes_scale_max,
                         const uint32_t* ranks_dev, const int32_t* rmax_dev, void* stream);
/* The same metrics for a list of channel pairs in ONE launch: an object's pixels of every channel in use are gathered
 * once and each wave of its workgroup takes pairs in turn (the builder's multi tree is C(5,2) = 10 pairs x 4 metrics,
 * pipe_builder.py:33-43).  pairs_host: n_pairs x 6 ints (ch0, ch1, col_pearson, col_manders, col_rwc, col_costes; -1
 * skips a metric).  Returns ALIBY_ERR_TOO_LARGE, without launching, when the pixel lists exceed the LDS budget: the
 * caller then goes pair by pair through aliby_features_coloc. */
int aliby_features_coloc_pairs(aliby_ctx* ctx, const uint16_t* labels, const void* planes, int dtype, int F, int C,
                               int Y, int X, const int32_t* pairs_host, int n_pairs, const aliby_object* table_dev,
                               int n_obj, int max_area, double* out, int ld, double thr_percent,
                               double costes_scale_max, const uint32_t* ranks_dev, const int32_t* rmax_dev,
                               void* stream);
/* Dense per-object ranks of one channel (CellProfiler's Rank_im of the RWC coefficient): ranks_dev
 * [F,C,Y,X] uint32 receives, at every object pixel, the number of distinct smaller values of that object in
 * `channel`; rmax_dev [n_obj, C] the largest rank.  One sort per (object, channel), shared by all pairs. */
int aliby_object_ranks(aliby_ctx* ctx, const uint16_t* labels, const void* planes, int dtype, int F, int C,
                       int Y, int X, int channel, const aliby_object* table_dev, int n_obj, int max_area,
                       uint32_t* ranks_dev, int32_t* rmax_dev, void* stream);

/* ---- §8f-2: image ingest --------------------------------------------------- */
/* Host-side TIFF decode feeding the stager (aliby_crop_pad_u16).  Replaces the per-file imageio.imread of
 * ImageList.get_data_lazy (src/aliby/io/image.py:395-408), the dask.array.image.imread of ImageDir /
 * ImageMultiTiff (image.py:190, 285) and zarr's chunk decompression behind ImageZarr (image.py:246-259).
 * Baseline TIFF 6.0 and BigTIFF; strips or tiles; compression none / LZW / Deflate / PackBits / Zstandard;
 * horizontal predictor; sample 0 of chunky multi-sample pixels.
 * aliby_tiff_probe: info[12] = pages, width, height, bits, sample_format (1 uint, 2 int, 3 float),
 * samples_per_pixel, compression, predictor, tiled, bigtiff, big_endian, uniform; description receives page 0's
 * ImageDescription (ImageJ hyperstack layout).  Needs no context and no GPU. */
int aliby_tiff_probe(const char* path, int64_t* info, char* description, int description_len);
/* Decode page pages[i] of paths[i] (i < n) into dst + i * plane_stride with a pool of n_threads host threads
 * (<= 0: one per core, at most 16).  dst_is_device = 0: dst is host memory, ctx and stream may be NULL.
 * dst_is_device = 1: every plane is decoded into pinned staging memory and queued for upload on `stream` as soon as
 * its thread finishes, so transfers overlap the remaining decodes; returns after the last upload completed. */
int aliby_ingest_tiff_planes(aliby_ctx* ctx, const char* const* paths, const int32_t* pages, int n, int width,
                             int height, int bytes_per_sample, void* dst, size_t plane_stride, int dst_is_device,
                             int n_threads, void* stream);
/* One compressed zarr chunk -> dst; codec 0 = zlib / gzip, 1 = Zstandard (libzstd.so.1 loaded on first use), 2 = a Blosc
 * version-1 frame (zarr v2's default compressor; blosclz / lz4 / zlib / zstd streams, byte or bit shuffle), decoded by hand. */
int aliby_ingest_inflate(int codec, const void* src, size_t src_bytes, void* dst, size_t dst_bytes,
                         size_t* out_bytes);

/* ---- §8f-3: trap detection -------------------------------------------------- */
/* Building blocks of segment_traps / identify_trap_locations (src/aliby/tile/process_traps.py:24-218), each standing
 * in for one scikit-image call of that file; float64 images, once per position.  aliby_amd/tile/traps.py sequences them.
 * gauss1d: one axis of transform.rescale's anti-aliasing filter (scipy gaussian_filter, mode 'mirror'; truncate = 1
 *   reproduces the integer frame's truncation).  warp: bilinear transform.warp with the 2x3 matrix acting on (col,row),
 *   mode 0 constant / 1 reflect (rescale, rotate).  entropy: filters.rank.entropy with disk(radius).  morph: k x k
 *   max / min (morphology.closing with square(k)).  label: measure.label, 8-connected, label = 1 + raster index of the
 *   first pixel.  region_sums: raw moments per label for regionprops centroid / major_axis_length, and the border flag of
 *   segmentation.clear_border.  match_template: feature.match_template on the median-padded image.  maxfilter1d: the
 *   window maximum of feature.peak_local_max. */
int aliby_trap_gauss1d(aliby_ctx* ctx, const double* in, double* out, int H, int W, int axis,
                       const double* weights_dev, int radius, int truncate, void* stream);
int aliby_trap_warp(aliby_ctx* ctx, const double* in, int H, int W, double* out, int OH, int OW,
                    const double* matrix6_host, int mode, double cval, void* stream);
int aliby_trap_entropy(aliby_ctx* ctx, const uint8_t* in, int H, int W, int radius, double* out, void* stream);
int aliby_trap_morph(aliby_ctx* ctx, const uint8_t* in, uint8_t* out, int H, int W, int lo, int hi, int is_max,
                     void* stream);
int aliby_trap_label(aliby_ctx* ctx, const uint8_t* bw, int H, int W, int32_t* labels, void* stream);
int aliby_trap_region_sums(aliby_ctx* ctx, const int32_t* labels, int H, int W, uint64_t* sums, void* stream);
int aliby_trap_match_template(aliby_ctx* ctx, const double* padded, int PH, int PW, const double* templ, int th,
                              int tw, double* out, int H, int W, double t_mean, double t_ssd, void* stream);
int aliby_trap_maxfilter1d(aliby_ctx* ctx, const double* in, double* out, int H, int W, int axis, int radius,
                           void* stream);

/* ---- round 3 extension: a Z-stack as a volume (BASELINE config 5, "true 3-D"; beyond what the reference wires) -------- */
/* Labels through a per-object table: out[t, p] = lut[offsets[t] + in[t, p] - 1] (0 stays 0): writes the Z-stitched labels
 * (aliby_track_stitch along Z, the reference's stitch_threshold = 0.01 of dispatch.py:193-198) back into the planes.  A
 * label >= 65535 is ALIBY_ERR_OVERFLOW. */
int aliby_labels_apply_lut(aliby_ctx* ctx, const uint16_t* labels_in, int T, int Y, int X, const int32_t* offsets_host,
                           const int32_t* lut_dev, uint16_t* labels_out, void* stream);
/* Per-object intensity statistics over labelled stacks: labels uint16 [F,Z,Y,X] (labels 1..n_f per stack), pixels uint16
 * [F,C,Z,Y,X]; object (f, label) is row offsets_host[f] + label - 1.  12 columns at out[row * ld + col0 ..]: Volume,
 * IntegratedIntensity, MeanIntensity, StdIntensity (population), MinIntensity, MaxIntensity, CenterMassIntensity_X/Y/Z,
 * Center_X/Y/Z.  Exact integer sums: run-to-run deterministic. */
int aliby_features_intensity3d(aliby_ctx* ctx, const uint16_t* labels, const uint16_t* pixels, int F, int C, int Z, int Y,
                               int X, int channel, const int32_t* offsets_host, double* out, int ld, int col0, void* stream);
/* The columns of the 2-D intensity family (aliby_features_intensity) that aliby_features_intensity3d does not give, over the same
 * labelled stacks: labels uint16 [F,Z,Y,X], pixels [F,C,Z,Y,X] of dtype ALIBY_U16 or ALIBY_F32, one channel per call.  The 2-D
 * definitions, applied to the voxels of object (f, label) = row offsets_host[f] + label - 1 in raster order (z, y, x); parity with
 * cp_measure on volumes is unpinned.  13 columns at out[row * ld + col0 ..] with edge = 1, the last 8 of them with edge = 0:
 *   0-4 IntegratedIntensityEdge, MeanIntensityEdge, StdIntensityEdge (population), MinIntensityEdge, MaxIntensityEdge over the edge
 *     voxels.  A voxel of the object is an edge voxel iff at least one of its six face neighbours INSIDE the volume carries another
 *     value: 0, another label, or a label above n_f (skimage find_boundaries, connectivity 1, mode "inner", on the 3-D labels;
 *     neighbours outside the volume do not count: the border is replicated).  An object with voxels but no edge voxel (it fills its
 *     stack) gets 0.0 in all five, as in 2-D.
 *   5 MassDisplacement: sqrt((dx dx + dy dy) + dz dz), d = Location_Center - Location_CenterMassIntensity in voxel indices, both
 *     centres as aliby_features_intensity3d computes them (sums, one rounded division each); NaN when the integrated intensity is 0.
 *   6, 7, 9 LowerQuartileIntensity, MedianIntensity, UpperQuartileIntensity: with the object's n values v sorted ascending and
 *     p = 1/4, 1/2, 3/4: q = n p, i = floor(q), f = q - i; v[i] (1 - f) + v[i + 1] f if i < n - 1, else v[i]; float64 arithmetic
 *     (CellProfiler's rule: n = 2 takes v[1] at 3/4).
 *   8 MADIntensity: the same rule at p = 1/2 on the sorted |v - median|, the difference taken in float64.
 *   10-12 Location_MaxIntensity_X, _Y, _Z: the voxel of the maximum; ties go to the LAST in raster order.
 * ALIBY_U16: every sum is an exact 64-bit integer (the edge variance from n sum v^2 - (sum v)^2 in 128 bits), and the order
 * statistics are exact.  ALIBY_F32: float64 sums in a tree that depends on the object's own voxels only, the edge deviation in a second
 * pass about the mean; NaN pixels give unspecified results.  A label of 1..n_f without voxels gets NaN in every column (the volume
 * families' convention; in the edge columns the 2-D family writes 0).  Labels above n_f are not measured.  Objects of up to
 * aliby_intensity3d_detail_lds_voxels() voxels are measured from LDS, larger ones from global scratch, by the same code: results are
 * bitwise independent of the run, of the other objects of the call and of the batch.  The object table and the larger objects' lists
 * live in the context's scratch, so this is a main-stream call: one in flight per context (the scratch rule, csrc/object_launch.h);
 * it waits for `stream` before it returns.  offsets_host[F] == 0 launches nothing.  Kernel: csrc/feat_intensity3d_detail.hip. */
int aliby_intensity3d_detail_lds_voxels(void);
int aliby_features_intensity3d_detail(aliby_ctx* ctx, const uint16_t* labels, const void* pixels, int dtype, int F, int C, int Z, int Y,
                                      int X, int channel, const int32_t* offsets_host, int edge, double* out, int ld, int col0,
                                      void* stream);
/* Per-object size and shape over the same labelled stacks (uint16 [F,Z,Y,X], object (f, label) = row offsets_host[f] + label - 1).
 * 19 columns at out[row * ld + col0 ..]: Volume, BoundingBoxMinimum_X/Y/Z, BoundingBoxMaximum_X/Y/Z (exclusive),
 * BoundingBoxVolume, Center_X/Y/Z (voxel indices: bit-identical to intensity3d's), Extent, EquivalentDiameter, EulerNumber
 * (of the union of the object's closed voxel cubes, i.e. 26-connected foreground), MajorAxisLength, MinorAxisLength
 * (sqrt(20 c), c the extreme eigenvalues of the population covariance of the coordinates scaled by spacing),
 * InertiaTensorEigenvalues_0/1/2 (of tr(C) Id - C, descending).  spacing = host double[3] (dz, dy, dx), positive; it scales
 * Volume, BoundingBoxVolume, EquivalentDiameter, the axis lengths and the inertia eigenvalues.  A label of 1..n_f without
 * voxels gets Volume 0 and NaN elsewhere.  Exact integer sums: run-to-run deterministic and independent of the batch. */
int aliby_features_sizeshape3d(aliby_ctx* ctx, const uint16_t* labels, int F, int Z, int Y, int X, const int32_t* offsets_host,
                               const double* spacing, double* out, int ld, int col0, void* stream);
/* SurfaceArea of the same labelled stacks, CellProfiler's 3-D MeasureObjectSizeShape column: one float64 per object at
 * out[row * ld + col], rows as in aliby_features_sizeshape3d.  The area of the mesh that scikit-image's
 * marching_cubes(method="lewiner", level=0) builds on the object's mask in its bounding box grown by one voxel and clipped to the
 * volume (mesh_surface_area), computed as the sum over the (Z-1)(Y-1)(X-1) cells of the volume grid of area256[configuration],
 * configuration bit 4 dz + 2 dy + dx = voxel (z + dz, y + dy, x + dx) carries the label.  Counts are exact integers and the sum runs
 * over the configurations in increasing order: bitwise independent of the run and of the batch.  An object on a face of the volume
 * is open there; at level 0 the vertices sit on the outside voxels' centres (one voxel measures 4 sqrt(3)).  A label of 1..n_f
 * without voxels gets NaN, an object that fills the whole volume 0 (scikit-image raises there).  Z, Y, X >= 2.
 * aliby_surface3d_table fills the 256 areas for a spacing (host double[3] (dz, dy, dx), positive) from the triangle table
 * recorded from scikit-image 0.18.3 (csrc/mc_level0_table.h): host arithmetic only, no device is touched. */
int aliby_surface3d_table(const double* spacing_zyx, double* area256);
int aliby_features_surface3d(aliby_ctx* ctx, const uint16_t* labels, int F, int Z, int Y, int X, const int32_t* offsets_host,
                             const double* spacing, double* out, int ld, int col, void* stream);
/* Colocalisation of channel pairs inside the objects of the same labelled stacks: labels uint16 [F,Z,Y,X], pixels [F,C,Z,Y,X] of
 * dtype ALIBY_U16 or ALIBY_F32, pairs_host = n_pairs x (ch0, ch1) with ch0 != ch1 (at most 64).  Over the voxels of object
 * (f, label) = row offsets_host[f] + label - 1 in raster order (z, y, x), the metrics of aliby_features_coloc with the same
 * definitions: pair p writes at out[row * ld + col0 + p * pair_stride + col_<metric>], two columns per metric (Pearson, Slope /
 * Manders_1, _2 / RWC_1, _2 / Costes_1, _2), col_<metric> = -1 skips it.  RWC's dense ranks and Costes' threshold are per
 * object.  A label of 1..n_f without voxels gets NaN in every requested column.  Objects of up to aliby_coloc3d_lds_voxels()
 * voxels are measured from LDS, larger ones from global scratch, by the same code: results are bitwise independent of the run,
 * of the other objects of the call and of the batch. */
int aliby_coloc3d_lds_voxels(void);
int aliby_features_coloc3d(aliby_ctx* ctx, const uint16_t* labels, const void* pixels, int dtype, int F, int C, int Z, int Y, int X,
                           const int32_t* pairs_host, int n_pairs, const int32_t* offsets_host, double* out, int ld, int col0,
                           int pair_stride, int col_pearson, int col_manders, int col_rwc, int col_costes, double thr_percent,
                           double costes_scale_max, void* stream);
/* Haralick texture of one channel inside the objects of the same labelled stacks: labels uint16 [F,Z,Y,X], pixels [F,C,Z,Y,X] of
 * dtype ALIBY_U16 or ALIBY_F32.  Per object (f, label) = row offsets_host[f] + label - 1: grey levels as aliby_features_texture
 * takes them (uint16 >> 8, or rint(255 f) clipped; rescaled to gray_levels), the bounding box in (z, y, x) with every voxel of
 * another label set to 0, and for each of 13 directions the symmetric co-occurrence matrix of the voxel pairs (p, p + scale d)
 * inside the box, pairs touching grey level 0 dropped; the 13 Haralick statistics of aliby_features_texture per direction, 169
 * columns at out[row * ld + col0 ..], direction-major.  Directions d on the axes (z, y, x), in column order: (1,0,0) (1,1,0)
 * (0,1,0) (1,-1,0) (0,0,1) (1,0,1) (0,1,1) (1,1,1) (1,-1,1) (1,0,-1) (0,1,-1) (1,1,-1) (1,-1,-1) (mahotas' order as recalled:
 * unpinned).  A direction without a pair gets 13 NaN, a label of 1..n_f without voxels a row of NaN.  Objects whose bounding box
 * holds up to aliby_texture3d_lds_voxels() voxels are measured from LDS, larger ones from global scratch, by the same code:
 * results are bitwise independent of the run, of the other objects of the call and of the batch. */
int aliby_texture3d_lds_voxels(void);
int aliby_features_texture3d(aliby_ctx* ctx, const uint16_t* labels, const void* pixels, int dtype, int F, int C, int Z, int Y, int X,
                             int channel, const int32_t* offsets_host, int scale, int gray_levels, double* out, int ld, int col0,
                             void* stream);
/* "neighbors3d": the `neighbors` family (aliby_features_neighbors: CellProfiler's MeasureObjectNeighbors with the objects as their
 * own neighbours) on the same labelled stacks.  PARITY UNPINNED: recalled from CellProfiler 4's measureobjectneighbors.py and
 * centrosome's outline / strel_disk, neither of which can be run beside this library (tests/neighbors3d_ref.py restates it).
 * Per stack [Z,Y,X] (labels 1..n, 0 = background), object L, integer distance d in 1..16: S = the offsets with
 * dz^2 + dy^2 + dx^2 <= d^2 (skimage.morphology.ball(d); the 6-neighbour cross for d = 1), T = those with
 * dz^2 + dy^2 + dx^2 <= d^2 + d (the integer-offset form of radius d + 0.5; the 18-neighbourhood for d = 1); offsets that leave the
 * volume are dropped (no wrap, no padding value).  The outline of L is taken plane by plane, as CellProfiler outlines a volume: its
 * voxels on the first / last row or column of their plane or with one of the 8 in-plane neighbours of another value (0 included);
 * the first and last planes are no borders, and the voxels above and below do not make an outline voxel.
 * out[row * ld + col0 + k], k = 0..6, row = offsets_host[f] + L - 1:
 *   0 NumberOfNeighbors: distinct labels v not in {0, L}, v <= n, at q + o, q a voxel of L, o in S
 *   1 PercentTouching: double(t) / double(p) * 100; p = outline voxels, t = those with a non-zero value other than L at q + o, o in
 *     T (a value above n counts here, as in 2-D)
 *   2, 3 FirstClosestObjectNumber, FirstClosestDistance; 4, 5 SecondClosest...: centres (sum z, sum y, sum x) / count from exact
 *     64-bit sums and one float64 division each; candidates = the other present labels of the stack, ranked by
 *     (dz dz + dy dy) + dx dx in float64 (every operation rounded on its own), ties to the lower label; distance = sqrt(key).  No
 *     first candidate: 2-3 are 0; no second: 4-6 are 0.
 *   6 AngleBetweenNeighbors: atan2(|v1 x v2|, v1 . v2) 180 / pi with the 3-D cross product, for the vectors from L's centre to the
 *     two centres, NaN when one is zero (the deliberate departure from CellProfiler's arccos, as in 2-D).
 * A label of 1..n without voxels: NaN in all seven, never a neighbour or a candidate.  Labels above n are not measured and not
 * counted in column 0.  Voxel spacing is not used.  On a stack of one plane every column is aliby_features_neighbors'.
 * Not built: "Expand until adjacent", neighbours from a second object set, physical-unit (anisotropic) balls.
 * Worked example, a stack [4, 6, 8] (z, y, x) at d = 1: A = 1 on z 0..1, y 1..2, x 1..2; B = 2 on z 0..1, y 1..2, x 3..4 (a face
 * shared with A); C = 3 on z 2..3, y 3..4, x 3..4 (it meets B along one edge, across planes: offset (1, 1, 0), in T, not in S).
 *   NumberOfNeighbors 1, 1, 0; PercentTouching 50, 62.5, 25 (every voxel is an outline voxel: 8 each; A's four at x = 2 reach B;
 *   B's four at x = 3 reach A, and of its two at (z 1, y 2), which reach C, (x 4) is a fifth; C's two at (z 2, y 3) reach B).
 *   Centres A (0.5, 1.5, 1.5), B (0.5, 1.5, 3.5), C (2.5, 3.5, 3.5): A -> 2 at 2, 3 at sqrt(12); B -> 1 at 2, 3 at sqrt(8);
 *   C -> 2 at sqrt(8), 1 at sqrt(12); angles atan2(sqrt(32), 4), 90 and atan2(sqrt(32), 8) degrees.
 * centres_dev [dev, offsets_host[F] x 3 float64]: workspace, holds the centres (z, y, x) afterwards.  The object table is built in
 * the context's scratch, so this is a main-stream call: one in flight per context (the scratch rule, csrc/object_launch.h); it
 * waits for `stream` before it returns.  offsets_host[F] == 0 launches nothing.  distance outside 1..16 is ALIBY_ERR_INVALID (the
 * cap bounds the per-voxel scan: a ball of radius 16.5 is about 19 k offsets; it is not a structural limit).  Results are bitwise
 * independent of the run, of the other stacks of the call and of the batch.  Kernels: csrc/feat_neighbors3d.hip. */
int aliby_features_neighbors3d(aliby_ctx* ctx, const uint16_t* labels, int F, int Z, int Y, int X, const int32_t* offsets_host,
                               int distance, double* centres_dev, double* out, int ld, int col0, void* stream);
/* "relate3d": the `relate` family (aliby_features_relate: CellProfiler's RelateObjects) on two sets of labelled stacks, and the
 * tertiary volume.  PARITY UNPINNED: recalled from CellProfiler 4's relateobjects.py and identifytertiaryobjects.py and centrosome's
 * outline, none of which can be run beside this library (tests/relate3d_ref.py restates it).
 * Per stack, A and B are two label volumes of one shape [Z,Y,X]: uint16, 0 = background, labels 1..n_A and 1..n_B from the offsets;
 * a label may be absent; values above the count are not measured and have no counter.  Row L of A relative to B,
 * out[row * ld + col0 + k], k = 0..4, row = offsets[f] + L - 1 — the 2-D family's five columns:
 *   0 Parent: the label p >= 1 of B under the most voxels of L, ties to the smallest p; 0 when no voxel of L lies under a B label in
 *     1..n_B, or when L is absent
 *   1 ParentOverlap: that voxel count, exact; 0 without a parent
 *   2 Children count: the B objects whose Parent in A, by the same rule with the roles swapped, is L
 *   3 Distance_Centroid: centres (sum z, sum y, sum x) / count from exact 64-bit sums and one float64 division each.  With
 *     spacing = (sz, sy, sx): ez = (pz - cz) sz, ey = (py - cy) sy, ex = (px - cx) sx (parent minus L), sqrt((ez ez + ey ey) + ex ex),
 *     every operation rounded on its own (-ffp-contract=off); NaN without a parent
 *   4 Distance_Minimum: the same expression with a voxel (z, y, x) in place of the parent's centre, over the outline voxels of the
 *     parent, reduced with fmin (order-free, exact), then one sqrt; NaN without a parent.  The outline is taken plane by plane, exactly
 *     as neighbors3d defines it: a voxel of p on the first or last row or column of its plane, or with one of its 8 in-plane
 *     neighbours of another value; the first and last planes are no borders, and the voxels above and below do not make an outline
 *     voxel.
 * Consequences.  With Z = 1 and spacing (1, 1, 1), cz = pz = 0.0, so ez = 0, 0 + ey ey is exact and a product with 1.0 is exact:
 * every column carries the bits of aliby_features_relate.  Distances are in the units of `spacing` (positive and finite; anisotropic
 * Z is the normal case for stacks).
 * The tertiary volume T(outer, inner, shrink_inner): T[q] = outer[q] where inner[q] == 0, or where shrink_inner is set and q is a
 * plane-by-plane outline voxel of its inner object; 0 elsewhere.  It keeps outer's labels and counts; a label that loses every voxel
 * is absent.  With the plane-wise outline this is aliby_tertiary_labels over the F * Z planes: call it on the [F * Z, Y, X] view (no
 * entry of its own).  At a nucleus's top and bottom caps the plane-wise rule removes the cap's interior although cytoplasm lies above
 * (below) it, and keeps only the cap's in-plane rim: CellProfiler's way of outlining a volume.
 * Worked example, a stack [3, 6, 8] (z, y, x), spacing (1, 1, 1).  B = cells: 1 on x 0..3, 2 on x 4..7, every plane and row.
 * A = nuclei: 1 on z 0..1, y 1..2, x 1..2; 2 on z 1..2, y 3..4, x 3..4; 3 on z 2, y 0, x 6..7.
 *   nucleus  Parent  ParentOverlap  Children  Distance_Centroid  Distance_Minimum
 *   1        1       8              1         sqrt(1.25)         sqrt(2.75)
 *   2        1       4              1         sqrt(5.25)         sqrt(0.75)    (a tie, 4 voxels in either cell: the smaller label)
 *   3        2       2              0         sqrt(8.25)         0.5
 *   cell     Parent  ParentOverlap  Children  Distance_Centroid  Distance_Minimum
 *   1        1       8              2         sqrt(1.25)         sqrt(0.5)
 *   2        2       4              1         sqrt(5.25)         sqrt(2.5)
 * Tertiary volumes of cells 1 and 2: 60 and 66 voxels with shrink_inner = 0; 72 and 72 with shrink_inner = 1.
 * Not built: per-parent means of child measurements, a batched run_positions form.
 *
 * The entry fills both directions in one call: rows of A relative to B into out_a, rows of B relative to A into out_b; either may be
 * NULL (both directions are still computed: column 2 of one needs the parents of the other).  vol_a, vol_b [dev, F x Z x Y x X
 * uint16]; offsets_a, offsets_b [host, F + 1]: row offsets (offsets[0] = 0, non-decreasing, at most 65535 rows a stack); spacing
 * [host, 3].  The counters are one int per label of the other set's stack, sized from the largest count of the call: in LDS up to
 * 8191 labels and in ctx scratch above (same bits).  The object tables, the per-row workspace and those counters live in the
 * context's scratch, so this is a main-stream call: one in flight per context (the scratch rule, csrc/object_launch.h); it waits for
 * `stream` before it returns.  offsets_a[F] == offsets_b[F] == 0 launches nothing.  A bad shape, F <= 0, offsets that are not
 * monotone or a bad spacing is ALIBY_ERR_INVALID with a message.  Results are bitwise independent of the run, of the other stacks of
 * the call, of the launch form and of the batch.  Kernels: csrc/feat_relate3d.hip. */
int aliby_features_relate3d(aliby_ctx* ctx, const uint16_t* vol_a, const uint16_t* vol_b, int F, int Z, int Y, int X,
                            const int32_t* offsets_a, const int32_t* offsets_b, const double* spacing, double* out_a, int ld_a,
                            int col0_a, double* out_b, int ld_b, int col0_b, void* stream);
/* "granularity3d": the `granularity` family (aliby_features_granularity: CellProfiler's MeasureGranularity) on the same labelled
 * stacks.  PARITY UNPINNED: CellProfiler's volumetric branch, recalled (tests/granularity3d_ref.py restates it).  Everything is
 * float64; every stack [Z,Y,X] of `channel` is on its own, nothing crosses from one stack of the batch into the next:
 *   1. shapes: the subsampled shape is ceil(n * subsample_size) per axis when the size is below 1, else n; the background shape is
 *      the same rule applied to the subsampled shape with image_sample_size.
 *   2. subsample: scipy.ndimage.map_coordinates(order=1) at positions i / subsample_size (a division): trilinear inside [0, n - 1]
 *      on every axis, 0 outside.
 *   3. background: resample again at i / image_sample_size; grey erosion, then grey dilation, with ball(element_size)
 *      (dz^2 + dy^2 + dx^2 <= r^2) under ndimage's "reflect" border (d c b a | a b c d | d c b a, folded as often as the footprint
 *      needs); resize back trilinearly at i * ((b - 1) / (s - 1)); pix = max(subsampled - background, 0).
 *   4. spectrum, spectrum_length times, from ero = pix: ero = grey erosion of ero with ball(1) (the centre and the six face
 *      neighbours) under "reflect"; rec = reconstruction by dilation of ero under pix with the same footprint (voxels outside the
 *      stack never contribute); rec resized to the stack's shape at i * ((s - 1) / (n - 1)); mean_i = its mean over the object's
 *      voxels; out[row * ld + col0 + i - 1] = (mean_{i-1} - mean_i) * 100 / max(mean_0, 2^-52), mean_0 over the ORIGINAL pixels.
 *   5. the one deliberate departure: where the destination axis of a resize has length 1 its coordinate is 0 (CellProfiler's
 *      (m - 1) / (n - 1) is 0 / 0 there).  With it a stack of one plane is aliby_features_granularity with the frame as image mask.
 * The image mask is the whole stack (CellProfiler's default); the "objects" mask of the 2-D entry is not built.
 * row = offsets_host[f] + L - 1; a label of 1..n_f without voxels gets NaN, labels above n_f are not measured.  Y, X and their two
 * sampled lengths must be above 1 (Z and its sampled lengths may be 1); element_size in 1..16 (the cap bounds the per-voxel scan of
 * the ball, about 17 k offsets at 16; it is not a structural limit), spectrum_length in 1..64; else ALIBY_ERR_INVALID.
 * `workspace` is device memory of at least aliby_granularity3d_workspace_bytes(), 8-byte aligned: the images, the object table
 * (count and bounding box per row, csrc/volume_table.h) and the offsets.  The reconstruction runs Jacobi sweeps in chunks of 16
 * between reads of one change flag, so the call waits on `stream` while it iterates (a main-stream call); a step that has not
 * converged after sz * sh * sw / 2 + 64 sweeps is ALIBY_ERR_TOO_LARGE, never a result.  sweeps_host (may be NULL) [spectrum_length]
 * receives the sweeps each step ran (a multiple of 16; flag reads = sweeps / 16).  offsets_host[F] == 0 launches nothing.  Per-object
 * means: one wave per row over the row's bounding box in a fixed lane and reduction order, so results are bitwise independent of the
 * run, of the other stacks of the call and of the batch.  Kernels: csrc/granularity_pass.h (shared with
 * granularity), csrc/feat_granularity3d.hip. */
size_t aliby_granularity3d_workspace_bytes(int F, int Z, int Y, int X, int rows, double subsample_size, double image_sample_size);
int aliby_features_granularity3d(aliby_ctx* ctx, const uint16_t* labels, const void* pixels, int dtype, int F, int C, int Z, int Y, int X,
                                 int channel, const int32_t* offsets_host, double subsample_size, double image_sample_size,
                                 int element_size, int spectrum_length, void* workspace, size_t workspace_bytes, int32_t* sweeps_host,
                                 double* out, int ld, int col0, void* stream);
/* "projection3d": how the collapse of a 3-D label result to 2-D (the maximum over z, then a sequential relabel: the reference's
 * segment/dispatch.py:218-223) sees each object of the same labelled stacks.  For a column (f, y, x), `top` is the maximum of the
 * values labels[f, z, y, x] over z.  Four columns at out[row * ld + col0 ..], row = offsets_host[f] + L - 1:
 *   0 Projection_Area: the number of columns (y, x) of stack f that hold at least one voxel of L.  A label that enters a column
 *     twice, with another value or background in between, counts once.
 *   1 Projection_VisibleArea: the number of columns whose top is L.
 *   2 Projection_VisibleFraction: double(VisibleArea) / double(Area), one float64 division; NaN when Area is 0.
 *   3 Projection_Label: the value the object carries in the collapsed image: the 1-based rank of L among the distinct non-zero
 *     values that are the top of some column of the stack; 0 when L is the top of no column (hidden).
 * A value above n_f gets no row, but it occludes what lies under it and counts in the rank, so Projection_Label is always the value
 * in the collapsed image.  A label of 1..n_f without voxels gets 0, 0, NaN, 0.  Everything but the division is an integer: results
 * are bitwise independent of the run, of the other stacks of the call and of the batch.  Worked example, a stack [2, 1, 4]
 * (z, y, x) with n = 3: z 0 = (1, 1, 3, 0), z 1 = (2, 0, 3, 7): tops 2, 1, 3, 7, ranks 1 -> 1, 2 -> 2, 3 -> 3, 7 -> 4; rows
 * (2, 1, 0.5, 1), (1, 1, 1, 2), (1, 1, 1, 3).  The counts and one presence bit per value and stack live in the context's scratch, so
 * this is a main-stream call: one in flight per context (the scratch rule, csrc/object_launch.h); it waits for `stream` before it
 * returns.  offsets_host[F] == 0 launches nothing.  Y * X < 2^32.  Kernels: csrc/feat_projection3d.hip. */
int aliby_features_projection3d(aliby_ctx* ctx, const uint16_t* labels, int F, int Z, int Y, int X, const int32_t* offsets_host,
                                double* out, int ld, int col0, void* stream);

/* ---- a17: the step API's files, encoded natively (host code, no GPU work) ------------------ */
/* profiles/<name>.parquet — pyarrow.parquet.write_table(profiles, path, compression="zstd")
 * (src/aliby/pipe_core.py:412-413).  One row group, one PLAIN data page per column, fields OPTIONAL with every value
 * present, zstd level `zstd_level` (negative levels are zstd's fast modes; ALIBY_PQ_UNCOMPRESSED: no compression) through
 * libzstd.so.1 (dlopen).  A column's rows come as n_segs
 * segments (a position's table is the concatenation of one slice per object set): values[c * n_segs + s] points at
 * seg_rows[s] items — double / int64 / uint16, or for ALIBY_PQ_STR the Arrow utf8 layout: int32 offsets[seg_rows[s] + 1]
 * with the characters at aux[c * n_segs + s].  Thread-safe (one compression context per calling thread). */
enum { ALIBY_PQ_F64 = 0, ALIBY_PQ_I64 = 1, ALIBY_PQ_U16 = 2, ALIBY_PQ_STR = 3 };
#define ALIBY_PQ_UNCOMPRESSED (-1000000)
typedef struct aliby_pq_column {
  const char* name; /* UTF-8, NUL-terminated */
  int32_t type;     /* ALIBY_PQ_* */
  int32_t reserved;
} aliby_pq_column;
int aliby_parquet_write(const char* path, const aliby_pq_column* cols, int n_cols, const int64_t* seg_rows, int n_segs,
                        const void* const* values, const void* const* aux, int zstd_level);
/* steps/<name>/<step>/<tp:04d>.npz — numpy.savez_compressed(out_file, labels) (src/aliby/io/write.py:25-51): a zip
 * archive of deflated .npy members (version 1.0 headers, C order).  libdeflate.so.0 (dlopen) when present, zlib otherwise. */
typedef struct aliby_npy_member {
  const char* name;     /* "arr_0", "tile_3", ... (".npy" is appended) */
  const char* descr;    /* NumPy dtype string, e.g. "<u2" */
  const int64_t* shape; /* [ndim] */
  const void* data;     /* C-contiguous */
  int32_t ndim;
  int32_t itemsize;     /* bytes per element */
} aliby_npy_member;
int aliby_npz_write(const char* path, const aliby_npy_member* members, int n_members, int level);
/* which of the two optional codec libraries were found on this machine */
int aliby_host_codecs(int* have_zstd, int* have_libdeflate);

/* memcpy of a large host block on `threads` threads (1..16; blocks under 8 MB are copied by the caller's thread): the
 * position-batched runner takes a batch's feature rows (~130 MB) out of its page-locked download arena into memory the returned
 * tables own — one thread pays ~12 ms for that, mostly first-touch page faults, while every writer thread of the batch waits for
 * the table (aliby_amd/runner.py _LazyRows; the reference has no such copy: extract.py:520-599 builds its table from Python
 * lists). */
int aliby_host_copy(void* dst, const void* src, size_t bytes, int threads);

#ifdef __cplusplus
}
#endif
#endif /* ALIBY_HIP_H */
