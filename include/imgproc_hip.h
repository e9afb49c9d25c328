/*
 * imgproc_hip.h — C ABI of libimgproc_hip.so, the MI355X (gfx950) implementation
 * of imgProcessor's per-pixel hot path (undistort / perspective remap, K x K
 * filters, IDW stencils).
 *
 * The reference (radjkarl/imgProcessor, pure Python) has no FFI layer; its
 * boundary for this path is a set of Python call sites into cv2 / numba /
 * scipy.  Each entry point below names the reference call it replaces
 * (paths relative to the reference checkout).  INTEGRATION.md shows the ctypes
 * binding a maintainer would add.
 *
 * Conventions
 *   - plain C types only; every function returns an ipa_status (0 = ok).
 *   - images are row-major [y][x], single channel; pitches are in ELEMENTS.
 *   - `*_dev` functions take DEVICE pointers and enqueue on the context's
 *     stream without synchronising (use ipa_ctx_synchronize / events).
 *     The un-suffixed variants take HOST pointers, stage H2D/D2H through the
 *     context's workspace and return after the result is in host memory.
 *   - batches: n_frames images, consecutive frames `*_frame_stride` ELEMENTS
 *     apart; maps / kernels / matrices are shared by all frames.
 *   - there is NO CPU fallback in this library.  Without a usable gfx950
 *     device ipa_ctx_create fails with IPA_ERR_NO_DEVICE.
 */
#ifndef IMGPROC_HIP_H
#define IMGPROC_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define IPA_VERSION 100 /* 0.1.0 */

typedef enum {
  IPA_OK = 0,
  IPA_ERR_BAD_ARG = -1,
  IPA_ERR_UNSUPPORTED = -2, /* dtype / mode combination not implemented */
  IPA_ERR_HIP = -3,         /* a HIP runtime call failed; see ipa_last_error */
  IPA_ERR_OOM = -4,
  IPA_ERR_NO_DEVICE = -5
} ipa_status;

/* pixel types (transformations.py:78-87 toFloatArray: u8,u16 -> f32) */
typedef enum { IPA_U8 = 0, IPA_U16 = 1, IPA_F32 = 2, IPA_F64 = 3 } ipa_dtype;

/* interpolation; numbering follows cv2.INTER_* where one exists */
typedef enum {
  IPA_INTER_NEAREST = 0,
  IPA_INTER_LINEAR = 1,     /* cv2.INTER_LINEAR   — LensDistortion.py:323 */
  IPA_INTER_CUBIC_CV = 2,   /* cv2.INTER_CUBIC (Keys a=-0.75) — PerspectiveCorrection.py:378 */
  IPA_INTER_LANCZOS4 = 4,   /* cv2.INTER_LANCZOS4 — PerspectiveCorrection.py:404 (always q5) */
  IPA_INTER_CUBIC_KEYS = 5, /* Keys a=-0.5 == skimage.transform.warp(order=3) */
  IPA_INTER_Q5 = 0x100      /* OR-able flag: round coordinates to 1/32 px like cv2 (INTER_BITS=5) */
} ipa_interp;

/* border modes; numbering follows cv2.BORDER_* */
typedef enum {
  IPA_BORDER_CONSTANT = 0,  /* cv2.BORDER_CONSTANT / scipy 'constant' (per-tap blend) */
  IPA_BORDER_REPLICATE = 1, /* scipy 'nearest' */
  IPA_BORDER_REFLECT = 2,   /* fedcba|abcdef: scipy 'reflect', numpy 'symmetric',
                               extendArrayForConvolution 'reflect' */
  IPA_BORDER_WRAP = 3,      /* scipy 'wrap' / 'grid-wrap', extendArray modex='wrap' */
  IPA_BORDER_REFLECT101 = 4 /* scipy 'mirror' */
} ipa_border;

typedef struct ipa_ctx ipa_ctx;     /* one per device; owns a stream + workspace */
typedef struct ipa_event ipa_event; /* HIP event on the context's stream */

/* ---------------------------------------------------------------- runtime */
int ipa_version(void);
const char* ipa_status_string(int status);
/* last error text of this context (or of the calling thread when ctx==NULL) */
const char* ipa_last_error(const ipa_ctx* ctx);
int ipa_device_count(int* count);
/* PCI address "dddd:bb:dd.f" of HIP device `device_id` as this process numbers it (honours
 * HIP_VISIBLE_DEVICES / ROCR_VISIBLE_DEVICES) - for host-side placement of the feeding threads
 * (sharding.numa_cpus_of_device reads /sys/bus/pci/devices/<address>/numa_node).  len >= 16. */
int ipa_device_pci_bus_id(int device_id, char* buf, size_t len);
int ipa_ctx_create(int device_id, ipa_ctx** ctx);
int ipa_ctx_destroy(ipa_ctx* ctx);
int ipa_ctx_synchronize(ipa_ctx* ctx);
/* Launch-shape knobs of a context (csrc/runtime.hip::kTuneNames is the list):
 *   "strip_h" (0 = by launch size), "frames_inner", "frames_wg", "frame_major", "big_wave",
 *   "big_fused", "stream_k", "pipe7", "ring_remap", "ring_min", "lens_cache", "u8_lz_lds",
 *   "stored_coords" (smallest batch whose homography / lens coordinates are evaluated once
 *   for all frames, 0 = never), "pipe", "tile_warp" (perspective warps of float32 frames with an
 *   output tile's source box in LDS: 0 never, 1 where it pays, 2 whenever the homography fits).
 *   "rank1_sep" (dense K x K kernels that are an outer product ky (x) kx on the separable K + K loops: bit 0
 *   the remap -> filter chains (float32 frames, bilinear taps, 3 / 5 / 7 / 9 taps), bit 1 the plain 9 x 9
 *   filter; default 3; the reference obtains its Gaussians separably: scipy.ndimage.gaussian_filter,
 *   filters/fastFilter.py:42).
 *   "strip_remap" (standalone bilinear remaps of camera frames - uint16 into float32, uint16 into uint16 with cv2's 16U
 *   arithmetic (IPA_INTER_LINEAR | IPA_INTER_Q5), uint8 into uint8 with its 8U fixed point; ipa_remap_dev, ipa_undistort_dev,
 *   ipa_warp_perspective_dev - on the marching strips of the chains with no filter: default 1; read-only counter
 *   "strip_remaps").
 *   Read-only "remap_path": the kernels the last ipa_remap_dev / ipa_undistort_dev / ipa_warp_perspective_dev /
 *   ipa_warp_grid_dev call enqueued, as IPA_REMAP_PATH_* bits (below).  The outermost of these calls clears the word on
 *   entry - ipa_undistort_dev's pass through its cached map into ipa_remap_dev keeps one word for the whole call; after
 *   a remap -> filter chain of two launches it describes that chain's remap -, every launch site sets its bit where the
 *   kernel is enqueued.  Written on the host, once per launch; no routing decision reads it.
 *   Read-only "chain_path": what the last remap -> filter chain call (the six ipa_*_conv2d_dev / ipa_*_sepconv2d_dev
 *   exports with a coordinate source) did, as IPA_CHAIN_PATH_* bits (below).  The export clears the word on entry; every
 *   bit is set where the thing happens, from what the launch used.  The word describes the chain's own kernels: what the
 *   remap of a chain of two launches enqueued stays in "remap_path".  Written on the host; no routing decision reads it.
 *   "sep_u16" (uint16 frames, bilinear remap by maps or a homography -> separable 3 / 5 / 7 / 9-tap filter in one kernel: default 1;
 *   0 = two launches through the workspace).
 *   "tail_rows" (chunked batches on the shared-record loop end every XCD's share of the launch on short strips -
 *   the workgroups that run while the launch drains: -1 = the measured rule by taps and launch size, 0 = uniform
 *   strips, n = short strips of n rows; same bits).
 *   "ste_frames" (frames per launch of ipa_ste_dev: 8, the halo tile, default; 1, one launch per frame; same bits).
 *   "nlf_grid" (workgroups of the persistent launches of ipa_nlf_moments_dev and ipa_nlf_bins_dev: 0, by launch size,
 *   default; n <= 4096, exactly n whatever the work - idle workgroups contribute zeros).
 *   ipa_ctx_get_tuning also answers the read-only names "tail_rows_used" (height of the short strips of the last such
 *   launch, 0 = uniform), "rank1_routed" (dense calls sent to the separable loops so far) and "group_chunk_used" (frame
 *   groups per chunk of the last launch on the shared-record loop; "group_chunk" values that do not divide
 *   the group count go to the nearest divisor).
 * Values are range-checked (IPA_ERR_BAD_ARG).  ipa_ctx_create reads the IPA_* environment
 * defaults once; no launch path consults the environment.  The reference has no counterpart
 * (its numba / cv2 calls take no launch parameters). */
enum {                                    /* bits of the read-only "remap_path" (csrc/remap_impl.hpp, remap.hip, fused.hip) */
  IPA_REMAP_PATH_GATHER = 1 << 0,       /* remap_kernel on the caller's coordinates (the uint8 bicubic table form too) */
  IPA_REMAP_PATH_REST = 1 << 1,         /* remap_kernel behind a ring kernel's skip mask */
  IPA_REMAP_PATH_RING = 1 << 2,         /* ring_remap_kernel */
  IPA_REMAP_PATH_TILE = 1 << 3,         /* the tile kernel of a homography, float32 or uint16 */
  IPA_REMAP_PATH_TILE_MAP = 1 << 4,     /* the tile kernel of a map pair */
  IPA_REMAP_PATH_STORED = 1 << 5,       /* remap_kernel on coordinates evaluated once into the plan buffer */
  IPA_REMAP_PATH_U8_LZ_LDS = 1 << 6,    /* remap_u8_lz_kernel */
  IPA_REMAP_PATH_STRIP = 1 << 7,        /* the marching strips of the chains, into float32 */
  IPA_REMAP_PATH_STRIP_INT = 1 << 8,    /* ... into the frames' own integer type */
  IPA_REMAP_PATH_LENS_MAP = 1 << 9,     /* ipa_undistort_dev through its cached map */
  IPA_REMAP_PATH_FRAMES_INNER = 1 << 10 /* the gather / rest launch had the frame index fastest */
};
enum {                                    /* bits of the read-only "chain_path" (csrc/fused.hip, fused_impl.hpp, fused_big.hip, wave_sep.hpp) */
  IPA_CHAIN_PATH_RESIDENT = 1 << 0,     /* wave_stencil_kernel with a sampling source: dense 3 / 5 / 7 taps */
  IPA_CHAIN_PATH_STREAMED = 1 << 1,     /* wave_stencil_big_kernel with a sampling source: dense 7 / 9 / 11 taps */
  IPA_CHAIN_PATH_SEP = 1 << 2,          /* wave_sep_kernel with a sampling source */
  IPA_CHAIN_PATH_TWO_LAUNCHES = 1 << 3, /* the remap into the workspace, then the plain filter */
  IPA_CHAIN_PATH_RANK1 = 1 << 4,        /* a dense kernel that is an outer product went to the separable chain */
  IPA_CHAIN_PATH_LENS_MAP = 1 << 5,     /* the lens model was replaced by its cached map */
  IPA_CHAIN_PATH_ROTATED = 1 << 6,      /* a rotated homography: two launches preferred to the one kernel */
  IPA_CHAIN_PATH_STORED = 1 << 7,       /* a homography's coordinates read from the table evaluated once */
  IPA_CHAIN_PATH_SPLIT = 1 << 8,        /* the batch ran as head and tail launches of the shared-record loop */
  IPA_CHAIN_PATH_FRAMES_WG = 1 << 9,    /* a launch whose workgroups were frames of one strip (WaveParams::frames_wg = 1) */
  IPA_CHAIN_PATH_PER_FRAME = 1 << 10    /* a launch whose waves each had a strip of their own (frames_wg = 0) */
};
int ipa_ctx_set_tuning(ipa_ctx* ctx, const char* name, int value);
int ipa_ctx_get_tuning(ipa_ctx* ctx, const char* name, int* value);
/* name (e.g. "gfx950...") and compute-unit count of the context's device */
int ipa_ctx_device_info(ipa_ctx* ctx, char* name, size_t name_len, int* cu_count,
                        size_t* total_mem_bytes);
/* free and total bytes of the context's device right now (hipMemGetInfo): what the Python layer's
 * block pool bounds its optional second candidate allocation by (imgprocessor_amd/device.py; the
 * reference has no device memory - this is library plumbing, not a reference call site) */
int ipa_mem_info(ipa_ctx* ctx, size_t* free_bytes, size_t* total_bytes);

/* device / pinned-host memory owned by the caller until freed */
int ipa_malloc(ipa_ctx* ctx, size_t bytes, void** dptr);
int ipa_free(ipa_ctx* ctx, void* dptr);
int ipa_host_alloc(ipa_ctx* ctx, size_t bytes, void** hptr);
int ipa_host_free(ipa_ctx* ctx, void* hptr);
int ipa_memcpy_h2d(ipa_ctx* ctx, void* dptr, const void* hptr, size_t bytes); /* synchronous */
int ipa_memcpy_d2h(ipa_ctx* ctx, void* hptr, const void* dptr, size_t bytes); /* synchronous */
int ipa_memcpy_d2d(ipa_ctx* ctx, void* dst, const void* src, size_t bytes);   /* stream-ordered */
int ipa_memset(ipa_ctx* ctx, void* dptr, int value, size_t bytes);            /* stream-ordered */

/* HIP events recorded on the stream the kernels run on (bench.py timing) */
int ipa_event_create(ipa_ctx* ctx, ipa_event** ev);
int ipa_event_destroy(ipa_ctx* ctx, ipa_event* ev);
int ipa_event_record(ipa_ctx* ctx, ipa_event* ev);
int ipa_event_elapsed_ms(ipa_ctx* ctx, ipa_event* start, ipa_event* stop, float* ms);

/* ------------------------------------------------------------ map builder */
/* replaces cv2.initUndistortRectifyMap(K, dist, None, newK, (w,h), CV_32FC1)
 * at camera/LensDistortion.py:355-357.  K,newK: 3x3 row-major double;
 * dist5 = [k1,k2,p1,p2,k3] (LensDistortion.py:370,380).  Maps are float32. */
int ipa_build_undistort_map_dev(ipa_ctx* ctx, const double* K, const double* dist5,
                                const double* newK, int h, int w, float* d_mapx, float* d_mapy,
                                long map_pitch);
int ipa_build_undistort_map(ipa_ctx* ctx, const double* K, const double* dist5,
                            const double* newK, int h, int w, float* mapx, float* mapy);

/* ------------------------------------------------------------------ remap */
/* replaces cv2.remap(image, mapx, mapy, interp, borderMode, borderValue) at
 * camera/LensDistortion.py:323-326,339-340 (and transform/polarTransform.py:66,105).
 * dst dtype may equal the src dtype or be IPA_F32 (fused toFloatArray ingest).
 * u8 -> u8 INTER_LINEAR uses cv2's exact fixed-point arithmetic. */
int ipa_remap_dev(ipa_ctx* ctx, const void* d_src, int src_dtype, int sh, int sw, long src_pitch,
                  const float* d_mapx, const float* d_mapy, long map_pitch, void* d_dst,
                  int dst_dtype, int dh, int dw, long dst_pitch, int n_frames,
                  long src_frame_stride, long dst_frame_stride, int interp, int border_mode,
                  double border_value);
int ipa_remap(ipa_ctx* ctx, const void* src, int src_dtype, int sh, int sw, const float* mapx,
              const float* mapy, void* dst, int dst_dtype, int dh, int dw, int n_frames,
              int interp, int border_mode, double border_value);

/* The tables of OpenCV's remap at 1/32 px that the cv2 modes read, exactly the bytes the library uploads
 * (csrc/cv_tables.hpp).  Host only: needs neither a context nor a device.  Returns the table's size in bytes, -1 for an
 * unknown `which`; the table is written to `out` when that is given and `cap` >= the size, nothing otherwise. */
typedef enum {
  IPA_CV_TABLE_ROWS = 0,        /* 384 float32: 32 x 8 Lanczos4 rows (interpolateLanczos4 at k / 32), then 32 x 4
                                   bicubic rows (interpolateCubic, A = -0.75) */
  IPA_CV_TABLE_U8_CUBIC = 1,    /* uint8 bicubic, 1024 x 8 int32: entry fy * 32 + fx holds the 4 x 4 int16 weights
                                   cvRound(wy[r] * wx[c] * 2^15) whose sum is forced to 2^15 (initInterTab2D, fixed
                                   point); tap row r = dwords 2 r, 2 r + 1 = {w0 | w2 << 16, w1 | w3 << 16}
                                   (low half | high half) */
  IPA_CV_TABLE_U8_LANCZOS4 = 2  /* uint8 Lanczos4, 1024 x 32 int32: the 8 x 8 weights likewise; tap row r = dwords
                                   4 r .. 4 r + 3 = {w0 | w1 << 16, w2 | w3 << 16, w4 | w5 << 16, w6 | w7 << 16} */
} ipa_cv_table_id;
int ipa_cv_table(int which, void* out, size_t cap);

/* LensDistortion.correct without materialised maps: the distortion model of
 * initUndistortRectifyMap is evaluated per pixel in double, rounded to the
 * float32 a CV_32FC1 map would hold, then sampled exactly like ipa_remap.
 * Bit-identical to ipa_build_undistort_map_dev + ipa_remap_dev. */
int ipa_undistort_dev(ipa_ctx* ctx, const void* d_src, int src_dtype, int sh, int sw,
                      long src_pitch, const double* K, const double* dist5, const double* newK,
                      void* d_dst, int dst_dtype, int dh, int dw, long dst_pitch, int n_frames,
                      long src_frame_stride, long dst_frame_stride, int interp, int border_mode,
                      double border_value);
int ipa_undistort(ipa_ctx* ctx, const void* src, int src_dtype, int sh, int sw, const double* K,
                  const double* dist5, const double* newK, void* dst, int dst_dtype, int dh,
                  int dw, int n_frames, int interp, int border_mode, double border_value);

/* replaces cv2.warpPerspective at camera/PerspectiveCorrection.py:241-242,
 * 377-378,401-405 (and transform/simplePerspectiveTransform.py:27-31).
 * M is the 3x3 row-major double matrix mapping DESTINATION (x,y,1) to source
 * coordinates: pass inv(H) for a plain call, H itself for WARP_INVERSE_MAP. */
int ipa_warp_perspective_dev(ipa_ctx* ctx, const void* d_src, int src_dtype, int sh, int sw,
                             long src_pitch, const double* M, void* d_dst, int dst_dtype, int dh,
                             int dw, long dst_pitch, int n_frames, long src_frame_stride,
                             long dst_frame_stride, int interp, int border_mode,
                             double border_value);
int ipa_warp_perspective(ipa_ctx* ctx, const void* src, int src_dtype, int sh, int sw,
                         const double* M, void* dst, int dst_dtype, int dh, int dw, int n_frames,
                         int interp, int border_mode, double border_value);

/* replaces the per-cell cv2.warpPerspective calls of PerspectiveCorrection.correctGrid
 * (camera/PerspectiveCorrection.py:281-372) with ONE launch: n_cells cells, each with a
 * destination rectangle cell_rects[i] = {x0, y0, w, h} and a 3x3 row-major double matrix
 * cell_M[9 i ..] that maps the cell's LOCAL destination pixel (X - x0, Y - y0, 1) to source
 * coordinates (both HOST pointers).  Rectangles come in paint order and may overlap: the last one
 * that covers a pixel owns it.  Every pixel is bit for bit what ipa_warp_perspective_dev gives for
 * its cell (same dtypes, interpolations and border modes).  A pixel no rectangle covers receives
 * what a pixel wholly outside the source receives under IPA_BORDER_CONSTANT with border_value,
 * whatever border_mode is.  IPA_ERR_BAD_ARG: n_cells outside [1, 32767], a rectangle that is
 * empty or not inside the destination, more than 65535 bands on an axis. */
int ipa_warp_grid_dev(ipa_ctx* ctx, const void* d_src, int src_dtype, int sh, int sw, long src_pitch,
                      const int* cell_rects, const double* cell_M, int n_cells, void* d_dst,
                      int dst_dtype, int dh, int dw, long dst_pitch, int n_frames,
                      long src_frame_stride, long dst_frame_stride, int interp, int border_mode,
                      double border_value);
int ipa_warp_grid(ipa_ctx* ctx, const void* src, int src_dtype, int sh, int sw, const int* cell_rects,
                  const double* cell_M, int n_cells, void* dst, int dst_dtype, int dh, int dw,
                  int n_frames, int interp, int border_mode, double border_value);
/* The ownership resolution behind ipa_warp_grid_dev as a pure host function (no context, no
 * device; the device entry calls it): the destination cut at every rectangle edge into column
 * and row bands.  colband[dw] / rowband[dh]: the band of a column / row; owner[n_rowbands *
 * n_colbands], row-major: the last cell that covers the band pair, -1 = none.  Each of the three
 * may be NULL (a first call for the band counts sizes `owner`).  The pixel (x, y) belongs to
 * owner[rowband[y] * n_colbands + colband[x]].  Errors as above (ipa_last_error(NULL)). */
int ipa_warp_grid_plan(const int* cell_rects, int n_cells, int dh, int dw, uint16_t* colband,
                       uint16_t* rowband, int16_t* owner, int* n_rowbands, int* n_colbands);

/* ---------------------------------------------------------------- filters */
/* dense kh x kw centred correlation (== scipy.ndimage.correlate, origin 0):
 *   dst[y,x] = sum_{i,j} kernel[i,j] * src[y+i-kh/2, x+j-kw/2]
 * replaces filters/maskedConvolve.py:24-43 (_calc) + the padding of
 * filters/_extendArrayForConvolution.py:5-97 (border_x / border_y per axis),
 * and the cv2.blur / scipy.ndimage.convolve call sites
 * (camera/lens/estimateSystematicErrorLensCorrection.py:206-207, features/hog.py:62-63).
 * kernel: HOST pointer, kh*kw doubles.  d_mask: optional uint8 (H,W) device
 * array; where it is 0 the output is 0 (maskedConvolve), NULL = everywhere.
 * dtype: IPA_F32 or IPA_F64 (src and dst). */
int ipa_conv2d_dev(ipa_ctx* ctx, const void* d_src, int dtype, int h, int w, long src_pitch,
                   const double* kernel, int kh, int kw, const uint8_t* d_mask, long mask_pitch,
                   void* d_dst, long dst_pitch, int n_frames, long src_frame_stride,
                   long dst_frame_stride, int border_x, int border_y, double border_value);
int ipa_conv2d(ipa_ctx* ctx, const void* src, int dtype, int h, int w, const double* kernel,
               int kh, int kw, const uint8_t* mask, void* dst, int n_frames, int border_x,
               int border_y, double border_value);

/* separable correlation, scipy.ndimage.gaussian_filter order: axis 0 (y) with
 * ky[nky] first, intermediate rounded to the image dtype, then axis 1 (x) with
 * kx[nkx].  nky==0 / nkx==0 skips that axis.  Replaces the gaussian_filter call
 * sites filters/standardDeviation.py:23, filters/fastFilter.py:42,
 * camera/flatField/flatField.py:47.  Single pass over HBM.
 * Tap counts: up to 63 per axis (and two LDS planes within 150 KiB) run in the single-pass
 * kernels, which are centred on an odd count only - an EVEN count there is IPA_ERR_BAD_ARG.
 * Longer kernels run axis by axis on the generic correlation and that check leaves them out
 * (sepconv_taps_ok, csrc/conv_paths.hpp), so an even count of 64 taps or more is accepted and
 * centred on tap n / 2 like scipy's correlate1d
 * (tests/test_gpu_conv_paths.py pins both).  The inconsistency is known and kept: callers that
 * need even kernels of any length have ipa_conv2d_dev with kh or kw = 1. */
int ipa_sepconv2d_dev(ipa_ctx* ctx, const void* d_src, int dtype, int h, int w, long src_pitch,
                      const double* ky, int nky, const double* kx, int nkx, void* d_dst,
                      long dst_pitch, int n_frames, long src_frame_stride, long dst_frame_stride,
                      int border_y, int border_x, double border_value);
int ipa_sepconv2d(ipa_ctx* ctx, const void* src, int dtype, int h, int w, const double* ky,
                  int nky, const double* kx, int nkx, void* dst, int n_frames, int border_y,
                  int border_x, double border_value);

/* Which kernel ipa_conv2d_dev / ipa_sepconv2d_dev launch for a kernel shape and dtype: the
 * launchers' own selection arithmetic (csrc/conv_paths.hpp), without a context or a device.
 * Returns 0 = refused, 1.. = the kernels in the order listed, -1 = unknown op.  The rank-1
 * routing of a dense float32 9x9 (knob rank1_sep, counter rank1_routed) depends on the kernel's
 * values and happens before this selection: it is not part of the query. */
typedef enum {
  IPA_CONV_CONV2D = 0,       /* k0, k1 = kh, kw; flags bit 0: with a mask, bit 1: knob big_wave
                                == 0.  1 marching wave (float32, no mask, square 3/5/7, and
                                9/11 unless big_wave == 0), 2 LDS tile (float32 square 3..11
                                otherwise, float64 square 3/5/7), 3 generic */
  IPA_CONV_SEPCONV2D = 1,    /* k0, k1 = nky, nkx.  1 marching separable wave (float32,
                                nky == nkx in 3/5/7/9), 2 LDS kernel within 64 KiB, 3 LDS kernel
                                with the dynamic-LDS opt-in, 4 two generic launches through a
                                temporary, 5 one generic launch (long kernel on one axis only) */
  IPA_CONV_SEPCONV2D_LDS = 2 /* k0, k1 = nky, nkx: not a path but the bytes of dynamic LDS the
                                LDS kernel needs (the formula behind 2 / 3 / 4 above) */
} ipa_conv_op;
int ipa_conv_path(int op, int dtype, int k0, int k1, int flags);

/* replaces filters/varYSizeGaussianFilter.py:53-68 (_2dConvolutionYdependentKernel):
 *   dst[r,c] = sum_{ii<k0, jj<k1} kernels[r][ii][jj] * src[r+ii-k0/2, c+jj-k1/2]
 * with NaN pixels skipped (no renormalisation) and borders resolved on the fly
 * (the reference pads first; its defaults are modex='wrap', modey='reflect').
 * d_kernels: DEVICE array of h*k0*k1 doubles (one k0 x k1 table per row). */
int ipa_conv_ydep_dev(ipa_ctx* ctx, const void* d_src, int dtype, int h, int w, long src_pitch,
                      const double* d_kernels, int k0, int k1, int border_x, int border_y,
                      void* d_dst, long dst_pitch);
/* filters/varYSizeGaussianFilter.py:9-50 in one call: the per-row Gaussian tables
 * (gaussian_filter(delta, (stdys[r], stdx)) with stdys = linspace(sig_min, sig_max, h), :22-46) are
 * built on the device as separable factors - `rowk` = the kx x-responses of the delta (host,
 * kx doubles) - and the NaN-skipping row-dependent correlation (:53-68) forms the coefficients
 * on the fly.  Returns after the launch has consumed `rowk`. */
int ipa_var_y_gauss_dev(ipa_ctx* ctx, const void* d_src, int dtype, int h, int w, long src_pitch,
                        double sig_min, double sig_max, int ky, const double* rowk, int kx,
                        int border_x, int border_y, void* d_dst, long dst_pitch);

/* replaces filters/standardDeviation.py:34-70 (_calc): local standard deviation of
 * img around blurred[i,j] over the window [i-kx/2, min(i+kx/2, h)) x [j-ky/2, min(j+ky/2, w)),
 * divided by (rows-1)*(cols-1) exactly as the reference does. */
int ipa_local_std_dev(ipa_ctx* ctx, const void* d_img, const void* d_blurred, int dtype, int h,
                      int w, long pitch, long blurred_pitch, int ksize_x, int ksize_y,
                      void* d_out, long out_pitch);

/* replaces filters/maskedFilter.py:43-72 (_calcMean, reached from maskedFilter(fn='mean'),
 * :12-37): mean of the pixels with mask == 0 inside the window
 * [i-ksize/2, min(i+ksize/2, h)) x [j-ksize/2, min(j+ksize/2, w)).
 *   fill_mask != 0: written for the pixels with mask != 0 that have at least one such
 *                   neighbour, everything else of d_out untouched; d_out may be d_arr
 *                   (the reference's in-place fill);
 *   fill_mask == 0: written for the pixels with mask == 0, NaN elsewhere; not in place.
 * d_mask: DEVICE uint8 h x w (non-zero = masked).  float32/float64, double accumulation. */
int ipa_masked_mean_dev(ipa_ctx* ctx, const void* d_arr, int dtype, const unsigned char* d_mask,
                        int h, int w, long pitch, long mask_pitch, int ksize, int fill_mask,
                        void* d_out, long out_pitch);

/* replaces filters/maskedFilter.py:76-102 (_calcMedian, maskedFilter(fn='median')): as
 * ipa_masked_mean_dev with np.median of the window's mask == 0 pixels (mean of the two middle
 * values for an even count; NaN if any of them is NaN).  The window (ksize/2*2)^2 must fit the
 * kernel's per-wave LDS buffers (two per wave, four waves, 64 KiB): ksize <= 45 for float32,
 * 33 for float64; IPA_ERR_UNSUPPORTED beyond, d_out untouched. */
int ipa_masked_median_dev(ipa_ctx* ctx, const void* d_arr, int dtype, const unsigned char* d_mask,
                          int h, int w, long pitch, long mask_pitch, int ksize, int fill_mask,
                          void* d_out, long out_pitch);

/* replaces filters/nan_maximum_filter.py:17-37 (_calc): np.nanmax over the same clipped
 * window; NaN where the whole window is NaN. */
int ipa_nan_max_dev(ipa_ctx* ctx, const void* d_arr, int dtype, int h, int w, long pitch,
                    int ksize, void* d_out, long out_pitch);

/* replaces render/closestDirectDistance.py:17-41 (_calc): for every zero pixel of d_arr (uint8,
 * non-zero = set) the distance to the closest set pixel within the +-ksize window, 2*ksize when
 * there is none; 0 on set pixels.  out_dtype IPA_U16 (the reference's default dtype, value
 * truncated) or IPA_F64. */
int ipa_closest_distance_dev(ipa_ctx* ctx, const unsigned char* d_arr, int h, int w, long pitch,
                             int ksize, void* d_out, int out_dtype, long out_pitch);

/* replaces uncertainty/positionToIntensityUncertainty.py:7-49 (_calc_constPSF / _calc_variPSF):
 *   sint[i,j] = sqrt( sum psf[ii,jj] * (img[i-ii+c, j-jj+c] - img[i,j])^2 ),  psf a (2*ksize+1)^2
 * Gaussian normalised to 1 with the FIRST sigma on the row axis (numbaGaussian2d as called at
 * :14,:39), pixels within ksize of the frame and NaN centres left 0.  d_sx / d_sy: per-pixel
 * float64 sigma maps, or both NULL to use the scalars sx / sy.  img float32/float64, d_sint
 * float64. */
int ipa_pos_intensity_unc_dev(ipa_ctx* ctx, const void* d_img, int dtype, int h, int w, long pitch,
                              const double* d_sx, const double* d_sy, long sigma_pitch, double sx,
                              double sy, int ksize, double* d_sint, long out_pitch);

/* replaces filters/medianThreshold.py:7-30 with size=3:
 *   blur = scipy.ndimage.median_filter(img, size=3)   (mode 'reflect': edge pixel repeated)
 *   hit  = |(img - blur) / blur| > threshold           ('<' when cond_less != 0), float64, IEEE
 *   out  = hit ? blur : img;   d_indices (uint8 h x w, may be NULL) = hit
 * threshold must be > 0 (the reference returns its input untouched otherwise).  Not in place. */
int ipa_median_threshold_dev(ipa_ctx* ctx, const void* d_img, int dtype, int h, int w, long pitch,
                             double threshold, int cond_less, void* d_out, long out_pitch,
                             unsigned char* d_indices, long idx_pitch);
/* the same for any window size (filters/medianThreshold.py:7-30 passes `size` to
 * scipy.ndimage.median_filter): blur = the element of rank size*size/2 of the size x size window
 * at offsets -size/2 .. size-1-size/2, edge pixels repeated; size = 3 takes the kernel above. */
int ipa_median_threshold_size_dev(ipa_ctx* ctx, const void* d_img, int dtype, int h, int w,
                                  long pitch, int size, double threshold, int cond_less,
                                  void* d_out, long out_pitch, unsigned char* d_indices,
                                  long idx_pitch);

/* replaces stages 2-4 of CameraCalibration.correct (camera/CameraCalibration.py:416-437) in one
 * pass over the frame:
 *   v = img - bg                      (:505  _correctDarkCurrent;   d_bg NULL = stage skipped)
 *   v = ff != 0 ? v / ff : v          (:527-528 _correctVignetting; d_ff NULL = stage skipped)
 *   if threshold > 0: v = nan_to_num(v); medianThreshold(v, threshold, size 3, '>')  (:566-567)
 * d_bg / d_ff: DEVICE arrays of the image dtype (float32/float64).  Not in place. */
int ipa_calib_prefilter_dev(ipa_ctx* ctx, const void* d_img, int dtype, const void* d_bg,
                            const void* d_ff, int h, int w, long pitch, long bg_pitch,
                            long ff_pitch, double threshold, void* d_out, long out_pitch);

/* Which kernel an entry point of this section launches for a window and dtype: the launchers'
 * own selection arithmetic (csrc/stencil_paths.hpp), without a context or a device.  Returns
 * 0 = refused, 1.. = the kernels in the order listed, -1 = unknown op.  kx / ky as below. */
typedef enum {
  IPA_STENCIL_LOCAL_STD = 0,         /* kx, ky = ksize_x, ksize_y: 1 wave (square, half window
                                        1..5), 2 LDS tile, 3 generic */
  IPA_STENCIL_MASKED_MEAN_FILL = 1,  /* kx = ksize, in place: 1 column sums, 2 wave */
  IPA_STENCIL_MASKED_MEDIAN = 2,     /* kx = ksize: 1 wave kernel, 0 refused */
  IPA_STENCIL_NAN_MAX = 3,           /* kx = ksize: 1 separable LDS, 2 generic */
  IPA_STENCIL_CLOSEST_DISTANCE = 4,  /* kx = ksize: 1 two-pass row distances, 2 direct */
  IPA_STENCIL_POS_INTENSITY_UNC = 5, /* kx = ksize (half window): 1 separable, 2 generic */
  IPA_STENCIL_MEDIAN_THRESHOLD = 6,  /* kx = size: 1 3x3 network, 2 counting, 0 refused */
  IPA_STENCIL_VAR_Y_GAUSS = 7,       /* kx, ky = taps along x, y: 1 tiled, 2 expanded table
                                        through the conv_ydep tile kernel, 3 ... generic */
  IPA_STENCIL_CONV_YDEP = 8          /* kx, ky = k1, k0: 1 LDS tile, 2 generic */
} ipa_stencil_op;
int ipa_stencil_path(int op, int dtype, int kx, int ky);

/* replaces filters/_extendArrayForConvolution.py:5-97 for callers that want the
 * padded array itself (the filters above resolve borders while staging and do
 * not need it): dst is (h + 2*(ky/2)) x (w + 2*(kx/2)), kx/ky = kernel size
 * along x/y.  Any dtype (pure copy). */
int ipa_extend_array_dev(ipa_ctx* ctx, const void* d_src, int dtype, int h, int w, long src_pitch,
                         int kx, int ky, int modex, int modey, void* d_dst, long dst_pitch);

/* (H, W, C) images - what cv2.remap / cv2.warpPerspective take in LensDistortion.correct
 * (camera/LensDistortion.py:323-326) and PerspectiveCorrection.correct
 * (camera/PerspectiveCorrection.py:401-405; the reference's own demo warps a colour PNG,
 * :858-900) - against the C planes of (H, W) every entry point above works on (n_frames = C):
 * device-side layout copies, so that a colour frame goes host -> device -> host once, without a
 * transposed copy on the host.  Pitches in elements (src_pitch of the interleaved image >= w * C),
 * any dtype. */
int ipa_deinterleave_dev(ipa_ctx* ctx, const void* d_src, int dtype, int h, int w, int channels,
                         long src_pitch, void* d_dst, long dst_pitch, long dst_plane_stride);
int ipa_interleave_dev(ipa_ctx* ctx, const void* d_src, int dtype, int h, int w, int channels,
                       long src_pitch, long src_plane_stride, void* d_dst, long dst_pitch);

/* --------------------------------------------- fused remap -> K x K filter */
/* the headline chain (LensDistortion.correct followed by a K x K filter, the
 * in-tree archetype being estimateSystematicErrorLensCorrection.py:199-207):
 * remapped pixels (incl. the filter halo, resolved with conv_border_*) are
 * produced into LDS and filtered there; the intermediate image never touches
 * HBM.  dst dtype is IPA_F32 (src may be u8/u16/f32) or IPA_F64 (src f64).
 * One kernel is built for float32 frames (bilinear, both bicubics), uint16 frames (bilinear;
 * maps or the lens model) and uint8 frames (bilinear, maps; 3 .. 7) with square 3 .. 11 kernels; every OTHER combination the standalone
 * entry points accept (Lanczos4 / nearest taps, uint8 frames, uint16 frames under a homography or
 * with bicubic taps, rectangular / even / larger kernels) runs as what it is - remap into the
 * context workspace, then ipa_conv2d_dev - with the bits of the two calls (round 6; these
 * returned IPA_ERR_UNSUPPORTED before).  Holds for the three *_conv2d_dev entry points. */
int ipa_remap_conv2d_dev(ipa_ctx* ctx, const void* d_src, int src_dtype, int sh, int sw,
                         long src_pitch, const float* d_mapx, const float* d_mapy, long map_pitch,
                         const double* kernel, int kh, int kw, void* d_dst, int dst_dtype, int dh,
                         int dw, long dst_pitch, int n_frames, long src_frame_stride,
                         long dst_frame_stride, int interp, int border_mode, double border_value,
                         int conv_border_x, int conv_border_y);
int ipa_undistort_conv2d_dev(ipa_ctx* ctx, const void* d_src, int src_dtype, int sh, int sw,
                             long src_pitch, const double* K, const double* dist5,
                             const double* newK, const double* kernel, int kh, int kw, void* d_dst,
                             int dst_dtype, int dh, int dw, long dst_pitch, int n_frames,
                             long src_frame_stride, long dst_frame_stride, int interp,
                             int border_mode, double border_value, int conv_border_x,
                             int conv_border_y);
int ipa_warp_perspective_conv2d_dev(ipa_ctx* ctx, const void* d_src, int src_dtype, int sh, int sw,
                                    long src_pitch, const double* M, const double* kernel, int kh,
                                    int kw, void* d_dst, int dst_dtype, int dh, int dw,
                                    long dst_pitch, int n_frames, long src_frame_stride,
                                    long dst_frame_stride, int interp, int border_mode,
                                    double border_value, int conv_border_x, int conv_border_y);

/* The same chain with a SEPARABLE filter (BASELINE config C3: PerspectiveCorrection remap +
 * separable 9-tap Gaussian; in the reference cv2.remap / cv2.warpPerspective followed by
 * scipy.ndimage.gaussian_filter, e.g. PerspectiveCorrection.py:401-405 then
 * filters/fastFilter.py:42): axis 0 with ky[nky], the float32 intermediate, then axis 1 with
 * kx[nkx], exactly as ipa_sepconv2d_dev on the materialised remap result.  One kernel for
 * float32 sources, INTER_LINEAR and nky == nkx in {3,5,7,9}; any other combination runs
 * as remap + ipa_sepconv2d_dev through the context workspace (same results).  dst is
 * IPA_F32; a constant filter border uses 0. */
int ipa_remap_sepconv2d_dev(ipa_ctx* ctx, const void* d_src, int src_dtype, int sh, int sw,
                            long src_pitch, const float* d_mapx, const float* d_mapy,
                            long map_pitch, const double* ky, int nky, const double* kx, int nkx,
                            void* d_dst, int dst_dtype, int dh, int dw, long dst_pitch, int n_frames,
                            long src_frame_stride, long dst_frame_stride, int interp,
                            int border_mode, double border_value, int conv_border_y,
                            int conv_border_x);
int ipa_undistort_sepconv2d_dev(ipa_ctx* ctx, const void* d_src, int src_dtype, int sh, int sw,
                                long src_pitch, const double* K, const double* dist5,
                                const double* newK, const double* ky, int nky, const double* kx,
                                int nkx, void* d_dst, int dst_dtype, int dh, int dw, long dst_pitch,
                                int n_frames, long src_frame_stride, long dst_frame_stride,
                                int interp, int border_mode, double border_value, int conv_border_y,
                                int conv_border_x);
int ipa_warp_perspective_sepconv2d_dev(ipa_ctx* ctx, const void* d_src, int src_dtype, int sh,
                                       int sw, long src_pitch, const double* M, const double* ky,
                                       int nky, const double* kx, int nkx, void* d_dst,
                                       int dst_dtype, int dh, int dw, long dst_pitch, int n_frames,
                                       long src_frame_stride, long dst_frame_stride, int interp,
                                       int border_mode, double border_value, int conv_border_y,
                                       int conv_border_x);

/* ------------------------------------------------------------ interpolate */
/* replaces interpolate/interpolate2dStructuredIDW.py:26-65 (_calc): every
 * pixel with mask!=0 becomes the weighted mean of the unmasked pixels in the
 * (2*ksize+1)^2 window; weights: HOST (2*ksize+1)^2 doubles (table built by the
 * caller exactly as :16-21).  In place on d_grid (F32 or F64). */
int ipa_idw_fill_dev(ipa_ctx* ctx, void* d_grid, int dtype, const uint8_t* d_mask, int h, int w,
                     long pitch, int ksize, const double* weights);
int ipa_idw_fill(ipa_ctx* ctx, void* grid, int dtype, const uint8_t* mask, int h, int w,
                 int ksize, const double* weights);

/* replaces interpolate/interpolate2dStructuredFastIDW.py:29-63: neighbours are
 * visited in the order of offsets[n][2] (int32 dy,dx pairs, HOST), stopping
 * after `minnvals`+1 hits exactly as the reference loop does. */
int ipa_fast_idw_fill_dev(ipa_ctx* ctx, void* d_grid, int dtype, const uint8_t* d_mask, int h,
                          int w, long pitch, const int32_t* offsets, const double* weights, int n,
                          int minnvals);
int ipa_fast_idw_fill(ipa_ctx* ctx, void* grid, int dtype, const uint8_t* mask, int h, int w,
                      const int32_t* offsets, const double* weights, int n, int minnvals);

/* replaces interpolate/interpolate2dUnstructuredIDW.py:7-38: every pixel of the grid
 * becomes sum(w v) / sum(w) over the n scattered points (x = ROW coordinate, y = column - the
 * reference indexes grid[i, j] with i against x), w = 1 / ((x-i)^2 + (y-j)^2)^(power/2), summed
 * in point order in float64; a pixel that is a point takes the first such point's value.
 * x, y, v: HOST doubles.  Writes every pixel of d_grid (F32 or F64). */
int ipa_unstructured_idw_dev(ipa_ctx* ctx, void* d_grid, int dtype, int h, int w, long pitch,
                             const double* x, const double* y, const double* v, int n,
                             double power);
int ipa_unstructured_idw(ipa_ctx* ctx, void* grid, int dtype, int h, int w, const double* x,
                         const double* y, const double* v, int n, double power);

/* replaces interpolate/interpolateCircular2dStructuredIDW.py:7-69 as written: IDW over the
 * window [i-k, min(i+k, h)) x [j-k, min(j+k, h)) (upper ends exclusive) with the distance
 * measured in polar coordinates about (cx, cy): ((fr dr)^2 + (fphi dphi midR)^2)^2; rows AND
 * columns run to shape[0] (:16-17), so w >= h is required and columns >= h stay untouched.
 * In place on d_grid (F32 or F64). */
int ipa_circular_idw_fill_dev(ipa_ctx* ctx, void* d_grid, int dtype, const uint8_t* d_mask, int h,
                              int w, long pitch, int ksize, double power, double fr, double fphi,
                              double cx, double cy);
int ipa_circular_idw_fill(ipa_ctx* ctx, void* grid, int dtype, const uint8_t* mask, int h, int w,
                          int ksize, double power, double fr, double fphi, double cx, double cy);

/* replaces interpolate/interpolate2dStructuredCrossAvg.py:7-115 as written: every masked
 * pixel blends the local averages (unmasked pixels within +-ksize) at the nearest unmasked
 * pixel towards row 0, towards column 0 and towards the last column with weights
 * 1 / distance^(power/2) (float32, normalised); the source's slot quirks (the search towards
 * the last row only validates the column-0 slot, which then keeps the previous pixel's value)
 * are reproduced.  In place on d_grid (F32 or F64). */
int ipa_cross_avg_fill_dev(ipa_ctx* ctx, void* d_grid, int dtype, const uint8_t* d_mask, int h,
                           int w, long pitch, int ksize, double power);
int ipa_cross_avg_fill(ipa_ctx* ctx, void* grid, int dtype, const uint8_t* mask, int h, int w,
                       int ksize, double power);

/* replaces interpolate/interpolate2dStructuredPointSpreadIDW.py:7-141 as written: sweeps over the
 * border pixels of the masked areas (_createBorder :31-63: row and column scans that carry their
 * previous value across row / column ends - index -1 marks the last pixel of the row / column),
 * each filled in raster order from the unmasked pixels within [i-k, i+k) x [j-k, j+k) with weights
 * 1 / distance^power and unmasked at once, so later pixels of the sweep see it (:75-135); repeated
 * until a border pass finds no transition or max_iter sweeps have run.  In place on grid (F32 or
 * F64) AND mask (filled pixels become 0). */
int ipa_point_spread_idw_dev(ipa_ctx* ctx, void* d_grid, int dtype, uint8_t* d_mask, int h, int w,
                             long pitch, int ksize, double power, long max_iter);
int ipa_point_spread_idw(ipa_ctx* ctx, void* grid, int dtype, uint8_t* mask, int h, int w,
                         int ksize, double power, long max_iter);

/* The constants and predicates by which the kernels and launchers behind the four fills above,
 * ipa_resize_dev and ipa_fast_filter_stat_dev choose a branch or a kernel (csrc/interp_paths.hpp:
 * the code they call), without a context or a device.  Arguments are doubles that hold integers
 * (a power and a byte address fit too); returns -1 for an unknown op or an argument out of range. */
typedef enum {
  IPA_INTERP_CONST = 0,            /* a = ipa_interp_const */
  IPA_INTERP_CROSS_FASTDIV = 1,    /* a = nt window positions, b = ny window columns: 1 when
                                      cross_local_avg_kernel takes t / ny by multiply-shift */
  IPA_INTERP_CIRCULAR_FASTDIV = 2, /* a = nx, b = ny window rows / columns: the same for
                                      circular_idw_kernel (t < nx ny) */
  IPA_INTERP_FASTDIV_MUL = 3,      /* a = ny: the multiplier M = ceil(2^shift / ny) */
  IPA_INTERP_POWER = 4,            /* a = power: 2 / 1 the kernels without pow, 0 the generic one */
  IPA_INTERP_POINT_SPREAD_ROWS = 5,/* a = h: 1 runs, 0 refused (one LDS word per row) */
  IPA_INTERP_STAT_SAMPLES = 6,     /* a = ksize, b = every: window samples per axis,
                                      ceil(2 ksize / every), or 0 when their square exceeds the
                                      wave's LDS buffer and the call is refused */
  IPA_INTERP_RESIZE_VEC4 = 7,      /* a = dtype, b = dw, c = dst_pitch (elements), d = byte address
                                      of the destination (OR-ed with that of the intermediate
                                      rows, which the library allocates 256-byte aligned):
                                      1 vresize4_kernel, 2 vresize_kernel, 0 not a float dtype */
  IPA_INTERP_RESIZE_AREA = 8,      /* a, b, c, d = sh, sw, dh, dw: 0 refused (enlarging),
                                      1 area_fast_kernel (integer scales), 2 area_kernel */
  IPA_INTERP_RESIZE_LINEAR = 9     /* a, b, c, d = sh, sw, dh, dw: 1 the exact 2 x 2 reduction,
                                      which runs as INTER_AREA, 2 the separable kernels */
} ipa_interp_op;
typedef enum {
  IPA_INTERP_K_CROSS_SEG = 0,          /* pixels of a row per wave of the cross-average fill */
  IPA_INTERP_K_CROSS_BALLOT_STEPS = 1, /* steps of each search taken from the first ballot */
  IPA_INTERP_K_CROSS_SEARCH_PASS = 2,  /* steps per pass of the further search; columns / rows per
                                          chunk of the stale-slot tables */
  IPA_INTERP_K_FASTDIV_SHIFT = 3,
  IPA_INTERP_K_PS_WAVES = 4,           /* waves (= rows in flight) of the point-spread sweep */
  IPA_INTERP_K_PS_MAX_ROWS = 5,
  IPA_INTERP_K_STAT_MAX = 6            /* window samples a wave of the statistics kernel keeps */
} ipa_interp_const;
int ipa_interp_path(int op, double a, double b, double c, double d);

/* ---------------------------------------------------------------- filters: fast* */
/* replaces cv2.resize(img, (dw, dh), interpolation=...) at filters/fastFilter.py:47-48
 * (INTER_LANCZOS4 on the float64 grid of statistics) and filters/fastMean.py:14-19 (INTER_AREA
 * down, INTER_LINEAR up), single-channel IPA_F32 / IPA_F64.  OpenCV's published algorithm
 * (coordinates (d + 0.5) scale - 0.5 in float32, float32 coefficients, horizontal pass first in
 * the image's type; INTER_AREA by block sums / decimation tables, downscaling only). */
typedef enum {
  IPA_RESIZE_LINEAR = 1, IPA_RESIZE_CUBIC = 2, IPA_RESIZE_AREA = 3, IPA_RESIZE_LANCZOS4 = 4
} ipa_resize_interp;   /* cv2's INTER_* numbers */
int ipa_resize_dev(ipa_ctx* ctx, const void* d_src, int dtype, int sh, int sw, long src_pitch,
                   void* d_dst, int dh, int dw, long dst_pitch, int interp);
int ipa_resize(ipa_ctx* ctx, const void* src, int dtype, int sh, int sw, void* dst, int dh, int dw,
               int interp);

/* replaces filters/fastFilter.py:52-122 (_iter + _calcMedian / _calcNanMedian / _calcMean /
 * _calcNanMean): out[ii, jj] = statistic of arr[max(i-k,0) : min(i+k,h) : every,
 * max(j-k,0) : min(j+k,w) : every] at i = ii every, j = jj every; out is ceil(h / every) x
 * ceil(w / every) doubles (the caller applies the reference's crop of the last row and column).
 * fn: 0 median (NaN when the window holds one), 1 nanmedian, 2 mean, 3 nanmean. */
int ipa_fast_filter_stat_dev(ipa_ctx* ctx, const void* d_arr, int dtype, int h, int w, long pitch,
                             int ksize, int every, int fn, double* d_out);
int ipa_fast_filter_stat(ipa_ctx* ctx, const void* arr, int dtype, int h, int w, int ksize,
                         int every, int fn, double* out);

/* ---------------------------------------------------------------- single-time effects */
/* replaces features/SingleTimeEffectDetection.py:23-75 (__init__ + addImage) for a given noise
 * level function, with filters/removeSinglePixels.py:4-30 as the neighbour rule.  Per pixel
 * (float64 throughout, every operation correctly rounded):
 *   first_pair:  avg = min(f0, f1), count = 1                  (:39, NaN propagates)
 *                thr = nlf(avg) * nstd                          (:44) with nlf = {minY, ax, ay}:
 *                max(nan_to_num(ay * sqrt(avg - ax)), minY)     (camera/NoiseLevelFunction.py:94-107),
 *                written to d_thr; nlf NULL: d_thr is an input (a threshold the caller evaluated)
 *                the frames stepped through are then max(f0, f1), f2, ... f(n-1)   (:46-49)
 *   otherwise:   avg / count / thr are read from the state, the frames are f0 ... f(n-1)
 *   per frame g (addImage, :55-75):
 *                s = g - avg > thr;  s &= one of the <= 8 in-image neighbours has s  (:62-63)
 *                where !s && mask: count += 1, avg += (g - avg) / count              (:65-70)
 *                mask_ste |= s (d_mask_ste, OR-accumulated)                          (:72-73)
 *   d_mask_clean: !s of the LAST frame (:65); d_mask: the caller's clean mask (uint8, non-zero =
 *   clean) applied to every frame of the call (:67-68), NULL = all clean.
 * The state (d_avg float64, d_count int32, d_thr float64; state_pitch) stays in HBM between
 * calls, so that a later call continues the stack.  d_avg, d_count and d_thr are ALWAYS required
 * (NULL: IPA_ERR_BAD_ARG), d_thr included when an NLF is given: it is the state a continuation
 * call reads.  nlf is a HOST pointer and is read only with first_pair.  frames: uint8 / uint16 / float32 / float64,
 * `frame_stride` elements apart.  State, masks and frames must not overlap (IPA_ERR_BAD_ARG), and
 * n >= 2 with first_pair.  Up to 8 frames per launch (tuning knob ste_frames = 1: one launch per
 * frame); a call of more launches uses the context workspace. */
int ipa_ste_dev(ipa_ctx* ctx, const void* d_frames, int dtype, int n, int h, int w, long pitch,
                long frame_stride, int first_pair, const double* nlf, double nstd, double* d_avg,
                int* d_count, double* d_thr, long state_pitch, const unsigned char* d_mask,
                unsigned char* d_mask_ste, unsigned char* d_mask_clean, long mask_pitch);
/* replaces filters/removeSinglePixels.py:4-30: out = in && one of the <= 8 in-image neighbours
 * of the pixel is set (uint8, non-zero = set).  Not in place. */
int ipa_remove_single_pixels_dev(ipa_ctx* ctx, const unsigned char* d_in, int h, int w, long pitch,
                                 unsigned char* d_out, long out_pitch);

/* ---------------------------------------------------------------- denoising */
/* replaces skimage.restoration.denoise_nl_means(image, patch_size, patch_distance, h,
 * fast_mode=True, sigma=sigma) of scikit-image 0.18 (camera/CameraCalibration.py:461-474), with
 * the exact exponential where that release uses its +-3 % fast_exp.  With s = patch_size (an even
 * size is s + 1), o = s / 2, d = patch_distance and P the frame continued by numpy's `reflect`
 * (no edge repeat, period 2 (n - 1), repeated where the pad exceeds the frame):
 *   D(p, t) = max((sum_q (P[q] - P[q + t])^2 - 2 sigma^2 (s - 1)^2) / (s^2 h_cut^2), 0),
 *             q over the (s - 1) x (s - 1) window at offsets -o + 1 ... +o from p in both axes
 *   w(p, t) = D > 5 ? 0 : exp(-D),  w(p, 0) = 2
 *   out[p]  = sum_t w P[p + t] / sum_t w,  t in [-d, d]^2,
 *             evaluated as P[p] + sum_t w (P[p + t] - P[p]) / sum_t w
 * IPA_F32 frames compute in float, IPA_F64 frames in double.  n frames (1 ... 65535) of h, w >= 2,
 * `frame_stride` / `dst_frame_stride` elements apart; not in place (IPA_ERR_BAD_ARG when source
 * and destination overlap).  Bounds (IPA_ERR_BAD_ARG beyond them, nothing launched):
 *   2 <= patch_size <= 11, patch_distance >= 0, h_cut > 0, sigma >= 0, and the LDS tile
 *   (rows + s - 2 + 2 d) * (64 + 2 d) * sizeof(element) <= 65536 bytes,
 *   rows = 64 for IPA_F32 and 32 for IPA_F64
 * which admits d <= 30 (float32) and d <= 20 (float64) at s = 7, and d <= 29 / 19 at s = 11. */
int ipa_nl_means_dev(ipa_ctx* ctx, const void* d_src, int dtype, int n, int h, int w, long pitch,
                     long frame_stride, int patch_size, int patch_distance, double h_cut, double sigma,
                     void* d_dst, long dst_pitch, long dst_frame_stride);
/* image[isnan(image)] = 0 (camera/CameraCalibration.py:467), in place, IPA_F32 / IPA_F64 */
int ipa_nan_to_zero_dev(ipa_ctx* ctx, void* d_img, int dtype, int n, int h, int w, long pitch,
                        long frame_stride);

/* ---------------------------------------------------------------- noise level function, SNR */
/* The frames of these calls are uint8 / uint16 / float32 / float64 (IPA_ERR_UNSUPPORTED otherwise),
 * h x w with a pitch in elements, at most 2^30 pixels; all arithmetic is float64 (the reference
 * starts with np.asfarray) and every operation is correctly rounded and unfused.  d_img2 (same
 * dtype, pitch2) is the second exposure or NULL.  A frame is read as `img - bg` with bg the
 * float64 array d_bg (bg_pitch) or, where that is NULL, the scalar `bg` (measure/SNR/SNR.py:33-40;
 * calcNLF passes NULL and 0.0: x - 0.0 is x). */

/* replaces camera/NoiseLevelFunction.py:208-228 and measure/SNR/SNR.py:37-47 (the signal):
 *   one image:   signal = scipy.ndimage.median_filter(img, 3)
 *   two images:  signal = median_filter(0.5 * (img + img2), 3)
 * rank 4 of the 9 values, the edge pixel repeated; written as float64.  Bit-equal to scipy for
 * frames without NaN; a NaN in the window gives NaN (scipy's answer there is unspecified).  Not in
 * place. */
int ipa_nlf_signal_dev(ipa_ctx* ctx, const void* d_img, int dtype, const void* d_img2, int h, int w,
                       long pitch, long pitch2, const double* d_bg, long bg_pitch, double bg,
                       double* d_signal, long signal_pitch);
/* replaces camera/NoiseLevelFunction.py:162-173 (_getMinMax: img.min(), img.max(), np.mean, np.std):
 * moments[0 ... 4] (HOST) = min, max, mean, population std of the non-NaN values of the frame d_img
 * (any of the four types, read as float64: the signal, or a raw frame as estimateFromImages passes
 * one), and the number of NaN values.  Two passes (sum; sum of (x - mean)^2) through per-workgroup
 * partials added in workgroup order: no float atomics, the same bits for the same grid.  Uses the
 * context workspace; returns after the stream has drained. */
int ipa_nlf_moments_dev(ipa_ctx* ctx, const void* d_img, int dtype, int h, int w, long pitch,
                        double* moments);
/* replaces the loop of camera/NoiseLevelFunction.py:243-271 (and the constant noise level of
 * measure/SNR/SNR.py:50-58 with one bin):
 *   diff = (img - signal) * factor        one image  (factor 1 + 1/9, or 1 with
 *                                                     signalFromMultipleImages)
 *   diff = (img - img2) / factor          two images (factor 2**0.5; a division, as in :226)
 *   bin n = every pixel with edges[n] <= signal <= edges[n + 1], BOTH ends inclusive (:259): a
 *           pixel on an interior edge counts in two bins, a NaN signal in none
 *   counts[n] = pixels of bin n (exact), sums[n] = sum |diff| (rms 0) or sum diff^2 (rms 1)
 * edges (nbins + 1 doubles, HOST) is the reference's table e[0] = mn, e[k + 1] = e[k] + step and
 * `step` its step: the kernel guesses floor((signal - e[0]) / step) and settles membership of that
 * bin and its two neighbours against the table.  step > 0 (or 0 with nbins 1: every pixel equal
 * to the one edge).  counts and sums are HOST arrays of nbins.  1 <= nbins <= 2048; above that
 * IPA_ERR_UNSUPPORTED and nothing is written.  Per-workgroup slabs added in workgroup order: no
 * float atomics on global memory.  Uses the context workspace; returns after the stream has
 * drained. */
int ipa_nlf_bins_dev(ipa_ctx* ctx, const void* d_img, int dtype, const void* d_img2, int h, int w,
                     long pitch, long pitch2, const double* d_bg, long bg_pitch, double bg,
                     const double* d_signal, long signal_pitch, const double* edges, int nbins,
                     double step, double factor, int rms, unsigned long long* counts, double* sums);
/* replaces measure/SNR/SNR.py:59-79 per pixel of the float64 signal:
 *   noise = max(nan_to_num(ay * sqrt(signal - ax)), minY), then 1 where below 1   nlf = {minY, ax, ay} (HOST)
 *         = d_noise[y, x], then 1 where below 1     nlf NULL: a noise level function evaluated by the caller
 *         = const_noise                             both NULL: constant_noise_level (:50-58, not clamped)
 *   noise = noise * noise_factor                    0.5**0.5 for imgs_to_be_averaged, else 1
 *   snr   = (signal - bg_level) / noise, then 1 where below 1; NaN stays NaN
 * bg_level: the estimated background (:72-74), 0 where the caller's bg was subtracted already. */
int ipa_snr_map_dev(ipa_ctx* ctx, const double* d_signal, int h, int w, long pitch, const double* nlf,
                    const double* d_noise, long noise_pitch, double const_noise, double noise_factor,
                    double bg_level, double* d_snr, long snr_pitch);
/* replaces the filter of measure/SNR/SNR.py:82-87 (getBackgroundLevel): d_grid (float64,
 * ceil((h - 20) / 10) x ceil((w - 20) / 10)) = median_filter(img[10:-10:10, 10:-10:10], 3); h, w > 20.
 * The caller takes the 1 % point of its histogram (utils/cdf.py:7-20). */
int ipa_snr_bg_median_dev(ipa_ctx* ctx, const void* d_img, int dtype, int h, int w, long pitch,
                          double* d_grid, long grid_pitch);

/* ---------------------------------------------------------------- dark current calibration */
/* What camera/DarkCurrentMap.py needs around ipa_ste_dev.  Frames are uint8 / uint16 / float32 /
 * float64 (IPA_ERR_UNSUPPORTED otherwise), pitches in elements; all arithmetic is float64, every
 * operation correctly rounded and unfused, NaN propagates as numpy propagates it. */

/* replaces np.min((i1, i2), axis=0) of features/SingleTimeEffectDetection.py:39-42, the image the
 * reference hands to oneImageNLF: d_out (float64) = min(f0, f1), a NaN in either frame wins.  Both
 * frames have the type `dtype`.  Not in place. */
int ipa_pair_min_dev(ipa_ctx* ctx, const void* d_f0, const void* d_f1, int dtype, int h, int w, long pitch0,
                     long pitch1, double* d_out, long out_pitch);

typedef enum {
  IPA_NLF_BOUNDED_SQRT = 0, /* {minY, ax, ay}:        max(nan_to_num(ay * sqrt(x - ax)), minY)        */
  IPA_NLF_CLIPPED_POLY = 1, /* {p2, p1, p0, x0, x1}:  np.poly1d(p)(np.clip(x, x0, x1))                */
  IPA_NLF_CONSTANT = 2      /* {c}:                   c, whatever x is                                */
} ipa_nlf_kind;
/* replaces `noise_level_function(self.mma.avg) * nStd` of features/SingleTimeEffectDetection.py:44
 * for the three functions camera/NoiseLevelFunction.py:94-151 (_evaluate, smooth) can return:
 * d_thr = nlf(d_x) * nstd over a float64 frame.  The bounded square root is the arithmetic of the
 * first pair of ipa_ste_dev.  The polynomial runs in numpy's Horner order ((0*c + p2)*c + p1)*c + p0
 * on c = minimum(maximum(x, x0), x1); a NaN x gives NaN.  params is a HOST pointer to 3 / 5 / 1
 * doubles; an unknown kind is IPA_ERR_BAD_ARG.  d_thr may be d_x itself (same pitch). */
int ipa_nlf_threshold_dev(ipa_ctx* ctx, const double* d_x, int h, int w, long pitch, int kind,
                          const double* params, double nstd, double* d_thr, long thr_pitch);

/* replaces getLinearityFunction of camera/DarkCurrentMap.py:61-80 in one launch: per pixel of a
 * (T, h, w) stack the line image(t) = offset + ascent * t through the samples that are not above
 * mx_intensity.  times: T doubles (HOST).  Sample k is valid where !(y[k] > mx_intensity) - the
 * reference masks `imgs > mxIntensity`, so a NaN sample is valid and poisons its pixel.  In frame
 * order, masked samples adding nothing:
 *   n  = #valid;  mx = sum(x[k]) / n;  my = sum(y[k]) / n
 *   sxx = sum((x[k]-mx)*(x[k]-mx));  sxy = sum((x[k]-mx)*(y[k]-my))
 *   ascent = sxy / sxx;  offset = my - ascent*mx
 *   error  = sqrt(sum((y[k] - (offset + ascent*x[k]))^2) / n)          the fit's rms residual
 * then the reference's own steps (:73-78):
 *   ascent = 0 where NaN
 *   min_ascent > 0: where ascent < min_ascent: offset += 0.5*(min(x)+max(x)) * ascent, ascent = 0
 * min(x), max(x) over all T times (np.min(expTimes)).  A pixel with n <= 1 ends with ascent 0 and
 * NaN in offset and error.
 * UNPINNED: fancytools.math.linRegressUsingMasked2dArrays, which the reference calls for the first
 * block, is neither in the reference tree nor installed where the fixtures are generated; the
 * least-squares definition above is this project's (as the running mean of ipa_ste_dev is).
 * 2 <= T <= 64 (above: IPA_ERR_UNSUPPORTED, nothing written; below: IPA_ERR_BAD_ARG).  d_offset,
 * d_ascent, d_error: float64, out_pitch; stack and outputs must not overlap (IPA_ERR_BAD_ARG).
 * For T <= 16 a pixel's samples stay in registers between the sums: every frame value is read
 * once.  Longer stacks read them once per sum. */
int ipa_stack_linregress_dev(ipa_ctx* ctx, const void* d_stack, int dtype, int T, int h, int w, long pitch,
                             long frame_stride, const double* times, double mx_intensity, double min_ascent,
                             double* d_offset, double* d_ascent, double* d_error, long out_pitch);

/* the model camera/CameraCalibration.py:509-519 (calcDarkCurrent) holds: bg = offset + ascent * t,
 * then `limit` where that exceeds it; NaN is kept.  d_out is IPA_F32 or IPA_F64 (IPA_ERR_UNSUPPORTED
 * otherwise), rounded once from the float64 value.  Not in place. */
int ipa_dark_current_eval_dev(ipa_ctx* ctx, const double* d_offset, const double* d_ascent, int h, int w,
                              long pitch, double t, double limit, void* d_out, int out_dtype, long out_pitch);

/* replaces `i[:] = avg` of camera/DarkCurrentMap.py:108-114 (the averages stack has the type of
 * imgs[0]): float64 -> uint8 / uint16 / float32 / float64 by C conversion, integers truncated
 * toward zero.  Defined for finite values inside the target's range; NaN into a float type stays
 * NaN.  Not in place. */
int ipa_cast_trunc_dev(ipa_ctx* ctx, const double* d_in, int h, int w, long pitch, void* d_out, int out_dtype,
                       long out_pitch);

/* ---------------------------------------------------------------- flat field calibration */
/* The frame passes of camera/flatField/flatFieldFromCloseDistance.py and camera/flatField/
 * sensitivity.py.  Frames are uint8 / uint16 / float32 / float64 (IPA_ERR_UNSUPPORTED otherwise),
 * pitches in elements; all arithmetic is float64, every operation correctly rounded and unfused. */

/* replaces transform/imgAverage.py:14-21 (`out = float(i0); out += float(i); out /= len(images)`):
 * d_out (float64) = the sum of the n frames in frame order, divided by n.  Any n >= 1.  A colour
 * stack (n, h, w, 3) is served as (n, h, 3 * w).  Stack and result must not overlap. */
int ipa_stack_mean_dev(ipa_ctx* ctx, const void* d_stack, int dtype, int n, int h, int w, long pitch,
                       long frame_stride, double* d_out, long out_pitch);

/* replaces toGray of transformations.py:126-135 (np.average(img, axis=-1, weights=(0.299, 0.587,
 * 0.114))) on an interleaved float64 frame (h, w, 3), `pitch` elements per row (>= 3 * w):
 * d_out = ((r * wgt[0] + g * wgt[1]) + b * wgt[2]) / wsum.  wgt: 3 doubles (HOST); wsum is the
 * caller's, computed as numpy computes wgt.sum().  Not in place. */
int ipa_luma_dev(ipa_ctx* ctx, const double* d_img, int h, int w, long pitch, const double* wgt, double wsum,
                 double* d_out, long out_pitch);

typedef enum {
  IPA_EXTREMUM_MEDIAN_MAX = 0, /* median_filter(a[::sy, ::sx], 3).max(), float64 frames */
  IPA_EXTREMUM_MIN = 1         /* a[::sy, ::sx].min() */
} ipa_extremum_mode;
/* replaces `median_filter(img[::10, ::10], 3).max()` of camera/flatField/flatFieldFromCloseDistance.py
 * :36 and :91 (scipy's 'reflect' border on the strided grid: the edge sample repeated) and the
 * `img[::s0 // 10, ::s1 // 10].min()` of its sort key (:62).  *result (HOST) is the extremum as a
 * double - every value of the four element types is one -, a NaN among the samples wins as in
 * numpy.  Per-workgroup partial extrema and a second small pass, no float atomics; the call
 * synchronises.  step_y, step_x >= 1. */
int ipa_strided_extremum_dev(ipa_ctx* ctx, const void* d_img, int dtype, int h, int w, long pitch, int step_y,
                             int step_x, int mode, double* result);

/* replaces `img -= bg` and `img /= mx` of camera/flatField/flatFieldFromCloseDistance.py:34-37 and
 * `ma / mx` of :96: d_out = (d_img - bg) / div over float64 frames, or one of the two steps
 * (subtract = 0 / divide = 0).  bg is d_bg (float64, bg_pitch) or, where that is NULL, bg_value.
 * d_out may be d_img itself (same pitch). */
int ipa_flat_scale_dev(ipa_ctx* ctx, const double* d_img, int h, int w, long pitch, const double* d_bg,
                       long bg_pitch, double bg_value, int subtract, double div, int divide, double* d_out,
                       long out_pitch);

/* replaces `thresh = det.noSTE - nlf(det.noSTE) * nstd; mask = i > thresh` of camera/flatField/
 * flatFieldFromCloseDistance.py:80-81: d_mask (uint8) = frame > avg - nlf(avg) * nstd, compared in
 * float64, 0 where either side is NaN.  kind / params as in ipa_nlf_threshold_dev.  The mask is
 * what ipa_ste_dev takes as d_mask. */
int ipa_nlf_lower_mask_dev(ipa_ctx* ctx, const void* d_img, int dtype, int h, int w, long pitch,
                           const double* d_avg, long avg_pitch, int kind, const double* params, double nstd,
                           unsigned char* d_mask, long mask_pitch);

/* replaces `fastMean(median_filter(i - bg, 3))` of camera/flatField/sensitivity.py:21-23 up to the
 * small image: d_small (float64, dh x dw) = cv2.resize(median_filter(frame - bg, 3), (dw, dh),
 * INTER_AREA) as ipa_resize_dev computes it.  bg as in ipa_nlf_signal_dev.  Where h = isy * dh and
 * w = isx * dw this is one kernel that writes no frame-sized intermediate: the medians of a block
 * are summed row-major in groups of four, times (float)(1 / area).  Otherwise the median frame goes
 * through the context's workspace and ipa_resize_dev shrinks it.  Enlarging is IPA_ERR_UNSUPPORTED. */
int ipa_sens_shrink_dev(ipa_ctx* ctx, const void* d_img, int dtype, int h, int w, long pitch,
                        const double* d_bg, long bg_pitch, double bg_value, int dh, int dw, double* d_small,
                        long small_pitch);

/* replaces `i /= smooth; out += i` and `out /= n + 1` of camera/flatField/sensitivity.py:24-29:
 * d_acc (float64) = (frame - bg) / up(small) where first, d_acc + that otherwise, then / n_last
 * where n_last > 0.  up(small) is cv2.resize(small, (w, h), INTER_LINEAR) as ipa_resize_dev
 * computes it, evaluated per pixel: the two horizontal blends, each rounded to float64, then the
 * vertical one.  d_acc must not overlap the frame, bg or small. */
int ipa_sens_accumulate_dev(ipa_ctx* ctx, const void* d_img, int dtype, int h, int w, long pitch,
                            const double* d_bg, long bg_pitch, double bg_value, const double* d_small, int dh,
                            int dw, long small_pitch, double* d_acc, long acc_pitch, int first, int n_last);

/* What uncertainty/temporalSignalStability.py needs after its line fit (ipa_stack_linregress_dev
 * with mx_intensity = inf, min_ascent = 0).  Frames are uint8 / uint16 / float32 / float64, pitches
 * and frame strides in elements; all arithmetic is float64, every operation correctly rounded and
 * unfused. */

/* replaces uncertainty/temporalSignalStability.py:56-66 and _calcAvgLen (:83-107) in one launch:
 * fn_imgs, diff, median_filter(diff, 5) over the (T, h, w) cube, evt = |.| > 0.5 * error and the
 * average run length of the events along the frames.  times: T doubles (HOST); d_offset, d_ascent,
 * d_error: float64 planes of one pitch (plane_pitch).  Per voxel, in this order:
 *   r[k](y, x)  = (double)img[k](y, x) - (offset(y, x) + times[k] * ascent(y, x))
 *   c           = 0.5 * error(y0, x0)                       the threshold of the CENTRE pixel
 *   plus[k]     = #{r[k'](y, x) >  c},  minus[k] = #{r[k'](y, x) < -c}  over the 5 x 5 x 5 window
 *                 around (k, y0, x0), indices beyond the cube taken by scipy's `reflect`
 *                 (d c b a | a b c d) on all three axes, reflected as often as it takes
 *   evt[k]      = plus[k] >= 63 || minus[k] >= 63
 * The median of 125 finite values is the value of rank 62 (from 0): it is above c exactly when at
 * least 63 values are, below -c exactly when at least 63 are below -c, so evt equals
 * |median_filter(diff, 5)| > 0.5 * error bit for bit without the median being formed.  A residual
 * beyond the centre pixel is formed with ITS pixel's offset and ascent.  Then per pixel, along k:
 *   nvals = #{evt[k]};  nclusters = #runs of consecutive event frames
 *   avlen = nclusters == 0 ? 0 : (double)nvals / (double)nclusters
 * d_avlen: float64.  d_zero_mask (uint8, may be NULL): 1 where avlen == 0, the mask of :69.
 * d_events (uint8 (T, h, w), ev_pitch, ev_frame_stride; may be NULL): evt itself.
 * NaN: with a NaN sample in a window scipy's own selection depends on the order of the values;
 * the result is undefined here too.  A NaN error gives no event (every comparison is false).
 * 2 <= T <= 64 (above, or another dtype: IPA_ERR_UNSUPPORTED; below: IPA_ERR_BAD_ARG); any
 * h, w >= 1.  Null pointers, an empty image, a pitch smaller than the width, frames that overlap
 * and an output that overlaps an input or another output are IPA_ERR_BAD_ARG.  Nothing is written
 * on refusal.  Every frame value is read once per 64 x 16 tile (and its 2-pixel halo); no
 * workspace, nothing of size T*h*w but d_events. */
int ipa_tss_event_length_dev(ipa_ctx* ctx, const void* d_stack, int dtype, int T, int h, int w, long pitch,
                             long frame_stride, const double* times, const double* d_offset,
                             const double* d_ascent, const double* d_error, long plane_pitch, double* d_avlen,
                             long avlen_pitch, unsigned char* d_zero_mask, long mask_pitch,
                             unsigned char* d_events, long ev_pitch, long ev_frame_stride);

/* replaces uncertainty/temporalSignalStability.py:72-78, the tail after maskedFilter.  d_mean: the
 * mean-filtered event length (float64, NaN where masked); d_mask: uint8, non-zero where the raw
 * event length was 0.  With the edge pixel repeated beyond the image in every step:
 *   m1 = 3 x 3 maximum of mask                      maximum_filter(i, 3)
 *   a2 = m1 ? 0 : mean                              avlen[i] = 0
 *   a3 = 3 x 3 maximum of a2                        maximum_filter(avlen, 3)
 *   out = a3 == 0 ? 0 : rank 4 of the 3 x 3 of a3   median_filter(avlen, 3); avlen[i] = 0
 * Selection only: every output value is an input value or 0.  a2 is finite when every unmasked
 * pixel of d_mean is (the masked mean averages at least the pixel itself); a NaN there is
 * undefined.  Not in place (IPA_ERR_BAD_ARG), any h, w >= 1. */
int ipa_tss_finish_dev(ipa_ctx* ctx, const double* d_mean, const unsigned char* d_mask, int h, int w, long pitch,
                       long mask_pitch, double* d_out, long out_pitch);

/* ---- object / vignetting separation (csrc/ovs.hip) --------------------------------------------
 * The refinement loop of camera/flatField/vignettingFromRandomSteps.py (ObjectVignettingSeparation
 * .__next__, :238-282) for fitted images and homographies the caller supplies.  d_fits: n images on
 * the object grid (oh x ow), uint8 / uint16 / float32 / float64, fit_pitch and fit_frame_stride in
 * elements.  mats: n destination -> source matrices, 9 row-major doubles each (HOST; they travel
 * through the context's table buffer, nothing is allocated per call).  A sample is what
 * ipa_warp_perspective_dev computes on a float64 image with IPA_INTER_LINEAR | IPA_INTER_Q5,
 * IPA_BORDER_CONSTANT, 0.0 - the same device functions - so the results equal the composed calls
 * bit for bit.  The running mean is MaskedMovingAverage.update as the project restates it
 * (tests/golden/gen_ste_golden.py): per accepted value x, n += 1; avg = n == 1 ? x : avg + (x - avg) / n.
 * All arithmetic is float64, every division IEEE, nothing fused beyond the sampler's own fma.
 * 1 <= n <= 64 (0: IPA_ERR_BAD_ARG, above: IPA_ERR_UNSUPPORTED); another dtype is
 * IPA_ERR_UNSUPPORTED; null pointers, an empty image, a pitch smaller than the width, frames that
 * overlap and an output that overlaps an input or another output are IPA_ERR_BAD_ARG.  Nothing is
 * written on refusal; padding is never written. */

/* replaces camera/flatField/vignettingFromRandomSteps.py:241-249 in one launch: per object pixel,
 * for k = 0 .. n-1 in order, w = sample(ff, mats[k] * (x, y, 1)); where w != 0 (a NaN is accepted,
 * as in numpy) the running mean takes (double)fit[k](y, x) / w.  d_ff: float64 fh x fw, at most
 * 2^28 elements; d_obj: float64, d_count: int32, both oh x ow - the average and the number of
 * accepted values (0 and 0 where none was).  No warped frame is written anywhere. */
int ipa_ovs_object_dev(ipa_ctx* ctx, const double* d_ff, int fh, int fw, long ff_pitch, const void* d_fits, int dtype,
                       int n, int oh, int ow, long fit_pitch, long fit_frame_stride, const double* mats,
                       double* d_obj, long obj_pitch, int* d_count, long count_pitch);

/* replaces camera/flatField/vignettingFromRandomSteps.py:253-265 in one launch: per flat-field
 * pixel, for k in order, v = sample(div[k], mats[k] * (x, y, 1)) of the image div[k] that is never
 * stored - NaN where d_masks[k] (uint8, oh x ow per frame) is set, (double)fit[k] / obj elsewhere,
 * each tap formed when it is read; taps beyond the frame are the constant 0 and a footprint wholly
 * outside gives 0 without a division.  Then np.nan_to_num (NaN -> 0, +-inf -> +-DBL_MAX), and the
 * running mean takes v where v != 0.  d_ff: float64, d_count: int32, both fh x fw.
 * clip01 != 0 stores np.clip(avg, 0, 1) (NaN stays) - the flat field of the next step, :278.
 * d_sub (may be NULL): float64 ceil(fh / sub_step) x ceil(fw / sub_step), the UNCLIPPED average at
 * every sub_step-th pixel of every sub_step-th row, what the residuum of :269-270 reads. */
int ipa_ovs_flatfield_dev(ipa_ctx* ctx, const double* d_obj, long obj_pitch, const void* d_fits, int dtype, int n,
                          int oh, int ow, long fit_pitch, long fit_frame_stride, const unsigned char* d_masks,
                          long mask_pitch, long mask_frame_stride, const double* mats, double* d_ff, int fh, int fw,
                          long ff_pitch, int* d_count, long count_pitch, int clip01, double* d_sub, int sub_step,
                          long sub_pitch);

/* one MaskedMovingAverage.update(data, mask) (camera/flatField/vignettingFromRandomSteps.py:146-151,
 * the initial flat field) on device-resident state: where d_mask (uint8; NULL: everywhere) is set,
 * n += 1; x = (double)data; avg = n == 1 ? x : avg + (x - avg) / n.  d_avg: float64, d_n: int32,
 * updated in place; d_data: uint8 / uint16 / float32 / float64.  The state must not overlap the
 * inputs (IPA_ERR_BAD_ARG). */
int ipa_masked_running_mean_dev(ipa_ctx* ctx, double* d_avg, long avg_pitch, int* d_n, long n_pitch, const void* d_data,
                                int dtype, long data_pitch, const unsigned char* d_mask, long mask_pitch, int h,
                                int w);

/* ---- 2-D polynomial fits of masked frames (csrc/poly.hip) ---------------------------------------
 * interpolate/polyfit2d.py (polyfit2dGrid) and camera/flatField/postprocessing/polynomial.py.  The
 * reference fits raw monomials x**i * y**j by lstsq on an (n_valid, (o+1)^2) design matrix; here the
 * basis is T_j(v) T_i(u), Chebyshev polynomials (T_0 = 1, T_1 = u, T_k = 2 u T_{k-1} - T_{k-2}) of
 *   u = (2 x - (w - 1)) / (w - 1),  v = (2 y - (h - 1)) / (h - 1)   (0 for a dimension of size 1):
 * the same polynomial space in a basis that stays well conditioned.  Frames are float32 / float64
 * (anything else IPA_ERR_UNSUPPORTED), order is 0 .. 5 (above: IPA_ERR_UNSUPPORTED), masks uint8
 * with non-zero = invalid.  The (o+1)^2 x (o+1)^2 system is the caller's to solve. */
typedef enum {
  IPA_POLY_FILL,   /* replace the masked pixels (a NULL mask: every pixel); the others are copied */
  IPA_POLY_ALL,    /* write every pixel */
  IPA_POLY_GRID    /* evaluate at an outgrid of pixel positions */
} ipa_poly_mode;

/* polyfit2d.py:13-18 with :46-49 - the sums of the normal equations over the VALID pixels (d_mask
 * NULL: all; a masked pixel is selected out, its value - NaN in the reference's own example - never
 * enters a sum).  moments (host): n = 2 order + 1, k = order + 1,
 *   moments[b n + a]           = sum T_b(v) T_a(u)      a, b <= 2 order
 *   moments[n n + j k + i]     = sum z T_j(v) T_i(u)    i, j <= order
 *   moments[n n + k k]         = the number of valid pixels.
 * The Gram matrix follows from T_i T_k = (T_{i+k} + T_{|i-k|}) / 2.  Per-workgroup partial sums are
 * added in a fixed order by a second launch, no float atomics: two calls give identical bits.
 * Synchronises the stream. */
int ipa_poly2d_moments_dev(ipa_ctx* ctx, const void* d_img, int dtype, int h, int w, long pitch,
                           const unsigned char* d_mask, long mask_pitch, int order, double* moments);

/* polyfit2d.py:22-28 with :50-64 - the polynomial with the (order+1)^2 host coefficients coef[j k + i]
 * of T_j(v) T_i(u), evaluated in double in the operation order csrc/poly.hip spells out and rounded
 * once into the frame's type.  h x w is the frame of the coordinate map in every mode.
 *   IPA_POLY_FILL  d_out = d_in with the pixels under d_mask replaced (d_mask NULL: all of them);
 *                  d_out may be d_in itself (same pointer and pitch: in place)
 *   IPA_POLY_ALL   every pixel of d_out (h x w); d_in may be NULL, d_mask is ignored
 *   IPA_POLY_GRID  d_out is gh x gw, pixel (r, c) evaluated at the position (d_gy, d_gx)[r][c] (float64,
 *                  grid_pitch); positions outside the frame extrapolate; d_in and d_mask are ignored
 * residuum (host, may be NULL; FILL and ALL with d_in): sum |new - old| over the replaced pixels, new
 * as stored - polynomial.py:37 times the frame's size.  Per-tile partials added in a fixed order;
 * asking for it synchronises the stream.  An overlap of d_out with anything but an in-place d_in is
 * IPA_ERR_BAD_ARG. */
int ipa_poly2d_eval_dev(ipa_ctx* ctx, const double* coef, int order, int mode, const void* d_in, int dtype, int h,
                        int w, long in_pitch, const unsigned char* d_mask, long mask_pitch, const double* d_gy,
                        const double* d_gx, int gh, int gw, long grid_pitch, void* d_out, long out_pitch,
                        double* residuum);

/* polynomial.py:10-14 (_highGrad) - d_mask = maximum_filter(|laplace(img, mode='reflect')| > threshold,
 * size): the Laplacian per axis c * (-2) + (l + r) in double, rounded to the frame's type, axis 0 plus
 * axis 1 and the comparison in the frame's type (scipy's arithmetic); then the separable dilation by
 * a window of offsets -(size / 2) .. size - size / 2 - 1, 1 <= size <= 31 (above:
 * IPA_ERR_UNSUPPORTED).  d_mask: uint8 0 / 1, must not overlap the frame; *count (host): its sum.
 * Synchronises the stream. */
int ipa_high_grad_dev(ipa_ctx* ctx, const void* d_img, int dtype, int h, int w, long pitch, double threshold, int size,
                      unsigned char* d_mask, long mask_pitch, double* count);

/* polynomial.py:49 - np.clip(img, 0, 1, out=img): in place, NaN stays. */
int ipa_clip01_dev(ipa_ctx* ctx, void* d_img, int dtype, int h, int w, long pitch);

/* ---- flat field from spot images (csrc/spot.hip) ------------------------------------------------
 * camera/flatField/vignettingFromSpotAverage.py ("Method B") and the primitives under it: a
 * histogram by np.histogram's bin rule, the range skimage's threshold_otsu starts from, the eroded
 * threshold mask, connected-component labelling, component sizes, the largest component and the
 * copy of a spot into the sparse result.  Frames are uint8 / uint16 / float32 / float64 (another
 * dtype: IPA_ERR_UNSUPPORTED), pitches in elements; a frame value is (double)px - bg, one IEEE
 * subtraction, with bg = d_bg[y][x] (float64, bg_pitch) or, where d_bg is NULL, the scalar bg.
 * h * w < 2^31.  Null pointers, an empty image and a pitch smaller than the width are
 * IPA_ERR_BAD_ARG; nothing is written on refusal and padding is never written.  The calls that
 * return host values synchronise the stream. */

/* vignettingFromSpotAverage.py:56 (threshold_otsu's `np.all(image == first_pixel)` and the range of
 * np.histogram) - range (HOST, 5 doubles) = {min, max, number of NaN, number of +-inf, the first
 * pixel}; min and max are exact and skip NaN (+inf, -inf without a comparable value).
 * Per-workgroup partials and a second small launch. */
int ipa_spot_range_dev(ipa_ctx* ctx, const void* d_img, int dtype, int h, int w, long pitch, const double* d_bg,
                       long bg_pitch, double bg, double* range);

/* vignettingFromSpotAverage.py:56 (np.histogram(image.ravel(), nbins) inside threshold_otsu) -
 * counts (HOST, nbins) over the edges (HOST, nbins + 1, np.linspace(lo, hi, nbins + 1)), by
 * np.histogram's rule for equal bins: the estimate k = (intp)((x - e[0]) * (nbins / (e[nbins] - e[0]))),
 * k == nbins -> nbins - 1, then `x < e[k]` lowers k and `x >= e[k + 1]` with k != nbins - 1 raises
 * it, so that e[k] <= x < e[k + 1] with the last bin closed.  Every frame value must be finite
 * and lie within [e[0], e[nbins]] (ipa_spot_range_dev tells).  1 <= nbins <= 2048 (above:
 * IPA_ERR_UNSUPPORTED).  Per-wave tables in LDS, integer adds only: the counts are exact. */
int ipa_spot_histogram_dev(ipa_ctx* ctx, const void* d_img, int dtype, int h, int w, long pitch, const double* d_bg,
                           long bg_pitch, double bg, const double* edges, int nbins, unsigned long long* counts);

/* vignettingFromSpotAverage.py:61 (minimum_filter(img > t, 3)) - d_mask (uint8 0 / 1) = the 3 x 3
 * erosion of `frame - bg > t`; positions beyond the frame do not count (scipy's `reflect` border on
 * a bool image), NaN > t is false.  Not in place. */
int ipa_spot_mask_dev(ipa_ctx* ctx, const void* d_img, int dtype, int h, int w, long pitch, const double* d_bg,
                      long bg_pitch, double bg, double t, unsigned char* d_mask, long mask_pitch);

/* vignettingFromSpotAverage.py:61 (skimage.measure.label(., background=0, return_num=True); also
 * scipy.ndimage.label) - d_labels (int32): 0 where d_mask (uint8) is 0, otherwise the number of the
 * pixel's connected component, 1 .. *n (HOST), numbered in the raster order of the components'
 * first pixels.  connectivity 1: the 4 edge neighbours (scipy's default); 2: all 8 (skimage's
 * default on images); anything else IPA_ERR_BAD_ARG.  A union-find whose roots are the smallest
 * linear index of their component, tiles in LDS, seams by atomic minimum; 4 h w bytes of the
 * context's workspace.  d_labels must not overlap d_mask. */
int ipa_label_dev(ipa_ctx* ctx, const unsigned char* d_mask, int h, int w, long mask_pitch, int connectivity,
                  int* d_labels, long label_pitch, int* n);

/* vignettingFromSpotAverage.py:63 (spot_sizes) - d_sizes (DEVICE, n int64): d_sizes[i] = the number
 * of pixels of label i + 1; labels beyond n are not counted.  Integer adds, aggregated per wave. */
int ipa_label_sizes_dev(ipa_ctx* ctx, const int* d_labels, int h, int w, long label_pitch, int n,
                        long long* d_sizes);

/* vignettingFromSpotAverage.py:66 and :72 (np.argmax(spot_sizes) + 1; the sums under
 * center_of_mass) - result (HOST, 4 int64) = {label, size, sum of y, sum of x} of the largest of
 * the n components, the lowest label among equals; all 0 for n = 0.  The sums are exact integers:
 * center_of_mass is sum / size in float64 on the host. */
int ipa_label_largest_dev(ipa_ctx* ctx, const int* d_labels, int h, int w, long label_pitch, int n,
                          long long* result);

/* vignettingFromSpotAverage.py:72-77 (mx2; fitimg[spot] = img[spot]; mask[spot] = 1) - for the
 * pixels p of `label` in d_labels (the spot form) or, where d_labels is NULL, of the whole rows
 * row_a and row_b (the row form: what `img[spot]` selects once `spot` is an index pair),
 * d_fit[p] (float64) = frame[p] - bg and d_mask[p] (uint8) = 1; every other pixel of both is left
 * alone.  result (HOST, 3 doubles) = {maximum (NaN if a value is; -inf for none), sum, count}; the
 * sum is added in an order the frame's size alone decides: identical bits from call to call.
 * label >= 1; 0 <= row_a, row_b < h.  An output that overlaps anything is IPA_ERR_BAD_ARG. */
int ipa_spot_take_dev(ipa_ctx* ctx, const void* d_img, int dtype, int h, int w, long pitch, const double* d_bg,
                      long bg_pitch, double bg, const int* d_labels, long label_pitch, int label, int row_a,
                      int row_b, double* d_fit, long fit_pitch, unsigned char* d_mask, long mask_pitch,
                      double* result);

/* ---- flat field from discrete steps (csrc/steps.hip) --------------------------------------------
 * camera/flatField/vignettingFromDiscreteSteps.py up to its post-processing: the device is imaged
 * at known cell positions, every frame is reduced to the thresholded means of a grid of cells, and
 * device and flat field are separated iteratively on that grid.  At most 64 frames
 * (IPA_ERR_UNSUPPORTED above); pitches and strides in elements.  Nothing is written on refusal. */

/* replaces vignettingFromDiscreteSteps.py:228-246 (array/subCell2D.py:87-107, subCell2DFnArray with
 * the cell function of :228-234) for all n frames: cell (i, j) is rows row_edges[i] ..
 * row_edges[i + 1] - 1 and columns col_edges[j] .. col_edges[j + 1] - 1 (HOST tables of g0 + 1 and
 * g1 + 1 entries that do not decrease and lie within [0, h] and [0, w]: the slices of
 * subCell2DSlices clipped to the frame).  With x = (double)frame - (double)bg (d_bg: one h x w
 * frame of any of the four types, or NULL: x = (double)frame), count = #(x > thresh) - a NaN is no
 * sample - and size = rows * cols, d_grid[n][i][j] (float64, dense n x g0 x g1) is NaN where
 * size == 0 or 2 * count < size and sum(x where x > thresh) / count elsewhere.
 * Every frame element is read once and nothing of frame size is written.  The sum's order is
 * fixed - a lane adds up to 32 rows of its column, a fixed tree adds the columns of a cell within
 * 256 columns, such spans are added left to right and the 32-row segments top to bottom; no
 * atomics - so two calls give identical bits.  The partial sums live in the context's workspace:
 * n * g0 * S * g1 of them, S = ceil(tallest cell row / 32), at most 2^24 (IPA_ERR_UNSUPPORTED
 * above, as for w >= 2^26). */
int ipa_cell_means_dev(ipa_ctx* ctx, const void* d_frames, int dtype, int n, int h, int w, long pitch,
                       long frame_stride, const void* d_bg, int bg_dtype, long bg_pitch, double thresh,
                       const int* row_edges, int g0, const int* col_edges, int g1, double* d_grid);

/* replaces vignettingFromDiscreteSteps.py:257-281 and :316 in ONE launch of one workgroup.
 * d_grid: float64, dense n x g0 x g1, what ipa_cell_means_dev wrote.  rects (HOST): per frame the
 * six ints {q0, q1, qq0, qq1, l0, l1} of _DeviceAndGridSlice.iter() (:26-60): device cells
 * [q0, q0 + l0) x [q1, q1 + l1) are grid cells [qq0, qq0 + l0) x [qq1, qq1 + l1); a rectangle that
 * leaves the n0 x n1 device or the grid is IPA_ERR_BAD_ARG.  Every np.nanmean(axis=0) is numpy's:
 * NaN -> 0, a sum in frame order, divided by the number of non-NaN terms (0 / 0 = NaN); the
 * initial flat field is nanmean(grid) [- bg_value where subtract_bg] / nanmax.
 * d_ff: float64 g0 x g1; d_avgobj: float64 n0 x n1; d_density: int32 g0 x g1, the number of
 * non-NaN frames per cell; *iterations and *dev (HOST): the iterations run and the last RMS
 * deviation (summed in this kernel's own fixed order; only the stop decision reads it).
 * DEVIATION: the reference's inner loops reuse the name of its iteration counter, so max_iter
 * never ends its loop.  Here iteration k = 1, 2, ... is the last when dev < max_dev or
 * k > max_iter + 1 - what the reference's counter would give - so at most max_iter + 2 run; a NaN
 * dev runs to that cap.  0 <= max_iter <= 10000 (IPA_ERR_BAD_ARG); at most 2^16 grid cells and
 * 2^16 device cells (IPA_ERR_UNSUPPORTED).  Synchronises the stream. */
int ipa_steps_separate_dev(ipa_ctx* ctx, const double* d_grid, int n, int g0, int g1, int n0, int n1,
                           const int* rects, double bg_value, int subtract_bg, int max_iter, double max_dev,
                           double* d_ff, double* d_avgobj, int* d_density, int* iterations, double* dev);

/* replaces interpolate/offsetMeshgrid.py:25-27 (and the astype(np.float32) of
 * vignettingFromDiscreteSteps.py:312): d_yy[y][x] = lin0[y], d_xx[y][x] = lin1[x] with
 * lin[i] = i * step + start and, for an axis longer than 1, the last element = stop - np.linspace
 * with step = (stop - start) / (len - 1) formed on the host.  dtype IPA_F64, or IPA_F32: the
 * double rounded once. */
int ipa_offset_meshgrid_dev(ipa_ctx* ctx, double start0, double step0, double stop0, double start1, double step1,
                            double stop1, int h, int w, int dtype, void* d_yy, void* d_xx, long pitch);

/* replaces vignettingFromDiscreteSteps.py:289 (np.isnan): d_mask (uint8) = 1 where the float32 /
 * float64 frame is NaN, 0 elsewhere. */
int ipa_isnan_mask_dev(ipa_ctx* ctx, const void* d_in, int dtype, int h, int w, long pitch, unsigned char* d_mask,
                       long mask_pitch);

/* ---- vignetting functions fitted to masked flat fields (csrc/fn2d.hip) ----------------------------
 * camera/flatField/postprocessing/function.py with the two functions camera/flatField/postProcessing.py
 * :50-74 fits through fancytools' fit2dArrayToFn.  The model's x is the ROW index, its y the COLUMN
 * index.  Frames are float32 / float64 (anything else IPA_ERR_UNSUPPORTED), masks uint8 with
 * non-zero = invalid; params is a HOST pointer.  An unknown model is IPA_ERR_BAD_ARG. */
typedef enum {
  IPA_FN2D_KW = 0,   /* equations/vignetting.py:21-37 with tilt = 0; params {f, alpha, cx, cy}:
                        d = sqrt((x - cx)^2 + (y - cy)^2);  (1 / (1 + (d / f)^2)^2) * (1 - alpha d) */
  IPA_FN2D_AOV = 1   /* equations/angleOfView.py:29-40; params {tan(a), c0, c1}, the fitted parameter is a:
                        1 / sqrt(1 + tan(a) * (((x - c0)^2 + (y - c1)^2) / c0)) */
} ipa_fn2d_model;

/* function.py:35-37 (one evaluation of the least-squares problem curve_fit solves) - over the VALID
 * pixels (d_mask NULL: all; a masked pixel is selected out, a NaN under the mask enters nothing),
 * with model value m, its Jacobian J by the P fitted parameters (KW: f, alpha, cx, cy; AoV: a) and
 * r = frame - m, sums (HOST, P (P + 1) / 2 + P + 2 doubles: 16 for KW, 4 for AoV) =
 *   the upper triangle of J^T J by rows | J^T r | sum r^2 | the number of valid pixels.
 * alpha * dx / d counts 0 where d == 0.  Per-workgroup partial sums are added in a fixed order by a
 * second launch, no float atomics: two calls give identical bits.  Synchronises the stream. */
int ipa_fn2d_normal_dev(ipa_ctx* ctx, const void* d_img, int dtype, int h, int w, long pitch,
                        const unsigned char* d_mask, long mask_pitch, int model, const double* params, double* sums);

/* function.py:35-40 - the model evaluated in double in the reference's operation order (bit for bit
 * numpy's value) and rounded once into the frame's type; the modes are those of ipa_poly2d_eval_dev:
 *   IPA_POLY_FILL  d_out = d_in with the pixels under d_mask replaced (d_mask NULL: all of them);
 *                  d_out may be d_in itself (same pointer and pitch: in place)
 *   IPA_POLY_ALL   every pixel of d_out (h x w); d_in and d_mask are ignored
 *   IPA_POLY_GRID  d_out is gh x gw, pixel (r, c) evaluated at row position d_gy[r][c] and column
 *                  position d_gx[r][c] (float64, grid_pitch); d_in and d_mask are ignored
 * maximum (host, may be NULL): np.max of all of d_out, the kept pixels included - NaN if any pixel
 * is; asking for it synchronises the stream.  An overlap of d_out with anything but an in-place d_in
 * is IPA_ERR_BAD_ARG. */
int ipa_fn2d_eval_dev(ipa_ctx* ctx, int model, const double* params, int mode, const void* d_in, int dtype, int h,
                      int w, long in_pitch, const unsigned char* d_mask, long mask_pitch, const double* d_gy,
                      const double* d_gx, int gh, int gw, long grid_pitch, void* d_out, long out_pitch,
                      double* maximum);

/* function.py:42 - img /= div in the frame's type (div rounded to it first): numpy's true division.
 * In place. */
int ipa_fn2d_divide_dev(ipa_ctx* ctx, void* d_img, int dtype, int h, int w, long pitch, double div);

#ifdef __cplusplus
}
#endif
#endif /* IMGPROC_HIP_H */
