/*
 * mi355cv.h -- C ABI of libmi355cv.so: the MI355X (gfx950) implementation of
 * OpenCV's imgproc hot path, shaped as a drop-in for the reference's imgproc
 * HAL replacement interface (reference: modules/imgproc/src/hal_replacement.hpp).
 *
 * Every `mi355cv_<hook>` below has EXACTLY the parameter list of the
 * `hal_ni_<hook>` stub it replaces (file:line cited per function), so a HAL
 * header only has to `#undef cv_hal_<hook>` / `#define cv_hal_<hook> mi355cv_<hook>`
 * (see include/mi355cv_hal.hpp and INTEGRATION.md).
 *
 * Contract (hal_replacement.hpp:1342-1357, core/hal/interface.h:9-11):
 *   return 0  (CV_HAL_ERROR_OK)              -> dst holds the result
 *   return 1  (CV_HAL_ERROR_NOT_IMPLEMENTED) -> nothing was written; caller falls back to its CPU path
 *   return <0 (CV_HAL_ERROR_UNKNOWN)         -> device failure after dst may have been touched
 * Hooks never throw.  Image pointers may be plain host memory (staged through
 * a pinned bounce buffer + H2D/D2H, synchronous) or device / managed memory
 * (launched in place on the calling thread's stream; synchronous unless
 * mi355cv_setAsync(1)).  There is NO CPU fallback inside this library.
 *
 * Plain C: pointers, sizes, ints and doubles only.
 */
#ifndef MI355CV_H
#define MI355CV_H

#include <stddef.h>
#include <stdint.h>
#ifndef __cplusplus
#include <stdbool.h>
#endif

#ifdef __cplusplus
extern "C" {
#endif

#ifndef MI355CV_API
#define MI355CV_API __attribute__((visibility("default")))
#endif

typedef unsigned char mi355cv_uchar;

/* return codes == CV_HAL_ERROR_* (modules/core/include/opencv2/core/hal/interface.h:9-11) */
#define MI355CV_OK               0
#define MI355CV_NOT_IMPLEMENTED  1
#define MI355CV_ERROR_UNKNOWN   -1

/* depth / border / interpolation constants, numerically equal to the reference's
 * (core/hal/interface.h:66-80, core/base.hpp:332-345, imgproc.hpp:248-294) */
#define MI355CV_8U 0
#define MI355CV_8S 1
#define MI355CV_16U 2
#define MI355CV_16S 3
#define MI355CV_32S 4
#define MI355CV_32F 5
#define MI355CV_64F 6
#define MI355CV_MAKETYPE(depth, cn) ((depth) + (((cn) - 1) << 3))
#define MI355CV_MAT_DEPTH(type) ((type) & 7)
#define MI355CV_MAT_CN(type) ((((type) >> 3) & 511) + 1)

#define MI355CV_BORDER_CONSTANT    0
#define MI355CV_BORDER_REPLICATE   1
#define MI355CV_BORDER_REFLECT     2
#define MI355CV_BORDER_WRAP        3
#define MI355CV_BORDER_REFLECT_101 4
#define MI355CV_BORDER_TRANSPARENT 5
#define MI355CV_BORDER_ISOLATED    16

#define MI355CV_INTER_NEAREST 0
#define MI355CV_INTER_LINEAR  1
#define MI355CV_INTER_CUBIC   2
#define MI355CV_INTER_LANCZOS4 4
#define MI355CV_INTER_AREA    3
#define MI355CV_INTER_LINEAR_EXACT 5
#define MI355CV_INTER_NEAREST_EXACT 6
#define MI355CV_WARP_INVERSE_MAP 16

/* ------------------------------------------------------------------ runtime */

/* library / device bring-up; returns 0 when a gfx950 device is usable.  `device` >= 0 names the process default device (first call wins;
 * otherwise MI355CV_DEVICE, or the device the host program had current at first use). */
MI355CV_API int  mi355cv_init(int device);
/* multi-GPU in one process (one host thread + its streams per device, frames sharded by index, no data-path collective):
 * mi355cv_setDevice binds the CALLING THREAD's hooks to a device ordinal (-1: back to the process default).  Streams, events and the scratch
 * pool are kept per thread AND device; the host program's own current HIP device is put back when a hook returns; an image that lives in
 * another GPU's memory makes the hook answer NOT_IMPLEMENTED (mi355cv_lastError names both devices).  Returns 0, or -1 for an ordinal that
 * does not exist / is not gfx950. */
MI355CV_API int  mi355cv_deviceCount(void);
MI355CV_API int  mi355cv_setDevice(int device);
MI355CV_API int  mi355cv_getDevice(void);
/* Batches across the GPUs of one node from a C / C++ host (csrc/shard.hip): device slot g of ndev takes the g-th of ndev contiguous blocks of frames whose sizes
 * differ by at most one ([g*B/ndev, (g+1)*B/ndev) when ndev divides B; the partition bench.py --gpus N and opencv_amd/shard.py use) -- and mi355cv_runSharded runs fn(user, slot, device, first, count) for every non-empty slot on its own host thread,
 * bound to devices[slot] (NULL: ordinals 0 .. ndev-1; an ordinal may repeat) when bind != 0; fn calls the ordinary mi355cv_* entry points on its frames, which must live
 * on that device (or in host / managed memory).  Returns 0, or the first non-zero code in slot order (mi355cv_lastError names slot and device).  There is no data-path
 * collective: parameters given as host arguments are uploaded by each device's own hooks; a device-resident parameter image (a matchTemplate template) is copied to every
 * device with mi355cv_replicate (one upload + an RCCL ncclBroadcast over xGMI when the list names more than one device; one hipMemcpy per device otherwise or with MI355CV_REPLICATE=copy; the Python layer broadcasts through torch.distributed). */
MI355CV_API void mi355cv_shardRange(int nframes, int ndev, int slot, int* first, int* count);
MI355CV_API int  mi355cv_runSharded(int ndev, const int* devices, int nframes, int (*fn)(void* user, int slot, int device, int first, int count), void* user, int bind);
MI355CV_API int  mi355cv_replicate(const void* src, size_t bytes, int ndev, const int* devices, void** out);
/* how the last mi355cv_replicate of this process moved its data: 0 = one hipMemcpy per device (a single device, MI355CV_REPLICATE=copy, or no usable librccl), 1 = one upload to the first device + an RCCL ncclBroadcast from
 * there over xGMI (the default for more than one device since round 6; MI355CV_REPLICATE=rccl also for one; librccl.so is resolved with dlopen; a device list RCCL cannot take -- a device twice, no library -- uses the copies) */
MI355CV_API int  mi355cv_replicateMode(void);
MI355CV_API const char* mi355cv_version(void);
/* Which host-resident images the hooks stage through HBM (device / managed pointers are always served).  0 = "auto" (the default: hooks whose CPU path is
 * multi-threaded and bandwidth-bound -- 8-bit Gaussian, colour conversions, threshold, pyrDown, morphology, integral, bilinear resize -- answer NOT_IMPLEMENTED for a plain host
 * image, because two PCIe crossings cost more than the reference's CPU path, and the caller's CPU path runs), 1 = "always" (every hook stages: for callers with no CPU path
 * to fall back to -- opencv_amd sets it when it loads the library), -1 = back to the MI355CV_HOST_POLICY environment variable.  Process-wide. */
MI355CV_API int mi355cv_setHostPolicy(int policy);
MI355CV_API int mi355cv_hostPolicy(void);          /* the policy in force: 0 auto, 1 always */
/* capacity bound of a served path by name (-1: no such key) -- "how far the GPU path was built", not the cases the reference itself has no engine for:
 * "sep_max_taps", "sep_max_taps_64f", "gauss8u_max_ksize", "gauss_float_max_ksize", "adaptive_gaussian_max_block", "adaptive_mean_max_block", "box_max_ksize",
 * "median8u_max_ksize", "bilateral_max_d", "orb_max_levels", "filter2d_dft_taps".  Needs no device.  A value above a bound is answered MI355CV_NOT_IMPLEMENTED by its hook. */
MI355CV_API int mi355cv_limit(const char* key);
MI355CV_API const char* mi355cv_lastError(void);
/* template instance + launch geometry of the dominant kernel the calling thread launched last (bench.py reports it beside the roofline) */
MI355CV_API const char* mi355cv_lastKernel(void);
/* MI355CV_TRACE=1: every entry point runs inside a roctx range named after it (roctxRangePushA / roctxRangePop, resolved with dlopen; rocprofv3 --marker-trace shows the
 * hooks around their kernels -- the role of CV_INSTRUMENT_REGION, core/private.hpp:794).  Returns 1 while ranges are emitted, 0 when MI355CV_TRACE is not set, -1 when no
 * roctx library could be loaded. */
MI355CV_API int mi355cv_traceState(void);
/* stream used for launches made by the calling thread on its current device (mi355cv_setDevice): exactly this hipStream_t (NULL = HIP's
 * null stream).  Until called -- or after mi355cv_resetStream() -- a library-owned per-thread, per-device stream is used. */
MI355CV_API int  mi355cv_setStream(void* hipStream);
MI355CV_API int  mi355cv_resetStream(void);
/* 1: calls on device-resident images return after enqueue (caller synchronises); 0 (default): synchronous */
MI355CV_API int  mi355cv_setAsync(int enable);
MI355CV_API int  mi355cv_synchronize(void);
/* number of times the named entry point ran its GPU path to completion in this process
 * (the analogue of the reference's CV_IMPL_ADD bookkeeping, core/private.hpp) */
MI355CV_API long long mi355cv_callCount(const char* entry);
/* the other side of the ledger: calls a hook DECLINED (answered MI355CV_NOT_IMPLEMENTED, so that the caller ran its own CPU path --
 * hal_replacement.hpp:1351-1357 makes that silent).  The HAL header (mi355cv_hal.hpp) and the Python mirror report every declined call
 * through mi355cv_noteDecline under the reference's hook name ("warpAffine", "sepFilter", ...); mi355cv_declineCount(hook) reads one
 * tally, mi355cv_declineCount(NULL) the total; MI355CV_PRINT_COUNTS=1 prints both ledgers at exit with the last reason per hook. */
MI355CV_API void      mi355cv_noteDecline(const char* hook);
MI355CV_API long long mi355cv_declineCount(const char* hook);
/* image bytes the hooks of this process have moved over PCIe so far (host-resident images staged into HBM + results staged back); stays
 * constant across calls on device-resident / managed images -- how a test shows that a pipeline ran in place in HBM */
MI355CV_API long long mi355cv_stagedBytes(void);
/* experiment knobs (see tools/tune_gauss.py) and the streaming-copy probe used as the measured-copy
 * roofline denominator */
MI355CV_API int mi355cv_setParam(const char* key, int value);
MI355CV_API int mi355cv_copyProbe(const void* src_dev, void* dst_dev, size_t bytes, int perThread, int nontemporal);
MI355CV_API int mi355cv_copyProbeColwalk(const void* src_dev, void* dst_dev, int width_bytes, int height, int nframes,
                                         int segRows, int unroll);
/* device memory helpers for hosts without a HIP binding (images that live in HBM) */
MI355CV_API void* mi355cv_deviceAlloc(size_t bytes);
MI355CV_API int   mi355cv_deviceFree(void* p);
MI355CV_API int   mi355cv_upload(void* dst_dev, const void* src_host, size_t bytes);
MI355CV_API int   mi355cv_download(void* dst_host, const void* src_dev, size_t bytes);
/* frame ingest / egress (the storage behind a cv::MatAllocator, core/mat.hpp:496-524): kind 0 = page-locked host memory
 * (a host frame is then staged by one DMA at PCIe rate), kind 1 = managed memory (the hooks run on it in place).  NULL without a device. */
MI355CV_API void* mi355cv_hostAlloc(size_t bytes, int kind);
MI355CV_API int   mi355cv_hostFree(void* p, int kind);

/* --------------------------------------------------- a1: Gaussian smoothing */

/* replaces hal_ni_gaussianBlurBinomial (hal_replacement.hpp:1169); caller: cv::GaussianBlur
 * smooth.dispatch.cpp:696 (8U) / :767 (16U).  Implemented: depth 8U, cn 1..4, ksize 3 or 5,
 * borders CONSTANT/REPLICATE/REFLECT/WRAP/REFLECT_101; bit-exact with fixedSmoothInvoker
 * (smooth.simd.hpp:1926). */
MI355CV_API int mi355cv_gaussianBlurBinomial(const mi355cv_uchar* src_data, size_t src_step,
        mi355cv_uchar* dst_data, size_t dst_step, int width, int height, int depth, int cn,
        size_t margin_left, size_t margin_top, size_t margin_right, size_t margin_bottom,
        size_t ksize, int border_type);

/* replaces hal_ni_gaussianBlur (hal_replacement.hpp:1146); callers smooth.dispatch.cpp:708,778,813.
 * Implemented: depth 8U with zero margins = the Q8.8 fixed-point path of GaussianBlurFixedPoint (:720), bit-exact (sigma>0 kernels are
 * generated as getGaussianKernelBitExact does).  Declined: other depths (the reference then runs sepFilter2D, whose hooks serve it) and an
 * 8U submatrix with real margins (call site :813 -- there the CPU result is sepFilter2D with float taps, not the fixed-point one). */
MI355CV_API int mi355cv_gaussianBlur(const mi355cv_uchar* src_data, size_t src_step,
        mi355cv_uchar* dst_data, size_t dst_step, int width, int height, int depth, int cn,
        size_t margin_left, size_t margin_top, size_t margin_right, size_t margin_bottom,
        size_t ksize_width, size_t ksize_height, double sigmaX, double sigmaY, int border_type);

/* a2: host-side tap generators.  getGaussianKernelBitExact (smooth.dispatch.cpp:81-198, also behind
 * cv::getGaussianKernel :200) and getGaussianKernelFixedPoint_ED (:224-258; fractionBits 8 -> the Q8.8
 * taps of the CV_8U path, 16 -> Q16.16 of CV_16U).  Bit-identical to the reference's softdouble code. */
MI355CV_API int mi355cv_getGaussianKernel(int n, double sigma, double* taps);
MI355CV_API int mi355cv_getGaussianKernelQ(int n, double sigma, int fractionBits, int64_t* taps);

/* Fixed-point separable smoothing with caller-supplied Q8.8 taps: the body of
 * GaussianBlurFixedPoint<uint16_t> (smooth.simd.hpp:2219; taps as produced by
 * getGaussianKernelFixedPoint_ED, smooth.dispatch.cpp:224).  dst = (sum_j ky[j]*sum_i kx[i]*p + 2^15) >> 16. */
MI355CV_API int mi355cv_sepSmoothFixedU8(const mi355cv_uchar* src_data, size_t src_step,
        mi355cv_uchar* dst_data, size_t dst_step, int width, int height, int cn,
        size_t margin_left, size_t margin_top, size_t margin_right, size_t margin_bottom,
        const uint16_t* kx, int kxlen, const uint16_t* ky, int kylen, int border_type);

/* Batched form (frames are independent units): `nframes` images of identical
 * geometry, frame f at src_data + f*src_frame_stride; one launch, grid-z = frame.  Host-resident batches: the chunked two-buffer pipeline (see the
 * batch section below).
 *
 * Frame counts.  grid.y and grid.z of a launch hold 65535 workgroups, and most batch kernels take their frame from blockIdx.z.  Every *Batch entry therefore does one
 * of two things with more than 65535 frames, and never hands the runtime a larger grid: it SERVES the batch -- in consecutive launches or calls of at most 65535
 * frames (mi355cv_resizeBatch, mi355cv_warpAffineBatch, mi355cv_warpPerspectiveBatch, mi355cv_cvtBGRtoGrayBatch, mi355cv_pyrdownBatch, mi355cv_buildPyramidBatch,
 * mi355cv_cornerHarrisBatch, mi355cv_integralBatch, mi355cv_matchTemplateBatch, mi355cv_demosaicBatch, mi355cv_pyrupBatch, the Gaussian entries), in groups its
 * scratch budget sets (CLAHE, connected components with CV_32S labels, distanceTransform), from a 1-D grid, or frame by frame (threshold, Sobel, box, separable and
 * 2-D filters) -- or it DECLINES with the bound in the reason and writes nothing: minMaxLoc, calcHist, calcBackProject, stereoBM, filterSpeckles, HoughLines,
 * connected components with CV_16U labels and their statistics, bfKnnMatchBatch (pairs), and a Gaussian of more than 33 taps. */
/* the same for any sigma (the Q8.8 taps cv::GaussianBlur computes for CV_8U, smooth.dispatch.cpp:658-724), device-resident frames only, kernel sizes odd and at most
 * mi355cv_limit("gauss8u_max_ksize") */
MI355CV_API int mi355cv_gaussianBlurBatch(const mi355cv_uchar* src_data, size_t src_step, size_t src_frame_stride,
        mi355cv_uchar* dst_data, size_t dst_step, size_t dst_frame_stride, int nframes, int width, int height, int depth, int cn,
        size_t ksize_width, size_t ksize_height, double sigmaX, double sigmaY, int border_type);
MI355CV_API int mi355cv_gaussianBlurBinomialBatch(const mi355cv_uchar* src_data, size_t src_step, size_t src_frame_stride,
        mi355cv_uchar* dst_data, size_t dst_step, size_t dst_frame_stride, int nframes,
        int width, int height, int depth, int cn, size_t ksize, int border_type);

/* --------------------------------------------------- a3/a4/a5: linear filters */

struct cvhalFilter2D;   /* opaque context, as in hal_replacement.hpp:87 */

/* replace hal_ni_filterInit / hal_ni_filter / hal_ni_filterFree (hal_replacement.hpp:109,125,131);
 * callers: replacementFilter2D filter.dispatch.cpp:1163-1185 (cv::filter2D).  Depths 8U/16U/16S/32F,
 * any kernel size up to 1024 taps, any anchor, borders CONSTANT(0)/REPLICATE/REFLECT/WRAP/REFLECT_101. */
MI355CV_API int mi355cv_filterInit(struct cvhalFilter2D** context, mi355cv_uchar* kernel_data, size_t kernel_step, int kernel_type,
        int kernel_width, int kernel_height, int max_width, int max_height, int src_type, int dst_type, int borderType,
        double delta, int anchor_x, int anchor_y, bool allowSubmatrix, bool allowInplace);
MI355CV_API int mi355cv_filter(struct cvhalFilter2D* context, mi355cv_uchar* src_data, size_t src_step, mi355cv_uchar* dst_data,
        size_t dst_step, int width, int height, int full_width, int full_height, int offset_x, int offset_y);
MI355CV_API int mi355cv_filterFree(struct cvhalFilter2D* context);
/* batched form over device-resident whole frames, with a context from mi355cv_filterInit */
MI355CV_API int mi355cv_filterBatch(struct cvhalFilter2D* context, const mi355cv_uchar* src_data, size_t src_step, size_t src_frame_stride,
        mi355cv_uchar* dst_data, size_t dst_step, size_t dst_frame_stride, int nframes, int width, int height);

/* cv::cvtColor(COLOR_BGR2GRAY | RGB2GRAY | BGRA2GRAY | RGBA2GRAY) (color.cpp:192 -> hal::cvtBGRtoGray, color_rgb.dispatch.cpp:269) followed by
 * cv::filter2D (filter.dispatch.cpp:1521) on device-resident CV_8UC3 / CV_8UC4 frames in one pass: the gray image is never written (SURVEY
 * section 8d: 33.2 MB per 4K frame instead of 49.8 MB).  `context` from mi355cv_filterInit for CV_8UC1 -> CV_8UC1, 3x3 or 5x5, centred anchor;
 * width a multiple of 16 pixels; NOT_IMPLEMENTED otherwise (make the two calls).  Bit-identical to the two-call sequence. */
MI355CV_API int mi355cv_cvtBGRtoGrayFilterBatch(struct cvhalFilter2D* context, const mi355cv_uchar* src_data, size_t src_step, size_t src_frame_stride,
        mi355cv_uchar* dst_data, size_t dst_step, size_t dst_frame_stride, int nframes, int width, int height, int scn, bool swapBlue);

/* replace hal_ni_sepFilterInit / hal_ni_sepFilter / hal_ni_sepFilterFree (hal_replacement.hpp:155,171,177);
 * callers: replacementSepFilter filter.dispatch.cpp:1362-1383 (cv::sepFilter2D, and through it Sobel/Scharr/
 * GaussianBlur on non-8U depths). */
MI355CV_API int mi355cv_sepFilterInit(struct cvhalFilter2D** context, int src_type, int dst_type, int kernel_type,
        mi355cv_uchar* kernelx_data, int kernelx_length, mi355cv_uchar* kernely_data, int kernely_length,
        int anchor_x, int anchor_y, double delta, int borderType);
MI355CV_API int mi355cv_sepFilter(struct cvhalFilter2D* context, mi355cv_uchar* src_data, size_t src_step, mi355cv_uchar* dst_data,
        size_t dst_step, int width, int height, int full_width, int full_height, int offset_x, int offset_y);
MI355CV_API int mi355cv_sepFilterFree(struct cvhalFilter2D* context);
/* what mi355cv_sepFilterInit decided (no reference counterpart; needs no device): info[8] = {mode (0 float, 1 CV_8U bit-exact x 2^8, 2 integer CV_8U -> CV_16S), symY,
 * nx, ny, anchor x, anchor y, delta as the integer modes add it, 1 if the destination is CV_64F}; kx / ky (room for mi355cv_limit("sep_max_taps") words each) receive
 * the taps as the kernels read them: float bits in mode 0, int32 otherwise.  tests/test_hostemu.py replays the LDS-ring kernel on the CPU with these. */
MI355CV_API int mi355cv_sepFilterDescribe(struct cvhalFilter2D* context, int* info, float* deltaF, unsigned* kx, unsigned* ky);

/* replaces hal_ni_sobel (hal_replacement.hpp:1197; caller deriv.cpp:456) and hal_ni_scharr (:1224; caller deriv.cpp:511) */
MI355CV_API int mi355cv_sobel(const mi355cv_uchar* src_data, size_t src_step, mi355cv_uchar* dst_data, size_t dst_step,
        int width, int height, int src_depth, int dst_depth, int cn, int margin_left, int margin_top, int margin_right,
        int margin_bottom, int dx, int dy, int ksize, double scale, double delta, int border_type);
MI355CV_API int mi355cv_scharr(const mi355cv_uchar* src_data, size_t src_step, mi355cv_uchar* dst_data, size_t dst_step,
        int width, int height, int src_depth, int dst_depth, int cn, int margin_left, int margin_top, int margin_right,
        int margin_bottom, int dx, int dy, double scale, double delta, int border_type);

/* replaces hal_ni_boxFilter (hal_replacement.hpp:1105; caller box_filter.dispatch.cpp:474) */
MI355CV_API int mi355cv_boxFilter(const mi355cv_uchar* src_data, size_t src_step, mi355cv_uchar* dst_data, size_t dst_step,
        int width, int height, int src_depth, int dst_depth, int cn, int margin_left, int margin_top, int margin_right,
        int margin_bottom, size_t ksize_width, size_t ksize_height, int anchor_x, int anchor_y, bool normalize, int border_type);

/* --------------------------------------------------- a6: colour conversion */

/* replaces hal_ni_cvtBGRtoGray (hal_replacement.hpp:442); caller hal::cvtBGRtoGray color_rgb.dispatch.cpp:276.
 * depth 8U / 16U / 32F, scn 3|4.  8U/16U bit-exact (RGB2Gray<uchar> color_rgb.simd.hpp:660), 32F = the FMA chain
 * of RGB2Gray<float> :608. */
MI355CV_API int mi355cv_cvtBGRtoGray(const mi355cv_uchar* src_data, size_t src_step, mi355cv_uchar* dst_data, size_t dst_step,
        int width, int height, int depth, int scn, bool swapBlue);
/* replaces hal_ni_cvtGraytoBGR (hal_replacement.hpp:456) */
MI355CV_API int mi355cv_cvtGraytoBGR(const mi355cv_uchar* src_data, size_t src_step, mi355cv_uchar* dst_data, size_t dst_step,
        int width, int height, int depth, int dcn);
/* replaces hal_ni_cvtBGRtoBGR (hal_replacement.hpp:395): reorder / add / drop alpha */
MI355CV_API int mi355cv_cvtBGRtoBGR(const mi355cv_uchar* src_data, size_t src_step, mi355cv_uchar* dst_data, size_t dst_step,
        int width, int height, int depth, int scn, int dcn, bool swapBlue);
/* batched BGR->gray over device-resident frames (grid-z = frame) */
MI355CV_API int mi355cv_cvtBGRtoGrayBatch(const mi355cv_uchar* src_data, size_t src_step, size_t src_frame_stride,
        mi355cv_uchar* dst_data, size_t dst_step, size_t dst_frame_stride, int nframes,
        int width, int height, int depth, int scn, int swapBlue);

/* --------------------------------------------------- a7/a8/a9: geometric transforms */

/* replaces hal_ni_resize (hal_replacement.hpp:257; caller hal::resize resize.cpp:3840).  INTER_NEAREST, INTER_LINEAR
 * (8U fixed point bit-exact; 16U/16S/32F float), INTER_AREA for integer ratios (resizeAreaFast_) and for upscaling. */
MI355CV_API int mi355cv_resize(int src_type, const mi355cv_uchar* src_data, size_t src_step, int src_width, int src_height,
        mi355cv_uchar* dst_data, size_t dst_step, int dst_width, int dst_height, double inv_scale_x, double inv_scale_y,
        int interpolation);
/* replaces hal_ni_warpAffine (hal_replacement.hpp:275; caller imgwarp.cpp:2678).  M maps dst -> src (already inverted) */
MI355CV_API int mi355cv_warpAffine(int src_type, const mi355cv_uchar* src_data, size_t src_step, int src_width, int src_height,
        mi355cv_uchar* dst_data, size_t dst_step, int dst_width, int dst_height, const double M[6], int interpolation,
        int borderType, const double borderValue[4]);
/* replaces hal_ni_warpPerspective (hal_replacement.hpp:316; caller imgwarp.cpp:3290) */
MI355CV_API int mi355cv_warpPerspective(int src_type, const mi355cv_uchar* src_data, size_t src_step, int src_width, int src_height,
        mi355cv_uchar* dst_data, size_t dst_step, int dst_width, int dst_height, const double M[9], int interpolation,
        int borderType, const double borderValue[4]);
/* replaces hal_ni_remap32f (hal_replacement.hpp:371; caller imgwarp.cpp:1820) */
MI355CV_API int mi355cv_remap32f(int src_type, const mi355cv_uchar* src_data, size_t src_step, int src_width, int src_height,
        mi355cv_uchar* dst_data, size_t dst_step, int dst_width, int dst_height, float* mapx, size_t mapx_step,
        float* mapy, size_t mapy_step, int interpolation, int border_type, const double border_value[4]);
/* cv::remap for every map representation it accepts (imgwarp.cpp:1718-1921; the HAL only has remap32f): (CV_32FC1, CV_32FC1), CV_32FC2, the
 * fixed-point form of cv::convertMaps -- CV_16SC2 + CV_16UC1 / CV_16SC1 (bilinear, nearest), CV_16SC2 alone (nearest).  map*_type: cv type codes. */
MI355CV_API int mi355cv_remap(int src_type, const mi355cv_uchar* src_data, size_t src_step, int src_width, int src_height,
        mi355cv_uchar* dst_data, size_t dst_step, int dst_width, int dst_height, const void* map1, size_t map1_step, int map1_type,
        const void* map2, size_t map2_step, int map2_type, int interpolation, int border_type, const double border_value[4]);
/* cv::convertMaps (imgwarp.cpp:1925): float maps <-> CV_16SC2 (+ CV_16UC1), bit-exact with the reference's rounding */
MI355CV_API int mi355cv_convertMaps(const void* map1, size_t map1_step, int map1_type, const void* map2, size_t map2_step, int map2_type,
        void* dstmap1, size_t dstmap1_step, int dstmap1_type, void* dstmap2, size_t dstmap2_step, int width, int height, int nninterpolate);
/* cv::warpPolar (imgwarp.cpp:3731-3845), both directions: the map is evaluated inside the sampling kernel -- forward from the per-row cos / sin and
 * per-column radii, WARP_INVERSE_MAP from the reference's float approximations of cartToPolar and log (source with one wrapped row above and below) */
MI355CV_API int mi355cv_warpPolar(int src_type, const mi355cv_uchar* src_data, size_t src_step, int src_width, int src_height,
        mi355cv_uchar* dst_data, size_t dst_step, int dst_width, int dst_height, float center_x, float center_y, double maxRadius, int flags);

/* --------------------------------------------------- a10/a11/a12: corners and pyramids */

/* replace hal_ni_pyrdown (hal_replacement.hpp:1244) and hal_ni_pyrdown_offset (:1268); caller cv::pyrDown pyramids.cpp:1371,1377.
 * depth 8U/16U/16S/32F, cn 1..4, every border cv::pyrDown accepts. */
MI355CV_API int mi355cv_pyrdown(const mi355cv_uchar* src_data, size_t src_step, int src_width, int src_height,
        mi355cv_uchar* dst_data, size_t dst_step, int dst_width, int dst_height, int depth, int cn, int border_type);
MI355CV_API int mi355cv_pyrdown_offset(const mi355cv_uchar* src_data, size_t src_step, int src_width, int src_height,
        mi355cv_uchar* dst_data, size_t dst_step, int dst_width, int dst_height, int depth, int cn,
        int margin_left, int margin_top, int margin_right, int margin_bottom, int border_type);
MI355CV_API int mi355cv_pyrdownBatch(const mi355cv_uchar* src_data, size_t src_step, size_t src_frame_stride, int src_width, int src_height,
        mi355cv_uchar* dst_data, size_t dst_step, size_t dst_frame_stride, int dst_width, int dst_height, int nframes,
        int depth, int cn, int border_type);
/* cv::pyrUp (pyramids.cpp, pyrUp_<CastOp>) has no HAL hook (csrc/pyrup.hip): depth 8U/16U/16S/32F, cn 1..4, dst = (2 * src_width) x (2 * src_height),
 * border_type BORDER_DEFAULT (the only one the reference accepts; the ISOLATED bit is ignored).  Integer depths bit-identical to the reference.  Everything
 * else -- CV_64F, the 2w +- 1 / 2h +- 1 sizes the reference also admits, source and destination that overlap in HBM, a source wider than 2^27 pixels or
 * taller than 2^29 rows (the kernels index a destination row and count destination rows in int) -- is answered MI355CV_NOT_IMPLEMENTED.
 * Both images in HBM, or both in host memory (staged under the host policy, cost class HOST_CHEAP). */
MI355CV_API int mi355cv_pyrup(const mi355cv_uchar* src_data, size_t src_step, int src_width, int src_height,
        mi355cv_uchar* dst_data, size_t dst_step, int dst_width, int dst_height, int depth, int cn, int border_type);
/* `nframes` frames of one geometry, `*_frame_stride` bytes apart, one launch; all in HBM, or all in host memory (the pipelined path) */
MI355CV_API int mi355cv_pyrupBatch(const mi355cv_uchar* src_data, size_t src_step, size_t src_frame_stride, int src_width, int src_height,
        mi355cv_uchar* dst_data, size_t dst_step, size_t dst_frame_stride, int dst_width, int dst_height, int nframes,
        int depth, int cn, int border_type);
/* cv::demosaicing / the Bayer codes of cv::cvtColor (demosaicing.cpp, Bayer2RGB_ / Bayer2Gray_) have no HAL hook (csrc/demosaic.hip): bilinear interpolation only.
 * src: one channel of CV_8U or CV_16U (depth 0 or 2), width x height; dst: dcn = 3 (B G R), 4 (B G R alpha, alpha = 255 / 65535) or 1 (gray, the reference's own
 * weights on the unrounded sums) channels of the same depth and size.  pattern 0..3 = BG, GB, RG, GR (COLOR_BayerBG2BGR .. COLOR_BayerGR2BGR), taken relative to
 * the pointer handed in, like a cv::Mat submatrix; for R G B order pass the pattern with red and blue exchanged (BG <-> RG, GB <-> GR).  Bit-identical to the
 * reference's definition restated in csrc/demosaic_math.h.  Declined (MI355CV_NOT_IMPLEMENTED, before any device is touched): null pointers, other depths, dcn or
 * patterns, width or height below 3 or above mi355cv_limit("demosaic_max_dim") = 16384, a pitch below the row, a pointer / pitch / frame stride that is no multiple
 * of the element size, nframes < 1; source and destination that overlap in HBM.  Both images in HBM, or both in host memory (staged under the host policy, cost
 * class HOST_CHEAP). */
MI355CV_API int mi355cv_demosaic(const mi355cv_uchar* src, size_t src_step, mi355cv_uchar* dst, size_t dst_step,
        int width, int height, int depth, int dcn, int pattern);
/* `nframes` frames of one geometry, `*_frame_stride` bytes apart, one launch; all in HBM, or all in host memory (the pipelined path) */
MI355CV_API int mi355cv_demosaicBatch(const mi355cv_uchar* src, size_t src_step, size_t src_frame_stride,
        mi355cv_uchar* dst, size_t dst_step, size_t dst_frame_stride, int width, int height, int nframes, int depth, int dcn, int pattern);
/* cv::distanceTransform (distransform.cpp) has no HAL hook (csrc/disttransform.hip).  src CV_8UC1, a pixel is a site iff it is 0; dst has the source's size.
 * Served: distance_type DIST_L2 (2) with mask_size DIST_MASK_PRECISE (0) -- the exact integer squared distance to the nearest site, square-rooted and correctly
 * rounded to float, dst_depth MI355CV_32F; DIST_L1 (1) and DIST_C (3) with mask_size 0, 3 or 5 (one result: the exact city-block / chessboard distance, which is what
 * the reference's 3 x 3 chamfer pass computes), dst_depth MI355CV_32F, or MI355CV_8U saturated at 255 for DIST_L1.  L2-precise equals the reference wherever its
 * float32 parabola envelope is exact; where that misrounds (frames a few thousand pixels wide) this returns the mathematically exact value.
 * A frame WITHOUT ANY SITE has no defined distance: every pixel of it is 31622776.0f (CV_32F) or 255 (CV_8U) and the call returns OK; parity with the reference,
 * which returns an implementation-specific large number there, is not claimed on such frames.
 * Answered MI355CV_NOT_IMPLEMENTED with the destination untouched: DIST_L2 with mask_size 3 or 5 (the chamfer approximations, raster-sequential), any other
 * distance type or mask size, the labelled variant (no entry point), CV_8U output without DIST_L1, other destination depths, source and destination that overlap in
 * HBM, width or height above mi355cv_limit("disttransform_max_dim") = 16384 (16-bit column distances and 32-bit squared distances in the kernels).
 * Both images in HBM, or both in host memory (staged under the host policy, cost class HOST_HEAVY). */
MI355CV_API int mi355cv_distanceTransform(const mi355cv_uchar* src_data, size_t src_step, int width, int height, mi355cv_uchar* dst_data, size_t dst_step,
        int distance_type, int mask_size, int dst_depth);
/* `nframes` frames of one geometry, `*_frame_stride` bytes apart; all in HBM, or all in host memory (the pipelined path).  A frame without a site gets the
 * value above; the other frames of the batch are unaffected. */
MI355CV_API int mi355cv_distanceTransformBatch(const mi355cv_uchar* src_data, size_t src_step, size_t src_frame_stride, int width, int height,
        mi355cv_uchar* dst_data, size_t dst_step, size_t dst_frame_stride, int nframes, int distance_type, int mask_size, int dst_depth);
/* cv::connectedComponents / cv::connectedComponentsWithStats (connectedcomponents.cpp) have no HAL hook (csrc/ccl.hip).  src CV_8UC1, a pixel is foreground iff
 * it is non-zero; connectivity 4 or 8; ltype MI355CV_32S or MI355CV_16U; labels has the source's size.  Labels run 0 .. N - 1 with 0 for the background, and
 * *nlabels = N is written to HOST memory (the call's one host synchronisation); N counts the background even when no pixel is background.  Every result is a pure
 * function of the input: the union-find keeps the smallest pixel index as the root, so nothing depends on the order in which merges land.
 * Numbering follows one of two orders.  PIXEL ORDER: components are numbered 1, 2, ... by the raster position of their first pixel (the smallest y * w + x) --
 * every ccltype with connectivity 4, and CCL_WU (0) / CCL_SAUF (3) with connectivity 8.  BLOCK ORDER: by the raster position of their first 2 x 2 block (the
 * smallest (y >> 1) * ceil(w / 2) + (x >> 1); two foreground pixels of one block are 8-connected, so the key is unique) -- connectivity 8 with CCL_DEFAULT (-1),
 * CCL_GRANA (1) / CCL_BBDT (4) and CCL_BOLELLI (2) / CCL_SPAGHETTI (5).  Both orders follow from where the reference's labellers create provisional labels: SAUF at
 * a component's first raster pixel, with set_union keeping the smaller root and flattenL renumbering roots in increasing order; the block-based ones per 2 x 2
 * block in raster order of blocks.  The reference was not available to pin either order; the tests hold them against a restatement and scipy.ndimage.label.
 * Answered MI355CV_NOT_IMPLEMENTED with every destination untouched: another ltype, connectivity other than 4 or 8, ccltype outside -1 .. 5, null pointers,
 * width or height <= 0 or above mi355cv_limit("ccl_max_dim") = 16384 (32-bit pixel indices and areas, coordinate sums below 2^53), source and labels that overlap
 * in HBM, and MI355CV_16U labels when N - 1 > 65535 (the reference's label type would wrap; labelling runs in 32-bit scratch and the decision is taken before the
 * destination is written).  Both images in HBM, or both in host memory (staged under the host policy, cost class HOST_HEAVY). */
MI355CV_API int mi355cv_connectedComponents(const mi355cv_uchar* src_data, size_t src_step, int width, int height, mi355cv_uchar* labels_data, size_t labels_step,
        int connectivity, int ltype, int ccltype, int* nlabels);
/* `nframes` frames of one geometry, `*_frame_stride` bytes apart; all in HBM, or all in host memory (the pipelined path).  nlabels: `nframes` ints in HOST memory,
 * one copy for all frames.  With MI355CV_16U one frame with more than 65535 components declines the whole call (at most 65535 frames then); in the pipelined host
 * path the chunks of frames already copied back stay written. */
MI355CV_API int mi355cv_connectedComponentsBatch(const mi355cv_uchar* src_data, size_t src_step, size_t src_frame_stride, int width, int height,
        mi355cv_uchar* labels_data, size_t labels_step, size_t labels_frame_stride, int nframes, int connectivity, int ltype, int ccltype, int* nlabels);
/* The statistics of a finished label image (ltype MI355CV_32S or MI355CV_16U): stats is nlabels rows of five CV_32S, CC_STAT_LEFT, TOP, WIDTH, HEIGHT, AREA = 0 .. 4,
 * row 0 the background's; centroids (may be null) is nlabels rows of two CV_64F, double(sum of x) / double(area) and double(sum of y) / double(area), the sums exact
 * 64-bit integers and the division the correctly rounded IEEE one.  A label without a pixel (label 0 of a frame without background) gets the library's own value:
 * the five stats 0 and the centroid (NaN, NaN); the call returns OK and parity with the reference is not claimed for that row.  A value >= nlabels in the label
 * image is skipped and never indexed.  The outputs live where the label image lives: all three on the device, or all on the host (staged).  Declined: null labels or
 * stats, another ltype, nlabels < 1, the size bounds above, outputs and labels that overlap in HBM. */
MI355CV_API int mi355cv_connectedComponentsStats(const mi355cv_uchar* labels_data, size_t labels_step, int width, int height, int ltype, int nlabels,
        int* stats, size_t stats_step, double* centroids, size_t centroids_step);
/* Device-resident frames only (host-resident ones are declined).  nlabels: `nframes` ints in HOST memory; frame f's rows from nlabels[f] up to max_labels are
 * zero-filled; any nlabels[f] > max_labels, or nframes > 65535, is declined. */
MI355CV_API int mi355cv_connectedComponentsStatsBatch(const mi355cv_uchar* labels_data, size_t labels_step, size_t labels_frame_stride, int width, int height, int ltype,
        int nframes, const int* nlabels, int max_labels, int* stats, size_t stats_step, size_t stats_frame_stride,
        double* centroids, size_t centroids_step, size_t centroids_frame_stride);
/* cv::HoughLines / cv::HoughLinesWithAccumulator, the standard transform (HoughLinesStandard, hough.cpp), have no HAL hook (csrc/hough.hip).  src CV_8UC1, a
 * pixel votes iff it is non-zero.  rho and theta arrive as doubles and are used as float; "float" below is IEEE binary32 with every operation rounded on its own
 * (no fused multiply-add), cvRound is round-half-to-even.
 *   geometry  numangle = floor((max_theta - min_theta) / theta) + 1 in double, one fewer when numangle > 1 and |CV_PI - (numangle - 1) theta| < theta / 2;
 *             numrho = cvRound(float(2 (width + height) + 1) / rho_f); irho = 1.f / rho_f.
 *   table     ang = (float)min_theta; tabSin[n] = (float)(sin((double)ang) * irho), tabCos[n] likewise (libm on the host, the product in double); ang += theta_f.
 *   votes     every non-zero pixel (x, y) and every n: r = cvRound(x * tabCos[n] + y * tabSin[n]) + (numrho - 1) / 2, cell (n + 1)(numrho + 2) + r + 1 of the
 *             (numangle + 2) x (numrho + 2) CV_32S accumulator gains 1.
 *   maxima    inner cell b is one iff a[b] > threshold, a[b] > a[b - 1], a[b] >= a[b + 1], a[b] > a[b - numrho - 2], a[b] >= a[b + numrho + 2].
 *   order     votes descending, equal votes by b ascending.
 *   lines     rho = (r - (numrho - 1) * 0.5f) * rho_f, theta = (float)min_theta + n * theta_f; lines_cn = 2 floats per line, or 3 with (float)votes.
 * The accumulator is integer and the order is total, so every result is a pure function of the input.  The reference was not available to pin these steps; the
 * tests hold the kernels bit for bit against two independent Python restatements of them (tests/hough_restate.py).
 * lines: max_lines rows of lines_cn floats, dense.  *nlines (HOST memory; reading it back is the call's one host synchronisation) receives the TOTAL number of
 * maxima; only the first min(*nlines, max_lines) rows are written, rows past the count never are.
 * Answered MI355CV_NOT_IMPLEMENTED with every destination untouched: srn != 0 or stn != 0 (the multi-scale variant), rho <= 0 or theta <= 0, angles outside
 * 0 <= min_theta < max_theta <= CV_PI, null pointers, lines_cn other than 2 or 3, max_lines < 1, width or height <= 0 or above mi355cv_limit("hough_max_dim") =
 * 16384 (a packed point (y << 16 | x) needs both <= 65535; 16384 is the bound of the neighbouring entries and keeps a frame's point list within 1 GiB and every
 * count below 2^28), an accumulator above mi355cv_limit("hough_max_accum") = 2^26 cells (256 MiB per frame; a cell index is the low word of the sort key), more than 65535 angles, and
 * lines that overlap the source in HBM.  Image and lines both in HBM, or both in host memory (staged under the host policy, cost class HOST_HEAVY; the lines then
 * come back in a second copy after the counts).  cv::HoughCircles: mi355cv_houghCircles below.  cv::HoughLinesP and cv::HoughLinesPointSet have no entry. */
MI355CV_API int mi355cv_houghLines(const mi355cv_uchar* src_data, size_t src_step, int width, int height, float* lines, int lines_cn, int max_lines,
        double rho, double theta, int threshold, double srn, double stn, double min_theta, double max_theta, int* nlines);
/* `nframes` frames of one geometry, `src_frame_stride` / `lines_frame_stride` bytes apart (the latter a multiple of 4 and at least max_lines rows); all in HBM,
 * or all in host memory.  One enqueue for all frames; nlines: `nframes` ints in HOST memory.  A frame without an edge pixel yields 0 lines and does not affect the
 * others.  At most 65535 frames. */
MI355CV_API int mi355cv_houghLinesBatch(const mi355cv_uchar* src_data, size_t src_step, size_t src_frame_stride, int width, int height, float* lines, int lines_cn,
        int max_lines, size_t lines_frame_stride, int nframes, double rho, double theta, int threshold, double srn, double stn, double min_theta, double max_theta,
        int* nlines);
/* The geometry, and the accumulator itself: *numangle and *numrho (HOST memory) always; with accum != NULL the full (numangle + 2) x (numrho + 2) CV_32S
 * accumulator of the frame, rows accum_step bytes apart (a multiple of 4, at least numrho + 2 ints), where the image lives.  With accum == NULL no device is
 * touched and src is only tested for NULL.  The same refusals as mi355cv_houghLines. */
MI355CV_API int mi355cv_houghLinesAccum(const mi355cv_uchar* src_data, size_t src_step, int width, int height, double rho, double theta, double min_theta,
        double max_theta, int* accum, size_t accum_step, int* numangle, int* numrho);
/* cv::HoughCircles with method HOUGH_GRADIENT (= 3; HoughCirclesGradient, hough.cpp) has no HAL hook (csrc/houghcircles.hip).  src CV_8UC1.  "float" below is IEEE
 * binary32 with every operation rounded on its own (no fused multiply-add), sqrtf and / correctly rounded, cvRound round-half-to-even; SHIFT = 10, ONE = 1024.
 *   arguments  dp = max((float)dp, 1.f), idp = 1.f / dp; canny = cvRound(param1), accT = cvRound(param2); minRadius = max(0, minRadius); centres only when
 *              maxRadius < 0; maxRadius <= 0 becomes max(width, height), otherwise maxRadius <= minRadius becomes minRadius + 2.
 *   edges      dx, dy = Sobel 3 x 3 into CV_16S, BORDER_REPLICATE (mi355cv_sobel); edges = the stages of mi355cv_canny on them with low = max(1, canny / 2),
 *              high = canny, L1 magnitude.  Both stay in HBM.
 *   accum      acols = ceil(width * idp), arows = ceil(height * idp) (the product in float); (arows + 2) x (acols + 2) CV_32S, row stride astep = acols + 2, zeroed.
 *   votes      every pixel (x, y) with edges != 0, (vx, vy) != (0, 0) and mag = sqrtf((float)(vx vx + vy vy)) >= 1 is a point.  sx = cvRound((vx * idp) * ONE / mag),
 *              sy likewise; x0 = cvRound((x * idp) * ONE), y0 likewise.  For both signs of (sx, sy) and r = minRadius .. maxRadius: x2 = (x0 + r sx) >> SHIFT,
 *              y2 = (y0 + r sy) >> SHIFT; the ray ends at the first r with x2 outside [0, acols) or y2 outside [0, arows), otherwise cell y2 * astep + x2 gains 1.
 *   centres    cells b = y * astep + x, y in 1 .. arows, x in 1 .. acols, with a[b] > accT, a[b] > a[b - 1], a[b] >= a[b + 1], a[b] > a[b - astep],
 *              a[b] >= a[b + astep]; ordered by a[b] descending, equal votes by b ascending; cx = (x + 0.5f) * dp, cy = (y + 0.5f) * dp.
 *   radius     nBins = cvRound((maxRadius - minRadius) / dp * 10).  Every point with (float)minRadius^2 <= r2 <= (float)maxRadius^2, r2 = ex ex + ey ey,
 *              ex = cx - px, ey = cy - py, adds 1 to bin clamp(cvRound((sqrtf(r2) - minRadius) / dp * 10), 0, nBins - 1).  The scan: maxCount = 0, rBest = 0;
 *              for (j = nBins - 1; j > 0; j--) if (bins[j]) { upbin = j; cur = 0; for (; j > upbin - 10 && j >= 0; j--) cur += bins[j];
 *              rCur = (upbin + j) / 2.f / 10 * dp + minRadius; if (cur * rBest >= maxCount * rCur || (rBest < FLT_EPSILON && cur >= maxCount))
 *              { rBest = rCur; maxCount = cur; } } -- the outer j-- after a window included.  The circle (cx, cy, rBest) with votes = maxCount is kept when
 *              maxCount > accT.  Centres only: every centre is a circle (cx, cy, 0) with votes = a[b].
 *   order      votes descending, equal votes by b ascending.
 *   suppress   the circles are walked in that order; one is kept unless a circle kept before it has ddx ddx + ddy ddy < minDist * minDist (in float); the walk
 *              stops after max_circles kept circles.
 * Every count is an integer and every float is computed per element, so the result is a pure function of the input.  The reference was not available to pin these
 * steps: they are this project's restatement of the rule, held bit for bit against two independent Python restatements (tests/houghcircles_restate.py).
 * circles: max_circles rows of circles_cn floats, dense: (x, y, radius), or with circles_cn = 4 (x, y, radius, (float)votes).  *ncircles (HOST memory; reading it
 * back is the call's one host synchronisation of its own -- the hysteresis of the edge stage has its own) receives the number of rows written; a count equal to
 * max_circles means there may be more.  Rows past the count are never written.
 * Answered MI355CV_NOT_IMPLEMENTED with every destination and count untouched, before any device is touched: a method other than HOUGH_GRADIENT (HOUGH_GRADIENT_ALT
 * = 4 among them), dp, minDist, cvRound(param1) or cvRound(param2) not positive or NaN, circles_cn other than 3 or 4, max_circles < 1 or above
 * mi355cv_limit("houghcircles_max_circles") = 65536, null pointers, width or height <= 0 or above mi355cv_limit("houghcircles_max_dim") = 16384 (a packed point
 * (y << 16 | x), counts below 2^28), (arows + 2)(acols + 2) above mi355cv_limit("houghcircles_max_accum") = 2^26 cells (a cell index is the low word of the sort
 * key), a prepared maxRadius above mi355cv_limit("houghcircles_max_radius") = 32768 (x0 + r sx stays inside 31 bits), nBins < 1, steps below a row; and, needing
 * the device, circles that overlap the source in HBM.  Image and circles both in HBM, or both in host memory (staged under the host policy, cost class HOST_HEAVY;
 * the circles then come back in a second copy after the counts).  mi355cv_limit("houghcircles_lds_bins") = 40960: radius histograms up to that many bins are kept
 * in LDS, longer ones in HBM with the same arithmetic. */
MI355CV_API int mi355cv_houghCircles(const mi355cv_uchar* src_data, size_t src_step, int width, int height, float* circles, int circles_cn, int max_circles, int method,
        double dp, double minDist, double param1, double param2, int minRadius, int maxRadius, int* ncircles);
/* `nframes` frames of one geometry, `src_frame_stride` / `circles_frame_stride` bytes apart (the former at least a frame, the latter a multiple of 4 and at least
 * max_circles rows); all in HBM, or all in host memory.  The hysteresis of the edge stage keeps its own host round-trips per frame; everything after it is one
 * sequence of launches for all frames, and the counts come back in one copy.  ncircles: `nframes` ints in HOST memory.  A frame without an edge pixel yields 0
 * circles and does not affect the others.  At most 65535 frames. */
MI355CV_API int mi355cv_houghCirclesBatch(const mi355cv_uchar* src_data, size_t src_step, size_t src_frame_stride, int width, int height, float* circles, int circles_cn,
        int max_circles, size_t circles_frame_stride, int nframes, int method, double dp, double minDist, double param1, double param2, int minRadius, int maxRadius,
        int* ncircles);
/* The transform from a given edge map (CV_8UC1, non-zero = edge, rows edges_step bytes apart) and its CV_16SC1 gradient planes (rows grad_step bytes apart, an even
 * number, both planes at even addresses): steps `votes` to `suppress` above; mi355cv_houghCircles is this entry after its edge stage.  An edge pixel whose gradient
 * is (0, 0) does not vote and is no point.  param1 is checked as above and otherwise unused.  All four buffers in HBM, or all in host memory. */
MI355CV_API int mi355cv_houghCirclesGradient(const mi355cv_uchar* edges, size_t edges_step, const short* dx, const short* dy, size_t grad_step, int width, int height,
        float* circles, int circles_cn, int max_circles, int method, double dp, double minDist, double param1, double param2, int minRadius, int maxRadius, int* ncircles);
/* The geometry, and the accumulator itself: *arows and *acols (HOST memory) always; with accum != NULL the full (arows + 2) x (acols + 2) CV_32S accumulator after
 * step `votes`, rows accum_step bytes apart (a multiple of 4, at least acols + 2 ints), where the planes live.  With accum == NULL no device is touched and the planes
 * are only tested for NULL.  The same refusals as mi355cv_houghCirclesGradient, as far as its arguments go. */
MI355CV_API int mi355cv_houghCirclesAccum(const mi355cv_uchar* edges, size_t edges_step, const short* dx, const short* dy, size_t grad_step, int width, int height,
        double dp, int minRadius, int maxRadius, int* accum, size_t accum_step, int* arows, int* acols);
/* A/B switch of the vote: -1 (the default) the library chooses, 0 k_hc_vote (integer atomicAdd into the accumulator in HBM; serves every parameter set),
 * 1 k_hc_vote_tile (a workgroup owns a tile of mi355cv_limit("houghcircles_tile")^2 cells in LDS and writes it with plain stores).  Both give the identical
 * accumulator.  The tile kernel was the slower one at every reach measured, so the library always chooses k_hc_vote.  Returns 0, or -1 for another
 * value. */
MI355CV_API int mi355cv_houghCirclesSetKernel(int mode);
/* cv::minMaxLoc (csrc/minmax.hip).  src: one channel of CV_8U, CV_8S, CV_16U, CV_16S, CV_32S, CV_32F or CV_64F (depth 0 .. 6), its base aligned to the element
 * only (a ROI that starts at an odd column is served).  mask: NULL, or CV_8UC1 of the same size with its own pitch; non-zero selects a pixel.
 *   candidates   the selected pixels whose value is not NaN.
 *   vals[0]      the least candidate value, vals[1] the greatest, as (double)element; -0.0 and +0.0 compare equal and the sign of a returned zero is unspecified;
 *                +-inf are ordinary values.
 *   locs         {minX, minY, maxX, maxY}: for both, the FIRST pixel in raster order (y, then x) that holds the value.
 *   empty set    (mask all zero, every pixel NaN, or both) vals = {0, 0}, locs = {-1, -1, -1, -1}.
 * The reference was not available to pin the treatment of NaN, of infinities and of the empty set: it is this restatement's (tests/minmax_restate.py), and the
 * kernels are held against it bit for bit.  No core-HAL binding (cv_hal_minMaxIdx) is made: its parameter list could not be checked.
 * src and mask both in HBM, or both in host memory (staged under the host policy, cost class HOST_CHEAP).  vals (2 doubles) and locs (4 ints) both in HBM -- the
 * last kernel writes them and the call adds no host synchronisation of its own -- or both in host memory, which costs the call's one read-back.
 * Answered MI355CV_NOT_IMPLEMENTED with vals and locs untouched: null src, vals or locs; a depth outside the seven; width or height <= 0 or above
 * mi355cv_limit("minmax_max_dim") = 16384 (the bound of the neighbouring entries; a pixel index stays below 2^28); a pitch smaller than the row; a source pointer,
 * pitch or frame stride that is no multiple of the element size; results that overlap the source or the mask in HBM; vals and locs in different kinds of memory. */
MI355CV_API int mi355cv_minMaxLoc(const mi355cv_uchar* src_data, size_t src_step, int width, int height, int depth, const mi355cv_uchar* mask_data, size_t mask_step,
        double* vals, int* locs);
/* `nframes` frames of one geometry, `src_frame_stride` bytes apart; mask_frame_stride 0: one mask for all frames.  vals: 2 doubles per frame, locs: 4 ints per
 * frame, dense.  One enqueue of two launches whatever nframes is (frames in host memory are staged in groups of at most 1 GiB).  A frame with an empty candidate
 * set does not affect the others.  1 <= nframes <= 65535. */
MI355CV_API int mi355cv_minMaxLocBatch(const mi355cv_uchar* src_data, size_t src_step, size_t src_frame_stride, int width, int height, int depth,
        const mi355cv_uchar* mask_data, size_t mask_step, size_t mask_frame_stride, int nframes, double* vals, int* locs);
/* cv::calcHist (csrc/calchist.hip).  src: ONE interleaved image of cn = 1 .. 4 channels, depth CV_8U (0), CV_16U (2) or CV_32F (5), its base aligned to the element
 * only.  dims = 1 .. 3; channels[d] in [0, cn), repeats and any order allowed; histSize[d] = n_d >= 1.  ranges: 2 * dims floats (lo_d, hi_d) when uniform, otherwise
 * the concatenated n_d + 1 strictly ascending boundaries of each dimension (CV_8U and CV_16U only).  mask: NULL, or CV_8UC1 with its own pitch; non-zero selects.
 *   uniform      a = n / ((double)hi - (double)lo), b = -a * lo, t = v * a + b with the product and the sum rounded separately (no fused multiply-add).
 *                CV_8U / CV_16U: v is counted iff lo <= v < hi, bin = min(max(floor(t), 0), n - 1).  CV_32F: counted iff 0 <= t < n (NaN, +-inf never), bin = floor(t).
 *   non-uniform  the bin is the k with r[k] <= v < r[k + 1]; outside [r[0], r[n]) not counted.
 *   counting     a pixel is counted iff the mask selects it and every dimension counts it; it adds 1 to the dense row-major cell [b0][b1][b2].
 *   hist         nframes x prod(n_d) cells of hist_depth CV_32S (4: the exact counts) or CV_32F (5: (float)count, round to nearest even), in HBM or in host memory.
 *   accumulate   non-zero: a cell starts from its incoming value (CV_32F through cvRound, ties to even, saturated to int32); a count beyond 2^31 - 1 is unspecified.
 * The reference was not available: this is the project's restatement (tests/calchist_restate.py) and the kernels are held against it bit for bit.  No cv_hal_calcHist
 * binding is made: the hook's parameter list could not be checked.
 * src and mask both in HBM, or both in host memory (staged under the host policy, cost class HOST_CHEAP, in groups of at most 1 GiB).
 * Answered MI355CV_NOT_IMPLEMENTED with hist untouched: a null src, channels, histSize, ranges or hist; another depth; cn outside 1 .. 4; dims outside 1 .. 3; a channel
 * index outside [0, cn); n_d < 1 or > 65536, or prod(n_d) above mi355cv_limit("calchist_max_bins") = 1048576; hi <= lo, a non-finite range value, boundaries that are
 * not strictly ascending; non-uniform ranges on CV_32F; width or height <= 0 or above mi355cv_limit("calchist_max_dim") = 16384; nframes < 1 or > 65535; a pitch smaller
 * than the row or no multiple of the element size; hist_depth other than CV_32S / CV_32F; arguments on different devices; a histogram that overlaps the source or the
 * mask in HBM. */
MI355CV_API int mi355cv_calcHist(const mi355cv_uchar* src_data, size_t src_step, int width, int height, int depth, int cn, const int* channels, int dims,
        const int* histSize, const float* ranges, int uniform, const mi355cv_uchar* mask_data, size_t mask_step, void* hist, int hist_depth, int accumulate);
/* `nframes` frames of one geometry, `src_frame_stride` bytes apart, one histogram per frame, dense; mask_frame_stride 0: one mask for all frames.  A fixed number of
 * launches whatever nframes is. */
MI355CV_API int mi355cv_calcHistBatch(const mi355cv_uchar* src_data, size_t src_step, size_t src_frame_stride, int width, int height, int depth, int cn, int nframes,
        const int* channels, int dims, const int* histSize, const float* ranges, int uniform, const mi355cv_uchar* mask_data, size_t mask_step, size_t mask_frame_stride,
        void* hist, int hist_depth, int accumulate);
/* cv::calcBackProject (csrc/calchist.hip): the same bin rule on the same image kinds, no mask.  hist: dense CV_32F of shape histSize with finite values, in HBM or in
 * host memory.  dst: one channel of the source's depth, where the source lives.  A pixel that any dimension does not count gets 0; otherwise p = (double)hist[bin] * scale,
 * stored as cvRound(p) (ties to even) saturated to the type for CV_8U / CV_16U and as (float)p for CV_32F.  The refusals of mi355cv_calcHist, and: a null hist or dst; a
 * destination pitch below the row or no multiple of the element size; a destination that overlaps the source or the histogram in HBM.  dst is left untouched then. */
MI355CV_API int mi355cv_calcBackProject(const mi355cv_uchar* src_data, size_t src_step, int width, int height, int depth, int cn, const int* channels, int dims,
        const int* histSize, const float* ranges, int uniform, const float* hist, double scale, mi355cv_uchar* dst_data, size_t dst_step);
/* hist_frame_stride (bytes) 0: one histogram shared by all frames, otherwise one per frame. */
MI355CV_API int mi355cv_calcBackProjectBatch(const mi355cv_uchar* src_data, size_t src_step, size_t src_frame_stride, int width, int height, int depth, int cn, int nframes,
        const int* channels, int dims, const int* histSize, const float* ranges, int uniform, const float* hist, size_t hist_frame_stride, double scale,
        mi355cv_uchar* dst_data, size_t dst_step, size_t dst_frame_stride);
/* cv::BackgroundSubtractorMOG2 (csrc/mog2.hip; modules/video, no HAL hook).  A handle owns the per-pixel mixture model in HBM (planes of weights, variances and means,
 * allocated by the first apply on the calling thread's device); frames of `type` CV_8UC1 (0), CV_8UC3 (16), CV_32FC1 (5) or CV_32FC3 (21) in HBM or host memory, the mask
 * CV_8UC1 (0 background, shadowValue, 255 foreground) where the frame lives.  The reference was not available: the definition is the project's restatement
 * (tests/mog2_restate.py) and the kernels are held against it bit for bit.  Parameter names of Set / GetParam: "history", "nmixtures", "varThreshold", "backgroundRatio",
 * "varThresholdGen", "varInit", "varMin", "varMax", "complexityReductionThreshold", "detectShadows", "shadowValue", "shadowThreshold"; real values are kept as float.
 * apply re-initialises the model when it has seen no frame, learningRate >= 1, the size or type differ from the model's, or "nmixtures" was set since the last apply;
 * learningRate < 0: the automatic rate 1 / min(2 nframes, history).
 * Declined (MI355CV_NOT_IMPLEMENTED, the model left untouched): other types; "nmixtures" outside 1 .. mi355cv_limit("mog2_max_mixtures") = 5; history < 1; an unknown
 * parameter name; width or height < 1 or above mi355cv_limit("mog2_max_dim") = 16384; a pitch below the row; a mask that overlaps the source in HBM;
 * GetBackgroundImage / GetModel before any apply or with a geometry other than the model's. */
MI355CV_API int mi355cv_mog2Create(void** ctx, int history, double varThreshold, int detectShadows);
MI355CV_API int mi355cv_mog2Free(void* ctx);
MI355CV_API int mi355cv_mog2SetParam(void* ctx, const char* name, double v);
MI355CV_API int mi355cv_mog2GetParam(void* ctx, const char* name, double* v);
MI355CV_API int mi355cv_mog2Apply(void* ctx, const mi355cv_uchar* src, size_t src_step, mi355cv_uchar* mask, size_t mask_step, int width, int height, int type,
        double learningRate);
/* `nframes` consecutive frames of one camera in time order, one mask per frame, in ONE launch per 64 frames: the model is read and written once.  learningRate < 0: each
 * frame gets its own automatic rate; learningRate >= 1 or a changed geometry re-initialises before the first frame only.  Both ends in HBM, or both in host memory. */
MI355CV_API int mi355cv_mog2ApplyBatch(void* ctx, const mi355cv_uchar* src, size_t src_step, size_t src_frame_stride, mi355cv_uchar* mask, size_t mask_step,
        size_t mask_frame_stride, int nframes, int width, int height, int type, double learningRate);
/* the weighted mean of the modes that make up backgroundRatio of the weight, in the model's type (CV_8U: rounded to nearest even, saturated) */
MI355CV_API int mi355cv_mog2GetBackgroundImage(void* ctx, mi355cv_uchar* dst, size_t dst_step, int width, int height, int type);
/* the model in the reference's order, dense: modesUsed h x w bytes; gmm h x w x nmixtures x {weight, variance}; mean h x w x nmixtures x cn; unused slots are zero */
MI355CV_API int mi355cv_mog2GetModel(void* ctx, mi355cv_uchar* modesUsed, float* gmm, float* mean);
/* cv::calcOpticalFlowFarneback (csrc/farneback.hip; modules/video, no HAL hook): dense optical flow between two CV_8UC1 frames of width x height, the flow CV_32FC2
 * (x, y displacement per pixel), all in HBM or all in host memory (staged).  The reference was not available: the definition is the project's restatement
 * (tests/farneback_restate.py, float32 arithmetic in a fixed order) and the kernels are held against it bit for bit.  flags: OPTFLOW_USE_INITIAL_FLOW (4), then `flow`
 * holds the initial flow, and OPTFLOW_FARNEBACK_GAUSSIAN (256).  The pyramid has the levels k = 0 .. levels - 1 of scale pyr_scale^k, cut at the first k >= 1 whose
 * scaled width or height falls below 32.
 * Declined (MI355CV_NOT_IMPLEMENTED, flow left untouched): width or height < 1 or above mi355cv_limit("farneback_max_dim") = 16384; winsize < 1 or above
 * mi355cv_limit("farneback_max_winsize") = 25; poly_n < 1 or above mi355cv_limit("farneback_max_poly_n") = 7; a pyramid level whose Gaussian needs more than
 * mi355cv_limit("farneback_max_smooth_taps") = 255 taps; iterations < 0; levels < 1 or > 32; pyr_scale outside (0, 1); poly_sigma < 0; other flags;
 * OPTFLOW_USE_INITIAL_FLOW with more than one effective level; a pitch below the row; a flow pointer or pitch that is no multiple of 4; a flow that overlaps a frame
 * (or another flow) in HBM. */
MI355CV_API int mi355cv_calcOpticalFlowFarneback(const mi355cv_uchar* prev, size_t prev_step, const mi355cv_uchar* next, size_t next_step, mi355cv_uchar* flow,
        size_t flow_step, int width, int height, double pyr_scale, int levels, int winsize, int iterations, int poly_n, double poly_sigma, int flags);
/* `nframes` consecutive frames -> nframes - 1 flows, flow i from frame i to frame i + 1, each equal to the single call bit for bit; the level images and polynomial
 * expansions of every shared frame are computed once.  OPTFLOW_USE_INITIAL_FLOW is declined.  Host-resident batches are staged whole (not pipelined). */
MI355CV_API int mi355cv_calcOpticalFlowFarnebackBatch(const mi355cv_uchar* frames, size_t step, size_t frame_stride, int nframes, mi355cv_uchar* flows, size_t flow_step,
        size_t flow_frame_stride, int width, int height, double pyr_scale, int levels, int winsize, int iterations, int poly_n, double poly_sigma, int flags);
/* The stages, one kernel each, so that a mismatch can be pinned at a tiny size.  Images are CV_32F: src one float per pixel, R0 / R1 / M five (interleaved), flow two.
 * PolyExp: R (y-linear, x-linear, yy, xx, xy) of src.  UpdateMatrices: M (G11, G12, G22, h1, h2) from R0, R1 and the flow.  UpdateFlow: the flow from the window sums of
 * M (flags: 0 or OPTFLOW_FARNEBACK_GAUSSIAN); with R0, R1 and M_next all given (else all NULL), M_next is the update matrix of the new flow, as every iteration but the
 * last computes it. */
MI355CV_API int mi355cv_farnebackPolyExp(const mi355cv_uchar* src, size_t src_step, mi355cv_uchar* dst, size_t dst_step, int width, int height, int poly_n, double poly_sigma);
MI355CV_API int mi355cv_farnebackUpdateMatrices(const mi355cv_uchar* R0, size_t r0_step, const mi355cv_uchar* R1, size_t r1_step, const mi355cv_uchar* flow, size_t flow_step,
        mi355cv_uchar* M, size_t m_step, int width, int height);
MI355CV_API int mi355cv_farnebackUpdateFlow(const mi355cv_uchar* M, size_t m_step, mi355cv_uchar* flow, size_t flow_step, const mi355cv_uchar* R0, size_t r0_step,
        const mi355cv_uchar* R1, size_t r1_step, mi355cv_uchar* M_next, size_t m_next_step, int width, int height, int winsize, int flags);
/* cv::buildPyramid (pyramids.cpp:1616-1643) has no HAL hook: dst_data[i] / dst_step[i] receive level i+1. */
MI355CV_API int mi355cv_buildPyramid(const mi355cv_uchar* src_data, size_t src_step, int width, int height, int depth, int cn,
        mi355cv_uchar** dst_data, const size_t* dst_step, int maxlevel, int border_type);
/* the same over a batch of frames, all levels of all frames enqueued by one call: dst_data[l-1] / dst_step[l-1] / dst_frame_stride[l-1] describe
 * level l (frame 0's pointer, row pitch, bytes between frames) of pre-allocated arrays.  Frames and levels all in HBM, or all in host memory */
MI355CV_API int mi355cv_buildPyramidBatch(const mi355cv_uchar* src_data, size_t src_step, size_t src_frame_stride, int width, int height, int depth, int cn,
        mi355cv_uchar* const* dst_data, const size_t* dst_step, const size_t* dst_frame_stride, int maxlevel, int nframes, int border_type);

/* cv::cornerHarris (corner.cpp:634) / cv::cornerMinEigenVal (:604) have no HAL hook: fused entry points with the cv::
 * argument list.  src_type CV_8UC1 or CV_32FC1, dst CV_32FC1. */
MI355CV_API int mi355cv_cornerHarris(const mi355cv_uchar* src_data, size_t src_step, mi355cv_uchar* dst_data, size_t dst_step,
        int width, int height, int src_type, int blockSize, int ksize, double k, int borderType);
MI355CV_API int mi355cv_cornerMinEigenVal(const mi355cv_uchar* src_data, size_t src_step, mi355cv_uchar* dst_data, size_t dst_step,
        int width, int height, int src_type, int blockSize, int ksize, int borderType);
MI355CV_API int mi355cv_cornerHarrisBatch(const mi355cv_uchar* src_data, size_t src_step, size_t src_frame_stride,
        mi355cv_uchar* dst_data, size_t dst_step, size_t dst_frame_stride, int nframes, int width, int height, int src_type,
        int blockSize, int ksize, double k, int borderType);
/* cv::goodFeaturesToTrack (featureselect.cpp:382): returns the number of corners written to `corners` (x,y pairs),
 * -1 if the arguments are unsupported, -2 on a device failure.  `quality` and `mask_data` may be NULL. */
MI355CV_API int mi355cv_goodFeaturesToTrack(const mi355cv_uchar* src_data, size_t src_step, int width, int height, int src_type,
        float* corners, float* quality, int maxCorners, double qualityLevel, double minDistance,
        const mi355cv_uchar* mask_data, size_t mask_step, int blockSize, int gradientSize, int useHarrisDetector, double harrisK);

/* --------------------------------------------------- f1/f4: YUV family, CV_8U */

/* replace hal_ni_cvtBGRtoYUV (hal_replacement.hpp:500), hal_ni_cvtYUVtoBGR (:533), hal_ni_cvtTwoPlaneYUVtoBGR (:664) and
 * hal_ni_cvtTwoPlaneYUVtoBGREx (:701); callers color_yuv.dispatch.cpp:33, :86, :166, :144.  depth CV_8U only (other depths answer
 * NOT_IMPLEMENTED).  The two-plane decoders take NV12 (uIdx 0) / NV21 (uIdx 1), even dst_width and dst_height. */
MI355CV_API int mi355cv_cvtBGRtoYUV(const mi355cv_uchar* src_data, size_t src_step, mi355cv_uchar* dst_data, size_t dst_step,
        int width, int height, int depth, int scn, bool swapBlue, bool isCbCr);
MI355CV_API int mi355cv_cvtYUVtoBGR(const mi355cv_uchar* src_data, size_t src_step, mi355cv_uchar* dst_data, size_t dst_step,
        int width, int height, int depth, int dcn, bool swapBlue, bool isCbCr);
MI355CV_API int mi355cv_cvtTwoPlaneYUVtoBGR(const mi355cv_uchar* src_data, size_t src_step, mi355cv_uchar* dst_data, size_t dst_step,
        int dst_width, int dst_height, int dcn, bool swapBlue, int uIdx);
/* hal_ni_cvtBGRtoHSV (hal_replacement.hpp:596; caller color_hsv.dispatch.cpp:65): CV_8U, isHSV only (HLS and CV_32F decline) */
MI355CV_API int mi355cv_cvtBGRtoHSV(const mi355cv_uchar* src_data, size_t src_step, mi355cv_uchar* dst_data, size_t dst_step,
        int width, int height, int depth, int scn, bool swapBlue, bool isFullRange, bool isHSV);
/* hal_ni_cvtThreePlaneYUVtoBGR (hal_replacement.hpp:763): I420 / IYUV (uIdx 0) and YV12 (uIdx 1) in one array */
MI355CV_API int mi355cv_cvtThreePlaneYUVtoBGR(const mi355cv_uchar* src_data, size_t src_step, mi355cv_uchar* dst_data, size_t dst_step,
        int dst_width, int dst_height, int dcn, bool swapBlue, int uIdx);
MI355CV_API int mi355cv_cvtTwoPlaneYUVtoBGREx(const mi355cv_uchar* y_data, size_t y_step, const mi355cv_uchar* uv_data, size_t uv_step,
        mi355cv_uchar* dst_data, size_t dst_step, int dst_width, int dst_height, int dcn, bool swapBlue, int uIdx);

/* --------------------------------------------------- f1: fixed-level threshold */

/* replaces hal_ni_threshold (hal_replacement.hpp:1058; caller ThresholdRunner thresh.cpp:1365, once per row stripe).
 * thresh / maxValue as cv::threshold hands them over (already floor/round/saturated for integer depths);
 * depth CV_8U / CV_16U / CV_16S / CV_32F, thresholdType THRESH_BINARY .. THRESH_TOZERO_INV (0..4). */
MI355CV_API int mi355cv_threshold(const mi355cv_uchar* src_data, size_t src_step, mi355cv_uchar* dst_data, size_t dst_step,
        int width, int height, int depth, int cn, double thresh, double maxValue, int thresholdType);

/* replaces hal_ni_imageMoments (hal_replacement.hpp:1309; caller cv::moments moments.cpp:578): the ten spatial moments m00, m10, m01, m20, m11, m02, m30, m21,
 * m12, m03 of a single-channel CV_8U / CV_16U / CV_16S image (or of its non-zero mask, `binary`), bit-identical: exact integer tile moments on the GPU,
 * the reference's double accumulation over the tiles on the host. */
MI355CV_API int mi355cv_imageMoments(const mi355cv_uchar* src_data, size_t src_step, int src_type, int width, int height, bool binary, double m[10]);

/* replaces hal_ni_bilateralFilter (hal_replacement.hpp:1016; caller cv::bilateralFilter bilateral_filter.dispatch.cpp:418): CV_8UC1 / CV_8UC3, radius <= 16,
 * the float sums in the three forms of the reference's AVX2 build (vector body / 4-group tail / scalar rest), bit-exact.  The hook carries no margins: an
 * image with padded rows and no BORDER_ISOLATED is declined (the reference pads a submatrix with its parent's pixels). */
MI355CV_API int mi355cv_bilateralFilter(const mi355cv_uchar* src_data, size_t src_step, mi355cv_uchar* dst_data, size_t dst_step, int width, int height,
                                        int depth, int cn, int d, double sigma_color, double sigma_space, int border_type);

/* replaces hal_ni_adaptiveThreshold (hal_replacement.hpp:1038; caller cv::adaptiveThreshold thresh.cpp:1711): CV_8UC1,
 * adaptiveMethod ADAPTIVE_THRESH_MEAN_C (0) with blockSize 3..15, thresholdType THRESH_BINARY (0) / THRESH_BINARY_INV (1). */
MI355CV_API int mi355cv_adaptiveThreshold(const mi355cv_uchar* src_data, size_t src_step, mi355cv_uchar* dst_data, size_t dst_step,
        int width, int height, double maxValue, int adaptiveMethod, int thresholdType, int blockSize, double C);

/* --------------------------------------------------- f1 / f4: remaining integer colour conversions (csrc/color_misc.hip) */

/* replaces hal_ni_cvtBGRtoTwoPlaneYUV (hal_replacement.hpp:743; caller color_yuv.dispatch.cpp:238): BGR/RGB(A) CV_8U -> NV12 (uIdx 1) / NV21 (uIdx 2) */
MI355CV_API int mi355cv_cvtBGRtoTwoPlaneYUV(const mi355cv_uchar* src_data, size_t src_step, mi355cv_uchar* y_data, size_t y_step,
        mi355cv_uchar* uv_data, size_t uv_step, int width, int height, int scn, bool swapBlue, int uIdx);
/* replaces hal_ni_cvtBGRtoThreePlaneYUV (:797; caller color_yuv.dispatch.cpp:222): -> I420 / IYUV (uIdx 1) or YV12 (uIdx 2), one (3/2 height) x width array */
MI355CV_API int mi355cv_cvtBGRtoThreePlaneYUV(const mi355cv_uchar* src_data, size_t src_step, mi355cv_uchar* dst_data, size_t dst_step,
        int width, int height, int scn, bool swapBlue, int uIdx);
/* replaces hal_ni_cvtOnePlaneYUVtoBGR (:833; caller color_yuv.dispatch.cpp:260): YUY2 / YVYU / UYVY (CV_8UC2) -> BGR/RGB(A) */
MI355CV_API int mi355cv_cvtOnePlaneYUVtoBGR(const mi355cv_uchar* src_data, size_t src_step, mi355cv_uchar* dst_data, size_t dst_step,
        int width, int height, int dcn, bool swapBlue, int uIdx, int ycn);
/* replaces hal_ni_cvtOnePlaneBGRtoYUV (:866; caller color_yuv.dispatch.cpp:281) */
MI355CV_API int mi355cv_cvtOnePlaneBGRtoYUV(const mi355cv_uchar* src_data, size_t src_step, mi355cv_uchar* dst_data, size_t dst_step,
        int width, int height, int scn, bool swapBlue, int uIdx, int ycn);
/* replace hal_ni_cvtBGRtoXYZ (:564; caller color_lab.cpp:4134) and hal_ni_cvtXYZtoBGR (:579): CV_8U, CV_16U, CV_32F (the body / tail association of the SSE-baseline build, see csrc/color_misc.hip) */
MI355CV_API int mi355cv_cvtBGRtoXYZ(const mi355cv_uchar* src_data, size_t src_step, mi355cv_uchar* dst_data, size_t dst_step, int width, int height,
        int depth, int scn, bool swapBlue);
MI355CV_API int mi355cv_cvtXYZtoBGR(const mi355cv_uchar* src_data, size_t src_step, mi355cv_uchar* dst_data, size_t dst_step, int width, int height,
        int depth, int dcn, bool swapBlue);
/* replace hal_ni_cvtBGRtoLab (hal_replacement.hpp:535; caller hal::cvtBGRtoLab color_lab.cpp:4230) and hal_ni_cvtLabtoBGR (:550; caller :4327): CV_8U
 * L*a*b* from / to sRGB (COLOR_BGR2Lab ...) or linear RGB (COLOR_LBGR2Lab ...) -- the reference's bit-exact integer paths RGB2Lab_b (:1573) and
 * Lab2RGBinteger (:2399) -- and CV_8U L*u*v* (isLab == false): sRGB -> Luv through the reference's 33^3 interpolation table (RGB2Luvinterpolate :3276),
 * Luv -> sRGB / linear RGB by Luv2RGBinteger (:3556) -- and CV_32F L*a*b* (RGB2Lab_f :1895, Lab2RGBfloat :2169, vector bodies and scalar row tails as the
 * reference has them), CV_32F L*u*v* and CV_8U L*u*v* from linear RGB (RGB2Luvfloat :2868, Luv2RGBfloat :3057): every (depth, isLab, srgb) case the
 * reference's pair of hooks receives (csrc/color_lab.hip) */
MI355CV_API int mi355cv_cvtBGRtoLab(const mi355cv_uchar* src_data, size_t src_step, mi355cv_uchar* dst_data, size_t dst_step, int width, int height,
        int depth, int scn, bool swapBlue, bool isLab, bool srgb);
MI355CV_API int mi355cv_cvtLabtoBGR(const mi355cv_uchar* src_data, size_t src_step, mi355cv_uchar* dst_data, size_t dst_step, int width, int height,
        int depth, int dcn, bool swapBlue, bool isLab, bool srgb);
/* diagnostics: the host-built tables behind the two hooks (0 gamma 256 x u16, 1 cbrt 3072 x u16, 2 invGamma 4096 x u16, 3 (y | ify << 16) 256 x u32,
 * 4 RGB -> Luv grid 33^3 x 4 x i16, 5 / 6 LuToUp / LvToVp 65536 x i32, 7 RGB -> Lab grid, 8 / 9 the cube-root / inverse-gamma splines 4096 x f32);
 * returns the entry count, needs no GPU */
MI355CV_API int mi355cv_labTable(int which, void* out);
/* replace hal_ni_cvtBGRtoBGR5x5 (:411), cvtBGR5x5toBGR (:427), cvtBGR5x5toGray (:470), cvtGraytoBGR5x5 (:484); callers color_rgb.dispatch.cpp */
MI355CV_API int mi355cv_cvtBGRtoBGR5x5(const mi355cv_uchar* src_data, size_t src_step, mi355cv_uchar* dst_data, size_t dst_step, int width, int height,
        int scn, bool swapBlue, int greenBits);
MI355CV_API int mi355cv_cvtBGR5x5toBGR(const mi355cv_uchar* src_data, size_t src_step, mi355cv_uchar* dst_data, size_t dst_step, int width, int height,
        int dcn, bool swapBlue, int greenBits);
MI355CV_API int mi355cv_cvtBGR5x5toGray(const mi355cv_uchar* src_data, size_t src_step, mi355cv_uchar* dst_data, size_t dst_step, int width, int height,
        int greenBits);
MI355CV_API int mi355cv_cvtGraytoBGR5x5(const mi355cv_uchar* src_data, size_t src_step, mi355cv_uchar* dst_data, size_t dst_step, int width, int height,
        int greenBits);
/* replace hal_ni_cvtRGBAtoMultipliedRGBA (:894) and hal_ni_cvtMultipliedRGBAtoRGBA (:907) */
MI355CV_API int mi355cv_cvtRGBAtoMultipliedRGBA(const mi355cv_uchar* src_data, size_t src_step, mi355cv_uchar* dst_data, size_t dst_step, int width, int height);
MI355CV_API int mi355cv_cvtMultipliedRGBAtoRGBA(const mi355cv_uchar* src_data, size_t src_step, mi355cv_uchar* dst_data, size_t dst_step, int width, int height);

/* replaces hal_ni_cvtHSVtoBGR (hal_replacement.hpp:613; caller color_hsv.dispatch.cpp:95): CV_8U, HSV (HLS and CV_32F decline).  The reference's
 * 8-bit result depends on its vector width (truncation in the vector loop, rounding in the scalar tail); this follows the 8-lane AVX2 build,
 * the widest `color_hsv` is dispatched for (modules/imgproc/CMakeLists.txt: SSE2 SSE4_1 AVX2). */
MI355CV_API int mi355cv_cvtHSVtoBGR(const mi355cv_uchar* src_data, size_t src_step, mi355cv_uchar* dst_data, size_t dst_step, int width, int height,
        int depth, int dcn, bool swapBlue, bool isFullRange, bool isHSV);

/* --------------------------------------------------- f1: histogram-driven point operations (csrc/hist.hip) */

/* replaces hal_ni_equalize_hist (hal_replacement.hpp:1120; caller histogram.cpp:3455): CV_8UC1 */
MI355CV_API int mi355cv_equalize_hist(const mi355cv_uchar* src_data, size_t src_step, mi355cv_uchar* dst_data, size_t dst_step, int width, int height);
/* replaces hal_ni_threshold_otsu (:1077; caller thresh.cpp:1568): CV_8UC1 / CV_16UC1; *thresh receives the Otsu level */
MI355CV_API int mi355cv_threshold_otsu(const mi355cv_uchar* src_data, size_t src_step, mi355cv_uchar* dst_data, size_t dst_step, int width, int height,
        int depth, double maxValue, int thresholdType, double* thresh);

/* --------------------------------------------------- CLAHE (csrc/clahe.hip) */

/* cv::createCLAHE(clipLimit, Size(tilesX, tilesY))->apply(src, dst) (imgproc/src/clahe.cpp; no HAL hook) on CV_8UC1 (depth MI355CV_8U) or CV_16UC1
 * (MI355CV_16U), bit-identical to the reference.  margin_right / margin_bottom: real pixels of the parent image right of and below the ROI (locateROI), which
 * the reference's copyMakeBorder takes in before it reflects when a side is not divisible by the tile count; 0 for a whole image.  src == dst is allowed. */
MI355CV_API int mi355cv_clahe(const mi355cv_uchar* src_data, size_t src_step, mi355cv_uchar* dst_data, size_t dst_step, int width, int height, int depth,
        int margin_right, int margin_bottom, double clipLimit, int tilesX, int tilesY);
/* `nframes` whole frames of one geometry, `*_frame_stride` bytes apart (as mi355cv_thresholdBatch): one set of launches per group of frames */
MI355CV_API int mi355cv_claheBatch(const mi355cv_uchar* src_data, size_t src_step, size_t src_frame_stride, mi355cv_uchar* dst_data, size_t dst_step,
        size_t dst_frame_stride, int nframes, int width, int height, int depth, double clipLimit, int tilesX, int tilesY);

/* --------------------------------------------------- f3: sparse pyramidal Lucas-Kanade (modules/video) */

/* replaces hal_ni_ScharrDeriv (modules/video/src/hal_replacement.hpp:84; caller calcScharrDeriv lkpyramid.cpp:67): CV_8U cn 1..4 ->
 * interleaved (dI/dx, dI/dy) CV_16S, 2*cn channels */
MI355CV_API int mi355cv_ScharrDeriv(const mi355cv_uchar* src_data, size_t src_step, short* dst_data, size_t dst_step, int width, int height, int cn);
/* replaces hal_ni_LKOpticalFlowLevel (modules/video/src/hal_replacement.hpp:54; caller LKTrackerInvoker::operator() lkpyramid.cpp:233): one
 * pyramid level.  The three images must be readable one window beyond every edge (the padded pyramids of buildOpticalFlowPyramid).
 * status is non-NULL at level 0 only; termination_epsilon is the squared threshold the caller prepares. */
MI355CV_API int mi355cv_LKOpticalFlowLevel(const mi355cv_uchar* prev_data, size_t prev_data_step, const short* prev_deriv_data, size_t prev_deriv_step,
        const mi355cv_uchar* next_data, size_t next_step, int width, int height, int cn,
        const float* prev_points, float* next_points, size_t point_count, mi355cv_uchar* status, float* err,
        const int win_width, const int win_height, int termination_count, double termination_epsilon,
        bool get_min_eigen_vals, float min_eigen_vals_threshold);
/* cv::calcOpticalFlowPyrLK (lkpyramid.cpp:1432) in one call: frames staged once, padded pyramids, derivatives and all tracker levels on the
 * device.  cv:: argument meaning (criteria = TermCriteria type / maxCount / epsilon, flags = OPTFLOW_*); err may be NULL.  Results are
 * bit-identical to the reference's.  Returns 0, 1 (declined, nothing written) or < 0. */
MI355CV_API int mi355cv_calcOpticalFlowPyrLK(const mi355cv_uchar* prev_data, size_t prev_step, const mi355cv_uchar* next_data, size_t next_step,
        int width, int height, int cn, const float* prev_points, float* next_points, int point_count, mi355cv_uchar* status, float* err,
        int win_width, int win_height, int max_level, int criteria_type, int criteria_max_count, double criteria_epsilon,
        int flags, double min_eig_threshold);
/* cv::copyMakeBorder (core/src/copy.cpp:1183; no HAL hook) for device-resident images: pixels of elem_size bytes, BORDER_CONSTANT = zeros;
 * src may be the interior of dst (then only the frame is written) -- what buildOpticalFlowPyramid does at lkpyramid.cpp:804 */
MI355CV_API int mi355cv_copyMakeBorder(const mi355cv_uchar* src_data, size_t src_step, int width, int height, mi355cv_uchar* dst_data, size_t dst_step,
        int top, int bottom, int left, int right, int elem_size, int border_type);

/* --------------------------------------------------- f1: Canny */

/* replaces hal_ni_canny (hal_replacement.hpp:1291; caller cv::Canny canny.cpp:864).  CV_8U, 1..4 channels, ksize 3 or 5; thresholds as
 * cv::Canny passes them to the hook (before the L2 squaring and the floor).  dst CV_8UC1, 255 on edges. */
MI355CV_API int mi355cv_canny(const mi355cv_uchar* src_data, size_t src_step, mi355cv_uchar* dst_data, size_t dst_step, int width, int height,
        int cn, double lowThreshold, double highThreshold, int ksize, bool L2gradient);

/* --------------------------------------------------- f1: erode / dilate */

/* replace hal_ni_morphInit / hal_ni_morph / hal_ni_morphFree (hal_replacement.hpp:207-233; caller halMorph
 * morph.dispatch.cpp:190-220).  operation 0 = MORPH_ERODE, 1 = MORPH_DILATE; kernel = CV_8UC1 mask; iterations must be 1 (the
 * reference folds iterated rectangles before the hook); borderValue all DBL_MAX = morphologyDefaultBorderValue(). */
MI355CV_API int mi355cv_morphInit(struct cvhalFilter2D** context, int operation, int src_type, int dst_type, int max_width, int max_height,
        int kernel_type, mi355cv_uchar* kernel_data, size_t kernel_step, int kernel_width, int kernel_height, int anchor_x, int anchor_y,
        int borderType, const double borderValue[4], int iterations, bool allowSubmatrix, bool allowInplace);
MI355CV_API int mi355cv_morph(struct cvhalFilter2D* context, mi355cv_uchar* src_data, size_t src_step, mi355cv_uchar* dst_data, size_t dst_step,
        int width, int height, int src_full_width, int src_full_height, int src_roi_x, int src_roi_y,
        int dst_full_width, int dst_full_height, int dst_roi_x, int dst_roi_y);
MI355CV_API int mi355cv_morphFree(struct cvhalFilter2D* context);

/* --------------------------------------------------- f1: median filter */

/* replaces hal_ni_medianBlur (hal_replacement.hpp:995; caller cv::medianBlur median_blur.dispatch.cpp:300).  CV_8U, ksize 3 or 5,
 * 1/3/4 channels; everything else answers NOT_IMPLEMENTED (CPU fallback). */
MI355CV_API int mi355cv_medianBlur(const mi355cv_uchar* src_data, size_t src_step, mi355cv_uchar* dst_data, size_t dst_step,
        int width, int height, int depth, int cn, int ksize);

/* --------------------------------------------------- a13: template matching */

/* cv::matchTemplate (templmatch.cpp:1158) has no HAL hook.  type CV_8UC1..C4 / CV_32FC1..C4, result CV_32FC1
 * (img_width - templ_width + 1) x (img_height - templ_height + 1), method = cv::TemplateMatchModes 0..5. */
MI355CV_API int mi355cv_matchTemplate(const mi355cv_uchar* img_data, size_t img_step, int img_width, int img_height,
        const mi355cv_uchar* templ_data, size_t templ_step, int templ_width, int templ_height, int type,
        mi355cv_uchar* result_data, size_t result_step, int method);
/* the same with a mask (matchTemplateMask, templmatch.cpp:762-904): mask of the template's size, CV_8U (non-zero counts as 1) or CV_32F (weights), one channel
 * or the template's channel count */
MI355CV_API int mi355cv_matchTemplateMask(const mi355cv_uchar* img_data, size_t img_step, int img_width, int img_height,
        const mi355cv_uchar* templ_data, size_t templ_step, int templ_width, int templ_height, int type,
        const mi355cv_uchar* mask_data, size_t mask_step, int mask_type, mi355cv_uchar* result_data, size_t result_step, int method);
/* frames x one shared template (frames shard, the template is replicated) */
MI355CV_API int mi355cv_matchTemplateBatch(const mi355cv_uchar* img_data, size_t img_step, size_t img_frame_stride, int nframes,
        int img_width, int img_height, const mi355cv_uchar* templ_data, size_t templ_step, int templ_width, int templ_height,
        int type, mi355cv_uchar* result_data, size_t result_step, size_t result_frame_stride, int method);
/* replaces hal_ni_integral (hal_replacement.hpp:977; caller sumpixels.dispatch.cpp:415): every (depth, sdepth, sqdepth) row of the reference's table
 * (sumpixels.dispatch.cpp:383-406), sqsum_data / tilted_data may be NULL.  Integer-valued sums are exact; float sums, float / int squared sums and tilted sums are
 * accumulated in the reference's order (bit for bit).  Declined: CV_8U -> CV_32F sums past 2^24 when neither sqsum nor tilted is asked for (the reference's
 * result then depends on the CPU's vector width). */
MI355CV_API int mi355cv_integral(int depth, int sdepth, int sqdepth, const mi355cv_uchar* src_data, size_t src_step,
        mi355cv_uchar* sum_data, size_t sum_step, mi355cv_uchar* sqsum_data, size_t sqsum_step,
        mi355cv_uchar* tilted_data, size_t tilted_step, int width, int height, int cn);

/* cv::integral over `nframes` device-resident CV_8UC1 frames: sums in CV_32S or CV_64F (sdepth), optional CV_64F squared sums (sqsum_data may be
 * NULL), each (height+1) x (width+1); strides in bytes; one set of launches for the whole batch */
MI355CV_API int mi355cv_integralBatch(const mi355cv_uchar* src_data, size_t src_step, size_t src_frame_stride, mi355cv_uchar* sum_data, size_t sum_step,
        size_t sum_frame_stride, mi355cv_uchar* sqsum_data, size_t sqsum_step, size_t sqsum_frame_stride, int nframes, int width, int height, int sdepth);

/* --------------------------------------------------- batches of device-resident frames (frames are the unit that shards)
 * The frame-batched forms of the hooks above: `nframes` whole images of identical geometry, `*_frame_stride` bytes apart, borders per frame.
 * One launch where the kernel takes a frame index (the rolling filters, nearest / bilinear / area-fast resize, the warps, threshold on
 * back-to-back frames), otherwise the per-frame kernels enqueued by one call.  Both ends in HBM -- or both in host memory (pageable or page-locked): the
 * batch then crosses PCIe in chunks of <= 16 frames / 64 MB through two sets of device buffers, upload of chunk i+1 overlapped with the kernels and the
 * download of chunk i; mi355cv_buildPyramidBatch (one output per level) and mi355cv_matchTemplateBatch included. */
MI355CV_API int mi355cv_sobelBatch(const mi355cv_uchar* src_data, size_t src_step, size_t src_frame_stride, mi355cv_uchar* dst_data, size_t dst_step,
        size_t dst_frame_stride, int nframes, int width, int height, int src_depth, int dst_depth, int cn, int dx, int dy, int ksize, double scale, double delta,
        int border_type);
MI355CV_API int mi355cv_sepFilterBatch(struct cvhalFilter2D* context, const mi355cv_uchar* src_data, size_t src_step, size_t src_frame_stride, mi355cv_uchar* dst_data,
        size_t dst_step, size_t dst_frame_stride, int nframes, int width, int height);
MI355CV_API int mi355cv_boxFilterBatch(const mi355cv_uchar* src_data, size_t src_step, size_t src_frame_stride, mi355cv_uchar* dst_data, size_t dst_step,
        size_t dst_frame_stride, int nframes, int width, int height, int src_depth, int dst_depth, int cn, size_t ksize_width, size_t ksize_height,
        int anchor_x, int anchor_y, bool normalize, int border_type);
MI355CV_API int mi355cv_thresholdBatch(const mi355cv_uchar* src_data, size_t src_step, size_t src_frame_stride, mi355cv_uchar* dst_data, size_t dst_step,
        size_t dst_frame_stride, int nframes, int width, int height, int depth, int cn, double thresh, double maxValue, int thresholdType);
MI355CV_API int mi355cv_resizeBatch(int src_type, const mi355cv_uchar* src_data, size_t src_step, size_t src_frame_stride, int src_width, int src_height,
        mi355cv_uchar* dst_data, size_t dst_step, size_t dst_frame_stride, int dst_width, int dst_height, int nframes, double inv_scale_x, double inv_scale_y,
        int interpolation);
MI355CV_API int mi355cv_warpAffineBatch(int src_type, const mi355cv_uchar* src_data, size_t src_step, size_t src_frame_stride, int src_width, int src_height,
        mi355cv_uchar* dst_data, size_t dst_step, size_t dst_frame_stride, int dst_width, int dst_height, int nframes, const double M[6], int interpolation,
        int borderType, const double borderValue[4]);
MI355CV_API int mi355cv_warpPerspectiveBatch(int src_type, const mi355cv_uchar* src_data, size_t src_step, size_t src_frame_stride, int src_width, int src_height,
        mi355cv_uchar* dst_data, size_t dst_step, size_t dst_frame_stride, int dst_width, int dst_height, int nframes, const double M[9], int interpolation,
        int borderType, const double borderValue[4]);

/* --------------------------------------------------- f3: features2d FAST corner detector (csrc/fast.hip) */
/* replace hal_ni_FAST_dense / hal_ni_FAST_NMS (modules/features2d/src/hal_replacement.hpp:75, :87; caller hal_FAST fast.cpp:438-493, which is reached
 * for threshold <= 20): dense score = largest t + 1 for which the pixel is a 9-of-16 corner at threshold t (0 in the 3-pixel frame); the suppression
 * keeps scores strictly greater than their 8 neighbours.  `type`: cv::FastFeatureDetector::DetectorType, TYPE_9_16 (2) only. */
MI355CV_API int mi355cv_FAST_dense(const mi355cv_uchar* src_data, size_t src_step, mi355cv_uchar* dst_data, size_t dst_step, int width, int height, int type);
MI355CV_API int mi355cv_FAST_NMS(const mi355cv_uchar* src_data, size_t src_step, mi355cv_uchar* dst_data, size_t dst_step, int width, int height);
/* cv::FAST (fast.cpp:496) as one call, any threshold: keypoints as (x, y, response) float triples in the reference's (raster) order, at most
 * `capacity` written.  Returns the number found (>= 0; call again with a larger array if it exceeds capacity), -1 unsupported, -2 device failure. */
MI355CV_API int mi355cv_FAST(const mi355cv_uchar* src_data, size_t src_step, int width, int height, int threshold, int nonmax_suppression, int type,
        float* keypoints_xyr, int capacity);

/* --------------------------------------------------- f3: features2d ORB (csrc/orb.hip) */
/* cv::KeyPoint (core/types.hpp:777) and the parameters of cv::ORB (features2d.hpp:449-510; scoreType: ORB::HARRIS_SCORE 0, FAST_SCORE 1).  scaleFactor is the
 * double the reference keeps: ORB::create takes a float (pass (double)(float)f for it), setScaleFactor a double */
typedef struct mi355cv_KeyPoint { float x, y, size, angle, response; int octave, class_id; } mi355cv_KeyPoint;
typedef struct mi355cv_OrbParams { int nfeatures; double scaleFactor; int nlevels, edgeThreshold, firstLevel, WTA_K, scoreType, patchSize, fastThreshold; } mi355cv_OrbParams;
/* cv::ORB::detectAndCompute (modules/features2d/src/orb.cpp:1012; the reference has no HAL hook for it) on a CV_8UC1 image in host or device
 * memory: pyramid, FAST, Harris responses, orientation, smoothing and the rBRIEF descriptors on the GPU; the two culls (KeyPointsFilter::retainBest)
 * on the host with the C++ library's nth_element, so keypoints leave in the reference's order.  `mask`: optional CV_8UC1 image of the same size.
 * use_provided_keypoints != 0: describe the nkeypoints_in keypoints passed in (Feature2D::compute).  `descriptors`: rows of 32 bytes, or NULL to
 * detect only.  At most `capacity` keypoints / rows are written.  Returns the keypoint count (>= 0; call again with larger arrays if it exceeds
 * capacity -- nothing was written then), -1 arguments not served, -2 device failure. */
MI355CV_API int mi355cv_ORB_detectAndCompute(const mi355cv_uchar* image, size_t step, int width, int height, const mi355cv_uchar* mask, size_t mask_step,
        const mi355cv_OrbParams* params, int use_provided_keypoints, mi355cv_KeyPoint* keypoints, int nkeypoints_in, int capacity,
        mi355cv_uchar* descriptors, size_t descriptors_step);

/* --------------------------------------------------- f3: features2d BFMatcher (csrc/bfmatch.hip) */
/* cv::DMatch (core/types.hpp): 16 bytes.  A list shorter than its plane is padded with cv::DMatch's default, {-1, -1, -1, FLT_MAX} */
typedef struct mi355cv_DMatch { int queryIdx, trainIdx, imgIdx; float distance; } mi355cv_DMatch;
/* cv::BFMatcher::knnMatch (modules/features2d, no HAL hook; the definition served is written down in DESIGN 6.16 and tests/bfmatch_restate.py).  `query`: nq rows of `len`
 * elements of `type` (MI355CV_8U or MI355CV_32F, one channel) at pitch query_step; the train collection: nimg matrices train[i] of train_rows[i] rows at train_step[i],
 * imgIdx = i; masks: NULL, or nimg pointers, each NULL or a CV_8UC1 nq x train_rows[i] matrix at mask_step[i] (0 excludes the pair).  normType: 6 NORM_HAMMING /
 * 7 NORM_HAMMING2 on CV_8U, 2 NORM_L1 / 4 NORM_L2 / 5 NORM_L2SQR on CV_32F (every float operation rounded on its own, elements ascending; L2 the correctly rounded
 * root).  A pair whose distance is NaN is not a candidate.  Candidates of a query are ordered by (distance, imgIdx, trainIdx); `matches` is the nq x k plane of the first
 * k of them per query, counts[q] = how many there are.  crossCheck != 0 (k = 1 only, anything else is an error): (q, t) stays iff q is also the best query of t by
 * (distance, queryIdx).  Every matrix may live in host memory (staged through HBM, host-cost class HOST_HEAVY) or in this thread's device memory, at any pitch and, for
 * CV_8U, any byte address; with device outputs nothing is downloaded.  nq = 0 and train_rows[i] = 0 are legal.
 * Declined (MI355CV_NOT_IMPLEMENTED): other (type, normType) pairs; nq or the collection's rows above mi355cv_limit("bfmatch_max_rows") = 2^24; k outside
 * 1 .. mi355cv_limit("bfmatch_max_k") = 8; rows above mi355cv_limit("bfmatch_max_row_bytes") = 2048 bytes; nimg outside 1 .. mi355cv_limit("bfmatch_max_images") = 64; a
 * pitch below the row; CV_32F rows, matches or counts off a 4-byte boundary; crossCheck with a mask or with nimg > 1. */
MI355CV_API int mi355cv_bfKnnMatch(const void* query, size_t query_step, int nq, int len, int type, const void* const* train, const size_t* train_step,
        const int* train_rows, const void* const* masks, const size_t* mask_step, int nimg, int normType, int k, int crossCheck, mi355cv_DMatch* matches, int* counts);
/* npairs independent (query[b], train[b]) pairs with their own row counts in ONE sequence of launches; exactly the results of npairs single calls (one train matrix,
 * no mask).  matches[b]: the nq[b] x k plane of pair b, counts[b]: its nq[b] counts.  npairs <= 65535. */
MI355CV_API int mi355cv_bfKnnMatchBatch(const void* const* query, const size_t* query_step, const int* nq, const void* const* train, const size_t* train_step,
        const int* train_rows, int npairs, int len, int type, int normType, int k, int crossCheck, mi355cv_DMatch* const* matches, int* const* counts);
/* cv::BFMatcher::radiusMatch: every candidate with distance <= maxDistance, per query in (distance, imgIdx, trainIdx) order; the lists of queries 0 .. nq - 1 follow one
 * another in `matches`, counts[q] their lengths.  The capacity convention of mi355cv_FAST: returns the total (>= 0; at most `capacity` records were written: call again
 * with a larger array if it exceeds capacity), -1 arguments not served, -2 device failure.  Declined as well: a query with more than
 * mi355cv_limit("bfmatch_max_radius_row") = 4096 matches (its list is sorted in LDS). */
MI355CV_API int mi355cv_bfRadiusMatch(const void* query, size_t query_step, int nq, int len, int type, const void* const* train, const size_t* train_step,
        const int* train_rows, const void* const* masks, const size_t* mask_step, int nimg, int normType, float maxDistance, mi355cv_DMatch* matches, int capacity,
        int* counts);
/* A/B switch of the split of the train rows over workgroups (tools/bfmatch_bench.py --ab): 0 one pass over all train rows per query, -1 or 1 the built-in rule
 * (parts of mi355cv_limit("bfmatch_split_rows") rows merged by key).  Results do not depend on it. */
MI355CV_API int mi355cv_bfSetSplitMode(int mode);

/* --------------------------------------------------- f3: calib3d StereoBM (csrc/stereobm.hip) */
/* The parameters of cv::StereoBM (calib3d.hpp).  numDisparities <= 0 means 64; preFilterType: 0 PREFILTER_NORMALIZED_RESPONSE, 1 PREFILTER_XSOBEL; roi1 / roi2 are
 * (x, y, width, height), all zero when unset.  mi355cv_stereoBMDefaults fills the values of StereoBM::create(0, 21). */
typedef struct mi355cv_StereoBMParams {
    int minDisparity, numDisparities, blockSize, preFilterType, preFilterSize, preFilterCap, textureThreshold, uniquenessRatio, speckleWindowSize, speckleRange, disp12MaxDiff;
    int roi1[4], roi2[4];
} mi355cv_StereoBMParams;
MI355CV_API void mi355cv_stereoBMDefaults(mi355cv_StereoBMParams* params);
/* cv::StereoBM::compute (modules/calib3d, no HAL hook; the definition served is written down in DESIGN 6.17 and tests/stereobm_restate.py) on two rectified CV_8UC1
 * images of width x height: the CV_16SC1 map of disparities times 16 (disp_depth = MI355CV_16S) or the CV_32FC1 map of disparities (MI355CV_32F, the former divided by
 * 16, exact).  A pixel without a disparity holds (minDisparity - 1) * 16, respectively minDisparity - 1.  All arithmetic is integer: the map is determined bit for bit.
 * Every image may live in host memory (staged through HBM, host-cost class HOST_HEAVY) or in this thread's device memory, at any pitch and byte address; device
 * pointers run on the current stream.
 * Declined (MI355CV_NOT_IMPLEMENTED, disp left untouched): PREFILTER_NORMALIZED_RESPONSE; speckleWindowSize > 0; roi1 / roi2 set; other disparity depths; numDisparities
 * not a positive multiple of 16 or above mi355cv_limit("stereobm_max_disparities") = 256; blockSize even, below 5, above min(width, height) or above
 * mi355cv_limit("stereobm_max_block") = 51; preFilterCap outside 1 .. 63; a negative textureThreshold or uniquenessRatio; width or height above
 * mi355cv_limit("stereobm_max_dim") = 16384; disparities that leave the CV_16S map's range (minDisparity < -2047 or minDisparity + numDisparities - 1 > 2046); a pitch below
 * the row; disparity rows off their element's boundary; a disparity map that overlaps an input. */
MI355CV_API int mi355cv_stereoBM(const mi355cv_uchar* left, size_t left_step, const mi355cv_uchar* right, size_t right_step, mi355cv_uchar* disp, size_t disp_step,
        int width, int height, int disp_depth, const mi355cv_StereoBMParams* params);
/* nframes pairs at left + f * left_frame_stride, right + f * right_frame_stride into disp + f * disp_frame_stride in ONE sequence of launches; exactly the results of
 * nframes single calls.  Declined as well: nframes < 1 or > 65535, a frame stride below the frame. */
MI355CV_API int mi355cv_stereoBMBatch(const mi355cv_uchar* left, size_t left_step, size_t left_frame_stride, const mi355cv_uchar* right, size_t right_step,
        size_t right_frame_stride, mi355cv_uchar* disp, size_t disp_step, size_t disp_frame_stride, int nframes, int width, int height, int disp_depth,
        const mi355cv_StereoBMParams* params);
/* The stage entry: the XSOBEL prefilter of one CV_8UC1 image, dst = clip(cap + the 3 x 3 x-Sobel, 0, 2 cap), rows under BORDER_REFLECT_101, the first and last column = cap.
 * cap in 1 .. 63. */
MI355CV_API int mi355cv_stereoPrefilterXSobel(const mi355cv_uchar* src, size_t src_step, mi355cv_uchar* dst, size_t dst_step, int width, int height, int cap);
/* A/B switch of the cost kernel (tools/stereobm_bench.py): -1 the built-in rule (blockSize <= mi355cv_limit("stereobm_roll_max_block") = 21: the rolling kernel), 0 always
 * the generic kernel.  Results do not depend on it. */
MI355CV_API int mi355cv_stereoBMSetKernel(int mode);

/* --------------------------------------------------- f3: calib3d filterSpeckles (csrc/speckle.hip) */
/* cv::filterSpeckles (modules/calib3d, no HAL hook; the definition served is written down in DESIGN 6.18 and tests/speckle_restate.py) on one channel of CV_8U or
 * CV_16S (depth = MI355CV_8U / MI355CV_16S), IN PLACE: a pixel is live iff its value != newVal; two live 4-neighbours are linked iff |a - b| <= maxDiff (in int);
 * every pixel of a connected component of at most maxSpeckleSize pixels becomes newVal, every other byte keeps its value.  maxSpeckleSize <= 0 erases nothing;
 * maxDiff < 0 links nothing.  The image depends on component sizes only: it is determined bit for bit.  The image may live in host memory (staged through HBM,
 * host-cost class HOST_HEAVY) or in this thread's device memory, at any pitch and any byte address a CV_8U / CV_16S row may have; device pointers run on the
 * current stream.
 * Declined (MI355CV_NOT_IMPLEMENTED, the image left untouched): other depths; a null pointer; width or height < 1 or above mi355cv_limit("speckle_max_dim") = 16384;
 * a pitch below the row; CV_16S rows off a 2-byte boundary; newVal outside the depth's range (the reference would store it truncated). */
MI355CV_API int mi355cv_filterSpeckles(mi355cv_uchar* img, size_t step, int width, int height, int depth, int newVal, int maxSpeckleSize, int maxDiff);
/* nframes maps at img + f * frame_stride in ONE sequence of launches, the frame in the grid's z; every frame is bit for bit the single call's.  Declined as well:
 * nframes < 1 or > 65535, frames that overlap (a frame stride below the frame). */
MI355CV_API int mi355cv_filterSpecklesBatch(mi355cv_uchar* img, size_t step, size_t frame_stride, int nframes, int width, int height, int depth, int newVal,
        int maxSpeckleSize, int maxDiff);
/* A/B switch (tools/speckle_bench.py): -1 the built-in rule (the tile kernel, tiles of mi355cv_limit("speckle_tile_cols") x mi355cv_limit("speckle_tile_rows") merged
 * in LDS), 0 always the plain per-pixel kernels.  Results do not depend on it. */
MI355CV_API int mi355cv_filterSpecklesSetKernel(int mode);

/* --------------------------------------------------- f3: calib3d StereoSGBM (csrc/sgbm.hip) */
/* The parameters of cv::StereoSGBM (calib3d.hpp).  mode: 0 MODE_SGBM (5 directions), 1 MODE_HH (8), 2 MODE_SGBM_3WAY (declined), 3 MODE_HH4 (4).
 * mi355cv_stereoSGBMDefaults fills the values of StereoSGBM::create(): 0, 16, 3, 0, 0, 0, 0, 0, 0, 0, MODE_SGBM. */
typedef struct mi355cv_StereoSGBMParams {
    int minDisparity, numDisparities, blockSize, P1, P2, disp12MaxDiff, preFilterCap, uniquenessRatio, speckleWindowSize, speckleRange, mode;
} mi355cv_StereoSGBMParams;
MI355CV_API void mi355cv_stereoSGBMDefaults(mi355cv_StereoSGBMParams* params);
/* cv::StereoSGBM::compute (modules/calib3d, no HAL hook; the definition served is written down in DESIGN 6.19 and tests/sgbm_restate.py) on two rectified CV_8UC1
 * images of width x height: the CV_16SC1 map of disparities times 16 (disp_depth = MI355CV_16S) or the CV_32FC1 map of disparities (MI355CV_32F, the former divided by
 * 16, exact).  A pixel without a disparity holds (minDisparity - 1) * 16, respectively minDisparity - 1.  All arithmetic is integer: the map is determined bit for bit.
 * speckleWindowSize > 0 runs mi355cv_filterSpecklesBatch on the CV_16S map (newVal (minDisparity - 1) * 16, maxDiff 16 * speckleRange) before it is delivered.
 * Every image may live in host memory (staged through HBM, host-cost class HOST_HEAVY) or in this thread's device memory, at any pitch and byte address; device
 * pointers run on the current stream.  Scratch: 6 bytes per valid pixel and disparity (the 16-bit block costs and the 32-bit path sums) from the runtime's pool.
 * Declined (MI355CV_NOT_IMPLEMENTED, disp left untouched): MODE_SGBM_3WAY and unknown modes; other disparity depths; numDisparities not a positive multiple of 16 or
 * above mi355cv_limit("sgbm_max_disparities") = 256; blockSize even or below 1; preFilterCap < 0; P1 < 0 or P2 < P1 (P1 = P2 = 0 is served as given); uniquenessRatio
 * outside 0 .. 100; negative speckle arguments; blockSize^2 * (2 ft + 63) + P2 > mi355cv_limit("sgbm_max_cost") = 32767 with ft = max(preFilterCap, 15) | 1 (costs are
 * 16 bit); minDisparity < -2047 or minDisparity + numDisparities - 1 > 2046; width or height above mi355cv_limit("sgbm_max_dim") = 16384; a frame whose scratch exceeds
 * mi355cv_limit("sgbm_max_scratch_mib") = 16384 MiB; a pitch below the row; disparity rows off their element's boundary; a disparity map that overlaps an input. */
MI355CV_API int mi355cv_stereoSGBM(const mi355cv_uchar* left, size_t left_step, const mi355cv_uchar* right, size_t right_step, mi355cv_uchar* disp, size_t disp_step,
        int width, int height, int disp_depth, const mi355cv_StereoSGBMParams* params);
/* nframes pairs at left + f * left_frame_stride, right + f * right_frame_stride into disp + f * disp_frame_stride; exactly the results of nframes single calls.  The
 * frames run in chunks whose volumes fit the scratch bound, each chunk one sequence of launches with the frame in the grid's z.  Declined as well: nframes < 1, a frame
 * stride below the frame, stacks whose extents overlap. */
MI355CV_API int mi355cv_stereoSGBMBatch(const mi355cv_uchar* left, size_t left_step, size_t left_frame_stride, const mi355cv_uchar* right, size_t right_step,
        size_t right_frame_stride, mi355cv_uchar* disp, size_t disp_step, size_t disp_frame_stride, int nframes, int width, int height, int disp_depth,
        const mi355cv_StereoSGBMParams* params);
/* A/B switch of the path aggregation (tools/sgbm_bench.py): -1 the built-in rule (the fast kernel: lanes across the disparities, loads of a block of steps in flight),
 * 0 always the plain kernel (a workgroup per path, a lane per disparity), 1 always the fast one.  Results do not depend on it. */
MI355CV_API int mi355cv_stereoSGBMSetKernel(int mode);
/* Lowers the scratch bound to `bytes` (0: back to the limit), so that the chunking of batches can be exercised at small shapes.  Results do not depend on it. */
MI355CV_API int mi355cv_stereoSGBMSetScratchLimit(size_t bytes);

/* --------------------------------------------------- f3: photo fastNlMeansDenoising (csrc/nlmeans.hip) */
/* cv::fastNlMeansDenoising (modules/photo, no HAL hook; the definition served is written down in DESIGN 6.20 and tests/nlmeans_restate.py) on a CV_8U image of
 * cn = 1 .. 4 channels: h[0] is the filter strength (hn = 1), templateWindowSize and searchWindowSize count as the next odd value when even, normType is
 * cv::NORM_L2 = 4.  The weights are a table of integers built once per call on the host; everything after it is integer arithmetic: the result is determined bit for bit.
 * Images may live in host memory (staged through HBM, host-cost class HOST_HEAVY) or in this thread's device memory, at any pitch and byte address; device pointers run
 * on the current stream.  Images narrower or shorter than the border th + sh are served.
 * Declined (MI355CV_NOT_IMPLEMENTED, dst left untouched, the reason in mi355cv_lastError): NORM_L1 (2) and CV_16U; other depths; cn outside 1 .. 4; hn != 1 (a per-channel
 * h vector); a window below 1 or, as used, above mi355cv_limit("nlm_max_window") = 181 (T * T <= 2^15; the same bound holds S, far inside the S whose S * S * 255 overflows);
 * S^2 T^2 cn, the squared differences per pixel of the rule as written, above mi355cv_limit("nlm_max_pixel_work") = 2^24; width or height above
 * mi355cv_limit("nlm_max_dim") = 16384; a pitch below the row; src and dst that overlap (in host memory as well). */
MI355CV_API int mi355cv_fastNlMeansDenoising(const mi355cv_uchar* src, size_t src_step, mi355cv_uchar* dst, size_t dst_step, int width, int height, int depth, int cn,
        const float* h, int hn, int templateWindowSize, int searchWindowSize, int normType);
/* nframes frames at src + f * src_frame_stride into dst + f * dst_frame_stride; exactly the results of nframes single calls.  Device-resident frames run with the frame in
 * the grid's z, in launches of at most 65535 frames (mi355cv_fastNlMeansSetChunk lowers that); host-resident batches cross PCIe in chunks through the shared pipeline.
 * Declined as well: nframes < 1, a frame stride below the frame. */
MI355CV_API int mi355cv_fastNlMeansDenoisingBatch(const mi355cv_uchar* src, size_t src_step, size_t src_frame_stride, mi355cv_uchar* dst, size_t dst_step,
        size_t dst_frame_stride, int nframes, int width, int height, int depth, int cn, const float* h, int hn, int templateWindowSize, int searchWindowSize, int normType);
/* cv::fastNlMeansDenoisingColored on CV_8UC3: mi355cv_cvtBGRtoLab (COLOR_LBGR2Lab), the rule on L with h and on a, b together with hColor (cn = 2) straight out of the Lab
 * image into a second one, mi355cv_cvtLabtoBGR (COLOR_Lab2LBGR).  Declined as above, and: cn = 4 (CV_8UC4) and every cn but 3. */
MI355CV_API int mi355cv_fastNlMeansDenoisingColored(const mi355cv_uchar* src, size_t src_step, mi355cv_uchar* dst, size_t dst_step, int width, int height, int depth, int cn,
        float h, float hColor, int templateWindowSize, int searchWindowSize);
MI355CV_API int mi355cv_fastNlMeansDenoisingColoredBatch(const mi355cv_uchar* src, size_t src_step, size_t src_frame_stride, mi355cv_uchar* dst, size_t dst_step,
        size_t dst_frame_stride, int nframes, int width, int height, int depth, int cn, float h, float hColor, int templateWindowSize, int searchWindowSize);
/* Host only, touches no device: the weight table of the rule.  info[0 .. 3] = its length, the shift of a distance, the weight of distance 0 (mult) and the length of
 * the non-zero prefix (the table is non-increasing); table, which may be NULL, receives min(length, capacity) entries. */
MI355CV_API int mi355cv_fastNlMeansWeights(float h, int cn, int templateWindowSize, int searchWindowSize, int* table, int capacity, int* info);
/* A/B switch (tools/nlmeans_bench.py): -1 the built-in rule, 0 always the plain kernel (a lane per pixel, the rule as written), 1 the tile kernel wherever it applies
 * (T <= mi355cv_limit("nlm_tile_max_template") = 9, a prefix of at most mi355cv_limit("nlm_lds_table") = 49152 entries, table and tile within
 * mi355cv_limit("nlm_tile_lds_kib") = 160 KiB of LDS; mi355cv_limit("nlm_tile_cols") = 128 counts the LANES across a workgroup, whose output columns are 2 (64 - (T - 1)); the plain kernel
 * serves the rest).  Results do not depend on it. */
MI355CV_API int mi355cv_fastNlMeansSetKernel(int mode);
/* Lowers the frames per launch of a device-resident batch (0: back to 65535; the Colored entries take 16 at most), so that the cutting of batches can be exercised at
 * small shapes.  Results do not depend on it. */
MI355CV_API int mi355cv_fastNlMeansSetChunk(int frames);

/* --------------------------------------------------- f3: calib3d rectification (csrc/undistort.hip) */
/* cv::initUndistortRectifyMap, cv::undistort, the rectifying warp and cv::reprojectImageTo3D (modules/calib3d, no HAL hook).  The definition served is written down in
 * DESIGN 6.21 and tests/undistort_restate.py: the closed form of the map per destination pixel in separately rounded IEEE doubles.  K: the camera matrix, 9 doubles row
 * by row; dist: ndist = 0, 4, 5, 8, 12 or 14 coefficients k1 k2 p1 p2 k3 k4 k5 k6 s1 s2 s3 s4 tauX tauY (NULL with ndist = 0); R: any 3 x 3 (a rotation or a
 * homography), NULL = identity; newK: 3 x 3 (the left 3 x 3 of a 3 x 4 P), NULL = K.  Out of scope: stereoRectify, getOptimalNewCameraMatrix, undistortPoints, the
 * fisheye model.
 * m1type: CV_32FC1 (map1 = u, map2 = v as floats), CV_32FC2 (map1 alone) or CV_16SC2 (map1 = the integer coordinates, map2 = CV_16UC1 fractions, the form of
 * cv::convertMaps; a non-finite coordinate gives entry (0, 0), fraction 0).  The maps may live in host or device memory, at any pitch that keeps their elements aligned.
 * Declined (MI355CV_NOT_IMPLEMENTED, nothing written, the reason in mi355cv_lastError), each before a device is touched: ndist outside the list; a non-zero tauX / tauY;
 * newK * R with a determinant that is 0 or not finite; width or height below 1 or above mi355cv_limit("undist_max_dim") = 16384; a pitch below the row; maps that
 * overlap; another m1type. */
MI355CV_API int mi355cv_initUndistortRectifyMap(const double* K, const double* dist, int ndist, const double* R, const double* newK, int width, int height, int m1type,
        void* map1, size_t map1_step, void* map2, size_t map2_step);
/* The rectifying warp: BY DEFINITION mi355cv_remap of the source with the CV_16SC2 + CV_16UC1 maps of the rule above, for every depth, channel count, interpolation and
 * border mode mi355cv_remap serves for fixed-point maps -- without the maps ever existing on CV_8U with 1, 3 or 4 channels under INTER_LINEAR (k_undist8_tile evaluates
 * the rule once per destination tile).  cv::undistort is this with R = NULL, the destination of the source's size, INTER_LINEAR, BORDER_CONSTANT, border value 0.
 * Declined as above, and: a source beyond mi355cv_limit("undist_max_src_dim") = 32767; src and dst that overlap (in host memory as well). */
MI355CV_API int mi355cv_undistortRectify(int src_type, const mi355cv_uchar* src, size_t src_step, int src_width, int src_height, mi355cv_uchar* dst, size_t dst_step,
        int dst_width, int dst_height, const double* K, const double* dist, int ndist, const double* R, const double* newK, int interpolation, int border_type,
        const double* border_value);
/* nframes frames of one camera; exactly the results of nframes single calls.  The tile kernel evaluates the rule once per tile and walks
 * mi355cv_limit("undist_frames_per_group") frames with it; host-resident batches cross PCIe in chunks through the shared pipeline.  Declined as well: nframes < 1, a frame
 * stride below the frame. */
MI355CV_API int mi355cv_undistortRectifyBatch(int src_type, const mi355cv_uchar* src, size_t src_step, size_t src_frame_stride, int src_width, int src_height,
        mi355cv_uchar* dst, size_t dst_step, size_t dst_frame_stride, int dst_width, int dst_height, int nframes, const double* K, const double* dist, int ndist,
        const double* R, const double* newK, int interpolation, int border_type, const double* border_value);
/* cv::reprojectImageTo3D: a one-channel disparity of CV_8U, CV_16S, CV_32S or CV_32F -> CV_32FC3 points, Q row by row (16 doubles).  Per pixel in double
 * h_r = ((Q[r][0] x + Q[r][1] y) + Q[r][2] d) + Q[r][3], the point is (float)(h_r * (1 / h_3)).  handleMissingValues: a pixel with |d - dmin| <= FLT_EPSILON gets
 * z = 10000, dmin the minimum of ITS frame (mi355cv_minMaxLocBatch, the result stays in HBM: no host synchronisation; a NaN is no candidate).  ddepth: -1 or CV_32F.
 * Declined: other disparity types; ddepth CV_16S / CV_32S; width or height above mi355cv_limit("reproject_max_dim") = 16384; pitches below the row or off the element
 * size; overlap; nframes < 1; a frame stride below the frame. */
MI355CV_API int mi355cv_reprojectImageTo3D(const mi355cv_uchar* disp, size_t disp_step, int disp_type, mi355cv_uchar* dst, size_t dst_step, int width, int height,
        const double* Q, int handleMissingValues, int ddepth);
MI355CV_API int mi355cv_reprojectImageTo3DBatch(const mi355cv_uchar* disp, size_t disp_step, size_t disp_frame_stride, int disp_type, mi355cv_uchar* dst, size_t dst_step,
        size_t dst_frame_stride, int width, int height, int nframes, const double* Q, int handleMissingValues, int ddepth);
/* A/B switch (tools/undistort_bench.py): -1 the built-in rule, 0 composed (the maps into scratch, then the remap kernels per frame), 1 the tile kernel wherever it
 * applies.  Results do not depend on it. */
MI355CV_API int mi355cv_undistortSetKernel(int mode);
/* The tile kernel's LDS allotment in bytes (0: back to mi355cv_limit("undist_lds_kib") = 24 KiB; at most mi355cv_limit("undist_max_lds_kib") = 48 KiB): a tile whose
 * source box exceeds it takes the per-pixel sampler, so a small value reaches that arm at small shapes.  Results do not depend on it. */
MI355CV_API int mi355cv_undistortSetLds(int bytes);
/* The frames a workgroup of the tile kernel walks with one evaluation of the rule (0: back to mi355cv_limit("undist_frames_per_group"); at most
 * mi355cv_limit("undist_max_frames_per_group") = 64).  Results do not depend on it. */
MI355CV_API int mi355cv_undistortSetFramesPerGroup(int frames);

#ifdef __cplusplus
}
#endif
#endif /* MI355CV_H */
