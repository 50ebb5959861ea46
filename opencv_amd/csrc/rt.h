// rt.h -- internal runtime of libmi355cv.so: per-thread HIP stream, pointer
// classification, host<->HBM staging, error/trace bookkeeping.
// Everything above this (the exported mi355cv_* hooks) speaks the HAL contract
// of the reference (hal_replacement.hpp:1342-1357): never throw, return
// OK / NOT_IMPLEMENTED / UNKNOWN.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>
#include <stdlib.h>
#include <vector>
#include <functional>
#include "../../include/mi355cv.h"

typedef unsigned char uchar;

namespace mi355 {

// border codes (core/base.hpp:332)
enum { B_CONSTANT = 0, B_REPLICATE = 1, B_REFLECT = 2, B_WRAP = 3, B_REFLECT_101 = 4, B_TRANSPARENT = 5 };

// Capacity bounds of the served paths -- "how far this was built", as opposed to the cases the reference itself has no engine for.  ONE definition: the entry points
// compare against these, mi355cv_limit() reports them, tests/test_declines_cpu.py pins their values on the CPU and the -m gpu tests derive every refusal they assert from
// mi355cv_limit(), so that widening a path without widening its parity cases fails a CPU test.
namespace lim {
constexpr int SEP_MAX_TAPS = 129;          // cv_hal_sepFilter: taps per axis (seplong.hip); a Gaussian of sigma 16 on CV_32F has 97
constexpr int SEP_MAX_TAPS_64F = 33;       // ... into CV_64F (k_sepfilter_generic64)
constexpr int GAUSS8U_MAX_KSIZE = 129;     // cv_hal_gaussianBlur on CV_8U (Q8.8 taps)
constexpr int GAUSS_FLOAT_MAX_KSIZE = 129; // cv_hal_gaussianBlur on CV_16U / CV_16S / CV_32F (= the separable hook's)
constexpr int ADAPTIVE_MEAN_MAX_BLOCK = 255;
constexpr int BOX_MAX_KSIZE = 255;
constexpr int MEDIAN8U_MAX_KSIZE = 31;
constexpr int BILATERAL_MAX_RADIUS = 16;
constexpr int ORB_MAX_LEVELS = 32;
constexpr int FILTER2D_DFT_TAPS = 130;     // whole-image filter2D from this many taps on is the reference's DFT case: declined unless MI355CV_FILTER_LARGE=1
constexpr int DISTTRANSFORM_MAX_DIM = 16384; // mi355cv_distanceTransform: width and height (16-bit column distances, 32-bit squared distances; disttransform_math.h)
constexpr int CCL_MAX_DIM = 16384;         // mi355cv_connectedComponents*: width and height (32-bit pixel indices and areas, coordinate sums below 2^53; ccl_math.h)
constexpr int HOUGH_MAX_DIM = 16384;       // mi355cv_houghLines*: width and height (packed 16-bit point coordinates, counts below 2^28; hough_math.h)
constexpr int HOUGH_MAX_ACCUM = 1 << 26;   // ... and the cells of the accumulator, (numangle + 2) x (numrho + 2): a cell index is the low word of the sort key
constexpr int HOUGHCIRCLES_MAX_DIM = 16384;   // mi355cv_houghCircles*: width and height (packed 16-bit point coordinates, counts below 2^28; houghcircles_math.h)
constexpr int HOUGHCIRCLES_MAX_ACCUM = 1 << 26; // ... the cells of the centre accumulator, (arows + 2) x (acols + 2): a cell index is the low word of the sort key
constexpr int HOUGHCIRCLES_MAX_RADIUS = 32768;  // ... the prepared maxRadius: x0 + r * sx of the fixed-point ray stays inside 31 bits
constexpr int HOUGHCIRCLES_MAX_CIRCLES = 65536; // ... max_circles: the kept list k_hc_suppress tests every candidate against
constexpr int HOUGHCIRCLES_LDS_BINS = 40960;    // ... geometry, reported for the tests' shapes: radius histograms up to this many bins live in LDS (160 KiB), longer ones in HBM
constexpr int HOUGHCIRCLES_TILE = 64;           // ... the side of the accumulator tile of k_hc_vote_tile (behind mi355cv_houghCirclesSetKernel(1) only: it won at no reach)
constexpr int MINMAX_MAX_DIM = 16384;      // mi355cv_minMaxLoc*: width and height (a raster pixel index below 2^28, item counts in 32 bits; minmax_math.h)
constexpr int DEMOSAIC_MAX_DIM = 16384;    // mi355cv_demosaic*: width and height (the neighbours' bound; a destination row offset of 8 bytes per pixel stays far below 2^31)
constexpr int CALCHIST_MAX_DIM = 16384;    // mi355cv_calcHist* / mi355cv_calcBackProject*: width and height (the neighbours' bound; a frame has at most 2^28 pixels, so no count of one call passes int32; calchist_math.h)
constexpr int CALCHIST_MAX_BINS = 1 << 20; // ... and the cells of the dense histogram, the product of histSize (each histSize also <= 65536): 4 MiB of counters per frame, a cell offset far from the table's SKIP mark
constexpr int MOG2_MAX_DIM = 16384;        // mi355cv_mog2*: width and height (the neighbours' bound; a pixel index and a plane of the model stay below 2^28 elements; mog2_math.h)
constexpr int MOG2_MAX_MIXTURES = 5;       // ... and the modes per pixel, held in registers with compile-time indices (the reference's default nmixtures)
constexpr int FARNEBACK_MAX_DIM = 16384;   // mi355cv_calcOpticalFlowFarneback* and its stages: width and height (the neighbours' bound; farneback_math.h)
constexpr int FARNEBACK_MAX_WINSIZE = 25;  // ... the averaging window: the M tile with its halo and the vertical sums of k_fb_update_flow fit 64 KiB of LDS
constexpr int FARNEBACK_MAX_POLY_N = 7;    // ... the half-width of the polynomial expansion: taps in the kernel arguments, LDS tiles sized for it
constexpr int FARNEBACK_MAX_SMOOTH_TAPS = 255; // ... the taps of a pyramid level's Gaussian, max(cvRound(5 sigma) | 1, 3) with sigma = (1 / scale - 1) / 2
constexpr int BFMATCH_MAX_ROWS = 1 << 24;      // mi355cv_bf*: rows per matrix and per train collection (the global train row is the low word of the 64-bit key; bfmatch_math.h)
constexpr int BFMATCH_MAX_K = 8;               // ... k of knnMatch: the list lives in registers with compile-time indices
constexpr int BFMATCH_MAX_ROW_BYTES = 2048;    // ... bytes per descriptor row (512 floats)
constexpr int BFMATCH_MAX_IMAGES = 64;         // ... train matrices per collection
constexpr int BFMATCH_MAX_RADIUS_ROW = 4096;   // ... matches of one query in radiusMatch: its keys are sorted in 32 KiB of LDS
constexpr int BFMATCH_TILE_ROWS = 256;         // ... geometry, reported for the tests' shapes: train rows per LDS tile of k_bf_hamming
constexpr int BFMATCH_SPLIT_ROWS = 512;        // ... and train rows per workgroup when the train set is split
constexpr int STEREOBM_MAX_DIM = 16384;        // mi355cv_stereoBM*: width and height (the neighbours' bound; a column fits the 16 bits the left-right key gives it; stereobm_math.h)
constexpr int STEREOBM_MAX_DISPARITIES = 256;  // ... numDisparities: a workgroup of the fast kernel is a wave per 16 disparities, 1024 lanes at most
constexpr int STEREOBM_MAX_BLOCK = 51;         // ... blockSize: the generic kernel's two tiles of blockSize rows and its SADs fit 64 KiB of LDS at 256 disparities
constexpr int STEREOBM_ROLL_MAX_BLOCK = 21;    // ... geometry, reported for the tests' shapes: the largest blockSize of the fast kernel (its SADs fit 16 bits)
constexpr int STEREOBM_CHUNK = 16;             // ... disparities per lane of the fast kernel
constexpr int STEREOBM_TILE_COLS = 64;         // ... window columns per workgroup of the fast kernel: 64 - (blockSize - 1) pixels of a row
constexpr int STEREOBM_STRIP_ROWS = 32;        // ... rows a workgroup of the fast kernel walks down
constexpr int STEREOBM_GENERIC_TILE_COLS = 32; // ... pixels of a row per workgroup of the generic kernel
constexpr int SPECKLE_MAX_DIM = 16384;         // mi355cv_filterSpeckles*: width and height (the neighbours' bound; a pixel index and a component size stay below 2^28; speckle_math.h)
constexpr int SPECKLE_TILE_COLS = 256;         // ... geometry, reported for the tests' shapes: columns of a tile of the fast kernel (64 lanes x 4 pixels)
constexpr int SPECKLE_TILE_ROWS = 16;          // ... and its rows, merged in LDS
constexpr int SGBM_MAX_DIM = 16384;            // mi355cv_stereoSGBM*: width and height (the neighbours' bound; a column fits the 16 bits the left-right key gives it; sgbm_math.h)
constexpr int SGBM_MAX_DISPARITIES = 256;      // ... numDisparities: four values per lane of a wave in the fast path kernel, a wave per 16 disparities in the cost kernel
constexpr int SGBM_MAX_COST = 32767;           // ... blockSize^2 * (2 ft + 63) + P2, ft = max(preFilterCap, 15) | 1: every block cost and path cost fits 16 bits
constexpr long long SGBM_MAX_SCRATCH_BYTES = 16384ll << 20; // ... the volumes of the frames in flight, 6 bytes per valid pixel and disparity (reported in MiB: "sgbm_max_scratch_mib")
constexpr int SGBM_TILE_COLS = 64;             // ... geometry, reported for the tests' shapes: window columns per workgroup of the cost kernel, 64 - (blockSize - 1) pixels of a row
constexpr int SGBM_STRIP_ROWS = 32;            // ... rows a workgroup of the cost kernel walks down
constexpr int SGBM_CHUNK = 16;                 // ... disparities per lane of the cost kernel
constexpr int SGBM_PATH_BLOCK = 16;            // ... steps of a path per block of loads in the fast path kernel up to 64 disparities (8 up to 128, 4 above)
constexpr int NLM_MAX_DIM = 16384;             // mi355cv_fastNlMeans*: width and height (the neighbours' bound; nlmeans_math.h)
constexpr int NLM_MAX_WINDOW = 181;            // ... templateWindowSize and searchWindowSize as used (odd): 181^2 <= 2^15, the reference's own bound on the patch; S * S * 255 stays far inside an int
constexpr int NLM_MAX_PIXEL_WORK = 1 << 24;      // ... S^2 T^2 cn, the squared differences per pixel of the rule as written: a lane of the plain kernel does them one after the other (7 / 21 on four channels: 86436)
constexpr int NLM_TILE_COLS = 128;             // ... geometry, reported for the tests' shapes: LANES across a workgroup of the tile kernel (two waves of 64), not output columns: a wave gives 64 - (T - 1) pixels of a row, a workgroup twice that
constexpr int NLM_TILE_ROWS = 32;              // ... and its rows, two waves of 16 rows each
constexpr int NLM_TILE_MAX_TEMPLATE = 9;       // ... the largest T of the tile kernel: the rows of a patch are a lane's registers with compile-time indices
constexpr int NLM_LDS_TABLE = 49152;           // ... entries of the weight table's non-zero prefix the tile kernel keeps in LDS: 96 KiB as 16-bit words (S >= 13), which holds the 39546 of h = 50 on three channels beside the tile
constexpr int NLM_TILE_LDS_KIB = 160;          // ... table and tile together: the LDS of a CU
constexpr int UNDIST_MAX_DIM = 16384;          // mi355cv_initUndistortRectifyMap / mi355cv_undistortRectify*: width and height of the destination (the neighbours' bound; a column and a row are exact doubles)
constexpr int UNDIST_MAX_SRC_DIM = 32767;      // ... and of the source: a map entry is 16 bits (mi355cv_remap's own bound)
constexpr int UNDIST_TILE_COLS = 128;          // ... geometry, reported for the tests' shapes: destination columns of a tile of k_undist8_tile (warp8.h)
constexpr int UNDIST_TILE_ROWS = 32;           // ... and its rows on one channel (16 on 3 / 4 channels)
constexpr int UNDIST_LDS_KIB = 24;             // ... the source tile's allotment: six workgroups of four waves a CU
constexpr int UNDIST_MAX_LDS_KIB = 48;         // ... the most mi355cv_undistortSetLds accepts (with the extremes' 64 bytes below the 64 KiB a launch gets unasked)
constexpr int UNDIST_FRAMES_PER_GROUP = 8;     // ... frames of a batch a workgroup walks with one evaluation of the rule
constexpr int UNDIST_MAX_FRAMES_PER_GROUP = 64; // ... the most mi355cv_undistortSetFramesPerGroup accepts
constexpr int REPROJECT_MAX_DIM = 16384;       // mi355cv_reprojectImageTo3D*: width and height (mi355cv_minMaxLoc's bound, which finds the frame's minimum)
}

struct ThreadCtx;
ThreadCtx& tctx();
hipStream_t stream();
hipStream_t auxStream();            // a second per-thread stream for work that may overlap the main one (ordered with events)
hipEvent_t pooledEvent(int i);      // per-thread reusable events (timing disabled), i < 64
bool asyncMode();
bool disabled();                    // MI355CV_DISABLE=1 -> every hook answers NOT_IMPLEMENTED
// Which host-resident images a hook accepts (device / managed pointers are always served).  MI355CV_MIN_PIXELS=<n>: images below n pixels
// are declined.  MI355CV_HOST_POLICY=auto (the default): a host image is staged through HBM only by hooks whose CPU path costs more than the two PCIe
// crossings (HOST_HEAVY: the reference's single-threaded FilterEngine paths -- filter2D, sepFilter2D, Sobel, box -- and medianBlur, Canny,
// corners, cubic / Lanczos / area resize, warps, LK, Otsu, bilateralFilter, float Lab / Luv, morphology with irregular elements or on deeper images); bandwidth-bound hooks whose CPU path is multi-threaded (HOST_CHEAP: 8U Gaussian,
// colour conversions, threshold, pyrDown, equalizeHist, morphology with CV_8U rectangles, integral, bilinear resize) decline and leave the image to the CPU.
// MI355CV_HOST_POLICY=always accepts everything, which is what the parity tests and the HAL tour set (tests/conftest.py).
enum HostCost { HOST_CHEAP = 0, HOST_HEAVY = 1 };
size_t minPixels(int cost = HOST_CHEAP);
// host-resident image below the policy threshold: true, and the reason is recorded for mi355cv_lastError / the decline ledger
bool hostImageTooSmall(const void* img, size_t pixels, size_t threshold);
int  setError(int code, const char* fmt, ...);
// a hook answers NOT_IMPLEMENTED: records WHY for mi355cv_lastError and the decline ledger (mi355cv_noteDecline) -- "<entry>:<line>: <the condition that held>" --
// unless a more specific reason was already recorded during this call (staging failure, host-policy threshold, foreign device ...).  Returns MI355CV_NOT_IMPLEMENTED.
// Call it through the macros below (next to MI355_CHECK_LAUNCH): MI355_DECLINE_IF(cond) where the condition is its own reason, `if (cond) return MI355_DECLINED("wording");`
// where a human wording says more than the expression.
int  declined(const char* fn, int line, const char* cond);
// first line of every extern "C" entry: the outermost entry on a thread starts a new call serial, so that a reason recorded by an EARLIER call that failed before it
// opened a Stager (argument checks, runSharded / replicate errors) is never reported as this call's; nested entries keep their caller's serial
// MI355CV_TRACE=1: the guard also opens a roctx range named after the entry (roctxRangePushA / roctxRangePop of librocprofiler-sdk-roctx.so or libroctx64.so, resolved with
// dlopen at the first traced call -- the library itself links HIP only), so that rocprofv3 --marker-trace / a timeline shows every cv_hal_* hook as a range around its
// kernels (the reference's CV_INSTRUMENT_REGION / CV_TRACE_REGION role, core/private.hpp:794; SURVEY section 5 tracing row).
struct EntryGuard { explicit EntryGuard(const char* name); ~EntryGuard(); EntryGuard(const EntryGuard&) = delete; EntryGuard& operator=(const EntryGuard&) = delete; bool traced_ = false; };
void beginCall();                   // start of a hook invocation (Stager's constructor): reasons recorded by earlier calls no longer count as this call's
void bump(const char* entry);       // per-entry completed-on-GPU counter
void noteKernel(const char* fmt, ...);   // name + launch geometry of the dominant kernel the calling thread launched last (mi355cv_lastKernel)
bool ensureDevice();                // makes the calling thread's device current (mi355cv_setDevice, else the process default); false if no usable GPU
int  activeDevice();                // ordinal of that device (per-device caches key on it)
int  threadDeviceBinding();         // what mi355cv_setDevice last set on the calling thread (-1: the process default)

// where an image lives: plain / page-locked host memory (staged through HBM), this thread's device or managed memory (launched in place),
// or ANOTHER GPU's memory (the hook declines: the thread is bound to the wrong device for that image)
enum PtrKind { PTR_HOST = 0, PTR_DEVICE = 1, PTR_FOREIGN = 2 };
int  ptrKind(const void* p);
void noteStagedBytes(long long n);                 // PCIe bytes moved outside Stager::in / out (pipelined host batches)
// true if p points into this device's or managed memory (launch in place)
bool isDevicePtr(const void* p);
// src and dst are the same buffer in HBM: a stencil cannot run in place on the GPU (host images are staged into separate buffers, so they may)
inline bool inPlaceOnDevice(const void* src, const void* dst) { return src == dst && src && isDevicePtr(src); }
// the general form for hooks that get no allowInplace argument (cv_hal_sepFilter, cv_hal_filter): the device-resident rows a stencil reads,
// [s, s + sbytes) -- the ROI plus the parent rows above / below it -- intersect the rows it writes.  FilterEngine is in-place safe on the CPU
// (ring buffer of rows); GPU threads would read neighbours other threads have already overwritten, so such a call is left to the CPU.
inline bool overlapOnDevice(const void* s, size_t sbytes, const void* d, size_t dbytes)
{
    const char* a = (const char*)s; const char* b = (const char*)d;
    if (!a || !b || a + sbytes <= b || b + dbytes <= a) return false;
    return isDevicePtr(s) && isDevicePtr(d);
}

// Stages host images into HBM scratch (and results back).  Device-resident
// images pass through untouched.  One Stager per hook invocation.
class Stager {
public:
    Stager();
    ~Stager();
    // input image: `rows` rows of `rowBytes` valid bytes at `p` with pitch `step`.
    const uchar* in(const uchar* p, size_t step, size_t rowBytes, int rows, size_t* dstep);
    // output image (contents undefined until the kernel writes them)
    uchar* out(uchar* p, size_t step, size_t rowBytes, int rows, size_t* dstep);
    // small parameter blocks (filter taps, tables): always copied, 256-B aligned
    void* param(const void* host, size_t bytes);
    // scratch in HBM that lives until finish()
    void* scratch(size_t bytes);
    // page-locked host memory that lives until the outermost hook returns (a per-thread pool, like the HBM scratch): the landing zone of results whose
    // size the GPU decides (candidate lists) -- a device-to-host copy into pageable memory goes through the runtime's own bounce buffer at a fraction of
    // the PCIe rate and blocks the host meanwhile
    void* pinned(size_t bytes);
    // copies staged outputs back and synchronises when required.  Returns HAL code.
    int finish(const char* entry);
    bool anyHost() const { return anyHost_; }
    bool failed() const { return failed_; }
private:
    struct Out { uchar* host; size_t hstep; uchar* dev; size_t dstep; size_t rowBytes; int rows; };
    std::vector<Out> outs_;
    bool anyHost_ = false, failed_ = false;
    void* bump_(size_t bytes);
    bool foreign_(const void* p);
};

// A batch of whole frames that lives in HOST memory (ingest / egress): the frames cross PCIe in chunks through two sets of device
// buffers -- the upload of chunk i+1 (aux stream) overlaps the kernels and the download of chunk i (main stream) -- and `run` is the entry's own
// device-resident batch path, called once per chunk with dense device frames.  Source and destination frames may differ in geometry and type.
struct HostBatch {
    const uchar* src; size_t sstep, sframe, srowBytes; int srows;       // source frames: pitch, frame stride, valid bytes per row, rows
    uchar* dst; size_t dstep, dframe, drowBytes; int drows;
    int nframes;
};
typedef std::function<int(const uchar* s, size_t sstep, size_t sframe, uchar* d, size_t dstep, size_t dframe, int nframes)> HostBatchFn;
// both ends are plain (pageable or page-locked) host memory: the batch entries take runHostBatch then
bool hostBatchEligible(const void* src, const void* dst, int nframes);
int runHostBatch(const char* entry, const HostBatch& hb, const HostBatchFn& run);

// The same pipeline for entries with several outputs per frame (cv::buildPyramid: one image per level): every output has its own geometry, the chunk
// size is what the largest of them allows.  `run` gets the chunk's dense device frames and one (pointer, pitch, frame stride) triple per output.
constexpr int HOST_BATCH_MAX_OUT = 32;
struct HostBatchOut { uchar* dst; size_t dstep, dframe, drowBytes; int drows; };
struct HostBatchN {
    const uchar* src; size_t sstep, sframe, srowBytes; int srows;
    int nout; HostBatchOut out[HOST_BATCH_MAX_OUT];
    int nframes;
};
typedef std::function<int(const uchar* s, size_t sstep, size_t sframe, uchar* const* d, const size_t* dstep, const size_t* dframe, int nframes)> HostBatchNFn;
int runHostBatchN(const char* entry, const HostBatchN& hb, const HostBatchNFn& run);

inline int depthBytes(int depth) { return depth <= 1 ? 1 : depth <= 3 ? 2 : depth <= 5 ? 4 : 8; }     // CV_8U .. CV_64F
inline int divUp(int a, int b) { return (a + b - 1) / b; }
inline int envInt(const char* name, int dflt) { const char* v = getenv(name); return v ? atoi(v) : dflt; }           // an A/B switch; `static const int x = envInt(...)` reads it once per process
inline size_t pad256(size_t b) { return (b + 255) & ~size_t(255); }                                                  // b bytes rounded up to 256: the start of the next array in a scratch block, a staged row's pitch
inline size_t span(size_t step, int rows, size_t rowBytes) { return (size_t)(rows - 1) * step + rowBytes; }          // bytes from the first byte of an image to one past its last

// grid.y and grid.z hold 65535 workgroups each, and most batch kernels take their frame from blockIdx.z (include/mi355cv.h, "Frame counts"): a longer batch of
// device-resident frames is served in slices of at most MAX_GRID_FRAMES frames -- run(f0, nf) is the entry's own path on frames [f0, f0 + nf) -- or declined by the
// entries that say so in their argument checks (MI355_DECLINE_IF(nframes > 65535)); no launch ever gets a grid dimension above 65535
constexpr int MAX_GRID_FRAMES = 65535;
template <class Run> inline int sliceFrames(int nframes, Run run)
{
    for (int f0 = 0; f0 < nframes; f0 += MAX_GRID_FRAMES) {
        const int rc = run((size_t)f0, nframes - f0 < MAX_GRID_FRAMES ? nframes - f0 : MAX_GRID_FRAMES);
        if (rc != MI355CV_OK) return rc;
    }
    return MI355CV_OK;
}

#if defined(__HIPCC__)
// Workgroups of a 1-D grid go to the 8 XCDs round-robin (id % 8), each XCD behind its own L2.  A kernel whose neighbouring workgroups write the two halves of
// the same 128-byte lines (rows whose pitch is not a multiple of the line: cv::integral's (W + 1)-element rows) sends every such line to memory twice as a
// partial write when the neighbours sit on different XCDs -- measured with tools/probes/fillbw2.hip: 3.1-3.9 TB/s for rows of 3841 ints against 6.5 TB/s
// when each XCD owns one contiguous run of workgroups.  This is that mapping: logical id = (id % 8) * (n / 8) + id / 8 (the last n % 8 ids keep their own).
__device__ __forceinline__ unsigned xcdContiguous(unsigned id, unsigned n)
{
    const unsigned per = n >> 3;
    return id < (per << 3) ? (id & 7u) * per + (id >> 3) : id;
}
#endif

#define MI355_CHECK_LAUNCH(entry)                                                        \
    do { hipError_t e__ = hipGetLastError();                                             \
         if (e__ != hipSuccess) return mi355::setError(MI355CV_ERROR_UNKNOWN, "%s: launch failed: %s", entry, hipGetErrorString(e__)); } while (0)

// the ONE way to decline: the reason is the condition's own source text, so the two cannot drift
#define MI355_DECLINED(why)   mi355::declined(__func__, __LINE__, why)
#define MI355_DECLINE_IF(...) do { if (__VA_ARGS__) return MI355_DECLINED(#__VA_ARGS__); } while (0)

// runResize / runWarp / runMatch try their served paths in order; a path answers NEXT_PATH for "not mine, try the next", anything else is the call's return code
constexpr int NEXT_PATH = -0x7fffffff;
static_assert(NEXT_PATH != MI355CV_OK && NEXT_PATH != MI355CV_NOT_IMPLEMENTED && NEXT_PATH != MI355CV_ERROR_UNKNOWN, "NEXT_PATH is none of the codes a hook answers");

#ifdef __HIPCC__
// (a << n) + b as ONE v_lshl_add_u32, and a + 4 b + 6 c on packed u16 pairs in four of them: written as plain C the optimiser folds the
// 4 c + 2 c into a 32-bit multiply by 6 (v_mul_lo_u32), which is not a full-rate instruction
__device__ __forceinline__ uint32_t lshlAdd(uint32_t a, int n, uint32_t b)
{
    uint32_t r;
    asm("v_lshl_add_u32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "n"(n), "v"(b));
    return r;
}
__device__ __forceinline__ uint32_t sum146(uint32_t a, uint32_t b, uint32_t c) { return lshlAdd(c, 1, lshlAdd(b + c, 2, a)); }
#endif
} // namespace mi355

// borderInterpolate (core/src/copy.cpp:748-793), device+host. Returns -1 for CONSTANT.
__host__ __device__ inline int mi355_borderInterpolate(int p, int len, int borderType)
{
    if ((unsigned)p < (unsigned)len) return p;
    if (borderType == mi355::B_REPLICATE) return p < 0 ? 0 : len - 1;
    if (borderType == mi355::B_REFLECT || borderType == mi355::B_REFLECT_101) {
        int delta = borderType == mi355::B_REFLECT_101;
        if (len == 1) return 0;
        do {
            if (p < 0) p = -p - 1 + delta;
            else p = len - 1 - (p - len) - delta;
        } while ((unsigned)p >= (unsigned)len);
        return p;
    }
    if (borderType == mi355::B_WRAP) {
        if (p < 0) p -= ((p - len + 1) / len) * len;
        if (p >= len) p %= len;
        return p;
    }
    return -1;
}
