// mi355cv_cv.hpp -- cv::-identical C++ signatures for the hot-path functions that have NO imgproc HAL hook
// (SURVEY.md §8b): cornerHarris, cornerMinEigenVal, goodFeaturesToTrack, buildPyramid, pyrUp, demosaicing, distanceTransform, connectedComponents,
// connectedComponentsWithStats, HoughLines, HoughCircles, minMaxLoc, calcHist, calcBackProject, matchTemplate -- and for the map
// representations of remap the HAL does not cover, convertMaps and warpPolar.  Header-only glue over
// the C ABI of mi355cv.h: each wrapper calls the fused MI355X entry point and falls back to the stock cv:: function when the
// library declines (unsupported arguments, no gfx950 device, MI355CV_DISABLE=1), exactly as a HAL hook returning
// CV_HAL_ERROR_NOT_IMPLEMENTED would.  A call site switches by replacing `cv::` with `mi355cv::`.
//
//   reference signatures: imgproc.hpp  cornerHarris :1925, cornerMinEigenVal :1895, goodFeaturesToTrack :2077 / :2106,
//                         buildPyramid :3308 (pyramids.cpp:1616), matchTemplate :3897 (templmatch.cpp:1158)
#pragma once
#include <climits>
#include <type_traits>
#include <vector>
#include "opencv2/core.hpp"
#include "opencv2/imgproc.hpp"
#include "mi355cv.h"

namespace mi355cv {

// cv::MatAllocator (core/mat.hpp:496-524) whose matrices live in memory the MI355X reaches without a pageable bounce:
//   FrameAllocator::Pinned   page-locked host memory -- a hook still stages the frame through HBM, but as one DMA at PCIe rate;
//   FrameAllocator::Managed  managed memory          -- hooks run on the matrix in place, CPU code keeps working on the same pointer;
//   FrameAllocator::Device   HBM (hipMalloc)         -- the matrix LIVES on the GPU: hooks run on it in place with no PCIe
//                            traffic at all, which is the regime the roofline numbers are quoted in.  The CPU must not dereference such a
//                            matrix: fill / read it with mi355cv::upload / mi355cv::download, and only hand it to cv:: functions whose hook
//                            serves the call (a call the library declines would fall back to CPU code on device memory).  Managed is the
//                            forgiving variant of the same thing.
// Install per matrix (`m.allocator = &alloc; m.create(...)`) or process-wide (`cv::Mat::setDefaultAllocator(&alloc)`, mat.hpp:2169).
// Without a gfx950 device the storage comes from cv::fastMalloc, so the same binary runs on a CPU-only host.
class FrameAllocator : public cv::MatAllocator
{
public:
    enum Kind { Pinned = 0, Managed = 1, Device = 2 };
    explicit FrameAllocator(Kind kind = Pinned) : kind_(kind) {}

    cv::UMatData* allocate(int dims, const int* sizes, int type, void* user, size_t* step, cv::AccessFlag, cv::UMatUsageFlags) const CV_OVERRIDE
    {
        size_t bytes = CV_ELEM_SIZE(type);                       // innermost dimension first: dense unless the caller brought its own steps
        for (int d = dims - 1; d >= 0; d--) {
            if (step) {
                if (user && step[d] != cv::Mat::AUTO_STEP) { CV_Assert(bytes <= step[d]); bytes = step[d]; }
                else step[d] = bytes;
            }
            bytes *= (size_t)sizes[d];
        }
        cv::UMatData* u = new cv::UMatData(this);
        u->size = bytes;
        if (user) { u->data = u->origdata = (uchar*)user; u->flags |= cv::UMatData::USER_ALLOCATED; return u; }
        void* p = kind_ == Device ? mi355cv_deviceAlloc(bytes) : mi355cv_hostAlloc(bytes, (int)kind_);
        u->userdata = p ? (void*)this : nullptr;                 // remembers which heap the block came from
        if (!p) p = cv::fastMalloc(bytes);
        u->data = u->origdata = (uchar*)p;
        return u;
    }
    bool allocate(cv::UMatData* u, cv::AccessFlag, cv::UMatUsageFlags) const CV_OVERRIDE { return u != nullptr; }
    void deallocate(cv::UMatData* u) const CV_OVERRIDE
    {
        if (!u) return;
        CV_Assert(u->urefcount == 0 && u->refcount == 0);
        if (!(u->flags & cv::UMatData::USER_ALLOCATED) && u->origdata) {
            if (!u->userdata) cv::fastFree(u->origdata);
            else if (kind_ == Device) mi355cv_deviceFree(u->origdata);
            else mi355cv_hostFree(u->origdata, (int)kind_);
            u->origdata = nullptr;
        }
        delete u;
    }
    Kind kind() const { return kind_; }
private:
    Kind kind_;
};

// host <-> device copies for matrices backed by FrameAllocator::Device (row by row when either side has padded rows); any other pair of
// matrices is copied with Mat::copyTo.  `dst` is created through its own allocator when it does not have the right geometry yet.
inline void upload(const cv::Mat& host, cv::Mat& dev)
{
    dev.create(host.rows, host.cols, host.type());
    const size_t row = (size_t)host.cols * host.elemSize();
    if (host.isContinuous() && dev.isContinuous()) { CV_Assert(mi355cv_upload(dev.data, host.data, row * host.rows) == 0); return; }
    for (int y = 0; y < host.rows; y++) CV_Assert(mi355cv_upload(dev.ptr(y), host.ptr(y), row) == 0);
}
inline void download(const cv::Mat& dev, cv::Mat& host)
{
    host.create(dev.rows, dev.cols, dev.type());
    const size_t row = (size_t)dev.cols * dev.elemSize();
    if (host.isContinuous() && dev.isContinuous()) { CV_Assert(mi355cv_download(host.data, dev.data, row * dev.rows) == 0); return; }
    for (int y = 0; y < dev.rows; y++) CV_Assert(mi355cv_download(host.ptr(y), dev.ptr(y), row) == 0);
}

// the stock functions read REAL parent pixels around a submatrix unless BORDER_ISOLATED is set (cornerEigenValsVecs runs Sobel / boxFilter on
// the view, corner.cpp:237; buildOpticalFlowPyramid's copyMakeBorder does the same, lkpyramid.cpp:747).  The fused entry points below get no
// margins and treat their input as a whole image, so such calls are left to cv::.
inline bool seesParent(const cv::Mat& m, int borderType) { return m.isSubmatrix() && !(borderType & cv::BORDER_ISOLATED); }

inline void cornerHarris(cv::InputArray _src, cv::OutputArray _dst, int blockSize, int ksize, double k, int borderType = cv::BORDER_DEFAULT)
{
    cv::Mat src = _src.getMat();
    if (src.dims <= 2 && (src.type() == CV_8UC1 || src.type() == CV_32FC1) && !seesParent(src, borderType)) {
        _dst.create(src.size(), CV_32FC1);
        cv::Mat dst = _dst.getMat();
        if (mi355cv_cornerHarris(src.data, src.step, dst.data, dst.step, src.cols, src.rows, src.type(), blockSize, ksize, k, borderType) == MI355CV_OK)
            return;
    }
    cv::cornerHarris(_src, _dst, blockSize, ksize, k, borderType);
}

inline void cornerMinEigenVal(cv::InputArray _src, cv::OutputArray _dst, int blockSize, int ksize = 3, int borderType = cv::BORDER_DEFAULT)
{
    cv::Mat src = _src.getMat();
    if (src.dims <= 2 && (src.type() == CV_8UC1 || src.type() == CV_32FC1) && !seesParent(src, borderType)) {
        _dst.create(src.size(), CV_32FC1);
        cv::Mat dst = _dst.getMat();
        if (mi355cv_cornerMinEigenVal(src.data, src.step, dst.data, dst.step, src.cols, src.rows, src.type(), blockSize, ksize, borderType) == MI355CV_OK)
            return;
    }
    cv::cornerMinEigenVal(_src, _dst, blockSize, ksize, borderType);
}

inline void goodFeaturesToTrack(cv::InputArray _image, cv::OutputArray _corners, int maxCorners, double qualityLevel, double minDistance,
                                cv::InputArray _mask = cv::noArray(), int blockSize = 3, int gradientSize = 3,
                                bool useHarrisDetector = false, double k = 0.04)
{
    cv::Mat image = _image.getMat(), mask = _mask.empty() ? cv::Mat() : _mask.getMat();
    const bool maskOk = mask.empty() || (mask.type() == CV_8UC1 && mask.size() == image.size());
    if (image.dims <= 2 && (image.type() == CV_8UC1 || image.type() == CV_32FC1) && maskOk && qualityLevel > 0 && minDistance >= 0 && maxCorners >= 0 &&
        !seesParent(image, cv::BORDER_DEFAULT)) {                          // featureselect.cpp:412-415 runs the corner measure with BORDER_DEFAULT
        // the entry point writes at most `cap` corners; with maxCorners <= 0 the reference returns every one it finds
        const int cap = maxCorners > 0 ? maxCorners : image.rows * image.cols;
        std::vector<cv::Point2f> pts((size_t)cap);
        const int n = mi355cv_goodFeaturesToTrack(image.data, image.step, image.cols, image.rows, image.type(),
                                                  cap ? reinterpret_cast<float*>(pts.data()) : nullptr, nullptr, maxCorners, qualityLevel, minDistance,
                                                  mask.empty() ? nullptr : mask.data, mask.empty() ? 0 : (size_t)mask.step,
                                                  blockSize, gradientSize, useHarrisDetector ? 1 : 0, k);
        if (n >= 0) {
            pts.resize((size_t)n);
            cv::Mat(pts).convertTo(_corners, _corners.fixedType() ? _corners.type() : CV_32F);      // featureselect.cpp:470
            return;
        }
    }
    cv::goodFeaturesToTrack(_image, _corners, maxCorners, qualityLevel, minDistance, _mask, blockSize, gradientSize, useHarrisDetector, k);
}

inline void buildPyramid(cv::InputArray _src, cv::OutputArrayOfArrays _dst, int maxlevel, int borderType = cv::BORDER_DEFAULT)
{
    cv::Mat src = _src.getMat();
    if (src.dims <= 2 && maxlevel >= 0 && maxlevel <= 30 && borderType != cv::BORDER_CONSTANT && !_dst.isUMatVector()) {
        _dst.create(maxlevel + 1, 1, 0);
        _dst.getMatRef(0) = src;                                          // level 0 is the source itself (pyramids.cpp:1634)
        std::vector<uchar*> ptr((size_t)maxlevel);
        std::vector<size_t> step((size_t)maxlevel);
        cv::Size sz = src.size();
        for (int i = 1; i <= maxlevel; i++) {
            sz = cv::Size((sz.width + 1) / 2, (sz.height + 1) / 2);
            _dst.create(sz, src.type(), i);
            cv::Mat& m = _dst.getMatRef(i);
            ptr[(size_t)i - 1] = m.data; step[(size_t)i - 1] = m.step;
        }
        if (maxlevel == 0 ||
            mi355cv_buildPyramid(src.data, src.step, src.cols, src.rows, src.depth(), src.channels(), ptr.data(), step.data(), maxlevel, borderType) == MI355CV_OK)
            return;
    }
    cv::buildPyramid(_src, _dst, maxlevel, borderType);
}

// cv::pyrUp (imgproc.hpp; pyramids.cpp): the default destination size 2w x 2h on the device; the 2w +- 1 / 2h +- 1 sizes the reference also admits, CV_64F
// and everything else the library declines go to the stock function.  When the destination is the source's own array, create() gives it a new buffer
// (the sizes differ) and `src` keeps the old one: both paths below therefore read `src`, not `_src`.
inline void pyrUp(cv::InputArray _src, cv::OutputArray _dst, const cv::Size& dstsize = cv::Size(), int borderType = cv::BORDER_DEFAULT)
{
    cv::Mat src = _src.getMat();
    const cv::Size dsz = dstsize.empty() ? cv::Size(src.cols * 2, src.rows * 2) : dstsize;
    if (src.dims <= 2 && !src.empty() && borderType == cv::BORDER_DEFAULT && dsz == cv::Size(src.cols * 2, src.rows * 2) && !_dst.isUMat()) {
        _dst.create(dsz, src.type());
        cv::Mat dst = _dst.getMat();
        if (mi355cv_pyrup(src.data, src.step, src.cols, src.rows, dst.data, dst.step, dst.cols, dst.rows, src.depth(), src.channels(), borderType) == MI355CV_OK)
            return;
    }
    cv::pyrUp(src, _dst, dstsize, borderType);
}

// cv::demosaicing (imgproc.hpp; demosaicing.cpp): the bilinear Bayer codes -- COLOR_BayerBG2BGR .. GR2BGR (46 .. 49, the ...2RGB names are the same codes with the
// B and R patterns exchanged), COLOR_Bayer..2GRAY (86 .. 89), COLOR_Bayer..2BGRA (139 .. 142) -- on CV_8UC1 / CV_16UC1 on the device; dstCn = 4 on a ...2BGR code
// gives the four-channel result.  The VNG (62 .. 65) and edge-aware (135 .. 138) codes, other types, images below 3 x 3 and everything else the library declines go
// to the stock function.  A cv::cvtColor call with a Bayer code ends in cv::demosaicing, so such call sites switch to this wrapper too.  Like mi355cv::pyrUp, this
// wrapper has not yet been compiled against the reference's headers.
inline void demosaicing(cv::InputArray _src, cv::OutputArray _dst, int code, int dstCn = 0)
{
    cv::Mat src = _src.getMat();
    int pattern = -1, dcn = 0;
    if (code >= 46 && code <= 49) { pattern = code - 46; dcn = dstCn > 0 ? dstCn : 3; }
    else if (code >= 86 && code <= 89) { pattern = code - 86; dcn = 1; }
    else if (code >= 139 && code <= 142) { pattern = code - 139; dcn = dstCn > 0 ? dstCn : 4; }
    if (pattern >= 0 && (dcn == 1 || dcn == 3 || dcn == 4) && src.dims <= 2 && src.channels() == 1 && src.cols >= 3 && src.rows >= 3 && !_dst.isUMat()) {
        // (when the destination is the source's own array, create() gives it a new buffer -- the types differ unless dcn == 1, and then the library declines the
        // overlap -- and `src` keeps the old one)
        _dst.create(src.size(), CV_MAKETYPE(src.depth(), dcn));
        cv::Mat dst = _dst.getMat();
        if (mi355cv_demosaic(src.data, src.step, dst.data, dst.step, src.cols, src.rows, src.depth(), dcn, pattern) == MI355CV_OK)
            return;
    }
    cv::demosaicing(src, _dst, code, dstCn);
}

// cv::distanceTransform (imgproc.hpp; distransform.cpp), the unlabelled overload: DIST_L2 with DIST_MASK_PRECISE, DIST_L1 and DIST_C on the device as the exact
// distance to the nearest zero pixel (mi355cv.h states where that is the reference's own result); DIST_L2 with a 3 x 3 / 5 x 5 mask, the other metrics and
// everything else the library declines go to the stock function.  A frame without any zero pixel gets the library's own value (31622776.0f / 255), not the
// reference's.  The source is cloned when the destination is its own array: the device passes cannot run in place.
inline void distanceTransform(cv::InputArray _src, cv::OutputArray _dst, int distanceType, int maskSize, int dstType = CV_32F)
{
    cv::Mat src = _src.getMat();
    if (src.dims <= 2 && !src.empty() && src.type() == CV_8UC1 && (dstType == CV_32F || (dstType == CV_8U && distanceType == cv::DIST_L1)) && !_dst.isUMat()) {
        if (_dst.kind() == cv::_InputArray::MAT && _dst.getMat().data == src.data) src = src.clone();
        _dst.create(src.size(), dstType);
        cv::Mat dst = _dst.getMat();
        if (mi355cv_distanceTransform(src.data, src.step, src.cols, src.rows, dst.data, dst.step, distanceType, maskSize, dst.depth()) == MI355CV_OK)
            return;
    }
    cv::distanceTransform(src, _dst, distanceType, maskSize, dstType);
}

// cv::connectedComponents / cv::connectedComponentsWithStats (imgproc.hpp; connectedcomponents.cpp), both overloads of each: the one without ccltype means
// CCL_DEFAULT.  CV_8UC1, connectivity 4 or 8, ltype CV_32S or CV_16U on the device (mi355cv.h states the numbering: by first pixel for connectivity 4 and for
// CCL_WU / CCL_SAUF, by first 2 x 2 block otherwise); everything the library declines -- CV_16U labels with more than 65535 components among it -- goes to the
// stock function.  A frame without background gets the library's own statistics row 0 (zeros, NaN centroid).  The source is cloned when the labels are its own
// array.  Like mi355cv::pyrUp, these wrappers have not yet been compiled against the reference's headers.
inline int connectedComponents(cv::InputArray _image, cv::OutputArray _labels, int connectivity, int ltype, int ccltype)
{
    cv::Mat image = _image.getMat();
    if (image.dims <= 2 && !image.empty() && image.type() == CV_8UC1 && (ltype == CV_32S || ltype == CV_16U) && !_labels.isUMat()) {
        if (_labels.kind() == cv::_InputArray::MAT && _labels.getMat().data == image.data) image = image.clone();
        _labels.create(image.size(), ltype);
        cv::Mat labels = _labels.getMat();
        int n = 0;
        if (mi355cv_connectedComponents(image.data, image.step, image.cols, image.rows, labels.data, labels.step, connectivity, ltype, ccltype, &n) == MI355CV_OK)
            return n;
    }
    return cv::connectedComponents(image, _labels, connectivity, ltype, ccltype);
}
inline int connectedComponents(cv::InputArray image, cv::OutputArray labels, int connectivity = 8, int ltype = CV_32S)
{
    return mi355cv::connectedComponents(image, labels, connectivity, ltype, cv::CCL_DEFAULT);
}

inline int connectedComponentsWithStats(cv::InputArray _image, cv::OutputArray _labels, cv::OutputArray _stats, cv::OutputArray _centroids, int connectivity, int ltype,
                                        int ccltype)
{
    cv::Mat image = _image.getMat();
    if (image.dims <= 2 && !image.empty() && image.type() == CV_8UC1 && (ltype == CV_32S || ltype == CV_16U) && !_labels.isUMat() && !_stats.isUMat() &&
        !_centroids.isUMat()) {
        if (_labels.kind() == cv::_InputArray::MAT && _labels.getMat().data == image.data) image = image.clone();
        _labels.create(image.size(), ltype);
        cv::Mat labels = _labels.getMat();
        int n = 0;
        if (mi355cv_connectedComponents(image.data, image.step, image.cols, image.rows, labels.data, labels.step, connectivity, ltype, ccltype, &n) == MI355CV_OK) {
            _stats.create(n, cv::CC_STAT_MAX, CV_32S);
            _centroids.create(n, 2, CV_64F);
            cv::Mat stats = _stats.getMat(), centroids = _centroids.getMat();
            if (mi355cv_connectedComponentsStats(labels.data, labels.step, labels.cols, labels.rows, ltype, n, stats.ptr<int>(), stats.step, centroids.ptr<double>(),
                                                 centroids.step) == MI355CV_OK)
                return n;
        }
    }
    return cv::connectedComponentsWithStats(image, _labels, _stats, _centroids, connectivity, ltype, ccltype);
}
inline int connectedComponentsWithStats(cv::InputArray image, cv::OutputArray labels, cv::OutputArray stats, cv::OutputArray centroids, int connectivity = 8,
                                        int ltype = CV_32S)
{
    return mi355cv::connectedComponentsWithStats(image, labels, stats, centroids, connectivity, ltype, cv::CCL_DEFAULT);
}

// cv::HoughLines (imgproc.hpp; hough.cpp HoughLinesStandard): the standard transform of a CV_8UC1 edge image on the device, Vec2f (rho, theta) or -- when `lines`
// is a Vec3f array, cv::HoughLinesWithAccumulator's form -- Vec3f (rho, theta, votes), ordered by votes.  A first call with room for 4096 lines; when the library
// reports more maxima, one more call with that capacity.  Everything the library declines (srn or stn != 0, the multi-scale variant, among it) goes to the stock
// function.  Like mi355cv::pyrUp, this wrapper has not yet been compiled against the reference's headers.
inline void HoughLines(cv::InputArray _image, cv::OutputArray _lines, double rho, double theta, int threshold, double srn = 0, double stn = 0, double min_theta = 0,
                       double max_theta = CV_PI)
{
    cv::Mat image = _image.getMat();
    const int type = _lines.fixedType() && _lines.type() == CV_32FC3 ? CV_32FC3 : CV_32FC2, cn = CV_MAT_CN(type);
    if (image.dims <= 2 && !image.empty() && image.type() == CV_8UC1 && !_lines.isUMat()) {
        int cap = 4096, n = 0;
        for (int pass = 0; pass < 2; pass++) {
            std::vector<float> buf((size_t)cap * cn);
            if (mi355cv_houghLines(image.data, image.step, image.cols, image.rows, buf.data(), cn, cap, rho, theta, threshold, srn, stn, min_theta, max_theta, &n) != MI355CV_OK)
                break;
            if (n <= cap) {
                if (n == 0) { _lines.release(); return; }
                cv::Mat(n, 1, type, buf.data()).copyTo(_lines);
                return;
            }
            cap = n;
        }
    }
    if (type == CV_32FC3) cv::HoughLinesWithAccumulator(image, _lines, rho, theta, threshold, srn, stn, min_theta, max_theta);
    else cv::HoughLines(image, _lines, rho, theta, threshold, srn, stn, min_theta, max_theta);
}

// cv::HoughCircles (imgproc.hpp; hough.cpp HoughCirclesGradient): the circle transform of a CV_8UC1 image on the device with method cv::HOUGH_GRADIENT, Vec3f
// (x, y, radius) or -- when `circles` is a Vec4f array -- Vec4f (x, y, radius, votes), strongest first.  A first call with room for 1024 circles; while the
// library reports a full list, one more call with twice the capacity.  The steps are this project's restatement of the reference's rule (mi355cv.h), the reference
// was not available to pin them.  Everything the library declines (cv::HOUGH_GRADIENT_ALT among it) goes to the stock function.  Like mi355cv::pyrUp, this wrapper
// has not yet been compiled against the reference's headers.
inline void HoughCircles(cv::InputArray _image, cv::OutputArray _circles, int method, double dp, double minDist, double param1 = 100, double param2 = 100,
                         int minRadius = 0, int maxRadius = 0)
{
    cv::Mat image = _image.getMat();
    const int type = _circles.fixedType() && _circles.type() == CV_32FC4 ? CV_32FC4 : CV_32FC3, cn = CV_MAT_CN(type);
    if (image.dims <= 2 && !image.empty() && image.type() == CV_8UC1 && !_circles.isUMat()) {
        const int top = mi355cv_limit("houghcircles_max_circles");
        for (int cap = 1024, n = 0; cap <= top; cap *= 2) {
            std::vector<float> buf((size_t)cap * cn);
            if (mi355cv_houghCircles(image.data, image.step, image.cols, image.rows, buf.data(), cn, cap, method, dp, minDist, param1, param2, minRadius, maxRadius, &n) !=
                MI355CV_OK)
                break;
            if (n < cap || cap == top) {
                if (n == 0) { _circles.release(); return; }
                cv::Mat(1, n, type, buf.data()).copyTo(_circles);
                return;
            }
        }
    }
    cv::HoughCircles(image, _circles, method, dp, minDist, param1, param2, minRadius, maxRadius);
}

// cv::minMaxLoc (core.hpp): one channel of CV_8U .. CV_64F with an optional CV_8UC1 mask; any output may be null.  NaN is never a candidate and an empty
// candidate set gives 0, 0, (-1, -1), (-1, -1) -- this project's restatement (mi355cv.h), the reference was not available to pin either.  Everything the library
// declines goes to the stock function.  Like mi355cv::pyrUp, this wrapper has not yet been compiled against the reference's headers.
inline void minMaxLoc(cv::InputArray _src, double* minVal, double* maxVal = 0, cv::Point* minLoc = 0, cv::Point* maxLoc = 0, cv::InputArray _mask = cv::noArray())
{
    cv::Mat src = _src.getMat(), mask = _mask.getMat();
    if (src.dims <= 2 && !src.empty() && src.channels() == 1 && !_src.isUMat() && (mask.empty() || (mask.type() == CV_8UC1 && mask.size() == src.size()))) {
        double vals[2];
        int locs[4];
        if (mi355cv_minMaxLoc(src.data, src.step, src.cols, src.rows, src.depth(), mask.empty() ? 0 : mask.data, mask.empty() ? 0 : (size_t)mask.step, vals, locs) == MI355CV_OK) {
            if (minVal) *minVal = vals[0];
            if (maxVal) *maxVal = vals[1];
            if (minLoc) *minLoc = cv::Point(locs[0], locs[1]);
            if (maxLoc) *maxLoc = cv::Point(locs[2], locs[3]);
            return;
        }
    }
    cv::minMaxLoc(_src, minVal, maxVal, minLoc, maxLoc, _mask);
}

// cv::calcHist (imgproc.hpp, the `const Mat* images, int nimages` form): ONE image (nimages == 1) of CV_8U / CV_16U / CV_32F with 1-4 channels, dims 1-3, a dense
// CV_32F histogram.  The bin rule is this project's restatement (mi355cv.h; the reference was not available to pin it).  Several images, other depths, SparseMat
// and everything the library declines go to the stock function.  Like mi355cv::minMaxLoc, not yet compiled against the reference's headers.
namespace detail {
// the ranges of the C ABI: 2 * dims floats when uniform, else the concatenated histSize[d] + 1 boundaries
inline bool flatRanges(const float** ranges, int dims, const int* histSize, bool uniform, std::vector<float>& out)
{
    if (!ranges || !histSize || dims < 1 || dims > 3) return false;
    for (int d = 0; d < dims; d++) {
        if (!ranges[d] || histSize[d] < 1) return false;
        out.insert(out.end(), ranges[d], ranges[d] + (uniform ? 2 : histSize[d] + 1));
    }
    return true;
}
} // namespace detail

inline void calcHist(const cv::Mat* images, int nimages, const int* channels, cv::InputArray _mask, cv::OutputArray _hist, int dims, const int* histSize,
                     const float** ranges, bool uniform = true, bool accumulate = false)
{
    std::vector<float> rg;
    cv::Mat mask = _mask.getMat();
    if (nimages == 1 && images && channels && images[0].dims <= 2 && !images[0].empty() && detail::flatRanges(ranges, dims, histSize, uniform, rg) &&
        (mask.empty() || (mask.type() == CV_8UC1 && mask.size() == images[0].size())) && !_hist.isUMat()) {
        const cv::Mat& src = images[0];
        cv::Mat hist;
        if (accumulate) hist = _hist.getMat();
        bool shaped = !hist.empty() && hist.type() == CV_32F && hist.isContinuous() && hist.dims == (dims == 1 ? 2 : dims);
        for (int d = 0; shaped && d < dims; d++) shaped = hist.size[d] == histSize[d];
        if (shaped && dims == 1) shaped = hist.size[1] == 1;
        if (!accumulate || shaped) {
            cv::Mat out = accumulate ? hist : cv::Mat(dims, histSize, CV_32F);
            if (mi355cv_calcHist(src.data, src.step, src.cols, src.rows, src.depth(), src.channels(), channels, dims, histSize, rg.data(), uniform ? 1 : 0,
                                 mask.empty() ? 0 : mask.data, mask.empty() ? 0 : (size_t)mask.step, out.data, CV_32F, accumulate ? 1 : 0) == MI355CV_OK) {
                if (!accumulate) out.copyTo(_hist);
                return;
            }
        }
    }
    cv::calcHist(images, nimages, channels, _mask, _hist, dims, histSize, ranges, uniform, accumulate);
}

// cv::calcBackProject: ONE image, a dense CV_32F histogram of 1-3 dimensions; the rest goes to the stock function.
// The signature carries no `dims`: it is taken from the histogram, and a cv::Mat has no one-dimensional form, so an n x 1 Mat is read as ONE dimension of n bins
// (what mi355cv::calcHist writes for dims == 1).  A genuinely two-dimensional histogram whose second size is 1 (two channels, histSize {n, 1}) cannot be told from
// it here and is read as one dimension too: its second channel's range test is then not made.  A caller that has one calls mi355cv_calcBackProject with dims = 2.
inline void calcBackProject(const cv::Mat* images, int nimages, const int* channels, cv::InputArray _hist, cv::OutputArray _backProject, const float** ranges,
                            double scale = 1, bool uniform = true)
{
    cv::Mat hist = _hist.getMat();
    int dims = hist.dims, hs[3] = {0, 0, 0};
    if (dims == 2 && hist.size[1] == 1) dims = 1;                            // a 1-D histogram is an n x 1 Mat
    std::vector<float> rg;
    if (nimages == 1 && images && channels && images[0].dims <= 2 && !images[0].empty() && !_hist.isUMat() && !_backProject.isUMat() && dims >= 1 && dims <= 3 &&
        hist.type() == CV_32F && hist.isContinuous()) {
        for (int d = 0; d < dims; d++) hs[d] = hist.size[d];
        const cv::Mat& src = images[0];
        if (detail::flatRanges(ranges, dims, hs, uniform, rg)) {
            cv::Mat dst(src.rows, src.cols, CV_MAKETYPE(src.depth(), 1));
            if (mi355cv_calcBackProject(src.data, src.step, src.cols, src.rows, src.depth(), src.channels(), channels, dims, hs, rg.data(), uniform ? 1 : 0,
                                        hist.ptr<float>(), scale, dst.data, dst.step) == MI355CV_OK) {
                dst.copyTo(_backProject);
                return;
            }
        }
    }
    cv::calcBackProject(images, nimages, channels, _hist, _backProject, ranges, scale, uniform);
}

inline void matchTemplate(cv::InputArray _image, cv::InputArray _templ, cv::OutputArray _result, int method, cv::InputArray _mask = cv::noArray())
{
    cv::Mat image = _image.getMat(), templ = _templ.getMat();
    if (_mask.empty() && image.dims <= 2 && image.type() == templ.type() && (image.depth() == CV_8U || image.depth() == CV_32F) &&
        image.cols >= templ.cols && image.rows >= templ.rows && method >= cv::TM_SQDIFF && method <= cv::TM_CCOEFF_NORMED) {
        _result.create(image.rows - templ.rows + 1, image.cols - templ.cols + 1, CV_32FC1);
        cv::Mat result = _result.getMat();
        if (mi355cv_matchTemplate(image.data, image.step, image.cols, image.rows, templ.data, templ.step, templ.cols, templ.rows, image.type(),
                                  result.data, result.step, method) == MI355CV_OK)
            return;
    }
    if (!_mask.empty() && image.dims <= 2 && image.type() == templ.type() && (image.depth() == CV_8U || image.depth() == CV_32F) &&
        image.cols >= templ.cols && image.rows >= templ.rows && method >= cv::TM_SQDIFF && method <= cv::TM_CCOEFF_NORMED) {
        cv::Mat mask = _mask.getMat();                                       // matchTemplateMask (templmatch.cpp:762)
        if (mask.dims <= 2 && mask.size() == templ.size() && (mask.depth() == CV_8U || mask.depth() == CV_32F) && (mask.channels() == 1 || mask.channels() == templ.channels())) {
            _result.create(image.rows - templ.rows + 1, image.cols - templ.cols + 1, CV_32FC1);
            cv::Mat result = _result.getMat();
            if (mi355cv_matchTemplateMask(image.data, image.step, image.cols, image.rows, templ.data, templ.step, templ.cols, templ.rows, image.type(),
                                          mask.data, mask.step, mask.type(), result.data, result.step, method) == MI355CV_OK)
                return;
        }
    }
    cv::matchTemplate(_image, _templ, _result, method, _mask);
}

// cv::remap (imgproc.hpp; imgwarp.cpp:1718).  The HAL only hooks the (CV_32FC1, CV_32FC1) pair of maps, which cv::remap already reaches; this wrapper
// adds the other representations -- one CV_32FC2 map and the fixed-point maps cv::convertMaps produces -- and hands everything else to cv::.
inline void remap(cv::InputArray _src, cv::OutputArray _dst, cv::InputArray _map1, cv::InputArray _map2, int interpolation,
                  int borderMode = cv::BORDER_CONSTANT, const cv::Scalar& borderValue = cv::Scalar())
{
    cv::Mat src = _src.getMat(), map1 = _map1.getMat(), map2 = _map2.empty() ? cv::Mat() : _map2.getMat();
    const bool pair32f = map1.type() == CV_32FC1 && map2.type() == CV_32FC1 && !map2.empty();
    if (!pair32f && src.dims <= 2 && !map1.empty() && (map2.empty() || map2.size() == map1.size()) && !_dst.isUMat() &&
        src.cols < SHRT_MAX && src.rows < SHRT_MAX && map1.cols < SHRT_MAX && map1.rows < SHRT_MAX) {
        _dst.create(map1.size(), src.type());
        cv::Mat dst = _dst.getMat();
        if (dst.data == src.data) src = src.clone();
        if (mi355cv_remap(src.type(), src.data, src.step, src.cols, src.rows, dst.data, dst.step, dst.cols, dst.rows, map1.data, map1.step, map1.type(),
                          map2.empty() ? nullptr : map2.data, map2.empty() ? 0 : (size_t)map2.step, map2.empty() ? 0 : map2.type(), interpolation,
                          borderMode, borderValue.val) == MI355CV_OK)
            return;
    }
    cv::remap(_src, _dst, _map1, _map2, interpolation, borderMode, borderValue);
}

// cv::convertMaps (imgwarp.cpp:1925): float maps <-> CV_16SC2 (+ CV_16UC1)
inline void convertMaps(cv::InputArray _map1, cv::InputArray _map2, cv::OutputArray _dstmap1, cv::OutputArray _dstmap2, int dstmap1type, bool nninterpolation = false)
{
    cv::Mat map1 = _map1.getMat(), map2 = _map2.empty() ? cv::Mat() : _map2.getMat();
    int dt = dstmap1type;
    if (dt <= 0) dt = map1.type() == CV_16SC2 ? CV_32FC2 : CV_16SC2;
    const bool toFixed = dt == CV_16SC2 && ((map1.type() == CV_32FC1 && map2.type() == CV_32FC1 && !map2.empty()) || (map1.type() == CV_32FC2 && map2.empty()));
    const bool toFloat = map1.type() == CV_16SC2 && (map2.empty() || map2.type() == CV_16UC1 || map2.type() == CV_16SC1) && (dt == CV_32FC1 || dt == CV_32FC2);
    if ((toFixed || toFloat) && map1.dims <= 2 && (map2.empty() || map2.size() == map1.size()) && !_dstmap1.isUMat()) {
        _dstmap1.create(map1.size(), dt);
        cv::Mat d1 = _dstmap1.getMat(), d2;
        const bool second = toFixed ? !nninterpolation : dt == CV_32FC1;
        if (second) { _dstmap2.create(map1.size(), toFixed ? CV_16UC1 : CV_32FC1); d2 = _dstmap2.getMat(); }
        else _dstmap2.release();
        if (mi355cv_convertMaps(map1.data, map1.step, map1.type(), map2.empty() ? nullptr : map2.data, map2.empty() ? 0 : (size_t)map2.step,
                                map2.empty() ? 0 : map2.type(), d1.data, d1.step, dt, second ? d2.data : nullptr, second ? (size_t)d2.step : 0,
                                map1.cols, map1.rows, nninterpolation ? 1 : 0) == MI355CV_OK)
            return;
    }
    cv::convertMaps(_map1, _map2, _dstmap1, _dstmap2, dstmap1type, nninterpolation);
}

// cv::warpPolar (imgwarp.cpp:3731): both directions run with the map evaluated inside the sampling kernel (WARP_INVERSE_MAP: the reference's float
// approximations of cartToPolar / log restated there); whatever the library declines goes to cv::warpPolar, whose own remap call is served by the
// remap32f hook.
inline void warpPolar(cv::InputArray _src, cv::OutputArray _dst, cv::Size dsize, cv::Point2f center, double maxRadius, int flags)
{
    cv::Mat src = _src.getMat();
    if (src.dims <= 2 && !_dst.isUMat() && src.cols < SHRT_MAX && src.rows < SHRT_MAX - 2) {
        if (dsize.width <= 0 && dsize.height <= 0) { dsize.width = cvRound(maxRadius); dsize.height = cvRound(maxRadius * CV_PI); }
        else if (dsize.height <= 0) dsize.height = cvRound(dsize.width * CV_PI);
        if (dsize.width > 0 && dsize.height > 0 && dsize.width < SHRT_MAX && dsize.height < SHRT_MAX) {
            _dst.create(dsize, src.type());
            cv::Mat dst = _dst.getMat();
            if (dst.data == src.data) src = src.clone();
            if (mi355cv_warpPolar(src.type(), src.data, src.step, src.cols, src.rows, dst.data, dst.step, dst.cols, dst.rows, center.x, center.y, maxRadius, flags) == MI355CV_OK)
                return;
        }
    }
    cv::warpPolar(_src, _dst, dsize, center, maxRadius, flags);
}

// cv::CLAHE (imgproc.hpp; CLAHE_Impl, clahe.cpp).  The reference has no HAL hook for it.  mi355cv::createCLAHE returns a cv::CLAHE whose apply sends a 2-D
// CV_8UC1 / CV_16UC1 cv::Mat through mi355cv_clahe -- tile histograms, clipping, LUTs and the blend on the device, bit-identical to cv::CLAHE, a submatrix's
// parent margins passed on for the padding rule -- and hands everything else (UMat, other types, calls the library declines, no device) to the stock object it
// wraps.  Parameters live in the stock object.
class CLAHE CV_FINAL : public cv::CLAHE
{
public:
    explicit CLAHE(const cv::Ptr<cv::CLAHE>& stock) : stock_(stock) {}
    void setClipLimit(double v) CV_OVERRIDE { stock_->setClipLimit(v); }                 double getClipLimit() const CV_OVERRIDE { return stock_->getClipLimit(); }
    void setTilesGridSize(cv::Size v) CV_OVERRIDE { stock_->setTilesGridSize(v); }       cv::Size getTilesGridSize() const CV_OVERRIDE { return stock_->getTilesGridSize(); }
    void collectGarbage() CV_OVERRIDE { stock_->collectGarbage(); }
    void clear() CV_OVERRIDE { stock_->clear(); }
    bool empty() const CV_OVERRIDE { return stock_->empty(); }
    void write(cv::FileStorage& fs) const CV_OVERRIDE { stock_->write(fs); }
    void read(const cv::FileNode& fn) CV_OVERRIDE { stock_->read(fn); }
    cv::String getDefaultName() const CV_OVERRIDE { return stock_->getDefaultName(); }

    void apply(cv::InputArray _src, cv::OutputArray _dst) CV_OVERRIDE
    {
        if (_src.kind() == cv::_InputArray::MAT && !_dst.isUMat()) {
            cv::Mat src = _src.getMat();
            const cv::Size grid = stock_->getTilesGridSize();
            if (src.dims <= 2 && (src.type() == CV_8UC1 || src.type() == CV_16UC1) && !src.empty() && grid.width > 0 && grid.height > 0) {
                cv::Size whole; cv::Point ofs;
                src.locateROI(whole, ofs);
                _dst.create(src.size(), src.type());
                cv::Mat dst = _dst.getMat();
                if (mi355cv_clahe(src.data, src.step, dst.data, dst.step, src.cols, src.rows, src.depth(), whole.width - ofs.x - src.cols,
                                  whole.height - ofs.y - src.rows, stock_->getClipLimit(), grid.width, grid.height) == MI355CV_OK)
                    return;
            }
        }
        stock_->apply(_src, _dst);
    }
private:
    cv::Ptr<cv::CLAHE> stock_;
};

inline cv::Ptr<cv::CLAHE> createCLAHE(double clipLimit = 40.0, cv::Size tileGridSize = cv::Size(8, 8))
{
    return cv::makePtr<mi355cv::CLAHE>(cv::createCLAHE(clipLimit, tileGridSize));
}

#ifdef OPENCV_FEATURES_2D_HPP   // cv::FAST lives in opencv2/features2d.hpp; include it before this header to get the wrapper
// cv::FAST (features2d.hpp; fast.cpp:496).  TYPE_9_16 runs as one call on the GPU at any threshold (cv::FAST's own HAL route, hal_FAST, only covers
// thresholds <= 20 and moves the score image over PCIe twice); everything else goes to the stock function.
inline void FAST(cv::InputArray _image, std::vector<cv::KeyPoint>& keypoints, int threshold, bool nonmaxSuppression = true,
                 cv::FastFeatureDetector::DetectorType type = cv::FastFeatureDetector::TYPE_9_16)
{
    cv::Mat image = _image.getMat();
    if (image.dims <= 2 && image.type() == CV_8UC1 && type == cv::FastFeatureDetector::TYPE_9_16 && !image.empty()) {
        std::vector<float> xyr(3 * 16384);
        for (;;) {
            const int cap = (int)(xyr.size() / 3);
            const int n = mi355cv_FAST(image.data, image.step, image.cols, image.rows, threshold, nonmaxSuppression ? 1 : 0, (int)type, xyr.data(), cap);
            if (n < 0) break;
            if (n > cap) { xyr.resize(3 * (size_t)n); continue; }
            keypoints.resize((size_t)n);
            for (int i = 0; i < n; i++) keypoints[(size_t)i] = cv::KeyPoint(xyr[3 * (size_t)i], xyr[3 * (size_t)i + 1], 7.f, -1, xyr[3 * (size_t)i + 2]);
            return;
        }
    }
    cv::FAST(_image, keypoints, threshold, nonmaxSuppression, type);
}

// cv::ORB (features2d.hpp:425-520; ORB_Impl, orb.cpp:655-1265).  The reference has no HAL hook for ORB: behind the imgproc / features2d hooks alone
// every pyramid level's resize, FAST and blur would cross PCIe on its own.  mi355cv::ORB_create returns a cv::ORB whose detectAndCompute sends a
// CV_8UC1 cv::Mat (and mask) through mi355cv_ORB_detectAndCompute -- one upload, pyramid / FAST / Harris / angles / smoothing / descriptors on the
// device, keypoints and descriptors identical to cv::ORB's, order included -- and hands everything else (UMat, colour images, parameters the library
// declines, no device) to the stock implementation it wraps.  Parameters live in the stock object, so getters / setters / write() behave as before.
class ORB CV_FINAL : public cv::ORB
{
public:
    explicit ORB(const cv::Ptr<cv::ORB>& stock) : stock_(stock) {}
    void setMaxFeatures(int v) CV_OVERRIDE { stock_->setMaxFeatures(v); }            int getMaxFeatures() const CV_OVERRIDE { return stock_->getMaxFeatures(); }
    void setScaleFactor(double v) CV_OVERRIDE { stock_->setScaleFactor(v); }          double getScaleFactor() const CV_OVERRIDE { return stock_->getScaleFactor(); }
    void setNLevels(int v) CV_OVERRIDE { stock_->setNLevels(v); }                     int getNLevels() const CV_OVERRIDE { return stock_->getNLevels(); }
    void setEdgeThreshold(int v) CV_OVERRIDE { stock_->setEdgeThreshold(v); }         int getEdgeThreshold() const CV_OVERRIDE { return stock_->getEdgeThreshold(); }
    void setFirstLevel(int v) CV_OVERRIDE { stock_->setFirstLevel(v); }               int getFirstLevel() const CV_OVERRIDE { return stock_->getFirstLevel(); }
    void setWTA_K(int v) CV_OVERRIDE { stock_->setWTA_K(v); }                         int getWTA_K() const CV_OVERRIDE { return stock_->getWTA_K(); }
    void setScoreType(cv::ORB::ScoreType v) CV_OVERRIDE { stock_->setScoreType(v); }  cv::ORB::ScoreType getScoreType() const CV_OVERRIDE { return stock_->getScoreType(); }
    void setPatchSize(int v) CV_OVERRIDE { stock_->setPatchSize(v); }                 int getPatchSize() const CV_OVERRIDE { return stock_->getPatchSize(); }
    void setFastThreshold(int v) CV_OVERRIDE { stock_->setFastThreshold(v); }         int getFastThreshold() const CV_OVERRIDE { return stock_->getFastThreshold(); }
    int descriptorSize() const CV_OVERRIDE { return stock_->descriptorSize(); }
    int descriptorType() const CV_OVERRIDE { return stock_->descriptorType(); }
    int defaultNorm() const CV_OVERRIDE { return stock_->defaultNorm(); }
    bool empty() const CV_OVERRIDE { return stock_->empty(); }
    void write(cv::FileStorage& fs) const CV_OVERRIDE { stock_->write(fs); }          // the parameters live in the stock object: so does their serialisation (orb.cpp:723-760)
    void read(const cv::FileNode& fn) CV_OVERRIDE { stock_->read(fn); }

    void detectAndCompute(cv::InputArray _image, cv::InputArray _mask, std::vector<cv::KeyPoint>& keypoints, cv::OutputArray _descriptors,
                          bool useProvidedKeypoints = false) CV_OVERRIDE
    {
        const bool doDesc = _descriptors.needed();
        if ((_image.kind() == cv::_InputArray::MAT) && (_mask.empty() || _mask.kind() == cv::_InputArray::MAT) && !_descriptors.isUMat() &&
            (doDesc || !useProvidedKeypoints)) {
            cv::Mat image = _image.getMat(), mask = _mask.getMat();
            const double sf = stock_->getScaleFactor();           // the double the stock object keeps (from create's float or from setScaleFactor)
            if (image.dims <= 2 && image.type() == CV_8UC1 && !image.empty() && (mask.empty() || (mask.type() == CV_8UC1 && mask.size() == image.size()))) {
                static_assert(sizeof(cv::KeyPoint) == sizeof(mi355cv_KeyPoint), "cv::KeyPoint is the 28-byte record mi355cv_KeyPoint declares");
                const mi355cv_OrbParams prm = {stock_->getMaxFeatures(), sf, stock_->getNLevels(), stock_->getEdgeThreshold(), stock_->getFirstLevel(), stock_->getWTA_K(),
                                               (int)stock_->getScoreType(), stock_->getPatchSize(), stock_->getFastThreshold()};
                std::vector<cv::KeyPoint> kp(keypoints);
                const int nIn = useProvidedKeypoints ? (int)kp.size() : 0;
                size_t cap = std::max<size_t>((size_t)nIn, (size_t)std::max(prm.nfeatures, 0) + 64);
                for (;;) {
                    kp.resize(cap);
                    cv::Mat desc;
                    if (doDesc) desc.create((int)cap, 32, CV_8U);
                    const int n = mi355cv_ORB_detectAndCompute(image.data, image.step, image.cols, image.rows, mask.empty() ? nullptr : mask.data, mask.empty() ? 0 : (size_t)mask.step, &prm,
                                                               useProvidedKeypoints ? 1 : 0, reinterpret_cast<mi355cv_KeyPoint*>(kp.data()), nIn, (int)cap,
                                                               doDesc ? desc.data : nullptr, doDesc ? (size_t)desc.step : 0);
                    if (n < 0) break;                                             // declined or failed: nothing was written to the caller's arrays
                    if ((size_t)n > cap) { cap = (size_t)n; if (useProvidedKeypoints) break; kp.assign(keypoints.begin(), keypoints.end()); continue; }
                    kp.resize((size_t)n);
                    keypoints.swap(kp);
                    if (doDesc) { if (n == 0) _descriptors.release(); else desc.rowRange(0, n).copyTo(_descriptors); }
                    return;
                }
            }
        }
        stock_->detectAndCompute(_image, _mask, keypoints, _descriptors, useProvidedKeypoints);
    }
    // Feature2D::detect / compute (feature2d.cpp:61-155) call detectAndCompute of *this
private:
    cv::Ptr<cv::ORB> stock_;
};

inline cv::Ptr<cv::ORB> ORB_create(int nfeatures = 500, float scaleFactor = 1.2f, int nlevels = 8, int edgeThreshold = 31, int firstLevel = 0, int WTA_K = 2,
                                   cv::ORB::ScoreType scoreType = cv::ORB::HARRIS_SCORE, int patchSize = 31, int fastThreshold = 20)
{
    return cv::makePtr<mi355cv::ORB>(cv::ORB::create(nfeatures, scaleFactor, nlevels, edgeThreshold, firstLevel, WTA_K, scoreType, patchSize, fastThreshold));
}

// cv::BFMatcher (features2d.hpp; matchers.cpp).  The reference has no HAL hook for matching.  mi355cv::BFMatcher is a cv::BFMatcher whose knnMatchImpl / radiusMatchImpl
// (what match / knnMatch / radiusMatch of DescriptorMatcher end in, with an explicit train matrix or the add()-ed collection) send cv::Mat descriptors through
// mi355cv_bfKnnMatch / mi355cv_bfRadiusMatch and hand everything the library declines (UMat, other types or norms, crossCheck with masks or several train matrices, no
// device) to the stock implementation.  The order the library serves -- (distance, imgIdx, trainIdx), DESIGN 6.16 -- fully determines every list; where the stock
// implementation orders equal distances otherwise the two differ in exactly those places.  Written against the reference's declarations as recollected: the reference's
// headers are not in this tree, so this class has not been compiled here.
class BFMatcher CV_FINAL : public cv::BFMatcher
{
public:
    explicit BFMatcher(int normType_ = cv::NORM_L2, bool crossCheck_ = false) : cv::BFMatcher(normType_, crossCheck_) {}
    static cv::Ptr<mi355cv::BFMatcher> create(int normType_ = cv::NORM_L2, bool crossCheck_ = false) { return cv::makePtr<mi355cv::BFMatcher>(normType_, crossCheck_); }

protected:
    struct Lists { std::vector<const void*> t, m; std::vector<size_t> tstep, mstep; std::vector<int> rows; bool ok = true; bool anyMask = false; };
    Lists gather(const cv::Mat& query, cv::InputArrayOfArrays _masks) const
    {
        Lists l;
        std::vector<cv::Mat> masks;
        if (!_masks.empty()) _masks.getMatVector(masks);
        if (!masks.empty() && masks.size() != trainDescCollection.size()) { l.ok = false; return l; }
        for (size_t i = 0; i < trainDescCollection.size(); i++) {
            const cv::Mat& t = trainDescCollection[i];
            if (t.dims > 2 || (!t.empty() && (t.type() != query.type() || t.cols != query.cols))) { l.ok = false; return l; }
            l.t.push_back(t.data); l.tstep.push_back(t.empty() ? 0 : (size_t)t.step); l.rows.push_back(t.rows);
            const bool has = !masks.empty() && !masks[i].empty();
            if (has && (masks[i].type() != CV_8UC1 || masks[i].rows != query.rows || masks[i].cols != t.rows)) { l.ok = false; return l; }
            l.m.push_back(has ? masks[i].data : nullptr); l.mstep.push_back(has ? (size_t)masks[i].step : 0);
            l.anyMask = l.anyMask || has;
        }
        if (!utrainDescCollection.empty() || trainDescCollection.empty()) l.ok = false;
        return l;
    }

    void knnMatchImpl(cv::InputArray _query, std::vector<std::vector<cv::DMatch> >& matches, int k, cv::InputArrayOfArrays _masks = cv::noArray(),
                      bool compactResult = false) CV_OVERRIDE
    {
        static_assert(sizeof(cv::DMatch) == sizeof(mi355cv_DMatch), "cv::DMatch is the 16-byte record mi355cv_DMatch declares");
        if (_query.kind() == cv::_InputArray::MAT && k >= 1) {
            const cv::Mat query = _query.getMat();
            const Lists l = gather(query, _masks);
            if (l.ok && query.dims <= 2 && !query.empty() && query.channels() == 1) {
                std::vector<cv::DMatch> plane((size_t)query.rows * k);
                std::vector<int> counts(query.rows);
                if (mi355cv_bfKnnMatch(query.data, query.step, query.rows, query.cols, query.type(), l.t.data(), l.tstep.data(), l.rows.data(), l.anyMask ? l.m.data() : nullptr,
                                       l.mstep.data(), (int)l.t.size(), normType, k, crossCheck ? 1 : 0, reinterpret_cast<mi355cv_DMatch*>(plane.data()), counts.data()) == MI355CV_OK) {
                    matches.clear();
                    for (int q = 0; q < query.rows; q++) {
                        if (compactResult && !counts[q]) continue;
                        matches.emplace_back(plane.begin() + (size_t)q * k, plane.begin() + (size_t)q * k + counts[q]);
                    }
                    return;
                }
            }
        }
        cv::BFMatcher::knnMatchImpl(_query, matches, k, _masks, compactResult);
    }

    void radiusMatchImpl(cv::InputArray _query, std::vector<std::vector<cv::DMatch> >& matches, float maxDistance, cv::InputArrayOfArrays _masks = cv::noArray(),
                         bool compactResult = false) CV_OVERRIDE
    {
        if (_query.kind() == cv::_InputArray::MAT && !crossCheck) {
            const cv::Mat query = _query.getMat();
            const Lists l = gather(query, _masks);
            if (l.ok && query.dims <= 2 && !query.empty() && query.channels() == 1) {
                std::vector<cv::DMatch> flat(std::max<size_t>(1024, 4 * (size_t)query.rows));
                std::vector<int> counts(query.rows);
                for (;;) {
                    const int n = mi355cv_bfRadiusMatch(query.data, query.step, query.rows, query.cols, query.type(), l.t.data(), l.tstep.data(), l.rows.data(),
                                                        l.anyMask ? l.m.data() : nullptr, l.mstep.data(), (int)l.t.size(), normType, maxDistance,
                                                        reinterpret_cast<mi355cv_DMatch*>(flat.data()), (int)flat.size(), counts.data());
                    if (n < 0) break;                                             // declined or failed: the stock implementation below
                    if ((size_t)n > flat.size()) { flat.resize((size_t)n); continue; }
                    matches.clear();
                    size_t at = 0;
                    for (int q = 0; q < query.rows; q++) {
                        if (!compactResult || counts[q]) matches.emplace_back(flat.begin() + at, flat.begin() + at + counts[q]);
                        at += (size_t)counts[q];
                    }
                    return;
                }
            }
        }
        cv::BFMatcher::radiusMatchImpl(_query, matches, maxDistance, _masks, compactResult);
    }
};
#endif

#ifdef OPENCV_TRACKING_HPP      // cv::calcOpticalFlowPyrLK lives in opencv2/video/tracking.hpp; include it before this header to get the wrapper
// cv::calcOpticalFlowPyrLK (video/tracking.hpp; lkpyramid.cpp:1432).  Two images (not precomputed pyramids) go through the one-call
// entry point -- frames cross PCIe once, pyramids, derivatives and all levels run on the device, results bit-identical to cv:: --
// everything else (pyramid vectors, UMat, unsupported arguments, no device) is handed to the stock function.
inline void calcOpticalFlowPyrLK(cv::InputArray _prevImg, cv::InputArray _nextImg, cv::InputArray _prevPts, cv::InputOutputArray _nextPts,
                                 cv::OutputArray _status, cv::OutputArray _err, cv::Size winSize = cv::Size(21, 21), int maxLevel = 3,
                                 cv::TermCriteria criteria = cv::TermCriteria(cv::TermCriteria::COUNT + cv::TermCriteria::EPS, 30, 0.01),
                                 int flags = 0, double minEigThreshold = 1e-4)
{
    if (_prevImg.kind() == cv::_InputArray::MAT && _nextImg.kind() == cv::_InputArray::MAT) {
        cv::Mat prev = _prevImg.getMat(), next = _nextImg.getMat(), pts = _prevPts.getMat();
        const int n = pts.checkVector(2, CV_32F, true);
        const bool initial = (flags & cv::OPTFLOW_USE_INITIAL_FLOW) != 0;
        if (prev.dims <= 2 && prev.depth() == CV_8U && prev.type() == next.type() && prev.size() == next.size() && n > 0 && maxLevel >= 0 &&
            winSize.width > 2 && winSize.height > 2 && !prev.isSubmatrix() && !next.isSubmatrix()) {
            if (!initial) _nextPts.create(pts.size(), pts.type(), -1, true);
            cv::Mat nextPts = _nextPts.getMat();
            if (nextPts.checkVector(2, CV_32F, true) == n) {
                _status.create(n, 1, CV_8U, -1, true);
                cv::Mat status = _status.getMat(), err;
                if (_err.needed()) { _err.create(n, 1, CV_32F, -1, true); err = _err.getMat(); }
                // the entry point writes its outputs only when it succeeds; an initial guess it might clobber is kept aside for the fallback
                cv::Mat guess = initial ? nextPts.clone() : cv::Mat();
                if (status.isContinuous() && (err.empty() || err.isContinuous()) &&
                    mi355cv_calcOpticalFlowPyrLK(prev.data, prev.step, next.data, next.step, prev.cols, prev.rows, prev.channels(), pts.ptr<float>(),
                                                 nextPts.ptr<float>(), n, status.data, err.empty() ? nullptr : err.ptr<float>(), winSize.width, winSize.height,
                                                 maxLevel, criteria.type, criteria.maxCount, criteria.epsilon, flags, minEigThreshold) == MI355CV_OK)
                    return;
                if (initial) guess.copyTo(nextPts);
            }
        }
    }
    cv::calcOpticalFlowPyrLK(_prevImg, _nextImg, _prevPts, _nextPts, _status, _err, winSize, maxLevel, criteria, flags, minEigThreshold);
}

// cv::calcOpticalFlowFarneback (video/tracking.hpp; optflowgf.cpp).  The reference has no HAL hook for it.  Two CV_8UC1 Mats go through mi355cv_calcOpticalFlowFarneback
// (csrc/farneback.hip): the frames and the flow live where the Mats live.  The entry computes the project's float32 restatement of the algorithm, which is not
// bit-identical to cv::; everything it declines (other types, sizes and windows over the limits, OPTFLOW_USE_INITIAL_FLOW with more than one pyramid level, UMat, no
// device) is handed to the stock function.
inline void calcOpticalFlowFarneback(cv::InputArray _prev, cv::InputArray _next, cv::InputOutputArray _flow, double pyr_scale, int levels, int winsize, int iterations,
                                     int poly_n, double poly_sigma, int flags)
{
    if (_prev.kind() == cv::_InputArray::MAT && _next.kind() == cv::_InputArray::MAT && _flow.kind() == cv::_InputArray::MAT) {
        cv::Mat prev = _prev.getMat(), next = _next.getMat();
        if (prev.dims <= 2 && prev.type() == CV_8UC1 && next.type() == CV_8UC1 && prev.size() == next.size() && !prev.empty()) {
            // the stock function creates the flow itself unless it carries the initial flow; the entry writes it only when it succeeds
            if (!(flags & cv::OPTFLOW_USE_INITIAL_FLOW)) _flow.create(prev.size(), CV_32FC2);
            cv::Mat flow = _flow.getMat();
            if (flow.size() == prev.size() && flow.type() == CV_32FC2 &&
                mi355cv_calcOpticalFlowFarneback(prev.data, prev.step, next.data, next.step, flow.data, flow.step, prev.cols, prev.rows, pyr_scale, levels, winsize,
                                                 iterations, poly_n, poly_sigma, flags) == MI355CV_OK)
                return;
        }
    }
    cv::calcOpticalFlowFarneback(_prev, _next, _flow, pyr_scale, levels, winsize, iterations, poly_n, poly_sigma, flags);
}
#endif

#ifdef OPENCV_BACKGROUND_SEGM_HPP   // cv::BackgroundSubtractorMOG2 lives in opencv2/video/background_segm.hpp; include it before this header to get the wrapper
// cv::BackgroundSubtractorMOG2 (video/background_segm.hpp; bgfg_gaussmix2.cpp).  The reference has no HAL hook for it.  mi355cv::createBackgroundSubtractorMOG2
// returns a cv::BackgroundSubtractorMOG2 that wraps the stock object and a mi355cv_mog2* handle: parameters live in the stock object and every setter forwards to the
// handle; apply sends a 2-D CV_8UC1 / CV_8UC3 / CV_32FC1 / CV_32FC3 cv::Mat through mi355cv_mog2Apply, the model staying in HBM.  When the entry declines the VERY FIRST
// frame (another type, UMat, no device, the host policy) the stock object takes over for good, with its own model; a decline after frames were served is an error,
// since the two models cannot be merged.
class BackgroundSubtractorMOG2 CV_FINAL : public cv::BackgroundSubtractorMOG2
{
public:
    explicit BackgroundSubtractorMOG2(const cv::Ptr<cv::BackgroundSubtractorMOG2>& stock) : stock_(stock)
    {
        if (mi355cv_mog2Create(&ctx_, stock_->getHistory(), stock_->getVarThreshold(), stock_->getDetectShadows() ? 1 : 0) != MI355CV_OK) ctx_ = nullptr;
        // the stock object's other defaults, kept in step from the start
        static const char* const names[] = {"nmixtures", "backgroundRatio", "varThresholdGen", "varInit", "varMin", "varMax", "complexityReductionThreshold", "shadowValue",
                                            "shadowThreshold"};
        const double values[] = {(double)stock_->getNMixtures(), stock_->getBackgroundRatio(), stock_->getVarThresholdGen(), stock_->getVarInit(), stock_->getVarMin(),
                                 stock_->getVarMax(), stock_->getComplexityReductionThreshold(), (double)stock_->getShadowValue(), stock_->getShadowThreshold()};
        for (int i = 0; ctx_ && i < 9; i++) forward(names[i], values[i]);
    }
    ~BackgroundSubtractorMOG2() CV_OVERRIDE { if (ctx_) mi355cv_mog2Free(ctx_); }
    BackgroundSubtractorMOG2(const BackgroundSubtractorMOG2&) = delete;
    BackgroundSubtractorMOG2& operator=(const BackgroundSubtractorMOG2&) = delete;

    int getHistory() const CV_OVERRIDE { return stock_->getHistory(); }                           void setHistory(int v) CV_OVERRIDE { stock_->setHistory(v); forward("history", v); }
    int getNMixtures() const CV_OVERRIDE { return stock_->getNMixtures(); }                       void setNMixtures(int v) CV_OVERRIDE { stock_->setNMixtures(v); forward("nmixtures", v); }
    double getBackgroundRatio() const CV_OVERRIDE { return stock_->getBackgroundRatio(); }        void setBackgroundRatio(double v) CV_OVERRIDE { stock_->setBackgroundRatio(v); forward("backgroundRatio", v); }
    double getVarThreshold() const CV_OVERRIDE { return stock_->getVarThreshold(); }              void setVarThreshold(double v) CV_OVERRIDE { stock_->setVarThreshold(v); forward("varThreshold", v); }
    double getVarThresholdGen() const CV_OVERRIDE { return stock_->getVarThresholdGen(); }        void setVarThresholdGen(double v) CV_OVERRIDE { stock_->setVarThresholdGen(v); forward("varThresholdGen", v); }
    double getVarInit() const CV_OVERRIDE { return stock_->getVarInit(); }                        void setVarInit(double v) CV_OVERRIDE { stock_->setVarInit(v); forward("varInit", v); }
    double getVarMin() const CV_OVERRIDE { return stock_->getVarMin(); }                          void setVarMin(double v) CV_OVERRIDE { stock_->setVarMin(v); forward("varMin", v); }
    double getVarMax() const CV_OVERRIDE { return stock_->getVarMax(); }                          void setVarMax(double v) CV_OVERRIDE { stock_->setVarMax(v); forward("varMax", v); }
    double getComplexityReductionThreshold() const CV_OVERRIDE { return stock_->getComplexityReductionThreshold(); }
    void setComplexityReductionThreshold(double v) CV_OVERRIDE { stock_->setComplexityReductionThreshold(v); forward("complexityReductionThreshold", v); }
    bool getDetectShadows() const CV_OVERRIDE { return stock_->getDetectShadows(); }              void setDetectShadows(bool v) CV_OVERRIDE { stock_->setDetectShadows(v); forward("detectShadows", v ? 1 : 0); }
    int getShadowValue() const CV_OVERRIDE { return stock_->getShadowValue(); }                   void setShadowValue(int v) CV_OVERRIDE { stock_->setShadowValue(v); forward("shadowValue", v); }
    double getShadowThreshold() const CV_OVERRIDE { return stock_->getShadowThreshold(); }        void setShadowThreshold(double v) CV_OVERRIDE { stock_->setShadowThreshold(v); forward("shadowThreshold", v); }
    void clear() CV_OVERRIDE { stock_->clear(); }
    bool empty() const CV_OVERRIDE { return stock_->empty(); }
    void write(cv::FileStorage& fs) const CV_OVERRIDE { stock_->write(fs); }
    void read(const cv::FileNode& fn) CV_OVERRIDE { stock_->read(fn); }
    cv::String getDefaultName() const CV_OVERRIDE { return stock_->getDefaultName(); }

    void apply(cv::InputArray _image, cv::OutputArray _fgmask, double learningRate = -1) CV_OVERRIDE
    {
        if (ctx_ && !forwardFailed_ && _image.kind() == cv::_InputArray::MAT && !_fgmask.isUMat()) {
            cv::Mat image = _image.getMat();
            const int t = image.type();
            if (image.dims <= 2 && !image.empty() && (t == CV_8UC1 || t == CV_8UC3 || t == CV_32FC1 || t == CV_32FC3)) {
                _fgmask.create(image.size(), CV_8U);
                cv::Mat mask = _fgmask.getMat();
                if (mi355cv_mog2Apply(ctx_, image.data, image.step, mask.data, mask.step, image.cols, image.rows, t, learningRate) == MI355CV_OK) {
                    served_ = true; size_ = image.size(); type_ = t;
                    return;
                }
            }
        }
        if (served_) CV_Error(cv::Error::StsNotImplemented, cv::String("mi355cv::BackgroundSubtractorMOG2: the model lives on the device and this frame was declined: ") + mi355cv_lastError());
        if (ctx_) { mi355cv_mog2Free(ctx_); ctx_ = nullptr; }                   // declined on the very first frame: the stock object from here on
        stock_->apply(_image, _fgmask, learningRate);
    }

    void getBackgroundImage(cv::OutputArray _dst) const CV_OVERRIDE
    {
        if (!served_) { stock_->getBackgroundImage(_dst); return; }
        _dst.create(size_, type_);
        cv::Mat dst = _dst.getMat();
        if (mi355cv_mog2GetBackgroundImage(ctx_, dst.data, dst.step, dst.cols, dst.rows, type_) != MI355CV_OK)
            CV_Error(cv::Error::StsNotImplemented, cv::String("mi355cv::BackgroundSubtractorMOG2::getBackgroundImage: ") + mi355cv_lastError());
    }
private:
    // a value the handle declines (nmixtures above mi355cv_limit("mog2_max_mixtures"), say) before any frame was served sends the object to the stock path
    void forward(const char* name, double v) { if (ctx_ && mi355cv_mog2SetParam(ctx_, name, v) != MI355CV_OK) forwardFailed_ = true; }
    cv::Ptr<cv::BackgroundSubtractorMOG2> stock_;
    void* ctx_ = nullptr;
    bool served_ = false, forwardFailed_ = false;
    cv::Size size_;
    int type_ = -1;
};

inline cv::Ptr<cv::BackgroundSubtractorMOG2> createBackgroundSubtractorMOG2(int history = 500, double varThreshold = 16, bool detectShadows = true)
{
    return cv::makePtr<mi355cv::BackgroundSubtractorMOG2>(cv::createBackgroundSubtractorMOG2(history, varThreshold, detectShadows));
}
#endif

#ifdef OPENCV_CALIB3D_HPP       // cv::StereoBM lives in opencv2/calib3d.hpp; include it before this header to get the wrapper
// cv::StereoBM (calib3d.hpp; stereobm.cpp).  The reference has no HAL hook for it.  mi355cv::StereoBM::create returns a cv::StereoBM that wraps the stock object, where
// the parameters live; compute sends two 2-D CV_8UC1 cv::Mat images through mi355cv_stereoBM (csrc/stereobm.hip), the images and the CV_16SC1 map staying where the Mats
// live.  The map is the project's restatement of the algorithm (tests/stereobm_restate.py), all integer and determined bit for bit; where recollection of
// the reference differs it is listed there.  Everything the entry declines (PREFILTER_NORMALIZED_RESPONSE, speckle filtering, ROIs, sizes over the limits, UMat, no
// device) goes to the stock object, which finds the map untouched.  Not compiled here: the reference's headers are absent.
class StereoBM CV_FINAL : public cv::StereoBM
{
public:
    explicit StereoBM(const cv::Ptr<cv::StereoBM>& stock) : stock_(stock) {}
    static cv::Ptr<cv::StereoBM> create(int numDisparities = 0, int blockSize = 21) { return cv::makePtr<mi355cv::StereoBM>(cv::StereoBM::create(numDisparities, blockSize)); }

    int getMinDisparity() const CV_OVERRIDE { return stock_->getMinDisparity(); }              void setMinDisparity(int v) CV_OVERRIDE { stock_->setMinDisparity(v); }
    int getNumDisparities() const CV_OVERRIDE { return stock_->getNumDisparities(); }          void setNumDisparities(int v) CV_OVERRIDE { stock_->setNumDisparities(v); }
    int getBlockSize() const CV_OVERRIDE { return stock_->getBlockSize(); }                    void setBlockSize(int v) CV_OVERRIDE { stock_->setBlockSize(v); }
    int getSpeckleWindowSize() const CV_OVERRIDE { return stock_->getSpeckleWindowSize(); }    void setSpeckleWindowSize(int v) CV_OVERRIDE { stock_->setSpeckleWindowSize(v); }
    int getSpeckleRange() const CV_OVERRIDE { return stock_->getSpeckleRange(); }              void setSpeckleRange(int v) CV_OVERRIDE { stock_->setSpeckleRange(v); }
    int getDisp12MaxDiff() const CV_OVERRIDE { return stock_->getDisp12MaxDiff(); }            void setDisp12MaxDiff(int v) CV_OVERRIDE { stock_->setDisp12MaxDiff(v); }
    int getPreFilterType() const CV_OVERRIDE { return stock_->getPreFilterType(); }            void setPreFilterType(int v) CV_OVERRIDE { stock_->setPreFilterType(v); }
    int getPreFilterSize() const CV_OVERRIDE { return stock_->getPreFilterSize(); }            void setPreFilterSize(int v) CV_OVERRIDE { stock_->setPreFilterSize(v); }
    int getPreFilterCap() const CV_OVERRIDE { return stock_->getPreFilterCap(); }              void setPreFilterCap(int v) CV_OVERRIDE { stock_->setPreFilterCap(v); }
    int getTextureThreshold() const CV_OVERRIDE { return stock_->getTextureThreshold(); }      void setTextureThreshold(int v) CV_OVERRIDE { stock_->setTextureThreshold(v); }
    int getUniquenessRatio() const CV_OVERRIDE { return stock_->getUniquenessRatio(); }        void setUniquenessRatio(int v) CV_OVERRIDE { stock_->setUniquenessRatio(v); }
    int getSmallerBlockSize() const CV_OVERRIDE { return stock_->getSmallerBlockSize(); }      void setSmallerBlockSize(int v) CV_OVERRIDE { stock_->setSmallerBlockSize(v); }
    cv::Rect getROI1() const CV_OVERRIDE { return stock_->getROI1(); }                         void setROI1(cv::Rect r) CV_OVERRIDE { stock_->setROI1(r); }
    cv::Rect getROI2() const CV_OVERRIDE { return stock_->getROI2(); }                         void setROI2(cv::Rect r) CV_OVERRIDE { stock_->setROI2(r); }
    void clear() CV_OVERRIDE { stock_->clear(); }
    bool empty() const CV_OVERRIDE { return stock_->empty(); }
    void write(cv::FileStorage& fs) const CV_OVERRIDE { stock_->write(fs); }
    void read(const cv::FileNode& fn) CV_OVERRIDE { stock_->read(fn); }
    cv::String getDefaultName() const CV_OVERRIDE { return stock_->getDefaultName(); }

    void compute(cv::InputArray _left, cv::InputArray _right, cv::OutputArray _disp) CV_OVERRIDE
    {
        if (_left.kind() == cv::_InputArray::MAT && _right.kind() == cv::_InputArray::MAT && !_disp.isUMat()) {
            cv::Mat left = _left.getMat(), right = _right.getMat();
            // the reference writes CV_16S unless the destination was fixed to CV_32F by the caller
            const int dtype = _disp.fixedType() && _disp.type() == CV_32FC1 ? CV_32FC1 : CV_16SC1;
            if (left.dims <= 2 && !left.empty() && left.type() == CV_8UC1 && right.type() == CV_8UC1 && left.size() == right.size()) {
                mi355cv_StereoBMParams p;
                mi355cv_stereoBMDefaults(&p);
                p.minDisparity = getMinDisparity(); p.numDisparities = getNumDisparities(); p.blockSize = getBlockSize(); p.preFilterType = getPreFilterType();
                p.preFilterSize = getPreFilterSize(); p.preFilterCap = getPreFilterCap(); p.textureThreshold = getTextureThreshold(); p.uniquenessRatio = getUniquenessRatio();
                p.speckleWindowSize = getSpeckleWindowSize(); p.speckleRange = getSpeckleRange(); p.disp12MaxDiff = getDisp12MaxDiff();
                const cv::Rect r1 = getROI1(), r2 = getROI2();
                p.roi1[0] = r1.x; p.roi1[1] = r1.y; p.roi1[2] = r1.width; p.roi1[3] = r1.height;
                p.roi2[0] = r2.x; p.roi2[1] = r2.y; p.roi2[2] = r2.width; p.roi2[3] = r2.height;
                // an overlapping destination is declined by the entry and the stock object then allocates as it always does
                cv::Mat disp = _disp.getMat();
                if (disp.size() != left.size() || disp.type() != dtype) { _disp.create(left.size(), dtype); disp = _disp.getMat(); }
                if (mi355cv_stereoBM(left.data, left.step, right.data, right.step, disp.data, disp.step, left.cols, left.rows, dtype == CV_32FC1 ? MI355CV_32F : MI355CV_16S, &p) == MI355CV_OK)
                    return;
            }
        }
        stock_->compute(_left, _right, _disp);
    }
private:
    cv::Ptr<cv::StereoBM> stock_;
};

// cv::StereoSGBM (calib3d.hpp; stereosgbm.cpp).  The reference has no HAL hook for it.  mi355cv::StereoSGBM::create returns a cv::StereoSGBM that wraps the stock object,
// where the parameters live; compute sends two 2-D CV_8UC1 cv::Mat images through mi355cv_stereoSGBM (csrc/sgbm.hip), the images and the map staying where the Mats live.
// The map is the project's restatement of the algorithm (tests/sgbm_restate.py), all integer and determined bit for bit; where recollection of the
// reference differs it is listed there.  speckleWindowSize > 0 is served (the map goes through the served filterSpeckles on the device).  Everything the entry declines
// (MODE_SGBM_3WAY, 3-channel images, parameters over the limits or outside the 16-bit cost bound, UMat, no device) goes to the stock object, which finds the map
// untouched.  Not compiled here: the reference's headers are absent.
class StereoSGBM CV_FINAL : public cv::StereoSGBM
{
public:
    explicit StereoSGBM(const cv::Ptr<cv::StereoSGBM>& stock) : stock_(stock) {}
    static cv::Ptr<cv::StereoSGBM> create(int minDisparity = 0, int numDisparities = 16, int blockSize = 3, int P1 = 0, int P2 = 0, int disp12MaxDiff = 0, int preFilterCap = 0,
                                          int uniquenessRatio = 0, int speckleWindowSize = 0, int speckleRange = 0, int mode = cv::StereoSGBM::MODE_SGBM)
    {
        return cv::makePtr<mi355cv::StereoSGBM>(cv::StereoSGBM::create(minDisparity, numDisparities, blockSize, P1, P2, disp12MaxDiff, preFilterCap, uniquenessRatio, speckleWindowSize,
                                                                       speckleRange, mode));
    }

    int getMinDisparity() const CV_OVERRIDE { return stock_->getMinDisparity(); }              void setMinDisparity(int v) CV_OVERRIDE { stock_->setMinDisparity(v); }
    int getNumDisparities() const CV_OVERRIDE { return stock_->getNumDisparities(); }          void setNumDisparities(int v) CV_OVERRIDE { stock_->setNumDisparities(v); }
    int getBlockSize() const CV_OVERRIDE { return stock_->getBlockSize(); }                    void setBlockSize(int v) CV_OVERRIDE { stock_->setBlockSize(v); }
    int getSpeckleWindowSize() const CV_OVERRIDE { return stock_->getSpeckleWindowSize(); }    void setSpeckleWindowSize(int v) CV_OVERRIDE { stock_->setSpeckleWindowSize(v); }
    int getSpeckleRange() const CV_OVERRIDE { return stock_->getSpeckleRange(); }              void setSpeckleRange(int v) CV_OVERRIDE { stock_->setSpeckleRange(v); }
    int getDisp12MaxDiff() const CV_OVERRIDE { return stock_->getDisp12MaxDiff(); }            void setDisp12MaxDiff(int v) CV_OVERRIDE { stock_->setDisp12MaxDiff(v); }
    int getPreFilterCap() const CV_OVERRIDE { return stock_->getPreFilterCap(); }              void setPreFilterCap(int v) CV_OVERRIDE { stock_->setPreFilterCap(v); }
    int getUniquenessRatio() const CV_OVERRIDE { return stock_->getUniquenessRatio(); }        void setUniquenessRatio(int v) CV_OVERRIDE { stock_->setUniquenessRatio(v); }
    int getP1() const CV_OVERRIDE { return stock_->getP1(); }                                  void setP1(int v) CV_OVERRIDE { stock_->setP1(v); }
    int getP2() const CV_OVERRIDE { return stock_->getP2(); }                                  void setP2(int v) CV_OVERRIDE { stock_->setP2(v); }
    int getMode() const CV_OVERRIDE { return stock_->getMode(); }                              void setMode(int v) CV_OVERRIDE { stock_->setMode(v); }
    void clear() CV_OVERRIDE { stock_->clear(); }
    bool empty() const CV_OVERRIDE { return stock_->empty(); }
    void write(cv::FileStorage& fs) const CV_OVERRIDE { stock_->write(fs); }
    void read(const cv::FileNode& fn) CV_OVERRIDE { stock_->read(fn); }
    cv::String getDefaultName() const CV_OVERRIDE { return stock_->getDefaultName(); }

    void compute(cv::InputArray _left, cv::InputArray _right, cv::OutputArray _disp) CV_OVERRIDE
    {
        if (_left.kind() == cv::_InputArray::MAT && _right.kind() == cv::_InputArray::MAT && !_disp.isUMat()) {
            cv::Mat left = _left.getMat(), right = _right.getMat();
            // the reference writes CV_16S unless the destination was fixed to CV_32F by the caller
            const int dtype = _disp.fixedType() && _disp.type() == CV_32FC1 ? CV_32FC1 : CV_16SC1;
            if (left.dims <= 2 && !left.empty() && left.type() == CV_8UC1 && right.type() == CV_8UC1 && left.size() == right.size()) {
                mi355cv_StereoSGBMParams p;
                mi355cv_stereoSGBMDefaults(&p);
                p.minDisparity = getMinDisparity(); p.numDisparities = getNumDisparities(); p.blockSize = getBlockSize(); p.P1 = getP1(); p.P2 = getP2();
                p.disp12MaxDiff = getDisp12MaxDiff(); p.preFilterCap = getPreFilterCap(); p.uniquenessRatio = getUniquenessRatio();
                p.speckleWindowSize = getSpeckleWindowSize(); p.speckleRange = getSpeckleRange(); p.mode = getMode();
                // an overlapping destination is declined by the entry and the stock object then allocates as it always does
                cv::Mat disp = _disp.getMat();
                if (disp.size() != left.size() || disp.type() != dtype) { _disp.create(left.size(), dtype); disp = _disp.getMat(); }
                if (mi355cv_stereoSGBM(left.data, left.step, right.data, right.step, disp.data, disp.step, left.cols, left.rows, dtype == CV_32FC1 ? MI355CV_32F : MI355CV_16S, &p) == MI355CV_OK)
                    return;
            }
        }
        stock_->compute(_left, _right, _disp);
    }
private:
    cv::Ptr<cv::StereoSGBM> stock_;
};

// cv::filterSpeckles (calib3d.hpp; stereosgbm.cpp).  The reference has no HAL hook for it.  A 2-D CV_8UC1 or CV_16SC1 cv::Mat goes through mi355cv_filterSpeckles
// (csrc/speckle.hip) in place, where the Mat lives: the step to take on the map mi355cv::StereoBM::compute left in HBM.  The image is the project's restatement of the
// algorithm (tests/speckle_restate.py): it depends on component sizes only and is determined bit for bit.  newVal and maxDiff are truncated to int as the
// reference does; buf is the reference's scratch and is not used.  Everything the entry declines (other types, a newVal outside the depth's range, sizes over the
// limit, UMat, no device) goes to the stock function, which finds the image untouched.  Not compiled here: the reference's headers are absent.
inline void filterSpeckles(cv::InputOutputArray _img, double newVal, int maxSpeckleSize, double maxDiff, cv::InputOutputArray _buf = cv::noArray())
{
    if (_img.kind() == cv::_InputArray::MAT) {
        cv::Mat img = _img.getMat();
        const bool ints = newVal >= -2147483648.0 && newVal <= 2147483647.0 && maxDiff >= -2147483648.0 && maxDiff <= 2147483647.0;
        if (ints && img.dims <= 2 && !img.empty() && (img.type() == CV_8UC1 || img.type() == CV_16SC1) &&
            mi355cv_filterSpeckles(img.data, img.step, img.cols, img.rows, img.type() == CV_8UC1 ? MI355CV_8U : MI355CV_16S, (int)newVal, maxSpeckleSize, (int)maxDiff) == MI355CV_OK)
            return;
    }
    cv::filterSpeckles(_img, newVal, maxSpeckleSize, maxDiff, _buf);
}
#endif

#ifdef OPENCV_PHOTO_HPP          // cv::fastNlMeansDenoising lives in opencv2/photo.hpp; include it before this header to get the wrappers
// cv::fastNlMeansDenoising / cv::fastNlMeansDenoisingColored (photo.hpp; denoising.cpp, fast_nlmeans_denoising_invoker.hpp).  The reference has no HAL hook for them.
// A 2-D CV_8U cv::Mat of 1 .. 4 channels (Colored: CV_8UC3) goes through mi355cv_fastNlMeansDenoising / ...Colored (csrc/nlmeans.hip), source and destination where
// the Mats live.  The image is the project's restatement of the rule (tests/nlmeans_restate.py): a table of integer weights built on the host, then
// integer arithmetic, determined bit for bit.  Everything the entries decline (other depths, NORM_L1, a per-channel h, windows or sizes over the limits, dst
// overlapping src, UMat, no device) goes to the stock function, which finds the destination untouched.  Not compiled here: the reference's headers are absent.
inline void fastNlMeansDenoising(cv::InputArray _src, cv::OutputArray _dst, float h = 3, int templateWindowSize = 7, int searchWindowSize = 21)
{
    if (_src.kind() == cv::_InputArray::MAT && _dst.kind() == cv::_InputArray::MAT) {
        cv::Mat src = _src.getMat();
        if (src.dims <= 2 && !src.empty() && src.depth() == CV_8U && src.channels() <= 4) {
            _dst.create(src.size(), src.type());
            cv::Mat dst = _dst.getMat();
            if (mi355cv_fastNlMeansDenoising(src.data, src.step, dst.data, dst.step, src.cols, src.rows, MI355CV_8U, src.channels(), &h, 1, templateWindowSize, searchWindowSize,
                                             cv::NORM_L2) == MI355CV_OK)
                return;
        }
    }
    cv::fastNlMeansDenoising(_src, _dst, h, templateWindowSize, searchWindowSize);
}

inline void fastNlMeansDenoisingColored(cv::InputArray _src, cv::OutputArray _dst, float h = 3, float hColor = 3, int templateWindowSize = 7, int searchWindowSize = 21)
{
    if (_src.kind() == cv::_InputArray::MAT && _dst.kind() == cv::_InputArray::MAT) {
        cv::Mat src = _src.getMat();
        if (src.dims <= 2 && !src.empty() && src.type() == CV_8UC3) {
            _dst.create(src.size(), src.type());
            cv::Mat dst = _dst.getMat();
            if (mi355cv_fastNlMeansDenoisingColored(src.data, src.step, dst.data, dst.step, src.cols, src.rows, MI355CV_8U, 3, h, hColor, templateWindowSize, searchWindowSize) ==
                MI355CV_OK)
                return;
        }
    }
    cv::fastNlMeansDenoisingColored(_src, _dst, h, hColor, templateWindowSize, searchWindowSize);
}
#endif

#ifdef OPENCV_CALIB3D_HPP        // cv::undistort, cv::initUndistortRectifyMap and cv::reprojectImageTo3D live in opencv2/calib3d.hpp; include it before this header
// The two ends of the stereo pipeline (csrc/undistort.hip; the reference has no HAL hook for them).  The images are the project's restatement (DESIGN 6.21,
// tests/undistort_restate.py): the closed form of the map per destination pixel in separately rounded doubles, so a map entry may differ from the stock function's,
// which accumulates along the row, by one unit of 1/32 px.  Everything the entries decline (tauX / tauY, a singular newCameraMatrix * R, sizes over the limits, dst
// overlapping src, UMat, no device) goes to the stock function, which finds the destination untouched.  Out of scope: stereoRectify, getOptimalNewCameraMatrix,
// undistortPoints, the fisheye model.  Not compiled here: the reference's headers are absent.
namespace detail {
// K (3 x 3), distCoeffs (a vector of 0, 4, 5, 8, 12 or 14), R (3 x 3 or empty), newK (3 x 3, 3 x 4 or empty) as contiguous doubles; -> false: leave it to the stock function
struct Camera {
    double K[9], R[9], nK[9], dist[14]; int ndist = 0; bool hasR = false, hasNK = false;
    bool set(cv::InputArray _K, cv::InputArray _dist, cv::InputArray _R, cv::InputArray _newK)
    {
        cv::Mat k, d, r, n;
        _K.getMat().convertTo(k, CV_64F);
        if (k.rows != 3 || k.cols != 3) return false;
        for (int i = 0; i < 9; i++) K[i] = k.at<double>(i / 3, i % 3);
        if (!_dist.empty()) {
            _dist.getMat().convertTo(d, CV_64F);
            if (d.total() > 14 || (d.rows != 1 && d.cols != 1)) return false;
            ndist = (int)d.total();
            d = d.reshape(1, 1);
            for (int i = 0; i < ndist; i++) dist[i] = d.at<double>(0, i);
        }
        if (!_R.empty()) {
            _R.getMat().convertTo(r, CV_64F);
            if (r.rows != 3 || r.cols != 3) return false;
            for (int i = 0; i < 9; i++) R[i] = r.at<double>(i / 3, i % 3);
            hasR = true;
        }
        if (!_newK.empty()) {
            _newK.getMat().convertTo(n, CV_64F);
            if (n.rows != 3 || (n.cols != 3 && n.cols != 4)) return false;
            for (int i = 0; i < 9; i++) nK[i] = n.at<double>(i / 3, i % 3);
            hasNK = true;
        }
        return true;
    }
};
} // namespace detail

inline void initUndistortRectifyMap(cv::InputArray cameraMatrix, cv::InputArray distCoeffs, cv::InputArray R, cv::InputArray newCameraMatrix, cv::Size size, int m1type,
                                    cv::OutputArray _map1, cv::OutputArray _map2)
{
    detail::Camera c;
    if (m1type <= 0) m1type = CV_16SC2;
    if (_map1.kind() == cv::_InputArray::MAT && _map2.kind() == cv::_InputArray::MAT && (m1type == CV_16SC2 || m1type == CV_32FC1 || m1type == CV_32FC2) &&
        c.set(cameraMatrix, distCoeffs, R, newCameraMatrix)) {
        _map1.create(size, m1type);
        cv::Mat map1 = _map1.getMat(), map2;
        if (m1type != CV_32FC2) { _map2.create(size, m1type == CV_16SC2 ? CV_16UC1 : CV_32FC1); map2 = _map2.getMat(); } else _map2.release();
        if (mi355cv_initUndistortRectifyMap(c.K, c.ndist ? c.dist : nullptr, c.ndist, c.hasR ? c.R : nullptr, c.hasNK ? c.nK : nullptr, size.width, size.height, m1type, map1.data,
                                            map1.step, map2.data, map2.step) == MI355CV_OK)
            return;
    }
    cv::initUndistortRectifyMap(cameraMatrix, distCoeffs, R, newCameraMatrix, size, m1type, _map1, _map2);
}

// the rectifying warp in one call: cv::remap(src, dst, maps of initUndistortRectifyMap(..., dsize, CV_16SC2), interpolation, borderMode, borderValue) without the maps
inline void undistortRectify(cv::InputArray _src, cv::OutputArray _dst, cv::InputArray cameraMatrix, cv::InputArray distCoeffs, cv::InputArray R, cv::InputArray newCameraMatrix,
                             cv::Size dsize, int interpolation = cv::INTER_LINEAR, int borderMode = cv::BORDER_CONSTANT, const cv::Scalar& borderValue = cv::Scalar())
{
    detail::Camera c;
    if (_src.kind() == cv::_InputArray::MAT && _dst.kind() == cv::_InputArray::MAT && c.set(cameraMatrix, distCoeffs, R, newCameraMatrix)) {
        cv::Mat src = _src.getMat();
        if (src.dims <= 2 && !src.empty()) {
            if (dsize.area() == 0) dsize = src.size();
            _dst.create(dsize, src.type());
            cv::Mat dst = _dst.getMat();
            if (dst.data != src.data &&
                mi355cv_undistortRectify(src.type(), src.data, src.step, src.cols, src.rows, dst.data, dst.step, dst.cols, dst.rows, c.K, c.ndist ? c.dist : nullptr, c.ndist,
                                         c.hasR ? c.R : nullptr, c.hasNK ? c.nK : nullptr, interpolation, borderMode, borderValue.val) == MI355CV_OK)
                return;
        }
    }
    cv::Mat map1, map2;
    cv::initUndistortRectifyMap(cameraMatrix, distCoeffs, R, newCameraMatrix.empty() ? cameraMatrix : newCameraMatrix, dsize.area() ? dsize : _src.size(), CV_16SC2, map1, map2);
    cv::remap(_src, _dst, map1, map2, interpolation, borderMode, borderValue);
}

inline void undistort(cv::InputArray src, cv::OutputArray dst, cv::InputArray cameraMatrix, cv::InputArray distCoeffs, cv::InputArray newCameraMatrix = cv::noArray())
{
    detail::Camera c;
    if (src.kind() == cv::_InputArray::MAT && dst.kind() == cv::_InputArray::MAT && c.set(cameraMatrix, distCoeffs, cv::noArray(), newCameraMatrix)) {
        cv::Mat s = src.getMat();
        if (s.dims <= 2 && !s.empty()) {
            dst.create(s.size(), s.type());
            cv::Mat d = dst.getMat();
            const double zero[4] = {0, 0, 0, 0};
            if (d.data != s.data &&
                mi355cv_undistortRectify(s.type(), s.data, s.step, s.cols, s.rows, d.data, d.step, d.cols, d.rows, c.K, c.ndist ? c.dist : nullptr, c.ndist, nullptr,
                                         c.hasNK ? c.nK : nullptr, cv::INTER_LINEAR, cv::BORDER_CONSTANT, zero) == MI355CV_OK)
                return;
        }
    }
    cv::undistort(src, dst, cameraMatrix, distCoeffs, newCameraMatrix);
}

inline void reprojectImageTo3D(cv::InputArray _disparity, cv::OutputArray _3dImage, cv::InputArray _Q, bool handleMissingValues = false, int ddepth = -1)
{
    if (_disparity.kind() == cv::_InputArray::MAT && _3dImage.kind() == cv::_InputArray::MAT && (ddepth == -1 || ddepth == CV_32F)) {
        cv::Mat disp = _disparity.getMat(), Q;
        _Q.getMat().convertTo(Q, CV_64F);
        const int t = disp.type();
        if (disp.dims <= 2 && !disp.empty() && Q.rows == 4 && Q.cols == 4 && Q.isContinuous() && (t == CV_8UC1 || t == CV_16SC1 || t == CV_32SC1 || t == CV_32FC1)) {
            _3dImage.create(disp.size(), CV_32FC3);
            cv::Mat out = _3dImage.getMat();
            if (mi355cv_reprojectImageTo3D(disp.data, disp.step, t, out.data, out.step, disp.cols, disp.rows, Q.ptr<double>(), handleMissingValues ? 1 : 0, ddepth) == MI355CV_OK)
                return;
        }
    }
    cv::reprojectImageTo3D(_disparity, _3dImage, _Q, handleMissingValues, ddepth);
}
#endif

// Batches across the GPUs of one node from C++: forEachShard({0,1,...,7}, nframes, [&](int slot, int device, int first, int count) { ... return 0; })
// runs the callable once per device on its own host thread bound to that device (mi355cv_runSharded, csrc/shard.hip), frames [first, first + count) being that
// device's share; inside, call cv:: functions of a HAL-enabled build or mi355cv:: / mi355cv_*Batch entry points on Mats whose storage lives on `device`
// (FrameAllocator::Device allocates on the calling thread's device).  Returns 0 or the first failing slot's code (mi355cv_lastError() says which and why).
template <typename F>
inline int forEachShard(const std::vector<int>& devices, int nframes, F&& body)
{
    struct Tr { static int call(void* u, int slot, int device, int first, int count) {
        try { return (*static_cast<typename std::remove_reference<F>::type*>(u))(slot, device, first, count); } catch (...) { return MI355CV_ERROR_UNKNOWN; } } };
    return mi355cv_runSharded((int)devices.size(), devices.data(), nframes, &Tr::call, (void*)&body, 1);
}

} // namespace mi355cv
