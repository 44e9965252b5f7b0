// Loop-closure slice of pose_graph on the GPU (include/vio_posegraph.h): what KeyFrame's constructor computes for every keyframe and what
// KeyFrame::findConnection's descriptor search does (pose_graph/src/keyframe/keyframe.cpp:80-169, 530; DVision::BRIEF::compute).
//   pg_blur_kernel        cv::GaussianBlur(9x9, sigma 2) on u8, 64 x 16 tiles staged in LDS (coalesced row loads, halo 4)
//   pg_fast_score_kernel  FAST-9/16 corner score of every pixel (threshold = argument), 64 x 16 tiles with halo 3
//   pg_fast_nms_kernel    3x3 non-maximum suppression + row-major ordered compaction over the whole image (cv::FAST's output order)
//   pg_brief_kernel       one wavefront per point: lane l evaluates the pair tests l, l + 64, l + 128, l + 192 -> four ballots = the descriptor
//   pg_match_kernel       one wavefront per window descriptor: lanes stride over the old descriptors (v_bcnt popcounts), wave arg-min on
//                         (distance, index) = the sequential scan's "first smallest"
// Integer arithmetic throughout (the blur's 8-bit fixed point included), so the results are the CPU restatement's bit for bit.  The kernel
// bodies live in pg_device.h, which the batched kernels of pg_batch.hip share.
#include <hip/hip_runtime.h>
#include <string>
#include <vector>
#include "../../include/vio_posegraph.h"
#include "camera_model.h"
#include "pg_device.h"

extern thread_local std::string g_err;   // vio_abi.hip

namespace {

__global__ __launch_bounds__(256) void pg_blur_kernel(const uint8_t *src, int W, int H, uint8_t *dst) { pgdev::blur_tile(src, W, H, dst); }

__global__ __launch_bounds__(256) void pg_fast_score_kernel(const uint8_t *img, int W, int H, int thr, uint8_t *score) {
    pgdev::fast_score_tile(img, W, H, thr, score);
}

__global__ __launch_bounds__(1024) void pg_fast_nms_kernel(const uint8_t *score, int W, int H, unsigned long long *words, float *kp_xy, int cap, int *count) {
    const int total = pgdev::fast_nms_image(score, W, H, words, kp_xy, cap);
    if (threadIdx.x == 0) *count = total;
}

__global__ __launch_bounds__(64) void pg_brief_kernel(const uint8_t *blur, int W, int H, const float *xy, int n, const int *pat, unsigned long long *desc) {
    const int p = blockIdx.x;
    if (p >= n) return;
    pgdev::brief_point(blur, W, H, xy, p, pat, desc);
}

__global__ void pg_lift_kernel(vio_config c, const float *xy, int n, float *nrm) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    pgdev::lift_pinhole(c, xy, i, nrm);
}

__global__ void pg_lift_camera_kernel(vio_camera cam, const float *xy, int n, float *nrm) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    pgdev::lift_camera(cam, xy, i, nrm);
}

// one wavefront per window descriptor
__global__ __launch_bounds__(64) void pg_match_kernel(const unsigned long long *wd, int n, const unsigned long long *od, int m, int *best_index, int *best_dist) {
    const int i = blockIdx.x;
    if (i >= n) return;
    const int key = pgdev::match_scan(wd + 4 * (size_t)i, od, m);
    if (threadIdx.x == 0) {
        best_dist[i] = key >> 20;
        best_index[i] = pgdev::match_index(key);
    }
}

struct DevBuf {   // scope-bound device allocation
    void *p = nullptr;
    ~DevBuf() { if (p) (void)hipFree(p); }
    hipError_t alloc(size_t n) { return hipMalloc(&p, n ? n : 1); }
    template <typename T> T *as() { return (T *)p; }
};
#define PGCHK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { g_err = std::string(#x) + ": " + hipGetErrorString(e_); return VIO_EDEVICE; } } while (0)

int have_device() {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) { g_err = "no HIP device: the pose-graph kernels have no CPU fallback"; return VIO_EDEVICE; }
    return VIO_OK;
}

}  // namespace

extern "C" int vio_pg_stage_blur(const uint8_t *gray, int width, int height, uint8_t *out) {
    if (!gray || !out || width < 16 || height < 16) return VIO_EINVAL;
    if (int rc = have_device()) return rc;
    DevBuf a, b;
    const size_t hw = (size_t)width * height;
    PGCHK(a.alloc(hw)); PGCHK(b.alloc(hw));
    PGCHK(hipMemcpy(a.p, gray, hw, hipMemcpyHostToDevice));
    pg_blur_kernel<<<dim3((width + PG_TW - 1) / PG_TW, (height + PG_TH - 1) / PG_TH), 256>>>(a.as<uint8_t>(), width, height, b.as<uint8_t>());
    PGCHK(hipDeviceSynchronize());
    PGCHK(hipMemcpy(out, b.p, hw, hipMemcpyDeviceToHost));
    return VIO_OK;
}

// vio_pg_describe (cam == nullptr: cfg's pinhole) and vio_pg_describe_camera
static int pg_describe(const vio_config *cfg, const vio_camera *cam, const uint8_t *gray, int n_win, const float *win_uv, const int32_t *pattern1024,
                       int fast_threshold, uint64_t *win_desc, int cap, float *kp_xy, uint64_t *kp_desc, float *kp_norm) {
    if (!cfg || !gray || !pattern1024 || n_win < 0 || cap < 0 || (n_win > 0 && (!win_uv || !win_desc)) || (cap > 0 && (!kp_xy || !kp_desc || !kp_norm))) return VIO_EINVAL;
    const int W = cfg->width, H = cfg->height;
    if (W < 16 || H < 16 || W > 4095 || H > 4095 || fast_threshold < 1 || fast_threshold > 254) return VIO_EINVAL;
    if (int rc = have_device()) return rc;
    const size_t hw = (size_t)W * H;
    DevBuf img, blur, score, words, pat, wuv, wdesc, kxy, kdesc, knrm, cnt;
    const int nchunk = ((W - 6) * (H - 6) + 63) / 64;
    PGCHK(img.alloc(hw)); PGCHK(blur.alloc(hw)); PGCHK(score.alloc(hw)); PGCHK(words.alloc((size_t)nchunk * 8)); PGCHK(pat.alloc(1024 * 4));
    PGCHK(wuv.alloc((size_t)n_win * 8)); PGCHK(wdesc.alloc((size_t)n_win * 32)); PGCHK(kxy.alloc((size_t)cap * 8)); PGCHK(kdesc.alloc((size_t)cap * 32));
    PGCHK(knrm.alloc((size_t)cap * 8)); PGCHK(cnt.alloc(4));
    PGCHK(hipMemcpy(img.p, gray, hw, hipMemcpyHostToDevice));
    PGCHK(hipMemcpy(pat.p, pattern1024, 1024 * 4, hipMemcpyHostToDevice));
    const dim3 tiles((W + PG_TW - 1) / PG_TW, (H + PG_TH - 1) / PG_TH);
    pg_blur_kernel<<<tiles, 256>>>(img.as<uint8_t>(), W, H, blur.as<uint8_t>());
    pg_fast_score_kernel<<<tiles, 256>>>(img.as<uint8_t>(), W, H, fast_threshold, score.as<uint8_t>());
    if (n_win > 0) {
        PGCHK(hipMemcpy(wuv.p, win_uv, (size_t)n_win * 8, hipMemcpyHostToDevice));
        pg_brief_kernel<<<n_win, 64>>>(blur.as<uint8_t>(), W, H, wuv.as<float>(), n_win, pat.as<int>(), wdesc.as<unsigned long long>());
    }
    pg_fast_nms_kernel<<<1, 1024>>>(score.as<uint8_t>(), W, H, words.as<unsigned long long>(), kxy.as<float>(), cap, cnt.as<int>());
    int total = 0;
    PGCHK(hipMemcpy(&total, cnt.p, 4, hipMemcpyDeviceToHost));
    const int m = total < cap ? total : cap;
    if (m > 0) {
        pg_brief_kernel<<<m, 64>>>(blur.as<uint8_t>(), W, H, kxy.as<float>(), m, pat.as<int>(), kdesc.as<unsigned long long>());
        if (cam) pg_lift_camera_kernel<<<(m + 255) / 256, 256>>>(*cam, kxy.as<float>(), m, knrm.as<float>());
        else pg_lift_kernel<<<(m + 255) / 256, 256>>>(*cfg, kxy.as<float>(), m, knrm.as<float>());
    }
    PGCHK(hipDeviceSynchronize());
    if (n_win > 0) PGCHK(hipMemcpy(win_desc, wdesc.p, (size_t)n_win * 32, hipMemcpyDeviceToHost));
    if (m > 0) {
        PGCHK(hipMemcpy(kp_xy, kxy.p, (size_t)m * 8, hipMemcpyDeviceToHost));
        PGCHK(hipMemcpy(kp_desc, kdesc.p, (size_t)m * 32, hipMemcpyDeviceToHost));
        PGCHK(hipMemcpy(kp_norm, knrm.p, (size_t)m * 8, hipMemcpyDeviceToHost));
    }
    return total;
}

extern "C" int vio_pg_describe(const vio_config *cfg, const uint8_t *gray, int n_win, const float *win_uv, const int32_t *pattern1024, int fast_threshold,
                               uint64_t *win_desc, int cap, float *kp_xy, uint64_t *kp_desc, float *kp_norm) {
    return pg_describe(cfg, nullptr, gray, n_win, win_uv, pattern1024, fast_threshold, win_desc, cap, kp_xy, kp_desc, kp_norm);
}

extern "C" int vio_pg_describe_camera(const vio_config *cfg, const vio_camera *cam, const uint8_t *gray, int n_win, const float *win_uv,
                                      const int32_t *pattern1024, int fast_threshold, uint64_t *win_desc, int cap, float *kp_xy, uint64_t *kp_desc,
                                      float *kp_norm) {
    if (!cam) return VIO_EINVAL;
    return pg_describe(cfg, cam, gray, n_win, win_uv, pattern1024, fast_threshold, win_desc, cap, kp_xy, kp_desc, kp_norm);
}

extern "C" int vio_pg_match(const uint64_t *win_desc, int n, const uint64_t *old_desc, int m, int32_t *best_index, int32_t *best_dist) {
    if (n < 0 || m < 0 || m > 0xFFFFE || (n > 0 && (!win_desc || !best_index || !best_dist)) || (m > 0 && !old_desc)) return VIO_EINVAL;
    if (n == 0) return VIO_OK;
    if (int rc = have_device()) return rc;
    DevBuf a, b, bi, bd;
    PGCHK(a.alloc((size_t)n * 32)); PGCHK(b.alloc((size_t)m * 32)); PGCHK(bi.alloc((size_t)n * 4)); PGCHK(bd.alloc((size_t)n * 4));
    PGCHK(hipMemcpy(a.p, win_desc, (size_t)n * 32, hipMemcpyHostToDevice));
    if (m > 0) PGCHK(hipMemcpy(b.p, old_desc, (size_t)m * 32, hipMemcpyHostToDevice));
    pg_match_kernel<<<n, 64>>>(a.as<unsigned long long>(), n, b.as<unsigned long long>(), m, bi.as<int>(), bd.as<int>());
    PGCHK(hipDeviceSynchronize());
    PGCHK(hipMemcpy(best_index, bi.p, (size_t)n * 4, hipMemcpyDeviceToHost));
    PGCHK(hipMemcpy(best_dist, bd.p, (size_t)n * 4, hipMemcpyDeviceToHost));
    return VIO_OK;
}
