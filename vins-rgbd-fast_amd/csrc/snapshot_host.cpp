// Sequence snapshots, the part that needs neither a handle nor a GPU: the shape key of a configuration and the validation of a blob's header.
// Plain C++ (no HIP): it also builds with the host compiler alone (-DVIO_SNAPSHOT_STANDALONE supplies vio_last_error), which is how
// tests/test_snapshot_cpu.py runs it under the address / undefined-behaviour sanitizers.
#include <stddef.h>
#include <string.h>
#include <string>
#include "snapshot.h"

#ifdef VIO_SNAPSHOT_STANDALONE
thread_local std::string g_err;
extern "C" const char *vio_last_error(void) { return g_err.c_str(); }
extern "C" int vio_abi_version(void) { return 12; }
#else
extern thread_local std::string g_err;
#endif

namespace {
struct ShapeField { const char *name; size_t off, size; };
#define SF(f) {#f, offsetof(vio_snapshot_shape, f), sizeof(((vio_snapshot_shape *)0)->f)}
const ShapeField kShapeFields[] = {
    SF(width), SF(height), SF(max_cnt), SF(min_dist), SF(grid_rows), SF(grid_cols), SF(window_size), SF(max_landmarks), SF(fix_depth),
    SF(estimate_extrinsic), SF(estimate_td), SF(max_iterations), SF(ransac_max_iters), SF(lk_max_level), SF(dynamic_init), SF(use_imu),
    SF(reference_quirks), SF(marg_exact), SF(equalize), SF(imu_capacity), SF(hist_cap), SF(pyramid_levels), SF(reserved), SF(focal_length),
    SF(f_threshold), SF(depth_min), SF(depth_max), SF(min_parallax_px), SF(init_depth)};
#undef SF
}  // namespace

const char *snap_shape_diff(const vio_snapshot_shape &a, const vio_snapshot_shape &b) {
    for (const ShapeField &f : kShapeFields)
        if (memcmp((const char *)&a + f.off, (const char *)&b + f.off, f.size) != 0) return f.name;
    return nullptr;
}

extern "C" {

int vio_shape_key(const vio_config *c, int imu_capacity, vio_snapshot_shape *out) {
    if (!c || !out) { g_err = "vio_shape_key: bad arguments"; return VIO_EINVAL; }
    vio_snapshot_shape k;
    memset(&k, 0, sizeof(k));
    k.width = c->width; k.height = c->height; k.max_cnt = c->max_cnt; k.min_dist = c->min_dist;
    k.grid_rows = c->grid_rows; k.grid_cols = c->grid_cols; k.window_size = c->window_size; k.max_landmarks = c->max_landmarks;
    k.fix_depth = c->fix_depth; k.estimate_extrinsic = c->estimate_extrinsic; k.estimate_td = c->estimate_td;
    k.max_iterations = c->max_iterations; k.ransac_max_iters = c->ransac_max_iters; k.lk_max_level = c->lk_max_level;
    k.dynamic_init = c->dynamic_init; k.use_imu = c->use_imu; k.reference_quirks = c->reference_quirks; k.marg_exact = c->marg_exact;
    k.equalize = c->equalize;
    k.imu_capacity = imu_capacity < 256 ? 256 : imu_capacity;   // as vio_create sizes the ring
    k.hist_cap = 2048;
    k.pyramid_levels = 3;
    k.focal_length = c->focal_length; k.f_threshold = c->f_threshold; k.depth_min = c->depth_min; k.depth_max = c->depth_max;
    k.min_parallax_px = c->min_parallax_px; k.init_depth = c->init_depth;
    *out = k;
    return VIO_OK;
}

int vio_snapshot_info(const void *blob, int64_t bytes, vio_snapshot_header *out) {
    if (!blob || bytes <= 0) { g_err = "vio_snapshot_info: empty buffer"; return VIO_EINVAL; }
    if (bytes < (int64_t)sizeof(vio_snapshot_header)) { g_err = "vio_snapshot_info: bytes: the buffer is shorter than a snapshot header"; return VIO_EINVAL; }
    vio_snapshot_header hd;
    memcpy(&hd, blob, sizeof(hd));   // (the caller's buffer need not be aligned)
    if (hd.magic != VIO_SNAPSHOT_MAGIC) { g_err = "vio_snapshot_info: magic: not a snapshot"; return VIO_EINVAL; }
    if (hd.format_version != VIO_SNAPSHOT_FORMAT) {
        g_err = "vio_snapshot_info: format_version " + std::to_string(hd.format_version) + " is not the version this library reads (" +
                std::to_string(VIO_SNAPSHOT_FORMAT) + ")";
        return VIO_EINVAL;
    }
    if (hd.device_bytes < 0 || hd.host_bytes < 0 || (hd.device_bytes & 15) || (hd.host_bytes & 15) ||
        hd.device_bytes > (INT64_MAX >> 2) || hd.host_bytes > (INT64_MAX >> 2) ||
        hd.total_bytes != (int64_t)sizeof(vio_snapshot_header) + hd.device_bytes + hd.host_bytes) {
        g_err = "vio_snapshot_info: total_bytes does not add up from device_bytes and host_bytes";
        return VIO_EINVAL;
    }
    if (hd.total_bytes > bytes) {
        g_err = "vio_snapshot_info: total_bytes: the blob is truncated (" + std::to_string(bytes) + " of " + std::to_string(hd.total_bytes) + " bytes)";
        return VIO_EINVAL;
    }
    if (hd.tracker_lag != 0 && hd.tracker_lag != 1) { g_err = "vio_snapshot_info: tracker_lag is neither 0 nor 1"; return VIO_EINVAL; }
    if (out) *out = hd;
    return VIO_OK;
}

}  // extern "C"
