// Sequence snapshots of the C ABI (include/vio_abi.h "sequence snapshots"): vio_snapshot_bytes, vio_save_seqs, vio_load_seqs and
// their debug entry points.  The rows of a snapshot come from the handle's array table (vio_handle.h).
#include "vio_handle.h"

using namespace vio_internal;

extern "C" {

// ---------------------------------------------------------------------------------------------------------------- sequence snapshots
// The rows of the layout come from the handle's array table (vio_handle.h, VIO_HANDLE_ARRAYS), in its order.  STATE rows are what a snapshot
// carries, each at the next multiple of 16 bytes of the blob's device part; the pack / unpack kernels, the naive reference loop and
// vio_debug_snapshot_layout all walk these rows.
static void snapshot_build_layout(vio_batch *h) {
    if (!h->snap_rows.empty()) return;
    Batch &B = h->B;
    DevCfg &C = h->hc;
    const HandleDims D = handle_dims(C, B.hist_cap);
    const int64_t S = h->S;
    std::vector<vio_batch::SnapRow> &R = h->snap_rows;
#define VIO_R_OVER(kind, name, ptr, count) R.push_back({name, ARR_##kind, (unsigned char *)(ptr), (ptr) ? (int64_t)(count) * (int64_t)sizeof(*(ptr)) : 0, -1});
#define VIO_R_SEQ(kind, member, count) VIO_R_OVER(kind, #member, B.member, count)
#define VIO_R_ROW(kind, name, lvalue, count, n) VIO_R_OVER(kind, name, lvalue, count)
#define VIO_R_VIEW(kind, name, lvalue, count, at) VIO_R_OVER(kind, name, lvalue, count)
#define VIO_R_WIDE(name, lvalue, n) R.push_back({name, ARR_HANDLE, nullptr, 0, -1});
#define VIO_R_DOC(name) R.push_back({name, ARR_HANDLE, nullptr, 0, -1});
#define VIO_R_HOST(kind, name, bytes) R.push_back({name, ARR_##kind, nullptr, (int64_t)(bytes), -1});
    VIO_HANDLE_ARRAYS(VIO_R_SEQ, VIO_R_ROW, VIO_R_VIEW, VIO_R_WIDE, VIO_R_DOC, VIO_R_HOST)
#undef VIO_R_OVER
#undef VIO_R_SEQ
#undef VIO_R_ROW
#undef VIO_R_VIEW
#undef VIO_R_WIDE
#undef VIO_R_DOC
#undef VIO_R_HOST
    (void)S; (void)D;
    int64_t off = 0, chunks = 0;
    int ne = 0;
    for (auto &r : R)
        if (r.kind == 1 && r.base && r.bytes > 0) { r.blob_off = off; off += (r.bytes + 15) & ~(int64_t)15; chunks += (r.bytes + 15) >> 4; ne++; }
    h->snap_dev_bytes = off; h->snap_chunks = chunks; h->snap_entries = ne;
}
static const vio_batch::SnapRow *snapshot_row(const vio_batch *h, const char *name) {
    for (const auto &r : h->snap_rows) if (!strcmp(r.name, name)) return &r;
    return nullptr;
}
static void snapshot_handle_shape(const vio_batch *h, vio_snapshot_shape *k) {
    (void)vio_shape_key(&h->hc.c, h->hc.NIMU, k);
    k->hist_cap = h->B.hist_cap;
}

// host part of a blob: last_imu_t and, on dynamic_init handles, the image-frame mirror (DynSeq).  Fixed little-endian records, padded with
// zeros to a multiple of 16.  Of an ImageFrame only what survives between two attempts travels (stamp, ids, points, the linearisation point,
// the raw samples, bg_lin): everything else is recomputed by vinit::run before it is read.
struct SnapHostFixed { double last_imu_t; int32_t has_dyn, n_frames; double initial_timestamp; int32_t nonlinear, attempts, failures, last_stage; double pad; };
struct SnapFrameFixed { double stamp; int32_t n_ids, n_dt; double lin_acc[3], lin_gyr[3], bg_lin[3]; };
static_assert(sizeof(SnapHostFixed) == 48 && sizeof(SnapFrameFixed) == 88, "snapshot host records");
static int64_t snapshot_host_bytes(const vio_batch *h, int seq) {
    int64_t b = sizeof(SnapHostFixed);
    if (!h->dyn.empty())
        for (const auto &f : h->dyn[seq].frames)
            b += (int64_t)sizeof(SnapFrameFixed) + (((int64_t)f.ids.size() + 1) & ~(int64_t)1) * 4 + (int64_t)(f.xy.size() + f.dt.size() + f.acc.size() + f.gyr.size()) * 8;
    return (b + 15) & ~(int64_t)15;
}
static void snapshot_write_host(const vio_batch *h, int seq, unsigned char *p, int64_t bytes) {
    memset(p, 0, (size_t)bytes);
    SnapHostFixed hf;
    memset(&hf, 0, sizeof(hf));
    hf.last_imu_t = h->last_imu_t[seq];
    if (!h->dyn.empty()) {
        const vio_batch::DynSeq &D = h->dyn[seq];
        hf.has_dyn = 1; hf.n_frames = (int32_t)D.frames.size(); hf.initial_timestamp = D.initial_timestamp;
        hf.nonlinear = D.nonlinear ? 1 : 0; hf.attempts = D.attempts; hf.failures = D.failures; hf.last_stage = D.last_stage;
    }
    memcpy(p, &hf, sizeof(hf)); p += sizeof(hf);
    if (h->dyn.empty()) return;
    for (const auto &f : h->dyn[seq].frames) {
        SnapFrameFixed ff;
        memset(&ff, 0, sizeof(ff));
        ff.stamp = f.stamp; ff.n_ids = (int32_t)f.ids.size(); ff.n_dt = (int32_t)f.dt.size();
        for (int k = 0; k < 3; k++) { ff.lin_acc[k] = f.lin_acc[k]; ff.lin_gyr[k] = f.lin_gyr[k]; ff.bg_lin[k] = f.bg_lin[k]; }
        memcpy(p, &ff, sizeof(ff)); p += sizeof(ff);
        if (!f.ids.empty()) memcpy(p, f.ids.data(), f.ids.size() * 4);
        p += ((f.ids.size() + 1) & ~(size_t)1) * 4;
        auto put = [&](const std::vector<double> &v) { if (!v.empty()) memcpy(p, v.data(), v.size() * 8); p += v.size() * 8; };
        put(f.xy); put(f.dt); put(f.acc); put(f.gyr);
    }
}
// parses (and bounds-checks) the host part; D may be NULL (validation only).  "" or the complaint.
static std::string snapshot_read_host(const unsigned char *p, int64_t bytes, bool want_dyn, int NP, double *last_imu_t, vio_batch::DynSeq *D) {
    const unsigned char *end = p + bytes;
    SnapHostFixed hf;
    if (bytes < (int64_t)sizeof(hf)) return "host_bytes: the host part is shorter than its fixed record";
    memcpy(&hf, p, sizeof(hf)); p += sizeof(hf);
    if ((hf.has_dyn != 0) != want_dyn) return "dynamic_init: the host part does not match the handle";
    if (hf.n_frames < 0 || (!hf.has_dyn && hf.n_frames != 0)) return "host part: bad image-frame count";
    if (last_imu_t) *last_imu_t = hf.last_imu_t;
    if (D) { *D = vio_batch::DynSeq(); D->initial_timestamp = hf.initial_timestamp; D->nonlinear = hf.nonlinear != 0; D->attempts = hf.attempts; D->failures = hf.failures; D->last_stage = hf.last_stage; }
    for (int i = 0; i < hf.n_frames; i++) {
        SnapFrameFixed ff;
        if (end - p < (int64_t)sizeof(ff)) return "host_bytes: an image frame runs past the end of the blob";
        memcpy(&ff, p, sizeof(ff)); p += sizeof(ff);
        if (ff.n_ids < 0 || ff.n_ids > NP || ff.n_dt < 0 || ff.n_dt > VIO_IMU_SLOT_CAP) return "host part: image frame counts out of range";
        const int64_t need = (((int64_t)ff.n_ids + 1) & ~(int64_t)1) * 4 + ((int64_t)2 * ff.n_ids + (int64_t)7 * ff.n_dt) * 8;
        if (end - p < need) return "host_bytes: an image frame runs past the end of the blob";
        if (D) {
            vinit::ImageFrame f;
            f.stamp = ff.stamp;
            for (int k = 0; k < 3; k++) { f.lin_acc[k] = ff.lin_acc[k]; f.lin_gyr[k] = ff.lin_gyr[k]; f.bg_lin[k] = ff.bg_lin[k]; }
            const unsigned char *q = p;
            f.ids.resize(ff.n_ids);
            if (ff.n_ids) memcpy(f.ids.data(), q, (size_t)ff.n_ids * 4);
            q += (((size_t)ff.n_ids + 1) & ~(size_t)1) * 4;
            auto get = [&](std::vector<double> &v, size_t cnt) { v.resize(cnt); if (cnt) memcpy(v.data(), q, cnt * 8); q += cnt * 8; };
            get(f.xy, (size_t)2 * ff.n_ids); get(f.dt, (size_t)ff.n_dt); get(f.acc, (size_t)3 * ff.n_dt); get(f.gyr, (size_t)3 * ff.n_dt);
            D->frames.push_back(std::move(f));
        }
        p += need;
    }
    return "";
}

// what vio_reset_seq does before it touches a slot (the staged IMU goes INTO the rings here instead of being dropped)
static int snapshot_quiesce(vio_batch *h, bool flush) {
    if (flush) VIO_TRY(flush_imu_backend(h));
    VIO_TRY(sync_all(h));
    return refresh_dynamic_state(h);
}
// device side of the first save / load: the table, and room for `count` sequences and `stage_bytes` of staging
static int snapshot_reserve(vio_batch *h, size_t count, size_t stage_bytes) {
    snapshot_build_layout(h);
    if (!h->d_snap_tab) {
        std::vector<SnapEntry> tab;
        int64_t c0 = 0;
        for (const auto &r : h->snap_rows)
            if (r.blob_off >= 0) { tab.push_back({r.base, r.bytes, r.bytes, r.blob_off, c0}); c0 += (r.bytes + 15) >> 4; }
        VIO_TRY(dev_alloc(h, &h->d_snap_tab, tab.size(), false));
        HIPCHK(hipMemcpy(h->d_snap_tab, tab.data(), tab.size() * sizeof(SnapEntry), hipMemcpyHostToDevice));
    }
    if (count > h->snap_seqs_cap) {
        dev_release(h, h->d_snap_seqs);
        h->snap_seqs_cap = 0;
        VIO_TRY(dev_alloc(h, &h->d_snap_seqs, count, false));
        h->snap_seqs_cap = count;
    }
    if (stage_bytes > h->snap_stage_cap) {
        dev_release(h, h->d_snap_stage);
        h->snap_stage_cap = 0;
        VIO_TRY(dev_alloc(h, &h->d_snap_stage, stage_bytes, false));
        h->snap_stage_cap = stage_bytes;
    }
    return VIO_OK;
}
// Where blob i sits in the staging buffer.  Blobs packed back to back in the caller's buffer keep that arrangement (one copy moves them all);
// otherwise they are laid out back to back here and move one by one.
static bool snapshot_place(int n, const int64_t *offsets, const std::vector<int64_t> &bytes, std::vector<int64_t> &pos, int64_t *span) {
    bool tight = true;
    for (int i = 0; i + 1 < n; i++) tight = tight && offsets[i + 1] == offsets[i] + bytes[i];
    for (int i = 0; i < n; i++) tight = tight && (bytes[i] & 15) == 0;
    pos.resize(n);
    int64_t at = 0;
    for (int i = 0; i < n; i++) { pos[i] = at; at += (bytes[i] + 15) & ~(int64_t)15; }
    *span = at;
    return tight;
}
// one launch per stream group over the sequences it owns, on that group's back-end stream (behind its last kernel), then wait for them
static int snapshot_launch(vio_batch *h, int n, const int32_t *seqs, const std::vector<int64_t> &pos, bool pack) {
    std::vector<SnapSeq> list;
    std::vector<std::pair<int, int>> runs;   // per group: first entry of its run in `list`, count
    for (auto &g : h->groups) {
        const int first = (int)list.size();
        for (int i = 0; i < n; i++)
            if (seqs[i] >= g.s0 && seqs[i] < g.s0 + g.n) list.push_back({pos[i] + (int64_t)sizeof(vio_snapshot_header), seqs[i], 0});
        runs.push_back({first, (int)list.size() - first});
    }
    HIPCHK(hipMemcpy(h->d_snap_seqs, list.data(), list.size() * sizeof(SnapSeq), hipMemcpyHostToDevice));
    const unsigned gx = (unsigned)((h->snap_chunks + SNAP_THREADS - 1) / SNAP_THREADS);
    for (size_t k = 0; k < h->groups.size(); k++) {
        if (runs[k].second == 0) continue;
        const dim3 grid(gx, (unsigned)runs[k].second);
        if (pack) snap_pack_kernel<<<grid, SNAP_THREADS, 0, h->groups[k].stream>>>(h->d_snap_tab, h->snap_entries, h->snap_chunks, h->d_snap_seqs + runs[k].first, h->d_snap_stage);
        else snap_unpack_kernel<<<grid, SNAP_THREADS, 0, h->groups[k].stream>>>(h->d_snap_tab, h->snap_entries, h->snap_chunks, h->d_snap_seqs + runs[k].first, h->d_snap_stage);
    }
    HIPCHK(hipGetLastError());
    for (size_t k = 0; k < h->groups.size(); k++) if (runs[k].second) HIPCHK(hipStreamSynchronize(h->groups[k].stream));
    return VIO_OK;
}
static void snapshot_fill_header(const vio_batch *h, unsigned char *blob, int64_t host_bytes) {
    vio_snapshot_header hd;
    memset(&hd, 0, sizeof(hd));
    hd.magic = VIO_SNAPSHOT_MAGIC; hd.format_version = VIO_SNAPSHOT_FORMAT; hd.abi_version = (uint32_t)vio_abi_version();
    hd.device_bytes = h->snap_dev_bytes; hd.host_bytes = host_bytes; hd.total_bytes = (int64_t)sizeof(hd) + hd.device_bytes + hd.host_bytes;
    static thread_local BeSeq be;
    memcpy(&be, blob + sizeof(hd) + snapshot_row(h, "be")->blob_off, sizeof(BeSeq));
    hd.frames_processed = be.frames_processed; hd.last_stamp = be.cur_stamp; hd.solver_flag = be.solver_flag;
    hd.tracker_lag = h->tracker_lag;
    snapshot_handle_shape(h, &hd.shape);
    memcpy(blob, &hd, sizeof(hd));
}

int64_t vio_snapshot_bytes(vio_batch *h, int seq) {
    VIO_ENTER_MSG(h, seq, false, "vio_snapshot_bytes: seq out of range");
    if (!h->dyn.empty()) VIO_TRY(snapshot_quiesce(h, false));
    snapshot_build_layout(h);
    return (int64_t)sizeof(vio_snapshot_header) + h->snap_dev_bytes + snapshot_host_bytes(h, seq);
}

int vio_save_seqs(vio_batch *h, int n, const int32_t *seqs, void *dst, const int64_t *offsets, const int64_t *caps, int64_t *bytes_out) {
    VIO_ENTER_MSG(h, VIO_NO_SEQ, false, "vio_save_seqs: bad arguments");
    if (n < 0 || (n > 0 && (!seqs || !dst || !offsets || !caps))) { g_err = "vio_save_seqs: bad arguments"; return VIO_EINVAL; }
    for (int i = 0; i < n; i++)
        if (seqs[i] < 0 || seqs[i] >= h->S) { g_err = "vio_save_seqs: seqs[" + std::to_string(i) + "] out of range"; return VIO_EINVAL; }
    if (n == 0) return VIO_OK;
    VIO_TRY(snapshot_quiesce(h, true));
    snapshot_build_layout(h);
    std::vector<int64_t> hostb(n), total(n), pos;
    for (int i = 0; i < n; i++) {
        hostb[i] = snapshot_host_bytes(h, seqs[i]);
        total[i] = (int64_t)sizeof(vio_snapshot_header) + h->snap_dev_bytes + hostb[i];
        if (offsets[i] < 0 || caps[i] < total[i]) { g_err = "vio_save_seqs: caps[" + std::to_string(i) + "] is smaller than vio_snapshot_bytes"; return VIO_ECAPACITY; }
    }
    int64_t span = 0;
    const bool tight = snapshot_place(n, offsets, total, pos, &span);
    VIO_TRY(snapshot_reserve(h, (size_t)n, (size_t)span));
    VIO_TRY(snapshot_launch(h, n, seqs, pos, true));
    unsigned char *out = (unsigned char *)dst;
    if (tight) HIPCHK(hipMemcpy(out + offsets[0], h->d_snap_stage, (size_t)span, hipMemcpyDeviceToHost));
    else
        for (int i = 0; i < n; i++)
            HIPCHK(hipMemcpy(out + offsets[i] + sizeof(vio_snapshot_header), h->d_snap_stage + pos[i] + sizeof(vio_snapshot_header), (size_t)h->snap_dev_bytes, hipMemcpyDeviceToHost));
    for (int i = 0; i < n; i++) {
        unsigned char *blob = out + offsets[i];
        snapshot_fill_header(h, blob, hostb[i]);
        snapshot_write_host(h, seqs[i], blob + sizeof(vio_snapshot_header) + h->snap_dev_bytes, hostb[i]);
        if (bytes_out) bytes_out[i] = total[i];
    }
    return VIO_OK;
}

int64_t vio_debug_save_seq_naive(vio_batch *h, int seq, void *dst, int64_t cap) {
    VIO_ENTER_MSG(h, seq, false, "vio_debug_save_seq_naive: bad arguments");
    if (!dst) { g_err = "vio_debug_save_seq_naive: bad arguments"; return VIO_EINVAL; }
    VIO_TRY(snapshot_quiesce(h, true));
    snapshot_build_layout(h);
    const int64_t hostb = snapshot_host_bytes(h, seq), total = (int64_t)sizeof(vio_snapshot_header) + h->snap_dev_bytes + hostb;
    if (cap < total) { g_err = "vio_debug_save_seq_naive: cap is smaller than vio_snapshot_bytes"; return VIO_ECAPACITY; }
    unsigned char *blob = (unsigned char *)dst, *dev = blob + sizeof(vio_snapshot_header);
    memset(dev, 0, (size_t)h->snap_dev_bytes);
    for (const auto &r : h->snap_rows)   // one copy per table entry: what the pack kernel replaces
        if (r.blob_off >= 0) HIPCHK(hipMemcpy(dev + r.blob_off, r.base + (int64_t)seq * r.bytes, (size_t)r.bytes, hipMemcpyDeviceToHost));
    snapshot_fill_header(h, blob, hostb);
    snapshot_write_host(h, seq, dev + h->snap_dev_bytes, hostb);
    return total;
}

int64_t vio_debug_snapshot_staging_bytes(vio_batch *h) {
    VIO_ENTER(h, VIO_NO_SEQ, false);
    return (int64_t)h->snap_stage_cap + (h->d_snap_tab ? 1 : 0) + (int64_t)h->snap_seqs_cap;
}

int vio_debug_snapshot_layout(vio_batch *h, int i, char *name64, int32_t *kind, int64_t *bytes_per_seq, int64_t *blob_offset) {
    VIO_ENTER(h, VIO_NO_SEQ, false);
    snapshot_build_layout(h);
    const int cnt = (int)h->snap_rows.size();
    if (i < 0 || i >= cnt) return cnt;
    const auto &r = h->snap_rows[i];
    if (name64) { strncpy(name64, r.name, 63); name64[63] = 0; }
    if (kind) *kind = r.kind;
    if (bytes_per_seq) *bytes_per_seq = r.bytes;
    if (blob_offset) *blob_offset = r.blob_off;
    return cnt;
}

int vio_load_seqs(vio_batch *h, int n, const int32_t *seqs, const void *src, const int64_t *offsets, const int64_t *bytes) {
    VIO_ENTER_MSG(h, VIO_NO_SEQ, false, "vio_load_seqs: bad arguments");
    if (n < 0 || (n > 0 && (!seqs || !src || !offsets || !bytes))) { g_err = "vio_load_seqs: bad arguments"; return VIO_EINVAL; }
    if (n == 0) return VIO_OK;
    // ---- validation first: nothing below this block runs after a refusal, so every slot is left untouched
    for (int i = 0; i < n; i++) {
        if (seqs[i] < 0 || seqs[i] >= h->S) { g_err = "vio_load_seqs: seqs[" + std::to_string(i) + "] out of range"; return VIO_EINVAL; }
        for (int j = 0; j < i; j++)
            if (seqs[j] == seqs[i]) { g_err = "vio_load_seqs: seqs[" + std::to_string(i) + "] is a duplicate slot"; return VIO_EINVAL; }
    }
    snapshot_build_layout(h);
    vio_snapshot_shape mine;
    snapshot_handle_shape(h, &mine);
    const unsigned char *in = (const unsigned char *)src;
    std::vector<int64_t> total(n), pos;
    std::vector<double> imu_t(n);
    std::vector<vio_batch::DynSeq> dyn(h->dyn.empty() ? 0 : n);
    std::vector<vio_calibration> cals(n);
    std::vector<vio_camera> cams(n);
    bool relo_pending = false;
    for (int i = 0; i < n; i++) {
        const std::string at = "vio_load_seqs: blob " + std::to_string(i) + ": ";
        if (offsets[i] < 0) { g_err = at + "negative offset"; return VIO_EINVAL; }
        const unsigned char *blob = in + offsets[i];
        vio_snapshot_header hd;
        if (vio_snapshot_info(blob, bytes[i], &hd) != VIO_OK) { g_err = at + g_err; return VIO_EINVAL; }
        if ((int)hd.abi_version > vio_abi_version()) { g_err = at + "abi_version " + std::to_string(hd.abi_version) + " is newer than this library"; return VIO_EINVAL; }
        if (const char *f = snap_shape_diff(hd.shape, mine)) { g_err = at + "shape key differs from the handle's in " + f; return VIO_EINVAL; }
        if (hd.tracker_lag != h->tracker_lag) { g_err = at + "tracker_lag " + std::to_string(hd.tracker_lag) + " differs from the handle's " + std::to_string(h->tracker_lag); return VIO_EINVAL; }
        if (hd.device_bytes != h->snap_dev_bytes) { g_err = at + "device_bytes does not match the handle's layout"; return VIO_EINVAL; }
        const unsigned char *dev = blob + sizeof(hd);
        memcpy(&cals[i], dev + snapshot_row(h, "cal")->blob_off, sizeof(vio_calibration));
        memcpy(&cams[i], dev + snapshot_row(h, "cam (cam_of)")->blob_off, sizeof(vio_camera));
        std::string why = calibration_check(cals[i]);
        if (!why.empty()) { g_err = at + "calibration: " + why; return VIO_EINVAL; }
        why = camera_check(cams[i], h->hc.c.width, h->hc.c.height);
        if (!why.empty()) { g_err = at + "camera: " + why; return VIO_EINVAL; }
        why = snapshot_read_host(dev + hd.device_bytes, hd.host_bytes, !h->dyn.empty(), h->hc.NP, &imu_t[i], dyn.empty() ? nullptr : &dyn[i]);
        if (!why.empty()) { g_err = at + why; return VIO_EINVAL; }
        static thread_local BeSeq be;
        memcpy(&be, dev + snapshot_row(h, "be")->blob_off, sizeof(BeSeq));
        relo_pending = relo_pending || be.relo_info != 0;
        total[i] = hd.total_bytes;
    }
    // ---- write: synchronise like vio_reset_seq, drop what is staged on the host for these slots, scatter
    VIO_TRY(snapshot_quiesce(h, false));
    int64_t span = 0;
    const bool tight = snapshot_place(n, offsets, total, pos, &span);
    VIO_TRY(snapshot_reserve(h, (size_t)n, (size_t)span));
    if (tight) HIPCHK(hipMemcpy(h->d_snap_stage, in + offsets[0], (size_t)span, hipMemcpyHostToDevice));
    else
        for (int i = 0; i < n; i++)
            HIPCHK(hipMemcpy(h->d_snap_stage + pos[i] + sizeof(vio_snapshot_header), in + offsets[i] + sizeof(vio_snapshot_header), (size_t)h->snap_dev_bytes, hipMemcpyHostToDevice));
    VIO_TRY(snapshot_launch(h, n, seqs, pos, false));
    {
        std::lock_guard<std::mutex> lk(h->imu_mu);
        auto loaded = [&](int s) { for (int i = 0; i < n; i++) if (seqs[i] == s) return true; return false; };
        size_t w = 0;
        for (size_t i = 0; i < h->p_seq.size(); i++) {
            if (loaded(h->p_seq[i])) continue;
            h->p_seq[w] = h->p_seq[i]; h->p_t[w] = h->p_t[i];
            for (int k = 0; k < 3; k++) { h->p_acc[3 * w + k] = h->p_acc[3 * i + k]; h->p_gyr[3 * w + k] = h->p_gyr[3 * i + k]; }
            w++;
        }
        h->p_seq.resize(w); h->p_t.resize(w); h->p_acc.resize(3 * w); h->p_gyr.resize(3 * w);
        for (int i = 0; i < n; i++) h->last_imu_t[seqs[i]] = imu_t[i];
    }
    for (int i = 0; i < n; i++) { h->cal[seqs[i]] = cals[i]; h->cam[seqs[i]] = cams[i]; }
    if (!h->dyn.empty()) {
        for (int i = 0; i < n; i++) h->dyn[seqs[i]] = std::move(dyn[i]);
        bool any = false;
        for (int s = 0; s < h->S; s++) any = any || !h->dyn[s].nonlinear;
        h->dyn_active = any;
    }
    if (relo_pending) h->relo_frames = 1 << 30;   // as vio_set_relo_frame: the pending request needs the two-kernel solver path launched
    return VIO_OK;
}

}  // extern "C"
