// Loop detection for a whole batch on the device, the keyframe databases resident in HBM (include/vio_posegraph.h, vio_pg_batch_*).
// One step = PoseGraph::detectLoop (pose_graph.cpp:308-393) + the descriptor search of KeyFrame::findConnection for S sequences, one chain of
// launches on the batch's stream, ordered by kernel boundaries alone:
//   pgb_blur / pgb_fast_score / pgb_fast_nms / pgb_brief_* / pgb_lift   vio_pg_describe's kernels with a sequence index (grid z, or one
//                        workgroup per sequence for the ordered compaction); the keypoint counts stay on the device, the BRIEF / lift
//                        launches are sized by max_keypoints and bounded by them; the per-sequence camera comes from a device table
//   pgb_walk_kernel      pg_voc_transform_kernel over [S][max_keypoints]: one wavefront per descriptor
//   pgb_bow_kernel       one workgroup per sequence: bow_vector() of pg_bow.hip.  Words of weight 0 dropped, bitonic sort in LDS of the keys
//                        (word << 13 | input index) -- unique, so the order is the stable sort's --, one thread per run of equal words sums its
//                        weights in input order (TF weightings) or keeps the first, one thread adds the L1 norm in ascending word order
//   pgb_score_kernel     one wavefront per (sequence, eligible entry): the lanes take query words and binary-search the entry's sorted words;
//                        the matched terms |q - r| - |q| - |r| are taken chunk by chunk in lane order (= ascending word id) and added
//                        serially: the order in which queryL1's inverted-file walk reaches that entry's accumulator
//   pgb_select_kernel    one workgroup per sequence: the four smallest (accumulator, entry id), the gates of vio_pg_detect_loop, then the append
//   pgb_match_kernel     pg_match_kernel's body, one wavefront per (sequence, window descriptor) against the candidate entry in the database
// The bodies shared with the per-keyframe entry points are in pg_device.h.  Every floating-point sum has one order, fixed by the reference;
// nothing here is reduced in a tree.
#include <hip/hip_runtime.h>

#include <climits>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/vio_posegraph.h"
#include "pg_device.h"
#include "pg_voc.h"

extern thread_local std::string g_err;   // vio_abi.hip

#define PGB_MAXKP 8192          // keys of the bag-of-words sort: (word << 13) | input index
#define PGB_NEV 8

namespace {

// what every kernel of the chain sees (passed by value)
struct Pgb {
    int S, K, MK, MW, W, H, thr, nchunk, weighting;
    long long A;                          // arena slots per sequence
    // database
    int *nent, *off, *nbow;               // [S], [S][K + 1], [S][K]
    unsigned long long *a_desc;           // [S][A][4]
    float *a_norm, *a_xy;                 // [S][A][2]
    int *a_bw;                            // [S][A]
    double *a_bv;                         // [S][A]
    // this step
    int *mode, *nfound, *nwin;            // [S] each
    const uint8_t *gray;                  // [S][H][W] (the batch's buffer or the caller's)
    uint8_t *blur, *score;
    unsigned long long *words;            // [S][nchunk]
    int *pat;
    const float *wuv;                     // [S][MW][2]
    unsigned long long *in_desc, *win_desc;   // [S][MK][4], [S][MW][4]
    float *in_norm, *in_xy;               // [S][MK][2]
    int *word; double *wgt;               // [S][MK]
    int *q_word; double *q_val; int *q_nbow;
    double *acc; int *hit;                // [S][K]
    const vio_config *cfg; const vio_camera *cam; const int *usecam;
    // tree
    const int *child_begin, *children, *node_word; const double *node_weight; const uint64_t *node_desc;
    // results
    vio_pg_step_out *out;                 // [S]
    int *best_index, *best_dist; float *old_norm;   // [S][MW], [S][MW], [S][MW][2]
};

__device__ __forceinline__ int pgb_kept(const Pgb &p, int s) { return min(p.nfound[s], p.MK); }
// this sequence adds an entry in this step: it has a keyframe, an entry slot and arena room for the keypoints it keeps
__device__ __forceinline__ bool pgb_adds(const Pgb &p, int s) {
    if (p.mode[s] == 0) return false;
    const int ne = p.nent[s];
    return ne < p.K && (long long)p.off[(size_t)s * (p.K + 1) + ne] + pgb_kept(p, s) <= p.A;
}

__global__ __launch_bounds__(256) void pgb_blur_kernel(Pgb p) {
    const int s = blockIdx.z;
    if (p.mode[s] == 0) return;
    const size_t hw = (size_t)p.W * p.H;
    pgdev::blur_tile(p.gray + s * hw, p.W, p.H, p.blur + s * hw);
}

__global__ __launch_bounds__(256) void pgb_fast_score_kernel(Pgb p) {
    const int s = blockIdx.z;
    if (p.mode[s] == 0) return;
    const size_t hw = (size_t)p.W * p.H;
    pgdev::fast_score_tile(p.gray + s * hw, p.W, p.H, p.thr, p.score + s * hw);
}

__global__ __launch_bounds__(1024) void pgb_fast_nms_kernel(Pgb p) {
    const int s = blockIdx.x;
    if (p.mode[s] == 0) return;
    const int total = pgdev::fast_nms_image(p.score + (size_t)s * p.W * p.H, p.W, p.H, p.words + (size_t)s * p.nchunk, p.in_xy + (size_t)s * p.MK * 2, p.MK);
    if (threadIdx.x == 0) p.nfound[s] = total;
}

// which = 0: the window points, 1: the FAST keypoints
__global__ __launch_bounds__(64) void pgb_brief_kernel(Pgb p, int which) {
    const int s = blockIdx.y, i = blockIdx.x;
    if (p.mode[s] == 0) return;
    const uint8_t *blur = p.blur + (size_t)s * p.W * p.H;
    if (which == 0) {
        if (i >= p.nwin[s]) return;
        pgdev::brief_point(blur, p.W, p.H, p.wuv + (size_t)s * p.MW * 2, i, p.pat, p.win_desc + (size_t)s * p.MW * 4);
    } else {
        if (i >= pgb_kept(p, s)) return;
        pgdev::brief_point(blur, p.W, p.H, p.in_xy + (size_t)s * p.MK * 2, i, p.pat, p.in_desc + (size_t)s * p.MK * 4);
    }
}

__global__ __launch_bounds__(256) void pgb_lift_kernel(Pgb p) {
    const int s = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x;
    if (p.mode[s] == 0 || i >= pgb_kept(p, s)) return;
    const float *xy = p.in_xy + (size_t)s * p.MK * 2;
    float *nrm = p.in_norm + (size_t)s * p.MK * 2;
    if (p.usecam[s]) pgdev::lift_camera(p.cam[s], xy, i, nrm);
    else pgdev::lift_pinhole(*p.cfg, xy, i, nrm);
}

__global__ __launch_bounds__(256) void pgb_walk_kernel(Pgb p) {
    const int s = blockIdx.y, i = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (!pgb_adds(p, s) || i >= pgb_kept(p, s)) return;
    const size_t q = (size_t)s * p.MK + i;
    const int node = pgdev::voc_walk((const uint64_t *)p.in_desc + q * 4, p.child_begin, p.children, p.node_desc);
    if ((threadIdx.x & 63) == 0) { p.word[q] = p.node_word[node]; p.wgt[q] = p.node_weight[node]; }
}

// TemplatedVocabulary::transform(features, BowVector) for an L1-scored vocabulary = bow_vector() of pg_bow.hip, one workgroup per sequence
__global__ __launch_bounds__(1024) void pgb_bow_kernel(Pgb p) {
    __shared__ unsigned long long keys[PGB_MAXKP];
    __shared__ double vals[PGB_MAXKP];
    __shared__ int scan[2][1024];
    __shared__ double s_norm;
    const int s = blockIdx.x, t = threadIdx.x;
    if (!pgb_adds(p, s)) return;
    const int n = pgb_kept(p, s);
    const int *word = p.word + (size_t)s * p.MK;
    const double *wgt = p.wgt + (size_t)s * p.MK;
    const bool tf = p.weighting == 0 /*TF_IDF*/ || p.weighting == 1 /*TF*/;
    int P = 1;
    while (P < n) P <<= 1;
    const unsigned long long NONE = ~0ULL;
    for (int i = t; i < P; i += 1024) {
        unsigned long long key = NONE;
        if (i < n && wgt[i] > 0) key = ((unsigned long long)(unsigned)word[i] << 13) | (unsigned)i;   // stopped words carry weight 0
        keys[i] = key;
    }
    __syncthreads();
    for (int k = 2; k <= P; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int i = t; i < P; i += 1024) {
                const int x = i ^ j;
                if (x > i) {
                    const unsigned long long a = keys[i], b = keys[x];
                    if ((a > b) == ((i & k) == 0)) { keys[i] = b; keys[x] = a; }
                }
            }
            __syncthreads();
        }
    // heads of the runs of equal words, counted per thread over a contiguous range, then an exclusive scan of the 1024 counts
    const int per = P > 1024 ? P >> 10 : 1, lo = t * per, hi = min(P, lo + per);
    int heads = 0;
    for (int j = lo; j < hi; j++) {
        const unsigned long long k = keys[j];
        if (k != NONE && (j == 0 || (keys[j - 1] >> 13) != (k >> 13))) heads++;
    }
    scan[0][t] = heads;
    __syncthreads();
    int cur = 0;
    for (int d = 1; d < 1024; d <<= 1) {
        scan[cur ^ 1][t] = scan[cur][t] + (t >= d ? scan[cur][t - d] : 0);
        cur ^= 1;
        __syncthreads();
    }
    const int m = scan[cur][1023];
    int pos = scan[cur][t] - heads;
    for (int j = lo; j < hi; j++) {
        const unsigned long long k = keys[j];
        if (k != NONE && (j == 0 || (keys[j - 1] >> 13) != (k >> 13))) {
            double val = wgt[k & 0x1FFF];                  // addWeight's first insert / addIfNotExist
            for (int r = j + 1; r < P; r++) {
                const unsigned long long kr = keys[r];
                if (kr == NONE || (kr >> 13) != (k >> 13)) break;
                if (tf) val += wgt[kr & 0x1FFF];           // the features of one word in input order
            }
            p.q_word[(size_t)s * p.MK + pos] = (int)(k >> 13);
            vals[pos] = val;
            pos++;
        }
    }
    __syncthreads();
    if (t == 0) {                                          // BowVector::normalize(L1): ascending word order
        double norm = 0.0;
        for (int j = 0; j < m; j++) norm += fabs(vals[j]);
        s_norm = norm;
        p.q_nbow[s] = m;
    }
    __syncthreads();
    const double norm = s_norm;
    for (int j = t; j < m; j += 1024) p.q_val[(size_t)s * p.MK + j] = norm > 0.0 ? vals[j] / norm : vals[j];
}

// queryL1's accumulator of one entry: the terms of the words common to query and entry, in ascending word id
__global__ __launch_bounds__(256) void pgb_score_kernel(Pgb p) {
    const int s = blockIdx.y, e = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (p.mode[s] != 1 || !pgb_adds(p, s)) return;
    const int nent = p.nent[s];
    if (e >= nent) return;
    const int max_id = nent - 50;                          // frame_index = the sequence's entry counter
    const size_t se = (size_t)s * p.K + e;
    if (!(e < max_id || max_id == -1 || e == nent - 1)) { if (lane == 0) p.hit[se] = 0; return; }
    const size_t base = (size_t)s * p.A + p.off[(size_t)s * (p.K + 1) + e];
    const int nb = p.nbow[se], nq = p.q_nbow[s];
    const int *ew = p.a_bw + base;
    const double *ev = p.a_bv + base;
    const int *qw = p.q_word + (size_t)s * p.MK;
    const double *qv = p.q_val + (size_t)s * p.MK;
    double acc = 0.0;
    bool first = true;
    for (int c = 0; c < nq; c += 64) {
        const int i = c + lane;
        bool found = false;
        double term = 0.0;
        if (i < nq) {
            const int w = qw[i];
            int lo = 0, hi = nb;
            while (lo < hi) { const int mid = (lo + hi) >> 1; if (ew[mid] < w) lo = mid + 1; else hi = mid; }
            if (lo < nb && ew[lo] == w) {
                const double q = qv[i], r = ev[lo];
                term = fabs(q - r) - fabs(q) - fabs(r);
                found = true;
            }
        }
        unsigned long long bal = __ballot(found);
        while (bal) {
            const int l = __ffsll((long long)bal) - 1;
            bal &= bal - 1;
            const double v = __shfl(term, l, 64);
            if (first) { acc = v; first = false; } else acc += v;
        }
    }
    if (lane == 0) { p.acc[se] = acc; p.hit[se] = first ? 0 : 1; }
}

// query(4, frame_index - 50)'s result list, detectLoop's gates, then BriefDatabase::add with the keyframe's descriptors and keypoints
__global__ __launch_bounds__(256) void pgb_select_kernel(Pgb p) {
    const int s = blockIdx.x, t = threadIdx.x;
    const int mode = p.mode[s];
    if (mode == 0) return;
    const int nent = p.nent[s], nfound = p.nfound[s], kept = pgb_kept(p, s);
    const bool adds = pgb_adds(p, s);
    vio_pg_step_out *o = p.out + s;
    if (!adds) {
        if (t == 0) {
            o->status = VIO_ECAPACITY; o->entry = nent; o->n_kp = nfound; o->n_bow = 0; o->n_ret = 0; o->loop_index = -1; o->n_match = 0;
            for (int r = 0; r < 4; r++) { o->ids4[r] = 0; o->scores4[r] = 0.0; }
        }
        return;
    }
    const int nb = p.q_nbow[s];
    const int fill = p.off[(size_t)s * (p.K + 1) + nent];
    if (t < 64) {
        int ids[4] = {0, 0, 0, 0}, n_ret = 0;
        double sc[4] = {0.0, 0.0, 0.0, 0.0};
        if (mode == 1) {
            const double *acc = p.acc + (size_t)s * p.K;
            const int *hit = p.hit + (size_t)s * p.K;
            double pa = 0.0; int pe = -1;                  // the pair taken last; ties go to the entry id
            for (int r = 0; r < 4; r++) {
                double a = 0.0; int e = -1;
                for (int q = t; q < nent; q += 64) {
                    if (!hit[q]) continue;
                    const double aq = acc[q];
                    if (pe >= 0 && !(aq > pa || (aq == pa && q > pe))) continue;
                    if (e < 0 || aq < a) { a = aq; e = q; }   // ascending q: an equal accumulator keeps the smaller id
                }
                for (int d = 32; d > 0; d >>= 1) {
                    const double oa = __shfl_xor(a, d, 64);
                    const int oe = __shfl_xor(e, d, 64);
                    if (oe >= 0 && (e < 0 || oa < a || (oa == a && oe < e))) { a = oa; e = oe; }
                }
                if (e < 0) break;
                ids[r] = e; sc[r] = -a / 2.0; n_ret = r + 1;
                pa = a; pe = e;
            }
        }
        if (t == 0) {
            int loop_index = -1;
            bool find_loop = false;
            if (n_ret >= 1 && sc[0] > 0.05)
                for (int i = 1; i < n_ret; i++)
                    if (sc[i] > 0.015) find_loop = true;
            if (find_loop && nent > 50) {
                int min_index = -1;
                for (int i = 0; i < n_ret; i++)
                    if (min_index == -1 || (ids[i] < min_index && sc[i] > 0.015)) min_index = ids[i];
                loop_index = min_index;
            }
            o->status = VIO_OK; o->entry = nent; o->n_kp = nfound; o->n_bow = nb; o->n_ret = n_ret; o->loop_index = loop_index; o->n_match = 0;
            for (int r = 0; r < 4; r++) { o->ids4[r] = ids[r]; o->scores4[r] = sc[r]; }
        }
    }
    __syncthreads();                                       // every thread has read nent
    const size_t dst = (size_t)s * p.A + fill, src = (size_t)s * p.MK;
    for (int i = t; i < kept * 4; i += 256) p.a_desc[dst * 4 + i] = p.in_desc[src * 4 + i];
    for (int i = t; i < kept * 2; i += 256) { p.a_norm[dst * 2 + i] = p.in_norm[src * 2 + i]; p.a_xy[dst * 2 + i] = p.in_xy[src * 2 + i]; }
    for (int i = t; i < nb; i += 256) { p.a_bw[dst + i] = p.q_word[src + i]; p.a_bv[dst + i] = p.q_val[src + i]; }
    if (t == 0) {
        p.off[(size_t)s * (p.K + 1) + nent + 1] = fill + kept;
        p.nbow[(size_t)s * p.K + nent] = nb;
        p.nent[s] = nent + 1;
    }
}

__global__ __launch_bounds__(64) void pgb_match_kernel(Pgb p) {
    const int s = blockIdx.y, i = blockIdx.x;
    if (p.mode[s] != 1) return;
    vio_pg_step_out *o = p.out + s;
    if (o->status != VIO_OK) return;
    const int li = o->loop_index;
    if (li < 0 || i >= p.nwin[s]) return;
    const int *off = p.off + (size_t)s * (p.K + 1);
    const int co = off[li], m = off[li + 1] - co;
    const size_t base = (size_t)s * p.A + co;
    const int key = pgdev::match_scan(p.win_desc + ((size_t)s * p.MW + i) * 4, p.a_desc + base * 4, m);
    if (threadIdx.x == 0) {
        const int bi = pgdev::match_index(key);
        const size_t q = (size_t)s * p.MW + i;
        p.best_dist[q] = key >> 20;
        p.best_index[q] = bi;
        p.old_norm[2 * q] = bi >= 0 ? p.a_norm[(base + bi) * 2] : 0.f;
        p.old_norm[2 * q + 1] = bi >= 0 ? p.a_norm[(base + bi) * 2 + 1] : 0.f;
        if (bi >= 0) atomicAdd(&o->n_match, 1);            // an integer count: the order of the additions does not matter
    }
}

}  // namespace

struct vio_pg_batch {
    Pgb p{};
    vio_config cfg{};
    vio_pg_voc *voc = nullptr;
    hipStream_t st = nullptr;
    std::vector<void *> dev;                               // every device allocation
    uint8_t *d_gray = nullptr; float *d_wuv = nullptr;     // the batch's own input buffers
    vio_config *d_cfg = nullptr; vio_camera *d_cam = nullptr; int *d_usecam = nullptr;
    int *d_ctl = nullptr, *h_ctl = nullptr;                // mode | nfound | nwin, [3][S]; h_ctl page-locked
    char *d_res = nullptr, *h_res = nullptr;               // out [S] | best_index | best_dist | old_norm; h_res page-locked
    size_t res_out = 0, res_all = 0;
    std::vector<int> h_ent;                                // entries per sequence (the only host state; fixed size)
    bool timing = false;
    hipEvent_t ev[PGB_NEV + 1] = {};
    float ms[PGB_NEV] = {};
};

namespace {

#define PGBCHK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { g_err = std::string(#x) + ": " + hipGetErrorString(e_); return VIO_EDEVICE; } } while (0)

template <typename T> bool dalloc(vio_pg_batch *b, T *&ptr, size_t count) {
    void *q = nullptr;
    if (hipMalloc(&q, (count ? count : 1) * sizeof(T)) != hipSuccess) return false;
    b->dev.push_back(q);
    ptr = (T *)q;
    return true;
}

void batch_free(vio_pg_batch *b) {
    if (!b) return;
    if (b->st) (void)hipStreamSynchronize(b->st);
    for (void *q : b->dev) (void)hipFree(q);
    if (b->h_ctl) (void)hipHostFree(b->h_ctl);
    if (b->h_res) (void)hipHostFree(b->h_res);
    for (hipEvent_t e : b->ev) if (e) (void)hipEventDestroy(e);
    if (b->st) (void)hipStreamDestroy(b->st);
    delete b;
}

void mark(vio_pg_batch *b, int i) { if (b->timing) (void)hipEventRecord(b->ev[i], b->st); }

// mode / n_win (and n_kp when the caller gives it) checked and staged; returns VIO_EINVAL before anything is launched
int stage_ctl(vio_pg_batch *b, const uint8_t *mode, const int32_t *n_kp, const int32_t *n_win) {
    const int S = b->p.S;
    for (int s = 0; s < S; s++) {
        if (mode[s] > 2) { g_err = "vio_pg_batch_step: mode must be 0, 1 or 2"; return VIO_EINVAL; }
        if (mode[s] == 0) continue;
        if (n_kp && (n_kp[s] < 0 || n_kp[s] > b->p.MK)) { g_err = "vio_pg_batch_step: n_kp outside 0 .. max_keypoints"; return VIO_EINVAL; }
        if (n_win[s] < 0 || n_win[s] > b->p.MW) { g_err = "vio_pg_batch_step: n_win outside 0 .. max_window"; return VIO_EINVAL; }
    }
    for (int s = 0; s < S; s++) {
        b->h_ctl[s] = mode[s];
        b->h_ctl[S + s] = (mode[s] && n_kp) ? n_kp[s] : 0;
        b->h_ctl[2 * S + s] = mode[s] ? n_win[s] : 0;
    }
    return VIO_OK;
}

// the chain after the descriptors are in place (in_desc, in_norm, in_xy, win_desc, ctl), the one wait and the one copy back
int run_chain(vio_pg_batch *b, const uint8_t *mode, int on_device, vio_pg_step_out *out, int32_t *best_index, int32_t *best_dist, float *old_norm) {
    Pgb p = b->p;
    const int S = p.S, MW = p.MW;
    if (on_device) { p.best_index = best_index; p.best_dist = best_dist; p.old_norm = old_norm; }
    int deepest = 0;                                       // launch width of the score kernel: the deepest queried database
    for (int s = 0; s < S; s++) if (mode[s] == 1 && b->h_ent[s] > deepest) deepest = b->h_ent[s];
    mark(b, 1);
    pgb_walk_kernel<<<dim3((p.MK + 3) / 4, S), 256, 0, b->st>>>(p);
    mark(b, 2);
    pgb_bow_kernel<<<S, 1024, 0, b->st>>>(p);
    mark(b, 3);
    if (deepest > 0) pgb_score_kernel<<<dim3((deepest + 3) / 4, S), 256, 0, b->st>>>(p);
    mark(b, 4);
    pgb_select_kernel<<<S, 256, 0, b->st>>>(p);
    mark(b, 5);
    if (MW > 0) pgb_match_kernel<<<dim3(MW, S), 64, 0, b->st>>>(p);
    mark(b, 6);
    PGBCHK(hipGetLastError());
    PGBCHK(hipMemcpyAsync(b->h_res, b->d_res, on_device ? b->res_out : b->res_all, hipMemcpyDeviceToHost, b->st));
    mark(b, 7);
    PGBCHK(hipStreamSynchronize(b->st));
    if (b->timing) {
        for (int i = 0; i < 7; i++) (void)hipEventElapsedTime(&b->ms[i], b->ev[i], b->ev[i + 1]);
        (void)hipEventElapsedTime(&b->ms[7], b->ev[0], b->ev[7]);
    }
    const vio_pg_step_out *ho = (const vio_pg_step_out *)b->h_res;
    const int32_t *hbi = (const int32_t *)(b->h_res + b->res_out), *hbd = hbi + (size_t)S * MW;
    const float *hon = (const float *)(hbd + (size_t)S * MW);
    for (int s = 0; s < S; s++) {
        if (mode[s] == 0) continue;
        out[s] = ho[s];
        if (ho[s].status == VIO_OK) b->h_ent[s]++;
        const int nw = b->h_ctl[2 * S + s];
        if (!on_device && ho[s].status == VIO_OK && ho[s].loop_index != -1 && nw > 0) {
            std::memcpy(best_index + (size_t)s * MW, hbi + (size_t)s * MW, (size_t)nw * 4);
            std::memcpy(best_dist + (size_t)s * MW, hbd + (size_t)s * MW, (size_t)nw * 4);
            std::memcpy(old_norm + (size_t)s * MW * 2, hon + (size_t)s * MW * 2, (size_t)nw * 8);
        }
    }
    return VIO_OK;
}

bool step_args_ok(vio_pg_batch *b, const uint8_t *mode, const int32_t *n_win, vio_pg_step_out *out, int32_t *best_index, int32_t *best_dist,
                  float *old_norm) {
    if (!b || !mode || !n_win || !out) return false;
    return b->p.MW == 0 || (best_index && best_dist && old_norm);
}

}  // namespace

extern "C" {

vio_pg_batch *vio_pg_batch_create_arena(const vio_config *cfg, vio_pg_voc *voc, int S, int max_keyframes, int max_keypoints, int max_window,
                                        const int32_t *pattern1024, int fast_threshold, int64_t arena_keypoints) {
    if (!cfg || !voc || !pattern1024 || S < 1 || max_keyframes < 1 || max_keypoints < 1 || max_keypoints > PGB_MAXKP || max_window < 0 ||
        arena_keypoints < max_keypoints || arena_keypoints > INT_MAX) {
        g_err = "vio_pg_batch_create: bad argument (NULL, S / max_keyframes / max_keypoints < 1, max_keypoints > 8192 or an arena below max_keypoints)";
        return nullptr;
    }
    const int W = cfg->width, H = cfg->height;
    if (W < 16 || H < 16 || W > 4095 || H > 4095 || fast_threshold < 1 || fast_threshold > 254) { g_err = "vio_pg_batch_create: image size or FAST threshold out of range"; return nullptr; }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) { g_err = "no HIP device: the batched loop detection has no CPU fallback"; return nullptr; }
    vio_pg_batch *b = new vio_pg_batch();
    b->cfg = *cfg; b->voc = voc;
    Pgb &p = b->p;
    p.S = S; p.K = max_keyframes; p.MK = max_keypoints; p.MW = max_window; p.W = W; p.H = H; p.thr = fast_threshold;
    p.nchunk = ((W - 6) * (H - 6) + 63) / 64; p.weighting = voc->weighting; p.A = arena_keypoints;
    const size_t K = (size_t)p.K, MK = (size_t)p.MK, MW = (size_t)p.MW, A = (size_t)p.A, hw = (size_t)W * H, s_ = (size_t)S;
    b->res_out = s_ * sizeof(vio_pg_step_out);
    b->res_all = b->res_out + s_ * MW * 16;
    bool ok = hipStreamCreate(&b->st) == hipSuccess;
    for (int i = 0; ok && i <= PGB_NEV; i++) ok = hipEventCreate(&b->ev[i]) == hipSuccess;
    ok = ok && hipHostMalloc((void **)&b->h_ctl, 3 * s_ * sizeof(int)) == hipSuccess && hipHostMalloc((void **)&b->h_res, b->res_all) == hipSuccess;
    ok = ok && dalloc(b, p.nent, s_) && dalloc(b, p.off, s_ * (K + 1)) && dalloc(b, p.nbow, s_ * K) && dalloc(b, p.a_desc, s_ * A * 4) &&
         dalloc(b, p.a_norm, s_ * A * 2) && dalloc(b, p.a_xy, s_ * A * 2) && dalloc(b, p.a_bw, s_ * A) && dalloc(b, p.a_bv, s_ * A) &&
         dalloc(b, b->d_ctl, 3 * s_) && dalloc(b, b->d_gray, s_ * hw) && dalloc(b, p.blur, s_ * hw) && dalloc(b, p.score, s_ * hw) &&
         dalloc(b, p.words, s_ * p.nchunk) && dalloc(b, p.pat, 1024) && dalloc(b, b->d_wuv, s_ * MW * 2) && dalloc(b, p.in_desc, s_ * MK * 4) &&
         dalloc(b, p.win_desc, s_ * MW * 4) && dalloc(b, p.in_norm, s_ * MK * 2) && dalloc(b, p.in_xy, s_ * MK * 2) && dalloc(b, p.word, s_ * MK) &&
         dalloc(b, p.wgt, s_ * MK) && dalloc(b, p.q_word, s_ * MK) && dalloc(b, p.q_val, s_ * MK) && dalloc(b, p.q_nbow, s_) && dalloc(b, p.acc, s_ * K) &&
         dalloc(b, p.hit, s_ * K) && dalloc(b, b->d_cfg, 1) && dalloc(b, b->d_cam, s_) && dalloc(b, b->d_usecam, s_) && dalloc(b, b->d_res, b->res_all);
    if (ok) {
        p.mode = b->d_ctl; p.nfound = b->d_ctl + S; p.nwin = b->d_ctl + 2 * S;
        p.gray = b->d_gray; p.wuv = b->d_wuv; p.cfg = b->d_cfg; p.cam = b->d_cam; p.usecam = b->d_usecam;
        p.child_begin = voc->d_child_begin; p.children = voc->d_children; p.node_word = voc->d_node_word; p.node_weight = voc->d_node_weight;
        p.node_desc = voc->d_node_desc;
        p.out = (vio_pg_step_out *)b->d_res;
        p.best_index = (int *)(b->d_res + b->res_out); p.best_dist = p.best_index + s_ * MW; p.old_norm = (float *)(p.best_dist + s_ * MW);
        ok = hipMemset(p.nent, 0, s_ * sizeof(int)) == hipSuccess && hipMemset(p.off, 0, s_ * (K + 1) * sizeof(int)) == hipSuccess &&
             hipMemset(b->d_usecam, 0, s_ * sizeof(int)) == hipSuccess && hipMemset(b->d_cam, 0, s_ * sizeof(vio_camera)) == hipSuccess &&
             hipMemset(b->d_res, 0, b->res_all) == hipSuccess && hipMemset(p.in_xy, 0, s_ * MK * 8) == hipSuccess &&
             hipMemcpy(p.pat, pattern1024, 1024 * 4, hipMemcpyHostToDevice) == hipSuccess &&
             hipMemcpy(b->d_cfg, cfg, sizeof(vio_config), hipMemcpyHostToDevice) == hipSuccess;
    }
    if (!ok) { g_err = "vio_pg_batch_create: device allocation failed (the arenas take 60 B x arena_keypoints x S)"; batch_free(b); return nullptr; }
    b->h_ent.assign(s_, 0);
    return b;
}

vio_pg_batch *vio_pg_batch_create(const vio_config *cfg, vio_pg_voc *voc, int S, int max_keyframes, int max_keypoints, int max_window,
                                  const int32_t *pattern1024, int fast_threshold) {
    const int64_t worst = (int64_t)(max_keyframes > 0 ? max_keyframes : 0) * (max_keypoints > 0 ? max_keypoints : 0);
    return vio_pg_batch_create_arena(cfg, voc, S, max_keyframes, max_keypoints, max_window, pattern1024, fast_threshold, worst);
}

void vio_pg_batch_destroy(vio_pg_batch *b) { batch_free(b); }

int vio_pg_batch_set_camera(vio_pg_batch *b, int seq, const vio_camera *cam) {
    if (!b || !cam || seq < 0 || seq >= b->p.S) return VIO_EINVAL;
    const int one = 1;
    PGBCHK(hipMemcpy(b->d_cam + seq, cam, sizeof(vio_camera), hipMemcpyHostToDevice));
    PGBCHK(hipMemcpy(b->d_usecam + seq, &one, sizeof(int), hipMemcpyHostToDevice));
    return VIO_OK;
}

int vio_pg_batch_reset_seq(vio_pg_batch *b, int seq) {
    if (!b || seq < 0 || seq >= b->p.S) return VIO_EINVAL;
    PGBCHK(hipMemset(b->p.nent + seq, 0, sizeof(int)));   // off[seq][0] stays 0: the arena is empty again
    b->h_ent[(size_t)seq] = 0;
    return VIO_OK;
}

int vio_pg_batch_step_desc(vio_pg_batch *b, const uint8_t *mode, const int32_t *n_kp, const uint64_t *kp_desc, const float *kp_norm,
                           const int32_t *n_win, const uint64_t *win_desc, int on_device, vio_pg_step_out *out,
                           int32_t *best_index, int32_t *best_dist, float *old_norm) {
    if (!step_args_ok(b, mode, n_win, out, best_index, best_dist, old_norm) || !n_kp || !kp_desc || !kp_norm || (b->p.MW > 0 && !win_desc)) return VIO_EINVAL;
    if (int rc = stage_ctl(b, mode, n_kp, n_win)) return rc;
    const Pgb &p = b->p;
    const size_t s_ = (size_t)p.S, MK = (size_t)p.MK, MW = (size_t)p.MW;
    const hipMemcpyKind kind = on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
    mark(b, 0);
    PGBCHK(hipMemcpyAsync(b->d_ctl, b->h_ctl, 3 * s_ * sizeof(int), hipMemcpyHostToDevice, b->st));
    PGBCHK(hipMemcpyAsync(p.in_desc, kp_desc, s_ * MK * 32, kind, b->st));
    PGBCHK(hipMemcpyAsync(p.in_norm, kp_norm, s_ * MK * 8, kind, b->st));
    PGBCHK(hipMemsetAsync(p.in_xy, 0, s_ * MK * 8, b->st));
    if (MW > 0) PGBCHK(hipMemcpyAsync(p.win_desc, win_desc, s_ * MW * 32, kind, b->st));
    return run_chain(b, mode, on_device, out, best_index, best_dist, old_norm);
}

int vio_pg_batch_step(vio_pg_batch *b, const uint8_t *mode, const uint8_t *gray, const int32_t *n_win, const float *win_uv, int on_device,
                      vio_pg_step_out *out, int32_t *best_index, int32_t *best_dist, float *old_norm) {
    if (!step_args_ok(b, mode, n_win, out, best_index, best_dist, old_norm) || !gray || (b->p.MW > 0 && !win_uv)) return VIO_EINVAL;
    if (int rc = stage_ctl(b, mode, nullptr, n_win)) return rc;
    Pgb p = b->p;
    const size_t s_ = (size_t)p.S, MW = (size_t)p.MW, hw = (size_t)p.W * p.H;
    mark(b, 0);
    PGBCHK(hipMemcpyAsync(b->d_ctl, b->h_ctl, 3 * s_ * sizeof(int), hipMemcpyHostToDevice, b->st));
    if (on_device) { p.gray = gray; p.wuv = win_uv; }
    else {
        PGBCHK(hipMemcpyAsync(b->d_gray, gray, s_ * hw, hipMemcpyHostToDevice, b->st));
        if (MW > 0) PGBCHK(hipMemcpyAsync(b->d_wuv, win_uv, s_ * MW * 8, hipMemcpyHostToDevice, b->st));
    }
    const dim3 tiles((p.W + PG_TW - 1) / PG_TW, (p.H + PG_TH - 1) / PG_TH, p.S);
    pgb_blur_kernel<<<tiles, 256, 0, b->st>>>(p);
    pgb_fast_score_kernel<<<tiles, 256, 0, b->st>>>(p);
    if (MW > 0) pgb_brief_kernel<<<dim3(p.MW, p.S), 64, 0, b->st>>>(p, 0);
    pgb_fast_nms_kernel<<<p.S, 1024, 0, b->st>>>(p);
    pgb_brief_kernel<<<dim3(p.MK, p.S), 64, 0, b->st>>>(p, 1);
    pgb_lift_kernel<<<dim3((p.MK + 255) / 256, p.S), 256, 0, b->st>>>(p);
    return run_chain(b, mode, on_device, out, best_index, best_dist, old_norm);
}

int vio_pg_batch_get_entry(vio_pg_batch *b, int seq, int entry, int32_t *counts2, float *kp_xy, uint64_t *kp_desc, float *kp_norm,
                           int32_t *bow_word, double *bow_value) {
    if (!b || seq < 0 || seq >= b->p.S || entry < 0 || entry >= b->h_ent[(size_t)seq]) return VIO_EINVAL;
    const Pgb &p = b->p;
    int off2[2] = {0, 0}, nb = 0;
    PGBCHK(hipMemcpy(off2, p.off + (size_t)seq * (p.K + 1) + entry, 2 * sizeof(int), hipMemcpyDeviceToHost));
    PGBCHK(hipMemcpy(&nb, p.nbow + (size_t)seq * p.K + entry, sizeof(int), hipMemcpyDeviceToHost));
    const size_t base = (size_t)seq * p.A + off2[0], n = (size_t)(off2[1] - off2[0]);
    if (counts2) { counts2[0] = (int32_t)n; counts2[1] = nb; }
    if (n > 0 && kp_xy) PGBCHK(hipMemcpy(kp_xy, p.a_xy + base * 2, n * 8, hipMemcpyDeviceToHost));
    if (n > 0 && kp_desc) PGBCHK(hipMemcpy(kp_desc, p.a_desc + base * 4, n * 32, hipMemcpyDeviceToHost));
    if (n > 0 && kp_norm) PGBCHK(hipMemcpy(kp_norm, p.a_norm + base * 2, n * 8, hipMemcpyDeviceToHost));
    if (nb > 0 && bow_word) PGBCHK(hipMemcpy(bow_word, p.a_bw + base, (size_t)nb * 4, hipMemcpyDeviceToHost));
    if (nb > 0 && bow_value) PGBCHK(hipMemcpy(bow_value, p.a_bv + base, (size_t)nb * 8, hipMemcpyDeviceToHost));
    return VIO_OK;
}

int vio_pg_batch_info(vio_pg_batch *b, int32_t *entries) {
    if (!b || !entries) return VIO_EINVAL;
    PGBCHK(hipMemcpy(entries, b->p.nent, (size_t)b->p.S * sizeof(int), hipMemcpyDeviceToHost));   // the device's counters, not the host's mirror
    return VIO_OK;
}

int vio_pg_batch_set_timing(vio_pg_batch *b, int on) {
    if (!b) return VIO_EINVAL;
    b->timing = on != 0;
    return VIO_OK;
}

int vio_pg_batch_last_timing(vio_pg_batch *b, float *ms8) {
    if (!b || !ms8) return VIO_EINVAL;
    for (int i = 0; i < PGB_NEV; i++) ms8[i] = b->ms[i];
    return VIO_OK;
}

}  // extern "C"
