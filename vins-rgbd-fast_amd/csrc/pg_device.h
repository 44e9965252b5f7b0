// Device bodies of the loop-closure kernels, shared by the single-image entry points (pg_kernels.hip, pg_bow.hip) and the batched ones
// (pg_batch.hip): one copy of the arithmetic, so that the batch computes the per-keyframe path's results bit for bit.  Every body is written
// for the launch shape its kernel documents; the caller passes the pointers of its own image / sequence.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/vio_posegraph.h"
#include "camera_model.h"

#define PG_TW 64
#define PG_TH 16

namespace pgdev {

__device__ __forceinline__ int refl101(int i, int n) { return i < 0 ? -i : (i >= n ? 2 * n - 2 - i : i); }

// separable 9-tap Gaussian, 8 fractional bits per pass (52 46 32 17 7 | sum 256), one rounding: (v + 2^15) >> 16.  256 threads, tile
// (blockIdx.x, blockIdx.y) of 64 x 16 pixels.
__device__ __forceinline__ void blur_tile(const uint8_t *src, int W, int H, uint8_t *dst) {
    __shared__ uint8_t tile[PG_TH + 8][PG_TW + 8];
    __shared__ int hrow[PG_TH + 8][PG_TW];
    const int ox = blockIdx.x * PG_TW, oy = blockIdx.y * PG_TH;
    for (int q = threadIdx.x; q < (PG_TH + 8) * (PG_TW + 8); q += 256) {
        const int ty = q / (PG_TW + 8), tx = q - ty * (PG_TW + 8);
        const int gy = min(max(refl101(oy + ty - 4, H), 0), H - 1), gx = min(max(refl101(ox + tx - 4, W), 0), W - 1);
        tile[ty][tx] = src[(size_t)gy * W + gx];
    }
    __syncthreads();
    for (int q = threadIdx.x; q < (PG_TH + 8) * PG_TW; q += 256) {
        const int ty = q / PG_TW, x = q - ty * PG_TW;
        const uint8_t *r = &tile[ty][x];
        hrow[ty][x] = 7 * (r[0] + r[8]) + 17 * (r[1] + r[7]) + 32 * (r[2] + r[6]) + 46 * (r[3] + r[5]) + 52 * r[4];
    }
    __syncthreads();
    for (int q = threadIdx.x; q < PG_TH * PG_TW; q += 256) {
        const int y = q / PG_TW, x = q - y * PG_TW;
        if (ox + x < W && oy + y < H) {
            const int v = 7 * (hrow[y][x] + hrow[y + 8][x]) + 17 * (hrow[y + 1][x] + hrow[y + 7][x]) + 32 * (hrow[y + 2][x] + hrow[y + 6][x]) +
                          46 * (hrow[y + 3][x] + hrow[y + 5][x]) + 52 * hrow[y + 4][x];
            dst[(size_t)(oy + y) * W + ox + x] = (uint8_t)((v + (1 << 15)) >> 16);
        }
    }
}

__device__ __forceinline__ int fast_score(const uint8_t *p, int stride, int thr) {
    const int v = p[0];
    int d[25];
    d[0] = v - p[3 * stride]; d[4] = v - p[3]; d[8] = v - p[-3 * stride]; d[12] = v - p[-3];
    const int nb = (d[0] < -thr) + (d[4] < -thr) + (d[8] < -thr) + (d[12] < -thr);
    const int nd = (d[0] > thr) + (d[4] > thr) + (d[8] > thr) + (d[12] > thr);
    if (nb < 2 && nd < 2) return 0;   // any 9-arc contains at least two of the four compass pixels
    d[1] = v - p[3 * stride + 1];   d[2] = v - p[2 * stride + 2];   d[3] = v - p[stride + 3];
    d[5] = v - p[-stride + 3];      d[6] = v - p[-2 * stride + 2];  d[7] = v - p[-3 * stride + 1];
    d[9] = v - p[-3 * stride - 1];  d[10] = v - p[-2 * stride - 2]; d[11] = v - p[-stride - 3];
    d[13] = v - p[stride - 3];      d[14] = v - p[2 * stride - 2];  d[15] = v - p[3 * stride - 1];
#pragma unroll
    for (int k = 16; k < 25; k++) d[k] = d[k - 16];
    int best = 0;
#pragma unroll
    for (int k = 0; k < 16; k++) {
        int mn = d[k], mx = d[k];
#pragma unroll
        for (int j = 1; j < 9; j++) { mn = min(mn, d[k + j]); mx = max(mx, d[k + j]); }
        best = max(best, max(mn, -mx));
    }
    return best > thr ? best - 1 : 0;
}
// score of every pixel at least 3 away from the border (0 elsewhere), tile (64 + 6) x (16 + 6) in LDS.  256 threads, tile (blockIdx.x, blockIdx.y).
__device__ __forceinline__ void fast_score_tile(const uint8_t *img, int W, int H, int thr, uint8_t *score) {
    __shared__ uint8_t tile[PG_TH + 6][PG_TW + 8];
    const int ox = blockIdx.x * PG_TW, oy = blockIdx.y * PG_TH;
    for (int q = threadIdx.x; q < (PG_TH + 6) * (PG_TW + 6); q += 256) {
        const int ty = q / (PG_TW + 6), tx = q - ty * (PG_TW + 6);
        const int gy = min(max(oy + ty - 3, 0), H - 1), gx = min(max(ox + tx - 3, 0), W - 1);
        tile[ty][tx] = img[(size_t)gy * W + gx];
    }
    __syncthreads();
    for (int q = threadIdx.x; q < PG_TH * PG_TW; q += 256) {
        const int y = q / PG_TW, x = q - y * PG_TW;
        const int gx = ox + x, gy = oy + y;
        if (gx < W && gy < H) {
            int sc = 0;
            if (gx >= 3 && gx < W - 3 && gy >= 3 && gy < H - 3) sc = fast_score(&tile[y + 3][x + 3], PG_TW + 8, thr);
            score[(size_t)gy * W + gx] = (uint8_t)sc;
        }
    }
}
// one workgroup of 1024 threads over one image: the interior pixels in row-major order, 64 at a time per wavefront, contiguous ranges per
// wavefront; the ballot words go to `words`, the per-wavefront counts are scanned after one barrier and the survivors are written at their
// final positions.  Returns the number of keypoints found (the same value in every thread).
__device__ __forceinline__ int fast_nms_image(const uint8_t *score, int W, int H, unsigned long long *words, float *kp_xy, int cap) {
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6, nw = blockDim.x >> 6;
    const int iw = W - 6, ih = H - 6, npx = iw * ih;
    const int nchunk = (npx + 63) >> 6, cpw = (nchunk + nw - 1) / nw;
    __shared__ int wtot[16];
    int mine = 0;
    for (int ch = wv * cpw; ch < min(nchunk, (wv + 1) * cpw); ch++) {
        const int q = ch * 64 + lane;
        bool mx = false;
        if (q < npx) {
            const int y = q / iw + 3, x = q - (q / iw) * iw + 3;
            const uint8_t *c = score + (size_t)y * W + x;
            const int sc = c[0];
            mx = sc && sc > c[-1] && sc > c[1] && sc > c[-W - 1] && sc > c[-W] && sc > c[-W + 1] && sc > c[W - 1] && sc > c[W] && sc > c[W + 1];
        }
        const unsigned long long bal = __ballot(mx);
        if (lane == 0) words[ch] = bal;
        mine += __popcll(bal);
    }
    if (lane == 0) wtot[wv] = mine;
    __syncthreads();
    int o = 0, total = 0;
    for (int k = 0; k < nw; k++) { if (k < wv) o += wtot[k]; total += wtot[k]; }
    for (int ch = wv * cpw; ch < min(nchunk, (wv + 1) * cpw); ch++) {
        const unsigned long long bal = words[ch];
        if ((bal >> lane) & 1ULL) {
            const int q = ch * 64 + lane, pos = o + __popcll(bal & ((1ULL << lane) - 1ULL));
            if (pos < cap) { kp_xy[2 * pos] = (float)(q - (q / iw) * iw + 3); kp_xy[2 * pos + 1] = (float)(q / iw + 3); }
        }
        o += __popcll(bal);
    }
    return total;
}

// DVision::BRIEF::compute of point p by one wavefront: bit i = I(p + (x1, y1)_i) < I(p + (x2, y2)_i) if both samples are inside the image;
// (int)(pt + offset) truncates
__device__ __forceinline__ void brief_point(const uint8_t *blur, int W, int H, const float *xy, int p, const int *pat, unsigned long long *desc) {
    const int lane = threadIdx.x & 63;
    const float px = xy[2 * p], py = xy[2 * p + 1];
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const int i = 64 * j + lane;
        const int x1 = (int)(px + (float)pat[i]), y1 = (int)(py + (float)pat[256 + i]);
        const int x2 = (int)(px + (float)pat[512 + i]), y2 = (int)(py + (float)pat[768 + i]);
        bool bit = false;
        if (x1 >= 0 && x1 < W && y1 >= 0 && y1 < H && x2 >= 0 && x2 < W && y2 >= 0 && y2 < H) bit = blur[(size_t)y1 * W + x1] < blur[(size_t)y2 * W + x2];
        const unsigned long long bal = __ballot(bit);
        if (lane == 0) desc[4 * (size_t)p + j] = bal;
    }
}

// PinholeCamera::liftProjective (camera_model/src/camera_models/PinholeCamera.cc:449-510): 8 fixed-point iterations of the radial-tangential model
__device__ __forceinline__ void lift_pinhole(const vio_config &c, const float *xy, int i, float *nrm) {
    const double u = xy[2 * i], v = xy[2 * i + 1];
    const double mx_d = (1.0 / c.fx) * u + (-c.cx / c.fx), my_d = (1.0 / c.fy) * v + (-c.cy / c.fy);
    auto dist = [&](double x, double y, double &dx, double &dy) {
        const double mx2 = x * x, my2 = y * y, mxy = x * y, rho2 = mx2 + my2, rad = c.k1 * rho2 + c.k2 * rho2 * rho2;
        dx = x * rad + 2.0 * c.p1 * mxy + c.p2 * (rho2 + 2.0 * mx2);
        dy = y * rad + 2.0 * c.p2 * mxy + c.p1 * (rho2 + 2.0 * my2);
    };
    double dx, dy;
    dist(mx_d, my_d, dx, dy);
    double mx_u = mx_d - dx, my_u = my_d - dy;
    for (int k = 1; k < 8; k++) { dist(mx_u, my_u, dx, dy); mx_u = mx_d - dx; my_u = my_d - dy; }
    nrm[2 * i] = (float)mx_u; nrm[2 * i + 1] = (float)my_u;
}
// the same through a camera model (KeyFrame::computeBRIEFPoint, keyframe.cpp:114-124): (x / z, y / z) of m_camera->liftProjective
__device__ __forceinline__ void lift_camera(const vio_camera &cam, const float *xy, int i, float *nrm) {
    double x, y;
    vcam::lift_plane(cam, xy[2 * i], xy[2 * i + 1], x, y);
    nrm[2 * i] = (float)x; nrm[2 * i + 1] = (float)y;
}

// KeyFrame::searchByBRIEFDes for window descriptor wd[4] by one wavefront: the lanes stride over the m old descriptors; the key
// (distance << 20) | index of the first smallest distance below 128, or (128 << 20) | 0xFFFFF
__device__ __forceinline__ int match_scan(const unsigned long long *wd, const unsigned long long *od, int m) {
    const int lane = threadIdx.x & 63;
    const unsigned long long a0 = wd[0], a1 = wd[1], a2 = wd[2], a3 = wd[3];
    int key = (128 << 20) | 0xFFFFF;   // (distance << 20) | index: the minimum key = smallest distance, then smallest index
    for (int j = lane; j < m; j += 64) {
        const unsigned long long *b = od + 4 * (size_t)j;
        const int dis = __popcll(a0 ^ b[0]) + __popcll(a1 ^ b[1]) + __popcll(a2 ^ b[2]) + __popcll(a3 ^ b[3]);
        if (dis < 128) key = min(key, (dis << 20) | j);
    }
    for (int off = 32; off > 0; off >>= 1) key = min(key, __shfl_xor(key, off, 64));
    return key;
}
__device__ __forceinline__ int match_index(int key) { return ((key >> 20) < 80 && (key & 0xFFFFF) != 0xFFFFF) ? (key & 0xFFFFF) : -1; }

// TemplatedVocabulary::transform(feature, word_id, weight) by one wavefront: the lanes stride over the children of the current node, wave
// arg-min on (distance, child position) = the sequential scan's "first child with the smallest distance".  Returns the leaf's node.
__device__ __forceinline__ int voc_walk(const uint64_t *f, const int *child_begin, const int *children, const uint64_t *ndesc) {
    const int lane = threadIdx.x & 63;
    const uint64_t f0 = f[0], f1 = f[1], f2 = f[2], f3 = f[3];
    int node = 0;
    for (;;) {
        const int b = child_begin[node], e = child_begin[node + 1];
        if (b == e) break;   // leaf = word
        unsigned best = 0xFFFFFFFFu;
        for (int c = b + lane; c < e; c += 64) {
            const uint64_t *d = ndesc + (size_t)children[c] * 4;
            const unsigned dist = (unsigned)(__popcll(f0 ^ d[0]) + __popcll(f1 ^ d[1]) + __popcll(f2 ^ d[2]) + __popcll(f3 ^ d[3]));
            best = min(best, (dist << 22) | (unsigned)(c - b));   // distance <= 256 (9 bits), child position < 2^22
        }
        for (int o = 32; o > 0; o >>= 1) best = min(best, (unsigned)__shfl_xor((int)best, o, 64));
        node = children[b + (int)(best & 0x3FFFFFu)];
    }
    return node;
}

}  // namespace pgdev
