// Pack / unpack kernels of the sequence snapshots (vio_save_seqs / vio_load_seqs): one launch gathers the state slices of the saved slots
// into one contiguous staging buffer (or scatters them back), so that a save is one launch and one copy instead of one small copy per state
// array and sequence.  The grid is 2-D: x runs over the 16-byte chunks of all layout-table entries, y over the sequences of the call.  Every
// blob offset is a multiple of 16, so a lane moves one dwordx4 wherever the array side is 16-byte aligned too; a chunk whose array address is
// not (byte arrays with a stride that is only a multiple of 8) or that holds an entry's tail goes byte by byte.  No LDS, no atomics.
#include "snapshot.h"

namespace {
// the entry whose chunk range holds c: chunk0 ascends, at most a few dozen entries
__device__ __forceinline__ int snap_entry_of(const SnapEntry *tab, int n, int64_t c) {
    int lo = 0, hi = n - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (tab[mid].chunk0 <= c) lo = mid; else hi = mid - 1;
    }
    return lo;
}
}  // namespace

__global__ void __launch_bounds__(SNAP_THREADS) snap_pack_kernel(const SnapEntry *tab, int n_entries, int64_t total_chunks, const SnapSeq *seqs, unsigned char *stage) {
    const int64_t c = (int64_t)blockIdx.x * SNAP_THREADS + threadIdx.x;
    if (c >= total_chunks) return;
    const SnapSeq q = seqs[blockIdx.y];
    const SnapEntry e = tab[snap_entry_of(tab, n_entries, c)];
    const int64_t o = (c - e.chunk0) * 16;
    const int64_t left = e.bytes - o;   // > 0: the entry's chunk range covers ceil(bytes / 16)
    const unsigned char *src = e.base + (int64_t)q.slot * e.stride + o;
    unsigned char *dst = stage + q.stage_off + e.blob_off + o;
    if (left >= 16 && ((uintptr_t)src & 15) == 0) {
        *(uint4 *)dst = *(const uint4 *)src;
    } else {
        // tail of an entry (the rest of its last chunk is padding: zero) or an array slice that is not 16-byte aligned
        // (fully unrolled, so the four words stay in registers: a byte array indexed by a loop variable would be promoted to LDS)
        const int nb = left < 16 ? (int)left : 16;
        uint32_t w[4] = {0u, 0u, 0u, 0u};
#pragma unroll
        for (int k = 0; k < 16; k++)
            if (k < nb) w[k >> 2] |= (uint32_t)src[k] << (8 * (k & 3));
        *(uint4 *)dst = make_uint4(w[0], w[1], w[2], w[3]);
    }
}

__global__ void __launch_bounds__(SNAP_THREADS) snap_unpack_kernel(const SnapEntry *tab, int n_entries, int64_t total_chunks, const SnapSeq *seqs, const unsigned char *stage) {
    const int64_t c = (int64_t)blockIdx.x * SNAP_THREADS + threadIdx.x;
    if (c >= total_chunks) return;
    const SnapSeq q = seqs[blockIdx.y];
    const SnapEntry e = tab[snap_entry_of(tab, n_entries, c)];
    const int64_t o = (c - e.chunk0) * 16;
    const int64_t left = e.bytes - o;
    const unsigned char *src = stage + q.stage_off + e.blob_off + o;
    unsigned char *dst = e.base + (int64_t)q.slot * e.stride + o;
    if (left >= 16 && ((uintptr_t)dst & 15) == 0) {
        *(uint4 *)dst = *(const uint4 *)src;
    } else {
        const uint4 v = *(const uint4 *)src;
        const uint32_t w[4] = {v.x, v.y, v.z, v.w};
        const int nb = left < 16 ? (int)left : 16;   // never beyond the slice: the next sequence's data follows it
#pragma unroll
        for (int k = 0; k < 16; k++)
            if (k < nb) dst[k] = (unsigned char)(w[k >> 2] >> (8 * (k & 3)));
    }
}
