// Sequence snapshots (include/vio_abi.h "sequence snapshots"): what the host translation units and the pack / unpack kernels share.
#pragma once
#include <stdint.h>
#include "../../include/vio_abi.h"

// One state entry of the layout table as the kernels see it: the slice of sequence s is `bytes` long and starts at base + s * stride; inside
// the device part of a blob it starts at blob_off (a multiple of 16) and covers chunks [chunk0, chunk0 + ceil(bytes / 16)) of the flattened
// chunk index the grid's x dimension runs over.
struct SnapEntry {
    unsigned char *base;
    int64_t stride, bytes, blob_off;
    int64_t chunk0;
};
// One sequence of a save / load call: the slot, and where its device part starts in the staging buffer (a multiple of 16)
struct SnapSeq {
    int64_t stage_off;
    int32_t slot, pad;
};
#define SNAP_THREADS 256

// host only (snapshot_host.cpp): name of the first field of the two keys that differs, nullptr when they are equal
const char *snap_shape_diff(const vio_snapshot_shape &a, const vio_snapshot_shape &b);

#ifdef __HIPCC__
#include <hip/hip_runtime.h>
// grid = (ceil(total chunks / SNAP_THREADS), sequences of the launch): gather (pack) the slot slices into the staging buffer / scatter them back
__global__ void snap_pack_kernel(const SnapEntry *tab, int n_entries, int64_t total_chunks, const SnapSeq *seqs, unsigned char *stage);
__global__ void snap_unpack_kernel(const SnapEntry *tab, int n_entries, int64_t total_chunks, const SnapSeq *seqs, const unsigned char *stage);
#endif
