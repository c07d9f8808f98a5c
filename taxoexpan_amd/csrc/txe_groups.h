// The group structure of a labelled batch, shared by the grouped ranking (txe_grouprank.hip) and the margin-rank loss
// (txe_pairloss.hip).
//
// Groups start at index 0 and at every i with label[i-1] == 0 and label[i] == 1 (the reference splits at every [0, 1] pair of the
// label bytes).  Positives are the entries with label 1; every other entry of the group is a negative.
//
//   flags: v[i] = (group start) << 32 | (positive) -- a single 64-bit exclusive scan (hipcub) gives both the group index (high half) and
//          the positive index (low half) of every entry; B < 2^31 keeps the low half from carrying.
//   index: see group_index_kernel.
//   entry i then belongs to group (e[i] >> 32) + (v[i] >> 32) - 1, and a positive i is positive number e[i] & 0xffffffff.
#pragma once
#include "txe_common.h"
#include <hipcub/hipcub.hpp>

namespace txe {

typedef unsigned long long u64;

template <typename L>
__global__ __launch_bounds__(256) void group_flags_kernel(const L* __restrict__ lab, int B, u64* __restrict__ v) {
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < B; i += (long long)gridDim.x * 256) {
        const L x = lab[i];
        const u64 f = (i == 0 || (lab[i - 1] == 0 && x == 1)) ? 1ull : 0ull;
        v[i] = (f << 32) | (x == 1 ? 1ull : 0ull);
    }
}

// index: pos_off[g] = positives before group g (n_groups + 1 entries), pos_elem[p] = the entry of positive p, per_pos[p] = INIT (the
// ranking starts its ranks at 1, the margin-rank loss its pair counts at 0), counts (may be NULL) = {n_groups, n_pos}.
template <int INIT>
__global__ __launch_bounds__(256) void group_index_kernel(const u64* __restrict__ v, const u64* __restrict__ e, int B, int* __restrict__ pos_off,
                                                          int* __restrict__ pos_elem, int* __restrict__ per_pos, int* __restrict__ counts) {
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < B; i += (long long)gridDim.x * 256) {
        const u64 vi = v[i], ei = e[i];
        const int f = (int)(vi >> 32), p = (int)(vi & 0xffffffffull);
        const int g = (int)(ei >> 32) + f - 1;
        const int pi = (int)(ei & 0xffffffffull);
        if (f) pos_off[g] = pi;
        if (p) {
            pos_elem[pi] = (int)i;
            per_pos[pi] = INIT;
        }
        if (i == B - 1) {
            pos_off[g + 1] = pi + p;
            if (counts) {
                counts[0] = g + 1;
                counts[1] = pi + p;
            }
        }
    }
}

static size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

static size_t group_scan_temp_bytes(int B) {
    size_t bytes = 0;
    (void)hipcub::DeviceScan::ExclusiveSum(nullptr, bytes, (const u64*)nullptr, (u64*)nullptr, B);
    return bytes;
}

// workgroups of 256 threads for a grid-stride pass over B entries
static int group_blocks(int B) { return (int)((B + 255LL) / 256 < 65536 ? (B + 255LL) / 256 : 65536); }

// e = exclusive scan of v (B entries); temp: group_scan_temp_bytes(B) bytes at least
static bool group_scan(const u64* v, u64* e, int B, void* temp, size_t temp_bytes, hipStream_t s) {
    return hipcub::DeviceScan::ExclusiveSum(temp, temp_bytes, v, e, B, s) == hipSuccess;
}

}  // namespace txe
