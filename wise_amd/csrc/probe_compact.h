// The first step of the rank-local scans over codes (wise_ivfpq_scan_local, wise_ivfsq_scan_local): drop the probes whose list
// holds no rows in this rank's slice, together with their bias.  One definition for both files; `static`, so each gets its own copy.
#pragma once
#include "topk_common.h"

namespace wise {

// one wave per query: keep, in probe order, the probes whose list holds rows in this slice together with their bias;
// count[q] = the number kept, used[q] = min(G, ceil(count / min_share)) = the probe groups the query uses
static __global__ __launch_bounds__(64) void compact_probes_bias_kernel(const long long* __restrict__ probes, const float* __restrict__ bias,
                                                                        int nprobe, const long long* __restrict__ list_off, int nlist, int G,
                                                                        int min_share, long long* __restrict__ out,
                                                                        float* __restrict__ out_bias, int* __restrict__ count,
                                                                        int* __restrict__ used) {
    const int lane = threadIdx.x;
    const size_t base = (size_t)blockIdx.x * nprobe;
    int n = 0;
    for (int i0 = 0; i0 < nprobe; i0 += 64) {
        const int i = i0 + lane;
        const long long l = (i < nprobe) ? probes[base + i] : -1;
        const bool keep = l >= 0 && l < nlist && list_off[l + 1] > list_off[l];
        const u64 mask = __ballot(keep);
        if (keep) {
            const int o = n + __popcll(mask & ((1ull << lane) - 1ull));
            out[base + o] = l;
            out_bias[base + o] = bias[base + i];
        }
        n += __popcll(mask);
    }
    if (lane == 0) {
        const int want = (n + min_share - 1) / min_share;
        count[blockIdx.x] = n;
        used[blockIdx.x] = want < G ? want : G;
    }
}

}  // namespace wise
