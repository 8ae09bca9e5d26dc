// What the rank-local scans over codes (wise_ivfpq_scan_local, wise_ivfsq_scan_local) share: the layout of their workspace and
// their first step — drop the probes whose list holds no rows in this rank's slice, together with their bias.  One definition
// for both files; `static`, so each gets its own copy.
#pragma once
#include "topk_common.h"

namespace wise {

// Workspace of a rank-local scan: the keys (part_bytes of them: [nprobe][nq][k] or [groups][nq][k], a multiple of 256), then the
// kept probes [nq][nprobe], their bias, the groups used per query and (for a call without probe_count) the kept counts
static size_t local_probe_bytes(int nq, int nprobe) { return align_up((size_t)nq * nprobe * sizeof(long long), 256); }
static size_t local_bias_bytes(int nq, int nprobe) { return align_up((size_t)nq * nprobe * sizeof(float), 256); }
static size_t local_count_bytes(int nq) { return align_up((size_t)nq * sizeof(int), 256); }

struct LocalWorkspace {
    u64* part;
    long long* live;
    float* lbias;
    int* used;
    int* count;
    static size_t bytes(size_t part_bytes, int nq, int nprobe) {
        return part_bytes + local_probe_bytes(nq, nprobe) + local_bias_bytes(nq, nprobe) + 2 * local_count_bytes(nq);
    }
    // pointers into `workspace` (bytes(...) of it); probe_count, when given, receives the kept counts instead
    static LocalWorkspace carve(void* workspace, size_t part_bytes, int nq, int nprobe, int32_t* probe_count) {
        unsigned char* wsb = reinterpret_cast<unsigned char*>(workspace);
        LocalWorkspace w;
        w.part = reinterpret_cast<u64*>(wsb);
        wsb += part_bytes;
        w.live = reinterpret_cast<long long*>(wsb);
        wsb += local_probe_bytes(nq, nprobe);
        w.lbias = reinterpret_cast<float*>(wsb);
        wsb += local_bias_bytes(nq, nprobe);
        w.used = reinterpret_cast<int*>(wsb);
        wsb += local_count_bytes(nq);
        w.count = probe_count ? probe_count : reinterpret_cast<int*>(wsb);
        return w;
    }
};

// one wave per query: keep, in probe order, the probes whose list holds rows in this slice together with their bias;
// count[q] = the number kept, used[q] = min(G, ceil(count / min_share)) = the probe groups the query uses.  BIAS = false: a scan
// without a bias term (wise_ivfl2_scan_local): neither bias array is touched
template <bool BIAS>
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
            if constexpr (BIAS) out_bias[base + o] = bias[base + i];
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
