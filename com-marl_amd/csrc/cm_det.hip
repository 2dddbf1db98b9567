// cm_det.hip - the second pass of the deterministic merges (include/commarl.h "Deterministic update mode").
//
// In slab mode a kernel that would add its per-workgroup partial sums into an output with float atomics plain-stores them
// into row blockIdx.x of a slab instead.  slab_reduce sums the rows in index order: every output element is the same
// sequence of f32 additions on every run, whatever order the workgroups finished in.
#include <algorithm>

#include "cm_internal.h"

namespace cm {

namespace {

constexpr int RED_TPB = 256;

// one thread per element of a slab row; the rows are read in order b = 0, 1, ... (coalesced across the threads)
__global__ __launch_bounds__(RED_TPB) void slab_reduce_kernel(const float *__restrict__ slab, int rows, int row_len, SlabSegs segs) {
    const int i = blockIdx.x * RED_TPB + threadIdx.x;
    if (i >= row_len) return;
    float *out = nullptr;
    int j = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k)
        if (k < segs.n_seg && i >= segs.s[k].off && i < segs.s[k].off + segs.s[k].n) { out = segs.s[k].out; j = i - segs.s[k].off; }
    if (!out) return;
    const float *p = slab + i;
    float s = 0.0f;
    int b = 0;
    for (; b + 4 <= rows; b += 4) {                       // four loads in flight, the additions still in row order
        const float v0 = p[(size_t)b * row_len], v1 = p[(size_t)(b + 1) * row_len];
        const float v2 = p[(size_t)(b + 2) * row_len], v3 = p[(size_t)(b + 3) * row_len];
        s += v0; s += v1; s += v2; s += v3;
    }
    for (; b < rows; ++b) s += p[(size_t)b * row_len];
    out[j] += s;
}

}  // namespace

int slab_reduce(const float *slab, int rows, int row_len, const SlabSegs &segs, hipStream_t st) {
    if (rows <= 0 || row_len <= 0) return CM_OK;
    hipLaunchKernelGGL(slab_reduce_kernel, dim3((unsigned)((row_len + RED_TPB - 1) / RED_TPB)), dim3(RED_TPB), 0, st, slab, rows, row_len, segs);
    CM_HIP(hipGetLastError());
    return CM_OK;
}

int slab_check(const void *ws, size_t ws_bytes, size_t need, const char *what) {
    if (!ws) return set_error(CM_ERR_ARG, std::string(what) + ": null slab workspace");
    if (ws_bytes < need)
        return set_error(CM_ERR_ARG, std::string(what) + ": slab workspace of " + std::to_string(ws_bytes) + " bytes, " + std::to_string(need) +
                                         " required");
    return CM_OK;
}

}  // namespace cm
