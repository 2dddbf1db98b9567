// cm_mlp_body.h - the BODY of the row-MLP forward kernels of cm_mlp.hip (no include guard: it is included inside a kernel's braces).
// 32 rows per workgroup through the layer chain, then softmax x avail + sample (or the value output).  The including kernel has the
// by-value argument block `a` (cm::mlp::Args) in scope and says, through macros it defines before and removes after the include,
// which rows are its own and where a layer's operands are:
//   CM_MLP_ROW0         first row of the workgroup, an index into the whole batch
//   CM_MLP_ROWS_LEFT    rows from CM_MLP_ROW0 to the end of the launch's (mlp_kernel) or the member's (mlp_set_kernel) rows
//   CM_MLP_LAYER(l)     statements at the head of layer l's scope (the set kernel reads the member's pointers there, once)
//   CM_MLP_HAS_PK(l)    layer l has B fragments;  CM_MLP_PK(l) they;  CM_MLP_WT(l) the plain weights otherwise;  CM_MLP_B(l) bias or NULL
// Everything indexed by row - x, avail, probs, actions, values, the Philox env id - uses the row's index in the whole batch.
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int c = lane & 15, g = lane >> 4;
    const int row0 = CM_MLP_ROW0;
    const int rows = min(ROWS, CM_MLP_ROWS_LEFT);
    const int sw = a.sw;
    float *buf0 = smem, *buf1 = smem + (size_t)ROWS * sw;

    // ---- layer 0: input streamed from HBM through buf1 in CHUNK-column pieces --------------------------------
    {
        CM_MLP_LAYER(0)
        const int K = a.in_dim, OUT = a.out_dim[0];
        const int nct = (OUT + 15) >> 4;                     // <= 8 (host-checked: OUT <= 128)
        const int KQ0 = (K + 15) >> 4;
        const float *__restrict__ Wt = CM_MLP_WT(0);
        v4f acc[2][2];
#pragma unroll
        for (int t = 0; t < 2; ++t) { acc[t][0] = (v4f){ 0.f, 0.f, 0.f, 0.f }; acc[t][1] = (v4f){ 0.f, 0.f, 0.f, 0.f }; }
        for (int c0 = 0; c0 < K; c0 += CHUNK) {
            __syncthreads();                                 // previous chunk fully consumed
            for (int i = tid; i < ROWS * CHUNK; i += TPB) {
                const int r = i >> 7, cc = i & (CHUNK - 1);
                const int k = c0 + cc;
                buf1[(size_t)r * sw + cc] = (r < rows && k < K) ? a.x[(size_t)(row0 + r) * K + k] : 0.0f;
            }
            __syncthreads();
            const int kc = min(CHUNK, K - c0);
            const int k16 = (kc + 15) >> 4;
            for (int kq = 0; kq < k16; ++kq) {
                const float4 a0 = *reinterpret_cast<const float4 *>(buf1 + (size_t)c * sw + 16 * kq + 4 * g);
                const float4 a1 = *reinterpret_cast<const float4 *>(buf1 + (size_t)(16 + c) * sw + 16 * kq + 4 * g);
                const float x0[4] = { a0.x, a0.y, a0.z, a0.w }, x1[4] = { a1.x, a1.y, a1.z, a1.w };
#pragma unroll
                for (int t = 0; t < 2; ++t) {
                    const int ct = wave + 4 * t;
                    if (ct >= nct) continue;                 // wave-uniform
                    const int col = ct * 16 + c;
                    float bw[4];
                    if (CM_MLP_HAS_PK(0)) {                  // one unconditional 16-byte load per lane
                        const float4 v = reinterpret_cast<const float4 *>(CM_MLP_PK(0))[((size_t)ct * KQ0 + (c0 >> 4) + kq) * 64 + lane];
                        bw[0] = v.x; bw[1] = v.y; bw[2] = v.z; bw[3] = v.w;
                    } else {
#pragma unroll
                        for (int j = 0; j < 4; ++j) {
                            const int k = c0 + 16 * kq + 4 * g + j;
                            bw[j] = (k < K && col < OUT) ? Wt[(size_t)k * OUT + col] : 0.0f;
                        }
                    }
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        acc[t][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(x0[j], bw[j], acc[t][0], 0, 0, 0);
                        acc[t][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(x1[j], bw[j], acc[t][1], 0, 0, 0);
                    }
                }
            }
        }
        const int act = layer_act(a, 0);
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            const int ct = wave + 4 * t;
            if (ct >= nct) continue;
            const int col = ct * 16 + c;
            const float bias = (CM_MLP_B(0) && col < OUT) ? CM_MLP_B(0)[col] : 0.0f;
            store_tile(buf0, sw, 0, ct, lane, acc[t][0], bias, act);
            store_tile(buf0, sw, 1, ct, lane, acc[t][1], bias, act);
        }
    }
    __syncthreads();

    // ---- layers 1..: LDS -> LDS --------------------------------------------------------------------------------
    float *in = buf0, *out = buf1;
    for (int l = 1; l < a.n_layers; ++l) {
        CM_MLP_LAYER(l)
        const int K = a.out_dim[l - 1], OUT = a.out_dim[l];
        const int nct = (OUT + 15) >> 4, k16 = (K + 15) >> 4;
        const float *__restrict__ Wt = CM_MLP_WT(l);
        const int act = layer_act(a, l);
        for (int ct = wave; ct < nct; ct += 4) {
            const int col = ct * 16 + c;
            v4f acc0 = (v4f){ 0.f, 0.f, 0.f, 0.f }, acc1 = (v4f){ 0.f, 0.f, 0.f, 0.f };
            for (int kq = 0; kq < k16; ++kq) {
                const float4 a0 = *reinterpret_cast<const float4 *>(in + (size_t)c * sw + 16 * kq + 4 * g);
                const float4 a1 = *reinterpret_cast<const float4 *>(in + (size_t)(16 + c) * sw + 16 * kq + 4 * g);
                const float x0[4] = { a0.x, a0.y, a0.z, a0.w }, x1[4] = { a1.x, a1.y, a1.z, a1.w };
                float bw[4];
                if (CM_MLP_HAS_PK(l)) {
                    const float4 v = reinterpret_cast<const float4 *>(CM_MLP_PK(l))[((size_t)ct * k16 + kq) * 64 + lane];
                    bw[0] = v.x; bw[1] = v.y; bw[2] = v.z; bw[3] = v.w;
                } else {
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const int k = 16 * kq + 4 * g + j;
                        bw[j] = (k < K && col < OUT) ? Wt[(size_t)k * OUT + col] : 0.0f;
                    }
                }
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(x0[j], bw[j], acc0, 0, 0, 0);
                    acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(x1[j], bw[j], acc1, 0, 0, 0);
                }
            }
            const float bias = (CM_MLP_B(l) && col < OUT) ? CM_MLP_B(l)[col] : 0.0f;
            store_tile(out, sw, 0, ct, lane, acc0, bias, act);
            store_tile(out, sw, 1, ct, lane, acc1, bias, act);
        }
        __syncthreads();
        float *t = in; in = out; out = t;
    }
    // `in` now holds the last layer's output [ROWS][>= out_dim[n_layers-1]]

    if (a.values) {                                          // GaussianMLPBaseline mean: one value per row
        for (int r = tid; r < rows; r += TPB) a.values[row0 + r] = in[(size_t)r * sw];
        return;
    }

    // ---- per-agent softmax * avail, renormalise, sample (same arithmetic order as cm_policy_mfma.hip) ------------
    const int G = a.groups, A = a.n_act;
    for (int it = tid; it < rows * G; it += TPB) {
        const int r = it / G, gi = it - r * G;
        const float *lg = in + (size_t)r * sw + gi * A;
        float p[MAX_ACT];
        float mx = -INFINITY, sum = 0.0f, msum = 0.0f;
#pragma unroll
        for (int k = 0; k < MAX_ACT; ++k) if (k < A) mx = fmaxf(mx, lg[k]);
#pragma unroll
        for (int k = 0; k < MAX_ACT; ++k) if (k < A) { p[k] = expf(lg[k] - mx); sum += p[k]; }
        const size_t flat = (size_t)(row0 + r) * G + gi;     // global agent-row index
#pragma unroll
        for (int k = 0; k < MAX_ACT; ++k) if (k < A) {
            const float av = a.avail ? a.avail[flat * A + k] : 1.0f;
            p[k] = (p[k] / sum) * av; msum += p[k];
        }
#pragma unroll
        for (int k = 0; k < MAX_ACT; ++k) if (k < A) p[k] = p[k] / msum;
        if (a.probs) {
#pragma unroll
            for (int k = 0; k < MAX_ACT; ++k) if (k < A) a.probs[flat * A + k] = p[k];
        }
        if (a.actions) {
            int act = 0;
            if (a.greedy) {
                float best = p[0];
#pragma unroll
                for (int k = 1; k < MAX_ACT; ++k) if (k < A && p[k] > best) { best = p[k]; act = k; }
            } else {
                const size_t e = flat / (size_t)a.agents_per_env;
                const uint32_t i = (uint32_t)(flat - e * a.agents_per_env);
                const u32x4 xr = philox4x32_10((uint32_t)(a.env_id_offset + (int)e),
                                               a.policy_step + (a.step_base ? *a.step_base : 0u), SITE_ACTION, i,
                                               a.key0, a.key1);
                const float u = unit_f32(xr.x);
                float acc = 0.0f;
                int sel = -1, last = 0;
#pragma unroll
                for (int k = 0; k < MAX_ACT; ++k) if (k < A) { if (p[k] > 0.0f) last = k; acc += p[k]; if (sel < 0 && u < acc) sel = k; }
                act = sel < 0 ? last : sel;
            }
            a.actions[flat] = act;
        }
    }
