// cm_policy_g_tail.h - the policy's sampler tail of the run-time-sized forward: per-agent softmax x avail, renormalise, sample,
// over the head's outputs in LDS plane `nxt` (stride SW).  A statement block, #included inside a kernel of cm_policy_g_dev.h's
// family behind head(), NOT a function: fwd_any_kernel's instruction stream is pinned against the parent build (tests.isa diff),
// and a function - which the compiler simplifies on its own before it inlines it - changes that stream.  Names it expects in
// scope: Args a; float *lds; int tid, N, SW, nxt, s0 (the workgroup's first env in `a`'s batch), rows (its agent rows).
{
    const int A = a.A;

    // ---- per-agent softmax * avail, renormalise, sample (same arithmetic order as cm_mlp_body.h) ----
    for (int r = tid; r < rows; r += TPB) {
        const int lg = nxt + r * SW;
        float p[MAX_ACT];
        float mx = -INFINITY, sum = 0.0f, msum = 0.0f;
#pragma unroll
        for (int k = 0; k < MAX_ACT; ++k) if (k < A) mx = fmaxf(mx, lds[lg + k]);
#pragma unroll
        for (int k = 0; k < MAX_ACT; ++k) if (k < A) { p[k] = expf(lds[lg + k] - mx); sum += p[k]; }
        const size_t flat = (size_t)s0 * N + r;             // global agent-row index
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
                const int e = r / N, i = r - e * N;
                const u32x4 xr = philox4x32_10((uint32_t)(a.env_id_offset + s0 + e),
                                               a.policy_step + (a.step_base ? *a.step_base : 0u), SITE_ACTION, (uint32_t)i,
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
}
