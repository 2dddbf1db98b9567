// cm_ppo_cat_dev.h - the Categorical arithmetic of one env step for the update statistics (cm_ppo_stats.hip): pass 1 of
// ppo_surrogate_kernel (cm_ppo.hip) as a device function, the same operations in the same order, so that the ratio the statistics
// judge is the ratio the loss used.  ppo_surrogate_kernel keeps its own text: routed through this function both of its
// instantiations came out with another instruction stream (same arithmetic, other schedule and registers), and the loss kernel
// is held to the code it had.  A change to either copy is a change to both.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace cm {

constexpr int PPO_MAX_A = 8;
constexpr float PPO_PROB_EPS = 1.1920928955078125e-07f;   // torch.finfo(float32).eps: probs_to_logits clamps to [eps, 1 - eps]

// Log-likelihood of the taken joint action (sum over the N agents) and H = mean_i H_i of one env step, from its logits z0 [N,A]
// and actions a0 [N] (comm_categorical_mlp_policy.py:121-137: probs = softmax renormalised twice, logits =
// log(clamp(probs, eps, 1 - eps))).  A <= PPO_MAX_A logits per agent in registers.
__device__ __forceinline__ void categorical_ll_entropy(const float *__restrict__ z0, const int32_t *__restrict__ a0, int N, int A,
                                                       float &new_ll_out, float &ent_out) {
    const float EPS = PPO_PROB_EPS;
    float new_ll = 0.0f, ent = 0.0f;
    for (int i = 0; i < N; ++i) {
        float z[PPO_MAX_A], p[PPO_MAX_A];
        float mx = -INFINITY;
#pragma unroll
        for (int b = 0; b < PPO_MAX_A; ++b) if (b < A) { z[b] = z0[i * A + b]; mx = fmaxf(mx, z[b]); }
        float s0 = 0.0f;
#pragma unroll
        for (int b = 0; b < PPO_MAX_A; ++b) if (b < A) { p[b] = expf(z[b] - mx); s0 += p[b]; }
        float s1 = 0.0f, s2 = 0.0f;
#pragma unroll
        for (int b = 0; b < PPO_MAX_A; ++b) if (b < A) { p[b] = p[b] / s0; s1 += p[b]; }
#pragma unroll
        for (int b = 0; b < PPO_MAX_A; ++b) if (b < A) { p[b] = p[b] / s1; s2 += p[b]; }
        const int ai = a0[i];
        float h = 0.0f;
#pragma unroll
        for (int b = 0; b < PPO_MAX_A; ++b) if (b < A) {
            const float p3 = p[b] / s2;
            const float lg = logf(fminf(fmaxf(p3, EPS), 1.0f - EPS));
            h -= lg * p3;
            if (b == ai) new_ll += lg;
        }
        ent += h;
    }
    ent /= (float)N;
    new_ll_out = new_ll;
    ent_out = ent;
}

}  // namespace cm
