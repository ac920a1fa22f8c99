// The categorical draw on the device, shared by policy_step.hip (a network's sample), draw_actions.hip
// (hftlob_draw_actions) and hftlob.hip (k_env_rollout_eval_drawn): the partitionable threefry's random
// word, jax.random.gumbel's float32 form of it, and the drawn action of a uniform baseline policy.
// hftlob/train/policy.py (random_bits, gumbel_from_bits) and hftlob/evaluate.py
// (draw_actions_reference) hold the same on the CPU.
#ifndef HFTLOB_DRAW_H
#define HFTLOB_DRAW_H

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace hftlob_draw {

__device__ __forceinline__ uint32_t rotl32(uint32_t x, int r) { return (x << r) | (x >> (32 - r)); }

// threefry2x32 with 20 rounds (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3"), as JAX
// runs it: returns y0 ^ y1, the partitionable random_bits word of counter (x0, x1)
__device__ __forceinline__ uint32_t threefry_bits(uint32_t k0, uint32_t k1, uint32_t x0, uint32_t x1) {
    const uint32_t ks[3] = {k0, k1, k0 ^ k1 ^ 0x1BD11BDAu};
    const int rot[2][4] = {{13, 15, 26, 6}, {17, 29, 16, 24}};
    x0 += ks[0];
    x1 += ks[1];
#pragma unroll
    for (int i = 1; i <= 5; ++i) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            x0 += x1;
            x1 = rotl32(x1, rot[(i - 1) & 1][j]) ^ x0;
        }
        x0 += ks[i % 3];
        x1 += ks[(i + 1) % 3] + (uint32_t)i;
    }
    return x0 ^ x1;
}

// jax.random.gumbel's float32 draw from one random word
__device__ __forceinline__ float gumbel_from_bits(uint32_t bits) {
    const float tiny = 1.17549435e-38f;  // float32's smallest normal
    const float f = __uint_as_float((bits >> 9) | 0x3f800000u) - 1.0f;
    const float u = fmaxf(tiny, f * (1.0f - tiny) + tiny);
    return -logf(-logf(u));
}

// The drawn action of actor b of a type with A <= 32 actions under the key (k0, k1): the smallest a
// with bit a of `allowed` set that maximises g[b, a], g = jax.random.gumbel(key, (n_actors, A)) (the
// random word of counter (0, b A + a)): jax.random.categorical on logits 0 on the allowed actions and
// -inf elsewhere.  A mask of one bit draws nothing and gives that action.
// An aligned group of 32 lanes computes it together, lane a of the group (lane & 31) action a's
// noise, and every lane of the group returns the action; both groups of a wave run at once, each on
// its own b.  All 64 lanes must be active, and A and allowed (non-empty, bits < A) the same in all of
// them; b A + a must fit 32 bits.
__device__ __forceinline__ int32_t draw_action(uint32_t k0, uint32_t k1, uint32_t b, int A, uint32_t allowed,
                                               int lane) {
    if ((allowed & (allowed - 1u)) == 0u) return (int32_t)__builtin_ctz(allowed);
    const int a = lane & 31;
    const float g = gumbel_from_bits(threefry_bits(k0, k1, 0u, b * (uint32_t)A + (uint32_t)a));
    float sc = ((allowed >> a) & 1u) ? g : -INFINITY;  // (bits >= A are clear)
    int idx = a;
#pragma unroll
    for (int m = 1; m < 32; m <<= 1) {
        const float os = __shfl_xor(sc, m);
        const int oi = __shfl_xor(idx, m);
        if (os > sc || (os == sc && oi < idx)) {
            sc = os;
            idx = oi;
        }
    }
    return idx;
}

}  // namespace hftlob_draw

#endif
