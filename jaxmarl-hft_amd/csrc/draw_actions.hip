// The drawn actions of a uniform baseline policy for a batch of actors as one launch (include/hftlob.h:
// hftlob_draw_actions), gfx950.
//
// The reference's multi-action FixedAction and its RandomPolicy (baseline_eval/baseline_only_JAXMARL.py
// :58-71, baseline_JAXMARL.py:367-394) sample a categorical that is uniform over a set of actions at
// every step.  hftlob_env_rollout_eval_drawn draws inside the env launch; a caller who steps the env
// himself (hftlob/evaluate.py evaluate_policy, next to a network's policy step) draws a type's actions
// here.  hftlob_draw.h draw_action is the draw, the same code in both, and hftlob/evaluate.py
// draw_actions_reference its definition.
//
// An aligned group of 32 lanes per actor, lane a of it action a's noise: one threefry block and two
// logs per (actor, action), a 5-step argmax over the group, one store per actor.  A group past the
// last actor repeats the last one (its lanes stay active for the exchange) and stores nothing.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/hftlob.h"
#include "hftlob_draw.h"
#include "hftlob_internal.h"

#pragma clang fp contract(off)

namespace {

constexpr int NT = 256;  // lanes per workgroup: 8 actors

__global__ __launch_bounds__(NT) void k_draw_actions(int n_actors, int n_actions, uint32_t allowed,
                                                     const uint32_t* __restrict__ key,
                                                     int32_t* __restrict__ actions) {
    const int lane = threadIdx.x & 63;
    const long long b = ((long long)blockIdx.x * NT + threadIdx.x) >> 5;
    const uint32_t bc = (uint32_t)(b < n_actors ? b : n_actors - 1);
    const int32_t act = hftlob_draw::draw_action(key[0], key[1], bc, n_actions, allowed, lane);
    if (b < n_actors && (lane & 31) == 0) actions[b] = act;
}

}  // namespace

extern "C" int hftlob_draw_actions(int n_actors, int n_actions, uint32_t allowed, const uint32_t* key, int32_t* actions,
                                   void* stream) {
    if (!key || !actions) return hftlob_fail(HFTLOB_EINVAL, "draw_actions: a null pointer");
    if (n_actors < 1) return hftlob_fail(HFTLOB_EINVAL, "draw_actions: n_actors must be >= 1");
    if (n_actions < 1 || n_actions > 32) return hftlob_fail(HFTLOB_EINVAL, "draw_actions: n_actions must be 1..32");
    if (allowed == 0u) return hftlob_fail(HFTLOB_EINVAL, "draw_actions: the allowed mask is empty");
    if (n_actions < 32 && (allowed >> n_actions) != 0u)
        return hftlob_fail(HFTLOB_EINVAL, "draw_actions: the allowed mask has bits >= n_actions");
    if ((long long)n_actors * n_actions > 0x100000000LL)
        return hftlob_fail(HFTLOB_EINVAL, "draw_actions: n_actors * n_actions is past the 32-bit counter");
    const long long blocks = ((long long)n_actors * 32 + NT - 1) / NT;
    k_draw_actions<<<dim3((unsigned)blocks), NT, 0, (hipStream_t)stream>>>(n_actors, n_actions, allowed, key, actions);
    const hipError_t err = hipGetLastError();
    return err == hipSuccess ? HFTLOB_OK : hftlob_fail(HFTLOB_ELAUNCH, hipGetErrorString(err));
}
