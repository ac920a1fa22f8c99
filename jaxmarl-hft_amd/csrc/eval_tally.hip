// The evaluation accumulators from per-step outputs as one launch (include/hftlob.h:
// hftlob_eval_tally), gfx950.
//
// hftlob_env_rollout_eval tallies inside the env launch; a caller whose actions come from somewhere
// else (a policy network) holds each step's rewards, info record and global dones instead and folds
// them into the same stats words here.  hftlob/evaluate.py reduce_steps is the definition, and the
// result is held to it bit for bit.
//
// One lane per (env, agent, quantity q = 0..24): q = 0 is the reward, q = 1 + k info word k.  Lane q
// keeps the words 8+2q, 9+2q (the quantity over all steps) and, for q >= 1, 56+2q, 57+2q (info word
// k = q - 1 at the episodes' last steps) in registers across the n_steps loop; the q = 0 lane also
// keeps words 0..7 (steps, episodes, the running sum and length, the episode sums).  Every stats word
// is read once and written once per launch, consecutive lanes read consecutive info words, and there
// is no LDS and no atomic.
//
// hftlob_eval_tally_episodes also writes the per-episode records (hftlob.h): at a step with done the lane
// of quantity q stores its word of record i, where i is the lane's own count of the agent's episodes,
// started from stats word 1.
//
// No floating-point contraction: every word is a plain double add of a separately rounded product
// (run_sum * run_sum and the square of an int32 above 2^26 are inexact in double, so a fused
// multiply-add changes the bits).  The whole library is compiled with -ffp-contract=off (Makefile,
// HIPFLAGS); the pragma below states it for this file whatever the command line says.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/hftlob.h"
#include "hftlob_internal.h"

#pragma clang fp contract(off)

namespace {

constexpr int NQ = 1 + HFTLOB_INFO_AGENT_WORDS;  // quantities per agent
constexpr int W_STEP_Q = 8;                      // + 2q, + 2q + 1
constexpr int W_END_INFO = W_STEP_Q + 2 * NQ;    // + 2k, + 2k + 1
static_assert(W_END_INFO + 2 * HFTLOB_INFO_AGENT_WORDS == HFTLOB_EVAL_WORDS, "the stats row of hftlob.h");
static_assert(HFTLOB_INFO_AGENT_WORDS <= 32, "an agent's float words are one 32-bit mask");

constexpr int NT = 256;  // lanes per workgroup
constexpr int AGENTS_PER_WAVE = 64 / NQ;  // (the launch with per-episode records)
static_assert(NT % 64 == 0 && AGENTS_PER_WAVE >= 1, "whole waves, an agent's lanes within one");

// the agents' float-word masks, by value: bit k of m[a] set = info word k of agent a is a float
struct FloatWords {
    uint32_t m[HFTLOB_MAX_AGENTS];
};

__global__ __launch_bounds__(NT) void k_eval_tally(int n_env, int n_agents, int n_steps, int info_words,
                                                   const float* __restrict__ rewards,
                                                   const int32_t* __restrict__ info,
                                                   const uint8_t* __restrict__ done_all, FloatWords fw,
                                                   double* __restrict__ stats, double* __restrict__ episodes,
                                                   int ep_cap) {
    const long long g = (long long)blockIdx.x * NT + threadIdx.x;
    long long ea = g / NQ;  // env * n_agents + agent
    int q = (int)(g - ea * NQ);
    if (episodes) {
        // with records every lane of an agent reads word 1, which the agent's q = 0 lane writes at the
        // end: the agent's NQ lanes stay inside one wave (AGENTS_PER_WAVE agents per wave, the other lanes
        // idle), whose lanes all load before any of them stores
        const int l = threadIdx.x & 63, slot = l / NQ;
        if (slot >= AGENTS_PER_WAVE) return;
        ea = (g >> 6) * AGENTS_PER_WAVE + slot;
        q = l - slot * NQ;
    }
    if (ea >= (long long)n_env * n_agents) return;
    const long long e = ea / n_agents;
    const int a = (int)(ea - e * n_agents);
    const bool isf = q > 0 && ((fw.m[a] >> (q - 1)) & 1u);

    double* const row = stats + ea * HFTLOB_EVAL_WORDS;
    double s = row[W_STEP_Q + 2 * q], s2 = row[W_STEP_Q + 2 * q + 1];
    double es = 0.0, es2 = 0.0;
    if (q > 0) {
        es = row[W_END_INFO + 2 * (q - 1)];
        es2 = row[W_END_INFO + 2 * (q - 1) + 1];
    }
    double steps = 0.0, n_done = 0.0, run_sum = 0.0, run_len = 0.0, ep_sum = 0.0, ep_sum2 = 0.0, ep_len = 0.0,
           ep_len2 = 0.0;
    if (q == 0) {
        steps = row[0], n_done = row[1], run_sum = row[2], run_len = row[3];
        ep_sum = row[4], ep_sum2 = row[5], ep_len = row[6], ep_len2 = row[7];
    }

    // the lane's word of a step: a float of rewards, or a word of the info record
    const int32_t* src = q == 0 ? reinterpret_cast<const int32_t*>(rewards) + ea
                                : info + e * info_words + HFTLOB_INFO_WORLD_WORDS + a * HFTLOB_INFO_AGENT_WORDS + (q - 1);
    const long long stride = q == 0 ? (long long)n_env * n_agents : (long long)n_env * info_words;
    const bool widen_float = q == 0 || isf;
    const uint8_t* dp = done_all + e;
    // the per-episode records (hftlob.h, hftlob_env_rollout_eval_episodes): every lane of the agent keeps
    // the episode index as its own running count from word 1, and stores its word of the record
    double* const erow = episodes ? episodes + ea * ep_cap * HFTLOB_EPISODE_WORDS : nullptr;
    double ei = erow ? row[1] : 0.0;

    for (int t = 0; t < n_steps; ++t, src += stride, dp += n_env) {
        const int32_t w = *src;
        const bool d = *dp != 0;
        const double x = widen_float ? (double)__int_as_float(w) : (double)w;
        const double x2 = x * x;
        s += x;
        s2 += x2;
        double* const rec = (erow && d && ei >= 0.0 && ei < (double)ep_cap) ? erow + (long long)(int)ei * HFTLOB_EPISODE_WORDS
                                                                           : nullptr;
        if (erow && d) ei += 1.0;
        if (q > 0) {
            if (d) {
                es += x;
                es2 += x2;
                if (rec) rec[1 + q] = x;
            }
        } else {
            steps += 1.0;
            n_done += d ? 1.0 : 0.0;
            run_sum += x;
            run_len += 1.0;
            if (d) {
                if (rec) rec[0] = run_sum, rec[1] = run_len;
                ep_sum += run_sum;
                ep_sum2 += run_sum * run_sum;
                ep_len += run_len;
                ep_len2 += run_len * run_len;
                run_sum = 0.0;
                run_len = 0.0;
            }
        }
    }

    row[W_STEP_Q + 2 * q] = s;
    row[W_STEP_Q + 2 * q + 1] = s2;
    if (q > 0) {
        row[W_END_INFO + 2 * (q - 1)] = es;
        row[W_END_INFO + 2 * (q - 1) + 1] = es2;
    } else {
        row[0] = steps, row[1] = n_done, row[2] = run_sum, row[3] = run_len;
        row[4] = ep_sum, row[5] = ep_sum2, row[6] = ep_len, row[7] = ep_len2;
    }
}

}  // namespace

// hftlob_eval_tally and hftlob_eval_tally_episodes: one launch, the second with the records' buffer
static int eval_tally(int n_env, int n_agents, int n_steps, int info_words, const float* rewards, const int32_t* info,
                      const uint8_t* done_all, const uint32_t* float_words, double* stats, double* episodes, int ep_cap,
                      void* stream) {
    if (n_env < 1 || n_agents < 1 || n_steps < 1)
        return hftlob_fail(HFTLOB_EINVAL, "eval_tally: n_env, n_agents and n_steps must be >= 1");
    if (n_agents > HFTLOB_MAX_AGENTS) return hftlob_fail(HFTLOB_EINVAL, "eval_tally: more than HFTLOB_MAX_AGENTS agents");
    if (info_words < HFTLOB_INFO_WORLD_WORDS + n_agents * HFTLOB_INFO_AGENT_WORDS)
        return hftlob_fail(HFTLOB_EINVAL, "eval_tally: info_words is smaller than the agents' info blocks need");
    if (!rewards || !info || !done_all || !float_words || !stats)
        return hftlob_fail(HFTLOB_EINVAL, "eval_tally: a null pointer");
    const long long lanes = episodes ? ((long long)n_env * n_agents + AGENTS_PER_WAVE - 1) / AGENTS_PER_WAVE * 64
                                     : (long long)n_env * n_agents * NQ;
    const long long blocks = (lanes + NT - 1) / NT;
    if (blocks > 0x7fffffffLL) return hftlob_fail(HFTLOB_EINVAL, "eval_tally: n_env * n_agents is too large for one launch");
    FloatWords fw;
    for (int a = 0; a < HFTLOB_MAX_AGENTS; ++a) fw.m[a] = a < n_agents ? float_words[a] : 0u;
    k_eval_tally<<<dim3((unsigned)blocks), NT, 0, (hipStream_t)stream>>>(n_env, n_agents, n_steps, info_words, rewards,
                                                                         info, done_all, fw, stats, episodes, ep_cap);
    const hipError_t err = hipGetLastError();
    return err == hipSuccess ? HFTLOB_OK : hftlob_fail(HFTLOB_ELAUNCH, hipGetErrorString(err));
}

extern "C" int hftlob_eval_tally(int n_env, int n_agents, int n_steps, int info_words, const float* rewards,
                                 const int32_t* info, const uint8_t* done_all, const uint32_t* float_words,
                                 double* stats, void* stream) {
    return eval_tally(n_env, n_agents, n_steps, info_words, rewards, info, done_all, float_words, stats, nullptr, 0,
                      stream);
}

extern "C" int hftlob_eval_tally_episodes(int n_env, int n_agents, int n_steps, int info_words, const float* rewards,
                                          const int32_t* info, const uint8_t* done_all, const uint32_t* float_words,
                                          double* stats, double* episodes, int ep_cap, void* stream) {
    if (!episodes) return hftlob_fail(HFTLOB_EINVAL, "eval_tally_episodes: episodes is NULL");
    if (ep_cap < 1) return hftlob_fail(HFTLOB_EINVAL, "eval_tally_episodes: ep_cap must be >= 1");
    return eval_tally(n_env, n_agents, n_steps, info_words, rewards, info, done_all, float_words, stats, episodes, ep_cap,
                      stream);
}
