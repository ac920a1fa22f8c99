// The training diagnostics' two reductions (include/hftlob.h: hftlob_rollout_diag, hftlob_world_tally), gfx950.
//
// hftlob_rollout_diag reduces one agent type's rollout buffers (N = T * n_actors elements: the action words,
// reward, value, log-prob, advantage, target and the global done) to HFTLOB_DIAG_WORDS doubles: counts, the
// sums and sums of squares of six quantities, and per head the action histogram.  hftlob/train/diag.py
// rollout_diag_reference is the definition, and the result is held to it bit for bit.  Two launches, no
// floating-point atomic, every floating-point sum in one fixed order (the header states it):
//   k_diag_partial  one workgroup of 256 lanes per stripe of the elements (the stripe rule of the header: a
//             function of N alone).  Lane l adds the stripe's elements l, l + 256, ... in that order into
//             twelve double accumulators in registers; the lanes' sums meet in LDS and lane q of the first
//             twelve adds the 256 sums of word q in lane order.  The counts (set done bytes, the heads'
//             histograms and out-of-range words) are 64-bit integer LDS atomics, exact in any order; a head's
//             sum of action words is sum_a a * count[a], an integer.  The workgroup leaves its partial of
//             HFTLOB_DIAG_WORDS doubles in the workspace.
//   k_diag_final    one workgroup; lane w adds word w of the stripes' partials in stripe order.
//
// hftlob_world_tally is the world half of hftlob_eval_tally: one lane per (env, world info word) adds the
// word and its square over the steps in step order, sequentially, into the env's wstats row (in/out).
// hftlob/train/diag.py world_tally_reference is its definition.
//
// No floating-point contraction: every word is a plain double add of a separately rounded product (the
// residual's square and the square of an int32 above 2^26 are inexact in double, so a fused multiply-add
// changes the bits).  The whole library is compiled with -ffp-contract=off (Makefile, HIPFLAGS); the pragma
// below states it for this file whatever the command line says.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/hftlob.h"
#include "hftlob_internal.h"

#pragma clang fp contract(off)

namespace {

constexpr int NT = 256;                                  // lanes per workgroup of k_diag_partial
constexpr int NQ = 6;                                    // quantities with a sum and a sum of squares
constexpr int NF = 2 * NQ;                               // the floating-point words of a partial
constexpr int MAXH = HFTLOB_DIAG_MAX_HEADS, MAXA = HFTLOB_DIAG_MAX_ACTIONS;
constexpr int W_N = 0, W_DONE = 1, W_Q = 2, W_ASUM = W_Q + NF, W_OOR = W_ASUM + MAXH, W_BIN = W_OOR + MAXH;
static_assert(W_BIN + MAXH * MAXA == HFTLOB_DIAG_WORDS, "the diag row of hftlob.h");
constexpr int NCNT = 1 + MAXH + MAXH * MAXA;             // integer counters: done, out of range [k], bins [k][a]
constexpr int NTF = 128;                                 // lanes of k_diag_final
static_assert(NTF >= HFTLOB_DIAG_WORDS, "a lane per word");
constexpr int STRIPE_ROWS = HFTLOB_DIAG_STRIPE_ROWS;
constexpr int MAX_STRIPES = HFTLOB_DIAG_MAX_STRIPES;

// the stripe rule of the header: the elements of a stripe and the number of stripes, from N alone
long long stripe_rows(long long N) {
    const long long g = (N + STRIPE_ROWS - 1) / STRIPE_ROWS;
    return g <= MAX_STRIPES ? STRIPE_ROWS : (N + MAX_STRIPES - 1) / MAX_STRIPES;
}

int stripes(long long N) {
    if (N <= 0) return 0;
    const long long r = stripe_rows(N);
    return (int)((N + r - 1) / r);
}

// the heads' widths, by value
struct Heads {
    int n[MAXH];
};

__global__ __launch_bounds__(NT) void k_diag_partial(long long N, long long rows, int K, Heads nvec,
                                                     const int32_t* __restrict__ action,
                                                     const float* __restrict__ reward,
                                                     const float* __restrict__ value,
                                                     const float* __restrict__ log_prob,
                                                     const float* __restrict__ adv,
                                                     const float* __restrict__ target,
                                                     const uint8_t* __restrict__ done, double* __restrict__ ws) {
    __shared__ double part[NF][NT + 1];                  // (+ 1: the twelve readers of a lane's column spread over banks)
    __shared__ unsigned long long cnt[NCNT];
    const int tid = threadIdx.x;
    const long long begin = (long long)blockIdx.x * rows;
    const long long end = begin + rows < N ? begin + rows : N;
    if (tid < NCNT) cnt[tid] = 0ull;
    __syncthreads();

    double s[NF];
#pragma unroll
    for (int q = 0; q < NF; ++q) s[q] = 0.0;
    unsigned long long n_done = 0ull;
    for (long long i = begin + tid; i < end; i += NT) {
        const double v = (double)value[i], tg = (double)target[i];
        const double x[NQ] = {(double)reward[i], v, (double)log_prob[i], (double)adv[i], tg, tg - v};
#pragma unroll
        for (int q = 0; q < NQ; ++q) {
            const double x2 = x[q] * x[q];
            s[2 * q] += x[q];
            s[2 * q + 1] += x2;
        }
        n_done += done[i] != 0 ? 1ull : 0ull;
        const int32_t* arow = action + i * K;
        for (int k = 0; k < K; ++k) {
            const int32_t a = arow[k];
            const int slot = (a >= 0 && a < nvec.n[k]) ? 1 + MAXH + k * MAXA + a : 1 + k;
            atomicAdd(&cnt[slot], 1ull);
        }
    }
    if (n_done) atomicAdd(&cnt[0], n_done);
#pragma unroll
    for (int q = 0; q < NF; ++q) part[q][tid] = s[q];
    __syncthreads();

    double* out = ws + (long long)blockIdx.x * HFTLOB_DIAG_WORDS;
    if (tid < NF) {                                      // the lanes' sums of word tid, in lane order
        double t = part[tid][0];
        for (int l = 1; l < NT; ++l) t += part[tid][l];
        out[W_Q + tid] = t;
    } else if (tid == NF) {
        out[W_N] = (double)(end - begin);
        out[W_DONE] = (double)cnt[0];
    } else if (tid >= 64 && tid < 64 + MAXH) {           // a head's out-of-range count and its sum of action words
        const int k = tid - 64;
        unsigned long long sum = 0ull;
        for (int a = 0; a < MAXA; ++a) sum += (unsigned long long)a * cnt[1 + MAXH + k * MAXA + a];
        out[W_ASUM + k] = (double)sum;
        out[W_OOR + k] = (double)cnt[1 + k];
    } else if (tid >= 128 && tid < 128 + MAXH * MAXA) {
        out[W_BIN + (tid - 128)] = (double)cnt[1 + MAXH + (tid - 128)];
    }
}
static_assert(NF < 64 && 128 + MAXH * MAXA <= NT, "the writers of a partial are distinct lanes");

__global__ __launch_bounds__(NTF) void k_diag_final(int G, const double* __restrict__ ws, double* __restrict__ diag) {
    const int w = threadIdx.x;
    if (w >= HFTLOB_DIAG_WORDS) return;
    double t = ws[w];
    for (int g = 1; g < G; ++g) t += ws[(long long)g * HFTLOB_DIAG_WORDS + w];
    diag[w] = t;
}

__global__ __launch_bounds__(NT) void k_world_tally(int n_env, int n_steps, int info_words,
                                                    const int32_t* __restrict__ info, uint32_t float_words,
                                                    double* __restrict__ wstats) {
    const long long g = (long long)blockIdx.x * NT + threadIdx.x;
    const long long e = g / HFTLOB_INFO_WORLD_WORDS;
    const int k = (int)(g - e * HFTLOB_INFO_WORLD_WORDS);
    if (e >= n_env) return;
    const bool isf = (float_words >> k) & 1u;
    double* const row = wstats + e * HFTLOB_WORLD_TALLY_WORDS;
    double s = row[2 * k], s2 = row[2 * k + 1];
    const int32_t* src = info + e * info_words + k;
    const long long stride = (long long)n_env * info_words;
    for (int t = 0; t < n_steps; ++t, src += stride) {
        const int32_t w = *src;
        const double x = isf ? (double)__int_as_float(w) : (double)w;
        const double x2 = x * x;
        s += x;
        s2 += x2;
    }
    row[2 * k] = s;
    row[2 * k + 1] = s2;
}

int hip_error(hipError_t err) {
    return err == hipSuccess ? HFTLOB_OK : hftlob_fail(HFTLOB_ELAUNCH, hipGetErrorString(err));
}

}  // namespace

extern "C" long long hftlob_rollout_diag_workspace(long long N) {
    if (N < 0) return hftlob_fail(HFTLOB_ESHAPE, "rollout_diag: N must be >= 0");
    return (long long)stripes(N) * HFTLOB_DIAG_WORDS;
}

extern "C" int hftlob_rollout_diag(long long N, int K, const int* nvec, const int32_t* action, const float* reward,
                                   const float* value, const float* log_prob, const float* adv, const float* target,
                                   const uint8_t* done, double* diag, double* workspace, void* stream) {
    if (N < 0) return hftlob_fail(HFTLOB_ESHAPE, "rollout_diag: N must be >= 0");
    if (K < 1 || K > MAXH) return hftlob_fail(HFTLOB_ESHAPE, "rollout_diag: K must be in 1..4");
    if (!nvec || !diag) return hftlob_fail(HFTLOB_ENULL, "rollout_diag: a null pointer (nvec, diag)");
    if (N > 0 && (!action || !reward || !value || !log_prob || !adv || !target || !done || !workspace))
        return hftlob_fail(HFTLOB_ENULL, "rollout_diag: a null pointer (an input array, workspace)");
    Heads h;
    for (int k = 0; k < MAXH; ++k) h.n[k] = 0;
    for (int k = 0; k < K; ++k) {
        if (nvec[k] < 1 || nvec[k] > MAXA) return hftlob_fail(HFTLOB_EINVAL, "rollout_diag: an nvec entry outside 1..16");
        h.n[k] = nvec[k];
    }
    hipStream_t s = (hipStream_t)stream;
    if (N == 0)   // an empty rollout: zeros, and nothing else is read
        return hip_error(hipMemsetAsync(diag, 0, sizeof(double) * HFTLOB_DIAG_WORDS, s));
    const long long rows = stripe_rows(N);
    const int G = stripes(N);
    k_diag_partial<<<dim3((unsigned)G), NT, 0, s>>>(N, rows, K, h, action, reward, value, log_prob, adv, target, done,
                                                    workspace);
    k_diag_final<<<dim3(1), NTF, 0, s>>>(G, workspace, diag);
    return hip_error(hipGetLastError());
}

extern "C" int hftlob_world_tally(int n_env, int n_steps, int info_words, const int32_t* info, uint32_t float_words,
                                  double* wstats, void* stream) {
    if (n_env < 1 || n_steps < 1) return hftlob_fail(HFTLOB_ESHAPE, "world_tally: n_env and n_steps must be >= 1");
    if (info_words < HFTLOB_INFO_WORLD_WORDS)
        return hftlob_fail(HFTLOB_ESHAPE, "world_tally: info_words is smaller than the world's info block");
    if (!info || !wstats) return hftlob_fail(HFTLOB_ENULL, "world_tally: a null pointer");
    if (float_words >> HFTLOB_INFO_WORLD_WORDS)
        return hftlob_fail(HFTLOB_EINVAL, "world_tally: float_words names a word past the world's info block");
    const long long lanes = (long long)n_env * HFTLOB_INFO_WORLD_WORDS;
    const long long blocks = (lanes + NT - 1) / NT;
    k_world_tally<<<dim3((unsigned)blocks), NT, 0, (hipStream_t)stream>>>(n_env, n_steps, info_words, info, float_words,
                                                                          wstats);
    return hip_error(hipGetLastError());
}
