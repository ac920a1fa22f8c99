// The IPPO update's objective as engine operators (include/hftlob.h: hftlob_gae, hftlob_ppo_loss),
// gfx950, float32.  hftlob/train/ippo.py calculate_gae and ppo_loss_multi are the definitions;
// hftlob/train/loss.py restates both operators in torch.
//
// hftlob_gae: one lane per actor walks t = T-1 .. 0 with gae and next_value in registers; consecutive
// lanes read consecutive floats of every [T][n] array.  Every operation is a separately rounded float32
// op in calculate_gae's order, so the result is that loop's bit for bit.
//
// hftlob_ppo_loss: three launches, no floating-point atomic, every sum combined in a fixed order.
//   k_moments  up to MOM_BLOCKS workgroups: double sums of (adv - adv[0]) and its square, one pair per
//              workgroup into the workspace (the shift by adv[0] keeps the squares small when
//              |mean| >> std)
//   k_loss     a workgroup owns LOSS_ROWS consecutive elements.  16 lanes hold one head of one element
//              (lane j its logit j), so a wave holds 4 / Kp elements at a time, Kp = K rounded up to a
//              power of two; max, sum, entropy and the action's log-probability are xor-shuffle
//              reductions inside the 16 lanes, the sums over the heads xor-shuffles between the groups.
//              Every wave first folds the moment pairs (the same order in every wave, so the same
//              bits).  logits is read once and d_logits written once, the per-element tail is computed
//              by all lanes of the element and stored by one.  The five per-element terms are summed in
//              double per lane, then over the wave and the workgroup, one row of five per workgroup
//              into the workspace.
//   k_final    one workgroup sums the rows in a fixed order and writes the six scalars.
//
// No floating-point contraction, as in the rest of the library (Makefile, HIPFLAGS): hftlob_gae's bits
// depend on it.  The pragma states it for this file whatever the command line says.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/hftlob.h"
#include "hftlob_internal.h"

#pragma clang fp contract(off)

namespace {

constexpr int NT = 256;                              // lanes per workgroup
constexpr int MAX_HEADS = 4, MAX_ACTIONS = 16;       // the policy step's limits
constexpr int LOSS_ROWS = HFTLOB_PPO_LOSS_ROWS;      // elements per workgroup of k_loss
constexpr int MOM_BLOCKS = 64;                       // at most one moment pair per lane of a wave
constexpr int NSUM = 5;                              // max(u^2, c^2), min(a, b), entropy, kl, clipped
constexpr int WS_SUMS = 2 * MOM_BLOCKS;              // workspace: the moment pairs, then NSUM per workgroup
static_assert(LOSS_ROWS % 16 == 0, "a workgroup's four waves hold up to 16 elements at a time");
static_assert(WS_SUMS == HFTLOB_PPO_LOSS_WS_HEAD, "the workspace formula of hftlob.h");
static_assert(NSUM == HFTLOB_PPO_LOSS_WS_ROW, "the workspace formula of hftlob.h");

__global__ __launch_bounds__(NT) void k_gae(int T, long long n, const float* __restrict__ reward,
                                            const float* __restrict__ value, const uint8_t* __restrict__ done,
                                            const float* __restrict__ last_val, float gamma, float gamma_lambda,
                                            float* __restrict__ adv, float* __restrict__ targets) {
    const long long i = (long long)blockIdx.x * NT + threadIdx.x;
    if (i >= n) return;
    float gae = 0.0f, next_value = last_val[i];
    for (long long o = (long long)(T - 1) * n + i; o >= 0; o -= n) {
        const float nd = 1.0f - (done[o] ? 1.0f : 0.0f);
        const float v = value[o];
        const float delta = (reward[o] + (gamma * next_value) * nd) - v;
        gae = delta + ((gamma_lambda * nd) * gae);
        adv[o] = gae;
        targets[o] = gae + v;
        next_value = v;
    }
}

__device__ __forceinline__ double wave_sum(double v) {
    for (int m = 1; m < 64; m <<= 1) v += __shfl_xor(v, m);
    return v;
}

__global__ __launch_bounds__(NT) void k_moments(long long N, const float* __restrict__ adv, double* __restrict__ ws) {
    __shared__ double part[2][NT / 64];
    const float x0 = adv[0];
    double s1 = 0.0, s2 = 0.0;
    for (long long i = (long long)blockIdx.x * NT + threadIdx.x; i < N; i += (long long)gridDim.x * NT) {
        const double d = (double)adv[i] - (double)x0;
        s1 += d;
        s2 += d * d;
    }
    s1 = wave_sum(s1);
    s2 = wave_sum(s2);
    if ((threadIdx.x & 63) == 0) part[0][threadIdx.x >> 6] = s1, part[1][threadIdx.x >> 6] = s2;
    __syncthreads();
    if (threadIdx.x == 0) {
        ws[2 * blockIdx.x] = ((part[0][0] + part[0][1]) + part[0][2]) + part[0][3];
        ws[2 * blockIdx.x + 1] = ((part[1][0] + part[1][1]) + part[1][2]) + part[1][3];
    }
}

// the heads' widths and first columns, by value
struct Heads {
    int n[MAX_HEADS], off[MAX_HEADS];
};

struct LossArgs {
    long long N;
    int K, S, kshift, mom_blocks;   // kshift: log2 of K rounded up to a power of two
    Heads hd;
    float eps, lo, hi, vf_coef, ent_coef;
};

__device__ __forceinline__ int pick4(const int (&a)[MAX_HEADS], int k) {   // selects, not an indexed (scratch) array
    return k == 0 ? a[0] : k == 1 ? a[1] : k == 2 ? a[2] : a[3];
}

__global__ __launch_bounds__(NT) void k_loss(LossArgs p, const float* __restrict__ logits,
                                             const float* __restrict__ values, const int32_t* __restrict__ actions,
                                             const float* __restrict__ rb_value, const float* __restrict__ rb_log_prob,
                                             const float* __restrict__ adv, const float* __restrict__ targets,
                                             double* __restrict__ ws, float* __restrict__ d_logits,
                                             float* __restrict__ d_values) {
    __shared__ double part[NSUM][NT / 64];
    const int l = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int j = l & 15, grp = l >> 4;
    const int k = grp & ((1 << p.kshift) - 1);           // the lane group's head
    const int rpw = 4 >> p.kshift;                       // elements a wave holds at a time
    const bool head = k < p.K;
    const int nk = head ? pick4(p.hd.n, k) : 0, offk = head ? pick4(p.hd.off, k) : 0;
    const bool col = j < nk;
    const bool first = j == 0 && k == 0;                 // lane 0 of an element's first group: its stores and sums

    // mean and population std of adv from the moment pairs, the same fold in every wave
    double m1 = 0.0, m2 = 0.0;
    if (l < p.mom_blocks) m1 = ws[2 * l], m2 = ws[2 * l + 1];
    m1 = wave_sum(m1) / (double)p.N;
    m2 = wave_sum(m2) / (double)p.N;
    const double var = m2 - m1 * m1;
    const float mean = (float)((double)adv[0] + m1);
    const float sdev = (float)sqrt(var > 0.0 ? var : 0.0);
    const float inv_n = 1.0f / (float)p.N;

    double acc[NSUM] = {0.0, 0.0, 0.0, 0.0, 0.0};
    const long long base = (long long)blockIdx.x * LOSS_ROWS;
    for (int it = 0; it < LOSS_ROWS; it += 4 * rpw) {
        const long long i = base + it + wave * rpw + (grp >> p.kshift);
        const bool live = i < p.N;
        const bool ld = live && col;
        const float x = ld ? logits[i * p.S + offk + j] : -INFINITY;
        const int a = (live && head) ? (actions[i * p.K + k] & 15) : 0;

        // the head's log-softmax, entropy and log-probability at its action, inside the 16 lanes
        float mx = x;
        for (int m = 1; m < 16; m <<= 1) mx = fmaxf(mx, __shfl_xor(mx, m));
        const float xs = ld ? x - mx : 0.0f;
        const float e = ld ? expf(xs) : 0.0f;
        float sum = e;
        for (int m = 1; m < 16; m <<= 1) sum += __shfl_xor(sum, m);
        const float lpj = ld ? xs - logf(sum) : 0.0f;
        const float pj = ld ? e / sum : 0.0f;
        float hk = pj * lpj;
        for (int m = 1; m < 16; m <<= 1) hk += __shfl_xor(hk, m);
        hk = -hk;                                       // H_k (0 in a dead group)
        float logp = __shfl(lpj, (l & 48) | a);
        float ent = hk;
        if (p.kshift >= 1) logp += __shfl_xor(logp, 16), ent += __shfl_xor(ent, 16);
        if (p.kshift == 2) logp += __shfl_xor(logp, 32), ent += __shfl_xor(ent, 32);

        // the element's tail, in every lane of the element
        float A = 0.0f, v = 0.0f, rbv = 0.0f, rblp = 0.0f, tgt = 0.0f;
        if (live) A = adv[i], v = values[i], rbv = rb_value[i], rblp = rb_log_prob[i], tgt = targets[i];
        A = (A - mean) / (sdev + 1e-8f);
        const float lr = logp - rblp;
        const float ratio = expf(lr);
        const bool inside = ratio >= p.lo && ratio <= p.hi;
        const float sa = ratio * A, sb = fminf(fmaxf(ratio, p.lo), p.hi) * A;
        const float w = sa < sb ? 1.0f : sa > sb ? 0.0f : (inside ? 1.0f : 0.5f);
        const float u = v - tgt, dv = v - rbv;
        const bool vin = dv >= -p.eps && dv <= p.eps;
        const float c = (rbv + fminf(fmaxf(dv, -p.eps), p.eps)) - tgt;
        const float u2 = u * u, c2 = c * c;
        const float cg = vin ? c : 0.0f;
        const float gv = u2 > c2 ? u : u2 < c2 ? cg : 0.5f * u + 0.5f * cg;

        if (d_logits) {   // (both or neither, checked on the host)
            if (ld) {
                const float g_lp = -((A * w) * ratio) * inv_n;
                d_logits[i * p.S + offk + j] =
                    g_lp * ((j == a ? 1.0f : 0.0f) - pj) + (p.ent_coef * inv_n) * (pj * (lpj + hk));
            }
            if (live && first) d_values[i] = (p.vf_coef * gv) * inv_n;
        }
        if (live && first) {
            acc[0] += (double)fmaxf(u2, c2);
            acc[1] += (double)fminf(sa, sb);
            acc[2] += (double)ent;
            acc[3] += (double)((ratio - 1.0f) - lr);
            acc[4] += fabsf(ratio - 1.0f) > p.eps ? 1.0 : 0.0;
        }
    }

    for (int q = 0; q < NSUM; ++q) {
        const double s = wave_sum(acc[q]);
        if (l == 0) part[q][wave] = s;
    }
    __syncthreads();
    if (threadIdx.x < NSUM) {
        const int q = threadIdx.x;
        ws[WS_SUMS + (long long)blockIdx.x * NSUM + q] = ((part[q][0] + part[q][1]) + part[q][2]) + part[q][3];
    }
}

__global__ __launch_bounds__(NT) void k_final(long long N, long long blocks, double vf_coef, double ent_coef,
                                              const double* __restrict__ ws, float* __restrict__ out6) {
    __shared__ double part[NSUM][NT];
    double s[NSUM] = {0.0, 0.0, 0.0, 0.0, 0.0};
    for (long long b = threadIdx.x; b < blocks; b += NT)
        for (int q = 0; q < NSUM; ++q) s[q] += ws[WS_SUMS + b * NSUM + q];
    for (int q = 0; q < NSUM; ++q) part[q][threadIdx.x] = s[q];
    __syncthreads();
    for (int h = NT / 2; h > 0; h >>= 1) {
        if ((int)threadIdx.x < h)
            for (int q = 0; q < NSUM; ++q) part[q][threadIdx.x] += part[q][threadIdx.x + h];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const double n = (double)N;
        const double value_loss = 0.5 * (part[0][0] / n), actor_loss = -(part[1][0] / n), entropy = part[2][0] / n;
        out6[0] = (float)(actor_loss + vf_coef * value_loss - ent_coef * entropy);
        out6[1] = (float)value_loss;
        out6[2] = (float)actor_loss;
        out6[3] = (float)entropy;
        out6[4] = (float)(part[3][0] / n);
        out6[5] = (float)(part[4][0] / n);
    }
}

int launched() {
    const hipError_t err = hipGetLastError();
    return err == hipSuccess ? HFTLOB_OK : hftlob_fail(HFTLOB_ELAUNCH, hipGetErrorString(err));
}

}  // namespace

extern "C" int hftlob_gae(int T, int n, const float* reward, const float* value, const uint8_t* done,
                          const float* last_val, float gamma, float gamma_lambda, float* adv, float* targets,
                          void* stream) {
    if (T < 1 || n < 1) return hftlob_fail(HFTLOB_EINVAL, "gae: T and n must be >= 1");
    if (!reward || !value || !done || !last_val || !adv || !targets)
        return hftlob_fail(HFTLOB_ENULL, "gae: a null pointer (reward, value, done, last_val, adv, targets)");
    const unsigned blocks = (unsigned)(((long long)n + NT - 1) / NT);
    k_gae<<<dim3(blocks), NT, 0, (hipStream_t)stream>>>(T, (long long)n, reward, value, done, last_val, gamma,
                                                        gamma_lambda, adv, targets);
    return launched();
}

extern "C" int hftlob_ppo_loss(int N, int K, const int* nvec, const float* logits, const float* values,
                               const int32_t* actions, const float* rb_value, const float* rb_log_prob,
                               const float* adv, const float* targets, double clip_eps, double vf_coef,
                               double ent_coef, double* workspace, float* out6, float* d_logits, float* d_values,
                               void* stream) {
    if (N < 1) return hftlob_fail(HFTLOB_EINVAL, "ppo_loss: N must be >= 1");
    if (K < 1 || K > MAX_HEADS) return hftlob_fail(HFTLOB_EINVAL, "ppo_loss: K must be in 1..4");
    if (!nvec) return hftlob_fail(HFTLOB_ENULL, "ppo_loss: nvec is NULL");
    LossArgs p;
    p.N = N;
    p.K = K;
    p.S = 0;
    for (int k = 0; k < MAX_HEADS; ++k) {
        p.hd.n[k] = p.hd.off[k] = 0;
        if (k >= K) continue;
        if (nvec[k] < 1 || nvec[k] > MAX_ACTIONS) return hftlob_fail(HFTLOB_EINVAL, "ppo_loss: nvec[k] must be in 1..16");
        p.hd.n[k] = nvec[k];
        p.hd.off[k] = p.S;
        p.S += nvec[k];
    }
    if (!logits || !values || !actions || !rb_value || !rb_log_prob || !adv || !targets || !workspace || !out6)
        return hftlob_fail(HFTLOB_ENULL, "ppo_loss: a null pointer (logits, values, actions, rb_value, rb_log_prob, "
                                         "adv, targets, workspace, out6)");
    if (!d_logits != !d_values)
        return hftlob_fail(HFTLOB_EINVAL, "ppo_loss: d_logits and d_values must both be given or both be NULL");
    p.kshift = K == 1 ? 0 : K == 2 ? 1 : 2;
    const long long blocks = ((long long)N + LOSS_ROWS - 1) / LOSS_ROWS;
    const long long mom = ((long long)N + NT - 1) / NT;
    p.mom_blocks = (int)(mom < MOM_BLOCKS ? mom : MOM_BLOCKS);
    p.eps = (float)clip_eps;
    p.lo = (float)(1.0 - clip_eps);
    p.hi = (float)(1.0 + clip_eps);
    p.vf_coef = (float)vf_coef;
    p.ent_coef = (float)ent_coef;
    hipStream_t s = (hipStream_t)stream;
    k_moments<<<dim3((unsigned)p.mom_blocks), NT, 0, s>>>((long long)N, adv, workspace);
    k_loss<<<dim3((unsigned)blocks), NT, 0, s>>>(p, logits, values, actions, rb_value, rb_log_prob, adv, targets,
                                                 workspace, d_logits, d_values);
    k_final<<<dim3(1), NT, 0, s>>>((long long)N, blocks, vf_coef, ent_coef, workspace, out6);
    return launched();
}
