// Fused recurrent policy step for IPPO rollouts and policy evaluation (include/hftlob.h:
// hftlob_policy_step, hftlob_policy_step_multi for MultiDiscrete action spaces, and
// hftlob_policy_step_grouped, which steps several independent nets' batches in one launch), gfx950.
//
// One ActorCriticRNN step (jaxrl/MARL/ippo_rnn_JAXMARL.py:53-78, 183-256) for a batch of actors as
// one launch: embedding, GRU cell, critic and actor heads, softmax, the sample (or the argmax) and
// its log-probability.  A workgroup owns a tile of 16 batch rows, the M side of the f32-input
// 16x16x4 MFMA (hftlob_tile.h, shared with gru_scan.hip), and waits on no other workgroup.  Every
// product is that MFMA, so every dot product is a k-ordered fmaf chain in float32.
//
// The layers chain through LDS, three padded [16][W + 4] buffers:
//     bx   x = relu(embed)            then relu(critic1) once the gates are done
//     bp   h_prev                     then relu(actor1)
//     bh   obs (zero-padded to 64 k)  then h
// with a barrier after the embedding, after the gates and after the two hidden head layers.
//
//   embedding  a wave takes column blocks w, w + NW, ... of x; k = D <= 64 is padded to 16 MFMAs, the
//              B operand is w_embed read as dwords (its rows are D floats, not 16-byte aligned)
//   gates      a wave owns CB blocks of 16 hidden indices j and computes gi and gh of the r, z and n
//              columns of those j, so the gate math runs in registers on the accumulators
//   heads      critic1 (FC columns) and actor1 (H columns) read the same h: their (FC + H) / 16
//              column blocks are dealt over the waves, a wave's blocks run together on one A operand
//   outputs    wave 0: a head's logits = relu(actor1) . w_a2[its rows]^T are one MFMA column block (<= 16
//              logits), then its softmax, Gumbel noise and first argmax over 16-lane rows.  The heads
//              (:80-100, 259-281; one for hftlob_policy_step, K <= 4 for the multi-head operator) are
//              NHD such blocks on the one A operand, each with its own row offset, width, key and
//              counters; the log-probs add up in head order.  wave 1: value, a 16-row dot product
//              over FC reduced across the lane quarters
//
// The weights (about 2.1 MB at 256 / 256) stream from L2 as float4 per lane into register buffers
// two chunks of 32 k ahead of the MFMAs that use them; the k order inside a chunk is permuted so that
// both operands are 16-byte reads (lane quarter q of chunk c has k = 32 c + 8 q + 0..7, as in
// k_gru_scan_fwd).  Loads are unconditional at clamped indices, no branch sits between a prefetch and
// its wait, and a sched_barrier keeps the loads where they are issued.  A stage's first chunks are
// requested before the previous stage's epilogue and barrier.
#include <stdint.h>
#include <stdio.h>

#include "hftlob_draw.h"  // threefry_bits, gumbel_from_bits
#include "hftlob_tile.h"  // f32x4, ld4 / splat, sigmoidf_, TILE and the MFMA operand maps

namespace {

typedef uint32_t u32;

constexpr int PF = 2;     // weight chunks in flight per stream
constexpr int DMAX = 64;  // obs columns in LDS (D <= 64, zero-padded)

// the partitionable threefry's random word and jax.random.gumbel's float32 draw from it
using hftlob_draw::gumbel_from_bits;
using hftlob_draw::threefry_bits;

// the first PF chunks of N weight rows (wp[n] is the lane's row, already at its quarter's 8 q)
template <int N>
__device__ __forceinline__ void prefetch(f32x4 (&wv)[PF][N][2], const float* const (&wp)[N]) {
#pragma unroll
    for (int p = 0; p < PF; ++p)
#pragma unroll
        for (int n = 0; n < N; ++n) {
            wv[p][n][0] = ld4(wp[n] + 32 * p);
            wv[p][n][1] = ld4(wp[n] + 32 * p + 4);
        }
}

// one chunk of 32 k: acc[n] += A (two float4 of the lane's LDS row) . wv[n], then the slot's refill
template <int N>
__device__ __forceinline__ void chunk(f32x4 (&acc)[N], f32x4 (&wv)[N][2], const float* ap, const float* const (&np)[N],
                                      int noff) {
    const f32x4 a[2] = {ld4(ap), ld4(ap + 4)};
#pragma unroll
    for (int s = 0; s < 8; ++s)
#pragma unroll
        for (int n = 0; n < N; ++n)
            acc[n] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[s >> 2][s & 3], wv[n][s >> 2][s & 3], acc[n], 0, 0, 0);
#pragma unroll
    for (int n = 0; n < N; ++n) {
        wv[n][0] = ld4(np[n] + noff);
        wv[n][1] = ld4(np[n] + noff + 4);
    }
    __builtin_amdgcn_sched_barrier(0);  // the loads stay here: a chunk of MFMAs between issue and use
}

// acc[n] += A[16][K] . W_n^T over K in chunks of 32, wv holding the first PF chunks on entry.  The
// prefetch is unconditional: the last PF chunks fetch the first PF chunks of wnext (the stream that
// follows, or wp again where nothing follows; those are never used)
template <int N, int K>
__device__ __forceinline__ void stream(f32x4 (&acc)[N], f32x4 (&wv)[PF][N][2], const float* const (&wp)[N],
                                       const float* const (&wnext)[N], const float* ap) {
    constexpr int NCH = K / 32;
    static_assert(NCH % PF == 0, "the k loop is unrolled by PF chunks");
#pragma unroll 1
    for (int ch = 0; ch < NCH - PF; ch += PF) {
#pragma unroll
        for (int p = 0; p < PF; ++p) chunk<N>(acc, wv[p], ap + 32 * (ch + p), wp, 32 * (ch + p + PF));
    }
#pragma unroll
    for (int p = 0; p < PF; ++p) chunk<N>(acc, wv[p], ap + 32 * (NCH - PF + p), wnext, 32 * p);
}

template <int H, int FC>
struct Shape {
    static constexpr int CB = H == 256 ? 2 : 1;                   // hidden column blocks per wave
    static constexpr int NW = H / 16 / CB;                        // waves
    static constexpr int NT = 64 * NW;
    static constexpr int NBE = (FC / 16 + NW - 1) / NW;           // embedding column blocks per wave
    static constexpr int NBH = ((FC + H) / 16 + NW - 1) / NW;     // head column blocks per wave
};

constexpr int MAXK = 4;  // action heads of the multi-head operator: the logits stage's column blocks

// the action heads, by value: head k has nv[k] logits from row off[k] of w_a2, S logits in all; the
// entries past K repeat head K - 1 (their loads stay in bounds, their results are dropped)
struct Heads {
    int K, S;
    int nv[MAXK], off[MAXK];
};

// one row's head: the first argmax of the scores sc over the head's nv live lanes of a 16-lane row, and
// the log-softmax of the logits x at it.  Every lane of the row returns the same pair
__device__ __forceinline__ void head_pick(float x, float sc, bool live_a, int l, int li, int& idx, float& lp) {
    sc = live_a ? sc : -INFINITY;
    idx = li;
    float mx = live_a ? x : -INFINITY;
#pragma unroll
    for (int m = 1; m < 16; m <<= 1) {
        const float os = __shfl_xor(sc, m);
        const int oi = __shfl_xor(idx, m);
        if (os > sc || (os == sc && oi < idx)) {
            sc = os;
            idx = oi;
        }
        mx = fmaxf(mx, __shfl_xor(mx, m));
    }
    float sum = live_a ? expf(x - mx) : 0.0f;
#pragma unroll
    for (int m = 1; m < 16; m <<= 1) sum += __shfl_xor(sum, m);
    const float xa = __shfl(x, (l & 48) | idx);
    lp = xa - mx - logf(sum);
}

// A batch as the kernel takes it: the operators' arguments (hftlob_policy_group's fields) with the heads'
// offsets worked out
struct Group {
    int B, D;
    Heads hd;
    hftlob_policy_weights W;
    const float* obs;
    const uint8_t* done;
    const float* h_in;
    float* h_out;
    const u32* key;
    int32_t* action;
    float *log_prob, *value, *logits;
};

// The batches of a launch, by value in the kernel arguments, as gru_scan.hip's table travels: the call
// needs no copy to the device and can be captured in a graph.  first[g] is group g's first tile,
// first[MG] the grid; the unused entries repeat group 0 and have no tiles.  MG is 1 for the single-batch
// operators (no lookup: the table is the batch) and HFTLOB_POLICY_MAX_GROUPS for hftlob_policy_step_grouped
template <int MG>
struct GroupTable {
    Group g[MG];
    int first[MG + 1];
};
constexpr int MAXG = HFTLOB_POLICY_MAX_GROUPS;
static_assert(sizeof(GroupTable<MAXG>) <= 4096, "the group table travels in the kernel arguments");

// The step of a tile: hd.K <= NHD heads, key [K][2], action [B][K], logits [B][S].  NHD is the number of
// column blocks the logits stage runs on the one A operand in wave 0: 1 where every batch has one head
// (hftlob_policy_step: action [B] and logits [B][A]), MAXK otherwise (hftlob_policy_step_multi).
// One kernel serves the single-batch operators and the grouped launch.  A workgroup of the grouped launch
// finds its group from blockIdx once: the index is wave-uniform, so the group's sizes and pointers are
// scalar loads from the kernarg segment, as the single batch's are.  The body stays in the kernel: as a
// __device__ function of a tile, inlined into two kernels, the same text compiles to a different schedule
// that spills at H = 256 ("The grouped policy step")
template <int H, int FC, int NHD, int MG>
__global__ __launch_bounds__((Shape<H, FC>::NT)) void k_policy_step(const GroupTable<MG> tb, int mode) {
    int grp = 0;
    if constexpr (MG > 1)
        while ((int)blockIdx.x >= tb.first[grp + 1]) ++grp;  // (the grid is first[MG] workgroups: grp stays below MG)
    const Group& x = tb.g[grp];
    const int B = x.B, D = x.D;
    const Heads& hd = x.hd;
    const hftlob_policy_weights& W = x.W;
    const float* __restrict__ obs = x.obs;
    const uint8_t* __restrict__ done = x.done;
    const float* h_in = x.h_in;
    float* h_out = x.h_out;
    const u32* __restrict__ key = x.key;
    int32_t* __restrict__ action = x.action;
    float* __restrict__ log_prob = x.log_prob;
    float* __restrict__ value = x.value;
    float* __restrict__ logits = x.logits;
    typedef Shape<H, FC> Sh;
    constexpr int CB = Sh::CB, NW = Sh::NW, NT = Sh::NT, NBE = Sh::NBE, NBH = Sh::NBH;
    constexpr int SX = FC + 4, SH = H + 4, NG = 3 * CB;
    static_assert(H >= DMAX, "the obs tile lives in the h buffer");
    __shared__ __attribute__((aligned(16))) float bx[TILE * SX];  // x, then relu(critic1)
    __shared__ __attribute__((aligned(16))) float bp[TILE * SH];  // h_prev, then relu(actor1)
    __shared__ __attribute__((aligned(16))) float bh[TILE * SH];  // obs, then h
    const int tid = threadIdx.x, w = tid >> 6, l = tid & 63, li = l & 15, q = l >> 4;
    const int b0 = ((int)blockIdx.x - (MG > 1 ? tb.first[grp] : 0)) * TILE;

    // the gates' W_ih rows and the embedding's B operands, requested before anything waits
    int col[CB];
    const float *wpi[NG], *wph[NG];
#pragma unroll
    for (int c = 0; c < CB; ++c) {
        col[c] = (w * CB + c) * 16 + li;
#pragma unroll
        for (int g = 0; g < 3; ++g) {
            wpi[c * 3 + g] = W.w_ih + (size_t)(g * H + col[c]) * FC + 8 * q;
            wph[c * 3 + g] = W.w_hh + (size_t)(g * H + col[c]) * H + 8 * q;
        }
    }
    f32x4 wg[PF][NG][2];
    prefetch<NG>(wg, wpi);
    float we[NBE][DMAX / 4];  // w_embed[col][4 s + q], zero past D
#pragma unroll
    for (int e = 0; e < NBE; ++e) {
        const int ecol = min(w + NW * e, FC / 16 - 1) * 16 + li;
#pragma unroll
        for (int s = 0; s < DMAX / 4; ++s) {
            const int k = 4 * s + q;
            const float v = W.w_embed[(size_t)ecol * D + min(k, D - 1)];
            we[e][s] = k < D ? v : 0.0f;
        }
    }

    // the tile's obs and h_prev = done ? 0 : h_in, at clamped rows (a row past B repeats row B - 1 and
    // is never stored)
    for (int i = tid; i < TILE * DMAX; i += NT) {
        const int row = i / DMAX, k = i % DMAX, b = min(b0 + row, B - 1);
        const float v = obs[(size_t)b * D + min(k, D - 1)];
        bh[row * SH + k] = k < D ? v : 0.0f;
    }
    for (int i = tid; i < TILE * H; i += NT) {
        const int row = i / H, j = i % H, b = min(b0 + row, B - 1);
        const float v = h_in[(size_t)b * H + j];
        bp[row * SH + j] = done[b] ? 0.0f : v;
    }
    __syncthreads();

    // x = relu(obs . w_embed^T + b_embed)
#pragma unroll
    for (int e = 0; e < NBE; ++e) {
        const int blk = w + NW * e, ecol = min(blk, FC / 16 - 1) * 16 + li;
        f32x4 acc = splat(W.b_embed[ecol]);
#pragma unroll
        for (int s = 0; s < DMAX / 4; ++s)
            acc = __builtin_amdgcn_mfma_f32_16x16x4f32(bh[li * SH + 4 * s + q], we[e][s], acc, 0, 0, 0);
        if (blk < FC / 16) {
#pragma unroll
            for (int i = 0; i < 4; ++i) bx[(4 * q + i) * SX + ecol] = fmaxf(acc[i], 0.0f);
        }
    }
    f32x4 gi[NG], gh[NG];
#pragma unroll
    for (int c = 0; c < CB; ++c)
#pragma unroll
        for (int g = 0; g < 3; ++g) {
            gi[c * 3 + g] = splat(W.b_ih[g * H + col[c]]);
            gh[c * 3 + g] = splat(W.b_hh[g * H + col[c]]);
        }
    __syncthreads();  // x complete; every read of obs is behind us

    // gi = x . w_ih^T + b_ih and gh = h_prev . w_hh^T + b_hh of the wave's columns
    stream<NG, FC>(gi, wg, wpi, wph, bx + li * SX + 8 * q);
    stream<NG, H>(gh, wg, wph, wph, bp + li * SH + 8 * q);

    // the heads' first chunks, in flight under the gate math.  Head block k < FC / 16 is a block of
    // critic1's columns, the others are actor1's; a wave's block past the last repeats the last
    int hblk[NBH], hcol[NBH];
    const float* wpc[NBH];
    float hbias[NBH];
#pragma unroll
    for (int n = 0; n < NBH; ++n) {
        hblk[n] = w + NW * n;
        const int blk = min(hblk[n], (FC + H) / 16 - 1);
        const bool critic = blk < FC / 16;
        hcol[n] = (critic ? blk : blk - FC / 16) * 16 + li;
        wpc[n] = (critic ? W.w_c1 : W.w_a1) + (size_t)hcol[n] * H + 8 * q;
        hbias[n] = (critic ? W.b_c1 : W.b_a1)[hcol[n]];
    }
    f32x4 wh[PF][NBH][2];
    prefetch<NBH>(wh, wpc);
    __builtin_amdgcn_sched_barrier(0);

#pragma unroll
    for (int c = 0; c < CB; ++c)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int row = 4 * q + i;
            const float hp = bp[row * SH + col[c]];
            const float r = sigmoidf_(gi[c * 3 + 0][i] + gh[c * 3 + 0][i]);
            const float z = sigmoidf_(gi[c * 3 + 1][i] + gh[c * 3 + 1][i]);
            const float n = tanhf(gi[c * 3 + 2][i] + r * gh[c * 3 + 2][i]);
            const float h = (1.0f - z) * n + z * hp;
            if (b0 + row < B) h_out[(size_t)(b0 + row) * H + col[c]] = h;
            bh[row * SH + col[c]] = h;
        }
    __syncthreads();  // h complete; x and h_prev are dead

    // relu(critic1) -> bx, relu(actor1) -> bp
    f32x4 ha[NBH];
#pragma unroll
    for (int n = 0; n < NBH; ++n) ha[n] = splat(hbias[n]);
    stream<NBH, H>(ha, wh, wpc, wpc, bh + li * SH + 8 * q);

    // the logits' first chunks (wave 0 uses them), in flight under the stores and the barrier; rows
    // of w_a2 past a head's last repeat that row and their columns are masked below
    int arow[NHD];
    const float* wpa[NHD];
#pragma unroll
    for (int n = 0; n < NHD; ++n) {
        arow[n] = hd.off[n] + min(li, hd.nv[n] - 1);
        wpa[n] = W.w_a2 + (size_t)arow[n] * H + 8 * q;
    }
    f32x4 wa[PF][NHD][2];
    prefetch<NHD>(wa, wpa);
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int n = 0; n < NBH; ++n) {
        if (hblk[n] < (FC + H) / 16) {
            float* dst = hblk[n] < FC / 16 ? bx + hcol[n] : bp + hcol[n];
            const int S = hblk[n] < FC / 16 ? SX : SH;
#pragma unroll
            for (int i = 0; i < 4; ++i) dst[(4 * q + i) * S] = fmaxf(ha[n][i], 0.0f);
        }
    }
    __syncthreads();  // both hidden head layers complete

    if (w == 1) {  // value = relu(critic1) . w_c2^T + b_c2: lane quarter q sums a quarter of FC for row li
        float v = 0.0f;
        const float* xr = bx + li * SX + q * (FC / 4);
        const float* wr = W.w_c2 + q * (FC / 4);
#pragma unroll 8
        for (int k = 0; k < FC / 4; ++k) v = fmaf(xr[k], wr[k], v);
        v += __shfl_xor(v, 16);
        v += __shfl_xor(v, 32);
        if (q == 0 && b0 + li < B) value[b0 + li] = v + W.b_c2[0];
    }
    if (w != 0) return;

    // logits of the tile: accumulator i of lane (li, q) is row 4 q + i, action li of head n
    f32x4 lg[NHD];
#pragma unroll
    for (int n = 0; n < NHD; ++n) lg[n] = splat(W.b_a2[arow[n]]);
    stream<NHD, H>(lg, wa, wpa, wpa, bp + li * SH + 8 * q);
    // head n's noise is drawn from key[n] at counter (0, b nv[n] + a); log_prob adds the heads in order
    float lps[4];
#pragma unroll
    for (int n = 0; n < NHD; ++n) {
        if (n >= hd.K) break;  // wave-uniform, and no load is in flight any more
        const int An = hd.nv[n];
        const bool live_a = li < An;
        u32 k0 = 0, k1 = 0;
        if (mode == 0) {
            k0 = key[2 * n];
            k1 = key[2 * n + 1];
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int b = b0 + 4 * q + i;
            const bool live = b < B;
            const float x = lg[n][i];
            if (logits && live && live_a) logits[(size_t)b * hd.S + hd.off[n] + li] = x;
            float sc = x;
            if (mode == 0)
                sc = x + gumbel_from_bits(threefry_bits(k0, k1, 0u, (u32)min(b, B - 1) * (u32)An + (u32)li));
            int idx;
            float lp;
            head_pick(x, sc, live_a, l, li, idx, lp);
            lps[i] = n == 0 ? lp : lps[i] + lp;
            if (live && li == 0) action[(size_t)b * hd.K + n] = idx;
        }
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int b = b0 + 4 * q + i;
        if (b < B && li == 0) log_prob[b] = lps[i];
    }
}

bool size_ok(int n) { return n == 64 || n == 128 || n == 256; }
bool misaligned(const void* p) { return ((uintptr_t)p & 15) != 0; }

#define HFTLOB_POLICY_CASES   \
    HFTLOB_POLICY_CASE(64, 64)    \
    HFTLOB_POLICY_CASE(64, 128)   \
    HFTLOB_POLICY_CASE(64, 256)   \
    HFTLOB_POLICY_CASE(128, 64)   \
    HFTLOB_POLICY_CASE(128, 128)  \
    HFTLOB_POLICY_CASE(128, 256)  \
    HFTLOB_POLICY_CASE(256, 64)   \
    HFTLOB_POLICY_CASE(256, 128)  \
    HFTLOB_POLICY_CASE(256, 256)

// The text in front of a check's message: the operator, and for a grouped call the group (else -1)
struct Who {
    const char* op;
    int group;
};

int fail_at(Who who, int code, const char* text) {
    char msg[200];
    if (who.group < 0) snprintf(msg, sizeof msg, "%s: %s", who.op, text);
    else snprintf(msg, sizeof msg, "%s: group %d: %s", who.op, who.group, text);
    return hftlob_fail(code, msg);
}

// Every operator's checks of one batch, and its heads.  The checks run in the order they always have:
// the sizes, then head_check (the operator's own check of K and nv, which are read only after it
// passes), then the mode, the pointers and the alignment
template <class HeadCheck>
int policy_check(Who who, int B, int D, int FC, int H, int K, const int* nv, HeadCheck head_check,
                 const hftlob_policy_weights* w, const float* obs, const uint8_t* done, const float* h_in,
                 const float* h_out, int mode, const uint32_t* key, const int32_t* action, const float* log_prob,
                 const float* value, Heads* hd) {
    if (B < 1) return fail_at(who, HFTLOB_ESHAPE, "B must be >= 1");
    if (!size_ok(H)) return fail_at(who, HFTLOB_ESHAPE, "H must be 64, 128 or 256");
    if (!size_ok(FC)) return fail_at(who, HFTLOB_ESHAPE, "FC must be 64, 128 or 256");
    if (D < 1 || D > DMAX) return fail_at(who, HFTLOB_ESHAPE, "D must be in 1..64");
    if (int rc = head_check()) return rc;
    if (mode != 0 && mode != 1) return fail_at(who, HFTLOB_EINVAL, "mode must be 0 (sample) or 1 (argmax)");
    if (!w) return fail_at(who, HFTLOB_ENULL, "w (the weight struct) is NULL");
    if (!w->w_embed || !w->b_embed || !w->w_ih || !w->b_ih || !w->w_hh || !w->b_hh || !w->w_c1 || !w->b_c1 ||
        !w->w_c2 || !w->b_c2 || !w->w_a1 || !w->b_a1 || !w->w_a2 || !w->b_a2)
        return fail_at(who, HFTLOB_ENULL, "a pointer of the weight struct w is NULL");
    if (!obs) return fail_at(who, HFTLOB_ENULL, "obs is NULL");
    if (!done) return fail_at(who, HFTLOB_ENULL, "done is NULL");
    if (!h_in) return fail_at(who, HFTLOB_ENULL, "h_in is NULL");
    if (!h_out) return fail_at(who, HFTLOB_ENULL, "h_out is NULL");
    if (mode == 0 && !key) return fail_at(who, HFTLOB_ENULL, "key is NULL (mode 0 samples from it)");
    if (!action) return fail_at(who, HFTLOB_ENULL, "action is NULL");
    if (!log_prob) return fail_at(who, HFTLOB_ENULL, "log_prob is NULL");
    if (!value) return fail_at(who, HFTLOB_ENULL, "value is NULL");
    if (misaligned(w->w_ih) || misaligned(w->w_hh) || misaligned(w->w_c1) || misaligned(w->w_a1) || misaligned(w->w_a2))
        return fail_at(who, HFTLOB_EINVAL, "w_ih, w_hh, w_c1, w_a1 and w_a2 must be 16-byte aligned");
    hd->K = K;
    hd->S = 0;
    for (int k = 0; k < K; ++k) {
        hd->nv[k] = nv[k];
        hd->off[k] = hd->S;
        hd->S += nv[k];
    }
    for (int k = K; k < MAXK; ++k) {  // the entries past K repeat head K - 1
        hd->nv[k] = hd->nv[K - 1];
        hd->off[k] = hd->off[K - 1];
    }
    return HFTLOB_OK;
}

// The launch of a checked table, with NHD logits blocks
template <int NHD, int MG>
int table_launch(int FC, int H, const GroupTable<MG>& tb, int mode, void* stream) {
    const dim3 grid((unsigned)tb.first[MG]);
    hipStream_t s = (hipStream_t)stream;
#define HFTLOB_POLICY_CASE(h, fc) \
    if (H == h && FC == fc) k_policy_step<h, fc, NHD, MG><<<grid, Shape<h, fc>::NT, 0, s>>>(tb, mode);
    HFTLOB_POLICY_CASES
#undef HFTLOB_POLICY_CASE
    return launch_status();
}

// The two single-batch operators' checks and launch, with NHD logits blocks
template <int NHD, class HeadCheck>
int policy_launch(int B, int D, int FC, int H, int K, const int* nv, HeadCheck head_check,
                  const hftlob_policy_weights* w, const float* obs, const uint8_t* done, const float* h_in, float* h_out,
                  int mode, const uint32_t* key, int32_t* action, float* log_prob, float* value, float* logits,
                  void* stream) {
    static_assert(NHD <= MAXK, "Heads holds MAXK entries");
    Heads hd;
    if (const int rc = policy_check(Who{"policy_step", -1}, B, D, FC, H, K, nv, head_check, w, obs, done, h_in, h_out,
                                    mode, key, action, log_prob, value, &hd))
        return rc;
    const GroupTable<1> tb{{Group{B, D, hd, *w, obs, done, h_in, h_out, key, action, log_prob, value, logits}},
                           {0, (B + TILE - 1) / TILE}};
    return table_launch<NHD>(FC, H, tb, mode, stream);
}

}  // namespace

extern "C" int hftlob_policy_step(int B, int D, int FC, int H, int A, const hftlob_policy_weights* w, const float* obs,
                                  const uint8_t* done, const float* h_in, float* h_out, int mode, const uint32_t* key,
                                  int32_t* action, float* log_prob, float* value, float* logits, void* stream) {
    const auto head_check = [&] {
        return A < 1 || A > 16 ? hftlob_fail(HFTLOB_ESHAPE, "policy_step: A must be in 1..16") : HFTLOB_OK;
    };
    return policy_launch<1>(B, D, FC, H, 1, &A, head_check, w, obs, done, h_in, h_out, mode, key, action, log_prob, value,
                            logits, stream);
}

extern "C" int hftlob_policy_step_multi(int B, int D, int FC, int H, int K, const int* nvec,
                                        const hftlob_policy_weights* w, const float* obs, const uint8_t* done,
                                        const float* h_in, float* h_out, int mode, const uint32_t* keys, int32_t* action,
                                        float* log_prob, float* value, float* logits, void* stream) {
    const auto head_check = [&] {
        if (K < 1 || K > MAXK) return hftlob_fail(HFTLOB_ESHAPE, "policy_step_multi: K must be in 1..4");
        if (!nvec) return hftlob_fail(HFTLOB_ENULL, "policy_step_multi: nvec is NULL");
        for (int k = 0; k < K; ++k)
            if (nvec[k] < 1 || nvec[k] > 16)
                return hftlob_fail(HFTLOB_ESHAPE, "policy_step_multi: every nvec entry must be in 1..16");
        return (int)HFTLOB_OK;
    };
    return policy_launch<MAXK>(B, D, FC, H, K, nvec, head_check, w, obs, done, h_in, h_out, mode, keys, action, log_prob,
                               value, logits, stream);
}

extern "C" int hftlob_policy_step_grouped(int FC, int H, int n_groups, const hftlob_policy_group* groups, int mode,
                                          void* stream) {
    const Who all{"policy_step_grouped", -1};
    if (n_groups < 1 || n_groups > MAXG) return fail_at(all, HFTLOB_ESHAPE, "n_groups must be in 1..8");
    if (!groups) return fail_at(all, HFTLOB_ENULL, "groups is NULL");
    if (!size_ok(H)) return fail_at(all, HFTLOB_ESHAPE, "H must be 64, 128 or 256");
    if (!size_ok(FC)) return fail_at(all, HFTLOB_ESHAPE, "FC must be 64, 128 or 256");
    GroupTable<MAXG> tb;
    long long tiles = 0;
    bool one_head = true;
    for (int g = 0; g < n_groups; ++g) {
        const hftlob_policy_group& x = groups[g];
        const Who who{"policy_step_grouped", g};
        const auto head_check = [&] {
            if (x.K < 1 || x.K > MAXK) return fail_at(who, HFTLOB_ESHAPE, "K must be in 1..4");
            for (int k = 0; k < x.K; ++k)
                if (x.nvec[k] < 1 || x.nvec[k] > 16) return fail_at(who, HFTLOB_ESHAPE, "every nvec entry must be in 1..16");
            return (int)HFTLOB_OK;
        };
        Group& t = tb.g[g];
        if (const int rc = policy_check(who, x.B, x.D, FC, H, x.K, x.nvec, head_check, &x.w, x.obs, x.done, x.h_in,
                                        x.h_out, mode, x.keys, x.action, x.log_prob, x.value, &t.hd))
            return rc;
        t.B = x.B;
        t.D = x.D;
        t.W = x.w;
        t.obs = x.obs;
        t.done = x.done;
        t.h_in = x.h_in;
        t.h_out = x.h_out;
        t.key = x.keys;
        t.action = x.action;
        t.log_prob = x.log_prob;
        t.value = x.value;
        t.logits = x.logits;
        tb.first[g] = (int)tiles;
        tiles += (x.B + TILE - 1) / TILE;
        if (tiles > INT32_MAX) return fail_at(all, HFTLOB_ESHAPE, "more than 2^31 - 1 tiles");
        one_head = one_head && x.K == 1;
    }
    for (int g = n_groups; g < MAXG; ++g) {  // the unused entries repeat group 0 and have no tiles
        tb.g[g] = tb.g[0];
        tb.first[g] = (int)tiles;
    }
    tb.first[MAXG] = (int)tiles;
    // one head everywhere: the single operator's one logits block, else the multi-head operator's MAXK
    return one_head ? table_launch<1>(FC, H, tb, mode, stream) : table_launch<MAXK>(FC, H, tb, mode, stream);
}
