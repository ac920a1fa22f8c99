// Fused GRU sequence scan for the IPPO learner (include/hftlob.h: hftlob_gru_scan_fwd / _bwd), gfx950.
// hftlob_gru_scan_fwd_grouped / _bwd_grouped launch the tiles of several such scans (independent nets
// that share T and H) at once; a tile's work is the same device function either way.
//
// The recurrent part of ScannedRNN (jaxrl/MARL/ippo_rnn_JAXMARL.py) is a dependent chain over
// time whose batch rows are independent, so it is launched the way the env rollout is: once per
// scan, each workgroup owning a tile of 16 batch rows for all T steps.  No workgroup waits on
// another.  The 16 rows are the M side of the f32-input 16x16x4 MFMA, whose result is bit for
// bit a k-ordered fmaf chain (no reduced precision anywhere).
//
//   forward   gh = h_prev . W_hh^T + b_hh, a [16, H] x [H, 3H] product per step.  The tile's h
//             lives in LDS (two buffers, one barrier per step).  A wave owns CB blocks of 16
//             hidden indices j and computes the r, z and n columns of those j, so the gate math
//             runs in registers on the three accumulators of a block.
//   backward  dh_prev = dh . z + d_gh . W_hh, a [16, 3H] x [3H, H] product per step.  The tile's
//             d_gh lives in LDS; a wave owns 64 hidden indices j (four interleaved 16-column
//             blocks, so its loads and stores are float4 along j) and keeps the carry of those
//             j in registers between steps.
//
// W_hh (768 KB at H = 256) does not fit LDS and streams from L2 every step as float4 per lane
// into register buffers, a chunk or more of MFMAs ahead of its use.  The prefetch has no branch
// and wraps into the next step (W_hh is the same every step).  The k order inside a chunk is
// permuted so that both operands are 16-byte reads (forward: chunks of 32 k, lane quarter q has
// k = 32 c + 8 q + 0..7; backward: chunks of 16 k, k = 16 c + 4 q + 0..3); A and B use the same
// k, and a sum does not depend on the permutation beyond its rounding order.
// What bounds the forward is that load path, not the MFMAs: a lane's B
// operand is a row of W_hh, so every quarter-wave of a load touches 16 rows.
#include <stdint.h>

#include "hftlob_tile.h"  // f32x4, ld4 / st4 / splat, TILE and the MFMA operand maps

namespace {

// The forward scan of one tile: rows b0 .. b0 + 15 of a [T, B] sequence batch, all T steps.  The body of
// both entry points (one batch, and the grouped launch whose workgroup has looked up its group first).
template <int H, int CB>
__device__ __forceinline__ void gru_fwd_tile(
    int T, int B, int b0, const float* __restrict__ gi, const float* __restrict__ h0,
    const uint8_t* __restrict__ done, const float* __restrict__ w_hh, const float* __restrict__ b_hh,
    float* __restrict__ hseq, float* __restrict__ gates) {
    constexpr int NW = H / 16 / CB, NT = 64 * NW, S = H + 4, NCH = H / 32, PF = 2;  // chunks of 32 k
    static_assert(NCH % PF == 0 && (NCH & (NCH - 1)) == 0, "the k loop is unrolled by PF chunks and wraps by a mask");
    __shared__ __attribute__((aligned(16))) float hbuf[2][TILE * S];  // h_prev(t) of the tile, by t & 1
    const int tid = threadIdx.x, w = tid >> 6, l = tid & 63, li = l & 15, q = l >> 4;

    for (int i = tid; i < TILE * H; i += NT) {  // h_prev(0) = done[0] ? 0 : h0; rows past B are zero
        const int row = i / H, j = i % H, b = b0 + row;
        hbuf[0][row * S + j] = (b < B && !done[b]) ? h0[(size_t)b * H + j] : 0.0f;
    }
    int col[CB];
    float bias[CB][3];
    const float* wp[CB][3];  // the lane's B operand: W_hh[g H + col][8 q + ...]
#pragma unroll
    for (int c = 0; c < CB; ++c) {
        col[c] = (w * CB + c) * 16 + li;
#pragma unroll
        for (int g = 0; g < 3; ++g) {
            bias[c][g] = b_hh[g * H + col[c]];
            wp[c][g] = w_hh + (size_t)(g * H + col[c]) * H + 8 * q;
        }
    }
    int bc[4];  // the lane's rows 4 q + i, clamped into the batch for loads
#pragma unroll
    for (int i = 0; i < 4; ++i) bc[i] = min(b0 + 4 * q + i, B - 1);
    // W_hh chunks in flight, by chunk mod PF.  The prefetch is unconditional and wraps around: the
    // last chunks of a step fetch the first chunks of the next one (W_hh is the same every step),
    // and no branch sits between a load and its wait
    f32x4 wv[PF][CB][3][2];
#pragma unroll
    for (int p = 0; p < PF; ++p)
#pragma unroll
        for (int c = 0; c < CB; ++c)
#pragma unroll
            for (int g = 0; g < 3; ++g) {
                wv[p][c][g][0] = ld4(wp[c][g] + 32 * p);
                wv[p][c][g][1] = ld4(wp[c][g] + 32 * p + 4);
            }
    __syncthreads();

    for (int t = 0; t < T; ++t) {
        const float* hc = hbuf[t & 1];
        float* hn = hbuf[(t & 1) ^ 1];
        // this step's gi and the next step's done of the lane's four rows, in flight under the k loop:
        // unconditional loads at clamped indices (a row past B reads row B - 1 and is never stored)
        float gv[CB][3][4];
        uint8_t dnext[4];
        const int tn = t + 1 < T ? t + 1 : t;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            dnext[i] = done[(size_t)tn * B + bc[i]];
#pragma unroll
            for (int c = 0; c < CB; ++c)
#pragma unroll
                for (int g = 0; g < 3; ++g) gv[c][g][i] = gi[((size_t)t * B + bc[i]) * (3 * H) + g * H + col[c]];
        }
        f32x4 acc[CB][3];
#pragma unroll
        for (int c = 0; c < CB; ++c)
#pragma unroll
            for (int g = 0; g < 3; ++g) acc[c][g] = splat(bias[c][g]);
#pragma unroll 1
        for (int ch = 0; ch < NCH; ch += PF) {
#pragma unroll
            for (int p = 0; p < PF; ++p) {
                const float* ap = hc + li * S + 32 * (ch + p) + 8 * q;
                const f32x4 a[2] = {ld4(ap), ld4(ap + 4)};
#pragma unroll
                for (int s = 0; s < 8; ++s)
#pragma unroll
                    for (int c = 0; c < CB; ++c)
#pragma unroll
                        for (int g = 0; g < 3; ++g)
                            acc[c][g] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[s >> 2][s & 3], wv[p][c][g][s >> 2][s & 3],
                                                                             acc[c][g], 0, 0, 0);
                const int nx = (ch + p + PF) & (NCH - 1);
#pragma unroll
                for (int c = 0; c < CB; ++c)
#pragma unroll
                    for (int g = 0; g < 3; ++g) {
                        wv[p][c][g][0] = ld4(wp[c][g] + 32 * nx);
                        wv[p][c][g][1] = ld4(wp[c][g] + 32 * nx + 4);
                    }
                __builtin_amdgcn_sched_barrier(0);  // the loads stay here: a chunk of MFMAs between issue and use
            }
        }
#pragma unroll
        for (int c = 0; c < CB; ++c)
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int row = 4 * q + i;
                const float hp = hc[row * S + col[c]];
                const float r = sigmoidf_(gv[c][0][i] + acc[c][0][i]);
                const float z = sigmoidf_(gv[c][1][i] + acc[c][1][i]);
                const float ghn = acc[c][2][i];
                const float n = tanhf(gv[c][2][i] + r * ghn);
                const float h = (1.0f - z) * n + z * hp;
                if (b0 + row < B) {
                    const size_t tb = (size_t)t * B + (b0 + row);
                    hseq[tb * H + col[c]] = h;
                    if (gates) {
                        float* gp = gates + tb * (4 * H) + col[c];
                        gp[0] = r;
                        gp[H] = z;
                        gp[2 * H] = n;
                        gp[3 * H] = ghn;
                    }
                }
                hn[row * S + col[c]] = dnext[i] ? 0.0f : h;  // h_prev(t + 1) (after the last step: unused)
            }
        __syncthreads();  // hn complete; every read of hc (the buffer step t + 1 writes) is behind us
    }
}

// The backward scan of one tile, as gru_fwd_tile is the forward's
template <int H>
__device__ __forceinline__ void gru_bwd_tile(
    int T, int B, int b0, const float* __restrict__ d_hseq, const float* __restrict__ hseq,
    const float* __restrict__ gates, const float* __restrict__ h0, const uint8_t* __restrict__ done,
    const float* __restrict__ w_hh, float* __restrict__ d_gi, float* __restrict__ d_gh_n,
    float* __restrict__ d_h0) {
    constexpr int K = 3 * H, S = K + 4, NCH = K / 16, PF = 4;
    static_assert(NCH % PF == 0, "the k loop is unrolled by PF chunks");
    __shared__ __attribute__((aligned(16))) float dgh[TILE * S];  // d_gh[t] of the tile: (dr, dz, dn r)
    const int tid = threadIdx.x, w = tid >> 6, l = tid & 63, li = l & 15, q = l >> 4;
    const int j0 = w * 64 + 4 * li;  // the lane's hidden indices j0 .. j0 + 3: column li of blocks 0 .. 3
    const float* wp = w_hh + (size_t)(4 * q) * H + j0;  // the lane's B operand: W_hh[4 q + ...][j0 ..]

    int bc[4];  // the lane's rows 4 q + i, clamped into the batch for loads
#pragma unroll
    for (int i = 0; i < 4; ++i) bc[i] = min(b0 + 4 * q + i, B - 1);
    f32x4 carry[4];  // by row 4 q + i, over j0 .. j0 + 3
#pragma unroll
    for (int i = 0; i < 4; ++i) carry[i] = splat(0.0f);

    // W_hh chunks in flight, by chunk mod PF and MFMA s of the chunk (k = 16 chunk + 4 q + s), over
    // j0 .. j0 + 3; prefetched without a branch and wrapping into the next step, as in the forward
    f32x4 wv[PF][4];
#pragma unroll
    for (int p = 0; p < PF; ++p)
#pragma unroll
        for (int s = 0; s < 4; ++s) wv[p][s] = ld4(wp + (size_t)(16 * p + s) * H);

    for (int t = T - 1; t >= 0; --t) {
        // the step's inputs: unconditional loads at clamped rows (a row past B repeats row B - 1: its
        // d_gh row feeds only its own carry, and nothing of it is stored)
        f32x4 dhz[4];
        uint8_t dn_[4];
        const float* hprev = t ? hseq + (size_t)(t - 1) * B * H : h0;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int row = 4 * q + i;
            const size_t tb = (size_t)t * B + bc[i];
            dn_[i] = done[tb];
            const f32x4 dh = ld4(d_hseq + tb * H + j0) + carry[i];
            const float* gp = gates + tb * (4 * H) + j0;
            const f32x4 r = ld4(gp), z = ld4(gp + H), n = ld4(gp + 2 * H), ghn = ld4(gp + 3 * H);
            const f32x4 hpv = ld4(hprev + (size_t)bc[i] * H + j0);
            const f32x4 hp = dn_[i] ? splat(0.0f) : hpv;
            const f32x4 dn = dh * (1.0f - z) * (1.0f - n * n);
            const f32x4 dz = dh * (hp - n) * z * (1.0f - z);
            const f32x4 dr = dn * ghn * r * (1.0f - r);
            const f32x4 dghn = dn * r;
            dhz[i] = dh * z;
            if (b0 + row < B) {
                float* op = d_gi + tb * (3 * H) + j0;
                st4(op, dr);
                st4(op + H, dz);
                st4(op + 2 * H, dn);
                st4(d_gh_n + tb * H + j0, dghn);
            }
            st4(dgh + row * S + j0, dr);
            st4(dgh + row * S + H + j0, dz);
            st4(dgh + row * S + 2 * H + j0, dghn);
        }
        __syncthreads();
        f32x4 acc[4];  // by column block c (hidden index j0 + c), over rows 4 q + i
#pragma unroll
        for (int c = 0; c < 4; ++c) acc[c] = splat(0.0f);
#pragma unroll 1
        for (int ch = 0; ch < NCH; ch += PF) {
#pragma unroll
            for (int p = 0; p < PF; ++p) {
                const f32x4 a = ld4(dgh + li * S + 16 * (ch + p) + 4 * q);
#pragma unroll
                for (int s = 0; s < 4; ++s)
#pragma unroll
                    for (int c = 0; c < 4; ++c)
                        acc[c] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[s], wv[p][s][c], acc[c], 0, 0, 0);
                const int nx = ch + p + PF < NCH ? ch + p + PF : ch + p + PF - NCH;
#pragma unroll
                for (int s = 0; s < 4; ++s) wv[p][s] = ld4(wp + (size_t)(16 * nx + s) * H);
                __builtin_amdgcn_sched_barrier(0);  // the loads stay here: PF - 1 chunks of MFMAs between issue and use
            }
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const f32x4 mm = {acc[0][i], acc[1][i], acc[2][i], acc[3][i]};
            carry[i] = dn_[i] ? splat(0.0f) : dhz[i] + mm;
        }
        __syncthreads();  // every read of dgh is behind us before step t - 1 rewrites it
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int b = b0 + 4 * q + i;
        if (b < B) st4(d_h0 + (size_t)b * H + j0, carry[i]);
    }
}

template <int H, int CB>
__global__ __launch_bounds__(64 * (H / 16 / CB)) void k_gru_scan_fwd(
    int T, int B, const float* __restrict__ gi, const float* __restrict__ h0, const uint8_t* __restrict__ done,
    const float* __restrict__ w_hh, const float* __restrict__ b_hh, float* __restrict__ hseq,
    float* __restrict__ gates) {
    gru_fwd_tile<H, CB>(T, B, blockIdx.x * TILE, gi, h0, done, w_hh, b_hh, hseq, gates);
}

template <int H>
__global__ __launch_bounds__(64 * (H / 64)) void k_gru_scan_bwd(
    int T, int B, const float* __restrict__ d_hseq, const float* __restrict__ hseq,
    const float* __restrict__ gates, const float* __restrict__ h0, const uint8_t* __restrict__ done,
    const float* __restrict__ w_hh, float* __restrict__ d_gi, float* __restrict__ d_gh_n,
    float* __restrict__ d_h0) {
    gru_bwd_tile<H>(T, B, blockIdx.x * TILE, d_hseq, hseq, gates, h0, done, w_hh, d_gi, d_gh_n, d_h0);
}

// The grouped launches (hftlob_gru_scan_fwd_grouped / _bwd_grouped): the groups by value in the kernel
// arguments, as optim_step.hip's tensor table travels, so that the call needs no copy to the device and
// can be captured in a graph.  first[g] is group g's first tile, first[MAXG] the grid; the unused entries
// repeat group 0 and have no tiles.  A workgroup finds its group from blockIdx once, before the t loop:
// the index is wave-uniform, so the group's B and pointers are scalar loads from the kernarg segment
// and live in SGPRs as the arguments of the single-batch kernels do.
constexpr int MAXG = HFTLOB_GRU_MAX_GROUPS;

template <class G>
struct GroupTable {
    G g[MAXG];
    int first[MAXG + 1];
};

template <class G>
__device__ __forceinline__ int find_group(const GroupTable<G>& tb, int tile) {
    int g = 0;
    while (tile >= tb.first[g + 1]) ++g;  // (the grid is first[MAXG] workgroups: g stays below MAXG)
    return g;
}

template <int H, int CB>
__global__ __launch_bounds__(64 * (H / 16 / CB)) void k_gru_scan_fwd_grouped(
    int T, const GroupTable<hftlob_gru_fwd_group> tb) {
    const int g = find_group(tb, blockIdx.x);
    const hftlob_gru_fwd_group& x = tb.g[g];
    gru_fwd_tile<H, CB>(T, x.B, (blockIdx.x - tb.first[g]) * TILE, x.gi, x.h0, x.done, x.w_hh, x.b_hh, x.hseq,
                        x.gates);
}

template <int H>
__global__ __launch_bounds__(64 * (H / 64)) void k_gru_scan_bwd_grouped(
    int T, const GroupTable<hftlob_gru_bwd_group> tb) {
    const int g = find_group(tb, blockIdx.x);
    const hftlob_gru_bwd_group& x = tb.g[g];
    gru_bwd_tile<H>(T, x.B, (blockIdx.x - tb.first[g]) * TILE, x.d_hseq, x.hseq, x.gates, x.h0, x.done, x.w_hh,
                    x.d_gi, x.d_gh_n, x.d_h0);
}

int check_TH(int T, int H) {
    if (T < 1) return hftlob_fail(HFTLOB_ESHAPE, "gru_scan: T and B must be >= 1");
    if (H != 64 && H != 128 && H != 256) return hftlob_fail(HFTLOB_ESHAPE, "gru_scan: H must be 64, 128 or 256");
    return HFTLOB_OK;
}

int check_shape(int T, int B, int H) {
    if (T < 1 || B < 1) return hftlob_fail(HFTLOB_ESHAPE, "gru_scan: T and B must be >= 1");
    return check_TH(T, H);
}

bool has_null(const hftlob_gru_fwd_group& x) {  // (gates may be NULL)
    return !x.gi || !x.h0 || !x.done || !x.w_hh || !x.b_hh || !x.hseq;
}

bool has_null(const hftlob_gru_bwd_group& x) {
    return !x.d_hseq || !x.hseq || !x.gates || !x.h0 || !x.done || !x.w_hh || !x.d_gi || !x.d_gh_n || !x.d_h0;
}

// the checks of a grouped call and its table; *grid receives the number of tiles
template <class G>
int make_table(int T, int H, int n_groups, const G* groups, GroupTable<G>* tb, unsigned* grid) {
    if (n_groups < 1 || n_groups > MAXG) return hftlob_fail(HFTLOB_ESHAPE, "gru_scan grouped: n_groups must be in 1..8");
    if (const int rc = check_TH(T, H)) return rc;
    if (!groups) return hftlob_fail(HFTLOB_ENULL, "gru_scan grouped: groups is NULL");
    long long tiles = 0;
    for (int g = 0; g < MAXG; ++g) {
        tb->first[g] = (int)tiles;
        if (g >= n_groups) {
            tb->g[g] = groups[0];
            continue;
        }
        const G& x = groups[g];
        if (x.B < 1) return hftlob_fail(HFTLOB_ESHAPE, "gru_scan grouped: a group's B must be >= 1");
        if (has_null(x)) return hftlob_fail(HFTLOB_ENULL, "gru_scan grouped: null array in a group");
        tb->g[g] = x;
        tiles += (x.B + TILE - 1) / TILE;
        if (tiles > INT32_MAX) return hftlob_fail(HFTLOB_ESHAPE, "gru_scan grouped: more than 2^31 - 1 tiles");
    }
    tb->first[MAXG] = (int)tiles;
    *grid = (unsigned)tiles;
    return HFTLOB_OK;
}

}  // namespace

extern "C" {

int hftlob_gru_scan_fwd(int T, int B, int H, const float* gi, const float* h0, const uint8_t* done, const float* w_hh,
                        const float* b_hh, float* hseq, float* gates, void* stream) {
    if (const int rc = check_shape(T, B, H)) return rc;
    if (!gi || !h0 || !done || !w_hh || !b_hh || !hseq) return hftlob_fail(HFTLOB_ENULL, "gru_scan_fwd: null array");
    const dim3 grid((unsigned)((B + TILE - 1) / TILE));
    hipStream_t s = (hipStream_t)stream;
    if (H == 64) k_gru_scan_fwd<64, 1><<<grid, 256, 0, s>>>(T, B, gi, h0, done, w_hh, b_hh, hseq, gates);
    else if (H == 128) k_gru_scan_fwd<128, 1><<<grid, 512, 0, s>>>(T, B, gi, h0, done, w_hh, b_hh, hseq, gates);
    else k_gru_scan_fwd<256, 2><<<grid, 512, 0, s>>>(T, B, gi, h0, done, w_hh, b_hh, hseq, gates);
    return launch_status();
}

int hftlob_gru_scan_bwd(int T, int B, int H, const float* d_hseq, const float* hseq, const float* gates,
                        const float* h0, const uint8_t* done, const float* w_hh, float* d_gi, float* d_gh_n,
                        float* d_h0, void* stream) {
    if (const int rc = check_shape(T, B, H)) return rc;
    if (!d_hseq || !hseq || !gates || !h0 || !done || !w_hh || !d_gi || !d_gh_n || !d_h0)
        return hftlob_fail(HFTLOB_ENULL, "gru_scan_bwd: null array");
    const dim3 grid((unsigned)((B + TILE - 1) / TILE));
    hipStream_t s = (hipStream_t)stream;
    if (H == 64) k_gru_scan_bwd<64><<<grid, 64, 0, s>>>(T, B, d_hseq, hseq, gates, h0, done, w_hh, d_gi, d_gh_n, d_h0);
    else if (H == 128) k_gru_scan_bwd<128><<<grid, 128, 0, s>>>(T, B, d_hseq, hseq, gates, h0, done, w_hh, d_gi, d_gh_n, d_h0);
    else k_gru_scan_bwd<256><<<grid, 256, 0, s>>>(T, B, d_hseq, hseq, gates, h0, done, w_hh, d_gi, d_gh_n, d_h0);
    return launch_status();
}

int hftlob_gru_scan_fwd_grouped(int T, int H, int n_groups, const hftlob_gru_fwd_group* groups, void* stream) {
    GroupTable<hftlob_gru_fwd_group> tb;
    unsigned tiles = 0;
    if (const int rc = make_table(T, H, n_groups, groups, &tb, &tiles)) return rc;
    const dim3 grid(tiles);
    hipStream_t s = (hipStream_t)stream;
    if (H == 64) k_gru_scan_fwd_grouped<64, 1><<<grid, 256, 0, s>>>(T, tb);
    else if (H == 128) k_gru_scan_fwd_grouped<128, 1><<<grid, 512, 0, s>>>(T, tb);
    else k_gru_scan_fwd_grouped<256, 2><<<grid, 512, 0, s>>>(T, tb);
    return launch_status();
}

int hftlob_gru_scan_bwd_grouped(int T, int H, int n_groups, const hftlob_gru_bwd_group* groups, void* stream) {
    GroupTable<hftlob_gru_bwd_group> tb;
    unsigned tiles = 0;
    if (const int rc = make_table(T, H, n_groups, groups, &tb, &tiles)) return rc;
    const dim3 grid(tiles);
    hipStream_t s = (hipStream_t)stream;
    if (H == 64) k_gru_scan_bwd_grouped<64><<<grid, 64, 0, s>>>(T, tb);
    else if (H == 128) k_gru_scan_bwd_grouped<128><<<grid, 128, 0, s>>>(T, tb);
    else k_gru_scan_bwd_grouped<256><<<grid, 256, 0, s>>>(T, tb);
    return launch_status();
}

}  // extern "C"
