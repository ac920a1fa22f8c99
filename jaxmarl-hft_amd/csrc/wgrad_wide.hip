// The weight and bias gradients of the IPPO net's wide layers as an engine operator (include/hftlob.h:
// hftlob_xty_wide), gfx950, float32:  C[P][Q] = sum_n A[n][p] B[n][q] and optionally the column sums of A,
// for P a multiple of 64 up to 768 and Q in {64, 128, 256} over N rows (65 536 in the metric config's
// minibatch).  A comes as one or two strided column blocks, B optionally shifted by `shift` rows behind a
// head and masked by row (the h_prev of the GRU's W_hh gradient without its cat and where).
// hftlob/train/wgrad.py restates it in torch (xty_wide_reference).
//
// The output is at most 768 KB and the reduction runs over all the rows, so the rows are split: two
// launches, no floating-point atomic, every sum combined in a fixed order.
//   k_xtyw_partial  one workgroup of four waves per (stripe, tile of C); the stripe rule of the header is a
//             function of (N, P, Q).  A tile is 128 rows of C by TQ = 64 MQ columns (MQ = 1 for Q = 64, else
//             2); wave w owns its quarter, 64 x 32 MQ, as 2 x MQ accumulators of
//             __builtin_amdgcn_mfma_f32_32x32x2f32 that stay in registers for the whole stripe.  The stripe
//             is walked in chunks of 32 rows through LDS: the chunk of A laid out [k][p] (128 floats a row),
//             the chunk of B [k][q], so that an MFMA operand is one ds_read_b32 per lane, lane l reading
//             element l & 31 of row l >> 5: 32 consecutive dwords per lane group, conflict-free.  The next
//             chunk's global loads (float4 along p and q, with the shift, the head and the row mask applied
//             to B's addresses and values) are issued before the current chunk is multiplied and land in
//             LDS after it.  Rows past the stripe's end and columns past P enter LDS as zeros.  The
//             workgroups of q-tile 0 also add their 128 columns of A, a chunk row at a time, from LDS.
//             The workgroup writes its tile of the stripe's partial [P][Q], and those sums, to the workspace.
//   k_xtyw_final    a lane per output element: adds the G partials in double, in stripe order, rounds once.
//
// The MFMA is bit for bit a k-ordered fmaf chain, so a partial is the float32 fmaf chain over the stripe's
// rows in row order, whatever the tile.  Workgroup v of the grid is (stripe v / tiles, tile v % tiles); the
// hardware deals consecutive workgroup ids round-robin to the 8 XCDs, so the id is first mapped to v such
// that an XCD's ids are consecutive v: the tiles of a stripe, which read the same rows, share one L2.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/hftlob.h"
#include "hftlob_internal.h"

#pragma clang fp contract(off)

namespace {

constexpr int NT = 256;                              // lanes per workgroup: 2 x 2 waves over the tile
constexpr int TP = HFTLOB_XTY_WIDE_TILE_P;           // rows of C in a tile
constexpr int KC = HFTLOB_XTY_WIDE_CHUNK;            // rows of A and B in an LDS chunk
constexpr int XCDS = 8;
static_assert(TP == 128 && KC == 32 && NT == 256, "the load and wave maps below");

typedef float f32x16 __attribute__((ext_vector_type(16)));

struct WideArgs {
    long long N, rows, shift;            // rows: of a stripe
    int P, Q, tiles_p, tiles_q;
    const float* a[2];                   // A's column blocks
    int cols0;                           // the columns of block 0 (block 1 has the rest of P)
    long long stride[2];
    const float* B;
    const float* head;
    const unsigned char* zero_row;
    int want_a;
    float* ws;
};

int tile_q(int Q) { return Q == 64 ? 64 : 128; }
int tiles_of(int P, int Q) { return ((P + TP - 1) / TP) * (Q / tile_q(Q)); }

// the stripe rule of the header: the rows of a stripe, from (N, P, Q)
long long stripe_rows(long long N, int P, int Q) {
    const int tiles = tiles_of(P, Q);
    const long long M = (HFTLOB_XTY_WIDE_TARGET_WGS + tiles - 1) / tiles;
    const long long R = HFTLOB_XTY_WIDE_STRIPE_ROWS;
    return (N + R - 1) / R <= M ? R : (N + M - 1) / M;
}

int stripes(long long N, int P, int Q) {
    if (N <= 0) return 0;
    const long long r = stripe_rows(N, P, Q);
    return (int)((N + r - 1) / r);
}

template <int MQ>
__global__ __launch_bounds__(NT, 2) void k_xtyw_partial(const WideArgs g) {
    constexpr int TQ = 64 * MQ;
    constexpr int AV = KC * TP / 4 / NT;             // float4 of A a lane loads per chunk: 4
    constexpr int BV = KC * TQ / 4 / NT;             // of B: 2 MQ
    constexpr int BL = TQ / 4;                       // lanes across a row of B's chunk
    constexpr int BR = NT / BL;                      // rows of B's chunk per pass
    __shared__ float sA[KC * TP];
    __shared__ float sB[KC * TQ];
    const int tid = threadIdx.x, lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);

    // the workgroup's stripe and tile
    const int nwg = gridDim.x, id = blockIdx.x;
    const int x = id % XCDS, per = nwg / XCDS, rem = nwg % XCDS;
    const int v = x * per + (x < rem ? x : rem) + id / XCDS;
    const int tiles = g.tiles_p * g.tiles_q;
    const int s = v / tiles, t = v - s * tiles;
    const int tp = t / g.tiles_q, tq = t - tp * g.tiles_q;
    const int p0 = tp * TP, q0 = tq * TQ;
    const long long begin = (long long)s * g.rows;
    const long long end = begin + g.rows < g.N ? begin + g.rows : g.N;

    // this lane's float4 of a chunk row of A: 64 columns of one block, or past P (the half tile): none
    const int ac = (tid & 31) * 4, ar = tid >> 5;
    const float* my_a = nullptr;
    long long my_stride = 0;
    {
        const int col = p0 + ac;
        if (col < g.P) {
            const bool first = col < g.cols0;
            my_a = first ? g.a[0] + col : g.a[1] + (col - g.cols0);
            my_stride = first ? g.stride[0] : g.stride[1];
        }
    }
    const int bc = (tid % BL) * 4, br = tid / BL;
    const float4 zero4 = make_float4(0.0f, 0.0f, 0.0f, 0.0f);

    float4 ra[AV], rb[BV];
    unsigned zb[BV];
#pragma unroll
    for (int i = 0; i < AV; ++i) ra[i] = zero4;
#pragma unroll
    for (int i = 0; i < BV; ++i) rb[i] = zero4, zb[i] = 0u;
    auto load_chunk = [&](long long base) {
#pragma unroll
        for (int i = 0; i < AV; ++i) {
            const long long n = base + ar + (NT / 32) * i;
            ra[i] = zero4;
            if (my_a && n < end) ra[i] = *reinterpret_cast<const float4*>(my_a + n * my_stride);
        }
#pragma unroll
        for (int i = 0; i < BV; ++i) {
            const long long n = base + br + BR * i;
            const float* src = nullptr;
            if (n < end) {
                if (n >= g.shift) src = g.B + (n - g.shift) * g.Q;
                else if (g.head) src = g.head + n * g.Q;
            }
            rb[i] = zero4;
            if (src) rb[i] = *reinterpret_cast<const float4*>(src + q0 + bc);
            zb[i] = g.zero_row && n < end ? g.zero_row[n] : 0u;
        }
    };

    // wave w's quarter of the tile, and whether its rows are rows of C
    const int wp = 64 * (w >> 1), wq = 32 * MQ * (w & 1);
    const bool live = p0 + wp < g.P;
    const bool sums = g.want_a && tq == 0 && tid < TP;
    f32x16 acc[2][MQ];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < MQ; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.0f;
    float sa = 0.0f;

    if (begin < end) load_chunk(begin);
    for (long long base = begin; base < end; base += KC) {
        __syncthreads();                             // the last chunk has been read
#pragma unroll
        for (int i = 0; i < AV; ++i)
            *reinterpret_cast<float4*>(&sA[(ar + (NT / 32) * i) * TP + ac]) = ra[i];
#pragma unroll
        for (int i = 0; i < BV; ++i)
        {
            const bool z = zb[i] != 0u;              // (selects, not a product: a masked row may hold NaN)
            *reinterpret_cast<float4*>(&sB[(br + BR * i) * TQ + bc]) =
                make_float4(z ? 0.0f : rb[i].x, z ? 0.0f : rb[i].y, z ? 0.0f : rb[i].z, z ? 0.0f : rb[i].w);
        }
        __syncthreads();
        if (base + KC < end) load_chunk(base + KC);  // in flight while this chunk is multiplied
        if (live) {
            const float* pa = &sA[(lane >> 5) * TP + wp + (lane & 31)];
            const float* pb = &sB[(lane >> 5) * TQ + wq + (lane & 31)];
#pragma unroll
            for (int k = 0; k < KC; k += 2) {
                float a[2], b[MQ];
#pragma unroll
                for (int i = 0; i < 2; ++i) a[i] = pa[k * TP + 32 * i];
#pragma unroll
                for (int j = 0; j < MQ; ++j) b[j] = pb[k * TQ + 32 * j];
#pragma unroll
                for (int i = 0; i < 2; ++i)
#pragma unroll
                    for (int j = 0; j < MQ; ++j)
                        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[i], b[j], acc[i][j], 0, 0, 0);
            }
        }
        if (sums) {
#pragma unroll
            for (int k = 0; k < KC; ++k) sa += sA[k * TP + tid];
        }
    }

    // the stripe's partial: [P][Q] of C, then sum_a
    float* out = g.ws + (long long)s * ((long long)g.P * g.Q + g.P);
    if (live) {
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < MQ; ++j)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int p = p0 + wp + 32 * i + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
                    const int q = q0 + wq + 32 * j + (lane & 31);
                    out[(long long)p * g.Q + q] = acc[i][j][r];
                }
    }
    if (sums && p0 + tid < g.P) out[(long long)g.P * g.Q + p0 + tid] = sa;
}

__global__ __launch_bounds__(NT) void k_xtyw_final(int G, int PQ, int P, const float* __restrict__ ws,
                                                   float* __restrict__ C, float* __restrict__ sum_a) {
    const int e = blockIdx.x * NT + threadIdx.x;     // an element of a partial: [C][sum_a]
    if (e >= PQ + (sum_a ? P : 0)) return;           // (sums nobody asked for were never written)
    const long long stride = (long long)PQ + P;
    const float* src = ws + e;
    double acc = 0.0;
#pragma unroll 8
    for (int s = 0; s < G; ++s) acc += (double)src[s * stride];
    if (e < PQ) C[e] = (float)acc;
    else sum_a[e - PQ] = (float)acc;
}

int shape_error(long long N, int P, int Q) {
    if (P < 64 || P > HFTLOB_XTY_WIDE_MAX_P || P % 64)
        return hftlob_fail(HFTLOB_ESHAPE, "xty_wide: P must be a multiple of 64 in 64..768");
    if (Q != 64 && Q != 128 && Q != 256) return hftlob_fail(HFTLOB_ESHAPE, "xty_wide: Q must be 64, 128 or 256");
    if (N < 0) return hftlob_fail(HFTLOB_ESHAPE, "xty_wide: N must be >= 0");
    return HFTLOB_OK;
}

int hip_error(hipError_t err) {
    return err == hipSuccess ? HFTLOB_OK : hftlob_fail(HFTLOB_ELAUNCH, hipGetErrorString(err));
}

bool misaligned(const void* p) { return ((uintptr_t)p & 15) != 0; }

}  // namespace

extern "C" long long hftlob_xty_wide_workspace(long long N, int P, int Q) {
    const int rc = shape_error(N, P, Q);
    if (rc != HFTLOB_OK) return rc;
    return stripes(N, P, Q) * ((long long)P * Q + P);
}

extern "C" int hftlob_xty_wide(long long N, int Q, const float* A0, int cols0, long long stride0, const float* A1,
                               int cols1, long long stride1, const float* B, const float* head, long long shift,
                               const unsigned char* zero_row, float* C, float* sum_a, float* workspace,
                               void* stream) {
    if (cols0 < 64 || cols0 % 64 || cols1 < 0 || cols1 % 64 || cols0 > HFTLOB_XTY_WIDE_MAX_P ||
        cols1 > HFTLOB_XTY_WIDE_MAX_P)
        return hftlob_fail(HFTLOB_ESHAPE, "xty_wide: a block's columns must be a multiple of 64 (block 1: or 0)");
    const int P = cols0 + cols1;
    const int rc = shape_error(N, P, Q);
    if (rc != HFTLOB_OK) return rc;
    if (shift < 0 || shift > N) return hftlob_fail(HFTLOB_ESHAPE, "xty_wide: shift must be in 0..N");
    if (!C) return hftlob_fail(HFTLOB_ENULL, "xty_wide: C is NULL");
    hipStream_t s = (hipStream_t)stream;
    if (N == 0) {   // empty sums: zeros, and nothing else is read
        hipError_t err = hipMemsetAsync(C, 0, sizeof(float) * P * Q, s);
        if (err == hipSuccess && sum_a) err = hipMemsetAsync(sum_a, 0, sizeof(float) * P, s);
        return hip_error(err);
    }
    if (!A0 || (cols1 && !A1) || (!B && shift < N) || !workspace)   // (with shift = N no row of B is read)
        return hftlob_fail(HFTLOB_ENULL, "xty_wide: a null pointer (A's blocks, B, workspace)");
    if (misaligned(A0) || (cols1 && misaligned(A1)) || misaligned(B) || misaligned(head))
        return hftlob_fail(HFTLOB_EINVAL, "xty_wide: A's blocks, B and head must be 16-byte aligned");
    if (stride0 < cols0 || stride0 % 4 || (cols1 && (stride1 < cols1 || stride1 % 4)))
        return hftlob_fail(HFTLOB_EINVAL, "xty_wide: a block's row stride must be >= its columns and a multiple of 4");
    WideArgs g;
    g.N = N, g.rows = stripe_rows(N, P, Q), g.shift = shift;
    g.P = P, g.Q = Q, g.tiles_p = (P + TP - 1) / TP, g.tiles_q = Q / tile_q(Q);
    g.a[0] = A0, g.a[1] = cols1 ? A1 : A0, g.cols0 = cols0;
    g.stride[0] = stride0, g.stride[1] = cols1 ? stride1 : stride0;
    g.B = B, g.head = head, g.zero_row = zero_row;
    g.want_a = sum_a != nullptr, g.ws = workspace;
    const int G = stripes(N, P, Q);
    const unsigned nwg = (unsigned)G * (unsigned)(g.tiles_p * g.tiles_q);
    if (Q == 64) k_xtyw_partial<1><<<nwg, NT, 0, s>>>(g);
    else k_xtyw_partial<2><<<nwg, NT, 0, s>>>(g);
    const int elems = P * Q + (sum_a ? P : 0);
    k_xtyw_final<<<(unsigned)((elems + NT - 1) / NT), NT, 0, s>>>(G, P * Q, P, workspace, C, sum_a);
    return hip_error(hipGetLastError());
}
