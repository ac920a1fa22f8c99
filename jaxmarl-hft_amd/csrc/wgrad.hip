// The weight and bias gradients of the IPPO net's narrow layers as an engine operator (include/hftlob.h:
// hftlob_xty), gfx950, float32:  C[P][Q] = sum_n A[n][p] B[n][q], and optionally the column sums of A and
// of B, for 1 <= P <= 64 and Q in {64, 128, 256} over N rows (65 536 in the metric config's minibatch).
// hftlob/train/wgrad.py restates it in torch (xty_reference).
//
// The output is a few KB and the reduction runs over all the rows, so the rows are split: two launches,
// no floating-point atomic, every sum combined in a fixed order.
//   k_xty_partial  grid (G, ceil(P / 16)).  Workgroup (g, c) takes stripe g of the rows (the stripe rule
//             of the header: a function of N alone) and the rows c 16 .. c 16 + 15 of C.  A lane owns
//             Q / 64 consecutive columns of B (one dword, dwordx2 or dwordx4 load per row) and keeps PT
//             x Q / 64 accumulators in registers, PT = 1, 2, 4, 8 or 16 the tile height that covers the
//             workgroup's rows of C.  Wave w of the four takes the stripe's rows w, w + 4, ...: the row
//             number is wave-uniform, so A's PT values of a row come through the scalar cache and feed
//             the fmaf chain as scalar operands.  Rows are taken up to four at a time per wave (their loads
//             issued together), then one by one.  The four waves' accumulators meet in LDS and are added
//             in wave order; the workgroup writes its partial [P][Q] tile rows, and (workgroups with c =
//             0 sum B's columns, every workgroup its own 16 columns of A) the partial sums, to the
//             workspace.
//   k_xty_final    one workgroup of 16 waves per 64 output elements.  Lane l owns an element; wave w adds
//             the partials of the stripes [w S, (w + 1) S), S = ceil(G / 16), in stripe order, in double;
//             the 16 sums meet in LDS and wave 0 adds them in wave order and rounds once to float32.
//
// Row n of A is 4 P bytes and starts 4-byte aligned only: it is read dword by dword (scalar loads).
// Every fused multiply-add is written as fmaf: the file is compiled without contraction, as the rest of
// the library (Makefile, HIPFLAGS), and the pragma states it whatever the command line says.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/hftlob.h"
#include "hftlob_internal.h"

#pragma clang fp contract(off)

namespace {

constexpr int NT = 256;                      // lanes per workgroup of k_xty_partial
constexpr int NW = NT / 64;                  // its waves: the row interleave
constexpr int UMAX = 4;                      // the most rows a wave has in flight
constexpr int PTMAX = 16;                    // the most rows of C a workgroup owns
constexpr int FW = 16;                       // waves per workgroup of k_xty_final
constexpr int STRIPE_ROWS = HFTLOB_XTY_STRIPE_ROWS;
constexpr int MAX_STRIPES = HFTLOB_XTY_MAX_STRIPES;
static_assert(HFTLOB_XTY_MAX_P <= 64 && HFTLOB_XTY_MAX_P % PTMAX == 0, "the p chunks of the grid");

// the stripe rule of the header: the rows of a stripe and the number of stripes, from N alone
long long stripe_rows(long long N) {
    const long long g = (N + STRIPE_ROWS - 1) / STRIPE_ROWS;
    return g <= MAX_STRIPES ? STRIPE_ROWS : (N + MAX_STRIPES - 1) / MAX_STRIPES;
}

int stripes(long long N) {
    if (N <= 0) return 0;
    const long long r = stripe_rows(N);
    return (int)((N + r - 1) / r);
}

long long partial_floats(int P, int Q) { return (long long)P * Q + P + Q; }

template <int V> struct Vec;
template <> struct Vec<1> { typedef float type; };
template <> struct Vec<2> { typedef float2 type; };
template <> struct Vec<4> { typedef float4 type; };

template <int V> __device__ __forceinline__ void unpack(const typename Vec<V>::type& x, float (&b)[V]);
template <> __device__ __forceinline__ void unpack<1>(const float& x, float (&b)[1]) { b[0] = x; }
template <> __device__ __forceinline__ void unpack<2>(const float2& x, float (&b)[2]) { b[0] = x.x, b[1] = x.y; }
template <> __device__ __forceinline__ void unpack<4>(const float4& x, float (&b)[4]) {
    b[0] = x.x, b[1] = x.y, b[2] = x.z, b[3] = x.w;
}

// one row: A's values of the tile's rows of C into a.  Past row P of C the tile's accumulators are never
// written out, so those a[p] only have to come from inside A.  load_a_wide reads PT consecutive floats
// (they run into the next rows where the tile is higher than the row is long: for rows below wide_end,
// where that stays inside A's N P floats); load_a repeats the row's last live value and leaves no row
template <int PT>
__device__ __forceinline__ void load_a_wide(const float* __restrict__ A, long long n, int P, int p0, float (&a)[PT]) {
    const float* ar = A + n * P + p0;
#pragma unroll
    for (int p = 0; p < PT; ++p) a[p] = ar[p];
}

template <int PT>
__device__ __forceinline__ void load_a(const float* __restrict__ A, long long n, int P, int p0, int live_p,
                                       float (&a)[PT]) {
    const float* ar = A + n * P + p0;
#pragma unroll
    for (int p = 0; p < PT; ++p) a[p] = ar[p < live_p ? p : live_p - 1];
}

template <int V>
__device__ __forceinline__ void load_b(const float* __restrict__ B, long long n, int Q, int lane, float (&b)[V]) {
    unpack<V>(*reinterpret_cast<const typename Vec<V>::type*>(B + n * Q + V * lane), b);
}

template <int PT, int V>
__device__ __forceinline__ void add_row(const float (&a)[PT], const float (&b)[V], bool want_a, bool want_b,
                                        float (&acc)[PT][V], float (&sa)[PT], float (&sb)[V]) {
#pragma unroll
    for (int p = 0; p < PT; ++p)
#pragma unroll
        for (int v = 0; v < V; ++v) acc[p][v] = fmaf(a[p], b[v], acc[p][v]);
    if (want_a) {
#pragma unroll
        for (int p = 0; p < PT; ++p) sa[p] += a[p];
    }
    if (want_b) {
#pragma unroll
        for (int v = 0; v < V; ++v) sb[v] += b[v];
    }
}

template <int PT, int Q>
__global__ __launch_bounds__(NT) void k_xty_partial(long long N, int P, long long rows, const float* __restrict__ A,
                                                    const float* __restrict__ B, int want_a, int want_b,
                                                    float* __restrict__ ws) {
    constexpr int V = Q / 64;
    constexpr int U = PT * UMAX <= 32 ? UMAX : 32 / PT;   // rows in flight: their values of A stay in scalar registers
    __shared__ float tile[NW][PT * Q];
    __shared__ float sums[NW][PTMAX + Q];
    const int tid = threadIdx.x, lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int p0 = blockIdx.y * PTMAX;
    const long long begin = (long long)blockIdx.x * rows;
    const long long end = begin + rows < N ? begin + rows : N;
    const bool wa = want_a != 0, wb = want_b != 0 && blockIdx.y == 0;
    const int live_p = P - p0 < PT ? P - p0 : PT;         // the tile's rows that are rows of C (>= 1)

    float acc[PT][V], sa[PT], sb[V];
#pragma unroll
    for (int p = 0; p < PT; ++p) {
        sa[p] = 0.0f;
#pragma unroll
        for (int v = 0; v < V; ++v) acc[p][v] = 0.0f;
    }
#pragma unroll
    for (int v = 0; v < V; ++v) sb[v] = 0.0f;

    // the rows n with n P + p0 + PT <= N P
    const long long wide_rows = (N * P - p0 - PT) / P + 1;
    const long long wide_end = N * P < p0 + PT ? 0 : wide_rows < end ? wide_rows : end;
    long long n = begin + w;
    for (; n + NW * (U - 1) < wide_end; n += NW * U) {
        float b[U][V];
#pragma unroll
        for (int u = 0; u < U; ++u) load_b<V>(B, n + NW * u, Q, lane, b[u]);
#pragma unroll
        for (int u = 0; u < U; ++u) {
            float a[PT];
            load_a_wide<PT>(A, n + NW * u, P, p0, a);
            add_row<PT, V>(a, b[u], wa, wb, acc, sa, sb);
        }
    }
    for (; n < end; n += NW) {
        float a[PT], b[V];
        load_b<V>(B, n, Q, lane, b);
        load_a<PT>(A, n, P, p0, live_p, a);
        add_row<PT, V>(a, b, wa, wb, acc, sa, sb);
    }

    // the four waves' sums meet in LDS
#pragma unroll
    for (int p = 0; p < PT; ++p)
#pragma unroll
        for (int v = 0; v < V; ++v) tile[w][p * Q + V * lane + v] = acc[p][v];
    if (lane == 0) {
#pragma unroll
        for (int p = 0; p < PT; ++p) sums[w][p] = sa[p];
    }
#pragma unroll
    for (int v = 0; v < V; ++v) sums[w][PTMAX + V * lane + v] = sb[v];
    __syncthreads();

    // ... and leave in wave order: the stripe's partial [P][Q] rows p0 .. p0 + PT - 1, then sum_a, sum_b
    float* out = ws + (long long)blockIdx.x * ((long long)P * Q + P + Q);
    const int live = live_p * Q;                          // the tile's elements that are rows of C
    for (int e = tid; e < live; e += NT)
        out[p0 * Q + e] = ((tile[0][e] + tile[1][e]) + tile[2][e]) + tile[3][e];
    if (wa && tid < live_p)
        out[(long long)P * Q + p0 + tid] = ((sums[0][tid] + sums[1][tid]) + sums[2][tid]) + sums[3][tid];
    if (wb) {
        for (int q = tid; q < Q; q += NT) {
            const int e = PTMAX + q;
            out[(long long)P * Q + P + q] = ((sums[0][e] + sums[1][e]) + sums[2][e]) + sums[3][e];
        }
    }
}
static_assert(NW == 4, "k_xty_partial adds four waves' sums");

__global__ __launch_bounds__(64 * FW) void k_xty_final(int G, int P, int Q, const float* __restrict__ ws,
                                                       float* __restrict__ C, float* __restrict__ sum_a,
                                                       float* __restrict__ sum_b) {
    __shared__ double part[FW][64];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int PQ = P * Q, stride = PQ + P + Q;
    const int e = blockIdx.x * 64 + lane;                 // an element of a partial: [C][sum_a][sum_b]
    // elements past the partial, and the sums nobody asked for (their partials were never written), are skipped
    float* dst = nullptr;
    if (e < PQ) dst = C + e;
    else if (e < PQ + P) dst = sum_a ? sum_a + (e - PQ) : nullptr;
    else if (e < stride) dst = sum_b ? sum_b + (e - PQ - P) : nullptr;
    const int per = (G + FW - 1) / FW;
    const int s0 = w * per, s1 = s0 + per < G ? s0 + per : G;
    double acc = 0.0;
    if (dst) {
        const float* src = ws + e;
#pragma unroll 8
        for (int s = s0; s < s1; ++s) acc += (double)src[(long long)s * stride];
    }
    part[w][lane] = acc;
    __syncthreads();
    if (w == 0 && dst) {
        double t = part[0][lane];
#pragma unroll
        for (int k = 1; k < FW; ++k) t += part[k][lane];
        *dst = (float)t;
    }
}

template <int Q>
void launch_partial(int PT, dim3 grid, hipStream_t s, long long N, int P, long long rows, const float* A,
                    const float* B, int wa, int wb, float* ws) {
    switch (PT) {
    case 1: k_xty_partial<1, Q><<<grid, NT, 0, s>>>(N, P, rows, A, B, wa, wb, ws); break;
    case 2: k_xty_partial<2, Q><<<grid, NT, 0, s>>>(N, P, rows, A, B, wa, wb, ws); break;
    case 4: k_xty_partial<4, Q><<<grid, NT, 0, s>>>(N, P, rows, A, B, wa, wb, ws); break;
    case 8: k_xty_partial<8, Q><<<grid, NT, 0, s>>>(N, P, rows, A, B, wa, wb, ws); break;
    default: k_xty_partial<16, Q><<<grid, NT, 0, s>>>(N, P, rows, A, B, wa, wb, ws); break;
    }
}

int shape_error(long long N, int P, int Q) {
    if (P < 1 || P > HFTLOB_XTY_MAX_P) return hftlob_fail(HFTLOB_ESHAPE, "xty: P must be in 1..64");
    if (Q != 64 && Q != 128 && Q != 256) return hftlob_fail(HFTLOB_ESHAPE, "xty: Q must be 64, 128 or 256");
    if (N < 0) return hftlob_fail(HFTLOB_ESHAPE, "xty: N must be >= 0");
    return HFTLOB_OK;
}

int hip_error(hipError_t err) {
    return err == hipSuccess ? HFTLOB_OK : hftlob_fail(HFTLOB_ELAUNCH, hipGetErrorString(err));
}

}  // namespace

extern "C" long long hftlob_xty_workspace(long long N, int P, int Q) {
    const int rc = shape_error(N, P, Q);
    if (rc != HFTLOB_OK) return rc;
    return stripes(N) * partial_floats(P, Q);
}

extern "C" int hftlob_xty(long long N, int P, int Q, const float* A, const float* B, float* C, float* sum_a,
                          float* sum_b, float* workspace, void* stream) {
    const int rc = shape_error(N, P, Q);
    if (rc != HFTLOB_OK) return rc;
    if (!C) return hftlob_fail(HFTLOB_ENULL, "xty: C is NULL");
    hipStream_t s = (hipStream_t)stream;
    if (N == 0) {   // empty sums: zeros, and nothing else is read
        hipError_t err = hipMemsetAsync(C, 0, sizeof(float) * P * Q, s);
        if (err == hipSuccess && sum_a) err = hipMemsetAsync(sum_a, 0, sizeof(float) * P, s);
        if (err == hipSuccess && sum_b) err = hipMemsetAsync(sum_b, 0, sizeof(float) * Q, s);
        return hip_error(err);
    }
    if (!A || !B || !workspace) return hftlob_fail(HFTLOB_ENULL, "xty: a null pointer (A, B, workspace)");
    if ((uintptr_t)B & 15) return hftlob_fail(HFTLOB_EINVAL, "xty: B must be 16-byte aligned");
    const long long rows = stripe_rows(N);
    const int G = stripes(N);
    // the smallest tile height that covers a workgroup's rows of C
    int PT = 1;
    while (PT < PTMAX && PT < P) PT *= 2;
    const dim3 grid((unsigned)G, (unsigned)((P + PTMAX - 1) / PTMAX));
    const int wa = sum_a != nullptr, wb = sum_b != nullptr;
    if (Q == 64) launch_partial<64>(PT, grid, s, N, P, rows, A, B, wa, wb, workspace);
    else if (Q == 128) launch_partial<128>(PT, grid, s, N, P, rows, A, B, wa, wb, workspace);
    else launch_partial<256>(PT, grid, s, N, P, rows, A, B, wa, wb, workspace);
    const int elems = P * Q + (wa || wb ? P + Q : 0);
    k_xty_final<<<dim3((unsigned)((elems + 63) / 64)), 64 * FW, 0, s>>>(G, P, Q, workspace, C, sum_a, sum_b);
    return hip_error(hipGetLastError());
}
