// The IPPO update's optimiser step as an engine operator (include/hftlob.h: hftlob_adam_clip), gfx950,
// float32: torch.nn.utils.clip_grad_norm_ followed by one step of torch.optim.Adam (capturable, no weight
// decay, no amsgrad) over the up to 16 parameter tensors of one net.  hftlob/train/optim.py restates it
// in torch (adam_clip_reference).
//
// The tensors' pointers and sizes travel by value in the kernel arguments (struct Table, about 900
// bytes): inside a captured graph the gradients' addresses are fixed, in eager steps they change with
// every call, and kernel arguments serve both without a copy to the device.  A workgroup indexes the
// table with a wave-uniform tensor number, which the compiler turns into scalar loads from the kernarg
// segment at a register offset; nothing is copied to scratch (make asm_opt prints the metadata).
//
// Two launches, no floating-point atomic, every sum combined in a fixed order:
//   k_norm    up to NORM_BLOCKS workgroups; workgroup b takes the chunks b, b + grid, b + 2 grid, ...
//             of CHUNK elements (a tensor's chunks are its own, so a chunk starts 16-byte aligned) and
//             sums g^2 in double: per lane over its chunks, then over the wave, then over the four
//             waves, one partial sum per workgroup into the workspace.  Workgroup 0 also adds 1 to
//             every tensor's step, lane t to tensor t's: k_update starts after k_norm has finished, so
//             it reads the incremented steps and no workgroup races with the writer.
//   k_update  one workgroup per chunk.  Every wave folds the partial sums with the same xor-shuffle
//             tree (the same bits in every lane of every workgroup), forms coef, the bias corrections
//             of its tensor's step and the step size in double, each rounded to float32 once, and
//             applies Adam to its chunk: a lane owns four consecutive elements, read and written as
//             one float4 where all four exist, one by one in a tensor's last, short quad.
//             p, g, m, v are read once, p, m, v written once: 28 bytes per parameter, and g a second
//             time after k_norm.
//
// No floating-point contraction, as in the rest of the library (Makefile, HIPFLAGS): the element math
// is the separately rounded operations the header lists.  The pragma states it for this file whatever
// the command line says.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/hftlob.h"
#include "hftlob_internal.h"

#pragma clang fp contract(off)

namespace {

constexpr int NT = 256;                               // lanes per workgroup
constexpr int MAXT = HFTLOB_ADAM_MAX_TENSORS;
constexpr int CHUNK = HFTLOB_ADAM_CHUNK;              // elements per workgroup of k_update
constexpr int NORM_BLOCKS = HFTLOB_ADAM_NORM_BLOCKS;  // at most one partial sum per lane of a wave
static_assert(CHUNK == 4 * NT, "a lane owns one float4 of its workgroup's chunk");
static_assert(NORM_BLOCKS <= 64, "k_update folds the partial sums inside one wave");
static_assert(HFTLOB_ADAM_WORKSPACE >= NORM_BLOCKS, "the workspace of hftlob.h");

// the tensors by value; first[t] is tensor t's first chunk, first[nt] the number of chunks
struct Table {
    float* p[MAXT];
    const float* g[MAXT];
    float* m[MAXT];
    float* v[MAXT];
    float* step[MAXT];
    long long n[MAXT];
    int first[MAXT + 1];
    int nt;
};

__device__ __forceinline__ double wave_sum(double v) {
    for (int m = 1; m < 64; m <<= 1) v += __shfl_xor(v, m);
    return v;
}

__device__ __forceinline__ double sq(float x) { return (double)x * (double)x; }

__global__ __launch_bounds__(NT) void k_adam_norm(const Table tb, double* __restrict__ ws) {
    __shared__ double part[NT / 64];
    const int tid = threadIdx.x;
    if (blockIdx.x == 0 && tid < tb.nt) {
        float* s = tb.step[tid];
        *s = *s + 1.0f;
    }
    const long long chunks = tb.first[tb.nt];
    double acc = 0.0;
    int t = 0;
    for (long long c = blockIdx.x; c < chunks; c += gridDim.x) {
        while (c >= tb.first[t + 1]) ++t;             // (c < first[nt]: t stays below nt)
        const long long off = (c - tb.first[t]) * CHUNK + 4 * tid;
        const long long left = tb.n[t] - off;         // the tensor's elements from this lane's first on
        const float* g = tb.g[t] + off;
        if (left >= 4) {
            const float4 x = *reinterpret_cast<const float4*>(g);
            acc += sq(x.x);
            acc += sq(x.y);
            acc += sq(x.z);
            acc += sq(x.w);
        } else {
            if (left > 0) acc += sq(g[0]);
            if (left > 1) acc += sq(g[1]);
            if (left > 2) acc += sq(g[2]);
        }
    }
    acc = wave_sum(acc);
    if ((tid & 63) == 0) part[tid >> 6] = acc;
    __syncthreads();
    if (tid == 0) ws[blockIdx.x] = ((part[0] + part[1]) + part[2]) + part[3];
}

struct Scalars {
    float coef, omb1, beta2, omb2, step_size, sqrt_bc2, eps;
};

__device__ __forceinline__ void adam1(const Scalars& s, float& p, float g, float& m, float& v) {
    const float gc = g * s.coef;
    m = m + (gc - m) * s.omb1;
    v = v * s.beta2 + s.omb2 * (gc * gc);
    p = p - s.step_size * (m / (sqrtf(v) / s.sqrt_bc2 + s.eps));
}

__global__ __launch_bounds__(NT) void k_adam_update(const Table tb, const float* __restrict__ lr, double log_beta1,
                                                    double log_beta2, float omb1, float beta2, float omb2, float eps,
                                                    double max_norm, int parts, const double* __restrict__ ws,
                                                    float* __restrict__ total_norm) {
    const int tid = threadIdx.x, l = tid & 63;
    const int c = blockIdx.x;
    int t = 0;
    while (c >= tb.first[t + 1]) ++t;                 // (the grid is first[nt] workgroups: t stays below nt)

    // the norm from the partial sums, the same tree in every wave of every workgroup
    const double tn = sqrt(wave_sum(l < parts ? ws[l] : 0.0));
    const double cd = max_norm / (tn + 1e-6);
    // the tensor's step after k_adam_norm's increment; 1 - beta^step as -expm1(step log beta)
    const double st = (double)*tb.step[t];
    const double bc1 = -expm1(st * log_beta1), bc2 = -expm1(st * log_beta2);
    Scalars s;
    s.coef = (float)(cd > 1.0 ? 1.0 : cd);            // (a NaN norm stays NaN)
    s.omb1 = omb1, s.beta2 = beta2, s.omb2 = omb2, s.eps = eps;
    s.step_size = (float)((double)*lr / bc1);
    s.sqrt_bc2 = (float)sqrt(bc2);
    if (c == 0 && tid == 0 && total_norm) *total_norm = (float)tn;

    const long long off = (long long)(c - tb.first[t]) * CHUNK + 4 * tid;
    const long long left = tb.n[t] - off;
    float* p = tb.p[t] + off;
    const float* g = tb.g[t] + off;
    float* m = tb.m[t] + off;
    float* v = tb.v[t] + off;
    if (left >= 4) {
        float4 P = *reinterpret_cast<const float4*>(p);
        const float4 G = *reinterpret_cast<const float4*>(g);
        float4 M = *reinterpret_cast<const float4*>(m);
        float4 V = *reinterpret_cast<const float4*>(v);
        adam1(s, P.x, G.x, M.x, V.x);
        adam1(s, P.y, G.y, M.y, V.y);
        adam1(s, P.z, G.z, M.z, V.z);
        adam1(s, P.w, G.w, M.w, V.w);
        *reinterpret_cast<float4*>(p) = P;
        *reinterpret_cast<float4*>(m) = M;
        *reinterpret_cast<float4*>(v) = V;
    } else {
        for (int j = 0; j < 3; ++j) {
            if (j >= left) break;
            float P = p[j], M = m[j], V = v[j];
            adam1(s, P, g[j], M, V);
            p[j] = P, m[j] = M, v[j] = V;
        }
    }
}

int launched() {
    const hipError_t err = hipGetLastError();
    return err == hipSuccess ? HFTLOB_OK : hftlob_fail(HFTLOB_ELAUNCH, hipGetErrorString(err));
}

bool aligned16(const void* q) { return ((uintptr_t)q & 15) == 0; }

}  // namespace

extern "C" int hftlob_adam_clip(int n_tensors, const hftlob_adam_tensor* tensors, const float* lr, double beta1,
                                double beta2, float eps, float max_norm, double* workspace, float* total_norm,
                                void* stream) {
    if (n_tensors < 1 || n_tensors > MAXT) return hftlob_fail(HFTLOB_ESHAPE, "adam_clip: n_tensors must be in 1..16");
    if (!tensors) return hftlob_fail(HFTLOB_ENULL, "adam_clip: tensors is NULL");
    Table tb;
    long long chunks = 0;
    for (int t = 0; t < MAXT; ++t) {
        const hftlob_adam_tensor& x = tensors[t < n_tensors ? t : 0];   // (the unused entries repeat the first)
        if (t < n_tensors) {
            if (x.n < 1) return hftlob_fail(HFTLOB_ESHAPE, "adam_clip: a tensor's n must be >= 1");
            if (!x.p || !x.g || !x.m || !x.v || !x.step)
                return hftlob_fail(HFTLOB_ENULL, "adam_clip: a null pointer in a tensor (p, g, m, v, step)");
            if (!aligned16(x.p) || !aligned16(x.g) || !aligned16(x.m) || !aligned16(x.v))
                return hftlob_fail(HFTLOB_EINVAL, "adam_clip: p, g, m and v must be 16-byte aligned");
            tb.first[t] = (int)chunks;
            chunks += (x.n + CHUNK - 1) / CHUNK;
            if (chunks > INT32_MAX) return hftlob_fail(HFTLOB_ESHAPE, "adam_clip: more than 2^31 - 1 chunks");
        } else {
            tb.first[t] = (int)chunks;
        }
        tb.p[t] = x.p, tb.g[t] = x.g, tb.m[t] = x.m, tb.v[t] = x.v, tb.step[t] = x.step, tb.n[t] = x.n;
    }
    tb.first[MAXT] = (int)chunks;
    tb.nt = n_tensors;
    if (!lr || !workspace) return hftlob_fail(HFTLOB_ENULL, "adam_clip: a null pointer (lr, workspace)");
    if (!isfinite(max_norm) || !(max_norm > 0.0f))
        return hftlob_fail(HFTLOB_EINVAL, "adam_clip: max_norm must be finite and > 0");
    if (!(beta1 >= 0.0 && beta1 < 1.0) || !(beta2 >= 0.0 && beta2 < 1.0))
        return hftlob_fail(HFTLOB_EINVAL, "adam_clip: beta1 and beta2 must be in [0, 1)");
    if (!isfinite(eps) || !(eps >= 0.0f)) return hftlob_fail(HFTLOB_EINVAL, "adam_clip: eps must be finite and >= 0");
    const int parts = (int)(chunks < NORM_BLOCKS ? chunks : NORM_BLOCKS);
    hipStream_t s = (hipStream_t)stream;
    k_adam_norm<<<dim3((unsigned)parts), NT, 0, s>>>(tb, workspace);
    k_adam_update<<<dim3((unsigned)chunks), NT, 0, s>>>(tb, lr, log(beta1), log(beta2), (float)(1.0 - beta1),
                                                        (float)beta2, (float)(1.0 - beta2), eps, (double)max_norm, parts,
                                                        workspace, total_norm);
    return launched();
}
