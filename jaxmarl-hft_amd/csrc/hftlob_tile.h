// The 16-row MFMA tile shared by the GRU scan (gru_scan.hip) and the policy step (policy_step.hip);
// not part of the public ABI (include/hftlob.h).
#ifndef HFTLOB_TILE_H
#define HFTLOB_TILE_H

#include <hip/hip_runtime.h>

#include "../../include/hftlob.h"
#include "hftlob_internal.h"

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int TILE = 16;  // batch rows per workgroup: the M of mfma_f32_16x16x4f32

// MFMA operand maps (16x16x4 f32): lane l gives A[row l & 15][k l >> 4] and B[k l >> 4][col l & 15];
// accumulator register i of lane l is D[row 4 (l >> 4) + i][col l & 15].

__device__ __forceinline__ float sigmoidf_(float x) { return 1.0f / (1.0f + expf(-x)); }
__device__ __forceinline__ f32x4 ld4(const float* p) { return *reinterpret_cast<const f32x4*>(p); }
__device__ __forceinline__ void st4(float* p, f32x4 v) { *reinterpret_cast<f32x4*>(p) = v; }
__device__ __forceinline__ f32x4 splat(float x) { return f32x4{x, x, x, x}; }

// the status of the launch just made, as the operator's return code
static inline int launch_status() {
    const hipError_t err = hipGetLastError();
    return err == hipSuccess ? HFTLOB_OK : hftlob_fail(HFTLOB_ELAUNCH, hipGetErrorString(err));
}

#endif
