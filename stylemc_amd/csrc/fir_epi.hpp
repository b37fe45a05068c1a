// The conv0 FIR + modconv epilogue pieces shared by blur_act_v4 (modconv_aux.hip) and the fused up=2 kernel
// (convt_fir.hip): both produce y bit for bit the same way -- per output one __fmaf_rn chain from 0 over the 16
// taps (jy ascending, jx ascending within it), then the same epilogue expression and the same store.
#pragma once
#include "common.hpp"

namespace smc {

// The synthesis' resample filter, setup_filter([1,3,3,1]) = k k^T / 64, times the conv0 FIR gain 4, as compile-time
// constants k_i k_j / 16 (exact in fp32, equal bit for bit to the values load_taps reads and scales): the FMAs take
// literal operands and the 16 taps need no registers (blur_act_v4: 140 -> fewer VGPRs, more waves per SIMD for a
// memory-bound kernel).  Symmetric, so the flip does not matter.
template <int FH, int FW>
__device__ __forceinline__ void std_taps(float (&tp)[FH][FW]) {
    constexpr float k[4] = {1.f, 3.f, 3.f, 1.f};
#pragma unroll
    for (int jy = 0; jy < FH; ++jy)
#pragma unroll
        for (int jx = 0; jx < FW; ++jx) tp[jy][jx] = k[jy] * k[jx] * 0.0625f;
}

template <bool NT>
__device__ __forceinline__ void st_f2(float* p, float2 v) {
    if (NT) {
        typedef float f32x2 __attribute__((ext_vector_type(2)));
        __builtin_nontemporal_store(f32x2{v.x, v.y}, reinterpret_cast<f32x2*>(p));   // one dwordx2 store
    } else {
        *reinterpret_cast<float2*>(p) = v;
    }
}

// the synthesis' conv0 epilogue (lrelu with 0 <= alpha <= 1, gain, clamp >= 0) takes the max / min forms of
// lrelu_gain_clamp, bit-identical to epi_y for finite values
__device__ __forceinline__ bool modact_lrelu_clamp(int act, float alpha, float clamp) {
    return act == SMC_ACT_LRELU && alpha >= 0.f && alpha <= 1.f && clamp >= 0.f;
}

// y of two adjacent FIR outputs u2 (nz: their noise already times its strength)
__device__ __forceinline__ float2 modact2(float2 u2, float dv, float2 nz, float bv, bool lrelu_clamp, int act,
                                          float alpha, float gain, float clamp) {
    float2 q;
    if (lrelu_clamp) {
        const float zx = __fmaf_rn(u2.x, dv, nz.x) + bv, zy = __fmaf_rn(u2.y, dv, nz.y) + bv;
        q.x = lrelu_gain_clamp(zx, alpha, gain, clamp);
        q.y = lrelu_gain_clamp(zy, alpha, gain, clamp);
    } else {
        q = make_float2(epi_y(u2.x, dv, nz.x, bv, act, alpha, gain, clamp),
                        epi_y(u2.y, dv, nz.y, bv, act, alpha, gain, clamp));
    }
    return q;
}

}  // namespace smc
