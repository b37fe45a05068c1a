// Device pieces of the split-bf16 4-phase transposed conv shared by convt_x3_kernel (conv_gemm.hip, raw T to HBM)
// and convt_x3_fir_kernel (convt_fir.hip, the 4x4 FIR and the modconv epilogue applied from LDS): the parameter
// block, the three-term bf16 split, its six-product MFMA and the K loop itself.  Both kernels run the same loop in
// the same order, so a position's accumulators are the same bits in either.
#pragma once
#include <type_traits>

#include "common.hpp"

namespace smc {
namespace cg {

constexpr int NT = 256;
typedef float f32x16 __attribute__((ext_vector_type(16)));

struct PhaseDev {
    int ntaps;
    int dy[9];
    int dx[9];
    int in_stride;
    int out_h, out_w, out_oy, out_ox, out_sy, out_sx;
    const float* wk;
    int64_t wstride;  // LDS-DMA kernel: floats between two samples' weights (0 = shared weights)
    const short* wx3;    // split-bf16 kernel: the three-term bf16 planes of wk (x3_weights_kernel layout)
    int64_t wx3_stride;  // bf16 elements between two samples' planes (0 = shared weights)
};

struct GemmParams {
    const float* x;
    int n, cin, in_h, in_w;
    float* y;
    int cout, y_h, y_w;
    PhaseDev ph[4];
    int nphases;
    const float* s;
    int mode;
    const float* d;
    const float* noise;
    int64_t noise_nstride;
    const float* noise_strength;
    const float* bias;
    int act;
    float alpha, gain, clamp;
    float* u_save;
    smc::EpiExt ext;
    int nsplit;
    int64_t split_stride;
    int per_sample;  // LDS-DMA kernel: blockIdx.x -> (sample, tile of that sample): no tile straddles two images
    int ntn;         // LDS-DMA kernel: column tiles; grid.x = row tiles x ntn, XCD-swizzled (0: 2-D grid)
};

template <int N>
__device__ __forceinline__ void wait_vmcnt() {
    asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
}

typedef short bf16x8 __attribute__((ext_vector_type(8)));

// a = t0 + t1 + t2 for each of 8 values, as three bf16x8 fragments (the high halves of a, a - t0, a - t0 - t1)
__device__ __forceinline__ void x3_split8(const float (&x)[8], bf16x8 (&t)[3]) {
    unsigned u0[8], u1[8], u2[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const unsigned u = __float_as_uint(x[j]);
        const float r1 = x[j] - __uint_as_float(u & 0xffff0000u);
        const unsigned v = __float_as_uint(r1);
        const float r2 = r1 - __uint_as_float(v & 0xffff0000u);
        u0[j] = u;
        u1[j] = v;
        u2[j] = __float_as_uint(r2);
    }
    typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
    u32x4 w0, w1, w2;
#pragma unroll
    for (int j = 0; j < 4; ++j) {  // (high half of element 2j) | (high half of element 2j + 1) << 16
        w0[j] = __builtin_amdgcn_perm(u0[2 * j + 1], u0[2 * j], 0x07060302u);
        w1[j] = __builtin_amdgcn_perm(u1[2 * j + 1], u1[2 * j], 0x07060302u);
        w2[j] = __builtin_amdgcn_perm(u2[2 * j + 1], u2[2 * j], 0x07060302u);
    }
    t[0] = __builtin_bit_cast(bf16x8, w0);
    t[1] = __builtin_bit_cast(bf16x8, w1);
    t[2] = __builtin_bit_cast(bf16x8, w2);
}

// acc += a * b over the six split products, smallest first
__device__ __forceinline__ f32x16 x3_mma(const bf16x8 (&a)[3], const bf16x8 (&b)[3], f32x16 acc) {
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[2], b[0], acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[1], b[1], acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[0], b[2], acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[1], b[0], acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[0], b[1], acc, 0, 0, 0);
    return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[0], b[0], acc, 0, 0, 0);
}

__host__ __device__ constexpr int shift_nph(int s) { return s == 0 ? 4 : (s == 3 ? 1 : 2); }

struct ConvTTaps {
    int tap[4][4];  // [shift][phase] -> tap index in phase `phase`'s packed weights (-1: phase unused)
};

template <int S>
__host__ __device__ constexpr int shift_phase(int j) {
    // j-th phase reading shift S (the ShiftPhases table as a constexpr function)
    return S == 0 ? j : (S == 1 ? (j ? 1 : 0) : (S == 2 ? (j ? 2 : 0) : 0));
}

// Tile constants of the split-bf16 transposed conv: BO output channels x BM super-pixels, 16-channel K steps
template <int WO, int WM, int TO, int TM>
struct ConvTX3 {
    static_assert(WO * WM == 4, "4 waves");
    static constexpr int BKT = 16;
    static constexpr int BO = WO * TO * 32;
    static constexpr int BM = WM * TM * 32;
    static constexpr int NCH = BM / 64;
    static_assert(NCH >= 1 && NCH <= 4 && 4 % NCH == 0, "BM in {64,128,256}");
    static constexpr int RSTEP = 4 / NCH;
    static constexpr int XI = BKT * NCH / 4;
    static constexpr int PB = 6 * BO * 16;              // bytes of one phase's planes per step
    static_assert(PB % 1024 == 0, "phase planes split into whole 1-KB DMAs");
    static constexpr int XB = BKT * BM * 4;
    static constexpr int STAGE = XB + 4 * PB;           // input slab + up to 4 phases' planes
    static constexpr int RING = 2 * STAGE;              // bytes of LDS the loop needs
};

// The K loop: per K step (16 channels, one input shift) the fp32 input slab [16][BM] and, for every phase reading
// that shift, its weight planes [3][2][BO][8] bf16 go global -> LDS by DMA into a 2-stage ring; a wave splits each B
// fragment once and feeds it to every phase's A fragments.  The calling lane stages the super-pixel (a, b) of image
// nn as position (wave % NCH) * 64 + lane of the tile (mvalid false, or a shift outside the image: zeros); wn is
// the workgroup's sample (per-sample weights), o0 its first output channel; steps ks_begin .. ks_end - 1, both
// multiples of 4 (whole channel chunks).  Leaves acc[phase][i][j] of the wave's TO x TM blocks.
template <int WO, int WM, int TO, int TM>
__device__ __forceinline__ void convt_x3_loop(const GemmParams& p, const ConvTTaps& tt, char* smem, bool mvalid,
                                              int nn, int a, int b, int wn, int o0, int ks_begin, int ks_end,
                                              f32x16 (&acc)[4][TO][TM]) {
    typedef ConvTX3<WO, WM, TO, TM> C;
    constexpr int BKT = C::BKT, BO = C::BO, BM = C::BM, NCH = C::NCH, RSTEP = C::RSTEP, XI = C::XI, PB = C::PB,
                  XB = C::XB, STAGE = C::STAGE;
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wo = wave / WM, wm = wave % WM;
    const int cw = wave % NCH, r0 = wave / NCH;
    const int in_hw = p.in_h * p.in_w;
    const __amdgpu_buffer_rsrc_t xrsrc = __builtin_amdgcn_make_buffer_rsrc(
        (void*)p.x, (short)0, (int)((int64_t)p.n * p.cin * in_hw * 4), 0x00020000);
    const int xvbase = nn * p.cin * in_hw * 4;
    const int c16n = p.cin / 16;

    auto issue = [&](int ks, int slot) {
        const int c = ks >> 2, sh = ks & 3;
        const int ci0 = c * BKT;
        const int iy = a - (sh & 1), ix = b - (sh >> 1);
        const bool ok = mvalid && iy >= 0 && iy < p.in_h && ix >= 0 && ix < p.in_w;
        const int voff = ok ? xvbase + (iy * p.in_w + ix) * 4 : 0x7ffffff0;
        char* st = smem + slot * STAGE;
        float* xs = reinterpret_cast<float*>(st);
#pragma unroll
        for (int j = 0; j < XI; ++j) {
            const int row = r0 + RSTEP * j;
            __builtin_amdgcn_raw_ptr_buffer_load_lds(
                xrsrc, (__attribute__((address_space(3))) void*)(xs + row * BM + cw * 64), 4, voff,
                (ci0 + row) * in_hw * 4, 0, 0);
        }
        const int nph = shift_nph(sh);
        for (int j = wave; j < nph * (PB / 1024); j += 4) {
            const int pj = j / (PB / 1024);          // which phase of this shift
            const int phase = sh == 0 ? pj : (sh == 1 ? (pj ? 1 : 0) : (sh == 2 ? (pj ? 2 : 0) : 0));
            const int L = (j - pj * (PB / 1024)) * 64 + lane;
            const int run = L / BO, o = L - run * BO;
            const PhaseDev& q = p.ph[phase];
            const short* src = q.wx3 + (q.wx3_stride ? (int64_t)wn * q.wx3_stride : 0) +
                               ((((int64_t)tt.tap[sh][phase] * c16n + ci0 / 16) * 6 + run) * p.cout + o0 + o) * 8;
            __builtin_amdgcn_global_load_lds((const void*)src, (__attribute__((address_space(3))) void*)(st + XB + j * 1024),
                                             16, 0, 0);
        }
    };

#pragma unroll
    for (int ph = 0; ph < 4; ++ph)
#pragma unroll
        for (int i = 0; i < TO; ++i)
#pragma unroll
            for (int j = 0; j < TM; ++j)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[ph][i][j][r] = 0.f;

    const int kh = lane >> 5, l32 = lane & 31;
    if (ks_begin < ks_end) issue(ks_begin, 0);
    auto step = [&](auto S_, int ks) {
        constexpr int S = decltype(S_)::value;
        constexpr int NP = shift_nph(S);
        wait_vmcnt<0>();
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
        const char* st = smem + (S & 1) * STAGE;
        const float* xcol = reinterpret_cast<const float*>(st) + wm * TM * 32 + l32;
        bf16x8 bt[TM][3];
#pragma unroll
        for (int j = 0; j < TM; ++j) {
            float xv[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) xv[e] = xcol[(8 * kh + e) * BM + j * 32];
            x3_split8(xv, bt[j]);
        }
        __builtin_amdgcn_sched_barrier(0);
        if (ks + 1 < ks_end) issue(ks + 1, (S + 1) & 1);
#pragma unroll
        for (int pj = 0; pj < NP; ++pj) {
            const short* Wp = reinterpret_cast<const short*>(st + XB + pj * PB);
            bf16x8 at[TO][3];
#pragma unroll
            for (int i = 0; i < TO; ++i)
#pragma unroll
                for (int s = 0; s < 3; ++s)
                    at[i][s] = *reinterpret_cast<const bf16x8*>(Wp + (((s * 2 + kh) * BO) + wo * TO * 32 + i * 32 + l32) * 8);
#pragma unroll
            for (int i = 0; i < TO; ++i)
#pragma unroll
                for (int j = 0; j < TM; ++j)
                    acc[shift_phase<S>(pj)][i][j] = x3_mma(at[i], bt[j], acc[shift_phase<S>(pj)][i][j]);
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    };
    for (int ks = ks_begin; ks < ks_end; ks += 4) {
        step(std::integral_constant<int, 0>{}, ks);
        step(std::integral_constant<int, 1>{}, ks + 1);
        step(std::integral_constant<int, 2>{}, ks + 2);
        step(std::integral_constant<int, 3>{}, ks + 3);
    }
}

}  // namespace cg

// conv_gemm.hip, for the fused up=2 launch (convt_fir.hip): validates the 4-phase stride-2 transposed conv
// description as smc_conv_gemm_f32 does for its convt_x3_kernel route, builds the per-sample split-bf16 weight planes
// W * s in `workspace` (s_in != NULL; the bytes smc_conv_gemm_workspace_size reports for the raw-T launch cover
// them) and fills the conv part of *p and *tt.  SMC_ERR_UNSUPPORTED where that route does not apply (no split
// planes, channels, >= 2 GiB input).
int convt_up2_prepare(const float* x, int n, int cin, int h, int w, float* y, int cout, const smc_conv_phase* phases,
                      int nphases, const float* s_in, float* workspace, int64_t workspace_bytes, void* stream,
                      cg::GemmParams* p, cg::ConvTTaps* tt);
// conv_gemm.hip: the shape conditions of that route alone (host logic), and whether the raw-T launch of the shape
// plans what the fused kernel computes -- one unsplit launch at the planning batch, style-scaled weights
bool convt_up2_shape_ok(int n, int cin, int cout, int h, int w);
bool convt_up2_plan_ok(int n, int cin, int cout, int h, int w);

}  // namespace smc
