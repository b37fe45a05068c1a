// Convolution weight gradient as an implicit GEMM on the exact-fp32 MFMA (v_mfma_f32_32x32x2_f32) for gfx950.
//
// Replaces the weight-gradient half of the reference's torch_utils/ops/conv2d_gradfix.py (the cuDNN
// conv2d_weight / conv_transpose2d weight gradient its Conv2dGradWeight function calls):
//     dw[o][i][ky][kx] = sum_{n,a,b} grad[n,o,a,b] * inp[n, i, a*stride + ky - pad_y, b*stride + kx - pad_x]
// (reads outside inp are 0).  GEMM shape: M = cout, N = cin x taps, K = n * out_h * out_w; K is the flattened
// (n, a, b) index, so both operands are K-contiguous in NCHW (a row of grad; a row of inp per tap shift).
//
// Tiling: one wave (a 64-thread workgroup) owns 32 output channels x 32 input channels x all taps -- 9 x 16 = 144
// accumulator registers for a 3x3 kernel -- and walks its K range in chunks of 16 positions.  Per chunk the wave
// stages grad[32 o][16 k] and, per tap, the shifted inp[32 i][16 k] into LDS (masked: channels past
// cout / cin, positions past the K range and taps that fall outside the image are written as zeros, so tile edges
// need no host-side padding), then issues 8 K-steps in which one ds_read_b32 of grad feeds the MFMAs of every tap.
// Channel-row pitch 18 floats: the 32 lanes of an operand read (row = lane & 31, k = 2q + (lane >> 5)) hit 64
// distinct banks.
//
// Split-K: cout x cin gives few tiles, so a host planner splits the K chunks across workgroups (grid.y).  Each
// split writes its partial [cout][cin][taps] block into the caller's workspace and a second kernel sums the
// partials in split order: no floating-point atomics, bit-identical from run to run.
#include <algorithm>

#include "common.hpp"

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int WT = 32;      // channels per tile side (one MFMA block)
constexpr int KC = 16;      // K positions per chunk: (1 + 9) x 32 x PITCH floats = 22.5 KiB of LDS, 7 workgroups per CU
constexpr int PITCH = 18;   // LDS floats per channel row: 18 j mod 64 = 2 (9 j mod 32), distinct even banks
constexpr int CG = 64 / KC; // staging: lane = (channel group, position); a lane loads channels CG j + group
constexpr int CJ = WT / CG;
constexpr int kMinChunks = 8;   // chunks per split at least: a split's partial store is spread over >= 128 positions
constexpr int kWavesPerCu = 8;  // split-K target: two waves per SIMD (the kernel's occupancy)

struct WgradParams {
    const float* inp;
    const float* grad;
    float* out;            // dw (nsplit == 1) or the partial planes
    int64_t split_stride;  // floats between partial planes
    int n, cin, cout, in_h, in_w, out_h, out_w, stride, pad_y, pad_x;
    int K, chunks, chunks_per_split, itiles;
};

template <int TAPS>
__global__ __launch_bounds__(64) void conv_wgrad_kernel(WgradParams p) {
    constexpr int KS = TAPS == 9 ? 3 : 1;
    __shared__ float gsh[WT * PITCH];
    __shared__ float ish[TAPS * WT * PITCH];
    const int lane = threadIdx.x;
    const int l32 = lane & 31, hi = lane >> 5;
    const int ot = blockIdx.x / p.itiles;
    const int o0 = ot * WT, i0 = (blockIdx.x - ot * p.itiles) * WT;
    const int split = blockIdx.y;
    const int c_begin = split * p.chunks_per_split;
    const int c_end = min(p.chunks, c_begin + p.chunks_per_split);
    const int ohw = p.out_h * p.out_w, ihw = p.in_h * p.in_w;

    f32x16 acc[TAPS];
#pragma unroll
    for (int t = 0; t < TAPS; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;

    for (int c = c_begin; c < c_end; ++c) {
        // this lane stages position k of the chunk for the channels CG j + cg of each operand
        const int lk = lane % KC, cg = lane / KC;
        const int k = c * KC + lk;
        const bool valid = k < p.K;
        const int kk = valid ? k : 0;
        const int en = kk / ohw;
        const int rem = kk - en * ohw;
        const int a = rem / p.out_w;
        const int b = rem - a * p.out_w;
        {
            // masked elements load element 0 (always in bounds) and are replaced by 0: unconditional loads, so the
            // CJ of them are in flight together instead of one branch region and one round trip each
            const int base = en * p.cout * ohw + rem;
            float v[CJ];
#pragma unroll
            for (int j = 0; j < CJ; ++j) {
                const int o = o0 + CG * j + cg;
                v[j] = p.grad[valid && o < p.cout ? base + o * ohw : 0];
            }
#pragma unroll
            for (int j = 0; j < CJ; ++j) {
                const int o = o0 + CG * j + cg;
                gsh[(CG * j + cg) * PITCH + lk] = valid && o < p.cout ? v[j] : 0.f;
            }
        }
#pragma unroll
        for (int t = 0; t < TAPS; ++t) {
            const int iy = a * p.stride + t / KS - p.pad_y;
            const int ix = b * p.stride + t % KS - p.pad_x;
            const bool ok = valid && iy >= 0 && iy < p.in_h && ix >= 0 && ix < p.in_w;
            const int base = en * p.cin * ihw + iy * p.in_w + ix;
            float v[CJ];
#pragma unroll
            for (int j = 0; j < CJ; ++j) {
                const int i = i0 + CG * j + cg;
                v[j] = p.inp[ok && i < p.cin ? base + i * ihw : 0];
            }
#pragma unroll
            for (int j = 0; j < CJ; ++j) {
                const int i = i0 + CG * j + cg;
                ish[(t * WT + CG * j + cg) * PITCH + lk] = ok && i < p.cin ? v[j] : 0.f;
            }
        }
        __syncthreads();
#pragma unroll 4
        for (int q = 0; q < KC / 2; ++q) {
            const float ga = gsh[l32 * PITCH + 2 * q + hi];  // A[o = lane & 31][k = lane >> 5]
#pragma unroll
            for (int t = 0; t < TAPS; ++t) {
                const float xb = ish[(t * WT + l32) * PITCH + 2 * q + hi];  // B[k = lane >> 5][i = lane & 31]
                acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(ga, xb, acc[t], 0, 0, 0);
            }
        }
        __syncthreads();
    }

    // D: column (lane & 31) = input channel, row (r & 3) + 8 (r >> 2) + 4 (lane >> 5) = output channel
    float* dst = p.out + (int64_t)split * p.split_stride;
    const int i = i0 + l32;
    if (i < p.cin) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int o = o0 + (r & 3) + 8 * (r >> 2) + 4 * hi;
            if (o < p.cout) {
#pragma unroll
                for (int t = 0; t < TAPS; ++t) dst[(o * p.cin + i) * TAPS + t] = acc[t][r];
            }
        }
    }
}

// dw[e] = partial[0][e] + partial[1][e] + ... in split order
__global__ __launch_bounds__(256) void wgrad_reduce_kernel(const float* part, int nsplit, int64_t split_stride,
                                                           float* dw, int total) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= total) return;
    float s = part[e];
    int k = 1;
    for (; k + 16 <= nsplit; k += 16) {  // 16 loads in flight, added in split order
        float v[16];
#pragma unroll
        for (int j = 0; j < 16; ++j) v[j] = part[(k + j) * split_stride + e];
#pragma unroll
        for (int j = 0; j < 16; ++j) s += v[j];
    }
    for (; k < nsplit; ++k) s += part[k * split_stride + e];
    dw[e] = s;
}

struct Plan {
    int tiles, itiles, chunks, chunks_per_split, nsplit;
};

// Host planner: split the K chunks so that tiles x splits reaches kWavesPerCu waves per CU, each split keeping at
// least kMinChunks chunks.  The weight gradient sums over the batch, so the planning batch (smc_set_plan_batch,
// which keeps a per-image result independent of its shard) does not enter.
Plan make_plan(int n, int cin, int cout, int out_h, int out_w) {
    Plan pl{};
    pl.itiles = (int)smc::ceil_div(cin, WT);
    pl.tiles = pl.itiles * (int)smc::ceil_div(cout, WT);
    const int64_t K = (int64_t)n * out_h * out_w;
    pl.chunks = (int)smc::ceil_div(K, KC);
    const int64_t target = (int64_t)kWavesPerCu * smc::device_cu_count();
    int64_t want = std::max<int64_t>(1, smc::ceil_div(target, pl.tiles));
    want = std::min<int64_t>(want, std::max<int64_t>(1, pl.chunks / kMinChunks));
    want = std::min<int64_t>(want, 65535);
    pl.chunks_per_split = (int)smc::ceil_div(pl.chunks, want);
    pl.nsplit = (int)smc::ceil_div(pl.chunks, pl.chunks_per_split);
    return pl;
}

bool shape_ok(int n, int cin, int cout, int in_h, int in_w, int out_h, int out_w, int kh, int kw, int stride) {
    return n >= 1 && cin >= 1 && cout >= 1 && in_h >= 1 && in_w >= 1 && out_h >= 1 && out_w >= 1 && kh == kw &&
           (kh == 1 || kh == 3) && (stride == 1 || stride == 2) &&
           (int64_t)n * cin * in_h * in_w * 4 < (1LL << 31) && (int64_t)n * cout * out_h * out_w * 4 < (1LL << 31) &&
           (int64_t)cin * cout * kh * kw * 4 < (1LL << 31);
}

thread_local int g_last_nsplit = 0;

}  // namespace

SMC_API int64_t smc_conv_wgrad_workspace_size(int n, int cin, int cout, int in_h, int in_w, int out_h, int out_w,
                                              int kh, int kw, int stride) {
    if (!shape_ok(n, cin, cout, in_h, in_w, out_h, out_w, kh, kw, stride)) return 0;
    const Plan pl = make_plan(n, cin, cout, out_h, out_w);
    return pl.nsplit > 1 ? (int64_t)pl.nsplit * cout * cin * kh * kw * (int64_t)sizeof(float) : 0;
}

SMC_API int smc_conv_wgrad_last_nsplit(void) { return g_last_nsplit; }

SMC_API int smc_conv_wgrad_f32(const float* inp, int n, int cin, int in_h, int in_w, const float* grad, int cout,
                               int out_h, int out_w, int kh, int kw, int stride, int pad_y, int pad_x, float* dw,
                               float* workspace, int64_t workspace_bytes, void* stream) {
    SMC_CHECK(inp && grad && dw, "smc_conv_wgrad_f32: null pointer");
    SMC_CHECK(n >= 1 && cin >= 1 && cout >= 1 && in_h >= 1 && in_w >= 1 && out_h >= 1 && out_w >= 1,
              "smc_conv_wgrad_f32: bad shape (n=%d cin=%d cout=%d in %dx%d out %dx%d)", n, cin, cout, in_h, in_w,
              out_h, out_w);
    SMC_CHECK(kh == kw && (kh == 1 || kh == 3), "smc_conv_wgrad_f32: kernel %dx%d (only 1x1 and 3x3)", kh, kw);
    SMC_CHECK(stride == 1 || stride == 2, "smc_conv_wgrad_f32: stride %d (only 1 and 2)", stride);
    SMC_CHECK(pad_y >= 0 && pad_y <= 2 && pad_x >= 0 && pad_x <= 2, "smc_conv_wgrad_f32: padding (%d, %d) outside 0..2",
              pad_y, pad_x);
    SMC_CHECK(in_h + 2 * pad_y >= kh && in_w + 2 * pad_x >= kw &&
                  out_h == (in_h + 2 * pad_y - kh) / stride + 1 && out_w == (in_w + 2 * pad_x - kw) / stride + 1,
              "smc_conv_wgrad_f32: out shape %dx%d inconsistent with in %dx%d, kernel %d, stride %d, padding (%d, %d)",
              out_h, out_w, in_h, in_w, kh, stride, pad_y, pad_x);
    SMC_CHECK((int64_t)n * cin * in_h * in_w * 4 < (1LL << 31) && (int64_t)n * cout * out_h * out_w * 4 < (1LL << 31) &&
                  (int64_t)cin * cout * kh * kw * 4 < (1LL << 31),
              "smc_conv_wgrad_f32: inp, grad and dw must each be below 2 GiB (32-bit offsets)");
    const Plan pl = make_plan(n, cin, cout, out_h, out_w);
    const int taps = kh * kw;
    const int64_t total = (int64_t)cout * cin * taps;
    const int64_t need = pl.nsplit > 1 ? (int64_t)pl.nsplit * total * (int64_t)sizeof(float) : 0;
    SMC_CHECK(need == 0 || (workspace && workspace_bytes >= need),
              "smc_conv_wgrad_f32: workspace of %lld bytes needed (got %lld)", (long long)need,
              (long long)(workspace ? workspace_bytes : 0));
    hipStream_t st = smc::as_stream(stream);
    WgradParams p{};
    p.inp = inp;
    p.grad = grad;
    p.out = pl.nsplit > 1 ? workspace : dw;
    p.split_stride = total;
    p.n = n; p.cin = cin; p.cout = cout; p.in_h = in_h; p.in_w = in_w; p.out_h = out_h; p.out_w = out_w;
    p.stride = stride; p.pad_y = pad_y; p.pad_x = pad_x;
    p.K = n * out_h * out_w;
    p.chunks = pl.chunks;
    p.chunks_per_split = pl.chunks_per_split;
    p.itiles = pl.itiles;
    const dim3 grid((unsigned)pl.tiles, (unsigned)pl.nsplit);
    if (taps == 9)
        hipLaunchKernelGGL(conv_wgrad_kernel<9>, grid, dim3(64), 0, st, p);
    else
        hipLaunchKernelGGL(conv_wgrad_kernel<1>, grid, dim3(64), 0, st, p);
    int rc = smc::check_launch("smc_conv_wgrad_f32");
    if (rc != SMC_OK) return rc;
    if (pl.nsplit > 1) {
        hipLaunchKernelGGL(wgrad_reduce_kernel, dim3((unsigned)smc::ceil_div(total, 256)), dim3(256), 0, st, workspace,
                           pl.nsplit, total, dw, (int)total);
        rc = smc::check_launch("smc_conv_wgrad_f32 (reduction)");
        if (rc != SMC_OK) return rc;
    }
    g_last_nsplit = pl.nsplit;
    return SMC_OK;
}
