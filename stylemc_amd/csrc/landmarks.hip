// Face-landmark stack (MTCNN detector + MobileNet-GDConv 68-point regressor), the three kernels the library lacked:
//
//   smc_dwconv_f32               depthwise convolution with a folded BatchNorm and ReLU6: the 3x3 pad-1 stride-1/2 layers
//                                of MobileNetV2's inverted residuals, and the "global" depthwise layer linear7 of
//                                MobileNet_GDConv (7x7 on a 7x7 plane) / MobileNet_GDConv_56 (2x2 on 2x2)
//                                (mobilenet_facial.py:55-85 of the reference).
//   smc_maxpool2d_f32            ceil-mode max-pool, (k, stride) = (2, 2) or (3, 2): the MTCNN pools (MTCNN/get_nets.py).
//   smc_crop_bilinear_norm_f32   denorm_img + crop + bilinear resize + normalise of one face box per image
//                                (find_direction.py:44-46,76-79, warp_images.py:100-103) in one launch.
//
// All fp32, no atomics, every output element summed by one thread (or one fixed 16-lane butterfly) in a fixed order:
// bit-identical from run to run.  Plane offsets are 64-bit.  No LDS.
#include <algorithm>

#include "common.hpp"

namespace {

// ------------------------------------------------------------------------------------------------ depthwise 3x3
// A thread owns 4 adjacent output columns of one plane and walks down R output rows with the three input rows of its
// strip in registers (a rolling window: stride 1 loads one new row per output row, stride 2 two).  Work items are
// numbered strip-fastest across all planes, so a workgroup covers as many small planes as fit 256 threads (a 14x14
// plane is 4 strips wide) and neighbouring lanes read neighbouring columns.
// VEC: the rows are 16-byte aligned (w % 4 == 0 at stride 1, w % 8 == 0 at stride 2, aligned bases): the centre of a
// strip is loaded as float4 (two at stride 2) and the outputs stored as one float4.
constexpr int kDwCols = 4;

template <int STRIDE, bool VEC>
__device__ __forceinline__ void dw_load_row(const float* __restrict__ xp, int iy, int H, int W, int ix0,
                                            float (&r)[3 * STRIDE + 3]) {
    constexpr int NIN = 3 * STRIDE + 3;
    if (iy < 0 || iy >= H) {
#pragma unroll
        for (int i = 0; i < NIN; ++i) r[i] = 0.f;
        return;
    }
    const float* row = xp + (int64_t)iy * W;
    if (VEC) {
        r[0] = ix0 >= 0 ? row[ix0] : 0.f;
        const float4 v = *reinterpret_cast<const float4*>(row + ix0 + 1);
        r[1] = v.x; r[2] = v.y; r[3] = v.z; r[4] = v.w;
        if constexpr (STRIDE == 1) {
            r[5] = ix0 + 5 < W ? row[ix0 + 5] : 0.f;
        } else {
            const float4 u = *reinterpret_cast<const float4*>(row + ix0 + 5);
            r[5] = u.x; r[6] = u.y; r[7] = u.z; r[8] = u.w;
        }
    } else {
#pragma unroll
        for (int i = 0; i < NIN; ++i) {
            const int ix = ix0 + i;
            r[i] = (ix >= 0 && ix < W) ? row[ix] : 0.f;
        }
    }
}

__device__ __forceinline__ float dw_epilogue(float acc, float sc, float sh, int relu6) {
    const float z = __fmaf_rn(acc, sc, sh);
    return relu6 ? fminf(fmaxf(z, 0.f), 6.f) : z;
}

template <int STRIDE, bool VEC>
__global__ __launch_bounds__(256) void dwconv3x3_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                        const float* __restrict__ scale,
                                                        const float* __restrict__ shift, float* __restrict__ y, int C,
                                                        int H, int W, int OH, int OW, int strips, int segs, int R,
                                                        int relu6, int64_t total) {
    constexpr int NIN = 3 * STRIDE + 3;
    const int64_t item = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (item >= total) return;
    const int strip = (int)(item % strips);
    const int64_t t = item / strips;
    const int seg = (int)(t % segs);
    const int64_t plane = t / segs;
    const int c = (int)(plane % C);
    const float* xp = x + plane * ((int64_t)H * W);
    float* yp = y + plane * ((int64_t)OH * OW);
    float k[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) k[i] = w[(int64_t)c * 9 + i];
    const float sc = scale ? scale[c] : 1.f, sh = shift ? shift[c] : 0.f;
    const int ox0 = strip * kDwCols, ix0 = ox0 * STRIDE - 1;
    const int oy0 = seg * R, oy1 = min(oy0 + R, OH);
    float ra[NIN], rb[NIN], rc[NIN];
    if (STRIDE == 1) {
        dw_load_row<STRIDE, VEC>(xp, oy0 - 1, H, W, ix0, ra);
        dw_load_row<STRIDE, VEC>(xp, oy0, H, W, ix0, rb);
    } else {
        dw_load_row<STRIDE, VEC>(xp, 2 * oy0 - 1, H, W, ix0, ra);
    }
    for (int oy = oy0; oy < oy1; ++oy) {
        if (STRIDE == 1) {
            dw_load_row<STRIDE, VEC>(xp, oy + 1, H, W, ix0, rc);
        } else {
            dw_load_row<STRIDE, VEC>(xp, 2 * oy, H, W, ix0, rb);
            dw_load_row<STRIDE, VEC>(xp, 2 * oy + 1, H, W, ix0, rc);
        }
        float o[kDwCols];
#pragma unroll
        for (int j = 0; j < kDwCols; ++j) {
            float acc = k[0] * ra[j * STRIDE];
            acc = __fmaf_rn(k[1], ra[j * STRIDE + 1], acc);
            acc = __fmaf_rn(k[2], ra[j * STRIDE + 2], acc);
#pragma unroll
            for (int i = 0; i < 3; ++i) acc = __fmaf_rn(k[3 + i], rb[j * STRIDE + i], acc);
#pragma unroll
            for (int i = 0; i < 3; ++i) acc = __fmaf_rn(k[6 + i], rc[j * STRIDE + i], acc);
            o[j] = dw_epilogue(acc, sc, sh, relu6);
        }
        float* yrow = yp + (int64_t)oy * OW + ox0;
        if (VEC) {
            *reinterpret_cast<float4*>(yrow) = make_float4(o[0], o[1], o[2], o[3]);
        } else {
#pragma unroll
            for (int j = 0; j < kDwCols; ++j)
                if (ox0 + j < OW) yrow[j] = o[j];
        }
#pragma unroll
        for (int i = 0; i < NIN; ++i) {
            ra[i] = STRIDE == 1 ? rb[i] : rc[i];
            if (STRIDE == 1) rb[i] = rc[i];
        }
    }
}

// ------------------------------------------------------------------------------------------------ global depthwise
// One k x k dot product per plane (k*k <= 64): 16 lanes per plane, lane l sums elements l, l + 16, l + 32, l + 48 in
// that order, then a xor butterfly (8, 4, 2, 1) whose additions commute, so every lane holds the same sum.
__global__ __launch_bounds__(256) void dwconv_global_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                            const float* __restrict__ scale,
                                                            const float* __restrict__ shift, float* __restrict__ y,
                                                            int C, int kk, int relu6, int64_t planes) {
    const int64_t plane = (int64_t)blockIdx.x * 16 + (threadIdx.x >> 4);
    const int lane = threadIdx.x & 15;
    const bool live = plane < planes;
    const int c = live ? (int)(plane % C) : 0;
    float acc = 0.f;
    if (live) {
        const float* xp = x + plane * kk;
        const float* wp = w + (int64_t)c * kk;
        for (int e = lane; e < kk; e += 16) acc = __fmaf_rn(wp[e], xp[e], acc);
    }
    acc += __shfl_xor(acc, 8, 16);
    acc += __shfl_xor(acc, 4, 16);
    acc += __shfl_xor(acc, 2, 16);
    acc += __shfl_xor(acc, 1, 16);
    if (live && lane == 0) y[plane] = dw_epilogue(acc, scale ? scale[c] : 1.f, shift ? shift[c] : 0.f, relu6);
}

const char* dw_shape_error(int n, int c, int in_h, int in_w, int k, int stride, int pad) {
    if (n < 1 || c < 1 || in_h < 1 || in_w < 1) return "n, c, in_h, in_w must be >= 1";
    if ((int64_t)n * c > 0x7fffffff || in_h > 32768 || in_w > 32768) return "more than 2^31 - 1 planes or a side above 32768";
    if (pad == 1) {
        if (k != 3) return "pad 1 needs k = 3";
        if (stride != 1 && stride != 2) return "stride must be 1 or 2";
        return nullptr;
    }
    if (pad != 0) return "pad must be 1 (3x3) or 0 (global form)";
    if (k < 2 || k > 8) return "global form needs 2 <= k <= 8";
    if (k != in_h || k != in_w) return "global form needs k == in_h == in_w";
    if (stride != 1) return "global form has stride 1";
    return nullptr;
}

// Output rows per thread: the longest walk that still leaves a 256-thread workgroup of items for each of the 256 CUs
// (the choice moves no sum: every output is one thread's fixed chain whatever R is).
int dw_rows_per_thread(int64_t planes, int strips, int OH) {
    for (int R = 8; R > 1; R /= 2)
        if (planes * strips * smc::ceil_div(OH, R) >= (int64_t)256 * 256) return R;
    return 1;
}

// ------------------------------------------------------------------------------------------------ max-pool
__global__ __launch_bounds__(256) void maxpool_kernel(const float* __restrict__ x, float* __restrict__ y, int H, int W,
                                                      int OH, int OW, int k, int stride, int64_t total) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= total) return;
    const int ox = (int)(e % OW);
    const int64_t t = e / OW;
    const int oy = (int)(t % OH);
    const int64_t plane = t / OH;
    const float* xp = x + plane * ((int64_t)H * W);
    const int y0 = oy * stride, x0 = ox * stride;
    const int y1 = min(y0 + k, H), x1 = min(x0 + k, W);  // ceil mode: the last window is clipped at the border
    float m = xp[(int64_t)y0 * W + x0];
    for (int yy = y0; yy < y1; ++yy)
        for (int xx = x0; xx < x1; ++xx) {
            const float v = xp[(int64_t)yy * W + xx];
            if (v > m || v != v) m = v;  // NaN propagates, as in torch
        }
    y[e] = m;
}

inline int pool_out(int in, int k, int stride) { return (in - k + stride - 1) / stride + 1; }

// ------------------------------------------------------------------------------------------------ crop + resize
struct CropNorm {
    float mean[3], std[3];
    int denorm, norm;
};

// One thread per output pixel, all three channels (they share the source cell and weights).  The source coordinate
// is torch's fp32 arithmetic for align_corners = False: scale = (float)in / out, src = max(scale * (dst + 0.5) - 0.5, 0),
// i0 = (int)src, i1 = i0 + (i0 < in - 1), l1 = src - i0, l0 = 1 - l1.  A box is clipped to the image here (it lives on
// the device, the host cannot check it), so no read can leave the plane.
__global__ __launch_bounds__(256) void crop_bilinear_norm_kernel(const float* __restrict__ img,
                                                                 const int* __restrict__ boxes, float* __restrict__ out,
                                                                 int H, int W, int S, CropNorm cn, int64_t total) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= total) return;
    const int ox = (int)(e % S);
    const int64_t t = e / S;
    const int oy = (int)(t % S);
    const int64_t n = t / S;
    const int bx1 = min(max(boxes[n * 4 + 0], 0), W - 1), by1 = min(max(boxes[n * 4 + 1], 0), H - 1);
    const int bx2 = min(max(boxes[n * 4 + 2], bx1 + 1), W), by2 = min(max(boxes[n * 4 + 3], by1 + 1), H);
    const int cw = bx2 - bx1, ch = by2 - by1;
    const float sx = (float)cw / (float)S, sy = (float)ch / (float)S;
    const float fx = fmaxf(__fsub_rn(__fmul_rn(sx, (float)ox + 0.5f), 0.5f), 0.f);
    const float fy = fmaxf(__fsub_rn(__fmul_rn(sy, (float)oy + 0.5f), 0.5f), 0.f);
    const int x0 = min((int)fx, cw - 1), y0 = min((int)fy, ch - 1);
    const int x1 = x0 + (x0 < cw - 1 ? 1 : 0), y1 = y0 + (y0 < ch - 1 ? 1 : 0);
    const float lx1 = fx - (float)x0, lx0 = 1.f - lx1, ly1 = fy - (float)y0, ly0 = 1.f - ly1;
    const int64_t plane = (int64_t)H * W;
    const int64_t o00 = (int64_t)(by1 + y0) * W + bx1 + x0, o01 = (int64_t)(by1 + y0) * W + bx1 + x1;
    const int64_t o10 = (int64_t)(by1 + y1) * W + bx1 + x0, o11 = (int64_t)(by1 + y1) * W + bx1 + x1;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float* p = img + (n * 3 + c) * plane;
        float a = p[o00], b = p[o01], cc = p[o10], d = p[o11];
        if (cn.denorm) {
            // denorm_img: clamp(x * 127.5 + 128, 0, 255), the product and the sum rounded separately as torch's two ops are
            a = fminf(fmaxf(__fadd_rn(__fmul_rn(a, 127.5f), 128.f), 0.f), 255.f);
            b = fminf(fmaxf(__fadd_rn(__fmul_rn(b, 127.5f), 128.f), 0.f), 255.f);
            cc = fminf(fmaxf(__fadd_rn(__fmul_rn(cc, 127.5f), 128.f), 0.f), 255.f);
            d = fminf(fmaxf(__fadd_rn(__fmul_rn(d, 127.5f), 128.f), 0.f), 255.f);
        }
        const float v = ly0 * (lx0 * a + lx1 * b) + ly1 * (lx0 * cc + lx1 * d);
        out[((n * 3 + c) * S + oy) * (int64_t)S + ox] = cn.norm ? (v / 255.f - cn.mean[c]) / cn.std[c] : v;
    }
}

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

}  // namespace

SMC_API int smc_dwconv_supported(int n, int c, int in_h, int in_w, int k, int stride, int pad) {
    return dw_shape_error(n, c, in_h, in_w, k, stride, pad) == nullptr ? 1 : 0;
}

SMC_API int smc_dwconv_f32(const float* x, int n, int c, int in_h, int in_w, const float* w, int k, int stride, int pad,
                           const float* scale_c, const float* shift_c, int act, float* y, void* stream) {
    const char* err = dw_shape_error(n, c, in_h, in_w, k, stride, pad);
    SMC_CHECK(!err, "smc_dwconv_f32: %s (n %d c %d h %d w %d k %d stride %d pad %d)", err ? err : "", n, c, in_h, in_w, k,
              stride, pad);
    SMC_CHECK(act == SMC_DW_ACT_LINEAR || act == SMC_DW_ACT_RELU6, "smc_dwconv_f32: bad act %d", act);
    SMC_CHECK(x && w && y, "smc_dwconv_f32: null pointer");
    hipStream_t st = smc::as_stream(stream);
    const int64_t planes = (int64_t)n * c;
    const int relu6 = act == SMC_DW_ACT_RELU6;
    if (pad == 0) {
        hipLaunchKernelGGL(dwconv_global_kernel, dim3((unsigned)smc::ceil_div(planes, 16)), dim3(256), 0, st, x, w,
                           scale_c, shift_c, y, c, k * k, relu6, planes);
        return smc::check_launch("dwconv global");
    }
    const int OH = (in_h + 2 - 3) / stride + 1, OW = (in_w + 2 - 3) / stride + 1;
    const int strips = (int)smc::ceil_div(OW, kDwCols);
    const int R = dw_rows_per_thread(planes, strips, OH);
    const int segs = (int)smc::ceil_div(OH, R);
    const int64_t total = planes * strips * segs;
    const int64_t blocks = smc::ceil_div(total, 256);
    SMC_CHECK(blocks <= 0x7fffffff, "smc_dwconv_f32: more than 2^31 - 1 workgroups");
    const bool vec = in_w % (4 * stride) == 0 && aligned16(x) && aligned16(y);
    const dim3 grid((unsigned)blocks), block(256);
#define SMC_DW_LAUNCH(S, V)                                                                                          \
    hipLaunchKernelGGL((dwconv3x3_kernel<S, V>), grid, block, 0, st, x, w, scale_c, shift_c, y, c, in_h, in_w, OH, OW, \
                       strips, segs, R, relu6, total)
    if (stride == 1) {
        if (vec) SMC_DW_LAUNCH(1, true);
        else SMC_DW_LAUNCH(1, false);
    } else {
        if (vec) SMC_DW_LAUNCH(2, true);
        else SMC_DW_LAUNCH(2, false);
    }
#undef SMC_DW_LAUNCH
    return smc::check_launch("dwconv 3x3");
}

SMC_API int smc_maxpool2d_f32(const float* x, int64_t planes, int in_h, int in_w, int k, int stride, float* y,
                              void* stream) {
    SMC_CHECK((k == 2 || k == 3) && stride == 2, "smc_maxpool2d_f32: (k, stride) = (%d, %d), have (2, 2) and (3, 2)", k,
              stride);
    SMC_CHECK(planes >= 1 && in_h >= k && in_w >= k, "smc_maxpool2d_f32: bad shape (planes %lld, %d x %d, k %d)",
              (long long)planes, in_h, in_w, k);
    SMC_CHECK(planes <= 0x7fffffff && in_h <= 32768 && in_w <= 32768,
              "smc_maxpool2d_f32: more than 2^31 - 1 planes or a side above 32768");
    SMC_CHECK(x && y, "smc_maxpool2d_f32: null pointer");
    const int OH = pool_out(in_h, k, stride), OW = pool_out(in_w, k, stride);
    const int64_t total = planes * OH * OW;
    const int64_t blocks = smc::ceil_div(total, 256);
    SMC_CHECK(blocks <= 0x7fffffff, "smc_maxpool2d_f32: more than 2^31 - 1 workgroups");
    hipLaunchKernelGGL(maxpool_kernel, dim3((unsigned)blocks), dim3(256), 0, smc::as_stream(stream), x, y, in_h, in_w,
                       OH, OW, k, stride, total);
    return smc::check_launch("maxpool2d");
}

SMC_API int smc_crop_bilinear_norm_f32(const float* img, int n, int in_h, int in_w, const int* boxes, int out_size,
                                       int denorm, const float* mean3, const float* std3, float* out, void* stream) {
    SMC_CHECK(n >= 1 && in_h >= 1 && in_w >= 1 && out_size >= 1, "smc_crop_bilinear_norm_f32: bad shape");
    SMC_CHECK(in_h <= 32768 && in_w <= 32768 && out_size <= 32768, "smc_crop_bilinear_norm_f32: a side above 32768");
    SMC_CHECK(img && boxes && out, "smc_crop_bilinear_norm_f32: null pointer");
    SMC_CHECK((mean3 == nullptr) == (std3 == nullptr), "smc_crop_bilinear_norm_f32: mean and std go together (null pointer)");
    CropNorm cn{};
    cn.denorm = denorm != 0;
    cn.norm = mean3 != nullptr;
    for (int c = 0; cn.norm && c < 3; ++c) {
        SMC_CHECK(std3[c] != 0.f, "smc_crop_bilinear_norm_f32: std[%d] is 0", c);
        cn.mean[c] = mean3[c];
        cn.std[c] = std3[c];
    }
    const int64_t total = (int64_t)n * out_size * out_size;
    const int64_t blocks = smc::ceil_div(total, 256);
    SMC_CHECK(blocks <= 0x7fffffff, "smc_crop_bilinear_norm_f32: more than 2^31 - 1 workgroups");
    hipLaunchKernelGGL(crop_bilinear_norm_kernel, dim3((unsigned)blocks), dim3(256), 0, smc::as_stream(stream), img,
                       boxes, out, in_h, in_w, out_size, cn, total);
    return smc::check_launch("crop_bilinear_norm");
}
