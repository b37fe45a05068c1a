// e4e / pSp encoder heads on gfx950 (encoder4editing/models/encoders/psp_encoders.py:34-55,95-121,173-200 and
// helpers.py:123-140 of the reference): the kernels no synthesis or IR-SE50 kernel is shaped for.
//
//   smc_conv_s2_grouped_f32  G independent 3x3 stride-2 pad-1 convolutions (cin -> cout) in one launch, each over its
//                            own (or a shared) input and its own weights, y = lrelu(acc + bias, alpha).  The 18
//                            "map2style" heads are chains of these on planes from 64x64 down to 1x1 at a batch of one
//                            photograph: M = n*oh*ow output pixels is at most a few hundred, so the work is streaming
//                            9.4 MB of weights per conv.  Per group the conv is a GEMM on the exact-fp32 MFMA
//                            (v_mfma_f32_32x32x2_f32) with M = n*oh*ow, N = cout, K = taps*cin; the grid is
//                            (N tile x M tile, group, K split), and where tiles x groups cannot fill the chip K is
//                            split across workgroups, each writing a partial plane that a second kernel sums in split
//                            order (no atomics: bit-identical from run to run).
//   smc_upsample_add_f32     y = bilinear(x -> size of lat, align_corners) + lat, the FPN's _upsample_add.
//
// Layout: fp32 NCHW; weights [G][tap][cin][cout] for the taps the caller lists (it drops the taps that only ever
// touch padding: 2x2 -> 1x1 keeps 4 of 9, 1x1 -> 1x1 keeps 1, which is also the heads' final EqualLinear).
#include <algorithm>

#include "common.hpp"

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int KC = 16;        // input channels per K chunk (one tap)
constexpr int NT = 128;       // output channels per workgroup: 4 waves x 32
constexpr int kCus = 256;     // planning target (gfx950); the plan is a pure function of the shapes
constexpr int kWgPerCu = 4;   // workgroups per CU the split-K plan aims for (weight streaming: loads in flight)
constexpr int kMinChunks = 4; // K chunks a split keeps at least

struct GroupedParams {
    const float* x;
    const float* wk;
    const float* bias;
    float* out;                // y (nsplit == 1) or the partial planes
    int64_t x_sample_stride, x_group_stride;
    int64_t split_stride;      // floats between partial planes (= G*n*cout*oh*ow)
    unsigned long long taps;   // 4 bits per listed tap: ky*3 + kx
    int n, cin, cout, h, w, oh, ow, M;
    int cchunks;               // cin / KC
    int chunks, chunks_per_split, mtiles, nsplit;
    float alpha;
};

// One workgroup: MB*32 output pixels x 128 output channels of one group over one K split.  Each wave owns 32 output
// channels and MB pixel blocks; A = weights [k][cout] (rows = cout), B = gathered input [k][pixel] (columns =
// pixels, so a store instruction writes 32 consecutive pixels of one channel).  The next chunk's global loads are
// issued before the current chunk's MFMAs and written to LDS after them.
template <int MB>
__global__ __launch_bounds__(256) void conv_s2_grouped_kernel(GroupedParams p) {
    constexpr int PIX = 32 * MB;
    constexpr int CSTEP = 256 / PIX;      // threads along channels in the input gather
    constexpr int NLD = KC / CSTEP;       // gathered elements per thread and chunk
    __shared__ float wsh[KC * NT];
    __shared__ float xsh[KC * PIX];
    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const int l32 = lane & 31, hi = lane >> 5;
    const int nt = blockIdx.x / p.mtiles;
    const int mt = blockIdx.x - nt * p.mtiles;
    const int g = blockIdx.y;
    const int split = blockIdx.z;
    const int c_begin = split * p.chunks_per_split;
    const int c_end = min(p.chunks, c_begin + p.chunks_per_split);
    const int ohw = p.oh * p.ow, hw = p.h * p.w;

    // input gather: this thread's pixel and first channel
    const int gp = tid % PIX, gc = tid / PIX;
    const int m = mt * PIX + gp;
    const bool m_ok = m < p.M;
    const int mm = m_ok ? m : 0;
    const int smp = mm / ohw;
    const int rem = mm - smp * ohw;
    const int oy = rem / p.ow, ox = rem - oy * p.ow;
    const float* xg = p.x + (int64_t)g * p.x_group_stride + (int64_t)smp * p.x_sample_stride;
    // weight tile: 2 float4 per thread: rows wr and wr + 8, 4 columns at wc
    const int wr = tid >> 5, wc = (tid & 31) * 4;
    const int co_w = nt * NT + wc;
    const bool w_ok = co_w < p.cout;  // cout % 32 == 0: a float4 is inside or outside as a whole
    const float* wg = p.wk + (int64_t)g * (p.chunks * (int64_t)KC) * p.cout + (w_ok ? co_w : 0);

    float4 wv[2];
    float xv[NLD];
    auto load = [&](int c) {
        const int ti = c / p.cchunks;
        const int c0 = (c - ti * p.cchunks) * KC;
        const int t = (int)((p.taps >> (4 * ti)) & 15ull);
        const int iy = 2 * oy - 1 + t / 3, ix = 2 * ox - 1 + t % 3;
        const bool ok = m_ok && iy >= 0 && iy < p.h && ix >= 0 && ix < p.w;
        const int off = ok ? iy * p.w + ix : 0;
#pragma unroll
        for (int j = 0; j < NLD; ++j) {
            // masked elements load an element that is in bounds and are replaced by 0: unconditional loads
            const float v = xg[(int64_t)(c0 + gc + CSTEP * j) * hw + off];
            xv[j] = ok ? v : 0.f;
        }
        const float* wp = wg + (int64_t)c * KC * p.cout;
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const float4 v = *reinterpret_cast<const float4*>(wp + (int64_t)(wr + 8 * j) * p.cout);
            wv[j] = w_ok ? v : make_float4(0.f, 0.f, 0.f, 0.f);
        }
    };
    auto stage = [&]() {
#pragma unroll
        for (int j = 0; j < NLD; ++j) xsh[(gc + CSTEP * j) * PIX + gp] = xv[j];
#pragma unroll
        for (int j = 0; j < 2; ++j) *reinterpret_cast<float4*>(&wsh[(wr + 8 * j) * NT + wc]) = wv[j];
    };

    f32x16 acc[MB];
#pragma unroll
    for (int b = 0; b < MB; ++b)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[b][r] = 0.f;

    const int co0 = nt * NT + wave * 32;
    const bool wave_ok = co0 < p.cout;
    if (c_begin < c_end) load(c_begin);
    for (int c = c_begin; c < c_end; ++c) {
        stage();
        __syncthreads();
        if (c + 1 < c_end) load(c + 1);
        if (wave_ok) {
#pragma unroll
            for (int q = 0; q < KC / 2; ++q) {
                const float a = wsh[(2 * q + hi) * NT + wave * 32 + l32];  // A[cout = lane & 31][k = lane >> 5]
#pragma unroll
                for (int b = 0; b < MB; ++b) {
                    const float xb = xsh[(2 * q + hi) * PIX + 32 * b + l32];  // B[k = lane >> 5][pixel = lane & 31]
                    acc[b] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, xb, acc[b], 0, 0, 0);
                }
            }
        }
        __syncthreads();
    }

    // D: column (lane & 31) = pixel, row (r & 3) + 8 (r >> 2) + 4 (lane >> 5) = output channel
    if (!wave_ok) return;
    float* dst = p.out + (int64_t)split * p.split_stride;
#pragma unroll
    for (int b = 0; b < MB; ++b) {
        const int mo = mt * PIX + 32 * b + l32;
        if (mo >= p.M) continue;
        const int s = mo / ohw;
        const int pr = mo - s * ohw;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int co = co0 + (r & 3) + 8 * (r >> 2) + 4 * hi;
            float v = acc[b][r];
            if (p.nsplit == 1) {
                v += p.bias ? p.bias[g * p.cout + co] : 0.f;
                v = v > 0.f ? v : v * p.alpha;
            }
            dst[(((int64_t)g * p.n + s) * p.cout + co) * ohw + pr] = v;
        }
    }
}

// y[e] = lrelu(partial[0][e] + partial[1][e] + ... + bias, alpha): the partials added in split order
__global__ __launch_bounds__(256) void grouped_reduce_kernel(const float* part, int nsplit, int64_t split_stride,
                                                             const float* bias, float alpha, float* y, int total,
                                                             int ohw, int cout, int n) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= total) return;
    float s = part[e];
    int k = 1;
    for (; k + 8 <= nsplit; k += 8) {  // 8 loads in flight, added in split order
        float v[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = part[(k + j) * split_stride + e];
#pragma unroll
        for (int j = 0; j < 8; ++j) s += v[j];
    }
    for (; k < nsplit; ++k) s += part[k * split_stride + e];
    const int ch = e / ohw;          // (g*n + sample)*cout + co
    const int co = ch % cout;
    const int g = ch / (cout * n);
    s += bias ? bias[g * cout + co] : 0.f;
    y[e] = s > 0.f ? s : s * alpha;
}

struct Plan {
    int mb, mtiles, ntiles, chunks, chunks_per_split, nsplit;
};

Plan make_plan(int groups, int n, int cin, int cout, int h, int w, int ntaps) {
    Plan pl{};
    const int64_t M = (int64_t)n * ((h - 1) / 2 + 1) * ((w - 1) / 2 + 1);
    pl.ntiles = (int)smc::ceil_div(cout, NT);
    pl.chunks = ntaps * (cin / KC);
    // A split writes and re-reads one partial plane (8 bytes per output); the splits are capped so that this traffic
    // stays below half the weight bytes (4 * taps * cin per output channel and group), and at kMinChunks per split.
    const int64_t cap = std::max<int64_t>(1, std::min<int64_t>((int64_t)ntaps * cin / (4 * M), pl.chunks / kMinChunks));
    // The largest pixel tile (most MFMAs per weight element read from LDS) whose tiles, times the splits allowed,
    // still give every CU a workgroup; 32 pixels otherwise.  A tile that M fills less than half is not considered.
    int64_t base = 0;
    for (pl.mb = 4; pl.mb >= 1; pl.mb >>= 1) {
        pl.mtiles = (int)smc::ceil_div(M, 32 * pl.mb);
        base = (int64_t)pl.mtiles * pl.ntiles * groups;
        if (pl.mb == 1 || (M > 16 * pl.mb && base * cap >= kCus)) break;
    }
    // tiles that give every CU a workgroup are not split; below that the launch is weight streaming and K is split
    // until kWgPerCu workgroups per CU are pulling weights
    const int64_t want = std::min(cap, base >= kCus ? 1 : smc::ceil_div((int64_t)kCus * kWgPerCu, base));
    pl.chunks_per_split = (int)smc::ceil_div(pl.chunks, want);
    pl.nsplit = (int)smc::ceil_div(pl.chunks, pl.chunks_per_split);
    return pl;
}

const char* shape_error(int groups, int n, int cin, int cout, int h, int w) {
    if (groups < 1 || groups > 65535) return "groups outside 1..65535";
    if (n < 1 || h < 1 || w < 1) return "n, h, w must be >= 1";
    if (cin < KC || cin % KC) return "cin must be a multiple of 16";
    if (cout < 32 || cout % 32) return "cout must be a multiple of 32";
    const int64_t oh = (h - 1) / 2 + 1, ow = (w - 1) / 2 + 1;
    const int64_t lim = (int64_t)1 << 29;  // floats in 2 GiB
    if ((int64_t)groups * n * cin * h * w >= lim) return "input of 2 GiB or more";
    if ((int64_t)groups * n * cout * oh * ow >= lim) return "output of 2 GiB or more";
    if ((int64_t)groups * 9 * cin * cout >= lim) return "weights of 2 GiB or more";
    return nullptr;
}

template <int MB>
void launch_grouped(const GroupedParams& p, const Plan& pl, int groups, hipStream_t st) {
    hipLaunchKernelGGL(conv_s2_grouped_kernel<MB>, dim3(pl.mtiles * pl.ntiles, groups, pl.nsplit), dim3(256), 0, st, p);
}

// 4 consecutive output columns per thread (V = 4: ow % 4 == 0, 16-byte loads of lat and stores of y) or one
template <int V>
__global__ __launch_bounds__(256) void upsample_add_kernel(const float* x, const float* lat, float* y, int planes,
                                                           int ih, int iw, int oh, int ow, int total /* / V */) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= total) return;
    const int owv = ow / V;
    const int xo = (e % owv) * V;
    const int t = e / owv;
    const int yo = t % oh;
    const int pl = t / oh;
    // align_corners: src = dst * (in - 1) / (out - 1), split exactly into an integer cell and a remainder
    const int dy = oh > 1 ? oh - 1 : 1, dx = ow > 1 ? ow - 1 : 1;
    const int ny = oh > 1 ? yo * (ih - 1) : 0;
    const int y0 = ny / dy;
    const float ly = (float)(ny - y0 * dy) / (float)dy;
    const int y1 = min(y0 + 1, ih - 1);
    const float* r0 = x + ((int64_t)pl * ih + y0) * iw;
    const float* r1 = x + ((int64_t)pl * ih + y1) * iw;
    const int64_t o = ((int64_t)pl * oh + yo) * ow + xo;
    float res[V];
#pragma unroll
    for (int j = 0; j < V; ++j) {
        const int nx = ow > 1 ? (xo + j) * (iw - 1) : 0;
        const int x0 = nx / dx;
        const float lx = (float)(nx - x0 * dx) / (float)dx;
        const int x1 = min(x0 + 1, iw - 1);
        const float top = r0[x0] * (1.f - lx) + r0[x1] * lx;
        const float bot = r1[x0] * (1.f - lx) + r1[x1] * lx;
        res[j] = top * (1.f - ly) + bot * ly;
    }
    if (V == 4) {
        const float4 l = *reinterpret_cast<const float4*>(lat + o);
        *reinterpret_cast<float4*>(y + o) = make_float4(res[0] + l.x, res[1] + l.y, res[2] + l.z, res[3] + l.w);
    } else {
#pragma unroll
        for (int j = 0; j < V; ++j) y[o + j] = res[j] + lat[o + j];
    }
}

}  // namespace

SMC_API int smc_conv_s2_grouped_supported(int groups, int n, int cin, int cout, int h, int w) {
    return shape_error(groups, n, cin, cout, h, w) == nullptr ? 1 : 0;
}

SMC_API int64_t smc_conv_s2_grouped_workspace_size(int groups, int n, int cin, int cout, int h, int w, int ntaps) {
    if (shape_error(groups, n, cin, cout, h, w) || ntaps < 1 || ntaps > 9) return -1;
    const Plan pl = make_plan(groups, n, cin, cout, h, w, ntaps);
    if (pl.nsplit == 1) return 0;
    const int64_t total = (int64_t)groups * n * cout * ((h - 1) / 2 + 1) * ((w - 1) / 2 + 1);
    return total * pl.nsplit * (int64_t)sizeof(float);
}

SMC_API int smc_conv_s2_grouped_f32(const float* x, int64_t x_sample_stride, int64_t x_group_stride, int groups, int n,
                                    int cin, int h, int w, const float* wk, const int* taps, int ntaps,
                                    const float* bias, float alpha, float* y, int cout, float* workspace,
                                    int64_t workspace_bytes, void* stream) {
    const char* err = shape_error(groups, n, cin, cout, h, w);
    SMC_CHECK(!err, "smc_conv_s2_grouped_f32: %s (G %d n %d cin %d cout %d h %d w %d)", err ? err : "", groups, n, cin,
              cout, h, w);
    SMC_CHECK(taps && ntaps >= 1 && ntaps <= 9, "smc_conv_s2_grouped_f32: %d taps (1..9)", ntaps);
    unsigned long long code = 0;
    for (int t = 0; t < ntaps; ++t) {
        SMC_CHECK(taps[t] >= 0 && taps[t] <= 8 && (t == 0 || taps[t] > taps[t - 1]),
                  "smc_conv_s2_grouped_f32: taps must be ky*3 + kx in 0..8, ascending");
        code |= (unsigned long long)taps[t] << (4 * t);
    }
    SMC_CHECK(x && wk && y, "smc_conv_s2_grouped_f32: null pointer");
    const int64_t plane = (int64_t)cin * h * w;
    SMC_CHECK(x_sample_stride >= plane && (x_group_stride == 0 || x_group_stride >= plane),
              "smc_conv_s2_grouped_f32: strides smaller than one [cin][h][w] block");
    SMC_CHECK((n - 1) * x_sample_stride + (groups - 1) * x_group_stride + plane < ((int64_t)1 << 29),
              "smc_conv_s2_grouped_f32: strided input spans 2 GiB or more");
    SMC_CHECK((reinterpret_cast<uintptr_t>(wk) & 15) == 0, "smc_conv_s2_grouped_f32: weights must be 16-byte aligned");
    const Plan pl = make_plan(groups, n, cin, cout, h, w, ntaps);
    GroupedParams p{};
    p.x = x; p.wk = wk; p.bias = bias;
    p.x_sample_stride = x_sample_stride; p.x_group_stride = x_group_stride;
    p.taps = code;
    p.n = n; p.cin = cin; p.cout = cout; p.h = h; p.w = w;
    p.oh = (h - 1) / 2 + 1; p.ow = (w - 1) / 2 + 1;
    p.M = n * p.oh * p.ow;
    p.cchunks = cin / KC;
    p.chunks = pl.chunks; p.chunks_per_split = pl.chunks_per_split; p.mtiles = pl.mtiles; p.nsplit = pl.nsplit;
    p.alpha = alpha;
    const int64_t total = (int64_t)groups * p.M * cout;
    p.split_stride = total;
    if (pl.nsplit > 1) {
        SMC_CHECK(workspace && workspace_bytes >= total * pl.nsplit * (int64_t)sizeof(float),
                  "smc_conv_s2_grouped_f32: workspace too small (%lld bytes needed)",
                  (long long)(total * pl.nsplit * (int64_t)sizeof(float)));
        p.out = workspace;
    } else {
        p.out = y;
    }
    hipStream_t st = smc::as_stream(stream);
    if (pl.mb == 4) launch_grouped<4>(p, pl, groups, st);
    else if (pl.mb == 2) launch_grouped<2>(p, pl, groups, st);
    else launch_grouped<1>(p, pl, groups, st);
    int rc = smc::check_launch("conv_s2_grouped");
    if (rc != SMC_OK || pl.nsplit == 1) return rc;
    hipLaunchKernelGGL(grouped_reduce_kernel, dim3((unsigned)smc::ceil_div(total, 256)), dim3(256), 0, st, workspace,
                       pl.nsplit, total, bias, alpha, y, (int)total, p.oh * p.ow, cout, n);
    return smc::check_launch("conv_s2_grouped reduce");
}

SMC_API int smc_upsample_add_f32(const float* x, int64_t planes, int in_h, int in_w, const float* lat, float* y,
                                 int out_h, int out_w, void* stream) {
    SMC_CHECK(planes >= 1 && in_h >= 1 && in_w >= 1 && out_h >= 1 && out_w >= 1, "smc_upsample_add_f32: bad shape");
    SMC_CHECK(planes * in_h * in_w < ((int64_t)1 << 29) && planes * out_h * out_w < ((int64_t)1 << 29),
              "smc_upsample_add_f32: tensor of 2 GiB or more");
    SMC_CHECK((int64_t)out_h * in_h < (1 << 30) && (int64_t)out_w * in_w < (1 << 30), "smc_upsample_add_f32: plane size");
    SMC_CHECK(x && lat && y, "smc_upsample_add_f32: null pointer");
    hipStream_t st = smc::as_stream(stream);
    const bool v4 = out_w % 4 == 0 && ((reinterpret_cast<uintptr_t>(lat) | reinterpret_cast<uintptr_t>(y)) & 15) == 0;
    const int64_t total = planes * out_h * (v4 ? out_w / 4 : out_w);
    if (v4)
        hipLaunchKernelGGL(upsample_add_kernel<4>, dim3((unsigned)smc::ceil_div(total, 256)), dim3(256), 0, st, x, lat, y,
                           (int)planes, in_h, in_w, out_h, out_w, (int)total);
    else
        hipLaunchKernelGGL(upsample_add_kernel<1>, dim3((unsigned)smc::ceil_div(total, 256)), dim3(256), 0, st, x, lat, y,
                           (int)planes, in_h, in_w, out_h, out_w, (int)total);
    return smc::check_launch("upsample_add");
}
