// The up=2 modconv layer in one launch for gfx950 (smc_modconv_up2_f32): the split-bf16 4-phase transposed conv of
// convt_x3_kernel, then the 4x4 [1,3,3,1] FIR (pad 1, gain 4) and the modconv epilogue of blur_act_v4 applied to the
// workgroup's T tile in LDS.  The raw transposed-conv output T = [n, cout, 2h+1, 2w+1] never reaches HBM: the
// two-launch form writes and re-reads it (538 MB at r = 1024, batch 4, against 0.8 GB of compulsory traffic).
//
// Tiling.  y[i, j] needs T rows i-1 .. i+2 and columns j-1 .. j+2 (T zero outside [0, 2h] x [0, 2w]), and a
// super-pixel (a, b) of the conv yields the 2x2 block T[2a .. 2a+1][2b .. 2b+1], so a workgroup owns a 2-D tile of
// PA x 18 super-pixels of ONE image (per-sample tiles, so the per-sample style-scaled weight planes apply as in
// convt_x3_kernel) = a 2 PA x 36 T tile whose first row / column is even, and produces the (2 PA - 4) x 32 outputs
// y[YR ti .. YR ti + YR - 1][32 tj .. 32 tj + 31] from tile rows 1 .. 2 PA - 1 and tile columns 1 .. 35.
// Neighbouring tiles overlap by the halo (4 rows and 4 columns, not 3: tile origins must stay even); every y row
// segment a workgroup stores is one aligned 128-B line.
//   TM = 1 (128 positions, 64 output channels): PA = 7,  T 14 x 36 -> y 10 x 32, 320 / 504  = 63.5 % useful
//   TM = 2 (256 positions, 32 output channels): PA = 14, T 28 x 36 -> y 24 x 32, 768 / 1008 = 76.2 % useful
// Super-pixels outside the image stage zeros for every shift (the K loop's bounds check), so their T values are +0
// without a branch -- and so are T row 2h+1 / column 2w+1 of the super-pixels a = h / b = w, whose only taps read x
// row h / column w.
//
// Arithmetic.  The K loop is convt_x3_kernel's own (convt_x3_loop: same channel-chunk order, shifts, split and
// MFMA order), so a T value is the same bits wherever it is computed, halo duplicates included.  Every output is
// then the __fmaf_rn chain of fir_block (from 0, jy ascending, jx ascending within it) with the std_taps constants,
// and the epilogue expression of blur_act_v4 (smc::modact2): y and u are bit-identical to the two-launch path where
// that path runs unsplit.
//
// LDS.  The T tile of one epilogue pass, [32 / TM channels][2 PA][36] fp32 with the channel pitch padded to 32 banks
// mod 64 (the FIR's ds_read_b128 of two channels' 8 column groups are conflict-free), is 68 / 66 KiB and overlays the
// staging ring (64 KiB at TO = 2, 56 KiB at TM = 2), dead after the K loop: two workgroups per CU.  A pass covers
// 32 / TM channels of one of the wave's TO blocks: TO TM = 2 passes either way.
#include "convt_x3.hpp"
#include "fir_epi.hpp"

namespace {

using namespace smc::cg;

constexpr int kPB = 18, kTC = 2 * kPB, kYC = kTC - 4;   // super-pixel / T / y columns of a tile

template <int TM>
struct FirTile {
    static constexpr int PA = 7 * TM;            // super-pixel rows
    static constexpr int TR = 2 * PA;            // T rows
    static constexpr int YR = TR - 4;            // y rows
    static constexpr int CH = 32 / TM;           // channels per epilogue pass
    static constexpr int RT = YR / TM;           // y rows per FIR thread (TM row groups of threads)
    static constexpr int CHS = TM == 1 ? 544 : 1056;   // floats between two channels' T tiles in LDS
    static constexpr int BYTES = CH * CHS * 4;
    static_assert(PA * kPB <= 128 * TM && CHS >= TR * kTC && CHS % 64 == 32 && kYC == 32 && YR % TM == 0 &&
                      CH * 8 * TM == NT, "tile geometry");
};

template <bool V4>
__device__ __forceinline__ void st_row(float* p, const float (&v)[4], bool hi) {
    if (V4) {
        typedef float f32x4 __attribute__((ext_vector_type(4)));
        __builtin_nontemporal_store(f32x4{v[0], v[1], v[2], v[3]}, reinterpret_cast<f32x4*>(p));
    } else {
        smc::st_f2<true>(p, make_float2(v[0], v[1]));
        if (hi) smc::st_f2<true>(p + 2, make_float2(v[2], v[3]));
    }
}

// TO: 32-channel blocks per wave (cout = 32 TO), TM: 32-position blocks per wave (128 TM positions per workgroup);
// grid.x = n x nty x ntx tiles, XCD-swizzled.
// V4: y_w % 4 == 0 and 16-B aligned y / u planes (one dwordx4 store per thread and row)
template <int TO, int TM, bool V4>
__global__ __launch_bounds__(NT, 2) void convt_x3_fir_kernel(GemmParams p, ConvTTaps tt, int nty, int ntx) {
    typedef ConvTX3<1, 4, TO, TM> C;
    typedef FirTile<TM> F;
    constexpr int LDSB = C::RING > F::BYTES ? C::RING : F::BYTES;
    __shared__ __attribute__((aligned(16))) char smem[LDSB];

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    // XCD-aware bijective tile order (see conv_gemm_lds_kernel): an XCD takes a contiguous run of tiles, column
    // tiles fastest, so the halo re-reads of x hit its L2
    const int nwg = gridDim.x, orig = blockIdx.x;
    const int xcd = orig % 8, q8 = nwg / 8, r8 = nwg % 8;
    const int wgid = (xcd < r8 ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8) + orig / 8;
    const int tps = nty * ntx;
    const int nb = wgid / tps;                 // the workgroup's image (grid.x = n * tps exactly)
    const int trem = wgid - nb * tps;
    const int ti = trem / ntx, tj = trem - ti * ntx;
    const int a0 = ti * (F::YR / 2) - 1, b0 = tj * (kYC / 2) - 1;

    // the staging lane's super-pixel (convt_x3_loop: position (wave % NCH) * 64 + lane)
    const int ms = (wave % C::NCH) * 64 + lane;
    const int spa = ms / kPB;
    f32x16 acc[4][TO][TM];
    convt_x3_loop<1, 4, TO, TM>(p, tt, smem, ms < F::PA * kPB, nb, a0 + spa, b0 + (ms - spa * kPB), nb, 0, 0,
                                4 * (p.cin / C::BKT), acc);

    // the accumulators' super-pixels (block column (wave * TM + j) * 32 + l32), registers walk the block's 32 channels
    const int kh = lane >> 5, l32 = lane & 31;
    float* T = reinterpret_cast<float*>(smem);
    float* tw[TM];
    bool tv[TM];
#pragma unroll
    for (int j = 0; j < TM; ++j) {
        const int me = (wave * TM + j) * 32 + l32;
        const int epa = me / kPB, epb = me - epa * kPB;
        tv[j] = me < F::PA * kPB;
        tw[j] = T + (2 * epa) * kTC + 2 * epb;
    }

    // FIR: thread = (row group, channel of the pass, column group) -> RT rows x 4 columns of y
    const int q = tid & 7, chl = (tid >> 3) % F::CH, rg = (tid >> 3) / F::CH;
    const int ox = tj * kYC + 4 * q, oy0 = ti * F::YR + rg * F::RT;
    const bool lo = ox < p.y_w, hi = ox + 2 < p.y_w;   // y_w is even
    const float* tr = T + chl * F::CHS + (rg * F::RT) * kTC + 4 * q;
    const float nstr = p.noise_strength ? *p.noise_strength : 1.f;
    const bool lrelu_clamp = smc::modact_lrelu_clamp(p.act, p.alpha, p.clamp);
    float tp[4][4];
    smc::std_taps<4, 4>(tp);
    const int64_t plane = (int64_t)p.y_h * p.y_w;

#pragma unroll
    for (int pass = 0; pass < TO * TM; ++pass) {
        const int i = pass / TM, cp = pass % TM;   // the wave's block i, channels cp * CH .. + CH - 1 of it
        __syncthreads();  // every wave is done with the ring (pass 0) / with the previous pass's tile
#pragma unroll
        for (int j = 0; j < TM; ++j) {
            if (!tv[j]) continue;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                if (r / (16 / TM) != cp) continue;   // register r: channel (r & 3) + 8 (r >> 2) + 4 kh of the block
                float* t0 = tw[j] + ((r & 3) + 8 * ((r >> 2) % (4 / TM)) + 4 * kh) * F::CHS;
                *reinterpret_cast<float2*>(t0) = make_float2(acc[0][i][j][r], acc[1][i][j][r]);
                *reinterpret_cast<float2*>(t0 + kTC) = make_float2(acc[2][i][j][r], acc[3][i][j][r]);
            }
        }
        __syncthreads();
        const int o = i * 32 + cp * F::CH + chl;
        const int64_t nc = (int64_t)nb * p.cout + o;
        const float dv = p.d ? p.d[nc] : 1.f;
        const float bv = p.bias ? p.bias[o] : 0.f;
        // the rows' noise before the first store (vmcnt counts loads and stores alike)
        float nz[F::RT][4];
#pragma unroll
        for (int yi = 0; yi < F::RT; ++yi) {
            nz[yi][0] = nz[yi][1] = nz[yi][2] = nz[yi][3] = 0.f;
            if (p.noise && lo) {
                const float* np = p.noise + nb * p.noise_nstride + (int64_t)min(oy0 + yi, p.y_h - 1) * p.y_w + ox;
                const float2 n0 = *reinterpret_cast<const float2*>(np);
                nz[yi][0] = n0.x * nstr;
                nz[yi][1] = n0.y * nstr;
                if (hi) {
                    const float2 n1 = *reinterpret_cast<const float2*>(np + 2);
                    nz[yi][2] = n1.x * nstr;
                    nz[yi][3] = n1.y * nstr;
                }
            }
        }
        float out[F::RT][4];
#pragma unroll
        for (int yi = 0; yi < F::RT; ++yi) out[yi][0] = out[yi][1] = out[yi][2] = out[yi][3] = 0.f;
#pragma unroll
        for (int r = 1; r < F::RT + 4; ++r) {  // the row group's tile row r; its y row yi reads rows yi + 1 .. yi + 4
            const float4 v0 = *reinterpret_cast<const float4*>(tr + r * kTC);
            const float4 v1 = *reinterpret_cast<const float4*>(tr + r * kTC + 4);
            const float v[8] = {v0.x, v0.y, v0.z, v0.w, v1.x, v1.y, v1.z, v1.w};
#pragma unroll
            for (int yi = 0; yi < F::RT; ++yi) {
                const int jy = r - 1 - yi;
                if (jy < 0 || jy >= 4) continue;
#pragma unroll
                for (int j = 0; j < 4; ++j)
#pragma unroll
                    for (int jx = 0; jx < 4; ++jx) out[yi][j] = __fmaf_rn(tp[jy][jx], v[1 + j + jx], out[yi][j]);
            }
            if (r < 4) continue;
            const int yi = r - 4;  // complete with this tile row
            const int oy = oy0 + yi;
            if (!lo || oy >= p.y_h) continue;
            const int64_t pix = nc * plane + (int64_t)oy * p.y_w + ox;
            if (p.u_save) st_row<V4>(p.u_save + pix, out[yi], hi);
            const float2 qa = smc::modact2(make_float2(out[yi][0], out[yi][1]), dv, make_float2(nz[yi][0], nz[yi][1]),
                                           bv, lrelu_clamp, p.act, p.alpha, p.gain, p.clamp);
            const float2 qb = smc::modact2(make_float2(out[yi][2], out[yi][3]), dv, make_float2(nz[yi][2], nz[yi][3]),
                                           bv, lrelu_clamp, p.act, p.alpha, p.gain, p.clamp);
            const float yv[4] = {qa.x, qa.y, qb.x, qb.y};
            st_row<V4>(p.y + pix, yv, hi);
        }
    }
}

enum Up2Route { U_NONE = 0, U_FIR_12, U_FIR_12_V4, U_FIR_21, U_FIR_21_V4, kUp2Routes };
constexpr const char* kUp2Names[] = {"none", "convt_x3_fir_kernel<1,2,false>", "convt_x3_fir_kernel<1,2,true>",
                                     "convt_x3_fir_kernel<2,1,false>", "convt_x3_fir_kernel<2,1,true>"};
static_assert(sizeof(kUp2Names) / sizeof(kUp2Names[0]) == kUp2Routes, "one name per route");
thread_local int g_up2_route = U_NONE;

}  // namespace

SMC_API int smc_modconv_up2_supported(int n, int cin, int cout, int h, int w) {
    return smc::convt_up2_shape_ok(n, cin, cout, h, w) ? 1 : 0;
}

SMC_API int smc_modconv_up2_plan_ok(int n, int cin, int cout, int h, int w) {
    return smc::convt_up2_shape_ok(n, cin, cout, h, w) && smc::convt_up2_plan_ok(n, cin, cout, h, w) ? 1 : 0;
}

SMC_API int smc_modconv_up2_last_route(void) { return g_up2_route; }

SMC_API const char* smc_modconv_up2_route_name(int route) {
    return route >= 0 && route < kUp2Routes ? kUp2Names[route] : nullptr;
}

SMC_API int smc_modconv_up2_f32(const float* x, int n, int cin, int h, int w, float* y, int cout,
                                const smc_conv_phase* phases, int nphases, const float* s_in, const float* f, int fh,
                                int fw, float fgain, const smc_conv_epilogue* epi, float* workspace,
                                int64_t workspace_bytes, void* stream) {
    g_up2_route = U_NONE;
    SMC_CHECK(x && y && phases && epi && n >= 1 && h >= 1 && w >= 1, "smc_modconv_up2_f32: bad args");
    if (f || fh != 4 || fw != 4 || fgain != 4.f) {
        smc::set_error("smc_modconv_up2_f32: only the built-in [1,3,3,1] filter (f = NULL, 4x4) at gain 4");
        return SMC_ERR_UNSUPPORTED;
    }
    SMC_CHECK(epi->mode == SMC_EPI_MODACT && !epi->residual && !epi->scale_c && !epi->grad_from_y,
              "smc_modconv_up2_f32: the MODACT epilogue only");
    const uintptr_t al = (uintptr_t)y | (uintptr_t)epi->u_save | (uintptr_t)epi->noise;
    SMC_CHECK(al % 8 == 0 && epi->noise_nstride % 2 == 0, "smc_modconv_up2_f32: y / u_save / noise need 8-B alignment");
    GemmParams p{};
    ConvTTaps tt{};
    int rc = smc::convt_up2_prepare(x, n, cin, h, w, y, cout, phases, nphases, s_in, workspace, workspace_bytes, stream, &p,
                                    &tt);
    if (rc != SMC_OK) return rc;
    p.y = y; p.y_h = 2 * h; p.y_w = 2 * w;
    p.mode = epi->mode; p.d = epi->d; p.noise = epi->noise; p.noise_nstride = epi->noise_nstride;
    p.noise_strength = epi->noise_strength; p.bias = epi->bias; p.act = epi->act; p.alpha = epi->alpha;
    p.gain = epi->gain; p.clamp = epi->clamp; p.u_save = epi->u_save;
    p.nsplit = 1;
    const int yr = cout == 32 ? FirTile<2>::YR : FirTile<1>::YR;
    const int nty = (int)smc::ceil_div(p.y_h, yr), ntx = (int)smc::ceil_div(p.y_w, kYC);
    const int64_t nwg = (int64_t)n * nty * ntx;
    SMC_CHECK(nwg < (1LL << 31), "smc_modconv_up2_f32: too many tiles");
    const bool v4 = p.y_w % 4 == 0 && ((uintptr_t)y | (uintptr_t)epi->u_save) % 16 == 0;
    const dim3 g((unsigned)nwg);
    hipStream_t st = smc::as_stream(stream);
    if (cout == 32 && v4) { g_up2_route = U_FIR_12_V4; hipLaunchKernelGGL((convt_x3_fir_kernel<1, 2, true>), g, dim3(NT), 0, st, p, tt, nty, ntx); }
    else if (cout == 32) { g_up2_route = U_FIR_12; hipLaunchKernelGGL((convt_x3_fir_kernel<1, 2, false>), g, dim3(NT), 0, st, p, tt, nty, ntx); }
    else if (v4) { g_up2_route = U_FIR_21_V4; hipLaunchKernelGGL((convt_x3_fir_kernel<2, 1, true>), g, dim3(NT), 0, st, p, tt, nty, ntx); }
    else { g_up2_route = U_FIR_21; hipLaunchKernelGGL((convt_x3_fir_kernel<2, 1, false>), g, dim3(NT), 0, st, p, tt, nty, ntx); }
    return smc::check_launch("smc_modconv_up2_f32");
}
