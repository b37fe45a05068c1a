// Launch report of the memory-bound companion kernels (modconv_aux.hip, torgb.hip): smc_modconv_aux_last_route and
// friends.  One row per kernel instantiation those two files can launch.  SMC_AUXK_<id> is the kernel exactly as its
// launch names it: SMC_AUX_LAUNCH(id, ...) launches those tokens and the route table stringifies the same tokens, so a
// route's name and the kernel it ran cannot differ.  A record only: no launch decision reads it.
#pragma once
#include "common.hpp"

#define SMC_AUXK_EPILOGUE epilogue_kernel
#define SMC_AUXK_BLUR_GENERIC blur_act_kernel
#define SMC_AUXK_BLUR_FAST blur_act_fast<4,4>
#define SMC_AUXK_BLUR_V4 blur_act_v4<4,4,kBlurTPB,kBlurNT>
#define SMC_AUXK_BLUR_V4_STD blur_act_v4<4,4,kBlurTPB,kBlurNT,true>
#define SMC_AUXK_BLUR_BWD_V4_U blur_act_bwd_v4<4,4,false>
#define SMC_AUXK_BLUR_BWD_V4_U_STD blur_act_bwd_v4<4,4,false,true>
#define SMC_AUXK_BLUR_BWD_V4_Y blur_act_bwd_v4<4,4,true>
#define SMC_AUXK_BLUR_BWD_V4_Y_STD blur_act_bwd_v4<4,4,true,true>
#define SMC_AUXK_BLUR_BWD_V2_U blur_act_bwd_fast<4,4,true,false>
#define SMC_AUXK_BLUR_BWD_V2_Y blur_act_bwd_fast<4,4,true,true>
#define SMC_AUXK_BLUR_BWD_S_U blur_act_bwd_fast<4,4,false,false>
#define SMC_AUXK_BLUR_BWD_S_Y blur_act_bwd_fast<4,4,false,true>
#define SMC_AUXK_DEMOD demod_kernel
#define SMC_AUXK_ACT_BWD_V4_U act_bwd_vec4_kernel<false>
#define SMC_AUXK_ACT_BWD_V4_Y act_bwd_vec4_kernel<true>
#define SMC_AUXK_ACT_BWD_U act_bwd_kernel<false>
#define SMC_AUXK_ACT_BWD_Y act_bwd_kernel<true>
#define SMC_AUXK_CHANNEL_DOT_V4 channel_dot_v4_kernel
#define SMC_AUXK_CHANNEL_DOT channel_dot_kernel
#define SMC_AUXK_DEMOD_BWD demod_bwd_kernel
#define SMC_AUXK_TORGB_FWD_SMALL torgb_fwd_small_kernel
#define SMC_AUXK_TORGB_FWD_VEC torgb_fwd_kernel<true>
#define SMC_AUXK_TORGB_FWD torgb_fwd_kernel<false>
#define SMC_AUXK_TORGB_BWD_SMALL torgb_bwd_small_kernel
#define SMC_AUXK_TORGB_BWD_VEC torgb_bwd_kernel<true>
#define SMC_AUXK_TORGB_BWD torgb_bwd_kernel<false>
#define SMC_AUXK_TORGB_ACT_BWD_VEC torgb_act_bwd_kernel<true>
#define SMC_AUXK_TORGB_ACT_BWD torgb_act_bwd_kernel<false>

#define SMC_AUX_ROUTES(X)                                                                                        \
    X(EPILOGUE) X(BLUR_GENERIC) X(BLUR_FAST) X(BLUR_V4) X(BLUR_V4_STD)                                            \
    X(BLUR_BWD_V4_U) X(BLUR_BWD_V4_U_STD) X(BLUR_BWD_V4_Y) X(BLUR_BWD_V4_Y_STD)                                   \
    X(BLUR_BWD_V2_U) X(BLUR_BWD_V2_Y) X(BLUR_BWD_S_U) X(BLUR_BWD_S_Y)                                             \
    X(DEMOD) X(ACT_BWD_V4_U) X(ACT_BWD_V4_Y) X(ACT_BWD_U) X(ACT_BWD_Y) X(CHANNEL_DOT_V4) X(CHANNEL_DOT)           \
    X(DEMOD_BWD) X(TORGB_FWD_SMALL) X(TORGB_FWD_VEC) X(TORGB_FWD) X(TORGB_BWD_SMALL) X(TORGB_BWD_VEC) X(TORGB_BWD) \
    X(TORGB_ACT_BWD_VEC) X(TORGB_ACT_BWD)

namespace smc {

enum AuxRoute : int {
    AUX_NONE = 0,
#define SMC_AUX_ENUM(id) AUX_##id,
    SMC_AUX_ROUTES(SMC_AUX_ENUM)
#undef SMC_AUX_ENUM
    AUX_COUNT
};

// (modconv_aux.hip) begin: an entry point was entered -- route "none", no flags, split 1; set: its launch site
void aux_route_begin();
void aux_route_set(int route);
void aux_route_flag(int flag);
void aux_route_nsplit(int nsplit);

}  // namespace smc

#define SMC_AUX_LAUNCH(id, grid, st, ...)                                             \
    do {                                                                              \
        smc::aux_route_set(smc::AUX_##id);                                            \
        hipLaunchKernelGGL((SMC_AUXK_##id), grid, dim3(256), 0, st, __VA_ARGS__);     \
    } while (0)
