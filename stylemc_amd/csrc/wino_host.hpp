// Host-side pieces shared by the Winograd entry points (wino.hip: smc_conv3x3_wino_ws_f32 and
// smc_modconv_conv1_torgb_f32; wino4.hip: smc_conv3x3_wino4_f32): the epilogue a call carries -- its checks, its copy
// into the kernel's parameter struct, the epilogue body the kernels compile for it -- and the form of a route table.
#pragma once
#include "common.hpp"

namespace smc {

// The checks on a call's epilogue (`who`: the entry point the message names; u_save is stored in runs of u_align bytes).
inline int check_epilogue(const smc_conv_epilogue& e, const char* who, int u_align) {
    SMC_CHECK(e.mode >= SMC_EPI_STORE && e.mode <= SMC_EPI_AFFINE, "%s: bad epilogue mode %d", who, e.mode);
    SMC_CHECK((e.mode != SMC_EPI_PRELU && e.mode != SMC_EPI_PRELU_GRAD) || e.alpha_c, "%s: PReLU epilogue needs alpha_c",
              who);
    SMC_CHECK(e.mode != SMC_EPI_PRELU_GRAD || e.act_ref, "%s: PRELU_GRAD needs act_ref", who);
    SMC_CHECK(!e.u_save || (reinterpret_cast<uintptr_t>(e.u_save) & (u_align - 1)) == 0, "%s: u_save alignment", who);
    return SMC_OK;
}

// The epilogue fields of WinoParams / Wino4Params.
template <class Params>
void fill_epilogue(Params& p, const smc_conv_epilogue& e) {
    p.mode = e.mode; p.d = e.d; p.noise = e.noise; p.noise_nstride = e.noise_nstride;
    p.noise_strength = e.noise_strength; p.bias = e.bias; p.act = e.act; p.alpha = e.alpha; p.gain = e.gain;
    p.clamp = e.clamp; p.u_save = e.u_save;
    p.ext = epi_ext(&e);
}

// EK, the epilogue body of the Winograd kernels: the synthesis' two MODACT forms have one with the activation fixed
// at compile time (1: lrelu with 0 <= alpha <= 1, gain, clamp >= 0 -- the conv1 forward; 2: linear without a clamp --
// the data gradient); 0: any epilogue through smc::epi_y / epi_ext_apply.  (Neither scale_c nor a NULL operand counts.)
inline int epi_body(const smc_conv_epilogue& e) {
    const bool modact_plain = e.mode == SMC_EPI_MODACT && !e.residual;
    if (modact_plain && e.act == SMC_ACT_LRELU && e.alpha >= 0.f && e.alpha <= 1.f && e.clamp >= 0.f) return 1;
    if (modact_plain && e.act == SMC_ACT_LINEAR && e.clamp < 0.f) return 2;
    return 0;
}

// A route table has one row per kernel instantiation an entry point can launch, written once as `kernel, template
// arguments`: the row's name is those tokens spelled out ("kernel<args>"), its launcher the function they instantiate
// and its key the arguments themselves, by which the plan finds the row (route_of).  So a reported name, the kernel
// that ran and the plan's choice cannot differ.  Row 0 is "none"; the numbers are an index for one build, the names
// the stable identity.  (Rows are written without blanks: the name is their spelling.)
template <class Run>
struct RouteRow {
    const char* name;
    Run run;
    int kern;     // which kernel template (where a table holds two)
    int key[3];   // its template arguments
};
#define SMC_WINO_ROUTE_ROW(kern, ...) {#kern "<" #__VA_ARGS__ ">", &run_##kern<__VA_ARGS__>, K_##kern, {__VA_ARGS__}},

template <class Run, int N>
int route_of(const RouteRow<Run> (&table)[N], int kern, int a, int b = 0, int c = 0) {
    for (int r = 1; r < N; ++r)
        if (table[r].kern == kern && table[r].key[0] == a && table[r].key[1] == b && table[r].key[2] == c) return r;
    return 0;
}

template <class Run, int N>
const char* route_name(const RouteRow<Run> (&table)[N], int route) {
    return route >= 0 && route < N ? table[route].name : nullptr;
}

}  // namespace smc
