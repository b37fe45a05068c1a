"""The Winograd entry points' host-side predicates (no GPU: the library loads without one) against a Python statement
of the rules include/stylemc_hip.h gives (tests/wino_cases.py), and the case table of tests/test_gpu_wino_routes.py
against those rules -- a table that drifts fails here, before any GPU run."""
import ctypes
import itertools

from stylemc_amd import _hip
from tests import wino_cases as wc

CIN = (0, 4, 8, 12, 16, 24, 64, 128, 136, 256, 512)
COUT = (0, 16, 32, 48, 64, 96, 128, 160, 192, 512)
H = (0, 2, 4, 6, 8, 12, 16, 24, 30, 32, 64, 66)
W = (16, 28, 32, 34, 36, 48, 64, 96, 112, 128, 160, 192, 256)


def test_wino_supported_equals_the_header_rule():
    lib = _hip.load()
    for n, cin, cout, h, w in itertools.product((0, 1, 3), CIN, COUT, H, W):
        assert lib.smc_conv3x3_wino_supported(n, cin, cout, h, w) == wc.wino_supported(n, cin, cout, h, w), \
            (n, cin, cout, h, w)
        assert lib.smc_conv3x3_wino4_supported(n, cin, cout, h, w) == wc.wino4_supported(n, cin, cout, h, w), \
            (n, cin, cout, h, w)
    # the header's example: h = 6, w = 64 meets "h even, w % 4 == 0, w >= 32" and has no kernel
    assert lib.smc_conv3x3_wino_supported(1, 32, 32, 6, 64) == 0
    # the 2 GiB limits (32-bit buffer offsets): input of both, taps of F(4x4)
    assert lib.smc_conv3x3_wino_supported(16, 512, 512, 256, 256) == wc.wino_supported(16, 512, 512, 256, 256) == 0
    assert lib.smc_conv3x3_wino_supported(8, 512, 512, 256, 256) == wc.wino_supported(8, 512, 512, 256, 256) == 1
    assert lib.smc_conv3x3_wino4_supported(16, 512, 512, 256, 256) == wc.wino4_supported(16, 512, 512, 256, 256) == 0
    assert lib.smc_conv3x3_wino4_supported(8, 512, 512, 256, 256) == wc.wino4_supported(8, 512, 512, 256, 256) == 1
    assert lib.smc_conv3x3_wino4_supported(1, 4096, 4096, 8, 64) == wc.wino4_supported(1, 4096, 4096, 8, 64) == 0
    assert lib.smc_conv3x3_wino4_supported(1, 2048, 4096, 8, 64) == wc.wino4_supported(1, 2048, 4096, 8, 64) == 1


def test_wino_workspace_equals_the_header_rule():
    lib = _hip.load()
    assert lib.smc_set_wino_x3(0) == 0   # the split-bf16 mode (its own plane bytes) is off by default
    for n, cin, cout, h, w in itertools.product((1, 2, 3, 4, 16), CIN, COUT, (4, 8, 16, 32, 64), (32, 64, 96, 128)):
        assert lib.smc_conv3x3_wino_workspace_size(n, cin, cout, h, w) == sum(wc.wino_workspace(n, cin, cout, h, w)), \
            (n, cin, cout, h, w)
    # the synthesis plans test_gpu_wino.test_wino_split_plan records
    assert wc.wino_workspace(4, 512, 512, 32, 32) == (2 * 4 * 512 * 32 * 32 * 4, 0)
    assert wc.wino_workspace(2, 512, 512, 32, 32) == (4 * 2 * 512 * 32 * 32 * 4, 0)
    assert wc.wino_workspace(4, 512, 512, 64, 64) == (0, 0)
    assert wc.wino_workspace(2, 32, 32, 32, 32) == (0, 2 * 32 * 16 * 32 * 4)


def test_wino_case_table_follows_the_rules():
    """Every table case is supported; its EXPECTED route, flags and split count are what the restated guards plan;
    each split / fold case gets the workspace its flags imply."""
    lib = _hip.load()
    for c in wc.CASES:
        if c.fam == 4:
            assert lib.smc_conv3x3_wino4_supported(c.n, c.cin, c.cout, c.h, c.w) == 1, c.id
            assert not c.ws
        else:
            assert lib.smc_conv3x3_wino_supported(c.n, c.cin, c.cout, c.h, c.w) == 1, c.id
            assert wc.wino_tc(c.h, c.w) == int(c.id[2:4]), c.id
        name, flags, ns = wc.EXPECTED[c.id]
        assert (name, flags, ns) == wc.planned_route(c), (c.id, wc.planned_route(c))
        if c.fam == 2:
            split, fold = wc.wino_workspace(c.n, c.cin, c.cout, c.h, c.w)
            nb = lib.smc_conv3x3_wino_workspace_size(c.n, c.cin, c.cout, c.h, c.w)
            assert nb == split + fold, c.id
            assert bool(flags & wc.SPLIT) == (c.ws and split > 0) and (ns > 1) == bool(flags & wc.SPLIT), c.id
            if flags & wc.SPLIT:
                assert c.cin >= 128 and split == ns * c.n * c.cout * c.h * c.w * 4, c.id
            if flags & wc.FOLD:
                assert c.style and c.ws and fold == c.n * c.cin * c.cout * 64 and c.cin * c.cout <= 128 * 128, c.id
            elif c.ws and c.style:
                assert fold == 0 and c.cin * c.cout > 128 * 128, c.id
            if not c.ws:   # no workspace passed: neither a split nor a fold may be planned for the launch
                assert flags == 0, c.id
    assert wc.FOLD == _hip.ROUTE_WINO_FOLD and wc.SPLIT == _hip.ROUTE_SPLIT_K


def _form_epilogue(form, h, w):
    """The smc_conv_epilogue of a FORMS entry as the plan query reads it: the scalar fields, and an aligned non-NULL
    placeholder for every operand the form sets (the query reads no memory behind a pointer)."""
    f = wc.FORMS[form]
    e = _hip.ConvEpilogue()
    e.mode = getattr(_hip, "EPI_" + f["mode"])
    e.act, e.alpha, e.gain, e.clamp = (_hip.ACT_CODES[f.get("act", "linear")], f.get("alpha", 0.0), f.get("gain", 1.0),
                                       f.get("clamp", -1.0))
    for field, key in (("d", "d"), ("noise", "noise"), ("noise_strength", "strength"), ("bias", "bias"),
                       ("u_save", "u_save"), ("scale_c", "scale_c"), ("alpha_c", "alpha_c"), ("act_ref", "act_ref"),
                       ("residual", "residual")):
        if f.get(key):
            setattr(e, field, 256)
    e.noise_nstride = h * w if f.get("noise") == "img" else 0
    e.residual_stride = f.get("residual") or 0
    return e


def _library_plan(lib, fam, n, cin, cout, h, w, style, form, nb):
    """(return code, route name, flags, K splits) of smc_conv3x3_wino_plan / smc_conv3x3_wino4_plan."""
    e = _form_epilogue(form, h, w) if isinstance(form, str) else form   # a form's name, an epilogue or None
    epi = ctypes.byref(e) if e is not None else None
    route, flags, ns = ctypes.c_int(-1), ctypes.c_int(-1), ctypes.c_int(-1)
    if fam == 2:
        rc = lib.smc_conv3x3_wino_plan(n, cin, cout, h, w, int(style), epi, nb, ctypes.byref(route),
                                       ctypes.byref(flags), ctypes.byref(ns))
    else:
        rc = lib.smc_conv3x3_wino4_plan(n, cin, cout, h, w, int(style), epi, ctypes.byref(route))
        flags.value, ns.value = 0, 1 if rc == 0 else 0
    return rc, wc.route_name(fam, route.value), flags.value, ns.value


def test_library_plan_reaches_the_recorded_routes():
    """The library's own plan (the host-only query, no device call) of every table case is the (route, flags, K
    splits) recorded from its GPU launch -- with the workspace the size query asks for where the case passes one."""
    lib = _hip.load()
    assert lib.smc_set_wino_x3(0) == 0
    for c in wc.CASES:
        nb = lib.smc_conv3x3_wino_workspace_size(c.n, c.cin, c.cout, c.h, c.w) if c.ws else 0
        rc, name, flags, ns = _library_plan(lib, c.fam, c.n, c.cin, c.cout, c.h, c.w, c.style, c.epi, nb)
        assert rc == 0 and (name, flags, ns) == wc.EXPECTED[c.id], (c.id, rc, name, flags, ns)


def test_library_plan_equals_the_restated_rules():
    """Over the shape grid of the workspace test x style x workspace offered x every epilogue form (and the NULL
    epilogue), the library's plan is what the restated rules give: wino_workspace, wino_nsplit, epilogue_body and the
    naming rule of planned_route."""
    lib = _hip.load()
    assert lib.smc_set_wino_x3(0) == 0
    forms = [None] + list(wc.FORMS)
    checked = 0
    for n, cin, cout, h, w in itertools.product((1, 2, 3, 4, 16), CIN, COUT, (4, 8, 16, 32, 64), (32, 64, 96, 128)):
        ok2, ok4 = wc.wino_supported(n, cin, cout, h, w), wc.wino4_supported(n, cin, cout, h, w)
        if not ok2:
            assert _library_plan(lib, 2, n, cin, cout, h, w, True, None, 0) == (2, "none", 0, 0), (n, cin, cout, h, w)
        if not ok4:
            assert _library_plan(lib, 4, n, cin, cout, h, w, True, None, 0)[:2] == (2, "none"), (n, cin, cout, h, w)
        if not (ok2 or ok4):
            continue
        need = lib.smc_conv3x3_wino_workspace_size(n, cin, cout, h, w)
        epis = {form: _form_epilogue(form, h, w) if form is not None else None for form in forms}
        for form, style, ws in itertools.product(forms, (False, True), (False, True)):
            ek = wc.epilogue_body(form) if form is not None else 0
            if ok2:
                c = wc.Case("grid", 2, n, cin, cout, h, w, form, style, 0, ws)
                # (planned_route reads the form through epilogue_body: NULL is the plain store, EK 0)
                want = wc.planned_route(c._replace(epi=form or "store"))
                got = _library_plan(lib, 2, n, cin, cout, h, w, style, epis[form], need if ws else 0)
                assert got == (0,) + want, (c, got, want)
                if ws and need > 0:   # a workspace one byte short is not used at all
                    short = _library_plan(lib, 2, n, cin, cout, h, w, style, epis[form], need - 1)
                    assert short == (0,) + wc.planned_route(c._replace(epi=form or "store", ws=False)), (c, short)
                checked += 1
            if ok4 and not ws:
                got = _library_plan(lib, 4, n, cin, cout, h, w, style, epis[form], 0)
                assert got == (0, f"wino4_kernel<{1 if style else 2},{ek}>", 0, 1), (n, cin, cout, h, w, form, style)
                checked += 1
    assert checked > 10000


def test_library_plan_in_the_split_bf16_mode():
    """smc_set_wino_x3(1) / (2): the 32 -> 32-channel TC 32 shape with its workspace plans the split-bf16 kernel for the
    MODACT lrelu form (mode 2: also for the linear form), and the fused conv1 + ToRGB launch leaves such a shape to the
    two-launch path.  Without the workspace, with unaligned noise or for another form the fp32 kernel keeps the call."""
    lib = _hip.load()
    shape = (2, 32, 32, 8, 64)
    try:
        for mode in (1, 2):
            lib.smc_set_wino_x3(mode)
            nb = lib.smc_conv3x3_wino_workspace_size(*shape)
            assert nb == 2 * 16 * 3 * 2 * 4 * 16 * 8 * 2   # the planes (96 KB per image) exceed the folded taps
            for style in (False, True):
                assert _library_plan(lib, 2, *shape, style, "modact_lrelu", nb) == (0, "wino_x3r_kernel<1>", 0, 1)
                lin = _library_plan(lib, 2, *shape, style, "modact_linear_bwd", nb)
                assert lin == (0, "wino_x3r_kernel<2>" if mode == 2 else "wino_kernel<32,2,2>",
                               wc.FOLD if style and mode == 1 else 0, 1), (mode, style, lin)
                assert _library_plan(lib, 2, *shape, style, "modact_lrelu", 0) == \
                    (0, f"wino_kernel<32,{1 if style else 2},1>", 0, 1)
            assert _library_plan(lib, 2, *shape, False, "store", nb) == (0, "wino_kernel<32,2,0>", 0, 1)
            e = _form_epilogue("modact_lrelu", 8, 64)
            e.noise = 260   # not 16-B aligned: the fp32 kernel
            route = ctypes.c_int(-1)
            assert lib.smc_conv3x3_wino_plan(*shape, 0, ctypes.byref(e), nb, ctypes.byref(route), None, None) == 0
            assert wc.route_name(2, route.value) == "wino_kernel<32,2,1>"
            assert lib.smc_modconv_conv1_torgb_supported(*shape, 3, None) == 0
            assert lib.smc_modconv_conv1_torgb_workspace_size(*shape) == 0
            assert lib.smc_modconv_conv1_torgb_supported(2, 64, 32, 8, 64, 3, None) == 1   # (cin 64: not that kernel's)
    finally:
        lib.smc_set_wino_x3(0)
    assert lib.smc_modconv_conv1_torgb_supported(*shape, 3, None) == 1
    assert lib.smc_conv3x3_wino_workspace_size(*shape) == sum(wc.wino_workspace(*shape))


def test_wino_case_table_covers_the_issue_list():
    """The K ladder, block geometry, item counts and tap forms the table is meant to hold, per block shape."""
    for g, geo in wc.GEOM.items():
        cs = [c for c in wc.CASES if c.id.startswith(g + "_")]
        step = 8 if geo["fam"] == 2 else 4
        assert {1, 2, 3} <= {c.cin // step for c in cs} and any(c.cin >= 64 for c in cs), g
        assert {(c.h, c.w) for c in cs} >= set(geo["hw"]), g
        assert any(c.n == 3 and c.cout == geo["cout"][2] for c in cs), g
        assert any(c.flip and c.cin != c.cout for c in cs) and any(not c.flip and c.cin != c.cout for c in cs), g
    # 3 x 3 blocks (an interior block with all four halos) and item counts that are no multiple of 8
    assert wc.GEOM["tc16"]["hw"][2] == (24, 96) and wc.GEOM["tc32"]["hw"][2] == (12, 192)
    assert wc.GEOM["f4"]["hw"][2] == (24, 192)
    items = lambda c: c.n * (c.h * c.w // (256 if c.fam == 2 else 512)) * (c.cout // (32 if c.fam == 2 else 64))
    for fam in (2, 4):
        assert any(items(c) % 8 and items(c) > 8 for c in wc.CASES if c.fam == fam)


def test_short_k_entries_are_the_algorithms_error():
    """A case held to the CPU fp32 model instead of TOL has one or two K steps of F(4x4) / one of F(2x2), and the model
    of the same arithmetic -- no kernel involved -- misses TOL on the case's inputs by the recorded figure."""
    for cid, (model, kernel) in wc.SHORT_K.items():
        c = wc.BY_ID[cid]
        assert c.cin in (4, 8), cid
        d = wc.make_inputs(c)
        u64, B = wc.conv64(c, d)
        got = ((wc.model_conv(c, d).double() - u64).abs() / B).max().item()
        assert got > wc.TOL[c.fam], (cid, got)
        assert abs(got - model) <= 0.15 * model, (cid, got, model)   # (the matmul's summation order may differ by host)
        assert wc.TOL[c.fam] < kernel * wc.TOL[c.fam] <= 2 * model, cid


def test_cpu_model_agrees_with_fp64():
    """model_conv() is a convolution: on one case per family it meets the family's bounds against fp64."""
    for cid in ("tc16_modact_lrelu", "tc32_store_flip_k64", "f4_store_flip_k64", "f4_modact_lrelu"):
        c = wc.BY_ID[cid]
        d = wc.make_inputs(c)
        u64, B = wc.conv64(c, d)
        m = wc.model_conv(c, d).double()
        assert ((m - u64).abs() / B).max().item() <= wc.TOL[c.fam], cid
        assert ((m - u64).norm() / u64.norm()).item() <= wc.REL[c.fam], cid


def test_route_names_without_gpu():
    """The route lists are host data: every instantiation the dispatchers can launch (TC 16 and 32: wino_tc() offers no
    64-column block; the register-U split-bf16 kernel), and no other."""
    f2, f4 = wc.route_names(2), wc.route_names(4)
    assert f2[0] == f4[0] == "none"
    want2 = {f"wino_kernel<{tc},{sm},{ek}>" for tc in (16, 32) for sm in (1, 2) for ek in (0, 1, 2, 3)}
    want2 |= {f"wino_x3r_kernel<{ek}>" for ek in (1, 2)}
    assert set(f2[1:]) == want2 and len(f2) == 1 + len(want2)
    assert f4[1:] == [f"wino4_kernel<{sm},{ek}>" for sm in (1, 2) for ek in (0, 1, 2)]
    lib = _hip.load()
    assert lib.smc_conv3x3_wino_route_name(-1) is None and lib.smc_conv3x3_wino_route_name(len(f2)) is None
    assert lib.smc_conv3x3_wino4_route_name(len(f4)) is None
    assert set(wc.EXPECTED[c.id][0] for c in wc.CASES) <= set(f2) | set(f4)
