"""e4e real-image inversion on the GPU: the grouped stride-2 conv kernel, the FPN upsample-add and the trunk taps
against float64, the whole encoder (both encoder types, grouped and composed heads) against the reference's outputs
(tests/golden/e4e.npz) and the restated module in float64, and the CLI end to end.

Bounds: 2e-5 of max|ref| for the conv + epilogue kernels at K <= 4608 (the project's bound for its conv epilogues,
test_gpu_irse.py; the exact-fp32 MFMA is about 3.5e-7 * sum|a b| at that K); 1e-6 of the max for the element-wise
upsample-add; 1e-4 of max|ref| for IR-SE50 features (test_gpu_irse.py) and for every W+ row.
"""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from stylemc_amd import _hip, e4e_hip, synthetic
from stylemc_amd.encoder4editing.models.encoders import psp_encoders as PE
from tests.golden.e4e_inputs import CASES, ENCODERS, SEED, e4e_input

pytestmark = pytest.mark.gpu
DEV = "cuda"


# ------------------------------------------------------------------------------------------ grouped kernel


def _run_grouped(x_store, x_blocks, ss, gs, W, bias, alpha, n, h, w):
    """x_store: the device tensor the strides address; x_blocks [G][n][cin][h][w]: the same blocks gathered for the
    float64 reference (F.conv2d(stride=2, padding=1) + bias + leaky_relu).  Returns (err / max|ref|, runs equal)."""
    G, cout, cin = W.shape[:3]
    taps = e4e_hip.live_taps(h, w)
    wk = e4e_hip.pack_taps(list(W), taps, DEV)
    taps_c = (ctypes.c_int * len(taps))(*taps)
    oh, ow = (h - 1) // 2 + 1, (w - 1) // 2 + 1
    ys = []
    for _ in range(2):
        y = torch.full((G, n, cout, oh, ow), float("nan"), device=DEV)
        e4e_hip.grouped_conv(x_store, ss, gs, G, n, cin, h, w, wk, taps_c, bias, alpha, y, cout)
        ys.append(y)
    torch.cuda.synchronize()
    ref = torch.stack([F.leaky_relu(F.conv2d(x_blocks[g].double().cpu(), W[g].double().cpu(), bias[g].double().cpu(),
                                             stride=2, padding=1), alpha) for g in range(G)])
    err = (ys[0].double().cpu() - ref).abs().max().item() / ref.abs().max().item()
    return err, torch.equal(ys[0], ys[1])


def _operands(G, n, cin, cout, h, w, seed):
    g = torch.Generator().manual_seed(seed)
    W = (torch.randn(G, cout, cin, 3, 3, generator=g) / (3 * cin ** 0.5)).to(DEV)
    bias = (torch.randn(G, cout, generator=g) * 0.5).to(DEV)
    x = torch.randn(G, n, cin, h, w, generator=g).to(DEV)
    return W, bias, x


GROUPED_CASES = {
    # name: (G, n, cin, cout, h, w, alpha, input form)
    "shared_input": (3, 1, 64, 64, 8, 8, 0.01, "shared"),          # group stride 0
    "split_k": (2, 2, 512, 512, 4, 4, 0.01, "own"),                # per-group input, K split across workgroups
    "taps4": (3, 1, 512, 512, 2, 2, 0.01, "own"),                  # 2x2 -> 1x1: 4 live taps
    "taps1": (3, 1, 512, 512, 1, 1, 0.01, "own"),                  # 1x1 -> 1x1: 1 live tap
    "odd_7x7": (2, 2, 64, 64, 7, 7, 0.01, "own"),
    "odd_5x3": (2, 2, 64, 64, 5, 3, 0.01, "own"),
    "many_groups": (11, 3, 64, 64, 16, 16, 0.01, "own"),           # M = 192: not a power of two, two M tiles, masked rows
    "linear": (18, 2, 512, 512, 1, 1, 1.0, "own"),                 # the final EqualLinear: 1 tap, alpha = 1
    "slices": (3, 2, 64, 64, 8, 8, 0.01, "slices"),                # channel slices of a wider tensor
    # beyond the issue's list: the planner's other pixel tiles and a masked N tile.  The planner (csrc/e4e.hip
    # make_plan) takes the largest tile whose tiles x allowed splits reach 256 workgroups:
    "tile64_split": (16, 1, 256, 256, 16, 12, 0.01, "own"),        # M = 48: 64-pixel tile (32 tiles x 12 splits), masked
    "tile128": (32, 1, 16, 64, 62, 62, 0.01, "shared"),            # M = 961: 128-pixel tiles (8 x 32), no split, masked
    "n_edge": (2, 1, 48, 160, 6, 6, 0.01, "own"),                  # cout = 128 + 32, cin = 3 chunks
}


@pytest.mark.parametrize("name", sorted(GROUPED_CASES))
def test_grouped_conv_vs_fp64(name):
    G, n, cin, cout, h, w, alpha, form = GROUPED_CASES[name]
    W, bias, x = _operands(G, n, cin, cout, h, w, seed=sum(map(ord, name)))
    plane = cin * h * w
    if form == "shared":
        store, blocks, ss, gs = x[0].contiguous(), x[:1].expand(G, -1, -1, -1, -1), plane, 0
    elif form == "own":
        store, blocks, ss, gs = x, x, plane, n * plane
    else:  # [n][16 + G*cin + 16][h][w]: sample stride != G x group stride, first block 16 channels in
        wide = torch.randn(n, G * cin + 32, h, w, device=DEV)
        wide[:, 16:16 + G * cin] = x.permute(1, 0, 2, 3, 4).reshape(n, G * cin, h, w)
        store, blocks, ss, gs = wide.reshape(-1)[16 * h * w:], x, (G * cin + 32) * h * w, plane
    if name == "linear":
        assert e4e_hip.live_taps(h, w) == [4]
    err, same = _run_grouped(store, blocks, ss, gs, W, bias, alpha, n, h, w)
    print(f"{name}: err / max|ref| = {err:.2e}")
    assert same, "two runs differ"
    assert err <= 2e-5, err


def test_grouped_split_regimes_are_the_ones_the_cases_name():
    lib = _hip.load()
    assert lib.smc_conv_s2_grouped_workspace_size(2, 2, 512, 512, 4, 4, 9) > 0     # split_k
    assert lib.smc_conv_s2_grouped_workspace_size(18, 2, 512, 512, 1, 1, 1) > 0    # linear
    assert lib.smc_conv_s2_grouped_workspace_size(16, 1, 256, 256, 16, 12, 9) > 0  # tile64_split
    assert lib.smc_conv_s2_grouped_workspace_size(32, 1, 16, 64, 62, 62, 9) == 0   # tile128: tiles fill the chip


# ------------------------------------------------------------------------------------------ upsample-add


@pytest.mark.parametrize("shape,size", [((2, 16, 4, 4), (8, 8)), ((1, 512, 16, 16), (32, 32)), ((1, 16, 3, 5), (7, 4))])
def test_upsample_add_vs_fp64(shape, size):
    g = torch.Generator().manual_seed(shape[1] + size[0])
    x = torch.randn(*shape, generator=g)
    lat = torch.randn(shape[0], shape[1], *size, generator=g)
    ref = F.interpolate(x.double(), size=size, mode="bilinear", align_corners=True) + lat.double()
    y = e4e_hip.upsample_add(x.to(DEV), lat.to(DEV))
    err = (y.double().cpu() - ref).abs().max().item() / ref.abs().max().item()
    print(f"{shape} -> {size}: err / max = {err:.2e}")
    assert err <= 1e-6, err


# ------------------------------------------------------------------------------------------ encoder


@pytest.fixture(scope="module")
def state_dict():
    net = PE.Encoder4Editing(50, "ir_se", 1024)
    return synthetic.e4e_state_dict(net, seed=SEED)


@pytest.fixture(scope="module")
def fp64(state_dict):
    """float64 CPU yardstick, computed once: the trunk taps at 64 px and the 18 head outputs per fixture case."""
    net = PE.Encoder4Editing(50, "ir_se", 1024).eval().requires_grad_(False)
    net.load_state_dict(state_dict)
    net = net.double()
    out = {}
    with torch.no_grad():
        for key, (n, size) in CASES.items():
            x = e4e_input(n, size).double()
            if key == "64":
                out["taps"] = net.features(x)
            out[key] = torch.stack(net.head_outputs(x), dim=1)
    return out


@pytest.fixture(scope="module")
def nets(state_dict):
    return {name: e4e_hip.build_e4e(state_dict=state_dict, device=DEV, encoder_type=name) for name in ENCODERS}


def test_trunk_taps_vs_fp64(nets, fp64):
    net = nets["Encoder4Editing"]
    n, size = CASES["64"]
    x = e4e_input(n, size).to(DEV)
    got = net.trunk(x, net.packed(size))
    torch.cuda.synchronize()
    assert [tuple(t.shape) for t in got] == [(n, 128, 16, 16), (n, 256, 8, 8), (n, 512, 4, 4)]
    for name, t, ref in zip(("c1", "c2", "c3"), got, fp64["taps"]):
        err = (t.double().cpu() - ref).abs().max().item() / ref.abs().max().item()
        print(f"{name}: err / max|ref| = {err:.2e}")
        assert err <= 1e-4, (name, err)


def _row_err(got, ref):
    """max over W+ rows of (max err of the row / max|ref| of the row)."""
    got, ref = torch.as_tensor(got).double(), torch.as_tensor(ref).double()
    return ((got - ref).abs().amax(dim=(0, 2)) / ref.abs().amax(dim=(0, 2))).max().item()


@pytest.mark.parametrize("grouped", [True, False], ids=["grouped", "composed"])
@pytest.mark.parametrize("key", sorted(CASES))
@pytest.mark.parametrize("name", ENCODERS)
def test_encoder_vs_reference_and_fp64(golden, nets, fp64, monkeypatch, name, key, grouped):
    monkeypatch.setattr(e4e_hip, "GROUPED", grouped)
    n, size = CASES[key]
    w = nets[name](e4e_input(n, size).to(DEV)).cpu()
    assert nets[name].packed(size).grouped == grouped
    assert w.shape == (n, 18, 512)
    e_ref = _row_err(w, golden("e4e.npz")[f"{name}/w{key}"])
    e_64 = _row_err(w, PE.ENCODERS[name].combine(fp64[key]))
    print(f"{name} {key} px {'grouped' if grouped else 'composed'}: row err vs reference {e_ref:.2e}, vs fp64 {e_64:.2e}")
    assert e_ref <= 1e-4 and e_64 <= 1e-4, (e_ref, e_64)


@pytest.mark.parametrize("fine0_gemm", [True, False], ids=["fine0_gemm", "fine0_grouped"])
def test_both_routes_of_the_first_fine_level(nets, fp64, monkeypatch, fine0_gemm):
    """The first fine level as one smc_conv_gemm_f32 call with cout = 11 * 512 (the next level then reads channel
    slices through the strides; the default, by measurement) and as a grouped launch with group stride 0."""
    monkeypatch.setattr(e4e_hip, "GROUPED", True)
    monkeypatch.setattr(e4e_hip, "FINE0_GEMM", fine0_gemm)
    n, size = CASES["64"]
    net = nets["GradualStyleEncoder"]
    w = net(e4e_input(n, size).to(DEV)).cpu()
    pk = net.packed(size)
    assert pk.fine0_gemm == fine0_gemm and (pk.families[2][2][0].wk_cat is not None) == fine0_gemm
    err = _row_err(w, fp64["64"])
    print(f"fine level 0 {'conv_gemm' if fine0_gemm else 'grouped'} route: row err vs fp64 {err:.2e}")
    assert err <= 1e-4, err


def test_latent_avg_is_added(nets):
    net = nets["Encoder4Editing"]
    n, size = CASES["64"]
    x = e4e_input(n, size).to(DEV)
    avg = torch.randn(18, 512, generator=torch.Generator().manual_seed(2))
    assert torch.equal(net(x, latent_avg=avg.to(DEV)), net(x) + avg.to(DEV))


def test_cpu_input_is_rejected(nets):
    with pytest.raises(RuntimeError):
        nets["Encoder4Editing"](torch.zeros(1, 3, 64, 64))


# ------------------------------------------------------------------------------------------ end to end


def test_infer_cli_writes_projected_w_that_w_to_s_accepts(tmp_path):
    from click.testing import CliRunner
    from PIL import Image
    from stylemc_amd import w_s
    from stylemc_amd.encoder4editing import infer
    from stylemc_amd.find_direction import load_generator
    rng = np.random.RandomState(3)
    img = str(tmp_path / "face.png")
    Image.fromarray(rng.randint(0, 256, (300, 280, 3), dtype=np.uint8)).save(img)
    out = str(tmp_path / "encoder4editing" / "projected_w.npz")
    res = CliRunner().invoke(infer._cli(), ["--input_image", img, "--out_file", out])
    assert res.exit_code == 0, res.output
    w = np.load(out)["w"]
    assert w.shape == (1, 18, 512) and w.dtype == np.float32 and np.isfinite(w).all()
    G = load_generator("synthetic", 1024, DEV)
    s = w_s.w_to_s(G, torch.tensor(w, device=DEV))
    assert tuple(s.shape) == (1, 26, 512) and torch.isfinite(s).all()
