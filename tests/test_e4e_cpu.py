"""e4e real-image inversion, host side (CPU): the restated encoders against the reference's own outputs
(tests/golden/e4e.npz, written by tests/golden/make_golden_e4e.py from the unmodified reference modules), their
state_dict names, the CLI's preprocessing and checkpoint handling, and the host-side validation of the new C-ABI entry
points (no device call, the pattern of test_capi.py::test_abi_version_and_errors_without_gpu)."""
import ctypes

import numpy as np
import pytest
import torch

from stylemc_amd import _hip, synthetic
from stylemc_amd.encoder4editing import infer
from stylemc_amd.encoder4editing.models.encoders import psp_encoders as PE
from tests.golden.e4e_inputs import CASES, ENCODERS, SEED, e4e_input


@pytest.fixture(scope="module")
def encoder():
    net = PE.Encoder4Editing(50, "ir_se", 1024).eval().requires_grad_(False)
    net.load_state_dict(synthetic.e4e_state_dict(net, seed=SEED), strict=True)
    return net


@pytest.fixture(scope="module")
def heads(encoder):
    """The 18 head outputs [n, 18, 512] per fixture case, computed once (both encoders combine the same heads: their
    state_dicts have the same names, and the seeded weights are drawn by name)."""
    with torch.no_grad():
        return {key: torch.stack(encoder.head_outputs(e4e_input(n, size)), dim=1) for key, (n, size) in CASES.items()}


@pytest.mark.parametrize("name", ENCODERS)
@pytest.mark.parametrize("key", sorted(CASES))
def test_restated_encoders_reproduce_the_reference(golden, heads, name, key):
    """fp32 CPU forward of the restated module vs the reference module's (fp32 CPU forwards differ from fp64 by about
    1e-6 of the max): 1e-5 of max|ref|."""
    ref = golden("e4e.npz")[f"{name}/w{key}"]
    got = PE.ENCODERS[name].combine(heads[key]).numpy()
    assert got.shape == ref.shape == (CASES[key][0], 18, 512)
    err = np.abs(got - ref).max() / np.abs(ref).max()
    print(f"{name} {key} px: max err / max|ref| = {err:.2e}")
    assert err <= 1e-5, err


def test_e4e_rows_are_w0_plus_deltas(heads):
    h = heads["64"]
    w = PE.Encoder4Editing.combine(h)
    assert torch.equal(w[:, 0], h[:, 0]) and torch.equal(w[:, 5], h[:, 0] + h[:, 5])
    assert torch.equal(PE.GradualStyleEncoder.combine(h), h)


@pytest.mark.parametrize("name", ENCODERS)
def test_state_dict_keys_equal_the_reference(golden, encoder, name):
    ref_keys = str(golden("e4e.npz")["keys"]).split("\n")
    net = encoder if name == "Encoder4Editing" else PE.ENCODERS[name](50, "ir_se", 1024)
    assert list(net.state_dict().keys()) == ref_keys
    assert "styles.17.convs.10.weight" in ref_keys and "styles.0.linear.bias" in ref_keys
    assert "latlayer1.bias" in ref_keys and "body.23.res_layer.5.fc2.weight" in ref_keys


def test_e4e_state_dict_doubles_only_head_and_lateral_conv_weights(encoder):
    plain = synthetic.seeded_state_dict(encoder, seed=SEED)
    for k, v in encoder.state_dict().items():
        doubled = k.endswith(".weight") and ((k.startswith("styles.") and ".convs." in k) or k.startswith("latlayer"))
        assert torch.equal(v, plain[k] * 2 if doubled else plain[k]), k


def test_preprocess_is_the_pil_and_numpy_arithmetic():
    """infer.py:73-77,94,112 of the reference: convert('RGB'), bilinear resize to 256 x 256, /255, (x - 0.5) / 0.5."""
    from PIL import Image
    rng = np.random.RandomState(0)
    img = Image.fromarray(rng.randint(0, 256, (300, 280, 4), dtype=np.uint8), "RGBA")  # 280 wide, 300 high
    x = infer.preprocess(img)
    assert x.shape == (1, 3, 256, 256) and x.dtype == torch.float32
    want = np.asarray(img.convert("RGB").resize((256, 256), Image.BILINEAR)).astype(np.float32)
    want = ((want / 255.0) - 0.5) / 0.5
    assert np.array_equal(x[0].numpy(), want.transpose(2, 0, 1))
    assert -1.0 <= x.min() and x.max() <= 1.0


def test_checkpoint_key_filtering(tmp_path):
    """psp.py:11-15,41-47,94-100 on a small fake checkpoint, through torch.load(weights_only=True)."""
    sd = {"encoder.input_layer.0.weight": torch.ones(2), "encoder.styles.0.linear.bias": torch.zeros(3),
          "decoder.conv1.weight": torch.ones(1), "latent_avg": torch.ones(1)}
    ckpt = {"state_dict": sd, "latent_avg": torch.full((18, 512), 0.5),
            "opts": {"encoder_type": "GradualStyleEncoder", "stylegan_size": 512, "start_from_latent_avg": True}}
    path = str(tmp_path / "ckpt.pt")
    torch.save(ckpt, path)
    loaded = torch.load(path, map_location="cpu", weights_only=True)
    etype, size, enc_sd, avg = infer.checkpoint_parts(loaded)
    assert (etype, size) == ("GradualStyleEncoder", 512)
    assert sorted(enc_sd) == ["input_layer.0.weight", "styles.0.linear.bias"]
    assert avg.shape == (18, 512) and float(avg[0, 0]) == 0.5
    ckpt["opts"]["start_from_latent_avg"] = False
    assert infer.checkpoint_parts(ckpt)[3] is None
    assert infer.get_keys(sd, "decoder") == {"conv1.weight": sd["decoder.conv1.weight"]}
    with pytest.raises(ValueError):
        infer.checkpoint_parts({"state_dict": {"decoder.x": torch.ones(1)}})


def test_infer_help_runs_without_a_gpu():
    from click.testing import CliRunner
    res = CliRunner().invoke(infer._cli(), ["--help"])
    assert res.exit_code == 0
    for word in ("--input_image", "--checkpoint", "--out_file", "encoder4editing/projected_w.npz", "aligned"):
        assert word in res.output, word


def test_live_taps():
    from stylemc_amd.e4e_hip import live_taps
    assert live_taps(1, 1) == [4]
    assert live_taps(2, 2) == [4, 5, 7, 8]
    assert live_taps(3, 3) == list(range(9)) and live_taps(16, 16) == list(range(9))
    assert live_taps(1, 4) == [3, 4, 5] and live_taps(2, 1) == [4, 7]


def test_new_entry_points_reject_bad_shapes_on_the_host():
    lib = _hip.load()
    taps9 = (ctypes.c_int * 9)(*range(9))
    fake = ctypes.c_void_p(256)

    def grouped(groups=2, n=1, cin=64, h=4, w=4, taps=taps9, ntaps=9, cout=64, ss=None, gs=0, x=fake, wk=fake, y=fake):
        ss = cin * h * w if ss is None else ss
        return lib.smc_conv_s2_grouped_f32(x, ss, gs, groups, n, cin, h, w, wk, taps, ntaps, None, 0.01, y, cout, None,
                                           0, None)

    for kwargs, word in (({"cin": 24}, b"cin"), ({"cout": 48}, b"cout"), ({"groups": 0}, b"groups"),
                         ({"h": 0}, b"h, w"), ({"ntaps": 0}, b"taps"), ({"ntaps": 10}, b"taps"),
                         ({"taps": (ctypes.c_int * 2)(5, 4), "ntaps": 2}, b"ascending"),
                         ({"taps": (ctypes.c_int * 1)(9), "ntaps": 1}, b"0..8"),
                         ({"x": None}, b"null"), ({"ss": 8}, b"strides"),
                         ({"n": 64, "cin": 512, "h": 256, "w": 256}, b"2 GiB"),
                         ({"wk": ctypes.c_void_p(260)}, b"aligned")):
        assert grouped(**kwargs) == 1, kwargs
        assert word in lib.smc_last_error(), (kwargs, lib.smc_last_error())
    assert lib.smc_conv_s2_grouped_supported(11, 1, 512, 512, 64, 64) == 1
    assert lib.smc_conv_s2_grouped_supported(3, 2, 64, 64, 7, 5) == 1      # odd, non-square planes
    assert lib.smc_conv_s2_grouped_supported(18, 1, 512, 512, 1, 1) == 1
    assert lib.smc_conv_s2_grouped_supported(1, 1, 24, 64, 8, 8) == 0      # cin % 16
    assert lib.smc_conv_s2_grouped_supported(1, 1, 64, 48, 8, 8) == 0      # cout % 32
    assert lib.smc_conv_s2_grouped_supported(11, 64, 512, 512, 64, 64) == 0  # input >= 2 GiB
    assert lib.smc_conv_s2_grouped_workspace_size(1, 1, 24, 64, 8, 8, 9) == -1
    assert lib.smc_conv_s2_grouped_workspace_size(11, 1, 512, 512, 64, 64, 9) == 0   # tiles fill the chip: no split
    assert lib.smc_conv_s2_grouped_workspace_size(11, 1, 512, 512, 2, 2, 4) > 0      # weight streaming: split K
    # a split launch without its workspace fails on the host
    assert grouped(groups=11, cin=512, cout=512, h=2, w=2, taps=(ctypes.c_int * 4)(4, 5, 7, 8), ntaps=4) == 1
    assert b"workspace" in lib.smc_last_error()

    assert lib.smc_upsample_add_f32(fake, 0, 4, 4, fake, fake, 8, 8, None) == 1
    assert b"shape" in lib.smc_last_error()
    assert lib.smc_upsample_add_f32(None, 4, 4, 4, fake, fake, 8, 8, None) == 1
    assert lib.smc_upsample_add_f32(fake, 1 << 20, 32, 32, fake, fake, 64, 64, None) == 1
    assert b"2 GiB" in lib.smc_last_error()

    assert lib.smc_irse_trunk_f32(None, fake, 1, None, None, 3, fake, 0, None) == 1
    assert b"bad net" in lib.smc_last_error()
    assert lib.smc_irse_trunk_workspace_bytes(None, 1) == -1
