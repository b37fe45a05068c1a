"""MTCNN on the GPU (mtcnn_hip.HipMTCNN over csrc/landmarks.hip and the gather GEMM), the detector end to end, crop_face's
tensor path, the landmarks term and the find_direction CLI with it.

Net tolerance: e_ref is the error of the same torch modules run in fp32 on the CPU (which reproduce the reference's
recorded outputs bit for bit, test_mtcnn_cpu.py) against their fp64 run, one figure per net over its cases; the HIP
nets are allowed 4 x e_ref against fp64 (summation order and the MFMA's accumulation differ).  Measured on an MI355X
(profiles/landmarks/README.md):
    pnet  e_ref 2.61e-07  HIP 3.11e-07     rnet  e_ref 3.04e-07  HIP 2.24e-07     onet  e_ref 3.91e-07  HIP 3.06e-07
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from stylemc_amd import align_faces, mobilenet_facial, mobilenet_hip, mtcnn_hip, synthetic, warp_images
from stylemc_amd.MTCNN import detector, get_nets
from tests.golden import landmarks_inputs as LI

pytestmark = pytest.mark.gpu
DEV = "cuda"
EPS = 2.0 ** -24


@pytest.fixture(scope="module")
def gold(golden):
    return golden("landmarks.npz")


@pytest.fixture(scope="module")
def nets(gold):
    """(HIP nets, fp64 torch nets, {net: [(key, input)]}, {net: e_ref})."""
    wts = synthetic.mtcnn_weights(seed=int(gold["nets/seed"]))
    t64 = get_nets.TorchMTCNN(wts, dtype=torch.float64)
    cases = {"pnet": [(f"nets/pnet/{k}", LI.net_input("pnet", hw=hw)) for k, hw in LI.PNET_SHAPES.items()],
             "rnet": [("nets/rnet", LI.net_input("rnet"))], "onet": [("nets/onet", LI.net_input("onet"))]}
    e_ref = {}
    for name, cs in cases.items():
        errs = []
        for key, x in cs:
            with torch.no_grad():
                outs64 = t64.nets[name](torch.as_tensor(x).double())
            errs += [np.abs(gold[f"{key}/out{j}"] - o.numpy()).max() for j, o in enumerate(outs64)]
        e_ref[name] = float(max(errs))
    return mtcnn_hip.HipMTCNN(wts, device=DEV), t64, cases, e_ref


def _err64(t64, name, x, outs):
    with torch.no_grad():
        outs64 = t64.nets[name](torch.as_tensor(x).double())
    assert len(outs) == len(outs64)
    for o, r in zip(outs, outs64):
        assert o.shape == tuple(r.shape) and np.isfinite(o).all()
    return max(float(np.abs(o - r.numpy()).max()) for o, r in zip(outs, outs64))


@pytest.mark.parametrize("shape", sorted(LI.PNET_SHAPES))
def test_pnet_against_fp64(nets, shape):
    hip, t64, cases, e_ref = nets
    x = dict(cases["pnet"])[f"nets/pnet/{shape}"]
    a, b = hip.pnet(x), hip.pnet(x)
    assert all(np.array_equal(p, q) for p, q in zip(a, b))
    err = _err64(t64, "pnet", x, a)
    print(f"pnet {shape}: e_ref {e_ref['pnet']:.2e}, HIP err {err:.2e}")
    assert e_ref["pnet"] > 0 and err <= 4 * e_ref["pnet"], (err, e_ref["pnet"])


@pytest.mark.parametrize("n", [1, 5])
@pytest.mark.parametrize("name", ["rnet", "onet"])
def test_rnet_onet_against_fp64(nets, name, n):
    hip, t64, cases, e_ref = nets
    x = cases[name][0][1][:n]
    a, b = getattr(hip, name)(x), getattr(hip, name)(x)
    assert all(np.array_equal(p, q) for p, q in zip(a, b))
    assert a[-1].shape == (n, 2) and np.allclose(a[-1].sum(1), 1.0, atol=1e-6)
    err = _err64(t64, name, x, a)
    print(f"{name} n {n}: e_ref {e_ref[name]:.2e}, HIP err {err:.2e}")
    assert e_ref[name] > 0 and err <= 4 * e_ref[name], (err, e_ref[name])


def test_detect_faces_end_to_end(gold, nets):
    """Every decision of the recorded run is at least 1e-3 from its threshold (the fixture's condition), the nets are
    within about 1e-6: the same boxes must come out, none skipped."""
    hip, _, _, e_ref = nets
    seed = int(gold["e2e/seed"])
    img = torch.from_numpy(LI.detect_image(seed).astype(np.float32)).to(DEV)
    boxes, lms = detector.detect_faces(img, thresholds=LI.THRESHOLDS, nms_thresholds=LI.NMS_THRESHOLDS, nets=hip)
    ref_b, ref_l = gold["e2e/boxes"], gold["e2e/landmarks"]
    assert len(boxes) == len(ref_b) >= 3
    assert np.abs(boxes[:, :4] - ref_b[:, :4]).max() <= 1.0
    assert np.abs(lms - ref_l).max() <= 1.0
    score_err = np.abs(boxes[:, 4] - ref_b[:, 4]).max()
    print(f"detect_faces: {len(boxes)} faces, max box diff {np.abs(boxes[:, :4] - ref_b[:, :4]).max():.2e} px, "
          f"score diff {score_err:.2e} (onet e_ref {e_ref['onet']:.2e})")
    assert score_err <= 4 * e_ref["onet"]


def test_crop_face_tensor_path_against_the_reference(gold):
    """The reference's crop_face on a tensor is an fp32 F.interpolate of the clipped window: the kernel's bound of
    test_gpu_landmarks.py in 0..255 units, 4 * 2^-24 * Smax * D + 8 * 2^-24 * 255."""
    img, faces = LI.crop_case()
    for key, f in faces.items():
        face, side, box = warp_images.crop_face(img.to(DEV), f, 32)
        meta = gold[f"crop/{key}/meta"]
        assert side == meta[0] and box == list(meta[1:])
        ref = gold[f"crop/{key}/face"]
        crop = img[box[1]:box[3], box[0]:box[2]]
        d = max((crop[1:] - crop[:-1]).abs().max().item(), (crop[:, 1:] - crop[:, :-1]).abs().max().item())
        bound = 4 * EPS * max(box[2] - box[0], box[3] - box[1]) * d + 8 * EPS * 255
        err = np.abs(face.cpu().numpy() - ref).max()
        print(f"crop_face {key}: err {err:.2e}, bound {bound:.2e}")
        assert face.shape == (32, 32, 3) and err <= bound, (key, err, bound)


def _generator_like(seed, shift):
    """A [1, 3, 96, 128] 'generator image' in [-1, 1] whose denormed uint8 copy is the fixture's image (so the seeded
    detector finds faces), optionally with a small smooth change (an 'edit')."""
    px = LI.detect_image(seed).astype(np.float32)
    x = torch.from_numpy((px + 0.25 - 128.0) / 127.5).permute(2, 0, 1).unsqueeze(0)
    if shift:
        yy, xx = torch.meshgrid(torch.arange(96.0), torch.arange(128.0), indexing="ij")
        x = x + shift * torch.sin(xx / 9.0) * torch.cos(yy / 7.0)
    return x.clamp(-1, 1)


def test_compute_landmarks_loss_against_the_torch_restatement(gold, nets):
    """Two batches (an 'original' and an 'edited' one) through compute_landmarks_loss on the GPU, against the same
    pipeline on the CPU from the torch modules: the detector's torch nets, the fp32 F.interpolate crop and the
    mobilenet_facial module.  Allowed: the regressor's tolerance (4 x e_ref of the fp32 CPU module against fp64 on these
    crops, in pixels: times the crop's side) through the loss's derivative, coef * 2 * max|delta landmark|."""
    from stylemc_amd import find_direction as FD
    from stylemc_amd.landmarks_loss import LandmarksLoss
    hip, _, _, _ = nets
    seed = int(gold["e2e/seed"])
    wts = synthetic.mtcnn_weights(seed=int(gold["nets/seed"]))
    t32 = get_nets.TorchMTCNN(wts)
    ref_net = mobilenet_facial.MobileNet_GDConv(136).eval().requires_grad_(False)
    sd = synthetic.mobilenet_state_dict(ref_net, seed=7)
    ref_net.load_state_dict(sd)
    model = mobilenet_hip.build_mobilenet(sd, device=DEV, input_size=224)
    mean, std = FD.utils.get_mean_std("cpu")
    orig = torch.cat([_generator_like(seed, 0.0), _generator_like(seed, 0.02)])
    edit = torch.cat([_generator_like(seed, 0.05), _generator_like(seed, 0.08)])
    coef = 25.0
    thr = dict(thresholds=LI.THRESHOLDS, nms_thresholds=LI.NMS_THRESHOLDS)

    def cpu_landmarks(batch, net):
        out, crops = [], []
        for x in batch:
            im = FD.denorm_img(x)
            faces, _ = detector.detect_faces(im, nets=t32, **thr)
            assert len(faces)
            box, _ = warp_images.crop_box(im.size(1), im.size(0), faces[0])
            crop = im[box[1]:box[3], box[0]:box[2]].permute(2, 0, 1).unsqueeze(0)
            crop = F.interpolate(crop, size=224, mode="bilinear", align_corners=False)
            crops.append(((crop / 255 - mean) / std, box))
        for c, box in crops:
            with torch.no_grad():
                lm = net(c.to(next(net.parameters()).dtype)).view(-1, 2).double()
            out.append(lm * (box[3] - box[1]) + torch.tensor([box[0], box[1]], dtype=torch.float64))
        return torch.stack(out), max(b[3] - b[1] for _, b in crops)

    l1_32, side = cpu_landmarks(orig, ref_net)
    l2_32, _ = cpu_landmarks(edit, ref_net)
    net64 = mobilenet_facial.MobileNet_GDConv(136).eval().requires_grad_(False)
    net64.load_state_dict(sd)
    net64 = net64.double()
    l1_64, _ = cpu_landmarks(orig, net64)
    l2_64, _ = cpu_landmarks(edit, net64)
    e_ref_px = max((l1_32 - l1_64).abs().max().item(), (l2_32 - l2_64).abs().max().item())
    want = coef * LandmarksLoss()(l1_64, l2_64).item()
    delta = (l1_64 - l2_64)[:, 17:].abs().max().item()

    got = FD.compute_landmarks_loss(edit.to(DEV), orig.to(DEV), LandmarksLoss(), coef, model, DEV, mean.to(DEV),
                                    std.to(DEV), 224, mtcnn=hip, **thr)
    got = float(got)
    tol = coef * 2 * delta * 4 * e_ref_px
    print(f"landmarks loss: HIP {got:.6f}, fp64 restatement {want:.6f}, max|delta| {delta:.3f} px, e_ref {e_ref_px:.2e} px, "
          f"|diff| {abs(got - want):.2e}, allowed {tol:.2e}")
    assert want > 0 and delta > 0 and np.isfinite(got)
    assert abs(got - want) <= tol, (got, want, tol)
    # an image without a face makes the term 0
    blank = torch.zeros(1, 3, 96, 128, device=DEV)
    assert FD.compute_landmarks_loss(blank, blank, LandmarksLoss(), coef, model, DEV, mean.to(DEV), std.to(DEV), 224,
                                     mtcnn=hip, **thr) == 0


def _run_cli(tmp_path, name, iterations, extra):
    from click.testing import CliRunner
    from stylemc_amd import find_direction as FD
    # 2 images per step; 2 * iterations seeds and one epoch make exactly `iterations` iterations
    base = ["--text_prompt", "a b", "--clip_type", "small", "--resolution", "256", "--n_seeds", str(2 * iterations),
            "--batch_size", "2", "--n_epochs", "1", "--max_iterations", str(iterations), "--network", "synthetic"]
    out = tmp_path / name
    res = CliRunner().invoke(FD._cli(), base + ["--outdir", str(out)] + extra, catch_exceptions=False)
    assert res.exit_code == 0, res.output
    return res.output, np.load(out / "direction_a_b.npz")["s"]


ON = ["--landmarks_loss_coef", "25", "--mobilenet_checkpoint", "synthetic", "--mtcnn_weights", "synthetic"]


def test_find_direction_cli_two_iterations_leave_the_direction_alone(tmp_path):
    """--landmarks_loss_coef 25 with the seeded nets, 256 px, 2 iterations: the saved direction is bit-equal to the run
    with coefficient 0 (the term is evaluated outside the step).  find_direction prints every 10th iteration, as the
    reference does, so a 2-iteration run prints no loss line with or without the term; the printed value is checked at
    iteration 10 below."""
    text_on, s_on = _run_cli(tmp_path, "on", 2, ON)
    text_off, s_off = _run_cli(tmp_path, "off", 2, ["--landmarks_loss_coef", "0"])
    assert s_on.shape == (1, 26, 512) and np.abs(s_on).max() > 0 and np.array_equal(s_on, s_off)
    assert "landmarks loss" not in text_on and "landmarks loss" not in text_off


def test_find_direction_cli_prints_the_term_at_printed_iterations(tmp_path):
    """20 iterations, so that the lines of iterations 10 and 20 are printed and ten steps run AFTER the first evaluation
    of the term (the step after it finds its original images already prefetched on the third stream): with the seeded
    nets a finite landmarks value stands in both lines and is part of the printed total; with coefficient 0, and with
    the coefficient but the default file names (absent here: the same warning as before), the lines say 0.0000.  All
    three directions are bit-equal, and so are the other printed terms of both lines."""
    import re
    pat = r"Iteration (\d+),.*\nTotal loss: (\S+), clip loss: (\S+), identity loss: (\S+), landmarks loss: (\S+), l2 loss: (\S+)"

    def lines(text):
        got = {int(m[0]): [float(v.rstrip(",")) for v in m[1:]] for m in re.findall(pat, text)}
        assert sorted(got) == [10, 20], text
        return got

    text_on, s_on = _run_cli(tmp_path, "on", 20, ON)
    on = lines(text_on)
    for total, clip, ident, lm, l2 in on.values():
        assert np.isfinite(lm) and lm >= 0 and abs(total - (clip + ident + lm + l2)) <= 5e-4 * max(1.0, abs(total))
    text_off, s_off = _run_cli(tmp_path, "off", 20, ["--landmarks_loss_coef", "0"])
    off = lines(text_off)
    assert text_off.count("landmarks loss: 0.0000") == 2
    assert np.array_equal(s_on, s_off)
    for it in (10, 20):
        assert on[it][1:3] == off[it][1:3] and on[it][4] == off[it][4]
    with pytest.warns(UserWarning, match="landmarks loss adds no gradient"):
        text_warn, s_warn = _run_cli(tmp_path, "warn", 20, ["--landmarks_loss_coef", "25",
                                                            "--mobilenet_checkpoint", str(tmp_path / "absent.pth.tar"),
                                                            "--mtcnn_weights", str(tmp_path / "absent")])
    assert text_warn.count("landmarks loss: 0.0000") == 2 and np.array_equal(s_warn, s_off)
    assert lines(text_warn) == off


def test_align_faces_takes_the_best_face(gold, nets):
    """align_faces.detect_landmarks on the fixture photograph (default thresholds: six faces with these seeded nets)
    against the same steps on the CPU from the torch modules: the best-scoring face, crop_face's PIL path, the
    regressor.  The points are truncated to integers, so values 1e-4 px apart may land one pixel apart."""
    from PIL import Image
    hip = nets[0]
    pixels = LI.detect_image(int(gold["e2e/seed"]))
    model, mean, std = align_faces.load_model(DEV, "synthetic")
    lm = align_faces.detect_landmarks(pixels, model, DEV, mean, std, mtcnn=hip)
    assert lm.shape == (68, 2) and lm.dtype.kind == "i"
    t32 = get_nets.TorchMTCNN(synthetic.mtcnn_weights(seed=int(gold["nets/seed"])))
    faces, _ = detector.detect_faces(torch.from_numpy(pixels.copy()), nets=t32)
    assert len(faces) >= 2 and np.argmax(faces[:, 4]) == 0 and faces[0, 4] > faces[1, 4]
    cropped, side, box = warp_images.crop_face(Image.fromarray(pixels), [faces[np.argmax(faces[:, 4])]], 224)
    ref_net = mobilenet_facial.MobileNet_GDConv(136).eval().requires_grad_(False)
    ref_net.load_state_dict(synthetic.mobilenet_state_dict(ref_net, seed=7))
    x = torch.from_numpy(np.array(cropped)).float().unsqueeze(0).permute(0, 3, 1, 2)
    x = (x / 255 - mean.cpu().unsqueeze(0)) / std.cpu().unsqueeze(0)
    with torch.no_grad():
        ref = ref_net(x).view(-1, 2) * side + torch.tensor([box[0], box[1]])
    assert np.abs(lm - ref.numpy().astype(int)).max() <= 1
    out = align_faces.align_face(pixels, lm, **LI.ALIGN_KW)
    assert out.size == (64, 64)


def test_photo_to_w_plus_without_an_aligned_input(gold, tmp_path):
    """photo -> align_faces -> infer, and infer --align on the photo itself, through the CLIs: MTCNN weight files in the
    reference's format (the seeded nets that find faces in the fixture photograph), the seeded regressor and encoder."""
    from click.testing import CliRunner
    from PIL import Image
    from stylemc_amd.encoder4editing import infer
    seed = int(gold["e2e/seed"])
    wdir = tmp_path / "weights"
    wdir.mkdir()
    for name, wts in synthetic.mtcnn_weights(seed=seed).items():
        get_nets.save_weight_file(str(wdir / f"{name}.npy"), wts)
    photo, aligned = str(tmp_path / "photo.png"), str(tmp_path / "aligned.png")
    Image.fromarray(LI.detect_image(seed)).save(photo)
    nets_args = ["--mobilenet_checkpoint", "synthetic", "--mtcnn_weights", str(wdir)]
    res = CliRunner().invoke(align_faces._cli(), ["--input_image", photo, "--out", aligned, "--output_size", "256",
                                                  "--transform_size", "512"] + nets_args, catch_exceptions=False)
    assert res.exit_code == 0, res.output
    assert Image.open(aligned).size == (256, 256)
    ws = []
    for name, args in (("a", ["--input_image", aligned]), ("b", ["--input_image", photo, "--align"] + nets_args)):
        out = str(tmp_path / f"w_{name}.npz")
        res = CliRunner().invoke(infer._cli(), args + ["--out_file", out], catch_exceptions=False)
        assert res.exit_code == 0, res.output
        ws.append(np.load(out)["w"])
        assert ws[-1].shape == (1, 18, 512) and np.isfinite(ws[-1]).all()
    # a blank photograph has no face: the CLI says so instead of writing something
    blank = str(tmp_path / "blank.png")
    Image.fromarray(np.zeros((96, 128, 3), np.uint8)).save(blank)
    res = CliRunner().invoke(align_faces._cli(), ["--input_image", blank, "--out", aligned] + nets_args)
    assert res.exit_code != 0 and "no face" in str(res.exception)
