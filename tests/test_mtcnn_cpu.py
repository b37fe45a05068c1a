"""MTCNN detector, host side (CPU), against the reference's own outputs (tests/golden/landmarks.npz, written by
tests/golden/make_golden_landmarks.py from the unmodified reference package): the box arithmetic bit for bit, detect_faces
with the nets replaced by the recorded outputs, the restated torch nets, the weight files, crop_box, the landmark
distances, and find_direction's behaviour without the new options."""
import os
import pickle

import numpy as np
import pytest
import torch
from PIL import Image

from stylemc_amd import align_faces, landmarks_loss, synthetic, warp_images
from stylemc_amd.MTCNN import box_utils, detector, first_stage, get_nets
from tests.golden import landmarks_inputs as LI


@pytest.fixture(scope="module")
def gold(golden):
    return golden("landmarks.npz")


def test_host_functions_bit_equal_the_reference(gold):
    boxes, offs = LI.host_boxes(), LI.host_offsets()
    assert np.array_equal(np.array(box_utils.nms(boxes.copy(), 0.5, "union")), gold["host/nms_union"])
    assert np.array_equal(np.array(box_utils.nms(boxes.copy(), 0.7, "min")), gold["host/nms_min"])
    assert 0 < len(gold["host/nms_min"]) < len(gold["host/nms_union"]) < len(boxes)   # both modes drop boxes
    assert box_utils.nms(np.zeros((0, 5))) == []
    assert np.array_equal(box_utils.calibrate_box(boxes.copy(), offs), gold["host/calibrate_box"])
    assert np.array_equal(box_utils.convert_to_square(boxes.copy()), gold["host/convert_to_square"])
    b = np.round(boxes.copy())
    got = np.stack(box_utils.correct_bboxes(b, 128, 96))
    assert got.dtype == np.int32 and np.array_equal(got, gold["host/correct_bboxes"])
    assert np.array_equal(b, gold["host/correct_bboxes_arg"]) and not np.array_equal(b, np.round(boxes))
    probs, poffs = LI.pnet_maps()
    assert np.array_equal(first_stage._generate_bboxes(probs, poffs, 0.6 * 0.707, 0.55), gold["host/generate_bboxes"])
    assert first_stage._generate_bboxes(probs, poffs, 0.5, 2.0).size == 0


def test_pyramid_scales_equal_the_reference(gold):
    h, w = LI.IMAGE_HW
    assert np.array_equal(np.array(detector.pyramid_scales(w, h, 20.0)), gold["e2e/scales"])
    assert detector.pyramid_scales(12, 12, 20.0) == []


class _Replay:
    """The nets of detect_faces replaced by the reference's recorded outputs, in call order."""

    def __init__(self, gold):
        self.gold, self.i = gold, 0

    def _next(self, name, x):
        assert str(self.gold[f"e2e/call{self.i}/net"]) == name
        outs, j = [], 0
        while f"e2e/call{self.i}/out{j}" in self.gold:
            outs.append(self.gold[f"e2e/call{self.i}/out{j}"].copy())
            j += 1
        assert x.dtype == np.float32 and x.shape[0] == outs[0].shape[0]
        self.i += 1
        return tuple(outs)

    def pnet(self, x):
        return self._next("pnet", x)

    def rnet(self, x):
        return self._next("rnet", x)

    def onet(self, x):
        return self._next("onet", x)


def test_detect_faces_with_recorded_net_outputs_is_bit_equal(gold):
    seed = int(gold["e2e/seed"])
    img = torch.from_numpy(LI.detect_image(seed).astype(np.float32))
    nets = _Replay(gold)
    boxes, lms = detector.detect_faces(img, thresholds=LI.THRESHOLDS, nms_thresholds=LI.NMS_THRESHOLDS, nets=nets)
    assert nets.i == int(gold["e2e/ncalls"])
    assert len(boxes) >= 3 and np.array_equal(boxes, gold["e2e/boxes"])
    assert lms.dtype == np.float32 and np.array_equal(lms, gold["e2e/landmarks"])
    assert gold["e2e/margins"].min() >= LI.MARGIN    # the fixture's condition: no decision within 1e-3 of its threshold
    # a PIL image is taken as it is
    nets = _Replay(gold)
    boxes2, _ = detector.detect_faces(Image.fromarray(LI.detect_image(seed)), thresholds=LI.THRESHOLDS,
                                      nms_thresholds=LI.NMS_THRESHOLDS, nets=nets)
    assert np.array_equal(boxes2, boxes)


def test_detect_faces_without_a_face_returns_empty(gold):
    class Nothing(_Replay):
        def pnet(self, x):
            o, p = super().pnet(x)
            p[:, 1] = 0.0
            return o, p
    img = torch.from_numpy(LI.detect_image(int(gold["e2e/seed"])).astype(np.float32))
    assert detector.detect_faces(img, thresholds=LI.THRESHOLDS, nets=Nothing(gold)) == ([], [])


@pytest.fixture(scope="module")
def torch_nets(gold):
    return get_nets.TorchMTCNN(synthetic.mtcnn_weights(seed=int(gold["nets/seed"])))


def test_restated_nets_reproduce_the_reference(gold, torch_nets):
    """Same layers, same fp32 CPU ops: 1e-6 absolute on outputs of order 1 (probabilities, offsets, landmarks)."""
    cases = [("pnet", f"nets/pnet/{k}", LI.net_input("pnet", hw=hw)) for k, hw in LI.PNET_SHAPES.items()]
    cases += [(n, f"nets/{n}", LI.net_input(n)) for n in ("rnet", "onet")]
    for name, key, x in cases:
        outs = getattr(torch_nets, name)(x)
        for j, o in enumerate(outs):
            ref = gold[f"{key}/out{j}"]
            assert o.shape == ref.shape, (key, j)
            err = np.abs(o - ref).max()
            print(f"{key} out{j}: max err {err:.2e}")
            assert err <= 1e-6, (key, j, err)
    assert gold["nets/pnet/13x12/out1"].shape == (1, 2, 2, 1)


def test_parameter_names_are_the_references():
    want = {"pnet": ["features.conv1.weight", "features.conv1.bias", "features.prelu1.weight", "features.conv2.weight",
                     "features.conv2.bias", "features.prelu2.weight", "features.conv3.weight", "features.conv3.bias",
                     "features.prelu3.weight", "conv4_1.weight", "conv4_1.bias", "conv4_2.weight", "conv4_2.bias"]}
    assert [k for k, _ in get_nets.PNet().named_parameters()] == want["pnet"]
    r = dict(get_nets.RNet().named_parameters())
    assert tuple(r["features.conv4.weight"].shape) == (128, 576) and "features.prelu4.weight" in r and "conv5_2.bias" in r
    o = dict(get_nets.ONet().named_parameters())
    assert tuple(o["features.conv5.weight"].shape) == (256, 1152) and tuple(o["conv6_3.weight"].shape) == (10, 256)
    assert len(o) == 21 and len(r) == 16


def test_weight_files_round_trip_and_refuse_code(tmp_path):
    wts = synthetic.mtcnn_weights(seed=2)
    for name in get_nets.NAMES:
        get_nets.save_weight_file(str(tmp_path / f"{name}.npy"), wts[name])
    # the file is what the reference reads: np.load(allow_pickle=True)[()] gives the dict
    raw = np.load(str(tmp_path / "pnet.npy"), allow_pickle=True)[()]
    assert sorted(raw) == sorted(wts["pnet"])
    got = get_nets.load_weights(str(tmp_path))
    for name in get_nets.NAMES:
        assert sorted(got[name]) == sorted(wts[name])
        assert all(np.array_equal(got[name][k], wts[name][k]) and got[name][k].dtype == np.float32 for k in wts[name])

    class Evil:
        def __reduce__(self):
            return (os.system, ("true",))

    bad = str(tmp_path / "bad.npy")
    with open(bad, "wb") as f:
        np.save(f, {"features.conv1.weight": Evil()}, allow_pickle=True)
    with pytest.raises(pickle.UnpicklingError, match="allow-list"):
        get_nets.load_weight_file(bad)
    with open(bad, "wb") as f:
        np.save(f, {"features.conv1.weight": "a string"}, allow_pickle=True)
    with pytest.raises(ValueError, match="numeric array"):
        get_nets.load_weight_file(bad)
    with open(bad, "wb") as f:
        np.save(f, np.zeros((3, 3), np.float32))
    with pytest.raises(ValueError, match="pickled dict"):
        get_nets.load_weight_file(bad)


def test_crop_box_equals_the_reference(gold):
    img, faces = LI.crop_case()
    for key, f in faces.items():
        box, pads = warp_images.crop_box(img.size(1), img.size(0), f[0])
        meta = gold[f"crop/{key}/meta"]
        assert box == list(meta[1:]) and box[3] - box[1] == meta[0]
        assert (max(pads) > 0) == (key == "clipped")


def test_crop_face_pil_path_pads_what_left_the_image():
    img, faces = LI.crop_case()
    pil = Image.fromarray(img.numpy().astype(np.uint8))
    face, side, box = warp_images.crop_face(pil, faces["clipped"], 32)
    assert face.shape == (32, 32, 3) and face.dtype == np.uint8
    wbox, pads = warp_images.crop_box(*pil.size, faces["clipped"][0])
    assert side == (wbox[3] - wbox[1]) + pads[1] + pads[3] and box == wbox
    assert (face[:, -1] == 0).all()       # the right edge lies in the zero padding
    face_in, side_in, _ = warp_images.crop_face(pil, faces["inside"], 32)
    assert side_in == 49 and face_in.min() >= 0


def test_landmark_distances():
    g = torch.Generator().manual_seed(0)
    a = torch.rand(2, 68, 2, generator=g) * 200
    b = a.clone()
    b[:, :17] += 50.0                      # the jaw line is not compared
    assert landmarks_loss.LandmarksLoss()(a, b).item() == 0.0 and landmarks_loss.WingLoss()(a, b).item() == 0.0
    b[:, 17:] += 3.0
    assert landmarks_loss.LandmarksLoss()(a, b).item() == pytest.approx(9.0, rel=1e-5)
    assert landmarks_loss.WingLoss()(a, b).item() == pytest.approx(10 * np.log(1 + 3.0 / 2), rel=1e-5)
    b[:, 17:] += 17.0                      # 20 >= omega: the linear piece
    c = 10 - 10 * np.log(1 + 10 / 2)
    assert landmarks_loss.WingLoss()(a, b).item() == pytest.approx(20.0 - c, rel=1e-5)


def test_find_direction_options_and_availability(tmp_path):
    from click.testing import CliRunner
    from stylemc_amd import find_direction as FD
    res = CliRunner().invoke(FD._cli(), ["--help"])
    assert res.exit_code == 0
    text = "".join(res.output.split())   # (click wraps the long default across lines)
    for word in ("--mobilenet_checkpoint", "--mtcnn_weights", "mobilenet_224_model_best_gdconv_external.pth.tar",
                 "MTCNN/weights", "--landmarks_loss_coef"):
        assert word in text, word
    # the defaults name files that are not there: the term stays off (the same warning and 0.0 as before)
    assert not FD.LandmarksTerm.available(str(tmp_path / "mobilenet.pth.tar"), str(tmp_path))
    assert not FD.LandmarksTerm.available("synthetic", str(tmp_path))
    assert FD.LandmarksTerm.available("synthetic", "synthetic")
    for name in get_nets.NAMES:
        get_nets.save_weight_file(str(tmp_path / f"{name}.npy"), synthetic.mtcnn_weights(seed=1)[name])
    assert FD.LandmarksTerm.available("synthetic", str(tmp_path))
    assert FD.compute_landmarks_loss(None, None, None, 0, None, "cpu", None, None) == 0


@pytest.mark.parametrize("key", ["nopad", "pad"])
def test_align_face_equals_the_reference(gold, key, monkeypatch):
    """align_faces.py:61-160 at output_size 64, transform_size 256 on a seeded photograph and seeded landmarks: equal to
    the reference's output; one level of slack only where the running Pillow is not the one that made the fixture (its
    resampling filters are the only arithmetic here that is not this module's own)."""
    import PIL
    import scipy.ndimage
    padded = []
    real = scipy.ndimage.gaussian_filter
    monkeypatch.setattr(scipy.ndimage, "gaussian_filter", lambda *a, **k: padded.append(1) or real(*a, **k))
    img, lm = LI.align_case(key)
    out = align_faces.align_face(img, lm, **LI.ALIGN_KW)
    assert out.size == (64, 64) and out.mode == "RGB"
    assert bool(padded) == (key == "pad")                # the case that pads runs the reflect-pad branch, the other not
    got, ref = np.asarray(out).astype(int), gold[f"align/{key}"].astype(int)
    slack = 0 if str(gold["align/pillow"]) == PIL.__version__ else 1
    assert np.abs(got - ref).max() <= slack, (np.abs(got - ref).max(), slack)
    assert ref.std() > 10                                # (a picture, not a flat field)


def test_align_face_options():
    img, lm = LI.align_case("nopad")
    level = np.asarray(align_faces.align_face(img, lm, rotate_level=False, **LI.ALIGN_KW)).astype(int)
    turned = np.asarray(align_faces.align_face(img, lm, **LI.ALIGN_KW)).astype(int)
    assert np.abs(level - turned).max() > 0              # the landmarks are tilted by 0.2 rad
    nopad = align_faces.align_face(*LI.align_case("pad"), enable_padding=False, **LI.ALIGN_KW)
    assert nopad.size == (64, 64)
    from click.testing import CliRunner
    res = CliRunner().invoke(align_faces._cli(), ["--help"])
    assert res.exit_code == 0
    for word in ("--input_image", "--out", "--output_size", "--mobilenet_checkpoint", "--mtcnn_weights"):
        assert word in res.output, word
