"""Real image -> W+ (the reference README's use case (b), encoder4editing/infer.py:73-134 + models/psp.py:57-68).

    python -m stylemc_amd.encoder4editing.infer --input_image IMG [--checkpoint e4e_ffhq_encode.pt]
                                                [--out_file encoder4editing/projected_w.npz]
    python -m stylemc_amd.w_s w_s_converter --projected-w encoder4editing/projected_w.npz ...

Writes ``np.savez(out_file, w=latents)`` with ``w`` [1, 18, 512] (infer.py:134), which ``w_s w_s_converter`` reads
unchanged.  The encoder runs on the HIP kernels (``stylemc_amd.e4e_hip.HipE4E``).

What is restated and what is not:
  preprocessing  infer.py:73-77,93-94,112: convert("RGB"), Resize((256, 256)) -- torchvision's Resize on a PIL image is
                 PIL's bilinear resize --, ToTensor (/255), Normalize(0.5, 0.5).  torchvision is absent here: parity
                 unpinned for the resize call itself.
  checkpoint     infer.py:81-87 + psp.py:11-15,41-47,94-100: ``opts`` (encoder_type, stylegan_size,
                 start_from_latent_avg), the ``encoder.``-prefixed state_dict keys, ``latent_avg``.  Loaded with
                 ``weights_only=True``.  Without --checkpoint the seeded synthetic encoder is used, as the other CLIs do
                 with ``--network synthetic``.
  alignment      infer.py:96-105 aligns with dlib landmarks; here ``--align`` runs stylemc_amd.align_faces first (MTCNN +
                 MobileNet-GDConv landmarks, the same FFHQ align_face), as the reference's own align_faces.py does.
                 Without ``--align`` the image is taken as an already aligned face crop.
  decoder        the rosinality generator only renders the inversion for display (infer.py:127-133); W does not need it.
"""
import os

import numpy as np
import torch

INPUT_SIZE = 256  # infer.py:74,77


def preprocess(image):
    """PIL image -> [1, 3, 256, 256] float32 in [-1, 1] (infer.py:73-77,94,112,127)."""
    from PIL import Image
    image = image.convert("RGB").resize((INPUT_SIZE, INPUT_SIZE), Image.BILINEAR)
    x = np.asarray(image, dtype=np.uint8).astype(np.float32) / 255.0           # ToTensor
    x = (x - 0.5) / 0.5                                                         # Normalize([0.5] * 3, [0.5] * 3)
    return torch.from_numpy(np.ascontiguousarray(x.transpose(2, 0, 1))).unsqueeze(0)


def get_keys(d, name):
    """psp.py:11-15: the entries of a checkpoint's state_dict under ``name.``, prefix removed."""
    if "state_dict" in d:
        d = d["state_dict"]
    return {k[len(name) + 1:]: v for k, v in d.items() if k[:len(name)] == name}


def checkpoint_parts(ckpt):
    """(encoder_type, stylegan_size, encoder state_dict, latent_avg or None) of an e4e / pSp checkpoint dict."""
    opts = ckpt.get("opts", {})
    if not isinstance(opts, dict):
        opts = vars(opts)
    encoder_type = opts.get("encoder_type", "Encoder4Editing")
    stylegan_size = int(opts.get("stylegan_size", 1024))
    sd = get_keys(ckpt, "encoder")
    if not sd:
        raise ValueError("checkpoint has no 'encoder.'-prefixed state_dict entries (psp.py:45)")
    latent_avg = ckpt.get("latent_avg") if opts.get("start_from_latent_avg", False) else None
    return encoder_type, stylegan_size, sd, latent_avg


def load_encoder(checkpoint=None, device="cuda", seed=5):
    from ..e4e_hip import build_e4e
    if checkpoint is None:
        return build_e4e(seed=seed, device=device)
    if not os.path.exists(checkpoint):
        raise SystemExit(f"checkpoint not found: {checkpoint}")
    ckpt = torch.load(checkpoint, map_location="cpu", weights_only=True)
    encoder_type, stylegan_size, sd, latent_avg = checkpoint_parts(ckpt)
    return build_e4e(state_dict=sd, device=device, encoder_type=encoder_type, stylegan_size=stylegan_size,
                     latent_avg=latent_avg)


def invert(net, image, device="cuda"):
    """W+ [1, style_count, 512] of one PIL image."""
    return net(preprocess(image).to(device))


def _cli():
    import click

    @click.command(help="Invert a face image to W+ with the e4e encoder on the HIP kernels and write "
                        "np.savez(out_file, w=[1, 18, 512]) for `w_s w_s_converter`.  The image is an aligned face "
                        "crop (taken as it is, resized to 256x256), or with --align any photograph of a face, which is "
                        "aligned first (stylemc_amd.align_faces).")
    @click.option("--input_image", type=str, required=True,
                  help="aligned face image, or with --align a photograph (any format PIL opens)")
    @click.option("--align", is_flag=True, help="detect the face and its landmarks and FFHQ-align the image first")
    @click.option("--mobilenet_checkpoint", type=str, default=None,
                  help="--align: landmark regressor checkpoint or 'synthetic' (default: align_faces' file name)")
    @click.option("--mtcnn_weights", type=str, default=None,
                  help="--align: MTCNN weights directory or 'synthetic' (default: align_faces' directory)")
    @click.option("--checkpoint", type=str, default=None,
                  help="e4e / pSp checkpoint (e4e_ffhq_encode.pt); default: the seeded synthetic encoder")
    @click.option("--out_file", type=str, default="encoder4editing/projected_w.npz", show_default=True)
    def main(input_image, align, mobilenet_checkpoint, mtcnn_weights, checkpoint, out_file):
        from PIL import Image
        if not os.path.exists(input_image):
            raise SystemExit(f"input image not found: {input_image}")
        image = Image.open(input_image)
        if align:
            from .. import align_faces
            image = align_faces.align_image(image, checkpoint=mobilenet_checkpoint or align_faces.DEFAULT_CHECKPOINT,
                                            mtcnn_weights=mtcnn_weights or align_faces.DEFAULT_MTCNN)
        net = load_encoder(checkpoint)
        w = invert(net, image)
        os.makedirs(os.path.dirname(out_file) or ".", exist_ok=True)
        np.savez(out_file, w=w.cpu().numpy())
        print(f"wrote {out_file}: w {tuple(w.shape)}")

    return main


if __name__ == "__main__":
    _cli()()
