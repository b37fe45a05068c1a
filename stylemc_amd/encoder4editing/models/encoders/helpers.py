"""Building blocks of the e4e / pSp encoders (encoder4editing/models/encoders/helpers.py of the reference).

The IR-SE bottleneck units are the ones the identity loss already uses (``stylemc_amd.id_loss.model_irse``: same
modules, same state_dict names as helpers.py:98-120); what this file adds is the FPN's ``_upsample_add``
(helpers.py:123-140) and the unit list of ``get_blocks`` (helpers.py:26-54).
"""
import torch.nn.functional as F

from ....id_loss.model_irse import STAGES, BottleneckIRSE


def get_units(num_layers, mode="ir_se"):
    """The body's bottleneck units in order (helpers.py:26-54 get_blocks, psp_encoders.py:137-142): every stage starts
    with a stride-2 unit."""
    assert num_layers in STAGES, "num_layers should be 50, 100, or 152"
    assert mode in ("ir", "ir_se"), "mode should be ir or ir_se"
    units = []
    for cin, depth, n in STAGES[num_layers]:
        units.append(BottleneckIRSE(cin, depth, 2, se=(mode == "ir_se")))
        units += [BottleneckIRSE(depth, depth, 1, se=(mode == "ir_se")) for _ in range(n - 1)]
    return units


def _upsample_add(x, y):
    """Bilinear (align_corners) upsampling of the top feature map x to the lateral map y's size, plus y
    (helpers.py:123-140)."""
    _, _, H, W = y.size()
    return F.interpolate(x, size=(H, W), mode="bilinear", align_corners=True) + y
