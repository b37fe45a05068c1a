"""HIP-backed mirrors of the reference's torch_utils.ops modules."""
from . import bias_act, conv2d_gradfix, conv2d_resample, upfirdn2d

__all__ = ["bias_act", "conv2d_gradfix", "conv2d_resample", "upfirdn2d"]
