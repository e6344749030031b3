"""ConvMLP, drop-in for the reference's models_pytorch/conv_mlp.py: the same classes, functions, constructor signatures, defaults and state_dict
keys and shapes.  Inference-only.  The classes, the packers and the forward are in `convmlp_impl.py` beside the engine (its docstring describes the
kernel sequence and says why they are defined there); this module gives them the reference's import path:
`from models_pytorch.conv_mlp import ConvMLP, convmlp_s, convmlp_m, convmlp_l`.  `model_urls` is the empty dict of the implementation: the tree
holds no checkpoint URL, and `pretrained=True` raises RuntimeError instead of downloading."""
from ..convmlp_impl import (  # noqa: F401
    __all__, model_urls, drop_path, DropPath, ConvTokenizer, ConvStage, Mlp, ConvMLPStage, ConvDownsample, BasicStage, ConvMLP,
    convmlp_s, convmlp_m, convmlp_l,
    conv_plan, conv3_columns, bn_scale_shift,
)
