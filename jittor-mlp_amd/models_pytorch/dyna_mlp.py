"""DynaMixer, drop-in for the reference's models_pytorch/dyna_mlp.py: the same classes, constructor signatures, defaults, `dynamlp_settings` and
state_dict keys and shapes.  Inference-only.  The classes, the packers and the forward are in `dyna_impl.py` beside the engine (its docstring
describes the kernel sequence and says why they are defined there); this module gives them the reference's import path:
`from models_pytorch.dyna_mlp import DynaMixer, DynaMLPBlock, DynaBlock, DynaMixerOp_h, DynaMixerOp_w, dynamlp_settings`.  `dynamlp_settings`
is the one dict object the constructor reads: an entry added here is seen there."""
from ..dyna_impl import (  # noqa: F401
    pair, Layout, PreNorm, FeedForward, DropPath, DynaMixerOp_w, DynaMixerOp_h, DynaBlock, DynaMLPBlock, dynamlp_settings, DynaMixer,
    cat_wd, fold_projections, pack_op, pack_block, pack_layers,
)
