"""ActiveMLP, drop-in for the reference's models_pytorch/active_mlp.py: the same class names, constructor signatures, defaults, state_dict keys
and shapes, and the five factories.  Inference-only.  The classes, the packers and the forward are in `active_impl.py` beside the engine (its
docstring describes the kernel sequence, says what of the reference's constructor is not reproduced -- the argument print through a broken import and
timm's `default_cfg` -- and why the classes are defined there); this module gives them the reference's import path:
`from models_pytorch.active_mlp import ActiveMLP, ATMLayer, ActiveTiny, ...`."""
from ..active_impl import (  # noqa: F401
    Mlp, ATMOp, ATMLayer, ActiveBlock, Downsample, PEG, OverlapPatchEmbed, ActiveMLP, ActivexTiny, ActiveTiny, ActiveSmall, ActiveBase, ActiveLarge,
    fusion_rows, peg_taps, pack_atm,
)
