"""RaftMLP, drop-in for the reference's models_pytorch/raft_mlp.py: the same module constants, class names, constructor signatures, defaults,
assertions and state_dict keys and shapes.  Inference-only, all four token_mixing_types.  The classes, the packers and the forward are in
`raft_impl.py` beside the engine (its docstring describes the kernel sequence and says why they are defined there); this module gives them the
reference's import path: `from models_pytorch.raft_mlp import RaftMLP, PermutedBlock, SER_PM, ...`."""
from ..raft_impl import (  # noqa: F401
    PATCH_SIZE, RAFT_SIZE, LOGGER_NAME, DIM, DEPTH, SER_PM, SEP_LN_CODIM_TM, SEP_LN_CH_TM, ORIGINAL_TM, TOKEN_MIXING_TYPES,
    Layout, DropPath, Block, ChannelBlock, TokenBlock, SpatiallySeparatedTokenBlock, PermutedBlock,
    Level, SeparatedLNCodimLevel, SeparatedLNChannelLevel, SerialPermutedLevel, OriginalLevel, RaftMLP,
    raft_affine, pad_token_mlp, embed_columns_nchw, classifier_columns_nhwc, fused_width, pack_token_mlp, pack_raft_half, pack_token_block,
)
