"""Sequencer2D, drop-in for the reference's models_pytorch/sequencer.py: the same classes, constructor signatures, defaults, `sequencer_settings`
and state_dict keys and shapes.  Inference-only.  The classes, the packers and the forward are in `sequencer_impl.py` beside the engine (its
docstring describes the kernel sequence and says why they are defined there); this module gives them the reference's import path:
`from models_pytorch.sequencer import Sequencer2D, Sequencer2DBlock, BiLSTM2D, sequencer_settings`.  `sequencer_settings` is the one dict object
the constructor reads: an entry added here is seen there."""
from ..sequencer_impl import (  # noqa: F401
    Layout, PatchEmbedOverlap, PreNormResidual, BiLSTM2D, Sequencer2DBlock, sequencer_settings, Sequencer2D,
    cat_lstm_ih, pack_bilstm, pack_layers,
)
