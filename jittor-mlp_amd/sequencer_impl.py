"""Sequencer2D, drop-in for the reference's models_pytorch/sequencer.py: the same classes, constructor signatures, defaults, the module-level
`sequencer_settings` table and the same state_dict keys and shapes (the LSTMs are real nn.LSTM modules that hold the parameters and are never
called); `models_pytorch/sequencer.py` gives them the reference's import path.  The classes are defined here, beside the engine, because every
EngineModule subclass defined under models_pytorch must have a row in the tables of tests/test_gpu_lifecycle.py; moving the family there is a
later change (DynaMixer arrived the same way).  Inference-only: train() takes the engine's warning path (Dropout runs as the identity).  The
einops `Reduce` slot of `mlp_head` is a `Layout` placeholder, so the head's Linear keeps index 1.

The forward runs on channel-last rows x[(b, h, w), c].  Per block (sequencer.py:49-72), hid = hidden_d_model:
  mean, rstd = row statistics of x                 the by-product of the previous GEMM's epilogue where it delivers them, else mlpk_row_stats
  xp = [v fwd | v rev | h fwd | h rev](LN(x))      ONE GEMM, N = 16 hid, LayerNorm folded in (engine.pack_ln_folded): the input projections
                                                   of both LSTMs, b_ih + b_hh folded into its bias at pack time (`cat_lstm_ih`)
  cat[:, 0:2 hid]     = rnn_v                      mlpk_lstm_scan, axis 0, on columns [0, 8 hid) of xp   (csrc/mlpk_lstm.hip)
  cat[:, 2 hid:4 hid] = rnn_h                      mlpk_lstm_scan, axis 1, on columns [8 hid, 16 hid): torch.cat (:44) costs nothing
  x += fc(cat)                                     ONE GEMM with K = 4 hid, the residual in its epilogue
then the channel MLP (common.channel_mlp, LayerNorm folded into fc1).  Stage 1 embeds the NCHW image (embed_patches, 7 x 7), stage 2 the
channel-last rows (stage_embed, 2 x 2), stages 3 and 4 are a plain GEMM (1 x 1); there is no final norm; the head is mlpk_pool_mean and one GEMM.

`Sequencer2D`, `Sequencer2DBlock` (NCHW in and out) and `BiLSTM2D` ((B, H, W, C) in and out) run on their own on the GPU.  `PreNormResidual`
and `PatchEmbedOverlap` hold parameters and raise NotImplementedError when called.  A hidden width mlpk_lstm_scan does not take (anything but
16, 32, 48, 96) raises NotImplementedError naming it; there is no fallback path.
"""
import torch
from torch import nn

from . import _native as N
from . import engine as E
from .models_pytorch.common import SubModule, channel_mlp, embed_patches, finalize_stats, head_linear, layernorm_stats, pack_channel_mlp, stage_embed


class Layout(nn.Module):
    """Stands where the reference has a parameterless einops layer (Reduce): keeps the indices of the module tree, and with them the
    state_dict keys.  The reduction itself is mlpk_pool_mean."""

    def __init__(self, pattern=""):
        super().__init__()
        self.pattern = pattern

    def extra_repr(self):
        return repr(self.pattern)

    def forward(self, x):
        raise NotImplementedError("Layout(%r) is a placeholder inside Sequencer2D: call the enclosing Sequencer2D" % self.pattern)


class _Container(nn.Module):
    """Holds parameters; the enclosing block packs them into its own kernel sequence and never calls the module."""

    def forward(self, *a, **k):
        raise NotImplementedError("%s only holds parameters inside Sequencer2D: call the enclosing Sequencer2D, Sequencer2DBlock or BiLSTM2D" % type(self).__name__)


class PatchEmbedOverlap(_Container):
    """sequencer.py:11-20 (the reference's Sequencer2D does not use it)"""

    def __init__(self, patch_size=16, stride=16, padding=0, embed_dim=768):
        super().__init__()
        self.proj = nn.Conv2d(3, embed_dim, patch_size, stride, padding)
        self.norm = nn.BatchNorm2d(embed_dim)


class PreNormResidual(_Container):
    """sequencer.py:22-29"""

    def __init__(self, dim, fn):
        super().__init__()
        self.fn = fn
        self.norm = nn.LayerNorm(dim)


# ------------------------------------------------------------------ packing (pure functions: they run on CPU tensors too)
def cat_lstm_ih(rnns, device):
    """the input projections of the given bidirectional nn.LSTMs as one (len(rnns) 8 hid, C) fp32 weight and its bias: per LSTM
    [forward: i f g o | reverse: i f g o] as torch holds the gates, bias = bias_ih + bias_hh (both are added to the same pre-activation)"""
    f = lambda v: v.detach().to(device=device, dtype=torch.float32)
    w = torch.cat([f(getattr(r, "weight_ih_l0" + sfx)) for r in rnns for sfx in ("", "_reverse")], 0)
    b = torch.cat([f(getattr(r, "bias_ih_l0" + sfx)) + f(getattr(r, "bias_hh_l0" + sfx)) for r in rnns for sfx in ("", "_reverse")], 0)
    return w.contiguous(), b.contiguous()


def pack_bilstm(pk, p, mod, norm, dtype, device):
    """a BiLSTM2D under prefix p; norm = the PreNormResidual's LayerNorm (folded into the projection GEMM), or None for the module on its own"""
    w, b = cat_lstm_ih([mod.rnn_v, mod.rnn_h], device)
    if norm is not None:
        pk[p + "ih.w"], pk[p + "ih.b"], pk[p + "ih.csum"] = E.pack_ln_folded(w, b, norm.weight, norm.bias, dtype, device)
    else:
        pk[p + "ih.w"], pk[p + "ih.b"] = E.pack_matrix(w, dtype, device), E.f32(b, device)
    for k, r in (("v.", mod.rnn_v), ("h.", mod.rnn_h)):
        pk[p + k + "hh"] = E.pack_lstm_hh(r.weight_hh_l0, r.weight_hh_l0_reverse, dtype, device)
    pk[p + "fc.w"], pk[p + "fc.b"] = E.pack_matrix(mod.fc.weight, dtype, device), E.f32(mod.fc.bias, device)


def pack_layers(pk, p, block, dtype, device):
    """a Sequencer2DBlock's layers under prefix p"""
    for j, (mix, ff) in enumerate(block.model):
        q = "%sb%d." % (p, j)
        pack_bilstm(pk, q, mix.fn[0], mix.norm, dtype, device)
        pack_channel_mlp(pk, q + "ff.", ff.norm, ff.fn[0], ff.fn[3], dtype, device)


# ------------------------------------------------------------------ forward pieces on channel-last rows
def require_hidden(what, dtype, H, W, hid):
    if not (E.lstm_scan_supported(dtype, H, hid) and E.lstm_scan_supported(dtype, W, hid)):
        raise NotImplementedError("%s: mlpk_lstm_scan does not take a hidden width of %d (16, 32, 48 or 96) in %s" % (what, hid, dtype))


def bilstm_rows(ws, pk, p, src, stats, B, H, W, C, hid, tag, out, residual):
    """BiLSTM2D on rows: out = [out +] fc([rnn_v | rnn_h]) of LayerNorm(src) (stats None: of `src` as it is).  Returns what the last GEMM's
    `part` delivered (residual only)."""
    rows = B * H * W
    xp = ws.get(tag + ".xp", (rows, 16 * hid))
    ln = (stats[0], stats[1], pk[p + "ih.csum"]) if stats is not None else None
    E.gemm(src, pk[p + "ih.w"], xp, rows, 16 * hid, C, bias=pk[p + "ih.b"], ln=ln, tag="lstm_ih")
    cat = ws.get(tag + ".cat", (rows, 4 * hid))
    E.lstm_scan(xp, 0, pk[p + "v.hh"], cat, 0, B, H, W, hid, 0)
    E.lstm_scan(xp, 8 * hid, pk[p + "h.hh"], cat, 2 * hid, B, H, W, hid, 1)
    if residual:
        return E.gemm(cat, pk[p + "fc.w"], out, rows, C, 4 * hid, bias=pk[p + "fc.b"], R=out, res=N.RES_ADD, tag="lstm_fc", part=(ws, tag + ".fc.part"))
    E.gemm(cat, pk[p + "fc.w"], out, rows, C, 4 * hid, bias=pk[p + "fc.b"], tag="lstm_fc")
    return None


def layers_rows(ws, pk, p, depth, cur, B, H, W, C, hid, hidden, tag):
    """a Sequencer2DBlock's layers in place on rows (B*H*W, C)"""
    rows = B * H * W
    st = None
    for j in range(depth):
        q = "%sb%d." % (p, j)
        if st is None:
            st = layernorm_stats(ws, cur, rows, C, tag=tag + ".ln")
        got = bilstm_rows(ws, pk, q, cur, st, B, H, W, C, hid, tag, cur, residual=True)
        got = channel_mlp(ws, cur, rows, C, pk, q + "ff.", hidden, tag=tag + ".cm", stats=finalize_stats(ws, got, rows, C, tag=tag + ".cm.ln"),
                          part=(ws, tag + ".fc2.part"))
        st = finalize_stats(ws, got, rows, C, tag=tag + ".ln")


class BiLSTM2D(SubModule):
    """sequencer.py:31-46.  Callable on its own like the reference's: x (B, H, W, C) -> (B, H, W, C)."""

    def __init__(self, d_model, hidden_d_model):
        super().__init__()
        self.rnn_v = nn.LSTM(d_model, hidden_d_model, num_layers=1, batch_first=True, bias=True, bidirectional=True)
        self.rnn_h = nn.LSTM(d_model, hidden_d_model, num_layers=1, batch_first=True, bias=True, bidirectional=True)
        self.fc = nn.Linear(4 * hidden_d_model, d_model)

    def _pack(self, dtype, device):
        pk = {}
        pack_bilstm(pk, "", self, None, dtype, device)
        return pk

    def forward(self, x):
        C, hid = self.fc.out_features, self.rnn_v.hidden_size
        pk = self._begin(x, C)
        if x.dim() != 4:
            raise ValueError("expected a channel-last (B, H, W, %d) tensor, got %s" % (C, tuple(x.shape)))
        B, H, W, _ = x.shape
        require_hidden("BiLSTM2D", x.dtype, H, W, hid)
        rows = B * H * W
        with E.on_device(x):
            ws = self._get_space((B, H, W), x.dtype, x.device)
            xb = ws.get("bl.x", (rows, E.round_up(C, 8)))
            xb[:, :C].copy_(x.reshape(rows, C))
            out = ws.get("bl.out", (rows, C))
            bilstm_rows(ws, pk, "", xb, None, B, H, W, xb.shape[1], hid, "bl", out, residual=False)
            return out.reshape(B, H, W, C).clone()


class Sequencer2DBlock(SubModule):
    """sequencer.py:49-72.  Callable on its own like the reference's: x (B, C, H, W) -> (B, C, H, W)."""

    def __init__(self, d_model, depth, hidden_d_model, expansion_factor=3, dropout=0.):
        super().__init__()
        self.model = nn.Sequential(
            *[nn.Sequential(
                PreNormResidual(d_model, nn.Sequential(
                    BiLSTM2D(d_model, hidden_d_model)
                )),
                PreNormResidual(d_model, nn.Sequential(
                    nn.Linear(d_model, d_model * expansion_factor),
                    nn.GELU(),
                    nn.Dropout(dropout),
                    nn.Linear(d_model * expansion_factor, d_model),
                    nn.Dropout(dropout)
                ))
            ) for _ in range(depth)]
        )
        self.__dict__["_geom"] = (depth, d_model, hidden_d_model, d_model * expansion_factor)

    def _pack(self, dtype, device):
        pk = {}
        pack_layers(pk, "", self, dtype, device)
        return pk

    def forward(self, x):
        depth, C, hid, hidden = self.__dict__["_geom"]
        pk = self._begin(x, C, axis=1)
        if x.dim() != 4:
            raise ValueError("expected a (B, %d, H, W) tensor, got %s" % (C, tuple(x.shape)))
        B, _, H, W = x.shape
        require_hidden("Sequencer2DBlock", x.dtype, H, W, hid)
        rows = B * H * W
        with E.on_device(x):
            ws = self._get_space((B, H, W), x.dtype, x.device)
            cur = ws.get("sb.x", (rows, C))
            cur.view(B, H, W, C).copy_(x.permute(0, 2, 3, 1))
            layers_rows(ws, pk, "", depth, cur, B, H, W, C, hid, hidden, "sb")
            return cur.view(B, H, W, C).permute(0, 3, 1, 2).clone(memory_format=torch.contiguous_format)


sequencer_settings = {
    'S': [[4, 3,  8, 3], [192, 384, 384, 384], [48, 96, 96, 96], 3],
    'M': [[4, 3, 14, 3], [192, 384, 384, 384], [48, 96, 96, 96], 3],
    'L': [[8, 8, 16, 4], [192, 384, 384, 384], [48, 96, 96, 96], 3]
}


class Sequencer2D(E.EngineModule):
    """sequencer.py:74-98.  Inference-only (no `_train_forward`): in train mode the forward warns and runs as in eval mode."""

    def __init__(self, model_name: str = 'M', pretrained: str = None, num_classes: int = 1000, in_channels=3, *args, **kwargs) -> None:
        super().__init__()
        assert model_name in sequencer_settings.keys(), f"Sequencer model name should be in {list(sequencer_settings.keys())}"
        depth, embed_dims, hidden_dims, expansion_factor = sequencer_settings[model_name]

        self.patch_size = [7, 2, 1, 1]

        self.stage = len(depth)
        self.stages = nn.Sequential(
            *[nn.Sequential(
                nn.Conv2d(in_channels if i == 0 else embed_dims[i - 1], embed_dims[i], kernel_size=self.patch_size[i], stride=self.patch_size[i]),
                Sequencer2DBlock(embed_dims[i], depth[i], hidden_dims[i], expansion_factor, dropout=0.)
            ) for i in range(self.stage)]
        )

        self.mlp_head = nn.Sequential(
            Layout('b c h w -> b c (mean)'),
            nn.Linear(embed_dims[-1], num_classes)
        )
        self.__dict__["_in_channels"] = in_channels

    # ------------------------------------------------------------------ packing
    def _pack(self, dtype, device):
        pk = {}
        for i, stage in enumerate(self.stages):
            conv = stage[0]
            w = conv.weight.detach()
            if i:
                w = w.permute(0, 2, 3, 1)                                   # (i, j, ci): the channel-last rows' patch order
            kpad = E.embed_kpad(dtype) if i == 0 else 8
            pk["s%d.embed.w" % i] = E.pack_matrix(w.reshape(w.shape[0], -1), dtype, device, kpad=kpad)
            pk["s%d.embed.b" % i] = E.f32(conv.bias, device)
            pack_layers(pk, "s%d." % i, stage[1], dtype, device)
        pk["head.w"], pk["head.b"] = E.pack_matrix(self.mlp_head[1].weight, dtype, device), E.f32(self.mlp_head[1].bias, device)
        return pk

    # ------------------------------------------------------------------ forward
    def forward(self, x):
        cd = self._resolve(x)
        B, cin, H, W = x.shape
        total = 1
        for ps in self.patch_size:
            total *= ps
        if cin != self.__dict__["_in_channels"] or H < total or W < total or H % total or W % total:
            raise ValueError("expected a (B, %d, H, W) tensor with H and W multiples of %d, got %s" % (self.__dict__["_in_channels"], total, tuple(x.shape)))
        h, w = H, W
        for i, stage in enumerate(self.stages):                            # before anything is launched
            h, w = h // self.patch_size[i], w // self.patch_size[i]
            require_hidden("Sequencer2D stage %d" % (i + 1), cd, h, w, stage[1].__dict__["_geom"][2])
        pk = self._get_pack(cd, x.device)
        ws = self._get_space(B, cd, x.device)
        cur = x.contiguous()
        for i, stage in enumerate(self.stages):
            depth, C, hid, hidden = stage[1].__dict__["_geom"]
            ps = self.patch_size[i]
            name = "s%d.embed" % i
            if i == 0:
                cur, H, W = embed_patches(ws, name, cur, pk[name + ".w"], pk[name + ".b"], cd, (ps, ps))
            elif ps > 1:
                cur, H, W = stage_embed(ws, name, cur, B, cin, H, W, pk[name + ".w"], pk[name + ".b"], (ps, ps), channel_last=True)
            else:
                nxt = ws.get(name + ".x", (B * H * W, C))
                E.gemm(cur, pk[name + ".w"], nxt, B * H * W, C, cin, bias=pk[name + ".b"], tag="stage_embed")
                cur = nxt
            layers_rows(ws, pk, "s%d." % i, depth, cur, B, H, W, C, hid, hidden, "s%d" % i)
            cin = C
        pooled = ws.get("pooled", (B, cin))
        E.pool_mean(cur, B, H * W, cin, cin, pooled, cin)
        return head_linear(ws, pooled, B, cin, pk["head.w"], pk["head.b"], self.mlp_head[1].out_features, x.dtype)
