"""RaftMLP, drop-in for the reference's models_pytorch/raft_mlp.py: same module constants, class names, constructor signatures, defaults, assertions
and state_dict keys and shapes, under the reference's import path: `from models_pytorch.raft_mlp import RaftMLP, PermutedBlock, SER_PM, ...`.
Inference-only, all four token_mixing_types: train() takes the engine's warning path (dropout / drop path are accepted and run as identity).

The forward runs on channel-last rows x[(b, h, w), c]; the parameterless einops slots of the reference's module tree are `Layout` placeholders.
  Level embedding   the (p1 p2 c) patch Linear: level 0 from the NCHW image through embed_patches (weight columns permuted to (c, p1, p2) at pack
                    time); later levels through mlpk_conv_gemm_nhwc (window p x p, stride p: already (p1 p2 c)) or the window gather + GEMM where it
                    refuses; a level whose size its patch does not divide interpolates first, as Level.forward does (torch, on an NCHW view)
  ser_pm / sep_ln_ch_tm   per axis (vertical, then horizontal), with r = raft_size (1 for sep_ln_ch_tm), c = j Co + co, z[j L + l]:
      mean, rstd = row statistics of x                                  mlpk_row_stats
      a[(b, q, co), j L + l] = LayerNorm(x)[b, pix(l, q), j Co + co]    mlpk_raft_gather_ln (the affine permuted from the reference's (co, j) order)
      y = W2 gelu(W1 a + b1) + b2                                       mlpk_channel_mlp on D = r L zero-padded to a multiple of 32 where it takes
                                                                        (padded D, T) -- 16-bit, 64 <= padded D <= 192 --, else two GEMMs
      x[b, pix(l, q), j Co + co] += y[(b, q, co), j L + l]              mlpk_raft_scatter_add
  original_tm / sep_ln_codim_tm   existing kernels with torch permutes around them (`token_mix_rows`): no new kernel, no performance claim
  channel mixer     common.channel_mlp, as in every family
  heads             LayerNorm statistics + mlpk_pool_mean (+ the Linear to 2 x the last width), the FiLM-style reduce over levels as torch
                    elementwise operations in fp32 on (B, <= 2 dim) tensors (gap=False: on the last level's normalised map), then the classifier GEMM
                    (gap=False: its columns permuted from (c h w) to (h w c) at pack time)
`PermutedBlock`, `SpatiallySeparatedTokenBlock` and `ChannelBlock` run on their own on the reference's 3-D layouts; `TokenBlock` and the Level
classes hold parameters.
"""
import math
from typing import Dict, List

import torch
from torch import nn
from torch.nn import functional as F

from .. import _native as N
from .. import engine as E
from .common import SubModule, channel_mlp, embed_patches, head_linear, layernorm_stats, pack_channel_mlp

PATCH_SIZE = "patch_size"
RAFT_SIZE = "raft_size"
LOGGER_NAME = "RaftMLP"
DIM = "dim"
DEPTH = "depth"
SER_PM = "ser_pm"
SEP_LN_CODIM_TM = "sep_ln_codim_tm"
SEP_LN_CH_TM = "sep_ln_ch_tm"
ORIGINAL_TM = "original_tm"

TOKEN_MIXING_TYPES = [
    SER_PM,
    SEP_LN_CODIM_TM,
    SEP_LN_CH_TM,
    ORIGINAL_TM,
]


class Layout(nn.Module):
    """Stands where the reference has a parameterless einops layer (Rearrange / Reduce): keeps the indices of the module tree, and with them the
    state_dict keys.  The layout change itself is index arithmetic inside the kernels of the enclosing model's forward."""

    def __init__(self, pattern=""):
        super().__init__()
        self.pattern = pattern

    def extra_repr(self):
        return repr(self.pattern)

    def forward(self, x):
        raise NotImplementedError("Layout(%r) is a placeholder inside RaftMLP: call the enclosing RaftMLP or one of its callable blocks" % self.pattern)


class DropPath(nn.Module):
    """raft_mlp.py:32-44: per-sample stochastic depth in train mode, identity otherwise."""

    def __init__(self, drop_path_rate=None):
        super(DropPath, self).__init__()
        self.drop_prob = drop_path_rate

    def forward(self, x):
        if self.drop_prob == 0.0 or not self.training:
            return x
        keep = 1 - self.drop_prob
        mask = torch.floor(keep + torch.rand((x.shape[0],) + (1,) * (x.ndim - 1), dtype=x.dtype, device=x.device))
        return x.div(keep) * mask


# ------------------------------------------------------------------ packing (pure functions: they run on CPU tensors too)
def raft_affine(v, r):
    """PermutedBlock's LayerNorm parameter, stored by the reference in (co, j) order, indexed by the activation's channel j * Co + co"""
    v = v.detach().reshape(-1)
    return v.reshape(v.numel() // r, r).t().reshape(-1).contiguous()


def pad_token_mlp(w1, b1, w2, b2, dp):
    """fp32 W1 (T, D) -> (T, dp), W2 (D, T) -> (dp, T), b2 (D) -> (dp): zero columns / rows for the operand's zero padding"""
    w1, w2 = w1.detach().float(), w2.detach().float()
    T, D = w1.shape
    w1p = torch.zeros((T, dp), dtype=torch.float32, device=w1.device)
    w1p[:, :D] = w1
    w2p = torch.zeros((dp, T), dtype=torch.float32, device=w2.device)
    w2p[:D] = w2
    b2p = torch.zeros((dp,), dtype=torch.float32, device=w2.device)
    b2p[:D] = b2.detach().float()
    return w1p, b1.detach().float(), w2p, b2p


def embed_columns_nchw(w, p, cin):
    """the patch Linear's columns from the reference's (p1 p2 c) order to mlpk_patchify's NCHW order (c, p1, p2)"""
    w = w.detach()
    return w.reshape(w.shape[0], p, p, cin).permute(0, 3, 1, 2).reshape(w.shape[0], -1).contiguous()


def classifier_columns_nhwc(w, C, S):
    """gap=False: the classifier's columns from the reference's flatten of (c, h, w) to the channel-last (h w, c)"""
    w = w.detach()
    return w.reshape(w.shape[0], C, S).permute(0, 2, 1).reshape(w.shape[0], -1).contiguous()


def fused_width(D):
    return E.round_up(D, 32)


def pack_token_mlp(pk, p, fn, dtype, device):
    """the two Linears of a Block's `fn` over vectors of length D: the fused entry where mlpk_channel_mlp takes (D padded to 32, T), and always the
    GEMM pair's weights (K zero-padded to whole 16-byte chunks)"""
    fc1, fc2 = fn[0], fn[3]
    T, D = fc1.weight.shape
    pk[p + "fc1.w"], pk[p + "fc1.b"] = E.pack_matrix(fc1.weight, dtype, device), E.f32(fc1.bias, device)
    pk[p + "fc2.w"], pk[p + "fc2.b"] = E.pack_matrix(fc2.weight, dtype, device), E.f32(fc2.bias, device)
    dp = fused_width(D)
    if E.channel_mlp_fused_supported(dtype, dp, T):
        w1p, b1, w2p, b2p = pad_token_mlp(fc1.weight, fc1.bias, fc2.weight, fc2.bias, dp)
        pk[p + "fused"] = E.pack_channel_mlp_fused(w1p, b1, w2p, b2p, dtype, device)


def pack_raft_half(pk, p, blk, r, dtype, device):
    """a PermutedBlock (r = raft_size) or SpatiallySeparatedTokenBlock (r = 1) under prefix p"""
    ln = blk.norm[1]
    pk[p + "ln.g"], pk[p + "ln.b"] = E.f32(raft_affine(ln.weight, r), device), E.f32(raft_affine(ln.bias, r), device)
    pack_token_mlp(pk, p, blk.fn, dtype, device)


def pack_token_block(pk, p, blk, perm, dtype, device):
    """a TokenBlock: LayerNorm over `channels` (its affine re-ordered by `perm` = (outer, inner) of the reference's order, or None) + the token MLP"""
    ln = blk.norm[1]
    g, b = ln.weight.detach(), ln.bias.detach()
    if perm is not None:
        g, b = g.reshape(perm).t().reshape(-1), b.reshape(perm).t().reshape(-1)
    pk[p + "ln.g"], pk[p + "ln.b"] = E.f32(g.contiguous(), device), E.f32(b.contiguous(), device)
    fc1, fc2 = blk.fn[0], blk.fn[3]
    pk[p + "fc1.w"], pk[p + "fc1.b"] = E.pack_matrix(fc1.weight, dtype, device), E.f32(fc1.bias, device)
    pk[p + "fc2.w"], pk[p + "fc2.b"] = E.pack_matrix(fc2.weight, dtype, device), E.f32(fc2.bias, device)


# ------------------------------------------------------------------ forward pieces on channel-last rows
def token_mlp_rows(ws, pk, p, a, rows, D, tag):
    """y = W2 gelu(W1 a + b1) + b2 on rows a (rows, K >= D, zero beyond D) by two GEMMs; returns y (rows, D padded to 8)"""
    T = pk[p + "fc1.w"].shape[0]
    h = ws.get(tag + ".h", (rows, pk[p + "fc2.w"].shape[1]))
    y = ws.get(tag + ".y", (rows, E.round_up(D, 8)))
    E.gemm(a, pk[p + "fc1.w"], h, rows, T, pk[p + "fc1.w"].shape[1], bias=pk[p + "fc1.b"], act=N.ACT_GELU, tag="raft_fc1")
    E.gemm(h, pk[p + "fc2.w"], y, rows, D, h.shape[1], bias=pk[p + "fc2.b"], tag="raft_fc2")
    return y


def raft_half(ws, pk, p, cur, B, H, W, C, r, axis, tag):
    """one PermutedBlock / SpatiallySeparatedTokenBlock in place on rows (B*H*W, C): statistics, gather, the MLP, scatter"""
    rows = B * H * W
    L, Q = (H, W) if axis == 0 else (W, H)
    D, ra = r * L, B * Q * (C // r)
    mean, rstd = layernorm_stats(ws, cur, rows, C, tag=tag + ".ln")
    if (p + "fused") in pk:
        dp = fused_width(D)
        a = ws.get(tag + ".a", (ra, dp))
        E.raft_gather_ln(cur, mean, rstd, pk[p + "ln.g"], pk[p + "ln.b"], a, dp, B, H, W, C, r, axis)
        y = ws.get(tag + ".y", (ra, dp))
        E.channel_mlp_fused(a, ra, dp, pk[p + "fused"], y)
    else:
        kp = pk[p + "fc1.w"].shape[1]
        a = ws.get(tag + ".a", (ra, kp))
        E.raft_gather_ln(cur, mean, rstd, pk[p + "ln.g"], pk[p + "ln.b"], a, kp, B, H, W, C, r, axis)
        y = token_mlp_rows(ws, pk, p, a, ra, D, tag)
    E.raft_scatter_add(cur, y, B, H, W, C, r, axis)


def token_mix_rows(ws, pk, p, x3, tag):
    """a TokenBlock in place on a contiguous (B, S, R) tensor: LayerNorm over R per (b, s), the MLP over S per (b, r), the residual.  Existing
    kernels; the two transposes are torch copies."""
    B, S, R = x3.shape
    rows = B * S
    flat = x3.view(rows, R)
    mean, rstd = layernorm_stats(ws, flat, rows, R, tag=tag + ".ln")
    xn = ws.get(tag + ".xn", (rows, R))
    E.norm_apply(flat, rows, R, R, mean=mean, rstd=rstd, gamma=pk[p + "ln.g"], beta=pk[p + "ln.b"], out_rm=xn, ld_rm=R)
    kp = pk[p + "fc1.w"].shape[1]
    a = ws.get(tag + ".a", (B * R, kp))
    a.view(B, R, kp)[:, :, :S].copy_(xn.view(B, S, R).transpose(1, 2))
    y = token_mlp_rows(ws, pk, p, a, B * R, S, tag)
    x3.add_(y.view(B, R, y.shape[1])[:, :, :S].transpose(1, 2))


class Block(SubModule):
    """raft_mlp.py:47-65: fn(norm(x)) + x with fn = Linear -> GELU -> Dropout -> Linear -> Dropout.  The base class and TokenBlock hold parameters;
    ChannelBlock, SpatiallySeparatedTokenBlock and PermutedBlock are callable on their own."""

    def __init__(self, dim, expansion_factor=4, dropout=0.0, drop_path_rate=0.0):
        super().__init__()
        self.norm = nn.Identity()
        self.drop = DropPath(drop_path_rate) if drop_path_rate > 0.0 else nn.Identity()
        self.fn = nn.Sequential(
            nn.Linear(dim, dim * expansion_factor),
            nn.GELU(),
            nn.Dropout(dropout),
            nn.Linear(dim * expansion_factor, dim),
            nn.Dropout(dropout),
        )

    def forward(self, x):
        raise NotImplementedError("%s only holds parameters inside RaftMLP: call the enclosing RaftMLP" % type(self).__name__)


class ChannelBlock(Block):
    """raft_mlp.py:68-73: the channel mixer, on the last dimension."""

    def __init__(self, dim, expansion_factor=4, dropout=0.0, drop_path_rate=0.0):
        super().__init__(dim, expansion_factor, dropout, drop_path_rate)
        self.norm = nn.LayerNorm(dim)

    def _pack(self, dtype, device):
        pk = {}
        pack_channel_mlp(pk, "", self.norm, self.fn[0], self.fn[3], dtype, device)
        return pk

    def forward(self, x):
        C = self.norm.normalized_shape[0]
        pk = self._begin(x, C)
        rows = x.numel() // C
        with E.on_device(x):
            ws = self._get_space(rows, x.dtype, x.device)
            xb = ws.get("cb.x", (rows, C))
            xb.copy_(x.reshape(rows, C))
            channel_mlp(ws, xb, rows, C, pk, "", self.fn[0].out_features, eps=self.norm.eps)
            return xb.reshape(x.shape).clone()


class TokenBlock(Block):
    """raft_mlp.py:76-92: LayerNorm over `channels` (dimension 1), the MLP over dimension 2.  A parameter container."""

    def __init__(self, dim, channels, expansion_factor=4, dropout=0.0, drop_path_rate=0.0):
        super().__init__(dim, expansion_factor, dropout, drop_path_rate)
        self.norm = nn.Sequential(*[Layout("b c o -> b o c"), nn.LayerNorm(channels), Layout("b o c -> b c o")])


class _RaftBlock(Block):
    """the two blocks the raft kernels serve, on the reference's layout (b, Co * other, r * spatial): dimension 1 = (co, the other spatial axis),
    dimension 2 = (j, this axis)"""

    def _geometry(self):
        raise NotImplementedError

    def _pack(self, dtype, device):
        pk = {}
        pack_raft_half(pk, "", self, self._geometry()[2], dtype, device)
        return pk

    def forward(self, x):
        L, C, r = self._geometry()
        pk = self._begin(x, r * L)
        Co = C // r
        if x.dim() != 3 or x.shape[1] % Co:
            raise ValueError("expected a (B, %d * n, %d) tensor" % (Co, r * L))
        B, O = x.shape[0], x.shape[1] // Co
        if not E.raft_supported(x.dtype, L, O, C, r, 0):
            raise NotImplementedError("%s: mlpk_raft_gather_ln does not take channels = %d in %s" % (type(self).__name__, C, x.dtype))
        with E.on_device(x):
            ws = self._get_space((B, O), x.dtype, x.device)
            cur = ws.get("rb.x", (B * L * O, C))                       # the map (B, H = L, W = O, C), this block's axis vertical
            cur.view(B, L, O, r, Co).copy_(x.reshape(B, Co, O, r, L).permute(0, 4, 2, 3, 1))
            raft_half(ws, pk, "", cur, B, L, O, C, r, 0, "rb")
            return cur.view(B, L, O, r, Co).permute(0, 4, 2, 3, 1).clone(memory_format=torch.contiguous_format).reshape(x.shape)


class SpatiallySeparatedTokenBlock(_RaftBlock):
    """raft_mlp.py:95-111: per-pixel LayerNorm over the channels, the MLP along one spatial axis (raft size 1)."""

    def __init__(self, dim, channels, expansion_factor=4, dropout=0.0, drop_path_rate=0.0):
        super().__init__(dim, expansion_factor, dropout, drop_path_rate)
        self.norm = nn.Sequential(*[Layout("b (c o1) o2 -> b (o1 o2) c"), nn.LayerNorm(channels), Layout("b (o1 o2) c -> b (c o1) o2")])

    def _geometry(self):
        return self.fn[0].in_features, self.norm[1].normalized_shape[0], 1


class PermutedBlock(_RaftBlock):
    """raft_mlp.py:114-146: per-pixel LayerNorm over the channels (affine in (co, j) order), the MLP over raft_size channel groups x one
    spatial axis."""

    def __init__(self, spatial_dim, channels, raft_size, expansion_factor=4, dropout=0.0, drop_path_rate=0.0):
        super().__init__(spatial_dim * raft_size, expansion_factor, dropout, drop_path_rate)
        self.norm = nn.Sequential(*[Layout("b (c1 o1) (c2 o2) -> b (o1 o2) (c1 c2)"), nn.LayerNorm(channels),
                                    Layout("b (o1 o2) (c1 c2) -> b (c1 o1) (c2 o2)")])
        self.__dict__["_geom"] = (spatial_dim, channels, raft_size)

    def _geometry(self):
        return self.__dict__["_geom"]


class Level(nn.Module):
    """raft_mlp.py:149-165: one resolution level, `fn` = [layout, patch Linear (or Identity), depth x block sequence, layout].  A parameter
    container: the enclosing RaftMLP runs it."""

    def __init__(self, image_size=224, patch_size=4):
        super().__init__()
        self.patch_size = patch_size
        self.fn = nn.Identity()
        self._bh = self._bw = image_size // patch_size
        self._h = self._w = math.ceil(image_size / patch_size)

    def _embedding(self, in_channels, out_channels):
        p = self.patch_size
        return nn.Linear((p ** 2) * in_channels, out_channels) if p != 1 or in_channels == out_channels else nn.Identity()

    def _build(self, embedding, blocks):
        self.fn = nn.Sequential(*[Layout("b c (h p1) (w p2) -> b (h w) (p1 p2 c)"), embedding, *blocks, Layout("b (h w) c -> b c h w")])

    def forward(self, input):
        raise NotImplementedError("%s only holds parameters inside RaftMLP: call the enclosing RaftMLP" % type(self).__name__)


class SeparatedLNCodimLevel(Level):
    """raft_mlp.py:168-232"""

    def __init__(self, in_channels, out_channels, depth=4, image_size=224, patch_size=4, token_expansion_factor=2, channel_expansion_factor=4,
                 dropout=0.0, drop_path_rate=0.0):
        super().__init__(image_size, patch_size)
        self._build(self._embedding(in_channels, out_channels), [nn.Sequential(*[
            Layout("b (h w) c -> b (c w) h"),
            TokenBlock(self._h, out_channels * self._w, token_expansion_factor, dropout, drop_path_rate),
            Layout("b (c w) h -> b (c h) w"),
            TokenBlock(self._w, out_channels * self._h, token_expansion_factor, dropout, drop_path_rate),
            Layout("b (c h) w -> b (h w) c"),
            ChannelBlock(out_channels, channel_expansion_factor, dropout, drop_path_rate),
        ]) for _ in range(depth)])


class SeparatedLNChannelLevel(Level):
    """raft_mlp.py:235-299"""

    def __init__(self, in_channels, out_channels, depth=4, image_size=224, patch_size=4, token_expansion_factor=2, channel_expansion_factor=4,
                 dropout=0.0, drop_path_rate=0.0):
        super().__init__(image_size, patch_size)
        self._build(self._embedding(in_channels, out_channels), [nn.Sequential(*[
            Layout("b (h w) c -> b (c w) h"),
            SpatiallySeparatedTokenBlock(self._h, out_channels, token_expansion_factor, dropout, drop_path_rate),
            Layout("b (c w) h -> b (c h) w"),
            SpatiallySeparatedTokenBlock(self._w, out_channels, token_expansion_factor, dropout, drop_path_rate),
            Layout("b (c h) w -> b (h w) c"),
            ChannelBlock(out_channels, channel_expansion_factor, dropout, drop_path_rate),
        ]) for _ in range(depth)])


class SerialPermutedLevel(Level):
    """raft_mlp.py:302-382"""

    def __init__(self, in_channels, out_channels, depth=4, image_size=224, patch_size=4, token_expansion_factor=2, channel_expansion_factor=4,
                 dropout=0.0, drop_path_rate=0.0, raft_size=4):
        super().__init__(image_size, patch_size)

        assert out_channels % raft_size == 0
        self._build(self._embedding(in_channels, out_channels), [nn.Sequential(*[
            Layout("b (h w) (chw co) -> b (co w) (chw h)"),
            PermutedBlock(self._h, out_channels, raft_size, token_expansion_factor, dropout, drop_path_rate),
            Layout("b (co w) (chw h) -> b (co h) (chw w)"),
            PermutedBlock(self._w, out_channels, raft_size, token_expansion_factor, dropout, drop_path_rate),
            Layout("b (co h) (chw w) -> b (h w) (chw co)"),
            ChannelBlock(out_channels, channel_expansion_factor, dropout, drop_path_rate),
        ]) for _ in range(depth)])


class OriginalLevel(Level):
    """raft_mlp.py:385-437 (its patch Linear is unconditional)"""

    def __init__(self, in_channels, out_channels, depth=4, image_size=224, patch_size=4, token_expansion_factor=2, channel_expansion_factor=4,
                 dropout=0.0, drop_path_rate=0.0):
        super().__init__(image_size, patch_size)
        self._build(nn.Linear((patch_size ** 2) * in_channels, out_channels), [nn.Sequential(*[
            Layout("b (h w) c -> b c (h w)"),
            TokenBlock(self._h * self._w, out_channels, token_expansion_factor, dropout, drop_path_rate),
            Layout("b c (h w) -> b (h w) c"),
            ChannelBlock(out_channels, channel_expansion_factor, dropout, drop_path_rate),
        ]) for _ in range(depth)])


class RaftMLP(E.EngineModule):
    """raft_mlp.py:442-548.  Inference-only (no `_train_forward`): in train mode the forward warns and runs as in eval mode."""

    def __init__(
        self,
        layers: List[Dict],
        in_channels: int = 3,
        image_size: int = 224,
        num_classes: int = 1000,
        token_expansion_factor: int = 2,
        channel_expansion_factor: int = 4,
        dropout: float = 0.0,
        token_mixing_type: str = SER_PM,
        shortcut: bool = True,
        gap: bool = False,
        drop_path_rate: float = 0.0,
    ):
        assert token_mixing_type in TOKEN_MIXING_TYPES
        for i, layer in enumerate(layers):
            assert DEPTH in layer
            assert DIM in layer
            assert PATCH_SIZE in layer
            assert token_mixing_type != SER_PM or RAFT_SIZE in layer
            assert 0 < layer.get(DIM)
        super().__init__()
        self.layers = layers
        self.shortcut = shortcut
        self.gap = gap
        self.__dict__["_mixing"] = token_mixing_type
        self.__dict__["_image_size"] = image_size
        self.__dict__["_in_channels"] = in_channels
        level = {ORIGINAL_TM: OriginalLevel, SEP_LN_CODIM_TM: SeparatedLNCodimLevel, SEP_LN_CH_TM: SeparatedLNChannelLevel}.get(
            token_mixing_type, SerialPermutedLevel)
        levels, heads = [], []
        last = len(self.layers) - 1
        for i, layer in enumerate(self.layers):
            params = {
                "in_channels": in_channels if i == 0 else self.layers[i - 1].get(DIM),
                "out_channels": layer.get(DIM),
                "depth": layer.get(DEPTH),
                "image_size": image_size,
                "patch_size": layer.get(PATCH_SIZE),
                "token_expansion_factor": token_expansion_factor,
                "channel_expansion_factor": channel_expansion_factor,
                "dropout": dropout,
                "drop_path_rate": drop_path_rate,
            }
            if token_mixing_type == SER_PM:
                params["raft_size"] = layer.get(RAFT_SIZE)
            levels.append(level(**params))
            if self.shortcut or i == last:
                seq = [Layout("b c h w -> b h w c"), nn.LayerNorm(layer.get(DIM)), Layout("b h w c -> b c h w")]
                if gap or i != last:
                    seq.append(Layout("b c h w -> b c (mean)"))
                if i != last:
                    seq.append(nn.Linear(layer.get(DIM), self.layers[-1].get(DIM) * 2))
                heads.append(nn.Sequential(*seq))
            image_size = math.ceil(image_size / layer.get(PATCH_SIZE))
        self.levels = nn.ModuleList(levels)
        self.heads = nn.ModuleList(heads)
        self.classifier = nn.Linear(self.layers[-1].get(DIM) if gap else self.layers[-1].get(DIM) * (image_size ** 2), num_classes)
        if not gap:
            self.flatten = nn.Flatten()

    # ------------------------------------------------------------------ packing
    def _pack(self, dtype, device):
        pk = {}
        mixing = self._mixing
        cin = self._in_channels
        for li, (layer, lvl) in enumerate(zip(self.layers, self.levels)):
            C, p, r = layer.get(DIM), layer.get(PATCH_SIZE), layer.get(RAFT_SIZE) if mixing == SER_PM else 1
            h = lvl._h
            lin = lvl.fn[1]
            if isinstance(lin, nn.Linear):
                if li == 0:
                    pk["l0.embed.w"] = E.pack_matrix(embed_columns_nchw(lin.weight, p, cin), dtype, device, kpad=E.embed_kpad(dtype))
                else:
                    pk["l%d.embed.w" % li] = E.pack_matrix(lin.weight, dtype, device)
                pk["l%d.embed.b" % li] = E.f32(lin.bias, device)
            for bi in range(layer.get(DEPTH)):
                seq, q = lvl.fn[2 + bi], "l%d.b%d." % (li, bi)
                if mixing in (SER_PM, SEP_LN_CH_TM):
                    pack_raft_half(pk, q + "v.", seq[1], r, dtype, device)
                    pack_raft_half(pk, q + "h.", seq[3], r, dtype, device)
                elif mixing == SEP_LN_CODIM_TM:
                    pack_token_block(pk, q + "v.", seq[1], (C, h), dtype, device)       # (c, w) -> (w, c)
                    pack_token_block(pk, q + "h.", seq[3], (C, h), dtype, device)       # (c, h) -> (h, c)
                else:
                    pack_token_block(pk, q + "t.", seq[1], None, dtype, device)
                cb = seq[-1]
                pack_channel_mlp(pk, q + "cm.", cb.norm, cb.fn[0], cb.fn[3], dtype, device)
            cin = C
        order = range(len(self.layers)) if self.shortcut else [len(self.layers) - 1]
        for hi, li in enumerate(order):
            hd = self.heads[hi]
            pk["h%d.g" % li], pk["h%d.b" % li] = E.f32(hd[1].weight, device), E.f32(hd[1].bias, device)
            if isinstance(hd[-1], nn.Linear):
                pk["h%d.w" % li], pk["h%d.wb" % li] = E.pack_matrix(hd[-1].weight, dtype, device), E.f32(hd[-1].bias, device)
        w = self.classifier.weight
        if not self.gap:
            C = self.layers[-1].get(DIM)
            w = classifier_columns_nhwc(w, C, w.shape[1] // C)
        pk["cls.w"], pk["cls.b"] = E.pack_matrix(w, dtype, device), E.f32(self.classifier.bias, device)
        return pk

    # ------------------------------------------------------------------ forward
    def _embed(self, ws, pk, li, lvl, src, B, S, cin, C, cd):
        """Level.forward's interpolation, the (p1 p2 c) layout and the patch Linear: src = the NCHW image (level 0) or channel-last rows of the
        S x S map; returns the rows (B h h, C) and h"""
        p, h = lvl.patch_size, lvl._h
        if lvl._bh != h:                                                # the patch does not divide the size: raft_mlp.py:158-164 (plumbing)
            nchw = src if li == 0 else src.view(B, S, S, cin).permute(0, 3, 1, 2)
            up = F.interpolate(nchw, (h * p, h * p), mode="bilinear", align_corners=False)
            S = h * p
            src = up.contiguous() if li == 0 else up.permute(0, 2, 3, 1).contiguous().view(B * S * S, cin)
        name = "l%d.embed" % li
        if not isinstance(lvl.fn[1], nn.Linear):                        # patch 1, widths differ: the reference keeps the input's channels
            if cin != C:
                raise ValueError("level %d has no patch Linear (patch_size 1) but changes the width %d -> %d: the reference fails here too" % (li, cin, C))
            rows = ws.get(name + ".x", (B * h * h, C))
            if li == 0:
                rows.view(B, h, h, C).copy_(src.permute(0, 2, 3, 1))
            else:
                rows.copy_(src)
            return rows, h
        w, b = pk[name + ".w"], pk[name + ".b"]
        out = ws.get(name + ".x", (B * h * h, C))
        if li == 0:
            embed_patches(ws, name, src, w, b, cd, (p, p), out=out)
        elif p == 1:
            E.gemm(src, w, out, B * h * h, C, cin, bias=b)
        elif w.shape[1] == p * p * cin and C % 8 == 0 and E.conv_gemm_nhwc_supported(cd, cin, p, p, p, 0):
            E.conv_gemm_nhwc(src, w, out, B, S, S, cin, p, p, p, 0, bias=b, tag="raft_embed")
        else:
            kp = w.shape[1]
            cols = ws.get(name + ".cols", (B * h * h, kp))
            E.patchify(src, cols, B, cin, S, S, p, p, 0, kp, layout=N.LAYOUT_NHWC, px_stride=cin)
            E.gemm(cols, w, out, B * h * h, C, kp, bias=b, tag="raft_embed")
        return out, h

    def forward(self, x):
        cd = self._resolve(x)
        B, cin, H_in, W_in = x.shape
        if cin != self._in_channels or H_in != self._image_size or W_in != self._image_size:
            raise ValueError("expected a (B, %d, %d, %d) tensor, got %s" % (self._in_channels, self._image_size, self._image_size, tuple(x.shape)))
        pk = self._get_pack(cd, x.device)
        ws = self._get_space(B, cd, x.device)
        mixing, last = self._mixing, len(self.layers) - 1
        dl = self.layers[-1].get(DIM)
        cur, S = x.contiguous(), self._image_size
        outs = []
        for li, (layer, lvl) in enumerate(zip(self.layers, self.levels)):
            C, r = layer.get(DIM), layer.get(RAFT_SIZE) if mixing == SER_PM else 1
            cur, S = self._embed(ws, pk, li, lvl, cur, B, S, cin, C, cd)
            rows = B * S * S
            if mixing in (SER_PM, SEP_LN_CH_TM) and not E.raft_supported(cd, S, S, C, r, 0):
                raise NotImplementedError("RaftMLP level %d: mlpk_raft_gather_ln does not take a %d x %d map of %d channels in %s" % (li, S, S, C, cd))
            for bi in range(layer.get(DEPTH)):
                q, tag = "l%d.b%d." % (li, bi), "l%d" % li
                if mixing in (SER_PM, SEP_LN_CH_TM):
                    raft_half(ws, pk, q + "v.", cur, B, S, S, C, r, 0, tag + ".v")
                    raft_half(ws, pk, q + "h.", cur, B, S, S, C, r, 1, tag + ".h")
                elif mixing == SEP_LN_CODIM_TM:
                    token_mix_rows(ws, pk, q + "v.", cur.view(B, S, S * C), tag + ".v")
                    xt = ws.get(tag + ".xt", (B, S, S * C))                        # the map transposed: (b, w, h, c)
                    xt.view(B, S, S, C).copy_(cur.view(B, S, S, C).transpose(1, 2))
                    token_mix_rows(ws, pk, q + "h.", xt, tag + ".h")
                    cur.view(B, S, S, C).copy_(xt.view(B, S, S, C).transpose(1, 2))
                else:
                    token_mix_rows(ws, pk, q + "t.", cur.view(B, S * S, C), tag + ".t")
                channel_mlp(ws, cur, rows, C, pk, q + "cm.", pk[q + "cm.fc1.w"].shape[0], tag=tag + ".cm")
            if self.shortcut or li == last:
                mean, rstd = layernorm_stats(ws, cur, rows, C, tag="h%d.ln" % li)
                g, b = pk["h%d.g" % li], pk["h%d.b" % li]
                if self.gap or li != last:
                    o = ws.get("h%d.pool" % li, (B, C))
                    E.pool_mean(cur, B, S * S, C, C, o, C, mean=mean, rstd=rstd, gamma=g, beta=b)
                    if li != last:
                        film = ws.get("h%d.film" % li, (B, 2 * dl))
                        E.gemm(o, pk["h%d.w" % li], film, B, 2 * dl, C, bias=pk["h%d.wb" % li])
                        o = film
                else:
                    o = ws.get("h%d.map" % li, (rows, C))
                    E.norm_apply(cur, rows, C, C, mean=mean, rstd=rstd, gamma=g, beta=b, out_rm=o, ld_rm=C)
                    o = o.view(B, S * S, C)
                outs.append(o)
            cin = C
        # the FiLM-style reduce over levels, last level first: a <- scale * a + shift (fp32, elementwise)
        a = outs[-1].float()
        for o in reversed(outs[:-1]):
            scale, shift = o[:, :dl].float(), o[:, dl:].float()
            a = scale * a + shift if self.gap else scale[:, None, :] * a + shift[:, None, :]
        K = self.classifier.in_features
        feat = ws.get("cls.x", (B, pk["cls.w"].shape[1]))
        feat[:, :K].copy_(a.reshape(B, K))
        return head_linear(ws, feat, B, feat.shape[1], pk["cls.w"], pk["cls.b"], self.classifier.out_features, x.dtype)
