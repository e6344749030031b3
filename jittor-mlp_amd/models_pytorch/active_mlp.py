"""ActiveMLP (Microsoft's ATM), drop-in for the reference's models_pytorch/active_mlp.py: same classes, constructor signatures, defaults, state_dict
keys and shapes, and the ActivexTiny / ActiveTiny / ActiveSmall / ActiveBase / ActiveLarge factories, under the reference's import path:
`from models_pytorch.active_mlp import ActiveMLP, ATMLayer, ActiveTiny, ...`.  Inference-only: train() takes the engine's
warning path (DropPath and Dropout run as the identity).  Two things the reference's constructor does are NOT done here: it prints its arguments
through `utils.dict_to_string` (an import that does not resolve inside the reference package), and its factories set `default_cfg` from timm.
`img_size`, `patch_size` and `in_chans` are accepted and ignored, as in the reference (:279 hard-codes the 7 x 7 / stride 4 / pad 2 stem of three
input channels); no parameter depends on the input size, so any H x W runs.

ATMOp (:65-81) hands torchvision's deform_conv2d a 1 x 1 kernel and a LEARNED real-valued offset per pixel and channel, along w (dx slots) or
along h (dy slots), the other slot zero: bilinear sampling with one offset identically zero is linear interpolation between two neighbours on a
row or a column of the map, zero outside it.  mlpk_atm_sample writes both sampled copies of LayerNorm(x) and LayerNorm(x) itself in one pass;
the 1 x 1 convolutions are NT GEMMs.  The block is CycleMLP's (cycle_mlp.py `CycleNet._block`) with that kernel in place of the fixed shift.

forward_blocks (:330-343), on channel-last rows (B*H*W, C); per stage i, block j:
  j % intv == 0 and j != depth_i - 1     x = PEG_i(x)                       mlpk_dwconv_plain_nhwc, the residual folded into the centre tap
                                         mean, rstd = row statistics of x   ONE pass: offset_layer[0] and norm1 normalise the same x
                                         off = Linear(LN(x))                the LN-folded GEMM (16-bit), else mlpk_norm_apply + GEMM; kept as
                                                                            rows (B*H*W, 2C / share_dim), NOT repeated, until the next one
  ATMLayer (:108-127)  w, h, c = three GEMMs on sample_w(xn), sample_h(xn), xn   mlpk_atm_sample; the two biased products as one pair launch
                       a = mean over pixels of (w + h + c)                  mlpk_split_sum with scale 1 / (H W)
                       fusion = Mlp(C -> C/4 -> 3C), fp32, B rows; its output index is c*3 + k (reshape(B, C, 3), :120): fc2's rows are
                                permuted to k*C + c at pack time (`fusion_rows`)
                       x += proj(w a0 + h a1 + c a2)                        mlpk_split_softmax, mlpk_split_apply, GEMM with the residual
  channel MLP          common.channel_mlp, LayerNorm folded into fc1
  Downsample           3 x 3 stride 2 pad 1 after the stage's last block: mlpk_conv_gemm_nhwc, or the window gather + GEMM where it refuses
A stage of depth 1 never generates an offset (its only block is also its last); the reference then reuses the previous stage's offset at the
wrong size or fails on an unbound name.  forward() raises ValueError for such a stage.

`ATMLayer` runs on its own on the reference's layouts -- x (B, H, W, C) already normalised, offset (B, 2C, H, W) already repeated, hence
share = 1.  The other inner classes hold parameters.
"""
import math

import torch
from torch import nn
from torch.nn import init

from .. import _native as N
from .. import engine as E
from .common import SubModule, channel_mlp, finalize_stats, head_linear, layernorm_stats, pack_channel_mlp


def _pair(v):
    return tuple(v) if isinstance(v, (tuple, list)) else (v, v)


class _Container(nn.Module):
    """Holds parameters; the enclosing ActiveMLP packs them into its own kernel sequence and never calls the module."""

    def forward(self, *a, **k):
        raise NotImplementedError("%s only holds parameters inside ActiveMLP: call the enclosing ActiveMLP (or an ATMLayer)" % type(self).__name__)


class Mlp(_Container):
    """active_mlp.py:18-34"""

    def __init__(self, in_features, hidden_features=None, out_features=None, act_layer=nn.GELU, drop=0.):
        super().__init__()
        out_features = out_features or in_features
        hidden_features = hidden_features or in_features
        self.fc1 = nn.Linear(in_features, hidden_features)
        self.act = act_layer()
        self.fc2 = nn.Linear(hidden_features, out_features)
        self.drop = nn.Dropout(drop)


class ATMOp(_Container):
    """active_mlp.py:37-91: the 1 x 1 weight (out, in, 1, 1) and bias of one deformable branch; `dimension` is 'w' or 'h'."""

    def __init__(self, in_chans, out_chans, stride: int = 1, padding: int = 0, dilation: int = 1, bias: bool = True, dimension: str = ''):
        super().__init__()
        self.in_chans = in_chans
        self.out_chans = out_chans
        self.stride = _pair(stride)
        self.padding = _pair(padding)
        self.dilation = _pair(dilation)
        self.dimension = dimension
        self.weight = nn.Parameter(torch.empty(out_chans, in_chans, 1, 1))
        if bias:
            self.bias = nn.Parameter(torch.empty(out_chans))
        else:
            self.register_parameter('bias', None)
        self.reset_parameters()

    def reset_parameters(self):
        init.kaiming_uniform_(self.weight, a=math.sqrt(5))
        if self.bias is not None:
            bound = 1 / math.sqrt(self.weight.shape[1])
            init.uniform_(self.bias, -bound, bound)

    def extra_repr(self):
        return "dimension=%s, in_chans=%d, out_chans=%d, stride=%s%s" % (self.dimension, self.in_chans, self.out_chans, self.stride,
                                                                         ", bias=False" if self.bias is None else "")


# ------------------------------------------------------------------ packing (pure functions: they run on CPU tensors too)
def fusion_rows(w2, b2, C):
    """ATMLayer.fusion.fc2: output index c * 3 + k (reshape(B, C, 3), :120) -> k * C + c, the [B][3][C] layout of mlpk_split_softmax"""
    w2, b2 = w2.detach(), b2.detach()
    return w2.reshape(C, 3, -1).permute(1, 0, 2).reshape(3 * C, -1).contiguous(), b2.reshape(C, 3).t().reshape(-1).contiguous()


def peg_taps(weight):
    """PEG's depthwise Conv2d weight (C, 1, 3, 3) -> fp32 [9][C] tap-major (mlpk_dwconv_plain_nhwc's order) with the residual `+ x` (:220) folded
    into the centre tap"""
    w = weight.detach().float().reshape(weight.shape[0], 9).t().contiguous()
    w[4] += 1.0
    return w


def pack_atm(pk, p, atm, dtype, device, lam=1.0):
    """an ATMLayer under prefix p"""
    C = atm.dim
    pk[p + "w.w"], pk[p + "w.b"] = E.pack_matrix(atm.atm_w.weight, dtype, device), E.f32(atm.atm_w.bias, device)
    pk[p + "h.w"], pk[p + "h.b"] = E.pack_matrix(atm.atm_h.weight, dtype, device), E.f32(atm.atm_h.bias, device)
    pk[p + "c.w"] = E.pack_matrix(atm.atm_c.weight, dtype, device)
    pk[p + "f1.w"], pk[p + "f1.b"] = E.pack_matrix(atm.fusion.fc1.weight, torch.float32, device), E.f32(atm.fusion.fc1.bias, device)
    w2, b2 = fusion_rows(atm.fusion.fc2.weight, atm.fusion.fc2.bias, C)
    pk[p + "f2.w"], pk[p + "f2.b"] = E.pack_matrix(w2, torch.float32, device), E.f32(b2, device)
    pk[p + "p.w"], pk[p + "p.b"] = E.pack_matrix(atm.proj.weight, dtype, device), E.f32(atm.proj.bias, device)


def atm_mix(ws, pk, p, src, stats, gamma, beta, off, share, B, H, W, C, tag, out, residual):
    """ATMLayer on rows: out = [out +] proj(w a0 + h a1 + c a2) with w, h, c the three products on the sampled / plain LayerNorm of `src`
    (stats / gamma / beta None: `src` is already normalised).  Returns what the proj GEMM's `part` delivered (residual only)."""
    rows = B * H * W
    mean, rstd = stats if stats is not None else (None, None)
    sw, sh, sc = ws.get(tag + ".sw", (rows, C)), ws.get(tag + ".sh", (rows, C)), ws.get(tag + ".sc", (rows, C))
    E.atm_sample(src, mean, rstd, gamma, beta, off, share, sw, sh, sc, B, H, W, C)
    tw, th, tc = ws.get(tag + ".tw", (rows, C)), ws.get(tag + ".th", (rows, C)), ws.get(tag + ".tc", (rows, C))
    E.gemm_pair(((sw, pk[p + "w.w"], tw, rows, C, C), dict(bias=pk[p + "w.b"], tag="atm_fc")),
                ((sh, pk[p + "h.w"], th, rows, C, C), dict(bias=pk[p + "h.b"], tag="atm_fc")))
    E.gemm(sc, pk[p + "c.w"], tc, rows, C, C, tag="atm_c")
    # fusion: mean over pixels -> Mlp -> softmax over the three branches (fp32, B rows)
    a = ws.get(tag + ".a", (B, C), torch.float32)
    E.split_sum(tw, th, tc, C, C, C, B, H, W, C, N.SHIFT_NONE, a, scale=1.0 / (H * W))
    hid = pk[p + "f1.w"].shape[0]
    hp = pk[p + "f2.w"].shape[1]                                       # hidden padded to whole 16-byte chunks (zero columns)
    t = ws.get(tag + ".t", (B, hp), torch.float32)
    E.gemm(a, pk[p + "f1.w"], t, B, hid, C, ldc=hp, bias=pk[p + "f1.b"], act=N.ACT_GELU)
    hat = ws.get(tag + ".hat", (B, 3 * C), torch.float32)
    E.gemm(t, pk[p + "f2.w"], hat, B, 3 * C, hp, bias=pk[p + "f2.b"])
    bar = ws.get(tag + ".bar", (B, 3 * C), torch.float32)
    E.split_softmax(hat, bar, B, C)
    m = ws.get(tag + ".m", (rows, C))
    E.split_apply(tw, th, tc, C, C, C, B, H, W, C, N.SHIFT_NONE, bar, m, C)
    if residual:
        return E.gemm(m, pk[p + "p.w"], out, rows, C, C, bias=pk[p + "p.b"], R=out, res=N.RES_ADD, tag="atm_proj", part=(ws, tag + ".p.part"))
    E.gemm(m, pk[p + "p.w"], out, rows, C, C, bias=pk[p + "p.b"], tag="atm_proj")
    return None


class ATMLayer(SubModule):
    """active_mlp.py:94-133.  Callable on its own like the reference's: x (B, H, W, C) (the block's norm1 output), offset (B, 2C, H, W) with one
    offset per channel (what ActiveBlock passes after repeat_interleave) -> (B, H, W, C)."""

    def __init__(self, dim, proj_drop=0.):
        super().__init__()
        self.dim = dim
        self.atm_c = nn.Linear(dim, dim, bias=False)
        self.atm_h = ATMOp(dim, dim, dimension='h')
        self.atm_w = ATMOp(dim, dim, dimension='w')
        self.fusion = Mlp(dim, dim // 4, dim * 3)
        self.proj = nn.Linear(dim, dim)
        self.proj_drop = nn.Dropout(proj_drop)

    def _pack(self, dtype, device):
        pk = {}
        pack_atm(pk, "", self, dtype, device)
        return pk

    def forward(self, x, offset):
        C = self.dim
        pk = self._begin(x, C)
        if x.dim() != 4:
            raise ValueError("expected a channel-last (B, H, W, %d) tensor" % C)
        B, H, W, _ = x.shape
        assert offset.shape == (B, 2 * C, H, W), f"offset shape not match, got {offset.shape}"
        if not E.atm_sample_supported(x.dtype, H, W, C, 1):
            raise NotImplementedError("ATMLayer: mlpk_atm_sample does not take a %d x %d map of %d channels in %s" % (H, W, C, x.dtype))
        rows = B * H * W
        with E.on_device(x):
            ws = self._get_space((B, H, W), x.dtype, x.device)
            xb = ws.get("atm.x", (rows, C))
            xb.copy_(x.reshape(rows, C))
            off = ws.get("atm.off", (rows, 2 * C))
            off.view(B, H, W, 2 * C).copy_(offset.permute(0, 2, 3, 1))
            out = ws.get("atm.out", (rows, C))
            atm_mix(ws, pk, "", xb, None, None, None, off, 1, B, H, W, C, "atm", out, residual=False)
            return out.reshape(B, H, W, C).clone()

    def extra_repr(self):
        return "dim: %d" % self.dim


class ActiveBlock(_Container):
    """active_mlp.py:136-184 (DropPath is the identity on the forward path built here)."""

    def __init__(self, dim, mlp_ratio=4., drop_path=0., act_layer=nn.GELU, norm_layer=nn.LayerNorm, share_dim=1, downsample=None, new_offset=False):
        super().__init__()
        self.norm1 = norm_layer(dim)
        self.atm = ATMLayer(dim)
        self.norm2 = norm_layer(dim)
        self.mlp = Mlp(in_features=dim, hidden_features=int(dim * mlp_ratio), act_layer=act_layer)
        self.drop_path = nn.Identity()
        self.drop_path_rate = drop_path
        self.downsample = downsample
        self.new_offset = new_offset
        self.share_dim = share_dim
        if new_offset:
            self.offset_layer = nn.Sequential(norm_layer(dim), nn.Linear(dim, dim * 2 // self.share_dim))
        else:
            self.offset_layer = None

    def extra_repr(self):
        return "new_offset: %s, share_dim: %d" % (self.new_offset, self.share_dim)


class Downsample(_Container):
    """active_mlp.py:187-199"""

    def __init__(self, in_chans, out_chans):
        super().__init__()
        self.proj = nn.Conv2d(in_chans, out_chans, kernel_size=(3, 3), stride=(2, 2), padding=1)


class PEG(_Container):
    """active_mlp.py:202-224: depthwise 3 x 3 with bias, plus x at stride 1"""

    def __init__(self, in_chans, embed_dim=768, stride=1):
        super().__init__()
        self.proj = nn.Conv2d(in_chans, embed_dim, kernel_size=3, stride=stride, padding=1, bias=True, groups=embed_dim)
        self.stride = stride


class OverlapPatchEmbed(_Container):
    """active_mlp.py:227-245"""

    def __init__(self, patch_size=7, stride=4, padding=2, in_chans=3, embed_dim=64):
        super().__init__()
        patch_size, stride, padding = _pair(patch_size), _pair(stride), _pair(padding)
        self.patch_size = patch_size
        self.proj = nn.Conv2d(in_chans, embed_dim, kernel_size=patch_size, stride=stride, padding=padding)


class ActiveMLP(E.EngineModule):
    """active_mlp.py:248-356.  Inference-only (no `_train_forward`): in train mode the forward warns and runs as in eval mode."""

    def __init__(
            self,
            img_size=224,
            patch_size=4,
            in_chans=3,
            num_classes=1000,
            depths=[2, 2, 4, 2],
            embed_dims=[64, 128, 320, 512],
            mlp_ratios=[4, 4, 4, 4],
            share_dims=[1, 1, 1, 1],  # how many channels share one offset
            drop_path_rate=0.,
            act_layer=nn.GELU,
            norm_layer=nn.LayerNorm,
            intv=2,  # interval for generating new offset
            **kwargs
    ):
        super().__init__()
        self.depths = depths
        self.num_classes = num_classes
        self.intv = intv
        self.patch_embed = OverlapPatchEmbed(patch_size=7, stride=4, padding=2, in_chans=3, embed_dim=embed_dims[0])
        dpr = [x.item() for x in torch.linspace(0, drop_path_rate, sum(depths))]
        ii = 0
        self.blocks = nn.ModuleList()
        for i in range(len(depths)):
            _block = nn.ModuleList([
                ActiveBlock(embed_dims[i],
                            mlp_ratio=mlp_ratios[i],
                            drop_path=dpr[ii + j],
                            share_dim=share_dims[i],
                            act_layer=act_layer,
                            norm_layer=norm_layer,
                            downsample=Downsample(embed_dims[i], embed_dims[i + 1]) if i < len(depths) - 1 and j == depths[i] - 1 else None,
                            new_offset=(j % self.intv == 0 and j != depths[i] - 1),
                            ) for j in range(depths[i])
            ])
            self.blocks.append(_block)
            ii += depths[i]
        # PEG for each resolution feature map
        self.pos_blocks = nn.ModuleList([PEG(ed, ed) for ed in embed_dims])
        self.norm = norm_layer(embed_dims[-1])
        self.head = nn.Linear(embed_dims[-1], num_classes) if num_classes > 0 else nn.Identity()
        self.apply(self._init_weights)

    def _init_weights(self, m):
        """active_mlp.py:308-324"""
        if isinstance(m, nn.Linear):
            init.trunc_normal_(m.weight, std=.02)
            if m.bias is not None:
                nn.init.constant_(m.bias, 0)
        elif isinstance(m, nn.LayerNorm):
            nn.init.constant_(m.bias, 0)
            nn.init.constant_(m.weight, 1.0)
        elif isinstance(m, ATMOp):
            init.trunc_normal_(m.weight, std=.02)
            nn.init.constant_(m.bias, 0)
        elif isinstance(m, nn.Conv2d):
            fan_out = m.kernel_size[0] * m.kernel_size[1] * m.out_channels
            fan_out //= m.groups
            m.weight.data.normal_(0, math.sqrt(2.0 / fan_out))
            if m.bias is not None:
                m.bias.data.zero_()

    @torch.jit.ignore
    def no_weight_decay(self):
        return set(['pos_blocks.' + n for n, p in self.pos_blocks.named_parameters()])

    # ------------------------------------------------------------------ packing
    def _pack(self, dtype, device):
        pk = {}
        conv = self.patch_embed.proj
        pk["embed.w"] = E.pack_matrix(conv.weight, dtype, device)
        if dtype != torch.float32:
            pk["embed.w7"] = E.pack_stem7(conv.weight, dtype, device)
        pk["embed.b"] = E.f32(conv.bias, device)
        for si, stage in enumerate(self.blocks):
            peg = self.pos_blocks[si].proj
            pk["s%d.peg.w" % si], pk["s%d.peg.b" % si] = peg_taps(peg.weight).to(device), E.f32(peg.bias, device)
            for bi, blk in enumerate(stage):
                p = "s%d.b%d." % (si, bi)
                C = blk.atm.dim
                pk[p + "ln.g"], pk[p + "ln.b"] = E.f32(blk.norm1.weight, device), E.f32(blk.norm1.bias, device)
                pack_atm(pk, p, blk.atm, dtype, device)
                pack_channel_mlp(pk, p + "ff.", blk.norm2, blk.mlp.fc1, blk.mlp.fc2, dtype, device)
                if blk.offset_layer is not None:
                    ln, lin = blk.offset_layer[0], blk.offset_layer[1]
                    pk[p + "o.g"], pk[p + "o.be"] = E.f32(ln.weight, device), E.f32(ln.bias, device)
                    pk[p + "o.w"], pk[p + "o.b"] = E.pack_matrix(lin.weight, dtype, device), E.f32(lin.bias, device)
                    if dtype != torch.float32 and C % 8 == 0:
                        pk[p + "of.w"], pk[p + "of.b"], pk[p + "of.csum"] = E.pack_ln_folded(lin.weight, lin.bias, ln.weight, ln.bias, dtype, device)
                if blk.downsample is not None:
                    w = blk.downsample.proj.weight
                    pk[p + "d.w"] = E.pack_matrix(w.detach().permute(0, 2, 3, 1).reshape(w.shape[0], -1), dtype, device)        # (i, j, ci)
                    pk[p + "d.b"] = E.f32(blk.downsample.proj.bias, device)
        pk["head.g"], pk["head.be"] = E.f32(self.norm.weight, device), E.f32(self.norm.bias, device)
        if isinstance(self.head, nn.Linear):
            pk["head.w"] = E.pack_matrix(self.head.weight, dtype, device)
            pk["head.b"] = E.f32(self.head.bias, device)
        return pk

    # ------------------------------------------------------------------ forward
    def _offsetless_stage(self):
        """index of a stage whose first block generates no offset (depth 1: `j != depth - 1` fails for j = 0), or None"""
        for i, d in enumerate(self.depths):
            if d == 1:
                return i
        return None

    def _new_offset(self, ws, pk, p, cur, st, rows, C, share, tag):
        """offset_layer of a block: Linear(LayerNorm(x)) on the un-normalised x, as rows (rows, 2C / share) at a pitch of whole 16-byte vectors"""
        n_off = 2 * C // share
        off = ws.get(tag + ".off", (rows, E.round_up(n_off, 8)))
        if (p + "of.w") in pk:
            E.gemm(cur, pk[p + "of.w"], off, rows, n_off, C, bias=pk[p + "of.b"], ln=(st[0], st[1], pk[p + "of.csum"]), tag="atm_off")
        else:
            xn = ws.get(tag + ".oxn", (rows, C))
            E.norm_apply(cur, rows, C, C, mean=st[0], rstd=st[1], gamma=pk[p + "o.g"], beta=pk[p + "o.be"], out_rm=xn, ld_rm=C)
            E.gemm(xn, pk[p + "o.w"], off, rows, n_off, C, bias=pk[p + "o.b"], tag="atm_off")
        return off

    def forward(self, x):
        bad = self._offsetless_stage()
        if bad is not None:
            raise ValueError("stage %d has depth 1: its only block is also its last, so it never generates an offset (a new offset needs "
                             "j %% intv == 0 and j != depth - 1) and the stage has none to sample with; give every stage at least two blocks" % bad)
        cd = self._resolve(x)
        B, cin, H_in, W_in = x.shape
        if cin != 3:
            raise ValueError("expected a (B, 3, H, W) tensor: the stem is Conv2d(3, C, 7, 4, 2) whatever in_chans says, as in the reference")
        pk = self._get_pack(cd, x.device)
        ws = self._get_space(B, cd, x.device)
        x = x.contiguous()
        C = pk["embed.w"].shape[0]
        H, W = (H_in + 4 - 7) // 4 + 1, (W_in + 4 - 7) // 4 + 1
        if H <= 0 or W <= 0:
            raise ValueError("the input is smaller than the 7 x 7 stem")
        kp = pk["embed.w"].shape[1]
        cur = ws.get("s0.x", (B * H * W, C))
        if "embed.w7" in pk and x.data_ptr() % 16 == 0 and E.stem7_supported(x.dtype, cur.dtype, cin, H_in, W_in, 2, C):
            E.stem7(x, pk["embed.w7"], pk["embed.b"], cur, B, H_in, W_in, 2, C)
        else:
            patches = ws.get("embed.patches", (B * H * W, kp))
            E.im2col(x, patches, B, cin, H_in, W_in, 7, 7, 4, 4, 2, kp)
            E.gemm(patches, pk["embed.w"], cur, B * H * W, C, kp, bias=pk["embed.b"])
        last_stage = len(self.blocks) - 1
        for si, stage in enumerate(self.blocks):
            rows = B * H * W
            tag = "s%d" % si
            share = stage[0].share_dim
            if not E.atm_sample_supported(cd, H, W, C, share):
                raise NotImplementedError("ActiveMLP stage %d: mlpk_atm_sample does not take a %d x %d map of %d channels (share %d) in %s" % (
                    si, H, W, C, share, cd))
            alt = ws.get(tag + ".y", (rows, C))
            off, st = None, None
            for bi, blk in enumerate(stage):
                p = "s%d.b%d." % (si, bi)
                if blk.offset_layer is not None:
                    # the stage's PEG, then a new offset from the un-normalised result; its LayerNorm and the block's norm1 share the statistics
                    E.dwconv_plain_nhwc(cur, alt, B, H, W, C, 3, pk[tag + ".peg.w"], pk[tag + ".peg.b"])
                    cur, alt = alt, cur
                    st = layernorm_stats(ws, cur, rows, C, tag=tag + ".ln")
                    off = self._new_offset(ws, pk, p, cur, st, rows, C, share, tag)
                elif st is None:
                    st = layernorm_stats(ws, cur, rows, C, tag=tag + ".ln")
                got = atm_mix(ws, pk, p, cur, st, pk[p + "ln.g"], pk[p + "ln.b"], off, share, B, H, W, C, tag, cur, residual=True)
                got = channel_mlp(ws, cur, rows, C, pk, p + "ff.", blk.mlp.fc1.weight.shape[0], tag=tag + ".cm",
                                  stats=finalize_stats(ws, got, rows, C, tag=tag + ".cm.ln"), part=(ws, tag + ".fc2.part"))
                st = finalize_stats(ws, got, rows, C, tag=tag + ".ln")
                if blk.downsample is not None:
                    Cout = pk[p + "d.w"].shape[0]
                    H2, W2 = (H + 2 - 3) // 2 + 1, (W + 2 - 3) // 2 + 1
                    kd = pk[p + "d.w"].shape[1]
                    nxt = ws.get("s%d.x" % (si + 1), (B * H2 * W2, Cout))
                    if kd == 9 * C and E.conv_gemm_nhwc_supported(cur.dtype, C, 3, 3, 2, 1):
                        E.conv_gemm_nhwc(cur, pk[p + "d.w"], nxt, B, H, W, C, 3, 3, 2, 1, bias=pk[p + "d.b"], tag="atm_down")
                    else:
                        cols = ws.get(tag + ".cols", (B * H2 * W2, kd))
                        E.im2col(cur, cols, B, C, H, W, 3, 3, 2, 2, 1, kd, layout=N.LAYOUT_NHWC, px_stride=C)
                        E.gemm(cols, pk[p + "d.w"], nxt, B * H2 * W2, Cout, kd, bias=pk[p + "d.b"], tag="atm_down")
                    cur, H, W, C, st = nxt, H2, W2, Cout, None
        rows = B * H * W
        mean, rstd = st if st is not None else layernorm_stats(ws, cur, rows, C, tag="head.ln")
        pooled = ws.get("pooled", (B, C))
        E.pool_mean(cur, B, H * W, C, C, pooled, C, mean=mean, rstd=rstd, gamma=pk["head.g"], beta=pk["head.be"])
        if not isinstance(self.head, nn.Linear):
            out = torch.empty((B, C), dtype=x.dtype, device=x.device)
            E.convert(pooled, out, B * C)
            return out
        return head_linear(ws, pooled, B, C, pk["head.w"], pk["head.b"], self.num_classes, x.dtype)


def _factory(depths, mlp_ratios, embed_dims, intv):
    def make(pretrained=False, **kwargs):
        return ActiveMLP(depths=depths, embed_dims=embed_dims, mlp_ratios=mlp_ratios, share_dims=[2, 4, 4, 8], intv=intv, **kwargs)
    return make


# active_mlp.py:359-411
ActivexTiny = _factory([2, 2, 4, 2], [4, 4, 4, 4], [64, 128, 320, 512], 2)
ActiveTiny = _factory([2, 3, 10, 3], [4, 4, 4, 4], [64, 128, 320, 512], 2)
ActiveSmall = _factory([3, 4, 18, 3], [8, 8, 4, 4], [64, 128, 320, 512], 6)
ActiveBase = _factory([3, 8, 27, 3], [8, 8, 4, 4], [64, 128, 320, 512], 6)
ActiveLarge = _factory([3, 4, 24, 3], [4, 4, 4, 4], [96, 192, 384, 768], 6)
