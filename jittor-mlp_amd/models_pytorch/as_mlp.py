"""AS-MLP, drop-in for the reference's models_pytorch/as_mlp.py (eval-mode forward).

The reference keeps NCHW and runs every "linear" as a 1x1 Conv2d; only the input image layout and
the logits are contractual, so activations live channel-last here and every 1x1 conv is the same
K-contiguous NT GEMM as the rest of the package.  Per block (as_mlp.py:149-162, 55-95):
  x <- x + conv3(GN(gelu(conv2_1(shift_W(t))) + gelu(conv2_2(shift_H(t))))),  t = gelu(GN(conv1(GN(x))))
  x <- x + fc2(gelu(fc1(GN(x))))
GroupNorm(1, C) (as_mlp.py:343-344) = one (mean, rstd) per SAMPLE over (C,H,W): mlpk_row_stats on the
sample viewed as one long row, applied (with GELU where the reference has it) by mlpk_norm_apply.
The axial shift (utils/shift_cuda.py:44-72) runs as mlpk_shift_nhwc; conv2_2's epilogue does
GELU and adds conv2_1's GELU output, conv3's and fc2's epilogues add the residual.
DropPath is the identity in eval mode (as_mlp.py:144,159-160); `use_checkpoint` is accepted and ignored.
"""

import torch
from torch import nn

from .. import _native as N
from .. import engine as E
from .common import Block, Holder, StochasticDepth, SubModule, TrainDropout, finalize_stats, head_linear, train_entry, two_layer_mlp
from .utils.shift import Shift

# The GroupNorm(1,C) statistics of what the GEMMs write come from a statistics pass: taking them from the GEMMs' epilogues (mlpk.h row_part)
# measured slower on AS-MLP-T -- the C = 96 / 192 GEMMs are short-K and epilogue-bound, and the pass over a whole sample runs at HBM speed
# (on the C >= 384 stages too: 6.52 vs 6.43 ms, profiles/r05_as_conv2_384_ab.txt).


def to_2tuple(v):
    return tuple(v) if isinstance(v, (tuple, list)) else (v, v)


class Mlp(SubModule):
    """as_mlp.py:8-24: Conv2d(1x1) -> GELU -> Dropout -> Conv2d(1x1) -> Dropout on (B, C, H, W); callable on its own like the
    reference's (channel-last inside: the 1 x 1 convolutions are the NT GEMM)."""

    def __init__(self, in_features, hidden_features=None, out_features=None, act_layer=nn.GELU, drop=0.):
        super().__init__()
        out_features = out_features or in_features
        hidden_features = hidden_features or in_features
        self.fc1 = nn.Conv2d(in_features, hidden_features, 1, 1)
        self.act = act_layer()
        self.fc2 = nn.Conv2d(hidden_features, out_features, 1, 1)
        self.drop = nn.Dropout(drop)

    def _pack(self, dtype, device):
        return {"fc1.w": E.pack_matrix(self.fc1.weight, dtype, device), "fc1.b": E.f32(self.fc1.bias, device),
                "fc2.w": E.pack_matrix(self.fc2.weight, dtype, device), "fc2.b": E.f32(self.fc2.bias, device)}

    def forward(self, x):
        if not isinstance(self.act, nn.GELU):
            raise NotImplementedError("Mlp runs on its own with the reference's default activation (GELU) only")
        cin, hidden, cout = self.fc1.in_channels, self.fc1.out_channels, self.fc2.out_channels
        if x.dim() != 4:
            raise ValueError("expected a (B, C, H, W) tensor")
        pk = self._begin(x, cin, axis=1)
        B, _, H, W = x.shape
        rows = B * H * W
        with E.on_device(x):
            ws = self._get_space(rows, x.dtype, x.device)
            xb = ws.get("mlp.x", (rows, pk["fc1.w"].shape[1]))
            xb[:, :cin].copy_(x.permute(0, 2, 3, 1).reshape(rows, cin))
            y = two_layer_mlp(ws, pk, xb, rows, cin, hidden, cout)
            return y.reshape(B, H, W, cout).permute(0, 3, 1, 2).contiguous()


class AxialShift(Holder):
    """as_mlp.py:27-53."""

    def __init__(self, dim, shift_size, as_bias=True, proj_drop=0.):
        super().__init__()
        self.dim = dim
        self.shift_size = shift_size
        self.pad = shift_size // 2
        self.conv1 = nn.Conv2d(dim, dim, 1, 1, 0, groups=1, bias=as_bias)
        self.conv2_1 = nn.Conv2d(dim, dim, 1, 1, 0, groups=1, bias=as_bias)
        self.conv2_2 = nn.Conv2d(dim, dim, 1, 1, 0, groups=1, bias=as_bias)
        self.conv3 = nn.Conv2d(dim, dim, 1, 1, 0, groups=1, bias=as_bias)
        self.actn = nn.GELU()
        self.norm1 = MyNorm(dim)
        self.norm2 = MyNorm(dim)
        self.shift_dim2 = Shift(self.shift_size, 2)
        self.shift_dim3 = Shift(self.shift_size, 3)

    def extra_repr(self):
        return f'dim={self.dim}, shift_size={self.shift_size}'

    def forward(self, x):
        """as_mlp.py:55-95 on (B, C, H, W) like the reference's: conv1 -> GroupNorm -> GELU -> the two axial shifts -> conv2_1 /
        conv2_2 (+ GELU) -> sum -> GroupNorm -> conv3.  Channel-last inside (the 1x1 convolutions are the NT GEMM, the shifts
        mlpk_shift_nhwc); the two layout changes of a lone call are torch permutes -- inside AS_MLP the whole network stays
        channel-last and the block additionally folds the norms into the GEMMs."""
        E.require_gpu(x, "AxialShift.forward")
        if x.dim() != 4 or x.shape[1] != self.dim:
            raise ValueError("expected (B, %d, H, W)" % self.dim)
        from .common import standalone_space
        B, C, H, W = x.shape
        rows, HW = B * H * W, H * W
        ws = standalone_space(x)
        dev, dt = x.device, x.dtype

        def conv(c, src, dst, **kw):
            E.gemm(src, E.pack_matrix(c.weight, dt, dev), dst, rows, C, C, bias=E.f32(c.bias, dev) if c.bias is not None else None, **kw)

        def gn(t, norm, act=N.ACT_NONE):
            g, b = _gn_params(norm, dev)
            mean, rstd = ws.get("gn.mean", (B,), torch.float32), ws.get("gn.rstd", (B,), torch.float32)
            E.row_stats(t, B, HW * C, HW * C, mean, rstd)
            E.norm_apply(t, rows, C, C, mean=mean, rstd=rstd, gamma=g, beta=b, act=act, stat_group=HW, out_rm=t, ld_rm=C)
        with E.on_device(x):
            cur = x.permute(0, 2, 3, 1).contiguous().view(rows, C)
            t0, t1, t2 = ws.get("t0", (rows, C)), ws.get("t1", (rows, C)), ws.get("t2", (rows, C))
            conv(self.conv1, cur, t1)
            gn(t1, self.norm1, act=N.ACT_GELU)
            E.shift_nhwc(t1, t0, B, H, W, C, self.shift_size, 3)
            conv(self.conv2_1, t0, t2, act=N.ACT_GELU)
            E.shift_nhwc(t1, t0, B, H, W, C, self.shift_size, 2)
            conv(self.conv2_2, t0, t2, act=N.ACT_GELU, R=t2, res=N.RES_ADD)
            gn(t2, self.norm2)
            out = torch.empty((rows, C), dtype=dt, device=dev)
            conv(self.conv3, t2, out)
        return out.view(B, H, W, C).permute(0, 3, 1, 2).contiguous()


class AxialShiftedBlock(Block):
    """as_mlp.py:118-147."""

    def __init__(self, dim, input_resolution, shift_size=7, mlp_ratio=4., as_bias=True, drop=0., drop_path=0.,
                 act_layer=nn.GELU, norm_layer=nn.LayerNorm):
        super().__init__()
        self.dim = dim
        self.input_resolution = input_resolution
        self.shift_size = shift_size
        self.mlp_ratio = mlp_ratio
        self.norm1 = norm_layer(dim)
        self.axial_shift = AxialShift(dim, shift_size=shift_size, as_bias=as_bias, proj_drop=drop)
        self.drop_path = nn.Identity()                 # DropPath(p) is the identity in eval mode
        self.drop_path_rate = drop_path
        self.norm2 = norm_layer(dim)
        self.mlp = Mlp(in_features=dim, hidden_features=int(dim * mlp_ratio), act_layer=act_layer, drop=drop)


class PatchMerging(Block):
    """as_mlp.py:182-216.  Inside an AS_MLP it runs on its own like the reference's -- (B, C, H, W) -> (B, 2C, H/2, W/2) -- through the
    model's packed weights and kernels (2 x 2 gather + GroupNorm folded into the bias-free reduction GEMM); round 5."""

    def __init__(self, input_resolution, dim, norm_layer=nn.LayerNorm):
        super().__init__()
        self.input_resolution = input_resolution
        self.dim = dim
        self.reduction = nn.Conv2d(4 * dim, 2 * dim, 1, 1, bias=False)
        self.norm = norm_layer(4 * dim)


class BasicLayer(Block):
    """as_mlp.py:228-272.  Inside an AS_MLP a stage runs on its own like the reference's (its blocks, then its PatchMerging); round 5."""

    def __init__(self, dim, input_resolution, depth, shift_size, mlp_ratio=4., as_bias=True, drop=0., drop_path=0.,
                 norm_layer=nn.LayerNorm, downsample=None, use_checkpoint=False):
        super().__init__()
        self.dim = dim
        self.input_resolution = input_resolution
        self.depth = depth
        self.use_checkpoint = use_checkpoint
        self.blocks = nn.ModuleList([
            AxialShiftedBlock(dim=dim, input_resolution=input_resolution, shift_size=shift_size, mlp_ratio=mlp_ratio,
                              as_bias=as_bias, drop=drop, drop_path=drop_path[i] if isinstance(drop_path, list) else drop_path,
                              norm_layer=norm_layer) for i in range(depth)])
        self.downsample = downsample(input_resolution, dim=dim, norm_layer=norm_layer) if downsample is not None else None


class PatchEmbed(Block):
    """as_mlp.py:296-333.  Inside an AS_MLP it runs on its own like the reference's: (B, 3, H, W) -> (B, embed_dim, H/4, W/4); round 5."""

    def __init__(self, img_size=224, patch_size=4, in_chans=3, embed_dim=96, norm_layer=None):
        super().__init__()
        img_size = to_2tuple(img_size)
        patch_size = to_2tuple(patch_size)
        self.img_size = img_size
        self.patch_size = patch_size
        self.patches_resolution = [img_size[0] // patch_size[0], img_size[1] // patch_size[1]]
        self.num_patches = self.patches_resolution[0] * self.patches_resolution[1]
        self.in_chans = in_chans
        self.embed_dim = embed_dim
        self.proj = nn.Conv2d(in_chans, embed_dim, kernel_size=patch_size, stride=patch_size)
        self.norm = norm_layer(embed_dim) if norm_layer is not None else None


def MyNorm(dim):
    """GroupNorm with ONE group (as_mlp.py:343-344)."""
    return nn.GroupNorm(1, dim)


def _gn_params(norm, device):
    if not (isinstance(norm, nn.GroupNorm) and norm.num_groups == 1):
        raise NotImplementedError("the MI355X path implements the reference's MyNorm = GroupNorm(1, C) only")
    return E.f32(norm.weight, device), E.f32(norm.bias, device)


class AS_MLP(StochasticDepth, TrainDropout, E.EngineModule):
    """Same signature and defaults as the reference (as_mlp.py:368-373).

    train() (round 5): the forward applies the blocks' stochastic depth (as_mlp.py:144,159-160: DropPath in front of both residual
    additions) -- see common.StochasticDepth; GroupNorm has no batch statistics.  Forward only: the outputs carry no grad_fn under
    torch.no_grad().  Round 6: with gradients enabled, train() runs `_forward_train` -- every step an autograd.Function whose
    forward and backward are C-ABI calls -- and loss.backward() fills every parameter's .grad.  Dropout (drop_rate: pos_drop and the two
    Mlp.drop of every block, as_mlp.py:16-23,391,430) runs there too -- see common.TrainDropout -- and train() takes that path under
    torch.no_grad() as well whenever a rate is > 0; with every rate 0 the fused path runs as before."""
    _train_forward = True

    def __init__(self, img_size=224, patch_size=4, in_chans=3, num_classes=1000, embed_dim=96, depths=[2, 2, 6, 2],
                 shift_size=5, mlp_ratio=4., as_bias=True, drop_rate=0., drop_path_rate=0.1, norm_layer=MyNorm,
                 patch_norm=True, use_checkpoint=False, **kwargs):
        super().__init__()
        self.num_classes = num_classes
        self.num_layers = len(depths)
        self.embed_dim = embed_dim
        self.patch_norm = patch_norm
        self.num_features = int(embed_dim * 2 ** (self.num_layers - 1))
        self.mlp_ratio = mlp_ratio
        self.patch_embed = PatchEmbed(img_size=img_size, patch_size=patch_size, in_chans=in_chans, embed_dim=embed_dim,
                                      norm_layer=norm_layer if self.patch_norm else None)
        patches_resolution = self.patch_embed.patches_resolution
        self.patches_resolution = patches_resolution
        self.pos_drop = nn.Dropout(p=drop_rate)
        dpr = [v.item() for v in torch.linspace(0, drop_path_rate, sum(depths))]
        self.layers = nn.ModuleList()
        for i_layer in range(self.num_layers):
            self.layers.append(BasicLayer(
                dim=int(embed_dim * 2 ** i_layer),
                input_resolution=(patches_resolution[0] // (2 ** i_layer), patches_resolution[1] // (2 ** i_layer)),
                depth=depths[i_layer], shift_size=shift_size, mlp_ratio=self.mlp_ratio, as_bias=as_bias, drop=drop_rate,
                drop_path=dpr[sum(depths[:i_layer]):sum(depths[:i_layer + 1])], norm_layer=norm_layer,
                downsample=PatchMerging if (i_layer < self.num_layers - 1) else None, use_checkpoint=use_checkpoint))
        self.norm = norm_layer(self.num_features)
        self.avgpool = nn.AdaptiveAvgPool2d(1)
        self.head = nn.Linear(self.num_features, num_classes) if num_classes > 0 else nn.Identity()
        self.apply(self._init_weights)
        self._shift = shift_size
        for li, layer in enumerate(self.layers):
            for bi, blk in enumerate(layer.blocks):
                blk.__dict__["_owner"] = (self, (li, bi))          # lets `model.layers[l].blocks[b](x)` run (common.Block)
            layer.__dict__["_owner"] = (self, (li, "layer"))       # ... `model.layers[l](x)`: the blocks, then the PatchMerging
            if layer.downsample is not None:
                layer.downsample.__dict__["_owner"] = (self, (li, "down"))
        self.patch_embed.__dict__["_owner"] = (self, ("embed", None))

    def _init_weights(self, m):
        # as_mlp.py:419-426: only nn.Linear (= the head) gets the truncated normal
        if isinstance(m, nn.Linear):
            nn.init.trunc_normal_(m.weight, std=.02)
            if m.bias is not None:
                nn.init.constant_(m.bias, 0)
        elif isinstance(m, nn.LayerNorm):
            nn.init.constant_(m.bias, 0)
            nn.init.constant_(m.weight, 1.0)

    def _pack(self, dtype, device):
        pk = {}
        pe = self.patch_embed
        pk["embed.w"] = E.pack_matrix(pe.proj.weight, dtype, device)
        pk["embed.b"] = E.f32(pe.proj.bias, device)
        if pe.norm is not None:
            pk["embed.g"], pk["embed.be"] = _gn_params(pe.norm, device)

        def conv(prefix, c, norm=None):
            """1x1 conv as a GEMM weight; `norm` = the GroupNorm(1,C) in front of it, folded in (gamma into the weights,
            beta into the bias, the per-sample mean / rstd applied on the accumulator, ln_group = H*W)."""
            if norm is None:
                pk[prefix + ".w"] = E.pack_matrix(c.weight, dtype, device)
                pk[prefix + ".b"] = E.f32(c.bias, device) if c.bias is not None else None
            else:
                g, b = _gn_params(norm, device)
                pk[prefix + ".w"], pk[prefix + ".b"], pk[prefix + ".csum"] = E.pack_ln_folded(c.weight, c.bias, g, b, dtype, device)

        for li, layer in enumerate(self.layers):
            for bi, blk in enumerate(layer.blocks):
                p = "l%d.b%d." % (li, bi)
                pk[p + "n1.g"], pk[p + "n1.b"] = _gn_params(blk.norm1, device)
                pk[p + "n2.g"], pk[p + "n2.b"] = _gn_params(blk.norm2, device)
                a = blk.axial_shift
                conv(p + "c1", a.conv1), conv(p + "c21", a.conv2_1), conv(p + "c22", a.conv2_2), conv(p + "c3", a.conv3)
                pk[p + "an1.g"], pk[p + "an1.b"] = _gn_params(a.norm1, device)
                pk[p + "an2.g"], pk[p + "an2.b"] = _gn_params(a.norm2, device)
                conv(p + "fc1", blk.mlp.fc1), conv(p + "fc2", blk.mlp.fc2)
                # the same three convolutions with the GroupNorm in front of them folded in (16-bit fast path)
                conv(p + "c1f", a.conv1, blk.norm1), conv(p + "c3f", a.conv3, a.norm2), conv(p + "fc1f", blk.mlp.fc1, blk.norm2)
                fc1, fc2 = blk.mlp.fc1, blk.mlp.fc2
                if E.channel_mlp_fused_supported(dtype, fc1.in_channels, fc1.out_channels) and fc2.out_channels == fc1.in_channels:
                    # narrow stages (C = 96, 192): norm2 + fc1 + GELU + fc2 + residual in one kernel (mlpk_channel_mlp)
                    g, b = _gn_params(blk.norm2, device)
                    pk[p + "mlpf"] = E.pack_channel_mlp_fused(fc1.weight, fc1.bias, fc2.weight, fc2.bias, dtype, device, g, b)
            if layer.downsample is not None:
                p = "l%d.down." % li
                pk[p + "g"], pk[p + "b"] = _gn_params(layer.downsample.norm, device)
                pk[p + "w"] = E.pack_matrix(layer.downsample.reduction.weight, dtype, device)
                conv(p + "f", layer.downsample.reduction, layer.downsample.norm)
                if dtype != torch.float32 and (p + "f.w") in pk:
                    pk[p + "f.wc"] = E.merge_taps(pk[p + "f.w"], pk[p + "f.w"].shape[1] // 4)     # round 6: the reduction as an implicit-convolution product
        pk["norm.g"], pk["norm.b"] = _gn_params(self.norm, device)
        if isinstance(self.head, nn.Linear):
            pk["head.w"] = E.pack_matrix(self.head.weight, dtype, device)
            pk["head.b"] = E.f32(self.head.bias, device)
        return pk

    @staticmethod
    def _gn(ws, tag, x, B, HW, C, g, b, out, act=N.ACT_NONE):
        """GroupNorm(1,C) of channel-last x (B*HW, C) -> out (may alias x), optional GELU."""
        mean = ws.get(tag + ".mean", (B,), torch.float32)
        rstd = ws.get(tag + ".rstd", (B,), torch.float32)
        E.row_stats(x, B, HW * C, HW * C, mean, rstd)
        E.norm_apply(x, B * HW, C, C, mean=mean, rstd=rstd, gamma=g, beta=b, act=act, stat_group=HW, out_rm=out, ld_rm=C)
        return out

    def _run_layers(self, ws, pk, cur, B, H, W, C, cd, only=None):
        """The stages on channel-last rows `cur` (B*H*W, C).  only = (layer, block): that one block alone, on a `cur` that already has
        the layer's resolution and width (AxialShiftedBlock called on its own).  Returns (cur, H, W, C, have, mean, rstd)."""
        mean = rstd = None
        have = False          # (mean, rstd) of the current layer already hold the per-sample statistics of `cur`
        for li, layer in enumerate(self.layers):
            if only is not None and li != only[0]:
                continue
            rows, HW = B * H * W, H * W
            t0 = ws.get("l%d.t0" % li, (rows, C))
            t1 = ws.get("l%d.t1" % li, (rows, C))
            t2 = ws.get("l%d.t2" % li, (rows, C))
            hid = int(C * self.mlp_ratio)
            hbuf = ws.get("l%d.h" % li, (rows, hid))
            tag = "l%d.gn" % li
            # 16-bit fast path: a GroupNorm(1,C) in front of a 1x1 conv is folded into that GEMM (per-sample statistics on the
            # accumulator, ln_group = H*W rows per statistic), and AxialShift's GroupNorm -> GELU -> two shifts is ONE
            # index-remapping pass that writes both shifted operands directly (t itself is never stored): per block 5
            # statistics passes, 1 normalise+shift pass and 6 GEMMs instead of 5 + 5 + 2 + 6 kernels.  fp32 and shapes the
            # remap kernel does not take (channel groups narrower than 8) keep the unfused sequence.
            fused = cd != torch.float32 and C % 8 == 0 and (C + self._shift - 1) // self._shift >= 8
            mean = ws.get(tag + ".mean", (B,), torch.float32)
            rstd = ws.get(tag + ".rstd", (B,), torch.float32)
            have = False

            def stats(t):
                # per-sample statistics: a pass over t
                E.row_stats(t, B, HW * C, HW * C, mean, rstd)

            for bi in range(len(layer.blocks)):
                if only is not None and only[1] != "layer" and bi != only[1]:
                    continue
                p = "l%d.b%d." % (li, bi)
                if fused:
                    if not have:
                        stats(cur)
                    E.gemm(cur, pk[p + "c1f.w"], t1, rows, C, C, bias=pk[p + "c1f.b"], ln=(mean, rstd, pk[p + "c1f.csum"]), ln_group=HW,
                           tag="as_conv")                                                            # conv1(norm1(x))
                    stats(t1)
                    if pk.get(p + "c21.b") is not None and pk.get(p + "c22.b") is not None and E.as_conv2_supported(cd, H, W, C, self._shift):
                        # round 4 (stages with C = 96 / 192): GroupNorm + GELU, both axial shifts, conv2_1, conv2_2, their GELUs and the sum
                        # in ONE kernel -- the shifts are LDS read addresses of the matrix-core operands (mlpk_as_conv2); bit-equal to the
                        # three kernels below, 2 tensor passes over HBM instead of 9
                        # (round 6: ... and the statistics of the sum for norm2, finished inside the kernel: no pass over it)
                        st2 = E.as_conv2(t1, t0, B, H, W, C, self._shift, mean, rstd, pk[p + "an1.g"], pk[p + "an1.b"],
                                         pk[p + "c21.w"], pk[p + "c21.b"], pk[p + "c22.w"], pk[p + "c22.b"], stats=(ws, tag + ".asc"))
                        t0, t1 = t1, t0                                                              # the sum now lives in what was t0
                    else:
                        st2 = None
                        E.norm_shift_nhwc(t1, t0, t2, B, H, W, C, self._shift, mean, rstd, pk[p + "an1.g"], pk[p + "an1.b"], N.ACT_GELU)
                        E.gemm(t0, pk[p + "c21.w"], t1, rows, C, C, bias=pk[p + "c21.b"], act=N.ACT_GELU, tag="as_conv")      # x_lr (W shift)
                        E.gemm(t2, pk[p + "c22.w"], t1, rows, C, C, bias=pk[p + "c22.b"], act=N.ACT_GELU, R=t1, res=N.RES_ADD,
                               tag="as_conv")                                                        # gelu(.) + x_lr (H shift)
                        stats(t1)
                        st2 = (mean, rstd)
                    dp1 = self._drop_scale(layer.blocks[bi].drop_path_rate, B, HW, cd, cur.device)  # train mode: x + drop_path(.) (as_mlp.py:159)
                    E.gemm(t1, pk[p + "c3f.w"], cur, rows, C, C, bias=pk[p + "c3f.b"], ln=(st2[0], st2[1], pk[p + "c3f.csum"]), ln_group=HW,
                           R=cur, res=N.RES_ADD, tag="as_conv", rscale=dp1, rperiod=rows if dp1 is not None else 0)  # x + conv3(norm2(.))
                    stats(cur)
                    dp2 = self._drop_scale(layer.blocks[bi].drop_path_rate, B, HW, cd, cur.device)  # ... x + drop_path(mlp(norm2(x))) (:160)
                    if dp2 is not None:
                        E.gemm(cur, pk[p + "fc1f.w"], hbuf, rows, hid, C, bias=pk[p + "fc1f.b"], act=N.ACT_GELU,
                               ln=(mean, rstd, pk[p + "fc1f.csum"]), ln_group=HW, tag="as_fc1")
                        E.gemm(hbuf, pk[p + "fc2.w"], cur, rows, C, hid, bias=pk[p + "fc2.b"], R=cur, res=N.RES_ADD, tag="as_fc2",
                               rscale=dp2, rperiod=rows)
                        got = None
                    elif (p + "mlpf") in pk and E.channel_mlp_fused_supported(cd, C, hid):
                        # (its by-product statistics are one plane, summed inside a wave: always taken -- unlike the s3 tile's, whose
                        # statistics epilogue costs more than the pass it saves, profiles/r04_epilogue_stats_ab.txt)
                        got = E.channel_mlp_fused(cur, rows, C, pk[p + "mlpf"], cur, R=cur, ln=(mean, rstd), ln_group=HW,
                                                  part=(ws, "l%d.mlppart" % li))
                    else:
                        E.gemm(cur, pk[p + "fc1f.w"], hbuf, rows, hid, C, bias=pk[p + "fc1f.b"], act=N.ACT_GELU,
                               ln=(mean, rstd, pk[p + "fc1f.csum"]), ln_group=HW, tag="as_fc1")
                        E.gemm(hbuf, pk[p + "fc2.w"], cur, rows, C, hid, bias=pk[p + "fc2.b"], R=cur, res=N.RES_ADD, tag="as_fc2")
                        got = None
                    # (mean, rstd) then describe `cur`: the next block's norm1, the PatchMerging norm (a permutation of the same
                    # elements per sample, as_mlp.py:207-213) or the final norm start from them
                    have = finalize_stats(ws, got, rows, C, tag=tag, group=HW) is not None
                    continue
                have = False                                                                         # (each _gn below computes its own)
                self._gn(ws, tag, cur, B, HW, C, pk[p + "n1.g"], pk[p + "n1.b"], t0)                 # norm1(x)
                E.gemm(t0, pk[p + "c1.w"], t1, rows, C, C, bias=pk[p + "c1.b"], tag="as_conv")       # conv1
                self._gn(ws, tag, t1, B, HW, C, pk[p + "an1.g"], pk[p + "an1.b"], t1, act=N.ACT_GELU)  # GN -> GELU
                E.shift_nhwc(t1, t0, B, H, W, C, self._shift, 3)                                     # shift along W
                E.gemm(t0, pk[p + "c21.w"], t2, rows, C, C, bias=pk[p + "c21.b"], act=N.ACT_GELU, tag="as_conv")
                E.shift_nhwc(t1, t0, B, H, W, C, self._shift, 2)                                     # shift along H
                E.gemm(t0, pk[p + "c22.w"], t2, rows, C, C, bias=pk[p + "c22.b"], act=N.ACT_GELU, R=t2, res=N.RES_ADD,
                       tag="as_conv")                                                                # gelu(.) + x_lr
                self._gn(ws, tag, t2, B, HW, C, pk[p + "an2.g"], pk[p + "an2.b"], t2)
                dp1 = self._drop_scale(layer.blocks[bi].drop_path_rate, B, HW, cd, cur.device)
                E.gemm(t2, pk[p + "c3.w"], cur, rows, C, C, bias=pk[p + "c3.b"], R=cur, res=N.RES_ADD, tag="as_conv",
                       rscale=dp1, rperiod=rows if dp1 is not None else 0)
                self._gn(ws, tag, cur, B, HW, C, pk[p + "n2.g"], pk[p + "n2.b"], t0)                 # norm2(x)
                E.gemm(t0, pk[p + "fc1.w"], hbuf, rows, hid, C, bias=pk[p + "fc1.b"], act=N.ACT_GELU, tag="as_fc1")
                dp2 = self._drop_scale(layer.blocks[bi].drop_path_rate, B, HW, cd, cur.device)
                E.gemm(hbuf, pk[p + "fc2.w"], cur, rows, C, hid, bias=pk[p + "fc2.b"], R=cur, res=N.RES_ADD, tag="as_fc2",
                       rscale=dp2, rperiod=rows if dp2 is not None else 0)
            if layer.downsample is not None and (only is None or only[1] in ("layer", "down")):
                assert H % 2 == 0 and W % 2 == 0, f"x size ({H}*{W}) are not even."                   # as_mlp.py:203
                p = "l%d.down." % li
                H2, W2 = H // 2, W // 2
                nxt = ws.get("l%d.x" % (li + 1), (B * H2 * W2, 2 * C))
                implicit = cd != torch.float32 and (p + "f.wc") in pk and pk[p + "f.w"].shape[1] == 4 * C and E.conv_gemm_nhwc_supported(cd, C, 2, 2, 2, 0)
                if implicit:
                    # round 6: no merged tensor -- GroupNorm(1, 4C) of it normalises over the same elements per sample as one over `cur`, and the
                    # reduction reads `cur` through the 2 x 2 window (mlpk_conv_gemm_nhwc, the weight's column blocks in its tap order)
                    if have:
                        mm, mr = mean, rstd
                    else:
                        mm = ws.get("l%d.gnm.mean" % li, (B,), torch.float32)
                        mr = ws.get("l%d.gnm.rstd" % li, (B,), torch.float32)
                        E.row_stats(cur, B, H * W * C, H * W * C, mm, mr)
                    E.conv_gemm_nhwc(cur, pk[p + "f.wc"], nxt, B, H, W, C, 2, 2, 2, 0, bias=pk[p + "f.b"], ln=(mm, mr, pk[p + "f.csum"]),
                                     ln_group=H2 * W2, tag="as_merge")
                    cur, H, W, C = nxt, H2, W2, 2 * C
                    continue
                merged = ws.get("l%d.merged" % li, (B * H2 * W2, 4 * C))
                E.patchify(cur, merged, B, C, H, W, 2, 2, 0, 4 * C, layout=N.LAYOUT_NHWC, px_stride=C, order=1)
                if cd != torch.float32:
                    if have:
                        # GroupNorm(1, 4C) of the merged tensor (as_mlp.py:212) normalises over the same elements per sample as
                        # a GroupNorm(1, C) of `cur` would: the statistics the last fc2 epilogue delivered are its statistics
                        mm, mr = mean, rstd
                    else:
                        mm = ws.get("l%d.gnm.mean" % li, (B,), torch.float32)
                        mr = ws.get("l%d.gnm.rstd" % li, (B,), torch.float32)
                        E.row_stats(merged, B, H2 * W2 * 4 * C, H2 * W2 * 4 * C, mm, mr)
                    E.gemm(merged, pk[p + "f.w"], nxt, B * H2 * W2, 2 * C, 4 * C, bias=pk[p + "f.b"], ln=(mm, mr, pk[p + "f.csum"]),
                           ln_group=H2 * W2, tag="as_merge")
                else:
                    self._gn(ws, "l%d.gnm" % li, merged, B, H2 * W2, 4 * C, pk[p + "g"], pk[p + "b"], merged)
                    E.gemm(merged, pk[p + "w"], nxt, B * H2 * W2, 2 * C, 4 * C, tag="as_merge")
                cur, H, W, C = nxt, H2, W2, 2 * C
        return cur, H, W, C, have, mean, rstd

    def _embed(self, ws, pk, x, B, H_in, W_in):
        pe = self.patch_embed
        ph, pw = pe.patch_size
        H, W = H_in // ph, W_in // pw
        C = self.embed_dim
        kp = pk["embed.w"].shape[1]
        cur = ws.get("l0.x", (B * H * W, C))
        if (ph, pw) == (4, 4) and x.data_ptr() % 16 == 0 and E.patch_embed4_supported(x.dtype, cur.dtype, pe.in_chans, H_in, W_in, C):
            E.patch_embed4(x, pk["embed.w"], pk["embed.b"], cur, B, H_in, W_in, C)            # round 6: gather + product in one kernel
        else:
            patches = ws.get("embed.patches", (B * H * W, kp))
            E.patchify(x, patches, B, pe.in_chans, H_in, W_in, ph, pw, 0, kp)
            E.gemm(patches, pk["embed.w"], cur, B * H * W, C, kp, bias=pk["embed.b"])
        if pe.norm is not None:
            self._gn(ws, "gn0", cur, B, H * W, C, pk["embed.g"], pk["embed.be"], cur)
        return cur, H, W, C

    def _run_single(self, key, x):
        """An inner module alone on (B, C, H, W), as calling it does in the reference: `model.layers[l].blocks[b](x)` (as_mlp.py:149-162),
        `model.layers[l](x)` (a stage: :258-266), `model.layers[l].downsample(x)` (:197-216), `model.patch_embed(x)` (:323-333)"""
        li, bi = key
        E.require_gpu(x, "AS_MLP inner module")
        E.dtype_code(x.dtype)
        if li == "embed":
            pe = self.patch_embed
            B, _, H_in, W_in = x.shape
            assert H_in == pe.img_size[0] and W_in == pe.img_size[1], \
                f"Input image size ({H_in}*{W_in}) doesn't match model ({pe.img_size[0]}*{pe.img_size[1]})."
            with E.on_device(x):
                pk = self._get_pack(x.dtype, x.device)
                ws = self._get_space(("embed", B, H_in, W_in), x.dtype, x.device)
                cur, H, W, C = self._embed(ws, pk, x.contiguous(), B, H_in, W_in)
                return cur.reshape(B, H, W, C).permute(0, 3, 1, 2).contiguous()
        C = self.layers[li].dim
        if x.dim() != 4 or x.shape[1] != C:
            raise ValueError("expected a (B, %d, H, W) tensor" % C)
        B, _, H, W = x.shape
        with E.on_device(x):
            pk = self._get_pack(x.dtype, x.device)
            ws = self._get_space(("block", B, H, W, C), x.dtype, x.device)     # (C: blocks of different stages can meet at one map size)
            cur = ws.get("l%d.x" % li, (B * H * W, C))
            cur.copy_(x.permute(0, 2, 3, 1).reshape(B * H * W, C))                     # channel-last rows, as the stages keep them
            cur, H, W, C = self._run_layers(ws, pk, cur, B, H, W, C, x.dtype, only=(li, bi))[:4]
            return cur.reshape(B, H, W, C).permute(0, 3, 1, 2).contiguous()

    def _forward_train(self, x):
        """Train mode WITH autograd (round 6, SURVEY 8f-4: the review's "AS-MLP block backward built on the Shift op's backward kernel"): the same
        mathematics as forward() with every step an autograd.Function of `..autograd` whose forward and backward are C-ABI calls -- 1x1
        convolutions = mlpk_gemm_nt (dX, dW as GEMMs on transposed operands), GroupNorm(1, C) = mlpk_row_stats + mlpk_norm_apply /
        mlpk_group_norm_backward, GELU = mlpk_gelu_elementwise, the two axial shifts = mlpk_shift_nhwc / mlpk_shift_nhwc_backward (the
        reference's shift_backward_grad_input_kernel, utils/shift_cuda.py:75-103, on the channel-last layout), PatchMerging's gather =
        mlpk_merge2x2_nhwc and its adjoint, stochastic depth = a per-sample row scale, Dropout = mlpk_dropout on the channel-last rows
        (as_mlp.py:8-24,55-95,118-162,197-216,428-443).
        Unfused on purpose: the pre-activations and normalised tensors are what the backward needs.  No gradient w.r.t. the input image."""
        from .. import autograd as AG
        cd = train_entry(self, x)
        pe = self.patch_embed
        B, _, H_in, W_in = x.shape
        assert H_in == pe.img_size[0] and W_in == pe.img_size[1], \
            f"Input image size ({H_in}*{W_in}) doesn't match model ({pe.img_size[0]}*{pe.img_size[1]})."

        def gn(t, norm):
            return AG.group_norm1(t, norm, B)

        def rate(drop):
            return float(drop.p) if self.training else 0.0

        seed = self.dropout_seed() if self._dropout_active() else 0
        t, H, W = AG.conv_rows(x, pe.proj, cd)
        if pe.norm is not None:
            t = gn(t, pe.norm)
        t = AG.dropout(t, rate(self.pos_drop), seed, 0)                                      # pos_drop (as_mlp.py:430)
        j = 0
        for layer in self.layers:
            HW = H * W
            for blk in layer.blocks:
                a = blk.axial_shift
                u = AG.Gelu.apply(gn(AG.linear(gn(t, blk.norm1), a.conv1), a.norm1))
                x_lr = AG.Gelu.apply(AG.linear(AG.ShiftNHWC.apply(u, B, H, W, self._shift, 3), a.conv2_1))
                x_td = AG.Gelu.apply(AG.linear(AG.ShiftNHWC.apply(u, B, H, W, self._shift, 2), a.conv2_2))
                s = gn(AG.ScaleAdd.apply(x_lr, x_td, None), a.norm2)
                if float(blk.drop_path_rate) > 0.0:
                    t = AG.drop_add(self, t, AG.linear(s, a.conv3), blk.drop_path_rate, B, HW)       # x + drop_path(.) (as_mlp.py:159)
                else:
                    t = AG.linear(s, a.conv3, t)
                t = AG.drop_mlp_add(self, t, gn(t, blk.norm2), blk.mlp, blk.drop_path_rate, rate(blk.mlp.drop), seed, 1 + 2 * j, B, HW)
                j += 1
            if layer.downsample is not None:
                assert H % 2 == 0 and W % 2 == 0, f"x size ({H}*{W}) are not even."
                ds = layer.downsample
                t = AG.linear(gn(AG.Merge2x2.apply(t, B, H, W), ds.norm), ds.reduction)
                H, W = H // 2, W // 2
        pooled = AG.TokenMean.apply(gn(t, self.norm), B, H * W)
        if not isinstance(self.head, nn.Linear):
            return pooled.to(x.dtype)
        return AG.linear(pooled, self.head).to(x.dtype)

    def _dropout_modules(self):
        return [self.pos_drop] + [blk.mlp.drop for layer in self.layers for blk in layer.blocks]

    def forward(self, x):
        if self._train_path():
            return self._forward_train(x)
        cd = self._resolve(x)
        pe = self.patch_embed
        B, _, H_in, W_in = x.shape
        # FIXME-free restatement of as_mlp.py:328: the input size must match the constructor's
        assert H_in == pe.img_size[0] and W_in == pe.img_size[1], \
            f"Input image size ({H_in}*{W_in}) doesn't match model ({pe.img_size[0]}*{pe.img_size[1]})."
        pk = self._get_pack(cd, x.device)
        ws = self._get_space(B, cd, x.device)
        cur, H, W, C = self._embed(ws, pk, x.contiguous(), B, H_in, W_in)
        cur, H, W, C, have, mean, rstd = self._run_layers(ws, pk, cur, B, H, W, C, cd)
        if not have:
            mean = ws.get("final.mean", (B,), torch.float32)
            rstd = ws.get("final.rstd", (B,), torch.float32)
            E.row_stats(cur, B, H * W * C, H * W * C, mean, rstd)
        pooled = ws.get("pooled", (B, C))
        E.pool_mean(cur, B, H * W, C, C, pooled, C, mean=mean, rstd=rstd, stat_group=H * W, gamma=pk["norm.g"], beta=pk["norm.b"])
        if not isinstance(self.head, nn.Linear):
            out = pooled.clone()
            return out if out.dtype == x.dtype else out.to(x.dtype)
        return head_linear(ws, pooled, B, C, pk["head.w"], pk["head.b"], self.num_classes, x.dtype)
