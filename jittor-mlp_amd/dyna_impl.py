"""DynaMixer, drop-in for the reference's models_pytorch/dyna_mlp.py: the same classes, constructor signatures, defaults, the module-level
`dynamlp_settings` table and the same state_dict keys and shapes; `models_pytorch/dyna_mlp.py` gives them the reference's import path.  The classes
are defined here, beside the engine, because every EngineModule subclass defined under models_pytorch must have a row in the tables of
tests/test_gpu_lifecycle.py; moving the family there is a later change (RaftMLP arrived the same way).  Inference-only: train() takes the
engine's warning path (DropPath and Dropout run as the identity).  The parameterless einops slots of the reference's module tree are `Layout`
placeholders, so the indices of `attend` and `mlp_head` (and with them the keys) are the reference's.

The forward runs on channel-last rows x[(b, h, w), c].  Per DynaBlock behind its PreNorm (dyna_mlp.py:96-111), s = segment, hd = hidden_dim_DMO:
  mean, rstd = row statistics of x                     the by-product of the previous GEMM's epilogue where it delivers them, else mlpk_row_stats
  cat[:, 2C:3C] = xn = LayerNorm(x)                    mlpk_norm_apply into a column block of the (rows, 3C) buffer `cat`
  t = [Wd_h(xn) | Wd_w(xn)]                            ONE GEMM for the 2 s Linears of both axes (rows, 2 s hd)
  cat[:, 0:C]  = mix along h, cat[:, C:2C] = along w   per axis (`mix_rows`): attend.1, the softmax and the L x L mix per (image, line, segment), x normalised
                                                       on load.  16-bit types, lines of 8 to 32 positions (engine.dyna_unfused_preferred): the UNFUSED form --
                                                       mlpk_dyna_gather, ONE GEMM for the logits, mlpk_dyna_mix_logits --, 7-20 % faster in the alternating
                                                       measurement (profiles/dyna_mix_fused_vs_unfused.jsonl); otherwise the fused mlpk_dyna_mix, whose
                                                       logits never reach memory.  Both run one device function for the softmax and the mix.
  x += [Wo Wh | Wo Ww | Wo Wc] cat + Wo (bh + bw + bc) + bo     ONE GEMM with K = 3C: proc_h, proc_w, proj_c and proj_o folded at pack time
                                                       (`fold_projections`, in fp64, rounded once to the compute type)
then the channel MLP (common.channel_mlp, LayerNorm folded into fc1).  Stage 1 embeds the NCHW image (embed_patches), stage 2 the channel-last rows
(stage_embed); the head is mlpk_pool_mean and one GEMM.

`DynaMixer`, `DynaMLPBlock` (NCHW in and out), `DynaBlock`, `DynaMixerOp_h` and `DynaMixerOp_w` ((b, h, w, C) in and out, already normalised, as
the reference calls them) run on their own on the GPU.  `PreNorm` and `FeedForward` hold parameters and raise NotImplementedError when called.
A shape mlpk_dyna_mix does not take (a line longer than 32, L hd > 256, a segment that is not a whole number of 16-byte vectors, C % 8 != 0)
raises NotImplementedError naming it; there is no fallback path.
"""
import torch
from torch import nn

from . import _native as N
from . import engine as E
from .models_pytorch.common import (SubModule, channel_mlp, embed_patches, finalize_stats, head_linear, layernorm_stats, pack_channel_mlp,
                                    stage_embed)


def pair(t):
    return t if isinstance(t, tuple) else (t, t)


class Layout(nn.Module):
    """Stands where the reference has a parameterless einops layer (Rearrange / Reduce): keeps the indices of the module tree, and with them the
    state_dict keys.  The layout change itself is index arithmetic inside the kernels."""

    def __init__(self, pattern=""):
        super().__init__()
        self.pattern = pattern

    def extra_repr(self):
        return repr(self.pattern)

    def forward(self, x):
        raise NotImplementedError("Layout(%r) is a placeholder inside DynaMixer: call the enclosing DynaMixer or one of its callable blocks" % self.pattern)


class _Container(nn.Module):
    """Holds parameters; the enclosing block packs them into its own kernel sequence and never calls the module."""

    def forward(self, *a, **k):
        raise NotImplementedError("%s only holds parameters inside DynaMixer: call the enclosing DynaMixer, DynaMLPBlock or DynaBlock" % type(self).__name__)


class PreNorm(_Container):
    """dyna_mlp.py:13-19"""

    def __init__(self, dim, fn):
        super().__init__()
        self.norm = nn.LayerNorm(dim)
        self.fn = fn


class FeedForward(_Container):
    """dyna_mlp.py:21-32"""

    def __init__(self, dim, hidden_dim, dropout=0.):
        super().__init__()
        self.net = nn.Sequential(
            nn.Linear(dim, hidden_dim),
            nn.GELU(),
            nn.Dropout(dropout),
            nn.Linear(hidden_dim, dim),
            nn.Dropout(dropout)
        )


class DropPath(nn.Module):
    """timm's DropPath where the reference puts it (dyna_mlp.py:117); the forward built here is inference-only and never calls it"""

    def __init__(self, drop_prob=0.):
        super().__init__()
        self.drop_prob = drop_prob

    def forward(self, x):
        return x


# ------------------------------------------------------------------ packing (pure functions: they run on CPU tensors too)
def cat_wd(ops, device):
    """the `Wd` Linears of the given DynaMixerOps, in order, as one (len(ops) s hd, C) fp32 weight and its bias: row g hd + j of an op's block
    is Wd[g]'s row j, the order of torch.cat(x_, -1) (dyna_mlp.py:54-57)"""
    w = torch.cat([lin.weight.detach().to(device=device, dtype=torch.float32) for op in ops for lin in op.Wd], 0)
    b = torch.cat([lin.bias.detach().to(device=device, dtype=torch.float32) for op in ops for lin in op.Wd], 0)
    return w, b


def fold_projections(blk, device):
    """proj_o(proc_h(mh) + proc_w(mw) + proj_c(xn)) = [Wo Wh | Wo Ww | Wo Wc] [mh | mw | xn] + Wo (bh + bw + bc) + bo: fp32 (C, 3C) and (C),
    the products taken in fp64"""
    f = lambda v: v.detach().to(device=device, dtype=torch.float64)
    wo, bo = f(blk.proj_o.weight), f(blk.proj_o.bias)
    oh, ow, pc = blk.DynaMixerOp_h.proc, blk.DynaMixerOp_w.proc, blk.proj_c
    w3 = torch.cat([wo @ f(oh.weight), wo @ f(ow.weight), wo @ f(pc.weight)], 1)
    b3 = wo @ (f(oh.bias) + f(ow.bias) + f(pc.bias)) + bo
    return w3.float().contiguous(), b3.float().contiguous()


def pack_op(pk, p, op, dtype, device):
    """a DynaMixerOp on its own under prefix p"""
    w, b = cat_wd([op], device)
    pk[p + "wd.w"], pk[p + "wd.b"] = E.pack_matrix(w, dtype, device), E.f32(b, device)
    pk[p + "aw"], pk[p + "ab"] = E.pack_dyna_attend(op.attend[1].weight, op.attend[1].bias, dtype, device)
    pk[p + "awr"] = E.pack_matrix(op.attend[1].weight, dtype, device)             # row-major, for the unfused form's GEMM
    pk[p + "proc.w"], pk[p + "proc.b"] = E.pack_matrix(op.proc.weight, dtype, device), E.f32(op.proc.bias, device)


def pack_block(pk, p, blk, norm, dtype, device):
    """a DynaBlock under prefix p; norm = the PreNorm's LayerNorm, or None for the block on its own (its input is already normalised)"""
    if norm is not None:
        pk[p + "ln.g"], pk[p + "ln.b"] = E.f32(norm.weight, device), E.f32(norm.bias, device)
    w, b = cat_wd([blk.DynaMixerOp_h, blk.DynaMixerOp_w], device)
    pk[p + "wd.w"], pk[p + "wd.b"] = E.pack_matrix(w, dtype, device), E.f32(b, device)
    for k, op in (("h.", blk.DynaMixerOp_h), ("w.", blk.DynaMixerOp_w)):
        pk[p + k + "aw"], pk[p + k + "ab"] = E.pack_dyna_attend(op.attend[1].weight, op.attend[1].bias, dtype, device)
        pk[p + k + "awr"] = E.pack_matrix(op.attend[1].weight, dtype, device)     # row-major, for the unfused form's GEMM
    w3, b3 = fold_projections(blk, device)
    pk[p + "o.w"], pk[p + "o.b"] = E.pack_matrix(w3, dtype, device), E.f32(b3, device)


def pack_layers(pk, p, mlp_block, dtype, device):
    """a DynaMLPBlock's layers under prefix p"""
    for j, (attn, ff) in enumerate(mlp_block.layers):
        q = "%sb%d." % (p, j)
        pack_block(pk, q, attn.fn, attn.norm, dtype, device)
        pack_channel_mlp(pk, q + "ff.", ff.norm, ff.fn.net[0], ff.fn.net[3], dtype, device)


# ------------------------------------------------------------------ forward pieces on channel-last rows
def require_shape(what, dtype, H, W, C, s, hd):
    if C % 8 or not (E.dyna_mix_supported(dtype, H, C, s, hd) and E.dyna_mix_supported(dtype, W, C, s, hd)):
        raise NotImplementedError("%s: mlpk_dyna_mix does not take a %d x %d map of %d channels in %d segments (hidden_dim_DMO %d) in %s" % (
            what, H, W, C, s, hd, dtype))


def mix_rows(ws, tag, pk, q, src, mean, rstd, g, b, t, t_off, out, B, H, W, C, s, hd, axis):
    """one axis of the dynamic mixing: the unfused form (gather, GEMM, mlpk_dyna_mix_logits) where engine.dyna_unfused_preferred says it is the
    faster one, else the fused mlpk_dyna_mix"""
    if E.dyna_unfused_preferred(src.dtype, (H, W)[axis]):
        E.dyna_mix_unfused(ws, tag, src, mean, rstd, g, b, t, t_off, pk[q + "awr"], pk[q + "ab"], out, B, H, W, C, s, hd, axis)
    else:
        E.dyna_mix(src, mean, rstd, g, b, t, t_off, pk[q + "aw"], pk[q + "ab"], out, B, H, W, C, s, hd, axis)


def block_rows(ws, pk, p, src, stats, B, H, W, C, s, hd, tag, out, residual):
    """DynaBlock on rows: out = [out +] proj_o(Y_h + Y_w + Y_c) of LayerNorm(src) (stats None: `src` is already normalised).  Returns what the
    last GEMM's `part` delivered (residual only)."""
    rows, nt = B * H * W, 2 * s * hd
    cat = ws.get(tag + ".cat", (rows, 3 * C))
    xn = cat[:, 2 * C:]
    if stats is not None:
        mean, rstd, g, b = stats[0], stats[1], pk[p + "ln.g"], pk[p + "ln.b"]
        E.norm_apply(src, rows, C, src.stride(0), mean=mean, rstd=rstd, gamma=g, beta=b, out_rm=xn, ld_rm=3 * C)
    else:
        mean = rstd = g = b = None
        xn.copy_(src)
    t = ws.get(tag + ".t", (rows, E.round_up(nt, 8)))
    E.gemm(xn, pk[p + "wd.w"], t, rows, nt, C, bias=pk[p + "wd.b"], tag="dyna_wd")
    mix_rows(ws, tag, pk, p + "h.", src, mean, rstd, g, b, t, 0, cat[:, :C], B, H, W, C, s, hd, 0)
    mix_rows(ws, tag, pk, p + "w.", src, mean, rstd, g, b, t, s * hd, cat[:, C:2 * C], B, H, W, C, s, hd, 1)
    if residual:
        return E.gemm(cat, pk[p + "o.w"], out, rows, C, 3 * C, bias=pk[p + "o.b"], R=out, res=N.RES_ADD, tag="dyna_proj", part=(ws, tag + ".o.part"))
    E.gemm(cat, pk[p + "o.w"], out, rows, C, 3 * C, bias=pk[p + "o.b"], tag="dyna_proj")
    return None


def layers_rows(ws, pk, p, depth, cur, B, H, W, C, s, hd, hidden, tag):
    """a DynaMLPBlock's layers in place on rows (B*H*W, C)"""
    rows = B * H * W
    st = None
    for j in range(depth):
        q = "%sb%d." % (p, j)
        if st is None:
            st = layernorm_stats(ws, cur, rows, C, tag=tag + ".ln")
        got = block_rows(ws, pk, q, cur, st, B, H, W, C, s, hd, tag, cur, residual=True)
        got = channel_mlp(ws, cur, rows, C, pk, q + "ff.", hidden, tag=tag + ".cm", stats=finalize_stats(ws, got, rows, C, tag=tag + ".cm.ln"),
                          part=(ws, tag + ".fc2.part"))
        st = finalize_stats(ws, got, rows, C, tag=tag + ".ln")


class _DynaMixerOp(SubModule):
    """dyna_mlp.py:34-94.  Callable on its own like the reference's: x (b, h, w, C), already normalised -> (b, h, w, C)."""
    AXIS = 0

    def __init__(self, length, dim, hidden_dim, segment):
        super().__init__()
        a = "h" if self.AXIS == 0 else "w"
        o = "w" if self.AXIS == 0 else "h"
        self.segment = segment
        self.reshape = Layout("b h w (s d) -> b %s s %s d" % (o, a))
        self.Wd = nn.ModuleList([nn.Linear(dim, hidden_dim) for i in range(segment)])
        self.attend = nn.Sequential(
            Layout("b h w (s d) -> b %s s (%s d)" % (o, a)),
            nn.Linear(int(hidden_dim * length), length * length),
            Layout("b %s s (%s1 %s2) -> b %s s %s1 %s2" % (o, a, a, o, a, a)),
            nn.Softmax(dim=-1),
        )
        self.recover = Layout("b %s s %s d -> b h w (s d)" % (o, a))
        self.proc = nn.Linear(dim, dim)

    def _pack(self, dtype, device):
        pk = {}
        pack_op(pk, "", self, dtype, device)
        return pk

    def forward(self, x):
        C, s, hd = self.proc.in_features, self.segment, self.Wd[0].out_features
        L = self.attend[1].out_features // max(self.attend[1].in_features // hd, 1)
        pk = self._begin(x, C)
        if x.dim() != 4 or x.shape[1 + self.AXIS] != L:
            raise ValueError("expected a channel-last (b, h, w, %d) tensor with %d positions along %s" % (C, L, "hw"[self.AXIS]))
        B, H, W, _ = x.shape
        if C % 8 or not E.dyna_mix_supported(x.dtype, L, C, s, hd):
            raise NotImplementedError("%s: mlpk_dyna_mix does not take lines of %d positions of %d channels in %d segments (hidden_dim_DMO %d) in %s" % (
                type(self).__name__, L, C, s, hd, x.dtype))
        rows, nt = B * H * W, s * hd
        with E.on_device(x):
            ws = self._get_space((B, H, W), x.dtype, x.device)
            xb = ws.get("op.x", (rows, C))
            xb.copy_(x.reshape(rows, C))
            t = ws.get("op.t", (rows, E.round_up(nt, 8)))
            E.gemm(xb, pk["wd.w"], t, rows, nt, C, bias=pk["wd.b"], tag="dyna_wd")
            m = ws.get("op.m", (rows, C))
            mix_rows(ws, "op", pk, "", xb, None, None, None, None, t, 0, m, B, H, W, C, s, hd, self.AXIS)
            out = ws.get("op.out", (rows, C))
            E.gemm(m, pk["proc.w"], out, rows, C, C, bias=pk["proc.b"], tag="dyna_proc")
            return out.reshape(B, H, W, C).clone()


class DynaMixerOp_w(_DynaMixerOp):
    """dyna_mlp.py:34-63: lines along w"""
    AXIS = 1

    def __init__(self, w, dim, hidden_dim, segment):
        super().__init__(w, dim, hidden_dim, segment)


class DynaMixerOp_h(_DynaMixerOp):
    """dyna_mlp.py:65-94: lines along h"""
    AXIS = 0

    def __init__(self, h, dim, hidden_dim, segment):
        super().__init__(h, dim, hidden_dim, segment)


class DynaBlock(SubModule):
    """dyna_mlp.py:96-111.  Callable on its own like the reference's: x (b, h, w, C), already normalised -> (b, h, w, C)."""

    def __init__(self, h, w, dim, hidden_dim_DMO=2, segment=8):
        super().__init__()
        self.proj_c = nn.Linear(dim, dim)
        self.proj_o = nn.Linear(dim, dim)
        self.DynaMixerOp_w = DynaMixerOp_w(w, dim, hidden_dim_DMO, segment)
        self.DynaMixerOp_h = DynaMixerOp_h(h, dim, hidden_dim_DMO, segment)
        self.__dict__["_geom"] = (h, w, dim, hidden_dim_DMO, segment)

    def _pack(self, dtype, device):
        pk = {}
        pack_block(pk, "", self, None, dtype, device)
        return pk

    def forward(self, x):
        H, W, C, hd, s = self.__dict__["_geom"]
        pk = self._begin(x, C)
        if x.dim() != 4 or tuple(x.shape[1:3]) != (H, W):
            raise ValueError("expected a channel-last (b, %d, %d, %d) tensor" % (H, W, C))
        require_shape("DynaBlock", x.dtype, H, W, C, s, hd)
        B = x.shape[0]
        rows = B * H * W
        with E.on_device(x):
            ws = self._get_space(B, x.dtype, x.device)
            xb = ws.get("blk.x", (rows, C))
            xb.copy_(x.reshape(rows, C))
            out = ws.get("blk.out", (rows, C))
            block_rows(ws, pk, "", xb, None, B, H, W, C, s, hd, "blk", out, residual=False)
            return out.reshape(B, H, W, C).clone()


class DynaMLPBlock(SubModule):
    """dyna_mlp.py:113-132.  Callable on its own like the reference's: x (b, C, h, w) -> (b, C, h, w)."""

    def __init__(self, depth, h, w, dim, hidden_dim_DMO, segment, mlp_dim, dropout=0.):
        super().__init__()
        self.layers = nn.ModuleList([])
        self.drop_path = DropPath(dropout) if dropout > 0. else nn.Identity()
        self.reshape = Layout("b c h w -> b h w c")
        self.recover = Layout("b h w c -> b c h w")
        for _ in range(depth):
            self.layers.append(nn.ModuleList([
                PreNorm(dim, DynaBlock(h, w, dim, hidden_dim_DMO, segment)),
                PreNorm(dim, FeedForward(dim, mlp_dim, dropout=0.)),
            ]))
        self.__dict__["_geom"] = (depth, h, w, dim, hidden_dim_DMO, segment, mlp_dim)

    def _pack(self, dtype, device):
        pk = {}
        pack_layers(pk, "", self, dtype, device)
        return pk

    def forward(self, x):
        depth, H, W, C, hd, s, hidden = self.__dict__["_geom"]
        pk = self._begin(x, C, axis=1)
        if x.dim() != 4 or tuple(x.shape[2:]) != (H, W):
            raise ValueError("expected a (b, %d, %d, %d) tensor" % (C, H, W))
        require_shape("DynaMLPBlock", x.dtype, H, W, C, s, hd)
        B = x.shape[0]
        rows = B * H * W
        with E.on_device(x):
            ws = self._get_space(B, x.dtype, x.device)
            cur = ws.get("mb.x", (rows, C))
            cur.view(B, H, W, C).copy_(x.permute(0, 2, 3, 1))
            layers_rows(ws, pk, "", depth, cur, B, H, W, C, s, hd, hidden, "mb")
            return cur.view(B, H, W, C).permute(0, 3, 1, 2).clone(memory_format=torch.contiguous_format)


dynamlp_settings = {
    'T': [[7, 2], [192, 384], [4, 14], [8, 16], 3, 0.1, 2],       # [layers]
    'M': [[7, 2], [256, 512], [7, 17], [8, 16], 3, 0.1, 2],
    'L': [[7, 2], [256, 512], [9, 27], [8, 16], 3, 0.3, 8],
}


class DynaMixer(E.EngineModule):
    """dyna_mlp.py:141-182.  Inference-only (no `_train_forward`): in train mode the forward warns and runs as in eval mode."""

    def __init__(self, model_name: str = 'M', image_size=224, in_channels: int = 3, num_classes: int = 1000):
        super().__init__()
        assert model_name in dynamlp_settings.keys(), f"DynaMLP model name should be in {list(dynamlp_settings.keys())}"
        patch_size, embed_dims, depths, segment, mlp_ratio, dropout, hidden_dim_DMO = dynamlp_settings[model_name]

        image_height, image_width = pair(image_size)
        h = []
        w = []
        oldps = [1, 1]
        for ps in patch_size:
            ps = pair(ps)
            if h:
                h.append(int(h[-1] / ps[0]))
                w.append(int(w[-1] / ps[1]))
            else:
                h.append(int(image_height / ps[0]))
                w.append(int(image_width / ps[1]))
            assert (image_height % (ps[0] * oldps[0])) == 0, 'image must be divisible by patch size'
            assert (image_width % (ps[1] * oldps[1])) == 0, 'image must be divisible by patch size'
            oldps[0] = oldps[0] * ps[0]
            oldps[1] = oldps[1] * ps[1]

        self.stage = len(patch_size)
        self.stages = nn.Sequential(
            *[nn.Sequential(
                nn.Conv2d(in_channels if i == 0 else embed_dims[i - 1], embed_dims[i], kernel_size=patch_size[i], stride=patch_size[i]),
                DynaMLPBlock(depth=depths[i], h=h[i], w=w[i], dim=embed_dims[i], hidden_dim_DMO=hidden_dim_DMO, segment=segment[i],
                             mlp_dim=embed_dims[i] * mlp_ratio, dropout=dropout)
            ) for i in range(self.stage)]
        )

        self.mlp_head = nn.Sequential(
            Layout('b c h w -> b c (mean)'),
            nn.Linear(embed_dims[-1], num_classes)
        )
        self.__dict__["_input"] = (in_channels, image_height, image_width)

    # ------------------------------------------------------------------ packing
    def _pack(self, dtype, device):
        pk = {}
        for i, stage in enumerate(self.stages):
            conv = stage[0]
            w = conv.weight.detach()
            if i:
                w = w.permute(0, 2, 3, 1)                                   # (i, j, ci): the channel-last rows' patch order
            pk["s%d.embed.w" % i] = E.pack_matrix(w.reshape(w.shape[0], -1), dtype, device, kpad=E.embed_kpad(dtype))
            pk["s%d.embed.b" % i] = E.f32(conv.bias, device)
            pack_layers(pk, "s%d." % i, stage[1], dtype, device)
        pk["head.w"], pk["head.b"] = E.pack_matrix(self.mlp_head[1].weight, dtype, device), E.f32(self.mlp_head[1].bias, device)
        return pk

    # ------------------------------------------------------------------ forward
    def forward(self, x):
        cd = self._resolve(x)
        if tuple(x.shape[1:]) != self.__dict__["_input"]:
            raise ValueError("expected a (B, %d, %d, %d) tensor, got %s" % (self.__dict__["_input"] + (tuple(x.shape),)))
        B, cin, H, W = x.shape
        for i, stage in enumerate(self.stages):                            # before anything is launched
            _, h, w, C, hd, s, _ = stage[1].__dict__["_geom"]
            require_shape("DynaMixer stage %d" % (i + 1), cd, h, w, C, s, hd)
        pk = self._get_pack(cd, x.device)
        ws = self._get_space(B, cd, x.device)
        cur = x.contiguous()
        for i, stage in enumerate(self.stages):
            depth, h, w, C, hd, s, hidden = stage[1].__dict__["_geom"]
            patch = pair(stage[0].kernel_size)
            name = "s%d.embed" % i
            if i == 0:
                cur, H, W = embed_patches(ws, name, cur, pk[name + ".w"], pk[name + ".b"], cd, patch)
            else:
                cur, H, W = stage_embed(ws, name, cur, B, cin, H, W, pk[name + ".w"], pk[name + ".b"], patch, channel_last=True)
            assert (H, W) == (h, w)
            layers_rows(ws, pk, "s%d." % i, depth, cur, B, H, W, C, s, hd, hidden, "s%d" % i)
            cin = C
        pooled = ws.get("pooled", (B, cin))
        E.pool_mean(cur, B, H * W, cin, cin, pooled, cin)
        return head_linear(ws, pooled, B, cin, pk["head.w"], pk["head.b"], self.mlp_head[1].out_features, x.dtype)
