"""ResMLP, drop-in for the reference's models_pytorch/res_mlp.py.

Block (res_mlp.py:52-57; the residual is taken on the AFFINE'd tensor, unlike the paper):
  x1 = a*x + b;  x2 = x1 + g1 * (Wt . x1 + bt);  x3 = a'*x2 + b';  x <- x3 + g2 * FF(x3)
Kernels: one affine pass writes x1 row-major AND token-transposed; the token GEMM's epilogue applies
bias, the per-channel gamma_1 (a per-ROW scale in the transposed problem) and the residual while
storing through the transpose; a second affine pass; FF as two GEMMs whose second epilogue applies
gamma_2 and the residual.
"""
import contextlib

import torch
from torch import nn

from .. import _native as N
from .. import engine as E
from .common import Block, Holder, SubModule, adopt_blocks, embed_patches, head_linear, two_layer_mlp, train_entry
from .utils.tools import check_sizes, pair


class Aff(SubModule):
    """x * alpha + beta with (1,1,dim) parameters (res_mlp.py:11-19); callable on (..., dim) like the reference's."""

    def __init__(self, dim):
        super().__init__()
        self.alpha = nn.Parameter(torch.ones([1, 1, dim]))
        self.beta = nn.Parameter(torch.zeros([1, 1, dim]))

    def _pack(self, dtype, device):
        return {"a": E.f32(self.alpha.reshape(-1), device), "b": E.f32(self.beta.reshape(-1), device)}

    def forward(self, x):
        dim = self.alpha.shape[-1]
        pk = self._begin(x, dim)
        rows = x.numel() // dim
        with E.on_device(x):
            ws = self._get_space(rows, x.dtype, x.device)
            xb = ws.get("aff.x", (rows, dim))
            xb.copy_(x.reshape(rows, dim))
            y = ws.get("aff.y", (rows, dim))
            E.norm_apply(xb, rows, dim, dim, gamma=pk["a"], beta=pk["b"], out_rm=y, ld_rm=dim)
            return y.reshape(x.shape).clone()


class FeedForward(SubModule):
    """Linear -> GELU -> Dropout -> Linear -> Dropout on the last dimension (res_mlp.py:21-32); callable like the reference's."""

    def __init__(self, dim, hidden_dim, dropout=0.):
        super().__init__()
        self.net = nn.Sequential(nn.Linear(dim, hidden_dim), nn.GELU(), nn.Dropout(dropout),
                                 nn.Linear(hidden_dim, dim), nn.Dropout(dropout))

    def _pack(self, dtype, device):
        return {"fc1.w": E.pack_matrix(self.net[0].weight, dtype, device), "fc1.b": E.f32(self.net[0].bias, device),
                "fc2.w": E.pack_matrix(self.net[3].weight, dtype, device), "fc2.b": E.f32(self.net[3].bias, device)}

    def forward(self, x):
        dim, hidden = self.net[0].in_features, self.net[0].out_features
        pk = self._begin(x, dim)
        rows = x.numel() // dim
        with E.on_device(x):
            ws = self._get_space(rows, x.dtype, x.device)
            xb = ws.get("mlp.x", (rows, pk["fc1.w"].shape[1]))          # K zero-padded to whole 16-byte chunks
            xb[:, :dim].copy_(x.reshape(rows, dim))
            return two_layer_mlp(ws, pk, xb, rows, dim, hidden, dim).reshape(x.shape).clone()


class MLPblock(Block):
    """res_mlp.py:34-57; layer-scale init by depth (:38-43).  Callable on (B, S, C) tokens once it sits in a ResMLP backbone."""

    def __init__(self, num_patch, dim, mlp_dim, dropout=0., depth=18):
        super().__init__()
        if depth <= 18:
            init_values = 0.1
        elif depth <= 24:
            init_values = 1e-5
        else:
            init_values = 1e-6
        self.pre_affine = Aff(dim)
        self.token_mix = nn.Conv1d(num_patch, num_patch, kernel_size=1)
        self.ff = FeedForward(dim, mlp_dim, dropout)
        self.post_affine = Aff(dim)
        self.gamma_1 = nn.Parameter(init_values * torch.ones((dim)), requires_grad=True)
        self.gamma_2 = nn.Parameter(init_values * torch.ones((dim)), requires_grad=True)


class ResMLP(E.EngineModule):
    def __init__(self, num_patch, d_model, depth, expansion_factor):
        super().__init__()
        self.model = nn.Sequential(*[MLPblock(num_patch, d_model, d_model * expansion_factor, depth=depth)
                                     for _ in range(depth)])
        self._dims = (num_patch, d_model, depth, expansion_factor)
        adopt_blocks(self, self.model)

    def _pack_blocks(self, pk, dtype, device):
        for i, blk in enumerate(self.model):
            p = "b%d." % i
            pk[p + "pre.a"], pk[p + "pre.b"] = E.f32(blk.pre_affine.alpha, device), E.f32(blk.pre_affine.beta, device)
            pk[p + "post.a"], pk[p + "post.b"] = E.f32(blk.post_affine.alpha, device), E.f32(blk.post_affine.beta, device)
            pk[p + "g1"], pk[p + "g2"] = E.f32(blk.gamma_1, device), E.f32(blk.gamma_2, device)
            pk[p + "tok.w"] = E.pack_matrix(blk.token_mix.weight, dtype, device, kpad=32)            # (S, S_pad)
            pk[p + "tok.b"] = E.f32(blk.token_mix.bias, device)
            S = blk.token_mix.weight.shape[0]
            if E.token_gemm_supported(dtype, S, E.round_up(S, 32)):
                pk[p + "tok.tg"] = E.pack_token_gemm(blk.token_mix.weight, blk.token_mix.bias, dtype, device)
            pk[p + "fc1.w"] = E.pack_matrix(blk.ff.net[0].weight, dtype, device)
            pk[p + "fc1.b"] = E.f32(blk.ff.net[0].bias, device)
            pk[p + "fc2.w"] = E.pack_matrix(blk.ff.net[3].weight, dtype, device)
            pk[p + "fc2.b"] = E.f32(blk.ff.net[3].bias, device)
            if dtype != torch.float32:
                # round 4: the layer scale gamma_2 (res_mlp.py:49,57) folded into fc2 -- W' = diag(gamma_2) F2, b' = gamma_2 f2 -- so the
                # product is the plain bias + residual class the generated q4 tile runs (with a per-column scale it fell to the 128 x 128
                # s3 tile: 34 % of ResMLP-24 at 650 TFLOP/s); one rounding of the scaled weights instead of a scale of the rounded ones
                g2 = blk.gamma_2.detach().to(device=device, dtype=torch.float32).reshape(-1, 1)
                w2 = blk.ff.net[3].weight.detach().to(device=device, dtype=torch.float32)
                pk[p + "fc2.wg"] = E.pack_matrix(w2 * g2, dtype, device)
                pk[p + "fc2.bg"] = (blk.ff.net[3].bias.detach().to(device=device, dtype=torch.float32) * g2.reshape(-1)).contiguous()

    def _pack(self, dtype, device):
        pk = {}
        self._pack_blocks(pk, dtype, device)
        return pk

    def _run_blocks(self, ws, pk, x, B, only=None):
        S, C, depth, ef = self._dims
        rows = B * S
        sp = E.round_up(S, 32)        # token K padding: whole half-slabs -> direct-to-LDS GEMM tiles
        hidden = C * ef
        for i in (range(depth) if only is None else only):
            p = "b%d." % i
            tg = pk.get(p + "tok.tg")
            if tg is not None and E.token_gemm_ln_supported(x.dtype, S, C, C):
                # round 4: Aff (res_mlp.py:17-19,53) is the cross-patch product's operand loader AND its residual -- the kernel reads x,
                # builds x1 = alpha x + beta for its operand (transposed through LDS) and for the residual items, and writes
                # x2 = x1 + gamma_1 (Wt x1 + bt) over x: no Aff pass, no x1 tensor, no token-transposed copy
                # round 5: ... and the Aff that FOLLOWS (post_affine, res_mlp.py:56) is applied where x2 is stored: x3 = alpha' x2 + beta' leaves
                # the kernel instead of x2 (the same two roundings as the separate pass)
                post = E.token_gemm_ln_post_supported(x.dtype, S, C, C)
                E.token_gemm_ln(x, C, B * C, S, None, None, pk[p + "pre.a"], pk[p + "pre.b"], tg[0], tg[1], tg[2], x, C, C,
                                R=x, ldr=C, res=N.RES_ADD_AFFINE, rscale=pk[p + "g1"], rperiod=C,
                                post=(pk[p + "post.a"], pk[p + "post.b"]) if post else None)
                if not post:
                    E.norm_apply(x, rows, C, C, gamma=pk[p + "post.a"], beta=pk[p + "post.b"], out_rm=x, ld_rm=C)
                h = ws.get("h", (rows, hidden))
                E.gemm(x, pk[p + "fc1.w"], h, rows, hidden, C, bias=pk[p + "fc1.b"], act=N.ACT_GELU)
                self._fc2(pk, p, h, x, rows, C, hidden)
                continue
            xt = ws.get("xt", (B * C, sp))
            # x1 = alpha*x + beta, in place, plus its token-transposed copy for the token GEMM
            E.norm_apply(x, rows, C, C, gamma=pk[p + "pre.a"], beta=pk[p + "pre.b"], out_rm=x, ld_rm=C, out_tt=xt, S=S, ld_tt=sp)
            # x2 = x1 + gamma_1[c] * (sum_s Wt[t,s] x1[b,s,c] + bt[t])
            tg = pk.get(p + "tok.tg")
            if tg is not None:
                E.token_gemm(xt, sp, B * C, S, tg[0], tg[1], tg[2], x, C, C, R=x, ldr=C, res=N.RES_ADD, rscale=pk[p + "g1"], rperiod=C)
            else:
                E.gemm(xt, pk[p + "tok.w"], x, B * C, S, sp, ldc=C, bias=pk[p + "tok.b"], rscale=pk[p + "g1"], rperiod=C,
                       R=x, ldr=C, res=N.RES_ADD, out_mode=N.OUT_TOKEN_T, t_rows=C, t_tokens=S)
            # x3 = alpha'*x2 + beta'
            E.norm_apply(x, rows, C, C, gamma=pk[p + "post.a"], beta=pk[p + "post.b"], out_rm=x, ld_rm=C)
            h = ws.get("h", (rows, hidden))
            E.gemm(x, pk[p + "fc1.w"], h, rows, hidden, C, bias=pk[p + "fc1.b"], act=N.ACT_GELU)
            # x = x3 + gamma_2 * (h F2^T + f2)
            self._fc2(pk, p, h, x, rows, C, hidden)
        return x

    @staticmethod
    def _fc2(pk, p, h, x, rows, C, hidden):
        """x <- x3 + gamma_2 (h F2^T + f2)   (res_mlp.py:57)"""
        if (p + "fc2.wg") in pk:
            E.gemm(h, pk[p + "fc2.wg"], x, rows, C, hidden, bias=pk[p + "fc2.bg"], R=x, res=N.RES_ADD)
        else:
            E.gemm(h, pk[p + "fc2.w"], x, rows, C, hidden, bias=pk[p + "fc2.b"], cscale=pk[p + "g2"], R=x, res=N.RES_ADD)

    def forward(self, x, _only=None):
        E.require_gpu(x, "ResMLP.forward")
        S, C, _, _ = self._dims
        if x.dim() != 3 or x.shape[1] != S or x.shape[2] != C:
            raise ValueError("expected tokens of shape (B, %d, %d)" % (S, C))
        B = x.shape[0]
        pk = self._get_pack(x.dtype, x.device)
        ws = self._get_space(B, x.dtype, x.device)
        buf = ws.get("x", (B * S, C))
        buf.copy_(x.reshape(B * S, C))
        self._run_blocks(ws, pk, buf, B, only=_only)
        return buf.reshape(B, S, C).clone()

    def _run_single(self, i, x):
        """block i alone, (B, S, C) -> (B, S, C): what `model.model[i](x)` computes in the reference (res_mlp.py:50-57)"""
        with E.on_device(x) if x.is_cuda else contextlib.nullcontext():
            return ResMLP.forward(self, x, _only=[i])       # (the image-classification subclass overrides forward)


class ResMLPForImageClassification(ResMLP):
    """Same signature and defaults as the reference (res_mlp.py:69-78).  `affine` exists in the
    state_dict but takes no part in forward (res_mlp.py:86, 91-99)."""

    def __init__(self, in_channels=3, d_model=384, num_classes=1000, patch_size=16, image_size=224, depth=12,
                 expansion_factor=4):
        num_patches = check_sizes(image_size, patch_size)
        super().__init__(num_patches, d_model, depth, expansion_factor)
        self.patcher = nn.Sequential(nn.Conv2d(in_channels, d_model, kernel_size=patch_size, stride=patch_size))
        self.affine = Aff(d_model)
        self.mlp_head = nn.Sequential(nn.Linear(d_model, num_classes))
        self._patch = pair(patch_size)
        self._num_classes = num_classes

    def _pack(self, dtype, device):
        pk = {}
        self._pack_blocks(pk, dtype, device)
        pk["embed.w"] = E.pack_matrix(self.patcher[0].weight, dtype, device)
        pk["embed.b"] = E.f32(self.patcher[0].bias, device)
        pk["head.w"] = E.pack_matrix(self.mlp_head[0].weight, dtype, device)
        pk["head.b"] = E.f32(self.mlp_head[0].bias, device)
        return pk

    _train_forward = True

    def _forward_train(self, x):
        """Train mode with autograd (round 6): res_mlp.py:11-57,88-99 as autograd.Functions of `..autograd`, forward and backward
        through the C ABI -- Aff and the layer scales gamma_1 / gamma_2 = mlpk_ew_cols (parameter gradients: mlpk_col_dot / mlpk_col_sum), the
        cross-patch Conv1d(k=1) and the FeedForward = mlpk_gemm_nt (+ the two GEMMs of their backward) between mlpk_transpose_batched rearranges.
        The model-level `affine` takes no part in forward (res_mlp.py:86,91-99): its parameters get no gradient, as in the reference."""
        from .. import autograd as AG
        cd = train_entry(self, x, warn_dropout=True)
        S, C, _, _ = self._dims
        B, _, H, W = x.shape
        ph, pw = self._patch
        if (H // ph) * (W // pw) != S:
            raise ValueError("input size gives %d patches, the model was built for %d" % ((H // ph) * (W // pw), S))
        t, _, _ = AG.conv_rows(x, self.patcher[0], cd)
        for blk in self.model:
            x1 = AG.Affine.apply(t, blk.pre_affine.alpha, blk.pre_affine.beta)
            z = AG.RowsToTokens.apply(AG.linear(AG.TokensToRows.apply(x1, B, S), blk.token_mix), B, S, C)
            x3 = AG.Affine.apply(AG.ScaleAdd.apply(x1, z, blk.gamma_1), blk.post_affine.alpha, blk.post_affine.beta)
            t = AG.ScaleAdd.apply(x3, AG.mlp(x3, blk.ff.net[0], blk.ff.net[3]), blk.gamma_2)
        logits = AG.linear(AG.TokenMean.apply(t, B, S), self.mlp_head[0])
        return logits.to(x.dtype)

    def forward(self, x):
        if self._train_path():
            return self._forward_train(x)
        cd = self._resolve(x)
        S, C, _, _ = self._dims
        B = x.shape[0]
        pk = self._get_pack(cd, x.device)
        ws = self._get_space(B, cd, x.device)
        x = x.contiguous()
        tokens, hp, wp = embed_patches(ws, "embed", x, pk["embed.w"], pk["embed.b"], cd, self._patch,
                                       out=ws.get("x", (B * S, C)))
        if hp * wp != S:
            raise ValueError("input size gives %d patches, the model was built for %d" % (hp * wp, S))
        self._run_blocks(ws, pk, tokens, B)
        pooled = ws.get("pooled", (B, C))
        E.pool_mean(tokens, B, S, C, C, pooled, C)
        return head_linear(ws, pooled, B, C, pk["head.w"], pk["head.b"], self._num_classes, x.dtype)
