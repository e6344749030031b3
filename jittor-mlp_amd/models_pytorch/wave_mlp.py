"""WaveMLP, drop-in for the reference's models_pytorch/wave_mlp.py: same classes, constructor signatures, `wavemlp_settings`, state_dict keys and
shapes, `pretrained` loading.  Inference-only: train() takes the engine's warning path (BatchNorm on batch statistics and a backward are not built).

Every BatchNorm is folded at pack time (fp32) into the convolution next to it; the forward runs on channel-last rows (B*H*W, C):
  patch_embed   Conv 7x7 / 4 pad 2 + BN            mlpk_stem7 (16-bit) or window gather + GEMM
  Block (:70-83), x += PATM(BN1(x)); x += MLP(BN2(x)):
    y = x W^T + b                                  ONE GEMM, N = 5C: theta_h, theta_w (their BN folded in), fc_h, fc_w, fc_c; BN1 folded into all five
    h, w = mlpk_wave_patm(y)                       ReLU, x cos / x sin and the grouped 7-tap convolutions tfc_h / tfc_w in one pass
    a = mean over pixels of (h + w + c)            mlpk_split_sum, scale 1 / (H W)
    reweight: fc1 -> GELU -> fc2 (fp32, B rows; fc2's rows permuted from c*3 + k to k*C + c as CycleMLP packs them), softmax over the 3 branches
    x += proj(h a0 + w a1 + c a2)                  mlpk_split_apply, GEMM with the residual in its epilogue
    x += fc2(gelu(fc1(x)))                         BN2 folded into fc1: mlpk_channel_mlp where it takes the width, else two GEMMs
  Downsample    Conv 3x3 / 2 pad 1 + BN            mlpk_conv_gemm_nhwc (or window gather + GEMM)
  norm + head   BN commutes with the mean          mlpk_pool_mean with the BN affine on the pooled rows, then the head GEMM
`Block` and `PATM` run on their own on the reference's NCHW layout (their own packed weights, the same kernels); `MLP`, `PatchEmbedOverlap` and
`Downsample` are parameter containers.
"""
import torch
from torch import nn

from .. import _native as N
from .. import engine as E
from .common import Holder, SubModule, channel_mlp, head_linear

wavemlp_settings = {
    'T': [[2, 2, 4, 2], [4, 4, 4, 4]],      # layers per stage, MLP ratios per stage
    'S': [[2, 3, 10, 3], [4, 4, 4, 4]],
    'M': [[3, 4, 18, 3], [8, 8, 4, 4]],
}


class _Held(Holder):
    def forward(self, *a, **k):
        raise NotImplementedError("%s only holds parameters inside WaveMLP: call the enclosing WaveMLP, its Block or its PATM" % type(self).__name__)


class MLP(_Held):
    """wave_mlp.py:10-19: 1x1 conv -> GELU -> 1x1 conv."""

    def __init__(self, dim, hidden_dim, out_dim=None) -> None:
        super().__init__()
        out_dim = out_dim or dim
        self.fc1 = nn.Conv2d(dim, hidden_dim, 1)
        self.act = nn.GELU()
        self.fc2 = nn.Conv2d(hidden_dim, out_dim, 1)


class PatchEmbedOverlap(_Held):
    """wave_mlp.py:85-95: Conv(patch_size, stride, padding) + BatchNorm."""

    def __init__(self, patch_size=16, stride=16, padding=0, embed_dim=768):
        super().__init__()
        self.proj = nn.Conv2d(3, embed_dim, patch_size, stride, padding)
        self.norm = nn.BatchNorm2d(embed_dim)


class Downsample(_Held):
    """wave_mlp.py:97-106: Conv 3x3 / 2 pad 1 + BatchNorm."""

    def __init__(self, c1, c2):
        super().__init__()
        self.proj = nn.Conv2d(c1, c2, 3, 2, 1)
        self.norm = nn.BatchNorm2d(c2)


# ------------------------------------------------------------------ packing (fp32 folding, then the compute dtype)
def bn_affine(bn, device):
    """eval-mode BatchNorm as y = s x + t (fp32)"""
    s = bn.weight.detach().to(device, torch.float32) / torch.sqrt(bn.running_var.detach().to(device, torch.float32) + bn.eps)
    t = bn.bias.detach().to(device, torch.float32) - bn.running_mean.detach().to(device, torch.float32) * s
    return s, t


def fold_conv(conv, device, pre=None, post=None):
    """conv's weight as an (out, in * kh * kw) fp32 matrix in (ci, i, j) order and its bias, with the per-input-channel affine `pre` = (s, t) in
    front of it (a 1 x 1 convolution only: padding would see t where the reference sees zeros) and the per-output-channel affine `post` after it"""
    w = conv.weight.detach().to(device, torch.float32)
    co = w.shape[0]
    b = conv.bias.detach().to(device, torch.float32) if conv.bias is not None else torch.zeros(co, dtype=torch.float32, device=device)
    w = w.reshape(co, -1)
    if pre is not None:
        b = b + w @ pre[1]
        w = w * pre[0].view(1, -1)
    if post is not None:
        w = w * post[0].view(-1, 1)
        b = b * post[0] + post[1]
    return w, b


def pack_patm(pk, p, att, dtype, device, pre=None):
    """PATM's weights under prefix p; `pre` = the affine of the BatchNorm in front of it (Block.norm1), folded into the five 1 x 1 convolutions"""
    C = att.proj.weight.shape[0]
    ws, bs = [], []
    for conv, bn in ((att.theta_h_conv[0], att.theta_h_conv[1]), (att.theta_w_conv[0], att.theta_w_conv[1]), (att.fc_h, None), (att.fc_w, None),
                     (att.fc_c, None)):
        w, b = fold_conv(conv, device, pre=pre, post=bn_affine(bn, device) if bn is not None else None)
        ws.append(w)
        bs.append(b)
    pk[p + "y.w"] = E.pack_matrix(torch.cat(ws), dtype, device)              # rows [theta_h | theta_w | x_h | x_w | c]
    pk[p + "y.b"] = torch.cat(bs).contiguous()
    pk[p + "th"] = E.f32(att.tfc_h.weight, device)                           # (C, 2, 1, 7) -> (C, 2, 7)
    pk[p + "tw"] = E.f32(att.tfc_w.weight, device)                           # (C, 2, 7, 1) -> (C, 2, 7)
    r1, r2 = att.reweight.fc1, att.reweight.fc2
    pk[p + "r1.w"] = E.pack_matrix(r1.weight, torch.float32, device)
    pk[p + "r1.b"] = E.f32(r1.bias, device)
    w2 = r2.weight.detach().reshape(3 * C, -1)                               # rows c*3 + k -> k*C + c
    pk[p + "r2.w"] = E.pack_matrix(w2.reshape(C, 3, -1).permute(1, 0, 2).reshape(3 * C, -1), torch.float32, device)
    pk[p + "r2.b"] = E.f32(r2.bias.detach().reshape(C, 3).t().reshape(-1), device)
    pk[p + "p.w"] = E.pack_matrix(att.proj.weight, dtype, device)
    pk[p + "p.b"] = E.f32(att.proj.bias, device)


def pack_block(pk, p, blk, dtype, device):
    pack_patm(pk, p, blk.attn, dtype, device, pre=bn_affine(blk.norm1, device))
    w1, b1 = fold_conv(blk.mlp.fc1, device, pre=bn_affine(blk.norm2, device))
    pk[p + "ff.fc1.w"], pk[p + "ff.fc1.b"] = E.pack_matrix(w1, dtype, device), b1.contiguous()
    pk[p + "ff.fc2.w"], pk[p + "ff.fc2.b"] = E.pack_matrix(blk.mlp.fc2.weight, dtype, device), E.f32(blk.mlp.fc2.bias, device)
    C, hidden = w1.shape[1], w1.shape[0]
    if E.channel_mlp_fused_supported(dtype, C, hidden) and blk.mlp.fc2.weight.shape[0] == C:
        pk[p + "ff.fused"] = E.pack_channel_mlp_fused(w1, b1, blk.mlp.fc2.weight, blk.mlp.fc2.bias, dtype, device)


# ------------------------------------------------------------------ forward pieces on channel-last rows
def patm_rows(ws, pk, p, src, dst, B, H, W, C, tag, residual):
    """dst = PATM(src) (+ dst when residual) on rows (B*H*W, C); the packed weights may carry the BatchNorm in front of PATM"""
    rows = B * H * W
    y = ws.get(tag + ".y", (rows, 5 * C))
    E.gemm(src, pk[p + "y.w"], y, rows, 5 * C, C, bias=pk[p + "y.b"], tag="wave_y")
    hw = ws.get(tag + ".hw", (rows, 2 * C))
    h, w, c = hw[:, :C], hw[:, C:], y[:, 4 * C:]
    E.wave_patm(y, pk[p + "th"], pk[p + "tw"], h, w, B, H, W, C)
    a = ws.get(tag + ".a", (B, C), torch.float32)
    E.split_sum(h, w, c, 2 * C, 2 * C, 5 * C, B, H, W, C, N.SHIFT_NONE, a, scale=1.0 / (H * W))
    hid = pk[p + "r1.w"].shape[0]
    hp = pk[p + "r2.w"].shape[1]                                   # hidden padded to whole 16-byte chunks (zero columns)
    t = ws.get(tag + ".t", (B, hp), torch.float32)
    E.gemm(a, pk[p + "r1.w"], t, B, hid, C, ldc=hp, bias=pk[p + "r1.b"], act=N.ACT_GELU)
    hat = ws.get(tag + ".hat", (B, 3 * C), torch.float32)
    E.gemm(t, pk[p + "r2.w"], hat, B, 3 * C, hp, bias=pk[p + "r2.b"])
    bar = ws.get(tag + ".bar", (B, 3 * C), torch.float32)
    E.split_softmax(hat, bar, B, C)
    m = ws.get(tag + ".m", (rows, C))
    E.split_apply(h, w, c, 2 * C, 2 * C, 5 * C, B, H, W, C, N.SHIFT_NONE, bar, m, C)
    if residual:
        E.gemm(m, pk[p + "p.w"], dst, rows, C, C, bias=pk[p + "p.b"], R=dst, res=N.RES_ADD, tag="wave_proj")
    else:
        E.gemm(m, pk[p + "p.w"], dst, rows, C, C, bias=pk[p + "p.b"], tag="wave_proj")


def block_rows(ws, pk, p, cur, B, H, W, C, hidden, tag):
    """one Block in place on rows (B*H*W, C)"""
    rows = B * H * W
    patm_rows(ws, pk, p, cur, cur, B, H, W, C, tag, residual=True)
    if (p + "ff.fused") in pk and E.channel_mlp_fused_supported(cur.dtype, C, hidden):
        E.channel_mlp_fused(cur, rows, C, pk[p + "ff.fused"], cur, R=cur)       # BN2 sits in the weights: no row statistics
    else:
        channel_mlp(ws, cur, rows, C, pk, p + "ff.", hidden, norm=False, tag=tag + ".cm")


def _nchw_rows(ws, x, name):
    B, C, H, W = x.shape
    rows = ws.get(name, (B * H * W, C))
    rows.view(B, H, W, C).copy_(x.permute(0, 2, 3, 1))
    return rows


def _rows_nchw(rows, B, H, W, C):
    out = torch.empty((B, C, H, W), dtype=rows.dtype, device=rows.device)
    E.rows_to_nchw(rows, B, H * W, C, out)
    return out


class PATM(SubModule):
    """wave_mlp.py:22-67.  Callable on its own on (B, C, H, W) like the reference's; inside a WaveMLP the model packs these weights into its own
    fused sequence (with the Block's norm1 folded in)."""

    def __init__(self, dim):
        super().__init__()
        self.fc_h = nn.Conv2d(dim, dim, 1)
        self.fc_w = nn.Conv2d(dim, dim, 1)
        self.fc_c = nn.Conv2d(dim, dim, 1)
        self.tfc_h = nn.Conv2d(2 * dim, dim, (1, 7), 1, (0, 7 // 2), groups=dim, bias=False)
        self.tfc_w = nn.Conv2d(2 * dim, dim, (7, 1), 1, (7 // 2, 0), groups=dim, bias=False)
        self.reweight = MLP(dim, dim // 4, dim * 3)
        self.proj = nn.Conv2d(dim, dim, 1)
        self.theta_h_conv = nn.Sequential(nn.Conv2d(dim, dim, 1), nn.BatchNorm2d(dim), nn.ReLU())
        self.theta_w_conv = nn.Sequential(nn.Conv2d(dim, dim, 1), nn.BatchNorm2d(dim), nn.ReLU())

    def _pack(self, dtype, device):
        pk = {}
        pack_patm(pk, "", self, dtype, device)
        return pk

    def forward(self, x):
        C = self.proj.weight.shape[0]
        pk = self._begin(x, C, axis=1)
        if x.dim() != 4:
            raise ValueError("expected a (B, %d, H, W) tensor" % C)
        B, _, H, W = x.shape
        with E.on_device(x):
            ws = self._get_space((B, H, W), x.dtype, x.device)
            src = _nchw_rows(ws, x, "patm.x")
            dst = ws.get("patm.out", (B * H * W, C))
            patm_rows(ws, pk, "", src, dst, B, H, W, C, "patm", residual=False)
            return _rows_nchw(dst, B, H, W, C)


class Block(SubModule):
    """wave_mlp.py:70-83: x + PATM(BN1(x)), then x + MLP(BN2(x)) (drop path rate `dpr`: identity at inference).  Callable on its own on
    (B, C, H, W) like the reference's."""

    def __init__(self, dim, mlp_ratio=4, dpr=0.):
        super().__init__()
        self.norm1 = nn.BatchNorm2d(dim)
        self.attn = PATM(dim)
        self.drop_path = nn.Identity()
        self.drop_path_rate = dpr
        self.norm2 = nn.BatchNorm2d(dim)
        self.mlp = MLP(dim, int(dim * mlp_ratio))

    def _pack(self, dtype, device):
        pk = {}
        pack_block(pk, "", self, dtype, device)
        return pk

    def forward(self, x):
        C = self.norm1.num_features
        pk = self._begin(x, C, axis=1)
        if x.dim() != 4:
            raise ValueError("expected a (B, %d, H, W) tensor" % C)
        B, _, H, W = x.shape
        with E.on_device(x):
            ws = self._get_space((B, H, W), x.dtype, x.device)
            cur = _nchw_rows(ws, x, "blk.x")
            block_rows(ws, pk, "", cur, B, H, W, C, self.mlp.fc1.out_channels, "blk")
            return _rows_nchw(cur, B, H, W, C)


class WaveMLP(E.EngineModule):
    """wave_mlp.py:115-186.  Inference-only (no `_train_forward`): in train mode the forward warns and runs as in eval mode."""

    def __init__(self, model_name: str = 'T', pretrained: str = None, num_classes: int = 1000, *args, **kwargs) -> None:
        super().__init__()
        assert model_name in wavemlp_settings.keys(), f"WaveMLP model name should be in {list(wavemlp_settings.keys())}"
        layers, mlp_ratios = wavemlp_settings[model_name]
        embed_dims = [64, 128, 320, 512]
        self.patch_embed = PatchEmbedOverlap(7, 4, 2, embed_dims[0])
        network = []
        for i, (depth, ratio) in enumerate(zip(layers, mlp_ratios)):
            network.append(nn.Sequential(*[Block(embed_dims[i], ratio) for _ in range(depth)]))
            if i + 1 < len(layers):
                network.append(Downsample(embed_dims[i], embed_dims[i + 1]))
        self.network = nn.ModuleList(network)
        self.norm = nn.BatchNorm2d(embed_dims[-1])
        self.head = nn.Linear(embed_dims[-1], num_classes)
        self.out_indices = [0, 2, 4, 6]
        self._init_weights(pretrained)

    def _init_weights(self, pretrained: str = None) -> None:
        """wave_mlp.py:146-165: a checkpoint's 'model' entry, or xavier-uniform weights and zero biases on every Conv2d / Linear except the head,
        which starts at zero."""
        if pretrained:
            self.load_state_dict(torch.load(pretrained, map_location='cpu')['model'])
            return
        for name, m in self.named_modules():
            if isinstance(m, (nn.Linear, nn.Conv2d)):
                if name.startswith('head'):
                    nn.init.zeros_(m.weight)
                    nn.init.zeros_(m.bias)
                    continue
                nn.init.xavier_uniform_(m.weight)
                if m.bias is not None:
                    nn.init.zeros_(m.bias)
            elif isinstance(m, nn.LayerNorm):
                nn.init.ones_(m.weight)
                nn.init.zeros_(m.bias)

    def return_features(self, x):
        """wave_mlp.py:167-176 reads `self.norm{i}`, which the reference never creates: AttributeError, as there."""
        for i in self.out_indices:
            getattr(self, "norm%d" % i)
        raise AssertionError("unreachable")

    # ------------------------------------------------------------------ packing
    def _pack(self, dtype, device):
        pk = {}
        pe = self.patch_embed
        w, b = fold_conv(pe.proj, device, post=bn_affine(pe.norm, device))      # (C, 3 * 7 * 7), (ci, i, j) order
        pk["embed.w"] = E.pack_matrix(w, dtype, device)
        if dtype != torch.float32:
            pk["embed.w7"] = E.pack_stem7(w.reshape(pe.proj.weight.shape), dtype, device)
        pk["embed.b"] = b.contiguous()
        for si, stage in enumerate(self.network):
            if isinstance(stage, Downsample):
                w, b = fold_conv(stage.proj, device, post=bn_affine(stage.norm, device))
                co, ci = stage.proj.weight.shape[:2]
                pk["n%d.w" % si] = E.pack_matrix(w.reshape(co, ci, 3, 3).permute(0, 2, 3, 1).reshape(co, -1), dtype, device)   # (i, j, ci)
                pk["n%d.b" % si] = b.contiguous()
                continue
            for bi, blk in enumerate(stage):
                pack_block(pk, "n%d.b%d." % (si, bi), blk, dtype, device)
        pk["head.s"], pk["head.t"] = bn_affine(self.norm, device)
        pk["head.w"] = E.pack_matrix(self.head.weight, dtype, device)
        pk["head.b"] = E.f32(self.head.bias, device)
        return pk

    # ------------------------------------------------------------------ forward
    def forward(self, x):
        cd = self._resolve(x)
        B, cin, H_in, W_in = x.shape
        if cin != 3:
            raise ValueError("expected a (B, 3, H, W) tensor")
        pk = self._get_pack(cd, x.device)
        ws = self._get_space(B, cd, x.device)
        x = x.contiguous()
        C = pk["embed.w"].shape[0]
        H, W = (H_in + 4 - 7) // 4 + 1, (W_in + 4 - 7) // 4 + 1
        cur = ws.get("n0.x", (B * H * W, C))
        if "embed.w7" in pk and x.data_ptr() % 16 == 0 and E.stem7_supported(x.dtype, cd, cin, H_in, W_in, 2, C):
            E.stem7(x, pk["embed.w7"], pk["embed.b"], cur, B, H_in, W_in, 2, C)
        else:
            kp = pk["embed.w"].shape[1]
            patches = ws.get("embed.patches", (B * H * W, kp))
            E.im2col(x, patches, B, cin, H_in, W_in, 7, 7, 4, 4, 2, kp)
            E.gemm(patches, pk["embed.w"], cur, B * H * W, C, kp, bias=pk["embed.b"])
        for si, stage in enumerate(self.network):
            if isinstance(stage, Downsample):
                Cout = pk["n%d.w" % si].shape[0]
                H2, W2 = (H + 2 - 3) // 2 + 1, (W + 2 - 3) // 2 + 1
                kp = pk["n%d.w" % si].shape[1]
                nxt = ws.get("n%d.x" % (si + 1), (B * H2 * W2, Cout))
                if kp == 9 * C and E.conv_gemm_nhwc_supported(cur.dtype, C, 3, 3, 2, 1):
                    E.conv_gemm_nhwc(cur, pk["n%d.w" % si], nxt, B, H, W, C, 3, 3, 2, 1, bias=pk["n%d.b" % si], tag="wave_down")
                else:
                    cols = ws.get("n%d.cols" % si, (B * H2 * W2, kp))
                    E.im2col(cur, cols, B, C, H, W, 3, 3, 2, 2, 1, kp, layout=N.LAYOUT_NHWC, px_stride=C)
                    E.gemm(cols, pk["n%d.w" % si], nxt, B * H2 * W2, Cout, kp, bias=pk["n%d.b" % si], tag="wave_down")
                cur, H, W, C = nxt, H2, W2, Cout
                continue
            for bi, blk in enumerate(stage):
                block_rows(ws, pk, "n%d.b%d." % (si, bi), cur, B, H, W, C, blk.mlp.fc1.out_channels, "n%d" % si)
        pooled = ws.get("pooled", (B, C))
        E.pool_mean(cur, B, H * W, C, C, pooled, C, gamma=pk["head.s"], beta=pk["head.t"])     # norm (an affine) commutes with the mean
        return head_linear(ws, pooled, B, C, pk["head.w"], pk["head.b"], self.head.out_features, x.dtype)
