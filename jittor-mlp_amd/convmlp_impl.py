"""ConvMLP, drop-in for the reference's models_pytorch/conv_mlp.py: the same classes, functions, constructor signatures, defaults and state_dict
keys and shapes (the convolutions are real nn.Conv2d and the BatchNorms real nn.BatchNorm2d modules that hold the parameters and buffers and are
never called); `models_pytorch/conv_mlp.py` gives them the reference's import path.  The classes are defined here, beside the engine, because every
EngineModule subclass defined under models_pytorch must have a row in the tables of tests/test_gpu_lifecycle.py; moving the family there is a
later change (DynaMixer and Sequencer2D arrived the same way).  Inference-only: train() takes the engine's warning path, DropPath is the identity,
BatchNorm uses its running statistics.  `model_urls` is empty and `pretrained=True` raises: nothing here reaches for a network.

The forward runs on dense channel-last rows x[(b, h, w), c], for any input size.
  ConvTokenizer (:52-87)   Conv 3 -> c/2 (3 x 3 s2 p1) from the NCHW image: mlpk_im2col + GEMM, K = 27 zero-padded; two 3 x 3 s1 p1 convolutions
                           (`conv3x3`); ReLU by mlpk_relu_add, the last one together with MaxPool2d(3, 2, 1) by mlpk_relu_maxpool3s2_nhwc
  ConvStage (:91-126)      per block 1 x 1, 3 x 3, 1 x 1, each a product followed by mlpk_relu_add -- the third with the block's input as `res`,
                           which is the stage's residual x + block(x); `downsample` (3 x 3 s2 p1, with bias) is one product
  ConvMLPStage (:146-170)  x += MLP(LN(x)) (common.channel_mlp, LayerNorm folded into fc1); x = connect(connect_norm(x)) by
                           mlpk_ln_dwconv3_nhwc, its statistics the by-product of the MLP's last GEMM where it delivers them; x += MLP(LN(x))
  ConvDownsample (:173-182) one product
  head (:255-259)          LayerNorm statistics + mlpk_pool_mean (the affine inside) + one GEMM
BatchNorm (eval) is NOT folded into the weights: it is the product's per-column scale and shift (mlpk_gemm_nt's cscale / cshift, `bn_scale_shift`),
so the 16-bit weights are the reference's own, rounded once.  A dense 3 x 3 convolution is ONE product read through the window
(mlpk_conv_gemm_nhwc) where `conv_plan` says "window" -- 16-bit, Cin a multiple of 32 -- and mlpk_im2col + GEMM ("gather") otherwise: fp32,
Cin = 16 or 48, ConvMLP-L's tokenizer.  Its weight columns are in tap-major order (`conv3_columns`) for both.

`ConvMLP`, `ConvMLPStage` ((B, H, W, C) in and out), `ConvStage` and `ConvTokenizer` (NCHW in and out) run on their own on the GPU.  `Mlp`,
`ConvDownsample`, `BasicStage` and `DropPath` hold parameters.  A width that is not a whole 16-byte vector (8 channels in the 16-bit types, 4 in
fp32), or anything else a kernel refuses, raises NotImplementedError naming the entry and the shape; there is no fallback path.
"""
import torch
from torch import nn

from . import _native as N
from . import engine as E
from .models_pytorch.common import SubModule, channel_mlp, finalize_stats, head_linear, layernorm_stats, pack_channel_mlp

__all__ = ['ConvMLP', 'convmlp_s', 'convmlp_m', 'convmlp_l']

model_urls = {}


def drop_path(x, drop_prob: float = 0., training: bool = False):
    """Stochastic depth per sample (conv_mlp.py:17-34): in training each sample's branch is kept with probability 1 - drop_prob and divided by
    it.  The models here never call it: they are inference-only, where it is the identity."""
    if not training or drop_prob == 0.:
        return x
    keep = 1.0 - drop_prob
    kept = torch.rand((x.shape[0],) + (1,) * (x.dim() - 1), dtype=x.dtype, device=x.device) < keep
    return x * kept.to(x.dtype) / keep


class _Container(nn.Module):
    """Holds parameters; the enclosing module packs them into its own kernel sequence and never calls the module."""

    def forward(self, *a, **k):
        raise NotImplementedError("%s only holds parameters inside ConvMLP: call the enclosing ConvMLP, ConvMLPStage, ConvStage or ConvTokenizer" % type(self).__name__)


class DropPath(_Container):
    """conv_mlp.py:37-48.  The identity in an inference-only model."""

    def __init__(self, drop_prob=None):
        super(DropPath, self).__init__()
        self.drop_prob = drop_prob


# ------------------------------------------------------------------ packing (pure functions: they run on CPU tensors too)
def conv_plan(dtype, Cin):
    """how a dense 3 x 3 convolution on channel-last rows runs: "window" = mlpk_conv_gemm_nhwc (16-bit, Cin a multiple of 32: a 64-byte slab of K
    is 32 channels of one tap), "gather" = mlpk_im2col + mlpk_gemm_nt"""
    return "window" if dtype in (torch.float16, torch.bfloat16) and Cin >= 32 and Cin % 32 == 0 else "gather"


def conv3_columns(weight):
    """Conv2d weight (Cout, Cin, kh, kw) -> (Cout, kh kw Cin) with columns in tap-major order (i kw + j) Cin + ci: mlpk_im2col's NHWC column order,
    which is mlpk_conv_gemm_nhwc's K order"""
    w = weight.detach()
    return w.permute(0, 2, 3, 1).reshape(w.shape[0], -1)


def bn_scale_shift(bn, device):
    """BatchNorm2d(eval) as the per-column scale and shift of the product in front of it: y = scale conv(x) + shift, scale = weight / sqrt(
    running_var + eps), shift = bias - running_mean scale (fp32; an affine-less BatchNorm counts as weight 1, bias 0)"""
    f = lambda v: v.detach().to(device=device, dtype=torch.float32)
    scale = torch.rsqrt(f(bn.running_var) + bn.eps)
    if bn.weight is not None:
        scale = scale * f(bn.weight)
    shift = -f(bn.running_mean) * scale
    if bn.bias is not None:
        shift = shift + f(bn.bias)
    return scale.contiguous(), shift.contiguous()


def pack_conv(pk, p, conv, bn, dtype, device, nchw=False):
    """a Conv2d (1 x 1 or 3 x 3) [+ BatchNorm2d] under prefix p: w, and b (the convolution's bias) or s / h (the BatchNorm)"""
    if nchw:                                                            # the tokenizer's first convolution reads the NCHW image: ci kh kw + i kw + j
        pk[p + "w"] = E.pack_matrix(conv.weight, dtype, device, kpad=E.embed_kpad(dtype))
    else:
        pk[p + "w"] = E.pack_matrix(conv3_columns(conv.weight), dtype, device)
    pk[p + "b"] = E.f32(conv.bias, device)
    pk[p + "s"], pk[p + "h"] = bn_scale_shift(bn, device) if bn is not None else (None, None)


def pack_tokenizer(pk, p, tok, dtype, device):
    blk = tok.block
    pack_conv(pk, p + "c0.", blk[0], blk[1], dtype, device, nchw=True)
    pack_conv(pk, p + "c1.", blk[3], blk[4], dtype, device)
    pack_conv(pk, p + "c2.", blk[6], blk[7], dtype, device)


def pack_conv_stage(pk, p, stage, dtype, device):
    for i, blk in enumerate(stage.conv_blocks):
        for j in range(3):
            pack_conv(pk, "%sb%d.c%d." % (p, i, j), blk[3 * j], blk[3 * j + 1], dtype, device)
    pack_conv(pk, p + "down.", stage.downsample, None, dtype, device)


def pack_mlp_stage(pk, p, blk, dtype, device):
    for k, (norm, mlp) in (("m1.", (blk.norm1, blk.channel_mlp1)), ("m2.", (blk.norm2, blk.channel_mlp2))):
        if not isinstance(mlp.act, nn.GELU):
            raise NotImplementedError("ConvMLPStage: Mlp runs with the reference's default activation (GELU) only")
        pack_channel_mlp(pk, p + k, norm, mlp.fc1, mlp.fc2, dtype, device)
    C = blk.connect.weight.shape[0]
    pk[p + "cn.w"] = blk.connect.weight.detach().to(device=device, dtype=torch.float32).reshape(C, 9).t().contiguous()        # [9][C] tap-major
    pk[p + "cn.g"], pk[p + "cn.be"] = E.f32(blk.connect_norm.weight, device), E.f32(blk.connect_norm.bias, device)


# ------------------------------------------------------------------ forward pieces on channel-last rows
def half(n):
    """the extent after a 3 x 3 stride-2 pad-1 window"""
    return (n - 1) // 2 + 1


def require(ok, entry, dtype, *shape):
    if not ok:
        raise NotImplementedError("ConvMLP: %s does not take %s in %s (widths must be whole 16-byte vectors: multiples of 8 channels in the 16-bit "
                                  "types, of 4 in float32)" % (entry, " x ".join(str(s) for s in shape), dtype))


def require_width(dtype, entry, *widths):
    vec = 4 if dtype == torch.float32 else 8
    for c in widths:
        require(c > 0 and c % vec == 0, entry, dtype, c)


def relu(buf, rows, C, res=None, out=None):
    E.relu_add(buf, res, out if out is not None else buf, rows * C)


def conv3x3(ws, tag, src, pk, p, out, B, H, W, Cin, stride):
    """a dense 3 x 3 pad-1 convolution of the channel-last rows `src` -> out (B Ho Wo, Cout): one product, the BatchNorm or the bias in its epilogue"""
    Ho, Wo = (half(H), half(W)) if stride == 2 else (H, W)
    w = pk[p + "w"]
    epi = dict(bias=pk[p + "b"], cscale=pk[p + "s"], cshift=pk[p + "h"], tag="convmlp_3x3")
    if conv_plan(src.dtype, Cin) == "window":
        E.conv_gemm_nhwc(src, w, out, B, H, W, Cin, 3, 3, stride, 1, **epi)
    else:
        kp = w.shape[1]
        cols = ws.get(tag + ".cols", (B * Ho * Wo, kp))
        E.im2col(src, cols, B, Cin, H, W, 3, 3, stride, stride, 1, kp, layout=N.LAYOUT_NHWC, px_stride=Cin)
        E.gemm(cols, w, out, B * Ho * Wo, w.shape[0], kp, **epi)
    return Ho, Wo


def tokenizer_check(dtype, B, H, W, c):
    require_width(dtype, "mlpk_relu_add (ConvTokenizer)", c // 2, c)
    H1, W1 = half(H), half(W)
    require(E.relu_add_supported(dtype, B * H1 * W1 * (c // 2)), "mlpk_relu_add", dtype, B, H1, W1, c // 2)
    require(E.relu_maxpool3s2_supported(dtype, B, H1, W1, c), "mlpk_relu_maxpool3s2_nhwc", dtype, B, H1, W1, c)


def tokenizer_rows(ws, pk, p, x, c, tag="tok"):
    """ConvTokenizer on the NCHW image x -> (rows (B H2 W2, c), H2, W2)"""
    B, cin, H, W = x.shape
    H1, W1 = half(H), half(W)
    rows, h = B * H1 * W1, c // 2
    w0 = pk[p + "c0.w"]
    cols = ws.get(tag + ".cols0", (rows, w0.shape[1]))
    E.im2col(x, cols, B, cin, H, W, 3, 3, 2, 2, 1, w0.shape[1])
    t0 = ws.get(tag + ".t0", (rows, h))
    E.gemm(cols, w0, t0, rows, h, w0.shape[1], cscale=pk[p + "c0.s"], cshift=pk[p + "c0.h"], tag="convmlp_stem")
    relu(t0, rows, h)
    t1 = ws.get(tag + ".t1", (rows, h))
    conv3x3(ws, tag + ".c1", t0, pk, p + "c1.", t1, B, H1, W1, h, 1)
    relu(t1, rows, h)
    t2 = ws.get(tag + ".t2", (rows, c))
    conv3x3(ws, tag + ".c2", t1, pk, p + "c2.", t2, B, H1, W1, h, 1)
    H2, W2 = half(H1), half(W1)
    out = ws.get(tag + ".out", (B * H2 * W2, c))
    E.relu_maxpool3s2_nhwc(t2, out, B, H1, W1, c)
    return out, H2, W2


def conv_stage_check(dtype, B, H, W, cin, hid, cout):
    require_width(dtype, "mlpk_relu_add (ConvStage)", cin, hid, cout)
    require(E.relu_add_supported(dtype, B * H * W * hid) and E.relu_add_supported(dtype, B * H * W * cin), "mlpk_relu_add", dtype, B, H, W, max(cin, hid))


def conv_stage_rows(ws, pk, p, cur, B, H, W, nblocks, cin, hid, cout, tag="cs"):
    """ConvStage on rows (B H W, cin), the blocks in place -> (rows (B H2 W2, cout), H2, W2)"""
    rows = B * H * W
    h1, h2, h3 = ws.get(tag + ".h1", (rows, hid)), ws.get(tag + ".h2", (rows, hid)), ws.get(tag + ".h3", (rows, cin))
    for i in range(nblocks):
        q = "%sb%d." % (p, i)
        E.gemm(cur, pk[q + "c0.w"], h1, rows, hid, cin, cscale=pk[q + "c0.s"], cshift=pk[q + "c0.h"], tag="convmlp_1x1")
        relu(h1, rows, hid)
        conv3x3(ws, tag + ".c1", h1, pk, q + "c1.", h2, B, H, W, hid, 1)
        relu(h2, rows, hid)
        E.gemm(h2, pk[q + "c2.w"], h3, rows, cin, hid, cscale=pk[q + "c2.s"], cshift=pk[q + "c2.h"], tag="convmlp_1x1")
        relu(h3, rows, cin, res=cur, out=cur)                           # x + block(x), the block's last ReLU inside
    H2, W2 = half(H), half(W)
    out = ws.get(tag + ".out", (B * H2 * W2, cout))
    conv3x3(ws, tag + ".down", cur, pk, p + "down.", out, B, H, W, cin, 2)
    return out, H2, W2


def mlp_stage_check(dtype, B, H, W, C, hidden):
    require_width(dtype, "mlpk_ln_dwconv3_nhwc (ConvMLPStage)", C, hidden)
    require(E.ln_dwconv3_supported(dtype, B, H, W, C), "mlpk_ln_dwconv3_nhwc", dtype, B, H, W, C)


def mlp_stage_rows(ws, pk, p, a, b, st, B, H, W, C, hidden, tag):
    """one ConvMLPStage: the rows in `a` (statistics `st`, or None) -> the rows in `b`; returns what the last GEMM's `part` delivered"""
    rows = B * H * W
    got = channel_mlp(ws, a, rows, C, pk, p + "m1.", hidden, tag=tag + ".m1", stats=st, part=(ws, tag + ".m1.part"))
    st = finalize_stats(ws, got, rows, C, tag=tag + ".cn.ln")
    if st is None:
        st = layernorm_stats(ws, a, rows, C, tag=tag + ".cn.ln")
    E.ln_dwconv3_nhwc(a, st[0], st[1], pk[p + "cn.g"], pk[p + "cn.be"], pk[p + "cn.w"], b, B, H, W, C)
    return channel_mlp(ws, b, rows, C, pk, p + "m2.", hidden, tag=tag + ".m2", part=(ws, tag + ".m2.part"))


def to_rows(ws, name, x, B, H, W, C, channel_last):
    cur = ws.get(name, (B * H * W, C))
    cur.view(B, H, W, C).copy_(x if channel_last else x.permute(0, 2, 3, 1))
    return cur


def to_nchw(cur, B, H, W, C):
    return cur.view(B, H, W, C).permute(0, 3, 1, 2).clone(memory_format=torch.contiguous_format)


# ------------------------------------------------------------------ the reference's classes
class ConvTokenizer(SubModule):
    """conv_mlp.py:52-87.  Callable on its own like the reference's: x (B, 3, H, W) -> (B, embedding_dim, H / 4, W / 4)."""

    def __init__(self, embedding_dim=64):
        super(ConvTokenizer, self).__init__()
        self.block = nn.Sequential(
            nn.Conv2d(3, embedding_dim // 2, kernel_size=(3, 3), stride=(2, 2), padding=(1, 1), bias=False),
            nn.BatchNorm2d(embedding_dim // 2),
            nn.ReLU(inplace=True),
            nn.Conv2d(embedding_dim // 2, embedding_dim // 2, kernel_size=(3, 3), stride=(1, 1), padding=(1, 1), bias=False),
            nn.BatchNorm2d(embedding_dim // 2),
            nn.ReLU(inplace=True),
            nn.Conv2d(embedding_dim // 2, embedding_dim, kernel_size=(3, 3), stride=(1, 1), padding=(1, 1), bias=False),
            nn.BatchNorm2d(embedding_dim),
            nn.ReLU(inplace=True),
            nn.MaxPool2d(kernel_size=(3, 3), stride=(2, 2), padding=(1, 1), dilation=(1, 1))
        )

    def _pack(self, dtype, device):
        pk = {}
        pack_tokenizer(pk, "", self, dtype, device)
        return pk

    def forward(self, x):
        c = self.block[6].out_channels
        pk = self._begin(x, 3, axis=1)
        if x.dim() != 4:
            raise ValueError("expected a (B, 3, H, W) tensor, got %s" % (tuple(x.shape),))
        B, _, H, W = x.shape
        tokenizer_check(x.dtype, B, H, W, c)
        with E.on_device(x):
            ws = self._get_space((B, H, W), x.dtype, x.device)
            out, H2, W2 = tokenizer_rows(ws, pk, "", x.contiguous(), c)
            return to_nchw(out, B, H2, W2, c)


class ConvStage(SubModule):
    """conv_mlp.py:91-126.  Callable on its own like the reference's: x (B, embedding_dim_in, H, W) -> (B, embedding_dim_out, H / 2, W / 2)."""

    def __init__(self, num_blocks=2, embedding_dim_in=64, hidden_dim=128, embedding_dim_out=128):
        super(ConvStage, self).__init__()
        self.conv_blocks = nn.ModuleList()
        for i in range(num_blocks):
            block = nn.Sequential(
                nn.Conv2d(embedding_dim_in, hidden_dim, kernel_size=(1, 1), stride=(1, 1), padding=(0, 0), bias=False),
                nn.BatchNorm2d(hidden_dim),
                nn.ReLU(inplace=True),
                nn.Conv2d(hidden_dim, hidden_dim, kernel_size=(3, 3), stride=(1, 1), padding=(1, 1), bias=False),
                nn.BatchNorm2d(hidden_dim),
                nn.ReLU(inplace=True),
                nn.Conv2d(hidden_dim, embedding_dim_in, kernel_size=(1, 1), stride=(1, 1), padding=(0, 0), bias=False),
                nn.BatchNorm2d(embedding_dim_in),
                nn.ReLU(inplace=True)
            )
            self.conv_blocks.append(block)
        self.downsample = nn.Conv2d(embedding_dim_in, embedding_dim_out, kernel_size=(3, 3), stride=(2, 2), padding=(1, 1))
        self.__dict__["_geom"] = (num_blocks, embedding_dim_in, hidden_dim, embedding_dim_out)

    def _pack(self, dtype, device):
        pk = {}
        pack_conv_stage(pk, "", self, dtype, device)
        return pk

    def forward(self, x):
        nblocks, cin, hid, cout = self.__dict__["_geom"]
        pk = self._begin(x, cin, axis=1)
        if x.dim() != 4:
            raise ValueError("expected a (B, %d, H, W) tensor, got %s" % (cin, tuple(x.shape)))
        B, _, H, W = x.shape
        conv_stage_check(x.dtype, B, H, W, cin, hid, cout)
        with E.on_device(x):
            ws = self._get_space((B, H, W), x.dtype, x.device)
            cur = to_rows(ws, "cs.x", x, B, H, W, cin, channel_last=False)
            out, H2, W2 = conv_stage_rows(ws, pk, "", cur, B, H, W, nblocks, cin, hid, cout)
            return to_nchw(out, B, H2, W2, cout)


class Mlp(_Container):
    """conv_mlp.py:129-143"""

    def __init__(self, embedding_dim_in, hidden_dim=None, embedding_dim_out=None, activation=nn.GELU):
        super().__init__()
        hidden_dim = hidden_dim or embedding_dim_in
        embedding_dim_out = embedding_dim_out or embedding_dim_in
        self.fc1 = nn.Linear(embedding_dim_in, hidden_dim)
        self.act = activation()
        self.fc2 = nn.Linear(hidden_dim, embedding_dim_out)


class ConvMLPStage(SubModule):
    """conv_mlp.py:146-170.  Callable on its own like the reference's: src (B, H, W, C) -> (B, H, W, C)."""

    def __init__(self, embedding_dim, dim_feedforward=2048, stochastic_depth_rate=0.1):
        super(ConvMLPStage, self).__init__()
        self.norm1 = nn.LayerNorm(embedding_dim)
        self.channel_mlp1 = Mlp(embedding_dim_in=embedding_dim, hidden_dim=dim_feedforward)
        self.norm2 = nn.LayerNorm(embedding_dim)
        self.connect = nn.Conv2d(embedding_dim, embedding_dim, kernel_size=(3, 3), stride=(1, 1), padding=(1, 1), groups=embedding_dim, bias=False)
        self.connect_norm = nn.LayerNorm(embedding_dim)
        self.channel_mlp2 = Mlp(embedding_dim_in=embedding_dim, hidden_dim=dim_feedforward)
        self.drop_path = DropPath(stochastic_depth_rate) if stochastic_depth_rate > 0 else nn.Identity()
        self.__dict__["_geom"] = (embedding_dim, dim_feedforward)

    def _pack(self, dtype, device):
        pk = {}
        pack_mlp_stage(pk, "", self, dtype, device)
        return pk

    def forward(self, src):
        C, hidden = self.__dict__["_geom"]
        pk = self._begin(src, C)
        if src.dim() != 4:
            raise ValueError("expected a channel-last (B, H, W, %d) tensor, got %s" % (C, tuple(src.shape)))
        B, H, W, _ = src.shape
        mlp_stage_check(src.dtype, B, H, W, C, hidden)
        with E.on_device(src):
            ws = self._get_space((B, H, W), src.dtype, src.device)
            a = to_rows(ws, "ms.a", src, B, H, W, C, channel_last=True)
            b = ws.get("ms.b", (B * H * W, C))
            mlp_stage_rows(ws, pk, "", a, b, None, B, H, W, C, hidden, "ms")
            return b.view(B, H, W, C).clone()


class ConvDownsample(_Container):
    """conv_mlp.py:173-182"""

    def __init__(self, embedding_dim_in, embedding_dim_out):
        super().__init__()
        self.downsample = nn.Conv2d(embedding_dim_in, embedding_dim_out, kernel_size=(3, 3), stride=(2, 2), padding=(1, 1))


class BasicStage(_Container):
    """conv_mlp.py:185-208"""

    def __init__(self, num_blocks, embedding_dims, mlp_ratio=1, stochastic_depth_rate=0.1, downsample=True):
        super(BasicStage, self).__init__()
        self.blocks = nn.ModuleList()
        dpr = [x.item() for x in torch.linspace(0, stochastic_depth_rate, num_blocks)]
        for i in range(num_blocks):
            block = ConvMLPStage(embedding_dim=embedding_dims[0], dim_feedforward=int(embedding_dims[0] * mlp_ratio), stochastic_depth_rate=dpr[i])
            self.blocks.append(block)
        self.downsample_mlp = ConvDownsample(embedding_dims[0], embedding_dims[1]) if downsample else nn.Identity()


class ConvMLP(E.EngineModule):
    """conv_mlp.py:212-275.  Inference-only (no `_train_forward`): in train mode the forward warns and runs as in eval mode."""

    def __init__(self, depth, d_model, expansion_factor, channels=64, n_conv_blocks=3, classifier_head=True, num_classes=1000, *args, **kwargs):
        super(ConvMLP, self).__init__()
        assert len(depth) == len(expansion_factor) == len(expansion_factor), \
            f"depth, d_model and expansion_factor must agree in size, {len(depth)}, {len(d_model)} and {len(expansion_factor)} passed."

        self.tokenizer = ConvTokenizer(embedding_dim=channels)
        self.conv_stages = ConvStage(n_conv_blocks, embedding_dim_in=channels, hidden_dim=d_model[0], embedding_dim_out=d_model[0])

        self.stages = nn.ModuleList()
        for i in range(0, len(depth)):
            stage = BasicStage(num_blocks=depth[i], embedding_dims=d_model[i:i + 2], mlp_ratio=expansion_factor[i], stochastic_depth_rate=0.1,
                               downsample=(i + 1 < len(depth)))
            self.stages.append(stage)
        if classifier_head:
            self.norm = nn.LayerNorm(d_model[-1])
            self.head = nn.Linear(d_model[-1], num_classes)
        else:
            self.head = None
        self.apply(self.init_weight)
        self.__dict__["_channels"] = channels

    @staticmethod
    def init_weight(m):
        if isinstance(m, (nn.Linear, nn.Conv1d)):
            nn.init.trunc_normal_(m.weight, std=.02)
            if m.bias is not None:
                nn.init.constant_(m.bias, 0)
        elif isinstance(m, nn.LayerNorm):
            nn.init.constant_(m.bias, 0)
            nn.init.constant_(m.weight, 1.0)
        elif isinstance(m, nn.Conv2d):
            nn.init.kaiming_normal_(m.weight, mode='fan_out', nonlinearity='relu')
        elif isinstance(m, nn.BatchNorm2d):
            nn.init.constant_(m.weight, 1.)
            nn.init.constant_(m.bias, 0.)

    # ------------------------------------------------------------------ packing
    def _pack(self, dtype, device):
        pk = {}
        pack_tokenizer(pk, "tok.", self.tokenizer, dtype, device)
        pack_conv_stage(pk, "cs.", self.conv_stages, dtype, device)
        for i, stage in enumerate(self.stages):
            for j, blk in enumerate(stage.blocks):
                pack_mlp_stage(pk, "s%d.b%d." % (i, j), blk, dtype, device)
            if isinstance(stage.downsample_mlp, ConvDownsample):
                pack_conv(pk, "s%d.down." % i, stage.downsample_mlp.downsample, None, dtype, device)
        if self.head is not None:
            pk["head.g"], pk["head.be"] = E.f32(self.norm.weight, device), E.f32(self.norm.bias, device)
            pk["head.w"], pk["head.b"] = E.pack_matrix(self.head.weight, dtype, device), E.f32(self.head.bias, device)
        return pk

    def _check(self, cd, B, H, W):
        """every kernel's shape check for a (B, 3, H, W) input, before anything is launched"""
        nblocks, cin, hid, cout = self.conv_stages.__dict__["_geom"]
        tokenizer_check(cd, B, H, W, self.__dict__["_channels"])
        H, W = half(half(H)), half(half(W))
        conv_stage_check(cd, B, H, W, cin, hid, cout)
        H, W = half(H), half(W)
        for stage in self.stages:
            for blk in stage.blocks[:1]:                                # (BasicStage builds every block of a stage with one geometry)
                mlp_stage_check(cd, B, H, W, *blk.__dict__["_geom"])
            if isinstance(stage.downsample_mlp, ConvDownsample):
                require_width(cd, "mlpk_gemm_nt (ConvDownsample)", stage.downsample_mlp.downsample.out_channels)
                H, W = half(H), half(W)

    # ------------------------------------------------------------------ forward
    def forward(self, x):
        cd = self._resolve(x)
        B, cin, H, W = x.shape
        if cin != 3 or H < 1 or W < 1:
            raise ValueError("expected a (B, 3, H, W) tensor, got %s" % (tuple(x.shape),))
        self._check(cd, B, H, W)
        pk = self._get_pack(cd, x.device)
        ws = self._get_space(B, cd, x.device)
        cur, H, W = tokenizer_rows(ws, pk, "tok.", x.contiguous(), self.__dict__["_channels"])
        nblocks, c_in, hid, C = self.conv_stages.__dict__["_geom"]
        cur, H, W = conv_stage_rows(ws, pk, "cs.", cur, B, H, W, nblocks, c_in, hid, C)
        got = None
        for i, stage in enumerate(self.stages):
            rows = B * H * W
            tag = "s%d" % i
            other = ws.get(tag + ".y", (rows, C))
            for j, blk in enumerate(stage.blocks):
                hidden = blk.__dict__["_geom"][1]
                got = mlp_stage_rows(ws, pk, "s%d.b%d." % (i, j), cur, other, finalize_stats(ws, got, rows, C, tag=tag + ".m1.ln"), B, H, W, C, hidden, tag)
                cur, other = other, cur
            if isinstance(stage.downsample_mlp, ConvDownsample):
                Cout = stage.downsample_mlp.downsample.out_channels
                nxt = ws.get("s%d.x" % (i + 1), (B * half(H) * half(W), Cout))
                H2, W2 = conv3x3(ws, tag + ".down", cur, pk, tag + ".down.", nxt, B, H, W, C, 2)
                cur, H, W, C, got = nxt, H2, W2, Cout, None
        rows = B * H * W
        if self.head is None:
            if cd != x.dtype:
                out = torch.empty((B, H, W, C), dtype=x.dtype, device=x.device)
                E.convert(cur, out, rows * C)
                return out
            return cur.view(B, H, W, C).clone()
        st = finalize_stats(ws, got, rows, C, tag="head.ln", eps=self.norm.eps)
        if st is None:
            st = layernorm_stats(ws, cur, rows, C, tag="head.ln", eps=self.norm.eps)
        pooled = ws.get("pooled", (B, C))
        E.pool_mean(cur, B, H * W, C, C, pooled, C, mean=st[0], rstd=st[1], gamma=pk["head.g"], beta=pk["head.be"])
        return head_linear(ws, pooled, B, C, pk["head.w"], pk["head.b"], self.head.out_features, x.dtype)


def _convmlp(arch, pretrained, progress, classifier_head, depth, d_model, expansion_factor, *args, **kwargs):
    if pretrained:
        raise RuntimeError("%s(pretrained=True): this tree holds no checkpoint URL and downloads nothing; build the model and call "
                           "load_state_dict with a checkpoint of the reference's ConvMLP (the keys and shapes are the same)" % arch)
    return ConvMLP(depth=depth, d_model=d_model, expansion_factor=expansion_factor, classifier_head=classifier_head, *args, **kwargs)


def convmlp_s(pretrained=False, progress=False, classifier_head=True, *args, **kwargs):
    return _convmlp('convmlp_s', pretrained=pretrained, progress=progress,
                    depth=[2, 4, 2], expansion_factor=[2, 2, 2], d_model=[128, 256, 512],
                    channels=64, n_conv_blocks=2, classifier_head=classifier_head,
                    *args, **kwargs)


def convmlp_m(pretrained=False, progress=False, classifier_head=True, *args, **kwargs):
    return _convmlp('convmlp_m', pretrained=pretrained, progress=progress,
                    depth=[3, 6, 3], expansion_factor=[3, 3, 3], d_model=[128, 256, 512],
                    channels=64, n_conv_blocks=3, classifier_head=classifier_head,
                    *args, **kwargs)


def convmlp_l(pretrained=False, progress=False, classifier_head=True, *args, **kwargs):
    return _convmlp('convmlp_l', pretrained=pretrained, progress=progress,
                    depth=[4, 8, 3], expansion_factor=[3, 3, 3], d_model=[192, 384, 768],
                    channels=96, n_conv_blocks=3, classifier_head=classifier_head,
                    *args, **kwargs)
