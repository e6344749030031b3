"""CPU checks of RaftMLP: the module tree and constructor contract of the reference's raft_mlp.py (tests/golden/raft_mlp.npz, made by
tests/golden/make_raft_golden.py from the reference itself), the packers on CPU tensors, and the argument checks of mlpk_raft_gather_ln /
mlpk_raft_scatter_add, which return before anything touches a device."""
import inspect
import json
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN, ROOT, load_pkg

FIX = os.path.join(GOLDEN, "raft_mlp.npz")
ENULL, EDTYPE, ESHAPE, EALIGN = -4, -1, -2, -3


def mp():
    return load_pkg().models_pytorch


@pytest.fixture(scope="module")
def z():
    return np.load(FIX)


@pytest.fixture(scope="module")
def meta(z):
    return json.loads(str(z["meta"]))


def table(model):
    return {k: list(v.shape) for k, v in model.state_dict().items()}


@pytest.mark.parametrize("tm", ["ser_pm", "sep_ln_codim_tm", "sep_ln_ch_tm", "original_tm"])
def test_state_dict_table_matches_reference_tiny(tm, z, meta):
    want = json.loads(str(z["shapes/" + tm]))
    got = table(mp().RaftMLP(meta["tiny"], image_size=40, num_classes=10, token_mixing_type=tm, gap=True))
    assert list(got) == list(want)
    assert got == want
    if tm == "ser_pm":
        assert "levels.0.fn.2.1.norm.1.weight" in got and "heads.0.4.weight" in got


@pytest.mark.parametrize("name", ["pyramid", "single"])
def test_state_dict_table_matches_reference_real(name, z, meta):
    want = json.loads(str(z["shapes/" + name]))
    got = table(mp().RaftMLP(meta["real"][name], gap=True))
    assert list(got) == list(want)
    assert got == want


def test_constants_exports_and_signature():
    pkg = load_pkg()
    rm = pkg.models_pytorch.raft_mlp
    assert "RaftMLP" in pkg.models_pytorch.__all__ and pkg.RaftMLP is pkg.models_pytorch.RaftMLP is rm.RaftMLP
    assert (rm.SER_PM, rm.SEP_LN_CODIM_TM, rm.SEP_LN_CH_TM, rm.ORIGINAL_TM) == ("ser_pm", "sep_ln_codim_tm", "sep_ln_ch_tm", "original_tm")
    assert rm.TOKEN_MIXING_TYPES == [rm.SER_PM, rm.SEP_LN_CODIM_TM, rm.SEP_LN_CH_TM, rm.ORIGINAL_TM]
    assert (rm.PATCH_SIZE, rm.RAFT_SIZE, rm.DIM, rm.DEPTH, rm.LOGGER_NAME) == ("patch_size", "raft_size", "dim", "depth", "RaftMLP")
    for name in ("DropPath", "Block", "ChannelBlock", "TokenBlock", "SpatiallySeparatedTokenBlock", "PermutedBlock", "Level",
                 "SeparatedLNCodimLevel", "SeparatedLNChannelLevel", "SerialPermutedLevel", "OriginalLevel", "RaftMLP"):
        assert inspect.isclass(getattr(rm, name)), name
    sig = [(p.name, p.default) for p in inspect.signature(rm.RaftMLP).parameters.values()]
    assert sig == [("layers", inspect._empty), ("in_channels", 3), ("image_size", 224), ("num_classes", 1000), ("token_expansion_factor", 2),
                   ("channel_expansion_factor", 4), ("dropout", 0.0), ("token_mixing_type", "ser_pm"), ("shortcut", True), ("gap", False),
                   ("drop_path_rate", 0.0)]
    sig = [(p.name, p.default) for p in inspect.signature(rm.PermutedBlock).parameters.values()]
    assert sig == [("spatial_dim", inspect._empty), ("channels", inspect._empty), ("raft_size", inspect._empty), ("expansion_factor", 4),
                   ("dropout", 0.0), ("drop_path_rate", 0.0)]
    sig = [(p.name, p.default) for p in inspect.signature(rm.SerialPermutedLevel).parameters.values()]
    assert sig == [("in_channels", inspect._empty), ("out_channels", inspect._empty), ("depth", 4), ("image_size", 224), ("patch_size", 4),
                   ("token_expansion_factor", 2), ("channel_expansion_factor", 4), ("dropout", 0.0), ("drop_path_rate", 0.0), ("raft_size", 4)]
    import re
    with open(rm.__file__) as f:
        assert re.search(r"^\s*(from|import)\s+einops", f.read(), re.M) is None                # the product does not import einops


def test_constructor_assertions(meta):
    RaftMLP = mp().RaftMLP
    tiny = meta["tiny"]
    with pytest.raises(AssertionError):
        RaftMLP(tiny, token_mixing_type="nope")
    with pytest.raises(AssertionError):
        RaftMLP([{"depth": 1, "dim": 16, "patch_size": 4}])                                   # ser_pm needs raft_size
    RaftMLP([{"depth": 1, "dim": 16, "patch_size": 4}], image_size=16, token_mixing_type="original_tm")
    for missing in ("depth", "dim", "patch_size"):
        with pytest.raises(AssertionError):
            RaftMLP([{k: v for k, v in tiny[0].items() if k != missing}])
    with pytest.raises(AssertionError):
        RaftMLP([{"depth": 1, "dim": 0, "patch_size": 4, "raft_size": 2}])
    with pytest.raises(AssertionError):
        RaftMLP([{"depth": 1, "dim": 18, "patch_size": 4, "raft_size": 4}])                   # dim % raft_size
    m = RaftMLP(tiny, image_size=42, num_classes=10, drop_path_rate=0.1, dropout=0.2)
    lvl = m.levels[0]
    assert (lvl._bh, lvl._h) == (10, 11) and (m.levels[1]._bh, m.levels[1]._h) == (5, 6)
    assert m.classifier.in_features == 32 * 36 and isinstance(m.flatten, torch.nn.Flatten)
    assert isinstance(lvl.fn[2][1].drop, mp().raft_mlp.DropPath) and lvl.fn[2][1].fn[2].p == 0.2
    ident = mp().raft_mlp.SerialPermutedLevel(8, 16, depth=1, image_size=8, patch_size=1, raft_size=2)
    assert isinstance(ident.fn[1], torch.nn.Identity)                                          # patch 1, widths differ: no Linear, as in the reference
    assert isinstance(mp().raft_mlp.SerialPermutedLevel(16, 16, depth=1, image_size=8, patch_size=1, raft_size=2).fn[1], torch.nn.Linear)


def test_containers_and_cpu_inputs_raise(meta):
    rm = mp().raft_mlp
    m = rm.RaftMLP(meta["tiny"], image_size=40, num_classes=10).eval()
    with pytest.raises(NotImplementedError, match="RaftMLP"):
        m.levels[0](torch.zeros(1, 3, 40, 40))
    with pytest.raises(NotImplementedError, match="RaftMLP"):
        rm.TokenBlock(4, 8)(torch.zeros(1, 8, 4))
    with pytest.raises(NotImplementedError, match="RaftMLP"):
        m.levels[0].fn[0](torch.zeros(1, 3, 40, 40))
    blk = m.levels[0].fn[2]
    for mod, x in ((m, torch.zeros(1, 3, 40, 40)), (blk[1], torch.zeros(1, 8 * 10, 2 * 10)), (blk[5], torch.zeros(1, 100, 16)),
                   (rm.SpatiallySeparatedTokenBlock(7, 24), torch.zeros(1, 24 * 3, 7))):
        with pytest.raises(NotImplementedError):            # no CPU implementation, as for every family
            mod(x)


def test_raft_entries_declared_and_exported_at_abi_14():
    N = load_pkg()._native
    with open(os.path.join(ROOT, "include", "mlpk.h")) as f:
        h = f.read()
    for name in ("mlpk_raft_gather_ln", "mlpk_raft_scatter_add", "mlpk_raft_supported"):
        assert name in N.PROTOTYPES and "int %s(" % name in h
    assert "mlpk_raft.hip" in __import__("importlib").import_module("jittor-mlp_amd.build").SOURCES
    assert N.lib().mlpk_abi_version() == 14


def test_raft_argument_errors():
    N = load_pkg()._native
    lib = N.lib()
    P = 1 << 20                                             # a 16-byte aligned address that is never dereferenced: every call below fails its checks
    base = dict(dtype=N.BF16, x=P, ldx=96, mean=P, rstd=P, gamma=P, beta=P, a=P, lda=128, kp=112, y=P, ldy=112, B=2, H=56, W=56, C=96, r=2, axis=0)

    def gather(**kw):
        k = dict(base, **kw)
        return lib.mlpk_raft_gather_ln(k["dtype"], k["x"], k["ldx"], k["mean"], k["rstd"], k["gamma"], k["beta"], k["a"], k["lda"], k["kp"],
                                       k["B"], k["H"], k["W"], k["C"], k["r"], k["axis"], None)

    def scatter(**kw):
        k = dict(base, **kw)
        return lib.mlpk_raft_scatter_add(k["dtype"], k["x"], k["ldx"], k["y"], k["ldy"], k["B"], k["H"], k["W"], k["C"], k["r"], k["axis"], None)

    for kw in ({"x": None}, {"a": None}, {"mean": None}, {"rstd": None}):
        assert gather(**kw) == ENULL, kw
    for kw in ({"x": None}, {"y": None}):
        assert scatter(**kw) == ENULL, kw
    for call in (gather, scatter):
        assert call(dtype=7) == EDTYPE
        for kw in ({"B": 0}, {"H": 0}, {"W": -1}, {"C": 0}, {"r": 0}, {"r": 5}, {"axis": 2}, {"axis": -1}, {"ldx": 88}, {"C": 100, "ldx": 104},
                   {"dtype": N.F32, "C": 6, "ldx": 8}):
            assert call(**kw) == ESHAPE, (call.__name__, kw)
        assert call(x=P + 2) == EALIGN and call(ldx=100) == EALIGN and call(dtype=N.F32, x=P + 8) == EALIGN and call(dtype=N.F32, ldx=98) == EALIGN
    assert gather(kp=111) == ESHAPE and gather(kp=136) == ESHAPE                   # kp < D, kp > lda
    assert gather(axis=1, H=28, kp=56) == ESHAPE                                     # D follows the axis: L = W = 56
    assert gather(a=P + 4) == EALIGN and gather(lda=132) == EALIGN
    assert scatter(ldy=104) == ESHAPE
    assert scatter(y=P + 6) == EALIGN and scatter(ldy=116) == EALIGN
    assert scatter(dtype=N.F32, H=2048, C=1024, ldx=1024, ldy=4096) == ESHAPE       # a line that does not fit the LDS it is turned over in
    S = lib.mlpk_raft_supported
    for dtype in (N.F32, N.F16, N.BF16):
        for H, W, C, r in ((56, 56, 96, 2), (14, 14, 768, 4), (1, 1, 8, 2), (7, 9, 24, 1), (5, 3, 16, 4)):
            assert S(dtype, H, W, C, r, 0) == 1 and S(dtype, H, W, C, r, 1) == 1
    assert S(N.F32, 5, 3, 12, 4, 0) == 1 and S(N.BF16, 5, 3, 12, 4, 0) == 0          # C % 4 for fp32, C % 8 for 16-bit
    assert S(9, 7, 7, 96, 2, 0) == 0 and S(N.BF16, 7, 7, 96, 5, 0) == 0 and S(N.BF16, 7, 7, 96, 2, 2) == 0 and S(N.BF16, 0, 7, 96, 2, 0) == 0
    assert S(N.F32, 2048, 4, 1024, 2, 0) == 0 and S(N.F32, 2048, 4, 1024, 2, 1) == 1 # the limit follows L


# ------------------------------------------------------------------ the packers, on CPU tensors
def test_layernorm_affine_permutation():
    rm = mp().raft_mlp
    Co, r = 6, 4
    v = torch.arange(Co * r, dtype=torch.float32)            # reference order: index co * r + j
    g = rm.raft_affine(v, r)
    for j in range(r):
        for co in range(Co):
            assert float(g[j * Co + co]) == co * r + j
    assert torch.equal(rm.raft_affine(v, 1), v)
    blk = rm.PermutedBlock(5, Co * r, r)
    with torch.no_grad():
        blk.norm[1].weight.copy_(v)
        blk.norm[1].bias.copy_(-v)
    pk = {}
    rm.pack_raft_half(pk, "p.", blk, r, torch.float32, torch.device("cpu"))
    assert torch.equal(pk["p.ln.g"], g) and torch.equal(pk["p.ln.b"], -g)
    assert "p.fused" not in pk                                # fp32 never takes the fused entry


def test_token_mlp_zero_padding():
    rm = mp().raft_mlp
    T, D, dp = 40, 20, 32
    w1, b1, w2, b2 = torch.randn(T, D), torch.randn(T), torch.randn(D, T), torch.randn(D)
    w1p, b1p, w2p, b2p = rm.pad_token_mlp(w1, b1, w2, b2, dp)
    assert tuple(w1p.shape) == (T, dp) and tuple(w2p.shape) == (dp, T) and tuple(b2p.shape) == (dp,)
    assert torch.equal(w1p[:, :D], w1) and float(w1p[:, D:].abs().max()) == 0.0
    assert torch.equal(w2p[:D], w2) and float(w2p[D:].abs().max()) == 0.0
    assert torch.equal(b2p[:D], b2) and float(b2p[D:].abs().max()) == 0.0 and torch.equal(b1p, b1)
    assert rm.fused_width(112) == 128 and rm.fused_width(56) == 64 and rm.fused_width(64) == 64
    blk = rm.PermutedBlock(7, 24, 2, 2)                       # D = 14, T = 28: the GEMM pair's K padded to whole 16-byte chunks
    pk = {}
    rm.pack_token_mlp(pk, "", blk.fn, torch.bfloat16, torch.device("cpu"))
    assert tuple(pk["fc1.w"].shape) == (28, 16) and tuple(pk["fc2.w"].shape) == (14, 32)
    assert float(pk["fc1.w"][:, 14:].float().abs().max()) == 0.0 and float(pk["fc2.w"][:, 28:].float().abs().max()) == 0.0
    assert torch.equal(pk["fc1.w"][:, :14], blk.fn[0].weight.detach().bfloat16())


def test_embedding_and_classifier_column_permutations():
    rm = mp().raft_mlp
    p, cin, out = 4, 3, 5
    w = torch.arange(out * p * p * cin, dtype=torch.float32).reshape(out, p * p * cin)        # columns (p1 p2 c)
    e = rm.embed_columns_nchw(w, p, cin)
    for c in range(cin):
        for i in range(p):
            for j in range(p):
                assert torch.equal(e[:, c * p * p + i * p + j], w[:, (i * p + j) * cin + c])
    C, S, nc = 8, 6, 3
    wc = torch.arange(nc * C * S, dtype=torch.float32).reshape(nc, C * S)                      # columns (c, h w)
    k = rm.classifier_columns_nhwc(wc, C, S)
    for c in range(C):
        for s in range(S):
            assert torch.equal(k[:, s * C + c], wc[:, c * S + s])
