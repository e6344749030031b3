"""CPU checks of DynaMixer: the module tree and constructor contract of the reference's dyna_mlp.py (tests/golden/dyna_mlp.npz, made by
tests/golden/make_dyna_golden.py from the reference itself), the packers on CPU tensors, the `_supported` truth table and the argument checks of
mlpk_dyna_mix, which return before anything touches a device, and the host side of the cache contract (tests/test_lifecycle_host.py's tests on a
Config registered in its _CACHE)."""
import importlib
import inspect
import json
import os
import re

import numpy as np
import pytest
import torch
from torch import nn

from conftest import GOLDEN, ROOT, load_pkg
import test_lifecycle_host as LH
from test_gpu_dyna import NAME, SHAPES, add_tiny_settings, dyna_config

FIX = os.path.join(GOLDEN, "dyna_mlp.npz")
DM = load_pkg().models_pytorch.dyna_mlp
ENULL, EDTYPE, ESHAPE, EALIGN = -4, -1, -2, -3


@pytest.fixture(scope="module")
def z():
    return np.load(FIX)


@pytest.fixture(scope="module")
def meta(z):
    return json.loads(str(z["meta"]))


def table(model):
    return {k: list(v.shape) for k, v in model.state_dict().items()}


def sig(f):
    return [(p.name, p.default) for p in inspect.signature(f).parameters.values()]


def test_exports_and_signatures():
    pkg = load_pkg()
    E_ = inspect._empty
    assert "DynaMixer" in pkg.models_pytorch.__all__ and pkg.DynaMixer is pkg.models_pytorch.DynaMixer is DM.DynaMixer
    for name in ("PreNorm", "FeedForward", "DynaMixerOp_w", "DynaMixerOp_h", "DynaBlock", "DynaMLPBlock", "DynaMixer"):
        cls = getattr(DM, name)
        assert inspect.isclass(cls) and not cls.__module__.startswith(pkg.__name__ + ".models_pytorch"), name
    assert sig(DM.DynaMixer) == [("model_name", 'M'), ("image_size", 224), ("in_channels", 3), ("num_classes", 1000)]
    assert sig(DM.DynaMLPBlock) == [("depth", E_), ("h", E_), ("w", E_), ("dim", E_), ("hidden_dim_DMO", E_), ("segment", E_), ("mlp_dim", E_), ("dropout", 0.)]
    assert sig(DM.DynaBlock) == [("h", E_), ("w", E_), ("dim", E_), ("hidden_dim_DMO", 2), ("segment", 8)]
    assert sig(DM.DynaMixerOp_h) == [("h", E_), ("dim", E_), ("hidden_dim", E_), ("segment", E_)]
    assert sig(DM.DynaMixerOp_w) == [("w", E_), ("dim", E_), ("hidden_dim", E_), ("segment", E_)]
    assert sig(DM.PreNorm) == [("dim", E_), ("fn", E_)] and sig(DM.FeedForward) == [("dim", E_), ("hidden_dim", E_), ("dropout", 0.)]
    assert DM.dynamlp_settings["T"] == [[7, 2], [192, 384], [4, 14], [8, 16], 3, 0.1, 2]
    assert DM.dynamlp_settings["M"] == [[7, 2], [256, 512], [7, 17], [8, 16], 3, 0.1, 2]
    assert DM.dynamlp_settings["L"] == [[7, 2], [256, 512], [9, 27], [8, 16], 3, 0.3, 8]
    assert DM.dynamlp_settings is importlib.import_module(pkg.__name__ + ".dyna_impl").dynamlp_settings
    with pytest.raises(AssertionError, match="DynaMLP model name"):
        DM.DynaMixer("XXL")
    with pytest.raises(AssertionError, match="divisible"):
        DM.DynaMixer("T", image_size=225)
    for mod in (DM, importlib.import_module(pkg.__name__ + ".dyna_impl")):
        with open(mod.__file__) as f:
            assert re.search(r"^\s*(from|import)\s+(einops|timm|torchvision)", f.read(), re.M) is None, mod.__file__


def test_state_dict_tables_match_reference(z, meta):
    add_tiny_settings(meta)
    makes = {n: (lambda n=n: DM.DynaMixer(n)) for n in ("T", "M", "L")}
    makes.update({n: (lambda n=n: DM.DynaMixer(n, image_size=tuple(meta["tiny_sizes"][0]), num_classes=meta["tiny_classes"])) for n in meta["tiny"]})
    for name, make in makes.items():
        want = json.loads(str(z["shapes/" + name]))
        got = table(make())
        assert list(got) == list(want), name
        assert got == want, name
    got = table(DM.DynaMixer("tiny", image_size=(24, 40)))
    assert got["stages.0.1.layers.0.0.fn.DynaMixerOp_h.attend.1.weight"] == [6 * 6, 6 * 2]              # image_size as a pair: L differs per axis
    assert got["stages.1.1.layers.1.0.fn.DynaMixerOp_w.attend.1.weight"] == [5 * 5, 5 * 2]
    assert got["stages.1.0.weight"] == [32, 16, 2, 2] and got["mlp_head.1.weight"] == [1000, 32]


def test_fixture_softmax_sites_exercise_the_mixer(meta):
    """what the generator asserted before it wrote the file: no softmax site of any recorded case is close to uniform, no logit is beyond 32"""
    lim = meta["limits"]
    assert lim == {"min_row_max": 0.4, "max_abs_logit": 32.0, "min_move_over_bf16": 20.0} and meta["scale"] == 8.0
    stats = meta["softmax_stats"]
    assert len(stats) == 6 + len(meta["blocks"]) + 3
    for name, st in stats.items():
        assert st["row_max_lo"] >= 0.4 and st["max_abs_logit"] <= 32.0 and st["sites"] >= 1, (name, st)


def test_real_fixture_moves_with_the_attend_scale(z):
    for name in ("T", "M", "L"):
        assert float(z["real/%s/move_x1" % name]) >= 20.0 * float(z["real/%s/err_bf16" % name]), name
        assert 0.0 < float(z["real/%s/err_fp32" % name]) < float(z["real/%s/err_fp16" % name]) < float(z["real/%s/err_bf16" % name]), name


def test_dyna_entries_declared_and_exported_at_abi_14():
    N = load_pkg()._native
    with open(os.path.join(ROOT, "include", "mlpk.h")) as f:
        h = f.read()
    for name in ("mlpk_dyna_mix", "mlpk_dyna_mix_supported", "mlpk_dyna_gather", "mlpk_dyna_mix_logits"):
        assert name in N.PROTOTYPES and "int %s(" % name in h
    assert "mlpk_dyna.hip" in importlib.import_module("jittor-mlp_amd.build").SOURCES
    assert N.lib().mlpk_abi_version() == 14
    E = load_pkg().engine
    assert callable(E.dyna_mix) and callable(E.dyna_mix_supported) and callable(E.pack_dyna_attend)


def test_dyna_supported_table():
    N = load_pkg()._native
    S = N.lib().mlpk_dyna_mix_supported
    for dtype in (N.F32, N.F16, N.BF16):
        for H, W, C, s, hd in SHAPES:
            assert S(dtype, H, C, s, hd) == 1 and S(dtype, W, C, s, hd) == 1, (dtype, H, W, C, s, hd)
        for L in range(1, 33):                                  # L = 1 .. 32 with L hd <= 256, d a multiple of 8
            for hd in (1, 2, 8):
                assert S(dtype, L, 64, 4, hd) == 1, (dtype, L, hd)
        for C, s, hd, L in ((192, 8, 2, 32), (384, 16, 2, 16), (256, 8, 2, 32), (512, 16, 2, 16), (256, 8, 8, 32), (512, 16, 8, 16),
                            (16, 2, 2, 10), (32, 4, 8, 5), (32, 4, 2, 1), (16, 2, 8, 2)):
            assert S(dtype, L, C, s, hd) == 1, (dtype, L, C, s, hd)  # every stage of T, M, L at 224 and of the tiny configurations
        assert S(dtype, 33, 64, 4, 2) == 0 and S(dtype, 32, 64, 4, 9) == 0 and S(dtype, 32, 64, 4, 8) == 1 and S(dtype, 16, 64, 4, 16) == 1
        assert S(dtype, 0, 64, 4, 2) == 0 and S(dtype, 8, 0, 4, 2) == 0 and S(dtype, 8, 64, 0, 2) == 0 and S(dtype, 8, 64, 4, 0) == 0
        assert S(dtype, 8, 64, 5, 2) == 0 and S(dtype, 8, 60, 5, 2) == (1 if dtype == N.F32 else 0)           # C % s; d = 12: fp32 only
    assert S(N.F32, 8, 16, 4, 2) == 1 and S(N.BF16, 8, 16, 4, 2) == 0 and S(N.F16, 8, 16, 4, 2) == 0               # d = 4
    assert S(N.F32, 8, 8, 4, 2) == 0 and S(9, 8, 64, 4, 2) == 0


def test_dyna_argument_errors():
    N = load_pkg()._native
    lib = N.lib()
    P = 1 << 20                                             # a 16-byte aligned address that is never dereferenced: every call below fails its checks
    base = dict(dtype=N.BF16, x=P, x_pitch=64, mean=P, rstd=P, gamma=P, beta=P, t=P, t_pitch=32, t_off=16, aw=P, ab=P, out=P, out_pitch=192,
                B=2, H=32, W=16, C=64, s=8, hd=2, axis=0)

    def call(**kw):
        k = dict(base, **kw)
        return lib.mlpk_dyna_mix(k["dtype"], k["x"], k["x_pitch"], k["mean"], k["rstd"], k["gamma"], k["beta"], k["t"], k["t_pitch"], k["t_off"],
                                 k["aw"], k["ab"], k["out"], k["out_pitch"], k["B"], k["H"], k["W"], k["C"], k["s"], k["hd"], k["axis"], None)

    for kw in ({"x": None}, {"t": None}, {"aw": None}, {"ab": None}, {"out": None}, {"mean": None}, {"rstd": None}):
        assert call(**kw) == ENULL, kw
    assert call(dtype=7) == EDTYPE
    for kw in ({"B": 0}, {"H": 0}, {"W": -1}, {"C": 0}, {"s": 0}, {"hd": 0}, {"axis": 2}, {"axis": -1}, {"H": 33}, {"axis": 1, "W": 33}, {"hd": 9},
               {"s": 7}, {"s": 16}, {"x_pitch": 56}, {"out_pitch": 56}, {"t_pitch": 31}, {"t_off": 17}, {"t_off": -1},
               {"dtype": N.F32, "C": 48, "s": 8, "x_pitch": 48}):
        assert call(**kw) == ESHAPE, kw
    for kw in ({"x": P + 2}, {"out": P + 8}, {"aw": P + 4}, {"x_pitch": 68}, {"out_pitch": 196}, {"t": P + 1}, {"ab": P + 2},
               {"dtype": N.F32, "x": P + 8}, {"dtype": N.F32, "x_pitch": 66}, {"dtype": N.F32, "t": P + 2}):
        assert call(**kw) == EALIGN, kw
    assert call(H=33, axis=1, x=P + 2) == EALIGN                # the shape passed: only the extent along the axis is bounded by 32


# ------------------------------------------------------------------ the packers, on CPU tensors
def test_pack_dyna_attend_layout():
    E = load_pkg().engine
    L, hd = 5, 2
    K, Nn = L * hd, L * L
    w = torch.arange(Nn * K, dtype=torch.float32).reshape(Nn, K) / 8.0
    b = -torch.arange(Nn, dtype=torch.float32)
    for dtype, e in ((torch.float32, 4), (torch.bfloat16, 8), (torch.float16, 8)):
        pw, pb = E.pack_dyna_attend(w, b, dtype, torch.device("cpu"))
        kp = (K + e - 1) // e * e
        assert tuple(pw.shape) == (kp // e, Nn, e) and pw.dtype == dtype and pw.is_contiguous() and pb.dtype == torch.float32
        for k in range(kp):
            want = w[:, k].to(dtype) if k < K else torch.zeros(Nn, dtype=dtype)
            assert torch.equal(pw[k // e, :, k % e], want), (dtype, k)
        assert torch.equal(pb, b) and pb.data_ptr() != b.data_ptr()


def test_cat_wd_and_fold_projections():
    torch.manual_seed(0)
    blk = DM.DynaBlock(5, 7, 16, 2, 2)
    w, b = DM.cat_wd([blk.DynaMixerOp_h, blk.DynaMixerOp_w], torch.device("cpu"))
    assert tuple(w.shape) == (2 * 2 * 2, 16) and tuple(b.shape) == (8,)
    for oi, op in enumerate((blk.DynaMixerOp_h, blk.DynaMixerOp_w)):
        for g in range(2):
            assert torch.equal(w[oi * 4 + g * 2:oi * 4 + g * 2 + 2], op.Wd[g].weight.detach()) and torch.equal(b[oi * 4 + g * 2:oi * 4 + g * 2 + 2], op.Wd[g].bias.detach())
    w3, b3 = DM.fold_projections(blk, torch.device("cpu"))
    assert tuple(w3.shape) == (16, 48) and w3.dtype == torch.float32
    g = torch.Generator().manual_seed(1)
    mh, mw, xn = (torch.randn(9, 16, generator=g, dtype=torch.float64) for _ in range(3))
    with torch.no_grad():
        d = blk.double()
        want = d.proj_o(d.DynaMixerOp_h.proc(mh) + d.DynaMixerOp_w.proc(mw) + d.proj_c(xn))
    got = torch.cat([mh, mw, xn], 1) @ w3.double().t() + b3.double()
    assert float((got - want).abs().max()) <= 1e-6 * float(want.abs().max())
    pk = {}
    DM.pack_block(pk, "q.", blk.float(), nn.LayerNorm(16), torch.bfloat16, torch.device("cpu"))
    assert set(pk) == {"q.ln.g", "q.ln.b", "q.wd.w", "q.wd.b", "q.h.aw", "q.h.ab", "q.w.aw", "q.w.ab", "q.h.awr", "q.w.awr", "q.o.w", "q.o.b"}
    assert tuple(pk["q.h.aw"].shape) == (2, 25, 8) and tuple(pk["q.w.aw"].shape) == (2, 49, 8) and pk["q.o.w"].dtype == torch.bfloat16


# ------------------------------------------------------------------ the cache contract on the host
def test_pack_aliasing_and_param_stamp():
    pkg = load_pkg()
    cfg = dyna_config()
    assert LH.config(NAME) is cfg
    LH.test_param_stamp_sees_every_visible_update_form(NAME)
    LH.test_param_stamp_changes_for_every_single_entry(NAME)
    LH.test_param_stamp_visits_each_state_dict_entry_exactly_once(NAME)
    for dtype in ("fp32", "bf16"):
        LH.test_no_eval_pack_tensor_aliases_a_parameter(pkg, NAME, dtype)
    LH.test_invalidate_caches_empties_the_module_tree_and_its_train_packs(pkg, NAME)
    LH.test_copies_and_pickles_travel_without_the_caches(pkg, NAME)
    m = cfg.fresh()
    with torch.no_grad():
        keys = set(m._pack(torch.float32, torch.device("cpu")))
    assert {"s0.embed.w", "s1.embed.b", "s0.b0.ln.g", "s1.b1.h.aw", "s1.b1.w.ab", "s0.b0.o.w", "s1.b0.ff.fc1.csum", "head.w"} <= keys


# ------------------------------------------------------------------ what cannot run
def test_containers_and_cpu_inputs_raise(meta):
    add_tiny_settings(meta)
    m = DM.DynaMixer("tiny", image_size=(40, 40), num_classes=3).eval()
    blk = m.stages[0][1]
    x = torch.zeros(1, 10, 10, 16)
    for mod in (blk.layers[0][0], blk.layers[0][1], blk.layers[0][1].fn, DM.FeedForward(16, 48), DM.PreNorm(16, nn.Identity())):
        with pytest.raises(NotImplementedError, match="DynaMixer"):
            mod(x)
    with pytest.raises(NotImplementedError, match="placeholder"):
        blk.reshape(x)
    for mod, arg in ((m, torch.zeros(1, 3, 40, 40)), (blk, torch.zeros(1, 16, 10, 10)), (blk.layers[0][0].fn, x), (blk.layers[0][0].fn.DynaMixerOp_h, x),
                     (blk.layers[0][0].fn.DynaMixerOp_w, x)):
        with pytest.raises(NotImplementedError):                # no CPU implementation, as for every family
            mod(arg)


def test_unfused_entries_argument_errors():
    N = load_pkg()._native
    lib = N.lib()
    P = 1 << 20
    g = dict(dtype=N.BF16, t=P, t_pitch=32, t_off=16, v=P, v_pitch=64, kp=64, B=2, H=32, W=16, s=8, hd=2, axis=0)

    def gather(**kw):
        k = dict(g, **kw)
        return lib.mlpk_dyna_gather(k["dtype"], k["t"], k["t_pitch"], k["t_off"], k["v"], k["v_pitch"], k["kp"], k["B"], k["H"], k["W"], k["s"], k["hd"],
                                    k["axis"], None)

    assert gather(t=None) == ENULL and gather(v=None) == ENULL and gather(dtype=7) == EDTYPE
    for kw in ({"B": 0}, {"axis": 2}, {"H": 33}, {"hd": 9}, {"kp": 63}, {"v_pitch": 56}, {"t_pitch": 31}, {"t_off": -1}, {"B": 1 << 22, "H": 32, "W": 32}):
        assert gather(**kw) == ESHAPE, kw
    assert gather(t=P + 1) == EALIGN and gather(v=P + 1) == EALIGN
    m = dict(dtype=N.BF16, x=P, x_pitch=64, mean=P, rstd=P, gamma=P, beta=P, z=P, z_pitch=1024, out=P, out_pitch=192, B=2, H=32, W=16, C=64, s=8, hd=2, axis=0)

    def mix(**kw):
        k = dict(m, **kw)
        return lib.mlpk_dyna_mix_logits(k["dtype"], k["x"], k["x_pitch"], k["mean"], k["rstd"], k["gamma"], k["beta"], k["z"], k["z_pitch"], k["out"],
                                        k["out_pitch"], k["B"], k["H"], k["W"], k["C"], k["s"], k["hd"], k["axis"], None)

    for kw in ({"x": None}, {"z": None}, {"out": None}, {"mean": None}):
        assert mix(**kw) == ENULL, kw
    assert mix(dtype=7) == EDTYPE
    for kw in ({"B": 0}, {"axis": 2}, {"H": 33}, {"s": 7}, {"z_pitch": 1023}, {"x_pitch": 56}, {"out_pitch": 56}):
        assert mix(**kw) == ESHAPE, kw
    for kw in ({"x": P + 2}, {"out": P + 8}, {"z": P + 1}, {"x_pitch": 68}):
        assert mix(**kw) == EALIGN, kw
    E = load_pkg().engine
    assert E.dyna_unfused_preferred(torch.bfloat16, 32) and E.dyna_unfused_preferred(torch.float16, 16) and E.dyna_unfused_preferred(torch.bfloat16, 8)
    assert not E.dyna_unfused_preferred(torch.float32, 32) and not E.dyna_unfused_preferred(torch.bfloat16, 10) and not E.dyna_unfused_preferred(torch.bfloat16, 4)
