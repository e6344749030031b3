"""CPU checks of Sequencer2D: the module tree and constructor contract of the reference's sequencer.py (tests/golden/sequencer.npz, made by
tests/golden/make_sequencer_golden.py from the reference itself), the packers on CPU tensors in fp64 against torch.nn.LSTM, the `_supported`
truth table and the argument checks of mlpk_lstm_scan, which return before anything touches a device, and the host side of the cache contract
(tests/test_lifecycle_host.py's tests on a Config registered in its _CACHE)."""
import copy
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
import lstm_model as LM
from test_gpu_sequencer import DTYPES, HIDS, IDS, MASK_MAP, NAME, SHAPES, add_tiny_settings, from_seqs, operands, restate, sequencer_config, to_seqs

FIX = os.path.join(GOLDEN, "sequencer.npz")
SQ = load_pkg().models_pytorch.sequencer
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
    return [(p.name, p.default, p.kind) for p in inspect.signature(f).parameters.values()]


def test_exports_and_signatures():
    pkg = load_pkg()
    E_, P = inspect._empty, inspect.Parameter
    impl = importlib.import_module(pkg.__name__ + ".sequencer_impl")
    assert "Sequencer2D" in pkg.models_pytorch.__all__ and pkg.Sequencer2D is pkg.models_pytorch.Sequencer2D is SQ.Sequencer2D
    for name in ("PatchEmbedOverlap", "PreNormResidual", "BiLSTM2D", "Sequencer2DBlock", "Sequencer2D"):
        cls = getattr(SQ, name)
        assert inspect.isclass(cls) and cls is getattr(impl, name) and not cls.__module__.startswith(pkg.__name__ + ".models_pytorch"), name
    K = P.POSITIONAL_OR_KEYWORD
    assert sig(SQ.Sequencer2D) == [("model_name", 'M', K), ("pretrained", None, K), ("num_classes", 1000, K), ("in_channels", 3, K),
                                   ("args", E_, P.VAR_POSITIONAL), ("kwargs", E_, P.VAR_KEYWORD)]
    assert sig(SQ.Sequencer2DBlock) == [("d_model", E_, K), ("depth", E_, K), ("hidden_d_model", E_, K), ("expansion_factor", 3, K), ("dropout", 0., K)]
    assert sig(SQ.BiLSTM2D) == [("d_model", E_, K), ("hidden_d_model", E_, K)]
    assert sig(SQ.PreNormResidual) == [("dim", E_, K), ("fn", E_, K)]
    assert sig(SQ.PatchEmbedOverlap) == [("patch_size", 16, K), ("stride", 16, K), ("padding", 0, K), ("embed_dim", 768, K)]
    assert SQ.sequencer_settings["S"] == [[4, 3, 8, 3], [192, 384, 384, 384], [48, 96, 96, 96], 3]
    assert SQ.sequencer_settings["M"] == [[4, 3, 14, 3], [192, 384, 384, 384], [48, 96, 96, 96], 3]
    assert SQ.sequencer_settings["L"] == [[8, 8, 16, 4], [192, 384, 384, 384], [48, 96, 96, 96], 3]
    assert SQ.sequencer_settings is impl.sequencer_settings
    with pytest.raises(AssertionError, match="Sequencer model name should be in"):
        SQ.Sequencer2D("XXL")
    SQ.sequencer_settings["one"] = [[1, 1, 1, 1], [16, 16, 16, 16], [16, 16, 16, 16], 2]       # an entry added to the table is seen
    try:
        got = table(SQ.Sequencer2D("one", num_classes=5, in_channels=4))
        assert got["stages.0.0.weight"] == [16, 4, 7, 7] and got["stages.0.1.model.0.1.fn.0.weight"] == [32, 16] and got["mlp_head.1.weight"] == [5, 16]
    finally:
        del SQ.sequencer_settings["one"]
    for mod in (SQ, impl):
        with open(mod.__file__) as f:
            assert re.search(r"^\s*(from|import)\s+(einops|timm|torchvision)", f.read(), re.M) is None, mod.__file__


def test_state_dict_tables_match_reference(z):
    for name in ("S", "M", "L"):
        want = json.loads(str(z["shapes/" + name]))
        got = table(SQ.Sequencer2D(name))
        assert list(got) == list(want), name
        assert got == want, name
    got = table(SQ.Sequencer2D("S"))
    for sfx in ("", "_reverse"):
        assert got["stages.0.1.model.0.0.fn.0.rnn_v.weight_ih_l0" + sfx] == [192, 192] and got["stages.1.1.model.2.0.fn.0.rnn_h.weight_hh_l0" + sfx] == [384, 96]
        assert got["stages.3.1.model.2.0.fn.0.rnn_h.bias_ih_l0" + sfx] == [384] and got["stages.0.1.model.3.0.fn.0.rnn_v.bias_hh_l0" + sfx] == [192]
    assert got["mlp_head.1.weight"] == [1000, 384] and got["stages.2.0.weight"] == [384, 384, 1, 1] and got["stages.1.0.weight"] == [384, 192, 2, 2]


def test_fixture_exercises_the_recurrence(z, meta):
    """what the generator asserted before it wrote the file, and the cases the GPU tests expect"""
    assert meta["limits"] == {"min_hh_move_over_gate": 100.0} and meta["hh_scale"] == 4.0
    assert meta["tiny"] == {"tiny": [[1, 2, 1, 1], [32, 64, 64, 64], [16, 32, 32, 32], 3]} and meta["tiny_sizes"] == [[56, 56], [70, 42]]
    assert set(meta["hh_move_over_gate"]) == set(meta["blocks"]) and all(v >= 100.0 for v in meta["hh_move_over_gate"].values())
    skipped = meta["lowp_skipped"]
    assert not any(k.startswith("real/S") for k in skipped)
    for tag in ("fp16", "bf16"):
        assert len([k for k in skipped if k.endswith("/" + tag)]) <= 1
    cases = ["tiny/56x56", "tiny/70x42", "real/S"] + ["block/" + n for n in meta["blocks"]]
    for case in cases:
        for tag in ("fp16", "bf16"):
            err = float(z["%s/err_%s" % (case, tag)])
            assert ("%s/%s" % (case, tag) in skipped) == (err != err), (case, tag)
            assert err != err or err > 0.0
    assert z["real/S/logits"].shape == (2, 1000) and z["tiny/70x42/logits"].shape == (2, 10)
    assert z["block/bilstm_32_16/out"].shape == (2, 5, 3, 32) and z["block/block_64_1_32/out"].shape == (2, 64, 4, 6)


def test_lstm_entries_declared_and_exported_at_abi_14():
    N = load_pkg()._native
    with open(os.path.join(ROOT, "include", "mlpk.h")) as f:
        h = f.read()
    for name in ("mlpk_lstm_scan", "mlpk_lstm_scan_supported"):
        assert name in N.PROTOTYPES and "int %s(" % name in h
    assert "mlpk_lstm.hip" in importlib.import_module("jittor-mlp_amd.build").SOURCES
    assert N.lib().mlpk_abi_version() == 14
    E = load_pkg().engine
    assert callable(E.lstm_scan) and callable(E.lstm_scan_supported) and callable(E.pack_lstm_hh)


def test_lstm_supported_table():
    N = load_pkg()._native
    S = N.lib().mlpk_lstm_scan_supported
    for dtype in (N.F32, N.F16, N.BF16):
        for hid in (16, 32, 48, 96):
            for L in (1, 2, 3, 5, 16, 32, 33, 37, 224, 100000):
                assert S(dtype, L, hid) == 1, (dtype, L, hid)
            assert S(dtype, 0, hid) == 0 and S(dtype, -1, hid) == 0
        for _, H, W, hid in SHAPES:
            assert S(dtype, H, hid) == 1 and S(dtype, W, hid) == 1
        for hid in (0, -16, 8, 15, 17, 24, 47, 49, 64, 80, 95, 97, 112, 128, 192):
            assert S(dtype, 16, hid) == 0, (dtype, hid)
    assert S(3, 16, 48) == 0 and S(-1, 16, 48) == 0


def test_lstm_argument_errors():
    N = load_pkg()._native
    lib = N.lib()
    P, Q = 1 << 20, 1 << 28                                  # 16-byte aligned addresses that are never dereferenced: every call below fails its checks
    base = dict(dtype=N.BF16, xp=P, xp_pitch=768, xp_off=384, whh=P, out=Q, out_pitch=192, out_off=96, B=2, H=32, W=16, hid=48, axis=0)

    def call(**kw):
        k = dict(base, **kw)
        return lib.mlpk_lstm_scan(k["dtype"], k["xp"], k["xp_pitch"], k["xp_off"], k["whh"], k["out"], k["out_pitch"], k["out_off"], k["B"], k["H"],
                                  k["W"], k["hid"], k["axis"], None)

    for kw in ({"xp": None}, {"whh": None}, {"out": None}):
        assert call(**kw) == ENULL, kw
    assert call(dtype=7) == EDTYPE and call(dtype=-1) == EDTYPE
    for kw in ({"B": 0}, {"H": 0}, {"W": -1}, {"hid": 0}, {"hid": 64}, {"hid": 40}, {"axis": 2}, {"axis": -1}, {"xp_off": -4}, {"out_off": -4},
               {"xp_pitch": 764}, {"xp_off": 388}, {"out_pitch": 188}, {"out_off": 100}, {"dtype": N.F32, "hid": 24}):
        assert call(**kw) == ESHAPE, kw
    for kw in ({"xp": P + 8}, {"out": Q + 8}, {"whh": P + 8}, {"xp": P + 2}, {"xp_pitch": 770}, {"out_pitch": 194}, {"xp_off": 382, "xp_pitch": 772},
               {"out_off": 94}, {"dtype": N.F32, "xp": P + 4}, {"dtype": N.F32, "out_pitch": 193},
               {"out": P}, {"out": P + 16}, {"out": P + 1024 * 768 * 2 - 192 - 16}, {"xp": Q, "out": Q + 2 * 384}):
        assert call(**kw) == EALIGN, kw
    assert call(axis=1, H=1 << 20, W=1, out=P) == EALIGN     # every earlier check passed: any B, H, W


# ------------------------------------------------------------------ the packers, in fp64 against torch
def scan_restate(xp, whh, B, H, W, hid, axis):
    """mlpk_lstm_scan's contract in fp64: xp (rows, 8 hid) = [forward i f g o | reverse i f g o], whh (2, 4 hid, hid) -> (rows, 2 hid)"""
    sx = to_seqs(xp.double(), B, H, W, axis)
    L = sx.shape[1]
    out = torch.zeros(sx.shape[0], L, 2 * hid, dtype=torch.float64)
    for d in range(2):
        h = torch.zeros(sx.shape[0], hid, dtype=torch.float64)
        c = torch.zeros_like(h)
        for t in range(L):
            l = L - 1 - t if d else t
            zz = sx[:, l, 4 * d * hid:4 * (d + 1) * hid] + h @ whh[d].double().t()
            i, f, g, o = zz.split(hid, 1)
            c = torch.sigmoid(f) * c + torch.sigmoid(i) * torch.tanh(g)
            h = torch.sigmoid(o) * torch.tanh(c)
            out[:, l, d * hid:(d + 1) * hid] = h
    return from_seqs(out, B, H, W, axis)


def test_projection_order_bias_fold_and_hh_pack_against_nn_lstm():
    """cat_lstm_ih + pack_lstm_hh + the kernel's contract restated in fp64 reproduce BiLSTM2D's two nn.LSTMs with the reference's reshapes"""
    E = load_pkg().engine
    torch.manual_seed(0)
    B, H, W, C, hid = 2, 5, 3, 12, 16
    mod = SQ.BiLSTM2D(C, hid)
    with torch.no_grad():
        for p in mod.parameters():
            p.mul_(3.0)
    ref = copy.deepcopy(mod).double()                        # (the packers read fp32 parameters exactly; torch runs the same values in fp64)
    x = torch.randn(B, H, W, C, dtype=torch.float64)
    w, b = SQ.cat_lstm_ih([mod.rnn_v, mod.rnn_h], torch.device("cpu"))
    assert tuple(w.shape) == (16 * hid, C) and tuple(b.shape) == (16 * hid,) and w.dtype == torch.float32
    assert torch.equal(w[:4 * hid], mod.rnn_v.weight_ih_l0.detach().float()) and torch.equal(w[12 * hid:], mod.rnn_h.weight_ih_l0_reverse.detach().float())
    assert torch.equal(b[4 * hid:8 * hid], mod.rnn_v.bias_ih_l0_reverse.detach().float() + mod.rnn_v.bias_hh_l0_reverse.detach().float())
    xp = x.reshape(-1, C) @ w.double().t() + b.double()
    with torch.no_grad():
        v, _ = ref.rnn_v(x.permute(0, 2, 1, 3).reshape(-1, H, C))
        v = v.reshape(B, W, H, -1).permute(0, 2, 1, 3)
        h, _ = ref.rnn_h(x.reshape(-1, W, C))
        h = h.reshape(B, H, W, -1)
    for axis, rnn, want, off in ((0, mod.rnn_v, v, 0), (1, mod.rnn_h, h, 8 * hid)):
        whh = E.pack_lstm_hh(rnn.weight_hh_l0, rnn.weight_hh_l0_reverse, torch.float32, torch.device("cpu"))
        got = scan_restate(xp[:, off:off + 8 * hid], whh, B, H, W, hid, axis)
        assert float((got - want.reshape(-1, 2 * hid)).abs().max()) <= 1e-6, axis


def test_pack_lstm_hh_round_trips():
    E = load_pkg().engine
    g = torch.Generator().manual_seed(1)
    for hid in (16, 48):
        wf, wr = torch.randn(4 * hid, hid, generator=g), torch.randn(4 * hid, hid, generator=g)
        for dtype in (torch.float32, torch.float16, torch.bfloat16):
            p = E.pack_lstm_hh(wf, wr, dtype, torch.device("cpu"))
            assert tuple(p.shape) == (2, 4 * hid, hid) and p.dtype == dtype and p.is_contiguous()
            a, b = E.unpack_lstm_hh(p)
            assert torch.equal(a, wf.to(dtype)) and torch.equal(b, wr.to(dtype))
            assert p.data_ptr() != wf.data_ptr()
    p = E.pack_lstm_hh(wf, wr, torch.float32, torch.device("cpu"))
    assert p.untyped_storage().data_ptr() not in (wf.untyped_storage().data_ptr(), wr.untyped_storage().data_ptr())


def test_layernorm_fold_of_the_projection():
    """pack_bilstm with the PreNormResidual's LayerNorm: rstd (x W'^T - mean csum) + b' is the projection of LayerNorm(x)"""
    torch.manual_seed(2)
    C, hid = 24, 16
    mod, norm = SQ.BiLSTM2D(C, hid), nn.LayerNorm(C)
    with torch.no_grad():
        norm.weight.uniform_(0.25, 4.0)
        norm.bias.uniform_(-1.0, 1.0)
    pk = {}
    SQ.pack_bilstm(pk, "q.", mod, norm, torch.float32, torch.device("cpu"))
    assert set(pk) == {"q.ih.w", "q.ih.b", "q.ih.csum", "q.v.hh", "q.h.hh", "q.fc.w", "q.fc.b"}
    assert tuple(pk["q.ih.w"].shape) == (16 * hid, C) and tuple(pk["q.v.hh"].shape) == (2, 4 * hid, hid) and tuple(pk["q.fc.w"].shape) == (C, 4 * hid)
    x = torch.randn(9, C, dtype=torch.float64) * 2 + 0.5
    mean, var = x.mean(1, keepdim=True), x.var(1, unbiased=False, keepdim=True)
    rstd = (var + norm.eps).rsqrt()
    got = rstd * (x @ pk["q.ih.w"].double().t() - mean * pk["q.ih.csum"].double()) + pk["q.ih.b"].double()
    w, b = SQ.cat_lstm_ih([mod.rnn_v, mod.rnn_h], torch.device("cpu"))
    with torch.no_grad():
        want = norm.double()(x) @ w.double().t() + b.double()
    assert float((got - want).abs().max()) <= 1e-5 * float(want.abs().max())
    alone = {}
    SQ.pack_bilstm(alone, "", mod, None, torch.bfloat16, torch.device("cpu"))
    assert "ih.csum" not in alone and alone["ih.w"].dtype == torch.bfloat16 and alone["ih.b"].dtype == torch.float32


# ------------------------------------------------------------------ the CPU model of the scan (tests/lstm_model.py) and its planted faults
MODEL_CASES = pytest.mark.parametrize("hid,dtype", [pytest.param(hid, dtype, id="hid%d-%s" % (hid, name)) for hid in HIDS for dtype, name in zip(DTYPES, IDS)])
AXES = pytest.mark.parametrize("axis", [0, 1], ids=["v", "h"])


def model(fault=None):
    return lambda xp, whh, B, H, W, hid, dtype, axis: LM.scan_model(xp, whh, B, H, W, hid, dtype, axis, fault)


@pytest.mark.parametrize("hid", HIDS)
@AXES
def test_the_model_equals_fp64_lstm_within_the_fp32_gate(hid, axis):
    """the faultless model in fp32 storage against fp64 nn.LSTM on random operands: 4 d, d = the distance of torch's own fp32 LSTM (the rule of
    tests/test_gpu_sequencer.py), at most a fifth of the distance to the restatement without the recurrence"""
    for B, H, W in (MASK_MAP, (2, 5, 3)):
        xp, whh = operands(B, H, W, hid, torch.float32, 100 * hid + axis)
        exact = restate(xp, whh, B, H, W, hid, axis, torch.float64)
        gate = 4.0 * float((restate(xp, whh, B, H, W, hid, axis, torch.float32) - exact).abs().max())
        far = float((restate(xp, torch.zeros_like(whh), B, H, W, hid, axis, torch.float64) - exact).abs().max())
        err = float((LM.scan_model(xp, whh, B, H, W, hid, torch.float32, axis).double() - exact).abs().max())
        assert 0.0 < gate <= 0.2 * far and err <= gate, (B, H, W, err, gate, far)


@MODEL_CASES
@AXES
def test_the_model_passes_the_recurrence_checks(hid, dtype, axis):
    """what tests/test_gpu_sequencer.py asks of the kernel, asked of the faultless model: the replay of every gate and permutation, the forget
    gate's value check (whose condition gate <= far / 5 is a CPU figure: it holds here before anything runs on a GPU) and the identical lines"""
    for kind in LM.KINDS:
        for gate in ("i", "g", "o"):
            assert LM.replay_check(model(), *MASK_MAP, hid, dtype, axis, gate, kind) > 0
        LM.forget_check(model(), *MASK_MAP, hid, dtype, axis, kind)
    LM.identical_check(model(), *MASK_MAP, hid, dtype, axis)


# fault -> check -> the axes of MASK_MAP on which the check fails the faulty model ("vh": both, "h": axis 1 only, "": the check CANNOT see it).
# replay, forget and identical are the checks of tests/test_gpu_sequencer.py.  What identical lines cannot see is common to all sequences; along
# axis 0 the map has three sequences, so no second 16-sequence tile exists there for the map itself -- the replay still sees dead_subtile on both
# axes because its single-step launch has B H W = 153 sequences.
FAULT_TABLE = {
    "k_swap": {"replay": "vh", "forget": "vh", "identical": ""},
    "row_tile": {"replay": "vh", "forget": "vh", "identical": ""},
    "dir_weights": {"replay": "vh", "forget": "vh", "identical": ""},
    "stale_h": {"replay": "vh", "forget": "vh", "identical": ""},
    "dead_subtile": {"replay": "vh", "forget": "h", "identical": "h"},
}


def fails(check):
    try:
        check()
    except AssertionError:
        return True
    return False


def test_the_fault_table_is_complete():
    assert set(FAULT_TABLE) == set(LM.FAULTS)
    for fault, row in FAULT_TABLE.items():
        assert set(row) == {"replay", "forget", "identical"}
        assert "".join(sorted(set(row["replay"] + row["identical"]))) == "hv", "%s: neither the replay nor the identical lines catch it on some axis" % fault
    for fault in ("k_swap", "row_tile", "dir_weights"):
        assert FAULT_TABLE[fault]["replay"] == "vh", fault


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("hid", [32, 96])
@pytest.mark.parametrize("fault", LM.FAULTS)
def test_every_planted_fault_is_caught_where_the_table_says(fault, hid, dtype):
    """every check against every faulty model on both axes: it fails exactly where FAULT_TABLE says.  The replay must fail for EVERY fed gate
    and both permutations where it is listed, and pass for every one where it is not."""
    m = model(fault)
    for axis, tag in ((0, "v"), (1, "h")):
        seen = {"replay": {fails(lambda: LM.replay_check(m, *MASK_MAP, hid, dtype, axis, gate, kind)) for gate in ("i", "g", "o") for kind in LM.KINDS},
                "forget": {fails(lambda: LM.forget_check(m, *MASK_MAP, hid, dtype, axis, kind)) for kind in LM.KINDS},
                "identical": {fails(lambda: LM.identical_check(m, *MASK_MAP, hid, dtype, axis))}}
        for check, outcomes in seen.items():
            assert outcomes == {tag in FAULT_TABLE[fault][check]}, (fault, check, "axis %d" % axis, outcomes)


def test_row_tile_is_no_fault_with_one_unit_tile():
    """hid 16 has one wave and one unit tile: the model with `row_tile` is the faultless model, bit for bit (why the table is held at hid 32, 96)"""
    xp, whh = operands(*MASK_MAP, 16, torch.bfloat16, 5)
    for axis in (0, 1):
        assert torch.equal(LM.scan_model(xp, whh, *MASK_MAP, 16, torch.bfloat16, axis, "row_tile").view(torch.int16),
                           LM.scan_model(xp, whh, *MASK_MAP, 16, torch.bfloat16, axis).view(torch.int16))


# ------------------------------------------------------------------ the cache contract on the host
def test_pack_aliasing_and_param_stamp():
    pkg = load_pkg()
    cfg = sequencer_config()
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
    assert {"s0.embed.w", "s3.embed.b", "s0.b0.ih.w", "s0.b0.ih.csum", "s1.b1.v.hh", "s1.b1.h.hh", "s2.b0.fc.w", "s1.b0.ff.fc1.csum", "head.w"} <= keys


# ------------------------------------------------------------------ what cannot run
def test_containers_and_cpu_inputs_raise(meta):
    add_tiny_settings(meta)
    m = SQ.Sequencer2D("tiny", num_classes=3).eval()
    blk = m.stages[0][1]
    x = torch.zeros(1, 8, 8, 32)
    for mod in (blk.model[0][0], blk.model[0][1], SQ.PreNormResidual(32, nn.Identity()), SQ.PatchEmbedOverlap(7, 7, 0, 32)):
        with pytest.raises(NotImplementedError, match="Sequencer2D"):
            mod(x)
    with pytest.raises(NotImplementedError, match="placeholder"):
        m.mlp_head[0](x)
    for mod, arg in ((m, torch.zeros(1, 3, 56, 56)), (blk, torch.zeros(1, 32, 8, 8)), (blk.model[0][0].fn[0], x), (SQ.BiLSTM2D(32, 16), x)):
        with pytest.raises(NotImplementedError):                # no CPU implementation, as for every family
            mod(arg)
    m.train()
    assert m.training and not hasattr(m, "_train_forward")
