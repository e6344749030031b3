"""CPU checks of WaveMLP: the module tree and constructor contract of the reference's wave_mlp.py (tests/golden/wave_mlp.npz, made by
tests/golden/make_wave_golden.py from the reference itself), and the argument checks of mlpk_wave_patm, which return before anything touches
a device."""
import json
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN, ROOT, load_pkg

FIX = os.path.join(GOLDEN, "wave_mlp.npz")


def models_pytorch():
    return load_pkg().models_pytorch


@pytest.mark.parametrize("name", ["T", "S", "M"])
def test_state_dict_table_matches_reference(name):
    want = json.loads(str(np.load(FIX)["shapes/" + name]))
    got = {k: list(v.shape) for k, v in models_pytorch().WaveMLP(name).state_dict().items()}
    assert list(got) == list(want)
    assert got == want


def test_import_and_export():
    pkg = load_pkg()
    mp = pkg.models_pytorch
    assert "WaveMLP" in mp.__all__
    assert pkg.WaveMLP is mp.WaveMLP                        # `from models_pytorch import *` re-exported at the package level


def test_bad_model_name_message():
    with pytest.raises(AssertionError) as e:
        models_pytorch().WaveMLP("X")
    assert str(e.value) == "WaveMLP model name should be in ['T', 'S', 'M']"


def test_settings_and_defaults():
    mp = models_pytorch()
    wm = mp.wave_mlp
    assert wm.wavemlp_settings == {'T': [[2, 2, 4, 2], [4, 4, 4, 4]], 'S': [[2, 3, 10, 3], [4, 4, 4, 4]], 'M': [[3, 4, 18, 3], [8, 8, 4, 4]]}
    m = mp.WaveMLP()
    assert m.head.out_features == 1000 and m.out_indices == [0, 2, 4, 6]
    assert float(m.head.weight.detach().abs().max()) == 0.0 and float(m.head.bias.detach().abs().max()) == 0.0      # the head starts at zero
    assert isinstance(m.network[1], wm.Downsample) and len(m.network) == 7
    blk = m.network[6][1]
    assert isinstance(blk, wm.Block) and blk.mlp.fc1.out_channels == 2048
    assert tuple(blk.attn.tfc_h.weight.shape) == (512, 2, 1, 7) and tuple(blk.attn.tfc_w.weight.shape) == (512, 2, 7, 1)


def test_pretrained_checkpoint(tmp_path):
    mp = models_pytorch()
    src = mp.WaveMLP("T", num_classes=7)
    with torch.no_grad():
        for p in src.parameters():
            p.uniform_(-1, 1)
    path = tmp_path / "ckpt.pth"
    torch.save({"model": src.state_dict()}, str(path))
    dst = mp.WaveMLP("T", pretrained=str(path), num_classes=7)
    for (k, a), (k2, b) in zip(src.state_dict().items(), dst.state_dict().items()):
        assert k == k2 and torch.equal(a, b)


def test_return_features_raises_like_reference():
    with pytest.raises(AttributeError, match="norm0"):
        models_pytorch().WaveMLP("T").return_features(torch.zeros(1, 3, 32, 32))


def test_containers_and_cpu_inputs_raise():
    mp = models_pytorch()
    m = mp.WaveMLP("T", num_classes=4).eval()
    with pytest.raises(NotImplementedError, match="WaveMLP"):
        m.patch_embed(torch.zeros(1, 3, 32, 32))
    with pytest.raises(NotImplementedError, match="WaveMLP"):
        m.network[1](torch.zeros(1, 64, 8, 8))
    for mod, x in ((m, torch.zeros(1, 3, 32, 32)), (m.network[0][0], torch.zeros(1, 64, 8, 8)), (m.network[0][0].attn, torch.zeros(1, 64, 8, 8))):
        with pytest.raises(NotImplementedError):            # no CPU implementation, as for every family
            mod(x)


def test_wave_patm_declared_and_exported_at_abi_14():
    N = load_pkg()._native
    assert "mlpk_wave_patm" in N.PROTOTYPES and "mlpk_wave_patm_supported" in N.PROTOTYPES
    with open(os.path.join(ROOT, "include", "mlpk.h")) as f:
        h = f.read()
    assert "int mlpk_wave_patm(" in h and "int mlpk_wave_patm_supported(" in h
    lib = N.lib()                                           # every PROTOTYPES entry resolved, ABI checked
    assert lib.mlpk_abi_version() == 14


def test_wave_patm_argument_errors():
    N = load_pkg()._native
    lib = N.lib()
    P = 1 << 20                                             # a 16-byte aligned address that is never dereferenced: every call below fails its checks
    C = 64

    def call(dtype=N.BF16, y=P, ldy=5 * C, wh=P, ww=P, oh=P, ow=P, ldo=2 * C, B=2, H=7, W=7, C=C):
        return lib.mlpk_wave_patm(dtype, y, ldy, wh, ww, oh, ow, ldo, B, H, W, C, None)
    ENULL, EDTYPE, ESHAPE, EALIGN = -4, -1, -2, -3
    for kw in ({"y": None}, {"wh": None}, {"ww": None}, {"oh": None}, {"ow": None}):
        assert call(**kw) == ENULL, kw
    assert call(dtype=7) == EDTYPE
    assert call(ldy=5 * C - 4) == ESHAPE                   # ldy < 5C
    assert call(ldo=C - 2) == ESHAPE
    assert call(C=6, ldy=32, ldo=8) == ESHAPE              # C % 4 != 0: not taken
    assert call(C=0) == ESHAPE and call(B=0) == ESHAPE and call(H=-1) == ESHAPE and call(W=0) == ESHAPE
    assert call(y=P + 2) == EALIGN and call(ldy=5 * C + 2) == EALIGN and call(oh=P + 2) == EALIGN and call(ldo=2 * C + 1) == EALIGN
    assert call(dtype=N.F32, y=P + 8) == EALIGN            # fp32: 4-element (16-byte) loads
    assert lib.mlpk_wave_patm_supported(N.BF16, 2, 7, 7, 64) == 1 and lib.mlpk_wave_patm_supported(N.F32, 1, 1, 1, 40) == 1
    assert lib.mlpk_wave_patm_supported(N.BF16, 2, 7, 7, 6) == 0 and lib.mlpk_wave_patm_supported(9, 2, 7, 7, 64) == 0
