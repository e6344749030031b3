"""CPU only: the host side of the cache contract, and the tables tests/test_gpu_lifecycle.py shares.

EngineModule keeps packed weights per (dtype, device) and re-derives them when `_param_stamp()` -- (data_ptr, _version) of every parameter
and buffer -- changes.  Nothing here launches a kernel: the models stay on the CPU and only the stamp and the cache dictionaries are read.
  * every update form torch's version counter or the tensor's identity records changes the stamp, on one model per family;
  * the stamp visits each entry of state_dict() exactly once (nested EngineModules included, no module walked twice);
  * the writes it cannot see (`p.data` in place) leave it unchanged -- that is the documented limit, pinned here so that the
    documentation and the code cannot drift apart -- and `invalidate_caches()` empties `_packs` / `_spaces` of the module and of every
    nested EngineModule and drops the module's entries of autograd._PACKS, and no other model's.

Configurations.  TINY: one entry per family from tests/golden/tiny_*.npz (built through test_gpu_models.build_from_tiny).  EVAL_ONLY: the
families without a train path, on the tiny configurations of their own fixtures -- WaveMLP-T (wave_mlp.npz's meta), RaftMLP ser_pm with the
gap=True and the gap=False head (raft_mlp.npz) and ActiveMLP s64 with widened offset biases (active_mlp.npz).  FUSED: the constructor kwargs
of tests/golden/train_grad_widths.npz -- benchmark widths at reduced depth -- with oracle.portable_init weights."""
import copy
import functools
import inspect
import json
import os
import re

import numpy as np
import pytest
import torch
from torch import nn

from conftest import GOLDEN, load_pkg
from oracle.portable_init import portable_input, portable_state_dict

TINY = ["mixer", "gmlp", "resmlp", "vip_weighted", "s2mlpv1", "s2mlpv2", "asmlp", "convmixer", "sparsemlp", "hiremlp", "msmlp", "swinmlp_ape",
        "cyclemlp"]
WAVE = "wavemlp"
EVAL_ONLY = [WAVE, "raftmlp", "raftmlp_nogap", "activemlp"]       # inference-only families: no train path
AT224 = "@224"                                     # suffix of the FUSED rows (tiny_s2mlpv2.npz and the benchmark S2-MLPv2 share a tag)
FUSED = [t + AT224 for t in ("mixer_b16", "gmlp_s", "resmlp_24", "vip_s7", "s2mlpv2", "asmlp_t", "convmixer_1536_20", "sparsemlp_t", "hiremlp_s",
                             "msmlp_t", "swinmlp_t", "cyclemlp_b1")]
BN_FAMILIES = {"convmixer", "sparsemlp", "convmixer_1536_20" + AT224, "sparsemlp_t" + AT224}       # train mode moves running statistics
HOLDS_BATCHNORM = BN_FAMILIES | {WAVE}             # the rows with a BatchNorm module (WaveMLP's never leaves eval mode)
_CACHE = {}


class Config:
    """One row of a table: `fresh()` constructs a new CPU instance in eval mode with the base weights (a COLD model once it is given
    a state_dict and moved to the GPU), `images(batch, seed)` seeded fp32 inputs of the configuration's resolution."""

    def __init__(self, name, ctor, kw, sd, hw, classes):
        self.name, self.ctor, self.kw, self.sd, self.hw, self.classes = name, ctor, kw, sd, hw, classes
        self._never_run = {}

    def fresh(self, sd=None, **override):
        """a new instance that has never run: constructed once per set of constructor overrides and kept untouched, then deep-copied
        (the constructors' random initialisation dominates the cost of a cold model; a copy of an instance that was never called holds
        no cache whatever EngineModule.__getstate__ does)"""
        key = tuple(sorted(override.items()))
        if key not in self._never_run:
            self._never_run[key] = self.ctor(**dict(self.kw, **override)).eval()
        m = copy.deepcopy(self._never_run[key])
        m.load_state_dict(self.sd if sd is None else sd, strict=True)
        return m

    def train_kw(self):
        """constructor overrides that switch the stochastic parts of train mode off (the same state_dict keys)"""
        names = inspect.signature(self.ctor).parameters
        return {k: 0.0 for k in ("drop_path_rate", "drop_rate", "dropout") if k in names}

    def images(self, batch, seed=0):
        return torch.from_numpy(portable_input((batch, 3) + tuple(self.hw), seed=1000 + seed)).float()


def config(name):
    if name in _CACHE:
        return _CACHE[name]
    pkg = load_pkg()
    if name == WAVE:
        meta = json.loads(str(np.load(os.path.join(GOLDEN, "wave_mlp.npz"))["meta"]))
        ctor, kw, hw, classes, seed = functools.partial(pkg.models_pytorch.WaveMLP, "T"), {"num_classes": 10}, tuple(meta["tiny_hw"]), 10, meta["tiny_seed"]
        sd = _portable(ctor(**kw), seed)
    elif name in ("raftmlp", "raftmlp_nogap"):
        meta = json.loads(str(np.load(os.path.join(GOLDEN, "raft_mlp.npz"))["meta"]))
        kw = dict(meta["tiny_cases"]["ser_pm" if name == "raftmlp" else "ser_pm_nogap"], num_classes=10)
        ctor, hw, classes = functools.partial(pkg.models_pytorch.RaftMLP, meta["tiny"]), (kw["image_size"],) * 2, 10
        sd = _portable(ctor(**kw), meta["tiny_seed"])
    elif name == "activemlp":
        from test_gpu_active import load_portable, widen           # the state test_gpu_active.tiny_model builds for its s64 case
        meta = json.loads(str(np.load(os.path.join(GOLDEN, "active_mlp.npz"))["meta"]))
        ctor, kw, hw, classes = pkg.models_pytorch.ActiveMLP, dict(meta["tiny"]), tuple(meta["tiny_cases"]["s64"]["size"]), meta["tiny"]["num_classes"]
        model = load_portable(ctor(**kw), meta["tiny_seed"])
        widen(model, meta, meta["tiny_seed"])                      # offset biases in [-3, 3): the sampler sees real offsets
        sd = {k: v.detach().clone() for k, v in model.state_dict().items()}
    elif name in FUSED:
        z = np.load(os.path.join(GOLDEN, "train_grad_widths.npz"))
        tag = name[:-len(AT224)]
        ctor, kw = getattr(pkg.models_pytorch, str(z[tag + "/ctor"])), json.loads(str(z[tag + "/kwargs"]))
        hw, classes = (224, 224), 1000
        sd = _portable(ctor(**kw), int(z[tag + "/seed"]))
    else:
        from test_gpu_models import build_from_tiny, ctor_for
        model, x, ref, kw, sd = build_from_tiny(pkg, name)
        ctor, hw, classes = ctor_for(pkg, name), tuple(x.shape[2:]), ref.shape[1]
    _CACHE[name] = Config(name, ctor, kw, sd, hw, classes)
    return _CACHE[name]


def _portable(model, seed):
    sd = portable_state_dict({k: tuple(v.shape) for k, v in model.state_dict().items()}, seed=seed)
    return {k: torch.from_numpy(v) for k, v in sd.items()}


def role(key):
    """the role of a state_dict entry: its name with the digits stripped"""
    return re.sub(r"\d+", "", key)


def one_per_role(model):
    """{role: key} -- the first entry of every distinct role (sampling one parameter per role; every role is kept)"""
    out = {}
    for k in model.state_dict():
        out.setdefault(role(k), k)
    return out


def noise_like(t, gen, scale=0.02):
    """a seeded perturbation of the same shape, dtype and device, |.| in [scale, 2 scale]: positive for a tensor that is positive
    throughout (a running variance stays one), of random sign otherwise (a shift of one sign on every weight of a deep model
    overflows); integer buffers (num_batches_tracked) move by one"""
    if not t.is_floating_point():
        return torch.ones_like(t)
    n = torch.rand(t.shape, generator=gen) * scale + scale
    if not bool((t > 0).all()):
        n = n * (torch.randint(0, 2, t.shape, generator=gen) * 2 - 1)
    return n.to(device=t.device, dtype=t.dtype)


def perturbed(sd, seed):
    gen = torch.Generator().manual_seed(seed)
    return {k: v + noise_like(v, gen) for k, v in sd.items()}


def owner_of(model, key):
    """(module, attribute name, is a buffer) of a state_dict key"""
    path, _, leaf = key.rpartition(".")
    mod = model.get_submodule(path) if path else model
    return mod, leaf, leaf in mod._buffers


# ------------------------------------------------------------------ update forms: each takes the model, returns nothing
def u_load_state_dict(m, gen):
    m.load_state_dict(perturbed({k: v.detach().clone() for k, v in m.state_dict().items()}, int(gen.initial_seed())), strict=True)


def u_no_grad_add(m, gen):
    with torch.no_grad():
        for t in m.state_dict(keep_vars=True).values():
            t.add_(noise_like(t, gen))


def u_data_assign(m, gen):
    for p in m.parameters():
        p.data = p.data + noise_like(p.data, gen)


def u_new_parameter(m, gen):
    for mod in m.modules():
        for k, p in list(mod._parameters.items()):
            if p is not None and k == "weight":
                setattr(mod, k, nn.Parameter(p.detach() + noise_like(p, gen)))


def u_half_update_float(m, gen):
    m.half()
    with torch.no_grad():
        for p in m.parameters():
            p.add_(noise_like(p, gen))
    m.float()


def u_data_inplace_then_invalidate(m, gen):
    for p in m.parameters():
        p.data.add_(noise_like(p.data, gen))                    # invisible to the stamp: `.data` has a version counter of its own
    m.invalidate_caches()


VISIBLE_UPDATES = [u_load_state_dict, u_no_grad_add, u_data_assign, u_new_parameter, u_half_update_float]


def u_optimizer(opt_ctor):
    """a train-mode backward on the CPU is not available (no CPU kernels): on the host an optimizer step with hand-set gradients"""
    def u(m, gen):
        params = [p for p in m.parameters()]
        for p in params:
            p.grad = noise_like(p, gen)
        opt_ctor(params).step()
    u.__name__ = "u_" + opt_ctor.__name__
    return u


def sgd(params):
    return torch.optim.SGD(params, lr=0.05)


def adamw(params):
    return torch.optim.AdamW(params, lr=0.01)


# ------------------------------------------------------------------ the host tests
HOST = TINY + EVAL_ONLY


@pytest.mark.parametrize("name", HOST)
def test_param_stamp_sees_every_visible_update_form(name):
    cfg = config(name)
    for upd in VISIBLE_UPDATES + [u_optimizer(sgd), u_optimizer(adamw)]:
        m = cfg.fresh()
        before = m._param_stamp()
        assert m._param_stamp() == before, "the stamp of an untouched model moved"
        upd(m, torch.Generator().manual_seed(5))
        assert m._param_stamp() != before, (name, upd.__name__)
    # ... moving BatchNorm's running statistics the way a train-mode forward does (in-place writes to buffers under no_grad)
    m = cfg.fresh()
    bns = [b for b in m.modules() if isinstance(b, nn.modules.batchnorm._BatchNorm)]
    assert bool(bns) == (name in HOLDS_BATCHNORM), name
    if bns:
        before = m._param_stamp()
        with torch.no_grad():
            bns[-1].running_mean.mul_(0.9)
        assert m._param_stamp() != before


@pytest.mark.parametrize("name", HOST)
def test_param_stamp_changes_for_every_single_entry(name):
    """one parameter or buffer at a time -- EVERY entry of the state_dict, not one per role: a module the walk skipped would show here"""
    m = config(name).fresh()
    gen = torch.Generator().manual_seed(9)
    for key, t in m.state_dict(keep_vars=True).items():
        before = m._param_stamp()
        with torch.no_grad():
            t.add_(noise_like(t, gen))
        assert m._param_stamp() != before, (name, key)


@pytest.mark.parametrize("name", HOST + FUSED)
def test_param_stamp_visits_each_state_dict_entry_exactly_once(name):
    m = config(name).fresh()
    want = sorted((t.data_ptr(), t._version) for t in m.state_dict(keep_vars=True).values())
    assert sorted(m._param_stamp()) == want, name
    assert len({p for p, _ in want}) == len(want), "two entries of the state_dict share storage: the comparison above would not count them"


def test_param_stamp_with_a_shared_module_and_a_nested_engine_module(pkg):
    """a module reachable on two paths is walked once (state_dict lists it under both names, the stamp once); an EngineModule nested in
    another contributes its parameters to the outer stamp"""
    mp = pkg.models_pytorch
    inner = mp.res_mlp.Aff(8)
    outer = mp.res_mlp.Aff(8)
    outer.first, outer.again = inner, inner
    stamp = outer._param_stamp()
    assert len(stamp) == 4 and len(outer.state_dict()) == 6
    assert sorted(p for p, _ in stamp) == sorted(t.data_ptr() for t in (outer.alpha, outer.beta, inner.alpha, inner.beta))
    before = outer._param_stamp()
    with torch.no_grad():
        inner.beta.add_(1.0)
    assert outer._param_stamp() != before


@pytest.mark.parametrize("name", ["mixer", "hiremlp"])
def test_data_inplace_writes_are_invisible_to_the_stamp(name):
    """the documented limit: `p.data` carries a version counter of its own, so these writes need
    invalidate_caches().  If torch ever makes them visible this test fails and the documentation can be relaxed."""
    m = config(name).fresh()
    before = m._param_stamp()
    p = next(m.parameters())
    p.data.mul_(2.0)
    p.data -= 0.1 * torch.ones_like(p)
    assert m._param_stamp() == before


def _span(t):
    s = t.untyped_storage()
    return s.data_ptr(), s.data_ptr() + s.nbytes()


@pytest.mark.parametrize("name,dtype", [(n, d) for n in HOST for d in ("fp32", "bf16")] + [(n, "bf16") for n in FUSED])
def test_no_eval_pack_tensor_aliases_a_parameter(pkg, name, dtype):
    """a forward reads packed weights only (streams): an in-place parameter update must not reach a forward that
    is still queued on another stream, so no tensor of `_pack`'s result may share storage with a parameter or buffer -- fp32 is the
    likely miss, where `.to(float32)` / `.reshape` / `.contiguous()` of a parameter are views.  Packed on the CPU: the packing is plain
    torch, and the aliasing does not depend on the device.  engine.pack_tensors (what _get_pack hands to record_stream) is held to the
    same walk: every leaf is a tensor, a plain number or None."""
    E = pkg.engine
    m = config(name).fresh()
    with torch.no_grad():
        pk = m._pack({"fp32": torch.float32, "bf16": torch.bfloat16}[dtype], torch.device("cpu"))
    leaves, stack = [], [pk]
    while stack:
        v = stack.pop()
        if isinstance(v, dict):
            stack.extend(v.values())
        elif isinstance(v, (tuple, list)):
            stack.extend(v)
        else:
            assert v is None or torch.is_tensor(v) or isinstance(v, (int, float, bool, str)), (name, type(v).__name__, "engine.pack_tensors does not walk this")
            if torch.is_tensor(v):
                leaves.append(v)
    assert len(leaves) >= 4
    own = {k: _span(t) for k, t in m.state_dict(keep_vars=True).items()}
    for t in leaves:
        lo, hi = _span(t)
        shared = [k for k, (a, b) in own.items() if not (b <= lo or hi <= a)]
        assert not shared, (name, dtype, tuple(t.shape), "a pack tensor aliases", shared)


def _fill_caches(pkg, m, marker):
    """what a forward leaves behind, without a launch: an entry in _packs and _spaces of every EngineModule of the tree"""
    E = pkg.engine
    mods = [x for x in m.modules() if isinstance(x, E.EngineModule)]
    for x in mods:
        x._packs[(torch.float32, "cpu")] = (x._param_stamp(), {"w": marker})
        x._spaces[(2, None, torch.float32, "cpu", 0)] = E.Workspace("cpu", torch.float32)
    return mods


@pytest.mark.parametrize("name", ["mixer", "resmlp", "hiremlp", "msmlp", WAVE, "raftmlp", "activemlp"])
def test_invalidate_caches_empties_the_module_tree_and_its_train_packs(pkg, name):
    E, AG = pkg.engine, importlib_autograd(pkg)
    cfg = config(name)
    m, other = cfg.fresh(), cfg.fresh()
    mods = _fill_caches(pkg, m, torch.zeros(1))
    omods = _fill_caches(pkg, other, torch.zeros(1))
    assert len(mods) > 1 or name in ("gmlp",), "the configuration has no nested EngineModule: pick another"
    saved = dict(AG._PACKS)
    try:
        AG._PACKS.clear()
        for model in (m, other):
            for p in model.parameters():
                if p.dim() >= 2:
                    AG._packed(p, p.reshape(p.shape[0], -1), torch.float32, torch.device("cpu"))
        mine = {id(p) for p in m.parameters()}
        n_mine = sum(k[0] in mine for k in AG._PACKS)
        n_other = len(AG._PACKS) - n_mine
        assert n_mine > 0 and n_other > 0
        assert m.invalidate_caches() is m
        assert all(not x._packs and not x._spaces for x in mods)
        assert all(x._packs and x._spaces for x in omods), "another model's caches were dropped"
        assert sum(k[0] in mine for k in AG._PACKS) == 0 and len(AG._PACKS) == n_other
    finally:
        AG._PACKS.clear()
        AG._PACKS.update(saved)


def importlib_autograd(pkg):
    import importlib
    return importlib.import_module(pkg.__name__ + ".autograd")


@pytest.mark.parametrize("name", ["mixer", "hiremlp", "raftmlp", "activemlp"])
def test_copies_and_pickles_travel_without_the_caches(pkg, name):
    """copy.deepcopy and torch.save(model) carry parameters, buffers and settings, not packed weights or workspaces; the original keeps
    its own; the block -> backbone links of the copy point into the copy"""
    import copy
    import io
    E = pkg.engine
    m = config(name).fresh().set_compute_dtype(torch.bfloat16)
    mods = _fill_caches(pkg, m, torch.zeros(1))
    buf = io.BytesIO()
    torch.save(m, buf)
    buf.seek(0)
    for c in (copy.deepcopy(m), torch.load(buf, weights_only=False)):
        cm = [x for x in c.modules() if isinstance(x, E.EngineModule)]
        assert len(cm) == len(mods) and all(x._packs == {} and x._spaces == {} for x in cm)
        assert all(x._packs and x._spaces for x in mods)
        assert c._compute_dtype == torch.bfloat16 and not c.training
        assert all(torch.equal(a, b) and a.data_ptr() != b.data_ptr() for a, b in zip(m.state_dict().values(), c.state_dict().values()))
        mine = {id(x) for x in c.modules()}
        owners = [x.__dict__["_owner"][0] for x in c.modules() if "_owner" in x.__dict__]
        assert all(id(o) in mine for o in owners)
        assert (name != "hiremlp") or owners
