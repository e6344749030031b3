"""No GPU: the case table of test_gpu_autograd_functions.py names every torch.autograd.Function of autograd.py, every restatement runs and
differentiates on the CPU, and every case can tell a wrong derivative from a right one: a restatement with one plausible fault lies at least five
gates from the true one (where the gate is "bit-exact": at least five roundings of the storage type)."""
import inspect

import pytest
import torch

import autograd_cases as T


def functions():
    ag = T.AG()
    return {n for n, v in vars(ag).items() if inspect.isclass(v) and issubclass(v, torch.autograd.Function) and v.__module__ == ag.__name__}


def test_the_table_names_every_function_of_autograd_py():
    have = functions()
    named = {c.fn for c in T.CASES}
    assert len(have) == 27, sorted(have)
    assert have - named == set(), "autograd.Function without a case in tests/autograd_cases.py: %s" % sorted(have - named)
    assert named - have == set(), sorted(named - have)
    for c in T.CASES:
        assert (c.ref is not None) != (c.values is not None), c.name              # a restatement here, or the name of the test that holds one
    direct = {c.fn for c in T.CASES if c.ref is None}
    assert direct == {"Linear", "Gelu", "LayerNorm", "DepthwiseConv", "GroupNorm1", "BatchNormTrain", "Dropout"}, sorted(direct)


def test_every_backward_is_once_differentiable():
    """the decorator's wrapper (torch/autograd/function.py) stands in front of the function: a backward without it would hand create_graph=True
    gradients without a graph"""
    ag = T.AG()
    for n in sorted(functions()):
        bw = getattr(ag, n).backward
        assert getattr(bw, "__wrapped__", None) is not None and bw.__code__.co_filename.endswith("function.py"), n


def test_operands_are_pairwise_distinct_in_every_storage_type():
    for dt in T.DTYPES:
        v = T.distinct((72, 70), dt, 1)
        assert v.dtype == dt and torch.unique(v.float()).numel() == v.numel()


@pytest.mark.parametrize("case,dtype", T.VALUE_CASES, ids=T.ids(T.VALUE_CASES))
def test_a_faulty_restatement_lies_five_gates_away(case, dtype):
    args = case.build(dtype, "cpu")
    a64 = [v.double() if torch.is_tensor(v) else v for v in args]
    with torch.no_grad():
        out = (case.ref_fwd or case.ref)(dtype, *a64)
    dy = T.cotangent(case, dtype, out.shape)
    true = T.evaluate(case, dtype, args, dy)
    gate = T.gates(case, dtype, args, dy, true)
    assert all(torch.isfinite(v).all() for v in true.values())
    assert case.faults, case.name
    for fault in case.faults:
        wrong = fault(case, dtype, a64, dy.double(), true)
        assert wrong, fault.__name__
        ratios = {}
        for name, w in wrong.items():
            if name not in gate:                                                  # a result this case does not check
                continue
            sdt = torch.float32 if case.fn == "SoftmaxBranches" else dtype
            g = gate[name] if gate[name] is not None else T.EPS[sdt] * true[name].abs() + T.TINY[sdt]
            ratios[name] = ((w - true[name]).abs() / g.clamp_min(1e-300)).max().item()
        # the faulty restatement as a whole: its worst result (a dropped term leaves the other gradients as they are)
        assert ratios and max(ratios.values()) >= 5.0, (case.name, fault.__name__, ratios)
