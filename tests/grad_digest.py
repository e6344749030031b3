"""What tests/golden/train_grad_widths.npz keeps of a gradient, computed the same way by its generator (make_train_widths_golden.py) and by
tests/test_gpu_train_widths.py.

Of every tensor: SAMPLES entries at evenly spaced flat indices (all of them up to SAMPLES), its max |g|, its L2 norm and NPROJ projections
<g, r_i> on seeded +-1 directions (oracle.portable_init.portable_signs, regenerated on both sides).  The samples pin single entries; the
projections make every entry count, so a wrong tail or a wrong index between the samples still moves them.  For an error e, E <e, r_i>^2 =
|e|^2: the mean square of the projection differences is an unbiased estimate of the squared L2 norm of the whole error.  Keeping the tensors of up to 4096 entries whole instead would take 1.2 MB over the twelve families."""
import numpy as np

from oracle.portable_init import portable_signs

SAMPLES = 64
NPROJ = 8
PROJ_SEED = 29


def projections(name, g):
    """<g, r_i>, i < NPROJ, in fp64, for the flattened gradient g of the parameter `name`"""
    g = np.asarray(g, dtype=np.float64).reshape(-1)
    return portable_signs("proj/" + name, g.size, NPROJ, PROJ_SEED) @ g


def sample_index(n):
    """the flat indices kept of an n-entry tensor"""
    if n <= SAMPLES:
        return np.arange(n, dtype=np.int64)
    return np.unique(np.linspace(0, n - 1, SAMPLES).round().astype(np.int64))


def digest(name, g):
    """(kept entries, [max |g|, L2 norm, NPROJ projections]) of a tensor, fp64"""
    g = np.asarray(g, dtype=np.float64).reshape(-1)
    return g[sample_index(g.size)], np.concatenate([[np.abs(g).max(), np.linalg.norm(g)], projections(name, g)])
