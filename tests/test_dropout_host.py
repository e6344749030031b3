"""CPU checks of the Dropout generator: tests/philox_ref.py (the numpy restatement the GPU tests and the fixture generator use) and
csrc/mlpk_philox.h (the code mlpk_dropout runs, compiled here for the host) against the published Philox4x32-10 known-answer vectors and
against each other -- including element indices past 2^34, whose counters have a non-zero high word that no GPU tensor here reaches."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

import philox_ref as P
from conftest import ROOT

CSRC = os.path.join(ROOT, "jittor-mlp_amd", "csrc")

# Random123's kat_vectors for philox4x32_10: (counter, key, expected)
KAT = [((0x00000000, 0x00000000, 0x00000000, 0x00000000), (0x00000000, 0x00000000), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
       ((0xffffffff, 0xffffffff, 0xffffffff, 0xffffffff), (0xffffffff, 0xffffffff), (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
       ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]

SHIM = r"""
#include "mlpk_philox.h"
extern "C" void kat(const uint32_t* c, const uint32_t* k, uint32_t* out) {
    const mlpk::philox4 r = mlpk::philox4x32_10(c[0], c[1], c[2], c[3], k[0], k[1]);
    for (int i = 0; i < 4; ++i) out[i] = r.v[i];
}
extern "C" void words(uint64_t seed, uint32_t site, const uint64_t* e, int n, uint32_t* out) {
    for (int i = 0; i < n; ++i) out[i] = mlpk::dropout_words(seed, site, e[i] >> 2).v[e[i] & 3];
}
"""


@pytest.fixture(scope="module")
def host_philox(tmp_path_factory):
    cxx = next((c for c in (os.environ.get("CXX"), "c++", "g++", "clang++", "/opt/rocm/lib/llvm/bin/clang++") if c and shutil.which(c)), None)
    assert cxx, "no host C++ compiler found"
    d = tmp_path_factory.mktemp("philox")
    src, lib = d / "shim.cpp", d / "libphilox_host.so"
    src.write_text(SHIM)
    r = subprocess.run([cxx, "-O2", "-std=c++17", "-shared", "-fPIC", "-I", CSRC, str(src), "-o", str(lib)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    h = ctypes.CDLL(str(lib))
    h.kat.argtypes = [ctypes.c_void_p] * 3
    h.words.argtypes = [ctypes.c_uint64, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p]
    return h


def test_numpy_philox_known_answers():
    for ctr, key, want in KAT:
        got = P.philox4x32_10(np.array([ctr], dtype=np.uint32), key)[0]
        assert tuple(int(v) for v in got) == want, (ctr, key)


def test_header_philox_known_answers(host_philox):
    for ctr, key, want in KAT:
        c, k, out = np.array(ctr, np.uint32), np.array(key, np.uint32), np.zeros(4, np.uint32)
        host_philox.kat(c.ctypes.data, k.ctypes.data, out.ctypes.data)
        assert tuple(int(v) for v in out) == want, (ctr, key)


@pytest.mark.parametrize("seed,site", [(0, 0), (1, 7), (0x0123456789ABCDEF, 3), (2 ** 63 - 2, 0xFFFFFFFF)])
def test_header_dropout_words_match_numpy(host_philox, seed, site):
    rng = np.random.default_rng(seed & 0xFFFF)
    e = np.concatenate([np.arange(64), rng.integers(0, 2 ** 31, 256), rng.integers(2 ** 34, 2 ** 62, 256),  # counters with a non-zero high word
                        [2 ** 34 - 1, 2 ** 34, 2 ** 34 + 1, 2 ** 34 + 3, 2 ** 62 - 1]]).astype(np.uint64)
    out = np.zeros(e.shape, np.uint32)
    host_philox.words(seed, site, e.ctypes.data, len(e), out.ctypes.data)
    assert np.array_equal(out, P.dropout_words(seed, site, e))
    # the high word of the counter matters: e and e + 2^34 (same low word of e >> 2) draw different words
    lo = np.arange(16, dtype=np.uint64)
    a, b = P.dropout_words(seed, site, lo), P.dropout_words(seed, site, lo + np.uint64(2 ** 34))
    assert (a != b).mean() > 0.9


def test_keep_rule_edges():
    assert P.threshold(0.0) == 0 and P.threshold(1.0) == 2 ** 32 and P.threshold(0.5) == 2 ** 31
    m = P.keep_mask(5, 0, 0.0, 3, 8)
    assert m.all()
    assert not P.keep_mask(5, 0, 1.0, 3, 8).any()
    frac = P.keep_mask(11, 2, 0.25, 256, 256).mean()
    assert abs(frac - 0.75) < 6 * np.sqrt(0.25 * 0.75 / 65536)
    assert P.scale(0.25) == np.float32(1.0 / 0.75)
