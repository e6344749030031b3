"""Exact-integer operand sets for the matrix-core kernels, and the checks that wrap every use of them.

Operands are small integers (or dyadic fractions), so every product and every partial sum is exact in fp32 IN ANY SUMMATION
ORDER, and the value after the whole epilogue is exactly representable in the storage type.  The mathematically exact result
is then the only admissible output of a kernel, whatever its tile, K order or pipeline: the gate is torch.equal, and a
mismatch names the element (and, with the one-hot pattern, the K index and the source row).

Three patterns (gemm_case):
  onehot   row n of B is a single 1 at k = n mod K; A[m, k] is a code of (m, k); C[m, n] = A[m, n mod K]
  ternary  sparse entries from {-2 .. 2}; every k weighs in some output, every output holds a non-zero term from every K slab
  cancel   a block of power-of-two entries drives |acc| past 2^12 (exact in fp32, far outside the 16-bit integer range); the
           fp32 bias (or cshift) brings the stored value back to a small integer: 16-bit accumulation, or a rounding before
           the bias, changes the result.  The cancellation goes through the fp32 vectors, never through R (several paths
           round before the residual by design).

Everything here runs on the CPU in float64; the GPU tests move a case's tensors to the device in the storage type."""
import os
import re
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# largest n such that every integer |v| <= n is exact in the type (2^(mantissa bits + 1))
INT_RANGE = {torch.bfloat16: 256, torch.float16: 2048, torch.float32: 1 << 24}
ACC_LIMIT = float(1 << 24)          # sum of |terms| of an fp32 accumulator stays below this: exact in any order
# From this integer on all three GELU forms of csrc/mlpk_common.h return x itself after the rounding to the storage type
# (tests/test_exact_host.py derives it from emulations of the three forms; tests/test_gpu_exact.py checks it on the device).
GELU_THRESHOLD = 8
GELU_OFFSET = {torch.bfloat16: 132.0, torch.float16: 132.0, torch.float32: 132.0}     # centre of [threshold, 256]
PATTERNS = ("onehot", "ternary", "cancel")
CANCEL_BIG = 64.0                   # the block's entries: 64 * 64 = 2^12 per product


def epc_of(dtype):
    """elements of a 16-byte chunk"""
    return 4 if dtype == torch.float32 else 8


def slab_of(dtype):
    """the finest K slab any kernel stages: 64 bytes (every coarser slab is a union of these)"""
    return 4 * epc_of(dtype)


def representable(t, dtype):
    t = t.double()
    return bool(torch.equal(t.to(dtype).double(), t))


# ------------------------------------------------------------------------------------------------- operand patterns
def onehot_operands(M, N, K, k_off=0):
    """A[m, k] in +-[1, 7] (a code of both indices: neighbours in m and in k differ), B[n, :] = e_((n + k_off) mod K)"""
    m = torch.arange(M, dtype=torch.int64)[:, None]
    k = torch.arange(K, dtype=torch.int64)[None, :]
    code = 1 + (3 * m + 5 * k + (m // 7) + (k // 7)) % 7
    A = (code * (1 - 2 * ((m + k) % 2))).double()
    B = torch.zeros((N, K), dtype=torch.float64)
    B[torch.arange(N), (torch.arange(N) + k_off) % K] = 1.0
    return A, B


def _forced_positions(K, slab):
    """one k per K slab (the last slab may be short)"""
    out = []
    for j, k0 in enumerate(range(0, K, slab)):
        out.append(k0 + (3 * j + 1) % min(slab, K - k0))
    return out


def ternary_operands(M, N, K, slab, seed, density=None):
    """Sparse {-2 .. 2}.  In every slab one position holds a non-zero in EVERY row of A and of B (signs alternate from slab to slab
    so that the forced terms cancel in pairs); the rest is seeded and sparse; a k without any weight gets one."""
    g = torch.Generator().manual_seed(seed)
    if density is None:
        density = min(1.0 / 12, K ** -0.5)               # about one seeded product term per output at long K: sums stay small

    def sparse(rows):
        mag = torch.randint(1, 3, (rows, K), generator=g).double()
        sgn = torch.randint(0, 2, (rows, K), generator=g).double() * 2 - 1
        keep = (torch.rand((rows, K), generator=g) < density).double()
        return mag * sgn * keep
    A, B = sparse(M), sparse(N)
    m = torch.arange(M, dtype=torch.int64)
    n = torch.arange(N, dtype=torch.int64)
    for j, k in enumerate(_forced_positions(K, slab)):
        # signs + + - - of A and + - - + of B: the products alternate, and neither operand's row sums grow with K
        A[:, k] = (1 + (m + j // 2) % 2).double() * (1 - 2 * ((j // 2) % 2))
        B[:, k] = (1 + (n + j // 2) % 2).double() * (1 - 2 * (((j + 1) // 2) % 2))
    for T, rows in ((A, M), (B, N)):                     # every k has a non-zero weight in some output
        ks = (~(T != 0).any(0)).nonzero().flatten()
        T[ks % rows, ks] = (1 - 2 * (ks % 2)).double()
    return A, B


def cancel_operands(M, N, K, dtype, seed):
    """Block = the first 16-byte chunk of K: A = B = 64 there, except k = 0 with A[m, 0] = 64 + m % 4 and B[n, 0] = 1, so that the
    block sums to (blk - 1) 2^12 + 64 + m % 4 -- odd values far beyond the 16-bit integer range.  The rest of K is ternary.
    Returns A, B and the n-independent part of the block sum, which the caller's bias takes away."""
    blk = epc_of(dtype)
    assert K >= blk
    if K > blk:
        A, B = ternary_operands(M, N, K, slab_of(dtype), seed)
    else:
        A, B = torch.zeros((M, K), dtype=torch.float64), torch.zeros((N, K), dtype=torch.float64)
    A[:, :blk] = CANCEL_BIG
    B[:, :blk] = CANCEL_BIG
    A[:, 0] = CANCEL_BIG + (torch.arange(M) % 4).double()
    B[:, 0] = 1.0
    return A, B, (blk - 1) * CANCEL_BIG * CANCEL_BIG + CANCEL_BIG


# ------------------------------------------------------------------------------------------------- one GEMM case
def gemm_case(pattern, dtype, M, N, K, *, seed=1, bias=True, affine=False, res=0, r_alias=False, rperiod=0, ln_group=0, gelu=False,
              t_rows=0, t_tokens=0, ldr_extra=0, k_off=0, slab=None):
    """Operands, epilogue vectors and the exact result of one mlpk_gemm_nt-shaped product (mlpk.h):
         v = (acc - mean[m / g] csum[n]) rstd[m / g] + bias[n];  gelu;  v cscale[n] + cshift[n];  v rscale[m % period];  (+|*) R
    All fields are float64 CPU tensors (None where unused).  t_rows > 0: token-transposed output, `want` is (images, N, t_rows).
    res: 0 none, 1 add, 2 multiply.  gelu: the pre-activations are integers in [GELU_THRESHOLD, 256], where the GELU is the identity."""
    assert pattern in PATTERNS
    c = types.SimpleNamespace(pattern=pattern, dtype=dtype, M=M, N=N, K=K, res=res, r_alias=r_alias, gelu=gelu, t_rows=t_rows,
                              t_tokens=t_tokens or N, rperiod=rperiod, ln_group=ln_group, bias=None, cscale=None, cshift=None, rscale=None,
                              ln=None, R=None, big=None, k_off=k_off, slab=slab or slab_of(dtype))
    n = torch.arange(N, dtype=torch.int64)
    m = torch.arange(M, dtype=torch.int64)
    block = 0.0
    if pattern == "onehot":
        c.A, c.B = onehot_operands(M, N, K, k_off)
    elif pattern == "ternary":
        c.A, c.B = ternary_operands(M, N, K, c.slab, seed)
    else:
        c.A, c.B, block = cancel_operands(M, N, K, dtype, seed)
    acc = c.A @ c.B.t()
    c.acc = acc
    c.abs_terms = [c.A.abs() @ c.B.abs().t()]
    v = acc
    if ln_group:
        # folded LayerNorm: integer means, power-of-two rstd, the exact row sums of B.  The cancel pattern keeps mean = 0 and rstd = 1:
        # its block is cancelled by bias[n], and a per-row factor in front of it could not be.
        ns = (M + ln_group - 1) // ln_group
        s = torch.arange(ns, dtype=torch.int64)
        mean = ((s * 3) % (3 if gelu else 4) - 1).double() if pattern != "cancel" else torch.zeros(ns, dtype=torch.float64)
        rstd = torch.tensor([1.0, 2.0, 1.0 if gelu else 0.5, 1.0])[s % 4].double() if pattern != "cancel" else torch.ones(ns, dtype=torch.float64)
        csum = c.B.sum(1)
        c.ln = (mean, rstd, csum)
        idx = m // ln_group
        c.abs_terms.append(c.abs_terms[0] + mean.abs()[idx][:, None] * csum.abs()[None, :])
        v = (acc - mean[idx][:, None] * csum[None, :]) * rstd[idx][:, None]
    use_shift_to_cancel = pattern == "cancel" and affine and not gelu         # the block goes through cshift instead of the bias
    offset = GELU_OFFSET[dtype] if gelu else 0.0
    if bias or gelu or (pattern == "cancel" and not use_shift_to_cancel):
        small = ((n * 5) % 7 - 3).double()                                    # neighbours differ: an index off by one shows
        c.bias = small + offset - (0.0 if use_shift_to_cancel else block)
        v = v + c.bias[None, :]
    c.pre_act = v if gelu else None                                           # identity on integers >= GELU_THRESHOLD
    if affine:
        # (behind a GELU the scale stays 1 and the shift small: the f16 form returns x (1 - 3.4e-6), which rounds to x where it is
        #  stored, but taking the offset of 132 away again in fp32 would leave that 4.5e-4 standing next to a small integer)
        c.cscale = torch.ones(N, dtype=torch.float64) if (gelu or use_shift_to_cancel) else torch.tensor([1.0, 2.0])[n % 2].double()
        c.cshift = ((n * 3) % 5 - 2).double() - (block if use_shift_to_cancel else 0.0)
        v = v * c.cscale[None, :] + c.cshift[None, :]
    if rperiod:
        r = torch.arange(rperiod, dtype=torch.int64)
        c.rscale = torch.tensor([1.0, 2.0, 1.0, 0.5])[r % 4].double()
        v = v * c.rscale[m % rperiod][:, None]
    c.big = acc.abs().max().item()
    if t_rows:
        assert M % t_rows == 0
        nimg = M // t_rows
        v = v.reshape(nimg, t_rows, N).permute(0, 2, 1).contiguous()          # (image, token n, channel)
    c.pre_res = v
    if res:
        g = torch.Generator().manual_seed(seed + 77)
        lim = 4 if res == 1 else 2
        if t_rows:
            c.ldr = t_rows + ldr_extra
            c.R = torch.randint(-lim, lim + 1, (nimg * c.t_tokens, c.ldr), generator=g).double()
            r = c.R.reshape(nimg, c.t_tokens, c.ldr)[:, :N, :t_rows]
        else:
            c.ldr = N + ldr_extra
            c.R = torch.randint(-lim, lim + 1, (M, c.ldr), generator=g).double()
            r = c.R[:, :N]
        v = v + r if res == 1 else v * r
    c.want = v
    return c


def check_case(c):
    """The premises, asserted before any comparison: every stored tensor is exact in the storage type (operands, the value before the
    residual -- some paths round there -- and the result), every accumulator's sum of |terms| is below 2^24, saturated GELU inputs
    are integers in [GELU_THRESHOLD, 256], and the cancel pattern's accumulator really leaves the storage type's integer range."""
    what = (c.pattern, str(c.dtype), c.M, c.N, c.K)
    for name in ("A", "B", "R", "pre_res", "want"):
        t = getattr(c, name)
        if t is not None:
            assert representable(t, c.dtype), (what, name, "not exact in the storage type")
    for name in ("bias", "cscale", "cshift", "rscale"):
        t = getattr(c, name)
        if t is not None:
            assert representable(t, torch.float32), (what, name)
    if c.ln is not None:
        for t in c.ln:
            assert representable(t, torch.float32), (what, "ln")
        assert torch.equal(c.ln[2], c.B.sum(1)), (what, "ln_csum is the exact row sum")
        assert ((torch.log2(c.ln[1]) % 1) == 0).all(), (what, "rstd is a power of two")
    for t in (c.cscale, c.rscale):
        if t is not None:
            assert ((torch.log2(t) % 1) == 0).all(), (what, "scales are powers of two")
    for t in c.abs_terms:
        extra = sum(x.abs().max().item() for x in (c.bias, c.cshift) if x is not None)
        assert t.max().item() * 2 + extra * 4 < ACC_LIMIT, (what, "accumulator may leave the exact range of fp32")
    if c.gelu:
        p = c.pre_act
        assert torch.equal(p, p.round()) and p.min().item() >= GELU_THRESHOLD and p.max().item() <= 256, (what, "GELU not saturated", p.min().item(), p.max().item())
    lim = INT_RANGE[c.dtype] if c.dtype != torch.float32 else 0
    if c.pattern == "cancel":
        assert c.acc.abs().min().item() > max(4096, lim), (what, "the cancel block does not leave the integer range", c.acc.abs().min().item())
        if c.dtype != torch.float32:
            assert not representable(c.acc, c.dtype), (what, "every accumulator is exact in the storage type: a rounding would not show")
    if c.pattern == "onehot":
        # (N < K: the caller runs one launch per offset of onehot_offsets(N, K); together they name every k)
        ks = torch.cat([(torch.arange(c.N) + o) % c.K for o in (onehot_offsets(c.N, c.K) if c.N < c.K else [c.k_off])])
        assert len(set(ks.tolist())) == c.K and c.k_off in onehot_offsets(c.N, c.K) + [0], (what, "not every k occurs")
        assert bool((c.B.sum(1) == 1).all()) and bool((c.B.abs().sum(1) == 1).all())
    if c.pattern == "ternary":
        assert c.A.abs().max().item() <= 2 and c.B.abs().max().item() <= 2
        assert bool(c.A.abs().sum(0).gt(0).all()) and bool(c.B.abs().sum(0).gt(0).all()), (what, "a k without weight")
        slab = c.slab
        for k0 in range(0, c.K, slab):
            nz = (c.A[:, k0:k0 + slab] != 0).double() @ (c.B[:, k0:k0 + slab] != 0).double().t()
            assert bool((nz > 0).all()), (what, "an output without a term from slab", k0 // slab)
        assert c.want.abs().max().item() <= INT_RANGE[c.dtype]


def assert_exact(got, want, what, K=None, k_off=0, col_axis=-1):
    """torch.equal, reporting the first differing element: (row, column) for a matrix, the full index otherwise; with K given also
    k = (column + k_off) mod K, the one-hot pattern's source index (col_axis: which index is the product's column n)."""
    got = got.detach().cpu().double()
    want = want.double()
    assert got.shape == want.shape, (what, tuple(got.shape), tuple(want.shape))
    bad = ~((got == want) | (torch.isnan(got) & torch.isnan(want)))
    if bad.any():
        idx = tuple(int(i) for i in bad.nonzero()[0])
        msg = "%s: %d of %d elements differ, first at %s: got %r, want %r" % (what, int(bad.sum()), bad.numel(), idx, got[idx].item(), want[idx].item())
        if K:
            msg += " (k = %d)" % ((idx[col_axis] + k_off) % K)
        e = AssertionError(msg)
        e.index, e.k = idx, ((idx[col_axis] + k_off) % K if K else None)          # for callers that check WHERE a fault shows
        raise e


# ------------------------------------------------------------------------------------------------- by-product sums
def row_part_want(stored, nparts):
    """mlpk.h row_part: (sum, sum of squares) of the values written to C[m, :] over the q-th block of 32 columns; with integer
    stored values every order of summation gives these floats exactly"""
    M, N = stored.shape
    out = torch.zeros((nparts, M, 2), dtype=torch.float64)
    for q in range(nparts):
        blk = stored[:, q * 32:(q + 1) * 32].double()
        out[q, :, 0] = blk.sum(1)
        out[q, :, 1] = (blk * blk).sum(1)
    return out


# ------------------------------------------------------------------------------------------------- GELU emulations
def _header():
    return open(os.path.join(ROOT, "jittor-mlp_amd", "csrc", "mlpk_common.h")).read()


def _coefs(src, name):
    return [float(v) for v in re.search(r"#define %s \{([^}]*)\}" % name, src).group(1).replace("f,", ",").rstrip("f").split(",")]


def _fma32(a, b, c):
    return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(np.float32)


def gelu_f32_emulated(x):
    """gelu_f / erf_fast of mlpk_common.h in emulated fp32 (reciprocal and exponential correctly rounded; the device's are within
    1 ulp, which the threshold test allows for by asking for a margin)"""
    x = np.asarray(x, np.float32)
    z = (x * np.float32(0.70710678118654752440)).astype(np.float32)
    ax = np.abs(z)
    t = (1.0 / _fma32(np.float32(0.3275911), ax, 1.0).astype(np.float64)).astype(np.float32)
    p = _fma32(np.float32(1.061405429), t, np.float32(-1.453152027))
    for cf in (1.421413741, -0.284496736, 0.254829592):
        p = _fma32(p, t, np.float32(cf))
    p = (p * t).astype(np.float32)
    e = np.exp(-(ax.astype(np.float64) ** 2)).astype(np.float32)
    r = np.copysign(_fma32(-p, e, 1.0), z)
    return ((np.float32(0.5) * x).astype(np.float32) * (np.float32(1.0) + r).astype(np.float32)).astype(np.float32), (p * e)


def gelu_f16_emulated(x):
    """the centred polynomial (gelu16_f<f16>) in emulated fp32"""
    src = _header()
    coefs = [np.float32(v) for v in _coefs(src, "MLPK_GELUP_COEFS")]
    scale = np.float32(re.search(r"#define MLPK_GELUP_SCALE ([0-9.]+)f", src).group(1))
    x = np.asarray(x, np.float32)
    r2 = np.float32(np.sqrt(2.0))
    t = np.clip((x * scale).astype(np.float32), -r2, r2)
    u = _fma32(t, t, -1.0)
    q = np.full_like(t, coefs[0])
    for cf in coefs[1:]:
        q = _fma32(q, u, cf)
    return (x * _fma32(t, q, 0.5)).astype(np.float32)


def gelu_bf16_emulated(x):
    """"h2b" (gelu_h2b_f): Phi in packed f16 on the f16 of x, the product in fp32; returns (gelu, Phi)"""
    src = _header()
    hc = _coefs(src, "MLPK_GELUH_COEFS")
    hs = float(re.search(r"#define MLPK_GELUH_SCALE ([0-9.]+)f", src).group(1))

    def f16(v):
        with np.errstate(over="ignore", invalid="ignore"):
            return np.asarray(v, np.float64).astype(np.float16).astype(np.float64)
    x = np.asarray(x, np.float32)
    h = x.astype(np.float16).astype(np.float64)
    t = f16(h * hs)
    u = f16(t * t - 1.0)
    q = f16(hc[0] * u + hc[1])
    for cf in hc[2:]:
        q = f16(q * u + cf)
    p = f16(t * q + 0.5)
    p = np.where(np.isnan(p), 0.0, np.clip(p, 0.0, 1.0))
    return (x * p.astype(np.float32)).astype(np.float32), p


# ------------------------------------------------------------------------------------------------- numpy model of a tiled GEMM
FAULTS = ("skip_last_chunk", "dup_k", "clamped_row", "bias_tail", "bf16_acc", "round_before_bias")


def _round_to(x, dtype):
    return torch.from_numpy(np.ascontiguousarray(x)).to(dtype).to(torch.float32).numpy()


def tiled_gemm_model(A, B, bias, dtype, bm=64, bn=64, slab=32, chunk=8, fault=None):
    """C = round(A B^T + bias) as a tiled kernel computes it: tiles of bm x bn, K walked in slabs with an fp32 accumulator, rows and
    columns past the edge clamped on load and masked on store.  `fault` plants ONE mistake, in the last (ragged) tile unless noted:
      skip_last_chunk    the tile's last 16-byte chunk of K is never multiplied
      dup_k              one k (the first of the last slab) enters twice
      clamped_row        the load clamps one row too early: the tile's last valid row reads the row before it
      bias_tail          the tail column takes bias[n - 1]
      bf16_acc           (every tile) accumulators rounded to bf16 between slabs
      round_before_bias  (every tile) the product rounded to the storage type before the bias is added"""
    assert fault is None or fault in FAULTS
    A = np.asarray(A, np.float32)
    B = np.asarray(B, np.float32)
    bias = np.asarray(bias, np.float32)
    M, K = A.shape
    N = B.shape[0]
    C = np.zeros((M, N), np.float32)
    tm, tn = (M + bm - 1) // bm, (N + bn - 1) // bn
    for ti in range(tm):
        for tj in range(tn):
            last = ti == tm - 1 and tj == tn - 1
            rows = np.minimum(np.arange(ti * bm, ti * bm + bm), M - 1)
            cols = np.minimum(np.arange(tj * bn, tj * bn + bn), N - 1)
            if fault == "clamped_row" and last:
                rows = np.minimum(rows, M - 2)
            a, b = A[rows], B[cols]
            acc = np.zeros((bm, bn), np.float32)
            for k0 in range(0, K, slab):
                k1 = min(K, k0 + slab)
                if fault == "skip_last_chunk" and last and k1 == K:
                    k1 -= chunk
                acc = (acc + a[:, k0:k1] @ b[:, k0:k1].T).astype(np.float32)
                if fault == "dup_k" and last and k0 + slab >= K:
                    acc = (acc + np.outer(a[:, k0], b[:, k0])).astype(np.float32)
                if fault == "bf16_acc":
                    acc = _round_to(acc, torch.bfloat16)
            if fault == "round_before_bias":
                acc = _round_to(acc, dtype)
            bcols = cols.copy()
            if fault == "bias_tail" and last:
                bcols[(N - 1) - tj * bn] = N - 2
            v = (acc + bias[bcols][None, :]).astype(np.float32)
            mm, nn = min(bm, M - ti * bm), min(bn, N - tj * bn)
            C[ti * bm:ti * bm + mm, tj * bn:tj * bn + nn] = v[:mm, :nn]
    return torch.from_numpy(_round_to(C, dtype)).double()


# ------------------------------------------------------------------------------------------------- case tables (shared by the host and the GPU file)
# mlpk_gemm_algo_info's answers for the template tiles (the GPU file asserts that they still are): algo -> (bm, bn, pipeline)
TILES = {1: (256, 256, "reg"), 2: (256, 128, "reg"), 3: (128, 256, "reg"), 4: (128, 128, "reg"), 5: (64, 64, "reg"),
         6: (256, 256, "glds"), 7: (256, 128, "glds"), 8: (128, 256, "glds"), 9: (128, 128, "glds"), 10: (64, 64, "glds"),
         11: (256, 128, "s3"), 12: (128, 128, "s3"), 13: (128, 256, "s3")}
STORAGE = (torch.float32, torch.float16, torch.bfloat16)
SIXTEEN = (torch.float16, torch.bfloat16)

EPILOGUES = {                       # name -> gemm_case keywords (row-major output)
    "bias": dict(),
    "affine": dict(affine=True),
    "res_add_alias": dict(res=1, r_alias=True),
    "res_mul": dict(res=2),
    "rscale": dict(rperiod=12),
    "ln_row": dict(ln_group=1),
    "ln_group": dict(ln_group=5),
    "gelu": dict(gelu=True),
    "gelu_affine_res": dict(gelu=True, affine=True, res=1),
}


def granule_of(algo, dtype):
    """K granule of a tile family: a 16-byte chunk for the register-staged tiles, half a 128-byte slab for direct-to-LDS and s3"""
    return epc_of(dtype) * (1 if TILES[algo][2] == "reg" else 4)


def k_sweep(algo, dtype):
    """every multiple of the granule from one granule to two 128-byte slabs past the pipeline depth (2 stages of 128 bytes for the
    register-staged and direct-to-LDS tiles, 3 stages of 64 bytes for s3: 4 slabs of 128 bytes cover both)"""
    g = granule_of(algo, dtype)
    return list(range(g, 4 * 8 * epc_of(dtype) + 1, g))


def k_plain(algo, dtype):
    """two whole 128-byte slabs and one granule: a peeled tail behind a full pipeline"""
    return 2 * 8 * epc_of(dtype) + granule_of(algo, dtype)


def edge_shapes(algo):
    bm, bn, _ = TILES[algo]
    return [(1, 8), (bm - 1, bn + 8), (bm + 1, bn - 8), (bm + 1, bn + 1)]         # the last: odd ldc, the scalar-store path


def onehot_offsets(N, K):
    """column offsets of the one-hot rows such that, over the launches, every k occurs (one launch when N >= K)"""
    return list(range(0, K, N)) if N < K else [0]


def pattern_offsets(pattern, N, K):
    return onehot_offsets(N, K) if pattern == "onehot" else [0]


def token_t_cases(algo, dtype):
    """token-transposed outputs: the direct path (tiles that straddle images) and, for the 16-bit 128-row tiles, the LDS-staged
    path (whole tiles inside one image).  (t_rows, images, tokens N, t_tokens, keywords)"""
    bm, bn, _ = TILES[algo]
    out = [(36, -(-(bm + 1) // 36), bn + 8, bn + 11, dict(res=1, rperiod=36)),
           (36, -(-(bm + 1) // 36), bn + 8, bn + 8, dict(res=2, ldr_extra=4))]
    if dtype != torch.float32 and algo in (4, 12, 13):
        out += [(bm, 2, bn + 8, bn + 8, dict(res=1, rperiod=bm)), (2 * bm, 1, bn - 8, bn, dict(res=2)), (bm, 2, 49, 49, dict(affine=True))]
    return out


# algo 14, the persistent tile: heights x widths x reserved bits, 2 .. 8 K slabs of 64
P8_HEIGHTS, P8_WIDTHS, P8_SLABS, P8_BITS = (64, 128, 192, 256, 320), (256, 512), (2, 3, 4, 5, 6, 7, 8), (0, 16, 64, 128)
P8_EPILOGUES = ["bias", "affine", "res_add_alias", "ln_row", "gelu"]
# algo 15, the generated tile
Q4_M, Q4_N, Q4_K = (256, 512, 768), (128, 384), (192, 256, 320, 384, 448, 768, 832)
Q4_EPILOGUES = {"bias": dict(), "ln": dict(ln_group=1), "gelu": dict(gelu=True), "gelu_ln": dict(gelu=True, ln_group=1), "res": dict(res=1)}
# algo 16, the skinny fp32 kernel: (M, N, K)
SKINNY_CASES = [(1, 64, 64), (8, 64, 128), (5, 128, 96), (16, 192, 256), (3, 1000, 64), (300, 40, 64), (7, 8, 16)]     # (N < 48: a lane per row)
# mlpk_gemm_nt_pair: two heights of the 256 x 128 / 128 x 128 s3 tiles
PAIR_CASES = [((64, 128, 96), (192, 128, 160)), ((130, 136, 64), (40, 264, 96))]


def template_cases(algo, dtype):
    """Every case of one template tile (algos 1 .. 13) and one storage type: (label, pattern, M, N, K, gemm_case keywords).
    Edge shapes and every epilogue at K = k_plain; at (bm + 1, bn + 8) the K sweep; the token-transposed forms."""
    bm, bn, _ = TILES[algo]
    kp = k_plain(algo, dtype)
    for pat in PATTERNS:
        offs = (lambda n, k: onehot_offsets(n, k)) if pat == "onehot" else (lambda n, k: [0])
        for (M, N) in edge_shapes(algo):
            for off in offs(N, kp):
                yield ("edge", pat, M, N, kp, dict(k_off=off))
        for K in k_sweep(algo, dtype):
            for off in offs(bn + 8, K):
                yield ("ksweep", pat, bm + 1, bn + 8, K, dict(k_off=off))
        for name, kw in EPILOGUES.items():
            for off in offs(bn + 8, kp):
                yield ("epi:" + name, pat, bm + 1, bn + 8, kp, dict(kw, k_off=off))
        for (t_rows, nimg, N, t_tokens, kw) in token_t_cases(algo, dtype):
            for off in offs(N, kp):
                yield ("token_t", pat, nimg * t_rows, N, kp, dict(kw, t_rows=t_rows, t_tokens=t_tokens, k_off=off))


def p8_cases():
    """(epilogue, pattern, M, N, K, reserved bits, keywords): every height x width x plan bit, the slab count and the epilogue walking
    through their values along the list (every slab count meets every epilogue: 7 and 5 are coprime), then every slab count with
    every epilogue at the mixed height.  Bit 64 (the LDS-staged epilogue) exists for 256-row tiles only: other heights are refused
    by the library (tests/test_gpu_ops.py holds that), so they are not listed."""
    i = 0
    for M in P8_HEIGHTS:
        for N in P8_WIDTHS:
            for bits in P8_BITS:
                if bits == 64 and M % 256:
                    continue
                name = P8_EPILOGUES[i % len(P8_EPILOGUES)]
                nslab = P8_SLABS[i % len(P8_SLABS)]
                i += 1
                for pat in PATTERNS:
                    for off in pattern_offsets(pat, N, nslab * 64):
                        yield (name, pat, M, N, nslab * 64, bits, dict(EPILOGUES[name], k_off=off))
    for nslab in P8_SLABS:
        for name in P8_EPILOGUES:
            for pat in PATTERNS:
                for off in pattern_offsets(pat, 256, nslab * 64):
                    yield (name, pat, 320, 256, nslab * 64, 0, dict(EPILOGUES[name], k_off=off))


def q4_cases(K):
    """(epilogue, pattern, M, N, K, keywords): every M x N x epilogue class x pattern at one K"""
    for M in Q4_M:
        for N in Q4_N:
            for name, kw in Q4_EPILOGUES.items():
                for pat in PATTERNS:
                    for off in pattern_offsets(pat, N, K):
                        yield (name, pat, M, N, K, dict(kw, k_off=off))


# ------------------------------------------------------------------------------------------------- token-mixing products
def token_gemm_cases():
    """mlpk_token_gemm / _ln / _ln_post: (images, channels per image t_rows, tokens S, variant, keywords).  S = 196 runs the pipelined
    kernel (>= 3 groups of 32 tokens, even), 16 and 49 the other one; three images of 96 channels span a 256-row tile."""
    for S in (16, 49, 196):
        for C in (32, 96):
            yield (3, C, S, "plain", dict())
            yield (3, C, S, "plain", dict(res=2, ldr_extra=C))                  # the gate inside a wider tensor
            yield (3, C, S, "plain", dict(res=1, r_alias=True, rperiod=C))      # in place, per-channel scale
            yield (3, C, S, "ln", dict(res=2, ldr_extra=C))
            yield (3, C, S, "ln", dict(res=1, rperiod=C))
            yield (3, C, S, "affine_res", dict(rperiod=C))                      # MLPK_RES_ADD_AFFINE, in place
            if S > 64 and S % 2 == 0:
                yield (3, C, S, "post", dict(rperiod=C))                        # ... with the affine that follows applied on store


def token_case(pattern, dtype, nimg, C, S, variant, **kw):
    """One token-mixing product: the gemm_case with A = xt (nimg C rows of S tokens), B = W (S x S), token-transposed output.
    variant "ln": x, mean, rstd, gamma, beta such that (x - mean) rstd gamma + beta IS xt (integers; gamma, rstd powers of two);
    "affine_res": no statistics, the residual is the affine output itself; "post": out = post_scale round(result) + post_shift."""
    c = gemm_case(pattern, dtype, nimg * C, S, S, t_rows=C, t_tokens=S, **kw)
    c.variant, c.nimg, c.C, c.S = variant, nimg, C, S
    c.x = c.mean = c.rstd = c.gamma = c.beta = c.post = None
    if variant != "plain":
        at = c.A.reshape(nimg, C, S).permute(0, 2, 1).reshape(nimg * S, C)      # token-major operand
        ch = torch.arange(C)
        r = torch.arange(nimg * S)
        c.gamma = torch.tensor([1.0, 2.0])[ch % 2].double()
        c.beta = (ch % 3 - 1).double()
        if variant == "ln":
            c.mean = (r % 4 - 1).double()
            c.rstd = torch.tensor([1.0, 2.0, 1.0])[r % 3].double()
            c.x = (at - c.beta[None, :]) / c.gamma[None, :] / c.rstd[:, None] + c.mean[:, None]
        else:
            c.x = (at - c.beta[None, :]) / c.gamma[None, :]
            assert c.res == 0
            c.want = c.pre_res + at.reshape(nimg, S, C)
        if variant == "post":
            c.post = (torch.tensor([2.0, 1.0])[ch % 2].double(), (ch % 5 - 2).double())
            c.pre_post = c.want
            c.want = c.want * c.post[0] + c.post[1]
    return c


def check_token_case(c):
    check_case(c)
    for name in ("x", "pre_post"):
        t = getattr(c, name, None)
        if t is not None:
            assert representable(t, c.dtype), (c.pattern, str(c.dtype), c.S, c.C, name)
    assert representable(c.want, c.dtype)


# ------------------------------------------------------------------------------------------------- implicit convolution
# mlpk_conv_gemm_nhwc: (images, H, W, Cin, k, stride, pad); Cout = K = k k Cin, so that the one-hot pattern names every (tap, channel)
CONV_CASES = [(2, 5, 7, 32, 3, 2, 1), (2, 6, 6, 64, 3, 2, 1), (2, 6, 6, 32, 2, 2, 0), (1, 5, 7, 64, 3, 2, 1), (2, 6, 6, 64, 2, 2, 0)]


def im2col_nhwc(x, k, stride, pad):
    """(B, H, W, Cin) -> (B Ho Wo, k k Cin), tap-major then channel, zeros outside the map; also which (row, tap) lie inside"""
    B, H, W, Cin = x.shape
    Ho, Wo = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
    A = torch.zeros((B, Ho, Wo, k * k, Cin), dtype=torch.float64)
    inside = torch.zeros((B, Ho, Wo, k * k), dtype=torch.bool)
    for oy in range(Ho):
        for ox in range(Wo):
            for i in range(k):
                for j in range(k):
                    y, xx = oy * stride + i - pad, ox * stride + j - pad
                    if 0 <= y < H and 0 <= xx < W:
                        A[:, oy, ox, i * k + j] = x[:, y, xx]
                        inside[:, oy, ox, i * k + j] = True
    return A.reshape(B * Ho * Wo, k * k * Cin), inside.reshape(B * Ho * Wo, k * k)


def conv_case(pattern, dtype, B, H, W, Cin, k, stride, pad, seed=3):
    """x, w (Cout, K), bias and the exact output.  onehot: C[m, n] = the window value at (tap, channel) n, exactly 0 for a tap outside
    the map.  ternary: sparse x and w; one channel in every 32 holds a non-zero in every pixel and every weight row, so that every
    output has a term from every K slab WHOSE TAP LIES INSIDE THE MAP (a border tap's slab is all zeros by the operation's
    definition: that is the reason this premise is restricted).  cancel: the block is channels 0 .. 7 of the centre tap (k = 3; tap 0
    for k = 2), which lies inside the map for every output, so bias[n] cancels it."""
    K = k * k * Cin
    N = K
    c = types.SimpleNamespace(pattern=pattern, dtype=dtype, geom=(B, H, W, Cin, k, stride, pad), N=N, K=K)
    pix = torch.arange(B * H * W).reshape(B, H, W, 1)
    ch = torch.arange(Cin).reshape(1, 1, 1, Cin)
    n = torch.arange(N)
    g = torch.Generator().manual_seed(seed)
    block = 0.0
    if pattern == "onehot":
        code = 1 + (3 * pix + 5 * ch + pix // 7) % 7
        x = (code * (1 - 2 * ((pix + ch) % 2))).double()
        w = torch.zeros((N, K), dtype=torch.float64)
        w[n, n % K] = 1.0
    else:
        def sparse(shape, density):
            mag = torch.randint(1, 3, shape, generator=g).double()
            sgn = torch.randint(0, 2, shape, generator=g).double() * 2 - 1
            return mag * sgn * (torch.rand(shape, generator=g) < density).double()
        x = sparse((B, H, W, Cin), 1.0 / 8)
        w = sparse((N, K), 1.0 / 12)
        for s, c0 in enumerate(range(1 + 8, Cin, 32)):                   # one forced channel per 32-channel slab (outside the cancel block)
            x[..., c0] = (1 + (pix[..., 0] + s) % 2).double()
            for tap in range(k * k):
                w[:, tap * Cin + c0] = (1 + (n + tap) % 2).double() * (1 - 2 * ((tap + s) % 2))
        if pattern == "cancel":
            tapc = (k * k) // 2 if k == 3 else 0
            x[..., :8] = CANCEL_BIG
            x[..., 0] = CANCEL_BIG + (pix[..., 0] % 4).double()
            for tap in range(k * k):
                w[:, tap * Cin:tap * Cin + 8] = 0.0
            w[:, tapc * Cin:tapc * Cin + 8] = CANCEL_BIG
            w[:, tapc * Cin] = 1.0
            block = 7 * CANCEL_BIG * CANCEL_BIG + CANCEL_BIG
            c.tapc = tapc
    c.x, c.w = x, w
    c.A, c.inside = im2col_nhwc(x, k, stride, pad)
    c.acc = c.A @ w.t()
    c.abs_terms = c.A.abs() @ w.abs().t()
    c.bias = ((n * 5) % 7 - 3).double() - block
    c.want = c.acc + c.bias[None, :]
    return c


def check_conv_case(c):
    what = (c.pattern, str(c.dtype), c.geom)
    B, H, W, Cin, k, stride, pad = c.geom
    for name in ("x", "w", "want"):
        assert representable(getattr(c, name), c.dtype), (what, name)
    assert c.abs_terms.max().item() * 2 + c.bias.abs().max().item() * 4 < ACC_LIMIT
    assert not c.inside.all() or pad == 0, (what, "no border tap in the case")
    if c.pattern == "onehot":
        assert bool((c.w.sum(0) == 1).all()), (what, "not every (tap, channel) is named")
        out = ~c.inside.repeat_interleave(Cin, dim=1)                      # (row, k) outside the map
        assert bool((c.want - c.bias[None, :])[out].eq(0).all())
    elif c.pattern == "ternary":
        assert c.x.abs().max().item() <= 2 and c.w.abs().max().item() <= 2
        for k0 in range(0, c.K, 32):
            nz = (c.A[:, k0:k0 + 32] != 0).double() @ (c.w[:, k0:k0 + 32] != 0).double().t()
            rows = c.inside[:, k0 // Cin]
            assert bool((nz[rows] > 0).all()), (what, "an output without a term from an inside slab", k0 // 32)
            assert bool((c.A[~rows][:, k0:k0 + 32] == 0).all())
    else:
        assert bool(c.inside[:, c.tapc].all()), (what, "the block's tap leaves the map")
        assert c.acc.abs().min().item() > max(4096, INT_RANGE[c.dtype]) and not representable(c.acc, c.dtype)


# ------------------------------------------------------------------------------------------------- patch embedding and stem
EMBED_C = (32, 128)
# the smallest image each _supported function takes (tests/test_exact_host.py asserts that it is), and a larger one
EMBED4_CASES = [(2, 4, 4), (3, 20, 12)]                      # (images, H, W)
STEM7_CASES = [(2, 1, 8, 3), (2, 3, 8, 2), (2, 18, 16, 3), (1, 21, 24, 2)]      # (images, H, W, pad)


def embed4_image(c, B, H, W):
    """the NCHW image whose 4 x 4 patches are the rows of c.A (k = (channel, row, column), Conv2d's order): non-overlapping windows,
    so every operand pattern of gemm_case carries over unchanged (K = 48; slab = 16, the 32 x 32 x 16 MFMA's K)"""
    return c.A.reshape(B, H // 4, W // 4, 3, 4, 4).permute(0, 3, 1, 4, 2, 5).reshape(B, 3, H, W).contiguous()


def stem7_case(pattern, dtype, B, H, W, pad, C, k_off=0, seed=4):
    """mlpk_stem7: Conv2d(3 -> C, 7, stride 4, pad) on an NCHW image, k = (ci * 7 + i) * 7 + j, K = 147.  onehot: weight row n selects
    k = (n + k_off) mod 147 (C < 147: one launch per offset); ternary: sparse, the centre tap of every input channel forced non-zero
    (it lies inside the map for every output; the other taps leave the map at the border, where their terms are zero by
    definition); cancel: the block is the centre tap of the three channels."""
    K = 147
    Ho, Wo = (H + 2 * pad - 7) // 4 + 1, (W + 2 * pad - 7) // 4 + 1
    g0 = 3 - pad                                             # the centre tap of window (oy, ox) is pixel (4 oy + g0, 4 ox + g0)
    assert 0 <= g0 < 4 and 4 * (Ho - 1) + g0 < H and 4 * (Wo - 1) + g0 < W
    c = types.SimpleNamespace(pattern=pattern, dtype=dtype, geom=(B, H, W, pad, C), K=K, N=C, k_off=k_off)
    g = torch.Generator().manual_seed(seed)
    n = torch.arange(C)
    pix = torch.arange(B * H * W).reshape(B, 1, H, W)
    ci = torch.arange(3).reshape(1, 3, 1, 1)
    block = 0.0
    if pattern == "onehot":
        code = 1 + (3 * pix + 5 * ci + pix // 7) % 7
        x = (code * (1 - 2 * ((pix + ci) % 2))).double()
        w = torch.zeros((C, K), dtype=torch.float64)
        w[n, (n + k_off) % K] = 1.0
    else:
        def sparse(shape, density):
            mag = torch.randint(1, 3, shape, generator=g).double()
            sgn = torch.randint(0, 2, shape, generator=g).double() * 2 - 1
            return mag * sgn * (torch.rand(shape, generator=g) < density).double()
        x = sparse((B, 3, H, W), 1.0 / 6)
        w = sparse((C, K), 1.0 / 8)
        centre = [(q * 7 + 3) * 7 + 3 for q in range(3)]
        grid = x[:, :, g0::4, g0::4]
        grid[:] = (1 + (pix[:, :, g0::4, g0::4] + ci) % 2).double()
        for q, k in enumerate(centre):
            w[:, k] = (1 + (n + q) % 2).double() * (1 - 2 * (q % 2))
        if pattern == "cancel":
            grid[:] = CANCEL_BIG
            grid[:, 0] = CANCEL_BIG + (pix[:, 0, g0::4, g0::4] % 4).double()
            w[:, centre[1]] = w[:, centre[2]] = CANCEL_BIG
            w[:, centre[0]] = 1.0
            block = 2 * CANCEL_BIG * CANCEL_BIG + CANCEL_BIG
    c.x, c.w = x, w
    c.bias = ((n * 5) % 7 - 3).double() - block
    F = torch.nn.functional
    c.acc = F.conv2d(x, w.reshape(C, 3, 7, 7), None, stride=4, padding=pad).permute(0, 2, 3, 1).reshape(-1, C)
    c.abs_terms = F.conv2d(x.abs(), w.abs().reshape(C, 3, 7, 7), None, stride=4, padding=pad)
    c.want = c.acc + c.bias[None, :]
    return c


def check_stem7_case(c):
    what = (c.pattern, str(c.dtype), c.geom)
    for name in ("x", "w", "want"):
        assert representable(getattr(c, name), c.dtype), (what, name)
    assert c.abs_terms.max().item() * 2 + c.bias.abs().max().item() * 4 < ACC_LIMIT
    if c.pattern == "onehot":
        assert bool((c.w.abs().sum(1) == 1).all()) and c.k_off in onehot_offsets(c.N, c.K)
    elif c.pattern == "ternary":
        assert c.x.abs().max().item() <= 2 and c.w.abs().max().item() <= 2
        for q in range(3):                                   # a term from every input channel (49 k each) in every output
            k = (q * 7 + 3) * 7 + 3
            assert bool((c.w[:, k] != 0).all())
    else:
        assert c.acc.abs().min().item() > max(4096, INT_RANGE[c.dtype]) and not representable(c.acc, c.dtype)


# ------------------------------------------------------------------------------------------------- fused two-product kernels
def mlp_case(pattern, dtype, M, K1, T, N2, *, norm=0, off1=0, off2=0, seed=7):
    """h = gelu(A W1^T + b1) (M x T), core = h W2^T + b2 (M x N2): mlpk_token_mlp (A = the rows of xt, K1 = N2 = tokens) and
    mlpk_channel_mlp (A = x, K1 = N2 = channels).  Every pre-activation is an integer in [GELU_THRESHOLD, 256], so the GELU is the
    identity and the kernel is linear: h[m, t] = hbase[t] + d[m, t] with hbase = 132 + a small code of t, and b2 = -W2 hbase + a small
    code of s takes the large part of the second accumulator away (an fp32 vector, as the cancel pattern asks): core = W2 d + code.
      onehot   W1[t] = e_((t + off1) mod K1), W2[s] = e_((s + off2) mod T): core[m, s] names the hidden unit and, through it, the k
      ternary  sparse {-2 .. 2} in A, W1 and W2, a non-zero term from every slab of 32 in both products
      cancel   product 1: the block of cancel_operands, taken away by b1; hidden units 0 .. 7 are pure bias (W1 rows zero) and meet
               W2 = 64 there, so that the second accumulator passes 8 x 64 x 132 whatever the order
    norm = g > 0: mlpk_channel_mlp's folded norm, one statistic per g rows: h = (A (W1 gamma)^T - mean csum) rstd + b1 + W1 beta, integer
    means, power-of-two gamma / rstd (the cancel pattern keeps mean 0, rstd 1, gamma 1, beta 0: its block is cancelled per column)."""
    c = types.SimpleNamespace(pattern=pattern, dtype=dtype, M=M, K1=K1, T=T, N2=N2, norm=norm, off1=off1, off2=off2)
    t = torch.arange(T)
    s = torch.arange(N2)
    block = 0.0
    if pattern == "onehot":
        c.A, c.w1 = onehot_operands(M, T, K1, off1)
        c.w2 = onehot_operands(1, N2, T, off2)[1]
    else:
        if pattern == "ternary":
            c.A, c.w1 = ternary_operands(M, T, K1, 32, seed)
        else:
            c.A, c.w1, block = cancel_operands(M, T, K1, dtype, seed)
            c.w1[:8] = 0.0
        c.w2 = ternary_operands(N2, N2, T, 32, seed + 1, density=min(1.0 / 12, 2.0 / T))[1]
        c.w2 = c.w2.sign()                                   # magnitude 1: sums over up to 28 slabs stay inside the bf16 integer range
        if pattern == "cancel":
            c.w2[:, :8] = CANCEL_BIG
    c.gamma = c.beta = c.mean = c.rstd = c.csum = None
    w1f = c.w1
    shift = torch.zeros(T, dtype=torch.float64)
    if norm:
        k = torch.arange(K1)
        plain = pattern == "cancel"
        c.gamma = torch.ones(K1, dtype=torch.float64) if plain else torch.tensor([1.0, 2.0])[k % 2].double()
        c.beta = torch.zeros(K1, dtype=torch.float64) if plain else (k % 3 - 1).double()
        ns = (M + norm - 1) // norm
        r = torch.arange(ns)
        c.mean = torch.zeros(ns, dtype=torch.float64) if plain else (r % 3 - 1).double()
        c.rstd = torch.ones(ns, dtype=torch.float64) if plain else torch.tensor([1.0, 2.0, 1.0])[r % 3].double()
        w1f = c.w1 * c.gamma[None, :]
        c.csum = w1f.sum(1)
        shift = c.w1 @ c.beta
    c.w1f = w1f
    acc1 = c.A @ w1f.t()
    c.acc1 = acc1
    d = acc1
    if norm:
        idx = torch.arange(M) // norm
        d = (acc1 - c.mean[idx][:, None] * c.csum[None, :]) * c.rstd[idx][:, None]
    blk = torch.full((T,), float(block), dtype=torch.float64)
    if pattern == "cancel":
        blk[:8] = 0.0
    c.hbase = GELU_OFFSET[dtype] + (t * 5 % 7 - 3).double()
    c.b1 = c.hbase - blk - shift                             # (the packer adds W1 beta back)
    c.h = d + (c.b1 + shift)[None, :]
    c.b2 = -(c.w2 @ c.hbase) + (s * 3 % 5 - 2).double()
    c.acc2 = c.h @ c.w2.t()
    c.core = c.acc2 + c.b2[None, :]
    c.abs1 = c.A.abs() @ w1f.abs().t() + (c.mean.abs()[torch.arange(M) // norm][:, None] * c.csum.abs()[None, :] if norm else 0.0)
    c.abs2 = c.h.abs() @ c.w2.abs().t()
    return c


def check_mlp_case(c, hidden_dtype=None, residual=None):
    """premises of a fused case; residual = the tensor added to core (same shape), so that what is STORED is checked too"""
    what = (c.pattern, str(c.dtype), c.M, c.K1, c.T, c.N2, c.norm)
    for name in ("A", "w1f", "w2"):
        assert representable(getattr(c, name), c.dtype), (what, name)
    if hidden_dtype is not None:
        assert representable(c.w2, hidden_dtype), (what, "w2 in the hidden's type")
    assert torch.equal(c.h, c.h.round()) and c.h.min().item() >= GELU_THRESHOLD and c.h.max().item() <= 256, (what, "GELU not saturated", c.h.min().item(), c.h.max().item())
    assert representable(c.h, hidden_dtype or c.dtype), (what, "hidden")
    for v in (c.b1, c.b2, c.gamma, c.beta, c.mean, c.rstd, c.csum):
        if v is not None:
            assert representable(v, torch.float32), what
    if c.norm:
        assert ((torch.log2(c.gamma) % 1) == 0).all() and ((torch.log2(c.rstd) % 1) == 0).all()
        assert representable(c.w1 @ c.beta + c.b1, torch.float32)
    assert c.abs1.max().item() * 2 + c.b1.abs().max().item() * 4 < ACC_LIMIT and c.abs2.max().item() * 2 + c.b2.abs().max().item() * 4 < ACC_LIMIT, (what, "fp32 range")
    stored = c.core if residual is None else c.core + residual
    assert representable(stored, c.dtype), (what, "stored value", stored.abs().max().item())
    assert representable(c.core, c.dtype)
    if c.pattern == "onehot":
        assert bool((c.w1.sum(1) == 1).all()) and bool((c.w2.sum(1) == 1).all())
    else:
        for (a, b, K) in ((c.A, c.w1f[8:] if c.pattern == "cancel" else c.w1f, c.K1), (c.h, c.w2, c.T)):
            for k0 in range(0, K, 32):
                nz = (a[:, k0:k0 + 32] != 0).double() @ (b[:, k0:k0 + 32] != 0).double().t()
                assert bool((nz > 0).all()), (what, "an output without a term from slab", k0 // 32)
    if c.pattern == "cancel":
        lim = max(4096, INT_RANGE[c.dtype])
        assert c.acc1[:, 8:].abs().min().item() > lim and c.acc2.abs().min().item() > lim, (what, "an accumulator stays in range")
        assert not representable(c.acc2, c.dtype)


def mlp_offsets(pattern, K1, T, N2):
    """(off1, off2) pairs of the one-hot launches: together they name every k of both products"""
    if pattern != "onehot":
        return [(0, 0)]
    o1, o2 = onehot_offsets(T, K1), onehot_offsets(N2, T)
    return [(o1[i % len(o1)], o2[i % len(o2)]) for i in range(max(len(o1), len(o2)))]


# mlpk_channel_mlp: (C, M, norm group (0: none), residual: "x" = out aliases x and R, "other", None)
CHANNEL_MLP_CASES = [(C, M, norm, res) for C in (64, 96, 192) for (M, norm, res) in ((257, 0, "x"), (511, 1, "x"), (257, 64, "other"), (511, 0, None))]
# mlpk_token_mlp layouts 0 / 1: (images, channels, S, nchunks); the hidden is 4 short of whole chunks (zero-padded rows)
TOKEN_MLP_CASES = [(2, 136, S, nch) for S in (16, 49, 196) for nch in (1, 3)]
# layouts 2 / 3 and mlpk_token_mlp_ln: S = 196, 256 channels per image, two images
TOKEN_MLP_T4_NCH = (2, 3, 28)


def token_mlp_residual(c, nimg, C, S, seed=9):
    """the residual stream x (nimg S, C), integer-valued, and what the kernel must leave in it: x[b, s, ch] + core[(b, ch), s]"""
    g = torch.Generator().manual_seed(seed)
    x = torch.randint(-4, 5, (nimg * S, C), generator=g).double()
    return x, x.reshape(nimg, S, C) + c.core.reshape(nimg, C, S).permute(0, 2, 1)


def token_stats_want(stored, planes):
    """mlpk_token_mlp `stats`: per plane of C / planes channels, (sum, sum of squares) of the values written to each token row"""
    rows, C = stored.shape
    w = C // planes
    blk = stored.reshape(rows, planes, w).permute(1, 0, 2).double()
    return torch.stack([blk.sum(2), (blk * blk).sum(2)], dim=2)


def token_mlp_ln_inputs(c, nimg, C, S):
    """mlpk_token_mlp_ln: the token-major x whose LayerNorm (x - mean) rstd gamma + beta IS the operand c.A (gamma in {1, 2}, rstd 1,
    integer mean and beta: x is half-integer valued), updated in place: want = x + core transposed"""
    at = c.A.reshape(nimg, C, S).permute(0, 2, 1).reshape(nimg * S, C)
    ch, r = torch.arange(C), torch.arange(nimg * S)
    gamma, beta = torch.tensor([1.0, 2.0])[ch % 2].double(), (ch % 3 - 1).double()
    mean, rstd = (r % 4 - 1).double(), torch.ones(nimg * S, dtype=torch.float64)
    x = (at - beta[None, :]) / gamma[None, :] + mean[:, None]
    return x, mean, rstd, gamma, beta, x.reshape(nimg, S, C) + c.core.reshape(nimg, C, S).permute(0, 2, 1)


# ------------------------------------------------------------------------------------------------- depthwise convolution: three forms
# mlpk_dwconv_nhwc is three kernels behind one entry point (csrc/mlpk_dwconv.hip, csrc/mlpk_remap.hip): the matrix-core form
# (dwconv_mfma_kernel, 16-bit, maps of at most 32 x 32; FULL = a 32 x 32 map and whole groups of 32 channels), the LDS-tiled form
# (dwconv_lds_kernel) and the generic one (mlpk_dwconv_direct).  dwconv_form / dwconv_plan / dwconv_redeal RESTATE the library's
# selection -- they are the coverage claim of the table below (tests/test_exact_host.py asserts it), not the oracle: if they go stale,
# the exact comparison still judges whatever kernel ran.
DWCONV_OLD_CASES = [(3, 8, 8, 40, k) for k in (3, 7, 9)]     # the table before this one (kept as its first rows): only res[0][0] holds data
# ((images, H, W, C, k), what the row reaches): every geometry once
DWCONV_TABLE = [((3, 8, 8, 40, k), "one block of 16 x 16, a partial channel group, one image range") for k in (3, 7, 9)] + [
    ((3, 8, 8, 40, 5), "... and k = 5"),
    ((2, 17, 19, 40, 9), "all four blocks, odd W, the store's tail at x >= 16"),
    ((2, 19, 17, 40, 7), "all four blocks, odd W, the store's tail at x >= 16"),
    ((2, 31, 25, 32, 5), "all four blocks, odd W, the store's tail at x >= 16"),
    ((2, 25, 31, 32, 3), "all four blocks, odd W, the store's tail at x >= 16"),
] + [((3, 32, 32, 32, k), "FULL with the prefetch of the next image running") for k in (3, 5, 7, 9)] + [
    ((2, 32, 32, 64, 9), "FULL, two channel groups"),
    ((2, 32, 32, 40, 7), "a full map with a partial channel group: not FULL"),
    ((6, 5, 6, 32, 5), "two image ranges, the last of 2 images"),
    ((9, 4, 4, 8, 3), "three ranges, the last of 1 image"),
    ((32, 4, 4, 256, 3), "a grid of 8 x 8 workgroups: the re-deal over the XCDs is on"),
    ((29, 6, 6, 256, 9), "the re-deal with a partial last range"),
    ((2, 1, 32, 8, 7), "one row"),
    ((2, 32, 1, 8, 7), "one column"),
    ((1, 1, 1, 8, 9), "one pixel"),
    ((2, 33, 9, 32, 9), "H just past 32: the 16-bit LDS-tiled form"),
    ((2, 9, 40, 32, 3), "LDS-tiled, five strips"),
    ((2, 9, 37, 40, 5), "LDS-tiled, W % 8 != 0, a partial channel tile"),
    ((1, 34, 34, 32, 7), "LDS-tiled, a 34 x 34 map at k = 7"),
    ((1, 48, 40, 32, 9), "the staged tile is over 160 KiB: generic"),
    ((1, 48, 40, 16, 9), "the staged tile is over 160 KiB: generic"),
    ((2, 7, 9, 12, 3), "C % 8 != 0: generic in 16 bits, LDS-tiled in fp32"),
    ((2, 7, 9, 20, 5), "C % 8 != 0: generic in 16 bits, LDS-tiled in fp32"),
    ((2, 7, 9, 68, 3), "C % 8 != 0 and the generic kernel's second channel block of 64"),
    ((2, 7, 9, 6, 3), "C % 4 != 0: generic in every type"),
    ((2, 7, 9, 66, 3), "C % 4 != 0, second channel block"),
    ((1, 6, 6, 8, 1), "k = 1: generic"),
    ((1, 6, 6, 8, 11), "k = 11: generic"),
    ((1, 20, 20, 40, 13), "k = 13: generic"),
]
DWCONV_CASES = [g for g, _ in DWCONV_TABLE]
DWCONV_OFFSET_CASE = ((2, 9, 9, 16, 5), 4)                   # 16-bit, x starts 4 elements = 8 bytes into its buffer: generic
DWCONV_SWEEP = [(3, 8, 8, 32, k) for k in (3, 5, 7, 9)]      # every tap in every channel slot: one-hot with off in range(k * k)
DWCONV_BATCH = [(6, 5, 6, 32, 5), (9, 4, 4, 8, 3), (29, 6, 6, 256, 9), (3, 32, 32, 32, 9), (2, 33, 9, 32, 9), (2, 7, 9, 20, 5)]
DWM_CPW, DWM_CREG = 4, {3: 4, 5: 4, 7: 3, 9: 2}              # dwconv_mfma_launch: cpw; creg_want (DWM_CREG7, DWM_CREG9), capped at cpw


def dwconv_form(dtype, H, W, C, k, aligned=True):
    """which kernel mlpk_dwconv_nhwc runs: "mfma_full" | "mfma" | "lds" | "direct".  aligned: x and out on 16-byte boundaries (False: x
    is off one, which sends every type to the generic kernel)."""
    es = 4 if dtype == torch.float32 else 2                  # mlpk_dwconv_nhwc: es
    epv = 16 // es                                           # mlpk_dwconv_nhwc: 16 / es;  dwconv_lds_launch: EPV
    fast_ok = C % epv == 0 and aligned                       # mlpk_dwconv_nhwc: fast_ok
    tiled_k = k in (3, 5, 7, 9)                              # dwconv_mfma_launch: switch (k), default DW_NOFIT;  dwconv_lds_launch: k != 3 && ...
    if fast_ok and es == 2 and H <= 32 and W <= 32 and C % 8 == 0 and tiled_k:      # mlpk_dwconv_nhwc: the matrix-pipe branch
        return "mfma_full" if (H == 32 and W == 32 and C % 32 == 0) else "mfma"     # dwconv_mfma_launch: full (cg = 8 waves x 4 channels)
    if fast_ok and tiled_k:
        P = (k - 1) // 2                                     # dwconv_lds_launch: P
        strips = (W + 7) // 8                                # dwconv_lds_launch: strips
        pitch = (strips - 1) * 8 + ((8 + k - 1 + epv - 1) // epv) * epv             # dwconv_lds_launch: pitch
        pitch = max(pitch, W + 2 * P)
        pitch = (pitch + epv - 1) // epv * epv
        plane = (H + 2 * P) * pitch                          # dwconv_lds_launch: plane, made an odd number of 16-byte slots
        plane = (plane + epv - 1) // epv * epv
        if (plane // epv) % 2 == 0:
            plane += epv
        ct = 16 if dtype == torch.float32 else 32            # DwCfg<T>::CT
        if ct * plane * es <= 160 * 1024:                    # dwconv_lds_launch: lds > 160 * 1024 -> DW_NOFIT
            return "lds"
    return "direct"


def dwconv_direct_reason(dtype, H, W, C, k, aligned=True):
    """why a geometry reaches the generic kernel: "k" | "channels" | "alignment" | "fit" (None: it does not)"""
    if dwconv_form(dtype, H, W, C, k, aligned) != "direct":
        return None
    if k not in (3, 5, 7, 9):
        return "k"
    if C % epc_of(dtype):
        return "channels"
    return "fit" if aligned else "alignment"


def dwconv_plan(B, C):
    """the matrix-core form's launch: (channel groups, image ranges, images per range, whether the kernel re-deals its workgroups)"""
    groups = (C + 31) // 32                                  # dwconv_mfma_launch: groups (cg = 32)
    per, best = 4, -1                                        # dwconv_mfma_launch: per, best
    for cand in (32, 16, 8, 4):                              # dwconv_mfma_launch: for (cand = 32; cand >= 4; cand /= 2)
        wgs = groups * ((B + cand - 1) // cand)
        cost = ((wgs + 255) // 256) * (cand + 2)             # dwconv_mfma_launch: slots = 256; cost
        if best < 0 or cost < best:
            best, per = cost, cand
    ranges = (B + per - 1) // per                            # dwconv_mfma_launch: grid.y
    redeal = groups % 8 == 0 and (groups * ranges) % 64 == 0                        # dwconv_mfma_kernel: gridDim.x % 8 == 0 && ... % 64 == 0
    return groups, ranges, per, redeal


def dwconv_redeal(bx, by, groups, ranges):
    """dwconv_mfma_kernel's five lines from blockIdx to (gx, gy) = (channel group, image range) when the re-deal is on"""
    idx = bx + groups * by                                   # id
    xcd, l = idx & 7, idx >> 3                               # xcd, l
    oct_, octs = (l >> 3) * 8 + xcd, groups >> 3             # oct, octs
    return (oct_ % octs) * 8 + (l & 7), oct_ // octs         # gx, gy


def dwconv_patterns(dtype, geom):
    """The patterns a geometry carries.  one-hot and ternary: all.  cancel needs (1) a 16-bit type -- its premise is an accumulator that
    the storage type cannot hold, and fp32 holds every one of them -- and (2) a corner tap that is not the centre tap and reaches the
    map: k > 1 and min(H, W) > k // 2 (without it every accumulator is 2^12 + 64 {0, 1}, which both 16-bit types hold)."""
    B, H, W, C, k = geom
    pats = ["onehot", "ternary"]
    if dtype != torch.float32 and k > 1 and min(H, W) > k // 2:
        pats.append("cancel")
    return pats


def dwconv_offsets(pattern, C, k, full=False):
    """one-hot launches: offsets such that every tap occurs (full: every tap in EVERY channel)"""
    if pattern != "onehot":
        return [0]
    return list(range(k * k)) if full else onehot_offsets(C, k * k)


def dwconv_case(pattern, dtype, B, H, W, C, k, off=0, seed=11):
    """mlpk_dwconv_nhwc: out = x + gelu(dw_k(x) + bias) bn_scale + bn_shift, with v = dw_k(x) + bias an integer in [GELU_THRESHOLD, 256].
    The contraction runs over the k k taps of ONE channel.  onehot: channel c's only tap is (c + off) mod k^2, so the output names the
    tap (exactly `bias` where it leaves the map).  ternary: sparse taps with a non-zero centre on a map without zeros (the K slabs of
    the matrix-core form are plane columns; a border tap's terms are zero by definition).  cancel: x = 64 + {0, 1}, the centre tap 64,
    one corner tap 1: the accumulator starts at 2^12 for every pixel -- the only pixel-independent large term a single-channel
    stencil has -- and bias takes it away; larger blocks would leave the map at the border and could not be cancelled per channel."""
    kk = k * k
    c = types.SimpleNamespace(pattern=pattern, dtype=dtype, geom=(B, H, W, C, k), K=kk, off=off)
    g = torch.Generator().manual_seed(seed)
    pix = torch.arange(B * H * W).reshape(B, H, W, 1)
    ch = torch.arange(C)
    w = torch.zeros((kk, C), dtype=torch.float64)
    centre = kk // 2
    block, offset, shift = 0.0, GELU_OFFSET[dtype], -20.0
    if pattern == "cancel":
        x = CANCEL_BIG + ((pix + ch) % 2).double()
        w[centre] = CANCEL_BIG
        w[0] = 1.0
        block, offset, shift = CANCEL_BIG * CANCEL_BIG, 100.0, -48.0
        c.bns = torch.ones(C, dtype=torch.float64)
    else:
        code = 1 + (3 * pix + 5 * ch + pix // 7) % (7 if pattern == "onehot" else 2)
        x = (code * (1 - 2 * ((pix + ch) % 2))).double()
        if pattern == "onehot":
            w[(ch + off) % kk, ch] = 1.0
        else:
            w = (torch.randint(1, 3, (kk, C), generator=g).double() * (torch.randint(0, 2, (kk, C), generator=g).double() * 2 - 1)
                 * (torch.rand((kk, C), generator=g) < 1.0 / 6).double())
            w[centre] = (1 + ch % 2).double()
        c.bns = torch.tensor([1.0, 0.5])[ch % 2].double()
    c.x, c.w = x, w
    c.bias = offset - block + (ch * 5 % 7 - 3).double()
    c.bnh = shift + (ch * 3 % 5 - 2).double()
    F = torch.nn.functional
    wt = w.t().reshape(C, 1, k, k)
    xn = x.permute(0, 3, 1, 2)
    c.acc = F.conv2d(xn, wt, None, padding=k // 2, groups=C).permute(0, 2, 3, 1)
    c.abs_terms = F.conv2d(xn.abs(), wt.abs(), None, padding=k // 2, groups=C)
    c.v = c.acc + c.bias
    c.scaled = c.v * c.bns + c.bnh
    c.want = x + c.scaled
    return c


def check_dwconv_case(c):
    what = (c.pattern, str(c.dtype), c.geom)
    for name in ("x", "w", "v", "want"):
        assert representable(getattr(c, name), c.dtype), (what, name)
    assert representable(c.scaled, c.dtype), (what, "the value in front of the residual")
    assert torch.equal(c.v, c.v.round()) and c.v.min().item() >= GELU_THRESHOLD and c.v.max().item() <= 256, (what, "GELU not saturated", c.v.min().item(), c.v.max().item())
    # (the f16 GELU returns v (1 - 3.4e-6): what is stored must stay well away from 0, where that residue would show)
    assert c.want.abs().min().item() >= GELU_THRESHOLD, (what, c.want.abs().min().item())
    assert c.abs_terms.max().item() * 2 + c.bias.abs().max().item() * 4 < ACC_LIMIT
    assert bool((c.x != 0).all())
    if c.pattern == "onehot":
        assert bool((c.w.sum(0) == 1).all()) and bool((c.w.abs().sum(0) == 1).all())
    elif c.pattern == "ternary":
        assert c.w.abs().max().item() <= 2 and bool((c.w[c.K // 2] != 0).all())
    else:
        assert c.acc.min().item() >= 4096 and not representable(c.acc, c.dtype), (what, "the accumulator stays exact in 16 bits")


# planted faults of the matrix-core form (tests/test_exact_host.py: which table sees which).  Each is ONE mistake in one region:
#   block_10         block (ty, tx) = (1, 0) reads its plane rows 16 too low (the ty term of the row offset is lost)
#   block_01         block (0, 1) reads its plane columns 16 too low (the tx term of the fragment offset is lost)
#   tail_dropped     the per-pixel tail of the four-pixel store (W % 4 != 0) is not written for x0 >= 16: the cell keeps the input
#   prefetch_behind  in a last range that is partial and not the only one, the prefetched registers are one image behind: image b > b0
#                    is computed from image b - 1
#   table_swap       in one channel slot j >= CREG (fragments built from the LDS table, k = 7 / 9) taps d and d + 1 of tap row i are
#                    swapped; `swap` = (j, i, d)
DW_FAULTS = ("block_10", "block_01", "tail_dropped", "prefetch_behind", "table_swap")


def dwconv_fault_region(c, fault, swap=None):
    """the outputs a planted fault can change: a bool mask over (B, H, W, C); all False where the fault's code does not run"""
    B, H, W, C, k = c.geom
    b, y, x, ch = torch.meshgrid(torch.arange(B), torch.arange(H), torch.arange(W), torch.arange(C), indexing="ij")
    none = torch.zeros((B, H, W, C), dtype=torch.bool)
    if not dwconv_form(c.dtype, H, W, C, k).startswith("mfma"):
        return none
    if fault == "block_10":
        return (y >= 16) & (x < 16)
    if fault == "block_01":
        return (y < 16) & (x >= 16)
    if fault == "tail_dropped":
        x0 = x // 4 * 4
        return (x0 >= 16) & (x0 + 3 >= W)
    if fault == "prefetch_behind":
        _, ranges, per, _ = dwconv_plan(B, C)
        return (b > (ranges - 1) * per) if (ranges > 1 and B % per) else none
    assert fault == "table_swap"
    j, i, d = swap
    assert j < DWM_CPW and i < k and d + 1 < k
    return (ch % DWM_CPW == j) if j >= DWM_CREG[k] else none


def dwconv_fault_model(c, fault, swap=None):
    """the reference convolution with one planted fault: what such a kernel would store (float64); c.want where the fault cannot show"""
    B, H, W, C, k = c.geom
    got = c.want.clone()
    if fault is None:
        return got
    region = dwconv_fault_region(c, fault, swap)
    if not region.any():
        return got
    if fault == "tail_dropped":
        got[region] = c.x.expand_as(got)[region]
        return got
    if fault == "prefetch_behind":
        got[region] = c.want.roll(1, 0)[region]
        return got
    if fault == "block_10":
        acc = c.acc.roll(16, 1)
    elif fault == "block_01":
        acc = c.acc.roll(16, 2)
    else:
        j, i, d = swap
        w = c.w.clone()
        sel = torch.arange(C) % DWM_CPW == j
        w[i * k + d, sel], w[i * k + d + 1, sel] = c.w[i * k + d + 1, sel], c.w[i * k + d, sel]
        acc = torch.nn.functional.conv2d(c.x.expand(B, H, W, C).permute(0, 3, 1, 2), w.t().reshape(C, 1, k, k), None, padding=k // 2, groups=C).permute(0, 2, 3, 1)
    v = acc + c.bias
    saturated = (v == v.round()) & (v >= GELU_THRESHOLD)                      # there every GELU form stores v itself
    g = torch.where(saturated, v, 0.5 * v * (1.0 + torch.erf(v * 0.7071067811865476)))
    got[region] = (c.x + g * c.bns + c.bnh)[region]
    return got


# ------------------------------------------------------------------------------------------------- mlpk_vip_branch
VIP_CASES = [(1, 16, 32, 256, 8), (1, 32, 32, 384, 12)]      # (images, H, W, C, seg): K = 128 (h branch) / 256 (w branch), and 384 / 384


def ln_inverse(y):
    """token-major rows x (and mean, rstd, gamma, beta) whose LayerNorm expression (x - mean) rstd gamma + beta is exactly y: gamma and
    rstd powers of two, mean and beta integers, so x is quarter-integer valued"""
    rows, C = y.shape
    ch, r = torch.arange(C), torch.arange(rows)
    gamma, beta = torch.tensor([1.0, 2.0])[ch % 2].double(), (ch % 3 - 1).double()
    mean, rstd = (r % 4 - 1).double(), torch.tensor([1.0, 2.0, 1.0])[r % 3].double()
    return (y - beta[None, :]) / gamma[None, :] / rstd[:, None] + mean[:, None], mean, rstd, gamma, beta


def vip_case(pattern, dtype, B, H, W, C, seg, which):
    """LayerNorm + rearrange + Linear of ViP's h (which = 0) / w (1) branch: the gemm_case whose A is the rearranged operand -- row
    (b, o, g), column l seg + j <- LN(x)[b, h, w, g seg + j] with (l, o) = (h, w) / (w, h) -- and the x that normalises to it;
    `sums` = the operand summed over l, rows (b, g), columns o seg + j"""
    G = C // seg
    L, O = (H, W) if which == 0 else (W, H)
    c = gemm_case(pattern, dtype, B * O * G, L * seg, L * seg)
    a = c.A.reshape(B, O, G, L, seg)
    y = a.permute(0, 3, 1, 2, 4) if which == 0 else a.permute(0, 1, 3, 2, 4)
    c.y = y.reshape(B * H * W, C)
    c.x, c.mean, c.rstd, c.gamma, c.beta = ln_inverse(c.y)
    c.sums = a.sum(3).permute(0, 2, 1, 3).reshape(B * G, O * seg)
    c.geom = (B, H, W, C, seg, which)
    return c


def check_vip_case(c):
    check_case(c)
    assert representable(c.x, c.dtype), (c.pattern, str(c.dtype), c.geom, "x")
    assert representable(c.sums, torch.float32)


# ------------------------------------------------------------------------------------------------- mlpk_smlp_mix, mlpk_smlp_mix_dw
SMLP_CASES = [(2, 7, 7, 32), (2, 14, 14, 64), (3, 7, 7, 64), (2, 14, 14, 32)]      # (images, H, W, C)


def _mix_weight(pattern, S, shift, g):
    """(S, S) mixing weight of one axis and the constant its block adds.  onehot: a cyclic permutation (row v selects v + shift);
    ternary: dense {-1, 0, 1} thirds with a non-zero diagonal; cancel: columns 1 and 2 are 64 (they meet a constant 64: 2^13), column 0
    is +1 and one further column -1, so that the other positions' weights sum to zero in every row"""
    w = torch.zeros((S, S), dtype=torch.float64)
    v = torch.arange(S)
    if pattern == "onehot":
        w[v, (v + shift) % S] = 1.0
        return w, 0.0
    if pattern == "ternary":
        w = torch.randint(-1, 2, (S, S), generator=g).double() * (torch.rand((S, S), generator=g) < 0.5).double()
        w[v, v] = (1 - 2 * (v % 2)).double()
        return w, 0.0
    w[:, 1] = w[:, 2] = CANCEL_BIG
    w[:, 0] = 1.0
    w[v, 3 + v % (S - 3)] = -1.0
    return w, 2 * CANCEL_BIG * CANCEL_BIG


def smlp_case(pattern, dtype, B, H, W, C, dw=False, seed=13):
    """Sparse-MLP's mixing: x^ = bn_s x' + bn_h, out = [Wh x^ along H + bh | Ww x^ along W + bw | x^]; dw: x' = x + dw3x3(dw_s x + dw_h) + dw_b in
    front (else x' = x).  The contraction runs over one image column (K = H) or row (K = W).  x^ is a code of the position (onehot),
    +-{1, 2} (ternary), or -- cancel -- 64 on rows and columns 1 and 2 and small elsewhere: a whole row or column of the map is the
    only block a separable mix can cancel through its per-position bias.  With dw the cancel pattern keeps the centre tap alone
    (x' = 2 x + dw_b): any other tap would carry the 64s across the block's edge."""
    c = types.SimpleNamespace(pattern=pattern, dtype=dtype, geom=(B, H, W, C), dw=dw)
    g = torch.Generator().manual_seed(seed)
    b_, y_, x_, ch = torch.meshgrid(torch.arange(B), torch.arange(H), torch.arange(W), torch.arange(C), indexing="ij")
    code = 1 + (3 * y_ + 5 * x_ + ch + b_) % (7 if pattern == "onehot" else 2)
    xh = (code * (1 - 2 * ((y_ + x_ + ch) % 2))).double()
    if pattern == "cancel":
        big = (y_ == 1) | (y_ == 2) | (x_ == 1) | (x_ == 2)
        xh = torch.where(big, torch.full_like(xh, CANCEL_BIG), xh)
    c.wh, blk_h = _mix_weight(pattern, H, 1, g)
    c.ww, blk_w = _mix_weight(pattern, W, 2, g)
    c.bh = (torch.arange(H) * 5 % 7 - 3).double() - blk_h
    c.bw = (torch.arange(W) * 3 % 5 - 2).double() - blk_w
    cc = torch.arange(C)
    if not dw:
        c.bn_s, c.bn_h = torch.tensor([1.0, 2.0])[cc % 2].double(), (cc % 3 - 1).double()
        c.xres = (xh - c.bn_h) / c.bn_s
        c.x = c.xres
    else:
        c.dw_w = torch.zeros((9, C), dtype=torch.float64)
        c.dw_w[4] = 1.0
        c.dw_b = (cc % 3 - 1).double()
        c.bn_s, c.bn_h = torch.ones(C, dtype=torch.float64), (cc % 2).double()
        if pattern == "cancel":
            c.dw_s, c.dw_h = torch.ones(C, dtype=torch.float64), torch.zeros(C, dtype=torch.float64)
            c.x = (xh - c.bn_h - c.dw_b) / 2                # x' = 2 x + dw_b
        else:
            c.x = xh                                        # (here xh is the INPUT; x^ follows from the sublayer)
            c.dw_w[(cc % 8) + (cc % 8 >= 4).long(), cc] = (1 - 2 * (cc % 2)).double()          # one further tap of +-1 per channel
            c.dw_s, c.dw_h = torch.tensor([1.0, 2.0])[cc % 2].double(), (cc % 2).double()
        inner = (c.x * c.dw_s + c.dw_h).permute(0, 3, 1, 2)
        conv = torch.nn.functional.conv2d(inner, c.dw_w.t().reshape(C, 1, 3, 3), None, padding=1, groups=C).permute(0, 2, 3, 1)
        c.inner = inner
        c.xres = c.x + conv + c.dw_b
        xh = c.xres * c.bn_s + c.bn_h
    c.xhat = xh
    c.acc_h = torch.einsum("gh,bhwc->bgwc", c.wh, xh)
    c.acc_w = torch.einsum("vw,bhwc->bhvc", c.ww, xh)
    c.want = torch.cat([c.acc_h + c.bh.view(1, H, 1, 1), c.acc_w + c.bw.view(1, 1, W, 1), xh], dim=3).reshape(B * H * W, 3 * C)
    return c


def check_smlp_case(c):
    what = (c.pattern, str(c.dtype), c.geom, c.dw)
    for name in ("x", "xres", "xhat", "wh", "ww", "want") + (("inner",) if c.dw else ()):
        assert representable(getattr(c, name), c.dtype), (what, name)
    assert bool((c.xhat != 0).all()) or c.dw
    if c.pattern == "onehot":
        assert bool((c.wh.sum(0) == 1).all()) and bool((c.ww.sum(0) == 1).all())        # every k of both axes is named
    elif c.pattern == "ternary":
        assert bool((c.wh.diagonal() != 0).all()) and bool((c.ww.diagonal() != 0).all())
    else:
        for acc in (c.acc_h, c.acc_w):
            assert acc.abs().min().item() > max(4096, INT_RANGE[c.dtype]) and not representable(acc, c.dtype), (what, "accumulator")


# ------------------------------------------------------------------------------------------------- mlpk_as_conv2, mlpk_as_conv2_stats
ASCONV_CASES = [(2, 7, 7, 96), (2, 14, 9, 192), (2, 7, 7, 192), (2, 14, 9, 96)]      # (images, H, W, C); kernel size 5


def _group_balanced(C, group, seed):
    """(C, C) weights in {-2 .. 2} whose non-zeros come in pairs (+a, -a) on neighbouring channels of ONE shift group: whichever groups
    the halo zeroes, the part 8 x (row sum) of the accumulator vanishes and the pre-activations stay small.  The first pair of every
    32-channel slab is non-zero in every row; the others are sparse."""
    g = torch.Generator().manual_seed(seed)
    w = torch.zeros((C, C), dtype=torch.float64)
    forced = set()
    for g0 in range(0, C, group):
        for c0 in range(g0, min(g0 + group, C) - 1, 2):
            a = torch.randint(1, 3, (C,), generator=g).double() * (torch.randint(0, 2, (C,), generator=g).double() * 2 - 1)
            slab = c0 // 32
            if slab == (c0 + 1) // 32 and slab not in forced:
                forced.add(slab)
            else:
                a = a * (torch.rand((C,), generator=g) < 1.0 / 8).double()
            w[:, c0], w[:, c0 + 1] = a, -a
    assert len(forced) == -(-C // 32)
    return w


def asconv_case(pattern, dtype, B, H, W, C, seed=17):
    """y = gelu(shift_W(u) W1^T + b1) + gelu(shift_H(u) W2^T + b2), u = gelu(t) with mean 0, rstd 1, gamma 1, beta 0 and t >= the threshold:
    all three GELUs are the identity.  The shifts zero whole channel groups at the border (the halo): those outputs must be exactly
    what the remaining groups and the bias give.  onehot: row n of W1 / W2 selects channel n + 1 / n + 2 (an output whose channel is
    in the halo is exactly the bias); ternary: t in {8, 9}, sparse weights with a term in every 32-channel slab; cancel: the block
    is the first 8 channels of the MIDDLE group, whose shift is 0 -- the only channels that never leave the map."""
    import oracle
    c = types.SimpleNamespace(pattern=pattern, dtype=dtype, geom=(B, H, W, C))
    rows = B * H * W
    pix = torch.arange(rows)[:, None]
    ch = torch.arange(C)[None, :]
    n = torch.arange(C)
    group = -(-C // 5)
    block, base = 0.0, 40.0
    if pattern == "onehot":
        t = (GELU_THRESHOLD + (3 * pix + 5 * ch + pix // 7) % 7).double()
        w1 = torch.zeros((C, C), dtype=torch.float64)
        w2 = torch.zeros((C, C), dtype=torch.float64)
        w1[n, (n + 1) % C] = 1.0
        w2[n, (n + 2) % C] = 1.0
    else:
        t = (GELU_THRESHOLD + (pix + ch) % 2).double()
        w1, w2 = _group_balanced(C, group, seed), _group_balanced(C, group, seed + 1)
        if pattern == "cancel":
            g2 = 2 * group
            t[:, g2:g2 + 8] = CANCEL_BIG
            t[:, g2] = CANCEL_BIG + (pix[:, 0] % 4).double()
            for w in (w1, w2):
                w[:, g2:g2 + 8] = CANCEL_BIG
                w[:, g2] = 1.0
            block = 7 * CANCEL_BIG * CANCEL_BIG + CANCEL_BIG
    c.t, c.w1, c.w2 = t, w1, w2
    un = t.reshape(B, H, W, C).permute(0, 3, 1, 2).contiguous()
    c.sw = oracle.axial_shift_nchw(un, 5, 3).permute(0, 2, 3, 1).reshape(rows, C)
    c.sh = oracle.axial_shift_nchw(un, 5, 2).permute(0, 2, 3, 1).reshape(rows, C)
    c.acc1, c.acc2 = c.sw @ w1.t(), c.sh @ w2.t()
    c.b1 = base - block + (n * 5 % 7 - 3).double()
    c.b2 = base - block + (n * 3 % 5 - 2).double()
    c.v1, c.v2 = c.acc1 + c.b1, c.acc2 + c.b2
    c.want = c.v1 + c.v2
    c.abs_terms = max((c.sw.abs() @ w1.abs().t()).max().item(), (c.sh.abs() @ w2.abs().t()).max().item())
    c.halo = ((c.sw == 0).any().item(), (c.sh == 0).any().item())
    return c


def check_asconv_case(c):
    what = (c.pattern, str(c.dtype), c.geom)
    for name in ("t", "w1", "w2", "v1", "v2", "want"):
        assert representable(getattr(c, name), c.dtype), (what, name)
    assert c.t.min().item() >= GELU_THRESHOLD and torch.equal(c.t, c.t.round())
    for v in (c.v1, c.v2):
        assert torch.equal(v, v.round()) and v.min().item() >= GELU_THRESHOLD and v.max().item() <= 256, (what, "GELU not saturated", v.min().item(), v.max().item())
    assert c.abs_terms * 2 + max(c.b1.abs().max().item(), c.b2.abs().max().item()) * 4 < ACC_LIMIT
    assert c.halo == (True, True), (what, "no halo in the case")
    if c.pattern == "onehot":
        assert bool((c.w1.sum(0) == 1).all()) and bool((c.w2.sum(0) == 1).all())
        assert bool(((c.acc1 == 0) == (c.sw.roll(-1, 1) == 0)).all())                   # a halo channel gives exactly the bias
    else:
        for w in (c.w1, c.w2):
            for k0 in range(0, w.shape[1], 32):
                assert bool((w[:, k0:k0 + 32] != 0).any(1).all()), (what, "a weight row without a term in slab", k0 // 32)
    if c.pattern == "cancel":
        for acc in (c.acc1, c.acc2):
            assert acc.abs().min().item() > max(4096, INT_RANGE[c.dtype]) and not representable(acc, c.dtype), (what, "accumulator")


# ------------------------------------------------------------------------------------------------- mlpk_swin_spatial
# (images, H, W, heads, window, shift): every (window, heads) pair, shifted and unshifted padding, maps that are not whole windows
SWIN_CASES = [(2, 8, 8, 1, 4, 0), (2, 8, 8, 1, 4, 2), (2, 12, 10, 2, 5, 0), (2, 12, 10, 2, 5, 2), (2, 14, 14, 3, 7, 0), (2, 14, 14, 3, 7, 3),
              (1, 7, 7, 24, 7, 0), (1, 7, 7, 24, 7, 3), (2, 16, 16, 1, 8, 0), (1, 20, 16, 1, 8, 4)]


def swin_geometry(H, W, ws, shift):
    pad = (ws - shift) if shift else 0
    Hp, Wp = -(-(H + pad + (shift if shift else 0)) // ws) * ws, -(-(W + pad + (shift if shift else 0)) // ws) * ws
    return pad, pad, Hp, Wp


def swin_cancel_possible(H, W, ws, shift):
    """the cancel pattern needs a block that every output sees in full; with padding inside a window the block's zeros differ from
    window to window and bias[head, t] cannot take it away -- only maps of whole, unshifted windows carry it"""
    return shift == 0 and H % ws == 0 and W % ws == 0


def swin_case(pattern, dtype, B, H, W, heads, ws, shift, seed=19):
    """x += crop(merge(W_head . partition(pad(LN(x)))) + bias): per head of 32 channels a (ws^2 x ws^2) matrix over the window's
    positions.  LN(x) is the integer field `xn` (x follows from ln_inverse with rstd 1: half-integers); padded positions are zeros
    AFTER the norm.  onehot: row t of head h selects position t + 1 + h (a padded one gives exactly the bias); ternary: sparse
    {-2 .. 2} with a non-zero diagonal; cancel: the first 8 positions of every window are 64 and meet weights of 64."""
    C, T = heads * 32, ws * ws
    c = types.SimpleNamespace(pattern=pattern, dtype=dtype, geom=(B, H, W, heads, ws, shift), K=T)
    g = torch.Generator().manual_seed(seed)
    pad_t, pad_l, Hp, Wp = swin_geometry(H, W, ws, shift)
    b_, y_, x_, ch = torch.meshgrid(torch.arange(B), torch.arange(H), torch.arange(W), torch.arange(C), indexing="ij")
    code = 1 + (3 * y_ + 5 * x_ + ch + b_) % (7 if pattern == "onehot" else 2)
    xn = (code * (1 - 2 * ((y_ + x_ + ch) % 2))).double()
    t = torch.arange(T)
    wd = torch.zeros((heads, T, T), dtype=torch.float64)
    block = 0.0
    if pattern == "onehot":
        for h in range(heads):
            wd[h, t, (t + 1 + h) % T] = 1.0
    else:
        wd = torch.randint(-2, 3, (heads, T, T), generator=g).double() * (torch.rand((heads, T, T), generator=g) < 1.0 / 6).double()
        wd[:, t, t] = (1 - 2 * (t % 2)).double()
        if pattern == "cancel":
            assert swin_cancel_possible(H, W, ws, shift)
            first = ((y_ % ws) * ws + (x_ % ws)) < 8                         # window positions 0 .. 7
            xn = torch.where(first, torch.full_like(xn, CANCEL_BIG), xn)
            xn = torch.where(((y_ % ws) == 0) & ((x_ % ws) == 0), CANCEL_BIG + ((y_ // ws + x_ // ws + ch) % 4).double(), xn)
            wd[:, :, :8] = CANCEL_BIG
            wd[:, :, 0] = 1.0
            block = 7 * CANCEL_BIG * CANCEL_BIG + CANCEL_BIG
    c.xn, c.wd = xn, wd
    c.bias = (torch.arange(heads * T) * 5 % 7 - 3).double() - block
    rows = B * H * W
    ch1, r = torch.arange(C), torch.arange(rows)
    c.gamma, c.beta = torch.tensor([1.0, 2.0])[ch1 % 2].double(), (ch1 % 3 - 1).double()
    c.mean, c.rstd = (r % 4 - 1).double(), torch.ones(rows, dtype=torch.float64)
    c.x = (xn.reshape(rows, C) - c.beta[None, :]) / c.gamma[None, :] + c.mean[:, None]
    xp = torch.zeros((B, Hp, Wp, C), dtype=torch.float64)
    xp[:, pad_t:pad_t + H, pad_l:pad_l + W] = xn
    win = xp.reshape(B, Hp // ws, ws, Wp // ws, ws, C).permute(0, 1, 3, 2, 4, 5).reshape(-1, T, heads, 32)
    acc = torch.einsum("hts,wshc->wthc", wd, win)
    c.abs_terms = torch.einsum("hts,wshc->wthc", wd.abs(), win.abs()).max().item()
    yw = acc + c.bias.reshape(heads, T).t().reshape(1, T, heads, 1)

    def unwin(v):
        return v.reshape(B, Hp // ws, Wp // ws, ws, ws, C).permute(0, 1, 3, 2, 4, 5).reshape(B, Hp, Wp, C)[:, pad_t:pad_t + H, pad_l:pad_l + W].reshape(rows, C)
    c.acc, c.y = unwin(acc), unwin(yw)
    c.want = c.x + c.y
    c.padded = bool((Hp, Wp) != (H, W))
    return c


def check_swin_case(c):
    what = (c.pattern, str(c.dtype), c.geom)
    for name in ("x", "xn", "wd", "y", "want"):
        assert representable(getattr(c, name), c.dtype), (what, name)
    assert c.abs_terms * 2 + c.bias.abs().max().item() * 4 < ACC_LIMIT
    if c.pattern == "onehot":
        assert bool((c.wd.sum(1) == 1).all())                                # every position of every head is named
    elif c.pattern == "ternary":
        assert c.wd.abs().max().item() <= 2 and bool((c.wd.diagonal(dim1=1, dim2=2) != 0).all())
    else:
        assert c.acc.abs().min().item() > max(4096, INT_RANGE[c.dtype]) and not representable(c.acc, c.dtype), (what, "accumulator")
