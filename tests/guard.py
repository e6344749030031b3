"""Guard bands for the pitched / offset-pointer contract of include/mlpk.h (a plain helper module, like philox_ref.py and grad_digest.py).

A `Guarded` is ONE flat allocation of lead + rows * ld + tail elements with a logical (rows, cols) tensor inside it at storage offset `lead` and
row pitch `ld`.  Everything a kernel has no business touching -- the lead, the tail and the pad columns [cols, ld) of every row -- holds a NaN of a
fixed payload (POISON_GUARD); `check()` compares INTEGER views, so any write there is seen, whatever value it wrote, and an input's NaN padding read as
data turns the result non-finite (`assert_finite`).  lead and tail are at least one whole pitch row and at least MIN_BAND elements: a clamped or
vectorised over-read of a few elements stays inside memory the test owns.

  role "out"    the logical area holds a DIFFERENT NaN (POISON_LOGICAL): what the kernel did not write is still visible after the call
  role "inout"  the logical area holds `data` (operands updated in place); only the guard is checked
  role "in"     the logical area holds `data`; `check()` asserts the WHOLE buffer bit-unchanged.  `zero_cols=(lo, hi)` puts the zeros a contract
                demands (K padding of a packed operand) into pad columns [lo, hi) and NaN only beyond them
"""
import torch

MIN_BAND = 2048
# (guard, logical) NaN bit patterns per storage type: quiet NaNs with distinct payloads
POISON = {
    torch.float32: (0x7FC5A5A5, 0x7FDB1234),
    torch.float16: (0x7E5A, 0x7DA5),
    torch.bfloat16: (0x7FA5, 0x7FDB),
}
INT_VIEW = {torch.float32: torch.int32, torch.float16: torch.int16, torch.bfloat16: torch.int16}
LEAD_OFFSETS = (0, 4, 2, 1)          # multiple of 8 elements, = 4 mod 8, = 2 mod 4, odd


def lead_for(ld, offset=0):
    """smallest lead >= max(ld, MIN_BAND) that is a multiple of 8 elements, plus `offset` elements (one of LEAD_OFFSETS)"""
    assert offset in LEAD_OFFSETS
    return (max(int(ld), MIN_BAND) + 7) // 8 * 8 + offset


def _bits(dtype, pattern):
    """the bit pattern as a value of the signed integer type of the same width"""
    width = 32 if dtype == torch.float32 else 16
    return pattern - (1 << width) if pattern >= 1 << (width - 1) else pattern


class Guarded:
    def __init__(self, rows, cols, ld=None, dtype=torch.float32, device="cpu", lead=None, tail=None, role="out", data=None, zero_cols=None):
        ld = cols if ld is None else int(ld)
        assert role in ("out", "in", "inout") and rows > 0 and 0 < cols <= ld and dtype in POISON
        lead = lead_for(ld) if lead is None else int(lead)
        tail = lead_for(ld) if tail is None else int(tail)
        assert lead >= max(ld, MIN_BAND) and tail >= max(ld, MIN_BAND), "lead / tail: at least one pitch row and MIN_BAND elements"
        assert (data is not None) == (role != "out"), "role 'in' / 'inout' carry data, role 'out' does not"
        self.rows, self.cols, self.ld, self.lead, self.tail, self.role, self.dtype = rows, cols, ld, lead, tail, role, dtype
        n = lead + rows * ld + tail
        it = INT_VIEW[dtype]
        guard, logical = (_bits(dtype, p) for p in POISON[dtype])
        raw = torch.full((n,), guard, dtype=it, device=device)
        body = raw[lead:lead + rows * ld].view(rows, ld)
        mask = torch.ones((n,), dtype=torch.bool, device=device)             # positions check() compares
        if role == "out":
            body[:, :cols] = logical
        else:
            body[:, :cols] = data.detach().to(device=device, dtype=dtype).reshape(rows, cols).contiguous().view(it)
        if zero_cols is not None:
            assert role == "in" and cols <= zero_cols[0] <= zero_cols[1] <= ld
            body[:, zero_cols[0]:zero_cols[1]] = 0
        if role != "in":
            mask[lead:lead + rows * ld].view(rows, ld)[:, :cols] = False
        self._mask = mask
        self._expect = raw.clone()
        self.flat = raw.view(dtype)
        self.view = torch.as_strided(self.flat, (rows, cols), (ld, 1), lead)

    # ------------------------------------------------------------------ contents
    def dense(self):
        """the logical (rows, cols) contents, contiguous"""
        return self.view.clone().contiguous()

    def raw(self):
        return self.flat.view(INT_VIEW[self.dtype])

    def where(self, i):
        """flat element index -> words"""
        if i < self.lead:
            return "lead element %d (of %d, %d before the first row)" % (i, self.lead, self.lead - i)
        j = i - self.lead
        if j >= self.rows * self.ld:
            return "tail element %d (of %d)" % (j - self.rows * self.ld, self.tail)
        return "row %d, column %d (cols %d, ld %d)" % (j // self.ld, j % self.ld, self.cols, self.ld)

    def _first_bad(self, expect, mask, what):
        got = self.raw()
        bad = (got != expect) & mask
        if bool(bad.any()):
            i = int(torch.nonzero(bad)[0])
            width = 8 if self.dtype == torch.float32 else 4
            m = (1 << (4 * width)) - 1
            raise AssertionError("%s: %s holds 0x%0*x, expected 0x%0*x (%d elements differ)" % (
                what, self.where(i), width, int(got[i]) & m, width, int(expect[i]) & m, int(bad.sum())))

    def check(self, zero_cols=None):
        """out / inout: every guard element bit-identical to the poison; with zero_cols=(lo, hi) pad columns [lo, hi) of every row exactly +0
        and everything beyond them poison.  in: the whole buffer bit-unchanged."""
        expect = self._expect
        if zero_cols is not None:
            lo, hi = zero_cols
            assert self.role != "in" and self.cols <= lo <= hi <= self.ld
            expect = expect.clone()
            expect[self.lead:self.lead + self.rows * self.ld].view(self.rows, self.ld)[:, lo:hi] = 0
        self._first_bad(expect, self._mask, "input modified" if self.role == "in" else "guard band written")

    def still_poison(self, c0, c1, r0=0, r1=None):
        """role out: the logical columns [c0, c1) of rows [r0, r1) were NOT written (the gap between two slices, rows a call must skip)"""
        assert self.role == "out"
        r1 = self.rows if r1 is None else r1
        mask = torch.zeros_like(self._mask)
        mask[self.lead:self.lead + self.rows * self.ld].view(self.rows, self.ld)[r0:r1, c0:c1] = True
        self._first_bad(self._expect, mask, "unowned part of the output written")

    def all_poison(self):
        """role out: nothing at all was written (a refused call)"""
        assert self.role == "out"
        self._first_bad(self._expect, torch.ones_like(self._mask), "a refused call wrote")


def assert_finite(t, what="output"):
    """NaN from an input's padding must not have been read as data"""
    f = t.detach().float()
    bad = ~torch.isfinite(f)
    if bool(bad.any()):
        idx = torch.nonzero(bad)[0].tolist()
        raise AssertionError("%s is not finite at %s (%d elements): padding read as data, or elements left unwritten" % (what, idx, int(bad.sum())))


def assert_bits_equal(a, b, what="result"):
    """two tensors of one storage type, bit for bit"""
    assert a.dtype == b.dtype and a.shape == b.shape, (a.dtype, b.dtype, a.shape, b.shape)
    ia, ib = a.contiguous().view(INT_VIEW[a.dtype]), b.contiguous().view(INT_VIEW[b.dtype])
    bad = ia != ib
    if bool(bad.any()):
        idx = torch.nonzero(bad)[0].tolist()
        raise AssertionError("%s differs from the dense call at %s: %r vs %r (%d elements)" % (
            what, idx, float(a[tuple(idx)]), float(b[tuple(idx)]), int(bad.sum())))
