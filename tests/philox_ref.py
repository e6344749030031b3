"""numpy restatement of Philox4x32-10 and of mlpk_dropout's keep rule (include/mlpk.h): the mask of logical element e = r * cols + c is
word (e & 3) of philox(counter = (lo32(e >> 2), hi32(e >> 2), site, 0), key = (lo32(seed), hi32(seed))), kept iff word >= floor(p * 2^32).
Shared by the dropout tests and tests/golden/make_dropout_golden.py."""
import numpy as np

M0, M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK32 = np.uint64(0xFFFFFFFF)


def philox4x32_10(ctr, key):
    """ctr: (n, 4) uint32-valued, key: (n, 2) or (2,) -> (n, 4) uint32"""
    c = [np.asarray(ctr, dtype=np.uint64)[..., i].copy() for i in range(4)]
    key = np.broadcast_to(np.asarray(key, dtype=np.uint64), c[0].shape + (2,))
    k0, k1 = key[..., 0].copy(), key[..., 1].copy()
    for _ in range(10):
        p0, p1 = M0 * c[0], M1 * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k0, p1 & MASK32, (p0 >> np.uint64(32)) ^ c[3] ^ k1, p0 & MASK32]
        k0, k1 = (k0 + np.uint64(W0)) & MASK32, (k1 + np.uint64(W1)) & MASK32
    return np.stack(c, -1).astype(np.uint32)


def dropout_words(seed, site, e):
    """the 32-bit word of each logical element index in e (int64 array)"""
    e = np.asarray(e, dtype=np.uint64)
    g = e >> np.uint64(2)
    ctr = np.stack([g & MASK32, g >> np.uint64(32), np.full_like(g, site), np.zeros_like(g)], -1)
    seed = int(seed)
    words = philox4x32_10(ctr, (seed & 0xFFFFFFFF, seed >> 32))
    return np.take_along_axis(words, (e & np.uint64(3)).astype(np.int64)[..., None], -1)[..., 0]


def threshold(p):
    return int(np.floor(float(p) * 2.0 ** 32))


def keep_mask(seed, site, p, rows, cols):
    """bool (rows, cols): True where mlpk_dropout keeps the element"""
    e = np.arange(rows * cols, dtype=np.int64)
    return (dropout_words(seed, site, e).astype(np.int64) >= threshold(p)).reshape(rows, cols)


def scale(p):
    return np.float32(1.0 / (1.0 - p)) if p < 1.0 else np.float32(0.0)


# ---- the gradient fixtures of make_dropout_golden.py ----------------------------------------------------------------------------------------
FULL_GRAD = 512         # gradients of at most this many entries are stored whole
GRAD_SAMPLES = 256      # of larger ones: this many entries at evenly spaced flat indices, plus the tensor's max |g| and L2 norm


def grad_sample_index(n):
    """the flat indices a fixture keeps of an n-entry gradient (all of them up to FULL_GRAD)"""
    if n <= FULL_GRAD:
        return np.arange(n, dtype=np.int64)
    return np.unique(np.linspace(0, n - 1, GRAD_SAMPLES).round().astype(np.int64))
