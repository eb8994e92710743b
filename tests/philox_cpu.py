"""Vectorised numpy Philox4x32-10 (Salmon et al. 2011, the Random123 generator) and the two random streams libmuse_hip documents,
restated on the CPU: the oracle of tests/test_gpu_row_edges.py for muse_dropout's keep masks and muse_sample_step's device draws,
pinned against the Random123 known answers by tests/test_philox_cpu.py.

Two layers:
  * the generator: `philox4x32_10(counter, key)` over arrays of counters (uint64 arithmetic, every word masked to 32 bits);
  * the streams: `dropout_uniforms` / `dropout_keep` (include/muse_hip.h, muse_dropout) and `sample_step_r0` / `sample_step_u` /
    `sample_step_q` (muse_sample_step with noise_exp == NULL).
"""
import numpy as np

M32 = np.uint64(0xFFFFFFFF)
_MUL0, _MUL1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
_W0, _W1 = 0x9E3779B9, 0xBB67AE85
DROPOUT_TAG = 0x6D757365   # counter word 2 of the dropout stream


def _words(a):
    return np.asarray(a, dtype=np.uint64) & M32


def philox4x32_10(counter, key):
    """counter: 4 arrays (or scalars) of 32-bit words, key: 2; broadcast against each other -> uint32 array [..., 4]"""
    c0, c1, c2, c3 = np.broadcast_arrays(*[_words(c) for c in counter])
    k0, k1 = int(key[0]) & 0xFFFFFFFF, int(key[1]) & 0xFFFFFFFF
    for _ in range(10):
        p0, p1 = _MUL0 * c0, _MUL1 * c2          # 32 x 32 -> 64 bit products: no overflow in uint64
        n0 = (p1 >> np.uint64(32)) ^ c1 ^ np.uint64(k0)
        n2 = (p0 >> np.uint64(32)) ^ c3 ^ np.uint64(k1)
        c0, c1, c2, c3 = n0, p1 & M32, n2, p0 & M32
        k0, k1 = (k0 + _W0) & 0xFFFFFFFF, (k1 + _W1) & 0xFFFFFFFF
    return np.stack([c0, c1, c2, c3], axis=-1).astype(np.uint32)


def _split64(v):
    """python ints / uint64 array -> (low word, high word) as uint64 arrays"""
    v = np.asarray(v, dtype=np.uint64)
    return v & M32, v >> np.uint64(32)


def dropout_uniforms(n, seed, offset):
    """u [n] float32 of muse_dropout(seed, offset): Philox block i has counter (lo(offset + i), hi(offset + i), DROPOUT_TAG, 0) and key
    (lo(seed), hi(seed)); its lane j serves element 4 i + j; u = (r >> 8) * 2^-24 in [0, 1)"""
    nblk = (n + 3) // 4
    c = np.uint64(int(offset) & (2 ** 64 - 1)) + np.arange(nblk, dtype=np.uint64)   # wraps modulo 2^64 like the kernel's uint64_t
    lo, hi = _split64(c)
    seed = int(seed) & (2 ** 64 - 1)
    r = philox4x32_10((lo, hi, DROPOUT_TAG, 0), (seed & 0xFFFFFFFF, seed >> 32))
    u = (r >> np.uint32(8)).astype(np.float32) * np.float32(2.0 ** -24)
    return u.reshape(-1)[:n]


def dropout_keep(n, p, seed, offset):
    """keep mask [n] bool: u >= p, compared in float32 like the kernel"""
    return dropout_uniforms(n, seed, offset) >= np.float32(p)


def sample_step_r0(rows, vocab, seed, step):
    """word 0 of the Philox block behind the categorical draw of (row, token j): counter (lo(row), hi(row), j, 2 * step), key
    (lo(seed), hi(seed)) -> uint32 [rows, vocab]"""
    lo, hi = _split64(np.arange(rows, dtype=np.uint64)[:, None])
    j = np.arange(vocab, dtype=np.uint64)[None, :]
    seed = int(seed) & (2 ** 64 - 1)
    return philox4x32_10((lo, hi, j, (2 * int(step)) & 0xFFFFFFFF), (seed & 0xFFFFFFFF, seed >> 32))[..., 0]


def sample_step_u(rows, vocab, seed, step):
    """u = ((r.x >> 8) + 1) * 2^-24 in (0, 1], float32 (exact: at most 25 significant bits only at u == 1)"""
    r = sample_step_r0(rows, vocab, seed, step)
    return ((r >> np.uint32(8)).astype(np.float32) + np.float32(1.0)) * np.float32(2.0 ** -24)


def sample_step_q(rows, vocab, seed, step):
    """q ~ Exp(1) as muse_sample_step draws it: -log(u) (float64 here), and 2^-25 for the draw u == 1 - strictly positive, below the
    next smallest draw -log(1 - 2^-24)"""
    u = sample_step_u(rows, vocab, seed, step).astype(np.float64)
    return np.where(u < 1.0, -np.log(np.minimum(u, 1.0 - 2.0 ** -24)), 2.0 ** -25)
