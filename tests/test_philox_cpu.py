"""CPU: tests/philox_cpu.py against the Random123 known answers for Philox4x32-10, and the layout of the two documented streams."""
import numpy as np

import philox_cpu as P

KAT = [
    ((0, 0, 0, 0), (0, 0), (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
    ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
    ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1)),
]


def test_random123_known_answers():
    for ctr, key, out in KAT:
        got = P.philox4x32_10(ctr, key)
        assert got.dtype == np.uint32 and got.shape == (4,)
        assert tuple(int(v) for v in got) == out, [hex(int(v)) for v in got]


def test_vectorised_equals_scalar():
    """arrays of counters give, per element, what the scalar call gives (the known answers as one batch)"""
    ctr = [np.array([k[0][w] for k in KAT], dtype=np.uint64) for w in range(4)]
    for i, (c, key, out) in enumerate(KAT):
        got = P.philox4x32_10(ctr, key)
        assert got.shape == (3, 4) and tuple(int(v) for v in got[i]) == out


def test_dropout_stream_layout():
    seed, off = 0xDEADBEEFCAFEF00D, 2 ** 32 - 2
    u = P.dropout_uniforms(13, seed, off)
    assert u.dtype == np.float32 and u.shape == (13,) and (u >= 0).all() and (u < 1).all()
    # element 4 i + j is lane j of block offset + i; block 2 sits behind the carry into counter word 1
    for i, (lo, hi) in enumerate([(0xFFFFFFFE, 0), (0xFFFFFFFF, 0), (0, 1), (1, 1)]):
        r = P.philox4x32_10((lo, hi, P.DROPOUT_TAG, 0), (seed & 0xFFFFFFFF, seed >> 32))
        for j in range(4):
            if 4 * i + j < 13:
                assert u[4 * i + j] == np.float32(int(r[j]) >> 8) * np.float32(2.0 ** -24)
    assert P.dropout_keep(13, 0.0, seed, off).all()
    k = P.dropout_keep(4096, 0.5, seed, 0)
    assert 0.45 < k.mean() < 0.55
    assert np.array_equal(P.dropout_uniforms(8, seed, 3 << 40)[4:], P.dropout_uniforms(4, seed, (3 << 40) + 1))


def test_sample_step_stream_and_the_unit_draw():
    r = P.sample_step_r0(4, 5, 42, 3)
    assert r.shape == (4, 5)
    one = P.philox4x32_10((2, 0, 4, 6), (42, 0))
    assert int(r[2, 4]) == int(one[0])
    u = P.sample_step_u(4, 5, 42, 3)
    assert u.dtype == np.float32 and (u > 0).all() and (u <= 1).all()
    # the draw the q = 0 defect of muse_sample_step needed: seed 36, step 0, row 216, token 502 has its top 24 bits all ones
    r = P.sample_step_r0(217, 512, 36, 0)
    assert int(r[216, 502]) >> 8 == 0xFFFFFF
    assert P.sample_step_u(217, 512, 36, 0)[216, 502] == np.float32(1.0)
    q = P.sample_step_q(217, 512, 36, 0)
    assert q[216, 502] == 2.0 ** -25 and (q > 0).all() and q[216, 502] < -np.log(1.0 - 2.0 ** -24)
