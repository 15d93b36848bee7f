"""CPU: the restatement of the device frame source (oracle/frame_source.py) on its own.

tests/test_frame_source_gpu.py compares sim.hip with the restatement value by value, so the statistical questions about the
frames every BER figure rests on are asked here, once, of the restatement: is the generator Philox4x32-10 (Random123's
known-answer vectors), is the noise standard normal and uncorrelated across frames, positions, Box-Muller partners and the
message stream, and do the high counter word, the high key word and the stream word each change the output.

The seed is fixed, so every statistic below is a constant: it holds or it does not.  Bar: 4.5 of its own standard errors."""
import math

import numpy as np
import pytest

from oracle import frame_source as fs

SEED, FRAMES, POSITIONS = 0x5EEDC0DE, 2048, 1408
K = POSITIONS            # a message bit for every noise position
BAR = 4.5


def _words(s):
    return [int(x, 16) for x in s.split()]


@pytest.mark.parametrize("counter,key,want", [
    ("0 0 0 0", "0 0", "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
    ("ffffffff ffffffff ffffffff ffffffff", "ffffffff ffffffff", "408f276d 41c83b0e a20bc7c6 6d5451fd"),
    ("243f6a88 85a308d3 13198a2e 03707344", "a4093822 299f31d0", "d16cfe09 94fdcceb 5001e420 24126ea1"),
])
def test_philox4x32_10_known_answers(counter, key, want):
    """Random123's kat_vectors for philox4x32_10"""
    got = fs.philox4x32_10(_words(counter), _words(key))
    assert [int(x) for x in got] == _words(want)


def test_philox_vectorised_equals_one_at_a_time():
    rng = np.random.default_rng(1)
    c = rng.integers(0, 2 ** 32, size=(4, 5, 3), dtype=np.uint64)
    k = rng.integers(0, 2 ** 32, size=(2, 5, 3), dtype=np.uint64)
    got = fs.philox4x32_10(c, k)
    for i in range(5):
        for j in range(3):
            assert np.array_equal(got[:, i, j], fs.philox4x32_10(c[:, i, j], k[:, i, j]))


@pytest.fixture(scope="module")
def sample():
    """2048 frames x 1408 positions of noise (2.88 M samples) and as many message bits of the same frames"""
    z, rad = fs.normals(SEED, np.arange(FRAMES), POSITIONS)
    bits = fs.message_bits(SEED, np.arange(FRAMES), K)
    z.setflags(write=False); rad.setflags(write=False); bits.setflags(write=False)
    return z, rad, bits


def _check(name, value, stderr):
    t = value / stderr
    print(f"{name}: {t:+.2f} standard errors")
    assert abs(t) <= BAR, (name, t)


def test_noise_moments(sample):
    z = sample[0]
    n = z.size
    assert n == FRAMES * POSITIONS and np.isfinite(z).all()
    _check("mean", z.mean(), 1 / math.sqrt(n))
    _check("variance - 1", (z ** 2).mean() - z.mean() ** 2 - 1.0, math.sqrt(2 / n))
    _check("third moment", (z ** 3).mean(), math.sqrt(15 / n))
    _check("fourth moment - 3", (z ** 4).mean() - 3.0, math.sqrt(96 / n))


@pytest.mark.parametrize("t", [2, 3, 4])
def test_noise_tails(sample, t):
    z = sample[0]
    expect = z.size * 0.5 * math.erfc(t / math.sqrt(2.0))           # n Q(t)
    _check(f"count above +{t}", (z > t).sum() - expect, math.sqrt(expect))
    _check(f"count below -{t}", (z < -t).sum() - expect, math.sqrt(expect))


def test_noise_is_uncorrelated(sample):
    z = sample[0]
    a, b = z[:-1], z[1:]
    _check("frame f with f+1", (a * b).mean(), 1 / math.sqrt(a.size))
    for d in (1, 2, 4):
        a, b = z[:, :-d], z[:, d:]
        _check(f"position n with n+{d}", (a * b).mean(), 1 / math.sqrt(a.size))
    # the two samples of a Box-Muller pair share a radius: uncorrelated, and their squares must be too
    p = z.reshape(FRAMES, POSITIONS // 2, 2)
    q = (p[..., 0] ** 2 - 1.0) * (p[..., 1] ** 2 - 1.0)
    _check("z^2 - 1 of the two samples of a pair", q.mean(), 2 / math.sqrt(q.size))


def test_radius_is_the_pairs(sample):
    z, rad, _ = sample
    p, r = z.reshape(FRAMES, POSITIONS // 2, 2), rad.reshape(FRAMES, POSITIONS // 2, 2)
    assert np.array_equal(r[..., 0], r[..., 1])
    assert np.allclose(np.hypot(p[..., 0], p[..., 1]), r[..., 0], rtol=1e-12, atol=1e-300)


def test_message_bits_are_fair_and_independent_of_the_noise(sample):
    z, _, bits = sample
    n = bits.size
    assert n == FRAMES * K
    _check("message-bit mean - 1/2", bits.mean() - 0.5, 0.5 / math.sqrt(n))
    _check("(2 bit - 1) x noise at the same position", ((2.0 * bits - 1.0) * z[:, :K]).mean(), 1 / math.sqrt(n))


def test_message_layout_and_mask():
    """bit i of word w is message bit 32 w + i; the last word is masked to k; a shorter k is a prefix"""
    f = np.array([5, 6, 2 ** 40 + 1], dtype=np.uint64)
    w = fs.message_words(SEED, f, 100)
    assert w.shape == (3, 4) and w.dtype == np.uint32 and (w[:, 3] >> 4 == 0).all()
    b = fs.message_bits(SEED, f, 100)
    assert b.shape == (3, 100)
    for i in (0, 31, 32, 99):
        assert np.array_equal(b[:, i], (w[:, i // 32] >> np.uint32(i % 32)) & 1)
    full = fs.message_words(SEED, f, 128)
    assert np.array_equal(full[:, :3], w[:, :3]) and np.array_equal(full[:, 3] & np.uint32(0xF), w[:, 3])
    # word w is output word 0 of counter (f lo, f hi, w, 0) under key (seed lo, seed hi)
    assert int(full[2, 1]) == int(fs.philox4x32_10([1, 2 ** 8, 1, 0], [SEED, 0])[0])


def test_noise_layout():
    """normal i of group g lands at position 4 g + i; an n_tx that is no multiple of 4 is a prefix"""
    z, rad = fs.normals(7, [3], 12)
    r = fs.philox4x32_10([3, 0, 2, 1], [7, 0]).astype(np.float64)
    ua, ub, uc, ud = (r[0] + 1) / 2 ** 32, r[1] / 2 ** 32, (r[2] + 1) / 2 ** 32, r[3] / 2 ** 32
    want = [math.sqrt(-2 * math.log(ua)) * math.cos(2 * math.pi * ub), math.sqrt(-2 * math.log(ua)) * math.sin(2 * math.pi * ub),
            math.sqrt(-2 * math.log(uc)) * math.cos(2 * math.pi * ud), math.sqrt(-2 * math.log(uc)) * math.sin(2 * math.pi * ud)]
    assert np.allclose(z[0, 8:12], want, rtol=0, atol=1e-6)          # (the float32 rounding of the uniforms: < 2^-24 relative)
    z2, rad2 = fs.normals(7, [3], 10)
    assert np.array_equal(z2, z[:, :10]) and np.array_equal(rad2, rad[:, :10])


def test_frames_seeds_and_streams_differ():
    k, n = 256, 256
    # the high counter word: frame 0 and frame 2^32
    m = fs.message_words(SEED, [0, 2 ** 32], k)
    z, _ = fs.normals(SEED, [0, 2 ** 32], n)
    assert (m[0] != m[1]).mean() > 0.9 and (z[0] != z[1]).mean() > 0.9
    # the high key word: seeds s and s + 2^32
    m2 = fs.message_words(SEED + 2 ** 32, [0, 2 ** 32], k)
    z2, _ = fs.normals(SEED + 2 ** 32, [0, 2 ** 32], n)
    assert (m != m2).mean() > 0.9 and (z != z2).mean() > 0.9
    # the stream word: stream 0 and stream 1 of the same (frame, index)
    s0 = fs.philox4x32_10([9, 0, np.arange(64), 0], [SEED, 0])
    s1 = fs.philox4x32_10([9, 0, np.arange(64), 1], [SEED, 0])
    assert (s0 != s1).mean() > 0.9
    # and two neighbouring frames
    za, _ = fs.normals(SEED, [17, 18], n)
    assert (za[0] != za[1]).mean() > 0.9


def test_llr_scaling():
    """sigma^2 = 1/(2 R 10^(dB/10)), R = k/n_tx; sg and sc are float32-rounded; the tail is zero"""
    k, n_tx, N = 1024, 1280, 1408
    sg, sc = fs.scales(k, n_tx, 3.0)
    s2 = 1.0 / (2 * 0.8 * 10 ** 0.3)
    assert sg == float(np.float32(math.sqrt(s2))) and sc == float(np.float32(2 / s2))
    cw = np.zeros((2, n_tx), np.uint8); cw[1] = 1
    llr, rad, sg2, sc2 = fs.llrs(SEED, [4, 4], cw, k, n_tx, N, 3.0)
    z, _ = fs.normals(SEED, [4], n_tx)
    assert (sg2, sc2) == (sg, sc) and llr.shape == (2, N) and (llr[:, n_tx:] == 0).all()
    assert np.array_equal(llr[0, :n_tx], sc * (-1.0 + sg * z[0])) and np.array_equal(llr[1, :n_tx], sc * (1.0 + sg * z[0]))
