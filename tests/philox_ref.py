"""NumPy restatement of the engine's documented noise streams (include/vitsmi.h, csrc/kernels.hip.hpp: philox_normal4):
Philox4x32-10 blocks, their four words as float32 uniforms in (0, 1], two Box-Muller pairs per block.  row_noise / flat_noise
do the Box-Muller arithmetic in float32 as the device does; the *64 variants evaluate it in float64 from the same float32
uniforms and the same float32-rounded angle, so they differ from the device by the device's logf / sqrtf / cosf / sinf
errors alone."""
import numpy as np

M32 = np.uint64(0xFFFFFFFF)


def philox4x32_10(c0, c1, c2, c3, key):
    c = [np.asarray(x, np.uint64) & M32 for x in (c0, c1, c2, c3)]
    k0, k1 = np.uint64(key & 0xFFFFFFFF), np.uint64(key >> 32)
    for _ in range(10):
        p0 = np.uint64(0xD2511F53) * c[0]
        p1 = np.uint64(0xCD9E8D57) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k0, p1 & M32, (p0 >> np.uint64(32)) ^ c[3] ^ k1, p0 & M32]
        k0 = (k0 + np.uint64(0x9E3779B9)) & M32
        k1 = (k1 + np.uint64(0xBB67AE85)) & M32
    return c


def row_noise(seed, stream, channels, n):
    """[channels, n]: element (ch, pos) = v[pos & 3] of Philox4x32-10(counter (pos >> 2, ch, stream, 0), key seed) + Box-Muller"""
    p4 = np.arange((n + 3) // 4, dtype=np.uint64)[None, :]
    ch = np.arange(channels, dtype=np.uint64)[:, None]
    r = philox4x32_10(np.broadcast_to(p4, (channels, p4.shape[1])), np.broadcast_to(ch, (channels, p4.shape[1])),
                      np.uint64(stream), np.uint64(0), int(seed))
    k = np.float32(2.3283064365386963e-10)
    u = [(x.astype(np.float32) + np.float32(0.5)) * k for x in r]
    u0 = np.minimum(np.maximum(u[0], np.float32(1e-12)), np.float32(1.0))
    u2 = np.minimum(np.maximum(u[2], np.float32(1e-12)), np.float32(1.0))
    ra, rb = np.sqrt(np.float32(-2.0) * np.log(u0)), np.sqrt(np.float32(-2.0) * np.log(u2))
    tp = np.float32(6.283185307179586)
    v = np.stack([ra * np.cos(tp * u[1]), ra * np.sin(tp * u[1]), rb * np.cos(tp * u[3]), rb * np.sin(tp * u[3])], -1)
    return v.reshape(channels, -1)[:, :n].astype(np.float32)


def _row_words(seed, stream, channels, n):
    p4 = np.arange((n + 3) // 4, dtype=np.uint64)[None, :]
    ch = np.arange(channels, dtype=np.uint64)[:, None]
    return philox4x32_10(np.broadcast_to(p4, (channels, p4.shape[1])), np.broadcast_to(ch, (channels, p4.shape[1])),
                         np.uint64(stream), np.uint64(0), int(seed))


def _flat_words(seed, stream_id, n):
    i4 = np.arange((n + 3) // 4, dtype=np.uint64)
    sid = int(stream_id)
    return philox4x32_10(i4 & M32, i4 >> np.uint64(32), np.uint64(sid & 0xFFFFFFFF), np.uint64(sid >> 32), int(seed))


def _uniforms(r):
    k = np.float32(2.3283064365386963e-10)
    u = [(x.astype(np.float32) + np.float32(0.5)) * k for x in r]
    u[0] = np.minimum(np.maximum(u[0], np.float32(1e-12)), np.float32(1.0))
    u[2] = np.minimum(np.maximum(u[2], np.float32(1e-12)), np.float32(1.0))
    assert all(x.dtype == np.float32 for x in u)
    return u


def _box_muller32(r):
    u = _uniforms(r)
    ra, rb = np.sqrt(np.float32(-2.0) * np.log(u[0])), np.sqrt(np.float32(-2.0) * np.log(u[2]))
    tp = np.float32(6.283185307179586)
    return np.stack([ra * np.cos(tp * u[1]), ra * np.sin(tp * u[1]), rb * np.cos(tp * u[3]), rb * np.sin(tp * u[3])], -1)


def _box_muller64(r):
    """(values, radii), both float64 [..., 4]: the float32 uniforms and the float32-rounded angles of the device, everything
    behind them in float64"""
    u = _uniforms(r)
    tp = np.float32(6.283185307179586)
    a1, a3 = (tp * u[1]).astype(np.float64), (tp * u[3]).astype(np.float64)
    ra, rb = np.sqrt(-2.0 * np.log(u[0].astype(np.float64))), np.sqrt(-2.0 * np.log(u[2].astype(np.float64)))
    return (np.stack([ra * np.cos(a1), ra * np.sin(a1), rb * np.cos(a3), rb * np.sin(a3)], -1),
            np.stack([ra, ra, rb, rb], -1))


def row_noise64(seed, stream, channels, n):
    """row_noise's elements in float64, and each element's Box-Muller radius sqrt(-2 ln u): two [channels, n]"""
    v, ra = _box_muller64(_row_words(seed, stream, channels, n))
    return v.reshape(channels, -1)[:, :n], ra.reshape(channels, -1)[:, :n]


def flat_noise(seed, stream_id, n):
    """[n] float32, the stream of calls without per-utterance seeds: element i = v[i & 3] of Philox4x32-10(counter
    (lo32(i >> 2), hi32(i >> 2), lo32(stream_id), hi32(stream_id)), key seed) + Box-Muller"""
    return _box_muller32(_flat_words(seed, stream_id, n)).reshape(-1)[:n].astype(np.float32)


def flat_noise64(seed, stream_id, n):
    """flat_noise's elements in float64, and each element's Box-Muller radius: two [n]"""
    v, ra = _box_muller64(_flat_words(seed, stream_id, n))
    return v.reshape(-1)[:n], ra.reshape(-1)[:n]
