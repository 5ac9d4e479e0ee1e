"""numpy restatement of the record_data map images (emba_amd/csrc/render_kernels.h), the rule the device render is tested against:
Gx / Gy / map_poisson = io.normalize_robust; G_hsv = the min-max normalised (0.5*angle, 255, magnitude) through OpenCV's 8-bit HSV -> RGB, in float32.
(OpenCV's cartToPolar uses an approximate arctangent: this is the project's definition, not pinned against the reference.)"""
import numpy as np

from emba_amd import io as eio

DBL_EPSILON = np.finfo(np.float64).eps


def polar_half(gx, gy):
    a = np.arctan2(gy, gx) * (180.0 / np.pi)
    a = np.where(a < 0.0, a + 360.0, a)
    return 0.5 * a, np.sqrt(gx * gx + gy * gy)


def minmax_u8(v, a):
    """cv::normalize(v, dst, 0, a, NORM_MINMAX, CV_8U): sat(rint(v*s + t)), s = a*(1/(max-min)) (0 below DBL_EPSILON), t = 0 - min*s."""
    mn, mx = float(v.min()), float(v.max())
    d = mx - mn
    s = a * (1.0 / d) if d > DBL_EPSILON else 0.0
    t = 0.0 - mn * s
    return np.clip(np.rint(v * s + t), 0, 255).astype(np.uint8)


def hsv_to_rgb(H, S, V):
    """OpenCV's 8-bit HSV -> RGB with hue range 180, float32; returns (..., 3) uint8 in R, G, B order."""
    f = np.float32
    h = H.astype(f) * (f(6) / f(180))
    s = S.astype(f) * (f(1) / f(255))
    v = V.astype(f) * (f(1) / f(255))
    sector = np.floor(h)
    h = (h - sector).astype(f)
    sector = sector.astype(np.int64)
    bad = (sector < 0) | (sector >= 6)
    sector = np.where(bad, 0, sector)
    h = np.where(bad, f(0), h).astype(f)
    one = f(1)
    tab = np.stack([v, v * (one - s), v * (one - s * h), v * (one - s * (one - h))]).astype(f)
    sd = np.array([[1, 3, 0], [1, 0, 2], [3, 0, 1], [0, 2, 1], [0, 1, 3], [2, 1, 0]])
    idx = sd[sector]                                        # (..., 3): (b, g, r) entries of tab
    b = np.take_along_axis(tab, idx[None, ..., 0], 0)[0]
    g = np.take_along_axis(tab, idx[None, ..., 1], 0)[0]
    r = np.take_along_axis(tab, idx[None, ..., 2], 0)[0]
    return np.stack([np.clip(np.rint(c * f(255)), 0, 255).astype(np.uint8) for c in (r, g, b)], axis=-1)


def hsv_channels(gx, gy):
    half, mag = polar_half(gx, gy)
    return minmax_u8(half, 179.0), minmax_u8(mag, 255.0)


def render_np(gx, gy, M=None, pct=0.1):
    Hc, Vc = hsv_channels(gx, gy)
    out = {"Gx": eio.normalize_robust(gx, pct), "Gy": eio.normalize_robust(gy, pct),
           "G_hsv": hsv_to_rgb(Hc, np.full_like(Hc, 255), Vc), "map_poisson": None}
    if M is not None:
        out["map_poisson"] = eio.normalize_robust(M, pct)
    return out


def ranks_f32(n, pct=0.1):
    """io.normalize_robust's float32 rank arithmetic."""
    f = np.float32
    q = f(f(0.5) * f(pct) / f(100.0))
    return int(q * f(n)), min(int(f(f(1.0) - f(0.5) * f(pct) / f(100.0)) * f(n)), n - 1)


def ranks_f64(n, pct=0.1):
    """image_util::minMaxLocRobust's own form (image_utils.cpp:22-23): 0.5f*double/100.f*total in double."""
    return int((0.5 * pct / 100.0) * n), min(int((1.0 - 0.5 * pct / 100.0) * n), n - 1)


def decode_png(path):
    """Minimal PNG reader for the files io.save_png writes (8-bit grey / RGB, filter 0, no interlace), with the standard library only."""
    import struct
    import zlib
    data = open(path, "rb").read()
    assert data[:8] == b"\x89PNG\r\n\x1a\n"
    pos, idat, hdr = 8, b"", None
    while pos < len(data):
        ln, = struct.unpack(">I", data[pos:pos + 4])
        tag, body = data[pos + 4:pos + 8], data[pos + 8:pos + 8 + ln]
        crc, = struct.unpack(">I", data[pos + 8 + ln:pos + 12 + ln])
        assert crc == zlib.crc32(tag + body) & 0xFFFFFFFF, tag
        if tag == b"IHDR":
            hdr = struct.unpack(">IIBBBBB", body)
        elif tag == b"IDAT":
            idat += body
        pos += 12 + ln
        if tag == b"IEND":
            break
    w, h, depth, color, _, _, interlace = hdr
    assert depth == 8 and color in (0, 2) and interlace == 0
    ch = 1 if color == 0 else 3
    raw = np.frombuffer(zlib.decompress(idat), np.uint8).reshape(h, 1 + w * ch)
    assert (raw[:, 0] == 0).all()
    img = raw[:, 1:].reshape(h, w, ch) if ch == 3 else raw[:, 1:].reshape(h, w)
    return img.copy()
