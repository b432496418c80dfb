"""NumPy restatement of the arithmetic include/sslcr.h defines for the six OpenCV-style ops of the v1 RandAugment pool
(sslcr_randaug_v1_slot): box blur, the 8-bit HSV shift, the fixed-point bicubic warp, the fixed-point bicubic resize and the
Philox / Box-Muller noise.  Written from the header's text alone; the kernels are held to it, and it is held to scipy, colorsys and
torch in tests/test_randaug_v1_cpu.py.  PARITY UNPINNED against OpenCV / albumentations / imgaug: none of them is installed.

Images are uint8 [H, W, 3] arrays."""
import numpy as np

F32 = np.float32


# ------------------------------------------------------------------------------------------------ borders
def reflect101(p, n):
    """cv::borderInterpolate(p, n, BORDER_REFLECT_101): the repeated reflection, any offset (array or int)"""
    p = np.asarray(p, dtype=np.int64)
    if n == 1:
        return np.zeros_like(p)
    period = 2 * n - 2
    m = np.mod(p, period)
    return np.where(m >= n, period - m, m)


# ------------------------------------------------------------------------------------------------ 1. box blur
def blur(img, k):
    h, w, _ = img.shape
    r = k // 2
    ys = reflect101(np.arange(-r, h + r), h)
    xs = reflect101(np.arange(-r, w + r), w)
    big = img[ys][:, xs].astype(np.int64)
    s = np.zeros((h, w, 3), np.int64)
    for dy in range(k):
        for dx in range(k):
            s += big[dy:dy + h, dx:dx + w]
    return ((2 * s + k * k) // (2 * k * k)).astype(np.uint8)


# ------------------------------------------------------------------------------------------------ 2. HSV shift
def hsv_tables():
    sdiv, hdiv = np.zeros(256, np.int64), np.zeros(256, np.int64)
    i = np.arange(1, 256, dtype=np.float64)
    sdiv[1:] = np.rint((255 << 12) / i).astype(np.int64)
    hdiv[1:] = np.rint((180 << 12) / (6.0 * i)).astype(np.int64)
    return sdiv, hdiv


def rgb_to_hsv8(img):
    """-> int64 h (0..179), s, v planes"""
    sdiv, hdiv = hsv_tables()
    r, g, b = (img[..., c].astype(np.int64) for c in range(3))
    v = np.maximum(r, np.maximum(g, b))
    diff = v - np.minimum(r, np.minimum(g, b))
    s = (diff * sdiv[v] + 2048) >> 12
    h = np.where(v == r, g - b, np.where(v == g, b - r + 2 * diff, r - g + 4 * diff))
    h = (h * hdiv[diff] + 2048) >> 12
    h = np.where(h < 0, h + 180, h)
    return h, s, v


def hsv8_to_rgb(h, s, v):
    """the float32 way back: h any integer 0..255 (half-degrees), s, v 0..255 -> uint8 [H, W, 3]"""
    hf = h.astype(F32) * F32(F32(6.0) / F32(180.0))
    hf = np.where(hf >= F32(6.0), hf - F32(6.0), hf).astype(F32)
    sec = np.floor(hf)
    f = (hf - sec).astype(F32)
    sec = sec.astype(np.int64)
    bad = (sec < 0) | (sec >= 6)
    sec = np.where(bad, 0, sec)
    f = np.where(bad, F32(0), f).astype(F32)
    k = F32(F32(1.0) / F32(255.0))
    sf, vf = s.astype(F32) * k, v.astype(F32) * k
    one = F32(1.0)
    tab = np.stack([vf, vf * (one - sf), vf * (one - sf * f), vf * (one - sf * (one - f))], -1).astype(F32)
    sector = np.array([[1, 3, 0], [1, 0, 2], [3, 0, 1], [0, 2, 1], [0, 1, 3], [2, 1, 0]])      # -> (b, g, r)
    idx = sector[sec]
    bgr = np.take_along_axis(tab, idx, -1)
    out = np.clip(np.rint(bgr * F32(255.0)), 0, 255).astype(np.uint8)
    return out[..., ::-1].copy()


def shift_hsv(img, dh, ds, dv):
    """dh, ds, dv: the integer shifts rint(draw)"""
    h, s, v = rgb_to_hsv8(img)
    h = h + int(dh)
    h = np.where(h < 0, 255 - h, h)
    h = np.where(h > 255, h - 255, h)
    s = np.clip(s + int(ds), 0, 255)
    v = np.clip(v + int(dv), 0, 255)
    return hsv8_to_rgb(h, s, v)


# ------------------------------------------------------------------------------------------------ cubic coefficients
def cubic_coeffs(x):
    """the four float32 weights of the A = -0.75 cubic at fraction x (float32 array) -> [..., 4]"""
    x = np.asarray(x, dtype=F32)
    A, one = F32(-0.75), F32(1.0)
    x1 = x + one
    c0 = ((A * x1 - F32(5) * A) * x1 + F32(8) * A) * x1 - F32(4) * A
    c1 = ((A + F32(2)) * x - (A + F32(3))) * x * x + one
    y = one - x
    c2 = ((A + F32(2)) * y - (A + F32(3))) * y * y + one
    c3 = one - c0 - c1 - c2
    return np.stack([c0, c1, c2, c3], -1).astype(F32)


def warp_table():
    """int16 [1024, 16]: entry [fy * 32 + fx][ky * 4 + kx]; bits as stored (entry 5 is read unsigned, see warp_weights)"""
    c = cubic_coeffs(np.arange(32, dtype=F32) * F32(1.0 / 32))
    tab = np.zeros((1024, 16), np.int64)
    for fy in range(32):
        for fx in range(32):
            v = (c[fy][:, None] * c[fx][None, :]).astype(F32)
            it = np.clip(np.rint(v * F32(32768.0)), -32768, 32767).astype(np.int64)
            diff = int(it.sum()) - 32768
            if diff:
                mk = Mk = (1, 1)
                for k1 in (1, 2):
                    for k2 in (1, 2):
                        if it[k1, k2] < it[mk]:
                            mk = (k1, k2)
                        elif it[k1, k2] > it[Mk]:
                            Mk = (k1, k2)
                if diff < 0:
                    it[Mk] -= diff
                else:
                    it[mk] -= diff
            tab[fy * 32 + fx] = it.reshape(-1)
    return (tab & 0xFFFF).astype(np.uint16).view(np.int16)


def warp_weights(tab):
    """the table as the integers the sum uses: int16, except entry 5 (the tap at (sx, sy), never negative), read as uint16"""
    w = tab.astype(np.int64)
    w[:, 5] = tab[:, 5].view(np.uint16).astype(np.int64)
    return w


# ------------------------------------------------------------------------------------------------ 3. bicubic warp
def rotation_matrix(cx, cy, angle, scale):
    import math
    a = angle * math.pi / 180
    al, be = math.cos(a) * scale, math.sin(a) * scale
    return [al, be, (1 - al) * cx - be * cy, -be, al, be * cx + (1 - al) * cy]


def invert_affine(m):
    m = [float(v) for v in m]
    D = m[0] * m[4] - m[1] * m[3]
    D = 1.0 / D if D != 0 else 0.0
    a11, a22 = m[4] * D, m[0] * D
    m[0], m[1], m[3], m[4] = a11, m[1] * -D, m[3] * -D, a22
    b1 = -m[0] * m[2] - m[1] * m[5]
    b2 = -m[3] * m[2] - m[4] * m[5]
    m[2], m[5] = b1, b2
    return m


def warp_coords(M, h, w):
    """-> X, Y int64 [h, w]: source coordinates in 1/32 pixel"""
    M = [np.float64(v) for v in M]
    x, y = np.arange(w, dtype=np.float64), np.arange(h, dtype=np.float64)

    def sat(v):
        return np.clip(np.rint(v), -2147483648, 2147483647).astype(np.int64)
    X = (sat((M[1] * y + M[2]) * 1024.0)[:, None] + 16 + sat(M[0] * x * 1024.0)[None, :]) >> 5
    Y = (sat((M[4] * y + M[5]) * 1024.0)[:, None] + 16 + sat(M[3] * x * 1024.0)[None, :]) >> 5
    return X, Y


def warp_affine(img, M, fx=0, fy=0, tab=None):
    """M: the six doubles of the INVERSE map; (fx, fy): the source is flipped horizontally / vertically first"""
    h, w, _ = img.shape
    wt = warp_weights(warp_table() if tab is None else tab)
    X, Y = warp_coords(M, h, w)
    sx, sy = X >> 5, Y >> 5
    wgt = wt[(Y & 31) * 32 + (X & 31)]                         # [h, w, 16]
    acc = np.zeros((h, w, 3), np.int64)
    for ky in range(4):
        yy = reflect101(sy - 1 + ky, h)
        if fy:
            yy = h - 1 - yy
        for kx in range(4):
            xx = reflect101(sx - 1 + kx, w)
            if fx:
                xx = w - 1 - xx
            acc += img[yy, xx].astype(np.int64) * wgt[..., ky * 4 + kx, None]
    return np.clip((acc + 16384) >> 15, 0, 255).astype(np.uint8)


# ------------------------------------------------------------------------------------------------ 4. bicubic resize
def resize_axis(src, dst):
    """-> (int64 [dst, 4] clamped tap indices, int64 [dst, 4] 11-bit coefficients)"""
    d = np.arange(dst, dtype=np.float64)
    f = ((d + 0.5) * (np.float64(src) / np.float64(dst)) - 0.5).astype(F32)
    s = np.floor(f)
    c = cubic_coeffs((f - s).astype(F32))
    co = np.clip(np.rint(c * F32(2048.0)), -32768, 32767).astype(np.int64)
    idx = np.clip(s.astype(np.int64)[:, None] + np.arange(-1, 3)[None, :], 0, src - 1)
    return idx, co


def resize(img, dh, dw):
    sh, sw, _ = img.shape
    xi, xc = resize_axis(sw, dw)
    yi, yc = resize_axis(sh, dh)
    a = img.astype(np.int64)
    hor = (a[:, xi] * xc[None, :, :, None]).sum(2)              # [sh, dw, 3]
    ver = (hor[yi] * yc[:, :, None, None]).sum(1)               # [dh, dw, 3]
    return np.clip((ver + (1 << 21)) >> 22, 0, 255).astype(np.uint8)


def scale_resize_crop(img, s1, y1, x1):
    """resize S -> s1, resize s1 -> S + 20, crop S at (y1, x1)"""
    S = img.shape[0]
    assert img.shape[1] == S and s1 >= 1
    big = resize(resize(img, s1, s1), S + 20, S + 20)
    return big[y1:y1 + S, x1:x1 + S].copy()


# ------------------------------------------------------------------------------------------------ 5. Gaussian noise
def philox4x32(counters, seed):
    """Philox4x32-10: counters uint32 [n] (word 0; words 1..3 are 0), key = the 64-bit seed -> uint32 [n, 4]"""
    M0, M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
    c = [np.asarray(counters, dtype=np.uint64) & np.uint64(0xFFFFFFFF)] + [np.zeros(len(counters), np.uint64) for _ in range(3)]
    k0, k1 = int(seed) & 0xFFFFFFFF, (int(seed) >> 32) & 0xFFFFFFFF
    mask = np.uint64(0xFFFFFFFF)
    for _ in range(10):
        p0, p1 = M0 * c[0], M1 * c[2]
        hi0, lo0, hi1, lo1 = p0 >> np.uint64(32), p0 & mask, p1 >> np.uint64(32), p1 & mask
        c = [hi1 ^ c[1] ^ np.uint64(k0), lo1, hi0 ^ c[3] ^ np.uint64(k1), lo0]
        k0, k1 = (k0 + 0x9E3779B9) & 0xFFFFFFFF, (k1 + 0xBB67AE85) & 0xFFFFFFFF
    return np.stack(c, -1).astype(np.uint32)


def noise_normals(npix, seed):
    """-> (float32 z [npix], uint32 words [ceil(npix / 4), 4])"""
    nq = (npix + 3) // 4
    w = philox4x32(np.arange(nq), seed)
    two24 = F32(2.0 ** -24)

    def pair(a, b):
        u1 = ((a >> 8) + 1).astype(F32) * two24
        u2 = (b >> 8).astype(F32) * two24
        r = np.sqrt(F32(-2.0) * np.log(u1)).astype(F32)
        th = (F32(6.2831853071795864769) * u2).astype(F32)
        return (r * np.cos(th)).astype(F32), (r * np.sin(th)).astype(F32)
    z0, z1 = pair(w[:, 0], w[:, 1])
    z2, z3 = pair(w[:, 2], w[:, 3])
    return np.stack([z0, z1, z2, z3], -1).reshape(-1)[:npix], w


def gaussian_noise(img, sigma, seed):
    """-> (uint8 out, float64 sigma * z per pixel [H, W])"""
    h, w, _ = img.shape
    z, _ = noise_normals(h * w, seed)
    sz = np.float64(sigma) * z.astype(np.float64).reshape(h, w)
    out = np.clip(img.astype(np.int64) + np.rint(sz).astype(np.int64)[..., None], 0, 255).astype(np.uint8)
    return out, sz
