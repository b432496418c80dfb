"""NumPy restatement of the two histopathology ops of the RSP v2 RandAugment pool -- ``hed`` (Pretraining_v2/models/randaugment.py:135-144)
and ``hsv`` (:125-132) -- and of the draw order of the whole pool with them in it.  Test infrastructure: it imports neither the
reference nor scikit-image.  PARITY UNPINNED against scikit-image itself, which is installed nowhere the tests run: the conversions
follow the PUBLISHED source of the pinned version (0.15.0: skimage/color/colorconv.py rgb2hsv / hsv2rgb, skimage/exposure
rescale_intensity, skimage/util/dtype.py img_as_float); the reference's own lines (models/augmenters/color/hsbcoloraugmenter.py:80-125,
hedcoloraugmenter.py:149-217, utils/custom_hed_transform.py:8-37) are followed statement by statement.  What IS pinned: the hsv
conversions against Python's ``colorsys`` (tests/test_randaug_v2_colour_cpu.py), the draw order against this planner, the device
against these functions.

Every image is an [H, W, 3] uint8 array.

hsv is float64 and uses only + - * / floor and the float remainder, all correctly rounded: ``hsv`` below is the expected result byte
for byte.

hed is float32 through logf / expf, which no two libraries round alike.  ``hed_bound`` therefore evaluates the chain in float64 ON THE
OPERANDS AS THE KERNEL SEES THEM (the float32 input x = float32(u8 * (1/255)) + 2, the float32 matrices, the float32 scalars) and
carries an absolute error bound along with every value: a pair (v, e) says that the float32 evaluation lies within e of v.
With u = 2^-24 (one rounding of a float32 operation, relative) the rules are
    c = a * k (k an exact float32)   v = a.v k,      e = |k| a.e + u (|v| + |k| a.e)
    c = a + b                        v = a.v + b.v,  e = a.e + b.e + u (|v| + a.e + b.e)
    c = -log(x), x exact             v = -log x,     e = 2u |v| (1 + 2u)        logf: 1 ulp, and ulp(y) <= 2^-23 |y| = 2u |y|
    c = exp(a)                       v = exp(a.v),   e = v expm1(a.e) + 2u v exp(a.e) (1 + 2u)        expf: 1 ulp
(|v| + propagated error bounds the magnitude of the value that gets rounded -- the magnitude companion of tests/_f64.py, per element.)
The 1 ulp of logf and expf is the HIP math API's documented maximum error of the two device functions ("HIP math API", single
precision floating-point: expf 1 ULP, logf 1 ULP); an ulp at the true value and at the returned one differ by the factor (1 + 2u) kept.
After r = exp(l) - 2 the chain is clip(r, -1, 1), + 1, / 2, * 2, + (-1), clip(., 0, 1), * 255, truncation.  In exact arithmetic that is
255 clip(r, 0, 1).  In float32 the divisions and multiplications by 2 are exact, the two additions round values of magnitude <= 2 and
<= 1 (3u in all), the product with 255 rounds once (255 u); every step is monotone, and r >= 1 gives exactly 255, r <= 0 exactly 0.
So with Y = 255 r and delta = 255 (e_r + 4u) the value the kernel truncates lies between clip(Y - delta, 0, 255) and
clip(Y + delta, 0, 255), and a byte is admissible iff it lies between the floors of the two.  A saturated byte has one admissible value.
"""
import numpy as np

POOL = ("identity", "contrast", "brightness", "sharpness", "rotate", "translate_x", "translate_y", "shear_x", "shear_y",
        "hed", "hsv", "autocontrast", "color", "equalize")          # augment_pool() order (:176-190)
SIGNED = ("rotate", "translate_x", "translate_y", "shear_x", "shear_y")
COLOUR = ("hed", "hsv")
CUTOFF = (0.15, 0.85)                                               # hed(): cutoff_range (:141)
U = 2.0 ** -24


# ------------------------------------------------------------------------------------------------ draws
def plan_image(rng, np_rng, n, m):
    """the draws of ONE ``RandAugment(n, m)(img)`` call (:203-208) with every op of the pool making its own: per op ``val``, then
    -- inside the op -- hed: ``randomize()`` draws the three sigmas and then the three biases, each uniform(-f, f) with f = val * 0.03
    (hedcoloraugmenter.py:216-217); hsv: uniform(-f, f) for hue, for saturation, and uniform(0, 0) for brightness, whose range is
    (0, 0) and not None (hsbcoloraugmenter.py:132); the five signed ops: random.choice([1, 0]).  -> [(name, val, third)]"""
    out = []
    for name in rng.sample(POOL, k=n):
        val = float(np_rng.uniform(1, m))
        f = val * 0.03
        if name == "hed":
            sig = [float(np_rng.uniform(-f, f)) for _ in range(3)]
            bias = [float(np_rng.uniform(-f, f)) for _ in range(3)]
            third = tuple(sig + bias)
        elif name == "hsv":
            third = tuple(float(np_rng.uniform(lo, hi)) for lo, hi in ((-f, f), (-f, f), (0, 0)))
        else:
            third = rng.choice([1, 0]) if name in SIGNED else None
        out.append((name, val, third))
    return out


# ------------------------------------------------------------------------------------------------ hsv (float64, exact)
def as_float(img_u8):
    """img_as_float of a uint8 image: a multiply by the reciprocal"""
    return np.multiply(img_u8, 1.0 / 255, dtype=np.float64)


def rgb2hsv(arr):
    """skimage 0.15.0 rgb2hsv on a float64 [H, W, 3] array in [0, 1]"""
    with np.errstate(invalid="ignore", divide="ignore"):
        v = arr.max(-1)
        delta = v - arr.min(-1)                     # ndarray.ptp
        s = delta / v
        s[delta == 0.0] = 0.0
        hue = np.zeros_like(v)
        idx = arr[..., 0] == v                      # red is the maximum; the later cases overwrite on a tie
        hue[idx] = (arr[idx, 1] - arr[idx, 2]) / delta[idx]
        idx = arr[..., 1] == v
        hue[idx] = 2.0 + (arr[idx, 2] - arr[idx, 0]) / delta[idx]
        idx = arr[..., 2] == v
        hue[idx] = 4.0 + (arr[idx, 0] - arr[idx, 1]) / delta[idx]
        h = (hue / 6.0) % 1.0
        h[delta == 0.0] = 0.0
    out = np.stack([h, s, v], axis=-1)
    out[np.isnan(out)] = 0
    return out


def hsv2rgb(arr):
    """skimage 0.15.0 hsv2rgb"""
    h, s, v = arr[..., 0], arr[..., 1], arr[..., 2]
    hi = np.floor(h * 6)
    f = h * 6 - hi
    p = v * (1 - s)
    q = v * (1 - f * s)
    t = v * (1 - (1 - f) * s)
    sel = hi.astype(np.uint8) % 6
    table = [(v, t, p), (q, v, p), (p, v, t), (p, q, v), (t, p, v), (v, p, q)]
    out = np.empty(arr.shape, np.float64)
    for c in range(3):
        out[..., c] = np.choose(sel, [row[c] for row in table])
    return out


def hsv_float(img_u8, sh, ss, sb=0.0):
    """HsbColorAugmenter.transform with the sigmas (sh, ss, sb) of randomize(), up to hsv2rgb: float64 rgb in [0, 1]"""
    assert sb == 0.0                                # the pool's brightness range is (0, 0)
    x = rgb2hsv(as_float(img_u8))
    if sh != 0.0:
        x[..., 0] += sh % 1.0
        x[..., 0] %= 1.0
    if ss != 0.0:
        if ss < 0.0:
            x[..., 1] *= (1.0 + ss)
        else:
            x[..., 1] *= (1.0 + (1.0 - x[..., 1]) * ss)
    return hsv2rgb(x)


def hsv(img_u8, sh, ss, sb=0.0):
    """... then ``patch_rgb *= 255.0`` and ``astype(uint8)``: the expected bytes"""
    rgb = hsv_float(img_u8, sh, ss, sb)
    rgb *= 255.0
    return rgb.astype(np.uint8)


# ------------------------------------------------------------------------------------------------ hed (float32)
def hed_matrices():
    """-> (hed_from_rgb, rgb_from_hed), float32: custom_hed_transform.py:8-11 (numpy's inverse here, scipy's there)"""
    m = np.array([[0.65, 0.70, 0.29], [0.07, 0.99, 0.11], [0.27, 0.57, 0.78]]).astype("float32")
    return np.linalg.inv(m).astype("float32"), m


def hed_scalars(draws):
    """(s_h, s_e, s_d, b_h, b_e, b_d) -> the float32 factors 1 + s_j and biases b_j that the in-place ops on a float32 array use"""
    d = [float(v) for v in draws]
    return [np.float32(1.0 + v) for v in d[:3]], [np.float32(v) for v in d[3:]]


def hed_applies(img_u8):
    """the cutoff test of HedColorAugmenter.transform: np.mean(patch) / 255.0 inside [0.15, 0.85]"""
    mean = np.mean(img_u8) / 255.0
    return bool(CUTOFF[0] <= mean <= CUTOFF[1])


def hed_input(img_u8):
    """separate_stains' operand: img_as_float, astype(float32), += 2"""
    x = as_float(img_u8).astype("float32")
    x += 2
    return x


def hed_f32(img_u8, draws):
    """the reference's own arithmetic in numpy float32, np.dot included: rgb2hed, the per-channel edits, hed2rgb with
    rescale_intensity(in_range=(-1, 1)) of a float image (out_range (-1, 1)), clip, * 255, astype(uint8)"""
    if not hed_applies(img_u8):
        return img_u8
    mi, m = hed_matrices()
    sig, bias = hed_scalars(draws)
    x = hed_input(img_u8)
    stains = np.reshape(np.dot(np.reshape(-np.log(x), (-1, 3)), mi), x.shape)
    for j in range(3):
        if draws[j] != 0.0:
            stains[..., j] *= sig[j]
        if draws[3 + j] != 0.0:
            stains[..., j] += bias[j]
    rgb2 = np.exp(np.dot(-np.reshape(stains, (-1, 3)), m))
    image = np.reshape(rgb2 - 2, stains.shape)
    assert image.dtype == np.float32
    image = np.clip(image, -1, 1)
    image = (image - np.float32(-1)) / np.float32(2.0)
    image = image * np.float32(2) + np.float32(-1)
    image = np.clip(image, 0.0, 1.0)
    image *= np.float32(255.0)
    assert image.dtype == np.float32
    return image.astype(np.uint8)


def _mulc(a, k):
    v, pe = a[0] * k, abs(k) * a[1]
    return v, pe + U * (np.abs(v) + pe)


def _add(a, b):
    v, pe = a[0] + b[0], a[1] + b[1]
    return v, pe + U * (np.abs(v) + pe)


def hed_bound(img_u8, draws):
    """-> (lo, hi, Y, delta): the admissible bytes lo <= byte <= hi of every element (uint8 arrays), the float64 value Y = 255 (e - 2)
    before the clips and the bound delta in byte steps (see the module text).  Outside the cutoff lo = hi = the input, delta = 0."""
    if not hed_applies(img_u8):
        z = np.zeros(img_u8.shape)
        return img_u8.copy(), img_u8.copy(), img_u8.astype(np.float64), z
    mi, m = hed_matrices()
    mi, m = mi.astype(np.float64), m.astype(np.float64)
    sig, bias = hed_scalars(draws)
    x = hed_input(img_u8).astype(np.float64)
    lv = -np.log(x)
    L = [(lv[..., c], 2 * U * (1 + 2 * U) * np.abs(lv[..., c])) for c in range(3)]
    st = []
    for j in range(3):
        d = _add(_add(_mulc(L[0], mi[0, j]), _mulc(L[1], mi[1, j])), _mulc(L[2], mi[2, j]))
        d = _add(_mulc(d, float(sig[j])), (float(bias[j]), 0.0))
        st.append((-d[0], d[1]))
    Y, delta = np.empty(img_u8.shape), np.empty(img_u8.shape)
    for c in range(3):
        l = _add(_add(_mulc(st[0], m[0, c]), _mulc(st[1], m[1, c])), _mulc(st[2], m[2, c]))
        ev = np.exp(l[0])
        e = (ev, ev * np.expm1(l[1]) + 2 * U * (1 + 2 * U) * ev * np.exp(l[1]))
        r = _add(e, (-2.0, 0.0))
        Y[..., c] = 255.0 * r[0]
        delta[..., c] = 255.0 * (r[1] + 4 * U)
    lo = np.floor(np.clip(Y - delta, 0.0, 255.0)).astype(np.uint8)
    hi = np.floor(np.clip(Y + delta, 0.0, 255.0)).astype(np.uint8)
    return lo, hi, Y, delta


def bound_stats(lo, hi, Y):
    """-> (fraction of bytes with more than one admissible value, fraction of unsaturated bytes: 0 < Y < 255)"""
    return float(np.mean(hi > lo)), float(np.mean((Y > 0.0) & (Y < 255.0)))


def tissue(h, w, seed, centre=(180, 110, 160), spread=25):
    """a tissue-like tile: per channel normal(centre, spread), clipped"""
    rs = np.random.RandomState(seed)
    return np.clip(rs.normal(centre, spread, (h, w, 3)), 0, 255).astype(np.uint8)


def colorsys_check_pixels():
    """[K, 3] uint8 pixels for the spec check: greys, black, white, channel ties of every kind, primaries, and a random lot"""
    px = [(0, 0, 0), (255, 255, 255), (7, 7, 7), (128, 128, 128), (200, 200, 50), (50, 200, 200), (200, 50, 200), (200, 50, 50),
          (50, 200, 50), (50, 50, 200), (255, 0, 0), (0, 255, 0), (0, 0, 255), (255, 255, 0), (0, 255, 255), (255, 0, 255), (1, 0, 0),
          (0, 0, 1), (254, 255, 255), (255, 254, 255)]
    rs = np.random.RandomState(5)
    return np.concatenate([np.array(px, np.uint8), rs.randint(0, 256, (400, 3)).astype(np.uint8)])
