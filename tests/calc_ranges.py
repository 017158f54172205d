"""CALC models over the ranges the kernel-family selection of csrc/calc.hip (lcd_create) decides on, shared by tests/test_calc_f64.py (host:
the f32 oracle against the f64 net on every one of them) and tests/test_gpu_lcd_ranges.py (device).

model(synth, name) -> (layers, weights, products): `products` is what DeepLCD.conv2_products() must report (3: f16 family, 6: bf16 family)."""
import numpy as np

import calc_f64

# flat blob: conv1.w [64][1][5][5], conv1.b [64], conv2.w [128][64][4][4], conv2.b [128], conv3.w [4][128][3][3], conv3.b [4]
O_W1, O_B1, O_W2, O_B2, O_W3, O_B3, O_END = np.cumsum([0, 1600, 64, 131072, 128, 4608, 4])

SCALE_K = (10, 14, 17, 20, 27)

# lcd_create keeps the f16 family only while max |w1| and max |w2| are at least this (csrc/calc.hip, F16_WMIN).  The w2min / w2below and
# w1min / w1below models sit on the bound and one f32 step under it with `products` 3 and 6: they pin this copy to the library.
F16_WMIN = 2.0 ** -6

BASE = ["base", "handcrafted"]
SCALED = ["c2down%d" % k for k in SCALE_K] + ["c1down%d" % k for k in SCALE_K]
THRESHOLDS = ["w2max30.9", "w2max31.0", "w2max31.5", "w1max30.9", "w1max31.5", "bound59000", "bound60500", "lrnk1.0", "lrnk0.99"]
LOWER = ["w2min", "w2below", "w1min", "w1below"]
MODELS = BASE + SCALED + THRESHOLDS + LOWER + ["mixed"]

BOUND_CHANNEL = 7                # the conv1 channel whose bias carries the bound59000 / bound60500 models to ~6e4


def _parts(w):
    return (w[O_W1:O_B1], w[O_B1:O_W2], w[O_W2:O_B2], w[O_B2:O_W3], w[O_W3:O_B3], w[O_B3:O_END])      # views


def _set_max(v, target):
    """scale v so that max |v| is exactly `target` in f32"""
    i = int(np.abs(v).argmax())
    v *= np.float32(target / float(np.abs(v[i])))
    v[i] = np.float32(np.sign(v[i]) * target)
    assert float(np.abs(v).max()) == float(np.float32(target))


def _pow2_below(f):
    return 2.0 ** np.floor(np.log2(f))


def _conv2_down(w2, b2, w3, f):
    """conv2 small: w2, b2 *= f, conv3 takes the scale back (as a power of two) so that the descriptor's entries keep their size against b3"""
    w2 *= np.float32(f); b2 *= np.float32(f); w3 *= np.float32(1.0 / _pow2_below(f))


def _conv1_down(w1, b1, w2, b2, w3, f):
    """conv1 small: w1, b1 *= f, the small values are conv2's ACTIVATIONS.  w2 takes back a power of two as long as |w2| stays below 31, conv3
    the rest; b2 follows the scale of conv2's products so that the bias does not bury them in the max-normalised figure"""
    w1 *= np.float32(f); b1 *= np.float32(f)
    k = -int(np.log2(_pow2_below(f))); j = k
    while float(np.abs(w2).max()) * 2.0 ** j >= 31.0:
        j -= 1
    w2 *= np.float32(2.0 ** j); b2 *= np.float32(2.0 ** (j - k)); w3 *= np.float32(2.0 ** (k - j))


def model(synth, name):
    L = calc_f64.default_layers()
    if name == "handcrafted":
        return L, synth.calc_weights_handcrafted(), 3
    w = synth.calc_weights().copy()
    w1, b1, w2, b2, w3, b3 = _parts(w)
    products = 3
    if name == "base":
        pass
    elif name.startswith("c2down"):
        # every k puts max |w2| (0.14 2^-k) under F16_WMIN: the loader has to keep the bf16 family
        _conv2_down(w2, b2, w3, 2.0 ** -int(name[6:])); products = 6
    elif name.startswith("c1down"):
        _conv1_down(w1, b1, w2, b2, w3, 2.0 ** -int(name[6:])); products = 6         # max |w1| = 0.7 2^-k
    elif name in ("w2min", "w2below"):
        # max |w2| exactly ON the lower bound (still the f16 family: the smallest weights' h and most m' are f16 subnormals) and one f32 step under it
        t = F16_WMIN if name == "w2min" else float(np.nextafter(np.float32(F16_WMIN), np.float32(0)))
        _conv2_down(w2, b2, w3, F16_WMIN / float(np.abs(w2).max())); _set_max(w2, t); products = 3 if name == "w2min" else 6
    elif name in ("w1min", "w1below"):
        t = F16_WMIN if name == "w1min" else float(np.nextafter(np.float32(F16_WMIN), np.float32(0)))
        _conv1_down(w1, b1, w2, b2, w3, F16_WMIN / float(np.abs(w1).max())); _set_max(w1, t); products = 3 if name == "w1min" else 6
    elif name.startswith("w2max"):
        t = float(name[5:]); _set_max(w2, t); products = 3 if t < 31.0 else 6
    elif name.startswith("w1max"):
        t = float(name[5:]); _set_max(w1, t); products = 3 if t < 31.0 else 6
    elif name.startswith("bound"):
        # sum |w1| + |b1| of channel 7 reaches the target through its bias: conv1's outputs of that channel really are ~6e4
        t = float(name[5:]); c = BOUND_CHANNEL
        b1[c] = np.float32(t - float(np.abs(w1[25 * c:25 * c + 25].astype(np.float64)).sum()))
        bound = float(np.abs(w1[25 * c:25 * c + 25].astype(np.float64)).sum() + abs(float(b1[c])))
        assert abs(bound - t) < 0.01
        products = 3 if t < 60000 else 6
    elif name.startswith("lrnk"):
        L["k"][3] = float(name[4:]); products = 3 if float(name[4:]) >= 1.0 else 6
    elif name == "mixed":
        # two output and two input channels of conv2 live 2^-24 below the rest: max |w2| stays where it was
        W2 = w2.reshape(128, 64, 16)
        for oc in (5, 77):
            W2[oc] *= np.float32(2.0 ** -24); b2[oc] *= np.float32(2.0 ** -24)
        for ic in (3, 40):
            W2[:, ic] *= np.float32(2.0 ** -24)
    else:
        raise KeyError(name)
    return L, w, products


def zero_norm_model(synth):
    """The hand-made bank with its ReLU after conv3 and conv3's biases pushed down: the map is empty on a flat image (centre minus surround
    of a flat map is zero, the bias decides) and still populated on a textured one."""
    L = calc_f64.default_layers()
    assert L["type"][-1] == calc_f64.RELU
    return L, synth.calc_weights_handcrafted(c3_bias=ZERO_NORM_BIAS)


ZERO_NORM_BIAS = 0.97            # flat images peak at 0.943 before the bias (f64), a textured one reaches 1.1


def inputs(synth):
    """name -> [120, 160] f32 network input in [0, 1]"""
    out = {"uniform": synth._rng(21).uniform(0, 1, (120, 160)).astype(np.float32),
           "u8": (synth.random_image(160120, 120, 160).astype(np.float32) * np.float32(1.0 / 255.0)),
           "zeros": np.zeros((120, 160), np.float32), "ones": np.ones((120, 160), np.float32),
           "checker": ((np.add.outer(np.arange(120), np.arange(160)) & 1).astype(np.float32))}
    for y, x in ((0, 0), (0, 159), (119, 0), (119, 159), (59, 80), (118, 158)):
        a = np.zeros((120, 160), np.float32); a[y, x] = 1.0
        out["impulse_%d_%d" % (y, x)] = a
    return out


def batch_images(synth, B):
    """B maximally different 120 x 160 8-bit neighbours: all 255, all 0, noise, texture, checkerboard"""
    imgs = [np.full((120, 160), 255, np.uint8), np.zeros((120, 160), np.uint8), synth.random_image(77, 120, 160, kind="noise"),
            synth.random_image(78, 120, 160), ((np.add.outer(np.arange(120), np.arange(160)) & 1) * 255).astype(np.uint8)]
    return imgs[:B]
