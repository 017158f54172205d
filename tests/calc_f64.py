"""The CALC / DeepLCD net in double precision (CPU torch, NCHW): the reference the device kernels' stage taps are compared with.

forward_f64(layers, weights, x) honours the layer list as data — convolution geometry, the presence of every ReLU, the LRN window / alpha /
beta / k, Caffe's ceil-mode max pooling with windows clipped to the map, the NCHW flatten and the L2 normalisation — and returns the five
stage taps of myslam_lcd_debug_forward: a stage ends where the next Convolution or Pooling layer begins, the last one is the descriptor."""
import numpy as np

CONV, RELU, POOL_MAX, LRN = 1, 2, 3, 4

LAYER_DTYPE = np.dtype([("type", "<i4"), ("num_output", "<i4"), ("kernel", "<i4"), ("stride", "<i4"), ("pad", "<i4"),
                        ("local_size", "<i4"), ("alpha", "<f4"), ("beta", "<f4"), ("k", "<f4")])


def default_layers():
    """the SURVEY A.6 list (what myslam_lcd_default_layers returns), as data: usable without the library"""
    return np.array([(CONV, 64, 5, 2, 4, 0, 0, 0, 0), (RELU, 0, 0, 0, 0, 0, 0, 0, 0), (POOL_MAX, 0, 3, 2, 0, 0, 0, 0, 0), (LRN, 0, 0, 0, 0, 5, 1e-4, 0.75, 1.0),
                     (CONV, 128, 4, 1, 2, 0, 0, 0, 0), (RELU, 0, 0, 0, 0, 0, 0, 0, 0), (POOL_MAX, 0, 3, 2, 0, 0, 0, 0, 0), (LRN, 0, 0, 0, 0, 5, 1e-4, 0.75, 1.0),
                     (CONV, 4, 3, 1, 0, 0, 0, 0, 0), (RELU, 0, 0, 0, 0, 0, 0, 0, 0)], LAYER_DTYPE)


def _lrn(t, n, alpha, beta, k):
    """Caffe LRN across channels: y = x (k + alpha / n sum_{|j - c| <= n / 2} x_j^2)^-beta, channels outside the map count as zero"""
    import torch.nn.functional as F
    half = n // 2
    sq = F.pad(t * t, (0, 0, 0, 0, half, half))
    C = t.shape[1]
    ss = sum(sq[:, j:j + C] for j in range(n))
    return t * (k + (alpha / n) * ss) ** (-beta)


def forward_f64(layers, weights, x):
    """x: [120, 160] in [0, 1].  Returns [stage0 .. stage4]: f64 arrays [C, H, W] for the taps and [1064] for the descriptor."""
    import torch
    import torch.nn.functional as F
    w = np.ascontiguousarray(weights, np.float32).ravel()
    t = torch.from_numpy(np.ascontiguousarray(x, np.float64))[None, None]
    blocks, o = [], 0
    for i, l in enumerate(layers):
        ty = int(l["type"])
        if ty in (CONV, POOL_MAX) and i > 0:
            blocks.append(t)
        if ty == CONV:
            oc, k, ic = int(l["num_output"]), int(l["kernel"]), t.shape[1]
            n = oc * ic * k * k
            wt = torch.from_numpy(w[o:o + n].reshape(oc, ic, k, k).astype(np.float64)); o += n
            b = torch.from_numpy(w[o:o + oc].astype(np.float64)); o += oc
            t = F.conv2d(t, wt, b, stride=int(l["stride"]), padding=int(l["pad"]))
        elif ty == RELU:
            t = F.relu(t)
        elif ty == POOL_MAX:
            t = F.max_pool2d(t, int(l["kernel"]), int(l["stride"]), ceil_mode=True)
        elif ty == LRN:
            t = _lrn(t, int(l["local_size"]), float(l["alpha"]), float(l["beta"]), float(l["k"]))
        else:
            raise ValueError("layer type %d" % ty)
    assert o == w.size, "weights do not fit the layer list"
    flat = t[0].numpy().ravel()                                        # NCHW order
    assert flat.size == 1064
    with np.errstate(divide="ignore", invalid="ignore"):
        d = flat / np.sqrt((flat * flat).sum())                        # a zero norm gives what x / 0 gives: NaN (or inf)
    return [b[0].numpy() for b in blocks] + [d]


def nhwc_to_nchw(a, shape):
    """a device tap ([H * W][C] floats) in the layout of a reference stage of `shape` = (C, H, W)"""
    c, h, w = shape
    return np.asarray(a).reshape(h, w, c).transpose(2, 0, 1)


def maxnorm_err(got, ref):
    """largest absolute error over the largest reference magnitude of the stage"""
    return float(np.abs(np.asarray(got, np.float64) - ref).max() / np.abs(ref).max())
