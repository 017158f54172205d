"""ctypes mirror of the reference's operator interface over libmyslam_hip.so (include/myslam_hip.h).

Names follow the reference: ORBextractor (include/myslam/ORBextractor.h), DeepLCD
(include/myslam/deeplcd.h), the BFMatcher-style `hamming_match`, `triangulation` (algorithm.h), the
loop database of LoopClosing::DetectLoop and the BA block build of Backend::OptimizeActiveMap.
Host-buffer calls take numpy arrays; *_batch calls take raw device pointers (e.g. torch.Tensor.data_ptr()).
There is no CPU fallback: a missing library or GPU raises.
"""
import ctypes as C
import os
import re

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libmyslam_hip.so")

OK, ERR_INVALID, ERR_HIP, ERR_CAPACITY, ERR_UNSUPPORTED = 0, -1, -2, -3, -4
LCD_DIM = 1064

KP_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("size", "<f4"), ("angle", "<f4"),
                     ("response", "<f4"), ("octave", "<i4"), ("class_id", "<i4")])
assert KP_DTYPE.itemsize == 28


class MyslamError(RuntimeError):
    def __init__(self, where, code):
        names = {-1: "INVALID", -2: "HIP", -3: "CAPACITY", -4: "UNSUPPORTED"}
        super().__init__(f"{where} failed: {code} ({names.get(code, '?')})")
        self.code = code


HEADER_PATH = os.path.join(_HERE, "..", "include", "myslam_hip.h")
CALC_LAYER_DTYPE = np.dtype([("type", "<i4"), ("num_output", "<i4"), ("kernel", "<i4"), ("stride", "<i4"), ("pad", "<i4"),
                             ("local_size", "<i4"), ("alpha", "<f4"), ("beta", "<f4"), ("k", "<f4")])     # myslam_calc_layer
assert CALC_LAYER_DTYPE.itemsize == 36
CALC_CONV, CALC_RELU, CALC_POOL_MAX, CALC_LRN = 1, 2, 3, 4
CAND_DTYPE = np.dtype([("best_id", "<u8"), ("max_score", "<f4"), ("cnt", "<i4")])      # myslam_lcd_candidate
assert CAND_DTYPE.itemsize == 16
OWNED_DTYPE = np.dtype([("pre_best_id", "<u8"), ("pre_max_score", "<f4"), ("pre_cnt", "<i4"),
                        ("suf_best_id", "<u8"), ("suf_max_score", "<f4"), ("suf_cnt", "<i4")])      # myslam_lcd_owned_candidate
assert OWNED_DTYPE.itemsize == 32

_lib = None
_SCALARS = {"int": C.c_int, "float": C.c_float, "double": C.c_double, "size_t": C.c_size_t, "uint64_t": C.c_uint64, "long": C.c_long,
            "int32_t": C.c_int32, "uint8_t": C.c_uint8, "int64_t": C.c_int64}


def header_prototypes(path=HEADER_PATH):
    """{function name: (return type, [parameter types])} parsed from include/myslam_hip.h — every pointer is 'ptr'."""
    txt = open(path).read()
    txt = re.sub(r"/\*.*?\*/", " ", txt, flags=re.S)
    txt = re.sub(r"//[^\n]*", " ", txt)
    out = {}
    for m in re.finditer(r"\b(int|float|size_t|const char\s*\*)\s+(myslam_\w+)\s*\(([^()]*)\)\s*;", txt):
        ret, name, params = m.group(1), m.group(2), m.group(3).strip()
        types = []
        if params and params != "void":
            for prm in params.split(","):
                prm = prm.strip()
                if "*" in prm:
                    types.append("ptr")
                else:
                    toks = [t for t in prm.split() if t != "const"]
                    types.append(toks[0])
        out[name] = ("char*" if "char" in ret else ret, types)
    return out


def lib():
    """Load libmyslam_hip.so (fails loudly when it has not been built) and declare every prototype of the header, so that 64-bit
    pointers, size_t and floating-point arguments never depend on how a call site wraps them."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(f"{LIB_PATH} is missing: run __graft_entry__.build() / build.py first (no CPU fallback)")
        L = C.CDLL(LIB_PATH)
        for name, (ret, types) in header_prototypes().items():
            fn = getattr(L, name)              # AttributeError = the library does not export what the header declares
            fn.restype = {"int": C.c_int, "float": C.c_float, "size_t": C.c_size_t, "char*": C.c_char_p}[ret]
            fn.argtypes = [C.c_void_p if t == "ptr" else _SCALARS[t] for t in types]
        _lib = L
    return _lib


def _check(code, where):
    if code != OK:
        raise MyslamError(where, code)


def _p(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def device_count():
    return lib().myslam_hip_device_count()


def version():
    """'myslam_hip <version> (gfx950) build <digest of the sources>'"""
    return lib().myslam_hip_version().decode()


def build_id():
    return version().rsplit(" ", 1)[-1]


def shader_clock_mhz(stream=0, spin_us=200.0):
    """the shader clock right now, measured on the device (one wave spins for spin_us); synchronises `stream`"""
    v = C.c_float()
    _check(lib().myslam_prof_shader_clock_mhz(stream, float(spin_us), C.byref(v)), "myslam_prof_shader_clock_mhz")
    return float(v.value)


# ---------------------------------------------------------------------------------- profiling
def prof_enable(on=True):
    lib().myslam_prof_enable(1 if on else 0)


def prof_reset():
    lib().myslam_prof_reset()


def prof_read():
    """{kernel name: (total ms, launches)} since the last reset (synchronises)."""
    L = lib()
    out = {}
    for i in range(L.myslam_prof_count()):
        name = C.c_char_p(); ms = C.c_double(); n = C.c_long()
        L.myslam_prof_get(i, C.byref(name), C.byref(ms), C.byref(n))
        out[name.value.decode()] = (ms.value, n.value)
    return out


# ---------------------------------------------------------------------------------- ORB
class ORBextractor:
    """ORBextractor(nfeatures, scaleFactor, nlevels, iniThFAST, minThFAST) — ORBextractor.h:55-56."""

    def __init__(self, nfeatures=2000, scaleFactor=1.2, nlevels=8, iniThFAST=20, minThFAST=7, stream=None):
        self._h = C.c_void_p()
        _check(lib().myslam_orb_create(C.byref(self._h), int(nfeatures), C.c_float(scaleFactor), int(nlevels),
                                       int(iniThFAST), int(minThFAST)), "myslam_orb_create")
        self.nfeatures, self.nlevels = nfeatures, nlevels
        if stream is not None:
            self.set_stream(stream)

    def __del__(self):
        if getattr(self, "_h", None) and self._h.value and _lib is not None:
            _lib.myslam_orb_destroy(self._h)
            self._h = C.c_void_p()

    def set_stream(self, stream_ptr):
        _check(lib().myslam_orb_set_stream(self._h, C.c_void_p(stream_ptr)), "myslam_orb_set_stream")

    def set_fast_event(self, event_ptr):
        """Record the hipEvent_t `event_ptr` (0 = off) on the handle's stream after the FAST stage of every following batched call."""
        _check(lib().myslam_orb_set_fast_event(self._h, C.c_void_p(event_ptr or None)), "myslam_orb_set_fast_event")

    def set_fast_gate(self, event_ptr):
        """Make the handle's stream wait for the hipEvent_t `event_ptr` (0 = off) before the FAST stage of every following batched call."""
        _check(lib().myslam_orb_set_fast_gate(self._h, C.c_void_p(event_ptr or None)), "myslam_orb_set_fast_gate")

    OPT_FAST_MODE, OPT_INTERNAL_STREAM, OPT_STOP_AFTER, OPT_COPY_INPUT, OPT_BLUR_MFMA, OPT_SIDE_BLOCKS_PER_CU = 1, 2, 3, 4, 5, 6

    def set_option(self, option, value):
        """scheduling / debugging knobs (myslam_orb_set_option): none of them changes a result"""
        _check(lib().myslam_orb_set_option(self._h, int(option), int(value)), "myslam_orb_set_option")

    def set_gauss_taps(self, q7=None):
        q = None if q7 is None else np.ascontiguousarray(q7, np.int32)
        _check(lib().myslam_orb_set_gauss_taps(self._h, _p(q) if q is not None else None), "myslam_orb_set_gauss_taps")

    def tables(self):
        n = self.nlevels
        sc = np.zeros(n, np.float32); isc = np.zeros(n, np.float32); npl = np.zeros(n, np.int32); um = np.zeros(16, np.int32)
        _check(lib().myslam_orb_get_tables(self._h, _p(sc), _p(isc), _p(npl), _p(um)), "myslam_orb_get_tables")
        return sc, isc, npl, um

    def max_keypoints(self, rows=None, cols=None):
        if rows is not None:
            return lib().myslam_orb_max_keypoints_for(self._h, int(rows), int(cols))
        return lib().myslam_orb_max_keypoints(self._h)

    @staticmethod
    def _img(img):
        img = np.ascontiguousarray(img, np.uint8)
        assert img.ndim == 2
        return img

    def DetectAndCompute(self, image, mask=None, cap=None):
        img = self._img(image)
        cap = cap or self.max_keypoints(*img.shape)
        kps = np.zeros(cap, KP_DTYPE); desc = np.zeros((cap, 32), np.uint8); n = C.c_int()
        m = self._img(mask) if mask is not None else None
        _check(lib().myslam_orb_detect_and_compute(self._h, _p(img), img.shape[0], img.shape[1], img.strides[0],
                                                   _p(m), m.strides[0] if m is not None else 0,
                                                   _p(kps), _p(desc), cap, C.byref(n)), "myslam_orb_detect_and_compute")
        return kps[:n.value].copy(), desc[:n.value].copy()

    def Detect(self, image, mask=None, cap=None):
        img = self._img(image)
        cap = cap or self.max_keypoints(*img.shape)
        kps = np.zeros(cap, KP_DTYPE); n = C.c_int()
        m = self._img(mask) if mask is not None else None
        _check(lib().myslam_orb_detect(self._h, _p(img), img.shape[0], img.shape[1], img.strides[0],
                                       _p(m), m.strides[0] if m is not None else 0, _p(kps), cap, C.byref(n)),
               "myslam_orb_detect")
        return kps[:n.value].copy()

    def ScreenAndComputeKPsParams(self, image, keypoints):
        """returns (out_keypoints, keypoints as modified in place by the call)"""
        img = self._img(image)
        kin = np.ascontiguousarray(keypoints, KP_DTYPE).copy()
        kout = np.zeros(max(len(kin), 1), KP_DTYPE); n = C.c_int()
        _check(lib().myslam_orb_screen_and_compute_params(self._h, _p(img), img.shape[0], img.shape[1], img.strides[0],
                                                          _p(kin), len(kin), _p(kout), len(kout), C.byref(n)),
               "myslam_orb_screen_and_compute_params")
        return kout[:n.value].copy(), kin

    def CalcDescriptors(self, image, keypoints):
        img = self._img(image)
        k = np.ascontiguousarray(keypoints, KP_DTYPE)
        desc = np.zeros((len(k), 32), np.uint8)
        _check(lib().myslam_orb_calc_descriptors(self._h, _p(img), img.shape[0], img.shape[1], img.strides[0],
                                                 _p(k), len(k), _p(desc)), "myslam_orb_calc_descriptors")
        return desc

    # device-resident batch (pointers are ints)
    def detect_and_compute_batch(self, d_imgs, batch, rows, cols, step, img_stride, d_kps, d_desc, d_counts, d_status, cap,
                                 d_masks=0):
        _check(lib().myslam_orb_detect_and_compute_batch(self._h, C.c_void_p(d_imgs), batch, rows, cols, step,
                                                         C.c_size_t(img_stride), C.c_void_p(d_masks or None),
                                                         C.c_void_p(d_kps), C.c_void_p(d_desc), C.c_void_p(d_counts),
                                                         C.c_void_p(d_status or None), cap),
               "myslam_orb_detect_and_compute_batch")

    def detect_batch(self, d_imgs, batch, rows, cols, step, img_stride, d_kps, d_counts, d_status, cap, d_masks=0):
        _check(lib().myslam_orb_detect_batch(self._h, C.c_void_p(d_imgs), batch, rows, cols, step, C.c_size_t(img_stride),
                                             C.c_void_p(d_masks or None), C.c_void_p(d_kps), C.c_void_p(d_counts),
                                             C.c_void_p(d_status or None), cap), "myslam_orb_detect_batch")

    def process_keyframes_batch(self, d_imgs, batch, rows, cols, step, img_stride, d_feat_xy, d_n_feat, feat_cap, d_pyr_kps, d_desc, d_counts,
                                d_status, cap):
        """The ORB half of LoopClosing::ProcessNewKF (loopclosing.cpp:93-113) for `batch` key-frames on the device, in the header's argument
        order: expansion of every feature over the levels, ScreenAndComputeKPsParams, CalcDescriptors.  Writes mvPyramidKeyPoints (batch x cap),
        mORBDescriptors (batch x cap x 32) and their counts where loop_match_batch reads them; d_status batch i32 = 0 or ERR_CAPACITY per item.
        Enqueues on the handle's stream and returns."""
        _check(lib().myslam_orb_process_keyframes_batch(self._h, C.c_void_p(d_imgs), int(batch), int(rows), int(cols), int(step),
                                                        C.c_size_t(img_stride), C.c_void_p(d_feat_xy), C.c_void_p(d_n_feat), int(feat_cap),
                                                        C.c_void_p(d_pyr_kps), C.c_void_p(d_desc), C.c_void_p(d_counts), C.c_void_p(d_status),
                                                        int(cap)), "myslam_orb_process_keyframes_batch")

    # stage taps
    def debug_pyramid(self, image, level, blurred=False):
        img = self._img(image)
        w = C.c_int(); h = C.c_int()
        _check(lib().myslam_orb_debug_pyramid(self._h, _p(img), img.shape[0], img.shape[1], img.strides[0], level,
                                              1 if blurred else 0, None, 0, C.byref(w), C.byref(h)), "debug_pyramid(size)")
        out = np.zeros((h.value, w.value), np.uint8)
        _check(lib().myslam_orb_debug_pyramid(self._h, _p(img), img.shape[0], img.shape[1], img.strides[0], level,
                                              1 if blurred else 0, _p(out), out.strides[0], C.byref(w), C.byref(h)),
               "debug_pyramid")
        return out

    def debug_candidates(self, image, level, mask=None):
        img = self._img(image)
        cap = 65536
        xs = np.zeros(cap, np.int32); ys = np.zeros(cap, np.int32); sc = np.zeros(cap, np.int32); n = C.c_int()
        m = self._img(mask) if mask is not None else None
        _check(lib().myslam_orb_debug_candidates(self._h, _p(img), img.shape[0], img.shape[1], img.strides[0],
                                                 _p(m), m.strides[0] if m is not None else 0, level,
                                                 _p(xs), _p(ys), _p(sc), cap, C.byref(n)), "debug_candidates")
        return xs[:n.value].copy(), ys[:n.value].copy(), sc[:n.value].copy()

    def fast_statistics(self, level):
        """what the last grid-FAST launch measured on `level`: (statistic, pixel pairs, path) — myslam_orb_debug_readback(what = 6)"""
        out = np.zeros(4, np.uint32)
        _check(lib().myslam_orb_debug_readback(self._h, 6, 0, level, _p(out), out.nbytes, 0), "debug_readback")
        return int(out[0]), int(out[1]), int(out[2])


# ---------------------------------------------------------------------------------- Hamming / triangulation
def hamming_match(query, train):
    """cv::BFMatcher(NORM_HAMMING).match(query, train) -> (trainIdx, distance) per query row."""
    q = np.ascontiguousarray(query, np.uint8).reshape(-1, 32); t = np.ascontiguousarray(train, np.uint8).reshape(-1, 32)
    idx = np.zeros(len(q), np.int32); dist = np.zeros(len(q), np.int32)
    _check(lib().myslam_hamming_match(_p(q), len(q), _p(t), len(t), _p(idx), _p(dist)), "myslam_hamming_match")
    return idx, dist


def hamming_match_batch(d_q, d_nq, d_t, d_nt, batch, cap, d_idx, d_dist, stream=0):
    _check(lib().myslam_hamming_match_batch(C.c_void_p(d_q), C.c_void_p(d_nq), C.c_void_p(d_t), C.c_void_p(d_nt), batch, cap,
                                            C.c_void_p(d_idx), C.c_void_p(d_dist), C.c_void_p(stream or None)),
           "myslam_hamming_match_batch")


def hamming_filter(dist):
    d = np.ascontiguousarray(dist, np.int32)
    keep = np.zeros(len(d), np.uint8); mn = C.c_int()
    _check(lib().myslam_hamming_filter(_p(d), len(d), _p(keep), C.byref(mn)), "myslam_hamming_filter")
    return keep.astype(bool), mn.value


def expand_pyramid_keypoints(feats, nlevels=8):
    """LoopClosing::ProcessNewKF (loopclosing.cpp:94-105): nlevels pyramid key-points per feature, class_id = feature index"""
    f = np.ascontiguousarray(feats, KP_DTYPE)
    out = np.zeros(len(f) * nlevels, KP_DTYPE)
    _check(lib().myslam_expand_pyramid_keypoints(_p(f), len(f), nlevels, _p(out)), "myslam_expand_pyramid_keypoints")
    return out


def match_feature_pairs(train_idx, dist, loop_pyr_kps, cur_pyr_kps):
    """LoopClosing::MatchFeatures (loopclosing.cpp:175-194): (current feature id, loop feature id) pairs, std::set order"""
    ti = np.ascontiguousarray(train_idx, np.int32); d = np.ascontiguousarray(dist, np.int32)
    lk = np.ascontiguousarray(loop_pyr_kps, KP_DTYPE); ck = np.ascontiguousarray(cur_pyr_kps, KP_DTYPE)
    assert len(ti) == len(d) == len(lk)
    pairs = np.zeros((max(len(ti), 1), 2), np.int32); n = C.c_int()
    _check(lib().myslam_match_feature_pairs(_p(ti), _p(d), len(ti), _p(lk), _p(ck), len(ck), _p(pairs), C.byref(n)), "myslam_match_feature_pairs")
    return pairs[:n.value].copy()


LOOP_MATCH_OK, LOOP_MATCH_FEW_PAIRS, LOOP_MATCH_FEW_POINTS = 0, 1, 2      # MYSLAM_LOOP_MATCH_*


def loop_match_batch(d_loop_desc, d_n_loop, d_cur_desc, d_n_cur, d_loop_pyr, d_cur_pyr, batch, cap, d_cur_feat_xy, d_loop_feat_landmark, feat_cap,
                     d_landmark_pos, landmark_stride, landmark_cap, min_matches, out_cap, d_train_idx, d_dist, d_pairs, d_n_pairs, d_valid_pairs,
                     d_pts3d, d_pts2d, d_counts, d_status, stream=0):
    """LoopClosing::MatchFeatures (loopclosing.cpp:167-203) and ComputeCorrectPose's gather (:210-253) for `batch` candidates on the device, in the
    header's argument order: matcher, distance filter, (current id, loop id) set, landmark filter, cv::Point3f / Point2f arrays and counts as
    PnPSolver.verify_batch reads them.  d_status batch i32 = LOOP_MATCH_* or a negative error code per item."""
    ptrs = [C.c_void_p(x) for x in (d_loop_desc, d_n_loop, d_cur_desc, d_n_cur, d_loop_pyr, d_cur_pyr)]
    outs = [C.c_void_p(x) for x in (d_train_idx, d_dist, d_pairs, d_n_pairs, d_valid_pairs, d_pts3d, d_pts2d, d_counts, d_status)]
    _check(lib().myslam_loop_match_batch(*ptrs, int(batch), int(cap), C.c_void_p(d_cur_feat_xy), C.c_void_p(d_loop_feat_landmark), int(feat_cap),
                                         C.c_void_p(d_landmark_pos), int(landmark_stride), int(landmark_cap), int(min_matches), int(out_cap), *outs,
                                         C.c_void_p(stream or None)), "myslam_loop_match_batch")


def triangulate_stereo(xl, yl, xr, yr, fx, fy, cx, cy, baseline):
    xl, yl, xr, yr = [np.ascontiguousarray(a, np.float32) for a in (xl, yl, xr, yr)]
    n = len(xl)
    xyz = np.zeros((n, 3)); ok = np.zeros(n, np.uint8)
    _check(lib().myslam_triangulate_stereo(_p(xl), _p(yl), _p(xr), _p(yr), n, C.c_double(fx), C.c_double(fy), C.c_double(cx),
                                           C.c_double(cy), C.c_double(baseline), _p(xyz), _p(ok)), "myslam_triangulate_stereo")
    return xyz, ok.astype(bool)


def triangulate_stereo_batch(d_kl, d_kr, d_match, d_nl, batch, cap, K, baseline, d_xyz, d_ok, stream=0):
    _check(lib().myslam_triangulate_stereo_batch(C.c_void_p(d_kl), C.c_void_p(d_kr), C.c_void_p(d_match), C.c_void_p(d_nl),
                                                 batch, cap, C.c_double(K[0]), C.c_double(K[1]), C.c_double(K[2]),
                                                 C.c_double(K[3]), C.c_double(baseline), C.c_void_p(d_xyz), C.c_void_p(d_ok),
                                                 C.c_void_p(stream or None)), "myslam_triangulate_stereo_batch")


def hamming_match_triangulate_batch(d_q, d_nq, d_t, d_nt, d_kl, d_kr, batch, cap, K, baseline, d_idx, d_dist, d_xyz, d_ok, stream=0):
    """myslam_hamming_match_triangulate_batch: match + triangulation of every match, one launch for fewer than 16 pairs."""
    _check(lib().myslam_hamming_match_triangulate_batch(C.c_void_p(d_q), C.c_void_p(d_nq), C.c_void_p(d_t), C.c_void_p(d_nt), C.c_void_p(d_kl),
                                                        C.c_void_p(d_kr), batch, cap, C.c_double(K[0]), C.c_double(K[1]), C.c_double(K[2]),
                                                        C.c_double(K[3]), C.c_double(baseline), C.c_void_p(d_idx), C.c_void_p(d_dist),
                                                        C.c_void_p(d_xyz), C.c_void_p(d_ok), C.c_void_p(stream or None)),
           "myslam_hamming_match_triangulate_batch")


# ---------------------------------------------------------------------------------- DeepLCD
def calc_default_layers():
    """the SURVEY A.6 layer list as CALC_LAYER_DTYPE records"""
    n = lib().myslam_lcd_default_layers(None, 0)
    L = np.zeros(n, CALC_LAYER_DTYPE)
    assert lib().myslam_lcd_default_layers(_p(L), n) == n
    return L


def calc_parse_caffe(prototxt_path, caffemodel_path):
    """(layer records, flat weights) of a deploy.prototxt + .caffemodel pair — host only, no device needed"""
    nl = C.c_int(); nw = C.c_size_t()
    _check(lib().myslam_calc_parse_caffe(prototxt_path.encode(), caffemodel_path.encode(), None, 0, C.byref(nl), None, 0, C.byref(nw)),
           "myslam_calc_parse_caffe")
    L = np.zeros(nl.value, CALC_LAYER_DTYPE); w = np.zeros(nw.value, np.float32)
    _check(lib().myslam_calc_parse_caffe(prototxt_path.encode(), caffemodel_path.encode(), _p(L), len(L), C.byref(nl), _p(w), w.size, C.byref(nw)),
           "myslam_calc_parse_caffe")
    return L, w


class DeepLCD:
    """DeepLCD(weights) — include/myslam/deeplcd.h:33.  `weights` = flat f32 blob of the SURVEY A.6 layer list; `layers` = explicit
    CALC_LAYER_DTYPE records; DeepLCD.from_caffe(prototxt, caffemodel) = the reference's constructor arguments."""
    OPT_GENERIC_KERNELS = 1
    OPT_CONV2_BF16X6 = 2
    OPT_SKIP_KERNELS = 3

    def __init__(self, weights=None, stream=None, layers=None, caffe=None, path=None):
        self._h = C.c_void_p()
        if caffe is not None:
            _check(lib().myslam_lcd_create_from_caffe(C.byref(self._h), caffe[0].encode(), caffe[1].encode()), "myslam_lcd_create_from_caffe")
        elif path is not None:
            _check(lib().myslam_lcd_create_from_file(C.byref(self._h), path.encode()), "myslam_lcd_create_from_file")
        else:
            w = np.ascontiguousarray(weights, np.float32).ravel()
            if layers is not None:
                L = np.ascontiguousarray(layers, CALC_LAYER_DTYPE)
                _check(lib().myslam_lcd_create_from_layers(C.byref(self._h), _p(L), len(L), _p(w), w.size), "myslam_lcd_create_from_layers")
            else:
                _check(lib().myslam_lcd_create(C.byref(self._h), _p(w), w.size), "myslam_lcd_create")
        if stream is not None:
            _check(lib().myslam_lcd_set_stream(self._h, C.c_void_p(stream)), "myslam_lcd_set_stream")

    @classmethod
    def from_caffe(cls, prototxt_path="calc_model/deploy.prototxt", caffemodel_path="calc_model/calc.caffemodel", stream=None):
        return cls(caffe=(prototxt_path, caffemodel_path), stream=stream)

    def set_option(self, option, value):
        _check(lib().myslam_lcd_set_option(self._h, int(option), int(value)), "myslam_lcd_set_option")

    def uses_fused_kernels(self):
        return lib().myslam_lcd_uses_fused_kernels(self._h) == 1

    def conv2_products(self):
        """3: conv2 runs as f16 x 3 on the matrix cores, 6: as bf16 x 6, 0: generic kernels"""
        return lib().myslam_lcd_conv2_products(self._h)

    def __del__(self):
        if getattr(self, "_h", None) and self._h.value and _lib is not None:
            _lib.myslam_lcd_destroy(self._h)
            self._h = C.c_void_p()

    def calcDescrOriginalImg(self, image, blur_in_place=True):
        """returns (descriptor[1064], image after the call) — the reference blurs the caller's image in place."""
        img = np.ascontiguousarray(image, np.uint8).copy()
        d = np.zeros(LCD_DIM, np.float32)
        _check(lib().myslam_lcd_calc_descr_original_img(self._h, _p(img), img.shape[0], img.shape[1], img.strides[0],
                                                        1 if blur_in_place else 0, _p(d)), "myslam_lcd_calc_descr_original_img")
        return d, img

    def calcDescr(self, im160x120):
        img = np.ascontiguousarray(im160x120, np.uint8)
        assert img.shape == (120, 160)
        d = np.zeros(LCD_DIM, np.float32)
        _check(lib().myslam_lcd_calc_descr(self._h, _p(img), img.strides[0], _p(d)), "myslam_lcd_calc_descr")
        return d

    @staticmethod
    def score(d1, d2):
        a = np.ascontiguousarray(d1, np.float32); b = np.ascontiguousarray(d2, np.float32)
        return float(lib().myslam_lcd_score(_p(a), _p(b)))

    def describe_batch(self, d_imgs, batch, rows, cols, step, img_stride, d_out, blur_in_place=False):
        _check(lib().myslam_lcd_describe_batch(self._h, C.c_void_p(d_imgs), batch, rows, cols, step, C.c_size_t(img_stride),
                                               1 if blur_in_place else 0, C.c_void_p(d_out)), "myslam_lcd_describe_batch")

    def debug_forward(self, x120x160, stage):
        x = np.ascontiguousarray(x120x160, np.float32)
        sizes = [62 * 82 * 64, 31 * 41 * 64, 32 * 42 * 128, 16 * 21 * 128, LCD_DIM]
        out = np.zeros(sizes[stage], np.float32)
        _check(lib().myslam_lcd_debug_forward(self._h, _p(x), _p(out), stage, C.c_size_t(out.size)), "myslam_lcd_debug_forward")
        return out


class _LoopQueries:
    """The query entry points of a loop database's built-in context (myslam_lcddb_*) and of a query context (myslam_lcddb_ctx_*)."""
    _prefix = "myslam_lcddb_"

    def _call(self, name, *args):
        fn = self._prefix + name
        _check(getattr(lib(), fn)(self._h, *args), fn)

    def query_batch(self, d_q, cur_ids, nq, d_best, d_max, d_cnt, thr_low=0.92):
        cur = np.ascontiguousarray(cur_ids, np.uint64)
        self._call("query_batch", C.c_void_p(d_q), _p(cur), nq, C.c_float(thr_low), C.c_void_p(d_best), C.c_void_p(d_max), C.c_void_p(d_cnt))

    def update_query_limits(self, cur_ids):
        """new cur_ids (or appended rows) for a query that was recorded into a HIP graph (StepGraph); MyslamError(CAPACITY) = record again"""
        cur = np.ascontiguousarray(cur_ids, np.uint64)
        self._call("update_query_limits", _p(cur), len(cur))

    def query_batch_sharded(self, d_q, cur_ids, nq, d_cand, thr_low=0.92):
        """per-shard records (myslam_lcd_candidate, 16 bytes each, device memory) for the multi-GPU exchange"""
        cur = np.ascontiguousarray(cur_ids, np.uint64)
        self._call("query_batch_sharded", d_q, _p(cur), nq, thr_low, d_cand)

    def query_batch_owned(self, d_q, cur_ids, nq, d_cand, thr_low=0.92):
        """records of a shard whose ids interleave with the other shards' (myslam_lcd_owned_candidate, 32 bytes each, device memory)"""
        cur = np.ascontiguousarray(cur_ids, np.uint64)
        self._call("query_batch_owned", d_q, _p(cur), nq, thr_low, d_cand)


class LoopDatabase(_LoopQueries):
    """LoopClosing::_mvDatabase + DetectLoop()/AddToDatabase() — loopclosing.cpp:124-161, 651-659."""

    def __init__(self, capacity, stream=None):
        self._h = C.c_void_p()
        _check(lib().myslam_lcddb_create(C.byref(self._h), int(capacity)), "myslam_lcddb_create")
        if stream is not None:
            _check(lib().myslam_lcddb_set_stream(self._h, C.c_void_p(stream)), "myslam_lcddb_set_stream")

    def __del__(self):
        if getattr(self, "_h", None) and self._h.value and _lib is not None:
            _lib.myslam_lcddb_destroy(self._h)
            self._h = C.c_void_p()

    def __len__(self):
        return lib().myslam_lcddb_size(self._h)

    def capacity(self):
        return lib().myslam_lcddb_capacity(self._h)

    def reserve(self, rows):
        _check(lib().myslam_lcddb_reserve(self._h, int(rows)), "myslam_lcddb_reserve")

    def AddToDatabase(self, kf_id, descr):
        d = np.ascontiguousarray(descr, np.float32)
        _check(lib().myslam_lcddb_append(self._h, C.c_uint64(kf_id), _p(d)), "myslam_lcddb_append")

    def append_batch(self, ids, d_descr, n):
        ids = np.ascontiguousarray(ids, np.uint64)
        _check(lib().myslam_lcddb_append_batch(self._h, _p(ids), C.c_void_p(d_descr), n), "myslam_lcddb_append_batch")

    def append_batch_async(self, ids, d_descr, n, stream):
        """AddToDatabase inside a pipelined step: copies enqueued on `stream`, no wait (MyslamError(CAPACITY) when the rows do not fit: reserve ahead)"""
        ids = np.ascontiguousarray(ids, np.uint64)
        _check(lib().myslam_lcddb_append_batch_async(self._h, _p(ids), C.c_void_p(d_descr), n, C.c_void_p(stream or None)), "myslam_lcddb_append_batch_async")

    def query(self, descr, cur_id, thr_low=0.92):
        d = np.ascontiguousarray(descr, np.float32)
        best = C.c_uint64(); mx = C.c_float(); cnt = C.c_int()
        _check(lib().myslam_lcddb_query(self._h, _p(d), C.c_uint64(cur_id), C.c_float(thr_low), C.byref(best), C.byref(mx),
                                        C.byref(cnt)), "myslam_lcddb_query")
        return best.value, mx.value, cnt.value

    def DetectLoop(self, descr, cur_id, thr_high=0.94, thr_low=0.92):
        """bool + candidate id, the decision rule of loopclosing.cpp:147."""
        best, mx, cnt = self.query(descr, cur_id, thr_low)
        if mx < thr_high or cnt > 3:
            return False, None
        return True, best

    def generation(self):
        """number of times the descriptor matrix has moved (growth): recorded steps are valid for the generation they were recorded in"""
        return lib().myslam_lcddb_generation(self._h)

    def context(self, stream):
        """A query context on `stream` (myslam_lcddb_query_ctx): several streams scan this ONE database concurrently."""
        return LoopQueryContext(self, stream)


class LoopQueryContext(_LoopQueries):
    """myslam_lcddb_query_ctx: the per-stream half of a loop database (row-limit staging, partial results, recorded-step state).
    LoopClosing::_mvDatabase is one std::map per process (loopclosing.h:120): L streams of one GPU scan it through L contexts."""
    _prefix = "myslam_lcddb_ctx_"

    def __init__(self, db, stream):
        self._db = db                       # keeps the database alive: contexts are destroyed before it
        self._h = C.c_void_p()
        _check(lib().myslam_lcddb_query_ctx_create(C.byref(self._h), db._h, C.c_void_p(stream)), "myslam_lcddb_query_ctx_create")

    def __del__(self):
        if getattr(self, "_h", None) and self._h.value and _lib is not None and getattr(self._db, "_h", None) and self._db._h.value:
            _lib.myslam_lcddb_query_ctx_destroy(self._h)
        self._h = C.c_void_p()


LCDBANK_SCANNED, LCDBANK_GATED, LCDBANK_IDLE, LCDBANK_ADDED = 0, 1, 2, 3


class LoopDatabaseBank:
    """S loop databases in one device allocation (myslam_lcdbank_*), item s = stream s: the gate of src/loopclosing.cpp:62, DetectLoop's scan
    (:126-143) and AddToDatabase (:651-659) per stream, with ids, counts and row limits on the device.  query / append / clear take device
    pointers as ints, enqueue on the handle's stream and return (recordable, StepGraph); load / get / sizes are synchronous and take numpy arrays."""

    def __init__(self, streams, rows_per_stream, stream=None):
        self.streams, self.rows_per_stream = int(streams), int(rows_per_stream)
        self._h = C.c_void_p()
        _check(lib().myslam_lcdbank_create(C.byref(self._h), self.streams, self.rows_per_stream), "myslam_lcdbank_create")
        if stream is not None:
            self.set_stream(stream)

    def __del__(self):
        if getattr(self, "_h", None) and self._h.value and _lib is not None:
            _lib.myslam_lcdbank_destroy(self._h)
            self._h = C.c_void_p()

    def set_stream(self, stream):
        _check(lib().myslam_lcdbank_set_stream(self._h, C.c_void_p(stream)), "myslam_lcdbank_set_stream")

    @staticmethod
    def row_tile():
        """rows of one stream that one workgroup of the scan owns"""
        return lib().myslam_lcdbank_row_tile()

    @staticmethod
    def launches_per_query():
        return lib().myslam_lcdbank_launches_per_query()

    def query_batch(self, d_q, d_cur_id, d_active, d_best_id, d_max_score, d_cnt, d_best_row, d_status, thr_low=0.92, min_size=0):
        """d_q S x 1064 f32, d_cur_id S u64, d_active S i32 or None -> S each: best id u64, max score f32, cnt i32 (LoopKeyFrameStore.detect_batch's
        inputs), best row i32 (-1: nothing above 0), status i32 (LCDBANK_SCANNED / _GATED: n <= min_size / _IDLE)"""
        vp = lambda p: C.c_void_p(p or None)
        _check(lib().myslam_lcdbank_query_batch(self._h, vp(d_q), vp(d_cur_id), vp(d_active), C.c_float(thr_low), int(min_size), vp(d_best_id),
                                                vp(d_max_score), vp(d_cnt), vp(d_best_row), vp(d_status)), "myslam_lcdbank_query_batch")

    def append_batch(self, d_descr, d_id, d_add, d_status):
        """d_descr S x 1064 f32, d_id S u64, d_add S i32 or None -> d_status S i32: LCDBANK_ADDED / _IDLE / ERR_CAPACITY (stream full) / ERR_INVALID
        (id not above the last one held)"""
        vp = lambda p: C.c_void_p(p or None)
        _check(lib().myslam_lcdbank_append_batch(self._h, vp(d_descr), vp(d_id), vp(d_add), vp(d_status)), "myslam_lcdbank_append_batch")

    def clear_batch(self, d_clear):
        """d_clear S i32: the streams with a non-zero entry are empty afterwards"""
        _check(lib().myslam_lcdbank_clear_batch(self._h, C.c_void_p(d_clear or None)), "myslam_lcdbank_clear_batch")

    def view(self):
        """device pointers as ints: rows (S x rows_per_stream x 1064 f32), ids (S x rows_per_stream u64), n (S i32)"""
        r, i, n = C.c_void_p(), C.c_void_p(), C.c_void_p()
        _check(lib().myslam_lcdbank_view(self._h, C.byref(r), C.byref(i), C.byref(n)), "myslam_lcdbank_view")
        return r.value, i.value, n.value

    def read_view(self):
        """the whole allocation behind view() as numpy arrays (rows, ids, n), bytes behind the counts included; waits for nothing but its own copies"""
        S, R = self.streams, self.rows_per_stream
        out = (np.empty((S, R, LCD_DIM), np.float32), np.empty((S, R), np.uint64), np.empty(S, np.int32))
        for ptr, a in zip(self.view(), out):
            _check(lib().myslam_debug_peek(C.c_void_p(ptr), _p(a), a.nbytes), "myslam_debug_peek")
        return out

    def load(self, s, ids, rows):
        """replaces stream s with len(ids) rows (host arrays); ids ascend strictly (MyslamError(INVALID)), at most rows_per_stream (CAPACITY)"""
        ids = np.ascontiguousarray(ids, np.uint64); rows = np.ascontiguousarray(rows, np.float32).reshape(-1, LCD_DIM) if len(ids) else np.zeros((0, LCD_DIM), np.float32)
        assert len(rows) == len(ids)
        _check(lib().myslam_lcdbank_load(self._h, int(s), _p(ids) if len(ids) else None, _p(rows) if len(ids) else None, len(ids)), "myslam_lcdbank_load")

    def get(self, s):
        """(ids u64, rows f32) of stream s"""
        ids = np.zeros(self.rows_per_stream, np.uint64); rows = np.zeros((self.rows_per_stream, LCD_DIM), np.float32)
        n = C.c_int()
        _check(lib().myslam_lcdbank_get(self._h, int(s), _p(ids), _p(rows), self.rows_per_stream, C.byref(n)), "myslam_lcdbank_get")
        return ids[:n.value].copy(), rows[:n.value].copy()

    def sizes(self):
        n = np.zeros(self.streams, np.int32)
        _check(lib().myslam_lcdbank_sizes(self._h, _p(n)), "myslam_lcdbank_sizes")
        return n


class StepGraph:
    """One batched step recorded into a HIP graph (myslam_graph_begin / _end) and replayed with one launch.
        g = StepGraph.record(origin_stream, [side streams...], body)      # body() issues the step's *_batch calls on those streams
        g.launch(origin_stream)"""

    def __init__(self, handle):
        self._h = handle

    @classmethod
    def record(cls, origin, sides, body):
        arr = (C.c_void_p * max(1, len(sides)))(*[C.c_void_p(s) for s in sides])
        _check(lib().myslam_graph_begin(C.c_void_p(origin), arr, len(sides)), "myslam_graph_begin")
        err = None
        try:
            body()
        except BaseException as e:          # the capture must be closed whatever the body did
            err = e
        h = C.c_void_p()
        rc = lib().myslam_graph_end(C.c_void_p(origin), arr, len(sides), C.byref(h))
        if err is not None:
            if rc == OK:
                lib().myslam_graph_destroy(h)
            raise err
        _check(rc, "myslam_graph_end")
        return cls(h)

    def launch(self, stream):
        _check(lib().myslam_graph_launch(self._h, C.c_void_p(stream)), "myslam_graph_launch")

    def node_count(self):
        return lib().myslam_graph_node_count(self._h)

    def __del__(self):
        if getattr(self, "_h", None) and self._h.value and _lib is not None:
            _lib.myslam_graph_destroy(self._h)
            self._h = C.c_void_p()


def lcd_merge_candidates(gathered):
    """gathered: [nshards, nq] CAND_DTYPE records in ascending id-range order (host) -> (best_id u64, max_score f32, cnt i32)"""
    g = np.ascontiguousarray(gathered, CAND_DTYPE)
    assert g.ndim == 2
    ns, nq = g.shape
    best = np.zeros(nq, np.uint64); mx = np.zeros(nq, np.float32); cnt = np.zeros(nq, np.int32)
    _check(lib().myslam_lcd_merge_candidates(_p(g), ns, nq, _p(best), _p(mx), _p(cnt)), "myslam_lcd_merge_candidates")
    return best, mx, cnt


def lcd_merge_candidates_device(d_gathered, nshards, nq, d_best, d_max, d_cnt, stream=0):
    _check(lib().myslam_lcd_merge_candidates_device(d_gathered, nshards, nq, d_best, d_max, d_cnt, stream or None),
           "myslam_lcd_merge_candidates_device")


def lcd_merge_owned_candidates(gathered):
    """gathered: [nshards, nq] OWNED_DTYPE records, any shard order (host) -> (best_id u64, max_score f32, cnt i32) of ONE scan of the whole map"""
    g = np.ascontiguousarray(gathered, OWNED_DTYPE)
    assert g.ndim == 2
    ns, nq = g.shape
    best = np.zeros(nq, np.uint64); mx = np.zeros(nq, np.float32); cnt = np.zeros(nq, np.int32)
    _check(lib().myslam_lcd_merge_owned_candidates(_p(g), ns, nq, _p(best), _p(mx), _p(cnt)), "myslam_lcd_merge_owned_candidates")
    return best, mx, cnt


def lcd_merge_owned_candidates_device(d_gathered, nshards, nq, d_best, d_max, d_cnt, stream=0):
    _check(lib().myslam_lcd_merge_owned_candidates_device(d_gathered, nshards, nq, d_best, d_max, d_cnt, stream or None),
           "myslam_lcd_merge_owned_candidates_device")


# ---------------------------------------------------------------------------------- BA
def ba_build(poses, points, edge_pose, edge_pt, obs, fixed, K, delta=5.991):
    poses = np.ascontiguousarray(poses, np.float64); points = np.ascontiguousarray(points, np.float64)
    ep = np.ascontiguousarray(edge_pose, np.int32); el = np.ascontiguousarray(edge_pt, np.int32)
    obs = np.ascontiguousarray(obs, np.float64)
    fixed = np.ascontiguousarray(fixed, np.uint8) if fixed is not None else None
    P, L, E = len(poses), len(points), len(ep)
    Hpp = np.zeros((P, 6, 6)); Hll = np.zeros((L, 3, 3)); Hpl = np.zeros((E, 6, 3)); bp = np.zeros((P, 6)); bl = np.zeros((L, 3))
    chi2 = np.zeros(E)
    _check(lib().myslam_ba_build(_p(poses), P, _p(points), L, _p(ep), _p(el), _p(obs), E, _p(fixed), C.c_double(K[0]),
                                 C.c_double(K[1]), C.c_double(K[2]), C.c_double(K[3]), C.c_double(delta), _p(Hpp), _p(Hll),
                                 _p(Hpl), _p(bp), _p(bl), _p(chi2)), "myslam_ba_build")
    return Hpp, Hll, Hpl, bp, bl, chi2


def ba_build_batch(d_poses, d_points, d_ep, d_el, d_obs, d_fixed, d_sizes, nwin, maxP, maxL, maxE, K, delta,
                   d_Hpp, d_Hll, d_Hpl, d_bp, d_bl, d_chi2, stream=0):
    _check(lib().myslam_ba_build_batch(C.c_void_p(d_poses), C.c_void_p(d_points), C.c_void_p(d_ep), C.c_void_p(d_el),
                                       C.c_void_p(d_obs), C.c_void_p(d_fixed or None), C.c_void_p(d_sizes), nwin, maxP, maxL, maxE,
                                       C.c_double(K[0]), C.c_double(K[1]), C.c_double(K[2]), C.c_double(K[3]), C.c_double(delta),
                                       C.c_void_p(d_Hpp), C.c_void_p(d_Hll), C.c_void_p(d_Hpl), C.c_void_p(d_bp), C.c_void_p(d_bl),
                                       C.c_void_p(d_chi2), C.c_void_p(stream or None)), "myslam_ba_build_batch")


def ba_optimize(poses, points, edge_pose, edge_pt, obs, fixed, K, delta=5.991, iters=10):
    """optimizer.optimize(iters) of Backend::OptimizeActiveMap (backend.cpp:212-214) on the device: returns
    (poses, points, robust chi2, iterations)."""
    poses = np.ascontiguousarray(poses, np.float64).copy(); points = np.ascontiguousarray(points, np.float64).copy()
    ep = np.ascontiguousarray(edge_pose, np.int32); el = np.ascontiguousarray(edge_pt, np.int32)
    obs = np.ascontiguousarray(obs, np.float64)
    fixed = np.ascontiguousarray(fixed, np.uint8) if fixed is not None else None
    chi = C.c_double(); it = C.c_int()
    _check(lib().myslam_ba_optimize(_p(poses), len(poses), _p(points), len(points), _p(ep), _p(el), _p(obs), len(ep), _p(fixed),
                                    C.c_double(K[0]), C.c_double(K[1]), C.c_double(K[2]), C.c_double(K[3]), C.c_double(delta),
                                    int(iters), C.byref(chi), C.byref(it)), "myslam_ba_optimize")
    return poses, points, chi.value, it.value


def ba_optimize_batch(d_poses, d_points, d_ep, d_el, d_obs, d_fixed, d_sizes, nwin, maxP, maxL, maxE, K, delta, iters,
                      d_scratch, d_chi2, d_iters, d_status, stream=0):
    _check(lib().myslam_ba_optimize_batch(C.c_void_p(d_poses), C.c_void_p(d_points), C.c_void_p(d_ep), C.c_void_p(d_el),
                                          C.c_void_p(d_obs), C.c_void_p(d_fixed or None), C.c_void_p(d_sizes), nwin, maxP, maxL, maxE,
                                          C.c_double(K[0]), C.c_double(K[1]), C.c_double(K[2]), C.c_double(K[3]), C.c_double(delta),
                                          int(iters), C.c_void_p(d_scratch), C.c_void_p(d_chi2), C.c_void_p(d_iters),
                                          C.c_void_p(d_status), C.c_void_p(stream or None)), "myslam_ba_optimize_batch")


def ba_flatten_window(active_kf_ids, mp_ids, mp_outlier, mp_first_observer_kf, obs_mp_id, obs_kf_id, obs_uv, obs_feat_outlier):
    """The graph-build rules of Backend::OptimizeActiveMap (src/backend.cpp:139-206) on the Map's tables (host only).
    Returns dict(pose_src, pt_src, edge_pose, edge_pt, edge_obs, edge_src, fixed): slots -> input rows, edges grouped by landmark."""
    kf = np.ascontiguousarray(active_kf_ids, np.uint64); mp = np.ascontiguousarray(mp_ids, np.uint64)
    mo = np.ascontiguousarray(mp_outlier, np.uint8); mf = np.ascontiguousarray(mp_first_observer_kf, np.uint64)
    om = np.ascontiguousarray(obs_mp_id, np.uint64); ok = np.ascontiguousarray(obs_kf_id, np.uint64)
    uv = np.ascontiguousarray(obs_uv, np.float32).reshape(-1, 2); fo = np.ascontiguousarray(obs_feat_outlier, np.uint8)
    assert len(mp) == len(mo) == len(mf) and len(om) == len(ok) == len(uv) == len(fo)
    pose_src = np.zeros(max(len(kf), 1), np.int32); pt_src = np.zeros(max(len(mp), 1), np.int32); fixed = np.zeros(max(len(mp), 1), np.uint8)
    n = max(len(om), 1)
    ep = np.zeros(n, np.int32); el = np.zeros(n, np.int32); eo = np.zeros((n, 2), np.float64); es = np.zeros(n, np.int32)
    npt = C.c_int32(); ne = C.c_int32()
    _check(lib().myslam_ba_flatten_window(_p(kf), len(kf), _p(mp), _p(mo), _p(mf), len(mp), _p(om), _p(ok), _p(uv), _p(fo), len(om),
                                          _p(pose_src), _p(pt_src), C.byref(npt), _p(ep), _p(el), _p(eo), _p(es), C.byref(ne), _p(fixed)),
           "myslam_ba_flatten_window")
    L, E = npt.value, ne.value
    return dict(pose_src=pose_src[:len(kf)], pt_src=pt_src[:L], fixed=fixed[:L], edge_pose=ep[:E], edge_pt=el[:E], edge_obs=eo[:E], edge_src=es[:E])


def ba_optimize_active_map(poses, points, edge_pose, edge_pt, obs, fixed, K, delta=5.991, chi2_th=5.991, rounds=5, iters=10):
    """The solve stage of Backend::OptimizeActiveMap (src/backend.cpp:208-243).
    Returns (poses, points, edge_chi2, outlier flags, failed rounds, outlier count)."""
    poses = np.ascontiguousarray(poses, np.float64).copy(); points = np.ascontiguousarray(points, np.float64).copy()
    ep = np.ascontiguousarray(edge_pose, np.int32); el = np.ascontiguousarray(edge_pt, np.int32)
    obs = np.ascontiguousarray(obs, np.float64)
    fixed = np.ascontiguousarray(fixed, np.uint8) if fixed is not None else None
    chi = np.zeros(len(ep)); out = np.zeros(len(ep), np.uint8); r = C.c_int(); no = C.c_int()
    _check(lib().myslam_ba_optimize_active_map(_p(poses), len(poses), _p(points), len(points), _p(ep), _p(el), _p(obs), len(ep), _p(fixed),
                                               C.c_double(K[0]), C.c_double(K[1]), C.c_double(K[2]), C.c_double(K[3]), C.c_double(delta),
                                               C.c_double(chi2_th), int(rounds), int(iters), _p(chi), _p(out), C.byref(r), C.byref(no)),
           "myslam_ba_optimize_active_map")
    return poses, points, chi, out, r.value, no.value


BA_OPT_LANDMARKS_IN_HBM = 1
BA_OPT_BUILD_POSE_ATOMICS = 2


def ba_set_option(option, value):
    """myslam_ba_set_option: process-wide scheduling knob of the solve kernel (include/myslam_hip.h)."""
    _check(lib().myslam_ba_set_option(int(option), int(value)), "myslam_ba_set_option")


def ba_optimize_active_map_batch(d_poses, d_points, d_ep, d_el, d_obs, d_fixed, d_sizes, nwin, maxP, maxL, maxE, K, delta, chi2_th,
                                 rounds, iters, d_scratch, d_edge_chi2, d_outlier, d_rounds, d_nout, d_status, stream=0):
    _check(lib().myslam_ba_optimize_active_map_batch(
        C.c_void_p(d_poses), C.c_void_p(d_points), C.c_void_p(d_ep), C.c_void_p(d_el), C.c_void_p(d_obs), C.c_void_p(d_fixed or None),
        C.c_void_p(d_sizes), nwin, maxP, maxL, maxE, C.c_double(K[0]), C.c_double(K[1]), C.c_double(K[2]), C.c_double(K[3]),
        C.c_double(delta), C.c_double(chi2_th), int(rounds), int(iters), C.c_void_p(d_scratch), C.c_void_p(d_edge_chi2),
        C.c_void_p(d_outlier), C.c_void_p(d_rounds), C.c_void_p(d_nout), C.c_void_p(d_status), C.c_void_p(stream or None)),
        "myslam_ba_optimize_active_map_batch")


# ---------------------------------------------------------------------------------- LK tracker
class LKTracker:
    """cv::calcOpticalFlowPyrLK(..., Size(11,11), 3, TermCriteria(COUNT+EPS, 30, 0.01), OPTFLOW_USE_INITIAL_FLOW) as the reference
    calls it in Frontend::TrackLastFrame / FindFeaturesInRight (src/frontend.cpp:150-153, 358-361)."""

    def __init__(self, win=11, max_level=3, max_iters=30, eps=0.01, min_eig=1e-4, stream=None):
        self._h = C.c_void_p()
        _check(lib().myslam_lk_create(C.byref(self._h), int(win), int(max_level), int(max_iters), C.c_float(eps), C.c_float(min_eig)),
               "myslam_lk_create")
        if stream is not None:
            _check(lib().myslam_lk_set_stream(self._h, C.c_void_p(stream)), "myslam_lk_set_stream")

    def __del__(self):
        if getattr(self, "_h", None) and self._h.value and _lib is not None:
            lib().myslam_lk_destroy(self._h)
            self._h = C.c_void_p()

    def track(self, prev, nxt, prev_pts, next_pts):
        """host arrays; returns (next_pts, status bool, err)"""
        prev = np.ascontiguousarray(prev, np.uint8); nxt = np.ascontiguousarray(nxt, np.uint8)
        pp = np.ascontiguousarray(prev_pts, np.float32).reshape(-1, 2)
        npts = np.ascontiguousarray(next_pts, np.float32).reshape(-1, 2).copy()
        n = len(pp); st = np.zeros(max(n, 1), np.uint8); err = np.zeros(max(n, 1), np.float32)
        _check(lib().myslam_lk_track(self._h, _p(prev), _p(nxt), prev.shape[0], prev.shape[1], prev.strides[0], nxt.strides[0],
                                     _p(pp), _p(npts), n, _p(st), _p(err)), "myslam_lk_track")
        return npts, st[:n].astype(bool), err[:n]

    def track_cached(self, prev, prev_token, nxt, next_token, prev_pts, next_pts):
        """track() with the handle's two-image cache: a non-zero token names an image whose bytes never change (myslam_lk_track_cached)"""
        prev = np.ascontiguousarray(prev, np.uint8); nxt = np.ascontiguousarray(nxt, np.uint8)
        pp = np.ascontiguousarray(prev_pts, np.float32).reshape(-1, 2)
        npts = np.ascontiguousarray(next_pts, np.float32).reshape(-1, 2).copy()
        n = len(pp); st = np.zeros(max(n, 1), np.uint8); err = np.zeros(max(n, 1), np.float32)
        _check(lib().myslam_lk_track_cached(self._h, _p(prev), C.c_uint64(prev_token), _p(nxt), C.c_uint64(next_token), prev.shape[0], prev.shape[1],
                                            prev.strides[0], nxt.strides[0], _p(pp), _p(npts), n, _p(st), _p(err)), "myslam_lk_track_cached")
        return npts, st[:n].astype(bool), err[:n]

    def prefetch(self, img, token):
        """asynchronous upload + pyramid of an image the next track_cached() call will name by `token`; the array must stay alive until then"""
        img = np.ascontiguousarray(img, np.uint8)
        self._keep = img
        _check(lib().myslam_lk_prefetch(self._h, _p(img), C.c_uint64(token), img.shape[0], img.shape[1], img.strides[0]), "myslam_lk_prefetch")

    def track_batch(self, d_prev, d_next, batch, rows, cols, step, stride, d_prev_pts, d_next_pts, d_counts, cap, d_status, d_err=0):
        _check(lib().myslam_lk_track_batch(self._h, C.c_void_p(d_prev), C.c_void_p(d_next), batch, rows, cols, step, C.c_size_t(stride),
                                           C.c_void_p(d_prev_pts), C.c_void_p(d_next_pts), C.c_void_p(d_counts), cap,
                                           C.c_void_p(d_status), C.c_void_p(d_err or None)), "myslam_lk_track_batch")


# ---------------------------------------------------------------------------------- multi-stream tracker
TRACKER_RESULT_DTYPE = np.dtype([("pose7", "<f8", (7,)), ("n_inliers", "<i4"), ("n_features", "<i4"), ("status", "<i4"), ("frame_id", "<i4"),
                                 ("needs_host", "<i4"), ("reserved", "<i4")])      # myslam_tracker_result
assert TRACKER_RESULT_DTYPE.itemsize == 80


class Tracker:
    """Frontend::Track() (src/frontend.cpp:86-122) for `streams` independent cameras of one image size and calibration, one frame per
    step_batch() with all tracker state on the device (myslam_tracker_*).  K = (fx, fy, cx, cy).  A stream's state travels as a dict:
    xy (n, 2) f32, lm (n,) i32 slots of the landmark table or -1, lm_pos (L, 3) f64, lm_outlier (L,) u8, ref_pose (7,), ref_frame_id,
    last_rel / rel_motion (4, 4), next_frame_id, status, kf_every; get_frame() adds frozen and outlier_list (landmark slots)."""

    def __init__(self, streams, rows, cols, cap, landmark_cap, K, tracking_good=50, tracking_bad=10, win=11, max_level=3, max_iters=30, eps=0.01,
                 min_eig=1e-4, stream=None):
        self.streams, self.rows, self.cols, self.cap, self.landmark_cap = int(streams), int(rows), int(cols), int(cap), int(landmark_cap)
        self._h = C.c_void_p()
        _check(lib().myslam_tracker_create(C.byref(self._h), self.streams, self.rows, self.cols, self.cap, self.landmark_cap, C.c_double(K[0]),
                                           C.c_double(K[1]), C.c_double(K[2]), C.c_double(K[3]), int(tracking_good), int(tracking_bad), int(win),
                                           int(max_level), int(max_iters), C.c_float(eps), C.c_float(min_eig)), "myslam_tracker_create")
        if stream is not None:
            self.set_stream(stream)

    def __del__(self):
        if getattr(self, "_h", None) and self._h.value and _lib is not None:
            lib().myslam_tracker_destroy(self._h)
            self._h = C.c_void_p()

    def set_stream(self, stream):
        _check(lib().myslam_tracker_set_stream(self._h, C.c_void_p(stream)), "myslam_tracker_set_stream")

    def launches_per_step(self):
        return lib().myslam_tracker_launches_per_step(self._h)

    def set_frame(self, s, state, image=None):
        """key-frame hand-off (host arrays, synchronous): uploads the state, unfreezes the stream; image replaces the stored previous image"""
        xy = np.ascontiguousarray(state["xy"], np.float32).reshape(-1, 2); lm = np.ascontiguousarray(state["lm"], np.int32).reshape(-1)
        pos = np.ascontiguousarray(state["lm_pos"], np.float64).reshape(-1, 3); out = np.ascontiguousarray(state["lm_outlier"], np.uint8).reshape(-1)
        if len(xy) != len(lm) or len(pos) != len(out):
            raise ValueError("feature / landmark arrays of different lengths")
        ref = np.ascontiguousarray(state["ref_pose"], np.float64).reshape(7)
        rel = np.ascontiguousarray(state["last_rel"], np.float64).reshape(16); mot = np.ascontiguousarray(state["rel_motion"], np.float64).reshape(16)
        img, step = None, 0
        if image is not None:
            img = np.ascontiguousarray(image, np.uint8)
            if img.shape != (self.rows, self.cols):
                raise ValueError(f"expected a {self.rows} x {self.cols} image")
            step = img.strides[0]
        _check(lib().myslam_tracker_set_frame(self._h, int(s), _p(xy), _p(lm), len(xy), _p(pos), _p(out), len(pos), _p(ref), int(state["ref_frame_id"]),
                                              _p(rel), _p(mot), int(state["next_frame_id"]), int(state["status"]), int(state.get("kf_every", 0)),
                                              _p(img), step), "myslam_tracker_set_frame")

    def get_frame(self, s, image=False):
        xy = np.zeros((self.cap, 2), np.float32); lm = np.zeros(self.cap, np.int32)
        pos = np.zeros((self.landmark_cap, 3), np.float64); out = np.zeros(self.landmark_cap, np.uint8)
        ref = np.zeros(7); rel = np.zeros((4, 4)); mot = np.zeros((4, 4)); lst = np.zeros(2 * self.cap, np.int32)
        iv = [C.c_int() for _ in range(8)]          # n_feat n_landmarks ref_frame_id next_frame_id status kf_every frozen n_outlier
        img = np.zeros((self.rows, self.cols), np.uint8) if image else None
        _check(lib().myslam_tracker_get_frame(self._h, int(s), _p(xy), _p(lm), C.byref(iv[0]), _p(pos), _p(out), C.byref(iv[1]), _p(ref), C.byref(iv[2]),
                                              _p(rel), _p(mot), C.byref(iv[3]), C.byref(iv[4]), C.byref(iv[5]), C.byref(iv[6]), _p(lst), C.byref(iv[7]),
                                              _p(img), self.cols if image else 0), "myslam_tracker_get_frame")
        n, L = iv[0].value, iv[1].value
        st = {"xy": xy[:n].copy(), "lm": lm[:n].copy(), "lm_pos": pos[:L].copy(), "lm_outlier": out[:L].copy(), "ref_pose": ref,
              "ref_frame_id": iv[2].value, "last_rel": rel, "rel_motion": mot, "next_frame_id": iv[3].value, "status": iv[4].value,
              "kf_every": iv[5].value, "frozen": iv[6].value, "outlier_list": lst[:iv[7].value].copy()}
        if image:
            st["image"] = img
        return st

    def step_batch(self, d_left, step, stride, d_results):
        """device pointers, asynchronous on the handle's stream: image s at d_left + s * stride; d_results: `streams` TRACKER_RESULT_DTYPE records"""
        _check(lib().myslam_tracker_step_batch(self._h, C.c_void_p(d_left), int(step), C.c_size_t(stride), C.c_void_p(d_results)),
               "myslam_tracker_step_batch")

    def debug_last_step(self, s):
        """(p0, p1, tracked, LK status) of stream s in the last step; empty when it was frozen"""
        p0 = np.zeros((self.cap, 2), np.float32); p1 = np.zeros((self.cap, 2), np.float32); nx = np.zeros((self.cap, 2), np.float32)
        st = np.zeros(self.cap, np.uint8); n = C.c_int()
        _check(lib().myslam_tracker_debug_last_step(self._h, int(s), _p(p0), _p(p1), _p(nx), _p(st), C.byref(n)), "myslam_tracker_debug_last_step")
        return p0[:n.value], p1[:n.value], nx[:n.value], st[:n.value].astype(bool)

    # ---- key-frame turns on the device (myslam_tracker_keyframe_*: the header states every rule) ----
    NO_TURN = 1                                  # MYSLAM_TRACKER_NO_TURN
    REPORT_FIELDS = ("status", "frame_id", "n_detected", "n_right", "n_new_mp", "n_feat", "n_landmarks", "reserved")

    def set_ids(self, s, landmark_id, ref_kf_id, next_kf_id, next_mp_id):
        """MapPoint::mnId by landmark slot and the stream's id counters (host arrays, synchronous); makes the stream's ids valid"""
        ids = np.ascontiguousarray(landmark_id, np.int64).reshape(-1)
        _check(lib().myslam_tracker_set_ids(self._h, int(s), _p(ids), len(ids), int(ref_kf_id), int(next_kf_id), int(next_mp_id)), "myslam_tracker_set_ids")

    def get_ids(self, s):
        ids = np.zeros(self.landmark_cap, np.int64); n, valid = C.c_int(), C.c_int()
        ref, nkf, nmp = C.c_int64(), C.c_int64(), C.c_int64()
        _check(lib().myslam_tracker_get_ids(self._h, int(s), _p(ids), C.byref(n), C.byref(ref), C.byref(nkf), C.byref(nmp), C.byref(valid)),
               "myslam_tracker_get_ids")
        return {"landmark_id": ids[:n.value].copy(), "ref_kf_id": ref.value, "next_kf_id": nkf.value, "next_mp_id": nmp.value, "valid": valid.value}

    def keyframe_masks(self, d_masks, step, stride):
        """device pointer, asynchronous: every stream's detection mask in myslam_orb_detect_batch's d_masks layout (all 0 for a stream without a turn)"""
        _check(lib().myslam_tracker_keyframe_masks(self._h, C.c_void_p(d_masks), int(step), C.c_size_t(stride)), "myslam_tracker_keyframe_masks")

    def keyframe_launches(self):
        return lib().myslam_tracker_keyframe_launches(self._h)

    # the outputs of a turn and of an init, in the order of the C calls' trailing pointers
    TURN_OUTPUTS = ("new_kf_id", "new_kf_pose", "feat_mp_id", "feat_mp_pos", "feat_uv", "feat_tag", "feat_flags", "n_feat", "outlier_mp_id", "n_outlier_mp",
                    "right_xy", "right_ok", "report")

    def keyframe_batch(self, d_right, step, stride, d_new_kps, d_n_new, kp_cap, baseline, out):
        """device pointers, asynchronous.  out: dict of device pointers, one per name in TURN_OUTPUTS (sizes: the header; feature stride = cap,
        outlier stride = 2 cap)"""
        o = [C.c_void_p(out[k]) for k in self.TURN_OUTPUTS]
        _check(lib().myslam_tracker_keyframe_batch(self._h, C.c_void_p(d_right), int(step), C.c_size_t(stride), C.c_void_p(d_new_kps), C.c_void_p(d_n_new),
                                                   int(kp_cap), C.c_double(baseline), *o), "myslam_tracker_keyframe_batch")

    def debug_last_turn(self, s):
        """(left pixels, right points, right status, triangulation in the camera frame, its ok) of stream s in the last turn; empty without one"""
        xy = np.zeros((self.cap, 2), np.float32); rx = np.zeros((self.cap, 2), np.float32); ro = np.zeros(self.cap, np.uint8)
        tx = np.zeros((self.cap, 3), np.float64); to = np.zeros(self.cap, np.uint8); n = C.c_int()
        _check(lib().myslam_tracker_debug_last_turn(self._h, int(s), _p(xy), _p(rx), _p(ro), _p(tx), _p(to), C.byref(n)), "myslam_tracker_debug_last_turn")
        n = n.value
        return xy[:n], rx[:n], ro[:n].astype(bool), tx[:n], to[:n].astype(bool)

    def debug_freeze(self, s, why=1):
        """test seam: freeze stream s as a step would, recording why (1 key-frame rule, 2 LOST, 3 capacity)"""
        _check(lib().myslam_tracker_debug_freeze(self._h, int(s), int(why)), "myslam_tracker_debug_freeze")

    def update_from_map(self, d_kf_id, d_kf_pose, d_n_kf, kf_cap, d_mp_id, d_mp_pos, d_mp_outlier, d_n_mp, mp_cap):
        """device pointers, asynchronous: landmarks and the reference pose of every running stream follow their ids in the back end's tables"""
        _check(lib().myslam_tracker_update_from_map_batch(self._h, C.c_void_p(d_kf_id), C.c_void_p(d_kf_pose), C.c_void_p(d_n_kf), int(kf_cap),
                                                          C.c_void_p(d_mp_id), C.c_void_p(d_mp_pos), C.c_void_p(d_mp_outlier), C.c_void_p(d_n_mp),
                                                          int(mp_cap)), "myslam_tracker_update_from_map_batch")

    def clear_links_batch(self, d_kf_id, d_tag, d_n, list_cap, d_n_cleared=None):
        """device pointers, asynchronous: Backend.culled_view()'s lists (stream s at + s * list_cap).  A stream with valid ids whose last frame is its
        reference key-frame's frame (no step since the turn or the init) drops the landmark of every listed feature of that key-frame; any other
        stream keeps every byte.  d_n_cleared `streams` i32 or None."""
        _check(lib().myslam_tracker_clear_links_batch(self._h, C.c_void_p(d_kf_id or None), C.c_void_p(d_tag or None), C.c_void_p(d_n or None),
                                                      int(list_cap), C.c_void_p(d_n_cleared or None)), "myslam_tracker_clear_links_batch")

    def relink_batch(self, d_kf_id, d_tag, d_slot, d_n, list_cap, map_archive, d_n_relinked=None, d_status=None):
        """device pointers, asynchronous: Relink.view()'s link lists (stream s at + s * list_cap) against `map_archive` (item s = stream s).  Guard of
        clear_links_batch; the landmark of every listed feature of the reference key-frame takes the target's id, position and outlier flag
        (src/loopclosing.cpp:524, :529), a feature without one gets the slot that carries the id or a new one, slot -1 drops the landmark.
        d_status `streams` i32 = 0 / ERR_INVALID / ERR_CAPACITY (the stream then keeps every byte); d_n_relinked `streams` i32 or None."""
        vp = lambda p: C.c_void_p(p or None)
        _check(lib().myslam_tracker_relink_batch(self._h, vp(d_kf_id), vp(d_tag), vp(d_slot), vp(d_n), int(list_cap), map_archive._h if map_archive else None,
                                                 vp(d_n_relinked), vp(d_status)), "myslam_tracker_relink_batch")

    def set_image_batch(self, d_imgs, step, stride, d_select):
        """device pointers, asynchronous: the stored previous left image of every selected stream <- d_imgs[s], pyramid rebuilt"""
        _check(lib().myslam_tracker_set_image_batch(self._h, C.c_void_p(d_imgs), int(step), C.c_size_t(stride), C.c_void_p(d_select)),
               "myslam_tracker_set_image_batch")

    # ---- StereoInit on the device (myslam_tracker_init_*: the header states every rule) ----
    INIT_RETRY = 2                               # MYSLAM_TRACKER_INIT_RETRY

    def reset_stream(self, s, next_frame_id=0, next_kf_id=0, next_mp_id=0, kf_every=0):
        """host call, synchronous: stream s back into the created (init-eligible) state, with the given id counters"""
        _check(lib().myslam_tracker_reset_stream(self._h, int(s), int(next_frame_id), int(next_kf_id), int(next_mp_id), int(kf_every)),
               "myslam_tracker_reset_stream")

    def init_masks(self, d_masks, step, stride):
        """device pointer, asynchronous: all 255 for every init-eligible stream, all 0 for the others (keyframe_masks' layout)"""
        _check(lib().myslam_tracker_init_masks(self._h, C.c_void_p(d_masks), int(step), C.c_size_t(stride)), "myslam_tracker_init_masks")

    def init_launches(self):
        return lib().myslam_tracker_init_launches(self._h)

    def init_batch(self, d_left, d_right, step, stride, d_new_kps, d_n_new, kp_cap, baseline, init_good, out):
        """device pointers, asynchronous: StereoInit of every init-eligible stream.  out: keyframe_batch's dict of device pointers"""
        o = [C.c_void_p(out[k]) for k in self.TURN_OUTPUTS]
        _check(lib().myslam_tracker_init_batch(self._h, C.c_void_p(d_left), C.c_void_p(d_right), int(step), C.c_size_t(stride), C.c_void_p(d_new_kps),
                                               C.c_void_p(d_n_new), int(kp_cap), C.c_double(baseline), int(init_good), *o), "myslam_tracker_init_batch")


# ---------------------------------------------------------------------------------- lens undistortion
class Undistorter:
    """Camera::UndistortImage (src/camera.cpp:36-48) = cv::undistort(src, dst, K, D) for one camera at one image size, as
    Frontend::GrabStereoImage runs it when Camera.bNeedUndistortion is 1 (src/frontend.cpp:47-51).  K = (fx, fy, cx, cy),
    D = (k1, k2, p1, p2), both passed as float."""

    def __init__(self, rows, cols, K, D, stream=None):
        self.rows, self.cols = int(rows), int(cols)
        k = np.ascontiguousarray(K, np.float32).reshape(4); d = np.ascontiguousarray(D, np.float32).reshape(4)
        self._h = C.c_void_p()
        _check(lib().myslam_undistort_create(C.byref(self._h), self.rows, self.cols, _p(k), _p(d)), "myslam_undistort_create")
        if stream is not None:
            _check(lib().myslam_undistort_set_stream(self._h, C.c_void_p(stream)), "myslam_undistort_set_stream")

    def __del__(self):
        if getattr(self, "_h", None) and self._h.value and _lib is not None:
            lib().myslam_undistort_destroy(self._h)
            self._h = C.c_void_p()

    def set_stream(self, stream):
        _check(lib().myslam_undistort_set_stream(self._h, C.c_void_p(stream)), "myslam_undistort_set_stream")

    def UndistortImage(self, src, dst=None):
        """host arrays (rows x cols uint8, any row pitch); dst=None returns a new array, dst=src undistorts in place"""
        if src.dtype != np.uint8 or src.shape != (self.rows, self.cols) or src.strides[1] != 1:
            raise ValueError(f"expected a {self.rows} x {self.cols} uint8 image with unit column stride")
        if dst is None:
            dst = np.empty((self.rows, self.cols), np.uint8)
        if dst.dtype != np.uint8 or dst.shape != (self.rows, self.cols) or dst.strides[1] != 1:
            raise ValueError(f"expected a {self.rows} x {self.cols} uint8 output with unit column stride")
        _check(lib().myslam_undistort_image(self._h, _p(src), src.strides[0], _p(dst), dst.strides[0]), "myslam_undistort_image")
        return dst

    def batch(self, d_src, batch, src_step, src_stride, d_dst, dst_step, dst_stride):
        """device pointers, asynchronous on the handle's stream"""
        _check(lib().myslam_undistort_batch(self._h, C.c_void_p(d_src), int(batch), int(src_step), C.c_size_t(src_stride), C.c_void_p(d_dst),
                                            int(dst_step), C.c_size_t(dst_stride)), "myslam_undistort_batch")

    def get_map(self):
        """OpenCV's maps: xy (rows, cols, 2) int16 (CV_16SC2) and frac (rows, cols) uint16 (CV_16UC1)"""
        xy = np.empty((self.rows, self.cols, 2), np.int16); frac = np.empty((self.rows, self.cols), np.uint16)
        _check(lib().myslam_undistort_get_map(self._h, _p(xy), _p(frac)), "myslam_undistort_get_map")
        return xy, frac


# ---------------------------------------------------------------------------------- pose-only optimisation
def pose_only_optimize(pose, pts3d, obs, K, chi2_th=5.991, rounds=4, iters=10, pre_optimize=0):
    """The g2o part of Frontend::EstimateCurrentPose (src/frontend.cpp:176-276).  Returns (pose7, outlier flags, inlier count)."""
    pose = np.ascontiguousarray(pose, np.float64).copy()
    pts3d = np.ascontiguousarray(pts3d, np.float64).reshape(-1, 3); obs = np.ascontiguousarray(obs, np.float64).reshape(-1, 2)
    n = len(pts3d); out = np.zeros(max(n, 1), np.uint8); ni = C.c_int()
    _check(lib().myslam_pose_only_optimize(_p(pose), _p(pts3d), _p(obs), n, C.c_double(K[0]), C.c_double(K[1]), C.c_double(K[2]),
                                           C.c_double(K[3]), C.c_double(chi2_th), int(rounds), int(iters), int(pre_optimize), _p(out), C.byref(ni)),
           "myslam_pose_only_optimize")
    return pose, out[:n].astype(bool), ni.value


def pose_only_optimize_batch(d_poses, d_pts3d, d_obs, d_counts, batch, cap, K, chi2_th, rounds, iters, d_outlier, d_ninl, d_status, stream=0,
                             pre_optimize=0):
    _check(lib().myslam_pose_only_optimize_batch(C.c_void_p(d_poses), C.c_void_p(d_pts3d), C.c_void_p(d_obs), C.c_void_p(d_counts), batch, cap,
                                                 C.c_double(K[0]), C.c_double(K[1]), C.c_double(K[2]), C.c_double(K[3]), C.c_double(chi2_th),
                                                 int(rounds), int(iters), int(pre_optimize), C.c_void_p(d_outlier), C.c_void_p(d_ninl), C.c_void_p(d_status),
                                                 C.c_void_p(stream or None)), "myslam_pose_only_optimize_batch")


# ---------------------------------------------------------------------------------- loop correction
def pose_graph_optimize(poses, fixed, edge_v0, edge_v1, meas, iters=20):
    """The g2o part of LoopClosing::PoseGraphOptimization (src/loopclosing.cpp:537-610).  poses (n,7) Tcw; meas[k] = the
    measured T[v0] * T[v1]^-1 of edge k.  Returns (poses, final chi2, iterations done)."""
    poses = np.ascontiguousarray(poses, np.float64).reshape(-1, 7).copy(); fixed = np.ascontiguousarray(fixed, np.uint8)
    e0 = np.ascontiguousarray(edge_v0, np.int32); e1 = np.ascontiguousarray(edge_v1, np.int32)
    meas = np.ascontiguousarray(meas, np.float64).reshape(-1, 7)
    assert len(fixed) == len(poses) and len(e0) == len(e1) == len(meas)
    chi = C.c_double(); it = C.c_int()
    _check(lib().myslam_pose_graph_optimize(_p(poses), len(poses), _p(fixed), _p(e0), _p(e1), _p(meas), len(e0), int(iters), C.byref(chi), C.byref(it)),
           "myslam_pose_graph_optimize")
    return poses, chi.value, it.value


def correct_map_points(old_poses, new_poses, first_kf, points):
    """src/loopclosing.cpp:621-633: every map point keeps its camera-frame position in the key-frame that first observed it."""
    old_poses = np.ascontiguousarray(old_poses, np.float64).reshape(-1, 7); new_poses = np.ascontiguousarray(new_poses, np.float64).reshape(-1, 7)
    first_kf = np.ascontiguousarray(first_kf, np.int32); points = np.ascontiguousarray(points, np.float64).reshape(-1, 3).copy()
    assert old_poses.shape == new_poses.shape and len(first_kf) == len(points)
    _check(lib().myslam_correct_map_points(_p(old_poses), _p(new_poses), len(old_poses), _p(first_kf), _p(points), len(points)), "myslam_correct_map_points")
    return points


def loop_local_fusion(active_poses, cur, corrected_cur, first_active_kf, points):
    """LoopClosing::LoopLocalFusion (src/loopclosing.cpp:466-507), arithmetic part: returns (corrected active poses, corrected points)"""
    poses = np.ascontiguousarray(active_poses, np.float64).reshape(-1, 7).copy(); cc = np.ascontiguousarray(corrected_cur, np.float64)
    kf = np.ascontiguousarray(first_active_kf, np.int32); pts = np.ascontiguousarray(points, np.float64).reshape(-1, 3).copy()
    assert len(kf) == len(pts)
    _check(lib().myslam_loop_local_fusion(_p(poses), len(poses), int(cur), _p(cc), _p(kf), _p(pts), len(pts)), "myslam_loop_local_fusion")
    return poses, pts


def solve_pnp_ransac(pts3d, pts2d, K, iterations=100, reproj_error=5.991, confidence=0.99):
    """cv::solvePnPRansac as LoopClosing::ComputeCorrectPose calls it (src/loopclosing.cpp:262-268).
    Returns (pose7 Tcw, inlier flags, inlier count); raises MyslamError(UNSUPPORTED) when no model exists."""
    p3 = np.ascontiguousarray(pts3d, np.float32).reshape(-1, 3); p2 = np.ascontiguousarray(pts2d, np.float32).reshape(-1, 2)
    assert len(p3) == len(p2)
    n = len(p3); pose = np.zeros(7); inl = np.zeros(max(n, 1), np.uint8); ni = C.c_int()
    _check(lib().myslam_solve_pnp_ransac(_p(p3), _p(p2), n, C.c_double(K[0]), C.c_double(K[1]), C.c_double(K[2]), C.c_double(K[3]), int(iterations),
                                         C.c_double(reproj_error), C.c_double(confidence), _p(pose), _p(inl), C.byref(ni)), "myslam_solve_pnp_ransac")
    return pose, inl[:n].astype(bool), ni.value


VERIFY_CONFIRMED, VERIFY_NO_MODEL, VERIFY_FEW_MATCHES, VERIFY_FEW_INLIERS = 0, 1, 2, 3      # MYSLAM_VERIFY_*


class PnPSolver:
    """Loop verification for a batch of candidates on the device (myslam_pnp_*): the handle owns the workspace of `max_batch` items of `cap`
    match slots and `max_iterations` hypotheses, the calls take device pointers as ints, enqueue on the handle's stream and return.
    K = (fx, fy, cx, cy)."""

    def __init__(self, max_batch, cap, max_iterations=100, stream=None):
        self.max_batch, self.cap, self.max_iterations = int(max_batch), int(cap), int(max_iterations)
        self._h = C.c_void_p()
        _check(lib().myslam_pnp_create(C.byref(self._h), self.max_batch, self.cap, self.max_iterations), "myslam_pnp_create")
        if stream is not None:
            self.set_stream(stream)

    def __del__(self):
        if getattr(self, "_h", None) and self._h.value and _lib is not None:
            lib().myslam_pnp_destroy(self._h)
            self._h = C.c_void_p()

    def set_stream(self, stream):
        _check(lib().myslam_pnp_set_stream(self._h, C.c_void_p(stream)), "myslam_pnp_set_stream")

    def solve_batch(self, d_pts3d, d_pts2d, d_counts, batch, K, d_pose7, d_inlier, d_n_inliers, d_status, iterations=100, reproj_error=5.991,
                    confidence=0.99):
        """cv::solvePnPRansac (src/loopclosing.cpp:262-272) per item: d_pts3d batch x cap x 3 f32, d_pts2d batch x cap x 2 f32, d_counts batch i32;
        d_pose7 batch x 7 f64, d_inlier batch x cap u8, d_n_inliers / d_status batch i32 (status 0 = model, 1 = none: pose left alone)"""
        _check(lib().myslam_solve_pnp_ransac_batch(self._h, C.c_void_p(d_pts3d), C.c_void_p(d_pts2d), C.c_void_p(d_counts), int(batch), C.c_double(K[0]),
                                                   C.c_double(K[1]), C.c_double(K[2]), C.c_double(K[3]), int(iterations), C.c_double(reproj_error),
                                                   C.c_double(confidence), C.c_void_p(d_pose7), C.c_void_p(d_inlier), C.c_void_p(d_n_inliers),
                                                   C.c_void_p(d_status)), "myslam_solve_pnp_ransac_batch")

    def verify_batch(self, d_pts3d, d_pts2d, d_counts, batch, K, d_pose7, d_outlier, d_n_inliers, d_status, d_pnp_pose7=0, d_pnp_inlier=0, iterations=100,
                     reproj_error=5.991, confidence=0.99, min_matches=10, chi2_th=5.991, rounds=4, iters=10):
        """LoopClosing::ComputeCorrectPose's arithmetic (src/loopclosing.cpp:208-335) per item: PnP-RANSAC, then the pose-only optimisation with
        pre_optimize 1 over all the item's matches; d_status batch i32 = VERIFY_*; d_pnp_pose7 / d_pnp_inlier (optional): PnP's own pose and mask"""
        _check(lib().myslam_loop_verify_batch(self._h, C.c_void_p(d_pts3d), C.c_void_p(d_pts2d), C.c_void_p(d_counts), int(batch), C.c_double(K[0]),
                                              C.c_double(K[1]), C.c_double(K[2]), C.c_double(K[3]), int(iterations), C.c_double(reproj_error),
                                              C.c_double(confidence), int(min_matches), C.c_double(chi2_th), int(rounds), int(iters), C.c_void_p(d_pose7),
                                              C.c_void_p(d_outlier), C.c_void_p(d_n_inliers), C.c_void_p(d_status), C.c_void_p(d_pnp_pose7 or None),
                                              C.c_void_p(d_pnp_inlier or None)), "myslam_loop_verify_batch")


LOOP_CORRECT_DONE, LOOP_CORRECT_NOT_NEEDED, LOOP_CORRECT_SKIPPED, LOOP_CORRECT_FUSED_ONLY = 0, 1, 2, 3      # MYSLAM_LOOP_CORRECT_*
LOOP_CORRECT_MAX_SEPARATORS = 32                                                                           # MYSLAM_LOOP_CORRECT_MAX_SEPARATORS


class LoopCorrector:
    """LoopClosing::LoopCorrect's arithmetic (src/loopclosing.cpp:437-463) for a batch of maps on the device (myslam_loop_corrector_*): the handle owns
    the workspace of `max_batch` maps of up to `kf_cap` key-frames, `edge_cap` edges, `active_cap` active key-frames and `point_cap` map points; the
    call takes device pointers as ints, enqueues on the handle's stream and returns."""

    def __init__(self, max_batch, kf_cap, edge_cap, active_cap, point_cap, stream=None):
        self.max_batch, self.kf_cap, self.edge_cap, self.active_cap, self.point_cap = int(max_batch), int(kf_cap), int(edge_cap), int(active_cap), int(point_cap)
        self._h = C.c_void_p()
        _check(lib().myslam_loop_corrector_create(C.byref(self._h), self.max_batch, self.kf_cap, self.edge_cap, self.active_cap, self.point_cap),
               "myslam_loop_corrector_create")
        if stream is not None:
            self.set_stream(stream)

    def __del__(self):
        if getattr(self, "_h", None) and self._h.value and _lib is not None:
            lib().myslam_loop_corrector_destroy(self._h)
            self._h = C.c_void_p()

    def set_stream(self, stream):
        _check(lib().myslam_loop_corrector_set_stream(self._h, C.c_void_p(stream)), "myslam_loop_corrector_set_stream")

    def correct_batch(self, d_poses, d_n_kf, d_active, d_n_active, d_cur, d_loop, d_corrected_pose7, d_verify_status, d_edge_v0, d_edge_v1, d_meas,
                      d_n_edges, d_points, d_n_points, d_first_active, d_first_kf, batch, correct_threshold, max_iters, d_chi2, d_iters, d_status):
        """The loop edge (:328-330), the need-correct test (:284-289), LoopLocalFusion (:470-507), PoseGraphOptimization (:537-610) and its write-back
        (:612-641) per item, arguments in the header's order, tables strided by the handle's caps (include/myslam_hip.h); d_verify_status 0 / None =
        every item is confirmed; correct_threshold = 1.0 (:285) and max_iters = 20 (:606) at the reference's call site;
        d_status batch i32 = LOOP_CORRECT_* or a negative error, d_chi2 batch f64, d_iters batch i32"""
        _check(lib().myslam_loop_correct_batch(self._h, C.c_void_p(d_poses), C.c_void_p(d_n_kf), C.c_void_p(d_active), C.c_void_p(d_n_active),
                                               C.c_void_p(d_cur), C.c_void_p(d_loop), C.c_void_p(d_corrected_pose7), C.c_void_p(d_verify_status or None),
                                               C.c_void_p(d_edge_v0), C.c_void_p(d_edge_v1), C.c_void_p(d_meas), C.c_void_p(d_n_edges),
                                               C.c_void_p(d_points or None), C.c_void_p(d_n_points), C.c_void_p(d_first_active or None),
                                               C.c_void_p(d_first_kf or None), int(batch), C.c_double(correct_threshold), int(max_iters),
                                               C.c_void_p(d_chi2), C.c_void_p(d_iters), C.c_void_p(d_status)), "myslam_loop_correct_batch")


BACKEND_DONE, BACKEND_EMPTY = 0, 1                     # MYSLAM_BACKEND_*
BACKEND_OBS_ACTIVE, BACKEND_OBS_OUTLIER = 1, 2         # bits of d_obs_flags
BA_MAX_WINDOW_POSES = 10                               # MYSLAM_BA_MAX_WINDOW_POSES


class Backend:
    """Backend::OptimizeActiveMap (src/backend.cpp:126-266) for a batch of active maps held in device tables (myslam_backend_*): the handle owns the
    flat windows and the solve's workspace for `max_batch` maps of up to `kf_cap` key-frames, `mp_cap` map points and `obs_cap` observation rows; the
    call takes device pointers as ints, enqueues three launches on the handle's stream and returns."""

    def __init__(self, max_batch, kf_cap, mp_cap, obs_cap, stream=None):
        self.max_batch, self.kf_cap, self.mp_cap, self.obs_cap = int(max_batch), int(kf_cap), int(mp_cap), int(obs_cap)
        self._h = C.c_void_p()
        _check(lib().myslam_backend_create(C.byref(self._h), self.max_batch, self.kf_cap, self.mp_cap, self.obs_cap), "myslam_backend_create")
        if stream is not None:
            self.set_stream(stream)

    def __del__(self):
        if getattr(self, "_h", None) and self._h.value and _lib is not None:
            lib().myslam_backend_destroy(self._h)
            self._h = C.c_void_p()

    def set_stream(self, stream):
        _check(lib().myslam_backend_set_stream(self._h, C.c_void_p(stream)), "myslam_backend_set_stream")

    def launches_per_call(self):
        return lib().myslam_backend_launches_per_call(self._h)

    def optimize_batch(self, d_kf_id, d_kf_pose, d_n_kf, d_mp_id, d_mp_pos, d_mp_outlier, d_n_mp, d_obs_mp, d_obs_kf, d_obs_flags, d_obs_uv, d_obs_tag,
                       d_n_obs, batch, K, d_obs_report, d_mp_report, d_new_outlier_mp, d_n_new_outlier_mp, d_obs_chi2, d_rounds, d_n_outlier_edges,
                       d_status, delta=5.991, chi2_th=5.991, rounds=5, iters=10):
        """Graph build (:139-206), solve (:208-243) and write-back (:234-266, map.cpp:126-175) per item, arguments in the header's order, tables strided
        by the handle's caps and updated in place (include/myslam_hip.h); K = (fx, fy, cx, cy); d_status batch i32 = BACKEND_DONE / BACKEND_EMPTY or
        a negative error"""
        ptrs = [C.c_void_p(p) for p in (d_kf_id, d_kf_pose, d_n_kf, d_mp_id, d_mp_pos, d_mp_outlier, d_n_mp, d_obs_mp, d_obs_kf, d_obs_flags, d_obs_uv,
                                        d_obs_tag, d_n_obs)]
        outs = [C.c_void_p(p) for p in (d_obs_report, d_mp_report, d_new_outlier_mp, d_n_new_outlier_mp, d_obs_chi2, d_rounds, d_n_outlier_edges, d_status)]
        _check(lib().myslam_backend_optimize_batch(self._h, *ptrs, int(batch), C.c_double(K[0]), C.c_double(K[1]), C.c_double(K[2]), C.c_double(K[3]),
                                                   C.c_double(delta), C.c_double(chi2_th), int(rounds), int(iters), *outs),
               "myslam_backend_optimize_batch")

    def solve_view(self):
        """(device pointer of the solve's positions by landmark slot, device pointer of the slot of every input map-point row): MapArchive.attach_solve"""
        pts, slot = C.c_void_p(), C.c_void_p()
        _check(lib().myslam_backend_solve_view(self._h, C.byref(pts), C.byref(slot)), "myslam_backend_solve_view")
        return pts.value, slot.value

    def culled_view(self):
        """(d_kf_id, d_tag, d_n_culled): device pointers of the list optimize_batch leaves of the features whose edge the solve removed
        (src/backend.cpp:236-247), per item in input row order, strided by obs_cap: LoopKeyFrameStore.clear_links_batch / Tracker.clear_links_batch"""
        kf, tag, n = C.c_void_p(), C.c_void_p(), C.c_void_p()
        _check(lib().myslam_backend_culled_view(self._h, C.byref(kf), C.byref(tag), C.byref(n)), "myslam_backend_culled_view")
        return kf.value, tag.value, n.value

    def insert_launches_per_call(self):
        return lib().myslam_backend_insert_launches_per_call(self._h)

    def insert_keyframe_batch(self, d_kf_id, d_kf_pose, d_n_kf, d_mp_id, d_mp_pos, d_mp_outlier, d_n_mp, d_obs_mp, d_obs_kf, d_obs_flags, d_obs_uv,
                              d_obs_tag, d_n_obs, d_new_kf_id, d_new_kf_pose, d_feat_mp_id, d_feat_mp_pos, d_feat_uv, d_feat_tag, d_feat_flags, d_n_feat,
                              feat_cap, d_prior_mp_id, d_prior_kf_id, d_prior_uv, d_prior_tag, d_prior_flags, d_n_prior, prior_cap, d_outlier_mp_id,
                              d_n_outlier_mp, outlier_cap, batch, window, min_dis_th, d_feat_row, d_mp_new_row, d_removed_kf_id, d_removed_kf_row, d_dis,
                              d_status):
        """Map::InsertKeyFrame (src/map.cpp:17-48, :78-140) per item on the tables of optimize_batch, all of them in/out, arguments in the header's
        order (include/myslam_hip.h); the optional prior / outlier inputs are None (or 0) when absent; window = Map.activeMap.size, min_dis_th = 0.2
        at the call site; one launch on the handle's stream; d_status batch i32 = 0 or a negative error"""
        vp = lambda p: C.c_void_p(p or None)
        tabs = [vp(p) for p in (d_kf_id, d_kf_pose, d_n_kf, d_mp_id, d_mp_pos, d_mp_outlier, d_n_mp, d_obs_mp, d_obs_kf, d_obs_flags, d_obs_uv, d_obs_tag,
                                d_n_obs, d_new_kf_id, d_new_kf_pose, d_feat_mp_id, d_feat_mp_pos, d_feat_uv, d_feat_tag, d_feat_flags, d_n_feat)]
        prior = [vp(p) for p in (d_prior_mp_id, d_prior_kf_id, d_prior_uv, d_prior_tag, d_prior_flags, d_n_prior)]
        outs = [vp(p) for p in (d_feat_row, d_mp_new_row, d_removed_kf_id, d_removed_kf_row, d_dis, d_status)]
        _check(lib().myslam_backend_insert_keyframe_batch(self._h, *tabs, int(feat_cap), *prior, int(prior_cap), vp(d_outlier_mp_id), vp(d_n_outlier_mp),
                                                          int(outlier_cap), int(batch), int(window), C.c_double(min_dis_th), *outs),
               "myslam_backend_insert_keyframe_batch")

    def debug_flat(self, item):
        """The flat window of one item as the last call built it, in ba_flatten_window's form (synchronises)"""
        ps = np.zeros(self.kf_cap, np.int32); pt = np.zeros(self.mp_cap, np.int32); fixed = np.zeros(self.mp_cap, np.uint8)
        ep = np.zeros(self.obs_cap, np.int32); el = np.zeros(self.obs_cap, np.int32); eo = np.zeros((self.obs_cap, 2)); es = np.zeros(self.obs_cap, np.int32)
        sz = np.zeros(3, np.int32)
        _check(lib().myslam_backend_debug_flat(self._h, int(item), _p(ps), _p(pt), _p(ep), _p(el), _p(eo), _p(es), _p(fixed), _p(sz)),
               "myslam_backend_debug_flat")
        P, L, E = (int(v) for v in sz)
        return dict(pose_src=ps[:P], pt_src=pt[:L], fixed=fixed[:L], edge_pose=ep[:E], edge_pt=el[:E], edge_obs=eo[:E], edge_src=es[:E])

    def debug_solved(self, item):
        """(poses, points, edge chi2, edge outlier flags, rounds, outlier count) the solve left for that flat window (synchronises)"""
        po = np.zeros((self.kf_cap, 7)); px = np.zeros((self.mp_cap, 3)); chi = np.zeros(self.obs_cap); out = np.zeros(self.obs_cap, np.uint8)
        sz = np.zeros(3, np.int32); ro = np.zeros(2, np.int32)
        _check(lib().myslam_backend_debug_flat(self._h, int(item), None, None, None, None, None, None, None, _p(sz)), "myslam_backend_debug_flat")
        _check(lib().myslam_backend_debug_solved(self._h, int(item), _p(po), _p(px), _p(chi), _p(out), _p(ro)), "myslam_backend_debug_solved")
        P, L, E = (int(v) for v in sz)
        return po[:P], px[:L], chi[:E], out[:E], int(ro[0]), int(ro[1])


MAP_AFTER_INSERT, MAP_AFTER_OPTIMIZE = 0, 1            # MYSLAM_MAP_AFTER_*
MAP_UPDATED, MAP_SKIPPED = 0, 1                        # MYSLAM_MAP_*
MAP_AFTER_RELINK = 2                                   # MYSLAM_MAP_AFTER_RELINK


class MapTables(C.Structure):                          # myslam_map_tables
    _fields_ = [(n, C.c_void_p) for n in ("kf_id", "kf_pose", "n_kf", "edge_v0", "edge_v1", "meas", "n_edges", "mp_id", "mp_pos", "mp_first_kf",
                                          "mp_state", "n_mp")] + \
               [(n, C.c_int32) for n in ("max_batch", "kf_cap", "edge_cap", "point_cap", "backend_mp_cap")]


class MapArchive:
    """Map::mmAllKeyFrames / mmAllMapPoints and KeyFrame::mpLastKF / mRelativePoseToLastKF of `max_batch` streams as device tables (myslam_map_*),
    kept up to date from the back end's active tables after every insert and optimise and laid out as LoopCorrector.correct_batch's tables.  The
    handle owns every buffer; `view()` gives the device pointers.  Batch calls take device pointers as ints, enqueue one launch on the handle's stream
    and return; `be` arguments are the back end's tables in the header's order."""

    def __init__(self, max_batch, kf_cap, edge_cap, point_cap, backend_mp_cap, stream=None):
        self.max_batch, self.kf_cap, self.edge_cap, self.point_cap, self.backend_mp_cap = (int(max_batch), int(kf_cap), int(edge_cap), int(point_cap),
                                                                                             int(backend_mp_cap))
        self._h = C.c_void_p()
        _check(lib().myslam_map_create(C.byref(self._h), self.max_batch, self.kf_cap, self.edge_cap, self.point_cap, self.backend_mp_cap),
               "myslam_map_create")
        if stream is not None:
            self.set_stream(stream)

    def __del__(self):
        if getattr(self, "_h", None) and self._h.value and _lib is not None:
            lib().myslam_map_destroy(self._h)
            self._h = C.c_void_p()

    def set_stream(self, stream):
        _check(lib().myslam_map_set_stream(self._h, C.c_void_p(stream)), "myslam_map_set_stream")

    def launches_per_update(self):
        return lib().myslam_map_launches_per_update(self._h)

    def attach_solve(self, d_solve_points, d_solve_mp_slot):
        """Backend.solve_view() of the back end whose tables the updates read: a point that leaves the active set with an optimise then takes the solve's
        position (None, None detaches)"""
        _check(lib().myslam_map_attach_solve(self._h, C.c_void_p(d_solve_points or None), C.c_void_p(d_solve_mp_slot or None)), "myslam_map_attach_solve")

    def view(self):
        """MapTables: the device pointers (ints or None) and caps of the per-item tables"""
        t = MapTables()
        _check(lib().myslam_map_view(self._h, C.byref(t)), "myslam_map_view")
        return t

    def load(self, item, kf_id, kf_pose, edge_v0, edge_v1, meas, mp_id, mp_pos, mp_first_kf, mp_state, snapshot=(), mp_gone_kf=None, mp_win_mask=None,
             win_kf=()):
        """one item from host arrays (synchronous); MyslamError(INVALID / CAPACITY) on what the header lists, the item then keeps every byte"""
        kf_id = np.ascontiguousarray(kf_id, np.int64); kf_pose = np.ascontiguousarray(kf_pose, np.float64).reshape(-1, 7)
        e0 = np.ascontiguousarray(edge_v0, np.int32); e1 = np.ascontiguousarray(edge_v1, np.int32); meas = np.ascontiguousarray(meas, np.float64).reshape(-1, 7)
        mp_id = np.ascontiguousarray(mp_id, np.int64); mp_pos = np.ascontiguousarray(mp_pos, np.float64).reshape(-1, 3)
        fk = np.ascontiguousarray(mp_first_kf, np.int32); st = np.ascontiguousarray(mp_state, np.uint8); snap = np.ascontiguousarray(snapshot, np.int32)
        gone = None if mp_gone_kf is None else np.ascontiguousarray(mp_gone_kf, np.int32)
        mask = None if mp_win_mask is None else np.ascontiguousarray(mp_win_mask, np.uint16)
        win = np.ascontiguousarray(win_kf, np.int32)
        assert len(kf_pose) == len(kf_id) and len(e1) == len(e0) == len(meas) and len(mp_pos) == len(mp_id) == len(fk) == len(st)
        assert (gone is None or len(gone) == len(mp_id)) and (mask is None or len(mask) == len(mp_id))
        _check(lib().myslam_map_load(self._h, int(item), _p(kf_id), _p(kf_pose), len(kf_id), _p(e0), _p(e1), _p(meas), len(e0), _p(mp_id), _p(mp_pos),
                                     _p(fk), _p(st), len(mp_id), _p(snap), len(snap), _p(gone), _p(mask), _p(win), len(win)), "myslam_map_load")

    def get(self, item):
        """one item's tables as a dict of numpy arrays cut to their counts (synchronises)"""
        K, E, P, M = self.kf_cap, self.edge_cap, self.point_cap, self.backend_mp_cap
        a = dict(kf_id=np.zeros(K, np.int64), kf_pose=np.zeros((K, 7)), edge_v0=np.zeros(E, np.int32), edge_v1=np.zeros(E, np.int32), meas=np.zeros((E, 7)),
                 mp_id=np.zeros(P, np.int64), mp_pos=np.zeros((P, 3)), mp_first_kf=np.zeros(P, np.int32), mp_state=np.zeros(P, np.uint8),
                 snapshot=np.zeros(M, np.int32), mp_gone_kf=np.zeros(P, np.int32), mp_win_mask=np.zeros(P, np.uint16),
                 win_kf=np.zeros(BA_MAX_WINDOW_POSES, np.int32))
        n = [C.c_int() for _ in range(5)]
        _check(lib().myslam_map_get(self._h, int(item), _p(a["kf_id"]), _p(a["kf_pose"]), C.byref(n[0]), _p(a["edge_v0"]), _p(a["edge_v1"]), _p(a["meas"]),
                                    C.byref(n[1]), _p(a["mp_id"]), _p(a["mp_pos"]), _p(a["mp_first_kf"]), _p(a["mp_state"]), C.byref(n[2]),
                                    _p(a["snapshot"]), C.byref(n[3]), _p(a["mp_gone_kf"]), _p(a["mp_win_mask"]), _p(a["win_kf"]), C.byref(n[4])),
               "myslam_map_get")
        nk, ne, nm, ns, nw = (v.value for v in n)
        cut = dict(kf_id=nk, kf_pose=nk, edge_v0=ne, edge_v1=ne, meas=ne, mp_id=nm, mp_pos=nm, mp_first_kf=nm, mp_state=nm, snapshot=ns, mp_gone_kf=nm,
                   mp_win_mask=nm, win_kf=nw)
        return {k: v[:cut[k]].copy() for k, v in a.items()}

    def update_batch(self, mode, d_kf_id, d_kf_pose, d_n_kf, be_kf_cap, d_mp_id, d_mp_pos, d_n_mp, be_mp_cap, d_obs_mp, d_obs_kf, d_obs_flags, d_n_obs,
                     be_obs_cap, d_backend_status, d_outlier_mp_id, d_n_outlier_mp, outlier_cap, d_mp_report, batch, d_status):
        """after each back-end call: mode MAP_AFTER_INSERT with insert_keyframe_batch's d_status and the turn's outlier ids (None / 0 = none), or
        MAP_AFTER_OPTIMIZE with optimize_batch's d_status and d_mp_report; d_status batch i32 = MAP_UPDATED / MAP_SKIPPED or a negative error"""
        vp = lambda p: C.c_void_p(p or None)
        _check(lib().myslam_map_update_batch(self._h, int(mode), vp(d_kf_id), vp(d_kf_pose), vp(d_n_kf), int(be_kf_cap), vp(d_mp_id), vp(d_mp_pos), vp(d_n_mp),
                                             int(be_mp_cap), vp(d_obs_mp), vp(d_obs_kf), vp(d_obs_flags), vp(d_n_obs), int(be_obs_cap), vp(d_backend_status),
                                             vp(d_outlier_mp_id), vp(d_n_outlier_mp), int(outlier_cap), vp(d_mp_report), int(batch), vp(d_status)),
               "myslam_map_update_batch")

    def loop_inputs_batch(self, d_kf_id, d_n_kf, be_kf_cap, d_mp_id, d_n_mp, be_mp_cap, d_obs_mp, d_obs_kf, d_obs_flags, d_n_obs, be_obs_cap, d_cur_kf_id,
                          d_loop_kf_id, d_detect_status, active_cap, batch, d_active, d_n_active, d_cur, d_loop, d_first_active, d_first_kf, d_n_points):
        """LoopCorrector.correct_batch's per-loop index inputs from the archive and the back end's tables"""
        vp = lambda p: C.c_void_p(p or None)
        _check(lib().myslam_map_loop_inputs_batch(self._h, vp(d_kf_id), vp(d_n_kf), int(be_kf_cap), vp(d_mp_id), vp(d_n_mp), int(be_mp_cap), vp(d_obs_mp),
                                                  vp(d_obs_kf), vp(d_obs_flags), vp(d_n_obs), int(be_obs_cap), vp(d_cur_kf_id), vp(d_loop_kf_id),
                                                  vp(d_detect_status), int(active_cap), int(batch), vp(d_active), vp(d_n_active), vp(d_cur), vp(d_loop),
                                                  vp(d_first_active), vp(d_first_kf), vp(d_n_points)), "myslam_map_loop_inputs_batch")

    def write_backend_batch(self, d_kf_id, d_kf_pose, d_n_kf, be_kf_cap, d_mp_id, d_mp_pos, d_n_mp, be_mp_cap, d_select, batch):
        """archive poses / positions into the back end's rows of the items with d_select != 0 (None / 0 = all)"""
        vp = lambda p: C.c_void_p(p or None)
        _check(lib().myslam_map_write_backend_batch(self._h, vp(d_kf_id), vp(d_kf_pose), vp(d_n_kf), int(be_kf_cap), vp(d_mp_id), vp(d_mp_pos), vp(d_n_mp),
                                                    int(be_mp_cap), vp(d_select), int(batch)), "myslam_map_write_backend_batch")

    def feature_slots_batch(self, d_feat_mp_id, d_n_feat, feat_cap, batch, d_feat_landmark):
        """map-point id -> archive slot per feature, -1 for none / absent / erased: LoopKeyFrameStore.put_batch's d_feat_landmark"""
        _check(lib().myslam_map_feature_slots_batch(self._h, C.c_void_p(d_feat_mp_id or None), C.c_void_p(d_n_feat or None), int(feat_cap), int(batch),
                                                    C.c_void_p(d_feat_landmark or None)), "myslam_map_feature_slots_batch")

    def filter_landmarks_batch(self, d_feat_landmark, feat_cap, batch, d_n_dropped=None):
        """LoopKeyFrameStore.detect_batch's d_loop_feat_landmark before loop_match_batch: every entry of the whole row that names an erased point
        (state 2) becomes -1 (src/map.cpp:166-175 as src/loopclosing.cpp:218-237 sees it); d_n_dropped batch i32 or None.  One launch, recordable."""
        _check(lib().myslam_map_filter_landmarks_batch(self._h, C.c_void_p(d_feat_landmark or None), int(feat_cap), int(batch),
                                                       C.c_void_p(d_n_dropped or None)), "myslam_map_filter_landmarks_batch")

    def relink_batch(self, d_merge, d_n_merge, merge_cap, d_plan_status, batch, d_status):
        """Relink.view()'s merge list (stride merge_cap = its out_cap) and Relink.plan_batch's d_status: every merged point is erased (state 2,
        src/loopclosing.cpp:527 with src/map.cpp:144-155); d_status batch i32 = MAP_UPDATED / MAP_SKIPPED / ERR_INVALID.  One launch, recordable."""
        vp = lambda p: C.c_void_p(p or None)
        _check(lib().myslam_map_relink_batch(self._h, vp(d_merge), vp(d_n_merge), int(merge_cap), vp(d_plan_status), int(batch), vp(d_status)),
               "myslam_map_relink_batch")


class ObsArchive:
    """MapPoint::GetObservations() of every map point of `max_batch` streams that is alive and not in the back end's table (myslam_obs_archive_*):
    the source of insert_keyframe_batch's prior rows.  `map_archive` is the MapArchive of the same streams (kept alive by this object), `be_obs_cap`
    the back end's obs_cap, `row_cap` the stored rows one item holds.  Order of a key-frame, one stream: prior_rows_batch -> insert ->
    MapArchive.update_batch -> update_batch -> optimise -> MapArchive.update_batch -> update_batch(d_obs_report).  Batch calls take device pointers
    as ints, enqueue one launch and return."""

    def __init__(self, map_archive, max_batch, be_obs_cap, row_cap, stream=None):
        self.map, self.max_batch, self.be_obs_cap, self.row_cap = map_archive, int(max_batch), int(be_obs_cap), int(row_cap)
        self.be_mp_cap = map_archive.backend_mp_cap
        self._h = C.c_void_p()
        _check(lib().myslam_obs_archive_create(C.byref(self._h), map_archive._h, self.max_batch, self.be_obs_cap, self.row_cap), "myslam_obs_archive_create")
        if stream is not None:
            self.set_stream(stream)

    def __del__(self):
        if getattr(self, "_h", None) and self._h.value and _lib is not None:
            lib().myslam_obs_archive_destroy(self._h)
            self._h = C.c_void_p()

    def set_stream(self, stream):
        _check(lib().myslam_obs_archive_set_stream(self._h, C.c_void_p(stream)), "myslam_obs_archive_set_stream")

    def launches_per_update(self):
        return lib().myslam_obs_archive_launches_per_update(self._h)

    def load(self, item, seg_mp_id, seg_count, row_kf_id, row_uv, row_tag, row_flags, table_mp_id=(), table_mp_rows=(), table_kf_id=(), table_uv=(),
             table_tag=(), table_flags=()):
        """one item from host arrays (synchronous): the live segments and the mirror of the back end's current table; clears the sticky error.
        MyslamError(INVALID / CAPACITY) on what the header lists, the item then keeps every byte"""
        a = [np.ascontiguousarray(seg_mp_id, np.int64), np.ascontiguousarray(seg_count, np.int32), np.ascontiguousarray(row_kf_id, np.int64),
             np.ascontiguousarray(row_uv, np.float32).reshape(-1, 2), np.ascontiguousarray(row_tag, np.int32), np.ascontiguousarray(row_flags, np.uint8),
             np.ascontiguousarray(table_mp_id, np.int64), np.ascontiguousarray(table_mp_rows, np.int32), np.ascontiguousarray(table_kf_id, np.int64),
             np.ascontiguousarray(table_uv, np.float32).reshape(-1, 2), np.ascontiguousarray(table_tag, np.int32), np.ascontiguousarray(table_flags, np.uint8)]
        assert len(a[0]) == len(a[1]) and len(a[2]) == len(a[3]) == len(a[4]) == len(a[5]) and len(a[6]) == len(a[7]) and len(a[8]) == len(a[9]) == len(a[10]) == len(a[11])
        _check(lib().myslam_obs_archive_load(self._h, int(item), _p(a[0]), _p(a[1]), len(a[0]), _p(a[2]), _p(a[3]), _p(a[4]), _p(a[5]), len(a[2]), _p(a[6]),
                                             _p(a[7]), len(a[6]), _p(a[8]), _p(a[9]), _p(a[10]), _p(a[11]), len(a[8])), "myslam_obs_archive_load")

    def get(self, item):
        """one item as a dict of numpy arrays cut to their counts (synchronises): the live segments in ascending id order (seg_mp_id, seg_count and the
        rows row_kf_id / row_uv / row_tag / row_flags), the mirror (table_*), rows_in_use, n_reclaims and the sticky error (0 = none)"""
        R, M, O = self.row_cap, self.be_mp_cap, self.be_obs_cap
        a = dict(seg_mp_id=np.zeros(R, np.int64), seg_count=np.zeros(R, np.int32), row_kf_id=np.zeros(R, np.int64), row_uv=np.zeros((R, 2), np.float32),
                 row_tag=np.zeros(R, np.int32), row_flags=np.zeros(R, np.uint8), table_mp_id=np.zeros(M, np.int64), table_mp_rows=np.zeros(M, np.int32),
                 table_kf_id=np.zeros(O, np.int64), table_uv=np.zeros((O, 2), np.float32), table_tag=np.zeros(O, np.int32), table_flags=np.zeros(O, np.uint8))
        n = [C.c_int() for _ in range(7)]
        _check(lib().myslam_obs_archive_get(self._h, int(item), _p(a["seg_mp_id"]), _p(a["seg_count"]), C.byref(n[0]), _p(a["row_kf_id"]), _p(a["row_uv"]),
                                            _p(a["row_tag"]), _p(a["row_flags"]), C.byref(n[1]), _p(a["table_mp_id"]), _p(a["table_mp_rows"]), C.byref(n[2]),
                                            _p(a["table_kf_id"]), _p(a["table_uv"]), _p(a["table_tag"]), _p(a["table_flags"]), C.byref(n[3]), C.byref(n[4]),
                                            C.byref(n[5]), C.byref(n[6])), "myslam_obs_archive_get")
        ns, nr, ntm, ntr = (v.value for v in n[:4])
        cut = dict(seg_mp_id=ns, seg_count=ns, row_kf_id=nr, row_uv=nr, row_tag=nr, row_flags=nr, table_mp_id=ntm, table_mp_rows=ntm, table_kf_id=ntr,
                   table_uv=ntr, table_tag=ntr, table_flags=ntr)
        out = {k: v[:cut[k]].copy() for k, v in a.items()}
        out.update(rows_in_use=n[4].value, n_reclaims=n[5].value, error=n[6].value)
        return out

    def update_batch(self, mode, d_kf_id, d_kf_pose, d_n_kf, d_mp_id, d_mp_pos, d_mp_outlier, d_n_mp, d_obs_mp, d_obs_kf, d_obs_flags, d_obs_uv, d_obs_tag,
                     d_n_obs, be_kf_cap, be_mp_cap, be_obs_cap, d_backend_status, d_map_status, d_obs_report, batch, d_status):
        """after each MapArchive.update_batch: the back end's thirteen tables as they stand (optimize_batch's order) and its caps, the back-end call's
        and the map update's d_status, and after an optimise its d_obs_report (None / 0 after an insert); d_status batch i32 = MAP_UPDATED /
        MAP_SKIPPED or a negative, sticky error"""
        vp = lambda p: C.c_void_p(p or None)
        _check(lib().myslam_obs_archive_update_batch(self._h, int(mode), vp(d_kf_id), vp(d_kf_pose), vp(d_n_kf), vp(d_mp_id), vp(d_mp_pos), vp(d_mp_outlier),
                                                     vp(d_n_mp), vp(d_obs_mp), vp(d_obs_kf), vp(d_obs_flags), vp(d_obs_uv), vp(d_obs_tag), vp(d_n_obs),
                                                     int(be_kf_cap), int(be_mp_cap), int(be_obs_cap), vp(d_backend_status), vp(d_map_status),
                                                     vp(d_obs_report), int(batch), vp(d_status)), "myslam_obs_archive_update_batch")

    def prior_rows_batch(self, d_feat_mp_id, d_n_feat, feat_cap, d_mp_id, d_n_mp, be_mp_cap, batch, d_prior_mp_id, d_prior_kf_id, d_prior_uv, d_prior_tag,
                         d_prior_flags, d_n_prior, prior_cap, d_status):
        """before the insert: the stored rows of every distinct stored point a feature names, ids ascending, in insert_keyframe_batch's prior arrays
        (batch x prior_cap); d_status batch i32 = 0, ERR_CAPACITY (more rows than prior_cap: n_prior 0) or the item's sticky error"""
        vp = lambda p: C.c_void_p(p or None)
        _check(lib().myslam_obs_archive_prior_rows_batch(self._h, vp(d_feat_mp_id), vp(d_n_feat), int(feat_cap), vp(d_mp_id), vp(d_n_mp), int(be_mp_cap),
                                                         int(batch), vp(d_prior_mp_id), vp(d_prior_kf_id), vp(d_prior_uv), vp(d_prior_tag), vp(d_prior_flags),
                                                         vp(d_n_prior), int(prior_cap), vp(d_status)), "myslam_obs_archive_prior_rows_batch")


MAPPER_IDLE, MAPPER_STATUS_WORDS = 3, 8                 # MYSLAM_MAPPER_*
MAPPER_STAGES = ("prior_rows", "insert", "map_after_insert", "obs_after_insert", "optimize", "map_after_optimize", "obs_after_optimize")
BE_TABLES = ("kf_id", "kf_pose", "n_kf", "mp_id", "mp_pos", "mp_outlier", "n_mp", "obs_mp", "obs_kf", "obs_flags", "obs_uv", "obs_tag", "n_obs")


class MapperTables(C.Structure):                       # myslam_mapper_tables
    _fields_ = [(n, C.c_void_p) for n in BE_TABLES + ("prior_mp_id", "prior_kf_id", "prior_uv", "prior_tag", "prior_flags", "n_prior", "feat_row",
                                                      "mp_new_row", "removed_kf_id", "removed_kf_row", "dis", "obs_report", "mp_report", "new_outlier_mp",
                                                      "n_new_outlier_mp", "obs_chi2", "rounds", "n_outlier_edges", "n_cleared", "gate", "fault")] + \
               [("stage_status", C.c_void_p * 7)] + [(n, C.c_void_p) for n in ("backend", "map", "obs")] + \
               [(n, C.c_int32) for n in ("streams", "kf_cap", "mp_cap", "obs_cap", "feat_cap", "prior_cap")]


class _Borrowed:
    """a handle the Mapper owns, seen through the class of its unit: same methods, never destroyed from here"""

    def __del__(self):
        pass


class Mapper:
    """The Backend thread's work for a bank of `streams` streams behind one handle (myslam_mapper_*): Backend::ProcessNewKeyFrame + OptimizeActiveMap
    (src/backend.cpp:82-121, :126-266) and Map::InsertKeyFrame (src/map.cpp:17-48) for exactly the streams that made a key-frame in the turn or
    StereoInit whose outputs the call is given; the decision is taken on the device.  The handle owns a Backend, a MapArchive (solve attached) and an
    ObsArchive (`.backend`, `.map`, `.obs`: borrowed views with their classes' methods), the back end's 13 tables and every array between the stages.
    keyframe_batch takes device pointers, enqueues launches_per_call() launches on the handle's stream and returns."""

    def __init__(self, streams, kf_cap, mp_cap, obs_cap, feat_cap, archive_kf_cap, archive_edge_cap, archive_point_cap, obs_row_cap, prior_cap, stream=None):
        self.streams = int(streams)
        self._h = C.c_void_p()
        _check(lib().myslam_mapper_create(C.byref(self._h), self.streams, int(kf_cap), int(mp_cap), int(obs_cap), int(feat_cap), int(archive_kf_cap),
                                          int(archive_edge_cap), int(archive_point_cap), int(obs_row_cap), int(prior_cap)), "myslam_mapper_create")
        if stream is not None:
            self.set_stream(stream)
        t = self.view()
        self.kf_cap, self.mp_cap, self.obs_cap, self.feat_cap, self.prior_cap = t.kf_cap, t.mp_cap, t.obs_cap, t.feat_cap, t.prior_cap

        def borrow(cls, handle, **attrs):
            o = object.__new__(type("Borrowed" + cls.__name__, (_Borrowed, cls), {}))
            o._h = C.c_void_p(handle)
            o.__dict__.update(attrs)
            return o
        self.backend = borrow(Backend, t.backend, max_batch=self.streams, kf_cap=t.kf_cap, mp_cap=t.mp_cap, obs_cap=t.obs_cap)
        self.map = borrow(MapArchive, t.map, max_batch=self.streams, kf_cap=int(archive_kf_cap), edge_cap=int(archive_edge_cap),
                          point_cap=int(archive_point_cap), backend_mp_cap=t.mp_cap)
        self.obs = borrow(ObsArchive, t.obs, map=self.map, max_batch=self.streams, be_obs_cap=t.obs_cap, row_cap=int(obs_row_cap), be_mp_cap=t.mp_cap)

    def __del__(self):
        if getattr(self, "_h", None) and self._h.value and _lib is not None:
            lib().myslam_mapper_destroy(self._h)
            self._h = C.c_void_p()

    def set_stream(self, stream):
        """the handle's stream, and that of the three owned handles"""
        _check(lib().myslam_mapper_set_stream(self._h, C.c_void_p(stream)), "myslam_mapper_set_stream")

    def launches_per_call(self, with_tracker=True):
        return lib().myslam_mapper_launches_per_call(self._h, int(bool(with_tracker)))

    def view(self):
        """MapperTables: the device pointers (ints or None), caps and owned handles"""
        t = MapperTables()
        _check(lib().myslam_mapper_view(self._h, C.byref(t)), "myslam_mapper_view")
        return t

    def keyframe_batch(self, trk, outs, window, K, d_status, min_dis_th=0.2, delta=5.991, chi2_th=5.991, rounds=5, iters=10):
        """outs: the dict of device pointers a turn or an init wrote (Tracker.TURN_OUTPUTS; StreamBank._turn_buffers builds it), trk the Tracker of the same
        streams or None, window = Map.activeMap.size, K = (fx, fy, cx, cy), d_status streams x MAPPER_STATUS_WORDS i32.  Asynchronous, recordable."""
        o = [C.c_void_p(outs.get(k) or None) for k in Tracker.TURN_OUTPUTS]
        _check(lib().myslam_mapper_keyframe_batch(self._h, trk._h if trk is not None else None, *o, int(window), C.c_double(min_dis_th), C.c_double(K[0]),
                                                  C.c_double(K[1]), C.c_double(K[2]), C.c_double(K[3]), C.c_double(delta), C.c_double(chi2_th), int(rounds),
                                                  int(iters), C.c_void_p(d_status or None)), "myslam_mapper_keyframe_batch")

    def status(self, d_status):
        """the status words of the last call as a (streams, MAPPER_STATUS_WORDS) array (synchronises): [:, 0] overall, [:, 1:] MAPPER_STAGES"""
        out = np.zeros((self.streams, MAPPER_STATUS_WORDS), np.int32)
        _check(lib().myslam_debug_peek(C.c_void_p(d_status), _p(out), out.nbytes), "myslam_debug_peek")
        return out

    def reset_item(self, s):
        """host call, synchronous: stream s's tables, map-archive item and observation-archive item empty, its sticky fault cleared"""
        _check(lib().myslam_mapper_reset_item(self._h, int(s)), "myslam_mapper_reset_item")

    def get(self, s):
        """stream s's whole map from the owned archive (synchronises): key-frame ids and poses, map-point ids, positions and states (0 alive, 1 listed
        as an outlier, 2 erased)"""
        a = self.map.get(s)
        return {k: a[k] for k in ("kf_id", "kf_pose", "mp_id", "mp_pos", "mp_state")}


RELINK_DONE, RELINK_SKIPPED, RELINK_REPORT_INTS = 0, 1, 6      # MYSLAM_RELINK_*


class RelinkLists(C.Structure):                        # myslam_relink_lists
    _fields_ = [(n, C.c_void_p) for n in ("merge", "n_merge", "adopt", "n_adopt", "target", "link_kf_id", "link_tag", "link_slot", "n_link", "report",
                                          "row_kf_id", "row_uv", "row_tag", "row_flags", "row_root_id", "row_slot", "row_place", "n_rows",
                                          "merge_from_id", "merge_root_id", "merge_rows", "merge_place", "n_staged_merges", "table_mp", "table_rows",
                                          "work_size")] + \
               [(n, C.c_int32) for n in ("max_batch", "out_cap", "feat_cap", "point_cap", "stage_cap")]


class Relink:
    """The plan of LoopLocalFusion's re-linking (src/loopclosing.cpp:509-532) for `max_batch` streams (myslam_relink_*): which point of the current
    key-frame is merged into which point of the loop key-frame, which feature adopts, where every archive slot's features end.  `map_archive` is
    the MapArchive of the same streams (kept alive by this object), `out_cap` the matcher's / verifier's cap, `feat_cap` the stride of the feature
    tables.  After plan_batch: MapArchive.relink_batch(view().merge ...), LoopKeyFrameStore.set_links_batch / Tracker.relink_batch with
    view().link_*.  Device pointers as ints; one launch per call."""

    def __init__(self, map_archive, max_batch, out_cap, feat_cap, stage_cap, stream=None):
        self.map, self.max_batch, self.out_cap, self.feat_cap, self.stage_cap = map_archive, int(max_batch), int(out_cap), int(feat_cap), int(stage_cap)
        self._h = C.c_void_p()
        _check(lib().myslam_relink_create(C.byref(self._h), map_archive._h, self.max_batch, self.out_cap, self.feat_cap, self.stage_cap),
               "myslam_relink_create")
        if stream is not None:
            self.set_stream(stream)

    def __del__(self):
        if getattr(self, "_h", None) and self._h.value and _lib is not None:
            lib().myslam_relink_destroy(self._h)
            self._h = C.c_void_p()

    def set_stream(self, stream):
        _check(lib().myslam_relink_set_stream(self._h, C.c_void_p(stream)), "myslam_relink_set_stream")

    def launches_per_plan(self):
        return lib().myslam_relink_launches_per_plan(self._h)

    def view(self):
        """device pointers (ints, None never) and caps of the plan's outputs: merge / adopt (max_batch x out_cap x 2 i32) with n_merge / n_adopt,
        target (max_batch x point_cap i32), link_kf_id / link_tag / link_slot (max_batch x feat_cap) with n_link, report (max_batch x 6 i32)"""
        v = RelinkLists()
        _check(lib().myslam_relink_view(self._h, C.byref(v)), "myslam_relink_view")
        return v

    def plan_batch(self, d_valid_pairs, d_counts, d_outlier, d_correct_status, d_cur_feat_landmark, d_loop_feat_landmark, d_cur_kf_id, batch, d_status):
        """loop_match_batch's pairs and counts, verify_batch's outlier flags, LoopCorrector.correct_batch's status, the current key-frame's feature ->
        slot table (batch x feat_cap i32, IN/OUT), the gathered loop table and the current mnKFId (batch i64) -> the handle's lists; d_status batch
        i32 = RELINK_DONE / RELINK_SKIPPED / ERR_INVALID"""
        vp = lambda p: C.c_void_p(p or None)
        _check(lib().myslam_loop_relink_plan_batch(self._h, vp(d_valid_pairs), vp(d_counts), vp(d_outlier), vp(d_correct_status), vp(d_cur_feat_landmark),
                                                   vp(d_loop_feat_landmark), vp(d_cur_kf_id), int(batch), vp(d_status)), "myslam_loop_relink_plan_batch")


    # ---- the rows (src/loopclosing.cpp:521-527): stage -> back end -> MapArchive.relink_batch -> MapArchive.update_batch(MAP_AFTER_RELINK) -> obs update ----
    def stage_batch(self, obs_archive, d_plan_status, batch, d_status):
        """GetObservations() of every merged point, read from `obs_archive` (nothing of it changes), into view().row_* with the place of every row in the
        list of the point it ends on; d_status batch i32 = RELINK_DONE / RELINK_SKIPPED / ERR_INVALID / ERR_CAPACITY (row_cap, the back end's obs_cap
        or stage_cap) or the archive's sticky error.  view().row_kf_id / row_tag / row_slot with n_rows are the link list of the moved rows."""
        vp = lambda p: C.c_void_p(p or None)
        _check(lib().myslam_relink_stage_batch(obs_archive._h if obs_archive else None, self._h, vp(d_plan_status), int(batch), vp(d_status)),
               "myslam_relink_stage_batch")

    def backend_batch(self, backend, d_kf_id, d_kf_pose, d_n_kf, d_mp_id, d_mp_pos, d_mp_outlier, d_n_mp, d_obs_mp, d_obs_kf, d_obs_flags, d_obs_uv, d_obs_tag,
                      d_n_obs, d_stage_status, batch, d_mp_new_row, d_status):
        """the back end's thirteen tables, in/out: merged points leave with their rows, a target in the table gets the staged rows at the end of its
        segment (ACTIVE 0); d_mp_new_row batch x mp_cap i32 by INPUT row; d_status batch i32 = 0, the stage's status when that is not 0,
        ERR_INVALID or ERR_CAPACITY (obs_cap) with every byte kept.  It is the one back-end call before the next updates."""
        vp = lambda p: C.c_void_p(p or None)
        _check(lib().myslam_relink_backend_batch(backend._h if backend else None, self._h, vp(d_kf_id), vp(d_kf_pose), vp(d_n_kf), vp(d_mp_id), vp(d_mp_pos),
                                                 vp(d_mp_outlier), vp(d_n_mp), vp(d_obs_mp), vp(d_obs_kf), vp(d_obs_flags), vp(d_obs_uv), vp(d_obs_tag), vp(d_n_obs),
                                                 vp(d_stage_status), int(batch), vp(d_mp_new_row), vp(d_status)), "myslam_relink_backend_batch")

    def obs_update_batch(self, obs_archive, d_kf_id, d_n_kf, d_mp_id, d_n_mp, d_obs_mp, d_obs_kf, d_obs_flags, d_obs_uv, d_obs_tag, d_n_obs, be_kf_cap, be_mp_cap,
                         be_obs_cap, d_backend_status, d_map_status, batch, d_status):
        """ObsArchive.update_batch's place after a re-link: the mirror follows the table, targets outside the table get the moved rows appended;
        d_status batch i32 = MAP_UPDATED / MAP_SKIPPED or a negative, sticky error"""
        vp = lambda p: C.c_void_p(p or None)
        _check(lib().myslam_relink_obs_update_batch(obs_archive._h if obs_archive else None, self._h, vp(d_kf_id), vp(d_n_kf), vp(d_mp_id), vp(d_n_mp), vp(d_obs_mp),
                                                    vp(d_obs_kf), vp(d_obs_flags), vp(d_obs_uv), vp(d_obs_tag), vp(d_n_obs), int(be_kf_cap), int(be_mp_cap),
                                                    int(be_obs_cap), vp(d_backend_status), vp(d_map_status), int(batch), vp(d_status)),
               "myslam_relink_obs_update_batch")

    @staticmethod
    def first_kf_batch(obs_archive, batch, d_first_kf):
        """LoopCorrector.correct_batch's d_first_kf (batch x point_cap i32) in LIST order: the archive row of the front observer, -1 without a row or
        for an erased point; what a stream that re-links passes instead of MapArchive.loop_inputs_batch's d_first_kf"""
        _check(lib().myslam_relink_first_kf_batch(obs_archive._h if obs_archive else None, int(batch), C.c_void_p(d_first_kf or None)),
               "myslam_relink_first_kf_batch")


LOOP_DETECT_CANDIDATE, LOOP_DETECT_NO_LOOP = 0, 1      # MYSLAM_LOOP_DETECT_*


class LoopKeyFrameStore:
    """What ProcessNewKF leaves in a KeyFrame, resident on the device (myslam_loop_store_*): `kf_capacity` slots of `cap` pyramid key-points and
    descriptors and `feat_cap` feature -> landmark entries, and LoopClosing::DetectLoop's decision (src/loopclosing.cpp:147, :151) over
    LoopDatabase.query_batch's outputs, written where loop_match_batch reads its loop side.  Device pointers as ints; every call enqueues on the
    handle's stream and returns."""

    def __init__(self, kf_capacity, cap, feat_cap, stream=None):
        self.cap, self.feat_cap = int(cap), int(feat_cap)
        self._h = C.c_void_p()
        _check(lib().myslam_loop_store_create(C.byref(self._h), int(kf_capacity), self.cap, self.feat_cap), "myslam_loop_store_create")
        if stream is not None:
            self.set_stream(stream)

    def __del__(self):
        if getattr(self, "_h", None) and self._h.value and _lib is not None:
            lib().myslam_loop_store_destroy(self._h)
            self._h = C.c_void_p()

    def set_stream(self, stream):
        _check(lib().myslam_loop_store_set_stream(self._h, C.c_void_p(stream)), "myslam_loop_store_set_stream")

    def __len__(self):
        return lib().myslam_loop_store_size(self._h)

    def capacity(self):
        return lib().myslam_loop_store_capacity(self._h)

    def put_batch(self, ids, d_pyr_kps, d_desc, d_counts, d_kf_status, d_feat_landmark, d_n_feat):
        """len(ids) key-frames as ORBextractor.process_keyframes_batch left them (d_kf_status 0 / None: every one is good) + their feature -> landmark
        tables (batch x feat_cap i32, -1 = no map point) and counts; ids strictly ascending and above every id held (MyslamError(INVALID)),
        MyslamError(CAPACITY) when they do not fit, MyslamError(UNSUPPORTED) on a capturing stream: nothing stored or enqueued then"""
        ids = np.ascontiguousarray(ids, np.uint64)
        _check(lib().myslam_loop_store_put_batch(self._h, _p(ids), len(ids), C.c_void_p(d_pyr_kps), C.c_void_p(d_desc), C.c_void_p(d_counts),
                                                 C.c_void_p(d_kf_status or None), C.c_void_p(d_feat_landmark), C.c_void_p(d_n_feat)),
               "myslam_loop_store_put_batch")

    def set_landmarks_batch(self, ids, d_feat_landmark, d_n_feat):
        """replaces the feature -> landmark table and count of key-frames already held (len(ids) x feat_cap i32); an unknown or repeated id: INVALID"""
        ids = np.ascontiguousarray(ids, np.uint64)
        _check(lib().myslam_loop_store_set_landmarks_batch(self._h, _p(ids), len(ids), C.c_void_p(d_feat_landmark), C.c_void_p(d_n_feat)),
               "myslam_loop_store_set_landmarks_batch")

    def clear_links_batch(self, d_kf_id, d_tag, d_n, list_cap, batch, d_pending_kf_id=None, d_pending_feat_landmark=None, d_n_cleared=None):
        """Backend.culled_view()'s lists (item b at + b * list_cap): the named feature of a key-frame held, or of the pending key-frame (its id per item
        and its batch x feat_cap table, in/out, both or neither), loses its landmark; ids not held and tags out of range are ignored.  d_n_cleared
        batch i32 or None.  One launch, no host bookkeeping: recordable (StepGraph)."""
        vp = lambda p: C.c_void_p(p or None)
        _check(lib().myslam_loop_store_clear_links_batch(self._h, vp(d_kf_id), vp(d_tag), vp(d_n), int(list_cap), int(batch), vp(d_pending_kf_id),
                                                         vp(d_pending_feat_landmark), vp(d_n_cleared)), "myslam_loop_store_clear_links_batch")

    def set_links_batch(self, d_kf_id, d_tag, d_slot, d_n, list_cap, batch, d_pending_kf_id=None, d_pending_feat_landmark=None, d_n_set=None):
        """clear_links_batch with a value per entry: Relink.view()'s link lists (item b at + b * list_cap); the named feature of a key-frame held, or
        of the pending key-frame, points at d_slot (>= -1) afterwards (src/loopclosing.cpp:524, :529).  d_n_set batch i32 or None.  One launch,
        recordable."""
        vp = lambda p: C.c_void_p(p or None)
        _check(lib().myslam_loop_store_set_links_batch(self._h, vp(d_kf_id), vp(d_tag), vp(d_slot), vp(d_n), int(list_cap), int(batch),
                                                       vp(d_pending_kf_id), vp(d_pending_feat_landmark), vp(d_n_set)), "myslam_loop_store_set_links_batch")

    def detect_batch(self, d_best_id, d_max_score, d_cnt, nq, d_loop_desc, d_n_loop, d_loop_pyr, d_loop_feat_landmark, d_loop_slot, d_status,
                     thr_high=0.94, max_suspected=3):
        """`max_score < thr_high or cnt > max_suspected` -> LOOP_DETECT_NO_LOOP, an id not held -> ERR_INVALID (both with n_loop 0, slot -1, nothing
        else written), else LOOP_DETECT_CANDIDATE with the key-frame's rows in loop_match_batch's d_loop_desc / d_n_loop / d_loop_pyr /
        d_loop_feat_landmark layout.  One launch, recordable (StepGraph)."""
        _check(lib().myslam_loop_detect_batch(self._h, C.c_void_p(d_best_id), C.c_void_p(d_max_score), C.c_void_p(d_cnt), int(nq), C.c_float(thr_high),
                                              int(max_suspected), C.c_void_p(d_loop_desc), C.c_void_p(d_n_loop), C.c_void_p(d_loop_pyr),
                                              C.c_void_p(d_loop_feat_landmark), C.c_void_p(d_loop_slot), C.c_void_p(d_status)),
               "myslam_loop_detect_batch")


LoopStore = LoopKeyFrameStore                          # the handle's name in the C ABI (myslam_loop_store)

LOOP_BANK_TURN, LOOP_BANK_SKIPPED, LOOP_BANK_IDLE, LOOP_BANK_CLOSED, LOOP_BANK_STORED = 0, 1, 2, 3, 4      # MYSLAM_LOOP_BANK_*


class LoopBankArrays(C.Structure):                     # myslam_loop_bank_arrays
    _fields_ = [(k, C.c_void_p) for k in ("kps", "desc", "feat_landmark", "rows", "n_feat", "ids", "n", "last_closed", "put_slot")] + \
               [(k, C.c_int32) for k in ("streams", "kfs_per_stream", "cap", "feat_cap")] + [("cap_stride", C.c_int64), ("feat_stride", C.c_int64)]


class LoopStoreBank:
    """S per-stream loop key-frame stores in device memory (myslam_loop_bank_*), item s = stream s, with LoopClosing::InsertNewKeyFrame's
    five-key-frames rule (src/loopclosing.cpp:671-681), DetectLoop's decision and lookup (:147, :151) by LoopDatabaseBank.query_batch's best row,
    `if(!bConfirmedLoopKF) AddToDatabase()` (:73-75) and _mpLastClosedKF (:331) on the device.  gate / detect / finish / set_links / clear take device
    pointers as ints, enqueue on the handle's stream and return (recordable, StepGraph); load / get / sizes are synchronous and take numpy arrays."""

    def __init__(self, streams, kfs_per_stream, cap, feat_cap, stream=None):
        self.streams, self.kfs_per_stream, self.cap, self.feat_cap = int(streams), int(kfs_per_stream), int(cap), int(feat_cap)
        self._h = C.c_void_p()
        _check(lib().myslam_loop_bank_create(C.byref(self._h), self.streams, self.kfs_per_stream, self.cap, self.feat_cap), "myslam_loop_bank_create")
        if stream is not None:
            self.set_stream(stream)

    def __del__(self):
        if getattr(self, "_h", None) and self._h.value and _lib is not None:
            _lib.myslam_loop_bank_destroy(self._h)
            self._h = C.c_void_p()

    def set_stream(self, stream):
        _check(lib().myslam_loop_bank_set_stream(self._h, C.c_void_p(stream)), "myslam_loop_bank_set_stream")

    @staticmethod
    def launches_per_finish():
        return lib().myslam_loop_bank_launches_per_finish()

    def gate_batch(self, d_new_kf_id, d_item_status, status_stride, d_active, d_status):
        """d_new_kf_id S i64 (-1: none), d_item_status None or Mapper's d_status with its stride -> d_active S i32 (LoopDatabaseBank.query_batch's),
        d_status S i32: LOOP_BANK_TURN / _SKIPPED (one of the five behind a closed loop) / _IDLE"""
        vp = lambda p: C.c_void_p(p or None)
        _check(lib().myslam_loop_bank_gate_batch(self._h, vp(d_new_kf_id), vp(d_item_status), int(status_stride), vp(d_active), vp(d_status)),
               "myslam_loop_bank_gate_batch")

    def detect_batch(self, d_best_id, d_best_row, d_max_score, d_cnt, d_loop_desc, d_n_loop, d_loop_pyr, d_loop_feat_landmark, d_loop_slot, d_status,
                     thr_high=0.94, max_suspected=3):
        """LoopKeyFrameStore.detect_batch per stream over LoopDatabaseBank.query_batch's four outputs; the key-frame is the one at d_best_row, which
        must carry d_best_id (else ERR_INVALID for that stream).  One launch."""
        vp = lambda p: C.c_void_p(p or None)
        _check(lib().myslam_loop_bank_detect_batch(self._h, vp(d_best_id), vp(d_best_row), vp(d_max_score), vp(d_cnt), C.c_float(thr_high),
                                                   int(max_suspected), vp(d_loop_desc), vp(d_n_loop), vp(d_loop_pyr), vp(d_loop_feat_landmark),
                                                   vp(d_loop_slot), vp(d_status)), "myslam_loop_bank_detect_batch")

    def finish_batch(self, d_cur_kf_id, d_active, d_verify_status, d_pyr_kps, d_desc, d_counts, d_kf_status, d_feat_landmark, d_n_feat, d_add, d_status):
        """per stream: idle / VERIFY_CONFIRMED -> LOOP_BANK_CLOSED (last_closed moves, nothing stored) / ERR_CAPACITY / ERR_INVALID (id not above the
        last one held) / LOOP_BANK_STORED (item s of LoopKeyFrameStore.put_batch's inputs goes into the stream's next slot).  d_add S i32 is
        LoopDatabaseBank.append_batch's.  Two launches."""
        vp = lambda p: C.c_void_p(p or None)
        _check(lib().myslam_loop_bank_finish_batch(self._h, vp(d_cur_kf_id), vp(d_active), vp(d_verify_status), vp(d_pyr_kps), vp(d_desc), vp(d_counts),
                                                   vp(d_kf_status), vp(d_feat_landmark), vp(d_n_feat), vp(d_add), vp(d_status)),
               "myslam_loop_bank_finish_batch")

    def set_links_batch(self, d_kf_id, d_tag, d_value, d_n, list_cap, d_pending_kf_id=None, d_pending_feat_landmark=None, d_n_set=None):
        """LoopKeyFrameStore.set_links_batch (d_value None: clear_links_batch) with item s walked against stream s's key-frames only.  One launch."""
        vp = lambda p: C.c_void_p(p or None)
        _check(lib().myslam_loop_bank_links_batch(self._h, vp(d_kf_id), vp(d_tag), vp(d_value), vp(d_n), int(list_cap), vp(d_pending_kf_id),
                                                      vp(d_pending_feat_landmark), vp(d_n_set)), "myslam_loop_bank_links_batch")

    def clear_batch(self, d_reset):
        """d_reset S i32: the streams with a non-zero entry hold nothing and have closed no loop afterwards"""
        _check(lib().myslam_loop_bank_clear_batch(self._h, C.c_void_p(d_reset or None)), "myslam_loop_bank_clear_batch")

    def view(self):
        """LoopBankArrays: the device pointers (ints) and shapes"""
        v = LoopBankArrays()
        _check(lib().myslam_loop_bank_view(self._h, C.byref(v)), "myslam_loop_bank_view")
        return v

    def read_view(self):
        """the whole allocation as numpy arrays, bytes behind the counts included: dict(kps [S, K, cap_st], desc [S, K, cap_st, 32], lm [S, K, feat_st],
        rows, nfeat, ids [S, K], n, last_closed, put_slot [S]); waits for nothing but its own copies"""
        v = self.view()
        S, K, cs, fs = v.streams, v.kfs_per_stream, v.cap_stride, v.feat_stride
        out = dict(kps=np.empty((S, K, cs), KP_DTYPE), desc=np.empty((S, K, cs, 32), np.uint8), lm=np.empty((S, K, fs), np.int32),
                   rows=np.empty((S, K), np.int32), nfeat=np.empty((S, K), np.int32), ids=np.empty((S, K), np.uint64), n=np.empty(S, np.int32),
                   last_closed=np.empty(S, np.int64), put_slot=np.empty(S, np.int32))
        ptr = dict(kps=v.kps, desc=v.desc, lm=v.feat_landmark, rows=v.rows, nfeat=v.n_feat, ids=v.ids, n=v.n, last_closed=v.last_closed, put_slot=v.put_slot)
        for k, a in out.items():
            _check(lib().myslam_debug_peek(C.c_void_p(ptr[k]), _p(a), a.nbytes), "myslam_debug_peek")
        return out

    def load(self, s, ids, kps, desc, rows, feat_landmark, n_feat, last_closed=-1):
        """replaces stream s (host arrays): ids [n] ascending, kps [n, cap] KP_DTYPE, desc [n, cap, 32] u8, rows [n], feat_landmark [n, feat_cap] i32,
        n_feat [n]; MyslamError(INVALID / CAPACITY) as the header says, the stream keeps every byte then"""
        ids = np.ascontiguousarray(ids, np.uint64)
        n = len(ids)
        if n == 0:                  # an empty stream: only the count and last_closed are written
            _check(lib().myslam_loop_bank_load(self._h, int(s), None, None, None, None, None, None, 0, int(last_closed)), "myslam_loop_bank_load")
            return
        kps = np.ascontiguousarray(kps, KP_DTYPE).reshape(n, self.cap); desc = np.ascontiguousarray(desc, np.uint8).reshape(n, self.cap, 32)
        lm = np.ascontiguousarray(feat_landmark, np.int32).reshape(n, self.feat_cap)
        rows = np.ascontiguousarray(rows, np.int32).reshape(n); n_feat = np.ascontiguousarray(n_feat, np.int32).reshape(n)
        a = [_p(x) if n else None for x in (ids, kps, desc, rows, lm, n_feat)]
        _check(lib().myslam_loop_bank_load(self._h, int(s), *a, n, int(last_closed)), "myslam_loop_bank_load")

    def get(self, s):
        """the whole of stream s: dict(ids [n], kps [n, cap], desc [n, cap, 32], rows [n], lm [n, feat_cap], nfeat [n], last_closed)"""
        K = self.kfs_per_stream
        ids = np.zeros(K, np.uint64); kps = np.zeros((K, self.cap), KP_DTYPE); desc = np.zeros((K, self.cap, 32), np.uint8)
        rows = np.zeros(K, np.int32); lm = np.zeros((K, self.feat_cap), np.int32); nf = np.zeros(K, np.int32)
        n, last = C.c_int(), C.c_int64()
        _check(lib().myslam_loop_bank_get(self._h, int(s), _p(ids), _p(kps), _p(desc), _p(rows), _p(lm), _p(nf), K, C.byref(n), C.byref(last)),
               "myslam_loop_bank_get")
        k = n.value
        return dict(ids=ids[:k].copy(), kps=kps[:k].copy(), desc=desc[:k].copy(), rows=rows[:k].copy(), lm=lm[:k].copy(), nfeat=nf[:k].copy(),
                    last_closed=last.value)

    def sizes(self):
        n = np.zeros(self.streams, np.int32)
        _check(lib().myslam_loop_bank_sizes(self._h, _p(n)), "myslam_loop_bank_sizes")
        return n


def loop_correct_structure(n_kf, active, loop, edge_v0, edge_v1):
    """The separator rule of LoopCorrector.correct_batch for one map, on the host -> (separators, chain length, supported)"""
    active = np.ascontiguousarray(active, np.int32); e0 = np.ascontiguousarray(edge_v0, np.int32); e1 = np.ascontiguousarray(edge_v1, np.int32)
    assert len(e0) == len(e1)
    ns = C.c_int(); nc = C.c_int(); ok = C.c_int()
    _check(lib().myslam_loop_correct_structure(int(n_kf), _p(active), len(active), int(loop), _p(e0), _p(e1), len(e0), C.byref(ns), C.byref(nc), C.byref(ok)),
           "myslam_loop_correct_structure")
    return ns.value, nc.value, bool(ok.value)


# ---------------------------------------------------------------------------------- host-side formats (no device needed)
def read_png_gray(path):
    """cv::imread(path, IMREAD_GRAYSCALE) for the KITTI grey PNGs (app/run_kitti_stereo.cpp:66-67) -> uint8 [rows, cols]"""
    r = C.c_int(); c = C.c_int(); b = path.encode()
    _check(lib().myslam_io_read_png_gray(b, None, 0, C.byref(r), C.byref(c)), "myslam_io_read_png_gray")
    out = np.zeros((r.value, c.value), np.uint8)
    _check(lib().myslam_io_read_png_gray(b, _p(out), out.size, C.byref(r), C.byref(c)), "myslam_io_read_png_gray")
    return out


def load_images(sequence_path):
    """LoadImages (app/run_kitti_stereo.cpp:114-144) -> (left paths, right paths, timestamps)"""
    n = C.c_int(); b = sequence_path.encode()
    _check(lib().myslam_io_load_images(b, None, 0, C.byref(n)), "myslam_io_load_images")
    ts = np.zeros(max(n.value, 1), np.float64)
    _check(lib().myslam_io_load_images(b, _p(ts), len(ts), C.byref(n)), "myslam_io_load_images")
    buf = C.create_string_buffer(len(b) + 64)

    def path(i, right):
        _check(lib().myslam_io_image_path(b, i, right, buf, len(buf)), "myslam_io_image_path")
        return buf.value.decode()
    return [path(i, 0) for i in range(n.value)], [path(i, 1) for i in range(n.value)], ts[:n.value]


def save_trajectory(path, ids, timestamps, poses7_cw):
    """System::SaveTrajectory (src/system.cpp:153-180); poses are Tcw (KeyFrame::Pose()) as qx qy qz qw tx ty tz"""
    ids = np.ascontiguousarray(ids, np.uint64); ts = np.ascontiguousarray(timestamps, np.float64); ps = np.ascontiguousarray(poses7_cw, np.float64).reshape(-1, 7)
    assert len(ids) == len(ts) == len(ps)
    _check(lib().myslam_io_save_trajectory(path.encode(), _p(ids), _p(ts), _p(ps), len(ids)), "myslam_io_save_trajectory")


def save_loop_edges(path, cur_ids, cur_ts, cur_poses, loop_ids, loop_ts, loop_poses):
    """System::SaveLoopEdges (src/system.cpp:188-224)"""
    a = [np.ascontiguousarray(cur_ids, np.uint64), np.ascontiguousarray(cur_ts, np.float64), np.ascontiguousarray(cur_poses, np.float64).reshape(-1, 7),
         np.ascontiguousarray(loop_ids, np.uint64), np.ascontiguousarray(loop_ts, np.float64), np.ascontiguousarray(loop_poses, np.float64).reshape(-1, 7)]
    _check(lib().myslam_io_save_loop_edges(path.encode(), *[_p(x) for x in a], len(a[0])), "myslam_io_save_loop_edges")
