"""The Python restatement of LoopClosing::ProcessNewKF's expansion (src/loopclosing.cpp:94-105) that tests/test_gpu_process_kf.py feeds to the oracle:
feature pixels -> KP_DTYPE rows as chain.process_new_kf builds them -> np.repeat / np.tile over the levels.  Pinned here, byte for byte, against
api.expand_pyramid_keypoints (myslam_expand_pyramid_keypoints), a host function: no device is needed."""
import numpy as np

NLEVELS = 8


def feature_rows(KP_DTYPE, xy):
    """mvpFeaturesLeft[i]->mkpPosition of features that carry a pixel only: the fields chain.process_new_kf sets"""
    xy = np.asarray(xy, np.float32).reshape(-1, 2)
    feats = np.zeros(len(xy), KP_DTYPE)
    feats["x"], feats["y"] = xy[:, 0], xy[:, 1]
    feats["size"], feats["angle"], feats["octave"], feats["class_id"] = 7, -1, 0, -1
    return feats


def expand(KP_DTYPE, xy, nlevels=NLEVELS):
    """feature i, level l, in that order: octave = l, response = -1, class_id = i (:94-105)"""
    feats = feature_rows(KP_DTYPE, xy)
    pyr = np.repeat(feats, nlevels)
    pyr["octave"] = np.tile(np.arange(nlevels, dtype=np.int32), len(feats))
    pyr["response"] = -1
    pyr["class_id"] = np.repeat(np.arange(len(feats), dtype=np.int32), nlevels)
    return pyr


def reference(oracle, params, img, xy):
    """(mvPyramidKeyPoints, mORBDescriptors) of a key-frame: the oracle's ScreenAndComputeKPsParams and CalcDescriptors on the expansion"""
    from pyoracle import KP_DTYPE
    if len(xy) == 0:
        return np.zeros(0, KP_DTYPE), np.zeros((0, 32), np.uint8)              # :1085-1088: logs and returns
    kps = oracle.screen(params, img, expand(KP_DTYPE, xy, params.nlevels))
    return kps, oracle.calc_descriptors(params, img, kps)


def test_restatement_equals_the_host_function(pkg):
    api = pkg.api
    rng = np.random.default_rng(3)
    xy = rng.uniform(-50, 1300, (37, 2)).astype(np.float32)
    xy[5] = [np.nan, np.inf]; xy[6] = [-np.inf, 1e9]; xy[7] = [-0.0, 0.0]          # the host function copies bits, whatever they are
    for nlevels in (8, 1, 5):
        got = api.expand_pyramid_keypoints(feature_rows(api.KP_DTYPE, xy), nlevels)
        want = expand(api.KP_DTYPE, xy, nlevels)
        assert len(got) == 37 * nlevels and got.tobytes() == want.tobytes()
    assert api.expand_pyramid_keypoints(feature_rows(api.KP_DTYPE, np.zeros((0, 2))), 8).tobytes() == expand(api.KP_DTYPE, np.zeros((0, 2))).tobytes() == b""
