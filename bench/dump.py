"""bench/dump.py — `bench.py --dump-outputs DIR`: what the last timed step computed, as DIR/<name>.npy in float32 / float64, so that two builds run with
the same arguments (identical inputs: every input of the step is generated from fixed seeds) can be compared output for output.

The per-frame outputs are written for a fixed, seeded sample of the batch's frames (the whole batch would be ~0.4 GB at 512 pairs per step); the loop-database
answers and the DeepLCD descriptors are small and written whole.  Slots past an image's key-point count are never written by the step and hold stale bytes:
they are zeroed here, and `orb_count` says how many slots of each image are valid."""
import os

import numpy as np

KP_FIELDS = ("x", "y", "size", "angle", "response", "octave", "class_id")
BA_NAMES = ("ba_Hpp", "ba_Hll", "ba_Hpl", "ba_bp", "ba_bl", "ba_chi2")
MAX_BYTES = 64 << 20
SAMPLE_SEED = 0xD0       # the frames written: the same for every run with the same --pairs
SAMPLE_FRAMES = 16


def sample_frames(P):
    """The sorted indices of the frames whose per-frame outputs are written."""
    rng = np.random.default_rng(SAMPLE_SEED)
    return np.sort(rng.choice(P, size=min(P, SAMPLE_FRAMES), replace=False))


def _valid(a, counts):
    """a: [images, cap, ...]; zero every slot at or past the image's count."""
    a = a.copy()
    for i, n in enumerate(counts):
        a[i, int(n):] = 0
    return a


def write(path, P, cap, kps, desc, cnt, midx, mdist, xyz, ok, lcd=None, ba=None):
    """Host arrays of the last timed step, already cut to the sample (sample_frames(P)): kps [n, 2, cap] of api.KP_DTYPE (left, right image of each frame),
    desc [n, 2, cap, 32] u8, cnt [n, 2], midx / mdist / ok [n, cap], xyz [n, cap, 3]; lcd = (descriptors [P, 1064], best ids, max scores, counts) of
    the whole batch or None; ba = the six block-build outputs [n, ...] or None.  Returns the names written."""
    n_l = cnt[:, 0]
    out = {
        "sample_frames": sample_frames(P).astype(np.float64),
        "orb_count": cnt.astype(np.float64),
        "orb_keypoints": np.stack([_valid(np.stack([kps[:, s][f].astype(np.float32) for f in KP_FIELDS], -1), cnt[:, s]) for s in range(2)], 1),
        "orb_descriptors": np.stack([_valid(desc[:, s].astype(np.float32), cnt[:, s]) for s in range(2)], 1),
        "match_index": _valid(midx.astype(np.float64), n_l),
        "match_distance": _valid(mdist.astype(np.float64), n_l),
        "triangulated_xyz": _valid(xyz.astype(np.float64), n_l),
        "triangulated_ok": _valid(ok.astype(np.float32), n_l),
    }
    if lcd is not None:
        descr, best, mx, dbcnt = lcd
        out.update({"lcd_descriptor": descr.astype(np.float32), "db_best_id": best.astype(np.float64), "db_max_score": mx.astype(np.float32),
                    "db_count": dbcnt.astype(np.float64)})
    if ba is not None:
        out.update({name: a.astype(np.float64) for name, a in zip(BA_NAMES, ba)})
    total = sum(a.nbytes for a in out.values())
    assert total <= MAX_BYTES, f"--dump-outputs: {total} bytes, more than {MAX_BYTES}"
    os.makedirs(path, exist_ok=True)
    for name, a in out.items():
        np.save(os.path.join(path, name + ".npy"), np.ascontiguousarray(a))
    return sorted(out)
