"""numpy restatement of the loop key-frame store and of LoopClosing::DetectLoop's decision (include/myslam_hip.h, myslam_loop_store_* and
myslam_loop_detect_batch): a dict of id -> arrays, and detect() with the expression of src/loopclosing.cpp:147 written out and the rule that a
rejected item, and every slot from an accepted item's counts on, keeps the bytes it had.  Shares no code with the library.  Small seeded generators
of key-frame arrays live here too."""
import numpy as np

KP_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("size", "<f4"), ("angle", "<f4"), ("response", "<f4"), ("octave", "<i4"), ("class_id", "<i4")])
assert KP_DTYPE.itemsize == 28

CANDIDATE, NO_LOOP = 0, 1                   # MYSLAM_LOOP_DETECT_*
OK, ERR_INVALID, ERR_CAPACITY = 0, -1, -3


def no_loop(max_score, cnt, thr_high, max_suspected):
    """`if(maxScore < _similarityThres1 || cntSuspected > 3) return false;` — float against float, int against int.  NaN < x is false."""
    return bool(np.float32(max_score) < np.float32(thr_high)) or int(cnt) > int(max_suspected)


class Store:
    def __init__(self, kf_capacity, cap, feat_cap):
        self.kf_capacity, self.cap, self.feat_cap = kf_capacity, cap, feat_cap
        self.kfs = {}                       # id -> dict(kps, desc, lm); insertion order = slot order = ascending id

    def __len__(self):
        return len(self.kfs)

    def slot(self, kf_id):
        return list(self.kfs).index(kf_id)

    def _landmarks(self, lm, n_feat):
        return np.array(lm[:min(max(int(n_feat), 0), self.feat_cap)], np.int32)

    def put(self, ids, kps, desc, counts, kf_status, lm, n_feat):
        """kps [B, cap] KP_DTYPE, desc [B, cap, 32] u8, counts [B], kf_status [B] or None, lm [B, feat_cap] i32, n_feat [B] -> a call-level code"""
        ids = [int(i) for i in ids]
        last = max(self.kfs) if self.kfs else -1
        for i in ids:
            if i <= last:
                return ERR_INVALID
            last = i
        if len(self.kfs) + len(ids) > self.kf_capacity:
            return ERR_CAPACITY
        for b, i in enumerate(ids):
            n = min(max(int(counts[b]), 0), self.cap)
            if kf_status is not None and kf_status[b] != 0:
                n = 0
            self.kfs[i] = dict(kps=np.array(kps[b, :n]), desc=np.array(desc[b, :n]), lm=self._landmarks(lm[b], n_feat[b]))
        return OK

    def set_landmarks(self, ids, lm, n_feat):
        ids = [int(i) for i in ids]
        if any(i not in self.kfs for i in ids) or len(set(ids)) != len(ids):
            return ERR_INVALID
        for b, i in enumerate(ids):
            self.kfs[i]["lm"] = self._landmarks(lm[b], n_feat[b])
        return OK

    def detect(self, best_id, max_score, cnt, thr_high, max_suspected, out):
        """out: dict(desc [nq, cap, 32] u8, n_loop [nq], pyr [nq, cap] KP_DTYPE, lm [nq, feat_cap], slot [nq], status [nq]), changed in place"""
        for b in range(len(best_id)):
            if no_loop(max_score[b], cnt[b], thr_high, max_suspected):
                out["status"][b], out["n_loop"][b], out["slot"][b] = NO_LOOP, 0, -1
                continue
            kf = self.kfs.get(int(best_id[b]))
            if kf is None:
                out["status"][b], out["n_loop"][b], out["slot"][b] = ERR_INVALID, 0, -1
                continue
            n, nf = len(kf["kps"]), len(kf["lm"])
            out["status"][b], out["n_loop"][b], out["slot"][b] = CANDIDATE, n, self.slot(int(best_id[b]))
            out["pyr"][b, :n] = kf["kps"]; out["desc"][b, :n] = kf["desc"]; out["lm"][b, :nf] = kf["lm"]
        return out


def sentinel_outputs(nq, cap, feat_cap, byte=0xA5):
    """every output buffer of detect filled with one byte value"""
    i32 = np.frombuffer(bytes([byte]) * 4, np.int32)[0]
    return dict(desc=np.full((nq, cap, 32), byte, np.uint8), n_loop=np.full(nq, i32, np.int32),
                pyr=np.frombuffer(bytes([byte]) * (nq * cap * 28), KP_DTYPE).reshape(nq, cap).copy(), lm=np.full((nq, feat_cap), i32, np.int32),
                slot=np.full(nq, i32, np.int32), status=np.full(nq, i32, np.int32))


def random_keyframes(seed, batch, cap, feat_cap):
    """`batch` key-frames whose every byte is random, slots beyond any count included: kps [B, cap], desc [B, cap, 32], lm [B, feat_cap] in
    [-1, 1000)"""
    rng = np.random.default_rng(seed)
    kps = np.frombuffer(rng.integers(0, 256, batch * cap * 28, dtype=np.uint8).tobytes(), KP_DTYPE).reshape(batch, cap).copy()
    desc = rng.integers(0, 256, (batch, cap, 32), dtype=np.uint8)
    lm = rng.integers(-1, 1000, (batch, feat_cap)).astype(np.int32)
    return kps, desc, lm


def flip_bits(row, d, rng):
    out = row.copy()
    for p in rng.choice(256, d, replace=False):
        out[p >> 3] ^= 1 << (p & 7)
    return out


def matching_keyframe(seed, n_feat, levels, lm):
    """A loop key-frame and a current key-frame that see the same n_feat features, `levels` pyramid rows per feature: the loop rows (shuffled) lie
    0..11 bits from the feature's descriptor, the current rows 0..3.  -> (loop desc, loop class ids, current desc, current class ids); lm is
    returned with them for convenience"""
    rng = np.random.default_rng(seed)
    base = rng.integers(0, 256, (n_feat, 32), dtype=np.uint8)
    cls = np.repeat(np.arange(n_feat), levels)
    order = rng.permutation(len(cls))
    loop_desc = np.stack([flip_bits(base[f], int(rng.integers(0, 12)), rng) for f in cls[order]])
    cur_desc = np.stack([flip_bits(base[f], int(rng.integers(0, 4)), rng) for f in cls])
    return loop_desc, cls[order].astype(np.int32), cur_desc, cls.astype(np.int32), np.asarray(lm, np.int32)
