"""The numpy restatement of the loop key-frame store (tests/loop_store_ref.py) against the reference's own words: the decision of
src/loopclosing.cpp:147 over a table of edge values, and the rule that a rejected item keeps every byte it had.  CPU only."""
import numpy as np

import loop_store_ref as R

THR = np.float32(0.94)
BELOW = np.nextafter(THR, np.float32(0))


def test_rule_is_the_expression_of_the_reference():
    table = [(THR, 3), (THR, 4), (BELOW, 0), (BELOW, 3), (np.float32(1.0), 0), (np.float32(1.0), 3), (np.float32(1.0), 4), (np.float32(0.0), 0),
             (np.float32(np.nan), 0), (np.float32(np.nan), 3), (np.float32(np.nan), 4), (np.float32(np.inf), 3), (np.float32(-np.inf), 0),
             (np.nextafter(THR, np.float32(1)), 3), (THR, -1), (THR, 2 ** 31 - 1)]
    want = [False, True, True, True, False, False, True, True, False, False, True, False, True, False, False, True]
    for (score, cnt), w in zip(table, want):
        maxScore, _similarityThres1, cntSuspected = np.float32(score), THR, int(cnt)
        with np.errstate(invalid="ignore"):
            ref = bool(maxScore < _similarityThres1 or cntSuspected > 3)           # loopclosing.cpp:147, as written
        assert R.no_loop(score, cnt, THR, 3) == ref == w, (score, cnt)
    assert BELOW < THR and float(BELOW) != float(THR)
    # thr_high = +inf switches a step off for every finite score; a NaN score still passes the compare
    assert all(R.no_loop(s, 0, np.inf, 3) for s in (0.0, 0.94, 1.0, 3e38)) and not R.no_loop(np.nan, 0, np.inf, 3)


def _store(cap=9, feat_cap=5):
    st = R.Store(4, cap, feat_cap)
    kps, desc, lm = R.random_keyframes(1, 3, cap, feat_cap)
    assert st.put([5, 9, 12], kps, desc, [4, cap + 2, -1], None, lm, [feat_cap + 1, 2, -3]) == R.OK
    return st, kps, desc, lm


def test_put_clamps_and_orders():
    st, kps, desc, lm = _store()
    assert len(st) == 3 and [len(k["kps"]) for k in st.kfs.values()] == [4, 9, 0] and [len(k["lm"]) for k in st.kfs.values()] == [5, 2, 0]
    more = R.random_keyframes(2, 2, 9, 5)
    for bad in ([12], [3], [13, 13], [14, 13]):
        assert st.put(bad, *more[:2], [1, 1], None, more[2], [1, 1]) == R.ERR_INVALID and len(st) == 3
    assert st.put([13, 14], *more[:2], [1, 1], None, more[2], [1, 1]) == R.ERR_CAPACITY and len(st) == 3
    assert st.put([13], *more[:2], [3], [7], more[2], [1]) == R.OK and len(st.kfs[13]["kps"]) == 0 and len(st.kfs[13]["lm"]) == 1
    assert st.set_landmarks([9, 77], more[2], [1, 1]) == R.ERR_INVALID and st.set_landmarks([9, 9], more[2], [1, 1]) == R.ERR_INVALID
    assert len(st.kfs[9]["lm"]) == 2
    assert st.set_landmarks([9], more[2], [4]) == R.OK and st.kfs[9]["lm"].tolist() == more[2][0, :4].tolist()


def test_rejected_items_keep_every_byte_and_accepted_ones_every_slot_from_their_counts_on():
    st, kps, desc, lm = _store()
    best = np.array([9, 9, 9, 6, 5, 12], np.uint64)
    score = np.array([0.5, 0.99, np.nan, 0.99, THR, 1.0], np.float32)
    cnt = np.array([0, 4, 0, 0, 3, 0], np.int32)
    out = st.detect(best, score, cnt, THR, 3, R.sentinel_outputs(6, 9, 5))
    fresh = R.sentinel_outputs(6, 9, 5)
    assert out["status"].tolist() == [R.NO_LOOP, R.NO_LOOP, R.CANDIDATE, R.ERR_INVALID, R.CANDIDATE, R.CANDIDATE]
    assert out["n_loop"].tolist() == [0, 0, 9, 0, 4, 0] and out["slot"].tolist() == [-1, -1, 1, -1, 0, 2]
    for b in (0, 1, 3, 5):                       # NO_LOOP, unknown id, and a key-frame without rows: nothing but status, count and slot
        for k in ("desc", "pyr", "lm"):
            assert out[k][b].tobytes() == fresh[k][b].tobytes(), (b, k)
    assert out["pyr"][2].tobytes() == kps[1].tobytes() and out["desc"][2].tobytes() == desc[1].tobytes()
    assert out["lm"][2, :2].tolist() == lm[1, :2].tolist() and out["lm"][2, 2:].tobytes() == fresh["lm"][2, 2:].tobytes()
    assert out["pyr"][4, :4].tobytes() == kps[0, :4].tobytes() and out["pyr"][4, 4:].tobytes() == fresh["pyr"][4, 4:].tobytes()
    assert out["desc"][4, 4:].tobytes() == fresh["desc"][4, 4:].tobytes() and out["lm"][4].tolist() == lm[0].tolist()
