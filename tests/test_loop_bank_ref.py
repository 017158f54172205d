"""Pins tests/loop_bank_ref.py, the model the device bank is held to, against a literal walk of the reference's loop-closing thread as far as the
key-frame store goes: LoopClosingRun (src/loopclosing.cpp:51-80), `_mpLastClosedKF = _mpCurrentKF` (:331), AddToDatabase (:651-659) and
InsertNewKeyFrame (:671-681) — a std::map-like dict, a new-key-frame list and _mpLastClosedKF per stream.  The two rules the reference does not have
(a full stream, an id that does not ascend) are the device form's and are tested on their own.  CPU only."""
import numpy as np
import pytest

import loop_bank_ref as B
import loop_store_ref as LS

CAP, FEAT = 5, 6
M64 = 1 << 64


class LoopClosing:
    """the reference's members and statements, one stream"""

    def __init__(self, min_size):
        self.mvDatabase = {}                    # std::map<unsigned long, KeyFrame::Ptr>
        self.mlNewKeyFrames = []                # std::list<KeyFrame::Ptr>
        self.mpLastClosedKF = None
        self.mnDatabaseMinSize = min_size
        self.released = []                      # pNewKF->mImageLeft.release()

    def InsertNewKeyFrame(self, kf_id):         # :671-681
        if self.mpLastClosedKF is None or (kf_id - self.mpLastClosedKF) % M64 > 5:
            self.mlNewKeyFrames.append(kf_id)
        else:
            self.released.append(kf_id)

    def Run(self, chain_confirms, payload):     # the body of the while loop, :55-76
        if not self.mlNewKeyFrames:             # CheckNewKeyFrames
            return None
        cur = self.mlNewKeyFrames.pop(0)        # ProcessNewKF
        confirmed = False
        if len(self.mvDatabase) > self.mnDatabaseMinSize:
            if chain_confirms:                  # DetectLoop && MatchFeatures && ComputeCorrectPose
                self.mpLastClosedKF = cur       # :331, inside ComputeCorrectPose
                confirmed = True
        if not confirmed:
            self.mvDatabase[cur] = payload      # AddToDatabase, :655
        return confirmed


def _kf(rng, S):
    kps, desc, lm = LS.random_keyframes(int(rng.integers(1 << 30)), S, CAP, FEAT)
    return kps, desc, rng.integers(-1, CAP + 2, S).astype(np.int32), lm, rng.integers(-1, FEAT + 2, S).astype(np.int32)


def _same_store(bank, s, ref):
    st = bank.stores[s]
    assert list(st.kfs) == sorted(ref.mvDatabase) == list(ref.mvDatabase), s
    for kf_id, (kps, desc, n, lm, nf) in ref.mvDatabase.items():
        n, nf = min(max(int(n), 0), CAP), min(max(int(nf), 0), FEAT)
        got = st.kfs[kf_id]
        assert got["kps"].tobytes() == kps[:n].tobytes() and got["desc"].tobytes() == desc[:n].tobytes() and got["lm"].tolist() == lm[:nf].tolist()
    assert bank.last_closed[s] == (-1 if ref.mpLastClosedKF is None else ref.mpLastClosedKF), s


@pytest.mark.parametrize("seed", range(6))
def test_random_histories_equal_the_literal_walk(seed):
    """S streams, 60 turns: a key-frame (ids advance by 1 to 3) or none per stream, verify statuses drawn; the model's gate / finish against
    InsertNewKeyFrame / Run of S literal loop closers; after every turn the stores, their order and last_closed are equal"""
    rng = np.random.default_rng(seed)
    S, K, min_size = 4, 200, 2
    bank = B.Bank(S, K, CAP, FEAT)
    refs = [LoopClosing(min_size) for _ in range(S)]
    next_id = [int(rng.integers(0, 3)) for _ in range(S)]
    seen = set()
    for t in range(60):
        has = rng.random(S) < 0.85
        new_id = np.array([next_id[s] if has[s] else -1 for s in range(S)], np.int64)
        for s in range(S):
            if has[s]:
                next_id[s] += int(rng.integers(1, 4))
        item_status = rng.integers(0, 8, S * 3).astype(np.int32) * (rng.random(S * 3) < 0.1)       # a mapper fault now and then, stride 3
        active, gst = bank.gate(new_id, item_status, 3)
        kps, desc, counts, lm, nf = _kf(rng, S)
        draws = rng.random(S) < 0.2
        verify = []
        for s in range(S):
            cand = new_id[s] >= 0 and item_status[3 * s] == 0
            before = len(refs[s].mlNewKeyFrames)
            if cand:
                refs[s].InsertNewKeyFrame(int(new_id[s]))
            took = len(refs[s].mlNewKeyFrames) > before
            assert active[s] == int(took) and gst[s] == (B.IDLE if not cand else (B.TURN if took else B.SKIPPED)), (t, s)
            gated = len(refs[s].mvDatabase) <= min_size
            confirms = bool(draws[s]) and not gated
            verify.append(B.VERIFY_CONFIRMED if confirms else int(rng.integers(1, 4)))
            r = refs[s].Run(confirms, (kps[s], desc[s], counts[s], lm[s], nf[s]))
            assert (r is None) == (not took)
        add, fst = bank.finish(new_id.astype(np.uint64), active, verify, kps, desc, counts, None, lm, nf)
        for s in range(S):
            want = B.IDLE if not active[s] else (B.CLOSED if verify[s] == B.VERIFY_CONFIRMED else B.STORED)
            assert fst[s] == want and add[s] == int(want == B.STORED), (t, s)
            _same_store(bank, s, refs[s])
        seen |= set(gst) | set(fst)
    assert seen == {B.TURN, B.SKIPPED, B.IDLE, B.CLOSED, B.STORED}


def test_the_five_after_a_closed_key_frame():
    """last_closed = 100: ids 101 .. 105 (difference 1 .. 5) are neither processed nor stored, 106 (difference 6) is; the closed one is never stored;
    an id BELOW last_closed wraps and is taken, as the reference's unsigned expression does; no loop closed yet: everything is taken"""
    bank, ref = B.Bank(1, 32, CAP, FEAT), LoopClosing(0)
    rng = np.random.default_rng(1)
    for kf_id, verify in ((90, 1), (95, 2), (100, B.VERIFY_CONFIRMED), (101, 0), (102, 3), (103, 0), (104, 1), (105, 0), (106, 3), (107, 0), (99, 2), (108, 1),
                          (113, 1), (114, 2)):
        active, gst = bank.gate([kf_id])
        ref.InsertNewKeyFrame(kf_id)
        kf = _kf(rng, 1)
        r = ref.Run(verify == B.VERIFY_CONFIRMED, tuple(x[0] for x in kf))
        assert active == [int(r is not None)]
        if kf_id != 99:                          # (the device form refuses an id that does not ascend: below)
            bank.finish(np.array([kf_id], np.uint64), active, [verify], kf[0], kf[1], kf[2], None, kf[3], kf[4])
            _same_store(bank, 0, ref)
        else:
            assert active == [1] and gst == [B.TURN]
            del ref.mvDatabase[99]
    assert bank.ids(0) == [90, 95, 106, 113, 114] and bank.last_closed == [107]
    assert ref.released == [101, 102, 103, 104, 105, 108] and B.taken(106, 100) and not B.taken(105, 100) and B.taken(5, -1) and B.taken(0, 3)


@pytest.mark.parametrize("verify", [B.VERIFY_CONFIRMED, B.VERIFY_NO_MODEL, B.VERIFY_FEW_MATCHES, B.VERIFY_FEW_INLIERS, -1, -3])
def test_only_confirmed_closes(verify):
    bank = B.Bank(2, 4, CAP, FEAT)
    kf = _kf(np.random.default_rng(2), 2)
    add, st = bank.finish([7, 7], [1, 0], [verify, verify], kf[0], kf[1], kf[2], None, kf[3], kf[4])
    if verify == B.VERIFY_CONFIRMED:
        assert (add, st, bank.last_closed, bank.sizes(), bank.put_slot) == ([0, 0], [B.CLOSED, B.IDLE], [7, -1], [0, 0], [-1, -1])
    else:
        assert (add, st, bank.last_closed, bank.sizes(), bank.put_slot) == ([1, 0], [B.STORED, B.IDLE], [-1, -1], [1, 0], [0, -1])


def test_device_form_rules_full_stream_and_ids_that_do_not_ascend():
    """K = 3: the fourth key-frame is refused with ERR_CAPACITY (a full stream that is also given a low id: CAPACITY, as the loop database bank
    orders the two); an id equal to or below the last one held: ERR_INVALID; both keep the stream, add 0; a confirmed loop on a full stream still closes"""
    bank = B.Bank(3, 3, CAP, FEAT)
    rng = np.random.default_rng(3)
    for kf_id in (4, 9, 10):
        kf = _kf(rng, 3)
        assert bank.finish([kf_id, kf_id, 2 * kf_id], [1, 1, 0], [1, 2, 3], kf[0], kf[1], kf[2], [0, 5, 0], kf[3], kf[4])[0] == [1, 1, 0]
    assert len(bank.stores[1].kfs[10]["kps"]) == 0 and len(bank.stores[1].kfs[10]["lm"]) == min(max(int(kf[4][1]), 0), FEAT)      # kf_status != 0: no rows
    assert bank.sizes() == [3, 3, 0]
    bank.clear([0, 1, 0])
    kf = _kf(rng, 3)
    bank.finish([0, 30, 0], [0, 1, 0], [1, 1, 1], kf[0], kf[1], kf[2], None, kf[3], kf[4])
    before = [{k: {a: v.copy() for a, v in d.items()} for k, d in st.kfs.items()} for st in bank.stores]
    add, st = bank.finish([3, 30, 8], [1, 1, 1], [1, 1, 1], kf[0], kf[1], kf[2], None, kf[3], kf[4])
    assert (add, st, bank.put_slot) == ([0, 0, 1], [B.ERR_CAPACITY, B.ERR_INVALID, B.STORED], [-1, -1, 0])
    add, st = bank.finish([11, 29, 8], [1, 1, 1], [0, 3, 2], kf[0], kf[1], kf[2], None, kf[3], kf[4])
    assert (add, st) == ([0, 0, 0], [B.CLOSED, B.ERR_INVALID, B.ERR_INVALID]) and bank.last_closed == [11, -1, -1]
    for s in (0, 1):
        assert list(bank.stores[s].kfs) == list(before[s])
        for k, d in before[s].items():
            assert all(bank.stores[s].kfs[k][a].tobytes() == v.tobytes() for a, v in d.items())
    assert bank.sizes() == [3, 1, 1]


def test_detect_reads_the_row_the_scan_found():
    """the decision is loop_store_ref's; the key-frame is the one at best_row when it carries best_id, else ERR_INVALID — rows -1, n and K, and a row in
    range with another id; a rejected item keeps its bytes whatever the row says"""
    S, K = 6, 4
    bank = B.Bank(S, K, CAP, FEAT)
    rng = np.random.default_rng(4)
    for kf_id in (3, 8):
        kf = _kf(rng, S)
        bank.finish([kf_id] * S, [1] * S, [1] * S, kf[0], kf[1], [CAP, 2, 3, 4, 5, 1], None, kf[3], [FEAT] * S)
    out = LS.sentinel_outputs(S, CAP, FEAT)
    fresh = LS.sentinel_outputs(S, CAP, FEAT)
    bank.detect([8, 8, 8, 8, 3, 8], [1, -1, 2, K, 1, 7], [0.95, 0.95, 0.95, 0.95, 0.95, 0.5], [0] * S, np.float32(0.94), 3, out)
    assert out["status"].tolist() == [B.CANDIDATE, B.ERR_INVALID, B.ERR_INVALID, B.ERR_INVALID, B.ERR_INVALID, B.NO_LOOP]
    assert out["slot"].tolist() == [1, -1, -1, -1, -1, -1] and out["n_loop"].tolist() == [CAP, 0, 0, 0, 0, 0]
    for k in ("desc", "pyr", "lm"):
        assert out[k][1:].tobytes() == fresh[k][1:].tobytes() and out[k][0].tobytes() != fresh[k][0].tobytes()


def test_links_stay_inside_their_stream():
    """both streams hold key-frame 5; stream 0's list names it and stream 1's list is empty: only stream 0's table changes.  The store's cases per stream:
    a pending hit, a stored hit, an id not held, a tag beyond nfeat, a value below -1, and the value column left out (-1)"""
    bank = B.Bank(2, 4, CAP, FEAT)
    rng = np.random.default_rng(5)
    kf = _kf(rng, 2)
    lm = np.arange(2 * FEAT, dtype=np.int32).reshape(2, FEAT) + 100
    bank.finish([5, 5], [1, 1], [1, 1], kf[0], kf[1], kf[2], None, lm, [4, 4])
    pending = np.full((2, FEAT), 7, np.int32)
    hits = bank.set_links([[(9, 1, 41), (5, 0, 42), (6, 0, 43), (5, 4, 44), (5, 1, -2), (5, 3, -1), (-1, 0, 1), (5, -1, 1)], []], pending_ids=[9, 9], pending=pending)
    assert hits == [3, 0]
    assert bank.stores[0].kfs[5]["lm"].tolist() == [42, 101, 102, -1] and bank.stores[1].kfs[5]["lm"].tolist() == [106, 107, 108, 109]
    assert pending.tolist() == [[7, 41, 7, 7, 7, 7], [7] * FEAT]
    assert bank.set_links([[(5, 1, -1)] * 3, [(5, 2, -1)]], n=[2, -4], list_cap=2) == [2, 0]
    assert bank.stores[0].kfs[5]["lm"].tolist() == [42, -1, 102, -1] and bank.stores[1].kfs[5]["lm"].tolist() == [106, 107, 108, 109]


def test_clear_starts_a_stream_again():
    bank = B.Bank(2, 4, CAP, FEAT)
    kf = _kf(np.random.default_rng(6), 2)
    bank.finish([5, 5], [1, 1], [1, 0], kf[0], kf[1], kf[2], None, kf[3], kf[4])
    bank.finish([6, 6], [1, 0], [0, 0], kf[0], kf[1], kf[2], None, kf[3], kf[4])
    assert bank.last_closed == [6, 5] and bank.sizes() == [1, 0] and bank.gate([8, 8])[1] == [B.SKIPPED, B.SKIPPED]
    bank.clear([0, 1])
    assert bank.last_closed == [6, -1] and bank.gate([8, 0])[1] == [B.SKIPPED, B.TURN] and bank.gate([-1, 0], [0, 0, 0, 0, 0, 0, 0, 0, 0, 4], 9)[1] == [B.IDLE, B.IDLE]
