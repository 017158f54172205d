"""The loop key-frame store bank (csrc/loop_bank.hip, api.LoopStoreBank) as plain Python: S objects over tests/loop_store_ref.py, each with its own
`last_closed`, and gate / detect / finish / set_links / clear written out — LoopClosing::InsertNewKeyFrame (src/loopclosing.cpp:671-681), DetectLoop's
decision and `_mvDatabase.at(bestId)` (:147, :151), `if(!bConfirmedLoopKF) AddToDatabase()` (:73-75, :651-659) and `_mpLastClosedKF = _mpCurrentKF`
(:331), plus the two rules of the device form (a fixed number of key-frames per stream, ids that ascend).  Nothing here looks at the device;
tests/test_loop_bank_ref.py pins it against a literal walk of the reference, tests/test_gpu_loop_bank.py holds the kernels to it."""
import numpy as np

import loop_store_ref as LS

TURN, SKIPPED, IDLE, CLOSED, STORED = 0, 1, 2, 3, 4                            # MYSLAM_LOOP_BANK_*
VERIFY_CONFIRMED, VERIFY_NO_MODEL, VERIFY_FEW_MATCHES, VERIFY_FEW_INLIERS = 0, 1, 2, 3      # MYSLAM_VERIFY_*
CANDIDATE, NO_LOOP = LS.CANDIDATE, LS.NO_LOOP
ERR_INVALID, ERR_CAPACITY = LS.ERR_INVALID, LS.ERR_CAPACITY
M64 = 1 << 64


def taken(kf_id, last_closed):
    """`_mpLastClosedKF == nullptr || pNewKF->mnKFId - _mpLastClosedKF->mnKFId > 5` with unsigned long ids (last_closed -1 = nullptr)"""
    return last_closed < 0 or (int(kf_id) - int(last_closed)) % M64 > 5


class Bank:
    def __init__(self, streams, kfs_per_stream, cap, feat_cap):
        self.S, self.K, self.cap, self.feat_cap = int(streams), int(kfs_per_stream), int(cap), int(feat_cap)
        self.stores = [LS.Store(self.K, self.cap, self.feat_cap) for _ in range(self.S)]
        self.last_closed = [-1] * self.S
        self.put_slot = [-1] * self.S

    def sizes(self):
        return [len(st) for st in self.stores]

    def ids(self, s):
        return list(self.stores[s].kfs)

    def load(self, s, ids, kps, desc, rows, lm, n_feat, last_closed=-1):
        st = LS.Store(self.K, self.cap, self.feat_cap)
        if len(ids):
            assert st.put(ids, np.asarray(kps), np.asarray(desc), rows, None, np.asarray(lm), n_feat) == LS.OK
        self.stores[s], self.last_closed[s] = st, int(last_closed)

    # ---- InsertNewKeyFrame --------------------------------------------------------------------------------------------------------------
    def gate(self, new_kf_id, item_status=None, status_stride=1):
        """-> (active [S], status [S]); item_status: a flat array read at s * status_stride, or None"""
        active, status = [], []
        for s in range(self.S):
            kf_id = int(new_kf_id[s])
            if kf_id < 0 or (item_status is not None and int(item_status[s * status_stride]) != 0):
                st = IDLE
            else:
                st = TURN if taken(kf_id, self.last_closed[s]) else SKIPPED
            active.append(1 if st == TURN else 0); status.append(st)
        return active, status

    # ---- DetectLoop's decision; the key-frame is the one at the row the scan found -------------------------------------------------------------
    def detect(self, best_id, best_row, max_score, cnt, thr_high, max_suspected, out):
        """out: loop_store_ref.sentinel_outputs(S, cap, feat_cap), changed in place (item s of every array)"""
        for s in range(self.S):
            item = {k: v[s:s + 1] for k, v in out.items()}                   # views: the store's detect writes item 0 of them
            ids = self.ids(s)
            row = int(best_row[s])
            if LS.no_loop(max_score[s], cnt[s], thr_high, max_suspected) or (0 <= row < len(ids) and ids[row] == int(best_id[s])):
                self.stores[s].detect([best_id[s]], [max_score[s]], [cnt[s]], thr_high, max_suspected, item)
            else:
                item["status"][0], item["n_loop"][0], item["slot"][0] = ERR_INVALID, 0, -1
        return out

    # ---- :73-75 with :331 and the store half of AddToDatabase -------------------------------------------------------------------------------------
    def finish(self, cur_id, active, verify_status, kps, desc, counts, kf_status, lm, n_feat):
        """-> (add [S], status [S]); arrays as loop_store_ref.Store.put takes them, item s = stream s"""
        add, status = [], []
        for s in range(self.S):
            st_, kf_id, slot = self.stores[s], int(cur_id[s]), -1
            if not active[s]:
                st = IDLE
            elif int(verify_status[s]) == VERIFY_CONFIRMED:
                self.last_closed[s] = kf_id                                    # the key-frame is NOT stored: `if(!bConfirmedLoopKF)`
                st = CLOSED
            elif len(st_) >= self.K:
                st = ERR_CAPACITY
            elif len(st_) and kf_id <= self.ids(s)[-1]:
                st = ERR_INVALID
            else:
                slot = len(st_)
                code = st_.put([kf_id], kps[s:s + 1], desc[s:s + 1], counts[s:s + 1], None if kf_status is None else kf_status[s:s + 1], lm[s:s + 1],
                               n_feat[s:s + 1])
                assert code == LS.OK
                st = STORED
            self.put_slot[s] = slot
            add.append(1 if slot >= 0 else 0); status.append(st)
        return add, status

    # ---- link upkeep per stream --------------------------------------------------------------------------------------------------------------------
    def set_links(self, lists, n=None, list_cap=None, pending_ids=None, pending=None):
        """lists[s]: [(kf id, tag, value)] (value -1: clear_links); n[s]: the device-side count, clamped to [0, list_cap], None = all; pending [S, feat_cap]
        in/out with pending_ids [S], both or neither.  -> hits [S]"""
        assert (pending_ids is None) == (pending is None)
        hits = []
        for s in range(self.S):
            entries = lists[s] if n is None else lists[s][:max(0, min(int(n[s]), int(list_cap)))]
            kfs, h = self.stores[s].kfs, 0
            for kf_id, tag, v in entries:
                if kf_id < 0 or tag < 0 or v < -1:
                    continue
                if pending is not None and kf_id == int(pending_ids[s]) and tag < self.feat_cap:
                    pending[s][tag] = v; h += 1
                elif kf_id in kfs and tag < len(kfs[kf_id]["lm"]):
                    kfs[kf_id]["lm"][tag] = v; h += 1
            hits.append(h)
        return hits

    def clear(self, flags):
        for s in range(self.S):
            if flags[s]:
                self.stores[s] = LS.Store(self.K, self.cap, self.feat_cap); self.last_closed[s] = -1
