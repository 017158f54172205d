"""The second half of LoopClosing::LoopLocalFusion (reference src/loopclosing.cpp:509-532) on the object model of tests/whole_map_model.py.  Test helper,
no GPU.

RelinkMap is WholeMap (by import, nothing of it is edited) plus what the re-link needs of the key-frames' features: mpMapPoint of every feature.  A
feature that was made with a map point is one of that point's observations, and the model's Obs objects carry (key-frame id, tag), so such a feature's
point is the point whose GetObservations() holds its Obs: moving the Obs to another point (:521-525) IS pointing the feature at it, and an Obs that the
optimiser removed (src/backend.cpp:236-247) leaves the feature without a point.  A feature that ADOPTED a point (:529) is no observation of it; those
are kept in `adopted`, as the weak pointer the reference keeps: it is null once the point is gone from the map.

relink(valid_pairs, cur_kf, loop_kf) is <pkg>/chain.py's loop (chain.py:716-729, with its declared deviation: a point is not merged into itself) on
these objects.  It raises RowlessTarget on a merge into a point without a single observation, which src/loopclosing.cpp:623 asserts does not exist."""
import copy

import whole_map_model as wm


class RowlessTarget(Exception):
    pass


class RelinkMap(wm.WholeMap):
    _STATE = wm.WholeMap._STATE + ("adopted",)

    def __init__(self, chain, window, min_dis_th=0.2):
        super().__init__(chain, window, min_dis_th)
        self.adopted = {}                           # (mnKFId, tag) -> MapPoint, for features that took a point at :529

    def clone(self):
        c = RelinkMap(self.chain, self.window, self.min_dis_th)
        for k, v in zip(self._STATE, copy.deepcopy(tuple(getattr(self, k) for k in self._STATE))):
            setattr(c, k, v)
        return c

    def links(self, kf_id):
        """tag -> MapPoint for every feature of key-frame kf_id whose mpMapPoint.lock() is not null"""
        out = {}
        for mp in self.all_mps.values():
            for o in mp.obs:
                if int(o.kf) == kf_id:
                    out[o.tag] = mp
        for (k, tag), mp in self.adopted.items():
            if k == kf_id and self.all_mps.get(mp.id) is mp:
                assert tag not in out                                       # an observation is never adopted as well
                out[tag] = mp
        return out

    def link(self, kf_id, tag):
        return self.links(kf_id).get(tag)

    def remove_map_point(self, mp):
        """Map::RemoveMapPoint, src/map.cpp:144-155"""
        del self.all_mps[mp.id]
        self.active_mps.pop(mp.id, None)
        self.erased.add(mp.id)

    def relink(self, valid_pairs, cur_kf, loop_kf):
        """valid_pairs: [(tag of a feature of cur_kf, tag of a feature of loop_kf)] -> dict(merges: [(from id, to id)], adopts: [(tag, id)], same, moved:
        [(observer's mnKFId, tag, to id)] in move order)"""
        rep = dict(merges=[], adopts=[], same=0, null_loop=0, moved=[])
        for cf, lf in valid_pairs:
            loop_mp = self.link(loop_kf, lf)                                # :514
            if loop_mp is None:
                rep["null_loop"] += 1
                continue
            cur_mp = self.link(cur_kf, cf)                                  # :518
            if cur_mp is not None:
                if cur_mp is loop_mp:                                       # the declared deviation
                    rep["same"] += 1
                    continue
                if not loop_mp.obs:
                    raise RowlessTarget((cur_mp.id, loop_mp.id))
                for o in list(cur_mp.obs):                                  # :521-525: AddObservation only, the active list does not change
                    loop_mp.obs.append(o)
                    rep["moved"].append((int(o.kf), o.tag, loop_mp.id))
                cur_mp.obs, cur_mp.active_obs = [], []
                self.remove_map_point(cur_mp)                               # :527
                rep["merges"].append((cur_mp.id, loop_mp.id))
            else:
                self.adopted[(cur_kf, cf)] = loop_mp                        # :529
                rep["adopts"].append((cf, loop_mp.id))
        return rep
