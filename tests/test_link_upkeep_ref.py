"""The rules of tests/link_upkeep_ref.py (culled list, loop-store clear_links, archive filter, tracker clear_links) against the object model of
tests/whole_map_model.py over the seeded histories of tests/test_whole_map_model.py, with the oracle's solve; and the rules' own edges.  CPU only."""
import numpy as np
import pytest

import link_upkeep_ref as lu
import test_whole_map_model as T


@pytest.fixture(scope="module")
def counts(pkg, oracle):
    return {spec: lu.run_history(pkg, oracle, spec, T.K) for spec in T.HISTORIES}


@pytest.mark.parametrize("spec", T.HISTORIES, ids=lambda s: "seed%d_w%d" % s[:2])
def test_filtered_tables_equal_the_model_after_every_event(counts, spec):
    print(counts[spec])                                                     # run_history asserts after every event
    assert counts[spec]["links_surviving"] > 0


def test_every_constructed_case_occurs(counts):
    total = {k: sum(c[k] for c in counts.values()) for k in lu.CASES}
    print("link upkeep cases over %d histories:" % len(counts), total)
    assert all(total[k] > 0 for k in lu.CASES), total
    for half in (T.HISTORIES[:6], T.HISTORIES[6:]):                         # each batch of tests/test_gpu_link_upkeep.py on its own
        part = {k: sum(counts[s][k] for s in half) for k in lu.CASES}
        assert all(v > 0 for v in part.values()), part


def test_culled_list_is_in_row_order_by_key_frame_id():
    t = dict(kf_id=np.array([5, 9, 12]), obs_kf=np.array([0, 2, -1, 1, 2]), obs_tag=np.array([7, 3, 4, 0, 11]), obs_mp=np.zeros(5, np.int32))
    assert lu.culled_list(t, np.array([1, 0, 2, 1, 1])) == [(5, 7), (9, 0), (12, 11)]
    assert lu.culled_list(t, np.zeros(5)) == []


def test_clear_links_rule_edges():
    s = lu.Store(8)
    s.put(10, np.arange(8), 5)
    s.put(20, np.arange(8) + 100, 8)
    assert s.clear_links([]) == 0
    assert s.clear_links([(10, 4), (10, 5), (10, -1), (-3, 1), (15, 0), (20, 7), (20, 8)]) == 2       # tag = count - 1 / = count / negative; ids not held
    assert s.gather(10, fill=-7).tolist() == [0, 1, 2, 3, -1, -7, -7, -7] and s.gather(20).tolist() == [100, 101, 102, 103, 104, 105, 106, -1]
    assert s.clear_links([(10, 0), (10, 0), (10, 0)]) == 3 and s.gather(10)[0] == -1                   # entries, not distinct features
    assert s.clear_links([(10, 1), (10, 2)], n=-4, list_cap=2) == 0 and s.clear_links([(10, 1), (10, 2)], n=9, list_cap=1) == 1
    assert s.gather(10).tolist()[:4] == [-1, -1, 2, 3]
    pend = np.arange(8, dtype=np.int32)
    assert s.clear_links([(30, 2), (30, 8), (10, 2), (20, 0)], pending_id=30, pending=pend) == 3       # tag = feat_cap: not the pending table's, and 30 is not held
    assert pend.tolist() == [0, 1, -1, 3, 4, 5, 6, 7] and s.gather(10)[2] == -1 and s.gather(20)[0] == -1
    pend20 = np.arange(8, dtype=np.int32)
    assert s.clear_links([(20, 1)], pending_id=20, pending=pend20) == 1 and pend20[1] == -1 and s.gather(20)[1] == 101   # the pending table comes first
    s.put(30, pend, 8)                                                      # a key-frame put afterwards is what its table said
    assert s.gather(30).tolist() == [0, 1, -1, 3, 4, 5, 6, 7]
    with pytest.raises(AssertionError):
        s.clear_links([], pending_id=1)


def test_filter_rule_edges():
    state = np.array([0, 1, 2, 2, 0], np.uint8)
    row = np.array([-1, 0, 1, 2, 3, 4, 5, 9, -2 ** 31], np.int32)
    out, n = lu.filter_landmarks(row, state)
    assert out.tolist() == [-1, 0, 1, -1, -1, 4, 5, 9, -2 ** 31] and n == 2
    assert lu.filter_landmarks(row, state[:2])[1] == 0                       # n_mp bounds the states that are read


def test_tracker_rule_edges():
    base = dict(ids_valid=1, ref_frame_id=6, next_frame_id=7, ref_kf_id=40, lm=np.array([0, 1, -1, 2], np.int32))
    fresh = lambda **kw: dict(base, lm=base["lm"].copy(), **kw)
    t = fresh()
    assert lu.tracker_clear_links(t, [(40, 1), (41, 0), (40, 4), (40, -1), (40, 2)]) == 2 and t["lm"].tolist() == [0, -1, -1, 2]
    for other in (fresh(ids_valid=0), fresh(next_frame_id=8), fresh(ref_kf_id=39)):
        assert lu.tracker_clear_links(other, [(40, 1)]) == 0 and other["lm"].tolist() == [0, 1, -1, 2]
