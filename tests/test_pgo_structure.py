"""tests/pgo_structure.py — the restatement of the pose graph's separator rule that the GPU tests use to assert which solver path a graph
takes — on hand-made graphs whose structure can be worked out on paper, and on the graph families of tests/test_gpu_pgo.py."""
import numpy as np

from pgo_structure import PG_MAXS, PG_MAXS_BIG, pg_structure


def _chain(n):
    return list(range(1, n)), list(range(0, n - 1))


def _skip2(n):
    """chain + an edge (i, i-2) for every i >= 2, key-frame 0 fixed"""
    a, b = _chain(n)
    fixed = np.zeros(n, np.uint8); fixed[0] = 1
    return n, fixed, np.array(a + list(range(2, n))), np.array(b + list(range(0, n - 2)))


def test_plain_chain_has_no_separator():
    e0, e1 = _chain(16)
    s = pg_structure(16, np.zeros(16, np.uint8), e0, e1)
    assert (s.natural, s.cuts, s.path, s.longest_run, s.n_chain) == (0, 0, "fast", 16, 16)
    # 50: lmax = max(16, ceil(sqrt(11 * 50))) = 24, three parts of 16 (two cuts)
    e0, e1 = _chain(50)
    s = pg_structure(50, np.zeros(50, np.uint8), e0, e1)
    assert (s.natural, s.cuts, s.path, s.longest_run, s.n_chain) == (0, 2, "fast", 16, 48)
    # in either orientation; a fixed key-frame splits the chain into runs of 20 and 29 (lmax 24: the second one cut once)
    fx = np.zeros(50, np.uint8); fx[20] = 1
    s = pg_structure(50, fx, e1, e0)
    assert (s.natural, s.cuts, s.longest_run, s.n_chain) == (0, 1, 20, 48)


def test_one_loop_is_one_separator():
    e0, e1 = _chain(20)
    s = pg_structure(20, np.zeros(20, np.uint8), e0 + [15], e1 + [3])
    assert (s.natural, s.cuts, s.path, s.longest_run, s.chosen) == (1, 0, "fast", 15, (15,))
    # a loop that only joins chain neighbours once the fixed key-frame between them is skipped is no loop
    fx = np.zeros(20, np.uint8); fx[6] = 1
    assert pg_structure(20, fx, e0 + [7], e1 + [5]).natural == 0


def test_ties_choose_the_later_key_frame():
    e0, e1 = _chain(10)
    assert pg_structure(10, np.zeros(10, np.uint8), e0 + [8], e1 + [2]).chosen == (8,)
    # degree first: key-frame 2 sits on two off-chain edges, 8 and 9 on one each
    assert pg_structure(10, np.zeros(10, np.uint8), e0 + [8, 9], e1 + [2, 2]).chosen == (2,)
    # after the first choice the remaining edge is a tie again: its later end
    s = pg_structure(12, np.zeros(12, np.uint8), _chain(12)[0] + [9, 6], _chain(12)[1] + [1, 3])
    assert s.chosen == (9, 6)


def test_long_runs_are_cut_and_lmax_doubles_when_the_cuts_do_not_fit():
    e0, e1 = _chain(1000)
    s = pg_structure(1000, np.zeros(1000, np.uint8), e0, e1)
    # lmax = ceil(sqrt(11 * 1000)) = 105: ceil(1001 / 106) = 10 parts, 9 cuts
    assert (s.natural, s.cuts, s.doublings, s.path) == (0, 9, 0, "fast")
    assert s.longest_run <= 105 and s.n_chain == 991
    # 95 natural separators leave room for one cut only: lmax doubles until a single cut remains
    n, fx, a, b = _skip2(286)
    base = pg_structure(n, fx, a, b)
    assert base.natural == 95 and base.path == "fast"
    assert base.doublings >= 1 and base.separators <= PG_MAXS


def test_the_families_of_the_gpu_tests(synth):
    """the issue's table: separators + cuts and the path of the skip-2 chain at its boundaries, and synth's 900 / 130 graph"""
    got = {}
    for n in (287, 289, 290, 3000, 3100):
        s = pg_structure(*_skip2(n))
        got[n] = (s.natural, s.cuts, s.path)
    assert got == {287: (96, 0, "fast"), 289: (96, 0, "fast"), 290: (97, 4, "general"), 3000: (999, 13, "general"),
                   3100: (PG_MAXS_BIG + 1, 0, "refused")}
    poses, fixed, e0, e1, meas, gt = synth.pose_graph(900, 130, seed=4)
    s = pg_structure(900, fixed, e0, e1)
    assert (s.natural, s.cuts, s.path) == (115, 1, "general")
