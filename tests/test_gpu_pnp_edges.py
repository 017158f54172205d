"""PnP-RANSAC on bad matches and parameter extremes: non-finite matches, matches behind the camera, duplicates, degenerate
point sets, confidence 0 and 1, reproj_error 0 and 1e6, one iteration, 5 and 6 points, and one item that fills the handle's 4096 slots.  The kernels
handle all of it by the fall-through of comparisons; the oracle gives a definite answer for every input (tests/pose_cases.pnp_edges says which, and
every test asserts that about the ORACLE first, so that a case cannot quietly stop testing what its name says).

Rules: status, count and mask of the one-item call are the oracle's.  The same item inside a batch among ordinary items: its status, count and mask
are the oracle's again, and the ordinary items carry the bits they have in the batch without it.  Pose: items with at least 20 inliers at the default
threshold are held at 1e-9 against the oracle; the others (few inliers, reproj_error 1e6) at 1e-9 against the library's other entry point and by cost
against the oracle (test_gpu_pose_moved.weak_pose_rule: relative 1e-6)."""
import numpy as np
import pytest

import pose_cases as PC
from test_gpu_pnp_batch import SENTINEL, _Bufs, _pack
from test_gpu_pose_moved import check_neighbours, weak_pose_rule

pytestmark = pytest.mark.gpu

CAP = 200


@pytest.fixture(scope="module")
def edges(synth):
    return PC.pnp_edges(synth)


@pytest.fixture(scope="module")
def ordinary(synth):
    """the items an odd one sits among: slots 0, 2 and 3 of every batch"""
    return [PC.pnp_problem(synth, k)[:2] for k in ("b", "a", "d")]


def _one_item(api, c, Kt):
    try:
        return api.solve_pnp_ransac(c["pw"], c["uv"], Kt, **c["kw"])
    except api.MyslamError as e:
        assert e.code == api.ERR_UNSUPPORTED
        return None


def _batch(api, solver, items, Kt, kw, cap=CAP):
    bufs = _Bufs(len(items), cap); bufs.K = Kt
    bufs.load(*_pack(items, cap))
    bufs.solve(solver, **kw)
    r = bufs.results()
    return [(r["pose"][b], r["flag"][b], r["ninl"][b], r["st"][b]) for b in range(len(items))]


def _judge(api, name, c, Kt, ref, one, inb):
    """one odd item: the one-item call `one` and its row `inb` of a batch against the oracle's `ref`"""
    rc, rp, rin, rn = ref
    n = len(c["pw"])
    pose, flag, ninl, st = inb
    assert not flag[n:].any(), name
    if rc != 0:
        assert one is None, (name, "the oracle finds no model, the one-item call does")
        assert st == 1 and ninl == 0 and not flag.any() and np.array_equal(pose, SENTINEL), (name, "batch row of an item without a model")
        return None
    assert one is not None, (name, "the oracle finds a model, the one-item call none")
    gp, gin, gn = one
    assert gn == rn and np.array_equal(gin, rin), (name, "one-item call: mask / count", gn, rn)
    assert st == 0 and ninl == rn and np.array_equal(flag[:n].astype(bool), rin), (name, "batch: mask / count", int(ninl), rn)
    if rn >= 20 and "reproj_error" not in c["kw"]:
        assert PC.pose_dist(gp, rp) < 1e-9 and PC.pose_dist(pose, rp) < 1e-9, (name, gp, pose, rp)
        return None
    return weak_pose_rule(c["pw"], c["uv"], Kt, pose, gp, ref, name)


@pytest.mark.parametrize("name", ["nonfinite", "mirrored", "doubled", "one_point_x30", "collinear40", "confidence0", "confidence1", "reproj0", "reproj1e6",
                                  "iterations1", "n5_inliers", "n6_inliers"])
def test_pnp_odd_item(api, oracle, edges, ordinary, name):
    E, Kt = edges
    c = E[name]
    ref = oracle.solve_pnp_ransac(c["pw"], c["uv"], Kt, **c["kw"])
    PC.expect_holds(ref, c, name)
    one = _one_item(api, c, Kt)
    solver = api.PnPSolver(4, CAP, 100)
    odd = (c["pw"], c["uv"])
    empty = (c["pw"][:0], c["uv"][:0])
    with_odd = _batch(api, solver, [ordinary[0], odd, ordinary[1], ordinary[2]], Kt, c["kw"])
    without = _batch(api, solver, [ordinary[0], empty, ordinary[1], ordinary[2]], Kt, c["kw"])
    check_neighbours(with_odd, without, 1, name)
    _judge(api, name, c, Kt, ref, one, with_odd[1])
    for b, item in zip((0, 2, 3), ordinary):                          # the ordinary items are themselves the oracle's under these parameters
        r = oracle.solve_pnp_ransac(item[0], item[1], Kt, **c["kw"])
        pose, flag, ninl, st = with_odd[b]
        assert (st == 0) == (r[0] == 0) and ninl == r[3] and np.array_equal(flag[:len(item[0])].astype(bool), r[2]), (name, "ordinary item", b)


def test_pnp_item_at_the_handles_limit(api, oracle, synth, ordinary):
    """one item of n = cap = 4096 between two ordinary ones"""
    pw, uv, Kt, _, _ = synth.pnp_problem(*PC.PNP_CAP_ITEM)
    assert len(pw) == 4096
    c = dict(pw=pw, uv=uv, kw={})
    ref = oracle.solve_pnp_ransac(pw, uv, Kt)
    assert ref[0] == 0 and ref[3] >= 2000
    solver = api.PnPSolver(3, 4096, 100)
    with_odd = _batch(api, solver, [ordinary[0], (pw, uv), ordinary[1]], Kt, {}, cap=4096)
    without = _batch(api, solver, [ordinary[0], (pw[:0], uv[:0]), ordinary[1]], Kt, {}, cap=4096)
    check_neighbours(with_odd, without, 1, "n = cap = 4096")
    _judge(api, "n = cap = 4096", c, Kt, ref, _one_item(api, c, Kt), with_odd[1])
    with pytest.raises(api.MyslamError) as e:
        api.PnPSolver(1, 4097, 100)
    assert e.value.code == api.ERR_CAPACITY
