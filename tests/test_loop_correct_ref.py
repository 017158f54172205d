"""The items the GPU tests of myslam_loop_correct_batch run (tests/loop_correct_ref.py), pinned on the CPU with the oracle: the need-correct gate of
every item sits at least 10 % away from the threshold, so no rounding can flip it; myslam_loop_correct_structure (the device's separator rule,
compiled for the host) puts each named case in the regime its name says; the reference composition closes the loop of every needed item."""
import numpy as np
import pytest

import loop_correct_ref as R


@pytest.fixture(scope="module")
def items(synth, oracle):
    out = {("needed", n): R.build_item(synth, oracle, n, loops, seed) for n, loops, seed in ((60, 1, 1), (120, 2, 2), (200, 3, 3), (30, 1, 4))}
    out[("small", 60)] = R.build_item(synth, oracle, 60, 1, 5, needed=False)
    out[("all-fixed", 11)] = R.build_item(synth, oracle, 11, 0, 6)
    out[("limit-base", 120)] = R.build_item(synth, oracle, 120, 1, 21)
    return out


def test_gate_values_sit_well_away_from_the_threshold(oracle, items):
    for k, it in items.items():
        g = R.gate_value(oracle, it)
        assert (g <= 0.9) if k[0] == "small" else (g >= 1.1), (k, g)


def test_items_have_the_shape_the_contract_asks_for(items):
    for k, it in items.items():
        n = it["n"]
        assert it["cur"] == n - 1 and it["cur"] in it["active"] and 0 <= it["loop"] < n and it["loop"] != it["cur"]
        assert np.all(np.diff(it["active"]) > 0) and it["active"].min() >= 0 and it["active"].max() < n
        assert np.all((it["e0"] >= 0) & (it["e0"] < n) & (it["e1"] >= 0) & (it["e1"] < n) & (it["e0"] != it["e1"]))
        assert not np.any((it["e0"] == it["cur"]) & (it["e1"] == it["loop"]))            # the call appends the loop edge itself
        assert it["first_active"].max() < len(it["active"]) and it["first_kf"].max() < n
        assert (it["first_active"] >= 0).any() and ((it["first_active"] < 0) & (it["first_kf"] >= 0)).any()


def test_structure_rule_puts_each_case_in_its_regime(pkg, oracle, items):
    st = pkg.api.loop_correct_structure
    header = open(pkg.api.HEADER_PATH).read()
    assert "#define MYSLAM_LOOP_CORRECT_MAX_SEPARATORS %d" % R.MAX_SEPARATORS in header and R.MAX_SEPARATORS >= 32

    def of(it):
        return st(it["n"], it["active"], it["loop"], it["e0"], it["e1"])
    base = items[("limit-base", 120)]
    free = 120 - 12                                                       # 10 active rows, the loop row, row 0
    assert of(items[("needed", 60)]) == (0, 60 - 12, True)                # one loop: the one the call appends, between two fixed rows
    assert of(items[("needed", 120)]) == (1, free - 1, True)              # one old loop
    assert of(items[("needed", 200)]) == (2, 200 - 12 - 2, True)
    assert of(items[("all-fixed", 11)]) == (0, 0, True)
    for count in (0, 1, 3, R.MAX_SEPARATORS, R.MAX_SEPARATORS + 1):
        it = R.add_short_loops(oracle, base, count) if count else base
        assert of(it) == (count, free - count, count <= R.MAX_SEPARATORS), count
    # the rule itself: the LATER free endpoint of an edge between free rows that are not neighbours; fixed rows do not count as rows between
    assert st(8, [6, 7], 5, [4, 3], [1, 2]) == (1, 3, True)               # free rows 1 2 3 4: (4, 1) is off the chain, (3, 2) is not
    assert st(8, [6, 7], 3, [4, 4], [2, 1]) == (1, 3, True)               # free rows 1 2 4 5: (4, 2) are neighbours, (4, 1) are not
    with pytest.raises(pkg.api.MyslamError):
        st(8, [6, 7], 8, [4], [2])


def test_reference_composition_closes_the_loop(oracle, items):
    for k, it in items.items():
        ref = R.reference(oracle, oracle, it)
        if k[0] == "small":
            assert ref["status"] == R.NOT_NEEDED and len(ref["e0"]) == len(it["e0"]) + 1 and np.array_equal(ref["poses"], it["poses"])
            continue
        assert ref["status"] == R.DONE
        fx = R.fixed_of(it)
        chi0 = oracle.pose_graph_optimize(ref["fused_poses"], fx, ref["e0"], ref["e1"], ref["meas"], iters=0)[1]
        if k[0] == "all-fixed":
            assert ref["iters"] == 0 and ref["chi2"] == chi0
            continue
        assert ref["iters"] >= 1 and ref["chi2"] < 0.5 * chi0, (k, ref["chi2"], chi0)
        # fusion put the current key-frame on the corrected pose, and the appended edge is then satisfied exactly
        assert np.abs(ref["fused_poses"][it["cur"]] - it["corrected"] / np.r_[np.full(4, np.linalg.norm(it["corrected"][:4])), 1, 1, 1]).max() < 1e-12
        moved = np.linalg.norm(ref["points"] - it["points"], axis=1)
        assert moved[it["first_active"] >= 0].min() > 0.5 and np.array_equal(ref["points"][(it["first_active"] < 0) & (it["first_kf"] < 0)],
                                                                               it["points"][(it["first_active"] < 0) & (it["first_kf"] < 0)])


def test_skipped_items_come_back_unchanged(synth, oracle):
    it = R.build_item(synth, oracle, 30, 1, 11, verify_status=2)
    ref = R.reference(oracle, oracle, it)
    assert ref["status"] == R.SKIPPED and all(np.array_equal(ref[k], it[k]) for k in ("poses", "points", "e0", "e1", "meas"))
