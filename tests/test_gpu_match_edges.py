"""GPU: the Hamming matcher's three instantiations and the stereo triangulation's three entry points on the hand-made inputs of
tests/match_tri_cases.py — ties at every register / half-wave / chunk / wave-group position, every distance 0 .. 256, counts outside [0, cap],
the 20-bit index limit and its refusal; the triangulation's two gates at their thresholds over four intrinsics sets, non-finite key-points,
match indices outside the slots.  Index and distance are compared bit for bit with the oracle AND with the builders' closed form; triangulated
points at the bar of tests/test_gpu_match_tri.py (rtol 1e-9, atol 1e-9), or 30 x the oracle's own one-ulp spread where that is larger.
The comparison helpers at the top need no GPU: tests/test_match_tri_cases.py feeds them faulty stand-ins and expects every one rejected."""
import numpy as np
import pytest

import match_tri_cases as MC

NARROW_MAX = 15                                        # fewer than 16 items per call: k_hamming_fp4<1, 4> (and <1, 4, true> with the tail)
WIDE_MIN = 16                                          # from 16 items on: k_hamming_fp4<4>
RTOL = ATOL = 1e-9                                     # test_triangulate_stereo's bar


# ---------------------------------------------------------------------------------------------------------- comparison helpers (CPU)
def check_hamming(oracle, case, idx, dist, tag):
    """idx, dist (B, cap) as a call left them in SENTINEL-filled outputs: equal to the oracle on every item's clamped counts, and to the
    builder's closed form in every slot (so slots past a count still hold the sentinel)"""
    q, nq, t, nt, ei, ed = case
    cap = q.shape[1]
    assert idx.shape == ei.shape and dist.shape == ed.shape and idx.dtype == np.int32 and dist.dtype == np.int32, tag
    for b in range(len(nq)):
        n, m = MC.clamp(nq[b], cap), MC.clamp(nt[b], cap)
        ri, rd = oracle.hamming_match(q[b, :n], t[b, :m])
        for name, got, want in (("index vs oracle", idx[b, :n], ri), ("distance vs oracle", dist[b, :n], rd),
                                ("index vs closed form", idx[b], ei[b]), ("distance vs closed form", dist[b], ed[b])):
            if not np.array_equal(got, want):
                k = int(np.flatnonzero(got != want)[0])
                raise AssertionError(f"{tag}: item {b} (nq {nq[b]}, nt {nt[b]}): {name}: slot {k}: got {got[k]}, want {want[k]}")


def xyz_tolerance(ref_xyz, spread):
    """per component: the project's bar, or 30 x the oracle's own spread where that spread exceeds a thirtieth of the bar"""
    bar = ATOL + RTOL * np.abs(ref_xyz)
    return np.where(spread < bar / 30, bar, 30 * spread), bar


def check_tri(ref, xyz, ok, tag):
    """ref: match_tri_cases.classify's result; xyz (n, 3) f64 and ok (n,) as the device wrote them.  Returns the figures DESIGN quotes:
    largest deviation and largest oracle spread over the stable accepted cases in units of the bar, and how many cases the spread rule held."""
    ok = np.asarray(ok)
    assert np.isin(ok.astype(np.int64), (0, 1)).all(), (tag, "ok is neither 0 nor 1")
    ok = ok.astype(bool)
    st = ref["stable"]
    bad = np.flatnonzero(st & (ok != ref["ok"]))
    assert len(bad) == 0, (tag, "decision differs on stable cases", bad[:8].tolist(), ref["ratio"][bad[:8]].tolist())
    un = ~st & ok
    assert (xyz[un, 2] > 0).all(), (tag, "accepted with z <= 0")
    sel = st & ref["ok"]
    tol, bar = xyz_tolerance(ref["xyz"][sel], ref["spread"][sel])
    dev = np.abs(xyz[sel] - ref["xyz"][sel])
    worst = np.flatnonzero(~(dev <= tol).all(1))
    assert len(worst) == 0, (tag, "xyz beyond the bar", np.flatnonzero(sel)[worst[:8]].tolist(), (dev / tol).max())
    return {"cases": int(len(st)), "unstable": int((~st).sum()), "compared": int(sel.sum()), "max_dev_over_bar": float((dev / bar).max()) if sel.any() else 0.0,
            "max_spread_over_bar": float((ref["spread"][sel] / bar).max()) if sel.any() else 0.0, "spread_rule_cases": int((tol > bar).any(1).sum())}


# ---------------------------------------------------------------------------------------------------------- device runners
def _dev(torch, a):
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.uint8) if a.dtype.fields else a).cuda()


def _benign_keypoints(B, cap, seed=9):
    rng = np.random.default_rng(seed)
    kl = np.zeros((B, cap), MC.KP); kr = np.zeros((B, cap), MC.KP)
    kl["x"] = rng.uniform(20, 1220, (B, cap)); kl["y"] = rng.uniform(20, 350, (B, cap))
    kr["x"] = kl["x"] - rng.uniform(3, 90, (B, cap)); kr["y"] = kl["y"] + rng.normal(0, 0.3, (B, cap))
    return kl, kr


KITTI = (718.856, 718.856, 607.1928, 185.2157)


def run_hamming(api, case, form):
    """the builder's items through one instantiation -> (idx, dist) (B, cap) with SENTINEL where nothing was written.
    "narrow": calls of 15 items; "wide": one call of >= 16 items (the items repeated if there are fewer); "fused": calls of 15 items through the
    matcher + triangulation call with benign key-points."""
    import torch
    q, nq, t, nt, _, _ = case
    B, cap = q.shape[:2]
    if form == "wide" and B < WIDE_MIN:
        rep = -(-WIDE_MIN // B)
        q, t, nq, nt = np.tile(q, (rep, 1, 1)), np.tile(t, (rep, 1, 1)), np.tile(nq, rep), np.tile(nt, rep)
    n = len(nq)
    dq, dt, dnq, dnt = _dev(torch, q), _dev(torch, t), _dev(torch, nq), _dev(torch, nt)
    di = torch.full((n, cap), MC.SENTINEL, dtype=torch.int32, device="cuda"); dd = torch.full((n, cap), MC.SENTINEL, dtype=torch.int32, device="cuda")
    s = torch.cuda.current_stream().cuda_stream
    if form == "wide":
        api.hamming_match_batch(dq.data_ptr(), dnq.data_ptr(), dt.data_ptr(), dnt.data_ptr(), n, cap, di.data_ptr(), dd.data_ptr(), s)
    else:
        if form == "fused":
            kl, kr = _benign_keypoints(n, cap)
            dkl, dkr = _dev(torch, kl), _dev(torch, kr)
            dx = torch.zeros((n, cap, 3), dtype=torch.float64, device="cuda"); dok = torch.full((n, cap), 9, dtype=torch.uint8, device="cuda")
        for lo in range(0, n, NARROW_MAX):
            k = min(NARROW_MAX, n - lo)
            a = (dq.data_ptr() + lo * cap * 32, dnq.data_ptr() + lo * 4, dt.data_ptr() + lo * cap * 32, dnt.data_ptr() + lo * 4)
            o = (di.data_ptr() + lo * cap * 4, dd.data_ptr() + lo * cap * 4)
            if form == "narrow":
                api.hamming_match_batch(*a, k, cap, *o, s)
            else:
                api.hamming_match_triangulate_batch(*a, dkl.data_ptr() + lo * cap * 28, dkr.data_ptr() + lo * cap * 28, k, cap, KITTI, 0.537, *o,
                                                    dx.data_ptr() + lo * cap * 24, dok.data_ptr() + lo * cap, s)
    torch.cuda.synchronize()
    gi, gd = di.cpu().numpy(), dd.cpu().numpy()
    if form == "fused":                                # the tail wrote exactly the slots the matcher wrote, with a decision
        ok = dok.cpu().numpy()
        assert ((ok == 9) == (gi == MC.SENTINEL)).all() and np.isin(ok, (0, 1, 9)).all()
        assert not ok[gi == -1].any()
    if n > B:
        assert np.array_equal(gi.reshape(-1, B, cap)[1:], np.broadcast_to(gi[:B], (n // B - 1, B, cap))), "repeated items differ"
    return gi[:B], gd[:B]


def layout(xl, yl, xr, yr, per, cap, seed=12):
    """flat points -> items of `per` points in `cap` slots for the key-point forms: left point i of an item is matched to right slot n - 1 - i,
    which the matcher finds by itself (its descriptor is left i's, every descriptor distinct)"""
    rng = np.random.default_rng(seed)
    n = len(xl)
    B = -(-n // per)
    kl = np.zeros((B, cap), MC.KP); kr = np.zeros((B, cap), MC.KP)
    kl["x"] = 100.0; kl["y"] = 100.0; kr["x"] = 90.0; kr["y"] = 100.0
    dl = rng.integers(0, 256, (B, cap, 32), dtype=np.uint8); dr = rng.integers(0, 256, (B, cap, 32), dtype=np.uint8)
    match = np.full((B, cap), -1, np.int32)
    nl = np.zeros(B, np.int32)
    for b in range(B):
        i = np.arange(b * per, min(n, (b + 1) * per))
        m = len(i)
        j = m - 1 - np.arange(m)
        nl[b] = m
        kl["x"][b, :m] = xl[i]; kl["y"][b, :m] = yl[i]
        kr["x"][b, j] = xr[i]; kr["y"][b, j] = yr[i]
        dr[b, j] = dl[b, :m]
        match[b, :m] = j
    return {"kl": kl, "kr": kr, "dl": dl, "dr": dr, "match": match, "nl": nl, "per": per, "cap": cap, "n": n}


def run_tri_forms(api, K5, xl, yl, xr, yr, per=40, cap=48):
    """the same points through myslam_triangulate_stereo, myslam_triangulate_stereo_batch and the fused matcher tail (calls of 15 items), the
    three compared byte for byte -> (xyz (n, 3), ok (n,) uint8)"""
    import torch
    K, base = K5[:4], K5[4]
    n = len(xl)
    fxyz, fok = api.triangulate_stereo(xl, yl, xr, yr, *K5)
    L = layout(xl, yl, xr, yr, per, cap)
    B = len(L["nl"])
    d = {k: _dev(torch, L[k]) for k in ("kl", "kr", "dl", "dr", "match", "nl")}
    s = torch.cuda.current_stream().cuda_stream
    new = lambda: (torch.full((B, cap, 3), -7.0, dtype=torch.float64, device="cuda"), torch.full((B, cap), 9, dtype=torch.uint8, device="cuda"))
    kx, kok = new()
    api.triangulate_stereo_batch(d["kl"].data_ptr(), d["kr"].data_ptr(), d["match"].data_ptr(), d["nl"].data_ptr(), B, cap, K, base, kx.data_ptr(), kok.data_ptr(), s)
    ux, uok = new()
    ui = torch.full((B, cap), MC.SENTINEL, dtype=torch.int32, device="cuda"); ud = torch.full((B, cap), MC.SENTINEL, dtype=torch.int32, device="cuda")
    for lo in range(0, B, NARROW_MAX):
        k = min(NARROW_MAX, B - lo)
        api.hamming_match_triangulate_batch(d["dl"].data_ptr() + lo * cap * 32, d["nl"].data_ptr() + lo * 4, d["dr"].data_ptr() + lo * cap * 32,
                                            d["nl"].data_ptr() + lo * 4, d["kl"].data_ptr() + lo * cap * 28, d["kr"].data_ptr() + lo * cap * 28, k, cap, K, base,
                                            ui.data_ptr() + lo * cap * 4, ud.data_ptr() + lo * cap * 4, ux.data_ptr() + lo * cap * 24, uok.data_ptr() + lo * cap, s)
    torch.cuda.synchronize()
    kx, kok, ux, uok, ui, ud = [a.cpu().numpy() for a in (kx, kok, ux, uok, ui, ud)]
    used = np.arange(cap)[None, :] < L["nl"][:, None]
    assert np.array_equal(ui[used], L["match"][used]) and (ud[used] == 0).all() and (ui[~used] == MC.SENTINEL).all(), "the matcher did not return the planted matches"
    assert kx.tobytes() == ux.tobytes() and kok.tobytes() == uok.tobytes(), "key-point form and fused tail differ"
    assert (kok[~used] == 9).all() and (kx[~used] == -7.0).all(), "slots past nl were written"
    gx, gok = kx[used], kok[used]                      # row-major: the flat order
    assert len(gok) == n and gx.tobytes() == np.ascontiguousarray(fxyz).tobytes() and np.array_equal(gok.astype(bool), fok), "float-array form and key-point form differ"
    return gx, gok


# ---------------------------------------------------------------------------------------------------------- matcher
FORMS = ["narrow", "wide", "fused"]


@pytest.mark.gpu
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("builder", list(MC.HAMMING_BUILDERS))
def test_hamming_builders_bit_exact(api, oracle, builder, form):
    case = MC.HAMMING_BUILDERS[builder]()
    gi, gd = run_hamming(api, case, form)
    check_hamming(oracle, case, gi, gd, f"{builder}/{form}")
    if form == "fused":
        ni, nd = run_hamming(api, case, "narrow")
        assert gi.tobytes() == ni.tobytes() and gd.tobytes() == nd.tobytes()


@pytest.mark.gpu
@pytest.mark.parametrize("builder", ["suffix_ties", "pair_ties"])
def test_tie_builders_through_the_single_call(api, oracle, builder):
    q, nq, t, nt, ei, ed = MC.HAMMING_BUILDERS[builder]()
    for b in range(len(nq)):
        gi, gd = api.hamming_match(q[b, :nq[b]], t[b, :nt[b]])
        ri, rd = oracle.hamming_match(q[b, :nq[b]], t[b, :nt[b]])
        assert np.array_equal(gi, ri) and np.array_equal(gd, rd), (builder, b)
        assert np.array_equal(gi, ei[b, :nq[b]]) and np.array_equal(gd, ed[b, :nq[b]]), (builder, b)


LIMIT = (1 << 20) - 1


@pytest.mark.gpu
def test_index_limit_and_its_refusal(api, oracle):
    """the largest accepted train set: the unique best of query 0 in the last row (0xFFFFE, key field 1), a tie between row 5 and the last row
    for query 1, a second item whose only row is at distance 256 (key 0xFFFFF: all that separates it from "no row"); one more row is refused."""
    import torch
    rng = np.random.default_rng(20)
    nq = 130
    q = rng.integers(0, 256, (nq, 32), dtype=np.uint8)
    t = rng.integers(0, 256, (LIMIT, 32), dtype=np.uint8)
    t[LIMIT - 1] = q[0]
    t[5] = q[0]; t[5, 0] ^= 3
    q[1] = q[0]; q[1, 0] ^= 1                            # one bit from the last row, one from row 5
    ri, rd = oracle.hamming_match(q, t)
    assert ri[0] == LIMIT - 1 == 0xFFFFE and rd[0] == 0 and ri[1] == 5 and rd[1] == 1
    gi, gd = api.hamming_match(q, t)
    assert np.array_equal(gi, ri) and np.array_equal(gd, rd)
    q2 = rng.integers(0, 256, (3, 32), dtype=np.uint8); q2[1:] = q2[0]
    # one buffer for both kernels: 16 items of LIMIT slots, items 2 .. 15 empty
    B = 16
    dq = torch.zeros((B, LIMIT, 32), dtype=torch.uint8, device="cuda"); dt = torch.zeros((B, LIMIT, 32), dtype=torch.uint8, device="cuda")
    dq[0, :nq] = torch.from_numpy(q).cuda(); dt[0] = torch.from_numpy(t).cuda()
    dq[1, :3] = torch.from_numpy(q2).cuda(); dt[1, 0] = torch.from_numpy(~q2[0]).cuda()
    cnt_q = np.zeros(B, np.int32); cnt_t = np.zeros(B, np.int32)
    cnt_q[:2] = (nq, 3); cnt_t[:2] = (LIMIT, 1)
    dnq, dnt = torch.from_numpy(cnt_q).cuda(), torch.from_numpy(cnt_t).cuda()
    s = torch.cuda.current_stream().cuda_stream
    for batch in (2, B):                               # k_hamming_fp4<1, 4> and k_hamming_fp4<4>
        di = torch.full((B, LIMIT), MC.SENTINEL, dtype=torch.int32, device="cuda"); dd = torch.full((B, LIMIT), MC.SENTINEL, dtype=torch.int32, device="cuda")
        api.hamming_match_batch(dq.data_ptr(), dnq.data_ptr(), dt.data_ptr(), dnt.data_ptr(), batch, LIMIT, di.data_ptr(), dd.data_ptr(), s)
        torch.cuda.synchronize()
        assert np.array_equal(di[0, :nq].cpu().numpy(), ri) and np.array_equal(dd[0, :nq].cpu().numpy(), rd), batch
        assert di[1, :3].cpu().tolist() == [0, 0, 0] and dd[1, :3].cpu().tolist() == [256, 256, 256], batch
        assert int((di != MC.SENTINEL).sum()) == nq + 3 and int((dd != MC.SENTINEL).sum()) == nq + 3, batch
    # refused before anything is launched: the outputs keep their bytes
    di = torch.full((B, LIMIT), MC.SENTINEL, dtype=torch.int32, device="cuda"); dd = torch.full((B, LIMIT), MC.SENTINEL, dtype=torch.int32, device="cuda")
    for batch in (1, 15):                              # 15 x 2^20 slots still lie inside the 16 x (2^20 - 1) allocated ones
        with pytest.raises(api.MyslamError) as e:
            api.hamming_match_batch(dq.data_ptr(), dnq.data_ptr(), dt.data_ptr(), dnt.data_ptr(), batch, 1 << 20, di.data_ptr(), dd.data_ptr(), s)
        assert e.value.code == api.ERR_UNSUPPORTED
    torch.cuda.synchronize()
    assert bool((di == MC.SENTINEL).all()) and bool((dd == MC.SENTINEL).all())
    with pytest.raises(api.MyslamError) as e:
        api.hamming_match(q[:2], np.concatenate([t, t[:1]]))
    assert e.value.code == api.ERR_UNSUPPORTED


# ---------------------------------------------------------------------------------------------------------- triangulation
INTRINSICS = ["kitti00", "anisotropic_off_centre", "baseline_5cm", "baseline_5m"]


@pytest.mark.gpu
@pytest.mark.parametrize("name", INTRINSICS)
def test_gate_ladder_three_forms_against_the_oracle(api, oracle, synth, name):
    L = MC.gate_ladder(oracle, synth, name)
    xyz, ok = run_tri_forms(api, L["K5"], L["xl"], L["yl"], L["xr"], L["yr"])
    fig = check_tri(L["ref"], xyz, ok, name)
    print(f"\ngate ladder {name}: {fig}")


@pytest.mark.gpu
def test_non_finite_key_points(api, oracle, synth):
    c = MC.nonfinite(synth)
    bx, bok = run_tri_forms(api, c["K5"], *c["bad"])
    gx, gok = run_tri_forms(api, c["K5"], *c["good"])
    assert not bok[c["nonfinite"]].any()
    keep = np.ones(len(bok), bool); keep[c["where"]] = False
    assert bx[keep].tobytes() == gx[keep].tobytes() and np.array_equal(bok[keep], gok[keep])
    assert gok[keep].mean() > 0.95
    rx, rok = oracle.triangulate_stereo(*c["good"], *c["K5"])
    assert np.array_equal(gok.astype(bool), rok) and np.allclose(gx[rok], rx[rok], rtol=RTOL, atol=ATOL)
    huge = np.setdiff1d(c["where"], c["nonfinite"])        # +-3e38 is a finite float: the oracle decides
    with np.errstate(all="ignore"):
        ref = MC.classify(oracle, c["K5"], *[a[huge] for a in c["bad"]])
    print(f"\n+-3e38 points: {check_tri(ref, bx[huge], bok[huge], 'huge')}, accepted {int(ref['ok'].sum())} of {len(huge)}")


@pytest.mark.gpu
def test_match_indices_outside_the_slots(api, oracle, synth):
    import torch
    c = MC.bad_matches(synth)
    want_xyz, want_ok, written = MC.bad_matches_expected(oracle, c)
    B, cap = c["match"].shape
    s = torch.cuda.current_stream().cuda_stream
    dm, dn = _dev(torch, c["match"]), _dev(torch, c["nl"])

    def run(kl, kr):
        dkl, dkr = _dev(torch, kl), _dev(torch, kr)
        x = torch.full((B, cap, 3), -7.0, dtype=torch.float64, device="cuda"); o = torch.full((B, cap), 9, dtype=torch.uint8, device="cuda")
        api.triangulate_stereo_batch(dkl.data_ptr(), dkr.data_ptr(), dm.data_ptr(), dn.data_ptr(), B, cap, c["K5"][:4], c["K5"][4], x.data_ptr(), o.data_ptr(), s)
        torch.cuda.synchronize()
        return x.cpu().numpy(), o.cpu().numpy()
    x, o = run(c["kl"], c["kr"])
    assert (o[~written] == 9).all() and (x[~written] == -7.0).all()                       # nl above cap is clamped, a negative nl writes nothing
    invalid = written & ((c["match"] < 0) | (c["match"] >= cap))
    assert invalid.sum() >= 5 * 5 and not o[invalid].any() and (x[invalid] == 0).all()
    valid = written & ~invalid
    assert np.array_equal(o[valid].astype(bool), want_ok[valid]) and want_ok[valid].mean() > 0.9
    sel = valid & want_ok
    assert np.allclose(x[sel], want_xyz[sel], rtol=RTOL, atol=ATOL)
    x2, o2 = run(c["kl_clean"], c["kr_clean"])                                            # only x and y are read
    assert x.tobytes() == x2.tobytes() and o.tobytes() == o2.tobytes()
