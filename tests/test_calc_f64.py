"""Host only.  (1) The f64 net of tests/calc_f64.py against the f32 CPU oracle on every model of tests/calc_ranges.py: the reference of the
device tests is pinned, and the oracle-vs-f64 error per model is the floor against which the device bars are judged.  (2) A NumPy emulation
of the f16 x 3 split product of k_conv2_f16x3 / k_conv1_f16x3_pool_lrn over weight and activation scales: the written-down derivation of
the lower bound in lcd_create's kernel-family selection.  Run with -s to see both tables."""
import numpy as np
import pytest

import calc_f64
import calc_ranges

DESC_ATOL = 2e-5            # the descriptor bar of tests/test_gpu_lcd.py (absolute, entries are O(0.03))
TAP_BAR = 5e-6              # the max-normalised bar of the stage taps

F16_WMIN = calc_ranges.F16_WMIN          # the lower bound of lcd_create's f16 family; tests/test_gpu_lcd_ranges.py pins it to the library


# ---- B1: the reference itself ----
@pytest.fixture(scope="module")
def floor_table():
    rows = []
    yield rows
    print("\noracle (f32, CPU) against forward_f64: largest |descriptor difference| per model   (bar %g, fair-case limit %g)" % (DESC_ATOL, DESC_ATOL / 2))
    for name, e in rows:
        print("  %-12s %.3g" % (name, e))


@pytest.mark.parametrize("name", calc_ranges.MODELS)
def test_f64_net_against_the_f32_oracle(oracle, synth, floor_table, name):
    """The oracle exposes the descriptor only (no stage taps): that is what is compared.  A model on which the f32 oracle alone is not inside
    HALF the device bar would not be a fair case for the device."""
    L, w, _ = calc_ranges.model(synth, name)
    x = calc_ranges.inputs(synth)["uniform"]
    ref = calc_f64.forward_f64(L, w, x)
    for s in range(5):
        assert np.isfinite(ref[s]).all() and np.abs(ref[s]).max() > 0, (name, s)
    got = oracle.calc_forward_net(L, w, x)
    err = float(np.abs(got - ref[4]).max())
    floor_table.append((name, err))
    assert err < DESC_ATOL / 2, (name, err)
    assert abs(np.linalg.norm(ref[4]) - 1) < 1e-12


def test_f64_net_default_list_equals_the_plain_torch_calls(synth):
    """forward_f64 walking the layer list = the torch calls written out for the SURVEY A.6 net (torch's own LRN included)"""
    import torch
    import torch.nn.functional as F
    L, w, _ = calc_ranges.model(synth, "base")
    x = calc_ranges.inputs(synth)["uniform"]
    w1, b1, w2, b2, w3, b3 = (torch.from_numpy(p.astype(np.float64)) for p in calc_ranges._parts(w))
    t = torch.from_numpy(x.astype(np.float64))[None, None]
    a1 = F.relu(F.conv2d(t, w1.reshape(64, 1, 5, 5), b1, stride=2, padding=4))
    p1 = F.local_response_norm(F.max_pool2d(a1, 3, 2, ceil_mode=True), 5, alpha=float(np.float32(1e-4)), beta=0.75, k=1.0)
    a2 = F.relu(F.conv2d(p1, w2.reshape(128, 64, 4, 4), b2, stride=1, padding=2))
    p2 = F.local_response_norm(F.max_pool2d(a2, 3, 2, ceil_mode=True), 5, alpha=float(np.float32(1e-4)), beta=0.75, k=1.0)
    a3 = F.relu(F.conv2d(p2, w3.reshape(4, 128, 3, 3), b3))
    ref = calc_f64.forward_f64(L, w, x)
    for s, r in enumerate((a1, p1, a2, p2)):
        assert ref[s].shape == tuple(r.shape[1:]) and np.abs(ref[s] - r[0].numpy()).max() <= 1e-13 * np.abs(ref[s]).max(), s
    d = a3[0].numpy().ravel()
    assert np.abs(ref[4] - d / np.linalg.norm(d)).max() < 1e-14


def test_f64_net_honours_the_layer_list(oracle, synth):
    """a dropped ReLU, an LRN window of 3 with other alpha / beta / k, a net without LRN layers: the oracle's layer-list forward agrees"""
    w = synth.calc_weights(); x = calc_ranges.inputs(synth)["u8"]
    base = calc_f64.default_layers()
    L1 = base[:-1]
    L2 = base.copy(); L2["local_size"][3] = 3; L2["alpha"][3] = 0.3; L2["beta"][7] = 1.25; L2["k"][7] = 2.0
    L3 = base[[0, 1, 2, 4, 5, 6, 8, 9]]
    outs = []
    for L in (base, L1, L2, L3):
        d = calc_f64.forward_f64(L, w, x)[4]
        assert np.abs(oracle.calc_forward_net(L, w, x) - d).max() < DESC_ATOL / 2
        outs.append(d)
    assert np.abs(outs[2] - outs[0]).max() > 10 * DESC_ATOL        # alpha = 0.3 on a window of 3 is no small change
    assert np.abs(outs[3] - outs[0]).max() > 1e-6                  # alpha = 1e-4 is: dropping the LRNs still shows, well above the f32 floor


def test_f64_net_zero_norm_is_ieee_division(oracle, synth):
    """an emptied map: x / 0 in IEEE arithmetic (0 / 0 = NaN everywhere), as the oracle's f32 division gives"""
    L, w = calc_ranges.zero_norm_model(synth)
    ins = calc_ranges.inputs(synth)
    for name in ("zeros", "ones"):
        d = calc_f64.forward_f64(L, w, ins[name])[4]
        assert np.isnan(d).all(), name
        assert np.isnan(oracle.calc_forward_net(L, w, ins[name])).all(), name
    d = calc_f64.forward_f64(L, w, ins["u8"])[4]
    assert np.isfinite(d).all() and (d > 0).sum() >= 4            # a textured image keeps a populated map
    assert np.abs(oracle.calc_forward_net(L, w, ins["u8"]) - d).max() < DESC_ATOL / 2


def test_references_of_the_device_tests_are_populated(oracle, synth):
    """What tests/test_gpu_lcd_ranges.py relies on: no stage of any (model, input) it compares is identically zero (a max-normalised bar would
    pass on an empty map), and the neighbours of its zero-norm batch keep every conv3 output well away from the ReLU's kink (an f32 rounding
    must not be able to empty or populate an entry)."""
    ins = calc_ranges.inputs(synth)
    for name in ("base", "c2down14", "c1down14"):
        L, w, _ = calc_ranges.model(synth, name)
        for iname, x in ins.items():
            for s, r in enumerate(calc_f64.forward_f64(L, w, x)):
                assert np.isfinite(r).all() and np.abs(r).max() > 0, (name, iname, s)
    L, w = calc_ranges.zero_norm_model(synth)
    for seed in (79, 80):
        x, _ = oracle.calc_preproc(synth.random_image(seed, 120, 160))
        lin = calc_f64.forward_f64(L[:-1], w, x)[4]                  # the map before the ReLU, normalised
        assert (lin > 0).sum() >= 4 and np.abs(lin).min() > 1e-4, (seed, float(np.abs(lin).min()))
    x, _ = oracle.calc_preproc(np.full((120, 160), 255, np.uint8))
    assert calc_f64.forward_f64(L[:-1], w, x)[4].max() < -1e-4       # the flat image is empty with room to spare


# ---- B2: the f16 x 3 split product, emulated ----
def _f16(v, flush):
    h = np.asarray(v, np.float32).astype(np.float16)              # round to nearest even, subnormals kept
    if flush:
        h = np.where(np.abs(h.astype(np.float32)) < 2.0 ** -14, np.float16(0), h)
    return h.astype(np.float64)


def _split(a, flush, weight_side):
    """a = h + m' 2^-11 as the kernels split it (cv_split2_f16 / lcd_create): h = f16(a), m' = f16((a - h) 2^11); weights carry Hs = f16(2^11 h).
    `flush` zeroes every f16 subnormal operand, as a matrix unit that flushes its inputs would see them."""
    a = np.asarray(a, np.float32)
    h32 = a.astype(np.float16).astype(np.float32)                  # the kernels compute the residual from the unflushed f16 value
    m = _f16((a - h32) * np.float32(2048.0), flush)
    hs = _f16(h32 * np.float32(2048.0), flush) if weight_side else None
    return _f16(a, flush), m, hs


def emulate_f16x3(s_w, s_a, flush, K=1024, M=48, N=64, seed=5, wmax=None):
    """(max-normalised error of the three-product sum against f64, the same of a plain f32 product, max |w|) for activations
    uniform(0, 1) s_a with half of them zero (after a ReLU) and weights N(0, 1) s_w; f64 products and sums of the f16 pieces (exact)."""
    rng = np.random.default_rng(seed)
    A = (rng.uniform(0, 1, (M, K)) * (rng.uniform(0, 1, (M, K)) < 0.5) * s_a).astype(np.float32)
    B = rng.standard_normal((K, N)) * s_w
    B = (B if wmax is None else B * (wmax / np.abs(B).max())).astype(np.float32)     # wmax: max |w| exactly there
    ref = A.astype(np.float64) @ B.astype(np.float64)
    ha, ma, _ = _split(A, flush, False)
    hb, mb, hsb = _split(B, flush, True)
    got = (ha @ hsb + ha @ mb + ma @ hb) / 2048.0
    f32 = (A @ B).astype(np.float64)
    den = np.abs(ref).max()
    return float(np.abs(got - ref).max() / den), float(np.abs(f32 - ref).max() / den), float(np.abs(B).max())


S_W = (3e-2, 2.0 ** -9, 1e-4, 2e-5, 1e-6, 1e-8) + tuple(2.0 ** -(5 + k) for k in calc_ranges.SCALE_K)      # the last five: conv2 of the c2down models
S_A = (1.0, 1e-5)


def test_f16x3_emulation_gives_the_lower_bound_of_the_f16_family():
    rows = []
    for s_w in sorted(S_W, reverse=True):
        kept = [emulate_f16x3(s_w, s_a, False) for s_a in S_A]
        flushed = [emulate_f16x3(s_w, s_a, True) for s_a in S_A]
        rows.append((s_w, kept[0][2], [r[0] for r in kept], [r[0] for r in flushed], kept[0][1]))
    print("\nf16 x 3 split product, K = 1024, max-normalised error against f64 (emulation: says nothing about any hardware)")
    print("      s_w    max|w| | kept: s_a=1  s_a=1e-5 | flushed: s_a=1  s_a=1e-5 | plain f32")
    for s_w, wmax, kept, flushed, f32 in rows:
        print("  %8.2e %8.2e |   %8.1e  %8.1e |      %8.1e  %8.1e |  %8.1e" % (s_w, wmax, kept[0], kept[1], flushed[0], flushed[1], f32))
    for s_w, wmax, kept, flushed, f32 in rows:
        if s_w >= 2e-5:
            assert max(kept) < TAP_BAR, (s_w, kept)               # f16 keeps its 10 mantissa bits above 6.1e-5: the split holds the bar
        assert f32 < TAP_BAR                                      # f32 (and a bf16 split, which has f32's exponent range) does not care
    assert any(kept[0] > TAP_BAR for s_w, _, kept, _, _ in rows if s_w < 2e-5), "the split must cross the bar somewhere below 2e-5"
    # With subnormals kept, 16 x the largest weight of the smallest passing scale (s_w = 2e-5), rounded up to a power of two, would do: 2^-9.
    wmax_ok = [wmax for s_w, wmax, _, _, _ in rows if s_w == 2e-5][0]
    assert 16 * wmax_ok <= 2.0 ** -9 < 32 * wmax_ok and F16_WMIN >= 2.0 ** -9, (wmax_ok, F16_WMIN)
    # Whether the f16 matrix instructions keep subnormal operands has not been measured, and no model below the bound can measure it (the loader
    # sends it to bf16 x 6).  So the loader's bound is the one that also holds were they flushed (the m' plane of a weight below ~1e-4 is
    # subnormal): with max |w| exactly on a power of two, the smallest one at which the flushed emulation stays under the bar on every seed
    # (2^-7, by a factor of 1.2 only, and the figure moves by more than that between seeds) times two.
    print("  max|w| exactly on a power of two, s_a = 1, seeds 5 6 7: inputs flushed / kept")
    flushed_at = {}
    for e in range(-9, -4):
        fl = [emulate_f16x3(1.0, 1.0, True, seed=sd, wmax=2.0 ** e)[0] for sd in (5, 6, 7)]
        kp = [emulate_f16x3(1.0, 1.0, False, seed=sd, wmax=2.0 ** e)[0] for sd in (5, 6, 7)]
        flushed_at[e] = max(fl)
        print("  2^%d   %s / %s" % (e, " ".join("%.1e" % v for v in fl), " ".join("%.1e" % v for v in kp)))
        assert max(kp) < TAP_BAR / 16
    e_min = int(np.log2(F16_WMIN))
    assert flushed_at[e_min] < flushed_at[e_min - 1] < TAP_BAR < flushed_at[e_min - 2], (F16_WMIN, flushed_at)
