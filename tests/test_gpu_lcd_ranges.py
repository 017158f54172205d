"""GPU: the CALC kernels over the ranges of the model, not only at N(0, 1 / fan_in) weights and a uniform(0, 1) image.

Every stage tap (0 .. 3) of a device handle is compared with the f64 net of tests/calc_f64.py at the project's bar of 5e-6 max-normalised, the
descriptor (stage 4) at DESC_ATOL absolute — for whatever kernel family lcd_create chose for the model (f16 x 3 or bf16 x 6), and for the bf16
family forced where the test says so.  The f32 CPU oracle alone sits at ~1e-7 on every one of these models (tests/test_calc_f64.py prints the
floor): all of them are fair cases.  Models: tests/calc_ranges.py."""
import numpy as np
import pytest

import calc_f64
import calc_ranges

pytestmark = pytest.mark.gpu

DESC_ATOL = 2e-5            # as tests/test_gpu_lcd.py
TAP_BAR = 5e-6              # as test_layer_taps_against_torch

_REF = {}


def _ref(synth, model, inp):
    """f64 stages of (model, input): computed once, shared, never written to"""
    if (model, inp) not in _REF:
        L, w, _ = calc_ranges.model(synth, model)
        r = calc_f64.forward_f64(L, w, calc_ranges.inputs(synth)[inp])
        for a in r:
            a.setflags(write=False)
        _REF[(model, inp)] = r
    return _REF[(model, inp)]


def _check(lcd, x, ref, label, without_channel=None):
    """stages 0 .. 4 of `lcd` on x against the f64 stages `ref`; prints every figure before it asserts anything.  `without_channel`: the
    conv1 stages (0, 1) are judged a second time with that channel left out of both the error and its normalisation."""
    errs, rest = [], []
    for s in range(5):
        assert np.abs(ref[s]).max() > 0, (label, s, "empty reference stage")
        got = lcd.debug_forward(x, s)
        if s < 4:
            got = calc_f64.nhwc_to_nchw(got, ref[s].shape)
            errs.append(calc_f64.maxnorm_err(got, ref[s]))
            if without_channel is not None and s < 2:
                keep = np.arange(ref[s].shape[0]) != without_channel
                assert np.abs(ref[s][keep]).max() > 0
                rest.append(calc_f64.maxnorm_err(got[keep], ref[s][keep]))
        else:
            errs.append(float(np.abs(got.astype(np.float64) - ref[4]).max()))
    print("%-34s products %d  taps %s  descriptor %.2e%s" % (label, lcd.conv2_products(), " ".join("%.2e" % e for e in errs[:4]), errs[4],
                                                              "  stages 0, 1 without channel %d: %s" % (without_channel, " ".join("%.2e" % e for e in rest)) if rest else ""))
    for s in range(4):
        assert errs[s] < TAP_BAR, (label, "stage", s, errs[s])
    for s, e in enumerate(rest):
        assert e < TAP_BAR, (label, "stage", s, "without channel", without_channel, e)
    assert errs[4] < DESC_ATOL, (label, "descriptor", errs[4])
    return errs


def _handle(api, synth, model, bf16=False):
    L, w, products = calc_ranges.model(synth, model)
    lcd = api.DeepLCD(w, layers=L)
    assert lcd.uses_fused_kernels()
    assert lcd.conv2_products() == products, (model, lcd.conv2_products())
    if bf16:
        lcd.set_option(lcd.OPT_CONV2_BF16X6, 1)
        assert lcd.conv2_products() == 6
    return lcd


@pytest.mark.parametrize("model", calc_ranges.MODELS)
def test_model_meets_the_bars_with_the_family_the_loader_chose(api, synth, model):
    """The contract: every model the loader accepts meets the bars with the kernels the loader chose, and the loader's choice is the expected
    one on each side of every bound of the selection rule.  The c2down / c1down models put conv2's weights / activations 2^-10 .. 2^-27 below
    the base model's, all under the rule's lower bound: from 2^-20 on the f16 x 3 split has lost the bar by orders of magnitude (emulation:
    tests/test_calc_f64.py), the loader has to send them to bf16 x 6.  w2min / w1min sit exactly ON the lower bound and run the f16 kernels
    with the smallest weights' h planes and many of the m' planes in f16's subnormal range.  The bound is chosen so that they hold the bar even
    on a matrix unit that flushes subnormal operands (emulated: 3e-6 on the taps flushed, 1e-7 kept — the printed figure tells which).  In the bound59000 / bound60500 models one
    conv1 channel is ~6e4 and owns the normalisation of stages 0 and 1: those stages are judged again without it."""
    lcd = _handle(api, synth, model)
    _check(lcd, calc_ranges.inputs(synth)["uniform"], _ref(synth, model, "uniform"), model,
           without_channel=calc_ranges.BOUND_CHANNEL if model.startswith("bound") else None)


def test_default_layer_list_is_the_librarys(api):
    """calc_f64.default_layers() is a copy of the library's list (so that the host tests need no library): pinned here"""
    assert calc_f64.default_layers().tobytes() == api.calc_default_layers().tobytes()


@pytest.mark.parametrize("model", calc_ranges.BASE)
def test_base_models_with_the_bf16_family_forced(api, synth, model):
    lcd = _handle(api, synth, model, bf16=True)
    _check(lcd, calc_ranges.inputs(synth)["uniform"], _ref(synth, model, "uniform"), model + " (bf16 forced)")


@pytest.mark.parametrize("model,bf16", [("base", False), ("base", True), ("c2down14", False), ("c1down14", False)])
def test_inputs_and_borders(api, synth, model, bf16):
    """A uniform image, an 8-bit image / 255, all zeros, all ones, a checkerboard, and single impulses: an impulse lays every tap of the
    (asymmetric) banks at a known place of every stage; the corner ones go through conv1's pad-4 rows, the clipped ceil-mode pool windows and
    conv2's pad-2 halo."""
    lcd = _handle(api, synth, model, bf16)
    for name, x in calc_ranges.inputs(synth).items():
        _check(lcd, x, _ref(synth, model, name), "%s%s / %s" % (model, " (bf16 forced)" if bf16 else "", name))


def _describe_batch(lcd, imgs):
    """descriptors of 120 x 160 images through describe_batch, row pitch cols + 7 (the padding bytes are not image)"""
    import torch
    B = len(imgs)
    host = np.full((B, 120, 167), 201, np.uint8)
    for b, im in enumerate(imgs):
        host[b, :, :160] = im
    d_imgs = torch.from_numpy(host).cuda(); d_out = torch.zeros(B, 1064, device="cuda")
    lcd.describe_batch(d_imgs.data_ptr(), B, 120, 160, 167, 120 * 167, d_out.data_ptr(), blur_in_place=False)
    torch.cuda.synchronize()
    assert np.array_equal(d_imgs.cpu().numpy(), host)
    return d_out.cpu().numpy()


@pytest.mark.parametrize("bf16", [False, True], ids=["f16x3", "bf16x6"])
@pytest.mark.parametrize("B", [2, 3, 5])
def test_batch_image_equals_the_image_alone(api, oracle, synth, B, bf16):
    """Image b of a batch = the same image described alone, bit for bit: no kernel of lcd_forward changes its per-image arithmetic with the
    batch size.  Neighbours are maximally different (all 255, all 0, noise, texture, checkerboard), so a halo of k_conv2_f16x3's 6 x 45 patch
    that read the next image instead of zeros, a row of k_conv2_bf16x6's 128-row tiles taken from the wrong image (M2 = 1344 = 10.5 tiles: a
    tile straddles two images at every odd index) or k_l2norm_1064's second block (B = 5) taking another image's norm cannot hide."""
    lcd = _handle(api, synth, "base", bf16)
    imgs = calc_ranges.batch_images(synth, B)
    out = _describe_batch(lcd, imgs)
    L, w, _ = calc_ranges.model(synth, "base")
    for b in range(B):
        alone, _ = lcd.calcDescrOriginalImg(imgs[b], blur_in_place=False)
        ref = calc_f64.forward_f64(L, w, oracle.calc_preproc(imgs[b])[0])[4]
        print("B %d image %d: batch vs alone %.2e, alone vs f64 %.2e" % (B, b, np.abs(out[b] - alone).max(), np.abs(alone - ref).max()))
        assert np.array_equal(out[b].view(np.uint32), alone.view(np.uint32)), (B, b, float(np.abs(out[b] - alone).max()))
        assert np.abs(out[b] - ref).max() < DESC_ATOL, (B, b)


ZERO_NORM_NEIGHBOURS = (79, 80)      # synth.random_image seeds whose conv3 map stays >= 2e-4 (normalised) away from the ReLU's kink: tests/test_calc_f64.py


@pytest.mark.parametrize("kernels", ["fused", "bf16x6", "generic"])
def test_zero_norm_is_the_oracles_division(api, oracle, synth, kernels):
    """A flat image empties the map of this model behind conv3's ReLU: the norm is zero and deeplcd.cpp:88 divides by it.  The oracle's f32
    division (0 / 0 = NaN in all 1064 places) is the contract, for every kernel family; in a batch the flat image's neighbours are untouched."""
    L, w = calc_ranges.zero_norm_model(synth)
    lcd = api.DeepLCD(w, layers=L)
    if kernels == "bf16x6":
        lcd.set_option(lcd.OPT_CONV2_BF16X6, 1)
    if kernels == "generic":
        lcd.set_option(lcd.OPT_GENERIC_KERNELS, 1)
    assert lcd.conv2_products() == {"fused": 3, "bf16x6": 6, "generic": 0}[kernels]
    ins = calc_ranges.inputs(synth)
    for name in ("zeros", "ones"):
        ref = oracle.calc_forward_net(L, w, ins[name])
        assert np.isnan(ref).all()
        got = lcd.debug_forward(ins[name], 4)
        assert np.allclose(got, ref, rtol=0, atol=DESC_ATOL, equal_nan=True), (name, got[:4])
    ref = calc_f64.forward_f64(L, w, ins["u8"])[4]
    assert np.abs(lcd.debug_forward(ins["u8"], 4) - ref).max() < DESC_ATOL          # the same handle still describes a textured image
    imgs = [synth.random_image(ZERO_NORM_NEIGHBOURS[0], 120, 160), np.full((120, 160), 255, np.uint8), synth.random_image(ZERO_NORM_NEIGHBOURS[1], 120, 160)]
    out = _describe_batch(lcd, imgs)
    for b in range(3):
        alone, _ = lcd.calcDescrOriginalImg(imgs[b], blur_in_place=False)
        oref = oracle.calc_forward_net(L, w, oracle.calc_preproc(imgs[b])[0])
        assert np.isnan(oref).all() == (b == 1)
        assert np.array_equal(out[b].view(np.uint32), alone.view(np.uint32)) or (b == 1 and np.isnan(out[b]).all() and np.isnan(alone).all()), b
        assert np.allclose(out[b], oref, rtol=0, atol=DESC_ATOL, equal_nan=True), b
