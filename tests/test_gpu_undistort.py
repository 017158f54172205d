"""Lens undistortion on the device (csrc/undistort.hip, myslam_undistort_*): Camera::UndistortImage (reference src/camera.cpp:36-48) as
Frontend::GrabStereoImage runs it when Camera.bNeedUndistortion is 1 (src/frontend.cpp:47-51).  Every map and every output byte equals the
numpy restatement tests/undistort_ref.py."""
import numpy as np
import pytest

import undistort_ref as U

pytestmark = pytest.mark.gpu

KITTI_K = (718.856, 718.856, 607.1928, 185.2157)
COEFFS = {"zero": (0.0, 0.0, 0.0, 0.0), "mild": (-0.05, 0.01, 1e-4, -5e-5), "strong": (-0.28, 0.07, 2e-4, 2e-5)}
SIZES = [(376, 1241, KITTI_K), (240, 720, (458.654, 457.296, 367.215, 120.375)), (121, 333, (300.5, 301.25, 170.3, 60.7))]


def _remap_batch(imgs, xy, frac):
    """tests/undistort_ref.remap over a leading batch axis"""
    B, H, W = imgs.shape
    sx = xy[..., 0].astype(np.int64); sy = xy[..., 1].astype(np.int64)
    fx = (frac & 31).astype(np.int64); fy = ((frac >> 5) & 31).astype(np.int64)
    acc = np.zeros((B, H, W), np.int64)
    for dx, dy, w in ((0, 0, (32 - fx) * (32 - fy)), (1, 0, fx * (32 - fy)), (0, 1, (32 - fx) * fy), (1, 1, fx * fy)):
        x, y = sx + dx, sy + dy
        ok = (x >= 0) & (x < W) & (y >= 0) & (y < H)
        acc += np.where(ok, imgs[:, np.clip(y, 0, H - 1), np.clip(x, 0, W - 1)].astype(np.int64), 0) * (w * 32)
    return ((acc + 16384) >> 15).astype(np.uint8)


@pytest.mark.parametrize("coef", list(COEFFS))
@pytest.mark.parametrize("size", range(len(SIZES)))
def test_get_map_equals_the_restatement(api, coef, size):
    rows, cols, K = SIZES[size]
    u = api.Undistorter(rows, cols, K, COEFFS[coef])
    xy, frac = u.get_map()
    rxy, rfrac = U.undistort_maps(rows, cols, K, COEFFS[coef])
    assert np.array_equal(xy, rxy) and np.array_equal(frac, rfrac)
    if coef == "zero":
        assert not frac.any()


@pytest.mark.parametrize("coef", list(COEFFS))
@pytest.mark.parametrize("size", range(len(SIZES)))
def test_undistort_image_is_byte_identical(api, synth, coef, size):
    rows, cols, K = SIZES[size]
    u = api.Undistorter(rows, cols, K, COEFFS[coef])
    img = synth.random_image(31 + size, rows, cols)
    got = u.UndistortImage(img)
    ref = U.undistort(img, K, COEFFS[coef])
    assert np.array_equal(got, ref)
    if coef == "zero":
        assert np.array_equal(got, img)
    # padded pitches on both sides: the bytes between the destination's rows stay as they were
    src = np.full((rows, cols + 13), 7, np.uint8); src[:, :cols] = img
    dst = np.full((rows, cols + 5), 0xAB, np.uint8)
    u.UndistortImage(src[:, :cols], dst[:, :cols])
    assert np.array_equal(dst[:, :cols], ref) and (dst[:, cols:] == 0xAB).all()
    # in place, as the reference calls it (cv::undistort(img, img, ...))
    inplace = img.copy()
    u.UndistortImage(inplace, inplace)
    assert np.array_equal(inplace, ref)


@pytest.mark.parametrize("batch", [1, 2, 1024])
def test_batch_is_byte_identical(api, synth, batch):
    import torch
    rows, cols = (376, 1241) if batch < 1024 else (96, 160)
    K = KITTI_K if batch < 1024 else (140.0, 141.0, 80.5, 47.25)
    D = COEFFS["strong"]
    u = api.Undistorter(rows, cols, K, D)
    rng = np.random.default_rng(batch)
    imgs = rng.integers(0, 256, (batch, rows, cols), dtype=np.uint8)
    if batch < 1024:
        imgs = np.stack([synth.random_image(50 + b, rows, cols) for b in range(batch)])
    xy, frac = U.undistort_maps(rows, cols, K, D)
    ref = _remap_batch(imgs, xy, frac)
    d_src = torch.from_numpy(imgs).cuda()
    d_dst = torch.zeros_like(d_src)
    u.batch(d_src.data_ptr(), batch, cols, rows * cols, d_dst.data_ptr(), cols, rows * cols)
    torch.cuda.synchronize()
    assert np.array_equal(d_dst.cpu().numpy(), ref)


@pytest.mark.parametrize("pitch", [(1241 + 13, 1241 + 3, 77, 5), (1248, 1248, 0, 0), (1244, 1250, 4, 32)])
def test_batch_padded_steps_and_strides(api, synth, pitch):
    import torch
    rows, cols, B = 376, 1241, 3
    sstep, dstep, sgap, dgap = pitch
    sstride, dstride = rows * sstep + sgap, rows * dstep + dgap
    u = api.Undistorter(rows, cols, KITTI_K, COEFFS["strong"])
    imgs = [synth.random_image(70 + b, rows, cols) for b in range(B)]
    src = np.full(B * sstride, 9, np.uint8)
    for b in range(B):
        src[b * sstride:b * sstride + rows * sstep].reshape(rows, sstep)[:, :cols] = imgs[b]
    d_src = torch.from_numpy(src).cuda()
    d_dst = torch.full((B * dstride,), 0xAB, dtype=torch.uint8, device="cuda")
    u.batch(d_src.data_ptr(), B, sstep, sstride, d_dst.data_ptr(), dstep, dstride)
    torch.cuda.synchronize()
    out = d_dst.cpu().numpy()
    touched = np.zeros(B * dstride, bool)
    for b in range(B):
        view = out[b * dstride:b * dstride + rows * dstep].reshape(rows, dstep)
        assert np.array_equal(view[:, :cols], U.undistort(imgs[b], KITTI_K, COEFFS["strong"]))
        touched[b * dstride:b * dstride + rows * dstep].reshape(rows, dstep)[:, :cols] = True
    assert (out[~touched] == 0xAB).all(), "bytes outside the output images were written"


def test_batch_refuses_overlapping_buffers(api):
    import torch
    rows, cols = 120, 200
    u = api.Undistorter(rows, cols, (150.0, 150.0, 100.0, 60.0), COEFFS["mild"])
    buf = torch.zeros(3 * rows * cols, dtype=torch.uint8, device="cuda")
    p = buf.data_ptr()
    for dst in (p, p + rows * cols - 1, p + 5):
        with pytest.raises(api.MyslamError) as e:
            u.batch(p, 2, cols, rows * cols, dst, cols, rows * cols)
        assert e.value.code == api.ERR_INVALID
    u.batch(p, 1, cols, rows * cols, p + rows * cols, cols, rows * cols)      # adjacent is fine
    with pytest.raises(api.MyslamError):
        u.batch(p, 2, cols, rows * cols, p + rows * cols, cols, rows * cols)     # image 1 of the source is image 0 of the output
    torch.cuda.synchronize()


def test_recorded_graph_replay_equals_the_eager_call(api, synth):
    import torch
    rows, cols, B = 376, 1241, 4
    s = torch.cuda.Stream()
    u = api.Undistorter(rows, cols, KITTI_K, COEFFS["strong"], stream=s.cuda_stream)
    imgs = np.stack([synth.random_image(90 + b, rows, cols) for b in range(B)])
    d_src = torch.from_numpy(imgs).cuda()
    d_dst = torch.zeros_like(d_src)
    torch.cuda.synchronize()
    body = lambda: u.batch(d_src.data_ptr(), B, cols, rows * cols, d_dst.data_ptr(), cols, rows * cols)
    body(); s.synchronize()
    eager = d_dst.cpu().numpy()
    assert np.array_equal(eager, _remap_batch(imgs, *U.undistort_maps(rows, cols, KITTI_K, COEFFS["strong"])))
    g = api.StepGraph.record(s.cuda_stream, [], body)
    d_dst.zero_(); torch.cuda.synchronize()
    g.launch(s.cuda_stream); s.synchronize()
    assert np.array_equal(d_dst.cpu().numpy(), eager)


# ---- the switch in the system: a corridor drive seen through distorting lenses ------------------------------------------------------------
SEQ_N = 200
D_RIGHT = (-0.27, 0.065, 1e-4, -3e-5)


def _distortion_cfg(on, D_left, D_right):
    import kitti_layout
    cfg = kitti_layout.parse_yaml(kitti_layout.KITTI00_02_YAML)
    cfg["Camera.bNeedUndistortion"] = 1 if on else 0
    for side, D in (("left", D_left), ("right", D_right)):
        for n, v in zip(("k1", "k2", "p1", "p2"), D):
            cfg[f"Camera.{side}.{n}"] = v
    return cfg


def _yaml(cfg):
    import kitti_layout
    lines = [l for l in kitti_layout.KITTI00_02_YAML.splitlines() if not l.startswith(("Camera.bNeedUndistortion", "Camera.left.k", "Camera.left.p",
                                                                                        "Camera.right.k", "Camera.right.p"))]
    lines += [f"{k}: {cfg[k]!r}" if isinstance(cfg[k], float) else f"{k}: {cfg[k]}" for k in cfg
              if k == "Camera.bNeedUndistortion" or k.split(".")[-1] in ("k1", "k2", "p1", "p2")]
    return "\n".join(lines) + "\n"


@pytest.fixture(scope="module")
def drive(synth):
    import kitti_layout
    scene = synth.corridor_scene()
    C, yaw = synth.corridor_poses(SEQ_N, 0.9)
    K = kitti_layout.camera(synth)
    distorted = [synth.render_corridor_stereo_distorted(scene, C[t], yaw[t], t, synth.EUROC_LIKE_D, D_RIGHT, K=K) for t in range(SEQ_N)]
    pinhole = [synth.render_corridor_stereo(scene, C[t], yaw[t], t, K=K) for t in range(SEQ_N)]
    return dict(distorted=distorted, pinhole=pinhole, C=C, yaw=yaw)


def _free_run(api, pkg, synth, cfg, frames):
    import kitti_layout
    chain = pkg.chain
    a = chain.Chain(chain.HipBackend(api, synth.calc_weights_handcrafted(), cfg), pkg.api, chain.camera_from_config(cfg), frames, cfg=cfg,
                    timestamps=[0.1 * t for t in range(len(frames))], log=False)
    n = 0
    for t in range(len(frames)):
        if not a.grab(t):
            break
        n += 1
    return a, n


def test_distorted_drive_lock_step_with_the_switch_on(api, oracle, synth, pkg, drive):
    """Camera.bNeedUndistortion = 1: Chain.grab undistorts both images first (frontend.cpp:47-51) — every undistort call equals the numpy
    restatement byte for byte, every other operator call meets its own parity bar against the oracle on the same (undistorted) inputs"""
    import kitti_layout
    from oracle_backend import CheckedBackend, OracleBackend
    chain = pkg.chain
    cfg = _distortion_cfg(True, synth.EUROC_LIKE_D, D_RIGHT)
    K = chain.camera_from_config(cfg)
    Kv = (K["fx"], K["fy"], K["cx"], K["cy"])

    class CheckedUndistortBackend(CheckedBackend):
        def undistort(self, img, which):
            got = self.h.undistort(img, which)
            assert np.array_equal(got, U.undistort(img, Kv, K["dist_right" if which else "dist_left"])), f"undistort #{self.calls.get('undistort', 0)}"
            self._note("undistort")
            return got

    w = synth.calc_weights_handcrafted()
    chk = CheckedUndistortBackend(chain.HipBackend(api, w, cfg), OracleBackend(oracle, w, cfg, chain))
    a = chain.Chain(chk, pkg.api, K, drive["distorted"], cfg=cfg, timestamps=[0.1 * t for t in range(SEQ_N)]).run()
    ninl = [int(x[2][0]) for t, x in a.log if t == "pose_only"]
    assert chk.calls["undistort"] == 2 * SEQ_N and len(ninl) == SEQ_N - 1 and min(ninl) > 10
    rmse, _ = kitti_layout.ate(chain, synth, a.poses, drive["C"], drive["yaw"])
    print(f"distorted drive, switch on, lock-step: {dict(chk.calls)}; ATE {rmse:.3f} m")


def test_switch_on_tracks_like_the_pinhole_drive_and_off_is_worse(api, synth, pkg, drive):
    """The undistorted drive tracks within 1.5 x the ATE of the same scene rendered pinhole; the same distorted frames with the switch off
    (distorted pixels taken for pinhole ones: what the product did before) are measurably worse — the distortion is strong enough to matter"""
    import kitti_layout
    chain = pkg.chain
    on, n_on = _free_run(api, pkg, synth, _distortion_cfg(True, synth.EUROC_LIKE_D, D_RIGHT), drive["distorted"])
    pin, n_pin = _free_run(api, pkg, synth, _distortion_cfg(False, synth.EUROC_LIKE_D, D_RIGHT), drive["pinhole"])
    off, n_off = _free_run(api, pkg, synth, _distortion_cfg(False, synth.EUROC_LIKE_D, D_RIGHT), drive["distorted"])
    assert n_on == n_pin == SEQ_N
    ate = lambda a: kitti_layout.ate(chain, synth, a.poses, drive["C"][:len(a.poses)], drive["yaw"][:len(a.poses)])[0]
    e_on, e_pin = ate(on), ate(pin)
    e_off = ate(off) if n_off == SEQ_N else float("inf")            # LOST before the end is worse than any ATE
    print(f"ATE over {SEQ_N} frames: pinhole {e_pin:.3f} m, distorted + undistortion {e_on:.3f} m, distorted without it {e_off:.3f} m ({n_off} frames tracked)")
    # measured on an MI355X (200 frames): pinhole 0.899 m, distorted + undistortion 1.242 m (1.38 x), distorted without it 1.979 m (1.59 x the
    # undistorted run).  The first bar is the proposed 1.5 x; the second asks for a clear gap below the measured one
    assert e_on <= 1.5 * e_pin + 1e-3
    assert e_off > 1.2 * max(e_on, e_pin)


def test_compiled_runner_equals_chain_with_the_switch_on(api, synth, pkg, drive, tmp_path):
    """bin/run_kitti_stereo reads Camera.bNeedUndistortion and the eight coefficients (StereoCamera::FromConfig) and undistorts in
    GrabStereoImage — the prefetched next left image once, reused as the next frame's left image: every frame pose and trajectory.txt equal
    chain.py's bit for bit"""
    import subprocess

    import kitti_layout
    import png_files
    chain = pkg.chain
    exe = pkg._build.build_app()
    frames = drive["distorted"]
    seq = tmp_path / "sequences" / "00"
    ts = kitti_layout.write(str(seq), frames, png_files)
    cfg = _distortion_cfg(True, synth.EUROC_LIKE_D, D_RIGHT)
    cfg_path = tmp_path / "distorted.yaml"; cfg_path.write_text(_yaml(cfg))
    assert chain.camera_from_config(kitti_layout.parse_yaml(cfg_path.read_text())) == chain.camera_from_config(cfg)
    w = np.ascontiguousarray(synth.calc_weights_handcrafted(), np.float32).ravel()
    wfile = tmp_path / "handcrafted.calcw"
    with open(wfile, "wb") as f:
        f.write(b"CALCW1\0\0"); f.write(np.uint64(w.size).tobytes()); f.write(w.tobytes())
    out = tmp_path / "cpp"
    r = subprocess.run([exe, str(cfg_path), str(seq), "--frames", str(len(frames)), "--out", str(out), "--calc-weights", str(wfile), "--frame-poses"],
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    a = chain.Chain(chain.HipBackend(api, w, cfg), pkg.api, chain.camera_from_config(cfg), frames, cfg=cfg, timestamps=ts, log=False).run()
    a.save(str(tmp_path / "py"))
    assert [int(x) for x in open(out / "key_frame_frames.txt").read().split()] == a.kf_frames
    poses = np.array([[float(x) for x in l.split()] for l in open(out / "frame_poses_cw.txt").read().strip().split("\n")])
    assert np.array_equal(poses, np.stack(a.poses)), float(np.abs(poses - np.stack(a.poses)).max())
    assert open(out / "trajectory.txt").read() == open(tmp_path / "py" / "trajectory.txt").read()
    print(f"compiled runner, distorted drive with the switch on: {r.stdout.strip().splitlines()[-1]}")
