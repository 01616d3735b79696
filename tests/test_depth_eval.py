"""Depth evaluation on the device (planedepth_amd.metrics, csrc/pd_depth_eval.hip) against a numpy / torch restatement of
its contract and against tests/golden/depth_eval.npz, which tests/golden/make_eval_golden.py produced with the reference's
own compute_errors, batch_post_process_disparity, layers.compute_depth_errors and Trainer.compute_depth_losses.

The restatement below is the executable form of the contract in metrics.py (steps A1-A9, B1-B5)."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import GOLDEN, ROOT

F32 = np.float32
EIGEN_CROP = (0.40810811, 0.99189189, 0.03594771, 0.96405229)
CONFIGS = [(pp, mono, split) for pp in (False, True) for mono in (True, False) for split in ("eigen_raw", "odom_9")]


def config_name(pp, mono, split):
    return "pp%d_%s_%s" % (pp, "mono" if mono else "stereo", split)


# ---- restatement: offline evaluation (A) --------------------------------------------------------------------------------
def cv2_resize(src, H, W):
    """A2: cv2.resize(src, (W, H)) INTER_LINEAR on fp32, as OpenCV 4's coefficient setup and resizeGeneric_ state it."""
    h, w = src.shape
    fx = ((np.arange(W) + 0.5) * (1.0 / (W / w)) - 0.5).astype(F32)
    sx = np.floor(fx).astype(np.int64)
    ax = fx - sx.astype(F32)
    left = sx < 0
    sx[left], ax[left] = 0, 0
    one_tap = sx >= w - 1
    sx[one_tap], ax[one_tap] = w - 1, 0
    sx1 = np.minimum(sx + 1, w - 1)
    fy = ((np.arange(H) + 0.5) * (1.0 / (H / h)) - 0.5).astype(F32)
    sy = np.floor(fy).astype(np.int64)
    ay = (fy - sy.astype(F32))[:, None]
    r0, r1 = np.clip(sy, 0, h - 1), np.clip(sy + 1, 0, h - 1)
    with np.errstate(invalid="ignore", over="ignore"):
        rows = src[:, sx] * (F32(1) - ax)
        rows = np.where(one_tap, rows, rows + src[:, sx1] * ax)
        return rows[r0] * (F32(1) - ay) + rows[r1] * ay


def post_process(l_disp, r_disp):
    """A1 for one image: r_disp is the mirrored pass as the network returned it (not flipped back yet)."""
    return F32(0.5) * (l_disp + r_disp[:, ::-1])


def eval_mask(gt, split):
    """A4: (valid mask, gt after the clamp) of one GT map."""
    if split in ("eigen_raw", "eigen_improved"):
        H, W = gt.shape
        g = gt.copy()
        g[g < F32(1e-3)] = F32(1e-3)
        g[g > F32(80)] = F32(80)
        crop = np.array([EIGEN_CROP[0] * H, EIGEN_CROP[1] * H, EIGEN_CROP[2] * W, EIGEN_CROP[3] * W]).astype(np.int32)
        inside = np.zeros(gt.shape, bool)
        inside[crop[0]:crop[1], crop[2]:crop[3]] = True
        return (g > F32(1e-3)) & (g < F32(80)) & inside, g
    return gt > 0, gt


def depth_pairs(disp_small, gt, *, width, split, scale_factor):
    """A2-A5 for one image: (gt_valid, depth_valid) fp32, and the resized disparity."""
    disp = cv2_resize(disp_small, *gt.shape)
    with np.errstate(divide="ignore", invalid="ignore"):
        depth = F32(0.1 * 0.58 * width) / disp
    mask, g = eval_mask(gt, split)
    d = depth[mask] * F32(scale_factor)
    return g[mask], d, disp


def np_median(v):
    return F32(np.median(v)) if v.size else F32(np.nan)


def finish(gt_v, d, ratio):
    """A6 (given the ratio) and A7."""
    d = d * F32(ratio)
    d[d < F32(1e-3)] = F32(1e-3)
    d[d > F32(80)] = F32(80)
    return d


def error_terms(g, d):
    """The fp32 terms of compute_errors / compute_depth_errors and their fp64 sums -> (metrics fp64 [7], counts [4])."""
    with np.errstate(divide="ignore", invalid="ignore"):
        thresh = np.maximum(g / d, d / g)
        e = g - d
        e2 = e * e
        le = np.log(g.astype(np.float64)).astype(F32) - np.log(d.astype(np.float64)).astype(F32)
        n = np.float64(g.size)   # (an empty set: 0/0 = NaN everywhere, as numpy's mean of nothing)
        hits = [int((thresh < F32(1.25 ** k)).sum()) for k in (1, 2, 3)]
        s = [np.sum((np.abs(e) / g).astype(np.float64)), np.sum((e2 / g).astype(np.float64)), np.sum(e2.astype(np.float64)),
             np.sum((le * le).astype(np.float64))]
        m = np.array([s[0] / n, s[1] / n, np.sqrt(s[2] / n), np.sqrt(s[3] / n)] + [h / n for h in hits])
    return m, np.array([g.size] + hits)


def restate_eval(preds, gts, *, width, split, pp, mono):
    """Steps A1-A8 for every image -> dict of per-image arrays (metrics fp64, ratio, medians, counts) + the resized maps."""
    M = len(gts)
    scale = 1.0 if mono else 5.4
    out = {"metrics": [], "ratio": [], "med": [], "counts": [], "resized": []}
    for i in range(M):
        src = post_process(preds[i], preds[i + M]) if pp else preds[i]
        g, d, disp = depth_pairs(src, gts[i], width=width, split=split, scale_factor=scale)
        if mono:
            mg, md = np_median(g), np_median(d)
            with np.errstate(divide="ignore", invalid="ignore"):
                ratio = mg / md
        else:
            mg = md = F32(np.nan)
            ratio = F32(1)
        m, c = error_terms(g, finish(g, d, ratio))
        for k, v in (("metrics", m), ("ratio", ratio), ("med", (mg, md)), ("counts", c), ("resized", disp)):
            out[k].append(v)
    return {k: (v if k == "resized" else np.array(v)) for k, v in out.items()}


# ---- restatement: trainer metrics (B), in torch on the host ---------------------------------------------------------------
def restate_trainer(depth, grid, gt, no_stereo):
    depth, grid, gt = (torch.as_tensor(x) for x in (depth, grid, gt))
    d = torch.clamp(depth * 2.0 / (grid[:, 0:1, :, -1:] - grid[:, 0:1, :, 0:1]), 1e-3, 80)
    _, _, H, W = gt.shape
    crop = torch.zeros_like(gt, dtype=torch.bool)
    crop[:, :, int(EIGEN_CROP[0] * H):int(EIGEN_CROP[1] * H), int(EIGEN_CROP[2] * W):int(EIGEN_CROP[3] * W)] = True
    mask = (gt > 0) & crop
    g, d = torch.clamp(gt[mask], 1e-3, 80), d[mask]
    med = (torch.median(g), torch.median(d)) if no_stereo else (torch.tensor(np.nan), torch.tensor(np.nan))
    ratio = (med[0] / med[1]) if no_stereo else torch.tensor(F32(5.4))
    d = d * ratio
    m, c = error_terms(g.numpy(), d.numpy())
    return {"metrics": m, "ratio": F32(ratio), "med": np.array([F32(med[0]), F32(med[1])]), "counts": c}


# ---- fixture ----------------------------------------------------------------------------------------------------------
def load_fixture():
    z = np.load(os.path.join(GOLDEN, "depth_eval.npz"))
    fx = {k: z[k] for k in z.files}
    gts = []
    for i, (h, w) in enumerate(fx["a_gt_shapes"]):
        g = np.zeros(h * w, F32)
        lo, hi = fx["a_gt_ptr"][i], fx["a_gt_ptr"][i + 1]
        g[fx["a_gt_idx"][lo:hi]] = fx["a_gt_val"][lo:hi]
        gts.append(g.reshape(h, w))
    fx["gts"] = gts
    return fx


def same_nan(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.array_equal(np.isnan(a), np.isnan(b))


def test_restatement_reproduces_fixture():
    fx = load_fixture()
    for pp, mono, split in CONFIGS:
        c = config_name(pp, mono, split)
        r = restate_eval(fx["a_pred"], fx["gts"], width=int(fx["a_width"]), split=split, pp=pp, mono=mono)
        assert np.array_equal(r["counts"], fx["A__%s__counts" % c]), c
        assert np.array_equal(r["ratio"].astype(F32), fx["A__%s__ratio" % c], equal_nan=True), c
        assert np.array_equal(r["med"].astype(F32), fx["A__%s__med" % c], equal_nan=True), c
        want = fx["A__%s__metrics" % c]
        assert same_nan(r["metrics"], want), c
        ok = ~np.isnan(want)
        assert np.allclose(r["metrics"][ok], want[ok], rtol=1e-5, atol=0), c
    for ns in (0, 1):
        r = restate_trainer(fx["b_depth"], fx["b_grid"], fx["b_gt"], bool(ns))
        assert np.array_equal(r["counts"], fx["B__%d__counts" % ns])
        assert r["ratio"] == fx["B__%d__ratio" % ns]
        assert np.array_equal(r["med"], fx["B__%d__med" % ns], equal_nan=True)
        assert np.allclose(r["metrics"], fx["B__%d__metrics" % ns], rtol=1e-5, atol=0)


def test_fixture_covers_the_contract_cases():
    fx = load_fixture()
    shapes = [tuple(s) for s in fx["a_gt_shapes"]]
    assert (375, 1242) in shapes and len(set(shapes)) > 2                      # ragged, one full-size image
    vals = np.concatenate([g.ravel() for g in fx["gts"]])
    assert (vals * 256 == np.round(vals * 256)).mean() > 0.99                  # KITTI-like 1/256 steps: the medians hit ties
    assert (vals == F32(1e-3)).any() and (vals == F32(80)).any() and (vals > 80).any() and (vals == 0).any()
    n = fx["A__pp0_mono_eigen_raw__counts"][:, 0]
    assert (n == 0).any() and (n % 2 == 1).any() and (n[n > 0] % 2 == 0).any()   # empty, odd and even sets
    assert np.isnan(fx["A__pp0_mono_eigen_raw__ratio"]).any()                    # a NaN in a median's set
    assert (fx["a_pred"] == 0).any()                                            # zero disparity -> infinite depth
    assert fx["B__1__counts"][0] % 2 == 0                                       # the pooled lower median differs from numpy's


def test_restatement_matches_live_reference():
    sys.path.insert(0, GOLDEN)
    from ref_import import reference_available
    if not reference_available():
        pytest.skip("reference tree not present")
    from make_eval_golden import reference_outputs
    fx = load_fixture()
    live = reference_outputs(fx)
    for k, v in live.items():
        assert np.array_equal(np.asarray(v), fx[k], equal_nan=True), k


def test_eval_entry_points_validate_without_gpu():
    from planedepth_amd import _capi as C
    lib = C.load()
    P = [None] * 8
    assert lib.pd_depth_eval(2, 8, 8, C.PD_EVAL_EIGEN, 1, 1.0, 1.0, None, None, 0, *P) == 1
    assert b"NULL" in lib.pd_last_error()
    assert lib.pd_depth_eval(0, 8, 8, 0, 1, 1.0, 1.0, None, None, 0, *P) == 1
    assert b"shape" in lib.pd_last_error()
    assert lib.pd_depth_eval(2, 8, 8, 0, 0, 1.0, 1.0, None, None, 0, *P) == 1
    assert b"max_tiles" in lib.pd_last_error()
    assert lib.pd_depth_eval(2, 8, 8, 16, 1, 1.0, 1.0, None, None, 0, *P) == 1
    assert b"flags" in lib.pd_last_error()
    assert lib.pd_depth_eval(2, 8, 8, C.PD_EVAL_TRAINER | C.PD_EVAL_POST_PROCESS, 1, 1.0, 1.0, None, None, 0, *P) == 1
    assert b"flags" in lib.pd_last_error()
    fake = ctypes.c_void_p(16)   # never dereferenced: the grid check comes before any launch
    assert lib.pd_depth_eval(2, 8, 8, C.PD_EVAL_TRAINER, 1, 1.0, 1.0, fake, None, 0, fake, fake, fake, fake, fake, fake,
                             fake, None) == 1
    assert b"grid" in lib.pd_last_error()
    assert lib.pd_depth_eval_resize(2, 8, 8, C.PD_EVAL_EIGEN, 64, None, None, None, None) == 1
    assert b"flags" in lib.pd_last_error()
    assert lib.pd_depth_eval_resize(2, 8, 8, 0, 64, None, None, None, None) == 1
    assert b"NULL" in lib.pd_last_error()
    assert lib.pd_depth_eval_workspace_bytes(2, 1, 32) == 0
    tiles = 3
    assert lib.pd_depth_eval_workspace_bytes(4, tiles, C.PD_EVAL_MEDIAN) >= 4 * tiles * C.PD_EVAL_TILE * 8


def test_ops_reexport_the_evaluation():
    from planedepth_amd import ops, trainer_path
    import planedepth_amd
    assert ops.eval_depth_errors is planedepth_amd.metrics.eval_depth_errors
    class T:
        pass
    planedepth_amd.patch_trainer_metrics(T)
    assert T.compute_depth_losses is trainer_path.compute_depth_losses
    with pytest.raises(Exception):
        ops.eval_depth_errors(torch.zeros(1, 4, 4), [np.ones((8, 8), F32)], width=640)   # CPU tensors: no fallback


# ---- GPU ---------------------------------------------------------------------------------------------------------------
gpu = pytest.mark.gpu


def _cuda(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def _check_against(res, r, want_metrics, tag):
    """Exact medians / ratios / counts; metrics within 2e-6 of the fp64 sums of the same fp32 terms and 1e-5 of the fixture."""
    got = {k: getattr(res, k).cpu().numpy() for k in ("metrics", "ratio", "medians", "counts")}
    assert np.array_equal(got["counts"], r["counts"].reshape(got["counts"].shape)), tag
    assert np.array_equal(got["ratio"], np.asarray(r["ratio"], F32).reshape(got["ratio"].shape), equal_nan=True), tag
    assert np.array_equal(got["medians"], np.asarray(r["med"], F32).reshape(got["medians"].shape), equal_nan=True), tag
    m = got["metrics"].astype(np.float64)
    ref = np.asarray(r["metrics"]).reshape(m.shape)
    want_metrics = np.asarray(want_metrics).reshape(m.shape)
    assert same_nan(m, ref) and same_nan(m, want_metrics), tag
    ok = ~np.isnan(ref)
    assert np.allclose(m[ok], ref[ok], rtol=2e-6, atol=0), (tag, np.abs(m[ok] / ref[ok] - 1).max())
    assert np.allclose(m[ok], want_metrics[ok], rtol=1e-5, atol=1e-7), tag


@gpu
@pytest.mark.parametrize("pp", [False, True])
def test_resize_is_bit_identical_to_the_restatement(pp):
    from planedepth_amd import metrics
    fx = load_fixture()
    M = len(fx["gts"])
    got = metrics.resize_disp(_cuda(fx["a_pred"] if pp else fx["a_pred"][:M]), [_cuda(g) for g in fx["gts"]], post_process=pp)
    for i, g in enumerate(fx["gts"]):
        src = post_process(fx["a_pred"][i], fx["a_pred"][i + M]) if pp else fx["a_pred"][i]
        want = cv2_resize(src, *g.shape)
        have = got[i].cpu().numpy()
        assert np.array_equal(have.view(np.uint32), want.view(np.uint32)) or np.array_equal(have, want, equal_nan=True), i


@gpu
@pytest.mark.parametrize("pp,mono,split", CONFIGS, ids=[config_name(*c) for c in CONFIGS])
def test_eval_matches_fixture(pp, mono, split):
    from planedepth_amd import metrics
    fx = load_fixture()
    M = len(fx["gts"])
    width = int(fx["a_width"])
    pred = _cuda(fx["a_pred"] if pp else fx["a_pred"][:M])
    res = metrics.eval_depth_errors(pred, fx["gts"], width=width, split=split, post_process=pp, median_scaling=mono,
                                    scale_factor=1.0 if mono else 5.4)
    r = restate_eval(fx["a_pred"], fx["gts"], width=width, split=split, pp=pp, mono=mono)
    c = config_name(pp, mono, split)
    _check_against(res, r, fx["A__%s__metrics" % c], c)
    # the split summary (A9) over the images with a finite row (an empty set or a NaN makes the reference's mean NaN)
    clean = int(fx["a_clean"])
    res = metrics.eval_depth_errors(_cuda(np.concatenate([fx["a_pred"][:clean], fx["a_pred"][M:M + clean]]) if pp else
                                          fx["a_pred"][:clean]), fx["gts"][:clean], width=width, split=split, post_process=pp,
                                    median_scaling=mono, scale_factor=1.0 if mono else 5.4)
    s = metrics.summarize(res, median_scaling=mono)
    assert np.allclose(s["mean_errors"], fx["A__%s__summary" % c], rtol=1e-5, atol=0), c
    if mono:
        assert np.allclose([s["ratio_med"], s["ratio_std"]], fx["A__%s__ratio_stats" % c], rtol=1e-6, atol=0), c


def _eigen_split(n, seed, h=192, w=640):
    """n full-size GT maps in the Eigen size mix (~5 % LiDAR-like valid points, quantised to 1/256) + [n,h,w] disparities."""
    rng = np.random.default_rng(seed)
    sizes = [(375, 1242), (370, 1224), (374, 1238), (376, 1241)]
    gts = []
    for i in range(n):
        H, W = sizes[i % 4]
        g = np.zeros((H, W), F32)
        keep = rng.random((H, W)) < 0.05
        g[keep] = (np.round(rng.uniform(2, 85, keep.sum()) * 256) / 256).astype(F32)
        gts.append(g)
    preds = rng.uniform(1, 60, (n, h, w)).astype(F32)
    return preds, gts


@gpu
def test_full_size_ragged_split_matches_the_restatement():
    from planedepth_amd import metrics
    preds, gts = _eigen_split(32, 3)
    res = metrics.eval_depth_errors(_cuda(preds), gts, width=640, split="eigen_raw")
    r = restate_eval(preds, gts, width=640, split="eigen_raw", pp=False, mono=True)
    _check_against(res, r, r["metrics"], "32 full-size images")


@gpu
def test_two_launches_are_bit_identical_and_follow_the_current_stream():
    from planedepth_amd import metrics
    preds, gts = _eigen_split(8, 4)
    packed = metrics.pack_gt(gts, "eigen_raw")
    pred = _cuda(preds)
    a = metrics.eval_depth_errors(pred, packed, width=640)
    b = metrics.eval_depth_errors(pred, packed, width=640)
    for x, y in zip(a, b):
        assert torch.equal(x.view(torch.int32) if x.dtype == torch.float32 else x,
                           y.view(torch.int32) if y.dtype == torch.float32 else y)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        torch.cuda._sleep(50_000_000)        # the input below is written late on this stream
        late = pred * 1.0
        c = metrics.eval_depth_errors(late, packed, width=640)
    side.synchronize()
    for x, y in zip(a, c):
        assert torch.equal(x, y) or torch.equal(x.isnan(), y.isnan())


def _stub_trainer(no_stereo):
    import types
    import planedepth_amd

    class Stub:
        depth_metric_names = ["de/abs_rel", "de/sq_rel", "de/rms", "de/log_rms", "da/a1", "da/a2", "da/a3"]

        def __init__(self):
            self.opt = types.SimpleNamespace(no_stereo=no_stereo)
    planedepth_amd.patch_trainer_metrics(Stub)
    return Stub()


@gpu
@pytest.mark.parametrize("no_stereo", [False, True])
def test_trainer_metrics_match_fixture(no_stereo):
    fx = load_fixture()
    inputs = {"grid": _cuda(fx["b_grid"]), ("depth_gt", "l"): _cuda(fx["b_gt"])}
    losses = _stub_trainer(no_stereo).compute_depth_losses(inputs, {"depth": _cuda(fx["b_depth"])})
    got = np.array([float(losses[k]) for k in _stub_trainer(no_stereo).depth_metric_names])
    assert all(losses[k].dim() == 0 and losses[k].is_cuda for k in losses)
    want = fx["B__%d__metrics" % no_stereo]
    assert np.allclose(got, want, rtol=1e-5, atol=0), (got, want)
    from planedepth_amd import metrics
    res = metrics.trainer_depth_metrics(inputs[("depth_gt", "l")] * 0 + _cuda(fx["b_depth"]), inputs["grid"],
                                        inputs[("depth_gt", "l")], no_stereo=no_stereo)
    r = restate_trainer(fx["b_depth"], fx["b_grid"], fx["b_gt"], no_stereo)
    _check_against(res, r, want, "trainer no_stereo=%d" % no_stereo)


@gpu
def test_trainer_metrics_refuse_mismatched_shapes():
    t = _stub_trainer(True)
    inputs = {"grid": torch.zeros(2, 2, 40, 128, device="cuda"), ("depth_gt", "l"): torch.ones(2, 1, 375, 1242, device="cuda")}
    with pytest.raises(ValueError):
        t.compute_depth_losses(inputs, {"depth": torch.ones(2, 1, 40, 128, device="cuda")})


@gpu
def test_no_host_sync():
    from planedepth_amd import metrics
    preds, gts = _eigen_split(4, 5)
    packed = metrics.pack_gt(gts, "eigen_raw")
    pred = _cuda(preds)
    depth, grid, gt = (torch.rand(2, 1, 48, 160, device="cuda") + 1, torch.rand(2, 2, 48, 160, device="cuda"),
                       torch.rand(2, 1, 48, 160, device="cuda") * 10)
    torch.cuda.synchronize()
    metrics._TRAINER_META.clear()
    torch.cuda.set_sync_debug_mode("error")
    try:
        with pytest.raises(RuntimeError):   # the mode reports on this build: a deliberate sync is caught
            pred.sum().item()
        metrics.eval_depth_errors(pred, packed, width=640)
        metrics.eval_depth_errors(pred, packed, width=640, median_scaling=False, scale_factor=5.4)
        _stub_trainer(True).compute_depth_losses({"grid": grid, ("depth_gt", "l"): gt}, {"depth": depth})
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()


@gpu
@pytest.mark.parametrize("mono", [True, False])
def test_cli_prints_the_fixture_numbers(tmp_path, mono):
    fx = load_fixture()
    M = int(fx["a_clean"])
    np.save(tmp_path / "disps.npy", fx["a_pred"][:M])
    gt = np.empty(M, dtype=object)
    for i, g in enumerate(fx["gts"][:M]):
        gt[i] = g
    np.savez(tmp_path / "gt_depths.npz", data=gt)
    out = subprocess.run([sys.executable, "-m", "planedepth_amd.evaluate", "--ext_disp_to_eval", str(tmp_path / "disps.npy"),
                          "--gt_path", str(tmp_path / "gt_depths.npz"), "--eval_mono" if mono else "--eval_stereo",
                          "--width", str(int(fx["a_width"]))], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    c = config_name(False, mono, "eigen_raw")
    row = ("&{: 8.5f}  " * 7).format(*fx["A__%s__summary" % c].tolist()) + "\\\\"
    assert row in out.stdout, (row, out.stdout)
    if mono:
        med, std = fx["A__%s__ratio_stats" % c]
        assert " Scaling ratios | med: {:0.3f} | std: {:0.3f}".format(med, std) in out.stdout, out.stdout
