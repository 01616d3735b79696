"""Novel views at arbitrary camera poses on the GPU (ops.render_poses / pd_render_poses, predict.render_poses) against the oracle
on the CPU, against the product's other routes, and for what must hold whatever the numbers are.

Oracle, per view (``_view_oracle``): ``oracle.decoder_tail`` (its logits / sigma; skipped for ``tail_applied``),
``oracle.homography_matrices`` in fp64 rounded once to fp32 and pinned through ``oracle.homography_grid(H_t2s=, Rn=)`` — the
operator's contract: it forms its matrices in fp64 and rounds once — then ``oracle.plane_sweep`` of the image and of a ones
image, and ``(probability_rec * disp_n).sum(1)`` with ``disp_n(x,y) = max(a x + b y + c, 0)``, ``(a,b,c) = 0.1 * 0.58 * W *
(K^-1)^T n_t / d_t`` (0 for ``d_t <= 0``).  It runs twice, in fp64 (``exact``) and in fp32 (``ref32``: the reference's
arithmetic), on the exactly widened inputs for bf16 conv outputs.  ``visible_only`` has its own composite (``_composite``):
``logit_rec = -inf`` where the mask is off, every output 0 where no plane is visible.

1. Parity: ``cases.three_way(got, ref32, exact, factor=2, tol=1e-4, cap=cases.FWD_CAP)`` for rgb, coverage and disp — the suite's
   bar for homography forwards.  No pixel is excluded.
2. Condition of the inputs, asserted on the CPU: the fp32 and fp64 oracle masks agree at every (view, plane, pixel), and in fp64
   ``|facing|`` and ``|z - 1e-7|`` stay clear of 0 by 1e-4 of their scale — the sum of the absolute values of the terms each is
   the sum of, which is what an fp32 evaluation's rounding error is relative to (about 1e-7 of it per term: the margin leaves three
   orders of magnitude).  The seeds in ``CONFIGS`` were picked so that this holds; a case that sat on a horizon line would compare
   two legitimate answers.  The xz cases use an off-centre crop window: with a centred K and a centred grid, row H/2 has facing == 0
   exactly for xz planes under the identity and stereo poses.
3. Cross-route, xy-plane cases: the stereo pose against ``ops.render_views(baselines=[1.0])`` (each side's bound against its own
   oracle — FWD_CAP here, 1e-4 there — plus the distance between the two fp64 oracles, which the test computes), and against the
   training route (``ops.decoder_tail`` + ``ops.plane_sweep_homography``'s forward with the image as target): 2 * FWD_CAP.
4. Invariants: the identity pose returns the image to 1e-4 with coverage 1 where every plane's fp64 mask is on; coverage in
   [0, 1 + 1e-6]; disp >= 0; a record that is not invertible (n = (0,0,1), R = I, t_z = -d exactly) masks its plane and leaves
   finite outputs.
5. Bits: a view alone equals the same view among four and among seven; a repeated call is bit-identical; NaN-prefilled outputs
   are fully written; with coverage / disp NULL rgb is unchanged.
6. Memory: peak allocated bytes of a call stay below outputs + workspace + a quarter of one plane tensor.

Shapes (B,N,H,W): (2,5,8,16) one partial workgroup per view, two images; (1,3,3,5) and (1,4,13,22) odd sizes; (1,2,5,300) several
workgroups per view, the last one partial; (1,1,4,8) N = 1, where the forward move masks every plane; (1,9,24,80) xy only, and
with 4 xz planes and a row mask; (2,7,16,48) with 3 xz planes.  Poses per case: identity, the dataset's stereo T,
small_pose(rot=0.02, trans=0.05), small_pose(rot=0.1, trans=0.3) and a forward move t = (0.03, 0, -0.5), which puts the nearest
planes behind the camera (d_t < 0)."""
import itertools

import pytest
import torch

import cases
import planedepth_amd
from cases import rel_err
from oracle import planedepth_oracle as oracle
from planedepth_amd import _capi as C
from planedepth_amd import decoder_tail as DT
from planedepth_amd import ops
from planedepth_amd import synthetic

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF = torch.bfloat16
F64 = torch.float64
MARGIN = 1e-4         # 2.: |facing|, |z - 1e-7| against their scale
RV_TOL = 1e-4         # tests/test_render_views.py's bound of render_views against its own oracle

# (shape, xz planes, seed): the seed draws the inputs and the two random poses (2.: picked so that the condition holds)
CONFIGS = [((2, 5, 8, 16), 0, 0), ((1, 3, 3, 5), 0, 0), ((1, 4, 13, 22), 0, 0), ((1, 2, 5, 300), 0, 0), ((1, 1, 4, 8), 0, 0),
           ((1, 9, 24, 80), 0, 0), ((1, 9, 24, 80), 4, 0), ((2, 7, 16, 48), 3, 0)]
POSES = ("identity", "stereo", "small", "large", "forward")


def _poses(g, B):
    fwd = torch.eye(4)[None].repeat(B, 1, 1)
    fwd[:, 0, 3], fwd[:, 2, 3] = 0.03, -0.5
    return torch.stack([torch.eye(4)[None].repeat(B, 1, 1), synthetic.small_pose(g, B, stereo=True),
                        synthetic.small_pose(g, B, rot=0.02, trans=0.05), synthetic.small_pose(g, B, rot=0.1, trans=0.3), fwd], 1)


def _case(shape, n_xz, seed, mix, bf16, applied):
    """The inputs of one case: what the operator gets (device) and the dense fp32 CPU tensors the oracle reads.  Conv outputs,
    image and the xy planes' disparities as tests/test_render_views.py::_case draws them."""
    B, N, H, W = shape
    g = torch.Generator().manual_seed(sum(shape) + 17 * n_xz + 1000 * seed)
    rl = torch.randn(B, N, H, W, generator=g) * 2.5
    rs = torch.randn(B, N, H, W, generator=g) * 3 - 1
    rs.view(-1)[0::7] = -12.0    # sigmoid = 6e-6: clamped to 0.01
    rs.view(-1)[2::11] = 30.0    # sigmoid = 1.0 exactly: on the upper bound
    image = torch.rand(B, 3, H, W, generator=g)
    n_xy = N - n_xz
    lv = torch.arange(n_xy, dtype=torch.float32)[None] + 0.5 * (torch.rand(B, n_xy, generator=g) - 0.5)
    disp_xy = 0.47 * W * (2.0 / 300.0) ** (lv.clamp_min(0.0) / max(n_xy - 1, 1))           # decreasing with the plane index
    distance = 0.1 * 0.58 * W / disp_xy
    norm = torch.tensor([0.0, 0.0, 1.0])[None, None].expand(B, n_xy, 3)
    mrows = torch.ones(B, N, H)
    if n_xz:   # ground planes as the decoder makes them, on an off-centre crop window of a larger frame
        grid = synthetic.crop_grid(H, W, 3 * H + 5, 2 * W + 3, H - 3, W // 3)[None].expand(B, -1, -1, -1)
        geo = synthetic.decoder_plane_geometry(grid, torch.zeros(B, 2 + n_xz), no_levels=2, xz_levels=n_xz, rows=True)
        distance = torch.cat([distance, geo["distance"][:, 2:]], 1)
        norm = torch.cat([norm, geo["norm"][:, 2:]], 1)
        mrows[:, n_xy:] = geo["padding_mask"][:, 2:, :, 0]
    distance, norm = distance.contiguous(), norm.contiguous()
    dense_pm = mrows[..., None].expand(B, N, H, W).contiguous()
    if applied:   # logits / sigma as a tail wrote them
        rl, rs = rl * dense_pm, torch.clamp(torch.sigmoid(rs), 0.01, 1.0)
    if bf16:
        rl, rs = rl.to(BF), rs.to(BF)
    K, inv_K = synthetic.dataset_intrinsics(B, H, W)
    T = _poses(g, B)
    pm = ops.row_view(mrows.to(DEV), W) if n_xz else None
    dev = lambda t: t.to(DEV)  # noqa: E731
    return dict(shape=shape, n_xz=n_xz, mix=mix, applied=applied, rl=dev(rl), rs=dev(rs) if mix else None, pm=pm,
                distance=dev(distance), norm=dev(norm), image=dev(image), T=dev(T), K=dev(K), inv_K=dev(inv_K), disp_xy=disp_xy,
                cpu=dict(rl=rl.float(), rs=rs.float(), pm=dense_pm, distance=distance, norm=norm, image=image, T=T, K=K, inv_K=inv_K))


def _ex(M, N):
    return M[:, None].expand(-1, N, -1, -1).reshape(-1, 4, 4)   # trainer.py:557-559


def _tail(c, shape, mix, applied, dt):
    """logits, sigma [B,N,H,W] in ``dt``: the tail's, or the inputs as they are."""
    rl, rs, pm = c["rl"].to(dt), c["rs"].to(dt), c["pm"].to(dt)
    if applied:
        return rl, (rs if mix else None)
    tail = oracle.decoder_tail(rl, rs, pm, torch.ones_like(rl), shape[3], mix)
    return tail["logits"], tail.get("sigma")


def _composite(image, logits, sigma, grid, mask, mix):
    """PD_RENDER_VISIBLE_ONLY: trainer.py:567-603 with logit_rec = -inf where the mask is off; (rgb, ones composite, prob)."""
    B, N, H, W = logits.shape
    chans = [image[:, None].expand(-1, N, -1, -1, -1).reshape(B * N, 3, H, W), torch.ones(B * N, 1, H, W, dtype=logits.dtype),
             logits.reshape(B * N, 1, H, W)] + ([sigma.reshape(B * N, 1, H, W)] if mix else [])
    rec = oracle.bilinear_sample(torch.cat(chans, 1), grid, "zeros").reshape(B, N, -1, H, W) * mask.to(logits.dtype)
    on = mask[:, :, 0]
    seen = on.any(1, keepdim=True)
    logit_rec = torch.where(on, rec[:, :, 4], torch.full_like(rec[:, :, 4], float("-inf")))
    prob = torch.softmax(torch.where(seen, logit_rec, torch.zeros_like(logit_rec)), 1) * seen   # (no NaN rows from all -inf)
    prob = torch.where(on, prob, torch.zeros_like(prob))
    if mix:
        w = prob / rec[:, :, 5].clamp(0.01, 1.0)
        prob = w / torch.where(seen, w.sum(1, True), torch.ones_like(w[:, :1]))
    return (rec[:, :, :3] * prob[:, :, None]).sum(1), (rec[:, :, 3] * prob).sum(1, True), prob


def _disp_planes(c, T, shape, dt):
    """disp_n(x,y) [B,N,H,W] in ``dt``: the plane's inverse depth in the new camera as a rig disparity."""
    B, N, H, W = shape
    d, n, Ki = c["distance"].to(dt), c["norm"].to(dt), c["inv_K"].to(dt)[:, :3, :3]
    R, t = T.to(dt)[:, :3, :3], T.to(dt)[:, :3, 3]
    nt = torch.einsum("bij,bnj->bni", R, n)
    d_t = d + (nt * t[:, None]).sum(-1)
    coef = (0.1 * 0.58 * W) * torch.einsum("bji,bnj->bni", Ki, nt) / d_t[..., None]
    coef = torch.where(d_t[..., None] > 0, coef, torch.zeros_like(coef))
    ys, xs = torch.meshgrid(torch.arange(H, dtype=dt), torch.arange(W, dtype=dt), indexing="ij")
    plane = coef[..., 0, None, None] * xs + coef[..., 1, None, None] * ys + coef[..., 2, None, None]
    return plane.clamp_min(0.0)


def _view_oracle(case, v, dt, visible):
    """(rgb [B,3,H,W], coverage [B,1,H,W], disp [B,1,H,W], mask bool [B,N,1,H,W], margins) of view ``v`` in ``dt``."""
    c, shape, mix = case["cpu"], case["shape"], case["mix"]
    B, N, H, W = shape
    T = c["T"][:, v]
    f = lambda t: t.to(dt)  # noqa: E731
    H64, Rn64 = oracle.homography_matrices(c["distance"].double(), c["norm"].double(), _ex(T.double(), N),
                                           _ex(c["K"].double(), N), _ex(c["inv_K"].double(), N))
    H32, Rn32 = H64.float(), Rn64.float().reshape(B * N, 3)            # fp64, rounded once
    grid, mask = oracle.homography_grid(f(c["distance"]), f(c["norm"]), _ex(f(T), N), _ex(f(c["K"]), N), _ex(f(c["inv_K"]), N),
                                        H, W, H_t2s=f(H32), Rn=f(Rn32))
    logits, sigma = _tail(c, shape, mix, case["applied"], dt)
    image = f(c["image"])
    if visible:
        rgb, cov, prob = _composite(image, logits, sigma, grid, mask, mix)
    else:
        out = oracle.plane_sweep(image, logits, sigma, grid, mask, use_mixture_loss=mix)
        ones = oracle.plane_sweep(torch.ones_like(image), logits, sigma, grid, mask, use_mixture_loss=mix)
        rgb, cov, prob = out["rgb_rec"], ones["rgb_rec"][:, :1], out["probability_rec"]
    disp = (prob * _disp_planes(c, T, shape, dt)).sum(1, True)
    margins = None
    if dt == F64:   # 2.: how far facing and z - 1e-7 stay from 0, in units of the terms they are sums of
        ys, xs = torch.meshgrid(torch.arange(H, dtype=F64), torch.arange(W, dtype=F64), indexing="ij")
        pix = torch.stack([xs.reshape(-1), ys.reshape(-1), torch.ones(H * W, dtype=F64)], 0)[None]            # [1,3,HW]
        h2 = H32.double()[:, 2, :, None]                                                                        # [BN,3,1]
        z, z_scale = (h2 * pix).sum(1), (h2 * pix).abs().sum(1)
        terms = torch.matmul(_ex(c["inv_K"].double(), N)[:, :3, :3], pix) * Rn32.double()[:, :, None]
        facing, f_scale = terms.sum(1), terms.abs().sum(1)
        margins = (float((facing.abs() / f_scale).min()), float(((z - 1e-7).abs() / z_scale).min()))
    return rgb, cov, disp, mask, margins


def _render(case, T=None, visible=False, want=("coverage", "disp")):
    with torch.no_grad():
        return ops.render_poses(case["rl"], case["rs"], case["pm"], case["distance"], case["norm"], case["image"],
                                case["T"] if T is None else T, case["K"], case["inv_K"], use_mixture_loss=case["mix"],
                                tail_applied=case["applied"], visible_only=visible, want=want)


def _xy_disp_layered(case):
    B, N, H, W = case["shape"]
    return case["disp_xy"].to(DEV)[:, :, None, None].expand(B, N, H, W)


def _training_route(case, v):
    """rgb_rec of the product's training route for pose ``v``: decoder_tail under no_grad, then the homography sweep's forward
    with the source image standing in as target (on the widened inputs for bf16 conv outputs, as tests/test_render_views.py)."""
    rl = case["rl"].float()
    rs = None if case["rs"] is None else case["rs"].float()
    with torch.no_grad():
        if case["applied"]:
            logits, sigma = rl, rs
        else:
            logits, sigma, _, _, _ = ops.decoder_tail(rl, rs, case["pm"], _xy_disp_layered(case), use_mixture_loss=case["mix"])
        return ops.plane_sweep_homography(case["image"], case["image"], logits, sigma, case["distance"], case["norm"],
                                          case["T"][:, v].contiguous(), case["K"], case["inv_K"], use_mixture_loss=case["mix"])[0]


def _variants():
    for (shape, n_xz, seed), mix, bf16, applied in itertools.product(CONFIGS, (True, False), (False, True), (False, True)):
        yield pytest.param(shape, n_xz, seed, mix, bf16, applied,
                           id="%s-%s-%s-%s-%s" % ("x".join(map(str, shape)), "xz%d" % n_xz if n_xz else "xy", "mix" if mix else "pi",
                                                  "bf16" if bf16 else "fp32", "applied" if applied else "raw"))


@pytest.mark.parametrize("shape,n_xz,seed,mix,bf16,applied", list(_variants()))
def test_render_poses(shape, n_xz, seed, mix, bf16, applied):
    B, N, H, W = shape
    case = _case(shape, n_xz, seed, mix, bf16, applied)
    c = case["cpu"]
    V = len(POSES)
    got = {False: _render(case), True: _render(case, visible=True)}
    for res in got.values():
        assert res.rgb.shape == (B, V, 3, H, W) and res.coverage.shape == res.disp.shape == (B, V, 1, H, W)
        for t in res:
            assert t.dtype == torch.float32 and not t.requires_grad and bool(torch.isfinite(t).all())
        # 4. invariants
        assert float(res.coverage.min()) >= 0.0 and float(res.coverage.max()) <= 1.0 + 1e-6
        assert float(res.disp.min()) >= 0.0
    exact64 = {}
    for v, name in enumerate(POSES):
        for visible in (False, True):
            exact = _view_oracle(case, v, F64, visible)
            ref32 = _view_oracle(case, v, torch.float32, visible)
            exact64[v, visible] = exact
            # 2. the condition of the inputs
            assert torch.equal(exact[3], ref32[3]), (name, "the fp32 and fp64 oracle masks differ")
            f_margin, z_margin = exact[4]
            print("%s: margins facing %.3g z %.3g" % (name, f_margin, z_margin))
            assert f_margin >= MARGIN and z_margin >= MARGIN, (name, f_margin, z_margin)
            # 1. parity
            res = got[visible]
            for key, g, r32, r64 in (("rgb", res.rgb[:, v], ref32[0], exact[0]), ("coverage", res.coverage[:, v], ref32[1], exact[1]),
                                     ("disp", res.disp[:, v], ref32[2], exact[2])):
                ok, e_got, e_ref = cases.three_way(g.cpu(), r32, r64, factor=2, tol=1e-4, cap=cases.FWD_CAP)
                print("PARITY %s%s %s: vs fp64 %.3g (the oracle's fp32 %.3g)" % (name, " visible_only" if visible else "", key, e_got, e_ref))
                assert ok, (name, visible, key, e_got, e_ref)
            if visible:   # a pixel no plane reaches is exactly 0 in every output
                unseen = ~exact[3][:, :, 0].any(1, keepdim=True)
                for t in (res.rgb[:, v], res.coverage[:, v], res.disp[:, v]):
                    assert float((t.cpu().abs() * unseen).max()) == 0.0
    if POSES[4] == "forward" and shape == (1, 1, 4, 8):
        assert not bool(exact64[4, False][3].any())      # the forward move masks every plane there
    # 4. the identity pose is the source camera, where no plane is masked
    clear = exact64[0, False][3][:, :, 0].all(1, keepdim=True)          # [B,1,H,W]
    for res in got.values():
        err_img = float(((res.rgb[:, 0].cpu() - c["image"]).abs() * clear).max())
        err_cov = float(((res.coverage[:, 0].cpu() - 1.0).abs() * clear).max())
        print("identity: rgb vs image %.3g, |coverage - 1| %.3g on %d pixels" % (err_img, err_cov, int(clear.sum())))
        assert err_img <= 1e-4 and err_cov <= 1e-4
    # 3. cross-route
    if not n_xz:
        res, exact = got[False], exact64[1, False]
        dl = _xy_disp_layered(case)
        with torch.no_grad():
            other = ops.render_views(case["rl"], case["rs"], None, dl, case["image"], [1.0], use_mixture_loss=mix, tail_applied=applied)
        logits, sigma = _tail(c, shape, mix, applied, F64)
        dl64 = dl.cpu().double()
        grid = oracle.disp_grid(dl64, "r")
        ones_mask = torch.ones(B, N, 1, H, W, dtype=F64)
        out = oracle.plane_sweep(c["image"].double(), logits, sigma, grid, ones_mask, use_mixture_loss=mix)
        ones = oracle.plane_sweep(torch.ones_like(c["image"]).double(), logits, sigma, grid, ones_mask, use_mixture_loss=mix)
        exact_rv = (out["rgb_rec"], ones["rgb_rec"][:, :1], (out["probability_rec"] * dl64).sum(1, True))
        for key, a, b, ea, eb in zip(("rgb", "coverage", "disp"), (res.rgb, res.coverage, res.disp), other, exact, exact_rv):
            between = rel_err(ea, eb)
            err = rel_err(a[:, 1].cpu(), b[:, 0].cpu())
            print("CROSS stereo %s: vs render_views %.3g (the two fp64 oracles %.3g apart)" % (key, err, between))
            assert err <= cases.FWD_CAP + RV_TOL + between, (key, err, between)
        for v, name in enumerate(POSES):
            err = rel_err(res.rgb[:, v], _training_route(case, v))
            print("CROSS %s: vs decoder_tail + plane_sweep_homography %.3g" % (name, err))
            assert err <= 2 * cases.FWD_CAP, (name, err)
    # 5. bits: alone, among four, among seven; a repeated call
    T = case["T"]
    four = T[:, [3, 0, 2, 4]].contiguous()
    seven = T[:, [4, 1, 2, 2, 0, 3, 1]].contiguous()
    for visible in (False, True):
        all5, r4, r7 = got[visible], _render(case, four, visible), _render(case, seven, visible)
        for v in range(V):
            alone = _render(case, T[:, v:v + 1].contiguous(), visible)
            for a, b in zip(alone, all5):
                assert torch.equal(a[:, 0], b[:, v]), (v, visible)
        for a, b, cc in zip(all5, r4, r7):
            for v, at4, at7 in ((3, 0, 5), (0, 1, 4), (2, 2, 2), (4, 3, 0)):
                assert torch.equal(a[:, v], b[:, at4]) and torch.equal(a[:, v], cc[:, at7]), (v, visible)
            assert torch.equal(cc[:, 2], cc[:, 3]) and torch.equal(cc[:, 1], cc[:, 6])
        for a, b in zip(all5, _render(case, visible=visible)):
            assert torch.equal(a, b)
    # [V,4,4] is the same pose set for every image
    if B > 1:
        shared = T[0].contiguous()
        for a, bb in zip(_render(case, shared), _render(case, shared[None].expand(B, -1, -1, -1).contiguous())):
            assert torch.equal(a, bb)


def test_records_are_the_matrices_of_the_training_route():
    """The record a view is rendered from holds H_t2s and R n bit for bit as pd_homography_matrices_fwd(PD_HMAT_PLANES) writes
    them for that pose, (a, b, c) as the fp64 formula rounded once, and the validity word."""
    shape = B, N, H, W = (2, 7, 16, 48)
    case = _case(shape, 3, 0, True, False, False)
    V = len(POSES)
    ws = torch.full((int(C.load().pd_render_poses_workspace_floats(B, N, V)),), float("nan"), device=DEV)
    assert ws.numel() == 16 * B * V * N
    new = lambda ch: torch.empty(B, V, ch, H, W, device=DEV)  # noqa: E731
    C.call("pd_render_poses", ws.device, B, N, H, W, V, C.PD_TAIL_MIXTURE, case["rl"], case["rs"], None, case["distance"], case["norm"],
           case["T"], case["K"], case["inv_K"], case["image"], new(3), None, None, ws)
    rec = ws.view(B, V, N, 16)
    assert not torch.isnan(rec).any()
    c = case["cpu"]
    for v in range(V):
        with torch.no_grad():
            Hm, Rn = ops.homography_matrices_fused(case["distance"], case["norm"], case["T"][:, v].contiguous(), case["K"], case["inv_K"])
        assert torch.equal(rec[:, v, :, :9], Hm.reshape(B, N, 9)), POSES[v]
        assert torch.equal(rec[:, v, :, 9:12], Rn.reshape(B, N, 3)), POSES[v]
        assert bool((rec[:, v, :, 15] == 1.0).all())
        T = c["T"][:, v].double()
        nt = torch.einsum("bij,bnj->bni", T[:, :3, :3], c["norm"].double())
        d_t = c["distance"].double() + (nt * T[:, None, :3, 3]).sum(-1)
        coef = (0.1 * 0.58 * W) * torch.einsum("bji,bnj->bni", c["inv_K"].double()[:, :3, :3], nt) / d_t[..., None]
        coef = torch.where(d_t[..., None] > 0, coef, torch.zeros_like(coef))
        got = rec[:, v, :, 12:15].cpu().double()
        # rounded once from fp64: half an ulp of fp32 (2^-24 relative), plus the fp64 evaluation orders' difference
        assert bool(((got - coef).abs() <= 2.0 ** -23 * coef.abs() + 1e-30).all()), POSES[v]


def test_a_record_that_is_not_invertible_masks_its_plane():
    """4. n = (0,0,1), R = I, t_z = -d exactly: d_t = 0, the new camera's centre lies on plane 0.  The reference's torch.inverse
    fails there; the record is invalid, the plane masked everywhere: with visible_only the view is, bit for bit, the view
    rendered without that plane, and the default mode's outputs are finite."""
    shape = B, N, H, W = (2, 5, 8, 16)
    for mix, applied in itertools.product((True, False), (False, True)):
        case = _case(shape, 0, 0, mix, False, applied)
        T = torch.eye(4, device=DEV)[None, None].repeat(B, 1, 1, 1)
        T[:, 0, 0, 3] = 0.03
        T[:, 0, 2, 3] = -case["distance"][:, 0]
        ws = torch.empty(16 * B * N, device=DEV)
        new = lambda ch: torch.full((B, 1, ch, H, W), float("nan"), device=DEV)  # noqa: E731
        flags = (C.PD_TAIL_MIXTURE if mix else 0) | (C.PD_RENDER_TAIL_APPLIED if applied else 0)
        rgb, cov, disp = new(3), new(1), new(1)
        C.call("pd_render_poses", ws.device, B, N, H, W, 1, flags, case["rl"], case["rs"], None, case["distance"], case["norm"], T,
               case["K"], case["inv_K"], case["image"], rgb, cov, disp, ws)
        rec = ws.view(B, 1, N, 16)
        assert bool((rec[:, 0, 0, 15] == 0.0).all()) and bool((rec[:, 0, 1:, 15] == 1.0).all())
        assert bool((rec[:, 0, 0, 12:15] == 0.0).all())
        for t in (rgb, cov, disp):
            assert bool(torch.isfinite(t).all())
        seen = _render(case, T, visible=True)
        rest = dict(case, rl=case["rl"][:, 1:].contiguous(), rs=case["rs"][:, 1:].contiguous() if mix else None,
                    distance=case["distance"][:, 1:].contiguous(), norm=case["norm"][:, 1:].contiguous())
        for a, b in zip(seen, _render(rest, T, visible=True)):
            assert bool(torch.isfinite(a).all()) and torch.equal(a, b)


@pytest.mark.parametrize("n_xz", [0, 4], ids=["xy", "xz4"])
def test_every_output_element_is_written(n_xz):
    """5. The C entry called directly on NaN-filled outputs; with coverage and disp NULL only rgb is written (and is the same)."""
    shape = B, N, H, W = (1, 9, 24, 80)
    case = _case(shape, n_xz, 0, True, False, False)
    V = len(POSES)
    flags = C.PD_TAIL_MIXTURE | (C.PD_TAIL_MASK_ROWS if n_xz else 0)
    pm = case["pm"][..., 0].contiguous() if n_xz else None
    ws = torch.empty(16 * B * V * N, device=DEV)
    nan = lambda ch: torch.full((B, V, ch, H, W), float("nan"), device=DEV)   # noqa: E731
    args = (case["rl"], case["rs"], pm, case["distance"], case["norm"], case["T"], case["K"], case["inv_K"], case["image"])
    rgb, coverage, disp = nan(3), nan(1), nan(1)
    C.call("pd_render_poses", ws.device, B, N, H, W, V, flags, *args, rgb, coverage, disp, ws)
    for t in (rgb, coverage, disp):
        assert not torch.isnan(t).any()
    only = nan(3)
    C.call("pd_render_poses", ws.device, B, N, H, W, V, flags, *args, only, None, None, ws)
    assert torch.equal(only, rgb)
    res = _render(case, want=())
    assert res.coverage is None and res.disp is None and torch.equal(res.rgb, rgb)
    assert _render(case, want="disp").coverage is None


def test_nothing_plane_sized_is_allocated():
    """6. Peak memory of the call beyond what was allocated before it: the outputs, the workspace and nothing plane-sized (less
    than a quarter of one [B,N,H,W] fp32 tensor on top of them); the training route under no_grad, which writes logits and
    sigma, is above a plane tensor — the probe sees the difference."""
    B, N, H, W = shape = (2, 9, 24, 80)
    plane_bytes = B * N * H * W * 4
    case = _case(shape, 0, 0, True, False, False)
    V = len(POSES)

    def peak(fn):
        torch.cuda.synchronize()
        before = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        with torch.no_grad():
            out = fn()
        torch.cuda.synchronize()
        return torch.cuda.max_memory_allocated() - before, out

    _render(case)   # (the first call's one-time allocations are not the operator's)
    fused, res = peak(lambda: _render(case))
    out_bytes = sum(t.numel() * t.element_size() for t in res)
    ws_bytes = 16 * B * V * N * 4
    train, _ = peak(lambda: _training_route(case, 2))
    print("peak bytes beyond the inputs: render_poses %d (outputs %d, workspace %d), training route %d, one plane tensor %d"
          % (fused, out_bytes, ws_bytes, train, plane_bytes))
    assert out_bytes == B * V * 5 * H * W * 4
    assert fused - out_bytes - ws_bytes < plane_bytes // 4
    assert train > plane_bytes


class _Net(torch.nn.Module):
    """encoder + decoder stand-in that fills the outputs dict as the decoders do.  ``tail``: "keep" = the inference tail with
    ``keep_conv_outputs=True``, "stock" = the reference's torch tail."""
    NO_LEVELS, XZ_LEVELS = 5, 3

    def __init__(self, tail, mix=True, seed=1):
        super().__init__()
        n = self.NO_LEVELS + self.XZ_LEVELS
        self.tail, self.mix = tail, mix
        self.body = torch.nn.Conv2d(3, 12, 3, padding=1)
        self.dispconv = torch.nn.Conv2d(12, n, 3, padding=1)
        self.sigmaconv = torch.nn.Conv2d(12, n, 3, padding=1)
        g = torch.Generator().manual_seed(seed)
        with torch.no_grad():
            for p in self.parameters():
                p.copy_(torch.randn(p.shape, generator=g) * (0.5 if p.dim() > 1 else 0.1))
        self.outputs = None

    def forward(self, x, grids):
        outputs = {}
        f = torch.relu(self.body(x))
        DT.fused_plane_geometry(outputs, grids, None, no_levels=self.NO_LEVELS, xz_levels=self.XZ_LEVELS, disp_min=0.5,
                                disp_max=20.0, xz_min=0.1852, xz_max=0.3704)
        raw_logits, raw_sigma = self.dispconv(f), self.sigmaconv(f)
        if self.tail == "stock":      # networks/depth_decoder.py:256-291
            mask, dl = outputs["padding_mask"], outputs["disp_layered"]
            outputs["logits"] = logits = raw_logits * mask
            prob = torch.softmax(logits.float(), 1)
            if self.mix:
                outputs["sigma"] = sigma = torch.clamp(torch.sigmoid(raw_sigma), 0.01, 1.0)
                weights = prob / sigma.float() * mask
                prob = weights / weights.sum(1, True)
            outputs["probability"] = prob
            outputs["disp"] = (prob * dl).sum(1, True)
        else:
            DT.fused_decoder_tail_inference(outputs, raw_logits, raw_sigma if self.mix else None, use_mixture_loss=self.mix,
                                            keep_conv_outputs=True)
        self.outputs = outputs
        return outputs


@pytest.mark.parametrize("mix", [True, False], ids=["mix", "pi"])
@pytest.mark.parametrize("autocast", [False, True], ids=["fp32", "autocast"])
def test_predict_render_poses(mix, autocast):
    """predict.render_poses against render_poses called directly, from the kept conv outputs and from a stock tail's logits /
    sigma; K / inv_K default to the dataset's intrinsics."""
    M, H, W = 2, 16, 48
    g = torch.Generator().manual_seed(4)
    images = torch.rand(M, 3, H, W, generator=g).to(DEV)
    poses = _poses(g, M)[:, 1:4].to(DEV)
    K, inv_K = (t.to(DEV) for t in synthetic.dataset_intrinsics(M, H, W))
    keep, stock = (_Net(t, mix).to(DEV).eval() for t in ("keep", "stock"))

    views, pred = planedepth_amd.predict.render_poses(keep, images, poses, autocast=autocast, visible_only=True)
    out = keep.outputs
    assert out["raw_logits"].dtype == (BF if autocast else torch.float32)
    with torch.no_grad():
        direct = ops.render_poses(out["raw_logits"], out.get("raw_sigma"), out["padding_mask"], out["distance"], out["norm"], images,
                                  poses, K, inv_K, use_mixture_loss=mix, visible_only=True)
    for a, b in zip(views, direct):
        assert a.shape[:2] == (M, 3) and torch.equal(a, b)
    for a, b in zip(pred, planedepth_amd.predict(keep, images, autocast=autocast)):
        assert torch.equal(a, b)

    views_s, pred_s = planedepth_amd.predict.render_poses(stock, images, poses[0], K, inv_K, autocast=autocast)
    so = stock.outputs
    lg, sg = so["logits"], so.get("sigma")
    if mix and autocast:   # logits * mask is fp32, sigma bf16: both are widened
        lg, sg = lg.float(), sg.float()
    with torch.no_grad():
        direct_s = ops.render_poses(lg, sg, None, so["distance"], so["norm"], images, poses[0], K, inv_K, use_mixture_loss=mix,
                                    tail_applied=True)
    for a, b in zip(views_s, direct_s):
        assert torch.equal(a, b)
    assert torch.equal(pred_s.raw_disp, so["disp"][:, 0])
    if not autocast:   # fp32: the stock tail's logits / sigma are the kept conv outputs after the tail step
        raw_s = planedepth_amd.predict.render_poses(keep, images, poses[0], K, inv_K)[0]
        assert rel_err(views_s.rgb, raw_s.rgb) < 2 * cases.FWD_CAP
