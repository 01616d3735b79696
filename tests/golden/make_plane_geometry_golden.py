"""Generate tests/golden/plane_geometry.npz (the vectors of tests/test_plane_geometry.py) with the REFERENCE's own
``DepthDecoder.forward`` (networks/depth_decoder.py:147-291): its geometry head on cropped grids and its tail behind it.

Run where the reference tree is present:

    python tests/golden/make_plane_geometry_golden.py            # writes the fixture
    python tests/golden/make_plane_geometry_golden.py --check    # writes nothing: re-runs the reference against the committed file

Forward hooks replace what ``residualconv`` / ``dispconv`` / ``sigmaconv`` return by seeded leaf tensors (as
make_golden.decoder_tail_vectors does); a hook on the decoder's ``nn.Sigmoid`` keeps the first sigmoid's output, so that
``residual_levels = sigmoid(.) - 0.5`` and its gradient through the reference's whole dense chain (``g_residual``) are the
reference's own tensors.  Everything after the hooks is the reference's code.

Size.  The file has to stay far below the 1 MiB limit for committed files while the decoder accepts nothing smaller than 64x64,
so: the conv outputs are drawn on a grid of 1/8 and stored as int8 (``raw = int8 / 8``, exact in fp32), the upstream weights of
``logits`` / ``sigma`` are outer products ``plane[B,N,1,1] * pixel[B,1,H,W]`` stored as their factors, and the four
[B,N,H,W]-sized results (``logits``, ``sigma``, ``g_raw_logits``, ``g_raw_sigma``) are stored at every ``STRIDE``-th row and
column from (1, 2).  ``disp``, ``depth``, the geometry and ``g_residual`` — which sums over every pixel — are stored whole.
Only data is written.
"""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from ref_import import load_reference  # noqa: E402

from planedepth_amd.synthetic import crop_grid  # noqa: E402

OUT = os.path.join(HERE, "plane_geometry.npz")
H = W = 64        # smallest the decoder's five stride-2 levels accept
STRIDE, Y0, X0 = 4, 1, 2
CFG = dict(disp_min=2.0, disp_max=30.0, xz_min=0.1852, xz_max=0.3704)
# (full_w, full_h, w0, h0) per sample: crops with the horizon (y = 0) inside the window and off its centre
CROPS = [(200, 150, 30, 40), (160, 120, 70, 31)]
CASES = (
    ("xz_res", dict(no_levels=4, xz_levels=3, plane_residual=True, use_mixture_loss=True), 2),
    ("xz_nores", dict(no_levels=4, xz_levels=3, plane_residual=False, use_mixture_loss=True), 2),
    ("xy_res", dict(no_levels=5, xz_levels=0, plane_residual=True, use_mixture_loss=True), 1),
)


def sub(t):
    return t[..., Y0::STRIDE, X0::STRIDE]


def run_case(ref, kw, B, seed):
    g = torch.Generator().manual_seed(seed)
    torch.manual_seed(11)
    dec = ref.networks.DepthDecoder([64, 64, 128, 256, 512], use_denseaspp=False, disp_min=CFG["disp_min"],
                                    disp_max=CFG["disp_max"], xz_min=CFG["xz_min"], xz_max=CFG["xz_max"], **kw)
    N = kw["no_levels"] + kw["xz_levels"]
    feats = [torch.randn(B, c, H >> (i + 1), W >> (i + 1), generator=g) * 0.5 for i, c in enumerate([64, 64, 128, 256, 512])]
    q_logits = torch.clamp(torch.round(torch.randn(B, N, H, W, generator=g) * 3 * 8), -127, 127).to(torch.int8)
    q_sigma = torch.clamp(torch.round((torch.randn(B, N, H, W, generator=g) * 3.5 - 1.0) * 8), -127, 127).to(torch.int8)
    raw_logits = (q_logits.float() / 8).requires_grad_(True)
    raw_sigma = (q_sigma.float() / 8).requires_grad_(True)          # both clamp bounds of sigma are hit
    raw_residual = torch.randn(B, N, 1, 1, generator=g).requires_grad_(True)
    dec.convs["dispconv"].register_forward_hook(lambda m, i, o: raw_logits)
    dec.convs["sigmaconv"].register_forward_hook(lambda m, i, o: raw_sigma)
    sig_out = []

    def keep(m, i, o):
        if o.requires_grad:
            o.retain_grad()
        sig_out.append(o)
    dec.sigmoid.register_forward_hook(keep)
    if kw["plane_residual"]:
        dec.convs["residualconv"].register_forward_hook(lambda m, i, o: raw_residual)
    grid = torch.stack([crop_grid(H, W, fh, fw, h0, w0) for fw, fh, w0, h0 in CROPS[:B]], 0)
    o = dec(feats, grid)
    gw_plane_l, gw_plane_s = torch.randn(B, N, 1, 1, generator=g), torch.randn(B, N, 1, 1, generator=g)
    gw_pix_l, gw_pix_s = torch.randn(B, 1, H, W, generator=g), torch.randn(B, 1, H, W, generator=g)
    gw_d = torch.randn(B, 1, H, W, generator=g)
    gw_z = torch.randn(B, 1, H, W, generator=g) * 0.1
    gw_dist = torch.randn(B, N, generator=g)
    obj = ((o["logits"] * (gw_plane_l * gw_pix_l)).sum() + (o["sigma"] * (gw_plane_s * gw_pix_s)).sum()
           + (o["disp"] * gw_d).sum() + (o["depth"] * gw_z).sum() + (o["distance"] * gw_dist).sum())
    obj.backward()
    dl, pm = o["disp_layered"], o["padding_mask"].float().expand(B, N, H, W)
    assert bool((dl == dl[..., :1]).all()) and bool((pm == pm[..., :1]).all())   # constant along x: the row form loses nothing
    blob = dict(grid=grid, q_logits=q_logits, q_sigma=q_sigma, disp_rows=dl[..., 0], mask_rows=pm[..., 0],
                distance=o["distance"], norm=o["norm"].float(), logits=sub(o["logits"]), sigma=sub(o["sigma"]), disp=o["disp"],
                depth=o["depth"], gw_plane_logits=gw_plane_l, gw_plane_sigma=gw_plane_s, gw_pix_logits=gw_pix_l,
                gw_pix_sigma=gw_pix_s, gw_disp=gw_d, gw_depth=gw_z, gw_distance=gw_dist, g_raw_logits=sub(raw_logits.grad),
                g_raw_sigma=sub(raw_sigma.grad))
    if kw["plane_residual"]:
        s = sig_out[0]                                   # sigmoid(residualconv(x)): residual_levels = s - 0.5 (:151)
        blob.update(residual=(s - 0.5).reshape(B, N), g_residual=s.grad.reshape(B, N))
    return {k: v.detach().numpy() for k, v in blob.items()}


def main():
    ref = load_reference()
    out, meta = {}, dict(cfg=CFG, stride=[STRIDE, Y0, X0], cases={})
    for i, (tag, kw, B) in enumerate(CASES):
        seed = 5150 if tag.startswith("xz") else 5151      # the two xz cases share their inputs
        blob = run_case(ref, kw, B, seed)
        inputs_of = tag
        if tag == "xz_nores":                              # the same draws as xz_res (no residual drawn after them is used):
            inputs_of = "xz_res"                           # the shared inputs are stored once
            for k in ("grid", "q_logits", "q_sigma"):
                assert np.array_equal(blob[k], out["xz_res/" + k]), k
                del blob[k]
        out.update({"%s/%s" % (tag, k): v for k, v in blob.items()})
        meta["cases"][tag] = dict(B=B, H=H, W=W, inputs_of=inputs_of, **kw)
        print("%-9s disp mean %.5f  masked rows %d" % (tag, float(blob["disp"].mean()), int((blob["mask_rows"] == 0).sum())))
    if "--check" in sys.argv:
        z = np.load(OUT)
        assert json.loads(str(z["meta"])) == meta, "meta differs"
        for k, v in out.items():
            err = float(np.abs(z[k].astype(np.float64) - v.astype(np.float64)).max() / max(np.abs(v).max(), 1e-30))
            assert err < 1e-5, (k, err)
        print("plane_geometry.npz agrees with the reference on this host")
        return
    np.savez_compressed(OUT, meta=np.asarray(json.dumps(meta)), **out)
    print("wrote %s (%d bytes)" % (OUT, os.path.getsize(OUT)))


if __name__ == "__main__":
    main()
