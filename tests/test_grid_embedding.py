"""The fused grid embedding pyramid (planedepth_amd/embedding.py, pd_grid_embed.hip): the decoders' positional encoding of
inputs["grid"] — ``epconv`` / ``Embedder`` / the raw grid, resampled to every decoder level — forward and backward.

CPU: the reference-made fixture (tests/golden/grid_embedding.npz, made by tests/golden/make_embedding_golden.py) against the fp64
restatement of tests/embedding_cases.py and against the live reference, the conditions the per-element inputs must meet, header <->
ctypes table <-> library, every refusal of the entry points, the workspace's closed form, the module dispatch's refusals.  GPU
(``-m gpu``): the kernels per element against fp64 for the three kinds and every padded channel count, the backward per parameter and
bit for bit across runs, the workload shape, the exact cases of the identity kind, the reference fixture through
``fused_grid_embedding``, write extents, the stream and autograd through a consuming convolution."""
import copy
import ctypes
import functools
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import capi_header
from conftest import GOLDEN
from embedding_cases import (DECODER_LEVELS, HIDDEN, LEVELS, SMALL, WORKLOAD, allowance, crop_grids, epconv_module, fixture_weights,
                             level_gradients, load_fixture, make_weights, negative_shares, pyramid_and_gradients_fp64, pyramid_fp64,
                             torch_pyramid)
from planedepth_amd import _capi as C
from planedepth_amd import embedding, ops

CHANNELS = (1, 2, 8, 16)     # neural E: the three padded instantiations (4, 8, 16), and the two-pass backward
MULTIRES = 3


def n_params(E):
    return 3 * HIDDEN + E * (HIDDEN + 1)


# ---------------------------------------------------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------------------------------------------------
def test_fixture_covers_the_contract_cases():
    meta, arrays = load_fixture()
    cases = meta["cases"]
    assert set(cases) == {"decoder", "pose", "frequency", "identity"}
    assert (meta["B"], meta["H"], meta["W"]) == (2, 32, 64)
    assert cases["decoder"]["sizes"] == [[1, 2], [2, 4], [4, 8], [8, 16], [16, 32]] and cases["decoder"]["E"] == 8
    assert cases["pose"]["sizes"] == [[1, 2]] and cases["pose"]["E"] == 8
    assert cases["frequency"]["E"] == 10 and cases["frequency"]["multires"] == 2 and cases["identity"]["E"] == 2
    grid = torch.from_numpy(arrays["grid"])
    flipped = grid[:1].clone()
    flipped[:, 0] *= -1.
    assert torch.equal(grid[1:], flipped.flip(-1))                        # the second sample: add_flip_right_inputs' flip
    assert float(grid[1, 0, 0, 0]) == -float(grid[0, 0, 0, -1]) and not torch.equal(grid[1, 0], grid[0, 0])   # another window
    for tag in ("decoder", "pose"):
        for l, (h, w) in enumerate(cases[tag]["sizes"]):
            assert arrays["%s/map%d" % (tag, l)].shape == arrays["%s/functional%d" % (tag, l)].shape == (2, 8, h, w)
        assert arrays[tag + "/g_w1"].shape == (16, 2, 1, 1) and arrays[tag + "/g_w2"].shape == (8, 16, 1, 1)
    assert os.path.getsize(os.path.join(GOLDEN, "grid_embedding.npz")) < 200 * 1024


@pytest.mark.parametrize("tag", ("decoder", "pose"))
def test_fp64_restatement_meets_the_reference_fixture_neural(tag):
    meta, arrays = load_fixture()
    case = meta["cases"][tag]
    grid, weights = torch.from_numpy(arrays["grid"]), fixture_weights(arrays, tag)
    functional = [torch.from_numpy(arrays["%s/functional%d" % (tag, l)]) for l in range(len(case["sizes"]))]
    levels, grads = pyramid_and_gradients_fp64(grid, case["sizes"], weights, functional)
    for l, lv in enumerate(levels):
        assert float((lv - torch.from_numpy(arrays["%s/map%d" % (tag, l)]).double()).abs().max()) < 1e-4, l
    for name, g in zip(("g_w1", "g_b1", "g_w2", "g_b2"), grads):
        assert float((g - torch.from_numpy(arrays["%s/%s" % (tag, name)]).double()).abs().max()) < 1e-4, name


@pytest.mark.parametrize("tag", ("frequency", "identity"))
def test_fp64_restatement_meets_the_reference_fixture_plain(tag):
    meta, arrays = load_fixture()
    case = meta["cases"][tag]
    levels = pyramid_fp64(torch.from_numpy(arrays["grid"]), case["sizes"], tag, multires=case.get("multires", 0))
    for l, lv in enumerate(levels):
        assert tuple(lv.shape[1:]) == (case["E"],) + tuple(case["sizes"][l])
        assert float((lv - torch.from_numpy(arrays["%s/map%d" % (tag, l)]).double()).abs().max()) < 1e-4, l


def test_fixture_matches_the_live_reference():
    sys.path.insert(0, GOLDEN)
    from ref_import import reference_available
    if not reference_available():
        pytest.skip("reference tree not present")
    from make_embedding_golden import reference_outputs
    meta, arrays = load_fixture()
    live_meta, live = reference_outputs()
    assert live_meta == meta
    assert set(live) == set(arrays)
    for k, v in live.items():
        assert float(np.abs(arrays[k].astype(np.float64) - v).max()) <= 1e-6 * max(1.0, float(np.abs(v).max())), k


@pytest.mark.parametrize("shape", (SMALL, WORKLOAD))
def test_per_element_inputs_keep_both_elu_branches_live(shape):
    """Between 20 % and 80 % of z1 and of z2 are negative for the inputs the GPU tests use (E = 8: the workload's)."""
    share1, share2 = negative_shares(crop_grids(*shape), make_weights(8))
    print("negative shares at %s: z1 %.2f, z2 %.2f" % (shape, share1, share2))
    assert 0.2 <= share1 <= 0.8 and 0.2 <= share2 <= 0.8


def test_header_capi_and_library_agree():
    for name, value in (("PD_EMBED_NEURAL", 0), ("PD_EMBED_FREQUENCY", 1), ("PD_EMBED_IDENTITY", 2)):
        assert capi_header.constant(name) == getattr(C, name) == value, name
    assert embedding.KINDS == {"neural": 0, "frequency": 1, "identity": 2}
    lib = C.load()
    for name, ret, kinds in (("pd_grid_embed_fwd", "int", "IIIIIIIPPPPP"), ("pd_grid_embed_bwd", "int", "IIIIIPPPPPPP"),
                             ("pd_grid_embed_bwd_workspace_floats", "size_t", "IIIP")):
        assert capi_header.prototype(name)[0] == ret
        res, args = C.SIGNATURES[name]
        assert res is (ctypes.c_int if ret == "int" else ctypes.c_size_t)
        assert capi_header.kinds(name) == capi_header.ctypes_kinds(args) == list(kinds), name
        assert hasattr(lib, name)
    import planedepth_amd
    assert lib.pd_version() == 290 and planedepth_amd.__version__ == "0.2.9"
    assert ops.grid_embedding is embedding.grid_embedding and ops.fused_grid_embedding is embedding.fused_grid_embedding
    assert planedepth_amd.fused_grid_embedding is embedding.fused_grid_embedding
    assert planedepth_amd.decoder_embedding_sizes is ops.decoder_embedding_sizes is embedding.decoder_embedding_sizes


def sizes_array(sizes):
    return (ctypes.c_int32 * (2 * len(sizes)))(*[v for hw in sizes for v in hw])


def test_entry_points_refuse_on_the_host_without_gpu():
    """Every refusal is PD_ERR_ARG (1) with a message naming the offender; no pointer is dereferenced."""
    lib = C.load()
    P = ctypes.c_void_p(16)
    one = sizes_array([(3, 5)])

    def fwd(B=2, H=8, W=16, kind=0, E=8, multires=0, n=1, sizes=one, grid=P, params=P, out=P):
        return lib.pd_grid_embed_fwd(B, H, W, kind, E, multires, n, sizes, grid, params, out, None)

    def bwd(B=2, H=8, W=16, E=8, n=1, sizes=one, ptrs=(P,) * 5):
        return lib.pd_grid_embed_bwd(B, H, W, E, n, sizes, *ptrs, None)

    def refused(rc, word):
        assert rc == 1 and word in lib.pd_last_error(), (rc, lib.pd_last_error())

    refused(fwd(grid=None), b"NULL")
    refused(fwd(out=None), b"NULL")
    refused(fwd(params=None), b"params")
    refused(fwd(sizes=None), b"sizes")
    refused(fwd(kind=3), b"kind 3")
    refused(fwd(kind=-1), b"kind -1")
    refused(fwd(E=0), b"E = 0")
    refused(fwd(E=17), b"E = 17")
    refused(fwd(kind=1, E=8, multires=2), b"E = 8")            # the frequency kind: E != 2 + 4 multires
    refused(fwd(kind=1, E=70, multires=17), b"multires = 17")
    refused(fwd(kind=2, E=3), b"E = 3")
    refused(fwd(n=0), b"n_levels = 0")
    refused(fwd(n=9, sizes=sizes_array([(1, 1)] * 9)), b"n_levels = 9")
    refused(fwd(sizes=sizes_array([(0, 5)])), b"level 0 is 0 x 5")
    refused(fwd(n=2, sizes=sizes_array([(3, 5), (4, -1)])), b"level 1 is 4 x -1")
    refused(fwd(B=0), b"bad shape")
    refused(fwd(H=40000), b"bad shape")
    refused(fwd(B=4, H=32768, W=32768), b"bad shape")            # 2 B H W reaches 2^31
    refused(fwd(B=1024, sizes=sizes_array([(2048, 1024)])), b"overflows")     # B h w = 2^31 output pixels
    refused(fwd(kind=1, E=10, multires=2, grid=None), b"NULL")    # the parameter-free kinds check their tensors too
    refused(bwd(E=0), b"E = 0")
    refused(bwd(E=17), b"E = 17")
    refused(bwd(n=9, sizes=sizes_array([(1, 1)] * 9)), b"n_levels = 9")
    refused(bwd(sizes=sizes_array([(3, 0)])), b"level 0 is 3 x 0")
    refused(bwd(B=1024, sizes=sizes_array([(2048, 1024)])), b"overflows")
    for k in range(5):
        refused(bwd(ptrs=tuple(None if j == k else P for j in range(5))), b"NULL")
    assert fwd(kind=2, E=2, params=None, grid=None) == 1 and b"NULL" in lib.pd_last_error()


@pytest.mark.parametrize("B,E,sizes", ((3, 8, LEVELS), (8, 8, DECODER_LEVELS), (1, 1, ((1, 1),)), (2, 16, ((16, 17),)),
                                       (4, 5, ((384, 1280), (192, 640)))))
def test_workspace_query_has_a_closed_form(B, E, sizes):
    lib = C.load()
    items = B * sum(h * w for h, w in sizes)
    want = min(-(-items // 256), 512) * n_params(E)
    assert lib.pd_grid_embed_bwd_workspace_floats(B, E, len(sizes), sizes_array(sizes)) == want
    assert lib.pd_grid_embed_bwd_workspace_floats(B, 0, len(sizes), sizes_array(sizes)) == 0      # what the backward refuses: 0
    assert lib.pd_grid_embed_bwd_workspace_floats(B, E, 0, sizes_array(sizes)) == 0


def test_module_dispatch_names_what_differs():
    grid = torch.zeros(1, 2, 4, 4)
    conv, elu = torch.nn.Conv2d, torch.nn.ELU
    with pytest.raises(ValueError, match="3 elements"):
        ops.fused_grid_embedding(torch.nn.Sequential(conv(2, 16, 1), elu(), conv(16, 8, 1)), grid, [(2, 2)])
    with pytest.raises(ValueError, match=r"epconv\[0\] is Conv2d\(2, 8"):
        ops.fused_grid_embedding(torch.nn.Sequential(conv(2, 8, 1), elu(), conv(8, 8, 1), elu()), grid, [(2, 2)])
    with pytest.raises(ValueError, match=r"epconv\[2\] is Conv2d\(16, 8, kernel_size=\(3, 3\)"):
        ops.fused_grid_embedding(torch.nn.Sequential(conv(2, 16, 1), elu(), conv(16, 8, 3, padding=1), elu()), grid, [(2, 2)])
    with pytest.raises(ValueError, match=r"epconv\[1\] is ReLU"):
        ops.fused_grid_embedding(torch.nn.Sequential(conv(2, 16, 1), torch.nn.ReLU(), conv(16, 8, 1), elu()), grid, [(2, 2)])
    with pytest.raises(ValueError, match="Conv2d"):
        ops.fused_grid_embedding(conv(2, 16, 1), grid, [(2, 2)])

    class Embedderish:
        kwargs = dict(include_input=False, input_dims=2, max_freq_log2=1, num_freqs=2, log_sampling=True,
                      periodic_fns=[torch.sin, torch.cos])
    with pytest.raises(ValueError, match="include_input"):
        ops.fused_grid_embedding(Embedderish(), grid, [(2, 2)])


def test_operator_refuses_cpu_tensors_and_bad_arguments():
    grid, weights = crop_grids(1, 5, 7), make_weights(8)
    with pytest.raises(C.PlaneDepthHipError):                      # valid arguments: only the device is wrong, and there is no fallback
        ops.grid_embedding(grid, [(2, 3)], weights)
    with pytest.raises(C.PlaneDepthHipError):
        ops.grid_embedding(grid, [(2, 3)], kind="identity")
    with pytest.raises(C.PlaneDepthHipError):
        ops.grid_embedding(grid, [(2, 3)], kind="frequency", multires=2)
    with pytest.raises(C.PlaneDepthHipError):
        ops.fused_grid_embedding(epconv_module(weights), grid, [(2, 3)])
    with pytest.raises(ValueError, match="requires a gradient"):
        ops.grid_embedding(grid.clone().requires_grad_(True), [(2, 3)], weights)
    with pytest.raises(ValueError, match="9 levels"):
        ops.grid_embedding(grid, [(1, 1)] * 9, weights)
    with pytest.raises(ValueError, match="sizes"):
        ops.grid_embedding(grid, [(0, 3)], weights)
    with pytest.raises(ValueError, match="kind"):
        ops.grid_embedding(grid, [(2, 3)], weights, kind="fourier")
    with pytest.raises(ValueError, match="w1"):
        ops.grid_embedding(grid, [(2, 3)], (weights[0][:8],) + weights[1:])
    with pytest.raises(ValueError, match="1 to 16"):
        ops.grid_embedding(grid, [(2, 3)], make_weights(17))
    with pytest.raises(ValueError, match="grid must be"):
        ops.grid_embedding(grid[:, :1], [(2, 3)], weights)
    feats = [torch.zeros(2, 4, 192 >> (i + 1), 640 >> (i + 1)) for i in range(5)]
    assert ops.decoder_embedding_sizes(feats) == DECODER_LEVELS


# ---------------------------------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------------------------------
gpu = pytest.mark.gpu
DEV = "cuda:0"


@functools.lru_cache(maxsize=None)
def neural_reference(shape, E, sizes):
    """(grid, weights, g_levels, fp64 levels, fp64 gradients) of one case, computed once and shared."""
    grid, weights = crop_grids(*shape), make_weights(E)
    g_levels = level_gradients(shape[0], E, sizes)
    levels, grads = pyramid_and_gradients_fp64(grid, sizes, weights, g_levels)
    return grid, weights, g_levels, levels, grads


def check_forward(got, want, torch_dev, what):
    """Per element |got - fp64| <= 1e-5 |fp64| + 1e-5 max|fp64|, and no further from fp64 than twice torch's fp32 chain + 1e-6."""
    for l, (g, w) in enumerate(zip(got, want)):
        assert g.dtype == torch.float32 and tuple(g.shape) == tuple(w.shape)
        err = (g.cpu().double() - w).abs()
        err_torch = float((torch_dev[l].cpu().double() - w).abs().max())
        print("%s level %d %s: kernel %.3e, torch fp32 on the device %.3e from fp64 (max |fp64| %.3g)"
              % (what, l, tuple(w.shape[2:]), float(err.max()), err_torch, float(w.abs().max())))
        assert bool((err <= allowance(w, 1e-5, 1e-5)).all()), (what, l, float(err.max()))
        assert float(err.max()) <= 2 * err_torch + 1e-6, (what, l, float(err.max()), err_torch)


def check_gradients(got, want, what, torch_grads=None):
    """Per parameter tensor |got - fp64| <= 1e-4 |g| + 1e-4 max|g|."""
    for k, (g, w) in enumerate(zip(got, want)):
        err = (g.cpu().double().reshape(w.shape) - w).abs()
        note = "" if torch_grads is None else ", torch fp32 %.3e" % float((torch_grads[k].cpu().double().reshape(w.shape) - w).abs().max())
        print("%s gradient %d: kernel %.3e from fp64%s (max |g| %.3g)" % (what, k, float(err.max()), note, float(w.abs().max())))
        assert bool((err <= allowance(w, 1e-4, 1e-4)).all()), (what, k, float(err.max()))


def run_fused(grid, weights, sizes, g_levels):
    """Forward and backward of ops.grid_embedding on the device -> (levels, parameter gradients)."""
    leaves = [t.to(DEV).requires_grad_(True) for t in weights]
    levels = ops.grid_embedding(grid.to(DEV), sizes, leaves)
    torch.autograd.backward(levels, [g.to(DEV) for g in g_levels])
    return [lv.detach() for lv in levels], [t.grad for t in leaves]


def run_torch(grid, weights, sizes, g_levels):
    module = epconv_module(weights).to(DEV)
    levels = torch_pyramid(module, grid.to(DEV), sizes)
    torch.autograd.backward(levels, [g.to(DEV) for g in g_levels])
    return [lv.detach() for lv in levels], [p.grad for p in module.parameters()]


@gpu
@pytest.mark.parametrize("E", CHANNELS)
def test_neural_forward_and_backward_match_fp64_per_element(E):
    """B = 3, 23 x 41, seven levels in one call (one pixel, one row, one column, down, the source's size, up, odd).  Torch's own fp32
    chain on the CPU is at most 0.013 of the forward allowance and 0.016 of the gradient allowance with these inputs."""
    grid, weights, g_levels, want, want_grads = neural_reference(SMALL, E, LEVELS)
    got, grads = run_fused(grid, weights, LEVELS, g_levels)
    ref, ref_grads = run_torch(grid, weights, LEVELS, g_levels)
    check_forward(got, want, ref, "E=%d" % E)
    check_gradients(grads, want_grads, "E=%d" % E, ref_grads)
    assert all(tuple(g.shape) == tuple(w.shape) for g, w in zip(grads, weights))
    base = got[0].untyped_storage().data_ptr()
    assert all(lv.untyped_storage().data_ptr() == base for lv in got)           # views of one allocation
    again, grads_again = run_fused(grid, weights, LEVELS, g_levels)
    assert all(torch.equal(a, b) for a, b in zip(got, again))
    assert all(torch.equal(a, b) for a, b in zip(grads, grads_again))           # no atomics: bit for bit


@gpu
@pytest.mark.parametrize("E", CHANNELS)
@pytest.mark.parametrize("size", ((7, 13), (23, 41), (1, 1)))
def test_neural_single_level_call(E, size):
    grid, weights, _, _, _ = neural_reference(SMALL, E, LEVELS)
    g_levels = level_gradients(SMALL[0], E, (size,), seed=3)
    want, want_grads = pyramid_and_gradients_fp64(grid, (size,), weights, g_levels)
    got, grads = run_fused(grid, weights, (size,), g_levels)
    ref, ref_grads = run_torch(grid, weights, (size,), g_levels)
    check_forward(got, want, ref, "E=%d single" % E)
    check_gradients(grads, want_grads, "E=%d single" % E, ref_grads)


@gpu
@pytest.mark.parametrize("kind,multires", (("frequency", MULTIRES), ("frequency", 0), ("identity", None)))
def test_plain_kinds_match_fp64_per_element(kind, multires):
    grid = crop_grids(*SMALL)
    m = multires or 0
    for sizes in (LEVELS, ((12, 21),)):
        want = pyramid_fp64(grid, sizes, kind, multires=m)
        got = ops.grid_embedding(grid.to(DEV), sizes, kind=kind, multires=multires)
        dev = grid.to(DEV)
        emb = dev if m == 0 else torch.cat([dev] + [fn(dev * 2.0 ** k) for k in range(m) for fn in (torch.sin, torch.cos)], 1)
        ref = torch_pyramid(None, emb, sizes)
        assert got[0].shape[1] == 2 + 4 * m
        check_forward(got, want, ref, "%s multires=%s" % (kind, multires))


@gpu
def test_workload_shape_forward_and_backward():
    """B = 8, 192 x 640, the decoder's five levels.  On the CPU torch's fp32 chain is 0.015 of the forward allowance and 0.06 of
    the gradient allowance here."""
    grid, weights, g_levels, want, want_grads = neural_reference(WORKLOAD, 8, DECODER_LEVELS)
    got, grads = run_fused(grid, weights, DECODER_LEVELS, g_levels)
    ref, ref_grads = run_torch(grid, weights, DECODER_LEVELS, g_levels)
    check_forward(got, want, ref, "workload")
    check_gradients(grads, want_grads, "workload", ref_grads)
    _, grads_again = run_fused(grid, weights, DECODER_LEVELS, g_levels)
    assert all(torch.equal(a, b) for a, b in zip(grads, grads_again))


@gpu
def test_identity_kind_is_exact():
    """A level of the source's size has the grid's bits (any values, NaN-free); on grids whose values and fractions are exactly
    representable every level has F.interpolate's bits."""
    grid = crop_grids(*SMALL).to(DEV)
    (full,) = ops.grid_embedding(grid, [SMALL[1:]], kind="identity")
    assert torch.equal(full, grid)
    H, W = 17, 33                                                   # (H - 1) and (W - 1) are powers of two
    ys, xs = torch.arange(H, dtype=torch.float32) / 8 - 1, torch.arange(W, dtype=torch.float32) / 16 - 1
    exact = torch.stack([xs[None, :].expand(H, W), ys[:, None].expand(H, W)])[None].repeat(2, 1, 1, 1).contiguous()
    exact[1, 0] = -exact[1, 0].flip(-1)
    exact = exact.to(DEV)
    sizes = ((17, 33), (9, 17), (5, 9), (3, 5), (2, 2), (1, 1), (33, 65))
    got = ops.grid_embedding(exact, sizes, kind="identity")
    for g, s in zip(got, sizes):
        assert torch.equal(g, F.interpolate(exact, size=s, align_corners=True, mode="bilinear")), s


@gpu
@pytest.mark.parametrize("tag", ("decoder", "pose", "frequency", "identity"))
def test_reference_fixture_through_fused_grid_embedding(tag):
    """The maps the reference's forward made and the gradients of its epconv parameters, through the reference-shaped modules rebuilt
    from the stored weights, at the plain 1e-4."""
    meta, arrays = load_fixture()
    case = meta["cases"][tag]
    grid = torch.from_numpy(arrays["grid"]).to(DEV)
    sizes = [tuple(s) for s in case["sizes"]]
    if tag == "identity":
        module = None
    elif tag == "frequency":
        class Embedder(torch.nn.Module):
            kwargs = dict(case["kwargs"], periodic_fns=[torch.sin, torch.cos])
        module = Embedder()
    else:
        module = epconv_module(fixture_weights(arrays, tag)).to(DEV)
    got = ops.fused_grid_embedding(module, grid, sizes)
    assert len(got) == len(sizes)
    for l, g in enumerate(got):
        want = torch.from_numpy(arrays["%s/map%d" % (tag, l)])
        assert tuple(g.shape) == tuple(want.shape)
        assert float((g.detach().cpu() - want).abs().max()) < 1e-4, (tag, l)
    if module is not None and tag != "frequency":
        loss = sum((g * torch.from_numpy(arrays["%s/functional%d" % (tag, l)]).to(DEV)).sum() for l, g in enumerate(got))
        loss.backward()
        for name, p in zip(("g_w1", "g_b1", "g_w2", "g_b2"), module.parameters()):
            want = torch.from_numpy(arrays["%s/%s" % (tag, name)])
            assert tuple(p.grad.shape) == tuple(want.shape)
            assert float((p.grad.cpu() - want).abs().max()) < 1e-4, (tag, name)
    else:
        assert not any(g.requires_grad for g in got)


@gpu
def test_writes_cover_exactly_the_outputs_and_gradients():
    """Outputs, workspace and gradients inside larger pre-filled buffers: every element around them keeps its fill."""
    lib = C.load()
    B, H, W = SMALL
    guard, fill = 4096, -7.0
    grid = crop_grids(*SMALL).to(DEV)
    arr = sizes_array(LEVELS)
    for E in CHANNELS:
        weights = make_weights(E)
        params = torch.cat([t.reshape(-1) for t in weights]).to(DEV)
        n = B * E * sum(h * w for h, w in LEVELS)
        buf = torch.full((2 * guard + n,), fill, device=DEV)
        C.check(lib.pd_grid_embed_fwd(B, H, W, C.PD_EMBED_NEURAL, E, 0, len(LEVELS), arr, C.ptr(grid), C.ptr(params),
                                      C.ptr(buf[guard:]), C.stream_handle(grid.device)), "pd_grid_embed_fwd")
        torch.cuda.synchronize()
        assert bool((buf[:guard] == fill).all()) and bool((buf[guard + n:] == fill).all()), E
        want = ops.grid_embedding(grid, LEVELS, [t.to(DEV) for t in weights])
        assert torch.equal(buf[guard:guard + n], torch.cat([w.reshape(-1) for w in want]))
        assert bool((buf[guard:guard + n] != fill).all())
        g_out = torch.randn(n, device=DEV)
        n_ws, M = lib.pd_grid_embed_bwd_workspace_floats(B, E, len(LEVELS), arr), n_params(E)
        wbuf = torch.full((2 * guard + n_ws,), fill, device=DEV)
        gbuf = torch.full((2 * guard + M,), fill, device=DEV)
        C.check(lib.pd_grid_embed_bwd(B, H, W, E, len(LEVELS), arr, C.ptr(grid), C.ptr(params), C.ptr(g_out), C.ptr(gbuf[guard:]),
                                      C.ptr(wbuf[guard:]), C.stream_handle(grid.device)), "pd_grid_embed_bwd")
        torch.cuda.synchronize()
        for b, m in ((wbuf, n_ws), (gbuf, M)):
            assert bool((b[:guard] == fill).all()) and bool((b[guard + m:] == fill).all()), E
        assert bool((wbuf[guard:guard + n_ws] != fill).all()) and bool((gbuf[guard:guard + M] != fill).all()), E
    for kind, multires in ((C.PD_EMBED_FREQUENCY, MULTIRES), (C.PD_EMBED_IDENTITY, 0)):
        E = 2 + 4 * multires
        n = B * E * sum(h * w for h, w in LEVELS)
        buf = torch.full((2 * guard + n,), fill, device=DEV)
        C.check(lib.pd_grid_embed_fwd(B, H, W, kind, E, multires, len(LEVELS), arr, C.ptr(grid), None, C.ptr(buf[guard:]),
                                      C.stream_handle(grid.device)), "pd_grid_embed_fwd")
        torch.cuda.synchronize()
        assert bool((buf[:guard] == fill).all()) and bool((buf[guard + n:] == fill).all()), kind
        assert bool((buf[guard:guard + n] != fill).all())


@gpu
def test_launches_follow_torchs_current_stream():
    grid, weights, g_levels, _, _ = neural_reference(SMALL, 8, LEVELS)
    want, want_grads = run_fused(grid, weights, LEVELS, g_levels)
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):
        staged = grid.to(DEV).clone()                 # produced on the side stream: only a launch there sees it in order
        leaves = [t.to(DEV).requires_grad_(True) for t in weights]
        got = ops.grid_embedding(staged, LEVELS, leaves)
        torch.autograd.backward(got, [g.to(DEV) for g in g_levels])
    side.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(got, want))
    assert all(torch.equal(t.grad, b) for t, b in zip(leaves, want_grads))


@gpu
def test_gradients_reach_epconv_through_a_consuming_convolution():
    """``conv(torch.cat([x, dgrid], 1))`` as the decoder trunk consumes the level: the gradients of ``epconv.parameters()`` against
    the torch formulation of the same module on the device, at 1e-4; under autocast the levels stay fp32."""
    torch.manual_seed(5)
    grid = crop_grids(2, 24, 40).to(DEV)
    fused_ep = epconv_module(make_weights(8)).to(DEV)
    torch_ep = copy.deepcopy(fused_ep)
    conv = torch.nn.Conv2d(5 + 8, 4, 3, padding=1).to(DEV)
    x = torch.randn(2, 5, 6, 10, device=DEV)
    r = torch.randn(2, 4, 6, 10, device=DEV)
    (dgrid,) = ops.fused_grid_embedding(fused_ep, grid, [(6, 10)])
    (conv(torch.cat([x, dgrid], 1)) * r).sum().backward()
    conv.zero_grad()
    dgrid_torch = F.interpolate(torch_ep(grid), size=(6, 10), align_corners=True, mode="bilinear")
    (conv(torch.cat([x, dgrid_torch], 1)) * r).sum().backward()
    assert float((dgrid - dgrid_torch).abs().max()) < 1e-4
    for p, q in zip(fused_ep.parameters(), torch_ep.parameters()):
        assert p.grad is not None and tuple(p.grad.shape) == tuple(p.shape)
        assert float((p.grad - q.grad).abs().max()) <= 1e-4 * max(1.0, float(q.grad.abs().max()))
    with torch.autocast("cuda", dtype=torch.bfloat16):
        (half,) = ops.fused_grid_embedding(fused_ep, grid, [(6, 10)])
    assert half.dtype == torch.float32 and torch.equal(half, dgrid)
