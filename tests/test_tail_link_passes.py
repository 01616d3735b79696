"""The tail link under backward passes that cover only part of the graph.

``decoder_tail(..., fuse_sweep_backward=True)`` keeps per-pass state with its ``TailLink``: the taps on ``disp`` / ``depth`` leave
their gradients in ``link.seen``, the sweep's backward takes them, applies the tail's backward in its own kernel
(pd_plane_sweep_bwd_tail / pd_plane_sweep_bwd_tail_rows) and says so in ``link.applied``, the tail's node consumes that.  Every
other test of the link runs tap, sweep and tail in one pass.  Here ``torch.autograd.grad`` walks parts of the graph — the tail's
outputs as inputs (the tail's node only captures), a ``disp``-only pass (no sweep), a pass that ends at ``disp`` taken before the
taps (neither sweep nor tail), a photometric-only pass (no tap), input subsets, two live graphs — and no pass may see what
another one left behind.

Both link forms on the smallest shapes at which the existing tests take the fused route ([2,7,9,256]: sigma on both clamp bounds,
an integer shift, and, for the rows, masked rows with an absurd disparity).  Every sequence of passes runs on three graphs: the
fused one, the same graph with ``fuse_sweep_backward=False`` (bound 5e-6, the project's bound for fused against unfused) and CPU
autograd through ``oracle.decoder_tail`` + ``oracle.warp_and_loss`` (bound 1e-4, the suite's bound).  The oracle runs in float32, as
test_tail_link_rows.run_cpu does: these cases sit ON the sampler's derivative discontinuity on purpose (the integer shift), where
the float32 grid round trip of the reference decides the side, and the oracle's float64 run lands on the other one — its own
float32 and float64 runs differ by 1.0e-1 (per-plane) / 7.9e-2 (rows) in the plane gradient (and so does the unfused product
from the float64 run: 1.03e-1 / 7.88e-2, against 1.9e-7 / 2.3e-7 from the float32 run; the conv outputs' gradients are within
1e-6 of both).  A float64 oracle is no reference for a 1e-4 bound on these cases.

Scenario A (``autograd.grad(obj, [logits, sigma])``) is REFUSED by the fused graph: the fused kernel has produced the conv
outputs' gradients by the time anyone can know that the tail's node will not run, so the pass ends with a PlaneDepthHipError that
names ``fuse_sweep_backward`` (TailLink).  The test accepts the right values as well, and nothing else.

Measured on an MI355X: profiles/operator_parity.md, "Tail link: partial passes"."""
import types

import pytest
import torch

import test_tail_link_rows as R
from cases import rel_err
from planedepth_amd._capi import PlaneDepthHipError
from planedepth_amd.decoder_tail import fused_decoder_tail

pytestmark = pytest.mark.gpu
TOL, TOL_FUSED, DEV = R.TOL, R.TOL_FUSED, R.DEV
TOL_ATOMIC = 2e-6   # two runs of the plane gradient of THESE cases (the bound of
                    # test_fused_decoder_tail_survives_a_second_backward_over_the_same_graph for a float-atomic sum): the per-plane
                    # link's [B,N] gradient is one, and on the rows the integer shift takes the irregular path, whose lanes add their
                    # shares to the row's slot with float atomics (measured: two identical passes over two identical graphs up to
                    # 1.3e-7 apart per plane, 5.8e-8 on the rows).  The conv outputs' gradients repeat bit for bit.
FORMS = ["per_plane", "rows"]
LEAVES = ("g_raw_logits", "g_raw_sigma", "g_plane")


def make_case(form, seed=78):
    c, _ = R.hand_built_rows(mask=form == "rows", rows_disp=form == "rows")
    if seed != 78:   # the same planes under other conv outputs, images and weights
        c = R.Case(c.shape, c.side, seed, c.leaf, c.build, c.xz_levels, sigma_bounds=True)
    return c


# ---- the graph and its handles -------------------------------------------------------------------------------------------------
def build_graph(c, fuse):
    """The product's graph as the trainer builds it: tail -> pred_novel_images (the sweep, then the taps).  ``early`` is ``disp``
    taken before the taps were installed."""
    from gpu_cases import make_stub_trainer
    a, s, p = (t.to(DEV).clone().requires_grad_(True) for t in (c.rl, c.rs, c.leaf))
    dl, pm = c.build(p, DEV, False)
    outputs = {"disp_layered": dl, "padding_mask": pm}
    fused_decoder_tail(outputs, a, s, use_mixture_loss=True, all_ones_mask=pm is None, fuse_sweep_backward=fuse)
    link = getattr(outputs["logits"], "_pd_tail_link", None)
    assert (link is not None) == fuse
    early = outputs["disp"]
    inputs = {("color", "l"): c.col_l.to(DEV), ("color", c.side): c.col_t.to(DEV), "K": c.K.to(DEV), "inv_K": c.inv_K.to(DEV)}
    make_stub_trainer(R.make_opt(c.xz_levels if pm is not None else 0), [c.side]).pred_novel_images(inputs, outputs)
    assert (outputs["disp"] is not early) == fuse   # the taps
    return types.SimpleNamespace(c=c, dev=DEV, leaves=(a, s, p), logits=outputs["logits"], sigma=outputs["sigma"], early=early,
                                 disp=outputs["disp"], depth=outputs["depth"], ph=outputs[("ph_mean", c.side)],
                                 rgb=outputs[("rgb_rec", c.side)], link=link)


def build_oracle(c, dtype=torch.float32):
    """The same handles on CPU autograd through the oracle (as test_tail_link_rows.run_cpu, in ``dtype``); the tap is a view.

    ``logits`` / ``sigma`` are views as well, and the oracle's sweep reads the views.  The product's tail is ONE node: its outputs
    ``logits`` / ``sigma`` carry what their consumer — the sweep — sends back and nothing else, fused or not.  ``oracle.decoder_tail``
    computes ``disp`` FROM its logits and sigma tensors, so ``retain_grad()`` on those would add the disp / depth share, a quantity
    no graph of the product reports there (measured: the unfused graph against it 1.0, the disp term dominates).  At the views the
    oracle reports the product's quantity: d obj / d (what the sweep reads)."""
    from oracle import planedepth_oracle as orc
    B, N, H, W = c.shape
    a, s, p = (t.to(dtype).clone().requires_grad_(True) for t in (c.rl, c.rs, c.leaf))
    dl, pm = c.build(p, "cpu", True)
    pm = torch.ones(B, N, H, W, dtype=dtype) if pm is None else pm.to(dtype)
    o = orc.decoder_tail(a, s, pm, dl, W, use_mixture_loss=True)
    logits, sigma = o["logits"].view_as(o["logits"]), o["sigma"].view_as(o["sigma"])
    r = orc.warp_and_loss(c.col_l.to(dtype), c.col_t.to(dtype), logits, sigma, warp_type="disp_warp", target_side=c.side,
                          disp_layered=dl.clamp(max=1e6), padding_mask=pm, distance=None, norm=None,
                          T=torch.eye(4, dtype=dtype)[None].repeat(B, 1, 1), K=c.K.to(dtype), inv_K=c.inv_K.to(dtype),
                          use_mixture_loss=True, automask=False)
    return types.SimpleNamespace(c=c, dev="cpu", leaves=(a, s, p), logits=logits, sigma=sigma, early=o["disp"],
                                 disp=o["disp"].view_as(o["disp"]), depth=o["depth"], ph=r["ph_loss"], rgb=r["rgb_rec"], link=None)


_REFERENCES = {}


def references(form, seed=78):
    """(unfused graph, oracle graph) of a case: built once, walked with retain_graph=True by every test, never changed."""
    if (form, seed) not in _REFERENCES:
        c = make_case(form, seed)
        _REFERENCES[form, seed] = (build_graph(c, False), build_oracle(c))
    return _REFERENCES[form, seed]


# ---- objectives and passes -----------------------------------------------------------------------------------------------------
def _w(G, i):
    return G.c.gw[i].to(G.dev)


def photometric(G):
    """Everything that reaches the leaves through the sweep: the photometric mean and a weight on rgb_rec."""
    return G.ph + (G.rgb * _w(G, 0)).sum()


def disp_depth(G):
    return (G.disp * _w(G, 1)).sum() + (G.depth * _w(G, 2)).sum()


def full(G):
    return photometric(G) + disp_depth(G)


def assert_clean(link):
    assert link.applied is None and not link.seen, (link.applied, link.seen)


def grad(G, obj, inputs, names):
    """One backward pass over the retained graph.  Whatever the pass did — a refusal included — the link holds nothing afterwards."""
    try:
        got = torch.autograd.grad(obj, inputs, retain_graph=True)
    finally:
        if G.link is not None:
            assert_clean(G.link)
    return {k: g.detach().cpu() for k, g in zip(names, got)}


def tail_outputs_pass(G):
    """Scenario A.  The gradients at logits / sigma, or ``None`` where the graph refuses the pass by name."""
    try:
        return grad(G, full(G), [G.logits, G.sigma], ("g_logits", "g_sigma"))
    except PlaneDepthHipError as e:
        assert "fuse_sweep_backward" in str(e), e
        return None


def compare(name, got, plain, want):
    """fused against unfused < TOL_FUSED, unfused and fused against the oracle < TOL; prints every figure first."""
    figures = {k: (rel_err(got[k], plain[k]), rel_err(plain[k], want[k]), rel_err(got[k], want[k])) for k in want}
    for k, e in figures.items():
        print("%s %s: fused vs unfused %.2e | unfused vs oracle %.2e | fused vs oracle %.2e" % ((name, k) + e))
    for k, e in figures.items():
        assert torch.isfinite(got[k]).all(), (name, k)
        assert e[0] < TOL_FUSED, (name, k, "fused vs unfused", e[0])
        assert e[1] < TOL, (name, k, "unfused vs oracle", e[1])
        assert e[2] < TOL, (name, k, "fused vs oracle", e[2])


def on_references(form, fn, seed=78):
    plain, oracle = references(form, seed)
    return fn(plain), fn(oracle)


def assert_clean_afterwards(G, form):
    """Scenario G: a full backward on the walked graph gives what a fresh fused graph gives: bit for bit in the conv outputs'
    gradients, within TOL_ATOMIC in the plane gradient (anything a pass left behind shows at 1e-2 and above)."""
    def full_backward(X):
        for t in X.leaves:
            t.grad = None
        before = X.link.fused_passes
        full(X).backward(retain_graph=True)
        assert X.link.fused_passes == before + 1
        assert_clean(X.link)
        return [t.grad.detach().cpu() for t in X.leaves]
    got, fresh = full_backward(G), full_backward(build_graph(G.c, True))
    for k, x, y in zip(LEAVES, got, fresh):
        if k == "g_plane":
            assert rel_err(x, y) < TOL_ATOMIC, (k, rel_err(x, y))
        else:
            assert torch.equal(x, y), (k, rel_err(x, y))


# ---- the scenarios -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", FORMS)
def test_a_tail_outputs_as_inputs(form):
    """``autograd.grad(obj, [logits, sigma])``: the engine runs the taps and the sweep and only CAPTURES at the tail's node.  The
    fused sweep has no output-space gradients to give: the right values or a refusal by name, never the conv outputs' gradients."""
    plain, oracle = references(form)
    want_plain, want = tail_outputs_pass(plain), tail_outputs_pass(oracle)
    # the test can tell the two spaces apart: on the unfused graph d obj / d sigma and d obj / d raw_sigma are far from each other
    # (sigmoid', the clamp gate on the bound columns, the disp share, and the mask on the rows)
    g_raw = grad(plain, full(plain), plain.leaves, LEAVES)
    apart = rel_err(want_plain["g_sigma"], g_raw["g_raw_sigma"])
    print("%s unfused: d obj / d sigma against d obj / d raw_sigma %.2e" % (form, apart))
    assert apart > 1e-2, apart
    for k in want:
        assert rel_err(want_plain[k], want[k]) < TOL, (k, "unfused vs oracle", rel_err(want_plain[k], want[k]))
    G = build_graph(make_case(form), True)
    got = tail_outputs_pass(G)
    assert G.link.fused_passes == 1          # the fused kernel did run in this pass, whatever became of its results
    if got is not None:
        compare(form + " A", got, want_plain, want)
    assert_clean_afterwards(G, form)


@pytest.mark.parametrize("form", FORMS)
def test_b_a_disp_only_pass_after_a_pass_the_tail_did_not_finish(form):
    """After A the sweep's "applied" note must not reach a later pass that runs the tap and the tail, but not the sweep: with A's
    own weights a stale note cancels the whole disp / depth gradient."""
    def passes(X):
        tail_outputs_pass(X)
        return grad(X, disp_depth(X), X.leaves, LEAVES)
    G = build_graph(make_case(form), True)
    got = passes(G)
    assert G.link.fused_passes == 1          # A's; the disp-only pass runs the tail's own kernel
    compare(form + " B", got, *on_references(form, passes))
    assert_clean_afterwards(G, form)


@pytest.mark.parametrize("form", FORMS)
def test_c_a_photometric_pass_after_a_pass_that_ended_at_the_early_disp(form):
    """The first pass runs a tap and nothing else; the gradient it left must not ride into the next pass's fused kernel."""
    def passes(X):
        first = grad(X, (X.disp * _w(X, 1)).sum(), [X.early], ("g_early",))
        return dict(first, **grad(X, X.ph, X.leaves, LEAVES))
    G = build_graph(make_case(form), True)
    got = passes(G)
    assert G.link.fused_passes == 1
    compare(form + " C", got, *on_references(form, passes))
    assert_clean_afterwards(G, form)


@pytest.mark.parametrize("form", FORMS)
def test_d_split_passes_add_up(form):
    def passes(X):
        out = {}
        for name, obj in (("ph", photometric), ("dd", disp_depth), ("full", full)):
            out.update(grad(X, obj(X), X.leaves, [name + " " + k for k in LEAVES]))
        return out
    G = build_graph(make_case(form), True)
    got = passes(G)
    assert G.link.fused_passes == 2          # the photometric and the full pass; the disp / depth pass does not reach the sweep
    compare(form + " D", got, *on_references(form, passes))
    for k in LEAVES:
        e = rel_err(got["ph " + k] + got["dd " + k], got["full " + k])
        print("%s D %s: photometric + disp/depth against full %.2e" % (form, k, e))
        assert e < TOL_FUSED, (k, e)
    assert_clean_afterwards(G, form)


@pytest.mark.parametrize("form", FORMS)
def test_e_input_subsets(form):
    """One leaf at a time: the matching slice of the full unfused result."""
    def passes(X):
        if X.link is None:
            return grad(X, full(X), X.leaves, LEAVES)
        out = {}
        for leaf, k in zip(X.leaves, LEAVES):
            out.update(grad(X, full(X), [leaf], (k,)))
        return out
    G = build_graph(make_case(form), True)
    got = passes(G)
    assert G.link.fused_passes == 3
    compare(form + " E", got, *on_references(form, passes))


@pytest.mark.parametrize("form", FORMS)
def test_f_two_live_graphs(form):
    """Two graphs, each with its own link, their passes interleaved: each gives what it gives alone."""
    def first(X):
        return grad(X, full(X), X.leaves, ["full " + k for k in LEAVES])

    def second(X):
        return grad(X, disp_depth(X), X.leaves, ["dd " + k for k in LEAVES])

    def third(X):
        return grad(X, photometric(X), X.leaves, ["ph " + k for k in LEAVES])
    c1, c2 = make_case(form), make_case(form, seed=178)
    G1, G2 = build_graph(c1, True), build_graph(c2, True)
    got1 = first(G1)
    got2 = third(G2)
    got1.update(second(G1))
    got2.update(first(G2))
    assert G1.link is not G2.link and G1.link.fused_passes == 1 and G2.link.fused_passes == 2
    for name, got, c, seed, order in (("1", got1, c1, 78, (first, second)), ("2", got2, c2, 178, (third, first))):
        def passes(X):
            return dict(order[0](X), **order[1](X))
        alone = passes(build_graph(c, True))
        for k in got:
            e = rel_err(got[k], alone[k])
            print("%s F graph %s %s: interleaved against alone %.2e" % (form, name, k, e))
            assert e < TOL_FUSED, (name, k, e)
        compare(form + " F graph " + name, got, *on_references(form, passes, seed))
