"""Records tests/golden/plane_forms.json: which form (per plane, rows, dense) every consumer of ``disp_layered`` / ``padding_mask``
takes for a grid of CPU tensors, and the operand it derives — flags, shape, dtype, strides, whether the operand IS the caller's
[B,N,H] rows tensor or shares its memory, its ``grad_fn`` and ``requires_grad``, for chains of a fused decoder tail and its sweep
whether a link was made and ``link.consumers`` afterwards, for refusals the exception's type and text.  Nothing launches a kernel.
tests/test_plane_forms.py replays the grid on the tree under test and compares every field.

    python tests/golden/make_plane_forms.py            # rewrites the fixture from the code of the checkout this file lies in

The fixture pins behaviour across a refactor, so it is recorded from the commit BEFORE that refactor (the fixture names it): copy
this file into a checkout of that commit, run it there, copy the fixture back.

How each consumer is captured on the CPU:
  sweep       ``plane_sweep_disp(..., defer=True)`` returns the SweepCall after the capability queries only;
  tail, plade ``tails._DecoderTail`` / ``tails._PladeTail`` are replaced by a stand-in whose ``apply`` notes its arguments, fills the
              link fields the real forward fills and returns tensors of the right shapes;
  layers      ``plane_sweep_layers`` with ``C.call`` replaced by a stub that notes the arguments of its one launch,
              ``pd_plane_sweep_layers``;
  pp          ``ops._pp_disp`` under ``torch.no_grad()`` on the detached map, as the three post-process operators call it.

The grid, at 2x5x6x16: both ``ops.SWEEP_IMPL = PD_IMPL_AUTO`` (the row kernels serve the shape) and ``PD_IMPL_GENERAL`` (they do
not; ``evaluate`` asserts both answers of pd_sweep_uses_rowshift) x the map forms MAPS x the mask forms MASKS x ``row_uniform`` off
and on x the five consumers, thinned only by what a consumer does not take: ``plade`` and ``pp`` have no mask, ``layers``, ``tail``
and ``plade`` no ``row_uniform``.  ``tail`` runs with ``fuse_sweep_backward`` off and on; with it on, a sweep (``row_uniform`` off
and on) is fed the tail's logits / sigma and first the tail's own views, then a dense copy of the map, then (with a mask) a dense
copy of the mask — the last two must count as a consumer the fused form does not serve.  ``rows_path``: the sweep's internal
``_rows=(shift, mask)`` call.  No case had to be left out."""
import itertools
import json
import os
import subprocess
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
FIXTURE = os.path.join(HERE, "plane_forms.json")

B, N, H, W = 2, 5, 6, 16
IMPLS = ("auto", "general")
MAPS = ("per_plane_expanded", "per_plane_unexpanded", "hw_expanded_other_base", "row_view", "row_view_batch_slice",
        "row_view_untagged", "row_view_no_grad", "dense_non_leaf", "dense_leaf", "row_view_wrong_w")
MASKS = ("none", "row_view_f32", "row_view_bool", "dense_f32", "dense_bool", "bnh1_f32")


def form_of(flags, consumer):
    """The form a consumer's flags name: "per_plane", "rows" or "dense" (its PD_*DISP_ROWS / PD_*DISP_DENSE bits)."""
    from planedepth_amd import _capi as C
    rows, dense = dict(sweep=(C.PD_DISP_ROWS, C.PD_DISP_DENSE), tail=(C.PD_TAIL_DISP_ROWS, C.PD_TAIL_DISP_DENSE),
                       pp=(C.PD_PP_DISP_ROWS, C.PD_PP_DISP_DENSE))[consumer]
    return {0: "per_plane", rows: "rows", dense: "dense"}[flags & (rows | dense)]


def _grad(*shape):
    """A non-leaf tensor that requires grad (what a decoder hands over)."""
    return torch.rand(*shape, requires_grad=True) * 1.0


def make_map(kind, ops, n=N):
    """-> (disp_layered, the caller's [B,N,H] rows tensor or None)."""
    if kind == "per_plane_expanded":
        return _grad(B, n, 1, 1).expand(B, n, H, W), None
    if kind == "per_plane_unexpanded":
        return _grad(B, n, 1, 1), None
    if kind == "hw_expanded_other_base":
        return _grad(B, n, 2, 1)[:, :, :1].expand(B, n, H, W), None
    if kind == "dense_non_leaf":
        return _grad(B, n, H, W), None
    if kind == "dense_leaf":
        return torch.rand(B, n, H, W, requires_grad=True), None
    if kind == "row_view_batch_slice":
        rows = _grad(B + 1, n, H)
        return ops.row_view(rows, W)[:B], rows
    rows = torch.rand(B, n, H) if kind == "row_view_no_grad" else _grad(B, n, H)
    if kind == "row_view_untagged":
        return rows.unsqueeze(-1).expand(B, n, H, W), rows
    return ops.row_view(rows, W + 1 if kind == "row_view_wrong_w" else W), rows


def make_mask(kind, ops, n=N):
    """-> (padding_mask, the caller's [B,N,H] rows tensor or None)."""
    if kind == "none":
        return None, None
    if kind.startswith("row_view"):
        rows = (torch.rand(B, n, H) > 0.3)
        rows = rows if kind.endswith("bool") else rows.float()
        return ops.row_view(rows, W), rows
    if kind == "bnh1_f32":
        return (torch.rand(B, n, H, 1) > 0.3).float(), None
    dense = torch.rand(B, n, H, W) > 0.3
    return (dense if kind.endswith("bool") else dense.float()), None


def describe(t, rows):
    """What the fixture keeps of an operand."""
    if t is None:
        return None
    return dict(shape=list(t.shape), dtype=str(t.dtype), strides=list(t.stride()), is_rows=t is rows,
                shares_rows=rows is not None and t.data_ptr() == rows.data_ptr(),
                grad_fn=None if t.grad_fn is None else type(t.grad_fn).__name__, requires_grad=t.requires_grad)


def _images():
    return torch.rand(B, 3, H, W), torch.rand(B, 3, H, W)


def run_sweep(ops, logits, sigma, disp_layered, rows, mask, mask_rows, row_uniform, **kw):
    src, tgt = _images()
    call = ops.plane_sweep_disp(src, tgt, logits, sigma, disp_layered, mask, row_uniform=row_uniform, defer=True, **kw)
    flags = int(call.flags)
    return dict(flags=flags, form=form_of(flags, "sweep"), plane=describe(call.plane, rows),
                mask=describe(call.padding_mask, mask_rows), linked=call.link is not None)


class _Recorder:
    """Stand-in for ``_DecoderTail`` / ``_PladeTail``: same ``apply`` signature, no kernel."""
    seen = None

    @classmethod
    def apply(cls, raw_logits, raw_sigma, plane, fourth, flags, link=None):
        from planedepth_amd import _capi as C
        from planedepth_amd._buffers import _contig
        cls.seen = dict(plane=plane, fourth=fourth, flags=int(flags), link=link)
        n = raw_sigma.shape[1]
        logits = raw_logits.view_as(raw_logits) if raw_logits.shape[1] == n else torch.rand(B, n, H, W) + 0 * raw_logits.sum()
        sigma, small = raw_sigma.view_as(raw_sigma), torch.rand(B, 1, H, W)
        if link is not None:   # (_DecoderTail.forward: the contiguous operands)
            link.raw_sigma, link.stash, link.disp = raw_sigma, torch.rand(B, 2, H, W), small
            link.mask_rows = _contig(fourth)
            link.disp_rows = _contig(plane) if flags & C.PD_TAIL_DISP_ROWS else None
        if cls is _PladeRecorder:
            return logits, torch.rand(B, n - 1, H, W), sigma, small, small.clone(), small.clone()
        return logits, sigma, small, small.clone(), small.clone()


class _PladeRecorder(_Recorder):
    pass


def run_tail(ops, tails, map_kind, mask_kind, fuse, feed=None, row_uniform=False):
    disp_layered, rows = make_map(map_kind, ops)
    mask, mask_rows = make_mask(mask_kind, ops)
    logits, sigma, _, _, _ = tails.decoder_tail(_grad(B, N, H, W), _grad(B, N, H, W), mask, disp_layered, fuse_sweep_backward=fuse)
    seen = _Recorder.seen
    link = seen["link"]
    out = dict(flags=seen["flags"], form=form_of(seen["flags"], "tail"), plane=describe(seen["plane"], rows),
               mask=describe(seen["fourth"], mask_rows), link=link is not None)
    if feed is not None:
        if feed == "dense_map":
            disp_layered = disp_layered.expand(B, N, H, W).clone()
        if feed == "dense_mask":
            mask = mask.expand(B, N, H, W).clone()
        out["sweep"] = run_sweep(ops, logits, sigma, disp_layered, rows, mask, mask_rows, row_uniform)
        out["consumers"] = None if link is None else link.consumers
    return out


def run_plade(ops, tails, map_kind):
    disp_layered, rows = make_map(map_kind, ops)
    tails.plade_tail(_grad(B, N - 1, H, W), _grad(B, N, H, W), disp_layered, ray_norm=torch.rand(H, W))
    seen = _PladeRecorder.seen
    return dict(flags=seen["flags"], form=form_of(seen["flags"], "tail"), plane=describe(seen["plane"], rows))


def run_layers(ops, C, map_kind, mask_kind):
    disp_layered, rows = make_map(map_kind, ops)
    mask, mask_rows = make_mask(mask_kind, ops)
    seen = {}

    def stub(name, device, d, src, logits, sigma, plane, aux, k3, padding_mask, *rest):
        assert name == "pd_plane_sweep_layers", name
        seen.update(flags=int(d._obj.flags), plane=plane, mask=padding_mask)
    real = C.call
    C.call = stub
    try:
        ops.plane_sweep_layers(torch.rand(B, 3, H, W), torch.rand(B, N, H, W), torch.rand(B, N, H, W), disp_layered=disp_layered,
                               padding_mask=mask, want=("logit_rec",))
    finally:
        C.call = real
    return dict(flags=seen["flags"], form=form_of(seen["flags"], "sweep"), plane=describe(seen["plane"], rows),
                mask=describe(seen["mask"], mask_rows))


def run_pp(ops, map_kind, row_uniform):
    disp_layered, rows = make_map(map_kind, ops)
    with torch.no_grad():
        t, flags = ops._pp_disp(disp_layered.detach(), B, N, H, W, row_uniform)
    return dict(flags=int(flags), form=form_of(flags, "pp"), plane=describe(t, rows))


def run_rows_path(ops):
    shift, mask = _grad(B, N, H), (torch.rand(B, N, H) > 0.3).float()
    return run_sweep(ops, torch.rand(B, N, H, W), torch.rand(B, N, H, W), None, shift, None, mask, True, _rows=(shift, mask))


def grid():
    """The case ids, in order: tuples whose first entry names the consumer."""
    cases = []
    for impl in IMPLS:
        for m, k, ru in itertools.product(MAPS, MASKS, (False, True)):
            cases.append(("sweep", impl, m, k, ru))
        for m, k in itertools.product(MAPS, MASKS):
            cases.append(("layers", impl, m, k))
            cases.append(("tail", impl, m, k, False))
            cases.append(("tail", impl, m, k, True))
            for feed, ru in itertools.product(("own", "dense_map") + (("dense_mask",) if k != "none" else ()), (False, True)):
                cases.append(("tail+sweep", impl, m, k, feed, ru))
        for m in MAPS:
            cases.append(("plade", impl, m))
            cases.append(("pp", impl, m, False))
            cases.append(("pp", impl, m, True))
        cases.append(("rows_path", impl))
    return cases


def evaluate():
    """{case id (joined with '/'): what the package of this checkout does}."""
    import ctypes
    from planedepth_amd import _capi as C, _state, ops, tails
    lib = C.load()
    impls = dict(auto=C.PD_IMPL_AUTO, general=C.PD_IMPL_GENERAL)
    for name, want in (("auto", 1), ("general", 0)):   # the table covers the row kernels serving the shape AND not serving it
        got = lib.pd_sweep_uses_rowshift(ctypes.byref(C.SweepDesc(B, N, H, W, C.PD_WARP_DISP, 0, 1.0, impls[name])))
        assert got == want, (name, got)
    saved = (_state.SWEEP_IMPL, tails._DecoderTail, tails._PladeTail)
    tails._DecoderTail, tails._PladeTail = _Recorder, _PladeRecorder
    out = {}
    try:
        for case in grid():
            kind, impl, rest = case[0], case[1], case[2:]
            _state.SWEEP_IMPL = impls[impl]
            torch.manual_seed(0)
            try:
                if kind == "sweep":
                    m, k, ru = rest
                    (dl, rows), (mask, mask_rows) = make_map(m, ops), make_mask(k, ops)
                    r = run_sweep(ops, torch.rand(B, N, H, W), torch.rand(B, N, H, W), dl, rows, mask, mask_rows, ru)
                elif kind == "layers":
                    r = run_layers(ops, C, *rest)
                elif kind == "tail":
                    r = run_tail(ops, tails, *rest)
                elif kind == "tail+sweep":
                    m, k, feed, ru = rest
                    r = run_tail(ops, tails, m, k, True, feed, ru)
                elif kind == "plade":
                    r = run_plade(ops, tails, *rest)
                elif kind == "pp":
                    r = run_pp(ops, *rest)
                else:
                    r = run_rows_path(ops)
            except Exception as e:   # a refusal is a recorded result
                r = dict(raises=type(e).__name__, text=str(e))
            out["/".join(map(str, case))] = r
    finally:
        _state.SWEEP_IMPL, tails._DecoderTail, tails._PladeTail = saved
    return out


def main():
    sys.path.insert(0, ROOT)
    got = evaluate()
    try:
        commit = subprocess.check_output(["git", "-C", ROOT, "rev-parse", "HEAD"], text=True).strip()
    except (OSError, subprocess.CalledProcessError):
        commit = "unknown"
    results, index = [], {}     # many cases share one result: the fixture keeps each once
    cases = {k: index.setdefault(json.dumps(r, sort_keys=True), len(index)) for k, r in got.items()}
    results = [json.loads(s) for s in index]
    with open(FIXTURE, "w") as f:
        json.dump(dict(generator="tests/golden/make_plane_forms.py", commit=commit, shape=[B, N, H, W], torch=torch.__version__,
                       results=results, cases=cases), f, sort_keys=True, separators=(",", ":"))
        f.write("\n")
    print("%s: %d cases, %d distinct results, %d bytes" % (FIXTURE, len(cases), len(results), os.path.getsize(FIXTURE)))


if __name__ == "__main__":
    main()
