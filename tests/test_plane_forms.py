"""The form decision for ``disp_layered`` / ``padding_mask`` (per plane, rows, dense), pinned on the CPU: for the grid of tensors that
tests/golden/make_plane_forms.py states — every map and mask form x ``row_uniform`` x the five consumers, with the row kernels
serving the shape and not, fused tail + sweep chains and refusals included — the package derives the flags and operands recorded in
tests/golden/plane_forms.json (taken at the commit the fixture names, before the consumers shared ``planeform``): the same shapes,
dtypes, strides, the same identity with the caller's rows tensor, the same autograd node, the same link and consumer count, the
same exception.  Nothing here launches a kernel; what the kernels compute from these operands is the GPU suite's to check."""
import importlib.util
import json
import os

from conftest import GOLDEN


def _generator():
    spec = importlib.util.spec_from_file_location("make_plane_forms", os.path.join(GOLDEN, "make_plane_forms.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_package_reproduces_the_recorded_plane_forms():
    gen = _generator()
    with open(os.path.join(GOLDEN, "plane_forms.json")) as f:
        z = json.load(f)
    assert z["shape"] == [gen.B, gen.N, gen.H, gen.W] and len(z["commit"]) == 40
    ids = ["/".join(map(str, c)) for c in gen.grid()]
    assert list(z["cases"]) == sorted(ids) and len(ids) == len(set(ids)) > 1000   # the grid the generator states, nothing left out
    got = gen.evaluate()
    bad = [(k, z["results"][z["cases"][k]], got[k]) for k in ids if got[k] != z["results"][z["cases"][k]]]
    assert not bad, "%d of %d cases differ; (case, recorded, got): %r" % (len(bad), len(ids), bad[:5])
    # every consumer and every form took part, refusals too
    seen = {(k.split("/")[0], r.get("form", r.get("raises"))) for k, r in got.items()}
    assert {(c, f) for c in ("sweep", "tail", "pp") for f in ("per_plane", "rows", "dense", "ValueError")} <= seen
    assert {(c, f) for c in ("layers", "plade") for f in ("per_plane", "dense", "RuntimeError")} <= seen
