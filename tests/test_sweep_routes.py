"""The plane sweep's route decision, pinned on the CPU: for the grid of descriptors recorded in tests/golden/sweep_routes.npz
(tests/golden/make_sweep_routes.py states the grid and records it; the fixture names the commit it was taken at) the built
library gives the same capability-query answers and the same return codes — and error texts — from the entry points called
with all-NULL tensors.  Nothing here launches a kernel — and with NULL tensors no call gets past validate(), so the entry-point
columns pin validate()'s refusals and their order only: the dispatch on the routed family (the PD_IMPL_TILE reach, the tail and
bf16 refusals, anything that depends on a per-pixel mask, unaligned tensors or no gradients wanted) is the GPU suite's to check."""
import importlib.util
import json
import os

import numpy as np

from conftest import GOLDEN
from planedepth_amd import _capi as C


def _generator():
    spec = importlib.util.spec_from_file_location("make_sweep_routes", os.path.join(GOLDEN, "make_sweep_routes.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_library_reproduces_the_recorded_route_table():
    gen = _generator()
    z = np.load(os.path.join(GOLDEN, "sweep_routes.npz"))
    meta = json.loads(str(z["meta"]))
    rows, want = z["rows"], z["answers"]
    # the fixture is the grid the generator states, taken with the columns it evaluates today
    assert tuple(meta["columns"]) == gen.COLUMNS and [tuple(s) for s in meta["shapes"]] == list(gen.SHAPES)
    assert tuple(meta["signs"]) == gen.SIGNS and len(meta["commit"]) == 40
    assert np.array_equal(rows, gen.grid())
    assert len(rows) > 100000
    got = gen.evaluate(C.load(), rows)
    bad = np.nonzero((got != want).any(axis=1))[0]
    detail = [(tuple(rows[i]), dict((c, (int(want[i, k]), int(got[i, k]))) for k, c in enumerate(gen.COLUMNS) if want[i, k] != got[i, k]))
              for i in bad[:10]]
    assert len(bad) == 0, "%d rows differ (shape index, mode, flags, impl, sign index) -> column: (recorded, got): %r" % (len(bad), detail)
