"""Records tests/golden/sweep_routes.npz: what the plane sweep's host side answers, without a GPU, for a fixed grid of
descriptors — the capability queries and the return codes of the entry points called with all-NULL tensors (which pins the
PD_ERR_ARG / PD_ERR_UNSUPPORTED split and the order of validate()'s refusals — no NULL call gets further; the CRC of
pd_last_error() pins their texts).
tests/test_sweep_routes.py asserts that the built library reproduces every row.

    python tests/golden/make_sweep_routes.py            # rewrites the fixture from the library of this tree

The grid (the full cross product is over a million rows; thinned by these rules, not by hand):
  A  the full product  flags (every subset of the 11 flags below) x impl 0..7 x both modes, sign +1, at the headline shape
     8x49x192x640 and at 2x9x24x80;
  B  every shape of SHAPES x both modes x impl 0..7 x the flag sets GROUPED: (mixture / automask) x (render) x (plane layout:
     per plane, dense, rows, rows + row mask, row mask alone, plane-uniform) x (backward extras: none, accumulate, zeroed
     plane block, deferred gather, bf16) — a superset of what bench.py's configurations and the GPU tests produce — plus every
     single flag on its own and DENSE | ROWS;
  C  the signs -1, 0, 0.5 next to +1 only where pd_sweep_bwd_tail_fuses can say 1: disp mode, mixture (with / without automask
     or the zeroed plane block), every shape, every impl.
SHAPES ends with rows that outgrow the LDS: W = 2560 (the row-stream backward fits, its decoder-tail form does not), W = 3000
(no row-stream backward; the plane-group row-shift kernels take it) and W = 3840 (beyond the row-shift kernels' own limit, which
is reached before the segment-stream forward's three row buffers stop fitting: general kernels)."""
import ctypes
import itertools
import json
import os
import subprocess
import sys
import zlib

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
FIXTURE = os.path.join(HERE, "sweep_routes.npz")

MIXTURE, AUTOMASK, RENDER_PROB, DISP_DENSE, DISP_ROWS, MASK_ROWS, HOMO_UNIFORM = 1, 2, 4, 8, 16, 32, 64
BWD_ACCUMULATE, BWD_DEFER_GATHER, BWD_PLANE_ZEROED, LOGITS_BF16 = 128, 256, 1024, 2048
FLAGS = (MIXTURE, AUTOMASK, RENDER_PROB, DISP_DENSE, DISP_ROWS, MASK_ROWS, HOMO_UNIFORM, BWD_ACCUMULATE, BWD_DEFER_GATHER,
         BWD_PLANE_ZEROED, LOGITS_BF16)
SHAPES = ((8, 49, 192, 640), (8, 63, 192, 640), (12, 49, 192, 640), (4, 49, 384, 1280), (1, 49, 192, 641), (2, 9, 24, 80),
          (1, 3, 5, 7), (1, 1, 20, 48), (1, 49, 8, 2560), (1, 49, 8, 3000), (1, 49, 8, 3840))
FULL_PRODUCT_SHAPES = (0, 5)
IMPLS = tuple(range(8))
SIGNS = (1.0, -1.0, 0.0, 0.5)
QUERIES = ("pd_sweep_uses_rowshift", "pd_sweep_native_bf16", "pd_sweep_bwd_accumulates", "pd_sweep_bwd_plane_adds",
           "pd_sweep_bwd_tail_fuses", "pd_sweep_stash_floats", "pd_sweep_bwd_workspace_floats")
ENTRIES = (("pd_plane_sweep_fwd", 14), ("pd_plane_sweep_bwd", 20), ("pd_plane_sweep_bwd_tail", 20))   # (name, NULL arguments)
COLUMNS = QUERIES + tuple(n + suffix for n, _ in ENTRIES for suffix in ("", ":error_crc"))


def grouped_flag_sets():
    out = set()
    for loss, render, layout, extra in itertools.product(
            (0, MIXTURE, MIXTURE | AUTOMASK, AUTOMASK), (0, RENDER_PROB),
            (0, DISP_DENSE, DISP_ROWS, DISP_ROWS | MASK_ROWS, MASK_ROWS, HOMO_UNIFORM),
            (0, BWD_ACCUMULATE, BWD_PLANE_ZEROED, BWD_DEFER_GATHER, LOGITS_BF16)):
        out.add(loss | render | layout | extra)
    out.update(FLAGS)
    out.add(DISP_DENSE | DISP_ROWS)
    return sorted(out)


def grid():
    """-> int64 [rows, 5]: (shape index, mode, flags, impl, index into SIGNS), sorted, no duplicates."""
    rows = set()
    every = [sum(c) for k in range(len(FLAGS) + 1) for c in itertools.combinations(FLAGS, k)]
    for s, mode, flags, impl in itertools.product(FULL_PRODUCT_SHAPES, (0, 1), every, IMPLS):          # A
        rows.add((s, mode, flags, impl, 0))
    for s, mode, flags, impl in itertools.product(range(len(SHAPES)), (0, 1), grouped_flag_sets(), IMPLS):   # B
        rows.add((s, mode, flags, impl, 0))
    for s, flags, impl, sg in itertools.product(range(len(SHAPES)), (MIXTURE, MIXTURE | AUTOMASK, MIXTURE | BWD_PLANE_ZEROED),
                                                IMPLS, range(1, len(SIGNS))):                          # C
        rows.add((s, 0, flags, impl, sg))
    return np.array(sorted(rows), dtype=np.int64)


def evaluate(lib, rows):
    """The library's answers for ``rows`` (as ``grid()`` returns them) -> int64 [rows, len(COLUMNS)]."""
    from planedepth_amd import _capi as C
    out = np.zeros((len(rows), len(COLUMNS)), dtype=np.int64)
    queries = [getattr(lib, q) for q in QUERIES]
    entries = [(getattr(lib, n), [None] * k) for n, k in ENTRIES]
    for r, (s, mode, flags, impl, sg) in enumerate(rows.tolist()):
        d = C.SweepDesc(*SHAPES[s], mode, flags, SIGNS[sg], impl)
        ref = ctypes.byref(d)
        vals = [int(q(ref)) for q in queries]
        for fn, null in entries:
            rc = int(fn(ref, *null))
            vals += [rc, zlib.crc32(lib.pd_last_error()) if rc else 0]
        out[r] = vals
    return out


def main():
    sys.path.insert(0, ROOT)
    from planedepth_amd import _capi as C
    lib = C.load()
    rows = grid()
    try:
        commit = subprocess.check_output(["git", "-C", ROOT, "rev-parse", "HEAD"], text=True).strip()
    except (OSError, subprocess.CalledProcessError):
        commit = "unknown"
    meta = dict(generator="tests/golden/make_sweep_routes.py", commit=commit, library_source_hash=lib.pd_source_hash().decode(),
                columns=COLUMNS, shapes=SHAPES, signs=SIGNS)
    np.savez_compressed(FIXTURE, rows=rows, answers=evaluate(lib, rows), meta=np.array(json.dumps(meta)))
    print("%s: %d rows, %d bytes" % (FIXTURE, len(rows), os.path.getsize(FIXTURE)))


if __name__ == "__main__":
    main()
