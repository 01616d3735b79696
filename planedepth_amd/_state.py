"""Process-wide switches of the operators (``planedepth_amd.ops.<NAME>`` reads and writes these: tests and ``bench.py`` flip
them between calls; the modules that act on them read ``_state.<NAME>`` at call time)."""
import os

from . import _capi as C


# Kernel selection for the sweep (C.PD_IMPL_AUTO | C.PD_IMPL_GENERAL | ...).  Tests flip it to cross-check the specialised
# row kernels against the general ones; leave it alone otherwise.
SWEEP_IMPL = int(os.environ.get("PD_SWEEP_IMPL", C.PD_IMPL_AUTO))  # 0 auto, 1 general kernels, 2 fast rows (A/B runs)
LAST_SWEEP_FLAGS = None  # flags of the most recent sweep forward (introspection for tests)
DEBUG_STASH = None       # diagnostics: set to a list to collect the forward's per-pixel stash
# two plane-uniform views of a step go through the forward and the backward together (pd_uniform_fwd_pair / _bwd_pair: one
# launch for both forwards, both first passes, one gather kernel for both second passes); off (either of PD_PAIR_FORWARD=0 /
# PD_PAIR_GATHER=0, the historical names of its halves): one view after the other, the A/B and the tests' reference
PAIR_VIEWS = os.environ.get("PD_PAIR_FORWARD", "1") != "0" and os.environ.get("PD_PAIR_GATHER", "1") != "0"
DEBUG_WORKSPACE = None   # diagnostics (tests): set to a list to collect (descriptor, workspace) of every sweep backward
KERNEL_EVENTS = None     # measurement (bench.py): set to a dict {"fwd": [], "bwd": []} to collect (start, end) CUDA events
                         # recorded on the launch stream around the sweep's C-ABI calls INSIDE a training step
PLANE_ADDS = os.environ.get("PD_PLANE_ADDS", "1") != "0"   # A/B switch: 0 = per-row partial sums + a reduction launch per backward
# PD_TORCH_HOMOGRAPHY=1: form the matrices with the stock torch chain (sweep.homography_matrices: torch.inverse and its
# rounding, ~12 launches + rocSOLVER, not graph-capturable) instead of pd_homography_matrices_fwd/bwd
TORCH_HOMOGRAPHY = bool(int(os.environ.get("PD_TORCH_HOMOGRAPHY", "0")))

SWITCHES = ("SWEEP_IMPL", "LAST_SWEEP_FLAGS", "DEBUG_STASH", "PAIR_VIEWS", "DEBUG_WORKSPACE", "KERNEL_EVENTS",
            "PLANE_ADDS", "TORCH_HOMOGRAPHY")
ALIASES = {"PAIR_GATHER": "PAIR_VIEWS", "PAIR_FORWARD": "PAIR_VIEWS"}   # ``ops.PAIR_GATHER`` / ``ops.PAIR_FORWARD`` are the one switch
