"""Autograd-aware operators over the C ABI (``include/planedepth_hip.h``) — the one namespace the rest of the package, the tests
and ``bench.py`` use.  The operators live in ``sweep`` (the fused plane sweep: autograd nodes, routing, homography algebra),
``tails`` (decoder / PladeNet tails), ``losses`` (SSIM, mixture NLL, masked photometric, smoothness, perceptual feature distance), ``postprocess``
(self-distillation warps, batch doubling, crop grid), ``metrics`` (depth evaluation), ``geometry`` (backproject / project /
homography grids, grid_sample), ``pipeline`` (the input pipeline: fused bicubic resize-crop and augmentation), ``embedding`` (the decoders' positional encoding of the grid: embedding and bilinear pyramid in one launch), ``pose`` (the pose path: decoder tail, rotation and conjugation with Rc in one launch), ``render`` (novel views at inference: up to four rendered views from the conv outputs in one launch, and views at arbitrary camera poses) and ``_buffers`` (descriptors, pre-zeroed pools); the switches tests flip between calls (``ops.SWEEP_IMPL = ...``) are attributes
of ``_state`` that this module forwards both ways.  ``planeform``: the forms of ``disp_layered`` / ``padding_mask`` (per plane, rows, dense) they all read.

Every function launches hand-written HIP kernels through ctypes on torch's current stream.  PyTorch is used for device
memory, streams and autograd plumbing only; there is no eager / CPU implementation behind these ops.
"""
import sys
import types

from . import _capi as C  # noqa: F401
from . import _state
from ._buffers import (  # noqa: F401
    _timed, _desc, _contig, _ZERO_POOL, _zero_scalar, _ZERO_BLOCKS,
    _ZERO_BLOCK_FLOATS, _zero_block, _plane_grad_buffer)
from .planeform import _per_plane_view, _FirstColumn, _row_view, _rows_of, _RowView, row_view  # noqa: F401
from .sweep import (  # noqa: F401
    SweepCall, SweepSaved, _sweep_forward, _sweep_forward_pair, _sweep_backward_pair, _sweep_backward, _sweep_backward_tail,
    TailLink, _GradTap, tail_taps, _PlaneSweep, _SIDE_FIELDS, _PER_SIDE, _MultiPlaneSweep,
    plane_sweep_multi, as_f32, _storage_route, _flags, _SIGN, plane_sweep_disp,
    homography_matrices, _HomographyMatrices, homography_matrices_fused, plane_sweep_homography, _stereo_rows_sweep, plane_sweep_layers)
from .tails import (  # noqa: F401
    _PlaneLevels, plane_disparities, _PlaneGeometry, plane_geometry,
    _DecoderTail, decoder_tail, _PladeTail, _RAY_NORM, camera_ray_norm, _camera_ray_norm,
    plade_tail, InferenceTail, decoder_tail_inference, plade_tail_inference)
from .losses import (  # noqa: F401
    _SSIM, ssim, _ReprojLoss, reprojection_loss, _MixtureNLL, multimodal_loss,
    _MaskedPhotometric, masked_photometric, _row_strided, _SmoothLoss, smooth_loss_disp,
    _FeatureDistance, feature_distance)
from .postprocess import (  # noqa: F401
    _pp_disp, warp_route, post_process_route, warp_softmax, warp_sum, pp_combine, post_process_disp, post_process_disp_stepwise, cat_flip,
    crop_grid)
from .metrics import (  # noqa: F401
    DepthEval, PackedGT, pack_gt, eval_depth_errors, resize_disp, trainer_depth_metrics, summarize)
from .geometry import (  # noqa: F401
    _Backproject, backproject_depth, _Project3D, project_3d, _HomographyGrid, homography_grid,
    _GridSample, grid_sample)
from .pipeline import resize_crop_augment, resize_crop_depth  # noqa: F401
from .embedding import grid_embedding, fused_grid_embedding, decoder_embedding_sizes  # noqa: F401
from .pose import _PoseTail, pose_matrices, pose_tail, pose_conjugate  # noqa: F401
from .render import Views, render_views, render_cols_per_lane, render_poses  # noqa: F401


class _OpsModule(types.ModuleType):
    """``ops.<SWITCH>`` is ``_state.<SWITCH>``: read at call time by the operator modules, so an assignment here (tests,
    bench.py, monkeypatch) takes effect everywhere."""

    def __getattr__(self, name):
        name = _state.ALIASES.get(name, name)
        if name in _state.SWITCHES:
            return getattr(_state, name)
        raise AttributeError("module %r has no attribute %r" % (self.__name__, name))

    def __setattr__(self, name, value):
        name = _state.ALIASES.get(name, name)
        if name in _state.SWITCHES:
            setattr(_state, name, value)
        else:
            super().__setattr__(name, value)

    def __delattr__(self, name):
        if name in _state.SWITCHES or name in _state.ALIASES:
            raise AttributeError("%s is a switch of planedepth_amd._state" % name)
        super().__delattr__(name)


sys.modules[__name__].__class__ = _OpsModule
