"""planedepth_amd — MI355X (gfx950) implementation of PlaneDepth's photometric-reconstruction hot path.

Importing the package does not need a GPU or the built library; calling any operator does (and raises otherwise).
"""
from . import decoder_tail, embedding, layers, metrics, ops, pipeline, pose, synthetic, trainer_path  # noqa: F401
from .decoder_tail import fused_decoder_tail  # noqa: F401
from .embedding import decoder_embedding_sizes, fused_grid_embedding  # noqa: F401
from .pipeline import device_batch, draw_params  # noqa: F401
from .pose import RawPose  # noqa: F401
from .predict import predict  # noqa: F401
from .layers import (SSIM, BackprojectDepth, HomographyWarp, Project3D, disp_to_depth,  # noqa: F401
                     get_smooth_loss_disp, multimodal_loss)
from .trainer_path import (add_flip_right_inputs, compute_depth_losses, compute_losses, compute_reprojection_loss,  # noqa: F401
                           generate_post_process_disp, patch_trainer, patch_trainer_metrics, patch_trainer_perceptual,
                           patch_trainer_poses, perceptual_loss, pred_novel_images, pred_self_images, predict_poses)

__version__ = "0.2.9"   # = pd_version() 290 of the library (tests/test_capi.py checks that they agree)
