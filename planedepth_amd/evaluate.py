"""``python -m planedepth_amd.evaluate``: the ``--ext_disp_to_eval`` route of ``evaluate_depth_HR.py`` (:184-279) with
the metrics computed on the GPU (``planedepth_amd.metrics``, contract A).

    python -m planedepth_amd.evaluate --ext_disp_to_eval disps.npy --gt_path splits/eigen_raw/gt_depths.npz --eval_mono

``disps.npy`` holds [M,h,w] disparities (with ``--post_process``: [2M,h,w], the mirrored passes after the images, and the
post-processing is applied here); ``gt_depths.npz`` is the reference's object array under ``"data"``.  Prints the
reference's lines.  Out of scope: the ``benchmark`` split's PNG export and ``--eval_eigen_to_benchmark``.
"""
import argparse
import sys

import numpy as np
import torch


def parse(argv=None):
    p = argparse.ArgumentParser(description=__doc__.split("\n\n")[0], formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--ext_disp_to_eval", required=True, help="a .npy of predicted disparities")
    p.add_argument("--gt_path", required=True, help="gt_depths.npz (object array under 'data')")
    p.add_argument("--eval_split", default="eigen_raw",
                   choices=["eigen_raw", "eigen_improved", "eigen_benchmark", "odom_9", "odom_10", "city"])
    p.add_argument("--eval_mono", action="store_true")
    p.add_argument("--eval_stereo", action="store_true")
    p.add_argument("--width", type=int, default=640, help="the network's input width (opt.width)")
    p.add_argument("--post_process", action="store_true")
    p.add_argument("--disable_median_scaling", action="store_true")
    p.add_argument("--pred_depth_scale_factor", type=float, default=1)
    return p.parse_args(argv)


def main(argv=None):
    from . import metrics
    opt = parse(argv)
    if int(opt.eval_mono) + int(opt.eval_stereo) != 1:
        sys.exit("Please choose mono or stereo evaluation by setting either --eval_mono or --eval_stereo")
    print("-> Loading predictions from {}".format(opt.ext_disp_to_eval))
    pred = np.load(opt.ext_disp_to_eval).astype(np.float32, copy=False)
    gt = np.load(opt.gt_path, fix_imports=True, encoding="latin1", allow_pickle=True)["data"]
    print("-> Evaluating")
    if opt.eval_stereo:
        print("   Stereo evaluation - disabling median scaling, scaling by {}".format(metrics.STEREO_SCALE_FACTOR))
        opt.disable_median_scaling = True
        opt.pred_depth_scale_factor = metrics.STEREO_SCALE_FACTOR
    else:
        print("   Mono evaluation - using median scaling")
    device = torch.device("cuda", torch.cuda.current_device())
    pred = torch.from_numpy(pred).to(device)
    res = metrics.eval_depth_errors(pred, list(gt), width=opt.width, split=opt.eval_split, post_process=opt.post_process,
                                    median_scaling=not opt.disable_median_scaling,
                                    scale_factor=opt.pred_depth_scale_factor)
    print(metrics.format_summary(metrics.summarize(res, median_scaling=not opt.disable_median_scaling)))
    print("\n-> Done!")


if __name__ == "__main__":
    main()
