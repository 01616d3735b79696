"""The oracle against the reference's own outputs on fresh seeds, from vectors the reference produced
(tests/golden/make_golden.py --only-live: live_<i>.npz, add_flip_right_inputs.npz, pair_transforms.npz).  What only
the reference tree itself can answer is checked by ``make_golden.py --check`` where that tree is present."""
import json
import os
import sys

import numpy as np
import pytest

from cases import load_fixture, rel_err, run_oracle
from conftest import GOLDEN

sys.path.insert(0, GOLDEN)
from make_golden import LIVE_CASES, PAIR_FH, PAIR_FW, PAIR_H, PAIR_SEED, PAIR_W, flip_inputs  # noqa: E402

CASES = LIVE_CASES


@pytest.mark.parametrize("bkw,rkw", CASES)
def test_live(bkw, rkw):
    from planedepth_amd.synthetic import build_case
    name = "live_%d" % CASES.index((bkw, rkw))
    case, want, run = load_fixture(name)
    assert run == rkw, (name, run)
    fresh = build_case(**bkw)       # the stored inputs are still what build_case draws for these seeds
    for k, v in case.items():
        assert np.array_equal(np.asarray(fresh[k]), v.numpy()), (name, k)
    got = run_oracle(case, rkw)
    for k, w in want.items():
        if k in ("smooth_loss", "total_loss"):
            continue
        if float(w.abs().max()) == 0.0:
            assert float(got[k].abs().max()) == 0.0, k
        else:
            assert rel_err(got[k], w) < 2e-6, (k, rel_err(got[k], w))


def test_add_flip_right_inputs_live():
    """trainer.py:252-276 against the oracle's restatement (bit-exact data movement)."""
    import torch
    from oracle import planedepth_oracle as orc
    z = np.load(os.path.join(GOLDEN, "add_flip_right_inputs.npz"))
    keys = [tuple(k) if isinstance(k, list) else k for k in json.loads(bytes(z["meta"]).decode())]
    want = {k: torch.from_numpy(z["key_%d" % i]) for i, k in enumerate(keys)}
    got = orc.add_flip_right_inputs(flip_inputs(), novel_frame_ids=(1,))
    assert set(got) == set(want)
    for k in want:
        assert torch.equal(got[k], want[k]), k


def test_synthetic_pipeline_follows_the_reference_conventions():
    """grid / K / inv_K / Rt of planedepth_amd.synthetic.kitti_like_inputs against what the
    reference's own transforms and dataset code produce (datasets/pair_transforms.py, mono_dataset.py:193-211)."""
    import random
    import torch
    from planedepth_amd import synthetic
    z = np.load(os.path.join(GOLDEN, "pair_transforms.npz"))
    H, W = PAIR_H, PAIR_W
    # Resize: the plain grid
    assert torch.equal(torch.from_numpy(z["resize_grid"]), synthetic.crop_grid(H, W, H, W, 0, 0))
    # RandomResizeCrop: replay its random draws to learn (factor, h0, w0), then rebuild the grid
    FH, FW = PAIR_FH, PAIR_FW
    np.random.seed(PAIR_SEED); random.seed(PAIR_SEED)
    fmin = max(max((H + 1) / FH, (W + 1) / FW), 0.75)
    factor = np.random.uniform(low=fmin, high=1.5)
    h0 = random.randint(0, int(FH * factor - H)); w0 = random.randint(0, int(FW * factor - W))
    assert torch.equal(torch.from_numpy(z["random_resize_crop_grid"]),
                       synthetic.crop_grid(H, W, int(FH * factor), int(FW * factor), h0, w0))
    # K, inv_K, Rt as the dataset builds them
    K = np.array([[0.58, 0, 0.5, 0], [0, 1.92, 0.5, 0], [0, 0, 1, 0], [0, 0, 0, 1]], dtype=np.float32)
    K[0, :] *= W; K[1, :] *= H
    batch = synthetic.kitti_like_inputs(2, H, W, seed=1)
    assert np.array_equal(batch["K"][0].numpy(), K) and np.array_equal(batch["inv_K"][1].numpy(), np.linalg.pinv(K))
    assert float(batch[("Rt", "l")][0, 0, 3]) == np.float32(0.1) and float(batch[("Rt", "r")][1, 0, 3]) == np.float32(-0.1)
    assert tuple(batch["grid"].shape) == (2, 2, H, W) and float(batch["grid"].abs().max()) <= 1.0
