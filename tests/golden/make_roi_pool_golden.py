#!/usr/bin/env python
"""Generates tests/golden/roi_pool.npz by running the REFERENCE's own Python composition on the CPU:
pcdet/ops/roiaware_pool3d/roiaware_pool3d_utils.py (RoIAwarePool3dFunction forward and backward for max and avg,
points_in_boxes_cpu) and pcdet/ops/roipoint_pool3d/roipoint_pool3d_utils.py (RoIPointPool3d.forward), with their extension
modules `roiaware_pool3d_cuda` / `roipoint_pool3d_cuda` replaced by stubs backed by the numpy restatement of the kernels
(roi_pool_restatement.py), as make_stack_pool_golden.py does for the stack module.  `common_utils` and `box_utils` are
stubbed with the two functions the files use (check_numpy_to_torch; enlarge_box3d, which here also takes one width for
the three extents: the reference's default pool_extra_width=1.0 does not pass its own enlarge_box3d).

    python tests/golden/make_roi_pool_golden.py <checkout of the reference>

The reference sources are imported from where they lie; nothing of them is copied.  What is committed is data: small inputs
and the composition's outputs.  Inputs are the `exact` scenes of roi_pool_inputs.py (1/8 lattice, heading 0), so the file
does not depend on the contraction mode.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import roi_pool_inputs as gen  # noqa: E402
import roi_pool_restatement as ref  # noqa: E402
from reference_loader import load, np_args as _args, reference_root  # noqa: E402

F32, I32 = np.float32, np.int32


def _check_numpy_to_torch(x):
    if isinstance(x, np.ndarray):
        return torch.from_numpy(x).float(), True
    return x, False


def _enlarge_box3d(boxes3d, extra_width=(0, 0, 0)):
    large = boxes3d.clone()
    width = (extra_width,) * 3 if isinstance(extra_width, (int, float)) else tuple(extra_width)
    large[:, 3:6] += boxes3d.new_tensor(width)[None, :]
    return large


def import_reference(root):
    stubs = {
        "utils.common_utils": {"check_numpy_to_torch": _check_numpy_to_torch},
        "utils.box_utils": {"enlarge_box3d": _enlarge_box3d},
        "ops.roiaware_pool3d.roiaware_pool3d_cuda": {
            "forward": lambda *a: ref.roiaware_pool3d_forward(*_args(a)),
            "backward": lambda *a: ref.roiaware_pool3d_backward(*_args(a)),
            "points_in_boxes_cpu": lambda *a: ref.points_in_boxes_cpu(*_args(a))},
        "ops.roipoint_pool3d.roipoint_pool3d_cuda": {"forward": lambda *a: ref.roipoint_pool3d_forward(*_args(a))},
    }
    return load(root, "pcdet", ["ops.roiaware_pool3d.roiaware_pool3d_utils", "ops.roipoint_pool3d.roipoint_pool3d_utils"],
                stubs=stubs, real_paths=True)


def main():
    aware, point = import_reference(reference_root())
    t = torch.from_numpy
    a, b = gen.roiaware_inputs("exact"), gen.roipoint_inputs("exact")
    rng = np.random.default_rng(5)
    out = dict(rois=a["rois"], pts=a["pts"], feat=a["feat3"], xyz=b["xyz"], boxes=b["boxes"], pfeat=b["feat5"])
    cases = []
    for method, out_size, k_slots in [("max", (3, 4, 5), 4), ("avg", (3, 4, 5), 4), ("max", 12, 128), ("avg", 12, 128)]:
        tag = "%s_o%s_k%d" % (method, out_size if isinstance(out_size, int) else "".join(map(str, out_size)), k_slots)
        cases.append(tag)
        grid = (out_size,) * 3 if isinstance(out_size, int) else out_size
        # max: small integers, so every float32 sum of the backward is exact whatever its order
        grad = (rng.integers(-4, 5, (6,) + grid + (3,)) if method == "max" else rng.normal(size=(6,) + grid + (3,))).astype(F32)
        f = t(a["feat3"].copy()).requires_grad_(True)
        rois, pts = t(a["rois"]).requires_grad_(True), t(a["pts"]).requires_grad_(True)
        pooled = aware.RoIAwarePool3d(out_size, k_slots)(rois, pts, f, pool_method=method)
        pooled.backward(t(grad))
        assert rois.grad is None and pts.grad is None
        slots, argmax = pooled.grad_fn.roiaware_pool3d_for_backward[:2]
        out[tag + "_args"] = np.array(list(grid) + [k_slots, 0 if method == "max" else 1], I32)
        out[tag + "_out"], out[tag + "_grad_out"], out[tag + "_grad_in"] = pooled.detach().numpy(), grad, f.grad.numpy()
        out[tag + "_slots"], out[tag + "_argmax"] = slots.numpy(), argmax.numpy()
        print(tag, "points kept", int(slots.numpy()[..., 0].sum()), "non-empty voxels", int((slots.numpy()[..., 0] > 0).sum()))
    out["aware_cases"] = np.array(cases)
    cases = []
    for n_sample, width in [(16, 1.0), (512, 0.0)]:
        tag = "s%d_w%d" % (n_sample, int(width))
        cases.append(tag)
        rows, flag = point.RoIPointPool3d(n_sample, width)(t(b["xyz"]), t(b["feat5"]), t(b["boxes"]))
        out[tag + "_args"] = np.array([n_sample, width], np.float64)
        out[tag + "_rows"], out[tag + "_flag"] = rows.numpy(), flag.numpy()
        print(tag, "empty boxes", flag.numpy().tolist())
    out["point_cases"] = np.array(cases)
    mask = aware.points_in_boxes_cpu(a["pts"], a["rois"])
    assert isinstance(mask, np.ndarray) and mask.shape == (6, gen.P)
    out["mask"] = mask
    path = os.path.join(HERE, "roi_pool.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
